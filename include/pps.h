/*
 * pps.h -- C-ABI of the MI355X-native plane-SLAM backend (libpps.so).
 *
 * One opaque handle `pps_graph` replaces, wholesale, the three seams the
 * reference exposes for this path (paths relative to
 * /root/reference/pop_planar_slam):
 *   - isam::Slam public API            Thirdparty/isam/include/isam/Slam.h:82-215
 *   - isam::OptimizationInterface      Thirdparty/isam/include/isam/OptimizationInterface.h:224-245
 *   - isam::Cholesky (solver plugin)   Thirdparty/isam/include/isam/Cholesky.h:148-178
 * plus the popup_plane statics the mapper calls
 *   - update_plane_equation_from_seg   /root/reference/pop_up_wall/include/pop_up_wall/popup_plane.h:137-139
 *   - generate_cloud / get_depth_map_good  popup_plane.h:142-143,155-157
 *
 * Everything is plain pointers and sizes; no C++/torch types.  All functions
 * return a status (PPS_OK == 0) and never exit()/abort() (the reference's
 * require() does: Thirdparty/isam/include/isam/util.h:174-184).
 *
 * Conventions
 *   quaternion  (x,y,z,w)                      -- Eigen coeffs() order
 *   pose        (tx,ty,tz,qx,qy,qz,qw)         -- isam::Pose3d (Pose3d.h:70-274)
 *   plane       unit 4-vector (a,b,c,d)        -- isam::Plane3d (src/isam_plane3d.h:27-193)
 *   meas6       (x,y,z,yaw,pitch,roll)         -- Pose3d::vector() (Pose3d.h:138-145)
 *   sqrtinf_ut  packed upper triangle, row-major (Factor.h:169-190): 21 (6x6) / 6 (3x3)
 *   ids         handle-local integers starting at 0 (the reference uses
 *               process-global counters, Slam.cpp:47-48)
 *
 * Threading: one handle = one device + one HIP stream; distinct handles may be
 * driven from distinct host threads.  No global mutable state.
 */
#ifndef PPS_H
#define PPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPS_VERSION 305   /* round.minor: bump whenever a struct of this header changes layout or an entry point is added (pps_stats grew in 200; pps_debug_front_factor: 301;
                              pps_multi_save_state / pps_multi_restore_state: 302; pps_debug_exmap AND pps_multi_phase_times' counts[] grown from 2 to 4
                              entries -- a caller built against 302 that passes counts[2] must be rebuilt: 303; pps_popup_run_async / _planes_wait / _wait: 304;
                              pps_debug_solve: 305) */

typedef struct pps_graph pps_graph;

enum pps_status {
  PPS_OK = 0,
  PPS_EINVAL = 1,     /* bad argument / unknown id                                   */
  PPS_ENOTPD = 2,     /* normal equations not positive definite (silent in CHOLMOD)  */
  PPS_EHIP = 3,       /* HIP runtime error (no device, OOM, launch failure)          */
  PPS_ENOMEM = 4,
  PPS_ESTATE = 5      /* operation not valid in the current state                    */
};

/* Jacobian evaluation mode of the per-edge sweep */
enum pps_jacobian_mode {
  PPS_JAC_NUMERIC = 0,   /* central differences, eps = 1e-4, through exmap: numericalDiff.cpp:32-87 (reference behaviour) */
  PPS_JAC_ANALYTIC = 1   /* closed-form derivative of the same residuals */
};

/* Mirrors isam::Properties (Properties.h:37-110); defaults = the app's values (Mapping.cpp:32-43). */
typedef struct pps_props {
  double epsilon2;          /* 1e-3 : stop when ||delta|| <= epsilon2                  */
  double epsilon_abs;       /* 1e-4 : stop when chi2 <= epsilon_abs                    */
  double epsilon_rel;       /* 1e-6 : stop when improvement < epsilon_rel * chi2       */
  int    max_iterations;    /* 500                                                      */
  double lm_lambda0;        /* 1e-6                                                     */
  double lm_lambda_factor;  /* 10                                                       */
  int    jacobian_mode;     /* enum pps_jacobian_mode, default PPS_JAC_NUMERIC          */
  int    device;            /* HIP device ordinal, default 0                            */
  int    verbose;           /* 0 = quiet (prop.quiet = true, Mapping.cpp:35)            */
} pps_props;

void pps_default_props(pps_props* p);
int  pps_version(void);
const char* pps_last_error(const pps_graph* g);      /* thread-compatible, handle-local */

/* ---- lifetime ------------------------------------------------------------------------ */
int pps_graph_create(const pps_props* props, pps_graph** out);   /* isam::Slam::Slam, Slam.cpp:69-78 */
int pps_graph_destroy(pps_graph* g);
int pps_get_props(const pps_graph* g, pps_props* out);           /* Slam::properties()     */
int pps_set_props(pps_graph* g, const pps_props* p);             /* Slam::set_properties() */

/* ---- nodes: Slam::add_node (Slam.cpp:91-94) + NodeT::init (Node.h:121-124) ------------ */
int pps_add_pose(pps_graph* g, const double tq[7], int* id);
int pps_add_plane(pps_graph* g, const double abcd[4], int* id);  /* normalised like Plane3d(Vector4d), isam_plane3d.h:59-66 */

/* ---- factors: Slam::add_factor (Slam.cpp:96-105) -------------------------------------- */
/* Pose3d_Factor            slam3d.h:58-89   */
int pps_add_pose_prior(pps_graph* g, int pose, const double meas6[6], const double sqrtinf_ut[21], int* fid);
/* Pose3d_Pose3d_Factor     slam3d.h:91-193  */
int pps_add_odometry(pps_graph* g, int pose1, int pose2, const double meas6[6], const double sqrtinf_ut[21], int* fid);
/* Pose3d_Plane3d_Factor    src/isam_plane3d.h:221-308 (relative = false, Mapping.cpp:21,513) */
int pps_add_plane_obs(pps_graph* g, int pose, int plane, const double meas4[4], const double sqrtinf_ut[6], int* fid);
/* Plane3d_Factor           src/isam_plane3d.h:428-474 */
/* Pose3d_Plane3d_Factor2 (src/isam_plane3d.h:314-424; the mapper's disabled call Mapping.cpp:515-521): a plane
 * observation whose measured plane is re-popped from the 2-D ground edge at every residual evaluation
 * (isam::get_wall_plane_equation, src/isam_plane3d.cpp:20-55, fp64) instead of being stored.  ray6 = the
 * 3x2 ground_edge_ray (column-major: ray of end point 0, ray of end point 1) from pps_edge_ray.  meas4 is
 * kept like FactorT::_measure but does not enter the error.  Its Jacobian is taken by central differences in
 * both jacobian modes (the pose perturbation moves the measurement).  Not for the ground plane. */
int pps_add_plane_obs2(pps_graph* g, int pose_id, int plane_id, const double meas4[4], const double ray6[6],
                       const double sqrtinf_ut[6], int* fid);
/* Pose3d_Plane3d_Factor2::precompute_edge_ray (src/isam_plane3d.h:361-373): fp32 invK * (u,v,1), cast to fp64 */
int pps_edge_ray(const float invK[9], const float seg2d[4], double ray6[6]);
int pps_add_plane_prior(pps_graph* g, int plane, const double meas4[4], const double sqrtinf_ut[6], int* fid);

/* FactorT::set_measurement (Factor.h:206) for plane factors; batched form for
 * Mapper_mono::update_plane_measurement (Mapping.cpp:590-607) */
int pps_set_measurement(pps_graph* g, int fid, const double meas4[4]);
int pps_set_measurements(pps_graph* g, int n, const int* fids, const double* meas4 /* n x 4 */);

/* Slam::remove_factor / remove_node (Slam.cpp:107-126); removing a node removes its factors */
int pps_remove_factor(pps_graph* g, int fid);
int pps_remove_node(pps_graph* g, int nid);

/* ---- solve ---------------------------------------------------------------------------- */
/* Slam::update with mod_batch = 1 (Slam.cpp:157-175 -> Optimizer::relinearize, Optimizer.cpp:114-185):
 * relinearise at the estimate, one Gauss-Newton step (lambda = 0). */
int pps_update(pps_graph* g);
/* Slam::batch_optimization (Slam.cpp:198-210) -> Optimizer::levenberg_marquardt (Optimizer.cpp:371-467) */
int pps_batch_optimize(pps_graph* g, int* iterations);
/* Slam::chi2(ESTIMATE) (Slam.cpp:266-268) */
int pps_chi2(pps_graph* g, double* chi2);

/* ---- marginal covariances: Slam::covariances() -> isam::Covariances (Covariances.h:42-110, isamlib/covariance.cpp) ----------
 * Sigma = (J'J)^-1 at the ESTIMATE, in tangent coordinates: a pose block is 6 x 6 over (dx, dy, dz, rotx, roty, rotz), a plane block 3 x 3
 * over the 3-vector of Plane3d::exmap_3dof -- the column order of pps_eval_factor.  The factor never leaves the device; the entries
 * of Sigma inside its sparsity pattern are recovered from it front by front, root -> leaves (selected inverse), without a dense inverse.
 * That pattern holds the diagonal block of EVERY node and the cross block of every pair of nodes that share a front of the
 * elimination tree: every pair joined by a factor (pose - plane observations, consecutive poses) and the fill between them.
 *
 * pps_cov_recover: relinearise at the estimate in the handle's jacobian_mode, factor H = J'J with lambda = 0 (the system of pps_update,
 * without applying a step), then the recursion.  The estimate, the linearisation point, the LM trace and the stats of the last solve stay
 * as they were; a pps_batch_optimize after it gives the trace it would have given without it.  Results stay on the device until read.
 *   PPS_ENOTPD  H is not positive definite: a pivot of the factor was not positive, or smaller than 1e-7 of the largest pivot of its
 *               front (H singular to working precision, e.g. a graph without any prior: its "covariance" would be rounding noise)
 *   PPS_ESTATE  the graph has fronts beyond the wave-per-front kernels (loop-closure graphs in the dense-front form: sphere2500, graphs
 *               after a landmark merge across the map -- what pps_multi_create refuses, too).  Not supported; the handle stays usable.
 * Validity: a recovery ends with every call that changes the estimate, the measurements or the topology -- any pps_add_*, pps_remove_*,
 * pps_set_* (pps_set_props: when it changes jacobian_mode), pps_update, pps_batch_optimize, pps_restore_state, pps_refresh_measurements,
 * membership in a pps_multi_optimize / pps_multi_restore_state.  The read calls then return PPS_ESTATE ("no valid recovery"): never stale
 * numbers, never a silent recomputation.  Ids are checked first (PPS_EINVAL), on the host, before anything is launched.
 * Pairs OUTSIDE the pattern (e.g. the newest pose against a plane it has not observed) are not available from these three read calls,
 * which report them; pps_cov_block below answers for any nodes, by column solves on the same factor.
 * PPS_VERSION was not bumped for them (it stayed 304): a caller detects these entry points by symbol lookup (dlsym "pps_cov_recover"). */
int pps_cov_recover(pps_graph* g);
/* diagonal blocks: ids[n] node ids (NULL = all live nodes in insertion order, n = their number); out = concatenated row-major blocks,
 * 36 doubles per pose, 9 per plane; offsets[n + 1] (may be NULL) = start of each block in out.  Every block is exactly symmetric. */
int pps_cov_marginals(pps_graph* g, int n, const int* ids, double* out, int64_t* offsets);
/* cross blocks Sigma(rows[i], cols[i]), row-major dim(rows[i]) x dim(cols[i]), block i at out + offsets[i] (blocks are laid out back to
 * back whether written or not; offsets[n + 1] may be NULL); in_pattern[i] = 1 if the pair lies in the factor's pattern (the block is
 * written), 0 otherwise (the block is left untouched, the call still returns PPS_OK) */
int pps_cov_access(pps_graph* g, int n, const int* rows, const int* cols, double* out, int64_t* offsets, int* in_pattern);
/* joint marginal over a list of distinct nodes (Covariances::marginal(list)): (sum of dims)^2 doubles, row-major, nodes in list order;
 * PPS_ESTATE, naming the first pair, when two of them lie outside the pattern */
int pps_cov_joint(pps_graph* g, int n, const int* ids, double* out);
/* device seconds (HIP events) of the last pps_cov_recover: sec[0] the whole call's launches, sec[1] the root -> leaves pass alone */
int pps_cov_last_times(const pps_graph* g, double sec[2]);
/* pps_cov_factor: the factor-only recovery -- all that pps_cov_block and pps_assoc_gate read, and the one recovery a dense-front graph
 * (loop closures: sphere2500, a landmark merge across the map) has.  Relinearises at the estimate in the handle's jacobian_mode (the
 * robustified error with a cost function set), assembles H = J'J and factors it with lambda = 0 in the form the graph is solved in: the
 * band stages of pps_cov_recover without its root -> leaves pass (about two thirds of that call's work, whose results a block or gate
 * query never reads), or the dense-front levels of pps_batch_optimize without the back-substitution.  Like pps_cov_recover it moves
 * neither the estimate, the linearisation point, the LM trace nor the stats of the last solve; a pps_batch_optimize after it is bit for
 * bit the one without it.
 *   PPS_EINVAL  NULL handle
 *   PPS_ESTATE  empty graph; or (a text of its own) a graph solved by the one-launch-per-level LDS kernels, neither band nor dense-front
 *   PPS_ENOTPD  no factor in the graph; a pivot of the factorisation was not positive; or a pivot of L_A was not positive, not finite, or
 *               below 1e-7 of the largest pivot of its front -- the criterion of pps_cov_recover, applied by one launch over all fronts.
 *               No valid factor is left behind; the handle stays usable.
 *   PPS_EHIP    no device, or a HIP error (the handle's device copy is abandoned, as by pps_cov_recover)
 * Validity: the handle keeps two flags, "selected inverse" and "factor".  pps_cov_recover sets both, pps_cov_factor the second alone; every
 * call listed above as ending a recovery clears both, and so does the start of either entry point (a pps_cov_recover that is refused
 * -- dense-front graph -- ends the factor of an earlier pps_cov_factor: call pps_cov_factor after it, not before).
 *   pps_cov_block, pps_assoc_gate (and their _last / debug companions) ask for the factor: either entry point provides it.
 *   pps_cov_marginals / _access / _joint ask for the selected inverse; after a pps_cov_factor alone they answer PPS_ESTATE with a text that
 *   names pps_cov_factor and pps_cov_recover.  With neither call made every read call answers PPS_ESTATE "no valid covariance recovery".
 * On a dense-front graph the root-path walks run in a second kernel (one workgroup of 256 threads per node, the right-hand sides in a
 * scratch buffer of the handle sized by the widest front on the paths of the query; PPS_ENOMEM from pps_cov_block / pps_assoc_gate if
 * it cannot be allocated); on a band graph both kernels write the same bits.  Not offered on such graphs: the selected inverse, pps_multi.
 * pps_cov_last_times reports the call in sec[0], with sec[1] = 0.
 * Found by symbol lookup (dlsym "pps_cov_factor"), like the calls above; PPS_VERSION was not bumped. */
int pps_cov_factor(pps_graph* g);
/* diagnostics, per handle: which kernel walks the root paths of pps_cov_block / pps_assoc_gate.  form 0 = automatic (the wave-per-node
 * kernel where its LDS fits the graph's fronts, the wide kernel otherwise), 1 = always the wide kernel -- to compare the two on any band
 * graph.  PPS_EINVAL: NULL handle, another form.  Changes no validity.  Found by symbol lookup. */
int pps_debug_cov_path_form(pps_graph* g, int form);
/* pps_cov_select: the selected inverse in whatever K3 form the graph is solved in -- what pps_cov_recover computes, on loop-closure graphs too.
 *   band graph         exactly pps_cov_recover: the same launches, the same bits, both validity flags.
 *   dense-front graph  the factor stage of pps_cov_factor, then one root -> leaves pass over the dense fronts (pps_cov_dense.hip: G = L_B L_A^-1
 *                      and L_A^-T L_A^-1 of all fronts in one launch, then per tree level a gather of Sigma_BB through the child map and the two
 *                      products on the matrix cores: 1 + 3 x levels launches).  Afterwards pps_cov_marginals / _access / _joint answer as on a band
 *                      graph (every node's diagonal block, every pair that shares a front), pps_cov_block and pps_assoc_gate as after pps_cov_factor.
 *   neither form       PPS_ESTATE with the text of pps_cov_factor (the one-launch-per-level LDS kernels keep no factor).
 * Validity, invalidation and PPS_ENOTPD are those of pps_cov_recover: the call starts by clearing both flags, sets both when it succeeds, and every
 * call that ends a recovery ends this one.  A later pps_cov_factor keeps the factor alone (the read calls then name both entry points), a later
 * pps_cov_recover on a dense-front graph is refused as always and ends the selection.  PPS_ENOMEM (never an abort): no device memory for the
 * selected inverse or for the scratch of the pass (two arrays of the factor's size).  The estimate, the linearisation point, the LM trace and the
 * stats stay untouched.  pps_cov_last_times: sec[0] the whole call, sec[1] the root -> leaves pass.
 * Found by symbol lookup (dlsym "pps_cov_select"), like the calls above; PPS_VERSION was not bumped. */
int pps_cov_select(pps_graph* g);
/* diagnostics, per handle: form 1 = pps_cov_select takes the dense-front pass on a band graph too (its factor sits in the same layout), so that
 * fronts whose shapes are no multiples of 4, 16 or 64 pass through the tiled kernels and can be compared with pps_cov_recover; 0 = as above.
 * PPS_EINVAL: NULL handle, another form.  Changes no validity.  Found by symbol lookup. */
int pps_debug_cov_select_form(pps_graph* g, int form);
/* Sigma(rows, cols) for ANY nodes, inside the pattern of the factor or not (the reference's marginal(node_list) / access(pairs) without
 * the limit above): out is (sum dim(rows)) x (sum dim(cols)), row-major, nodes in the order given.  cols == NULL (nc ignored): cols =
 * rows, the joint marginal, exactly symmetric.  A node may appear in both lists, not twice in one.
 * With H = L L' and E_S the unit columns of a node set S, Sigma(R, C) = (L^-1 E_R)' (L^-1 E_C): each distinct node costs one forward
 * solve along its path from its front to the root of the elimination tree (its columns of L^-1 are zero elsewhere), the block one
 * product over the pivots of common ancestors.  Cost: about (pivots on the path) x (front rows) x dim(node) multiply-adds per node, all
 * nodes side by side; one upload, two launches and one copy per call, whatever nr, nc and the depth of the tree.  Nothing is factored
 * again: the call reads the factor of the last pps_cov_recover or pps_cov_factor and falls under the same validity rules.
 *   PPS_EINVAL  NULL handle, rows or out; a negative count; an unknown or removed node id; a node twice in rows or twice in cols
 *   PPS_ESTATE  no valid factor (a dense-front graph has one after pps_cov_factor; pps_cov_recover has none to give there)
 *   PPS_ENOMEM  dense-front graphs: no device memory for the right-hand sides of the walks; any graph: no host memory for the request or
 *               the result (never an abort)
 *   PPS_OK      with out untouched for nr == 0 or nc == 0
 * pps_cov_marginals / _access / _joint keep their in-pattern contract and their refusals.  Found by symbol lookup, like the calls above. */
int pps_cov_block(pps_graph* g, int nr, const int* rows, int nc, const int* cols, double* out);
/* the last pps_cov_block: device seconds (HIP events) around its two kernels, and the number of kernel launches it made (either may be NULL) */
int pps_cov_block_last(const pps_graph* g, double* kernel_sec, int* launches);

/* ---- Mahalanobis gate of plane association, from the recovered covariances -------------------------------------
 * What isam::Covariances is for in a SLAM front end: a candidate pairing of a measurement with a landmark is accepted when its innovation
 * is small against the innovation covariance.  For pose node pose_id, candidate landmark l, measurement m (a plane 4-vector in the sensor
 * frame, normalised on entry like Plane3d(Vector4d)) and its packed upper-triangular sqrt information W (6 doubles, as in
 * pps_add_plane_obs): with r (3) and Jw (3 x 9, over pose 6 | plane 3) the whitened residual and Jacobian a
 * Pose3d_Plane3d_Factor(pose, l, m, W) would have at the current ESTIMATE -- Jw in the handle's jacobian_mode, the linearisation of
 * pps_cov_recover -- and Sigma (9 x 9) the joint marginal of (pose, l) from the current recovery,
 *     S = I + Jw Sigma Jw'     d2 = r' S^-1 r      (S^-1 r by a 3 x 3 Cholesky solve)
 * d2 is chi-square distributed with 3 degrees of freedom for a correct pairing: 7.815 is the usual (0.95) threshold.
 * d2 is n_meas x n_planes, row-major; best[i] (best may be NULL) = the index INTO plane_ids of the smallest finite d2 of measurement i,
 * the first candidate on ties, -1 if no d2 of the row is finite.  plane_ids == NULL (n_planes ignored): all live planes in insertion order.
 * Everything is computed on the device: one upload, two launches (the root-path walks of pps_cov_block for the 1 + n_planes nodes, the
 * gate), one copy; no covariance block is downloaded and Sigma is never formed.  The candidate factors are not added to the graph: the
 * estimate, the linearisation point, the LM trace, the stats and the recovery stay untouched.  A candidate's d2 does not depend on which
 * other candidates or measurements are in the call.  In JAC_NUMERIC r and Jw are pps_eval_factor's bit for bit (the lane form of K1).
 *   PPS_EINVAL  NULL handle, meas4, sqrtinf_ut or d2; a negative count; n_meas above 65535 (the grid's second dimension); a non-finite
 *               input; an unknown or removed id; pose_id is not a
 *               pose; a plane_ids entry is not a plane; a plane twice in the list (all checked on the host before anything is launched)
 *   PPS_OK      with the outputs untouched for n_meas == 0 or n_planes == 0 -- answered after the argument checks and BEFORE the recovery
 *               is looked at (nothing is read from it), unlike pps_cov_block, which asks for the recovery first
 *   PPS_ESTATE  no valid factor: the text and the validity rules of pps_cov_block (a dense-front graph: after pps_cov_factor)
 *   PPS_ENOTPD  a pivot of a 3 x 3 factor was not positive or not finite (the outputs are untouched)
 *   PPS_ENOMEM  as pps_cov_block: the right-hand sides of the walks on the device, the request or the result on the host
 * Mapper_mono::findClosestPlane's geometric gate (pps_find_closest_planes) is independent of this call and unchanged.
 * Found by symbol lookup, like the pps_cov_* calls; PPS_VERSION was not bumped. */
int pps_assoc_gate(pps_graph* g, int pose_id, int n_meas, const double* meas4, const double* sqrtinf_ut, int n_planes, const int* plane_ids,
                   double* d2, int* best);
/* the last pps_assoc_gate: device seconds (HIP events) around its two kernels, and the number of kernel launches it made (either may be NULL) */
int pps_assoc_gate_last(const pps_graph* g, double* kernel_sec, int* launches);
/* diagnostics: r and Jw of every candidate of the last successful pps_assoc_gate, as the gate kernel evaluated them: n_meas x n_planes
 * records of 30 doubles [Jp 3 x 6 | Jl 3 x 3 | r 3], row-major, candidate (i, j) at (i * n_planes + j) * 30 -- the layout of K1's record
 * of a plane observation, so that a test can compare them with pps_eval_factor bit for bit.  *needed = the number of doubles; nothing is
 * copied when rec is NULL or cap is smaller.  PPS_ESTATE before the first successful gate call of the handle. */
int pps_debug_assoc_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed);

/* ---- Mahalanobis merge gate between plane landmarks, from the recovered covariances ---------------------------
 * pps_assoc_gate asks "does this measurement belong to that landmark"; this call asks what a map needs after a revisit: "are these two
 * landmarks the same wall" -- the decision of Mapper_mono::findLoopPlane (Mapping.cpp:174-252), made there by the 2-D image distance of
 * end points against frame 0.  For two distinct live plane nodes a, b, a the one that comes FIRST in the list, in the tangent coordinates
 * of Plane3d::exmap_3dof (the column order of pps_eval_factor):
 *     e   = r(a | pi_b)     residual of a Plane3d_Factor on node a with measurement pi_b (b's estimate) and identity sqrt information
 *     J_a = its 3 x 3 Jacobian by central differences (eps = 1e-4, the device's step quaternions): pps_eval_factor's bits for such a
 *           factor in PPS_JAC_NUMERIC
 *     J_b = -J(b | pi_a)    the NEGATED Jacobian of the mirrored factor (node b, measurement pi_a), the same differences
 *     S   = J_a Sigma_aa J_a' + J_b Sigma_bb J_b' + J_a Sigma_ab J_b' + J_b Sigma_ba J_a' + floor_var I
 *     d2  = e' S^-1 e       (3 x 3 Cholesky solve); chi-square with 3 degrees of freedom for one wall: 7.815 is the usual (0.95) threshold
 * The Jacobians are ALWAYS central differences, whatever the handle's jacobian_mode; Sigma is whatever linearisation the recovery used
 * (jacobian_mode, and the robustified system with a cost function set -- e and the Jacobians are never robustified: the call is not
 * refused with a cost function, unlike pps_assoc_gate).  floor_var >= 0 (rad^2, 0 allowed) stands for plane error the graph does not
 * model and keeps S positive definite for perfectly correlated pairs.
 *   plane_ids  n_planes node ids; NULL (n_planes ignored): all live planes in insertion order
 *   d2         (may be NULL) n x n, row-major, diagonal 0, EXACTLY symmetric: a pair is computed once, for the list order i < j, and
 *              mirrored.  When NULL nothing n x n is copied to the host.
 *   best       (may be NULL) n: per row the index INTO plane_ids of the smallest finite off-diagonal d2, the first on ties, -1 if none
 *   pairs, n_pairs  (may be NULL together) all index pairs (i < j) with finite d2 < threshold, ascending by (i, j), 2 ints each; at most
 *              cap_pairs are written, *n_pairs is always the full count (pairs may be NULL with cap_pairs == 0: the count alone)
 * A pair whose S is NOT positive definite (a pivot of its 3 x 3 factor not positive or not finite) gets d2 = NaN, is never `best` and
 * never in `pairs`, and the call still returns PPS_OK; pps_merge_gate_last reports how many there were.  This differs from pps_assoc_gate
 * (PPS_ENOTPD) on purpose: one degenerate pair among n^2 / 2 must not void the query.
 * Everything is computed on the device: one upload, two launches (the root-path walks of pps_cov_block for the n planes, ONE pair
 * kernel: a wave per pair, the common ancestors of a pair found on the device from the tree), one copy.  A pair's d2 does not depend on
 * which other planes are in the call as long as the pair keeps its order.  The estimate, the linearisation point, the LM trace, the
 * stats and the recovery stay untouched: a pps_batch_optimize after the call is bit for bit the one without it.
 *   PPS_EINVAL  (checked on the host before any launch) NULL handle; a negative count; more than 65535 planes; floor_var not finite or
 *               negative; threshold not finite; an unknown, removed or non-plane id; an id listed twice; d2, best and pairs / n_pairs all
 *               NULL; pairs without n_pairs, or n_pairs without pairs and cap_pairs > 0
 *   PPS_OK      with the outputs untouched for fewer than 2 planes -- answered before the recovery is looked at
 *   PPS_ESTATE  no valid factor: the text and the validity rules of pps_cov_block (either recovery provides the factor; a dense-front
 *               graph has it after pps_cov_factor)
 *   PPS_ENOMEM  the strips, the walk scratch or the n x n result cannot be allocated
 * Found by symbol lookup, like the pps_cov_* calls; PPS_VERSION was not bumped. */
int pps_merge_gate(pps_graph* g, int n_planes, const int* plane_ids, double floor_var, double threshold, double* d2, int* best, int cap_pairs,
                   int* pairs, int* n_pairs);
/* the last pps_merge_gate: device seconds (HIP events) around its two kernels, the kernel launches it made, and the number of its pairs
 * whose S was not positive definite (each may be NULL) */
int pps_merge_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd);
/* diagnostics: J_a, J_b and e of every pair of the last successful pps_merge_gate, as the pair kernel evaluated them: 21 doubles per pair
 * [J_a 3 x 3 | J_b 3 x 3 | e 3], row-major, pair (i < j) at index i * n - i (i + 1) / 2 + (j - i - 1), so that a test can compare them
 * with pps_eval_factor bit for bit.  *needed = the number of doubles; nothing is copied when rec is NULL or cap is smaller.  PPS_ESTATE
 * before the first successful call of the handle, and after a call of more than 262144 pairs (the records of such a call are not kept). */
int pps_debug_merge_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed);

/* ---- Mahalanobis gate for loop-closure pose candidates, from the recovered covariances -------------------------
 * The question the pose-graph side asks before it adds a loop closure: "is this relative-pose measurement between two existing poses
 * consistent with the current estimate?" (the reference leaves it open: Mapping.cpp:658 always associates to the first frame).  Candidate k
 * is the factor Pose3d_Pose3d_Factor(pose_a[k], pose_b[k], meas6[k], W_k) that pps_add_odometry would add; at the current ESTIMATE, in the
 * handle's jacobian_mode and the column order of pps_eval_factor (columns of a, then of b):
 *     r (6), Jw (6 x 12)   its whitened residual and Jacobian; the measurement is used as pps_add_odometry stores it (the six numbers as given)
 *     Sigma (12 x 12)      the joint marginal of (a, b) from the current factor
 *     S   = I + Jw Sigma Jw'
 *     d2  = r' S^-1 r      (6 x 6 Cholesky solve); chi-square with 6 degrees of freedom for a correct closure: 12.592 is the 0.95 threshold
 * Sigma is never formed and no covariance block goes to the host.
 *   pose_a, pose_b  n node ids each; a pose may appear in any number of candidates and a pair may appear twice: every entry is answered on
 *              its own, and its d2 and S are bit for bit independent of what else is in the call
 *   meas6      n x 6 (x y z yaw pitch roll, as pps_add_odometry takes it);  sqrtinf_ut  n x 21, the packed upper triangle
 *   d2         (may be NULL) n
 *   S          (may be NULL) n x 36, row-major, EXACTLY symmetric: computed as the lower triangle and mirrored.  When NULL nothing n x 36
 *              is copied to the host.
 *   accepted, n_accepted  (may be NULL together) the indices INTO the list, ascending, of the entries with finite d2 < threshold; at most
 *              cap_accepted are written, *n_accepted is always the full count (accepted may be NULL with cap_accepted == 0: the count alone)
 * A candidate whose S is NOT positive definite (a pivot of its 6 x 6 factor not positive or not finite) gets d2 = NaN, is never accepted,
 * and the call still returns PPS_OK; pps_loop_gate_last reports how many there were (the rule of pps_merge_gate: one bad candidate must not
 * void the list).  Its S is still written, as computed.
 * Everything is computed on the device: one upload, two launches (the root-path walks of pps_cov_block for the DISTINCT poses of the
 * list, ONE candidate kernel: a wave per candidate, the common ancestors of its two poses found on the device from the tree), one copy.
 * Nothing is added to the graph: the estimate, the linearisation point, the LM trace, the stats, both validity flags and the recovery stay
 * untouched, and a pps_batch_optimize after the call is bit for bit the one without it.
 *   PPS_EINVAL  (checked on the host before any launch, without a device) NULL handle or a NULL input array; negative n or cap_accepted;
 *               d2, S and accepted / n_accepted all NULL; accepted without n_accepted, or n_accepted without accepted and
 *               cap_accepted > 0; a threshold that is not finite while n_accepted is given; a non-finite measurement or weight; an
 *               unknown, removed or non-pose id; pose_a[k] == pose_b[k]
 *   PPS_OK      with the outputs untouched for n == 0 -- answered before the recovery is looked at
 *   PPS_ESTATE  a robust cost function is set (the rule of pps_assoc_gate: a candidate measurement against a Gaussian innovation);
 *               no valid factor: the text and the validity rules of pps_cov_block (either recovery provides the factor; a dense-front
 *               graph has it after pps_cov_factor alone)
 *   PPS_ENOMEM  a buffer of the call cannot be had
 * Found by symbol lookup, like the pps_cov_* calls; PPS_VERSION was not bumped. */
int pps_loop_gate(pps_graph* g, int n, const int* pose_a, const int* pose_b, const double* meas6 /* n x 6 */,
                  const double* sqrtinf_ut /* n x 21 */, double threshold, double* d2 /* n */, double* S /* n x 36, may be NULL */,
                  int cap_accepted, int* accepted, int* n_accepted);
/* the last pps_loop_gate: device seconds (HIP events) around its two kernels, the kernel launches it made (2), and the number of its
 * candidates whose S was not positive definite (each may be NULL) */
int pps_loop_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd);
/* diagnostics: Jw and r of every candidate of the last successful pps_loop_gate, as the kernel evaluated them: one slot of 78 doubles per
 * entry, [Jw 6 x 12 row-major | r 6] -- the slot of pps_debug_factor_gate_records for an odometry factor --, so that a test can compare
 * them with pps_eval_factor.  *needed = the number of doubles; nothing is copied when rec is NULL or cap is smaller.  PPS_ESTATE before
 * the first successful call of the handle, and after a call of more than 65536 entries (the records of such a call are not kept). */
int pps_debug_loop_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed);

/* ---- leave-one-out chi-square test of every factor, from the recovered covariances ----------------------------
 * pps_assoc_gate and pps_merge_gate judge candidates; this call asks what a front end asks after a solve: "which factor already in the
 * graph is wrong?" (plane association is greedy and geometric, and one wrong pps_add_plane_obs bends the corridor).  For factor f, at
 * the current ESTIMATE and in the handle's jacobian_mode, with r (m = 3 or 6) and J (m x c, c = 3, 6, 9 or 12 over its one or two nodes)
 * the whitened residual and Jacobian in the column order of pps_eval_factor, and Sigma_ff (c x c) the joint marginal of its nodes from
 * the current selected inverse (every pair joined by a factor lies in its pattern):
 *     P   = J Sigma_ff J'       the factor's block of the hat matrix, eigenvalues in [0, 1]
 *     lev = trace(P)            how much of its own m rows the factor determines (m - lev: its redundancy); the sum over all factors
 *                               is the state dimension
 *     d2  = r' (I - P)^-1 r     (m x m Cholesky solve)
 * At a converged estimate d2 is the squared Mahalanobis distance of the factor's residual at the solution of the graph WITHOUT this factor,
 * against that graph's innovation covariance (Woodbury: I + J Sigma_- J' = (I - P)^-1, r_- = (I - P)^-1 r): chi-square with m degrees of
 * freedom for a correct factor, 7.815 (m = 3) and 12.592 (m = 6) at 0.95.  A factor that is the only constraint on some direction (the
 * gauge prior, the single observation of a plane) has a singular I - P: when a pivot of the Cholesky factor, taken before its square root,
 * is not finite or <= 1e-7 (the pivot criterion of the recovery on a matrix of scale 1), d2 = NaN -- "untestable" --, the leverage is
 * still written, the entry is never flagged and the call still returns PPS_OK, as pps_merge_gate treats a degenerate pair;
 * pps_factor_gate_last reports how many there were.
 *   fids       n factor ids; NULL (n ignored): all live factors in insertion order.  A fid may appear more than once; each entry is
 *              answered on its own, and its d2 and leverage do not depend on what else is in the list (the same bits)
 *   d2, leverage   (either may be NULL) n each
 *   flagged, n_flagged  (may be NULL together) the indices INTO the list, ascending, of the entries whose finite d2 exceeds thr3 (m = 3)
 *              or thr6 (m = 6); at most cap_flagged are written, *n_flagged is always the full count (flagged may be NULL with
 *              cap_flagged == 0: the count alone)
 * Every factor type is answered; a pps_add_plane_obs2 factor has its J by central differences in both modes, as pps_eval_factor gives it.
 * In PPS_JAC_NUMERIC r and J are pps_eval_factor's lane form (compiled without contraction).  Everything is computed on the device: the
 * table that says where each factor's blocks sit in the selected inverse is built and uploaded once per analysis, a call uploads its fid
 * list, makes ONE launch (a wave per entry) and one copy; no covariance block is downloaded.  Nothing is added to the graph: the estimate,
 * the linearisation point, the LM trace, the stats, both validity flags and the recovery stay untouched, and a pps_batch_optimize after
 * the call is bit for bit the one without it.
 *   PPS_EINVAL  (checked on the host before any launch, without a device) NULL handle; negative n or cap_flagged; d2, leverage and
 *               flagged / n_flagged all NULL; flagged without n_flagged, or n_flagged without flagged and cap_flagged > 0; a threshold
 *               that is not finite while n_flagged is given; an unknown or removed fid
 *   PPS_ESTATE  a robust cost function is set (after the argument checks, without a device: the robustified statistic is not offered);
 *               no valid SELECTED INVERSE: the texts of pps_cov_marginals (pps_cov_recover or pps_cov_select provide it, so a
 *               dense-front graph is served after pps_cov_select; the factor of pps_cov_factor alone is not enough)
 *   PPS_OK      with the outputs untouched for n == 0 (or no live factor with fids NULL) -- answered before the recovery is looked at
 *   PPS_ENOMEM  a buffer of the call cannot be had
 * Found by symbol lookup, like the pps_cov_* calls; PPS_VERSION was not bumped. */
int pps_factor_gate(pps_graph* g, int n, const int* fids, double thr3, double thr6, double* d2, double* leverage, int cap_flagged, int* flagged,
                    int* n_flagged);
/* the last pps_factor_gate: device seconds (HIP events) around its kernel, the kernel launches it made (1), and the number of its
 * untestable entries (each may be NULL) */
int pps_factor_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_untestable);
/* diagnostics: J and r of every entry of the last successful pps_factor_gate, as the kernel evaluated them: one slot of 78 doubles per list
 * entry, [J m x c row-major, packed | r m], the rest of the slot unspecified, so that a test can compare them with pps_eval_factor.
 * *needed = the number of doubles; nothing is copied when rec is NULL or cap is smaller.  PPS_ESTATE before the first successful call of
 * the handle, and after a call of more than 65536 entries (the records of such a call are not kept). */
int pps_debug_factor_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed);

/* ---- robust cost functions: Slam::set_cost_function (Slam.h; Factor::error, Factor.h:67-77; isam/robust.h) ------
 * With a cost function set, every evaluation of a factor's error replaces each whitened component by
 *     r_i <- sign(r_i) sqrt(rho(r_i)),  sign(0) = +1
 * -- in all 2 n + 1 evaluations of the central differences (PPS_JAC_NUMERIC differentiates through rho), in weighted_errors and in
 * chi2 = sum rho(r_i).  PPS_JAC_ANALYTIC scales row i of the whitened J by phi'(r_i) = rho'(r_i) / (2 sqrt(rho(r_i))), at r_i = 0 by its limit.
 * LM itself does not change.  A function pointer cannot cross to the device: the cost is a kind and one parameter b.
 *   PPS_COST_HUBER         rho = d^2 for |d| < b, else 2 b |d| - b^2
 *   PPS_COST_PSEUDO_HUBER  rho = 2 b^2 (sqrt(1 + d^2 / b^2) - 1)            (iSAM's command line: -R)
 *   PPS_COST_CAUCHY        rho = log(pi / b) * log(1 + d^2 / b^2) -- a product of two logarithms, as the reference writes it (a quirk that
 *                          is kept); positive only for b < pi
 * Not offered (csrc/pps_cost.h gives the reasons): Blake-Zisserman (rho(0) < 0), corrupted Gaussian (rho(0) > 0), L1 (infinite slope at 0).
 * With a cost set, pps_batch_optimize, pps_update, pps_chi2, pps_eval_factor (the robustified r and J) and pps_cov_recover use the
 * robustified error, for every factor type (pps_add_plane_obs2 included), both Jacobian modes, band and dense-front graphs alike: K1 and
 * the chi2 sweeps run in kernels of their own (csrc/pps_robust.hip), everything behind them is unchanged.  pps_batch_optimize then takes
 * the one-step-at-a-time LM loop whatever PPS_NO_DUAL says.  PPS_COST_NONE returns the handle to exactly the launches it took before.
 *   PPS_EINVAL  NULL handle; unknown kind; b not finite or <= 0; PPS_COST_CAUCHY with b >= pi.  b is ignored for PPS_COST_NONE.
 * The call counts as a pps_set_*: a valid covariance recovery ends.  While a cost is set, pps_multi_create over the graph (and
 * pps_multi_optimize, if it was set later) and pps_assoc_gate return PPS_ESTATE with a text that names the cost function -- they have no
 * robustified form --; the handle stays usable.  pps_graph_save does not write the cost function and pps_graph_load starts with
 * PPS_COST_NONE (the reference's file format has no place for it: Slam::save writes nodes and factors).
 * Found by symbol lookup, like the pps_cov_* calls; PPS_VERSION was not bumped. */
enum pps_cost_kind { PPS_COST_NONE = 0, PPS_COST_HUBER = 1, PPS_COST_PSEUDO_HUBER = 2, PPS_COST_CAUCHY = 3 };
int pps_set_cost_function(pps_graph* g, int kind, double b);
int pps_get_cost_function(const pps_graph* g, int* kind, double* b);   /* PPS_COST_NONE reports b = 1 */

/* ---- many graphs side by side (BASELINE config 4 on one device; north_star reports graphs/sec) ----------------
 * One C2-size LM solve is a dependency chain that occupies a few dozen of the 256 CUs.  pps_multi runs
 * Optimizer::levenberg_marquardt (Optimizer.cpp:371-467) on n independent graphs in rounds: every kernel of an LM
 * trial is launched once for a chunk of up to 128 graphs, lambda / accept / reject stay per graph (host side, one 32-byte record per
 * graph and round).  While a chunk holds at most 120 000 factors, arithmetic, lambda schedule, iteration count and trace of every
 * graph are exactly -- bit for bit -- those of its own pps_batch_optimize.  A larger chunk takes the throughput forms (K1 as one
 * thread per factor without product records, K2 multiplying the Jacobian slices): the same sums in another rounding order, H and
 * chi2 equal to about 1e-12 relative, LM verdicts and iteration counts the same on every graph measured; which chunk a graph
 * lands in depends on the factor count of the whole batch, so below that level a graph's low-order bits can depend on what else
 * is in its batch (pps_multi_phase_times reports the forms taken).  The graphs keep belonging to the caller (same device; they must outlive the pps_multi and must
 * not be used from another thread during the call); topology edits between calls are picked up.  Graphs with
 * loop-closure fronts (dense-front kernels) are refused with PPS_ESTATE.
 *   iterations[n], status[n] (either may be NULL): LM iterations and PPS_OK / PPS_ENOTPD per graph. */
typedef struct pps_multi pps_multi;
int pps_multi_create(int n, pps_graph* const* graphs, pps_multi** out);
int pps_multi_destroy(pps_multi* m);
const char* pps_multi_last_error(const pps_multi* m);
int pps_multi_optimize(pps_multi* m, int* iterations, int* status);
int pps_multi_rounds(const pps_multi* m, int* rounds);    /* rounds of the last call (of the chunk of graphs that took most) = its longest LM run + 1 */
/* pps_save_state / pps_restore_state of every graph of the batch; the restore is ONE launch and complete on return (a benchmark
 * that solves the same graphs again from their initial estimates pays 30 us for it instead of a copy per handle) */
int pps_multi_save_state(pps_multi* m);
int pps_multi_restore_state(pps_multi* m);
/* level 1: HIP events at the phase boundaries of every round (no host syncs); after the next pps_multi_optimize
 * sec[5] = device seconds in K1 (Jacobian sweep) | K2 (H blocks) | K3 factor | K3 back-substitution | trial step + chi2,
 * counts[4] (may be NULL) = graphs re-linearised | factorised, summed over the rounds | chunks the batch of the last call was cut
 * into | forms its chunks took: bit 0 = thread-per-factor K1 + class-body K2 (throughput), bit 1 = one launch per tree level (K3);
 * the last two are valid without profiling */
int pps_multi_set_profiling(pps_multi* m, int level);
int pps_multi_phase_times(const pps_multi* m, double sec[5], long long counts[4]);

/* ---- state access (NodeT::value(), Node.h:130) ---------------------------------------- */
int pps_num_nodes(const pps_graph* g, int* n);
int pps_num_factors(const pps_graph* g, int* n);
int pps_get_pose(pps_graph* g, int id, double tq[7]);
int pps_get_plane(pps_graph* g, int id, double abcd[4]);
int pps_set_pose(pps_graph* g, int id, const double tq[7]);     /* NodeT::init on an existing node */
int pps_set_plane(pps_graph* g, int id, const double abcd[4]);
/* bulk: ids may be NULL (= all poses / all planes in insertion order); out is n x 7 / n x 4 */
int pps_get_poses(pps_graph* g, int n, const int* ids, double* out);
int pps_get_planes(pps_graph* g, int n, const int* ids, double* out);
/* Device-resident snapshot of the current estimate and its restore (bench / what-if solves):
 * the analogue of copying every NodeT::_value aside and back (Node.h:104-146). */
int pps_save_state(pps_graph* g);
int pps_restore_state(pps_graph* g);

/* ---- introspection (tests, bench, INTEGRATION) ---------------------------------------- */
typedef struct pps_stats {
  int    n_poses, n_planes, n_factors;
  int    dim_nodes, dim_measure;           /* Slam::_dim_nodes / _dim_measure               */
  int    n_fronts, n_levels, max_front;    /* multifrontal elimination tree of the last analysis */
  int64_t nnz_L;                           /* scalars stored in the factor panels           */
  int    lm_iterations;                    /* of the last batch_optimize                    */
  int    lm_trials_accepted, lm_trials_rejected;
  double chi2_initial, chi2_final, lambda_final;
  double last_delta_norm;
  /* wall-clock seconds of the last solve call, host side */
  double t_total, t_analysis, t_upload;
  /* device time (HIP events) of the last solve call, seconds, summed over launches */
  double t_linearize, t_assemble, t_factor, t_backsolve, t_retract_chi2;
  int    n_linearize, n_factorize;         /* launches of the sweep / factorizations        */
  int    lm_trials_notpd;                  /* LM trials whose factorisation hit a non-positive pivot (the step is then
                                              rejected like any other bad step; PPS_ENOTPD only if the last trial did) */
  int    n_launches;                       /* kernel launches of the last solve call (all streams)                    */
} pps_stats;
int pps_get_stats(const pps_graph* g, pps_stats* out);
/* LM trace of the last batch_optimize: per trial (lambda, chi2_new, accepted); returns count via n */
int pps_get_trace(const pps_graph* g, int cap, double* lambda, double* chi2, int* accepted, int* n);
/* HIP-event timing: 0 = off (default); 1 = event pairs around the Jacobian sweep only, no host syncs
 * (t_linearize / n_linearize = mean launch duration); 2 = every phase, adds stream syncs. */
int pps_set_profiling(pps_graph* g, int level);

/* Per-factor residual / Jacobian of the device sweep, for parity tests.
 * sel: 0 = linearisation point, 1 = estimate.  J is (dim x cols) row-major, r is the whitened residual. */
int pps_factor_shape(const pps_graph* g, int fid, int* dim, int* cols);
int pps_eval_factor(pps_graph* g, int fid, int mode /* enum pps_jacobian_mode */, double* J, double* r);

/* Host-side symbolic analysis only (no device needed): runs ordering + front construction. */
int pps_analyze(pps_graph* g);
/* Frame loops: a graph that only GROWS between two analyses (nodes / factors appended, every new factor touching a new node)
 * is analysed incrementally -- the part of the elimination tree left of the new poses, with all of its index arrays, is
 * kept (csrc/pps_symbolic.h).  fronts_kept of fronts_total of the last analysis were taken over (0 = from scratch). */
int pps_analysis_reuse(const pps_graph* g, int* fronts_kept, int* fronts_total);
/* What the last analysis left exactly as the analysis before it had it: leading entries of its index arrays (csrc/pps_symbolic.h,
 * Analysis::Kept) -- kept[6] = fronts, fronts_lists, blocks, segs, contribs, nd_segs.  The topology upload of a frame loop does not
 * compare those parts with its mirror again; tests/test_host_incremental.py checks the claim array by array. */
int pps_analysis_kept(const pps_graph* g, int kept[6]);
/* Flat dump of the analysis for host-logic tests.  Call with out == NULL to get the needed length. */
int pps_analysis_dump(pps_graph* g, int64_t cap, int32_t* out, int64_t* needed);

/* ---- K1 micro-benchmark entry: the Jacobian sweep over a batch of replicated graphs --- */
/* Replicates the handle's plane-observation and odometry edges `replicas` times in device
 * memory (state shared), runs `iters` sweeps and returns mean kernel times (HIP events, seconds):
 * sec[0] = both launches, sec[1] = plane-edge launch alone, sec[2] = odometry launch alone; plus the
 * number of plane / odometry edges per sweep.  Used for the HBM roofline figure.  mode: PPS_JAC_NUMERIC / PPS_JAC_ANALYTIC = the
 * thread-per-factor kernels, 2 = the lane-parallel numeric form (19 lanes per plane observation; what a graph below 200 000
 * factors runs). */
/* K1 of the handle's own graph, `iters` back-to-back launches on the solver's stream between two HIP events */
int pps_time_linearize(pps_graph* g, int mode, int iters, double* sec_per_launch);
int pps_bench_sweep(pps_graph* g, int mode, int replicas, int iters, double sec_per_sweep[3],
                    int64_t* n_plane_edges, int64_t* n_odo_edges);

/* ---- K3 diagnostic: one frontal matrix through the register-tile elimination, outside any graph ---- */
/* The dense partial Cholesky a front of the multifrontal factorisation goes through (the part of Cholesky.cpp's factorisation,
 * isam/Cholesky.cpp:86-130 via CHOLMOD's supernodal kernel, that happens inside one supernode), with the right-hand side as the
 * front's last row.  A: packed lower triangle, p + b + 1 rows (pivot rows, boundary rows, rhs row; row i holds i + 1 values).
 * L: (p + b + 1) x p row-major factor panel [L_A; L_B; y^T] (entries above the diagonal of L_A unspecified); U: packed lower
 * triangle of the (b + 1)-row update matrix [S; r^T].  tiles: 16-row tile rows held in registers, 2 .. 5, or 0 for what the solver
 * picks for a front of this size; strip != 0: rows 64 .. 79 as a strip of the LDS triangle under four tile rows (fronts of 65 .. 80
 * rows only).  not_pd: 1.0 when a pivot was not positive.  p <= 64, p + b + 1 <= 80.  Runs on the current device. */
int pps_debug_front_factor(int tiles, int strip, int p, int b, const double* A, double* L, double* U, double* not_pd);
/* The same with the panel width chosen: width 8 (two chained 4 x 4 pivot blocks per panel step: the level and wide kernels; what
 * pps_debug_front_factor runs) or 4 (one pivot block per step, the tile column a compile-time constant: the register-only band kernels,
 * fronts of at most 64 rows in 2 .. 4 tile rows -- width 4 with strip or five tile rows is PPS_EINVAL).  Found by symbol lookup, like the
 * pps_cov_* calls; PPS_VERSION was not bumped. */
int pps_debug_front_factor_w(int tiles, int strip, int p, int b, const double* A, double* L, double* U, double* not_pd, int width);

/* ---- K4 diagnostic: the retraction of n nodes outside any graph ---- */
/* kind 0: Pose3d::exmap (Pose3d.h:131-136: t += d[0:3], q <- q * Exp(d[3:6])); x n x 7 (tx ty tz qx qy qz qw), delta n x 6, out n x 7.
 * kind 1: Plane3d::exmap_3dof (isam_plane3d.h:101-127: Exp(d) * q, then normalised); x n x 4, delta n x 3, out n x 4.  The device
 * functions every retraction and every numerical-difference step of the solver goes through.  Runs on the current device. */
int pps_debug_exmap(int kind, int n, const double* x, const double* delta, double* out);

/* ---- K3 diagnostic: the solved step of the handle's graph, for one damping value or two ---- */
/* delta = (J'J + lambda diag(J'J))^-1 (-J'r) at the current estimate (Optimizer::compute_gauss_newton_step with the damping of
 * Cholesky.cpp:94-97), through the launches pps_update / pps_batch_optimize issue for this graph: K1 and K2 at the estimate, then the
 * factorisation and back-substitution of whichever K3 form the analysis chose.  The estimate stays where it is (the linearisation point
 * moves onto it, as in pps_eval_factor); the statistics and the LM trace of the last solve are kept; a covariance recovery ends.
 * delta: n_scalars doubles (pps_analysis_dump), one block per node at its node_voff -- 6 per pose (t, then the rotation vector), 3 per
 * plane; it is the step the retraction applies (x <- x (+) delta).
 * lambda2 >= 0 (band forms only, PPS_ESTATE elsewhere): both damping values in the launches of the LM loop's dual solve, delta2
 * (required then) receives the second step.  lambda2 < 0: one damping value, delta2 is not written.
 * form (optional): 0 band kernels, one launch per stage | 1 band kernels, the whole tree in one launch pair | 2 dense fronts | 3 one
 * launch per tree level (LDS fronts).  not_pd (optional): the status word the factorisation left, the larger one of a dual solve -- 0 ok,
 * 1 a pivot was not positive (delta is then no solution), >= 64 internal.  The status words are zero again when the call returns.
 * PPS_EINVAL (before the device is touched): null handle, null delta, lambda or lambda2 not a number, lambda < 0 or infinite,
 * lambda2 >= 0 without delta2. */
int pps_debug_solve(pps_graph* g, double lambda, double lambda2, double* delta, double* delta2, int* form, double* not_pd);

/* ---- pop-up (fp32), /root/reference/pop_up_wall --------------------------------------- */
/* popup_plane::update_plane_equation_from_seg (libs/popup_plane.cpp:654-705).
 * seg2d n x 4 (u1,v1,u2,v2); invK 3x3, T_wc 4x4 row-major; planes_out (n+1) x 4, row 0 = ground.
 * Host pointers; runs on `device`. */
int pps_popup_planes(int device, const float* seg2d, int n, const float invK[9], const float T_wc[16],
                     float* planes_out);

/* One pop-up point: world xyz + packed colour, 16 bytes (pcl::PointXYZRGB carries the same payload in
 * 32 B: popup_plane.cpp:943-983).  rgba = valid<<24 | r<<16 | g<<8 | b. */
typedef struct pps_point { float x, y, z; uint32_t rgba; } pps_point;

typedef struct pps_popup pps_popup;   /* per-camera context: device buffers for one image size */
int pps_popup_create(int device, int width, int height, const float invK[9], pps_popup** out);
int pps_popup_destroy(pps_popup* p);
const char* pps_popup_last_error(const pps_popup* p);
/* upload a BGR image (u8, width*height*3); stays resident for the following runs.  NULL = no colour. */
int pps_popup_set_image(pps_popup* p, const unsigned char* bgr);
/* Fused frame kernel, one launch: K5 segments -> plane equations (get_plane_equation,
 * popup_plane.cpp:551-603) and K6 pixels -> 3-D (generate_cloud + matrixToCloud :807-863,925-985;
 * get_depth_map_good :866-921).  Results stay on the device until pps_popup_download.
 *   seg2d    n x 4 ground segments; plane i >= 1 comes from segment i-1, plane 0 = ground
 *   polys    closed 2-D polygons (x,y) of the planes to pop up (all_closed_2d_bound_polygons,
 *            popup_plane.h:70-76), poly_off[nplanes+1] vertex offsets; an empty polygon skips the plane.
 *            The pixels of a polygon are the ones popup_plane::closed_polygons_homo_pts yields (popup_plane.cpp:81-116):
 *            vertices truncated to integers like cv::Point(float, float), shifted into their bounding box, rasterised
 *            with cv::fillConvexPoly's rules (8-connected Bresenham outline + 16.16 fixed-point scanline spans) --
 *            bit for bit, for any vertex list (|coordinate| < 2^15), convex or not.  Planes are written in order, so
 *            a pixel keeps the LAST polygon that covers it (generate_cloud / get_depth_map_good, :820-850, :893-911).
 *   step     1 = every pixel; 2 = downsample_poly (:86-87,104-108): the polygon is halved BEFORE the truncation,
 *            rasterised at half size and the pixel coordinates doubled -- even pixels only
 * Filters (matrixToCloud :948-960): z_s < 0, z_s > depth_thre, z_w < -0.2 dropped; z_w clamped to
 * ceiling_thre.  Depth: z_s, with the ceiling plane substituted above ceiling_thre (:903-916). */
int pps_popup_run(pps_popup* p, const float* seg2d, int n, const float T_wc[16], const float* polys,
                  const int* poly_off, int nplanes, int step, float depth_thre, float ceiling_thre, int* n_valid);
/* The same run without waiting for it (the frame loop, Mapping.cpp:401-586 / main_3d.cpp:423-503: the graph construction needs the plane
 * equations, the pixels are read later: by pps_map_add_frame, or when the frame is drawn).  pps_popup_planes_wait returns the (n+1) x 4 plane equations as soon as
 * the kernel's first workgroup has written them -- a few microseconds after the launch --, pps_popup_wait the end of the run (n_valid may be
 * NULL).  Every entry point that reads results of a run (download, plane_info, fill_depth, download_segments3d, the next run) waits for a
 * run in flight by itself. */
int pps_popup_run_async(pps_popup* p, const float* seg2d, int n, const float T_wc[16], const float* polys,
                        const int* poly_off, int nplanes, int step, float depth_thre, float ceiling_thre);
int pps_popup_planes_wait(pps_popup* p, float* planes);
int pps_popup_wait(pps_popup* p, int* n_valid);
/* any output may be NULL: planes (n+1)x4 sensor-frame, cloud width*height pps_point, depth width*height,
 * plane_id width*height (-1 = none) */
int pps_popup_download(pps_popup* p, float* planes, pps_point* cloud, float* depth, int32_t* plane_id);
/* switch the optional per-pixel outputs of pps_popup_run off / on (default: both on).  The cloud alone is 16 B per pixel
 * (what generate_cloud produces); the depth map (get_depth_map_good) and the plane-id map add 4 B each. */
int pps_popup_set_outputs(pps_popup* p, int want_depth, int want_plane_id);
/* The rest of get_plane_equation's per-plane outputs for the last run (popup_plane.cpp:616-640), n+1 entries, plane 0 = ground:
 *   dist_to_cam  all_plane_dist_to_cam: camera height for the ground, distance from the camera footprint to the world
 *                ground segment for a wall (what the mapper's sigma model reads, Mapping.cpp:507-512)
 *   good         1 for the ground and for every wall whose two ground points lie in front of the camera, closer than
 *                plane_cam_dist_thre (popup_plane.h:86: 10) and -- if actual_plane_indices is given (n_actual > 0; plane
 *                indices >= 1, e.g. open_in_closed + 1 of pps_edges_select) -- not a manually connected edge: good_plane_indices
 * Either output may be NULL. */
int pps_popup_plane_info(pps_popup* p, float plane_cam_dist_thre, const int* actual_plane_indices, int n_actual,
                         float* dist_to_cam, int32_t* good);
/* Tail of get_depth_map_good for the half-resolution pop-up (popup_plane.cpp:913-917, as main_3d.cpp:454 calls it): after
 * a pps_popup_run with step = 2 the depth map is defined on the even pixels only; this spreads it over the full frame the
 * way the reference does (resize 0.5, x 4, resize 2: bilinear from the half-size map).  Even image sizes only. */
int pps_popup_fill_depth(pps_popup* p);
/* ground_seg3d_lines_world of the last run (popup_plane.cpp:569-578): n x 6 = (x0,y0,0,x1,y1,0), the
 * world-frame ground end points of every segment -- columns 0,1 of all_3d_bound_polygons_world (:494-495),
 * which data association compares (Mapping.cpp:355-360). */
int pps_popup_download_segments3d(pps_popup* p, float* seg3d_world);
/* device time of the last pps_popup_run kernel (HIP events), seconds */
int pps_popup_last_kernel_time(const pps_popup* p, double* sec);
/* popup_plane::find_2d_3d_closed_polygon_simplemode (libs/popup_plane.cpp:409-500; simple_polygon_mode, popup_plane.h): the
 * closed 2-D polygon of every wall plane of a frame, from the ground / wall boundary segments pps_edges_select returns
 * (closed_segs) and the camera pose -- what pps_popup_run takes as `polys`.  walllength_threshold <= 0 (the class default,
 * popup_plane.h:81); the wall-length cut of :502-546 relies on cv::intersectConvexConvex and is not offered.  Host code (a
 * handful of fp32 operations per segment).  K / invK: the calibration and its inverse (popup_plane::set_calibration, :72-76).
 *   verts      (x, y) pairs, cap_verts >= 8 * n;  poly_off[n + 2]: vertex offsets of planes 0 .. n; plane 0 (ground) is empty
 *   a wall whose vertical lines do not reach the image boundary gets no polygon (:480-481) */
int pps_popup_polygons_simple(const float K[9], const float invK[9], const float T_wc[16], int width, int height, const float* seg2d, int n,
                              float* verts, int cap_verts, int* poly_off, int* n_verts);
/* The polygon -> pixel-set rules of pps_popup_run (closed_polygons_homo_pts / cv::fillConvexPoly, popup_plane.cpp:81-116)
 * evaluated on the host by the same interval code the kernel runs (no device needed; used by the CPU tests):
 * plane_id width*height, -1 = none. */
int pps_popup_mask_host(const float* polys, const int* poly_off, int nplanes, int width, int height, int step, int32_t* plane_id);

/* ---- pop-up feeding the graph: Mapper_mono::update_plane_measurement (Mapping.cpp:590-607) ------
 * Frames register their 2-D ground segments once; pps_refresh_measurements then re-derives every
 * registered edge's measurement from the CURRENT pose estimate, on the device, and writes it straight
 * into the edge array the Jacobian sweep reads (fp32 pop-up math, cast to fp64 and normalised like
 * Plane3d(Vector4d)).  fids has n_seg+1 entries (plane 0 = ground); -1 skips a plane. */
int pps_frames_set_calibration(pps_graph* g, const float invK[9]);
int pps_frames_add(pps_graph* g, int pose_id, int n_seg, const float* seg2d, const int* fids, int* frame_id);
int pps_refresh_measurements(pps_graph* g);
/* read back a plane factor's current measurement (FactorT::measurement(), Factor.h:203) */
int pps_get_measurement(pps_graph* g, int fid, double meas4[4]);

/* ---- plane data association: Mapper_mono::findClosestPlane (src/Mapping.cpp:256-397) ------------
 * The handle keeps one record per landmark (what findClosestPlane reads of a Map_plane, Map_plane.h:28-44);
 * the landmark's plane itself is read from the solver state on the device.  Landmark order (= tie-break
 * order, = all_landmarks index) is the order of first registration. */
typedef struct pps_assoc_params {   /* Mapping.h:70-77; tum yaml: 10000, 2, -1, 35, 1000 */
  double edge_asso_2ddist;          /* 50   mean 2-D end-point distance gate [px] */
  double edge_asso_planedist;       /* 4    plane distance gate [m] */
  double edge_asso_proj;            /* 0.5  minimum mutual 1-D overlap of the ground segments */
  double edge_asso_angle;           /* 60   normal angle gate [deg] */
  int assoc_near_frames;            /* 5    only landmarks seen within this many frames */
} pps_assoc_params;
void pps_assoc_default_params(pps_assoc_params* p);
/* copy_plane (Map_plane.cpp:11-22) after an observation: (re)write the landmark's latest frame
 * properties; the first call for a plane id registers it (all_landmarks.push_back, Mapping.cpp:485-488).
 * seg2d = ground edge end points in the image (u0,v0,u1,v1); seg3d_xy = their world x,y (x0,y0,x1,y1);
 * both may be NULL for the ground plane. */
int pps_landmark_update(pps_graph* g, int plane_id, int frame_plane_indice, int frame_seq_id, const float seg2d[4],
                        const float seg3d_xy[4]);
int pps_landmark_set_merged(pps_graph* g, int plane_id);      /* deteted_by_merge = true (Mapping.cpp:697) */
/* n query planes of one frame against all landmarks, one launch.  planes_local n x 4 (sensor frame,
 * Map_plane::temp_value), est_pose = latest pose (+) odometry (Mapping.cpp:413-416).
 * best_plane_id[i] = plane node id of the match or -1; best_err[i] = its score (-1: none / ground). */
int pps_find_closest_planes(pps_graph* g, const double est_pose[7], int frame_seq_id, int n, const double* planes_local,
                            const int* frame_plane_indice, const float* seg2d, const float* seg3d_xy,
                            const pps_assoc_params* prm, int* best_plane_id, double* best_err);

/* ---- graph text format: Slam::save (isamlib/Slam.cpp:84-89) / Graph::write (include/isam/Graph.h:120-131) ----
 * One line per factor, then one line per node, in insertion order:
 *   Pose3d_Pose3d_Factor 3 4 (x, y, z; yaw, pitch, roll) {s11,s12,...,s66}
 *   Pose3d_Plane3d_Factor 4 17 (a, b, c; d) {s11,s12,s13,s22,s23,s33}
 *   Pose3d_Factor 0 (...) {...}            pose prior AND plane prior (name quirk, isam_plane3d.h:438)
 *   Pose3d_Node 4 (x, y, z; yaw, pitch, roll)     Plane3d_Node 17 (a, b, c; d)
 * precision <= 0: 6 significant digits like the reference's ostream default (lossy); 17 round-trips doubles.
 * pps_graph_load reads this format back into a new handle (the reference has no reader for it); node ids are
 * re-assigned densely in file order.  A Factor2 edge (pps_add_plane_obs2) prints like the reference's -- same name,
 * stored measurement (isam_plane3d.h:327) -- so its ground-edge rays are not part of the file and it reloads as a
 * plain observation. */
int pps_graph_save(pps_graph* g, const char* path, int precision);
int pps_graph_load(const char* path, const pps_props* props, pps_graph** out);

/* Mapper_mono::reproj_to_newplane (src/Mapping.cpp:609-632): stored polygon vertices (fp32 world points) projected onto
 * the CURRENT estimate of their landmark plane -- Plane3d::project_to_plane (src/isam_plane3d.h:173-178) in fp64, result
 * cast back to fp32.  plane_ids[i] is the plane node of point i; points of removed (merged) landmarks are copied through. */
int pps_reproject_points(pps_graph* g, int n, const int* plane_ids, const float* pts_xyz, float* out_xyz);

/* ---- ground-edge selection: popup_plane::edge_get_polygons (pop_up_wall/libs/select_edge.cpp:66-409) -------------
 * The step before the pop-up: the CNN label map (u8, ground = 255) and the raw LSD line segments of a frame become
 * the ground / wall boundary polyline pps_popup_run and pps_frames_add take.  Per-pixel work runs on the device:
 * [half-size nearest resize], dilate, erode and inversion of the label map in one kernel (select_edge.cpp:69-78),
 * then the marching-squares cells of skimage.measure.find_contours(label, 0) in raster order (the reference calls it
 * through boost::python, pop_up_fun.py:85-106).  The contour linking and the segment selection (steps 1-6 of
 * select_edge.cpp and interval_tree_optimization, pop_up_fun.py:109-204) are sequential work on a few hundred
 * segments and run on the host inside the same call.  LSD detection itself (line_lbd, OpenCV) is not part of this
 * library: lsd_lines are an input, as they are for edge_get_polygons. */
typedef struct pps_edge_params {
  int downsample_contour;                    /* popup_plane.h:82 (false) */
  int dilation_distance, erosion_distance;   /* popup_plane.cpp:32-33 (11, 11) */
  /* popup_plane.h:184-192: 15 15 50 20 30 10 20 10 15 */
  double pre_vertical_thre, pre_minium_len, pre_contour_close_thre, interval_overlap_thre, post_short_thre,
         post_bind_dist_thre, post_merge_dist_thre, post_merge_angle_thre, post_extend_thre;
  /* popup_plane.h:194-200: 5 10 10 20 0.6 0.8 100 */
  double pre_boundary_thre, pre_merge_angle_thre, pre_merge_dist_thre, pre_proj_angle_thre, pre_proj_cover_thre,
         pre_proj_cover_large_thre, pre_proj_dist_thre;
} pps_edge_params;
void pps_edge_default_params(pps_edge_params* p);

typedef struct pps_edges pps_edges;   /* per-camera context: device buffers for one label-map size */
int pps_edges_create(int device, int width, int height, pps_edges** out);
int pps_edges_destroy(pps_edges* e);
const char* pps_edges_last_error(const pps_edges* e);
/* label_map: width*height u8, a host pointer or (label_on_device != 0) a device pointer on the context's device (the
 * kernels run on the context's own stream: the producer of a device-resident map must have finished, e.g. by an event
 * or stream synchronisation on the caller's side).
 * lsd_lines n_lines x 4 (x1 y1 x2 y2), host.  Outputs (host, caller-allocated, 2*n_lines+2 rows each):
 *   open_segs       n_open x 4    ground_seg2d_lines_actual
 *   closed_segs     n_closed x 4  ground_seg2d_lines_connect (connecting pieces inserted)
 *   open_in_closed  n_open        row of each open segment in closed_segs (actual_walls_in_closepoly_ind)
 * No boundary in the label map / no line survives: n_open = n_closed = 0, PPS_OK (the reference prints
 * "cannot find ground edges"). */
int pps_edges_select(pps_edges* e, const unsigned char* label_map, int label_on_device, const float* lsd_lines,
                     int n_lines, const pps_edge_params* prm, float* open_segs, int* n_open, float* closed_segs,
                     int* n_closed, float* open_in_closed);
/* intermediate results of the last pps_edges_select, for tests and debugging: the pre-processed label map
 * (w x h bytes, ground = 0), the sub-sampled ground contour as (x, y) pairs, the number of contours found and the
 * length of the chosen one */
int pps_edges_download_label(pps_edges* e, unsigned char* out, int* w, int* h);
int pps_edges_contour(pps_edges* e, float* xy, int cap, int* n, int* n_contours, int* n_points);
/* device time of the kernels of the last pps_edges_select (HIP events), seconds */
int pps_edges_last_kernel_time(const pps_edges* e, double* sec);
/* The two host stages of pps_edges_select on their own (no device needed; used by the CPU tests):
 * cell segments (n x 4 int16: from row, from column, to row, to column, in raster order of the cells) -> sub-sampled
 * ground contour; contour + LSD lines -> selection. */
int pps_edges_host_contour(const int16_t* cell_segs, int n, float scale, float* xy, int cap, int* n_xy, int* n_contours,
                           int* n_points);
int pps_edges_host_select(const float* contour_xy, int n_contour, int width, int height, const float* lsd_lines, int n_lines,
                          const pps_edge_params* prm, float* open_segs, int* n_open, float* closed_segs, int* n_closed,
                          float* open_in_closed);

/* ---- dense map: the per-plane clouds of every frame, kept on the device and re-projected there ------------------
 * The reference's final product.  Every frame keeps the cloud of each of its good planes (Map_plane::plane_cloud /
 * tracking_frame::partplane_clouds, main_3d.cpp:475,493, cut out of the frame by popup_plane::matrixToCloud, popup_plane.cpp:925-985); when
 * the sequence ends, every kept point is projected onto the current estimate of its landmark plane and published, frames and planes thinned
 * by age and by how often the landmark was tracked (main_3d.cpp:535-588).  A pps_map is that store for one graph: pps_map_add_frame splits
 * the cloud of the last pps_popup_run by plane id into chunks -- on the device, the cloud is not downloaded --, pps_map_build writes the map.
 *
 * The map belongs to a graph (same device; the graph must outlive it; one host thread drives both) and reads that graph's plane estimates.
 * It holds `capacity_points` pps_point in one device buffer (taken by the first pps_map_add_frame) and as many for the built map (taken by
 * the first pps_map_build); it never grows.  Creating a map, its bookkeeping calls and every argument check work without a device.
 * The RAW points are kept: a build after further optimisation projects the original points again.  (The reference overwrites its clouds in
 * place, main_3d.cpp:574-576 -- a second pass there would project the projections.)
 * PPS_VERSION was not bumped for them (it stayed 304): a caller detects these entry points by symbol lookup (dlsym "pps_map_create"), like pps_cov_*. */
typedef struct pps_map pps_map;
/* one chunk = the points of one plane of one frame, `count` consecutive points from `offset` in the buffer the table describes */
typedef struct pps_map_chunk {
  int32_t frame;            /* frame index in insertion order (frame_ind of main_3d.cpp:538)                     */
  int32_t frame_seq_id;     /* tracking_frame::frame_seq_id                                                       */
  int32_t frame_plane;      /* plane index inside the frame, 0 = ground (Map_plane::frame_plane_indice)            */
  int32_t plane_id;         /* plane node the chunk belongs to NOW (observed_planes[k]->plane_vertex)              */
  int64_t offset, count;
} pps_map_chunk;
typedef struct pps_map_totals {
  int64_t capacity, n_points;          /* points the store can hold / holds                                       */
  int64_t built_points;                /* points of the last build                                                */
  int32_t n_frames, n_chunks, built_chunks, reserved;
} pps_map_totals;
/* the thinning of main_3d.cpp:544-562 */
typedef struct pps_map_select {
  int32_t counter;                     /* frame_seq_id of the last frame (`counter` when the map is published)    */
  int32_t every_frame;                 /* final_reproject_label_img: keep every frame                             */
  int32_t old_age, old_every, new_every;   /* 10 3 2: frames with frame_seq_id <= counter - old_age keep every old_every-th frame index, newer ones every new_every-th (:545-551) */
  int32_t age[3], min_tracked[3];      /* (15, 10) (8, 5) (4, 2): a chunk with frame_seq_id <= counter - age[i] needs tracked times >= min_tracked[i] (:554-562) */
} pps_map_select;
void pps_map_default_select(pps_map_select* s, int counter);
int pps_map_create(pps_graph* g, int64_t capacity_points, pps_map** out);
int pps_map_destroy(pps_map* m);
const char* pps_map_last_error(const pps_map* m);
/* The last run of `p` (a run in flight is waited for) becomes a frame of the map: one chunk per frame plane k = 0 .. nplanes-1 (ground
 * included) with plane_node_ids[k] >= 0, holding the points whose valid bit is set and whose plane-id pixel equals k, in raster order of
 * their pixels (after a step = 2 run: the even pixels), copied bit for bit.  plane_node_ids[k] = -1 skips the plane; a plane without a
 * valid point still gets an (empty) chunk: it is an observation of its landmark.  counts[nplanes] (may be NULL): points per plane.
 * The call waits for its own kernels (the pop-up context may start its next run when it returns).
 *   PPS_ESTATE  no run yet, or the run had the plane-id output switched off (pps_popup_set_outputs)
 *   PPS_EINVAL  NULL handle, nplanes outside 0 .. 65, an id that is not a live plane node of the graph, a context on another device
 *   PPS_ENOMEM  the frame's kept points exceed the remaining capacity; the map is unchanged */
int pps_map_add_frame(pps_map* m, pps_popup* p, int frame_seq_id, int nplanes, const int* plane_node_ids, int* counts);
/* Test hook: a frame of the map from HOST arrays -- cloud[npx] and plane_id[npx] in raster order, what pps_popup_download returns of a
 * run -- so that a test chooses the pixel count, the plane count and the pattern of ids itself.  The two arrays are copied to scratch device
 * buffers of the map on the graph's stream; from there on the call IS pps_map_add_frame (one function serves both: tiling, count, scan,
 * totals, capacity check, scatter, chunk table, counts, pps_map_last_times), so what it stores is what a pop-up run with these pixels
 * would have stored.  Only the upload is the hook's own.  A frame with nplanes = 0 reads no pixel and needs no device.
 *   PPS_EINVAL  answered on the host before any device work, the map unchanged: NULL m / cloud / plane_id, npx outside 1 .. 2^30 (the
 *               kernels index pixels with int), nplanes outside 0 .. 65, an id that is neither -1 nor a live plane node of the graph
 *   PPS_ENOMEM  as pps_map_add_frame: the map is unchanged */
int pps_debug_map_add_points(pps_map* m, const pps_point* cloud, const int* plane_id, int64_t npx, int frame_seq_id, int nplanes,
                             const int* plane_node_ids, int* counts);
/* loopclose_merge / copy_plane (Mapping.cpp:659-700, Map_plane.cpp:25): every chunk of from_plane belongs to to_plane from now on (and
 * counts towards its tracked times).  from_plane: a plane node id of the graph, live or removed; to_plane: a live one. */
int pps_map_redirect(pps_map* m, int from_plane, int to_plane);
int pps_map_info(const pps_map* m, pps_map_totals* out);
/* chunk table of the store / of the last build (offsets into the built map): *n = chunks in all, the first min(cap, *n) are copied */
int pps_map_chunks(const pps_map* m, int cap, pps_map_chunk* out, int* n);
int pps_map_built_chunks(const pps_map* m, int cap, pps_map_chunk* out, int* n);
/* main_3d.cpp:544-562 over a chunk table, host only: keep[i] = 1 if chunk i is published.  being_tracked_times of a landmark = the
 * chunks of the table, empty ones included, that belong to it.  sel == NULL keeps all.  n_keep may be NULL. */
int pps_map_select_host(const pps_map_chunk* chunks, int n, const pps_map_select* sel, int32_t* keep, int* n_keep);
/* The map: the selected chunks (sel == NULL: all) back to back in chunk order, every point projected onto the current estimate of its
 * landmark -- Plane3d::project_to_plane (src/isam_plane3d.h:173-178) in fp64 on the fp32 point, result cast to fp32, the device function of
 * pps_reproject_points, bit for bit --, rgba copied.  Points of a landmark that was removed and not redirected pass through untouched.
 * The estimate is brought to the device like pps_reproject_points does; the store is not modified. */
int pps_map_build(pps_map* m, const pps_map_select* sel, int64_t* n_points, int* n_chunks);
/* points [first, first + n) of the store (which = 0) or of the built map (which = 1) */
int pps_map_download(pps_map* m, int which, int64_t first, int64_t n, pps_point* out);
/* device seconds (HIP events): sec[0] the kernels of the last pps_map_add_frame, sec[1] the kernel of the last pps_map_build */
int pps_map_last_times(const pps_map* m, double sec[2]);

/* ---- grid map: one point per cell of every landmark plane ----------------------------------------------------------
 * pps_map_build writes every kept point of every selected chunk: the map grows with the length of the run although the walls do not.
 * A landmark is a plane, so its points live on a 2-D lattice in that plane; pps_map_build_grid keeps ONE point per lattice cell.
 *
 * Let B be the map pps_map_build(m, sel, ..) would write at the current estimate.  The grid map is a subset of B's records, bit for bit.
 *   taking part   the points of B whose chunk belongs to a live plane node.  Points of a landmark that was removed and not redirected
 *                 take no part (n_passed_through counts them; the grid has no cells for them).
 *   frame         per landmark, on the host in fp64 from the four doubles p[0..3] of the estimate the device projects with:
 *                 l = sqrt(p0^2 + p1^2 + p2^2), n = (p0, p1, p2) / l, a = (0,0,1) if |n_z| <= 0.7 else (1,0,0), e1 = (a x n) / |a x n|,
 *                 e2 = n x e1.  Anchored at the foot of the world origin: a point's plane coordinates are u = p . e1, v = p . e2.
 *   cell          with x, y, z the fp32 coordinates B holds, converted to double: u = (x*e1[0] + y*e1[1]) + z*e1[2] (every product and sum
 *                 rounded once, never fused), i = floor(u * inv_cell) with inv_cell = 1.0 / cell; j likewise from e2.  A point whose u or
 *                 v is not finite, or whose |i| or |j| is 2^30 or more, is dropped (n_dropped).
 *   winner        of a cell: the point with the greatest (PPS_GRID_NEWEST) or smallest (PPS_GRID_OLDEST) index in B.  A cell is emitted
 *                 if at least min_count points fell into it; it carries that count.
 *   order         landmarks by ascending plane node id; inside a landmark the cells of its bounding box (i0, j0, ni, nj: the extent of
 *                 the points that voted) in raster order, j ascending, then i.  Nothing depends on the order waves run in: two calls on
 *                 the same state give the same bytes.
 *   limit         the boxes of all landmarks together hold at most max_cells cells, else PPS_ENOMEM before anything of that size is
 *                 allocated; the text names the landmark with the largest box (one far outlier makes such a box).
 * The grid has device buffers of its own; the store, the result of the last pps_map_build, the chunk tables and the graph are not touched.
 * A call that fails leaves no grid (pps_map_grid_info reports zeros); the map stays usable.  Found by symbol lookup, like pps_map_create;
 * PPS_VERSION was not bumped. */
enum pps_grid_rule { PPS_GRID_NEWEST = 0, PPS_GRID_OLDEST = 1 };
typedef struct pps_map_grid_params {
  double cell;                     /* edge of a cell in metres */
  int32_t rule, min_count;
  int64_t max_cells;
} pps_map_grid_params;
void pps_map_grid_default_params(pps_map_grid_params* p);          /* 0.02 m, NEWEST, 1, 1 << 26 */
typedef struct pps_map_grid_plane {
  int32_t plane_id, n_chunks;      /* selected chunks that belong to it now, empty ones included */
  int32_t i0, j0, ni, nj;          /* bounding box of its cells (all 0 if no point of it voted) */
  int64_t offset, count;           /* its cells in the grid map */
  int64_t n_in;                    /* points that took part and were not dropped */
  double  n[3], e1[3], e2[3];
} pps_map_grid_plane;
typedef struct pps_map_grid_totals {
  int64_t n_points;                /* points of B = n_in + n_dropped + n_passed_through */
  int64_t n_cells;                 /* cells emitted: the points of the grid map */
  int64_t n_in, n_dropped, n_passed_through;
  int32_t n_planes, launches;
  double  cell, inv_cell;
  double  sec[4];                  /* device seconds (HIP events): extent pass | vote pass | emission | whole call */
} pps_map_grid_totals;
/* n_points (may be NULL): cells emitted; n_planes (may be NULL): rows of the plane table = live landmarks with a selected chunk.
 *   PPS_EINVAL  answered on the host without a device: NULL m, cell not finite or <= 0 or so small that 1.0 / cell is not finite, an
 *               unknown rule, min_count < 1, max_cells < 1, an invalid sel (the rule of pps_map_build).  prm == NULL: the defaults.
 *   PPS_ENOMEM  more than max_cells cells, or the device has no room for the grid's buffers
 * A selection without a point that takes part returns PPS_OK with zero points and needs no device. */
int pps_map_build_grid(pps_map* m, const pps_map_select* sel, const pps_map_grid_params* prm, int64_t* n_points, int* n_planes);
/* the plane table of the last grid: *n = rows in all, the first min(cap, *n) are copied */
int pps_map_grid_planes(const pps_map* m, int cap, pps_map_grid_plane* out, int* n);
int pps_map_grid_info(const pps_map* m, pps_map_grid_totals* out);
/* cells [first, first + n) of the last grid; every output may be NULL: the point, the points that fell into the cell, (i, j),
 * and the winner's index in the map pps_map_build writes for the same selection.  PPS_EINVAL: a range outside the grid. */
int pps_map_grid_download(pps_map* m, int64_t first, int64_t n, pps_point* pts, uint32_t* counts, int32_t* ij, int64_t* src);
/* host only, no device: the frame and the cell arithmetic as stated above, compiled from the header the kernels include.
 * frame: PPS_EINVAL if abc has no finite positive length.  cell: *cell = floor(u * inv_cell) for one axis e, *dropped = 1 if the point
 * is dropped on that axis (*cell is then 0). */
int pps_map_grid_frame_host(const double abcd[4], double n[3], double e1[3], double e2[3]);
int pps_map_grid_cell_host(const double e[3], double inv_cell, const float xyz[3], int64_t* cell, int* dropped);

/* ---- rendered view: the grid map seen from a camera pose ---------------------------------------------------------------
 * pps_map_render casts the ray of every pixel of a pinhole camera onto every landmark plane of the LAST GRID and keeps the nearest hit
 * whose lattice cell was emitted: the inverse of the pop-up kernel.  It leaves four images on the device, in the shapes of
 * pps_popup_download: the cloud, the depth, the plane id, and the index of the grid cell that answered.  The view is of the grid as it was
 * built: the plane equations are the ones grid_frame was given (pps_map_grid_plane_eq), not the graph's current estimate.
 *
 * All arithmetic is fp64 in the order written; every product and sum is rounded once, nothing is fused.
 *   ray           of pixel (col, row): x = col, y = row as doubles, iK and T the floats of the view converted to double.
 *                 ds[k] = (iK[3k]*x + iK[3k+1]*y) + iK[3k+2];  dw[k] = (T[4k]*ds[0] + T[4k+1]*ds[1]) + T[4k+2]*ds[2];  o[k] = T[4k+3].
 *   landmark      rows of pps_map_grid_planes in their order (ascending plane id); rows with ni * nj = 0 are skipped.  With p the row's four
 *                 doubles and l, n, e1, e2 exactly as the grid's frame computes them: dn = p[3] / l,
 *                 den = (n0*dw0 + n1*dw1) + n2*dw2,  h = ((n0*o0 + n1*o1) + n2*o2) + dn.  No hit if den is 0 or not finite.
 *                 t = (-h) / den; no hit unless t > 0.  z = t * ds[2]; no hit unless z_near <= z <= z_far (a NaN fails).
 *                 X[k] = o[k] + t*dw[k], Xf = (float)X; no hit if a component is not finite.  (i, j) = the grid's cell of Xf along e1 and
 *                 e2 with the grid's inv_cell; no hit if either axis drops the point.  A plane is seen from both sides.
 *   cell          for ring k = 0 .. reach: for dj = -k .. k ascending, for di = -k .. k ascending, only pairs with max(|di|, |dj|) = k:
 *                 the first (i + di, j + dj) inside the row's box that is an emitted cell (its count >= the grid's min_count) answers.
 *                 If none answers there is no hit on this landmark.
 *   pixel         the hit with the smallest z wins, among equal z the earlier row.  depth = (float)z, plane_id = the landmark's node id,
 *                 cell = the index of the answering cell in the grid map (what pps_map_grid_download indexes), cloud = (Xf, the rgba of
 *                 that grid point).  Without a hit: cloud all zero bits, depth 0, plane_id -1, cell -1.  n_hit = the pixels with a hit.
 * Not offered: anti-aliasing, a back-face rule, a view at the current estimate without a new grid.
 * The render changes nothing else: the store, the built map, the grid and its download calls, the chunk tables and the graph.  A grid call
 * of either kind, whether it succeeds or fails, ends the rendered view.  Found by symbol lookup, like pps_map_create; PPS_VERSION was not bumped. */
typedef struct pps_map_view {
  int32_t width, height;        /* 1 .. 4096 each */
  int32_t reach;                /* 0 .. 4: how many rings of neighbouring cells may answer for an empty cell */
  int32_t reserved;             /* 0 */
  float   invK[9];              /* row-major, as pps_popup_create takes it */
  float   T_wc[16];             /* row-major 4x4, sensor -> world; rigid by the rule of pps_map_set_frame_pose */
  double  z_near, z_far;        /* 0 <= z_near < z_far; z_far may be +inf */
} pps_map_view;
typedef struct pps_map_render_totals {
  int32_t width, height;
  int32_t n_planes;             /* landmarks cast: the rows of the plane table that have a box */
  int32_t launches;             /* kernels of the call: 1, 2 on the first render after a grid (the slot table), 0 without a device */
  int64_t n_hit;
  double  sec;                  /* device seconds (HIP events) of the render kernels */
} pps_map_render_totals;
void pps_map_default_view(pps_map_view* v, int width, int height, const float invK[9], const float T_wc[16]);  /* reach 1, z_near 0, z_far +inf */
/* n_hit may be NULL.
 *   PPS_EINVAL  answered on the host before any device work, nothing changed: NULL m or v, a size outside 1 .. 4096, reach outside 0 .. 4,
 *               reserved != 0, a non-finite invK entry, a T_wc that is not rigid, z_near not finite or < 0, z_far NaN or <= z_near
 *   PPS_ESTATE  there is no grid: no grid call has succeeded yet, or the last one failed
 *   PPS_ENOMEM  the device has no room for the images or for the slot table (one int per box cell, made by the first render after a
 *               grid and kept until the next grid call); the grid stays valid
 * A grid with zero cells renders PPS_OK with every pixel empty and needs no device. */
int  pps_map_render(pps_map* m, const pps_map_view* v, int64_t* n_hit);
/* the images of the last render, width * height records each in raster order; any may be NULL.  PPS_ESTATE: no render present. */
int  pps_map_render_download(pps_map* m, pps_point* cloud, float* depth, int32_t* plane_id, int64_t* cell);
int  pps_map_render_info(const pps_map* m, pps_map_render_totals* out);                                       /* PPS_ESTATE: no render present */
/* the plane equation the last grid was built with: row r of pps_map_grid_planes -> abcd[4 r .. 4 r + 3] (the four doubles the frame was
 * computed from); *n = rows in all, the first min(cap, *n) are copied */
int  pps_map_grid_plane_eq(const pps_map* m, int cap, double* abcd, int* n);
/* host only, no device: ONE pixel against ONE landmark as stated above, compiled from the header the kernel includes.  hit: returns 1 for
 * a hit (z, xyz = Xf, ij = the cell of Xf, before any ring), 0 for none (outputs zeroed), -1 for a NULL pointer or a plane without a normal. */
int  pps_map_render_ray_host(const pps_map_view* v, int col, int row, double o[3], double ds[3], double dw[3]);
int  pps_map_render_hit_host(const double o[3], const double ds[3], const double dw[3], const double abcd[4], double inv_cell,
                             double z_near, double z_far, double* z, float xyz[3], int64_t ij[2]);

/* ---- posed map: stored points follow their frame's pose estimate -----------------------------------------------------
 * The store holds every frame's points in world coordinates, made with the T_wc its pop-up run was given -- the pose predicted from
 * odometry (main_3d.cpp:426-431).  pps_map_build repairs a point along the normal of its landmark only; when the optimiser moves the
 * frame's pose (a loop closure moves it by metres), the point stays where the old pose put it inside the plane.  A posed build first moves
 * every stored point rigidly with the correction of its frame's pose and then projects it as pps_map_build does.
 *
 * All arithmetic is fp64 in the order written, nothing is fused.
 *   frame record  a frame may carry T0 (row-major 4x4 fp32, sensor -> world, as given to the pop-up run) and the id of a pose node.
 *                 R0 = T0[0:3,0:3], t0 = T0[0:3,3], converted to double.  T0 must be rigid to fp32: every entry finite, last row
 *                 (0,0,0,1), max |R0^T R0 - I| <= 1e-4.
 *   motion        D = (R_D, t_D), 12 doubles (R_D row-major, then t_D).  With (t, q) the current estimate of the pose node and R the
 *                 rotation matrix of q as the solver forms it (Eigen::Matrix3d(q), no renormalisation): R_D = R R0^T, every entry
 *                 (a*b + c*d) + e*f; t_D = t - R_D t0, the product summed the same way, then one subtraction.  Computed on the device
 *                 from the estimate in place, one thread per frame; no pose is downloaded.  A frame without a record, or whose pose node
 *                 is not live any more, has no motion: its points are not moved (n_unposed_frames counts such frames).
 *   point         (x, y, z) the fp32 store coordinates converted to double; x' = ((R_D[0]*x + R_D[1]*y) + R_D[2]*z) + t_D[0], y' and z'
 *                 likewise.  If the chunk's landmark is live, Plane3d::project_to_plane on the DOUBLES (x', y', z') with the arithmetic
 *                 of pps_map_build (no cast to fp32 in between); if it is gone and was not redirected, (x', y', z') itself.  One cast to
 *                 fp32; rgba copied.  A point that is not moved is pps_map_build's point, bit for bit: a posed build of a map without
 *                 any frame record IS pps_map_build's map.
 *   order, selection, chunk tables: pps_map_build's.  The result replaces the built map (pps_map_download(which = 1), pps_map_built_chunks).
 * Rigid motion plus projection is exact to first order in the plane's correction; it does not re-intersect the pixel's ray with the moved
 * plane.  Found by symbol lookup, like pps_map_create; PPS_VERSION was not bumped. */
typedef struct pps_map_frame {
  int32_t frame, frame_seq_id;     /* insertion index (pps_map_chunk.frame), tracking_frame::frame_seq_id */
  int32_t pose_id, reserved;       /* pose node of the record, -1: none */
  float   T_wc[16];                /* T0 of the record (zeros without one) */
} pps_map_frame;
/* The record of `frame` (its insertion index).  T_wc == NULL: the T_wc of the pop-up run the frame was added from (pps_map_add_frame
 * remembers it).  pose_node_id = -1 clears the record.  Needs no device.
 *   PPS_EINVAL  NULL m, an unknown frame, an id that is not a live pose node of the graph, a T_wc that is not rigid (above), T_wc == NULL
 *               for a frame added with pps_debug_map_add_points.  The record is unchanged. */
int pps_map_set_frame_pose(pps_map* m, int frame, int pose_node_id, const float T_wc[16]);
/* the frame table: *n = frames in all, the first min(cap, *n) are copied.  Needs no device. */
int pps_map_frames(const pps_map* m, int cap, pps_map_frame* out, int* n);
/* pps_map_build with every point moved as stated above; arguments and errors of pps_map_build. */
int pps_map_build_posed(pps_map* m, const pps_map_select* sel, int64_t* n_points, int* n_chunks);
/* pps_map_build_grid with B replaced by the map pps_map_build_posed writes for the same selection and state: every sentence of the grid
 * statement holds with that B (subset bit for bit, src indexes it); pps_map_grid_* read the result like any grid.  The built map itself
 * is not touched. */
int pps_map_build_grid_posed(pps_map* m, const pps_map_select* sel, const pps_map_grid_params* prm, int64_t* n_points, int* n_planes);
/* The motion table of the last posed build or posed grid that ran on the device, copied from it: one row per frame that has a point in the
 * selection, in frame order (the distinct `frame` values of the selected non-empty chunks, ascending).  *n = rows in all; the first
 * min(cap, *n) rows go to D (cap x 12, may be NULL) and moved (may be NULL; 0: the frame has no motion, its row is the identity).
 * For callers that move polygons the same way. */
int pps_map_frame_motions(pps_map* m, int cap, double* D, int32_t* moved, int* n);
/* of the last posed call (each output may be NULL): device seconds (HIP events) of the motion kernel and of the posed build kernel (0
 * after a posed grid: pps_map_grid_info has its passes); kernels launched outside the grid passes; frames of the motion table without a motion */
int pps_map_posed_last(const pps_map* m, double sec[2], int* launches, int* n_unposed_frames);
/* host only, no device: the statement above, compiled from the header the kernels include.  motion: tq in the layout of pps_get_pose;
 * PPS_EINVAL if T_wc is not rigid.  move_point: D == NULL leaves the point unmoved, abcd == NULL unprojected. */
int pps_map_motion_host(const float T_wc[16], const double tq[7], double D[12]);
int pps_map_move_point_host(const double* D, const double* abcd, const float xyz[3], float out[3]);

/* ---- compared views: a pop-up frame against the rendered map view ----------------------------------------------------
 * pps_map_compare compares the last run of a pop-up context with the LAST RENDER of the map: pixel for pixel, at the same raster index, it
 * fills a table of integer counters on the device.  It changes neither of them.  Everything is integer except one fp64 expression per
 * pixel, evaluated in the order written, every product and sum rounded once, nothing fused.
 *   inputs        the render's images (width x height); the plane table of the grid it was rendered from (the rows of pps_map_grid_planes,
 *                 n_rows of them, ascending node id) with the grid's own plane equations (pps_map_grid_plane_eq), not the graph's current
 *                 estimate; the run's cloud and plane-id map (a run in flight is waited for); nplanes (1 .. 65 frame planes, 0 = ground);
 *                 tol (metres, finite, >= 0).
 *   frame side    k = the run's plane id of the pixel.  0 <= k < nplanes and the valid bit (bit 24 of rgba) set: valid with frame plane k.
 *                 k = -1 or the valid bit clear: none.  Any other k (k < -1 or k >= nplanes): none as well, and counted in n_bad_id,
 *                 whatever its valid bit says.
 *   view side     the render's plane id is -1: none.  Otherwise r = the row of the plane table whose plane_id equals it.
 *   classes       every pixel adds 1 to exactly one of: n[k][r] (both sides present), n_new[k] (a frame and no view), n_unseen[r] (a view
 *                 and no frame), n_neither.
 *   pair          both sides present.  p = the row's four doubles; l, n exactly as the grid's frame computes them, dn = p[3] / l as the
 *                 render computes it; x, y, z the fp32 coordinates of the POP-UP point converted to double.
 *                 e = ((n[0]*x + n[1]*y) + n[2]*z) + dn: the signed distance of the frame's point from the map's plane (a distance to the
 *                 plane, not a depth difference: the ceiling clamp of the pop-up moves a point along a vertical wall, not off it).
 *                 agree = fabs(e) <= tol (a NaN fails).  s = e * 4096.0 (exact).  s NaN or s >= 524288: q = 524288; s <= -524288:
 *                 q = -524288; else q = (long long)rint(s), ties to even.  The pair accumulates n += 1, n_agree += agree, sum_q += q,
 *                 sum_q2 += q*q, all int64 (width, height <= 4096: sum_q2 <= 2^38 * 2^24).  Mean and rms distance in metres:
 *                 sum_q / (4096 n) and sqrt(sum_q2 / n) / 4096, to a quantum of 0.24 mm.
 *   best landmark of frame plane k: the row with the greatest n_agree; among equal rows the greater n, among those the earlier row;
 *                 best_row = best_plane_id = -1 if no row has n_agree >= 1.
 *   pair list     the entries with n >= 1, by k ascending, then r ascending.
 * Every accumulator is an integer: the result does not depend on the order waves run in, two calls on the same state give the same bytes.
 * The views are compared index by index: nothing asks that the render's T_wc is the run's; render at the pose the frame is to be tested at.
 * Not offered: a comparison against the graph's current estimate, depth-along-the-ray statistics, a per-pixel output image.
 * A comparison ends with whatever ends the render (any grid call, a new render) and with the next comparison.  It holds device buffers of
 * its own, freed with the map.  Found by symbol lookup, like pps_map_create; PPS_VERSION was not bumped. */
typedef struct pps_map_compare_plane {   /* one per frame plane k */
  int64_t n_valid, n_new;                /* valid pixels of k; of those, pixels without a view */
  int32_t best_row, best_plane_id;       /* -1, -1: none */
  int64_t best_n, best_agree;
} pps_map_compare_plane;
typedef struct pps_map_compare_row { int64_t n_view, n_unseen; } pps_map_compare_row;   /* one per row of the plane table */
typedef struct pps_map_compare_pair {
  int32_t frame_plane, row, plane_id, reserved;
  int64_t n, n_agree, sum_q, sum_q2;
} pps_map_compare_pair;
typedef struct pps_map_compare_totals {
  int32_t width, height, nplanes, n_rows;
  int64_t n_both, n_frame_only, n_view_only, n_neither, n_bad_id, n_pairs;
  int32_t launches, reserved;            /* kernels of the call */
  double  tol, sec;                      /* device seconds (HIP events) of the compare kernels */
} pps_map_compare_totals;
/* planes ([nplanes], may be NULL): the per-plane records.
 *   PPS_EINVAL  answered on the host before any device work; the map, the view and an earlier comparison stay as they were: NULL m or p,
 *               nplanes outside 1 .. 65, tol NaN, infinite or negative, a context on another device, a run whose width x height is not the
 *               render's
 *   PPS_ESTATE  no render present; no run yet, or a run with the plane-id output off
 *   PPS_ENOMEM  the device has no room for the table or the scratch images; the render stays valid */
int pps_map_compare(pps_map* m, pps_popup* p, int nplanes, double tol, pps_map_compare_plane* planes);
/* pps_map_compare fed host arrays (npx = width * height records each, raster order: what pps_popup_download returns) in place of a run:
 * they are copied to scratch buffers of the map, from there on it IS pps_map_compare.  PPS_EINVAL also for NULL cloud or plane_id and
 * for npx != width * height of the render. */
int pps_debug_map_compare_points(pps_map* m, const pps_point* cloud, const int* plane_id, int64_t npx, int nplanes, double tol,
                                 pps_map_compare_plane* planes);
/* of the last comparison; PPS_ESTATE: no comparison present.  rows: *n = rows in all, the first min(cap, *n) are copied.  pairs: entries
 * [first, first + count) of the pair list; PPS_EINVAL for a range outside [0, n_pairs]. */
int pps_map_compare_info(const pps_map* m, pps_map_compare_totals* out);
int pps_map_compare_rows(pps_map* m, int cap, pps_map_compare_row* out, int* n);
int pps_map_compare_pairs(pps_map* m, int64_t first, int64_t count, pps_map_compare_pair* out);
/* host only, no device, compiled from the header the kernel includes: ONE point against ONE plane.  Returns agree (0 / 1), -1 for a NULL
 * pointer or a plane without a normal. */
int pps_map_compare_point_host(const double abcd[4], const float xyz[3], double tol, double* e, int64_t* q);

#ifdef __cplusplus
}
#endif
#endif /* PPS_H */
