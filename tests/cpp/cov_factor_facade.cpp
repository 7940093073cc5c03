// cov_factor_facade.cpp -- Covariances::marginal_any / block / gate of the C++ facade (include/pps_isam.hpp) on a graph pps_cov_recover refuses:
// a pose chain with loop closures between distant poses (a front beyond 127 rows: the dense-front form) and four planes.  The facade falls back
// to pps_cov_factor by itself; per query one line "F <what> ..." through Slam::covariances() and one line "C <what> ..." through the C-ABI after
// an explicit pps_cov_factor, compared bit for bit by tests/test_gpu_cov_factor_facade.py.  Then the same on a small band graph, where the "C"
// lines come from pps_cov_recover + the C-ABI: what the facade returned before pps_cov_factor existed.
#include <cmath>
#include <cstdio>
#include <list>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void print(const char* tag, const char* what, int a, int b, const double* v, size_t n) {
  printf("%s %s %d %d", tag, what, a, b);
  for (size_t k = 0; k < n; k++) printf(" %a", v[k]);
  printf("\n");
}

static Pose3d truth_of(int k) { return Pose3d(3.0 * std::sin(0.21 * k), 0.35 * k, 1.0 + 0.05 * (k % 4), 0.02 * k, 0.01 * (k % 5), 0.0); }

static int run(const char* name, int n_poses, int loops_per_pose, bool dense) {
  Slam slam;
  Properties prop = slam.properties();
  prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true; prop.jacobian_mode = PPS_JAC_ANALYTIC;
  slam.set_properties(prop);
  const double pose_var[6] = {0.01, 0.01, 0.01, 0.0004, 0.0004, 0.0004}, plane_var[3] = {0.0025, 0.0025, 0.0025};
  Covariance poseCov = Covariance::diagonal(pose_var, 6), planeCov = Covariance::diagonal(plane_var, 3);
  const Vector4d world[4] = {{{0, 0, 1, 0}}, {{1, 0, 0, 6.5}}, {{-1, 0, 0, 7.0}}, {{0, 1, 0, -30}}};
  std::vector<Plane3d_Node*> planes;
  for (int j = 0; j < 4; j++) { planes.push_back(new Plane3d_Node()); slam.add_node(planes.back()); }
  std::vector<Pose3d_Node*> poses;
  std::vector<Factor*> factors;
  for (int k = 0; k < n_poses; k++) {
    Pose3d_Node* p = new Pose3d_Node(); slam.add_node(p);
    if (k == 0) factors.push_back(new Pose3d_Factor(p, truth_of(0), poseCov));
    else factors.push_back(new Pose3d_Pose3d_Factor(poses.back(), p, truth_of(k).ominus(truth_of(k - 1)), poseCov));
    slam.add_factor(factors.back());
    poses.push_back(p);
    for (int j = 0; j < 4; j++) {
      if ((k + j) % 3 != 0) continue;
      factors.push_back(new Pose3d_Plane3d_Factor(p, planes[j], Plane3d(world[j]).transform_to(truth_of(k).wTo()), planeCov));
      slam.add_factor(factors.back());
    }
    if (k == 0) { factors.push_back(new Plane3d_Factor(planes[0], Plane3d(world[0]), planeCov)); slam.add_factor(factors.back()); }
  }
  unsigned lcg = 12345u;                                   // loop closures: every pose to a few poses far away
  for (int k = 0; k < n_poses; k++)
    for (int l = 0; l < loops_per_pose; l++) {
      lcg = lcg * 1664525u + 1013904223u;
      const int j = (int)((lcg >> 8) % (unsigned)n_poses);
      if (j + 2 > k) continue;
      factors.push_back(new Pose3d_Pose3d_Factor(poses[j], poses[k], truth_of(k).ominus(truth_of(j)), poseCov));
      slam.add_factor(factors.back());
    }
  slam.batch_optimization();
  pps_graph* g = slam.handle();
  pps_stats st; detail::check(pps_get_stats(g, &st), g, "pps_get_stats");
  printf("S %s %d\n", name, st.max_front);
  const int rec = pps_cov_recover(g);
  printf("R %s %d %s\n", name, rec, rec == PPS_OK ? "" : pps_last_error(g));
  // ends whatever the handle held without moving the estimate (a pps_update would take a step: the two sides would differ by it)
  detail::check(pps_set_cost_function(g, PPS_COST_NONE, 1.0), g, "pps_set_cost_function");
  Covariances cov = slam.covariances();
  const std::list<Node*> mixed{planes[3], poses[0], planes[1], poses[n_poses - 1], poses[n_poses / 2]};
  const std::list<Node*> ends{poses[0], poses[n_poses - 1]};
  const std::list<Node*> all_planes(planes.begin(), planes.end());
  std::vector<Plane3d> meas; std::vector<Noise> noises;
  for (int j = 0; j < 3; j++) {
    Vector4d v = Plane3d(world[j]).transform_to(truth_of(n_poses - 1).wTo()).vector();
    v[(j + 1) % 3] += 0.01 * (j + 1); v[3] += 0.02 * j;
    meas.push_back(Plane3d(v)); noises.push_back(planeCov);
  }
  std::vector<int> best;
  const MatrixXd A = cov.marginal_any(mixed), B = cov.block(ends, mixed), D = cov.gate(poses.back(), meas, noises, all_planes, best);
  print("F", "any", A.rows(), A.cols(), A.data(), (size_t)A.rows() * A.cols());
  print("F", "block", B.rows(), B.cols(), B.data(), (size_t)B.rows() * B.cols());
  print("F", "d2", D.rows(), D.cols(), D.data(), (size_t)D.rows() * D.cols());
  printf("F best"); for (int b : best) printf(" %d", b); printf("\n");
  // the C-ABI, from nothing again, at the same estimate
  detail::check(pps_set_cost_function(g, PPS_COST_NONE, 1.0), g, "pps_set_cost_function");
  if (dense) detail::check(pps_cov_factor(g), g, "pps_cov_factor"); else detail::check(pps_cov_recover(g), g, "pps_cov_recover");
  auto ids_of = [](const std::list<Node*>& l, int* dim) { std::vector<int> ids; *dim = 0; for (Node* n : l) { ids.push_back(n->backend_id()); *dim += n->dim(); } return ids; };
  int N = 0, R = 0, Np = 0;
  const std::vector<int> im = ids_of(mixed, &N), ie = ids_of(ends, &R), ip = ids_of(all_planes, &Np);
  std::vector<double> a((size_t)N * N), b((size_t)R * N), d2(meas.size() * ip.size()), m4, ut;
  std::vector<int> cbest(meas.size(), -7);
  detail::check(pps_cov_block(g, (int)im.size(), im.data(), 0, nullptr, a.data()), g, "pps_cov_block");
  detail::check(pps_cov_block(g, (int)ie.size(), ie.data(), (int)im.size(), im.data(), b.data()), g, "pps_cov_block");
  for (size_t i = 0; i < meas.size(); i++) {
    const Vector4d v = meas[i].vector();
    m4.insert(m4.end(), v.begin(), v.end()); ut.insert(ut.end(), noises[i].sqrtinf_ut().begin(), noises[i].sqrtinf_ut().end());
  }
  detail::check(pps_assoc_gate(g, poses.back()->backend_id(), (int)meas.size(), m4.data(), ut.data(), (int)ip.size(), ip.data(), d2.data(), cbest.data()), g, "pps_assoc_gate");
  print("C", "any", N, N, a.data(), a.size());
  print("C", "block", R, N, b.data(), b.size());
  print("C", "d2", (int)meas.size(), (int)ip.size(), d2.data(), d2.size());
  printf("C best"); for (int x : cbest) printf(" %d", x); printf("\n");
  // the strict forms keep their contract: on the dense-front graph they throw with the library's text
  try { slam.covariances().marginal(std::list<Node*>{poses[0]}); printf("X %s ok\n", name); }
  catch (const std::exception& e) { printf("X %s %s\n", name, e.what()); }
  for (Factor* f : factors) delete f;
  for (Node* n : poses) delete n;
  for (Node* n : planes) delete n;
  return 0;
}

int main() {
  try {
    run("dense", 60, 8, true);
    run("band", 9, 0, false);
  } catch (const std::exception& e) { fprintf(stderr, "cov_factor_facade: %s\n", e.what()); return 1; }
  return 0;
}
