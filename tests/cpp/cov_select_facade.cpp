// cov_select_facade.cpp -- Covariances::select of the C++ facade (include/pps_isam.hpp) on the loop-closure graph of cov_factor_facade.cpp: a pose
// chain with loop closures between distant poses (a front beyond 127 rows: the dense-front form) and four planes.  marginal() throws before
// select(); after it marginal({pose}), marginal({pose, plane}) of a factor-joined pair and access() are printed next to marginal_any() / block()
// of the same handle -- the column solves on the same factor -- as hex doubles, compared by tests/test_gpu_cov_select_facade.py; after
// add_factor they throw again.
#include <cmath>
#include <cstdio>
#include <list>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void print(const char* tag, const char* what, const MatrixXd& M) {
  printf("%s %s %d %d", tag, what, (int)M.rows(), (int)M.cols());
  for (size_t k = 0; k < (size_t)M.rows() * M.cols(); k++) printf(" %a", M.data()[k]);
  printf("\n");
}

static Pose3d truth_of(int k) { return Pose3d(3.0 * std::sin(0.21 * k), 0.35 * k, 1.0 + 0.05 * (k % 4), 0.02 * k, 0.01 * (k % 5), 0.0); }

int main() {
  try {
    const int n_poses = 60, loops_per_pose = 8;
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
    int joined_pose = -1, joined_plane = -1;
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
        if (k == n_poses / 2 || (joined_pose < 0 && k > n_poses / 2)) { joined_pose = k; joined_plane = j; }
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
    printf("S front %d\n", st.max_front);
    Covariances cov = slam.covariances();
    const std::list<Node*> one{poses[joined_pose]}, two{poses[joined_pose], planes[joined_plane]};
    try { cov.marginal(one); printf("X before ok\n"); }
    catch (const std::exception& e) { printf("X before %s\n", e.what()); }
    cov.select();
    print("F", "one", cov.marginal(one));
    print("F", "two", cov.marginal(two));
    Covariances::node_pair_list_t pairs;
    pairs.push_back(std::make_pair((Node*)poses[joined_pose], (Node*)planes[joined_plane]));
    pairs.push_back(std::make_pair((Node*)planes[joined_plane], (Node*)poses[joined_pose]));
    std::list<MatrixXd> acc = cov.access(pairs);
    int k = 0;
    for (const MatrixXd& M : acc) print("F", k++ == 0 ? "pose_plane" : "plane_pose", M);
    print("C", "one", cov.marginal_any(one));
    print("C", "two", cov.marginal_any(two));
    print("C", "pose_plane", cov.block(one, std::list<Node*>{planes[joined_plane]}));
    print("C", "plane_pose", cov.block(std::list<Node*>{planes[joined_plane]}, one));
    // any change of the graph ends the selection: the strict forms throw again
    factors.push_back(new Plane3d_Factor(planes[1], Plane3d(world[1]), planeCov)); slam.add_factor(factors.back());
    try { slam.covariances().marginal(one); printf("X after ok\n"); }
    catch (const std::exception& e) { printf("X after %s\n", e.what()); }
    for (Factor* f : factors) delete f;
    for (Node* n : poses) delete n;
    for (Node* n : planes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "cov_select_facade: %s\n", e.what()); return 1; }
  return 0;
}
