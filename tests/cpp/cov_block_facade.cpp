// cov_block_facade.cpp -- Covariances::block / marginal_any of the C++ facade (include/pps_isam.hpp) next to pps_cov_block, which they
// forward to: the corridor run of tests/cpp/cov_facade.cpp, then per query one line "F <what> <hex doubles>" through Slam::covariances()
// and one line "C <what> <hex doubles>" through the C-ABI on the same handle.  tests/test_gpu_cov_block_facade.py compares the two bit
// for bit, and checks that marginal_any answers for a list of nodes for which marginal still throws.
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

static std::vector<int> ids_of(const std::list<Node*>& l, int* dim) {
  std::vector<int> ids; *dim = 0;
  for (Node* n : l) { ids.push_back(n->backend_id()); *dim += n->dim(); }
  return ids;
}

int main() {
  try {
    Slam slam;
    Properties prop = slam.properties();
    prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
    slam.set_properties(prop);
    const double pose_var[6] = {0.01, 0.01, 0.01, 0.0004, 0.0004, 0.0004}, plane_var[3] = {0.0025, 0.0025, 0.0025};
    Covariance poseCov = Covariance::diagonal(pose_var, 6), planeCov = Covariance::diagonal(plane_var, 3);
    const Vector4d world[4] = {{{0, 0, 1, 0}}, {{1, 0, 0, 1.5}}, {{-1, 0, 0, 1.6}}, {{0, 1, 0, -9}}};
    std::vector<Plane3d_Node*> planes;
    for (int j = 0; j < 4; j++) { planes.push_back(new Plane3d_Node()); slam.add_node(planes.back()); }
    std::vector<Pose3d_Node*> poses;
    std::vector<Factor*> factors;
    const int n_poses = 9;
    for (int k = 0; k < n_poses; k++) {
      const Pose3d truth(0.02 * (k % 3), 0.4 * k, 1.0, 0.01 * k, 0.0, 0.0);
      Pose3d_Node* p = new Pose3d_Node(); slam.add_node(p);
      if (k == 0) factors.push_back(new Pose3d_Factor(p, truth, poseCov));
      else {
        const Pose3d prev(0.02 * ((k - 1) % 3), 0.4 * (k - 1), 1.0, 0.01 * (k - 1), 0.0, 0.0);
        factors.push_back(new Pose3d_Pose3d_Factor(poses.back(), p, truth.ominus(prev), poseCov));
      }
      slam.add_factor(factors.back());
      poses.push_back(p);
      for (int j = 0; j < 4; j++) {
        if (j == 3 && k < 4) continue;
        const Plane3d m = Plane3d(world[j]).transform_to(truth.wTo());
        factors.push_back(new Pose3d_Plane3d_Factor(p, planes[j], m, planeCov));
        slam.add_factor(factors.back());
      }
      if (k == 0) { factors.push_back(new Plane3d_Factor(planes[0], Plane3d(world[0]), planeCov)); slam.add_factor(factors.back()); }
    }
    slam.batch_optimization();
    pps_graph* g = slam.handle();
    for (int round = 0; round < 2; round++) {
      // round 1: after an update() the handle holds no valid recovery; the facade recovers by itself, the C-ABI reads follow it
      if (round == 1) slam.update();
      Covariances cov = slam.covariances();
      const std::list<Node*> ends{poses[0], poses[n_poses - 1]};
      const std::list<Node*> mixed{planes[3], poses[0], planes[1], poses[n_poses - 1], poses[4]};
      const std::list<Node*> all_planes(planes.begin(), planes.end());
      for (const std::list<Node*>& l : {ends, mixed}) {
        int N = 0; const std::vector<int> ids = ids_of(l, &N);
        const MatrixXd M = cov.marginal_any(l);
        print("F", round ? "any2" : "any", M.rows(), M.cols(), M.data(), (size_t)M.rows() * M.cols());
        std::vector<double> out((size_t)N * N);
        detail::check(pps_cov_block(g, (int)ids.size(), ids.data(), 0, nullptr, out.data()), g, "pps_cov_block");
        print("C", round ? "any2" : "any", N, N, out.data(), out.size());
      }
      const std::pair<std::list<Node*>, std::list<Node*> > rect[3] = {{std::list<Node*>{poses[0]}, std::list<Node*>{poses[n_poses - 1]}},
                                                                       {std::list<Node*>{poses[n_poses - 1]}, all_planes}, {mixed, ends}};
      for (const auto& q : rect) {
        int R = 0, Cn = 0; const std::vector<int> r = ids_of(q.first, &R), c = ids_of(q.second, &Cn);
        const MatrixXd M = cov.block(q.first, q.second);
        print("F", round ? "block2" : "block", M.rows(), M.cols(), M.data(), (size_t)M.rows() * M.cols());
        std::vector<double> out((size_t)R * Cn);
        detail::check(pps_cov_block(g, (int)r.size(), r.data(), (int)c.size(), c.data(), out.data()), g, "pps_cov_block");
        print("C", round ? "block2" : "block", R, Cn, out.data(), out.size());
      }
    }
    // the strict form keeps its refusal for the very list marginal_any answers
    try {
      slam.covariances().marginal(std::list<Node*>{poses[0], poses[n_poses - 1]});
      printf("X no exception\n");
    } catch (const std::exception& e) { printf("X %s\n", e.what()); }
    try {
      const MatrixXd M = slam.covariances().marginal_any(std::list<Node*>{poses[0], poses[n_poses - 1]});
      printf("Y %d %d\n", M.rows(), M.cols());
    } catch (const std::exception& e) { printf("Y %s\n", e.what()); }
    for (Factor* f : factors) delete f;
    for (Node* n : poses) delete n;
    for (Node* n : planes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "cov_block_facade: %s\n", e.what()); return 1; }
  return 0;
}
