// cov_facade.cpp -- isam::Covariances of the C++ facade (include/pps_isam.hpp) next to the C-ABI calls it forwards to: a short
// corridor run built like Mapper_mono::processFrame builds its graph, then per node / pair / list one line "F <what> <hex doubles>"
// through Slam::covariances() and one line "C <what> <hex doubles>" through pps_cov_* on the same handle.
// tests/test_gpu_cov_facade.py compares the two bit for bit.
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

int main() {
  try {
    Slam slam;
    Properties prop = slam.properties();
    prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
    slam.set_properties(prop);
    const double pose_var[6] = {0.01, 0.01, 0.01, 0.0004, 0.0004, 0.0004}, plane_var[3] = {0.0025, 0.0025, 0.0025};
    Covariance poseCov = Covariance::diagonal(pose_var, 6), planeCov = Covariance::diagonal(plane_var, 3);
    // world planes: ground z = 0, two side walls, one end wall (unit 4-vectors after normalisation)
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
        if (j == 3 && k < 4) continue;                                   // a landmark that appears later
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
      std::vector<Node*> nodes(planes.begin(), planes.end());
      nodes.insert(nodes.end(), poses.begin(), poses.end());
      for (Node* n : nodes) {
        const MatrixXd M = cov.marginal(std::list<Node*>{n});
        print("F", round ? "marginal2" : "marginal", n->backend_id(), n->backend_id(), M.data(), (size_t)M.rows() * M.cols());
        std::vector<double> out(36); const int id = n->backend_id();
        detail::check(pps_cov_marginals(g, 1, &id, out.data(), nullptr), g, "pps_cov_marginals");
        print("C", round ? "marginal2" : "marginal", id, id, out.data(), (size_t)n->dim() * n->dim());
      }
      Covariances::node_pair_list_t pairs;
      for (int k = 0; k < n_poses; k++) { pairs.push_back(std::make_pair((Node*)poses[k], (Node*)planes[k % 3])); pairs.push_back(std::make_pair((Node*)planes[0], (Node*)poses[k])); }
      for (int k = 1; k < n_poses; k++) pairs.push_back(std::make_pair((Node*)poses[k - 1], (Node*)poses[k]));
      const std::list<MatrixXd> acc = cov.access(pairs);
      std::list<MatrixXd>::const_iterator it = acc.begin();
      for (const std::pair<Node*, Node*>& pr : pairs) {
        print("F", round ? "access2" : "access", pr.first->backend_id(), pr.second->backend_id(), it->data(), (size_t)it->rows() * it->cols());
        std::vector<double> out(36); int in = 0; const int r = pr.first->backend_id(), c = pr.second->backend_id();
        detail::check(pps_cov_access(g, 1, &r, &c, out.data(), nullptr, &in), g, "pps_cov_access");
        if (!in) throw std::runtime_error("pair outside the pattern");
        print("C", round ? "access2" : "access", r, c, out.data(), (size_t)pr.first->dim() * pr.second->dim());
        ++it;
      }
      Covariances::node_lists_t lists;
      lists.push_back(std::list<Node*>{poses[n_poses - 1], planes[0], planes[1], planes[2], planes[3]});
      lists.push_back(std::list<Node*>{planes[1], poses[2]});
      for (const MatrixXd& M : cov.marginal(lists)) print("F", round ? "joint2" : "joint", M.rows(), M.cols(), M.data(), (size_t)M.rows() * M.cols());
      for (const std::list<Node*>& l : lists) {
        std::vector<int> ids; int N = 0;
        for (Node* n : l) { ids.push_back(n->backend_id()); N += n->dim(); }
        std::vector<double> out((size_t)N * N);
        detail::check(pps_cov_joint(g, (int)ids.size(), ids.data(), out.data()), g, "pps_cov_joint");
        print("C", round ? "joint2" : "joint", N, N, out.data(), out.size());
      }
    }
    // a pair outside the pattern is an exception of the facade, with the library's reason
    try {
      slam.covariances().marginal(std::list<Node*>{poses[0], poses[n_poses - 1]});
      printf("X no exception\n");
    } catch (const std::exception& e) { printf("X %s\n", e.what()); }
    for (Factor* f : factors) delete f;
    for (Node* n : poses) delete n;
    for (Node* n : planes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "cov_facade: %s\n", e.what()); return 1; }
  return 0;
}
