// gate_facade.cpp -- Covariances::gate of the C++ facade (include/pps_isam.hpp) next to pps_assoc_gate, which it forwards to: the
// corridor run of tests/cpp/cov_block_facade.cpp, then the last pose's gate of four measurements against all planes -- one line
// "F d2 <M> <L> <hex doubles>" / "F best ..." through Slam::covariances() and one line "C ..." through the C-ABI on the same handle (the
// call the Python binding makes).  tests/test_gpu_gate_facade.py compares the two bit for bit.
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
static void print_best(const char* tag, const char* what, const std::vector<int>& b) {
  printf("%s %s", tag, what);
  for (int v : b) printf(" %d", v);
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
    const Vector4d world[4] = {{{0, 0, 1, 0}}, {{1, 0, 0, 1.5}}, {{-1, 0, 0, 1.6}}, {{0, 1, 0, -9}}};
    std::vector<Plane3d_Node*> planes;
    for (int j = 0; j < 4; j++) { planes.push_back(new Plane3d_Node()); slam.add_node(planes.back()); }
    std::vector<Pose3d_Node*> poses;
    std::vector<Factor*> factors;
    const int n_poses = 9;
    Pose3d last_truth;
    for (int k = 0; k < n_poses; k++) {
      const Pose3d truth(0.02 * (k % 3), 0.4 * k, 1.0, 0.01 * k, 0.0, 0.0);
      last_truth = truth;
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
    // four measurements of the last pose: the planes as seen from its true pose, each nudged a little differently
    std::vector<Plane3d> meas;
    std::vector<Noise> noises;
    for (int j = 0; j < 4; j++) {
      Vector4d v = Plane3d(world[j]).transform_to(last_truth.wTo()).vector();
      v[(j + 1) % 3] += 0.01 * (j + 1); v[3] += 0.02 * j;
      meas.push_back(Plane3d(v)); noises.push_back(planeCov);
    }
    const std::list<Node*> all_planes(planes.begin(), planes.end());
    const std::list<Node*> some{planes[2], planes[0]};
    for (int round = 0; round < 2; round++) {
      // round 1: after an update() the handle holds no valid recovery; gate() recovers by itself (ensure), the C-ABI call follows it
      if (round == 1) slam.update();
      Covariances cov = slam.covariances();
      for (const std::list<Node*>& l : {all_planes, some}) {
        std::vector<int> ids, best, cbest(meas.size(), -7);
        for (Node* n : l) ids.push_back(n->backend_id());
        const MatrixXd M = cov.gate(poses.back(), meas, noises, l, best);
        const MatrixXd M2 = cov.gate(poses.back(), meas, noises, l);
        print("F", "d2", M.rows(), M.cols(), M.data(), (size_t)M.rows() * M.cols());
        print("F", "d2", M2.rows(), M2.cols(), M2.data(), (size_t)M2.rows() * M2.cols());
        print_best("F", "best", best);
        std::vector<double> m4, ut, out(meas.size() * ids.size());
        for (size_t i = 0; i < meas.size(); i++) {
          const Vector4d v = meas[i].vector();
          m4.insert(m4.end(), v.begin(), v.end()); ut.insert(ut.end(), noises[i].sqrtinf_ut().begin(), noises[i].sqrtinf_ut().end());
        }
        detail::check(pps_assoc_gate(g, poses.back()->backend_id(), (int)meas.size(), m4.data(), ut.data(), (int)ids.size(), ids.data(), out.data(), cbest.data()),
                      g, "pps_assoc_gate");
        print("C", "d2", (int)meas.size(), (int)ids.size(), out.data(), out.size());
        print("C", "d2", (int)meas.size(), (int)ids.size(), out.data(), out.size());
        print_best("C", "best", cbest);
      }
    }
    const MatrixXd E = slam.covariances().gate(poses.back(), meas, noises, std::list<Node*>());
    printf("E %d %d\n", E.rows(), E.cols());
    for (Factor* f : factors) delete f;
    for (Node* n : poses) delete n;
    for (Node* n : planes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "gate_facade: %s\n", e.what()); return 1; }
  return 0;
}
