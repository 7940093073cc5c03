// robust_facade.cpp -- Slam::set_cost_function of the C++ facade (include/pps_isam.hpp) next to the C-ABI calls it forwards to: a short
// corridor run with one grossly wrong plane measurement; per cost function one line "F <kind> <iterations> <chi2 as hex double>" from the
// facade (set_cost_function, batch_optimization, chi2 on one Slam) and one line "C ..." from pps_set_cost_function / pps_batch_optimize /
// pps_chi2 on the handle of a second, identically built Slam.  tests/test_gpu_robust.py compares the two bit for bit.
#include <cstdio>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void build(Slam& slam, std::vector<Node*>& keep, std::vector<Factor*>& factors) {
  Properties prop = slam.properties();
  prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
  slam.set_properties(prop);
  const double pose_var[6] = {0.01, 0.01, 0.01, 0.0004, 0.0004, 0.0004}, plane_var[3] = {0.0025, 0.0025, 0.0025};
  Covariance poseCov = Covariance::diagonal(pose_var, 6), planeCov = Covariance::diagonal(plane_var, 3);
  const Vector4d world[3] = {{{0, 0, 1, 0}}, {{1, 0, 0, 1.5}}, {{-1, 0, 0, 1.6}}};
  std::vector<Plane3d_Node*> planes;
  for (int j = 0; j < 3; j++) { planes.push_back(new Plane3d_Node()); slam.add_node(planes.back()); keep.push_back(planes.back()); }
  Pose3d_Node* last = nullptr;
  for (int k = 0; k < 7; k++) {
    const Pose3d truth(0.02 * (k % 3), 0.4 * k, 1.0, 0.01 * k, 0.0, 0.0);
    Pose3d_Node* p = new Pose3d_Node(); slam.add_node(p); keep.push_back(p);
    if (k == 0) factors.push_back(new Pose3d_Factor(p, truth, poseCov));
    else {
      const Pose3d prev(0.02 * ((k - 1) % 3), 0.4 * (k - 1), 1.0, 0.01 * (k - 1), 0.0, 0.0);
      factors.push_back(new Pose3d_Pose3d_Factor(last, p, truth.ominus(prev), poseCov));
    }
    slam.add_factor(factors.back());
    last = p;
    for (int j = 0; j < 3; j++) {
      Vector4d w = world[j];
      if (k == 4 && j == 1) w = Vector4d{{0.6, 0.8, 0, 2.5}};          // the outlier: another wall altogether
      factors.push_back(new Pose3d_Plane3d_Factor(p, planes[j], Plane3d(w).transform_to(truth.wTo()), planeCov));
      slam.add_factor(factors.back());
    }
    if (k == 0) { factors.push_back(new Plane3d_Factor(planes[0], Plane3d(world[0]), planeCov)); slam.add_factor(factors.back()); }
  }
}

int main() {
  try {
    const pps::Cost kinds[4] = {pps::Cost::PseudoHuber, pps::Cost::Huber, pps::Cost::Cauchy, pps::Cost::None};
    const double bs[4] = {0.5, 0.8, 1.5, 1.0};
    for (int c = 0; c < 4; c++) {
      std::vector<Node*> n1, n2; std::vector<Factor*> f1, f2;
      Slam a, b;
      build(a, n1, f1); build(b, n2, f2);
      a.set_cost_function(kinds[c], bs[c]);
      int kind = -1; double bb = 0;
      if (pps_get_cost_function(a.handle(), &kind, &bb) != PPS_OK || kind != static_cast<int>(kinds[c])) { fprintf(stderr, "facade did not set the cost\n"); return 2; }
      const int it = a.batch_optimization();
      const double chi = a.chi2();
      printf("F %d %d %a\n", kind, it, chi);
      int it2 = 0; double chi2 = 0;
      if (pps_set_cost_function(b.handle(), static_cast<int>(kinds[c]), bs[c]) != PPS_OK || pps_batch_optimize(b.handle(), &it2) != PPS_OK ||
          pps_chi2(b.handle(), &chi2) != PPS_OK) { fprintf(stderr, "C ABI: %s\n", pps_last_error(b.handle())); return 3; }
      printf("C %d %d %a\n", kind, it2, chi2);
      for (Factor* f : f1) delete f;
      for (Factor* f : f2) delete f;
      for (Node* n : n1) delete n;
      for (Node* n : n2) delete n;
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
