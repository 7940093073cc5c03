// merge_gate_facade.cpp -- Covariances::merge_gate of the C++ facade (include/pps_isam.hpp) next to pps_merge_gate, which it forwards to.
// argv[1]: a graph as tests/test_gpu_merge_gate_facade.py writes it (hex doubles) --
//   "P tx ty tz qx qy qz qw" / "L a b c d"                       a node with its initial value, in id order
//   "p a | 6 meas | 21 sqrtinf"   "o a b | 6 meas | 21 sqrtinf"   "l a b | 4 meas | 6 sqrtinf"   "q a | 4 meas | 6 sqrtinf"   factors (packed upper triangles)
// The graph is built through the facade, optimised, and the merge gate of all planes (and of a permuted sub-list) is printed once through
// Slam::covariances() ("F ...") and once through the C-ABI on the same handle ("C ...": the call the Python binding makes), d2 as hex doubles.
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void print(const char* tag, int n, const double* d2, const std::vector<int>& best, const std::vector<int>& flat, int count, int not_pd) {
  printf("%s d2 %d", tag, n);
  for (int k = 0; k < n * n; k++) printf(" %a", d2[k]);
  printf("\n%s best", tag);
  for (int v : best) printf(" %d", v);
  printf("\n%s pairs %d", tag, count);
  for (int k = 0; k < 2 * count; k++) printf(" %d", flat[k]);
  printf("\n%s notpd %d\n", tag, not_pd);
}

static SqrtInformation noise_of(const double* ut, int n) {
  std::vector<double> full((size_t)n * n, 0.0);
  int k = 0;
  for (int r = 0; r < n; r++) for (int c = r; c < n; c++) full[(size_t)r * n + c] = ut[k++];
  return SqrtInformation(full.data(), n);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: merge_gate_facade graph.txt\n"); return 2; }
  try {
    Slam slam;
    Properties prop = slam.properties();
    prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
    slam.set_properties(prop);
    std::vector<Node*> nodes;
    std::vector<Plane3d_Node*> planes;
    std::vector<Factor*> factors;
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "merge_gate_facade: cannot open %s\n", argv[1]); return 2; }
    char tag[8];
    while (fscanf(f, "%7s", tag) == 1) {
      auto num = [&](double* v, int n) { for (int k = 0; k < n; k++) if (fscanf(f, "%la", &v[k]) != 1) throw std::runtime_error("bad number"); };
      auto idx = [&]() { int a; if (fscanf(f, "%d", &a) != 1 || a < 0 || a >= (int)nodes.size()) throw std::runtime_error("bad node index"); return a; };
      double m[6], w[21];
      if (!strcmp(tag, "P")) { double tq[7]; num(tq, 7); Pose3d_Node* p = new Pose3d_Node(); slam.add_node(p); p->init(Pose3d::from_tq(tq)); nodes.push_back(p); }
      else if (!strcmp(tag, "L")) {
        Vector4d v; num(v.data(), 4);
        Plane3d_Node* p = new Plane3d_Node(); slam.add_node(p); p->init(Plane3d(v)); nodes.push_back(p); planes.push_back(p);
      }
      else if (!strcmp(tag, "p")) { const int a = idx(); num(m, 6); num(w, 21);
        factors.push_back(new Pose3d_Factor(static_cast<Pose3d_Node*>(nodes[a]), Pose3d(m[0], m[1], m[2], m[3], m[4], m[5]), noise_of(w, 6))); slam.add_factor(factors.back()); }
      else if (!strcmp(tag, "o")) { const int a = idx(), b = idx(); num(m, 6); num(w, 21);
        factors.push_back(new Pose3d_Pose3d_Factor(static_cast<Pose3d_Node*>(nodes[a]), static_cast<Pose3d_Node*>(nodes[b]), Pose3d(m[0], m[1], m[2], m[3], m[4], m[5]), noise_of(w, 6)));
        slam.add_factor(factors.back()); }
      else if (!strcmp(tag, "l")) { const int a = idx(), b = idx(); num(m, 4); num(w, 6);
        factors.push_back(new Pose3d_Plane3d_Factor(static_cast<Pose3d_Node*>(nodes[a]), static_cast<Plane3d_Node*>(nodes[b]), Plane3d(Vector4d{{m[0], m[1], m[2], m[3]}}), noise_of(w, 3)));
        slam.add_factor(factors.back()); }
      else if (!strcmp(tag, "q")) { const int a = idx(); num(m, 4); num(w, 6);
        factors.push_back(new Plane3d_Factor(static_cast<Plane3d_Node*>(nodes[a]), Plane3d(Vector4d{{m[0], m[1], m[2], m[3]}}), noise_of(w, 3))); slam.add_factor(factors.back()); }
      else throw std::runtime_error(std::string("unknown record ") + tag);
    }
    fclose(f);
    slam.batch_optimization();
    pps_graph* g = slam.handle();
    const std::list<Node*> all(planes.begin(), planes.end());
    std::list<Node*> some;
    for (size_t k : {9, 2, 5, 0, 11}) if (k < planes.size()) some.push_back(planes[k]);
    for (int round = 0; round < 2; round++) {
      // round 1: after an update() the handle holds no valid recovery; merge_gate() recovers by itself, the C-ABI call follows it
      if (round == 1) slam.update();
      Covariances cov = slam.covariances();
      for (const std::list<Node*>& l : {all, some}) {
        const double floor_var = round == 0 ? 0.0 : 1e-4;
        const Covariances::MergeGate r = cov.merge_gate(l, floor_var, 7.815);
        std::vector<int> ids, flat;
        for (Node* n : l) ids.push_back(n->backend_id());
        for (const std::pair<int, int>& pr : r.pairs) { flat.push_back(pr.first); flat.push_back(pr.second); }
        const int n = (int)ids.size();
        print("F", n, r.d2.data(), r.best, flat, (int)r.pairs.size(), r.n_not_pd);
        std::vector<double> d2((size_t)n * n, -1.0);
        std::vector<int> best(n, -7), cflat((size_t)n * (n - 1), -7);
        int count = -7, not_pd = -7;
        detail::check(pps_merge_gate(g, n, ids.data(), floor_var, 7.815, d2.data(), best.data(), n * (n - 1) / 2, cflat.data(), &count), g, "pps_merge_gate");
        detail::check(pps_merge_gate_last(g, nullptr, nullptr, &not_pd), g, "pps_merge_gate_last");
        print("C", n, d2.data(), best, cflat, count, not_pd);
      }
    }
    const Covariances::MergeGate one = slam.covariances().merge_gate(std::list<Node*>{planes[0]});
    printf("E %d %d %d %zu\n", one.d2.rows(), one.d2.cols(), one.best[0], one.pairs.size());
    for (Factor* fp : factors) delete fp;
    for (Node* n : nodes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "merge_gate_facade: %s\n", e.what()); return 1; }
  return 0;
}
