// factor_gate_facade.cpp -- Covariances::factor_gate of the C++ facade (include/pps_isam.hpp) next to pps_factor_gate, which it forwards to.
// argv[1]: a graph in the format of tests/cpp/merge_gate_facade.cpp (hex doubles) --
//   "P tx ty tz qx qy qz qw" / "L a b c d"                       a node with its initial value, in id order
//   "p a | 6 meas | 21 sqrtinf"   "o a b | 6 meas | 21 sqrtinf"   "l a b | 4 meas | 6 sqrtinf"   "q a | 4 meas | 6 sqrtinf"   factors (packed upper triangles)
// The graph is built through the facade and optimised; the gate of all factors (no list) and of a sub-list with a repeated factor is printed
// once through Slam::covariances() ("F ...") and once through the C-ABI on the same handle ("C ...": the call the Python binding makes), d2 and
// the leverages as hex doubles.  Round 0 starts without a recovery, round 1 after an update(): factor_gate() recovers by itself both times.
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void print(const char* tag, const std::vector<double>& d2, const std::vector<double>& lev, const std::vector<int>& flagged, int untestable) {
  printf("%s d2 %zu", tag, d2.size());
  for (double v : d2) printf(" %a", v);
  printf("\n%s lev", tag);
  for (double v : lev) printf(" %a", v);
  printf("\n%s flagged %zu", tag, flagged.size());
  for (int v : flagged) printf(" %d", v);
  printf("\n%s untestable %d\n", tag, untestable);
}

static SqrtInformation noise_of(const double* ut, int n) {
  std::vector<double> full((size_t)n * n, 0.0);
  int k = 0;
  for (int r = 0; r < n; r++) for (int c = r; c < n; c++) full[(size_t)r * n + c] = ut[k++];
  return SqrtInformation(full.data(), n);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: factor_gate_facade graph.txt\n"); return 2; }
  try {
    Slam slam;
    Properties prop = slam.properties();
    prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
    slam.set_properties(prop);
    std::vector<Node*> nodes;
    std::vector<Factor*> factors;
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "factor_gate_facade: cannot open %s\n", argv[1]); return 2; }
    char tag[8];
    while (fscanf(f, "%7s", tag) == 1) {
      auto num = [&](double* v, int n) { for (int k = 0; k < n; k++) if (fscanf(f, "%la", &v[k]) != 1) throw std::runtime_error("bad number"); };
      auto idx = [&]() { int a; if (fscanf(f, "%d", &a) != 1 || a < 0 || a >= (int)nodes.size()) throw std::runtime_error("bad node index"); return a; };
      double m[6], w[21];
      if (!strcmp(tag, "P")) { double tq[7]; num(tq, 7); Pose3d_Node* p = new Pose3d_Node(); slam.add_node(p); p->init(Pose3d::from_tq(tq)); nodes.push_back(p); }
      else if (!strcmp(tag, "L")) { Vector4d v; num(v.data(), 4); Plane3d_Node* p = new Plane3d_Node(); slam.add_node(p); p->init(Plane3d(v)); nodes.push_back(p); }
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
    std::list<Factor*> some;
    for (size_t k : {40, 3, 17, 3, 0, 200}) if (k < factors.size()) some.push_back(factors[k]);
    for (int round = 0; round < 2; round++) {
      if (round == 1) slam.update();
      Covariances cov = slam.covariances();
      for (const std::list<Factor*>& l : {std::list<Factor*>(), some}) {
        const Covariances::FactorGate r = cov.factor_gate(l, 7.815, 12.592);
        print("F", r.d2, r.leverage, r.flagged, r.n_untestable);
        std::vector<int> ids;
        for (Factor* fp : l) ids.push_back(fp->backend_id());
        const int n = l.empty() ? (int)factors.size() : (int)ids.size();
        std::vector<double> d2((size_t)n, -1.0), lev((size_t)n, -1.0);
        std::vector<int> flagged((size_t)n, -7);
        int count = -7, untestable = -7;
        detail::check(pps_factor_gate(g, n, l.empty() ? nullptr : ids.data(), 7.815, 12.592, d2.data(), lev.data(), n, flagged.data(), &count), g, "pps_factor_gate");
        detail::check(pps_factor_gate_last(g, nullptr, nullptr, &untestable), g, "pps_factor_gate_last");
        flagged.resize((size_t)count);
        print("C", d2, lev, flagged, untestable);
      }
    }
    for (Factor* fp : factors) delete fp;
    for (Node* n : nodes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "factor_gate_facade: %s\n", e.what()); return 1; }
  return 0;
}
