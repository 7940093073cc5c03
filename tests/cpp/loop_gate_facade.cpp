// loop_gate_facade.cpp -- Covariances::loop_gate of the C++ facade (include/pps_isam.hpp) next to pps_loop_gate, which it forwards to.
// argv[1]: a graph as tests/test_gpu_loop_gate_facade.py writes it (hex doubles), the records of tests/cpp/merge_gate_facade.cpp --
//   "P tx ty tz qx qy qz qw" / "L a b c d"                       a node with its initial value, in id order
//   "p a | 6 meas | 21 sqrtinf"   "o a b | 6 meas | 21 sqrtinf"   "l a b | 4 meas | 6 sqrtinf"   "q a | 4 meas | 6 sqrtinf"   factors (packed upper triangles)
// -- and, after the graph, "c a b | 6 meas | 21 sqrtinf": a candidate loop closure between poses a and b.
// The graph is built through the facade and optimised; the loop gate of all candidates (and of a reversed sub-list) is printed once through
// Slam::covariances() ("F ...") and once through the C-ABI on the same handle ("C ...": the call the Python binding makes), d2 as hex doubles.
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "pps_isam.hpp"

using namespace isam;

static void print(const char* tag, const std::vector<double>& d2, const std::vector<int>& accepted, int not_pd) {
  printf("%s d2 %zu", tag, d2.size());
  for (double v : d2) printf(" %a", v);
  printf("\n%s accepted %zu", tag, accepted.size());
  for (int v : accepted) printf(" %d", v);
  printf("\n%s notpd %d\n", tag, not_pd);
}

static SqrtInformation noise_of(const double* ut, int n) {
  std::vector<double> full((size_t)n * n, 0.0);
  int k = 0;
  for (int r = 0; r < n; r++) for (int c = r; c < n; c++) full[(size_t)r * n + c] = ut[k++];
  return SqrtInformation(full.data(), n);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: loop_gate_facade graph.txt\n"); return 2; }
  try {
    Slam slam;
    Properties prop = slam.properties();
    prop.method = LEVENBERG_MARQUARDT; prop.mod_batch = 1; prop.quiet = true;
    slam.set_properties(prop);
    std::vector<Node*> nodes;
    std::vector<Factor*> factors;
    std::vector<Covariances::LoopCandidate> cands;
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "loop_gate_facade: cannot open %s\n", argv[1]); return 2; }
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
      else if (!strcmp(tag, "c")) { const int a = idx(), b = idx(); num(m, 6); num(w, 21);
        cands.push_back(Covariances::LoopCandidate{static_cast<Pose3d_Node*>(nodes[a]), static_cast<Pose3d_Node*>(nodes[b]), Pose3d(m[0], m[1], m[2], m[3], m[4], m[5]), noise_of(w, 6)}); }
      else throw std::runtime_error(std::string("unknown record ") + tag);
    }
    fclose(f);
    slam.batch_optimization();
    pps_graph* g = slam.handle();
    std::vector<Covariances::LoopCandidate> some;
    for (size_t k = cands.size(); k-- > 0;) if (k % 2 == 0) some.push_back(cands[k]);
    for (int round = 0; round < 2; round++) {
      // round 1: after an update() the handle holds no valid recovery; loop_gate() recovers by itself, the C-ABI call follows it
      if (round == 1) slam.update();
      Covariances cov = slam.covariances();
      for (const std::vector<Covariances::LoopCandidate>& l : {cands, some}) {
        const double thr = round == 0 ? 12.592 : 3.0;
        const Covariances::LoopGate r = cov.loop_gate(l, thr);
        print("F", r.d2, r.accepted, r.n_not_pd);
        const int n = (int)l.size();
        std::vector<int> ia, ib, acc((size_t)n, -7);
        std::vector<double> m6, ut, d2((size_t)n, -1.0);
        for (const Covariances::LoopCandidate& c : l) {
          ia.push_back(c.a->backend_id()); ib.push_back(c.b->backend_id());
          const Vector6d v = c.measure.vector();
          m6.insert(m6.end(), v.begin(), v.end());
          ut.insert(ut.end(), c.noise.sqrtinf_ut().begin(), c.noise.sqrtinf_ut().end());
        }
        int count = -7, not_pd = -7;
        detail::check(pps_loop_gate(g, n, ia.data(), ib.data(), m6.data(), ut.data(), thr, d2.data(), nullptr, n, acc.data(), &count), g, "pps_loop_gate");
        detail::check(pps_loop_gate_last(g, nullptr, nullptr, &not_pd), g, "pps_loop_gate_last");
        acc.resize((size_t)count);
        print("C", d2, acc, not_pd);
      }
    }
    const Covariances::LoopGate none = slam.covariances().loop_gate(std::vector<Covariances::LoopCandidate>());
    printf("E %zu %zu %d\n", none.d2.size(), none.accepted.size(), none.n_not_pd);
    for (Factor* fp : factors) delete fp;
    for (Node* n : nodes) delete n;
  } catch (const std::exception& e) { fprintf(stderr, "loop_gate_facade: %s\n", e.what()); return 1; }
  return 0;
}
