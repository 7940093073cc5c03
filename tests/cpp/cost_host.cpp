// csrc/pps_cost.h compiled for the host (g++, no HIP): rho, phi = sign sqrt(rho) and phi' of the three cost kinds, for tests/test_host_robust.py
#include "pps_cost.h"

extern "C" {
double cost_host_rho(int kind, double b, double d) { return pps::cost_rho(pps::make_cost(kind, b), d); }
double cost_host_phi(int kind, double b, double d) { return pps::cost_phi(pps::make_cost(kind, b), d); }
double cost_host_dphi(int kind, double b, double d) { return pps::cost_dphi(pps::make_cost(kind, b), d); }
// robustify<3> as the kernels call it: in place on a whitened residual
void cost_host_robustify3(int kind, double b, double* r) { pps::robustify<3>(pps::make_cost(kind, b), r); }
}
