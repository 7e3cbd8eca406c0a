// Host-side pieces shared by the translation units of the quadrature weights, the kernel-level methods, ML-II and predict
// (ssmq_weights.hip, ssmq_kernel_methods.hip, ssmq_ml2.hip, ssmq_predict.hip) and by nothing else.
#pragma once
#include "ssmq_host.h"

namespace ssmq {

// a device allocation that lives as long as the entry point that made it
struct DBuf {
    void *p = nullptr;
    ~DBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hip_fail(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc"); }
    double *d() { return (double *)p; }
};

// polynomial moments under N(0, I) of the Bayes-Sard basis (ssmq_weights.hip)
void poly_moments(int D, int NB, const int32_t *mi, std::vector<double> &px, std::vector<double> &xpx, std::vector<double> &pxpx);

// Fits on one workgroup each, K and its inverse LDS-resident (ML-II: ssmq_ml2.hip, predict: ssmq_predict.hip): the supported
// range (with D <= SSMQ_MAX_DIM) and the argument check their entry points share.  `ok` / `in_range`: the caller's own
// conditions, `more`: what it appends to the range text.
constexpr int kFitMaxN = 128, kFitMaxE = 16;
inline int fit_check(const char *what, int D, int N, int E, int64_t B, double nu, bool ok, bool in_range = true,
                     const char *more = "") {
    if (D < 1 || N < 1 || E < 1 || B < 0 || !(nu == 0.0 || nu > 2.0) || !ok) {
        set_error(std::string(what) + ": bad argument");
        return SSMQ_E_ARG;
    }
    if (D > SSMQ_MAX_DIM || N > kFitMaxN || E > kFitMaxE || B > INT32_MAX || !in_range) {
        set_error(std::string(what) + ": supported range is D <= 16, N <= 128, E <= 16" + more);
        return SSMQ_E_UNSUPPORTED;
    }
    return SSMQ_OK;
}

}  // namespace ssmq
