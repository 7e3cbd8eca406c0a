// Noise sweep of a Gaussian filter (ssmq_filter_noise_sweep_dev): the dispatch table of k_noise_sweep<> (ssmq_noise_sweep_kernel.h) -
// the dense BQ, t-process BQ and sigma-point instantiation of every shape the fused time loop is instantiated for
// (ssmq_filter_shapes.h), in a translation unit of its own.
#include <cstring>
#include "ssmq_noise_sweep_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int N, int FD, int FO, int SELO, int FORM, int TP>
static hipError_t launch_noise_sweep_one(const NoiseSweepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_noise_sweep<D, Y, N, N, FD, FO, SELO, FORM, TP>), dim3((unsigned)a.P * (unsigned)a.nblk), dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*noise_sweep_fn)(const NoiseSweepArgs &, hipStream_t);
struct NoiseSweepEntry {
    FilterShape shape;
    noise_sweep_fn fn;
    const char *name;
};
// an instantiation of SSMQ_SHAPE (ssmq_filter_shapes.h: OPT = 0, the dense kernel of the form) -> its entry
#define SSMQ_NOISE_SWEEP_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                      \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT}, &launch_noise_sweep_one<D, Y, N, FD, FO, SELO, FORM, TP>, \
     "k_noise_sweep<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO ",SELO=" #SELO "," #FORM ",TP=" #TP ">"}

static const NoiseSweepEntry kNoiseSweep[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_NOISE_SWEEP_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_NOISE_SWEEP_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_NOISE_SWEEP_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_NOISE_SWEEP_ONE),
};
static_assert(sizeof(kNoiseSweep) / sizeof(kNoiseSweep[0]) == 45, "k_noise_sweep: three forms of fifteen shapes");

// shape.opt is 0: the dense kernel of the form
const char *find_noise_sweep_kernel(const FilterShape &shape) {
    const NoiseSweepEntry *e = find_entry(kNoiseSweep, shape);
    return e ? e->name : nullptr;
}

// SSMQ_OK launched, SSMQ_E_UNSUPPORTED no instantiation for this shape (the caller has asked find_noise_sweep_kernel first), or a HIP error
int launch_noise_sweep(const FilterShape &shape, const NoiseSweepArgs &a, hipStream_t s) {
    const NoiseSweepEntry *e = find_entry(kNoiseSweep, shape);
    return e ? hip_fail(e->fn(a, s), e->name) : SSMQ_E_UNSUPPORTED;
}

}  // namespace ssmq
