// Kernel-parameter sweep of a BQ filter (ssmq_filter_sweep_dev): the dispatch table of k_filter_sweep<> (ssmq_filter_sweep_kernel.h) -
// the dense BQ-form instantiation of every shape the fused time loop is instantiated for (ssmq_filter_shapes.h).
#include <cstring>
#include "ssmq_filter_sweep_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int N, int FD, int FO, int SELO>
static hipError_t launch_sweep_one(const SweepArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_filter_sweep<D, Y, N, N, FD, FO, SELO>), dim3((unsigned)a.P * (unsigned)a.nblk), dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*sweep_fn)(const SweepArgs &, hipStream_t);
struct SweepEntry {
    FilterShape shape;
    sweep_fn fn;
    const char *name;
};
// a shape of ssmq_filter_shapes.h -> its one entry: the dense kernel of the BQ form
#define SSMQ_SWEEP_SHAPE(ONE, FD, FO, D, Y, N, SELO)                                           \
    {{FD, FO, D, Y, N, N, SSMQ_FORM_BQ, 0, SELO, 0}, &launch_sweep_one<D, Y, N, FD, FO, SELO>, \
     "k_filter_sweep<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO ",SELO=" #SELO ">"}

static const SweepEntry kSweep[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SWEEP_SHAPE, _),
    SSMQ_SHAPES_MID(SSMQ_SWEEP_SHAPE, _),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SWEEP_SHAPE, _),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SWEEP_SHAPE, _),
};
static_assert(sizeof(kSweep) / sizeof(kSweep[0]) == 15, "k_filter_sweep: the BQ form of fifteen shapes");

// shape: BQ form, tp 0, opt 0
const char *find_sweep_kernel(const FilterShape &shape) {
    const SweepEntry *e = find_entry(kSweep, shape);
    return e ? e->name : nullptr;
}

// SSMQ_OK launched, SSMQ_E_UNSUPPORTED no instantiation for this shape (the caller has asked find_sweep_kernel first), or a HIP error
int launch_sweep(const FilterShape &shape, const SweepArgs &a, hipStream_t s) {
    const SweepEntry *e = find_entry(kSweep, shape);
    return e ? hip_fail(e->fn(a, s), e->name) : SSMQ_E_UNSUPPORTED;
}

}  // namespace ssmq
