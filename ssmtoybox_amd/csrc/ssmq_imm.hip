// Interacting multiple-model filter over noise modes (ssmq_filter_imm_dev): the dispatch table of k_imm_loop<> (ssmq_imm_kernel.h) -
// the dense BQ, t-process BQ and sigma-point instantiation of every shape the fused time loop is instantiated for
// (ssmq_filter_shapes.h), in a translation unit of its own.
#include <cstring>
#include "ssmq_imm_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

// One workgroup per 64 trajectories, M waves each; the LDS of the M slots is sized at launch and the kernel's limit raised to what
// kImmMaxModes modes need (116 KiB at D = 6), once per device binding of the calling thread.
template <int D, int Y, int N, int FD, int FO, int SELO, int FORM, int TP>
static int launch_imm_one(const ImmArgs &a, hipStream_t s) {
    static thread_local unsigned attr_epoch = ~0u;
    const void *kernel = (const void *)k_imm_loop<D, Y, N, N, FD, FO, SELO, FORM, TP>;
    if (int rc = set_max_dynamic_lds(attr_epoch, {kernel}, imm_lds_bytes(D, kImmMaxModes))) return rc;
    hipLaunchKernelGGL((k_imm_loop<D, Y, N, N, FD, FO, SELO, FORM, TP>), dim3((unsigned)(a.ld / kSmallBlock)), dim3(kSmallBlock * (unsigned)a.M),
                       imm_lds_bytes(D, a.M), s, a);
    return hip_fail(hipGetLastError(), "k_imm_loop");
}

typedef int (*imm_fn)(const ImmArgs &, hipStream_t);
struct ImmEntry {
    FilterShape shape;
    imm_fn fn;
    const char *name;
};
// an instantiation of SSMQ_SHAPE (ssmq_filter_shapes.h: OPT = 0, the dense kernel of the form) -> its entry
#define SSMQ_IMM_ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT)                                      \
    {{FD, FO, D, Y, N, N, FORM, TP, SELO, OPT}, &launch_imm_one<D, Y, N, FD, FO, SELO, FORM, TP>, \
     "k_imm_loop<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO ",SELO=" #SELO "," #FORM ",TP=" #TP ">"}

static const ImmEntry kImm[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SHAPE, SSMQ_IMM_ONE),
    SSMQ_SHAPES_MID(SSMQ_SHAPE, SSMQ_IMM_ONE),
    SSMQ_SHAPES_HEAVY_UT(SSMQ_SHAPE, SSMQ_IMM_ONE),
    SSMQ_SHAPES_HEAVY_SR(SSMQ_SHAPE, SSMQ_IMM_ONE),
};
static_assert(sizeof(kImm) / sizeof(kImm[0]) == 45, "k_imm_loop: three forms of fifteen shapes");
static_assert(imm_lds_bytes(6, kImmMaxModes) <= 160 * 1024 - 64, "k_imm_loop: the slots of eight modes at D = 6 fit the LDS of a CU");

// shape.opt is 0: the dense kernel of the form
const char *find_imm_kernel(const FilterShape &shape) {
    const ImmEntry *e = find_entry(kImm, shape);
    return e ? e->name : nullptr;
}

// SSMQ_OK launched, SSMQ_E_UNSUPPORTED no instantiation for this shape (the caller has asked find_imm_kernel first), or a HIP error.
// a.M is 1 .. kImmMaxModes, a.B >= 1 and a.ld a multiple of 64: the caller has checked.
int launch_imm(const FilterShape &shape, const ImmArgs &a, hipStream_t s) {
    if (a.M < 1 || a.M > kImmMaxModes || a.B < 1 || a.ld % kSmallBlock != 0 || a.ld < a.B) return SSMQ_E_ARG;
    const ImmEntry *e = find_entry(kImm, shape);
    return e ? e->fn(a, s) : SSMQ_E_UNSUPPORTED;
}

}  // namespace ssmq
