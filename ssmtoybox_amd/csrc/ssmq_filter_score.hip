// Scoring recursion of the t-process and Studentian filters (ssmq_student_scores_dev, ssmq_filter_sweep_t_dev): the dispatch table of
// k_filter_score<> (ssmq_filter_score_kernel.h).  Per shape three instantiations: the t-process BQ form with the Gaussian and with the
// Studentian recursion, and the sigma-point form with the Studentian recursion.  Shapes: the scalar and the two- to four-state groups
// of ssmq_filter_shapes.h - every instantiation within 256 registers and without scratch; the five- and six-state
// t-process passes do not fit one lane (they live in k_filter_wsplit for that reason) and are refused.
#include <cstring>
#include "ssmq_filter_score_kernel.h"
#include "ssmq_filter_shapes.h"

namespace ssmq {

template <int D, int Y, int N, int FD, int FO, int FORM, int TP, int SELO, int STU>
static hipError_t launch_score_one(const ScoreArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_filter_score<D, Y, N, N, FD, FO, FORM, TP, SELO, STU>), dim3((unsigned)(a.ld / kSmallBlock), (unsigned)a.P), dim3(kSmallBlock), 0, s, a);
    return hipGetLastError();
}

typedef hipError_t (*score_fn)(const ScoreArgs &, hipStream_t);
struct ScoreEntry {
    ScoreShape shape;
    score_fn fn;
    const char *name;
};
#define SSMQ_SCORE_ONE(FD, FO, D, Y, N, SELO, FORM, TP, STU)                                               \
    {{{FD, FO, D, Y, N, N, FORM, TP, SELO, 0}, STU}, &launch_score_one<D, Y, N, FD, FO, FORM, TP, SELO, STU>, \
     "k_filter_score<D=" #D ",Y=" #Y ",ND=" #N ",NO=" #N "," #FD "," #FO "," #FORM ",TP=" #TP ",SELO=" #SELO ",STU=" #STU ">"}
// a shape of ssmq_filter_shapes.h -> its three entries
#define SSMQ_SCORE_SHAPE(ONE, FD, FO, D, Y, N, SELO)              \
    SSMQ_SCORE_ONE(FD, FO, D, Y, N, SELO, SSMQ_FORM_BQ, 1, 0),    \
    SSMQ_SCORE_ONE(FD, FO, D, Y, N, SELO, SSMQ_FORM_BQ, 1, 1),    \
    SSMQ_SCORE_ONE(FD, FO, D, Y, N, SELO, SSMQ_FORM_SIGMA, 0, 1)

static const ScoreEntry kScore[] = {
    SSMQ_SHAPES_UNGM(SSMQ_SCORE_SHAPE, _),
    SSMQ_SHAPES_MID(SSMQ_SCORE_SHAPE, _),
};
static_assert(sizeof(kScore) / sizeof(kScore[0]) == 27, "k_filter_score: three instantiations of nine shapes");

// shape.opt is 0: the dense kernel of the form
const char *find_score_kernel(const ScoreShape &shape) {
    const ScoreEntry *e = find_entry(kScore, shape);
    return e ? e->name : nullptr;
}

// SSMQ_OK launched, SSMQ_E_UNSUPPORTED no instantiation for this shape (the caller has asked find_score_kernel first), or a HIP error
int launch_score(const ScoreShape &shape, const ScoreArgs &a, hipStream_t s) {
    const ScoreEntry *e = find_entry(kScore, shape);
    return e ? hip_fail(e->fn(a, s), e->name) : SSMQ_E_UNSUPPORTED;
}

}  // namespace ssmq
