// The model shapes the time-loop kernels are instantiated for, once, and the rules by which a pass picks among the instantiations
// of a shape.  Host only: included by the table files (ssmq_filter_fused.hip, ssmq_filter_chunked.hip, ssmq_filter_piped.hip, those of
// the scoring kernels, ...) and by the run-time compiler's host code, never embedded in the text it compiles.
#pragma once
#include <array>
#include <utility>
#include "ssmq_fused.h"
#include "ssmq_host.h"

// One instantiation is ONE(FD, FO, D, Y, N, FORM, TP, SELO, OPT) - the table file's own entry macro.  A shape expands to its BQ,
// t-process BQ and sigma-point kernels ...
#define SSMQ_SHAPE(ONE, FD, FO, D, Y, N, SELO)        \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 0),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 1, SELO, 0),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_SIGMA, 0, SELO, 0)
// ... and a "fast" shape also to the LDL' / unscented-point / reflection-symmetry fast paths of ssmq_apply_small.h (OPT: SSMQ_OPT_*)
#define SSMQ_SHAPE_FAST(ONE, FD, FO, D, Y, N, SELO)   \
    SSMQ_SHAPE(ONE, FD, FO, D, Y, N, SELO),           \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 7),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 0, SELO, 3),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_BQ, 1, SELO, 2),   \
    ONE(FD, FO, D, Y, N, SSMQ_FORM_SIGMA, 0, SELO, 2)

// The groups; X is SSMQ_SHAPE or SSMQ_SHAPE_FAST.  A new model family is one line in one of them.
// scalar UNGM (BASELINE configs[1] and the six filters of the reference's UNGM studies): 2, 3 and 5 points
#define SSMQ_SHAPES_UNGM(X, ONE)                           \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 2, 0), \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 3, 0), \
    X(ONE, SSMQ_F_UNGM_DYN, SSMQ_F_UNGM_MEAS, 1, 1, 5, 0)
// two to four states: unscented (2 D + 1) and spherical-radial (2 D) point sets
#define SSMQ_SHAPES_MID(X, ONE)                                                                                   \
    X(ONE, SSMQ_F_PENDULUM_DYN, SSMQ_F_PENDULUM_MEAS, 2, 1, 5, 0),                                                  \
    X(ONE, SSMQ_F_REENTRY1D_DYN, SSMQ_F_RANGE_MEAS, 3, 1, 7, 0),   /* tests/test_ssinf.py:40-50 of the reference */ \
    X(ONE, SSMQ_F_CV_DYN, SSMQ_F_RADAR2D_MEAS, 4, 2, 9, 0),        /* constant velocity + radar (Student filters) */ \
    X(ONE, SSMQ_F_PENDULUM_DYN, SSMQ_F_PENDULUM_MEAS, 2, 1, 4, 0),                                                  \
    X(ONE, SSMQ_F_REENTRY1D_DYN, SSMQ_F_RANGE_MEAS, 3, 1, 6, 0),                                                    \
    X(ONE, SSMQ_F_CV_DYN, SSMQ_F_RADAR2D_MEAS, 4, 2, 8, 0)
// five or six states (BASELINE configs[2] and configs[3]: 2 000+ vector instructions per step) with unscented points ...
#define SSMQ_SHAPES_HEAVY_UT(X, ONE)                                    \
    X(ONE, SSMQ_F_REENTRY2D_DYN, SSMQ_F_RADAR2D_MEAS, 5, 2, 11, 0),      \
    X(ONE, SSMQ_F_REENTRY2D_BIAS_DYN, SSMQ_F_RADAR2D_MEAS, 6, 2, 13, 0), \
    X(ONE, SSMQ_F_CT_DYN, SSMQ_F_BEARING_MEAS, 5, 4, 11, 1)
// ... and with spherical-radial points (the cubature Kalman filter and every BQ transform built with 'sr')
#define SSMQ_SHAPES_HEAVY_SR(X, ONE)                                    \
    X(ONE, SSMQ_F_REENTRY2D_DYN, SSMQ_F_RADAR2D_MEAS, 5, 2, 10, 0),      \
    X(ONE, SSMQ_F_REENTRY2D_BIAS_DYN, SSMQ_F_RADAR2D_MEAS, 6, 2, 12, 0), \
    X(ONE, SSMQ_F_CT_DYN, SSMQ_F_BEARING_MEAS, 5, 4, 10, 1)

namespace ssmq {

// The OPT values a pass asks its table for, best first, -1 = no such variant for these handles: the fast path BOTH handles qualify
// for - reflection-symmetric weights on top of LDL' and unscented points (7, plain BQ only), LDL' and / or unscented points - and
// the dense kernel.
inline std::array<int, 3> opt_preference(const ssmq_transform *hd, const ssmq_transform *ho) {
    const int both = hd->opt_mask & ho->opt_mask;
    const bool plain = !(hd->tp_nu > 0.0 || hd->form == SSMQ_FORM_SIGMA);
    return {(plain && (both & 7) == 7) ? 7 : -1, both & (plain ? 3 : SSMQ_OPT_UT), 0};
}

// The entry of a dispatch table for a key: entries carry the key as `shape` (a FilterShape, or a type that extends it), null = no
// instantiation.
template <class Entry, size_t N, class Key>
const Entry *find_entry(const Entry (&table)[N], const Key &shape) {
    for (const Entry &e : table)
        if (e.shape == shape) return &e;
    return nullptr;
}

// has_time_table() is what the host goes by, HasTimeTable<> what the kernels are compiled with: the same set of integrands
template <int... F>
constexpr bool time_table_ids_agree(std::integer_sequence<int, F...>) {
    return ((HasTimeTable<F>::value == has_time_table(F)) && ...);
}
static_assert(time_table_ids_agree(std::make_integer_sequence<int, SSMQ_F_USER_FIRST + SSMQ_F_USER_SLOTS>{}),
              "has_time_table() and HasTimeTable<> disagree");

}  // namespace ssmq
