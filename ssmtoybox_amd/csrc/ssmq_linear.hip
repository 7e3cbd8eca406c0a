// The linearisation and the Taylor-GPQD transform for the built-in models: the instantiations of k_linearize<DT, ET> and
// k_taylor_gpqd<DT, ET> (ssmq_jacobian_kernel.h, where the transforms are described) and the one launcher of both forms.  The
// Jacobian is the model's own (ssmq_device.h: jac_integrand - the seven models whose dyn_fcn_dx / meas_fcn_dx the reference
// implements and the three tracking models: coordinated turn, radar, bearings); a user model's kernels are compiled for it at run
// time (ssmq_rtc.hip).
#include "ssmq_device.h"
#include "ssmq_host.h"
#include "ssmq_math.h"
// (the run-time-size instantiations <0, 0> cannot unroll the loops of the front end and the item bodies: no warning for that)
#pragma clang diagnostic ignored "-Wpass-failed"
#include "ssmq_jacobian_kernel.h"

namespace ssmq {

int refuse_taylor_gpqd(const char *what) {
    set_error(std::string("the Taylor-GPQD transform (k_taylor_gpqd) has neither points nor weights: not implemented for ") + what);
    return SSMQ_E_UNSUPPORTED;
}

template <bool LIN, int DT, int ET>
static void launch_shape(const TaylorGpqdArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)((a.B + 255) / 256)), block(256);
    if constexpr (LIN) hipLaunchKernelGGL((k_linearize<DT, ET>), grid, block, 0, s, static_cast<const LinArgs &>(a));
    else hipLaunchKernelGGL((k_taylor_gpqd<DT, ET>), grid, block, 0, s, a);
}
// register-resident bodies for the (D, E) pairs of the models that have a Jacobian (0.6-0.7 of HBM) - constant velocity or the
// coordinated turn with radar or four bearings among them - the run-time-size body for the rest (0.13-0.21; other sensor counts) -
// and for every shape under the form's switch (tools/alt_paths.sh, tests)
template <bool LIN>
static void launch_ladder(const TaylorGpqdArgs &a, hipStream_t s) {
    const int D = a.D, E = a.E;
    if (ssmq::sw(LIN ? "SSMQ_LINEAR_GENERIC" : "SSMQ_TAYLOR_GPQD_GENERIC") != nullptr) launch_shape<LIN, 0, 0>(a, s);
    else if (D == 1 && E == 1) launch_shape<LIN, 1, 1>(a, s);
    else if (D == 2 && E == 1) launch_shape<LIN, 2, 1>(a, s);
    else if (D == 2 && E == 2) launch_shape<LIN, 2, 2>(a, s);
    else if (D == 4 && E == 2) launch_shape<LIN, 4, 2>(a, s);
    else if (D == 4 && E == 4) launch_shape<LIN, 4, 4>(a, s);
    else if (D == 5 && (E == 2 || E == 4 || E == 5)) {
        // the linearisation only: the D = 5 bodies of k_taylor_gpqd index a Cholesky factor in scratch memory and
        // are not instantiated - those shapes keep the run-time-size body there
        if constexpr (LIN) {
            if (E == 2) launch_shape<LIN, 5, 2>(a, s);
            else if (E == 4) launch_shape<LIN, 5, 4>(a, s);
            else launch_shape<LIN, 5, 5>(a, s);
        } else {
            launch_shape<LIN, 0, 0>(a, s);
        }
    } else launch_shape<LIN, 0, 0>(a, s);
}

// h: a linearisation or a Taylor-GPQD handle (D, E, and for the latter alpha, ell and the optional variance planes); din: the
// integrand's own input count (ssmq_api_transform.hip: check_integrand, FInfo); planes: the planes, time argument, B, ld and hooks
int launch_jacobian(const ssmq_transform *h, int din, const ssmq_integrand *f, const LinArgs &planes, hipStream_t s, const char **name,
                    bool dry_run) {
    const bool lin = h->form == SSMQ_FORM_TAYLOR1;
    const int D = h->D, E = h->E;
    TaylorGpqdArgs a;
    static_cast<LinArgs &>(a) = planes;
    a.D = D; a.E = E; a.din = din; a.fid = f->id; a.bcast = (f->n_idx == 0 && din == 1 && D > 1) ? 1 : 0;
    a.model_var = h->d_tg_mvar; a.integ_var = h->d_tg_ivar; a.alpha = h->tg_alpha;      // (a linearisation handle: null, 0 - not read)
    for (int d = 0; d < SSMQ_MAX_DIM; ++d) a.ell[d] = d < D ? h->tg_ell[d] : 1.0;
    if (is_user_integrand(f)) return rtc_launch_jacobian(h->form, f, a, s, name, dry_run);      // (makes the checks of that route)
    if (name) *name = lin ? "k_linearize" : "k_taylor_gpqd";
    if (dry_run) return SSMQ_OK;
    const std::string what = lin ? "linearisation" : "Taylor-GPQD";
    if (!integrand_has_jacobian(f->id)) {
        set_error(what + ": this model has no Jacobian (its dyn_fcn_dx / meas_fcn_dx returns None in the reference too)");
        return SSMQ_E_UNSUPPORTED;
    }
    // (a Jacobian of 1 < din < D columns without a state index lands in the leading din columns, the rest zero: how a user model's
    // is placed and how meas_eval reads its inputs; din == 1 < D is the pendulum's broadcast)
    if (!jacobian_fits(f->id, D, E)) {
        set_error(what + ": this model's Jacobian does not fit the shape (D, E) = (" + std::to_string(D) + ", " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    if (lin) launch_ladder<true>(a, s);
    else launch_ladder<false>(a, s);
    return hip_fail(hipGetLastError(), lin ? "k_linearize" : "k_taylor_gpqd");
}

}  // namespace ssmq
