// C ABI of libssmq (include/ssmq.h), one moment transform: the handle's life cycle with the upload of its constant blocks, and
// the route selection that takes a batch to the kernel family for its shape (apply_dev_impl).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "ssmq_host.h"
#include "ssmq_apply_small.h"
#include "ssmq_jacobian_kernel.h"   // LinArgs

namespace ssmq {

void fill_fpar(const ssmq_integrand *f, FPar *fp) {
    memset(fp, 0, sizeof(*fp));
    fp->n_par = std::max(0, std::min<int>(f->n_par, SSMQ_MAX_FPAR));
    fp->n_idx = std::max(0, std::min<int>(f->n_idx, SSMQ_MAX_FIDX));
    for (int i = 0; i < fp->n_par; ++i) fp->p[i] = f->par[i];
    for (int i = 0; i < fp->n_idx; ++i) fp->idx[i] = f->idx[i];
    fp->ttab = nullptr;
}

const SmallEntry *find_small(int fid, int D, int E, int N, int form, int tp, int sel, int opt) {
    typedef const SmallEntry *(*tab_fn)(int *);
    static const tab_fn tabs[] = {small_table_a, small_table_b, small_table_c, small_table_d};
    for (tab_fn t : tabs) {
        int n = 0;
        const SmallEntry *e = t(&n);
        for (int i = 0; i < n; ++i)
            if (e[i].fid == fid && e[i].D == D && e[i].E == E && e[i].N == N && e[i].form == form && e[i].tp == tp &&
                e[i].sel == sel && e[i].opt == opt)
                return &e[i];
    }
    return nullptr;
}

static int upload_consts(ssmq_transform *h) {
    ++h->generation;   // part of the filter loop's graph key: new constants never replay a graph captured for old ones
    const int D = h->D, E = h->E, N = h->N;
    const bool sigma = h->form == SSMQ_FORM_SIGMA;
    const ConstLayout cs = const_layout(D, E, N, h->form);
    const WideLayout cw = wide_layout(D, E, N, h->form);
    std::vector<double> s(cs.total, 0.0), w(cw.total, 0.0);
    for (int d = 0; d < D; ++d)
        for (int n = 0; n < N; ++n) {
            s[cs.xi + n * D + d] = h->xi[d * N + n];
            w[cw.xiT + n * D + d] = h->xi[d * N + n];
        }
    for (int n = 0; n < N; ++n) s[cs.wm + n] = w[cw.wm + n] = h->wm[n];
    if (sigma) {
        for (int n = 0; n < N; ++n) s[cs.Wc + n] = w[cw.Wc + n] = h->Wc[n];
        // the centred form's cross-covariance sum_n wc_n (fx_n - m)(x_n - m_x)' with x_n - m_x = L xi_n is (fx_c W') L' for
        // W[d][n] = xi[d][n] wc_n: kept in the natural-layout block's Wcc slot for the kernels that form it that way
        for (int d = 0; d < D; ++d)
            for (int n = 0; n < N; ++n) w[cw.Wcc + d * N + n] = h->xi[d * N + n] * h->Wc[n];
    } else {
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                s[cs.Wc + j * N + i] = h->Wc[i * N + j];  // transposed: column j contiguous
                w[cw.Wc + i * N + j] = h->Wc[i * N + j];
            }
        for (int d = 0; d < D; ++d)
            for (int n = 0; n < N; ++n) {
                s[cs.Wcc + d * N + n] = h->Wcc[d * N + n];   // row d contiguous (one body of the ccov stage)
                w[cw.Wcc + d * N + n] = h->Wcc[d * N + n];
            }
    }
    for (int i = 0; i < E * E; ++i) s[cs.emv + i] = w[cw.emv + i] = h->emv[i];
    if (h->tp_nu > 0.0) {
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                s[cs.iK + j * N + i] = h->iK[i * N + j];
                w[cw.iK + i * N + j] = h->iK[i * N + j];
            }
    }
    // per-point records (const_layout: rec / rs); record N stays zero
    for (int n = 0; n < N; ++n) {
        double *r = s.data() + cs.rec + (size_t)n * cs.rs;
        for (int d = 0; d < D; ++d) r[d] = h->xi[d * N + n];
        r[D] = h->wm[n];
        if (sigma) {
            r[D + 1] = h->Wc[n];
        } else {
            for (int d = 0; d < D; ++d) r[D + 1 + d] = h->Wcc[d * N + n];
            for (int i = 0; i < N; ++i) r[2 * D + 1 + i] = h->Wc[i * N + n];
            if (h->tp_nu > 0.0)
                for (int i = 0; i < N; ++i) r[2 * D + 1 + N + i] = h->iK[i * N + n];
        }
    }
    // ---- optional fast paths (ssmq_apply_small.h: SSMQ_OPT_LDL / SSMQ_OPT_UT), each verified before it is offered ----
    h->opt_mask = 0;
    if (!sigma) {
        // Wc = U diag(d) U', unit lower U, no pivoting; accepted only if the factorisation reproduces Wc to 1e-14
        std::vector<double> U((size_t)N * N, 0.0), dd(N, 0.0), A(h->Wc);
        bool ok = true;
        double wmax = 0.0;
        for (double v : A) wmax = std::max(wmax, std::fabs(v));
        for (int j = 0; j < N && ok; ++j) {
            double dj = A[j * N + j];
            for (int k = 0; k < j; ++k) dj -= U[j * N + k] * U[j * N + k] * dd[k];
            if (!(std::fabs(dj) > 1e-13 * wmax)) ok = false;
            dd[j] = dj;
            U[j * N + j] = 1.0;
            for (int i = j + 1; i < N && ok; ++i) {
                double v = 0.5 * (A[i * N + j] + A[j * N + i]);
                for (int k = 0; k < j; ++k) v -= U[i * N + k] * U[j * N + k] * dd[k];
                U[i * N + j] = v / dj;
            }
        }
        double err = 0.0;
        for (int i = 0; i < N && ok; ++i)
            for (int j = 0; j < N; ++j) {
                double v = 0.0;
                for (int k = 0; k <= std::min(i, j); ++k) v += U[i * N + k] * dd[k] * U[j * N + k];
                err = std::max(err, std::fabs(v - A[i * N + j]));
            }
        if (ok && err <= 1e-14 * wmax && !ssmq::sw("SSMQ_NO_FASTPATH")) {
            h->opt_mask |= SSMQ_OPT_LDL;
            for (int j = 0; j < N; ++j) {
                s[cs.ldlD + j] = dd[j];
                for (int i = 0; i < N; ++i) s[cs.ldlU + j * N + i] = U[i * N + j];   // column j contiguous
            }
        }
    }
    if (N == 2 * D + 1 && !ssmq::sw("SSMQ_NO_FASTPATH")) {
        const double cc = h->xi[0 * N + 1];
        bool ut = cc > 0.0;
        for (int d = 0; d < D && ut; ++d)
            for (int n = 0; n < N; ++n) {
                double want = 0.0;
                if (n == 1 + d) want = cc;
                if (n == 1 + D + d) want = -cc;
                if (h->xi[d * N + n] != want) ut = false;
            }
        if (ut) {
            h->opt_mask |= SSMQ_OPT_UT;
            s[cs.utc] = cc;
        }
        // SSMQ_OPT_SYM: weights invariant under every reflection of the point set (swap of points 1 + k and 1 + D + k) up to the
        // round-off of the weight computation: symmetrise, rebuild (wm, Wc, Wcc) from the symmetric parameters, accept if no
        // weight moved by more than 2e-13 of the largest of its array; then the LDL' of the (D + 1) x (D + 1) symmetric block.
        if (ut && !sigma && h->tp_nu <= 0.0) {
            const int M = D + 1;
            const double tol = 2e-13;
            auto W = [&](int i, int j) { return h->Wc[(size_t)i * N + j]; };
            std::vector<double> wms(M), gam(D), beta(D), Mt((size_t)M * M);
            double dev_wm = 0.0, dev_wc = 0.0, dev_cc = 0.0, mx_wm = 0.0, mx_wc = 0.0, mx_cc = 0.0;
            wms[0] = h->wm[0];
            for (int k = 0; k < D; ++k) wms[1 + k] = 0.5 * (h->wm[1 + k] + h->wm[1 + D + k]);
            for (int n = 0; n < N; ++n) {
                mx_wm = std::max(mx_wm, std::fabs(h->wm[n]));
                dev_wm = std::max(dev_wm, std::fabs(h->wm[n] - wms[n == 0 ? 0 : 1 + (n - 1) % D]));
            }
            for (int d = 0; d < D; ++d) {
                gam[d] = 0.5 * (h->Wcc[(size_t)d * N + 1 + d] - h->Wcc[(size_t)d * N + 1 + D + d]);
                for (int n = 0; n < N; ++n) {
                    const double want = n == 1 + d ? gam[d] : (n == 1 + D + d ? -gam[d] : 0.0);
                    mx_cc = std::max(mx_cc, std::fabs(h->Wcc[(size_t)d * N + n]));
                    dev_cc = std::max(dev_cc, std::fabs(h->Wcc[(size_t)d * N + n] - want));
                }
            }
            Mt[0] = W(0, 0);
            for (int k = 0; k < D; ++k) {
                const int p = 1 + k, q = 1 + D + k;
                Mt[1 + k] = Mt[(size_t)(1 + k) * M] = 0.25 * (W(0, p) + W(0, q) + W(p, 0) + W(q, 0));
                beta[k] = 0.25 * (W(p, p) + W(q, q) - W(p, q) - W(q, p));
                for (int j = 0; j < D; ++j) {
                    const int r = 1 + j, t = 1 + D + j;
                    Mt[(size_t)(1 + k) * M + 1 + j] = 0.25 * (W(p, r) + W(p, t) + W(q, r) + W(q, t));
                }
            }
            for (int i = 0; i < M; ++i)          // (symmetric by construction up to the asymmetry of Wc itself)
                for (int j = 0; j < i; ++j) Mt[(size_t)i * M + j] = Mt[(size_t)j * M + i] = 0.5 * (Mt[(size_t)i * M + j] + Mt[(size_t)j * M + i]);
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    const int ci = i == 0 ? 0 : 1 + (i - 1) % D, cj = j == 0 ? 0 : 1 + (j - 1) % D;
                    double want = Mt[(size_t)ci * M + cj];
                    if (i != 0 && ci == cj) want += (i == j) ? beta[ci - 1] : -beta[ci - 1];
                    mx_wc = std::max(mx_wc, std::fabs(W(i, j)));
                    dev_wc = std::max(dev_wc, std::fabs(W(i, j) - want));
                }
            bool ok = dev_wm <= tol * mx_wm && dev_wc <= tol * mx_wc && dev_cc <= tol * mx_cc;
            // Mt = Ut diag(d) Ut' with Ut unit UPPER triangular (the kernel meets the columns of G in increasing order): the LDL' of
            // the index-reversed matrix, reversed back.  No pivoting; accepted only if it reproduces Mt to 1e-14.
            std::vector<double> Lr((size_t)M * M, 0.0), dr(M, 0.0), Ut((size_t)M * M, 0.0), dd(M, 0.0);
            auto Mr = [&](int i, int j) { return Mt[(size_t)(M - 1 - i) * M + (M - 1 - j)]; };
            for (int j = 0; j < M && ok; ++j) {
                double dj = Mr(j, j);
                for (int k = 0; k < j; ++k) dj -= Lr[(size_t)j * M + k] * Lr[(size_t)j * M + k] * dr[k];
                if (!(std::fabs(dj) > 1e-13 * mx_wc)) ok = false;
                dr[j] = dj;
                Lr[(size_t)j * M + j] = 1.0;
                for (int i = j + 1; i < M && ok; ++i) {
                    double v = Mr(i, j);
                    for (int k = 0; k < j; ++k) v -= Lr[(size_t)i * M + k] * Lr[(size_t)j * M + k] * dr[k];
                    Lr[(size_t)i * M + j] = v / dj;
                }
            }
            for (int i = 0; i < M; ++i) {
                dd[i] = dr[M - 1 - i];
                for (int j = 0; j < M; ++j) Ut[(size_t)i * M + j] = Lr[(size_t)(M - 1 - i) * M + (M - 1 - j)];
            }
            double err = 0.0;
            for (int i = 0; i < M && ok; ++i)
                for (int j = 0; j < M; ++j) {
                    double v = 0.0;
                    for (int k = std::max(i, j); k < M; ++k) v += Ut[(size_t)i * M + k] * dd[k] * Ut[(size_t)j * M + k];
                    err = std::max(err, std::fabs(v - Mt[(size_t)i * M + j]));
                }
            if (ok && err <= 1e-14 * mx_wc && (h->opt_mask & SSMQ_OPT_LDL) && !ssmq::sw("SSMQ_NO_SYM")) {
                h->opt_mask |= SSMQ_OPT_SYM;
                for (int j = 0; j < M; ++j) {
                    double *r = s.data() + cs.sym + (size_t)j * cs.sym_rs;
                    r[0] = wms[j];
                    r[1] = dd[j];
                    r[2] = j ? gam[j - 1] : 0.0;
                    r[3] = j ? beta[j - 1] : 0.0;
                    for (int i = 0; i < j; ++i) r[4 + i] = Ut[(size_t)i * M + j];
                }
            }
        }
    }
    std::vector<double> wpad;
    const int np = sigma ? 0 : gemm_mfma_padded(N);
    if (np && !ssmq::sw("SSMQ_NO_MFMA")) {
        wpad.assign((size_t)np * np, 0.0);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) wpad[(size_t)i * np + j] = h->Wc[i * N + j];
        if (!h->d_wc_pad) SSMQ_HIP(hipMalloc(&h->d_wc_pad, sizeof(double) * np * np));
        h->np_pad = np;
        SSMQ_HIP(hipMemcpyAsync(h->d_wc_pad, wpad.data(), sizeof(double) * np * np, hipMemcpyHostToDevice, stream()));
        // X = [Wc | Wcc'] for the route whose GEMM epilogue forms both covariances (row k: row k of Wc, then
        // Wcc[0..D)[k]): T = FX Wc exactly as the other kernels form it, also for a Wc that is not symmetric to the last bit
        const int nx = np + 16;
        std::vector<double> xpad((size_t)np * nx, 0.0);
        for (int k = 0; k < N; ++k) {
            for (int j = 0; j < N; ++j) xpad[(size_t)k * nx + j] = h->Wc[k * N + j];
            for (int d = 0; d < D && d < 16; ++d) xpad[(size_t)k * nx + np + d] = h->Wcc[d * N + k];
            // the tile's last column is free up to D = 15: wm there makes FX wm a by-product of the same GEMM
            // (k_bq_fused reads it; k_fxwc_cov_mfma only looks at columns < D)
            if (D <= 15) xpad[(size_t)k * nx + np + 15] = h->wm[k];
        }
        if (!h->d_wcx_pad) SSMQ_HIP(hipMalloc(&h->d_wcx_pad, sizeof(double) * np * nx));
        SSMQ_HIP(hipMemcpyAsync(h->d_wcx_pad, xpad.data(), sizeof(double) * np * nx, hipMemcpyHostToDevice, stream()));
        // the same with S in place of Wc: S = lower triangle of Wc with half its diagonal, so that Wc = S + S' and
        // fx Wc fx' = C + C', C = (fx S) fx' (k_bq_fused / k_bq_stream: half the matrix instructions of the main product).
        // Only for a Wc that is symmetric to the last bit - every Wc the weight kernels (and the reference, bq/bqmod.py:520-521)
        // produce; an injected non-symmetric one keeps the routes that form (fx Wc) fx' as written.
        bool symmetric = true;
        for (int k = 0; k < N && symmetric; ++k)
            for (int j = 0; j < k; ++j)
                if (h->Wc[k * N + j] != h->Wc[j * N + k]) {
                    symmetric = false;
                    break;
                }
        if (symmetric) {
            std::vector<double> spad(xpad);
            for (int k = 0; k < N; ++k)
                for (int j = 0; j < N; ++j)
                    spad[(size_t)k * nx + j] = j < k ? h->Wc[k * N + j] : (j == k ? 0.5 * h->Wc[k * N + k] : 0.0);
            if (!h->d_sx_pad) SSMQ_HIP(hipMalloc(&h->d_sx_pad, sizeof(double) * np * nx));
            SSMQ_HIP(hipMemcpyAsync(h->d_sx_pad, spad.data(), sizeof(double) * np * nx, hipMemcpyHostToDevice, stream()));
            SSMQ_HIP(hipStreamSynchronize(stream()));   // spad goes out of scope
        } else if (h->d_sx_pad) {
            SSMQ_HIP(hipStreamSynchronize(stream()));
            hipFree(h->d_sx_pad);
            h->d_sx_pad = nullptr;
        }
        SSMQ_HIP(hipStreamSynchronize(stream()));   // xpad goes out of scope
    }
    if (!sigma && bq_stream_supported(D, E, N)) {
        // one-launch route for these sizes (k_bq_stream): S = tril(Wc), half the diagonal, by panels - a Wc symmetric to the last
        // bit only (see d_sx_pad above)
        bool symmetric = bq_stream_supported(D, E, N) && h->tp_nu <= 0.0;
        for (int k = 0; k < N && symmetric; ++k)
            for (int j = 0; j < k; ++j)
                if (h->Wc[(size_t)k * N + j] != h->Wc[(size_t)j * N + k]) {
                    symmetric = false;
                    break;
                }
        if (h->d_sx_pan) {
            SSMQ_HIP(hipStreamSynchronize(stream()));
            hipFree(h->d_sx_pan);
            h->d_sx_pan = nullptr;
        }
        if (symmetric) {
            std::vector<double> xs(bq_stream_x_doubles(N));
            bq_stream_pack(D, N, h->Wc.data(), h->Wcc.data(), h->wm.data(), xs.data());
            SSMQ_HIP(hipMalloc(&h->d_sx_pan, sizeof(double) * xs.size()));
            SSMQ_HIP(hipMemcpyAsync(h->d_sx_pan, xs.data(), sizeof(double) * xs.size(), hipMemcpyHostToDevice, stream()));
            SSMQ_HIP(hipStreamSynchronize(stream()));
        }
    }
    if (!sigma && N > 64 && !np && !ssmq::sw("SSMQ_NO_MFMA")) {
        // any other point count beyond the wave kernels: Wc (and iK for the t-process) as column blocks of kBigCols
        // columns, block c = [kb 16][kBigCols] zero-padded, for the blocked GEMM (launch_fxwc_blocks)
        // the Wc blocks carry D extra columns from column 16 kb on: Wcc', so that fx Wcc' comes out of the same GEMM
        const int kb = (N + 15) / 16, ncols = 16 * kb + D, ncb = (ncols + kBigCols - 1) / kBigCols;
        const size_t per = (size_t)kb * 16 * kBigCols, total = per * ncb;
        auto pack = [&](const std::vector<double> &src, double **dst, bool with_wcc) -> int {
            std::vector<double> blk(total, 0.0);
            auto at = [&](int i, int j) -> double & { return blk[(size_t)(j / kBigCols) * per + (size_t)i * kBigCols + j % kBigCols]; };
            for (int i = 0; i < N; ++i) {
                for (int j = 0; j < N; ++j) at(i, j) = src[(size_t)i * N + j];
                if (with_wcc)
                    for (int d = 0; d < D; ++d) at(i, 16 * kb + d) = h->Wcc[(size_t)d * N + i];
            }
            // on the library's stream, as every other upload of this function: a transform queued there (the entry points ending
            // in _dev are asynchronous) may still be reading the old blocks
            if (*dst && (h->big_kb != kb || h->big_ncb != ncb)) {
                SSMQ_HIP(hipStreamSynchronize(stream()));
                hipFree(*dst);
                *dst = nullptr;
            }
            if (!*dst) SSMQ_HIP(hipMalloc(dst, sizeof(double) * total));
            SSMQ_HIP(hipMemcpyAsync(*dst, blk.data(), sizeof(double) * total, hipMemcpyHostToDevice, stream()));
            SSMQ_HIP(hipStreamSynchronize(stream()));   // blk goes out of scope
            return SSMQ_OK;
        };
        int rcp = pack(h->Wc, &h->d_wc_blk, true);
        if (rcp) return rcp;
        if (h->tp_nu > 0.0 && (int)h->iK.size() == N * N && (rcp = pack(h->iK, &h->d_ik_blk, false))) return rcp;
        h->big_kb = kb;
        h->big_ncb = ncb;
    }
    SSMQ_HIP(hipMemcpyAsync(h->d_small, s.data(), sizeof(double) * cs.total, hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipMemcpyAsync(h->d_wide, w.data(), sizeof(double) * cw.total, hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}

int sel_pattern(const ssmq_integrand *f, int din) {
    // 0: leading entries, 1: (0, 2, 4, ...), -1: anything else
    if (f->n_idx <= 0) return 0;
    bool lead = true, even = true;
    for (int k = 0; k < din && k < f->n_idx; ++k) {
        lead = lead && f->idx[k] == k;
        even = even && f->idx[k] == 2 * k;
    }
    if (f->n_idx < din) return -1;
    return lead ? 0 : (even ? 1 : -1);
}

int check_integrand(const ssmq_transform *h, const ssmq_integrand *f, FInfo *fi) {
    if (!f || !integrand_info(f->id, fi)) {
        set_error("unknown integrand id");
        return SSMQ_E_ARG;
    }
    if (f->id == SSMQ_F_BEARING_MEAS) {
        fi->dout = f->n_par / 2;
        if (fi->dout < 1 || fi->dout > SSMQ_MAX_FPAR / 2) {
            set_error("bearing measurement: n_par must be 2 * sensors, 1..8 sensors");
            return SSMQ_E_ARG;
        }
    }
    if (fi->dout != h->E) {
        set_error("integrand output dimension does not match the transform's E");
        return SSMQ_E_ARG;
    }
    if (f->n_idx > SSMQ_MAX_FIDX || f->n_par > SSMQ_MAX_FPAR || f->n_idx < 0 || f->n_par < 0) {
        set_error("integrand: n_idx / n_par out of range");
        return SSMQ_E_ARG;
    }
    if (f->n_idx > 0) {
        if (f->n_idx < fi->din) {
            set_error("integrand: state index shorter than the integrand's input");
            return SSMQ_E_ARG;
        }
        for (int k = 0; k < f->n_idx; ++k)
            if (f->idx[k] < 0 || f->idx[k] >= h->D) {
                set_error("integrand: state index out of range");
                return SSMQ_E_ARG;
            }
    } else if (fi->din > h->D) {
        set_error("integrand reads more inputs than the transform's D");
        return SSMQ_E_ARG;
    }
    return SSMQ_OK;
}

// Grow-only scratch of the matrix-core route (asynchronous callers cannot own temporaries): FX and T = FX Wc as
// (B E) x NP row-major, the Cholesky factors [B][D][D].
#define g_gemm_ws (ssmq::ctx().gemm_ws)                  // (the calling thread's context: ssmq_host.h)
#define g_gemm_ws_bytes (ssmq::ctx().gemm_ws_bytes)
static int gemm_scratch(int64_t M, int NP, int64_t B, int D, double **fx, double **tt, double **chol, bool fused = false) {
    // three-pass route: FX | T | factors; two-pass route: FX | transformed means as rows | factors
    const size_t n_fx = (size_t)M * NP, n_t = fused ? (size_t)M : n_fx,
                 need = sizeof(double) * (n_fx + n_t + (size_t)B * D * D);
    if (g_gemm_ws_bytes < need) {
        if (g_gemm_ws) {
            SSMQ_HIP(hipStreamSynchronize(stream()));
            hipFree(g_gemm_ws);
        }
        g_gemm_ws = nullptr;
        g_gemm_ws_bytes = 0;
        SSMQ_HIP(hipMalloc(&g_gemm_ws, need));
        g_gemm_ws_bytes = need;
    }
    *fx = (double *)g_gemm_ws;
    *tt = *fx + n_fx;
    *chol = *tt + n_t;
    return SSMQ_OK;
}
// scratch of the blocked route: FX [M][lda] | T [M][ldt] x n_t | means [M] | factors [B][D][D]
static int big_scratch(int64_t M, int lda, int ldt, int n_t, int64_t B, int D, double **fx, double **tt, double **mrow,
                       double **chol) {
    const size_t n_fx = (size_t)M * lda, n_tt = (size_t)M * ldt * n_t;
    const size_t need = sizeof(double) * (n_fx + n_tt + (size_t)M + (size_t)B * D * D);
    if (g_gemm_ws_bytes < need) {
        if (g_gemm_ws) {
            SSMQ_HIP(hipStreamSynchronize(stream()));
            hipFree(g_gemm_ws);
        }
        g_gemm_ws = nullptr;
        g_gemm_ws_bytes = 0;
        SSMQ_HIP(hipMalloc(&g_gemm_ws, need));
        g_gemm_ws_bytes = need;
    }
    *fx = (double *)g_gemm_ws;
    *tt = *fx + n_fx;
    *mrow = *tt + n_tt;
    *chol = *mrow + M;
    return SSMQ_OK;
}
void drop_gemm_scratch() {
    if (g_gemm_ws) hipFree(g_gemm_ws);
    g_gemm_ws = nullptr;
    g_gemm_ws_bytes = 0;
}

int apply_dev_impl(ssmq_transform *h, const ssmq_integrand *f, int64_t B, int64_t ld, const double *d_mean,
                   const double *d_cov, const double *d_time, int time_stride, double *d_mean_f, double *d_cov_f,
                   double *d_cov_fx, int32_t *d_status, const double *d_cov_add, const char **kernel_name,
                   bool dry_run, double cov_scale, double ccov_scale, const double *ttab, bool stream_out) {
    FInfo fi;
    int rc = check_integrand(h, f, &fi);
    if (rc) return rc;
    auto null_args = [&]() {
        if (d_mean && d_cov && d_mean_f && d_cov_f && d_cov_fx && d_status && (!fi.uses_time || d_time) && ld >= B) return false;
        set_error("apply: null pointer or ld < B");
        return true;
    };
    if (is_mo(h)) {
        // the multi-output form: one kernel for the whole supported range (ssmq_apply_mo.hip), built-in integrands
        if (is_user_integrand(f)) return refuse_user_integrand("multi-output transform (k_apply_mo)");
        if (kernel_name) *kernel_name = "k_apply_mo";
        if (dry_run || B <= 0) return SSMQ_OK;
        if (null_args()) return SSMQ_E_ARG;
        MoArgs m;
        memset(&m, 0, sizeof(m));
        m.D = h->D; m.E = h->E; m.N = h->N; m.mode = SSMQ_MO_FULL; m.fid = f->id; m.time_stride = d_time ? time_stride : 0;
        m.tp_nu = h->tp_nu; m.cov_scale = cov_scale; m.ccov_scale = ccov_scale; m.consts = h->d_mo; m.cov_add = d_cov_add;
        m.mean = d_mean; m.cov = d_cov; m.time = d_time; m.es_in = ld; m.bs_mean = m.bs_cov = 1;
        m.mean_f = d_mean_f; m.cov_f = d_cov_f; m.cov_fx = d_cov_fx; m.es_out = ld; m.bs_mf = m.bs_cf = m.bs_cfx = 1;
        m.status = d_status;
        fill_fpar(f, &m.fp);
        m.fp.ttab = ttab;
        return launch_apply_mo(m, B, stream());
    }
    if (is_trunc(h)) {
        // the truncated sigma-point form: one kernel for the whole supported range (ssmq_apply_trunc.hip), built-in integrands
        if (is_user_integrand(f)) return refuse_user_integrand("truncated sigma-point transform (k_apply_trunc)");
        if (kernel_name) *kernel_name = "k_apply_trunc";
        if (dry_run || B <= 0) return SSMQ_OK;
        if (null_args()) return SSMQ_E_ARG;
        LinArgs a;
        memset(&a, 0, sizeof(a));
        a.mean = d_mean; a.cov = d_cov; a.time = d_time; a.time_stride = d_time ? time_stride : 0; a.cov_add = d_cov_add;
        a.mean_f = d_mean_f; a.cov_f = d_cov_f; a.cov_fx = d_cov_fx; a.status = d_status; a.B = B; a.ld = ld;
        a.cov_scale = cov_scale; a.ccov_scale = ccov_scale;
        fill_fpar(f, &a.fp);
        a.fp.ttab = ttab;
        return launch_apply_trunc(h, f, a, stream());
    }
    if (is_gpqd(h)) {
        // GPQ with derivative observations: one launch (ssmq_apply_gpqd.hip) - for a user integrand, which must have been registered
        // with its Jacobian, of a kernel compiled for it at run time
        const bool user = is_user_integrand(f);
        if (user && !user_integrand_has_jacobian(f->id)) return refuse_user_integrand("GPQ+D transform (k_apply_gpqd) without a Jacobian");
        const bool dry = dry_run || B <= 0;
        LinArgs a;
        memset(&a, 0, sizeof(a));
        if (!dry) {
            if (null_args()) return SSMQ_E_ARG;
            a.mean = d_mean; a.cov = d_cov; a.time = d_time; a.time_stride = d_time ? time_stride : 0; a.cov_add = d_cov_add;
            a.mean_f = d_mean_f; a.cov_f = d_cov_f; a.cov_fx = d_cov_fx; a.status = d_status; a.B = B; a.ld = ld;
            a.cov_scale = cov_scale; a.ccov_scale = ccov_scale;
            fill_fpar(f, &a.fp);
            if (!user) a.fp.ttab = ttab;
        }
        return launch_apply_gpqd(h, fi.din, f, a, stream(), kernel_name, dry);
    }
    // argument block of the register-resident kernels; fp.ttab stays null (the table route sets it, the user route has no table)
    auto fill_args = [&](ApplyArgs &a) {
        a.mean = d_mean; a.cov = d_cov; a.time = d_time ? d_time : d_mean; a.mean_f = d_mean_f; a.cov_f = d_cov_f;
        a.cov_fx = d_cov_fx; a.status = d_status; a.consts = h->d_small;
        a.cov_add = d_cov_add ? d_cov_add : h->d_small + const_layout(h->D, h->E, h->N, h->form).zero; a.B = B; a.ld = ld;
        a.time_stride = d_time ? time_stride : 0; a.emv_mode = h->emv_mode; a.tp_nu = h->tp_nu;
        a.cov_scale = cov_scale; a.ccov_scale = ccov_scale;
        fill_fpar(f, &a.fp);
    };
    if (h->form == SSMQ_FORM_TAYLOR1 || is_taylor_gpqd(h)) {
        // the two Jacobian forms (mtran.py:49-59, 668-701): no points, no weights, one launch (ssmq_linear.hip) - for a user
        // integrand, which must have been registered with its Jacobian, of a kernel compiled for it at run time
        const bool user = is_user_integrand(f);
        if (user && !user_integrand_has_jacobian(f->id))
            return refuse_user_integrand(is_taylor_gpqd(h) ? "Taylor-GPQD transform (k_taylor_gpqd)" : "linearisation transform (k_linearize)");
        const bool dry = dry_run || B <= 0;
        LinArgs a;
        memset(&a, 0, sizeof(a));
        if (!dry) {
            if (null_args()) return SSMQ_E_ARG;
            a.mean = d_mean; a.cov = d_cov; a.time = d_time; a.time_stride = d_time ? time_stride : 0; a.cov_add = d_cov_add;
            a.mean_f = d_mean_f; a.cov_f = d_cov_f; a.cov_fx = d_cov_fx; a.status = d_status; a.B = B; a.ld = ld;
            a.cov_scale = cov_scale; a.ccov_scale = ccov_scale;
            fill_fpar(f, &a.fp);
            if (!user) a.fp.ttab = ttab;      // (a user integrand evaluates its time dependence itself)
        }
        return launch_jacobian(h, fi.din, f, a, stream(), kernel_name, dry);
    }
    if (is_user_integrand(f)) {
        // a user-defined integrand: k_apply_small compiled for it at run time (ssmq_rtc.hip), nothing else
        ApplyArgs a;
        memset(&a, 0, sizeof(a));
        if (!dry_run && B > 0) {
            if (null_args()) return SSMQ_E_ARG;
            fill_args(a);
        }
        a.stream_out = stream_out ? 1 : 0;
        return rtc_launch_apply(h, f, sel_pattern(f, fi.din), a, stream(), kernel_name, dry_run || B <= 0);
    }
    const int tp = h->tp_nu > 0.0 ? 1 : 0;
    const int sel = sel_pattern(f, fi.din);
    const SmallEntry *se = nullptr;
    if (sel >= 0) {
        // best available fast path first (TP keeps the dense covariance form; see SSMQ_OPT_* in ssmq_apply_small.h)
        const int want[5] = {(!tp && (h->opt_mask & 7) == 7) ? 7 : -1, h->opt_mask & (tp ? SSMQ_OPT_UT : 3), h->opt_mask & SSMQ_OPT_UT,
                             h->opt_mask & SSMQ_OPT_LDL & (tp ? 0 : 1), 0};
        for (int k = 0; k < 5 && !se; ++k)
            if (want[k] >= 0) se = find_small(f->id, h->D, h->E, h->N, h->form, tp, sel, want[k]);
    }
    const bool wide_fits = wide_lds_bytes(h->D, h->E, h->N) <= 160 * 1024 - 64;
    // point sets beyond the wave kernels without a fused matrix-core instantiation: evaluation pass, blocked GEMM, rest
    // (the kernel-name query runs with B = 0: it reports the route of a large batch)
    const int64_t b_route = dry_run ? ((int64_t)1 << 20) : B;
    const bool big = !se && h->N > 64 && ((h->form == SSMQ_FORM_BQ && h->d_wc_blk && (b_route * h->E >= kGemmMinRows || !wide_fits) &&
                                           (h->tp_nu <= 0.0 || h->d_ik_blk)) ||
                                          (h->form == SSMQ_FORM_SIGMA && !wide_fits));
    const bool streamed = !se && h->form == SSMQ_FORM_BQ && h->tp_nu <= 0.0 && h->d_sx_pan && b_route * h->E >= kGemmMinRows &&
                          bq_stream_supported(h->D, h->E, h->N);
    const bool one_launch = !se && !big && h->form == SSMQ_FORM_BQ && h->d_wc_pad && h->d_sx_pad && h->tp_nu <= 0.0 &&
                            b_route * h->E >= kGemmMinRows && bq_fused_supported(h->D, h->E, h->N);
    if (kernel_name) *kernel_name = se ? se->name : streamed ? "k_bq_stream" : big ? "k_apply_big" : one_launch ? "k_bq_fused" : ((wide_full_uses_tile(h->D, h->E, h->N) && tile_ld_ok(dry_run ? 0 : ld)) ? "k_apply_tile" : wide_full_uses_wave(h->D, h->E, h->N) ? "k_apply_wave" : "k_apply_wide");
    // (the same two conditions launch_apply_wide tests - tile_pitch_ok there, with unit batch strides as set below; the name
    // query has no batch and reports the route of planes shorter than 2^29 doubles)
    if (dry_run) return SSMQ_OK;
    if (B <= 0) return SSMQ_OK;
    if (null_args()) return SSMQ_E_ARG;
    if (se) {
        ApplyArgs a;
        fill_args(a);
        a.stream_out = stream_out ? 1 : 0;
        a.fp.ttab = ttab;
        return hip_fail(se->fn(a, stream()), se->name);
    }
    if (!big && !wide_fits) {
        set_error("apply: shape too large for the LDS-resident generic kernel");
        return SSMQ_E_UNSUPPORTED;
    }
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.D = h->D; a.E = h->E; a.N = h->N; a.form = h->form; a.mode = SSMQ_WIDE_FULL; a.fid = f->id;
    a.time_stride = d_time ? time_stride : 0; a.emv_mode = h->emv_mode; a.tp_nu = h->tp_nu; a.consts = h->d_wide;
    a.cov_scale = cov_scale; a.ccov_scale = ccov_scale;
    a.cov_add = d_cov_add; a.mean = d_mean; a.cov = d_cov; a.time = d_time; a.es_in = ld; a.bs_mean = 1; a.bs_cov = 1;
    a.mean_f = d_mean_f; a.cov_f = d_cov_f; a.cov_fx = d_cov_fx; a.es_out = ld; a.bs_mf = a.bs_cf = a.bs_cfx = 1;
    a.status = d_status;
    fill_fpar(f, &a.fp);
    a.fp.ttab = ttab;
    if (streamed) {
        // two launches: (1) one wave per trajectory: factor, points, integrand values FX, factors; (2) the streamed product whose
        // epilogues form mean, covariance and cross-covariance (ssmq_bq_stream.hip)
        const int kb = (h->N + 15) / 16, lda = kb * 16;
        // FX in fragment order: blocks of 64 / E trajectories, 64 rows each (ssmq_wide.h: fx_frag)
        const int tpw = bq_stream_tpw(h->E);
        const int64_t M = (B + tpw - 1) / tpw * 64;
        // the last, partly empty round of workgroups is cut by panel (ssmq_bq_stream.hip: bq_stream_split): room for the parts
        static thread_local int cus = 0;
        static thread_local unsigned cus_epoch = ~0u;
        if (cus_epoch != device_epoch()) {
            int dev = 0;
            hipDeviceProp_t prop;
            SSMQ_HIP(hipGetDevice(&dev));
            SSMQ_HIP(hipGetDeviceProperties(&prop, dev));
            cus = prop.multiProcessorCount;
            cus_epoch = device_epoch();
        }
        const size_t parts_n = bq_stream_parts_doubles(h->E, h->N, B, cus);
        const int ldt = (int)((parts_n + (size_t)M - 1) / (size_t)M);
        double *fx, *tt, *mrow, *chol;
        if ((rc = big_scratch(M, lda, ldt, ldt ? 1 : 0, B, h->D, &fx, &tt, &mrow, &chol))) return rc;
        WideArgs e = a;
        e.fx_ld = lda; e.fx_out = fx; e.mrow_out = mrow; e.chol_out = chol; e.fx_frag = tpw;
        if ((rc = hip_fail(launch_eval_wave(e, B, stream()), "k_eval_wave"))) return rc;
        const WideLayout wl = wide_layout(h->D, h->E, h->N, h->form);
        return launch_bq_stream(a, h->d_sx_pan, h->d_wide + wl.emv, h->emv_mode == SSMQ_EMV_BROADCAST ? 1 : 0, B, fx, chol, lda, cus,
                                parts_n ? tt : nullptr, stream());
    }
    if (big) {
        const bool bq = h->form == SSMQ_FORM_BQ, tpb = bq && h->tp_nu > 0.0;
        const int kb = (h->N + 15) / 16, lda = kb * 16, ldt = bq ? h->big_ncb * kBigCols : 0;
        const int64_t M = B * h->E;
        double *fx, *tt, *mrow, *chol;
        if ((rc = big_scratch(M, lda, ldt, bq ? (tpb ? 2 : 1) : 0, B, h->D, &fx, &tt, &mrow, &chol))) return rc;
        WideArgs e = a;
        e.fx_ld = lda; e.fx_out = fx; e.mrow_out = mrow; e.chol_out = chol;
        if ((rc = hip_fail(launch_eval_wave(e, B, stream()), "k_eval_wave"))) return rc;
        if (bq && (rc = launch_fxwc_blocks(fx, h->d_wc_blk, tt, M, lda, ldt, kb, h->big_ncb, stream()))) return rc;
        if (tpb && (rc = launch_fxwc_blocks(fx, h->d_ik_blk, tt + (size_t)M * ldt, M, lda, ldt, kb, h->big_ncb, stream()))) return rc;
        BigRest r;
        memset(&r, 0, sizeof(r));
        r.D = h->D; r.E = h->E; r.N = h->N; r.form = h->form; r.emv_mode = h->emv_mode; r.tp_nu = h->tp_nu;
        r.cov_scale = cov_scale; r.ccov_scale = ccov_scale; r.consts = h->d_wide; r.fx = fx; r.t = bq ? tt : nullptr;
        r.t2 = tpb ? tt + (size_t)M * ldt : nullptr; r.lda = lda; r.ldt = ldt; r.p_col = 16 * kb; r.mean_rows = mrow; r.chol = chol;
        r.cov_add = d_cov_add; r.cov_f = d_cov_f; r.cov_fx = d_cov_fx; r.es = ld; r.bs_cf = 1; r.bs_cfx = 1; r.status = d_status;
        return launch_big_rest(r, B, stream());
    }
    if (h->d_wc_pad && h->form == SSMQ_FORM_BQ && B * h->E >= kGemmMinRows) {
        // large point set: integrand values of the whole batch -> one GEMM on the matrix cores -> per-trajectory rest
        const int NP = h->np_pad;
        const int64_t M = B * h->E;
        double *fx, *tt, *chol;
        if (h->tp_nu <= 0.0 && h->d_sx_pad && bq_fused_supported(h->D, h->E, h->N)) {
            // one launch: the workgroup that owns a block of the GEMM's rows evaluates the integrand into LDS itself
            const WideLayout wl = wide_layout(h->D, h->E, h->N, h->form);
            return launch_bq_fused(a, h->d_sx_pad, h->d_wide + wl.emv, h->emv_mode == SSMQ_EMV_BROADCAST ? 1 : 0, B, stream());
        }
        if (h->tp_nu <= 0.0 && h->d_wcx_pad && fxwc_cov_supported(h->E) && h->D <= 16 && !ssmq::sw("SSMQ_NO_FUSED_COV")) {
            // two passes: (1) one wave per trajectory: factor, points, integrand values, mean; (2) the GEMM whose
            // epilogue forms the covariance and the cross-covariance from its accumulators
            if ((rc = gemm_scratch(M, NP, B, h->D, &fx, &tt, &chol, true))) return rc;
            double *mrow = tt;
            WideArgs e = a;
            e.fx_ld = NP; e.fx_out = fx; e.mrow_out = mrow; e.chol_out = chol;
            if ((rc = hip_fail(launch_eval_wave(e, B, stream()), "k_eval_wave"))) return rc;
            const WideLayout wl = wide_layout(h->D, h->E, h->N, h->form);
            return launch_fxwc_cov_mfma(NP, fx, h->d_wcx_pad, M, NP, mrow, chol, h->d_wide + wl.emv,
                                        h->emv_mode == SSMQ_EMV_BROADCAST ? 1 : 0, d_cov_add, cov_scale, ccov_scale, h->E,
                                        h->D, d_cov_f, d_cov_fx, ld, 1, 1, stream());
        }
        if ((rc = gemm_scratch(M, NP, B, h->D, &fx, &tt, &chol))) return rc;
        WideArgs e = a;
        e.mode = SSMQ_WIDE_EVAL; e.fx_ld = NP; e.fx_out = fx; e.chol_out = chol;
        if ((rc = hip_fail(launch_apply_wide(e, B, stream()), "k_apply_wide(eval)"))) return rc;
        if ((rc = launch_fxwc_mfma(NP, fx, h->d_wc_pad, tt, M, NP, NP, stream()))) return rc;
        a.mode = SSMQ_WIDE_FX; a.fx_ld = NP; a.fx_in = fx; a.t_in = tt; a.chol_in = chol; a.status = nullptr;
        return hip_fail(launch_apply_wide(a, B, stream()), "k_apply_wide(fx + T)");
    }
    return hip_fail(launch_apply_wide(a, B, stream()), "k_apply_wide");
}

}  // namespace ssmq

using namespace ssmq;

extern "C" {

// ---- transform handle ----------------------------------------------------------------------------------------------
ssmq_transform *ssmq_transform_create(int D, int E, int N, int form, const double *xi, const double *wm,
                                      const double *Wc, const double *Wcc, const double *emv, int emv_mode,
                                      double tp_nu, const double *tp_iK) {
    if (D < 1 || D > SSMQ_MAX_DIM || E < 1 || E > SSMQ_MAX_DIM || N < 1 || N > SSMQ_MAX_PTS ||
        (form != SSMQ_FORM_BQ && form != SSMQ_FORM_SIGMA) || !xi || !wm || !Wc || (form == SSMQ_FORM_BQ && !Wcc) ||
        (tp_nu > 0.0 && !tp_iK) || (emv_mode != SSMQ_EMV_DIAG && emv_mode != SSMQ_EMV_BROADCAST)) {
        set_error("transform_create: bad argument");
        return nullptr;
    }
    if (ensure_device()) return nullptr;
    ssmq_transform *h = new ssmq_transform();
    h->D = D; h->E = E; h->N = N; h->form = form; h->emv_mode = emv_mode; h->tp_nu = tp_nu;
    hipGetDevice(&h->device);
    h->xi.assign(xi, xi + D * N);
    h->wm.assign(wm, wm + N);
    h->Wc.assign(Wc, Wc + (form == SSMQ_FORM_SIGMA ? N : N * N));
    if (form == SSMQ_FORM_BQ) h->Wcc.assign(Wcc, Wcc + D * N);
    h->emv.assign(E * E, 0.0);
    if (emv) h->emv.assign(emv, emv + E * E);
    if (tp_nu > 0.0) h->iK.assign(tp_iK, tp_iK + N * N);
    h->d_small = h->d_wide = nullptr;
    const ConstLayout cs = const_layout(D, E, N, form);
    const WideLayout cw = wide_layout(D, E, N, form);
    if (hipMalloc((void **)&h->d_small, sizeof(double) * cs.total) != hipSuccess ||
        hipMalloc((void **)&h->d_wide, sizeof(double) * cw.total) != hipSuccess || upload_consts(h) != SSMQ_OK) {
        if (!*ssmq_last_error()) set_error("transform_create: device allocation failed");
        ssmq_transform_destroy(h);
        return nullptr;
    }
    return h;
}

// The linearisation transform has neither points nor weights; the handle keeps a one-point placeholder block so that every
// code path that sizes or frees constants finds what it expects.
ssmq_transform *ssmq_transform_create_linear(int D, int E) {
    if (D < 1 || D > SSMQ_MAX_DIM || E < 1 || E > SSMQ_MAX_DIM) {
        set_error("transform_create_linear: bad argument");
        return nullptr;
    }
    std::vector<double> xi((size_t)D, 0.0);
    const double one = 1.0;
    ssmq_transform *h = ssmq_transform_create(D, E, 1, SSMQ_FORM_SIGMA, xi.data(), &one, &one, nullptr, nullptr, SSMQ_EMV_DIAG, 0.0,
                                              nullptr);
    if (h) h->form = SSMQ_FORM_TAYLOR1;
    return h;
}

// The Taylor-GPQD transform likewise keeps the one-point placeholder block; its kernel parameters live in the handle and reach
// the kernel by value.  `generation` carries a hash of them: a handle that a later allocation puts at the address of a destroyed
// one must not find the launch loop captured for the old parameters (key_of_pair, ssmq_host.h).
ssmq_transform *ssmq_transform_create_taylor_gpqd(int D, int E, double alpha, const double *ell) {
    if (D < 1 || D > SSMQ_MAX_DIM || E < 1 || E > SSMQ_MAX_DIM || !ell || !std::isfinite(alpha)) {
        set_error("transform_create_taylor_gpqd: bad argument (1 <= D, E <= 16, finite alpha, ell [D])");
        return nullptr;
    }
    for (int d = 0; d < D; ++d)
        if (!std::isfinite(ell[d]) || !(ell[d] > 0.0)) {
            set_error("transform_create_taylor_gpqd: length-scales must be finite and positive (ell[" + std::to_string(d) + "])");
            return nullptr;
        }
    ssmq_transform *h = ssmq_transform_create_linear(D, E);
    if (!h) return nullptr;
    h->form = SSMQ_FORM_TAYLOR_GPQD;
    h->tg_alpha = alpha;
    std::copy(ell, ell + D, h->tg_ell);
    std::vector<uint64_t> words;
    key_bytes(words, &alpha, sizeof(double));
    key_bytes(words, ell, sizeof(double) * D);
    uint64_t hash = 1469598103934665603ull;
    for (uint64_t w : words) hash = (hash ^ w) * 1099511628211ull;
    h->generation = (uint32_t)(hash ^ (hash >> 32));
    return h;
}

int ssmq_taylor_gpqd_variance_planes(ssmq_transform *h, double *d_model_var, double *d_integ_var) {
    SSMQ_HANDLE_LOCK(h);
    if (!is_taylor_gpqd(h)) {
        set_error("taylor_gpqd_variance_planes: not a Taylor-GPQD handle");
        return SSMQ_E_ARG;
    }
    // (a captured launch loop holds the old pointers by value: a new generation is a new graph key)
    h->generation += 1;
    h->d_tg_mvar = d_model_var;
    h->d_tg_ivar = d_integ_var;
    return SSMQ_OK;
}

int ssmq_transform_update(ssmq_transform *h, const double *xi, const double *wm, const double *Wc, const double *Wcc,
                          const double *emv, int emv_mode, double tp_nu, const double *tp_iK) {
    SSMQ_HANDLE_LOCK(h);
    if (is_mo(h)) return refuse_mo("ssmq_transform_update (use ssmq_transform_update_mo)");
    if (is_trunc(h)) return refuse_trunc("ssmq_transform_update (recreate the handle)");
    if (is_gpqd(h)) return refuse_gpqd("ssmq_transform_update (use ssmq_transform_gpqd_set)");
    if (h && h->form == SSMQ_FORM_TAYLOR1) {
        set_error("transform_update: the linearisation transform has no constants");
        return SSMQ_E_ARG;
    }
    if (is_taylor_gpqd(h)) return refuse_taylor_gpqd("ssmq_transform_update (its kernel parameters are fixed at creation)");
    if (!h) return SSMQ_E_ARG;
    const int D = h->D, E = h->E, N = h->N;
    if (xi) h->xi.assign(xi, xi + D * N);
    if (wm) h->wm.assign(wm, wm + N);
    if (Wc) h->Wc.assign(Wc, Wc + (h->form == SSMQ_FORM_SIGMA ? N : N * N));
    if (Wcc && h->form == SSMQ_FORM_BQ) h->Wcc.assign(Wcc, Wcc + D * N);
    if (emv) h->emv.assign(emv, emv + E * E);
    if (emv_mode == SSMQ_EMV_DIAG || emv_mode == SSMQ_EMV_BROADCAST) h->emv_mode = emv_mode;
    if (tp_iK) h->iK.assign(tp_iK, tp_iK + N * N);
    if (tp_nu > 0.0) {
        if (h->iK.empty()) {
            set_error("transform_update: tp_nu > 0 needs tp_iK");
            return SSMQ_E_ARG;
        }
        h->tp_nu = tp_nu;
    }
    return upload_consts(h);
}

void ssmq_transform_destroy(ssmq_transform *h) {
    if (!h) return;
    {   // whatever context used the handle last has finished with its device blocks (the guard waits for that stream) ...
        SSMQ_HANDLE_LOCK(h);
        if (ssmq::stream()) hipStreamSynchronize(ssmq::stream());
    }   // ... and nobody may hold the handle any more: destroying it while another thread uses it is the caller's error
    if (h->d_mo) hipFree(h->d_mo);
    if (h->d_trunc) hipFree(h->d_trunc);
    if (h->d_gpqd) hipFree(h->d_gpqd);
    if (h->d_small) hipFree(h->d_small);
    if (h->d_wide) hipFree(h->d_wide);
    if (h->d_wc_pad) hipFree(h->d_wc_pad);
    if (h->d_wcx_pad) hipFree(h->d_wcx_pad);
    if (h->d_sx_pad) hipFree(h->d_sx_pad);
    if (h->d_sx_pan) hipFree(h->d_sx_pan);
    if (h->d_wc_blk) hipFree(h->d_wc_blk);
    if (h->d_ik_blk) hipFree(h->d_ik_blk);
    delete h;
}

int ssmq_transform_dims(const ssmq_transform *h, int *D, int *E, int *N) {
    SSMQ_HANDLE_LOCK(h);
    if (!h) return SSMQ_E_ARG;
    if (D) *D = h->D;
    if (E) *E = h->E;
    if (N) *N = h->N;
    return SSMQ_OK;
}

// ---- apply -----------------------------------------------------------------------------------------------------------
int ssmq_apply_batch_dev(ssmq_transform *h, const ssmq_integrand *f, int64_t B, int64_t ld, const double *d_mean,
                         const double *d_cov, const double *d_time, int time_stride, double *d_mean_f,
                         double *d_cov_f, double *d_cov_fx, int32_t *d_status) {
    SSMQ_HANDLE_LOCK(h);
    if (!h || !f) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    return apply_dev_impl(h, f, B, ld, d_mean, d_cov, d_time, time_stride, d_mean_f, d_cov_f, d_cov_fx, d_status,
                          nullptr, nullptr, false);
}

int ssmq_apply_kernel_name(const ssmq_transform *h, const ssmq_integrand *f, char *buf, int len) {
    SSMQ_HANDLE_LOCK(h);
    if (!h || !f || !buf || len <= 0) return SSMQ_E_ARG;
    const char *name = nullptr;
    int rc = apply_dev_impl(const_cast<ssmq_transform *>(h), f, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, &name, true);
    if (rc) return rc;
    snprintf(buf, len, "%s", name ? name : "");
    return SSMQ_OK;
}

}  // extern "C"
