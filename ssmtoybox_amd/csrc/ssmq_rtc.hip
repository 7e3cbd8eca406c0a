// User-defined integrands compiled for the device at run time (ROCm's hiprtc).  A model's function body is registered once
// (ssmq_integrand_define) and becomes `template <> struct Fn<id>` next to the built-in functors of ssmq_device.h; the kernels that
// run it are the AOT ones - k_filter_fused<> (ssmq_filter_fused_kernel.h) and k_apply_small<> (ssmq_apply_small.h) - instantiated
// for the model in one translation unit made of:
//   a prelude (the integer types and NAN, which hiprtc does not declare) | the device headers, embedded into the library at build
//   time (ssmq_rtc_src.inc, made by the Makefile; their host-only parts sit behind #ifndef __HIPCC_RTC__) | the Fn<> wrapper of
//   every user body involved | one explicit instantiation.
// Compiled with the Makefile's -O3 -std=c++17 for the current device's architecture, found by lowered name, loaded as a module and
// launched with the AOT launcher's grid, block and argument struct - the same code as a built-in model up to the functor.
// The streaming Monte-Carlo transform runs a user integrand the same way: k_mc_moments<> (ssmq_mc_moments.h), one explicit
// instantiation per (integrand id, D, E), launched with the arguments ssmq_mc_transform_dev made for the AOT route.
// A body registered with its Jacobian (ssmq_integrand_define_dx) also runs the linearisation and the Taylor-GPQD transform: its
// Fn<> has jac() next to eval(), and k_linearize_fn<> / k_taylor_gpqd_fn<> (ssmq_jacobian_kernel.h) are instantiated per
// (integrand id, D, E, DIN) - the built-in models' kernels reach the model through a run-time switch instead.
// Code objects are cached for the life of the process (key: the body hashes, kernel and template arguments, architecture) - failed
// compiles too, with their message, so a broken body is compiled once - and modules per device.  Locks: the registry of bodies has
// a mutex of its own (held for a lookup only); the cache mutex is held while a kernel is looked up, compiled or loaded, so a
// compile (0.2 - 0.6 s) delays the lookups of other threads for that long - once per kernel and process; the launch itself runs
// outside both.
#include <hip/hiprtc.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "ssmq_host.h"
#include "ssmq_fused.h"
#include "ssmq_innovation_kernel.h"
#include "ssmq_iterated_kernel.h"
#include "ssmq_robust_kernel.h"
#include "ssmq_masked_kernel.h"
#include "ssmq_ipls_kernel.h"
#include "ssmq_filter_shapes.h"
#include "ssmq_mc_moments.h"
#include "ssmq_jacobian_kernel.h"
#include "ssmq_apply_gpqd_kernel.h"
#include "ssmq_pcrlb.h"
#include "ssmq_pcrlb_kernel.h"

namespace ssmq {

static const char kRtcHeaders[] =
#include "ssmq_rtc_src.inc"
    ;

static const char kRtcPrelude[] =
    "typedef __hip_internal::int32_t int32_t;\n"
    "typedef __hip_internal::uint32_t uint32_t;\n"
    "typedef __hip_internal::int64_t int64_t;\n"
    "typedef __hip_internal::uint64_t uint64_t;\n"
    "#define NAN __builtin_nan(\"\")\n";

namespace {

struct UserFn {
    std::string body, jac;                         // jac empty: registered without a Jacobian (ssmq_integrand_define)
    int din, dout;
    bool uses_time;
    uint64_t hash;
};

struct Compiled {
    std::string error;                             // non-empty: the compile failed with this message (nothing to load)
    std::vector<char> code;
    std::string lowered;
    std::map<int, std::pair<hipModule_t, hipFunction_t>> loaded;   // per device
};

std::mutex g_reg_mu;                               // g_user (taken inside g_mu, never the other way round)
std::vector<UserFn> g_user;                        // slot = id - SSMQ_F_USER_FIRST
std::mutex g_mu;                                   // cache, counters, names
std::map<std::string, std::unique_ptr<Compiled>> g_cache;
int64_t g_compiles = 0, g_hits = 0;
double g_compile_s = 0.0;
std::map<std::string, std::string> g_names;        // printable kernel names handed out as const char * (stable storage)

uint64_t fnv1a(const std::string &s, uint64_t h = 1469598103934665603ull) {
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ull;
    }
    return h;
}

// Braces balanced, never closing more than it opened, outside comments and literals; no preprocessor lines, digraphs, raw strings
// or line splices (a backslash before a line break joins two lines before comments are recognised: the end of a `//` comment, or a
// `*` + `/`, would then lie elsewhere for the compiler than for this scan) - each could close the function the body is placed in
// without a visible brace.  Empty string = accepted.
std::string check_body_text(const char *body);
// ... `what` names the body in the message ("integrand body" / "Jacobian body")
std::string check_body(const char *body, const char *what = "integrand body") {
    std::string why = check_body_text(body);
    if (!why.empty() && strcmp(what, "integrand body") != 0) why.replace(0, strlen("integrand body"), what);
    return why;
}
std::string check_body_text(const char *body) {
    const size_t n = strlen(body);
    if (n == 0) return "integrand body is empty";
    if (n > SSMQ_USER_BODY_MAX) return "integrand body is longer than SSMQ_USER_BODY_MAX (" + std::to_string(SSMQ_USER_BODY_MAX) + ") characters";
    for (size_t i = 0; i < n; ++i) {   // (clang also splices a backslash followed by blanks and then the line break)
        if (body[i] != '\\') continue;
        size_t j = i + 1;
        while (j < n && (body[j] == ' ' || body[j] == '\t' || body[j] == '\v' || body[j] == '\f')) ++j;
        if (j < n && (body[j] == '\n' || body[j] == '\r'))
            return "integrand body: line continuations (a backslash before a line break) are not allowed";
    }
    int depth = 0;
    for (size_t i = 0; i < n; ++i) {
        const char c = body[i], d = i + 1 < n ? body[i + 1] : '\0';
        if (c == '/' && d == '/') {
            while (i < n && body[i] != '\n') ++i;
            continue;
        }
        if (c == '/' && d == '*') {
            const char *e = strstr(body + i + 2, "*/");
            if (!e) return "integrand body: unterminated comment";
            i = (size_t)(e - body) + 1;
            continue;
        }
        if (c == '"' || c == '\'') {
            if (i > 0 && (body[i - 1] == 'R')) return "integrand body: raw string literals are not allowed";
            size_t j = i + 1;
            while (j < n && body[j] != c && body[j] != '\n') j += body[j] == '\\' ? 2 : 1;
            if (j >= n || body[j] != c) return "integrand body: unterminated literal";
            i = j;
            continue;
        }
        if (c == '#') return "integrand body: preprocessor directives are not allowed";
        if (c == '\\') return "integrand body: backslashes are only allowed inside literals";
        if ((c == '<' && d == '%') || (c == '%' && (d == '>' || d == ':'))) return "integrand body: digraphs are not allowed";
        if (c == '{') ++depth;
        if (c == '}' && --depth < 0) return "integrand body: unbalanced braces ('}' without '{')";
    }
    if (depth != 0) return "integrand body: unbalanced braces (" + std::to_string(depth) + " '{' not closed)";
    return "";
}

bool user_fn(int id, UserFn *out) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!is_user_integrand(id) || id - SSMQ_F_USER_FIRST >= (int)g_user.size()) return false;
    *out = g_user[id - SSMQ_F_USER_FIRST];
    return true;
}

std::string wrapper(int id, const UserFn &u) {
    std::string s;
    s += "namespace ssmq {\ntemplate <>\nstruct Fn<" + std::to_string(id) + "> {\n";
    s += "    static constexpr int DIN = " + std::to_string(u.din) + ";\n";
    s += std::string("    static constexpr bool HAS_JAC = ") + (u.jac.empty() ? "false" : "true") + ";\n";
    s += "    double t_;\n    const FPar *fp_;\n";
    s += "    __device__ __forceinline__ void init(double t, const FPar &par) { t_ = t; fp_ = &par; }\n";
    s += "    template <int E>\n    __device__ __forceinline__ void eval(const double *x, double *o) const {\n";
    s += "        const double t = t_;\n        const double *p = fp_->p;\n        (void)t; (void)p; (void)x; (void)o;\n        {\n";
    s += "#line 1 \"user_integrand_" + std::to_string(id) + "\"\n";
    s += u.body;
    s += "\n        }\n    }\n";
    if (!u.jac.empty()) {
        // J: dout x DIN entries at pitch ldj, all zero on entry
        s += "    __device__ __forceinline__ void jac(const double *x, double *J, const int ldj) const {\n";
        s += "        const double t = t_;\n        const double *p = fp_->p;\n        (void)t; (void)p; (void)x; (void)J; (void)ldj;\n        {\n";
        s += "#line 1 \"user_jacobian_" + std::to_string(id) + "\"\n";
        s += u.jac;
        s += "\n        }\n    }\n";
    }
    s += "};\n}  // namespace ssmq\n";
    return s;
}

std::string first_lines(const std::string &log, int lines) {
    size_t pos = 0;
    for (int k = 0; k < lines && pos != std::string::npos; ++k) {
        pos = log.find('\n', pos);
        if (pos != std::string::npos) ++pos;
    }
    return pos == std::string::npos ? log : log.substr(0, pos);
}

// Compiles (or finds) the program that instantiates the kernel `expr`, whose one parameter is a `const arg_type`, for the user
// integrands `ids`; g_mu held.  remarks: also ask the compiler for its resource-usage remarks (compile check only; they do not
// change the code).
int compile(const std::string &expr, const char *arg_type, const std::vector<int> &ids, const std::string &arch, Compiled **out,
            std::string *log, bool remarks) {
    std::string key = expr + "|" + arch;
    std::string wrappers;
    for (int id : ids) {
        UserFn u;
        if (!user_fn(id, &u)) {
            set_error("integrand id " + std::to_string(id) + " is not a registered user integrand");
            return SSMQ_E_ARG;
        }
        char hx[32];
        snprintf(hx, sizeof(hx), "|%016llx", (unsigned long long)u.hash);
        key += hx;
        wrappers += wrapper(id, u);
    }
    if (!remarks) {
        auto it = g_cache.find(key);
        if (it != g_cache.end()) {
            ++g_hits;
            if (!it->second->error.empty()) {
                set_error(it->second->error);
                return SSMQ_E_UNSUPPORTED;
            }
            *out = it->second.get();
            return SSMQ_OK;
        }
    }
    std::string src = kRtcPrelude;
    src += kRtcHeaders;
    src += wrappers;
    src += "template __global__ void " + expr + "(const " + arg_type + ");\n";
    const auto t0 = std::chrono::steady_clock::now();
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "ssmq_user.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        set_error("hiprtcCreateProgram failed");
        return SSMQ_E_HIP;
    }
    hiprtcAddNameExpression(prog, expr.c_str());
    const std::string arch_opt = "--offload-arch=" + arch;
    std::vector<const char *> opts = {arch_opt.c_str(), "-O3", "-std=c++17"};
    if (remarks) opts.push_back("-Rpass-analysis=kernel-resource-usage");
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string lg(ls, '\0');
    if (ls) hiprtcGetProgramLog(prog, &lg[0]);
    while (!lg.empty() && lg.back() == '\0') lg.pop_back();
    if (log) *log = lg;
    if (rc != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        const std::string msg = "run-time compilation of " + expr + " failed: " + first_lines(lg, 12);
        set_error(msg);
        ++g_compiles;
        g_compile_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!remarks) {
            auto c = std::unique_ptr<Compiled>(new Compiled);
            c->error = msg;
            g_cache[key] = std::move(c);
        }
        return SSMQ_E_UNSUPPORTED;
    }
    const char *lowered = nullptr;
    size_t cs = 0;
    auto c = std::unique_ptr<Compiled>(new Compiled);
    if (hiprtcGetLoweredName(prog, expr.c_str(), &lowered) != HIPRTC_SUCCESS || !lowered || hiprtcGetCodeSize(prog, &cs) != HIPRTC_SUCCESS ||
        cs == 0) {
        hiprtcDestroyProgram(&prog);
        set_error("run-time compilation of " + expr + ": no code object / lowered name");
        return SSMQ_E_HIP;
    }
    c->lowered = lowered;
    c->code.resize(cs);
    hiprtcGetCode(prog, c->code.data());
    hiprtcDestroyProgram(&prog);
    ++g_compiles;
    g_compile_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    Compiled *p = c.get();
    if (remarks) {
        static std::unique_ptr<Compiled> last_check;   // (compile checks are not cached: the remarks are wanted every time)
        last_check = std::move(c);
    } else {
        g_cache[key] = std::move(c);
    }
    *out = p;
    return SSMQ_OK;
}

int device_arch(std::string *arch, int *dev) {
    static thread_local std::map<int, std::string> known;      // (per thread: no lock; properties are asked once per device)
    SSMQ_HIP(hipGetDevice(dev));
    auto it = known.find(*dev);
    if (it == known.end()) {
        hipDeviceProp_t p;
        SSMQ_HIP(hipGetDeviceProperties(&p, *dev));
        std::string a = p.gcnArchName;      // "gfx950:sramecc+:xnack-": the Makefile builds for the processor alone
        it = known.emplace(*dev, a.substr(0, a.find(':'))).first;
    }
    *arch = it->second;
    return SSMQ_OK;
}

int function_of(Compiled *c, int dev, hipFunction_t *fn) {   // g_mu held
    auto it = c->loaded.find(dev);
    if (it != c->loaded.end()) {
        *fn = it->second.second;
        return SSMQ_OK;
    }
    hipModule_t m;
    SSMQ_HIP(hipModuleLoadData(&m, c->code.data()));
    hipFunction_t f;
    hipError_t e = hipModuleGetFunction(&f, m, c->lowered.c_str());
    if (e != hipSuccess) {
        hipModuleUnload(m);
        return hip_fail(e, "hipModuleGetFunction");
    }
    c->loaded[dev] = {m, f};
    *fn = f;
    return SSMQ_OK;
}

// The loaded kernel for `expr` on the current device: compiled, or found in the cache, under g_mu; the launch is the caller's.
int kernel_for(const std::string &expr, const char *arg_type, const std::vector<int> &ids, hipFunction_t *fn) {
    std::string arch;
    int dev = 0;
    int rc = device_arch(&arch, &dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    Compiled *c = nullptr;
    if ((rc = compile(expr, arg_type, ids, arch, &c, nullptr, false))) return rc;
    return function_of(c, dev, fn);
}

const char *stable_name(const std::string &s) {   // g_mu held
    auto it = g_names.find(s);
    if (it == g_names.end()) it = g_names.emplace(s, s).first;
    return it->second.c_str();
}

// The tail of every launcher: the printable name, the dry run (SSMQ_OK, nothing compiled), the kernel, its launch with the one
// argument block `arg`; `what` names the launch in an error
int launch_compiled(const std::string &expr, const char *arg_type, const std::vector<int> &ids, void *arg, unsigned grid, unsigned block,
                    hipStream_t s, const char **name, bool dry_run, const char *what) {
    if (name) {
        std::lock_guard<std::mutex> lk(g_mu);
        *name = stable_name(expr.substr(6) + " (run-time compiled)");
    }
    if (dry_run) return SSMQ_OK;
    hipFunction_t fn;
    const int rc = kernel_for(expr, arg_type, ids, &fn);
    if (rc) return rc;
    void *args[] = {arg};
    return hip_fail(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, s, args, nullptr), what);
}

std::string fused_expr(int D, int Y, int ND, int NO, int FD, int FO, int form, int tp, int selo, int opt, int stu) {
    char b[256];
    snprintf(b, sizeof(b), "ssmq::k_filter_fused<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d>", D, Y, ND, NO, FD, FO, form, tp, selo,
             opt, stu);
    return b;
}
std::string innovation_expr(int D, int Y, int ND, int NO, int FD, int FO, int form, int tp, int selo, int opt) {
    char b[256];
    snprintf(b, sizeof(b), "ssmq::k_innovation<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d>", D, Y, ND, NO, FD, FO, form, tp, selo, opt);
    return b;
}
// The whole-pass kernels of the measurement-update variants and of the iterated smoother: kind, kernel, the format of its template
// id (D, Y, ND, NO, FD, FO, FORM, TP, SELO; the three passes: the dense kernel, OPT 0), its argument type, what errors call the pass
struct PassKernel {
    int kind;
    const char *kernel, *expr_fmt, *args_type, *pass;
};
static const PassKernel kPassKernels[] = {
    {SSMQ_RTC_ITERATED, "k_iplf_loop", "ssmq::k_iplf_loop<%d, %d, %d, %d, %d, %d, %d, %d, %d, 0>", "ssmq::IplfArgs", "iterated pass"},
    {SSMQ_RTC_ROBUST, "k_robust_loop", "ssmq::k_robust_loop<%d, %d, %d, %d, %d, %d, %d, %d, %d, 0>", "ssmq::RobustArgs", "robust pass"},
    {SSMQ_RTC_MASKED, "k_masked_loop", "ssmq::k_masked_loop<%d, %d, %d, %d, %d, %d, %d, %d, %d, 0>", "ssmq::MaskedArgs", "masked pass"},
    {SSMQ_RTC_SMOOTHER_ITERATED, "k_ipls_pass", "ssmq::k_ipls_pass<%d, %d, %d, %d, %d, %d, %d, %d, %d>", "ssmq::IplsArgs", "iterated smoother"},
};
static const PassKernel *pass_kernel(int kind) {
    for (const PassKernel &k : kPassKernels)
        if (k.kind == kind) return &k;
    return nullptr;
}
static std::string pass_expr(const PassKernel &k, int D, int Y, int ND, int NO, int FD, int FO, int form, int tp, int selo) {
    char b[256];
    snprintf(b, sizeof(b), k.expr_fmt, D, Y, ND, NO, FD, FO, form, tp, selo);
    return b;
}
std::string apply_expr(int D, int E, int N, int F, int form, int tp, int sel, int opt, bool nts) {
    char b[256];
    snprintf(b, sizeof(b), "ssmq::k_apply_small<%d, %d, %d, %d, %d, %d, %d, %d, %s>", D, E, N, F, form, tp, sel, opt, nts ? "true" : "false");
    return b;
}

// Shape range of the run-time route (the span of the AOT table kFused): D <= 6, Y <= 4, point counts up to 2 D + 1.
bool shape_ok(int D, int E, int N, std::string *why) {
    if (D < 1 || D > SSMQ_USER_MAX_D || E < 1 || E > std::max(D, SSMQ_USER_MAX_Y) || N < 2 || N > 2 * D + 1) {
        *why = "user integrands run for D <= " + std::to_string(SSMQ_USER_MAX_D) + ", outputs <= max(D, " + std::to_string(SSMQ_USER_MAX_Y) +
               ") and 2 .. 2 D + 1 points (got D = " + std::to_string(D) + ", E = " + std::to_string(E) + ", N = " + std::to_string(N) + ")";
        return false;
    }
    return true;
}

// The fast-path variant: as the AOT route, which has the LDL' / unscented-point variants for the D >= 5 shapes only (kFused,
// SSMQ_SHAPE_FAST in ssmq_filter_shapes.h; ssmq_small_*.hip, SSMQ_SMALL_FAST) - below that the dense kernel, so a restated built-in model runs the same code.
int pick_opt_fused(const ssmq_transform *hd, const ssmq_transform *ho) {
    if (hd->D < 5) return 0;
    const auto want = opt_preference(hd, ho);     // as the AOT tables: the best fast path both handles qualify for
    return want[0] >= 0 ? want[0] : want[1];
}

}  // namespace

int refuse_user_integrand(const char *what) {
    set_error(std::string(what) + ": user-defined integrands run on ssmq_filter_forward_dev / ssmq_student_filter_forward_dev "
              "(additive noise) and ssmq_apply_batch[_dev] only");
    return SSMQ_E_UNSUPPORTED;
}

bool user_integrand_info(int id, FInfo *o) {
    UserFn u;
    if (!user_fn(id, &u)) return false;
    *o = {u.din, u.dout, u.uses_time};
    return true;
}

static int check_user_pair(const ssmq_integrand *fd, const ssmq_integrand *fo, std::vector<int> *ids) {
    for (const ssmq_integrand *f : {fd, fo}) {
        if (f->n_idx != 0) {
            set_error("user integrands take the leading state entries: no state index (n_idx = 0)");
            return SSMQ_E_UNSUPPORTED;
        }
        if (f->n_par < 0 || f->n_par > SSMQ_MAX_FPAR) {
            set_error("integrand: n_par out of range");
            return SSMQ_E_ARG;
        }
        if (is_user_integrand(f->id) && (ids->empty() || ids->back() != f->id)) ids->push_back(f->id);
    }
    return SSMQ_OK;
}

// The checks of a pair with a user member that runs ONE kernel instantiated for it (the time loop, the innovation scores): the ids
// to compile for, both transforms of one form and in the shape range, dimensions that fit
static int user_pair_shape(const FilterPass &p, std::vector<int> *ids_out) {
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    const ssmq_integrand *fd = p.fd, *fo = p.fo;
    std::vector<int> &ids = *ids_out;
    int rc = check_user_pair(fd, fo, &ids);
    if (rc) return rc;
    FInfo id_, io_;
    if (!integrand_info(fd->id, &id_) || !integrand_info(fo->id, &io_)) {
        set_error("unknown integrand id");
        return SSMQ_E_ARG;
    }
    const int D = hd->D, Y = ho->E;
    std::string why;
    if (!shape_ok(D, D, hd->N, &why) || !shape_ok(D, Y, ho->N, &why) || Y > SSMQ_USER_MAX_Y) {
        if (why.empty()) why = "user integrands: at most " + std::to_string(SSMQ_USER_MAX_Y) + " measurements";
        set_error(why);
        return SSMQ_E_UNSUPPORTED;
    }
    if (hd->form != ho->form || (hd->tp_nu > 0.0) != (ho->tp_nu > 0.0) || p.sel_obs != 0 || hd->form == SSMQ_FORM_TAYLOR1 ||
        is_taylor_gpqd(hd) || is_trunc(hd) || is_trunc(ho) || is_gpqd(hd)) {
        set_error("user integrands: both transforms of one form (sigma-point or BQ), no linearisation, no state index");
        return SSMQ_E_UNSUPPORTED;
    }
    if (id_.dout != D || id_.din > D || (io_.dout ? io_.dout : Y) != Y || io_.din > D) {
        set_error("user integrands: input / output dimensions do not match the transforms");
        return SSMQ_E_ARG;
    }
    return SSMQ_OK;
}

int rtc_launch_fused(const FilterPass &p) {
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    const ssmq_integrand *fd = p.fd, *fo = p.fo;
    std::vector<int> ids;
    int rc = user_pair_shape(p, &ids);
    if (rc) return rc;
    const int D = hd->D, Y = ho->E;
    const int tp = hd->tp_nu > 0.0 ? 1 : 0, opt = pick_opt_fused(hd, ho);
    const int stu = (p.sscale != nullptr && p.student_dof > 0.0) ? 1 : 0;
    // scalar state: recursion type fixed at compile time, as the AOT table does (SSMQ_FUSED_ONE_S)
    const std::string expr = fused_expr(D, Y, hd->N, ho->N, fd->id, fo->id, hd->form, tp, 0, opt, D == 1 && Y == 1 ? stu : -1);
    const char *what = "k_filter_fused (run-time compiled)";
    if (p.dry_run) {
        rc = launch_compiled(expr, "ssmq::FusedArgs", ids, nullptr, 0, kSmallBlock, p.s, p.name, true, what);
        return rc ? rc : 1;
    }
    // A built-in member with a host time table (UNGM) is read through that table at every step of the loop, unconditionally: the
    // caller must have uploaded it (filter_forward_impl does, with the pass's constants).
    FusedArgs a = fused_args(p);
    for (const ssmq_integrand *f : {fd, fo}) {
        const double *tab = f == fd ? a.fd.ttab : a.fo.ttab;
        if (!is_user_integrand(f) && has_time_table(f->id) && !tab) {
            set_error("run-time compiled filter: the time table of built-in integrand " + std::to_string(f->id) + " is missing");
            return SSMQ_E_ARG;
        }
    }
    if (is_user_integrand(fd)) a.fd.ttab = nullptr;   // (user integrands evaluate their time dependence themselves)
    if (is_user_integrand(fo)) a.fo.ttab = nullptr;
    rc = launch_compiled(expr, "ssmq::FusedArgs", ids, &a, (unsigned)((a.B + a.lpw - 1) / a.lpw), kSmallBlock, p.s, p.name, false, what);
    return rc ? rc : 1;
}

// k_innovation<> (ssmq_score_step.h) for a pair with a user member: the shapes, the fast-path choice and the time tables
// of rtc_launch_fused, the grid and the argument block of the AOT launcher (ssmq_innovation.hip)
int rtc_launch_innovation(const FilterPass &p, const InnovOut &o) {
    std::vector<int> ids;
    int rc = user_pair_shape(p, &ids);
    if (rc) return rc;
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    const std::string expr = innovation_expr(hd->D, ho->E, hd->N, ho->N, p.fd->id, p.fo->id, hd->form, hd->tp_nu > 0.0 ? 1 : 0, 0, pick_opt_fused(hd, ho));
    const char *what = "k_innovation (run-time compiled)";
    if (p.dry_run) {
        rc = launch_compiled(expr, "ssmq::InnovArgs", ids, nullptr, 0, kSmallBlock, p.s, p.name, true, what);
        return rc ? rc : 1;
    }
    InnovArgs a = innov_args(p, o);
    for (const ssmq_integrand *f : {p.fd, p.fo}) {
        const double *tab = f == p.fd ? a.fd.ttab : a.fo.ttab;
        if (!is_user_integrand(f) && has_time_table(f->id) && !tab) {
            set_error("run-time compiled innovation scores: the time table of built-in integrand " + std::to_string(f->id) + " is missing");
            return SSMQ_E_ARG;
        }
    }
    if (is_user_integrand(p.fd)) a.fd.ttab = nullptr;   // (user integrands evaluate their time dependence themselves)
    if (is_user_integrand(p.fo)) a.fo.ttab = nullptr;
    rc = launch_compiled(expr, "ssmq::InnovArgs", ids, &a, (unsigned)a.T * (unsigned)a.nblk, kSmallBlock, p.s, p.name, false, what);
    return rc ? rc : 1;
}

// A whole-pass kernel of kPassKernels for a pair with a user member: the shape checks and the time tables of rtc_launch_innovation,
// the grid of the AOT launchers; the caller built the argument block as for them
int rtc_launch_pass(const FilterPass &p, int kind, void *args, FPar *fd, FPar *fo, int64_t B) {
    const PassKernel *found = pass_kernel(kind);
    if (!found) {
        set_error("rtc_launch_pass: not a whole-pass kernel kind");
        return SSMQ_E_ARG;
    }
    const PassKernel &pk = *found;
    std::vector<int> ids;
    int rc = user_pair_shape(p, &ids);
    if (rc) return rc;
    const ssmq_transform *hd = p.hd, *ho = p.ho;
    const std::string expr = pass_expr(pk, hd->D, ho->E, hd->N, ho->N, p.fd->id, p.fo->id, hd->form, hd->tp_nu > 0.0 ? 1 : 0, 0);
    const std::string what = std::string(pk.kernel) + " (run-time compiled)";
    if (p.dry_run) {
        rc = launch_compiled(expr, pk.args_type, ids, nullptr, 0, kSmallBlock, p.s, p.name, true, what.c_str());
        return rc ? rc : 1;
    }
    for (const ssmq_integrand *f : {p.fd, p.fo}) {
        const double *tab = f == p.fd ? fd->ttab : fo->ttab;
        if (!is_user_integrand(f) && has_time_table(f->id) && !tab) {
            set_error(std::string("run-time compiled ") + pk.pass + ": the time table of built-in integrand " + std::to_string(f->id) + " is missing");
            return SSMQ_E_ARG;
        }
    }
    if (is_user_integrand(p.fd)) fd->ttab = nullptr;   // (user integrands evaluate their time dependence themselves)
    if (is_user_integrand(p.fo)) fo->ttab = nullptr;
    rc = launch_compiled(expr, pk.args_type, ids, args, (unsigned)((B + kSmallBlock - 1) / kSmallBlock), kSmallBlock, p.s, p.name, false, what.c_str());
    return rc ? rc : 1;
}

int rtc_launch_apply(const ssmq_transform *h, const ssmq_integrand *f, int sel, const ApplyArgs &a0, hipStream_t s, const char **name,
                     bool dry_run) {
    std::vector<int> ids;
    int rc = check_user_pair(f, f, &ids);
    if (rc) return rc;
    std::string why;
    if (!shape_ok(h->D, h->E, h->N, &why)) {
        set_error(why);
        return SSMQ_E_UNSUPPORTED;
    }
    if (sel != 0 || h->form == SSMQ_FORM_TAYLOR1 || is_taylor_gpqd(h) || is_trunc(h) || is_gpqd(h)) {
        set_error("user integrands: sigma-point or BQ transforms only, no state index");
        return SSMQ_E_UNSUPPORTED;
    }
    const int tp = h->tp_nu > 0.0 ? 1 : 0;
    int opt = 0;
    if (h->D >= 5) {   // the AOT selection (apply_dev_impl) over the variants SSMQ_SMALL_FAST instantiates
        const int want[5] = {(!tp && (h->opt_mask & 7) == 7) ? 7 : -1, h->opt_mask & (tp ? SSMQ_OPT_UT : 3), h->opt_mask & SSMQ_OPT_UT,
                             h->opt_mask & SSMQ_OPT_LDL & (tp ? 0 : 1), 0};
        for (int k = 0; k < 5; ++k) {
            const int w = want[k];
            const bool have = w == 0 || (h->form == SSMQ_FORM_BQ && !tp && (w == 7 || w == 3 || w == 1)) ||
                              (w == SSMQ_OPT_UT && (tp || h->form == SSMQ_FORM_SIGMA));
            if (w >= 0 && have) {
                opt = w;
                break;
            }
        }
    }
    const bool nts = opt != 0 && a0.stream_out;
    const std::string expr = apply_expr(h->D, h->E, h->N, f->id, h->form, tp, 0, opt, nts);
    ApplyArgs a = a0;
    a.fp.ttab = nullptr;
    return launch_compiled(expr, "ssmq::ApplyArgs", ids, &a, (unsigned)((a.B + kSmallBlock - 1) / kSmallBlock), kSmallBlock, s, name, dry_run,
                           "k_apply_small (run-time compiled)");
}

bool user_integrand_has_jacobian(int id) {
    UserFn u;
    return user_fn(id, &u) && !u.jac.empty();
}

// The two Jacobian kernels of a user integrand (form: SSMQ_FORM_TAYLOR1 or SSMQ_FORM_TAYLOR_GPQD): the checks of the route, the
// instantiation k_<kernel>_fn<id, D, E, DIN> and the type of its argument block
struct JacKernel {
    const char *kernel, *what, *arg_type;
};
static JacKernel jac_kernel(int form) {
    return form == SSMQ_FORM_TAYLOR1 ? JacKernel{"k_linearize_fn", "linearisation", "ssmq::LinArgs"}
                                     : JacKernel{"k_taylor_gpqd_fn", "Taylor-GPQD", "ssmq::TaylorGpqdArgs"};
}
static int jac_expr(int form, int D, int E, const ssmq_integrand *f, std::string *expr, std::vector<int> *ids) {
    const char *kernel = jac_kernel(form).kernel, *what = jac_kernel(form).what;
    int rc = check_user_pair(f, f, ids);
    if (rc) return rc;
    UserFn u;
    if (!user_fn(f->id, &u)) {
        set_error("integrand id " + std::to_string(f->id) + " is not a registered user integrand");
        return SSMQ_E_ARG;
    }
    if (u.jac.empty()) {
        set_error(std::string(what) + ": this model has no Jacobian (a user integrand gets one through ssmq_integrand_define_dx)");
        return SSMQ_E_UNSUPPORTED;
    }
    std::string why;
    if (!shape_ok(D, E, 2, &why)) {      // (no points: the count is not part of the range)
        set_error(std::string(what) + ": user integrands run for D <= " + std::to_string(SSMQ_USER_MAX_D) + " and outputs <= max(D, " +
                  std::to_string(SSMQ_USER_MAX_Y) + ") (got D = " + std::to_string(D) + ", E = " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    if (u.dout != E || u.din > D) {
        set_error(std::string(what) + ": the user integrand's input / output dimensions do not match the transform");
        return SSMQ_E_ARG;
    }
    char b[160];
    snprintf(b, sizeof(b), "ssmq::%s<%d, %d, %d, %d>", kernel, f->id, D, E, u.din);
    *expr = b;
    return SSMQ_OK;
}
int rtc_launch_jacobian(int form, const ssmq_integrand *f, const TaylorGpqdArgs &a0, hipStream_t s, const char **name, bool dry_run) {
    std::string expr;
    std::vector<int> ids;
    const int rc = jac_expr(form, a0.D, a0.E, f, &expr, &ids);
    if (rc) return rc;
    TaylorGpqdArgs a = a0;      // (k_linearize_fn takes the LinArgs it begins with)
    a.fp.ttab = nullptr;
    return launch_compiled(expr, jac_kernel(form).arg_type, ids, static_cast<LinArgs *>(&a), (unsigned)((a.B + 255) / 256), 256, s, name,
                           dry_run, jac_kernel(form).kernel);      // grid and block as launch_jacobian
}
int rtc_prepare_jacobian(const ssmq_transform *h, const ssmq_integrand *f) {
    if (h->form != SSMQ_FORM_TAYLOR1 && !is_taylor_gpqd(h)) {
        set_error("rtc_prepare_jacobian: neither a linearisation nor a Taylor-GPQD handle");
        return SSMQ_E_ARG;
    }
    std::string expr;
    std::vector<int> ids;
    const int rc = jac_expr(h->form, h->D, h->E, f, &expr, &ids);
    if (rc) return rc;
    hipFunction_t fn;
    return kernel_for(expr, jac_kernel(h->form).arg_type, ids, &fn);
}

// The GPQ+D kernel of a user integrand that has a Jacobian: k_apply_gpqd<id, D, E, DIN> (observations in registers) or
// k_apply_gpqd_lds<id, D, E, DIN>, as launch_apply_gpqd chooses for the built-in models
static int gpqd_expr(int D, int E, bool lds, const ssmq_integrand *f, std::string *expr, std::vector<int> *ids) {
    int rc = check_user_pair(f, f, ids);
    if (rc) return rc;
    UserFn u;
    if (!user_fn(f->id, &u)) {
        set_error("integrand id " + std::to_string(f->id) + " is not a registered user integrand");
        return SSMQ_E_ARG;
    }
    if (u.jac.empty()) {
        set_error("GPQ+D: this model has no Jacobian (a user integrand gets one through ssmq_integrand_define_dx)");
        return SSMQ_E_UNSUPPORTED;
    }
    if (!gpqd_range_ok(D, E, 2)) {
        set_error("GPQ+D: user integrands run for D <= " + std::to_string(SSMQ_USER_MAX_D) + " and outputs <= max(D, " +
                  std::to_string(SSMQ_USER_MAX_Y) + ") (got D = " + std::to_string(D) + ", E = " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    if (u.dout != E || u.din > D) {
        set_error("GPQ+D: the user integrand's input / output dimensions do not match the transform");
        return SSMQ_E_ARG;
    }
    char b[160];
    snprintf(b, sizeof(b), "ssmq::%s<%d, %d, %d, %d>", lds ? "k_apply_gpqd_lds" : "k_apply_gpqd", f->id, D, E, u.din);
    *expr = b;
    return SSMQ_OK;
}
int rtc_launch_gpqd(const ssmq_integrand *f, const GpqdArgs &a0, bool lds, hipStream_t s, const char **name, bool dry_run) {
    std::string expr;
    std::vector<int> ids;
    const int rc = gpqd_expr(a0.D, a0.E, lds, f, &expr, &ids);
    if (rc) return rc;
    GpqdArgs a = a0;
    a.fp.ttab = nullptr;
    const int ipw = gpqd_lds_items(a.D, a.E);      // grid and block as launch_apply_gpqd
    return launch_compiled(expr, "ssmq::GpqdArgs", ids, &a, lds ? (unsigned)((a.B + ipw - 1) / ipw) : (unsigned)((a.B + 255) / 256),
                           lds ? kGpqdLdsBlock : 256, s, name, dry_run, lds ? "k_apply_gpqd_lds" : "k_apply_gpqd");
}
int rtc_prepare_gpqd(const ssmq_transform *h, const ssmq_integrand *f) {
    if (!is_gpqd(h)) {
        set_error("rtc_prepare_gpqd: not a GPQ+D handle");
        return SSMQ_E_ARG;
    }
    std::string expr;
    std::vector<int> ids;
    const int rc = gpqd_expr(h->D, h->E, h->D > kGpqdRegMaxD, f, &expr, &ids);
    if (rc) return rc;
    hipFunction_t fn;
    return kernel_for(expr, "ssmq::GpqdArgs", ids, &fn);
}

// The posterior Cramer-Rao kernel of a user integrand that has a Jacobian: k_pcrlb_dyn_fn<id, D, DIN> (a D -> D transition) or
// k_pcrlb_obs_fn<id, D, E, DIN> (ssmq_pcrlb_kernel.h); D <= 6, a measurement's E <= 4
static int pcrlb_expr(bool dyn, int D, int E, const ssmq_integrand *f, std::string *expr, std::vector<int> *ids) {
    const char *kernel = dyn ? "k_pcrlb_dyn_fn" : "k_pcrlb_obs_fn";
    int rc = check_user_pair(f, f, ids);
    if (rc) return rc;
    UserFn u;
    if (!user_fn(f->id, &u)) {
        set_error("integrand id " + std::to_string(f->id) + " is not a registered user integrand");
        return SSMQ_E_ARG;
    }
    if (u.jac.empty()) {
        set_error(std::string(kernel) + ": this model has no Jacobian (a user integrand gets one through ssmq_integrand_define_dx)");
        return SSMQ_E_UNSUPPORTED;
    }
    if (D < 1 || D > kPcrlbMaxD || E < 1 || (dyn ? E != D : E > kPcrlbMaxY)) {
        set_error(std::string(kernel) + ": user integrands run for D <= " + std::to_string(kPcrlbMaxD) + (dyn ? " and D outputs" : " and outputs <= " +
                  std::to_string(kPcrlbMaxY)) + " (got D = " + std::to_string(D) + ", E = " + std::to_string(E) + ")");
        return SSMQ_E_UNSUPPORTED;
    }
    if (u.dout != E || u.din > D) {
        set_error(std::string(kernel) + ": the user integrand's input / output dimensions do not match the model");
        return SSMQ_E_ARG;
    }
    char b[160];
    if (dyn) snprintf(b, sizeof(b), "ssmq::k_pcrlb_dyn_fn<%d, %d, %d>", f->id, D, u.din);
    else snprintf(b, sizeof(b), "ssmq::k_pcrlb_obs_fn<%d, %d, %d, %d>", f->id, D, E, u.din);
    *expr = b;
    return SSMQ_OK;
}
int rtc_launch_pcrlb(bool dyn, const ssmq_integrand *f, const PcrlbArgs &a0, unsigned grid, hipStream_t s, const char **name, bool dry_run) {
    std::string expr;
    std::vector<int> ids;
    const int rc = pcrlb_expr(dyn, a0.lin.D, a0.lin.E, f, &expr, &ids);
    if (rc) return rc;
    PcrlbArgs a = a0;
    a.lin.fp.ttab = nullptr;
    return launch_compiled(expr, "ssmq::PcrlbArgs", ids, &a, grid, kPcrlbBlock, s, name, dry_run, dyn ? "k_pcrlb_dyn_fn" : "k_pcrlb_obs_fn");
}

// k_mc_moments<> for a user integrand (ssmq_mc_transform.hip has checked the range and filled `a0`): SSMQ_OK launched, or < 0
int rtc_launch_mc(const ssmq_integrand *f, int D, int E, const McMomArgs &a0, unsigned grid, hipStream_t s) {
    char b[128];
    snprintf(b, sizeof(b), "ssmq::k_mc_moments<%d, %d, %d, 0>", f->id, D, E);
    McMomArgs a = a0;
    a.fp.ttab = nullptr;
    return launch_compiled(b, "ssmq::McMomArgs", {f->id}, &a, grid, kMcBlock, s, nullptr, false, "k_mc_moments (run-time compiled)");
}

}  // namespace ssmq

using namespace ssmq;

// jac: null for ssmq_integrand_define (an entry without a Jacobian), the Jacobian body for ssmq_integrand_define_dx.  An entry is
// found again by (body, Jacobian body, din, dout): the same body with and without a Jacobian, or with two Jacobians, are
// different integrands with different kernels.
static int define_impl(const char *fn, const char *body, const char *jac, int din, int dout, int uses_time, int32_t *id) {
    if (!body || !id) {
        set_error(std::string(fn) + ": null argument");
        return SSMQ_E_ARG;
    }
    if (din < 1 || din > SSMQ_MAX_DIM || dout < 1 || dout > SSMQ_MAX_DIM) {
        set_error(std::string(fn) + ": din and dout must be in 1 .. " + std::to_string(SSMQ_MAX_DIM));
        return SSMQ_E_ARG;
    }
    std::string why = check_body(body);
    if (why.empty() && jac) why = check_body(jac, "Jacobian body");
    if (!why.empty()) {
        set_error(why);
        return SSMQ_E_ARG;
    }
    const std::string jb = jac ? jac : "";
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (size_t k = 0; k < g_user.size(); ++k) {
        UserFn &u = g_user[k];
        if (u.body == body && u.jac == jb && u.din == din && u.dout == dout) {
            u.uses_time = u.uses_time || uses_time != 0;
            *id = SSMQ_F_USER_FIRST + (int32_t)k;
            return SSMQ_OK;
        }
    }
    if ((int)g_user.size() >= SSMQ_F_USER_SLOTS) {
        set_error(std::string(fn) + ": all " + std::to_string(SSMQ_F_USER_SLOTS) + " user integrand slots are taken");
        return SSMQ_E_UNSUPPORTED;
    }
    UserFn u{body, jb, din, dout, uses_time != 0, 0};
    u.hash = fnv1a(u.body, fnv1a(std::to_string(din) + "," + std::to_string(dout)));
    if (jac) u.hash = fnv1a(u.jac, fnv1a("|dx|", u.hash));
    g_user.push_back(u);
    *id = SSMQ_F_USER_FIRST + (int32_t)(g_user.size() - 1);
    return SSMQ_OK;
}

extern "C" int ssmq_integrand_define(const char *body, int din, int dout, int uses_time, int32_t *id) {
    return define_impl("ssmq_integrand_define", body, nullptr, din, dout, uses_time, id);
}

extern "C" int ssmq_integrand_define_dx(const char *body, const char *jac_body, int din, int dout, int uses_time, int32_t *id) {
    if (!jac_body) {
        set_error("ssmq_integrand_define_dx: null argument");
        return SSMQ_E_ARG;
    }
    return define_impl("ssmq_integrand_define_dx", body, jac_body, din, dout, uses_time, id);
}

// Compiles `expr` for `arch` with the resource remarks on and writes the text of a compile check to `log`
static int compile_check_text(const std::string &expr, const char *arg_type, const std::vector<int> &ids, const char *arch, char *log,
                              int len) {
    std::lock_guard<std::mutex> lk(g_mu);
    Compiled *c = nullptr;
    std::string lg;
    const int rc = compile(expr, arg_type, ids, arch, &c, &lg, true);
    std::string text = lg;
    if (rc == SSMQ_OK) {   // the lowered name, then the resource remarks alone ("VGPRs: 67", "ScratchSize [bytes/lane]: 0", ...)
        text = c->lowered + "\n";
        size_t pos = 0;
        while (pos < lg.size()) {
            size_t e = lg.find('\n', pos);
            if (e == std::string::npos) e = lg.size();
            const std::string ln = lg.substr(pos, e - pos);
            const size_t r = ln.find("remark: ");
            if (r != std::string::npos) text += ln.substr(r + 8, ln.find(" [-Rpass") - r - 8) + "\n";
            pos = e + 1;
        }
    }
    if (log && len > 0) {
        const size_t n = std::min(text.size(), (size_t)len - 1);
        memcpy(log, text.data(), n);
        log[n] = '\0';
    }
    return rc;
}

extern "C" int ssmq_rtc_compile_check(int32_t id, int32_t id_obs, int kind, int D, int E, int N, int N_obs, int form, int tp, int opt,
                                      const char *arch, char *log, int len) {
    if (kind == SSMQ_RTC_LINEAR || kind == SSMQ_RTC_TAYLOR_GPQD) {   // k_<kernel>_fn<id, D, E, DIN>: N, N_obs, form, tp and opt are not read
        if (!arch || !*arch) {
            set_error("ssmq_rtc_compile_check: bad argument");
            return SSMQ_E_ARG;
        }
        const int jform = kind == SSMQ_RTC_LINEAR ? SSMQ_FORM_TAYLOR1 : SSMQ_FORM_TAYLOR_GPQD;
        ssmq_integrand f;
        memset(&f, 0, sizeof(f));
        f.id = id;
        std::string expr;
        std::vector<int> ids;
        int rc = jac_expr(jform, D, E, &f, &expr, &ids);
        if (rc) return rc;
        return compile_check_text(expr, jac_kernel(jform).arg_type, ids, arch, log, len);
    }
    if (kind == SSMQ_RTC_GPQD) {   // k_apply_gpqd[_lds]<id, D, E, DIN>: N, N_obs, form, tp and opt are not read
        if (!arch || !*arch) {
            set_error("ssmq_rtc_compile_check: bad argument");
            return SSMQ_E_ARG;
        }
        ssmq_integrand f;
        memset(&f, 0, sizeof(f));
        f.id = id;
        std::string expr;
        std::vector<int> ids;
        int rc = gpqd_expr(D, E, D > kGpqdRegMaxD, &f, &expr, &ids);
        if (rc) return rc;
        return compile_check_text(expr, "ssmq::GpqdArgs", ids, arch, log, len);
    }
    if (kind == SSMQ_RTC_PCRLB_DYN || kind == SSMQ_RTC_PCRLB_OBS) {   // k_pcrlb_dyn_fn<id, D, DIN> / k_pcrlb_obs_fn<id, D, E, DIN>
        if (!arch || !*arch) {
            set_error("ssmq_rtc_compile_check: bad argument");
            return SSMQ_E_ARG;
        }
        ssmq_integrand f;
        memset(&f, 0, sizeof(f));
        f.id = id;
        std::string expr;
        std::vector<int> ids;
        int rc = pcrlb_expr(kind == SSMQ_RTC_PCRLB_DYN, D, kind == SSMQ_RTC_PCRLB_DYN ? D : E, &f, &expr, &ids);   // (a transition: D outputs)
        if (rc) return rc;
        return compile_check_text(expr, "ssmq::PcrlbArgs", ids, arch, log, len);
    }
    if (kind == SSMQ_RTC_IMM) {   // k_imm_loop<D, E (= Y), N, N_obs, id, id_obs, opt (= SELO), form, tp>: built-in integrands
        FInfo fd, fo;
        if (!arch || !*arch || is_user_integrand(id) || is_user_integrand(id_obs) || !integrand_info(id, &fd) || !integrand_info(id_obs, &fo) || D < 1 ||
            D > 6 || E < 1 || E > 4 || N < 2 || N_obs < 2 || (form != SSMQ_FORM_BQ && form != SSMQ_FORM_SIGMA) || tp < 0 || tp > 1 ||
            (form == SSMQ_FORM_SIGMA && tp) || (opt != 0 && opt != 1)) {
            set_error("ssmq_rtc_compile_check: bad argument");
            return SSMQ_E_ARG;
        }
        char b[256];
        snprintf(b, sizeof(b), "ssmq::k_imm_loop<%d, %d, %d, %d, %d, %d, %d, %d, %d>", D, E, N, N_obs, id, id_obs, opt, form, tp);
        return compile_check_text(b, "ssmq::ImmArgs", {}, arch, log, len);
    }
    if (kind == SSMQ_RTC_MC) {   // k_mc_moments<id, D, E, 0>: N, N_obs, form, tp and opt are not read
        FInfo fm;
        if (!arch || !*arch || !integrand_info(id, &fm)) {
            set_error("ssmq_rtc_compile_check: bad argument");
            return SSMQ_E_ARG;
        }
        if (!mc_range_ok(D, E, 2) || fm.din > D) {
            set_error("ssmq_rtc_compile_check: the streaming Monte-Carlo kernel covers 1 <= D, E <= 6, integrand inputs <= D");
            return SSMQ_E_UNSUPPORTED;
        }
        N = N_obs = 2;
        form = SSMQ_FORM_SIGMA;
        tp = opt = 0;
    }
    const PassKernel *pk = pass_kernel(kind);   // the whole-pass kernels of the update variants and the smoother: dense alone
    if (!arch || !*arch || (kind != SSMQ_RTC_FILTER && kind != SSMQ_RTC_APPLY && kind != SSMQ_RTC_MC && kind != SSMQ_RTC_INNOVATION && !pk) ||
        (pk && opt != 0) || (form != SSMQ_FORM_BQ && form != SSMQ_FORM_SIGMA) ||
        tp < 0 || tp > 1 || (opt != 0 && opt != 1 && opt != 2 && opt != 3 && opt != 7)) {
        set_error("ssmq_rtc_compile_check: bad argument");
        return SSMQ_E_ARG;
    }
    const bool pair = kind == SSMQ_RTC_FILTER || kind == SSMQ_RTC_INNOVATION || pk;      // (id, id_obs): the two models of a filter
    std::string why;
    if (kind != SSMQ_RTC_MC && (!shape_ok(D, E, N, &why) || (pair && !shape_ok(D, D, N_obs, &why)))) {
        set_error(why);
        return SSMQ_E_UNSUPPORTED;
    }
    FInfo fi;
    if (!integrand_info(id, &fi) || (pair && !integrand_info(id_obs, &fi))) {
        set_error("ssmq_rtc_compile_check: unknown integrand id");
        return SSMQ_E_ARG;
    }
    std::vector<int> ids;
    if (is_user_integrand(id)) ids.push_back(id);
    if (pair && is_user_integrand(id_obs) && id_obs != id) ids.push_back(id_obs);
    const std::string expr = kind == SSMQ_RTC_FILTER       ? fused_expr(D, E, N, N_obs, id, id_obs, form, tp, 0, opt, -1)
                             : kind == SSMQ_RTC_INNOVATION ? innovation_expr(D, E, N, N_obs, id, id_obs, form, tp, 0, opt)
                             : pk                          ? pass_expr(*pk, D, E, N, N_obs, id, id_obs, form, tp, 0)
                             : kind == SSMQ_RTC_MC         ? "ssmq::k_mc_moments<" + std::to_string(id) + ", " + std::to_string(D) + ", " + std::to_string(E) + ", 0>"
                                                           : apply_expr(D, E, N, id, form, tp, 0, opt, false);
    return compile_check_text(expr, kind == SSMQ_RTC_FILTER ? "ssmq::FusedArgs" : kind == SSMQ_RTC_INNOVATION ? "ssmq::InnovArgs"
                                    : pk ? pk->args_type
                                    : kind == SSMQ_RTC_MC   ? "ssmq::McMomArgs" : "ssmq::ApplyArgs", ids, arch, log, len);
}

extern "C" int ssmq_rtc_stats(int64_t *compiles, int64_t *cache_hits, double *compile_seconds) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (compiles) *compiles = g_compiles;
    if (cache_hits) *cache_hits = g_hits;
    if (compile_seconds) *compile_seconds = g_compile_s;
    return SSMQ_OK;
}
