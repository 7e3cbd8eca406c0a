"""
The pendulum as device code against the built-in pendulum, on the CPU (no device needed): compiles the whole-pass filter kernel
three ways - ahead of time (hipcc, the Makefile flags), and with hiprtc from the embedded header source for the built-in ids and
for the same formulas as user bodies - and compares the instruction streams (llvm-objdump) and the resource remarks.
Needs a built tree (csrc/ssmq_rtc_src.inc).  Output: profiles/r07_user_models_isa.txt.
  python tools/rtc_isa_compare.py
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ssmtoybox_amd', 'csrc')
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
PRELUDE = ('typedef __hip_internal::int32_t int32_t;\ntypedef __hip_internal::uint32_t uint32_t;\n'
           'typedef __hip_internal::int64_t int64_t;\ntypedef __hip_internal::uint64_t uint64_t;\n#define NAN __builtin_nan("")\n')
USER = '''namespace ssmq {
template <> struct Fn<1024> {
    static constexpr int DIN = 2;
    double t_; const FPar *fp_;
    __device__ __forceinline__ void init(double t, const FPar &par) { t_ = t; fp_ = &par; }
    template <int E> __device__ __forceinline__ void eval(const double *x, double *o) const {
        const double t = t_; const double *p = fp_->p; (void)t; (void)p; (void)x; (void)o;
        { o[0] = x[0] + x[1] * p[0];  o[1] = x[1] - 9.81 * p[0] * sin_nr(x[0]); }
    }
};
template <> struct Fn<1025> {
    static constexpr int DIN = 1;
    double t_; const FPar *fp_;
    __device__ __forceinline__ void init(double t, const FPar &par) { t_ = t; fp_ = &par; }
    template <int E> __device__ __forceinline__ void eval(const double *x, double *o) const {
        const double t = t_; const double *p = fp_->p; (void)t; (void)p; (void)x; (void)o;
        { o[0] = sin_nr(x[0]); }
    }
};
}
'''


def rtc(expr, extra, out):
    lib = ctypes.CDLL(os.path.join(ROCM, 'lib', 'libhiprtc.so'))
    inc = open(os.path.join(CSRC, 'ssmq_rtc_src.inc')).read()
    body = inc[inc.index('(') + 1:inc.rindex(')')]                  # the raw string literal's content
    src = PRELUDE + body + extra + 'template __global__ void {}(const ssmq::FusedArgs);\n'.format(expr)
    prog = ctypes.c_void_p()
    assert lib.hiprtcCreateProgram(ctypes.byref(prog), src.encode(), b'u.hip', 0, None, None) == 0
    lib.hiprtcAddNameExpression(prog, expr.encode())
    opts = (ctypes.c_char_p * 4)(b'--offload-arch=gfx950', b'-O3', b'-std=c++17', b'-Rpass-analysis=kernel-resource-usage')
    rc = lib.hiprtcCompileProgram(prog, 4, opts)
    n = ctypes.c_size_t()
    lib.hiprtcGetProgramLogSize(prog, ctypes.byref(n))
    log = ctypes.create_string_buffer(n.value + 1)
    lib.hiprtcGetProgramLog(prog, log)
    assert rc == 0, log.value.decode()
    lib.hiprtcGetCodeSize(prog, ctypes.byref(n))
    code = ctypes.create_string_buffer(n.value)
    lib.hiprtcGetCode(prog, code)
    low = ctypes.c_char_p()
    lib.hiprtcGetLoweredName(prog, expr.encode(), ctypes.byref(low))
    open(out, 'wb').write(code.raw)
    return low.value.decode(), log.value.decode()


def disasm(co, sym):
    txt = subprocess.run([os.path.join(ROCM, 'llvm', 'bin', 'llvm-objdump'), '-d', '--no-show-raw-insn', '--disassemble-symbols=' + sym, co],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
    return [re.sub(r'\s*//.*', '', l).strip() for l in txt.splitlines() if re.match(r'^\s+[a-z_]', l)]


def remarks(log, sym):
    blk = log.split('Function Name: ' + sym)[1].split('Function Name: ')[0]
    return dict(re.findall(r'remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)', blk))


def main():
    tmp = tempfile.mkdtemp()
    aot = os.path.join(tmp, 'aot.co')
    r = subprocess.run([os.path.join(ROCM, 'bin', 'hipcc'), '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '--cuda-device-only',
                        '--no-gpu-bundle-output', '-c', os.path.join(CSRC, 'ssmq_filter_fused.hip'), '-o', aot,
                        '-Rpass-analysis=kernel-resource-usage'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    lines = []
    for form, tag in ((1, 'UKF (SIGMA)'), (0, 'GPQKF (BQ)')):
        e_bi = 'ssmq::k_filter_fused<2, 1, 5, 5, 5, 6, {}, 0, 0, 0, -1>'.format(form)
        e_us = 'ssmq::k_filter_fused<2, 1, 5, 5, 1024, 1025, {}, 0, 0, 0, -1>'.format(form)
        s_bi, l_bi = rtc(e_bi, '', os.path.join(tmp, 'bi.co'))
        s_us, l_us = rtc(e_us, USER, os.path.join(tmp, 'us.co'))
        a, b, c = disasm(aot, s_bi), disasm(os.path.join(tmp, 'bi.co'), s_bi), disasm(os.path.join(tmp, 'us.co'), s_us)
        lines.append('pendulum {}: instructions AOT {} | hiprtc built-in ids {} | hiprtc user bodies {}; identical: {} / {}'.format(
            tag, len(a), len(b), len(c), a == b, b == c))
        lines.append('  AOT       {}'.format(remarks(r.stdout, s_bi)))
        lines.append('  hiprtc bi {}'.format(remarks(l_bi, s_bi)))
        lines.append('  hiprtc us {}'.format(remarks(l_us, s_us)))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    open(os.path.join(ROOT, 'profiles', 'r07_user_models_isa.txt'), 'w').write(
        '# tools/rtc_isa_compare.py: the pendulum filter kernel ahead of time, through hiprtc with the built-in ids, and with the\n'
        '# same formulas as user bodies (D = 2, Y = 1, N = 5, gfx950)\n' + text)


if __name__ == '__main__':
    main()
