"""The time loop's constants layout (csrc/ssmq_host.h: pass_consts_doubles, fill_pass_consts, wire_pass_consts) under
AddressSanitizer and UBSan on the CPU: tests/pass_consts_check.hip is a stand-alone program that calls no HIP API."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_consts_layout_under_sanitizers(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')      # (the default of csrc/Makefile)
    exe = str(tmp_path / 'pass_consts_check')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-w'] + [a for f in san for a in ('-Xarch_host', f)] + \
        [san[0], '-I', os.path.join(ROOT, 'ssmtoybox_amd', 'csrc'), '-I', os.path.join(ROOT, 'include'),
         os.path.join(ROOT, 'tests', 'pass_consts_check.hip'), '-o', exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    syms = subprocess.run(['nm', exe], stdout=subprocess.PIPE, text=True).stdout
    assert '__asan_init' in syms and '__ubsan_handle' in syms, 'the program was built without the sanitizers'
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0, ran.stdout
    # 3 model pairs x 4 shapes x 8 combinations of null / non-null GQG, R, scale
    assert ran.stdout.strip().splitlines()[-1] == 'ok 96', ran.stdout
