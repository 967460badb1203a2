"""The C side of the row rule (waveforms_amd/csrc/wfk_row_rule.h; DESIGN.md, "The row rule") without a device: the
stand-alone host program tests/c_abi/row_rule_host.cpp -- its own main, no HIP, addresses as plain integers -- built
with g++ as tools/plan_image.sh builds its program, once plain and once under ASan + UBSan, and run directly.  The
program holds the extent arithmetic of test_rows_cpu.py::test_disjointness with sides that differ in element size, row
length and row count, every clause of every stage's line of the acceptance table, rows more than 2^32 elements apart
and the int64 report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {'plain': ['-O3'],   # (the runtimes linked statically: the program runs whatever else the process loads first)
          'sanitized': ['-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan']}


@pytest.mark.parametrize('build', list(BUILDS))
def test_the_rule_holds_its_table(build, tmp_path):
    exe = tmp_path / f'row_rule_{build}'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', *BUILDS[build],
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'waveforms_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c_abi', 'row_rule_host.cpp'), '-o', str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == 'row rule ok' and not r.stderr, (r.stdout, r.stderr)


def test_the_header_is_apart_from_hip():
    with open(os.path.join(ROOT, 'waveforms_amd', 'csrc', 'wfk_row_rule.h')) as f:
        includes = [line.split()[1] for line in f if line.startswith('#include')]
    assert includes == ['<cstddef>', '<cstdint>', '<initializer_list>', '<string>', '"wfk.h"']
