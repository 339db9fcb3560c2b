"""The register engine's LDS block per class: sizeof(RLds<K>) as a host compiler lays it out, pinned to
the table in profiles/r10_resource_usage_reg.txt (the sizes decide how many waves a CU's LDS admits:
K = 9 runs four waves per SIMD only at <= 10240 bytes)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, 'fluidframework_amd', 'csrc')
TABLE = os.path.join(REPO, 'profiles', 'r10_resource_usage_reg.txt')

PROGRAM = os.path.join(CSRC, 'mt_reg_lds_sizes.cpp')  # prints "K sizeof(RLds<K>)" for K = 2 .. 16


def committed():
    """{K: (bytes, waves per CU)} of the table's `lds K=` rows"""
    rows = {}
    for line in open(TABLE):
        m = re.match(r'\s*lds K=(\d+)\s+(\d+)\s+(\d+)\s*$', line)
        if m:
            rows[int(m.group(1))] = (int(m.group(2)), int(m.group(3)))
    return rows


def test_rlds_sizes_match_the_committed_table(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = tmp_path / 'rlds_sizes'
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-o', str(exe), PROGRAM], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {int(k): int(v) for k, v in (x.split() for x in out.strip().split('\n'))}
    want = committed()
    assert sorted(got) == list(range(2, 17)) == sorted(want)
    assert got == {k: v[0] for k, v in want.items()}
    # what the occupancy picks lean on (the table's waves per CU, as tools/resource_usage.py derives them from the
    # sizes): K = 9 at four waves per SIMD, K = 11 / 12 at three
    assert want[9][1] >= 16 and want[11][1] >= 12 and want[12][1] >= 12
