"""The pair-packed per-lane tables of the row-lane kernels (gr-gfdm_amd/csrc/gfdm_packed_tables.h), on the host: no GPU.

tests/packed_tables_host.cc is compiled with g++ under AddressSanitizer + UBSan into a stand-alone program and run.  It packs the twiddle and
root tables as the plan builder does and reads them back the way the kernels address them: every value must have the bits of the plain
table's, the roots must be the ones the plain code reads (in its order), every plane must start on a 16-byte boundary.
Shapes (K, M): odd and even M - 1, K below 64 (several blocks per wavefront), the wide plans, a mixed-radix K -- and beyond the compiled list
every other plan of the family once (radix-4 passes with and without the trailing radix-2 pass, three-pass plans, a single-pass K)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gr-gfdm_amd", "csrc")

SHAPES = [(64, 9), (128, 15), (256, 31), (4, 16), (4, 8), (32, 5), (96, 25)]
# (the plans the list above does not reach; counts from the pass plans in gfdm_rowgeom.h)
MORE = [(8, 5), (16, 6), (32, 9), (512, 4), (1024, 3), (12, 7), (48, 3), (200, 5), (51, 9), (64, 2), (64, 3)]
# K: roots a lane reads before its first transform
ROOTS = {64: 3, 128: 7, 256: 15, 4: 0, 32: 6, 96: 5, 8: 3, 16: 3, 512: 14, 1024: 14, 12: 0, 48: 2, 200: 1 + 9, 51: 2}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("packed") / "packed_tables_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "packed_tables_host.cc"), "-o", exe])
    return exe


def _run(exe, shapes):
    args = [str(v) for s in shapes for v in s]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()[:-1]
    assert len(lines) == len(shapes)
    return lines


def test_packed_tables_unpack_to_the_plain_tables_bit_for_bit(program):
    lines = _run(program, SHAPES + MORE)
    for (K, M), line in zip(SHAPES + MORE, lines):
        n = M - 1
        assert line == "K=%d M=%d: %d twiddles (%d 16-byte + %d 8-byte loads), %d roots (%d + %d)" % (K, M, n, n // 2, n % 2, ROOTS[K], ROOTS[K] // 2, ROOTS[K] % 2)


def test_load_counts_of_the_benchmark_shapes(program):
    """the figures the stage is there for: table loads per wave 8 + 3 -> 4 + 2 at K=64 M=9, 14 + 7 -> 7 + 4 at K=128 M=15, 30 + 15 -> 15 + 8 at K=256 M=31"""
    got = {}
    for (K, M), line in zip(SHAPES[:3], _run(program, SHAPES[:3])):
        w = line.replace("(", " ").replace(")", " ").replace(",", " ").split()
        got[K] = (int(w[2]), int(w[4]) + int(w[7]), int(w[10]), int(w[12]) + int(w[14]))
    assert got == {64: (8, 4, 3, 2), 128: (14, 7, 7, 4), 256: (30, 15, 15, 8)}
