"""The geometry of the CSR export (mgroms_amd/csrc/mgx_export.h) on the host, no GPU: tests/export_host/export_main.cpp, a stand-alone
program over the header's pure functions in the pattern of tests/kernel_choice/, walks

  - the colouring: for closed, singly periodic and doubly periodic levels of 2, 4, 6, 8, 10, 12 and 20 cells per horizontal axis (nz = 2, 3,
    4, 5, 8), for A, R and P, halving and held pairs, no two cells that share a row have the same colour, and the column recovered for
    every (row, colour) is the cell that was coloured.  What a row can see is spelled out in the program, not taken from the header;
  - the colours along one axis, which this file checks against the rule itself (any three consecutive cells differ, cyclically where the
    axis wraps);
  - the launch choice and the int limits, against the table below.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgroms_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "export_host")
OPEN, MIRROR, WRAP = 0, 1, 2
A, R, P = 0, 1, 2
SIZES = (4, 6, 8, 10, 12, 20)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("export_host")), "export_main")
    clangxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    subprocess.run([clangxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, os.path.join(HERE, "export_main.cpp"), "-o", out], check=True)
    return out


def lines(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    return r.returncode, r.stdout.splitlines()


def test_no_two_cells_of_a_row_share_a_colour_and_every_column_is_recovered(exe):
    with ThreadPoolExecutor(4) as pool:
        runs = list(pool.map(lambda q: lines(exe, "colouring", str(q)), range(4)))
    seen = set()
    for rc, out in runs:
        bad = [l for l in out if not l.startswith("ok ")]
        assert rc == 0 and not bad, bad[:20]
        for l in out:
            f = dict(kv.split("=") for kv in l.split()[1:])
            nx, ny, nz = map(int, f["columns"].split("x"))
            assert int(f["colours"]) <= 64 and int(f["rows"]) > 0 and int(f["visible"]) >= int(f["rows"])
            seen.add((int(f["mode"]), int(f["held"]), nx, ny, int(f["rule_j"]), int(f["rule_i"])))
    # every case the export is asked for was walked: closed, singly and doubly periodic, every size per axis, A, R, P, halving and held
    for rj, ri in ((MIRROR, MIRROR), (WRAP, MIRROR), (MIRROR, WRAP), (WRAP, WRAP)):
        for nx in SIZES:
            for ny in SIZES:
                for mode, held in ((A, 0), (R, 0), (R, 1), (P, 0), (P, 1)):
                    assert (mode, held, nx, ny, rj, ri) in seen, (mode, held, nx, ny, rj, ri)


def test_any_three_consecutive_cells_of_an_axis_differ(exe):
    rc, out = lines(exe, "axis")
    assert rc == 0 and len(out) == 3 * 40
    for l in out:
        head, cols = l.split(" : ")
        _, rule, n, ncol = head.split()
        rule, n, ncol = int(rule), int(n), int(ncol)
        c = [int(v) for v in cols.split()]
        assert len(c) == n and set(c) == set(range(ncol)), l
        if rule == WRAP:
            # cyclically; an axis shorter than three cells only has to tell its cells apart
            for x in range(n):
                trio = {(x + d) % n for d in (-1, 0, 1)}
                assert len({c[y] for y in trio}) == len(trio), l
            # a period of 3 where it divides the size, a mixed 3 / 4 pattern otherwise: never more than four colours from six cells on
            assert ncol == (n if n < 6 else (3 if n % 3 == 0 else 4)), l
        else:
            assert ncol == min(n, 3), l
            assert all(len(set(c[x:x + 3])) == len(c[x:x + 3]) for x in range(max(n - 2, 1))), l


def test_launch_choice_and_int_limits(exe):
    rc, out = lines(exe, "choice")
    assert rc == 0
    got = {int(l.split()[1]): tuple(int(v) for v in l.split()[2:]) for l in out if l.startswith("choice ")}
    # rows: one lane per row, 256 per workgroup; scan: n + 1 entries (the last is rowptr[n] = nnz), 2048 per workgroup
    want = {1: (256, 1, 1), 2: (256, 1, 1), 255: (256, 1, 1), 256: (256, 1, 1), 257: (256, 2, 1), 2046: (256, 8, 1), 2047: (256, 8, 1),
            2048: (256, 8, 2), 2049: (256, 9, 2), 4095: (256, 16, 2), 4096: (256, 16, 3), 524287: (256, 2048, 256), 524288: (256, 2048, 257),
            16 * 16 * 8: (256, 8, 2), 512 * 512 * 64: (256, 65536, 8193), 2147483646: (256, 8388608, 1048576)}
    assert got == want
    fits = [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith("fits ")]
    assert fits == [(1, 1, 0, 0), (2147483646, 8, 19, 0), (2147483647, 8, 19, 1), (8, 2147483647, 19, 1), (1 << 20, 1 << 20, 2147483647, 0),
                    (1 << 20, 1 << 20, 2147483648, 2), (1 << 27, 1 << 27, 19 << 27, 2)]
