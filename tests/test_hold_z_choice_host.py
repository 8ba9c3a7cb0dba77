"""The launches option "hold_z_levels" adds, pinned on the host (no GPU) in the pattern of tests/test_kernel_choice_host.py:
tests/kernel_choice/record_held_main.cpp calls the wrappers of mgx_resrest_held.hip -- compiled host-only behind record_shim.h, which
records a launch instead of making it -- over shapes, flags and A/B switches either side of every condition of choose_resrest_held
(mgx_choice_transfer.h), plainly and with an error reported after every launch, and asks the smoother's pure choice functions (mgx_choice.h)
for the colour pass of the levels the option creates.  The lines are hashed and compared with tests/golden/hold_z_choice.json.

    python tests/test_hold_z_choice_host.py --dump DIR      the full lines (normal.txt, fail.txt)
    python tests/test_hold_z_choice_host.py --write-golden  regenerate the table (only ever from a commit whose choices are the wanted ones)
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgroms_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "kernel_choice")
GOLDEN = os.path.join(ROOT, "tests", "golden", "hold_z_choice.json")
PASSES = ["normal", "fail"]
KF_COLOUR = 10   # KernelFamily of mgx_choice.h: the generic column pass, one launch per colour and a halo launch behind it
KF_KS, KF_KS2, KF_NZ = 5, 6, 7


def build(outdir):
    hipcc = os.environ.get("HIPCC", "hipcc")
    common = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w", "-I" + CSRC, "-I" + HERE]
    unit = os.path.join(outdir, "mgx_resrest_held.o")
    main = os.path.join(outdir, "record_held_main.o")
    subprocess.run([hipcc, *common, "-include", "record_shim.h", "-c", "-x", "hip", os.path.join(CSRC, "mgx_resrest_held.hip"), "-o", unit], check=True)
    subprocess.run([hipcc, *common, "-c", "-x", "hip", os.path.join(HERE, "record_held_main.cpp"), "-o", main], check=True)
    undefined = subprocess.run(["nm", "-u", unit, main], check=True, capture_output=True, text=True).stdout
    fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", undefined)))
    exe = os.path.join(outdir, "record_held_main")
    clangxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    subprocess.run([clangxx, "-rdynamic", unit, main, *["-Wl,--defsym=%s=0" % f for f in fatbins], "-ldl", "-o", exe], check=True)
    return exe, unit


def record(exe):
    return {p: subprocess.run([exe] + ([] if p == "normal" else [p]), check=True, capture_output=True, text=True).stdout.splitlines() for p in PASSES}


def digest(passes):
    return {p: [len(passes[p]), hashlib.sha256(("\n".join(passes[p]) + "\n").encode()).hexdigest()] for p in PASSES}


def calls(lines):
    out = []
    for line in lines:
        if line.startswith("call "):
            out.append((line, []))
        elif out and line.startswith("  "):
            out[-1][1].append(line)
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe, unit = build(str(tmp_path_factory.mktemp("hold_z_choice")))
    return exe, unit, record(exe)


def test_table(run):
    """no choice, grid, block, argument or return value moved"""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert digest(run[2]) == want


def test_every_instance_launched(run):
    """all eight instances (matrix-free or stored, cmatrix, with the norm or without) are reached"""
    exe, unit, passes = run
    syms = subprocess.run(["nm", "--defined-only", unit], check=True, capture_output=True, text=True).stdout
    stubs = sorted(set(re.findall(r"\b(\w*__device_stub__\w+)", syms)))
    have = set(subprocess.run([exe, "names"], input="\n".join(stubs) + "\n", check=True, capture_output=True, text=True).stdout.splitlines())
    seen = {m.group(1) for line in passes["normal"] for m in [re.match(r"  launch (.*?) grid=", line)] if m}
    assert len(have) == 8 and seen == have, sorted(have ^ seen)


def test_served_exactly_where_the_rule_says(run):
    """a launch is made iff the coarse level has the fine level's nz and half its nx and ny, nz is even, and the switches allow it; the
    instance is matrix-free iff the level has its slopes and nz >= 3; the grid is ceil(ny_c / 16) x ceil(nx_c / 4) workgroups of 64 x 4
    lanes and equals what mgxk_residual_restrict_held_grid said (mgx_init sizes the norm's partials by it); under an error behind the
    launch the wrapper reports 0"""
    n = 0
    for head, body in calls(run[2]["normal"]):
        m = re.match(r"call mgxk_residual_restrict_held \| (\d+)x(\d+)x(\d+) zy=(\d) real=(\d) norm=(\d) coarse=(\d) sw=(\d)", head)
        nx, ny, nz, zy, real, norm, cv, sw = map(int, m.groups())
        served = cv == 0 and nz % 2 == 0 and sw != 1 and not (sw == 2 and nx * ny * nz < 32 * 32 * 16)
        launches = [l for l in body if l.startswith("  launch ")]
        assert len(launches) == (1 if served else 0), head
        assert body[-1] == "  -> %d" % served, head
        said = [int(l.split()[1]) for l in body if l.startswith("  held_grid ")]
        if served:
            g = re.match(r"  launch void k_residual_restrict_held<(\w+), (\w+), (\w+)>\(.*\) grid=(\d+),(\d+),1 block=64,4,1 lds=0 ", launches[0])
            assert g, launches[0]
            assert g.group(1) == ("true" if zy and nz >= 3 else "false") and g.group(2) == ("true" if real else "false") and g.group(3) == ("true" if norm else "false"), head
            gx, gy = int(g.group(4)), int(g.group(5))
            assert (gx, gy) == ((ny // 2 + 15) // 16, (nx // 2 + 3) // 4), head
            assert said == [gx * gy], head
            # the streaming hint: only matrix-free and beyond the cache
            assert launches[0].rstrip().endswith(" 1" if zy and nx * ny * nz * 72.0 > 256e6 else " 0"), launches[0]
            n += 1
    assert n > 300
    for head, body in calls(run[2]["fail"]):
        assert body[-1] == "  -> 0", head


def test_partials_fit_the_level_one_allocation(run):
    """mgx_init sizes the partial sums by max(workgroups of the level's residual, workgroups of the fused closing residual): the held
    kernel's count never exceeds the residual's own 2 * ceil(ny / 128) * ceil(nx / 4)"""
    for head, body in calls(run[2]["normal"]):
        m = re.match(r"call mgxk_residual_restrict_held \| (\d+)x(\d+)x(\d+) .* coarse=0 ", head)
        if m:
            nx, ny, _ = map(int, m.groups())
            said = [int(l.split()[1]) for l in body if l.startswith("  held_grid ")][0]
            assert said <= 2 * ((ny // 2 + 63) // 64) * ((nx + 3) // 4), head


def test_held_levels_keep_the_instance_of_their_shape(run):
    """the levels the option creates -- a large even nz on half or a quarter of level 1's plane -- get the register-resident, k-split or
    colour-pair instance of their shape, never the generic column pass"""
    lines = [l for l in run[2]["normal"] if l.startswith("smoother ")]
    assert len(lines) == 9 * 2 * 2
    for l in lines:
        m = re.match(r"smoother (\d+)x(\d+)x(\d+) zy=(\d) rb=(\d) \| ks family=(\d+) .* \| pair family=(\d+) \| colour family=(\d+) nz=(\d+) .* \| reg=(\d)", l)
        nx, ny, nz, zy, rb, ks, pair, colour, cnz, reg = map(int, m.groups())
        assert colour == KF_NZ and cnz == nz and reg == 1, l
        assert colour != KF_COLOUR
        if zy and nz in (16, 32) and (ny // 2 + 63) // 64 * (nx if rb else nx // 2) <= 512:
            assert ks == KF_KS, l
        if zy and nz == 64 and not rb and (ny // 2 + 63) // 64 * (nx // 2) <= 512:
            assert ks == KF_KS, l
        if zy and nz == 16 and ny // 2 <= 64:
            assert pair == KF_KS2, l


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe, unit = build(tmp)
        passes = record(exe)
        print({p: len(passes[p]) for p in PASSES})
        if "--dump" in sys.argv:
            d = sys.argv[sys.argv.index("--dump") + 1]
            os.makedirs(d, exist_ok=True)
            for p in PASSES:
                with open(os.path.join(d, p + ".txt"), "w") as f:
                    f.write("\n".join(passes[p]) + "\n")
        if "--write-golden" in sys.argv:
            with open(GOLDEN, "w") as f:
                json.dump(digest(passes), f, indent=0, sort_keys=True)
                f.write("\n")
