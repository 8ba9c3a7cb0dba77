"""Which kernel serves which level, pinned on the host (no GPU): tests/kernel_choice/record_main.cpp calls the kernel wrappers of the smoother
units (mgx_relax.hip, mgx_relax_coarse.hip, mgx_relax_ks.hip, mgx_relax_tall.hip), of the sequential-order red-black walk (mgx_rbseq.hip), of
the fused residual + restriction (mgx_resrest.hip), and of the operator, the transfers, the halo and gather transport, the layout conversions,
the Krylov passes and the model coupling (mgx_residual.hip, mgx_transfer.hip, mgx_hold.hip, mgx_halo.hip, mgx_layout.hip, mgx_krylov.hip,
mgx_model.hip) -- compiled host-only behind record_shim.h, which records a launch instead of making it --
over shapes, flags and A/B switches either side of every threshold, three times: plainly, with every hipFuncSetAttribute refused, and with
an error reported after every launch.  Per group (wrapper x nz x method; one per wrapper for the units that only choose a launch) the lines of the three passes are hashed and compared with
tests/golden/kernel_choice.json; every kernel instance the objects hold must have been launched at least once, but for the ones named below
with the reason; and the two functions that predict another wrapper's choice (mgxk_residual_restrict_grid, mgxk_rbseq_wants_d0) agree with it.

    python tests/test_kernel_choice_host.py --dump DIR      the full lines (normal.txt, refuse.txt, fail.txt), to diff against another checkout's
    python tests/test_kernel_choice_host.py --write-golden  regenerate the table (only ever from a commit whose choices are the wanted ones)
    python tests/test_kernel_choice_host.py --sanitize address,undefined    build the program with sanitizers and run its three passes
"""
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgroms_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "kernel_choice")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_choice.json")
UNITS = ["mgx_relax", "mgx_relax_coarse", "mgx_relax_ks", "mgx_relax_tall", "mgx_rbseq", "mgx_resrest",
         "mgx_residual", "mgx_transfer", "mgx_halo", "mgx_layout", "mgx_hold", "mgx_krylov", "mgx_model"]
PASSES = ["normal", "refuse", "fail"]

# Kernel instances of the units that no call of the recorder can launch, one by one with the reason.  (The instances of k_relax_ksp
# belong to mgxk_relax_ks_persist, whose workgroups wait for each other: its wrapper is not enumerated.)
SIG = "(LevView, int, int, int, int, int, Sides, int)"
UNREACHABLE = {
    # launch_relax_nz_d picks MF at run time (slopes and NZ >= 16), so the compiler also emits the matrix-free instances of the NZ below 16
    "void k_relax_nz<%d, %s, %d, true, %s>%s" % (nz, rs, 1 if nz < 8 else 2, st, SIG): "matrix-free cross terms are chosen from nz = 16 on"
    for nz in (2, 4, 8, 12) for rs in ("false, false", "true, false", "true, true") for st in ("false", "true")
}
# rbseq_scan_launch (mgx_rbseq.hip) names an instance per (row of its ladder, ring depth, colour, full half-rows or not); the ladder itself
# keeps some of them from ever being asked for
SCAN = "void k_rbseq_scan<%d, %d, %d, %s, %d, false, 0>(LevView, int, int, RbFuse)"
UNREACHABLE.update({SCAN % (16, d, rbp, "true", 1): "a full half-row of 1024 columns is served by the eight-wave instance" for d in (2, 4) for rbp in (0, 1)})
UNREACHABLE.update({SCAN % (16, 4, rbp, "false", 1): "the ring depth 2 divides every even nx: depth 4 is never asked of this row" for rbp in (0, 1)})
UNREACHABLE.update({SCAN % (8, d, rbp, "true", 1): "a full half-row of 512 columns is served by the four-wave instance" for d in (2, 4) for rbp in (0, 1)})
UNREACHABLE.update({SCAN % (2, d, rbp, "false", nw): "the several-wave instances serve full half-rows of 512 and 1024 columns only"
                    for d in (16, 4, 2) for rbp in (0, 1) for nw in (4, 8)})


def build(outdir, sanitize=None):
    """the recorder program: the units host-only behind the shim, linked with record_main.cpp and nothing of the HIP runtime;
    sanitize: e.g. "address,undefined" (the program is stand-alone: it runs without a preload)"""
    hipcc = os.environ.get("HIPCC", "hipcc")
    common = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w", "-I" + CSRC, "-I" + HERE,
              *(["-Xarch_host", "-fsanitize=" + sanitize, "-g"] if sanitize else [])]

    def unit(u):
        obj = os.path.join(outdir, u + ".o")
        subprocess.run([hipcc, *common, "-include", "record_shim.h", "-c", "-x", "hip", os.path.join(CSRC, u + ".hip"), "-o", obj], check=True)
        return obj

    def main():
        obj = os.path.join(outdir, "record_main.o")
        subprocess.run([hipcc, *common, "-c", "-x", "hip", os.path.join(HERE, "record_main.cpp"), "-o", obj], check=True)
        return obj

    with ThreadPoolExecutor(len(UNITS) + 1) as pool:
        jobs = [pool.submit(unit, u) for u in UNITS] + [pool.submit(main)]
        objs = [j.result() for j in jobs]
    # the one fat-binary symbol each object refers to: defined as an absolute zero, never read
    undefined = subprocess.run(["nm", "-u", *objs], check=True, capture_output=True, text=True).stdout
    fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", undefined)))
    exe = os.path.join(outdir, "record_main")
    clangxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    subprocess.run([clangxx, "-rdynamic", *(["-fsanitize=" + sanitize] if sanitize else []), *objs, *["-Wl,--defsym=%s=0" % f for f in fatbins], "-ldl", "-o", exe], check=True)
    return exe, objs[:len(UNITS)]


def record(exe):
    """{pass: lines}"""
    out = {}
    for p in PASSES:
        r = subprocess.run([exe] + ([] if p == "normal" else [p]), check=True, capture_output=True, text=True)
        out[p] = r.stdout.splitlines()
    return out


def groups(passes):
    """{'wrapper nz=N method=M': [lines, sha256]} over the three passes in order"""
    acc = {}
    for p in PASSES:
        key = None
        for line in passes[p]:
            if line.startswith("call "):
                key = line.split(" | ")[0][5:]
                if key not in acc:
                    acc[key] = [0, hashlib.sha256()]
            g = acc[key]
            g[0] += 1
            g[1].update((p + " " + line + "\n").encode())
    return {k: [n, h.hexdigest()] for k, (n, h) in acc.items()}


def launched(passes):
    return {m.group(1) for p in PASSES for line in passes[p] for m in [re.match(r"  launch (.*?) grid=", line)] if m}


def instances(exe, objs):
    """the kernel instances the objects define, in the recorder's own spelling"""
    syms = subprocess.run(["nm", "--defined-only", *objs], check=True, capture_output=True, text=True).stdout
    stubs = sorted({s for s in re.findall(r"\b(\w*__device_stub__\w+)", syms)})
    r = subprocess.run([exe, "names"], input="\n".join(stubs) + "\n", check=True, capture_output=True, text=True)
    return set(r.stdout.splitlines())


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe, objs = build(str(tmp_path_factory.mktemp("kernel_choice")))
    return exe, objs, record(exe)


def test_table(run):
    """every group's digest and line count is the committed one: no choice, grid, block, LDS size, argument or return value moved"""
    got = groups(run[2])
    with open(GOLDEN) as f:
        want = json.load(f)
    assert {p: len(run[2][p]) for p in PASSES} == want["lines"]
    assert sorted(got) == sorted(want["groups"])
    moved = [k for k in sorted(got) if got[k] != want["groups"][k]]
    assert not moved, "groups that differ from tests/golden/kernel_choice.json (compare two --dump directories): %s" % moved


def test_every_instance_launched(run):
    """a kernel instance that no call reaches is pinned by nothing: each is launched at least once, or named in UNREACHABLE with the reason"""
    exe, objs, passes = run
    have = instances(exe, objs)
    assert len(have) > 100
    seen = launched(passes)
    assert seen <= have
    missing = {k for k in have - seen if not k.startswith("void k_relax_ksp<")}
    assert missing == set(UNREACHABLE), sorted(missing ^ set(UNREACHABLE))


def calls(lines):
    """[(head, [the call's other lines])]"""
    out = []
    for line in lines:
        if line.startswith("call "):
            out.append((line, []))
        else:
            out[-1][1].append(line)
    return out


def test_restrict_grid_is_the_launch(run):
    """the norm's partials are sized by mgxk_residual_restrict_grid: it is the workgroup count of the launch mgxk_residual_restrict_ex makes"""
    n = 0
    for head, body in calls(run[2]["normal"]):
        said = [int(l.split()[1]) for l in body if l.startswith("  restrict_grid ")]
        for l in body:
            m = re.match(r"  launch .* grid=(\d+),(\d+),(\d+) ", l)
            if m and said:
                assert said == [int(m.group(1)) * int(m.group(2)) * int(m.group(3))], head
                n += 1
    assert n > 1000


def test_a_walk_that_reads_d0_has_asked_for_it(run):
    """where the walk reads d0 from u1 -- k_rbseq_scan with D0IN false, or k_rbseq_walk_apply -- mgxk_rbseq_wants_d0 told the colour pass to write it"""
    n = 0
    for head, body in calls(run[2]["normal"]):
        said = [l for l in body if l.startswith("  wants_d0 ")]
        reads = [l for l in body if re.match(r"  launch void k_rbseq_scan<\d+, \d+, \d+, \w+, \d+, false, ", l) or l.startswith("  launch void k_rbseq_walk_apply<")]
        if said and reads:
            assert said == ["  wants_d0 1"], head
            n += 1
    assert n > 1000


def test_fall_back_passes_launch_and_report_nothing_served(run):
    """with an error behind every launch, a wrapper that reports what ran reports 0: the caller falls back"""
    lines = run[2]["fail"]
    after_launch = [lines[i + 1] for i, l in enumerate(lines[:-1]) if l.startswith("  launch ") and lines[i + 1].startswith("  -> ")]
    heads = {}
    key = None
    for l in lines:
        if l.startswith("call "):
            key = l.split()[1]
        elif l.startswith("  -> ") and key in ("mgxk_relax_small", "mgxk_relax_wave", "mgxk_relax_wave_fused", "mgxk_relax_ks", "mgxk_relax_ks_pair", "mgxk_relax_tall",
                                                "mgxk_rbseq_walk_apply", "mgxk_rbseq_window", "mgxk_residual_restrict_ex", "mgxk_residual_restrict"):
            heads.setdefault(key, set()).add(l)
    assert after_launch
    assert all(v == {"  -> 0"} for v in heads.values()), heads


def test_p2p_plan(run):
    """the block plan of the one-launch halo exchange (choose_halo_p2p) over the recorder's shapes and a sweep of nz in {1 .. 128}, nx, ny in
    {2 .. 4096}, all 3^4 edge patterns (absent, peer, self) and MGX_P2P_MAXBLK = 1, 8, 128: nreal <= maxblk + 7, blk0 does not decrease over the
    present directions, absent directions sit past the end, and nreal <= 128 at maxblk = 128 while nx, ny <= 1024, nz <= 128"""
    r = subprocess.run([run[0], "p2p"], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and not [l for l in r.stdout.splitlines() if l.startswith("violation ")], r.stdout[-2000:]
    m = re.search(r"p2p_plan checked=(\d+) violations=0 max_nreal maxblk1=(\d+) maxblk8=(\d+) maxblk128=(\d+) maxblk128_to_1024x1024x128=(\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    checked, m1, m8, m128, small = map(int, m.groups())
    assert checked >= 3 * 81 * 10 * 9 * 9
    assert m1 <= 8 and m8 <= 15 and m128 <= 135 and small <= 128
    assert m128 > 128   # the sweep does hold the sizes at which the plan exceeds maxblk: the bound is maxblk + 7, not maxblk


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs = build(tmp, sys.argv[sys.argv.index("--sanitize") + 1] if "--sanitize" in sys.argv else None)
        passes = record(exe)
        print(subprocess.run([exe, "p2p"], check=True, capture_output=True, text=True).stdout, end="")
        if "--dump" in sys.argv:
            d = sys.argv[sys.argv.index("--dump") + 1]
            os.makedirs(d, exist_ok=True)
            for p in PASSES:
                with open(os.path.join(d, p + ".txt"), "w") as f:
                    f.write("\n".join(passes[p]) + "\n")
            print({p: len(passes[p]) for p in PASSES})
        if "--write-golden" in sys.argv:
            with open(GOLDEN, "w") as f:
                json.dump({"lines": {p: len(passes[p]) for p in PASSES}, "groups": groups(passes)}, f, indent=0, sort_keys=True)
                f.write("\n")
        missing = instances(exe, objs) - launched(passes)
        print("not launched:", *sorted(missing), sep="\n  ")
