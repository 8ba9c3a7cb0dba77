#!/usr/bin/env python3
"""One record per kernel of device assembly files (`make -C mgroms_amd/csrc -j8 isa` writes build/*.s): resources and a hash of
the instruction text.  Two trees whose records are equal compile to the same kernels -- the check a refactor of the hand-written
kernels has to pass.

  python scripts/kernel_isa.py mgroms_amd/csrc/build/mgx_relax.s ... > branch.json
  python scripts/kernel_isa.py --diff parent.json branch.json        # prints the kernels that differ, exit status 1 if any
  python scripts/kernel_isa.py --merge parent.json branch.json [more.json]   # both tables side by side with what differs, as
                                                                             # committed under profiles/; more.json: further top-level keys
"""
import hashlib, json, re, sys

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def records(path):
    lines = open(path).read().split("\n")
    meta, cur = {}, {}  # the amdhsa.kernels metadata: one "  - " block per kernel, .name among its keys
    for ln in lines[next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels")):]:
        if ln.startswith("  - "):
            cur = {}
        m = re.match(r"(?:    |  - )(\.\w+):\s+(\S+)$", ln)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    out = {}
    for name, md in meta.items():
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        text = []
        for ln in lines[a + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith(".") and not ln.endswith(":"):  # no directives, labels, comments
                # block and long-branch labels carry the function's position in the unit: the order of emission, not an instruction
                text.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", " ".join(ln.split()))))
        out[name] = {f[1:]: int(md[f]) for f in FIELDS}
        out[name].update(instructions=len(text), hash=hashlib.sha256("\n".join(text).encode()).hexdigest()[:16])
    return out


def main(argv):
    if argv and argv[0] == "--diff":
        a, b = (json.load(open(p)) for p in argv[1:3])
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        for k in bad:
            print(k, a.get(k), b.get(k), sep="\n  ")
        print(f"{len(a)} / {len(b)} kernels, {len(bad)} differ")
        return 1 if bad else 0
    if argv and argv[0] == "--merge":
        a, b = (json.load(open(p)) for p in argv[1:3])
        res = [f[1:] for f in FIELDS]
        out = {"same_kernel_symbols": set(a) == set(b),
               "kernels_with_different_resources": sorted(k for k in set(a) & set(b) if any(a[k][f] != b[k][f] for f in res)),
               "kernels_with_different_hash": sorted(k for k in set(a) & set(b) if a[k]["hash"] != b[k]["hash"])}
        for p in argv[3:]:
            out.update(json.load(open(p)))
        out["kernels"] = {k: {"parent": a.get(k), "branch": b.get(k)} for k in sorted(set(a) | set(b))}
        json.dump(out, sys.stdout, indent=1)
        return 0
    out = {}
    for p in argv:
        out.update(records(p))
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
