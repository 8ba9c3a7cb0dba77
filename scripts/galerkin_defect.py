#!/usr/bin/env python3
"""The Galerkin defect of a hierarchy from the CSR exports (include/mgx.h: mgx_operator_csr, mgx_transfer_csr):
per pair of levels  || R A_f P - A_c ||_F / || A_c ||_F  with the live P (--interp nearest by default), seamount geometry, four colours.
The reference does not build its coarse operators by the Galerkin product (it rediscretises on the coarsened geometry), so this is a
diagnostic of how far the two are apart, not an identity: a held pair of option "hold_z_levels" beside the halving pairs of the same size.
The products are torch sparse x dense on the device: P is made dense (rows of lev x rows of lev + 1), A_f and R stay CSR.
  python3 scripts/galerkin_defect.py --size 32 32 16 --out profiles/galerkin_defect.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def defects(mg, size, hold_z, interp):
    import torch
    from mgroms_amd import nhydro
    from mgroms_amd.testcases import seamount_geometry
    nx, ny, nz = size
    mg.nhydro_clean()
    nhydro.set_option("hold_z_levels", hold_z)
    mg.nhydro_init(nx, ny, nz, 1, 1, 0, nhydro.default_params(relax_method="FC", interp_type=interp))
    mg.nhydro_matrices(*seamount_geometry(nx, ny, 1, 1, 0), None, 4e3, 0.0, 0.0)
    out = []
    for lev in range(1, mg.nlevs()):
        F, C = mg.grid(lev), mg.grid(lev + 1)
        Af, Ac = nhydro.operator_csr(lev), nhydro.operator_csr(lev + 1)
        R, P = nhydro.restriction_csr(lev), nhydro.prolongation_csr(lev)
        D = torch.sparse.mm(R, torch.sparse.mm(Af, P.to_dense())) - Ac.to_dense()
        out.append({"pair": [lev, lev + 1], "fine": [F.nx, F.ny, F.nz], "coarse": [C.nx, C.ny, C.nz], "held": F.nz == C.nz,
                    "defect": float(torch.linalg.norm(D) / torch.linalg.norm(Ac.values()))})
    mg.nhydro_clean()
    nhydro.set_option("hold_z_levels", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[32, 32, 16])
    ap.add_argument("--interp", default="nearest")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import mgroms_amd as mg
    mg.nhydro.set_verbose(0)
    res = {"size": a.size, "interp_type": a.interp, "relax_method": "FC", "geometry": "seamount",
           "what": "|| R A_f P - A_c ||_F / || A_c ||_F per pair of levels",
           "hold_z_levels=0": defects(mg, a.size, 0, a.interp), "hold_z_levels=1": defects(mg, a.size, 1, a.interp)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
