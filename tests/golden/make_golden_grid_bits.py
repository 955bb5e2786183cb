"""The bits of the interpol grid kernels (spline_grid.hip, grid_hess.hip, label_pull.hip, the axis tables of restrict.hip)
as the built library gives them, so that a refactor of what these files share can be held to torch.equal.  The other
fixtures of the family compare with the reference at 2e-5 and would not see a changed last bit.

Run on an MI355X with the library built: python tests/golden/make_golden_grid_bits.py -> grid_family_bits.npz.
Regenerate it only from a commit whose kernels are known good; the cases are in tests/grid_bits_cases.py.

  in/*                 the inputs of the small cases (one CPU seed)
  cases                names of the deterministic cases; pull / grad / hess / hessc and label/<dtype> (the four variants
                       AUTO, LDS, REGS, PASSES) hold one entry per case
  table/*              rowptr / col / val of _axis_table, one row per name
  big/sha              SHA-256 of the outputs of the two 130^3 launches that take the grid-stride loop
  atomic/*             push / pushgrad of 8 source voxels into 16^3.  fp32 atomics commute only up to two addends per
                       address, (0 + a) + b = (0 + b) + a, so the coordinates are checked against that cap on the CPU
                       first (grid_bits_cases.max_addends) and nothing is written if a case breaks it.

python tests/golden/make_golden_grid_bits.py nd -> grid_nd_bits.npz, made from the kernels as they stood before the 2-D
and the 3-D kernels became one dimension-generic set.  It reads its inputs from grid_family_bits.npz and draws nothing.

  cases2d              names of the 2-D cases; pull2d / grad2d hold one entry per case
  atomic2d/*           push of 8 source pixels into 16^2, under the same two-addend cap
  lin3d/*              pull / grad of the all-linear 3-D exports under the two batch broadcasts
  big/*                SHA-256 of the all-linear pull at 130^3 (a second grid-stride round)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import grid_bits_cases as GB  # noqa: E402


def main():
    import torch
    from brainfm_amd import interpol as IP
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "grid_family_bits.npz")
    d = GB.make_inputs()
    GB.check_two_addends(d)                              # raises: no file for coordinates that break the cap
    cases = GB.det_cases()
    res = [GB.run_det_case(IP, torch, d, c) for c in cases]
    d["cases"] = np.array([c[0] for c in cases])
    for k in res[0]:
        d[k] = np.stack([r[k] for r in res])
    tables = GB.table_cases()
    tres = [GB.run_table_case(IP, torch, d, c) for c in tables]
    d["table/names"] = np.array([c[0] for c in tables])
    for i, k in enumerate(("table/rowptr", "table/col", "table/val")):
        d[k] = np.stack([t[i] for t in tres])
    atomics = GB.atomic_cases()
    ares = [GB.run_atomic_case(IP, torch, d, c) for c in atomics]
    d["atomic/names"] = np.array([c[0] for c in atomics])
    d["atomic/push"] = np.stack([a[0] for a in ares])
    d["atomic/pushgrad"] = np.stack([a[1] for a in ares])
    d["big/names"] = np.array(GB.BIG_CASES)
    d["big/sha"] = GB.run_big(IP, torch)
    torch.cuda.synchronize()
    np.savez_compressed(out_path, **d)
    print("%s: %d keys, %d bytes" % (out_path, len(d), os.path.getsize(out_path)))
    for k in ("pull", "grad", "hess", "hessc", "atomic/push", "atomic/pushgrad"):
        print("  %-16s %s  non-zero %.3f  finite %s" % (k, d[k].shape, float((d[k] != 0).mean()), bool(np.isfinite(d[k]).all())))


def main_nd():
    """grid_nd_bits.npz: the 2-D kernels and the gaps of the all-linear 3-D ones, on the inputs grid_family_bits.npz holds"""
    import torch
    from brainfm_amd import interpol as IP
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "grid_nd_bits.npz")
    d = dict(np.load(os.path.join(HERE, "grid_family_bits.npz")))
    GB.check_two_addends2(d)                             # raises: no file for coordinates that break the cap
    out = {}
    cases = GB.det2_cases()
    res = [GB.run_det2_case(IP, torch, d, c) for c in cases]
    out["cases2d"] = np.array([c[0] for c in cases])
    out["pull2d"], out["grad2d"] = (np.stack([r[i] for r in res]) for i in (0, 1))
    atomics = GB.atomic2_cases()
    out["atomic2d/names"] = np.array([c[0] for c in atomics])
    out["atomic2d/push"] = np.stack([GB.run_atomic2_case(IP, torch, d, c) for c in atomics])
    lres = [GB.run_lin3_case(IP, torch, d, c) for c in GB.LIN3_CASES]
    out["lin3d/names"] = np.array([c[0] for c in GB.LIN3_CASES])
    out["lin3d/pull"], out["lin3d/grad"] = (np.stack([r[i] for r in lres]) for i in (0, 1))
    out["big/names"] = np.array(GB.BIG2_CASES)
    out["big/sha"] = GB.run_big2(IP, torch)
    torch.cuda.synchronize()
    np.savez_compressed(out_path, **out)
    print("%s: %d keys, %d bytes" % (out_path, len(out), os.path.getsize(out_path)))
    for k in ("pull2d", "grad2d", "atomic2d/push", "lin3d/pull", "lin3d/grad"):
        print("  %-16s %s  non-zero %.3f  finite %s" % (k, out[k].shape, float((out[k] != 0).mean()),
                                                       bool(np.isfinite(out[k]).all())))


if __name__ == "__main__":
    main_nd() if sys.argv[1:2] == ["nd"] else main()
