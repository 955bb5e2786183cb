"""Golden vectors for the label branch of interpol.grid_pull (an integer image: one pull per label of unique(), the label
with the largest interpolated weight wins), for the grid builders identity_grid / add_identity_grid / affine_grid and
for spline_coeff along one dimension, from the reference's vendored torch-interpol on the CPU (utils/interpol/api.py).

Run: python tests/golden/make_golden_label_pull.py -> label_pull.npz (small arrays only).

Label pull.  Three images with B = 2, C = 2, each pulled through one grid of shape (2, 6, 7, 5, 3) whose coordinates are
uniform in [-2.5, n + 1.5]:
  P  (2,2,9,8,7)  labels {-7, -1, 0, 3, 12, 200, 70000}, run as int64 and as int32 (asserted equal, stored once)
  Q  (2,2,7,6,5)  labels {0, 1, 2, 5, 77, 255}, uint8
  S  (2,2,7,6,5)  labels {-300, -2, 0, 5, 77, 3000}, int16 (the voxels of Q under another map)
for the orders 0, 1, 2, 3, [1,3,0], [2,1,3], the seven bounds and extrapolate False / True: key
<image>/<order tag>/b<bound>_e<extrapolate>.  The reference runs with a float64 grid; its float32 run is compared in
tests/test_host_label_pull.py's terms here as well (it must agree wherever the float64 gap exceeds 1e-5) and the number
of voxels where the two runs differ is printed.

Grid builders: float32 and float64, shape (5,6,7), matrices (3,4) and (4,4) with batch shapes (), (2,), (2,3).  The
reference's affine_grid raises on a batched matrix (it un-squeezes the matrix before slicing it), so the batched arrays
are its un-batched results stacked matrix by matrix.
spline_coeff: orders 2 and 3 under dct1, dct2, dft along dim -1, 0, 1 of a (5,6,7) and a (3,5,4,6) tensor; float64 run
rounded to float32 with max|ref32 - ref64| next to it (`.err`), like the other fixtures of this family."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402
import label_pull_refs as LR  # noqa: E402

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o130": [1, 3, 0], "o213": [2, 1, 3]}
SETS = {"P": ([-7, -1, 0, 3, 12, 200, 70000], np.int64), "Q": ([0, 1, 2, 5, 77, 255], np.uint8),
        "S": ([-300, -2, 0, 5, 77, 3000], np.int16)}
INS = {"P": (9, 8, 7), "Q": (7, 6, 5), "S": (7, 6, 5)}
OUTS = (6, 7, 5)


def draw_image(rng, ins, n):
    """label indices: random per voxel, then a majority of 2 x 2 x 2 blocks made uniform, so that footprints hold from one
    to many distinct labels"""
    idx = rng.integers(0, n, (2, 2) + ins)
    blocks = rng.integers(0, n, (2, 2) + tuple(-(-s // 2) for s in ins))
    for a in range(3):
        blocks = np.repeat(blocks, 2, axis=2 + a)
    blocks = blocks[:, :, :ins[0], :ins[1], :ins[2]]
    return np.where(rng.random((2, 2) + ins) < 0.6, blocks, idx)


def main():
    from utils import interpol
    from utils.interpol import api
    rng = np.random.default_rng(41)
    out = {}
    idx_small = draw_image(rng, INS["Q"], 6)
    images = {"P": np.asarray(SETS["P"][0])[draw_image(rng, INS["P"], 7)].astype(np.int64),
              "Q": np.asarray(SETS["Q"][0])[idx_small].astype(np.uint8),
              "S": np.asarray(SETS["S"][0])[idx_small].astype(np.int16)}
    differ = total = 0
    for tag, img in images.items():
        ins = INS[tag]
        grid = (rng.random((2,) + OUTS + (3,)) * (np.array(ins) + 4.0) - 2.5).astype(np.float32)
        out[tag + "/img"], out[tag + "/grid"] = img, grid
        for otag, order in ORDERS.items():
            for bound in range(7):
                for ext in (0, 1):
                    k = "%s/%s/b%d_e%d" % (tag, otag, bound, ext)
                    ti = torch.from_numpy(img)
                    r64 = interpol.grid_pull(ti, torch.from_numpy(grid).double(), order, bound, bool(ext))
                    r32 = interpol.grid_pull(ti, torch.from_numpy(grid), order, bound, bool(ext))
                    assert r64.dtype == ti.dtype and tuple(r64.shape) == (2, 2) + OUTS
                    if tag == "P":
                        r_i32 = interpol.grid_pull(ti.to(torch.int32), torch.from_numpy(grid).double(), order, bound, bool(ext))
                        assert r_i32.dtype == torch.int32 and torch.equal(r_i32.long(), r64)
                    win, gap = LR.label_pull(img, grid, order, bound, ext)
                    keep, under = LR.decided(gap)
                    assert under, k
                    assert np.array_equal(win[keep], r64.numpy()[keep]), k
                    assert np.array_equal(r32.numpy()[keep], r64.numpy()[keep]), k
                    differ += int((r32 != r64).sum())
                    total += r64.numel()
                    out[k] = r64.numpy()
    print("label pull: %d cases, %d of %d voxels differ between the reference's float32 and float64 runs" %
          (len([k for k in out if "/b" in k]), differ, total))

    # ---- grid builders
    g = torch.Generator().manual_seed(41)
    shape = (5, 6, 7)
    for dt, dn in ((torch.float32, "f32"), (torch.float64, "f64")):
        out["builders/identity_" + dn] = interpol.identity_grid(shape, dtype=dt).numpy()
        for bs, bn in (((), "b"), ((2,), "b2"), ((2, 3), "b23")):
            disp = torch.randn(bs + shape + (3,), generator=g, dtype=torch.float64).to(dt) * 3
            out["builders/disp_%s_%s" % (bn, dn)] = disp.numpy()
            out["builders/add_%s_%s" % (bn, dn)] = interpol.add_identity_grid(disp).numpy()
            for rows in (3, 4):
                mat = torch.randn(bs + (rows, 4), generator=g, dtype=torch.float64).to(dt)
                k = "builders/affine%d_%s_%s" % (rows, bn, dn)
                out[k + "_mat"] = mat.numpy()
                if bs:
                    # the reference un-squeezes a batched matrix before it slices it (api.py:552-558) and then fails in
                    # matvec: the batched result is its own un-batched result, matrix by matrix
                    try:
                        api.affine_grid(mat, shape)
                        raise AssertionError("the reference takes batched matrices now: store its result instead")
                    except RuntimeError:
                        pass
                    res = torch.stack([api.affine_grid(m, shape) for m in mat.reshape(-1, rows, 4)]).reshape(
                        bs + shape + (3,))
                else:
                    res = api.affine_grid(mat, shape)
                assert tuple(res.shape) == bs + shape + (3,), (k, res.shape)
                out[k] = res.numpy()
    # ---- spline_coeff along one dimension
    for tn, tshape in (("t3", (5, 6, 7)), ("t4", (3, 5, 4, 6))):
        x = torch.randn(tshape, generator=g)
        out["coeff/%s" % tn] = x.numpy()
        for order in (2, 3):
            for bound in ("dct1", "dct2", "dft"):
                for dim in (-1, 0, 1):
                    k = "coeff/%s/o%d_%s_d%d" % (tn, order, bound, dim)
                    r64 = interpol.spline_coeff(x.double(), order, bound, dim)
                    r32 = interpol.spline_coeff(x.clone(), order, bound, dim)
                    out[k] = r64.float().numpy()
                    out[k + ".err"] = np.float64((r32.double() - r64).abs().max().item())
    path = os.path.join(HERE, "label_pull.npz")
    np.savez_compressed(path, **out)
    print("label_pull.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
