"""Float64 numpy restatement of interpol.grid_pull on an integer image (the label branch of utils/interpol/api.py:182-193),
written from its definition and not as a loop of pulls: per output voxel the taps of the footprint (per-axis orders 0 to
3, the seven bounds with their signs, the inbounds mask of `extrapolate`; nodes and weights are those of
tests/spline_grid_refs.py) are summed per label, w_L = sum over the taps whose source voxel holds L of weight * sign, and
the label with the largest w_L > 0 comes out, the smallest label value among equal sums (the reference walks unique() in
ascending order and replaces on a strict >), 0 if no label has a positive sum.

Next to the winner it returns the gap that says how far the winner can be trusted against another precision.  With
S_L = sum of |weight * sign| over the taps of L, a float32 sum w_L is off by a few 2^-24 per weight and 64 * 2^-24 for the
sum, relative to S_L: within 1e-5 * S_L with a factor of two to spare.  The gap is the smallest of
(w_k - w_L) / (S_k + S_L) over the other labels L with a tap of non-zero weight and w_k / S_k for the winner k itself (it
must stay positive); without a winner, the smallest of -w_L / S_L (every sum must stay non-positive).  A voxel is decided
where gap > GAP = 1e-5.  Because the S of a footprint add up to at most 1 (the weights of an axis are a partition of
unity, the signs are -1, 0 or 1), every voxel whose two largest sums differ by more than 1e-5 in absolute terms is
decided: the absolute rule would also throw out the voxels whose only taps have small weights (a `zero` bound two voxels
outside the volume) or small negative ones (`dst1` / `dst2`), which no precision can get wrong, and there are enough of
them to break any cap.  A label none of whose taps has a non-zero weight has the sum 0 exactly in every precision (a
dropped `zero` tap, a masked voxel) and cannot interfere: a voxel outside the field of view has gap = inf and result 0.

Also the label images of the tests and of scripts/bench_label_pull.py (blocky_labels)."""
import itertools

import numpy as np

import spline_grid_refs as SR

GAP = 1e-5          # an fp32 sum of at most 64 weights of magnitude <= 1 is off by at most 64 * 2^-24 = 3.8e-6, twice that
CAP = 0.005         # for a difference (relative to the S above); at most this share of a case's voxels may be undecided


def label_pull(img, grid, orders, bounds, ext):
    """img (Bi, C, X, Y, Z) integer, grid (Bg, *out, 3) -> (winner (B, C, *out) of img's dtype, gap (B, C, *out) float64)"""
    img = np.asarray(img)
    assert img.dtype.kind in "iu"
    shape, oshape = img.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = SR._setup(grid, shape, orders, bounds, ext)
    B, Cc, nvox = max(img.shape[0], g.shape[0]), img.shape[1], g.shape[1]
    labels, inv = np.unique(img, return_inverse=True)                       # ascending
    inv = inv.reshape(img.shape[0], Cc, -1)
    nl = len(labels)
    win = np.zeros((B, Cc, nvox), img.dtype)
    gap = np.zeros((B, Cc, nvox))
    vox = np.arange(nvox)
    for b in range(B):
        (ix, wx, _), (iy, wy, _), (iz, wz, _) = ax[b % g.shape[0]]
        m = mask[b % g.shape[0]]
        for c in range(Cc):
            src = inv[b % img.shape[0], c]
            W = np.zeros((nl, nvox))
            S = np.zeros((nl, nvox))
            for a, e, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
                lin = (ix[a] * shape[1] + iy[e]) * shape[2] + iz[d]
                w = wx[a] * wy[e] * wz[d] * m
                W[src[lin], vox] += w
                S[src[lin], vox] += np.abs(w)
            pmax = np.zeros(nvox)
            out = np.zeros(nvox, img.dtype)
            k = np.full(nvox, -1)
            for q in range(nl):                                             # api.py:186-193, strict >
                better = W[q] > pmax
                out[better] = labels[q]
                k[better] = q
                pmax = np.maximum(pmax, W[q])
            has = k >= 0
            kk = np.maximum(k, 0)
            Wk, Sk = np.where(has, W[kk, vox], 0.0), np.where(has, S[kk, vox], 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(S > 0, (Wk - W) / (Sk + S), np.inf)       # a label without a non-zero tap cannot interfere
                ratio[kk, vox] = np.where(has, Wk / Sk, ratio[kk, vox])
            win[b, c], gap[b, c] = out, ratio.min(0)
    return win.reshape((B, Cc) + tuple(oshape)), gap.reshape((B, Cc) + tuple(oshape))


def decided(gap):
    """the voxels a float32 implementation is held to, and whether the rest stays under the cap"""
    keep = gap > GAP
    return keep, (1.0 - keep.mean()) <= CAP


def blocky_labels(shape, n_labels, seed, block=4):
    """A label image like a segmentation: background 0 outside an ellipsoid, inside it about n_labels - 1 structures, the
    cells of a jittered lattice of seeds (nearest seed, computed on a grid `block` times coarser and repeated, so that the
    borders are blocky like those of an upsampled atlas).  int32, labels 0 .. n_labels - 1."""
    rng = np.random.default_rng(seed)
    coarse = tuple(-(-s // block) for s in shape)
    k = max(1, int(round((n_labels - 1) ** (1.0 / 3.0))))
    cells = [max(1, -(-(n_labels - 1) // (k * k))), k, k]
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in coarse], indexing="ij"), -1).astype(np.float64)
    cell = [np.minimum((idx[..., a] * cells[a] / coarse[a]).astype(np.int64), cells[a] - 1) for a in range(3)]
    # a smooth jitter of the cell borders, then the cell index is the label
    for a in range(3):
        wob = 0.35 * np.sin(idx[..., (a + 1) % 3] * (2 * np.pi / max(coarse[(a + 1) % 3], 1)) * 3 + rng.random() * 6.28)
        cell[a] = np.clip(np.floor(idx[..., a] * cells[a] / coarse[a] + wob), 0, cells[a] - 1).astype(np.int64)
    lab = (cell[0] * cells[1] + cell[1]) * cells[2] + cell[2]
    lab = lab % (n_labels - 1) + 1
    r2 = sum(((idx[..., a] + 0.5) / coarse[a] * 2 - 1) ** 2 / 0.9 ** 2 for a in range(3))
    lab[r2 > 1] = 0
    for a in range(3):
        lab = np.repeat(lab, block, axis=a)
    return np.ascontiguousarray(lab[:shape[0], :shape[1], :shape[2]]).astype(np.int32)
