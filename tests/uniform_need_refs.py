"""numpy restatements for tests/test_gpu_uniform_need.py: the uniform-box flags of an image (the rule of
test_uniform_background_boxes_change_no_bit), the `need` table behind them, and the layout of the flag buffer."""
import numpy as np


def ellipsoid_volume(dims, seed=3):
    """The volume of test_uniform_background_boxes_change_no_bit: an off-centre ellipsoid of rand + 0.05, zero outside."""
    import torch
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n_) for n_ in dims], indexing="ij")
    inside = torch.from_numpy((zz / 0.45) ** 2 + (yy / 0.4) ** 2 + ((xx + 0.5) / 0.3) ** 2 < 1)
    return (torch.rand(dims, generator=g) + 0.05) * inside


def grid(ldims, box):
    return tuple(-(-ldims[a] // box[a]) for a in range(3))


def flags(img, dims, box, lvl, rad):
    """flags[box] = 0, or 1 + class, for the box grid of the tensor `lvl` poolings down; img: the (D,H,W) float32 image."""
    ld = tuple(v >> lvl for v in dims)
    nt = grid(ld, box)
    bits = np.ascontiguousarray(img).view(np.uint32)
    out = []
    for iz in range(nt[0]):
        for iy in range(nt[1]):
            for ix in range(nt[2]):
                org = (iz * box[0], iy * box[1], ix * box[2])
                lo = [max((v << lvl) - rad, 0) for v in org]
                hi = [min(((v + b) << lvl) + rad, d) for v, b, d in zip(org, box, dims)]
                blk = bits[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                ok = bool((blk == blk.flat[0]).all())
                c = [0 if i == 0 else (2 if i == n - 1 else 1) for i, n in zip((iz, iy, ix), nt)]
                far = any(i != n - 1 and (((i + 1) * b) << lvl) + rad > ((d >> lvl) << lvl)
                          for i, n, b, d in zip((iz, iy, ix), nt, box, dims))
                out.append(1 + 9 * c[0] + 3 * c[1] + c[2] if ok and not far else 0)
    return np.array(out, dtype=np.uint8), nt


def first_boxes(fl):
    """first[c] = the first box of class c, len(fl) where there is none."""
    first = np.full(27, fl.size, dtype=np.int32)
    for c in range(27):
        hit = np.flatnonzero(fl == c + 1)
        if hit.size:
            first[c] = hit[0]
    return first


def need(fl, nt):
    """need[b] = 1 iff b is flagged, is not its class's first box, and one of its up to 26 neighbours inside the grid is
    unflagged or a class's first box.  Returns (need uint8 [n], computed bool [n])."""
    first = first_boxes(fl)
    idx = np.arange(fl.size)
    computed = (fl == 0) | (first[np.maximum(fl.astype(np.int64) - 1, 0)] == idx)
    comp3 = computed.reshape(nt)
    pad = np.zeros(tuple(n + 2 for n in nt), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = comp3
    near = np.zeros(nt, dtype=bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near |= pad[dz:dz + nt[0], dy:dy + nt[1], dx:dx + nt[2]]
    nd = (~comp3) & near
    return nd.reshape(-1).astype(np.uint8), computed


def parse(raw, n):
    """The fields of a flag buffer of n boxes (numpy uint8 array of bfm_uniform_boxes_bytes bytes)."""
    p4 = (n + 3) // 4 * 4
    words = raw[p4:p4 + 4 * (27 + 2 + 2 * n + 1 + n)].view(np.int32)
    need_off = p4 + 4 * (27 + 2 + 2 * n + 1 + n)
    assert raw.size == need_off + p4, (raw.size, need_off + p4)
    return dict(flags=raw[:n], first=words[:27], counts=words[27:29], rest=words[29:29 + n], uniform=words[29 + n:29 + 2 * n],
                need_count=int(words[29 + 2 * n]), need_list=words[30 + 2 * n:30 + 3 * n], need=raw[need_off:need_off + n])


def box_mask(per_box, nt, box, ldims):
    """(D,H,W) bool: a per-box boolean spread over the boxes' voxels, clipped to the tensor."""
    m = np.asarray(per_box, dtype=bool).reshape(nt)
    m = m.repeat(box[0], 0).repeat(box[1], 1).repeat(box[2], 2)
    return m[:ldims[0], :ldims[1], :ldims[2]]
