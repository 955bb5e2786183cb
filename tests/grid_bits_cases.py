"""The cases of tests/golden/grid_family_bits.npz: the bits of the interpol grid kernels (spline_grid.hip, grid_hess.hip,
label_pull.hip, the axis tables of restrict.hip) as they stood before their shared layer was factored out.  The generator
(tests/golden/make_golden_grid_bits.py) and the tests (test_gpu_grid_bits.py, test_host_grid_bits.py) both take the
inputs, the case lists and the calls from here, so what was stored and what is compared cannot drift apart.  The second
half of the file holds the cases of tests/golden/grid_nd_bits.npz in the same way.

Only names that the refactor keeps are used: the C exports and IP._opts / _order_list / _pull_raw / _grad_raw / _hess_raw /
_push_raw / _pushgrad_raw / _label_pull_raw / _axis_table.

Bounds: 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft.  extrapolate: 0 no, 1 yes, 2 hist."""
import ctypes as C
import hashlib
import itertools

import numpy as np

import spline_grid_refs as SR

SEED = 20261020
VOL, GRID = (2, 2, 5, 6, 7), (2, 3, 2, 5)            # (B, C, *in) and (B, *out); the grid is GRID + (3,)
ORDERS = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (3, 1, 2), (0, 2, 1)]
CONFIGS = ([((b, b, b), 1) for b in range(7)] + [((0, 3, 6), 1)] + [((b, b, b), e) for b in (0, 3) for e in (0, 2)])
VARIANTS = (0, 1, 2, 3)                                  # AUTO, LDS, REGS, PASSES
LABEL_DTYPES = ("u8", "i16", "i32", "i64")
FLOAT_OPS = ("pull", "grad", "hess", "hessc")


def otag(o):
    return "o%d%d%d" % tuple(o)


def det_cases():
    """(name, orders, bounds, ext, Bi, Bg): every order under every configuration, then one broadcast each way"""
    out = [("%s/b%d%d%d_e%d" % ((otag(o),) + b + (e,)), o, b, e, 2, 2) for o in ORDERS for b, e in CONFIGS]
    out.append(("o312/b036_e1/Bi1", (3, 1, 2), (0, 3, 6), 1, 1, 2))
    out.append(("o312/b036_e1/Bg1", (3, 1, 2), (0, 3, 6), 1, 2, 1))
    return out


def table_cases():
    """(name, order, bound, transpose, ties_even): m = 9 coordinates against n = 5 nodes, extrapolate 1"""
    out = []
    for order in range(4):
        for bound in (0, 3, 5, 6):
            for tr in (0, 1):
                for ties in ((0, 1) if order == 0 else (0,)):
                    out.append(("t%d/b%d/%s%s" % (order, bound, "push" if tr else "pull", "/even" if ties else ""),
                                order, bound, tr, ties))
    return out


TABLE_M, TABLE_N = 9, 5
ATOMIC_BOUNDS = (0, 3, 6)
ATOMIC_SHAPE = (16, 16, 16)


def atomic_cases():
    """(name, orders, bound): 8 source voxels (2,2,2), C = 2, into 16^3, extrapolate 1"""
    return [("%s/b%d" % (otag(o), b), o, b) for b in ATOMIC_BOUNDS for o in ORDERS]


BIG = 130                                                # 130^3 > 8192 * 256: the grid-stride loop runs a second round
BIG_CASES = ("big/pull_o0", "big/label_o0_u8")


# ------------------------------------------------------------------------------------------------------------- inputs
def make_inputs():
    """Everything the small cases read, from one CPU seed; stored in the fixture, so the tests never draw anything."""
    rng = np.random.default_rng(SEED)
    d = {}
    d["in/vol"] = rng.standard_normal(VOL).astype(np.float32)
    g = np.empty(GRID + (3,), np.float32)
    for a in range(3):
        g[..., a] = (rng.random(GRID) * (VOL[2 + a] + 5.0) - 3.0).astype(np.float32)
    # the floor ties of the odd orders (integers) and of the even ones (half-integers), which are also the branch points of
    # the weight functions (node distances 0, 0.5, 1, 1.5, 2): inside, on both faces and outside, in both batches
    flat = g.reshape(2, -1, 3)
    nx, ny, nz = VOL[2:]
    special = [(2.0, 3.0, 1.0), (0.0, 0.0, 0.0), (nx - 1.0, ny - 1.0, nz - 1.0), (-1.0, float(ny), -2.0),
               (1.5, 2.5, 3.5), (-0.5, -0.5, -0.5), (nx - 0.5, ny - 0.5, nz - 0.5), (0.5, 4.0, -1.5),
               (3.0, 0.5, 5.5), (float(nx), 1.5, 6.0), (2.5, -1.0, 3.0), (-2.5, 6.5, 8.0)]
    for b in range(2):
        for i, p in enumerate(special):
            flat[b, (7 * i + 3 * b) % flat.shape[1]] = p if b == 0 else p[::-1][:1] + p[:2]
    d["in/grid"] = g
    d["in/cot"] = rng.standard_normal(GRID[:1] + VOL[1:2] + GRID[1:] + (3,)).astype(np.float32)
    idx = rng.integers(0, 6, VOL)
    blocks = rng.integers(0, 6, VOL[:2] + tuple(-(-s // 2) for s in VOL[2:]))
    for a in range(3):
        blocks = np.repeat(blocks, 2, axis=2 + a)
    d["in/labels"] = np.where(rng.random(VOL) < 0.6, blocks[:, :, :nx, :ny, :nz], idx).astype(np.int64)
    c = (rng.random(TABLE_M) * (TABLE_N + 5.0) - 3.0).astype(np.float32)
    c[[0, 2, 4, 6, 8]] = (2.0, 0.5, -1.0, 4.5, 5.0)
    d["in/coord"] = c
    d["atomic/src"] = rng.standard_normal((1, 2, 2, 2, 2)).astype(np.float32)
    d["atomic/src3"] = rng.standard_normal((1, 2, 2, 2, 2, 3)).astype(np.float32)
    # four places of 16^3 far from each other hold two source voxels each whose footprints overlap, or one voxel whose
    # footprint leaves the volume through one face only (a fold puts two of its own nodes on one address)
    base = np.array([(3.3, 3.6, 3.2), (4.7, 4.3, 5.3), (3.7, 11.2, 10.4), (5.0, 12.5, 11.0),
                     (11.4, 3.1, 11.7), (12.6, 4.9, 9.9), (0.3, 11.3, 3.4), (11.5, 14.8, 4.5)], np.float32)
    for b in ATOMIC_BOUNDS:
        jit = (rng.random(base.shape) * 0.2 - 0.1).astype(np.float32)
        jit[3] = 0.0                                     # keeps its integer and half-integer coordinates
        d["atomic/grid_b%d" % b] = (base + jit).reshape(1, 2, 2, 2, 3)
    return d


def label_image(base, tag):
    """The label indices 0..5 as labels of each dtype: negative ones for the signed types, both halves of an int64"""
    if tag == "u8":
        return (base * 51).astype(np.uint8)
    if tag == "i16":
        return ((base - 2) * 1500).astype(np.int16)
    if tag == "i32":
        return ((base - 2) * 70001).astype(np.int32)
    return (base - 2) * ((1 << 33) + 5)


def big_inputs():
    """130^3 volume, labels and identity-plus-jitter grid from integer arithmetic alone (no generator to depend on)"""
    n = BIG ** 3
    i = np.arange(n, dtype=np.int64)
    vol = (((i * 40503) % 2048).astype(np.float32) / 1024.0 - 1.0).reshape(1, 1, BIG, BIG, BIG)
    lab = ((((i // 3) * 2654435761) >> 7) % 6).astype(np.uint8).reshape(1, 1, BIG, BIG, BIG)
    ident = np.stack(np.meshgrid(*[np.arange(BIG, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(n, 3)
    k = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    jit = ((k * 2246822519 + 374761393) % 4096).astype(np.float32) / 4096.0 * 1.5 - 0.75
    return vol, lab, (ident + jit).reshape(1, BIG, BIG, BIG, 3)


# ------------------------------------------------------------------------------- the two-addend cap of the atomic cases
def max_addends(grid, shape, orders, bound):
    """The largest number of atomic adds that any address of `shape` (2 or 3 extents) can receive from the source voxels
    at `grid` (1, ..., len(shape)): every node of every voxel's footprint that the bound does not drop (sign != 0) counts,
    whatever its weight, with the node indices of the float64 restatement.  A cap, not a measurement."""
    dim = len(shape)
    g = np.asarray(grid, np.float64).reshape(-1, dim)
    ax = []
    for a in range(dim):
        g0 = np.floor(g[:, a] - (orders[a] - 1) / 2).astype(np.int64)
        nodes = np.stack([g0 + k for k in range(orders[a] + 1)])
        ax.append((SR.bound_index(nodes, shape[a], bound), SR.bound_sign(nodes, shape[a], bound) != 0))
    count = np.zeros(int(np.prod(shape)), np.int64)
    for taps in itertools.product(*[range(orders[a] + 1) for a in range(dim)]):
        live, lin = True, 0
        for a, k in enumerate(taps):
            live = live & ax[a][1][k]
            lin = lin * shape[a] + ax[a][0][k]
        np.add.at(count, lin[live], 1)
    return int(count.max())


def check_two_addends(d):
    for name, o, b in atomic_cases():
        m = max_addends(d["atomic/grid_b%d" % b], ATOMIC_SHAPE, o, b)
        if m > 2:
            raise ValueError("%s: an address receives %d addends; the sum would depend on their order" % (name, m))


# ------------------------------------------------------------------------- the second fixture: tests/golden/grid_nd_bits.npz
# What grid_family_bits.npz does not pin, taken from the kernels as they stood before the 2-D and the 3-D kernels became
# one dimension-generic set: pull / grad / push on 2-D grids, the two batch broadcasts of the all-linear 3-D kernels and
# their second grid-stride round.  Every input is one of the first fixture's (`d` below is that fixture): nothing is drawn.
ORDERS2 = [(0, 0), (1, 1), (2, 2), (3, 3), (3, 1), (0, 2)]
ATOMIC_SHAPE2 = (16, 16)
BIG2_CASES = ("big/pull_o111",)
LIN3_CASES = (("o111/b036_e1/Bi1", 1, 2), ("o111/b036_e1/Bg1", 2, 1))


def otag2(o):
    return "o%d%d" % tuple(o)


def _pad3(v):
    """two per-axis values -> the three an export reads its first two of, padded with the last like IP._opts pads"""
    return tuple(v) + (v[-1],)


def inputs2d(d):
    """image (2,2,5,6): the first slice of in/vol along z; grid (2,6,5,2): the x and y coordinates of in/grid, which keeps
    the integer and half-integer ties against nx = 5, ny = 6"""
    return np.ascontiguousarray(d["in/vol"][..., 0]), np.ascontiguousarray(d["in/grid"][..., :2]).reshape(2, 6, 5, 2)


def det2_cases():
    """(name, orders, bounds, ext, Bi, Bg): every 2-D order under the first two bounds of every configuration, then one
    broadcast each way"""
    out = [("%s/b%d%d_e%d" % ((otag2(o),) + b[:2] + (e,)), o, b[:2], e, 2, 2) for o in ORDERS2 for b, e in CONFIGS]
    out.append(("o31/b03_e1/Bi1", (3, 1), (0, 3), 1, 1, 2))
    out.append(("o31/b03_e1/Bg1", (3, 1), (0, 3), 1, 2, 1))
    return out


def run_det2_case(IP, torch, d, case):
    """-> pull (B,C,6,5), grad (B,C,6,5,2).  Bi == Bg goes through the _raw wrappers, a broadcast through the exports."""
    from brainfm_amd import _lib as L
    name, o, b, ext, Bi, Bg = case
    vol, grid = inputs2d(d)
    x, g = _dev(vol[:Bi], torch), _dev(grid[:Bg], torch)
    if Bi == Bg:
        res = IP._pull_raw(x, g, _c3(_pad3(b)), _pad3(o), ext), IP._grad_raw(x, g, _c3(_pad3(b)), _pad3(o), ext)
    else:
        B, Cc, gs = max(Bi, Bg), x.shape[1], tuple(g.shape[1:3])
        lib = L.load()
        head = (L.ptr(x), Bi, Cc, x.shape[2], x.shape[3], L.ptr(g), Bg, gs[0], gs[1], _c3(_pad3(b)), _c3(_pad3(o)), ext)
        pull = torch.empty((B, Cc) + gs, dtype=torch.float32, device=x.device)
        grad = torch.empty((B, Cc) + gs + (2,), dtype=torch.float32, device=x.device)
        L.check(lib.bfm_grid_pull2d_spline(*head, L.ptr(pull), L.stream_ptr()), "pull2d")
        L.check(lib.bfm_grid_grad2d_spline(*head, L.ptr(grad), L.stream_ptr()), "grad2d")
        res = pull, grad
    return res[0].cpu().numpy(), res[1].cpu().numpy()


def atomic2_inputs(d, bound):
    """source (1,2,2,4) and grid (1,2,4,2): the 8 source voxels of the 3-D atomic cases with their x and y coordinates"""
    return (d["atomic/src"].reshape(1, 2, 2, 4),
            np.ascontiguousarray(d["atomic/grid_b%d" % bound][..., :2]).reshape(1, 2, 4, 2))


def atomic2_cases():
    """(name, orders, bound): 8 source pixels, C = 2, into 16^2, extrapolate 1"""
    return [("%s/b%d" % (otag2(o), b), o, b) for b in ATOMIC_BOUNDS for o in ORDERS2]


def check_two_addends2(d):
    for name, o, b in atomic2_cases():
        m = max_addends(atomic2_inputs(d, b)[1], ATOMIC_SHAPE2, o, b)
        if m > 2:
            raise ValueError("%s: an address receives %d addends; the sum would depend on their order" % (name, m))


def run_atomic2_case(IP, torch, d, case):
    name, o, b = case
    src, grid = atomic2_inputs(d, b)
    return IP._push_raw(_dev(src, torch), _dev(grid, torch), ATOMIC_SHAPE2, _c3((b, b, b)), _pad3(o), 1).cpu().numpy()


def run_lin3_case(IP, torch, d, case):
    """The all-linear 3-D exports under a batch broadcast, which the _raw wrappers do not take: bounds (0,3,6),
    extrapolate 1 -> pull (2,2,3,2,5), grad (2,2,3,2,5,3)"""
    from brainfm_amd import _lib as L
    name, Bi, Bg = case
    x, g = _dev(d["in/vol"][:Bi], torch), _dev(d["in/grid"][:Bg], torch)
    B, Cc, gs = max(Bi, Bg), x.shape[1], tuple(g.shape[1:4])
    lib = L.load()
    head = (L.ptr(x), Bi, Cc, x.shape[2], x.shape[3], x.shape[4], L.ptr(g), Bg, gs[0], gs[1], gs[2], _c3((0, 3, 6)), 1)
    pull = torch.empty((B, Cc) + gs, dtype=torch.float32, device=x.device)
    grad = torch.empty((B, Cc) + gs + (3,), dtype=torch.float32, device=x.device)
    L.check(lib.bfm_grid_pull3d_linear(*head, L.ptr(pull), L.stream_ptr()), "pull3d_linear")
    L.check(lib.bfm_grid_grad3d_linear(*head, L.ptr(grad), L.stream_ptr()), "grad3d_linear")
    return pull.cpu().numpy(), grad.cpu().numpy()


def run_big2(IP, torch):
    """-> the SHA-256 of the all-linear pull of big_inputs() under dct2, extrapolate 1: (1, 32) uint8"""
    vol, _, grid = big_inputs()
    pull = IP._pull_raw(_dev(vol, torch), _dev(grid, torch), _c3((3, 3, 3)), (1, 1, 1), 1).cpu().numpy()
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(pull).tobytes()).digest(), np.uint8).reshape(1, 32)


# --------------------------------------------------------------------------------------------------- calls on the device
def _dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _c3(v):
    return (C.c_int * 3)(*v)


def run_float(IP, torch, x, g, cot, o, b, ext):
    """pull, grad, hess, hess contracted with cot -> numpy.  Bi == Bg goes through the _raw wrappers; a broadcast, which
    they do not take, through the exports themselves."""
    from brainfm_amd import _lib as L
    Bi, Bg, Cc = x.shape[0], g.shape[0], x.shape[1]
    if Bi == Bg:
        bb = _c3(b)
        res = (IP._pull_raw(x, g, bb, o, ext), IP._grad_raw(x, g, bb, o, ext), IP._hess_raw(x, g, bb, o, ext),
               IP._hess_raw(x, g, bb, o, ext, cot=cot))
    else:
        B, gs = max(Bi, Bg), tuple(g.shape[1:4])
        lib = L.load()
        head = (L.ptr(x), Bi, Cc, x.shape[2], x.shape[3], x.shape[4], L.ptr(g), Bg, gs[0], gs[1], gs[2], _c3(b), _c3(o), ext)
        pull = torch.empty((B, Cc) + gs, dtype=torch.float32, device=x.device)
        grad = torch.empty((B, Cc) + gs + (3,), dtype=torch.float32, device=x.device)
        hess = torch.empty((B, Cc) + gs + (3, 3), dtype=torch.float32, device=x.device)
        hessc = torch.empty((B,) + gs + (3,), dtype=torch.float32, device=x.device)
        L.check(lib.bfm_grid_pull3d_spline(*head, L.ptr(pull), L.stream_ptr()), "pull")
        L.check(lib.bfm_grid_grad3d_spline(*head, L.ptr(grad), L.stream_ptr()), "grad")
        L.check(lib.bfm_grid_hess3d(*head, None, L.ptr(hess), L.stream_ptr()), "hess")
        L.check(lib.bfm_grid_hess3d(*head, L.ptr(cot), L.ptr(hessc), L.stream_ptr()), "hessc")
        res = (pull, grad, hess, hessc)
    return dict(zip(FLOAT_OPS, (r.cpu().numpy() for r in res)))


def run_det_case(IP, torch, d, case):
    """-> {'pull': ..., 'grad': ..., 'hess': ..., 'hessc': ..., 'label/u8': (4 variants, ...), ...}"""
    name, o, b, ext, Bi, Bg = case
    g = _dev(d["in/grid"][:Bg], torch)
    out = run_float(IP, torch, _dev(d["in/vol"][:Bi], torch), g, _dev(d["in/cot"], torch), o, b, ext)
    for tag in LABEL_DTYPES:
        x = _dev(label_image(d["in/labels"][:Bi], tag), torch)
        out["label/" + tag] = np.stack([IP._label_pull_raw(x, g, _c3(b), o, ext, v).cpu().numpy() for v in VARIANTS])
    return out


def run_table_case(IP, torch, d, case):
    """-> rowptr (TABLE_M + 1, padded with -1), col and val (4 * TABLE_M, zero behind the last entry)"""
    name, order, bound, tr, ties = case
    rowptr, col, val, rows = IP._axis_table(_dev(d["in/coord"], torch), TABLE_N, order, bound, 1, bool(tr), bool(ties))
    rowptr, col, val = rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    assert rows == (TABLE_N if tr else TABLE_M) and rowptr.shape == (rows + 1,)
    nnz = int(rowptr[-1])
    rp = np.full(TABLE_M + 1, -1, np.int32)
    rp[:rows + 1] = rowptr
    cc, vv = np.zeros(4 * TABLE_M, np.int32), np.zeros(4 * TABLE_M, np.float32)
    cc[:nnz], vv[:nnz] = col[:nnz], val[:nnz]
    return rp, cc, vv


def run_atomic_case(IP, torch, d, case):
    name, o, b = case
    g = _dev(d["atomic/grid_b%d" % b], torch)
    push = IP._push_raw(_dev(d["atomic/src"], torch), g, ATOMIC_SHAPE, _c3((b, b, b)), o, 1)
    pushgrad = IP._pushgrad_raw(_dev(d["atomic/src3"], torch), g, ATOMIC_SHAPE, _c3((b, b, b)), o, 1)
    return push.cpu().numpy(), pushgrad.cpu().numpy()


def run_big(IP, torch):
    """-> the SHA-256 of the output bytes of BIG_CASES, (2, 32) uint8"""
    vol, lab, grid = big_inputs()
    g = _dev(grid, torch)
    b = _c3((3, 3, 3))
    pull = IP._pull_raw(_dev(vol, torch), g, b, (0, 0, 0), 1).cpu().numpy()
    label = IP._label_pull_raw(_dev(lab, torch), g, b, (0, 0, 0), 1).cpu().numpy()
    return np.stack([np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
                     for a in (pull, label)])
