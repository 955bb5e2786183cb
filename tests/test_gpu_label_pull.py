"""interpol.grid_pull on integer (label) images on the device (brainfm_amd/csrc/label_pull.hip), the grid builders
(grid_builders.hip) and spline_coeff along one dimension, against the reference's own results
(tests/golden/label_pull.npz) and the float64 restatement of tests/label_pull_refs.py.

Label maps are compared exactly, at every voxel that the restatement's gap decides (gap > 1e-5; label_pull_refs.py
derives the figure and why it is taken relative to the weights of the two labels), and at most 0.5 % of a case's voxels
may be left out; tests/test_host_label_pull.py shows with the reference alone that the stored cases meet that cap.  The
tie and copy tests have no tolerance.  Grid builders are bit-equal to the reference.  spline_coeff is held to the bar of
spline_coeff_nd's test (test_gpu_spline_grid.py): max|hip - ref| <= 2e-5 * max(1, max|ref|)."""
import numpy as np
import pytest
import torch

from conftest import load_npz
import label_pull_refs as LR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o130": [1, 3, 0], "o213": [2, 1, 3]}
DTYPES = {"P": (torch.int64, torch.int32), "Q": (torch.uint8,), "S": (torch.int16,)}
_D = {}


def golden():
    if not _D:
        _D.update(load_npz("label_pull.npz"))
    return _D


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def held(got, win, gap, what):
    """got (device tensor) equals win wherever the gap decides; the undecided share stays under the cap"""
    keep, under = LR.decided(gap)
    assert under, (what, 1.0 - keep.mean())
    got = got.cpu().numpy()
    assert got.shape == win.shape, (what, got.shape, win.shape)
    bad = (got != win) & keep
    assert not bad.any(), (what, int(bad.sum()), got[bad][:5], win[bad][:5])
    return 1.0 - keep.mean()


# ------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("otag", list(ORDERS))
@pytest.mark.parametrize("tag", list(DTYPES))
def test_parity_with_the_reference(tag, otag):
    """The stored cases: 9x8x7 (P; int64 and int32, labels -7 .. 70000) and 7x6x5 (Q uint8, S int16 with negative labels)
    images with B = 2 and C = 2 pulled onto a 6x7x5 grid with coordinates in [-2.5, n + 1.5], the seven bounds,
    extrapolate both ways.  Dtype and shape as the reference; labels equal to the reference's and to the restatement's
    at every decided voxel.  On a commit that samples an integer image as values this fails at the dtype."""
    from brainfm_amd import interpol as IP
    d = golden()
    img, grid = d[tag + "/img"], d[tag + "/grid"]
    tg = T(grid)
    worst = 0.0
    for bound in range(7):
        for ext in (0, 1):
            k = "%s/%s/b%d_e%d" % (tag, otag, bound, ext)
            ref = d[k]
            win, gap = LR.label_pull(img, grid, ORDERS[otag], bound, ext)
            for dt in DTYPES[tag]:
                got = IP.grid_pull(T(img).to(dt), tg, ORDERS[otag], bound, bool(ext))
                assert got.dtype == dt and tuple(got.shape) == ref.shape == (2, 2, 6, 7, 5), (k, got.dtype, got.shape)
                worst = max(worst, held(got.long(), ref.astype(np.int64), gap, k + " vs the reference"))
                held(got.long(), win.astype(np.int64), gap, k + " vs the restatement")
    print("%s %s: largest undecided share %.4f" % (tag, otag, worst))


def test_batch_broadcast_channelless_input_and_float64_grid():
    """One image under two grids, two images under one grid, the (X, Y, Z) form, and a float64 grid (taken like the float
    path takes it: rounded to float32, here a no-op on float32 values)."""
    from brainfm_amd import interpol as IP
    d = golden()
    img, grid = d["S/img"], d["S/grid"]
    timg, tg = T(img), T(grid)
    for order, bound, ext in ((1, 3, 1), (3, 0, 0), ([2, 1, 3], 5, 1)):
        got = IP.grid_pull(timg[:1], tg, order, bound, bool(ext))
        assert tuple(got.shape) == (2, 2, 6, 7, 5)
        held(got, *LR.label_pull(img[:1], grid, order, bound, ext), "Bi=1")
        got = IP.grid_pull(timg, tg[:1], order, bound, bool(ext))
        held(got, *LR.label_pull(img, grid[:1], order, bound, ext), "Bg=1")
        got = IP.grid_pull(timg[0, 0], tg[0], order, bound, bool(ext))
        assert tuple(got.shape) == (6, 7, 5) and got.dtype == torch.int16
        win, gap = LR.label_pull(img[:1, :1], grid[:1], order, bound, ext)
        held(got, win[0, 0], gap[0, 0], "(X,Y,Z)")
        assert torch.equal(got, IP.grid_pull(timg[0, 0], tg[0].double(), order, bound, bool(ext)))
        got = IP.grid_pull(timg[0], tg[0], order, bound, bool(ext))              # (C, X, Y, Z) under an unbatched grid
        assert tuple(got.shape) == (2, 6, 7, 5)
        held(got[None], *LR.label_pull(img[:1], grid[:1], order, bound, ext), "(C,X,Y,Z)")
    assert not IP.grid_pull(timg, tg, 1).requires_grad


# ---------------------------------------------------------------------------------------- 2. exact ties and exact copies
def blocks_of_two(shape, rng):
    """every voxel shares its label with its 2 x 2 x 2 block, and all blocks differ"""
    coarse = tuple(s // 2 for s in shape)
    lab = rng.permutation(int(np.prod(coarse))).reshape(coarse) * 7 - 40
    for a in range(3):
        lab = np.repeat(lab, 2, axis=a)
    return lab


@pytest.mark.parametrize("order", [0, 1, 2, 3, [1, 3, 0], [2, 1, 3]])
def test_integer_coordinates_return_the_image(order):
    """No tolerance.  Orders 0 and 1 interpolate, so any image comes back: one label per voxel at random.  Orders 2 and 3
    do not (no prefilter): at an integer coordinate the voxel itself has the weight 3/4 or 2/3 per axis, (3/4)^3 < 1/2, and
    a voxel whose 26 neighbours share another label loses to them.  There the image is made of 2 x 2 x 2 blocks: a voxel
    and its block mates hold at least 7/8 (5/6) per axis, (5/6)^3 = 0.58 of the whole weight of 1, under 'dct2' also at
    the faces, where the reflection lands in the same block."""
    from brainfm_amd import interpol as IP
    rng = np.random.default_rng(3)
    shape = (8, 6, 4)
    orders = order if isinstance(order, list) else [order] * 3
    if max(orders) <= 1:
        img = rng.choice(np.array([-9, -1, 0, 2, 40, 70000]), size=(2,) + shape)
    else:
        img = np.stack([blocks_of_two(shape, rng), blocks_of_two(shape, rng)])
    grid = IP.identity_grid(shape, dtype=torch.float32, device=DEV)
    for dt in (torch.int32, torch.int64):
        seg = T(img).to(dt)
        got = IP.grid_pull(seg, grid, order, "dct2", True)
        assert got.dtype == dt and torch.equal(got, seg)
        assert torch.equal(IP.grid_pull(seg, grid, order, "dct2", False), seg)


def test_exact_ties_go_to_the_smaller_label_and_no_weight_gives_zero():
    """A coordinate at an exact half along one axis and at integers along the others has exactly two taps of weight 0.5 at
    order 1 (the other six are exactly 0): where the two neighbours differ the smaller label comes out, negative labels
    included.  A voxel with no positive weight gives 0."""
    from brainfm_amd import interpol as IP
    rng = np.random.default_rng(4)
    shape = (7, 6, 5)
    img = rng.choice(np.array([-300, -2, 0, 5, 77, 3000]), size=shape)
    for dt in (torch.int16, torch.int32, torch.int64):
        seg = T(img).to(dt)
        for axis in range(3):
            grid = IP.identity_grid(shape, dtype=torch.float32, device=DEV)
            grid = grid.narrow(axis, 0, shape[axis] - 1).clone()
            grid[..., axis] += 0.5
            lo = np.take(img, np.arange(shape[axis] - 1), axis)
            hi = np.take(img, np.arange(1, shape[axis]), axis)
            assert (lo != hi).mean() > 0.5
            for bound in ("dct2", "zero", "dft"):
                got = IP.grid_pull(seg, grid, 1, bound, True)
                assert np.array_equal(got.cpu().numpy(), np.minimum(lo, hi)), (dt, axis, bound)
    # uint8: the same rule among non-negative labels
    img8 = rng.choice(np.array([0, 1, 2, 200, 255]), size=shape).astype(np.uint8)
    grid = IP.identity_grid(shape, dtype=torch.float32, device=DEV)[:, :, :-1].clone()
    grid[..., 2] += 0.5
    got = IP.grid_pull(T(img8), grid, 1, "dct2", True)
    assert np.array_equal(got.cpu().numpy(), np.minimum(img8[:, :, :-1], img8[:, :, 1:]))
    # no positive weight: every tap dropped by `zero`, masked without extrapolation, and a lone negative dst2 tap
    seg = T(np.full(shape, 9)).to(torch.int32)
    far = torch.tensor([[-3.0, 2.0, 2.0], [3.0, 9.5, 2.0], [3.0, 2.0, -7.25]], device=DEV).reshape(3, 1, 1, 3)
    for order in (0, 1, 2, 3):
        assert IP.grid_pull(seg, far, order, "zero", True).flatten().tolist() == [0, 0, 0]
        assert IP.grid_pull(seg, far, order, "dct2", False).flatten().tolist() == [0, 0, 0]
        assert IP.grid_pull(seg, far, order, "dct2", True).flatten().tolist() == [9, 9, 9]
    assert IP.grid_pull(seg, torch.tensor([[-1.0, 2.0, 2.0]], device=DEV).reshape(1, 1, 1, 3), 0, "dst2",
                        True).flatten().tolist() == [0]


# ------------------------------------------------------------------------------------- 3. a footprint of distinct labels
def test_sixty_four_distinct_labels_and_a_constant_image():
    """arange as the image: no two taps of a cubic footprint share a label, the thread's table is full.  The ways of keeping
    the table give the same bits.  A constant image comes back constant wherever anything is in view."""
    from brainfm_amd import interpol as IP
    rng = np.random.default_rng(5)
    shape = (6, 5, 7)
    img = (np.arange(int(np.prod(shape))).reshape((1, 1) + shape) * 331 - 30000).astype(np.int64)
    grid = (rng.random((1, 9, 8, 7, 3)) * (np.array(shape) - 1.0)).astype(np.float32)
    for order in (3, 2, 1, [3, 3, 2]):
        o = IP._order_list(order)
        win, gap = LR.label_pull(img, grid, order, 3, 1)
        for dt in (torch.int32, torch.int64):
            seg, tg = T(img).to(dt), T(grid)
            b = IP._opts(order, "dct2", True)[0]
            outs = [IP._label_pull_raw(seg, tg, b, o, 1, v) for v in (IP.LABEL_PULL_AUTO, IP.LABEL_PULL_LDS,
                                                                        IP.LABEL_PULL_REGS, IP.LABEL_PULL_PASSES)]
            assert all(torch.equal(outs[0], other) for other in outs[1:]), (order, dt)
            assert torch.equal(outs[0], IP.grid_pull(seg, tg, order, "dct2", True))
            held(outs[0].long(), win, gap, "arange order %s" % (order,))
    spill = (rng.random((1, 9, 8, 7, 3)) * (np.array(shape) + 4.0) - 2.5).astype(np.float32)
    for dt, val in ((torch.uint8, 255), (torch.int16, -32768), (torch.int32, 70000), (torch.int64, -(2 ** 40))):
        const = torch.full((1, 1) + shape, val, dtype=dt, device=DEV)
        for order in (0, 1, 2, 3):
            for bound in ("dct2", "dft", "replicate"):
                assert bool((IP.grid_pull(const, T(spill), order, bound, True) == val).all()), (dt, order, bound)


_BIG = {}


def big():
    """33 x 17 x 40 image of about 40 blocky labels, 40 x 9 x 33 grid: 11 880 voxels, 47 blocks of 256 or 186 of 64, the
    last one ragged; the coordinates spill 2.5 voxels over every face"""
    if not _BIG:
        rng = np.random.default_rng(7)
        ins, outs = (33, 17, 40), (40, 9, 33)
        _BIG.update(img=LR.blocky_labels(ins, 40, 1, block=3)[None, None] + 1,
                    grid=(rng.random((1,) + outs + (3,)) * (np.array(ins) + 4.0) - 2.5).astype(np.float32))
    return _BIG


@pytest.mark.parametrize("bound", ["zero", "dct2", "dst2"])
def test_several_blocks_and_a_ragged_tail_against_the_restatement(bound):
    from brainfm_amd import interpol as IP
    b = big()
    for order in (0, 1, 2, 3, [1, 3, 0]):
        win, gap = LR.label_pull(b["img"], b["grid"], order, IP._BOUND[bound], 1)
        got = IP.grid_pull(T(b["img"]), T(b["grid"]), order, bound, True)
        held(got, win, gap, "big order %s %s" % (order, bound))


# ------------------------------------------------------------------------------------ 4. independence of the label count
@pytest.mark.parametrize("bound", ["zero", "dct2", "dst2"])
def test_monotone_relabelling_commutes_with_the_pull(bound):
    """The labels 1 .. 40 against the same image under a monotone map onto a sparse set of large values (negative ones
    too): the second result is the first mapped, bit for bit -- a monotone map keeps the order of a tie, and 0 ("no
    label has a positive weight") stays 0, which is why the first image has no label 0."""
    from brainfm_amd import interpol as IP
    b = big()
    img = b["img"].astype(np.int64)
    assert img.min() == 1
    table = np.concatenate([[0], np.sort(np.random.default_rng(8).choice(np.arange(-2 ** 33, 2 ** 33, 1001), img.max(),
                                                                          replace=False))])
    table[1:][table[1:] == 0] = 1
    tt, tg = T(table), T(b["grid"])
    for order in (0, 1, 2, 3, [2, 1, 3]):
        first = IP.grid_pull(T(img), tg, order, bound, True)
        second = IP.grid_pull(tt[T(img)], tg, order, bound, True)
        assert second.dtype == torch.int64 and torch.equal(second, tt[first]), (order, bound)
        assert torch.equal(first, IP.grid_pull(T(img), tg, order, bound, True))      # and the same bits run to run


# ------------------------------------------------------------------------------------------------------ 5. grid builders
@pytest.mark.parametrize("dn,dt", [("f32", torch.float32), ("f64", torch.float64)])
def test_grid_builders_equal_the_reference_bit_for_bit(dn, dt):
    from brainfm_amd import interpol as IP
    d = golden()
    shape = (5, 6, 7)
    ident = IP.identity_grid(shape, dtype=dt, device=DEV)
    assert ident.dtype == dt and np.array_equal(ident.cpu().numpy(), d["builders/identity_" + dn])
    for bn, bs in (("b", ()), ("b2", (2,)), ("b23", (2, 3))):
        disp = T(d["builders/disp_%s_%s" % (bn, dn)])
        keep = disp.clone()
        out = IP.add_identity_grid(disp)
        assert torch.equal(disp, keep) and out.data_ptr() != disp.data_ptr()
        assert out.dtype == dt and np.array_equal(out.cpu().numpy(), d["builders/add_%s_%s" % (bn, dn)])
        same = IP.add_identity_grid_(disp)
        assert same is disp and torch.equal(disp, out)
        # a field that is not contiguous is still changed in place
        perm = keep.movedim(-2, -4).contiguous().movedim(-4, -2)
        assert not perm.is_contiguous() or perm.numel() == 0
        assert IP.add_identity_grid_(perm) is perm and torch.equal(perm, out)
        for rows in (3, 4):
            k = "builders/affine%d_%s_%s" % (rows, bn, dn)
            got = IP.affine_grid(T(d[k + "_mat"]), shape)
            assert got.dtype == dt and tuple(got.shape) == bs + shape + (3,)
            assert np.array_equal(got.cpu().numpy(), d[k]), k
    eye = torch.eye(4, dtype=dt, device=DEV)
    assert torch.equal(IP.affine_grid(eye, shape), ident) and torch.equal(IP.affine_grid(eye[:3], shape), ident)


def test_identity_displacement_returns_the_segmentation_and_low_dimensions():
    from brainfm_amd import interpol as IP
    d = golden()
    seg = T(d["S/img"])
    zeros = torch.zeros((2,) + tuple(seg.shape[2:]) + (3,), device=DEV)
    for order in (0, 1):
        assert torch.equal(IP.grid_pull(seg, IP.add_identity_grid(zeros), order, "dct2", True), seg)
    assert IP.identity_grid((4, 5, 6), device=DEV).dtype == torch.get_default_dtype()
    # 1-D and 2-D: torch on the device, the reference's values
    g2 = IP.identity_grid((3, 4), dtype=torch.float32, device=DEV)
    assert tuple(g2.shape) == (3, 4, 2) and g2[2, 3].tolist() == [2.0, 3.0] and g2[1, 0].tolist() == [1.0, 0.0]
    assert IP.identity_grid((5,), dtype=torch.float64, device=DEV).flatten().tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert torch.equal(IP.add_identity_grid(torch.zeros(2, 3, 4, 2, device=DEV)), g2.expand(2, 3, 4, 2))
    m = torch.tensor([[2.0, 0.0, 1.0], [0.0, 3.0, -1.0]], device=DEV)
    a2 = IP.affine_grid(m, (3, 4))
    assert a2[2, 3].tolist() == [5.0, 8.0]


# ------------------------------------------------------------------------------------------------------- 6. spline_coeff
def close(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)
    return err


def test_spline_coeff_against_the_reference_and_against_spline_coeff_nd():
    from brainfm_amd import interpol as IP
    d = golden()
    worst = 0.0
    for tn in ("t3", "t4"):
        x = T(d["coeff/" + tn])
        for order in (2, 3):
            for bound in ("dct1", "dct2", "dft"):
                for dim in (-1, 0, 1):
                    k = "coeff/%s/o%d_%s_d%d" % (tn, order, bound, dim)
                    got = IP.spline_coeff(x, order, bound, dim)
                    assert got.dtype == torch.float32 and got.data_ptr() != x.data_ptr()
                    worst = max(worst, close(got, d[k].astype(np.float64), k))
                    assert torch.equal(got, IP.spline_coeff(x, ["quadratic", "cubic"][order - 2], bound, dim % x.dim()))
    print("spline_coeff: worst max|hip - ref| %.2e" % worst)
    x = T(d["coeff/t3"])
    assert torch.equal(x, T(d["coeff/t3"]))                                    # never touched without inplace
    for order in (2, 3):
        for bound in ("dct1", "dct2", "dft", "zero", "nearest"):
            step = x
            for dim in (0, 1, 2):
                step = IP.spline_coeff(step, order, bound, dim)
            nd = IP.spline_coeff_nd(x, order, bound, 3)
            close(step, nd.cpu().numpy().astype(np.float64), "axis by axis vs nd o%d %s" % (order, bound))
    # a leading batch dimension of the 4-D tensor: dims 1, 2, 3 in turn are spline_coeff_nd over the last three
    x4 = T(d["coeff/t4"])
    step = x4
    for dim in (1, 2, 3):
        step = IP.spline_coeff(step, 3, "dct2", dim)
    close(step, IP.spline_coeff_nd(x4, 3, "dct2", 3).cpu().numpy().astype(np.float64), "4-D vs nd")


def test_spline_coeff_low_orders_inplace_and_gradient():
    from brainfm_amd import interpol as IP
    x = torch.randn(5, 6, 7, device=DEV)
    for order in (0, 1, "nearest", "linear"):
        y = IP.spline_coeff(x, order, "dct2", 1)
        assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()
        assert IP.spline_coeff(x, order, "dct2", 1, inplace=True) is x
    ref = IP.spline_coeff(x, 3, "dct2", 1)
    assert not torch.equal(ref, x)
    work = x.clone()
    assert IP.spline_coeff(work, 3, "dct2", 1, inplace=True) is work and torch.equal(work, ref)
    view = x.clone().movedim(0, 2)                                             # not contiguous: still changed in place
    want = IP.spline_coeff(view.contiguous(), 2, "dft", 0)
    assert IP.spline_coeff(view, 2, "dft", 0, inplace=True) is view and torch.equal(view, want)
    x64 = x.double()
    y64 = IP.spline_coeff(x64, 3, "dct1", -1)
    assert y64.dtype == torch.float64 and torch.equal(y64.float(), IP.spline_coeff(x, 3, "dct1", -1))
    one = torch.randn(4, 1, device=DEV)
    assert torch.equal(IP.spline_coeff(one, 3, "dct2", 1), one)                # an axis of length 1 is left alone
    # backward = the same filter on the gradient (the filter is symmetric)
    xr = x.clone().requires_grad_(True)
    w = torch.cos(torch.arange(x.numel(), dtype=torch.float32, device=DEV)).reshape(x.shape)
    IP.spline_coeff(xr, 3, "dct2", 0).backward(w)
    assert torch.equal(xr.grad, IP.spline_coeff(w, 3, "dct2", 0)) and not torch.equal(xr.grad, w)
    xr = x.clone().requires_grad_(True)
    IP.spline_coeff(xr, 2, "dct1", 2).backward(w)                             # the reference's backward under DCT-I too
    assert torch.equal(xr.grad, IP.spline_coeff(w, 2, "dct1", 2))
    # gradcheck in float64 on a length-7 axis.  The arithmetic is float32 and the map is linear: a central difference has
    # no truncation error at any step, so the step is 1e-2 and what is left is the float32 rounding of values of a few
    # units, ~5e-7, over 2e-2: 2.5e-5 per entry of the Jacobian, held to 2e-4.  Under the DCT-II and DFT conditions, where
    # the filter matrix is symmetric and the reference's backward (the filter itself, autograd.py:267-273) is the true
    # gradient.  Under DCT-I ('zero' / 'dct1') the matrix is not symmetric in its first and last rows (the mirrored
    # neighbour of an end sample counts twice), so there the backward mirrored from the reference is not the transpose
    # and gradcheck cannot pass (measured: entries -0.243 against -0.485); spline_coeff_nd has had the same backward
    for order, bound, shape, dim in ((3, "dct2", (3, 7), -1), (2, "dct2", (7, 2), 0), (3, "dft", (2, 7, 2), 1),
                                     (2, "dft", (7,), 0)):
        xd = torch.randn(shape, dtype=torch.float64, device=DEV, requires_grad=True)
        assert torch.autograd.gradcheck(lambda t: IP.spline_coeff(t, order, bound, dim), (xd,), eps=1e-2, atol=2e-4,
                                        rtol=0.0)


# --------------------------------------------------------------------------------------------------- 7. resize of labels
def test_resize_of_a_label_map_at_orders_below_two_is_the_label_pull_on_the_resize_grid():
    """resize defaults to prefilter=True, which a label map refuses; below order 2 there is nothing to filter, so the default
    call pulls the labels through the grid that resize builds (anchor 'c': linspace(0, n - 1, m) per axis), under
    'nearest' with extrapolation.  Order 2 keeps the refusal."""
    from brainfm_amd import interpol as IP
    seg = T(golden()["S/img"])
    shape = [2 * n - 1 for n in seg.shape[2:]]
    grid = torch.stack(torch.meshgrid(*[torch.linspace(0, n - 1, m, dtype=torch.float32, device=DEV)
                                        for n, m in zip(seg.shape[2:], shape)], indexing="ij"), dim=-1)
    for order in (1, "linear", 0):
        got = IP.resize(seg, shape=shape, interpolation=order)
        assert got.dtype == seg.dtype and tuple(got.shape[2:]) == tuple(shape)
        assert torch.equal(got, IP.grid_pull(seg, grid, order, "nearest", True))
    assert torch.equal(IP.resize(seg, shape=shape)[..., ::2, ::2, ::2], seg)          # the nodes themselves come back
    with pytest.raises(NotImplementedError, match="prefilter"):
        IP.resize(seg, shape=shape, interpolation=2)
