"""Kernel-level tests of conv_wino_b5 (conv3d_wino_b5.hip): F(2,3) along x on boxes of 5 x 5 x 10 output voxels with a split
K loop, through the C ABI (bfm_conv3x3x3_wino_b5_batch) -- against float64, every sample against its own S = 1 launch and
the reversed batch bit for bit, accumulate mode on padded affine rows, the moment rows, the refused arguments.
Needs an MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

G, SLOPE = 8, 0.01
# one box; two boxes along z and y; two along x; (2, 1, 2): halos from a neighbouring box, from the padding, from both
SHAPES = [(5, 5, 10), (10, 10, 10), (5, 5, 20), (10, 5, 20)]
# cin 16: one K chunk; 48: an odd number of chunks (the weight ring's parity), one chunk per slab; cout 128: two column tiles
CHANNELS = [(16, 64), (48, 128), (16, 128), (48, 64)]
# slabs of several chunks, as the layers of the network run them: 256 -> 4 slabs of 4 chunks, 272 -> 4 of 4 and one of 1
DEEP = [((10, 10, 10), 256, 64), ((5, 5, 10), 272, 64)]
CASES = [(s, ci, co) for s in SHAPES for ci, co in CHANNELS] + DEEP


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _group_bound(Y, groups):
    s, c = Y.shape[0], Y.shape[-1]
    return Y.abs().reshape(s, -1, groups, c // groups).amax((1, 3)).float().contiguous()


def _pack(w):
    """conv_wino's pack of w (Cout, Cin, 3, 3, 3) on the device -> (buffer, wexp): the kernel reads it as it is."""
    L, lib = _lib()
    cout, cin = w.shape[:2]
    wp = torch.empty(lib.bfm_pack_conv_weights_wino_bytes(cin, cout, 3), dtype=torch.uint8, device=w.device)
    wexp = C.c_int(0)
    L.check(lib.bfm_pack_conv_weights_wino(L.ptr(w), cin, cout, float(w.abs().max()), 3, L.ptr(wp), C.byref(wexp),
                                           L.stream_ptr()), "pack_wino")
    return wp, wexp.value


def _call(A, cin, ss, dims, sc, sh, bd, wp, wexp, cout, out, rows=None, flags=0, aff=0, passes=3, ws=None, ws_bytes=None):
    """The raw call; the workspace is NaN-filled so that a slab entry nobody wrote would show in the sum."""
    L, lib = _lib()
    if ws is None:
        nb = lib.bfm_conv3x3x3_wino_b5_workspace(cin, cout, ss, *dims)
        ws = torch.full((max(nb, 16) // 4,), float("nan"), device=out.device)
        ws_bytes = nb
    return lib.bfm_conv3x3x3_wino_b5_batch(L.ptr(A), cin, ss, dims[0], dims[1], dims[2], L.ptr(sc), L.ptr(sh), L.ptr(bd), G,
                                           L.ptr(wp), wexp, cout, SLOPE, passes, flags, L.ptr(out),
                                           L.ptr(rows) if rows is not None else None, aff, L.ptr(ws), ws_bytes,
                                           L.stream_ptr())


def _run(*a, **k):
    L, _ = _lib()
    L.check(_call(*a, **k), "conv_wino_b5_batch")
    torch.cuda.synchronize()


_CASE = {}


def _case(dims, cin, cout, S=3):
    """Inputs of one (shape, channels) case and its float64 reference (before accumulate and LeakyReLU), made once and left
    unchanged: S samples of different statistics, one of them all zero; affine tables at a pitch of cin + 32."""
    key = (dims, cin, cout, S)
    if key not in _CASE:
        dev = _dev()
        g = torch.Generator().manual_seed(cin + 7 * cout + dims[0] + 3 * dims[2])
        X = torch.randn((S,) + dims + (cin,), generator=g)
        X[1] = X[1] * 3 + 0.5
        X[2] = 0
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05
        pitch = cin + 32
        aff = torch.zeros(2, S, pitch)
        aff[0, :, :cin] = torch.rand(S, cin, generator=g) + 0.5
        aff[1, :, :cin] = torch.randn(S, cin, generator=g) * 0.2
        aff[:, :, cin:] = float("nan")                              # columns of another layer: never read
        Y = X * aff[0, :, None, None, None, :cin] + aff[1, :, None, None, None, :cin]
        bound = _group_bound(Y, G).to(dev)
        conv = F.conv3d(Y.double().permute(0, 4, 1, 2, 3), w.double(), padding=1).permute(0, 2, 3, 4, 1).contiguous()
        prior = torch.randn((S,) + dims + (cout,), generator=g)
        w = w.to(dev).contiguous()
        wp, wexp = _pack(w)
        aff = aff.to(dev)
        _CASE[key] = dict(X=X.to(dev), aff=aff, sc=aff[0, :, :cin].contiguous(), sh=aff[1, :, :cin].contiguous(), bound=bound,
                          conv=conv, prior=prior, wp=wp, wexp=wexp, pitch=pitch)
    return _CASE[key]


def _lrelu64(y):
    return torch.where(y >= 0, y, y * SLOPE)


def _rows_views(rows, n, cout):
    k = n * cout
    return (rows[:k * 8].view(torch.float64).view(n, cout), rows[k * 8:k * 16].view(torch.float64).view(n, cout),
            rows[k * 16:k * 20].view(torch.float32).view(n, cout), rows[k * 20:k * 24].view(torch.float32).view(n, cout))


def _boxes(t, dims):
    """(D,H,W,C) -> [boxes][250][C] in the kernel's box order (z, then y, then x)."""
    D, H, W = dims
    c = t.shape[-1]
    return t.reshape(D // 5, 5, H // 5, 5, W // 10, 10, c).permute(0, 2, 4, 1, 3, 5, 6).reshape(-1, 250, c)


@pytest.mark.parametrize("dims,cin,cout", CASES)
def test_b5_vs_float64_rows_and_two_runs_bitwise(dims, cin, cout):
    """One sample against the float64 convolution of the affine'd, zero-padded input, within 1e-5 of max |y| -- the bound
    test_winograd_f43_kernel_vs_float64_convolution holds F(4,3) to (F(2,3) rounds about half as much).  Output
    NaN-prefilled: an unwritten voxel shows.  A second run gives the same bits (the slabs are summed in a fixed order).
    The moment rows: one per box, equal to sum / sum of squares / min / max of the box's 250 stored voxels -- min and max
    bit for bit, the sums within 16 * 2^-24 of the sum of magnitudes (a thread adds at most 16 values in fp32, the rest
    is fp64) -- so the three padding rows of the 128 reach neither."""
    L, lib = _lib()
    dev = _dev()
    c = _case(dims, cin, cout)
    n = lib.bfm_conv3x3x3_wino_b5_rows(dims[0], dims[1], dims[2], 3)
    assert n == (dims[0] // 5) * (dims[1] // 5) * (dims[2] // 10)
    sk = lib.bfm_conv3x3x3_wino_b5_splitk(cin, cout, *dims)
    assert sk >= 1
    for s_ in (0, 1):
        out = torch.full(dims + (cout,), float("nan"), device=dev)
        rows = torch.zeros(lib.bfm_moment_rows_bytes(n, cout), dtype=torch.uint8, device=dev)
        _run(c["X"][s_], cin, 1, dims, c["sc"][s_], c["sh"][s_], c["bound"][s_], c["wp"], c["wexp"], cout, out, rows)
        assert bool(torch.isfinite(out).all()), "an output voxel was not written"
        want = _lrelu64(c["conv"][s_])
        err = float((out.double().cpu() - want).abs().max() / want.abs().max())
        print("wino_b5 %s %d->%d sample %d, %d slabs: float64 error %.2e" % (dims, cin, cout, s_, sk, err))
        assert err <= 1e-5, err
        again = torch.full_like(out, float("nan"))
        _run(c["X"][s_], cin, 1, dims, c["sc"][s_], c["sh"][s_], c["bound"][s_], c["wp"], c["wexp"], cout, again)
        assert torch.equal(out, again)
        rs, rq, rmn, rmx = (t.cpu() for t in _rows_views(rows, n, cout))
        ob = _boxes(out.cpu(), dims)
        o64 = ob.double()
        assert torch.equal(rmn, ob.min(1)[0]) and torch.equal(rmx, ob.max(1)[0])
        u = 16 * 2.0 ** -24
        assert bool(((rs - o64.sum(1)).abs() <= u * o64.abs().sum(1) + 1e-300).all())
        assert bool(((rq - (o64 * o64).sum(1)).abs() <= u * (o64 * o64).sum(1) + 1e-300).all())


def test_b5_planner_splits_these_shapes_and_never_by_batch_size():
    """The split factors the planner returns over the cases above: no split (one chunk), one chunk per slab, slabs of
    four chunks with and without a short last one -- all of them run by the test above.  The factor is a function of the
    layer shape; the workspace is S times one sample's."""
    _, lib = _lib()
    got = {(ci, co, d): lib.bfm_conv3x3x3_wino_b5_splitk(ci, co, *d) for d, ci, co in CASES}
    assert all(v == 1 for (ci, _, _), v in got.items() if ci == 16)
    assert all(v == 3 for (ci, _, _), v in got.items() if ci == 48)
    assert got[(256, 64, (10, 10, 10))] == 4 and got[(272, 64, (5, 5, 10))] == 5
    one = lib.bfm_conv3x3x3_wino_b5_workspace(48, 128, 1, 10, 5, 20)
    assert one == 3 * 1000 * 128 * 4 and lib.bfm_conv3x3x3_wino_b5_workspace(48, 128, 7, 10, 5, 20) == 7 * one
    # the 512 -> 512 layer of the 10^3 level: 32 chunks in 8 slabs of 4
    assert lib.bfm_conv3x3x3_wino_b5_splitk(512, 512, 10, 10, 10) == 8
    assert lib.bfm_conv3x3x3_wino_b5_splitk(512, 512, 10, 10, 15) == 0


@pytest.mark.parametrize("dims,cin,cout", [((10, 10, 10), 48, 128), ((10, 5, 20), 16, 64), ((10, 10, 10), 256, 64)])
def test_b5_batch_equals_each_sample_alone_and_the_reversed_batch_bitwise(dims, cin, cout):
    """S = 3 samples of different statistics, one all zero, in one launch: every sample's output and moment rows are the
    bits of its own S = 1 launch and of the launch with the batch reversed."""
    _, lib = _lib()
    dev = _dev()
    c = _case(dims, cin, cout)
    S = 3
    n = lib.bfm_conv3x3x3_wino_b5_rows(dims[0], dims[1], dims[2], 3)
    rb = lib.bfm_moment_rows_bytes(S * n, cout)
    out = torch.full((S,) + dims + (cout,), float("nan"), device=dev)
    rows = torch.zeros(rb, dtype=torch.uint8, device=dev)
    _run(c["X"], cin, S, dims, c["sc"], c["sh"], c["bound"], c["wp"], c["wexp"], cout, out, rows)
    assert bool(torch.isfinite(out).all())
    views = _rows_views(rows, S * n, cout)
    for s_ in range(S):
        one = torch.full(dims + (cout,), float("nan"), device=dev)
        r1 = torch.zeros(lib.bfm_moment_rows_bytes(n, cout), dtype=torch.uint8, device=dev)
        _run(c["X"][s_], cin, 1, dims, c["sc"][s_], c["sh"][s_], c["bound"][s_], c["wp"], c["wexp"], cout, one, r1)
        assert torch.equal(out[s_], one), s_
        for a, b in zip(views, _rows_views(r1, n, cout)):
            assert torch.equal(a[s_ * n:(s_ + 1) * n], b), s_
    rev = torch.full_like(out, float("nan"))
    rr = torch.zeros_like(rows)
    _run(c["X"].flip(0).contiguous(), cin, S, dims, c["sc"].flip(0).contiguous(), c["sh"].flip(0).contiguous(),
         c["bound"].flip(0).contiguous(), c["wp"], c["wexp"], cout, rev, rr)
    assert torch.equal(out, rev.flip(0))
    for a, b in zip(views, _rows_views(rr, S * n, cout)):
        assert torch.equal(a.view(S, n, cout), b.view(S, n, cout).flip(0))


@pytest.mark.parametrize("dims,cin,cout", [((10, 5, 20), 48, 128), ((10, 10, 10), 256, 64)])
def test_b5_accumulates_onto_a_prior_tensor_with_padded_affine_rows_bitwise(dims, cin, cout):
    """Accumulate mode (the skip half of a decoder's first conv) with the affine rows as column windows of a wider table
    (pitch cin + 32, the other columns NaN): LeakyReLU(prior + conv) within 1e-5 of float64, and the batch bit-identical
    to one accumulating launch per sample on that sample's row of the table."""
    dev = _dev()
    c = _case(dims, cin, cout)
    S = 3
    sc, sh = c["aff"][0], c["aff"][1]                               # [S][pitch] views: rows `pitch` apart
    out = c["prior"].to(dev).clone()
    _run(c["X"], cin, S, dims, sc, sh, c["bound"], c["wp"], c["wexp"], cout, out, None, 1, c["pitch"])
    want = _lrelu64(c["conv"] + c["prior"].double())
    err = float((out.double().cpu() - want).abs().max() / want.abs().max())
    print("wino_b5 accumulate %s %d->%d: float64 error %.2e" % (dims, cin, cout, err))
    assert err <= 1e-5, err
    for s_ in range(S):
        one = c["prior"][s_].to(dev).clone()
        _run(c["X"][s_], cin, 1, dims, sc[s_], sh[s_], c["bound"][s_], c["wp"], c["wexp"], cout, one, None, 1, c["pitch"])
        assert torch.equal(out[s_], one), s_


def test_b5_refuses_bad_arguments_before_any_launch():
    """Volumes the box does not divide, channel counts off the chunk / column tile, a misaligned pointer, passes = 2, a
    short workspace: the documented codes, and `out` keeps its NaN prefill (nothing was launched)."""
    L, lib = _lib()
    dev = _dev()
    dims, cin, cout = (5, 5, 10), 16, 64
    c = _case(dims, cin, cout)
    out = torch.full((6, 5, 20, 128), float("nan"), device=dev)     # large enough for every shape tried below
    X = torch.zeros(6 * 5 * 20 * 16 + 4, device=dev)
    a = (c["sc"][0], c["sh"][0], c["bound"][0], c["wp"], c["wexp"])
    ws = torch.full((1 << 16,), float("nan"), device=dev)

    def rc(dims=dims, cin=cin, cout=cout, A=X, passes=3, flags=0, ws_bytes=ws.numel() * 4, aff=0):
        return _call(A, cin, 1, dims, *a, cout, out, None, flags, aff, passes, ws, ws_bytes)
    E_ARG, E_SHAPE, E_WS = (k for k, v in sorted(L.ERR.items(), reverse=True) if v in ("BFM_E_ARG", "BFM_E_SHAPE", "BFM_E_WORKSPACE"))
    assert rc(dims=(6, 5, 10)) == E_SHAPE
    assert rc(dims=(5, 4, 10)) == E_SHAPE
    assert rc(dims=(5, 5, 15)) == E_SHAPE
    assert rc(cin=8) == E_SHAPE
    assert rc(cout=32) == E_SHAPE
    assert rc(A=X[1:]) == E_ARG                                     # 4 bytes off a 16-byte boundary
    assert rc(passes=2) == E_ARG
    assert rc(flags=2) == E_ARG
    assert rc(aff=cin - 4) == E_ARG
    assert rc(ws_bytes=5 * 5 * 10 * 64 * 4 - 4) == E_WS
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.reshape(-1)[:5 * 5 * 10 * 64]).all())
