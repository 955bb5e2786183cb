"""interpol.grid_hess / grid_pushgrad and the backward of grid_grad on the device (brainfm_amd/csrc/grid_hess.hip) against
the reference's own results (tests/golden/interpol_grid_hess_*.npz, float64 runs of the vendored torch-interpol rounded to
float32) and against the float64 restatement (tests/grid_hess_refs.py) where the reference has no result: a mask with more
than one batch or channel, broadcast batches, a launch that takes the grid-stride loop.

The bar is the family's own (test_gpu_spline_grid.py): max|hip - ref| <= 2e-5 * max(1, max|ref|), the stored
max|ref32 - ref64| of the reference printed beside the measured distance.  pushgrad adds with fp32 atomics, so its last
bit is not reproducible; the bar covers that."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_npz
import grid_hess_refs as HR
import spline_grid_refs as SR
from test_gpu_spline_grid import DEV, Log, T, base

pytestmark = pytest.mark.gpu

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
_FIX = {}


def fixture(otag):
    if otag not in _FIX:
        _FIX[otag] = load_npz("interpol_grid_hess_%s.npz" % otag)
    return _FIX[otag]


def sin_w(y):
    return torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(y.device)


def three(v):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * 3)[:3]


@pytest.mark.parametrize("otag", list(ORDERS))
def test_every_array_of_the_fixture(otag):
    """hess and pushgrad for the seven bounds, d/dinput and d/dgrid of sum(grid_grad * sin(arange)) through backward()
    under 'zero' and 'dct2', d/dinput with prefilter=True at orders 2 and 3: both shapes, and the B = C = 1 mask cases."""
    from brainfm_amd import interpol as IP
    d = fixture(otag)
    order = ORDERS[otag]
    log = Log()
    seen = set()
    for tag in ("A", "T"):
        vol, grid, cot = T(base()[tag + "/vol"]), T(base()[tag + "/grid"]), T(d["cot/" + tag])
        ins = list(vol.shape[2:])
        for combo in sorted({k.split("/")[1] for k in d if k.startswith(tag + "/")}):
            bound, ext = int(combo[1]), int(combo[4])
            k = "%s/%s/" % (tag, combo)

            def chk(got, name):
                log.close(got, d[k + name], k + name, name, d[k + name + ".err"])
                seen.add(k + name)

            if k + "hess" in d:
                chk(IP.grid_hess(vol, grid, order, bound, ext), "hess")
            chk(IP.grid_pushgrad(cot, grid, ins, order, bound, ext), "pushgrad")
            if k + "grad_dinput" not in d:
                continue
            v, gr = vol.clone().requires_grad_(True), grid.clone().requires_grad_(k + "grad_dgrid" in d)
            y = IP.grid_grad(v, gr, order, bound, ext)
            w = sin_w(y)
            (y * w).sum().backward()
            chk(v.grad, "grad_dinput")
            if k + "grad_dgrid" in d:
                chk(gr.grad, "grad_dgrid")
            if k + "grad_pf_dinput" in d:
                v = vol.clone().requires_grad_(True)
                (IP.grid_grad(v, grid, order, bound, ext, prefilter=True) * w).sum().backward()
                chk(v.grad, "grad_pf_dinput")
    v11, inner = T(base()["A/vol"][:1, :1]), T(d["inner/grid"])
    for bound in range(7):
        for ext in (0, 2):
            k = "inner/b%d_e%d/hess" % (bound, ext)
            log.close(IP.grid_hess(v11, inner, order, bound, ext), d[k], k, "hess B=C=1 mask", d[k + ".err"])
            seen.add(k)
    stored = {k for k in d if not k.endswith(".err") and not k.startswith("cot/") and k != "inner/grid"}
    assert seen == stored, sorted(stored - seen)[:5]
    assert ("grad_pf_dinput" in log.worst) == (otag in ("o2", "o3"))
    log.show(otag)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_contracted_kernel_against_the_materialised_hessian(otag):
    """out[b,v,j] = sum_c sum_i H[b,c,v,i,j] cot[b,c,v,i], the reference's (grid_hess * grad.unsqueeze(-1)).sum((1, -2));
    the materialised Hessian is symmetric to the bit."""
    from brainfm_amd import interpol as IP
    vol, grid, cot = T(base()["A/vol"]), T(base()["A/grid"]), T(fixture(otag)["cot/A"])
    log = Log()
    for bound, ext in ((0, 1), (3, 1), (4, 0), (6, 2)):
        b, o, e = IP._opts(ORDERS[otag], bound, ext)
        h = IP.grid_hess(vol, grid, ORDERS[otag], bound, ext)
        assert tuple(h.shape) == (2, 3, 5, 9, 6, 3, 3) and torch.equal(h, h.transpose(-1, -2))
        want = (h.double() * cot.double().unsqueeze(-1)).sum((1, -2)).cpu().numpy()
        got = IP._hess_raw(vol, grid, b, o, e, cot=cot)
        assert tuple(got.shape) == (2, 5, 9, 6, 3)
        log.close(got, want, "contracted b%d e%d" % (bound, ext), "contracted")
    log.show(otag)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_mask_with_several_batches_and_channels(otag):
    """extrapolate 0 and 2 on the inner grid with B = 2, C = 3, where the reference raises: the Hessian times the mask,
    against the restatement; voxels outside the mask are exact zeros, in the contraction too."""
    from brainfm_amd import interpol as IP
    d = fixture(otag)
    vol = base()["A/vol"]
    inner = np.concatenate([d["inner/grid"], d["inner/grid"][:, ::-1, :, ::-1]], 0).copy()
    cot = d["cot/A"]
    log = Log()
    for bound in (0, 3, 5):
        for ext in (0, 2):
            ref = HR.hess(vol, inner, ORDERS[otag], bound, ext)
            got = IP.grid_hess(T(vol), T(inner), ORDERS[otag], bound, ext)
            log.close(got, ref, "hess b%d e%d" % (bound, ext), "hess B=2 C=3 mask")
            out = SR._mask(inner.astype(np.float64).reshape(2, -1, 3), vol.shape[2:], ext) == 0
            out = np.broadcast_to(out.reshape(2, 1, 5, 9, 6, 1, 1), ref.shape)
            assert out.any() and not out.all() and (ext == 2 or 0.1 < out.mean() < 0.6)
            assert not got.cpu().numpy()[out].any()
            b, o, e = IP._opts(ORDERS[otag], bound, ext)
            gc = IP._hess_raw(T(vol), T(inner), b, o, e, cot=T(cot))
            log.close(gc, HR.contract(ref, cot), "contracted b%d e%d" % (bound, ext), "contracted mask")
            assert not gc.cpu().numpy()[out[:, 0, ..., 0]].any()
    log.show(otag)


@pytest.mark.parametrize("bound", [0, 3, 5])
@pytest.mark.parametrize("otag", ["o1", "o3", "o312"])
def test_pushgrad_is_the_adjoint_of_grad_on_the_device(otag, bound):
    """<pushgrad(c), v> = <c, grid_grad(v)>, both sums on the host in float64, 1e-5 relative"""
    from brainfm_amd import interpol as IP
    vol, grid, cot = T(base()["A/vol"]), T(base()["A/grid"]), T(fixture(otag)["cot/A"])
    p = IP.grid_pushgrad(cot, grid, list(vol.shape[2:]), ORDERS[otag], bound, 1)
    g = IP.grid_grad(vol, grid, ORDERS[otag], bound, 1)
    lhs = float((p.cpu().double() * vol.cpu().double()).sum())
    rhs = float((cot.cpu().double() * g.cpu().double()).sum())
    print("%s bound %d: <pushgrad(c), v> %.9g  <c, grad(v)> %.9g" % (otag, bound, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("otag", ["o1", "o3", "o312"])
def test_grid_grad_keeps_its_bits(otag):
    from brainfm_amd import interpol as IP
    vol, grid = T(base()["A/vol"]), T(base()["A/grid"])
    for bound, ext in ((0, 0), (3, 1)):
        plain = IP.grid_grad(vol, grid, ORDERS[otag], bound, ext)
        assert plain.grad_fn is None and not plain.requires_grad
        y = IP.grid_grad(vol.clone().requires_grad_(True), grid.clone().requires_grad_(True), ORDERS[otag], bound, ext)
        assert y.grad_fn is not None and torch.equal(y.detach(), plain)
        with torch.no_grad():
            z = IP.grid_grad(vol.clone().requires_grad_(True), grid, ORDERS[otag], bound, ext)
        assert z.grad_fn is None and torch.equal(z, plain)
        with pytest.raises(RuntimeError):                    # no double backward, as in the reference
            v = vol.clone().requires_grad_(True)
            (gi,) = torch.autograd.grad(IP.grid_grad(v, grid, ORDERS[otag], bound, ext).sum(), v, create_graph=True)
            gi.sum().backward()


@pytest.mark.parametrize("otag", ["o1", "o2", "o312"])
def test_batch_broadcast_at_the_exports_and_through_backward(otag):
    """One image under two grids and the reverse at the C exports; a channel-less (X, Y, Z) input and a grid shared by a
    batch of two through grid_grad(...).backward(): the grid's gradient is then the sum over the batch."""
    from brainfm_amd import interpol as IP
    from brainfm_amd import _lib as L
    lib = L.load()
    b = base()
    d = fixture(otag)
    order = ORDERS[otag]
    vol, grid, cot = b["A/vol"], b["A/grid"], d["cot/A"]
    ins, outs = vol.shape[2:], grid.shape[1:4]
    bd, od = (C.c_int * 3)(3, 3, 3), (C.c_int * 3)(*three(order))
    log = Log()
    for Bi, Bg in ((1, 2), (2, 1)):
        v, g, c, ci = T(vol[:Bi]), T(grid[:Bg]), T(cot), T(cot[:Bi])
        h = torch.empty((2, 3) + outs + (3, 3), device=DEV)
        assert lib.bfm_grid_hess3d(L.ptr(v), Bi, 3, *ins, L.ptr(g), Bg, *outs, bd, od, 1, None, L.ptr(h), L.stream_ptr()) == 0
        ref = HR.hess(vol[:Bi], grid[:Bg], order, 3, 1)
        log.close(h, ref, "hess Bi=%d Bg=%d" % (Bi, Bg), "hess broadcast")
        hc = torch.empty((2,) + outs + (3,), device=DEV)
        assert lib.bfm_grid_hess3d(L.ptr(v), Bi, 3, *ins, L.ptr(g), Bg, *outs, bd, od, 1, L.ptr(c), L.ptr(hc),
                                   L.stream_ptr()) == 0
        log.close(hc, HR.contract(ref, cot), "contracted Bi=%d Bg=%d" % (Bi, Bg), "contracted broadcast")
        p = torch.zeros((2, 3) + ins, device=DEV)
        assert lib.bfm_grid_pushgrad3d(L.ptr(ci), Bi, 3, *outs, L.ptr(g), Bg, *ins, bd, od, 1, L.ptr(p),
                                       L.stream_ptr()) == 0
        log.close(p, HR.pushgrad(cot[:Bi], grid[:Bg], ins, order, 3, 1), "pushgrad Bi=%d Bg=%d" % (Bi, Bg),
                  "pushgrad broadcast")
    # (X, Y, Z) input, no batch and no channel
    x, g = T(vol[0, 0]).requires_grad_(True), T(grid[0]).requires_grad_(True)
    y = IP.grid_grad(x, g, order, 3, 1)
    assert tuple(y.shape) == outs + (3,)
    w = sin_w(y)
    (y * w).sum().backward()
    wn = w.cpu().numpy().astype(np.float64)[None, None]
    assert tuple(x.grad.shape) == ins and tuple(g.grad.shape) == outs + (3,)
    log.close(x.grad, HR.pushgrad(wn, grid[:1], ins, order, 3, 1)[0, 0], "dinput (X,Y,Z)", "backward (X,Y,Z)")
    log.close(g.grad, HR.contract(HR.hess(vol[:1, :1], grid[:1], order, 3, 1), wn)[0], "dgrid (X,Y,Z)", "backward (X,Y,Z)")
    # a grid without batch dimension under a batch of two images
    x, g = T(vol).requires_grad_(True), T(grid[0]).requires_grad_(True)
    y = IP.grid_grad(x, g, order, 3, 1)
    assert tuple(y.shape) == (2, 3) + outs + (3,)
    w = sin_w(y)
    (y * w).sum().backward()
    wn = w.cpu().numpy().astype(np.float64)
    log.close(x.grad, HR.pushgrad(wn, grid[:1], ins, order, 3, 1), "dinput shared grid", "backward shared grid")
    log.close(g.grad, HR.contract(HR.hess(vol, grid[:1], order, 3, 1), wn).sum(0), "dgrid shared grid",
              "backward shared grid")
    log.show(otag)


def test_order_zero_gives_zeros_of_the_right_shapes():
    from brainfm_amd import interpol as IP
    vol, grid, cot = T(base()["A/vol"]), T(base()["A/grid"]), T(fixture("o0")["cot/A"])
    for order in (0, "nearest", [0, 0, 0]):
        h = IP.grid_hess(vol, grid, order, "dct2", True)
        assert tuple(h.shape) == (2, 3, 5, 9, 6, 3, 3) and not bool(h.any())
        p = IP.grid_pushgrad(cot, grid, [7, 6, 8], order, "dct2", True)
        assert tuple(p.shape) == (2, 3, 7, 6, 8) and not bool(p.any())
        v, g = vol.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        y = IP.grid_grad(v, g, order, "dct2", True)
        assert not bool(y.any())
        (y * sin_w(y)).sum().backward()
        assert v.grad is not None and tuple(v.grad.shape) == tuple(vol.shape) and not bool(v.grad.any())
        assert g.grad is not None and tuple(g.grad.shape) == tuple(grid.shape) and not bool(g.grad.any())
    b, o, e = IP._opts(0, 3, 1)                              # the contraction is written, not left as it was
    out = IP._hess_raw(vol, grid, b, o, e, cot=cot)
    assert tuple(out.shape) == (2, 5, 9, 6, 3) and not bool(out.any())
    assert not bool(IP.grid_pushgrad(cot[0, 0], grid[0], None, 0).any())


def test_one_launch_that_takes_the_grid_stride_loop():
    """(130,128,128) grid points, more than the 8192 x 256 threads of one launch, over a 16^3 one-channel volume at order 3
    under 'dct2'.  The contraction is compared on every 997th voxel and the last 4096; pushgrad gets a cotangent that is
    zero elsewhere, so that the same voxels make up its whole result."""
    from brainfm_amd import interpol as IP
    rng = np.random.default_rng(23)
    ins, outs = (16, 16, 16), (130, 128, 128)
    n = int(np.prod(outs))
    assert n > 8192 * 256
    vol = rng.standard_normal((1, 1) + ins).astype(np.float32)
    grid = (rng.random((1, n, 3)) * 21.0 - 2.5).astype(np.float32)
    cot = rng.standard_normal((1, 1, n, 3)).astype(np.float32)
    pick = np.unique(np.concatenate([np.arange(0, n, 997), np.arange(n - 4096, n)]))
    assert pick[-1] == n - 1 and (pick >= 8192 * 256).sum() > 4096
    sub_g, sub_c = grid[:, pick].reshape(1, -1, 1, 1, 3), cot[:, :, pick].reshape(1, 1, -1, 1, 1, 3)
    log = Log()
    b, o, e = IP._opts(3, "dct2", True)
    got = IP._hess_raw(T(vol), T(grid.reshape((1,) + outs + (3,))), b, o, e, cot=T(cot.reshape((1, 1) + outs + (3,))))
    ref = HR.contract(HR.hess(vol, sub_g, 3, 3, 1), sub_c)
    log.close(got.reshape(1, n, 3)[:, torch.from_numpy(pick).to(DEV)].reshape(ref.shape), ref, "contracted", "contracted")
    sparse = np.zeros_like(cot)
    sparse[:, :, pick] = cot[:, :, pick]
    p = IP.grid_pushgrad(T(sparse.reshape((1, 1) + outs + (3,))), T(grid.reshape((1,) + outs + (3,))), ins, 3, "dct2", True)
    log.close(p, HR.pushgrad(sub_c, sub_g, ins, 3, 3, 1), "pushgrad", "pushgrad")
    log.show("grid-stride")


def test_exports_refuse_bad_arguments_and_write_nothing():
    from brainfm_amd import _lib as L
    lib = L.load()
    vol = torch.randn(2, 1, 4, 5, 6, device=DEV)
    grid = torch.rand(2, 3, 3, 3, 3, device=DEV) * 4
    vec = torch.randn(2, 1, 3, 3, 3, 3, device=DEV)
    ok_b, ok_o = (C.c_int * 3)(0, 3, 6), (C.c_int * 3)(3, 0, 2)
    E_ARG, E_SHAPE = -1, -2

    def hess(cot):
        def run(inp, idims, g, gdims, out, bound=ok_b, order=ok_o, ext=1, Bi=2, Bg=2):
            return lib.bfm_grid_hess3d(L.ptr(inp), Bi, 1, *idims, L.ptr(g), Bg, *gdims, bound, order, ext, L.ptr(cot),
                                       L.ptr(out), L.stream_ptr())
        return run

    def pushgrad(inp, idims, g, gdims, out, bound=ok_b, order=ok_o, ext=1, Bi=2, Bg=2):
        return lib.bfm_grid_pushgrad3d(L.ptr(inp), Bi, 1, *idims, L.ptr(g), Bg, *gdims, bound, order, ext, L.ptr(out),
                                       L.stream_ptr())

    for name, run, inp, idims, gdims, oshape in (("hess", hess(None), vol, (4, 5, 6), (3, 3, 3), (3, 1, 3, 3, 3, 3, 3)),
                                                 ("hess contracted", hess(vec), vol, (4, 5, 6), (3, 3, 3), (3, 3, 3, 3, 3)),
                                                 ("pushgrad", pushgrad, vec, (3, 3, 3), (4, 5, 6), (3, 1, 4, 5, 6))):
        out = torch.full(oshape, 7.0, device=DEV)
        assert run(None, idims, grid, gdims, out) == E_ARG, name
        assert run(inp, idims, None, gdims, out) == E_ARG, name
        assert run(inp, idims, grid, gdims, None) == E_ARG, name
        assert run(inp, idims, grid, gdims, out, bound=None) == E_ARG, name
        assert run(inp, idims, grid, gdims, out, order=None) == E_ARG, name
        for bad in ((4, 0, 0), (0, -1, 0), (3, 3, 7)):
            assert run(inp, idims, grid, gdims, out, order=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        for bad in ((7, 0, 0), (0, 0, -1)):
            assert run(inp, idims, grid, gdims, out, bound=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        assert run(inp, idims, grid, gdims, out, ext=3) == E_ARG, name
        assert run(inp, idims, grid, gdims, out, ext=-1) == E_ARG, name
        assert run(inp, (4, 0, 6), grid, gdims, out) == E_ARG, name
        assert run(inp, idims, grid, (3, -3, 3), out) == E_ARG, name
        assert run(inp, idims, grid, gdims, out, Bi=0) == E_ARG, name
        assert run(inp, idims, grid, gdims, out, Bi=2, Bg=3) == E_SHAPE, name
        assert run(inp, idims, grid, gdims, out, Bi=3, Bg=2) == E_SHAPE, name
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), name
