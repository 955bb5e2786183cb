"""interpol.grid_pull / grid_push / grid_count on 2-D grids on the device (the D = 2 instantiations of
brainfm_amd/csrc/spline_grid.hip), their
first-order backward, the 2-D prefilter and the 2-D resize, against the reference's own results
(tests/golden/interpol_grid2d*.npz, float64 runs of the vendored torch-interpol rounded to float32), against the float64
restatement (tests/grid2d_refs.py) on shapes the fixture does not have, and bit for bit against the 3-D kernels on the
embedded problem.

The bar is the one test_gpu_spline_grid.py applies to this family: max|hip - ref| <= 2e-5 * max(1, max|ref|)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_npz
import grid2d_refs as GR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o31": [3, 1], "o02": [0, 2]}
_BASE = {}


def base():
    if not _BASE:
        _BASE.update(load_npz("interpol_grid2d.npz"))
    return _BASE


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Log:
    """worst max|hip - ref| per kind of array, with the stored max|ref32 - ref64| of the same array"""

    def __init__(self):
        self.worst = {}

    def close(self, got, ref, what, kind, stored=float("nan")):
        got = got.detach().cpu().numpy()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        if err >= self.worst.get(kind, (-1.0, 0.0))[0]:
            self.worst[kind] = (err, float(stored))
        assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)

    def show(self, title):
        for kind, (err, stored) in sorted(self.worst.items()):
            ref = "stored max|ref32 - ref64| %.2e" % stored if stored == stored else "ref: float64 restatement"
            print("%-10s %-16s max|hip - ref| %.2e   %s" % (title, kind, err, ref))


@pytest.mark.parametrize("otag", list(ORDERS))
def test_every_array_of_the_fixture(otag):
    """pull / push / count for the seven bounds with and without extrapolation (and 'hist' once), the four backward arrays
    under 'zero' and 'dct2', pull with prefilter=True and its gradient at orders 2 and 3: both shapes."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_grid2d_%s.npz" % otag)
    order = ORDERS[otag]
    log = Log()
    for tag in ("A", "T"):
        vol, grid, src = (T(base()["%s/%s" % (tag, k)]) for k in ("vol", "grid", "src"))
        ins = list(vol.shape[2:])
        combos = sorted({k.split("/")[1] for k in d if k.startswith(tag + "/")})
        assert len(combos) == 15
        for combo in combos:
            bound, ext = int(combo[1]), int(combo[4])
            k = "%s/%s/" % (tag, combo)

            def chk(got, name):
                log.close(got, d[k + name], k + name, name, d[k + name + ".err"])

            chk(IP.grid_pull(vol, grid, order, bound, ext), "pull")
            chk(IP.grid_push(src, grid, ins, order, bound, ext), "push")
            chk(IP.grid_count(grid, ins, order, bound, ext), "count")
            if k + "pull_dinput" not in d:
                continue
            v, gr = vol.clone().requires_grad_(True), grid.clone().requires_grad_(True)
            y = IP.grid_pull(v, gr, order, bound, ext)
            w = torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(DEV)
            (y * w).sum().backward()
            chk(v.grad, "pull_dinput")
            chk(gr.grad, "pull_dgrid")
            s_, gr = src.clone().requires_grad_(True), grid.clone().requires_grad_(True)
            y = IP.grid_push(s_, gr, ins, order, bound, ext)
            w2 = torch.cos(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(DEV)
            (y * w2).sum().backward()
            chk(s_.grad, "push_dinput")
            chk(gr.grad, "push_dgrid")
            if k + "pull_pf" in d:
                v = vol.clone().requires_grad_(True)
                y = IP.grid_pull(v, grid, order, bound, ext, prefilter=True)
                chk(y, "pull_pf")
                (y * w).sum().backward()
                chk(v.grad, "pull_pf_dinput")
    assert "pull_dgrid" in log.worst and ("pull_pf" in log.worst) == (otag in ("o2", "o3"))
    log.show(otag)


def test_all_nearest_pull_takes_every_batch_and_channel_count():
    """B = 2, C = 3 under a mask, where the reference's iso0.pull2d has no defined result: the
    goldens of these cases come from the reference's generic path."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_grid2d_o0.npz")
    vol, grid = T(base()["A/vol"]), T(base()["A/grid"])
    log = Log()
    for combo in ["b%d_e0" % b for b in range(7)] + ["b3_e2"]:
        bound, ext = int(combo[1]), int(combo[4])
        got = IP.grid_pull(vol, grid, "nearest", bound, ext)
        assert tuple(got.shape) == (2, 3, 5, 9)
        log.close(got, d["A/%s/pull" % combo], combo, "pull o0", d["A/%s/pull.err" % combo])
        assert bool((got == 0).any()) and bool((got != 0).any())              # some pixels masked, some not
    log.show("nearest")


@pytest.mark.parametrize("otag", list(ORDERS))
def test_batch_broadcast_and_the_unbatched_forms(otag):
    """Bi = 1 against Bg = 2 and the reverse, and the (X, Y) image with an (X, Y, 2) grid, against the restatement."""
    from brainfm_amd import interpol as IP
    order = ORDERS[otag]
    b = base()
    vol, grid, src = T(b["A/vol"]), T(b["A/grid"]), T(b["A/src"])
    ins = list(vol.shape[2:])
    log = Log()
    for bound, ext in ((0, 0), (3, 1), (6, 1)):
        k = "b%d_e%d " % (bound, ext)
        got = IP.grid_pull(vol[:1], grid, order, bound, ext)                   # one image under two grids
        assert tuple(got.shape) == (2, 3, 5, 9)
        log.close(got, GR.pull(b["A/vol"][:1], b["A/grid"], order, bound, ext), k + "pull Bi=1", "pull Bi=1")
        got = IP.grid_pull(vol, grid[:1], order, bound, ext)                   # two images under one grid
        log.close(got, GR.pull(b["A/vol"], b["A/grid"][:1], order, bound, ext), k + "pull Bg=1", "pull Bg=1")
        got = IP.grid_push(src[:1], grid, ins, order, bound, ext)
        log.close(got, GR.push(b["A/src"][:1], b["A/grid"], ins, order, bound, ext), k + "push Bi=1", "push Bi=1")
        got = IP.grid_push(src, grid[:1], ins, order, bound, ext)
        log.close(got, GR.push(b["A/src"], b["A/grid"][:1], ins, order, bound, ext), k + "push Bg=1", "push Bg=1")
        got = IP.grid_pull(vol[0, 0], grid[0], order, bound, ext)              # no batch, no channel
        assert tuple(got.shape) == (5, 9)
        log.close(got, GR.pull(b["A/vol"][:1, :1], b["A/grid"][:1], order, bound, ext)[0, 0], k + "pull (X,Y)", "pull (X,Y)")
        got = IP.grid_push(src[0, 0], grid[0], ins, order, bound, ext)
        assert tuple(got.shape) == tuple(ins)
        log.close(got, GR.push(b["A/src"][:1, :1], b["A/grid"][:1], ins, order, bound, ext)[0, 0], k + "push (X,Y)",
                  "push (X,Y)")
        got = IP.grid_count(grid[0], ins, order, bound, ext)                   # (..., [1], *shape), as in 3-D
        assert tuple(got.shape) == (1,) + tuple(ins)
        log.close(got, GR.count(b["A/grid"][:1], ins, order, bound, ext)[0], k + "count (X,Y,2)", "count (X,Y,2)")
        got = IP.grid_pull(vol[0], grid[0], order, bound, ext)                 # channels, no batch
        assert tuple(got.shape) == (3, 5, 9)
        log.close(got, GR.pull(b["A/vol"][:1], b["A/grid"][:1], order, bound, ext)[0], k + "pull (C,X,Y)", "pull (C,X,Y)")
    log.show(otag)


_BIG = {}


def big_inputs():
    """37 x 29 image with two channels, 2 x 61 x 43 grid (5 246 pixels: 21 blocks of 256, the last one ragged); the
    coordinates spill 2.5 pixels over every edge and keep the fixture's margin from every jump."""
    if not _BIG:
        rng = np.random.default_rng(11)
        ins, outs = (37, 29), (61, 43)
        grid = (rng.random((2,) + outs + (2,)) * (np.array(ins) + 5.0) - 2.5).astype(np.float32)
        grid = GR.redraw_near_jumps(grid, ins, rng, 1e-3)
        assert not GR.near_jumps(grid, ins, 1e-3).any()
        _BIG.update(vol=rng.standard_normal((1, 2) + ins).astype(np.float32), grid=grid,
                    src=rng.standard_normal((1, 2) + outs).astype(np.float32),
                    w=rng.standard_normal((2, 2) + outs).astype(np.float32))
    return _BIG


@pytest.mark.parametrize("otag", list(ORDERS))
def test_several_blocks_and_a_ragged_tail_against_the_restatement(otag):
    """pull, push, count, the 2-D gradient and both gradients of pull"""
    from brainfm_amd import interpol as IP
    order = ORDERS[otag]
    b = big_inputs()
    vol, grid, src, w = T(b["vol"]), T(b["grid"]), T(b["src"]), T(b["w"])
    ins = list(vol.shape[2:])
    log = Log()
    for bound, ext in (("zero", 0), ("dct2", 1)):
        bi = IP._BOUND[bound]
        log.close(IP.grid_pull(vol, grid, order, bound, ext), GR.pull(b["vol"], b["grid"], order, bi, ext), "pull", "pull")
        log.close(IP.grid_push(src, grid, ins, order, bound, ext), GR.push(b["src"], b["grid"], ins, order, bi, ext),
                  "push", "push")
        log.close(IP.grid_count(grid, ins, order, bound, ext), GR.count(b["grid"], ins, order, bi, ext), "count", "count")
        bb, oo, ee = IP._opts(order, bound, ext)
        ref_grad = GR.grad(b["vol"], b["grid"], order, bi, ext)
        log.close(IP._grad_raw(vol, grid, bb, oo, ee), ref_grad, "grad", "grad")
        v, gr = vol.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        (IP.grid_pull(v, gr, order, bound, ext) * w).sum().backward()
        log.close(v.grad, GR.push(b["w"], b["grid"], ins, order, bi, ext).sum(0, keepdims=True), "pull_dinput", "pull_dinput")
        log.close(gr.grad, (ref_grad * b["w"].astype(np.float64)[..., None]).sum(1), "pull_dgrid", "pull_dgrid")
    log.show(otag)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_pull_has_the_bits_of_the_3d_kernels_on_the_embedded_problem(otag):
    """image[..., None], a third coordinate 0 and orders (ox, oy, 0): the extra factor of the 3-D kernels is an exact 1 and
    their padded taps add exact zeros to finite sums, so equal bits pin the nodes, weights, signs and the tap order."""
    from brainfm_amd import interpol as IP
    order = ORDERS[otag]
    o2 = order if isinstance(order, list) else [order, order]
    for data in (dict(vol=base()["A/vol"], grid=base()["A/grid"]), big_inputs()):
        vol, grid = T(data["vol"]), T(data["grid"])
        vol3 = vol[..., None].contiguous()
        grid3 = torch.cat([grid, torch.zeros_like(grid[..., :1])], -1)[..., None, :].contiguous()
        for bound in (0, 3, 6):
            for ext in (0, 1):
                got = IP.grid_pull(vol, grid, order, bound, ext)
                emb = IP.grid_pull(vol3, grid3, o2 + [0], bound, ext)[..., 0]
                assert torch.equal(got, emb), (otag, bound, ext, float((got - emb).abs().max()))
                assert bool((got != 0).any())


def test_prefilter_families_its_gradient_and_interpolation_at_the_nodes():
    from brainfm_amd import interpol as IP
    b = base()
    log = Log()
    for tag in ("A", "T"):
        vol = T(b[tag + "/vol"])
        w = torch.cos(torch.arange(vol.numel(), dtype=torch.float32)).reshape(vol.shape).to(DEV)
        for order in (2, 3):
            for bound in (0, 1, 2, 3, 6):
                k = "%s/coeff/o%d_b%d" % (tag, order, bound)
                x = vol.clone().requires_grad_(True)
                c = IP.spline_coeff_nd(x, order, bound, 2)
                log.close(c, b[k], k, "coeff o%d" % order, b[k + ".err"])
                assert torch.equal(c.detach(), IP.spline_coeff_nd(vol, order, bound, 2))
                c.backward(w)
                assert torch.equal(x.grad, IP.spline_coeff_nd(w, order, bound, 2)), k
                assert not torch.equal(x.grad, w)
    vol = T(b["A/vol"])
    # one launch per filtered axis over the whole batch gives what one image at a time gives
    whole = IP.spline_coeff_nd(vol, 3, "dct2", 2)
    assert torch.equal(whole[1, 2], IP.spline_coeff_nd(vol[1, 2], 3, "dct2", 2))
    mixed = IP.spline_coeff_nd(vol, [3, 2], "dct2", 2)
    assert torch.equal(mixed, IP.spline_coeff_nd(IP.spline_coeff_nd(vol, [3, 1], "dct2", 2), [1, 2], "dct2", 2))
    assert torch.equal(IP.spline_coeff_nd(vol, [0, 1], "dct2", 2), vol)
    inplace = vol.clone()
    assert IP.spline_coeff_nd(inplace, 3, "dct2", 2, inplace=True).data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace, whole)
    # prefilter=True interpolates: at the nodes the image comes back
    ident = IP.identity_grid(vol.shape[2:], dtype=torch.float32, device=DEV)
    for order in (2, 3, [3, 2]):
        for bound in ("dct2", "dct1", "dft"):
            got = IP.grid_pull(vol, ident, order, bound, True, prefilter=True)
            log.close(got, b["A/vol"].astype(np.float64), "nodes o%s %s" % (order, bound), "at the nodes")
    log.show("prefilter")


def test_resize_goldens_and_its_gradient():
    from brainfm_amd import interpol as IP
    b = base()
    vol = T(b["A/vol"])
    log = Log()
    y = IP.resize(vol, shape=[10, 9], interpolation=3, bound="dct2", prefilter=True)
    log.close(y, b["resize/o3_dct2"], "resize o3 dct2", "resize o3", b["resize/o3_dct2.err"])
    y = IP.resize(vol, factor=[2, 1.5], anchor="e", interpolation=1)
    log.close(y, b["resize/o1_edge"], "resize o1 edge", "resize o1", b["resize/o1_edge.err"])
    y = IP.resize(vol[0, 0], shape=[9, 8], interpolation=2, prefilter=True)
    assert tuple(y.shape) == (9, 8)
    log.close(y, b["resize/o2_unbatched"], "resize o2 unbatched", "resize o2", b["resize/o2_unbatched.err"])
    y = IP.resize(vol, shape=[10, 9], interpolation="cubic", bound="dct2", prefilter=True)     # orders by name
    log.close(y, b["resize/o3_dct2"], "resize cubic by name", "resize o3", b["resize/o3_dct2.err"])
    y0 = IP.resize(vol, shape=[9, 8], interpolation=0)
    assert tuple(y0.shape) == (2, 3, 9, 8) and bool(torch.isin(y0, vol).all())
    # the gradient of the sum is the push of ones through the resize grid (bound 'nearest', extrapolate on)
    ins = tuple(vol.shape[2:])
    for order, kw in ((1, dict(factor=[2, 1.5], anchor="e")), (2, dict(shape=[9, 8], anchor="c")),
                      (3, dict(shape=[10, 9], anchor=["f", "l"]))):
        x = vol.clone().requires_grad_(True)
        y = IP.resize(x, interpolation=order, prefilter=False, **kw)
        y.sum().backward()
        outs = tuple(y.shape[2:])
        factor = kw.get("factor", [o / i for o, i in zip(outs, ins)])
        anchor = kw["anchor"] if isinstance(kw["anchor"], list) else [kw["anchor"]] * 2
        lin = [IP._anchor_coords(a, f, i, o).numpy() for a, f, i, o in zip(anchor, factor, ins, outs)]
        grid = np.stack(np.meshgrid(*lin, indexing="ij"), -1)[None]
        ref = GR.push(np.ones((1, 1) + outs), grid, ins, order, 1, 1)
        log.close(x.grad, np.broadcast_to(ref, x.shape), "resize backward o%d" % order, "resize backward")
    for kw in (dict(factor=[2]), dict(shape=[8]), dict(factor=2, anchor=["c"])):       # one entry: a 1-D resize
        with pytest.raises(NotImplementedError):
            IP.resize(vol, **kw)
    log.show("resize")


def test_pull_and_gradient_give_the_same_bits_twice():
    from brainfm_amd import interpol as IP
    b = big_inputs()
    vol, grid = T(b["vol"]), T(b["grid"])
    for order in ORDERS.values():
        bb, oo, ee = IP._opts(order, "dct2", 1)
        assert torch.equal(IP.grid_pull(vol, grid, order, "dct2", 1), IP.grid_pull(vol, grid, order, "dct2", 1))
        assert torch.equal(IP._grad_raw(vol, grid, bb, oo, ee), IP._grad_raw(vol, grid, bb, oo, ee))


def test_second_backward_and_one_dimensional_grids_raise_on_the_device():
    from brainfm_amd import interpol as IP
    vol, grid = T(base()["A/vol"]), T(base()["A/grid"])
    v = vol.clone().requires_grad_(True)
    y = IP.grid_pull(v, grid, 3, "dct2", 1)
    (g,) = torch.autograd.grad(y.sum(), v, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    line, g1 = torch.zeros(1, 1, 4, device=DEV), torch.zeros(1, 2, 1, device=DEV)
    for call in (lambda: IP.grid_pull(line, g1), lambda: IP.grid_push(line[..., :2], g1), lambda: IP.grid_count(g1),
                 lambda: IP.spline_coeff_nd(line, 3, "dct2", 1), lambda: IP.grid_grad(vol, grid),
                 lambda: IP.grid_pull(vol.to(torch.int32), grid)):
        with pytest.raises(NotImplementedError):
            call()


def test_exports_refuse_bad_arguments_and_write_nothing():
    from brainfm_amd import _lib as L
    lib = L.load()
    vol = torch.randn(2, 1, 4, 5, device=DEV)
    grid = torch.rand(2, 3, 3, 2, device=DEV) * 4
    src = torch.randn(2, 1, 3, 3, device=DEV)
    ok_b, ok_o = (C.c_int * 3)(0, 3, 6), (C.c_int * 3)(3, 0, 2)
    E_ARG, E_SHAPE = -1, -2

    def run(fn, inp, idims, g, gdims, out, bound=ok_b, order=ok_o, ext=1, Bi=2, Bg=2):
        return fn(L.ptr(inp), Bi, 1, *idims, L.ptr(g), Bg, *gdims, bound, order, ext, L.ptr(out), L.stream_ptr())

    for name, inp, idims, gdims, oshape in (("bfm_grid_pull2d_spline", vol, (4, 5), (3, 3), (3, 1, 3, 3)),
                                            ("bfm_grid_grad2d_spline", vol, (4, 5), (3, 3), (3, 1, 3, 3, 2)),
                                            ("bfm_grid_push2d_spline", src, (3, 3), (4, 5), (3, 1, 4, 5))):
        fn = getattr(lib, name)
        out = torch.full(oshape, 7.0, device=DEV)
        assert run(fn, None, idims, grid, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, None, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, None) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, bound=None) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, order=None) == E_ARG, name
        for bad in ((4, 0, 0), (0, -1, 0)):
            assert run(fn, inp, idims, grid, gdims, out, order=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        for bad in ((7, 0, 0), (0, -1, 0)):
            assert run(fn, inp, idims, grid, gdims, out, bound=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        assert run(fn, inp, idims, grid, gdims, out, ext=3) == E_ARG, name
        assert run(fn, inp, (4, 0), grid, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, Bi=2, Bg=3) == E_SHAPE, name
        assert run(fn, inp, idims, grid, gdims, out, Bi=3, Bg=2) == E_SHAPE, name
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), name
    # two entries of bound and order are read: a third one is not looked at
    out = torch.empty(2, 1, 3, 3, device=DEV)
    assert run(lib.bfm_grid_pull2d_spline, vol, (4, 5), grid, (3, 3), out, bound=(C.c_int * 3)(0, 3, 9),
               order=(C.c_int * 3)(3, 0, 9)) == 0
    want = torch.empty_like(out)
    assert run(lib.bfm_grid_pull2d_spline, vol, (4, 5), grid, (3, 3), want) == 0
    assert torch.equal(out, want)
