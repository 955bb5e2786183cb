"""interpol.grid_pull / grid_push / grid_count / grid_grad at spline orders 0, 2, 3 and mixed orders on the device
(brainfm_amd/csrc/spline_grid.hip), the prefilter under its three families of boundary conditions and its gradient,
against the reference's own results (tests/golden/interpol_spline_grid*.npz, float64 runs of the vendored torch-interpol
rounded to float32) and against the float64 restatement (tests/spline_grid_refs.py) on a shape that takes several
blocks and a ragged tail.

The bar is the one the project applies to this family at order 1 (test_gpu_synth.py): max|hip - ref| <= 2e-5 * max(1,
max|ref|).  The reference's own float32 run sits 1e-7 to 4e-6 from its float64 run on these arrays (stored next to each
array and printed beside the measured distance); a wrong tap, weight or sign is off by 1e-2 or more."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_npz
import spline_grid_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = {"o0": 0, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
_BASE = {}


def base():
    if not _BASE:
        _BASE.update(load_npz("interpol_spline_grid.npz"))
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
    """pull / push / grad for the seven bounds with and without extrapolation (and 'hist' once), count and the four
    backward arrays under 'zero' and 'dct2', pull with prefilter=True and its gradient at orders 2 and 3: both shapes."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_spline_grid_%s.npz" % otag)
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
            chk(IP.grid_grad(vol, grid, order, bound, ext), "grad")
            if k + "count" not in d:
                continue
            chk(IP.grid_count(grid, ins, order, bound, ext), "count")
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
    assert ("pull_pf" in log.worst) == (otag in ("o2", "o3"))
    log.show(otag)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_batch_broadcast_and_channelless_input(otag):
    """Bi = 1 against Bg = 2 (and the reverse for push), and the (X, Y, Z) input form of the high-level interface."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_spline_grid_%s.npz" % otag)
    order = ORDERS[otag]
    b = base()
    vol, grid, src = T(b["A/vol"]), T(b["A/grid"]), T(b["A/src"])
    ins = list(vol.shape[2:])
    log = Log()
    for bound, ext in ((0, 0), (3, 1), (6, 1)):
        k = "A/b%d_e%d/" % (bound, ext)
        got = IP.grid_pull(vol[:1], grid, order, bound, ext)                   # one image under two grids
        assert tuple(got.shape) == (2, 3, 5, 9, 6)
        log.close(got[:1], d[k + "pull"][:1], k + "pull Bi=1", "pull Bi=1")
        log.close(got, SR.pull(b["A/vol"][:1], b["A/grid"], order, bound, ext), k + "pull Bi=1 vs restatement", "pull Bi=1")
        got = IP.grid_grad(vol, grid[:1], order, bound, ext)                   # two images under one grid
        log.close(got[:1], d[k + "grad"][:1], k + "grad Bg=1", "grad Bg=1")
        log.close(got, SR.grad(b["A/vol"], b["A/grid"][:1], order, bound, ext), k + "grad Bg=1 vs restatement", "grad Bg=1")
        got = IP.grid_push(src[:1], grid, ins, order, bound, ext)
        log.close(got[:1], d[k + "push"][:1], k + "push Bi=1", "push Bi=1")
        log.close(got, SR.push(b["A/src"][:1], b["A/grid"], ins, order, bound, ext), k + "push Bi=1 vs restatement",
                  "push Bi=1")
        got = IP.grid_pull(vol[0, 0], grid[0], order, bound, ext)              # no batch, no channel
        assert tuple(got.shape) == (5, 9, 6)
        log.close(got, d[k + "pull"][0, 0], k + "pull (X,Y,Z)", "pull (X,Y,Z)")
        got = IP.grid_grad(vol[0, 0], grid[0], order, bound, ext)
        assert tuple(got.shape) == (5, 9, 6, 3)
        log.close(got, d[k + "grad"][0, 0], k + "grad (X,Y,Z)", "grad (X,Y,Z)")
        got = IP.grid_push(src[0, 0], grid[0], ins, order, bound, ext)
        assert tuple(got.shape) == tuple(ins)
        log.close(got, d[k + "push"][0, 0], k + "push (X,Y,Z)", "push (X,Y,Z)")
    log.show(otag)


_BIG = {}


def big_inputs():
    """33 x 17 x 40 input, 40 x 9 x 33 grid (11 880 voxels: 47 blocks of 256, the last one ragged), two channels; the
    coordinates spill 2.5 voxels over every face and keep the fixture's margin from every jump."""
    if not _BIG:
        rng = np.random.default_rng(7)
        ins, outs = (33, 17, 40), (40, 9, 33)
        grid = (rng.random((1,) + outs + (3,)) * (np.array(ins) + 5.0) - 2.5).astype(np.float32)
        grid = SR.redraw_near_jumps(grid, ins, rng, 1e-3)
        assert not SR.near_jumps(grid, ins, 1e-3).any()
        _BIG.update(vol=rng.standard_normal((1, 2) + ins).astype(np.float32), grid=grid,
                    src=rng.standard_normal((1, 2) + outs).astype(np.float32))
    return _BIG


@pytest.mark.parametrize("bound", ["zero", "dct2", "dft"])
@pytest.mark.parametrize("otag", ["o0", "o2", "o3", "o312"])
def test_several_blocks_and_a_ragged_tail_against_the_restatement(otag, bound):
    from brainfm_amd import interpol as IP
    order = ORDERS[otag]
    bi = IP._BOUND[bound]
    ext = 0 if bound == "zero" else 1
    b = big_inputs()
    vol, grid, src = T(b["vol"]), T(b["grid"]), T(b["src"])
    ins = list(vol.shape[2:])
    log = Log()
    log.close(IP.grid_pull(vol, grid, order, bound, ext), SR.pull(b["vol"], b["grid"], order, bi, ext), "pull", "pull")
    log.close(IP.grid_grad(vol, grid, order, bound, ext), SR.grad(b["vol"], b["grid"], order, bi, ext), "grad", "grad")
    log.close(IP.grid_push(src, grid, ins, order, bound, ext), SR.push(b["src"], b["grid"], ins, order, bi, ext), "push",
              "push")
    log.show("%s %s" % (otag, bound))


def test_prefilter_families_and_its_gradient():
    """spline_coeff_nd at orders 2 and 3 under 'zero' / 'dct1' (DCT-I), 'nearest' / 'dct2' (DCT-II) and 'dft' against the
    reference, both shapes (the thin one has an axis of length 1, which is skipped, and one of length 2); on a tensor
    that requires grad it returns the filter of the incoming gradient (the filter is symmetric)."""
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
                c = IP.spline_coeff_nd(x, order, bound, 3)
                log.close(c, b[k], k, "coeff o%d" % order, b[k + ".err"])
                assert torch.equal(c.detach(), IP.spline_coeff_nd(vol, order, bound, 3))
                c.backward(w)
                assert torch.equal(x.grad, IP.spline_coeff_nd(w, order, bound, 3)), k
                assert not torch.equal(x.grad, w)                              # not the identity it used to be
    # mixed orders filter each axis with its own pole; orders 0 / 1 leave an axis alone
    vol = T(b["A/vol"])
    mixed = IP.spline_coeff_nd(vol, [3, 1, 2], "dct2", 3)
    step = IP.spline_coeff_nd(IP.spline_coeff_nd(vol, [3, 1, 1], "dct2", 3), [1, 1, 2], "dct2", 3)
    assert torch.equal(mixed, step)
    assert torch.equal(IP.spline_coeff_nd(vol, [0, 1, 0], "dct2", 3), vol)
    log.show("prefilter")


def test_resize_orders_and_the_cases_the_separable_path_refuses():
    from brainfm_amd import interpol as IP
    b = base()
    vol = T(b["A/vol"])
    log = Log()
    y = IP.resize(vol, shape=[10, 9, 11], anchor="e", interpolation=2, prefilter=True)
    log.close(y, b["resize/o2_edge"], "resize o2 edge", "resize o2", b["resize/o2_edge.err"])
    y = IP.resize(vol, shape=[9, 8, 11], anchor="c", interpolation=3, prefilter=True, bound="zero", extrapolate=False)
    log.close(y, b["resize/o3_zero_noext"], "resize o3 zero", "resize o3", b["resize/o3_zero_noext.err"])
    y0 = IP.resize(vol, shape=[9, 8, 11], interpolation=0)                    # nearest: values of the input itself
    assert tuple(y0.shape) == (2, 3, 9, 8, 11) and bool(torch.isin(y0, vol).all())
    log.show("resize")


def test_linear_calls_keep_their_kernels_and_their_bits():
    """interpolation=1 and [1, 1, 1] go to the linear kernels, whose arithmetic is iso1's as it always was: equal bits
    for pull and grad.  push adds with fp32 atomics, whose order differs from launch to launch (spline_grid.hip says so),
    so two launches are held to 4 units in the last place of the largest value instead; all three still meet the order-1
    fixture."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_pushgrad.npz")
    vol, grid, src = (T(d[k]) for k in ("vol", "grid", "src"))
    ins = list(vol.shape[2:])
    log = Log()
    for bound in range(7):
        for ext in (0, 1):
            k = "b%d_e%d/" % (bound, ext)
            a, a3 = IP.grid_pull(vol, grid, 1, bound, bool(ext)), IP.grid_pull(vol, grid, [1, 1, 1], bound, bool(ext))
            assert torch.equal(a, a3), k
            g1, g3 = IP.grid_grad(vol, grid, 1, bound, bool(ext)), IP.grid_grad(vol, grid, ["linear"] * 3, bound, bool(ext))
            assert torch.equal(g1, g3), k
            log.close(g1, d[k + "grad"], k + "grad", "grad order 1")
            p1, p3 = IP.grid_push(src, grid, ins, 1, bound, bool(ext)), IP.grid_push(src, grid, ins, [1, 1, 1], bound, bool(ext))
            assert float((p1 - p3).abs().max()) <= 4 * 2.0 ** -23 * float(p1.abs().max()), k
            log.close(p1, d[k + "push"], k + "push", "push order 1")
            # the generic kernels at order {1,1,1} (the export accepts it) agree with the linear ones on pull
            out = torch.empty_like(a)
            B, Cc = vol.shape[:2]
            from brainfm_amd import _lib as L
            rc = L.load().bfm_grid_pull3d_spline(L.ptr(vol), B, Cc, *ins, L.ptr(grid), B, *grid.shape[1:4],
                                                 (C.c_int * 3)(bound, bound, bound), (C.c_int * 3)(1, 1, 1), ext,
                                                 L.ptr(out), L.stream_ptr())
            assert rc == 0
            log.close(out, a.cpu().numpy().astype(np.float64), k + "generic pull at order 1", "generic o1")
    log.show("linear")


def test_exports_refuse_bad_arguments_and_write_nothing():
    from brainfm_amd import _lib as L
    lib = L.load()
    vol = torch.randn(2, 1, 4, 5, 6, device=DEV)
    grid = torch.rand(2, 3, 3, 3, 3, device=DEV) * 4
    src = torch.randn(2, 1, 3, 3, 3, device=DEV)
    ok_b, ok_o = (C.c_int * 3)(0, 3, 6), (C.c_int * 3)(3, 0, 2)
    E_ARG, E_SHAPE = -1, -2

    def run(fn, inp, idims, g, gdims, out, bound=ok_b, order=ok_o, ext=1, Bi=2, Bg=2):
        return fn(L.ptr(inp), Bi, 1, *idims, L.ptr(g), Bg, *gdims, bound, order, ext, L.ptr(out), L.stream_ptr())

    for name, inp, idims, gdims, oshape in (("bfm_grid_pull3d_spline", vol, (4, 5, 6), (3, 3, 3), (3, 1, 3, 3, 3)),
                                            ("bfm_grid_grad3d_spline", vol, (4, 5, 6), (3, 3, 3), (3, 1, 3, 3, 3, 3)),
                                            ("bfm_grid_push3d_spline", src, (3, 3, 3), (4, 5, 6), (3, 1, 4, 5, 6))):
        fn = getattr(lib, name)
        out = torch.full(oshape, 7.0, device=DEV)
        assert run(fn, None, idims, grid, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, None, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, None) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, bound=None) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, order=None) == E_ARG, name
        for bad in ((4, 0, 0), (0, -1, 0), (3, 3, 7)):
            assert run(fn, inp, idims, grid, gdims, out, order=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        for bad in ((7, 0, 0), (0, 0, -1)):
            assert run(fn, inp, idims, grid, gdims, out, bound=(C.c_int * 3)(*bad)) == E_ARG, (name, bad)
        assert run(fn, inp, idims, grid, gdims, out, ext=3) == E_ARG, name
        assert run(fn, inp, (4, 0, 6), grid, gdims, out) == E_ARG, name
        assert run(fn, inp, idims, grid, gdims, out, Bi=2, Bg=3) == E_SHAPE, name
        assert run(fn, inp, idims, grid, gdims, out, Bi=3, Bg=2) == E_SHAPE, name
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), name
