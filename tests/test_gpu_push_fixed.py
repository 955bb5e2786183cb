"""The "fixed" push mode of interpol on the device: grid_push / grid_count / grid_pushgrad and the backward of grid_pull /
grid_grad through 64-bit fixed-point accumulators (brainfm_amd/csrc/push_accum.h, push_fixed.hip).

Bits are compared against the int64 emulation of the format (tests/push_fixed_refs.py) where the kernels' weights are
exactly 0 or +-1, so that the emulation's contributions are the kernels' to the bit; sums against the float64
restatements of the family (spline_grid_refs, grid2d_refs, grid_hess_refs) under the family's bar, max|hip - ref| <= 2e-5
* max(1, max|ref|).  Every test sets the mode and restores it in `finally` (the `mode` context)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import grid2d_refs as G2
import grid_hess_refs as HR
import push_fixed_refs as FR
import spline_grid_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VOL, PTS = (5, 6, 7), (9, 8, 7)               # volume and points, 3-D
VOL2, PTS2 = (6, 7), (11, 13)                 # 2-D
B, CH = 2, 3


@contextlib.contextmanager
def mode(m):
    from brainfm_amd import interpol as IP
    IP.set_push_mode(m)
    try:
        yield IP
    finally:
        IP.set_push_mode(None)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def wide(rng, shape):
    """randn * 2^randint(-20, 20)"""
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 20, shape)).astype(np.float32)


def free_grid(rng, b, pts, vol, redraw):
    g = (rng.random((b,) + pts + (len(vol),)) * (np.array(vol) + 5.0) - 2.5).astype(np.float32)
    return redraw(g, vol, rng)


def int_grid(rng, b, pts, vol):
    return rng.integers(-3, np.array(vol) + 3, (b,) + pts + (len(vol),)).astype(np.float32)


def close(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)
    return err


# ------------------------------------------------------------------------------------------------ 1. bits against the emulation
def test_exact_bits_order0_every_bound_and_extrapolate():
    rng = np.random.default_rng(10)
    x, g = wide(rng, (B, CH) + PTS), free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
    x2, g2 = wide(rng, (B, CH) + PTS2), free_grid(rng, B, PTS2, VOL2, G2.redraw_near_jumps)
    with mode("fixed") as IP:
        for bound in range(7):
            for ext in (0, 1, "hist"):
                e = IP._extrap(ext)
                got = IP.grid_push(T(x), T(g), VOL, 0, bound, ext)
                assert bits_equal(got, T(FR.fixed("push", x, g, VOL, 0, bound, e))), ("3-D", bound, ext)
                got = IP.grid_push(T(x2), T(g2), VOL2, 0, bound, ext)
                assert bits_equal(got, T(FR.fixed("push", x2, g2, VOL2, 0, bound, e))), ("2-D", bound, ext)


def test_exact_bits_order1_on_integer_coordinates():
    """3-D linear export (order 1), 3-D spline export (orders {1,1,1} called directly, {1,0,1} padded), 2-D orders 1 and
    {1,0}, a broadcast input (Bi = 1), and grid_pushgrad at order 1 and {1,0,1}."""
    rng = np.random.default_rng(11)
    x, g = wide(rng, (B, CH) + PTS), int_grid(rng, B, PTS, VOL)
    x2, g2 = wide(rng, (B, CH) + PTS2), int_grid(rng, B, PTS2, VOL2)
    t = wide(rng, (B, CH) + PTS + (3,))
    with mode("fixed") as IP:
        for bound in (0, 3, 4, 5, 6):
            for ext in (0, 1):
                tag = (bound, ext)
                got = IP.grid_push(T(x), T(g), VOL, 1, bound, ext)
                want = T(FR.fixed("push", x, g, VOL, 1, bound, ext))
                assert bits_equal(got, want), ("linear",) + tag
                b, o, e = IP._opts(1, bound, ext)
                got = IP._fixed_export("grid_push3d_spline", T(x), T(g), VOL, b, o, e)
                assert bits_equal(got, want), ("spline {1,1,1}",) + tag
                got = IP.grid_push(T(x), T(g), VOL, [1, 0, 1], bound, ext)
                assert bits_equal(got, T(FR.fixed("push", x, g, VOL, [1, 0, 1], bound, ext))), ("padded",) + tag
                got = IP.grid_push(T(x[:1]), T(g), VOL, 1, bound, ext)
                assert bits_equal(got, T(FR.fixed("push", x[:1], g, VOL, 1, bound, ext))), ("Bi = 1",) + tag
                for o2 in (1, [1, 0]):
                    got = IP.grid_push(T(x2), T(g2), VOL2, o2, bound, ext)
                    assert bits_equal(got, T(FR.fixed("push", x2, g2, VOL2, o2, bound, ext))), ("2-D", o2) + tag
                for o3 in (1, [1, 0, 1]):
                    got = IP.grid_pushgrad(T(t), T(g), VOL, o3, bound, ext)
                    assert bits_equal(got, T(FR.fixed("pushgrad", t, g, VOL, o3, bound, ext))), ("pushgrad", o3) + tag
        got = IP.grid_pushgrad(T(t[:1]), T(g), VOL, 1, 3, 1)
        assert bits_equal(got, T(FR.fixed("pushgrad", t[:1], g, VOL, 1, 3, 1))), "pushgrad Bi = 1"
        got = IP.grid_pushgrad(T(t), T(g), VOL, 0, 3, 1)                  # all-nearest: zeros, written by the finalize pass
        assert bits_equal(got, torch.zeros_like(got))


# ------------------------------------------------------------------------------------------------------ 2. order independence
def _three_layouts(rng, pts, vol, tail=()):
    """The same points as (B, N, 1.., D), as (B, *pts, D) and under a random permutation of N, with their values"""
    D, N = len(vol), int(np.prod(pts))
    g = (rng.random((B, N, D)) * (np.array(vol) + 3.0) - 1.5).astype(np.float32)
    x = wide(rng, (B, CH, N) + tail)
    p = rng.permutation(N)
    one = (1,) * (D - 1)
    return [(x.reshape((B, CH, N) + one + tail), g.reshape((B, N) + one + (D,))),
            (x.reshape((B, CH) + pts + tail), g.reshape((B,) + pts + (D,))),
            (x[:, :, p].reshape((B, CH, N) + one + tail), g[:, p].reshape((B, N) + one + (D,)))]


@pytest.mark.parametrize("order", [1, 2, 3, [3, 1, 2]], ids=str)
def test_order_independence_3d(order):
    rng = np.random.default_rng(20)
    lay = _three_layouts(rng, PTS, VOL)
    with mode("fixed") as IP:
        for bound, ext in ((3, 1), (0, 0), (5, 2)):
            runs = [IP.grid_push(T(x), T(g), VOL, order, bound, ext) for x, g in lay + lay]
            assert all(bits_equal(r, runs[0]) for r in runs), (order, bound, ext)


@pytest.mark.parametrize("order", [0, 1, 2, 3, [2, 3]], ids=str)
def test_order_independence_2d(order):
    rng = np.random.default_rng(21)
    lay = _three_layouts(rng, PTS2, VOL2)
    with mode("fixed") as IP:
        for bound, ext in ((3, 1), (4, 0)):
            runs = [IP.grid_push(T(x), T(g), VOL2, order, bound, ext) for x, g in lay + lay]
            assert all(bits_equal(r, runs[0]) for r in runs), (order, bound, ext)


@pytest.mark.parametrize("order", [1, 2, 3, [3, 1, 2]], ids=str)
def test_order_independence_pushgrad(order):
    rng = np.random.default_rng(22)
    lay = _three_layouts(rng, PTS, VOL, tail=(3,))
    with mode("fixed") as IP:
        for bound, ext in ((3, 1), (0, 0)):
            runs = [IP.grid_pushgrad(T(x), T(g), VOL, order, bound, ext) for x, g in lay + lay]
            assert all(bits_equal(r, runs[0]) for r in runs), (order, bound, ext)


# -------------------------------------------------------------------------------------------------------- 3. contended, exact
def test_4096_points_on_one_voxel_sum_exactly():
    """One 2^20, one -2^20 and 4094 times 2^-4: the sum is 4094 * 2^-4 whatever the order; an fp32 running sum loses the
    small terms while the large one is in it."""
    rng = np.random.default_rng(30)
    n = 4096
    v = np.full(n, 2.0 ** -4, np.float32)
    i, j = rng.choice(n, 2, replace=False)
    v[i], v[j] = 2.0 ** 20, -2.0 ** 20
    at = (2, 3, 4)
    want = np.zeros(VOL, np.float32)
    want[at] = 4094 * 2.0 ** -4
    with mode("fixed") as IP:
        for shape in ((n, 1, 1), (16, 16, 16)):
            x = T(v.reshape((1, 1) + shape))
            g = T(np.tile(np.array(at, np.float32), shape + (1,))[None])
            for order in (0, 1, [1, 0, 1]):
                got = IP.grid_push(x, g, VOL, order, "dct2", True)
                assert bits_equal(got, T(want)[None, None]), (shape, order, got[0, 0][at].item())
        x2 = T(v.reshape(1, 1, 64, 64))
        g2 = T(np.tile(np.array(at[:2], np.float32), (64, 64, 1))[None])
        for order in (0, 1):
            got = IP.grid_push(x2, g2, VOL2, order, "dct2", True)
            assert got[0, 0, 2, 3].item() == 4094 * 2.0 ** -4 and got.abs().sum().item() == 4094 * 2.0 ** -4, order


# ----------------------------------------------------------------------------------------------------------------- 4. accuracy
ACC_ORDERS = [0, 1, 2, 3, [3, 1, 2], [0, 2, 3]]


@pytest.mark.parametrize("order", ACC_ORDERS, ids=str)
def test_accuracy_against_float64(order):
    rng = np.random.default_rng(40)
    x = rng.standard_normal((B, CH) + PTS).astype(np.float32)
    t = rng.standard_normal((B, CH) + PTS + (3,)).astype(np.float32)
    g = free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
    x2 = rng.standard_normal((B, CH) + PTS2).astype(np.float32)
    g2 = free_grid(rng, B, PTS2, VOL2, G2.redraw_near_jumps)
    o2 = order[:2] if isinstance(order, list) else order
    worst = {}
    with mode("fixed") as IP:
        for bound, ext in ((0, 0), (1, 1), (2, 2), (3, 1), (4, 0), (5, 1), (6, 2)):
            e = IP._extrap(ext)
            err = [close(IP.grid_push(T(x), T(g), VOL, order, bound, e), SR.push(x, g, VOL, order, bound, e), "push"),
                   close(IP.grid_push(T(x[:1]), T(g), VOL, order, bound, e), SR.push(x[:1], g, VOL, order, bound, e), "Bi=1"),
                   close(IP.grid_pushgrad(T(t), T(g), VOL, order, bound, e), HR.pushgrad(t, g, VOL, order, bound, e),
                         "pushgrad"),
                   close(IP.grid_push(T(x2), T(g2), VOL2, o2, bound, e), G2.push(x2, g2, VOL2, o2, bound, e), "push2d"),
                   close(IP.grid_count(T(g), VOL, order, bound, e), SR.push(np.ones((B, 1) + PTS), g, VOL, order, bound, e),
                         "count")]
            for name, v in zip(("push", "push Bi=1", "pushgrad", "push2d", "count"), err):
                worst[name] = max(worst.get(name, 0.0), v)
    print("order %s: max|hip - ref64| %s" % (order, {k: "%.2e" % v for k, v in worst.items()}))


# ---------------------------------------------------------------------------------------------------- 5. slice independence
def test_a_slice_does_not_depend_on_the_other_slices():
    rng = np.random.default_rng(50)
    x, g = rng.standard_normal((B, CH) + PTS).astype(np.float32), free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
    t = rng.standard_normal((B, CH) + PTS + (3,)).astype(np.float32)
    x[1] *= 2.0 ** 30
    x[0, 1] *= 2.0 ** 30
    t[1] *= 2.0 ** 30
    t[0, 2] *= 2.0 ** 30
    with mode("fixed") as IP:
        for order in (1, 3, [3, 1, 2]):
            whole = IP.grid_push(T(x), T(g), VOL, order, "dct2", True)
            wholeg = IP.grid_pushgrad(T(t), T(g), VOL, order, "dct2", True)
            for b in range(B):
                for c in range(CH):
                    alone = IP.grid_push(T(x[b:b + 1, c:c + 1]), T(g[b:b + 1]), VOL, order, "dct2", True)
                    assert bits_equal(whole[b, c], alone[0, 0]), ("push", order, b, c)
                    alone = IP.grid_pushgrad(T(t[b:b + 1, c:c + 1]), T(g[b:b + 1]), VOL, order, "dct2", True)
                    assert bits_equal(wholeg[b, c], alone[0, 0]), ("pushgrad", order, b, c)
        whole = IP.grid_push(T(x[:, :, :, :, 0]), T(g[:, :, :, 0, :2]), VOL2, 3, "dct2", True)
        alone = IP.grid_push(T(x[1:, 2:, :, :, 0]), T(g[1:, :, :, 0, :2]), VOL2, 3, "dct2", True)
        assert bits_equal(whole[1, 2], alone[0, 0])


# -------------------------------------------------------------------------------------------------------- 6. special inputs
@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")], ids=str)
def test_a_nonfinite_slice_is_nan_and_the_others_are_untouched(poison):
    rng = np.random.default_rng(60)
    x, g = rng.standard_normal((B, CH) + PTS).astype(np.float32), free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
    t = rng.standard_normal((B, CH) + PTS + (3,)).astype(np.float32)
    x[0, 2] = 0                                                           # and an all-zero slice
    t[0, 2] = 0
    xp, tp = x.copy(), t.copy()
    xp[1, 1, 4, 3, 0] = poison                                            # z = 0: in the 2-D slice of the volume too
    tp[1, 1, 4, 3, 0, 1] = poison
    with mode("fixed") as IP:
        calls = [("linear", lambda a: IP.grid_push(T(a), T(g), VOL, 1, "dct2", True), x, xp),
                 ("cubic", lambda a: IP.grid_push(T(a), T(g), VOL, 3, "zero", False), x, xp),
                 ("mixed", lambda a: IP.grid_push(T(a), T(g), VOL, [3, 1, 2], "dst2", True), x, xp),
                 ("2-D", lambda a: IP.grid_push(T(a[..., 0]), T(g[:, :, :, 0, :2]), VOL2, 2, "dct2", True), x, xp),
                 ("pushgrad", lambda a: IP.grid_pushgrad(T(a), T(g), VOL, 2, "dct2", True), t, tp),
                 ("pushgrad o0", lambda a: IP.grid_pushgrad(T(a), T(g), VOL, 0, "dct2", True), t, tp)]
        for name, f, clean, bad in calls:
            want, got = f(clean), f(bad)
            assert torch.isfinite(want).all(), name
            assert torch.isnan(got[1, 1]).all(), name
            for b in range(B):
                for c in range(CH):
                    if (b, c) != (1, 1):
                        assert bits_equal(got[b, c], want[b, c]), (name, b, c)
            assert bits_equal(got[0, 2], torch.zeros_like(got[0, 2])), name          # +0, not -0


def test_exports_refuse_a_short_workspace_and_write_nothing():
    from brainfm_amd import _lib as L
    rng = np.random.default_rng(61)
    x, g = T(rng.standard_normal((1, 1) + PTS).astype(np.float32)), T(free_grid(rng, 1, PTS, VOL, SR.redraw_near_jumps))
    lib = L.load()
    need = lib.bfm_grid_push_fixed_workspace(1, 1, int(np.prod(VOL)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1) + VOL, 7.0, device=DEV)
    bound, order = (C.c_int * 3)(3, 3, 3), (C.c_int * 3)(2, 2, 2)
    args = (L.ptr(x), 1, 1, *PTS, L.ptr(g), 1, *VOL, bound, order, 1, L.ptr(out))
    with mode("fixed"):
        assert lib.bfm_grid_push3d_spline_fixed(*args, L.ptr(ws), need - 1, L.stream_ptr()) == -1
        assert lib.bfm_grid_push3d_spline_fixed(*args, None, need, L.stream_ptr()) == -1
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        assert lib.bfm_grid_push3d_spline_fixed(*args, L.ptr(ws), need, L.stream_ptr()) == 0
        close(out, SR.push(x.cpu().numpy(), g.cpu().numpy(), VOL, 2, 3, 1), "out need not be zero on entry")


# ----------------------------------------------------------------------------------------------------------------- 7. autograd
def _pull_grad(IP, x, g, w, order):
    v = T(x).requires_grad_(True)
    (IP.grid_pull(v, T(g), order, "dct2", True) * T(w)).sum().backward()
    return v.grad


def _grad_grad(IP, x, g, w, order):
    v = T(x).requires_grad_(True)
    (IP.grid_grad(v, T(g), order, "dct2", True) * T(w)).sum().backward()
    return v.grad


@pytest.mark.parametrize("order", [1, 3, [3, 1, 2]], ids=str)
def test_backward_of_pull_and_grad_follow_the_mode(order):
    rng = np.random.default_rng(70)
    N = int(np.prod(PTS))
    x = rng.standard_normal((B, CH) + VOL).astype(np.float32)
    g = (rng.random((B, N, 1, 1, 3)) * (np.array(VOL) + 3.0) - 1.5).astype(np.float32)
    w, w3 = wide(rng, (B, CH, N, 1, 1)), wide(rng, (B, CH, N, 1, 1, 3))
    p = rng.permutation(N)
    with mode("atomic") as IP:
        a_pull, a_grad = _pull_grad(IP, x, g, w, order), _grad_grad(IP, x, g, w3, order)
    with mode("fixed") as IP:
        f_pull, f_grad = _pull_grad(IP, x, g, w, order), _grad_grad(IP, x, g, w3, order)
        close(f_pull, a_pull.cpu().numpy().astype(np.float64), "pull backward, fixed against atomic")
        close(f_grad, a_grad.cpu().numpy().astype(np.float64), "grad backward, fixed against atomic")
        assert bits_equal(_pull_grad(IP, x, g[:, p], w[:, :, p], order), f_pull)
        assert bits_equal(_grad_grad(IP, x, g[:, p], w3[:, :, p], order), f_grad)
        assert bits_equal(_pull_grad(IP, x, g.reshape((B,) + PTS + (3,)), w.reshape((B, CH) + PTS), order), f_pull)
    # 2-D pull
    x2 = rng.standard_normal((B, CH) + VOL2).astype(np.float32)
    g2 = (rng.random((B, 143, 1, 2)) * (np.array(VOL2) + 3.0) - 1.5).astype(np.float32)
    w2, p2 = wide(rng, (B, CH, 143, 1)), rng.permutation(143)
    o2 = order[:2] if isinstance(order, list) else order
    with mode("fixed") as IP:
        assert bits_equal(_pull_grad(IP, x2, g2[:, p2], w2[:, :, p2], o2), _pull_grad(IP, x2, g2, w2, o2))


def test_torch_deterministic_flag_alone_selects_the_fixed_route(monkeypatch):
    monkeypatch.delenv("BFM_PUSH_MODE", raising=False)
    rng = np.random.default_rng(71)
    x, g = wide(rng, (B, CH) + PTS), free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
    v = np.full(4096, 2.0 ** -4, np.float32)
    v[[7, 4000]] = 2.0 ** 20, -2.0 ** 20
    gv = T(np.tile(np.array((2, 3, 4), np.float32), (4096, 1, 1, 1))[None])
    was = torch.are_deterministic_algorithms_enabled()
    with mode("fixed") as IP:
        want = IP.grid_push(T(x), T(g), VOL, 3, "dct2", True)
    with mode(None) as IP:
        try:
            torch.use_deterministic_algorithms(True)
            assert IP.push_mode() == "fixed"
            got = IP.grid_push(T(x), T(g), VOL, 3, "dct2", True)
            one = IP.grid_push(T(v.reshape(1, 1, 4096, 1, 1)), gv, VOL, 0, "dct2", True)
        finally:
            torch.use_deterministic_algorithms(was)
        assert bits_equal(got, want)
        assert one[0, 0, 2, 3, 4].item() == 4094 * 2.0 ** -4          # the exact sum only the fixed route promises


# ------------------------------------------------------------------------------------------------------------------ 8. default
def test_default_mode_is_atomic(monkeypatch):
    monkeypatch.delenv("BFM_PUSH_MODE", raising=False)
    was = torch.are_deterministic_algorithms_enabled()
    with mode(None) as IP:
        try:
            torch.use_deterministic_algorithms(False)
            assert IP.push_mode() == "atomic"
            rng = np.random.default_rng(80)
            x, g = rng.standard_normal((B, CH) + PTS).astype(np.float32), free_grid(rng, B, PTS, VOL, SR.redraw_near_jumps)
            close(IP.grid_push(T(x), T(g), VOL, 3, "dct2", True), SR.push(x, g, VOL, 3, 3, 1), "atomic push")
        finally:
            torch.use_deterministic_algorithms(was)
