"""The fixed-point accumulation format of interpol's scatter kernels on the host: the int64 emulation the GPU tests compare
bits against (tests/push_fixed_refs.py), the library's `bits` helper and the resolution of the push mode.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import push_fixed_refs as FR


def _contributions(rng, n, nvox, m_exp):
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(m_exp - 30, m_exp, n)).astype(np.float32)
    return rng.integers(0, nvox, n), c


def test_the_sum_does_not_depend_on_the_order_of_the_contributions():
    rng = np.random.default_rng(0)
    nvox, n = 37, 5000
    lin, c = _contributions(rng, n, nvox, 12)
    m = np.abs(c).max()
    bits = FR.bits_for(n, [0], 1)
    want = FR.fixed_sum(nvox, lin, c, m, bits)
    k = FR.slice_k(m, bits)
    q = FR.quantize(c, k)
    for _ in range(5):
        p = rng.permutation(n)
        assert np.array_equal(FR.fixed_sum(nvox, lin[p], c[p], m, bits).view(np.uint32), want.view(np.uint32))
        # one contribution at a time, and in two halves summed apart: wrapping int64 additions in another association
        acc = np.zeros(nvox, np.int64)
        for i in p[: n // 2]:
            acc[lin[i]] += q[i]
        acc = acc + FR.accumulate(nvox, lin[p[n // 2:]], q[p[n // 2:]])
        assert np.array_equal(FR.finalize(acc, k).view(np.uint32), want.view(np.uint32))
    # a float32 running sum of the same contributions does depend on it: the property is the format's, not the data's
    sums = set()
    for _ in range(5):
        p = rng.permutation(n)
        acc = np.zeros(nvox, np.float32)
        np.add.at(acc, lin[p], c[p])
        sums.add(acc.tobytes())
    assert len(sums) > 1


@pytest.mark.parametrize("bits", [10, 28, 40])
@pytest.mark.parametrize("G", [1, 3])
def test_no_overflow_when_every_contribution_is_as_large_as_it_can_be(bits, G):
    """P * T * G <= 2^bits contributions of +-G * m: the sum of |q| stays below 2^63 for every m, in exact integers."""
    tiny = np.float32(1e-45)
    below = lambda x: np.nextafter(np.float32(x), np.float32(0))
    for m in (np.float32(1), below(1), below(2.0 ** 127), below(2.0 ** 126), np.float32(2.0 ** -126), tiny,
              np.float32(3e-41), np.float32(1.75), np.float32(np.finfo(np.float32).max)):
        k = FR.slice_k(m, bits, G)
        if G > 1 and m >= 2.0 ** 126:
            assert k is None                  # G * m need not be a finite float: the slice is NaN
            continue
        largest = np.float32(G) * m           # fl(G * m): the largest value a rounded contribution can take
        q = int(FR.quantize(largest, k))
        n = (1 << bits) // G                  # P * T
        assert q > 0 and n * q < 1 << 63, (m, k, q)
        assert int(FR.quantize(-largest, k)) == -q
        # and int64 holds a sum that alternates in sign, or does not, without wrapping
        some = min(n, 1 << 16)
        acc = FR.accumulate(1, np.zeros(some, np.int64), np.full(some, q, np.int64))
        assert int(acc[0]) == some * q


@pytest.mark.parametrize("m_exp", [-20, 0, 20])
def test_the_sum_is_the_float64_sum_to_half_a_unit_per_contribution_and_one_rounding(m_exp):
    rng = np.random.default_rng(1)
    nvox, n = 11, 4096
    lin, c = _contributions(rng, n, nvox, m_exp)
    m = np.abs(c).max()
    for bits in (FR.bits_for(n, [0], 1), 28, 40):
        k = FR.slice_k(m, bits)
        got = FR.fixed_sum(nvox, lin, c, m, bits).astype(np.float64)
        ref = np.zeros(nvox)
        np.add.at(ref, lin, c.astype(np.float64))
        n_v = np.bincount(lin, minlength=nvox)
        bound = n_v * 2.0 ** -(k + 1) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) / 2
        assert (np.abs(got - ref) <= bound).all(), (bits, np.abs(got - ref).max(), bound.min())


def test_special_slices():
    lin, c = np.array([0, 1, 1]), np.array([1.5, -2.0, 0.25], np.float32)
    assert np.isnan(FR.fixed_sum(3, lin, c, np.float32("nan"), 10)).all()
    assert np.isnan(FR.fixed_sum(3, lin, c, np.float32("inf"), 10)).all()
    z = FR.fixed_sum(3, lin, np.zeros(3, np.float32), np.float32(0), 10)
    assert np.array_equal(z.view(np.uint32), np.zeros(3, np.uint32))       # +0, not -0
    assert np.array_equal(FR.fixed_sum(3, lin, c, np.float32(2), 10), np.array([1.5, -1.75, 0], np.float32))
    assert FR.slice_k(np.float32(1), 10) == 62 - 10 - 1 and FR.slice_k(np.float32(0.75), 10) == 62 - 10
    assert FR.slice_k(np.float32(1e-45), 40) == 62 - 40 + 148               # the smallest denormal is 2^-149 < 2^-148


BITS_TABLE = [                                # P, orders, G -> bits
    (1, [0, 0, 0], 1, 0),
    (2, [0, 0, 0], 1, 1),
    (9 * 8 * 7, [0, 0, 0], 1, 9),
    (9 * 8 * 7, [3, 1, 2], 1, 14),
    (9 * 8 * 7, [1, 1, 1], 3, 14),
    (4096, [1, 1, 1], 1, 15),
    (4096, [1, 1, 1], 3, 17),
    (4097, [1, 1, 1], 1, 16),
    (11 * 13, [2, 3], 1, 11),
    (2048 * 2048, [3, 3], 1, 26),
    (160 ** 3, [3, 3, 3], 1, 28),
    (160 ** 3, [3, 3, 3], 3, 30),
    (1 << 34, [3, 3, 3], 1, 40),
    ((1 << 34) + 1, [3, 3, 3], 1, None),
    (1 << 35, [3, 3, 3], 1, None),
    (1 << 34, [3, 3, 3], 3, None),
    (1 << 40, [0, 0, 0], 1, 40),
    ((1 << 40) + 1, [0, 0, 0], 1, None),
    (1 << 62, [3, 3, 3], 3, None),
]


def test_bits_helper_of_the_library_and_of_the_emulation():
    from brainfm_amd import _lib as L
    lib = L.load()
    for P, orders, G, want in BITS_TABLE:
        arr = (C.c_int * 3)(*(orders + [0])[:3])
        got = lib.bfm_grid_push_fixed_bits(P, arr, len(orders), G)
        assert got == (-1 if want is None else want), (P, orders, G, got)
        if want is None:
            with pytest.raises(ValueError):
                FR.bits_for(P, orders, G)
        else:
            assert FR.bits_for(P, orders, G) == want
    ok = (C.c_int * 3)(1, 1, 1)
    for args in ((0, ok, 3, 1), (-5, ok, 3, 1), (8, None, 3, 1), (8, ok, 0, 1), (8, ok, 4, 1), (8, ok, 3, 0), (8, ok, 3, 4),
                 (8, (C.c_int * 3)(1, 4, 1), 3, 1), (8, (C.c_int * 3)(-1, 1, 1), 3, 1)):
        assert lib.bfm_grid_push_fixed_bits(*args) == -1, args[0:1] + args[2:]


def test_workspace_size():
    from brainfm_amd import _lib as L
    lib = L.load()
    for B, Cn, nvox in ((1, 1, 1), (2, 3, 210), (1, 1, 160 ** 3), (4, 2, 2048 * 2048)):
        got = lib.bfm_grid_push_fixed_workspace(B, Cn, nvox)
        assert got >= B * Cn * (nvox * 8 + 8) and got % 256 == 0 and got <= B * Cn * (nvox * 8 + 8) + 3 * 256
    assert lib.bfm_grid_push_fixed_workspace(0, 1, 1) == 0 and lib.bfm_grid_push_fixed_workspace(1, 1, 0) == 0


def test_mode_resolution(monkeypatch):
    """set_push_mode, then BFM_PUSH_MODE, then torch's deterministic flag, then 'atomic'; resolved at every call."""
    import torch
    from brainfm_amd import interpol as IP
    monkeypatch.delenv("BFM_PUSH_MODE", raising=False)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        IP.set_push_mode(None)
        torch.use_deterministic_algorithms(False)
        assert IP.push_mode() == "atomic"
        torch.use_deterministic_algorithms(True)
        assert IP.push_mode() == "fixed"
        monkeypatch.setenv("BFM_PUSH_MODE", "atomic")
        assert IP.push_mode() == "atomic"                # the environment goes before the torch flag
        torch.use_deterministic_algorithms(False)
        monkeypatch.setenv("BFM_PUSH_MODE", "fixed")
        assert IP.push_mode() == "fixed"
        IP.set_push_mode("atomic")
        assert IP.push_mode() == "atomic"                # the override goes before the environment
        IP.set_push_mode("fixed")
        monkeypatch.setenv("BFM_PUSH_MODE", "atomic")
        assert IP.push_mode() == "fixed"
        IP.set_push_mode(None)
        assert IP.push_mode() == "atomic"                # cleared: the environment again
        monkeypatch.setenv("BFM_PUSH_MODE", "sorted")
        with pytest.raises(ValueError):
            IP.push_mode()
        monkeypatch.delenv("BFM_PUSH_MODE")
        for bad in ("Fixed", "", 0, True, "float"):
            with pytest.raises(ValueError):
                IP.set_push_mode(bad)
        assert IP.push_mode() == "atomic"                # a refused mode changes nothing
    finally:
        IP.set_push_mode(None)
        torch.use_deterministic_algorithms(was)


def test_contributions_are_the_float64_reference_where_the_weights_are_exact():
    """The fp32 restatement the bit tests rest on, against the float64 references on the same exact-weight cases."""
    import grid2d_refs as G2
    import grid_hess_refs as HR
    import spline_grid_refs as SR
    rng = np.random.default_rng(2)
    shape, pts = (5, 6, 7), (4, 3, 5)
    x = rng.standard_normal((2, 3) + pts).astype(np.float32)
    g = (rng.random((2,) + pts + (3,)) * 9 - 2).astype(np.float32)
    SR.redraw_near_jumps(g, shape, rng)
    gi = rng.integers(-2, 9, (2,) + pts + (3,)).astype(np.float32)
    t = rng.standard_normal((2, 3) + pts + (3,)).astype(np.float32)

    def dense(cons, B, Cn, nvox):
        out = np.zeros((B, Cn, nvox))
        for (b, ch), (lin, c) in cons.items():
            np.add.at(out[b, ch], lin, c.astype(np.float64))
        return out

    for bound in range(7):
        for ext in (0, 1, 2):
            got = dense(FR.contributions("push", x, g, shape, 0, bound, ext), 2, 3, 210)
            assert np.allclose(got.reshape(2, 3, *shape), SR.push(x, g, shape, 0, bound, ext), atol=1e-5)
            got = dense(FR.contributions("push", x, gi, shape, 1, bound, ext), 2, 3, 210)
            assert np.allclose(got.reshape(2, 3, *shape), SR.push(x, gi, shape, 1, bound, ext), atol=1e-5)
            got = dense(FR.contributions("pushgrad", t, gi, shape, 1, bound, ext), 2, 3, 210)
            assert np.allclose(got.reshape(2, 3, *shape), HR.pushgrad(t, gi, shape, 1, bound, ext), atol=1e-5)
    g2 = (rng.random((2, 4, 5, 2)) * 9 - 2).astype(np.float32)
    G2.redraw_near_jumps(g2, (6, 7), rng)
    x2 = rng.standard_normal((2, 3, 4, 5)).astype(np.float32)
    got = dense(FR.contributions("push", x2, g2, (6, 7), 0, 4, 0), 2, 3, 42)
    assert np.allclose(got.reshape(2, 3, 6, 7), G2.push(x2, g2, (6, 7), 0, 4, 0), atol=1e-5)
    with pytest.raises(AssertionError):
        FR.contributions("push", x, g, shape, 1, 0, 1)                     # weights that round are refused
