"""The references, bounds and case list of tests/tail_refs.py without a GPU.

Pinning: every function reproduces tests/golden/tail_edges.npz -- the reference's own F.normalize, TaskHead final convs,
SegProcessor / DistProcessor / PatholProcessor and get_postprocessor on the same inputs (tests/golden/make_golden_tail.py),
and torch.softmax / torch.argmax on the non-finite rows.  Routes: bfm_tail_route is host arithmetic (the library loads
without a device) and equals tail_refs.tail_route.  The split emulation equals a second, independent spelling.
Discrimination: tail_refs.simulate, an fp32 model of the kernel, passes check_stage_a / check_stage_b, and each named
mistake -- and a dropped bias -- fails them on the case list.  A mistake that no case catches means a case is missing."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from conftest import load_npz
from conv_forward_refs import prescale_exp, split_hi_lo
import tail_refs as T

F32, F64 = np.float32, np.float64


def _gold():
    return load_npz("tail_edges.npz")


# ------------------------------------------------------------------------------------------------------------ routes
def test_route_table_of_the_library_equals_the_reference_and_the_case_list_reaches_every_route():
    from brainfm_amd import _lib as L
    lib = L.load()

    def route(c, n_out, n_seg, unit, wmax):
        d = L.TailDesc(n_out, c, None, None, None, None, 0, n_seg, None, 0, 0, 3.0, unit, -1, -1, 0, wmax, 0)
        return lib.bfm_tail_route(C.byref(d))

    assert lib.bfm_tail_route(None) == -1
    for c, n_out, n_seg, unit, wmax in itertools.product((8, 16, 24, 32, 48, 64), (0, 1, 27, 32, 33, 64, 65, 69, 96),
                                                         (0, 18, 20, 56), (0, 1), (0.0, 1e-30, 0.7, float("inf"), float("nan"))):
        assert route(c, n_out, n_seg, unit, wmax) == T.tail_route(c, n_out, n_seg, unit, wmax), (c, n_out, n_seg, unit, wmax)
    assert route(64, 69, 56, 1, 0.5) == 2 and route(64, 64, 56, 1, 0.5) == 1 and route(64, 96, 56, 1, 0.5) == 2
    assert route(64, 29, 18, 1, 0.5) == 3 and route(64, 27, 18, 1, 0.5) == 3 and route(64, 33, 18, 1, 0.5) == 1
    assert route(64, 69, 56, 0, 0.5) == 0 and route(64, 69, 56, 1, 0.0) == 0 and route(24, 69, 56, 1, 0.5) == 0
    assert route(8, 5, 0, 1, 0.5) == 0 and route(16, 5, 0, 1, 0.5) == 1
    seen = {T.tail_route(c, n, 0, u, 1.0) for c, n, u, _, _ in T.stage_a_grid()}
    assert seen == {0, 1}                                   # the grid has no segmentation: routes 2 and 3 are the head sets
    sets = {name: T.head_spec(g) for name, g in T.HEAD_SETS.items()}
    assert T.tail_route(64, 69, sets["full69"]["n_seg"], 1, 1.0) == 2
    assert {T.tail_route(64, sets[k]["n_out"], sets[k]["n_seg"], 1, 1.0) for k in ("left29", "left27")} == {3}


def test_stage_a_grid_is_a_pairwise_cover():
    g = T.stage_a_grid()
    vals = (T.GRID_C, T.GRID_N, (0, 1), T.GRID_V)
    for i, j in itertools.combinations(range(4), 2):
        assert {(c[i], c[j]) for c in g} == set(itertools.product(vals[i], vals[j])), (i, j)
    assert all(T.tail_route(c, n, 0, 1, 1.0) == 0 for c, n, u, _, _ in g if c in (8, 24))


# ------------------------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("name", T.GOLDEN_SETS)
def test_references_reproduce_the_reference_implementation(name):
    g = _gold()
    spec, x, W, b, inp = T.golden_case(name)
    fn, raw, maps, seg, label = (g["%s/%s" % (name, k)] for k in ("fn", "raw", "maps", "seg", "label"))
    # F.normalize and the head convs in fp32 against the float64 definitions: a few roundings / a chain of 64
    u, fb = T.feat_norm_bound(x)
    assert (np.abs(fn - u) <= fb).all()
    t, _ = T.stage_a_true(x, W, b, True)
    absum = np.abs(u) @ np.abs(W.astype(F64)).T
    # (the reference's convolution may start its chain from the bias: every one of its 64 roundings then sees |b| too)
    assert (np.abs(raw - t) <= (64 + T.NORM_ROUNDINGS) * T.EPS * (absum + np.abs(b)) + T.EPS * np.abs(t)).all()
    assert np.abs(raw[3] - b).max() == 0                    # the all-zero row: the bias alone
    # every processor, as a function of the reference's own logits, under the bounds the kernels are held to
    out = T.check_stage_b(raw, maps, seg, label, None, spec, inp, ulp_limit={"ulp_exp": 2.0, "ulp_sigmoid": 2.0})
    assert out["near"] == 0
    kinds = [r[0] for r in T.processors64(raw, spec, inp)[0]]
    assert "none" not in kinds and {"bits", "ulp_exp", "abs"} <= set(kinds)
    md = spec["max_dist"]
    d = raw[:, spec["dist_first"]:spec["dist_first"] + spec["n_dist"]]
    assert (d > md).any() and (d < -md).any() and (np.abs(d) < md).any()        # the clamp is active and inactive


def test_non_finite_rows_follow_torch():
    g = _gold()
    z = T.nonfinite_rows()
    p_t, a_t = g["nonfinite/softmax"], g["nonfinite/argmax"]
    assert np.array_equal(p_t, torch.softmax(torch.from_numpy(z), 1).numpy(), equal_nan=True)
    p = T.softmax64(z)
    assert np.array_equal(np.isnan(p), np.isnan(p_t)) and np.allclose(p[~np.isnan(p)], p_t[~np.isnan(p_t)], rtol=1e-6, atol=0)
    assert list(np.isnan(p_t).all(1)) == [True, True, True, True, False, False, False, True]
    # the tail's rule (first maximum of the probabilities, 0 for a NaN row) and argmax_rule (a NaN wins only from column 0)
    p32 = p.astype(F32)
    first = np.where(np.isnan(p32).any(1), 0, np.argmax(np.where(np.isnan(p32), -1, p32), 1))
    assert np.array_equal(first, a_t) and np.array_equal(T.argmax_rule(p32), a_t)
    assert list(a_t) == [0, 0, 0, 0, 3, 2, 1, 0]
    # on the logits themselves torch.argmax picks the NaN, the documented rule does not unless it is in column 0
    zz = np.array([[0.5, np.nan, 1.0, 0.0], [np.nan, 0.5, 1.0, 0.0], [np.nan] * 4, [1.0, 2.0, 2.0, 0.0]], F32)
    assert list(torch.argmax(torch.from_numpy(zz), 1).numpy()) == [1, 0, 0, 1] and list(T.argmax_rule(zz)) == [2, 0, 0, 1]
    assert list(T.argmax_rule(zz, [7, 5, 3, 1])) == [3, 7, 7, 5]


# ------------------------------------------------------------------------------------------------------------ emulation
def test_rtz16_equals_a_rounded_cast_stepped_toward_zero():
    rs = np.random.RandomState(0)
    v = np.concatenate([rs.randn(4000) * 10.0 ** rs.randint(-9, 5, 4000), [0.0, -0.0, 16384.0, 65504.0, 65519.0, 1e5, -1e5,
                                                                              2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 6e-8]]).astype(F32)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    h = np.where(np.isinf(h), np.copysign(np.float16(65504), h), h).astype(np.float16)
    over = np.abs(h.astype(F64)) > np.abs(v.astype(F64))
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    assert np.array_equal(T.rtz16(v), h.astype(F64))


@pytest.mark.parametrize("c,n_out,wscale", [(16, 5, 1.0), (64, 69, 2.0 ** 10), (48, 33, 2.0 ** -20)])
def test_split_emulation_equals_a_second_spelling(c, n_out, wscale):
    """Element by element: (hi + lo)(whi + wlo) - lo * wlo summed over the channels, the feature halves by a rounded cast
    stepped toward zero, the weight halves by conv_forward_refs.split_hi_lo (torch .half())."""
    x, W, b = T.operands(c, n_out, 37, 5, wscale=wscale)
    wmax = float(np.abs(W).max())
    e, absum = T.stage_a_emulation(x, W, b, 1, wmax)
    wexp = prescale_exp(wmax)
    nrm = np.sqrt((x.astype(F64) ** 2).sum(1))
    a = (x * (T.inv_norm32(x) * F32(16384))[:, None])
    assert np.allclose(a / 16384.0, x / nrm[:, None], rtol=1e-5)

    def trunc16(v):
        h = v.astype(np.float16)
        return np.where(np.abs(h.astype(F64)) > np.abs(v.astype(F64)), np.nextafter(h, np.float16(0)), h).astype(F32)
    hi = trunc16(a)
    lo = trunc16(a - hi)
    whi, wlo = (t.numpy() for t in split_hi_lo(torch.from_numpy(W), wexp))
    full = np.einsum("vk,ok->vo", hi.astype(F64) + lo, whi + wlo) - np.einsum("vk,ok->vo", lo.astype(F64), wlo)
    e2 = full * 2.0 ** -(wexp + 14) + b
    assert np.abs(e - e2).max() <= 1e-12 * max(1.0, np.abs(e).max())
    assert np.allclose(absum, np.abs(x / nrm[:, None]) @ np.abs(W.astype(F64)).T, rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------ mistakes
def _sim_checks(x, W, b, spec, unit, wmax, inp=None, gate=False, mistake=None, random_case=False):
    s = T.simulate(x, W, b, spec, unit, wmax, inp, gate, mistake)
    T.check_stage_a(s["raw"], x, W, b, unit, wmax)
    keep = T.gate_keep(inp, len(x)) if gate else None
    T.check_stage_b(s["raw"], s["maps"], s["seg"], s["label"], s["label"], spec, inp, keep, ulp_limit={"ulp_exp": 1.0, "ulp_sigmoid": 1.0},
                    random_case=random_case)


def _fails(*a, **k):
    with pytest.raises(AssertionError):
        _sim_checks(*a, **k)


def test_simulator_passes_and_stage_a_mistakes_fail_on_the_grid():
    caught = {m: 0 for m in ("swap_halves", "drop_kstep", "lost_lo", "bias_first")}
    for c, n_out, unit, nvox, seed in T.stage_a_grid()[::3]:
        x, W, b = T.operands(c, n_out, nvox, seed)
        spec = T.head_spec([(T.PLAIN, n_out)])
        wmax = float(np.abs(W).max())
        _sim_checks(x, W, b, spec, unit, wmax)
        split = T.tail_route(c, n_out, 0, unit, wmax) != 0
        for m in caught:
            if m in ("lost_lo", "bias_first") and not split:
                continue                                    # the fp32 chain has neither a lo pass nor a de-scale
            _fails(x, W, b, spec, unit, wmax, mistake=m)
            caught[m] += 1
        # a dropped bias: the biases are as large as the logits
        raw = T.simulate(x, W, np.zeros_like(b), spec, unit, wmax)["raw"]
        with pytest.raises(AssertionError):
            T.check_stage_a(raw, x, W, b, unit, wmax)
    assert min(caught.values()) >= 5, caught


def _set_case(name, nvox, seed, wscale=4.0, c=64):
    spec = T.head_spec(T.HEAD_SETS[name])
    x, W, b = T.operands(c, spec["n_out"], nvox, seed, wscale=wscale)
    return spec, x, W, b, float(np.abs(W).max()), T.image_input(nvox, seed)


@pytest.mark.parametrize("name", sorted(T.HEAD_SETS))
def test_simulator_passes_on_every_head_set(name):
    spec, x, W, b, wmax, inp = _set_case(name, 130, 3, c=16 if name == "big" else 64)
    for unit in (0, 1):
        _sim_checks(x, W, b, spec, unit, wmax, inp, random_case=True)


@pytest.mark.parametrize("mistake,name", [("lp_lw", "dist2"), ("lp_lw", "dist4"), ("lp_lw", "full69"), ("clamp_ct", "full69"),
                                          ("clamp_ct", "seg70"), ("lut_offset", "seg20_first7"), ("lut_offset", "full69"),
                                          ("high_res_slot", "sr2"), ("high_res_slot", "left29"), ("high_res_slot", "uncert")])
def test_processor_mistakes_fail(mistake, name):
    spec, x, W, b, wmax, inp = _set_case(name, 130, 3)
    _sim_checks(x, W, b, spec, 1, wmax, inp)
    _fails(x, W, b, spec, 1, wmax, inp, mistake=mistake)


def test_last_maximum_argmax_fails_on_the_planted_ties():
    for name, pos in (("full69", 0), ("full69", 30), ("left29", 16), ("seg70", 68), ("seg20_first7", 5)):
        spec = T.head_spec(T.HEAD_SETS[name])
        W, b = T.planted_rows(spec["n_seg"], spec["seg_first"], spec["n_out"], 64, 9, pos)
        x = T.operands(64, spec["n_out"], 70, 11)[0]
        wmax = float(np.abs(W).max())
        b0 = T.planted_bias(b, spec["seg_first"], pos, 0.0)
        s = T.simulate(x, W, b0, spec, 1, wmax)
        z = s["raw"][:, spec["seg_first"]:spec["seg_first"] + spec["n_seg"]]
        assert (z[:, pos] == z[:, pos + 1]).all() and (np.argmax(z, 1) == pos).all()      # an exact tie on top, everywhere
        _sim_checks(x, W, b0, spec, 1, wmax)
        _fails(x, W, b0, spec, 1, wmax, mistake="last_max")
        for gap in T.GAPS[1:]:                              # the second of the pair leads by the gap, to within a rounding
            z = T.simulate(x, W, T.planted_bias(b, spec["seg_first"], pos, gap), spec, 1, wmax)["raw"]
            z = z[:, spec["seg_first"]:spec["seg_first"] + spec["n_seg"]].astype(F64)
            want = 2.0 ** -22 if gap == "ulp" else gap
            assert (np.abs((z[:, pos + 1] - z[:, pos]) - want) <= 2.0 ** -21).all(), (name, gap)


def test_gate_and_slot_mistakes_fail():
    """Groups of four: tail_refs.BIG_NVOX puts chunks into slot 1, into slots 1..3 and into a second lap.  The input is
    zero on a pattern of chunks in which the chunk one slot further on (cstride chunks away) is never in the same state as
    a zero chunk, and distinct elsewhere: a slot off by one moves both the gate's decision and the high_res addend."""
    spec = T.head_spec(T.HEAD_SETS["big"])
    laps = [T.chunk_slot(n) for n in T.BIG_NVOX]
    assert [s[2] for s in laps] == [2048] * 3
    assert set(laps[0][0]) == {0, 1} and set(laps[1][0]) == {0, 1, 2, 3} and set(laps[1][1]) == {0}
    assert set(laps[2][1]) == {0, 1} and set(laps[2][0][laps[2][1] == 1]) == {0}
    n, cstride = T.BIG_NVOX[1], 2048
    x, W, b = T.operands(16, spec["n_out"], n, 21)
    wmax = float(np.abs(W).max())
    inp = T.slot_pattern_input(n)
    z = (inp[:n // 64 * 64].reshape(-1, 64) == 0).all(1)
    assert (z[:-cstride] != z[cstride:]).mean() > 0.6 and not (z[:-cstride] & z[cstride:]).any()
    for gate in (False, True):
        _sim_checks(x, W, b, spec, 1, wmax, inp, gate=gate)
        _fails(x, W, b, spec, 1, wmax, inp, gate=gate, mistake="ivq_slot")
    # the gate is on ALL zero: one non-zero voxel at lane 0, lane 63 or in the partial last chunk keeps the chunk
    spec, x, W, b, wmax, _ = _set_case("sr2", 64 * 5 + 9, 4)
    inp = T.gate_input(len(x))
    keep = T.gate_keep(inp, len(x))
    assert list(keep[::64]) == [True, False, False, True, False, False]
    _sim_checks(x, W, b, spec, 1, wmax, inp, gate=True)
    _fails(x, W, b, spec, 1, wmax, inp, gate=True, mistake="gate_any")


# ------------------------------------------------------------------------------------------------------------ per-voxel
def test_per_voxel_references_follow_torch():
    x = torch.from_numpy(T.ew_operand(1027, 1))
    y = torch.from_numpy(T.ew_operand(1027, 2)[::-1].copy())
    a, b = float(T.EW_A), float(T.EW_B)
    want = {"AFFINE": x * a + b, "CLAMP_MIN": torch.where(x < a, torch.tensor(a), x), "DIV": x / a,
            "NONZERO": (x != 0).float(), "SUB_DIV": (x - a) / b, "GE": (x >= a).float(), "NAN_TO_NUM": torch.nan_to_num(x)}
    for name, w in want.items():
        kind, r = T.ew_unary_ref(T.EW_UNARY.index(name), x.numpy())
        assert kind == "bits" and T.bits_equal(r, w.numpy()), name
    kind, r = T.ew_unary_ref(T.EW_UNARY.index("CLAMP"), x.numpy())
    fin = ~torch.isnan(x).numpy()
    assert T.bits_equal(r[fin], torch.clamp(x, a, b).numpy()[fin]) and (r[~fin] == T.EW_A).all()     # fmaxf(NaN, a) = a
    want = {"ADD": x + y, "MUL": x * y, "AXPY": x + a * y, "DIV2": x / y, "ZERO_WHERE_ZERO": torch.where(y == 0, torch.zeros_like(x), x),
            "AXPY_CLAMP0": torch.where(x + a * y < 0, torch.zeros_like(x), x + a * y)}
    for name, w in want.items():
        kind, r = T.ew_binary_ref(T.EW_BINARY.index(name), x.numpy(), y.numpy())
        assert kind == "bits" and T.bits_equal(r, w.numpy()), name
    for op in ("EXP", "SIGMOID"):
        kind, r = T.ew_unary_ref(T.EW_UNARY.index(op), x.numpy())
        w = (torch.exp(x) if op == "EXP" else torch.sigmoid(x)).numpy()
        fin = np.isfinite(r) & (r > 1e-37)
        assert kind == "ulp" and T.ulps32(w[fin], r[fin]).max() <= 2.0, op
    yv = np.random.RandomState(3).randn(50, 12).astype(F32)
    bias = np.random.RandomState(4).randn(12).astype(F32)
    r, bound = T.bias_lrelu_ref(yv, bias, 0.2)
    w = torch.nn.functional.leaky_relu(torch.from_numpy(yv) + torch.from_numpy(bias), 0.2).numpy()
    assert T.bits_equal(r, w) and bound == np.abs(w).max()
    mask = (np.arange(50) % 3 != 0).astype(F32)
    r, bound = T.bias_lrelu_ref(yv, bias, 0.2, mask)
    assert T.bits_equal(r[::3], yv[::3]) and T.bits_equal(r[1::3], w[1::3]) and bound == np.abs(w[mask != 0]).max()
