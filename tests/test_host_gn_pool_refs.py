"""tests/gn_pool_refs.py against the reference implementation, without a GPU: gn_truth against torch.nn.functional.group_norm
in float64 on the materialised concat and against F.interpolate(mode='nearest') for the replication counts; pool_truth is
torch's max_pool3d; pool_rows_as_coded against the float64 sums; the two host-only route exports (bfm_gn_stats_plan,
bfm_gn_stats_rows_route: host arithmetic, the library loads without a device) against the rules written in
include/brainfm_hip.h; every derived bound non-vacuous on its case list; and each named mistake failing the checks that
tests/test_gpu_gn_pool.py applies to the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import gn_pool_refs as R

F32, F64, LD = np.float32, np.float64, np.longdouble
Fn = torch.nn.functional


def _lib():
    from brainfm_amd import _lib as L
    return L.load()


def _cat_cases():
    return [(lo, hi, ca, cb, g) for lo, hi in R.UPSAMPLES for ca, cb, g in R.GN_CAT_CHANNELS] + [R.GN_CAT_UNROLLED]


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", _cat_cases()[:12] + [None], ids=str)
def test_gn_truth_is_torch_group_norm_in_float64(case):
    if case is None:
        A, gamma, beta = R.tensor_inputs((12, R.SHORT, 3, 0, "randn", 0))
        B, maps, G = None, None, 3
    else:
        lo, hi, ca, cb, G = case
        A, B, gamma, beta = R.cat_inputs(lo, hi, ca, cb, G)
        maps = R.up_maps(lo, hi)
    t = R.gn_truth(A, B, maps, gamma, beta, G)
    x = torch.from_numpy(R.materialise(A, B, maps)).double().permute(3, 0, 1, 2)[None]
    y = Fn.group_norm(x, G, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), float(F32(R.EPS)))
    y = y[0].permute(1, 2, 3, 0).numpy()
    mine = R.materialise(A, B, maps).astype(F64) * t["scale"] + t["shift"]
    assert np.abs(mine - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    cpg = y.shape[-1] // G
    assert np.allclose(np.abs(y).reshape(-1, G, cpg).max((0, 2)), t["bound"], rtol=1e-12, atol=0)
    live = t["scale"] != 0                       # (y - shift) / scale gives the input back, where gamma is not 0
    xh = (y[..., live] - t["shift"][live]) / t["scale"][live]
    assert np.abs(xh - R.materialise(A, B, maps).astype(F64)[..., live]).max() <= 1e-10
    x64 = R.materialise(A, B, maps).astype(F64).reshape(-1, G, cpg)
    assert np.allclose(x64.mean((0, 2)), t["mean"], rtol=1e-12, atol=1e-14) and np.allclose(x64.var((0, 2)), t["var"], rtol=1e-12)


@pytest.mark.parametrize("lo, hi", R.UPSAMPLES + [((3, 5, 7), (7, 11, 20)), ((4, 4, 4), (8, 8, 8))])
def test_replication_is_interpolate_nearest(lo, hi):
    from brainfm_amd.engine import nearest_index_map
    maps = R.up_maps(lo, hi)
    for a in range(3):
        assert (maps[a] == nearest_index_map(lo[a], hi[a])).all()
    B = R.field("randn", tuple(lo) + (3,), "nearest")
    up = Fn.interpolate(torch.from_numpy(B).permute(3, 0, 1, 2)[None], size=hi, mode="nearest")[0].permute(1, 2, 3, 0).numpy()
    assert R.bits_equal(R.materialise(np.zeros(tuple(hi) + (0,), F32), B, maps), up)
    reps = R.rep_counts(maps, lo)
    w = reps[0][:, None, None] * reps[1][None, :, None] * reps[2][None, None, :]
    assert w.sum() == np.prod(hi)
    assert np.allclose((B.astype(F64) * w[..., None]).sum((0, 1, 2)), up.astype(F64).sum((0, 1, 2)), rtol=1e-13)


def test_fma32_is_the_correctly_rounded_fused_operation():
    from fractions import Fraction
    g = np.random.default_rng(5)
    a, b = g.standard_normal(4000).astype(F32), g.standard_normal(4000).astype(F32)
    c = (-(a.astype(F64) * b.astype(F64)) * (1 + g.standard_normal(4000) * 1e-6)).astype(F32)      # heavy cancellation
    c[:2000] = g.standard_normal(2000).astype(F32)
    # forced double-rounding traps: a float32 midpoint plus a tiny product
    a[-3:], b[-3:], c[-3:] = F32(2.0 ** -30), [F32(1), F32(-1), F32(1)], F32(1) + F32(2.0 ** -23)
    got = R.fma32(a, b, c)
    for i in list(range(0, 4000, 7)) + [3997, 3998, 3999]:
        e = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r = got[i]
        for nb in (np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))):
            assert abs(Fraction(float(r)) - e) <= abs(Fraction(float(nb)) - e), i


def test_pool_truth_and_the_row_emulation():
    for c in R.POOL_ROWS_CHANNELS:
        for dims in R.POOL_ROWS_EXTENTS + [(20, 20, 20)]:
            x = R.field("offset30" if c == 16 else "randn", tuple(dims) + (c,), "pool")
            p = R.pool_truth(x)
            d, h, w = (n // 2 for n in dims)
            win = x[:2 * d, :2 * h, :2 * w].reshape(d, 2, h, 2, w, 2, c).max((1, 3, 5))
            assert R.bits_equal(p, win)
            nb = R.pool_rows(c, *dims)
            for nblocks in {nb, min(nb, 128)}:
                rows = R.pool_rows_as_coded(p, c, nblocks)
                S, dS, Q, dQ, j = R.pool_row_bounds(p, c, nblocks)
                assert (np.abs(rows["sum"].astype(LD).sum(0) - S) <= dS).all()
                assert (np.abs(rows["sq"].astype(LD).sum(0) - Q) <= dQ).all()
                assert (dS <= 1e-5 * np.abs(p.astype(F64)).sum((0, 1, 2)) * max(j, 1)).all()
                assert R.bits_equal(rows["mn"].min(0), p.min((0, 1, 2))) and R.bits_equal(rows["mx"].max(0), p.max((0, 1, 2)))


# ------------------------------------------------------------------------------------------------------ the two exports
def test_gn_stats_plan_export_obeys_the_header():
    lib = _lib()
    r, nb, vpb, rp = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
    seen = set()
    for c in list(range(1, 70)) + [96, 192, 255, 256, 257, 258, 512, 514, 1020, 1024, 1025, 1028, 2048, 2052, 4096, 40000]:
        for nvox in (1, 15, 16, 17, 210, 245, 4096, 27000, 2 ** 21, 2 ** 31 + 5):
            for al in (0, 1):
                assert lib.bfm_gn_stats_plan(c, nvox, al, C.byref(r), C.byref(nb), C.byref(vpb), C.byref(rp)) == 0
                got = (r.value, nb.value, vpb.value, rp.value)
                assert got == R.gn_plan(c, nvox, al), (c, nvox, al, got)
                assert (nb.value - 1) * vpb.value < nvox <= nb.value * vpb.value
                seen.add(r.value)
    assert seen == {0, 1, 2, 3}
    assert lib.bfm_gn_stats_plan(8, 100, 1, None, None, None, None) == 0
    assert lib.bfm_gn_stats_plan(0, 100, 1, None, None, None, None) == -1
    assert lib.bfm_gn_stats_plan(8, 0, 1, None, None, None, None) == -1
    for case in R.GN_TENSOR_CASES:
        assert R.gn_plan(case[0], int(np.prod(case[1])), not case[3])[0] == case[5], case
    for c, dims in R.GN_UNROLLED:
        _, _, v, p = R.gn_plan(c, int(np.prod(dims)), 1)
        assert v > 3 * p and v % (4 * p) != 0
    lo_, _, _, cb_, _ = R.GN_CAT_UNROLLED
    r_, _, v, p = R.gn_plan(cb_, int(np.prod(lo_)), 1)
    assert r_ == R.ROUTE_ROWS_VEC4 and v > 3 * p and v % (4 * p) != 0
    _, nblk, v, _ = R.gn_plan(8, int(np.prod(R.SHORT)), 1)
    assert int(np.prod(R.SHORT)) % v != 0 and nblk > 1                 # a short last block


def test_gn_stats_rows_route_export_obeys_the_header():
    lib = _lib()
    seen = set()
    for na in (1, 5, 127, 128, 129, 130, 257, 1000, 16000):
        for ca in (1, 8, 64, 1024):
            for nb_, cb in ((0, 0), (1, 64), (5, 128), (128, 8), (129, 8), (4000, 256)):
                for g in (1, 2, 8, 16, 32):
                    for tk in (0, 1):
                        got = lib.bfm_gn_stats_rows_route(na, ca, nb_, cb, g, tk)
                        if (ca + cb) % g:
                            assert got == -2
                            continue
                        assert got == R.rows_route(na, ca, nb_, cb, g, tk), (na, ca, nb_, cb, g, tk, got)
                        seen.add(got)
    assert seen == {0, 1, 2}
    assert lib.bfm_gn_stats_rows_route(0, 8, 0, 0, 1, 1) == -1 and lib.bfm_gn_stats_rows_route(4, 8, 0, 8, 1, 1) == -1
    assert lib.bfm_gn_stats_rows_route(4, 8, 0, 0, 0, 1) == -2 and lib.bfm_gn_stats_rows_route(4, 4096, 0, 0, 1, 1) == -2
    for case in R.GN_ROWS_CASES:
        assert lib.bfm_gn_stats_rows_route(*case[:5], 0) == case[6] and lib.bfm_gn_stats_rows_route(*case[:5], 1) == case[7]
    assert -(-129 // 16) == 9 and 129 - 14 * 9 == 3 and 15 * 9 >= 129          # 129 rows: slice 14 holds three, slice 15 none
    for c, dims in ((12, (4, 4, 4)), (192, (4, 4, 4)), (2048, (4, 4, 4)), (6, (4, 4, 4)), (8, (1, 4, 4)), (1028, (4, 4, 4))):
        assert lib.bfm_maxpool2_rows(c, *dims) == 0 == R.pool_rows(c, *dims)
    for c in R.POOL_ROWS_CHANNELS:
        for dims in R.POOL_ROWS_EXTENTS + [(82, 82, 82), (20, 20, 20)]:
            assert lib.bfm_maxpool2_rows(c, *dims) == R.pool_rows(c, *dims) > 0
            assert lib.bfm_maxpool2_batch_rows(c, *dims) == min(128, R.pool_rows(c, *dims))
    assert R.pool_rows(64, 82, 82, 82) == 4096 and 41 ** 3 * 16 > 4096 * 256          # the second grid-stride lap
    assert 10 ** 3 * 64 > 128 * 256                                                  # and the batch's, at 20^3 x 256


# --------------------------------------------------------------------------------- a model of the kernel and its mistakes
def _model(A, B, lo, hi, gamma, beta, G, mistake=None, acc=F64):
    """One-pass statistics the way the kernel takes them (weighted sums of the two sources, never the materialised
    concat), in `acc`; `mistake` names one of the issue's defects."""
    CA = A.shape[-1]
    nvox = int(np.prod(hi))

    def tot(v):
        v = v.astype(acc)
        return np.cumsum(v, axis=0, dtype=acc)[-1] if acc is F32 else v.sum(0)        # fp32: sequential, as a thread adds
    a = A.reshape(-1, CA).astype(acc)
    S, Q = [tot(a)], [tot(a * a)]
    if B is not None:
        reps = R.rep_counts(R.up_maps(lo, hi), lo)
        if mistake == "axes_swapped":
            reps = [reps[2], reps[1], reps[0]] if lo[0] == lo[2] else [reps[1], reps[0], reps[2]]
        w = (reps[0][:, None, None] * reps[1][None, :, None] * reps[2][None, None, :]).reshape(-1, 1).astype(acc)
        if mistake == "weight_dropped":
            w = np.ones_like(w)
        b = B.reshape(-1, B.shape[-1]).astype(acc)
        sb, qb = tot(w * b), tot(w * b * b)
        if mistake == "straddle_to_A":
            cpg = (CA + B.shape[-1]) // G
            k = (-CA) % cpg                                  # B channels that share a group with A channels
            sb[:k], qb[:k] = tot(b)[:k], tot(b * b)[:k]
        S.append(sb)
        Q.append(qb)
    S, Q = np.concatenate(S).astype(F64), np.concatenate(Q).astype(F64)
    cpg = len(S) // G
    count = int(np.prod(lo)) * 8 if (mistake == "count_from_B" and B is not None) else nvox
    n = float(count * cpg)
    mean = S.reshape(G, cpg).sum(1) / n
    var = np.maximum(Q.reshape(G, cpg).sum(1) / n - mean * mean, 0)
    if mistake == "sample_var" and n > 1:
        var = var * n / (n - 1)
    eps = F64(F32(R.EPS))
    rstd = 1 / (np.sqrt(var) + eps) if mistake == "eps_outside" else 1 / np.sqrt(var + eps)
    mean32, rstd32 = mean.astype(F32), rstd.astype(F32)
    sc, sh = R.affine_as_coded(mean32, rstd32, gamma, beta, G)
    return dict(mean=mean32, rstd=rstd32, scale=sc, shift=sh)


def _worst(truth, m):
    return max(R.gn_ratios(truth, m["scale"], m["shift"], m["mean"], m["rstd"]).values())


def _gn_case_list():
    out = []
    for case in R.GN_TENSOR_CASES:
        if int(np.prod(case[1])) * case[0] > 300000 and case[4] == "randn":
            continue                                             # the two large shapes add nothing here
        A, gamma, beta = R.tensor_inputs(case)
        out.append((str(case), A, None, None, case[1], gamma, beta, case[2]))
    for lo, hi, ca, cb, g in _cat_cases():
        A, B, gamma, beta = R.cat_inputs(lo, hi, ca, cb, g)
        out.append((str((lo, hi, ca, cb, g)), A, B, lo, hi, gamma, beta, g))
    return out


@pytest.fixture(scope="module")
def gn_cases():
    cases = _gn_case_list()
    return [(c, R.gn_truth(c[1], c[2], R.up_maps(c[3], c[4]) if c[2] is not None else None, c[5], c[6], c[7]))
            for c in cases]


def test_bounds_hold_for_float64_one_pass_and_are_not_vacuous(gn_cases):
    worst, off = 0.0, []
    for (name, A, B, lo, hi, gamma, beta, G), t in gn_cases:
        m = _model(A, B, lo, hi, gamma, beta, G)
        r = _worst(t, m)
        assert r <= 1.0, (name, r)
        worst = max(worst, r)
        # the float64 one-pass variance itself, before any fp32 rounding, against dvar
        cpg = (A.shape[-1] + (B.shape[-1] if B is not None else 0)) // G
        tight = np.concatenate([(t["drstd"] / t["rstd"]), (t["dscale"] / np.maximum(np.abs(t["scale"]), 1e-300))[t["scale"] != 0]])
        if "offset" in name:
            off.append((name, float(tight.max())))
        else:
            assert tight.max() <= 1e-5, (name, tight.max())
            ok = np.abs(t["mean"]) > 1e-3 * np.sqrt(t["ex2"])
            assert (t["dmean"][ok] <= 1e-5 * np.abs(t["mean"][ok])).all(), name
    print("\nfloat64 one-pass + fp32 outputs: worst ratio to the bound %.3g; offset cases bound / |quantity|: %s" % (worst, off))
    assert off and all(v <= 1e-5 for _, v in off)                 # ~4e-6: still far below what fp32 accumulation does


MISTAKES = ["weight_dropped", "count_from_B", "axes_swapped", "straddle_to_A", "sample_var", "eps_outside"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_each_statistics_mistake_fails_the_bounds(gn_cases, mistake):
    hit = []
    for (name, A, B, lo, hi, gamma, beta, G), t in gn_cases:
        if _worst(t, _model(A, B, lo, hi, gamma, beta, G, mistake)) > 1.0:
            hit.append(name)
    assert hit, mistake
    if mistake == "count_from_B":
        assert any(str(R.UPSAMPLES[1][1]) in h for h in hit)        # the non-2x upsample is what catches it
    if mistake == "straddle_to_A":
        assert any("64, 128, 8" in h for h in hit)


def test_fp32_accumulation_is_caught_by_the_offset_case(gn_cases):
    seen = False
    for (name, A, B, lo, hi, gamma, beta, G), t in gn_cases:
        if "offset1e3" not in name:
            continue
        seen = True
        m = _model(A, B, lo, hi, gamma, beta, G, acc=F32)
        rel = np.abs(m["rstd"].astype(F64) - t["rstd"]) / t["rstd"]
        ratio = _worst(t, m)
        print("\n%s: fp32 accumulation rstd error %.3g, %.3g x the bound" % (name, rel.max(), ratio))
        assert ratio > 1e3
    assert seen


def test_each_bound_mistake_changes_the_bits(gn_cases):
    hits = {"from_mean": 0, "neg_gamma": 0}
    for (name, A, B, lo, hi, gamma, beta, G), t in gn_cases:
        m = _model(A, B, lo, hi, gamma, beta, G)
        mn, mx = R.extremes_as_coded(A, B)
        good = R.gn_bound_as_coded(m["scale"], m["shift"], mn, mx, G)
        assert (np.abs(good.astype(F64) - t["bound"]) <= t["dbound"]).all(), name
        cmean = np.repeat(m["mean"], len(mn) // G)
        hits["from_mean"] += R.n_diff(good, R.gn_bound_as_coded(m["scale"], m["shift"], cmean, cmean, G)) > 0
        with np.errstate(all="ignore"):
            naive = np.fmax(R.fma32(mx, m["scale"], m["shift"]), -R.fma32(mn, m["scale"], m["shift"]))
        naive = np.fmax.reduce(np.fmax(naive, F32(0)).reshape(G, -1), axis=1)
        hits["neg_gamma"] += R.n_diff(good, naive) > 0
    assert all(v > 0 for v in hits.values()), hits
    swapped = 0
    for case in R.GN_ROWS_CASES[:8]:
        tA, tB, gamma, beta, nvox = R.rows_inputs(case)
        t = R.rows_truth(tA, tB, case[5], nvox, gamma, beta, case[4])
        sc, sh = R.affine_as_coded(t["mean"].astype(F32), t["rstd"].astype(F32), gamma, beta, case[4])
        good = R.gn_bound_as_coded(sc, sh, t["chan_min"], t["chan_max"], case[4])
        tabs = [x for x in (tA, tB) if x is not None]
        mn = np.concatenate([np.fmin.reduce(x["mx"], axis=0) for x in tabs])          # the planes taken for each other
        mx = np.concatenate([np.fmax.reduce(x["mn"], axis=0) for x in tabs])
        swapped += R.n_diff(good, R.gn_bound_as_coded(sc, sh, mn, mx, case[4])) > 0
    assert swapped >= 6                                       # a one-row table has min == max planes folded alike


def test_each_pool_mistake_fails():
    x = R.field("randn", (5, 7, 9, 4), "poolm")
    good = R.pool_truth(x)
    odd = x[1:, 1:, 1:]                                                     # window anchored at odd indices
    anchored = odd[:4, :6, :8].reshape(2, 2, 3, 2, 4, 2, 4).max((1, 3, 5))
    assert anchored.shape == good.shape and R.n_diff(good, anchored) > 0
    t = torch.from_numpy(x).permute(3, 0, 1, 2)[None]
    assert tuple(Fn.max_pool3d(t, 2, ceil_mode=True).shape[2:]) != good.shape[:3]      # ceil instead of floor
    p = R.pool_truth(R.field("randn", (12, 10, 14, 16), "poolm"))
    nb = R.pool_rows(16, 12, 10, 14)
    rows = R.pool_rows_as_coded(p, 16, nb)
    assert nb > 1
    t_ = rows["sum"].T.reshape(nb, 16)                                          # [C][rows] read as [rows][C]
    assert not R.bits_equal(np.ascontiguousarray(t_), rows["sum"])
    S = p.astype(F64).sum((0, 1, 2))
    assert np.abs(np.ascontiguousarray(t_).sum(0) - S).max() > 1e-3 * np.abs(S).max()
