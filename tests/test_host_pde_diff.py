"""The diffusion terms and the general velocity of AdvDiffPDE restated in float64 NumPy (tests/pde_diff_refs.py) against
golden outputs of the real reference (tests/golden/make_golden_pde_diff.py), the stencil facts the HIP stage kernels rest
on, and what the constructor takes and refuses.  CPU only."""
import functools

import numpy as np
import pytest

import pde_diff_refs as R
from conftest import load_npz


@functools.lru_cache(maxsize=None)
def _npz():
    return load_npz("pde_diff.npz")


def _gold_rhs(vol, case):
    d = _npz()
    if vol != "c":
        return d["rhs_" + R.case_tag(vol, *case)]
    is64 = lambda c: c[4] == "f64" and c[0] == "adv_diff" and c[1] == "vector"
    same = [c for c in R.small_rhs_cases() if is64(c) == is64(case)]
    return d["c_rhs_f64" if is64(case) else "c_rhs_f32"][same.index(case)]


def restated(vol, case):
    """(golden, float64 restatement) of one RHS case."""
    perf, vt, dty, bc, dt = case
    d = _npz()
    C, V, D = R.fields(d, vol)
    want = R.rhs(R.state(C, dt), perf, dty, vt, bc, V, R.d_dict(dty, D, np.float32(d["D_const"])))
    return _gold_rhs(vol, case), want


def fp32_bound(vol, case):
    """What fp32 evaluation may differ from exact arithmetic by: every term is a coefficient (a V or D value, or a
    difference of them, at most 2 max) times a first or second difference of C (at most 4 max|C|); the upwind and div V
    terms number 6, the diffusion terms at most 18, each is formed from fp32-rounded factors and about 25 partial sums
    are rounded, so 2 * 25 roundings of quantities bounded by the sum of the terms' bounds."""
    perf, vt, dty, bc, dt = case
    C, V, D = R.fields(_npz(), vol)
    amp = 0.0
    if "adv" in perf:
        amp += 6 * 2 * max(float(np.abs(v).max()) for v in V.values()) * 4 * float(np.abs(C).max())
    amp += 18 * 2 * max(0.3, max(float(np.abs(v).max()) for v in D.values())) * 4 * float(np.abs(C).max())
    return 50 * 2.0 ** -24 * amp


ALL_RHS = [("c",) + c for c in R.small_rhs_cases()] + [(v,) + c for v in ("a", "b") for c in R.BOX_RHS_CASES]


@pytest.mark.parametrize("vol,perf,vt,dty,bc,dt", ALL_RHS)
def test_restatement_equals_the_reference_golden_up_to_fp32_rounding(vol, perf, vt, dty, bc, dt):
    case = (perf, vt, dty, bc, dt)
    gold, want = restated(vol, case)
    assert gold.shape == want.shape == R.SHAPES[vol]
    assert gold.dtype == (np.float64 if (dt == "f64" and perf == "adv_diff" and vt == "vector") else np.float32)
    dist = float(np.abs(gold - want).max())
    assert dist <= fp32_bound(vol, case), (dist, fp32_bound(vol, case))
    assert dist <= 1e-5 * float(np.abs(want).max())


def test_fixture_covers_what_it_should():
    d = _npz()
    cases = [("c",) + c for c in R.small_rhs_cases()] + [(v,) + c for v in ("a", "b") for c in R.BOX_RHS_CASES]
    for axis, want in ((3, set(R.D_TYPES)), (4, set(R.BCS)), (5, set(R.DTS)), (2, {"vector", "vector_div_free"}),
                       (1, {"diff", "adv_diff"})):
        for v in "abc":
            assert {c[axis] for c in cases if c[0] == v} == want, (v, axis)
    assert d["c_rhs_f32"].shape[0] + d["c_rhs_f64"].shape[0] == len(R.small_rhs_cases())
    for v, perf, vt, dty, methods in R.INTEG_CASES:
        for m in methods:
            tag = R.case_tag(v, perf, vt, dty, m)
            assert d["sol_%s_f32" % tag].dtype == np.float32 and d["sol_%s_f64" % tag].dtype == np.float64
            nfe = int(d["nfe_" + tag])
            if m == "dopri5":                               # f(t0, y0), one more for the first step size, 6 per step
                assert nfe > 2 and (nfe - 2) % 6 == 0
            else:
                assert nfe == 6 * R.STAGES[m]
            # the reference's own fp32-state against fp64-state distance, as recorded
            a, b = d["sol_%s_f32" % tag].astype(np.float64), d["sol_%s_f64" % tag]
            assert float(d["dist_" + tag]) == float(np.abs(a - b).max() / np.abs(b).max())
    for v in ("a", "b"):
        assert any(c[0] == v and c[4] == R.METHODS for c in R.INTEG_CASES)


# ---- the stencil facts the stage kernels rest on
@pytest.mark.parametrize("a", [0, 1, 2])
def test_second_difference_on_a_ramp_and_at_the_ends(a):
    shape = (5, 4, 6)
    ramp = np.arange(shape[a], dtype=np.float64).reshape([-1 if i == a else 1 for i in range(3)]) * np.ones(shape)
    assert np.array_equal(R.lap_term(ramp, a), np.zeros(shape))
    assert np.array_equal(R.grad_c(ramp, a), np.ones(shape))
    C = np.random.RandomState(a).rand(*shape)
    lap = R.lap_term(C, a)
    take = lambda X, i: np.take(X, i, axis=a)
    # index 0: f[1] - f[0] reaches index 2;  last index: f[n-1] - f[n-2] with both C[n-1] - C[n-2], exactly 0
    assert np.array_equal(take(lap, 0), (take(C, 2) - take(C, 1)) - (take(C, 1) - take(C, 0)))
    assert np.array_equal(take(lap, -1), np.zeros_like(take(lap, -1)))
    assert np.array_equal(take(lap, 2), (take(C, 3) - take(C, 2)) - (take(C, 2) - take(C, 1)))


def test_a_delta_is_seen_from_the_3x3x3_neighbourhood_and_from_index_0_only():
    shape = (9, 8, 10)
    rs = np.random.RandomState(3)
    D = {k: 0.2 + rs.rand(*shape) for k in R.D_FIELDS}
    V = {k: rs.randn(*shape) for k in ("Vx", "Vy", "Vz")}
    p = (4, 4, 5)
    C = np.zeros(shape)
    C[p] = 1.0
    out = R.rhs(C, "adv_diff", "full", "vector", "none", V, D)
    idx = np.argwhere(out != 0) - np.array(p)
    assert np.abs(idx).max() == 1
    # the cross terms read edge neighbours: the voxel at p + (1, -1, 0) sees the delta through b_x(f_y C)
    assert out[p[0] + 1, p[1] - 1, p[2]] != 0 and out[p[0], p[1] + 1, p[2] - 1] != 0
    only_diag = R.rhs(C, "diff", "diag", "vector", "none", V, D)
    assert only_diag[p[0] + 1, p[1] - 1, p[2]] == 0
    # a delta at index 2 of an axis is seen from index 0 of that axis, and from nowhere else two voxels away
    for a in range(3):
        q = [4, 4, 5]
        q[a] = 2
        C = np.zeros(shape)
        C[tuple(q)] = 1.0
        out = R.rhs(C, "diff", "constant", "vector", "none", V, {"D": 0.3})
        far = np.argwhere(out != 0) - np.array(q)
        two = far[np.abs(far).max(axis=1) == 2]
        assert len(two) == 1 and two[0][a] == -2 and np.abs(far).max() == 2
        assert out[tuple(0 if i == a else q[i] for i in range(3))] == 0.3


def test_neumann_condition_replicates_the_interior_and_dirichlet_is_the_identity():
    C = np.random.RandomState(5).rand(5, 4, 6)
    assert R.set_bc(C, "dirichlet") is C and R.set_bc(C, "none") is C
    N = R.set_bc(C, "neumann")
    assert np.array_equal(N[1:-1, 1:-1, 1:-1], C[1:-1, 1:-1, 1:-1])
    assert np.array_equal(N[0], N[1]) and np.array_equal(N[:, -1], N[:, -2]) and np.array_equal(N[:, :, 0], N[:, :, 1])


# ---- the constructor (Python layer only)
U = [1., 1., 1.]


def _pde(*a, **k):
    from brainfm_amd import shapeid as SH
    return SH.AdvDiffPDE(*a, **k)


@pytest.mark.parametrize("perf", ["diff", "adv_diff", "diff_adv", "adv"])
@pytest.mark.parametrize("dty", list(R.D_TYPES) + ["full_spectral", "full_cholesky", "full_symmetric"])
@pytest.mark.parametrize("vt", list(R.V_DIV_FREE) + ["vector"])
def test_constructor_accepts_the_configurations_the_reference_runs(perf, dty, vt):
    for bc in (None, "neumann", "cauchy", "dirichlet"):
        pde = _pde(U, perf, D_type=dty, V_type=vt, BC=bc)
        assert (pde.perf_pattern, pde.D_type, pde.V_type, pde.BC, pde.nfe) == (perf, dty, vt, bc, 0)


def test_constructor_refuses_by_name():
    for kw, pat in ((dict(perf_pattern="adv_diff", stochastic=True), "stochastic"),
                    (dict(perf_pattern="diff", stochastic=True), "stochastic"),
                    (dict(perf_pattern="adv", V_type="constant"), "'constant'"),
                    (dict(perf_pattern="adv_diff", V_type="scalar"), "'scalar'"),
                    (dict(perf_pattern="adv_diff", BC="dirichlet_neumann"), "dirichlet_neumann"),
                    (dict(perf_pattern="diff", BC="source_neumann"), "source_neumann")):
        with pytest.raises(NotImplementedError, match=pat):
            _pde(U, **kw)
    with pytest.raises(NotImplementedError):
        _pde([1., 1., 2.], "adv_diff")
    with pytest.raises(NotImplementedError):
        _pde([1., 1.], "diff")
    with pytest.raises(NotImplementedError):
        _pde([1.], "diff")
    with pytest.raises(NotImplementedError):
        _pde(U, "diff", D_type="tensor")
    with pytest.raises(NotImplementedError):
        _pde(U, "adv", V_type="vector_div_free", BC="periodic")
