"""The fixed-grid ODE solvers (euler, midpoint, rk4) restated in NumPy (tests/ode_fixed_refs.py) against golden vectors
produced by the real reference (tests/golden/make_golden_ode_fixed.py).  CPU only."""
import functools

import numpy as np
import pytest

import ode_fixed_refs as R
from conftest import load_npz
from oracle import synth_ref as S

T10 = np.arange(10) * 0.1
NTS = (2, 5, 10)


@functools.lru_cache(maxsize=None)
def _npz(name):
    return load_npz(name)


def _case(file, m, dt, bc):
    d = _npz(file)
    y0 = d["y0"][0] if dt == "f64" else d["y0"][0].astype(np.float32)
    V = (d["Vx"], d["Vy"], d["Vz"])
    rhs = lambda y: S.advect_rhs(y, *V, bc=None if bc == "none" else bc)
    tag = "%s_%s_%s" % (m, dt, bc)
    return d, y0, rhs, d["sol_" + tag][:, 0], d["nfe_" + tag]


@functools.lru_cache(maxsize=None)
def _solution(file, m, dt, bc, form):
    """The nt = 10 restatement, computed once per case: the nt = 2 and 5 runs are its leading rows (the same steps)."""
    d, y0, rhs, gold, nfe = _case(file, m, dt, bc)
    st = {}
    sol = R.integrate(m, rhs, y0, T10, step=getattr(R, "step_" + form), stats=st)
    return sol, st["nfe"]


@pytest.mark.parametrize("file,vol,m,dt,bc", R.golden_cases())
def test_reference_expression_order_equals_the_golden_bit_for_bit(file, vol, m, dt, bc):
    d, y0, rhs, gold, nfe = _case(file, m, dt, bc)
    sol, n = _solution(file, m, dt, bc, "reference")
    assert sol.dtype == gold.dtype and sol.shape == (10,) + y0.shape
    assert n == int(nfe[2]) == R.STAGES[m] * 9
    rows = list(range(10)) if vol == "small" else [int(r) for r in d["rows"]]
    assert gold.shape[0] == len(rows)
    assert np.array_equal(sol[rows], gold)
    assert [int(v) for v in nfe] == [R.STAGES[m] * (nt - 1) for nt in NTS]


@pytest.mark.parametrize("file,vol,m,dt,bc", R.golden_cases())
def test_kset_form_is_the_reference_for_euler_and_midpoint_and_close_for_rk4(file, vol, m, dt, bc):
    """The library forms every stage state and the final sum as sum_j fp32(dt c_j) k_j (bfm_rk_combine).  That IS the
    reference's expression for euler and midpoint.  rk4's `dt * k1 / 3`, `dt * (k1 / -3 + k2)` and
    `(k1 + 3 k2 + 3 k3 + k4) * (dt / 8)` round differently in the last fp32 place of dy, so that form is held at the
    tolerance test_advection_rhs_and_dopri5 applies to dopri5 states: 1e-6 (fp64 state), 3e-5 (fp32 state)."""
    d, y0, rhs, gold, nfe = _case(file, m, dt, bc)
    sol, n = _solution(file, m, dt, bc, "kset")
    rows = list(range(10)) if vol == "small" else [int(r) for r in d["rows"]]
    assert sol.dtype == gold.dtype and n == R.STAGES[m] * 9
    if m in ("euler", "midpoint"):
        assert np.array_equal(sol[rows], gold)
    else:
        e = R.rel_err(sol[rows], gold)
        print("rk4 kset form against the golden:", file, dt, bc, e)
        assert e <= (1e-6 if dt == "f64" else 3e-5), e


def test_the_fp32_grid_is_not_steps_of_a_tenth():
    """solvers.py:160-165 casts `t` to the state dtype: an fp32 state steps by differences of fp32 times."""
    g32, g64 = R.time_grid(T10, np.float32), R.time_grid(T10, np.float64)
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    s32 = np.diff(g32)
    assert s32.dtype == np.float32
    assert s32[0] == np.float32(0.1)                              # t[1] - 0 is fp32(0.1) itself
    assert np.any(s32 != np.float32(0.1))                         # ... but later differences are not
    assert s32[2] == np.float32(np.float32(0.1 * 3) - np.float32(0.1 * 2)) != np.float32(0.1)
    s64 = np.diff(g64)
    assert np.array_equal(g64, T10) and np.any(s64 != 0.1)        # fp64: differences of arange(10) * 0.1, not 0.1 either
    # and it matters: stepping the fp32 state by fp32(0.1) everywhere leaves the golden
    d, y0, rhs, gold, nfe = _case("ode_fixed.npz", "euler", "f32", "neumann")
    y = y0
    for _ in range(9):
        y = y + np.float32(0.1) * rhs(y)
    assert not np.array_equal(y, gold[9])
    assert np.array_equal(_solution("ode_fixed.npz", "euler", "f32", "neumann", "reference")[0][9], gold[9])


def test_output_rule_appends_one_row_per_step():
    """A row is appended while t1 >= t[j]; with grid == t that is exactly one per step, never interpolated."""
    calls = []

    def rhs(y):
        calls.append(1)
        return np.ones_like(y, dtype=np.float32)
    y0 = np.zeros((3, 3, 3), np.float64)
    t = np.array([0.0, 0.25, 0.75, 1.0])
    st = {}
    sol = R.integrate("euler", rhs, y0, t, stats=st)
    assert sol.shape == (4, 3, 3, 3) and st["nfe"] == 3 == len(calls)
    assert np.array_equal(sol[:, 0, 0, 0], np.array([0.0, 0.25, 0.75, 1.0]))


def test_library_tables_grid_and_coefficients_are_the_restated_ones():
    """The host side of shapeid.FixedGridSolver (no kernel runs): its stage tables are the ones step_kset restates, its
    steps are differences of the grid in the state dtype, and a coefficient is (dt c) in the state dtype rounded to fp32."""
    import torch
    from brainfm_amd import shapeid as SH
    assert set(SH._FIXED_TABLES) == set(R.METHODS)
    for m in R.METHODS:
        assert SH._FIXED_TABLES[m] == R.KSET_TABLES[m]
        assert len(SH._FIXED_TABLES[m][0]) + 1 == R.STAGES[m]
        for dtype, sd in ((torch.float32, np.float32), (torch.float64, np.float64)):
            s = SH.FixedGridSolver(None, torch.zeros(1, 3, 3, 3, dtype=dtype), m)
            steps = s.grid_steps([float(v) for v in T10])
            assert all(type(v) is sd for v in steps)
            assert np.array_equal(np.array(steps), np.diff(R.time_grid(T10, sd)))
            got = s._coefs(steps[2], [1 / 3, -1 / 3, 3 / 8])
            want = [float(np.float32(steps[2] * sd(c))) for c in (1 / 3, -1 / 3, 3 / 8)]
            assert got == want
    from brainfm_amd import _lib as L
    lib = L.load()
    assert [lib.bfm_ode_fixed_ncoef(i) for i in (L.ODE_EULER, L.ODE_MIDPOINT, L.ODE_RK4, 3, -1)] == [1, 2, 10, 0, 0]
    for m in R.METHODS:
        stages, first, final = SH._FIXED_TABLES[m]
        assert sum(len(c) for c in stages) + len(final) == lib.bfm_ode_fixed_ncoef(SH._FIXED_IDS[m])


def test_the_export_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from brainfm_amd import _lib as L
    lib = L.load()
    d = L.OdeFixedAdvect()
    assert lib.bfm_ode_fixed_advect(None, None) != 0
    d.sx, d.sy, d.sz, d.nt, d.method = 4, 4, 4, 3, L.ODE_EULER
    assert lib.bfm_ode_fixed_advect(C.byref(d), None) != 0                    # null solution / velocity / coefficients
    assert C.sizeof(d) == 96                                                  # bfm_ode_fixed_advect_t on LP64


def test_generator_fixture_is_consistent():
    d = _npz("ode_fixed.npz")
    np.random.seed(int(d["gen_seed"]))
    assert np.random.randint(1, 11) == int(d["gen_nt"]) >= 2
    assert d["gen_out"].shape == d["gen_P"].shape[1:] and d["gen_out"].dtype == np.float64
    assert np.isfinite(d["gen_out"]).all()
