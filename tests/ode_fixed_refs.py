"""NumPy restatement of the reference's fixed-grid ODE solvers (ShapeID/DiffEqs/fixed_grid.py:5-33,
solvers.py:158-207, rk_common.py:72-78) on fp32 right-hand sides, for tests/test_host_ode_fixed.py and
tests/test_gpu_ode_fixed.py.

Two forms of the step functions:

  step_reference   the reference's expression order with torch's promotion rules written out: the step `dt` is a 0-dim
                   tensor in the state dtype, the stages are fp32 tensors, so `dt * k` multiplies in fp32 by dt rounded
                   to fp32, and Python scalars (2, 3, -3, 8) act in the dtype of the tensor they meet.
  step_kset        what the library computes: every stage state and the final sum as sum_j fp32((dt c_j) in the state
                   dtype) * k_j, left to right in fp32 (bfm_rk_combine).  Equal to step_reference for euler and
                   midpoint (a division by 2 is exact); rk4's `/ 3`, `k1 / -3 + k2` and `(..) * (dt / 8)` round
                   differently in the last fp32 place of dy.
"""
import numpy as np

F32 = np.float32
METHODS = ("euler", "midpoint", "rk4")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}

# the tables of brainfm_amd/shapeid.py, restated: stage states after the first, first k of the final sum, final sum
KSET_TABLES = {
    "euler": ([], 0, [1.]),
    "midpoint": ([[1 / 2]], 1, [1.]),
    "rk4": ([[1 / 3], [-1 / 3, 1.], [1., -1., 1.]], 0, [1 / 8, 3 / 8, 3 / 8, 1 / 8]),
}


def time_grid(t, sd):
    """solvers.py:160-165: the requested times cast to the state dtype ARE the grid (no step_size is given)."""
    return np.asarray(t, np.float64).astype(sd)


def step_reference(method, rhs, dt, y):
    """dy of one step; `dt` a scalar of the state dtype, y the state, rhs(y) -> fp32."""
    d = F32(dt)                                     # the fp32 value a 0-dim `dt` multiplies an fp32 tensor with
    if method == "euler":                           # fixed_grid.py:7-8
        return d * rhs(y)
    if method == "midpoint":                        # fixed_grid.py:17-19
        y_mid = y + rhs(y) * d / F32(2)
        return d * rhs(y_mid)
    assert method == "rk4"                          # rk_common.py:72-78 (the 3/8 rule)
    sd = type(dt)
    k1 = rhs(y)
    k2 = rhs(y + d * k1 / F32(3))
    k3 = rhs(y + d * (k1 / F32(-3) + k2))
    k4 = rhs(y + d * (k1 - k2 + k3))
    return (k1 + F32(3) * k2 + F32(3) * k3 + k4) * F32(dt / sd(8))


def _sum(dt, coef, ks):
    sd = type(dt)
    acc = None
    for c, k in zip(coef, ks):
        term = F32(dt * sd(c)) * k
        acc = term if acc is None else acc + term
    return acc


def step_kset(method, rhs, dt, y):
    stages, first, final = KSET_TABLES[method]
    ks = [rhs(y)]
    for c in stages:
        ks.append(rhs(y + _sum(dt, c, ks)))
    return _sum(dt, final, ks[first:])


def integrate(method, rhs, y0, t, step=step_reference, stats=None):
    """FixedGridODESolver.integrate: y1 = y0 + dy per grid interval; a row is appended while t1 >= t[j], which with
    grid == t is once per step, and _linear_interp returns y1 itself (t == t1)."""
    sd = y0.dtype.type
    grid = time_grid(t, sd)
    tt = grid
    sol = [y0]
    y = y0
    j = 1
    nfe = [0]

    def counted(v):
        nfe[0] += 1
        out = rhs(v)
        assert out.dtype == F32
        return out
    for t0, t1 in zip(grid[:-1], grid[1:]):
        dy = step(method, counted, sd(t1 - t0), y)
        assert dy.dtype == F32
        y = (y + dy).astype(sd)
        while j < len(tt) and t1 >= tt[j]:
            sol.append(y)
            j += 1
    if stats is not None:
        stats["nfe"] = nfe[0]
    return np.stack(sol)


def rel_err(a, b):
    """The measure of test_gpu_synth._close: max |a - b| over max |b|."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))


def golden_cases():
    """(file, volume tag, method, dtype tag, bc tag) of every stored reference solution."""
    out = []
    for m in METHODS:
        for dt in ("f32", "f64"):
            for bc in ("neumann", "none"):
                out.append(("ode_fixed.npz", "small", m, dt, bc))
                out.append(("ode_fixed_large_%s.npz" % dt, "large", m, dt, bc))
    return out
