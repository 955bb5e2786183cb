"""Float64 numpy restatement of the right-hand sides of AdvDiffPDE beyond the generator's configuration
(ShapeID/DiffEqs/pde.py:13-190, :362-441, :499-524, :587-640), 3-D, unit spacing, one volume.  Written from the
formulas, with no rounding anywhere: what the golden outputs of the reference (tests/golden/pde_diff.npz) and the HIP
kernels are both measured against."""
import numpy as np

SHAPES = {"a": (12, 10, 14), "b": (11, 9, 37), "c": (4, 3, 5)}
D_FIELDS = ("Dxx", "Dyy", "Dzz", "Dxy", "Dyz", "Dxz")
FULL_NAMES = ("full", "full_dual", "full_spectral", "full_cholesky", "full_symmetric")
V_DIV_FREE = ("vector_div_free", "vector_div_free_clebsch", "vector_div_free_stream", "vector_div_free_stream_gauge")


def _sl(a, s):
    out = [slice(None)] * 3
    out[a] = s
    return tuple(out)


def grad_f(X, a):
    """Forward difference along axis a, backward at the last index (gradient_f)."""
    d = np.empty_like(X)
    d[_sl(a, slice(None, -1))] = X[_sl(a, slice(1, None))] - X[_sl(a, slice(None, -1))]
    d[_sl(a, -1)] = X[_sl(a, -1)] - X[_sl(a, -2)]
    return d


def grad_b(X, a):
    """Backward difference along axis a, forward at index 0 (gradient_b)."""
    d = np.empty_like(X)
    d[_sl(a, slice(1, None))] = X[_sl(a, slice(1, None))] - X[_sl(a, slice(None, -1))]
    d[_sl(a, 0)] = X[_sl(a, 1)] - X[_sl(a, 0)]
    return d


def grad_c(X, a):
    """Central difference along axis a, one-sided at both ends (gradient_c)."""
    d = np.empty_like(X)
    d[_sl(a, slice(1, -1))] = (X[_sl(a, slice(2, None))] - X[_sl(a, slice(None, -2))]) / 2
    d[_sl(a, 0)] = X[_sl(a, 1)] - X[_sl(a, 0)]
    d[_sl(a, -1)] = X[_sl(a, -1)] - X[_sl(a, -2)]
    return d


def lap_term(C, a):
    """b_a(f_a C)."""
    return grad_b(grad_f(C, a), a)


def set_bc(C, bc):
    """'neumann' / 'cauchy': the interior replicated onto the faces (pde.py:591-597); anything else: identity."""
    if bc in ("neumann", "cauchy"):
        return np.pad(C[1:-1, 1:-1, 1:-1], 1, mode="edge")
    return C


def diffusion(C, D_type, D):
    if D_type == "constant":
        return float(D["D"]) * (lap_term(C, 0) + lap_term(C, 1) + lap_term(C, 2))
    if D_type == "scalar":
        out = sum(grad_c(D["D"], a) * grad_c(C, a) for a in range(3))
        return out + sum(D["D"] * lap_term(C, a) for a in range(3))
    if D_type == "diag":
        return sum(grad_c(D[n], a) * grad_c(C, a) + D[n] * lap_term(C, a) for a, n in enumerate(D_FIELDS[:3]))
    if D_type in FULL_NAMES:
        x, y, z = 0, 1, 2
        f = [grad_f(C, a) for a in range(3)]
        c = [grad_c(C, a) for a in range(3)]
        return ((grad_c(D["Dxx"], x) + grad_c(D["Dxy"], y) + grad_c(D["Dxz"], z)) * c[x]
                + (grad_c(D["Dxy"], x) + grad_c(D["Dyy"], y) + grad_c(D["Dyz"], z)) * c[y]
                + (grad_c(D["Dxz"], x) + grad_c(D["Dyz"], y) + grad_c(D["Dzz"], z)) * c[z]
                + D["Dxx"] * grad_b(f[x], x) + D["Dyy"] * grad_b(f[y], y) + D["Dzz"] * grad_b(f[z], z)
                + D["Dxy"] * (grad_b(f[y], x) + grad_b(f[x], y))
                + D["Dyz"] * (grad_b(f[z], y) + grad_b(f[y], z))
                + D["Dxz"] * (grad_b(f[x], z) + grad_b(f[z], x)))
    raise KeyError(D_type)


def advection(C, V_type, V):
    out = 0.0
    for a, n in enumerate(("Vx", "Vy", "Vz")):
        up = np.where(V[n] > 0, grad_b(C, a), grad_f(C, a))
        out = out + V[n] * up
    out = -out
    if V_type == "vector":
        out = out - C * (grad_c(V["Vx"], 0) + grad_c(V["Vy"], 1) + grad_c(V["Vz"], 2))
    elif V_type not in V_DIV_FREE:
        raise KeyError(V_type)
    return out


def rhs(C, perf, D_type, V_type, bc, V, D):
    """AdvDiffPDE.forward (pde.py:616-640) on one (s, r, c) volume, all float64."""
    C = set_bc(np.asarray(C, np.float64), bc)
    V = {k: np.asarray(v, np.float64).reshape(C.shape) for k, v in V.items()}
    D = {k: (np.asarray(v, np.float64).reshape(C.shape) if np.size(v) > 1 else float(np.asarray(v).reshape(-1)[0]))
         for k, v in D.items()}
    if "diff" not in perf:
        return advection(C, V_type, V)
    if "adv" not in perf:
        return diffusion(C, D_type, D)
    return advection(C, V_type, V) + diffusion(C, D_type, D)


# ---- the cases of tests/golden/pde_diff.npz ---------------------------------------------------------------------------
BCS = ("none", "neumann", "dirichlet")
D_TYPES = ("constant", "scalar", "diag", "full", "full_dual")
# (perf_pattern, V_type): 'diff' reads no V
PERFS = (("diff", "vector"), ("adv_diff", "vector_div_free"), ("adv_diff", "vector"))
DTS = ("f32", "f64")


def small_rhs_cases():
    """Every combination on the 4 x 3 x 5 volume."""
    return [(perf, vt, dty, bc, dt) for perf, vt in PERFS for dty in D_TYPES for bc in BCS for dt in DTS]


# a covering choice on the two volumes that span boxes: every D type and the alias, both V types, every BC, both dtypes
BOX_RHS_CASES = (
    ("diff", "vector", "constant", "none", "f32"),
    ("diff", "vector", "scalar", "neumann", "f64"),
    ("diff", "vector", "diag", "dirichlet", "f32"),
    ("diff", "vector", "full", "neumann", "f32"),
    ("adv_diff", "vector_div_free", "full_dual", "neumann", "f64"),
    ("adv_diff", "vector", "scalar", "none", "f32"),
    ("adv_diff", "vector", "full", "neumann", "f64"),
    ("adv_diff", "vector_div_free", "diag", "dirichlet", "f32"),
    ("adv_diff", "vector", "constant", "dirichlet", "f64"),
)

METHODS = ("dopri5", "rk4", "midpoint", "euler")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
T7 = 0.1 * np.arange(7)
# (volume, perf_pattern, V_type, D_type, methods): BC 'neumann', both state dtypes; the last solution row is kept
INTEG_CASES = (
    ("a", "adv_diff", "vector_div_free", "full", METHODS),
    ("b", "adv_diff", "vector_div_free", "full", METHODS),
    ("a", "diff", "vector", "scalar", ("dopri5",)),
    ("a", "adv_diff", "vector", "diag", ("dopri5",)),
    ("a", "diff", "vector", "constant", ("dopri5",)),
)


# the one integration whose every row is kept (dopri5's dense output at the inner times), as "rows_<tag>_<dtype>"
ALL_ROWS_CASE = ("a", "adv_diff", "vector_div_free", "full", "dopri5")


def case_tag(*parts):
    return "_".join(str(p) for p in parts)


def fields(d, vol):
    """(state fp64, V, D) of one volume of the fixture, as (s, r, c) arrays."""
    V = {k: d["%s_%s" % (vol, k)] for k in ("Vx", "Vy", "Vz")}
    D = {k: d["%s_%s" % (vol, k)] for k in D_FIELDS}
    D["D"] = D["Dxx"]
    return d["%s_C" % vol], V, D


def d_dict(D_type, D, const):
    """The D_dict entries a D_type reads (a scalar field is the fixture's Dxx)."""
    if D_type == "constant":
        return {"D": const}
    if D_type == "scalar":
        return {"D": D["D"]}
    return {k: D[k] for k in (D_FIELDS[:3] if D_type == "diag" else D_FIELDS)}


def state(C, dt):
    return C if dt == "f64" else C.astype(np.float32)


def rhs_bound(gold, want):
    """The bound on a kernel's distance to the restatement: 3 x the reference's own fp32 distance + 1e-7 max|rhs|."""
    ref_dist = float(np.abs(gold.astype(np.float64) - want).max())
    return 3 * ref_dist + 1e-7 * float(np.abs(want).max()), ref_dist
