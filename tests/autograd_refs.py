"""Float64 closed forms and derived fp32 error bounds of the per-voxel processors' backward kernels
(brainfm_amd/csrc/elementwise.hip: bfm_softmax_cl_bwd, bfm_ew_unary_bwd), and an fp32 model of them with named mistakes.

Plain helpers, no test in here: tests/test_host_autograd.py proves the closed forms against torch's float64 autograd of
oracle.train_ref.processors and shows that every bound notices every named mistake; tests/test_gpu_autograd.py holds the
HIP kernels to the bounds.  Rows are (n, C) arrays, as the kernels see a channels-last tensor.

Notation: EPS = 2^-24 is the relative error of one fp32 rounding.  The library is built with -ffp-contract=off, so a
product and the sum it enters are two roundings.  All closed forms take the kernel's OWN fp32 operands (the stored posterior
p, the stored sigmoid output y, the clamp's input x, the cotangent g) as exact float64 numbers.

softmax   dx_c = p_c (g_c - s), s = sum_j p_j g_j.  As coded: s is a chain of C products and C additions in channel order,
          |s32 - s| <= gamma_C sum_j |p_j g_j| with gamma_C = (C + 1) EPS / (1 - (C + 1) EPS) (each term passes its product's
          rounding and at most C additions); then d = fl(g_c - s32) and fl(p_c d), one rounding each:
          |dx32 - dx| <= |p_c| (gamma_C sum_j |p_j g_j| (1 + 2 EPS) + 2 EPS |g_c - s| (1 + EPS)) + 2^-149
          (2^-149: a result below the normal range is rounded to the subnormal grid).
sigmoid   dx = g y (1 - y): fl(g y), fl(1 - y) and their product, three roundings of exact factors:
          |dx32 - dx| <= ((1 + EPS)^3 - 1) |dx| + 2^-149.  A saturated output y == 1 gives exactly 0 on both sides.
clamp     dx = g where a <= x <= b, else 0: a selection, no arithmetic: the bound is 0.
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -149
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------ closed forms
def softmax_bwd64(p, g):
    p, g = np.asarray(p, F64), np.asarray(g, F64)
    s = (p * g).sum(axis=1, keepdims=True)
    return p * (g - s)


def sigmoid_bwd64(y, g):
    y, g = np.asarray(y, F64), np.asarray(g, F64)
    return g * y * (1.0 - y)


def clamp_bwd64(x, g, a, b):
    x, g = np.asarray(x, F64), np.asarray(g, F64)
    return np.where((x >= a) & (x <= b), g, 0.0)


# ------------------------------------------------------------------------------------------------------ bounds
def softmax_bwd_bound(p, g):
    p, g = np.asarray(p, F64), np.asarray(g, F64)
    C = p.shape[1]
    gamma = (C + 1) * EPS / (1.0 - (C + 1) * EPS)
    s = (p * g).sum(axis=1, keepdims=True)
    sabs = np.abs(p * g).sum(axis=1, keepdims=True)
    return np.abs(p) * (gamma * sabs * (1 + 2 * EPS) + 2 * EPS * np.abs(g - s) * (1 + EPS)) + TINY


def sigmoid_bwd_bound(y, g):
    return ((1 + EPS) ** 3 - 1) * np.abs(sigmoid_bwd64(y, g)) + TINY


def clamp_bwd_bound(x, g, a, b):
    return np.zeros(np.shape(x), F64)


# ------------------------------------------------------------------------------------------------------ fp32 models
def simulate_softmax_bwd(p, g, mistake=None):
    """The kernel's arithmetic in fp32, in its order.  mistake: 'no_sum' drops the sum_j p_j g_j term (dx = p g)."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    s = np.zeros((p.shape[0],), F32)
    if mistake != "no_sum":
        for c in range(p.shape[1]):
            s = (s + (p[:, c] * g[:, c]).astype(F32)).astype(F32)
    return (p * (g - s[:, None]).astype(F32)).astype(F32)


def simulate_unary_bwd(op, v, g, a=0.0, b=0.0, mistake=None, x=None):
    """op 'sigmoid': v is the OUTPUT y; mistake 'from_input' forms y (1 - y) from the INPUT x instead (x given).
    op 'clamp': v is the INPUT x; mistake 'exclusive' uses a < x < b."""
    v, g = np.asarray(v, F32), np.asarray(g, F32)
    if op == "sigmoid":
        if mistake == "from_input":
            v = np.asarray(x, F32)
        return ((g * v).astype(F32) * (F32(1.0) - v).astype(F32)).astype(F32)
    if op == "clamp":
        a, b = F32(a), F32(b)
        keep = ((v > a) & (v < b)) if mistake == "exclusive" else ((v >= a) & (v <= b))
        return np.where(keep, g, F32(0.0)).astype(F32)
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------------ cases
def softmax_case(C, n, seed):
    """(logits x, cotangent g) of n rows: random rows, the first one one-hot-sharp (one logit 60 above the rest: the
    posterior is 1 and exact zeros in fp32), the second one uniform."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, C)) * 3.0).astype(F32)
    g = rng.standard_normal((n, C)).astype(F32)
    x[0] = -30.0
    x[0, C // 2] = 30.0
    if n > 1:
        x[1] = 0.25
    return x, g


def softmax32(x):
    """A posterior as the forward stores it: float64 softmax rounded to fp32 (the backward takes p as given)."""
    x = np.asarray(x, F64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def sigmoid_case(n, seed):
    """Inputs with saturated entries: x = 40 (y == 1 in fp32 and fp64 arithmetic alike), x = -110 (y underflows to 0 in
    fp32), x = 20 (y == 1 in fp32 only)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 4.0).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    x[:3] = (40.0, -110.0, 20.0)
    return x, g


def sigmoid32(x):
    return (1.0 / (1.0 + np.exp(-np.asarray(x, F64)))).astype(F32)


def clamp_case(n, seed, a=-3.0, b=3.0):
    """Inputs on both sides of [a, b], with entries exactly on each edge, just outside each edge, and a NaN."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 3.0).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    x[:5] = (a, b, np.nextafter(F32(a), F32(-np.inf)), np.nextafter(F32(b), F32(np.inf)), np.nan)
    return x, g


def check(got, ref, bound, what):
    """Element-wise |got - ref| <= bound; returns the worst ratio (error / bound) over the elements with a non-zero bound."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d elements over the bound, worst |err| %.3e against %.3e" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad].max()))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
