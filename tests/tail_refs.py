"""Float64 references, derived error bounds and the case list of the fused network tail (brainfm_amd/csrc/tail_heads.hip)
and of the per-voxel kernels beside it (csrc/elementwise.hip, bfm_head_bias_lrelu of csrc/head_layers.hip).

Plain helpers, no test in here: tests/test_host_tail_refs.py pins them on the CPU (to tests/golden/tail_edges.npz, the
reference implementation's own results), tests/test_gpu_tail_kernels.py compares the HIP kernels with them.  Features are
channels-last (nvox, c_feat), head weights (n_out, c_feat), as the kernel sees them.

Stage A is normalise + head GEMM + bias, stage B everything after it, checked as float64 functions of the kernel's OWN raw
logits so that no GEMM error enters those tolerances.  `simulate` is an fp32 model of the kernel with named mistakes, which
the host test uses to show that check_stage_a / check_stage_b would notice each of them.

Notation: EPS = 2^-24 is the relative error of one fp32 rounding, one ulp <= 2 EPS relative.

---------------------------------------------------------------------------------------------------- stage A, bound (a)
stage_a_emulation follows the arithmetic as coded and keeps every product and sum exact (float64):
  inv   = 1 / max(sqrtf(ss), 1e-12f), ss = two fmaf chains over the two halves of the row, added          (inv_norm32)
  split: a = fp32(x * (inv 2^14)); hi = fp16 by truncation toward zero, lo = fp16 trunc of (a - hi)        (rtz16)
         w' = w 2^wexp; whi, wlo by round-to-nearest; acc = sum lo*whi + hi*wlo + hi*whi; e = acc * dq + bias
  fp32:  a = fp32(x * inv); e = sum a*w + bias
What the kernel adds to that is the fp32 accumulation of the matrix core, at most one rounding per product of a chain of
c_feat: |raw - e| <= c_feat EPS sum_k |a_k w_k|, and the single rounding of the last fmaf / add, EPS |e| (step 5 of the
arithmetic itself: the emulation is not rounded, the kernel's result is).  (The fmaf chains of ss are emulated as a float64
product-sum rounded to fp32; the double rounding can differ from a true fmaf once in about 2^29 operations.)

---------------------------------------------------------------------------------------------------- stage A, bound (b)
against t = normalize(x) @ W^T + b in float64, u = normalize(x) (stage_a_true_bound), per logit, first order:
  inv: ss carries <= 33 EPS (32 fmaf + the shuffle add, all terms positive), halved by the root; sqrtf, the division and
       the product x * inv one EPS each: 33/2 + 3 = 19.5, taken as NORM_ROUNDINGS = 20 for the second-order terms.  This
       is also the element-wise bound of feat_norm.  Below the 1e-12 floor the constant's own rounding replaces the root.
       -> 20 EPS sum |u_k w_k|        (nothing when unit_feat = 0: inv = 1 exactly)
  accumulation and the last rounding as in (a): c_feat EPS sum |u_k w_k| + EPS |t|
  split routes only, in units scaled by 2^14 (features, A = 2^14 |u|) and 2^wexp (weights, w'), times dq = 2^-(wexp+14):
    truncating split of a feature: |a - hi - lo| < spacing(lo) <= max(2^-20 A, 2^-24)     (2^-24: the fp16 subnormal floor)
    rounded split of a weight:     |w' - whi - wlo| <= max(2^-22 w', 2^-25)
    dropped lo*lo:                 |alo| < 2^-10 A, |wlo| <= max(2^-11 w', 2^-25)
With head_wmax around 1e-30 the exponent is clamped at wexp = 60, w' is around 1e-12 and below the fp16 subnormals: whi =
wlo = 0, the kernel returns the bias alone, and this bound (about c_feat 2^-85) allows exactly that.

---------------------------------------------------------------------------------------------------- stage B
exp and sigmoid use expf: compared in ulps of the float64 value (ulps32).  fake_cortical and the softmax use v_exp_f32 and
v_rcp_f32 (1 ulp each) on an argument scaled by log2 e in fp32:
  softmax_bound: d = fp32(x - m) (EPS |d|), fp32(d L) with L = fp32(log2 e) (2 EPS of the argument), so exp2's argument is
       off by 3 EPS |d| log2 e and e_s by 3 EPS |d| relative, plus 2 EPS for the instruction: r_s = (3 |d_s| + 2) EPS.
       The sum carries sum_s p_s r_s + (n - 1) EPS, the reciprocal 2 EPS, the product EPS:
       |p - p64| <= p (r_s + sum_s p_s r_s + (n + 2) EPS) + 2^-126   (results below the normal range may be flushed)
  SOFTMAX_DELTA: two classes can change order only through their own e_s and the last product (the sum and 1/sum are
       shared and the product is monotone): 2 (2 EPS + EPS) = 6 EPS of the ratio, plus the roundings of d: 8 EPS in logits.
  fake_bound: per term gain * (1 - (tanh(2 s) + 1) / 2), s = fp32(v + add): s is off by EPS (|s| + |add|) (the rounding and
       the constant 0.3f), e = exp(4 s) relatively by 4 EPS (|s| + |add|) + 2 EPS |4 s| + 2 EPS, tanh by that times
       2 e / (e + 1)^2, plus 5 EPS |tanh| (e - 1, e + 1, rcp 2, product); + 1, 1 - and the gain one EPS each; clamping
       2 s at +-15 changes tanh by < 2 exp(-30); every addition of terms one EPS of the partial sum.
"""
import math

import numpy as np

from conv_forward_refs import prescale_exp

EPS = 2.0 ** -24
NORM_ROUNDINGS = 20.0
SOFTMAX_DELTA = 8 * EPS
ULP_CAP = 8.0
PLAIN, CT, BIAS_LOG, SEG, DIST, SR, PATHOL = range(7)
LABELS_LEFT = [0, 1, 2, 3, 4, 7, 8, 9, 10, 14, 15, 17, 31, 34, 36, 38, 40, 42]
LABELS_FULL = [0, 11, 12, 13, 16, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 46,
               1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 17, 47, 49, 51, 53, 55,
               18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 48, 50, 52, 54, 56]
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------ head sets
MAX_ROW_MAPS = 60            # the kernel takes at most 64 maps: rows beyond the 60th map of a set have no map (slot -1)


def head_spec(groups, max_dist=3.0, lut=None):
    """groups: [(role, channels)] in head-row order.  Map slots in row order (segmentation rows have none), then one slot
    per super-resolution channel for high_res, then fake_cortical: the layout engine.Tail builds."""
    roles, slots, n_maps = [], [], 0
    s = dict(seg_first=0, n_seg=0, dist_first=0, n_dist=0, sr_first=0, n_sr=0)
    for role, n in groups:
        if role == SEG:
            s["seg_first"], s["n_seg"] = len(roles), n
        elif role == DIST:
            s["dist_first"], s["n_dist"] = len(roles), n
        elif role == SR:
            s["sr_first"], s["n_sr"] = len(roles), n
        for _ in range(n):
            roles.append(role)
            has_map = role != SEG and n_maps < MAX_ROW_MAPS
            slots.append(n_maps if has_map else -1)
            n_maps += has_map
    s["slot_high_res"] = n_maps if s["n_sr"] else -1
    n_maps += s["n_sr"]
    s["slot_fake"] = n_maps if s["n_dist"] else -1
    n_maps += 1 if s["n_dist"] else 0
    if lut is None:
        ns = s["n_seg"]
        lut = LABELS_FULL if ns == 56 else LABELS_LEFT if ns == 18 else [(5 + 3 * i) % 251 for i in range(ns)]
    s.update(roles=np.array(roles, np.int32), out_slot=np.array(slots, np.int32), n_maps=n_maps, n_out=len(roles),
             lut=np.array(lut, np.int32), max_dist=float(max_dist))
    return s


_REG = [(PLAIN, 3), (CT, 1), (BIAS_LOG, 1)]
HEAD_SETS = {
    # process_args' order: T1 T2 FLAIR CT bias_field_log segmentation distance registration high_res_residual [pathology]
    "full69": _REG + [(SEG, 56), (DIST, 4), (PLAIN, 3), (SR, 1)],
    "left29": _REG + [(SEG, 18), (DIST, 2), (PLAIN, 3), (SR, 1)],            # what process_args gives with left_hemis_only
    "left27": [(PLAIN, 2), (BIAS_LOG, 1), (SEG, 18), (DIST, 2), (PLAIN, 3), (SR, 1)],   # the 27 outputs tail_launch names
    "seg20_first7": [(PLAIN, 2), (CT, 1), (PATHOL, 1), (BIAS_LOG, 1), (SR, 1), (PLAIN, 1), (SEG, 20), (DIST, 2)],
    "seg70": [(PLAIN, 1), (SEG, 70), (CT, 1)],
    "seg96": [(SEG, 96)],
    # more than 16 non-segmentation outputs, one role of each kind beyond the 16th (the LDS-table fallback, nplain > PMAX)
    "uncert": [(PLAIN, 17), (SEG, 18), (CT, 2), (BIAS_LOG, 2), (PATHOL, 1), (DIST, 4), (SR, 2)],
    "sr2": [(PLAIN, 1), (SR, 2), (SEG, 5)],
    "dist2": [(DIST, 2), (PLAIN, 1)],
    "dist4": [(PLAIN, 1), (DIST, 4)],
    "noseg": [(PLAIN, 2), (CT, 1), (BIAS_LOG, 1), (PATHOL, 1), (SR, 1)],
    "big": [(PLAIN, 1), (SR, 2), (SEG, 5), (CT, 1)],
}
GOLDEN_SETS = ("full69", "left29", "seg20_first7", "uncert")         # the reference has a head layout for these
GOLDEN_NVOX = 40
# the same sets as the reference's TaskHead sees them: ordered (task, channels); get_postprocessor goes by name
GOLDEN_TASKS = {
    "full69": [("T1", 1), ("T2", 1), ("FLAIR", 1), ("CT", 1), ("bias_field_log", 1), ("segmentation", 56), ("distance", 4),
               ("registration", 3), ("high_res_residual", 1)],
    "left29": [("T1", 1), ("T2", 1), ("FLAIR", 1), ("CT", 1), ("bias_field_log", 1), ("segmentation", 18), ("distance", 2),
               ("registration", 3), ("high_res_residual", 1)],
    "seg20_first7": [("T1", 1), ("T2", 1), ("CT", 1), ("pathology", 1), ("bias_field_log", 1), ("high_res_residual", 1),
                     ("FLAIR", 1), ("segmentation", 20), ("distance", 2)],
    "uncert": [("T1", 2), ("T2", 2), ("FLAIR", 2), ("registration", 3), ("surface", 8), ("segmentation", 18), ("CT", 2),
               ("bias_field_log", 2), ("pathology", 1), ("distance", 4), ("high_res_residual", 2)],
}
TASK_ROLE = {"CT": CT, "bias_field_log": BIAS_LOG, "segmentation": SEG, "distance": DIST, "high_res_residual": SR,
             "pathology": PATHOL}


def golden_case(name):
    """Operands of a golden head set: 64 features, logits and biases of a few units (so that the distance clamp, the CT
    scale and the exponentials all see values on both sides of their thresholds), one all-zero row and one of norm 1e-20."""
    spec = head_spec(HEAD_SETS[name])
    x, W, b = operands(64, spec["n_out"], GOLDEN_NVOX, 40 + sorted(HEAD_SETS).index(name), wscale=4.0)
    x[3] = 0
    x[5] *= F32(1e-20 / np.sqrt((x[5].astype(F64) ** 2).sum()))
    return spec, x, W, b, image_input(GOLDEN_NVOX, 7)


def tail_route(c_feat, n_out, n_seg, unit_feat, wmax):
    """bfm_tail_route: 0 fp32 chain, 1 split generic, 2 split <56, 3>, 3 split <18, 1>."""
    w = float(np.float32(wmax))
    if not (unit_feat and w > 0.0 and math.isfinite(w) and c_feat % 16 == 0):
        return 0
    nnb = (n_out + 31) >> 5
    return 2 if (n_seg == 56 and nnb == 3) else 3 if (n_seg == 18 and nnb == 1) else 1


def operands(c_feat, n_out, nvox, seed, fscale=1.0, wscale=1.0, bscale=None):
    """Random features, ASYMMETRIC weights (row o is scaled by 0.5 + o / n_out and column k by 1 + k / (2 c): no two rows
    or columns are exchangeable) and biases as large as the logits of unit features (N(0, 0.5))."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(nvox, c_feat) * fscale).astype(F32)
    W = rs.randn(max(n_out, 1), c_feat) * 0.5
    W *= (0.5 + np.arange(max(n_out, 1))[:, None] / max(n_out, 1)) * (1 + np.arange(c_feat)[None] / (2.0 * c_feat))
    W = (W * wscale).astype(F32)[:n_out]
    b = (rs.randn(n_out) * (0.5 * wscale if bscale is None else bscale)).astype(F32)
    return x, W, b


GRID_C, GRID_N, GRID_V = (8, 16, 24, 48, 64), (1, 31, 32, 33, 64, 65, 96), (1, 63, 64, 65, 257)


def stage_a_grid():
    """[(c_feat, n_out, unit_feat, nvox, seed)]: 70 cases in which every pair of values of any two of the four factors
    occurs (all 35 (c_feat, n_out) pairs under both unit_feat; the host test counts the pairs)."""
    return [(GRID_C[i % 5], GRID_N[i % 7], i // 35, GRID_V[(i % 35 // 7 + i) % 5], 100 + i) for i in range(70)]


def image_input(nvox, seed=0):
    return (np.random.RandomState(1000 + seed).rand(nvox) + 0.25).astype(F32)


# ------------------------------------------------------------------------------------------------------------ stage A
def normalize64(x):
    x = np.asarray(x, F64)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def inv_norm32(x):
    """The kernel's 1 / max(||x||, 1e-12) in fp32: one fmaf chain per half of the row, the two added, sqrtf, one division."""
    x = np.asarray(x, F32)
    half = x.shape[1] // 2
    ss = []
    with np.errstate(all="ignore"):
        for h in (0, 1):
            s = np.zeros(x.shape[0], F32)
            for k in range(half):
                v = x[:, h * half + k].astype(F64)
                s = (v * v + s.astype(F64)).astype(F32)
            ss.append(s)
        return F32(1.0) / np.maximum(np.sqrt(ss[0] + ss[1]), F32(1e-12))


def rtz16(v):
    """fp16 by truncation toward zero (v_cvt_pkrtz_f16_f32) of exact fp32 values, as float64."""
    v = np.asarray(v, F64)
    av = np.abs(v)
    _, e = np.frexp(av)
    q = np.where(av >= 2.0 ** -14, np.ldexp(1.0, e - 11), 2.0 ** -24)
    return np.copysign(np.minimum(np.floor(av / q) * q, 65504.0), v)


def split_weights(W, wexp):
    w = np.asarray(W, F32) * F32(2.0 ** wexp)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(F32)).astype(np.float16)
    return hi.astype(F64), lo.astype(F64), w.astype(F64)


def stage_a_emulation(x, W, b, unit_feat, wmax, terms=("lh", "hl", "hh"), swap_halves=False, drop_kstep=None,
                      bias_first=False):
    """(e, absum): the unrounded logits of the arithmetic as coded and sum_k |a_k w_k| per logit (module docstring).
    The keyword arguments are the mistakes of the host test."""
    x = np.asarray(x, F32)
    W, b = np.asarray(W, F32), np.asarray(b, F32).astype(F64)
    n, c = x.shape
    route = tail_route(c, W.shape[0], 0, unit_feat, wmax)
    inv = inv_norm32(x) if unit_feat else np.ones(n, F32)
    with np.errstate(all="ignore"):
        if route == 0:
            a = (x * inv[:, None]).astype(F64)
            wq, dq = W.astype(F64), 1.0
        else:
            wexp = prescale_exp(np.float32(wmax))
            a = (x * (inv * F32(16384.0))[:, None]).astype(F64)
            dq = 2.0 ** -(wexp + 14)
        if swap_halves:
            a = np.concatenate([a[:, c // 2:], a[:, :c // 2]], 1)
        if drop_kstep is not None:                      # k-step ks: 8 channels of each half
            a = a.copy()
            for h in (0, 1):
                a[:, h * (c // 2) + 8 * drop_kstep:h * (c // 2) + 8 * drop_kstep + 8] = 0
        if route == 0:
            acc = a @ wq.T
            absum = np.abs(a) @ np.abs(wq).T
        else:
            hi = rtz16(a)
            lo = rtz16(a - hi)
            whi, wlo, wq = split_weights(W, wexp)
            ops = {"hh": (hi, whi), "hl": (hi, wlo), "lh": (lo, whi)}
            acc = sum(ops[t][0] @ ops[t][1].T for t in terms)
            absum = (np.abs(a) @ np.abs(wq).T) * dq
        e = (acc + b) * dq if bias_first else acc * dq + b
    return e, absum


def stage_a_bound(e, absum, c_feat):
    with np.errstate(invalid="ignore"):
        return c_feat * EPS * absum + EPS * np.abs(e)


def stage_a_true(x, W, b, unit_feat):
    u = normalize64(x) if unit_feat else np.asarray(x, F64)
    W = np.asarray(W, F64)
    return u @ W.T + np.asarray(b, F64), u


def stage_a_true_bound(x, W, b, unit_feat, wmax):
    """(t, bound): the float64 logits and the per-logit bound (b) of the module docstring."""
    t, u = stage_a_true(x, W, b, unit_feat)
    c = u.shape[1]
    au, aw = np.abs(u), np.abs(np.asarray(W, F64))
    absum = au @ aw.T
    ea = NORM_ROUNDINGS * EPS if unit_feat else 0.0
    bound = ea * absum + c * EPS * absum * (1 + ea) + EPS * np.abs(t)
    if tail_route(c, aw.shape[0], 0, unit_feat, wmax):
        wexp = prescale_exp(np.float32(wmax))
        A, ws = au * 16384.0 * (1 + ea), aw * 2.0 ** wexp
        r = np.maximum(2.0 ** -20 * A, 2.0 ** -24)
        s = np.maximum(2.0 ** -22 * ws, 2.0 ** -25)
        lolo = (2.0 ** -10 * A) @ np.maximum(2.0 ** -11 * ws, 2.0 ** -25).T
        bound = bound + (r @ ws.T + A @ s.T + lolo) * 2.0 ** -(wexp + 14)
    return t, bound


def feat_norm_bound(x):
    u = normalize64(x)
    return u, NORM_ROUNDINGS * EPS * np.abs(u) + 2.0 ** -149


def _ratio(diff, bound):
    """max diff / bound; 0 / 0 counts as 0, anything over a zero bound as inf."""
    diff, bound = np.asarray(diff, F64), np.asarray(bound, F64)
    if diff.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.where(diff == 0, 0.0, diff / bound)
    return float(np.nanmax(np.where(np.isnan(r), np.inf, r)))


def check_stage_a(raw, x, W, b, unit_feat, wmax, feat_norm=None):
    """Asserts raw (nvox, n_out) fp32 against both bounds; returns {'emul': ratio, 'true': ratio, 'fn': ratio}."""
    raw = np.asarray(raw, F32)
    c = np.asarray(x).shape[1]
    out = {}
    if raw.shape[1]:
        e, absum = stage_a_emulation(x, W, b, unit_feat, wmax)
        fin = np.isfinite(e)
        assert np.array_equal(np.isfinite(raw), fin), "finite pattern of the logits"
        assert np.array_equal(np.isnan(raw), np.isnan(e)) and np.array_equal(raw[~fin & ~np.isnan(e)], e[~fin & ~np.isnan(e)])
        out["emul"] = _ratio(np.abs(raw.astype(F64) - e)[fin], stage_a_bound(e, absum, c)[fin])
        t, tb = stage_a_true_bound(x, W, b, unit_feat, wmax)
        out["true"] = _ratio(np.abs(raw.astype(F64) - t)[fin], tb[fin])
        assert out["emul"] <= 1.0, "emulation bound: ratio %g" % out["emul"]
        assert out["true"] <= 1.0, "float64 bound: ratio %g" % out["true"]
    if feat_norm is not None and not unit_feat:
        assert bits_equal(feat_norm, x), "feat_norm without unit_feat is the copy"
        out["fn"] = 0.0
    elif feat_norm is not None:
        u, fb = feat_norm_bound(x)
        fin = np.isfinite(u)
        out["fn"] = _ratio(np.abs(np.asarray(feat_norm, F64) - u)[fin], fb[fin])
        assert out["fn"] <= 1.0, "feat_norm bound: ratio %g" % out["fn"]
    return out


# ------------------------------------------------------------------------------------------------------------ stage B
def ulps32(got, ref64):
    """Distance in fp32 ulps of the float64 value (0 where both are the same infinity)."""
    got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(ref64).astype(F32)).astype(F64)
        d = np.abs(got - ref64) / sp
    return np.where((got == ref64) | (np.isnan(got) & np.isnan(ref64)), 0.0, np.where(np.isnan(d), np.inf, d))


def softmax64(z):
    """softmax of fp32 logits in float64, with torch's non-finite results (a +inf or NaN member makes the row NaN)."""
    z = np.asarray(z, F64)
    with np.errstate(all="ignore"):
        m = z.max(1, keepdims=True)
        e = np.exp(z - m)
        return e / e.sum(1, keepdims=True)


def softmax_bound(z, arg_roundings=3):
    """arg_roundings = 3: the tail (exp2 of an argument scaled in fp32); 1: bfm_softmax_cl, whose expf (taken at 1 ulp,
    as its documentation states, like v_exp_f32) sees fp32(x - m) itself and whose division is one rounding."""
    z = np.asarray(z, F64)
    p = softmax64(z)
    with np.errstate(all="ignore"):
        d = np.abs(z - z.max(1, keepdims=True))
        r = (arg_roundings * np.where(np.isfinite(d), d, 0.0) + 2) * EPS
        return p * (r + (p * r).sum(1, keepdims=True) + (z.shape[1] + 2) * EPS) + 2.0 ** -126


def _fake_term64(v, add, gain):
    return gain * (1 - (np.tanh(2 * (v + add)) + 1) / 2)


def fake_cortical64(d, lp=0, lw=1):
    """Trainer/models/__init__.py:321-337 on clamped fp32 distances d (nvox, 2 | 4): order lp, lw[, rp, rw]."""
    d = np.asarray(d, F64)
    f = _fake_term64(d[:, lw], 0.3, 70.0) + _fake_term64(d[:, lp], 0.0, 40.0)
    if d.shape[1] == 4:
        f = f + (_fake_term64(d[:, 3], 0.3, 70.0) + _fake_term64(d[:, 2], 0.0, 40.0))
    return f


def fake_bound(d, tanh_ulps=None):
    """tanh_ulps: bfm_fake_cortical, which calls tanhf (so many ulps of tanh in place of the exp / rcp terms)."""
    d = np.asarray(d, F64)
    tot, mag = 0.0, 0.0
    for col, add, gain in ((1, 0.3, 70.0), (0, 0.0, 40.0), (3, 0.3, 70.0), (2, 0.0, 40.0))[:d.shape[1]]:
        s = np.abs(d[:, col] + add)
        y4 = np.minimum(4 * s, 30.0)
        sech = 2 * np.exp(-y4) / (1 + np.exp(-y4)) ** 2                 # 2 e / (e + 1)^2
        th = np.tanh(2 * np.minimum(s, 7.5))
        if tanh_ulps is None:
            a_th = (4 * (s + add) + 2 * y4 + 2) * EPS * sech + 5 * EPS * th + 2 * math.exp(-30.0)
        else:
            a_th = 4 * (s + add) * EPS * sech + tanh_ulps * 2 * EPS * th
        term = np.abs(_fake_term64(d[:, col], add, gain))
        tot = tot + gain * (a_th / 2 + 2 * EPS) + EPS * term
        mag = mag + term
    return tot + 3 * EPS * mag


def gate_keep(inp, nvox):
    """True per voxel where the zero-input gate leaves the outputs unwritten: its chunk of 64 is ALL zero."""
    nch = (nvox + 63) // 64
    z = np.zeros(nch * 64, bool)
    z[:nvox] = np.asarray(inp) != 0
    return np.repeat(~z.reshape(nch, 64).any(1), 64)[:nvox]


def chunk_slot(nvox, blocks_cap=512, wpb=4):
    """(slot k, lap) of every chunk of 64 voxels in the kernel's group-of-four schedule."""
    nch = (nvox + 63) // 64
    cstride = min((nch + wpb - 1) // wpb, blocks_cap) * wpb
    c = np.arange(nch)
    return (c // cstride) % 4, c // (4 * cstride), cstride


# The grid is capped at 512 blocks of 4 waves, so chunk c sits in slot (c // 2048) % 4 of its wave's group and in lap
# c // 8192: slot 1 from 131 072 voxels on, slots 2 and 3 from 262 144 and 393 216, the second lap from 524 288.
BIG_NVOX = (131072 + 3 * 64 + 5, 3 * 131072 + 64 + 7, 524288 + 64 + 7)


def slot_pattern_input(nvox):
    """Zero on the chunks with (c + 2 (c // 2048)) % 3 == 0 (so chunk c + 2048, one slot further on, is never in the same
    state as a zero chunk), distinct non-zero values elsewhere."""
    v = np.arange(nvox)
    c = v // 64
    return np.where((c + 2 * (c // 2048)) % 3 == 0, 0.0, 0.5 + (v % 8191) / 8192.0).astype(F32)


def gate_input(nvox):
    """For 64 * 5 + 9 voxels: chunk 0 all zero, 1 non-zero at lane 0 only, 2 at lane 63 only, 3 all zero, 4 non-zero but
    for a few voxels, the partial last chunk non-zero at its last voxel only."""
    assert nvox == 64 * 5 + 9
    inp = np.zeros(nvox, F32)
    inp[64], inp[191], inp[nvox - 1] = 0.5, -2.0, 1e-30
    inp[256:320] = image_input(64, 3)
    inp[[257, 300]] = 0
    return inp


def clamp32(a, md):
    """fminf(fmaxf(a, -md), md): a NaN logit comes out as -md (fmaxf returns its other operand), where torch.clamp keeps
    the NaN -- the documented behaviour of the DIST role and of BFM_EW_CLAMP (include/brainfm_hip.h)."""
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), -F32(md), np.minimum(np.maximum(a, -F32(md)), F32(md))).astype(F32)


def processors64(raw, spec, inp=None):
    """Everything after the GEMM as float64 functions of fp32 logits raw (nvox, n_out).  Returns per map slot
    (kind, value[, bound]): kind 'bits' (value is the fp32 result), 'ulp_exp' / 'ulp_sigmoid' (float64 value, compared in
    ulps), 'abs' (float64 value, bound);
    'none' for a slot nothing writes; plus seg (float64) or None."""
    raw = np.asarray(raw, F32)
    maps = [("none", None)] * spec["n_maps"]
    md = F32(spec["max_dist"])
    with np.errstate(all="ignore"):
        for o, (role, slot) in enumerate(zip(spec["roles"], spec["out_slot"])):
            a = raw[:, o]
            if role == SEG or slot < 0:
                continue
            if role == CT:
                maps[slot] = ("bits", a * F32(1000.0))
            elif role == BIAS_LOG:
                maps[slot] = ("ulp_exp", np.exp(a.astype(F64)))
            elif role == PATHOL:
                maps[slot] = ("ulp_sigmoid", 1.0 / (1.0 + np.exp(-a.astype(F64))))
            elif role == DIST:
                maps[slot] = ("bits", clamp32(a, md))
            else:
                maps[slot] = ("bits", a)
        if spec["n_sr"] and spec["slot_high_res"] >= 0 and inp is not None:
            for j in range(spec["n_sr"]):
                maps[spec["slot_high_res"] + j] = ("bits", raw[:, spec["sr_first"] + j] + np.asarray(inp, F32))
        if spec["n_dist"] and spec["slot_fake"] >= 0:
            d = clamp32(raw[:, spec["dist_first"]:spec["dist_first"] + spec["n_dist"]], md)
            maps[spec["slot_fake"]] = ("abs", fake_cortical64(d), fake_bound(d))
        seg = softmax64(raw[:, spec["seg_first"]:spec["seg_first"] + spec["n_seg"]]) if spec["n_seg"] else None
    return maps, seg


def bits_equal(a, b):
    """Same fp32 bits, any NaN equal to any NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check_stage_b(raw, maps, seg, label, label_fast, spec, inp=None, keep=None, ulp_limit=None, random_case=False):
    """maps (n_maps, nvox) fp32, seg (nvox, n_seg) or None, label / label_fast (nvox,) int64 or None (with / without
    seg_prob in the call) against processors64(raw).  keep: voxels the gate leaves unwritten (not compared here).
    ulp_limit: {'ulp_exp': limit, 'ulp_sigmoid': limit} (default: ULP_CAP each).
    Returns the worst figures: {'ulp_exp', 'ulp_sigmoid', 'fake', 'softmax', 'softmax_n', 'near'} (softmax_n: the softmax
    ratio over the probabilities above 2^-100 alone; a probability flushed just under 2^-126 has ratio 1 by construction)."""
    ulp_limit = ulp_limit or {"ulp_exp": ULP_CAP, "ulp_sigmoid": ULP_CAP}
    raw = np.asarray(raw, F32)
    n = raw.shape[0]
    live = np.ones(n, bool) if keep is None else ~keep
    ref, seg64 = processors64(raw, spec, inp)
    if keep is not None:                                # the gate: nothing of an all-zero chunk is written
        assert all(np.isnan(maps[slot][keep]).all() for slot, r in enumerate(ref) if r[0] != "none"), "gated chunk written"
        assert seg is None or np.isnan(np.asarray(seg)[keep]).all(), "gated chunk: seg_prob written"
        assert all(l is None or (l[keep] == -1).all() for l in (label, label_fast)), "gated chunk: label written"
    out = {"ulp_exp": 0.0, "ulp_sigmoid": 0.0, "fake": 0.0, "softmax": 0.0, "softmax_n": 0.0, "near": 0.0}
    for slot, r in enumerate(ref):
        got = maps[slot][live]
        if r[0] == "bits":
            assert bits_equal(got, r[1][live]), "map %d differs from its fp32 definition" % slot
        elif r[0].startswith("ulp"):
            out[r[0]] = max(out[r[0]], float(ulps32(got, r[1][live]).max(initial=0.0)))
        elif r[0] == "abs":
            fin = ~np.isnan(r[1][live])
            assert np.array_equal(np.isnan(got), ~fin), "NaN pattern of map %d" % slot
            out["fake"] = max(out["fake"], _ratio(np.abs(got.astype(F64) - r[1][live])[fin], r[2][live][fin]))
    for k, lim in ulp_limit.items():
        assert out[k] <= lim, "%s: %g ulp, limit %g" % (k, out[k], lim)
    assert out["fake"] <= 1.0, "fake_cortical: ratio %g" % out["fake"]
    if spec["n_seg"]:
        z = raw[:, spec["seg_first"]:spec["seg_first"] + spec["n_seg"]][live]
        lut = spec["lut"]
        if seg is not None:
            s, s64 = np.asarray(seg, F32)[live], seg64[live]
            assert np.array_equal(np.isnan(s), np.isnan(s64)), "NaN rows of the softmax"
            fin = ~np.isnan(s64)
            sb = softmax_bound(z)
            out["softmax"] = _ratio(np.abs(s.astype(F64) - s64)[fin], sb[fin])
            big = fin & (s64 >= 2.0 ** -100)            # for the record: without the probabilities at the flush floor
            out["softmax_n"] = _ratio(np.abs(s.astype(F64) - s64)[big], sb[big])
            assert out["softmax"] <= 1.0, "softmax: ratio %g" % out["softmax"]
            if label is not None:
                first = np.where(np.isnan(s).any(1), 0, np.argmax(np.where(np.isnan(s), -1, s), 1))
                assert np.array_equal(label[live], lut[first]), "label != lut[first argmax of the returned seg_prob]"
        if label is not None and label_fast is not None:
            assert np.array_equal(label[live], label_fast[live]), "label with and without seg_prob differ"
        lab = label if label is not None else label_fast
        if lab is not None:
            ok_rows = np.isfinite(z).all(1)
            zz = z[ok_rows].astype(F64)
            m = zz.max(1, keepdims=True)
            allowed = zz >= m - SOFTMAX_DELTA
            got = lab[live][ok_rows]
            hit = (lut[None, :] == got[:, None]) & allowed
            assert hit.any(1).all(), "label is not a class within delta of the largest logit"
            srt = np.sort(zz, 1)
            near = (srt[:, -1] - srt[:, -2] <= SOFTMAX_DELTA) if zz.shape[1] > 1 else np.zeros(len(zz), bool)
            clear = ~near
            assert np.array_equal(got[clear], lut[np.argmax(zz[clear], 1)]), "label != lut[argmax raw] at a clear voxel"
            out["near"] = float(near.mean()) if len(near) else 0.0
            if random_case:
                assert out["near"] <= 1e-3, "%g of the voxels within delta" % out["near"]
    return out


# ------------------------------------------------------------------------------------------------------------ simulator
def simulate(x, W, b, spec, unit_feat, wmax, inp=None, gate=False, mistake=None):
    """An fp32 model of the kernel: the emulation rounded once, the processors from float64 rounded once.  Unwritten
    outputs are NaN (maps, seg) and -1 (label).  mistake: one of MISTAKES."""
    kw = {"swap_halves": dict(swap_halves=True), "drop_kstep": dict(drop_kstep=0), "lost_lo": dict(terms=("hl", "hh")),
          "bias_first": dict(bias_first=True)}.get(mistake, {})
    e, _ = stage_a_emulation(x, W, b, unit_feat, wmax, **kw)
    with np.errstate(all="ignore"):
        raw = e.astype(F32)
    n = raw.shape[0]
    sp = dict(spec)
    inp_seen = inp
    if mistake == "ivq_slot" and inp is not None:       # slot k reads the input of slot k + 1: cstride chunks further on
        cs = chunk_slot(n)[2] * 64
        pad = np.concatenate([np.asarray(inp, F32), np.zeros(cs, F32)])
        inp_seen = pad[cs:cs + n]
    ref, seg64 = processors64(raw, sp, inp_seen)
    maps = np.full((spec["n_maps"], n), np.nan, F32)
    with np.errstate(all="ignore"):
        for slot, r in enumerate(ref):
            if r[0] != "none":
                maps[slot] = r[1].astype(F32)
        if mistake == "lp_lw" and spec["n_dist"]:
            d = np.clip(raw[:, spec["dist_first"]:spec["dist_first"] + spec["n_dist"]], -spec["max_dist"], spec["max_dist"])
            maps[spec["slot_fake"]] = fake_cortical64(d, lp=1, lw=0).astype(F32)
        if mistake == "clamp_ct":
            for o, role in enumerate(spec["roles"]):
                if role == CT:
                    maps[spec["out_slot"][o]] = np.clip(raw[:, o], -F32(spec["max_dist"]), F32(spec["max_dist"])) * F32(1000)
        if mistake == "high_res_slot" and spec["n_sr"] and inp is not None:
            hr, rs_ = spec["slot_high_res"], spec["out_slot"][spec["sr_first"]]
            maps[[hr, rs_]] = maps[[rs_, hr]]
        seg = label = None
        if spec["n_seg"]:
            seg = seg64.astype(F32)
            nanrow = np.isnan(seg).any(1)
            filled = np.where(np.isnan(seg), -1, seg)
            best = np.argmax(filled, 1)
            if mistake == "last_max":
                best = seg.shape[1] - 1 - np.argmax(filled[:, ::-1], 1)
            best = np.where(nanrow, 0, best)
            if mistake == "lut_offset":
                best = np.minimum(best + spec["seg_first"], spec["n_seg"] - 1)
            label = spec["lut"][best].astype(np.int64)
    if gate and inp is not None:
        keep = gate_keep(inp_seen, n) if mistake != "gate_any" else np.repeat(
            (np.pad(np.asarray(inp_seen) == 0, (0, -n % 64), constant_values=False).reshape(-1, 64)).any(1), 64)[:n]
        maps[:, keep] = np.nan
        if seg is not None:
            seg[keep] = np.nan
            label[keep] = -1
    return dict(raw=raw, maps=maps, seg=seg, label=label)


MISTAKES = ("swap_halves", "drop_kstep", "lost_lo", "bias_first", "lp_lw", "clamp_ct", "last_max", "lut_offset", "ivq_slot",
            "gate_any", "high_res_slot")


# ------------------------------------------------------------------------------------------------------------ planted logits
GAPS = (0.0, "ulp", 5e-6, 9.9e-6, 1.01e-5, 2e-5, 1e-3)


def planted_rows(n_seg, seg_first, n_out, c_feat, seed, pos):
    """Weights whose segmentation rows pos and pos + 1 are IDENTICAL (the two logits then see the same arithmetic and
    differ by the difference of their biases to within one rounding) and lie well above every other class."""
    x, W, b = operands(c_feat, n_out, 1, seed)
    W[seg_first:seg_first + n_seg] *= F32(0.05)
    b[seg_first:seg_first + n_seg] = F32(-1.0)
    W[seg_first + pos + 1] = W[seg_first + pos]
    return W, b


def planted_bias(b, seg_first, pos, gap):
    """Bias of the pair: class pos gets 2, class pos + 1 gets 2 + gap (so the SECOND of the pair leads, unless gap = 0,
    where the first index must win)."""
    b = b.copy()
    b[seg_first + pos] = F32(2.0)
    b[seg_first + pos + 1] = np.nextafter(F32(2.0), F32(3.0)) if gap == "ulp" else F32(2.0 + gap)
    return b


def nonfinite_rows():
    """Five-class logit rows holding NaN and infinities; what torch.softmax / torch.argmax make of them is in the golden
    file (a NaN or +inf member turns the whole row into NaN and argmax then gives 0; -inf is an ordinary zero)."""
    n, i = np.nan, np.inf
    return np.array([[0.5, n, 1.0, 0.0, -1.0], [n, n, n, n, n], [0.5, 1.0, i, 0.0, -1.0], [i, 1.0, i, 0.0, -1.0],
                     [0.5, 1.0, -i, 2.0, -1.0], [-i, -i, 1.0, -i, -i], [-i, 0.25, 0.25, -i, 0.0], [0.5, 1.0, -i, 2.0, n]], F32)


# ------------------------------------------------------------------------------------------------------------ per-voxel
EW_UNARY = ("EXP", "AFFINE", "CLAMP", "CLAMP_MIN", "GAMMA", "SIGMOID", "DIV", "NONZERO", "SUB_DIV", "GE", "NAN_TO_NUM")
EW_BINARY = ("ADD", "MUL", "MUL_EXP", "AXPY_CLAMP0", "AXPY", "DIV2", "ZERO_WHERE_ZERO")
EW_A, EW_B = F32(-0.75), F32(1.5)
EW_SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -0.75, 1.5, np.nextafter(F32(-0.75), F32(-1)),
                       np.nextafter(F32(-0.75), F32(0)), np.nextafter(F32(1.5), F32(2)), 1e-38, -1e-38, 3e38, -3e38, 88.0,
                       -88.0, 20.0, -20.0], F32)


def ew_operand(n, seed):
    rs = np.random.RandomState(seed)
    v = (rs.randn(n) * 2).astype(F32)
    k = min(n, len(EW_SPECIAL))
    v[:k] = EW_SPECIAL[:k]
    if n > 600:
        v[n - k:] = EW_SPECIAL[:k][::-1]              # specials in the float4 body AND in the n & 3 tail
    return v


def ew_unary_ref(op, x, a=EW_A, b=EW_B):
    """('bits', fp32 result) for the ops that are one or two IEEE operations (two roundings: no contraction), ('ulp',
    float64) for the expf ops, ('gamma', float64) for GAMMA."""
    x = np.asarray(x, F32)
    name = EW_UNARY[op]
    big = F32(3.402823466e+38)
    with np.errstate(all="ignore"):
        if name == "EXP":
            return "ulp", np.exp(x.astype(F64))
        if name == "SIGMOID":
            return "ulp", 1.0 / (1.0 + np.exp(-x.astype(F64)))
        if name == "GAMMA":
            return "gamma", F64(a) * np.power(x.astype(F64) / F64(a), F64(b))
        r = {"AFFINE": lambda: x * a + b,
             "CLAMP": lambda: np.where(np.isnan(x), a, np.minimum(np.maximum(x, a), b)),     # fmaxf(NaN, a) = a
             "CLAMP_MIN": lambda: np.where(x < a, a, x),
             "DIV": lambda: x / a,
             "NONZERO": lambda: (x != 0).astype(F32),
             "SUB_DIV": lambda: (x - a) / b,
             "GE": lambda: (x >= a).astype(F32),
             "NAN_TO_NUM": lambda: np.where(np.isnan(x), F32(0), np.where(x == np.inf, big, np.where(x == -np.inf, -big, x)))}[name]()
    return "bits", r.astype(F32)


def ew_binary_ref(op, p, q, a=EW_A):
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    name = EW_BINARY[op]
    with np.errstate(all="ignore"):
        if name == "MUL_EXP":
            return "ulp", p.astype(F64) * np.exp(q.astype(F64))
        t = p + a * q
        r = {"ADD": lambda: p + q, "MUL": lambda: p * q,
             "AXPY_CLAMP0": lambda: np.where(t < 0, F32(0), t), "AXPY": lambda: t,
             "DIV2": lambda: p / q, "ZERO_WHERE_ZERO": lambda: np.where(q == 0, F32(0), p)}[name]()
    return "bits", r.astype(F32)


def argmax_rule(p, lut=None):
    """What bfm_argmax_lut_cl documents: the first maximum; a NaN is never greater, so it wins only from column 0."""
    p = np.asarray(p, F32)
    best = np.zeros(p.shape[0], np.int64)
    bv = p[:, 0].copy()
    for c in range(1, p.shape[1]):
        with np.errstate(invalid="ignore"):
            g = p[:, c] > bv
        best[g], bv[g] = c, p[g, c]
    return best if lut is None else np.asarray(lut)[best].astype(np.int64)


def bias_lrelu_ref(y, bias, slope, mask=None):
    """(result, bound): y + bias (one add), select, multiply by the slope; masked-out voxels keep their bits."""
    y = np.asarray(y, F32)
    v = y + np.asarray(bias, F32)[None]
    r = np.where(v > 0, v, v * F32(slope)).astype(F32)
    if mask is not None:
        r = np.where((np.asarray(mask) != 0)[:, None], r, y)
        live = r[np.asarray(mask) != 0]
    else:
        live = r
    return r, F32(np.abs(live).max(initial=0.0))
