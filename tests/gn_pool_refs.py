"""Float64 / longdouble references, emulations of the arithmetic as coded, derived error bounds and the shared case lists
for the GroupNorm statistics kernels (brainfm_amd/csrc/gn_stats.hip) and the pooling half of csrc/pool_stitch.hip.
numpy / torch-CPU only.  The network's GroupNorm is torch.nn.GroupNorm and its pooling nn.MaxPool3d(2), so torch in float64
is the oracle (tests/test_host_gn_pool_refs.py pins gn_truth and pool_truth to it).

Derivation of the bounds (u32 = 2^-24, u64 = 2^-53; first order, the (1 + SLACK) factor covers the products of errors).
A group has N addends x_i with weights w_i (the replication count of the nearest upsample, an integer; 1 for the skip half),
n = sum w_i = count_per_channel * cpg.

 Tensor pass (gn_partial + gn_finalize).  Every addend is widened to fp64 before anything else; w*x is exact (w < 2^8,
 x has 24 bits) and w*x*x rounds at most once.  S = sum w x and Q = sum w x^2 are sums of N fp64 terms in SOME order
 (threads, LDS rows, blocks, channels, a wave butterfly): for any order |dS| <= (N-1) u64 sum|w x| and
 |dQ| <= (N-1) u64 sum w x^2 [Higham, Accuracy and Stability, eq. 4.4: the factor is the depth of the summation tree, at
 most N-1].  The source weight of the rows form, the division by n, the product mean*mean and the subtraction add four
 roundings of quantities no larger than E[x^2] = Q/n.  Hence
     |dvar|  <= (N + 4) u64 E[x^2]
     |dmean| <=  N u64 E|x|  +  u32 |mean|              (the second term: mean is stored as fp32)
 The term of var that comes through mean^2, 2 |mean| |dS|/n, is of the same order only if the summation tree really had
 depth N; the kernels' longest chain is vox_per_block / rows_in_flight + rows_in_flight + nblocks + 70 << N, so it is
 covered by the slack of the first line at every shape here (the host test measures the float64 one-pass error of numpy's
 own summation against the bound: it stays below 1e-3 of it).
     rstd = fl32(1 / sqrt(var + eps)):  relative error <= u32 + 1/2 |dvar| / (var + eps)    [d(v^-1/2) / v^-1/2 = -dv / 2v]
     scale = fl32(rstd32 * gamma):      |dscale| <= |scale| (rel(rstd) + u32)
     bound[g] = max_c |fmaf(x_c, scale_c, shift_c)| over the channel extremes x_c:
             |dbound| <= max_c (|x_c| |dscale_c| + |dshift_c| + u32 |y_c|)      (max is 1-Lipschitz)
     shift = fl32(fl32(-scale32 * mean32) + beta):
             |dshift| <= |dscale| |mean| + |scale| |dmean| + u32 |scale mean| + u32 |shift|
 (the library is built with -ffp-contract=off: the product and the sum round separately.)

 Statistics from given rows: the addends are the table entries (N = rows * cpg per source, summed over the sources of the
 group), with the table's own sums in the place of x and x^2: E[x^2] := sum w rsq / n, E|x| := sum w |rsum| / n.

 Rows written by the pool (maxpool2_kernel).  A thread visits j = ceil(items / (rows * 256)) items of ONE channel quad in
 its grid-stride loop and keeps fs += m (j - 1 fp32 additions after the exact first one) and fq = fmaf(m, m, fq) (j fused
 operations, each one rounding).  Each rounding is at most u32 times the magnitude of a partial sum, itself at most the
 thread's sum |m| (or sum m^2).  Widening is exact; the block's fold of 256 / (C/4) threads and the later fold of the rows
 are fp64 sums of T = rows * 256 / (C/4) terms.  So for a channel's totals over all rows
     |dS| <= (j - 1) u32 sum|m| + T u64 sum|m|          |dQ| <= j u32 sum m^2 + T u64 sum m^2
 (the u64 terms matter only at j = 1, where the fp32 part of dS vanishes.)  min and max are exact.
 The statistics from such rows then carry dS and dQ on top of the bound for given rows:
     |dvar| <= dQ/n + 2 |mean| dS/n + (N + 4) u64 E[x^2]
 which is about j u32 (mean^2 + var): relative to var it grows with (mean/std)^2 -- the conditioning of the rows route.

bound[g] is checked bit for bit as a function of the kernel's own scale and shift (gn_bound_as_coded), never under a
tolerance; gn_truth's bound is the float64 value it approximates."""
import numpy as np
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 2.0 ** -20
F32, F64, LD = np.float32, np.float64, np.longdouble
EPS = 1e-5
TPB = 256

ROUTE_ROWS_VEC4, ROUTE_ROWS_SCALAR, ROUTE_WIDE_VEC4, ROUTE_WIDE_SCALAR = range(4)
ROWS_DIRECT, ROWS_FOLD, ROWS_ONE_LAUNCH = range(3)
RR_MAX, KS, GN_TICKETS = 128, 16, 16


# ----------------------------------------------------------------------------------------------- the rules of the header
def gn_plan(C, nvox, aligned):
    """bfm_gn_stats_plan as include/brainfm_hip.h words it: (route, nblocks, vox_per_block, rows_in_flight)."""
    vec4 = C % 4 == 0 and bool(aligned)
    cv = C // 4 if vec4 else C
    rp = 0 if cv > TPB else TPB // cv
    route = (ROUTE_WIDE_VEC4 if cv > TPB else ROUTE_ROWS_VEC4) + (0 if vec4 else 1)
    nb = min(max(min(32768 // C, 2048), 8), -(-nvox // 16))
    nb = max(nb, 1)
    vpb = -(-nvox // nb)
    return route, -(-nvox // vpb), vpb, rp


def rows_fold_bytes(nrows, C):
    return 0 if nrows <= RR_MAX else (RR_MAX * C * 24 + 255) & ~255


def rows_route(nA, CA, nB, CB, G, has_ticket):
    """bfm_gn_stats_rows_route as the header words it."""
    need = rows_fold_bytes(nA, CA) + (rows_fold_bytes(nB, CB) if CB > 0 else 0)
    if need == 0:
        return ROWS_DIRECT
    if has_ticket and G <= GN_TICKETS and KS * (CA + CB) * 24 <= need:
        return ROWS_ONE_LAUNCH
    return ROWS_FOLD


def pool_rows(C, D, H, W):
    """bfm_maxpool2_rows as documented: 0 unless C % 4 == 0, C/4 <= 256 and 256 % (C/4) == 0."""
    if C <= 0 or C % 4 or min(D, H, W) < 2:
        return 0
    cv = C // 4
    if cv > 256 or 256 % cv:
        return 0
    return min(max(-(-((D // 2) * (H // 2) * (W // 2) * cv) // 256), 1), 4096)


def nearest_map(n_in, n_out):
    """F.interpolate(mode='nearest'): min(floor(dst * float32(in / out)), in - 1)."""
    s = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * s).astype(np.int64), n_in - 1)


def up_maps(lo, hi):
    return [nearest_map(lo[a], hi[a]) for a in range(3)]


def rep_counts(maps, lo):
    return [np.bincount(m, minlength=n).astype(np.int32) for m, n in zip(maps, lo)]


# ------------------------------------------------------------------------------------------------ exact fp32 operations
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64, the sum is taken with its
    rounding error (TwoSum) and the one double-rounding case -- the float64 sum lands on a float32 midpoint with a
    non-zero error -- is resolved by the sign of that error."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)
        c64 = c.astype(F64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        r = s.astype(F32)
        fin = np.isfinite(s) & np.isfinite(err)
        mid = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
        flag = fin & mid & (err != 0)
        if flag.any():
            lo = np.where(r.astype(F64) > s, np.nextafter(r, F32(-np.inf)), r)
            hi = np.nextafter(lo, F32(np.inf))
            r = np.where(flag, np.where(err > 0, hi, lo), r)
    return r.astype(F32)


def gn_bound_as_coded(scale32, shift32, chan_min, chan_max, G):
    """group_affine's bound, bit for bit, from the kernel's OWN scale and shift and the exact per-channel extremes:
    max(|fmaf(mn, sc, sh)|, |fmaf(mx, sc, sh)|) folded with fmaxf (which drops NaN) from 0."""
    sc, sh = np.asarray(scale32, F32), np.asarray(shift32, F32)
    b0 = np.abs(fma32(chan_min, sc, sh))
    b1 = np.abs(fma32(chan_max, sc, sh))
    b = np.fmax(np.fmax(b0, b1), F32(0)).reshape(G, -1)
    return np.fmax.reduce(b, axis=1).astype(F32)


def affine_as_coded(mean32, rstd32, gamma, beta, G):
    """scale and shift as group_affine forms them from the fp32 mean and rstd (each operation rounds on its own)."""
    g = np.asarray(gamma, F32).reshape(G, -1)
    with np.errstate(all="ignore"):
        sc = (np.asarray(rstd32, F32)[:, None] * g).astype(F32)
        sh = ((-sc) * np.asarray(mean32, F32)[:, None]).astype(F32) + np.asarray(beta, F32).reshape(G, -1)
    return sc.reshape(-1), sh.astype(F32).reshape(-1)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def n_diff(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# --------------------------------------------------------------------------------------------------- GroupNorm truth
def _finish(S, Q, SA, N, n, mn, mx, gamma, beta, G, eps, two_pass_var=None):
    """From per-channel longdouble totals to the statistics and the bounds.  S, Q, SA (sum |.|): [Ctot]; N addends and
    n = count * cpg per group."""
    cpg = len(S) // G
    with np.errstate(all="ignore"):
        Sg, Qg, SAg = (v.reshape(G, cpg).sum(1) for v in (S, Q, SA))
        mean = Sg / n
        ex2, eabs = Qg / n, SAg / n
        var = two_pass_var if two_pass_var is not None else np.maximum(ex2 - mean * mean, 0)
        rstd = 1 / np.sqrt(var + LD(F32(eps)))
        gam, bet = np.asarray(gamma, F32).astype(LD).reshape(G, cpg), np.asarray(beta, F32).astype(LD).reshape(G, cpg)
        scale = rstd[:, None] * gam
        shift = bet - mean[:, None] * scale
        mnl, mxl = np.asarray(mn, F32).astype(LD).reshape(G, cpg), np.asarray(mx, F32).astype(LD).reshape(G, cpg)
        y = np.maximum(np.abs(mnl * scale + shift), np.abs(mxl * scale + shift))
        bound = y.max(1)
        dvar = (N + 4) * U64 * ex2
        dmean = N * U64 * eabs + U32 * np.abs(mean)
        rel_rstd = U32 + 0.5 * dvar / (var + LD(F32(eps)))
        dscale = np.abs(scale) * (rel_rstd[:, None] + U32) * (1 + SLACK)
        dshift = (dscale * np.abs(mean)[:, None] + np.abs(scale) * dmean[:, None] + U32 * np.abs(scale * mean[:, None]) +
                  U32 * (np.abs(shift) + dscale * np.abs(mean)[:, None])) * (1 + SLACK)
        # max over channels is 1-Lipschitz: the group's bound moves by at most the largest move of a channel's |y|,
        # |x| dscale + dshift, plus the rounding of the fmaf
        dbound = ((np.maximum(np.abs(mnl), np.abs(mxl)) * dscale + dshift + U32 * y) * (1 + SLACK)).max(1)
    f = lambda v: np.asarray(v, F64)
    return dict(dbound=f(dbound), mean=f(mean), var=f(var), rstd=f(rstd), scale=f(scale).reshape(-1), shift=f(shift).reshape(-1),
                bound=f(bound), ex2=f(ex2), eabs=f(eabs), N=N, n=n, G=G, chan_min=np.asarray(mn, F32),
                chan_max=np.asarray(mx, F32), dvar=f(dvar), dmean=f(dmean) * (1 + SLACK),
                drstd=f(rel_rstd * rstd) * (1 + SLACK), dscale=f(dscale).reshape(-1), dshift=f(dshift).reshape(-1))


def materialise(A, B=None, maps=None):
    """cat((A, nearest_up(B)), -1): A (D, H, W, CA), B (d, h, w, CB), maps = the three index maps."""
    if B is None:
        return np.asarray(A)
    up = np.asarray(B)[maps[0]][:, maps[1]][:, :, maps[2]]
    return np.concatenate([np.asarray(A), up], axis=-1)


def gn_truth(A, B, maps, gamma, beta, G, eps=EPS):
    """Two-pass (centred) longdouble statistics of the materialised cat((A, nearest_up(B)), -1).  Returns a dict: mean,
    var, rstd [G]; scale, shift [C]; bound [G] = max over the group of |x * scale + shift|; the exact per-channel
    extremes; N (addends per group: the values the kernel reads, not the replicated count) and the derived absolute
    bounds dmean, drstd [G], dscale, dshift [C] of the module docstring."""
    x = materialise(A, B, maps).astype(LD)
    D, H, W, C = x.shape
    cpg = C // G
    nvox = D * H * W
    with np.errstate(all="ignore"):
        xg = x.reshape(nvox, G, cpg)
        mean = xg.sum((0, 2)) / (nvox * cpg)
        var = ((xg - mean[None, :, None]) ** 2).sum((0, 2)) / (nvox * cpg)
        flat = x.reshape(nvox, C)
        S, Q, SA = flat.sum(0), (flat * flat).sum(0), np.abs(flat).sum(0)
    CA = np.asarray(A).shape[-1]
    per_src = np.full(C, nvox)
    if B is not None:
        per_src[CA:] = int(np.prod(np.asarray(B).shape[:3]))
    N = per_src.reshape(G, cpg).sum(1).astype(F64)
    f32 = materialise(A, B, maps).reshape(nvox, C)
    mn, mx = f32.min(0), f32.max(0)                      # numpy's min / max keep a NaN
    return _finish(S, Q, SA, N, float(nvox * cpg), mn, mx, gamma, beta, G, eps, two_pass_var=var)


def extremes_as_coded(A, B=None):
    """The per-channel min / max the kernel folds with fminf / fmaxf (NaN dropped) from +-inf: of the sources."""
    parts = [np.asarray(A, F32)] + ([np.asarray(B, F32)] if B is not None else [])
    mn = np.concatenate([np.fmin.reduce(p.reshape(-1, p.shape[-1]), axis=0, initial=F32(np.inf)) for p in parts])
    mx = np.concatenate([np.fmax.reduce(p.reshape(-1, p.shape[-1]), axis=0, initial=F32(-np.inf)) for p in parts])
    return mn.astype(F32), mx.astype(F32)


def rows_truth(tabA, tabB, weightB, nvox, gamma, beta, G, eps=EPS):
    """Statistics from given rows in longdouble: tab = dict(sum, sq [nrows][C] float64; mn, mx float32) or None."""
    S, Q, SA, mn, mx, N = [], [], [], [], [], []
    for tab, w in ((tabA, 1.0), (tabB, weightB)):
        if tab is None:
            continue
        w = LD(w)
        S.append(tab["sum"].astype(LD).sum(0) * w)
        Q.append(tab["sq"].astype(LD).sum(0) * w)
        SA.append(np.abs(tab["sum"]).astype(LD).sum(0) * w)
        mn.append(np.fmin.reduce(tab["mn"], axis=0))
        mx.append(np.fmax.reduce(tab["mx"], axis=0))
        N.append(np.full(tab["sum"].shape[1], tab["sum"].shape[0]))
    S, Q, SA, mn, mx, N = (np.concatenate(v) for v in (S, Q, SA, mn, mx, N))
    cpg = len(S) // G
    return _finish(S, Q, SA, N.reshape(G, cpg).sum(1).astype(F64), float(nvox) * cpg, mn, mx, gamma, beta, G, eps)


def gn_ratios(truth, scale=None, shift=None, mean=None, rstd=None, extra=None, bound=None):
    """Worst |got - truth| / bound per quantity (0 where both vanish).  extra: dict of absolute additions to the bounds
    (the producer's share for rows written by the pool)."""
    out = {}
    for name, got in (("scale", scale), ("shift", shift), ("mean", mean), ("rstd", rstd), ("bound", bound)):
        if got is None:
            continue
        bnd = truth["d" + name] + (extra["d" + name] if extra and name != "bound" else 0.0)
        ok = np.isfinite(truth[name])
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got, F64) - truth[name])
        if name != "bound":                          # the bound of a non-finite group is 0 (fmaxf drops the NaN), pinned apart
            assert (np.isfinite(np.asarray(got, F64)) == ok).all(), name + ": finite pattern differs from the reference"
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / bnd)
        out[name] = float(np.max(np.where(ok, r, 0.0), initial=0.0))
    return out


def make_table(vals):
    """Moment rows of a value tensor [nrows][C][k] (float32): the table a producer would write, sums in float64."""
    v = np.asarray(vals, F32)
    v64 = v.astype(F64)
    return dict(sum=v64.sum(2), sq=(v64 * v64).sum(2), mn=v.min(2), mx=v.max(2))


def table_bytes(tab):
    return b"".join(np.ascontiguousarray(tab[k]).tobytes() for k in ("sum", "sq", "mn", "mx"))


def table_from_bytes(raw, nrows, C):
    k = nrows * C
    raw = np.frombuffer(raw, np.uint8)
    return dict(sum=raw[:k * 8].view(F64).reshape(nrows, C), sq=raw[k * 8:k * 16].view(F64).reshape(nrows, C),
                mn=raw[k * 16:k * 20].view(F32).reshape(nrows, C), mx=raw[k * 20:k * 24].view(F32).reshape(nrows, C))


# ------------------------------------------------------------------------------------------------------------ pooling
def pool_truth(x):
    """nn.MaxPool3d(2) of a channels-last (D, H, W, C) float32 array, by torch in float64 (max selects: exact)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).double().permute(3, 0, 1, 2)[None]
    y = torch.nn.functional.max_pool3d(t, 2)[0].permute(1, 2, 3, 0).contiguous().numpy()
    return y.astype(F32)


def pool_rows_as_coded(pooled, C, nblocks):
    """maxpool2_kernel's row arithmetic on the pooled values (d, h, w, C): per global thread fp32 sequential sums over
    its grid-stride laps (fs += m; fq = fmaf(m, m, fq); fminf / fmaxf), per block the fp64 fold of the 256 / (C/4)
    threads of a channel quad in the order j = 0 .. per-1.  Returns dict(sum, sq, mn, mx) of [nblocks][C]."""
    cv = C // 4
    m = np.ascontiguousarray(pooled, F32).reshape(-1, 4)            # item i = voxel * cv + quad
    n, T = m.shape[0], nblocks * TPB
    fs, fq = np.zeros((T, 4), F32), np.zeros((T, 4), F32)
    fmn, fmx = np.full((T, 4), np.inf, F32), np.full((T, 4), -np.inf, F32)
    for lap in range(-(-n // T)):
        k = min(T, n - lap * T)
        v = m[lap * T:lap * T + k]
        fs[:k] = fs[:k] + v
        fq[:k] = fma32(v, v, fq[:k])
        fmn[:k], fmx[:k] = np.fmin(fmn[:k], v), np.fmax(fmx[:k], v)
    per = TPB // cv
    shp = (nblocks, per, cv, 4)                                      # thread cv0 + j * cv of a block holds quad cv0
    fs, fq, fmn, fmx = (a.reshape(shp) for a in (fs, fq, fmn, fmx))
    S, Q = np.zeros((nblocks, cv, 4), F64), np.zeros((nblocks, cv, 4), F64)
    for j in range(per):
        S = S + fs[:, j].astype(F64)
        Q = Q + fq[:, j].astype(F64)
    return dict(sum=S.reshape(nblocks, C), sq=Q.reshape(nblocks, C), mn=np.fmin.reduce(fmn, axis=1).reshape(nblocks, C),
                mx=np.fmax.reduce(fmx, axis=1).reshape(nblocks, C))


def pool_row_bounds(pooled, C, nblocks):
    """(S, dS, Q, dQ, j) per channel over all rows: the longdouble totals and the derived bounds of the docstring."""
    p = np.asarray(pooled, F32).reshape(-1, C).astype(LD)
    items = p.shape[0] * (C // 4)
    j = -(-items // (nblocks * TPB))
    T = nblocks * TPB // (C // 4)
    S, SA, Q = p.sum(0), np.abs(p).sum(0), (p * p).sum(0)
    dS = ((j - 1) * U32 + T * U64) * SA * (1 + SLACK)
    dQ = (j * U32 + T * U64) * Q * (1 + SLACK)
    return S, np.asarray(dS, F64), Q, np.asarray(dQ, F64), j


def pool_rows_extra(truth, dS, dQ, G):
    """What a producer's dS, dQ [C] add to the bounds of statistics taken from its rows (module docstring)."""
    n = truth["n"]
    cpg = len(dS) // G
    dSg, dQg = dS.reshape(G, cpg).sum(1), dQ.reshape(G, cpg).sum(1)
    mean, var, rstd = truth["mean"], truth["var"], truth["rstd"]
    eps = F64(F32(EPS))
    dmean = dSg / n
    dvar = dQg / n + 2 * np.abs(mean) * dmean
    drstd = rstd * 0.5 * dvar / (var + eps)
    sc = np.abs(truth["scale"]).reshape(G, cpg)
    dscale = sc * (drstd / rstd)[:, None]
    dshift = dscale * np.abs(mean)[:, None] + sc * dmean[:, None]
    k = 1 + SLACK
    return dict(dmean=dmean * k, drstd=drstd * k, dscale=dscale.reshape(-1) * k, dshift=dshift.reshape(-1) * k)


# --------------------------------------------------------------------------------------------------------- case data
def _seed(*key):
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def field(kind, shape, *key):
    """The value kinds of the case lists, float32 (deterministic in `key`)."""
    g = np.random.default_rng(_seed(kind, shape, *key))
    x = (g.standard_normal(shape) * 1.5 + 0.3).astype(F32)
    C = shape[-1]
    if kind == "randn":
        pass
    elif kind == "const":
        x[...] = F32(0.75)                              # every sum exact in fp64: var is exactly 0
    elif kind == "zero_channel":
        x[..., C // 2] = 0
    elif kind == "offset1e3":
        x = (g.standard_normal(shape) + 1000.0).astype(F32)           # mean / std = 10^3
    elif kind == "offset30":
        x = (g.standard_normal(shape) + 30.0).astype(F32)
    elif kind == "neg_heavy":
        x[..., 0] = -np.abs(x[..., 0]) * 3 - 1                       # |min| > |max|
    elif kind in ("pinf", "ninf", "nan"):
        v = {"pinf": np.inf, "ninf": -np.inf, "nan": np.nan}[kind]
        x.reshape(-1, C)[x.reshape(-1, C).shape[0] // 2, C // 2] = v   # one element, in the group of channel C // 2
    else:
        raise ValueError(kind)
    return x


def affine(C, *key):
    """gamma with negative entries and (C >= 3) a zero; beta."""
    g = np.random.default_rng(_seed("affine", C, *key))
    gamma = (g.random(C) + 0.5).astype(F32)
    gamma[::2] *= -1
    if C >= 3:
        gamma[C - 1] = 0
    return gamma, g.standard_normal(C).astype(F32)


SHORT = (5, 7, 7)        # 245 voxels: 16 blocks of 16, the last one of 5 (5x6x7 = 210 splits into 14 x 15 evenly)
# (C, dims, G, misaligned, kind, route)
GN_TENSOR_CASES = (
    [(c, SHORT, g, 0, "randn", ROUTE_ROWS_VEC4) for c, g in ((4, 4), (8, 2), (12, 3), (32, 8), (64, 1), (192, 8),
                                                             (1024, 8))] +
    [(c, SHORT, g, 0, "randn", ROUTE_ROWS_SCALAR) for c, g in ((1, 1), (2, 2), (3, 1), (6, 2))] +
    [(8, SHORT, 2, 1, "randn", ROUTE_ROWS_SCALAR), (256, SHORT, 8, 1, "randn", ROUTE_ROWS_SCALAR),
     (1028, SHORT, 4, 0, "randn", ROUTE_WIDE_VEC4), (2048, SHORT, 8, 0, "randn", ROUTE_WIDE_VEC4),
     (258, SHORT, 2, 0, "randn", ROUTE_WIDE_SCALAR), (1024, SHORT, 8, 1, "randn", ROUTE_WIDE_SCALAR)] +
    [(c, d, g, 0, "randn", r) for c, g, r in ((8, 2, ROUTE_ROWS_VEC4), (3, 3, ROUTE_ROWS_SCALAR))
     for d in ((1, 1, 1), (1, 3, 5), (2, 2, 4), (1, 1, 17), (5, 6, 7))] +
    [(192, (16, 16, 16), 8, 0, "randn", ROUTE_ROWS_VEC4), (64, (30, 30, 30), 8, 0, "randn", ROUTE_ROWS_VEC4),
     (1024, SHORT, 2, 0, "randn", ROUTE_ROWS_VEC4), (514, SHORT, 2, 0, "randn", ROUTE_WIDE_SCALAR),
     (64, SHORT, 64, 0, "randn", ROUTE_ROWS_VEC4)] +
    [(8, SHORT, 2, 0, k, ROUTE_ROWS_VEC4) for k in ("const", "zero_channel", "neg_heavy")] +
    [(6, SHORT, 3, 0, "const", ROUTE_ROWS_SCALAR), (8, (16, 16, 16), 1, 0, "offset1e3", ROUTE_ROWS_VEC4),
     (8, (16, 16, 16), 4, 0, "offset1e3", ROUTE_ROWS_VEC4)])
GN_UNROLLED = {(192, (16, 16, 16)), (64, (30, 30, 30))}              # vox_per_block > 3 * rows_in_flight: loop and tail
GN_NONFINITE_CASES = [(8, SHORT, 4, k) for k in ("pinf", "ninf", "nan")] + [(6, SHORT, 3, "nan")]

# (lo, hi): exact 2x; non-uniform and non-cubic (d*h*w*8 = 96 != 140 = D*H*W); a low-res axis of length 1
UPSAMPLES = [((2, 3, 2), (4, 6, 4)), ((2, 3, 2), (5, 7, 4)), ((1, 3, 2), (2, 6, 4))]
GN_CAT_CHANNELS = [(4, 4, 1), (8, 24, 4), (64, 128, 8), (20, 12, 4), (3, 5, 8), (4, 2052, 8)]
# B on the narrow float4 route with vox_per_block > 3 * rows_in_flight: the unrolled loop takes four replication weights
GN_CAT_UNROLLED = ((6, 5, 7), (13, 11, 15), 8, 256, 8)
GN_BATCH_CASES = [(3, 8, 24, 4), (3, 3, 5, 8), (3, 64, 0, 8), (1, 8, 24, 4)]          # (S, CA, CB, G)

# (nrowsA, CA, nrowsB, CB, G, weightB, route without tickets, route with tickets)
_D, _F, _O = ROWS_DIRECT, ROWS_FOLD, ROWS_ONE_LAUNCH
GN_ROWS_CASES = (
    [(n, 64, 0, 0, 8, 1.0, _D, _D) for n in (1, 127, 128)] +
    [(n, 64, 0, 0, 8, 1.0, _F, _O) for n in (129, 130, 257, 1000)] +
    [(300, 64, 1, 128, 8, 8.0, _F, _O), (300, 64, 5, 128, 8, 3.7, _F, _O), (40, 64, 4000, 128, 8, 8.0, _F, _O),
     (1000, 8, 40, 64, 8, 8.0, _F, _F),                 # 16 * 72 * 24 > 128 * 8 * 24: tickets given, two launches
     (300, 64, 0, 0, 32, 1.0, _F, _F),                  # G = 32 > BFM_GN_TICKETS
     (200, 16, 0, 0, 16, 1.0, _F, _O),                  # cpg = 1
     (40, 64, 200, 128, 8, 8.0, _F, _O),                # cpg = 24: group 2 straddles the seam
     (129, 1024, 0, 0, 2, 1.0, _F, _O)])                # cpg = 512
ROWS_K = 12                                                # values behind a table entry

# (C, dims): channels, extents; the scalar route C in {1, 3, 6}; NaN planes on the odd extents
POOL_EXTENTS = [(2, 2, 2), (3, 3, 3), (5, 7, 9), (4, 6, 2)]
POOL_CHANNELS = [1, 3, 6, 4, 16, 64, 1024]
POOL_ROWS_CHANNELS = [4, 16, 64, 1024]
POOL_ROWS_EXTENTS = [(5, 7, 9), (4, 6, 2), (12, 10, 14)]
POOL_NO_ROWS = [12, 192, 2048, 6]


def tensor_inputs(case):
    """A (dims + (C,)), gamma, beta of a GN_TENSOR_CASES / GN_NONFINITE_CASES entry."""
    C, dims, G, kind = case[0], case[1], case[2], case[4] if len(case) > 4 else case[3]
    gamma, beta = affine(C, G, kind)
    return field(kind, tuple(dims) + (C,), "A", G), gamma, beta


def cat_inputs(lo, hi, CA, CB, G):
    """A on the high-res grid, B on the low-res grid (another distribution, so that its weight shows), gamma, beta."""
    A = field("randn", tuple(hi) + (CA,), "catA", lo, CB)
    B = (field("randn", tuple(lo) + (CB,), "catB", hi, CA) * F32(1.3) - F32(0.5)).astype(F32)
    gamma, beta = affine(CA + CB, "cat", G)
    return A, B, gamma, beta


def rows_inputs(case):
    """tabA, tabB (or None), gamma, beta, nvox of a GN_ROWS_CASES entry: tables of known value tensors."""
    nA, CA, nB, CB, G = case[:5]
    g = np.random.default_rng(_seed("rows", *case[:6]))
    tA = make_table((g.standard_normal((nA, CA, ROWS_K)) * 2.0 + 0.3).astype(F32))
    tB = make_table((g.standard_normal((nB, CB, ROWS_K)) * 1.3 - 0.5).astype(F32)) if CB else None
    gamma, beta = affine(CA + CB, "rows", G)
    return tA, tB, gamma, beta, ROWS_K * nA
