"""Numpy restatement of the fixed-point accumulation of interpol's scatter kernels (brainfm_amd/csrc/push_accum.h and
push_fixed.hip), in int64, and of the contributions the kernels hand it.

The format, per (batch, channel) slice of the input:
  m    = max |x| over the slice in fp32 (grid_pushgrad: over the 3 components too)
  e    = the exponent with m < 2^e (frexp)
  bits = ceil(log2(P * T * G)): P grid points per batch item, T = prod(order + 1) over the axes, G = 1 (push) or 3
         (pushgrad) with |contribution| <= G * m; more than 40 bits are refused
  k    = 62 - bits - e
  q    = rint(c * 2^k), nearest even, of every fp32 contribution c the float route would add; the sum of q in int64
  out  = (float)((double)sum * 2^-k)
  m = 0: the slice is +0.  m NaN or Inf (or, with G > 1, m >= 2^126, where G * m need not be finite): the slice is NaN.

`contributions` restates the arithmetic of the kernels in fp32.  It is exact, bit for bit, where every weight is 0 or +-1
(order 0 on any grid, order 1 on integer coordinates): a product with such a weight does not round.  It asserts that, so
it cannot be used by mistake where the kernels' weights round."""
import itertools

import numpy as np

import grid_hess_refs as HR
import spline_grid_refs as SR

MAX_BITS = 40


def bits_for(P, orders, G):
    """ceil(log2(P * T * G)), T = prod(order + 1); ValueError beyond 40 bits"""
    n = int(P) * int(G)
    for o in orders:
        n *= int(o) + 1
    bits = (n - 1).bit_length()
    if bits > MAX_BITS:
        raise ValueError("%d bits" % bits)
    return bits


def slice_k(m, bits, G=1):
    """m: max |x| of the slice (fp32).  -> k, or None for a slice that is all NaN"""
    m = np.float32(m)
    if not np.isfinite(m):
        return None
    if m == 0:
        return 0
    _, e = np.frexp(m)                        # m = f * 2^e, 1/2 <= f < 1
    if G > 1 and e >= 127:
        return None
    return 62 - bits - int(e)


def quantize(c, k):
    """fp32 contributions -> int64: rint(c * 2^k), the product exact in double"""
    c = np.asarray(c, np.float32).astype(np.float64)
    return np.rint(np.ldexp(c, k)).astype(np.int64)


def finalize(acc, k):
    """int64 sums -> fp32: int64 -> double and double -> float round to nearest even, the product is exact"""
    return np.ldexp(np.asarray(acc, np.int64).astype(np.float64), -k).astype(np.float32)


def accumulate(nvox, lin, q):
    acc = np.zeros(nvox, np.int64)
    np.add.at(acc, lin, q)
    return acc


def fixed_sum(nvox, lin, c, m, bits, G=1):
    """One slice: contributions c (fp32) onto the voxels lin of nvox -> fp32 (nvox,)"""
    k = slice_k(m, bits, G)
    if k is None:
        return np.full(nvox, np.nan, np.float32)
    return finalize(accumulate(nvox, lin, quantize(c, k)), k)


def _exact(w):
    w32 = w.astype(np.float32)
    assert np.isin(w32, (-1.0, 0.0, 1.0)).all(), "contributions(): weights other than 0 and +-1 round in the kernels"
    return w32


def _mask(g, shape, ext):
    if ext not in (0, 2):
        return np.ones(g.shape[:-1], bool)
    thr = 0.55 if ext == 2 else 0.05
    m = np.ones(g.shape[:-1], bool)
    for a in range(g.shape[-1]):
        m &= (g[..., a] > -thr) & (g[..., a] < shape[a] - 1 + thr)
    return m


def _list(v, D):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * D)[:D]


def contributions(kind, inp, grid, shape, orders, bounds, ext):
    """kind 'push': inp (Bi, C, *in), 'pushgrad': inp (Bi, C, *in, 3); grid (Bg, *in, D) fp32, D = 2 or 3 ('pushgrad': 3).
    -> {(b, ch): (lin int64, c fp32)} over the slices of the output (B, C, *shape): the contributions the kernels add, a
    masked point and a contribution of exactly 0 left out as there."""
    D = grid.shape[-1]
    shape = tuple(shape)
    orders, bounds = _list(orders, D), _list(bounds, D)
    grad = kind == "pushgrad"
    inp = np.asarray(inp, np.float32)
    g = np.asarray(grid, np.float64).reshape(grid.shape[0], -1, D)
    Bi, C = inp.shape[:2]
    B = max(Bi, g.shape[0])
    flat = inp.reshape(Bi, C, g.shape[1], 3) if grad else inp.reshape(Bi, C, g.shape[1])
    iso1 = orders == [1, 1, 1]
    out = {}
    for b in range(B):
        gb = g[b % g.shape[0]]
        keep = _mask(gb, shape, ext)
        if grad:
            ax = [HR._nodes(gb[:, a], orders[a], shape[a], bounds[a], iso1)[:3] for a in range(D)]
        else:
            ax = [SR._nodes(gb[:, a], orders[a], shape[a], bounds[a]) for a in range(D)]
        idx = [n[0] for n in ax]
        w = [_exact(n[1]) for n in ax]
        dw = [_exact(n[2]) for n in ax] if grad else None
        for ch in range(C):
            src = flat[b % Bi, ch]
            lins, cs = [], []
            for taps in itertools.product(*[range(o + 1) for o in orders]):
                lin = np.zeros(g.shape[1], np.int64)
                for a in range(D):
                    lin = lin * shape[a] + idx[a][taps[a]]
                if grad:                      # grid_hess.hip: fmaf(pw, wz, pd * dz), pw = fmaf(tx, dx wy, ty (wx dy)), pd = tz (wx wy)
                    (a0, a1, a2) = taps
                    pw = src[:, 0] * (dw[0][a0] * w[1][a1]) + src[:, 1] * (w[0][a0] * dw[1][a1])
                    pd = src[:, 2] * (w[0][a0] * w[1][a1])
                    c = pw * w[2][a2] + pd * dw[2][a2]
                else:                         # spline_grid.hip: val * ((w0 * w1) * w2)
                    wt = w[0][taps[0]]
                    for a in range(1, D):
                        wt = wt * w[a][taps[a]]
                    c = src * wt
                assert c.dtype == np.float32
                use = keep & (c != 0)
                lins.append(lin[use])
                cs.append(c[use])
            out[(b, ch)] = (np.concatenate(lins), np.concatenate(cs))
    return out


def fixed(kind, inp, grid, shape, orders, bounds, ext):
    """What the fixed route returns where `contributions` is exact: fp32 (B, C, *shape)"""
    D = grid.shape[-1]
    shape = tuple(shape)
    G = 3 if kind == "pushgrad" else 1
    P = int(np.prod(grid.shape[1:-1]))
    bits = bits_for(P, _list(orders, D), G)
    inp = np.asarray(inp, np.float32)
    Bi, C = inp.shape[:2]
    B = max(Bi, grid.shape[0])
    nvox = int(np.prod(shape))
    if kind == "pushgrad" and _list(orders, D) == [0, 0, 0]:
        cons = {(b, ch): (np.zeros(0, np.int64), np.zeros(0, np.float32)) for b in range(B) for ch in range(C)}
    else:
        cons = contributions(kind, inp, grid, shape, orders, bounds, ext)
    out = np.zeros((B, C, nvox), np.float32)
    for (b, ch), (lin, c) in cons.items():
        with np.errstate(invalid="ignore"):
            m = np.abs(inp[b % Bi, ch]).max()
        out[b, ch] = fixed_sum(nvox, lin, c, m, bits, G)
    return out.reshape((B, C) + shape)
