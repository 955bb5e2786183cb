"""Float64 numpy restatement of interpol's generic grid_pull / grid_push / grid_grad for spline orders 0 to 3 and the
seven boundary conditions (what utils/interpol/nd.py, splines.py and bounds.py of the reference compute), written from
their definitions: per axis of order o, grid0 = floor(g - (o-1)/2); node k in 0..o is read at index(grid0 + k) with
sign(grid0 + k) and weight B_o(g - grid0 - k); grad replaces the weight of its own axis by the derivative the reference
uses (B_o' for orders 2 and 3, 0 for order 0 and -- a quirk of the reference's generic path that is kept -- sign(x) for
order 1, the opposite of the true derivative).  tests/test_host_spline_grid.py holds it against the reference's own
results (tests/golden/interpol_spline_grid.npz); the GPU tests use it on shapes the fixture does not have.

Bounds: 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft.  extrapolate: 0 no, 1 yes, 2 hist."""
import itertools

import numpy as np


def bound_index(i, n, b):
    i = np.asarray(i, np.int64)
    if b in (0, 1):
        return np.clip(i, 0, n - 1)
    if b in (3, 5):
        n2 = 2 * n
        i = np.where(i < 0, n2 - 1 - np.remainder(-i - 1, n2), np.remainder(i, n2))
        return np.where(i >= n, n2 - 1 - i, i)
    if b == 2:
        if n == 1:
            return np.zeros_like(i)
        n2 = 2 * (n - 1)
        i = np.remainder(np.abs(i), n2)
        return np.where(i >= n, n2 - i, i)
    if b == 4:
        n2 = 2 * (n + 1)
        i = np.where(i < 0, -i - 2, i)
        i = np.remainder(i, n2)
        i = np.where(i > n, n2 - 2 - i, i)
        i = np.where(i == -1, 0, i)
        return np.where(i == n, n - 1, i)
    if b == 6:
        return np.remainder(i, n)
    raise ValueError(b)


def bound_sign(i, n, b):
    i = np.asarray(i, np.int64)
    if b == 0:
        return np.where((i < 0) | (i >= n), 0.0, 1.0)
    if b == 4:
        if n == 1:
            return np.ones(i.shape)
        n2 = 2 * (n + 1)
        i = np.where(i < 0, n - 1 - i, i)
        i = np.remainder(i, n2)
        x = np.where(i == 0, 0.0, 1.0)
        x = np.where(np.remainder(i, n + 1) == n, 0.0, x)
        return np.where((i // (n + 1)) % 2 > 0, -x, x)
    if b == 5:
        i = np.where(i < 0, n - 1 - i, i)
        return np.where((i // n) % 2 > 0, -1.0, 1.0)
    return np.ones(i.shape)


def weight(order, x):
    x = np.abs(x)
    if order == 0:
        return np.ones_like(x)
    if order == 1:
        return 1 - x
    if order == 2:
        return np.where(x < 0.5, 0.75 - x * x, 0.5 * (1.5 - x) ** 2)
    if order == 3:
        return np.where(x < 1, (x * x * (x - 2) * 3 + 4) / 6, (2 - x) ** 3 / 6)
    raise ValueError(order)


def dweight(order, x):
    a = np.abs(x)
    if order == 0:
        return np.zeros_like(x)
    if order == 1:
        g = np.ones_like(x)
    elif order == 2:
        g = np.where(a < 0.5, -2 * a, a - 1.5)
    elif order == 3:
        g = np.where(a < 1, a * (a * 1.5 - 2), -0.5 * (2 - a) ** 2)
    else:
        raise ValueError(order)
    return g * np.sign(x)


def _nodes(g, order, n, b):
    """g: (N,) coordinates along one axis -> index (order+1, N), weight * sign, derivative * sign"""
    g0 = np.floor(g - (order - 1) / 2)
    d0 = g - g0
    g0 = g0.astype(np.int64)
    idx, w, dw = [], [], []
    for k in range(order + 1):
        s = bound_sign(g0 + k, n, b)
        idx.append(bound_index(g0 + k, n, b))
        w.append(weight(order, d0 - k) * s)
        dw.append(dweight(order, d0 - k) * s)
    return np.stack(idx), np.stack(w), np.stack(dw)


def _mask(g, shape, ext):
    if ext not in (0, 2):
        return np.ones(g.shape[:-1])
    thr = 0.55 if ext == 2 else 0.05
    m = np.ones(g.shape[:-1], bool)
    for a in range(3):
        m &= (g[..., a] > -thr) & (g[..., a] < shape[a] - 1 + thr)
    return m.astype(np.float64)


def _three(v):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * 3)[:3]


def _setup(grid, shape, orders, bounds, ext):
    orders, bounds = _three(orders), _three(bounds)
    g = np.asarray(grid, np.float64).reshape(grid.shape[0], -1, 3)
    ax = [[_nodes(g[b, :, a], orders[a], shape[a], bounds[a]) for a in range(3)] for b in range(g.shape[0])]
    return orders, g, ax, _mask(g, shape, ext)


def pull(inp, grid, orders, bounds, ext):
    """inp (Bi, C, X, Y, Z), grid (Bg, *out, 3) -> (max(Bi, Bg), C, *out), float64"""
    inp = np.asarray(inp, np.float64)
    shape, oshape = inp.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], g.shape[1]))
    for b in range(B):
        (ix, wx, _), (iy, wy, _), (iz, wz, _) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]]
        for a, c, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
            lin = (ix[a] * shape[1] + iy[c]) * shape[2] + iz[d]
            out[b] += src[:, lin] * (wx[a] * wy[c] * wz[d])
        out[b] *= mask[b % g.shape[0]]
    return out.reshape((B, inp.shape[1]) + tuple(oshape))


def grad(inp, grid, orders, bounds, ext):
    """-> (B, C, *out, 3), float64"""
    inp = np.asarray(inp, np.float64)
    shape, oshape = inp.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], g.shape[1], 3))
    for b in range(B):
        (ix, wx, dx), (iy, wy, dy), (iz, wz, dz) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]]
        for a, c, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
            val = src[:, (ix[a] * shape[1] + iy[c]) * shape[2] + iz[d]]
            out[b, :, :, 0] += val * (dx[a] * wy[c] * wz[d])
            out[b, :, :, 1] += val * (wx[a] * dy[c] * wz[d])
            out[b, :, :, 2] += val * (wx[a] * wy[c] * dz[d])
        out[b] *= mask[b % g.shape[0]][None, :, None]
    return out.reshape((B, inp.shape[1]) + tuple(oshape) + (3,))


def push(inp, grid, shape, orders, bounds, ext):
    """inp (Bi, C, *in), grid (Bg, *in, 3) -> (B, C, *shape), float64: the adjoint of pull"""
    inp = np.asarray(inp, np.float64)
    shape = tuple(shape)
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], int(np.prod(shape))))
    for b in range(B):
        (ix, wx, _), (iy, wy, _), (iz, wz, _) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]] * mask[b % g.shape[0]]
        for a, c, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
            lin = (ix[a] * shape[1] + iy[c]) * shape[2] + iz[d]
            val = src * (wx[a] * wy[c] * wz[d])
            for ch in range(inp.shape[1]):
                np.add.at(out[b, ch], lin, val[ch])
    return out.reshape((B, inp.shape[1]) + shape)


def redraw_near_jumps(grid, shape, rng, margin=1e-3):
    """Coordinates closer than `margin` to a multiple of 0.5 (where a nearest-neighbour node, or the derivative on a
    linear axis, jumps) or to a threshold of the inbounds mask are drawn again, until none is left.  grid (..., 3) fp32,
    changed in place; `rng` is a numpy Generator."""
    for _ in range(100):
        bad = near_jumps(grid, shape, margin)
        if not bad.any():
            return grid
        for a in range(3):
            k = bad[..., a]
            grid[..., a][k] = (rng.random(int(k.sum())) * (shape[a] + 5.0) - 2.5).astype(np.float32)
    raise RuntimeError("could not clear the jumps")


def near_jumps(grid, shape, margin=1e-3):
    g = np.asarray(grid, np.float64)
    bad = np.abs(g * 2 - np.round(g * 2)) < 2 * margin
    for a in range(3):
        for t in (-0.05, shape[a] - 1 + 0.05, -0.55, shape[a] - 1 + 0.55):
            bad[..., a] |= np.abs(g[..., a] - t) < margin
    return bad
