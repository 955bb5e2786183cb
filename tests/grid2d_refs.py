"""Float64 numpy restatement of interpol's grid_pull / grid_push / grid_grad on 2-D grids for spline orders 0 to 3 and
the seven boundary conditions, from the per-axis pieces of tests/spline_grid_refs.py (nodes, weights, signs): image
(Bi, C, X, Y), grid (Bg, *out, 2).  The reference computes this in iso0.py (all-nearest), iso1.py (all-linear) and nd.py
(every other combination); the one place where they differ in more than rounding is the gradient of an all-linear call,
which takes iso1's slope (-1 at the lower node, +1 at the upper) where a linear axis of a mixed-order call takes the
generic path's sign(x), the opposite.  tests/test_host_grid2d.py holds it against the reference's own results
(tests/golden/interpol_grid2d*.npz) and against spline_grid_refs on the embedded 3-D problem.

Bounds: 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft.  extrapolate: 0 no, 1 yes, 2 hist."""
import itertools

import numpy as np

import spline_grid_refs as SR


def _two(v):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * 2)[:2]


def _mask(g, shape, ext):
    if ext not in (0, 2):
        return np.ones(g.shape[:-1])
    thr = 0.55 if ext == 2 else 0.05
    m = np.ones(g.shape[:-1], bool)
    for a in range(2):
        m &= (g[..., a] > -thr) & (g[..., a] < shape[a] - 1 + thr)
    return m.astype(np.float64)


def _setup(grid, shape, orders, bounds, ext):
    orders, bounds = _two(orders), _two(bounds)
    g = np.asarray(grid, np.float64).reshape(grid.shape[0], -1, 2)
    ax = [[SR._nodes(g[b, :, a], orders[a], shape[a], bounds[a]) for a in range(2)] for b in range(g.shape[0])]
    return orders, g, ax, _mask(g, shape, ext)


def pull(inp, grid, orders, bounds, ext):
    """inp (Bi, C, X, Y), grid (Bg, *out, 2) -> (max(Bi, Bg), C, *out), float64"""
    inp = np.asarray(inp, np.float64)
    shape, oshape = inp.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], g.shape[1]))
    for b in range(B):
        (ix, wx, _), (iy, wy, _) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]]
        for a, c in itertools.product(range(orders[0] + 1), range(orders[1] + 1)):
            out[b] += src[:, ix[a] * shape[1] + iy[c]] * (wx[a] * wy[c])
        out[b] *= mask[b % g.shape[0]]
    return out.reshape((B, inp.shape[1]) + tuple(oshape))


def grad(inp, grid, orders, bounds, ext):
    """-> (B, C, *out, 2), float64; orders {1, 1}: iso1's slope, the opposite sign of the generic path's derivative"""
    inp = np.asarray(inp, np.float64)
    shape, oshape = inp.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    flip = -1.0 if orders == [1, 1] else 1.0
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], g.shape[1], 2))
    for b in range(B):
        (ix, wx, dx), (iy, wy, dy) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]]
        for a, c in itertools.product(range(orders[0] + 1), range(orders[1] + 1)):
            val = src[:, ix[a] * shape[1] + iy[c]]
            out[b, :, :, 0] += val * (flip * dx[a] * wy[c])
            out[b, :, :, 1] += val * (wx[a] * flip * dy[c])
        out[b] *= mask[b % g.shape[0]][None, :, None]
    return out.reshape((B, inp.shape[1]) + tuple(oshape) + (2,))


def push(inp, grid, shape, orders, bounds, ext):
    """inp (Bi, C, *in), grid (Bg, *in, 2) -> (B, C, *shape), float64: the adjoint of pull"""
    inp = np.asarray(inp, np.float64)
    shape = tuple(shape)
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], int(np.prod(shape))))
    for b in range(B):
        (ix, wx, _), (iy, wy, _) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]] * mask[b % g.shape[0]]
        for a, c in itertools.product(range(orders[0] + 1), range(orders[1] + 1)):
            lin = ix[a] * shape[1] + iy[c]
            val = src * (wx[a] * wy[c])
            for ch in range(inp.shape[1]):
                np.add.at(out[b, ch], lin, val[ch])
    return out.reshape((B, inp.shape[1]) + shape)


def count(grid, shape, orders, bounds, ext):
    """push of an image of ones: (Bg, 1, *shape)"""
    return push(np.ones((grid.shape[0], 1) + tuple(grid.shape[1:-1])), grid, shape, orders, bounds, ext)


def embed(inp, grid, orders, bounds):
    """The 3-D problem that holds the 2-D one: image (..., X, Y, 1), a third coordinate 0, orders (ox, oy, 0) and the
    bound of the second axis on the third."""
    orders, bounds = _two(orders), _two(bounds)
    g3 = np.concatenate([np.asarray(grid), np.zeros(grid.shape[:-1] + (1,), grid.dtype)], -1)[..., None, :]
    return np.asarray(inp)[..., None], g3, orders + [0], bounds + [bounds[1]]


def redraw_near_jumps(grid, shape, rng, margin=1e-3):
    """spline_grid_refs.redraw_near_jumps over two axes: grid (..., 2) fp32, changed in place"""
    for _ in range(100):
        bad = near_jumps(grid, shape, margin)
        if not bad.any():
            return grid
        for a in range(2):
            k = bad[..., a]
            grid[..., a][k] = (rng.random(int(k.sum())) * (shape[a] + 5.0) - 2.5).astype(np.float32)
    raise RuntimeError("could not clear the jumps")


def near_jumps(grid, shape, margin=1e-3):
    g = np.asarray(grid, np.float64)
    bad = np.abs(g * 2 - np.round(g * 2)) < 2 * margin
    for a in range(2):
        for t in (-0.05, shape[a] - 1 + 0.05, -0.55, shape[a] - 1 + 0.55):
            bad[..., a] |= np.abs(g[..., a] - t) < margin
    return bad
