"""Float64 numpy restatement of interpol's grid_hess and grid_pushgrad for spline orders 0 to 3 and the seven boundary
conditions (what utils/interpol/nd.py:291-464, iso1.py:390-675 and iso0.py:326-368 of the reference compute, and what
pushpull.py:303-325 makes of them), written from their definitions on the nodes of tests/spline_grid_refs.py:

  hess[.., d, d]   takes the second derivative of the weight on axis d and the plain weights on the other two axes,
  hess[.., d, d2]  takes the first derivative on axes d and d2 and the plain weight on the third, and is symmetric,
  pushgrad         is the adjoint of grad: a source voxel with the 3-vector c adds sign * mask * (c_x dwx wy wz +
                   c_y wx dwy wz + c_z wx wy dwz) to each of its nodes,
  contract         sum over channel c and row i of hess[b, c, v, i, j] * cot[b, c, v, i]: d/dgrid of grid_grad.

The first derivative on an order-1 axis is sign(x) in the generic path -- the opposite of the true slope, a quirk of the
reference that is kept (spline_grid_refs.py) -- and the true slope (-1 at the lower node, +1 at the upper one) when all
three orders are 1, where the reference runs iso1.py.  `grad` here follows the same rule, so it is what grid_grad
returns for every order.  The inbounds mask multiplies hess for every batch and channel count: the reference's nd.hess
raises or returns a wrongly shaped result there unless B = C = 1, where it gives exactly this product."""
import itertools

import numpy as np

import spline_grid_refs as SR


def d2weight(order, x):
    a = np.abs(x)
    if order in (0, 1):
        return np.zeros_like(a)
    if order == 2:
        return np.where(a < 0.5, -2.0, 1.0)
    if order == 3:
        return np.where(a < 1, 3 * a - 2, 2 - a)
    raise ValueError(order)


def _nodes(g, order, n, b, iso1):
    """g: (N,) coordinates along one axis -> index (order+1, N), weight * sign, first and second derivative * sign"""
    g0 = np.floor(g - (order - 1) / 2)
    d0 = g - g0
    g0 = g0.astype(np.int64)
    idx, w, dw, hw = [], [], [], []
    for k in range(order + 1):
        s = SR.bound_sign(g0 + k, n, b)
        idx.append(SR.bound_index(g0 + k, n, b))
        w.append(SR.weight(order, d0 - k) * s)
        dw.append((np.full_like(d0, 2.0 * k - 1.0) if iso1 else SR.dweight(order, d0 - k)) * s)
        hw.append(d2weight(order, d0 - k) * s)
    return np.stack(idx), np.stack(w), np.stack(dw), np.stack(hw)


def _setup(grid, shape, orders, bounds, ext):
    orders, bounds = SR._three(orders), SR._three(bounds)
    iso1 = orders == [1, 1, 1]
    g = np.asarray(grid, np.float64).reshape(grid.shape[0], -1, 3)
    ax = [[_nodes(g[b, :, a], orders[a], shape[a], bounds[a], iso1) for a in range(3)] for b in range(g.shape[0])]
    return orders, g, ax, SR._mask(g, shape, ext)


def grad(inp, grid, orders, bounds, ext):
    """What grid_grad returns: spline_grid_refs.grad, with the true slope when all three orders are 1 -> (B, C, *out, 3)"""
    out = SR.grad(inp, grid, orders, bounds, ext)
    return -out if SR._three(orders) == [1, 1, 1] else out


def hess(inp, grid, orders, bounds, ext):
    """inp (Bi, C, X, Y, Z), grid (Bg, *out, 3) -> (max(Bi, Bg), C, *out, 3, 3), float64"""
    inp = np.asarray(inp, np.float64)
    shape, oshape = inp.shape[2:], grid.shape[1:-1]
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1)
    out = np.zeros((B, inp.shape[1], g.shape[1], 3, 3))
    for b in range(B):
        (ix, wx, dx, hx), (iy, wy, dy, hy), (iz, wz, dz, hz) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]]
        for a, c, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
            val = src[:, (ix[a] * shape[1] + iy[c]) * shape[2] + iz[d]]
            out[b, :, :, 0, 0] += val * (hx[a] * wy[c] * wz[d])
            out[b, :, :, 1, 1] += val * (wx[a] * hy[c] * wz[d])
            out[b, :, :, 2, 2] += val * (wx[a] * wy[c] * hz[d])
            out[b, :, :, 0, 1] += val * (dx[a] * dy[c] * wz[d])
            out[b, :, :, 0, 2] += val * (dx[a] * wy[c] * dz[d])
            out[b, :, :, 1, 2] += val * (wx[a] * dy[c] * dz[d])
        out[b] *= mask[b % g.shape[0]][None, :, None, None]
    out[..., 1, 0], out[..., 2, 0], out[..., 2, 1] = out[..., 0, 1], out[..., 0, 2], out[..., 1, 2]
    return out.reshape((B, inp.shape[1]) + tuple(oshape) + (3, 3))


def contract(h, cot):
    """h (B, C, *out, 3, 3), cot (B, C, *out, 3) -> (B, *out, 3): sum over the channel and the row of h"""
    return (np.asarray(h, np.float64) * np.asarray(cot, np.float64)[..., None]).sum(axis=(1, -2))


def pushgrad(inp, grid, shape, orders, bounds, ext):
    """inp (Bi, C, *in, 3), grid (Bg, *in, 3) -> (B, C, *shape), float64: the adjoint of grad"""
    inp = np.asarray(inp, np.float64)
    shape = tuple(shape)
    orders, g, ax, mask = _setup(grid, shape, orders, bounds, ext)
    B = max(inp.shape[0], g.shape[0])
    flat = inp.reshape(inp.shape[0], inp.shape[1], -1, 3)
    out = np.zeros((B, inp.shape[1], int(np.prod(shape))))
    for b in range(B):
        (ix, wx, dx, _), (iy, wy, dy, _), (iz, wz, dz, _) = ax[b % g.shape[0]]
        src = flat[b % inp.shape[0]] * mask[b % g.shape[0]][None, :, None]
        for a, c, d in itertools.product(range(orders[0] + 1), range(orders[1] + 1), range(orders[2] + 1)):
            lin = (ix[a] * shape[1] + iy[c]) * shape[2] + iz[d]
            val = (src[..., 0] * (dx[a] * wy[c] * wz[d]) + src[..., 1] * (wx[a] * dy[c] * wz[d]) +
                   src[..., 2] * (wx[a] * wy[c] * dz[d]))
            for ch in range(inp.shape[1]):
                np.add.at(out[b, ch], lin, val[ch])
    return out.reshape((B, inp.shape[1]) + shape)
