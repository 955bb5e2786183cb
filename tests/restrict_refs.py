"""Float64 numpy restatement of interpol.restrict (what utils/interpol/restrict.py computes through grid_push on a
meshgrid of three coordinate lists) and of the gradient of the separable cubic interpol.resize, written from the
definitions and independent of the device's table code: per axis a dense matrix M[j, i] = sum over the nodes k of
coordinate i that land on node j of weight * sign * mask (spline_grid_refs supplies weights and bounds), then three
einsums and the division by `fullscale`.  The spline prefilter (DCT-II conditions only) is restated as its recursion.

When all three orders are 0 the reference takes iso0.py, whose node is round(g): a tie goes to the even node, where the
generic path (floor(g + 0.5)) takes the upper one.  Integer factors under the 'f' / 'l' anchors put every second
sample on a tie, so the rule matters here and is restated (`matrices`).

Bounds: 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft.  extrapolate: 0 no, 1 yes, 2 hist."""
import numpy as np

import spline_grid_refs as SR


def _three(v):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * 3)[:3]


def geometry(inshape, factor=None, shape=None, anchor="c"):
    """The output shape, the float64 coordinates of the input samples in the output lattice (one array per axis) and
    `fullscale` of restrict.py:66-110, for 3-element (or scalar-padded) factor / shape / anchor."""
    inshape = list(inshape)[-3:]
    anchor = [a[0].lower() for a in _three(anchor)]
    factor = _three(factor) if factor else []
    if shape:
        shape = [int(s) for s in _three(shape)]
    else:
        shape = [int(i / f) for i, f in zip(inshape, factor)]
    if not factor:
        factor = [i / o for o, i in zip(shape, inshape)]
    coords, fullscale = [], 1.0
    for a, f, n_in, n_out in zip(anchor, factor, inshape, shape):
        i = np.arange(n_in, dtype=np.float64)
        if a == "c":
            coords.append(np.linspace(0, n_out - 1, n_in))
            fullscale *= (n_in - 1) / (n_out - 1)
        elif a == "e":
            scale = n_out / n_in
            coords.append(i * scale + 0.5 * (scale - 1))
            fullscale *= scale
        elif a == "f":
            coords.append(i / f)
            fullscale *= 1 / f
        elif a == "l":
            coords.append(i / f + ((n_out - 1) - (n_in - 1) / f))
            fullscale *= 1 / f
        else:
            raise ValueError(a)
    return shape, coords, fullscale


def axis_mask(coord, n, ext):
    g = np.asarray(coord, np.float64)
    if ext not in (0, 2):
        return np.ones(g.shape)
    thr = 0.55 if ext == 2 else 0.05
    return ((g > -thr) & (g < n - 1 + thr)).astype(np.float64)


def axis_matrix(coord, n, order, bound, ext, ties_even=False):
    """(n, m): column i holds the weights coordinate i puts on the n nodes (push: out = M @ in, pull: out = M.T @ in).
    ties_even (order 0 only): the node is round(g) with ties to even (iso0.py:12) instead of floor(g + 0.5)."""
    g = np.asarray(coord, np.float64)
    if ties_even and order == 0:
        g0 = np.rint(g).astype(np.int64)
        idx, w = SR.bound_index(g0, n, bound)[None], SR.bound_sign(g0, n, bound)[None]
    else:
        idx, w, _ = SR._nodes(g, order, n, bound)
    mask = axis_mask(g, n, ext)
    M = np.zeros((n, g.shape[0]))
    cols = np.arange(g.shape[0])
    for k in range(order + 1):
        np.add.at(M, (idx[k], cols), w[k] * mask)
    return M


def matrices(coords, shape, orders, bounds, ext):
    orders, bounds = _three(orders), _three(bounds)
    iso0 = all(o == 0 for o in orders)
    return [axis_matrix(coords[a], shape[a], orders[a], bounds[a], ext, iso0) for a in range(3)]


def push(x, mats):
    """x (..., X, Y, Z) -> (..., nx, ny, nz)"""
    return np.einsum("ax,by,cz,...xyz->...abc", mats[0], mats[1], mats[2], np.asarray(x, np.float64), optimize=True)


def pull(y, mats):
    """the adjoint of push"""
    return np.einsum("ax,by,cz,...abc->...xyz", mats[0], mats[1], mats[2], np.asarray(y, np.float64), optimize=True)


_POLE = {2: 8.0 ** 0.5 - 3.0, 3: 3.0 ** 0.5 - 2.0}


def prefilter_axis_dct2(x, axis, order):
    """coeff.py:254-281 along one axis under the DCT-II conditions ('nearest' / 'dct2'; coeff.py:141-175, 216-224), in
    float64: gain, initial condition, causal recursion, final condition, anticausal recursion.  Not quite the inverse of
    the sampling matrix on a short axis (1e-5 relative at n = 4), so the recursion itself is restated."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0).copy()
    n = x.shape[0]
    if order < 2 or n == 1:
        return np.moveaxis(x, 0, axis)
    z = _POLE[order]
    x *= (1 - z) * (1 - 1 / z)
    polen = z ** n
    pole_last = polen * (1 + 1 / (z + polen * polen))
    w = z ** np.arange(1, n - 1, dtype=np.float64) + z ** np.arange(2 * n - 2, n, -1, dtype=np.float64)
    c0 = np.tensordot(w, x[1:-1], axes=(0, 0)) + (x[0] + pole_last * x[-1])
    x[0] = c0 * (z / (1 - polen * polen)) + x[0]
    for i in range(1, n):
        x[i] += z * x[i - 1]
    x[-1] *= z / (z - 1)
    for i in range(n - 2, -1, -1):
        x[i] = z * (x[i + 1] - x[i])
    return np.moveaxis(x, 0, axis)


def prefilter_dct2(x, orders):
    """the filter over the last three axes; it is symmetric, so it is its own adjoint (autograd.py:276-300)"""
    for a, o in enumerate(_three(orders)):
        x = prefilter_axis_dct2(x, np.ndim(x) - 3 + a, o)
    return x


def restrict(x, coords, shape, fullscale, orders, bounds, ext, reduce_sum=False, prefilter=False):
    out = push(x, matrices(coords, shape, orders, bounds, ext))
    if prefilter:
        assert all(b in (1, 3) for b in _three(bounds))
        out = prefilter_dct2(out, orders)
    return out if reduce_sum else out / fullscale


def restrict_backward(w, coords, shape, fullscale, orders, bounds, ext, reduce_sum=False):
    """d sum(restrict(x) * w) / dx"""
    out = pull(w, matrices(coords, shape, orders, bounds, ext))
    return out if reduce_sum else out / fullscale


def resize_backward(w, coords, inshape, bound, prefilter):
    """d sum(resize(x, interpolation=3, bound, prefilter) * w) / dx with the resize coordinates `coords` (per axis, of
    the output samples in the input lattice): the pull matrices transposed, then the prefilter transposed."""
    g = push(w, matrices(coords, inshape, 3, bound, 1))
    if prefilter:
        assert bound in (1, 3)
        g = prefilter_dct2(g, 3)
    return g


def resize_coords(inshape, shape, anchor):
    """resize.py:88-108 for the 'c' and 'e' anchors, float64"""
    out = []
    for a, n_in, n_out in zip(_three(anchor), inshape, shape):
        if a[0] == "c":
            out.append(np.linspace(0, n_in - 1, n_out))
        else:
            scale = n_in / n_out
            out.append(np.arange(n_out, dtype=np.float64) * scale + 0.5 * (scale - 1))
    return out


def near_jumps(coord, n, order, ext, margin=1e-3, exact=None):
    """Coordinates of one axis closer than `margin` to a half-integer on an axis of order 0 (where the nearest node,
    floor(g + 0.5), jumps; at an integer it does not, and the splines of the other orders are continuous) or, without
    extrapolation, to a threshold of the inbounds mask.  `exact`: a boolean array marking coordinates
    that are representable and computed exactly (i / 2, say): those sit on the same side in every precision."""
    g = np.asarray(coord, np.float64)
    bad = np.zeros(g.shape, bool)
    if order == 0:
        bad |= np.abs(g - np.floor(g) - 0.5) < margin
    if ext in (0, 2):
        for t in (-0.05, n - 1 + 0.05, -0.55, n - 1 + 0.55):
            bad |= np.abs(g - t) < margin
    if exact is not None:
        bad &= ~np.asarray(exact, bool)
    return bad
