"""Host-side mirror of ``utils/interpol`` (vendored torch-interpol): ``grid_pull`` / ``grid_push`` / ``grid_count`` /
``grid_grad`` for spline orders 0 to 3, any order per axis, in 3-D (utils/interpol/api.py:137-335, autograd.py:125-245,
pushpull.py:35-282), ``resize`` (resize.py:13-119) and ``restrict`` (restrict.py:9-122; separable axis passes on
restrict.hip, which also give the separable cubic ``resize`` its gradient).  All-linear calls run ``iso1``
(iso1.py:28-387) on the linear kernels of spline_grid.hip; every other combination runs the generic path (nd.py:30-290,
splines.py:30-103, bounds.py:24-89) on the dimension-generic kernels of the same file.  ``prefilter`` goes through
``spline_coeff_nd`` (coeff.py:254-344), which is differentiable (autograd.py:276-300).

``grid_pull`` / ``grid_push`` / ``grid_count`` of a floating-point image, ``spline_coeff_nd`` and ``resize`` also take
2-D grids (..., X, Y, 2) on the 2-D instantiations of spline_grid.hip, differentiable to first order like their 3-D
forms; there every order, the all-linear one included, is an instantiation of one kernel.  Label maps, ``grid_grad`` /
``grid_hess`` / ``grid_pushgrad`` and ``restrict`` are 3-D only, and 1-D grids raise everywhere.

grid_pull / grid_push are differentiable to first order through grid_push / grid_grad, and grid_grad through
``grid_pushgrad`` and ``grid_hess`` (pushpull.py:176-233 and :303-325; nd.py:291-464, iso1.py:390-675, iso0.py:326-368)
on grid_hess.hip, which takes every order 0 to 3 in one export per operation.  Nothing here has a double backward, as in
the reference.

``grid_pull`` of an integer image is the reference's label branch (api.py:182-193) in one pass of label_pull.hip.  The grid
builders ``identity_grid`` / ``add_identity_grid`` / ``add_identity_grid_`` / ``affine_grid`` (api.py:455-560) run on
grid_builders.hip, and ``spline_coeff`` (api.py:335-383) filters one dimension on the prefilter kernels.

The scatter kernels behind ``grid_push`` / ``grid_count`` / ``grid_pushgrad`` and the backward of ``grid_pull`` /
``grid_grad`` / the 2-D ``resize`` add with fp32 atomics by default, so their last bit differs from run to run.
``set_push_mode("fixed")``, ``BFM_PUSH_MODE=fixed`` or ``torch.use_deterministic_algorithms(True)`` send them through
64-bit fixed-point accumulators instead (``push_mode()``): the same bits on every run, whatever the
order of the points.
"""
import ctypes as C
import os

import torch

from . import _lib as L

_BOUND = dict(zero=0, zeros=0, replicate=1, nearest=1, repeat=1, border=1, dct1=2, mirror=2, dct2=3, reflect=3,
              reflection=3, neumann=3, dst1=4, antimirror=4, dst2=5, antireflect=5, dirichlet=5, dft=6, wrap=6,
              circular=6)
_SPLINE_ORDER = {"nearest": 0, "zeroth": 0, "linear": 1, "first": 1, "quadratic": 2, "second": 2, "cubic": 3, "third": 3,
                 "fourth": 4, "fifth": 5, "sixth": 6, "seventh": 7}
_LINEAR = (1, 1, 1)


def _order_list(interpolation, high_names=True):
    """autograd.py:77-122 inter_to_nitorch + jit_utils.pad_list_int: names or integers, one per axis, padded with the
    last entry.  Orders 4 to 7 exist in the reference and are not implemented here.  high_names=False (grid_pull / push /
    count / grad): orders 2 and 3 are taken as integers only -- their names ('quadratic', 'cubic', ...) keep raising
    NotImplementedError there, the behaviour those functions are pinned to; 'nearest' and 'linear' are taken."""
    orders = list(interpolation) if isinstance(interpolation, (list, tuple)) else [interpolation]
    out = []
    for o in orders:
        if isinstance(o, str):
            if o.lower() not in _SPLINE_ORDER:
                raise ValueError("Unknown interpolation order {}".format(o))
            if not high_names and 2 <= _SPLINE_ORDER[o.lower()] <= 3:
                raise NotImplementedError("interpolation order '%s' by name is not implemented for pull / push / count / "
                                          "grad: pass the integer %d" % (o, _SPLINE_ORDER[o.lower()]))
            o = _SPLINE_ORDER[o.lower()]
        o = int(o)
        if not 0 <= o <= 7:
            raise ValueError("Unknown interpolation order {}".format(o))
        if o > 3:
            raise NotImplementedError("interpolation order %d is not implemented (orders 0 to 3 are)" % o)
        out.append(o)
    while len(out) < 3:
        out.append(out[-1])
    return tuple(out[:3])


def _bound_list(bound):
    if isinstance(bound, (str, int)):
        bound = [bound] * 3
    out = []
    for b in bound:
        if isinstance(b, str):
            if b.lower() not in _BOUND:
                raise ValueError("Unknown bound {}".format(b))
            out.append(_BOUND[b.lower()])
        else:
            out.append(int(b))
    while len(out) < 3:
        out.append(out[-1])
    return out[:3]


def _prep(input, grid, dim=3, tail=(), cast=True):
    """api.py:81-118 _preproc: broadcast batch dims, default channel of 1.  Returns (x (B,C,*in,*tail), g (B,*out,dim), info).
    tail: trailing dimensions of `input` behind the spatial ones (grid_pushgrad: (3,)); cast=False keeps the dtype of
    `input` (a label map) where the default computes in float32."""
    grid_spatial = tuple(grid.shape[-dim - 1:-1])
    grid_batch = tuple(grid.shape[:-dim - 1])
    lead = tuple(input.shape[:input.dim() - len(tail)])
    in_spatial = lead[-dim:]
    channel = 0 if len(lead) == dim else lead[-dim - 1]
    in_batch = lead[:-dim - 1] if len(lead) > dim else ()
    batch = torch.broadcast_shapes(grid_batch, in_batch)
    g = grid.to(torch.float32).expand(*batch, *grid_spatial, dim).reshape(-1, *grid_spatial, dim).contiguous()
    x = input.to(torch.float32) if cast else input
    x = x.expand(*batch, channel or 1, *in_spatial, *tail).reshape(-1, channel or 1, *in_spatial, *tail).contiguous()
    return x, g, (batch, channel, in_spatial, grid_spatial)


def _unprep(out, batch, channel, *trailing):
    """(B,C,*trailing) back to the caller's batch dims and channel: no channel dim for a channel-less, unbatched call"""
    out_channel = [channel] if channel else ([1] if batch else [])
    return out.reshape(*batch, *out_channel, *trailing)


def _extrap(extrapolate):
    """False / 'no' -> 0, True / 'yes' -> 1, 'hist' -> 2; an integer as it is"""
    return int({False: 0, True: 1, "no": 0, "yes": 1, "hist": 2}.get(extrapolate, extrapolate))


def _opts(interpolation, bound, extrapolate):
    return (C.c_int * 3)(*_bound_list(bound)), _order_list(interpolation, high_names=False), _extrap(extrapolate)


_LABEL_DTYPE = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3}      # BFM_LABEL_* of include/brainfm_hip.h
LABEL_PULL_AUTO, LABEL_PULL_LDS, LABEL_PULL_REGS, LABEL_PULL_PASSES = 0, 1, 2, 3         # BFM_LABEL_PULL_*


def _export(name, x, g, dims, b, o, ext, extra, out, workspace=None):
    """One call of an export of the grid family, which all take (inp[, label dtype], Bi, C, *in, grid, Bg, *dims, bound[,
    order], extrapolate, *extra, out[, workspace, bytes], stream): x (Bi,C,*in[,3]) and g (Bg,*,D) contiguous, `dims` the
    other spatial shape of the call (the grid's for a pull, the volume's for a push), o None for a _linear export, which
    takes no order.  D = 2: the two extents of each shape; the export reads the first two of the three bounds and orders.
    Returns `out`."""
    dim = g.shape[-1]
    args = [L.ptr(x)] + ([] if x.dtype.is_floating_point else [_LABEL_DTYPE[x.dtype]])
    args += [x.shape[0], x.shape[1], *x.shape[2:2 + dim], L.ptr(g), g.shape[0], *dims[:dim], b]
    args += [] if o is None else [(C.c_int * 3)(*o)]
    ws = [] if workspace is None else [L.ptr(workspace), workspace.numel()]
    L.check(getattr(L.load(), "bfm_" + name)(*args, ext, *extra, L.ptr(out), *ws, L.stream_ptr()), name)
    return out


PUSH_MODES = ("atomic", "fixed")
_push_mode_override = None


def _check_push_mode(mode, what):
    if mode not in PUSH_MODES:
        raise ValueError("%s: %r is not a push mode (%s)" % (what, mode, " / ".join(PUSH_MODES)))
    return mode


def set_push_mode(mode):
    """How grid_push, grid_count, grid_pushgrad and the backward of grid_pull / grid_grad / the 2-D resize accumulate:
    'atomic' (fp32 atomics: the last bit depends on the order of arrival) or 'fixed' (64-bit fixed-point integer atomics:
    the same bits on every run, in every order of the points).  None clears the choice, and
    push_mode() follows the environment and torch again."""
    global _push_mode_override
    _push_mode_override = None if mode is None else _check_push_mode(mode, "set_push_mode")


def push_mode():
    """The accumulation mode of the scatter kernels, resolved at every call: set_push_mode(mode) if one was given, else the
    environment variable BFM_PUSH_MODE, else 'fixed' under torch.use_deterministic_algorithms(True), else 'atomic'."""
    if _push_mode_override is not None:
        return _push_mode_override
    env = os.environ.get("BFM_PUSH_MODE")
    if env:
        return _check_push_mode(env, "BFM_PUSH_MODE")
    return "fixed" if torch.are_deterministic_algorithms_enabled() else "atomic"


def _fixed_export(name, x, g, shape, b, o, ext):
    """The _fixed sibling of a scatter export: the same sums through int64 fixed-point accumulators in a workspace; `out`
    need not be zero, every element is written."""
    out = _out(x, g, *shape)
    nvox = 1
    for n in shape:
        nvox *= n
    nbytes = L.load().bfm_grid_push_fixed_workspace(out.shape[0], out.shape[1], nvox)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    return _export(name + "_fixed", x, g, shape, b, o, ext, (), out, workspace=ws)


def _linear_or_spline(op, o, dim=3):
    """3-D: all-linear calls run iso1 on the linear kernels of spline_grid.hip, every other combination the generic path.
    2-D: every order is an instantiation of the generic kernels."""
    if dim == 2:
        return "grid_%s2d_spline" % op, o
    return ("grid_%s3d_linear" % op, None) if o == _LINEAR else ("grid_%s3d_spline" % op, o)


def _out(x, g, *trailing, fill=torch.empty):
    return fill((max(x.shape[0], g.shape[0]), x.shape[1]) + trailing, dtype=x.dtype, device=x.device)


def _pull_raw(x, g, b, o, ext):
    """x (Bi,C,*in), g (Bg,*out,D), D = 2 or 3 -> (B,C,*out)"""
    gs = tuple(g.shape[1:-1])
    name, o = _linear_or_spline("pull", o, g.shape[-1])
    return _export(name, x, g, gs, b, o, ext, (), _out(x, g, *gs))


def _push_raw(x, g, shape, b, o, ext):
    name, o = _linear_or_spline("push", o, g.shape[-1])
    if push_mode() == "fixed":
        return _fixed_export(name, x, g, shape, b, o, ext)
    return _export(name, x, g, shape, b, o, ext, (), _out(x, g, *shape, fill=torch.zeros))


def _grad_raw(x, g, b, o, ext):
    """-> (B,C,*out,D).  On a 2-D grid this serves the autograd of pull and push only; the public grid_grad is 3-D."""
    gs = tuple(g.shape[1:-1])
    name, o = _linear_or_spline("grad", o, g.shape[-1])
    return _export(name, x, g, gs, b, o, ext, (), _out(x, g, *gs, g.shape[-1]))


def _hess_raw(x, g, b, o, ext, cot=None):
    """cot None: the Hessian (B,C,*out,3,3); cot (B,C,*out,3): its contraction with cot over channel and row, (B,*out,3)"""
    gs = tuple(g.shape[1:4])
    out = _out(x, g, *gs, 3, 3) if cot is None else torch.empty((cot.shape[0],) + gs + (3,), dtype=x.dtype, device=x.device)
    return _export("grid_hess3d", x, g, gs, b, o, ext, (L.ptr(cot),), out)


def _pushgrad_raw(x, g, shape, b, o, ext):
    """x (B,C,*in,3) -> (B,C,*shape)"""
    if push_mode() == "fixed":
        return _fixed_export("grid_pushgrad3d", x, g, shape, b, o, ext)
    return _export("grid_pushgrad3d", x, g, shape, b, o, ext, (), _out(x, g, *shape, fill=torch.zeros))


def _label_pull_raw(x, g, b, o, ext, variant=LABEL_PULL_AUTO):
    """x (Bi,C,*in) uint8 / int16 / int32 / int64, g (Bg,*out,3) fp32, both contiguous -> (B,C,*out) of x's dtype"""
    gs = tuple(g.shape[1:4])
    return _export("label_pull3d", x, g, gs, b, o, ext, (variant,), _out(x, g, *gs))


class _GridGrad(torch.autograd.Function):
    """autograd.py:216-245 + pushpull.py:303-325: d/dinput = pushgrad(grad), d/dgrid = sum over channel and row of
    hess(input) * grad, which grid_hess.hip forms without writing the Hessian.  First order only."""

    @staticmethod
    def forward(ctx, x, g, b, o, ext):
        ctx.opt = (b, o, ext)
        ctx.save_for_backward(x, g)
        return _grad_raw(x, g, b, o, ext)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, g = ctx.saved_tensors
        b, o, ext = ctx.opt
        grad = grad.contiguous().to(torch.float32)
        gi = _pushgrad_raw(grad, g, x.shape[2:], b, o, ext) if ctx.needs_input_grad[0] else None
        gg = _hess_raw(x, g, b, o, ext, cot=grad) if ctx.needs_input_grad[1] else None
        return gi, gg, None, None, None


class _GridPull(torch.autograd.Function):
    """autograd.py:125-152 + pushpull.py:237-258: d/dinput = push(grad), d/dgrid = sum_c grad * grid_grad(input) (zero at
    order 0, where grid_grad is)."""

    @staticmethod
    def forward(ctx, x, g, b, o, ext):
        ctx.opt = (b, o, ext)
        ctx.save_for_backward(x, g)
        return _pull_raw(x, g, b, o, ext)

    @staticmethod
    def backward(ctx, grad):
        x, g = ctx.saved_tensors
        b, o, ext = ctx.opt
        grad = grad.contiguous().to(torch.float32)
        gi = _push_raw(grad, g, x.shape[2:], b, o, ext) if ctx.needs_input_grad[0] else None
        gg = (_grad_raw(x, g, b, o, ext) * grad.unsqueeze(-1)).sum(dim=1) if ctx.needs_input_grad[1] else None
        return gi, gg, None, None, None


class _GridPush(torch.autograd.Function):
    """autograd.py:155-190 + pushpull.py:262-282: d/dinput = pull(grad), d/dgrid = sum_c input * grid_grad(grad)."""

    @staticmethod
    def forward(ctx, x, g, shape, b, o, ext):
        ctx.opt = (b, o, ext)
        ctx.save_for_backward(x, g)
        return _push_raw(x, g, shape, b, o, ext)

    @staticmethod
    def backward(ctx, grad):
        x, g = ctx.saved_tensors
        b, o, ext = ctx.opt
        grad = grad.contiguous().to(torch.float32)
        gi = _pull_raw(grad, g, b, o, ext) if ctx.needs_input_grad[0] else None
        gg = (_grad_raw(grad, g, b, o, ext) * x.unsqueeze(-1)).sum(dim=1) if ctx.needs_input_grad[1] else None
        return gi, gg, None, None, None, None


def _require_cuda(t, what):
    if t.device.type != "cuda":
        raise L.BfmError("%s runs on a HIP device only; there is no CPU fallback in the product path" % what)


def _grid_dim(grid, what):
    """The number of spatial dimensions of a call, from the last dimension of its grid: 2 or 3"""
    dim = grid.shape[-1]
    if dim not in (2, 3) or (dim == 2 and grid.dim() < 3):
        raise NotImplementedError("%s: only 2-D and 3-D grids (..., *spatial, 2 or 3) are implemented" % what)
    return dim


def _needs_prefilter(prefilter, o, b, shape):
    """Orders 0 and 1: the prefilter is the identity.  Raises for an axis it would have to filter under 'dst1' / 'dst2'."""
    if not prefilter or all(k < 2 for k in o):
        return False
    _check_prefilter_bounds(o, b, shape)
    return True


def _check_prefilter_bounds(orders, bounds, shape):
    for o, b, n in zip(orders, bounds, shape):
        if o > 1 and n > 1 and b not in _PREFILTER_FAMILY:
            raise NotImplementedError("spline prefilter: no 'dst1' / 'dst2' boundary conditions (the reference has none)")


def grid_push(input, grid, shape=None, interpolation="linear", bound="zero", extrapolate=False, prefilter=False):
    """api.py:203-250: splat `input` (..., [channel], *spatial) at the coordinates `grid` (..., *spatial, D) into a
    volume of `shape` (default: the input's spatial shape), D = 2 or 3.  Differentiable w.r.t. input and grid.
    `prefilter` filters the result, as the reference does."""
    b, o, ext = _opts(interpolation, bound, extrapolate)
    dim = _grid_dim(grid, "grid_push")
    shape = tuple(int(v) for v in (shape if shape is not None else input.shape[-dim:]))
    prefilter = _needs_prefilter(prefilter, o[:dim], list(b)[:dim], shape)
    _require_cuda(input, "grid_push")
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input, grid, dim)
    if in_spatial != grid_spatial:
        raise ValueError("Input and grid should have the same spatial shape")
    out = _GridPush.apply(x, g, shape, b, o, ext)
    if prefilter:
        out = spline_coeff_nd(out, interpolation=list(o), bound=bound, dim=dim, inplace=True)
    return _unprep(out, batch, channel, *shape)


def grid_count(grid, shape=None, interpolation="linear", bound="zero", extrapolate=False):
    """api.py:253-287: push of an image of ones (the Jacobian-free 'count' image)."""
    _opts(interpolation, bound, extrapolate)
    dim = _grid_dim(grid, "grid_count")
    _require_cuda(grid, "grid_count")
    gs = tuple(grid.shape[-dim - 1:-1])
    ones = torch.ones(tuple(grid.shape[:-dim - 1]) + (1,) + gs, dtype=torch.float32, device=grid.device)
    out = grid_push(ones, grid, shape, interpolation, bound, extrapolate)
    return out


def grid_grad(input, grid, interpolation="linear", bound="zero", extrapolate=False, prefilter=False):
    """api.py:290-332: spatial gradient of the interpolated image at `grid`: (..., [channel], *spatial_out, 3).
    Differentiable to first order w.r.t. input (grid_pushgrad) and grid (grid_hess contracted with the incoming gradient),
    autograd.py:216-245; with `prefilter` the gradient reaches the un-filtered image through spline_coeff_nd.  Zero at
    order 0, and so are both gradients.  A second backward raises."""
    b, o, ext = _opts(interpolation, bound, extrapolate)
    if grid.shape[-1] != 3:
        raise NotImplementedError("grid_grad: only 3-D grids are implemented (1-D and 2-D grids are not)")
    prefilter = _needs_prefilter(prefilter, o, list(b), input.shape[-3:])
    _require_cuda(input, "grid_grad")
    if prefilter:
        input = spline_coeff_nd(input, interpolation=list(o), bound=bound, dim=3)
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input, grid)
    out = _GridGrad.apply(x, g, b, o, ext)
    return _unprep(out, batch, channel, *grid_spatial, 3)


def grid_hess(input, grid, interpolation="linear", bound="zero", extrapolate=False):
    """pushpull.py:207-233: the Hessian of the interpolated image at `grid`, (..., [channel], *spatial_out, 3, 3), symmetric.
    Entry (d, d) takes the second derivative of the spline on axis d, entry (d, d2) the first derivative on both; zero
    at order 0, zero diagonal at order 1.  The inbounds mask of extrapolate 0 / 2 multiplies it for every batch and
    channel count (the reference's nd.hess raises there unless B = C = 1).  Forward only."""
    b, o, ext = _opts(interpolation, bound, extrapolate)
    if grid.shape[-1] != 3:
        raise NotImplementedError("grid_hess: only 3-D grids are implemented (1-D and 2-D grids are not)")
    _require_cuda(input, "grid_hess")
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input.detach(), grid.detach())
    out = _hess_raw(x, g, b, o, ext)
    return _unprep(out, batch, channel, *grid_spatial, 3, 3)


def grid_pushgrad(input, grid, shape=None, interpolation="linear", bound="zero", extrapolate=False):
    """pushpull.py:176-203: the adjoint of grid_grad.  input (..., [channel], *spatial, 3) holds a 3-vector per voxel and
    is splatted at the coordinates `grid` (..., *spatial, 3) into a volume of `shape` (default: the input's spatial
    shape): (..., [channel], *shape).  fp32 atomics, like grid_push, or fixed point under push_mode().  Forward only."""
    b, o, ext = _opts(interpolation, bound, extrapolate)
    if grid.shape[-1] != 3 or input.shape[-1] != 3:
        raise NotImplementedError("grid_pushgrad: only 3-D grids are implemented (1-D and 2-D grids are not)")
    if input.dim() < 4:
        raise ValueError("grid_pushgrad: input must be (..., [channel], X, Y, Z, 3)")
    if tuple(input.shape[-4:-1]) != tuple(grid.shape[-4:-1]):
        raise ValueError("Input and grid should have the same spatial shape")
    shape = tuple(int(v) for v in (shape if shape is not None else input.shape[-4:-1]))
    _require_cuda(input, "grid_pushgrad")
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input.detach(), grid.detach(), tail=(3,))
    out = _pushgrad_raw(x, g, shape, b, o, ext)
    return _unprep(out, batch, channel, *shape)


def _label_pull(input, grid, b, o, ext, prefilter):
    """api.py:182-193: an integer image holds labels, and labels are not interpolated.  The result holds, per output
    voxel, the label whose indicator has the largest interpolated weight at the call's orders, bounds and `extrapolate`
    (the smallest label among equal weights, 0 where no weight is positive), in one pass of label_pull.hip instead of
    one pull per label.  Same dtype as the image, no gradient."""
    if input.dtype == torch.bool:
        raise TypeError("grid_pull: a bool image is neither an image nor a label map; cast it to a float dtype to "
                        "interpolate it or to uint8 to pull it as labels")
    if input.dtype not in _LABEL_DTYPE:
        raise TypeError("grid_pull: label maps are uint8, int16, int32 or int64, not %s" % input.dtype)
    if prefilter:
        raise NotImplementedError("grid_pull: prefilter=True is not implemented for an integer (label) image: the "
                                  "reference overwrites its own input with the first label's coefficients there and has "
                                  "no defined result")
    _require_cuda(input, "grid_pull")
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input, grid.detach(), cast=False)
    out = _label_pull_raw(x, g, b, o, ext)
    return _unprep(out, batch, channel, *grid_spatial)


def grid_pull(input, grid, interpolation="linear", bound="zero", extrapolate=False, prefilter=False):
    """Sample `input` at the voxel coordinates in `grid` (api.py:137-200).

    input: (..., [channel], *spatial) ; grid: (..., *spatial_out, D), D = 2 or 3.  Returns (..., [channel], *spatial_out).
    Computes in fp32 like the reference's custom_fwd(cast_inputs=torch.float32).  `prefilter` turns the image into
    spline coefficients first, so that the result interpolates it.  An integer image (uint8, int16, int32, int64) is a
    label map: the result has its dtype and holds the label with the largest interpolated weight (_label_pull); label
    maps are pulled through 3-D grids only.  On a 2-D grid the first two of the orders and bounds are read."""
    b, o, ext = _opts(interpolation, bound, extrapolate)
    if not input.dtype.is_floating_point:
        if grid.shape[-1] != 3:
            raise NotImplementedError("only 3-D grids are on the hot path")
        return _label_pull(input, grid, b, o, ext, prefilter)
    dim = _grid_dim(grid, "grid_pull")
    prefilter = _needs_prefilter(prefilter, o[:dim], list(b)[:dim], input.shape[-dim:])
    _require_cuda(input, "grid_pull")
    if prefilter:
        input = spline_coeff_nd(input, interpolation=list(o), bound=bound, dim=dim)
    x, g, (batch, channel, in_spatial, grid_spatial) = _prep(input, grid, dim)
    out = _GridPull.apply(x, g, b, o, ext)                       # differentiable w.r.t. input and grid (first order)
    return _unprep(out, batch, channel, *grid_spatial)


# ----------------------------------------------------------------------------- resize (bspline_zooming)
_PREFILTER_CACHE = {}
_PREFILTER_FAMILY = {1: 0, 3: 0, 0: 1, 2: 1, 6: 2}               # coeff.py:229-251: DCT-II, DCT-I, DFT conditions
_POLE = {2: 8.0 ** 0.5 - 3.0, 3: 3.0 ** 0.5 - 2.0}                # coeff.py:35-42


def _prefilter_scalars_dev(n, dev, order=3, family=0):
    """_prefilter_scalars with the fp32 table already on the device, cached per (n, device, order, family)."""
    key = (int(n), str(dev), order, family)
    if key not in _PREFILTER_CACHE:
        sc = _prefilter_scalars(n, order, family)
        _PREFILTER_CACHE[key] = sc[:5] + (sc[5].to(dev) if sc[5] is not None and n > 2 else None, sc[6])
    return _PREFILTER_CACHE[key]


def _prefilter_scalars(n, order=3, family=0):
    """The host scalars of coeff.py's one-pole prefilter (orders 2 and 3) for a line of n samples: (pole, gain,
    pole_last, init_scale, final_scale, fp32 table or None, max_iter).  family 0: DCT-II (:55-60, :141-175, :216-224);
    1: DCT-I (:96-140, :207-214); 2: DFT (:69-95, :181-205).  What each scalar means per family: include/brainfm_hip.h."""
    import math
    z = _POLE[order]
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    max_iter = int(math.ceil(-30.0 / math.log(abs(z))))
    if family == 0:
        polen = z ** n
        pole_last = polen * (1 + 1 / (z + polen * polen))
        init_scale = z / (1 - polen * polen)
        final_scale = z / (z - 1)
        zt = torch.as_tensor(z, dtype=torch.float32)
        w = (zt.pow(torch.arange(1, n - 1, dtype=torch.float32)) +
             zt.pow(torch.arange(2 * n - 2, n, -1, dtype=torch.float32)))        # fp32 table exactly as the reference builds it
        return z, gain, pole_last, init_scale, final_scale, w, max_iter
    if family == 1:
        polen = z ** (n - 1)
        return z, gain, polen, 1.0 / (1.0 - polen * polen), z / (z * z - 1.0), None, max_iter
    zm = z ** min(max_iter, n)
    return z, gain, 0.0, 1.0 / (1.0 - zm), 1.0 / (zm - 1.0), None, max_iter


def _coeff_raw(inp, orders, bounds, inplace, dim=3):
    """coeff.py:313-344 over the last three dimensions, one launch per volume and filtered axis (order 2 or 3, length
    above 1).  dim = 2: over the last two, the whole batch as one (N, X, Y) volume filtered along its axes 1 and 2, one
    launch per filtered axis.  Filters `inp` itself only if `inplace` and it is contiguous fp32; returns fp32."""
    vols = inp.to(torch.float32).reshape((-1,) + tuple(inp.shape[-3:])).contiguous()
    if not inplace or vols.data_ptr() != inp.data_ptr():
        vols = vols.clone()
    lib = L.load()
    if dim == 2:
        vols, orders, bounds = vols.reshape((1, -1) + tuple(inp.shape[-2:])), (0,) + tuple(orders[:2]), (0,) + tuple(bounds[:2])
    nx, ny, nz = vols.shape[-3:]
    for v in vols:
        for axis, n in enumerate((nx, ny, nz)):
            if n == 1 or orders[axis] < 2:
                continue
            z, gain, pole_last, init_scale, final_scale, wd, max_iter = _prefilter_scalars_dev(
                n, inp.device, orders[axis], _PREFILTER_FAMILY[bounds[axis]])
            L.check(lib.bfm_bspline3_prefilter_axis(L.ptr(v), nx, ny, nz, axis, bounds[axis], z, gain, L.ptr(wd), pole_last,
                                                    init_scale, final_scale, max_iter, L.stream_ptr()), "bspline3_prefilter")
    return vols.reshape(inp.shape)


class _SplineCoeffND(torch.autograd.Function):
    """autograd.py:276-300: the filter is symmetric, so its backward is the same filter applied to the gradient."""

    @staticmethod
    def forward(ctx, x, orders, bounds, dim=3):
        ctx.opt = (orders, bounds, x.dtype, dim)
        return _coeff_raw(x, orders, bounds, False, dim)

    @staticmethod
    def backward(ctx, grad):
        orders, bounds, dtype, dim = ctx.opt
        return _coeff_raw(grad.contiguous(), orders, bounds, False, dim).to(dtype), None, None, None


def spline_coeff_nd(input, interpolation="linear", bound="dct2", dim=None, inplace=False):
    """utils/interpol/api.py:386-432 -> coeff.py:313-344 over the last three dimensions (`dim` None or 3) or the last two
    (`dim` 2, which reads the first two orders and bounds): orders 2 and 3, per axis if given as a list, under the DCT-I
    ('zero' / 'dct1'), DCT-II ('nearest' / 'dct2') or DFT ('dft') conditions; an axis of order 0 / 1 or of length 1 is
    left as it is.  Differentiable (autograd.py:276-300); `inplace` holds only for a tensor that needs no gradient."""
    inp = input
    orders = _order_list(interpolation)
    bounds = tuple(_bound_list(bound))
    dim = 3 if dim is None else dim
    if dim in (2, 3):
        orders, bounds = orders[:dim], bounds[:dim]
        _check_prefilter_bounds(orders, bounds, inp.shape[-dim:])
    if inp.device.type != "cuda":
        raise L.BfmError("spline_coeff_nd runs on a HIP device only")
    if all(o < 2 for o in orders):
        return inp if inplace else inp.clone()
    if dim not in (2, 3) or inp.dim() < dim:
        raise NotImplementedError("only 2-D and 3-D prefiltering is implemented")
    if torch.is_grad_enabled() and inp.requires_grad:
        return _SplineCoeffND.apply(inp, orders, bounds, dim)
    return _coeff_raw(inp, orders, bounds, inplace, dim)


def _coeff_axis_raw(inp, order, bound, dim):
    """The prefilter of _coeff_raw along one dimension of a tensor of any rank: the contiguous fp32 tensor is the volume
    (everything before `dim`, the length of `dim`, everything behind it) filtered along its middle axis, one launch.
    Filters `inp` itself if it is contiguous fp32, a copy otherwise; returns what it filtered."""
    x = inp.to(torch.float32).contiguous()
    n = x.shape[dim]
    if n > 1 and x.numel():
        outer = 1
        for s in x.shape[:dim]:
            outer *= s
        inner = x.numel() // (outer * n)
        z, gain, pole_last, init_scale, final_scale, wd, max_iter = _prefilter_scalars_dev(
            n, x.device, order, _PREFILTER_FAMILY[bound])
        dims, axis = ((1, outer, n), 2) if inner == 1 else ((outer, n, inner), 1)
        L.check(L.load().bfm_bspline3_prefilter_axis(L.ptr(x), dims[0], dims[1], dims[2], axis, bound, z, gain, L.ptr(wd),
                                                     pole_last, init_scale, final_scale, max_iter, L.stream_ptr()),
                "bspline3_prefilter")
    return x


class _SplineCoeff(torch.autograd.Function):
    """autograd.py:249-273: the filter is symmetric, so its backward is the same filter applied to the gradient."""

    @staticmethod
    def forward(ctx, x, order, bound, dim):
        ctx.opt = (order, bound, dim, x.dtype)
        return _coeff_axis_raw(x.detach().clone(), order, bound, dim).to(x.dtype)

    @staticmethod
    def backward(ctx, grad):
        order, bound, dim, dtype = ctx.opt
        return _coeff_axis_raw(grad.clone(), order, bound, dim).to(dtype), None, None, None


def spline_coeff(input, interpolation="linear", bound="dct2", dim=-1, inplace=False):
    """utils/interpol/api.py:335-383 -> coeff.py:254-310: the interpolating spline coefficients along the one dimension
    `dim` of a tensor of any rank, for one order and one bound.  Orders 2 and 3 under the DCT-I ('zero' / 'dct1'), DCT-II
    ('nearest' / 'dct2') or DFT ('dft') conditions, on the prefilter kernels of spline_coeff_nd (fp32 arithmetic; the
    result has the input's dtype); orders 0 and 1 return the input (a clone unless `inplace`).  'dst1' / 'dst2' and
    orders 4 to 7 raise as in spline_coeff_nd.  Differentiable (autograd.py:249-273); `inplace` holds only for a tensor
    that needs no gradient."""
    orders = interpolation if isinstance(interpolation, (list, tuple)) else [interpolation]
    bounds = bound if isinstance(bound, (list, tuple)) else [bound]
    if len(orders) != 1 or len(bounds) != 1:
        raise ValueError("spline_coeff takes one interpolation order and one bound (spline_coeff_nd takes one per dimension)")
    order = _order_list(orders[0])[0]
    b = _bound_list(bounds[0])[0]
    if not -input.dim() <= dim < input.dim():
        raise IndexError("Dimension out of range (expected to be in range of [%d, %d], but got %d)"
                         % (-input.dim(), input.dim() - 1, dim))
    dim = dim % input.dim()
    _check_prefilter_bounds((order,), (b,), (input.shape[dim],))
    if input.device.type != "cuda":
        raise L.BfmError("spline_coeff runs on a HIP device only")
    if order < 2:
        return input if inplace else input.clone()
    if not input.dtype.is_floating_point:
        input, inplace = input.to(torch.float32), False
    if torch.is_grad_enabled() and input.requires_grad:
        return _SplineCoeff.apply(input, order, b, dim)
    if not inplace:
        return _coeff_axis_raw(input.clone(), order, b, dim).to(input.dtype)
    res = _coeff_axis_raw(input, order, b, dim)
    if res.data_ptr() != input.data_ptr():                        # not contiguous fp32: filtered in a copy
        input.copy_(res)
    return input


# ----------------------------------------------------------------------------- grid builders (api.py:455-560)
def _builder_dtype(dtype):
    dtype = torch.get_default_dtype() if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("grid builders: float32 or float64, not %s" % dtype)
    return dtype


def _affine_raw(mat, nb, shape, dtype, device):
    """mat (nb,3,4) contiguous on the device, or None for the identity -> (nb,*shape,3)"""
    out = torch.empty((nb,) + tuple(shape) + (3,), dtype=dtype, device=device)
    if out.numel():
        L.check(L.load().bfm_affine_grid3d(L.ptr(mat), int(dtype == torch.float64), nb, shape[0], shape[1], shape[2],
                                           L.ptr(out), L.stream_ptr()), "affine_grid3d")
    return out


def identity_grid(shape, dtype=None, device=None):
    """api.py:455-476: the (*shape, dim) grid of voxel indices, dim = len(shape).  3-D shapes are written by one kernel
    (no meshgrid); 1-D and 2-D shapes are built with torch on the device (a 2-D grid is what grid_pull / grid_push /
    grid_count take on spline_grid.hip; no kernel of this package reads a 1-D grid)."""
    shape = tuple(int(s) for s in shape)
    dtype = _builder_dtype(dtype)
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise L.BfmError("identity_grid runs on a HIP device only; there is no CPU fallback in the product path")
    if len(shape) != 3:
        mesh = torch.meshgrid(*[torch.arange(s, dtype=dtype, device=device) for s in shape], indexing="ij")
        return torch.stack(mesh, dim=-1)
    with torch.cuda.device(device):
        return _affine_raw(None, 1, shape, dtype, device)[0]


def add_identity_grid_(disp):
    """api.py:479-503: adds the voxel index to a displacement field (..., *spatial, dim) in place and returns it."""
    dim = disp.shape[-1]
    if disp.dim() < dim + 1:
        raise ValueError("add_identity_grid_: a (..., *spatial, %d) field has at least %d dimensions" % (dim, dim + 1))
    _require_cuda(disp, "add_identity_grid_")
    if dim != 3:
        for i, s in enumerate(disp.shape[-dim - 1:-1]):
            view = [1] * dim
            view[i] = s
            disp[..., i].add_(torch.arange(s, dtype=disp.dtype, device=disp.device).reshape(view))
        return disp
    _builder_dtype(disp.dtype)
    work = disp if disp.is_contiguous() else disp.contiguous()
    if work.numel():
        nx, ny, nz = work.shape[-4:-1]
        L.check(L.load().bfm_add_identity_grid3d(L.ptr(work), int(work.dtype == torch.float64), work.numel() // (nx * ny * nz * 3),
                                                 nx, ny, nz, L.stream_ptr()), "add_identity_grid3d")
    if work is not disp:
        disp.copy_(work)
    return disp


def add_identity_grid(disp):
    """api.py:506-521: add_identity_grid_ on a copy."""
    _require_cuda(disp, "add_identity_grid")
    return add_identity_grid_(disp.clone(memory_format=torch.contiguous_format))


def affine_grid(mat, shape):
    """api.py:524-560: the dense grid (..., *shape, D) of an affine matrix (..., D[+1], D+1): lin @ index + offset per
    voxel, in the reference's summation order.  Batched matrices give one grid per matrix (the reference means to, its
    docstring says so, but raises on them).  3-D on one kernel, 1-D / 2-D with torch on the device."""
    mat = torch.as_tensor(mat)
    shape = [int(s) for s in shape]
    nb_dim = mat.shape[-1] - 1
    if nb_dim != len(shape):
        raise ValueError("Dimension of the affine matrix ({}) and shape ({}) are not the same.".format(nb_dim, len(shape)))
    if mat.dim() < 2 or mat.shape[-2] not in (nb_dim, nb_dim + 1):
        raise ValueError("First argument should be matrices of shape (..., {0}, {1}) or (..., {1}, {1}) but got {2}."
                         .format(nb_dim, nb_dim + 1, tuple(mat.shape)))
    _require_cuda(mat, "affine_grid")
    batch = tuple(mat.shape[:-2])
    if nb_dim != 3:
        grid = identity_grid(shape, mat.dtype, mat.device)
        lin = mat[..., :nb_dim, :nb_dim].reshape(batch + (1,) * nb_dim + (nb_dim, nb_dim))
        off = mat[..., :nb_dim, -1].reshape(batch + (1,) * nb_dim + (nb_dim,))
        return torch.matmul(lin, grid[..., None])[..., 0] + off
    dtype = _builder_dtype(mat.dtype)
    m = mat[..., :3, :].reshape(-1, 3, 4).contiguous()
    if m.shape[0] == 0:
        return torch.empty(batch + tuple(shape) + (3,), dtype=dtype, device=mat.device)
    with torch.cuda.device(mat.device):
        return _affine_raw(m, m.shape[0], shape, dtype, mat.device).reshape(batch + tuple(shape) + (3,))


def _make_list(x, n=None):
    x = list(x) if isinstance(x, (list, tuple)) else [x]
    if n is not None and len(x) < n:
        x = x + [x[-1]] * (n - len(x))
    return x


def _anchor_coords(anchor, f, n_src, n_dst):
    """resize.py:86-104 / restrict.py:81-104: the coordinates of the n_dst samples of a resampled axis in the lattice of
    its n_src samples, for the anchors 'c' (centers of the corner voxels aligned), 'e' (edges aligned), 'f' / 'l' (first /
    last voxel aligned, spacing 1 / f).  fp32 on the host: the same values as torch on the CPU."""
    if anchor == "c":
        return torch.linspace(0, n_src - 1, n_dst, dtype=torch.float32)
    if anchor == "e":
        scale = n_src / n_dst
        return torch.arange(0., n_dst, dtype=torch.float32) * scale + 0.5 * (scale - 1)
    if anchor == "f":
        return torch.arange(0., n_dst, dtype=torch.float32) / f
    if anchor == "l":
        return torch.arange(0., n_dst, dtype=torch.float32) / f + ((n_src - 1) - (n_dst - 1) / f)
    raise ValueError("Unknown anchor {}".format(anchor))


def resize(image, factor=None, shape=None, anchor="c", interpolation=1, prefilter=True, **kwargs):
    """utils/interpol/resize.py:13-119.  image: (..., X, Y, Z).  Cubic (interpolation=3) with extrapolation under the
    'nearest' / 'dct2' bounds runs as prefilter + three separable 4-tap passes; every other case (orders 0 to 3, any
    bound, extrapolate=False) builds the grid and goes through grid_pull like the reference.  Two entries in `factor`,
    `shape` or `anchor` (or none and an image (B, C, X, Y)) make it a 2-D resize of (..., X, Y), which always takes the
    grid route, on the 2-D grid_pull."""
    orders = _order_list(kwargs.get("interpolation", interpolation))
    if image.device.type != "cuda":
        raise L.BfmError("resize runs on a HIP device only; there is no CPU fallback in the product path")
    factor = _make_list(factor) if factor else []
    shape = _make_list(shape) if shape else []
    anchor = _make_list(anchor)
    nb_dim = max(len(factor), len(shape), len(anchor)) or (image.dim() - 2)
    if nb_dim not in (2, 3):
        raise NotImplementedError("only 2-D and 3-D resize is implemented")
    anchor = [a[0].lower() for a in _make_list(anchor, nb_dim)]
    inshape = image.shape[-nb_dim:]
    if factor:
        factor = _make_list(factor, nb_dim)
    elif not shape:
        raise ValueError("One of `factor` or `shape` must be provided")
    if shape:
        shape = _make_list(shape, nb_dim)
    else:
        shape = [int(i * f) for i, f in zip(inshape, factor)]
    if not factor:
        factor = [o / i for o, i in zip(shape, inshape)]
    lin = [_anchor_coords(anch, f, inshp, outshp) for anch, f, inshp, outshp in zip(anchor, factor, inshape, shape)]
    bound = kwargs.get("bound", "nearest")
    prefilter = kwargs.get("prefilter", prefilter)
    bl = _bound_list(bound)
    b = bl[0] if bl[0] in (1, 3) and bl == [bl[0]] * 3 else None           # the separable path: 'nearest' / 'dct2'
    if nb_dim != 3 or orders != (3, 3, 3) or not kwargs.get("extrapolate", True) or b is None:
        # every case but the separable cubic one: build the grid and pull, like the reference (resize.py:111-117).  Below
        # order 2 there is nothing to prefilter, and the flag is dropped here, so that a label map still resizes at those
        # orders (grid_pull refuses a label map with prefilter=True)
        grid = torch.stack(torch.meshgrid(*[v.to(image.device) for v in lin], indexing="ij"), dim=-1)
        return grid_pull(image, grid, interpolation=list(orders), bound=bound, extrapolate=kwargs.get("extrapolate", True),
                         prefilter=prefilter and any(o >= 2 for o in orders[:nb_dim]))
    coeff = spline_coeff_nd(image, interpolation=3, bound=b, dim=3) if prefilter else image.to(torch.float32)
    lead = coeff.shape[:-3]
    vols = coeff.reshape((-1,) + tuple(coeff.shape[-3:])).contiguous()
    out = _ResizeCubic.apply(vols, [v.to(image.device) for v in lin], tuple(shape), b)
    return out.reshape(tuple(lead) + tuple(shape))


class _ResizeCubic(torch.autograd.Function):
    """The separable cubic route of resize: three 4-tap passes per volume (spline.hip).  Its backward is the transposed
    operator of each axis (restrict.hip) applied in reverse axis order, all volumes in one launch per axis."""

    @staticmethod
    def forward(ctx, vols, coords, shape, b):
        ctx.opt = (coords, tuple(vols.shape[1:]), b)
        lib = L.load()
        outs = []
        for v in vols:
            cur = v
            dims = list(v.shape)
            for axis in range(3):
                nxt_dims = list(dims)
                nxt_dims[axis] = shape[axis]
                nxt = torch.empty(nxt_dims, dtype=torch.float32, device=vols.device)
                L.check(lib.bfm_bspline3_resample_axis(L.ptr(cur), dims[0], dims[1], dims[2], axis, L.ptr(coords[axis]),
                                                       shape[axis], b, L.ptr(nxt), L.stream_ptr()), "bspline3_resample")
                cur, dims = nxt, nxt_dims
            outs.append(cur)
        return torch.stack(outs, 0) if len(outs) > 1 else outs[0][None]

    @staticmethod
    def backward(ctx, grad):
        coords, inshape, b = ctx.opt
        cur = grad.contiguous().to(torch.float32)
        for axis in (2, 1, 0):
            cur = _axis_pass(cur, axis, _axis_table(coords[axis], inshape[axis], 3, b, 1, True))
        return cur, None, None, None


# ----------------------------------------------------------------------------- separable axis operators (restrict.hip)
def _axis_table(coord, n, order, bound, ext, transpose, ties_even=False):
    """The sparse operator of the fp32 device coordinates `coord` against an axis of n nodes as a CSR table (rowptr, col,
    val, rows): rows = len(coord) in the pull direction, n in the transposed (push) direction.  ties_even: the node of
    an order-0 axis is round(coord) as in iso0.py, not floor(coord + 0.5)."""
    lib = L.load()
    m = coord.numel()
    rows = n if transpose else m
    rowptr = torch.empty(rows + 1, dtype=torch.int32, device=coord.device)
    col = torch.empty(m * (order + 1), dtype=torch.int32, device=coord.device)
    val = torch.empty(m * (order + 1), dtype=torch.float32, device=coord.device)
    nbytes = lib.bfm_spline_axis_table_workspace(m, n, order) if transpose else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=coord.device) if transpose else None
    L.check(lib.bfm_spline_axis_table(L.ptr(coord), m, n, order, bound, ext, int(ties_even), int(transpose), L.ptr(rowptr),
                                      L.ptr(col), L.ptr(val), L.ptr(ws), nbytes, L.stream_ptr()), "spline_axis_table")
    return rowptr, col, val, rows


def _axis_pass(x, axis, table):
    """x (lead, X, Y, Z) contiguous fp32 -> the same block with `axis` (0, 1, 2) mapped through `table`."""
    rowptr, col, val, rows = table
    dims = list(x.shape)
    out_dims = list(dims)
    out_dims[axis + 1] = rows
    out = torch.empty(out_dims, dtype=torch.float32, device=x.device)
    if out.numel():
        L.check(L.load().bfm_spline_axis_pass(L.ptr(x), dims[0], dims[1], dims[2], dims[3], axis, L.ptr(rowptr), L.ptr(col),
                                              L.ptr(val), rows, L.ptr(out), L.stream_ptr()), "spline_axis_pass")
    return out


class _SeparablePush(torch.autograd.Function):
    """grid_push on the meshgrid of three coordinate lists as three transposed axis passes, x then y then z (the order is
    part of the result: it fixes the last bit).  Backward: the pull-direction passes of the same coordinates, z, y, x."""

    @staticmethod
    def forward(ctx, x, coords, shape, orders, bounds, ext):
        ctx.opt = (coords, shape, orders, bounds, ext)
        cur = x
        iso0 = orders == (0, 0, 0)                   # the reference then takes iso0.py, which rounds ties to even
        for axis in (0, 1, 2):
            cur = _axis_pass(cur, axis, _axis_table(coords[axis], shape[axis], orders[axis], bounds[axis], ext, True, iso0))
        return cur

    @staticmethod
    def backward(ctx, grad):
        coords, shape, orders, bounds, ext = ctx.opt
        cur = grad.contiguous().to(torch.float32)
        iso0 = orders == (0, 0, 0)
        for axis in (2, 1, 0):
            cur = _axis_pass(cur, axis, _axis_table(coords[axis], shape[axis], orders[axis], bounds[axis], ext, False, iso0))
        return cur, None, None, None, None, None


def _restrict_geometry(image_shape, factor=None, shape=None, anchor="c"):
    """restrict.py:66-110 as it stands: (output shape, fp32 host coordinates of the input samples in the output lattice,
    one list per axis, fullscale).  Anchor 'c' with an output axis of length 1 divides by zero, as there."""
    factor = _make_list(factor) if factor else []
    shape = _make_list(shape) if shape else []
    anchor = _make_list(anchor)
    nb_dim = max(len(factor), len(shape), len(anchor)) or (len(image_shape) - 2)
    if nb_dim != 3:
        raise NotImplementedError("only 3-D restrict is implemented (factor, shape and anchor set the number of "
                                  "dimensions: %d here)" % nb_dim)
    anchor = [a[0].lower() for a in _make_list(anchor, nb_dim)]
    inshape = tuple(image_shape[-nb_dim:])
    if factor:
        factor = _make_list(factor, nb_dim)
    elif not shape:
        raise ValueError("One of `factor` or `shape` must be provided")
    if shape:
        shape = _make_list(shape, nb_dim)
    else:
        shape = [int(i / f) for i, f in zip(inshape, factor)]
    if not factor:
        factor = [i / o for o, i in zip(shape, inshape)]
    lin = []
    fullscale = 1
    for anch, f, inshp, outshp in zip(anchor, factor, inshape, shape):
        lin.append(_anchor_coords(anch, f, outshp, inshp))                     # resize's lattice, input and output swapped
        fullscale *= (inshp - 1) / (outshp - 1) if anch == "c" else (outshp / inshp if anch == "e" else 1 / f)
    return tuple(int(v) for v in shape), lin, fullscale


def restrict(image, factor=None, shape=None, anchor="c", interpolation=1, reduce_sum=False, **kwargs):
    """utils/interpol/restrict.py:9-122, the adjoint of resize: image (..., X, Y, Z) is splatted onto the coarser lattice
    of `shape` (or int(in / factor)) and divided by `fullscale` unless `reduce_sum`.  kwargs: bound ('nearest'),
    extrapolate (True), interpolation (overrides the argument), prefilter (False; filters the result, like grid_push).
    Orders 0 to 3 per axis, all seven bounds.  The grid is separable, so the push runs as three axis passes without
    atomics (x, then y, then z): deterministic, and differentiable to first order in `image`.  Returns fp32."""
    unknown = sorted(set(kwargs) - {"bound", "extrapolate", "interpolation", "prefilter"})
    if unknown:
        raise TypeError("grid_push() got an unexpected keyword argument '%s'" % unknown[0])
    orders = _order_list(kwargs.get("interpolation", interpolation))
    shape, lin, fullscale = _restrict_geometry(tuple(image.shape), factor, shape, anchor)
    bound = kwargs.get("bound", "nearest")
    b = _bound_list(bound)
    ext = _extrap(kwargs.get("extrapolate", True))
    if any(not 0 <= v <= 6 for v in b) or not 0 <= ext <= 2:
        raise ValueError("Unknown bound or extrapolate value")
    prefilter = _needs_prefilter(kwargs.get("prefilter", False), orders, b, shape)
    _require_cuda(image, "restrict")
    lead = tuple(image.shape[:-3])
    x = image.to(torch.float32).reshape((-1,) + tuple(image.shape[-3:])).contiguous()
    out = _SeparablePush.apply(x, [v.to(image.device) for v in lin], shape, orders, tuple(b), ext)
    if prefilter:
        out = spline_coeff_nd(out, interpolation=list(orders), bound=bound, dim=3, inplace=True)
    if not reduce_sum:
        out = out.div_(fullscale)
    return out.reshape(lead + shape)
