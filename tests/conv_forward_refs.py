"""Float64 references of the forward 3x3x3 convolution kernels (brainfm_amd/csrc/conv3d_mfma.hip, conv3d_wino.hip,
conv3d_direct.hip), written from the definitions.

Plain helpers, no test in here: tests/test_host_conv_forward_refs.py pins them on the CPU, tests/test_gpu_conv_forward.py
compares the HIP kernels with them.  Tensors are channels-last, (D, H, W, C), as the kernels see them; weights are
(Cout, Cin, 3, 3, 3).

conv_ref is the operation itself, SingleConv 'gcl' after the statistics:
    LeakyReLU_slope(prior + conv3d(zero_pad(x * scale + shift), w)),  x = cat(A, nearest_up(B))
with the zero padding applied AFTER the affine.  split_emulation is the arithmetic the header of conv3d_mfma.hip documents
for the matrix-core kernels: both operands pre-scaled by a power of two, split into fp16 hi + lo, products hi*hi + hi*lo +
lo*hi (passes = 3) or hi*hi alone (passes = 1), here with every product and the sum exact (float64).  The kernels'
activation operand is one fmaf (affine_fp32(fused=True)); the one-pass kernels round it to fp16 once (affine_hi_once).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from backward_refs import join as _join, rel_err, up_maps  # noqa: F401  (re-exported: one join / up_maps for both families)

TERMS = {1: ("hh",), 3: ("hh", "hl", "lh")}


def join(A, B=None, maps=None):
    """The virtual concat of the skip tensor A and the nearest-upsampled low tensor B (backward_refs.join)."""
    return _join(A, B, maps)


def lrelu(p, slope):
    return torch.where(p >= 0, p, p * slope)


def _conv_cl(x, w):
    """conv3d(padding=1, no bias) of a channels-last (D, H, W, Cin) tensor, channels-last out, in x's dtype."""
    return F.conv3d(x.permute(3, 0, 1, 2)[None], w.to(x.dtype), None, padding=1)[0].permute(1, 2, 3, 0)


def conv_ref(A, B, maps, scale, shift, w, slope, prior=None):
    """LeakyReLU(prior + conv3d(zero_pad(affine(cat(A, up(B)))), w)) in float64: the affine first, then the padding.
    prior (D, H, W, Cout) or None: what accumulate mode finds in `out`."""
    x = join(A.double(), None if B is None else B.double(), maps) * scale.double() + shift.double()
    p = _conv_cl(x, w.double())
    if prior is not None:
        p = p + prior.double()
    return lrelu(p, slope)


def affine_fp32(X, scale, shift, fused=False):
    """x * scale + shift in fp32, the y32 that split_emulation takes: as a separate multiply and add (two roundings; the
    library is built without contraction), or with fused=True as the one fmaf the kernels spell out (one rounding: the
    product of two fp32 values is exact in float64, and the sum is rounded to fp32 from there)."""
    if fused:
        return (X.float().double() * scale.float().double() + shift.float().double()).float()
    return (X.float() * scale.float()) + shift.float()


def prescale_exp(vmax):
    """The power-of-two pre-scale exponent the kernels derive from a bound / from max |w|: 14 - frexp(vmax).exponent,
    clamped to +-60; 0 for 0, inf or nan."""
    vmax = float(vmax)
    if not (vmax > 0.0 and math.isfinite(vmax)):
        return 0
    return max(-60, min(60, 14 - math.frexp(vmax)[1]))


def split_hi_lo(v32, exp):
    """v * 2^exp in fp32 -> (hi, lo) as float64 tensors: hi = fp16(v) rounded to nearest even, lo = fp16(v - hi)."""
    v = v32.float() * (2.0 ** exp)
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double(), lo.double()


def affine_hi_once(X, scale, shift, bound_max):
    """The activation hi plane of the passes = 1 kernels, as a float64 tensor: fp16(2^aexp (x * scale + shift)) rounded ONCE
    from the exact value (their staging compiles to v_fma_mixlo_f16: the fp32 affine is never rounded on its own).  It
    differs from fp16(fp32 affine) where the fp32 value is an fp16 tie that the exact value is not.  numpy converts
    float64 to float16 directly (torch goes through float32, which would round twice again)."""
    exact = (X.float().double() * scale.float().double() + shift.float().double()) * (2.0 ** prescale_exp(bound_max))
    return torch.from_numpy(exact.numpy().astype(np.float16).astype(np.float64))


def split_emulation(y32, w, bound_max, wmax, terms=3, a_hi=None):
    """The documented numerics of conv3d_mfma.hip on the affine-applied fp32 input y32 (D, H, W, Cin): the pre-activation
    convolution (D, H, W, Cout) in float64.  terms = 1: hi*hi; terms = 3: hi*hi + hi*lo + lo*hi; or a tuple out of
    'hh', 'hl' (activation hi x weight lo), 'lh' (activation lo x weight hi) to leave one out.  a_hi: the pre-scaled
    activation hi plane to use in place of fp16(y32 2^aexp) (affine_hi_once, for the passes = 1 kernels)."""
    names = TERMS[terms] if isinstance(terms, int) else tuple(terms)
    aexp, wexp = prescale_exp(bound_max), prescale_exp(wmax)
    ahi, alo = split_hi_lo(y32, aexp)
    if a_hi is not None:
        ahi = a_hi.double()
    whi, wlo = split_hi_lo(w, wexp)
    ops = {"hh": (ahi, whi), "hl": (ahi, wlo), "lh": (alo, whi)}
    acc = None
    for n in names:
        t = _conv_cl(*ops[n])
        acc = t if acc is None else acc + t
    return acc * (2.0 ** -(aexp + wexp))


def group_bound(Y, groups):
    """Per-group max |y| of the affine-applied input Y (D, H, W, C): what bfm_gn_stats hands the kernels as `bound`."""
    c = Y.shape[-1]
    return Y.abs().reshape(-1, groups, c // groups).amax((0, 2)).float().contiguous()
