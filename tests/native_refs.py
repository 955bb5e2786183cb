"""NumPy restatements behind tests/test_host_native.py and tests/test_gpu_native.py (no torch device code).

    coords            the coordinate rule of csrc/affine_pull.hip, float64, bit for bit
    linear_exact      the zero-padded trilinear sum with float64 weights and float64 products (and sum |w||v|)
    linear_f32        the kernel's float32 chain, bit for bit
    nearest           floor(x + 0.5), bit patterns copied, 0 outside
    argmax_labels     first strict positive maximum over the channels of linear_f32, through a lut
    prepare_voxel_map the explicit resize -> align -> crop map of prepare_image in voxel coordinates
"""
import numpy as np

from brainfm_amd import misc as MI

F32 = np.float32


def coords(M, shape):
    """x_r[i,j,k] = ((M[r][0]*i + M[r][1]*j) + M[r][2]*k) + M[r][3] in float64, one rounding per operation (NumPy does
    not contract).  M: anything whose first three rows are the 3 x 4 matrix."""
    M = np.asarray(M, dtype=np.float64)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return tuple(((M[r, 0] * i + M[r, 1] * j) + M[r, 2] * k) + M[r, 3] for r in range(3))


def _corners(src_shape, x, y, z):
    """floor indices (int64, 0 where the footprint is outside), the `any` mask and the float64 fractions."""
    D, H, W = src_shape
    ok = (x > -1.0) & (x < D) & (y > -1.0) & (y < H) & (z > -1.0) & (z < W)
    fl = [np.floor(np.where(ok, c, 0.0)) for c in (x, y, z)]
    frac = [np.where(ok, c, 0.0) - f for c, f in zip((x, y, z), fl)]
    return [f.astype(np.int64) for f in fl], ok, frac


def _texel(src, ix, iy, iz, pad):
    D, H, W = src.shape
    inside = (ix >= 0) & (ix < D) & (iy >= 0) & (iy < H) & (iz >= 0) & (iz < W)
    v = src[np.clip(ix, 0, D - 1), np.clip(iy, 0, H - 1), np.clip(iz, 0, W - 1)]
    if pad == "clamp":                                   # the named mistake: replicate the border instead of zeros
        return v
    return np.where(inside, v, src.dtype.type(0))


def linear_exact(src, x, y, z, pad="zeros", weights="f64"):
    """(value, sum |w||v|): sum over the eight corners of w * v in float64, w the product of the axis weights and v the
    texel (0 outside the source).  weights='f64': wc = x - floor(x), wf = 1 - wc in float64, the trilinear sum itself
    (what grid_sample computes).  weights='f32': the weights the kernel forms, wc = (float)(x - floor(x)), wf = 1.f - wc,
    taken as exact numbers -- the sum the float32 chain approximates by rounding its products and additions."""
    src = np.asarray(src, dtype=np.float64)
    (fx, fy, fz), ok, frac = _corners(src.shape, x, y, z)
    if weights == "f32":
        wc = [f.astype(F32) for f in frac]
        wf = [(F32(1) - w).astype(np.float64) for w in wc]
        wc = [w.astype(np.float64) for w in wc]
    else:
        wc = frac
        wf = [1.0 - w for w in wc]
    val = np.zeros(x.shape, dtype=np.float64)
    mag = np.zeros(x.shape, dtype=np.float64)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = (wc[0] if a else wf[0]) * (wc[1] if b else wf[1]) * (wc[2] if c else wf[2])
                v = _texel(src, fx + a, fy + b, fz + c, pad)
                val += w * v
                mag += np.abs(w) * np.abs(v)
    return np.where(ok, val, 0.0), np.where(ok, mag, 0.0)


def corner_abs_sum(src, x, y, z):
    """sum of |v| over the eight corners (0 outside the source), for weight_rounding_bound."""
    src = np.asarray(src, dtype=np.float64)
    (fx, fy, fz), ok, _ = _corners(src.shape, x, y, z)
    tot = np.zeros(x.shape, dtype=np.float64)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                tot += np.abs(_texel(src, fx + a, fy + b, fz + c, "zeros"))
    return np.where(ok, tot, 0.0)


def weight_rounding_bound(vsum):
    """|sum with the kernel's float32 weights - sum with float64 weights|.  wc < 1 is rounded to float32 with an error
    of at most 2^-25; wf = 1.f - wc inherits it and adds at most 2^-25 of its own (nothing when wc >= 0.5, where the
    subtraction is exact), so an axis weight is off by at most 2^-24 and a product of three weights, each at most 1, by
    at most 3 * 2^-24 to first order; 3.01 covers the second-order terms.  Absolute, not relative to the weight: where a
    small weight's partner belongs to a zero texel (the zero padding just inside the far border, say) this term and not
    bound() is what holds the chain to the float64 trilinear value."""
    return 3.01 * 2.0 ** -24 * vsum


def linear_f32(src, x, y, z):
    """The kernel's arithmetic: wc = (float)(x - floor(x)), wf = 1.f - wc, the c00, c01, c10, c11, c0, c1, c chain of
    gather3d.h's trilin_lerp in float32, one rounding per operation."""
    src = np.asarray(src, dtype=F32)
    (fx, fy, fz), ok, frac = _corners(src.shape, x, y, z)
    wcx, wcy, wcz = [f.astype(F32) for f in frac]
    wfx, wfy, wfz = [F32(1) - w for w in (wcx, wcy, wcz)]
    t = lambda a, b, c: _texel(src, fx + a, fy + b, fz + c, "zeros")
    c00 = t(0, 0, 0) * wfx + t(1, 0, 0) * wcx
    c01 = t(0, 0, 1) * wfx + t(1, 0, 1) * wcx
    c10 = t(0, 1, 0) * wfx + t(1, 1, 0) * wcx
    c11 = t(0, 1, 1) * wfx + t(1, 1, 1) * wcx
    c0 = c00 * wfy + c10 * wcy
    c1 = c01 * wfy + c11 * wcy
    out = c0 * wfz + c1 * wcz
    assert out.dtype == F32
    return np.where(ok, out, F32(0))


def nearest(src, x, y, z, rounding="floor"):
    """src[floor(x + 0.5), ...] with the 4-byte pattern kept, 0 outside.  rounding='even' is the named mistake (np.round
    rounds half to even, as grid_sample does)."""
    src = np.asarray(src)
    assert src.dtype.itemsize == 4
    D, H, W = src.shape
    r = [np.floor(c + 0.5) if rounding == "floor" else np.round(c) for c in (x, y, z)]
    ok = (r[0] >= 0) & (r[0] < D) & (r[1] >= 0) & (r[1] < H) & (r[2] >= 0) & (r[2] < W)
    ix, iy, iz = [np.where(ok, c, 0.0).astype(np.int64) for c in r]
    bits = src.view(np.uint32)[ix, iy, iz]
    return np.where(ok, bits, np.uint32(0)).view(src.dtype)


def argmax_labels(post_cl, lut, x, y, z, take="first"):
    """(label int32, best float32) from channels-last posteriors (D,H,W,C): each channel through linear_f32, the winner
    the first channel whose value is > 0 and > every earlier one (a NaN never wins), label 0 and best 0 where there is
    none.  take='last' is the named mistake (>= keeps the last of equal maxima)."""
    post_cl = np.asarray(post_cl, dtype=F32)
    lut = np.asarray(lut, dtype=np.int32)
    best = np.zeros(x.shape, dtype=F32)
    chan = np.full(x.shape, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(post_cl.shape[-1]):
            v = linear_f32(post_cl[..., c], x, y, z)
            win = (v > best) if take == "first" else ((v >= best) & (v > 0))
            best = np.where(win, v, best)
            chan = np.where(win, c, chan)
    return np.where(chan >= 0, lut[np.maximum(chan, 0)], 0).astype(np.int32), best


# ------------------------------------------------------------------------------------------------- the shared cases
SRC = (5, 6, 7)
DSTS = ((9, 7, 8), (3, 5, 67), (1, 1, 1))      # (3,5,67): a z row that crosses one wave; (1,1,1): a single voxel


def _rot_shear():
    a, b = 0.35, -0.2
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Sh = np.array([[1, 0.15, 0], [0, 1, -0.1], [0.05, 0, 1]])
    return 0.55 * (Rz @ Ry @ Sh)


def matrices(dst):
    """name -> 3 x 4 float64 matrix (destination index -> source coordinate) for a destination shape.  `half_free` names
    those none of whose coordinates comes within 1e-6 of a half-integer (checked by the host test)."""
    c_src = (np.array(SRC) - 1) / 2.0
    c_dst = (np.array(dst) - 1) / 2.0
    lin = _rot_shear()
    scale = np.array([0.5, 0.75, 1.25]) if dst[2] < 32 else np.array([0.5, 0.75, 0.125])
    out = {
        "identity": np.hstack([np.eye(3), np.zeros((3, 1))]),
        # x = 5 - j, y = k - 1, z = i + 2: weights exactly 0 and 1, part of the destination outside
        "signed_perm": np.array([[0., -1, 0, 5], [0, 0, 1, -1], [1, 0, 0, 2]]),
        # coordinates on quarters and halves: exact weights 0.25 / 0.5 / 0.75 and exact ties of floor(x + 0.5) vs round
        "aniso_half": np.hstack([np.diag(scale), np.array([[-0.25], [0.5], [-0.5]])]),
        "aniso_third": np.hstack([np.diag([0.8 / 1.0, 1.0 / 1.1, 1.3 / 3.0 if dst[2] > 32 else 1.3]),
                                  np.array([[-0.13], [0.05], [-0.15]])]),
        "rot_shear": np.hstack([lin, (c_src + np.array([0.13, -0.21, 0.17]) - lin @ c_dst)[:, None]]),
        "mostly_outside": np.array([[1.1, 0, 0, 3.37], [0, 1.1, 0.05, -5.01],
                                    [0, 0.02, 1.1 if dst[2] < 32 else 0.11, 5.235]]),
    }
    return out


HALF_FREE = ("identity", "signed_perm", "aniso_third", "rot_shear", "mostly_outside")


def source(K=1, seed=0):
    """K signed float32 maps on SRC."""
    return np.random.RandomState(seed).randn(K, *SRC).astype(F32)


def posteriors(C, seed=0):
    """Channels-last softmax posteriors (D,H,W,C) on SRC with planted exact ties and all-zero voxels.
    Ties: at every voxel with (x + y + z) % 3 == 0 the largest value is copied into one more channel (C >= 2), so two
    channels hold the same maximum there and, wherever the weights are exact, after interpolation too.
    Zeros: the voxels of the plane x == 1 are 0 in every channel."""
    rs = np.random.RandomState(100 + C + seed)
    logit = rs.randn(*SRC, C) * 2.0
    p = np.exp(logit - logit.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(F32)
    if C >= 2:
        ix, iy, iz = np.meshgrid(*[np.arange(n) for n in SRC], indexing="ij")
        tie = (ix + iy + iz) % 3 == 0
        top = p.argmax(-1)
        other = (top + 1 + rs.randint(0, C - 1, size=SRC)) % C
        pt = p.copy()
        np.put_along_axis(pt, other[..., None], p.max(-1, keepdims=True), axis=-1)
        p = np.where(tie[..., None], pt, p)
    p[1] = 0
    return p


def lut_for(C):
    return ((np.arange(C) * 7 + 3) % 251).astype(np.int32)


def bound(mag):
    """The float32 chain against the float64 sum over the same weights (linear_exact(weights='f32')): two roundings for
    a weight product, one for the texel product and seven additions, rounded up to 12 units of 2^-24 of sum |w||v|.
    The count holds no rounding for FORMING a weight, so w are the weights the chain is given; against the float64
    weights the same figure fails where a weight is small and its partner multiplies a zero texel (z = 6.976 in a
    source of 7 planes: error 1.41 x this bound, found with 17 random maps on (3,5,67) under 'rot_shear') -- that
    distance is weight_rounding_bound's."""
    return 12.0 * 2.0 ** -24 * mag


def zoom_affine(aff, shape, newsize):
    """The affine update of myzoom_torch_anisotropic (utils/misc.py:1106-1114)."""
    factors = np.array(newsize) / np.array(shape)
    out = aff.copy()
    for c in range(3):
        out[:-1, c] = out[:-1, c] / factors[c]
    out[:-1, -1] = out[:-1, -1] - aff[:-1, :-1] @ (0.5 - 0.5 / factors)
    return out


def prepare_voxel_map(native_shape, native_aff, win_size=None, half_voxel=True, flip_offset=1, align=True):
    """(4 x 4 map native voxel index -> processed voxel coordinates, processed shape) written out step by step:

    resize  output index p of an axis samples the input at delta + p / factor, delta = (1 - factor) / (2 factor)
            (utils/misc.py:1060-1066), so p = (v - delta) * factor;
    align   aligned[i] = resized[j] with j[perm[a]] = flip[a] ? n - 1 - i_a : i_a (misc.align_plan);
    crop    i -= max(S - win, 0) // 2 when any axis exceeds the window (center_crop).

    align=True is the map onto prepare_image's `orig`.  align=False leaves the middle step out: the map onto `final` and
    `high_res`, which prepare_image (like the reference) sends through align_volume_to_ref with the affine of the already
    aligned volume, so that nothing is swapped or flipped -- the grid every inference output lies on.
    half_voxel=False drops delta and flip_offset=0 uses n instead of n - 1: the named mistakes."""
    native_aff = np.asarray(native_aff, dtype=np.float64)
    newsize, _ = MI.resize_plan(tuple(native_shape), native_aff, 1.)
    factors = np.array(newsize) / np.array(native_shape)
    Z = np.eye(4)
    for a in range(3):
        delta = (1.0 - factors[a]) / (2.0 * factors[a]) if half_voxel else 0.0
        Z[a, a] = factors[a]
        Z[a, 3] = -delta * factors[a]
    perm, flip, _ = MI.align_plan(tuple(int(n) for n in newsize), zoom_affine(native_aff, native_shape, newsize),
                                  np.eye(4), 3)
    if not align:
        perm, flip = [0, 1, 2], [0, 0, 0]
    P = np.zeros((4, 4))
    P[3, 3] = 1.0
    for a in range(3):
        n = int(newsize[perm[a]])
        P[a, perm[a]] = -1.0 if flip[a] else 1.0
        P[a, 3] = (n - flip_offset) if flip[a] else 0.0
    full = [int(newsize[perm[a]]) for a in range(3)]
    Cm = np.eye(4)
    shape = list(full)
    if win_size is not None and any(full[a] > win_size[a] for a in range(3)):
        for a in range(3):
            Cm[a, 3] = -(max(full[a] - win_size[a], 0) // 2)
            shape[a] = min(full[a] + int(Cm[a, 3]), win_size[a])
    return Cm @ P @ Z, tuple(shape)
