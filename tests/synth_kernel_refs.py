"""Case lists and references of the kernel-by-kernel tests of the synthesis path (brainfm_amd/csrc/synth_interp.hip and the
small kernels of csrc/prep.hip), shared by tests/test_gpu_synth_kernels.py (the kernels through the C ABI, on the device),
tests/test_host_synth_kernel_refs.py (routes, oracle pinning, mutants; no device) and
tests/golden/make_golden_synth_edges.py (the reference's own functions on the same inputs).

Interpolation, zoom, label synthesis and one-hot use the functions of oracle/synth_ref.py; where the oracle has no function,
or one that does not take the edge inputs (labels outside the table, a mask with NaN), a NumPy restatement in the kernel's
operation order stands here.  Every input is a pure function of a seed (np.random.RandomState), so the three users see the
same arrays and the golden file holds results only.  NumPy only: nothing here needs torch or a device."""
import math

import numpy as np

from oracle import synth_ref as S

F32 = np.float32
NAN = F32(np.nan)
INT_MIN = -2 ** 31


def _rs(seed):
    return np.random.RandomState(seed)


def bits_equal(a, b, nan_class=False):
    """Bit equality of two 4-byte arrays (so -0.0 != +0.0 and NaN payloads count).  nan_class: a NaN equals any NaN -- for
    results in which a NaN is *computed* (0 * Inf), whose sign differs between x86 and the GPU; everything else by bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != 4 or b.dtype.itemsize != 4:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    if not nan_class:
        return bool(np.array_equal(ua, ub))
    na, nb = np.isnan(a.view(F32)), np.isnan(b.view(F32))
    return bool(np.array_equal(na, nb) and np.array_equal(ua[~na], ub[~nb]))


def n_diff(a, b, nan_class=False):
    """Number of elements that differ in the sense of bits_equal (what a test prints)."""
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    d = ua != ub
    if nan_class:
        d &= ~(np.isnan(ua.view(F32)) & np.isnan(ub.view(F32)))
    return int(d.sum())


# ------------------------------------------------------------------------------------------ bfm_interp3d_linear
# (shape, spiked): spiked volumes hold +Inf at z = 0 of every second row.  A sample exactly at z = nz-1 has weight 0 on its
# upper z corner; the reference clamps that corner to the row's last voxel, and a kernel that took it from the next address
# (the start of the next row) would turn the sample into 0 * Inf = NaN.  With finite voxels such a read is invisible.
INTERP_VOLUMES = [((5, 4, 6), False), ((5, 4, 6, 3), False), ((3, 2, 2, 4), False), ((4, 3, 2), False), ((7, 1, 5), False),
                  ((5, 4, 6), True), ((4, 3, 2), True)]
INTERP_DEFAULTS = (0.0, -7.5)
INTERP_BIG_N = 8192 * 256 + 37          # more than the 8192 blocks x 256 threads of one lap of the grid-stride loop


def interp_volume(shape, spiked=False):
    X = (_rs(100 + sum(shape) + len(shape)).randn(*shape) * 3 + 1).astype(F32)
    if spiked:
        rows = X.reshape(-1, shape[2])
        rows[1::2, 0] = np.inf
    return X


def lattice_points(shape):
    """(a) every lattice point: integer coordinates, every point with a coordinate equal to 0 or n-1, the last voxel."""
    g = np.meshgrid(*[np.arange(n, dtype=F32) for n in shape[:3]], indexing="ij")
    return tuple(v.ravel().copy() for v in g)


def hand_points(shape):
    """(b) the hand list."""
    nx, ny, nz = shape[:3]
    p = [(nx - 1, ny - 1, nz - 1), (0, 1, 1), (1e-30, 1, 1), (nx - 1, 1, 1), (nx - 1 + 1e-3, 1, 1), (np.nan, 1, 1),
         (1, np.inf, 1), (-1, 1, 1), (0.5, ny - 1, 0.25), (3.999, 2.5, 4.9999995)]
    p = np.array(p, dtype=np.float64).astype(F32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def random_points(shape, n, seed=7):
    """(c) uniform in [-1, n] per axis."""
    rs = _rs(seed)
    return tuple((rs.rand(n) * (s + 1) - 1).astype(F32) for s in shape[:3])


def interp3d_linear_variant(X, II, JJ, KK, default_value=0.0, lower_inclusive=False, upper_strict=False,
                            z_unclamped=False, pair_next_row=False):
    """fast_3D_interp_torch 'linear' for C = 1 over the volume's flat memory, with the named mistakes as switches (all off:
    the oracle's bits, which tests/test_host_synth_kernel_refs.py asserts).  z_unclamped: the upper z corner is fz + 1 even
    at fz = nz-1, read by an ordinary load (the next row; past the volume the NaN guard of the tests).  pair_next_row: the
    pair load's second dword used unconditionally (the next row; past the volume the 0 a range-checked buffer load gives)."""
    X = np.asarray(X, F32)
    nx, ny, nz = X.shape
    II, JJ, KK = (np.asarray(a, F32) for a in (II, JJ, KK))
    lo = (lambda a: a >= 0) if lower_inclusive else (lambda a: a > 0)
    hi = (lambda a, n: a < n - 1) if upper_strict else (lambda a, n: a <= n - 1)
    ok = lo(II) & lo(JJ) & lo(KK) & hi(II, nx) & hi(JJ, ny) & hi(KK, nz)
    x, y, z = II[ok], JJ[ok], KK[ok]
    fx, fy, fz = (np.floor(a).astype(np.int64) for a in (x, y, z))
    cx, cy = np.minimum(fx + 1, nx - 1), np.minimum(fy + 1, ny - 1)
    wcx, wcy, wcz = x - fx.astype(F32), y - fy.astype(F32), z - fz.astype(F32)
    wfx, wfy, wfz = F32(1) - wcx, F32(1) - wcy, F32(1) - wcz
    flat = np.concatenate([X.ravel(), [NAN if z_unclamped else F32(0)]]).astype(F32)
    dz = np.ones_like(fz) if (z_unclamped or pair_next_row) else np.minimum(fz + 1, nz - 1) - fz

    def at(a, b, up):
        return flat[(a * ny + b) * nz + fz + (dz if up else 0)]
    with np.errstate(invalid="ignore"):
        c00 = at(fx, fy, 0) * wfx + at(cx, fy, 0) * wcx
        c01 = at(fx, fy, 1) * wfx + at(cx, fy, 1) * wcx
        c10 = at(fx, cy, 0) * wfx + at(cx, cy, 0) * wcx
        c11 = at(fx, cy, 1) * wfx + at(cx, cy, 1) * wcx
        c0 = c00 * wfy + c10 * wcy
        c1 = c01 * wfy + c11 * wcy
        c = c0 * wfz + c1 * wcz
    Y = np.full(II.shape, F32(default_value), dtype=F32)
    Y[ok] = c
    return Y


def interp_linear_ref(X, II, JJ, KK, default_value):
    with np.errstate(invalid="ignore"):
        return S.interp3d_linear(X, II, JJ, KK, default_value)


# ------------------------------------------------------------------------------------------ bfm_interp3d_nearest
NEAREST_SHAPE = (5, 4, 6)
# |coordinate| stays below 2^31: the kernel converts rintf(x) to int32, the reference to int64, and a float at or beyond
# 2^31 has no int32 value (the conversion saturates on the device and is undefined in C), so the two may only be compared
# below it.  2e9 is as far outside as that allows.
NEAREST_FAR = 2.0e9


def nearest_points(shape=NEAREST_SHAPE):
    """Per axis: the ties -0.5, 0.5, 1.5, 2.5 and n-0.5 (half to even), an interior value, far outside on both sides; the
    full product over the three axes."""
    ax = [np.array([-0.5, 0.5, 1.5, 2.5, n - 0.5, 1.2, n - 1.4, -NEAREST_FAR, NEAREST_FAR, -3.2, n + 7.7], F32) for n in shape]
    g = np.meshgrid(*ax, indexing="ij")
    return tuple(v.ravel().copy() for v in g)


def nearest_volume(kind, C):
    """'int32': labels with negatives and INT_MIN; 'bits': fp32 patterns with NaN payloads, -0.0, Inf, a denormal."""
    shape = NEAREST_SHAPE + ((C,) if C > 1 else ())
    rs = _rs(300 + C)
    if kind == "int32":
        X = rs.randint(-50, 2000, size=shape).astype(np.int32)
        X.ravel()[::7] = INT_MIN
        X.ravel()[3::11] = -1
        return X
    X = rs.randn(*shape).astype(F32).view(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0xFFFFFFFF], np.uint32)
    X.ravel()[::5] = special[np.arange(X.ravel()[::5].size) % special.size]
    return X


def nearest_variant(X, II, JJ, KK, half_away=False):
    """The oracle's nearest with round-half-away as a switch."""
    if not half_away:
        return S.interp3d_nearest(X, II, JJ, KK)
    squeeze = X.ndim == 3
    Xc = X[..., None] if squeeze else X
    r = []
    for a, n in zip((II, JJ, KK), Xc.shape[:3]):
        a = np.asarray(a, np.float64)
        r.append(np.clip((np.sign(a) * np.floor(np.abs(a) + 0.5)).astype(np.int64), 0, n - 1))
    Y = Xc[r[0], r[1], r[2]]
    return Y[..., 0] if squeeze else Y


# ------------------------------------------------------------------------------------------ bfm_deformed_atlas[_tile]
ATLAS_SHAPE = (6, 5, 7)
FIELD_SHAPE = (4, 3, 5)
ATLAS_MASK_CYCLE = np.array([0.0, 1.0, 0.5, -1.0, np.nan, -0.0], F32)
ATLAS_CASES = ["inside", "last_texel", "partly_outside"]


def atlas_case(name):
    """(mask, rx, ry, rz, atlas, A[3][4]) -- mask values cycle through {0, 1, 0.5, -1, NaN, -0.0}."""
    rs = _rs(400)
    n = int(np.prod(FIELD_SHAPE))
    mask = ATLAS_MASK_CYCLE[np.arange(n) % 6].reshape(FIELD_SHAPE).copy()
    atlas = (rs.rand(*ATLAS_SHAPE) * 5 + 0.5).astype(F32)
    reg = [(rs.randn(*FIELD_SHAPE) * 0.012).astype(F32) for _ in range(3)]
    nx, ny, nz = ATLAS_SHAPE
    if name == "inside":
        A = np.array([[0.9, 0.05, 0.0, 2.5], [0.0, 1.1, -0.05, 2.0], [0.02, 0.0, 1.0, 3.0]], F32)
    elif name == "last_texel":                # reg = 0 and the translation (nx-1, ny-1, nz-1): every kept voxel samples the
        reg = [np.zeros(FIELD_SHAPE, F32) for _ in range(3)]                       # last texel, all corners clamped
        A = np.array([[1, 0, 0, nx - 1], [0, 1, 0, ny - 1], [0, 0, 1, nz - 1]], F32)
    else:                                     # the cloud's centre on the far corner: about half the samples fall outside
        A = np.array([[1.5, 0, 0, nx - 1.2], [0, 1.5, 0, ny - 1.3], [0, 0, 1.5, nz - 1.1]], F32)
    return mask, reg[0], reg[1], reg[2], atlas, A


def atlas_lap_case():
    """n = INTERP_BIG_N voxels (a second lap of the 8192 blocks) scattered over and around the atlas."""
    rs = _rs(401)
    n = INTERP_BIG_N
    mask = ATLAS_MASK_CYCLE[rs.randint(0, 6, size=n)]
    atlas = (rs.rand(*ATLAS_SHAPE) * 5 + 0.5).astype(F32)
    reg = [((rs.rand(n) * (s + 1) - 1) / 100).astype(F32) for s in ATLAS_SHAPE]
    A = np.array([[1, 0.01, 0, 0.1], [0, 1, -0.01, 0.05], [0.01, 0, 1, -0.1]], F32)
    return mask, reg[0], reg[1], reg[2], atlas, A


def atlas_ref(mask, rx, ry, rz, atlas, A, tile=False):
    """The oracle's get_deformed_atlas; the tile form is the same fed M = (im != 0) (1 where the image is negative or NaN)."""
    A4 = np.concatenate([np.asarray(A, F32), np.array([[0, 0, 0, 1]], F32)])
    with np.errstate(invalid="ignore"):
        m = (mask != 0).astype(F32) if tile else mask
        return S.deformed_atlas(m, rx, ry, rz, atlas, A4)


# ------------------------------------------------------------------------------------------ bfm_zoom_linear
ZOOM_SMALL, ZOOM_ROWS_VEC, ZOOM_ROWS_SCALAR, ZOOM_LONG = 0, 1, 2, 3
ZOOM_ROUTE_NAMES = {0: "zoom_linear_small", 1: "zoom_linear (16-byte stores)", 2: "zoom_linear (scalar stores)",
                    3: "zoom_linear_long"}
# (name, source shape, factors, route with a 16-byte aligned output)
ZOOM_CASES = [
    ("small_5x4", (5, 5, 5), (4, 4, 4), ZOOM_SMALL),
    ("small_2048_sources", (8, 16, 16), (0.5, 0.25, 0.5), ZOOM_SMALL),                 # -> (4, 4, 8)
    ("rows_2176_sources", (8, 16, 17), (0.5, 0.25, 0.5), ZOOM_ROWS_VEC),
    ("small_tables_1024", (2, 2, 2), (1, 1, 510), ZOOM_SMALL),                         # -> (2, 2, 1020)
    ("rows_tables_1028", (2, 2, 2), (1, 1, 512), ZOOM_ROWS_VEC),                       # -> (2, 2, 1024)
    ("rows_scalar_oz21", (5, 5, 5), (4, 4, 4.2), ZOOM_ROWS_SCALAR),
    ("rows_scalar_c3", (4, 3, 7, 3), (2.5, 1, 1), ZOOM_ROWS_SCALAR),
    ("rows_vec_c3", (3, 2, 8, 3), (2, 1.5, 1), ZOOM_ROWS_VEC),
    ("rows_lds_48k", (2, 2, 1024), (1, 1, 2), ZOOM_ROWS_VEC),                          # nz*C = 1024 and oz*C = 2048
    ("long_oz2100", (2, 3, 5), (1.5, 1, 420), ZOOM_LONG),
    ("long_nz1030", (2, 2, 1030), (1, 1.5, 0.5), ZOOM_LONG),
    ("long_c3", (3, 2, 350, 3), (1, 2, 1), ZOOM_LONG),
    ("down", (6, 5, 9), (0.5, 0.4, 0.7), ZOOM_ROWS_SCALAR),
    ("unit_axis", (4, 1, 5), (2, 1, 1.4), ZOOM_ROWS_SCALAR),
]
# the second lap of the two grid-stride forms (zoom_linear laps twice at any size): more than 1024 x 256 groups of four outputs
# in the LDS-resident form, more than 8192 x 4 output rows in the long form (oz = 4: the outputs stay few)
ZOOM_LAP_CASES = [
    ("small_second_lap", (5, 5, 5), (20.4, 20.4, 20.8), ZOOM_SMALL),                   # -> (102, 102, 104): 1 082 016 outputs
    ("long_second_lap", (2, 2, 1030), (91, 91, 0.004), ZOOM_LONG),                     # -> (182, 182, 4): 33 124 rows
]
# the output pointer one float off its alignment: a rows case and a would-be-small case, both on scalar stores
ZOOM_MISALIGNED = [("rows_2176_sources", ZOOM_ROWS_SCALAR), ("small_5x4", ZOOM_ROWS_SCALAR)]


def zoom_case(name):
    for i, (nm, shape, factor, route) in enumerate(ZOOM_CASES + ZOOM_LAP_CASES):
        if nm == name:
            return (_rs(500 + i).randn(*shape) * 2).astype(F32), np.array(factor, np.float64), route
    raise KeyError(name)


def zoom_out_shape(shape, factor):
    return tuple(int(np.round(n * f)) for n, f in zip(shape[:3], factor))


# ------------------------------------------------------------------------------------------ bfm_conv1d_axis
C1D_FALLBACK = 3
# (name, volume, axis, klen, sigma of the Gaussian with that many taps, route); taps: "gauss" and "random" for every entry
CONV1D_CASES = [
    ("k_longer_than_x", (5, 70, 3), 0, 13, 2.0, 0),
    ("nz_below_64_y", (5, 70, 3), 1, 5, 0.6, 1),
    ("k_longer_than_z", (5, 70, 3), 2, 25, 4.0, 2),
    ("z_tail_lane_x", (9, 4, 65), 0, 9, 1.3, 0),
    ("z_tail_lane_y", (9, 4, 65), 1, 9, 1.3, 1),
    ("z_tail_lane_z", (9, 4, 65), 2, 9, 1.3, 2),
    ("long_segment", (200, 6, 896), 0, 11, 1.6, 0),
    ("partial_last_slab", (3, 3, 1024), 2, 9, 1.3, 2),
    ("nz_1025", (3, 3, 1025), 2, 9, 1.3, C1D_FALLBACK),
    ("k63_x", (12, 10, 70), 0, 63, 10.3, 0),
    ("k63_y", (12, 10, 70), 1, 63, 10.3, 1),
    ("k63_z", (12, 10, 70), 2, 63, 10.3, 2),
    ("k67_x", (12, 10, 70), 0, 67, 11.0, C1D_FALLBACK),
    ("k67_y", (12, 10, 70), 1, 67, 11.0, C1D_FALLBACK),
    ("k67_z", (12, 10, 70), 2, 67, 11.0, C1D_FALLBACK),
    ("fallback_second_lap", (182, 182, 3), 1, 67, 11.0, C1D_FALLBACK),                # 33 124 rows: more than 8192 blocks x 4 waves
]
C1D_U = 2.0 ** -24
# the Gaussian cases whose result by the reference's own gaussian_blur_3d is in the golden file (the others are too large)
CONV1D_GOLDEN = ["k_longer_than_x", "nz_below_64_y", "k_longer_than_z", "z_tail_lane_x", "z_tail_lane_y", "z_tail_lane_z",
                 "k63_x", "k67_z"]


def conv1d_case(name, taps):
    """(x, taps, axis, sigma, route): 'gauss' taps are the oracle's make_gaussian_kernel(sigma), 'random' are asymmetric."""
    for i, (nm, shape, axis, klen, sigma, route) in enumerate(CONV1D_CASES):
        if nm == name:
            rs = _rs(600 + i)
            x = (rs.randn(*shape) + 0.3).astype(F32)
            if taps == "gauss":
                k = S.make_gaussian_kernel(sigma)
                assert len(k) == klen, (name, len(k), klen)
            else:
                k = (rs.randn(klen) * np.linspace(0.2, 1.5, klen)).astype(F32)
            return x, k, axis, sigma, route
    raise KeyError(name)


def correlate1d_ref(x, k, axis, reverse=False):
    """Zero-padded 1-D correlation along `axis` in float64: (out, sum_j |k_j| |x_j|) per output.  reverse: the taps flipped
    (convolution instead of correlation), the mistake a symmetric Gaussian cannot show."""
    x = np.asarray(x, np.float64)
    k = np.asarray(k, np.float64)
    if reverse:
        k = k[::-1]
    half = len(k) // 2
    pad = [(0, 0)] * 3
    pad[axis] = (half, half)
    P = np.pad(x, pad)
    out, mag = np.zeros(x.shape), np.zeros(x.shape)
    for j in range(len(k)):
        sl = [slice(None)] * 3
        sl[axis] = slice(j, j + x.shape[axis])
        out += k[j] * P[tuple(sl)]
        mag += abs(k[j]) * np.abs(P[tuple(sl)])
    return out, mag


def conv1d_bound(klen, mag):
    """|out - ref64| <= (klen + 1) * 2^-24 * sum_j |k_j| |x_j|: the kernel is an fp32 fmaf chain in tap order, whose
    worst-case error is klen roundings of 2^-24 relative to the sum of magnitudes; one more for the reference's rounding."""
    return (klen + 1) * C1D_U * mag


def conv1d_ratio(out, ref, mag, klen):
    """max over the outputs of |out - ref| / bound (<= 1 passes); 0 / 0 counts as 0."""
    err = np.abs(np.asarray(out, np.float64) - ref)
    b = conv1d_bound(klen, mag)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())


def blur_stds(axis, sigma):
    s = [0.0, 0.0, 0.0]
    s[axis] = sigma
    return s


# ------------------------------------------------------------------------------------------ bfm_deform_grid
DEFORM_SHP = (40, 36, 44)
# (name, size, with F, kind of affine)
DEFORM_CASES = [
    ("below_a_wave", (5, 3, 2), False, "general"), ("below_a_wave_F", (5, 3, 2), True, "general"),
    ("golden_size", (24, 20, 28), False, "general"), ("golden_size_F", (24, 20, 28), True, "general"),
    ("second_lap", (70, 64, 64), False, "general"), ("second_lap_F", (70, 64, 64), True, "general"),
    ("all_below", (24, 20, 28), True, "below"), ("all_above", (5, 3, 2), False, "above"),
]


def deform_case(name):
    """(size, shp, A[3][3], c2[3], F or None)."""
    for i, (nm, size, withF, kind) in enumerate(DEFORM_CASES):
        if nm == name:
            rs = _rs(700 + i)
            A = (np.eye(3) * [1.1, 0.9, 1.05] + rs.randn(3, 3) * 0.08).astype(F32)
            c2 = ((np.array(DEFORM_SHP) - 1) / 2).astype(F32)
            if kind == "below":
                c2 = c2 - F32(1000)
            elif kind == "above":
                c2 = c2 + F32(1000)
            F = (rs.randn(*size, 3) * 2).astype(F32) if withF else None
            return size, DEFORM_SHP, A, c2, F
    raise KeyError(name)


def deform_grid_raw(size, shp, A, c2, F=None):
    """The kernel's values: clamped source coordinates BEFORE the box offset is subtracted, and their six extrema
    [min x, min y, min z, max x, max y, max z].  fp32, ((a0*x1 + a1*y1) + a2*z1) + c, no contraction."""
    A, c2 = np.asarray(A, F32), np.asarray(c2, F32)
    g = np.meshgrid(*[np.arange(n, dtype=F32) for n in size], indexing="ij")
    c = [F32((n - 1) / 2.0) for n in size]
    p = [g[a] - c[a] for a in range(3)]
    if F is not None:
        p = [p[a] + np.asarray(F, F32)[..., a] for a in range(3)]
    out = []
    for r in range(3):
        v = ((A[r, 0] * p[0] + A[r, 1] * p[1]) + A[r, 2] * p[2]) + c2[r]
        v = np.where(v < 0, F32(0), v)
        v = np.where(v > F32(shp[r] - 1), F32(shp[r] - 1), v).astype(F32)
        out.append(v)
    mm = np.array([v.min() for v in out] + [v.max() for v in out], F32)
    return out[0], out[1], out[2], mm


# ------------------------------------------------------------------------------------------ label kernels
NTAB = 256
LABEL_EDGES = np.array([0, 2, 41, 77, 2.5, 3.5, NTAB - 1, 300, -3], F32)      # 77 -> 2; 2.5 -> 2, 3.5 -> 4; 300, -3: clamped
LABEL_SIZES = [1, 63, 257]
CLASS_STATS_BIG = 256 * 1024 + 5                                              # past the 1024 blocks x 256 threads of one lap


def label_case(n, in_range=False):
    """(G, mus, sigmas, randn, syn): G starts with the edge labels (all of them when n allows), then random ones."""
    rs = _rs(800 + n)
    edges = LABEL_EDGES[:7] if in_range else LABEL_EDGES
    G = rs.randint(0, NTAB, size=n).astype(F32)
    G[rs.rand(n) < 0.3] = 0
    G[rs.rand(n) < 0.2] = rs.choice([2, 41, 77])
    m = min(n, len(edges))
    G[:m] = edges[:m] if n > 1 else edges[3:4]
    mus = (rs.rand(NTAB) * 200).astype(F32)
    sigmas = (rs.rand(NTAB) * 150).astype(F32)                                 # wide enough for negative draws: the clamp at 0
    rn = rs.randn(n).astype(F32)
    syn = (rs.rand(n) * 100 + 0.1).astype(F32)
    return G, mus, sigmas, rn, syn


def _label_index(G):
    G = np.asarray(G, F32).copy()
    G[G == 77] = 2
    return np.rint(G).astype(np.int64)


def label_gauss_ref(G, mus, sigmas, rn, ntab=NTAB):
    """mus[l] + sigmas[l] * randn clamped at 0, l = rint(G with 77 -> 2) clamped to the table.  In range it is the oracle's
    synth_from_labels (used as it is); outside the oracle has no answer and the clamp is restated."""
    l = _label_index(G)
    if l.min() >= 0 and l.max() < ntab:
        return S.synth_from_labels(G, mus, sigmas, rn)
    l = np.clip(l, 0, ntab - 1)
    v = (np.asarray(mus, F32)[l] + np.asarray(sigmas, F32)[l] * np.asarray(rn, F32)).astype(F32)
    v[v < 0] = 0
    return v


def label_class_stats_ref(G, syn):
    """(cerebral, [sum, count] of labels 2 / 41, [sum, count] of every other non-zero label, sum of |v| per class);
    sums by math.fsum (exact, rounded once).  The label is NOT clamped here: -3 and 300 are 'other'."""
    l = _label_index(G)
    syn = np.asarray(syn, F32)
    cerebral = np.where(l == 0, F32(0), syn).astype(F32)
    a = (l == 2) | (l == 41)
    b = ~a & (l != 0)
    v = syn.astype(np.float64)
    stats = [math.fsum(v[a]), float(a.sum()), math.fsum(v[b]), float(b.sum())]
    mags = [math.fsum(np.abs(v[a])), math.fsum(np.abs(v[b]))]
    return cerebral, stats, mags


NLUT = 64
ONEHOT_CASES = [(1, 63), (56, 257), (57, 63)]                                  # (n_labels, n)
ONEHOT_LAP = (57, 36800)                                                       # n * n_labels > 8192 x 256: a second lap
LABEL_LAP = INTERP_BIG_N


def onehot_case(n_labels, n, in_range=False):
    """(S int32, lut int32[NLUT]): S below 0 and at or above nlut, LUT entries outside [0, n_labels)."""
    rs = _rs(900 + n_labels)
    lut = rs.randint(0, n_labels, size=NLUT).astype(np.int32)
    Sv = rs.randint(0, NLUT, size=n).astype(np.int32)
    if not in_range:
        lut[5], lut[9], lut[NLUT - 1], lut[0] = -1, n_labels, n_labels + 3, n_labels - 1
        Sv[:8] = [-1, INT_MIN, NLUT, NLUT + 100, 2 ** 31 - 1, 5, 9, 0]
    return Sv, lut


def onehot_ref(Sv, lut, n_labels):
    """In range the oracle's onehot_lut; otherwise S clamped to the table and a LUT entry outside [0, n_labels) -> no 1."""
    Sv, lut = np.asarray(Sv), np.asarray(lut)
    if Sv.min() >= 0 and Sv.max() < len(lut) and lut.min() >= 0 and lut.max() < n_labels:
        return S.onehot_lut(Sv, lut, n_labels)
    idx = lut[np.clip(Sv.astype(np.int64), 0, len(lut) - 1)]
    return (idx[..., None] == np.arange(n_labels)).astype(F32)


# ------------------------------------------------------------------------------------------ csrc/prep.hip
PERMUTE_SHAPE = (3, 5, 7)
PERMUTE_LAP = ((101, 103, 105), (2, 0, 1), (1, 0, 1))     # 1 092 315 voxels: past one lap of 4096 blocks x 256 threads


def permute_flip_ref(x, perm, flip, inverse=False):
    """out[i] = in[j], j[perm[a]] = flip[a] ? n_out[a]-1-i[a] : i[a]  ==  transpose by perm, then flip the flagged OUTPUT
    axes.  inverse: the transpose taken with the inverse permutation (the classic mistake)."""
    p = np.argsort(perm) if inverse else perm
    y = np.transpose(x, p)
    axes = tuple(a for a in range(3) if flip[a])
    return np.ascontiguousarray(np.flip(y, axes) if axes else y)


INT_MAX = 2 ** 31 - 1
BBOX_EMPTY = [INT_MAX] * 3 + [0] * 3
BBOX_CASES = ["nothing_above_tol", "first_voxel", "last_voxel", "nan_voxels", "negative_tol", "above_512_blocks"]


def bbox_case(name):
    """(volume, tol)."""
    rs = _rs(1000)
    shape = (6, 5, 9)
    if name == "nothing_above_tol":
        return (rs.rand(*shape) * 0.5).astype(F32), 0.5
    x = np.zeros(shape, F32)
    if name == "first_voxel":
        x[0, 0, 0] = 1
        return x, 0.0
    if name == "last_voxel":
        x[-1, -1, -1] = 1
        return x, 0.0
    if name == "nan_voxels":                   # NaN > tol is false: the NaN voxels lie outside the box of the two real ones
        x[0, :, :] = np.nan
        x[-1, -1, -1] = np.nan
        x[2, 1, 3] = 2
        x[4, 3, 5] = 0.1
        return x, 0.0
    if name == "negative_tol":                 # zeros count, -2 does not
        x[:] = -2
        x[1:4, 2:3, 4:8] = 0
        return x, -1.0
    x = np.zeros((64, 48, 50), F32)            # 153 600 voxels: more than 512 blocks x 256 threads
    x[5:60:7, 3:44:5, 2:49:3] = 1
    x[61, 45, 1] = 1e-3
    return x, 1e-4


def bbox_ref(x, tol):
    with np.errstate(invalid="ignore"):
        idx = np.argwhere(x > F32(tol))
    if len(idx) == 0:
        return list(BBOX_EMPTY)
    return [int(v) for v in idx.min(0)] + [int(v) + 1 for v in idx.max(0)]


MEAN_C = [1, 2, 3, 7]
MEAN_N = [1, 255]
MEAN_BIG = 4096 * 256 + 3                      # past one lap of 4096 blocks x 256 threads


def mean_case(n, c):
    return (_rs(1100 + c).randn(n, c) * 10 + 3).astype(F32)


def mean_lastdim_ref(x):
    """Sequential fp32 sum over the last axis (starting from 0), divided by float(c)."""
    x = np.asarray(x, F32)
    s = np.zeros(x.shape[0], F32)
    for j in range(x.shape[1]):
        s = s + x[:, j]
    return (s / F32(x.shape[1])).astype(F32)
