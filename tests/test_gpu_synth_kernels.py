"""Every gather / resample kernel of the synthesis path on its own, through the C ABI, route by route, against the references
of tests/synth_kernel_refs.py: the eleven entry points of brainfm_amd/csrc/synth_interp.hip (bfm_interp3d_linear / nearest,
bfm_deformed_atlas / _tile, bfm_zoom_linear, bfm_conv1d_axis, bfm_deform_grid, bfm_label_gauss, bfm_label_class_stats,
bfm_onehot_lut) and the three small kernels of csrc/prep.hip (bfm_permute_flip3d, bfm_bbox_nonzero, bfm_mean_lastdim).
tests/test_gpu_synth.py sees them at one golden shape each with uniformly random coordinates; here are the shapes, routes
and coordinates at which such kernels go wrong.  tests/test_host_synth_kernel_refs.py pins the references to the reference
implementation's own results and shows that each named mistake changes them on these cases.

Conventions (those of tests/test_gpu_conv_forward.py): outputs start as 0xFFFFFFFF (a NaN when read as fp32) between a
64-word front guard and a 4096-word sentinel tail that must both come back untouched; every input sits between NaN guard
bands inside a larger allocation, so a read one element outside an operand shows up in the result and cannot fault.  All
comparisons are bit for bit on uint32 views unless a bound is stated (where the reference itself computes a NaN, as 0 * Inf
in the spiked volumes, any NaN equals any NaN: the sign of a computed NaN differs between x86 and the GPU).  The route of
bfm_zoom_linear and bfm_conv1d_axis is asked of the library (bfm_zoom_linear_route, bfm_conv1d_axis_plan) and asserted.
Each case prints one line: kernel, route, measured difference.

Left out: the C = 1 general-kernel route of bfm_interp3d_linear, taken only for volumes of 4 GiB and more (the pair-load
kernel's byte offsets are 32-bit); it is the C > 1 kernel, which the C = 3 and C = 4 volumes run.

bfm_conv1d_axis, measured on MI355X (also in HISTORY.md section 1): worst |out - ref64| / ((klen + 1) 2^-24 sum |k||x|)
over the cases of a route, Gaussian and random taps (the bar is 1), and the worst distance of a Gaussian case to
oracle.gaussian_blur_3d, of max |out|:
    route 0  conv1d_slab<0>   0.320 (long_segment, gauss)       2.0e-7
    route 1  conv1d_slab<1>   0.362 (nz_below_64_y, gauss)      1.2e-7
    route 2  conv1d_slab<2>   0.336 (partial_last_slab, gauss)  2.9e-7
    route 3  conv1d_axis      0.348 (nz_1025, gauss)            4.1e-7 (fallback_second_lap, 67 taps)
The ratio falls with klen (0.04 - 0.07 at 63 and 67 taps): the bound is the worst case of a chain, the error a random walk.
Everything else in this module measured 0 differing elements.
Needs an MI355X: run with `-m gpu`."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import synth_ref as S
import synth_kernel_refs as K

pytestmark = pytest.mark.gpu

GUARD = 64                       # words; 256 bytes, so an operand keeps the allocation's 16-byte alignment
TAIL = 4096
NAN_BITS = 0x7FC00000
UNWRITTEN = -1                   # 0xFFFFFFFF
SENT = -7777
E_ARG = -1


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _in(a, offset=0):
    """A device copy of a 4-byte array between NaN guard bands, `offset` words off the 16-byte alignment."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    n = a.size
    flat = torch.full((GUARD + offset + n + GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())
    v = flat[GUARD + offset:GUARD + offset + n]
    v.copy_(torch.from_numpy(a.reshape(-1).view(np.int32)))
    assert v.data_ptr() % 16 == 4 * (offset % 4)
    return v


class _Out:
    """n unwritten 4-byte words, `offset` words off alignment, a guard in front and a sentinel tail behind."""

    def __init__(self, n, offset=0):
        self.n, self.lo = n, GUARD + offset
        self.flat = torch.full((self.lo + n + TAIL,), SENT, dtype=torch.int32, device=_dev())
        self.view = self.flat[self.lo:self.lo + n]
        self.view.fill_(UNWRITTEN)
        assert self.view.data_ptr() % 16 == 4 * (offset % 4)

    def get(self, label, dtype=np.float32, shape=None):
        torch.cuda.synchronize()
        h = self.flat.cpu().numpy()
        assert (h[:self.lo] == SENT).all(), label + ": wrote in front of the output"
        assert (h[self.lo + self.n:] == SENT).all(), label + ": wrote behind the output"
        out = h[self.lo:self.lo + self.n].view(dtype)
        return out.reshape(shape) if shape is not None else out


def _same(label, route, got, ref, nan_class=False):
    bad = K.n_diff(got, ref, nan_class) if got.shape == ref.shape else -1
    print("%s [%s]: %d of %d elements differ" % (label, route, bad, ref.size))
    assert got.shape == ref.shape and K.bits_equal(got, ref, nan_class), (label, bad)


# ------------------------------------------------------------------------------------------ bfm_interp3d_linear
def _interp_linear(X, pts, dv, offset=0):
    L, lib = _lib()
    shape = X.shape
    Cc = shape[3] if X.ndim == 4 else 1
    n = pts[0].size
    dX, dI, dJ, dK = _in(X, offset), _in(pts[0]), _in(pts[1]), _in(pts[2])
    out = _Out(n * Cc)
    rc = lib.bfm_interp3d_linear(L.ptr(dX), shape[0], shape[1], shape[2], Cc, L.ptr(dI), L.ptr(dJ), L.ptr(dK), n, dv,
                                 L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    return out.get("interp3d_linear", shape=(n, Cc) if Cc > 1 else (n,))


@pytest.mark.parametrize("vi", range(len(K.INTERP_VOLUMES)))
def test_interp3d_linear_lattice_and_hand_points(vi):
    """(a) every lattice point -- integer coordinates, every coordinate equal to 0 (excluded) or n-1 (included), the last
    voxel, where the pair load's second dword lies past the volume -- and (b) the hand list, with defaults 0 and -7.5.
    nz = 2: every pair load sits at a row end; ny = 1: everything is the default; the spiked volumes make a second dword
    taken from the next row visible."""
    shape, spiked = K.INTERP_VOLUMES[vi]
    X = K.interp_volume(shape, spiked)
    route = "interp_linear1 pair loads" if len(shape) == 3 else "interp_linear C=%d" % shape[3]
    for pname, pts in (("lattice", K.lattice_points(shape)), ("hand", K.hand_points(shape))):
        for dv in K.INTERP_DEFAULTS:
            got = _interp_linear(X, pts, dv)
            _same("interp3d_linear %s%s %s default %g" % (shape, " spiked" if spiked else "", pname, dv), route, got,
                  K.interp_linear_ref(X, *pts, dv), nan_class=spiked)


def test_interp3d_linear_second_lap_of_the_grid_stride_loop():
    shape = (5, 4, 6)
    X = K.interp_volume(shape)
    pts = K.random_points(shape, K.INTERP_BIG_N)
    got = _interp_linear(X, pts, -7.5)
    _same("interp3d_linear %s random n=%d" % (shape, K.INTERP_BIG_N), "interp_linear1 pair loads", got,
          K.interp_linear_ref(X, *pts, -7.5))


def test_interp3d_linear_volume_base_not_8_byte_aligned():
    """The 8-byte pair loads over a volume whose base is 4-byte but not 8-byte aligned (a view one float into the guarded
    allocation, so everything stays in bounds)."""
    for shape, spiked in (((5, 4, 6), False), ((4, 3, 2), True)):
        X = K.interp_volume(shape, spiked)
        for pts in (K.lattice_points(shape), K.hand_points(shape)):
            got = _interp_linear(X, pts, -7.5, offset=1)
            _same("interp3d_linear %s base + 4 bytes" % (shape,), "interp_linear1 pair loads", got,
                  K.interp_linear_ref(X, *pts, -7.5), nan_class=spiked)


# ------------------------------------------------------------------------------------------ bfm_interp3d_nearest
@pytest.mark.parametrize("kind,Cc", [("int32", 1), ("int32", 3), ("bits", 1), ("bits", 3)])
def test_interp3d_nearest_ties_clamps_and_bit_copies(kind, Cc):
    """Coordinates exactly at -0.5, 0.5, 1.5, 2.5 and n-0.5 (half to even) and far outside on both sides (|x| = 2e9, below
    2^31: see synth_kernel_refs.NEAREST_FAR); int32 labels with negatives and INT_MIN, fp32 bit patterns with NaN payloads
    and -0.0, copied bit for bit."""
    L, lib = _lib()
    X = K.nearest_volume(kind, Cc)
    pts = K.nearest_points()
    n = pts[0].size
    nx, ny, nz = K.NEAREST_SHAPE
    out = _Out(n * Cc)
    dX, dI, dJ, dK = _in(X), _in(pts[0]), _in(pts[1]), _in(pts[2])
    rc = lib.bfm_interp3d_nearest(L.ptr(dX), nx, ny, nz, Cc, L.ptr(dI), L.ptr(dJ), L.ptr(dK), n, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    got = out.get("interp3d_nearest", np.uint32, (n, Cc) if Cc > 1 else (n,))
    _same("interp3d_nearest %s C=%d" % (kind, Cc), "interp_nearest", got, S.interp3d_nearest(X, *pts).view(np.uint32))


def test_interp3d_nearest_second_lap_of_the_grid_stride_loop():
    L, lib = _lib()
    X = K.nearest_volume("int32", 1)
    pts = K.random_points(K.NEAREST_SHAPE, K.INTERP_BIG_N, seed=8)
    n = pts[0].size
    out = _Out(n)
    dX, dI, dJ, dK = _in(X), _in(pts[0]), _in(pts[1]), _in(pts[2])
    rc = lib.bfm_interp3d_nearest(L.ptr(dX), *K.NEAREST_SHAPE, 1, L.ptr(dI), L.ptr(dJ), L.ptr(dK), n, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    _same("interp3d_nearest int32 random n=%d" % n, "interp_nearest", out.get("interp3d_nearest", np.uint32),
          S.interp3d_nearest(X, *pts).view(np.uint32))


# ------------------------------------------------------------------------------------------ bfm_deformed_atlas[_tile]
def _atlas(case, tile, label):
    L, lib = _lib()
    mask, rx, ry, rz, atlas, A = case
    n = mask.size
    out = _Out(n)
    ops = [_in(a) for a in (mask, rx, ry, rz, atlas)]
    fn = lib.bfm_deformed_atlas_tile if tile else lib.bfm_deformed_atlas
    rc = fn(*[L.ptr(t) for t in ops], atlas.shape[0], atlas.shape[1], atlas.shape[2], (C.c_float * 12)(*A.ravel().tolist()), n,
            L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    got = out.get("deformed_atlas", shape=mask.shape)
    _same("deformed_atlas%s %s" % ("_tile" if tile else "", label), "mask != 0" if tile else "mask > 0", got,
          K.atlas_ref(mask, rx, ry, rz, atlas, A, tile=tile))


@pytest.mark.parametrize("tile", [False, True], ids=["mask_gt_0", "tile_ne_0"])
@pytest.mark.parametrize("name", K.ATLAS_CASES)
def test_deformed_atlas_mask_predicates_and_last_texel(name, tile):
    """A (4, 3, 5) field into a (6, 5, 7) atlas; mask values cycle through {0, 1, 0.5, -1, NaN, -0.0}: `> 0` keeps 1 and
    0.5, `!= 0` keeps -1 and NaN too.  last_texel: every kept voxel samples exactly (nx-1, ny-1, nz-1)."""
    _atlas(K.atlas_case(name), tile, name)


@pytest.mark.parametrize("tile", [False, True], ids=["mask_gt_0", "tile_ne_0"])
def test_deformed_atlas_second_lap_of_the_grid_stride_loop(tile):
    _atlas(K.atlas_lap_case(), tile, "n=%d" % K.INTERP_BIG_N)


# ------------------------------------------------------------------------------------------ bfm_zoom_linear
def _zoom(name, want_route, offset=0):
    from brainfm_amd.generator_utils import zoom_tables
    L, lib = _lib()
    X, factor, _ = K.zoom_case(name)
    Cc = X.shape[3] if X.ndim == 4 else 1
    nx, ny, nz = X.shape[:3]
    tabs = [zoom_tables(n, float(f)) for n, f in zip((nx, ny, nz), factor)]
    o = [len(t[0]) for t in tabs]
    assert tuple(o) == K.zoom_out_shape(X.shape, factor)
    keep = [[_in(v) for v in t] for t in tabs]
    axes = (L.ZoomAxis * 3)(*[L.ZoomAxis(*[v.data_ptr() for v in t]) for t in keep])
    out = _Out(o[0] * o[1] * o[2] * Cc, offset)
    route = lib.bfm_zoom_linear_route(nx, ny, nz, Cc, o[0], o[1], o[2], 1 if out.view.data_ptr() % 16 == 0 else 0)
    assert route == want_route, (name, route, want_route)
    dX = _in(X)
    rc = lib.bfm_zoom_linear(L.ptr(dX), nx, ny, nz, Cc, axes, o[0], o[1], o[2], L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    got = out.get("zoom_linear", shape=tuple(o) + ((Cc,) if Cc > 1 else ()))
    _same("zoom_linear %s %s -> %s%s" % (name, X.shape, tuple(o), " out + 4 bytes" if offset else ""),
          "route %d %s" % (route, K.ZOOM_ROUTE_NAMES[route]), got, S.myzoom(X, factor))


@pytest.mark.parametrize("case", K.ZOOM_CASES, ids=[c[0] for c in K.ZOOM_CASES])
def test_zoom_linear_every_route_and_threshold(case):
    """The three kernels and the two store forms, on both sides of each switching threshold: 2048 source elements,
    ox + oy + oz = 1024, nz*C = 1024 with oz*C = 2048 (48 KB of dynamic LDS), and the long form by oz, by nz and with C = 3."""
    _zoom(case[0], case[3])


@pytest.mark.parametrize("case", K.ZOOM_LAP_CASES, ids=[c[0] for c in K.ZOOM_LAP_CASES])
def test_zoom_linear_second_lap_of_the_small_and_long_forms(case):
    _zoom(case[0], case[3])


@pytest.mark.parametrize("name,route", K.ZOOM_MISALIGNED)
def test_zoom_linear_misaligned_output_takes_scalar_stores(name, route):
    _zoom(name, route, offset=1)


# ------------------------------------------------------------------------------------------ bfm_conv1d_axis
@pytest.mark.parametrize("taps", ["gauss", "random"])
@pytest.mark.parametrize("case", K.CONV1D_CASES, ids=[c[0] for c in K.CONV1D_CASES])
def test_conv1d_axis_slab_and_fallback_vs_float64(case, taps):
    """Against float64 correlation, Gaussian and random ASYMMETRIC taps (a flipped tap order passes every Gaussian).  The
    bound is derived: |out - ref64| <= (klen + 1) 2^-24 sum_j |k_j||x_j| per output (synth_kernel_refs.conv1d_bound)."""
    L, lib = _lib()
    name, shape, axis, klen, sigma, want_route = case
    x, k, axis, sigma, _ = K.conv1d_case(name, taps)
    seg, nslab, lds = C.c_int(), C.c_int(), C.c_size_t()
    route = lib.bfm_conv1d_axis_plan(shape[0], shape[1], shape[2], axis, klen, C.byref(seg), C.byref(nslab), C.byref(lds))
    assert route == want_route, (name, route)
    if name == "long_segment":
        assert seg.value > 8 and nslab.value == shape[1] * ((shape[2] + 63) // 64) * -(-shape[0] // seg.value)
    if name == "partial_last_slab":
        assert seg.value == 4 and nslab.value == 3
    out = _Out(x.size)
    dx, dk = _in(x), _in(k)
    rc = lib.bfm_conv1d_axis(L.ptr(dx), shape[0], shape[1], shape[2], axis, L.ptr(dk), klen, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    got = out.get("conv1d_axis", shape=shape)
    ref, mag = K.correlate1d_ref(x, k, axis)
    assert bool(np.isfinite(got).all()), name + ": an element was not written"
    ratio = K.conv1d_ratio(got, ref, mag, klen)
    extra = ""
    if taps == "gauss":
        orc = S.gaussian_blur_3d(x, K.blur_stds(axis, sigma))
        extra = ", vs oracle gaussian_blur_3d %.2e of max |out|" % (float(np.abs(got - orc).max()) / float(np.abs(orc).max()))
    print("conv1d_axis %s %s axis %d klen %d %s [route %d %s seg %d nslab %d lds %d]: ratio to bound %.3f%s"
          % (name, shape, axis, klen, taps, route, "fallback" if route == 3 else "slab", seg.value, nslab.value, lds.value,
             ratio, extra))
    assert ratio <= 1.0, (name, taps, ratio)


# ------------------------------------------------------------------------------------------ bfm_deform_grid
@pytest.mark.parametrize("name", [c[0] for c in K.DEFORM_CASES])
def test_deform_grid_values_and_extrema(name):
    """n = 30 (less than a wave), the golden's size, and 286 720 voxels (a second lap of the 1024 blocks), with and without
    F; an affine that sends everything below 0 / above shp-1, so that min equals max at a clamp.  xx / yy / zz bit for
    bit, the six extrema exactly."""
    L, lib = _lib()
    size, shp, A, c2, F = K.deform_case(name)
    n = int(np.prod(size))
    outs = [_Out(n) for _ in range(3)]
    mm = _Out(6)
    nws = lib.bfm_deform_grid_workspace(*size)
    ws = torch.full((nws // 4 + GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())
    dF = _in(F) if F is not None else None
    rc = lib.bfm_deform_grid(L.ptr(dF), size[0], size[1], size[2], (C.c_float * 9)(*A.ravel().tolist()),
                             (C.c_float * 3)(*c2.tolist()), (C.c_int * 3)(*shp), L.ptr(outs[0].view), L.ptr(outs[1].view),
                             L.ptr(outs[2].view), L.ptr(mm.view), L.ptr(ws), nws, L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    ref = K.deform_grid_raw(size, shp, A, c2, F)
    for o, r, nm in zip(outs, ref[:3], "xyz"):
        _same("deform_grid %s %s%s" % (name, nm * 2, " F" if F is not None else ""), "deform_grid_k", o.get("deform_grid", shape=size), r)
    got = mm.get("deform_grid minmax")
    print("deform_grid %s [minmax6_final]: %s vs %s" % (name, got.tolist(), ref[3].tolist()))
    assert got.tolist() == ref[3].tolist(), name
    assert (ws[nws // 4:] == NAN_BITS).all(), "wrote behind the workspace"


# ------------------------------------------------------------------------------------------ label kernels
@pytest.mark.parametrize("n", K.LABEL_SIZES + [K.LABEL_LAP])
def test_label_gauss_table_clamp_and_rounding(n):
    """n = 1, 63, 257 and 8192 * 256 + 37 (a second lap).  Labels 0, 2, 41, 77 (-> 2), 2.5 and 3.5 (half to even), ntab-1, 300 with ntab = 256 and -3 (clamped to the table)."""
    L, lib = _lib()
    G, mus, sg, rn, _ = K.label_case(n)
    out = _Out(n)
    ops = [_in(a) for a in (G, mus, sg, rn)]
    rc = lib.bfm_label_gauss(*[L.ptr(t) for t in ops], n, K.NTAB, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    _same("label_gauss n=%d" % n, "label_gauss", out.get("label_gauss"), K.label_gauss_ref(G, mus, sg, rn))


@pytest.mark.parametrize("n", K.LABEL_SIZES + [K.CLASS_STATS_BIG])
def test_label_class_stats_counts_sums_and_reproducibility(n):
    """Counts exact, cerebral bit for bit, sums within n 2^-53 sum |v| of math.fsum (double accumulation in a fixed order),
    two runs bit-identical."""
    L, lib = _lib()
    G, _, _, _, syn = K.label_case(n)
    dG, dsyn = _in(G), _in(syn)
    runs = []
    for _ in range(2):
        cer = _Out(n)
        stats = torch.full((4 + 16,), float("nan"), dtype=torch.float64, device=_dev())
        partials = torch.full((L.CLASS_STATS_BLOCKS * 4 + 16,), float("nan"), dtype=torch.float64, device=_dev())
        rc = lib.bfm_label_class_stats(L.ptr(dG), L.ptr(dsyn), n, L.ptr(cer.view), L.ptr(stats), L.ptr(partials), L.stream_ptr())
        assert rc == 0, L.ERR.get(rc, rc)
        c = cer.get("label_class_stats")
        assert bool(torch.isnan(stats[4:]).all()) and bool(torch.isnan(partials[L.CLASS_STATS_BLOCKS * 4:]).all())
        runs.append((c, stats[:4].cpu().numpy()))
    ref_c, ref_s, mags = K.label_class_stats_ref(G, syn)
    _same("label_class_stats n=%d cerebral" % n, "label_class_stats", runs[0][0], ref_c)
    got = runs[0][1]
    print("label_class_stats n=%d [label_class_fold]: stats %s, sum errors %.2e %.2e"
          % (n, got.tolist(), abs(got[0] - ref_s[0]), abs(got[2] - ref_s[2])))
    assert got[1] == ref_s[1] and got[3] == ref_s[3]
    assert abs(got[0] - ref_s[0]) <= n * 2.0 ** -53 * mags[0] and abs(got[2] - ref_s[2]) <= n * 2.0 ** -53 * mags[1]
    assert np.array_equal(runs[0][1].view(np.uint64), runs[1][1].view(np.uint64)) and K.bits_equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize("nl,n", K.ONEHOT_CASES + [K.ONEHOT_LAP])
def test_onehot_lut_clamps_and_entries_outside_the_labels(nl, n):
    """n_labels 1, 56, 57 (and 57 x 36 800 outputs: a second lap); S below 0 and at or above nlut (clamped); LUT entries outside [0, n_labels) (a row of zeros)."""
    L, lib = _lib()
    Sv, lut = K.onehot_case(nl, n)
    out = _Out(n * nl)
    dS, dl = _in(Sv), _in(lut)
    rc = lib.bfm_onehot_lut(L.ptr(dS), L.ptr(dl), K.NLUT, nl, n, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    _same("onehot_lut n_labels=%d n=%d" % (nl, n), "onehot_lut", out.get("onehot_lut", shape=(n, nl)), K.onehot_ref(Sv, lut, nl))


# ------------------------------------------------------------------------------------------ csrc/prep.hip
def test_permute_flip3d_all_48_and_refusal():
    L, lib = _lib()
    x = (np.random.RandomState(5).randn(*K.PERMUTE_SHAPE)).astype(np.float32)
    dx = _in(x)
    bad = 0
    for perm in itertools.permutations(range(3)):
        for flip in itertools.product((0, 1), repeat=3):
            out = _Out(x.size)
            rc = lib.bfm_permute_flip3d(L.ptr(dx), *K.PERMUTE_SHAPE, (C.c_int * 3)(*perm), (C.c_int * 3)(*flip), L.ptr(out.view),
                                        L.stream_ptr())
            assert rc == 0, (perm, flip, rc)
            ref = K.permute_flip_ref(x, perm, flip)
            got = out.get("permute_flip3d", shape=ref.shape)
            bad += K.n_diff(got, ref)
            assert K.bits_equal(got, ref), (perm, flip)
    print("permute_flip3d %s 6 x 8 pairs [permute_flip_kernel]: %d elements differ" % (K.PERMUTE_SHAPE, bad))
    out = _Out(x.size)
    for perm in ((0, 0, 1), (0, 1, 3), (-1, 1, 2), (2, 2, 2)):
        rc = lib.bfm_permute_flip3d(L.ptr(dx), *K.PERMUTE_SHAPE, (C.c_int * 3)(*perm), (C.c_int * 3)(0, 0, 0), L.ptr(out.view),
                                    L.stream_ptr())
        assert rc == E_ARG, (perm, rc)
    assert (out.get("permute_flip3d refused", np.int32) == UNWRITTEN).all()


def test_permute_flip3d_second_lap_of_the_grid_stride_loop():
    L, lib = _lib()
    shape, perm, flip = K.PERMUTE_LAP
    x = np.random.RandomState(6).randn(*shape).astype(np.float32)
    out = _Out(x.size)
    dx = _in(x)
    rc = lib.bfm_permute_flip3d(L.ptr(dx), *shape, (C.c_int * 3)(*perm), (C.c_int * 3)(*flip), L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    ref = K.permute_flip_ref(x, perm, flip)
    _same("permute_flip3d %s perm %s flip %s" % (shape, perm, flip), "permute_flip_kernel", out.get("permute_flip3d", shape=ref.shape), ref)


@pytest.mark.parametrize("name", K.BBOX_CASES)
def test_bbox_nonzero(name):
    L, lib = _lib()
    x, tol = K.bbox_case(name)
    out = _Out(6)
    dx = _in(x)
    rc = lib.bfm_bbox_nonzero(L.ptr(dx), x.shape[0], x.shape[1], x.shape[2], tol, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    got = out.get("bbox_nonzero", np.int32).tolist()
    ref = K.bbox_ref(x, tol)
    print("bbox_nonzero %s %s tol %g [bbox_kernel]: %s vs %s" % (name, x.shape, tol, got, ref))
    assert got == ref, name


@pytest.mark.parametrize("n,c", [(n, c) for n in K.MEAN_N + [K.MEAN_BIG] for c in K.MEAN_C])
def test_mean_lastdim_sequential_fp32(n, c):
    """c = 1, 2, 3, 7 at n = 1, 255 and 4096 * 256 + 3 (a second lap of the grid-stride loop)."""
    L, lib = _lib()
    x = K.mean_case(n, c)
    out = _Out(n)
    dx = _in(x)
    rc = lib.bfm_mean_lastdim(L.ptr(dx), n, c, L.ptr(out.view), L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    _same("mean_lastdim n=%d c=%d" % (n, c), "mean_lastdim_kernel", out.get("mean_lastdim"), K.mean_lastdim_ref(x))
