"""The case lists and references of tests/synth_kernel_refs.py without a GPU.

Routes: bfm_zoom_linear_route and bfm_conv1d_axis_plan are host arithmetic and the library loads without a device; the
case lists reach every route of both launchers and every threshold case falls on the side written next to it.
Oracle pinning: the references reproduce tests/golden/synth_edges.npz -- the reference's own fast_3D_interp_torch,
myzoom_torch, get_deformed_atlas (bit for bit) and gaussian_blur_3d (within the float64 bound) on the same inputs
(tests/golden/make_golden_synth_edges.py).  The new restatements agree with the oracle where the two overlap.
Discrimination: each named mistake, applied to a reference, changes the result on the case list (for the blur: by more
than the bound).  A mutant that no case catches means a case is missing."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import load_npz
from oracle import synth_ref as S
import synth_kernel_refs as K


def _lib():
    from brainfm_amd import _lib as L
    return L.load()


def _conv_plan(lib, shape, axis, klen):
    seg, nslab, lds = C.c_int(-1), C.c_int(-1), C.c_size_t(1 << 40)
    route = lib.bfm_conv1d_axis_plan(shape[0], shape[1], shape[2], axis, klen, C.byref(seg), C.byref(nslab), C.byref(lds))
    return route, seg.value, nslab.value, lds.value


def _zoom_route(lib, shape, factor, aligned=1):
    C_ = shape[3] if len(shape) == 4 else 1
    o = K.zoom_out_shape(shape, factor)
    return lib.bfm_zoom_linear_route(shape[0], shape[1], shape[2], C_, o[0], o[1], o[2], aligned)


# ------------------------------------------------------------------------------------------------- routes
def test_zoom_cases_reach_every_route_and_sit_on_the_stated_side_of_each_threshold():
    lib = _lib()
    seen = set()
    for name, shape, factor, want in K.ZOOM_CASES:
        got = _zoom_route(lib, shape, factor)
        assert got == want, (name, got, want)
        seen.add(got)
    for name, shape, factor, want in K.ZOOM_LAP_CASES:
        assert _zoom_route(lib, shape, factor) == want, name
    o = K.zoom_out_shape(*K.ZOOM_LAP_CASES[0][1:3])
    assert o[0] * o[1] * o[2] > 1024 * 256 * 4 and sum(o) <= 1024          # a second lap of the LDS-resident form
    o = K.zoom_out_shape(*K.ZOOM_LAP_CASES[1][1:3])
    assert o[0] * o[1] > 8192 * 4                                           # and of the long form
    for name, want in K.ZOOM_MISALIGNED:
        X, factor, aligned_route = K.zoom_case(name)
        assert _zoom_route(lib, X.shape, factor, 0) == want and aligned_route != want, name
    assert seen == {0, 1, 2, 3}
    # the thresholds themselves: 2048 source elements, tables of 1024, rows of 1024 / 2048 floats
    r = lib.bfm_zoom_linear_route
    assert r(8, 16, 16, 1, 4, 4, 8, 1) == 0 and r(8, 16, 17, 1, 4, 4, 8, 1) == 1
    assert r(2, 2, 2, 1, 2, 2, 1020, 1) == 0 and r(2, 2, 2, 1, 2, 2, 1024, 1) == 1
    assert r(2, 2, 2, 3, 2, 2, 8, 1) == 1                                   # C = 3 never takes the LDS-resident form
    assert r(2, 2, 1024, 1, 2, 2, 2048, 1) == 1 and r(2, 2, 1025, 1, 2, 2, 2048, 1) == 3
    assert r(2, 2, 1024, 1, 2, 2, 2049, 1) == 3 and r(2, 2, 1024, 1, 2, 2, 2052, 1) == 3
    assert r(2, 2, 1024, 1, 2, 2, 2048, 0) == 2
    assert r(0, 2, 2, 1, 2, 2, 2, 1) == -1 and r(2, 2, 2, 1, 2, 2, 0, 1) == -1 and r(2, 2, 2, 0, 2, 2, 2, 1) == -1
    assert r(2, 2, 2, 1, 1 << 16, 1 << 16, 2, 1) == -2


def test_conv1d_cases_reach_every_route_with_the_stated_segments():
    lib = _lib()
    seen = set()
    plans = {}
    for name, shape, axis, klen, sigma, want in K.CONV1D_CASES:
        route, seg, nslab, lds = _conv_plan(lib, shape, axis, klen)
        assert route == want, (name, route, want)
        assert lds <= 64 * 1024, (name, lds)
        assert nslab >= 1 and (seg >= (4 if axis == 2 else 8) if route != K.C1D_FALLBACK else (seg == 0 and lds == 0)), name
        seen.add(route)
        plans[name] = (seg, nslab, lds)
    assert seen == {0, 1, 2, 3}
    assert plans["fallback_second_lap"][1] == 8192 and 182 * 182 > 8192 * 4    # the fallback's grid is capped: a second lap
    # a segment longer than the minimum: 6 x 14 = 84 lines, 2048 // 84 = 24 segments wanted, ceil(200 / 24) = 9
    assert plans["long_segment"] == (9, 84 * 23, (9 + 11 - 1) * 65 * 4)
    # nine rows in slabs of four: the last slab holds one row
    assert plans["partial_last_slab"] == (4, 3, 4 * 1025 * 4)
    p = lib.bfm_conv1d_axis_plan
    assert p(3, 3, 1024, 2, 9, None, None, None) == 2 and p(3, 3, 1025, 2, 9, None, None, None) == 3
    assert p(3, 3, 1025, 0, 9, None, None, None) == 0                      # the z limit is the axis-2 slab's alone
    for axis in range(3):
        assert p(12, 10, 70, axis, 63, None, None, None) == axis and p(12, 10, 70, axis, 65, None, None, None) == 3
    for bad in ((0, 3, 3, 0, 9), (3, 3, 3, 3, 9), (3, 3, 3, -1, 9), (3, 3, 3, 0, 8), (3, 3, 3, 0, 0)):
        assert p(*bad, None, None, None) == -1, bad
    assert p(1 << 16, 1 << 16, 1, 0, 9, None, None, None) == -2


def test_plan_lds_stays_under_64k_over_a_grid():
    lib = _lib()
    for shape, axis, klen in itertools.product([(1, 1, 1), (7, 300, 65), (300, 7, 1024), (2000, 3, 64), (160, 160, 160),
                                                (256, 256, 256), (3, 5000, 1000)], range(3), (1, 9, 63, 64 + 1)):
        route, seg, nslab, lds = _conv_plan(lib, shape, axis, klen)
        assert route in (axis, 3) and lds <= 64 * 1024, (shape, axis, klen, lds)


# ------------------------------------------------------------------------------------------------- oracle pinning
@pytest.fixture(scope="module")
def edges():
    return load_npz("synth_edges.npz")


def test_interp_references_reproduce_the_reference_bit_for_bit(edges):
    for vi, (shape, spiked) in enumerate(K.INTERP_VOLUMES):
        X = K.interp_volume(shape, spiked)
        for pname, pts in (("lattice", K.lattice_points(shape)), ("hand", K.hand_points(shape))):
            for dv in K.INTERP_DEFAULTS:
                want = edges["lin/%d/%s/%g" % (vi, pname, dv)]
                assert K.bits_equal(K.interp_linear_ref(X, *pts, dv), want, nan_class=spiked), (shape, spiked, pname, dv)
                if len(shape) == 3:                    # the switchable restatement with every switch off: the same bits
                    assert K.bits_equal(K.interp3d_linear_variant(X, *pts, dv), want, nan_class=spiked), (shape, pname, dv)
    # ny = 1: nothing is valid
    assert np.all(edges["lin/4/lattice/-7.5"] == -7.5) and np.all(edges["lin/4/hand/0"] == 0)
    pts = K.nearest_points()
    for kind in ("int32", "bits"):
        for C_ in (1, 3):
            X = K.nearest_volume(kind, C_)
            assert K.bits_equal(S.interp3d_nearest(X, *pts), edges["near/%s/%d" % (kind, C_)]), (kind, C_)


def test_zoom_and_atlas_references_reproduce_the_reference_bit_for_bit(edges):
    for name, shape, factor, _ in K.ZOOM_CASES:
        X, f, _ = K.zoom_case(name)
        ref = S.myzoom(X, f)
        assert ref.shape[:3] == K.zoom_out_shape(shape, factor)
        assert K.bits_equal(ref, edges["zoom/" + name]), name
    for name in K.ATLAS_CASES:
        case = K.atlas_case(name)
        assert K.bits_equal(K.atlas_ref(*case), edges["atlas/" + name]), name
        assert K.bits_equal(K.atlas_ref(*case, tile=True), edges["atlas_tile/" + name]), name
    # the cases do what their names say
    m, rx, ry, rz, atlas, A = K.atlas_case("last_texel")
    out = K.atlas_ref(m, rx, ry, rz, atlas, A)
    assert np.all(out[m > 0] == atlas[-1, -1, -1]) and np.all(out[~(m > 0)] == 0)
    out = K.atlas_ref(*K.atlas_case("partly_outside"))
    kept = K.atlas_case("partly_outside")[0] > 0
    assert 0 < int((out[kept] == 0).sum()) < int(kept.sum())


def test_float64_correlation_is_within_its_bound_of_the_references_blur(edges):
    """|gaussian_blur_3d - ref64| <= (klen + 1) 2^-24 sum |k||x| for the reference's own fp32 result too, and the oracle's
    blur (float64 accumulation, one rounding) within two roundings."""
    for name in K.CONV1D_GOLDEN:
        x, k, axis, sigma, _ = K.conv1d_case(name, "gauss")
        ref, mag = K.correlate1d_ref(x, k, axis)
        assert K.conv1d_ratio(edges["blur/" + name], ref, mag, len(k)) <= 1.0, name
        orc = S.gaussian_blur_3d(x, K.blur_stds(axis, sigma))
        assert float(np.abs(orc - ref).max()) <= 2.0 ** -24 * float(np.abs(ref).max()), name


# ------------------------------------------------------------------------------------------------- restatements vs oracle
def test_restatements_agree_with_the_oracle_where_they_overlap():
    for name, size, withF, kind in K.DEFORM_CASES:
        size, shp, A, c2, F = K.deform_case(name)
        xx, yy, zz, mm = K.deform_grid_raw(size, shp, A, c2, F)
        oxx, oyy, ozz, lo, hi = S.deform_grid(size, shp, A, c2, F)
        assert lo == [int(np.floor(v)) for v in mm[:3]] and hi == [1 + int(np.ceil(v)) for v in mm[3:]], name
        for got, want, l in zip((xx, yy, zz), (oxx, oyy, ozz), lo):
            assert K.bits_equal((got - np.float32(l)).astype(np.float32), want), name
        if kind == "below":
            assert np.all(mm == 0)
        if kind == "above":
            assert list(mm[:3]) == list(mm[3:]) == [s - 1 for s in shp]
    for n in K.LABEL_SIZES:
        G, mus, sg, rn, _ = K.label_case(n, in_range=True)
        l = np.clip(K._label_index(G), 0, K.NTAB - 1)
        v = (mus[l] + sg[l] * rn).astype(np.float32)
        v[v < 0] = 0
        assert K.bits_equal(v, S.synth_from_labels(G, mus, sg, rn)), n
        G, mus, sg, rn, _ = K.label_case(n)
        out = K.label_gauss_ref(G, mus, sg, rn)
        assert out.min() >= 0 and (n < 9 or (out[7] == max(0, mus[255] + sg[255] * rn[7]) and out[8] == max(0, mus[0] + sg[0] * rn[8])))
    for nl, n in K.ONEHOT_CASES:
        Sv, lut = K.onehot_case(nl, n, in_range=True)
        idx = lut[Sv]
        assert K.bits_equal((idx[..., None] == np.arange(nl)).astype(np.float32), S.onehot_lut(Sv, lut, nl)), nl
        Sv, lut = K.onehot_case(nl, n)
        out = K.onehot_ref(Sv, lut, nl)
        assert out.shape == (n, nl) and set(out.sum(1)) == {0.0, 1.0}          # LUT entries outside the range: an all-zero row
        assert out[0].argmax() == nl - 1 and out[2].sum() == 0                 # S = -1 -> lut[0]; S = nlut -> lut[nlut-1]
    G, _, _, _, syn = K.label_case(63)
    cer, stats, mags = K.label_class_stats_ref(G, syn)
    assert stats[1] + stats[3] == float((np.rint(np.where(G == 77, 2, G)) != 0).sum()) and stats[1] >= 4   # 2, 41, 77, 2.5
    assert cer[0] == 0 and cer[1] == syn[1]


# ------------------------------------------------------------------------------------------------- the cases discriminate
INTERP_MUTANTS = ["lower_inclusive", "upper_strict", "z_unclamped", "pair_next_row"]


@pytest.mark.parametrize("mutant", INTERP_MUTANTS)
def test_interp_linear_cases_catch(mutant):
    caught = []
    for shape, spiked in K.INTERP_VOLUMES:
        if len(shape) != 3:
            continue
        X = K.interp_volume(shape, spiked)
        for pname, pts in (("lattice", K.lattice_points(shape)), ("hand", K.hand_points(shape))):
            ref = K.interp_linear_ref(X, *pts, -7.5)
            if not K.bits_equal(K.interp3d_linear_variant(X, *pts, -7.5, **{mutant: True}), ref, nan_class=True):
                caught.append((shape, spiked, pname))
    print(mutant, "caught by", caught)
    assert caught, mutant
    if mutant == "pair_next_row":
        # the second dword of the pair at a row end is only visible through a non-finite voxel at the next row's start
        assert all(spiked for _, spiked, _ in caught)


def test_nearest_cases_catch_round_half_away():
    pts = K.nearest_points()
    for kind, C_ in (("int32", 1), ("bits", 3)):
        X = K.nearest_volume(kind, C_)
        assert not K.bits_equal(K.nearest_variant(X, *pts, half_away=True), S.interp3d_nearest(X, *pts)), kind
        assert K.bits_equal(K.nearest_variant(X, *pts), S.interp3d_nearest(X, *pts))


def test_atlas_cases_catch_swapped_mask_predicates():
    for name in K.ATLAS_CASES:
        case = K.atlas_case(name)
        assert not K.bits_equal(K.atlas_ref(*case), K.atlas_ref(*case, tile=True)), name


def test_conv1d_cases_catch_reversed_taps():
    """With the random (asymmetric) taps the flipped kernel misses the bound in every case; with the Gaussians it is the
    same kernel, which is why Gaussians alone cannot see it."""
    for name, shape, axis, klen, sigma, _ in K.CONV1D_CASES:
        if np.prod(shape) > 100000:
            continue
        x, k, axis, _, _ = K.conv1d_case(name, "random")
        ref, mag = K.correlate1d_ref(x, k, axis)
        rev, _ = K.correlate1d_ref(x, k, axis, reverse=True)
        assert K.conv1d_ratio(rev.astype(np.float32), ref, mag, klen) > 1.0, name
        assert K.conv1d_ratio(ref.astype(np.float32), ref, mag, klen) <= 1.0, name
        g = K.conv1d_case(name, "gauss")[1]
        assert np.array_equal(g, g[::-1]) and not np.array_equal(k, k[::-1])


def test_permute_cases_catch_the_inverse_permutation():
    x = np.arange(np.prod(K.PERMUTE_SHAPE), dtype=np.float32).reshape(K.PERMUTE_SHAPE)
    caught = 0
    for perm in itertools.permutations(range(3)):
        for flip in itertools.product((0, 1), repeat=3):
            a, b = K.permute_flip_ref(x, perm, flip), K.permute_flip_ref(x, perm, flip, inverse=True)
            assert a.shape == tuple(K.PERMUTE_SHAPE[p] for p in perm)
            # the kernel's own definition, element by element
            i = np.array([1, 2, 0]) % np.array(a.shape)
            j = [0, 0, 0]
            for ax in range(3):
                j[perm[ax]] = a.shape[ax] - 1 - i[ax] if flip[ax] else i[ax]
            assert a[tuple(i)] == x[tuple(j)], (perm, flip)
            caught += int(a.shape != b.shape or not np.array_equal(a, b))
    assert caught == 2 * 8                                 # the two 3-cycles are the permutations that are not their own inverse


def test_bbox_and_mean_references():
    assert K.bbox_ref(*K.bbox_case("nothing_above_tol")) == K.BBOX_EMPTY
    assert K.bbox_ref(*K.bbox_case("first_voxel")) == [0, 0, 0, 1, 1, 1]
    assert K.bbox_ref(*K.bbox_case("last_voxel")) == [5, 4, 8, 6, 5, 9]
    assert K.bbox_ref(*K.bbox_case("nan_voxels")) == [2, 1, 3, 5, 4, 6]
    assert K.bbox_ref(*K.bbox_case("negative_tol")) == [1, 2, 4, 4, 3, 8]
    assert K.bbox_ref(*K.bbox_case("above_512_blocks")) == [5, 3, 1, 62, 46, 48]
    x = K.mean_case(255, 7)
    assert float(np.abs(K.mean_lastdim_ref(x) - x.astype(np.float64).mean(1)).max()) <= 8 * 2.0 ** -24 * float(np.abs(x).sum(1).max())
    assert K.bits_equal(K.mean_lastdim_ref(K.mean_case(255, 1)), K.mean_case(255, 1)[:, 0])
