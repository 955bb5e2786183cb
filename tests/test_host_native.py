"""brainfm_amd.native without a GPU: the references of tests/native_refs.py and the host arithmetic.

Independent pin: the exact reference equals torch's CPU float64 grid_sample(padding_mode='zeros', align_corners=True) in
both modes (nearest on matrices with no coordinate near a half-integer, where grid_sample rounds half to even).
Emulation bound: the float32 chain stays within 12 * 2^-24 * sum |w||v| of the float64 sum over the weights it is given
(the bound counts the chain's roundings, none for forming a weight), and that sum within 3.01 * 2^-24 * sum |v| of the
trilinear value with float64 weights (native_refs.bound and weight_rounding_bound say why there are two terms).
Composition: vox2vox(aff_processed, aff_native) equals the explicit resize -> align -> crop map to 1e-9 voxels, with
aff_processed from the host arithmetic prepare_image runs (the grid of its `orig`); the grid to_native rebuilds for the
inference outputs equals the explicit resize -> crop map onto `final`, which prepare_image does not reorient.
Named mistakes: each one changes the reference's result on the test's inputs by more than the GPU tests tolerate."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from brainfm_amd import _lib as L
from brainfm_amd import misc as MI
from brainfm_amd import native as N
from brainfm_amd import test_utils as TU
import native_refs as NR

CASES = [(dst, name) for dst in NR.DSTS for name in NR.matrices(dst)]


def _grid_sample(src, x, y, z, mode):
    """torch CPU float64 grid_sample of one (D,H,W) volume at voxel coordinates (x,y,z)."""
    D, H, W = src.shape
    g = np.stack([2.0 * z / (W - 1) - 1.0, 2.0 * y / (H - 1) - 1.0, 2.0 * x / (D - 1) - 1.0], -1)
    out = TF.grid_sample(torch.from_numpy(np.asarray(src, dtype=np.float64))[None, None], torch.from_numpy(g)[None],
                         mode=mode, padding_mode="zeros", align_corners=True)
    return out[0, 0].numpy()


# ------------------------------------------------------------------------------------------------- independent pin
@pytest.mark.parametrize("dst,name", CASES)
def test_exact_linear_reference_equals_torch_float64_grid_sample(dst, name):
    src = NR.source(1)[0]
    x, y, z = NR.coords(NR.matrices(dst)[name], dst)
    val, mag = NR.linear_exact(src, x, y, z)
    ref = _grid_sample(src, x, y, z, "bilinear")
    # grid_sample goes through normalised coordinates: a few float64 roundings of the coordinate, times the slope
    assert np.abs(val - ref).max() <= 1e-12 * max(1.0, np.abs(src).max())
    assert (mag >= np.abs(val) - 1e-15).all()


@pytest.mark.parametrize("dst,name", [c for c in CASES if c[1] in NR.HALF_FREE])
def test_nearest_reference_equals_torch_grid_sample_away_from_half_integers(dst, name):
    src = NR.source(1)[0]
    x, y, z = NR.coords(NR.matrices(dst)[name], dst)
    excluded = sum(int((np.abs((c - np.floor(c)) - 0.5) < 1e-6).sum()) for c in (x, y, z))
    assert excluded == 0
    got = NR.nearest(src, x, y, z)
    assert np.array_equal(got.astype(np.float64), _grid_sample(src, x, y, z, "nearest"))


def test_nearest_copies_bit_patterns():
    src = NR.source(1)[0].copy()
    src.view(np.uint32)[2, 3, 4] = 0x7fc12345                     # a NaN with a payload
    src.view(np.uint32)[0, 0, 0] = 0x80000000                     # -0.0
    x, y, z = NR.coords(NR.matrices(NR.DSTS[0])["identity"], NR.SRC)
    assert np.array_equal(NR.nearest(src, x, y, z).view(np.uint32), src.view(np.uint32))
    ints = np.arange(np.prod(NR.SRC), dtype=np.int32).reshape(NR.SRC) - 50
    assert np.array_equal(NR.nearest(ints, x, y, z), ints)


# ------------------------------------------------------------------------------------------------- emulation
@pytest.mark.parametrize("dst,name", CASES)
def test_float32_emulation_within_the_derived_bound(dst, name):
    x, y, z = NR.coords(NR.matrices(dst)[name], dst)
    worst = [0.0, 0.0]
    for src in NR.source(17):
        val, mag = NR.linear_exact(src, x, y, z, weights="f32")
        truth, _ = NR.linear_exact(src, x, y, z)
        emu = NR.linear_f32(src, x, y, z)
        assert emu.dtype == np.float32
        err = np.abs(emu.astype(np.float64) - val)
        assert (err <= NR.bound(mag)).all()
        # ... and the sum over the kernel's float32 weights lies within the weight rounding of the trilinear value
        # itself, the one pinned to grid_sample above
        wr = NR.weight_rounding_bound(NR.corner_abs_sum(src, x, y, z))
        assert (np.abs(val - truth) <= wr).all()
        worst[0] = max(worst[0], float((err / np.maximum(NR.bound(mag), 1e-300)).max()))
        worst[1] = max(worst[1], float((np.abs(val - truth) / np.maximum(wr, 1e-300)).max()))
        if name in ("identity", "signed_perm"):                   # weights 0 and 1: the chain is exact
            assert np.array_equal(emu.astype(np.float64), truth)
    print("%s %s: worst chain error / bound = %.3f, worst weight rounding / its bound = %.3f" % (dst, name, *worst))


def test_signed_permutation_is_plain_indexing():
    src = NR.source(1)[0]
    dst = NR.DSTS[0]
    x, y, z = NR.coords(NR.matrices(dst)["signed_perm"], dst)
    want = np.zeros(dst, dtype=np.float32)
    for i, j, k in itertools.product(*[range(n) for n in dst]):
        s = (5 - j, k - 1, i + 2)
        if all(0 <= s[a] < NR.SRC[a] for a in range(3)):
            want[i, j, k] = src[s]
    assert np.array_equal(NR.linear_f32(src, x, y, z), want)
    assert np.array_equal(NR.nearest(src, x, y, z), want)
    assert 0 < (want != 0).sum() < want.size


# ------------------------------------------------------------------------------------------------- argmax rules
def test_argmax_reference_rules():
    x, y, z = NR.coords(NR.matrices(NR.SRC)["identity"], NR.SRC)
    p = NR.posteriors(5)
    lut = NR.lut_for(5)
    lab, best = NR.argmax_labels(p, lut, x, y, z)
    first = np.argmax(p, -1)                                      # np.argmax takes the first of equal maxima
    want = np.where(p.max(-1) > 0, lut[first], 0)
    assert np.array_equal(lab, want) and np.array_equal(best, p.max(-1))
    assert (lab[1] == 0).all() and (best[1] == 0).all()           # the all-zero plane
    ties = (p == p.max(-1, keepdims=True)).sum(-1) > 1
    assert ties[p.max(-1) > 0].sum() >= 20
    q = p.copy()
    q[2, 2, 2, :] = np.nan                                        # a NaN never wins, not even over nothing
    q[3, 3, 3, 0] = np.nan
    lab2, best2 = NR.argmax_labels(q, lut, x, y, z)
    assert lab2[2, 2, 2] == 0 and best2[2, 2, 2] == 0
    assert lab2[3, 3, 3] == lut[1 + int(np.argmax(p[3, 3, 3, 1:]))]
    far = [np.full((1, 1, 1), 50.0)] * 3                           # outside the field of view
    assert NR.argmax_labels(p, lut, *far)[0][0, 0, 0] == 0


def test_route_function():
    r = L.load().bfm_affine_pull_route
    assert [r(c) for c in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 70, 1000)] == \
        [1, 1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 16, 16]
    assert r(0) == -1 and r(-3) == -1


# ------------------------------------------------------------------------------------------------- composition
def _native_affine(perm, flips, spacing, oblique=False):
    """Voxel axis a runs along world axis perm[a] (reversed where flips[a]) with the given spacing."""
    A = np.eye(4)
    A[:3, :3] = 0
    for a in range(3):
        A[perm[a], a] = (-1.0 if flips[a] else 1.0) * spacing[a]
    if oblique:
        t = 0.03
        A[:3, :3] = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]]) @ A[:3, :3]
    A[:3, 3] = [-11.5, 7.25, 3.0]
    return A


def _prepare_affine(shape, aff, win_size, crops=1):
    """aff_processed by the host arithmetic prepare_image runs: resize_plan and the zoom's affine update, align_plan,
    then center_crop itself (indexing only) on a host tensor of the aligned shape -- `crops` times on ONE array, as
    prepare_image calls it."""
    newsize, _ = MI.resize_plan(shape, aff, 1.)
    aff_r = NR.zoom_affine(aff, shape, newsize)
    perm, _, aff_a = MI.align_plan(tuple(int(n) for n in newsize), aff_r, np.eye(4), 3)
    vol = torch.zeros([int(newsize[p]) for p in perm])
    for _ in range(crops):
        crop, _, _, aff_c = TU.center_crop(vol, win_size, aff=aff_a)
    return aff_c, tuple(crop.shape[2:])


FLIPS = ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1))
SHAPE = (20, 24, 18)


@pytest.mark.parametrize("spacing", [(0.8, 1.0, 1.3), (1.0, 1.0, 1.0)])
@pytest.mark.parametrize("win_size", [None, (14, 15, 13)])
def test_vox2vox_equals_the_explicit_three_step_map(spacing, win_size):
    seen = 0
    for perm, flips in itertools.product(itertools.permutations(range(3)), FLIPS):
        aff = _native_affine(perm, flips, spacing)
        aff_p, shape_p = _prepare_affine(SHAPE, aff, win_size)
        want, shape_w = NR.prepare_voxel_map(SHAPE, aff, win_size)
        got = N.vox2vox(aff_p, aff)
        assert shape_p == shape_w
        assert np.abs(got - want).max() <= 1e-9, (perm, flips)
        grid_shape, grid_aff = N.processed_grid(SHAPE, aff, shape_p, aligned=True)
        assert grid_shape == shape_p and np.abs(grid_aff - aff_p).max() <= 1e-12
        if win_size is not None:
            assert all(s <= w for s, w in zip(shape_p, win_size)) and shape_p != N.processed_grid(SHAPE, aff, aligned=True)[0]
        seen += 1
    assert seen == 24


def _prepare_image_host(shape, aff, win_size, add_bf=False):
    """What prepare_image hands back, by its own host arithmetic on host tensors: (`aff`, the shape of `final`).  `orig`
    is aligned and cropped; `high_res` and `final` (and `bf`) go through align_plan with the affine of the ALREADY aligned
    volume, which leaves them as they are, and through center_crop with the same affine array once more each."""
    newsize, _ = MI.resize_plan(shape, aff, 1.)
    resized = tuple(int(n) for n in newsize)
    perm, _, aff_before_crop = MI.align_plan(resized, NR.zoom_affine(aff, shape, newsize), np.eye(4), 3)
    _, _, _, aff_ret = TU.center_crop(torch.zeros([resized[p] for p in perm]), win_size, aff=aff_before_crop)
    for _ in range(3 if add_bf else 2):
        perm2, flip2, _ = MI.align_plan(resized, aff_before_crop, np.eye(4), 3)
        assert perm2 == [0, 1, 2] and not any(flip2)
        final, _, _, _ = TU.center_crop(torch.zeros(resized), win_size, aff=aff_before_crop)
    assert aff_ret is aff_before_crop
    return aff_ret, tuple(final.shape[2:])


@pytest.mark.parametrize("spacing", [(0.8, 1.0, 1.3), (1.0, 1.0, 1.0)])
@pytest.mark.parametrize("win_size", [None, (14, 15, 13)])
def test_the_grid_to_native_rebuilds_is_the_explicit_map_onto_final(spacing, win_size):
    """The outputs lie on `final`'s grid: resize and crop, no reorientation.  to_native rebuilds it from the scan and the
    shape; the `aff` prepare_image returns (the reoriented `orig`'s, with crop offsets of two shapes piled up) would not
    do, which the test shows for every scan that is not already on the identity axes and for every crop."""
    wrong = 0
    for perm, flips in itertools.product(itertools.permutations(range(3)), FLIPS):
        aff = _native_affine(perm, flips, spacing)
        for add_bf in (False, True):
            aff_ret, shape_f = _prepare_image_host(SHAPE, aff, win_size, add_bf)
            want, shape_w = NR.prepare_voxel_map(SHAPE, aff, win_size, align=False)
            assert shape_f == shape_w
            got = N.vox2vox(N._output_grid_affine(aff_ret, shape_f, SHAPE, aff), aff)
            assert np.abs(got - want).max() <= 1e-9, (perm, flips)
            assert N.processed_grid(SHAPE, aff, shape_f)[0] == shape_f
            naive = np.abs(N.vox2vox(aff_ret, aff) - want).max()
            identity_axes = perm == (0, 1, 2) and not any(flips)
            assert (naive <= 1e-9) == (identity_axes and win_size is None), (perm, flips, naive)
            wrong += naive > 0.5
    assert wrong >= (46 if win_size is None else 48)


def test_to_native_recognises_the_scan_and_a_zero_crop():
    aff = _native_affine((2, 0, 1), (1, 0, 1), (0.8, 1.0, 1.3))
    full, _ = N.processed_grid(SHAPE, aff)
    full_al, aff_al = N.processed_grid(SHAPE, aff, aligned=True)
    assert sorted(full) == sorted(full_al) and full != full_al
    small = tuple(n - 3 for n in full)
    with pytest.raises(L.BfmError, match="zero_crop_first"):     # a smaller volume under the uncropped affine
        N._output_grid_affine(aff_al, small, SHAPE, aff)
    one_plane = (full[0] - 1,) + full[1:]                         # center_crop's own crop by one: start 0, no offset
    assert np.array_equal(N._output_grid_affine(aff_al, one_plane, SHAPE, aff), N.processed_grid(SHAPE, aff)[1])
    with pytest.raises(L.BfmError, match="axes differ"):
        N._output_grid_affine(aff, full, SHAPE, aff)
    with pytest.raises(L.BfmError, match="does not fit"):
        N._output_grid_affine(aff_al, tuple(n + 1 for n in full), SHAPE, aff)


def test_oblique_scan_composes_too():
    aff = _native_affine((1, 2, 0), (0, 1, 0), (0.8, 1.0, 1.3), oblique=True)
    aff_p, shape_p = _prepare_affine(SHAPE, aff, (14, 15, 13))
    want, _ = NR.prepare_voxel_map(SHAPE, aff, (14, 15, 13))
    assert np.abs(N.vox2vox(aff_p, aff) - want).max() <= 1e-9


# ------------------------------------------------------------------------------------------------- named mistakes
def _ramp_case():
    """A smooth volume on the processed grid of a flipped, permuted, anisotropic scan, pulled onto the native grid."""
    aff = _native_affine((2, 0, 1), (1, 0, 1), (0.8, 1.0, 1.3))
    aff_p, shape_p = _prepare_affine(SHAPE, aff, (14, 15, 13))
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape_p], indexing="ij")
    vol = (0.031 * i - 0.022 * j + 0.017 * k + 0.4).astype(np.float32)
    return aff, aff_p, shape_p, vol


def _pull(vol, M, **kw):
    return NR.linear_exact(vol, *NR.coords(M, SHAPE), **kw)


def test_each_named_mistake_moves_the_result_beyond_the_gpu_tolerances():
    aff, aff_p, shape_p, vol = _ramp_case()
    good, mag = _pull(vol, N.vox2vox(aff_p, aff))
    rng = float(vol.max() - vol.min())
    inside = mag > 0
    tol = np.maximum(NR.bound(mag), 0.0) + 1e-4 * rng             # the kernel bound plus the end-to-end tolerance
    interior = np.zeros(SHAPE, dtype=bool)
    interior[4:-4, 4:-4, 4:-4] = True                             # where the end-to-end test looks
    for what, M in (("half-voxel term dropped", NR.prepare_voxel_map(SHAPE, aff, (14, 15, 13), half_voxel=False)[0]),
                    ("flip offset n instead of n - 1", NR.prepare_voxel_map(SHAPE, aff, (14, 15, 13), flip_offset=0)[0]),
                    ("inv(dst) @ src", N.vox2vox(aff, aff_p))):
        bad, _ = _pull(vol, M)
        moved = np.abs(bad - good) > tol
        assert moved[inside & interior].any(), what
        print("%s: %d of %d interior voxels move, worst %.3g of the range" % (
            what, int(moved[inside & interior].sum()), int((inside & interior).sum()),
            float(np.abs(bad - good)[inside & interior].max() / rng)))
    clamped, _ = _pull(vol, N.vox2vox(aff_p, aff), pad="clamp")
    assert (np.abs(clamped - good) > tol).any(), "clamping instead of zero padding"
    # nearest: np.round takes halves to even, floor(x + 0.5) up
    src = NR.source(1)[0]
    x, y, z = NR.coords(NR.matrices(NR.DSTS[0])["aniso_half"], NR.DSTS[0])
    assert (NR.nearest(src, x, y, z).view(np.uint32) != NR.nearest(src, x, y, z, rounding="even").view(np.uint32)).any()
    # argmax: the last of equal maxima
    p, lut = NR.posteriors(5), NR.lut_for(5)
    xi, yi, zi = NR.coords(NR.matrices(NR.SRC)["identity"], NR.SRC)
    assert (NR.argmax_labels(p, lut, xi, yi, zi)[0] != NR.argmax_labels(p, lut, xi, yi, zi, take="last")[0]).any()


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_that_need_no_device():
    eye = np.eye(4)
    sing = np.diag([1.0, 1.0, 0.0, 1.0])
    with pytest.raises(L.BfmError, match="singular affine"):
        N.vox2vox(sing, eye)
    with pytest.raises(L.BfmError, match="singular affine"):
        N.vox2vox(eye, sing)
    with pytest.raises(L.BfmError, match="4 x 4"):
        N.vox2vox(np.eye(3), eye)
    with pytest.raises(L.BfmError, match="HIP device only"):
        N.resample_maps(torch.zeros(2, 3, 4, 5), eye, (3, 4, 5), eye)
    with pytest.raises(L.BfmError, match="HIP device only"):
        N.resample_labels(torch.zeros(1, 2, 3, 4, 5), [0, 1], eye, (3, 4, 5), eye)
    with pytest.raises(L.BfmError, match="HIP device only"):
        N.to_native({"T1": torch.zeros(3, 4, 5)}, eye, (3, 4, 5), eye)
    assert np.array_equal(N.vox2vox(eye, eye), eye) and N.vox2vox(eye, eye).dtype == np.float64
