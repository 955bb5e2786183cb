"""brainfm_amd.native on the device (csrc/affine_pull.hip) against the restatements of tests/native_refs.py.

bfm_affine_pull_multi: bit for bit against the float32 emulation in both modes and within the derived bound
(12 * 2^-24 * sum |w||v|) of the float64 sum over the weights the chain is given, on every shape x matrix x K of the
shared case list; against the trilinear value with float64 weights the rounding of the weights themselves is added
(native_refs.weight_rounding_bound: the first figure alone fails there, 1.41 x at one voxel of 'rot_shear' on (3,5,67),
where a weight of 0.024 has its partner on a zero-padded texel).  The signed permutation equals plain indexing bit for
bit.  bfm_affine_pull_argmax: labels and winning values equal the emulation at
every voxel, and the labels equal "pull C volumes with bfm_affine_pull_multi, torch.argmax, lut" at every voxel (the same
arithmetic), for channel counts that reach every lane width bfm_affine_pull_route names and more than 64 channels;
every width that can be forced (1 to 64) gives the bits of the chosen one.
Containers, the offsets past 2^31, the refusals, and prepare_image -> to_native end to end on a ramp that is linear in
world coordinates (1e-4 of its range: a half-voxel or flip-offset slip moves it by 5e-3, see test_host_native.py):
`final`, which keeps the scan's axes, through to_native, and `orig`, the reoriented one, through its own grid."""
import numpy as np
import pytest
import torch

from brainfm_amd import _lib as L
from brainfm_amd import native as N
from brainfm_amd import test_utils as TU
import native_refs as NR
from test_host_native import _native_affine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EYE = np.eye(4)
CASES = [(dst, name) for dst in NR.DSTS for name in NR.matrices(dst)]
CHANNELS = (1, 2, 5, 7, 12, 20, 33, 70)          # lane widths 1, 1, 1, 2, 4, 4, 8, 16: one to five channels per lane
_REF = {}


def T(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)     # a copy: the shared references are read-only


def M4(dst, name):
    return np.vstack([NR.matrices(dst)[name], [0, 0, 0, 1.0]])


def ref_maps(dst, name, K):
    """(source, emulation linear, exact linear, sum |w||v|, nearest) of the K maps, computed once."""
    key = (dst, name, K)
    if key not in _REF:
        src = NR.source(K)
        xyz = NR.coords(NR.matrices(dst)[name], dst)
        emu = np.stack([NR.linear_f32(s, *xyz) for s in src])
        ex = [NR.linear_exact(s, *xyz, weights="f32") for s in src]
        truth = np.stack([NR.linear_exact(s, *xyz)[0] for s in src])
        wr = np.stack([NR.weight_rounding_bound(NR.corner_abs_sum(s, *xyz)) for s in src])
        near = np.stack([NR.nearest(s, *xyz) for s in src])
        _REF[key] = (src, emu, np.stack([e[0] for e in ex]), np.stack([e[1] for e in ex]), near, truth, wr)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------- multi
@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("dst,name", CASES)
def test_pull_multi_equals_the_emulation_bit_for_bit(dst, name, K):
    src, emu, exact, mag, near, truth, wr = ref_maps(dst, name, K)
    dsrc = T(src)
    lin = N.resample_maps(dsrc, EYE, dst, M4(dst, name), nearest=())
    assert lin.shape == (K,) + dst and lin.dtype == torch.float32
    assert np.array_equal(bits(lin), bits(emu))
    got = lin.cpu().numpy().astype(np.float64)
    assert (np.abs(got - exact) <= NR.bound(mag)).all()           # the float64 sum over the weights the chain is given
    assert (np.abs(got - truth) <= NR.bound(mag) + wr).all()      # the trilinear value itself: plus the weight rounding
    nn = N.resample_maps(dsrc, EYE, dst, M4(dst, name), nearest=tuple(range(K)))
    assert np.array_equal(bits(nn), bits(near))
    mixed = N.resample_maps(dsrc, EYE, dst, M4(dst, name), nearest=tuple(range(1, K, 2)))
    want = np.stack([near[m] if m % 2 else emu[m] for m in range(K)])
    assert np.array_equal(bits(mixed), bits(want))


def test_nearest_copies_nan_payloads_and_int32():
    dst = NR.SRC
    src = NR.source(2).copy()
    src.view(np.uint32)[0, 2, 3, 4] = 0x7fc12345
    src.view(np.uint32)[1, 0, 0, 0] = 0x80000000
    out = N.resample_maps(T(src), EYE, dst, EYE, nearest=(0, 1))
    assert np.array_equal(bits(out), bits(src))
    ints = (np.arange(np.prod(dst), dtype=np.int32).reshape(dst) - 50)
    got = N.resample_maps({"label": T(ints)}, EYE, dst, EYE)["label"]
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ints)


@pytest.mark.parametrize("dst", NR.DSTS[:2])
def test_signed_permutation_is_plain_indexing(dst):
    src = NR.source(3)
    want = np.zeros((3,) + dst, dtype=np.float32)
    for i in range(dst[0]):
        for j in range(dst[1]):
            for k in range(dst[2]):
                s = (5 - j, k - 1, i + 2)
                if all(0 <= s[a] < NR.SRC[a] for a in range(3)):
                    want[:, i, j, k] = src[:, s[0], s[1], s[2]]
    for nearest in ((), (0, 1, 2)):
        out = N.resample_maps(T(src), EYE, dst, M4(dst, "signed_perm"), nearest=nearest)
        assert np.array_equal(bits(out), bits(want))


def test_offsets_past_2_to_the_31():
    """17 maps whose rows lie 2^27 + 8 elements apart onto 512^3: the last map's source offset (2^31 + 128 elements) and
    the last map's destination offsets (2^31 and up) do not fit a signed 32-bit integer.  Each map must equal the same map
    pulled on its own."""
    K, n, stride, dst = 17, int(np.prod(NR.SRC)), (1 << 27) + 8, (512, 512, 512)
    src = NR.source(K)
    buf = torch.empty(K * stride, dtype=torch.float32, device=DEV)
    rows = {}
    for m in range(K):
        row = buf[m * stride:m * stride + n].view(NR.SRC)
        row.copy_(T(src[m]))
        rows["m%d" % m] = row
    Mx = np.diag([4.5 / 511, 5.5 / 511, 6.5 / 511, 1.0])
    Mx[:3, 3] = [-0.25, -0.25, -0.25]
    out = N.resample_maps(rows, EYE, dst, Mx, nearest=("m3",))
    assert out["m16"].data_ptr() - out["m0"].data_ptr() == 16 * 4 * 512 ** 3 >= 4 * (1 << 31)
    assert 16 * stride > (1 << 31)
    for m in (0, 3, 15, 16):
        alone = N.resample_maps(T(src[m:m + 1]), EYE, dst, Mx, nearest=(0,) if m == 3 else ())
        assert torch.equal(out["m%d" % m].view(torch.int32), alone[0].view(torch.int32)), m
    assert float(out["m16"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------- argmax
def test_channel_counts_reach_every_route():
    r = L.load().bfm_affine_pull_route
    assert {r(c) for c in CHANNELS} == {1, 2, 4, 8, 16} and max(CHANNELS) > 64   # 32 and 64: the forced-width test
    assert {1, 2, 5, 33, 70} <= set(CHANNELS)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("dst", NR.DSTS)
def test_pull_argmax_equals_the_emulation_and_the_composed_route(dst, C):
    post = NR.posteriors(C)
    lut = NR.lut_for(C)
    dpost = T(post).permute(3, 0, 1, 2)[None]                     # (1,C,D,H,W) over channels-last memory
    assert dpost[0].permute(1, 2, 3, 0).is_contiguous()
    planes = T(np.ascontiguousarray(np.moveaxis(post, -1, 0)))    # (C,D,H,W)
    dlut = T(lut).long()
    for name in NR.matrices(dst):
        xyz = NR.coords(NR.matrices(dst)[name], dst)
        want_lab, want_best = NR.argmax_labels(post, lut, *xyz)
        lab, best = N.resample_labels(dpost, lut, EYE, dst, M4(dst, name), return_max=True)
        assert lab.dtype == torch.int32 and lab.shape == dst
        assert np.array_equal(lab.cpu().numpy(), want_lab), (name, int((lab.cpu().numpy() != want_lab).sum()))
        assert np.array_equal(bits(best), bits(want_best)), name
        only = N.resample_labels(dpost, lut, EYE, dst, M4(dst, name))
        assert torch.equal(only, lab)
        vols = N.resample_maps(planes, EYE, dst, M4(dst, name), nearest=())
        top, arg = vols.max(0), torch.argmax(vols, 0)             # argmax: the first of equal maxima
        composed = torch.where(top.values > 0, dlut[arg], torch.zeros_like(arg)).to(torch.int32)
        assert torch.equal(composed, lab), name
        assert np.array_equal(bits(top.values.clamp_min(0)), bits(best)), name
    if C >= 2 and dst == NR.DSTS[0]:                              # the planted ties and zeros did their work
        xyz = NR.coords(NR.matrices(dst)["identity"], dst)
        lab_last, _ = NR.argmax_labels(post, lut, *xyz, take="last")
        want_lab, _ = NR.argmax_labels(post, lut, *xyz)
        assert (lab_last != want_lab).any() and (want_lab[1] == 0).all()


@pytest.mark.parametrize("C", [5, 33, 70])
def test_every_forced_lane_width_gives_the_bits_of_the_chosen_one(C):
    dst = NR.DSTS[1]
    dpost = T(NR.posteriors(C)).permute(3, 0, 1, 2)[None]
    lut = NR.lut_for(C)
    for name in ("rot_shear", "aniso_half"):
        lab, best = N.resample_labels(dpost, lut, EYE, dst, M4(dst, name), return_max=True)
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            l2, b2 = N.resample_labels(dpost, lut, EYE, dst, M4(dst, name), return_max=True, lanes=lanes)
            assert torch.equal(l2, lab) and torch.equal(b2.view(torch.int32), best.view(torch.int32)), (name, lanes)
    with pytest.raises(L.BfmError, match="BFM_E_ARG"):
        N.resample_labels(dpost, lut, EYE, dst, EYE, lanes=3)


def test_argmax_nan_never_wins_and_strided_posteriors_are_made_channels_last():
    C, dst = 5, NR.SRC
    post = NR.posteriors(C).copy()
    post[2, 2, 2, :] = np.nan
    post[3, 3, 3, 0] = np.nan
    lut = NR.lut_for(C)
    xyz = NR.coords(EYE, dst)
    want, _ = NR.argmax_labels(post, lut, *xyz)
    ncdhw = T(np.ascontiguousarray(np.moveaxis(post, -1, 0)))[None]          # contiguous (1,C,D,H,W): converted once
    for p in (T(post).permute(3, 0, 1, 2)[None], ncdhw):
        lab = N.resample_labels(p, T(lut), EYE, dst, EYE)
        assert np.array_equal(lab.cpu().numpy(), want)
    assert want[2, 2, 2] == 0 and want[3, 3, 3] != 0


# ------------------------------------------------------------------------------------------------- containers
def test_rows_of_one_buffer_give_the_bits_of_separate_copies():
    dst, name, K = NR.DSTS[0], "rot_shear", 5
    src = NR.source(K)
    keys = ["T1", "T2", "label", "bias", "dist"]
    acc_buf = T(src)
    rows = {k: acc_buf[j] for j, k in enumerate(keys)}
    assert N._rows_of_one_buffer(list(rows.values()))[1] == int(np.prod(NR.SRC))
    copies = {k: v.clone() for k, v in rows.items()}
    assert N._rows_of_one_buffer(list(copies.values())) is None
    a = N.resample_maps(rows, EYE, dst, M4(dst, name))
    b = N.resample_maps(copies, EYE, dst, M4(dst, name))
    c = N.resample_maps(acc_buf, EYE, dst, M4(dst, name), nearest=(2,))
    assert list(a.keys()) == keys and type(a) is dict
    xyz = NR.coords(NR.matrices(dst)[name], dst)
    for j, k in enumerate(keys):
        want = NR.nearest(src[j], *xyz) if k == "label" else NR.linear_f32(src[j], *xyz)
        assert np.array_equal(bits(a[k]), bits(want)), k
        assert np.array_equal(bits(b[k]), bits(want)), k
        assert np.array_equal(bits(c[j]), bits(want)), k


# ------------------------------------------------------------------------------------------------- end to end
SHAPE = (20, 24, 18)


def _ramp(aff):
    """A function linear in world coordinates on the native grid, scaled to [0, 1]."""
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE], indexing="ij")
    w = [aff[r, 0] * i + aff[r, 1] * j + aff[r, 2] * k + aff[r, 3] for r in range(3)]
    f = 0.7 * w[0] - 0.4 * w[1] + 0.55 * w[2]
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


@pytest.mark.parametrize("win_size", [None, (14, 15, 13)])
def test_prepare_image_then_to_native_returns_the_scan(win_size):
    aff = _native_affine((2, 0, 1), (1, 0, 1), (0.8, 1.0, 1.3))
    vol = _ramp(aff)
    final, orig, _, _, aff_p, _, _ = TU.prepare_image((vol, aff), win_size=win_size, rescale=False, device=DEV)
    shape_p = tuple(final.shape[2:])
    if win_size is not None:
        assert shape_p != N.processed_grid(SHAPE, aff)[0]         # it did crop
    out = N.to_native({"T1": final}, aff_p, SHAPE, aff)
    assert list(out.keys()) == ["T1"] and out["T1"].shape == SHAPE
    got = out["T1"].cpu().numpy().astype(np.float64)
    # where to look: the trilinear footprint inside the processed volume, and the native voxel further from every border
    # of the scan than the Gaussian's half-width (ceil(2.5 sigma) = 2 on the 0.8 mm axis) plus 2
    M = N.vox2vox(N.processed_grid(SHAPE, aff, shape_p)[1], aff)
    p = NR.coords(M, SHAPE)
    inside = np.ones(SHAPE, dtype=bool)
    for c, n in zip(p, shape_p):
        inside &= (c >= 0) & (c <= n - 1)
    deep = np.zeros(SHAPE, dtype=bool)
    deep[4:-4, 4:-4, 4:-4] = True
    look = inside & deep
    assert look.sum() >= (600 if win_size is None else 200)
    err = np.abs(got - vol)[look].max()
    print("win_size %s: %d voxels, worst error %.3g of the range" % (win_size, int(look.sum()), err))
    assert err <= 1e-4                                            # the ramp's range is 1
    # `orig` is the output prepare_image does reorient: the same through the three-step grid (flip offsets included)
    shape_o = tuple(orig.shape[2:])
    aff_o = N.processed_grid(SHAPE, aff, shape_o, aligned=True)[1]
    got = N.resample_maps({"T1": orig[0, 0]}, aff_o, SHAPE, aff)["T1"].cpu().numpy().astype(np.float64)
    inside = np.ones(SHAPE, dtype=bool)
    for c, n in zip(NR.coords(N.vox2vox(aff_o, aff), SHAPE), shape_o):
        inside &= (c >= 0) & (c <= n - 1)
    look = inside & deep
    assert look.sum() >= 200
    err = np.abs(got - vol)[look].max()
    print("win_size %s, orig: %d voxels, worst error %.3g of the range" % (win_size, int(look.sum()), err))
    assert err <= 1e-4


def test_to_native_takes_labels_from_posteriors_or_from_the_label_map():
    aff = _native_affine((1, 2, 0), (0, 1, 0), (0.8, 1.0, 1.3))
    shape_p, aff_p = N.processed_grid(SHAPE, aff)                # the outputs' grid ...
    aff_ret = N.processed_grid(SHAPE, aff, aligned=True)[1]       # ... and the affine prepare_image returns
    C = 5
    rs = np.random.RandomState(3)
    post = rs.rand(1, C, *shape_p).astype(np.float32)
    dpost = T(post).to(memory_format=torch.channels_last_3d)
    lut = [0, 14, 15, 16, 24]
    stitched = T(np.asarray(lut, dtype=np.float32)[post[0].argmax(0)])
    outputs = {"T1": T(post[0, 0]), "segmentation": dpost, "label": stitched, "age": torch.zeros(1, 1, device=DEV),
               "feat": [T(post)]}
    res = N.to_native(outputs, aff_ret, SHAPE, aff, lut=lut)
    assert list(res.keys()) == ["T1", "label"] and res["label"].dtype == torch.int32
    want = N.resample_labels(dpost, lut, aff_p, SHAPE, aff)
    assert torch.equal(res["label"], want)
    forced = N.to_native(outputs, aff_ret, SHAPE, aff, label_from="label")
    near = N.resample_maps({"label": stitched}, aff_p, SHAPE, aff)["label"]
    assert forced["label"].dtype == torch.float32 and torch.equal(forced["label"], near)
    no_post = {k: v for k, v in outputs.items() if k != "segmentation"}
    assert torch.equal(N.to_native(no_post, aff_ret, SHAPE, aff)["label"], near)
    with pytest.raises(L.BfmError, match="no posteriors"):
        N.to_native(no_post, aff_ret, SHAPE, aff, label_from="segmentation")
    with pytest.raises(L.BfmError, match="match no shipped label list"):
        N.to_native(outputs, aff_ret, SHAPE, aff)


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    m = torch.zeros(NR.SRC, device=DEV)
    with pytest.raises(L.BfmError, match="not 3-D"):
        N.resample_maps({"T1": m[0]}, EYE, (3, 4, 5), EYE)
    with pytest.raises(L.BfmError, match=r"\(K,D,H,W\)"):
        N.resample_maps(m, EYE, (3, 4, 5), EYE)
    with pytest.raises(L.BfmError, match="not a 3-D map"):
        N.to_native({"T1": torch.zeros(2, 2, 3, 4, device=DEV)}, EYE, NR.SRC, EYE)
    with pytest.raises(L.BfmError, match="singular affine"):
        N.resample_maps({"T1": m}, np.diag([1.0, 0.0, 1.0, 1.0]), (3, 4, 5), EYE)
    with pytest.raises(L.BfmError, match="singular affine"):
        N.resample_labels(torch.zeros((1, 2) + NR.SRC, device=DEV), [0, 1], EYE, (3, 4, 5), np.zeros((4, 4)))
    with pytest.raises(L.BfmError, match="2 posterior channels but 3 labels"):
        N.resample_labels(torch.zeros((1, 2) + NR.SRC, device=DEV), [0, 1, 2], EYE, (3, 4, 5), EYE)
    with pytest.raises(L.BfmError, match="HIP device only"):
        N.resample_maps({"T1": m.cpu()}, EYE, (3, 4, 5), EYE)
    # a zero_crop_first=True result: the volume shrank, the affine did not move
    aff = _native_affine((2, 0, 1), (1, 0, 1), (0.8, 1.0, 1.3))
    vol = np.zeros(SHAPE, dtype=np.float32)
    vol[5:15, 6:18, 4:14] = 1.0
    final, _, _, _, aff_p, _, _ = TU.prepare_image((vol, aff), win_size=None, zero_crop_first=True, rescale=False,
                                                   device=DEV)
    assert tuple(final.shape[2:]) != N.processed_grid(SHAPE, aff)[0]
    with pytest.raises(L.BfmError, match="zero_crop_first"):
        N.to_native({"T1": final}, aff_p, SHAPE, aff)
