"""Uniform-box class mates are stored only where a later kernel reads them.  The flag buffer ends with a `need` table (a mate
with a computed box among its 26 neighbours); class_fill and the accumulating conv_wino4d_uniform store a mate's box of
`out` by that table when bit 1 of the flag argument is set, and the engine asks for it when the tensor's only reader takes the
uniform-box pair on the same flags.  Every stored voxel and every moment row holds the bits of the full launch.

The input is the volume of test_uniform_background_boxes_change_no_bit (an off-centre ellipsoid of rand + 0.05, zero
outside): at level 0 it has unflagged boxes, mates with `need` and mates without; each test asserts the three counts."""
import ctypes as C

import numpy as np
import pytest
import torch

import uniform_need_refs as R

pytestmark = pytest.mark.gpu

PASSES = 3
LEVELS = ((0, 3), (1, 8))          # (level, radius): the engine's, one set of flags per level


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _box(lib, L, ld):
    box = (C.c_int * 3)()
    L.check(lib.bfm_conv3x3x3_wino_box(ld[0], ld[1], ld[2], PASSES, box), "box")
    return tuple(box)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


_KINDS = {}


def _kinds(dims, lvl, rad):
    """numpy: (flags, grid, box, need, computed) of the ellipsoid volume, once per case; asserts at level 0 that unflagged
    boxes, mates with need and mates without are all present."""
    key = (dims, lvl, rad)
    if key not in _KINDS:
        L, lib = _lib()
        ld = tuple(v >> lvl for v in dims)
        box = _box(lib, L, ld)
        fl, nt = R.flags(R.ellipsoid_volume(dims).numpy(), dims, box, lvl, rad)
        nd, comp = R.need(fl, nt)
        _KINDS[key] = (fl, nt, box, nd, comp)
    fl, nt, box, nd, comp = _KINDS[key]
    if lvl == 0:
        assert int((fl == 0).sum()) > 0 and int(nd.sum()) > 0 and int(((nd == 0) & ~comp).sum()) > 0
    return _KINDS[key]


def _flag_buffer(img, dims, lvl, rad):
    L, lib = _lib()
    D, H, W = dims
    buf = torch.full((lib.bfm_uniform_boxes_bytes(D >> lvl, H >> lvl, W >> lvl, PASSES),), 0xAB, dtype=torch.uint8, device=img.device)
    L.check(lib.bfm_uniform_boxes_level(L.ptr(img), D, H, W, lvl, rad, PASSES, L.ptr(buf), L.stream_ptr()), "flags")
    return buf


@pytest.mark.parametrize("dims", [(48, 64, 128), (50, 66, 130)])
def test_need_table_equals_the_rule(dims):
    """need[], the need list and its count are the numpy restatement at levels 0 (radius 3) and 1 (radius 8), from the
    per-level call and from the one-launch call alike; the flag bytes, first[27], the counts and both lists stay what
    they were."""
    L, lib = _lib()
    dev = _dev()
    D, H, W = dims
    img = R.ellipsoid_volume(dims).to(dev)
    one = [_flag_buffer(img, dims, lvl, rad) for lvl, rad in LEVELS]
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    both = [torch.full_like(b, 0xAB) for b in one]
    L.check(lib.bfm_uniform_boxes_levels(L.ptr(img), D, H, W, 2, (C.c_int * 2)(*[l for l, _ in LEVELS]),
                                         (C.c_int * 2)(*[r for _, r in LEVELS]), PASSES,
                                         (C.c_void_p * 2)(*[b.data_ptr() for b in both]), L.ptr(ticket), L.stream_ptr()), "levels")
    torch.cuda.synchronize()
    assert int(ticket.item()) == 0
    for (lvl, rad), a, b in zip(LEVELS, one, both):
        assert torch.equal(a, b), lvl                          # byte for byte, unwritten slots (0xAB) included
        fl, nt, box, nd, comp = _kinds(dims, lvl, rad)
        n = fl.size
        got = R.parse(a.cpu().numpy(), n)
        assert np.array_equal(got["flags"], fl), lvl
        assert np.array_equal(got["first"], R.first_boxes(fl)), lvl
        rest, uni = np.flatnonzero(comp), np.flatnonzero(~comp)
        assert tuple(got["counts"]) == (rest.size, uni.size)
        assert np.array_equal(got["rest"][:rest.size], rest) and np.array_equal(got["uniform"][:uni.size], uni)
        assert np.array_equal(got["need"], nd), lvl
        want = np.flatnonzero(nd)
        assert got["need_count"] == want.size
        assert np.array_equal(got["need_list"][:want.size], want), lvl


class _Conv:
    """Operands of one conv layer on the ellipsoid volume at (48, 64, 128): the input is a per-channel affine map of the
    image, so it is one vector wherever the image is constant, which is what the flags promise."""

    dims = (48, 64, 128)

    def __init__(self, cin, cout, family, background=0.0):
        L, lib = _lib()
        self.L, self.lib, self.cin, self.cout, self.family = L, lib, cin, cout, family
        dev = _dev()
        D, H, W = self.dims
        g = torch.Generator().manual_seed(5)
        img = R.ellipsoid_volume(self.dims)
        if background:
            img = torch.where(img == 0, torch.full_like(img, background), img)
        a = torch.rand(cin, generator=g) + 0.5
        b = torch.randn(cin, generator=g) * 0.3
        self.A = (img[..., None] * a + b).contiguous().to(dev)
        self.img = img.contiguous().to(dev)
        w = (torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.05).to(dev).contiguous()
        self.scale = (torch.rand(cin, generator=g) + 0.5).to(dev)
        self.shift = (torch.randn(cin, generator=g) * 0.1).to(dev)
        self.bound = torch.full((8,), 6.0, device=dev)
        nbytes, pack = ((lib.bfm_pack_conv_weights_wino_bytes, lib.bfm_pack_conv_weights_wino) if family == 3 else
                        (lib.bfm_pack_conv_weights_wino4_bytes, lib.bfm_pack_conv_weights_wino4))
        self.wp = torch.empty(nbytes(cin, cout, PASSES), dtype=torch.uint8, device=dev)
        wexp = C.c_int(0)
        L.check(pack(L.ptr(w), cin, cout, float(w.abs().max()), PASSES, L.ptr(self.wp), C.byref(wexp), L.stream_ptr()), "pack")
        self.wexp = wexp.value
        self.nrows = lib.bfm_conv3x3x3_wino_rows(D, H, W, PASSES)
        self.flags = _flag_buffer(self.img, self.dims, 0, 3)
        scratch = lib.bfm_conv3x3x3_wino_uniform_scratch if family == 3 else lib.bfm_conv3x3x3_wino4_uniform_scratch
        self.scratch = torch.empty(scratch(cout), dtype=torch.uint8, device=dev)
        self.prior = torch.randn((D, H, W, cout), generator=g).to(dev)

    def run(self, bits, pool=False, keep=None):
        """One launch of the pair with this flag argument; `out` starts as NaN, or as the prior when it accumulates."""
        L, lib, dev = self.L, self.lib, self.A.device
        D, H, W = self.dims
        cout, st = self.cout, L.stream_ptr()
        out = self.prior.clone() if bits & 1 else torch.full((D, H, W, cout), float("nan"), device=dev)
        rows = torch.zeros(lib.bfm_moment_rows_bytes(self.nrows, cout), dtype=torch.uint8, device=dev)
        pooled = prow = None
        common = (L.ptr(self.A), self.cin, D, H, W, L.ptr(self.scale), L.ptr(self.shift), L.ptr(self.bound), 8, L.ptr(self.wp),
                  self.wexp, cout, 0.01, PASSES, bits, L.ptr(out), L.ptr(rows), L.ptr(self.flags), L.ptr(self.scratch))
        if pool:
            pooled = torch.full((D // 2, H // 2, W // 2, cout), float("nan"), device=dev)
            prow = torch.zeros(lib.bfm_moment_rows_bytes(self.nrows, cout), dtype=torch.uint8, device=dev)
            rc = lib.bfm_conv3x3x3_wino_uniform_pool(*common, L.ptr(pooled), L.ptr(prow), st)
        elif keep is not None:
            rc = lib.bfm_conv3x3x3_wino4_uniform_keep(*common, L.ptr(keep), st)
        elif self.family == 3:
            rc = lib.bfm_conv3x3x3_wino_uniform(*common, st)
        else:
            rc = lib.bfm_conv3x3x3_wino4_uniform(*common, st)
        L.check(rc, "conv")
        torch.cuda.synchronize()
        return out, rows, pooled, prow

    def stored(self):
        """(D,H,W) bool on the device: the voxels a launch by need stores -- computed boxes and mates with need."""
        fl, nt, box, nd, comp = _kinds(self.dims, 0, 3)
        assert np.array_equal(self.flags[:fl.size].cpu().numpy(), fl)
        return torch.from_numpy(R.box_mask(comp | (nd != 0), nt, box, self.dims)).to(self.A.device)


@pytest.mark.parametrize("pool", [False, True])
def test_class_fill_by_need(pool):
    """32 -> 64 F(2,3), plain and with the fused pooling, `out` pre-filled with NaN: computed boxes and mates with need hold
    the full launch's bits, mates without need are still NaN, the pooled tensor and both moment tables are equal."""
    ly = _Conv(32, 64, 3)
    assert ly.lib.bfm_conv3x3x3_wino_pool_ok(*ly.dims, PASSES) == 1
    full = ly.run(0, pool=pool)
    need = ly.run(2, pool=pool)
    assert not bool(torch.isnan(full[0]).any())
    st = ly.stored()
    assert torch.equal(_bits(need[0][st]), _bits(full[0][st]))
    assert bool(torch.isnan(need[0][~st]).all())
    for a, b in zip(need[1:], full[1:]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(_bits(a), _bits(b))
    # the completion the engine falls back to for a reader that looks everywhere: the full launch's tensor
    D, H, W = ly.dims
    ly.L.check(ly.lib.bfm_uniform_fill(ly.L.ptr(need[0]), D, H, W, 64, PASSES, ly.L.ptr(ly.flags), ly.L.stream_ptr()), "fill")
    torch.cuda.synchronize()
    assert torch.equal(_bits(need[0]), _bits(full[0]))


def test_accumulating_f43_pair_by_need():
    """64 -> 64 F(4,3) accumulating onto a random prior: stored boxes and all moment rows equal the full launch, skipped
    boxes still hold the prior.  For a masked reader (_keep) a background that is zero stores the same boxes, and one that
    is not zero stores them all."""
    ly = _Conv(64, 64, 4)
    full = ly.run(1)
    need = ly.run(3)
    st = ly.stored()
    assert torch.equal(need[0][st], full[0][st])
    assert torch.equal(need[0][~st], ly.prior[~st])
    assert not torch.equal(full[0][~st], ly.prior[~st])
    assert torch.equal(need[1], full[1])
    keep = ly.run(3, keep=ly.img)
    assert torch.equal(keep[0], need[0]) and torch.equal(keep[1], full[1])
    bg = _Conv(64, 64, 4, background=0.37)
    assert int(bg.flags[:bg.nrows].count_nonzero()) > 100
    full, keep, need = bg.run(1), bg.run(3, keep=bg.img), bg.run(3)
    assert torch.equal(keep[0], full[0]) and torch.equal(keep[1], full[1])
    assert not torch.equal(need[0], full[0])
    # the F(2,3) accumulate form and the F(4,3) form without accumulation store every box, with bit 1 or without
    assert torch.equal(_bits(ly.run(2)[0]), _bits(ly.run(0)[0]))
    f23 = _Conv(64, 64, 3)
    assert torch.equal(f23.run(3)[0], f23.run(1)[0])


def _session(ver, monkeypatch):
    from brainfm_amd import test_utils as TU
    monkeypatch.setenv("BFM_CONV_VER", str(ver))
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=3)
    torch.manual_seed(4)
    return TU, TU.InferenceSession(ga, ta, _dev(), passes=PASSES)


def _spy(eng):
    """Counts the launches by need of an engine: [for the pair, for the masked reader]."""
    seen = [0, 0]
    inner = eng._conv_launch

    def launch(*a, **kw):
        nd = kw.get("need")
        if nd is not None:
            seen[0 if nd is True else 1] += 1
        return inner(*a, **kw)
    eng._conv_launch = launch
    return seen


@pytest.mark.parametrize("ver", [3, 4])
@pytest.mark.parametrize("dims", [(48, 64, 128), (50, 66, 130)])
def test_flow_by_need_changes_no_bit(dims, ver, monkeypatch):
    """forward_fused on the 3-level, 64-wide net, stores by need with the skipped boxes poisoned against every box stored:
    every decoder feature map, every tail map and the labels are equal.  No mask is in play, so the last decoder's first
    conv stores in full."""
    _kinds(dims, 0, 3)
    x = R.ellipsoid_volume(dims)[None, None].to(_dev())
    outs = {}
    for need in (True, False):
        TU, s = _session(ver, monkeypatch)
        s.engine.uniform_need, s.engine.poison_skipped = need, need
        seen = _spy(s.engine)
        outs[need], _ = s.forward_fused(x)
        assert seen[1] == 0
        assert (seen[0] > 0) == need, seen
    for k in outs[True]:
        if k == "feat":
            for a, b in zip(outs[True][k], outs[False][k]):
                assert torch.equal(a, b)
        else:
            assert torch.equal(outs[True][k], outs[False][k]), k


def test_flow_by_need_with_the_tune_table_choices(monkeypatch):
    """No variant pinned: at 80^3 the committed tune table settles the first two levels' shapes (F(2,3) producers, the last
    decoder's skip half on F(4,3)), which is how the default flow learns its readers' kernels before they run
    (engine._settled_variant's table branch).  Stores by need are made, and no output bit moves."""
    from brainfm_amd import test_utils as TU
    from brainfm_amd import engine as E
    monkeypatch.delenv("BFM_CONV_VER", raising=False)
    monkeypatch.delenv("BFM_CONV_TUNE", raising=False)
    dims = (80, 80, 80)
    dev = torch.cuda.current_device()
    assert E._tune_lookup(dev, PASSES, (32, 64, dims, False, False)) == 3
    assert E._tune_lookup(dev, PASSES, (64, 64, dims, False, True)) == 4
    x = R.ellipsoid_volume(dims)[None, None].to(_dev())
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=3)
    outs = {}
    for need in (True, False):
        torch.manual_seed(4)
        s = TU.InferenceSession(ga, ta, _dev(), passes=PASSES)
        s.engine.uniform_need, s.engine.poison_skipped = need, need
        seen = _spy(s.engine)
        outs[need], _ = s.forward_fused(x)
        assert (seen[0] > 0) == need and seen[1] == 0, seen
        assert s.engine.need_completed == 0
    for k in outs[True]:
        if k == "feat":
            for a, b in zip(outs[True][k], outs[False][k]):
                assert torch.equal(a, b)
        else:
            assert torch.equal(outs[True][k], outs[False][k]), k


def test_tile_flow_by_need_changes_no_bit(monkeypatch):
    """tiled_inference of a 96^3 volume, window 64, stride 32 (the last convolution runs masked, so the last decoder's first
    conv stores for it by need where it runs F(4,3)): all stitched keys are equal to the run with every box stored."""
    vol = R.ellipsoid_volume((96, 96, 96))
    full = vol[None, None].to(_dev())
    outs, seen = {}, {}
    for need in (True, False):
        TU, s = _session(4, monkeypatch)
        s.engine.uniform_need, s.engine.poison_skipped = need, need
        seen[need] = _spy(s.engine)
        acc, _, _ = TU.tiled_inference(full, s, [32] * 3, [64] * 3, graphs=False)
        outs[need] = {k: v.clone() for k, v in acc.items()}
    assert seen[True][0] > 0 and seen[True][1] > 0 and seen[False] == [0, 0]
    assert set(outs[True]) == set(outs[False])
    for k in outs[True]:
        assert torch.equal(outs[True][k], outs[False][k]), k


def test_a_tensor_stored_by_need_refuses_another_reader(monkeypatch):
    """encoders.1's first conv stores by need for its second; handed to that layer forced onto another variant
    (BFM_CONV_VER=0), or to it without the flags, the engine raises instead of reading boxes that were never written."""
    from brainfm_amd import _lib as L
    dims = (48, 64, 128)
    TU, s = _session(3, monkeypatch)
    eng = s.engine
    x_cl = eng.to_cl(R.ellipsoid_volume(dims)[None, None].to(_dev()))
    eng._uf_cache = {}
    (l1, l2), (m1, m2) = eng.enc[0], eng.enc[1]
    f0 = eng._layer_flags(("enc", 0, 1), x_cl, dims)
    t = eng.single_conv(l2, eng.single_conv(l1, x_cl, dims), dims, uni_flags=f0, pool=True)
    p, d = eng.maxpool(t, dims)
    f1 = eng._layer_flags(("enc", 1, 0), x_cl, dims)
    y = eng.single_conv(m1, p, d, uni_flags=f1, reader=("conv", m2, f1))
    assert getattr(y, "_bfm_need", None) is not None and y._bfm_need[0] is f1
    assert getattr(t, "_bfm_need", None) is None               # no reader named: stored in full
    with pytest.raises(L.BfmError, match="stored by need"):
        eng.single_conv(m2, y, d)                                # the dense launch
    monkeypatch.setenv("BFM_CONV_VER", "0")
    eng._plan_cache.clear()
    eng._tuned.clear()
    with pytest.raises(L.BfmError, match="stored by need"):
        eng.single_conv(m2, y, d, uni_flags=f1)
    monkeypatch.setenv("BFM_CONV_VER", "3")
    eng._plan_cache.clear()
    want = eng.single_conv(m2, y, d, uni_flags=f1)               # the reader it was stored for
    assert eng.need_completed == 0
    eng._complete(y, d)
    assert y._bfm_need is None and eng.need_completed == 1
    assert torch.equal(eng.single_conv(m2, y, d), want)          # completed: any reader
    torch.cuda.synchronize()
