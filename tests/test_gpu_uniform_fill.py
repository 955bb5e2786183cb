"""The uniform-box pair of the F(2,3) kernel without accumulation: the class mates of a flagged box are filled by class_fill,
a copy of their representative's box, pooled box and moment rows (conv3d_wino.hip).  Every tensor must hold the bits of the
dense entry point on the same inputs; the accumulating form keeps the epilogue replay and must equal the dense
accumulating launch."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

RADIUS = 2             # the layer input below is a voxel-wise function of the image: constant within 1 voxel would do

# (cin, cout, dims, pooled)
CASES = {
    "pooled_32_64": (32, 64, (40, 40, 20), True),        # box 8 x 8 x 4: 5 x 5 x 5 boxes, all 27 classes
    "ragged_64_64": (64, 64, (36, 30, 18), False),       # last boxes cut by the far faces
    "two_cout_tiles_64_128": (64, 128, (40, 40, 20), True),
}
IMAGES = ("blob", "constant", "random")


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _image(kind, dims, g):
    D, H, W = dims
    if kind == "random":
        return torch.rand(dims, generator=g)
    img = torch.full(dims, 0.37)
    if kind == "blob":
        z, y, x = D // 2, H // 2, W // 2
        img[z - 4:z + 4, y - 4:y + 4, x - 2:x + 2] = torch.rand((8, 8, 4), generator=g)
    return img


class _Layer:
    """One conv layer's operands on the device: the input is a per-channel affine map of the image, so it is one vector
    wherever the image is constant, which is what the flags promise."""

    def __init__(self, case, kind, passes):
        from brainfm_amd import _lib as L
        self.L, self.lib, self.passes = L, L.load(), passes
        lib, dev = self.lib, _dev()
        self.cin, self.cout, self.dims, self.pooled = CASES[case]
        cin, cout = self.cin, self.cout
        D, H, W = self.dims
        g = torch.Generator().manual_seed(5)
        img = _image(kind, self.dims, g)
        a = torch.rand(cin, generator=g) + 0.5
        b = torch.randn(cin, generator=g) * 0.3
        self.A = (img[..., None] * a + b).contiguous().to(dev)
        self.img = img.to(dev)
        w = (torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.05).to(dev).contiguous()
        self.scale = (torch.rand(cin, generator=g) + 0.5).to(dev)
        self.shift = (torch.randn(cin, generator=g) * 0.1).to(dev)
        self.bound = torch.full((8,), 6.0, device=dev)
        self.wp = torch.empty(lib.bfm_pack_conv_weights_wino_bytes(cin, cout, passes), dtype=torch.uint8, device=dev)
        wexp = C.c_int(0)
        L.check(lib.bfm_pack_conv_weights_wino(L.ptr(w), cin, cout, float(w.abs().max()), passes, L.ptr(self.wp), C.byref(wexp),
                                               L.stream_ptr()), "pack")
        self.wexp = wexp.value
        self.nrows = lib.bfm_conv3x3x3_wino_rows(D, H, W, passes)
        if self.pooled:
            assert lib.bfm_conv3x3x3_wino_pool_ok(D, H, W, passes) == 1
        self.flags = torch.empty(lib.bfm_uniform_boxes_bytes(D, H, W, passes), dtype=torch.uint8, device=dev)
        L.check(lib.bfm_uniform_boxes_level(L.ptr(self.img), D, H, W, 0, RADIUS, passes, L.ptr(self.flags), L.stream_ptr()), "flags")
        self.scratch = torch.empty(lib.bfm_conv3x3x3_wino_uniform_scratch(cout), dtype=torch.uint8, device=dev)
        self.prev = torch.randn((D, H, W, cout), generator=g).to(dev)      # what `out` holds before an accumulating launch

    def counts(self):
        """(flagged boxes, class mates) of the flag buffer."""
        n = self.nrows
        tail = self.flags[(n + 3) // 4 * 4:].view(torch.int32)
        return int((self.flags[:n] != 0).sum()), int(tail[28])

    def run(self, uniform, accumulate=False):
        L, lib, dev = self.L, self.lib, self.A.device
        D, H, W = self.dims
        cout, st = self.cout, L.stream_ptr()
        out = self.prev.clone() if accumulate else torch.full((D, H, W, cout), float("nan"), device=dev)
        rows = torch.zeros(lib.bfm_moment_rows_bytes(self.nrows, cout), dtype=torch.uint8, device=dev)
        pooled = prow = None
        if self.pooled:
            pooled = torch.full((D // 2, H // 2, W // 2, cout), float("nan"), device=dev)
            prow = torch.zeros(lib.bfm_moment_rows_bytes(self.nrows, cout), dtype=torch.uint8, device=dev)
        common = (L.ptr(self.A), self.cin, D, H, W, L.ptr(self.scale), L.ptr(self.shift), L.ptr(self.bound), 8, L.ptr(self.wp),
                  self.wexp, cout, 0.01, self.passes, 1 if accumulate else 0, L.ptr(out), L.ptr(rows))
        if uniform and self.pooled:
            rc = lib.bfm_conv3x3x3_wino_uniform_pool(*common, L.ptr(self.flags), L.ptr(self.scratch), L.ptr(pooled), L.ptr(prow), st)
        elif uniform:
            rc = lib.bfm_conv3x3x3_wino_uniform(*common, L.ptr(self.flags), L.ptr(self.scratch), st)
        elif self.pooled:
            rc = lib.bfm_conv3x3x3_wino_pool(*common, L.ptr(pooled), L.ptr(prow), st)
        else:
            rc = lib.bfm_conv3x3x3_wino_ex(*common, st)
        L.check(rc, "conv")
        torch.cuda.synchronize()
        return out, rows, pooled, prow


def _same(got, want):
    names = ("out", "moment rows", "pooled", "pooled moment rows")
    for name, a, b in zip(names, got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            # NaN != NaN under torch.equal: compare the bits
            ai = a.view(torch.int32) if a.dtype == torch.float32 else a
            bi = b.view(torch.int32) if b.dtype == torch.float32 else b
            assert torch.equal(ai, bi), name


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("case", list(CASES))
def test_class_fill_gives_the_dense_launch_bits(case, kind, passes):
    """out, the pooled tensor and both moment tables of the uniform pair equal the dense entry point's, for an image with a
    blob (mates in the classes around it), a constant image (every box flagged) and a random one (no box flagged)."""
    ly = _Layer(case, kind, passes)
    nboxes = ly.nrows
    flagged, mates = ly.counts()
    classes = int(torch.unique(ly.flags[:nboxes][ly.flags[:nboxes] != 0]).numel())
    assert mates == flagged - classes
    if kind == "random":
        assert flagged == 0
    elif kind == "constant":
        assert flagged == nboxes and mates > 0
    else:
        assert 0 < flagged < nboxes and mates > 0
    want = ly.run(uniform=False)
    assert not bool(torch.isnan(want[0]).any())
    _same(ly.run(uniform=True), want)


@pytest.mark.parametrize("case", ["pooled_32_64", "ragged_64_64"])
def test_accumulating_pair_still_equals_the_dense_accumulating_launch(case):
    """flags & 1: a mate adds its own voxels of `out`, so nothing may be copied from the representative."""
    ly = _Layer(case, "blob", 3)
    assert ly.counts()[1] > 0
    want = ly.run(uniform=False, accumulate=True)
    got = ly.run(uniform=True, accumulate=True)
    _same(got, want)
    assert not torch.equal(got[0], ly.run(uniform=True)[0])


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("dims", [(40, 40, 24), (48, 40, 40)])
def test_one_launch_flags_equal_the_per_level_calls(dims, passes):
    """bfm_uniform_boxes_levels for levels {0, 1} with the engine's radii: every byte of both flag buffers (flags, first
    boxes, counts, both lists) is what bfm_uniform_boxes_level writes for that level; the ticket is left zero, so the call
    can be repeated."""
    from brainfm_amd import _lib as L
    from brainfm_amd.engine import UNetEngine
    lib, dev = L.load(), _dev()
    D, H, W = dims
    levels = sorted({k[1] for k in UNetEngine.UNIFORM_RADIUS})
    radii = [max(r for k, r in UNetEngine.UNIFORM_RADIUS.items() if k[1] == l) for l in levels]
    assert levels == [0, 1]
    g = torch.Generator().manual_seed(3)
    for kind in IMAGES:
        img = _image(kind, dims, g).to(dev)
        sizes = [lib.bfm_uniform_boxes_bytes(D >> l, H >> l, W >> l, passes) for l in levels]
        assert min(sizes) > 0
        want = [torch.full((n,), 0xAB, dtype=torch.uint8, device=dev) for n in sizes]
        for l, r, b in zip(levels, radii, want):
            L.check(lib.bfm_uniform_boxes_level(L.ptr(img), D, H, W, l, r, passes, L.ptr(b), L.stream_ptr()), "level")
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(2):
            got = [torch.full((n,), 0xAB, dtype=torch.uint8, device=dev) for n in sizes]
            L.check(lib.bfm_uniform_boxes_levels(L.ptr(img), D, H, W, len(levels), (C.c_int * 2)(*levels), (C.c_int * 2)(*radii),
                                                 passes, (C.c_void_p * 2)(*[b.data_ptr() for b in got]), L.ptr(ticket),
                                                 L.stream_ptr()), "levels")
            torch.cuda.synchronize()
            assert int(ticket.item()) == 0
            for l, a, b in zip(levels, got, want):
                assert torch.equal(a, b), (kind, l)
        if kind == "constant":
            assert int((want[0][:8] != 0).sum()) == 8
