"""Engine-level test of the tap-wise GEMM route (UNetEngine._batch_conv_tap): the 64-wide 6-level net on tiles whose
deepest levels have 2^3 and 3 x 2 x 2 voxels.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))


def test_tap_route_is_batch_independent_and_agrees_with_the_conv_mfma_route():
    """Tiles of 80^3 (level 5 is 2^3, decoders.0.1 goes 2 -> 5) and 96 x 80 x 80 (3 x 2 x 2; mixed exact / 2 -> 5): with
    the route on, three samples are bit-identical whether they run alone, batched, or batched in reverse; with it off
    (the conv_mfma route of the same layers, another summation order) every feature level agrees within 2e-5 relative,
    the project's figure for two such routes (test_deep_levels_batched_over_tiles_equal_the_single_tile_path_bit_for_bit)."""
    from brainfm_amd.engine import UNetEngine
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    dev = torch.device("cuda:0")
    sd = O.random_state_dict(1, 64, 6, seed=3)
    eng = UNetEngine(sd, in_channels=1, f_maps=64, num_levels=6, device=dev)
    assert eng.has_deep_region() and eng.use_tap
    calls = []
    inner = eng._batch_conv_tap

    def counted(ly, *a, **k):
        calls.append(ly.name)
        return inner(ly, *a, **k)
    eng._batch_conv_tap = counted
    g = torch.Generator().manual_seed(9)
    for dims in ((80, 80, 80), (96, 80, 80)):
        xs = [torch.rand(dims + (1,), generator=g).to(dev) for _ in range(3)]
        xs[1][: dims[0] // 2] = 0                                   # a half-empty tile: constant input to GroupNorm
        del calls[:]
        single = [eng.backbone_cl(x, dims) for x in xs]
        assert len(calls) == 9 and sum("decoders.0" in n and n.endswith("SingleConv1") for n in calls) == 3, calls
        batch = eng.backbone_batch(xs, dims)
        rev = eng.backbone_batch(xs[::-1], dims)[::-1]
        for s_ in range(3):
            assert len(single[s_]) == len(batch[s_]) == 6
            for (a, da), (b, db), (c, dc) in zip(single[s_], batch[s_], rev[s_]):
                assert da == db == dc and torch.equal(a, b) and torch.equal(a, c), (dims, s_, da)
        eng.use_tap = False
        try:
            del calls[:]
            old = eng.backbone_cl(xs[0], dims)
            assert not calls
        finally:
            eng.use_tap = True
        errs = [_relerr(a.cpu().numpy(), b.cpu().numpy()) for (a, da), (b, db) in zip(single[0], old)]
        print("tap route vs conv_mfma route, tile %s: relative difference per level %s" % (dims, ["%.1e" % e for e in errs]))
        assert all(da == db for (_, da), (_, db) in zip(single[0], old)) and max(errs) <= 2e-5, (dims, errs)
