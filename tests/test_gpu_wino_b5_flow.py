"""Engine-level test of the conv_wino_b5 route of the batched levels (UNetEngine._deep_b5, variant 5): the 64-wide 6-level
net on tiles whose levels 2 and 3 are 20 and 10 voxels wide.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))


def test_wino_b5_route_is_batch_independent_and_agrees_with_the_routes_without_it():
    """Three 80^3 tiles, one half empty (levels 2 / 3 are 20^3 / 10^3), and one 80 x 80 x 160 tile (level 3 is 10 x 10 x 20):
    with the route on (the layers the committed tune table gives it), a sample's feature levels are bit-identical whether
    it runs alone, batched, or batched in reverse, and the route really ran -- plain and accumulating launches (the skip
    halves), at these levels.
    With the route off every level agrees within 2e-5 relative, the project's figure for two routes of different summation
    order (test_deep_levels_batched_over_tiles_equal_the_single_tile_path_bit_for_bit)."""
    from brainfm_amd.engine import UNetEngine
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    dev = torch.device("cuda:0")
    sd = O.random_state_dict(1, 64, 6, seed=3)
    eng = UNetEngine(sd, in_channels=1, f_maps=64, num_levels=6, device=dev)
    assert eng.has_deep_region()
    calls = []
    inner = eng._batch_launch

    def counted(ly, cfg, A, B, upp, dims, *a, **k):
        if cfg[6] == 5:
            calls.append((tuple(dims), cfg[7] & 1, A.shape[0]))
        return inner(ly, cfg, A, B, upp, dims, *a, **k)
    eng._batch_launch = counted
    g = torch.Generator().manual_seed(11)
    was = eng.use_wino_b5
    try:
        for dims, ntile, seen in (((80, 80, 80), 3, {(20, 20, 20), (10, 10, 10)}),
                                  ((80, 80, 160), 1, {(10, 10, 20)})):
            xs = [torch.rand(dims + (1,), generator=g).to(dev) for _ in range(ntile)]
            if ntile > 1:
                xs[1][: dims[0] // 2] = 0                           # a half-empty tile: constant input to GroupNorm
            eng.use_wino_b5 = "1"                                   # on: the layers the committed tune table gives it
            del calls[:]
            single = [eng.backbone_cl(x, dims) for x in xs]
            assert seen <= {c[0] for c in calls}, calls
            assert {0, 1} == {c[1] for c in calls} and all(c[2] == 1 for c in calls), calls
            del calls[:]
            batch = eng.backbone_batch(xs, dims)
            assert calls and all(c[2] == ntile for c in calls), calls
            rev = eng.backbone_batch(xs[::-1], dims)[::-1]
            for s_ in range(ntile):
                assert len(single[s_]) == len(batch[s_]) == 6
                for (a, da), (b, db), (c, dc) in zip(single[s_], batch[s_], rev[s_]):
                    assert da == db == dc and torch.equal(a, b) and torch.equal(a, c), (dims, s_, da)
            eng.use_wino_b5 = "0"
            del calls[:]
            old = eng.backbone_cl(xs[0], dims)
            assert not calls
            errs = [_relerr(a.cpu().numpy(), b.cpu().numpy()) for (a, da), (b, db) in zip(single[0], old)]
            print("wino_b5 route vs the routes without it, tile %s: relative difference per level %s"
                  % (dims, ["%.1e" % e for e in errs]))
            assert all(da == db for (_, da), (_, db) in zip(single[0], old)) and max(errs) <= 2e-5, (dims, errs)
    finally:
        eng.use_wino_b5 = was
