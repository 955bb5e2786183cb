"""The host-built (output voxel, tap) -> low-res row table of the tap-wise GEMM route (engine.tap_row_table, read by
bfm_tap_sum_batch): summing the per-tap products P[tap][row] through it is the 3x3x3 zero-padded conv over the
nearest-upsampled tensor.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from brainfm_amd.engine import nearest_index_map, tap_row_table

CASES = [((2, 2, 2), (5, 5, 5)), ((5, 2, 2), (10, 5, 5)), ((2, 5, 5), (5, 10, 10)), ((2, 2, 3), (4, 4, 6)),
         ((2, 2, 2), (2, 2, 2)), ((5, 2, 2), (5, 2, 2)), ((5, 5, 2), (5, 5, 2)), ((1, 2, 1), (1, 2, 1))]


@pytest.mark.parametrize("lo,hi", CASES)
def test_tap_table_sum_equals_conv3d_of_the_nearest_upsample(lo, hi):
    """sum_tap P[tap][table[o][tap]] with P[tap][v] = W[tap] . y[v] in float64 == F.conv3d(nearest_up(y), w, padding=1)
    to 1e-12 relative; the upsample is built from nearest_index_map, the function the engine uses (and equals
    F.interpolate(mode='nearest'))."""
    cin, cout = 5, 4
    g = torch.Generator().manual_seed(sum(lo) + 7 * sum(hi))
    y = torch.randn(lo + (cin,), generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64)
    maps = [torch.from_numpy(nearest_index_map(lo[a], hi[a])).long() for a in range(3)]
    up = y[maps[0]][:, maps[1]][:, :, maps[2]]                                 # (D, H, W, cin)
    assert torch.equal(up.permute(3, 0, 1, 2)[None],
                       F.interpolate(y.permute(3, 0, 1, 2)[None], size=hi, mode="nearest"))
    want = F.conv3d(up.permute(3, 0, 1, 2)[None], w, padding=1)[0].permute(1, 2, 3, 0).reshape(-1, cout)
    tab = torch.from_numpy(tap_row_table(lo, hi)).long()
    n_lo, n_hi = lo[0] * lo[1] * lo[2], hi[0] * hi[1] * hi[2]
    assert tuple(tab.shape) == (n_hi, 27) and int(tab.min()) >= -1 and int(tab.max()) < n_lo
    P = torch.einsum("vc,oct->tvo", y.reshape(n_lo, cin), w.reshape(cout, cin, 27))   # [tap][row][cout]
    got = torch.zeros(n_hi, cout, dtype=torch.float64)
    for tap in range(27):
        r = tab[:, tap]
        got += torch.where((r >= 0)[:, None], P[tap][r.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-12, err
    if lo == hi:                                                               # identity map: interior voxels drop no tap
        inner = [(tab[i] >= 0).all() for i in range(n_hi)]
        assert sum(bool(v) for v in inner) == max(hi[0] - 2, 0) * max(hi[1] - 2, 0) * max(hi[2] - 2, 0)
