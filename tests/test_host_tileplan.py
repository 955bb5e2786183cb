"""plan_exchange: the host-only arithmetic behind both tile flows (who owns a tile, its round and offset, the buffer sizes),
checked from plain numbers: no device, no process group."""
import pytest

from brainfm_amd import test_utils as TU

LISTS = {27: TU.tiling_ranges((32,) * 3, [10] * 3, [20] * 3), 216: TU.tiling_ranges((64,) * 3, [10] * 3, [20] * 3)}
NKEYS = 3


def _pattern(ranges, name):
    """(width, live): dense rows; compact rows where every third tile keeps nothing (and is not run); dense rows with
    every fourth tile switched off although it has columns."""
    cost = [TU.tile_cost(r) for r in ranges]
    if name == "dense":
        return cost, [True] * len(ranges)
    if name == "compact":
        width = [c * (i % 3) // 2 for i, c in enumerate(cost)]
        return width, [w > 0 for w in width]
    return cost, [i % 4 != 1 for i in range(len(ranges))]


@pytest.mark.parametrize("pattern", ["dense", "compact", "dead"])
@pytest.mark.parametrize("nlanes", [1, 2])
@pytest.mark.parametrize("rounds", [True, False])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("ntiles", [27, 216])
def test_plan_gives_every_live_tile_one_slot_and_sizes_the_rounds(ntiles, world, rounds, nlanes, pattern):
    ranges = LISTS[ntiles]
    assert len(ranges) == ntiles
    width, live = _pattern(ranges, pattern)
    plan = TU.plan_exchange(ranges, world, rounds, nlanes, NKEYS, width, live)
    assert plan.owner == TU.assign_tiles(ranges, world)
    assert len(plan.batches_of) == world
    nrounds = len(plan.round_numel)
    assert len(plan.own_numel) == nrounds
    assert nrounds == (max([len(b) for b in plan.batches_of] + [1]) if rounds else 1)
    seen = []
    fills = []
    for r, batches in enumerate(plan.batches_of):
        mine = [i for i in range(ntiles) if plan.owner[i] == r and live[i]]
        assert batches == TU.tile_batches(ranges, mine, min_batches=nlanes)
        fill = [0] * nrounds
        for k, batch in enumerate(batches):
            kk = k if rounds else 0
            for i in batch:                                   # batch order, back to back: disjoint within (rank, round)
                assert (plan.round_of[i], plan.off_of[i]) == (kk, fill[kk]), i
                fill[kk] += width[i] * NKEYS
                seen.append(i)
        fills.append(fill)
    assert sorted(seen) == [i for i in range(ntiles) if live[i]]           # exactly one slot per live tile
    for i in range(ntiles):
        if not live[i]:
            assert (plan.round_of[i], plan.off_of[i]) == (0, 0)
    for k in range(nrounds):
        assert plan.own_numel[k] == max(1, fills[0][k])
        assert plan.round_numel[k] == max([1] + [f[k] for f in fills[1:]])


# what tiled_inference_distributed reported through stats= before the plan was its own function (gloo, the stand-in ops of
# test_host_cpu.py with 3 keys, dense rows, no session and so one lane): rounds, round_bytes_per_peer, bytes_sent_per_peer
RECORDED = [
    (27, 8, True, 1, [96000], 96000),
    (27, 8, False, 1, [96000], 96000),
    (27, 2, True, 5, [96000, 96000, 96000, 4, 4], 288008),
    (27, 2, False, 1, [288000], 288000),
    (27, 3, True, 3, [96000, 96000, 96000], 288000),
    (27, 3, False, 1, [288000], 288000),
    (216, 8, True, 6, [168000, 144000, 240000, 144000, 84000, 84000], 864000),
    (216, 8, False, 1, [576000], 576000),
    (216, 3, True, 12, [168000, 168000, 168000, 144000, 144000, 144000, 144000, 144000, 240000, 240000, 144000, 144000],
     1992000),
]


@pytest.mark.parametrize("ntiles,world,rounds,nrounds,round_bytes,sent", RECORDED)
def test_plan_reproduces_the_recorded_exchange_sizes(ntiles, world, rounds, nrounds, round_bytes, sent):
    ranges = LISTS[ntiles]
    plan = TU.plan_exchange(ranges, world, rounds, 1, NKEYS, [TU.tile_cost(r) for r in ranges], [True] * ntiles)
    assert len(plan.round_numel) == nrounds
    assert [4 * v for v in plan.round_numel] == round_bytes
    assert 4 * sum(plan.round_numel) == sent
