"""What each rank of an N-rank run of the 256^3 volume computes, timed alone on ONE GPU (no transfers): its batches of
same-shape tiles on its two lanes as tiled_inference_distributed runs them (its plan_exchange and _run_batches, one
round), plus -- on rank 0 -- the stitch of all 27 tiles.
A model of the N-GPU step without the exchange: max over ranks.   python scripts/bench_rank_share.py [N=8] [size=256]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from brainfm_amd import test_utils as TU  # noqa: E402

world = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = torch.device("cuda", 0)
torch.manual_seed(1)
ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
sess = TU.InferenceSession(ga, ta, dev, passes=3)
sess.use_graphs = True
full = bench.make_volume(n, dev)
stride, win = [80] * 3, [160] * 3
ranges = TU.tiling_ranges((n, n, n), stride, win)
ops = sess.stitch_ops
nkeys = ops.n_keys
width = [TU.tile_cost(r) for r in ranges]
batches_of = TU.plan_exchange(ranges, world, False, sess.lanes, nkeys, width, [True] * len(ranges)).batches_of
offs = [sum(width[:i]) * nkeys for i in range(len(ranges))]          # every tile's slot in one buffer, in tile order
buf = torch.zeros(sum(width) * nkeys, dtype=torch.float32, device=dev)
slot = [buf[o:o + w * nkeys] for o, w in zip(offs, width)]
cnt = TU.count_volume((n, n, n), ranges, dev)


def share(rank):
    main = torch.cuda.current_stream(dev)
    start = torch.cuda.Event()
    start.record(main)
    index = ops.index_volume(full, ranges) if TU.COMPACT else None
    _, done = TU._run_batches(sess, ops, full, ranges, batches_of[rank], slot, width, index, [0] * sess.lanes, start)
    for ev in done:
        main.wait_event(ev)
    if rank == 0:
        ops.stitch([s_.view(nkeys, w) for s_, w in zip(slot, width)], ranges, (n, n, n), cnt, index=index)


worst = 0.0
for rank in range(world):
    for _ in range(3):                                      # eager pass, capture, first replay of this rank's batch graphs
        share(rank)
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        share(rank)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 5
    worst = max(worst, ms)
    print("rank %d of %d: batches %s (tiles x 80^3 units each)%s: %.2f ms" % (
        rank, world, ["%dx%d" % (len(b_), TU.tile_cost(ranges[b_[0]]) // 512000) for b_ in batches_of[rank]],
        " + stitch of all tiles" if rank == 0 else "", ms))
print("modelled %d-GPU step without the exchange: %.2f ms = %.0f Mvoxel/s" % (world, worst, n ** 3 / worst / 1e3))
