"""Bits of the training-loss kernels, for comparing two trees (profiles/loss_kernels_refactor.txt).

    python <path>/scripts/loss_kernels_dump.py OUT_DIR          run from the root of the tree under test (built, on the GPU)
    python scripts/loss_kernels_dump.py --compare DIR_A DIR_B   sha256 of every file, both ways

The package, the tests' helpers and the golden case come from the CURRENT DIRECTORY's tree, so the same script file serves a
checkout of another commit.  On the golden training case (tests/test_gpu_train.py::_build) it calls
TrainStep._sample_losses in both layouts of the head outputs on one fixed random `raw` and writes dRaw and the fp64 loss
slots, then runs one full loss_and_grads (the layout BFM_TRAIN_ROWS selects) and writes every gradient."""
import hashlib
import os
import sys


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("file lists differ: only in %s: %s; only in %s: %s" % (a, sorted(set(fa) - set(fb)), b, sorted(set(fb) - set(fa))))
        return 1
    bad = [f for f in fa if sha(os.path.join(a, f)) != sha(os.path.join(b, f))]
    print("%d files in each of %s and %s; differing: %s" % (len(fa), a, b, bad if bad else "none"))
    return 1 if bad else 0


def dump(out):
    root = os.getcwd()
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    import torch
    import test_gpu_train as TG
    from test_oracle_train import load_case
    os.makedirs(out, exist_ok=True)
    c = load_case()
    step, xs, target, samples = TG._build(c)
    dev = torch.device("cuda:0")
    dims = tuple(xs[0].shape[-3:])
    nvox = dims[0] * dims[1] * dims[2]
    n_out = step.tail.n_out
    raw = (torch.randn((nvox, n_out), generator=torch.Generator().manual_seed(11)) * 1.5).to(dev)
    for rows in (False, True):
        r = raw.t().contiguous() if rows else raw
        dRaw = torch.zeros_like(r)
        vals = torch.zeros(4 * len(step.loss_names) + 2 * n_out + 8, dtype=torch.float64, device=dev)
        step._sample_losses(r, dims, target, samples[0], dRaw, vals, 1.0, rows=rows)
        torch.cuda.synchronize()
        tag = "rows" if rows else "cl"
        np.save(os.path.join(out, "sample_losses_%s_dRaw.npy" % tag), dRaw.cpu().numpy())
        np.save(os.path.join(out, "sample_losses_%s_vals.npy" % tag), vals.cpu().numpy())
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    np.save(os.path.join(out, "losses.npy"), np.array([total] + [loss_dict[k] for k in loss_dict], np.float64))
    for k, g in grads.items():
        np.save(os.path.join(out, "grad_%s.npy" % k), g.cpu().numpy())
    print("BFM_TRAIN_ROWS=%s: %d files in %s" % (os.environ.get("BFM_TRAIN_ROWS", "(unset)"), len(os.listdir(out)), out))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(os.path.abspath(sys.argv[1]))
