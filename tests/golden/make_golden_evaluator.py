"""Generate the evaluator's golden vectors by RUNNING the reference's Evaluator (Trainer/models/evaluator.py).

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_evaluator.py
Writes tests/golden/evaluator.npz:
  o, t (1,2,9,11,13) fp32      a pair of volumes (t has zeros: the nonzero_only mask), 2574 elements: no multiple of 4
  l1_32/64, l1nz_32/64, psnr_32/64, nl2_32/64    get_l1 (both modes), get_psnr, get_normalized_l2 on the fp32 tensors as the
                               reference runs them, and on float64 copies of the same values (the arbiter)
  z_l1_*, z_nl2_*              the same pair against an all-zero target (get_psnr raises there: log10(0))
  dice_o, dice_t (1,3,6,7,9)   probabilities and a one-hot target; dice_32/64 = get_dice
  lab_p_a/lab_t_a (20,24,28), lab_p_b/lab_t_b (7,5,3) int16    label volumes drawn from label_list_segmentation plus a few
                               labels that are not in it (the LUT sends them to class 0); labdice_{a,b}_32/64 = get_dice of
                               their get_onehot maps (float64: the one-hot cast up)
  tasks_<i>, metrics_<i>       get_evaluator's metric names for five task sets; empty_asserts = 1: [] trips its assertion
and tests/golden/api_signatures_evaluator.json: inspect.signature of the mirrored callables.
pytorch_msssim is a stub in this container (ref_import.py), so nothing here touches SSIM: tests/ssim_refs.py restates it.
"""
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.setup()
import torch  # noqa: E402


def main():
    import Trainer.models as TM
    import Trainer.models.evaluator as E
    args = types.SimpleNamespace(ssim_win_sigma=1.5)
    ev = E.Evaluator(args, ['feat_l1'], 'cpu')
    rs = np.random.RandomState(20)
    out = {}

    o = rs.rand(1, 2, 9, 11, 13).astype(np.float32)
    t = (o + 0.1 * rs.randn(*o.shape)).astype(np.float32)
    t[rs.rand(*o.shape) < 0.3] = 0
    out["o"], out["t"] = o, t

    def both(fn, a, b, **kw):
        r32 = fn('m', torch.from_numpy(a), torch.from_numpy(b), **kw)['m']
        r64 = fn('m', torch.from_numpy(a.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), **kw)['m']
        return np.asarray(r32), np.asarray(r64)

    out["l1_32"], out["l1_64"] = both(ev.get_l1, o, t)
    out["l1nz_32"], out["l1nz_64"] = both(ev.get_l1, o, t, nonzero_only=True)
    out["psnr_32"], out["psnr_64"] = both(ev.get_psnr, o, t)
    out["nl2_32"], out["nl2_64"] = both(ev.get_normalized_l2, o, t)
    z = np.zeros_like(t)
    out["z_l1_32"], out["z_l1_64"] = both(ev.get_l1, o, z)
    out["z_nl2_32"], out["z_nl2_64"] = both(ev.get_normalized_l2, o, z)
    assert both(ev.get_psnr, o, o)[0] == float('inf')

    logits = rs.randn(1, 3, 6, 7, 9).astype(np.float32)
    do = torch.softmax(torch.from_numpy(logits), dim=1).numpy()
    dt = np.eye(3, dtype=np.float32)[rs.randint(0, 3, size=(6, 7, 9))].transpose(3, 0, 1, 2)[None].copy()
    out["dice_o"], out["dice_t"] = do, dt
    out["dice_32"], out["dice_64"] = both(ev.get_dice, do, dt)

    pool = np.array(E.label_list_segmentation + [1, 5, 99, 250], dtype=np.int16)
    for tag, shape in (("a", (20, 24, 28)), ("b", (7, 5, 3))):
        T = pool[rs.randint(0, len(pool), size=shape)]
        P = T.copy()
        flip = rs.rand(*shape) < 0.25
        P[flip] = pool[rs.randint(0, len(pool), size=int(flip.sum()))]
        out["lab_p_" + tag], out["lab_t_" + tag] = P, T
        hp = E.get_onehot(P.astype(np.int64), 'cpu')[None]
        ht = E.get_onehot(T.astype(np.int64), 'cpu')[None]
        out["labdice_%s_32" % tag] = np.asarray(ev.get_dice('m', hp, ht)['m'])
        out["labdice_%s_64" % tag] = np.asarray(ev.get_dice('m', hp.double(), ht.double())['m'])

    task_sets = [['T1'], ['super_resolution'], ['bias_field', 'segmentation'], ['segmentation', 'pathology'],
                 ['T1', 'super_resolution']]
    for i, ts in enumerate(task_sets):
        out["tasks_%d" % i] = np.array(ts)
        out["metrics_%d" % i] = np.array(TM.get_evaluator(args, ts, 'cpu').metric_names)
    try:
        TM.get_evaluator(args, [], 'cpu')
        out["empty_asserts"] = np.array(0)
    except AssertionError:
        out["empty_asserts"] = np.array(1)

    np.savez_compressed(os.path.join(HERE, "evaluator.npz"), **out)

    sig = {"get_onehot": E.get_onehot, "align_shape": E.align_shape, "get_evaluator": TM.get_evaluator,
           "Evaluator.__init__": E.Evaluator.__init__}
    for m in ("get_dice", "get_normalized_l2", "get_l1", "get_psnr", "get_ssim", "get_ms_ssim", "get_score", "eval"):
        sig["Evaluator." + m] = getattr(E.Evaluator, m)
    with open(os.path.join(HERE, "api_signatures_evaluator.json"), "w") as f:
        json.dump({k: str(inspect.signature(v)) for k, v in sig.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(out):
        if out[k].size <= 4:
            print(k, out[k])


if __name__ == "__main__":
    main()
