"""Generate the optimiser fixtures by RUNNING the reference's utils.LARS and build_schedulers.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_optim.py
Writes tests/golden/optim.npz:
  lars_hyper                   lr, weight_decay, momentum, eta of the LARS runs below
  lars_names                   the four parameters: 'mat' (73,137), 'conv' (2,3,1,1,1), 'vec' (41,) and 'zero' (5,7), all zeros
  lars_p0/<name>               start values (float32 numbers: both runs start from exactly these)
  lars_g<t>/<name>             the gradient of step t = 1..3 (unit normal * 10^(t-3), float32 numbers)
  lars64_p1/<name>, lars64_p3/<name>, lars64_mu3/<name>   parameter after steps 1 and 3 and state['mu'] after step 3 of
                               utils.LARS on float64 tensors (the later values depend on every step before them)
  lars32_p3/<name>, lars32_mu3/<name>       the same run on float32 tensors
  sched_args                   n_epochs, itr_per_epoch, warmup_epochs, lr, min_lr, weight_decay, weight_decay_end, lr_drop_multi
  sched_lr_drops               train_args.lr_drops
  sched_<kind>_lr, sched_<kind>_wd          build_schedulers' two arrays for lr_scheduler = 'cosine' | 'multistep'
and tests/golden/api_signatures_optim.json: inspect.signature of build_optimizer, build_schedulers and LARS.__init__.
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

SHAPES = (("mat", (73, 137)), ("conv", (2, 3, 1, 1, 1)), ("vec", (41,)), ("zero", (5, 7)))
LR, WD, MOM, ETA = 0.3, 0.1, 0.9, 1e-3


def main():
    import Trainer.models as TM
    import utils.misc as UM
    rs = np.random.RandomState(31)
    out = {"lars_hyper": np.array([LR, WD, MOM, ETA]), "lars_names": np.array([n for n, _ in SHAPES])}
    p0 = {n: (rs.randn(*s) if n != "zero" else np.zeros(s)).astype(np.float32) for n, s in SHAPES}
    gs = {t: {n: (rs.randn(*s) * 10.0 ** (t - 3)).astype(np.float32) for n, s in SHAPES} for t in (1, 2, 3)}
    for n, _ in SHAPES:
        out["lars_p0/" + n] = p0[n]
        for t in (1, 2, 3):
            out["lars_g%d/%s" % (t, n)] = gs[t][n]
    for tag, dt in (("lars64", torch.float64), ("lars32", torch.float32)):
        ps = {n: torch.nn.Parameter(torch.from_numpy(p0[n].copy()).to(dt)) for n, _ in SHAPES}   # step() works in place
        opt = UM.LARS([{"params": list(ps.values())}])
        for t in (1, 2, 3):
            for g in opt.param_groups:                      # Trainer/engine.py:95-97
                g["lr"], g["weight_decay"] = LR, WD
            for n, p in ps.items():
                p.grad = torch.from_numpy(gs[t][n]).to(dt)
            opt.step()
            for n, p in ps.items():
                if t == 3 or (t == 1 and dt == torch.float64):
                    out["%s_p%d/%s" % (tag, t, n)] = p.detach().numpy().copy()
                if t == 3:
                    out["%s_mu%d/%s" % (tag, t, n)] = opt.state[p]["mu"].numpy().copy()
    assert sorted(opt.state_dict()["param_groups"][0].keys()) == sorted(
        ["lr", "weight_decay", "momentum", "eta", "weight_decay_filter", "lars_adaptation_filter", "params"])

    n_epochs, itr, warm, lr, min_lr, wd0, wd1, gamma, drops = 3, 4, 1, 1e-4, 1e-6, 0.04, 0.4, 0.1, [1]
    out["sched_args"] = np.array([n_epochs, itr, warm, lr, min_lr, wd0, wd1, gamma])
    out["sched_lr_drops"] = np.array(drops)
    for kind in ("cosine", "multistep"):
        ta = types.SimpleNamespace(lr_scheduler=kind, n_epochs=n_epochs, warmup_epochs=warm, lr_drops=drops,
                                   lr_drop_multi=gamma, weight_decay=wd0, weight_decay_end=wd1)
        a, b = TM.build_schedulers(ta, itr, lr, min_lr)
        out["sched_%s_lr" % kind], out["sched_%s_wd" % kind] = np.asarray(a), np.asarray(b)

    np.savez_compressed(os.path.join(HERE, "optim.npz"), **out)
    sig = {"build_optimizer": TM.build_optimizer, "build_schedulers": TM.build_schedulers, "LARS.__init__": UM.LARS.__init__}
    with open(os.path.join(HERE, "api_signatures_optim.json"), "w") as f:
        json.dump({k: str(inspect.signature(v)) for k, v in sig.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: v.shape for k, v in out.items() if k.startswith("sched")})


if __name__ == "__main__":
    main()
