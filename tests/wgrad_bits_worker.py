"""One child process of tests/test_gpu_wgrad_bits.py and tests/golden/make_golden_wgrad_bits.py: the weight-gradient cases of
one entry of wgrad_cases.BITS_RUNS through _Wg.run, in the environment the parent gave (BFM_WGRAD_WS and BFM_WGRAD_UPFOLD
are read once per process, so each setting needs a process of its own).

    python tests/wgrad_bits_worker.py <default|ws0|upfold0>

prints one JSON line per case: {"case": id, "sha": SHA-256 of dW's bytes, "head": dW's first 16 values, "plan": the array of
bfm_conv3x3x3_wgrad_plan with allow = -1, or null where the library has no such export}.  spawn() is the parents' side."""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TIMEOUT = 120


def case_id(case, passes):
    return "-".join(str(v).replace(" ", "") for v in case) + "/p%d" % passes


def spawn(run):
    """{case id: record} of one child process.  A child that ends on a signal, a non-zero status or the time limit raises
    (subprocess.TimeoutExpired kills it first): the caller starts nothing after it."""
    import wgrad_cases as WC
    env = dict(os.environ, **WC.BITS_RUNS[run][0])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), run], capture_output=True, text=True, timeout=TIMEOUT,
                       env=env, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("wgrad_bits_worker %s ended with status %d\n%s\n%s" % (run, r.returncode, r.stdout[-2000:],
                                                                                  r.stderr[-4000:]))
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    want = [case_id(c, p) for c, p in WC.BITS_RUNS[run][2]]
    assert [x["case"] for x in recs] == want, (run, [x["case"] for x in recs], want)
    return {x.pop("case"): x for x in recs}


def main(run):
    for p in (HERE, ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import wgrad_cases as WC
    from brainfm_amd import _lib as L
    lib = L.load()
    has_plan = hasattr(lib, "bfm_conv3x3x3_wgrad_plan") and "bfm_conv3x3x3_wgrad_plan" in L.SIGNATURES
    for case, passes in WC.BITS_RUNS[run][2]:
        w = WC._Wg(*case)
        dW = w.run(w.dP, passes=passes)
        torch.cuda.synchronize()
        host = dW.cpu().contiguous()
        assert bool(torch.isfinite(host).all()), case
        rec = {"case": case_id(case, passes), "sha": hashlib.sha256(host.numpy().tobytes()).hexdigest(),
               "head": [float(v) for v in host.reshape(-1)[:16].tolist()],
               "plan": WC.plan(lib, case, passes, -1)[0] if has_plan else None}
        print(json.dumps(rec), flush=True)
        del w, dW


if __name__ == "__main__":
    main(sys.argv[1])
