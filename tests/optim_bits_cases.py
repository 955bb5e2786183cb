"""The cases of tests/golden/optim_bits.npz: the bits of the four optimiser steps (adamw, adam, sgd, lars) as the library
gave them while AdamW still had kernels of its own in train_heads.hip, so that moving it into optim.hip can be held to
torch.equal.  tests/golden/make_golden_optim_bits.py stores what these functions return, tests/test_gpu_optim_bits.py runs
them again and compares, tests/test_host_optim_bits.py checks the file against expected_keys().

  abi/<kind>/{p,s0,s1}/<tensor>   three steps through the C ABI on the tensor list of tests/test_gpu_optim.py (chunk and
                                  alignment edges): parameters and state buffers after step 3, whole up to FULL elements
                                  and for the view, else the SHA-256 of the tensor's bytes (uint8[32])
  abi/sumsq, abi/lars_sums        float64 outputs of bfm_grad_sumsq_multi ([n], the same for adamw, adam and sgd) and of
                                  bfm_lars_sums_multi ([n][3]) at step 1
  apply/<kind>/{norms,p_sha,s_sha}  TrainStep.apply twice on seeded gradients (no backward pass: no atomics): the returned
                                  norms [2][n] as float64, the digests of every parameter [n][32] and state buffer
                                  [n][buffers][32] after the second call
  apply/names                     the parameters, in TrainStep.parameters() order"""
import hashlib

import numpy as np
import torch

KINDS = ("adamw", "adam", "sgd", "lars")
FULL = 4099
SCALE = 1024.0
BOOSTED = 2
N_STATE = {"adamw": 2, "adam": 2, "sgd": 1, "lars": 1}


def sha(t):
    """SHA-256 of a CPU tensor's bytes as uint8[32]."""
    return np.frombuffer(hashlib.sha256(t.contiguous().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def _stored(name, t):
    return t.numpy().copy() if (t.numel() <= FULL or name == "view") else sha(t)


def run_abi(kind):
    """{key: array} of the C-ABI half for one kind (test_gpu_optim._run_kernels, three steps)."""
    import test_gpu_optim as TG
    tensors = TG._tensor_list(kind)
    ps, states, sums = TG._run_kernels(kind, tensors)
    out = {}
    for (name, _, _, _, _), p, bufs in zip(tensors, ps, states):
        out["abi/%s/p/%s" % (kind, name)] = _stored(name, p)
        for j, b in enumerate(bufs):
            if b is not None:
                out["abi/%s/s%d/%s" % (kind, j, name)] = _stored(name, b)
    out["abi/lars_sums" if kind == "lars" else "abi/sumsq"] = sums.numpy().astype(np.float64)
    return out


def apply_grads(params, call):
    """Seeded gradients for every parameter, times SCALE as a scaled backward pass would leave them.  Unscaled they have the
    norm 1e-3 sqrt(n): below the golden case's clip_max_norm (0.05) for the small tensors, above it for the conv weights; the
    first conv weight's (parameter BOOSTED) is a thousand times that, far above."""
    g_ = torch.Generator().manual_seed(4242 + call)
    out = {}
    for i, (k, p) in enumerate(params.items()):
        g = torch.randn(p.shape, generator=g_) * (1e-3 * SCALE)
        out[k] = g * 1e3 if i == BOOSTED else g
    return out


def run_apply(kind):
    """{key: array} of the TrainStep.apply half for one kind, and the parameter names."""
    import test_gpu_optim as TG
    from brainfm_amd import train as TR
    c = TG.load_case()
    step, _, _, _ = TG._build(c, kind, scaler=TR.LossScaler(init_scale=SCALE))
    params = step.parameters()
    norms = []
    for call in range(2):
        grads = {k: g.to(step.dev) for k, g in apply_grads(params, call).items()}
        ok, nrm = step.apply(grads)
        assert ok and step.scaler.scale == SCALE
        norms.append(nrm)
    torch.cuda.synchronize()
    norms = np.array(norms, dtype=np.float64)
    assert c["clip"] > 0 and norms[:, BOOSTED].min() > 10 * c["clip"] and (norms < c["clip"]).any()
    assert (np.delete(norms, BOOSTED, axis=1) > c["clip"]).any()
    out = {"apply/%s/norms" % kind: norms,
           "apply/%s/p_sha" % kind: np.stack([sha(p.cpu()) for p in params.values()]),
           "apply/%s/s_sha" % kind: np.stack([np.stack([sha(b.cpu()) for b in step.state[k]]) for k in params])}
    return out, list(params.keys())


def expected_keys():
    """{key: (dtype, shape)} of everything the file holds besides apply/names; None in a shape: the parameter count."""
    import test_gpu_optim as TG
    want = {}
    for kind in KINDS:
        tensors = TG._tensor_list(kind)
        for name, _, p0, _, _ in tensors:
            whole = p0.numel() <= FULL or name == "view"
            for what in ("p", "s0", "s1")[:1 + N_STATE[kind]]:
                want["abi/%s/%s/%s" % (kind, what, name)] = (np.float32, (p0.numel(),)) if whole else (np.uint8, (32,))
        want["apply/%s/norms" % kind] = (np.float64, (2, None))
        want["apply/%s/p_sha" % kind] = (np.uint8, (None, 32))
        want["apply/%s/s_sha" % kind] = (np.uint8, (None, N_STATE[kind], 32))
    want["abi/sumsq"] = (np.float64, (len(TG._tensor_list("adamw")),))
    want["abi/lars_sums"] = (np.float64, (len(TG._tensor_list("lars")), 3))
    return want
