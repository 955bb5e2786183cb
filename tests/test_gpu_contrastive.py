"""The contrastive pre-training mode on the HIP kernels: bfm_loss_contrastive against float64 torch autograd of the
reference's formula (criterion.py:96-109) with torch's own fp32 evaluation as the yardstick, stress and overflow
temperatures, all-zero rows, linearity in coef, determinism; the head-less model, its processor and criterion, one full
ContrastiveStep iteration and its AdamW move against the float64 golden vectors made by running the reference
(tests/golden/make_golden_contrastive.py); sample count handling; the shipped 160^3 shape on two lanes.
Needs an MI355X: run with `-m gpu`."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import sd_from_npz

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_contrastive.npz")
EPS = 1e-12


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


# ----------------------------------------------------------------------------- the formula in torch
def torch_loss(x, y, n_norm, temps, dtype, coef=1.0, stop_at_pq=False):
    """The reference's evaluation on (N, C) maps in `dtype` on the CPU: F.normalize n_norm times, num, den by the loop over
    the channels with the inner sum over channels, mean of -log(num / den).  Returns (loss, per-voxel loss, d/dx, d/dy) of
    coef * loss; stop_at_pq: the gradients w.r.t. the normalised p, q instead, plus the chains [x0, x1, ..] of both."""
    alpha, beta, gamma = temps
    p = x.t().unsqueeze(0).to(dtype).clone().requires_grad_(not stop_at_pq)         # (1, C, N)
    q = y.t().unsqueeze(0).to(dtype).clone().requires_grad_(not stop_at_pq)
    leaf_p, leaf_q = p, q
    chain_p, chain_q = [p.detach()], [q.detach()]
    for _ in range(n_norm):
        p, q = F.normalize(p, dim=1), F.normalize(q, dim=1)
        chain_p.append(p.detach())
        chain_q.append(q.detach())
    if stop_at_pq:
        p, q = p.detach().requires_grad_(True), q.detach().requires_grad_(True)
        leaf_p, leaf_q = p, q
    num = torch.exp(p * q / alpha).sum(1)
    den = torch.zeros_like(p[:, 0])
    for i in range(p.shape[1]):
        pi = p[:, i]
        den = den + torch.exp(pi ** 2 / beta) + torch.exp(((pi[:, None] * p).sum(1) - pi ** 2) / gamma)
    vox = -torch.log(num / den)
    loss = vox.mean()
    (coef * loss).backward()
    out = (float(loss.detach()), vox.detach()[0], leaf_p.grad[0].t().contiguous(), leaf_q.grad[0].t().contiguous())
    return out + ((chain_p, chain_q),) if stop_at_pq else out


def kernel(x, y, n_norm, temps, coef=1.0, want_pq=False, grads=True):
    """bfm_loss_contrastive on (N, C) fp32 maps.  Returns (loss, dx, dy[, p, q]) as CPU tensors."""
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    n, c = xd.shape
    dx, dy = (torch.full_like(xd, float("nan")), torch.full_like(yd, float("nan"))) if grads else (None, None)
    po, qo = (torch.empty_like(xd), torch.empty_like(yd)) if want_pq else (None, None)
    val = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.bfm_loss_contrastive_workspace(), dtype=torch.uint8, device=dev)
    L.check(lib.bfm_loss_contrastive(L.ptr(xd), L.ptr(yd), c, n, n_norm, EPS, temps[0], temps[1], temps[2], coef, L.ptr(dx),
                                     L.ptr(dy), L.ptr(po), L.ptr(qo), L.ptr(val), L.ptr(ws), ws.numel(), L.stream_ptr()),
            "loss_contrastive")
    torch.cuda.synchronize()
    out = (float(val.item()), dx.cpu() if grads else None, dy.cpu() if grads else None)
    return out + (po.cpu(), qo.cpu()) if want_pq else out


def maps(c, n, n_norm, seed, noise=0.3):
    """x: random rows of varied length; y = x + noise.  n_norm = 0 means the maps ARE the features, so they come with unit
    rows (the reference's exponents p_i^2 / beta of an unnormalised row overflow any format)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c), generator=g, dtype=torch.float64) * (0.2 + 3.0 * torch.rand((n, 1), generator=g, dtype=torch.float64))
    y = x + noise * x.norm(dim=1, keepdim=True) / c ** 0.5 * torch.randn((n, c), generator=g, dtype=torch.float64)
    if n_norm == 0:
        x, y = F.normalize(x, dim=1), F.normalize(y, dim=1)
    return x.float(), y.float()


def check_against_torch(x, y, n_norm, temps, tag, bound=None, rows=None):
    """The rule of every comparison: error of the kernel against float64 torch <= 8 x the error of torch's fp32 evaluation
    against float64 torch on the same inputs, floor 1e-6 (loss: relative; gradients: max abs error / max abs of the
    float64 result).  bound: (loss, dx, dy) bounds measured elsewhere, where fp32 torch gives no yardstick.
    rows: boolean mask of the rows that enter the gradient norms."""
    l64, _, gx64, gy64 = torch_loss(x, y, n_norm, temps, torch.float64)
    lk, dx, dy = kernel(x, y, n_norm, temps)
    sel = slice(None) if rows is None else rows
    if bound is None:
        l32, _, gx32, gy32 = torch_loss(x, y, n_norm, temps, torch.float32)
        assert np.isfinite(l32) and bool(torch.isfinite(gx32).all()) and bool(torch.isfinite(gy32).all()), tag
        yard = (abs(l32 - l64) / abs(l64), _rel(gx32[sel], gx64[sel]), _rel(gy32[sel], gy64[sel]))
        bound = tuple(max(8.0 * e, 1e-6) for e in yard)
    else:
        yard = (float("nan"),) * 3
    assert np.isfinite(lk) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all()), tag
    err = (abs(lk - l64) / abs(l64), _rel(dx[sel], gx64[sel]), _rel(dy[sel], gy64[sel]))
    print("contrastive %-34s loss %.6f  err loss/dp/dq %.2e %.2e %.2e  torch-fp32 %.2e %.2e %.2e  bound %.2e %.2e %.2e"
          % ((tag, l64) + err + yard + bound))
    assert err[0] <= bound[0] and err[1] <= bound[1] and err[2] <= bound[2], (tag, err, bound)
    return bound


N_ODD = 4099                                              # not a multiple of the 32 (C = 64) or 4 voxels of a block trip


@pytest.mark.parametrize("temps", [(0.5, 0.5, 1.0), (0.1, 0.1, 0.1)])
@pytest.mark.parametrize("n_norm", [0, 1, 2])
@pytest.mark.parametrize("c", [8, 24, 64])
def test_kernel_vs_float64_autograd(c, n_norm, temps):
    x, y = maps(c, N_ODD, n_norm, seed=100 * c + n_norm)
    check_against_torch(x, y, n_norm, temps, "C=%d n_norm=%d T=%s" % (c, n_norm, temps))


def _stress_maps(n_norm):
    x, y = maps(64, N_ODD, n_norm, seed=77)
    v = torch.ones(64)
    v[5] = 63.0 ** 0.5                                    # p_5 * sum_{j != 5} p_j = sqrt(C - 1) / 2 after normalisation
    x[1234] = F.normalize(v, dim=0) if n_norm == 0 else 2.5 * v
    y[1234] = x[1234]
    return x, y


@pytest.mark.parametrize("n_norm", [0, 2])
def test_kernel_stress_temperatures(n_norm):
    """(0.07, 0.07, 0.05) at C = 64 with one voxel whose largest exponent of den is sqrt(63) / (2 * 0.05) = 79.4: the
    reference's fp32 is still finite there (asserted), so it stays the yardstick."""
    x, y = _stress_maps(n_norm)
    check_against_torch(x, y, n_norm, (0.07, 0.07, 0.05), "stress C=64 n_norm=%d" % n_norm)


def test_kernel_finite_where_fp32_reference_overflows():
    """alpha = 0.01 and a voxel with p = q = one channel: exponent 100 in num, exp overflows fp32 (asserted), the kernel
    subtracts the voxel's maximum first.  Bound: the one measured for (0.1, 0.1, 0.1) on the same maps."""
    x, y = maps(64, N_ODD, 2, seed=78)
    e = torch.zeros(64)
    e[9] = 3.0
    x[321], y[321] = e, e
    bound = check_against_torch(x, y, 2, (0.1, 0.1, 0.1), "overflow yardstick T=0.1")
    l32 = torch_loss(x, y, 2, (0.01, 0.1, 0.1), torch.float32)[0]
    assert not np.isfinite(l32), l32
    check_against_torch(x, y, 2, (0.01, 0.1, 0.1), "overflow alpha=0.01", bound=bound)


@pytest.mark.parametrize("n_norm", [1, 2])
def test_kernel_zero_rows(n_norm):
    """All-zero rows in x, y or both take F.normalize's eps branch.  The loss follows the rule; the gradients of those rows
    are finite and equal bfm_normalize_bwd applied n_norm times to float64 torch's gradient w.r.t. p, q (that kernel hands
    the incoming gradient / eps through); the other rows follow the rule with the zero rows kept out of the norms."""
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    temps = (0.1, 0.1, 0.1)
    c = 64
    x, y = maps(c, N_ODD, n_norm, seed=91)
    zx, zy, zb = [3, 700, 4098], [11, 701], [64, 2048]
    x[zx + zb] = 0.0
    y[zy + zb] = 0.0
    nz = torch.ones(N_ODD, dtype=torch.bool)
    nz[zx + zy + zb] = False
    bound = check_against_torch(x, y, n_norm, temps, "zero rows n_norm=%d (other rows)" % n_norm, rows=nz)
    # zero rows: both sides are fp32 evaluations of g / eps^n_norm.  g is the kernel's gradient w.r.t. p (or q), held to the
    # rule's bound as on the other rows; each normalisation then adds one rounding in the chain (a division by eps) and two
    # in the kernel (1 / eps, then a product): 3 * 2^-24 per normalisation on top of the rule's bound.
    extra = n_norm * 3 * 2.0 ** -24
    _, dx, dy = kernel(x, y, n_norm, temps)
    _, _, gp, gq, (chain_p, chain_q) = torch_loss(x, y, n_norm, temps, torch.float64, stop_at_pq=True)
    for name, got, g, chain, zero, bnd in (("dp", dx, gp, chain_p, zx + zb, bound[1] + extra),
                                           ("dq", dy, gq, chain_q, zy + zb, bound[2] + extra)):
        g = g.float().to(dev).contiguous()
        for j in range(n_norm - 1, -1, -1):
            feat = chain[j][0].t().contiguous().float().to(dev)
            out = torch.empty_like(g)
            L.check(lib.bfm_normalize_bwd(L.ptr(feat), L.ptr(g), c, N_ODD, EPS, L.ptr(out), L.stream_ptr()), "normalize_bwd")
            g = out
        ref = g.cpu()[zero]
        assert bool(torch.isfinite(got[zero]).all())
        if float(ref.abs().max()) == 0.0:
            assert float(got[zero].abs().max()) == 0.0
            continue
        err = _rel(got[zero], ref)
        print("contrastive zero rows n_norm=%d %s: max |grad| %.3e, err vs normalize_bwd chain %.2e, bound %.2e" %
              (n_norm, name, float(ref.abs().max()), err, bnd))
        assert err <= bnd, (name, err, bnd)
    # a row that is zero in x only still has 1 / eps per normalisation in dp; in both maps: no gradient at all
    assert float(dx[zx].abs().max()) > 1e6 and float(dx[zb].abs().max()) == 0.0 and float(dy[zb].abs().max()) == 0.0


def test_coef_is_linear_and_loss_ignores_it():
    x, y = maps(64, N_ODD, 2, seed=5)
    base = kernel(x, y, 2, (0.1, 0.1, 0.1), coef=1.0)
    for coef in (0.25, 1024.0, 65536.0):
        got = kernel(x, y, 2, (0.1, 0.1, 0.1), coef=coef)
        assert got[0] == base[0]
        assert torch.equal(got[1], base[1] * coef) and torch.equal(got[2], base[2] * coef)
    # the value-only call gives the same loss and the normalised maps
    lv, _, _, p, q = kernel(x, y, 2, (0.1, 0.1, 0.1), want_pq=True, grads=False)
    assert lv == base[0]
    p64 = F.normalize(F.normalize(x.double(), dim=1), dim=1)
    assert _rel(p, p64) <= 1e-6 and _rel(q, F.normalize(y.double(), dim=1)) <= 1e-6


@pytest.mark.parametrize("c", [24, 64])
def test_two_runs_give_the_same_bits(c):
    x, y = maps(c, 50021, 2, seed=6)
    a = kernel(x, y, 2, (0.1, 0.1, 0.1))
    b = kernel(x, y, 2, (0.1, 0.1, 0.1))
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_kernel_rejects_bad_arguments():
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    x = torch.zeros((16, 72), device=dev)
    val = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.bfm_loss_contrastive_workspace(), dtype=torch.uint8, device=dev)
    args = lambda c, n_norm, wsn: (L.ptr(x), L.ptr(x), c, 16, n_norm, EPS, 0.1, 0.1, 0.1, 1.0, None, None, None, None,  # noqa: E731
                                   L.ptr(val), L.ptr(ws), wsn, L.stream_ptr())
    assert lib.bfm_loss_contrastive(*args(72, 2, ws.numel())) == -2
    assert lib.bfm_loss_contrastive(*args(1, 2, ws.numel())) == -2
    assert lib.bfm_loss_contrastive(*args(64, 3, ws.numel())) == -1
    assert lib.bfm_loss_contrastive(*args(64, 2, 8)) == -3


# ----------------------------------------------------------------------------- model, criterion, training step
def _case():
    d = dict(np.load(GOLDEN))
    f_maps, levels, groups, size, stride = (int(v) for v in d["cfg"])
    xs = [torch.from_numpy(d["xq%d" % i].astype(np.float32) / np.float32(255)) for i in range(2)]
    return d, f_maps, levels, groups, size, stride, xs


def _session(d, f_maps, levels, groups, size):
    from brainfm_amd import test_utils as TU
    tasks = {str(t): True for t in d["tasks"]}
    ga, ta = TU.default_inference_args(f_maps=f_maps, num_levels=levels, num_groups=groups, size=(size,) * 3, tasks=tasks)
    wts = {str(k): float(v) for k, v in zip(d["loss_weight_names"], d["loss_weights"])}
    ta.weights = NS(contrastive=wts["loss_contrastive"])
    a, b, g = (float(t) for t in d["temperatures"])
    ta.contrastive_temperatures = NS(alpha=a, beta=b, gamma=g)
    return TU.InferenceSession(ga, ta, _dev(), state_dict=sd_from_npz(d), passes=3), wts, (a, b, g)


def test_headless_model_processor_and_criterion_vs_reference_golden():
    from brainfm_amd import models as M
    d, f_maps, levels, groups, size, stride, xs = _case()
    s, wts, temps = _session(d, f_maps, levels, groups, size)
    assert dict(s.train_args.out_channels) == {} and not list(s.model.head.parameters())
    samples = [{"input": x.to(_dev())} for x in xs]
    outs, _ = s.model(samples)
    assert all(list(o.keys()) == ["feat"] for o in outs)
    assert [type(p).__name__ for p in s.processors] == [str(n) for n in d["processor_names"]]
    for p in s.processors:
        outs = p(outs, None, "synth")
    for i, o in enumerate(outs):
        got = o["feat"][-1].cpu().numpy()[..., ::stride, ::stride, ::stride]
        err = _rel(got, d["feat_%d" % i])
        print("contrastive model feat[-1] of sample %d vs reference fp64: %.2e" % (i, err))
        assert err <= 1e-4
    crit = M.get_criterion(s.gen_args, s.train_args, s.tasks, _dev())
    assert dict(crit.weight_dict) == wts
    losses = crit(outs, None, samples)
    assert list(losses.keys()) == ["loss_contrastive"]
    ref = float(d["loss/loss_contrastive"])
    got = float(losses["loss_contrastive"])
    print("contrastive forward-only criterion: %.8f vs reference %.8f" % (got, ref))
    assert abs(got - ref) <= 1e-4 * abs(ref)


def _step(s, wts, temps, d, lanes=None):
    from brainfm_amd import train as TR
    hyper = d["hyper"]
    step = TR.ContrastiveStep(s.engine, wts, temps, lr=float(hyper[0]), weight_decay=float(hyper[1]),
                              betas=(float(hyper[2]), float(hyper[3])), eps=float(hyper[4]))
    if lanes is not None:
        step.sample_lanes = lanes
    return step


def test_training_iteration_vs_reference_golden(tmp_path):
    """loss_contrastive, the weighted total, every backbone gradient and the parameters after AdamW against the reference
    in float64; checkpoint round trip under the reference's names and shapes."""
    d, f_maps, levels, groups, size, stride, xs = _case()
    s, wts, temps = _session(d, f_maps, levels, groups, size)
    step = _step(s, wts, temps, d)
    assert step.n_norm == 2
    loss_dict, total, grads = step.loss_and_grads(xs, None, [{} for _ in xs])
    assert list(loss_dict.keys()) == [str(n) for n in d["loss_weight_names"]] == ["loss_contrastive"]
    ref = float(d["loss/loss_contrastive"])
    print("contrastive step loss %.8f vs reference %.8f" % (loss_dict["loss_contrastive"], ref))
    assert abs(loss_dict["loss_contrastive"] - ref) <= 1e-4 * abs(ref)
    assert abs(total - float(d["loss_total"])) <= 1e-4 * float(d["loss_total"])
    names = [str(n) for n in d["param_names"]]
    assert set(grads.keys()) == set(names)
    assert set(step.parameters().keys()) == set(names)
    worst = {k: _rel(grads[k].reshape(d["grad/" + k].shape).cpu().numpy(), d["grad/" + k]) for k in names}
    print("contrastive step max rel grad err vs reference fp64: %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > 2e-3}
    assert not bad, bad
    before = {k: v.detach().double().cpu().clone() for k, v in step.parameters().items()}
    stepped, _ = step.apply(grads)
    assert stepped and step.t == 1
    after = step.parameters()
    lr = float(d["hyper"][0])
    # the reference's AdamW move: torch.optim.AdamW on the reference's state and gradient (what the generator ran)
    params = {k: torch.nn.Parameter(torch.from_numpy(d["sd/" + k]).double().clone()) for k in names}
    opt = torch.optim.AdamW(list(params.values()), lr=lr, weight_decay=float(d["hyper"][1]),
                            betas=(float(d["hyper"][2]), float(d["hyper"][3])), eps=float(d["hyper"][4]))
    for k in names:
        params[k].grad = torch.from_numpy(d["grad/" + k]).double()
    opt.step()
    for k in names:
        ref_delta = params[k].detach().numpy() - d["sd/" + k]
        got = (after[k].double().cpu() - before[k]).reshape(ref_delta.shape).numpy()
        # step 1 of Adam moves a weight by about lr * sign(g): compared where the reference's gradient is well clear of the
        # fp32 gradient's error, so that its sign is not in doubt
        well = np.abs(d["grad/" + k]) > 1e-2 * np.abs(d["grad/" + k]).max()
        tol = 2e-2 * lr + 4e-7 * float(before[k].abs().max())
        assert np.abs(got - ref_delta)[well].max(initial=0.0) <= tol, k
    sd = step.state_dict()
    assert set(sd.keys()) == set(names)
    for k in names:
        assert tuple(sd[k].shape) == tuple(d["sd/" + k].shape), k
    path = str(tmp_path / "ckp.pth")
    step.save_checkpoint(path, epoch=3)
    s2, _, _ = _session(d, f_maps, levels, groups, size)
    step2 = _step(s2, wts, temps, d)
    ckp = step2.load_checkpoint(path)
    assert int(ckp["epoch"]) == 3 and step2.t == 1
    for k, v in step2.parameters().items():
        assert torch.equal(v, after[k]), k
    # the next iteration runs on the updated weights (on the two lanes) and lowers nothing it should not: finite, stepped
    ld2, total2, stepped2 = step.step(xs, None, [{} for _ in xs])
    assert stepped2 and np.isfinite(total2) and step.t == 2


def test_sample_count():
    """Samples after the second are not run and change nothing; fewer than two is an error."""
    from brainfm_amd import _lib as L
    d, f_maps, levels, groups, size, stride, xs = _case()
    s, wts, temps = _session(d, f_maps, levels, groups, size)
    step = _step(s, wts, temps, d)
    two = step.loss_and_grads(xs, None, [{}, {}])
    third = torch.rand_like(xs[0])
    three = step.loss_and_grads(xs + [third], None, [{}, {}, {}])
    assert two[0] == three[0] and two[1] == three[1]
    for k, v in two[2].items():
        assert torch.equal(v, three[2][k]), k
    with pytest.raises(L.BfmError, match="two"):
        step.loss_and_grads(xs[:1], None, [{}])
    with pytest.raises(L.BfmError):
        step.loss_and_grads([], None, [])


def test_two_lanes_equal_one_lane_small():
    d, f_maps, levels, groups, size, stride, xs = _case()
    s, wts, temps = _session(d, f_maps, levels, groups, size)
    step = _step(s, wts, temps, d)
    step.loss_and_grads(xs, None, [{}, {}])                # first pass: packs and tunes
    step.t = 1
    res = {}
    for lanes in (1, 2):
        step.sample_lanes = lanes
        ld, total, grads = step.loss_and_grads(xs, None, [{}, {}])
        torch.cuda.synchronize()
        res[lanes] = (ld, total, {k: v.detach().clone() for k, v in grads.items()})
    assert res[1][0] == res[2][0] and res[1][1] == res[2][1]
    for k, v in res[1][2].items():
        assert torch.equal(v, res[2][2][k]), k


def test_shipped_shape_two_lanes_equal_one_lane():
    """160^3, C = 64, 6 levels: a contrastive iteration with the two forwards and the two backwards on the two sample lanes
    gives the single-lane bits."""
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    ga, ta = TU.default_inference_args(tasks=dict(T1=True, contrastive=True))
    torch.manual_seed(0)
    s = TU.InferenceSession(ga, ta, _dev(), passes=3)
    step = TR.ContrastiveStep(s.engine, {"loss_contrastive": 1.0}, (0.1, 0.1, 0.1), lr=1e-4)
    assert step.c_feat == 64 and step.n_norm == 2
    g = torch.Generator().manual_seed(1)
    x0 = torch.rand((1, 1, 160, 160, 160), generator=g)
    xs = [x0, (x0 + 0.05 * torch.rand((1, 1, 160, 160, 160), generator=g)).clamp(0, 1)]
    step.t = 1                                                # lanes are used from the second iteration on
    res = {}
    for lanes in (1, 2):
        step.sample_lanes = lanes
        ld, total, grads = step.loss_and_grads(xs, None, [{}, {}])
        torch.cuda.synchronize()
        res[lanes] = (ld, total, {k: v.detach().clone() for k, v in grads.items()})
    assert res[1][0] == res[2][0] and res[1][1] == res[2][1]
    assert np.isfinite(res[1][1]) and res[1][1] > 0
    for k, v in res[1][2].items():
        assert torch.equal(v, res[2][2][k]), k
        assert bool(torch.isfinite(v).all()), k
    assert float(res[1][2]["backbone.encoders.0.basic_module.SingleConv1.conv.weight"].abs().sum()) > 0
