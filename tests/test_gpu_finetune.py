"""Head-only fine-tuning on a frozen backbone (TrainStep(trainable="head"), train_args.freeze_feat): the weight-gradient
kernel of the 1x1x1 heads against float64, one frozen iteration against the reference's golden vectors
(tests/golden/train_step.npz), what the step must leave alone, the optimisers, the scaler, checkpoints, hidden head layers,
the pooled scalar head and the refusals.  Needs an MI355X: run with `-m gpu`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import sd_from_npz
from test_oracle_train import load_case

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def _session(c):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=c["f_maps"], num_levels=c["levels"], left_hemis_only=True,
                                       num_groups=c["groups"])
    return TU.InferenceSession(ga, ta, _dev(), state_dict=sd_from_npz(c["d"]), passes=3)


def _build(c, trainable="head", scaler=None, optimizer="adamw", session=None):
    """tests/test_gpu_train.py's _build with the `trainable` (and optimiser) argument."""
    from brainfm_amd import train as TR
    d = c["d"]
    s = _session(c) if session is None else session
    step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), c["loss_names"], c["loss_weights"], d["weights_ce"], c["all_samples"],
                        max_surf_distance=c["max_dist"], bias_field_log_type="l2" if c["bias_l2"] else "l1",
                        lr=c["lr"], weight_decay=c["wd"], betas=(c["b1"], c["b2"]), eps=c["eps"],
                        clip_max_norm=c["clip"], scaler=scaler, optimizer=optimizer, trainable=trainable)
    target = {k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("target/")}
    xs = [torch.from_numpy(d["x%d" % i]) for i in range(c["n_samples"])]
    samples = [{"bias_field_log": torch.from_numpy(d["bias_field_log%d" % i]),
                "high_res_residual": torch.from_numpy(d["high_res_residual%d" % i])} for i in range(c["n_samples"])]
    return step, xs, target, samples


def _heads(names):
    return [n for n in names if n.startswith("head.")]


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("n_out,nvox", [(1, 64), (8, 1000), (33, 64), (69, 128 * 77 + 5), (96, 4096), (97, 4096)])
def test_head_wgrad_kernel_vs_float64(n_out, nvox):
    """bfm_head_wgrad / bfm_head_wgrad_rows: dW = dRaw^T . Fn and db = column sums of dRaw, written into NaN-filled outputs,
    within 2e-5 of the largest entry of the float64 result (the bound bfm_head_bwd is held to for the same sums,
    test_heads_backward_fused_pass_vs_float64); head widths on both sides of the 32-row blocks, voxel counts below, at and
    off the 64-voxel tile, one width (97) the rows form refuses.  The rows form reads a pitch of nvox + 24 with NaN padding
    and gives the channels-last form's bits; two runs give the same bits; an all-zero dRaw gives exact zeros."""
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    for cf in (64, 16):
        g = torch.Generator().manual_seed(n_out * 7 + cf)
        dRaw = (torch.randn(nvox, n_out, generator=g) * (torch.rand(nvox, 1, generator=g) > 0.3)).to(dev)
        Fn = torch.randn(nvox, cf, generator=g).to(dev)
        ws = torch.empty(lib.bfm_head_wgrad_workspace(n_out, cf, nvox), dtype=torch.uint8, device=dev)

        def run(src):
            dW = torch.full((n_out, cf), float("nan"), device=dev)
            db = torch.full((n_out,), float("nan"), device=dev)
            L.check(lib.bfm_head_wgrad(L.ptr(src), L.ptr(Fn), n_out, cf, nvox, L.ptr(dW), L.ptr(db), L.ptr(ws), ws.numel(),
                                       L.stream_ptr()), "head_wgrad")
            return dW, db

        dW, db = run(dRaw)
        r64, f64 = dRaw.double(), Fn.double()
        for got, ref, what in ((dW, r64.t() @ f64, "dW"), (db, r64.sum(0), "db")):
            err = float((got.double() - ref).abs().max()) / max(1e-6, float(ref.abs().max()))
            print("head_wgrad n_out=%d nvox=%d C=%d %s: err %.2e of the largest entry" % (n_out, nvox, cf, what, err))
            assert err <= 2e-5, (cf, what, err)
        dW_b, db_b = run(dRaw)
        assert torch.equal(dW_b, dW) and torch.equal(db_b, db)
        pitch = nvox + 24
        rows = torch.full((n_out, pitch), float("nan"), device=dev)
        rows[:, :nvox] = dRaw.t()
        dW2 = torch.full((n_out, cf), float("nan"), device=dev)
        db2 = torch.full((n_out,), float("nan"), device=dev)
        rc = lib.bfm_head_wgrad_rows(L.ptr(rows), pitch, L.ptr(Fn), n_out, cf, nvox, L.ptr(dW2), L.ptr(db2), L.ptr(ws),
                                     ws.numel(), L.stream_ptr())
        if cf == 64 and n_out <= 96:
            L.check(rc, "head_wgrad_rows")
            assert torch.equal(dW2, dW) and torch.equal(db2, db)
        else:
            assert rc == -2                            # as bfm_head_bwd_rows: C == 64 and n_out <= 96 only
        assert lib.bfm_head_wgrad_rows(L.ptr(rows), nvox - 1, L.ptr(Fn), n_out, cf, nvox, L.ptr(dW2), L.ptr(db2), L.ptr(ws),
                                       ws.numel(), L.stream_ptr()) == -1
        dW0, db0 = run(torch.zeros_like(dRaw))
        assert float(dW0.abs().max()) == 0.0 and float(db0.abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. one frozen iteration
def test_frozen_iteration_vs_reference_golden():
    """Losses to 1e-4 and every head gradient to 2e-3 relative of the reference's float64 run (the rules of
    test_training_iteration_vs_reference_golden for the same tensors); the gradient dictionary holds the head's names alone."""
    c = load_case()
    d = c["d"]
    step, xs, target, samples = _build(c)
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    assert list(loss_dict.keys()) == ["loss_" + n for n in c["loss_names"]]
    for k, v in loss_dict.items():
        ref = float(d["loss/" + k])
        print("loss %-26s frozen %.6f  reference %.6f" % (k, v, ref))
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, v, ref)
    assert abs(total - float(d["loss_total"])) <= 1e-4 * float(d["loss_total"])
    heads = _heads(c["names"])
    assert list(step.parameters().keys()) == c["names"]           # parameters() still lists everything
    assert set(grads.keys()) == set(heads) and len(heads) == 2 * len(step.tail.row_of)
    worst = {k: _rel(grads[k].reshape(d["grad/" + k].shape).cpu().numpy(), d["grad/" + k]) for k in heads}
    print("frozen step: max rel head grad err vs reference fp64: %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    full, _, _, _ = _build(c, trainable="all")
    _, total_full, gfull = full.loss_and_grads(xs, target, samples)
    diff = {k: _rel(grads[k].cpu().numpy(), gfull[k].cpu().numpy()) for k in heads}
    print("frozen step: max rel head grad difference from the full step: %.2e (%s); totals %.8f / %.8f"
          % (max(diff.values()), max(diff, key=diff.get), total, total_full))
    bad = {k: v for k, v in worst.items() if v > 2e-3}
    assert not bad, bad


# ----------------------------------------------------------------------------- 3. nothing frozen moves
def test_frozen_steps_leave_the_backbone_and_its_packs_alone():
    c = load_case()
    step, xs, target, samples = _build(c)
    eng = step.eng
    heads = set(_heads(c["names"]))
    before = {k: v.clone() for k, v in step.parameters().items()}
    packs = {}
    totals, counts = [], []
    for it in range(5):
        _, total, stepped = step.step(xs, target, samples)
        assert stepped
        totals.append(total)
        counts.append(eng.pack_count)
        if it == 1:
            packs = {ly.name: {k: v[0].clone() for k, v in ly.packs.items() if isinstance(v, tuple)}
                     for pair in eng.enc + eng.dec for ly in pair}
    after = step.parameters()
    for k, v in before.items():
        if k in heads:
            assert not torch.equal(v, after[k]), k
        else:
            assert torch.equal(v, after[k]), k
    assert counts[4] == counts[1], counts                        # nothing is packed after the first steps
    for pair in eng.enc + eng.dec:
        for ly in pair:
            for k, buf in packs[ly.name].items():
                assert torch.equal(ly.packs[k][0], buf), (ly.name, k)
    assert totals[1] != totals[0]
    assert step.__dict__.get("_grad_store") is None               # the GradStore is never made


# ----------------------------------------------------------------------------- 4. the same update
@pytest.mark.parametrize("kind", ["adamw", "adam", "sgd", "lars"])
def test_frozen_step_updates_the_heads_like_the_full_step(kind):
    """A full step given the frozen step's head gradients (beside its own backbone gradients) moves the heads, and their
    optimiser state, to the same bits: the frozen step's table, norms and descriptors are the full step's, head rows only."""
    c = load_case()
    a, xs, target, samples = _build(c, trainable="all", optimizer=kind)
    b, _, _, _ = _build(c, trainable="head", optimizer=kind)
    heads = _heads(c["names"])
    for it in range(2):
        _, _, ga = a.loss_and_grads(xs, target, samples)
        _, _, gb = b.loss_and_grads(xs, target, samples)
        mixed = {k: (gb[k].clone() if k in gb else v) for k, v in ga.items()}
        ok_a, _ = a.apply(mixed)
        ok_b, norms_b = b.apply(gb)
        assert ok_a and ok_b and len(norms_b) == len(heads)
        pa, pb = a.parameters(), b.parameters()
        for k in heads:
            assert torch.equal(pa[k], pb[k]), (kind, it, k)
            assert len(a.state[k]) == len(b.state[k])
            for sa, sb in zip(a.state[k], b.state[k]):
                assert torch.equal(sa, sb), (kind, it, k)
        assert set(b.state.keys()) == set(heads)
        # the heads see the same features in the next round only while the backbone has not moved: put A's back
        if it == 0:
            for k, v in a.parameters().items():
                if k not in heads:
                    v.copy_(pb[k])
            a._weights_changed()


# ----------------------------------------------------------------------------- 5. the scaler
def test_frozen_step_scaler_skips_a_nonfinite_head_gradient():
    from brainfm_amd import train as TR
    c = load_case()
    step, xs, target, samples = _build(c, scaler=TR.LossScaler(init_scale=1024.0))
    _, _, grads = step.loss_and_grads(xs, target, samples)
    grads["head.final_conv_T1.weight"][0, 0] = float("inf")
    before = {k: v.clone() for k, v in step.parameters().items()}
    stepped, _ = step.apply(grads)
    assert stepped is False and step.scaler.scale == 512.0 and step.t == 0
    for k, v in step.parameters().items():
        assert torch.equal(v, before[k]), k
    with pytest.raises(Exception, match="frozen"):               # a backbone gradient handed to a frozen step is refused
        step.apply({"backbone.encoders.0.basic_module.SingleConv1.conv.weight":
                    torch.zeros_like(before["backbone.encoders.0.basic_module.SingleConv1.conv.weight"])})


# ----------------------------------------------------------------------------- 6. checkpoints
def test_frozen_checkpoint_round_trip(tmp_path):
    from brainfm_amd import _lib as L
    from brainfm_amd import test_utils as TU
    c = load_case()
    s = _session(c)
    vol = torch.from_numpy(c["d"]["x0"]).to(_dev())
    out0, _ = s.forward_fused(vol)
    feat0, t1_0 = out0["feat"][-1].clone(), out0["T1"].clone()
    a, xs, target, samples = _build(c, session=s)
    for _ in range(2):
        a.step(xs, target, samples)
    path = str(tmp_path / "finetuned.pth")
    a.save_checkpoint(path, epoch=1)
    ckp = torch.load(path, map_location="cpu", weights_only=False)
    heads = _heads(c["names"])
    assert ckp["trainable"] == "head" and set(ckp["model"].keys()) == set(c["names"])
    opt = ckp["optimizer"]
    assert opt["param_groups"][0]["params"] == list(range(len(heads)))
    assert sorted(opt["state"].keys()) == [i for i, k in enumerate(heads) if k in a.state] and len(opt["state"]) > 0
    for i in opt["state"]:
        assert tuple(opt["state"][i]["exp_avg"].shape) == tuple(ckp["model"][heads[i]].shape), heads[i]
    # torch's own optimiser over the head's parameters takes the state (what get_params_groups leaves of a frozen model)
    ps = [torch.nn.Parameter(ckp["model"][k].clone()) for k in heads]
    torch.optim.AdamW(ps).load_state_dict(opt)
    b, _, _, _ = _build(c)
    b.load_checkpoint(path)
    assert b.t == 2
    _, ta_, _ = a.step(xs, target, samples)
    _, tb_, _ = b.step(xs, target, samples)
    assert ta_ == tb_
    pa, pb = a.parameters(), b.parameters()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    # the two kinds of step do not read each other's optimiser state
    full, _, _, _ = _build(c, trainable="all")
    with pytest.raises(L.BfmError, match="'head'.*'all'"):
        full.load_checkpoint(path)
    full.step(xs, target, samples)
    path_all = str(tmp_path / "full.pth")
    full.save_checkpoint(path_all)
    with pytest.raises(L.BfmError, match="'all'.*'head'"):
        b.load_checkpoint(path_all)
    # the model part is an ordinary checkpoint: same backbone features as before training, other head maps
    ga, ta = TU.default_inference_args(f_maps=c["f_maps"], num_levels=c["levels"], left_hemis_only=True,
                                       num_groups=c["groups"])
    s2 = TU.InferenceSession(ga, ta, _dev(), ckp_path=path, passes=3)
    out2, _ = s2.forward_fused(vol)
    assert torch.equal(out2["feat"][-1], feat0)
    assert not torch.equal(out2["T1"], t1_0)


# ----------------------------------------------------------------------------- 7. hidden head layers, the pooled head
def _head_grads_frozen_and_full(make):
    out = []
    for trainable in ("head", "all"):
        step, xs, target, samples = make(trainable)
        _, total, grads = step.loss_and_grads(xs, target, samples)
        out.append((step, total, grads))
    return out


def test_frozen_step_with_a_hidden_head_layer():
    """task_f_maps = [8, 8] on a 3-level, 8-wide net and a 16^3 crop: the hidden layer is trained (its input gradient is
    not formed), its gradients and the 1x1x1 heads' match the full step's to 2e-3 relative."""
    from brainfm_amd import test_utils as TU, train as TR
    dims = (16, 16, 16)

    def make(trainable):
        ga, ta = TU.default_inference_args(f_maps=8, num_levels=3, left_hemis_only=True, size=dims)
        ta.task_f_maps = [8, 8]
        torch.manual_seed(21)
        s = TU.InferenceSession(ga, ta, _dev(), passes=3)
        tail = s.model.head.tail(s.engine)
        ns = tail.desc.n_seg
        names = ["T1", "seg_ce", "seg_dice", "distance"]
        step = TR.TrainStep(s.engine, tail, names, {"loss_" + n: 1.0 for n in names}, torch.full((ns,), 1.0 / ns), 2, lr=1e-3,
                            trainable=trainable)
        g = torch.Generator().manual_seed(4)
        xs = [torch.rand((1, 1) + dims, generator=g) for _ in range(2)]
        lab = torch.randint(0, ns, (1,) + dims, generator=g)
        target = {"segmentation": torch.nn.functional.one_hot(lab, ns).permute(0, 4, 1, 2, 3).float().contiguous(),
                  "T1": torch.rand((1, 1) + dims, generator=g), "distance": torch.randn((1, 4) + dims, generator=g)}
        return step, xs, target, [{}, {}]

    (fz, tot_f, gf), (full, tot_a, ga_) = _head_grads_frozen_and_full(make)
    heads = _heads(list(fz.parameters().keys()))
    assert "head.layers.0.main.weight" in heads and "head.layers.0.main.bias" in heads
    assert set(gf.keys()) == set(heads)
    assert abs(tot_f - tot_a) <= 1e-4 * abs(tot_a)
    for k in heads:
        e = _rel(gf[k].cpu().numpy(), ga_[k].cpu().numpy())
        print("hidden-layer net, %-36s frozen vs full %.2e" % (k, e))
        assert e <= 2e-3, (k, e)
        assert "head.layers." not in k or float(ga_[k].abs().max()) > 0.0, k
    before = {k: v.clone() for k, v in fz.parameters().items()}
    stepped, _ = fz.apply(gf)
    assert stepped
    for k, v in fz.parameters().items():
        if k not in heads:
            assert torch.equal(v, before[k]), k
        elif "head.layers." in k or k.startswith("head.final_conv_T1."):
            assert not torch.equal(v, before[k]), k               # (a head without a loss has a zero gradient and stays)
    _, tot2, _ = fz.loss_and_grads(*make("head")[1:])             # the repacked hidden layer is what the next pass runs
    assert tot2 != tot_f


def test_frozen_step_with_the_pooled_age_head():
    """The fixture's net (width, levels, groups) with the pooled scalar head at its smallest legal size, 16^3: the age
    head's gradients match the full step's to 2e-3 relative."""
    from brainfm_amd import test_utils as TU, train as TR
    c = load_case()
    dims = (16, 16, 16)

    def make(trainable):
        ga, ta = TU.default_inference_args(f_maps=c["f_maps"], num_levels=c["levels"], num_groups=c["groups"], size=dims,
                                           tasks=dict(T1=True, age=True))
        torch.manual_seed(33)
        s = TU.InferenceSession(ga, ta, _dev(), passes=3)
        step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), ["T1", "age"], {"loss_T1": 1.0, "loss_age": 1.0},
                            torch.ones(1), 2, lr=1e-3, age_head=s.model.head.age_head(), trainable=trainable)
        g = torch.Generator().manual_seed(6)
        xs = [torch.rand((1, 1) + dims, generator=g) for _ in range(2)]
        target = {"T1": torch.rand((1, 1) + dims, generator=g), "age": torch.tensor([0.7], dtype=torch.float64)}
        return step, xs, target, [{}, {}]

    (fz, tot_f, gf), (full, tot_a, ga_) = _head_grads_frozen_and_full(make)
    heads = _heads(list(fz.parameters().keys()))
    age = [k for k in heads if "_age." in k or "pool_layers" in k]
    assert len(age) == 10 and set(gf.keys()) == set(heads)
    assert abs(tot_f - tot_a) <= 1e-4 * abs(tot_a)
    for k in heads:
        e = _rel(gf[k].cpu().numpy(), ga_[k].cpu().numpy())
        print("age net, %-36s frozen vs full %.2e" % (k, e))
        assert e <= 2e-3, (k, e)
        assert float(ga_[k].abs().max()) > 0.0, k
    _, _, stepped = fz.step(*make("head")[1:])
    assert stepped and set(fz.state.keys()) == set(heads)


# ----------------------------------------------------------------------------- 8. refusals
def test_freeze_feat_refusals():
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    c = load_case()
    step, xs, target, samples = _build(c)
    before = {k: v.clone() for k, v in step.parameters().items()}
    with pytest.raises(L.BfmError, match="single-rank"):
        step.step(xs, target, samples, group=object())
    with pytest.raises(L.BfmError, match="one rank"):
        step.grad_store()
    for k, v in step.parameters().items():
        assert torch.equal(v, before[k]), k
    with pytest.raises(L.BfmError, match="freeze_feat"):
        TR.twostage_train_step(SimpleNamespace(), SimpleNamespace(freeze_feat=True), None, None, [1.0], 1)
    with pytest.raises(L.BfmError, match="freeze_feat"):
        TR.contrastive_train_step(SimpleNamespace(tasks=["contrastive"]), SimpleNamespace(freeze_feat=True), None)
    full, _, _, _ = _build(c, trainable="all")
    with pytest.raises(L.BfmError, match="trainable='all'"):
        TR.TwoStageTrainStep(step, full)


def test_factories_read_freeze_feat_beside_the_default_feat_opt_block():
    """train_step on the session's own (gen_args, train_args, model) with the keys the default yaml carries: freeze_feat
    True gives a frozen step that runs (one iteration, head gradients only), False the full step; the feat_opt block is not
    read.  contrastive_train_step builds the step ContrastiveStep's constructor builds: same loss, same gradient bits."""
    import test_gpu_contrastive as TC
    from brainfm_amd import train as TR
    c = load_case()
    s = _session(c)
    ta, ga = s.train_args, s.gen_args
    ta.feat_opt = SimpleNamespace(lr=0.0001, min_lr=0.000001)
    ta.losses.image_grad = True
    ta.weights = SimpleNamespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                                 registration=1.0)
    _, xs, target, samples = _build(c, session=s)
    for freeze, want in ((False, "all"), (True, "head")):
        ta.freeze_feat = freeze
        step = TR.train_step(ga, ta, s.model, c["d"]["weights_ce"], c["all_samples"], lr=c["lr"])
        assert step.trainable == want and "T1_grad" in step.loss_names and "seg_dice" in step.loss_names
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    assert np.isfinite(total) and set(grads.keys()) == set(_heads(c["names"]))
    d, f_maps, levels, groups, size, stride, cxs = TC._case()
    cs, wts, temps = TC._session(d, f_maps, levels, groups, size)
    cs.train_args.feat_opt = ta.feat_opt
    cs.train_args.freeze_feat = False
    a = TR.contrastive_train_step(cs.gen_args, cs.train_args, cs.model, lr=1e-4)
    b = TR.ContrastiveStep(cs.engine, wts, temps, lr=1e-4)
    (_, ta_, ga_), (_, tb_, gb_) = a.loss_and_grads(cxs), b.loss_and_grads(cxs)
    assert ta_ == tb_ and (a.alpha, a.beta, a.gamma) == temps
    for k in ga_:
        assert torch.equal(ga_[k], gb_[k]), k
