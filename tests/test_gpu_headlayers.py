"""Hidden task-head layers (task_f_maps longer than one; Trainer/models/head.py:27-31,52-55,152-167) on the device: the
layer's forward and backward against the float64 closed forms of tests/head_layer_refs.py, the whole network, the tile
flows and one training iteration against what the reference computed (tests/golden/head_layers*.npz, made by
tests/golden/make_golden_headlayers.py).  Needs an MI355X: run with `-m gpu`."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import head_layer_refs as HR
import twostage_weights as TW
from test_gpu_twostage import _ref_of, _samples_of

pytestmark = pytest.mark.gpu

TOL_NET = 1e-3              # whole network (tests/test_gpu_infer.py:17)
TOL_KERNEL = 1e-5           # one convolution against float64: test_winograd_f43_kernel_vs_float64_convolution's bound
WGRAD_TOL = 2e-5            # a weight gradient (tests/test_gpu_backward.py:231)
COLSUM_TOL = 2e-6           # a column sum (tests/test_gpu_backward.py:158, dbeta)

_SESSIONS = {}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))


def _layer_session(cin, cout):
    """A session whose head has ONE hidden layer cin -> cout (2-level net of width cin), kept for the module."""
    from brainfm_amd import test_utils as TU
    key = (cin, cout)
    if key not in _SESSIONS:
        ga, ta = TU.default_inference_args(f_maps=cin, num_levels=2)
        ta.task_f_maps = [cin, cout]
        torch.manual_seed(cin + cout)
        _SESSIONS[key] = TU.InferenceSession(ga, ta, _dev())
    return _SESSIONS[key]


def _layer_case(cin, cout, dims, seed):
    """(engine, layer record, x, w, b) with w and b written into the session's model; b at the scale of the outputs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(dims + (cin,), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.05
    conv = HR.conv_bias(x.numpy(), w.numpy(), np.zeros(cout))
    b = torch.randn(cout, generator=g) * float(conv.std())
    s = _layer_session(cin, cout)
    main = s.model.head.layers[0].main
    with torch.no_grad():
        main.weight.copy_(w.to(_dev()))
        main.bias.copy_(b.to(_dev()))
    eng = s.engine
    (hl,) = eng.head_layers([cin, cout])
    return eng, hl, x, w, b


# the issue's four, and a volume below the F(4,3) kernel's 8 x 8 x 4 box: the shape rule's other branch (conv_mfma)
FWD_CASES = [(8, 16, (5, 7, 9)), (64, 64, (8, 8, 16)), (64, 64, (11, 9, 14)), (64, 64, (16, 16, 8)), (64, 64, (6, 10, 12))]


@pytest.mark.parametrize("cin,cout,dims", FWD_CASES)
def test_hidden_layer_forward_vs_float64(cin, cout, dims):
    """Conv3d(3, p=1) + bias + LeakyReLU(0.2) of engine.head_conv against the float64 closed form; the bias is as large as
    the convolution's outputs, so a dropped bias fails.  The bound the pass writes is max |y| of what it stored."""
    eng, hl, x, w, b = _layer_case(cin, cout, dims, 7 + dims[2])
    want = HR.forward(x.numpy(), w.numpy(), b.numpy())
    no_bias = HR.forward(x.numpy(), w.numpy(), np.zeros(cout))
    assert HR.rel_err(no_bias, want) > 0.1                      # the test can tell
    xd = x.to(_dev())
    got, nb = eng.head_conv(hl, xd, dims, eng.absmax(xd))
    torch.cuda.synchronize()
    e = HR.rel_err(got, want)
    print("head layer %d->%d %s: kind %s, variant %d, hip-ref64 %.2e" % (cin, cout, dims, hl.kind,
                                                                         eng._head_cfg(hl, dims)[6] if hl.kind == "mfma" else -1, e))
    assert bool(torch.isfinite(got).all())
    assert e <= TOL_KERNEL, e
    assert float(nb) == float(got.abs().max())
    if cin == 64:
        assert hl.kind == "mfma"                                # the matrix core carried it
        assert eng._head_cfg(hl, dims)[6] == (4 if (dims[0] >= 8 and dims[1] >= 8 and dims[2] >= 4) else 0)


def test_hidden_layer_masked_equals_dense_where_the_mask_is_set():
    """The last hidden layer of a tile takes the tile's mask: on a 16^3 image that is zero in half of the 8 x 8 x 4 boxes
    the masked launch is bit-equal to the dense one wherever the image is non-zero."""
    dims = (16, 16, 16)
    eng, hl, x, w, b = _layer_case(64, 64, dims, 23)
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(dims, generator=g) + 0.1
    mask[:8] = 0                                                 # half of the boxes hold no voxel
    mask[8:, :, ::3] = 0                                         # and zeros inside the computed boxes
    xd, md = x.to(_dev()), mask.to(_dev()).contiguous()
    bound = eng.absmax(xd)
    dense, _ = eng.head_conv(hl, xd, dims, bound)
    assert eng._head_cfg(hl, dims)[6] == 4 and eng.mask_skip
    masked, _ = eng.head_conv(hl, xd, dims, bound, mask_img=md, want_bound=False)
    torch.cuda.synchronize()
    on = md != 0
    assert torch.equal(masked[on], dense[on])


@pytest.mark.parametrize("cin,cout,dims", [(8, 16, (5, 7, 9)), (64, 64, (11, 9, 14))])
def test_hidden_layer_backward_vs_float64(cin, cout, dims):
    """backward.backward_head_layer: dP bit-equal to dY * lrelu'(Y), its maximum exact, dbias a column sum, dW and dX
    against the float64 closed forms; every result has the same bits on a second run."""
    from brainfm_amd import backward as BW
    eng, hl, x, w, b = _layer_case(cin, cout, dims, 40 + cin)
    g = torch.Generator().manual_seed(3)
    y64 = HR.forward(x.numpy(), w.numpy(), b.numpy())
    y = torch.from_numpy(y64).to(torch.float32)
    dY = torch.randn(dims + (cout,), generator=g)
    dp64 = HR.lrelu_bwd(dY.numpy(), y.numpy())
    want = {"dW": HR.dweight(x.numpy(), dp64), "db": HR.dbias(dp64), "dX": HR.dinput(dp64, w.numpy())}
    xd, yd, dYd = x.to(_dev()), y.to(_dev()), dY.to(_dev())
    bound = eng.absmax(xd)
    runs = []
    for _ in range(2):
        dX, gr = BW.backward_head_layer(eng, hl, xd, bound, yd, dYd, dims)
        torch.cuda.synchronize()
        runs.append({"dW": gr[hl.name + ".weight"].clone(), "db": gr[hl.name + ".bias"].clone(), "dX": dX.clone()})
    errs = {k: HR.rel_err(runs[0][k], want[k]) for k in want}
    print("head layer backward %d->%d %s: %s" % (cin, cout, dims, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["dW"] <= WGRAD_TOL and errs["db"] <= COLSUM_TOL and errs["dX"] <= TOL_KERNEL, errs
    for k in want:
        assert torch.equal(runs[0][k], runs[1][k]), k
    # the element-wise half on its own: dP and its maximum are exact
    from brainfm_amd import _lib as L
    lib = L.load()
    nv = dims[0] * dims[1] * dims[2]
    dP = torch.full_like(dYd, float("nan"))
    db = torch.full((cout,), float("nan"), device=_dev())
    mx = torch.full((1,), float("nan"), device=_dev())
    ws = torch.empty(lib.bfm_head_bias_lrelu_bwd_workspace(cout, nv), dtype=torch.uint8, device=_dev())
    L.check(lib.bfm_head_bias_lrelu_bwd(L.ptr(dYd), L.ptr(yd), cout, nv, 0.2, L.ptr(dP), L.ptr(db), L.ptr(mx), L.ptr(ws),
                                        ws.numel(), L.stream_ptr()), "head_bias_lrelu_bwd")
    torch.cuda.synchronize()
    ref = dYd * torch.where(yd > 0, torch.ones_like(yd), torch.full_like(yd, 0.2))
    assert torch.equal(dP, ref) and float(mx) == float(ref.abs().max())
    assert torch.equal(db, runs[0]["db"])


# ----------------------------------------------------------------------------- the whole network against the reference
def _golden_session(stem):
    from brainfm_amd import test_utils as TU
    if stem not in _SESSIONS:
        d = TW.load(stem)
        ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]))
        ta.task_f_maps = [int(v) for v in d["task_f_maps"]]
        _SESSIONS[stem] = (d, TU.InferenceSession(ga, ta, _dev(), state_dict=TW.fixture_state_dict(d, "model")))
    return _SESSIONS[stem]


@pytest.mark.parametrize("stem", ["head_layers", "head_layers_wide"])
def test_network_with_hidden_head_layers_against_the_reference(stem):
    """Per key relerr(hip, ref64) <= max(1e-3, 3 relerr(ref32, ref64)); the labels equal the reference's voxel for voxel;
    'feat' stays the backbone's list with its last entry normalised."""
    d, s = _golden_session(stem)
    x = torch.from_numpy(d["x"]).to(_dev())
    out = s.evaluate(x, feature_only=False)
    assert sorted(out.keys()) == sorted(str(k) for k in d["out_keys"])
    for name, (got, j) in _samples_of(out, d).items():
        r32, r64 = _ref_of(d, name, j), _ref_of(d, name, j, "ref64/")
        e, e_ref = _relerr(got, r64), _relerr(r32, r64)
        print("%s %-20s hip-ref64 %.2e   ref32-ref64 %.2e" % (stem, name, e, e_ref))
        assert e <= max(TOL_NET, 3.0 * e_ref), (stem, name, e, e_ref)
    lab = out["label"].cpu().numpy().reshape(-1)
    want = d["label"].reshape(-1).astype(np.int64)
    flips = np.nonzero(lab != want)[0]
    print("%s: %d label flips %s (listed ties: %s)" % (stem, len(flips), flips[:8], d["tie_idx"][:8]))
    assert len(flips) == 0
    kinds = [hl.kind for hl in s.engine.head_layers([int(v) for v in d["task_f_maps"]])]
    assert kinds == (["mfma"] if stem == "head_layers_wide" else ["direct"]), kinds
    assert torch.equal(s.evaluate(x, feature_only=True), out["feat"][-1])
    nrm = out["feat"][-1].float().pow(2).sum(1).sqrt()
    assert float((nrm - 1).abs().max()) < 1e-5                  # hidden activations are not features


def _toy_volume():
    return torch.from_numpy(TW.load("head_layers_tiled")["full"]).to(_dev())


def test_tile_loop_with_hidden_head_layers_against_the_reference():
    """The reference's tile loop on the 48 x 40 x 56 toy volume (window 32, stride 16): every stitched key meets the
    network's rule at the fixture's sampled voxels, the stitched label map equals the reference's voxel for voxel."""
    from brainfm_amd import test_utils as TU
    t = TW.load("head_layers_tiled")
    _, s = _golden_session("head_layers")
    acc, ranges, _ = TU.tiled_inference(_toy_volume(), s, [16] * 3, [32] * 3, graphs=False)
    assert len(ranges) == int(t["n_tiles"])
    idx = torch.from_numpy(t["idx"])
    for j, k in enumerate(str(v) for v in t["keys"]):
        got = acc[k].cpu().reshape(-1)[idx].numpy()
        e, e_ref = _relerr(got, t["ref64/stitched"][j]), _relerr(t["stitched"][j], t["ref64/stitched"][j])
        print("tiled %-18s hip-ref64 %.2e   ref32-ref64 %.2e" % (k, e, e_ref))
        assert e <= max(TOL_NET, 3.0 * e_ref), (k, e, e_ref)
    assert np.array_equal(acc["label"].cpu().numpy(), t["label_full"])


def test_tile_flows_with_hidden_head_layers_are_bit_equal():
    """Graph replay against eager, and the mask and uniform shortcuts on against off: the same stitched bits (64-wide
    head, so the last hidden layer is the masked F(4,3) launch)."""
    from brainfm_amd import test_utils as TU
    _, s = _golden_session("head_layers_wide")
    full = _toy_volume()
    res = {}
    for on in (True, False):
        s.engine.mask_skip = s.engine.uniform_skip = on
        try:
            eager, _, _ = TU.tiled_inference(full, s, [16] * 3, [32] * 3, graphs=False, batched=False)
            res[on] = {k: v.clone() for k, v in eager.items()}
            if on:
                TU.prepare_tile_graphs(full, s, [16] * 3, [32] * 3)
                rep, _, _ = TU.tiled_inference(full, s, [16] * 3, [32] * 3, graphs=True)
                for k in eager:
                    assert torch.equal(rep[k], res[on][k]), ("graph replay", k)
        finally:
            s.engine.mask_skip = s.engine.uniform_skip = True
    assert len(res[True]) >= 15
    for k in res[True]:
        assert bool(torch.isfinite(res[True][k]).all()), k
        assert torch.equal(res[True][k], res[False][k]), ("shortcuts", k)


# ----------------------------------------------------------------------------- one training iteration
def _train_step():
    from brainfm_amd import test_utils as TU, train as TR
    d = TW.load("head_layers_train")
    ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]), left_hemis_only=True)
    ta.task_f_maps = [int(v) for v in d["task_f_maps"]]
    sd = OrderedDict((k[3:], torch.from_numpy(v)) for k, v in d.items() if k.startswith("sd/"))
    s = TU.InferenceSession(ga, ta, _dev(), state_dict=sd)
    eng = s.engine
    names = [str(v) for v in d["loss_names"]]
    weights = {str(k): float(v) for k, v in zip(d["loss_weight_names"], d["loss_weights"])}
    step = TR.TrainStep(eng, s.model.head.tail(eng), names, weights, d["weights_ce"], d["hyper"][0],
                        max_surf_distance=d["hyper"][1], bias_field_log_type=str(d["bias_field_log_type"]), lr=1e-3)
    xs = [torch.from_numpy(d["x%d" % i]) for i in range(2)]
    samples = [{"bias_field_log": torch.from_numpy(d["bias_field_log%d" % i]),
                "high_res_residual": torch.from_numpy(d["high_res_residual%d" % i])} for i in range(2)]
    target = {k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("target/")}
    return d, s, step, xs, target, samples


def test_training_iteration_with_hidden_head_layers_against_float64(tmp_path):
    """One iteration against the reference's float64 run: every loss to 1e-4, every gradient -- head.layers.* included --
    to max(2e-3, 3 x the reference's own fp32 distance); a checkpoint saved after a step reloads to bit-equal outputs."""
    from brainfm_amd import test_utils as TU
    d, s, step, xs, target, samples = _train_step()
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    for k in (str(v) for v in d["loss_weight_names"]):
        if "ref64/loss/" + k in d:
            want = float(d["ref64/loss/" + k])
            print("loss %-24s hip %.6f  ref64 %.6f" % (k, float(loss_dict[k]), want))
            assert abs(float(loss_dict[k]) - want) <= 1e-4 * max(1.0, abs(want)), k
    assert abs(total - float(d["ref64/loss_total"])) <= 1e-4 * abs(float(d["ref64/loss_total"]))
    names = [str(v) for v in d["param_names"]]
    assert set(step.parameters().keys()) == set(names) and set(grads.keys()) == set(names)
    assert [k for k in step.parameters() if k.startswith("head.")] == [n for n in names if n.startswith("head.")]
    assert sum("head.layers." in n for n in names) == 2
    for n in names:
        r64, r32 = d["ref64/grad/" + n], d["ref32/grad/" + n]
        e, e_ref = _relerr(grads[n].cpu().numpy().reshape(r64.shape), r64), _relerr(r32, r64)
        if "head.layers." in n or e > 1e-3:
            print("grad %-60s hip-ref64 %.2e   ref32-ref64 %.2e" % (n, e, e_ref))
        assert e <= max(2e-3, 3.0 * e_ref), (n, e, e_ref)
    # a step, a checkpoint, a fresh session from it: the same bits
    _, _, stepped = step.step(xs, target, samples)
    assert stepped
    path = str(tmp_path / "ckp.pth")
    step.save_checkpoint(path)
    before = torch.from_numpy(d["sd/head.layers.0.main.weight"])
    after = step.state_dict()["head.layers.0.main.weight"]
    assert after.shape == before.shape and not torch.equal(after, before)
    ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]), left_hemis_only=True)
    ta.task_f_maps = [int(v) for v in d["task_f_maps"]]
    s2 = TU.InferenceSession(ga, ta, _dev(), ckp_path=path)
    s3 = TU.InferenceSession(ga, ta, _dev(), state_dict=step.state_dict())
    x0 = xs[0].to(_dev())
    o2, o3 = s2.evaluate(x0, feature_only=False), s3.evaluate(x0, feature_only=False)
    for k in o2:
        if k != "feat":
            assert torch.equal(o2[k], o3[k]), k
