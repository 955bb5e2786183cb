"""Hidden task-head layers (task_f_maps longer than one; Trainer/models/head.py:27-31,52-55,152-167) on the host, no
GPU: the model builds with the reference's parameter names and shapes (tests/golden/head_layers*.npz hold the reference's
own key lists), checkpoints load by suffix, the combinations that are not built refuse by naming the knob, and the float64
closed forms the GPU tests lean on (tests/head_layer_refs.py) agree with torch float64 autograd."""
import numpy as np
import pytest
import torch

import head_layer_refs as HR
import twostage_weights as TW

TASKS = dict(T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
             super_resolution=True, surface=False, pathology=False, contrastive=False)


def _args(f_maps, levels, task_f_maps, **tasks):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=f_maps, num_levels=levels, tasks=dict(TASKS, **tasks))
    ta.task_f_maps = list(task_f_maps)
    return ga, ta


@pytest.mark.parametrize("stem", ["head_layers", "head_layers_wide"])
def test_build_model_with_hidden_head_layers_has_the_reference_parameters(stem):
    from brainfm_amd import models as M
    d = TW.load(stem)
    tfm = [int(v) for v in d["task_f_maps"]]
    assert len(tfm) == 2
    ga, ta = _args(int(d["cfg"][0]), int(d["cfg"][1]), tfm)
    model = M.build_model(ga, ta, "cpu")[2]
    own = model.state_dict()
    assert list(own.keys()) == [str(s) for s in d["model/names"]]
    assert [",".join(str(v) for v in t.shape) for t in own.values()] == [str(s) for s in d["model/shapes"]]
    assert tuple(own["head.layers.0.main.weight"].shape) == (tfm[1], tfm[0], 3, 3, 3)
    assert tuple(own["head.final_conv_T1.weight"].shape) == (1, tfm[1], 1, 1, 1)


def test_checkpoint_with_module_prefix_loads_the_hidden_layers(tmp_path):
    from brainfm_amd import models as M
    d = TW.load("head_layers")
    sd = TW.fixture_state_dict(d, "model")
    ga, ta = _args(int(d["cfg"][0]), int(d["cfg"][1]), [int(v) for v in d["task_f_maps"]])
    model = M.build_model(ga, ta, "cpu")[2]
    path = str(tmp_path / "ckp.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}, "epoch": 3}, path)
    M.load_checkpoint(path, [model], model_keys=["model"])
    got = model.state_dict()
    for k in ("head.layers.0.main.weight", "head.layers.0.main.bias", "head.final_conv_segmentation.weight"):
        assert torch.equal(got[k], sd[k]), k


def test_combinations_that_are_not_built_name_the_knob():
    from brainfm_amd import _lib as L
    from brainfm_amd import models as M
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # the mask-conditioned model
        ga, ta = _args(8, 3, [8, 16], pathology=True)
        ta.condition = "mask"
        M.build_conditioned_model(ga, ta, "cpu")
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # the two-stage model
        ga, ta = _args(8, 3, [8, 16], pathology=True)
        ta.backbone = "unet3d+unet3d"
        M.build_inpaint_model(ga, ta, "cpu")
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # the head-less contrastive model
        ga, ta = _args(8, 3, [8, 16], contrastive=True)
        M.build_model(ga, ta, "cpu")
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # the pooled scalar head behind hidden layers
        ga, ta = _args(8, 3, [8, 16], age=True)
        ta.size = [32, 32, 32]
        M.build_model(ga, ta, "cpu")
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # widths the kernels do not take
        M.build_model(*_args(8, 3, [8, 10]), "cpu")
    with pytest.raises(L.BfmError, match="task_f_maps"):                       # the head on a bare feature list
        model = M.build_model(*_args(8, 3, [8, 16]), "cpu")[2]
        model.head([torch.zeros(1, 8, 4, 4, 4)])
    # a single entry builds everywhere, as before
    assert len(M.build_model(*_args(8, 3, [8]), "cpu")[2].head.layers) == 0


@pytest.mark.parametrize("cin,cout,dims", [(3, 5, (4, 5, 6)), (8, 16, (5, 3, 7))])
def test_float64_closed_forms_agree_with_torch_autograd(cin, cout, dims):
    g = torch.Generator().manual_seed(cin * 10 + cout)
    x = torch.randn((1, cin) + dims, generator=g, dtype=torch.float64, requires_grad=True)
    conv = torch.nn.Conv3d(cin, cout, 3, 1, 1).double()
    y = torch.nn.functional.leaky_relu(conv(x), 0.2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    cl = lambda t: t.detach()[0].permute(1, 2, 3, 0).numpy()                   # noqa: E731
    w, b = conv.weight.detach().numpy(), conv.bias.detach().numpy()
    y_ref = HR.forward(cl(x), w, b)
    assert HR.rel_err(y_ref, cl(y)) <= 1e-13
    dp = HR.lrelu_bwd(cl(dy), y_ref)
    assert HR.rel_err(HR.dweight(cl(x), dp), conv.weight.grad.numpy()) <= 1e-13
    assert HR.rel_err(HR.dbias(dp), conv.bias.grad.numpy()) <= 1e-13
    assert HR.rel_err(HR.dinput(dp, w), cl(x.grad)) <= 1e-13
    assert np.count_nonzero(y_ref < 0) > 0 and np.count_nonzero(y_ref > 0) > 0
