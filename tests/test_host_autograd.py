"""brainfm_amd.autograd on the host, no GPU: the float64 closed forms of the processors' backward kernels
(tests/autograd_refs.py) against torch's float64 autograd of oracle.train_ref.processors, their derived fp32 bounds against
an fp32 model of the kernels with named mistakes, and what differentiable(model) shares with the model and refuses."""
import numpy as np
import pytest
import torch

import autograd_refs as AR
from oracle import train_ref as TRF

TASKS = dict(T1=True, T2=False, FLAIR=False, CT=False, segmentation=True, distance=True, bias_field=False,
             registration=False, super_resolution=False, surface=False, pathology=True, contrastive=False)


def _args(f_maps=8, levels=3, **tasks):
    from brainfm_amd import test_utils as TU
    return TU.default_inference_args(f_maps=f_maps, num_levels=levels, left_hemis_only=True, tasks=dict(TASKS, **tasks))


def _autograd64(key, x, g, shape):
    """d(sum(processors(x) * g)) / dx in float64 through the oracle's processors; x, g (n, C) rows -> (1,C,n,1,1)."""
    xt = torch.from_numpy(np.asarray(x, np.float64).T.reshape(shape).copy()).requires_grad_(True)
    gt = torch.from_numpy(np.asarray(g, np.float64).T.reshape(shape).copy())
    out = TRF.processors({key: xt}, max_surf_distance=3.0)[key]
    (out * gt).sum().backward()
    return out.detach().numpy().reshape(shape[1], -1).T, xt.grad.numpy().reshape(shape[1], -1).T


# ----------------------------------------------------------------------------- closed forms vs torch float64 autograd
@pytest.mark.parametrize("C", [2, 7, 56])
def test_softmax_closed_form_is_torch_autograd(C):
    x, g = AR.softmax_case(C, 33, seed=C)
    p, ref = _autograd64("segmentation", x, g, (1, C, 33, 1, 1))
    got = AR.softmax_bwd64(p, g)
    assert np.abs(got - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
    assert p[0].max() == 1.0 and np.abs(got[0]).max() < 1e-24      # the one-hot-sharp row: p (g - s) vanishes


def test_sigmoid_closed_form_is_torch_autograd():
    x, g = AR.sigmoid_case(64, seed=3)
    y, ref = _autograd64("pathology", x[:, None], g[:, None], (1, 1, 64, 1, 1))
    got = AR.sigmoid_bwd64(y, g[:, None])
    assert np.abs(got - ref).max() <= 1e-15
    assert y[0, 0] == 1.0 and got[0, 0] == 0.0                      # saturated: no gradient


def test_clamp_closed_form_is_torch_autograd():
    x, g = AR.clamp_case(64, seed=4)
    x, g = x[[0, 1, 2, 3] + list(range(5, 64))], g[[0, 1, 2, 3] + list(range(5, 64))]   # autograd of a NaN: left to the kernel test
    _, ref = _autograd64("distance", x[:, None], g[:, None], (1, 1, x.size, 1, 1))
    got = AR.clamp_bwd64(x[:, None], g[:, None], -3.0, 3.0)
    assert np.array_equal(got, ref)
    assert got[0, 0] == g[0] and got[1, 0] == g[1] and got[2, 0] == 0.0 and got[3, 0] == 0.0   # edges pass, inclusive


# ----------------------------------------------------------------------------- the bounds hold and notice the mistakes
@pytest.mark.parametrize("C", [2, 7, 56])
def test_softmax_bound_holds_for_the_fp32_model_and_notices_a_missing_sum(C):
    x, g = AR.softmax_case(C, 4099, seed=10 + C)
    p = AR.softmax32(x)
    ref, bound = AR.softmax_bwd64(p, g), AR.softmax_bwd_bound(p, g)
    worst = AR.check(AR.simulate_softmax_bwd(p, g), ref, bound, "softmax_bwd C=%d" % C)
    print("softmax_bwd model C=%d: worst error %.2f of its bound" % (C, worst))
    with pytest.raises(AssertionError, match="over the bound"):
        AR.check(AR.simulate_softmax_bwd(p, g, mistake="no_sum"), ref, bound, "no_sum")


def test_sigmoid_bound_holds_and_notices_the_input_taken_for_the_output():
    x, g = AR.sigmoid_case(4099, seed=5)
    y = AR.sigmoid32(x)
    ref, bound = AR.sigmoid_bwd64(y, g), AR.sigmoid_bwd_bound(y, g)
    AR.check(AR.simulate_unary_bwd("sigmoid", y, g), ref, bound, "sigmoid_bwd")
    with pytest.raises(AssertionError, match="over the bound"):
        AR.check(AR.simulate_unary_bwd("sigmoid", y, g, mistake="from_input", x=x), ref, bound, "from_input")


def test_clamp_bound_is_exact_and_notices_exclusive_edges():
    x, g = AR.clamp_case(4099, seed=6)
    ref, bound = AR.clamp_bwd64(x, g, -3.0, 3.0), AR.clamp_bwd_bound(x, g, -3.0, 3.0)
    AR.check(AR.simulate_unary_bwd("clamp", x, g, -3.0, 3.0), ref, bound, "clamp_bwd")
    with pytest.raises(AssertionError, match="over the bound"):
        AR.check(AR.simulate_unary_bwd("clamp", x, g, -3.0, 3.0, mistake="exclusive"), ref, bound, "exclusive")


# ----------------------------------------------------------------------------- the module surface
def test_differentiable_shares_parameter_objects_and_state_dict_keys():
    from brainfm_amd import autograd as AG
    from brainfm_amd import models as M
    model = M.build_model(*_args(), "cpu")[2]
    dm = AG.differentiable(model)
    a, b = list(dm.parameters()), list(model.parameters())
    assert len(a) == len(b) and all(p is q for p, q in zip(a, b))
    assert [k for k, _ in dm.named_parameters()] == [k for k, _ in model.named_parameters()]
    assert list(dm.state_dict().keys()) == list(model.state_dict().keys())
    for k, v in model.state_dict().items():
        assert dm.state_dict()[k].data_ptr() == v.data_ptr(), k
    assert all(p.requires_grad for p in a)                       # building the counterpart changes no requires_grad state
    dm.load_state_dict(model.state_dict())                      # checkpoints pass between the two unchanged


def test_cpu_inputs_raise_no_cpu_fallback():
    from brainfm_amd import _lib as L
    from brainfm_amd import autograd as AG
    from brainfm_amd import models as M
    ga, ta, model, processors = M.build_model(*_args(), "cpu")[:4]
    dm = AG.differentiable(model)
    x = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(L.BfmError, match="no CPU fallback"):
        dm([{"input": x}])
    with pytest.raises(L.BfmError, match="no CPU fallback"):
        dm.backbone.get_feature(x)
    with pytest.raises(L.BfmError, match="no CPU fallback"):
        dm.backbone(x)
    procs = AG.differentiable_processors(processors)
    assert len(procs) == len(processors) == 3
    outs = [{"segmentation": torch.zeros(1, 18, 2, 2, 2), "distance": torch.zeros(1, 2, 2, 2, 2),
             "pathology": torch.zeros(1, 1, 2, 2, 2)}]
    for p in procs:
        with pytest.raises(L.BfmError, match="no CPU fallback"):
            p(outs)


def test_refused_configurations_raise_by_name():
    from brainfm_amd import _lib as L
    from brainfm_amd import autograd as AG
    from brainfm_amd import models as M
    ga, ta = _args()
    ta.task_f_maps = [8, 8]
    with pytest.raises(NotImplementedError, match="task_f_maps"):
        AG.differentiable(M.build_model(ga, ta, "cpu")[2])
    ga, ta = _args(age=True, segmentation=False, distance=False, pathology=False)
    ga.generator.size = [16, 16, 16]
    with pytest.raises(NotImplementedError, match="pooled age head"):
        AG.differentiable(M.build_model(ga, ta, "cpu")[2])
    ga, ta = _args()
    ta.condition = "mask"
    with pytest.raises(NotImplementedError, match="conditioned"):
        AG.differentiable(M.build_conditioned_model(ga, ta, "cpu")[2])
    ga, ta = _args()
    ta.backbone = "unet3d+unet3d"
    built = M.build_inpaint_model(ga, ta, "cpu")
    for stage in (built[2], built[3]):
        with pytest.raises(NotImplementedError, match="two-stage|conditioned"):
            AG.differentiable(stage)
    model = M.build_model(*_args(), "cpu")[2]
    dm = AG.differentiable(model)
    x = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(NotImplementedError, match="conditioned"):
        dm([{"input": x}], cond=[x])
    with pytest.raises(L.BfmError, match="expected the model"):
        AG.differentiable(model.backbone)
    with pytest.raises(L.BfmError, match="no counterpart"):
        AG.differentiable_processors([torch.nn.Identity()])
