"""The two-stage (pathology-conditioned) model surface on the host (no GPU): the reference's signatures
(tests/golden/api_signatures_twostage.json), the 8-tuple of build_inpaint_model with the reference's state-dict names
(tests/golden/twostage_small.npz, made by running the reference's own pieces), the stage argument of get_head,
merge_list_of_dict, and the CPU refusal of evaluate_image_twostage."""
import inspect
import json
import os

import pytest
import torch

import twostage_weights as TW

TASKS = dict(T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
             super_resolution=True, surface=False, pathology=True, contrastive=False)
NINE = ["T1", "T2", "FLAIR", "CT", "bias_field_log", "segmentation", "distance", "registration", "high_res_residual"]


def _args(f_maps=8, levels=3, backbone="unet3d+unet3d"):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=f_maps, num_levels=levels, tasks=dict(TASKS))
    ta.backbone = backbone
    return ga, ta


def test_signatures_equal_the_reference():
    from brainfm_amd import misc as MI
    from brainfm_amd import models as M
    from brainfm_amd import twostage as TS
    with open(os.path.join(TW.GOLDEN, "api_signatures_twostage.json")) as f:
        want = json.load(f)
    got = {"evaluate_image_twostage": TS.evaluate_image_twostage, "build_inpaint_model": M.build_inpaint_model,
           "build_conditioned_model": M.build_conditioned_model, "merge_list_of_dict": MI.merge_list_of_dict}
    assert sorted(want) == sorted(got)
    for name, fn in got.items():
        assert str(inspect.signature(fn)) == want[name], name


def test_build_inpaint_model_returns_the_reference_tuple_and_names():
    from brainfm_amd import models as M
    d = TW.load("twostage_small")
    ga, ta = _args(int(d["cfg"][0]), int(d["cfg"][1]))
    res = M.build_inpaint_model(ga, ta, "cpu")
    assert len(res) == 8
    ga, ta, pathol_model, task_model, pathol_processors, task_processors, criterion, postprocessor = res
    assert criterion is None and postprocessor is M.get_postprocessor
    assert list(pathol_model.state_dict().keys()) == [str(s) for s in d["pathol/names"]]
    assert list(task_model.state_dict().keys()) == [str(s) for s in d["task/names"]]
    assert len(pathol_model.state_dict()) == 32 and len(task_model.state_dict()) == 48
    assert pathol_model.postfix == "_pathol" and task_model.postfix == "_task"
    assert [type(p).__name__ for p in pathol_processors] == ["PatholProcessor"]
    assert [type(p).__name__ for p in task_processors] == ["SegProcessor", "DistProcessor"]
    # stage 1 reads two channels: GroupNorm(1, 2) then Conv3d(2, max(f_maps // 2, 2), 3)
    sd = task_model.state_dict()
    assert tuple(sd["backbone.encoders.0.basic_module.SingleConv1.groupnorm.weight"].shape) == (2,)
    assert tuple(sd["backbone.encoders.0.basic_module.SingleConv1.conv.weight"].shape) == (4, 2, 3, 3, 3)
    assert task_model.backbone.in_channels == 2 and pathol_model.backbone.in_channels == 1
    # the reference's state dicts load per model, by suffix (DDP 'module.' prefix included)
    for prefix, model in (("pathol", pathol_model), ("task", task_model)):
        ref = {"module." + k: v for k, v in TW.fixture_state_dict(d, prefix).items()}
        M.load_state_dict_by_suffix(model, ref)
        for k, v in model.state_dict().items():
            assert torch.equal(v, ref["module." + k]), k


def test_build_conditioned_model_counts_the_condition_channels():
    from brainfm_amd import models as M
    d = TW.load("conditioned_wide")
    ga, ta = _args(8, 2, backbone="unet3d")
    ta.condition = "mask+flip"
    res = M.build_conditioned_model(ga, ta, "cpu")
    assert len(res) == 6
    model = res[2]
    assert model.backbone.in_channels == 3 and model.postfix == ""
    assert list(model.state_dict().keys()) == [str(s) for s in d["model/names"]]
    assert "pathology" not in model.head.out_channels
    assert [type(p).__name__ for p in res[3]] == ["SegProcessor", "DistProcessor"]


def test_get_head_stages():
    from brainfm_amd import models as M
    ga, ta = _args()
    ga, ta = M.process_args(ga, ta, task=ga.task)
    assert list(ta.out_channels) == NINE + ["pathology"]
    h0 = M.get_head(ta, ta.task_f_maps, ta.out_channels, True, -1, stage=0)
    h1 = M.get_head(ta, ta.task_f_maps, ta.out_channels, True, -1, stage=1)
    assert list(h0.out_channels.items()) == [("pathology", 1)]
    assert list(h1.out_channels) == NINE
    # without '+' in the backbone the stage is ignored and exclude_keys rules, as before
    ta.backbone = "unet3d"
    assert list(M.get_head(ta, ta.task_f_maps, ta.out_channels, True, -1, stage=0).out_channels) == NINE + ["pathology"]
    assert list(M.get_head(ta, ta.task_f_maps, ta.out_channels, True, -1, stage=1,
                           exclude_keys=["pathology"]).out_channels) == NINE


def test_merge_list_of_dict():
    from brainfm_amd import misc as MI
    a = [{"x": 1, "y": 2}, {"x": 3}]
    b = [{"y": 5, "z": 6}, {"w": 7}]
    out = MI.merge_list_of_dict(a, b)
    assert out is a and a == [{"x": 1, "y": 5, "z": 6}, {"x": 3, "w": 7}]
    with pytest.raises(AssertionError):
        MI.merge_list_of_dict([{}], [{}, {}])


def test_evaluate_image_twostage_refuses_the_cpu():
    from brainfm_amd import _lib as L
    from brainfm_amd import twostage as TS
    with pytest.raises(L.BfmError):
        TS.evaluate_image_twostage(torch.zeros(1, 1, 8, 8, 8), "a.pth", "b.pth", device="cpu")
