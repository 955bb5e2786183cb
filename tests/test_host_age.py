"""The pooled scalar (brain-age) head's parameter tree, built on the host (no GPU): reference state-dict names and shapes
(tests/golden/train_age.npz, made by running the reference's build_model), its processor, its size check, its target."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_age.npz")


def _args(size, tasks=None):
    from brainfm_amd import test_utils as TU
    return TU.default_inference_args(f_maps=8, num_levels=3, size=size, tasks=tasks or dict(T1=True, age=True))


def test_age_model_has_the_reference_state_dict():
    from brainfm_amd import models as M
    d = np.load(GOLDEN)
    ga, ta = _args((48, 48, 48))
    _, ta, model, processors, _, _ = M.build_model(ga, ta, "cpu")
    assert list(ta.out_channels.items()) == [("T1", 1), ("age", -1)]
    sd = model.state_dict()
    want = [str(s) for s in d["sd_names"]]
    assert list(sd.keys()) == want
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in d["param_shapes"]]
    assert [n for n, _ in model.named_parameters()] == [str(s) for s in d["param_names"]]
    assert tuple(sd["head.final_linear1_age.weight"].shape) == (160, 108)
    assert [type(p).__name__ for p in processors] == ["AgeProcessor"]
    # a reference-format state dict loads by suffix (DDP 'module.' prefix included)
    ref = {"module." + k: torch_from(d["sd/" + k]) for k in want}
    M.load_state_dict_by_suffix(model, ref)
    assert np.array_equal(model.state_dict()["head.final_linear3_age.bias"].numpy(), d["sd/head.final_linear3_age.bias"])
    # the dense heads alone reach the fused tail
    assert list(model.head.dense_channels) == ["T1"] and model.head.age_task == "age"


def torch_from(a):
    import torch
    return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("size,n", [((160, 160, 160), 4000), ((128, 128, 128), 2048), ((48, 48, 48), 108)])
def test_age_linear_width_follows_the_reference_formula(size, n):
    from brainfm_amd import models as M
    assert M.age_flat_features(size) == n
    ga, ta = _args(size)
    _, _, model, _, _, _ = M.build_model(ga, ta, "cpu")
    assert model.head.final_linear1_age.in_features == n and model.head.n_flat == n


def test_age_size_whose_flatten_does_not_match_raises():
    from brainfm_amd import _lib as L
    from brainfm_amd import models as M
    ga, ta = _args((40, 40, 40))                     # 4*40//16*40//16*40//16 = 62, pooled 4 x 2^3 = 32
    with pytest.raises(L.BfmError, match="62"):
        M.build_model(ga, ta, "cpu")


def test_age_head_must_be_last():
    from collections import OrderedDict
    from argparse import Namespace
    from brainfm_amd import _lib as L
    from brainfm_amd import models as M
    with pytest.raises(L.BfmError, match="last"):
        M.TaskHead(Namespace(size=[48, 48, 48]), [8], OrderedDict([("age", -1), ("T1", 1)]))


def test_age_target_forms():
    import torch
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    assert "age" in TR.SUPPORTED
    assert TR.TrainStep._age_target({"age": 57.0}) == 57.0
    assert TR.TrainStep._age_target({"age": torch.tensor(57.0, dtype=torch.float64)}) == 57.0
    assert TR.TrainStep._age_target({"age": torch.tensor([57.0])}) == 57.0
    assert TR.TrainStep._age_target({"T1": 1}) is None
    with pytest.raises(L.BfmError):
        TR.TrainStep._age_target({"age": torch.tensor([57.0, 3.0])})
