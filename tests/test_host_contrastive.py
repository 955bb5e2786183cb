"""The head-less contrastive pre-training mode on the host: the fixture made by running the reference
(tests/golden/make_golden_contrastive.py) against a NumPy restatement of loss_feat_contrastive (criterion.py:96-109), the
processor list, the loss-name builder, the mirrors' signatures and the error TrainStep keeps raising.  CPU only."""
import inspect
from types import SimpleNamespace as NS

import numpy as np
import pytest

from conftest import load_npz


def voxel_loss(p, q, alpha, beta, gamma):
    """log(den) - log(num) per voxel of (b, C, s, r, c) float64 maps; den's inner sum written as p_i * S."""
    S = p.sum(1, keepdims=True)
    num = np.exp(p * q / alpha).sum(1)
    den = (np.exp(p ** 2 / beta) + np.exp((p * S - p ** 2) / gamma)).sum(1)
    return np.log(den) - np.log(num)


def test_fixture_is_self_consistent():
    d = load_npz("train_contrastive.npz")
    p, q = d["feat_0"], d["feat_1"]
    assert p.dtype == np.float64 and p.shape == q.shape and p.shape[1] == int(d["cfg"][0])
    for f in (p, q):
        assert np.abs(np.sqrt((f ** 2).sum(1)) - 1.0).max() <= 1e-12           # unit rows after the processor
    a, b, g = (float(t) for t in d["temperatures"])
    got = voxel_loss(p, q, a, b, g)[0]
    ref = d["voxel_loss"]
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # the two maps are related (the second input is a perturbed copy of the first): num is not flat over the voxels
    num = np.exp(p * q / a).sum(1)
    assert num.max() > 1.5 * num.min()
    assert not np.array_equal(p, q)
    # the whole-volume loss is of the size of the stored voxels' mean, and the total is weight * loss
    full = float(d["loss/loss_contrastive"])
    assert abs(full - ref.mean()) < 0.1 * abs(full)
    w = dict(zip([str(k) for k in d["loss_weight_names"]], d["loss_weights"]))
    assert w["loss_contrastive"] != 1.0
    assert abs(float(d["loss_total"]) - w["loss_contrastive"] * full) <= 1e-12 * abs(full)
    # other tasks are ignored and no head exists
    assert "T1" in [str(t) for t in d["tasks"]] and "contrastive" in [str(t) for t in d["tasks"]]
    assert not [str(n) for n in d["param_names"] if str(n).startswith("head.")]
    for n in d["param_names"]:
        assert np.abs(d["grad/" + str(n)]).max() > 0, n


def _args(tasks):
    from brainfm_amd import test_utils as TU
    return TU.default_inference_args(f_maps=8, num_levels=3, size=(48, 48, 48), tasks=tasks)


def test_get_processors_matches_the_reference_list():
    """Fails on the parent commit: get_processors dropped ContrastiveProcessor."""
    from brainfm_amd import models as M
    d = load_npz("train_contrastive.npz")
    tasks = {str(t): True for t in d["tasks"]}
    ga, ta = _args(tasks)
    ga, ta = M.process_args(ga, ta, ga.task)
    assert dict(ta.out_channels) == {}
    procs = M.get_processors(ga, ta, ga.tasks, "cpu")
    assert [type(p).__name__ for p in procs] == [str(n) for n in d["processor_names"]]
    # the reference's position: after UncertaintyProcessor, before AgeProcessor (joiner.py:238-256)
    ta.losses.uncertainty = "gaussian"
    ta.output_names = []
    procs = M.get_processors(ga, ta, ["contrastive", "age", "segmentation"], "cpu")
    assert [type(p).__name__ for p in procs] == ["UncertaintyProcessor", "ContrastiveProcessor", "AgeProcessor",
                                                  "SegProcessor"]
    ta.losses.uncertainty = None
    assert "ContrastiveProcessor" not in [type(p).__name__ for p in M.get_processors(ga, ta, ["T1", "age"], "cpu")]


def test_build_model_headless():
    from brainfm_amd import models as M
    ga, ta = _args(dict(T1=True, contrastive=True))
    _, ta, model, procs, crit, _ = M.build_model(ga, ta, "cpu")
    assert not list(model.head.parameters()) and [type(p).__name__ for p in procs] == ["ContrastiveProcessor"]
    assert crit is None                                   # no weights / temperatures in train_args: nothing to build from
    ga, ta = _args(dict(T1=True, contrastive=True))
    ta.weights = NS(contrastive=0.75)
    ta.contrastive_temperatures = NS(alpha=0.1, beta=0.2, gamma=0.3)
    crit = M.build_model(ga, ta, "cpu")[4]
    assert type(crit).__name__ == "SetCriterion" and crit.loss_names == ["contrastive"]
    assert dict(crit.weight_dict) == {"loss_contrastive": 0.75}
    assert (crit.temp_alpha, crit.temp_beta, crit.temp_gamma) == (0.1, 0.2, 0.3)
    # every other task set keeps criterion None
    ga, ta = _args(dict(T1=True))
    ta.weights = NS(contrastive=0.75)
    ta.contrastive_temperatures = NS(alpha=0.1, beta=0.2, gamma=0.3)
    assert M.build_model(ga, ta, "cpu")[4] is None


def test_criterion_losses_match_fixture():
    from brainfm_amd import train as TR
    d = load_npz("train_contrastive.npz")
    ta = NS(losses=NS(image_grad=True), weights=NS(contrastive=0.75, image=1.0, image_grad=1.0))
    names, wd = TR.criterion_losses(ta, [str(t) for t in d["tasks"]])
    assert names == [str(n) for n in d["loss_names"]]
    assert list(wd) == [str(n) for n in d["loss_weight_names"]]
    assert wd["loss_contrastive"] == float(d["loss_weights"][0])


def test_mirror_signatures():
    from brainfm_amd import models as M
    d = load_npz("train_contrastive.npz")
    assert str(inspect.signature(M.ContrastiveProcessor.forward)) == str(d["sig_processor_forward"])
    assert str(inspect.signature(M.SetCriterion.loss_feat_contrastive)) == str(d["sig_loss_feat_contrastive"])
    assert str(inspect.signature(M.ContrastiveProcessor.__init__)) == "(self)"


def test_trainstep_still_refuses_contrastive():
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    with pytest.raises(L.BfmError, match="ContrastiveStep"):
        TR.TrainStep(None, None, ["contrastive"], {}, [1.0], 1)
    with pytest.raises(L.BfmError, match="ContrastiveStep"):
        TR.TrainStep(None, None, ["T1", "contrastive"], {}, [1.0], 1)
    assert issubclass(TR.ContrastiveStep, TR.TrainStep)
    assert "contrastive" not in TR.SUPPORTED
