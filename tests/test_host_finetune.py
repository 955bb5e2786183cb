"""Head-only fine-tuning on a frozen backbone (train_args.freeze_feat): the host-side pieces -- which parameter names a
step trains, and how the factories read the switch.  No device needed."""
from types import SimpleNamespace

import pytest

from test_oracle_train import load_case


def test_trainable_names_splits_the_fixture_parameter_list():
    from brainfm_amd import train as TR
    names = load_case()["names"]
    heads = [n for n in names if n.startswith("head.")]
    assert heads and len(heads) < len(names)
    assert TR.trainable_names(names, "head") == heads             # exactly the head's names, in the list's order
    assert TR.trainable_names(names, "all") == list(names)
    assert TR.trainable_names([], "head") == []
    with pytest.raises(ValueError, match="'all'.*'head'"):
        TR.trainable_names(names, "encoder")
    with pytest.raises(ValueError):
        TR.trainable_names(names, None)


# the block cfgs/trainer/default_train.yaml:90-92 always carries; no line of the reference reads it
DEFAULT_FEAT_OPT = SimpleNamespace(lr=0.0001, min_lr=0.000001)


def test_freeze_feat_key_missing_reads_as_false():
    from brainfm_amd import train as TR
    assert TR.freeze_feat_of(SimpleNamespace()) is False
    assert TR.freeze_feat_of(SimpleNamespace(freeze_feat=False)) is False
    assert TR.freeze_feat_of(SimpleNamespace(freeze_feat=True, feat_opt=None)) is True
    assert TR.freeze_feat_of({"freeze_feat": True}) is True and TR.freeze_feat_of({}) is False
    # the default config's feat_opt block changes nothing, whatever freeze_feat says
    assert TR.freeze_feat_of(SimpleNamespace(freeze_feat=False, feat_opt=DEFAULT_FEAT_OPT)) is False
    assert TR.freeze_feat_of(SimpleNamespace(freeze_feat=True, feat_opt=DEFAULT_FEAT_OPT)) is True
    assert TR.freeze_feat_of({"feat_opt": {"lr": 0.0001, "min_lr": 0.000001}}) is False


class _Reached(Exception):
    pass


def test_factories_take_the_default_config_feat_opt_block(monkeypatch):
    """train_args as the default yaml gives them (feat_opt present, freeze_feat False) pass every factory's reading of the
    switch: each one goes on to its model (a stand-in that says so) or to its own, older refusals instead of raising for the
    dead key; with freeze_feat True the plain and the conditioned factory ask for trainable='head'."""
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR

    class Model:
        class backbone:
            @staticmethod
            def engine(head):
                raise _Reached()
        head = None

    seen = {}

    class Step:
        def __init__(self, *a, **kw):
            seen.update(kw)

    losses = SimpleNamespace(image_grad=False)
    weights = SimpleNamespace(image=1.0, contrastive=1.0, pathol_ce=1.0, pathol_dice=1.0)
    for freeze in (False, True):
        ta = SimpleNamespace(freeze_feat=freeze, feat_opt=DEFAULT_FEAT_OPT, condition="mask", losses=losses, weights=weights,
                             contrastive_temperatures=SimpleNamespace(alpha=0.1, beta=0.1, gamma=0.1))
        ga = SimpleNamespace(tasks=["T1"], max_surf_distance=3.0)
        if freeze:
            with pytest.raises(L.BfmError, match="freeze_feat"):
                TR.twostage_train_step(ga, ta, Model, Model, [1.0], 1)
            with pytest.raises(L.BfmError, match="freeze_feat"):
                TR.contrastive_train_step(SimpleNamespace(tasks=["contrastive"]), ta, Model)
        else:
            with pytest.raises(_Reached):
                TR.twostage_train_step(ga, ta, Model, Model, [1.0], 1)
            with pytest.raises(_Reached):
                TR.contrastive_train_step(SimpleNamespace(tasks=["contrastive"]), ta, Model)

    class Eng:
        in_channels = 2

    class Built:
        class backbone:
            @staticmethod
            def engine(head):
                return Eng

        class head:
            age_task = None

            @staticmethod
            def tail(eng):
                return None

    monkeypatch.setattr(TR, "TrainStep", Step)
    for freeze, want in ((False, "all"), (True, "head")):
        ta = SimpleNamespace(freeze_feat=freeze, feat_opt=DEFAULT_FEAT_OPT, condition="mask", losses=losses, weights=weights)
        ga = SimpleNamespace(tasks=["T1"], max_surf_distance=3.0)
        for factory in (TR.train_step, TR.conditioned_train_step):
            seen.clear()
            factory(ga, ta, Built, [1.0], 1)
            assert seen["trainable"] == want, (factory.__name__, freeze)


def test_front_doors_refuse_freeze_feat_by_name_and_unknown_trainable():
    """The refusals that need no device: the two-stage and the contrastive factory (before they touch a model), and a
    TrainStep with a value of `trainable` nobody defined."""
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    with pytest.raises(L.BfmError, match="freeze_feat"):
        TR.twostage_train_step(SimpleNamespace(), SimpleNamespace(freeze_feat=True), None, None, [1.0], 1)
    with pytest.raises(L.BfmError, match="freeze_feat"):
        TR.contrastive_train_step(SimpleNamespace(tasks=["contrastive"]), SimpleNamespace(freeze_feat=True), None)
    with pytest.raises(ValueError, match="trainable"):
        TR.TrainStep(None, None, ["T1"], {}, [1.0], 1, trainable="encoder")
