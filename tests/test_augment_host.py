"""The augmentation recipe's one place (`augment.StepPlans`, `augment.AugmentChain`) and the plan classes' shared `part` /
`take`, without a GPU: stages that record their calls stand in for the device stages."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _plans(n=12):
    from lsm_speech_classifier_amd import augment, frontend
    return augment.StepPlans(speed=frontend.speed_plan(n, 3, prob=0.5, seed=4), reverb=frontend.reverb_plan(n, 4, prob=0.5, seed=4),
                             mix=frontend.mix_plan(n, 3, 500, (0.0, 20.0), max_shift=40, level_db=(-6.0, 0.0), seed=4),
                             mask=frontend.mask_plan(n, 40, 100, freq_masks=2, freq_width=9, time_masks=1, time_width=20, seed=4))


def _same(a, b):
    assert type(a) is type(b) and len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


class Stage:
    """A device stage that records its call and hands back a new object: ``result()``, or (its name, its input)."""

    def __init__(self, log, name, result=None):
        self.log, self.name, self.result = log, name, result

    def _call(self, *args, **kw):
        self.log.append((self.name, args, kw))
        return self.result() if self.result else (self.name, args[0])

    perturb = reverb = mix = _call


def _chain(log, result=None, **absent):
    from lsm_speech_classifier_amd import augment
    stages = dict(speed=Stage(log, "speed", result), reverb=Stage(log, "reverb", result), mixer=Stage(log, "mix", result))
    stages.update(absent)
    return augment.AugmentChain(**stages)


# ---- the plan classes' shared part / take ---------------------------------------------------------------------------------
def test_every_plan_class_slices_and_gathers_every_field_into_its_own_type():
    plans = _plans()
    idx = [7, 3, 11, 3, 0]
    for plan in plans:
        part, take = plan.part(2, 9), plan.take(idx)
        assert type(part) is type(plan) and type(take) is type(plan) and len(plan._fields) == len(part) == len(take)
        for field, a in zip(plan._fields, plan):
            assert np.array_equal(getattr(part, field), a[2:9]) and getattr(part, field).dtype == a.dtype, field
            assert np.array_equal(getattr(take, field), a[np.asarray(idx)]) and getattr(take, field).dtype == a.dtype, field
        assert len(plan.part(10, 20)[0]) == 2 and len(plan.part(12, 20)[0]) == 0 and len(plan.take([])[0]) == 0
        _same(plan.take(np.arange(12)), plan)
    assert [len(p._fields) for p in plans] == [1, 1, 5, 2]


# ---- StepPlans -----------------------------------------------------------------------------------------------------------
def test_step_plans_part_and_take_are_the_members_own_and_none_stays_none():
    from lsm_speech_classifier_amd import augment
    plans = _plans()
    assert augment.StepPlans._fields == ("speed", "reverb", "mix", "mask") and augment.StepPlans() == (None,) * 4
    idx = np.array([5, 5, 1, 10])
    for got, want in zip(plans.part(3, 8), (p.part(3, 8) for p in plans)):
        _same(got, want)
    for got, want in zip(plans.take(idx), (p.take(idx) for p in plans)):
        _same(got, want)
    some = plans._replace(reverb=None, mask=None)
    for got in (some.part(3, 8), some.take(idx)):
        assert isinstance(got, augment.StepPlans) and got.reverb is None and got.mask is None
        assert len(got.speed.choice) in (4, 5) and len(got.mix.rows) in (4, 5)
    assert augment.StepPlans().part(0, 4) == augment.StepPlans() == augment.StepPlans().take(idx)
    assert augment.StepPlans().mask_keyword() == {} and set(plans.mask_keyword()) == {"mask"}
    assert plans.mask_keyword()["mask"] is plans.mask


def test_check_covers_raises_each_of_the_four_messages():
    plans = _plans(12)
    plans.check_covers(12)
    _plans(0).check_covers(0)
    type(plans)().check_covers(5)
    short = plans.part(0, 11)
    for keep, text in (("mask", "the mask plan covers 11 / 11 clips, audio has 12"),
                       ("speed", "the speed plan covers 11 clips, audio has 12"),
                       ("reverb", "the reverb plan covers 11 clips, audio has 12"),
                       ("mix", "the plan covers 11 clips, audio has 12")):
        with pytest.raises(ValueError) as e:
            plans._replace(**{keep: getattr(short, keep)}).check_covers(12)
        assert str(e.value) == text
    lopsided = plans._replace(mask=type(plans.mask)(plans.mask.freq, short.mask.time))
    with pytest.raises(ValueError, match="the mask plan covers 12 / 11 clips"):
        lopsided.check_covers(12)


# ---- AugmentChain --------------------------------------------------------------------------------------------------------
def test_apply_calls_speed_reverb_mix_in_order_with_the_plans_arrays():
    log, plans, x = [], _plans(), object()
    got = _chain(log).apply(x, plans)
    assert [name for name, _, _ in log] == ["speed", "reverb", "mix"]
    (_, a0, k0), (_, a1, k1), (_, a2, k2) = log
    assert k0 == k1 == k2 == {"out": None}
    assert len(a0) == 2 and a0[0] is x and a0[1] is plans.speed.choice
    assert len(a1) == 2 and a1[0] == ("speed", x) and a1[1] is plans.reverb.rows            # each stage reads the one before
    m = plans.mix
    assert len(a2) == 6 and a2[0] == ("reverb", ("speed", x))
    assert all(got is want for got, want in zip(a2[1:], (m.snr_db, m.rows, m.offsets, m.shift, m.scale)))
    assert got == ("mix", ("reverb", ("speed", x)))


def test_apply_skips_a_stage_without_a_plan_whatever_the_chain_holds():
    from lsm_speech_classifier_amd import augment
    plans, x = _plans(), object()
    for absent in (("speed",), ("reverb",), ("mix",), ("speed", "mix"), ("speed", "reverb", "mix")):
        log = []
        got = _chain(log).apply(x, plans._replace(**dict.fromkeys(absent)))
        assert [name for name, _, _ in log] == [s for s in ("speed", "reverb", "mix") if s not in absent]
        assert (got is x) == (len(absent) == 3)
    log = []
    assert _chain(log).apply(x, augment.StepPlans(mask=plans.mask)) is x and not log        # the mask is the encoder's
    assert augment.AugmentChain().apply(x, augment.StepPlans()) is x


def test_apply_asks_the_buffer_once_per_stage_that_runs_and_passes_it_as_out():
    class Audio:
        shape = (12, 500)
    for absent in ((), ("reverb",), ("speed", "mix")):
        log, asked = [], []

        def buffer(name, shape):
            asked.append((name, shape))
            return "buffer of " + name

        _chain(log, result=Audio).apply(Audio(), _plans()._replace(**dict.fromkeys(absent)), buffer)
        ran = [s for s in ("speed", "reverb", "mix") if s not in absent]
        assert asked == [(s, (12, 500)) for s in ran]
        assert [(name, kw) for name, _, kw in log] == [(s, {"out": "buffer of " + s}) for s in ran]


def test_apply_and_refuse_raise_the_three_messages():
    plans, x = _plans(), object()
    for plan, stage, text in (("mix", "mixer", "submit(mix=...) needs a HotPath built with a mixer and a step that has a front end"),
                              ("reverb", "reverb",
                               "submit(reverb=...) needs a HotPath built with a reverberator and a step that has a front end"),
                              ("speed", "speed",
                               "submit(speed=...) needs a HotPath built with a speed perturber and a step that has a front end")):
        log = []
        only = type(plans)(**{plan: getattr(plans, plan)})
        with pytest.raises(ValueError) as e:
            _chain(log, **{stage: None}).apply(x, only)
        assert str(e.value) == text and not log                     # refused before any stage ran
        with pytest.raises(ValueError) as e:
            _chain(log).refuse(only, front_end=False)               # a step without a front end takes no plan
        assert str(e.value) == text
        _chain(log).refuse(only)
        _chain(log, **{stage: None}).refuse(type(plans)(mask=plans.mask), front_end=False)
    log = []
    with pytest.raises(ValueError, match="speed perturber"):        # the last stage missing: nothing ran before the refusal
        _chain(log, speed=None).apply(x, plans)
    assert not log


def test_check_device_names_the_stage_that_lives_elsewhere():
    from lsm_speech_classifier_amd import augment

    class On:
        def __init__(self, device):
            self.device = device

    augment.AugmentChain().check_device("cuda:0")
    augment.AugmentChain(On("cuda:0"), On("cuda:0"), On("cuda:0")).check_device("cuda:0")
    for kw, text in ((dict(mixer=On("cuda:1")), "mixer on cuda:1, front end on cuda:0"),
                     (dict(reverb=On("cuda:1")), "reverberator on cuda:1, front end on cuda:0"),
                     (dict(speed=On("cuda:1")), "speed perturber on cuda:1, front end on cuda:0")):
        with pytest.raises(ValueError) as e:
            augment.AugmentChain(**kw).check_device("cuda:0")
        assert str(e.value) == text
