"""The host plumbing the audio stages share ("What a batch stage's host side does"), on CPU tensors: the
refusals of a caller-owned output, word for word as every stage made them before they shared one check, through the
stages' own methods (objects made with ``__new__`` on the CPU: a refusal comes before any device work) and through the
helpers; the lengths conversion; the row chunks; the pointer helpers; the push counts; `pipeline`'s unpacking."""
import numpy as np
import pytest
import torch

CPU = torch.device("cpu")
HOP = 160
REVERB = "an output reads the samples in front of it"
SPEED = "an output reads the samples around it"
TRIM = "a clip moves towards the start of its row"
MIX = "a shift reads across what it would write"


def _stage(cls, **attrs):
    from lsm_speech_classifier_amd import frontend
    obj = getattr(frontend, cls).__new__(getattr(frontend, cls))
    obj.device = CPU
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def _perturber():
    from lsm_speech_classifier_amd import frontend
    tables, row_of_choice = frontend.speed_bank(["11/10"])
    return _stage("SpeedPerturber", factors=["11/10"], tables=tables, row_of_choice=row_of_choice)


def _audio():
    return torch.zeros((3, 3 * HOP), dtype=torch.float32)


# every batch stage: (how to call it with ``out``, the shape its refusal names, its reason clause or None, " on cpu" or "")
def _calls():
    from lsm_speech_classifier_amd import frontend
    return {
        "resample": (lambda a, out: _stage("Resampler", up=1, down=1).resample(a, out=out), "(3, 480)", None, " on cpu"),
        "reverb": (lambda a, out: _stage("Reverberator").reverb(a, out=out), "(3, 480)", REVERB, " on cpu"),
        "perturb": (lambda a, out: _perturber().perturb(a, out=out), "(3, 480)", SPEED, " on cpu"),
        "perturb_ragged": (lambda a, out: _perturber().perturb_ragged(a, [480, 0, 7], out=out), "(3, 480)", SPEED, " on cpu"),
        "trim": (lambda a, out: _stage("SilenceTrimmer", min_bins=3).trim(a, out=out), "(3, >= 480)", TRIM, " on cpu"),
        "mix_arguments": (lambda a, out: frontend.mix_arguments(a, 10.0, out=out), "(3, 480)", MIX, ""),
    }


STAGES = ("resample", "reverb", "perturb", "perturb_ragged", "trim", "mix_arguments")


@pytest.mark.parametrize("stage", STAGES)
def test_every_stage_refuses_a_bad_out_in_its_own_words(stage):
    call, shape, _, where = _calls()[stage]
    text = f"out must be a contiguous float32 {shape} tensor{where}"
    bad = {"dtype": torch.zeros((3, 480), dtype=torch.float64), "rows": torch.zeros((2, 480)), "short": torch.zeros((3, 479)),
           "dims": torch.zeros((3, 480, 1)), "strided": torch.zeros((3, 960))[:, ::2], "ndarray": np.zeros((3, 480), np.float32)}
    assert tuple(bad["strided"].shape) == (3, 480) and not bad["strided"].is_contiguous()
    for name, out in bad.items():
        with pytest.raises(ValueError) as e:
            call(_audio(), out)
        assert str(e.value) == text, (stage, name)
    if stage != "resample":             # (the resampler's own check never asked for a tensor: its words to a list are not pinned)
        with pytest.raises(ValueError) as e:
            call(_audio(), [[0.0] * 480] * 3)
        assert str(e.value) == text


@pytest.mark.parametrize("stage", STAGES[1:])
def test_every_stage_but_the_resampler_refuses_out_over_audio(stage):
    call, _, reason, _ = _calls()[stage]
    audio = _audio()
    for out in (audio, audio[:], audio.view(3, 480)):               # the tensor itself, and another one at the same address
        assert out is audio or out.data_ptr() == audio.data_ptr()
        with pytest.raises(ValueError) as e:
            call(audio, out)
        assert str(e.value) == f"out must not be audio: {reason}"


def test_the_trimmer_takes_a_wider_out_and_the_exact_form_does_not():
    from lsm_speech_classifier_amd import frontend
    wide = torch.zeros((3, 500))
    assert frontend.checked_out(wide, (3, 480), CPU, _audio(), TRIM, at_least=True, word="float32") is wide
    with pytest.raises(ValueError, match=r"^out must be a contiguous float32 \(3, 480\) tensor on cpu$"):
        frontend.checked_out(wide, (3, 480), CPU, word="float32")
    with pytest.raises(ValueError, match=r"^out must be a contiguous float32 \(3, >= 480\) tensor on cpu$"):
        frontend.checked_out(torch.zeros((3, 479)), (3, 480), CPU, at_least=True, word="float32")


def test_aliasing_is_allowed_without_a_reason_and_empty_batches_share_no_address():
    from lsm_speech_classifier_amd import frontend
    audio = _audio()
    assert frontend.checked_out(audio, (3, 480), CPU, audio, None, word="float32") is audio     # `Resampler.resample`
    assert frontend.checked_out(audio, (3, 480), CPU, word="float32") is audio
    a, b = torch.zeros((0, 480)), torch.zeros((0, 480))
    assert a.data_ptr() == b.data_ptr()                             # two empty tensors: equal pointers mean nothing
    assert frontend.checked_out(b, (0, 480), CPU, a, REVERB, word="float32") is b
    with pytest.raises(ValueError, match="must not be audio"):
        frontend.checked_out(a, (0, 480), CPU, a, REVERB, word="float32")          # identity still does
    other = torch.zeros((3, 480))
    assert frontend.checked_out(other, (3, 480), None, audio, MIX) is other                    # no device: none is checked
    with pytest.raises(ValueError, match=r"^rows must be a contiguous int32 \(3,\) tensor$"):   # the word follows the dtype
        frontend.checked_out(other, (3,), None, name="rows", dtype=torch.int32)


def test_the_device_is_part_of_the_check_where_one_is_given():
    from lsm_speech_classifier_amd import frontend
    meta = torch.zeros((3, 480), device="meta")
    with pytest.raises(ValueError, match=r"^out must be a contiguous float32 \(3, 480\) tensor on cpu$"):
        frontend.checked_out(meta, (3, 480), CPU, word="float32")
    assert frontend.checked_out(meta, (3, 480), None, word="float32") is meta


def test_a_stream_bank_checks_its_outputs_with_the_same_function_and_makes_zeros_where_none_is_given():
    bank = _stage("_StreamPush")
    made = bank._owned(None, (2, 3), torch.uint8, "raster_out")
    assert made.dtype == torch.uint8 and tuple(made.shape) == (2, 3) and not made.any() and made.device == CPU
    good = torch.ones((2, 3), dtype=torch.float64)
    assert bank._owned(good, (2, 3), torch.float64, "db_out") is good
    for word, says in ((None, "torch.uint8"), ("uint8", "uint8")):
        for bad in (torch.zeros((2, 3)), torch.zeros((2, 4), dtype=torch.uint8), torch.zeros((2, 6), dtype=torch.uint8)[:, ::2],
                    np.zeros((2, 3), np.uint8)):
            with pytest.raises(ValueError) as e:
                bank._owned(bad, (2, 3), torch.uint8, "raster_out", word)
            assert str(e.value) == f"raster_out must be a contiguous {says} (2, 3) tensor on cpu"
    audio = torch.zeros((2, 3))
    with pytest.raises(ValueError) as e:                            # `ReverbStream.push`
        bank._owned(audio[:], (2, 3), torch.float32, "out", "float32", audio, REVERB)
    assert str(e.value) == f"out must not be audio: {REVERB}"


def test_n_out_defaults_and_is_refused_below_one_before_the_output_is_looked_at():
    from lsm_speech_classifier_amd import frontend
    assert frontend.checked_n_out(None, 7) == 7 and frontend.checked_n_out(3, 7) == 3
    bad_out = torch.zeros((1, 1), dtype=torch.float64)
    calls = (lambda n: _stage("Resampler", up=1, down=1).resample(_audio(), n, bad_out),
             lambda n: _stage("Reverberator").reverb(_audio(), None, n, bad_out),
             lambda n: _perturber().perturb(_audio(), None, n, bad_out),
             lambda n: _perturber().perturb_ragged(_audio(), [0, 0, 0], None, n, None, bad_out))
    for call in calls:
        for n in (0, -5):
            with pytest.raises(ValueError) as e:
                call(n)
            assert str(e.value) == f"n_out must be >= 1, got {n}"


def test_lengths_from_the_host_are_checked_and_become_int32():
    from lsm_speech_classifier_amd import frontend
    for given in ([0, 5, 480], (0, 5, 480), np.array([0, 5, 480]), np.array([0, 5, 480], dtype=np.uint16),
                  torch.tensor([0, 5, 480]), torch.tensor([0, 5, 480], dtype=torch.int32)):
        got = frontend.checked_lengths(given, 3, 480, CPU)
        assert got.dtype == torch.int32 and got.tolist() == [0, 5, 480] and got.device == CPU
        assert frontend.checked_lengths(given, 3, 480, None).tolist() == [0, 5, 480]           # checked only: still on the host
    for given, got in (([1, 2], "int64 (2,)"), ([[1, 2, 3]], "int64 (1, 3)"), (7, "int64 ()"), ([1.0, 2.0, 3.0], "float64 (3,)"),
                       (torch.zeros(3), "float32 (3,)"), ([True, False, True], "bool (3,)")):
        with pytest.raises(ValueError) as e:
            frontend.checked_lengths(given, 3, 480, CPU)
        assert str(e.value) == f"lengths must be 3 integers, got {got}"
    with pytest.raises(ValueError) as e:
        frontend.checked_lengths([-1, 480, 481], 3, 480, CPU)
    assert str(e.value) == "lengths [-1, 481] of clips [0, 2] outside [0, 480]"
    with pytest.raises(ValueError) as e:
        frontend.checked_lengths(np.array([0, 481, 0]), 3, 480, CPU)
    assert str(e.value) == "lengths [481] of clips [1] outside [0, 480]"


def test_the_ragged_mixer_keeps_its_own_lengths_conversion_and_its_words():
    """`NoiseMixer.mix_ragged` checks no range (the kernel clamps), takes one number for every clip and any int32 tensor as it
    is: not `checked_lengths`.  Its refusals are the parent's, and what it accepts reaches `_mix` as an int32 tensor."""
    mixer, seen = _stage("NoiseMixer"), []
    mixer._mix = lambda audio, lengths, *rest: seen.append(lengths)
    for given, want in (([-1, 481, 7], [-1, 481, 7]), (np.array([2, 3, 4], dtype=np.int64), [2, 3, 4]), (7, [7, 7, 7]),
                        (torch.tensor([1, 2, 3], dtype=torch.int32), [1, 2, 3])):
        mixer.mix_ragged(_audio(), given, 10.0, None, None, None, None)
        assert seen[-1].dtype == torch.int32 and seen[-1].tolist() == want and seen[-1].device == CPU
    for bad, text in (([1, 2], "lengths must be a number or 3 of them, got shape (2,)"),
                      ([[1, 2, 3]], "lengths must be a number or 3 of them, got shape (1, 3)"),
                      ([0.5, 1.0, 2.0], "lengths must be integers that fit int32, got array([0.5"),      # (then NumPy's repr)
                      (None, "lengths must be integers that fit int32, got array(None"),
                      ([2 ** 40, 0, 0], "lengths must be integers that fit int32, got array([1099511627776"),
                      (torch.tensor([1, 2, 3]), "lengths must be an int32 (3,) tensor or 3 host integers"),
                      (torch.zeros(2, dtype=torch.int32), "lengths must be an int32 (3,) tensor or 3 host integers")):
        with pytest.raises(ValueError) as e:
            mixer.mix_ragged(_audio(), bad, 10.0, None, None, None, None)
        assert str(e.value) == text or ("got array(" in text and str(e.value).startswith(text)), bad
    assert len(seen) == 4


def test_the_stages_refuse_host_lengths_as_the_trimmer_did():
    sp = _perturber()
    for bad, text in (([1, 2], "lengths must be 3 integers, got int64 (2,)"),
                      ([0, 481, -2], "lengths [481, -2] of clips [1, 2] outside [0, 480]")):
        with pytest.raises(ValueError) as e:
            sp.perturb_ragged(_audio(), bad)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:                            # lengths are refused before the output
        sp.perturb_ragged(_audio(), [1, 2], out=torch.zeros((1, 1)))
    assert str(e.value) == "lengths must be 3 integers, got int64 (2,)"


@pytest.mark.parametrize("n", [0, 1, 4, 5, 9])
def test_row_chunks_tile_the_batch_in_order(n):
    from lsm_speech_classifier_amd import frontend
    chunks = list(frontend.row_chunks(n, 4))
    assert all(1 <= k <= 4 for _, k in chunks) and len(chunks) == -(-n // 4)
    at = 0
    for r0, k in chunks:
        assert r0 == at
        at += k
    assert at == n
    assert list(frontend.row_chunks(n, frontend.SPEED_MAX_ROWS)) == ([(0, n)] if n else [])
    assert frontend.Resampler.MAX_ROWS == frontend.REVERB_MAX_ROWS == frontend.SPEED_MAX_ROWS == 65535


def test_one_pair_of_pointer_helpers_and_none_stays_none():
    from lsm_speech_classifier_amd import frontend, pipeline, snn
    assert frontend._dev(None) is None and frontend._dev(None, 3) is None
    assert snn._dev is frontend._dev and snn._host is frontend._host
    assert pipeline._dev is frontend._dev and pipeline._host is frontend._host
    t = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    assert frontend._dev(t).value == t.data_ptr() == frontend._dev(t, 0).value
    assert frontend._dev(t, 2).value == t.data_ptr() + 2 * 3 * 4 == t[2:].data_ptr()
    v = torch.arange(5, dtype=torch.int32)
    assert frontend._dev(v, 3).value == v.data_ptr() + 12
    a = np.arange(3, dtype=np.float64)
    assert frontend._host(a).value == a.ctypes.data


def test_a_push_refuses_its_hops_in_the_words_of_the_other_counts():
    from lsm_speech_classifier_amd import frontend
    bank = _stage("GammatoneStream", n_streams=3, hop=HOP)
    audio = np.zeros((3, 4 * HOP), dtype=np.float32)
    for bad in ([5, 0, 0], [-1, 0, 0], [1, 2], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError) as e:
            bank._pushed(audio, bad)
        assert str(e.value) == f"hops must be 3 integers in [0, 4], got {bad!r}"
        with pytest.raises(ValueError) as e:
            frontend.checked_counts(bad, 3, 4, "hops")
        assert str(e.value) == f"hops must be 3 integers in [0, 4], got {bad!r}"
    _, H, new = bank._pushed(audio, None)
    assert H == 4 and new.dtype == np.int64 and new.tolist() == [4, 4, 4]
    _, _, new = bank._pushed(audio, np.array([0, 4, 2], dtype=np.int32))
    assert new.dtype == np.int64 and new.tolist() == [0, 4, 2]
    with pytest.raises(ValueError, match=r"^audio must be \(3, H \* 160\) with H >= 1, got \(3, 100\)$"):
        bank._pushed(np.zeros((3, 100), dtype=np.float32), None)


def test_the_listing_functions_share_one_unpacking_and_one_pinned_copy():
    from lsm_speech_classifier_amd import frontend, pipeline
    stages, plans = pipeline._stages_and_plans(None, None, None)
    assert stages == dict(speed=None, reverb=None, mixer=None) and plans == pipeline.StepPlans()
    sp, rv, mx = object(), object(), object()
    speeds, rooms = frontend.speed_plan(3, 2), frontend.reverb_plan(3, 2)
    mixes, masks = frontend.mix_plan(3, 2, 100, 10.0), frontend.mask_plan(3, 8, 10, 1, 2, 1, 2)
    stages, plans = pipeline._stages_and_plans((sp, speeds), (rv, rooms), (mx, mixes), masks, 3)
    assert stages["speed"] is sp and stages["reverb"] is rv and stages["mixer"] is mx
    assert plans.speed is speeds and plans.reverb is rooms and plans.mix is mixes and plans.mask is masks
    chain = pipeline.AugmentChain(**stages)
    assert chain.speed is sp and chain.reverb is rv and chain.mixer is mx
    pipeline._stages_and_plans((sp, speeds), None, None)                                # no count given: none checked
    for args, text in ((((sp, speeds), None, None, None), "the speed plan covers 3 clips, audio has 4"),
                       ((None, (rv, rooms), None, None), "the reverb plan covers 3 clips, audio has 4"),
                       ((None, None, (mx, mixes), None), "the plan covers 3 clips, audio has 4"),
                       ((None, None, None, masks), "the mask plan covers 3 / 3 clips, audio has 4")):
        with pytest.raises(ValueError) as e:
            pipeline._stages_and_plans(*args, 4)
        assert str(e.value) == text
    x = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]
    t = pipeline._pinned_float32(x)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.tolist() == x.tolist() and t.device == CPU
    empty = pipeline._pinned_float32(np.zeros((0, 4)))
    assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.float32
