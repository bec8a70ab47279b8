"""The resampler's and the reverberation's NumPy restatements (resample_restatement.py, reverb_restatement.py) against the
operations' definitions (fir_definition.py), on the CPU, for every tap table and row length that the GPU tests use: the
restatements stay within the derived bound per output, and the bound is not vacuous -- a restatement with each row's last
tap dropped, with the phase taken one too far, with a row one tap short or with the input one sample late leaves it."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fir_definition as D  # noqa: E402
import resample_restatement as R  # noqa: E402
import reverb_restatement as RR  # noqa: E402

PACKAGED = (8000, 11025, 22050, 32000, 44100, 48000, 96000)
# blocks of `down` samples: a few thousand outputs at most
BLOCKS = {8000: 400, 11025: 3, 22050: 4, 32000: 500, 44100: 6, 48000: 500, 96000: 300}


def _tables():
    from lsm_speech_classifier_amd import frontend
    cases = [(f"{rate}Hz", (lambda rate=rate: frontend.resample_table(rate)), BLOCKS[rate]) for rate in PACKAGED]
    cases += [(f"{up}/{down}-K{K}", (lambda a=(up, down, K): D.range_table(*a)), None) for up, down, K in D.RANGE_TABLES]
    return cases


def _last_taps_dropped(t):
    """The table without the last tap of every phase: the last ``up`` taps (every one of them ends another row)."""
    taps = np.array(t.taps, dtype=np.float64)
    dropped = taps[max(0, len(taps) - t.up):].copy()
    taps[max(0, len(taps) - t.up):] = 0.0
    return SimpleNamespace(taps=taps, up=t.up, down=t.down, delay=t.delay, history=t.history), dropped


def _phase_one_further(t):
    """The table read with the phase taken as (p + 1) % up: phase r holds the taps of phase (r + 1) % up."""
    J = -(-len(t.taps) // t.up)
    rows = np.zeros(J * t.up, dtype=np.float64)
    rows[:len(t.taps)] = t.taps
    rows = np.roll(rows.reshape(J, t.up), -1, axis=1)
    return SimpleNamespace(taps=rows.ravel(), up=t.up, down=t.down, delay=t.delay, history=t.history)


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("name,make,blocks", _tables(), ids=[c[0] for c in _tables()])
def test_resample_restatement_meets_the_bound_and_mutations_leave_it(name, make, blocks, dtype):
    t = make()
    K, up = len(t.taps), t.up
    if blocks is None:
        x = D.range_input(t, dtype)
        count, delays = D.RANGE_N_OUT, D.range_delays(t)
    else:
        x = D.pcm_noise(3, blocks * t.down, K, dtype)
        count, delays = blocks * t.up, [0, t.delay]
    no_last, dropped = _last_taps_dropped(t)
    # a dropped tap below 2^-30 of the largest is under every bound: a float32 output cannot show it
    carries = np.abs(dropped).max() > 2.0 ** -30 * np.abs(t.taps).max()
    shifted = _phase_one_further(t)
    runs = [D.resample(row, t, 0, count + max(delays)) for row in x]    # one causal run per row serves every delay
    for first in delays:
        far = {"last tap": 0.0, "phase": 0.0}
        for b, row in enumerate(x):
            ref, S = (v[first:first + count] for v in runs[b])
            bound = D.resample_bound(ref, S, t)
            assert np.isfinite(ref).all() and ref.any() and (bound > 0).all()
            D.check(R.causal(row, t, first, count), ref, bound, f"{name} {np.dtype(dtype).name} z[{first}:] row {b}")
            far["last tap"] = max(far["last tap"], D.worst(R.causal(row, no_last, first, count), ref, bound))
            far["phase"] = max(far["phase"], D.worst(R.causal(row, shifted, first, count), ref, bound))
        print(f"{name} z[{first}:]: last taps dropped {far['last tap']:.3g} bounds off, phase + 1 {far['phase']:.3g}")
        if carries:
            assert far["last tap"] > 1.0, "the bound lets a dropped tap pass"
        else:
            # 32, 48 and 96 kHz: one phase, whose last tap is the sinc's zero at 10 periods (|tap| ~ 1e-20)
            assert up == 1 and blocks is not None and far["last tap"] <= 1.0
        if up > 1:
            assert far["phase"] > 1.0, "the bound lets a wrong phase pass"
        else:
            assert far["phase"] <= 1.0                              # (p + 1) % 1 is p % 1: there is no other phase to take


def test_both_forms_of_the_definition_give_the_same_values():
    """`full_literal` is np.convolve of the zero-stuffed signal itself; `full_by_columns` leaves the stuffed zeros out."""
    for up, down, K in ((5, 4, 10), (7, 3, 5), (2, 1, 1), (3, 2, 2000), (1, 2, 1100), (160, 441, 700), (33, 7, 40)):
        t = D.range_table(up, down, K)
        x = R.widen(D.pcm_noise(1, 300, K, np.float32)[0]).astype(D.LD)
        x[17] = 0.0
        pos = np.arange(0, 300 * up + K + 50, down, dtype=np.int64)     # to the end of `full` and past it
        taps = t.taps.astype(D.LD)
        a, b = D.full_literal(x, taps, up, pos), D.full_by_columns(x, taps, up, pos)
        assert a.dtype == b.dtype == D.LD and (a == b).all() and a.any(), (up, down, K)
        assert not a[pos >= 300 * up + K - 1].any()
    # past LITERAL_MACS `resample` takes the second form; below it, the first
    t = D.range_table(640, 441, 19840)
    x = D.pcm_noise(1, 40, 1, np.int16)[0]
    z, _ = D.resample(x, t, 3, 50)
    assert len(x) * t.up * len(t.taps) > D.LITERAL_MACS
    assert (z == D.full_literal(R.widen(x).astype(D.LD), t.taps.astype(D.LD), t.up, np.arange(3, 53) * t.down)).all()


def test_the_resampler_definition_by_hand():
    """up = 2, down = 3, taps 1 2 3 4 5 over x = 1 10 100: stuffed 1 0 10 0 100 0, full = 1 2 13 24 135 240 350 400 500 0."""
    t = SimpleNamespace(taps=np.array([1.0, 2.0, 3.0, 4.0, 5.0]), up=2, down=3, delay=1, history=2)
    x = np.array([1.0, 10.0, 100.0], dtype=np.float32)
    z, S = D.resample(x, t, 0, 5)
    assert z.tolist() == [1.0, 24.0, 350.0, 0.0, 0.0] and S.tolist() == z.tolist()
    z, S = D.resample(-x, t, 1, 2)
    assert z.tolist() == [-24.0, -350.0] and S.tolist() == [24.0, 350.0]
    assert R.causal(x, t, 0, 5).tolist() == [1.0, 24.0, 350.0, 0.0, 0.0]
    assert D.resample_bound(z, S, t)[0] == D.LD(2.0 ** -24) * 24 + D.LD(D.MIDDLE * 6 * 2.0 ** -52) * 24 + D.LD(2.0 ** -149)
    y, S = D.reverb(x, np.array([1.0, -2.0], dtype=np.float32), 5)
    assert y.tolist() == [1.0, 8.0, 80.0, -200.0, 0.0] and S.tolist() == [1.0, 12.0, 120.0, 200.0, 0.0]
    assert D.reverb_bound(y, S, 2)[3] == D.LD(2.0 ** -24) * 200 + D.LD(D.MIDDLE * 2 * 2.0 ** -52) * 200 + D.LD(2.0 ** -149)


def test_outputs_with_a_non_finite_reference_are_compared_by_class():
    ref = np.array([1.0, np.nan, np.inf, -np.inf], dtype=D.LD)
    bound = np.full(4, 0.5, dtype=D.LD)
    good = np.array([1.25, np.nan, np.inf, -np.inf], dtype=np.float32)
    assert D.worst(good, ref, bound) == 0.5 and D.check(good, ref, bound, "classes") == 0.5
    for at, v in ((0, np.nan), (0, np.inf), (1, 7.0), (2, -np.inf), (2, np.nan), (3, 3.0e38)):
        bad = good.copy()
        bad[at] = v
        assert D.worst(bad, ref, bound) == float("inf")
        with pytest.raises(AssertionError):
            D.check(bad, ref, bound, "classes")
    assert D.worst(good[1:], ref[1:], bound[1:]) == 0.0


# ---- reverberation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", range(len(D.REVERB_LENGTHS)), ids=[f"len{n}" for n in D.REVERB_LENGTHS])
def test_reverb_restatement_meets_the_bound_and_mutations_leave_it(r):
    bank, lengths = D.reverb_edge_bank()
    n = int(lengths[r])
    x, h = D.reverb_edge_audio()[r], bank[r, :n]
    assert np.isfinite(h).all() and bank[r, n] == np.float32(1e30)
    # with the whole tail behind the clip: the last taps of the longest row meet no sample before it
    n_out = D.REVERB_N_OUT
    ref, S = D.reverb(x, h, n_out)
    bound = D.reverb_bound(ref, S, n)
    assert np.isfinite(ref).all() and (bound > 0).all()
    assert ref[D.REVERB_N + n - 2] != 0 and not ref[D.REVERB_N + n - 1:].any()
    D.check(RR.reverb(x[None], bank, lengths, [r], n_out)[0], ref, bound, f"reverb len {n} batch")
    cut, _ = RR.stream_cut(x, bank, list(D.REVERB_CUTS), lengths, r)
    D.check(cut, ref[:D.REVERB_N], bound[:D.REVERB_N], f"reverb len {n} cut at {D.REVERB_CUTS}")
    short = D.worst(RR.convolve(x, h[:n - 1], n_out), ref, bound)
    late = D.worst(RR.convolve(np.concatenate([np.zeros(1, dtype=np.float32), x[:-1]]), h, n_out), ref, bound)
    print(f"reverb len {n}: h[:len - 1] {short:.3g} bounds off, x one sample late {late:.3g}")
    assert short > 1.0 and late > 1.0, "the bound lets a mutation pass"
