"""Silence trimming on the GPU (SPEC.md 1.15; `lsm_trim_silence_f32`, `frontend.SilenceTrimmer`,
`features_from_utterances(trim=...)`, `create_dataset.py --trim-silence`).  Every launch is compared byte for byte with the
NumPy restatement (tests/trim_restatement.py): the whole output row, `first`, `bins` and the bin energies.  Every buffer a
launch writes lies in the middle of 0xAA bytes that must keep their fill, inputs hold NaN behind a clip's count, and the
counts go through the ABI as they are, INT32_MIN and INT32_MAX included: the kernel clamps them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_restatement as TR  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 160
FILL = 0xAA
GUARD = 64                                      # bytes in front of and behind every output that must keep their fill
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _lib_():
    from lsm_speech_classifier_amd import _lib
    return _lib.load()


def _clips(n_clips, n_samples, seed, floor=0.002):
    """Seeded clips: a quiet floor and, per clip, one or two louder stretches of its own place, length and level."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_clips, n_samples)) * floor
    for b in range(n_clips):
        for _ in range(1 + b % 2):
            lo = int(rng.integers(0, max(1, n_samples - 1)))
            hi = min(n_samples, lo + 1 + int(rng.integers(0, max(1, n_samples // 2))))
            x[b, lo:hi] += rng.standard_normal(hi - lo) * rng.uniform(0.1, 0.5)
    return np.ascontiguousarray(x.astype(np.float32))


class _Guarded:
    """``nbytes`` of device memory in the middle of FILL bytes, at ``skew`` bytes behind a 256-byte boundary."""

    def __init__(self, torch, nbytes, skew=0):
        self.n, self.at = nbytes, 256 + skew
        self.buf = torch.full((self.at + nbytes + GUARD + 256,), FILL, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.at += (-base) % 256                                    # torch allocations are 256-byte aligned; be sure
        self.ptr = base + self.at

    def bytes(self):
        got = self.buf.cpu().numpy()
        assert (got[:self.at] == FILL).all() and (got[self.at + self.n:] == FILL).all(), "written outside the buffer"
        return got[self.at:self.at + self.n]


def _launch(torch, audio, counts, time_bins, ratio, pad, minb, n_out=None, skew=0, first=True, bins=True, energy=True,
            stream=None):
    """`lsm_trim_silence_f32` -> (rc, audio_out (B, n_out), first, bins, energy); an output not asked for is None.  ``skew``
    (a multiple of 4): input and output rows start that many bytes behind a 16-byte boundary."""
    B, n_samples = audio.shape
    n_out = HOP * time_bins if n_out is None else n_out
    src = _Guarded(torch, 4 * B * n_samples, skew)
    src.buf[src.at:src.at + src.n] = torch.from_numpy(audio.reshape(-1).view(np.uint8)).cuda()
    cnt = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int64).astype(np.int32)).cuda()
    out = _Guarded(torch, 4 * B * n_out, skew)
    f, b_, e = (_Guarded(torch, 4 * B) if first else None, _Guarded(torch, 4 * B) if bins else None,
                _Guarded(torch, 8 * B * time_bins) if energy else None)
    rc = _lib_().lsm_trim_silence_f32(
        C.c_void_p(src.ptr), B, n_samples, time_bins, C.c_void_p(cnt.data_ptr()) if cnt is not None else None, C.c_double(ratio),
        pad, minb, C.c_void_p(out.ptr), n_out, C.c_void_p(f.ptr) if f else None, C.c_void_p(b_.ptr) if b_ else None,
        C.c_void_p(e.ptr) if e else None, stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc, out.bytes().view(np.float32).reshape(B, n_out), f.bytes().view(np.int32) if f else None,
            b_.bytes().view(np.int32) if b_ else None, e.bytes().view(np.float64).reshape(B, time_bins) if e else None)


def _check(torch, audio, counts, time_bins, ratio, pad, minb, n_out=None, skew=0):
    """One launch against the restatement, byte for byte; returns the restatement's (out, first, bins, energy)."""
    clean = audio.copy()
    poisoned = audio.copy()
    for b in range(len(audio)):                                     # what lies behind a clip's count influences nothing
        poisoned[b, TR.clip_length(None if counts is None else counts[b], audio.shape[1]):] = np.nan
    with np.errstate(all="ignore"):
        want = TR.trim(clean, counts, time_bins, ratio, pad, minb, n_out)
    rc, out, first, bins, energy = _launch(torch, poisoned, counts, time_bins, ratio, pad, minb, n_out, skew)
    assert rc == 0, _lib_().lsm_last_error()
    assert np.array_equal(first, want[1]) and np.array_equal(bins, want[2]), (first, want[1], bins, want[2])
    assert energy.tobytes() == want[3].tobytes(), "bin energies differ from the pinned-order sum"
    assert out.tobytes() == want[0].tobytes(), "audio_out differs from the slice the restatement names"
    return want


# ---- 1. shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_bins", [3, 4, 100])
@pytest.mark.parametrize("n_clips", [1, 3, 65])
def test_shapes_equal_the_restatement(torch_cuda, n_clips, time_bins):
    """Rows shorter than a bin, of three bins and a sample, one sample short of the bins and seven beyond them; an output row
    longer than the bins; rows that start 4, 8 and 12 bytes behind a 16-byte boundary (odd row lengths, a skewed base)."""
    trimmed = 0
    for at, n_samples in enumerate([1, 321, HOP * time_bins - 1, HOP * time_bins + 7]):
        audio = _clips(n_clips, n_samples, 100 * time_bins + at)
        n_out = HOP * time_bins + (0, 5, 1, 0)[at]
        want = _check(torch_cuda, audio, None, time_bins, 1e-2, at % 2, 3, n_out, skew=(0, 4, 12, 8)[at])
        trimmed += int((want[2] < TR.clip_bins(n_samples, time_bins)).sum())
    assert trimmed > 0 or time_bins == 3                             # the cases are not all "kept whole"


def test_the_top_of_the_range(torch_cuda):
    """2 clips of 4096 bins: 64 tiles of energies per clip, an LDS image above 64 KB."""
    assert _lib_().lsm_trim_lds_bytes(4096) > 65536
    audio = _clips(2, HOP * 4096, 7, floor=0.001)
    audio[0, :HOP * 1000] *= 0.01                                   # long quiet stretches around the speech of clip 0
    audio[0, HOP * 3000:] *= 0.01
    want = _check(torch_cuda, audio, [HOP * 4096, HOP * 4000 + 17], 4096, 1e-3, 2, 3)
    assert 3 <= want[2][0] < 4096


# ---- 2. counts through the ABI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1603, 640])
def test_counts_are_clamped(torch_cuda, n_samples):
    counts = [0, 1, 320, 321, n_samples, n_samples + 1, -1, I32_MIN, I32_MAX, 700]
    audio = _clips(len(counts), n_samples, 31)
    want = _check(torch_cuda, audio, counts, 10, 1e-2, 0, 3, HOP * 10 + 3, skew=4)
    assert list(want[2][:3]) == [0, 1, 2] and want[2][6] == 0 and want[2][7] == 0
    last = TR.clip_bins(n_samples, 10) - 1                          # n_samples, n_samples + 1 and INT32_MAX: the whole row
    assert (want[3][[4, 5, 8], last] > 0).all() and not want[3][[0, 6, 7]].any() and not want[3][3, 3:].any()
    _check(torch_cuda, audio, None, 10, 1e-2, 0, 3)                 # a NULL count array: n_samples everywhere
    _check(torch_cuda, audio, counts, 4, 1e-2, 1, 4)                # fewer bins than the rows hold: NB_b stops at time_bins


# ---- 3. endpoint corners ------------------------------------------------------------------------------------------------------
def _bins_clip(n_bins, loud, level=0.3, floor=0.0, seed=3, n_samples=None):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n_bins * HOP) * floor).astype(np.float32) + np.float32(0.0)
    for j in loud:
        x[HOP * j:HOP * (j + 1)] = (rng.standard_normal(HOP) * level).astype(np.float32)
    return x if n_samples is None else x[:n_samples]


def test_endpoint_corners(torch_cuda):
    T = 12
    rows = [_bins_clip(T, [0]), _bins_clip(T, [T - 1]), _bins_clip(T, [5, 6]), _bins_clip(T, []), _bins_clip(T, [10]),
            _bins_clip(T, [1]), _bins_clip(T, [4], floor=0.001)]
    audio = np.stack(rows)
    audio[3] = 0.0                                                   # an all-zero clip
    for ratio, pad, minb, spans in (
            # min_bins grows to the right, then to the left: bin 10 alone takes bin 11 and bin 9; ratio 0 with a floor: whole
            (0.0, 0, 3, [(0, 3), (9, 3), (5, 3), (0, 12), (9, 3), (1, 3), (0, 12)]),
            (0.0, 2, 3, [(0, 3), (9, 3), (3, 6), (0, 12), (8, 4), (0, 4), (0, 12)]),         # pad clamped at both ends
            (1e-3, 1, 5, [(0, 5), (7, 5), (4, 5), (0, 12), (7, 5), (0, 5), (3, 5)]),
            (1e-3, 0, T, [(0, 12)] * 7),                                                     # min_bins = time_bins
            (1e-3, 40, 3, [(0, 12)] * 7)):
        want = _check(torch_cuda, audio, None, T, ratio, pad, minb)
        got = list(zip(want[1].tolist(), want[2].tolist()))
        assert got == spans, (ratio, pad, minb, got)
    # speech in a last bin that holds one sample (len = 160 k + 1), and a one-bin clip
    audio = np.stack([_bins_clip(T, [4]), _bins_clip(T, [0])])
    audio[0, HOP * 4:] = 0.0
    audio[0, HOP * 7] = 0.25
    want = _check(torch_cuda, audio, [HOP * 7 + 1, 100], T, 0.0, 0, 3)
    assert (want[1][0], want[2][0]) == (5, 3) and (want[1][1], want[2][1]) == (0, 1)
    assert want[0][0, 2 * HOP] == np.float32(0.25) and not want[0][0, 2 * HOP + 1:].any()


def test_an_exact_tie_is_not_active(torch_cuda):
    """One sample of 2.0 gives E = 4; one of 1.0 in another bin gives e = 1 = E * 0.25: strictly greater it is not."""
    audio = np.zeros((2, HOP * 8), dtype=np.float32)
    audio[:, HOP * 2 + 5] = 2.0
    audio[0, HOP * 6 + 9] = 1.0
    audio[1, HOP * 6 + 9] = np.nextafter(np.float32(1.0), np.float32(2.0))
    want = _check(torch_cuda, audio, None, 8, 0.25, 0, 3)
    assert (want[1][0], want[2][0]) == (2, 3) and (want[1][1], want[2][1]) == (2, 5)
    assert want[3][0, 2] == 4.0 and want[3][0, 6] == 1.0


def test_values_that_are_not_finite_keep_their_clip_whole_and_no_other(torch_cuda):
    T = 9
    audio = np.stack([_bins_clip(T, [3, 4], floor=0.001, seed=s) for s in range(7)])
    clean = TR.trim(audio, None, T, 1e-3, 0, 3)
    assert all((f, n) == (3, 3) for f, n in zip(clean[1], clean[2]))
    audio[1, HOP * 7 + 1] = np.nan
    audio[3, HOP * 0 + 159] = np.inf
    audio[5, HOP * 8] = 3e38                                        # a finite energy of 9e76: a very loud bin, nothing else
    want = _check(torch_cuda, audio, None, T, 1e-3, 0, 3)
    assert list(zip(want[1].tolist(), want[2].tolist())) == [(3, 3), (0, 9), (3, 3), (0, 9), (3, 3), (6, 3), (3, 3)]
    assert np.isnan(want[3][1, 7]) and np.isinf(want[3][3, 0]) and np.isfinite(want[3][5]).all()
    for b in (0, 2, 4, 6):
        assert want[0][b].tobytes() == clean[0][b].tobytes()


# ---- 4. the order of the sum ------------------------------------------------------------------------------------------------
def test_the_energies_are_the_pinned_sum_and_not_numpys(torch_cuda):
    rng = np.random.default_rng(77)
    audio = (rng.standard_normal((5, HOP * 40)) * 0.2).astype(np.float32)
    want = _check(torch_cuda, audio, None, 40, 1e-3, 0, 3)
    pairwise = (audio.astype(np.float64).reshape(5, 40, HOP) ** 2).sum(axis=2)
    assert (want[3].view(np.uint64) != pairwise.view(np.uint64)).any(), "the case no longer tells the two orders apart"


# ---- 5. optional outputs, refusals, graph capture -------------------------------------------------------------------------
def test_null_optional_outputs_leave_the_others_as_they_are(torch_cuda):
    audio = _clips(5, 1500, 8)
    full = _launch(torch_cuda, audio, None, 9, 1e-2, 1, 3)
    assert full[0] == 0
    for first, bins, energy in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = _launch(torch_cuda, audio, None, 9, 1e-2, 1, 3, first=first, bins=bins, energy=energy)
        assert got[0] == 0 and got[1].tobytes() == full[1].tobytes()
        for mine, ref, asked in zip(got[2:], full[2:], (first, bins, energy)):
            assert (mine is None) if not asked else mine.tobytes() == ref.tobytes()


def test_refusals_in_their_order_launch_nothing(torch_cuda):
    torch = torch_cuda
    lib = _lib_()
    assert lib.lsm_trim_lds_bytes(2) < 0 and lib.lsm_trim_lds_bytes(4097) < 0
    assert lib.lsm_trim_lds_bytes(3) == 24 + 4 * 64 * 161 and lib.lsm_trim_lds_bytes(4096) == 32768 + 4 * 64 * 161
    B, n_samples, T = 2, 700, 4
    audio = torch.from_numpy(_clips(B, n_samples, 5)).cuda()
    counts = torch.full((B,), n_samples, dtype=torch.int32, device="cuda")
    out = torch.full((B * HOP * T * 4,), FILL, dtype=torch.uint8, device="cuda")
    first, bins = (torch.full((B * 4,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
    energy = torch.full((B * T * 8 + 8,), FILL, dtype=torch.uint8, device="cuda")
    good = dict(audio=audio.data_ptr(), n_clips=B, n_samples=n_samples, time_bins=T, clip_samples=counts.data_ptr(), ratio=1e-3,
                pad_bins=1, min_bins=3, audio_out=out.data_ptr(), n_samples_out=HOP * T, first=first.data_ptr(),
                bins=bins.data_ptr(), energy=energy.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lsm_trim_silence_f32(a["audio"] or None, a["n_clips"], a["n_samples"], a["time_bins"], a["clip_samples"] or None,
                                      C.c_double(a["ratio"]), a["pad_bins"], a["min_bins"], a["audio_out"] or None,
                                      a["n_samples_out"], a["first"] or None, a["bins"] or None, a["energy"] or None,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for t in (out, first, bins, energy):
            assert bool((t == FILL).all()), f"a refused call launched something: {kw}"
        return rc, lib.lsm_last_error().decode()

    # a call that breaks a rule and every later one is refused for the earliest
    later = [dict(n_clips=-1), dict(time_bins=2), dict(ratio=float("nan")), dict(pad_bins=-1), dict(min_bins=2),
             dict(audio=0), dict(audio_out=good["audio"]), dict(n_samples_out=HOP * T - 1), dict(energy=good["energy"] + 4)]
    texts = ["n_clips=-1", "time_bins=2 must be", "ratio=", "pad_bins=-1", "min_bins=2 outside", "are required", "must not be audio",
             "n_samples_out=639", "8-byte aligned"]
    for at, text in enumerate(texts):
        broken = {}
        for kw in reversed(later[at:]):
            broken.update(kw)
        rc, msg = call(**broken)
        assert rc == -1 and text in msg, (at, rc, msg)
    for kw, text, code in ((dict(n_samples=0), "n_samples=0", -1), (dict(time_bins=4097), "4096", -4), (dict(ratio=1.0), "ratio=1", -1),
                           (dict(ratio=-1e-9), "ratio=", -1), (dict(ratio=float("inf")), "ratio=inf", -1),
                           (dict(min_bins=T + 1), "min_bins=5 outside", -1), (dict(audio_out=0), "are required", -1),
                           (dict(audio=good["audio"] + 2), "4-byte aligned", -1), (dict(audio_out=good["audio_out"] + 1), "4-byte", -1),
                           (dict(clip_samples=good["clip_samples"] + 2), "4-byte aligned", -1),
                           (dict(first=good["first"] + 1), "4-byte aligned", -1), (dict(bins=good["bins"] + 2), "4-byte aligned", -1)):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert call(n_clips=0)[0] == 0                                   # nothing to do: nothing launched, nothing written


def test_a_captured_launch_replays_to_the_same_bytes(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    audio = _clips(6, HOP * 20 + 3, 12)
    counts = [3203, 2000, 0, 481, 3203, 1601]
    out_w, first_w, bins_w, energy_w = TR.trim(audio, counts, 21, TR.ratio_of(20.0), 1, 3)
    want = (out_w, bins_w, first_w, energy_w)                        # the order `SilenceTrimmer.trim` returns them in
    trimmer = frontend.SilenceTrimmer(top_db=20.0, pad_bins=1, min_bins=3)
    x = torch.from_numpy(audio).cuda()
    n = torch.tensor(counts, dtype=torch.int32, device="cuda")
    out = torch.full((6, HOP * 21), 7.0, dtype=torch.float32, device="cuda")
    eager = trimmer.trim(x, n, out=out, want_energy=True)           # also the first launch: nothing left to set up in capture
    torch.cuda.synchronize()
    for got, ref in zip(eager, want):
        assert got.cpu().numpy().tobytes() == ref.tobytes()
    assert eager[0] is out and eager[1].dtype == torch.int32 and eager[1].is_cuda
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = trimmer.trim(x, n, out=out, want_energy=True)
    for replay in range(2):
        for t in captured:
            t.fill_(7 if t.dtype != torch.float64 else 7.0)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(captured, want):
            assert got.cpu().numpy().tobytes() == ref.tobytes(), replay


def test_the_python_layer_checks_its_arguments_and_takes_host_lengths(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    trimmer = frontend.SilenceTrimmer(top_db=None, pad_bins=0, min_bins=3)
    assert trimmer.ratio == 0.0 and frontend.SilenceTrimmer().ratio == 1e-3
    audio = np.stack([_bins_clip(8, [2, 3]), _bins_clip(8, [6])])
    out, bins, first = trimmer.trim(audio, [HOP * 8, HOP * 7 - 5])
    want = TR.trim(audio, [HOP * 8, HOP * 7 - 5], 8, 0.0, 0, 3)
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
    assert bins.cpu().tolist() == want[2].tolist() == [3, 3] and first.cpu().tolist() == want[1].tolist() == [2, 4]
    for bad, text in ((dict(lengths=[1, 2, 3]), "lengths must be 2 integers"), (dict(lengths=[0, HOP * 8 + 1]), "outside"),
                      (dict(time_bins=2), "time_bins = 2"), (dict(time_bins=4097), "time_bins = 4097"),
                      (dict(out=torch.empty((2, HOP * 8 - 1), device="cuda")), "out must be")):
        with pytest.raises(ValueError, match=text):
            trimmer.trim(audio, **bad)
    x = torch.from_numpy(audio).cuda()
    with pytest.raises(ValueError, match="out must not be audio"):
        trimmer.trim(x, out=x)
    empty = trimmer.trim(np.zeros((0, HOP * 8), dtype=np.float32))
    assert tuple(empty[0].shape) == (0, HOP * 8) and tuple(empty[1].shape) == (0,)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------
KEYS = ["spike_counts", "spike_variances", "last_spike_times", "mean_isi"]


def _utterances(n_bins_max, seed, n=6):
    """Utterances of their own lengths: tones and noise over a stretch of bins of their own, a floor 60 dB below around it."""
    rng = np.random.default_rng(seed)
    utts = []
    for r in range(n):
        total = int(rng.integers(n_bins_max // 2, n_bins_max + 1)) * HOP - int(rng.integers(0, 2)) * int(rng.integers(1, HOP))
        lo = int(rng.integers(0, total // 3))
        hi = min(total, lo + int(rng.integers(max(4 * HOP, total // 3), max(4 * HOP, total // 3) + total // 6 + 1)))
        t = np.arange(total) / 16000.0
        x = 0.0002 * rng.standard_normal(total)
        f0, f1 = rng.uniform(200, 3000, size=2)
        x[lo:hi] += (0.3 * np.sin(2 * np.pi * (f0 + (f1 - f0) * t / t[-1]) * t) * (0.4 + np.abs(np.sin(2 * np.pi * 9 * t)))
                     + 0.05 * rng.standard_normal(total))[lo:hi]
        utts.append(np.ascontiguousarray(x.astype(np.float32)))
    return utts


def _small_net(c):
    """The small reservoir of the ragged feature tests at half the membrane threshold, so that clips of a dozen bins drive it:
    rows of zeros would compare equal whatever the trimmer did."""
    from lsm_speech_classifier_amd import reservoir as R, snn
    n, k, n_out = 256, 50, 100
    return snn.SNN(None, reservoir=R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                                                        mean_weight=2.0 / (k // 2), refractory_period=2,
                                                                        membrane_threshold=1.0), c))


@pytest.mark.parametrize("fb", ["gammatone", "mel"])
def test_trimmed_features_equal_the_features_of_the_host_slices(torch_cuda, fb):
    """F = 16, 40 bins, the small reservoir of the ragged feature tests: `features_from_utterances(trim=...)` rows are, bit for
    bit, `features_from_utterances` on the slices the restatement cuts on the host; whole bins of exact zeros around an
    utterance change nothing (pad_bins = 0), which the untrimmed route cannot say."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline
    T = 40
    fe = frontend.SpikeFrontEnd(16, fb, redundancy=2, thresholds=[0.40, 0.55, 0.70, 0.85], gap=0.1, time_bins=T, n_samples=HOP * T)
    net = _small_net(fe.n_channels)
    utts = _utterances(32, 5)
    for top_db, pad, minb in ((30.0, 1, 3), (30.0, 0, 3)):
        cut, _, counts = TR.slices(utts, top_db, pad, minb)
        assert all(3 <= c < -(-len(u) // HOP) for c, u in zip(counts, utts)), "every utterance trims"
        want = pipeline.features_from_utterances(cut, fe, net, KEYS).cpu().numpy()
        live = want[want.any(axis=1)]
        assert len(live) >= 3 and len({w.tobytes() for w in live}) == len(live)      # the reference tells the clips apart
        trimmer = frontend.SilenceTrimmer(top_db, pad, minb)
        for kw in (dict(), dict(batch=4), dict(fused=True)):
            got = pipeline.features_from_utterances(utts, fe, net, KEYS, trim=trimmer, **kw).cpu().numpy()
            assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (top_db, pad, kw)
    # padding invariance (the last pass had pad_bins = 0): zeros in front and behind, in whole bins
    padded = []
    for r, u in enumerate(utts):
        front, whole = 1 + r % 3, HOP * -(-len(u) // HOP)
        row = np.zeros(HOP * T, np.float32)                          # `front` bins of zeros, the utterance, zeros to 40 bins
        row[HOP * front:HOP * front + len(u)] = u
        assert HOP * front + whole < HOP * T
        padded.append(row)
    again = pipeline.features_from_utterances(padded, fe, net, KEYS, trim=trimmer).cpu().numpy()
    assert again.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    plain = pipeline.features_from_utterances(utts, fe, net, KEYS).cpu().numpy()
    plain_padded = pipeline.features_from_utterances(padded, fe, net, KEYS).cpu().numpy()
    assert not np.array_equal(plain, plain_padded) and not np.array_equal(plain, want)
    none = pipeline.features_from_utterances(utts, fe, net, KEYS, trim=None).cpu().numpy()
    assert none.tobytes() == plain.tobytes()


def test_trimmed_utterances_take_the_ragged_fused_launch(torch_cuda, oracle_c, monkeypatch):
    """128 filters, 16 bins, the reservoir of the one-launch step's tests: there the ragged form is served, and
    `fused=True` behind the trimmer is that launch, with the rows of the two launches on the host slices."""
    import step_fused_forms_ref as REF
    from lsm_speech_classifier_amd import frontend, pipeline, snn
    fe = frontend.SpikeFrontEnd(128, "gammatone", thresholds=REF.thresholds(4), time_bins=16, n_samples=2560)
    net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, 128, 16, 4, 160, 384))
    assert pipeline.step_fused_supported(fe, net, 6, "ragged")
    utts = _utterances(16, 9)
    cut, _, counts = TR.slices(utts, 30.0, 1, 3)
    assert all(3 <= c < -(-len(u) // HOP) for c, u in zip(counts, utts))
    want = pipeline.features_from_utterances(cut, fe, net, None).cpu().numpy()
    calls = []
    real = pipeline.step_fused_ragged
    monkeypatch.setattr(pipeline, "step_fused_ragged", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = pipeline.features_from_utterances(utts, fe, net, None, batch=4, fused=True,
                                            trim=frontend.SilenceTrimmer(30.0, 1, 3)).cpu().numpy()
    assert len(calls) == 2 and got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    live = want[want.any(axis=1)]
    assert len(live) >= 3 and len({w.tobytes() for w in live}) == len(live)


def test_create_dataset_trims_on_the_way_to_file_1(torch_cuda, tmp_path):
    """`create_dataset.py --variable-length --trim-silence 30 --synthetic-per-class 2`: File 1's n_steps are four steps per bin
    the restatement keeps, its rows the ragged front end's rasters of the host slices."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_dataset.py"), "--variable-length", "--trim-silence", "30",
                        "--synthetic-per-class", "2", "--n-filters", "16"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    clips, labels = cd._synthetic_utterances(list(cd.COMMANDS), 2, 100)
    cut, _, counts = TR.slices(clips, 30.0, 3, 3)
    line = [ln for ln in r.stdout.splitlines() if "Trimmed at 30 dB" in ln]
    assert line and f"{counts.min()} / {counts.mean():.1f} / {counts.max()} time bins" in line[0], r.stdout
    with np.load(str(tmp_path / cd.OUTPUT_FILE)) as data:
        X, n_steps, y = data["X_spikes"], data["n_steps"], data["y_labels"]
    assert n_steps.tolist() == (counts * 4).tolist() and y.tolist() == list(labels)
    fe = frontend.SpikeFrontEnd(16, "gammatone", redundancy=cd.REDUNDANCY_FACTOR, thresholds=cd.SPIKE_THRESHOLDS,
                                gap=cd.HYSTERESIS_GAP, time_bins=100, n_samples=16000)
    audio, bins = frontend.pack_utterances(cut, 100)
    want = fe.encode_ragged(audio, bins)[0].cpu().numpy()
    assert X.shape == want.shape and np.array_equal(X, want) and X.any()
