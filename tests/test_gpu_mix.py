"""Noise mixer on the GPU (SPEC.md 1.10; `lsm_mix_power_f32`, `lsm_mix_f32`, `lsm_mix_stream_f32`, `frontend.NoiseMixer`,
`frontend.MixStream`, `HotPath(mixer=...)`, `features_from_audio(corrupt=...)`, `AudioStreamBank(mixer=...)`): byte for byte
against the NumPy restatement (tests/mix_restatement.py), cut against uncut byte for byte, the refusals, graph capture."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_restatement as M  # noqa: E402
from test_mix_host import wide_spread  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = np.float32(-1234.5)
_BANKS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _noise(rows, n, seed, level=0.1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, n)) * level).astype(np.float32)


def _bank(L):
    """(noise bank (3, L), its NoiseMixer), shared by the tests of one length."""
    from lsm_speech_classifier_amd import frontend
    if L not in _BANKS:
        noise = _noise(3, L, 1000 + L, 0.05)
        _BANKS[L] = (noise, frontend.NoiseMixer(noise))
    return _BANKS[L]


def _void(p):
    return C.c_void_p(p) if p else None


# ---- power ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 16000])
def test_power_equals_the_restatement_bit_for_bit(torch_cuda, n):
    _, mixer = _bank(100)
    x = _noise(4, n, n)
    x[0] = wide_spread(n)                                           # the row whose order of summation shows
    x[3] = 0.0
    got = mixer.power(x)
    assert got.dtype == torch_cuda.float64 and tuple(got.shape) == (4,) and got.is_cuda
    want = M.power(x)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert want[3] == 0.0 and (want[:3] > 0).all()
    if n == 16000:
        assert want[0].tobytes() != np.sum(x[0].astype(np.float64) ** 2).tobytes(), "the comparison could not fail"


# ---- batch ---------------------------------------------------------------------------------------------------------------
def _batch_case(n, L, variant):
    """Six clips with different parameters each; variant 1 holds the values outside their ranges."""
    if variant == 0:
        return dict(snr=[np.inf, 30.0, 0.0, -20.0, 0.0, 30.0], shift=[-n, -1, 0, 1, n - 1, n],
                    scale=[1.0, 2.0 ** -7, 0.3, 1.0, 0.3, 2.0 ** -7], rows=[0, 1, 2, 1, 0, 2], offsets=[0, 1, L - 1, 5, L // 2, 3])
    return dict(snr=[0.0, -20.0, 30.0, np.inf, 0.0, 0.0], shift=[2 ** 31 - 1, -2 ** 31, 3, -3, 0, -n - 1000],
                scale=[0.3, 1.0, 1.0, 0.3, 2.0 ** -7, 1.0], rows=[3, -1, 10 ** 6, -2 ** 31, 2, 1],
                offsets=[-1, L + 3, -7 * L - 2, 2 ** 31 - 1, -2 ** 31, 0])


@pytest.mark.parametrize("variant", [0, 1], ids=["in-range", "clamped"])
@pytest.mark.parametrize("L", [1, 100, 4097])
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 16000])
def test_batch_equals_the_restatement_byte_for_byte(torch_cuda, n, L, variant):
    torch = torch_cuda
    noise, mixer = _bank(L)
    B, p = 6, _batch_case(n, L, variant)
    audio = _noise(B, n, 7 * n + L)
    snr = np.asarray(p["snr"])
    ratio = 10.0 ** (-snr / 10.0)                                   # 0, 1e-3, 1 and 1e2
    want_y, want_g, want_p = M.mix(audio, noise, ratio, p["rows"], p["offsets"], p["shift"], p["scale"])
    # canaries before and behind out; out starts 12 bytes into the buffer, so rows begin at every alignment
    buf = torch.full((3 + B * n + 64,), float(CANARY), dtype=torch.float32, device="cuda")
    out = buf[3:3 + B * n].view(B, n)
    got, gain, powers = mixer.mix(audio, snr, p["rows"], p["offsets"], p["shift"], np.asarray(p["scale"], dtype=np.float32),
                                  out=out, want_gain=True)
    assert got is out
    host = buf.cpu().numpy()
    assert powers.cpu().numpy().tobytes() == want_p.tobytes()
    assert gain.cpu().numpy().tobytes() == want_g.tobytes()
    assert host[3:3 + B * n].tobytes() == want_y.tobytes()
    assert (host[:3] == CANARY).all() and (host[3 + B * n:] == CANARY).all(), "the launch wrote outside out"
    noisy = (ratio > 0) & (want_p[:, 0] > 0)
    assert (want_g[noisy] > 0).all() and not want_g[~noisy].any()


def test_null_optional_arrays_equal_explicit_defaults(torch_cuda):
    noise, mixer = _bank(100)
    audio = _noise(4, 1000, 5)
    a = mixer.mix(audio, [0.0, 10.0, 20.0, np.inf], want_gain=True)
    b = mixer.mix(audio, [0.0, 10.0, 20.0, np.inf], rows=0, offsets=0, shift=0, scale=1.0, want_gain=True)
    want = M.mix(audio, noise, 10.0 ** (-np.array([0.0, 10.0, 20.0, np.inf]) / 10.0))
    for x, y, w in zip(a, b, want):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == w.tobytes()
    assert mixer.mix(audio[:0], 10.0).shape == (0, 1000)            # no clips: nothing launched, nothing wrong


def test_a_nan_stays_in_its_clip_and_a_nan_bank_out_of_clean_clips(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    noise, mixer = _bank(100)
    audio = _noise(4, 1000, 9)
    audio[1, 700] = np.nan
    audio[2, 300] = np.inf
    y, g, p = (t.cpu().numpy() for t in mixer.mix(audio, 10.0, rows=[0, 1, 2, 0], shift=[0, 5, -5, 0], want_gain=True))
    want = M.mix(audio, noise, 0.1, rows=[0, 1, 2, 0], shift=[0, 5, -5, 0])
    assert y.tobytes() == want[0].tobytes() and g.tobytes() == want[1].tobytes() and p.tobytes() == want[2].tobytes()
    # an Inf sample makes the gain Inf: no finite sample is left in that clip either
    assert np.isnan(y[1]).all() and not np.isfinite(y[2]).any() and np.isfinite(y[0]).all() and np.isfinite(y[3]).all()
    bad = noise.copy()
    bad[1, 17] = np.nan
    y, g, _ = (t.cpu().numpy() for t in frontend.NoiseMixer(bad).mix(audio[[0, 3]], [np.inf, 10.0], rows=[1, 0],
                                                                     want_gain=True))
    assert y[0].tobytes() == audio[0].tobytes() and g[0] == 0.0     # ratio 0 on the NaN row: the clip, bit for bit
    assert y[1].tobytes() == want[0][3].tobytes()


# ---- streams -------------------------------------------------------------------------------------------------------------
S_STREAMS, S_H, S_L = 5, 64, 41                                     # L smaller than one push
S_GAIN = np.array([0.0, 0.37, 1.5, 0.01, 2.0])
S_SCALE = np.array([1.0, 0.3, 2.0 ** -7, 1.0, 0.3], dtype=np.float32)
S_ROWS = np.array([0, 1, 2, 1, 0], dtype=np.int32)
S_POS = np.array([S_L - 1, 0, 7, 40, 13], dtype=np.int32)


def _stream_setup(torch, T):
    from lsm_speech_classifier_amd import frontend
    noise, mixer = _bank(S_L)
    x = _noise(S_STREAMS, T, 77 + T)
    ms = frontend.MixStream(mixer, S_STREAMS)
    ms.gain.copy_(torch.from_numpy(S_GAIN))
    ms.scale.copy_(torch.from_numpy(S_SCALE))
    ms.rows.copy_(torch.from_numpy(S_ROWS))
    ms.pos.copy_(torch.from_numpy(S_POS))
    want = [M.stream(x[b], noise, S_GAIN[b], S_ROWS[b], S_SCALE[b], S_POS[b]) for b in range(S_STREAMS)]
    return x, ms, np.stack([w[0] for w in want]), np.array([w[1] for w in want])


@pytest.mark.parametrize("cuts", [[64], [1] * 64], ids=["whole", "ones"])
def test_streams_cut_equal_the_uncut_run(torch_cuda, cuts):
    torch = torch_cuda
    x, ms, want, want_pos = _stream_setup(torch, 64)
    got, at = np.full((S_STREAMS, 64), CANARY), 0
    for c in cuts:
        row = np.full((S_STREAMS, S_H), CANARY)
        row[:, :c] = x[:, at:at + c]
        out, counts = ms.push(row, np.full(S_STREAMS, c))
        out = out.cpu().numpy()
        assert counts.tolist() == [c] * S_STREAMS and (out[:, c:] == CANARY).all()
        got[:, at:at + c] = out[:, :c]
        at += c
    assert got.tobytes() == want.tobytes() and ms.pos.cpu().numpy().tolist() == want_pos.tolist()


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_streams_with_idle_and_over_large_counts_through_the_abi(torch_cuda, in_place):
    """Per-stream cut lists holding 0 and a count beyond the row (clamped to its 64 samples), state and samples in place
    and out of place.  A count of 0 leaves the row and the position alone."""
    torch = torch_cuda
    base, eff = [0, 3, 1000, 37, 0, 26], [0, 3, 64, 37, 0, 26]
    T = sum(eff)
    x, ms, want, want_pos = _stream_setup(torch, T)
    mixer, lib = ms.mixer, ms.mixer.lib
    stream = torch.cuda.current_stream().cuda_stream
    pos = ms.pos.clone()
    got, at = np.full((S_STREAMS, T), CANARY), np.zeros(S_STREAMS, dtype=np.int64)
    for k in range(len(base)):
        given = [base[(k + b) % len(base)] for b in range(S_STREAMS)]
        c = [eff[(k + b) % len(base)] for b in range(S_STREAMS)]
        row = np.full((S_STREAMS, S_H), CANARY)
        for b in range(S_STREAMS):
            row[b, :c[b]] = x[b, at[b]:at[b] + c[b]]
        audio = torch.from_numpy(row).cuda()
        out = audio if in_place else torch.full((S_STREAMS, S_H), 99.0, dtype=torch.float32, device="cuda")
        pos_out = pos if in_place else torch.full((S_STREAMS,), -5, dtype=torch.int32, device="cuda")
        cnt = torch.tensor(given, dtype=torch.int32, device="cuda")
        before = pos.cpu().numpy().copy()
        rc = lib.lsm_mix_stream_f32(_void(audio.data_ptr()), S_STREAMS, S_H, _void(mixer.noise.data_ptr()), mixer.n_rows,
                                    mixer.noise_len, _void(cnt.data_ptr()), _void(ms.gain.data_ptr()),
                                    _void(ms.scale.data_ptr()), _void(ms.rows.data_ptr()), _void(pos.data_ptr()),
                                    _void(pos_out.data_ptr()), _void(out.data_ptr()), stream)
        assert rc == 0
        res, pos = out.cpu().numpy(), pos_out
        for b in range(S_STREAMS):
            got[b, at[b]:at[b] + c[b]] = res[b, :c[b]]
            assert (res[b, c[b]:] == (CANARY if in_place else 99.0)).all()
            if c[b] == 0:
                assert int(pos[b]) == before[b]
        if not in_place:
            assert audio.cpu().numpy().tobytes() == row.tobytes()
        at += np.asarray(c)
    assert got.tobytes() == want.tobytes() and pos.cpu().numpy().tolist() == want_pos.tolist()


def test_mix_stream_set_reset_and_defaults(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    noise, mixer = _bank(100)
    assert mixer.row_power.tobytes() == M.power(noise).tobytes()
    ms = frontend.MixStream(mixer, 3)
    x = _noise(3, 50, 21)
    out, _ = ms.push(x)                                             # before `set`: unchanged, the position still moves
    assert out.cpu().numpy().tobytes() == x.tobytes() and ms.pos.tolist() == [50, 50, 50]
    gains = ms.set([2, 0], [10.0, np.inf], speech_power=0.01, rows=[1, 2], scale=[0.5, 1.0])
    want = np.sqrt(0.25 * 0.01 * 0.1 / (M.power(noise[1]) / 100))
    assert gains.tolist() == [want, 0.0] and ms.gain.tolist() == [0.0, 0.0, want]
    assert ms.rows.tolist() == [2, 0, 1] and ms.scale.tolist() == [1.0, 1.0, 0.5]
    out, _ = ms.push(x, [50, 0, 50])
    w2, p2 = M.stream(x[2], noise, want, 1, 0.5, 50)
    got = out.cpu().numpy()
    assert got[2].tobytes() == w2.tobytes() and got[1].tobytes() == x[1].tobytes() and got[0].tobytes() == x[0].tobytes()
    assert ms.pos.tolist() == [0, 50, p2]
    ms.reset([2])
    assert ms.pos.tolist() == [0, 50, 0]
    for bad in (dict(rows=3), dict(speech_power=-1.0), dict(snr_db=np.nan)):
        with pytest.raises(ValueError):
            ms.set([0], **{**dict(snr_db=10.0, speech_power=0.01), **bad})


# ---- the ABI's refusals ----------------------------------------------------------------------------------------------------
def test_abi_refusals(torch_cuda):
    torch = torch_cuda
    noise, mixer = _bank(100)
    lib = mixer.lib
    B, n = 3, 40
    audio = torch.zeros((B, n + 4), dtype=torch.float32, device="cuda")
    out = torch.full((B, n + 4), -7.0, dtype=torch.float32, device="cuda")
    ratio = torch.ones(B + 1, dtype=torch.float64, device="cuda")
    ints = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    scale = torch.ones(B + 1, dtype=torch.float32, device="cuda")
    dbl = torch.full((2 * B + 2,), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    bank = mixer.noise.data_ptr()

    def batch(a=audio.data_ptr(), B=B, n=n, nz=bank, M_=3, L=100, row=ints.data_ptr(), off=ints.data_ptr(),
              sh=ints.data_ptr(), sc=scale.data_ptr(), q=ratio.data_ptr(), o=out.data_ptr(), g=dbl.data_ptr(), p=dbl.data_ptr()):
        return lib.lsm_mix_f32(_void(a), B, n, _void(nz), M_, L, _void(row), _void(off), _void(sh), _void(sc), _void(q),
                               _void(o), _void(g), _void(p), stream)

    def streamed(a=audio.data_ptr(), B=B, n=n, nz=bank, M_=3, L=100, cnt=ints.data_ptr(), g=ratio.data_ptr(),
                 sc=scale.data_ptr(), row=ints.data_ptr(), pi=ints.data_ptr(), po=ints.data_ptr(), o=out.data_ptr()):
        return lib.lsm_mix_stream_f32(_void(a), B, n, _void(nz), M_, L, _void(cnt), _void(g), _void(sc), _void(row),
                                      _void(pi), _void(po), _void(o), stream)

    def power(x=audio.data_ptr(), R=B, n=n, p=dbl.data_ptr()):
        return lib.lsm_mix_power_f32(_void(x), R, n, _void(p), stream)

    cases = []
    for f in (batch, streamed):
        cases += [
            (lambda f=f: f(n=0), "=0 outside \\[1, 16777216\\]"), (lambda f=f: f(n=(1 << 24) + 1), "outside \\[1, 16777216\\]"),
            (lambda f=f: f(L=0), "noise_len=0"), (lambda f=f: f(M_=0), "n_noise_rows=0"), (lambda f=f: f(B=-1), "negative"),
            (lambda f=f: f(a=0), "null buffer"), (lambda f=f: f(nz=0), "null buffer"), (lambda f=f: f(o=0), "null buffer"),
            (lambda f=f: f(a=audio.data_ptr() + 2), "audio is misaligned"), (lambda f=f: f(nz=bank + 1), "noise is misaligned"),
            (lambda f=f: f(o=out.data_ptr() + 2), "out is misaligned"), (lambda f=f: f(sc=scale.data_ptr() + 2), "scale is misaligned"),
            (lambda f=f: f(row=ints.data_ptr() + 2), "noise_row is misaligned"),
        ]
    cases += [
        (lambda: batch(q=0), "null buffer"), (lambda: batch(q=ratio.data_ptr() + 4), "ratio is misaligned"),
        (lambda: batch(off=ints.data_ptr() + 1), "noise_offset is misaligned"), (lambda: batch(sh=ints.data_ptr() + 2), "shift is misaligned"),
        (lambda: batch(g=dbl.data_ptr() + 4), "gain_out is misaligned"), (lambda: batch(p=dbl.data_ptr() + 4), "power_out is misaligned"),
        (lambda: batch(o=audio.data_ptr()), "out must not be audio"),
        (lambda: streamed(g=0), "null buffer"), (lambda: streamed(g=ratio.data_ptr() + 4), "gain is misaligned"),
        (lambda: streamed(cnt=ints.data_ptr() + 2), "count is misaligned"), (lambda: streamed(pi=ints.data_ptr() + 2), "pos_in is misaligned"),
        (lambda: streamed(po=ints.data_ptr() + 2), "pos_out is misaligned"),
        (lambda: power(n=0), "n_samples=0"), (lambda: power(n=(1 << 24) + 1), "n_samples"), (lambda: power(R=-2), "negative"),
        (lambda: power(x=0), "null buffer"), (lambda: power(p=0), "null buffer"),
        (lambda: power(x=audio.data_ptr() + 1), "x is misaligned"), (lambda: power(p=dbl.data_ptr() + 4), "power_out is misaligned"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        assert re.search(words, lib.lsm_last_error().decode()), f"refusal {i} ({words}): {lib.lsm_last_error().decode()!r}"
    assert batch(B=0) == 0 and streamed(B=0) == 0 and power(R=0) == 0 and batch(B=0, a=0, o=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((dbl == -7.0).all()) and not bool(ints.any()), "a refused call wrote"
    # every optional array absent, and the calls the refusals start from
    assert batch(row=0, off=0, sh=0, sc=0, g=0, p=0) == 0 and streamed(cnt=0, sc=0, row=0, pi=0, po=0) == 0
    assert batch() == 0 and streamed() == 0 and power() == 0
    torch.cuda.synchronize()


# ---- graph capture -----------------------------------------------------------------------------------------------------------
def test_a_captured_mix_launch_replays_to_the_same_bytes(torch_cuda):
    torch = torch_cuda
    noise, mixer = _bank(100)
    B, n = 4, 1000
    a0, a1 = _noise(B, n, 31), _noise(B, n, 32)
    kw = dict(rows=[0, 1, 2, 1], offsets=[3, 50, 99, 0], shift=[0, -7, 7, 100], scale=[1.0, 0.5, 0.3, 1.0])
    eager0 = mixer.mix(a0, [0.0, 10.0, 20.0, np.inf], **kw)         # the kernel's first use lies before the capture
    eager1 = mixer.mix(a1, [0.0, 10.0, 20.0, np.inf], **kw)
    dev = lambda v, t: torch.tensor(v, dtype=t, device="cuda")
    rows, offs, sh = (dev(kw[k], torch.int32) for k in ("rows", "offsets", "shift"))
    sc, q = dev(kw["scale"], torch.float32), dev(list(10.0 ** (-np.array([0.0, 10.0, 20.0, np.inf]) / 10.0)), torch.float64)
    static_in, out = torch.from_numpy(a0).cuda(), torch.zeros((B, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # one linear capture: the launch and nothing else
        rc = mixer.lib.lsm_mix_f32(_void(static_in.data_ptr()), B, n, _void(mixer.noise.data_ptr()), 3, 100,
                                   _void(rows.data_ptr()), _void(offs.data_ptr()), _void(sh.data_ptr()), _void(sc.data_ptr()),
                                   _void(q.data_ptr()), _void(out.data_ptr()), None, None,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    static_in.copy_(torch.from_numpy(a1))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1) and not torch.equal(eager0, eager1)


# ---- end to end ----------------------------------------------------------------------------------------------------------
KEYS = ['spike_counts', 'mean_spike_times', 'mean_isi']


def _small_net(F):
    from lsm_speech_classifier_amd import reservoir as Rv, snn
    res = Rv.build_reservoir(Rv.SimulationParams(num_neurons=64, num_output_neurons=32, small_world_graph_k=8,
                                                 mean_weight=2.0 / 4, refractory_period=2), F)
    return snn.SNN(None, reservoir=res)


def test_features_from_corrupted_audio_equal_those_of_the_restatements_mix(torch_cuda):
    from lsm_speech_classifier_amd import frontend, pipeline, synth
    F, n = 8, 5
    noise, mixer = _bank(4097)
    audio = synth.class_chirps(np.arange(n), seed=3)
    plan = frontend.mix_plan(n, 3, 4097, (0.0, 20.0), max_shift=1600, level_db=(-6.0, 0.0), seed=9)
    assert plan.shift.any() and len(set(plan.rows)) > 1
    mixed, _, _ = M.mix(audio, noise, 10.0 ** (-plan.snr_db / 10.0), plan.rows, plan.offsets, plan.shift, plan.scale)
    fe, net = frontend.SpikeFrontEnd(F, "gammatone"), _small_net(F)
    for streams in (1, pipeline.DEFAULT_STREAMS):                   # the serial path and the two-stage topology
        got = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, corrupt=(mixer, plan))
        want = pipeline.features_from_audio(mixed, fe, net, KEYS, batch=2, streams=streams)
        clean = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams)
        assert got.shape == want.shape == (n, len(KEYS) * 32) and want.any()
        assert got.tobytes() == want.tobytes()
        assert got.tobytes() != clean.tobytes(), "the corruption changed nothing: the comparison shows nothing"
    hp = pipeline.HotPath(fe, net, KEYS, streams=1)
    with pytest.raises(ValueError, match="mixer"):
        hp.submit(audio, mix=plan)


def test_audio_stream_bank_with_a_mixer_in_two_cuts(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline
    F, n, hops = 8, 2, 60
    noise, mixer = _bank(4097)
    x = _noise(n, hops * 160, 55, 0.2)
    fe = frontend.SpikeFrontEnd(F, "gammatone")
    db_range = fe.db_range(torch.from_numpy(_noise(1, 16000, 11, 0.2)).cuda())
    net = _small_net(F)

    def run(cuts):
        ms = frontend.MixStream(mixer, n)
        ms.set([0, 1], [5.0, 15.0], speech_power=0.04, rows=[1, 2], scale=[1.0, 0.5])
        bank = pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, 8, 3, 1, KEYS, mixer=ms)
        rows, at = [[] for _ in range(n)], np.zeros(n, dtype=np.int64)
        for new in cuts:
            new = np.asarray(new, dtype=np.int64)
            chunk = np.full((n, int(new.max()) * 160), 7.0, dtype=np.float32)
            for b in range(n):
                chunk[b, :new[b] * 160] = x[b, at[b] * 160:(at[b] + new[b]) * 160]
            r, cnt = bank.push(chunk, new)
            r = r.cpu().numpy()
            for b in range(n):
                rows[b].append(r[b, :cnt[b]])
            at += new
        assert at.tolist() == [hops] * n
        return [np.concatenate(r) for r in rows], ms, bank

    a, ms, bank = run([(60, 60)])
    b, _, _ = run([(3, 17), (0, 2), (27, 1), (30, 40)])
    for ra, rb in zip(a, b):
        assert len(ra) > 0 and ra.any() and ra.tobytes() == rb.tobytes()
    assert ms.pos.tolist() == [(hops * 160) % 4097] * n
    bank.reset([1])
    assert ms.pos.tolist() == [(hops * 160) % 4097, 0]


def test_create_dataset_with_the_corruption_flags(torch_cuda, tmp_path):
    """File 1 written with `augment` holds the rasters of the restatement's mixed clips; without it, today's rasters."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend, synth
    words, noisy, clean = ["a", "b", "c"], str(tmp_path / "noisy.npz"), str(tmp_path / "clean.npz")
    augment = dict(noise_dir="synthetic", snr_db=(0.0, 10.0), time_shift_ms=100.0, level_db=(-6.0, 0.0), seed=7)
    cd.create_dataset(8, "gammatone", commands=words, synthetic_per_class=2, output_file=noisy, augment=augment)
    cd.create_dataset(8, "gammatone", commands=words, synthetic_per_class=2, output_file=clean)
    bank, plan = cd.corruption(augment, 6)
    assert bank.shape == (cd.SYNTHETIC_NOISE_ROWS, cd.SYNTHETIC_NOISE_SECONDS * 16000) and np.abs(plan.shift).max() <= 1600
    audio = synth.class_chirps(np.repeat(np.arange(3), 2), seed=1234)
    mixed, _, _ = M.mix(audio, bank, 10.0 ** (-plan.snr_db / 10.0), plan.rows, plan.offsets, plan.shift, plan.scale)
    fe = frontend.SpikeFrontEnd(8, "gammatone")
    got, plain = np.load(noisy)["X_spikes"], np.load(clean)["X_spikes"]
    assert got.tobytes() == fe.encode(mixed).cpu().numpy().tobytes()
    assert plain.tobytes() == fe.encode(audio).cpu().numpy().tobytes() and got.tobytes() != plain.tobytes()
