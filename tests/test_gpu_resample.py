"""Polyphase resampler on the GPU (SPEC.md 1.8; `lsm_resample_f32`, `lsm_resample_stream_f32`, `frontend.Resampler`,
`frontend.ResampleStream`, `pipeline.AudioStreamBank(resampler=...)`, `create_dataset(resample="device")`): bit for bit
against the NumPy restatement (tests/resample_restatement.py) run with the package's own tap table, within the float32
rounding of `scipy.signal.resample_poly` in float64, per output within the derived bound of the definition
(tests/fir_definition.py), and cut against uncut byte for byte -- at every packaged design of test_resample_host.DESIGNS."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_definition as D  # noqa: E402
import resample_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xAA
# rate -> (n_in, n_out): lengths that are no multiples of anything; 44100: all 160 phases over several waves; 11025: the
# table over 64 KB, and more than one tile of 2048 outputs
BATCH = {48000: (1501, 501), 44100: (1340, 487), 8000: (403, 806), 11025: (2700, 3919), 22050: (1340, 973), 32000: (1501, 751),
         96000: (3005, 501)}
# blocks of an uncut stream run: a stream's outputs cross one tile of 2048 by an uneven remainder and no further.  8 kHz is
# the streamed kernel with up > down, 11.025 kHz with a table over 64 KB (the big-LDS opt-in) as well.
STREAM_BLOCKS = {48000: 2200, 44100: 14, 8000: 1100, 11025: 4, 22050: 7, 32000: 2200, 96000: 2200}
# blocks of the run with a NaN in it: two pushes, the second longer than the history
NAN_BLOCKS = {48000: 100, 44100: 6, 8000: 100, 11025: 4, 22050: 6, 32000: 100, 96000: 100}
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _noise(n_rows, n, seed, dtype):
    """Rows of seeded noise under a level ramp; row 2 begins with exact zeros."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, n)) * np.linspace(0.02, 0.6, n)[None, :]
    if n_rows > 2:
        x[2, :n // 7] = 0.0
    if dtype == np.int16:
        return np.clip(np.round(x * 8192), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def _table(rate):
    from lsm_speech_classifier_amd import frontend
    if rate not in _CACHE:
        _CACHE[rate] = frontend.resample_table(rate)
    return _CACHE[rate]


# ---- batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("rate", sorted(BATCH))
def test_batch_equals_the_restatement_and_resample_poly(torch_cuda, rate, dtype):
    torch = torch_cuda
    from scipy.signal import resample_poly
    from lsm_speech_classifier_amd import frontend
    n_in, n_out = BATCH[rate]
    t = _table(rate)
    x = _noise(3, n_in, rate, dtype)
    rs = frontend.Resampler(rate)
    assert (rs.up, rs.down, rs.delay, rs.history) == (t.up, t.down, t.delay, t.history)
    assert rs.taps.tobytes() == t.taps.tobytes() and rs.default_length(n_in) == n_out
    got = rs.resample(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, n_out) and got.is_cuda
    got = got.cpu().numpy()
    want = np.stack([R.batch(row, t) for row in x])
    assert got.tobytes() == want.tobytes(), f"max |diff| = {np.abs(got - want).max():.3e}"
    for b in range(3):
        ref = resample_poly(R.widen(x[b]), t.up, t.down)
        err, bound = np.abs(got[b] - ref).max(), 2.0 ** -23 * np.abs(ref).max()
        print(f"{rate} Hz {np.dtype(dtype).name} clip {b}: max |y - resample_poly| = {err:.3e}, {err / bound:.2f} of the bound")
        assert ref.shape == (n_out,) and err <= bound
        # per output, against the definition: a quiet stretch of a clip is held to its own level
        ref, S = D.resample(x[b], t, t.delay, n_out)
        D.check(got[b], ref, D.resample_bound(ref, S, t), f"resample batch {rate} Hz {np.dtype(dtype).name} clip {b}")
    # a tensor on the device gives the same samples
    assert rs.resample(torch.from_numpy(x).cuda()).cpu().numpy().tobytes() == want.tobytes()
    # a smaller n_out is the prefix, and nothing is written past it: the rows of a caller-owned output lie in a buffer
    # prefilled with 0xAA
    short = n_out - 37
    buf = torch.full(((3 * short + 64) * 4,), FILL, dtype=torch.uint8, device="cuda").view(torch.float32)
    out = buf[:3 * short].view(3, short)
    assert rs.resample(x, n_out=short, out=out) is out
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == np.ascontiguousarray(want[:, :short]).tobytes()
    assert bool((buf[3 * short:].view(torch.uint8) == FILL).all()), "written past n_out"
    # a longer one continues over the zeros behind the clip
    longer = rs.resample(x[:1], n_out=n_out + 2 * t.delay + 3).cpu().numpy()
    assert longer.tobytes() == R.batch(x[0], t, n_out + 2 * t.delay + 3)[None].tobytes()


def test_equal_rates_are_the_identity(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    rs = frontend.Resampler(16000)
    x = _noise(3, 100, 5, np.int16)
    assert rs.resample(x).cpu().numpy().tobytes() == (x.astype(np.float32) / np.float32(32768)).tobytes()
    got = rs.resample(x.astype(np.float32), n_out=120).cpu().numpy()
    assert np.ascontiguousarray(got[:, :100]).tobytes() == x.astype(np.float32).tobytes() and not got[:, 100:].any()
    st = frontend.ResampleStream(16000, 3)
    assert (st.unit_blocks, st.unit_in, st.unit_hops) == (160, 160, 1)
    out, counts = st.push(x, [100, 0, 40])
    out = out.cpu().numpy()
    assert counts.tolist() == [100, 0, 40] and out[0].tobytes() == (x[0].astype(np.float32) / np.float32(32768)).tobytes()
    assert not out[1].any() and not out[2, 40:].any() and out[2, :40].tobytes() == (x[2, :40].astype(np.float32) / np.float32(32768)).tobytes()


# ---- streams ---------------------------------------------------------------------------------------------------------------
def _uncut(rate, dtype):
    """(x (3, G * down), z (3, G * up)): three streams and the restatement's uncut run over them."""
    key = ("uncut", rate, np.dtype(dtype).name)
    if key not in _CACHE:
        t = _table(rate)
        x = _noise(3, STREAM_BLOCKS[rate] * t.down, rate + 7, dtype)
        _CACHE[key] = (x, np.stack([R.stream(row, t) for row in x]))
    return _CACHE[key]


def _history(rs):
    return rs.state.cpu().numpy().view(np.float32)[:, :rs.history]


def _push_cut(rs, x, plan, done=None):
    """Push ``x`` (n, G * down) in the pieces of ``plan`` (rows of per-stream block counts); the space behind a stream's
    blocks holds 7s that must never be read, and the outputs behind a stream's count keep the canary of the caller-owned
    ``out``.  Returns the samples per stream, concatenated."""
    import torch
    n = x.shape[0]
    done = np.zeros(n, dtype=np.int64) if done is None else done
    got = [[] for _ in range(n)]
    for i, new in enumerate(plan):
        new = np.asarray(new, dtype=np.int64)
        G = max(int(new.max()), 1)
        chunk = np.full((n, G * rs.down), 7, dtype=x.dtype)
        for b in range(n):
            chunk[b, :new[b] * rs.down] = x[b, done[b] * rs.down:(done[b] + new[b]) * rs.down]
        # every other push into a caller-owned `out` full of canaries, the rest into the zeros that `push` allocates
        mine = None if i % 2 else torch.full((n, G * rs.up * 4), FILL, dtype=torch.uint8, device="cuda").view(torch.float32)
        out, counts = rs.push(chunk, new, out=mine)
        assert counts.tolist() == (new * rs.up).tolist() and tuple(out.shape) == (n, G * rs.up)
        assert mine is None or out is mine
        out = out.cpu().numpy()
        for b in range(n):
            got[b].append(out[b, :counts[b]])
            behind = out[b, counts[b]:].view(np.uint8)
            assert not behind.any() if mine is None else (behind == FILL).all(), "written behind a stream's samples"
        done += new
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("rate", sorted(STREAM_BLOCKS))
def test_streams_uncut_and_cut(torch_cuda, rate, dtype):
    from lsm_speech_classifier_amd import frontend
    t = _table(rate)
    G = STREAM_BLOCKS[rate]
    x, z = _uncut(rate, dtype)
    rs = frontend.ResampleStream(rate, 3)
    assert (rs.unit_blocks, rs.unit_in, rs.unit_hops) == frontend.resample_units(t.up, t.down)
    assert rs.unit_blocks == 160 // np.gcd(t.up, 160) and rs.unit_in == rs.unit_blocks * t.down
    assert rs.unit_blocks * t.up == rs.unit_hops * 160              # a unit is a whole number of front-end hops
    known = {48000: (160, 480, 1), 44100: (1, 441, 1), 8000: (80, 80, 1), 11025: (1, 441, 4)}
    assert rate not in known or (rs.unit_blocks, rs.unit_in, rs.unit_hops) == known[rate]
    assert 2048 < G * t.up < 2 * 2048                               # one tile and a part of the second
    assert rs.state_bytes % 16 == 0 and rs.state_bytes >= 4 * t.history and not rs.state.any()
    out, counts = rs.push(x)
    assert counts.tolist() == [G * t.up] * 3
    out = out.cpu().numpy()
    assert out.tobytes() == z.tobytes(), "the uncut run differs from the restatement"
    for b in range(3):
        ref, S = D.resample(x[b], t, 0, G * t.up)
        D.check(out[b], ref, D.resample_bound(ref, S, t), f"resample streamed {rate} Hz {np.dtype(dtype).name} stream {b}")
    final = _history(rs).copy()
    want_hist = np.stack([R.widen(row).astype(np.float32)[-t.history:] for row in x])
    assert final.tobytes() == want_hist.tobytes()
    # cut at block boundaries: single blocks (shorter than the history), pushes in which a stream delivers nothing, the
    # state always in place
    a, c = G // 3, G // 5
    plan = [(1, 1, 1), (2, 0, 1), (0, 0, 0), (a, c, 1), (1, a, c), (c, 1, 0)]
    if G < 10:                                                      # 11.025 and 22.05 kHz: 4 and 7 blocks in all
        plan = [(1, 1, 1), (1, 0, 1), (0, 0, 0), (1, 1, 0)]
    plan.append(tuple(G - sum(p[b] for p in plan) for b in range(3)))
    assert min(plan[-1]) > 0
    rs2 = frontend.ResampleStream(rate, 3)
    got = _push_cut(rs2, x, plan)
    for b in range(3):
        assert got[b].tobytes() == z[b].tobytes(), f"stream {b}: cut differs from uncut"
    assert rs2.state.cpu().numpy().tobytes() == rs.state.cpu().numpy().tobytes()
    # a slot is reset mid-run: that stream starts over, the others go on
    rs3 = frontend.ResampleStream(rate, 3)
    h = G // 2
    _push_cut(rs3, x, [(h, h, h)])
    rs3.reset([1])
    assert not rs3.state[1].any() and rs3.state[0].any()
    got = _push_cut(rs3, x, [(G - h,) * 3], done=np.full(3, h, dtype=np.int64))
    restarted = R.stream(x[1, h * t.down:], t)
    assert got[1].tobytes() == restarted.tobytes() and got[1].tobytes() != z[1, h * t.up:].tobytes()
    for b in (0, 2):
        assert got[b].tobytes() == z[b, h * t.up:].tobytes()


@pytest.mark.parametrize("rate", sorted(STREAM_BLOCKS))
def test_a_nan_sample_costs_the_outputs_whose_taps_cover_it(torch_cuda, rate):
    from lsm_speech_classifier_amd import frontend
    t = _table(rate)
    G = NAN_BLOCKS[rate]
    x = _uncut(rate, np.float32)[0][:, :G * t.down].copy()
    cut = G // 2
    at = cut * t.down - 10                                           # in the history of the second push
    assert t.history > 10
    x[1, at] = np.nan
    rs = frontend.ResampleStream(rate, 3)
    got = _push_cut(rs, x, [(cut,) * 3, (G - cut,) * 3])
    m = np.arange(G * t.up, dtype=np.int64)
    i0, k0 = m * t.down // t.up, m * t.down % t.up
    n_taps = (len(t.taps) - k0 + t.up - 1) // t.up
    covered = (i0 - n_taps + 1 <= at) & (at <= i0)
    assert covered.any() and not covered[i0 - t.history > at].any()
    assert np.isnan(got[1]).tolist() == covered.tolist()
    want = R.stream(x[1], t)
    assert np.isnan(want).tolist() == covered.tolist()
    assert got[1][~covered].tobytes() == want[~covered].tobytes()
    for b in (0, 2):
        assert got[b].tobytes() == R.stream(x[b], t).tobytes()
    assert not np.isnan(_history(rs)).any()                         # more than Hs samples have passed


def test_out_of_place_state_through_the_c_abi(torch_cuda):
    """`state_in` NULL is the start of every stream, `state_out` another buffer than `state_in`: the whole block travels,
    the padding and an idle stream's block included; a stream's row is written up to its count and no further."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    rate, G, n = 44100, 3, 3
    t = _table(rate)
    x = _noise(n, 2 * G * t.down, 99, np.int16)
    taps = torch.from_numpy(t.taps).cuda()
    nbytes = lib.lsm_resample_state_bytes(len(t.taps), t.up)
    assert nbytes == 240 and t.history * 4 == 228                   # three words of padding
    stream = torch.cuda.current_stream().cuda_stream
    states = [torch.full((n, nbytes), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(2)]
    plans = [(3, 0, 1), (1, 3, 0)]
    done = np.zeros(n, dtype=np.int64)
    got = [[] for _ in range(n)]
    for call, new in enumerate(plans):
        chunk = np.full((n, G * t.down), 7, dtype=np.int16)
        for b in range(n):
            chunk[b, :new[b] * t.down] = x[b, done[b] * t.down:(done[b] + new[b]) * t.down]
        audio = torch.from_numpy(chunk).cuda()
        blocks = torch.tensor(new, dtype=torch.int32, device="cuda")
        out = torch.full((n, G * t.up * 4), FILL, dtype=torch.uint8, device="cuda")
        _lib.check(lib.lsm_resample_stream_f32(
            C.c_void_p(audio.data_ptr()), 1, n, G, C.c_void_p(taps.data_ptr()), len(t.taps), t.up, t.down,
            C.c_void_p(blocks.data_ptr()), C.c_void_p(states[0].data_ptr()) if call else None,
            C.c_void_p(states[call].data_ptr()), C.c_void_p(out.data_ptr()), stream), "lsm_resample_stream_f32")
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for b in range(n):
            got[b].append(out[b, :new[b] * t.up * 4].view(np.float32))
            assert (out[b, new[b] * t.up * 4:] == FILL).all(), "written behind a stream's samples"
        done += np.asarray(new)
    first, second = (s.cpu().numpy() for s in states)
    for b in range(n):
        cuts = [p[b] for p in plans]
        want, hist = R.stream_cut(x[b], t, cuts)
        assert np.concatenate(got[b]).tobytes() == want.tobytes(), f"stream {b}"
        assert second[b, :228].tobytes() == hist.tobytes() and not second[b, 228:].any()
        assert first[b, :228].tobytes() == R.stream_cut(x[b], t, cuts[:1])[1].tobytes() and not first[b, 228:].any()
    assert second[2].tobytes() == first[2].tobytes() and not first[1].any()     # the idle streams' blocks


def test_refusals_launch_nothing(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    t = _table(48000)
    K, n, L, G = len(t.taps), 2, 90, 4
    taps = torch.from_numpy(np.concatenate([t.taps, t.taps])).cuda()
    audio = torch.zeros((n, L + 4), dtype=torch.float32, device="cuda")
    out = torch.full((n, 64), -7.0, dtype=torch.float32, device="cuda")
    state = torch.full((n, 256 + 16), 0x3C, dtype=torch.uint8, device="cuda")
    blocks = torch.full((n + 1,), G, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    void = lambda p: C.c_void_p(p) if p else None

    def batch(a=audio.data_ptr(), fmt=0, n=n, n_in=L, tp=taps.data_ptr(), K=K, up=1, down=3, D=t.delay, n_out=30,
              o=out.data_ptr()):
        return lib.lsm_resample_f32(void(a), fmt, n, n_in, void(tp), K, up, down, D, n_out, void(o), stream)

    def streamed(a=audio.data_ptr(), fmt=0, n=n, G=G, tp=taps.data_ptr(), K=K, up=1, down=3, bl=blocks.data_ptr(),
                 s_in=state.data_ptr(), s_out=state.data_ptr(), o=out.data_ptr()):
        return lib.lsm_resample_stream_f32(void(a), fmt, n, G, void(tp), K, up, down, void(bl), void(s_in), void(s_out),
                                           void(o), stream)

    cases = []
    for f, name in ((batch, "batch"), (streamed, "streamed")):
        cases += [
            (lambda f=f: f(up=3, down=3), "up == down"), (lambda f=f: f(up=2, down=6), "share the factor 2"),
            (lambda f=f: f(up=0), "must be >= 1"), (lambda f=f: f(down=-3), "must be >= 1"),
            (lambda f=f: f(K=0), "n_taps=0"), (lambda f=f: f(fmt=2), "sample_format=2"),
            (lambda f=f: f(a=0), "null buffer"), (lambda f=f: f(tp=0), "null buffer"), (lambda f=f: f(o=0), "out is required"),
            (lambda f=f: f(a=audio.data_ptr() + 2), "audio is misaligned"),
            (lambda f=f: f(a=audio.data_ptr() + 1, fmt=1), "audio is misaligned"),
            (lambda f=f: f(tp=taps.data_ptr() + 4), "taps_dev is misaligned"),
            (lambda f=f: f(o=out.data_ptr() + 2), "out is misaligned"),
            (lambda f=f: f(n=0), "outside \\[1, 65535\\]"), (lambda f=f: f(n=65536), "outside \\[1, 65535\\]"),
        ]
    cases += [
        (lambda: batch(n_in=0), "n_in=0"), (lambda: batch(n_out=0), "n_out=0"), (lambda: batch(n_out=-5), "n_out=-5"),
        (lambda: batch(D=-1), "delay=-1 does not fit"), (lambda: batch(D=22), "delay=22 does not fit"),
        (lambda: streamed(G=0), "n_blocks=0"), (lambda: streamed(G=1 << 30), "2\\^31 - 1"),
        (lambda: streamed(bl=blocks.data_ptr() + 2), "stream_blocks is misaligned"),
        (lambda: streamed(s_in=state.data_ptr() + 8), "state_in is misaligned"),
        (lambda: streamed(s_out=state.data_ptr() + 8), "state_out is misaligned"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        with pytest.raises(_lib.LsmHipError, match=words):
            _lib.check(rc, "refused")
    # a table that does not fit the LDS laid out by phase: 30000 phases are 240 KB
    for call in (lambda: batch(K=2 * K, up=30000, down=30001, D=0), lambda: streamed(K=2 * K, up=30000, down=30001)):
        rc = call()
        assert rc == -4
        with pytest.raises(_lib.LsmHipError, match="LDS"):
            _lib.check(rc, "refused")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((state == 0x3C).all()), "a refused call wrote to its outputs"
    assert batch() == 0 and streamed() == 0                         # the arguments the refusals start from are good
    torch.cuda.synchronize()


# ---- AudioStreamBank with a resampler in front ---------------------------------------------------------------------------
def test_audio_stream_bank_with_a_resampler(torch_cuda):
    """Device-rate PCM in uneven unit pushes through `AudioStreamBank(resampler=...)` against a second bank without one,
    fed the 16 kHz samples a separate `ResampleStream` made of the same audio in one push."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as Rv, snn
    rate, F, S, K, H, U, n = 48000, 64, 8, 3, 1, 40, 2
    keys = ['spike_counts', 'mean_spike_times', 'mean_isi']
    x = _noise(n, U * 480, 4848, np.int16)
    calib = torch.from_numpy(_noise(1, 16000, 11, np.float32) * np.float32(0.25)).cuda()       # the level of the PCM below
    db_range = frontend.SpikeFrontEnd(F, "gammatone").db_range(calib)
    res = Rv.build_reservoir(Rv.SimulationParams(num_neurons=200, num_output_neurons=40, small_world_graph_k=40,
                                                 mean_weight=2.0 / 20, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    # the reference route: resample alone, then the bank as it was
    samples, counts = frontend.ResampleStream(rate, n).push(x)
    assert counts.tolist() == [U * 160] * n
    plain = pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, S, K, H, keys)
    rs = frontend.ResampleStream(rate, n)
    assert (rs.unit_in, rs.unit_hops) == (480, 1)
    bank = pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, S, K, H, keys, resampler=rs)
    plan = [(3, 5), (0, 2), (7, 1), (10, 12), (20, 20)]
    done = np.zeros(n, dtype=np.int64)
    total, seen_rows = 0, False
    for new in plan:
        new = np.asarray(new, dtype=np.int64)
        Uu = int(new.max())
        chunk = np.full((n, Uu * 480), 7, dtype=np.int16)
        fed = torch.full((n, Uu * 160), 7.0, dtype=torch.float32, device="cuda")
        for b in range(n):
            chunk[b, :new[b] * 480] = x[b, done[b] * 480:(done[b] + new[b]) * 480]
            fed[b, :new[b] * 160] = samples[b, done[b] * 160:(done[b] + new[b]) * 160]
        rows, cnt = bank.push(chunk, new)
        want_rows, want_cnt = plain.push(fed, new)
        assert cnt.tolist() == want_cnt.tolist()
        assert rows.cpu().numpy().tobytes() == want_rows.cpu().numpy().tobytes()
        assert bank.pending_steps.tolist() == plain.pending_steps.tolist()
        total += int(cnt.sum())
        seen_rows = seen_rows or bool(rows.any())
        done += new
    assert done.tolist() == [U] * n and total == 2 * (19 - K + 1)
    assert seen_rows, "the rows are all zeros: the comparison shows nothing"
    bank.reset([0])
    assert not rs.state[0].any() and rs.state[1].any() and not bank.gt.state[0].any()


# ---- create_dataset --resample device -------------------------------------------------------------------------------------
def test_create_dataset_with_the_device_resampler(torch_cuda, tmp_path, monkeypatch, oracle_c, capsys):
    import create_dataset as cd
    from scipy.io import wavfile
    from oracle import ref_numpy as O
    from lsm_speech_classifier_amd import frontend
    root = tmp_path / "corpus"
    decoded = {}

    def put(word, name, rate, pcm):
        (root / word).mkdir(parents=True, exist_ok=True)
        wavfile.write(str(root / word / name), rate, pcm)
        x = pcm.astype(np.float32) / 32768.0
        if x.ndim == 2:
            x = x.mean(axis=1)
        if rate != 16000:
            x = R.batch(np.ascontiguousarray(x, dtype=np.float32), frontend.resample_table(rate))
        x = x[:16000]
        decoded[(word, name)] = np.ascontiguousarray(np.pad(x, (0, 16000 - len(x))), dtype=np.float32)

    def pcm(rate, seconds, seed, channels=1):
        rng = np.random.default_rng(seed)
        n = int(rate * seconds)
        t = np.arange(n) / rate
        x = [0.4 * np.sin(2 * np.pi * (300 + 200 * c + 300 * t) * t) + 0.02 * rng.standard_normal(n) for c in range(channels)]
        x = np.clip(np.round(np.stack(x, axis=1) * 32767), -32768, 32767).astype(np.int16)
        return x if channels > 1 else x[:, 0]

    put("yes", "a_48k.wav", 48000, pcm(48000, 1.0, 1))
    put("yes", "b_44k_long.wav", 44100, pcm(44100, 1.3, 2))
    put("no", "a_8k_stereo_short.wav", 8000, pcm(8000, 0.6, 3, channels=2))
    put("no", "b_16k.wav", 16000, pcm(16000, 1.0, 4))
    (root / "no" / "c_broken.wav").write_bytes(b"RIFF\x00\x00this is not a wav file")
    monkeypatch.chdir(tmp_path)
    words = ["yes", "no"]
    cd.create_dataset(64, "gammatone", commands=words, dataset_root=root, resample="device")
    assert "c_broken.wav" in capsys.readouterr().out
    with np.load(cd.OUTPUT_FILE) as d:
        X, y = d["X_spikes"], d["y_labels"]
    expect = [("yes", "a_48k.wav", 0), ("yes", "b_44k_long.wav", 0), ("no", "a_8k_stereo_short.wav", 1), ("no", "b_16k.wav", 1)]
    assert X.shape == (4, 64, 400) and X.dtype == np.uint8 and y.tolist() == [lab for _, _, lab in expect]
    coefs = O.gammatone_coefs(16000, 64, 50)
    for row, (word, name, _) in enumerate(expect):
        a = decoded[(word, name)]
        ref = oracle_c.encode_hysteresis(oracle_c.normalise_resize(oracle_c.gammatone_db(
            oracle_c.gammatone_spec(a, coefs, 400, 160, 98))), [0.70, 0.80, 0.90, 0.95], 0.1)
        np.testing.assert_array_equal(X[row], ref, err_msg=name)
        assert X[row].any(), name
    # the short file ends where resample_poly ends it: the filter's tail behind 9600 samples is dropped
    assert not decoded[("no", "a_8k_stereo_short.wav")][9600:].any()
    # labels and order are the host route's
    cd.create_dataset(64, "gammatone", commands=words, dataset_root=root, output_file="host.npz")
    with np.load("host.npz") as d:
        assert d["y_labels"].tolist() == y.tolist() and d["X_spikes"].shape == X.shape
    with pytest.raises(ValueError, match="resample"):
        cd.create_dataset(64, "gammatone", commands=words, dataset_root=root, resample="gpu")
