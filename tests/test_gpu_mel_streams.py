"""Streamed mel front end (SPEC.md 1.7, include/lsm_hip_mel_stream.h: `lsm_mel_stream_f32`, `frontend.MelStream`,
`frontend.mel_stream_frame_plan`, `SpikeFrontEnd.mel_db_range`, `pipeline.AudioStreamBank`).

The references: `oracle.ref_numpy.mel_power` for the power values (SPEC.md 1.5's tolerance: an FFT of its own), the batch
kernel `lsm_mel_power_f32` for the same values bit for bit (it is the same transform), NumPy's float32 `log10` for the dB
values (1e-4 dB), and -- from the DEVICE's dB array, so that no libm stands between the two sides -- NumPy's float32
normalisation and the oracle's `encode_hysteresis` for the raster (bit for bit).  A cut run is compared with the uncut one
byte for byte, state block included.  The code under test is never its own reference."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOPS, N_STREAMS, N_FFT = 40, 3, 2048
THR, GAP = [0.70, 0.80, 0.90, 0.95], 0.1
FILL = 0xAA
ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _lg(hop):
    return -(-(N_FFT // 2) // hop)


def _ncols(hop, hops=HOPS):
    """Frames t with t * hop + 1024 <= hops * hop: the ones that never see an end padding."""
    return max(0, hops - _lg(hop) + 1)


def _audio(hop=160):
    """3 streams of 40 hops of seeded noise under a level ramp of 50 dB up and down again (its peak at another place in
    every stream); stream 2 starts with four hops of exact silence."""
    if ("audio", hop) not in _CACHE:
        rng = np.random.RandomState(20260 + hop)
        n = HOPS * hop
        t = np.arange(n) / n
        audio = np.empty((N_STREAMS, n), dtype=np.float32)
        for b, peak in enumerate((0.5, 0.35, 0.65)):
            level_db = -50.0 * np.abs(t - peak) / max(peak, 1 - peak)
            audio[b] = (rng.standard_normal(n) * 0.3 * 10.0 ** (level_db / 20.0)).astype(np.float32)
        audio[2, :4 * hop] = 0.0
        _CACHE[("audio", hop)] = audio
    return _CACHE[("audio", hop)]


def _db32(power):
    """NumPy's float32 10 * log10(maximum(1e-10, S)): np.maximum propagates a NaN."""
    power = np.asarray(power, dtype=np.float32)
    return np.float32(10.0) * np.log10(np.maximum(np.float32(1e-10), power))


def _norm32(db, db_range):
    """SPEC.md 1.7's floor and normalisation in NumPy float32, the bounds rounded to float32 once."""
    lo, hi = np.float32(db_range[0]), np.float32(db_range[1])
    norm = (np.maximum(np.asarray(db, dtype=np.float32), hi - np.float32(80.0)) - lo) / ((hi - lo) + np.float32(1e-8))
    assert norm.dtype == np.float32
    return norm


def _oracle(n_filters, hop=160):
    """(power (n, F, ncols) of the oracle over the frames that see no end padding, the calibration range chosen from its
    absolute dB): the 20th and 80th percentile, so that the normalised values leave [0, 1] on both sides."""
    from oracle import ref_numpy
    key = ("oracle", n_filters, hop)
    if key not in _CACHE:
        ncols = _ncols(hop)
        power = np.stack([ref_numpy.mel_power(a, n_filters, hop=hop)[:, :ncols] for a in _audio(hop)])
        assert power.shape == (N_STREAMS, n_filters, ncols) and power.dtype == np.float32
        lo, hi = (float(v) for v in np.percentile(_db32(power), (20, 80)))
        _CACHE[key] = (power, (lo, hi))
    return _CACHE[key]


def _expected_raster(oracle_c, db_dev, db_range, thr=THR, gap=GAP):
    """NumPy's float32 floor and normalisation of a dB array and the oracle's encoder, per stream: (n, F, ncols * n_thr)."""
    norm = _norm32(db_dev, db_range)
    return np.stack([oracle_c.encode_hysteresis(x, thr, gap) for x in norm])


def _filled(torch, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def _push_plan(torch, ms, audio, plan):
    """Push `audio` (n, samples) through `ms` as `plan` says (a list of per-push hop counts, an int for every stream or one
    per stream), into outputs pre-filled with 0xAA, behind every stream's samples a constant nobody may read.  Checks the
    counts, the fill behind them and that an idle stream's state block stays; returns the concatenated (raster, power, db)
    per stream and the final state bytes."""
    from lsm_speech_classifier_amd import frontend
    n, n_thr, F, R, hop = ms.n_streams, ms.n_thr, ms.n_filters, ms.redundancy, ms.hop
    done = np.zeros(n, dtype=np.int64)
    parts = [([], [], []) for _ in range(n)]
    for step in plan:
        new = np.full(n, step, dtype=np.int64) if np.ndim(step) == 0 else np.asarray(step, dtype=np.int64)
        H = max(int(new.max()), 1)
        chunk = np.full((n, H * hop), 7.0, dtype=np.float32)
        for b in range(n):
            chunk[b, :new[b] * hop] = audio[b, done[b] * hop:(done[b] + new[b]) * hop]
        raster = _filled(torch, (n, F * R, H * n_thr), torch.uint8)
        power, db = _filled(torch, (n, F, H), torch.float32), _filled(torch, (n, F, H), torch.float32)
        before = ms.state.clone()
        want = frontend.mel_stream_frame_plan(ms.seen.copy(), new, hop)
        got_r, cols, got_db, got_p = ms.push(chunk, new, raster_out=raster, db_out=db, power_out=power)
        torch.cuda.synchronize()
        assert got_r is raster and got_db is db and got_p is power
        assert cols.tolist() == want.tolist(), f"frames of push {new.tolist()}"
        r_h, p_h, d_h = raster.cpu().numpy(), power.cpu().numpy(), db.cpu().numpy()
        for b in range(n):
            c = int(cols[b])
            assert (r_h[b, :, c * n_thr:] == FILL).all(), f"raster behind stream {b}'s {c} frames, push {new.tolist()}"
            assert (p_h[b, :, c:].view(np.uint8) == FILL).all() and (d_h[b, :, c:].view(np.uint8) == FILL).all()
            assert set(np.unique(r_h[b, :, :c * n_thr])) <= {0, 1}
            parts[b][0].append(r_h[b, :, :c * n_thr])
            parts[b][1].append(p_h[b, :, :c])
            parts[b][2].append(d_h[b, :, :c])
            if new[b] == 0:
                assert torch.equal(ms.state[b], before[b]), f"state block of idle stream {b}"
        done += new
    out = [tuple(np.concatenate(p, axis=1) for p in parts[b]) for b in range(n)]
    return out, ms.state.cpu().numpy()


def _uncut(torch, n_filters, hop=160, redundancy=1, thr=THR, gap=GAP):
    """One push of all 40 hops (cached): (per-stream (raster, power, db), final state, calibration range)."""
    from lsm_speech_classifier_amd import frontend
    key = ("uncut", n_filters, hop, redundancy, tuple(thr), gap)
    if key not in _CACHE:
        _, db_range = _oracle(n_filters, hop)
        ms = frontend.MelStream(n_filters, N_STREAMS, db_range, thresholds=thr, gap=gap, redundancy=redundancy, hop=hop)
        out, state = _push_plan(torch, ms, _audio(hop), [HOPS])
        _CACHE[key] = (out, state, db_range)
    return _CACHE[key]


def _check_raster(oracle_c, out, db_range, thr=THR, gap=GAP, redundancy=1):
    """The rasters of `out` against the oracle's encoder on NumPy's normalisation of the device's dB values, bit for bit;
    before that: every stream's raster has zeros and ones, and the normalised values leave [0, 1] on both sides."""
    db = np.stack([o[2] for o in out])
    norm = _norm32(db, db_range)
    assert (norm < 0).any() and (norm > 1).any(), "the normalised values stay inside [0, 1]"
    want = _expected_raster(oracle_c, db, db_range, thr, gap)
    for b in range(N_STREAMS):
        assert (out[b][0] == 0).any() and (out[b][0] == 1).any(), f"the raster of stream {b} is constant"
        np.testing.assert_array_equal(out[b][0], np.repeat(want[b], redundancy, axis=0), err_msg=f"raster of stream {b}")
    return want


# the ragged plan: per stream pushes of 0 hops, of 1 hop and of 13 hops or more (longer than the history), 40 hops in all
_RAGGED = np.array([[1, 0, 13, 5, 2, 7, 12], [0, 14, 1, 3, 9, 6, 7], [4, 1, 0, 20, 1, 13, 1]]).T
assert (_RAGGED.sum(axis=0) == HOPS).all()
PLANS = {"1-1-1-37": [1, 1, 1, 37], "3-0-5-32": [3, 0, 5, 32], "20x2": [2] * 20, "ragged": [row for row in _RAGGED]}


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("hop,n_filters", [(160, 13), (160, 40), (160, 80), (256, 40), (1024, 40)])
def test_uncut_push_equals_the_oracle(torch_cuda, oracle_c, hop, n_filters):
    torch = torch_cuda
    from lsm_speech_classifier_amd import mel
    out, _, db_range = _uncut(torch, n_filters, hop)
    p_ref, _ = _oracle(n_filters, hop)
    ncols = _ncols(hop)
    assert ncols == {160: 34, 256: 37, 1024: 40}[hop]
    # the batch kernel on the same audio: frame t of the stream is frame t of the clip (the clip's last frames, which see its
    # end padding, have no counterpart in the stream)
    batch = mel.MelSpectrogram(n_filters, HOPS * hop, HOPS, torch.device("cuda", torch.cuda.current_device()))
    assert batch.hop == hop and batch.n_frames == HOPS + 1
    p_batch = batch.power(torch.from_numpy(_audio(hop)).cuda()).cpu().numpy()
    worst = 0.0
    for b in range(N_STREAMS):
        raster, power, db = out[b]
        assert power.shape == db.shape == (n_filters, ncols) and raster.shape == (n_filters, ncols * 4)
        assert power.dtype == db.dtype == np.float32
        # SPEC.md 1.5: float64 FFT on both sides, float32 power and projection
        np.testing.assert_allclose(power, p_ref[b], rtol=1e-5, atol=2e-6 * p_ref[b].max(), err_msg=f"power of stream {b}")
        assert power.tobytes() == p_batch[b][:, :ncols].tobytes(), f"power of stream {b} against lsm_mel_power_f32"
        err = float(np.abs(db - _db32(power)).max())
        worst = max(worst, err)
        assert err <= 1e-4, f"dB of stream {b}: {err:.3e}"
    print(f"hop={hop} F={n_filters}: max |dB - 10 log10(max(1e-10, S))| = {worst:.3e} dB")
    _check_raster(oracle_c, out, db_range)
    if hop >= 256:
        # the floor is in use: stream 2's first frame is all silence (1024 + four hops of it), 80 dB below the upper bound
        assert (np.stack([o[2] for o in out]) < np.float32(db_range[1]) - np.float32(80.0)).any()


@pytest.mark.parametrize("hop,n_filters,plan", [
    (160, 13, "ragged"), (160, 40, "1-1-1-37"), (160, 40, "3-0-5-32"), (160, 40, "20x2"), (160, 40, "ragged"),
    (160, 80, "ragged"), (256, 40, "3-0-5-32"), (256, 40, "ragged"), (1024, 40, "1-1-1-37"), (1024, 40, "ragged")])
def test_a_cut_run_equals_the_uncut_run(torch_cuda, hop, n_filters, plan):
    """hop 256: Lg * hop == n_fft / 2 exactly; hop 1024: Lg = 1, every hop completes a frame."""
    from lsm_speech_classifier_amd import frontend
    out, state, db_range = _uncut(torch_cuda, n_filters, hop)
    ms = frontend.MelStream(n_filters, N_STREAMS, db_range, thresholds=THR, gap=GAP, hop=hop)
    cut, cut_state = _push_plan(torch_cuda, ms, _audio(hop), PLANS[plan])
    for b in range(N_STREAMS):
        for got, want, what in zip(cut[b], out[b], ("raster", "power", "dB")):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{what} of stream {b}, plan {plan}"
    assert cut_state.tobytes() == state.tobytes(), f"final state blocks, plan {plan}"
    assert ms.seen.tolist() == [HOPS] * N_STREAMS


class _Raw:
    """`lsm_mel_stream_f32` called directly with the tables of a MelStream: what the class does not expose (state_in and
    state_out apart, NULL pointers, bad arguments)."""

    def __init__(self, torch, ms):
        from lsm_speech_classifier_amd import _lib
        self.torch, self.ms, self.lib = torch, ms, _lib.load()
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self, audio, H, hops, state_in, state_out, raster, power=None, db=None, ws=None, **kw):
        ms, torch = self.ms, self.torch
        ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        if ws is None:
            ws = torch.empty((max(int(self.lib.lsm_mel_stream_workspace(ms.n_streams, ms.n_filters, max(H, 1))), 256),),
                             dtype=torch.uint8, device="cuda")
        a = dict(n_streams=ms.n_streams, n_fft=N_FFT, hop=ms.hop, n_mels=ms.n_filters, lo=ms.db_lo, hi=ms.db_hi,
                 n_thr=ms.n_thr, red=ms.redundancy, window=ms.window, twiddle=ms.twiddle, basis=ms.basis, flo=ms.lo,
                 fhi=ms.hi, ws_bytes=0 if isinstance(ws, int) else int(ws.numel()))
        a.update(kw)
        return self.lib.lsm_mel_stream_f32(
            ptr(audio), a["n_streams"], H, a["n_fft"], a["hop"], ptr(a["window"]), ptr(a["twiddle"]), ptr(a["basis"]),
            ptr(a["flo"]), ptr(a["fhi"]), a["n_mels"], ptr(hops), a["lo"], a["hi"], C.c_void_p(ms.on.ctypes.data),
            C.c_void_p(ms.off.ctypes.data), a["n_thr"], a["red"], ptr(state_in), ptr(state_out), ptr(raster), ptr(power),
            ptr(db), ptr(ws), a["ws_bytes"], self.stream)


def test_zero_hops_and_separate_state_buffers(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, hop = 40, 160
    _, db_range = _oracle(F, hop)
    audio = torch.from_numpy(_audio(hop)).cuda()
    ms = frontend.MelStream(F, N_STREAMS, db_range)
    ms.push(audio[:, :10 * hop])
    raw = _Raw(torch, ms)
    s0 = ms.state.clone()
    assert s0.any()
    H = 5
    chunk = audio[:, 10 * hop:15 * hop].contiguous()
    zeros = torch.zeros(N_STREAMS, dtype=torch.int32, device="cuda")

    def outputs():
        return (_filled(torch, (N_STREAMS, F, H * 4), torch.uint8), _filled(torch, (N_STREAMS, F, H), torch.float32),
                _filled(torch, (N_STREAMS, F, H), torch.float32))

    # explicit all-zero stream_hops, in place: the state and every output stay as they are
    raster, power, db = outputs()
    state = s0.clone()
    assert raw(chunk, H, zeros, state, state, raster, power, db) == 0
    torch.cuda.synchronize()
    assert torch.equal(state, s0)
    for t in (raster, power, db):
        assert bool((t.view(torch.uint8) == FILL).all())
    # ... out of place: the blocks travel byte for byte; without a state_in they are zeros
    other = torch.full_like(s0, 0x3C)
    assert raw(chunk, H, zeros, s0, other, raster, power, db) == 0
    fresh = torch.full_like(s0, 0x3C)
    assert raw(chunk, H, zeros, None, fresh, raster, power, db) == 0
    torch.cuda.synchronize()
    assert torch.equal(other, s0) and not fresh.any() and bool((raster == FILL).all())
    # five hops: state_in != state_out equals the in-place run, and state_in is left as it was
    r1, p1, d1 = outputs()
    state = s0.clone()
    assert raw(chunk, H, None, state, state, r1, p1, d1) == 0
    r2, p2, d2 = outputs()
    kept, other = s0.clone(), torch.full_like(s0, 0x3C)
    assert raw(chunk, H, None, kept, other, r2, p2, d2) == 0
    torch.cuda.synchronize()
    assert torch.equal(kept, s0) and torch.equal(other, state) and not torch.equal(state, s0)
    assert torch.equal(r1, r2) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32)) and bool((r1 != FILL).all())
    # no state_in: a stream's start, as from a block of zeros; no state_out: nothing is kept
    z = torch.zeros_like(s0)
    first = audio[:, :10 * hop].contiguous()
    r3 = _filled(torch, (N_STREAMS, F, 40), torch.uint8)
    r4 = _filled(torch, (N_STREAMS, F, 40), torch.uint8)
    assert raw(first, 10, None, None, None, r3) == 0 and raw(first, 10, None, z, z, r4) == 0
    torch.cuda.synchronize()
    assert torch.equal(r3, r4) and torch.equal(z, s0)
    assert bool((r3[:, :, :16] != FILL).all()) and bool((r3[:, :, 16:] == FILL).all())      # 10 hops: 4 frames


@pytest.mark.parametrize("redundancy,thr,gap", [(2, THR, GAP), (1, [0.8], 0.1), (2, [0.1, 0.3, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95], 0.05),
                                                (1, [0.35, 0.55, 0.75, 0.9], -0.05), (1, [0.6, 0.8, 0.9], -0.2)])
def test_other_parameters(torch_cuda, oracle_c, redundancy, thr, gap):
    """Row repeat, one, three (byte stores) and eight thresholds, and off-thresholds ABOVE their on-thresholds (an active
    latch can see both comparisons true and is cleared): uncut against the oracle's encoder, cut against uncut."""
    from lsm_speech_classifier_amd import frontend
    F = 13
    out, state, db_range = _uncut(torch_cuda, F, 160, redundancy, thr, gap)
    want = _check_raster(oracle_c, out, db_range, thr, gap, redundancy)
    assert out[0][0].shape == (F * redundancy, _ncols(160) * len(thr))
    for k in range(len(thr)):
        assert want[:, :, k::len(thr)].any(), f"threshold plane {k} is empty"
    if gap < 0:
        on, off = frontend.threshold_tables(thr, gap, np.float32)
        assert (off > on).all()
    ms = frontend.MelStream(F, N_STREAMS, db_range, thresholds=thr, gap=gap, redundancy=redundancy)
    cut, cut_state = _push_plan(torch_cuda, ms, _audio(), PLANS["ragged"])
    for b in range(N_STREAMS):
        assert cut[b][0].tobytes() == out[b][0].tobytes(), f"stream {b}"
    assert cut_state.tobytes() == state.tobytes()


def test_start_of_a_stream_and_reset(torch_cuda):
    """The first six hops of a stream complete no frame, the seventh completes frame 0; after reset([1]) that stream alone
    starts over and equals a fresh stream on the remaining audio."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, hop = 40, 160
    out, _, db_range = _uncut(torch, F, hop)
    audio = _audio(hop)
    ms = frontend.MelStream(F, N_STREAMS, db_range)
    assert not ms.state.any()
    got = [[] for _ in range(N_STREAMS)]

    def push(bank, first_hop, hops, into):
        """Every stream's hops [first_hop[b], first_hop[b] + hops[b])."""
        H = max(max(hops), 1)
        chunk = np.zeros((bank.n_streams, H * hop), dtype=np.float32)
        for b in range(bank.n_streams):
            chunk[b, :hops[b] * hop] = audio[b, first_hop[b] * hop:(first_hop[b] + hops[b]) * hop]
        raster, cols = bank.push(chunk, np.asarray(hops))
        for b in range(bank.n_streams):
            into[b].append(raster[b, :, :cols[b] * 4].cpu().numpy())
        return cols.tolist()

    assert push(ms, [0, 0, 0], [6, 6, 6], got) == [0, 0, 0]
    assert push(ms, [6, 6, 6], [1, 1, 1], got) == [1, 1, 1]
    for b in range(N_STREAMS):
        np.testing.assert_array_equal(np.concatenate(got[b], axis=1), out[b][0][:, :4], err_msg=f"frame 0 of stream {b}")
    assert push(ms, [7, 7, 7], [5, 5, 5], got) == [5, 5, 5]
    ms.reset([1])
    assert not ms.state[1].any() and ms.state[0].any() and ms.state[2].any() and ms.seen.tolist() == [12, 0, 12]
    got[1] = []
    # stream 1 now runs the audio from hop 12 on as a stream of its own
    assert push(ms, [12, 12, 12], [3, 3, 3], got) == [3, 0, 3]
    assert push(ms, [15, 15, 15], [25, 25, 25], got) == [25, 22, 25]
    for b in (0, 2):
        np.testing.assert_array_equal(np.concatenate(got[b], axis=1), out[b][0], err_msg=f"stream {b}")
    fresh = frontend.MelStream(F, N_STREAMS, db_range)
    alone = [[] for _ in range(N_STREAMS)]
    assert push(fresh, [12, 12, 12], [0, 28, 0], alone) == [0, 22, 0]
    restarted = np.concatenate(got[1], axis=1)
    assert restarted.shape == (F, 22 * 4) and restarted.tobytes() == np.concatenate(alone[1], axis=1).tobytes()
    assert restarted.any() and torch.equal(ms.state[1], fresh.state[1])


def test_a_nan_sample(torch_cuda, oracle_c):
    """One NaN sample in stream 0: exactly the frames that contain it have NaN power and dB in every filter and repeat the
    previous raster column; every other frame, and the other streams, are those of the clean run bit for bit."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    F, hop, at = 40, 160, 4201
    out, state, db_range = _uncut(torch, F, hop)
    audio = _audio(hop).copy()
    audio[0, at] = np.nan
    ms = frontend.MelStream(F, N_STREAMS, db_range)
    bad, bad_state = _push_plan(torch, ms, audio, [HOPS])
    ncols = _ncols(hop)
    hit = np.array([t * hop - N_FFT // 2 <= at < t * hop + N_FFT // 2 for t in range(ncols)])
    assert hit.sum() == -(-N_FFT // hop) and hit[20] and hit[32] and not hit[19] and not hit[33]
    raster, power, db = bad[0]
    assert np.isnan(db[:, hit]).all() and np.isnan(power[:, hit]).all()
    assert not np.isnan(db[:, ~hit]).any()
    assert power[:, ~hit].tobytes() == out[0][1][:, ~hit].tobytes() and db[:, ~hit].tobytes() == out[0][2][:, ~hit].tobytes()
    cols = raster.reshape(F, ncols, 4)
    for t in np.nonzero(hit)[0]:
        assert cols[:, t].tobytes() == cols[:, t - 1].tobytes(), f"frame {t} does not repeat frame {t - 1}"
    assert cols[:, 19].any(), "the latches were all off when the NaN arrived: nothing is kept"
    for b in (1, 2):
        for got, want, what in zip(bad[b], out[b], ("raster", "power", "dB")):
            assert got.tobytes() == want.tobytes(), f"{what} of stream {b}"
    assert bad_state[1:].tobytes() == state[1:].tobytes()
    # the NaN has left the history (13 frames later): stream 0 has recovered, its samples apart
    want = _expected_raster(oracle_c, np.stack([o[2] for o in bad]), db_range)
    for b in range(N_STREAMS):
        np.testing.assert_array_equal(bad[b][0], want[b], err_msg=f"raster of stream {b}")
    # cut at hop boundaries inside the NaN frames: the same bytes
    ms2 = frontend.MelStream(F, N_STREAMS, db_range)
    cut, cut_state = _push_plan(torch, ms2, audio, [19, 1, 0, 6, 14])
    assert cut[0][0].tobytes() == raster.tobytes() and cut_state.tobytes() == bad_state.tobytes()
    assert cut[0][2].tobytes() == db.tobytes()


def test_refusals_launch_nothing(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib, frontend
    F, n, H, hop = 40, 2, 4, 160
    ms = frontend.MelStream(F, n, (-60.0, -10.0))
    raw = _Raw(torch, ms)
    lib = raw.lib
    nbytes = lib.lsm_mel_stream_state_bytes(F, N_FFT, hop)
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes >= 1984 * 4 + F * 4 + 4 and nbytes == ms.state_bytes
    for bad in ((0, N_FFT, hop), (F, 1024, hop), (F, N_FFT, 127), (F, N_FFT, 1025)):
        assert lib.lsm_mel_stream_state_bytes(*bad) == 0
    need = lib.lsm_mel_stream_workspace(n, F, H)
    assert need >= n * F * H * 4 and lib.lsm_mel_stream_workspace(n, 0, H) == 0 and lib.lsm_mel_stream_workspace(n, F, 0) == 0
    audio = torch.zeros((n, H * hop + 4), dtype=torch.float32, device="cuda")
    state = torch.full((n, nbytes + 16), 0x3C, dtype=torch.uint8, device="cuda")
    raster = torch.full((n, F, H * 4 + 4), FILL, dtype=torch.uint8, device="cuda")
    power = torch.full((n, F, H + 1), -7.0, dtype=torch.float32, device="cuda")
    db = torch.full((n, F, H + 1), -7.0, dtype=torch.float32, device="cuda")
    hops = torch.full((n + 1,), H, dtype=torch.int32, device="cuda")
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")

    def run(H=H, a=audio.data_ptr(), hp=hops.data_ptr(), s_in=state.data_ptr(), s_out=state.data_ptr(),
            r=raster.data_ptr(), p=power.data_ptr(), d=db.data_ptr(), w=ws.data_ptr(), **kw):
        kw.setdefault("ws_bytes", need)
        return raw(a or None, H, hp or None, s_in or None, s_out or None, r or None, p or None, d or None, w or None, **kw)

    cases = [
        (lambda: run(n_fft=1024), "n_fft"), (lambda: run(n_fft=4096), "n_fft"), (lambda: run(hop=127), "hop=127"),
        (lambda: run(hop=1025), "hop=1025"), (lambda: run(n_mels=0), "n_mels"), (lambda: run(H=0), "n_hops=0"),
        (lambda: run(H=-2), "n_hops"), (lambda: run(lo=-10.0, hi=-10.0), "db_lo < db_hi"),
        (lambda: run(lo=-10.0, hi=-60.0), "db_lo < db_hi"), (lambda: run(lo=float("nan")), "finite"),
        (lambda: run(hi=float("inf")), "finite"), (lambda: run(lo=float("-inf")), "finite"),
        (lambda: run(r=0), "raster_out is required"), (lambda: run(ws_bytes=need - 256), "workspace of"),
        (lambda: run(ws_bytes=0), "workspace of"), (lambda: run(r=raster.data_ptr() + 2), "raster_out is misaligned"),
        (lambda: run(a=audio.data_ptr() + 2), "audio is misaligned"), (lambda: run(window=ms.window.data_ptr() + 8), "window"),
        (lambda: run(twiddle=ms.twiddle.data_ptr() + 8), "twiddle"), (lambda: run(basis=ms.basis.data_ptr() + 2), "basis"),
        (lambda: run(hp=hops.data_ptr() + 2), "stream_hops is misaligned"),
        (lambda: run(s_in=state.data_ptr() + 8), "state_in is misaligned"),
        (lambda: run(s_out=state.data_ptr() + 8), "state_out is misaligned"),
        (lambda: run(p=power.data_ptr() + 2), "power_out is misaligned"), (lambda: run(d=db.data_ptr() + 2), "db_out is misaligned"),
        (lambda: run(w=ws.data_ptr() + 4), "workspace is misaligned"), (lambda: run(n_thr=0), "n_thr"),
        (lambda: run(n_thr=9), "n_thr"), (lambda: run(red=0), "redundancy"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        with pytest.raises(_lib.LsmHipError, match=words):
            _lib.check(rc, "refused")
    torch.cuda.synchronize()
    assert bool((raster == FILL).all()) and bool((power == -7.0).all()) and bool((db == -7.0).all()) \
        and bool((state == 0x3C).all()) and bool((ws == 0x5A).all()), "a refused call wrote to its outputs"
    # the Python layer refuses before it calls the library
    with pytest.raises(ValueError, match="n_filters"):
        frontend.MelStream(0, 2, (-60.0, -10.0))
    for bad in ((-10.0, -60.0), (-10.0, -10.0), (float("nan"), 0.0), (-60.0, float("inf"))):
        with pytest.raises(ValueError, match="db_range"):
            frontend.MelStream(8, 2, bad)
    for bad in (127, 1025):
        with pytest.raises(ValueError, match="hop"):
            frontend.MelStream(8, 2, (-60.0, -10.0), hop=bad)
    ms.push(np.zeros((2, 3 * hop), dtype=np.float32))
    seen, before = ms.seen.copy(), ms.state.clone()
    for bad in ((5, 0), (0, -1), (1,), (1.0, 2.0)):
        with pytest.raises(ValueError, match="hops"):
            ms.push(np.zeros((2, 4 * hop), dtype=np.float32), np.asarray(bad))
    for shape in ((2, 4 * hop + 1), (3, 4 * hop), (2, 0)):
        with pytest.raises(ValueError, match="audio"):
            ms.push(np.zeros(shape, dtype=np.float32))
    with pytest.raises(ValueError, match="raster_out"):
        ms.push(np.zeros((2, 4 * hop), dtype=np.float32), raster_out=torch.zeros((2, F, 15), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert ms.seen.tolist() == seen.tolist() == [3, 3] and torch.equal(ms.state, before)


def test_mel_db_range_is_the_absolute_floored_range(torch_cuda):
    from lsm_speech_classifier_amd import frontend, synth
    from oracle import ref_numpy
    fe = frontend.SpikeFrontEnd(16, "mel")
    clips = synth.class_chirps([0, 3, 7], seed=12)
    clips[1] *= 1e-6                                                    # far below: the 80 dB floor decides the lower bound
    lo, hi = fe.mel_db_range(clips)
    assert isinstance(lo, float) and isinstance(hi, float)
    db = 10 * np.log10(np.maximum(1e-10, np.stack([ref_numpy.mel_power(a, 16) for a in clips]).astype(np.float64)))
    assert abs(hi - db.max()) <= 1e-4 and db.min() < db.max() - 80 and lo == hi - 80.0
    # un-floored: white noise, whose quietest mel power value lies well inside 80 dB of its loudest.  The bound on lo is what
    # SPEC.md 1.5's power tolerance (1e-5 relative + 2e-6 of the peak) allows at that smallest value, plus the 1e-4 dB of log10
    noise = synth.white_noise(2, seed=31)
    p_ref = np.stack([ref_numpy.mel_power(a, 16) for a in noise]).astype(np.float64)
    db2 = 10 * np.log10(np.maximum(1e-10, p_ref))
    assert db2.min() > db2.max() - 80 + 1.0
    tol_lo = 10 * np.log10(1 + 1e-5 + 2e-6 * p_ref.max() / p_ref.min()) + 1e-4
    lo2, hi2 = fe.mel_db_range(noise)
    print(f"mel_db_range on noise: |hi - oracle| = {abs(hi2 - db2.max()):.3e}, |lo - oracle| = {abs(lo2 - db2.min()):.3e} "
          f"(bound {tol_lo:.3e}) dB")
    assert abs(hi2 - db2.max()) <= 1e-4 and abs(lo2 - db2.min()) <= tol_lo and tol_lo < 0.01
    with pytest.raises(ValueError, match="mel"):
        frontend.SpikeFrontEnd(16, "gammatone").mel_db_range(clips)
    with pytest.raises(ValueError, match="mel"):                        # db_range stays the gammatone front end's
        fe.db_range(clips)


def test_audio_stream_bank_end_to_end(torch_cuda, oracle_c):
    """Audio in, sliding-window rows out: ragged pushes through AudioStreamBank over a MelStream equal StreamBank fed with
    the uncut raster of the first test in one push."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline, reservoir as R, snn
    F, S, K, H, hop = 40, 8, 3, 1, 160
    out, _, db_range = _uncut(torch, F, hop)
    steps = _ncols(hop) * 4
    G = steps // S
    assert steps == 136 and G == 17
    uncut = np.stack([o[0] for o in out])
    res = R.build_reservoir(R.SimulationParams(num_neurons=200, num_output_neurons=40, small_world_graph_k=40,
                                               mean_weight=2.0 / 20, refractory_period=2), F)
    net = snn.SNN(None, reservoir=res)
    bank = pipeline.StreamBank(net, N_STREAMS, S, K, H, ALL_KEYS)
    want, want_counts = bank.push(uncut[:, :, :G * S], [G] * N_STREAMS)
    assert want_counts.tolist() == [G - K + 1] * N_STREAMS
    want = want[:, :G - K + 1].cpu().numpy()
    for b in range(N_STREAMS):
        sm = oracle_c.lif_run(res, uncut[b][:, :G * S], ALL_KEYS)[1]
        assert sm[:, res.out_idx].any(), f"the reservoir's output neurons stay silent on stream {b}"
    ms = frontend.MelStream(F, N_STREAMS, db_range)
    abank = pipeline.AudioStreamBank(ms, net, S, K, H, ALL_KEYS)
    audio = _audio(hop)
    done = np.zeros(N_STREAMS, dtype=np.int64)
    got = [[] for _ in range(N_STREAMS)]
    emitted = np.zeros(N_STREAMS, dtype=np.int64)
    for new in PLANS["ragged"]:
        Hh = max(int(new.max()), 1)
        chunk = np.full((N_STREAMS, Hh * hop), 7.0, dtype=np.float32)
        for b in range(N_STREAMS):
            chunk[b, :new[b] * hop] = audio[b, done[b] * hop:(done[b] + new[b]) * hop]
        rows, counts = abank.push(chunk, new)
        done += new
        # frames so far -> steps -> segments -> windows
        segs = frontend.mel_stream_frame_plan(0, done) * 4 // S
        total = np.where(segs >= K, (segs - K) // H + 1, 0)
        assert counts.tolist() == (total - emitted).tolist(), f"counts after {done.tolist()} hops"
        emitted = total
        for b in range(N_STREAMS):
            got[b].append(rows[b, :counts[b]].cpu().numpy())
            assert not rows[b, counts[b]:].any()
    for b in range(N_STREAMS):
        rows_b = np.concatenate(got[b])
        assert rows_b.shape == want[b].shape and rows_b.tobytes() == want[b].tobytes(), f"stream {b}"
        assert rows_b.any()
    # a stream ends, a new one takes its slot: both halves and the pending columns start over
    abank.reset([2])
    assert not ms.state[2].any() and abank.pending_steps[2] == 0 and abank.bank.seen.tolist()[2] == 0
    chunk = np.zeros((N_STREAMS, HOPS * hop), dtype=np.float32)
    chunk[2] = audio[2]
    rows, counts = abank.push(chunk, np.array([0, 0, HOPS]))
    assert counts.tolist() == [0, 0, G - K + 1]
    assert rows[2, :counts[2]].cpu().numpy().tobytes() == want[2].tobytes()
