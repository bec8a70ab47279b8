"""The resampler's kernels over the range the C ABI accepts (`lsm_resample_f32`, `lsm_resample_stream_f32` through ctypes), with
tap tables that no packaged design produces -- byte for byte against the NumPy restatement (resample_restatement.py) and,
per output, within the derived bound of the definition (fir_definition.py):

    up/down, K          what it reaches
    1/2, 1100           Hs = 1099: the state shift runs three chunks of 512, the last one partial
    3/2, 2000           Hs = 666: rows of 667, 667 and 666 taps; two chunks
    5/4, 10             every row has 2 taps, an even count, so the row stride is padded to 3
    7/3, 5              K < up: Hs = 0; phases 5 and 6 are empty, their outputs +0.0; a 16-byte state block
    2/1, 1              one tap
    640/441, 19840      a table of 158 720 bytes: rows of 31 taps, more than one tile
    4096/4095, 20480    163 840 bytes, exactly the LDS of a compute unit; one tap more is refused"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_definition as D  # noqa: E402
import resample_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xAA                          # behind outputs
PAD = 0x3C                           # a state block's padding at a stream's start
TABLES = {f"{up}/{down}-K{K}": (up, down, K) for up, down, K in D.RANGE_TABLES}
DTYPES = {"f32": np.float32, "i16": np.int16}
# Blocks of a whole stream run: its outputs cross one tile of 2048 by an uneven remainder where `up` allows it.  The plans
# below cut it into pushes, rows of per-stream block counts, that add up to it for every stream.
STREAM_TOTAL = {"1/2-K1100": 2200, "3/2-K2000": 700, "5/4-K10": 420, "7/3-K5": 300, "2/1-K1": 1100, "640/441-K19840": 4,
                "4096/4095-K20480": 4}
# pushes that advance by less than Hs, by between 512 samples and Hs, and by more than Hs; idle pushes
LONG_HISTORY = {"1/2-K1100": [(1, 300, 600), (0, 0, 0), (300, 600, 1), (0, 5, 0), (600, 1, 300), (5, 0, 5), (1294,) * 3],
                "3/2-K2000": [(1, 300, 350), (0, 0, 0), (300, 350, 1), (0, 5, 0), (350, 1, 300), (5, 0, 5), (44,) * 3]}
_CACHE = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch, _lib.load(), torch.cuda.current_stream().cuda_stream


def _table(name):
    if name not in _CACHE:
        _CACHE[name] = D.range_table(*TABLES[name])
    return _CACHE[name]


def _plan(name):
    total = STREAM_TOTAL[name]
    plan = LONG_HISTORY.get(name) or [(1, 2, 0), (0, 0, 0), (2, 0, 1), (0, 1, 2), (total - 3,) * 3]
    assert all(sum(p[b] for p in plan) == total for b in range(3)) and min(plan[-1]) > 0
    return plan


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _state_bytes(lib, t):
    n = int(lib.lsm_resample_state_bytes(len(t.taps), t.up))
    assert n == max(16, (4 * t.history + 15) // 16 * 16)
    return n


def _batch(gpu, x, t, delay, n_out):
    """`lsm_resample_f32` over the rows of ``x`` into a buffer with a canary behind it -> (n, n_out) float32."""
    torch, lib, stream = gpu
    n, n_in = x.shape
    buf = torch.full(((n * n_out + 64) * 4,), FILL, dtype=torch.uint8, device="cuda")
    audio, taps = torch.from_numpy(x).cuda(), torch.from_numpy(t.taps).cuda()
    rc = lib.lsm_resample_f32(_ptr(audio), int(x.dtype == np.int16), n, n_in, _ptr(taps), len(t.taps), t.up, t.down, delay,
                              n_out, _ptr(buf), stream)
    assert rc == 0, (rc, lib.lsm_last_error())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[n * n_out * 4:] == FILL).all(), "written behind out"
    return got[:n * n_out * 4].view(np.float32).reshape(n, n_out)


def _stream(gpu, chunk, t, blocks, state_in, state_out):
    """`lsm_resample_stream_f32` over the rows of ``chunk`` (n, G * down) -> the whole of out (n, G * up * 4) as bytes, the
    canaries behind every stream's count included."""
    torch, lib, stream = gpu
    n, G = chunk.shape[0], chunk.shape[1] // t.down
    out = torch.full((n, G * t.up * 4), FILL, dtype=torch.uint8, device="cuda")
    audio, taps = torch.from_numpy(chunk).cuda(), torch.from_numpy(t.taps).cuda()
    counts = None if blocks is None else torch.tensor(list(blocks), dtype=torch.int32, device="cuda")
    rc = lib.lsm_resample_stream_f32(_ptr(audio), int(chunk.dtype == np.int16), n, G, _ptr(taps), len(t.taps), t.up, t.down,
                                     _ptr(counts), _ptr(state_in), _ptr(state_out), _ptr(out), stream)
    assert rc == 0, (rc, lib.lsm_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(TABLES))
def test_batch_over_the_range(gpu, name, dtype):
    t = _table(name)
    x = D.range_input(t, DTYPES[dtype])
    n_out = D.RANGE_N_OUT
    delays = D.range_delays(t)
    assert delays[0] == 0 and delays[-1] * t.down <= len(t.taps) - 1 < (delays[-1] + 1) * t.down
    # the batch form is z[m + delay]: one causal run per clip serves every delay
    runs = [D.resample(row, t, 0, n_out + delays[-1]) for row in x]
    for delay in delays:
        got = _batch(gpu, x, t, delay, n_out)
        worst = 0.0
        for b, row in enumerate(x):
            want = R.causal(row, t, delay, n_out)
            assert got[b].tobytes() == want.tobytes(), f"delay {delay} row {b}: max |diff| = {np.abs(got[b] - want).max():.3e}"
            ref, S = (v[delay:delay + n_out] for v in runs[b])
            worst = max(worst, D.worst(got[b], ref, D.resample_bound(ref, S, t)))
        print(f"resample batch {name} {dtype} delay {delay}: worst err / bound = {worst:.4f}")
        assert worst <= 1.0
        empty = (np.arange(delay, delay + n_out, dtype=np.int64) * t.down) % t.up >= len(t.taps)
        assert empty.any() == (len(t.taps) < t.up)                 # 7/3 with 5 taps, 2/1 with one
        assert not got.view(np.uint32)[:, empty].any(), "an output of an empty phase is not +0.0"
        assert got[:, ~empty].any()


# ---- streams -------------------------------------------------------------------------------------------------------------
def _stream_input(name, dtype):
    t = _table(name)
    return D.pcm_noise(3, STREAM_TOTAL[name] * t.down, 31 * t.up + len(t.taps), DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(TABLES))
def test_streams_uncut_over_the_range(gpu, name, dtype):
    """One call, `stream_blocks` NULL (G everywhere) and `state_in` NULL (every stream starts)."""
    torch = gpu[0]
    t, x = _table(name), _stream_input(name, dtype)
    G, Hs = STREAM_TOTAL[name], t.history
    nbytes = _state_bytes(gpu[1], t)
    state = torch.full((3, nbytes), 0x5A, dtype=torch.uint8, device="cuda")
    got = _stream(gpu, x, t, None, None, state).view(np.float32)
    assert got.shape == (3, G * t.up)
    state = state.cpu().numpy()
    worst = 0.0
    for b in range(3):
        want = R.stream(x[b], t)
        assert got[b].tobytes() == want.tobytes(), f"stream {b}: max |diff| = {np.abs(got[b] - want).max():.3e}"
        ref, S = D.resample(x[b], t, 0, G * t.up)
        worst = max(worst, D.worst(got[b], ref, D.resample_bound(ref, S, t)))
        hist = R.widen(x[b]).astype(np.float32)[len(x[b]) - Hs:]
        assert state[b, :4 * Hs].tobytes() == hist.tobytes() and not state[b, 4 * Hs:].any()    # from no block: zeros behind
    print(f"resample streamed {name} {dtype}: worst err / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("in_place", [True, False], ids=["in-place", "out-of-place"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(TABLES))
def test_streams_cut_over_the_range(gpu, name, dtype, in_place):
    torch = gpu[0]
    t, x, plan = _table(name), _stream_input(name, dtype), _plan(name)
    Hs, down, up = t.history, t.down, t.up
    nbytes = _state_bytes(gpu[1], t)
    if name in LONG_HISTORY:
        adv = sorted({p[0] * down for p in plan})
        assert any(0 < a < Hs for a in adv) and any(512 <= a <= Hs for a in adv) and any(a > Hs for a in adv)
    # every stream starts from a history of zeros; the padding behind it is the caller's and travels with the block
    start = np.full((3, nbytes), PAD, dtype=np.uint8)
    start[:, :4 * Hs] = 0
    state = torch.from_numpy(start).cuda()
    x32 = np.stack([R.widen(row).astype(np.float32) for row in x])
    hist = np.zeros((3, Hs), dtype=np.float32)
    done, got = np.zeros(3, dtype=np.int64), [[] for _ in range(3)]
    for new in plan:
        G = max(max(new), 1)
        chunk = np.full((3, G * down), 7, dtype=x.dtype)
        for b in range(3):
            chunk[b, :new[b] * down] = x[b, done[b] * down:(done[b] + new[b]) * down]
        nxt = state if in_place else torch.full_like(state, 0x5A)
        out = _stream(gpu, chunk, t, new, state, nxt)
        state = nxt
        for b in range(3):
            got[b].append(out[b, :new[b] * up * 4].view(np.float32))
            assert (out[b, new[b] * up * 4:] == FILL).all(), "written behind a stream's samples"
            run = np.concatenate([hist[b], x32[b, done[b] * down:(done[b] + new[b]) * down]])
            hist[b] = run[len(run) - Hs:]
        done += np.asarray(new)
        # after every push: the histories, an idle stream's included, and the padding as it was
        block = state.cpu().numpy()
        assert block[:, :4 * Hs].tobytes() == hist.tobytes(), f"the state after the push {new}"
        assert (block[:, 4 * Hs:] == PAD).all(), "the padding of a state block changed"
    for b in range(3):
        want, final = R.stream_cut(x[b], t, [p[b] for p in plan])
        assert np.concatenate(got[b]).tobytes() == want.tobytes(), f"stream {b}: cut differs from the restatement"
        assert want.tobytes() == R.stream(x[b], t).tobytes() and final.tobytes() == hist[b].tobytes()


@pytest.mark.parametrize("name", list(TABLES))
def test_stream_blocks_outside_the_call_are_clamped(gpu, name):
    """Counts of (-3, G + 9, 2) are those of (0, G, 2): outputs, canaries and state, in place and out of place."""
    torch = gpu[0]
    t = _table(name)
    G = min(STREAM_TOTAL[name], 700)
    nbytes = _state_bytes(gpu[1], t)
    for dtype in DTYPES:
        chunk = D.pcm_noise(3, G * t.down, 77, DTYPES[dtype])
        start = np.full((3, nbytes), PAD, dtype=np.uint8)
        start[:, :4 * t.history] = np.ascontiguousarray(D.pcm_noise(3, t.history + 1, 78, np.float32)[:, 1:]).view(np.uint8)
        results = []
        for counts in ((-3, G + 9, 2), (0, G, 2)):
            state, other = torch.from_numpy(start).cuda(), torch.full((3, nbytes), 0x5A, dtype=torch.uint8, device="cuda")
            out = _stream(gpu, chunk, t, counts, state, other)
            same = state.clone()
            inplace = _stream(gpu, chunk, t, counts, same, same)
            assert state.cpu().numpy().tobytes() == start.tobytes(), "state_in was written"
            results.append((out.tobytes(), other.cpu().numpy().tobytes(), inplace.tobytes(), same.cpu().numpy().tobytes()))
        assert results[0] == results[1]
        out, block = np.frombuffer(results[1][0], dtype=np.uint8).reshape(3, -1), np.frombuffer(results[1][1], dtype=np.uint8)
        assert results[1][2] == results[1][0] and results[1][3] == results[1][1]
        block = block.reshape(3, nbytes)
        assert (out[0] == FILL).all() and (out[2, 2 * t.up * 4:] == FILL).all() and block[0].tobytes() == start[0].tobytes()
        for b, kb in ((1, G), (2, 2)):
            hist = start[b, :4 * t.history].view(np.float32)
            run = np.concatenate([hist, R.widen(chunk[b, :kb * t.down]).astype(np.float32)])
            want = R.causal(run, t, 0, kb * t.up, origin=t.history)
            assert out[b, :kb * t.up * 4].tobytes() == want.tobytes()
            assert block[b, :4 * t.history].tobytes() == run[len(run) - t.history:].tobytes()
            assert (block[b, 4 * t.history:] == PAD).all()


# ---- the edge of the LDS ---------------------------------------------------------------------------------------------------
def test_one_tap_over_the_lds_is_refused_and_writes_nothing(gpu):
    torch, lib, stream = gpu
    from lsm_speech_classifier_amd import _lib
    up, down, K = 4096, 4095, 20480
    assert up * (-(-K // up) | 1) * 8 == 160 * 1024 and up * (-(-(K + 1) // up) | 1) * 8 > 160 * 1024
    taps = torch.zeros(K + 1, dtype=torch.float64, device="cuda")
    audio = torch.zeros((3, 2 * down), dtype=torch.float32, device="cuda")
    out = torch.full((3, 2 * up), -7.0, dtype=torch.float32, device="cuda")
    nbytes = int(lib.lsm_resample_state_bytes(K + 1, up))
    assert nbytes == 32 and lib.lsm_resample_state_bytes(K, up) == 16
    state = torch.full((3, nbytes), PAD, dtype=torch.uint8, device="cuda")
    calls = (lambda k: lib.lsm_resample_f32(_ptr(audio), 0, 3, 2 * down, _ptr(taps), k, up, down, 0, 2 * up, _ptr(out), stream),
             lambda k: lib.lsm_resample_stream_f32(_ptr(audio), 0, 3, 2, _ptr(taps), k, up, down, None, _ptr(state), _ptr(state),
                                                   _ptr(out), stream))
    for call in calls:
        rc = call(K + 1)
        assert rc == -4
        with pytest.raises(_lib.LsmHipError, match="LDS"):
            _lib.check(rc, "refused")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((state == PAD).all()), "a refused call wrote to its outputs"
    for call in calls:                                              # exactly 160 KB is accepted
        assert call(K) == 0, lib.lsm_last_error()
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not np.signbit(out.cpu().numpy()).any()       # taps of zero: +0.0 everywhere
