"""Reverberation on the GPU (SPEC.md 1.11; `lsm_reverb_f32`, `lsm_reverb_stream_f32`, `frontend.Reverberator`,
`frontend.ReverbStream`, `HotPath(reverb=...)`, `features_from_audio(reverb=...)`, `AudioStreamBank(reverb=...)`): byte for
byte against the NumPy restatement (tests/reverb_restatement.py), cut against uncut byte for byte, the refusals; at the edges
of the tap loop -- its groups of 8, its chunks of 1024, one tap short of the 16384 a row can hold -- also per output within the
derived bound of the definition (tests/fir_definition.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_definition as D  # noqa: E402
import mix_restatement as M  # noqa: E402
import reverb_restatement as RR  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = np.float32(-1234.5)
_CACHE = {}


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


def _rir(rows, K, seed):
    """Decaying Gaussian rows, h[0] = 1."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((rows, K)) * 0.3 * np.exp(-np.arange(K) / max(1.0, K / 5.0))[None, :]
    h[:, 0] = 1.0
    return h.astype(np.float32)


def _same(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def _void(p):
    return C.c_void_p(p) if p else None


# ---- batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,K", [(1, 1, 1), (3, 5, 8), (4, 2049, 1), (4, 2049, 2), (5, 4100, 700), (2, 3000, 1500),
                                   (8, 1000, 16384)])
def test_batch_equals_the_restatement_byte_for_byte(torch_cuda, B, n, K):
    from lsm_speech_classifier_amd import frontend
    audio, bank = _noise(B, n, 100 + n + K), _rir(2, K, 200 + K)
    rows = np.arange(B, dtype=np.int32) % 2
    got = frontend.Reverberator(bank).reverb(audio, rows).cpu().numpy()
    want = RR.reverb(audio, bank, None, rows)
    assert got.shape == want.shape == (B, n) and want.any()
    assert _same(got, want)


def test_a_batch_over_65535_clips_is_cut_into_launches(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    B, n, K = 65535 + 70, 3, 2
    audio, bank = _noise(B, n, 5), _rir(2, K, 6)
    rows = (np.arange(B) % 3 - 1).astype(np.int32)                    # dry, row 0, row 1 in turn
    got = frontend.Reverberator(bank).reverb(audio, rows).cpu().numpy()
    want = np.empty_like(audio)
    for r in (-1, 0, 1):                                              # the restatement clip by clip is a loop of 65 605
        sel = rows == r
        ext = np.concatenate([np.zeros((int(sel.sum()), 1)), audio[sel].astype(np.float64)], axis=1)
        h = bank[max(r, 0)].astype(np.float64)
        want[sel] = audio[sel] if r < 0 else ((0.0 + h[0] * ext[:, 1:]) + h[1] * ext[:, :-1]).astype(np.float32)
    assert _same(want[:9], RR.reverb(audio[:9], bank, None, rows[:9])) and _same(got, want)


def test_rows_of_different_lengths_clamped_and_dry_rows_in_one_launch(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    K, n = 300, 2500
    bank = _rir(4, K, 7)
    lengths = np.array([1, K, 77, 200], dtype=np.int32)
    for r in range(4):
        bank[r, lengths[r]:] = np.float32(1e30)                       # garbage behind a row's end: never read
    audio = _noise(7, n, 8)
    audio[5, 3], audio[5, 10], audio[5, 11] = np.float32(-0.0), np.float32(np.nan), np.float32("inf")
    audio[5].view(np.uint32)[20] = 0x7FC12345                       # a NaN with a payload
    rows = np.array([0, 1, 2, 3, 4 + 5, -1, -7], dtype=np.int32)      # M + 5 is clamped to row 3; -1 and -7 are dry
    rv = frontend.Reverberator(bank, lengths)
    got = rv.reverb(audio, rows).cpu().numpy()
    want = RR.reverb(audio, bank, lengths, rows)
    assert _same(got, want)
    assert np.isfinite(got[:5]).all() and np.abs(got[:5]).max() < 1e3, "a tap behind a row's length reached the output"
    assert _same(got[4], RR.convolve(audio[4], bank[3, :200]))
    assert _same(got[5], audio[5]) and _same(got[6], audio[6])        # dry: the same bytes, -0.0 and the NaN's payload kept
    assert _same(got[0], audio[0])                                    # one tap of 1: the product is exact
    # no lengths: K everywhere, the garbage included
    full = frontend.Reverberator(bank).reverb(audio[:1], [2]).cpu().numpy()
    assert _same(full, RR.reverb(audio[:1], bank, None, [2])) and np.abs(full).max() > 1e20


def test_output_lengths_and_canaries(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    K, n, B = 130, 2100, 3
    bank, audio = _rir(2, K, 17), _noise(B, n, 18)
    rows = np.array([0, 1, -1], dtype=np.int32)
    rv = frontend.Reverberator(bank)
    for n_out in (1, 777, n, n + K - 1, n + K + 40):
        buf = torch.full((B * n_out + 64,), float(CANARY), dtype=torch.float32, device="cuda")
        out = buf[:B * n_out].view(B, n_out)
        assert rv.reverb(audio, rows, n_out=n_out, out=out) is out
        want = RR.reverb(audio, bank, None, rows, n_out)
        assert _same(out.cpu().numpy(), want), n_out
        assert bool((buf[B * n_out:] == float(CANARY)).all()), "the launch wrote behind out"
    tail = RR.reverb(audio, bank, None, rows, n + K - 1)
    ref = np.convolve(audio[0].astype(np.float64), bank[0].astype(np.float64))
    assert np.abs(tail[0] - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    assert not tail[2, n:].any() and not np.signbit(tail[2, n:]).any()          # a dry clip's samples behind n are +0.0


def test_non_finite_samples_stay_under_their_taps_and_in_their_clip(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    K, n, j = 64, 2300, 2040
    bank = _rir(1, K, 27)
    bank[0, 5] = 0.0                                                  # a zero tap
    lengths = np.array([40], dtype=np.int32)
    audio = _noise(3, n, 28)
    clean = frontend.Reverberator(bank, lengths).reverb(audio).cpu().numpy()
    audio[1, j] = np.nan
    audio[2, j] = np.inf
    got = frontend.Reverberator(bank, lengths).reverb(audio).cpu().numpy()
    assert _same(got, RR.reverb(audio, bank, lengths))
    assert _same(got[0], clean[0])
    nan = np.isnan(got[1])
    assert nan[j:j + 40].all() and nan.sum() == 40                    # exactly the len_r outputs whose taps cover it
    assert np.isnan(got[2, j + 5]) and np.isinf(got[2, j]) and np.isfinite(got[2, :j]).all() and np.isfinite(got[2, j + 40:]).all()
    assert (~np.isfinite(got[2])).sum() == 40


# ---- streams -------------------------------------------------------------------------------------------------------------
def _cuts(rng, total, K, n_streams):
    """Per-push counts (pushes, n_streams) that add up to `total` per stream: 0, 1, below and above K - 1, an idle stream."""
    menu = [0, 1, max(1, K - 2), K - 1 + 3, 2 * K + 50, 2049]
    plans = []
    for b in range(n_streams):
        left, cuts = total, []
        while left:
            c = min(left, int(menu[rng.integers(len(menu))]))
            cuts.append(c)
            left -= c
        plans.append(cuts)
    pushes = max(len(c) for c in plans) + 1
    table = np.zeros((pushes, n_streams), dtype=np.int64)
    for b, cuts in enumerate(plans):
        table[1:1 + len(cuts), b] = cuts                              # push 0: everybody idle
    return table


@pytest.mark.parametrize("in_place", [True, False], ids=["in-place", "out-of-place"])
@pytest.mark.parametrize("K", [2, 700, 1500])
def test_streams_cut_equal_the_uncut_run_and_the_restatement(torch_cuda, K, in_place):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    S, total = 4, 5000
    bank = _rir(3, K, 300 + K)
    lengths = np.array([K, max(1, K // 2), 1], dtype=np.int32)
    rows = np.array([0, 1, 2, -1], dtype=np.int32)
    x = _noise(S, total, 301 + K)
    x[3, 7] = np.float32(-0.0)
    rv = frontend.Reverberator(bank, lengths)
    lib, stream = rv.lib, torch.cuda.current_stream().cuda_stream
    sb = int(lib.lsm_reverb_state_bytes(K))
    assert sb == max(16, (4 * (K - 1) + 15) // 16 * 16)
    rows_dev = torch.from_numpy(rows).cuda()

    def run(table):
        state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
        got, at = [[] for _ in range(S)], np.zeros(S, dtype=np.int64)
        for new in table:
            H = max(1, int(new.max()))
            chunk = np.full((S, H), 7.0, dtype=np.float32)
            for b in range(S):
                chunk[b, :new[b]] = x[b, at[b]:at[b] + new[b]]
            a = torch.from_numpy(chunk).cuda()
            out = torch.full((S, H), float(CANARY), dtype=torch.float32, device="cuda")
            cnt = torch.from_numpy(new.astype(np.int32)).cuda()
            nxt = state if in_place else torch.full_like(state, 0x5A)
            rc = lib.lsm_reverb_stream_f32(_void(a.data_ptr()), S, H, _void(rv.rir.data_ptr()), 3, K,
                                           _void(rv.lengths_dev.data_ptr()), _void(rows_dev.data_ptr()), _void(cnt.data_ptr()),
                                           _void(state.data_ptr()), _void(nxt.data_ptr()), _void(out.data_ptr()), stream)
            assert rc == 0, lib.lsm_last_error()
            state = nxt
            o = out.cpu().numpy()
            for b in range(S):
                got[b].append(o[b, :new[b]])
                assert (o[b, new[b]:] == CANARY).all(), "samples of out behind count were written"
            at += new
        assert at.tolist() == [total] * S
        hist = state.cpu().numpy()[:, :4 * (K - 1)].copy().view(np.float32)
        return [np.concatenate(g) for g in got], hist

    uncut, hist_u = run(np.full((1, S), total, dtype=np.int64))
    cut, hist_c = run(_cuts(np.random.default_rng(K), total, K, S))
    batch = rv.reverb(x, rows).cpu().numpy()
    for b in range(S):
        want, st = RR.stream_cut(x[b], bank, [total], lengths, int(rows[b]))
        assert _same(uncut[b], want) and _same(cut[b], want) and _same(uncut[b], batch[b]), b
        assert _same(hist_u[b], st) and _same(hist_c[b], st), b
    assert np.signbit(uncut[3][7]) and uncut[3][7] == 0                # the dry stream keeps -0.0


def test_reverb_stream_set_reset_and_a_row_changed_between_pushes(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    K, S = 90, 3
    bank = _rir(2, K, 41)
    lengths = np.array([K, 30], dtype=np.int32)
    x = _noise(S, 400, 42)
    rs = frontend.ReverbStream(frontend.Reverberator(bank, lengths), S)
    rs.set([1, 2], [1, -1])
    o1, c1 = rs.push(x[:, :150], [150, 100, 150])
    rs.set([0, 2], [1, 0])                                            # the rows change; the histories stay
    o2, c2 = rs.push(x[:, 150:], [250, 0, 250])
    o3, _ = rs.push(x[1:2, 100:].repeat(S, axis=0), [0, 300, 0])
    assert c1.tolist() == [150, 100, 150] and c2.tolist() == [250, 0, 250]
    got = [np.concatenate([o1.cpu().numpy()[0, :150], o2.cpu().numpy()[0]]),
           np.concatenate([o1.cpu().numpy()[1, :100], o3.cpu().numpy()[1]]),
           np.concatenate([o1.cpu().numpy()[2, :150], o2.cpu().numpy()[2]])]
    want = [RR.stream_cut(x[0], bank, [150, 250], lengths, [0, 1]), RR.stream_cut(x[1], bank, [100, 300], lengths, 1),
            RR.stream_cut(x[2], bank, [150, 250], lengths, [-1, 0])]
    hist = rs.state.cpu().numpy()[:, :4 * (K - 1)].copy().view(np.float32)
    for b in range(S):
        assert _same(got[b], want[b][0]) and _same(hist[b], want[b][1]), b
    assert not o1.cpu().numpy()[1, 100:].any()                        # behind a count: the zeros of a fresh out
    rs.reset([1])
    assert not rs.state[1].any() and rs.state[0].any()
    with pytest.raises(ValueError, match="rows"):
        rs.set([0], [2])
    with pytest.raises(ValueError, match="out must not be audio"):
        a = o1.clone()
        rs.push(a, out=a)


# ---- the edges of the tap loop and of the ABI's ranges, through the C ABI ---------------------------------------------------
def _ptr(tensor):
    return None if tensor is None else C.c_void_p(tensor.data_ptr())


def _dev_ints(torch, values):
    return None if values is None else torch.from_numpy(np.asarray(values, dtype=np.int32)).cuda()


def _abi_batch(torch, audio, bank, lengths, rows, n_out):
    """`lsm_reverb_f32` into a buffer with canaries behind it -> (B, n_out) float32.  ``lengths`` and ``rows`` go as they
    are: nothing in front of the kernel looks at them."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    (B, n), (M_, K) = audio.shape, bank.shape
    a, h = torch.from_numpy(audio).cuda(), torch.from_numpy(bank).cuda()
    ln, rw = _dev_ints(torch, lengths), _dev_ints(torch, rows)
    buf = torch.full((B * n_out + 64,), float(CANARY), dtype=torch.float32, device="cuda")
    rc = lib.lsm_reverb_f32(_void(a.data_ptr()), B, n, _void(h.data_ptr()), M_, K, _ptr(ln),
                            _ptr(rw), n_out, _void(buf.data_ptr()),
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.lsm_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[B * n_out:] == CANARY).all(), "the launch wrote behind out"
    return got[:B * n_out].reshape(B, n_out)


def _abi_stream(torch, chunk, bank, lengths, rows, counts, state_in, state_out):
    """`lsm_reverb_stream_f32` -> the whole of out (S, n_cols), the canaries behind every count included."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    (S, H), (M_, K) = chunk.shape, bank.shape
    a, h = torch.from_numpy(chunk).cuda(), torch.from_numpy(bank).cuda()
    ln, rw, cn = _dev_ints(torch, lengths), _dev_ints(torch, rows), _dev_ints(torch, counts)
    out = torch.full((S, H), float(CANARY), dtype=torch.float32, device="cuda")
    rc = lib.lsm_reverb_stream_f32(_void(a.data_ptr()), S, H, _void(h.data_ptr()), M_, K, _ptr(ln),
                                   _ptr(rw), _ptr(cn),
                                   _ptr(state_in),
                                   _ptr(state_out), _void(out.data_ptr()),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.lsm_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _push_all(torch, x, bank, lengths, rows, table, in_place, start=None, pad=0):
    """Push ``x`` (S, total) in the pieces of ``table`` (pushes, S) -> (samples per stream, the final state blocks as
    bytes).  Out of place every call writes a fresh block prefilled with 0x5A; the first one reads ``start`` (None: NULL)."""
    S, K = x.shape[0], bank.shape[1]
    sb = max(16, (4 * (K - 1) + 15) // 16 * 16)
    state = None if start is None else torch.from_numpy(start).cuda()
    if in_place and state is None:
        state = torch.zeros((S, sb), dtype=torch.uint8, device="cuda")
    got, at = [[] for _ in range(S)], np.zeros(S, dtype=np.int64)
    for new in np.asarray(table, dtype=np.int64):
        H = max(1, int(new.max()))
        chunk = np.full((S, H), 7.0, dtype=np.float32)
        for b in range(S):
            chunk[b, :new[b]] = x[b, at[b]:at[b] + new[b]]
        nxt = state if in_place else torch.full((S, sb), 0x5A, dtype=torch.uint8, device="cuda")
        o = _abi_stream(torch, chunk, bank, lengths, rows, new, state, nxt)
        state = nxt
        for b in range(S):
            got[b].append(o[b, :new[b]])
            assert (o[b, new[b]:] == CANARY).all(), "samples of out behind count were written"
        at += new
    assert at.tolist() == [x.shape[1]] * S
    return [np.concatenate(g) for g in got], state.cpu().numpy()


def _edges():
    """The bank of `fir_definition.reverb_edge_bank`, one clip per row, the restatement and the definition with its bound."""
    if "edges" not in _CACHE:
        bank, lengths = D.reverb_edge_bank()
        audio = D.reverb_edge_audio()
        rows = np.arange(len(lengths), dtype=np.int32)
        want = RR.reverb(audio, bank, lengths, rows, D.REVERB_N_OUT)
        refs = [D.reverb(audio[r], bank[r, :lengths[r]], D.REVERB_N_OUT) for r in rows]
        bounds = [D.reverb_bound(ref, S, lengths[r]) for r, (ref, S) in enumerate(refs)]
        _CACHE["edges"] = (bank, lengths, audio, rows, want, [ref for ref, _ in refs], bounds)
    return _CACHE["edges"]


def test_row_lengths_at_the_edges_of_the_tap_loop_batch(torch_cuda):
    """Rows that end a tap in front of, at and behind a group of 8 and a chunk of 1024 -- 1025: a second chunk of one tap,
    nothing but the remainder group -- and one tap short of MAX_TAPS, 1e30 behind each row's length.  With the whole tail
    behind the clips, so that the last tap of the longest row meets a sample."""
    bank, lengths, audio, rows, want, refs, bounds = _edges()
    assert bank.shape == (12, 16384) and audio.shape == (12, 2100) and lengths.tolist() == list(D.REVERB_LENGTHS)
    got = _abi_batch(torch_cuda, audio, bank, lengths, rows, D.REVERB_N_OUT)
    worst = 0.0
    for r, n in enumerate(lengths):
        assert _same(got[r], want[r]), f"len {n}: max |diff| = {np.abs(got[r] - want[r]).max():.3e}"
        w = D.worst(got[r], refs[r], bounds[r])
        print(f"reverb batch len {n}: worst err / bound = {w:.4f}")
        worst = max(worst, w)
        assert got[r, D.REVERB_N + n - 2] != 0 and not got[r, D.REVERB_N + n - 1:].any()
    print(f"reverb batch: worst err / bound = {worst:.4f}")
    assert worst <= 1.0
    assert np.isfinite(got).all() and np.abs(got).max() < 1e3, "a tap behind a row's length reached the output"
    # n_out = n, the recipe's length, is the prefix
    short = _abi_batch(torch_cuda, audio, bank, lengths, rows, D.REVERB_N)
    assert _same(short, want[:, :D.REVERB_N])


def test_row_lengths_at_the_edges_of_the_tap_loop_streamed(torch_cuda):
    """The same clips as streams cut at 1, 2047 and the rest, then a push of zeros as long as the tail: the deepest taps
    of the longest row read the clip out of the history."""
    bank, lengths, audio, rows, want, refs, bounds = _edges()
    K, N = bank.shape[1], D.REVERB_N_OUT
    x = np.concatenate([audio, np.zeros((len(rows), N - D.REVERB_N), dtype=np.float32)], axis=1)
    cuts = list(D.REVERB_CUTS) + [N - D.REVERB_N]
    table = np.repeat(np.array(cuts, dtype=np.int64)[:, None], len(rows), axis=1)
    got, state = _push_all(torch_cuda, x, bank, lengths, rows, table, in_place=True)
    worst = 0.0
    assert state.shape == (12, 65536)
    for r, n in enumerate(lengths):
        assert _same(got[r], want[r]), f"len {n}: max |diff| = {np.abs(got[r] - want[r]).max():.3e}"
        w = D.worst(got[r], refs[r], bounds[r])
        print(f"reverb streamed len {n}: worst err / bound = {w:.4f}")
        worst = max(worst, w)
        assert _same(state[r, :4 * (K - 1)].view(np.float32), x[r, N - (K - 1):]) and not state[r, 4 * (K - 1):].any()
    print(f"reverb streamed: worst err / bound = {worst:.4f}")
    assert worst <= 1.0
    y, st = RR.stream_cut(x[9], bank, cuts, lengths, 9)
    assert _same(y, got[9]) and _same(st, state[9, :4 * (K - 1)].view(np.float32))


def test_rir_len_outside_its_range_is_clamped(torch_cuda):
    """`rir_len` of 0, -3 and K + 5 behaves as 1, 1 and K (the Python layer refuses such lengths; the ABI clamps them)."""
    K, n = 40, 2100
    bank, audio = _rir(3, K, 81), _noise(3, n, 82)
    bank[:2, 1:] = np.float32(1e30)                                   # rows 0 and 1 end behind their first tap
    raw, rule = np.array([0, -3, K + 5], dtype=np.int32), np.array([1, 1, K], dtype=np.int32)
    rows = np.array([0, 1, 2], dtype=np.int32)
    assert [RR.row_length(raw, r, K) for r in range(3)] == rule.tolist()
    want = RR.reverb(audio, bank, raw, rows, n + K)
    assert np.isfinite(want).all() and want.any(axis=1).all()
    for lengths in (raw, rule):
        assert _same(_abi_batch(torch_cuda, audio, bank, lengths, rows, n + K), want)
        got, state = _push_all(torch_cuda, audio, bank, lengths, rows, [[700] * 3, [1400] * 3], in_place=False)
        assert all(_same(got[b], want[b, :n]) for b in range(3))
        assert _same(state[:, :4 * (K - 1)].copy().view(np.float32), audio[:, n - (K - 1):])


@pytest.mark.parametrize("in_place", [True, False], ids=["in-place", "out-of-place"])
def test_count_outside_its_range_is_clamped(torch_cuda, in_place):
    """`count` of -1 and n_cols + 9 behaves as 0 and n_cols.  For 0 nothing is written to the row, and the state block
    stays as it is in place and is copied out of place."""
    torch = torch_cuda
    K, H, S = 40, 300, 3
    bank, x = _rir(1, K, 83), _noise(S, H, 84)
    sb = 160
    start = np.full((S, sb), 0x3C, dtype=np.uint8)                    # a word of padding behind the 39 samples
    start[:, :4 * (K - 1)] = _noise(S, K - 1, 85).view(np.uint8)
    raw, rule = [-1, H + 9, 5], [0, H, 5]
    assert [RR.push_count(raw, b, H) for b in range(S)] == rule
    results = []
    for counts in (raw, rule):
        state = torch.from_numpy(start).cuda()
        nxt = state if in_place else torch.full((S, sb), 0x5A, dtype=torch.uint8, device="cuda")
        out = _abi_stream(torch, x, bank, None, None, counts, state, nxt)
        assert in_place or state.cpu().numpy().tobytes() == start.tobytes(), "state_in was written"
        results.append((out, nxt.cpu().numpy()))
    (out, state), (out_rule, state_rule) = results
    assert _same(out, out_rule) and state.tobytes() == state_rule.tobytes()
    assert (out[0] == CANARY).all() and state[0].tobytes() == start[0].tobytes()
    for b in (1, 2):
        c = rule[b]
        y, st = RR.stream(x[b, :c], bank, start[b, :4 * (K - 1)].view(np.float32))
        assert _same(out[b, :c], y) and (out[b, c:] == CANARY).all()
        assert _same(state[b, :4 * (K - 1)].view(np.float32), st) and (state[b, 4 * (K - 1):] == 0x3C).all()


@pytest.mark.parametrize("in_place", [True, False], ids=["in-place", "out-of-place"])
def test_streams_of_one_tap(torch_cuda, in_place):
    """K = 1: no history, `have_hist` false, a state block of 16 bytes that is all padding."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    S, total = 3, 2500
    bank = np.array([[0.75], [-1.5]], dtype=np.float32)
    rows = np.array([0, 1, -1], dtype=np.int32)
    x = _noise(S, total, 86)
    x[2, 5] = np.float32(-0.0)
    assert _lib.load().lsm_reverb_state_bytes(1) == 16
    table = [[0, 0, 0], [1, 2100, 0], [2049, 0, 7], [450, 400, 2493]]
    start = np.full((S, 16), 0x3C, dtype=np.uint8)
    got, state = _push_all(torch, x, bank, None, rows, table, in_place, start=start)
    assert (state == 0x3C).all(), "the padding of a state block changed"
    for b in range(S):
        y, _ = RR.stream_cut(x[b], bank, [total], None, int(rows[b]))
        assert _same(got[b], y), b
    assert _same(got[0], x[0] * np.float32(0.75)) and _same(got[2], x[2])
    # every stream starts (state_in NULL): out of place the block is zeros
    got, state = _push_all(torch, x, bank, None, rows, [[total] * 3], in_place=False)
    assert not state.any() and _same(got[1], x[1] * np.float32(-1.5))
    # and no state at all
    out = _abi_stream(torch, x, bank, None, rows, None, None, None)
    assert all(_same(out[b], got[b]) for b in range(S))


def test_counts_that_end_inside_a_tile(torch_cuda):
    """513: the second wave owns one output; 2041: the last lane of the tile stores one of its 8; 2049: a second tile for one
    output.  Behind each count the canary stays."""
    torch = torch_cuda
    K, H = 130, 2100
    counts = [513, 2041, 2049]
    bank, x = _rir(2, K, 87), _noise(3, H, 88)
    rows = np.array([0, 1, 0], dtype=np.int32)
    sb = 528
    for in_place in (True, False):
        state = torch.zeros((3, sb), dtype=torch.uint8, device="cuda")
        nxt = state if in_place else torch.full((3, sb), 0x5A, dtype=torch.uint8, device="cuda")
        out = _abi_stream(torch, x, bank, None, rows, counts, state, nxt)
        state = nxt.cpu().numpy()
        for b, c in enumerate(counts):
            y, st = RR.stream(x[b, :c], bank, RR.new_state(K), None, int(rows[b]))
            assert _same(out[b, :c], y), f"count {c}"
            assert (out[b, c:] == CANARY).all(), f"count {c}: written behind it"
            assert _same(state[b, :4 * (K - 1)].view(np.float32), st) and not state[b, 4 * (K - 1):].any()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_abi_refusals(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    K, B, n = 16, 3, 40
    rv = frontend.Reverberator(_rir(2, K, 51))
    lib = rv.lib
    audio = torch.zeros((B, n + 4), dtype=torch.float32, device="cuda")
    out = torch.full((B, n + 4), -7.0, dtype=torch.float32, device="cuda")
    ints = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    sb = int(lib.lsm_reverb_state_bytes(K))
    state = torch.full((B, sb + 16), 0x3C, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    h = rv.rir.data_ptr()

    def batch(a=audio.data_ptr(), B=B, n=n, h=h, M_=2, K=K, ln=ints.data_ptr(), row=ints.data_ptr(), n_out=n,
              o=out.data_ptr()):
        return lib.lsm_reverb_f32(_void(a), B, n, _void(h), M_, K, _void(ln), _void(row), n_out, _void(o), stream)

    def streamed(a=audio.data_ptr(), B=B, n=n, h=h, M_=2, K=K, ln=ints.data_ptr(), row=ints.data_ptr(), cnt=ints.data_ptr(),
                 si=state.data_ptr(), so=state.data_ptr(), o=out.data_ptr()):
        return lib.lsm_reverb_stream_f32(_void(a), B, n, _void(h), M_, K, _void(ln), _void(row), _void(cnt), _void(si),
                                         _void(so), _void(o), stream)

    cases = []
    for f in (batch, streamed):
        cases += [
            (lambda f=f: f(K=0), "n_taps=0 outside \\[1, 16384\\]"), (lambda f=f: f(K=16385), "n_taps=16385 outside"),
            (lambda f=f: f(n=0), "=0 outside \\[1, 16777216\\]"), (lambda f=f: f(n=(1 << 24) + 1), "outside \\[1, 16777216\\]"),
            (lambda f=f: f(M_=0), "n_rir_rows=0"), (lambda f=f: f(B=-1), "rows outside"), (lambda f=f: f(B=65536), "rows outside"),
            (lambda f=f: f(a=0), "null buffer"), (lambda f=f: f(h=0), "null buffer"), (lambda f=f: f(o=0), "null buffer"),
            (lambda f=f: f(a=audio.data_ptr() + 2), "audio is misaligned"), (lambda f=f: f(h=h + 1), "rir is misaligned"),
            (lambda f=f: f(o=out.data_ptr() + 2), "out is misaligned"), (lambda f=f: f(ln=ints.data_ptr() + 2), "rir_len is misaligned"),
            (lambda f=f: f(row=ints.data_ptr() + 1), "rir_row is misaligned"),
            (lambda f=f: f(o=audio.data_ptr()), "out must not be audio"),
        ]
    cases += [
        (lambda: batch(n_out=0), "n_out=0"), (lambda: batch(n_out=-5), "n_out=-5"),
        (lambda: streamed(cnt=ints.data_ptr() + 2), "count is misaligned"),
        (lambda: streamed(si=state.data_ptr() + 8), "state_in is misaligned"),
        (lambda: streamed(so=state.data_ptr() + 4), "state_out is misaligned"),
    ]
    for i, (call, words) in enumerate(cases):
        rc = call()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        assert re.search(words, lib.lsm_last_error().decode()), f"refusal {i} ({words}): {lib.lsm_last_error().decode()!r}"
    assert lib.lsm_reverb_state_bytes(0) == 0 and lib.lsm_reverb_state_bytes(16385) == 0
    assert lib.lsm_reverb_state_bytes(1) == 16 and lib.lsm_reverb_state_bytes(6) == 32 and lib.lsm_reverb_state_bytes(16384) == 65536
    assert batch(B=0) == 0 and streamed(B=0) == 0 and batch(B=0, a=0, o=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((state == 0x3C).all()), "a refused call wrote"
    # every optional array absent, and the calls the refusals start from
    assert batch(ln=0, row=0) == 0 and streamed(ln=0, row=0, cnt=0, si=0, so=0) == 0
    assert batch() == 0 and streamed() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="out must not be audio"):
        rv.reverb(audio, out=audio)


# ---- end to end ----------------------------------------------------------------------------------------------------------
KEYS = ['spike_counts', 'mean_spike_times', 'mean_isi']


def _small_net(F):
    from lsm_speech_classifier_amd import reservoir as Rv, snn
    res = Rv.build_reservoir(Rv.SimulationParams(num_neurons=64, num_output_neurons=32, small_world_graph_k=8,
                                                 mean_weight=2.0 / 4, refractory_period=2), F)
    return snn.SNN(None, reservoir=res)


def _rooms():
    """A small bank for the end-to-end tests: (bank (3, 400), lengths, its Reverberator)."""
    from lsm_speech_classifier_amd import frontend
    if "rooms" not in _CACHE:
        bank, lengths = _rir(3, 400, 61), np.array([400, 150, 9], dtype=np.int32)
        _CACHE["rooms"] = (bank, lengths, frontend.Reverberator(bank, lengths))
    return _CACHE["rooms"]


def test_features_from_reverberated_audio_equal_those_of_the_restatement(torch_cuda):
    from lsm_speech_classifier_amd import frontend, pipeline, synth
    F, n = 8, 5
    bank, lengths, rv = _rooms()
    audio = synth.class_chirps(np.arange(n), seed=3)
    rooms = frontend.reverb_plan(n, 3, prob=0.8, seed=3)
    assert (rooms.rows < 0).any() and len(set(rooms.rows.tolist())) > 2
    wet = RR.reverb(audio, bank, lengths, rooms.rows)
    noise = _noise(3, 4097, 62, 0.05)
    mixer = frontend.NoiseMixer(noise)
    plan = frontend.mix_plan(n, 3, 4097, (0.0, 20.0), max_shift=1600, level_db=(-6.0, 0.0), seed=9)
    both, _, _ = M.mix(wet, noise, 10.0 ** (-plan.snr_db / 10.0), plan.rows, plan.offsets, plan.shift, plan.scale)
    fe, net = frontend.SpikeFrontEnd(F, "gammatone"), _small_net(F)
    for streams in (1, pipeline.DEFAULT_STREAMS):                   # the serial path and the two-stage topology
        got = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, reverb=(rv, rooms))
        want = pipeline.features_from_audio(wet, fe, net, KEYS, batch=2, streams=streams)
        clean = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams)
        assert got.shape == want.shape == (n, len(KEYS) * 32) and want.any()
        assert got.tobytes() == want.tobytes()
        assert got.tobytes() != clean.tobytes(), "the reverberation changed nothing: the comparison shows nothing"
        got2 = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, reverb=(rv, rooms),
                                            corrupt=(mixer, plan))
        want2 = pipeline.features_from_audio(both, fe, net, KEYS, batch=2, streams=streams)
        assert got2.tobytes() == want2.tobytes() and got2.tobytes() != got.tobytes()
    # HotPath itself: one step with reverb=, then with both
    hp = pipeline.HotPath(fe, net, KEYS, streams=1, reverb=rv, mixer=mixer)
    plain = pipeline.HotPath(fe, net, KEYS, streams=1)
    a, st = hp.submit(audio, reverb=rooms)
    st.synchronize()
    b, st = plain.submit(wet)
    st.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    a, st = hp.submit(audio, reverb=rooms, mix=plan)
    st.synchronize()
    b, st = plain.submit(both)
    st.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="reverberator"):
        plain.submit(audio, reverb=rooms)


@pytest.mark.parametrize("rate", [16000, 48000], ids=["16k", "resampler-in-front"])
def test_audio_stream_bank_with_a_reverb_stream(torch_cuda, rate):
    """`AudioStreamBank(reverb=...)` fed in uneven pushes against a bank without one fed the restated streams."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend, pipeline
    F, n, hops, S, K, H = 8, 2, 60, 8, 3, 1
    bank, lengths, rv = _rooms()
    fe = frontend.SpikeFrontEnd(F, "gammatone")
    db_range = fe.db_range(torch.from_numpy(_noise(1, 16000, 11, 0.2)).cuda())
    net = _small_net(F)
    per = rate // 100                                                 # device-rate samples per hop of 160
    if rate == 16000:
        x, resampler = _noise(n, hops * 160, 71, 0.2), None
        samples = x
    else:
        x = (np.random.default_rng(72).standard_normal((n, hops * per)) * 6000).astype(np.int16)
        samples = frontend.ResampleStream(rate, n).push(x)[0].cpu().numpy()
        resampler = frontend.ResampleStream(rate, n)
    rows = [1, 0]
    wet = np.stack([RR.stream_cut(samples[b], bank, [hops * 160], lengths, rows[b])[0] for b in range(n)])
    rs = frontend.ReverbStream(rv, n)
    rs.set([0, 1], rows)
    plain = pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, S, K, H, KEYS)
    with pytest.raises(ValueError, match="reverberator serves"):
        pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, S, K, H, KEYS,
                                 reverb=frontend.ReverbStream(rv, n + 1))
    wetbank = pipeline.AudioStreamBank(frontend.GammatoneStream(F, n, db_range), net, S, K, H, KEYS, resampler=resampler,
                                       reverb=rs)
    done, seen_rows = np.zeros(n, dtype=np.int64), False
    for new in [(3, 17), (0, 2), (27, 1), (30, 40)]:
        new = np.asarray(new, dtype=np.int64)
        top = int(new.max())
        chunk = np.full((n, top * per), 7, dtype=x.dtype)
        fed = np.full((n, top * 160), 7.0, dtype=np.float32)
        for b in range(n):
            chunk[b, :new[b] * per] = x[b, done[b] * per:(done[b] + new[b]) * per]
            fed[b, :new[b] * 160] = wet[b, done[b] * 160:(done[b] + new[b]) * 160]
        got, cnt = wetbank.push(chunk, new)
        want, want_cnt = plain.push(fed, new)
        assert cnt.tolist() == want_cnt.tolist()
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        seen_rows = seen_rows or bool(got.any())
        done += new
    assert done.tolist() == [hops] * n and seen_rows
    wetbank.reset([1])
    assert not rs.state[1].any() and rs.state[0].any()


def test_create_dataset_with_the_reverb_flags(torch_cuda, tmp_path):
    """File 1 written with `reverb` holds the rasters of the restated clips; together with `augment`, those of the restated
    reverberation followed by the restated mix; without either, today's rasters."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend, synth
    words = ["a", "b", "c"]
    wet_file, both_file, clean_file = (str(tmp_path / f"{k}.npz") for k in ("wet", "both", "clean"))
    room = dict(rir_dir="synthetic", prob=0.7, max_ms=20.0, seed=7)
    augment = dict(noise_dir="synthetic", snr_db=(0.0, 10.0), time_shift_ms=100.0, level_db=(-6.0, 0.0), seed=7)
    cd.create_dataset(8, "gammatone", commands=words, synthetic_per_class=2, output_file=wet_file, reverb=room)
    cd.create_dataset(8, "gammatone", commands=words, synthetic_per_class=2, output_file=both_file, reverb=room, augment=augment)
    cd.create_dataset(8, "gammatone", commands=words, synthetic_per_class=2, output_file=clean_file)
    bank, lengths, rooms = cd.reverberation(room, 6)
    assert bank.shape == (cd.SYNTHETIC_RIR_ROWS, 320) and (rooms.rows < 0).any() and (rooms.rows >= 0).any()
    audio = synth.class_chirps(np.repeat(np.arange(3), 2), seed=1234)
    wet = RR.reverb(audio, bank, lengths, rooms.rows)
    noise, plan = cd.corruption(augment, 6)
    both, _, _ = M.mix(wet, noise, 10.0 ** (-plan.snr_db / 10.0), plan.rows, plan.offsets, plan.shift, plan.scale)
    fe = frontend.SpikeFrontEnd(8, "gammatone")
    got, got_both, plain = (np.load(f)["X_spikes"] for f in (wet_file, both_file, clean_file))
    assert got.tobytes() == fe.encode(wet).cpu().numpy().tobytes()
    assert got_both.tobytes() == fe.encode(both).cpu().numpy().tobytes()
    assert plain.tobytes() == fe.encode(audio).cpu().numpy().tobytes() and got.tobytes() != plain.tobytes()
