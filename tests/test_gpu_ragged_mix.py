"""The ragged noise mixer (`lsm_mix_ragged_f32`, `NoiseMixer.mix_ragged`; SPEC.md 1.16, include/lsm_hip_ragged_augment.h).

Eight clips at a row stride of 1001 samples -- odd, so every row starts at another alignment and both the head of the mixed
samples and the head of the zero fill take every length -- with clip_samples -3, 0, 1, 255, 256, 257, 1001 and 1500 (the 256-lane
structure of P has its edges at 255 / 256 / 257).  Each launch is compared byte for byte with the NumPy restatement
(tests/ragged_augment_restatement.py: tests/mix_restatement.py on the clip alone) and with `lsm_mix_f32` on the clip alone at
n_samples = n_b.  The audio rows hold NaN from n_b on and `out` is pre-filled, so a kernel that reads behind a clip or leaves
the rest of a row unwritten fails.  The shifts 0, +5, -5, +n_b, -n_b, +2000, -2000, 0 are rotated through the clips, so that
every clip meets every shift (at its own place in the list a clip of n_b samples under a shift of +-n_b or beyond is all zeros)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_augment_restatement as RA  # noqa: E402

pytestmark = pytest.mark.gpu

STRIDE = 1001
CLIP_SAMPLES = [-3, 0, 1, 255, 256, 257, 1001, 1500]
N_B = [0, 0, 1, 255, 256, 257, 1001, 1001]
SENTINEL = np.float32(7.5)
CLEAN, ZERO_ROW = 3, 2                      # the clip with ratio = 0, the clip whose noise row is all zeros
BANKS = {"short-37": (3, 37), "long-4099": (2, 4099)}
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _inputs(bank):
    """Audio (clean, and with NaN behind every clip), the bank (its last row zeros) and the per-clip arrays of one bank."""
    if bank not in _CACHE:
        M, L = BANKS[bank]
        rng = np.random.default_rng(L)
        audio = (rng.standard_normal((8, STRIDE)) * 0.2).astype(np.float32)
        dirty = audio.copy()
        for b, n in enumerate(N_B):
            dirty[b, n:] = np.nan
        noise = (rng.standard_normal((M, L)) * 0.05).astype(np.float32)
        noise[M - 1] = 0.0
        rows = rng.integers(0, M - 1, 8).astype(np.int32)
        rows[ZERO_ROW] = M - 1
        rows[5], rows[6] = -4, M + 3                                # clamped to row 0, and to the last row: zeros too
        ratio = 10.0 ** (-rng.uniform(0, 20, 8) / 10.0)
        ratio[CLEAN] = 0.0
        offsets = rng.integers(-3 * L, 3 * L, 8).astype(np.int32)
        scale = rng.uniform(0.5, 2.0, 8).astype(np.float32)
        for a in (audio, dirty, noise):
            a.setflags(write=False)
        _CACHE[bank] = audio, dirty, noise, rows, offsets, scale, ratio
    return _CACHE[bank]


def _shifts(turn):
    """The eight shifts, moved on by ``turn`` clips; "+n" and "-n" are +n_b and -n_b of the clip that gets them."""
    base = [0, 5, -5, "+n", "-n", 2000, -2000, 0]
    own = {"+n": 1, "-n": -1}
    return np.array([own[s] * N_B[b] if s in own else s for b, s in ((b, base[(b + turn) % 8]) for b in range(8))], dtype=np.int32)


def _launch(torch, name, audio, lengths, noise, rows, offsets, shift, scale, ratio):
    """One call of lsm_mix_f32 / lsm_mix_ragged_f32 through the C ABI into pre-filled outputs -> (out, gain, powers) on the host."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    B, n = audio.shape
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (audio, noise, rows, offsets, shift, scale, ratio)]
    out = torch.full((B, n), float(SENTINEL), dtype=torch.float32, device="cuda")
    gain = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    powers = torch.full((B, 2), -1.0, dtype=torch.float64, device="cuda")
    head = [_p(dev[0]), B, n]
    if lengths is not None:
        ln = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda()
        head.append(_p(ln))
    rc = getattr(lib, name)(*head, _p(dev[1]), noise.shape[0], noise.shape[1], *[_p(d) for d in dev[2:]], _p(out), _p(gain),
                            _p(powers), None)
    assert rc == 0, lib.lsm_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy(), gain.cpu().numpy(), powers.cpu().numpy()


@pytest.mark.parametrize("bank", list(BANKS))
def test_every_clip_equals_the_restatement_and_the_unragged_mixer_on_it_alone(torch_cuda, bank):
    torch = torch_cuda
    audio, dirty, noise, rows, offsets, scale, ratio = _inputs(bank)
    assert noise.shape[1] < 256 or noise.shape[1] > STRIDE
    noisy_rows = 0
    for turn in range(8):
        shift = _shifts(turn)
        got, gain, powers = _launch(torch, "lsm_mix_ragged_f32", dirty, CLIP_SAMPLES, noise, rows, offsets, shift, scale, ratio)
        want, want_g, want_p = RA.mix_ragged(audio, CLIP_SAMPLES, noise, ratio, rows, offsets, shift, scale)
        for b, n in enumerate(N_B):
            assert not got[b, n:].view(np.uint32).any(), f"turn {turn} clip {b}: the row behind its {n} samples is not +0.0"
            assert got[b, :n].tobytes() == want[b, :n].tobytes(), f"turn {turn} clip {b}: samples against the restatement"
            assert gain[b].tobytes() == want_g[b].tobytes() and powers[b].tobytes() == want_p[b].tobytes(), (turn, b)
            if n == 0:
                assert gain[b] == 0.0 and not powers[b].view(np.uint64).any()
                continue
            one = slice(b, b + 1)
            alone, g1, p1 = _launch(torch, "lsm_mix_f32", np.ascontiguousarray(audio[one, :n]), None, noise, rows[one], offsets[one],
                                    shift[one], scale[one], ratio[one])
            assert got[b, :n].tobytes() == alone[0].tobytes(), f"turn {turn} clip {b} ({n} samples): against lsm_mix_f32 alone"
            assert gain[b].tobytes() == g1[0].tobytes() and powers[b].tobytes() == p1[0].tobytes(), (turn, b)
        assert gain[CLEAN] == 0.0 and gain[ZERO_ROW] == 0.0 and gain[6] == 0.0 and powers[ZERO_ROW, 1] == 0.0
        noisy_rows += int((gain > 0).sum())
        assert not np.isnan(got).any() and not (got == SENTINEL).any()
    assert noisy_rows >= 12, "hardly a clip got noise: the comparison shows little"


def test_full_lengths_give_the_unragged_bytes(torch_cuda):
    torch = torch_cuda
    audio, _, noise, rows, offsets, scale, ratio = _inputs("long-4099")
    shift = np.array([0, 5, -5, 1001, -1001, 300, -2000, 17], dtype=np.int32)
    want = _launch(torch, "lsm_mix_f32", audio, None, noise, rows, offsets, shift, scale, ratio)
    for lengths in ([STRIDE] * 8, [STRIDE + 1, 2 ** 31 - 1] * 4):
        got = _launch(torch, "lsm_mix_ragged_f32", audio, lengths, noise, rows, offsets, shift, scale, ratio)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
    # by construction: clip 2 has the zero noise row, 3 is clean, 4 and 6 are shifted out of their rows (6 has a zero row too)
    assert np.flatnonzero(want[1] > 0).tolist() == [0, 1, 5, 7]


def test_mix_ragged_of_the_python_layer(torch_cuda):
    """`NoiseMixer.mix_ragged` with host lengths, with a device tensor (never read back: wild values are clamped) and into a
    caller's buffer gives the ABI's bytes; `mix_plan`'s shift, drawn for the stride, is clamped to the clip by the kernel."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    audio, dirty, noise, rows, offsets, scale, ratio = _inputs("short-37")
    mixer = frontend.NoiseMixer(noise)
    plan = frontend.mix_plan(8, noise.shape[0], noise.shape[1], (0.0, 20.0), max_shift=600, seed=5)
    assert (np.abs(plan.shift) > 257).any()
    q = frontend.snr_ratio(plan.snr_db, 8)
    want = RA.mix_ragged(audio, CLIP_SAMPLES, noise, q, plan.rows, plan.offsets, plan.shift, plan.scale)[0]
    x = torch.from_numpy(dirty).cuda()
    got = mixer.mix_ragged(x, N_B, plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale)
    wild = torch.tensor(CLIP_SAMPLES, dtype=torch.int32, device="cuda")
    out = torch.full((8, STRIDE), float(SENTINEL), dtype=torch.float32, device="cuda")
    got2 = mixer.mix_ragged(x, wild, plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale, out=out)
    torch.cuda.synchronize()
    assert got2 is out and got.cpu().numpy().tobytes() == want.tobytes() and torch.equal(got, got2)
    with pytest.raises(ValueError, match="lengths"):
        mixer.mix_ragged(x, N_B[:7], plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale)
    with pytest.raises(ValueError, match="out must not be audio"):
        mixer.mix_ragged(x, N_B, plan.snr_db, plan.rows, plan.offsets, plan.shift, plan.scale, out=x)
