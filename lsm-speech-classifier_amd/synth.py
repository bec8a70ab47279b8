"""Synthetic inputs: no Speech Commands corpus exists on either box.

* ``white_noise``: the roofline-stress input of BASELINE.json configs[4].
* ``class_chirps``: class-structured, speech-like 1 s clips (three amplitude-modulated chirps per
  class + noise) so that accuracy-equality checks have something learnable.
* ``bernoulli_raster``: reservoir-only timing input, uint8 (B, C, T) at a given density.
* ``coloured_noise``: a small noise bank for the mixer (SPEC.md §1.10) where no ``_background_noise_`` folder exists.
* ``room_responses``: a small bank of room impulse responses for the reverberator (SPEC.md §1.11).
"""
from __future__ import annotations

import numpy as np

SAMPLE_RATE = 16000
CLIP_SAMPLES = 16000


def white_noise(n_clips: int, seed: int = 1234, n_samples: int = CLIP_SAMPLES) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_clips, n_samples)) * 0.1).astype(np.float32)


def class_chirps(labels, seed: int = 1234, n_samples: int = CLIP_SAMPLES, noise: float = 0.04) -> np.ndarray:
    """One speech-like clip per entry of ``labels``: a harmonic source (pitch glide) shaped by
    three formant resonances whose start/end frequencies, onset and duration are fixed by the
    class; the clip index jitters them a little and adds ``noise``-sigma background noise (0.04: about 10 dB under the
    loudest 10 ms bin; 0.001 gives the quiet surroundings a silence trimmer can cut, SPEC.md §1.15)."""
    labels = np.asarray(labels, dtype=np.int64)
    t = np.arange(n_samples) / SAMPLE_RATE
    out = np.empty((len(labels), n_samples), dtype=np.float32)
    harm = np.arange(1, 41)[:, None]
    for n, c in enumerate(labels):
        crng = np.random.default_rng(seed + int(c))                 # class template
        f_start = crng.uniform(300.0, 3800.0, size=3)
        f_end = crng.uniform(300.0, 3800.0, size=3)
        onset = crng.uniform(0.05, 0.30)
        dur = crng.uniform(0.45, 0.65)
        pitch0, pitch1 = crng.uniform(100.0, 220.0, size=2)
        srng = np.random.default_rng((seed + 7919) * 1000003 + n)   # per-clip jitter
        on = onset + 0.02 * srng.standard_normal()
        u = np.clip((t - on) / dur, 0.0, 1.0)
        gate = (t >= on) & (t <= on + dur)
        env = (np.sin(np.pi * u) ** 2) * (0.6 + 0.4 * np.sin(2 * np.pi * 4.0 * t + c)) * gate
        pitch = (pitch0 + (pitch1 - pitch0) * u) * (1 + 0.02 * srng.standard_normal())
        phase = 2 * np.pi * np.cumsum(pitch) / SAMPLE_RATE
        hf = harm * pitch[None, :]
        gain = np.zeros_like(hf)
        for j in range(3):
            fc = (f_start[j] + (f_end[j] - f_start[j]) * u) * (1 + 0.03 * srng.standard_normal())
            gain += np.exp(-0.5 * ((hf - fc[None, :]) / 500.0) ** 2)
        gain *= hf < 0.45 * SAMPLE_RATE
        x = (gain * np.sin(harm * phase[None, :])).sum(axis=0) * env
        x *= 0.5 / max(1e-9, np.abs(x).max())
        x += noise * srng.standard_normal(n_samples)
        out[n] = x.astype(np.float32)
    return out


def coloured_noise(n_rows: int, n_samples: int = 4 * CLIP_SAMPLES, seed: int = 1234) -> np.ndarray:
    """A noise bank (n_rows, n_samples) float32 with a peak of 0.5: white noise shaped in the frequency domain to a power
    spectrum of 1 / f^r for row r -- white, pink, brown, ... -- so that the rows differ the way the hum, hiss and rumble of
    a background-noise folder do."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(n_samples)
    f[0] = f[1] if n_samples > 1 else 1.0
    out = np.empty((n_rows, n_samples), dtype=np.float32)
    for r in range(n_rows):
        x = np.fft.irfft(np.fft.rfft(rng.standard_normal(n_samples)) * f ** (-0.5 * r), n=n_samples)
        out[r] = (x * (0.5 / max(1e-30, np.abs(x).max()))).astype(np.float32)
    return out


REVERB_TAIL_GAIN = 0.05                 # the noise tail's amplitude at its start, against the direct path's 1


def room_responses(n_rows: int, rt60=(0.2, 0.8), seed: int = 1234, fs: int = SAMPLE_RATE):
    """A bank of room impulse responses ``(bank (n_rows, K) float32, lengths (n_rows,) int32)``: exponentially decaying
    Gaussian noise behind a direct path of 1 (SPEC.md §1.11).  Row r has the reverberation time ``rt60[0] + (rt60[1] -
    rt60[0]) * r / max(1, n_rows - 1)`` seconds (``rt60`` a number: every row) and ends at its -60 dB point,
    ``len_r = int(rt60_r * fs)`` taps: ``h[0] = 1`` and ``h[k] = 0.05 * g[k] * 10 ** (-3 * k / len_r)`` with ``g`` the row's
    ``len_r`` draws of ``np.random.RandomState(seed).standard_normal``, rows in order; float64 rounded to float32, zeros
    behind a row's end, K the longest row."""
    lo, hi = (float(rt60), float(rt60)) if np.ndim(rt60) == 0 else (float(rt60[0]), float(rt60[1]))
    if n_rows < 1 or not 0 < lo <= hi or int(lo * fs) < 1:
        raise ValueError(f"room_responses needs n_rows >= 1 and 0 < rt60[0] <= rt60[1] with at least one tap, got {n_rows}, {rt60!r}")
    rs = np.random.RandomState(int(seed))
    lengths = np.array([int((lo + (hi - lo) * r / max(1, n_rows - 1)) * fs) for r in range(n_rows)], dtype=np.int32)
    bank = np.zeros((n_rows, int(lengths.max())), dtype=np.float32)
    for r, n in enumerate(lengths):
        h = REVERB_TAIL_GAIN * rs.standard_normal(int(n)) * 10.0 ** (-3.0 * np.arange(int(n), dtype=np.float64) / float(n))
        h[0] = 1.0
        bank[r, :n] = h.astype(np.float32)
    return bank, lengths


def bernoulli_raster(n_clips: int, n_channels: int, n_steps: int = 400, density: float = 0.2,
                     seed: int = 1234) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.random((n_clips, n_channels, n_steps)) < density).astype(np.uint8)
