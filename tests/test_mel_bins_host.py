"""The per-bin mel tests (SPEC.md 1.5), the part that needs no GPU: it keeps the conditions of tests/test_gpu_mel_bins.py
honest.  The float64 DFT that test uses as its reference is anchored to `np.fft.rfft`; the tolerance it asserts is shown to
be one that correct code meets (the oracle's own complex64 route stays inside it); the float32 restatement of the projection
is anchored to a float64 dot product; and the designed inputs are what their names say."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mel_restatement as MR  # noqa: E402


def _report(what, rel, families):
    for family in sorted(set(f.split()[0] for f in families)):
        rows = [i for i, f in enumerate(families) if f.split()[0] == family]
        if np.isfinite(rel[rows]).any():
            print(f"{what}, {family}: {np.nanmax(rel[rows]):.3g}")


@pytest.mark.parametrize("n_samples,hop", MR.SHAPES)
def test_the_direct_dft_agrees_with_rfft(n_samples, hop):
    """|X| of `dft_power64` against np.fft.rfft on every designed frame, within e / 4 (e: the bound on the float64
    transform's error that the GPU test's tolerance carries; measured e / 8 or better)."""
    frames = MR.designed_frames(n_samples, hop)
    p_ref, e = MR.reference(n_samples, hop)
    assert p_ref.shape == frames.shape[:2] + (MR.N_BINS,) and p_ref.dtype == np.float64 and e.shape == frames.shape[:2]
    mag = np.abs(np.fft.rfft(MR.windowed(frames), axis=-1))
    err = np.abs(np.sqrt(p_ref) - mag)
    live = e > 0
    worst = float((err[live] / e[live][:, None]).max())
    print(f"({n_samples}, {hop}): max | |X|_dft - |X|_rfft | = {worst:.3g} e")
    assert (err <= e[..., None] / 4).all(), worst
    assert not p_ref[~live].any()                                       # an empty frame: exactly zero


@pytest.mark.parametrize("n_samples,hop", MR.SHAPES)
def test_the_oracle_route_meets_the_per_bin_bound_with_one_ulp(n_samples, hop):
    """`oracle.ref_numpy.stft_power` (float64 FFT, complex64 storage, np.abs, ** 2 in float32: librosa's route, the one the
    kernel follows) stays inside `bin_tolerance` with h = 1 on every designed frame: correct code can meet the bound the
    GPU test asserts (there with the h its math library documents).  Measured worst |P - P_ref| / P_ref: 3.3 x 2^-23 (bound 3.5)."""
    from oracle import ref_numpy as O
    clips, families, _ = MR.designed_clips(n_samples, hop)
    p_ref, e = MR.reference(n_samples, hop)
    got = np.stack([O.stft_power(c, hop=hop).T for c in clips])
    assert got.dtype == np.float32 and got.shape == p_ref.shape
    err = np.abs(got.astype(np.float64) - p_ref)
    tol = MR.bin_tolerance(p_ref, e, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(p_ref * 2.0 ** -23 > 2.0 * np.sqrt(p_ref) * e[..., None] + (e * e)[..., None], err / p_ref, np.nan)
    _report(f"({n_samples}, {hop}) oracle route, worst relative deviation in units of 2^-23", rel * 2.0 ** 23, families)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    assert not got[families.index("zero")].any()


def test_the_designed_clips_are_what_they_claim():
    for n_samples, hop in MR.SHAPES:
        clips, families, impulses = MR.designed_clips(n_samples, hop)
        frames = MR.designed_frames(n_samples, hop)
        p_ref, e = MR.reference(n_samples, hop)
        assert clips.dtype == np.float32 and clips.shape == (len(families), n_samples)
        assert frames.shape == (len(families), 1 + n_samples // hop, MR.N_FFT)
        assert families.count("tone") == len(MR.TONE_BINS) == 18 and families.count("zero") == 1
        assert [f for f in families if f.startswith("noise")] == ["noise 0.1", "noise 0.0001", "noise 1000"]
        # an impulse: one sample of 0.75 at the named window position of the named frame, and a flat spectrum there --
        # every bin, 0 and 1024 included, has the power (w[n0] * 0.75)^2
        w = MR.hann_periodic()
        for clip, frame, position in impulses:
            assert np.count_nonzero(clips[clip]) == 1 and frames[clip, frame, position] == MR.IMPULSE_LEVEL
            flat = (w[position] * 0.75) ** 2
            assert flat > 1e-12 and np.abs(p_ref[clip, frame] - flat).max() <= 1e-12 * flat
        if (n_samples, hop) == (4096, 1024):
            # the shape with whole frames: all eight positions, each in a frame that lies inside the clip
            assert [p for _, _, p in impulses] == list(MR.IMPULSE_POSITIONS)
            assert all(0 <= t * hop - 1024 and t * hop + 1024 <= n_samples for _, t, _ in impulses)
            # a tone on bin k0 under the periodic Hann window: bins k0 - 1, k0, k0 + 1 live, the others hold what rounding
            # the samples to float32 left, 130 dB below or less (whole frame 2)
            first = families.index("tone")
            for i, k0 in enumerate(MR.TONE_BINS):
                p = p_ref[first + i, 2]
                live = [k for k in (k0 - 1, k0, k0 + 1) if 0 <= k <= 1024]
                dead = np.setdiff1d(np.arange(MR.N_BINS), live)
                assert p[live].min() > 1e4 and p[dead].max() < 1e-9, k0
        else:
            assert impulses and not any(0 <= t * hop - 1024 and t * hop + 1024 <= n_samples
                                        for t in range(1 + n_samples // hop))       # no frame lies inside the clip


def test_the_float32_projection_agrees_with_a_float64_dot_product():
    """`project32` against sum_f row[f] * pw[f] in float64, within (terms + 2) * 2^-24 * sum |row[f] * pw[f]|; an empty
    filter gives +0.0; and no product or sum of the designed projections lies below float32's normal range (a device that
    flushes such values to zero would otherwise differ from NumPy for a reason that is not the kernel's)."""
    bases = MR.designed_bases()
    assert sorted(len(b[1]) for b in bases.values()) == [1, 293, 304]
    seen = set()
    for n_samples, hop in MR.SHAPES:
        p_ref, _ = MR.reference(n_samples, hop)
        pw = np.ascontiguousarray(p_ref[MR.projection_clip(n_samples, hop)].T.astype(np.float32))      # (1025, n_frames)
        assert pw.min() > 1e-12
        for name, (basis, lo, hi) in bases.items():
            got, least = MR.project32(pw, basis, lo, hi, smallest=True)
            assert got.dtype == np.float32 and got.shape == (len(lo), pw.shape[1])
            assert least >= MR.TINY, (name, least)
            for m in range(len(lo)):
                a, b = int(lo[m]), int(hi[m])
                terms = basis[m, a:b].astype(np.float64)[:, None] * pw[a:b].astype(np.float64)
                bound = (b - a + 2) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
                assert (np.abs(got[m].astype(np.float64) - terms.sum(axis=0)) <= bound).all(), (name, m)
                if a == b:
                    assert got[m].tobytes() == bytes(4 * pw.shape[1]), (name, m)       # +0.0, not -0.0
                assert (basis[m, :a] == MR.FILL).all() and (basis[m, b:] == MR.FILL).all()
                w = np.abs(basis[m, a:b])
                assert ((w >= np.float32(2.0 ** -10)) & (w <= 1)).all()
                seen.add((b - a, a % 4, a == 0, b == MR.N_BINS))
            assert (basis[basis != MR.FILL] < 0).any()                      # negative weights are legal through the ABI
    for width in range(MR.MAX_WIDTH + 1):
        assert {r for w, r, _, _ in seen if w == width} == {0, 1, 2, 3}, width
    assert any(w == 1025 for w, *_ in seen) and any(z for *_, z, _ in seen) and any(t for *_, t in seen)
    # the identity basis returns the power values themselves
    basis, lo, hi = MR.identity_basis()
    assert MR.project32(pw, basis, lo, hi).tobytes() == pw.tobytes()


@pytest.mark.parametrize("n_mels", [13, 40, 128, 700])
def test_the_slaney_bases_give_bins_0_and_1024_no_weight(n_mels):
    """Every mel basis the project builds has weight exactly 0.0 at the DC and the Nyquist bin (and at most 6.3e-3 at bin
    1023): a kernel that computed those bins wrongly -- they are the ones with special code in csrc/mel_body.h -- would
    pass every test that goes through such a basis.  This is why tests/test_gpu_mel_bins.py exists: it reads all 1025 bins
    back through a basis of one-bin filters."""
    from lsm_speech_classifier_amd import mel
    from oracle import ref_numpy as O
    basis, lo, hi = mel.mel_basis(16000, 2048, n_mels)
    assert basis.shape == (n_mels, 1025) and basis.dtype == np.float32
    assert not basis[:, 0].any() and not basis[:, 1024].any()
    assert lo.min() >= 1 and hi.max() <= 1024
    assert 0 < basis[:, 1023].max() < 7e-3
    ref = O.mel_filterbank(16000, 2048, n_mels)
    assert not ref[:, 0].any() and not ref[:, 1024].any()
