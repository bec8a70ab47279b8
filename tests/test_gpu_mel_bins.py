"""The mel kernels bin by bin (SPEC.md 1.5; `lsm_mel_power_f32`, `lsm_mel_stream_f32`, one device function: csrc/mel_body.h).

Every mel basis the project builds gives bins 0 and 1024 the weight 0.0 (tests/test_mel_bins_host.py), so no test that goes
through such a basis sees them -- and they are the bins with code of their own (the seventeenth row of lane 0, the wrapped
partner index, W_32^16, the store of pw[1024]).  `basis`, `lo` and `hi` are the caller's device arrays: a basis of 1025
one-bin filters makes the kernel return its float32 power spectrum itself, which is compared here, bin by bin, with a
float64 DFT (tests/mel_restatement.py) -- no tolerance tied to the clip's loudest value.  With that spectrum known, designed
bases (every width 0..72 at every lo % 4, 1025, negative weights, 1e30 outside [lo, hi)) pin the projection byte for byte to
its float32 restatement, and the streamed kernel must return the batch kernel's bins."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mel_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu

# hypotf's error in ulps, the h of mel_restatement.bin_tolerance.  The ROCm installation documents no bound for HIP's hypotf
# (its math API reference is not part of it), so this is OpenCL's: OpenCL C specification, "Relative Error as ULPs", hypot
# <= 4 ulp -- ROCm's device library (ocml) serves both languages.
HYPOT_ULPS = 4
CANARY = 0x7FC0BEEF                      # a NaN with a payload: behind every output buffer, and in it before the launch
GUARD = 1024
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _stft_tables(torch):
    """The window and twiddle tables the package hands the kernels (they are the caller's, like the basis)."""
    if "tables" not in _CACHE:
        from lsm_speech_classifier_amd import mel
        _CACHE["tables"] = tuple(_dev(torch, a) for a in mel.stft_tables())
    return _CACHE["tables"]


def _canaries(torch, n):
    return torch.full((n + GUARD,), CANARY, dtype=torch.int32, device="cuda")


def _mel_power(torch, clips, hop, basis, lo, hi):
    """`lsm_mel_power_f32` through ctypes on caller-made tables -> float32 (B, n_mels, n_frames), read from a buffer that
    was all canaries: every element written, none behind the buffer touched."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    B, n = clips.shape
    T, M = MR.n_frames_of(n, hop), len(lo)
    window, twiddle = _stft_tables(torch)
    audio, basis_d, lo_d, hi_d = (_dev(torch, a) for a in (clips, basis, lo, hi))
    assert basis_d.dtype == torch.float32 and lo_d.dtype == hi_d.dtype == torch.int32 and audio.dtype == torch.float32
    assert ((0 <= lo) & (lo <= hi) & (hi <= MR.N_BINS)).all()
    out = _canaries(torch, B * M * T)
    _lib.check(lib.lsm_mel_power_f32(_ptr(audio), B, n, MR.N_FFT, hop, T, _ptr(window), _ptr(twiddle), _ptr(basis_d),
                                     _ptr(lo_d), _ptr(hi_d), M, _ptr(out), torch.cuda.current_stream().cuda_stream),
               "lsm_mel_power_f32")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[B * M * T:] == CANARY).all(), "the NaN canary behind the output buffer was overwritten"
    assert not (host[:B * M * T] == CANARY).any(), "an element of the output buffer was not written"
    got = host[:B * M * T].view(np.float32).reshape(B, M, T)
    assert got.dtype == np.float32 and got.shape == (B, M, T)
    return got


def _bins(torch, n_samples, hop):
    """The identity run of a shape's designed clips (cached): float32 (B, 1025, n_frames), the kernel's power spectrum."""
    key = ("bins", n_samples, hop)
    if key not in _CACHE:
        _CACHE[key] = _mel_power(torch, MR.designed_clips(n_samples, hop)[0], hop, *MR.identity_basis())
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _check_bins(got, p_ref, e, names, what):
    """``got`` (B, 1025, T) float32 against ``p_ref`` (B, T, 1025) float64 per bin; prints, per family of clips, the worst
    |P - P_ref| / P_ref over the bins where the relative term of the bound is the larger one."""
    ref = p_ref.transpose(0, 2, 1)
    rel_term = (1.5 + 2.0 * HYPOT_ULPS) * 2.0 ** -23 * ref
    tol = MR.bin_tolerance(p_ref, e, HYPOT_ULPS).transpose(0, 2, 1)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where((ref > 0) & (rel_term > tol - rel_term), err / ref, np.nan)
    for family in sorted(set(n.split()[0] for n in names)):
        rows = [i for i, n in enumerate(names) if n.split()[0] == family]
        if np.isfinite(rel[rows]).any():
            print(f"{what}, {family}: worst |P - P_ref| / P_ref = {np.nanmax(rel[rows]) * 2.0 ** 23:.3f} x 2^-23 "
                  f"over {int(np.isfinite(rel[rows]).sum())} bins")
    bad = ~(err <= tol)                                     # a NaN is bad; measured 3.47 x 2^-23 at the worst (MEASURED below)
    if bad.any():
        b, k, t = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} values outside the bound, in bins {np.unique(np.nonzero(bad)[1])[:12]}"
                             f"; first: clip {b} ({names[b]}), bin {k}, frame {t}: {got[b, k, t]!r} against {ref[b, k, t]!r}, "
                             f"bound {tol[b, k, t]:.3e}")


@pytest.mark.parametrize("n_samples,hop", MR.SHAPES)
def test_every_bin_equals_the_float64_dft(torch_cuda, n_samples, hop):
    """All 1025 bins of every frame of the designed clips (impulses at eight window positions, tones beside every pass
    stride, noise at three levels, silence) against the direct float64 DFT:
    |P - P_ref| <= (1.5 + 2 h) 2^-23 P_ref + 2 sqrt(P_ref) e + e^2, h = 4, e = 64 * 2^-53 * sum |w x| (mel_restatement.
    bin_tolerance; test_mel_bins_host.py shows the oracle's route inside it with h = 1).
    Measured worst |P - P_ref| / P_ref, in units of 2^-23 (bound 9.5): see MEASURED below."""
    clips, names, impulses = MR.designed_clips(n_samples, hop)
    got = _bins(torch_cuda, n_samples, hop)
    p_ref, e = MR.reference(n_samples, hop)
    assert got.dtype == np.float32 and got.shape == (len(clips), MR.N_BINS, MR.n_frames_of(n_samples, hop))
    _check_bins(got, p_ref, e, names, f"({n_samples}, {hop})")
    # silence: +0.0 in every bin, not -0.0 and not a small number
    assert got[names.index("zero")].tobytes() == bytes(4 * MR.N_BINS * got.shape[2])
    # an impulse at window position n0: the same power (w[n0] * 0.75)^2 in every bin, 0 and 1024 included
    w = MR.hann_periodic()
    for clip, frame, position in impulses:
        flat = (w[position] * 0.75) ** 2
        dev = np.abs(got[clip, :, frame].astype(np.float64) - flat).max() / flat
        assert dev <= (1.5 + 2.0 * HYPOT_ULPS) * 2.0 ** -23 + 1e-12, (position, dev)


# MEASURED on an MI355X: worst |P - P_ref| / P_ref per family of clips, in units of 2^-23, over the bins where the relative
# term of the bound is the larger one; the bound is 9.5 (h = 4).
#   shape (n_samples, hop)   impulses   tones   noise
#   (4096, 1024)             2.09       2.74    2.87
#   (1500, 333)              3.07       3.02    3.08
#   (333, 33)                2.09       3.47    2.70
#   streams, hop 160         -          2.58    2.88
# (the oracle's NumPy route on the same frames: 3.3, tests/test_mel_bins_host.py)


@pytest.mark.parametrize("n_samples,hop", MR.SHAPES)
def test_the_projection_equals_its_float32_restatement_byte_for_byte(torch_cuda, n_samples, hop):
    """The noise clip's power spectrum, as the identity run returned it, through the designed bases: 293 filters (the last
    group of sixteen holds five), 304 (whole groups) and one; widths 0..72 at every lo % 4 and 1025 (the eight-term loop,
    the four-term block, the single-term tail, and lanes with nothing to add); lo = 0 and hi = 1025; weights of both signs;
    1e30 outside [lo, hi).  Equal to mel_restatement.project32 in every byte; an empty filter gives +0.0."""
    clip = MR.projection_clip(n_samples, hop)
    pw = _bins(torch_cuda, n_samples, hop)[clip]                        # (1025, n_frames), the kernel's own float32 values
    audio = MR.designed_clips(n_samples, hop)[0][clip:clip + 1]
    for name, (basis, lo, hi) in MR.designed_bases().items():
        want, least = MR.project32(pw, basis, lo, hi, smallest=True)
        assert least >= MR.TINY, (name, least)                          # nothing below the normal range (see the host test)
        got = _mel_power(torch_cuda, audio, hop, basis, lo, hi)[0]
        assert got.shape == want.shape == (len(lo), pw.shape[1])
        differ = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not differ.any(), (f"{name}: filters {np.nonzero(differ)[0][:12]} differ, (lo, hi) = "
                                  f"{[(int(lo[m]), int(hi[m])) for m in np.nonzero(differ)[0][:12]]}")
        assert np.abs(got).max() < 1e9, f"{name}: a weight outside [lo, hi) reached the output"
        empty = np.nonzero(lo == hi)[0]
        assert got[empty].tobytes() == bytes(4 * len(empty) * pw.shape[1])


def test_the_streamed_kernel_returns_the_batch_kernels_bins(torch_cuda):
    """`lsm_mel_stream_f32` with the identity basis, hop 160, two streams pushed in uneven pieces, `power_out` requested:
    its columns equal `lsm_mel_power_f32`'s frames of the same samples byte for byte in all 1025 bins (test_gpu_mel_streams.py
    asserts this for Slaney bases, which cannot see bins 0 and 1024), and those frames meet the per-bin bound."""
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    hop, n, F = 160, 2, MR.N_BINS
    plan = [(3, 0), (7, 9), (1, 10), (9, 1)]                            # hops per push and stream: 20 each, 6 of latency
    hops_total, Lg = 20, 7
    complete = lambda h: max(0, h - Lg + 1)
    rng = np.random.default_rng(160)
    t = np.arange(hops_total * hop)
    audio = np.stack([rng.standard_normal(len(t)) * 0.1,
                      0.5 * np.cos(np.pi * t + 0.3) + 0.01 * rng.standard_normal(len(t))]).astype(np.float32)
    basis, lo, hi = (_dev(torch, a) for a in MR.identity_basis())
    window, twiddle = _stft_tables(torch)
    on, off = np.array([0.5], dtype=np.float32), np.array([0.4], dtype=np.float32)
    state_bytes = int(lib.lsm_mel_stream_state_bytes(F, MR.N_FFT, hop))
    assert state_bytes > 0
    state = torch.zeros((n, state_bytes), dtype=torch.uint8, device="cuda")
    seen, columns = [0, 0], [[], []]
    for push in plan:
        H = max(push)
        chunk = np.full((n, H * hop), 7.0, dtype=np.float32)            # behind a stream's hops: nobody may read it
        for b in range(n):
            chunk[b, :push[b] * hop] = audio[b, seen[b] * hop:(seen[b] + push[b]) * hop]
        chunk_d, hops_d = _dev(torch, chunk), _dev(torch, np.array(push, dtype=np.int32))
        raster = torch.zeros((n, F, H), dtype=torch.uint8, device="cuda")
        power = _canaries(torch, n * F * H)
        ws = torch.empty((max(int(lib.lsm_mel_stream_workspace(n, F, H)), 256),), dtype=torch.uint8, device="cuda")
        _lib.check(lib.lsm_mel_stream_f32(
            _ptr(chunk_d), n, H, MR.N_FFT, hop, _ptr(window), _ptr(twiddle), _ptr(basis), _ptr(lo), _ptr(hi), F,
            _ptr(hops_d), -60.0, 0.0, C.c_void_p(on.ctypes.data), C.c_void_p(off.ctypes.data), 1, 1, _ptr(state),
            _ptr(state), _ptr(raster), _ptr(power), None, _ptr(ws), int(ws.numel()),
            torch.cuda.current_stream().cuda_stream), "lsm_mel_stream_f32")
        torch.cuda.synchronize()
        host = power.cpu().numpy()
        assert (host[n * F * H:] == CANARY).all(), "the NaN canary behind power_out was overwritten"
        host = host[:n * F * H].reshape(n, F, H)
        for b in range(n):
            cols = complete(seen[b] + push[b]) - complete(seen[b])
            assert (host[b, :, cols:] == CANARY).all() and not (host[b, :, :cols] == CANARY).any(), (push, b)
            columns[b].append(host[b, :, :cols].view(np.float32))
            seen[b] += push[b]
    streamed = np.stack([np.concatenate(c, axis=1) for c in columns])
    n_cols = complete(hops_total)
    assert seen == [hops_total] * n and streamed.shape == (n, F, n_cols) and n_cols == 14
    batch = _mel_power(torch, audio, hop, *MR.identity_basis())
    assert batch.shape == (n, F, hops_total + 1)
    assert streamed.tobytes() == np.ascontiguousarray(batch[:, :, :n_cols]).tobytes()
    assert streamed[:, 0].min() > 0 and streamed[:, 1024].min() > 0     # the DC and the Nyquist bin are live in both streams
    frames = np.stack([MR.frames_of(a, hop)[:n_cols] for a in audio])
    _check_bins(streamed, MR.dft_power64(frames), MR.transform_error(frames), ["noise", "tone"], "streams, hop 160")
