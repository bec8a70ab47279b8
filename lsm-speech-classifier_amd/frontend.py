"""Host mirror of the reference's front end (/root/reference/create_dataset.py:39-104) over the
HIP kernels: same function names, argument meaning and defaults; batched variants underneath.

Host code here only builds small parameter tables (filter coefficients, thresholds) and moves
pointers; all per-sample arithmetic runs in liblsm_hip.so.  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction
from math import gcd
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

# create_dataset.py:10-17
SAMPLE_RATE = 16000
DURATION = 1.0
TIME_BINS = 100
SPIKE_THRESHOLDS = [0.70, 0.80, 0.90, 0.95]
HYSTERESIS_GAP = 0.1
REDUNDANCY_FACTOR = 1
# gtgram call at create_dataset.py:51-58
GT_WINDOW_TIME = 0.025
GT_F_MIN = 50

_EAR_Q = 9.26449          # Glasberg & Moore
_MIN_BW = 24.7


def gammatone_filter_table(fs: float, channels: int, f_min: float) -> np.ndarray:
    """(channels, 10) float64 rows [A0, A11, A12, A13, A14, A2, B0, B1, B2, gain], ordered from
    the lowest to the highest centre frequency: Slaney's ERB filterbank design (Apple TR #35) on
    ERB-spaced centre frequencies between f_min and fs/2, as gammatone==1.0.3 computes it for
    gtgram (the package itself is not available; SPEC.md §1.1)."""
    frac = np.arange(1, channels + 1) / channels
    c = _EAR_Q * _MIN_BW
    high = fs / 2
    cf = -c + np.exp(frac * (np.log(f_min + c) - np.log(high + c))) * (high + c)
    cf = cf[::-1].copy()
    T = 1.0 / fs
    B = 1.019 * 2 * np.pi * (cf / _EAR_Q + _MIN_BW)
    arg = 2 * cf * np.pi * T
    ebt = np.exp(B * T)
    vec = np.exp(2j * arg)
    rt_pos, rt_neg = np.sqrt(3 + 2 ** 1.5), np.sqrt(3 - 2 ** 1.5)
    common = -T * np.exp(-(B * T))
    ks = [np.cos(arg) + rt_pos * np.sin(arg), np.cos(arg) - rt_pos * np.sin(arg),
          np.cos(arg) + rt_neg * np.sin(arg), np.cos(arg) - rt_neg * np.sin(arg)]
    gain_arg = np.exp(1j * arg - B * T)
    gain = np.abs((vec - gain_arg * ks[0]) * (vec - gain_arg * ks[1]) * (vec - gain_arg * ks[2])
                  * (vec - gain_arg * ks[3]) * (T * ebt / (-1 / ebt + 1 + vec * (1 - ebt))) ** 4)
    tab = np.empty((channels, 10), dtype=np.float64)
    tab[:, 0] = T
    for q in range(4):
        tab[:, 1 + q] = common * ks[q]
    tab[:, 5] = 0.0
    tab[:, 6] = 1.0
    tab[:, 7] = -2 * np.cos(arg) / ebt
    tab[:, 8] = np.exp(-2 * B * T)
    tab[:, 9] = gain
    return tab


def coef_flags(tab: np.ndarray) -> int:
    """Properties of a coefficient table that let the kernel skip work without changing a bit:
    bit 0: every A2 is exactly zero; bit 1: no gain has an all-ones significand (the one case in
    which the FMA division sequence is not guaranteed to round like a true division); bit 2: A0/B0 is the
    same float64 for every channel (the fused kernel then forms b0*x once for the two channels of a lane)."""
    flags = 0
    if not np.any(tab[:, 5]):
        flags |= 1
    mant = np.ascontiguousarray(tab[:, 9]).view(np.uint64) & np.uint64((1 << 52) - 1)
    if np.all(np.isfinite(tab[:, 9])) and not np.any(mant == np.uint64((1 << 52) - 1)) \
            and np.all(np.abs(tab[:, 9]) > 1e-200) and np.all(np.abs(tab[:, 9]) < 1e200):
        flags |= 2
    b0 = tab[:, 0] / tab[:, 6]
    if np.all(np.isfinite(b0)) and np.all(b0.view(np.uint64) == b0[:1].view(np.uint64)):
        flags |= 4
    return flags


def _round_half_away(x: float) -> int:
    return int(np.sign(x) * np.floor(np.abs(x) + 0.5))


def gtgram_strides(fs: float, window_time: float, hop_time: float, n_samples: int):
    nwin = _round_half_away(window_time * fs)
    hop = _round_half_away(hop_time * fs)
    return nwin, hop, 1 + int(np.floor((n_samples - nwin) / hop))


def threshold_tables(thresholds, gap: float, dtype):
    """ON thresholds sorted descending and the Python-float ``thr - gap`` OFF bounds
    (create_dataset.py:87-89), rounded to the spectrogram dtype the comparison happens in."""
    thr = sorted(thresholds, reverse=True)
    on = np.array([dtype(t) for t in thr], dtype=dtype)
    off = np.array([dtype(t - gap) for t in thr], dtype=dtype)
    return on, off


def _stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dev(t, row: int = 0):
    """The pointer a kernel gets for tensor ``t`` from its row ``row`` on; None (an argument the call leaves out) stays None.
    The package's one definition, with `_host`."""
    if t is None:
        return None
    return C.c_void_p((t[row:] if row else t).data_ptr())


def _host(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _up(a, device):
    """A per-clip host array as a tensor on ``device``, copied on the current stream without waiting; None stays None."""
    return None if a is None else torch.from_numpy(a).to(device, non_blocking=True)


def indexed_device(device=None) -> torch.device:
    """``device`` (None = "cuda") with its index: a tensor's device always carries one, ``torch.device("cuda")`` does not,
    and means whatever device is current when it is used."""
    d = torch.device(device if device is not None else "cuda")
    return d if d.index is not None or d.type != "cuda" else torch.device("cuda", torch.cuda.current_device())


# ---- what a stage's host side is made of ("What a batch stage's host side does") ----------------------------
def _open(device=None):
    """How a stage's constructor opens, once its own arguments are checked: ``(lib, device)`` -- a GPU required first, then
    the library loaded, then the device pinned with its index NOW: later calls may come under another current device."""
    _lib.require_gpu()
    lib = _lib.load()
    return lib, indexed_device(device)


def checked_out(out, shape, device=None, audio=None, reason=None, *, at_least: bool = False, name: str = "out",
                dtype=torch.float32, word=None):
    """A caller-owned output checked and returned: a contiguous ``dtype`` tensor (the refusal says "float32" for torch.float32;
    ``word``: another spelling, which some stream outputs have always had) of ``shape`` -- with ``at_least`` of ``shape[0]``
    rows of ``shape[1]`` columns or more -- on ``device`` (None: any device, for a check made before a device is touched).
    ``reason``: why the stage cannot write over its input -- ``out`` is then refused where it is ``audio`` or starts where
    ``audio`` starts; None: the stage may.  Host code only."""
    shape = tuple(shape)
    if at_least:
        fits = torch.is_tensor(out) and out.ndim == 2 and out.shape[0] == shape[0] and out.shape[1] >= shape[1]
    else:
        fits = torch.is_tensor(out) and tuple(out.shape) == shape
    if not fits or out.dtype != dtype or not out.is_contiguous() or (device is not None and out.device != device):
        want = f"({shape[0]}, >= {shape[1]})" if at_least else f"{shape}"
        word = word or str(dtype).replace("torch.", "")
        raise ValueError(f"{name} must be a contiguous {word} {want} tensor" + ("" if device is None else f" on {device}"))
    if reason is not None and (out is audio or (shape[0] and out.data_ptr() == audio.data_ptr())):
        raise ValueError(f"{name} must not be audio: {reason}")
    return out


def checked_lengths(lengths, n: int, limit: int, device):
    """The valid samples of ``n`` clips as the int32 tensor on ``device`` that a kernel reads.  A device tensor is taken as it
    is -- int32 (n,), never read back: the kernel clamps it.  Host integers (a sequence, an array, a CPU tensor) are checked
    against ``[0, limit]`` with the offenders named and uploaded without waiting.  ``device`` None: checked only, for a caller
    that uploads later (host integers come back as a CPU tensor).  (`NoiseMixer.mix_ragged` keeps a conversion of its own.)"""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (n,):
            raise ValueError(f"lengths must hold {n} int32 values, got {lengths.dtype} {tuple(lengths.shape)}")
        return lengths if device is None else lengths.to(device).contiguous()
    arr = np.asarray(lengths.numpy() if torch.is_tensor(lengths) else lengths)
    if arr.shape != (n,) or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"lengths must be {n} integers, got {arr.dtype} {arr.shape}")
    bad = np.nonzero((arr < 0) | (arr > limit))[0]
    if len(bad):
        raise ValueError(f"lengths {arr[bad].tolist()} of clips {bad.tolist()} outside [0, {limit}]")
    host = torch.from_numpy(arr.astype(np.int32))
    return host if device is None else host.to(device, non_blocking=True)


def checked_n_out(n_out, default: int) -> int:
    """The samples of an output row: ``n_out``, or ``default`` for None; at least 1."""
    n_out = int(default) if n_out is None else int(n_out)
    if n_out < 1:
        raise ValueError(f"n_out must be >= 1, got {n_out}")
    return n_out


def row_chunks(n: int, limit: int):
    """``(r0, k)`` of the launches a batch of ``n`` rows is cut into, ``limit`` rows at the most each: rows ``r0 .. r0 + k - 1``,
    in order, none empty (a launch's row count is a grid dimension)."""
    for r0 in range(0, n, limit):
        yield r0, min(limit, n - r0)


def as_float32(audio) -> torch.Tensor:
    """NumPy array (copied) or tensor -> contiguous float32 tensor, on the device it is on."""
    if isinstance(audio, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    return audio.to(torch.float32).contiguous()


def checked_slots(slots, n_streams: int) -> np.ndarray:
    """The stream slots a ``reset`` names, as an int64 array; refused when one lies outside ``[0, n_streams)``."""
    slots = np.atleast_1d(np.asarray(slots, dtype=np.int64))
    if ((slots < 0) | (slots >= n_streams)).any():
        raise ValueError(f"slots {slots.tolist()} outside [0, {n_streams})")
    return slots


class SpikeFrontEnd:
    """Batched filterbank -> dB -> normalise -> resize -> hysteresis encoder on one GPU."""

    def __init__(self, n_filters: int, filterbank: str = "gammatone", device=None,
                 redundancy: int = REDUNDANCY_FACTOR, thresholds=None, gap: float = HYSTERESIS_GAP,
                 time_bins: int = TIME_BINS, n_samples: int = int(SAMPLE_RATE * DURATION)):
        if filterbank not in ("gammatone", "mel"):
            raise ValueError(f"filterbank must be 'mel' or 'gammatone', got {filterbank!r}")
        if int(n_filters) < 1:
            raise ValueError(f"n_filters must be >= 1, got {n_filters}")
        if filterbank == "gammatone" and int(n_filters) == 1:
            # SPEC.md 1.1: with ONE gammatone channel NumPy sums each 400-sample window pairwise (the fancy-index result
            # (1, 400) is contiguous along the reduced axis), with two or more element by element; the kernels implement
            # the latter.  One filter is refused rather than answered 6e-16 beside the reference.
            raise ValueError("the gammatone branch needs n_filters >= 2: with a single channel the reference's window sums "
                             "take NumPy's pairwise order, which the GPU filterbank does not restate (SPEC.md 1.1); use "
                             "--filterbank mel for one filter")
        self.lib, self.device = _open(device)
        self.n_filters = int(n_filters)
        self.filterbank = filterbank
        self.redundancy = int(redundancy)
        self.thresholds = list(SPIKE_THRESHOLDS if thresholds is None else thresholds)
        self.gap = float(gap)
        self.time_bins = int(time_bins)
        self.n_samples = int(n_samples)
        if filterbank == "gammatone":
            hop_time = self.n_samples / (SAMPLE_RATE * self.time_bins)       # create_dataset.py:50
            self.nwin, self.hop, self.ncols = gtgram_strides(SAMPLE_RATE, GT_WINDOW_TIME, hop_time,
                                                             self.n_samples)
            tab = gammatone_filter_table(SAMPLE_RATE, self.n_filters, GT_F_MIN)
            self.coefs = torch.from_numpy(tab).to(self.device)
            self.coef_flags = coef_flags(tab)
            self.dtype = torch.float64
        else:
            from . import mel as _mel
            self._mel = _mel.MelSpectrogram(self.n_filters, self.n_samples, self.time_bins, self.device)
            self.ncols = self._mel.n_frames
            self.dtype = torch.float32

    @property
    def n_channels(self) -> int:
        return self.n_filters * self.redundancy

    @property
    def n_steps(self) -> int:
        return self.time_bins * len(self.thresholds)

    def _stream(self) -> int:
        """The current stream of THIS front end's device (not of whatever device is current)."""
        return _stream(self.device)

    def workspace_elems(self, n_clips: int) -> int:
        """float64 elements of the fused launch's scratch for a batch of `n_clips` (0 for the mel branch)."""
        if self.filterbank != "gammatone":
            return 0
        return max(int(self.lib.lsm_gammatone_spikes_workspace(int(n_clips), self.n_filters, self.ncols)), 8) // 8

    def will_fuse(self) -> bool:
        """Whether `encode()` takes the one-launch route by default.  ONE decision for `encode()` and for
        `pipeline.HotPath`, which hands its own raster buffers to the fused launch only.  Gammatone: up to 1024 filters
        (`lsm_gammatone_spikes_f64`).  Mel: the one-launch route (`lsm_mel_spikes_f32`, `encode(fused=True)`) exists and
        gives the same rasters, but measured slower than the three split launches at the reference's CPU-runnable shape
        (40 filters, 200 clips: 0.318 against 0.305 ms per step, profiles/r04_mel_one_launch_ab.txt), so it is taken by
        default only with LSM_MEL_ONE_LAUNCH=1.
        LSM_FRONTEND_SPLIT=1: diagnostic switch for same-box A/B runs of the two routes (exp/r03_fused_sweep.sh)."""
        if os.environ.get("LSM_FRONTEND_SPLIT") == "1":
            return False
        if self.filterbank == "mel":
            return (os.environ.get("LSM_MEL_ONE_LAUNCH") == "1"
                    and self._mel.fits_one_launch(self.time_bins, len(self.thresholds)))
        return self.n_filters <= 1024

    def new_workspace(self, n_clips: int) -> torch.Tensor:
        """Scratch of the one-launch route for batches of up to `n_clips` clips, to pass as `encode(workspace=...)`: one per
        stream when launches may overlap (the mel scratch carries per-clip arrival counters and starts zeroed)."""
        if self.filterbank == "mel":
            return self._mel.new_workspace(n_clips)
        return torch.empty((self.workspace_elems(n_clips),), dtype=torch.float64, device=self.device)

    def _raster_for(self, n_clips: int, raster_out) -> torch.Tensor:
        """The uint8 raster (n_clips, C, n_steps) of a launch: the caller's ``raster_out``, checked, or a new one."""
        shape = (n_clips, self.n_channels, self.n_steps)
        if raster_out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if (raster_out.dtype != torch.uint8 or tuple(raster_out.shape) != shape or not raster_out.is_contiguous()
                or raster_out.device != self.device):
            raise ValueError(f"raster_out must be a contiguous uint8 {shape} tensor on {self.device}")
        return raster_out

    def _workspace_for(self, n_clips: int, workspace):
        """The scratch of a fused gammatone launch of ``n_clips`` clips and the bytes the launch needs of it: the caller's
        ``workspace``, checked, or a new one."""
        ws_bytes = int(self.lib.lsm_gammatone_spikes_workspace(n_clips, self.n_filters, self.ncols))
        if workspace is None:
            return torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=self.device), ws_bytes
        if (workspace.dtype != torch.float64 or workspace.numel() * 8 < ws_bytes or not workspace.is_contiguous()
                or workspace.device != self.device):
            raise ValueError(f"workspace must be a contiguous float64 tensor of >= {ws_bytes // 8} elements on {self.device}")
        return workspace, ws_bytes

    @staticmethod
    def _launch_flags(low_latency: bool, share_lds: bool) -> int:
        """`lsm_gammatone_spikes_f64`'s launch_flags: bit 0 the low-latency layout, bit 1 no LDS reservation."""
        return (1 if low_latency else 0) | (2 if share_lds else 0)

    def _audio(self, audio) -> torch.Tensor:
        audio = as_float32(audio).to(self.device)
        if audio.dim() == 1:
            audio = audio[None]
        if audio.shape[1] != self.n_samples:
            raise ValueError(f"clips must have {self.n_samples} samples, got {audio.shape[1]}")
        return audio

    def spectrogram_db(self, audio, want_spec: bool = False):
        """(B, n_samples) float32 -> dB spectrogram (B, F, ncols) in the filterbank's dtype
        (gammatone: float64 20*log10(gtgram+1e-9), un-floored; mel: float32 power_to_db)."""
        audio = self._audio(audio)
        B = audio.shape[0]
        if self.filterbank == "mel":
            with torch.cuda.device(self.device):
                return self._mel.power_db(audio), None
        with torch.cuda.device(self.device):       # launch on THIS device's current stream
            db = torch.empty((B, self.n_filters, self.ncols), dtype=torch.float64, device=self.device)
            spec = torch.empty_like(db) if want_spec else None
            _lib.check(self.lib.lsm_gammatone_spec_f64(
                _dev(audio), B, self.n_samples, _dev(self.coefs), self.n_filters, self.nwin, self.hop, self.ncols, _dev(spec),
                _dev(db), self.coef_flags, self._stream()), "lsm_gammatone_spec_f64")
        return db, spec

    def spikes_from_db(self, db: torch.Tensor, want_norm: bool = False, want_raster: bool = True, mask=None):
        """dB spectrogram -> (uint8 raster (B, C, n_steps), normalised spectrogram or None).  ``mask``: a `MaskPlan` of the
        batch's clips (SPEC.md 1.13): the masked entry point encodes -- and, with ``want_norm``, shows -- the masked
        spectrogram; None makes exactly the unmasked call."""
        B = db.shape[0]
        f64 = db.dtype == torch.float64
        np_dt = np.float64 if f64 else np.float32
        on, off = threshold_tables(self.thresholds, self.gap, np_dt)
        if db.device != indexed_device(self.device):      # pinned by __init__; an instance built without it may still say "cuda"
            raise ValueError(f"spectrogram on {db.device}, front end on {self.device}")
        db = db.contiguous()
        with torch.cuda.device(self.device):
            raster = (torch.empty((B, self.n_channels, self.n_steps), dtype=torch.uint8, device=self.device)
                      if want_raster else None)
            norm = (torch.empty((B, self.n_filters, self.time_bins), dtype=db.dtype, device=self.device)
                    if want_norm else None)
            args = (_dev(db), B, self.n_filters, db.shape[2], self.time_bins,
                    1 if self.filterbank == "gammatone" else 0, _host(on), _host(off), len(on),
                    self.redundancy, _dev(raster), _dev(norm))
            if mask is None:
                fn = self.lib.lsm_spec_to_spikes_f64 if f64 else self.lib.lsm_spec_to_spikes_f32
                _lib.check(fn(*args, self._stream()), "lsm_spec_to_spikes")
            else:
                fm, tm = upload_mask(mask, B, self.n_filters, self.time_bins, self.device)
                fn = self.lib.lsm_spec_to_spikes_masked_f64 if f64 else self.lib.lsm_spec_to_spikes_masked_f32
                _lib.check(fn(*args, _dev(fm), _dev(tm), self._stream()), "lsm_spec_to_spikes_masked")
        return raster, norm

    def encode(self, audio, fused: bool | None = None, low_latency: bool = False,
               raster_out: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
               share_lds: bool = False, mask=None) -> torch.Tensor:
        """audio (B, n_samples) -> uint8 spike raster (B, C, n_steps) on the device.  The gammatone branch is one
        launch (`lsm_gammatone_spikes_f64`); `fused=False` takes the split entry points (identical rasters), which is
        also what the mel branch takes by default (its one-launch route, `fused=True` -> `lsm_mel_spikes_f32`, measured
        slower) and what shapes too large for the one-launch kernels use (`will_fuse()`).  `low_latency`: the
        fused launch in its one-chain layout (twice the waves, each half as long) -- for a batch that meets an idle
        GPU; `pipeline.HotPath` asks for it when none of its front ends is in flight.  `share_lds`: the launch runs
        beside LDS-hungry workgroups of another kernel (the ring-row reservoir kernel, two 64 KB clips per CU): it then
        asks for the 27 KB of LDS it uses instead of reserving half a CU's (the reservation is a placement tool for small
        launches, `lsm_gammatone_spikes_f64` flag bit 1).  `raster_out` / `workspace`
        (fused launch only): caller-owned uint8 (B, C, n_steps) output and scratch from `new_workspace(B)` (gammatone:
        float64, at least `workspace_elems(B)` elements; mel: zero-initialised bytes), so that a steady stream of
        batches makes no allocator call at all.  ``mask``: a `MaskPlan` of the batch's clips (SPEC.md 1.13), applied inside
        the encoder of whichever route is taken (the masked entry points of include/lsm_hip_mask.h); its words are uploaded on
        the current stream; None makes exactly the unmasked calls."""
        if fused is None:
            fused = self.will_fuse()
        if mask is not None:
            checked_mask(mask, 1 if getattr(audio, "ndim", 2) == 1 else len(audio), self.n_filters, self.time_bins)
        if not fused:
            if raster_out is not None or workspace is not None:
                # the split route allocates its own outputs on the current stream: a caller that owns the raster
                # buffer (pipeline.HotPath's rings) must not be handed another tensor silently
                raise ValueError("raster_out / workspace belong to the fused launch; this front end takes the split "
                                 "route (mel branch, > 1024 filters or LSM_FRONTEND_SPLIT=1)")
            db, _ = self.spectrogram_db(audio)
            raster, _ = self.spikes_from_db(db, mask=mask)
            return raster
        audio = self._audio(audio)
        B = audio.shape[0]
        if self.filterbank == "mel":
            if not self._mel.fits_one_launch(self.time_bins, len(self.thresholds)):
                raise ValueError(f"{self.n_filters} mel filters do not fit the one-launch front end; use fused=False")
            on32, off32 = threshold_tables(self.thresholds, self.gap, np.float32)
            with torch.cuda.device(self.device):
                masks = None if mask is None else upload_mask(mask, B, self.n_filters, self.time_bins, self.device)
                return self._mel.spikes(audio, on32, off32, self.time_bins, self.redundancy, raster_out, workspace, masks)
        on, off = threshold_tables(self.thresholds, self.gap, np.float64)
        with torch.cuda.device(self.device):
            raster = self._raster_for(B, raster_out)
            ws, ws_bytes = self._workspace_for(B, workspace)
            args = (_dev(audio), B, self.n_samples, _dev(self.coefs), self.n_filters, self.nwin, self.hop,
                    self.ncols, self.time_bins, _host(on), _host(off), len(on), self.redundancy, _dev(raster),
                    _dev(ws), ws_bytes, self.coef_flags, self._launch_flags(low_latency, share_lds))
            if mask is None:
                _lib.check(self.lib.lsm_gammatone_spikes_f64(*args, self._stream()), "lsm_gammatone_spikes_f64")
            else:
                fm, tm = upload_mask(mask, B, self.n_filters, self.time_bins, self.device)
                _lib.check(self.lib.lsm_gammatone_spikes_masked_f64(*args, _dev(fm), _dev(tm), self._stream()),
                           "lsm_gammatone_spikes_masked_f64")
        return raster

    # ---- ragged batches (SPEC.md §1.14, include/lsm_hip_ragged.h) ---------------------------------------------------------
    def _device_bins(self, bins, n_clips: int) -> torch.Tensor:
        """``bins`` of a ragged batch as the int32 device tensor the kernels read: host values checked
        (`checked_ragged_bins`), a device tensor taken as it is -- never read back, the kernels clamp it."""
        host = checked_ragged_bins(bins, n_clips, self.time_bins)
        if host is None:
            return bins.to(self.device).contiguous()
        return torch.from_numpy(host).to(self.device)

    def _clamped_bins(self, bins_dev: torch.Tensor) -> torch.Tensor:
        """The kernels' clamp of a bin count (0, or 3 .. time_bins), as device arithmetic: what the split routes derive their
        column and frame counts from, so that the launches of one batch agree whatever the tensor holds."""
        t = bins_dev.clamp(0, self.time_bins)
        return torch.where(t < 3, torch.zeros_like(t), t)

    def spikes_from_db_ragged(self, db: torch.Tensor, cols: torch.Tensor, bins: torch.Tensor, want_norm: bool = False,
                              want_raster: bool = True, raster_out: torch.Tensor | None = None, mask=None):
        """`spikes_from_db` for a ragged batch (`lsm_spec_to_spikes_ragged_*`): ``db`` (B, F, ncols) holds clip b's dB values
        in its first ``cols[b]`` columns, ``bins[b]`` is its number of time bins (int32 device tensors).  Returns (raster
        (B, C, n_steps), normalised spectrogram (B, F, time_bins) or None); both are zeros past a clip's bins.  ``mask``: a
        `MaskPlan` whose time bits name the bins of each clip's own length (SPEC.md §1.16, `mask_plan_ragged`): the masked
        ragged entry point; None makes exactly the unmasked call."""
        B = db.shape[0]
        f64 = db.dtype == torch.float64
        on, off = threshold_tables(self.thresholds, self.gap, np.float64 if f64 else np.float32)
        if db.device != indexed_device(self.device):
            raise ValueError(f"spectrogram on {db.device}, front end on {self.device}")
        for name, t in (("cols", cols), ("bins", bins)):
            if (not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != db.device
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 ({B},) tensor on {db.device}")
        db = db.contiguous()
        with torch.cuda.device(self.device):
            raster = raster_out if raster_out is not None else (
                torch.empty((B, self.n_channels, self.n_steps), dtype=torch.uint8, device=self.device) if want_raster else None)
            norm = (torch.empty((B, self.n_filters, self.time_bins), dtype=db.dtype, device=self.device)
                    if want_norm else None)
            args = (_dev(db), B, self.n_filters, db.shape[2], self.time_bins, _dev(cols), _dev(bins),
                    1 if self.filterbank == "gammatone" else 0, _host(on), _host(off), len(on), self.redundancy,
                    _dev(raster), _dev(norm))
            if mask is None:
                fn = self.lib.lsm_spec_to_spikes_ragged_f64 if f64 else self.lib.lsm_spec_to_spikes_ragged_f32
                _lib.check(fn(*args, self._stream()), "lsm_spec_to_spikes_ragged")
            else:
                fm, tm = upload_mask(mask, B, self.n_filters, self.time_bins, self.device)
                fn = self.lib.lsm_spec_to_spikes_ragged_masked_f64 if f64 else self.lib.lsm_spec_to_spikes_ragged_masked_f32
                _lib.check(fn(*args, _dev(fm), _dev(tm), self._stream()), "lsm_spec_to_spikes_ragged_masked")
        return raster, norm

    def encode_ragged(self, audio, bins, fused: bool | None = None, low_latency: bool = False,
                      raster_out: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                      share_lds: bool = False, mask=None):
        """Clips of different lengths in the launches a batch of equal clips takes (SPEC.md §1.14).  ``audio``
        (B, n_samples): clip b is the first ``160 * bins[b]`` samples of its row, and what lies behind them influences
        nothing.  ``bins``: B host integers, each 0 or 3 .. time_bins (checked), or an int32 device tensor (not read: the
        kernels clamp it).  Returns ``(raster, steps)``: the uint8 raster (B, C, n_steps) -- clip b's rows hold, in their
        first ``bins[b] * n_thr`` bytes, what ``SpikeFrontEnd(n_filters, filterbank, n_samples=160 * bins[b],
        time_bins=bins[b])`` encodes for the clip alone, and zeros behind them -- and ``steps``, the int32 device tensor
        ``bins * n_thr`` that ``SNN.run_batch(lengths=...)`` takes, made on the device without a host round trip.
        Needs a front end with ``n_samples == 160 * time_bins`` (`ragged_refusal`).  Gammatone: one launch
        (`lsm_gammatone_spikes_ragged_f64`; ``low_latency``, ``share_lds``, ``raster_out`` and ``workspace`` as `encode`
        takes them), or with ``fused=False`` `lsm_gammatone_spec_f64` on the padded rows and the ragged encoder: the same
        bytes.  Mel: always the split route -- the rows are zeroed from each clip's end on into a staging tensor, then
        `lsm_mel_power_f32`, `lsm_power_to_db_ragged_f32` and the ragged encoder.  ``mask``: a `MaskPlan` of the batch's clips
        at the launch's strides whose time bit j names bin j of clip b's own bins (SPEC.md §1.16, `mask_plan_ragged`), applied
        inside the encoder of whichever route is taken (include/lsm_hip_ragged_augment.h); None makes exactly the unmasked
        calls."""
        why = ragged_refusal(self.n_samples, self.time_bins)
        if why:
            raise ValueError(why)
        audio = self._audio(audio)
        B = audio.shape[0]
        if mask is not None:
            checked_mask(mask, B, self.n_filters, self.time_bins)
        if fused is None:
            fused = self.filterbank == "gammatone" and self.will_fuse()
        if fused and self.filterbank == "mel":
            raise ValueError("the mel branch has no one-launch ragged kernel: encode_ragged takes its split route (fused=False)")
        if not fused and workspace is not None:
            raise ValueError("workspace belongs to the fused launch; this call takes the split route")
        raster = self._raster_for(B, raster_out)        # (refused before the bins are looked at, the workspace after them)
        n_thr = len(self.thresholds)
        with torch.cuda.device(self.device):
            bins_dev = self._device_bins(bins, B)
            if fused:
                on, off = threshold_tables(self.thresholds, self.gap, np.float64)
                steps = torch.empty((B,), dtype=torch.int32, device=self.device)
                ws, ws_bytes = self._workspace_for(B, workspace)
                args = (_dev(audio), B, self.n_samples, _dev(self.coefs), self.n_filters, self.nwin, self.hop, self.ncols,
                        self.time_bins, _dev(bins_dev), _host(on), _host(off), len(on), self.redundancy, _dev(raster),
                        _dev(steps), _dev(ws), ws_bytes, self.coef_flags, self._launch_flags(low_latency, share_lds))
                if mask is None:
                    _lib.check(self.lib.lsm_gammatone_spikes_ragged_f64(*args, self._stream()),
                               "lsm_gammatone_spikes_ragged_f64")
                else:
                    fm, tm = upload_mask(mask, B, self.n_filters, self.time_bins, self.device)
                    _lib.check(self.lib.lsm_gammatone_spikes_ragged_masked_f64(*args, _dev(fm), _dev(tm), self._stream()),
                               "lsm_gammatone_spikes_ragged_masked_f64")
                return raster, steps
            t = self._clamped_bins(bins_dev)
            steps = (t * n_thr).to(torch.int32)
            if self.filterbank == "gammatone":
                # the filter is causal: the padded row's columns below a clip's count are the clip's own
                cols = torch.where(t > 0, t - (self.time_bins - self.ncols), torch.zeros_like(t)).to(torch.int32)
                db = torch.empty((B, self.n_filters, self.ncols), dtype=torch.float64, device=self.device)
                _lib.check(self.lib.lsm_gammatone_spec_f64(
                    _dev(audio), B, self.n_samples, _dev(self.coefs), self.n_filters, self.nwin, self.hop, self.ncols, None,
                    _dev(db), self.coef_flags, self._stream()), "lsm_gammatone_spec_f64")
            else:
                # frames are independent and centred with zero padding: with zeros from a clip's end on, the padded row's
                # frames up to the clip's last are the clip's own
                live = torch.arange(self.n_samples, device=self.device)[None, :] < (t * RAGGED_HOP)[:, None]
                staged = torch.where(live, audio, torch.zeros((), dtype=audio.dtype, device=self.device))
                cols = torch.where(t > 0, t + 1, torch.zeros_like(t)).to(torch.int32)
                power = self._mel.power(staged)
                db = torch.empty_like(power)
                from . import mel as _mel
                _lib.check(self.lib.lsm_power_to_db_ragged_f32(
                    _dev(power), B, self.n_filters, int(power.shape[2]), _dev(cols), C.c_float(_mel.AMIN),
                    C.c_float(_mel.TOP_DB), _dev(db), self._stream()), "lsm_power_to_db_ragged_f32")
            self.spikes_from_db_ragged(db, cols.contiguous(), t.to(torch.int32).contiguous(), raster_out=raster, mask=mask)
        return raster, steps


    def db_range(self, audio):
        """Calibration range for `GammatoneStream` from a batch of calibration clips (B, n_samples): ``(lo, hi)`` Python
        floats, the minimum and maximum of the split path's dB values over the whole batch after the 80 dB floor below the
        maximum (``lo = max(min, hi - 80)``)."""
        if self.filterbank != "gammatone":
            raise ValueError("db_range calibrates the streamed gammatone front end; this front end is a mel filterbank")
        db, _ = self.spectrogram_db(audio)
        hi = db.max()
        lo = torch.maximum(db.min(), hi - 80.0)
        return float(lo), float(hi)

    def mel_db_range(self, audio):
        """Calibration range for `MelStream` from a batch of calibration clips (B, n_samples): ``(lo, hi)`` Python floats in
        ABSOLUTE dB (no per-clip reference level): ``hi = 10 * log10(max(amin, max S))`` over the mel power values
        (`MelSpectrogram.power`) of the whole batch and ``lo = max(10 * log10(max(amin, min S)), hi - 80)``."""
        if self.filterbank != "mel":
            raise ValueError("mel_db_range calibrates the streamed mel front end; this front end is a gammatone filterbank "
                             "(use db_range)")
        from . import mel as _mel
        with torch.cuda.device(self.device):
            S = self._mel.power(self._audio(audio))
            db = 10.0 * torch.log10(torch.clamp(torch.stack([S.min(), S.max()]), min=_mel.AMIN))
        lo, hi = (float(v) for v in db.cpu())
        return max(lo, hi - _mel.TOP_DB), hi


# ---- ragged batches: host side (SPEC.md §1.14) -------------------------------------------------------------------------
RAGGED_HOP = 160            # samples per time bin of a ragged clip: the reference's 100 bins per second (= STREAM_HOP)
RAGGED_MIN_BINS = 3         # gtgram on 160 * T samples has T - 2 columns: a clip needs one


def ragged_refusal(n_samples: int, time_bins: int) -> str | None:
    """Why a front end of this shape cannot take ragged batches, or None: its rows must hold ``time_bins`` bins of 160
    samples, so that a clip of T bins is the front end of ``(160 * T, T)`` whatever T is."""
    if int(time_bins) < RAGGED_MIN_BINS:
        return f"ragged batches need time_bins >= {RAGGED_MIN_BINS}, this front end has {time_bins}"
    if int(n_samples) != RAGGED_HOP * int(time_bins):
        return (f"ragged batches take {RAGGED_HOP} samples per time bin: a front end of {time_bins} bins needs n_samples = "
                f"{RAGGED_HOP * int(time_bins)}, this one has {n_samples} (hops other than {RAGGED_HOP} are not built)")
    return None


def checked_ragged_bins(bins, n_clips: int, time_bins: int):
    """The ``bins`` of a ragged batch: host integers -> an int32 array, each 0 or RAGGED_MIN_BINS .. time_bins, refused
    otherwise with the offenders named; an int32 tensor of ``n_clips`` values on a GPU -> None (its values are never read
    back: the kernels clamp them)."""
    if isinstance(bins, torch.Tensor):
        if bins.dtype != torch.int32 or tuple(bins.shape) != (n_clips,):
            raise ValueError(f"bins must hold {n_clips} int32 values, got {bins.dtype} {tuple(bins.shape)}")
        if bins.is_cuda:
            return None
        bins = bins.numpy()
    arr = np.asarray(bins)
    if arr.shape != (n_clips,) or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"bins must be {n_clips} integers, got {arr.dtype} {arr.shape}")
    arr = arr.astype(np.int64)
    bad = np.nonzero(((arr != 0) & (arr < RAGGED_MIN_BINS)) | (arr < 0) | (arr > time_bins))[0]
    if len(bad):
        raise ValueError(f"bins {arr[bad].tolist()} of clips {bad.tolist()}: a clip has 0 or {RAGGED_MIN_BINS} .. {time_bins} "
                         f"time bins")
    return arr.astype(np.int32)


def pack_utterances(utterances, max_bins: int):
    """Utterances of any length as one ragged batch: a list of n 1-D arrays -> ``(audio (n, 160 * max_bins) float32, bins
    (n,) int32)`` in the input order.  Utterance r is zero-padded up to a whole bin, ``bins[r] = ceil(len / 160)``, and lies
    at the start of row r; the rest of the row is zeros.  Refused, with the index of the offender: anything that is not
    1-D, an utterance of fewer than 3 bins (321 samples at least) and one of more than ``max_bins``.  NumPy only."""
    max_bins = int(max_bins)
    if max_bins < RAGGED_MIN_BINS:
        raise ValueError(f"max_bins = {max_bins}: a clip has at least {RAGGED_MIN_BINS} time bins")
    audio = np.zeros((len(utterances), RAGGED_HOP * max_bins), dtype=np.float32)
    bins = np.zeros(len(utterances), dtype=np.int32)
    for r, u in enumerate(utterances):
        a = np.asarray(u)
        if a.ndim != 1:
            raise ValueError(f"utterance {r} must be a 1-D array, got shape {tuple(a.shape)}")
        t = -(-a.shape[0] // RAGGED_HOP)
        if t < RAGGED_MIN_BINS or t > max_bins:
            raise ValueError(f"utterance {r} has {a.shape[0]} samples = {t} time bins of {RAGGED_HOP}, outside "
                             f"[{RAGGED_MIN_BINS}, {max_bins}]")
        audio[r, :a.shape[0]] = a
        bins[r] = t
    return audio, bins


# ---- streamed gammatone front end (SPEC.md §1.6, include/lsm_hip_audio.h) ----------------------------------------------
STREAM_NWIN = 400           # 25 ms at 16 kHz
STREAM_HOP = 160            # 10 ms: 100 columns per second, one time bin each


def _check_stream_strides(nwin: int, hop: int) -> None:
    if hop < 1 or nwin < hop or nwin > 4 * hop:
        raise ValueError(f"nwin = {nwin} and hop = {hop}: need hop >= 1 and hop <= nwin <= 4 * hop")


def stream_column_plan(seen_hops, new_hops, nwin: int = STREAM_NWIN, hop: int = STREAM_HOP):
    """The columns one push completes, host integers only.  Column c of a stream covers its samples
    ``[c * hop, c * hop + nwin)`` counted from the stream's start, and a stream that has seen n whole hops has
    ``complete(n) = 0 if n * hop < nwin else (n * hop - nwin) // hop + 1`` of them.  A stream that had seen ``seen_hops``
    hops and receives ``new_hops`` more completes ``complete(seen + new) - complete(seen)`` columns.  Scalars or arrays of
    equal shape; returns an int or an int64 array."""
    nwin, hop = int(nwin), int(hop)
    _check_stream_strides(nwin, hop)
    seen_a, new_a = np.asarray(seen_hops, dtype=np.int64), np.asarray(new_hops, dtype=np.int64)
    if (seen_a < 0).any() or (new_a < 0).any():
        raise ValueError("stream_column_plan: seen_hops and new_hops must be >= 0")

    def complete(n):
        return np.where(n * hop >= nwin, (n * hop - nwin) // hop + 1, 0)

    cols = complete(seen_a + new_a) - complete(seen_a)
    return int(cols) if np.ndim(seen_hops) == 0 and np.ndim(new_hops) == 0 else cols


class _StreamPush:
    """What a push of any bank of streams needs: the check of a caller-owned output and the upload of its counts.  A
    subclass sets n_streams and device.  (`MixStream`, whose whole state is a noise position per stream, stops here.)"""

    def _owned(self, t, shape, dtype, name, word=None, audio=None, reason=None):
        """A caller-owned output checked (`checked_out`), or zeros where the caller gave none.  (``word``: the dtype as the
        refusal says it; the front-end streams, which give none, have always said "torch.uint8".)"""
        if t is None:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        return checked_out(t, shape, self.device, audio, reason, name=name, dtype=dtype, word=word or str(dtype))

    def _count_array(self, given, new):
        """A push's per-stream counts for the kernel: None where the caller gave none (every stream takes the whole row),
        or the checked counts ``new`` as int32 on the device."""
        return None if given is None else torch.from_numpy(new.astype(np.int32)).to(self.device)


class _StreamBank(_StreamPush):
    """A bank with ``n_streams`` state blocks on the device (DESIGN.md "The state block"; all zeros are a stream's start).
    A subclass sets n_streams and device before it asks for the state."""

    def _new_state(self, state_bytes) -> None:
        self.state_bytes = int(state_bytes)
        self.state = torch.zeros((self.n_streams, self.state_bytes), dtype=torch.uint8, device=self.device)

    def _reset_state(self, slots) -> np.ndarray:
        """The state blocks of ``slots`` back to zeros; returns the checked slots for what else a subclass clears."""
        slots = checked_slots(slots, self.n_streams)
        self.state[torch.from_numpy(slots).to(self.device)] = 0
        return slots

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: their state blocks back to zeros."""
        self._reset_state(slots)


class _AudioStreamBase(_StreamBank):
    """What the streamed front ends share beyond `_StreamBank`: the hops each stream has seen and the checks of a push's
    arguments.  A subclass sets n_filters, n_streams, hop, redundancy, on, device, state and seen."""

    @property
    def n_thr(self) -> int:
        return len(self.on)

    @property
    def n_channels(self) -> int:
        return self.n_filters * self.redundancy

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: state block and hop count back to zero."""
        self.seen[self._reset_state(slots)] = 0

    def _pushed(self, audio, hops):
        """A push's arguments checked: (audio on the device, H, the new hops per stream as int64)."""
        audio = as_float32(audio).to(self.device)
        if audio.dim() != 2 or audio.shape[0] != self.n_streams or audio.shape[1] % self.hop or audio.shape[1] < self.hop:
            raise ValueError(f"audio must be ({self.n_streams}, H * {self.hop}) with H >= 1, got {tuple(audio.shape)}")
        H = int(audio.shape[1]) // self.hop
        return audio, H, checked_counts(hops, self.n_streams, H, "hops")


class GammatoneStream(_AudioStreamBase):
    """``n_streams`` open-ended audio streams through one gammatone -> dB -> fixed-range normalise -> hysteresis encoder
    kernel (`lsm_gammatone_stream_f64`, SPEC.md §1.6).  Every ``push`` advances each stream by the whole hops it delivers --
    any number, 0 included -- from the state the bank holds (filter state, open window sums, latches), and returns the
    raster columns those hops completed: one time bin per column, normalised with the calibration range ``db_range``
    (``SpikeFrontEnd.db_range``) fixed for the streams' lives.  A stream cut into pushes at any hop boundaries gives, bit for
    bit, the raster of its uncut run."""
    filterbank = "gammatone"

    def __init__(self, n_filters: int, n_streams: int, db_range, thresholds=None, gap: float = HYSTERESIS_GAP,
                 redundancy: int = REDUNDANCY_FACTOR, device=None, nwin: int = STREAM_NWIN, hop: int = STREAM_HOP):
        self.n_filters, self.n_streams = int(n_filters), int(n_streams)
        self.nwin, self.hop, self.redundancy = int(nwin), int(hop), int(redundancy)
        if self.n_filters < 2:
            raise ValueError("the gammatone branch needs n_filters >= 2 (SPEC.md 1.1)")
        if self.n_streams < 1 or self.redundancy < 1:
            raise ValueError(f"GammatoneStream needs n_streams >= 1 and redundancy >= 1, got {n_streams}, {redundancy}")
        _check_stream_strides(self.nwin, self.hop)
        self.db_lo, self.db_hi = (float(v) for v in db_range)
        if not (np.isfinite(self.db_lo) and np.isfinite(self.db_hi) and self.db_lo < self.db_hi):
            raise ValueError(f"db_range = ({self.db_lo}, {self.db_hi}) must be finite with lo < hi")
        self.thresholds = list(SPIKE_THRESHOLDS if thresholds is None else thresholds)
        self.gap = float(gap)
        self.on, self.off = threshold_tables(self.thresholds, self.gap, np.float64)
        self.lib, self.device = _open(device)
        tab = gammatone_filter_table(SAMPLE_RATE, self.n_filters, GT_F_MIN)
        self.coefs = torch.from_numpy(tab).to(self.device)
        self.coef_flags = coef_flags(tab)
        self._new_state(self.lib.lsm_gammatone_stream_state_bytes(self.n_filters, self.nwin, self.hop))
        self.seen = np.zeros(self.n_streams, dtype=np.int64)            # hops since the stream's start

    def push(self, audio, hops=None, want_db: bool = False, want_spec: bool = False, raster_out=None, db_out=None,
             spec_out=None):
        """``audio`` (n_streams, H * hop) float32: stream b's new samples are the first ``hops[b] * hop`` of its row;
        ``hops``: n_streams host integers in [0, H], or None for H everywhere.  Returns ``(raster, cols)``: ``raster`` uint8
        (n_streams, C, H * n_thr) on the device and ``cols`` (int64, host) -- the first ``cols[b] * n_thr`` steps of stream
        b's rows are the columns this push completed (`stream_column_plan`); what lies behind them is zeros, or what a
        caller-owned ``raster_out`` held.  With ``want_db`` / ``want_spec`` (or caller-owned ``db_out`` / ``spec_out``) the
        return is ``(raster, cols, db, spec)``: float64 (n_streams, F, H), written like the raster, None where not asked."""
        audio, H, new = self._pushed(audio, hops)
        cols = stream_column_plan(self.seen, new, self.nwin, self.hop)
        with torch.cuda.device(self.device):
            raster = self._owned(raster_out, (self.n_streams, self.n_channels, H * self.n_thr), torch.uint8, "raster_out")
            shape = (self.n_streams, self.n_filters, H)
            db = self._owned(db_out, shape, torch.float64, "db_out") if (want_db or db_out is not None) else None
            spec = self._owned(spec_out, shape, torch.float64, "spec_out") if (want_spec or spec_out is not None) else None
            counts = self._count_array(hops, new)
            _lib.check(self.lib.lsm_gammatone_stream_f64(
                _dev(audio), self.n_streams, H, _dev(self.coefs), self.n_filters, self.nwin, self.hop, _dev(counts), self.db_lo,
                self.db_hi, _host(self.on), _host(self.off), self.n_thr, self.redundancy, _dev(self.state), _dev(self.state),
                _dev(raster), _dev(spec), _dev(db), self.coef_flags, _stream(self.device)), "lsm_gammatone_stream_f64")
        self.seen += new
        if db is not None or spec is not None:
            return raster, cols, db, spec
        return raster, cols


# ---- streamed mel front end (SPEC.md §1.7, include/lsm_hip_mel_stream.h) ------------------------------------------------
MEL_N_FFT = 2048


def _check_mel_hop(hop: int, n_fft: int) -> None:
    if n_fft != MEL_N_FFT:
        raise ValueError(f"n_fft = {n_fft}: the mel kernels transform {MEL_N_FFT}-sample frames only")
    if hop < n_fft // 16 or hop > n_fft // 2:
        raise ValueError(f"hop = {hop} outside [{n_fft // 16}, {n_fft // 2}] (n_fft / 16 .. n_fft / 2)")


def mel_stream_frame_plan(seen_hops, new_hops, hop: int = STREAM_HOP, n_fft: int = MEL_N_FFT):
    """The frames one push completes, host integers only.  Frame t of a stream is centred on its sample ``t * hop`` and is
    complete once the stream holds ``t * hop + n_fft / 2`` samples (no frame touches an end padding), so a stream that has
    seen n whole hops has ``complete(n) = max(0, n - Lg + 1)`` of them, ``Lg = ceil((n_fft / 2) / hop)``.  A stream that
    had seen ``seen_hops`` hops and receives ``new_hops`` more completes ``complete(seen + new) - complete(seen)`` frames.
    Scalars or arrays of equal shape; returns an int or an int64 array."""
    hop, n_fft = int(hop), int(n_fft)
    _check_mel_hop(hop, n_fft)
    seen_a, new_a = np.asarray(seen_hops, dtype=np.int64), np.asarray(new_hops, dtype=np.int64)
    if (seen_a < 0).any() or (new_a < 0).any():
        raise ValueError("mel_stream_frame_plan: seen_hops and new_hops must be >= 0")
    lg = -(-(n_fft // 2) // hop)

    def complete(n):
        return np.maximum(n - lg + 1, 0)

    cols = complete(seen_a + new_a) - complete(seen_a)
    return int(cols) if np.ndim(seen_hops) == 0 and np.ndim(new_hops) == 0 else cols


class MelStream(_AudioStreamBase):
    """``n_streams`` open-ended audio streams through the streamed mel front end (`lsm_mel_stream_f32`, SPEC.md §1.7):
    centred STFT frames -> mel power -> absolute dB -> fixed-range normalise -> hysteresis encoder.  Every ``push`` advances
    each stream by the whole hops it delivers -- any number, 0 included -- from the state the bank holds (the tail of samples
    the next frames reach back into, the latches, a hop count), and returns the raster columns of the frames those hops
    completed: one time bin per frame, normalised with the calibration range ``db_range`` (``SpikeFrontEnd.mel_db_range``)
    fixed for the streams' lives.  A stream cut into pushes at any hop boundaries gives, byte for byte, the raster of its
    uncut run.  The interface is `GammatoneStream`'s."""
    filterbank = "mel"
    streamed = True

    def __init__(self, n_filters: int, n_streams: int, db_range, thresholds=None, gap: float = HYSTERESIS_GAP,
                 redundancy: int = REDUNDANCY_FACTOR, device=None, hop: int = STREAM_HOP):
        self.n_filters, self.n_streams = int(n_filters), int(n_streams)
        self.hop, self.redundancy = int(hop), int(redundancy)
        if self.n_filters < 1:
            raise ValueError(f"n_filters must be >= 1, got {n_filters}")
        if self.n_streams < 1 or self.redundancy < 1:
            raise ValueError(f"MelStream needs n_streams >= 1 and redundancy >= 1, got {n_streams}, {redundancy}")
        _check_mel_hop(self.hop, MEL_N_FFT)
        self.db_lo, self.db_hi = (float(v) for v in db_range)
        lo32, hi32 = np.float32(self.db_lo), np.float32(self.db_hi)     # the kernel's values: rounded to float32 once
        if not (np.isfinite(lo32) and np.isfinite(hi32) and lo32 < hi32):
            raise ValueError(f"db_range = ({self.db_lo}, {self.db_hi}) must be finite with lo < hi (as float32 values)")
        self.thresholds = list(SPIKE_THRESHOLDS if thresholds is None else thresholds)
        self.gap = float(gap)
        self.on, self.off = threshold_tables(self.thresholds, self.gap, np.float32)
        self.lib, self.device = _open(device)
        from . import mel as _mel
        self.window, self.twiddle, self.basis, self.lo, self.hi = _mel.device_tables(self.n_filters, self.device)
        self._new_state(self.lib.lsm_mel_stream_state_bytes(self.n_filters, MEL_N_FFT, self.hop))
        self.seen = np.zeros(self.n_streams, dtype=np.int64)            # hops since the stream's start
        self._ws = None                                                 # scratch of the launches, grown on demand

    def push(self, audio, hops=None, want_db: bool = False, want_power: bool = False, raster_out=None, db_out=None,
             power_out=None):
        """``audio`` (n_streams, H * hop) float32: stream b's new samples are the first ``hops[b] * hop`` of its row;
        ``hops``: n_streams host integers in [0, H], or None for H everywhere.  Returns ``(raster, cols)``: ``raster`` uint8
        (n_streams, C, H * n_thr) on the device and ``cols`` (int64, host) -- the first ``cols[b] * n_thr`` steps of stream
        b's rows are the frames this push completed (`mel_stream_frame_plan`); what lies behind them is zeros, or what a
        caller-owned ``raster_out`` held.  With ``want_db`` / ``want_power`` (or caller-owned ``db_out`` / ``power_out``) the
        return is ``(raster, cols, db, power)``: float32 (n_streams, F, H), written like the raster, None where not asked;
        ``db`` holds the un-floored ``10 * log10(max(1e-10, power))``."""
        audio, H, new = self._pushed(audio, hops)
        cols = mel_stream_frame_plan(self.seen, new, self.hop)
        with torch.cuda.device(self.device):
            raster = self._owned(raster_out, (self.n_streams, self.n_channels, H * self.n_thr), torch.uint8, "raster_out")
            shape = (self.n_streams, self.n_filters, H)
            db = self._owned(db_out, shape, torch.float32, "db_out") if (want_db or db_out is not None) else None
            power = self._owned(power_out, shape, torch.float32, "power_out") if (want_power or power_out is not None) else None
            counts = self._count_array(hops, new)
            need = int(self.lib.lsm_mel_stream_workspace(self.n_streams, self.n_filters, H))
            if self._ws is None or self._ws.numel() < need:
                # launches of one bank run in order on the current stream and may share the scratch; the caching allocator
                # keeps a replaced one alive until the launches that used it have run
                self._ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.lsm_mel_stream_f32(
                _dev(audio), self.n_streams, H, MEL_N_FFT, self.hop, _dev(self.window), _dev(self.twiddle), _dev(self.basis),
                _dev(self.lo), _dev(self.hi), self.n_filters, _dev(counts), self.db_lo, self.db_hi, _host(self.on),
                _host(self.off), self.n_thr, self.redundancy, _dev(self.state), _dev(self.state), _dev(raster), _dev(power),
                _dev(db), _dev(self._ws), int(self._ws.numel()), _stream(self.device)), "lsm_mel_stream_f32")
        self.seen += new
        if db is not None or power is not None:
            return raster, cols, db, power
        return raster, cols


# ---- adaptive normalisation range (SPEC.md §1.9, include/lsm_hip_adaptive.h) ---------------------------------------------
ADAPTIVE_WINDOW_COLS = 100          # columns of STREAM_HOP samples: one second, the reference's own window
ADAPTIVE_MAX_WINDOW = 4096
_ADAPTIVE_DTYPES = {torch.float64: np.float64, torch.float32: np.float32}


class AdaptiveEncoder(_StreamBank):
    """The spike encoder with a sliding normalisation range (`lsm_adaptive_encode_f64` / `_f32`, SPEC.md §1.9): dB columns
    of ``n_streams`` streams in, raster columns out.  Column c is normalised with the minimum and maximum of the stream's
    columns ``max(0, c - window_cols + 1) .. c`` after the 80 dB floor -- the reference's per-clip rule made causal -- and
    goes through the hysteresis latches, which the encoder carries over pushes together with the extrema of the last
    ``window_cols - 1`` columns.  A stream cut into pushes anywhere gives, byte for byte, the raster of its uncut run.
    ``dtype``: torch.float64 (the gammatone stream's dB) or torch.float32 (the mel stream's)."""

    def __init__(self, n_filters: int, n_streams: int, dtype, window_cols: int = ADAPTIVE_WINDOW_COLS, thresholds=None,
                 gap: float = HYSTERESIS_GAP, redundancy: int = REDUNDANCY_FACTOR, device=None):
        self.n_filters, self.n_streams = int(n_filters), int(n_streams)
        self.window_cols, self.redundancy = int(window_cols), int(redundancy)
        if isinstance(dtype, torch.dtype):
            if dtype not in _ADAPTIVE_DTYPES:
                raise ValueError(f"dtype must be float64 or float32, got {dtype}")
            self.dtype = dtype
        else:
            if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
                raise ValueError(f"dtype must be float64 or float32, got {dtype!r}")
            self.dtype = torch.float64 if np.dtype(dtype) == np.dtype(np.float64) else torch.float32
        if self.n_filters < 1:
            raise ValueError(f"n_filters must be >= 1, got {n_filters}")
        if self.n_streams < 1 or self.redundancy < 1:
            raise ValueError(f"AdaptiveEncoder needs n_streams >= 1 and redundancy >= 1, got {n_streams}, {redundancy}")
        if not 1 <= self.window_cols <= ADAPTIVE_MAX_WINDOW:
            raise ValueError(f"window_cols = {window_cols} outside [1, {ADAPTIVE_MAX_WINDOW}]")
        self.thresholds = list(SPIKE_THRESHOLDS if thresholds is None else thresholds)
        self.gap = float(gap)
        self.on, self.off = threshold_tables(self.thresholds, self.gap, _ADAPTIVE_DTYPES[self.dtype])
        self.lib, self.device = _open(device)
        self._encode = self.lib.lsm_adaptive_encode_f64 if self.dtype == torch.float64 else self.lib.lsm_adaptive_encode_f32
        elem = 8 if self.dtype == torch.float64 else 4
        state_bytes = int(self.lib.lsm_adaptive_state_bytes(self.n_filters, self.window_cols, elem))
        if state_bytes < 1:
            raise ValueError(f"the encoder refuses n_filters = {n_filters} with window_cols = {window_cols}")
        self._new_state(state_bytes)

    @property
    def n_thr(self) -> int:
        return len(self.on)

    @property
    def n_channels(self) -> int:
        return self.n_filters * self.redundancy

    def push_db(self, db, cols=None, raster_out=None, want_range: bool = False):
        """``db`` (n_streams, n_filters, H) of the encoder's dtype: stream b's new columns are the first ``cols[b]`` of its
        rows; ``cols``: n_streams host integers in [0, H], or None for H everywhere.  Returns ``raster`` uint8 (n_streams, C,
        H * n_thr) on the device -- the first ``cols[b] * n_thr`` steps of stream b's rows; what lies behind them is zeros,
        or what a caller-owned ``raster_out`` held -- or, with ``want_range``, ``(raster, lo, hi)``: the range every column
        was normalised with, (n_streams, H) of the encoder's dtype, written like the raster."""
        if isinstance(db, np.ndarray):
            db = torch.from_numpy(np.ascontiguousarray(db))
        if not torch.is_tensor(db) or db.dtype != self.dtype or db.dim() != 3 \
                or tuple(db.shape[:2]) != (self.n_streams, self.n_filters) or db.shape[2] < 1:
            raise ValueError(f"db must be a {self.dtype} ({self.n_streams}, {self.n_filters}, H) array with H >= 1, got "
                             f"{getattr(db, 'dtype', type(db).__name__)} {tuple(getattr(db, 'shape', ()))}")
        H = int(db.shape[2])
        new = checked_counts(cols, self.n_streams, H, "cols")
        shape = (self.n_streams, self.n_channels, H * self.n_thr)
        with torch.cuda.device(self.device):
            raster = self._owned(raster_out, shape, torch.uint8, "raster_out", "uint8")
            db = db.to(self.device).contiguous()
            lo = hi = None
            if want_range:
                lo = torch.zeros((self.n_streams, H), dtype=self.dtype, device=self.device)
                hi = torch.zeros((self.n_streams, H), dtype=self.dtype, device=self.device)
            counts = self._count_array(cols, new)
            _lib.check(self._encode(
                _dev(db), self.n_streams, H, self.n_filters, _dev(counts), self.window_cols, _host(self.on), _host(self.off),
                self.n_thr, self.redundancy, _dev(self.state), _dev(self.state), _dev(raster), _dev(lo), _dev(hi),
                _stream(self.device)), "lsm_adaptive_encode")
        return (raster, lo, hi) if want_range else raster


class AdaptiveStream:
    """A streamed front end (`GammatoneStream` or `MelStream`) whose columns are normalised with the range of the stream's
    last ``window_cols`` columns instead of a calibration range (SPEC.md §1.9): every ``push`` runs ``inner``'s push for its
    dB columns and then `AdaptiveEncoder.push_db` on them.  The raster no longer depends on the recording level, and no
    calibration batch is needed: ``inner``'s ``db_range`` is a placeholder -- any valid range will do, it only feeds
    ``inner``'s own raster, which goes to a scratch buffer and is not used.  Thresholds, gap and redundancy are ``inner``'s.
    ``window_cols = 100`` columns of 10 ms are one second, the clip the reference normalises over: a stream that has held at
    most ``window_cols`` columns is normalised exactly like the reference's clip of those columns.  The interface is
    `GammatoneStream`'s, so `pipeline.AudioStreamBank` takes it in ``inner``'s place."""
    streamed = True

    def __init__(self, inner, window_cols: int = ADAPTIVE_WINDOW_COLS):
        if getattr(inner, "filterbank", None) not in ("gammatone", "mel") or not isinstance(inner, _AudioStreamBase):
            raise ValueError("AdaptiveStream wraps a streamed front end: frontend.GammatoneStream or frontend.MelStream")
        self.inner = inner
        self.filterbank = inner.filterbank
        self.n_filters, self.n_streams, self.hop = inner.n_filters, inner.n_streams, inner.hop
        self.redundancy, self.device = inner.redundancy, inner.device
        self.db_dtype = torch.float64 if inner.filterbank == "gammatone" else torch.float32
        self.encoder = AdaptiveEncoder(inner.n_filters, inner.n_streams, self.db_dtype, window_cols, inner.thresholds,
                                       inner.gap, inner.redundancy, inner.device)
        self.window_cols = self.encoder.window_cols
        self._scratch = None                                            # (H, inner raster, dB) of the last push's shape

    @property
    def n_thr(self) -> int:
        return self.encoder.n_thr

    @property
    def n_channels(self) -> int:
        return self.encoder.n_channels

    @property
    def seen(self) -> np.ndarray:
        """Hops since each stream's start: ``inner``'s count."""
        return self.inner.seen

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: both halves start over."""
        checked_slots(slots, self.n_streams)
        self.inner.reset(slots)
        self.encoder.reset(slots)

    def push(self, audio, hops=None, raster_out=None, want_db: bool = False):
        """``audio`` and ``hops`` as `GammatoneStream.push` takes them.  Returns ``(raster, cols)`` with its meaning -- the
        first ``cols[b] * n_thr`` steps of stream b's rows are the columns this push completed -- or, with ``want_db``,
        ``(raster, cols, db)``: ``inner``'s dB columns (n_streams, F, H), float64 for gammatone and float32 for mel."""
        audio, H, _ = self.inner._pushed(audio, hops)
        with torch.cuda.device(self.device):
            if self._scratch is None or self._scratch[0] != H:
                self._scratch = (H, torch.zeros((self.n_streams, self.n_channels, H * self.n_thr), dtype=torch.uint8,
                                                device=self.device),
                                 torch.zeros((self.n_streams, self.n_filters, H), dtype=self.db_dtype, device=self.device))
            _, unused, db = self._scratch
            if want_db:                                                 # the caller keeps it: not the buffer of the next push
                db = torch.zeros_like(db)
            _, cols, db, _ = self.inner.push(audio, hops, raster_out=unused, db_out=db)
            # every stream completed all H columns (the steady state): no count array to upload
            raster = self.encoder.push_db(db, None if (cols == H).all() else cols, raster_out=raster_out)
        return (raster, cols, db) if want_db else (raster, cols)


# ---- polyphase resampler (SPEC.md §1.8, include/lsm_hip_resample.h) -----------------------------------------------------
RESAMPLE_HALF_WIDTH = 10            # scipy.signal.resample_poly: half = 10 * max(up, down)
RESAMPLE_KAISER_BETA = 5.0          # its default window, ('kaiser', 5.0)
RESAMPLE_LDS_BYTES = 160 * 1024     # the tap table laid out by phase must fit a CU's LDS


class ResampleTable(NamedTuple):
    """The design of one rate pair: ``taps`` is hp, the prototype filter behind its ``pre`` leading zeros (float64, K
    values); ``delay`` D the batch form's shift in output samples; ``history`` Hs the input samples a stream carries."""
    up: int
    down: int
    taps: np.ndarray
    delay: int
    history: int
    pre: int


def _checked_rates(rate_in, rate_out):
    for name, r in (("rate_in", rate_in), ("rate_out", rate_out)):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or int(r) < 1:
            raise ValueError(f"{name} must be a positive integer number of samples per second, got {r!r}")
    return int(rate_in), int(rate_out)


def resample_table(rate_in: int, rate_out: int = SAMPLE_RATE) -> ResampleTable:
    """The polyphase filter of SPEC.md §1.8 for ``rate_in`` -> ``rate_out``, on the host in float64 with NumPy only:
    ``scipy.signal.firwin(2 * half + 1, 1 / mr, window=('kaiser', 5.0)) * up`` restated, ``mr = max(up, down)``,
    ``half = 10 * mr``, behind ``pre = down - half % down`` zeros as ``resample_poly`` places it."""
    rate_in, rate_out = _checked_rates(rate_in, rate_out)
    if rate_in == rate_out:
        raise ValueError(f"rate_in == rate_out ({rate_in}): there is nothing to design")
    g = gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    mr = max(up, down)
    half = RESAMPLE_HALF_WIDTH * mr
    n = np.arange(2 * half + 1, dtype=np.float64)
    h = (1.0 / mr) * np.sinc((n - half) / mr) * np.kaiser(2 * half + 1, RESAMPLE_KAISER_BETA)
    h = h / h.sum() * up
    pre = down - half % down
    taps = np.concatenate([np.zeros(pre, dtype=np.float64), h])
    table_bytes = up * (-(-len(taps) // up) | 1) * 8            # [phase][tap] with an odd row stride (csrc/resample_body.h)
    if table_bytes > RESAMPLE_LDS_BYTES:
        raise ValueError(f"{rate_in} -> {rate_out} Hz needs {len(taps)} taps in {up} phases: {table_bytes} bytes laid out by "
                         f"phase, over the {RESAMPLE_LDS_BYTES} of a compute unit's LDS (lsm_resample_f32 refuses it)")
    return ResampleTable(up, down, taps, (half + pre) // down, (len(taps) - 1) // up, pre)


def resample_units(up: int, down: int, hop: int = STREAM_HOP):
    """The smallest push of a resampled stream that is a whole number of front-end hops: ``(unit_blocks, unit_in,
    unit_hops)`` -- ``unit_blocks = hop / gcd(up, hop)`` blocks of ``down`` input samples, which are ``unit_in`` samples in
    and ``unit_blocks * up = unit_hops * hop`` out."""
    g = gcd(int(up), int(hop))
    return hop // g, hop // g * int(down), int(up) // g


def checked_pcm(audio, n_rows: int | None = None, multiple: int = 1, what: str = "audio"):
    """Mono PCM rows as the resampler takes them: a 2-D float32 or int16 NumPy array (copied) or tensor, ``n_rows`` rows when
    given, a positive multiple of ``multiple`` samples each.  Returns ``(contiguous tensor on the device it is on,
    sample_format)``, 0 for float32 and 1 for int16; refuses everything else with a ValueError."""
    if isinstance(audio, np.ndarray):
        if audio.dtype not in (np.float32, np.int16):
            raise ValueError(f"{what} must be float32 or int16, got {audio.dtype}")
        audio = torch.from_numpy(np.ascontiguousarray(audio))
    elif not torch.is_tensor(audio) or audio.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"{what} must be a float32 or int16 NumPy array or tensor, got "
                         f"{audio.dtype if torch.is_tensor(audio) else type(audio).__name__}")
    shape = tuple(audio.shape)
    if audio.dim() != 2 or (n_rows is not None and shape[0] != n_rows) or shape[1] < multiple or shape[1] % multiple:
        rows = "n" if n_rows is None else str(n_rows)
        cols = "L >= 1" if multiple == 1 else f"G * {multiple} with G >= 1"
        raise ValueError(f"{what} must be ({rows}, {cols}), got {shape}")
    return audio.contiguous(), 1 if audio.dtype == torch.int16 else 0


def checked_counts(counts, n_streams: int, limit: int, what: str = "blocks") -> np.ndarray:
    """Per-stream counts of a push as an int64 array: ``n_streams`` integers in ``[0, limit]``, or None for ``limit``
    everywhere."""
    if counts is None:
        return np.full(n_streams, limit, dtype=np.int64)
    new = np.asarray(counts)
    if new.shape != (n_streams,) or new.dtype.kind not in "iu" or (new < 0).any() or (new > limit).any():
        raise ValueError(f"{what} must be {n_streams} integers in [0, {limit}], got {counts!r}")
    return new.astype(np.int64)


class _ResampleBase:
    """The design of a rate pair on the host, then -- unless the rates are equal -- the library and the taps on the device."""

    def __init__(self, rate_in, rate_out, device):
        self.rate_in, self.rate_out = _checked_rates(rate_in, rate_out)
        self.identity = self.rate_in == self.rate_out
        table = (ResampleTable(1, 1, np.ones(1, dtype=np.float64), 0, 0, 0) if self.identity
                 else resample_table(self.rate_in, self.rate_out))
        self.up, self.down, self.taps, self.delay, self.history, _ = table
        self.table = table
        self.lib, self.device = _open(device)
        self.taps_dev = torch.from_numpy(self.taps).to(self.device)

    def _as_float(self, audio: torch.Tensor) -> torch.Tensor:
        """Equal rates: the samples as the kernels widen them, float32, an int16 sample times 2^-15."""
        return audio.to(torch.float32) * (1.0 / 32768.0) if audio.dtype == torch.int16 else audio.clone()


class Resampler(_ResampleBase):
    """Batches of mono clips from ``rate_in`` to ``rate_out`` in one launch (`lsm_resample_f32`, SPEC.md §1.8): the samples
    of ``scipy.signal.resample_poly(x, up, down)`` computed in float64 and rounded once to float32, zeros outside a clip.
    ``up``, ``down``, ``delay``, ``taps`` and ``history`` are the design (`resample_table`).  Equal rates are the identity."""
    MAX_ROWS = 65535                    # rows of one launch

    def __init__(self, rate_in: int, rate_out: int = SAMPLE_RATE, device=None):
        super().__init__(rate_in, rate_out, device)

    def default_length(self, n_in: int) -> int:
        """``ceil(n_in * up / down)``, `resample_poly`'s output length."""
        return -(-int(n_in) * self.up // self.down)

    def resample(self, audio, n_out: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """``audio`` (n, L) float32 or int16, NumPy or tensor -> float32 (n, n_out) on the device.  ``n_out`` defaults to
        ``ceil(L * up / down)``; a smaller one gives the first samples of the same result, a larger one continues over the
        zeros behind the clips.  ``out``: a caller-owned contiguous float32 (n, n_out) tensor on the device."""
        audio, fmt = checked_pcm(audio)
        n, L = (int(v) for v in audio.shape)
        n_out = checked_n_out(n_out, self.default_length(L))
        if out is not None:
            checked_out(out, (n, n_out), self.device)
        with torch.cuda.device(self.device):
            audio = audio.to(self.device)
            if out is None:
                out = torch.empty((n, n_out), dtype=torch.float32, device=self.device)
            if self.identity:
                out.zero_()
                out[:, :min(L, n_out)] = self._as_float(audio[:, :n_out])
                return out
            stream = _stream(self.device)
            for r0, k in row_chunks(n, self.MAX_ROWS):
                _lib.check(self.lib.lsm_resample_f32(
                    _dev(audio, r0), fmt, k, L, _dev(self.taps_dev), len(self.taps), self.up, self.down, self.delay, n_out,
                    _dev(out, r0), stream), "lsm_resample_f32")
        return out


class ResampleStream(_ResampleBase, _StreamBank):
    """``n_streams`` open-ended PCM streams from ``rate_in`` to ``rate_out`` (`lsm_resample_stream_f32`, SPEC.md §1.8): every
    ``push`` advances each stream by the whole blocks of ``down`` input samples it delivers -- any number, 0 included -- from
    the history the bank holds (the stream's last ``history`` samples) and returns ``up`` samples per block: the next samples
    of the stream's causal run, which lags `Resampler`'s alignment by ``delay`` samples.  A stream cut into pushes at any
    block boundaries gives, byte for byte, the samples of its uncut run.  ``unit_blocks`` blocks (``unit_in`` samples) are the
    smallest push that is a whole number, ``unit_hops``, of front-end hops (`resample_units`)."""

    def __init__(self, rate_in: int, n_streams: int, rate_out: int = SAMPLE_RATE, device=None):
        self.n_streams = int(n_streams)
        if self.n_streams < 1 or self.n_streams > Resampler.MAX_ROWS:
            raise ValueError(f"ResampleStream needs n_streams in [1, {Resampler.MAX_ROWS}], got {n_streams}")
        super().__init__(rate_in, rate_out, device)
        self.unit_blocks, self.unit_in, self.unit_hops = resample_units(self.up, self.down)
        self._new_state(self.lib.lsm_resample_state_bytes(len(self.taps), self.up))

    def push(self, audio, blocks=None, out: torch.Tensor | None = None):
        """``audio`` (n_streams, G * down) float32 or int16: stream b's new samples are the first ``blocks[b] * down`` of its
        row; ``blocks``: n_streams host integers in [0, G], or None for G everywhere.  Returns ``(out, counts)``: ``out``
        float32 (n_streams, G * up) on the device and ``counts = blocks * up`` (int64, host) -- the first ``counts[b]``
        samples of row b are the stream's next ones; what lies behind them is zeros, or what a caller-owned ``out`` held."""
        audio, fmt = checked_pcm(audio, self.n_streams, self.down)
        G = int(audio.shape[1]) // self.down
        new = checked_counts(blocks, self.n_streams, G)
        with torch.cuda.device(self.device):
            out = self._owned(out, (self.n_streams, G * self.up), torch.float32, "out", "float32")
            audio = audio.to(self.device)
            if self.identity:
                live = torch.from_numpy(np.arange(G)[None, :] < new[:, None]).to(self.device)
                out[live] = self._as_float(audio)[live]
                return out, new * self.up
            counts = self._count_array(blocks, new)
            _lib.check(self.lib.lsm_resample_stream_f32(
                _dev(audio), fmt, self.n_streams, G, _dev(self.taps_dev), len(self.taps), self.up, self.down, _dev(counts),
                _dev(self.state), _dev(self.state), _dev(out), _stream(self.device)), "lsm_resample_stream_f32")
        return out, new * self.up


# ---- per-clip plans (`MixPlan`, `ReverbPlan`, `SpeedPlan`, `MaskPlan`): host arrays of one length, one entry per clip -----------
def _plan_part(plan, lo: int, hi: int):
    """The plan of clips ``lo .. hi - 1``: a batch's or a shard's slice of the whole listing's plan."""
    return type(plan)(*(a[lo:hi] for a in plan))


def _plan_take(plan, idx):
    """The plan of the clips ``idx`` names, in that order (a split of the listing)."""
    idx = np.asarray(idx, dtype=np.int64)
    return type(plan)(*(a[idx] for a in plan))


# ---- noise mixer (SPEC.md §1.10, include/lsm_hip_mix.h) -----------------------------------------------------------------
MIX_MAX_SAMPLES = 1 << 24


class MixPlan(NamedTuple):
    """Per-clip corruption parameters (`mix_plan`), host arrays of one length: ``snr_db`` float64 (+inf = clean), ``rows``
    and ``offsets`` into the noise bank and ``shift`` in samples (int32), ``scale`` float32."""
    snr_db: np.ndarray
    rows: np.ndarray
    offsets: np.ndarray
    shift: np.ndarray
    scale: np.ndarray

    part, take = _plan_part, _plan_take


def _range_draw(value, u: np.ndarray, name: str) -> np.ndarray:
    """A scalar, or ``lo + (hi - lo) * u`` for a ``(lo, hi)`` range; float64."""
    v = np.asarray(value, dtype=np.float64)
    if v.shape == ():
        return np.full(len(u), float(v), dtype=np.float64)
    if v.shape != (2,) or not v[0] <= v[1]:
        raise ValueError(f"{name} must be a number or a (lo, hi) range with lo <= hi, got {value!r}")
    return v[0] + (v[1] - v[0]) * u


def mix_plan(n_clips: int, n_noise_rows: int, noise_len: int, snr_db, max_shift: int = 0, level_db=0.0,
             seed: int = 42) -> MixPlan:
    """The corruption of every clip of a listing, drawn from ``np.random.RandomState(seed)`` for ALL ``n_clips`` clips in
    listing order -- noise rows, noise offsets, shifts in [-max_shift, max_shift], then the SNRs and the levels -- so that
    a shard or a batch takes its slice (`MixPlan.part`) and a multi-rank run corrupts every clip exactly as one process
    does.  ``snr_db`` and ``level_db`` are a number or a ``(lo, hi)`` range drawn uniformly in dB; the draws are made in
    either form, so a scalar changes no other array.  ``scale = float32(10 ** (level_db / 20))``."""
    n, M, L, S = int(n_clips), int(n_noise_rows), int(noise_len), int(max_shift)
    if n < 0 or M < 1 or L < 1 or S < 0:
        raise ValueError(f"mix_plan needs n_clips >= 0, n_noise_rows >= 1, noise_len >= 1 and max_shift >= 0, got "
                         f"{n_clips}, {n_noise_rows}, {noise_len}, {max_shift}")
    rs = np.random.RandomState(int(seed))
    rows = rs.randint(0, M, size=n).astype(np.int32)
    offsets = rs.randint(0, L, size=n).astype(np.int32)
    shift = rs.randint(-S, S + 1, size=n).astype(np.int32)
    snr = _range_draw(snr_db, rs.random_sample(n), "snr_db")
    level = _range_draw(level_db, rs.random_sample(n), "level_db")
    snr_ratio(snr, n)                                            # refuses NaN and -inf
    return MixPlan(snr, rows, offsets, shift, (10.0 ** (level / 20.0)).astype(np.float32))


def snr_ratio(snr_db, n_clips: int) -> np.ndarray:
    """``10 ** (-snr_db / 10)`` per clip in float64, the ``ratio`` of SPEC.md §1.10: ``snr_db`` a number or ``n_clips`` of
    them; +inf means clean (ratio 0).  NaN, -inf and an SNR whose ratio overflows are refused."""
    snr = np.asarray(snr_db, dtype=np.float64)
    if snr.shape not in ((), (int(n_clips),)):
        raise ValueError(f"snr_db must be a number or {n_clips} of them, got shape {snr.shape}")
    with np.errstate(over="ignore"):
        ratio = np.float64(10.0) ** (-snr / 10.0)
    if np.isnan(snr).any() or not np.isfinite(ratio).all():
        raise ValueError(f"snr_db must be a number above -3000 dB or +inf (clean); NaN and -inf are refused, got {snr_db!r}")
    return np.broadcast_to(ratio, (int(n_clips),)).copy()


def _per_clip(value, n: int, dtype, name: str):
    """None, or a scalar or ``n`` values as a contiguous array of ``dtype``; integers must fit int32."""
    if value is None:
        return None
    if torch.is_tensor(value):
        value = value.cpu().numpy()
    v = np.asarray(value)
    if v.shape not in ((), (n,)):
        raise ValueError(f"{name} must be a number or {n} of them, got shape {v.shape}")
    if dtype == np.int32:
        if v.dtype.kind not in "iu" or (v < -2 ** 31).any() or (v >= 2 ** 31).any():
            raise ValueError(f"{name} must be integers that fit int32, got {value!r}")
    elif v.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be numbers, got {v.dtype}")
    return np.broadcast_to(v.astype(dtype), (n,)).copy()


def checked_noise_bank(noise_bank) -> torch.Tensor:
    """A noise bank as the mixer takes it: (M, L) float32 with M, L >= 1, NumPy (copied) or tensor; a 1-D array is one row."""
    if isinstance(noise_bank, np.ndarray):
        noise_bank = torch.from_numpy(np.array(noise_bank))
    if not torch.is_tensor(noise_bank) or noise_bank.dtype != torch.float32:
        raise ValueError("the noise bank must be a float32 NumPy array or tensor")
    if noise_bank.dim() == 1:
        noise_bank = noise_bank[None, :]
    if noise_bank.dim() != 2 or noise_bank.shape[0] < 1 or noise_bank.shape[1] < 1 or noise_bank.shape[1] >= 2 ** 31:
        raise ValueError(f"the noise bank must be (M, L) with M >= 1 and 1 <= L < 2^31, got {tuple(noise_bank.shape)}")
    return noise_bank.contiguous()


def mix_arguments(audio, snr_db, rows=None, offsets=None, shift=None, scale=None, out=None):
    """The arguments of `NoiseMixer.mix` checked on the host, before anything touches a device: ``(audio tensor, ratio,
    rows, offsets, shift, scale)``, the per-clip ones as host arrays (None where not given).  Raises ValueError."""
    if isinstance(audio, np.ndarray):
        if audio.dtype != np.float32:
            raise ValueError(f"audio must be float32, got {audio.dtype}")
        audio = torch.from_numpy(np.ascontiguousarray(audio))
    if not torch.is_tensor(audio) or audio.dtype != torch.float32 or audio.dim() != 2 or audio.shape[1] < 1 \
            or audio.shape[1] > MIX_MAX_SAMPLES:
        raise ValueError(f"audio must be (n, L) float32 with 1 <= L <= {MIX_MAX_SAMPLES}, NumPy or tensor, got "
                         f"{tuple(audio.shape) if hasattr(audio, 'shape') else type(audio).__name__}")
    audio = audio.contiguous()
    n = int(audio.shape[0])
    if out is not None:                 # its device is the mixer's to check (`NoiseMixer._mix`): nothing here knows one
        checked_out(out, audio.shape, None, audio, "a shift reads across what it would write")
    return (audio, snr_ratio(snr_db, n), _per_clip(rows, n, np.int32, "rows"), _per_clip(offsets, n, np.int32, "offsets"),
            _per_clip(shift, n, np.int32, "shift"), _per_clip(scale, n, np.float32, "scale"))


class NoiseMixer:
    """A noise bank ``(M, L)`` float32 on the device and the mixer kernels over it (SPEC.md §1.10): `mix` shifts, scales and
    adds a bank row at a requested SNR to every clip of a batch in one launch (`lsm_mix_f32`); `power` is the row power the
    SNR is defined with (`lsm_mix_power_f32`); `MixStream` is the streamed form."""

    def __init__(self, noise_bank, device=None):
        bank = checked_noise_bank(noise_bank)
        self.lib, self.device = _open(device)
        self.noise = bank.to(self.device)
        self.n_rows, self.noise_len = (int(v) for v in bank.shape)
        self._row_power = None

    def power(self, x) -> torch.Tensor:
        """``x`` (R, n) float32 -> the row powers P, float64 (R,) on the device."""
        x = as_float32(x)
        if x.dim() != 2 or x.shape[1] < 1 or x.shape[1] > MIX_MAX_SAMPLES:
            raise ValueError(f"x must be (R, n) with 1 <= n <= {MIX_MAX_SAMPLES}, got {tuple(x.shape)}")
        with torch.cuda.device(self.device):
            x = x.to(self.device)
            out = torch.empty(int(x.shape[0]), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.lsm_mix_power_f32(_dev(x), int(x.shape[0]), int(x.shape[1]), _dev(out),
                                                  _stream(self.device)), "lsm_mix_power_f32")
        return out

    @property
    def row_power(self) -> np.ndarray:
        """P of every bank row over its L samples, float64 on the host (computed once; the first use synchronises)."""
        if self._row_power is None:
            self._row_power = self.power(self.noise).cpu().numpy()
        return self._row_power

    def mix(self, audio, snr_db, rows=None, offsets=None, shift=None, scale=None, out=None, want_gain: bool = False):
        """``audio`` (n, L) float32, NumPy or tensor -> the corrupted clips, float32 (n, L) on the device.  Per clip (a number
        or n of them): ``snr_db`` (+inf = clean; NaN and -inf are refused), ``rows`` and ``offsets`` into the bank (a row
        outside the bank is clamped, an offset taken modulo the row length; the row wraps), ``shift`` in samples (zero
        filled, clamped to the clip) and ``scale``; None is 0, 0, 0 and 1.  ``out``: a caller-owned contiguous float32
        (n, L) tensor on the device, never ``audio``.  ``want_gain``: returns ``(out, gain (n), powers (n, 2))``, float64 on
        the device -- g and {Px, Pv} of SPEC.md §1.10."""
        return self._mix(audio, None, snr_db, rows, offsets, shift, scale, out, want_gain)

    def mix_ragged(self, x, lengths, snr_db, rows, offsets, shift, scale, out=None):
        """`mix` on rows of a stride whose clips have their own lengths (SPEC.md §1.16, `lsm_mix_ragged_f32`): ``x`` (n, L)
        float32, clip b is the first ``lengths[b]`` samples of its row -- an int32 device tensor (never read back) or a host
        sequence; the kernel clamps a length into [0, L] and the shift to the clip's own length, so a `mix_plan` drawn for the
        listing is taken as it is.  The SNR is that of the clip alone; what lies behind a clip influences nothing and comes
        back as +0.0.  Returns the float32 (n, L) tensor on the device (``out`` where given)."""
        n = len(x)
        # not `checked_lengths`: any int32 tensor goes as it is, a host sequence (or one number for every clip) has no range to
        # keep to -- the kernel clamps it -- and both keep the words they were always refused with
        if torch.is_tensor(lengths):
            if lengths.dtype != torch.int32 or tuple(lengths.shape) != (n,):
                raise ValueError(f"lengths must be an int32 ({n},) tensor or {n} host integers")
        else:
            lengths = torch.from_numpy(_per_clip(np.asarray(lengths), n, np.int32, "lengths"))
        return self._mix(x, lengths, snr_db, rows, offsets, shift, scale, out, False)

    def _mix(self, audio, lengths, snr_db, rows, offsets, shift, scale, out, want_gain):
        """`mix` (``lengths`` None: `lsm_mix_f32`) and `mix_ragged` (an int32 tensor: `lsm_mix_ragged_f32`)."""
        audio, ratio, rows, offsets, shift, scale = mix_arguments(audio, snr_db, rows, offsets, shift, scale, out)
        n, L = (int(v) for v in audio.shape)
        if out is not None and out.device != self.device:
            raise ValueError(f"out must be on {self.device}")
        with torch.cuda.device(self.device):
            audio = audio.to(self.device)
            if out is None:
                out = torch.empty((n, L), dtype=torch.float32, device=self.device)
            gain = torch.empty(n, dtype=torch.float64, device=self.device) if want_gain else None
            powers = torch.empty((n, 2), dtype=torch.float64, device=self.device) if want_gain else None
            args = [_up(a, self.device) for a in (rows, offsets, shift, scale, ratio)]
            if lengths is None:
                fn, name, head = self.lib.lsm_mix_f32, "lsm_mix_f32", [_dev(audio), n, L]
            else:
                lengths = lengths.to(self.device, non_blocking=True).contiguous()
                fn, name, head = self.lib.lsm_mix_ragged_f32, "lsm_mix_ragged_f32", [_dev(audio), n, L, _dev(lengths)]
            _lib.check(fn(*head, _dev(self.noise), self.n_rows, self.noise_len, *(_dev(a) for a in args), _dev(out), _dev(gain),
                          _dev(powers), _stream(self.device)), name)
        return (out, gain, powers) if want_gain else out


class MixStream(_StreamPush):
    """``n_streams`` open-ended streams through the mixer's streamed form (`lsm_mix_stream_f32`): every `push` scales each
    stream's new samples and adds the next samples of its noise row, from the position the bank holds -- a stream's whole
    state.  A stream cut into pushes anywhere gives, byte for byte, the samples of its uncut run.  A stream has no clip to
    take a power of, so `set` computes its gain on the host from the speech power the caller states.  Until `set`, a stream
    passes unchanged (gain 0, scale 1)."""

    def __init__(self, mixer: NoiseMixer, n_streams: int):
        self.mixer, self.n_streams, self.device = mixer, int(n_streams), mixer.device
        if self.n_streams < 1:
            raise ValueError(f"MixStream needs n_streams >= 1, got {n_streams}")
        self.pos = torch.zeros(self.n_streams, dtype=torch.int32, device=self.device)
        self.gain = torch.zeros(self.n_streams, dtype=torch.float64, device=self.device)
        self.scale = torch.ones(self.n_streams, dtype=torch.float32, device=self.device)
        self.rows = torch.zeros(self.n_streams, dtype=torch.int32, device=self.device)

    def set(self, slots, snr_db, speech_power, rows=0, scale=1.0) -> np.ndarray:
        """The corruption of the streams in ``slots`` from here on: ``speech_power`` is the mean square per sample of the
        stream as it arrives (before ``scale``), ``rows`` the bank row (refused outside the bank).  The gain is
        ``sqrt(scale^2 * speech_power * ratio / (P(row) / L))`` in float64 on the host, 0 for a clean stream or a silent
        row; it is returned.  The noise positions stay where they are."""
        slots = checked_slots(slots, self.n_streams)
        k, mixer = len(slots), self.mixer
        ratio = snr_ratio(snr_db, k)
        sp = _per_clip(speech_power, k, np.float64, "speech_power")
        rows = _per_clip(rows, k, np.int32, "rows")
        sc = _per_clip(scale, k, np.float32, "scale")
        if not (np.isfinite(sp).all() and (sp >= 0).all()):
            raise ValueError(f"speech_power must be finite and >= 0, got {speech_power!r}")
        if ((rows < 0) | (rows >= mixer.n_rows)).any():
            raise ValueError(f"rows {rows.tolist()} outside [0, {mixer.n_rows})")
        per_sample = mixer.row_power[rows] / mixer.noise_len
        noisy = (ratio > 0) & (per_sample > 0)
        a = sc.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            gain = np.where(noisy, np.sqrt(a * a * sp * ratio / np.where(noisy, per_sample, 1.0)), 0.0)
        at = torch.from_numpy(slots).to(self.device)
        self.gain[at] = torch.from_numpy(gain).to(self.device)
        self.scale[at] = torch.from_numpy(sc).to(self.device)
        self.rows[at] = torch.from_numpy(rows).to(self.device)
        return gain

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: their noise positions back to 0."""
        slots = checked_slots(slots, self.n_streams)
        self.pos[torch.from_numpy(slots).to(self.device)] = 0

    def push(self, audio, counts=None, out: torch.Tensor | None = None):
        """``audio`` (n_streams, H) float32: stream b's new samples are the first ``counts[b]`` of its row; ``counts``:
        n_streams host integers in [0, H], or None for H everywhere.  Returns ``(out, counts)``: float32 (n_streams, H) on
        the device, whose first ``counts[b]`` samples of row b are mixed; behind them lies what ``audio`` held, or what a
        caller-owned ``out`` held.  ``out`` may be ``audio`` (a device tensor): the mix is then in place."""
        audio = as_float32(audio)
        if audio.dim() != 2 or audio.shape[0] != self.n_streams or audio.shape[1] < 1 or audio.shape[1] > MIX_MAX_SAMPLES:
            raise ValueError(f"audio must be ({self.n_streams}, H) with 1 <= H <= {MIX_MAX_SAMPLES}, got {tuple(audio.shape)}")
        H = int(audio.shape[1])
        new = checked_counts(counts, self.n_streams, H, "counts")
        if out is not None:
            self._owned(out, (self.n_streams, H), torch.float32, "out", "float32")
        mixer = self.mixer
        with torch.cuda.device(self.device):
            if out is None:                                     # a copy of the rows, mixed in place
                out = audio.to(self.device, copy=True)
                audio = out
            else:
                audio = audio.to(self.device)
            cnt = self._count_array(counts, new)
            _lib.check(mixer.lib.lsm_mix_stream_f32(
                _dev(audio), self.n_streams, H, _dev(mixer.noise), mixer.n_rows, mixer.noise_len, _dev(cnt), _dev(self.gain),
                _dev(self.scale), _dev(self.rows), _dev(self.pos), _dev(self.pos), _dev(out), _stream(self.device)),
                "lsm_mix_stream_f32")
        return out, new


# ---- reverberation (SPEC.md §1.11, include/lsm_hip_reverb.h) ------------------------------------------------------------
REVERB_MAX_TAPS = 16384
REVERB_MAX_ROWS = 65535                 # rows of one launch
_REVERB_READS = "an output reads the samples in front of it"         # why ``out`` is never ``audio`` (`checked_out`)


class ReverbPlan(NamedTuple):
    """Per-clip rows of a bank of room impulse responses (`reverb_plan`): ``rows`` int32 on the host, -1 = a dry clip."""
    rows: np.ndarray

    part, take = _plan_part, _plan_take


def reverb_plan(n_clips: int, n_rir_rows: int, prob: float = 1.0, seed: int = 42) -> ReverbPlan:
    """The room of every clip of a listing, drawn from ``np.random.RandomState([seed, 1])`` -- a generator of its own, so
    `mix_plan`'s draws for the same seed stay as they are -- for ALL ``n_clips`` clips in listing order: the rows
    (``randint(0, M)``), then ``u = random_sample``; a clip with ``u >= prob`` is dry (row -1)."""
    n, M, p = int(n_clips), int(n_rir_rows), float(prob)
    if n < 0 or M < 1 or not 0.0 <= p <= 1.0:
        raise ValueError(f"reverb_plan needs n_clips >= 0, n_rir_rows >= 1 and prob in [0, 1], got {n_clips}, {n_rir_rows}, "
                         f"{prob}")
    rs = np.random.RandomState([int(seed), 1])
    rows = rs.randint(0, M, size=n).astype(np.int32)
    u = rs.random_sample(n)
    rows[u >= p] = -1
    return ReverbPlan(rows)


def checked_rir_bank(rir_bank, lengths=None):
    """A bank of impulse responses as the kernels take it: ``(bank (M, K) float32 tensor, lengths (M,) int32 array or
    None)`` with M >= 1 and 1 <= K <= 16384; a 1-D array is one row; ``lengths`` must lie in [1, K]."""
    if isinstance(rir_bank, np.ndarray):
        rir_bank = torch.from_numpy(np.array(rir_bank))
    if not torch.is_tensor(rir_bank) or rir_bank.dtype != torch.float32:
        raise ValueError("the bank of impulse responses must be a float32 NumPy array or tensor")
    if rir_bank.dim() == 1:
        rir_bank = rir_bank[None, :]
    if rir_bank.dim() != 2 or rir_bank.shape[0] < 1 or not 1 <= rir_bank.shape[1] <= REVERB_MAX_TAPS:
        raise ValueError(f"the bank of impulse responses must be (M, K) with M >= 1 and 1 <= K <= {REVERB_MAX_TAPS}, got "
                         f"{tuple(rir_bank.shape)}")
    M, K = (int(v) for v in rir_bank.shape)
    if lengths is not None:
        lengths = _per_clip(lengths, M, np.int32, "lengths")
        if ((lengths < 1) | (lengths > K)).any():
            raise ValueError(f"lengths must lie in [1, {K}], got {lengths.tolist()}")
    return rir_bank.contiguous(), lengths


def _reverb_audio(audio, n_rows=None, what="audio"):
    """(n, L) float32 with 1 <= L <= 2^24, NumPy (float32 only) or tensor -> contiguous tensor."""
    if isinstance(audio, np.ndarray):
        if audio.dtype != np.float32:
            raise ValueError(f"{what} must be float32, got {audio.dtype}")
        audio = torch.from_numpy(np.ascontiguousarray(audio))
    if not torch.is_tensor(audio) or audio.dtype != torch.float32 or audio.dim() != 2 or audio.shape[1] < 1 \
            or audio.shape[1] > MIX_MAX_SAMPLES or (n_rows is not None and audio.shape[0] != n_rows):
        raise ValueError(f"{what} must be ({'n' if n_rows is None else n_rows}, L) float32 with 1 <= L <= {MIX_MAX_SAMPLES}, "
                         f"NumPy or tensor, got {tuple(audio.shape) if hasattr(audio, 'shape') else type(audio).__name__}")
    return audio.contiguous()


class Reverberator:
    """A bank ``(M, K)`` float32 of room impulse responses on the device and the convolution kernels over it (SPEC.md
    §1.11): `reverb` convolves every clip of a batch with its row in one launch (`lsm_reverb_f32`); `ReverbStream` is the
    streamed form.  ``lengths`` (M integers in [1, K]) says where each row ends; None: K everywhere."""

    def __init__(self, rir_bank, lengths=None, device=None):
        bank, lengths = checked_rir_bank(rir_bank, lengths)
        self.lib, self.device = _open(device)
        self.rir = bank.to(self.device)
        self.n_rows, self.n_taps = (int(v) for v in bank.shape)
        self.lengths = lengths
        self.lengths_dev = None if lengths is None else torch.from_numpy(lengths).to(self.device)

    def reverb(self, audio, rows=None, n_out: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """``audio`` (n, L) float32, NumPy or tensor -> float32 (n, n_out) on the device.  ``rows``: a number or n of them
        (None: row 0); a row below 0 is dry -- the clip's bits -- and one at or above M is clamped.  ``n_out`` defaults to
        L, the recipe's ``convolve(x, h)[:L]``; ``L + K - 1`` is the full tail.  ``out``: a caller-owned contiguous
        float32 (n, n_out) tensor on the device, never ``audio``."""
        audio = _reverb_audio(audio)
        n, L = (int(v) for v in audio.shape)
        n_out = checked_n_out(n_out, L)
        rows = _per_clip(rows, n, np.int32, "rows")
        if out is not None:
            checked_out(out, (n, n_out), self.device, audio, _REVERB_READS)
        with torch.cuda.device(self.device):
            audio = audio.to(self.device)
            if out is None:
                out = torch.empty((n, n_out), dtype=torch.float32, device=self.device)
            rows_dev = _up(rows, self.device)
            stream = _stream(self.device)
            for r0, k in row_chunks(n, REVERB_MAX_ROWS):
                _lib.check(self.lib.lsm_reverb_f32(
                    _dev(audio, r0), k, L, _dev(self.rir), self.n_rows, self.n_taps, _dev(self.lengths_dev),
                    _dev(rows_dev, r0), n_out, _dev(out, r0), stream), "lsm_reverb_f32")
        return out


class ReverbStream(_StreamBank):
    """``n_streams`` open-ended streams through the reverberator's streamed form (`lsm_reverb_stream_f32`): every `push`
    convolves each stream's new samples -- any number, 0 included -- behind the history the bank holds, the stream's last
    K - 1 input samples.  A stream cut into pushes anywhere gives, byte for byte, the samples of its uncut run.  Until `set`,
    every stream uses row 0; row -1 is dry.  The history is kept at the bank's K, so `set` may change a stream's row between
    pushes."""

    def __init__(self, reverberator: Reverberator, n_streams: int):
        self.reverberator, self.n_streams, self.device = reverberator, int(n_streams), reverberator.device
        if self.n_streams < 1 or self.n_streams > REVERB_MAX_ROWS:
            raise ValueError(f"ReverbStream needs n_streams in [1, {REVERB_MAX_ROWS}], got {n_streams}")
        self._new_state(reverberator.lib.lsm_reverb_state_bytes(reverberator.n_taps))
        self.rows = torch.zeros(self.n_streams, dtype=torch.int32, device=self.device)

    def set(self, slots, rows) -> None:
        """The rows of the streams in ``slots`` from here on (below 0: dry; refused at or above M).  The histories stay."""
        slots = checked_slots(slots, self.n_streams)
        rows = _per_clip(rows, len(slots), np.int32, "rows")
        if (rows >= self.reverberator.n_rows).any():
            raise ValueError(f"rows {rows.tolist()} outside the bank's {self.reverberator.n_rows} rows")
        self.rows[torch.from_numpy(slots).to(self.device)] = torch.from_numpy(rows).to(self.device)

    def push(self, audio, counts=None, out: torch.Tensor | None = None):
        """``audio`` (n_streams, H) float32: stream b's new samples are the first ``counts[b]`` of its row; ``counts``:
        n_streams host integers in [0, H], or None for H everywhere.  Returns ``(out, counts)``: float32 (n_streams, H) on
        the device, whose first ``counts[b]`` samples of row b are the stream's next ones; behind them lie zeros, or what a
        caller-owned ``out`` held.  ``out`` is never ``audio``."""
        audio = _reverb_audio(audio, self.n_streams)
        H = int(audio.shape[1])
        new = checked_counts(counts, self.n_streams, H, "counts")
        rv = self.reverberator
        with torch.cuda.device(self.device):
            out = self._owned(out, (self.n_streams, H), torch.float32, "out", "float32", audio, _REVERB_READS)
            audio = audio.to(self.device)
            cnt = self._count_array(counts, new)
            _lib.check(rv.lib.lsm_reverb_stream_f32(
                _dev(audio), self.n_streams, H, _dev(rv.rir), rv.n_rows, rv.n_taps, _dev(rv.lengths_dev), _dev(self.rows),
                _dev(cnt), _dev(self.state), _dev(self.state), _dev(out), _stream(self.device)), "lsm_reverb_stream_f32")
        return out, new


# ---- speed perturbation (SPEC.md §1.12, include/lsm_hip_speed.h) --------------------------------------------------------
SPEED_MAX_DESIGNS = 16
SPEED_MAX_ROWS = 65535                  # rows of one launch
_SPEED_READS = "an output reads the samples around it"              # why ``out`` is never ``audio`` (`checked_out`)


def _speed_fraction(factor) -> Fraction:
    """A speed factor as an exact fraction: an int, a Fraction, a string such as "11/10" or "1.1"; a float through its
    shortest decimal form (``Fraction(str(x))``: 1.1 is 11/10, not the binary value next to it)."""
    if isinstance(factor, bool):
        raise ValueError(f"a speed factor must be a number or a string, got {factor!r}")
    try:
        if isinstance(factor, (float, np.floating)):
            return Fraction(str(float(factor)))
        if isinstance(factor, (int, np.integer)):
            return Fraction(int(factor))
        if isinstance(factor, (Fraction, str)):
            return Fraction(factor)
    except (ValueError, ZeroDivisionError, OverflowError) as e:
        raise ValueError(f"{factor!r} is no speed factor: {e}") from None
    raise ValueError(f"a speed factor must be an int, a Fraction, a float or a string, got {type(factor).__name__}")


def speed_design(factor) -> ResampleTable | None:
    """The design of playing a clip ``factor`` times faster (SPEC.md §1.12): ``resample_table(int(16000 * factor), 16000)``,
    or None for 1, the identity.  ``factor`` must lie in [1/2, 2] and make ``16000 * factor`` an integer rate."""
    s = _speed_fraction(factor)
    if not Fraction(1, 2) <= s <= 2:
        raise ValueError(f"speed factor {factor!r} outside [1/2, 2]")
    rate = SAMPLE_RATE * s
    if rate.denominator != 1:
        raise ValueError(f"speed factor {factor!r}: {SAMPLE_RATE} * factor = {float(rate):.6g} is no integer sample rate")
    return None if s == 1 else resample_table(int(rate), SAMPLE_RATE)


class SpeedPlan(NamedTuple):
    """Per-clip choices among a list of speed factors (`speed_plan`): ``choice`` int32 on the host, an index into the list,
    -1 = an unperturbed clip."""
    choice: np.ndarray

    part, take = _plan_part, _plan_take


def speed_plan(n_clips: int, n_factors: int, prob: float = 1.0, seed: int = 42) -> SpeedPlan:
    """The speed of every clip of a listing, drawn from ``np.random.RandomState([seed, 2])`` -- a generator of its own, so
    `mix_plan`'s and `reverb_plan`'s draws for the same seed stay as they are -- for ALL ``n_clips`` clips in listing order:
    the choices (``randint(0, n_factors)``), then ``u = random_sample``; a clip with ``u >= prob`` is unperturbed (-1)."""
    n, M, p = int(n_clips), int(n_factors), float(prob)
    if n < 0 or M < 1 or not 0.0 <= p <= 1.0:
        raise ValueError(f"speed_plan needs n_clips >= 0, n_factors >= 1 and prob in [0, 1], got {n_clips}, {n_factors}, "
                         f"{prob}")
    rs = np.random.RandomState([int(seed), 2])
    choice = rs.randint(0, M, size=n).astype(np.int32)
    u = rs.random_sample(n)
    choice[u >= p] = -1
    return SpeedPlan(choice)


def speed_bank(factors):
    """``factors`` -> ``(tables, row_of_choice)``: the designs of the non-unit factors in the list's order (`speed_design`,
    at most 16, all distinct) and, per factor, its row among them as int32, -1 for a unit factor."""
    factors = list(factors)
    if not factors:
        raise ValueError("a list of speed factors must name at least one")
    seen, tables, row_of_choice = {}, [], []
    for f in factors:
        s = _speed_fraction(f)
        if s in seen:
            raise ValueError(f"speed factor {f!r} is named twice")
        table = speed_design(f)
        seen[s] = -1 if table is None else len(tables)
        row_of_choice.append(seen[s])
        if table is not None:
            tables.append(table)
    if len(tables) > SPEED_MAX_DESIGNS:
        raise ValueError(f"{len(tables)} speed factors other than 1: one launch serves at most {SPEED_MAX_DESIGNS} designs")
    return tables, np.asarray(row_of_choice, dtype=np.int32)


class SpeedPerturber:
    """Clips played at per-clip speeds in one launch (`lsm_speed_f32`, SPEC.md §1.12).  ``factors``: the speeds a plan's
    choices index (`speed_design`), up to 16 distinct ones other than 1 and at least one; a factor of 1 maps to row -1, the
    unperturbed copy.  ``tables`` are the designs, ``designs`` their (n, 5) int32 rows of up, down, n_taps, delay and
    tap_offset on the host, ``taps_dev`` their taps one behind the other on the device, ``row_of_choice`` the design row of
    every factor."""

    def __init__(self, factors, device=None):
        self.factors = list(factors)
        self.tables, self.row_of_choice = speed_bank(self.factors)
        if not self.tables:
            raise ValueError("every speed factor is 1: there is nothing to perturb")
        offsets = np.cumsum([0] + [len(t.taps) for t in self.tables])
        self.designs = np.ascontiguousarray(
            [[t.up, t.down, len(t.taps), t.delay, int(o)] for t, o in zip(self.tables, offsets)], dtype=np.int32)
        self.n_taps_total = int(offsets[-1])
        self.lib, self.device = _open(device)
        self.taps_dev = torch.from_numpy(np.concatenate([t.taps for t in self.tables])).to(self.device)
        self.lds_bytes = int(self.lib.lsm_speed_lds_bytes(_host(self.designs), len(self.designs)))

    def rows_of(self, choice, n: int):
        """``choice`` (a number or ``n`` of them, indices into ``factors``, below 0 = unperturbed; None: factor 0
        everywhere) -> the design rows as int32, or None where every clip takes row 0."""
        if choice is None:
            return None if self.row_of_choice[0] == 0 else np.full(n, self.row_of_choice[0], dtype=np.int32)
        choice = _per_clip(choice, n, np.int32, "choice")
        if (choice >= len(self.factors)).any():
            raise ValueError(f"choice {choice.tolist()} outside the {len(self.factors)} speed factors")
        return np.where(choice < 0, np.int32(-1), self.row_of_choice[np.maximum(choice, 0)]).astype(np.int32)

    def perturb(self, audio, choice=None, n_out: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """``audio`` (n, L) float32 or int16, NumPy or tensor -> float32 (n, n_out) on the device, clip c played at
        ``factors[choice[c]]`` (`rows_of`).  ``n_out`` defaults to L: a faster clip is padded with what the filter rings
        out and zeros, a slower one trimmed, to the clip length.  ``out``: a caller-owned contiguous float32 (n, n_out)
        tensor on the device, never ``audio``."""
        audio, fmt = checked_pcm(audio)
        n, L = (int(v) for v in audio.shape)
        n_out = checked_n_out(n_out, L)
        rows = self.rows_of(choice, n)
        if out is not None:
            checked_out(out, (n, n_out), self.device, audio, _SPEED_READS)
        with torch.cuda.device(self.device):
            audio = audio.to(self.device)
            if out is None:
                out = torch.empty((n, n_out), dtype=torch.float32, device=self.device)
            rows_dev = _up(rows, self.device)
            stream = _stream(self.device)
            for r0, k in row_chunks(n, SPEED_MAX_ROWS):
                _lib.check(self.lib.lsm_speed_f32(
                    _dev(audio, r0), fmt, k, L, _dev(self.taps_dev), self.n_taps_total, _host(self.designs),
                    len(self.designs), _dev(rows_dev, r0), n_out, _dev(out, r0), stream), "lsm_speed_f32")
        return out

    def perturb_ragged(self, audio, lengths, choice=None, n_out: int | None = None, time_bins: int | None = None,
                       out: torch.Tensor | None = None):
        """`perturb` on rows of one stride whose clips have their own lengths (`lsm_speed_ragged_f32`, SPEC.md §1.18):
        ``audio`` (n, L) float32 or int16, clip b its first ``lengths[b]`` samples -- n host integers in [0, L] (checked) or
        an int32 device tensor (not read: the kernel clamps it).  -> ``(rows, samples, bins)``, device tensors produced on
        the current stream with no host synchronisation: ``rows`` float32 (n, n_out) -- ``out`` where given -- holds clip b
        played at ``factors[choice[b]]`` as the clip alone, ``samples[b]`` = min(ceil(lengths[b] * up / down), n_out) samples
        of it (`speed_ragged_lengths` gives the same integers on the host) and +0.0 behind: no ring-out tail, and a slowed
        clip that outgrows the row is cut; ``samples`` and ``bins`` = min(ceil(samples / 160), time_bins) are int32 (n,),
        what `NoiseMixer.mix_ragged`, `SilenceTrimmer.trim` and `SpikeFrontEnd.encode_ragged`, `pipeline.step_fused_ragged`,
        `SNN.run_batch(lengths=...)` take unread.  ``n_out`` defaults to L, ``time_bins`` (>= 3, with
        160 * time_bins <= n_out) to n_out // 160."""
        audio, fmt = checked_pcm(audio)
        n, L = (int(v) for v in audio.shape)
        n_out = checked_n_out(n_out, L)
        time_bins = n_out // RAGGED_HOP if time_bins is None else int(time_bins)
        if time_bins < RAGGED_MIN_BINS or RAGGED_HOP * time_bins > n_out:
            raise ValueError(f"time_bins = {time_bins}: a row of n_out = {n_out} samples holds {RAGGED_MIN_BINS} .. "
                             f"{n_out // RAGGED_HOP} time bins of {RAGGED_HOP}")
        rows = self.rows_of(choice, n)
        lengths = checked_lengths(lengths, n, L, None)          # refused here, uploaded below
        if out is not None:
            checked_out(out, (n, n_out), self.device, audio, _SPEED_READS)
        with torch.cuda.device(self.device):
            audio = audio.to(self.device)
            lengths = lengths.to(self.device, non_blocking=True).contiguous()
            if out is None:
                out = torch.empty((n, n_out), dtype=torch.float32, device=self.device)
            samples = torch.empty((n,), dtype=torch.int32, device=self.device)
            bins = torch.empty((n,), dtype=torch.int32, device=self.device)
            rows_dev = _up(rows, self.device)
            stream = _stream(self.device)
            for r0, k in row_chunks(n, SPEED_MAX_ROWS):
                _lib.check(self.lib.lsm_speed_ragged_f32(
                    _dev(audio, r0), fmt, k, L, _dev(lengths, r0), _dev(self.taps_dev), self.n_taps_total, _host(self.designs),
                    len(self.designs), _dev(rows_dev, r0), n_out, _dev(out, r0), _dev(samples, r0), _dev(bins, r0), time_bins,
                    stream), "lsm_speed_ragged_f32")
        return out, samples, bins


def speed_ragged_lengths(lengths, choice, perturber, n_out: int) -> np.ndarray:
    """The sample counts `SpeedPerturber.perturb_ragged` writes, computed on the host (`lsm_speed_ragged_length`, the one
    function the kernel calls): ``lengths`` n host integers (below 0 counts as 0), ``choice`` as `SpeedPerturber.rows_of`
    takes it, ``perturber`` the `SpeedPerturber` (only its designs are read), ``n_out`` the samples of an output row ->
    int64 (n,): min(ceil(lengths * up / down), n_out), up = down = 1 for an unperturbed clip."""
    arr = np.asarray(lengths)
    if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"lengths must be a 1-D sequence of integers, got {arr.dtype} {arr.shape}")
    if len(arr) and (arr.max() > np.iinfo(np.int32).max or arr.min() < np.iinfo(np.int32).min):
        raise ValueError("lengths must fit int32")
    n_out = int(n_out)
    if not 0 <= n_out <= np.iinfo(np.int32).max:
        raise ValueError(f"n_out must lie in [0, 2^31), got {n_out}")
    rows = perturber.rows_of(choice, len(arr))
    rows = np.zeros(len(arr), dtype=np.int32) if rows is None else rows
    lib = _lib.load()
    new = np.empty(len(arr), dtype=np.int64)
    for b, (n_b, r) in enumerate(zip(arr.tolist(), rows.tolist())):
        up, down = (1, 1) if r < 0 else (int(v) for v in perturber.designs[min(r, len(perturber.designs) - 1), :2])
        new[b] = lib.lsm_speed_ragged_length(int(n_b), up, down, n_out)
        if new[b] < 0:
            _lib.check(int(new[b]), "lsm_speed_ragged_length")
    return new


# ---- silence trimming in front of the ragged front end (SPEC.md §1.15, include/lsm_hip_trim.h) ---------------------------
TRIM_MAX_BINS = 4096        # time_bins of a trim launch: 3 .. 4096


def trim_ratio(top_db) -> float:
    """The activity threshold of `lsm_trim_silence_f32` as a share of a clip's loudest bin: ``10 ** (-top_db / 10)`` for a
    bin ``top_db`` dB (> 0, finite) under the loudest, 0.0 for None: only bins of exact zeros count as silence."""
    if top_db is None:
        return 0.0
    top_db = float(top_db)
    if not (np.isfinite(top_db) and top_db > 0.0):
        raise ValueError(f"top_db must be a finite number of dB above 0, or None, got {top_db!r}")
    return 10.0 ** (-top_db / 10.0)


class SilenceTrimmer:
    """Clips cut to their speech on the device (`lsm_trim_silence_f32`, SPEC.md §1.15): per clip the energies of its
    160-sample bins, the span of the bins louder than ``ratio`` times the loudest, ``pad_bins`` bins kept on either side
    and at least ``min_bins`` (>= 3) bins in all; the span's samples move to the start of the clip's row.  ``top_db``: the
    threshold in dB under the loudest bin (`trim_ratio`); None trims digital silence only."""

    def __init__(self, top_db=30.0, pad_bins: int = 3, min_bins: int = 3, device=None):
        self.top_db = top_db
        self.ratio = trim_ratio(top_db)
        self.pad_bins, self.min_bins = int(pad_bins), int(min_bins)
        if self.pad_bins < 0:
            raise ValueError(f"pad_bins must be >= 0, got {pad_bins}")
        if not RAGGED_MIN_BINS <= self.min_bins <= TRIM_MAX_BINS:
            raise ValueError(f"min_bins must lie in [{RAGGED_MIN_BINS}, {TRIM_MAX_BINS}], got {min_bins}")
        self.lib, self.device = _open(device)

    def trim(self, audio, lengths=None, time_bins: int | None = None, out: torch.Tensor | None = None,
             want_energy: bool = False):
        """``audio`` (n, L) float32, NumPy or tensor -> ``(audio_out, bins, first[, energy])``, device tensors produced on
        the current stream with no host synchronisation.  ``lengths``: the clips' valid samples, n host integers in
        [0, L] (checked) or an int32 device tensor (not read: the kernel clamps it); None: L everywhere.  ``time_bins``
        (3 .. 4096): the bins of a row, ceil(L / 160) by default.  ``audio_out`` float32 (n, 160 * time_bins) -- or ``out``,
        a caller-owned contiguous float32 (n, >= 160 * time_bins) tensor on the device, never ``audio`` -- holds clip b's
        span at the start of row b and +0.0 behind; ``bins`` and ``first`` int32 (n,): the span's bins, which
        `SpikeFrontEnd.encode_ragged`, `pipeline.step_fused_ragged` and `SNN.run_batch(lengths=...)` take unread, and its
        first bin in the clip; ``energy`` float64 (n, time_bins): the bin energies, +0.0 behind a clip's last bin."""
        audio = as_float32(audio)
        if audio.ndim != 2 or audio.shape[1] < 1:
            raise ValueError(f"audio must be (n, L >= 1), got {tuple(audio.shape)}")
        n, L = (int(v) for v in audio.shape)
        time_bins = -(-L // RAGGED_HOP) if time_bins is None else int(time_bins)
        if not RAGGED_MIN_BINS <= time_bins <= TRIM_MAX_BINS:
            raise ValueError(f"time_bins = {time_bins} outside [{RAGGED_MIN_BINS}, {TRIM_MAX_BINS}]")
        if self.min_bins > time_bins:
            raise ValueError(f"min_bins = {self.min_bins} exceeds the row's {time_bins} time bins")
        if out is not None:
            checked_out(out, (n, RAGGED_HOP * time_bins), self.device, audio, "a clip moves towards the start of its row",
                        at_least=True)                                  # a wider row is welcome: the kernel takes its stride
        with torch.cuda.device(self.device):
            audio = audio.to(self.device).contiguous()
            counts = None if lengths is None else checked_lengths(lengths, n, L, self.device)
            if out is None:
                out = torch.empty((n, RAGGED_HOP * time_bins), dtype=torch.float32, device=self.device)
            bins = torch.empty((n,), dtype=torch.int32, device=self.device)
            first = torch.empty((n,), dtype=torch.int32, device=self.device)
            energy = torch.empty((n, time_bins), dtype=torch.float64, device=self.device) if want_energy else None
            if n:
                _lib.check(self.lib.lsm_trim_silence_f32(
                    _dev(audio), n, L, time_bins, _dev(counts), C.c_double(self.ratio), self.pad_bins, self.min_bins, _dev(out),
                    int(out.shape[1]), _dev(first), _dev(bins), _dev(energy), _stream(self.device)), "lsm_trim_silence_f32")
        return (out, bins, first, energy) if want_energy else (out, bins, first)


# ---- stream endpointing in front of the ragged launches (SPEC.md §1.17, include/lsm_hip_endpoint.h) ----------------------
ENDPOINT_MAX_HOPS = 4096        # hops of one push
ENDPOINT_MAX_WINDOW = 1024      # window_bins and hang_bins: up to 1024
ENDPOINT_MAX_BINS = 4096        # max_bins: 3 .. 4096
ENDPOINT_CUT, ENDPOINT_FLUSHED = 1, 2       # bits of an utterance's flags


def endpoint_floor(floor_db) -> float:
    """The absolute activity floor of `lsm_endpoint_stream_f32` as a bin energy: ``160 * 10 ** (floor_db / 10)``, the energy of
    a bin of 160 samples at ``floor_db`` dB relative to full scale (finite), 0.0 for None: no floor."""
    if floor_db is None:
        return 0.0
    floor_db = float(floor_db)
    if not np.isfinite(floor_db):
        raise ValueError(f"floor_db must be a finite number of dB, or None, got {floor_db!r}")
    return RAGGED_HOP * 10.0 ** (floor_db / 10.0)


def endpoint_max_utterances(n_hops: int, pad_bins: int, hang_bins: int, max_bins: int) -> int:
    """The slots per stream no push of ``n_hops`` hops can exceed: ``2 + (n_hops - 1) / d``, d the fewest bins between the
    closes of two kept utterances -- ``min(hang_bins + 1, max_bins)``, `lsm_endpoint_max_utterances`' divisor, and where
    ``max_bins >= hang_bins + 3`` also ``max(max_bins - pad_bins, max_bins + pad_bins - hang_bins)``: a forced cut behind a
    close by silence starts ``hang_bins - pad_bins`` bins before that close (SPEC.md §1.17).  Host integers only."""
    H, P, G, M = int(n_hops), int(pad_bins), int(hang_bins), int(max_bins)
    d = min(G + 1, M)
    if G + 3 <= M:
        d = min(d, max(M - P, M + P - G))
    return 2 + (H - 1) // d


class Utterances(NamedTuple):
    """What one `EndpointStream.push` emitted, device tensors: ``audio`` float32 (n_streams * max_utts, 160 * max_bins), slot
    ``b * max_utts + u`` holding stream b's u-th utterance of the push at its start and +0.0 behind; ``bins`` int32
    (n_streams * max_utts,): its bins, 0 for an empty slot; ``first`` int64 and ``flags`` int32 of the same shape: its first
    bin on the stream's timeline and `ENDPOINT_CUT` / `ENDPOINT_FLUSHED` (empty slots: unspecified); ``count`` int32
    (n_streams,): the emitted slots per stream."""
    audio: torch.Tensor
    bins: torch.Tensor
    first: torch.Tensor
    flags: torch.Tensor
    count: torch.Tensor


class EndpointStream(_StreamBank):
    """``n_streams`` open-ended audio streams cut into utterances on the device (`lsm_endpoint_stream_f32`, SPEC.md §1.17).
    A bin of 160 samples is active when its energy exceeds ``top_db`` dB under the loudest of the last ``window_bins`` bins and
    ``floor_db`` dB relative to full scale; an utterance opens ``pad_bins`` bins before an active bin, closes ``pad_bins`` bins
    behind the last active one once ``hang_bins`` quiet bins have followed it, is cut at ``max_bins`` bins, and is dropped as
    a click when its active span has fewer than ``min_span_bins`` bins.  Every ``push`` advances each stream by the whole hops
    it delivers from the state the bank holds; a stream cut into pushes at any hop boundaries emits, byte for byte, the
    utterances of its uncut run.  The slots of a push are a ragged batch: `SpikeFrontEnd.encode_ragged`,
    `pipeline.step_fused_ragged` and `SNN.run_batch(lengths=...)` take ``audio`` and ``bins`` unread."""

    def __init__(self, n_streams: int, top_db=30.0, floor_db=-60.0, window_bins: int = 100, pad_bins: int = 3,
                 hang_bins: int = 20, min_span_bins: int = 3, max_bins: int = 100, device=None):
        self.n_streams = int(n_streams)
        self.top_db, self.floor_db = top_db, floor_db
        self.ratio, self.floor = trim_ratio(top_db), endpoint_floor(floor_db)
        self._window_bins, self.pad_bins, self.hang_bins = int(window_bins), int(pad_bins), int(hang_bins)
        self.min_span_bins, self._max_bins = int(min_span_bins), int(max_bins)
        W, P, G, A, M = self.window_bins, self.pad_bins, self.hang_bins, self.min_span_bins, self.max_bins
        if self.n_streams < 1:
            raise ValueError(f"EndpointStream needs n_streams >= 1, got {n_streams}")
        if not 1 <= W <= ENDPOINT_MAX_WINDOW:
            raise ValueError(f"window_bins must lie in [1, {ENDPOINT_MAX_WINDOW}], got {window_bins}")
        if not RAGGED_MIN_BINS <= M <= ENDPOINT_MAX_BINS:
            raise ValueError(f"max_bins must lie in [{RAGGED_MIN_BINS}, {ENDPOINT_MAX_BINS}], got {max_bins}")
        if not 0 <= P < M:
            raise ValueError(f"pad_bins must lie in [0, max_bins = {M}), got {pad_bins}")
        if not max(P, 1) <= G <= ENDPOINT_MAX_WINDOW:
            raise ValueError(f"hang_bins must lie in [max(pad_bins, 1) = {max(P, 1)}, {ENDPOINT_MAX_WINDOW}], got {hang_bins}")
        if not RAGGED_MIN_BINS <= A <= M:
            raise ValueError(f"min_span_bins must lie in [{RAGGED_MIN_BINS}, max_bins = {M}], got {min_span_bins}")
        self.lib, self.device = _open(device)
        self._new_state(self.lib.lsm_endpoint_state_bytes(W, M))
        self._outputs = {}                                              # per n_hops: the slot buffers of a push

    # a state block means what it says only under the window_bins and max_bins it was made with: read-only
    @property
    def window_bins(self) -> int:
        return self._window_bins

    @property
    def max_bins(self) -> int:
        return self._max_bins

    @property
    def params(self) -> dict:
        """The rule's parameters: what a second `EndpointStream` needs to cut the same utterances."""
        return dict(top_db=self.top_db, floor_db=self.floor_db, window_bins=self.window_bins, pad_bins=self.pad_bins,
                    hang_bins=self.hang_bins, min_span_bins=self.min_span_bins, max_bins=self.max_bins)

    def max_utterances(self, n_hops: int) -> int:
        """Slots per stream of a push of ``n_hops`` hops (`endpoint_max_utterances`; never below the library's figure)."""
        return max(endpoint_max_utterances(n_hops, self.pad_bins, self.hang_bins, self.max_bins),
                   int(self.lib.lsm_endpoint_max_utterances(int(n_hops), self.hang_bins, self.max_bins)))

    def _counts(self, values, n_hops: int, what: str):
        """``hops`` / ``finish`` as the int32 device tensor the kernel reads, or None: host integers checked, a device tensor
        taken as it is -- never read back, the kernel clamps it."""
        if values is None:
            return None
        n = self.n_streams
        if torch.is_tensor(values) and values.is_cuda:
            if values.dtype != torch.int32 or tuple(values.shape) != (n,):
                raise ValueError(f"{what} must hold {n} int32 values, got {values.dtype} {tuple(values.shape)}")
            return values.to(self.device).contiguous()
        arr = np.asarray(values.numpy() if torch.is_tensor(values) else values)
        if arr.dtype == np.bool_:
            arr = arr.astype(np.int64)
        if arr.shape != (n,) or arr.dtype.kind not in "iu" or (arr < 0).any() or (arr > n_hops).any():
            raise ValueError(f"{what} must be {n} integers in [0, {n_hops}], got {values!r}")
        return torch.from_numpy(arr.astype(np.int32)).to(self.device, non_blocking=True)

    def push(self, audio, hops=None, finish=None) -> Utterances:
        """``audio`` (n_streams, H * 160) float32, NumPy or tensor, 1 <= H <= 4096: stream b's new samples are the first
        ``hops[b] * 160`` of its row.  ``hops``: n_streams host integers in [0, H] (checked) or an int32 device tensor (not
        read: the kernel clamps it); None: H everywhere.  ``finish``: n_streams flags, host or device, non-zero where the stream
        ends behind this push's hops -- an open utterance is flushed and the stream starts afresh; None: no stream ends.
        Returns `Utterances`, device tensors produced on the current stream with NO host synchronisation.  The buffers belong
        to the bank, one set per H: the next push of the same H overwrites them."""
        audio = as_float32(audio)
        if audio.dim() != 2 or audio.shape[0] != self.n_streams or audio.shape[1] % RAGGED_HOP or audio.shape[1] < RAGGED_HOP \
                or audio.shape[1] > ENDPOINT_MAX_HOPS * RAGGED_HOP:
            raise ValueError(f"audio must be ({self.n_streams}, H * {RAGGED_HOP}) with 1 <= H <= {ENDPOINT_MAX_HOPS}, got "
                             f"{tuple(audio.shape)}")
        H = int(audio.shape[1]) // RAGGED_HOP
        n, M = self.n_streams, self.max_bins
        with torch.cuda.device(self.device):
            audio = audio.to(self.device).contiguous()
            counts = self._counts(hops, H, "hops")
            ends = self._counts(finish, 1, "finish")
            out = self._outputs.get(H)
            if out is None:
                U = self.max_utterances(H)
                out = self._outputs[H] = Utterances(
                    torch.zeros((n * U, RAGGED_HOP * M), dtype=torch.float32, device=self.device),
                    torch.zeros((n * U,), dtype=torch.int32, device=self.device),
                    torch.zeros((n * U,), dtype=torch.int64, device=self.device),
                    torch.zeros((n * U,), dtype=torch.int32, device=self.device),
                    torch.zeros((n,), dtype=torch.int32, device=self.device))
            U = int(out.bins.shape[0]) // n
            _lib.check(self.lib.lsm_endpoint_stream_f32(
                _dev(audio), n, H, _dev(counts), _dev(ends), C.c_double(self.ratio), C.c_double(self.floor), self.window_bins,
                self.pad_bins, self.hang_bins, self.min_span_bins, M, _dev(self.state), _dev(self.state), U, _dev(out.audio),
                _dev(out.bins), _dev(out.first), _dev(out.flags), _dev(out.count), None, None, _stream(self.device)),
                "lsm_endpoint_stream_f32")
        return out


# ---- SpecAugment-style masks inside the spike encoders (SPEC.md §1.13, include/lsm_hip_mask.h) ---------------------------

def mask_words(starts, widths, n_bits: int) -> np.ndarray:
    """Bands -> mask words: ``starts`` and ``widths`` are ``(n_clips, k)`` integers (k bands per clip, a width of 0 is no
    band); returns ``(n_clips, ceil(n_bits / 32))`` uint32 with bit ``i & 31`` of word ``i >> 5`` set where a band of the clip
    covers index ``i``.  Every band must lie inside ``[0, n_bits)``."""
    starts, widths = np.asarray(starts), np.asarray(widths)
    if starts.ndim != 2 or starts.shape != widths.shape or starts.dtype.kind not in "iu" or widths.dtype.kind not in "iu":
        raise ValueError(f"starts and widths must be integer arrays of one (n_clips, k) shape, got {starts.shape}, {widths.shape}")
    n_bits = int(n_bits)
    if n_bits < 1:
        raise ValueError(f"n_bits must be >= 1, got {n_bits}")
    starts, widths = starts.astype(np.int64), widths.astype(np.int64)
    if (starts < 0).any() or (widths < 0).any() or (starts + widths > n_bits).any():
        raise ValueError(f"a band lies outside [0, {n_bits})")
    i = np.arange(n_bits, dtype=np.int64)
    bits = ((i >= starts[:, :, None]) & (i < (starts + widths)[:, :, None])).any(axis=1)        # (n_clips, n_bits)
    n_words = (n_bits + 31) // 32
    padded = np.zeros((len(starts), n_words * 32), dtype=np.uint64)
    padded[:, :n_bits] = bits
    return (padded.reshape(len(starts), n_words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


class MaskPlan(NamedTuple):
    """Per-clip frequency and time masks (`mask_plan`, `mask_words`), host arrays of uint32 words, one row per clip: ``freq``
    ``(n, ceil(n_filters / 32))`` over the filter rows before redundancy, ``time`` ``(n, ceil(time_bins / 32))`` over the
    time bins."""
    freq: np.ndarray
    time: np.ndarray

    part, take = _plan_part, _plan_take


def mask_plan(n_clips: int, n_filters: int, time_bins: int, freq_masks: int = 0, freq_width: int = 0, time_masks: int = 0,
              time_width: int = 0, prob: float = 1.0, seed: int = 42) -> MaskPlan:
    """The masks of every clip of a listing, drawn from ``np.random.RandomState([seed, 3])`` -- a generator of its own, so
    `mix_plan`'s, `reverb_plan`'s and `speed_plan`'s draws for the same seed stay as they are -- for ALL ``n_clips`` clips in
    listing order.  The draws, in this order: (1) the frequency widths, ``randint(0, freq_width + 1, (n, freq_masks))``;
    (2) the frequency positions, ``floor(random_sample((n, freq_masks)) * (n_filters - width + 1))``; (3) the time widths,
    ``randint(0, time_width + 1, (n, time_masks))``, and (4) the time positions, ``floor(random_sample((n, time_masks)) *
    (time_bins - width + 1))``; (5) ``u = random_sample(n)``: a clip with ``u >= prob`` gets no mask.  Band ``k`` of a clip
    covers ``[position, position + width)``."""
    return _drawn_masks(n_clips, n_filters, time_bins, None, freq_masks, freq_width, time_masks, time_width, prob, seed)


def mask_plan_ragged(bins, n_filters: int, time_bins: int, freq_masks: int = 0, freq_width: int = 0, time_masks: int = 0,
                     time_width: int = 0, prob: float = 1.0, seed: int = 42) -> MaskPlan:
    """`mask_plan` for a listing whose clip b has ``bins[b]`` of the launch's ``time_bins`` bins (SPEC.md §1.16): the same
    generator, the same five draws in the same order, the words at the launch's strides.  Only the time bands differ: a
    band of drawn width ``w`` covers ``w_eff = min(w, T_b)`` bins from ``floor(u * (T_b - w_eff + 1))``, so every band lies
    inside the clip's own bins; a clip of 0 bins gets no time bits.  With every ``bins[b] == time_bins`` the plan is
    `mask_plan`'s, word for word."""
    bins = np.asarray(bins)
    if bins.ndim != 1 or bins.dtype.kind not in "iu" or (bins < 0).any() or (bins > int(time_bins)).any():
        raise ValueError(f"bins must be a 1-D integer array with every entry in [0, {time_bins}]")
    return _drawn_masks(len(bins), n_filters, time_bins, bins.astype(np.int64), freq_masks, freq_width, time_masks, time_width,
                        prob, seed)


def _drawn_masks(n_clips, n_filters, time_bins, bins, freq_masks, freq_width, time_masks, time_width, prob, seed) -> MaskPlan:
    """`mask_plan` (``bins`` None) and `mask_plan_ragged`: one copy of the refusals and the draws."""
    n, F, Tb, p = int(n_clips), int(n_filters), int(time_bins), float(prob)
    nf, wf, nt, wt = int(freq_masks), int(freq_width), int(time_masks), int(time_width)
    if n < 0 or F < 1 or Tb < 1 or nf < 0 or nt < 0 or wf < 0 or wt < 0 or not 0.0 <= p <= 1.0:
        raise ValueError(f"mask_plan needs n_clips >= 0, n_filters and time_bins >= 1, counts and widths >= 0 and prob in "
                         f"[0, 1], got {n_clips}, {n_filters}, {time_bins}, {freq_masks}, {freq_width}, {time_masks}, "
                         f"{time_width}, {prob}")
    if wf > F or wt > Tb:
        raise ValueError(f"a mask cannot be wider than its axis: freq_width {wf} of {F} filters, time_width {wt} of {Tb} bins")
    rs = np.random.RandomState([int(seed), 3])
    f_w = rs.randint(0, wf + 1, size=(n, nf)).astype(np.int64)
    f_p = np.floor(rs.random_sample((n, nf)) * (F - f_w + 1)).astype(np.int64)
    t_w = rs.randint(0, wt + 1, size=(n, nt)).astype(np.int64)
    t_u = rs.random_sample((n, nt))
    if bins is not None:
        t_w = np.minimum(t_w, bins[:, None])
    t_p = np.floor(t_u * ((Tb if bins is None else bins[:, None]) - t_w + 1)).astype(np.int64)
    u = rs.random_sample(n)
    freq, time = mask_words(f_p, f_w, F), mask_words(t_p, t_w, Tb)
    freq[u >= p] = 0
    time[u >= p] = 0
    return MaskPlan(freq, time)


def checked_mask(mask, n_clips: int, n_filters: int, time_bins: int):
    """A `MaskPlan` for a batch of ``n_clips`` as the entry points take it: ``(freq, time)`` contiguous uint32 host arrays of
    the shapes the ABI reads.  Raises ValueError."""
    if not isinstance(mask, MaskPlan):
        raise ValueError(f"mask must be a frontend.MaskPlan, got {type(mask).__name__}")
    out = []
    for name, a, bits in (("freq", mask.freq, n_filters), ("time", mask.time, time_bins)):
        a = np.asarray(a)
        shape = (int(n_clips), (int(bits) + 31) // 32)
        if a.dtype != np.uint32 or a.shape != shape:
            raise ValueError(f"mask.{name} must be uint32 {shape} (one row of words per clip), got {a.dtype} {a.shape}")
        out.append(np.ascontiguousarray(a))
    return tuple(out)


def upload_mask(mask, n_clips: int, n_filters: int, time_bins: int, device):
    """`checked_mask`, then the two word arrays on ``device`` (int32 tensors holding the uint32 bits), copied on the current
    stream without waiting, the way the mixer's per-clip arrays travel.  A plan of zero clips uploads nothing."""
    freq, time = checked_mask(mask, n_clips, n_filters, time_bins)
    return tuple(torch.from_numpy(a.view(np.int32)).to(device, non_blocking=True) for a in (freq, time))


_FRONT_ENDS: dict = {}


def _front_end(n_filters: int, filterbank: str, n_samples: int) -> SpikeFrontEnd:
    key = (int(n_filters), filterbank, int(n_samples))
    if key not in _FRONT_ENDS:
        _FRONT_ENDS[key] = SpikeFrontEnd(n_filters, filterbank, n_samples=n_samples)
    return _FRONT_ENDS[key]


def audio_to_spectrogram(audio: np.ndarray, n_filters: int, filterbank: str) -> np.ndarray:
    """create_dataset.py:39-78 for one clip: (n_samples,) -> (n_filters, TIME_BINS) in [0, 1]
    (float64 for gammatone, float32 for mel and for the flat-input zeros, as in the reference)."""
    fe = _front_end(n_filters, filterbank, len(audio))
    db, _ = fe.spectrogram_db(np.asarray(audio, dtype=np.float32))
    _, norm = fe.spikes_from_db(db, want_norm=True, want_raster=False)
    hi, lo = db.max(), db.min()
    if filterbank == "gammatone":
        lo = torch.maximum(lo, hi - 80.0)                  # create_dataset.py:60
    if float(hi - lo) < 1e-8:                              # create_dataset.py:64-65
        return np.zeros((n_filters, TIME_BINS), dtype=np.float32)
    return norm[0].cpu().numpy()


def convert_spectrogram_to_spikes_hysteresis(spectrogram, thresholds, hysteresis_gap=0.05):
    """create_dataset.py:81-98: (F, n_time) float -> (F, n_time*len(thresholds)) uint8."""
    _lib.require_gpu()
    lib = _lib.load()
    spec = np.ascontiguousarray(spectrogram)
    if spec.dtype not in (np.float32, np.float64):
        spec = spec.astype(np.float64)
    F, n_time = spec.shape
    on, off = threshold_tables(thresholds, hysteresis_gap, spec.dtype.type)
    dspec = torch.from_numpy(spec).cuda()
    out = torch.empty((F, n_time * len(on)), dtype=torch.uint8, device="cuda")
    fn = lib.lsm_encode_hysteresis_f64 if spec.dtype == np.float64 else lib.lsm_encode_hysteresis_f32
    _lib.check(fn(_dev(dspec), F, n_time, _host(on), _host(off), len(on), _dev(out), _stream()),
               "lsm_encode_hysteresis")
    return out.cpu().numpy()


def create_pure_redundancy(spike_train: np.ndarray, redundancy_factor: int) -> np.ndarray:
    """create_dataset.py:101-104 (host copy; the batched path repeats rows inside the kernel)."""
    return np.repeat(spike_train, redundancy_factor, axis=0)


# ---- bit-packed rasters: the packed variant of File 1 --------------------------

def pack_raster(raster: torch.Tensor) -> torch.Tensor:
    """(..., T) uint8 on the GPU (any non-zero byte is a spike) -> (..., ceil(T/8)) uint8, time step
    8q+k in bit k of byte q (``numpy.packbits(x != 0, axis=-1, bitorder="little")``)."""
    _lib.require_gpu()
    if raster.dtype != torch.uint8 or not raster.is_cuda:
        raise ValueError("pack_raster: expected a uint8 CUDA tensor")
    raster = raster.contiguous()
    T = raster.shape[-1]
    rows = raster.numel() // T if T else 0
    out = torch.empty(raster.shape[:-1] + ((T + 7) // 8,), dtype=torch.uint8, device=raster.device)
    _lib.check(_lib.load().lsm_raster_pack_bits(_dev(raster), rows, T, _dev(out), _stream()),
               "lsm_raster_pack_bits")
    return out


def unpack_raster(packed: torch.Tensor, n_steps: int) -> torch.Tensor:
    """Inverse of :func:`pack_raster`: (..., ceil(T/8)) uint8 on the GPU -> (..., T) bytes of 0/1."""
    _lib.require_gpu()
    if packed.dtype != torch.uint8 or not packed.is_cuda:
        raise ValueError("unpack_raster: expected a uint8 CUDA tensor")
    if packed.shape[-1] != (n_steps + 7) // 8:
        raise ValueError(f"unpack_raster: last dimension {packed.shape[-1]} does not hold {n_steps} steps")
    packed = packed.contiguous()
    rows = packed.numel() // packed.shape[-1] if packed.shape[-1] else 0
    out = torch.empty(packed.shape[:-1] + (n_steps,), dtype=torch.uint8, device=packed.device)
    _lib.check(_lib.load().lsm_raster_unpack_bits(_dev(packed), rows, n_steps, _dev(out), _stream()),
               "lsm_raster_unpack_bits")
    return out
