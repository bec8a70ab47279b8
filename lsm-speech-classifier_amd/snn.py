"""Host mirror of the reference's reservoir object protocol over the HIP reservoir kernel.

``SNN`` / ``SimulationParams`` stand in for ``snnpy.snn.SNN`` / ``SimulationParams`` as the
reference uses them (/root/reference/extract_lsm_features.py:2,79-83,100,109-116,164-188):
``SNN(simulation_params=P)``, ``.reset()``, ``.set_input_spike_times(u8 (C, T))``, ``.simulate()``,
``.extract_features_from_spikes() -> dict``, attributes ``.num_neurons`` and ``.spike_matrix``
(T, N).  ``run_batch`` is the batched path ``extract_all_features`` uses.  All arithmetic runs
in liblsm_hip.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .frontend import _dev, _host        # the package's one pair of pointer helpers
from .reservoir import Reservoir, SimulationParams, build_reservoir

# FEATURE_SETS['all'] order (extract_lsm_features.py:20-22) = key ids of the C ABI
FEATURE_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
                'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']

MAX_STEPS = 65535                    # steps of one run, launches of a continued run added up (16-bit spike times)

__all__ = ["SNN", "SimulationParams", "FEATURE_KEYS", "ReservoirState", "split_steps", "ragged_chunks", "MAX_STEPS"]


def split_steps(n_steps: int, max_steps: int) -> list:
    """Cut a run of ``n_steps`` into consecutive launches of at most ``max_steps``: [(first_step, steps), ...], every
    launch but the last one full."""
    n_steps, max_steps = int(n_steps), int(max_steps)
    if n_steps < 0 or max_steps < 1:
        raise ValueError(f"split_steps({n_steps}, {max_steps}): need n_steps >= 0 and max_steps >= 1")
    return [(t0, min(max_steps, n_steps - t0)) for t0 in range(0, n_steps, max_steps)]


def ragged_chunks(lengths, chunk_steps: int) -> list:
    """Cut the runs of clips of ``lengths[b]`` steps into consecutive ragged launches of at most ``chunk_steps``
    (SPEC.md §4c): [(first_step, n_steps, clip_steps), ...] with ``first_step = k * chunk_steps``, ``n_steps =
    min(chunk_steps, max(lengths) - first_step)`` and ``clip_steps = clip(lengths - first_step, 0, n_steps)`` (int32), one
    launch per ``chunk_steps`` of the longest clip -- none when every length is 0.  A clip that has ended rides along with
    0 steps."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    chunk_steps = int(chunk_steps)
    if chunk_steps < 1 or (lengths < 0).any():
        raise ValueError(f"ragged_chunks: need chunk_steps >= 1 (got {chunk_steps}) and lengths >= 0")
    longest = int(lengths.max()) if len(lengths) else 0
    return [(t0, n, np.clip(lengths - t0, 0, n).astype(np.int32)) for t0, n in split_steps(longest, chunk_steps)]


class ReservoirState:
    """What a reservoir carries from one launch to the next (SPEC.md §4a, ``lsm_reservoir_run_from``): ``data``, a
    (B, state_bytes) uint8 device tensor in the library's layout -- all zeros is ``reset()`` --, and ``steps_done``, the
    host's count of the steps it holds.  ``SNN.run_batch(..., state=...)`` updates both in place.  ``ended`` (host, (B,) bool): clip b ran fewer steps than a ragged
    launch's ``n_steps`` (``run_batch(lengths=...)``, SPEC.md §4c) -- its run is over, later launches must give it 0 steps;
    ``steps_done`` keeps advancing by every launch's ``n_steps`` (the one ``first_step`` of the next launch)."""

    def __init__(self, data: torch.Tensor, num_neurons: int, num_output_neurons: int, steps_done: int = 0, ended=None):
        self.data = data
        self.num_neurons = int(num_neurons)
        self.num_output_neurons = int(num_output_neurons)
        self.steps_done = int(steps_done)
        self.ended = (np.zeros(int(data.shape[0]), dtype=bool) if ended is None
                      else np.array(ended, dtype=bool).reshape(-1))
        self._np = (self.num_neurons + 63) // 64 * 64

    def clone(self) -> "ReservoirState":
        return ReservoirState(self.data.clone(), self.num_neurons, self.num_output_neurons, self.steps_done, self.ended)

    def _field(self, offset: int, nbytes: int, dtype) -> torch.Tensor:
        return self.data[:, offset:offset + nbytes].contiguous().view(dtype)

    def _bits(self, offset: int) -> torch.Tensor:
        words = self._field(offset, self._np // 8, torch.int32)                       # (B, NP/32), bit i%32 of word i/32
        shifts = torch.arange(32, device=words.device, dtype=torch.int32)
        return ((words[:, :, None] >> shifts) & 1).reshape(words.shape[0], -1)[:, :self.num_neurons].bool()

    def spike_total(self) -> torch.Tensor:
        """(B,) spikes of the whole reservoir so far."""
        return self._field(0, 4, torch.int32)[:, 0]

    def membrane(self) -> torch.Tensor:
        """(B, N) float32 membrane potentials after the last step done."""
        return self._field(16, 4 * self._np, torch.float32)[:, :self.num_neurons]

    def refractory(self) -> torch.Tensor:
        """(B, N) int32 refractory countdowns after the last step done."""
        return self._field(16 + 4 * self._np, 2 * self._np, torch.int16)[:, :self.num_neurons].to(torch.int32) & 0xFFFF

    def last_spikes(self) -> torch.Tensor:
        """(B, N) bool: fired at the last step done."""
        return self._bits(16 + 6 * self._np)

    def ever_fired(self) -> torch.Tensor:
        """(B, N) bool: fired at least once so far."""
        return self._bits(16 + 6 * self._np + self._np // 8)


def _select_keys(feature_keys):
    """``(keys, key_ids)``: the names of ``feature_keys`` that are FEATURE_KEYS, in the given order (``None``: all of them),
    and their ids in the C ABI as an int32 array."""
    keys = FEATURE_KEYS if feature_keys is None else [k for k in feature_keys if k in FEATURE_KEYS]
    return keys, np.array([FEATURE_KEYS.index(k) for k in keys], dtype=np.int32)


def _check_stats_out(stats_out, n_clips: int, device) -> None:
    if stats_out is not None and (stats_out.dtype != torch.int32 or tuple(stats_out.shape) != (n_clips, 2)
                                  or not stats_out.is_contiguous() or stats_out.device != device):
        raise ValueError(f"stats_out must be a contiguous int32 ({n_clips}, 2) tensor on {device}")


class SNN:
    def __init__(self, simulation_params: SimulationParams, n_channels: int | None = None,
                 device=None, reservoir: Reservoir | None = None):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.params = simulation_params
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:        # pin it now (as frontend.SpikeFrontEnd)
            self.device = torch.device("cuda", torch.cuda.current_device())
        if reservoir is None:
            if n_channels is None:
                ist = simulation_params.input_spike_times
                if ist is None:
                    raise ValueError("SNN needs n_channels or simulation_params.input_spike_times")
                n_channels = int(np.asarray(ist).shape[0])
            reservoir = build_reservoir(simulation_params, n_channels)
        self.reservoir = reservoir
        self.num_neurons = reservoir.num_neurons
        self.n_channels = reservoir.n_channels
        self.num_output_neurons = len(reservoir.out_idx)
        self._handle = C.c_void_p()
        self._compute_units = torch.cuda.get_device_properties(self.device).multi_processor_count
        r = reservoir
        with torch.cuda.device(self.device):
            _lib.check(self.lib.lsm_reservoir_create(
                C.byref(self._handle), r.num_neurons, r.n_channels, _host(r.csc_ptr),
                _host(r.csc_post), _host(r.csc_w), _host(r.leak),
                _host(np.ascontiguousarray(r.in_tgt, dtype=np.int32)), int(r.in_fanout),
                float(r.w_in), _host(r.out_idx), len(r.out_idx), float(r.theta),
                int(r.refractory_period), int(r.burst_isi_max)), "lsm_reservoir_create")
        self._input = None
        self.spike_matrix = None
        self._features = None
        self._max_steps = {}             # (n_clips, waves_per_clip) -> max_steps, until set_kernel changes the plans

    def __del__(self):
        try:
            h = getattr(self, "_handle", None)
            if h is not None and h.value:
                self.lib.lsm_reservoir_destroy(h)
                self._handle = None
        except Exception:          # interpreter shutdown: modules may already be torn down
            pass

    # ---- batched path -------------------------------------------------------------------
    def run_batch(self, spikes, feature_keys=None, want_spike_matrix=False, want_v_trace=False,
                  waves_per_clip: int = 0, packed_time_steps: int = 0, stats_out=None, features_out=None,
                  longest_first: bool | None = None, state: ReservoirState | None = None,
                  state_out: ReservoirState | None = None, lengths=None):
        """spikes: uint8 (B, C, T) torch tensor on this device (or NumPy, copied).  Returns
        (features float32 (B, n_keys*N_out) device tensor, spike_matrix or None, v_trace or None);
        NaN entries are already 0 and keys are concatenated in the given order
        (extract_lsm_features.py:85-87).  With ``packed_time_steps=T`` the input is the bit-packed
        form (B, C, ceil(T/8)) of ``spikefile``: it is uploaded as it is and unpacked on the GPU.
        ``stats_out``: optional int32 (B, 2) device tensor that receives, per clip, the number of neurons
        that fired at least once and the spikes of the whole reservoir (accumulated inside the kernel).
        ``waves_per_clip``: 0 = the library's layout for a lone launch, -1 = its layout for a launch that
        shares the GPU with other kernels (``pipeline.HotPath``), else 1, 2, 4, 8 or 16.
        ``features_out``: optional contiguous float32 (B, n_keys*N_out) device tensor to write the rows into
        (e.g. this step's slice of a gather buffer) instead of a fresh one.
        ``longest_first``: start the clips with the most input spikes first (``lsm_reservoir_run_ordered``: a
        clip's time grows with its activity, and a launch of several rounds is otherwise as long as whichever
        clip starts last); results are the same either way.  Default: on when the batch has more clips than the
        GPU has compute units (``LSM_RESERVOIR_ORDER=0`` turns the default off).
        ``state``: a ``ReservoirState`` (``new_state(B)``) to continue from: the launch runs steps
        ``[state.steps_done, state.steps_done + T)``, updates the state in place and returns the features of the whole run
        so far (absolute spike times); ``spike_matrix`` / ``v_trace`` cover this launch's T steps, ``stats_out`` the run so
        far.  A run cut at any step gives what the uncut run gives, bit for bit (``lsm_reservoir_run_from``).
        ``state_out``: with ``state``, write the new state there and leave ``state`` as it is.
        ``lengths``: the steps every clip runs in this launch (``lsm_reservoir_run_ragged``, SPEC.md §4c) -- a sequence, a
        NumPy array or an int32 tensor of B values in [0, T]; T stays the row stride of ``spikes`` and of the (B, T, N)
        outputs.  Clip b's results are those of a launch over ``spikes[b, :, :lengths[b]]`` alone; input at
        ``t >= lengths[b]`` influences nothing, and a clip of 0 steps keeps its feature row, statistics and state.  The
        outputs allocated here start as zeros, so rows past a clip's length read as zeros.  Host values outside [0, T]
        raise ``ValueError`` (values of a device tensor are not read back: the kernels clamp them).  With ``state``, a
        clip given fewer than T steps is marked ``state.ended`` and may only be given 0 steps from then on."""
        spikes = self._spikes(spikes, packed_time_steps).to(self.device, dtype=torch.uint8).contiguous()
        B, _, T = spikes.shape
        keys, key_ids = _select_keys(feature_keys)
        ragged = lengths is not None
        host_lengths = self._host_counts(lengths, B, T, "lengths") if ragged else None
        if ragged and state is not None and host_lengths is not None and (host_lengths[state.ended] > 0).any():
            raise ValueError(f"clips {np.nonzero(state.ended & (host_lengths > 0))[0].tolist()} have ended (they ran fewer "
                             f"steps than an earlier launch's n_steps) and can only be given 0 steps")
        alloc = torch.zeros if ragged else torch.empty          # ragged: what a clip does not write reads as zeros
        if features_out is not None:
            if (features_out.dtype != torch.float32 or tuple(features_out.shape) != (B, len(keys) * self.num_output_neurons)
                    or not features_out.is_contiguous() or features_out.device != spikes.device):
                raise ValueError(f"features_out must be a contiguous float32 ({B}, {len(keys) * self.num_output_neurons}) "
                                 f"tensor on {spikes.device}")
            feats = features_out
        else:
            feats = alloc((B, len(keys) * self.num_output_neurons), dtype=torch.float32, device=self.device)
        sm = (alloc((B, T, self.num_neurons), dtype=torch.uint8, device=self.device)
              if want_spike_matrix else None)
        vt = (alloc((B, T, self.num_neurons), dtype=torch.float32, device=self.device)
              if want_v_trace else None)
        _check_stats_out(stats_out, B, spikes.device)
        first_step, src, dst = self._continuation(state, state_out, B)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            ws, need = self._order_workspace(B, longest_first)
            clips = (self._handle, _dev(spikes), B, T)
            outputs = (_host(key_ids), len(keys), _dev(feats), _dev(sm), _dev(vt), _dev(stats_out), int(waves_per_clip))
            if ragged:
                steps = self._device_counts(lengths, host_lengths)
                _lib.check(self.lib.lsm_reservoir_run_ragged(*clips, _dev(steps), first_step, _dev(src), _dev(dst), *outputs,
                                                             _dev(ws), need, stream), "lsm_reservoir_run_ragged")
            elif state is not None:
                _lib.check(self.lib.lsm_reservoir_run_from(*clips, first_step, _dev(src), _dev(dst), *outputs,
                                                           _dev(ws), need, stream), "lsm_reservoir_run_from")
            elif ws is not None:
                _lib.check(self.lib.lsm_reservoir_run_ordered(*clips, *outputs, _dev(ws), need, stream),
                           "lsm_reservoir_run_ordered")
            else:
                _lib.check(self.lib.lsm_reservoir_run(*clips, *outputs, stream), "lsm_reservoir_run")
        if state is not None:
            done = state_out or state
            if ragged:
                done.ended = state.ended | (host_lengths < T) if host_lengths is not None else state.ended.copy()
            done.steps_done = state.steps_done + T
        return feats, sm, vt

    # ---- the argument steps the launch methods share ------------------------------------
    def _spikes(self, spikes, packed_time_steps: int = 0):
        """A launch's ``spikes`` (tensor, or NumPy: copied) as a (B, C, T) tensor, unpacked on the GPU first when
        ``packed_time_steps`` says they are bit-packed; another shape is refused.  The caller moves it to the device."""
        if isinstance(spikes, np.ndarray):
            spikes = torch.from_numpy(np.ascontiguousarray(spikes, dtype=np.uint8))
        if packed_time_steps:
            from .frontend import unpack_raster
            with torch.cuda.device(self.device):
                spikes = unpack_raster(spikes.to(self.device, dtype=torch.uint8).contiguous(), int(packed_time_steps))
        if spikes.dim() != 3 or spikes.shape[1] != self.n_channels:
            raise ValueError(f"spikes must be (B, {self.n_channels}, T), got {tuple(spikes.shape)}")
        return spikes

    @staticmethod
    def _host_counts(counts, n_clips: int, limit: int, noun: str):
        """A launch's per-clip ``lengths`` or ``segments`` (``noun``) as an int64 host array, checked against [0, limit];
        ``None`` for a device tensor (never read back: the kernels clamp its values)."""
        if isinstance(counts, torch.Tensor):
            if counts.dtype != torch.int32 or tuple(counts.shape) != (n_clips,):
                raise ValueError(f"{noun} must hold {n_clips} int32 values, got {counts.dtype} {tuple(counts.shape)}")
            if counts.is_cuda:
                return None
            counts = counts.numpy()
        arr = np.asarray(counts)
        if arr.shape != (n_clips,) or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"{noun} must be {n_clips} integers, got {arr.dtype} {arr.shape}")
        arr = arr.astype(np.int64)
        if ((arr < 0) | (arr > limit)).any():
            bad = np.nonzero((arr < 0) | (arr > limit))[0]
            raise ValueError(f"{noun} {arr[bad].tolist()} of clips {bad.tolist()} outside [0, {limit}]")
        return arr

    @staticmethod
    def _host_segments(segments, n_clips: int, n_segments: int):
        """``_host_counts`` of a launch's ``segments``: what ``pipeline.StreamBank`` asks of its net."""
        return SNN._host_counts(segments, n_clips, n_segments, "segments")

    def _device_counts(self, counts, host_counts):
        """The int32 device tensor of per-clip counts a launch reads: from ``_host_counts``' array, else the caller's device
        tensor."""
        if host_counts is None:
            return counts.to(self.device, dtype=torch.int32).contiguous()
        return torch.from_numpy(host_counts.astype(np.int32)).to(self.device)

    def _continuation(self, state, state_out, n_clips: int):
        """``(first_step, state_in, state_out)`` of a launch as tensors: from ``state`` into ``state_out`` or back into
        ``state``; without ``state`` the launch starts from ``reset()`` and keeps nothing: (0, None, None)."""
        if state is None:
            if state_out is not None:
                raise ValueError("state_out needs state (SNN.new_state(B) is the state after reset())")
            return 0, None, None
        self._check_state(state, n_clips)
        if state_out is not None:
            self._check_state(state_out, n_clips)
        return state.steps_done, state.data, (state_out or state).data

    def _order_workspace(self, n_clips: int, longest_first):
        """``(workspace, bytes)`` of a launch that starts its clips longest first (``longest_first``, ``None``: the default
        for a batch of this size), else ``(None, 0)``.  Scratch of this call alone: the caching allocator hands a block back
        to the stream it was taken on."""
        if longest_first is None:
            longest_first = self.longest_first_default(n_clips)
        if not longest_first:
            return None, 0
        need = self.lib.lsm_reservoir_order_workspace(n_clips)
        return torch.empty((need + 3) // 4, dtype=torch.int32, device=self.device), need

    # ---- continuation -------------------------------------------------------------------
    def state_bytes(self) -> int:
        """Bytes of one clip's state block (``lsm_reservoir_state_bytes``)."""
        return int(self.lib.lsm_reservoir_state_bytes(self._handle))

    def new_state(self, n_clips: int) -> ReservoirState:
        """The state of ``n_clips`` reservoirs after ``reset()``: zeros, no step done."""
        data = torch.zeros((int(n_clips), self.state_bytes()), dtype=torch.uint8, device=self.device)
        return ReservoirState(data, self.num_neurons, self.num_output_neurons, 0)

    def _check_state(self, state, n_clips: int) -> None:
        if not isinstance(state, ReservoirState):
            raise _lib.LsmHipError(f"state must be a ReservoirState (SNN.new_state), got {type(state).__name__}")
        d = state.data
        if (d.dtype != torch.uint8 or tuple(d.shape) != (n_clips, self.state_bytes()) or not d.is_contiguous()
                or d.device != self.device):
            raise _lib.LsmHipError(f"state must hold a contiguous uint8 ({n_clips}, {self.state_bytes()}) tensor on "
                                   f"{self.device}, got {d.dtype} {tuple(d.shape)} on {d.device}")

    def max_steps(self, n_clips: int, waves_per_clip: int = 0) -> int:
        """Largest T ``plan(n_clips, T, waves_per_clip)`` accepts (``lsm_reservoir_max_steps``)."""
        n = int(self.lib.lsm_reservoir_max_steps(self._handle, int(n_clips), int(waves_per_clip)))
        if n < 0:
            _lib.check(n, "lsm_reservoir_max_steps")
        return n

    def _max_steps_cached(self, n_clips: int, waves_per_clip: int = 0) -> int:
        key = (int(n_clips), int(waves_per_clip))
        if key not in self._max_steps:
            self._max_steps[key] = self.max_steps(*key)
        return self._max_steps[key]

    def run_chunked(self, spikes, feature_keys=None, chunk_steps: int | None = None, want_spike_matrix=False,
                    want_v_trace=False, waves_per_clip: int = 0, stats_out=None, longest_first: bool | None = None,
                    lengths=None, want_state: bool = False):
        """``run_batch`` for clips of any length up to 65535 steps: the run is cut into launches of ``chunk_steps`` (default:
        the longest launch the plan accepts, ``max_steps``) that hand their state on.  Same returns and the same values as
        one launch over the whole clip would give; ``spike_matrix`` / ``v_trace`` are assembled over the launches.
        ``lengths``: host integers, the steps of every clip (SPEC.md §4c; ``ragged_chunks``): clip b's results are those of
        the uncut run over ``spikes[b, :, :lengths[b]]`` alone.  One features and one statistics buffer serve all launches,
        so a clip keeps the row of the launch it ended in; rows of ``spike_matrix`` / ``v_trace`` past a clip's length,
        and everything of a clip of length 0, are zeros.
        ``want_state``: return the ``ReservoirState`` after the last launch as a fourth value (each clip's state after its
        own last step)."""
        spikes = self._spikes(spikes).to(self.device, dtype=torch.uint8)
        B, _, T = spikes.shape
        if T < 1 or T > MAX_STEPS:
            raise _lib.LsmHipError(f"n_steps = {T} outside [1, {MAX_STEPS}]")
        if chunk_steps is None:
            chunk_steps = self.max_steps(B, waves_per_clip)
        if lengths is not None:
            return self._run_chunked_ragged(spikes, lengths, feature_keys, int(chunk_steps), want_spike_matrix, want_v_trace,
                                            waves_per_clip, stats_out, longest_first, want_state)
        state = self.new_state(B)
        feats, sms, vts = None, [], []
        for t0, n in split_steps(T, chunk_steps):
            feats, sm, vt = self.run_batch(spikes[:, :, t0:t0 + n], feature_keys, want_spike_matrix, want_v_trace,
                                           waves_per_clip, stats_out=stats_out, longest_first=longest_first, state=state)
            sms.append(sm)
            vts.append(vt)
        out = (feats, torch.cat(sms, dim=1) if want_spike_matrix else None,
               torch.cat(vts, dim=1) if want_v_trace else None)
        return out + (state,) if want_state else out

    def _run_chunked_ragged(self, spikes, lengths, feature_keys, chunk_steps, want_spike_matrix, want_v_trace,
                            waves_per_clip, stats_out, longest_first, want_state):
        B, _, T = spikes.shape
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.cpu().numpy()
        lengths = self._host_counts(lengths, B, T, "lengths")
        keys, _ = _select_keys(feature_keys)
        feats = torch.zeros((B, len(keys) * self.num_output_neurons), dtype=torch.float32, device=self.device)
        sm = torch.zeros((B, T, self.num_neurons), dtype=torch.uint8, device=self.device) if want_spike_matrix else None
        vt = torch.zeros((B, T, self.num_neurons), dtype=torch.float32, device=self.device) if want_v_trace else None
        state = self.new_state(B)
        for t0, n, steps in ragged_chunks(lengths, chunk_steps):
            _, sm_k, vt_k = self.run_batch(spikes[:, :, t0:t0 + n], feature_keys, want_spike_matrix, want_v_trace,
                                           waves_per_clip, stats_out=stats_out, features_out=feats,
                                           longest_first=longest_first, state=state, lengths=steps)
            if want_spike_matrix:
                sm[:, t0:t0 + n] = sm_k
            if want_v_trace:
                vt[:, t0:t0 + n] = vt_k
        return (feats, sm, vt, state) if want_state else (feats, sm, vt)

    # ---- segments and windows (SPEC.md §4b) ---------------------------------------------
    def run_segment_records(self, spikes, segment_steps: int, feature_keys=(), want_spike_matrix=False,
                            want_v_trace=False, waves_per_clip: int = 0, stats_out=None,
                            longest_first: bool | None = None, state: ReservoirState | None = None,
                            state_out: ReservoirState | None = None):
        """One segmented launch (``lsm_reservoir_run_segments``): ``run_batch(state=...)`` whose feature bookkeeping is cut
        every ``segment_steps`` steps.  Returns ``(records, features, spike_matrix, v_trace)``: ``records`` is the
        (B, T // segment_steps, N_out, 4) int32 device tensor of the segments' integer records (times local to the
        segment), the other three are ``run_batch``'s for the same launch (``features`` cumulative, ``None`` without
        ``feature_keys``).  Without ``state`` the launch starts from ``reset()``."""
        spikes = self._spikes(spikes).to(self.device, dtype=torch.uint8).contiguous()
        B, _, T = spikes.shape
        S = int(segment_steps)
        if S < 1 or T % S != 0:
            raise _lib.LsmHipError(f"segment_steps = {S} must be >= 1 and divide the launch's {T} steps")
        keys, key_ids = _select_keys(feature_keys or ())
        feats = (torch.empty((B, len(keys) * self.num_output_neurons), dtype=torch.float32, device=self.device)
                 if keys else None)
        sm = torch.empty((B, T, self.num_neurons), dtype=torch.uint8, device=self.device) if want_spike_matrix else None
        vt = torch.empty((B, T, self.num_neurons), dtype=torch.float32, device=self.device) if want_v_trace else None
        _check_stats_out(stats_out, B, spikes.device)
        first_step, src, dst = self._continuation(state, state_out, B)
        records = torch.empty((B, T // S, self.num_output_neurons, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            ws, need = self._order_workspace(B, longest_first)
            _lib.check(self.lib.lsm_reservoir_run_segments(
                self._handle, _dev(spikes), B, T, S, first_step, _dev(src), _dev(dst), _dev(records),
                _host(key_ids) if keys else None, len(keys), _dev(feats), _dev(sm), _dev(vt), _dev(stats_out),
                int(waves_per_clip), _dev(ws), need, stream), "lsm_reservoir_run_segments")
        if state is not None:
            (state_out or state).steps_done = state.steps_done + T
        return records, feats, sm, vt

    # ---- streams (SPEC.md §4d) ----------------------------------------------------------
    def run_stream_records(self, spikes, segment_steps: int, segments=None, state: ReservoirState | None = None,
                           state_out: ReservoirState | None = None, want_spike_matrix=False, want_v_trace=False,
                           waves_per_clip: int = 0, stats_out=None, longest_first: bool | None = None):
        """One stream launch (``lsm_reservoir_run_stream``, SPEC.md §4d): a segmented launch that keeps no cumulative
        feature record, so that it needs no position -- streams anywhere on their own timelines share it, and a stream has
        no length limit.  ``spikes`` is (B, C, T) with ``T % segment_steps == 0``; ``segments``: a sequence, a NumPy array or
        an int32 tensor of B values in [0, T // segment_steps], the whole segments every clip runs (default: all).  Clip b
        runs the first ``segments[b] * segment_steps`` columns of its row from ``state`` (else from ``reset()``); a clip of 0
        segments keeps its state, statistics and rows.  Returns ``(records, spike_matrix, v_trace)``: ``records``
        (B, T // segment_steps, N_out, 4) int32 as ``run_segment_records`` gives them, valid at ``g < segments[b]``.  The
        tensors allocated here start as zeros, so unwritten records and rows read as zeros.  Host values out of range raise
        ``ValueError`` (a device tensor is not read back: the kernels clamp).  ``state.data`` is updated in place (or
        ``state_out.data`` written) with its feature-record block zeroed; ``steps_done`` and ``ended`` are not touched -- a
        stream has neither."""
        spikes = self._spikes(spikes)                   # every refusal below comes before the library or a device is touched
        B, _, T = spikes.shape
        S = int(segment_steps)
        if S < 1 or T < 1 or T % S != 0:
            raise ValueError(f"segment_steps = {S} must be >= 1 and divide the launch's {T} steps")
        G = T // S
        host_segments = self._host_segments(segments, B, G) if segments is not None else None
        spikes = spikes.to(self.device, dtype=torch.uint8).contiguous()
        _check_stats_out(stats_out, B, spikes.device)
        _, src, dst = self._continuation(state, state_out, B)
        records = torch.zeros((B, G, self.num_output_neurons, 4), dtype=torch.int32, device=self.device)
        sm = torch.zeros((B, T, self.num_neurons), dtype=torch.uint8, device=self.device) if want_spike_matrix else None
        vt = torch.zeros((B, T, self.num_neurons), dtype=torch.float32, device=self.device) if want_v_trace else None
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            counts = self._device_counts(segments, host_segments) if segments is not None else None
            ws, need = self._order_workspace(B, longest_first)
            _lib.check(self.lib.lsm_reservoir_run_stream(
                self._handle, _dev(spikes), B, T, S, _dev(counts), _dev(src), _dev(dst), _dev(records), _dev(sm), _dev(vt),
                _dev(stats_out), int(waves_per_clip), _dev(ws), need, stream), "lsm_reservoir_run_stream")
        return records, sm, vt

    @staticmethod
    def segment_windows(n_segments: int, window_segments: int = 1, hop_segments: int = 1) -> int:
        """Number of windows of ``window_segments`` segments, ``hop_segments`` apart, in ``n_segments`` segments."""
        G, K, H = int(n_segments), int(window_segments), int(hop_segments)
        if K < 1 or K > G or H < 1:
            raise _lib.LsmHipError(f"window_segments = {K} must be in [1, {G}] and hop_segments = {H} >= 1")
        return (G - K) // H + 1

    def segment_features(self, records, segment_steps: int, feature_keys=None, window_segments: int = 1,
                         hop_segments: int = 1, features_out=None, segments=None):
        """Feature rows of sliding windows over segment records (``lsm_segment_features``): ``records`` (B, G, N_out, 4)
        int32 as ``run_segment_records`` returns them (launches concatenated along dim 1).  Returns float32
        (B, W, n_keys*N_out); window w covers segments ``[w*hop, w*hop + window_segments)`` and its row is the feature row
        of that slice of the spike matrix.
        ``segments``: the valid records of every clip (``lsm_segment_features_ragged``, SPEC.md §4d) -- B values as
        ``run_stream_records`` takes them, in [0, G].  Clip b then has ``(segments[b] - window_segments) // hop_segments + 1``
        rows (none below ``window_segments``); the rows past them are zeros, or in a caller's ``features_out`` left as they
        are."""
        if (records.dtype != torch.int32 or records.dim() != 4 or tuple(records.shape[2:]) != (self.num_output_neurons, 4)
                or records.device != self.device):
            raise ValueError(f"records must be an int32 (B, G, {self.num_output_neurons}, 4) tensor on {self.device}")
        records = records.contiguous()
        B, G = int(records.shape[0]), int(records.shape[1])
        keys, key_ids = _select_keys(feature_keys)
        W = self.segment_windows(G, window_segments, hop_segments)
        shape = (B, W, len(keys) * self.num_output_neurons)
        ragged = segments is not None
        host_segments = self._host_segments(segments, B, G) if ragged else None
        if features_out is not None:
            if (features_out.dtype != torch.float32 or tuple(features_out.shape) != shape
                    or not features_out.is_contiguous() or features_out.device != self.device):
                raise ValueError(f"features_out must be a contiguous float32 {shape} tensor on {self.device}")
            feats = features_out
        else:
            feats = (torch.zeros if ragged else torch.empty)(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if ragged:
                counts = self._device_counts(segments, host_segments)
                _lib.check(self.lib.lsm_segment_features_ragged(
                    self._handle, _dev(records), B, G, _dev(counts), int(segment_steps), int(window_segments),
                    int(hop_segments), _host(key_ids), len(keys), _dev(feats), stream), "lsm_segment_features_ragged")
                return feats
            _lib.check(self.lib.lsm_segment_features(
                self._handle, _dev(records), B, G, int(segment_steps), int(window_segments), int(hop_segments),
                _host(key_ids), len(keys), _dev(feats), stream), "lsm_segment_features")
        return feats

    def run_segments(self, spikes, segment_steps: int, feature_keys=None, window_segments: int = 1,
                     hop_segments: int = 1, state: ReservoirState | None = None,
                     state_out: ReservoirState | None = None, waves_per_clip: int = 0,
                     longest_first: bool | None = None, want_records: bool = False, features_out=None,
                     stats_out=None):
        """Features per time segment or sliding window: float32 (B, W, n_keys*N_out) on the device, and with
        ``want_records`` the (B, G, N_out, 4) records tensor as well.  The reservoir runs once over the clip (from
        ``state``, else from ``reset()``); every ``segment_steps`` steps the integer feature records are closed, and
        window w folds those of segments ``[w*hop_segments, w*hop_segments + window_segments)``: its row is, bit for
        bit, the feature row of that slice of the spike matrix (``window_segments=1``: one row per segment).  Clips
        longer than ``max_steps`` are cut at segment boundaries into launches that hand their state on.  ``features_out`` /
        ``stats_out``: as ``run_batch``'s (a contiguous (B, W, n_keys*N_out) tensor; the statistics of the run so far)."""
        spikes = self._spikes(spikes).to(self.device, dtype=torch.uint8)
        B, _, T = spikes.shape
        S = int(segment_steps)
        if S < 1 or T < 1 or T % S != 0:
            raise _lib.LsmHipError(f"segment_steps = {S} must be >= 1 and divide the clip's {T} steps")
        self.segment_windows(T // S, window_segments, hop_segments)      # refuse before anything is launched
        if int(window_segments) * S > MAX_STEPS:
            raise _lib.LsmHipError(f"a window of {window_segments} segments of {S} steps exceeds {MAX_STEPS} steps")
        longest = self._max_steps_cached(B, waves_per_clip)
        chunk = longest // S * S
        if chunk < 1:
            raise _lib.LsmHipError(f"segment_steps = {S} exceeds the longest launch the plan accepts for {B} clips "
                                   f"({longest} steps)")
        parts = split_steps(T, chunk)
        if state is None and len(parts) > 1:
            state = self.new_state(B)                                     # carried between the launches only
            state_out = None
        recs = []
        for i, (t0, n) in enumerate(parts):
            # the caller's state stays as it is when state_out is given: the first launch moves over to state_out
            r, _, _, _ = self.run_segment_records(spikes[:, :, t0:t0 + n], S, (), False, False, waves_per_clip,
                                                  stats_out, longest_first, state, state_out)
            if state_out is not None:
                state, state_out = state_out, None
            recs.append(r)
        records = recs[0] if len(recs) == 1 else torch.cat(recs, dim=1)
        feats = self.segment_features(records, S, feature_keys, window_segments, hop_segments, features_out)
        return (feats, records) if want_records else feats

    def longest_first_default(self, n_clips: int) -> bool:
        """Whether ``run_batch`` starts the clips of a batch of this size longest first by default."""
        return n_clips > self._compute_units and os.environ.get("LSM_RESERVOIR_ORDER", "1") != "0"

    def diagnostics(self, spikes) -> dict:
        """Batched health statistics (the quantities /root/reference/extract_lsm_features.py:119-133
        derives per clip from ``lsm.spike_matrix``): per clip the share of neurons that fired at least
        once, the number of silent neurons and the mean spikes per neuron.  The two integers behind them
        come out of the reservoir kernel itself (one flag per neuron, one count per wave): no (T, N) spike
        matrix is written or reduced."""
        B = int(spikes.shape[0])
        stats = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        self.run_batch(spikes, ['spike_counts'], stats_out=stats)
        st = stats.cpu().numpy().astype(np.int64)                        # exact integers from here on
        active, total = st[:, 0], st[:, 1]
        return {
            "participation": active / self.num_neurons * 100,           # same expression as the reference
            "dead_neurons": self.num_neurons - active,
            "mean_spikes_per_neuron": total / self.num_neurons,
        }

    # 'band': round-1 name of 'ring'; 'ring-contiguous': ring rows with contiguous quad ownership only (tests)
    # 'ring-pairs' / 'ring-quads': ring rows shared out in 128-neuron pair blocks (csrc/lif_pair.h) / in 256-neuron quads
    # (csrc/lif_ring.h) only -- 'ring' takes pair blocks where the reservoir has them and they pay (tests, same-box A/B runs)
    KERNEL_MODES = {"auto": 0, "sparse": 1, "dense": 2, "ring": 3, "band": 3, "ring-contiguous": 4, "ring-pairs": 5,
                    "ring-quads": 6}

    def set_kernel(self, mode: str = "auto"):
        """'auto' (register accumulation over dense presynaptic rows; over ring rows -- dense ring window
        plus a list of the rewired synapses -- for ring-like reservoirs whose dense table exceeds the L2
        caches), 'sparse' (CSC scatter through LDS), 'dense' or 'ring'.  'dense' on a reservoir that 'auto' serves
        with ring rows builds the dense table now (one allocation + synchronisation on this device)."""
        with torch.cuda.device(self.device):
            return self._set_kernel(mode)

    def _set_kernel(self, mode: str = "auto"):
        self._max_steps.clear()
        _lib.check(self.lib.lsm_reservoir_set_kernel(self._handle, self.KERNEL_MODES[mode]),
                   "lsm_reservoir_set_kernel")

    def kernel_in_use(self) -> str:
        return {1: "sparse", 2: "dense", 3: "ring"}[self.lib.lsm_reservoir_kernel_in_use(self._handle)]

    def plan(self, n_clips: int, n_steps: int, waves_per_clip: int = 0) -> dict:
        """What `run_batch` would launch for this batch: kernel, layout, LDS bytes per clip and the bytes of the
        weight table that kernel gathers from (`lsm_reservoir_plan`), plus the bytes one spike requests from it, mean
        over the presynaptic neurons (`lsm_reservoir_row_request_bytes`).  ``ring_form``: how ring rows are shared out --
        ``"quads-contiguous"``, ``"quads"`` (strided ownership) or ``"pairs"`` (pair blocks) -- and ``None`` for the other
        kernels (`lsm_reservoir_ring_form`)."""
        k, wpc, sl, lds, tab = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_long()
        _lib.check(self.lib.lsm_reservoir_plan(self._handle, n_clips, n_steps, waves_per_clip, C.byref(k),
                                               C.byref(wpc), C.byref(sl), C.byref(lds), C.byref(tab)),
                   "lsm_reservoir_plan")
        rb = C.c_double()
        _lib.check(self.lib.lsm_reservoir_row_request_bytes(self._handle, n_clips, n_steps, waves_per_clip,
                                                            C.byref(rb)), "lsm_reservoir_row_request_bytes")
        return {"kernel": {1: "sparse", 2: "dense", 3: "ring"}[k.value], "waves_per_clip": wpc.value,
                "slots_per_lane": sl.value, "lds_bytes": lds.value, "table_bytes": tab.value,
                "row_request_bytes": rb.value,
                "input_mode": self._input_mode(n_clips, n_steps, waves_per_clip),
                "ring_form": self._ring_form(n_clips, n_steps, waves_per_clip)}

    RING_FORMS = {0: None, 1: "quads-contiguous", 2: "quads", 3: "pairs"}

    def _ring_form(self, n_clips: int, n_steps: int, waves_per_clip: int):
        form = int(self.lib.lsm_reservoir_ring_form(self._handle, n_clips, n_steps, waves_per_clip))
        if form < 0:
            _lib.check(form, "lsm_reservoir_ring_form")
        return self.RING_FORMS[form]

    def _input_mode(self, n_clips: int, n_steps: int, waves_per_clip: int) -> int:
        mode = int(self.lib.lsm_reservoir_input_mode(self._handle, n_clips, n_steps, waves_per_clip))
        if mode < 0:                         # an LSM_ERR_* code is not a mode
            _lib.check(mode, "lsm_reservoir_input_mode")
        return mode

    def layout(self, n_clips: int, n_steps: int, waves_per_clip: int = 0):
        wpc, sl, lds = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.lib.lsm_reservoir_layout(self._handle, n_clips, n_steps, waves_per_clip,
                                                 C.byref(wpc), C.byref(sl), C.byref(lds)))
        return {"waves_per_clip": wpc.value, "slots_per_lane": sl.value, "lds_bytes": lds.value}

    # ---- the reference's single-clip protocol -------------------------------------------
    def reset(self):
        self._input = None
        self.spike_matrix = None
        self._features = None

    def set_input_spike_times(self, sample):
        self._input = np.ascontiguousarray(sample, dtype=np.uint8)

    def simulate(self):
        if self._input is None:
            raise RuntimeError("simulate() before set_input_spike_times()")
        feats, sm, _ = self.run_batch(self._input[None], FEATURE_KEYS, want_spike_matrix=True)
        self.spike_matrix = sm[0].cpu().numpy()
        self._features = feats[0].cpu().numpy().reshape(len(FEATURE_KEYS), self.num_output_neurons)

    def extract_features_from_spikes(self) -> dict:
        """dict[str -> (N_out,) float32]; entries that are undefined for a silent neuron are NaN
        here (the batched path returns them as 0, which is what the caller's nan_to_num makes)."""
        if self._features is None:
            raise RuntimeError("extract_features_from_spikes() before simulate()")
        f = {k: self._features[i].copy() for i, k in enumerate(FEATURE_KEYS)}
        n = f['spike_counts']
        for k in ('mean_spike_times', 'first_spike_times', 'last_spike_times'):
            f[k][n < 1] = np.nan
        for k in ('mean_isi', 'isi_variances'):
            f[k][n < 2] = np.nan
        return f
