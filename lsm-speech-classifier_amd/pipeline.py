"""The overlapped hot path as a library component: audio batches -> reservoir feature rows.

The reference chains its stages through files and serial Python loops
(/root/reference/main.py:19-27; clip loops at create_dataset.py:143 and extract_lsm_features.py:78).
Here one STEP = one batch of clips through filterbank -> dB/normalise/resize -> hysteresis encoder ->
LIF reservoir -> features, all on the GPU -- two launches since round 3, the fused front end
(`lsm_gammatone_spikes_f64`) and the reservoir -- and consecutive steps are issued on rotating HIP streams: the
work of a step is ordered on its own stream, the float64 filterbank of step s+1 runs beside the
latency-bound reservoir kernel of step s and refills the CUs that clips finishing early leave idle.
Every step still does all its work; per-step latency grows, throughput rises.
Where HIP has at most 4 hardware queues a plain full step of a served shape is ONE launch (`step_fused`,
include/lsm_hip_step.h): front end and reservoir of a clip in one workgroup, rotating over hw_queues - 1 streams.

`HotPath` owns what used to live in bench.py: the stream rotation, the layout hint for the reservoir
kernel (a launch that shares the chip with other kernels prefers fewer, fatter waves than a lone one:
`waves_per_clip=-1`, decided inside liblsm_hip.so) and the hardware-queue count.
"""
from __future__ import annotations

import contextlib
from typing import NamedTuple

import numpy as np
import torch

from .augment import AugmentChain, StepPlans
from .frontend import (_dev, _host, as_float32, checked_counts, checked_mask, checked_pcm, checked_slots, indexed_device,
                       threshold_tables, RAGGED_HOP)

DEFAULT_STREAMS = 6
# front-end streams of their own (0 = rotation: every step keeps to one stream).  Measured at 128 filters / 1000
# neurons / 256 clips (profiles/r03_stream_topology.txt, r03_priorities_and_stream_counts.txt): 5 + 6 streams 0.65 ms
# per step over 200 steps and 0.80-0.81 over the driver's 20, 4 + 6 streams 0.66 / 0.82-0.83, the rotation over 6
# streams 0.70 / 0.86-0.90 on the same box -- a rotation stream cannot issue its next front end before its own
# reservoir kernel has finished; four one-launch front ends (64 workgroups each, one per CU) cover the chip and the
# fifth is already queued when the first CUs come free.  5 + 6 + the default stream = the 12 hardware queues.
DEFAULT_FE_STREAMS = 5
DEFAULT_HW_QUEUES = 12
RASTER_DEPTH = 4                     # raster buffers per front-end stream (two-stage topology)
# the last batches of a finite list take the low-latency layouts (HotPath.submit(tail=True)); measured at cfg2,
# 20-step bursts (profiles/r04_tail_steps.txt)
TAIL_STEPS = 2
STAGES = ("full", "frontend", "reservoir")
# With this many hardware queues or fewer a full step is ONE launch where the library has it (include/lsm_hip_step.h,
# `step_fused`): the pipeline's 11 streams share the queues, and a reservoir launch that waits at the head of a
# queue for its front end's event holds back the front ends queued behind it (profiles/step_fused_premise.txt).
FUSED_STEP_MAX_HW_QUEUES = 4


STEP_FORMS = {"plain": 0, "masked": 1, "ragged": 2}       # lsm_step_fused_form_supported's `form`


def step_fused_supported(fe, net, n_clips: int, form: str = "plain") -> bool:
    """Whether `step_fused` serves batches of `n_clips` clips of this front end and reservoir (`lsm_step_fused_supported`):
    a gammatone front end of 97..128 filters without redundancy, and a reservoir whose pipeline launch is the dense-row
    kernel with 4 waves per clip and coloured input masks.  Anything else takes the two launches.  `form`: "plain";
    "masked" (`step_fused(mask=...)`: wherever the plain step is served); "ragged" (`step_fused_ragged`: additionally a front
    end that takes ragged batches, `frontend.ragged_refusal`) -- `lsm_step_fused_form_supported`; "ragged-masked"
    (`step_fused_ragged(mask=...)`: wherever the ragged step is served) -- `lsm_step_fused_ragged_masked_supported`."""
    if form not in STEP_FORMS and form != "ragged-masked":
        raise ValueError(f"form must be one of {tuple(STEP_FORMS)}, got {form!r}")
    if getattr(fe, "filterbank", None) != "gammatone" or not fe.will_fuse() or int(n_clips) < 1:
        return False
    from . import _lib
    if form == "plain":
        rc = int(_lib.load().lsm_step_fused_supported(net._handle, int(n_clips), fe.n_filters, fe.nwin, fe.hop, fe.time_bins,
                                                      len(fe.thresholds), fe.redundancy, fe.coef_flags))
    else:
        from .frontend import ragged_refusal
        if form != "masked" and (ragged_refusal(fe.n_samples, fe.time_bins) or fe.ncols != fe.time_bins - 2):
            return False
        if form == "ragged-masked":
            rc = int(_lib.load().lsm_step_fused_ragged_masked_supported(
                net._handle, int(n_clips), fe.n_filters, fe.nwin, fe.hop, fe.time_bins, len(fe.thresholds), fe.redundancy,
                fe.coef_flags))
            if rc < 0:
                _lib.check(rc, "lsm_step_fused_ragged_masked_supported")
            return rc == 1
        rc = int(_lib.load().lsm_step_fused_form_supported(net._handle, int(n_clips), fe.n_filters, fe.nwin, fe.hop,
                                                           fe.time_bins, len(fe.thresholds), fe.redundancy, fe.coef_flags,
                                                           STEP_FORMS[form]))
    if rc < 0:
        _lib.check(rc, "lsm_step_fused_supported")
    return rc == 1


def _step_outputs(fe, net, audio, feature_keys, stats_out, features_out):
    """What the step launches share: the checked batch, its key ids and the feature rows they write (`features_out` or None:
    the caller allocates inside its device context)."""
    from .snn import _check_stats_out, _select_keys
    audio = fe._audio(audio)
    B = int(audio.shape[0])
    keys, key_ids = _select_keys(feature_keys)
    shape = (B, len(keys) * net.num_output_neurons)
    if features_out is not None:
        if (features_out.dtype != torch.float32 or tuple(features_out.shape) != shape or not features_out.is_contiguous()
                or features_out.device != audio.device):
            raise ValueError(f"features_out must be a contiguous float32 {shape} tensor on {audio.device}")
    _check_stats_out(stats_out, B, audio.device)
    return audio, B, keys, key_ids, shape


def step_fused(fe, net, audio, feature_keys=None, stats_out=None, features_out=None, workspace=None, mask=None):
    """One step in ONE launch on the current stream (`lsm_step_fused_f64`): audio (B, n_samples) float32 on the device ->
    feature rows (B, n_keys * N_out) float32, bit for bit ``net.run_batch(fe.encode(audio), feature_keys)[0]``; no raster is
    written.  `stats_out` / `features_out`: as `SNN.run_batch`'s; `workspace`: as `SpikeFrontEnd.encode`'s (from
    `fe.new_workspace(B)`).  `mask`: a `frontend.MaskPlan` of the batch's clips (SPEC.md §1.13), checked (`checked_mask`) and
    uploaded on the current stream as `encode(mask=...)` does: the launch is `lsm_step_fused_masked_f64` and the rows are those
    of ``net.run_batch(fe.encode(audio, mask=mask), feature_keys)[0]``; None makes exactly the unmasked call.  A shape the
    launch does not serve (`step_fused_supported`) raises: the caller makes the two launches."""
    from . import _lib
    from .frontend import upload_mask
    if mask is not None:
        checked_mask(mask, 1 if getattr(audio, "ndim", 2) == 1 else len(audio), fe.n_filters, fe.time_bins)
    audio, B, keys, key_ids, shape = _step_outputs(fe, net, audio, feature_keys, stats_out, features_out)
    on, off = threshold_tables(fe.thresholds, fe.gap, np.float64)
    with torch.cuda.device(fe.device):
        feats = features_out if features_out is not None else torch.empty(shape, dtype=torch.float32, device=fe.device)
        ws, ws_bytes = fe._workspace_for(B, workspace)
        args = (net._handle, _dev(audio), B, fe.n_samples, _dev(fe.coefs), fe.n_filters, fe.nwin, fe.hop, fe.ncols, fe.time_bins,
                _host(on), _host(off), len(on), fe.redundancy, _dev(ws), ws_bytes, fe.coef_flags, _host(key_ids), len(keys),
                _dev(feats), _dev(stats_out))
        if mask is None:
            _lib.check(fe.lib.lsm_step_fused_f64(*args, fe._stream()), "lsm_step_fused_f64")
        else:
            fm, tm = upload_mask(mask, B, fe.n_filters, fe.time_bins, fe.device)
            _lib.check(fe.lib.lsm_step_fused_masked_f64(*args, _dev(fm), _dev(tm), fe._stream()), "lsm_step_fused_masked_f64")
    return feats


def step_fused_ragged(fe, net, audio, bins, feature_keys=None, stats_out=None, features_out=None, workspace=None, mask=None):
    """One step on clips of different lengths in ONE launch on the current stream (`lsm_step_fused_ragged_f64`): clip b is the
    first ``160 * bins[b]`` samples of its row and runs ``bins[b] * n_thr`` reservoir steps; its feature row is, bit for bit,
    that of ``raster, steps = fe.encode_ragged(audio, bins)`` followed by ``net.run_batch(raster, feature_keys,
    lengths=steps)[0]``.  `bins`: B host integers, each 0 or 3 .. time_bins (checked), or an int32 device tensor (not read:
    the kernel clamps it), as `encode_ragged` takes them.  A clip of 0 bins leaves its row of `features_out` and of
    `stats_out` as it was (a row of a tensor allocated here is then uninitialised).  The other parameters are `step_fused`'s.
    `mask`: a `frontend.MaskPlan` at the launch's strides whose time bits name the bins of each clip's own length (SPEC.md
    §1.16, `frontend.mask_plan_ragged`): the launch is `lsm_step_fused_ragged_masked_f64` and the rows are those of
    ``fe.encode_ragged(audio, bins, mask=mask)`` followed by the ragged run; None makes exactly the unmasked call.  Needs
    `step_fused_supported(fe, net, B, form="ragged")` (with a mask: ``form="ragged-masked"``)."""
    from . import _lib
    from .frontend import checked_ragged_bins, ragged_refusal, upload_mask
    why = ragged_refusal(fe.n_samples, fe.time_bins)
    if why:
        raise ValueError(why)
    if mask is not None:
        checked_mask(mask, 1 if getattr(audio, "ndim", 2) == 1 else len(audio), fe.n_filters, fe.time_bins)
    checked_ragged_bins(bins, 1 if getattr(audio, "ndim", 2) == 1 else len(audio), fe.time_bins)     # before any device work
    audio, B, keys, key_ids, shape = _step_outputs(fe, net, audio, feature_keys, stats_out, features_out)
    on, off = threshold_tables(fe.thresholds, fe.gap, np.float64)
    with torch.cuda.device(fe.device):
        bins_dev = fe._device_bins(bins, B)
        feats = features_out if features_out is not None else torch.empty(shape, dtype=torch.float32, device=fe.device)
        ws, ws_bytes = fe._workspace_for(B, workspace)
        args = (net._handle, _dev(audio), B, fe.n_samples, _dev(fe.coefs), fe.n_filters, fe.nwin, fe.hop, fe.ncols, fe.time_bins,
                _dev(bins_dev), _host(on), _host(off), len(on), fe.redundancy, _dev(ws), ws_bytes, fe.coef_flags, _host(key_ids),
                len(keys), _dev(feats), _dev(stats_out))
        if mask is None:
            _lib.check(fe.lib.lsm_step_fused_ragged_f64(*args, fe._stream()), "lsm_step_fused_ragged_f64")
        else:
            fm, tm = upload_mask(mask, B, fe.n_filters, fe.time_bins, fe.device)
            _lib.check(fe.lib.lsm_step_fused_ragged_masked_f64(*args, _dev(fm), _dev(tm), fe._stream()),
                       "lsm_step_fused_ragged_masked_f64")
    return feats


def step_fused_state_supported(fe, net, n_clips: int) -> bool:
    """Whether `step_fused_from` and `step_fused_segments` serve batches of `n_clips` clips of this front end and reservoir
    (`lsm_step_fused_state_supported`): the shapes of the plain `step_fused`."""
    if getattr(fe, "filterbank", None) != "gammatone" or not fe.will_fuse() or int(n_clips) < 1:
        return False
    from . import _lib
    rc = int(_lib.load().lsm_step_fused_state_supported(net._handle, int(n_clips), fe.n_filters, fe.nwin, fe.hop, fe.time_bins,
                                                        len(fe.thresholds), fe.redundancy, fe.coef_flags))
    if rc < 0:
        _lib.check(rc, "lsm_step_fused_state_supported")
    return rc == 1


def _front_args(fe, net, audio, B, workspace):
    """The front-end half of a state step's argument list (up to and including coef_flags); inside the device context."""
    on, off = threshold_tables(fe.thresholds, fe.gap, np.float64)
    ws, ws_bytes = fe._workspace_for(B, workspace)
    return (net._handle, _dev(audio), B, fe.n_samples, _dev(fe.coefs), fe.n_filters, fe.nwin, fe.hop, fe.ncols, fe.time_bins,
            _host(on), _host(off), len(on), fe.redundancy, _dev(ws), ws_bytes, fe.coef_flags), (on, off, ws)


def step_fused_from(fe, net, audio, feature_keys=None, state=None, state_out=None, stats_out=None, features_out=None,
                    workspace=None):
    """One step that continues a run, in ONE launch on the current stream (`lsm_step_fused_from_f64`, SPEC.md §4f): bit for
    bit ``net.run_batch(fe.encode(audio), feature_keys, state=state, state_out=state_out)[0]`` -- the feature rows of the whole
    run so far, `stats_out` its totals, the state advanced by ``fe.n_steps`` steps in place (or written to `state_out`) -- and
    no raster is written.  Without `state` it is `step_fused`.  The other parameters are `step_fused`'s; masks and ragged
    batches are not offered.  Needs `step_fused_state_supported(fe, net, B)`."""
    from . import _lib
    n = 1 if getattr(audio, "ndim", 2) == 1 else len(audio)
    first_step, src, dst = net._continuation(state, state_out, n)        # before any device work
    audio, B, keys, key_ids, shape = _step_outputs(fe, net, audio, feature_keys, stats_out, features_out)
    with torch.cuda.device(fe.device):
        feats = features_out if features_out is not None else torch.empty(shape, dtype=torch.float32, device=fe.device)
        front, keep = _front_args(fe, net, audio, B, workspace)
        _lib.check(fe.lib.lsm_step_fused_from_f64(*front, int(first_step), _dev(src), _dev(dst), _host(key_ids), len(keys),
                                                  _dev(feats), _dev(stats_out), fe._stream()), "lsm_step_fused_from_f64")
    if state is not None:
        (state_out or state).steps_done = state.steps_done + fe.n_steps
    return feats


def step_fused_segments(fe, net, audio, segment_steps: int, feature_keys=None, state=None, state_out=None,
                        want_records: bool = False, stats_out=None, rows_out=None, workspace=None):
    """One step with its features per time segment, in ONE launch on the current stream (`lsm_step_fused_segments_f64`,
    SPEC.md §4f).  Returns the rows float32 (B, G, n_keys * N_out), G = ``fe.n_steps // segment_steps``, bit for bit
    ``net.run_segments(fe.encode(audio), segment_steps, feature_keys, state=state, state_out=state_out)``: the workgroup of a
    clip closes its segment records and writes the clip's rows itself; with `want_records` also the (B, G, N_out, 4) int32
    records of ``net.run_segment_records``.  `rows_out`: a contiguous float32 (B, G, n_keys * N_out) tensor to write into.
    `state` / `state_out` / `stats_out` / `workspace`: as `step_fused_from`'s.  Needs `step_fused_state_supported`."""
    from . import _lib
    from .snn import _check_stats_out, _select_keys
    S, T = int(segment_steps), int(fe.n_steps)
    if S < 1 or T < 1 or T % S != 0:
        raise _lib.LsmHipError(f"segment_steps = {S} must be >= 1 and divide the clip's {T} steps")
    n = 1 if getattr(audio, "ndim", 2) == 1 else len(audio)
    first_step, src, dst = net._continuation(state, state_out, n)        # before any device work
    audio = fe._audio(audio)
    B, G = int(audio.shape[0]), T // S
    keys, key_ids = _select_keys(feature_keys)
    shape = (B, G, len(keys) * net.num_output_neurons)
    if rows_out is not None:
        if (rows_out.dtype != torch.float32 or tuple(rows_out.shape) != shape or not rows_out.is_contiguous()
                or rows_out.device != audio.device):
            raise ValueError(f"rows_out must be a contiguous float32 {shape} tensor on {audio.device}")
    _check_stats_out(stats_out, B, audio.device)
    with torch.cuda.device(fe.device):
        rows = rows_out if rows_out is not None else torch.empty(shape, dtype=torch.float32, device=fe.device)
        # the records are the kernel's own working set (it folds and reads them back): always a buffer, returned when asked for
        records = torch.empty((B, G, net.num_output_neurons, 4), dtype=torch.int32, device=fe.device)
        front, keep = _front_args(fe, net, audio, B, workspace)
        # (cumulative features are not asked for: features_out NULL is the library's "no cumulative rows" only with n_keys 0,
        #  so the keys go with a scratch row buffer of their own); without keys (`feature_keys=()`: the records alone) the
        #  launch has neither cumulative rows nor segment rows
        cumulative = torch.empty((B, shape[2]), dtype=torch.float32, device=fe.device) if keys else None
        _lib.check(fe.lib.lsm_step_fused_segments_f64(*front, int(first_step), _dev(src), _dev(dst),
                                                      _host(key_ids) if keys else None, len(keys), _dev(cumulative),
                                                      _dev(stats_out), S, _dev(records), _dev(rows if keys else None),
                                                      fe._stream()), "lsm_step_fused_segments_f64")
    if state is not None:
        (state_out or state).steps_done = state.steps_done + T
    return (rows, records) if want_records else rows


def configure_hardware_queues(n: int = DEFAULT_HW_QUEUES) -> int:
    """The HIP runtime multiplexes streams onto 4 hardware queues by default, and kernels of streams that
    share a queue serialise: with 4 queues three streams are the optimum, with 8-12 six streams overlap
    (0.96 -> 0.72 ms per step; 12 also leave RCCL's stream a queue of its own).  The variable is read when
    HIP initialises, so it must be set BEFORE the first CUDA/HIP call of the process: importing the package
    does that (`lsm_speech_classifier_amd.__init__`, an existing GPU_MAX_HW_QUEUES wins; a warning when HIP
    was already up).  Returns the number of queues IN FORCE for this process, which is what `HotPath.hw_queues`
    and the bench line report -- 4 when the package was imported too late, whatever the variable says now."""
    from . import EFFECTIVE_HW_QUEUES
    return int(EFFECTIVE_HW_QUEUES)


class RasterRing:
    """What one front-end slot of the two-stage topology owns for batches of `n_clips`: RASTER_DEPTH raster buffers
    handed round behind events -- a buffer is written again only after the reservoir launch that read it has finished (a
    GPU-side wait of the front-end stream, never a host wait) -- and the slot's front-end scratch.  Built on the
    front-end stream, so that the allocator counts the buffers as that stream's."""

    def __init__(self, fe, n_clips: int, device):
        self.buffers = [torch.empty((n_clips, fe.n_channels, fe.n_steps), dtype=torch.uint8, device=device)
                        for _ in range(RASTER_DEPTH)]
        self.free = [None] * RASTER_DEPTH               # per buffer: the event of its last reader
        self.next = 0
        self.workspace = fe.new_workspace(n_clips)      # one per front-end stream

    def acquire(self, fe_stream) -> torch.Tensor:
        """The next buffer, once `fe_stream` has been made to wait for that buffer's last reader."""
        bi = self.next
        self.next = (bi + 1) % RASTER_DEPTH
        if self.free[bi] is not None:
            fe_stream.wait_event(self.free[bi])
        return self.buffers[bi]

    def release(self, reader_stream) -> None:
        """The launch just issued on `reader_stream` is the last reader of the buffer `acquire` handed out last."""
        bi = (self.next - 1) % RASTER_DEPTH
        self.free[bi] = torch.cuda.Event()
        self.free[bi].record(reader_stream)


def _get_or_make(cache: dict, key, make):
    """``cache[key]``, made by ``make()`` on first use: the buffers a stream slot of the pipeline owns."""
    got = cache.get(key)
    if got is None:
        got = cache[key] = make()
    return got


class _Step(NamedTuple):
    """One `HotPath.submit`, as the topologies take it: `submit`'s arguments, its four plans packed and checked."""
    audio: object
    stats_out: object
    after: object
    out: object
    stage: str
    tail: bool
    plans: StepPlans


class HotPath:
    """fe: frontend.SpikeFrontEnd, net: snn.SNN (same device).  `streams` = reservoir streams (1 = serial:
    everything on the current stream); `fe_streams` = front-end streams of their own (0 = rotation: a step keeps to
    one of the `streams`; None = DEFAULT_FE_STREAMS).  `time_segments` = K > 1: a step's reservoir launch is the segmented
    one (`SNN.run_segments`, K segments of T // K steps, SPEC.md §4b) and a clip's row is its K segment rows side by side
    (segment-major, then key-major: K times the columns); 1 = the whole-clip row, the calls of a pipeline without it.
    `speed`, `reverb`, `mixer` = a `frontend.SpeedPerturber`, `Reverberator`, `NoiseMixer`, the stages of the pipeline's
    `augment.AugmentChain`: a step submitted with `speed=`, `reverb=` or `mix=` (a `frontend.SpeedPlan`, `ReverbPlan`, `MixPlan`
    of its clips) is played at its clips' speeds (SPEC.md §1.12), then convolved with their room responses (§1.11), then
    corrupted (§1.10) on the device before its front end; a step without a plan launches what it launches without the stage.
    With at most FUSED_STEP_MAX_HW_QUEUES hardware queues a full step without any of these, of a shape `step_fused_supported`
    accepts, is one launch (`_submit_fused`); `time_reservoir`'s event pair then brackets that launch, front end included.
    `fused_forms` = True: there a masked step is one launch too (`lsm_step_fused_masked_f64`), and a step with speed, reverb or
    mixer runs its augmentation launches on the fused rotation stream and then the one launch; the rows are byte for byte
    those of the default routes.  Off by default (profiles/step_fused_forms.txt).  With `time_segments` = K > 1 and
    `fused_forms` = True a full step without mixer, reverb, speed or mask, of a shape `step_fused_state_supported` accepts, is
    one launch as well (`step_fused_segments`: the kernel writes the step's K rows itself) instead of front end, segmented
    reservoir launch and fold (profiles/step_fused_state.txt)."""

    def __init__(self, fe, net, feature_keys=None, streams: int = DEFAULT_STREAMS,
                 waves_per_clip: int | None = None, time_reservoir: bool = False,
                 fe_streams: int | None = None, time_segments: int = 1, mixer=None, reverb=None, speed=None,
                 fused_forms: bool = False):
        if indexed_device(fe.device) != indexed_device(net.device):
            raise ValueError(f"front end on {fe.device}, reservoir on {net.device}")
        self.chain = AugmentChain(speed, reverb, mixer)    # the stages a step's plans (`submit`) run through, in its order
        self.chain.check_device(fe.device)
        if fe.n_channels != net.n_channels:
            raise ValueError(f"front end has {fe.n_channels} channels, reservoir expects {net.n_channels}")
        self.fe, self.net = fe, net
        self.device = indexed_device(fe.device)   # so that a device-resident batch is recognised as such (not copied again)
        self.feature_keys = feature_keys
        self.time_segments = int(time_segments)
        if self.time_segments < 1 or fe.n_steps % self.time_segments:
            raise ValueError(f"time_segments = {time_segments} must be >= 1 and divide the front end's {fe.n_steps} steps")
        self.n_streams = max(1, int(streams))
        # inside the rotation the reservoir launch shares the chip: let the library pick for that case
        self.waves_per_clip = (-1 if self.n_streams > 1 else 0) if waves_per_clip is None else int(waves_per_clip)
        self.time_reservoir = bool(time_reservoir)
        self.hw_queues = configure_hardware_queues()
        # Stream topology.  fe_streams == 0 ("rotation"): step s runs front end AND reservoir on stream s % streams, so
        # the stream cannot issue its next front end before this step's reservoir kernel has finished.
        # fe_streams > 0 ("two stages"): the front ends go round `fe_streams` streams of their own and never wait
        # for a reservoir kernel; step s's reservoir launch goes to reservoir stream s % streams behind an event.
        self.n_fe_streams = (DEFAULT_FE_STREAMS if fe_streams is None else max(0, int(fe_streams))) if self.n_streams > 1 else 0
        with torch.cuda.device(self.device):
            self.streams = ([torch.cuda.Stream(device=self.device) for _ in range(self.n_streams)]
                            if self.n_streams > 1 else [None])
            self.fe_streams = [torch.cuda.Stream(device=self.device) for _ in range(self.n_fe_streams)]
        self._fe_done = []                  # events of the front ends issued, newest last (two-stage topology)
        # Back-pressure: the host enqueues a step in ~0.1 ms, the GPU runs it in ~0.64: without a bound a long run is
        # enqueued thousands of steps ahead and everything a step allocates stays reserved until the GPU gets there
        # (measured before the pipeline owned its raster buffers: 12 GB after 3000 steps).  submit() therefore waits
        # for step s - max_ahead before it issues step s; the GPU keeps max_ahead steps queued, far more than it overlaps.
        self.max_ahead = max(16, 4 * (self.n_streams + self.n_fe_streams))
        # Two-stage topology: a fused full step's raster and front-end scratch live in buffers the pipeline owns, one
        # `RasterRing` per front-end stream.  Allocating them per step from torch's allocator needs the block of step s to
        # stay reserved until its reservoir launch has finished on ANOTHER stream (`record_stream`): memory then grows with
        # the steps enqueued ahead and a burst allocates inside the timed path.  Throughput is the same either way
        # (profiles/r03_pipeline_buffer_pool.txt); the rings make the steady path free of allocator calls.
        self._rasters = {}                  # (front-end slot, batch size) -> RasterRing
        # One launch per step where queues are scarce (FUSED_STEP_MAX_HW_QUEUES): a full step without mixer, reverb, speed,
        # mask or time segments, of a shape the library serves, rotates over min(hw_queues - 1, streams) of the reservoir
        # streams and makes one launch there -- no front-end stream, no event, no raster.  One queue is left to the stream the
        # caller submits from: with as many rotation streams as queues one of them shares its queue with that stream, and
        # at 4 queues the step took 1.03 ms over 4 streams against 0.84 over 3 (and 0.96 over 2;
        # profiles/step_fused_ab.txt).  With more queues nothing changes.
        # `fused_forms` (off unless asked for; cfg2, 4 queues: a masked step 1.00 -> 0.82 ms, mixer + mask 1.29 -> 0.95 ms,
        # profiles/step_fused_forms.txt, which also says why it is not the default yet): a masked step takes the masked launch
        # (`step_fused(mask=...)`), and a pipeline with a mixer, a reverberator or a speed perturber keeps the fused step and runs
        # a step's augmentation chain on the fused rotation stream in front of it.  The rows are those of the two launches.
        self.fused_forms = bool(fused_forms)
        self.fused_step = (self.n_streams > 1 and self.hw_queues <= FUSED_STEP_MAX_HW_QUEUES and self.time_segments == 1
                           and (self.fused_forms or (mixer is None and reverb is None and speed is None)))
        # `fused_forms` with time segments: the step's K rows from one launch (`_submit_fused_segments`); `fused_step` stays
        # what it says about the whole-clip step
        self.fused_segments = (self.n_streams > 1 and self.hw_queues <= FUSED_STEP_MAX_HW_QUEUES and self.time_segments > 1
                               and self.fused_forms and mixer is None and reverb is None and speed is None)
        self.n_fused_streams = max(1, min(self.hw_queues - 1, self.n_streams))
        self._fused_ok = {}                 # (batch size, form) -> step_fused_supported
        # what a slot owns beside its raster ring (`_owned`): ("h2d" / "speed" / "reverb" / "mix", slot, batch shape) -> the
        # upload's / that launch's output buffer, ("workspace", slot, batch size) -> the fused step's front-end scratch
        self._buffers = {}
        self._in_flight = []                # one event per submitted step, on the stream its last launch went to
        self._step = 0
        self.reservoir_events = []          # (start, end) HIP event pairs, one per submitted step (time_reservoir)

    # ---- one step ---------------------------------------------------------------------------
    @contextlib.contextmanager
    def _timed(self):
        """With `time_reservoir`: an event pair on the current stream around the launches made inside."""
        if not self.time_reservoir:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self.reservoir_events.append((e0, e1))

    def _one(self, x, step, stage=None):
        """The launches of `step` (or only those of `stage`) over `x` on the current stream."""
        stage = stage or step.stage
        rasters = x if stage == "reservoir" else self.fe.encode(x, **step.plans.mask_keyword())
        if stage == "frontend":
            return rasters
        # a tail step's reservoir launch meets a draining GPU: the layout of a lone launch (more, thinner waves) when the
        # choice is the library's (profiles/r04_tail_steps.txt)
        wpc = 0 if (step.tail and self.waves_per_clip == -1) else self.waves_per_clip
        with self._timed():
            if self.time_segments > 1:
                K, B = self.time_segments, int(rasters.shape[0])
                return self.net.run_segments(rasters, int(rasters.shape[2]) // K, self.feature_keys, waves_per_clip=wpc,
                                             stats_out=step.stats_out,
                                             features_out=step.out.view(B, K, -1) if step.out is not None else None).view(B, -1)
            return self.net.run_batch(rasters, self.feature_keys, waves_per_clip=wpc, stats_out=step.stats_out,
                                      features_out=step.out)[0]

    def submit(self, audio, stats_out=None, after=None, out=None, stage: str = "full", tail: bool = False,
               mix=None, reverb=None, speed=None, mask=None):
        """Issue one step on the next stream of the rotation.  `audio`: (B, n_samples) float32 -- device tensor,
        or pinned/pageable host tensor / NumPy array, uploaded on the step's own stream.  Returns (features
        (B, n_keys*N_out) device tensor, stream it is produced on); the caller waits (`stream.synchronize()`,
        `HotPath.synchronize()`, or an event) before reading the features.

        Ordering of a DEVICE input: the step's stream waits for `after` when that event is given, otherwise for
        everything the current stream of the device has issued so far (so a batch produced there just before
        `submit()` is never read early); host inputs are copied on the step's stream itself.
        `out`: write the rows into this (B, n_feat) float32 tensor (a slice of a gather buffer) instead of a new one.
        `stage`: "full"; "frontend" (returns the uint8 rasters; `out`/`stats_out` unused); "reservoir" (`audio` IS a
        uint8 raster batch (B, C, T) on the device) -- the same rotation, launches and layout hint as a full step,
        so that per-stage timings go through the code the headline goes through.
        `tail`: the caller has (almost) nothing to submit behind this step -- one of the last batches of a finite list
        (`run()` sets it for the last `TAIL_STEPS` batches).  The step then takes the low-latency layouts: the front end
        with one chain per lane (twice the waves, each half as long), the reservoir launch as a lone launch would be laid
        out.  At the end of a burst the last front end otherwise runs alone on a quarter of the chip for ~2 ms while the
        rest drains (profiles/r04_tail_steps.txt); inside a long run the normal layouts use fewer CU-cycles.
        `speed`, `reverb`, `mix`: a `frontend.SpeedPlan` / `ReverbPlan` / `MixPlan` of this step's B clips (each needs the
        pipeline's stage of that kind): one more launch each (`AugmentChain.apply`: speed, reverberation, mixer) on the stream
        that runs the step's front end, between the upload and `encode`, each into a buffer the stream slot owns; no host
        synchronisation.
        `mask`: a `frontend.MaskPlan` of this step's B clips (SPEC.md §1.13): the step's front end is the masked entry point
        -- the mask acts inside the encoder, behind every corruption of the audio -- and still writes into the pipeline's
        raster rings; the words are uploaded on the front end's stream, no host synchronisation.  A step without it launches
        what it always did.
        Back-pressure: when `max_ahead` earlier steps have not finished, submit() first waits for the oldest."""
        step = _Step(audio, stats_out, after, out, stage, tail, StepPlans(speed, reverb, mix, mask))
        self.chain.refuse(step.plans, front_end=stage != "reservoir")
        if mask is not None:
            if stage == "reservoir":
                raise ValueError("submit(mask=...) needs a step that has a front end")
            checked_mask(mask, len(audio), self.fe.n_filters, self.fe.time_bins)
        if stage not in STAGES:
            raise ValueError(f"stage must be one of {STAGES}, got {stage!r}")
        slot = self._step % self.n_streams
        self._step += 1
        while len(self._in_flight) >= self.max_ahead:
            self._in_flight.pop(0).synchronize()
        res, st = self._submit(slot, step)
        if st is not None and self.n_streams > 1:
            ev = torch.cuda.Event()
            ev.record(st)
            self._in_flight.append(ev)
        return res, st

    def _submit(self, slot, step):
        """The step on the topology that serves it."""
        masked = step.plans.mask is not None
        if self.n_streams == 1:
            topology = self._submit_serial
        elif step.stage == "full" and (not masked or self.fused_forms) and self._takes_fused_step(step.audio, masked):
            topology = self._submit_fused
        elif step.stage == "full" and not masked and self._takes_fused_segments(step.audio):
            topology = self._submit_fused_segments
        elif self.n_fe_streams and step.stage != "reservoir":
            topology = self._submit_two_stages
        else:
            topology = self._submit_rotation
        return topology(slot, step)

    def _wait_for_input(self, stream, cur, audio, after) -> None:
        """The ordering of a device input (`submit`): `stream` waits for `after`, or for what `cur` has issued so far."""
        if after is not None:
            stream.wait_event(after)
        elif torch.is_tensor(audio) and audio.device == self.device:
            stream.wait_stream(cur)

    def _submit_serial(self, slot, step):
        """Everything on the current stream."""
        cur = torch.cuda.current_stream(self.device)
        if step.after is not None:
            cur.wait_event(step.after)
        with torch.cuda.device(self.device):
            return self._one(self._input(step, slot), step), cur

    def _submit_rotation(self, slot, step):
        """The step keeps to reservoir stream `slot`: its front end, then its reservoir launch."""
        st, cur = self.streams[slot], torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            self._wait_for_input(st, cur, step.audio, step.after)
            return self._one(self._input(step, slot), step), st

    def _submit_two_stages(self, slot, step):
        """The front end on the next front-end stream, the reservoir launch on reservoir stream `slot` behind an event."""
        fslot = (self._step - 1) % self.n_fe_streams
        st, fst, cur = self.streams[slot], self.fe_streams[fslot], torch.cuda.current_stream(self.device)
        stage = step.stage
        with torch.cuda.device(self.device):
            with torch.cuda.stream(fst):
                self._wait_for_input(fst, cur, step.audio, step.after)
                low_latency = self._low_latency(step.tail)
                x = self._input(step, ("fe", fslot))
                # the front end's own decision (mel branch, > 1024 filters and LSM_FRONTEND_SPLIT=1 take the split
                # route, which allocates its raster on the front-end stream): only the fused launch of a full step
                # writes into the pipeline's rings, everything else goes through record_stream below
                ring, owned = None, {}
                if stage == "full" and self.fe.will_fuse():
                    ring = _get_or_make(self._rasters, (fslot, int(x.shape[0])),
                                        lambda: RasterRing(self.fe, int(x.shape[0]), self.device))
                    owned = dict(raster_out=ring.acquire(fst), workspace=ring.workspace)
                # `share_lds` stays off: beside the ring-row kernel at 4000 neurons (64 KB of LDS per clip, two per CU)
                # the whole path runs 6.37-6.40 ms per step without the front end's LDS reservation against 6.26-6.28
                # with it (profiles/r04_cfg4_frontend_lds_placement.txt)
                rasters = self.fe.encode(x, low_latency=low_latency, **owned, **step.plans.mask_keyword())
                done = torch.cuda.Event()
                done.record(fst)
                self._fe_done.append(done)
                if stage == "frontend":
                    return rasters, fst
            if ring is None:
                rasters.record_stream(st)      # allocated on the front-end stream, read on the reservoir stream
            with torch.cuda.stream(st):
                st.wait_event(done)
                feats = self._one(rasters, step, "reservoir")
                if ring is not None:
                    ring.release(st)
                return feats, st

    def _takes_fused_step(self, audio, masked: bool = False) -> bool:
        """Whether a full step over `audio` is the one-launch step (decided once per batch size and form)."""
        form = "masked" if masked else "plain"
        return self.fused_step and _get_or_make(self._fused_ok, (int(len(audio)), form),
                                                lambda: step_fused_supported(self.fe, self.net, int(len(audio)), form))

    def _submit_fused(self, slot, step):
        """The whole step as one launch (`step_fused`) on stream (step number) % n_fused_streams.  With `time_reservoir` the
        event pair brackets that launch: front end and reservoir of the step together."""
        slot = (self._step - 1) % self.n_fused_streams
        st, cur = self.streams[slot], torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            self._wait_for_input(st, cur, step.audio, step.after)
            x = self._input(step, slot)
            B = int(x.shape[0])
            ws = _get_or_make(self._buffers, ("workspace", slot, B), lambda: self.fe.new_workspace(B))
            with self._timed():
                return step_fused(self.fe, self.net, x, self.feature_keys, stats_out=step.stats_out, features_out=step.out,
                                  workspace=ws, **step.plans.mask_keyword()), st

    def _takes_fused_segments(self, audio) -> bool:
        """Whether a full step over `audio` is the one-launch segmented step (decided once per batch size)."""
        return self.fused_segments and _get_or_make(self._fused_ok, (int(len(audio)), "segments"),
                                                    lambda: step_fused_state_supported(self.fe, self.net, int(len(audio))))

    def _submit_fused_segments(self, slot, step):
        """The whole step with its `time_segments` rows as one launch (`step_fused_segments`), on the fused rotation."""
        slot = (self._step - 1) % self.n_fused_streams
        st, cur = self.streams[slot], torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            self._wait_for_input(st, cur, step.audio, step.after)
            x = self._input(step, slot)
            B, K = int(x.shape[0]), self.time_segments
            ws = _get_or_make(self._buffers, ("workspace", slot, B), lambda: self.fe.new_workspace(B))
            with self._timed():
                return step_fused_segments(self.fe, self.net, x, self.fe.n_steps // K, self.feature_keys,
                                           stats_out=step.stats_out,
                                           rows_out=step.out.view(B, K, -1) if step.out is not None else None,
                                           workspace=ws).view(B, -1), st

    def _low_latency(self, tail: bool) -> bool:
        """Whether this step's fused gammatone front end goes out in the low-latency layout: on a tail step, and when it
        meets an idle GPU -- none of this pipeline's front ends still in flight: the first step after a synchronisation,
        or a caller that submits rarely.  It is then done after 1.47 instead of 2.43 ms, and -- what matters for a short
        burst of steps -- the burst's front ends no longer run in lockstep rounds of four that all end, and all release
        their reservoir launches, together (profiles/r03_low_latency_layout_when_idle.txt)."""
        self._fe_done = [ev for ev in self._fe_done[-8:] if not ev.query()]
        return self.fe.filterbank == "gammatone" and self.fe.will_fuse() and (tail or not self._fe_done)

    def _owned(self, kind: str, slot, shape) -> torch.Tensor:
        """The float32 buffer of `shape` that stream slot `slot` owns for its uploads ("h2d") or for the output of one of its
        augmentation launches ("speed", "reverb", "mix"); made on first use, on the current stream."""
        return _get_or_make(self._buffers, (kind, slot, tuple(shape)),
                            lambda: torch.empty(tuple(shape), dtype=torch.float32, device=self.device))

    def _input(self, step, slot):
        """What the step's first launch reads, on the current stream: a raster batch as it is; audio uploaded when it lies
        on the host (an asynchronous copy), then through the augmentation chain for the plans the step has."""
        audio = step.audio
        if step.stage == "reservoir":
            return audio
        if isinstance(audio, np.ndarray):
            audio = as_float32(audio)
        if audio.device != self.device:
            host, audio = audio, self._owned("h2d", slot, audio.shape)
            audio.copy_(host, non_blocking=True)
        return self.chain.apply(audio, step.plans, lambda stage, shape: self._owned(stage, slot, shape))

    def prime(self, audio, stage: str = "full", min_ms: float = 0.0):
        """One untimed step on EVERY stream of the pipeline, then a synchronisation: each stream's first use
        pays for its allocator pool (torch caches device memory per stream: the first `encode` on a stream
        calls hipMalloc, which stalls every queue), for the pipeline's own buffers, for the first launch on its
        hardware queue and for the kernels' one-off attribute calls.  Part of set-up; afterwards a step makes no
        runtime call but launches and (host inputs) one asynchronous copy.

        `min_ms` > 0: keep submitting untimed steps until that much time has passed -- the GPU's clock governor
        needs tens of milliseconds of load to reach the clock the pipeline then holds; a burst of steps that
        starts right after a set-up phase (seconds of host work, an idle GPU) otherwise runs its first ~15 ms
        6-9 % slower than the same steps in the middle of a long run (profiles/r03_clock_ramp.txt)."""
        import time
        self.fork_from_current()
        events = self.reservoir_events
        self.reservoir_events = []
        t0 = time.perf_counter()
        n = 0
        while n < max(self.n_streams, self.n_fe_streams) or (time.perf_counter() - t0) * 1e3 < min_ms:
            self.submit(audio, stage=stage)
            n += 1
            if n % 8 == 0:                       # let the GPU catch up: the loop is timed by work done, not enqueued
                self._in_flight and self._in_flight[-1].synchronize()
        self.synchronize()
        self.reservoir_events = events
        return n

    def fork_from_current(self):
        """Make every stream of the rotation wait for what the current stream has issued so far
        (inputs produced there, e.g. an upload or a reservoir build)."""
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams + self.fe_streams:
            if st is not None:
                st.wait_stream(cur)

    def join_to_current(self):
        """The reverse edge: the current stream waits for everything the rotation has issued (no host
        synchronisation) -- e.g. before ONE collective over the rows of many steps."""
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams + self.fe_streams:
            if st is not None:
                cur.wait_stream(st)

    def synchronize(self):
        self._in_flight.clear()
        for st in self.streams + self.fe_streams:
            if st is not None:
                st.synchronize()
        torch.cuda.current_stream(self.device).synchronize()

    # ---- many steps -------------------------------------------------------------------------
    def run(self, audio_batches, out: torch.Tensor | None = None, mixes=None, reverbs=None, speeds=None,
            masks=None) -> torch.Tensor:
        """Feature rows of every batch, in order, as one (n_clips, n_feat) device tensor.  `audio_batches`
        is an iterable of (B_i, n_samples) arrays/tensors (host or device); `mixes`, when given, an iterable of one
        `frontend.MixPlan` per batch (`submit(mix=...)`); `reverbs` likewise one `frontend.ReverbPlan` per batch, `speeds` one
        `frontend.SpeedPlan` per batch, `masks` one `frontend.MaskPlan` per batch (`submit(mask=...)`)."""
        its = [None if plans is None else iter(plans) for plans in (speeds, reverbs, mixes, masks)]

        def each_batch():
            while True:             # a list, not a generator expression: `next` runs here, once per batch
                yield StepPlans(*[None if it is None else next(it) for it in its])

        return self._run(audio_batches, each_batch(), out)

    def _run(self, audio_batches, plans, out=None) -> torch.Tensor:
        """`run` with one iterator of `StepPlans`, asked for one per batch as the batches come."""
        self.fork_from_current()
        # The last TAIL_STEPS batches are submitted in the low-latency layouts: that needs a look-ahead of TAIL_STEPS
        # batches, not the whole list -- a lazily produced stream of (pinned or device) batches is consumed as it comes and
        # never held in full.
        from collections import deque
        parts, ahead = [], deque()

        def step(audio, p, tail):
            return self.submit(audio, tail=tail, mix=p.mix, reverb=p.reverb, speed=p.speed, **p.mask_keyword())[0]

        for a in audio_batches:
            ahead.append((a, next(plans)))
            if len(ahead) > TAIL_STEPS:
                parts.append(step(*ahead.popleft(), False))
        while ahead:
            parts.append(step(*ahead.popleft(), True))
        self.synchronize()
        if not parts:
            n_keys = len(self.feature_keys) if self.feature_keys is not None else 8
            return torch.empty((0, self.time_segments * n_keys * self.net.num_output_neurons), dtype=torch.float32,
                               device=self.device)
        if out is None:
            return torch.cat(parts)
        torch.cat(parts, out=out)
        return out


def _stages_and_plans(speed, reverb, corrupt, mask=None, n_clips: int | None = None):
    """``speed=``, ``reverb=``, ``corrupt=`` (each None or a ``(stage, plan)`` pair) and ``mask=`` of a listing function as ``(the
    speed=, reverb=, mixer= keywords of HotPath and AugmentChain, the listing's StepPlans)``, checked to cover ``n_clips``."""
    (sp, speeds), (rv, reverbs), (mixer, mixes) = ((None, None) if pair is None else pair for pair in (speed, reverb, corrupt))
    plans = StepPlans(speeds, reverbs, mixes, mask)
    if n_clips is not None:
        plans.check_covers(n_clips)
    return dict(speed=sp, reverb=rv, mixer=mixer), plans


def _pinned_float32(audio) -> torch.Tensor:
    """``audio`` as a contiguous float32 host tensor, in pinned memory where the runtime grants it."""
    host = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    with contextlib.suppress(RuntimeError):
        return host.pin_memory() if len(host) else host
    return host


def features_from_audio(audio: np.ndarray, fe, net, feature_keys, batch: int = 1024,
                        streams: int = DEFAULT_STREAMS, device_out: bool = False, time_segments: int = 1, corrupt=None,
                        reverb=None, speed=None, mask=None):
    """Host convenience for the drop-in scripts' in-memory path: (n, n_samples) float32 on the host ->
    (n, n_feat) float32 on the host (or, `device_out`, still on the GPU for a gather), batches of `batch` clips
    through the overlapped pipeline (pinned staging, uploads on the steps' streams).  n = 0 (an empty shard)
    gives an empty (0, n_feat) block.  `time_segments` = K > 1: K segment rows per clip side by side (`HotPath`), n_feat is
    K times as wide.  `speed` = ``(frontend.SpeedPerturber, frontend.SpeedPlan of the n clips)``, `reverb` =
    ``(frontend.Reverberator, frontend.ReverbPlan of the n clips)``, `corrupt` = ``(frontend.NoiseMixer, frontend.MixPlan of the
    n clips)``: every batch goes through these stages on the device, in this order (`augment.AugmentChain`; SPEC.md §1.12,
    §1.11, §1.10), with its slice of each plan, before its front end.  `mask` = a ``frontend.MaskPlan`` of the n clips: every
    batch's front end masks its slice of the plan inside the encoder (SPEC.md §1.13)."""
    stages, plans = _stages_and_plans(speed, reverb, corrupt, mask, len(audio))
    hp = HotPath(fe, net, feature_keys, streams=streams, time_segments=time_segments, **stages)
    pinned = _pinned_float32(audio)
    with torch.cuda.device(hp.device):
        starts = range(0, len(pinned), batch)
        feats = hp._run((pinned[lo:lo + batch] for lo in starts), (plans.part(lo, lo + batch) for lo in starts))
    return feats if device_out else feats.cpu().numpy()


FIT_ROW_BUFFERS = 4                  # row buffers a `fit_from_audio` run hands round between its steps and their pushes


def fit_from_audio(audio: np.ndarray, labels, fe, net, feature_keys, stats, batch: int = 1024,
                   streams: int = DEFAULT_STREAMS, corrupt=None, reverb=None, speed=None, mask=None) -> int:
    """`features_from_audio` with a sink: every step's rows go into ``stats`` (a `readout.RidgeStatistics` on the pipeline's
    device; SPEC.md §7) instead of being kept.  ``labels`` int32 (n): a clip whose label lies outside the statistics' classes
    is skipped by the push.  A step writes its rows into one of `FIT_ROW_BUFFERS` buffers (`HotPath.submit(out=...)`); the
    push runs on one stream of its own behind the step's event -- so the pushes are ordered among themselves --, and an
    event of the push releases the buffer to the step that takes it next.  No row outlives its push and the host waits for
    nothing per step (but for `HotPath`'s back-pressure); the call returns, after one synchronisation, the number of clips
    it has run.  The augmentation arguments are `features_from_audio`'s."""
    stages, plans = _stages_and_plans(speed, reverb, corrupt, mask, len(audio))
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if labels.shape != (len(audio),):
        raise ValueError(f"labels must hold one value per clip, got {labels.shape} for {len(audio)} clips")
    hp = HotPath(fe, net, feature_keys, streams=streams, **stages)
    if indexed_device(stats.device) != hp.device:
        raise ValueError(f"statistics on {stats.device}, pipeline on {hp.device}")
    n_keys = len(feature_keys) if feature_keys is not None else 8
    if n_keys * net.num_output_neurons != stats.D or n_keys != len(stats.feature_keys):
        raise ValueError(f"the statistics hold rows of {len(stats.feature_keys)} keys x {stats.n_out}, the pipeline gives "
                         f"{n_keys} keys x {net.num_output_neurons}")
    pinned = _pinned_float32(audio)
    starts = list(range(0, len(pinned), batch))
    with torch.cuda.device(hp.device):
        cur = torch.cuda.current_stream(hp.device)
        y = torch.from_numpy(labels).to(hp.device)
        rows = [torch.empty((batch, stats.D), dtype=torch.float32, device=hp.device)
                for _ in range(min(FIT_ROW_BUFFERS, len(starts)))]
        released = [None] * len(rows)
        pusher = torch.cuda.Stream(device=hp.device)
        pusher.wait_stream(cur)                  # the labels, the buffers and whatever filled `stats` before this call
        hp.fork_from_current()
        for s, lo in enumerate(starts):
            part, at = plans.part(lo, lo + batch), s % len(rows)
            n = min(batch, len(pinned) - lo)
            feats, st = hp.submit(pinned[lo:lo + n], out=rows[at][:n], after=released[at], tail=s >= len(starts) - TAIL_STEPS,
                                  mix=part.mix, reverb=part.reverb, speed=part.speed, **part.mask_keyword())
            if feats.data_ptr() != rows[at].data_ptr():
                raise RuntimeError("the step did not write its rows into the buffer it was given")
            done = torch.cuda.Event()
            done.record(st)
            pusher.wait_event(done)
            with torch.cuda.stream(pusher):
                stats.push(feats, y[lo:lo + n])
            released[at] = torch.cuda.Event()
            released[at].record(pusher)
        hp.synchronize()
        pusher.synchronize()
    return len(pinned)


def _audio_windows(audio, fe):
    """``audio`` (n, W * fe.n_samples) float32, tensor or NumPy (copied), checked: ``(audio tensor, n, W)``."""
    audio = as_float32(audio)
    ns = int(fe.n_samples)
    if audio.dim() != 2 or audio.shape[1] < ns or audio.shape[1] % ns:
        raise ValueError(f"audio must be (n, W * {ns}), got {tuple(audio.shape)}")
    return audio, int(audio.shape[0]), int(audio.shape[1]) // ns


def _encode_audio_windows(audio, n: int, W: int, fe, net):
    """The rasters (n, W, C, T) of ``_audio_windows``' audio: the front end runs on the n * W windows as independent clips.
    Called on ``net.device``."""
    x = audio.to(net.device).reshape(n * W, int(fe.n_samples))
    return fe.encode(x).reshape(n, W, fe.n_channels, -1)


def _recording_windows(recordings, fe, caller: str):
    """``recordings`` (1-D arrays or tensors of whole windows of fe.n_samples samples) as contiguous float32 arrays, and
    their window counts W_r (int64); ``caller`` is the public function's name, for the refusal of an empty list."""
    ns = int(fe.n_samples)
    arrays, windows = [], []
    for r, rec in enumerate(recordings):
        a = rec.detach().cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
        if a.ndim != 1 or a.shape[0] < ns or a.shape[0] % ns:
            raise ValueError(f"recording {r} must be a 1-D array of a whole number (at least 1) of windows of {ns} samples, "
                             f"got shape {tuple(a.shape)}")
        arrays.append(np.ascontiguousarray(a, dtype=np.float32))
        windows.append(a.shape[0] // ns)
    if not arrays:
        raise ValueError(f"{caller} needs at least one recording")
    return arrays, np.asarray(windows, dtype=np.int64)


def _scatter_recording_windows(arrays, windows, fe, net):
    """The rasters (n, W_max, C, T) of ``_recording_windows``' recordings: the front end runs once on all windows of all
    recordings as independent clips, window w of recording r lands at [r, w], and what lies past a recording's W_r windows
    is zeros.  Called on ``net.device``."""
    n, w_max = len(arrays), int(windows.max())
    x = torch.from_numpy(np.concatenate(arrays).reshape(-1, int(fe.n_samples))).to(net.device)
    enc = fe.encode(x)                                                  # (sum of W_r, C, T), recording-major
    rec_of = torch.from_numpy(np.repeat(np.arange(n), windows)).to(net.device)
    win_of = torch.from_numpy(np.concatenate([np.arange(w) for w in windows])).to(net.device)
    rasters = torch.zeros((n, w_max, fe.n_channels, int(enc.shape[2])), dtype=torch.uint8, device=net.device)
    rasters[rec_of, win_of] = enc
    return rasters


def _audio_window(x, w: int, fe):
    """Window w of every recording of the device audio (n, W * n_samples) as a contiguous (n, n_samples) batch."""
    ns = int(fe.n_samples)
    return x[:, w * ns:(w + 1) * ns].contiguous()


def features_from_long_audio(audio, fe, net, feature_keys, carry_state: bool = True, fused: bool = False):
    """A recording taken window by window: ``audio`` (n, W * fe.n_samples) float32 -> (n, W, n_feat) float32 device
    tensor.  The front end runs on the n * W windows as independent clips (its normalisation is per clip, as the
    reference's); the reservoir then takes window after window and, with ``carry_state``, keeps its membrane, refractory
    and spike state between them (``SNN.run_batch(state=...)``): row w holds the features of steps [0, (w + 1) * T) of
    the recording, what one run over the concatenated rasters gives.  ``carry_state=False``: every window from
    ``reset()``, W independent ``run_batch`` calls.  ``fused`` = True: where `step_fused_state_supported` serves the shape,
    window w is ONE launch over its audio (`step_fused_from`) with the state carried -- W launches, no raster tensor, the same
    rows; another shape takes the route above.  Off by default (profiles/step_fused_state.txt)."""
    audio, n, W = _audio_windows(audio, fe)
    with torch.cuda.device(net.device):
        if fused and step_fused_state_supported(fe, net, n):
            x = audio.to(net.device)
            state = net.new_state(n) if carry_state else None
            return torch.stack([step_fused_from(fe, net, _audio_window(x, w, fe), feature_keys, state=state)
                                for w in range(W)], dim=1)
        rasters = _encode_audio_windows(audio, n, W, fe, net)
        state = net.new_state(n) if carry_state else None
        rows = [net.run_batch(rasters[:, w].contiguous(), feature_keys, state=state)[0] for w in range(W)]
        return torch.stack(rows, dim=1)


def features_from_recordings(recordings, fe, net, feature_keys):
    """Recordings of different lengths in one batch: ``recordings``, a list of n 1-D float32 arrays of ``W_r *
    fe.n_samples`` samples each (W_r >= 1 whole windows), -> (n, n_feat) float32 device tensor.  Row r holds the features of
    recording r's one uncut run over its ``W_r * fe.n_steps`` steps, what ``features_from_long_audio`` gives for that
    recording alone in its last row.  The front end runs once on all windows of all recordings as independent clips (its
    normalisation is per window, as the reference's); the rasters are scattered into (n, W_max, C, T), and the reservoir
    takes W_max ragged launches with its state carried (``SNN.run_batch(lengths=...)``, SPEC.md §4c): in launch w a
    recording that still has a window runs its T steps, one that has ended rides along with 0 and keeps its row."""
    arrays, windows = _recording_windows(recordings, fe, "features_from_recordings")
    n = len(arrays)
    with torch.cuda.device(net.device):
        rasters = _scatter_recording_windows(arrays, windows, fe, net)
        T = int(rasters.shape[3])
        from .snn import _select_keys
        keys, _ = _select_keys(feature_keys)
        feats = torch.zeros((n, len(keys) * net.num_output_neurons), dtype=torch.float32, device=net.device)
        state = net.new_state(n)
        for w in range(rasters.shape[1]):
            net.run_batch(rasters[:, w].contiguous(), feature_keys, features_out=feats, state=state,
                          lengths=np.where(windows > w, T, 0))
        return feats


def _trimmed_listing(trim, audio, bins: np.ndarray, fe, device, batch: int, lengths=None):
    """A packed listing (`frontend.pack_utterances`) through ``trim`` in batches of ``batch`` rows: -> ``(the trimmed rows, a
    float32 (n, 160 * time_bins) DEVICE tensor, their bins as host int32)``.  Launches only, then one read-back of the bins.
    ``audio`` may be a device tensor (the perturbed listing) and ``lengths`` the int32 device tensor of its clips' samples;
    None: 160 * bins from the host."""
    n = len(bins)
    rows = torch.empty((n, RAGGED_HOP * fe.time_bins), dtype=torch.float32, device=device)
    kept = torch.empty((n,), dtype=torch.int32, device=device)
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        x = audio[lo:hi] if torch.is_tensor(audio) else torch.from_numpy(audio[lo:hi]).to(device)
        _, part, _ = trim.trim(x, bins[lo:hi].astype(np.int64) * RAGGED_HOP if lengths is None else lengths[lo:hi],
                               time_bins=fe.time_bins, out=rows[lo:hi])
        kept[lo:hi] = part
    return rows, kept.cpu().numpy()


def _perturbed_listing(chain, speeds, audio: np.ndarray, bins: np.ndarray, fe, device, batch: int):
    """A packed listing through the speed stage (`AugmentChain.speed_ragged`, SPEC.md §1.18) in batches of ``batch`` rows, every
    utterance at ``160 * bins`` samples: -> ``(the perturbed rows, a float32 (n, 160 * time_bins) DEVICE tensor, their samples
    as an int32 DEVICE tensor, their bins as host int32)``.  Launches only: the host bins come from the length formula
    (`frontend.speed_ragged_lengths`), which also refuses, before any launch, an utterance that a speed leaves under 3 bins."""
    from .frontend import RAGGED_MIN_BINS, speed_ragged_lengths
    n, n_out = len(bins), RAGGED_HOP * fe.time_bins
    lengths = bins.astype(np.int64) * RAGGED_HOP
    new_bins = -(-speed_ragged_lengths(lengths, speeds.choice, chain.speed, n_out) // RAGGED_HOP)
    short = np.nonzero(new_bins < RAGGED_MIN_BINS)[0]
    if len(short):
        r = int(short[0])
        raise ValueError(f"utterance {r} has {int(bins[r])} time bins and {int(new_bins[r])} at its speed "
                         f"(choice {int(speeds.choice[r])}): a clip needs {RAGGED_MIN_BINS}")
    rows = torch.empty((n, n_out), dtype=torch.float32, device=device)
    samples = torch.empty((n,), dtype=torch.int32, device=device)
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        _, part, _ = chain.speed_ragged(torch.from_numpy(audio[lo:hi]).to(device), lengths[lo:hi],
                                        StepPlans(speed=speeds.part(lo, hi)), time_bins=fe.time_bins, out=rows[lo:hi])
        samples[lo:hi] = part
    return rows, samples, new_bins.astype(np.int32)


def features_from_utterances(utterances, fe, net, feature_keys, batch: int = 1024, fused: bool = False, trim=None,
                             corrupt=None, reverb=None, mask=None, speed=None):
    """Utterances of different lengths, each one clip: ``utterances``, a list of n 1-D float32 arrays of 321 to
    ``fe.n_samples`` samples, -> (n, n_feat) float32 device tensor in the input order.  Row r holds the features of utterance
    r taken alone: its own ``ceil(len / 160)`` time bins through the front end of that length (its normalisation range is the
    utterance's, SPEC.md §1.14) and its own ``bins * n_thr`` reservoir steps (§4c) -- no padding takes part in either.
    Batches of ``batch`` utterances, longest first (the waves of a launch finish with their clips, so clips of like length
    share a launch); within a batch the ragged front end (`SpikeFrontEnd.encode_ragged`) hands its raster and its device step
    counts to the ragged reservoir launch on the same stream, with no host synchronisation between them.  Where
    ``fe.n_steps`` exceeds the longest launch the reservoir's plan accepts, the reservoir runs in chunks
    (``SNN.run_chunked(lengths=...)``, host lengths).  ``fused`` = True: a batch whose shape the ragged one-launch step
    serves (`step_fused_supported(..., form="ragged")`) is that one launch (`step_fused_ragged`) -- no raster, no step counts
    in memory, the same rows; every other batch takes the two launches.  Off by default (profiles/step_fused_forms.txt).
    ``trim`` (a `frontend.SilenceTrimmer`): every utterance is first cut to its speech on the device (SPEC.md §1.15) and row r
    holds the features of that slice taken alone.  The packed listing is uploaded and trimmed in batches of ``batch``,
    launches only; the trimmed bin counts are then read back ONCE, for the longest-first order and the host lengths the
    batches take, and the batches run as above on the trimmed rows, gathered on the device.  None: nothing changes.
    ``reverb`` = ``(frontend.Reverberator, frontend.ReverbPlan of the n utterances)``, ``corrupt`` = ``(frontend.NoiseMixer,
    frontend.MixPlan of the n utterances)``, as `features_from_audio` takes them, and ``mask`` = a `frontend.MaskPlan` of the n
    utterances (`frontend.mask_plan_ragged`) or a callable ``bins -> MaskPlan``, called once with the (trimmed) host bins: the
    plans are in listing order and every batch takes its longest-first slice of each.  Per batch, on the one stream
    (SPEC.md §1.16): the trim above, reverberation at the row stride (causal: a clip's own samples are the clip-alone
    ones, its tail is ignored), the ragged mixer at the clip's (trimmed) length -- the SNR is taken against the speech, and
    the noise does not decide the trim -- then the ragged front end with the mask.  Row r is the row of that chain on
    utterance r alone.  With ``fused`` a masked batch takes `step_fused_ragged(mask=...)` where
    `step_fused_supported(..., form="ragged-masked")` says so.  All three None: nothing changes.
    ``speed`` = ``(frontend.SpeedPerturber, frontend.SpeedPlan of the n utterances)``: every utterance is first played at its
    speed, as the clip alone (SPEC.md §1.18) -- the recipe's first stage, because everything behind it sees the recording as
    played: speed, trim, reverberation, ragged mixer, ragged front end with the mask.  The packed listing is perturbed in
    batches of ``batch`` at ``160 * bins`` samples per utterance, launches only; an utterance's new bins,
    ``ceil(min(ceil(160 * bins * up / down), fe.n_samples) / 160)`` -- a slowed utterance is cut at the row -- are known on the
    host from the formula (`frontend.speed_ragged_lengths`), so the longest-first order costs no read-back, and an utterance
    that its speed leaves under 3 bins is refused with its index before anything is launched.  With ``trim`` the trimmer takes
    the device lengths the speed launch wrote, and the one read-back of the trimmed bins stays the only one.  ``mask`` as a
    callable is called with the final bins; a ready `MaskPlan` drawn for the bins before the speed stage has its time bands
    placed against those old lengths (bits at or behind a clip's new end are ignored, §1.16).  Row r is the row of the whole
    chain on utterance r alone.  None: not one launch changes."""
    from .frontend import pack_utterances
    from .snn import _select_keys
    stages, plans = _stages_and_plans(speed, reverb, corrupt)
    audio, bins = pack_utterances(utterances, fe.time_bins)
    n = len(bins)
    keys, _ = _select_keys(feature_keys)
    batch = max(1, int(batch))
    chain = AugmentChain(**stages)
    with torch.cuda.device(net.device):
        samples = None
        if plans.speed is not None:
            chain.refuse(StepPlans(speed=plans.speed))
            StepPlans(speed=plans.speed).check_covers(n)
            audio, samples, bins = _perturbed_listing(chain, plans.speed, audio, bins, fe, net.device, batch)
        if trim is not None:
            audio, bins = _trimmed_listing(trim, audio, bins, fe, net.device, batch, samples)
        plans = plans._replace(speed=None, mask=mask(bins) if callable(mask) else mask)        # what is left, at the final bins
        plans.check_covers(n)
        feats = torch.zeros((n, len(keys) * net.num_output_neurons), dtype=torch.float32, device=net.device)
        order = np.argsort(-bins.astype(np.int64), kind="stable")
        n_thr = len(fe.thresholds)
        for lo in range(0, n, batch):
            idx = order[lo:lo + batch]
            x = audio[torch.from_numpy(idx).to(net.device)] if torch.is_tensor(audio) else torch.from_numpy(audio[idx]).to(net.device)
            p = plans.take(idx)
            x = chain.apply_ragged(x, bins[idx].astype(np.int64) * RAGGED_HOP, p)
            if fused and step_fused_supported(fe, net, len(idx), "ragged" if p.mask is None else "ragged-masked"):
                rows = torch.zeros((len(idx), feats.shape[1]), dtype=torch.float32, device=net.device)
                step_fused_ragged(fe, net, x, bins[idx], feature_keys, features_out=rows, **p.mask_keyword())
                feats[torch.from_numpy(idx).to(net.device)] = rows
                continue
            raster, steps = fe.encode_ragged(x, bins[idx], **p.mask_keyword())
            if fe.n_steps > net.max_steps(len(idx)):
                rows = net.run_chunked(raster, feature_keys, lengths=bins[idx].astype(np.int64) * n_thr)[0]
            else:
                rows = net.run_batch(raster, feature_keys, lengths=steps)[0]
            feats[torch.from_numpy(idx).to(net.device)] = rows
        return feats


def sliding_features_from_long_audio(audio, fe, net, feature_keys, segment_steps: int, window_segments: int,
                                     hop_segments: int = 1, fused: bool = False):
    """Features of sliding windows over a recording: ``audio`` (n, W * fe.n_samples) float32 -> (n, Wn, n_feat) float32
    device tensor.  The front end runs on the n * W audio windows as independent clips, as in
    ``features_from_long_audio``; the reservoir takes them one after the other with its state carried, one segmented
    launch per audio window (``segment_steps`` divides ``fe.n_steps``), and the records of all launches, concatenated, go
    through one ``lsm_segment_features`` call: row w is the feature row of steps
    ``[w * hop_segments * segment_steps, (w * hop_segments + window_segments) * segment_steps)`` of the recording's one
    uncut run -- windows may straddle the audio windows.  ``fused`` = True: where `step_fused_state_supported` serves the
    shape, audio window w is ONE launch (`step_fused_segments`) with the state carried and no raster tensor; the records are
    concatenated and folded once, as above.  Off by default (profiles/step_fused_state.txt)."""
    audio, n, W = _audio_windows(audio, fe)
    S = int(segment_steps)
    if S < 1 or fe.n_steps % S:
        raise ValueError(f"segment_steps = {segment_steps} must be >= 1 and divide the front end's {fe.n_steps} steps")
    net.segment_windows(W * (fe.n_steps // S), window_segments, hop_segments)     # refuse before anything is launched
    with torch.cuda.device(net.device):
        if fused and step_fused_state_supported(fe, net, n):
            x = audio.to(net.device)
            state = net.new_state(n)
            records = torch.cat([step_fused_segments(fe, net, _audio_window(x, w, fe), S, (), state=state, want_records=True)[1]
                                 for w in range(W)], dim=1)
            return net.segment_features(records, S, feature_keys, window_segments, hop_segments)
        rasters = _encode_audio_windows(audio, n, W, fe, net)
        state = net.new_state(n)
        records = torch.cat([net.run_segment_records(rasters[:, w].contiguous(), S, state=state)[0] for w in range(W)],
                            dim=1)
        return net.segment_features(records, S, feature_keys, window_segments, hop_segments)


# ---- open-ended streams (SPEC.md §4d) -------------------------------------------------------------------------------------
def completed_windows(n_segments, window_segments: int, hop_segments: int):
    """How many windows ``[w * H, w * H + K)`` lie wholly inside the first ``n_segments`` segments (an int or an array of
    them): none below K, then one more every H segments."""
    K, H = int(window_segments), int(hop_segments)
    return np.where(n_segments >= K, (n_segments - K) // H + 1, 0)


def stream_window_plan(seen, new, window_segments: int, hop_segments: int = 1):
    """The bookkeeping of one push into a stream, host integers only.  Window w of a stream covers its segments
    ``[w * H, w * H + K)`` counted from the stream's start, and is complete once the stream has seen ``w * H + K`` segments.
    A stream that had seen ``seen`` segments and receives ``new`` more completes ``n_windows`` windows and must keep its last
    ``keep`` records for the windows still open: those from the start of the next window on, at most ``K - 1`` of them
    (``H <= K`` is required: with a larger hop whole segments would be skipped, not kept).  Scalars or arrays of equal
    shape; returns ``(n_windows, keep)`` as ints or int64 arrays."""
    K, H = int(window_segments), int(hop_segments)
    if K < 1 or H < 1 or H > K:
        raise ValueError(f"window_segments = {K} must be >= 1 and hop_segments = {H} in [1, {K}]")
    seen_a, new_a = np.asarray(seen, dtype=np.int64), np.asarray(new, dtype=np.int64)
    if (seen_a < 0).any() or (new_a < 0).any():
        raise ValueError("stream_window_plan: seen and new must be >= 0")
    total = seen_a + new_a
    n_windows = completed_windows(total, K, H) - completed_windows(seen_a, K, H)
    keep = total - completed_windows(total, K, H) * H              # 0 <= keep <= K - 1 for H <= K
    if np.ndim(seen) == 0 and np.ndim(new) == 0:
        return int(n_windows), int(keep)
    return n_windows, keep


def model_params(fe, sim_params, **more) -> dict:
    """Every parameter the front end ``fe`` (``frontend.SpikeFrontEnd``) and a reservoir of ``sim_params``
    (``reservoir.SimulationParams``, with the weight actually used in ``mean_weight``) were built from, as the plain dict a
    ``readout.LinearModel`` carries in its file; ``more``: what the caller adds (feature_set, multiplier, time_segments)."""
    p = dict(filterbank=fe.filterbank, n_filters=fe.n_filters, redundancy=fe.redundancy,
             thresholds=[float(t) for t in fe.thresholds], gap=fe.gap, time_bins=fe.time_bins, n_samples=fe.n_samples,
             n_channels=fe.n_channels)
    for name in ("num_neurons", "num_output_neurons", "mean_weight", "weight_variance", "membrane_threshold",
                 "leak_coefficient", "refractory_period", "small_world_graph_p", "small_world_graph_k", "seed"):
        p[name] = getattr(sim_params, name)
    lvd = sim_params.leak_variance_divisor
    p["leak_variance_divisor"] = None if lvd is None else float(lvd)
    p.update(more)
    return p


def pipeline_from_params(params: dict, device=None):
    """``(fe, net)`` rebuilt from ``model_params``' dict: the same front end and, the wiring being a function of the
    parameters and the seed alone (SPEC.md §2), the same reservoir -- their feature rows equal the training run's byte for
    byte."""
    from . import frontend
    from .snn import SNN, SimulationParams
    fe = frontend.SpikeFrontEnd(params["n_filters"], params["filterbank"], device=device, redundancy=params["redundancy"],
                                thresholds=params["thresholds"], gap=params["gap"], time_bins=params["time_bins"],
                                n_samples=params["n_samples"])
    sim = SimulationParams(**{name: params[name] for name in (
        "num_neurons", "mean_weight", "num_output_neurons", "membrane_threshold", "leak_coefficient", "refractory_period",
        "small_world_graph_p", "small_world_graph_k", "leak_variance_divisor", "weight_variance", "seed")})
    return fe, SNN(sim, n_channels=params["n_channels"], device=fe.device)


def _checked_readout(readout, net, feature_keys):
    """A bank's ``readout`` (``readout.DeviceReadout`` or None) scores the rows the bank would return: same keys, same
    output neurons, same device."""
    if readout is None:
        return None
    from .snn import _select_keys
    m = readout.model
    if (list(m.feature_keys) != list(_select_keys(feature_keys)[0]) or m.n_out != net.num_output_neurons
            or readout.device != net.device):
        raise ValueError(f"the readout was fitted on {m.feature_keys} x {m.n_out} output neurons on {readout.device}; the bank "
                         f"returns {_select_keys(feature_keys)[0]} x {net.num_output_neurons} on {net.device}")
    return readout


def debounce(labels, counts, state, hold: int, background: int):
    """Events from the labels of consecutive pushes, host integers only.  ``labels`` (n_streams, W) and ``counts``
    (n_streams) as ``push_scores`` returns them (arrays on the host); ``state``: the dict a previous call returned, or None
    at the streams' start.  Stream b emits ``(b, window index, label)`` at the window in which the same label -- neither
    ``background`` nor -1 -- has won ``hold`` consecutive windows, counted across pushes, and nothing more until its label
    changes.  Window indices count from the stream's start.  Returns ``(events, state)``."""
    labels, counts = np.asarray(labels), np.asarray(counts)
    n = int(counts.shape[0])
    hold = int(hold)
    if hold < 1:
        raise ValueError(f"hold = {hold} must be >= 1")
    if state is None:
        state = dict(last=np.zeros(n, dtype=np.int64), run=np.zeros(n, dtype=np.int64), seen=np.zeros(n, dtype=np.int64))
    last, run, seen = state["last"].copy(), state["run"].copy(), state["seen"].copy()
    events = []
    for b in range(n):
        for j in range(int(counts[b])):
            lab = int(labels[b, j])
            run[b] = run[b] + 1 if (run[b] > 0 and lab == last[b]) else 1
            last[b] = lab
            if run[b] == hold and lab != background and lab != -1:
                events.append((b, int(seen[b]), lab))
            seen[b] += 1
    return events, dict(last=last, run=run, seen=seen)


class CarryBuffer:
    """What ``n_streams`` streams carry from one push to the next: per stream up to ``cap`` trailing items (records, raster
    steps -- tensors of shape ``item``) in ``kept`` (n_streams, cap, *item), left-aligned and zero-padded, and how many of
    them, in the host array ``count``.  A push first joins the kept items with the new ones into one run per stream, then
    keeps the tail of that run.  Lives on ``device``, CPU included; ``cap`` may be 0."""

    def __init__(self, n_streams: int, cap: int, item, dtype, device):
        self.kept = torch.zeros((n_streams, cap, *item), dtype=dtype, device=device)
        self.count = np.zeros(n_streams, dtype=np.int64)

    def _gather(self, run, src):
        """``run[b, src[b, j]]`` with the indices clipped to the run's width: (n_streams, src.shape[1], *item)."""
        src = torch.from_numpy(np.clip(src, 0, max(run.shape[1] - 1, 0))).to(run.device)
        return run[torch.arange(run.shape[0], device=run.device)[:, None], src]

    def reset(self, slots) -> None:
        """The streams in ``slots`` (an int64 array) carry nothing any more."""
        self.kept[torch.from_numpy(slots).to(self.kept.device)] = 0
        self.count[slots] = 0

    def join(self, new, counts):
        """``new`` (n_streams, G, *item): stream b delivers its first ``counts[b]`` items.  Returns ``(run, have)``: ``run``
        (n_streams, cap + G, *item) holds per stream its kept items, then the new ones, contiguous from position 0;
        ``have = count + counts`` of them are valid, what lies behind is never to be read."""
        cap = self.kept.shape[1]
        j = np.arange(cap + new.shape[1], dtype=np.int64)[None, :]
        src = np.where(j < self.count[:, None], j, cap + j - self.count[:, None])
        return self._gather(torch.cat([self.kept, new], dim=1), src).contiguous(), self.count + counts

    def keep(self, run, have, keep) -> None:
        """The last ``keep[b] <= cap`` of the ``have[b]`` items of ``join``'s ``run`` are what stream b carries on."""
        j = np.arange(self.kept.shape[1], dtype=np.int64)[None, :]
        kept = self._gather(run, (have - keep)[:, None] + j)
        live = torch.from_numpy(j < keep[:, None]).to(run.device).reshape(kept.shape[:2] + (1,) * (kept.dim() - 2))
        self.kept = torch.where(live, kept, torch.zeros_like(kept)).contiguous()
        self.count = np.array(keep, dtype=np.int64)


class StreamBank:
    """``n_streams`` open-ended streams served by one reservoir: every ``push`` takes whatever whole segments each stream
    has delivered since the last one -- any number, 0 included, the streams anywhere on their own timelines -- through one
    ragged stream launch (``SNN.run_stream_records``) and returns the sliding-window feature rows the push completed.
    Window w of a stream covers its segments ``[w * hop_segments, w * hop_segments + window_segments)``, counted from the
    stream's start or last ``reset``; its row is the feature row of that slice of the stream's one uncut run.  The bank holds
    the reservoir state, per stream the trailing records still needed (at most ``window_segments - 1``) and a host count of
    the segments seen; a stream has no length limit."""

    def __init__(self, net, n_streams: int, segment_steps: int, window_segments: int, hop_segments: int = 1,
                 feature_keys=None, readout=None):
        self.net = net
        self.readout = _checked_readout(readout, net, feature_keys)      # readout.DeviceReadout or None: push_scores
        self.n_streams = int(n_streams)
        self.S, self.K, self.H = int(segment_steps), int(window_segments), int(hop_segments)
        if self.n_streams < 1 or self.S < 1:
            raise ValueError(f"StreamBank needs n_streams >= 1 and segment_steps >= 1, got {n_streams}, {segment_steps}")
        stream_window_plan(0, 0, self.K, self.H)                         # H <= K
        if self.K * self.S > 65535:
            raise ValueError(f"a window of {self.K} segments of {self.S} steps exceeds 65535 steps")
        self.feature_keys = feature_keys
        self.state = net.new_state(self.n_streams)
        self.seen = np.zeros(self.n_streams, dtype=np.int64)             # segments since the stream's start
        self.tail = CarryBuffer(self.n_streams, self.K - 1, (net.num_output_neurons, 4), torch.int32, net.device)

    @property
    def tail_count(self) -> np.ndarray:
        """Records kept per stream for the windows still open."""
        return self.tail.count

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: state block, tail and count back to zero."""
        slots = checked_slots(slots, self.n_streams)
        self.state.data[torch.from_numpy(slots).to(self.net.device)] = 0
        self.tail.reset(slots)
        self.seen[slots] = 0

    def push(self, rasters, segments):
        """``rasters`` (n_streams, C, G * S) uint8: stream b's new steps are the first ``segments[b] * S`` columns of its
        row; ``segments``: n_streams host integers in [0, G].  Returns ``(rows, counts)``: ``rows`` float32
        (n_streams, W, n_feat) on the device and ``counts`` (int64, host) -- ``rows[b, j]`` for ``j < counts[b]`` are the
        windows of stream b this push completed, in order; rows past a count are zeros.  A push longer than the longest
        launch the plan accepts is cut at segment boundaries."""
        from .snn import _select_keys
        n_feat = len(_select_keys(self.feature_keys)[0]) * self.net.num_output_neurons
        return self._push(rasters, segments,
                          lambda joined, have: self.net.segment_features(joined, self.S, self.feature_keys, self.K, self.H,
                                                                         segments=have),
                          lambda: torch.zeros((self.n_streams, 0, n_feat), dtype=torch.float32, device=self.net.device))

    def push_scores(self, rasters, segments):
        """``push`` that scores the windows it completes instead of returning their rows (SPEC.md §6): returns
        ``(logits, labels, counts)`` -- float64 (n_streams, W, n_classes), int32 (n_streams, W) and ``push``'s ``counts``;
        ``logits[b, j]``, ``labels[b, j]`` for ``j < counts[b]`` are what ``readout.score_rows`` gives on ``push``'s
        ``rows[b, j]``, byte for byte, from one launch that writes no feature row; past a count, zeros and -1."""
        if self.readout is None:
            raise ValueError("push_scores needs a readout: StreamBank(..., readout=readout.DeviceReadout(model, device))")
        ro = self.readout
        out = self._push(rasters, segments,
                         lambda joined, have: ro.score_windows(self.net, joined, self.S, self.K, self.H, segments=have),
                         lambda: (torch.zeros((self.n_streams, 0, ro.model.n_classes), dtype=torch.float64,
                                              device=self.net.device),
                                  torch.zeros((self.n_streams, 0), dtype=torch.int32, device=self.net.device)))
        (logits, labels), counts = out
        return logits, labels, counts

    def _push(self, rasters, segments, windows_of, nothing):
        """One push: ``windows_of(joined, have)`` is what the caller wants of every stream's joined records (feature rows,
        scores), ``nothing()`` the same for a push that delivers no segment.  Returns ``(that, counts)``."""
        net, S, K, H = self.net, self.S, self.K, self.H
        if isinstance(rasters, np.ndarray):
            rasters = torch.from_numpy(np.ascontiguousarray(rasters, dtype=np.uint8))
        if rasters.dim() != 3 or rasters.shape[0] != self.n_streams or rasters.shape[2] % S:
            raise ValueError(f"rasters must be ({self.n_streams}, C, G * {S}), got {tuple(rasters.shape)}")
        Gp = int(rasters.shape[2]) // S
        new = net._host_segments(np.asarray(segments), self.n_streams, Gp)
        counts, keep = stream_window_plan(self.seen, new, K, H)
        from .snn import ragged_chunks
        if Gp == 0 or int(new.max()) == 0:
            return nothing(), counts
        chunk = net._max_steps_cached(self.n_streams) // S * S
        if chunk < 1:
            raise ValueError(f"segment_steps = {S} exceeds the longest launch the plan accepts for {self.n_streams} streams")
        with torch.cuda.device(net.device):
            rasters = rasters.to(net.device, dtype=torch.uint8)
            fresh = torch.zeros((self.n_streams, Gp, net.num_output_neurons, 4), dtype=torch.int32, device=net.device)
            for t0, n, steps in ragged_chunks(new * S, chunk):
                rec, _, _ = net.run_stream_records(rasters[:, :, t0:t0 + n], S, segments=steps // S, state=self.state)
                fresh[:, t0 // S:(t0 + n) // S] = rec
            # per stream: its kept records, then the new ones, contiguous from column 0 (the start of its next window)
            joined, have = self.tail.join(fresh, new)
            rows = windows_of(joined, have)
            self.tail.keep(joined, have, keep)
        self.seen += new
        return rows, counts


class AudioStreamBank:
    """``StreamBank`` fed with audio: ``gt_stream`` (``frontend.GammatoneStream`` or ``frontend.MelStream``) turns every push of whole hops into the
    raster columns it completed, the bank keeps each stream's columns that do not yet fill a segment (fewer than
    ``segment_steps / n_thr`` of them) and forwards whole segments to an inner ``StreamBank`` over ``net``.  Both halves
    continue from saved state, so the rows are those of each stream's one uncut run, audio to features.  With a ``resampler``
    (``frontend.ResampleStream``) in front, the streams arrive as PCM at its input rate, in whole units (SPEC.md §1.8).  With a
    ``mixer`` (``frontend.MixStream``), every stream's new samples are corrupted on the device (SPEC.md §1.10) behind the
    resampler and in front of the front end.  With a ``reverb`` (``frontend.ReverbStream``), they are convolved with the
    stream's room first (SPEC.md §1.11): behind the resampler, in front of the mixer."""

    def __init__(self, gt_stream, net, segment_steps: int, window_segments: int, hop_segments: int = 1, feature_keys=None,
                 resampler=None, mixer=None, reverb=None, readout=None):
        # the refusals come before anything touches a device
        streamed = getattr(gt_stream, "filterbank", None) == "gammatone" or getattr(gt_stream, "streamed", None) is True
        if not streamed or not hasattr(gt_stream, "push"):
            raise ValueError("AudioStreamBank needs a streamed front end, frontend.GammatoneStream or frontend.MelStream: the "
                             "batch mel front end (SpikeFrontEnd) normalises every window by its own maximum and keeps no "
                             "state between launches, so it cannot be streamed; frontend.MelStream is the streamed one")
        S, n_thr = int(segment_steps), int(gt_stream.n_thr)
        if S < 1 or S % n_thr:
            raise ValueError(f"segment_steps = {segment_steps} must be a positive multiple of the front end's {n_thr} "
                             f"thresholds: a column is {n_thr} steps and is never split over two segments")
        stream_window_plan(0, 0, int(window_segments), int(hop_segments))        # hop_segments <= window_segments
        if resampler is not None:
            if int(resampler.n_streams) != int(gt_stream.n_streams):
                raise ValueError(f"the resampler serves {resampler.n_streams} streams, the front end {gt_stream.n_streams}")
            if resampler.unit_blocks * resampler.up != resampler.unit_hops * int(gt_stream.hop):
                raise ValueError(f"a unit of the resampler is {resampler.unit_blocks * resampler.up} samples, not "
                                 f"{resampler.unit_hops} hops of the front end's {gt_stream.hop}")
        for name, stage in (("mixer", mixer), ("reverberator", reverb)):
            if stage is not None and int(stage.n_streams) != int(gt_stream.n_streams):
                raise ValueError(f"the {name} serves {stage.n_streams} streams, the front end {gt_stream.n_streams}")
        if net.n_channels != gt_stream.n_channels:
            raise ValueError(f"the front end has {gt_stream.n_channels} channels, the reservoir {net.n_channels}")
        self.gt, self.net, self.S, self.n_thr, self.resampler = gt_stream, net, S, n_thr, resampler
        # behind the resampler, in front of the front end, in this order: frontend.ReverbStream, frontend.MixStream
        self.stages = [stage for stage in (reverb, mixer) if stage is not None]
        self.n_streams = int(gt_stream.n_streams)
        self.bank = StreamBank(net, self.n_streams, S, window_segments, hop_segments, feature_keys)
        if readout is not None:
            self.bank.readout = _checked_readout(readout, net, feature_keys)
        # time-major: an item is one raster step, (C,)
        self.pending = CarryBuffer(self.n_streams, S - n_thr, (gt_stream.n_channels,), torch.uint8, net.device)

    @property
    def pending_steps(self) -> np.ndarray:
        """Raster steps kept per stream that do not yet fill a segment (fewer than ``segment_steps``)."""
        return self.pending.count

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: both halves and the pending columns."""
        if self.resampler is not None:
            self.resampler.reset(slots)
        for stage in (*self.stages, self.gt, self.bank):
            stage.reset(slots)
        self.pending.reset(checked_slots(slots, self.n_streams))

    def push(self, audio, hops=None):
        """``audio`` (n_streams, H * hop) float32 and ``hops`` as ``GammatoneStream.push`` takes them.  Returns
        ``(rows, counts)`` with ``StreamBank.push``'s meaning: the sliding-window rows this push completed.
        With a ``resampler`` (``frontend.ResampleStream``): ``audio`` (n_streams, U * unit_in) float32 or int16 at the
        resampler's input rate and ``hops`` per-stream UNIT counts in [0, U] (None: U everywhere); stream b's first
        ``hops[b] * unit_in`` samples are resampled and reach the front end as ``hops[b] * unit_hops`` hops."""
        return self.bank.push(*self._whole_segments(audio, hops))

    def push_scores(self, audio, hops=None):
        """``push`` with ``StreamBank.push_scores`` behind the front end: ``(logits, labels, counts)`` of the windows this
        push completed."""
        if getattr(self.bank, "readout", None) is None:
            raise ValueError("push_scores needs a readout: AudioStreamBank(..., readout=readout.DeviceReadout(model, device))")
        return self.bank.push_scores(*self._whole_segments(audio, hops))

    def _whole_segments(self, audio, hops):
        """A push through the front end: ``(rasters, segments)`` as ``StreamBank.push`` takes them."""
        S = self.S
        if self.resampler is not None:
            audio, hops = self._resampled(audio, hops)
        for stage in self.stages:
            audio = self._through(stage, audio, hops)
        raster, cols = self.gt.push(audio, hops)
        dev = self.net.device
        with torch.cuda.device(dev):
            # per stream its pending steps, then the new ones, contiguous from step 0; whole segments go on
            run, total = self.pending.join(raster.to(dev).transpose(1, 2), cols * self.n_thr)
            segs = total // S
            self.pending.keep(run, total, total - segs * S)
            joined = run[:, :int(segs.max()) * S].transpose(1, 2).contiguous()
        return joined, segs

    def _through(self, stage, audio, hops):
        """The first ``hops[b]`` hops of every row through ``stage`` (the reverberator, the mixer); the rows keep their length."""
        return _stage_through(stage, audio, hops, self.n_streams, int(self.gt.hop))

    def _resampled(self, audio, units):
        """A push at the resampler's input rate -> ``(samples, hops)`` as the front end takes them."""
        return _stream_resampled(self.resampler, audio, units, self.n_streams)


def _stage_through(stage, audio, hops, n_streams: int, hop: int):
    """The first ``hops[b]`` hops of every row of a bank's push through ``stage`` (``frontend.ReverbStream``,
    ``frontend.MixStream``); the rows keep their length.  One copy for `AudioStreamBank` and `UtteranceBank`."""
    audio = as_float32(audio)
    if audio.dim() != 2 or audio.shape[0] != n_streams or audio.shape[1] % hop or audio.shape[1] < hop:
        raise ValueError(f"audio must be ({n_streams}, H * {hop}) with H >= 1, got {tuple(audio.shape)}")
    new = checked_counts(hops, n_streams, int(audio.shape[1]) // hop, "hops")
    return stage.push(audio, None if hops is None else new * hop)[0]


def _stream_resampled(rs, audio, units, n_streams: int):
    """A bank's push at the input rate of its ``frontend.ResampleStream`` -> ``(samples, hops)`` as the stages behind it take
    them.  One copy for `AudioStreamBank` and `UtteranceBank`."""
    audio, _ = checked_pcm(audio, n_streams, rs.unit_in)
    units = checked_counts(units, n_streams, int(audio.shape[1]) // rs.unit_in, "units")
    samples, _ = rs.push(audio, units * rs.unit_blocks)
    return samples, units * rs.unit_hops


class UtteranceBank:
    """Audio streams in, utterance feature rows (or labels) out, with no host round trip in between (SPEC.md §1.17):
    ``endpoint`` (``frontend.EndpointStream``) cuts every push into utterances, whose slots -- a ragged batch of
    ``n_streams * max_utts`` clips, most of them empty -- go through the ragged route unread: the one-launch step
    (`step_fused_ragged`) where `step_fused_supported(..., form="ragged")` holds, else `SpikeFrontEnd.encode_ragged` and
    ``SNN.run_batch(lengths=...)``.  An utterance's row is, bit for bit, that of `features_from_utterances` on its samples taken
    alone.  ``fe``: a `SpikeFrontEnd` whose rows are the endpoint's slots (``n_samples == 160 * max_bins``, ``time_bins ==
    max_bins``).  ``fused``: None takes the one-launch step where it is served, False never, True refuses a shape it does not
    serve.  ``resampler``, ``reverb`` and ``mixer`` are `AudioStreamBank`'s optional stages, in its order, in front of the
    endpoint detector; with any of them ``hops`` are host integers."""

    def __init__(self, endpoint, fe, net, feature_keys=None, readout=None, resampler=None, reverb=None, mixer=None, fused=None):
        from .frontend import ragged_refusal
        if not hasattr(endpoint, "max_utterances") or not hasattr(endpoint, "push"):
            raise ValueError("UtteranceBank needs a frontend.EndpointStream")
        M = int(endpoint.max_bins)
        why = ragged_refusal(fe.n_samples, fe.time_bins)
        if why is None and int(fe.time_bins) != M:
            why = (f"the endpoint detector emits rows of max_bins = {M} bins: the front end needs n_samples = {RAGGED_HOP * M} "
                   f"and time_bins = {M}, this one has {fe.n_samples} and {fe.time_bins}")
        if why:
            raise ValueError(why)
        n = int(endpoint.n_streams)
        if resampler is not None:
            if int(resampler.n_streams) != n:
                raise ValueError(f"the resampler serves {resampler.n_streams} streams, the endpoint detector {n}")
            if resampler.unit_blocks * resampler.up != resampler.unit_hops * RAGGED_HOP:
                raise ValueError(f"a unit of the resampler is {resampler.unit_blocks * resampler.up} samples, not "
                                 f"{resampler.unit_hops} hops of {RAGGED_HOP}")
        for name, stage in (("mixer", mixer), ("reverberator", reverb)):
            if stage is not None and int(stage.n_streams) != n:
                raise ValueError(f"the {name} serves {stage.n_streams} streams, the endpoint detector {n}")
        if net.n_channels != fe.n_channels:
            raise ValueError(f"the front end has {fe.n_channels} channels, the reservoir {net.n_channels}")
        if indexed_device(endpoint.device) != indexed_device(net.device) or indexed_device(fe.device) != indexed_device(net.device):
            raise ValueError(f"endpoint detector on {endpoint.device}, front end on {fe.device}, reservoir on {net.device}")
        self.endpoint, self.fe, self.net, self.feature_keys, self.fused = endpoint, fe, net, feature_keys, fused
        self.readout = _checked_readout(readout, net, feature_keys)
        self.resampler = resampler
        self.stages = [stage for stage in (reverb, mixer) if stage is not None]
        self.n_streams = n

    def reset(self, slots) -> None:
        """The streams in ``slots`` have ended and new ones take their places: every stage's state back to zero."""
        if self.resampler is not None:
            self.resampler.reset(slots)
        for stage in (*self.stages, self.endpoint):
            stage.reset(slots)

    def cut(self, audio, hops=None, finish=None):
        """A push through the optional stages and the endpoint detector: ``frontend.Utterances``."""
        if self.resampler is not None:
            audio, hops = _stream_resampled(self.resampler, audio, hops, self.n_streams)
        for stage in self.stages:
            audio = _stage_through(stage, audio, hops, self.n_streams, 160)
        return self.endpoint.push(audio, hops, finish)

    def _takes_fused(self, n_clips: int) -> bool:
        if self.fused is False:
            return False
        served = step_fused_supported(self.fe, self.net, n_clips, "ragged")
        if self.fused and not served:
            raise ValueError(f"fused=True: the one-launch ragged step does not serve {n_clips} clips of this front end and reservoir")
        return served

    def _run(self, audio, bins):
        """A ragged batch through the route the bank takes: float32 (n, n_feat)."""
        from .snn import _select_keys
        fe, net = self.fe, self.net
        n = int(audio.shape[0])
        if self._takes_fused(n):
            rows = torch.zeros((n, len(_select_keys(self.feature_keys)[0]) * net.num_output_neurons), dtype=torch.float32,
                               device=net.device)
            step_fused_ragged(fe, net, audio, bins, self.feature_keys, features_out=rows)
            return rows
        if fe.n_steps > net.max_steps(n):
            raise ValueError(f"{n} slots of {fe.n_steps} steps exceed the longest launch the reservoir's plan accepts "
                             f"({net.max_steps(n)} steps): fewer streams, or a smaller max_bins")
        raster, steps = fe.encode_ragged(audio, bins)
        return net.run_batch(raster, self.feature_keys, lengths=steps)[0]

    def _rows(self, utt, compact: bool):
        with torch.cuda.device(self.net.device):
            if not compact:
                return self._run(utt.audio, utt.bins)
            from .snn import _select_keys
            bins = utt.bins.cpu().numpy()                               # the one read-back of a compact push
            idx = np.nonzero(bins)[0]
            rows = torch.zeros((len(bins), len(_select_keys(self.feature_keys)[0]) * self.net.num_output_neurons),
                               dtype=torch.float32, device=self.net.device)
            if len(idx):
                where = torch.from_numpy(idx).to(self.net.device)
                rows[where] = self._run(utt.audio[where], bins[idx])
            return rows

    def push(self, audio, hops=None, finish=None, compact: bool = False):
        """``audio``, ``hops`` and ``finish`` as ``frontend.EndpointStream.push`` takes them (with a ``resampler``: PCM at its
        input rate and per-stream UNIT counts, as `AudioStreamBank.push`).  Returns ``(rows, bins, first, flags)``, device
        tensors over the push's ``n_streams * max_utts`` slots, slot ``b * max_utts + u`` stream b's u-th utterance: ``rows``
        float32 (slots, n_feat), ``bins`` int32 -- 0 for an empty slot, whose row is unspecified --, ``first`` int64 and
        ``flags`` int32.  Nothing is read on the host: ``bins`` goes to the ragged launches as the endpoint kernel wrote it.
        ``compact`` = True reads ``bins`` back once and runs only the emitted slots (rows of empty slots: zeros): the same
        bytes for the emitted ones."""
        utt = self.cut(audio, hops, finish)
        return self._rows(utt, compact), utt.bins, utt.first, utt.flags

    def push_scores(self, audio, hops=None, finish=None, compact: bool = False):
        """``push`` with ``readout.score_rows`` behind it: ``(logits, labels, bins, first, flags)`` -- float64 (slots,
        n_classes) and int32 (slots,); logits and labels of empty slots are unspecified."""
        if self.readout is None:
            raise ValueError("push_scores needs a readout: UtteranceBank(..., readout=readout.DeviceReadout(model, device))")
        utt = self.cut(audio, hops, finish)
        logits, labels = self.readout.score_rows(self._rows(utt, compact))
        return logits, labels, utt.bins, utt.first, utt.flags


def utterances_from_recordings(recordings, endpoint_params=None, chunk_hops: int = 100, device=None):
    """Whole recordings cut into utterances: ``recordings``, a list of n 1-D float32 arrays (zero-padded to whole bins of 160
    samples), go through one ``frontend.EndpointStream(n, **endpoint_params)`` in pushes of ``chunk_hops`` hops, each
    recording with ``finish`` at its end.  Returns ``(utterances, table)``: a list of 1-D float32 host arrays and an int64
    array (len, 4) of ``(recording, first_bin, bins, flags)`` per utterance, ordered by recording, then by time -- what
    `features_from_utterances` takes.  One read-back per push."""
    from .frontend import EndpointStream
    arrays = [np.ascontiguousarray(np.asarray(r, dtype=np.float32)) for r in recordings]
    for r, a in enumerate(arrays):
        if a.ndim != 1:
            raise ValueError(f"recording {r} must be a 1-D array, got shape {tuple(a.shape)}")
    n, H = len(arrays), int(chunk_hops)
    if n < 1 or H < 1:
        raise ValueError(f"utterances_from_recordings needs at least one recording and chunk_hops >= 1, got {n}, {chunk_hops}")
    ep = EndpointStream(n, device=device, **(endpoint_params or {}))
    U = ep.max_utterances(H)
    nb = np.array([-(-len(a) // RAGGED_HOP) for a in arrays], dtype=np.int64)
    found = [[] for _ in range(n)]
    for lo in range(0, max(int(nb.max()), 1), H):
        block = np.zeros((n, H * RAGGED_HOP), dtype=np.float32)
        for r, a in enumerate(arrays):
            part = a[lo * RAGGED_HOP:(lo + H) * RAGGED_HOP]
            block[r, :len(part)] = part
        hops = np.clip(nb - lo, 0, H)
        ends = ((nb > lo) | (lo == 0)) & (nb <= lo + H)                 # the push that holds the recording's last bin
        utt = ep.push(block, hops, ends.astype(np.int64))
        count, bins = utt.count.cpu().numpy(), utt.bins.cpu().numpy().reshape(n, U)
        if not count.any():
            continue
        audio, first, flags = utt.audio.cpu().numpy().reshape(n, U, -1), utt.first.cpu().numpy().reshape(n, U), \
            utt.flags.cpu().numpy().reshape(n, U)
        for r in range(n):
            for u in range(int(count[r])):
                found[r].append((audio[r, u, :RAGGED_HOP * int(bins[r, u])].copy(), (r, int(first[r, u]), int(bins[r, u]),
                                                                                     int(flags[r, u]))))
    utterances = [x for per in found for x, _ in per]
    table = np.array([row for per in found for _, row in per], dtype=np.int64).reshape(-1, 4)
    return utterances, table


def sliding_features_from_recordings(recordings, fe, net, feature_keys, segment_steps: int, window_segments: int,
                                     hop_segments: int = 1):
    """``sliding_features_from_long_audio`` for recordings of different lengths in one batch: ``recordings``, a list of n
    1-D float32 arrays of ``W_r * fe.n_samples`` samples each (W_r >= 1 whole audio windows), -> ``(rows, counts)``: ``rows``
    float32 (n, Wn, n_feat) on the device, ``counts`` (int64, host).  ``rows[r, :counts[r]]`` are the sliding-window rows of
    recording r alone; rows past a count are zeros.  The front end and the scatter are ``features_from_recordings``'; the
    reservoir takes W_max stream launches with its state carried (``SNN.run_stream_records``, SPEC.md §4d): in launch w a
    recording that still has an audio window runs all its segments, one that has ended rides along with 0."""
    S = int(segment_steps)
    if S < 1 or fe.n_steps % S:
        raise ValueError(f"segment_steps = {segment_steps} must be >= 1 and divide the front end's {fe.n_steps} steps")
    arrays, windows = _recording_windows(recordings, fe, "sliding_features_from_recordings")
    n, w_max = len(arrays), int(windows.max())
    Gt = fe.n_steps // S                                                # segments per audio window
    K, H = int(window_segments), int(hop_segments)
    net.segment_windows(w_max * Gt, K, H)                               # refuse before anything is launched
    valid = windows * Gt
    counts = completed_windows(valid, K, H)
    with torch.cuda.device(net.device):
        rasters = _scatter_recording_windows(arrays, windows, fe, net)
        state = net.new_state(n)
        records = torch.cat([net.run_stream_records(rasters[:, w].contiguous(), S, segments=np.where(windows > w, Gt, 0),
                                                    state=state)[0] for w in range(w_max)], dim=1)
        return net.segment_features(records, S, feature_keys, K, H, segments=valid), counts
