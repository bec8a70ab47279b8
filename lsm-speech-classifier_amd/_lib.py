"""ctypes binding of liblsm_hip.so (include/lsm_hip.h).  There is no CPU fallback: if the
library is missing or a call fails, this module raises."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

_lib = None
ABI_VERSION = _build.version_number()      # lsm_version() of a library built from this tree (= __version__, one literal)

c_void = C.c_void_p
c_int = C.c_int
c_float = C.c_float

_SIGS = {
    "lsm_version": (c_int, []),
    "lsm_build_id": (C.c_char_p, []),
    "lsm_last_error": (C.c_char_p, []),
    "lsm_device_count": (c_int, []),
    "lsm_gammatone_spec_f64": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_int,
                                       c_void, c_void, c_int, c_void]),
    "lsm_gammatone_spikes_workspace": (C.c_long, [c_int, c_int, c_int]),
    "lsm_gammatone_spikes_layout": (c_int, [c_int, c_int, c_int]),
    "lsm_gammatone_spikes_f64": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_int, c_int,
                                         c_void, c_void, c_int, c_int, c_void, c_void, C.c_long, c_int, c_int, c_void]),
    "lsm_spec_to_spikes_f64": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void,
                                       c_int, c_int, c_void, c_void, c_void]),
    "lsm_spec_to_spikes_f32": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void,
                                       c_int, c_int, c_void, c_void, c_void]),
    "lsm_mel_power_f32": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void, c_void,
                                  c_void, c_void, c_int, c_void, c_void]),
    "lsm_power_to_db_f32": (c_int, [c_void, c_int, c_int, c_float, c_float, c_void, c_void]),
    "lsm_mel_spikes_workspace": (C.c_long, [c_int, c_int, c_int]),
    "lsm_mel_spikes_f32": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void, c_void,
                                   c_int, c_float, c_float, c_int, c_void, c_void, c_int, c_int, c_void, c_void, C.c_long,
                                   c_void]),
    "lsm_encode_hysteresis_f64": (c_int, [c_void, c_int, c_int, c_void, c_void, c_int, c_void, c_void]),
    "lsm_encode_hysteresis_f32": (c_int, [c_void, c_int, c_int, c_void, c_void, c_int, c_void, c_void]),
    "lsm_raster_pack_bits": (c_int, [c_void, C.c_long, c_int, c_void, c_void]),
    "lsm_raster_unpack_bits": (c_int, [c_void, C.c_long, c_int, c_void, c_void]),
    "lsm_reservoir_create": (c_int, [C.POINTER(c_void), c_int, c_int, c_void, c_void, c_void, c_void,
                                     c_void, c_int, c_float, c_void, c_int, c_float, c_int, c_int]),
    "lsm_reservoir_destroy": (c_int, [c_void]),
    "lsm_reservoir_set_kernel": (c_int, [c_void, c_int]),
    "lsm_reservoir_kernel_in_use": (c_int, [c_void]),
    "lsm_reservoir_run": (c_int, [c_void, c_void, c_int, c_int, c_void, c_int, c_void, c_void,
                                  c_void, c_void, c_int, c_void]),
    "lsm_reservoir_order_workspace": (C.c_long, [c_int]),
    "lsm_reservoir_run_ordered": (c_int, [c_void, c_void, c_int, c_int, c_void, c_int, c_void, c_void,
                                          c_void, c_void, c_int, c_void, C.c_long, c_void]),
    "lsm_reservoir_state_bytes": (C.c_long, [c_void]),
    "lsm_reservoir_run_from": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void, c_void, c_int, c_void,
                                       c_void, c_void, c_void, c_int, c_void, C.c_long, c_void]),
    "lsm_reservoir_run_ragged": (c_int, [c_void, c_void, c_int, c_int, c_void, c_int, c_void, c_void, c_void, c_int, c_void,
                                         c_void, c_void, c_void, c_int, c_void, C.c_long, c_void]),
    "lsm_reservoir_run_segments": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void,
                                           c_int, c_void, c_void, c_void, c_void, c_int, c_void, C.c_long, c_void]),
    "lsm_segment_features": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_int, c_void, c_void]),
    "lsm_reservoir_max_steps": (c_int, [c_void, c_int, c_int]),
    "lsm_reservoir_layout": (c_int, [c_void, c_int, c_int, c_int, C.POINTER(c_int),
                                     C.POINTER(c_int), C.POINTER(c_int)]),
    "lsm_reservoir_plan": (c_int, [c_void, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int),
                                   C.POINTER(c_int), C.POINTER(c_int), C.POINTER(C.c_long)]),
    "lsm_reservoir_row_request_bytes": (c_int, [c_void, c_int, c_int, c_int, C.POINTER(C.c_double)]),
    "lsm_reservoir_input_mode": (c_int, [c_void, c_int, c_int, c_int]),
    "lsm_reservoir_ring_form": (c_int, [c_void, c_int, c_int, c_int]),
    "lsm_debug_pair_layout": (c_int, [c_int, c_void, c_void, c_void, c_int, C.c_ulonglong, C.c_ulonglong,
                                      C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(c_int), c_void, c_void, c_void]),
    "lsm_debug_pair_inputs": (c_int, [c_int, c_int, c_void, c_int, c_int, c_void, c_void]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

# include/lsm_hip_streams.h (SPEC.md §4d): bound beside the table above, which stays the mirror of include/lsm_hip.h
STREAM_SIGS = {
    "lsm_reservoir_run_stream": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void, c_void, c_void, c_void,
                                         c_void, c_void, c_int, c_void, C.c_long, c_void]),
    "lsm_segment_features_ragged": (c_int, [c_void, c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_void, c_int,
                                            c_void, c_void]),
}
STREAM_SYMBOLS = tuple(STREAM_SIGS)

# include/lsm_hip_audio.h (SPEC.md §1.6): the streamed gammatone front end, a table of its own likewise
c_double = C.c_double
AUDIO_SIGS = {
    "lsm_gammatone_stream_state_bytes": (C.c_long, [c_int, c_int, c_int]),
    "lsm_gammatone_stream_f64": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_void, c_double, c_double,
                                         c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_void, c_int,
                                         c_void]),
}
AUDIO_SYMBOLS = tuple(AUDIO_SIGS)

# include/lsm_hip_mel_stream.h (SPEC.md §1.7): the streamed mel front end
MEL_STREAM_SIGS = {
    "lsm_mel_stream_state_bytes": (C.c_long, [c_int, c_int, c_int]),
    "lsm_mel_stream_workspace": (C.c_long, [c_int, c_int, c_int]),
    "lsm_mel_stream_f32": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void, c_void, c_int,
                                   c_void, c_double, c_double, c_void, c_void, c_int, c_int, c_void, c_void, c_void,
                                   c_void, c_void, c_void, C.c_long, c_void]),
}
MEL_STREAM_SYMBOLS = tuple(MEL_STREAM_SIGS)

# include/lsm_hip_resample.h (SPEC.md §1.8): the polyphase resampler, batch and streamed
RESAMPLE_SIGS = {
    "lsm_resample_state_bytes": (C.c_long, [c_int, c_int]),
    "lsm_resample_f32": (c_int, [c_void, c_int, c_int, c_int, c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void]),
    "lsm_resample_stream_f32": (c_int, [c_void, c_int, c_int, c_int, c_void, c_int, c_int, c_int, c_void, c_void, c_void,
                                        c_void, c_void]),
}
RESAMPLE_SYMBOLS = tuple(RESAMPLE_SIGS)

# include/lsm_hip_adaptive.h (SPEC.md §1.9): the adaptive-range encoder behind the streamed front ends' dB columns
_ADAPTIVE_ENCODE = (c_int, [c_void, c_int, c_int, c_int, c_void, c_int, c_void, c_void, c_int, c_int, c_void, c_void, c_void,
                            c_void, c_void, c_void])
ADAPTIVE_SIGS = {
    "lsm_adaptive_state_bytes": (C.c_long, [c_int, c_int, c_int]),
    "lsm_adaptive_encode_f64": _ADAPTIVE_ENCODE,
    "lsm_adaptive_encode_f32": _ADAPTIVE_ENCODE,
}
ADAPTIVE_SYMBOLS = tuple(ADAPTIVE_SIGS)

# include/lsm_hip_mix.h (SPEC.md §1.10): the noise mixer in front of the front ends, batch and streamed
MIX_SIGS = {
    "lsm_mix_power_f32": (c_int, [c_void, c_int, c_int, c_void, c_void]),
    "lsm_mix_f32": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_void, c_void,
                            c_void, c_void, c_void]),
    "lsm_mix_stream_f32": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_void,
                                   c_void, c_void, c_void]),
}
MIX_SYMBOLS = tuple(MIX_SIGS)

# include/lsm_hip_reverb.h (SPEC.md §1.11): reverberation in front of the mixer, batch and streamed
REVERB_SIGS = {
    "lsm_reverb_state_bytes": (C.c_long, [c_int]),
    "lsm_reverb_f32": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_void, c_void, c_int, c_void, c_void]),
    "lsm_reverb_stream_f32": (c_int, [c_void, c_int, c_int, c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_void,
                                      c_void, c_void]),
}
REVERB_SYMBOLS = tuple(REVERB_SIGS)

# include/lsm_hip_speed.h (SPEC.md §1.12): speed perturbation in front of the reverberation, a bank of resampler designs
SPEED_SIGS = {
    "lsm_speed_lds_bytes": (C.c_long, [c_void, c_int]),
    "lsm_speed_f32": (c_int, [c_void, c_int, c_int, c_int, c_void, c_int, c_void, c_int, c_void, c_int, c_void, c_void]),
}
SPEED_SYMBOLS = tuple(SPEED_SIGS)

# include/lsm_hip_mask.h (SPEC.md §1.13): the masked spike encoders -- each its twin's list with freq_mask, time_mask before
# the stream
def _masked(twin: str):
    res, args = _SIGS[twin]
    return res, args[:-1] + [c_void, c_void] + args[-1:]


MASK_SIGS = {
    "lsm_spec_to_spikes_masked_f64": _masked("lsm_spec_to_spikes_f64"),
    "lsm_spec_to_spikes_masked_f32": _masked("lsm_spec_to_spikes_f32"),
    "lsm_gammatone_spikes_masked_f64": _masked("lsm_gammatone_spikes_f64"),
    "lsm_mel_spikes_masked_f32": _masked("lsm_mel_spikes_f32"),
}
MASK_SYMBOLS = tuple(MASK_SIGS)


# include/lsm_hip_ragged.h (SPEC.md §1.14): the ragged front end -- each spike encoder its twin's list with the per-clip DEVICE
# counts after time_bins (and clip_steps_out after the fused launch's raster)
def _ragged_encoder(twin: str):
    res, args = _SIGS[twin]
    return res, args[:5] + [c_void, c_void] + args[5:]


RAGGED_SIGS = {
    "lsm_spec_to_spikes_ragged_f64": _ragged_encoder("lsm_spec_to_spikes_f64"),
    "lsm_spec_to_spikes_ragged_f32": _ragged_encoder("lsm_spec_to_spikes_f32"),
    "lsm_power_to_db_ragged_f32": (c_int, [c_void, c_int, c_int, c_int, c_void, c_float, c_float, c_void, c_void]),
    "lsm_gammatone_spikes_ragged_f64": (c_int, _SIGS["lsm_gammatone_spikes_f64"][1][:9] + [c_void]
                                        + _SIGS["lsm_gammatone_spikes_f64"][1][9:14] + [c_void]
                                        + _SIGS["lsm_gammatone_spikes_f64"][1][14:]),
}
RAGGED_SYMBOLS = tuple(RAGGED_SIGS)


# include/lsm_hip_step.h: a whole step -- lane-pair gammatone front end and dense-row reservoir -- in one launch
STEP_SIGS = {
    "lsm_step_fused_supported": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "lsm_step_fused_f64": (c_int, [c_void, c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void,
                                   c_int, c_int, c_void, C.c_long, c_int, c_void, c_int, c_void, c_void, c_void]),
}
# the forms of the step: the query with `form` last, the masked step with freq_mask, time_mask before the stream, the ragged
# step with the DEVICE clip_bins after time_bins
STEP_SIGS["lsm_step_fused_form_supported"] = (c_int, STEP_SIGS["lsm_step_fused_supported"][1] + [c_int])
STEP_SIGS["lsm_step_fused_masked_f64"] = (c_int, STEP_SIGS["lsm_step_fused_f64"][1][:-1] + [c_void, c_void, c_void])
STEP_SIGS["lsm_step_fused_ragged_f64"] = (c_int, STEP_SIGS["lsm_step_fused_f64"][1][:10] + [c_void]
                                          + STEP_SIGS["lsm_step_fused_f64"][1][10:])
STEP_SYMBOLS = tuple(STEP_SIGS)

# include/lsm_hip_step_state.h (SPEC.md §4f): the step with carried state and time segments -- a query of its own, the plain
# step with first_step, state_in, state_out in front of key_ids, and that list with segment_steps, records_out,
# segment_rows_out in front of the stream
STEP_STATE_SIGS = {
    "lsm_step_fused_state_supported": (c_int, list(STEP_SIGS["lsm_step_fused_supported"][1])),
    "lsm_step_fused_from_f64": (c_int, STEP_SIGS["lsm_step_fused_f64"][1][:17] + [c_int, c_void, c_void]
                                + STEP_SIGS["lsm_step_fused_f64"][1][17:]),
}
STEP_STATE_SIGS["lsm_step_fused_segments_f64"] = (c_int, STEP_STATE_SIGS["lsm_step_fused_from_f64"][1][:-1]
                                                  + [c_int, c_void, c_void, c_void])
STEP_STATE_SYMBOLS = tuple(STEP_STATE_SIGS)

# include/lsm_hip_trim.h (SPEC.md §1.15): silence trimming in front of the ragged front end
TRIM_SIGS = {
    "lsm_trim_lds_bytes": (c_int, [c_int]),
    "lsm_trim_silence_f32": (c_int, [c_void, c_int, c_int, c_int, c_void, c_double, c_int, c_int, c_void, c_int, c_void,
                                     c_void, c_void, c_void]),
}
TRIM_SYMBOLS = tuple(TRIM_SIGS)

# include/lsm_hip_ragged_augment.h (SPEC.md §1.16): the mixer and the masks on ragged launches -- lsm_mix_f32's list with the
# DEVICE clip_samples behind n_samples, each ragged encoder's (and the ragged step's) with freq_mask, time_mask before the stream
def _ragged_masked(sig):
    res, args = sig
    return res, args[:-1] + [c_void, c_void] + args[-1:]


RAGGED_AUGMENT_SIGS = {
    "lsm_mix_ragged_f32": (c_int, MIX_SIGS["lsm_mix_f32"][1][:3] + [c_void] + MIX_SIGS["lsm_mix_f32"][1][3:]),
    "lsm_gammatone_spikes_ragged_masked_f64": _ragged_masked(RAGGED_SIGS["lsm_gammatone_spikes_ragged_f64"]),
    "lsm_spec_to_spikes_ragged_masked_f64": _ragged_masked(RAGGED_SIGS["lsm_spec_to_spikes_ragged_f64"]),
    "lsm_spec_to_spikes_ragged_masked_f32": _ragged_masked(RAGGED_SIGS["lsm_spec_to_spikes_ragged_f32"]),
    "lsm_step_fused_ragged_masked_supported": (c_int, list(STEP_SIGS["lsm_step_fused_supported"][1])),
    "lsm_step_fused_ragged_masked_f64": _ragged_masked(STEP_SIGS["lsm_step_fused_ragged_f64"]),
}
RAGGED_AUGMENT_SYMBOLS = tuple(RAGGED_AUGMENT_SIGS)

# include/lsm_hip_readout.h (SPEC.md §6): scaler and linear readout over feature rows and over the windows of segment records
_MODEL = [c_void, c_void, c_void, c_void]           # mean, scale, coef, intercept
READOUT_SIGS = {
    "lsm_readout_supported": (c_int, [c_int, c_int, c_int]),
    "lsm_readout_rows_f32": (c_int, _MODEL + [c_void, c_int, c_int, c_int, c_int, c_void, c_void, c_void]),
    "lsm_readout_windows": (c_int, [c_void] + _MODEL + [c_void, c_int, c_int, c_void, c_int, c_int, c_int, c_void, c_int,
                                                        c_int, c_void, c_void, c_void]),
}
READOUT_SYMBOLS = tuple(READOUT_SIGS)

# include/lsm_hip_fit.h (SPEC.md §7): the statistics of a standard scaler and a ridge readout, updated from a step's rows
FIT_SIGS = {
    "lsm_fit_supported": (c_int, [c_int, c_int, c_int]),
    "lsm_fit_accumulate_f32": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void, c_void,
                                       c_void]),
}
FIT_SYMBOLS = tuple(FIT_SIGS)

# include/lsm_hip_endpoint.h (SPEC.md §1.17): stream endpointing -- utterances cut from audio streams into ragged slots
ENDPOINT_SIGS = {
    "lsm_endpoint_state_bytes": (C.c_long, [c_int, c_int]),
    "lsm_endpoint_max_utterances": (c_int, [c_int, c_int, c_int]),
    "lsm_endpoint_stream_f32": (c_int, [c_void, c_int, c_int, c_void, c_void, c_double, c_double, c_int, c_int, c_int, c_int,
                                        c_int, c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_void, c_void,
                                        c_void]),
}
ENDPOINT_SYMBOLS = tuple(ENDPOINT_SIGS)

# include/lsm_hip_ragged_speed.h (SPEC.md §1.18): speed perturbation on ragged batches -- lsm_speed_f32's list with the DEVICE
# clip_samples behind n_in and clip_samples_out, clip_bins_out, time_bins in front of the stream; the length formula, host only
RAGGED_SPEED_SIGS = {
    "lsm_speed_ragged_length": (c_int, [c_int, c_int, c_int, c_int]),
    "lsm_speed_ragged_f32": (c_int, SPEED_SIGS["lsm_speed_f32"][1][:4] + [c_void] + SPEED_SIGS["lsm_speed_f32"][1][4:-1]
                             + [c_void, c_void, c_int] + SPEED_SIGS["lsm_speed_f32"][1][-1:]),
}
RAGGED_SPEED_SYMBOLS = tuple(RAGGED_SPEED_SIGS)


class LsmHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises LsmHipError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Import it first so that this
    # library binds to the runtime torch already initialised: two HIP runtimes in one process
    # leave the second one without devices.
    import torch  # noqa: F401
    path = _build.lib_path()
    own = "LSM_HIP_LIB" not in os.environ        # a diagnostic build named by the user is loaded as it is
    # A library that is absent, of another version or built from other sources than this tree's (build.source_id, linked
    # into the binary) is rebuilt ONCE -- hipcc runs as a child process, nothing here touches the GPU -- and refused if
    # that does not help: never a silent stale binary, never a CPU fallback.
    if own and _build.needs_build(path) and os.environ.get("LSM_NO_AUTO_BUILD") != "1":
        try:
            import fcntl
            os.makedirs(os.path.join(_build.PKG_DIR, "build"), exist_ok=True)
            with open(os.path.join(_build.PKG_DIR, "build", ".lock"), "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)         # the ranks of a launcher find the same stale library together
                _build.build()                           # (a no-op for every rank but the first)
        except Exception as e:                   # no hipcc (a box that only received the binary): judged below
            import warnings
            warnings.warn(f"rebuilding {path} failed: {e}", RuntimeWarning)
    if not os.path.exists(path):
        raise LsmHipError(
            f"{path} not found: the HIP extension is not built. Run `python -c \"import "
            f"__graft_entry__ as g; g.build()\"` (needs hipcc). There is no CPU fallback.")
    lib = C.CDLL(path)
    try:
        lib.lsm_version.restype = c_int
        have = int(lib.lsm_version())
    except AttributeError:
        have = -1
    if have != ABI_VERSION:              # a stale .so: say so instead of failing on the first new symbol
        raise LsmHipError(
            f"{path} reports ABI version {have}, this package needs {ABI_VERSION}: rebuild the extension "
            f"(`python -c \"import __graft_entry__ as g; g.build()\"`).")
    if own and _build.built_id(path) != _build.source_id():
        raise LsmHipError(
            f"{path} was built from other sources than this tree's (build id {_build.built_id(path)}, sources "
            f"{_build.source_id()}): rebuild the extension (`python -c \"import __graft_entry__ as g; g.build()\"`).")
    for name, (res, args) in (list(_SIGS.items()) + list(STREAM_SIGS.items()) + list(AUDIO_SIGS.items())
                              + list(MEL_STREAM_SIGS.items()) + list(RESAMPLE_SIGS.items()) + list(ADAPTIVE_SIGS.items())
                              + list(MIX_SIGS.items()) + list(REVERB_SIGS.items()) + list(SPEED_SIGS.items())
                              + list(MASK_SIGS.items()) + list(RAGGED_SIGS.items()) + list(STEP_SIGS.items())
                              + list(STEP_STATE_SIGS.items()) + list(TRIM_SIGS.items()) + list(RAGGED_AUGMENT_SIGS.items())
                              + list(READOUT_SIGS.items()) + list(FIT_SIGS.items()) + list(ENDPOINT_SIGS.items())
                              + list(RAGGED_SPEED_SIGS.items())):
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().lsm_last_error().decode("utf-8", "replace")
        raise LsmHipError(f"{what or 'liblsm_hip call'} failed ({rc}): {msg}")


def require_gpu() -> int:
    """Number of HIP devices; raises when there is none (the product path never runs on CPU)."""
    n = load().lsm_device_count()
    if n <= 0:
        msg = load().lsm_last_error().decode("utf-8", "replace")
        raise LsmHipError(f"no HIP device visible ({n}): {msg}")
    return n
