"""The first refusal wins in the two gammatone entry points: a call that is wrong in two ways at once returns LSM_ERR_ARG
with the message of the check that csrc/frontend.hip reaches first, word for word.  The order is part of the ABI's
behaviour -- it decides which reason a caller reads -- and the two entry points do not share it: the split one accepts an
empty batch before it looks at buffers and windows, the fused one after every argument check (threshold tables included)
and before the buffers.  The fused one's masked and ragged twins refuse what it refuses, in its order and words, and their own
arguments after that.  Shapes of 2 filters x 16 samples; every call is refused or empty, so nothing is launched and the
host arrays passed as buffers are never read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LSM_OK, LSM_ERR_ARG = 0, -1
TWO_FILTERS = (b"the gammatone filterbank needs n_filters >= 2 (one channel: NumPy's pairwise window sums, "
               b"SPEC.md 1.1)")
FLAGS = b"launch_flags: only bit 0 (low-latency layout) and bit 1 (no LDS reservation) are defined"
WINDOWS = b"nwin=17 needs more than 4 overlapping windows of hop=4"
COLUMNS = b"columns exceed the clip"

SPEC_PARAMS = "audio n_clips n_samples coefs n_filters nwin hop ncols spec_out db_out coef_flags stream".split()
SPIKES_PARAMS = ("audio n_clips n_samples coefs n_filters nwin hop ncols time_bins thr_on thr_off n_thr redundancy raster "
                 "workspace workspace_bytes coef_flags launch_flags stream").split()
# (the two bad arguments, the message that wins); "+k" is the good address plus k bytes
SPEC_BOTH_BAD = [
    (dict(n_samples=0, n_filters=1), b"bad shape"),
    (dict(n_filters=1, nwin=0), TWO_FILTERS),
    (dict(audio=None, spec_out=None, db_out=None), b"gammatone: null input"),
    (dict(spec_out=None, db_out=None, hop=0), b"gammatone: both outputs null"),
    (dict(hop=0, nwin=1), b"bad window"),
    (dict(ncols=0, nwin=17), b"bad window"),
    (dict(nwin=17), WINDOWS),                                   # 17 > 4 * 4, and (4 - 1) * 4 + 17 > 16
    (dict(n_samples=7), COLUMNS),                               # (4 - 1) * 4 + 4 > 7, and 7 < 8
]
SPIKES_BOTH_BAD = [
    (dict(launch_flags=4, n_samples=0), FLAGS),
    (dict(n_samples=0, n_filters=1), b"bad shape"),
    (dict(n_filters=1, nwin=0), TWO_FILTERS),
    (dict(time_bins=1, nwin=17), b"bad window"),
    (dict(nwin=17), WINDOWS),
    (dict(n_samples=7), COLUMNS),
    (dict(n_samples=7, nwin=1, hop=1, ncols=2, n_thr=9), b"clips shorter than 8 samples are not supported"),
    (dict(n_thr=9, thr_on=None), b"n_thr=9 outside [1, 8]"),
    (dict(redundancy=0, thr_off=None), b"redundancy must be >= 1"),
    (dict(thr_on=None, raster=None), b"null threshold table"),
    (dict(raster=None, workspace_bytes=8), b"gammatone_spikes: null buffer"),
    (dict(workspace_bytes=8, workspace="+4"), b"workspace of 8 bytes, need 4096 (lsm_gammatone_spikes_workspace)"),
    (dict(workspace="+4", raster="+1"), b"workspace must be 8-byte aligned"),
]
# The masked and the ragged twin (include/lsm_hip_mask.h, lsm_hip_ragged.h): "the twin's refusals first, in the twin's order"
# is the whole table above, word for word; then each form's own refusal loses to the last of the twin's, and stands alone.
MASKED_PARAMS = SPIKES_PARAMS[:-1] + ["freq_mask", "time_mask", "stream"]
RAGGED_PARAMS = ("audio n_clips n_samples coefs n_filters nwin hop ncols time_bins clip_bins thr_on thr_off n_thr redundancy "
                 "raster clip_steps_out workspace workspace_bytes coef_flags launch_flags stream").split()
MASKED_OWN = [
    (dict(freq_mask="+1", workspace="+4"), b"workspace must be 8-byte aligned"),
    (dict(time_mask="+2"), b"freq_mask and time_mask must be 4-byte aligned"),
]
RAGGED_OWN = [
    (dict(clip_bins="+1", workspace="+4"), b"workspace must be 8-byte aligned"),
    (dict(clip_bins=None, time_bins=2, ncols=2), b"ragged: null per-clip count array"),
    (dict(clip_bins="+1", clip_steps_out="+2"), b"ragged: per-clip count arrays must be 4-byte aligned"),
    (dict(clip_steps_out="+2"), b"ragged: clip_steps_out must be 4-byte aligned"),
]


def test_the_first_refusal_wins_in_both_gammatone_entry_points():
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    n_clips, n_samples, n_filters, nwin, hop, ncols, time_bins, n_thr = 1, 16, 2, 4, 4, 4, 4, 4
    assert (ncols - 1) * hop + nwin == n_samples
    need = lib.lsm_gammatone_spikes_workspace(n_clips, n_filters, ncols)
    assert need == 4096
    audio = np.zeros((n_clips, n_samples), dtype=np.float32)
    coefs = np.ones((n_filters, 10), dtype=np.float64)
    thr_on, thr_off = np.full(8, 0.5), np.full(8, 0.25)
    spec_out, db_out = (np.full((n_clips, n_filters, ncols), np.nan) for _ in range(2))
    raster = np.full((n_clips, n_filters, time_bins * n_thr + 8), 0xAB, dtype=np.uint8)
    workspace = np.full(need // 8 + 1, np.nan)
    assert workspace.ctypes.data % 8 == 0 and raster.ctypes.data % 4 == 0 and (time_bins * n_thr) % 4 == 0
    # the twins' own arrays (device arrays in a launch; here never read): mask words, bin counts in, step counts out
    masks = np.full(4, 0xABABABAB, dtype=np.uint32)
    counts = np.full(4, 0x2B2B2B2B, dtype=np.int32)
    assert masks.ctypes.data % 4 == 0 and counts.ctypes.data % 4 == 0
    assert time_bins >= 3 and n_samples >= hop * time_bins            # the ragged preconditions hold for the good call
    twins_own = dict(freq_mask=masks.ctypes.data, time_mask=masks.ctypes.data + 8, clip_bins=counts.ctypes.data,
                     clip_steps_out=counts.ctypes.data + 8)
    good = dict(**twins_own,audio=audio.ctypes.data, n_clips=n_clips, n_samples=n_samples, coefs=coefs.ctypes.data,
                n_filters=n_filters, nwin=nwin, hop=hop, ncols=ncols, time_bins=time_bins, thr_on=thr_on.ctypes.data,
                thr_off=thr_off.ctypes.data, n_thr=n_thr, redundancy=1, spec_out=spec_out.ctypes.data,
                db_out=db_out.ctypes.data, raster=raster.ctypes.data, workspace=workspace.ctypes.data,
                workspace_bytes=need, coef_flags=0, launch_flags=0, stream=None)

    def call(export, params, changed):
        values = {**good, **{name: good[name] + int(v) if isinstance(v, str) else v for name, v in changed.items()}}
        assert set(changed) <= set(params), (export, changed)
        assert lib.lsm_reservoir_set_kernel(None, 0) == LSM_ERR_ARG        # another message, so a stale one cannot pass
        return getattr(lib, export)(*[values[name] for name in params])

    for export, params, table in (("lsm_gammatone_spec_f64", SPEC_PARAMS, SPEC_BOTH_BAD),
                                  ("lsm_gammatone_spikes_f64", SPIKES_PARAMS, SPIKES_BOTH_BAD),
                                  ("lsm_gammatone_spikes_masked_f64", MASKED_PARAMS, SPIKES_BOTH_BAD + MASKED_OWN),
                                  ("lsm_gammatone_spikes_ragged_f64", RAGGED_PARAMS, SPIKES_BOTH_BAD + RAGGED_OWN)):
        for bad, message in table:
            rc = call(export, params, bad)
            assert rc == LSM_ERR_ARG and lib.lsm_last_error() == message, (export, bad, rc, lib.lsm_last_error())

    # an empty batch: accepted with null buffers by both (the fused entry point has checked the threshold tables by then)
    buffers = dict.fromkeys(["audio", "coefs", "spec_out", "db_out", "raster", "workspace"])
    assert call("lsm_gammatone_spec_f64", SPEC_PARAMS, {**{k: None for k in buffers if k in SPEC_PARAMS},
                                                        "n_clips": 0}) == LSM_OK, lib.lsm_last_error()
    empty = {**{k: None for k in buffers if k in SPIKES_PARAMS}, "n_clips": 0, "workspace_bytes": 0}
    assert call("lsm_gammatone_spikes_f64", SPIKES_PARAMS, empty) == LSM_OK, lib.lsm_last_error()
    assert call("lsm_gammatone_spikes_f64", SPIKES_PARAMS, {**empty, "thr_on": None, "thr_off": None}) == LSM_ERR_ARG
    assert lib.lsm_last_error() == b"null threshold table"
    # the twins likewise, with null buffers and with null mask and count arrays as well
    for export, params in (("lsm_gammatone_spikes_masked_f64", MASKED_PARAMS), ("lsm_gammatone_spikes_ragged_f64", RAGGED_PARAMS)):
        assert call(export, params, empty) == LSM_OK, (export, lib.lsm_last_error())
        own = {k: None for k in twins_own if k in params}
        assert call(export, params, {**empty, **own}) == LSM_OK, (export, lib.lsm_last_error())
    # ... and before the windows by the split entry point, after them by the fused one
    assert call("lsm_gammatone_spec_f64", SPEC_PARAMS, dict(n_clips=0, nwin=17)) == LSM_OK, lib.lsm_last_error()
    assert call("lsm_gammatone_spikes_f64", SPIKES_PARAMS, dict(n_clips=0, nwin=17)) == LSM_ERR_ARG
    assert lib.lsm_last_error() == WINDOWS

    # nothing was launched: no buffer was written
    assert np.isnan(spec_out).all() and np.isnan(db_out).all() and np.isnan(workspace).all() and (raster == 0xAB).all()
    assert (masks == 0xABABABAB).all() and (counts == 0x2B2B2B2B).all()
