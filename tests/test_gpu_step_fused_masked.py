"""The masked one-launch step (`lsm_step_fused_masked_f64`, `pipeline.step_fused(mask=...)`): all six kernel forms, the word
edges of the two masks, a resized spectrogram, null and trivial masks, more clips than compute units, and the refusals.
Every case is compared bit for bit with (a) the two launches it replaces, `net.run_batch(fe.encode(x, mask=plan), keys,
waves_per_clip=-1)`, rows and `stats_out`; (b) the NumPy restatement of SPEC.md 1.13 (tests/mask_restatement.py) for the
raster; (c) the C oracle's `lif_run` on that raster, `stats_out` against its spike matrix.

What keeps the comparisons from being vacuous is asserted: in the form cases every clip keeps input spikes and reservoir
spikes under its mask, every masked clip's rows differ from its unmasked rows, and a masked raster differs from the unmasked
raster with the masked cells zeroed (the latch rule of 1.13: a masked value is +0.0 BEFORE the latches).  The stock clips of
test_gpu_step_fused_range.py meet all of it with the bands of tests/step_fused_forms_ref.py (checked there on the CPU with the
restatement and the oracle alone), so neither clips nor conditions were changed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_restatement as MR  # noqa: E402
import step_fused_forms_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu
_built = {}


def _build(oracle_c, F, bins, n_thr, hop, N):
    """Front end, reservoir and the three clips of a shape, built once; the tests leave them as they are."""
    key = (F, bins, n_thr, hop, N)
    if key not in _built:
        from lsm_speech_classifier_amd import frontend, snn
        fe = frontend.SpikeFrontEnd(F, "gammatone", thresholds=REF.thresholds(n_thr), time_bins=bins, n_samples=bins * hop)
        sh = REF.shape(F, bins, n_thr, hop)
        assert (fe.nwin, fe.hop, fe.ncols, fe.gap) == (sh.nwin, sh.hop, sh.ncols, sh.gap) and fe.coef_flags == 7
        net = snn.SNN(None, reservoir=REF.reservoir(oracle_c, F, bins, n_thr, hop, N))
        _built[key] = fe, net, REF.clips(bins * hop), sh
    return _built[key]


def _table_3(fe, sh):
    """A front end of the same shape on the range test's channel-dependent table (coef_flags 3), and that table."""
    import torch
    from lsm_speech_classifier_amd import frontend
    tab = REF.coef_table_3(sh.tab)
    fe3 = frontend.SpikeFrontEnd(sh.F, "gammatone", thresholds=sh.thresholds, time_bins=sh.bins, n_samples=sh.n_samples)
    fe3.coefs = torch.from_numpy(tab).cuda()
    fe3.coef_flags = frontend.coef_flags(tab)
    assert fe3.coef_flags == 3
    return fe3, tab


def _check(oracle_c, fe, net, sh, audio, fm, tm, plan=None, tab=None, keys=None, live_min=0, oracle_clips=None):
    """The masked step on `audio` under bool masks fm (B, F), tm (B, bins) (or `plan`, the words to launch with) against (a),
    (b) and (c) of the module's text.  Returns (rows, masked rasters of the restatement, unmasked rows)."""
    import torch
    from lsm_speech_classifier_amd import pipeline
    B = len(audio)
    plan = REF.plan_of(fm, tm) if plan is None else plan
    assert pipeline.step_fused_supported(fe, net, B, "masked") and pipeline.step_fused_supported(fe, net, B)
    x = torch.from_numpy(audio).cuda()
    stats = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    got = pipeline.step_fused(fe, net, x, keys, stats_out=stats, mask=plan)
    stats2 = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    rasters = fe.encode(x, mask=plan)
    want = net.run_batch(rasters, keys, stats_out=stats2, waves_per_clip=-1)[0]
    plain = pipeline.step_fused(fe, net, x, keys)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "rows differ from run_batch(encode(x, mask=plan))"
    assert torch.equal(stats, stats2), "stats_out differs from the two launches'"
    rows, st, rasters, plain = got.cpu().numpy(), stats.cpu().numpy(), rasters.cpu().numpy(), plain.cpu().numpy()
    live, restated = 0, {}
    for b in range(B) if oracle_clips is None else oracle_clips:
        raster = REF.masked_raster(oracle_c, sh, audio[b], fm[b], tm[b], tab)
        np.testing.assert_array_equal(raster, rasters[b], err_msg=f"clip {b}: raster")
        feats, want_st, sm = REF.lif(oracle_c, net.reservoir, raster, keys)
        np.testing.assert_array_equal(rows[b], feats, err_msg=f"clip {b}: rows")
        assert st[b].tolist() == want_st, f"clip {b}: stats_out"
        live += bool(raster.any() and sm.any())
        restated[b] = raster
    assert live >= live_min, f"{live} clips with input and reservoir spikes under their masks"
    return rows, restated, plain


# 1. all six masked forms

@pytest.mark.parametrize("N", [256, 384, 1000])
def test_every_masked_form_equals_the_two_launches_the_restatement_and_the_oracle(oracle_c, N):
    """F = 128, 16 bins x 4 thresholds on hop 160 (T = 64), masks that differ per clip; the stock table (shared first-section
    gain) and the coef_flags 3 table on the same reservoir: 1, 2 and 4 slots per lane x the two forms."""
    fe, net, audio, sh = _build(oracle_c, 128, 16, 4, 160, N)
    assert net.plan(3, 64, -1)["slots_per_lane"] == {256: 1, 384: 2, 1000: 4}[N]
    fm, tm = REF.form_masks()
    assert len({fm[b].tobytes() + tm[b].tobytes() for b in range(3)}) == 3
    fe3, tab3 = _table_3(fe, sh)
    latch = 0
    for f, tab in ((fe, None), (fe3, tab3)):
        rows, restated, plain = _check(oracle_c, f, net, sh, audio, fm, tm, tab=tab, live_min=2)
        for b in range(3):
            assert not np.array_equal(rows[b], plain[b]), f"clip {b}: the mask changed nothing"
            unmasked = REF.oracle_raster(oracle_c, sh, audio[b], tab)
            latch += not np.array_equal(restated[b], MR.zeroed_raster(unmasked, 4, 1, fm[b], tm[b]))
    assert latch >= 1, "no clip shows the latch rule: masking equals zeroing raster cells everywhere"


# 2. word edges, four time words, a resized spectrogram

def test_only_valid_bit_of_the_last_words_and_bits_beyond_the_axes(oracle_c):
    """(97, 33, 1, 160, 257): filter 96 is the only valid bit of the fourth frequency word, bin 32 of the second time word;
    every bit at or beyond F and time_bins is set in the words and must be ignored."""
    fe, net, audio, sh = _build(oracle_c, 97, 33, 1, 160, 257)
    fm, tm, plan = REF.edge_masks_97_33()
    assert plan.freq.shape == (3, 4) and plan.time.shape == (3, 2)
    assert (plan.freq[:, 3] == 0xFFFFFFFF).all() and (plan.time[:, 1] == 0xFFFFFFFF).all()
    assert MR.bits_of(plan.freq, 97)[:, 96].all() and MR.bits_of(plan.time, 33)[:, 32].all()
    rows, restated, plain = _check(oracle_c, fe, net, sh, audio, fm, tm, plan=plan, live_min=2)
    clean = _check(oracle_c, fe, net, sh, audio, fm, tm)[0]              # the same masks without the stray bits
    assert np.array_equal(rows, clean)
    for b in range(3):
        assert not np.array_equal(rows[b], plain[b])
        assert not restated[b][96].any() and not restated[b][:, 32].any()


@pytest.mark.parametrize("shape,masks", [((128, 100, 4, 160, 64), "straddle_masks"), ((128, 10, 4, 199, 300), "resized_masks")])
def test_four_time_words_and_resized_bins(oracle_c, shape, masks):
    """(128, 100, 4, 160, 64): four time words, T = 400, bands across bins 31|32 and 63|64.  (128, 10, 4, 199, 300): 8 columns
    resized to 10 bins on a hop of 199 samples, so the mask indexes the resized bins."""
    fe, net, audio, sh = _build(oracle_c, *shape)
    assert (fe.hop, fe.ncols, fe.time_bins) == ((160, 98, 100) if masks == "straddle_masks" else (199, 8, 10))
    fm, tm = getattr(REF, masks)()
    rows, _, plain = _check(oracle_c, fe, net, sh, audio, fm, tm, live_min=2)
    for b in range(3):
        assert not np.array_equal(rows[b], plain[b])


# 3. null and trivial masks

def test_null_and_trivial_masks(oracle_c):
    """One mask pointer NULL (through the C ABI), both NULL and an all-clear mask against the plain step, a clip with every
    filter masked, and a clip with a NaN sample under a mask."""
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, pipeline
    from lsm_speech_classifier_amd.snn import _dev, _host, _select_keys
    fe, net, audio, sh = _build(oracle_c, 128, 16, 4, 160, 384)
    fm, tm = REF.form_masks()
    x = torch.from_numpy(audio).cuda()
    plain_stats = torch.full((3, 2), -1, dtype=torch.int32, device="cuda")
    plain = pipeline.step_fused(fe, net, x, stats_out=plain_stats)
    keys, key_ids = _select_keys(None)
    on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
    ws = fe.new_workspace(3)

    def launch(freq, time):
        out = torch.full_like(plain, -7.0)
        st = torch.full((3, 2), -1, dtype=torch.int32, device="cuda")
        _lib.check(fe.lib.lsm_step_fused_masked_f64(
            net._handle, _dev(x), 3, fe.n_samples, _dev(fe.coefs), fe.n_filters, fe.nwin, fe.hop, fe.ncols, fe.time_bins,
            _host(on), _host(off), len(on), fe.redundancy, _dev(ws), ws.numel() * 8, fe.coef_flags, _host(key_ids), len(keys),
            _dev(out), _dev(st), None if freq is None else _dev(freq), None if time is None else _dev(time), fe._stream()))
        torch.cuda.synchronize()
        return out, st

    fw, tw = frontend.upload_mask(REF.plan_of(fm, tm), 3, 128, 16, fe.device)
    none = np.zeros_like
    only_f, _ = launch(fw, None)
    assert torch.equal(only_f, pipeline.step_fused(fe, net, x, mask=REF.plan_of(fm, none(tm))))
    only_t, _ = launch(None, tw)
    assert torch.equal(only_t, pipeline.step_fused(fe, net, x, mask=REF.plan_of(none(fm), tm)))
    assert not torch.equal(only_f, plain) and not torch.equal(only_t, plain) and not torch.equal(only_f, only_t)
    both_null, st = launch(None, None)
    assert torch.equal(both_null, plain) and torch.equal(st, plain_stats)
    stats = torch.full((3, 2), -1, dtype=torch.int32, device="cuda")
    clear = pipeline.step_fused(fe, net, x, stats_out=stats, mask=REF.plan_of(none(fm), none(tm)))
    torch.cuda.synchronize()
    assert torch.equal(clear, plain) and torch.equal(stats, plain_stats)
    # clip 1 with every filter masked: a zero raster, no reservoir spike; clip 2 with a NaN sample under its mask
    fm2, audio2 = fm.copy(), audio.copy()
    fm2[1] = True
    audio2[2, 1000] = np.nan
    _, restated, _ = _check(oracle_c, fe, net, sh, audio2, fm2, tm, live_min=1)
    assert not restated[1].any() and not restated[2].any()
    stats = torch.full((3, 2), -1, dtype=torch.int32, device="cuda")
    pipeline.step_fused(fe, net, torch.from_numpy(audio2).cuda(), stats_out=stats, mask=REF.plan_of(fm2, tm))
    torch.cuda.synchronize()
    assert stats[1].tolist() == [0, 0] and stats[2].tolist() == [0, 0] and stats[0, 1] > 0


# 4. more clips than compute units: the mask row follows the batch position

def test_three_hundred_clips_with_masks_on_three_of_them(oracle_c):
    """300 clips of 5 bins x 4 thresholds, N = 100, a mask on clips 0, 150 and 299 only: every row against the two launches,
    the three masked rows and three unmasked ones against the oracle, and each masked row against the same clip in a batch
    of three."""
    import torch
    from lsm_speech_classifier_amd import pipeline, synth
    fe, net, _, sh = _build(oracle_c, 128, 5, 4, 160, 100)
    audio = np.ascontiguousarray(synth.class_chirps(np.arange(300) % 12, seed=77, n_samples=800))
    fm, tm = np.zeros((300, 128), dtype=bool), np.zeros((300, 5), dtype=bool)
    for i, b in enumerate((0, 150, 299)):
        fm[b, 20 + 30 * i:50 + 30 * i] = True
        tm[b, i + 1] = True
    rows, _, plain = _check(oracle_c, fe, net, sh, audio, fm, tm, oracle_clips=(0, 1, 149, 150, 298, 299))
    masked = [0, 150, 299]
    others = np.setdiff1d(np.arange(300), masked)
    assert np.array_equal(rows[others], plain[others])
    for b in masked:
        assert not np.array_equal(rows[b], plain[b]), f"clip {b}: the mask changed nothing"
    three = pipeline.step_fused(fe, net, torch.from_numpy(audio[masked]).cuda(), mask=REF.plan_of(fm[masked], tm[masked]))
    assert np.array_equal(three.cpu().numpy(), rows[masked])


# 5. refusals

def test_refusals_of_the_masked_step(oracle_c):
    """A misaligned mask pointer; each shape the plain query refuses is refused for form 1 too; the masked entry on such a
    shape gives LSM_ERR_UNSUPPORTED (-4); a form the query does not know is a bad argument."""
    import torch
    from lsm_speech_classifier_amd import _lib, frontend, pipeline
    from lsm_speech_classifier_amd.snn import _dev, _host, _select_keys
    fe, net, audio, sh = _build(oracle_c, 128, 16, 4, 160, 384)
    x = torch.from_numpy(audio).cuda()
    keys, key_ids = _select_keys(None)
    on, off = frontend.threshold_tables(fe.thresholds, fe.gap, np.float64)
    ws = fe.new_workspace(3)
    out = torch.zeros((3, len(keys) * net.num_output_neurons), dtype=torch.float32, device="cuda")
    words = torch.zeros(64, dtype=torch.int32, device="cuda")

    def rc(f, n, freq, time):
        return fe.lib.lsm_step_fused_masked_f64(
            n._handle, _dev(x), 3, f.n_samples, _dev(f.coefs), f.n_filters, f.nwin, f.hop, f.ncols, f.time_bins, _host(on),
            _host(off), len(on), f.redundancy, _dev(ws), ws.numel() * 8, f.coef_flags, _host(key_ids), len(keys), _dev(out),
            None, freq, time, fe._stream())

    assert rc(fe, net, words.data_ptr(), words.data_ptr() + 64) == 0
    for freq, time in ((words.data_ptr() + 2, None), (None, words.data_ptr() + 1)):
        assert rc(fe, net, freq, time) == -1                                     # LSM_ERR_ARG
        assert "freq_mask and time_mask must be 4-byte aligned" in fe.lib.lsm_last_error().decode()
    torch.cuda.synchronize()

    def query(f, n, form):
        return fe.lib.lsm_step_fused_form_supported(n._handle, 3, f.n_filters, f.nwin, f.hop, f.time_bins, len(f.thresholds),
                                                    f.redundancy, f.coef_flags, form)

    assert query(fe, net, 0) == 1 and query(fe, net, 1) == 1 and query(fe, net, 3) < 0 and query(fe, net, -1) < 0
    f200 = frontend.SpikeFrontEnd(128, "gammatone", thresholds=fe.thresholds, time_bins=16, n_samples=16 * 200)   # 2 windows
    f96 = frontend.SpikeFrontEnd(96, "gammatone", thresholds=fe.thresholds, time_bins=16, n_samples=2560)        # 3 groups
    net1025 = REF.reservoir(oracle_c, 128, 16, 4, 160, 1025)                                                      # 8 waves
    from lsm_speech_classifier_amd import snn
    net1025 = snn.SNN(None, reservoir=net1025)
    slow = frontend.SpikeFrontEnd(128, "gammatone", thresholds=fe.thresholds, time_bins=16, n_samples=2560)
    slow.coef_flags = 0                                                                                           # not the fast path
    for why, f, n in (("2 live windows", f200, net), ("96 filters", f96, net), ("8 waves per clip", fe, net1025),
                      ("coef_flags 0", slow, net)):
        assert query(f, n, 0) == 0 and query(f, n, 1) == 0, why
        assert not pipeline.step_fused_supported(f, n, 3, "masked"), why
    xs = torch.zeros((3, f200.n_samples), dtype=torch.float32, device="cuda")
    plan = frontend.mask_plan(3, 128, 16, freq_masks=1, freq_width=8)
    with pytest.raises(_lib.LsmHipError, match=r"\(-4\).*lsm_step_fused_masked_f64: shape not served.*make the two launches"):
        pipeline.step_fused(f200, net, xs, mask=plan)
    with pytest.raises(_lib.LsmHipError, match=r"lsm_step_fused_masked_f64 failed \(-4\)"):      # the reservoir half's own words
        pipeline.step_fused(fe, net1025, x, mask=plan)
