"""The spike encoder -- dB -> normalise -> resize -> hysteresis latch -> raster (SPEC.md 1.2-1.4) -- over the range its C
ABI accepts, in its three device implementations: `lsm_spec_to_spikes_f64/_f32` with the finishing workgroup of
`lsm_mel_spikes_f32` (csrc/spikes_body.h), the epilogue of `lsm_gammatone_spikes_f64` in its three layouts
(csrc/frontend.hip), and `lsm_encode_hysteresis_f32/_f64`.

Expected values never come from another device route: the normalised spectrogram is the C oracle's (held against
scipy.ndimage.zoom itself by tests/test_encoder_host.py, the widths whose last bin SciPy answers with 0.0 included), the
raster is the reference's latch loop restated in tests/encoder_restatement.py.  Given the dB array everything downstream is
IEEE arithmetic with contraction off, so normalised values and rasters are compared BYTE FOR BYTE, in float32 too; that the
routes agree with each other is asserted in addition."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_restatement as ER  # noqa: E402

pytestmark = pytest.mark.gpu

THR8 = [0.3, 0.6, 0.65, 0.7, 0.8, 0.9, 0.95, 0.99]
THR = [0.70, 0.80, 0.90, 0.95]
GAP = 0.1
GUARD = 256                          # bytes behind every output buffer that must keep their fill
LSM_ERR_ARG = -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return C.c_void_p(a.ctypes.data) if a is not None and len(a) else None


def _guarded(torch, n_bytes, fill):
    return torch.full((n_bytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


def _same_bits(got, want, what=""):
    """Equal byte for byte; a NaN equals any NaN (the payload of a NaN is not the reference's to define)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {tuple(np.argwhere(bad)[0])}"


def _spec_to_spikes(torch, db, time_bins, on, off, floor=1, red=1):
    """`lsm_spec_to_spikes_*` on (B, F, ncols) dB values -> (rc, norm (B, F, time_bins), raster or None); the outputs lie
    in front of guard bytes, which must survive, and start filled with 0xA5 so that a byte nobody wrote shows."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    B, F, nc = db.shape
    dt = db.dtype
    nq = len(on)
    dev = torch.from_numpy(np.ascontiguousarray(db)).cuda()
    n_norm, n_ras = B * F * time_bins * dt.itemsize, B * F * red * time_bins * nq
    norm_buf = _guarded(torch, n_norm, 0xA5)
    ras_buf = _guarded(torch, n_ras, 0xA5) if nq else None
    fn = lib.lsm_spec_to_spikes_f64 if dt == np.float64 else lib.lsm_spec_to_spikes_f32
    on = np.ascontiguousarray(on, dtype=dt)
    off = np.ascontiguousarray(off, dtype=dt)
    rc = fn(_p(dev), B, F, nc, time_bins, floor, _h(on), _h(off), nq, red, _p(ras_buf), _p(norm_buf),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    nb, rb = norm_buf.cpu().numpy(), (ras_buf.cpu().numpy() if nq else None)
    assert (nb[n_norm:] == 0xA5).all() and (rb is None or (rb[n_ras:] == 0xA5).all()), "bytes behind an output were written"
    norm = nb[:n_norm].view(dt).reshape(B, F, time_bins)
    raster = rb[:n_ras].reshape(B, F * red, time_bins * nq) if nq else None
    return rc, norm, raster


def _check_split(torch, oracle_c, db, time_bins, on, off, floor=1, red=1):
    """The split route on `db` against the definition, every clip; returns (expected norms, expected rasters)."""
    on = np.asarray(on, dtype=db.dtype)
    off = np.asarray(off, dtype=db.dtype)
    rc, norm, raster = _spec_to_spikes(torch, db, time_bins, on, off, floor, red)
    assert rc == 0
    norms, rasters = [], []
    for b in range(db.shape[0]):
        n_ref, r_ref = ER.expected(oracle_c, db[b], time_bins, on, off, bool(floor), red)
        _same_bits(norm[b], n_ref, f"clip {b} norm_out")
        if len(on):
            assert raster[b].max() <= 1, f"clip {b}: raster bytes other than 0 / 1"
            assert np.array_equal(raster[b], r_ref), f"clip {b}: {int((raster[b] != r_ref).sum())} raster bytes differ"
        norms.append(n_ref)
        rasters.append(r_ref)
    return np.stack(norms), (np.stack(rasters) if len(on) else None)


def _bins(raster, time_bins):
    """(..., C, time_bins * n_thr) -> (..., C, time_bins, n_thr)."""
    return raster.reshape(raster.shape[:-1] + (time_bins, raster.shape[-1] // time_bins))


# ---- 1. widths whose last bin lies outside the input: every route --------------------------------------------------------

OVERSHOOT = [(105, 100), (58, 100), (30, 8), (8, 26), (32, 31)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("ncols,time_bins", OVERSHOOT)
def test_overshooting_widths_split_route(torch_cuda, oracle_c, ncols, time_bins, dt):
    """Latches that are on in the last bin but one are released in the last: SciPy answers 0.0 for a coordinate outside the
    input (SPEC.md 1.2).  70 filters: two row groups; clip 1 holds a NaN -- NaN everywhere, and still +0.0 in the last bin."""
    assert ER.overshoots(ncols, time_bins)
    db = ER.plateau_db(ncols * time_bins, 3, 70, ncols, dt)
    db[1, 5, ncols // 2] = np.nan
    on, off = ER.tables(THR, GAP, dt)
    for red in (1, 2):
        norm, raster = _check_split(torch_cuda, oracle_c, db, time_bins, on, off, 1, red)
    for b in (0, 2):
        r = _bins(raster[b], time_bins)
        assert r[:, time_bins - 2].any(), "no latch is on in the last bin but one: the case tests nothing"
        assert not r[:, time_bins - 1].any()
        assert not norm[b][:, time_bins - 1].view(np.uint64 if dt == np.float64 else np.uint32).any()
    assert np.isnan(norm[1][:, :time_bins - 1]).all() and not norm[1][:, time_bins - 1].any() and not raster[1].any()


def _fe(n_filters, n_samples=16000, hop=None, ncols=None, **kw):
    """A gammatone front end with the column grid set by hand (the C ABI takes nwin / hop / ncols as they are)."""
    from lsm_speech_classifier_amd import frontend
    fe = frontend.SpikeFrontEnd(n_filters, "gammatone", n_samples=n_samples, **kw)
    if hop is not None:
        fe.hop, fe.ncols = hop, ncols
    assert (fe.ncols - 1) * fe.hop + fe.nwin <= n_samples
    return fe


def _layout(n_clips, n_filters, flags=0):
    from lsm_speech_classifier_amd import _lib
    return _lib.load().lsm_gammatone_spikes_layout(n_clips, n_filters, flags)


def _fused_layouts(torch, fe, audio, monkeypatch):
    """The one-launch route in the lane-pair, one-chain and (above 64 filters) two-chain layout, selected as
    tests/test_gpu_lane_pair.py does: {layout: raster}."""
    out = {}
    with monkeypatch.context() as m:
        m.setenv("GPU_MAX_HW_QUEUES", "4")
        assert _layout(len(audio), fe.n_filters) == 0
        out[0] = fe.encode(audio, fused=True).cpu().numpy()
        m.setenv("GPU_MAX_HW_QUEUES", "12")
        assert _layout(len(audio), fe.n_filters, 1) == 1
        out[1] = fe.encode(audio, fused=True, low_latency=True).cpu().numpy()
        if fe.n_filters > 64:
            assert _layout(len(audio), fe.n_filters) == 2
            out[2] = fe.encode(audio, fused=True).cpu().numpy()
    return out


_DB_CACHE = {}


def _oracle_db(oracle_c, audio_key, audio, fe):
    """The C oracle's floored dB spectrograms of `audio` on `fe`'s column grid, computed once per grid."""
    key = (audio_key, fe.n_filters, fe.nwin, fe.hop, fe.ncols)
    if key not in _DB_CACHE:
        coefs = fe.coefs.cpu().numpy()
        _DB_CACHE[key] = np.stack([oracle_c.gammatone_db(oracle_c.gammatone_spec(a, coefs, fe.nwin, fe.hop, fe.ncols))
                                   for a in audio])
        _DB_CACHE[key].setflags(write=False)
    return _DB_CACHE[key]


def _swelling_audio(n_samples, seed):
    """Three clips that grow louder to the end: latches are on in the last bins."""
    from lsm_speech_classifier_amd import synth
    audio = synth.class_chirps([1, 6, 10], seed=seed, n_samples=n_samples)
    audio = audio + 0.02 * synth.white_noise(3, seed=seed + 1, n_samples=n_samples)
    return np.ascontiguousarray((audio * np.linspace(0.02, 1.0, n_samples) ** 2).astype(np.float32))


def test_overshooting_width_fused_gammatone_every_layout(torch_cuda, oracle_c, monkeypatch):
    """nwin 400, hop 160, 105 columns -> 100 bins through `lsm_gammatone_spikes_f64` in its three layouts and through the
    split entry points, 96 filters (a ragged last channel group in every layout), redundancy 1 and 3."""
    audio = _swelling_audio(17040, seed=17)
    for red in (1, 3):
        fe = _fe(96, 17040, hop=160, ncols=105, redundancy=red)
        assert (fe.nwin, fe.hop, fe.ncols, fe.time_bins) == (400, 160, 105, 100) and ER.overshoots(105, 100)
        db = _oracle_db(oracle_c, "swell17040", audio, fe)
        on, off = ER.tables(THR, GAP, np.float64)
        ref = np.stack([ER.expected(oracle_c, d, 100, on, off, True, red)[1] for d in db])
        r = _bins(ref, 100)
        assert r[:, :, 98].any(axis=(1, 2)).all(), "every clip needs a latch that is on in bin 98"
        assert not r[:, :, 99].any()
        split = fe.encode(audio, fused=False).cpu().numpy()
        assert np.array_equal(split, ref), "split route"
        for layout, got in _fused_layouts(torch_cuda, fe, audio, monkeypatch).items():
            assert np.array_equal(got, ref), f"fused layout {layout}: {int((got != ref).sum())} bytes differ"
            assert np.array_equal(got, split)


def test_overshooting_width_mel_routes(torch_cuda, oracle_c):
    """The shape Python reaches it with: 2499 samples -> hop 24, 105 frames -> 100 bins, float32, the three split launches
    and the one-launch route (whose finishing workgroup runs csrc/spikes_body.h).  Expected from the device's own dB
    values: what comes before them involves an FFT (SPEC.md 1.5), what comes after is exact."""
    from lsm_speech_classifier_amd import frontend
    audio = _swelling_audio(2499, seed=23)
    fe = frontend.SpikeFrontEnd(24, "mel", n_samples=2499, time_bins=100)
    assert fe._mel.hop == 24 and fe.ncols == 105 and ER.overshoots(105, 100)
    db, _ = fe.spectrogram_db(audio)
    raster, norm = fe.spikes_from_db(db, want_norm=True)
    db, raster, norm = db.cpu().numpy(), raster.cpu().numpy(), norm.cpu().numpy()
    assert db.dtype == np.float32
    on, off = ER.tables(THR, GAP, np.float32)
    for b in range(3):
        n_ref, r_ref = ER.expected(oracle_c, db[b], 100, on, off, apply_floor=False)
        _same_bits(norm[b], n_ref, f"clip {b} norm_out")
        assert np.array_equal(raster[b], r_ref)
        r = _bins(r_ref, 100)
        assert r[:, 98].any() and not r[:, 99].any()
    assert np.array_equal(fe.encode(audio, fused=True).cpu().numpy(), raster), "one-launch route"


# ---- 2. the fused epilogue: threshold counts that do not divide 32 -------------------------------------------------------

# (n_thr, time_bins, hop, ncols): bit accumulator straddling a word (3, 5, 6, 7), byte stores (231, 250, 154 raster bytes
# per row) and word stores (700, 588, 300), the 4-bit and the 8-bit field, resize and none
EPILOGUE = [(3, 77, 200, 77), (5, 50, 300, 50), (7, 100, 160, 98), (6, 98, 160, 98), (3, 100, 160, 98), (2, 77, 208, 76),
            (5, 100, 160, 98), (7, 31, 480, 32)]


@pytest.mark.parametrize("n_filters", [33, 96])
@pytest.mark.parametrize("n_thr,time_bins,hop,ncols", EPILOGUE)
def test_fused_epilogue_threshold_counts_and_row_lengths(torch_cuda, oracle_c, monkeypatch, n_thr, time_bins, hop, ncols,
                                                         n_filters):
    from lsm_speech_classifier_amd import synth
    audio = np.concatenate([synth.class_chirps([2, 9], seed=41), synth.white_noise(1, seed=42)])
    thr, gap = THR8[8 - n_thr:], 0.05
    on, off = ER.tables(thr, gap, np.float64)
    assert ((time_bins * n_thr) % 4 == 0) == ((n_thr, time_bins) in ((7, 100), (6, 98), (3, 100), (5, 100)))
    for red in (1, 3):
        fe = _fe(n_filters, 16000, hop=hop, ncols=ncols, time_bins=time_bins, thresholds=thr, gap=gap, redundancy=red)
        db = _oracle_db(oracle_c, "chirps41", audio, fe)
        ref = np.stack([ER.expected(oracle_c, d, time_bins, on, off, True, red)[1] for d in db])
        assert ref.any(axis=(1, 2)).all() and _bins(ref, time_bins).any(axis=(0, 1, 2)).all()     # every threshold fires
        split = fe.encode(audio, fused=False).cpu().numpy()
        assert np.array_equal(split, ref), "split route"
        for layout, got in _fused_layouts(torch_cuda, fe, audio, monkeypatch).items():
            assert got.shape == ref.shape
            assert np.array_equal(got, ref), f"fused layout {layout}, redundancy {red}: {int((got != ref).sum())} bytes differ"


# ---- 3. the split kernel's shape edges ---------------------------------------------------------------------------------

def _edge_cases():
    tbs = [2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129]
    kinds = ["2", "tb-1", "tb", "tb+1", "3tb", "1000"]
    fs, nqs, reds = [1, 63, 64, 65, 129], [0, 1, 3, 8], [1, 2, 5]
    cases = []
    for i, tb in enumerate(tbs):
        for k in (0, 1):
            kind = kinds[(i + 3 * k) % 6]
            nc = {"2": 2, "tb-1": max(2, tb - 1), "tb": tb, "tb+1": tb + 1, "3tb": 3 * tb, "1000": 1000}[kind]
            cases.append((tb, nc, fs[(i + 2 * k) % 5], nqs[(i + k) % 4], reds[(i + k) % 3]))
    assert {c[0] for c in cases} == set(tbs) and {c[2] for c in cases} == set(fs)
    assert {c[3] for c in cases} == set(nqs) and {c[4] for c in cases} == set(reds)
    assert all(any((c[1] == n(c[0])) for c in cases) for n in (lambda t: 2, lambda t: t - 1, lambda t: t, lambda t: t + 1,
                                                               lambda t: 3 * t, lambda t: 1000))
    return cases


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("time_bins,ncols,n_filters,n_thr,red", _edge_cases())
def test_split_kernel_shape_edges(torch_cuda, oracle_c, time_bins, ncols, n_filters, n_thr, red, dt):
    """Rows of exactly, one less and one more than 1, 2, 3, 4 words of 32 bins (W, the second word of a 64-bin piece, the
    four-piece loop), widths from 2 columns to 1000, one row to three row groups, no threshold (norm_out alone) to eight,
    row repeat; three clips, the middle one flat where the case number is even; a negative gap where it is odd."""
    seed = time_bins * 1000 + ncols
    db = ER.walk_db(seed, 3, n_filters, ncols, dt)
    if seed % 2 == 0:
        db[1] = dt(-20.0)
    thr = THR8[:n_thr]
    on, off = ER.tables(thr, -0.07 if seed % 2 else 0.05, dt)
    floor = 0 if dt == np.float32 else 1                        # as the mel and the gammatone branch call it
    norm, raster = _check_split(torch_cuda, oracle_c, db, time_bins, on, off, floor, red)
    if seed % 2 == 0:
        assert not norm[1].any() and (raster is None or not raster[1].any())
    assert norm[0].max() > 0.5 and (raster is None or raster[0].any())          # (a resize may step over the maximum)


# ---- 4. the latch: carry from word to word, fast and slow words, values equal to a bound ---------------------------------

@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n_bins", [100, 130])
def test_latch_carry_across_words(torch_cuda, oracle_c, n_bins, dt):
    """Step rows placed bin by bin (ncols == time_bins): edges at bins 31/32, 63/64, ..., the first and the last bin, a
    latch held on across every word, a row that never crosses.  With a positive gap every word takes the adder; with a
    negative one (OFF above ON) the rows holding 0.5 take the bit loop in the words behind their edge and the adder before
    it, and the latch flips every bin there."""
    x = ER.step_rows(n_bins, dt)
    db = ER.db_of_norm(x)[None]
    nw = (n_bins - 1) // 32
    for on, off in (([0.7], [0.3]), ([0.8, 0.7, 0.6], [0.4, 0.3, 0.2]), ([0.3], [0.7]), ([0.7, 0.3], [0.3, 0.7])):
        norm, raster = _check_split(torch_cuda, oracle_c, db, n_bins, np.array(on, dtype=dt), np.array(off, dtype=dt))
        r = _bins(raster[0], n_bins)[:, :, 0]
        n = norm[0]
        assert (n[0] < 0.2).all() and (n[1] > 0.8).all() and n.min() == 0.0 and 0.45 < n[8, 40] < 0.55
        assert not r[0].any() and r[1].all()
        if on[0] > off[0]:
            assert r[4, :32].all() and not r[4, 32:].any() and not r[5, :32].any() and r[5, 32:].all()
            assert r[6, 31] and r[6].sum() == 1 and r[7, 32] and r[7].sum() == 1
            for w in range(nw):                                   # on at bin 32 (w + 1) - 1, held by 0.5 to the end
                row = r[8 + 5 * w]
                assert not row[:32 * (w + 1) - 1].any() and row[32 * (w + 1) - 1:].all()
        else:
            assert np.array_equal(r[8, 30:38], [0, 1, 0, 1, 0, 1, 0, 1])


def _bounds_from_values(norm):
    """(on, off) of two thresholds whose bounds are values of `norm` placed where equality decides: ON = a value that
    exceeds everything before it in its row (a strict comparison leaves the latch off in that bin, `>=` would set it); OFF =
    the first value below ON after the latch has been set (strict: the latch holds in that bin, `<=` would release it)."""
    on, off = [], []
    for row in norm:
        records = [j for j in range(1, len(row)) if row[j] > row[:j].max()]
        for j_on in records[len(records) // 3:]:
            later = np.nonzero(row[j_on + 1:] > row[j_on])[0]
            if not len(later):
                continue
            j_set = j_on + 1 + later[0]
            below = np.nonzero(row[j_set + 1:] < row[j_on])[0]
            if len(below):
                on.append(row[j_on])
                off.append(row[j_set + 1 + below[0]])
                break
        if len(on) == 2:
            break
    assert len(on) == 2, "no row of the clip rises, rises again and falls"
    return np.array(on, dtype=norm.dtype), np.array(off, dtype=norm.dtype)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("ncols,time_bins", [(64, 64), (98, 100), (105, 100)])
def test_values_equal_to_a_bound_do_not_cross_it(torch_cuda, oracle_c, ncols, time_bins, dt):
    """The comparisons are strict.  ON and OFF bounds are taken from the definition's own normalised values, so bins whose
    value EQUALS a bound exist (asserted), in places where a non-strict comparison changes the raster (asserted); also
    after a resize, whose values the device forms bit for bit."""
    db = ER.walk_db(7 * ncols + time_bins, 2, 5, ncols, dt)
    norm = np.stack([ER.expected(oracle_c, d, time_bins, [], [])[0] for d in db])
    on, off = _bounds_from_values(norm[0])
    assert (on > off).all() and (norm[0][:, :, None] == on).any(axis=(0, 1)).all() and \
        (norm[0][:, :, None] == off).any(axis=(0, 1)).all()
    _check_split(torch_cuda, oracle_c, db, time_bins, on, off)
    want = ER.latch_loop(norm[0], on, off)
    for loose_on, loose_off in ((True, False), (False, True)):
        act = np.zeros((5, 2), dtype=bool)
        got = np.zeros((5, time_bins, 2), dtype=np.uint8)
        for j in range(time_bins):
            v = norm[0][:, j, None]
            act = np.where(act, ~((v <= off) if loose_off else (v < off)), (v >= on) if loose_on else (v > on))
            got[:, j] = act
        assert (got.reshape(want.shape) != want).sum() >= 2, "a non-strict comparison would go unnoticed"


# ---- 5. LDS edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("time_bins,lds", [(1000, 131200), (1248, 159872)])
def test_big_lds_rows_are_exact(torch_cuda, oracle_c, time_bins, lds):
    """8 thresholds x 1000 bins: above 64 KB, the opt-in path; x 1248 bins: 159 872 bytes, the last size that fits."""
    assert 128 + 2 * 64 * 8 * ((time_bins + 31) // 32) * 4 == lds and 64 * 1024 < lds <= 160 * 1024
    db = ER.walk_db(time_bins, 2, 70, 300, np.float64)
    on, off = ER.tables(THR8, 0.05, np.float64)
    _, raster = _check_split(torch_cuda, oracle_c, db, time_bins, on, off)
    assert _bins(raster, time_bins).any(axis=(0, 1, 2)).all()


def test_rows_past_the_lds_are_refused_before_any_launch(torch_cuda):
    from lsm_speech_classifier_amd import _lib
    db = ER.walk_db(1249, 1, 3, 300, np.float64)
    on, off = ER.tables(THR8, 0.05, np.float64)
    assert 128 + 2 * 64 * 8 * ((1249 + 31) // 32) * 4 > 160 * 1024
    rc, norm, raster = _spec_to_spikes(torch_cuda, db, 1249, on, off)
    assert rc == LSM_ERR_ARG and b"LDS" in _lib.load().lsm_last_error()
    assert (raster == 0xA5).all() and (norm.view(np.uint8) == 0xA5).all()       # nothing ran
    rc, _, _ = _spec_to_spikes(torch_cuda, db, 1249, on[:7], off[:7])          # 7 x 40 words fit
    assert rc == 0


# ---- 6. lsm_encode_hysteresis_f32/_f64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_encode_hysteresis_against_the_latch_definition(torch_cuda, n_rows, dt):
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    fn = lib.lsm_encode_hysteresis_f64 if dt == np.float64 else lib.lsm_encode_hysteresis_f32
    rng = np.random.default_rng(n_rows)
    for n_bins in (1, 33, 100):
        for n_thr, gap in ((1, 0.1), (2, -0.15), (3, 0.0), (4, 0.1), (5, 0.05), (6, -0.05), (7, 0.02), (8, 0.1)):
            x = rng.random((n_rows, n_bins)).astype(dt)
            on, off = ER.tables(THR8[:n_thr], gap, dt)
            x[0, ::2] = on[0]                                     # equal to a bound: no crossing
            x[-1, ::3] = off[-1]
            dev = torch_cuda.from_numpy(x).cuda()
            n_out = n_rows * n_bins * n_thr
            out = _guarded(torch_cuda, n_out, 0xA5)
            rc = fn(_p(dev), n_rows, n_bins, _h(on), _h(off), n_thr, _p(out), torch_cuda.cuda.current_stream().cuda_stream)
            torch_cuda.cuda.synchronize()
            assert rc == 0
            got = out.cpu().numpy()
            assert (got[n_out:] == 0xA5).all()
            want = ER.latch_loop(x, on, off)
            assert np.array_equal(got[:n_out].reshape(want.shape), want), (n_bins, n_thr, gap)
