"""Speed perturbation on the GPU (SPEC.md 1.12; `lsm_speed_f32`, `frontend.SpeedPerturber`, `HotPath(speed=...)`,
`features_from_audio(speed=...)`, `create_dataset(speed=...)`): byte for byte against the NumPy restatement
(tests/speed_restatement.py), nothing written outside the output, the refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_restatement as M  # noqa: E402
import reverb_restatement as RR  # noqa: E402
import speed_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xAA
GUARD = 64                                    # floats in front of and behind the output that must keep their fill
BANK = ["9/10", "11/10", "401/400", "2", "1/2"]
_CACHE = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from lsm_speech_classifier_amd import _lib
    _lib.require_gpu()
    return torch


def _noise(rows, n, seed, level=0.1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, n)) * level).astype(np.float32)


def _pcm(rows, n, seed, dtype):
    """Seeded noise as float32, or as int16 at a third of full scale."""
    x = _noise(rows, n, seed)
    return x if dtype == np.float32 else np.round(x * 32768.0 / 3.0).clip(-32768, 32767).astype(np.int16)


def _same(a, b):
    return np.ascontiguousarray(a).view(np.uint32).tobytes() == np.ascontiguousarray(b).view(np.uint32).tobytes()


def _void(p):
    return C.c_void_p(p) if p else None


def _bank(factors=BANK):
    """(tables, design rows (n, 5) int32, taps one behind the other) of a list of non-unit factors."""
    from lsm_speech_classifier_amd import frontend
    key = tuple(factors)
    if key not in _CACHE:
        tables = [frontend.speed_design(f) for f in factors]
        offsets = np.cumsum([0] + [len(t.taps) for t in tables])
        designs = np.ascontiguousarray([[t.up, t.down, len(t.taps), t.delay, int(o)] for t, o in zip(tables, offsets)],
                                       dtype=np.int32)
        _CACHE[key] = (tables, designs, np.concatenate([t.taps for t in tables]))
    return _CACHE[key]


def _abi(torch, audio, designs, taps, rows, n_out):
    """`lsm_speed_f32` into the middle of a buffer of 0xAA bytes -> (B, n_out) float32; what lies around stays 0xAA."""
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    B, n_in = audio.shape
    a, t = torch.from_numpy(audio).cuda(), torch.from_numpy(taps).cuda()
    rw = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda()
    buf = torch.full(((B * n_out + 2 * GUARD) * 4,), FILL, dtype=torch.uint8, device="cuda")
    rc = lib.lsm_speed_f32(_void(a.data_ptr()), 1 if audio.dtype == np.int16 else 0, B, n_in, _void(t.data_ptr()), len(taps),
                           C.c_void_p(designs.ctypes.data), len(designs), None if rw is None else _void(rw.data_ptr()),
                           n_out, _void(buf.data_ptr() + 4 * GUARD), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.lsm_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:4 * GUARD] == FILL).all() and (got[4 * (GUARD + B * n_out):] == FILL).all(), "written outside out"
    return got[4 * GUARD:4 * (GUARD + B * n_out)].view(np.float32).reshape(B, n_out)


# ---- the kernel against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["float32", "int16"])
def test_every_path_of_the_kernel_equals_the_restatement_byte_for_byte(torch_cuda, dtype):
    """Two full tiles and one of 4 outputs per clip; a table over 64 KB (401/400), whole tiles of zeros (2), a clip cut
    at n_out (1/2), an unperturbed clip, a clamped row."""
    tables, designs, taps = _bank()
    from lsm_speech_classifier_amd import _lib
    lds = int(_lib.load().lsm_speed_lds_bytes(C.c_void_p(designs.ctypes.data), len(designs)))
    assert 65536 < lds <= 160 * 1024
    n_in, n_out = 2500, 4100
    rows = [0, 1, 2, -1, 3, 99, 4]
    audio = _pcm(7, n_in, 11, dtype)
    if dtype == np.float32:
        audio[3, 5] = np.float32(-0.0)
        audio[3].view(np.uint32)[9] = 0x7FC12345                      # a NaN with a payload, in the unperturbed clip
    assert SR.zero_from(n_in, tables[3]) <= 2048 and -(-n_in * tables[4].up // tables[4].down) > n_out
    want = SR.perturb_batch(audio, tables, rows, n_out)
    got = _abi(torch_cuda, audio, designs, taps, rows, n_out)
    for c, r in enumerate(rows):
        assert _same(got[c], want[c]), f"clip {c} (row {r}): max |diff| = {np.nanmax(np.abs(got[c] - want[c])):.3e}"
    assert want[[0, 1, 2, 4, 5, 6]].any(axis=1).all()
    assert not got[4, 2048:].view(np.uint32).any()                    # factor 2: the last two tiles are +0.0
    assert _same(got[5], SR.perturb(audio[5], tables[4], n_out))      # row 99 is the bank's last
    widened = audio[3].astype(np.float32) * np.float32(2.0 ** -15) if dtype == np.int16 else audio[3]
    assert _same(got[3, :n_in], widened) and not got[3, n_in:].view(np.uint32).any()


def test_no_rows_means_row_0_and_a_smaller_n_out_is_a_prefix(torch_cuda):
    tables, designs, taps = _bank()
    audio = _noise(3, 2500, 12)
    full = _abi(torch_cuda, audio, designs, taps, None, 4100)
    assert _same(full, SR.perturb_batch(audio, tables, None, 4100)) and _same(full, _abi(torch_cuda, audio, designs, taps, [0] * 3, 4100))
    for n_out in (1, 513, 2048, 2049):
        assert _same(_abi(torch_cuda, audio, designs, taps, None, n_out), full[:, :n_out]), n_out
    # a bank of one design, the same clips
    _, one, one_taps = _bank(["9/10"])
    assert _same(_abi(torch_cuda, audio, one, one_taps, None, 4100), full)


def test_one_clip_of_one_sample(torch_cuda):
    tables, designs, taps = _bank()
    for row in (0, 1, 2, 3, 4, -1):
        for x in (np.array([[0.5]], dtype=np.float32), np.array([[-12345]], dtype=np.int16)):
            got = _abi(torch_cuda, x, designs, taps, [row], 1)
            assert _same(got, SR.perturb_batch(x, tables, [row], 1)) and got[0, 0] != 0, row


def test_a_nan_sample_stays_under_its_taps_and_in_its_clip(torch_cuda):
    tables, designs, taps = _bank(["11/10", "9/10"])
    n_in, n_out, j = 2500, 2500, 2060
    audio = _noise(3, n_in, 13)
    rows = [0, 0, 1]
    clean = _abi(torch_cuda, audio, designs, taps, rows, n_out)
    audio[1, j] = np.nan
    got = _abi(torch_cuda, audio, designs, taps, rows, n_out)
    assert _same(got, SR.perturb_batch(audio, tables, rows, n_out))
    assert _same(got[0], clean[0]) and _same(got[2], clean[2]) and np.isfinite(got[[0, 2]]).all()
    # the outputs whose taps cover sample j: y[m] reads x[i0 - t] for t < the taps of phase k0 (a zero tap covers it too)
    t = tables[0]
    p = (np.arange(n_out, dtype=np.int64) + t.delay) * t.down
    k0, i0 = p % t.up, p // t.up
    covered = (i0 >= j) & (i0 - j < (len(t.taps) - k0 + t.up - 1) // t.up)
    assert 0 < covered.sum() < 40 and np.array_equal(np.isnan(got[1]), covered)


def _by_design(x, tables, rows, n_out):
    """`SR.perturb_batch` for many short clips: the same sums in the same order, over all the clips of a design at once."""
    out = np.zeros((len(x), n_out), dtype=np.float32)
    n_in = x.shape[1]
    for r in sorted(set(rows.tolist())):
        sel = rows == r
        if r < 0:
            out[sel, :min(n_in, n_out)] = x[sel, :n_out]
            continue
        t = tables[min(r, len(tables) - 1)]
        taps, K, x64 = np.asarray(t.taps, dtype=np.float64), len(t.taps), x[sel].astype(np.float64)
        for m in range(n_out):
            p = (m + t.delay) * t.down
            i, acc = p // t.up, np.zeros(int(sel.sum()), dtype=np.float64)
            for k in range(p % t.up, K, t.up):
                acc = acc + taps[k] * (x64[:, i] if 0 <= i < n_in else 0.0)
                i -= 1
            out[sel, m] = acc.astype(np.float32)
    return out


def test_a_batch_over_65535_clips_is_cut_into_launches(torch_cuda):
    from lsm_speech_classifier_amd import frontend
    B, n = 65536 + 3, 4
    sp = frontend.SpeedPerturber(["0.9", 1, "1.1"])
    assert sp.row_of_choice.tolist() == [0, -1, 1] and sp.designs.shape == (2, 5) and sp.lds_bytes == 2000
    audio = _noise(B, n, 14)
    choice = (np.arange(B) % 4 - 1).astype(np.int32)                  # unperturbed, 0.9, 1 (unperturbed too), 1.1 in turn
    rows = np.where(choice < 0, -1, sp.row_of_choice[np.maximum(choice, 0)])
    got = sp.perturb(audio, choice).cpu().numpy()
    want = _by_design(audio, sp.tables, rows, n)
    assert _same(want[:9], SR.perturb_batch(audio[:9], sp.tables, rows[:9], n)) and _same(want[-9:], SR.perturb_batch(audio[-9:], sp.tables, rows[-9:], n))
    assert got.shape == (B, n) and _same(got, want)


def test_the_perturber_checks_its_arguments(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import frontend
    sp = frontend.SpeedPerturber(["1.0", "1.1"])
    audio = _noise(3, 300, 15)
    # no choice: factor 0 everywhere, here the unit factor
    assert _same(sp.perturb(audio).cpu().numpy(), audio)
    out = torch.empty((3, 310), dtype=torch.float32, device="cuda")
    assert sp.perturb(audio, [1, -1, 0], n_out=310, out=out) is out
    assert _same(out.cpu().numpy(), SR.perturb_batch(audio, sp.tables, [0, -1, -1], 310))
    assert _same(sp.perturb(np.round(audio * 8000).astype(np.int16), 1).cpu().numpy(),
                 SR.perturb_batch(np.round(audio * 8000).astype(np.int16), sp.tables, [0] * 3, 300))
    dev = torch.from_numpy(audio).cuda()
    for bad in (dict(choice=[0, 1]), dict(choice=2), dict(choice=[0.5] * 3), dict(n_out=0), dict(out=out)):
        with pytest.raises(ValueError):
            sp.perturb(dev, **bad)
    with pytest.raises(ValueError, match="out must not be audio"):
        sp.perturb(dev, out=dev)
    with pytest.raises(ValueError):
        sp.perturb(audio.astype(np.float64))


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_abi_refusals(torch_cuda):
    torch = torch_cuda
    from lsm_speech_classifier_amd import _lib
    lib = _lib.load()
    _, designs, taps = _bank(["9/10", "11/10"])
    B, n = 3, 40
    audio = torch.zeros((B, n + 4), dtype=torch.float32, device="cuda")
    out = torch.full((B, n + 4), -7.0, dtype=torch.float32, device="cuda")
    ints = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(np.concatenate([taps, np.zeros(1)])).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def call(a=audio.data_ptr(), fmt=0, B=B, n=n, t=t.data_ptr(), total=len(taps), d=designs, nd=None, row=ints.data_ptr(),
             n_out=n, o=out.data_ptr()):
        d = None if d is None else np.ascontiguousarray(d, dtype=np.int32)
        nd = (0 if d is None else len(d)) if nd is None else nd
        return lib.lsm_speed_f32(_void(a), fmt, B, n, _void(t), total, None if d is None else C.c_void_p(d.ctypes.data), nd,
                                 _void(row), n_out, _void(o), stream)

    def design(**change):
        d = designs.copy()
        for name, v in change.items():
            d[1, ["up", "down", "n_taps", "delay", "tap_offset"].index(name)] = v
        return d

    cases = [
        (lambda: call(d=design(up=11)), "design 1 .*up == down"), (lambda: call(d=design(up=22)), "design 1 .*share a factor"),
        (lambda: call(d=design(up=0)), "design 1 .*must be >= 1"), (lambda: call(d=design(down=-11)), "design 1 .*must be >= 1"),
        (lambda: call(d=design(n_taps=0)), "design 1 .*n_taps must be >= 1"),
        (lambda: call(d=design(delay=22)), "design 1 .*delay does not fit"), (lambda: call(d=design(delay=-1)), "delay does not fit"),
        (lambda: call(d=design(tap_offset=-1)), "design 1 .*tap_offset must be >= 0"),
        (lambda: call(d=design(tap_offset=210)), "design 1: tap_offset=210 \\+ n_taps=232 runs past"),
        (lambda: call(total=len(taps) - 1), "runs past the n_taps_total"), (lambda: call(total=0), "n_taps_total=0"),
        (lambda: call(nd=0), "n_designs=0 outside \\[1, 16\\]"), (lambda: call(d=np.tile(designs[:1], (17, 1))), "n_designs=17 outside"),
        (lambda: call(d=None, nd=1), "designs is required"),
        (lambda: call(fmt=2), "sample_format=2"), (lambda: call(fmt=-1), "sample_format=-1"),
        (lambda: call(a=0), "null buffer"), (lambda: call(t=0), "null buffer"), (lambda: call(o=0), "out is required"),
        (lambda: call(a=audio.data_ptr() + 2), "audio is misaligned: it must be 4-byte"),
        (lambda: call(a=audio.data_ptr() + 1, fmt=1), "audio is misaligned: it must be 2-byte"),
        (lambda: call(t=t.data_ptr() + 4), "taps_dev is misaligned"), (lambda: call(o=out.data_ptr() + 2), "out is misaligned"),
        (lambda: call(row=ints.data_ptr() + 2), "design_row is misaligned"),
        (lambda: call(o=audio.data_ptr()), "out must not be audio"),
        (lambda: call(B=0), "n_clips=0 outside \\[1, 65535\\]"), (lambda: call(B=65536), "n_clips=65536 outside"),
        (lambda: call(n=0), "n_in=0"), (lambda: call(n_out=0), "n_out=0"), (lambda: call(n_out=-5), "n_out=-5"),
    ]
    for i, (refused, words) in enumerate(cases):
        rc = refused()
        assert rc == -1, f"refusal {i} ({words}): returned {rc}"
        assert re.search(words, lib.lsm_last_error().decode()), f"refusal {i} ({words}): {lib.lsm_last_error().decode()!r}"
    # a table over a compute unit's LDS: another code
    big = np.array([[1000, 1001, 21022, 10, 0]], dtype=np.int32)
    assert call(d=big, total=21022) == -4 and re.search("184000 bytes", lib.lsm_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote"
    # the call the refusals start from, with and without rows, and int16 at a 2-byte boundary
    assert call() == 0 and call(row=0) == 0 and call(a=audio.data_ptr() + 2, fmt=1) == 0
    torch.cuda.synchronize()
    flat = out.view(-1)                                               # the calls take out as (B, n): its first B * n samples
    assert bool((flat[:B * n] == 0).all()) and bool((flat[B * n:] == -7.0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------
KEYS = ['spike_counts', 'mean_spike_times', 'mean_isi']
FACTORS = ["0.9", "1.0", "1.1"]


def _small_net(F):
    from lsm_speech_classifier_amd import reservoir as Rv, snn
    res = Rv.build_reservoir(Rv.SimulationParams(num_neurons=64, num_output_neurons=32, small_world_graph_k=8,
                                                 mean_weight=2.0 / 4, refractory_period=2), F)
    return snn.SNN(None, reservoir=res)


def _clips():
    """Five synthetic clips, a plan over FACTORS that names every choice, and the restatement's perturbed clips."""
    from lsm_speech_classifier_amd import frontend, synth
    if "clips" not in _CACHE:
        n = 5
        audio = synth.class_chirps(np.arange(n), seed=3)
        paces = frontend.speed_plan(n, 3, prob=0.8, seed=8)
        tables, row_of_choice = frontend.speed_bank(FACTORS)
        rows = np.where(paces.choice < 0, -1, row_of_choice[np.maximum(paces.choice, 0)])
        _CACHE["clips"] = (audio, paces, SR.perturb_batch(audio, tables, rows, audio.shape[1]))
    return _CACHE["clips"]


@pytest.mark.parametrize("filterbank,F", [("gammatone", 8), ("mel", 16)])
def test_features_from_perturbed_audio_equal_those_of_the_restatement(torch_cuda, filterbank, F):
    from lsm_speech_classifier_amd import frontend, pipeline
    audio, paces, fast = _clips()
    n = len(audio)
    assert set(paces.choice.tolist()) == {-1, 0, 1, 2}
    sp = frontend.SpeedPerturber(FACTORS)
    fe, net = frontend.SpikeFrontEnd(F, filterbank), _small_net(F)
    # the whole chain on the restatements, in the recipe's order: speed, reverberation, mix
    bank = (np.random.default_rng(61).standard_normal((3, 400)) * 0.3 * np.exp(-np.arange(400) / 80.0)[None, :]).astype(np.float32)
    bank[:, 0] = 1.0
    lengths = np.array([400, 150, 9], dtype=np.int32)
    rv = frontend.Reverberator(bank, lengths)
    rooms = frontend.reverb_plan(n, 3, prob=0.8, seed=3)
    noise = _noise(3, 4097, 62, 0.05)
    mixer = frontend.NoiseMixer(noise)
    plan = frontend.mix_plan(n, 3, 4097, (0.0, 20.0), max_shift=1600, level_db=(-6.0, 0.0), seed=9)
    wet = RR.reverb(fast, bank, lengths, rooms.rows)
    chain, _, _ = M.mix(wet, noise, 10.0 ** (-plan.snr_db / 10.0), plan.rows, plan.offsets, plan.shift, plan.scale)
    hp = pipeline.HotPath(fe, net, KEYS, streams=1, speed=sp, reverb=rv, mixer=mixer)
    plain = pipeline.HotPath(fe, net, KEYS, streams=1)

    def rows_of(pipe, x, **plans):
        feats, st = pipe.submit(x, **plans)
        st.synchronize()
        return feats.cpu().numpy().tobytes()

    clean = rows_of(plain, audio)
    assert rows_of(hp, audio, speed=paces) == rows_of(plain, fast) != clean
    assert rows_of(hp, audio, speed=paces, reverb=rooms, mix=plan) == rows_of(plain, chain) != rows_of(plain, fast)
    assert rows_of(hp, audio) == clean
    with pytest.raises(ValueError, match="speed perturber"):
        plain.submit(audio, speed=paces)
    for streams in (1, pipeline.DEFAULT_STREAMS):                   # the serial path and the two-stage topology
        got = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, speed=(sp, paces))
        want = pipeline.features_from_audio(fast, fe, net, KEYS, batch=2, streams=streams)
        assert got.shape == want.shape == (n, len(KEYS) * 32) and want.any() and got.tobytes() == want.tobytes()
        got = pipeline.features_from_audio(audio, fe, net, KEYS, batch=2, streams=streams, speed=(sp, paces),
                                           reverb=(rv, rooms), corrupt=(mixer, plan))
        assert got.tobytes() == pipeline.features_from_audio(chain, fe, net, KEYS, batch=2, streams=streams).tobytes()
    with pytest.raises(ValueError, match="speed plan covers"):
        pipeline.features_from_audio(audio, fe, net, KEYS, speed=(sp, paces.part(0, 2)))


def test_create_dataset_with_the_speed_flags(torch_cuda, tmp_path):
    """File 1 written with `speed` holds the rasters of the restated clips; without it, the bytes of a run that never
    passes the argument."""
    from scipy.io import wavfile
    import create_dataset as cd
    from lsm_speech_classifier_amd import frontend
    words = ["a", "b", "c"]
    rng = np.random.default_rng(21)
    clips = []
    for w in words:
        os.makedirs(tmp_path / "corpus" / w)
        for k in range(2):
            t = np.arange(16000) / 16000.0
            x = 0.4 * np.sin(2 * np.pi * (300 + 400 * len(clips)) * t * (1 + 0.5 * t)) + 0.02 * rng.standard_normal(16000)
            pcm = np.round(x * 20000).astype(np.int16)
            wavfile.write(str(tmp_path / "corpus" / w / f"{k}.wav"), 16000, pcm)
            clips.append(pcm)
    fast_file, none_file, plain_file = (str(tmp_path / f"{k}.npz") for k in ("fast", "none", "plain"))
    pace = dict(factors=["0.9", "1.0", "1.1"], prob=0.8, seed=2)
    common = dict(commands=words, dataset_root=str(tmp_path / "corpus"))
    cd.create_dataset(8, "gammatone", output_file=fast_file, speed=pace, **common)
    cd.create_dataset(8, "gammatone", output_file=none_file, speed=None, **common)
    cd.create_dataset(8, "gammatone", output_file=plain_file, **common)
    assert open(none_file, "rb").read() == open(plain_file, "rb").read()
    factors, paces = cd.speeds(pace, 6)
    assert set(paces.choice.tolist()) == {-1, 0, 1, 2}
    loaded, labels = cd._load_listing(cd._list_files(words, tmp_path / "corpus", cd.MAX_SAMPLES_PER_CLASS))
    audio = np.stack(loaded).astype(np.float32)
    assert labels == [0, 0, 1, 1, 2, 2] and audio.shape == (6, 16000)
    tables, row_of_choice = frontend.speed_bank(factors)
    rows = np.where(paces.choice < 0, -1, row_of_choice[np.maximum(paces.choice, 0)])
    fast = SR.perturb_batch(audio, tables, rows, 16000)
    fe = frontend.SpikeFrontEnd(8, "gammatone")
    got, plain = np.load(fast_file)["X_spikes"], np.load(plain_file)["X_spikes"]
    assert got.tobytes() == fe.encode(fast).cpu().numpy().tobytes()
    assert plain.tobytes() == fe.encode(audio).cpu().numpy().tobytes() and got.tobytes() != plain.tobytes()
