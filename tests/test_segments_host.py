"""Segments and windows (SPEC.md 4b): what can be checked without a GPU -- the two exports and their ctypes signatures,
the window count, a NumPy restatement of "segment records -> merge fold -> feature_value" against the oracle's
`feature_row` on slices of one oracle spike matrix, and the `--time-segments` flag of the scripts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_KEYS = ['spike_counts', 'spike_variances', 'mean_spike_times', 'first_spike_times',
            'last_spike_times', 'mean_isi', 'isi_variances', 'burst_counts']
NEW_EXPORTS = {"lsm_reservoir_run_segments": 19, "lsm_segment_features": 11}
M32 = 0xFFFFFFFF


def test_the_header_declares_the_exports_and_the_signatures_match():
    from lsm_speech_classifier_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|long)\s+(lsm_[a-z0-9_]+)\s*\(", header, re.M))
    for name, n_params in NEW_EXPORTS.items():
        assert name in declared, f"{name} is not declared in include/lsm_hip.h"
        assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS, f"{name} has no ctypes signature"
        proto = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGS[name][1]) == n_params, name
        assert _lib._SIGS[name][0] is _lib.c_int
    # the unsegmented launch keeps its signature
    proto = re.search(r"int lsm_reservoir_run_from\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["lsm_reservoir_run_from"][1]) == 17


def _windows(G, K, H):
    return (G - K) // H + 1


def test_window_count_and_shapes():
    from lsm_speech_classifier_amd import _lib, snn
    net = snn.SNN                              # a static method: no GPU, no handle
    for G, K, H, want in [(12, 1, 1, 12), (12, 2, 1, 11), (12, 3, 2, 5), (12, 12, 1, 1), (12, 12, 5, 1), (7, 3, 3, 2),
                          (4, 1, 4, 1), (5, 2, 4, 1), (96, 1, 1, 96)]:
        assert net.segment_windows(G, K, H) == _windows(G, K, H) == want
        starts = [w * H for w in range(want)]
        assert starts[-1] + K <= G and (want == 0 or starts[-1] + H + K > G)      # the last window fits, one more would not
    for G, K, H in [(4, 0, 1), (4, 5, 1), (4, 1, 0), (4, -1, 1), (4, 2, -3)]:
        with pytest.raises(_lib.LsmHipError):
            net.segment_windows(G, K, H)


# ---- NumPy restatement of csrc/lif_common.h: the step update of a record, the segment close, the merge, feature_value ----
def _segment_records(sm_out, S, burst_isi_max):
    """(T, n_out) spikes of the output neurons -> (G, n_out) records (n, bursts, first, last, S1, Q) the way the kernels
    keep them: accumulated on launch-local times, rebased to the segment's own times and zeroed at each segment end."""
    T, n_out = sm_out.shape
    G = T // S
    rec = np.zeros((G, n_out, 6), dtype=np.int64)
    cur = np.zeros((n_out, 6), dtype=np.int64)
    for t in range(T):
        for o in np.nonzero(sm_out[t])[0]:
            n, bursts, first, last, s1, q = cur[o]
            isi = t - last
            if n == 0:
                first = t
            else:
                q = (q + isi * isi) & M32
                bursts += 1 if isi <= burst_isi_max else 0
            cur[o] = (n + 1, bursts, first, t, (s1 + t) & M32, q)
        if (t + 1) % S == 0:
            g = t // S
            t_begin = g * S
            for o in range(n_out):
                n, bursts, first, last, s1, q = cur[o]
                if n:
                    first, last, s1 = first - t_begin, last - t_begin, (s1 - n * t_begin) & M32
                rec[g, o] = (n, bursts, first, last, s1, q)
            cur[:] = 0
    return rec


def _merge(f1, f2, t0, burst_isi_max):
    n1, b1, first1, last1, s1a, q1 = (int(x) for x in f1)
    n2, b2, first2, last2, s1b, q2 = (int(x) for x in f2)
    if n2 == 0:
        return (n1, b1, first1, last1, s1a, q1)
    first2, last2 = first2 + t0, last2 + t0
    s1 = (s1a + s1b + n2 * t0) & M32
    if n1 == 0:
        return (n2, b2, first2, last2, s1, q2)
    isi = first2 - last1
    return (n1 + n2, b1 + b2 + (1 if isi <= burst_isi_max else 0), first1, last2, s1, (q1 + q2 + isi * isi) & M32)


def _feature_value(key, rec, T):
    n, bursts, first, last, s1, q = rec
    if key == 0:
        v = float(n)
    elif key == 1:
        p = n / T
        v = p * (1.0 - p)
    elif key == 2:
        v = s1 / n if n >= 1 else 0.0
    elif key == 3:
        v = float(first) if n >= 1 else 0.0
    elif key == 4:
        v = float(last) if n >= 1 else 0.0
    elif key == 5:
        v = (last - first) / (n - 1) if n >= 2 else 0.0
    elif key == 6:
        if n >= 2:
            m = (last - first) / (n - 1)
            v = q / (n - 1) - m * m
        else:
            v = 0.0
    else:
        v = float(bursts)
    return np.float32(v)


def _window_row(rec, g0, K, S, burst_isi_max, keys):
    n_out = rec.shape[1]
    row = np.empty((len(keys), n_out), dtype=np.float32)
    for o in range(n_out):
        f = (0, 0, 0, 0, 0, 0)
        for j in range(K):
            f = _merge(f, rec[g0 + j, o], j * S, burst_isi_max)
        for kq, k in enumerate(keys):
            row[kq, o] = _feature_value(ALL_KEYS.index(k), f, K * S)
    return row.reshape(-1)


@pytest.fixture(scope="module")
def oracle_clip(oracle_c):
    """One oracle spike matrix: the first reservoir and the first raster of tests/test_gpu_state.py (N = 256, T = 96)."""
    from lsm_speech_classifier_amd import reservoir as R
    n, k, n_out, c = 256, 50, 100, 40
    res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k,
                                               mean_weight=2.0 / (k // 2), refractory_period=2), c)
    raster = (np.random.RandomState(0).random_sample((c, 96)) < 0.35).astype(np.uint8)
    whole, sm, _ = oracle_c.lif_run(res, raster, ALL_KEYS)
    return res, sm, whole


@pytest.mark.parametrize("S", [1, 8, 24])
def test_records_fold_to_the_oracles_rows_on_slices(oracle_clip, S):
    from oracle import ref_numpy
    res, sm, whole = oracle_clip
    T = sm.shape[0]
    G = T // S
    burst = int(res.burst_isi_max)
    rec = _segment_records(sm[:, res.out_idx], S, burst)
    assert rec[:, :, 0].sum() == int(sm[:, res.out_idx].sum()) > 0
    for K in sorted({1, 2, G}):
        for keys in (ALL_KEYS, ['burst_counts', 'spike_variances']):
            for w in range(_windows(G, K, 1)):
                want = ref_numpy.feature_row(sm[w * S:(w + K) * S], res.out_idx, burst, keys)
                got = _window_row(rec, w, K, S, burst, keys)
                np.testing.assert_array_equal(got, want, err_msg=f"S={S} K={K} window {w} keys {keys}")
    # K = G is the whole clip: the C oracle's own row
    np.testing.assert_array_equal(_window_row(rec, 0, G, S, burst, ALL_KEYS), whole)
    # hop 2, K = 3 where it fits
    if G >= 3:
        for w in range(_windows(G, 3, 2)):
            want = ref_numpy.feature_row(sm[2 * w * S:(2 * w + 3) * S], res.out_idx, burst, ALL_KEYS)
            np.testing.assert_array_equal(_window_row(rec, 2 * w, 3, S, burst, ALL_KEYS), want)


@pytest.mark.parametrize("script", ["extract_lsm_features.py", "main.py"])
def test_the_scripts_offer_time_segments(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--time-segments" in out.stdout, f"{script} lacks --time-segments"


def test_main_forwards_time_segments_only_when_set(monkeypatch):
    import main as pipeline
    calls = []
    monkeypatch.setattr(pipeline.subprocess, "call", lambda cmd, **kw: calls.append(list(cmd)) or 0)
    monkeypatch.delenv("LSM_SYNTHETIC_PER_CLASS", raising=False)
    pipeline.run_pipeline(128, "gammatone", "original", 0.6)
    assert [c[1:] for c in calls] == [
        [os.path.join(ROOT, "create_dataset.py"), "--n-filters", "128", "--filterbank", "gammatone"],
        [os.path.join(ROOT, "extract_lsm_features.py"), "--feature-set", "original", "--multiplier", "0.6"],
        [os.path.join(ROOT, "train_classifier.py")]]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, time_segments=1)
    assert calls[1][2:] == ["--feature-set", "original", "--multiplier", "0.6"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, time_segments=4, num_neurons=500)
    assert calls[1][2:] == ["--feature-set", "original", "--multiplier", "0.6", "--num-neurons", "500", "--time-segments", "4"]
    calls.clear()
    pipeline.run_pipeline(128, "gammatone", "original", 0.6, in_memory=True, time_segments=4)
    assert "time_segments=a.time_segments" in calls[0][2] and "'time_segments': 4" in calls[0][2]


def test_time_segments_must_divide_the_steps():
    import inspect
    import extract_lsm_features as ex
    assert ex.check_time_segments(400, 4) == 100 and ex.check_time_segments(400, 1) == 400
    for bad in (3, 0, -2, 401):
        with pytest.raises(ValueError, match="time-segments"):
            ex.check_time_segments(400, bad)
    # extract_all_features keeps the reference's four parameters (tests/test_host_logic.py pins them); its per-segment
    # twin takes the count after them, default 1; main (whose keyword-only defaults are all None = the reference's value)
    # and main_from_audio take it likewise
    assert list(inspect.signature(ex.extract_all_features).parameters) == ["lsm", "spike_data", "feature_keys", "desc"]
    params = list(inspect.signature(ex.extract_all_segment_features).parameters.values())
    assert [p.name for p in params] == ["lsm", "spike_data", "feature_keys", "desc", "time_segments"]
    assert params[4].default == 1
    assert inspect.signature(ex.main).parameters["time_segments"].default is None
    assert inspect.signature(ex.main_from_audio).parameters["time_segments"].default == 1
