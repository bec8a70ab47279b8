"""Label new audio with a saved model: ``python classify.py --model PATH FILE.wav ...``

The model file (``main.py --save-model``, ``lsm_speech_classifier_amd.readout.LinearModel``) holds the scaler, the readout
and every parameter the front end and the reservoir were built from; nothing else is configured here.  By default every
file is decoded like create_dataset.py decodes it (mono, 16 kHz, one clip of the model's length), goes front end ->
reservoir -> ``DeviceReadout.score_rows`` on the GPU, and one line is printed per file: name, class name, top-two logit
margin.  With ``--stream`` every file is one open-ended stream at its own length: it is pushed in chunks through
``AudioStreamBank.push_scores`` (sliding windows of ``--window-ms`` every ``--hop-ms``), the window labels go through
``pipeline.debounce`` and the events are printed.  With ``--stream --endpoint`` the stream is cut into utterances on the device
instead (``UtteranceBank.push_scores``, SPEC.md 1.17) -- the form a model trained with ``--variable-length --trim-silence`` was
fitted on -- and one line is printed per utterance: start and end time, then the label.  There is no CPU fallback.
"""
import argparse
from pathlib import Path

import numpy as np


def class_name(model, label: int) -> str:
    if label < 0:
        return "(not a number)"
    return model.class_names[label] if model.class_names else f"class_{int(model.classes[label])}"


def top_two_margin(logits: np.ndarray) -> float:
    """Largest minus second-largest logit of one row (inf for a single class, nan when a logit is NaN)."""
    if np.isnan(logits).any():
        return float("nan")
    top = np.sort(logits)
    return float(top[-1] - top[-2]) if len(top) > 1 else float("inf")


def window_plan(window_ms: float, hop_ms: float, n_thr: int, segment_steps=None):
    """``(segment_steps, window_segments, hop_segments)`` for windows of ``window_ms`` every ``hop_ms``: a time bin is 10 ms
    and ``n_thr`` raster steps; a segment is one hop unless ``segment_steps`` says otherwise, and the window is whole hops."""
    if hop_ms < 10 or window_ms < hop_ms:
        raise SystemExit("--hop-ms must be >= 10 (one time bin) and --window-ms >= --hop-ms")
    hop_bins = int(round(hop_ms / 10.0))
    S = int(segment_steps) if segment_steps else hop_bins * n_thr
    window_segments = max(1, int(round(window_ms / 10.0)) * n_thr // S)
    hop_segments = max(1, hop_bins * n_thr // S)
    if window_segments * S > 65535:
        raise SystemExit(f"--window-ms {window_ms}: a window may hold at most 65535 raster steps")
    return S, window_segments, min(hop_segments, window_segments)


def classify_clips(model, files, batch: int = 256):
    """One line per file: the clip route."""
    import create_dataset as cd
    from lsm_speech_classifier_amd import pipeline, readout
    fe, net = pipeline.pipeline_from_params(model.params)
    ro = readout.DeviceReadout(model, net.device)
    clips, names = [], []
    for f in files:
        data = cd.load_audio_file(Path(f))
        if data is None:
            continue
        clip = np.zeros(fe.n_samples, dtype=np.float32)
        clip[:min(len(data), fe.n_samples)] = data[:fe.n_samples]
        clips.append(clip)
        names.append(str(f))
    if not clips:
        return []
    rows = pipeline.features_from_audio(np.stack(clips), fe, net, model.feature_keys, batch=batch, device_out=True)
    logits, labels = ro.score_rows(rows)
    logits, labels = logits.cpu().numpy(), labels.cpu().numpy()
    out = []
    for name, lg, lab in zip(names, logits, labels):
        out.append((name, class_name(model, int(lab)), top_two_margin(lg)))
        print(f"{name}\t{out[-1][1]}\t{out[-1][2]:.6g}")
    return out


def classify_streams(model, files, window_ms: float, hop_ms: float, hold: int, background: int, chunk_ms: float = 500.0):
    """The stream route: every file one stream, events ``(file, time of the window's end in ms, class name)``."""
    import create_dataset as cd
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline, readout
    fe, net = pipeline.pipeline_from_params(model.params)
    ro = readout.DeviceReadout(model, net.device)
    n_thr = len(fe.thresholds)
    S, K, H = window_plan(window_ms, hop_ms, n_thr)
    hop = frontend.STREAM_HOP
    out = []
    for f in files:
        rate, data = cd._decode_wav(Path(f))
        if rate != cd.SAMPLE_RATE:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(rate), cd.SAMPLE_RATE)
            data = resample_poly(data, cd.SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
        n_hops = len(data) // hop
        if n_hops < 1:
            continue
        audio = np.ascontiguousarray(data[:n_hops * hop], dtype=np.float32)[None, :]
        # the streamed front ends normalise by a fixed range: calibrated on the file's own whole clips
        whole = -(-audio.shape[1] // fe.n_samples) * fe.n_samples
        calib = np.zeros(whole, dtype=np.float32)
        calib[:audio.shape[1]] = audio[0]
        calib = calib.reshape(-1, fe.n_samples)
        if fe.filterbank == "gammatone":
            front = frontend.GammatoneStream(fe.n_filters, 1, fe.db_range(calib), thresholds=fe.thresholds, gap=fe.gap,
                                             redundancy=fe.redundancy, device=fe.device)
        else:
            front = frontend.MelStream(fe.n_filters, 1, fe.mel_db_range(calib), thresholds=fe.thresholds, gap=fe.gap,
                                       redundancy=fe.redundancy, device=fe.device)
        bank = pipeline.AudioStreamBank(front, net, S, K, H, model.feature_keys, readout=ro)
        chunk = max(1, int(round(chunk_ms / 10.0))) * hop
        state = None
        for at in range(0, audio.shape[1], chunk):
            _, labels, counts = bank.push_scores(audio[:, at:at + chunk])
            events, state = pipeline.debounce(labels.cpu().numpy(), counts, state, hold, background)
            for _, w, lab in events:
                # window w ends after (w * H + K) segments of S steps; a step is 10 / n_thr ms (plus the front end's latency)
                t_ms = (w * H + K) * S * 10.0 / n_thr
                out.append((str(f), t_ms, class_name(model, lab)))
                print(f"{f}\t{t_ms:.0f} ms\t{out[-1][2]}")
        torch.cuda.synchronize()
    return out


def endpoint_from_args(a, max_bins: int) -> dict:
    """The ``frontend.EndpointStream`` keywords the ``--endpoint-*`` flags ask for; a time bin is 10 ms."""
    pad, hang, span = (int(round(v / 10.0)) for v in (a.endpoint_pad_ms, a.endpoint_hang_ms, a.endpoint_min_ms))
    if a.endpoint_top_db is not None and not (np.isfinite(a.endpoint_top_db) and a.endpoint_top_db > 0):
        raise SystemExit("--endpoint-top-db must be a finite number of dB above 0")
    if not 0 <= pad < max_bins:
        raise SystemExit(f"--endpoint-pad-ms must lie in [0, {10 * max_bins}) for this model's clips of {max_bins} time bins")
    if not max(pad, 1) <= hang <= 1024:
        raise SystemExit("--endpoint-hang-ms must be at least --endpoint-pad-ms and 10, and at most 10240")
    if not 3 <= span <= max_bins:
        raise SystemExit(f"--endpoint-min-ms must lie in [30, {10 * max_bins}]")
    return dict(top_db=a.endpoint_top_db, floor_db=a.endpoint_floor_db, pad_bins=pad, hang_bins=hang, min_span_bins=span,
                max_bins=int(max_bins))


def classify_utterances(model, files, endpoint: dict, chunk_ms: float = 500.0):
    """The endpointed stream route: every file one stream cut into utterances on the device, ``(file, start ms, end ms, class
    name)`` per utterance."""
    import create_dataset as cd
    import torch
    from lsm_speech_classifier_amd import frontend, pipeline, readout
    fe, net = pipeline.pipeline_from_params(model.params)
    why = frontend.ragged_refusal(fe.n_samples, fe.time_bins)
    if why:
        raise SystemExit(f"--endpoint needs a model whose front end takes ragged batches: {why}")
    ro = readout.DeviceReadout(model, net.device)
    hop = frontend.RAGGED_HOP
    out = []
    for f in files:
        rate, data = cd._decode_wav(Path(f))
        if rate != cd.SAMPLE_RATE:
            from math import gcd
            from scipy.signal import resample_poly
            g = gcd(int(rate), cd.SAMPLE_RATE)
            data = resample_poly(data, cd.SAMPLE_RATE // g, int(rate) // g).astype(np.float32)
        n_hops = -(-len(data) // hop)
        if n_hops < 1:
            continue
        audio = np.zeros((1, n_hops * hop), dtype=np.float32)
        audio[0, :len(data)] = data
        bank = pipeline.UtteranceBank(frontend.EndpointStream(1, device=net.device, **endpoint), fe, net, model.feature_keys,
                                      readout=ro)
        chunk = max(1, int(round(chunk_ms / 10.0)))
        for at in range(0, n_hops, chunk):
            h = min(chunk, n_hops - at)
            block = np.zeros((1, chunk * hop), dtype=np.float32)
            block[0, :h * hop] = audio[0, at * hop:(at + h) * hop]
            _, labels, bins, first, _ = bank.push_scores(block, [h], [1 if at + chunk >= n_hops else 0])
            labels, bins, first = labels.cpu().numpy(), bins.cpu().numpy(), first.cpu().numpy()
            for u in np.nonzero(bins)[0]:
                out.append((str(f), 10.0 * int(first[u]), 10.0 * int(first[u] + bins[u]), class_name(model, int(labels[u]))))
                print(f"{f}\t{out[-1][1]:.0f} ms\t{out[-1][2]:.0f} ms\t{out[-1][3]}")
        torch.cuda.synchronize()
    return out


def add_endpoint_flags(ap) -> None:
    ap.add_argument("--endpoint", action="store_true",
                    help="With --stream: cut every stream into utterances on the device and label each one.")
    ap.add_argument("--endpoint-top-db", type=float, default=30.0,
                    help="With --endpoint: a bin is speech above this many dB under the loudest of the last second (default 30).")
    ap.add_argument("--endpoint-floor-db", type=float, default=-60.0,
                    help="With --endpoint: ... and above this level relative to full scale (default -60).")
    ap.add_argument("--endpoint-pad-ms", type=float, default=30.0, help="With --endpoint: kept around an utterance (default 30).")
    ap.add_argument("--endpoint-hang-ms", type=float, default=200.0,
                    help="With --endpoint: silence that closes an utterance (default 200).")
    ap.add_argument("--endpoint-min-ms", type=float, default=30.0,
                    help="With --endpoint: a shorter burst is dropped as a click (default 30).")


def build_parser():
    ap = argparse.ArgumentParser(description="Label wav files with a saved model (main.py --save-model).")
    ap.add_argument("--model", type=str, required=True, help="Model file written by main.py --save-model.")
    ap.add_argument("files", nargs="+", help="PCM wav files.")
    ap.add_argument("--stream", action="store_true",
                    help="Treat every file as an open-ended stream: sliding windows, debounced events.")
    ap.add_argument("--window-ms", type=float, default=1000.0, help="With --stream: window length (default 1000).")
    ap.add_argument("--hop-ms", type=float, default=100.0, help="With --stream: a window every this many ms (default 100).")
    ap.add_argument("--hold", type=int, default=3,
                    help="With --stream: a label fires after winning this many consecutive windows (default 3).")
    ap.add_argument("--background", type=int, default=-1,
                    help="With --stream: label index that never fires (default: none).")
    add_endpoint_flags(ap)
    return ap


if __name__ == "__main__":
    a = build_parser().parse_args()
    from lsm_speech_classifier_amd import readout
    model = readout.LinearModel.load(a.model)
    if a.endpoint and not a.stream:
        raise SystemExit("--endpoint needs --stream")
    if a.endpoint:
        classify_utterances(model, a.files, endpoint_from_args(a, int(model.params["time_bins"])))
    elif a.stream:
        classify_streams(model, a.files, a.window_ms, a.hop_ms, a.hold, a.background)
    else:
        classify_clips(model, a.files)
