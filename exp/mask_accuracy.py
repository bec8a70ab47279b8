"""Accuracy with and without masks in training on the synthetic 12-class chirps (profiles/spec_mask.txt, section 3): 128
gammatone filters, the reference's reservoir, the ridge readout on the device, an 80 / 20 split.  The TRAINING clips are
encoded plain or with masks drawn by `frontend.mask_plan` (2 frequency masks up to 15 filters wide, 2 time masks up to 20
bins wide, every clip, seed 42); the TEST clips are never masked and are encoded clean and with coloured noise at 10 dB SNR
(`synth.coloured_noise(4, seed=42)`, `frontend.mix_plan(seed=42)`).  One run per cell; nothing is asserted."""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import create_dataset as cd  # noqa: E402
import extract_lsm_features as ex  # noqa: E402
import torch  # noqa: E402
from sklearn.model_selection import train_test_split  # noqa: E402
from lsm_speech_classifier_amd import frontend, pipeline, readout as ro, synth  # noqa: E402
from lsm_speech_classifier_amd.snn import SNN  # noqa: E402

audio, labels = cd.collect_audio(commands=None, synthetic_per_class=40)
audio, labels = np.ascontiguousarray(audio, dtype=np.float32), np.asarray(labels, dtype=np.int32)
idx_train, idx_test, y_train, y_test = train_test_split(np.arange(len(audio)), labels, test_size=0.2, random_state=42,
                                                        stratify=labels)
fe = frontend.SpikeFrontEnd(128, "gammatone")
with contextlib.redirect_stdout(io.StringIO()):
    head = fe.encode(audio[idx_train[:500]]).cpu().numpy()
    params = ex._simulation_params(head[0], None, None, None, None, None)
    params.mean_weight = ex.calculate_theoretical_w_critico(params, head) * 0.6
    params.weight_variance = ex.WEIGHT_VARIANCE
    net = SNN(simulation_params=params)
keys = ex.FEATURE_SETS["original"]
plan = frontend.mask_plan(len(audio), fe.n_filters, fe.time_bins, freq_masks=2, freq_width=15, time_masks=2, time_width=20,
                          seed=42)
noise = synth.coloured_noise(4, seed=42).astype(np.float32)
mixer = frontend.NoiseMixer(noise)
mix = frontend.mix_plan(len(audio), 4, noise.shape[1], 10.0, seed=42)


def rows(idx, mask=None, corrupt=None):
    return pipeline.features_from_audio(audio[idx], fe, net, keys, device_out=True,
                                        **({} if mask is None else {"mask": mask.take(idx)}),
                                        corrupt=None if corrupt is None else (mixer, corrupt.take(idx)))


tests = {"clean": rows(idx_test), "10 dB": rows(idx_test, corrupt=mix)}
y = torch.from_numpy(y_train).to(fe.device)
print("training  | test clean | test 10 dB SNR")
for name, mask in (("plain", None), ("masked", plan)):
    scaler = ro.StandardScaler()
    model = ro.RidgeReadout(1.0).fit(scaler.fit_transform(rows(idx_train, mask=mask)), y)
    cells = [float((model.predict(scaler.transform(X)).cpu().numpy() == y_test).mean()) for X in tests.values()]
    print(f"{name:9s} | " + " | ".join(f"{100 * a:8.2f} %" for a in cells), flush=True)
