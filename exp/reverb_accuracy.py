"""Accuracy against RT60 on the synthetic 12-class chirps (profiles/reverb.txt, section 3): every clip, training and test
alike, convolved on the GPU with one of four synthetic rooms of one reverberation time (`synth.room_responses(4, rt60=X,
seed=42)`, rows drawn by `frontend.reverb_plan(n, 4, seed=42)`), then the in-memory route with the ridge readout on the
device.  One run per cell; prints one table row per filterbank: clean, then RT60 = 0.2, 0.4 and 0.8 s."""
import contextlib
import io
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import create_dataset as cd  # noqa: E402
import extract_lsm_features as ex  # noqa: E402
from lsm_speech_classifier_amd import frontend, synth  # noqa: E402

os.chdir(tempfile.mkdtemp())                        # File 2 lands here
audio, labels = cd.collect_audio(commands=None, synthetic_per_class=40)
for fb in ("gammatone", "mel"):
    cells = []
    for rt60 in (None, 0.2, 0.4, 0.8):
        reverb = None
        if rt60 is not None:
            bank, lengths = synth.room_responses(4, rt60=rt60, seed=42)
            reverb = (bank, lengths, frontend.reverb_plan(len(audio), 4, seed=42))
        with contextlib.redirect_stdout(io.StringIO()):
            acc = ex.main_from_audio(audio, labels, 128, fb, "original", 0.6, readout="torch-ridge", class_names=cd.COMMANDS,
                                     reverb=reverb)
        cells.append(acc)
    print(f"{fb:9s} | " + " | ".join(f"{100 * a:6.2f} %" for a in cells), flush=True)
