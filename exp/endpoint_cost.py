"""Writes profiles/endpoint.txt (`--out`; printed as well).  Four parts.

The code object: csrc/endpoint.hip and csrc/trim.hip compiled with the build's flags and
`-Rpass-analysis=kernel-resource-usage`, the compiler's own report of `endpoint_kernel` and of `trim_kernel` (which shares
bin_energy.h) -- registers, scratch, spills, occupancy, static LDS.  Needs hipcc, no GPU (`--no-timing` stops here).

(a) The endpoint launch alone: 256 streams, pushes of 10 and of 100 hops cut from synthetic speech (`class_chirps(noise=0.001)`
between stretches of faint noise), `lsm_endpoint_stream_f32` at the defaults (30 dB, -60 dB floor, W 100, P 3, G 20, M 100)
beside `lsm_trim_silence_f32` on the same bytes (rows of n_hops bins) and the NumPy restatement of the same push on one core.
Device events, medians of 20 after 4 warm-up launches, the forms alternating, `--rounds` times over.  The state goes from one
block to another, so that every launch does the same work (and copies the whole audio ring), and in place as `EndpointStream`
keeps it (the same push again and again: the stream moves on, the work is a push's).

(b) `UtteranceBank.push_scores` per push of 100 hops, 256 streams at cfg2's front end and reservoir (128 filters, 1000
neurons, k = 200, 400 output neurons), a 12-class readout: the slot batch with its empty slots riding along against
`compact=True`, at the speech duty cycle the streams have (printed).  Host clock around a push and a device synchronise,
the two forms alternating on banks of their own, medians over the pushes of a 6-second stream after one warm-up stream.

(c) 256 recordings of 3 seconds: `UtteranceBank` end to end (pushes of 100 hops, finish with the last) against reading the
audio back -- `utterances_from_recordings` on the host, then `features_from_utterances` and `score_rows`.  Host clock, medians
of 3 after a warm-up run each, alternating."""
import argparse
import collections
import copy
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lsm_speech_classifier_amd import build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-timing", action="store_true", help="the code objects only (no GPU needed)")
args = ap.parse_args()

lines = []


def code_object(src, kernel):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc] + build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
                                                     "-c", os.path.join(build.PKG_DIR, "csrc", src), "-o",
                                                     os.path.join(tmp, "out.o")], capture_output=True, text=True, check=True)
    report = [m.group(1).strip() for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr)]
    lines.append(f"{kernel}, the compiler's resource report (hipcc " + " ".join(build.CFLAGS) + "):")
    lines.extend("  " + ln for ln in report)
    fields = dict(ln.split(": ", 1) for ln in report if ": " in ln)
    assert fields["ScratchSize [bytes/lane]"] == "0" and fields["VGPRs Spill"] == "0", f"{kernel} uses scratch"


code_object("endpoint.hip", "endpoint_kernel")
code_object("trim.hip", "trim_kernel")

if not args.no_timing:
    import torch
    import endpoint_restatement as ER
    from lsm_speech_classifier_amd import _lib, frontend, pipeline, readout, reservoir, snn, synth
    from oracle import ref_numpy

    lib = _lib.load()
    _lib.require_gpu()
    B, HOP, F = 256, 160, 128
    W, P, G, A, M = 100, 3, 20, 3, 100
    ratio, floor = frontend.trim_ratio(30.0), frontend.endpoint_floor(-60.0)
    lines += [f"build id {lib.lsm_build_id().decode()}", f"device: {torch.cuda.get_device_name(0)}",
              f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}"]
    void = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream

    def speech(n_streams, seconds, seed):
        """Streams of ``seconds`` seconds: a synthetic word (a second of `class_chirps(noise=0.001)`) in every second second,
        faint noise in between, every stream shifted by its own number of bins."""
        rng = np.random.default_rng(seed)
        x = (0.0003 * rng.standard_normal((n_streams, seconds * 16000))).astype(np.float32)
        for s in range(0, seconds, 2):
            x[:, s * 16000:(s + 1) * 16000] = synth.class_chirps(np.arange(n_streams) % 12, seed=seed + s, noise=0.001)
        for b in range(n_streams):
            x[b] = np.roll(x[b], HOP * int(rng.integers(0, 100)))
        return x

    def timed(fn, reps=20, warm=4):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    # ---- (a) the launch alone ---------------------------------------------------------------------------------------------
    line = speech(B, 4, 11)
    p = ER.params(ratio, floor, W, P, G, A, M)
    for H in (10, 100):
        U = frontend.endpoint_max_utterances(H, P, G, M)
        assert U == lib.lsm_endpoint_max_utterances(H, G, M)
        # the second second of the streams' history is in the state: the timed push is the one behind it
        sb = int(lib.lsm_endpoint_state_bytes(W, M))
        state0 = torch.zeros((B, sb), dtype=torch.uint8, device="cuda")
        state1 = torch.empty_like(state0)
        utt = torch.zeros((B * U, HOP * M), dtype=torch.float32, device="cuda")
        bins, flags, count = (torch.zeros((n,), dtype=torch.int32, device="cuda") for n in (B * U, B * U, B))
        first = torch.zeros((B * U,), dtype=torch.int64, device="cuda")

        def push(x, s_in, s_out):
            assert lib.lsm_endpoint_stream_f32(void(x), B, H, None, None, C.c_double(ratio), C.c_double(floor), W, P, G, A, M,
                                               void(s_in), void(s_out), U, void(utt), void(bins), void(first), void(flags),
                                               void(count), None, None, stream) == 0
        states = [ER.fresh() for _ in range(B)]
        at = 200 - H if H == 10 else 200                            # the history: bins 0 .. at - 1, in pushes of 100 and the rest
        lo = 0
        big = torch.zeros((B * 6, HOP * M), dtype=torch.float32, device="cuda")
        big_bins = torch.zeros((B * 6,), dtype=torch.int32, device="cuda")
        while lo < at:
            step = min(100, at - lo)                                # at most 6 slots per stream
            chunk = np.ascontiguousarray(line[:, lo * HOP:(lo + step) * HOP])
            xh = torch.from_numpy(chunk).cuda()
            assert lib.lsm_endpoint_stream_f32(void(xh), B, step, None, None, C.c_double(ratio), C.c_double(floor), W, P, G, A, M,
                                               void(state0), void(state0), 6, void(big), void(big_bins), None, None, None, None,
                                               None, stream) == 0
            torch.cuda.synchronize()
            ER.push(states, chunk, None, None, p, 6)
            lo += step
        del big
        now = np.ascontiguousarray(line[:, at * HOP:(at + H) * HOP])
        x = torch.from_numpy(now).cuda()
        push(x, state0, state1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = ER.push(copy.deepcopy(states), now, None, None, p, U)
        t_numpy = (time.perf_counter() - t0) * 1e3
        got = dict(audio=utt.cpu().numpy().reshape(B, U, -1), bins=bins.cpu().numpy().reshape(B, U), first=first.cpu().numpy().reshape(B, U),
                   flags=flags.cpu().numpy().reshape(B, U), count=count.cpu().numpy())
        same = ER.listing(got) == ER.listing(want)
        lines.append(f"(a) {B} streams x {H} hops behind {at} bins of history: {int(want['count'].sum())} utterances close in the push, "
                     f"{int(want['bins'].sum())} bins; max_utts {U}; the launch's utterances equal the restatement's byte for byte: {same}")
        t_out = torch.empty((B, HOP * max(H, 3)), dtype=torch.float32, device="cuda")
        t_first, t_bins = (torch.empty((B,), dtype=torch.int32, device="cuda") for _ in range(2))
        state2 = state0.clone()
        forms = [(f"lsm_endpoint_stream_f32, {H:3d} hops, block to block", lambda: push(x, state0, state1)),
                 (f"lsm_endpoint_stream_f32, {H:3d} hops, state in place", lambda: push(x, state2, state2)),
                 (f"lsm_trim_silence_f32, rows of {H:3d} bins", lambda: lib.lsm_trim_silence_f32(
                     void(x), B, H * HOP, H, None, C.c_double(ratio), P, 3, void(t_out), int(t_out.shape[1]), void(t_first), void(t_bins),
                     None, stream))]
        med = collections.defaultdict(list)
        for rnd in range(1, args.rounds + 1):
            for name, fn in forms:
                t = timed(fn)
                med[name].append(t[0])
                lines.append(f"  round {rnd}: {name}  median {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f})")
        for name, v in med.items():
            lines.append(f"  {name}: median of the rounds {np.median(v):8.1f} us, rounds between {min(v):.1f} and {max(v):.1f}")
        lines.append(f"  the NumPy restatement of the same push, one core: {t_numpy:8.1f} ms (one run)")

    # ---- (b) a push through the bank: empty slots riding along against compact -----------------------------------------------
    fe = frontend.SpikeFrontEnd(F, "gammatone")
    k = 200
    quiet = synth.class_chirps(np.arange(32) % 12, seed=1234, noise=0.001)
    wc = ref_numpy.w_critico(k, 2.0, 2, fe.encode(quiet).cpu().numpy())
    params = reservoir.SimulationParams(num_neurons=1000, num_output_neurons=400, small_world_graph_k=k, mean_weight=wc * 0.6)
    net = snn.SNN(params, n_channels=fe.n_channels)
    keys = ['spike_counts', 'spike_variances', 'mean_spike_times', 'mean_isi', 'isi_variances']
    rng = np.random.default_rng(0)
    D = len(keys) * 400
    model = readout.LinearModel(rng.standard_normal(D), rng.uniform(0.5, 2.0, D), rng.standard_normal((12, D)) * 0.01,
                                rng.standard_normal(12), np.arange(12), keys, 400)
    ro = readout.DeviceReadout(model, net.device)
    seconds = 6
    line = speech(B, seconds, 23)
    U = frontend.endpoint_max_utterances(100, P, G, M)
    lines.append(f"(b) UtteranceBank.push_scores, {B} streams x 100 hops per push, {B * U} slots of {M} bins; ragged fused step served for "
                 f"the slot batch: {pipeline.step_fused_supported(fe, net, B * U, 'ragged')}; GPU_MAX_HW_QUEUES="
                 f"{os.environ.get('GPU_MAX_HW_QUEUES')}")

    def stream_run(compact, took, emitted):
        bank = pipeline.UtteranceBank(frontend.EndpointStream(B), fe, net, keys, readout=ro)
        for s in range(seconds):
            x = torch.from_numpy(np.ascontiguousarray(line[:, s * 16000:(s + 1) * 16000])).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = bank.push_scores(x, compact=compact)
            torch.cuda.synchronize()
            took.append((time.perf_counter() - t0) * 1e3)
            emitted.append(int((out[2] > 0).sum()))
            speech_bins.append(int(out[2].sum()))

    speech_bins = []
    for compact in (False, True):
        stream_run(compact, [], [])
    took, emitted = {False: [], True: []}, {False: [], True: []}
    speech_bins = []
    for rnd in range(args.rounds):
        for compact in (False, True):
            stream_run(compact, took[compact], emitted[compact])
    duty = sum(speech_bins) / (len(speech_bins) * B * 100)
    lines.append(f"  utterances per push: {np.mean(emitted[False]):.1f} of {B * U} slots on average (min {min(emitted[False])}, max "
                 f"{max(emitted[False])}); speech duty cycle {duty:.3f} of the streams' bins lie inside emitted utterances")
    for compact, name in ((False, "empty slots riding along (no host read)"), (True, "compact=True (one read-back of the bins) ")):
        v = took[compact]
        lines.append(f"  {name}: median {np.median(v):8.2f} ms per push (min {min(v):.2f}, max {max(v):.2f}, {len(v)} pushes)")
    lines.append(f"  riding along / compact = {np.median(took[False]) / np.median(took[True]):.3f}")

    # ---- (c) recordings end to end ------------------------------------------------------------------------------------------
    recs = speech(B, 3, 41)
    lines.append(f"(c) {B} recordings of 3 s: UtteranceBank end to end against utterances_from_recordings + features_from_utterances + "
                 f"score_rows")

    def bank_route(compact):
        bank = pipeline.UtteranceBank(frontend.EndpointStream(B), fe, net, keys, readout=ro)
        labels = []
        for s in range(3):
            out = bank.push_scores(recs[:, s * 16000:(s + 1) * 16000], None, np.full(B, int(s == 2)), compact=compact)
            labels.append((out[1].cpu().numpy(), out[2].cpu().numpy()))
        return sum(int((b > 0).sum()) for _, b in labels)

    def host_route():
        utts, table = pipeline.utterances_from_recordings(list(recs), None, chunk_hops=100)
        rows = pipeline.features_from_utterances(utts, fe, net, keys)
        ro.score_rows(rows)[1].cpu()
        return len(utts)

    routes = [("UtteranceBank, slots riding along", lambda: bank_route(False)), ("UtteranceBank, compact=True      ", lambda: bank_route(True)),
              ("read back, host slices, clips    ", host_route)]
    n_found = {name: fn() for name, fn in routes}
    torch.cuda.synchronize()
    lines.append(f"  utterances found: {n_found}")
    took = collections.defaultdict(list)
    for rep in range(3):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            took[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in took.items():
        lines.append(f"  {name}: median of 3 {np.median(v):8.2f} ms (min {min(v):.2f}, max {max(v):.2f})")

print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
