"""SPEC.md 1.17 restated in NumPy for the stream endpoint detector's tests (test_endpoint_host.py, test_gpu_endpoint.py): the
bin energies in the pinned order (trim_restatement.energies), the sliding maximum, the activity test, the state machine one
Python statement per line of the rule, and the arrays a launch writes, byte for byte, with what it leaves alone taken from a
prefill.  The state of a stream is a Python dict here: the device's block is opaque."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_restatement as TR  # noqa: E402

HOP = 160
CUT, FLUSHED = 1, 2


def params(ratio=1e-3, floor=0.0, W=100, P=3, G=20, A=3, M=100):
    return dict(ratio=float(ratio), floor=float(floor), W=int(W), P=int(P), G=int(G), A=int(A), M=int(M))


def ratio_of(top_db):
    """What `frontend.EndpointStream` passes: 10 ** (-top_db / 10), or 0.0 for None."""
    return 0.0 if top_db is None else 10.0 ** (-float(top_db) / 10.0)


def floor_of(floor_db):
    """160 * 10 ** (floor_db / 10): the energy of a bin at that level relative to full scale, or 0.0 for None."""
    return 0.0 if floor_db is None else HOP * 10.0 ** (float(floor_db) / 10.0)


def max_utterances(H, G, M):
    """lsm_endpoint_max_utterances."""
    return 2 + (int(H) - 1) // min(int(G) + 1, int(M))


def closure_spacing(P, G, M):
    """The fewest bins between the closes of two kept utterances (csrc/endpoint_body.h)."""
    d = min(G + 1, M)
    if G + 3 <= M:
        d = min(d, max(M - P, M + P - G))
    return d


def max_utterances_padded(H, P, G, M):
    return 2 + (int(H) - 1) // closure_spacing(int(P), int(G), int(M))


def fresh():
    """A stream at its start."""
    return dict(n=0, mode=0, s=0, f=0, last=0, avail=0, ehat=[], tail=np.zeros(0, dtype=np.float32), events=[])


def clamp_hops(v, n_hops):
    return int(n_hops) if v is None else int(min(max(int(v), 0), int(n_hops)))


def _stream_push(st, x, h, fin, p, max_utts):
    """One stream's push: ``x`` its 160 * h new samples.  Returns ``(e, active, utterances)``; every utterance is ``(first,
    bins, flags, samples)``, kept ones only, at most ``max_utts``.  ``st`` is advanced in place; ``st['events']`` collects
    what the run exercised (for the tests' coverage condition)."""
    W, P, G, A, M = p["W"], p["P"], p["G"], p["A"], p["M"]
    with np.errstate(all="ignore"):
        e = TR.energies(x, HOP * h, h)
    eh = np.where(np.isfinite(e), e, 0.0)
    line = np.concatenate([st["tail"], np.asarray(x[:HOP * h], dtype=np.float32)])     # the stream's timeline, its last bins
    line_first = st["n"] - len(st["tail"]) // HOP
    seen = list(st["ehat"])
    active = np.zeros(h, dtype=np.uint8)
    out = []

    def close(end, flags):
        bins = end - st["s"] + 1
        kept = bool(flags & CUT) or st["last"] - st["f"] + 1 >= A
        if kept and len(out) < max_utts:
            lo = (st["s"] - line_first) * HOP
            out.append((st["s"], bins, flags, line[lo:lo + bins * HOP].copy()))
            if st["s"] < st["n0"]:
                st["events"].append("spans_push")
        st["events"].append(("cut" if flags & CUT else "flushed" if flags & FLUSHED else "normal") if kept else "click")
        st["avail"] = end + 1
        st["mode"] = 0

    st["n0"] = st["n"]
    for j in range(h):
        n = st["n"] + j
        seen.append(eh[j])
        E = max(seen[-W:])
        on = bool(eh[j] > np.float64(E) * np.float64(p["ratio"]) and eh[j] > np.float64(p["floor"]))
        active[j] = on
        if st["mode"] == 0:
            if not on:
                continue
            if st["avail"] > n - P and n - P >= 0:
                st["events"].append("preroll_avail")
            st["s"], st["f"], st["last"], st["mode"] = max(n - P, st["avail"]), n, n, 1
        elif on:
            st["last"] = n
        if n - st["last"] == G:
            close(st["last"] + P, 0)
        elif n - st["s"] + 1 == M:
            close(n, CUT)
    st["n"] += h
    if fin and st["mode"] == 1:
        close(min(st["last"] + P, st["n"] - 1), FLUSHED)
    st["ehat"] = seen[-(W - 1):] if W > 1 else []
    st["tail"] = line[-M * HOP:]
    if fin:
        events = st["events"]
        st.update(fresh())
        st["events"] = events
    return e, active, out


def push(states, audio, hops, finish, p, max_utts, prefill=None):
    """What `lsm_endpoint_stream_f32` writes.  ``states``: a list of per-stream dicts (`fresh`), advanced in place;
    ``audio`` (B, n_hops * 160) float32; ``hops`` / ``finish``: B integers or None.  ``prefill``: a dict of the arrays as they
    stood before the launch (any subset; the others start as zeros).  Returns a dict: ``audio`` (B, max_utts, 160 * M)
    float32, ``bins`` (B, max_utts) int32, ``first`` (B, max_utts) int64, ``flags`` (B, max_utts) int32, ``count`` (B,) int32,
    ``energy`` (B, n_hops) float64, ``active`` (B, n_hops) uint8."""
    audio = np.asarray(audio)
    assert audio.ndim == 2 and audio.dtype == np.float32 and audio.shape[1] % HOP == 0
    B, n_hops, M = audio.shape[0], audio.shape[1] // HOP, p["M"]
    shapes = dict(audio=((B, max_utts, HOP * M), np.float32), bins=((B, max_utts), np.int32), first=((B, max_utts), np.int64),
                  flags=((B, max_utts), np.int32), count=((B,), np.int32), energy=((B, n_hops), np.float64),
                  active=((B, n_hops), np.uint8))
    out = {}
    for name, (shape, dtype) in shapes.items():
        if prefill is not None and name in prefill:
            out[name] = np.array(prefill[name], dtype=dtype, copy=True).reshape(shape)
        else:
            out[name] = np.zeros(shape, dtype=dtype)
    out["bins"][:] = 0
    out["count"][:] = 0
    for b in range(B):
        h = clamp_hops(None if hops is None else hops[b], n_hops)
        fin = finish is not None and int(finish[b]) != 0
        if h == 0:
            states[b]["events"].append("no_hops")
        if h == 0 and not fin:
            continue
        e, active, utts = _stream_push(states[b], audio[b], h, fin, p, max_utts)
        out["energy"][b, :h].view(np.uint64)[:] = e.view(np.uint64)
        out["active"][b, :h] = active
        out["count"][b] = len(utts)
        for u, (first, bins, flags, samples) in enumerate(utts):
            row = out["audio"][b, u].view(np.uint32)
            row[:] = 0
            row[:bins * HOP] = samples.view(np.uint32)
            out["bins"][b, u], out["first"][b, u], out["flags"][b, u] = bins, first, flags
    return out


def listing(out):
    """The utterances of one push's arrays: ``[(stream, first, bins, flags, samples as bytes)]`` in slot order."""
    found = []
    for b in range(out["count"].shape[0]):
        for u in range(int(out["count"][b])):
            bins = int(out["bins"][b, u])
            found.append((b, int(out["first"][b, u]), bins, int(out["flags"][b, u]), out["audio"][b, u, :bins * HOP].tobytes()))
    return found


def cut_recording(x, p, chunk_hops=100):
    """A whole recording (1-D float32, zero-padded to whole bins) pushed in chunks of ``chunk_hops`` with a finish at its end:
    ``[(first, bins, flags, samples as a float32 array)]``."""
    x = np.asarray(x, dtype=np.float32)
    nb = -(-len(x) // HOP)
    padded = np.zeros(nb * HOP, dtype=np.float32)
    padded[:len(x)] = x
    st = [fresh()]
    found = []
    max_utts = max_utterances_padded(chunk_hops, p["P"], p["G"], p["M"])
    for lo in range(0, max(nb, 1), chunk_hops):
        h = min(chunk_hops, nb - lo)
        row = np.zeros((1, chunk_hops * HOP), dtype=np.float32)
        row[0, :h * HOP] = padded[lo * HOP:(lo + h) * HOP]
        out = push(st, row, [h], [1 if lo + chunk_hops >= nb else 0], p, max_utts)
        found += [(first, bins, flags, np.frombuffer(raw, dtype=np.float32).copy()) for _, first, bins, flags, raw in listing(out)]
    return found
