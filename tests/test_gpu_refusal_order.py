"""The first refusal wins: a run export given two bad arguments at once reports the one its checks reach first, returns
LSM_ERR_ARG and launches nothing.  The order is part of the ABI's behaviour -- it decides which reason a caller reads -- and
all six run exports share it (csrc/reservoir.hip, check_run): null handle, n_clips / n_steps, the segment arguments, the
continuation arguments and n_keys, the alignment of the per-clip counts, waves_per_clip, the empty batch (LSM_OK before any
buffer is looked at), null buffers, the device, the key ids, the plan, the order workspace.  Only the ABI is touched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CLIPS, N_STEPS, SEGMENT_STEPS = 2, 24, 8

_KEYED = "key_ids n_keys feats sm vt stats wpc".split()
_WORKSPACE = "ws ws_bytes stream".split()
_FROM = "first_step state_in state_out".split()
# the parameters of every run export behind (handle, spikes, n_clips, n_steps), in the order of include/lsm_hip*.h
PARAMS = {
    "lsm_reservoir_run": _KEYED + ["stream"],
    "lsm_reservoir_run_ordered": _KEYED + _WORKSPACE,
    "lsm_reservoir_run_from": _FROM + _KEYED + _WORKSPACE,
    "lsm_reservoir_run_segments": ["segment_steps"] + _FROM + ["records"] + _KEYED + _WORKSPACE,
    "lsm_reservoir_run_ragged": ["counts"] + _FROM + _KEYED + _WORKSPACE,
    "lsm_reservoir_run_stream": "segment_steps counts state_in state_out records sm vt stats wpc".split() + _WORKSPACE,
}
# (the two bad arguments, the message of the check that comes first, the exports that take both arguments)
BOTH_BAD = [
    (dict(n_steps=0, wpc=17), b"bad n_clips/n_steps", list(PARAMS)),
    (dict(segment_steps=0, state_in="misaligned"), b"segment_steps=0 must be >= 1",
     ["lsm_reservoir_run_segments", "lsm_reservoir_run_stream"]),
    (dict(first_step=-1, n_keys=9), b"first_step=-1 must be >= 0",
     ["lsm_reservoir_run_from", "lsm_reservoir_run_segments", "lsm_reservoir_run_ragged"]),
    (dict(counts="misaligned", wpc=17), b"clip_steps must be 4-byte aligned", ["lsm_reservoir_run_ragged"]),
    (dict(counts="misaligned", wpc=17), b"clip_segments must be 4-byte aligned", ["lsm_reservoir_run_stream"]),
    (dict(n_keys=0, spikes=None), b"n_keys must be in [1, 8]", ["lsm_reservoir_run", "lsm_reservoir_run_ordered"]),
    (dict(ws_bytes=8, key_ids="nine"), b"key id 9 out of range",
     ["lsm_reservoir_run_ordered", "lsm_reservoir_run_from", "lsm_reservoir_run_segments", "lsm_reservoir_run_ragged"]),
]


def test_the_first_refusal_wins():
    import torch
    from lsm_speech_classifier_amd import _lib, reservoir as R, snn
    from test_gpu_ragged import REFRACTORY, SHAPES
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    n, k, n_out, c = SHAPES[0]
    net = snn.SNN(None, reservoir=R.build_reservoir(R.SimulationParams(
        num_neurons=n, num_output_neurons=n_out, small_world_graph_k=k, mean_weight=2.0 / (k // 2),
        refractory_period=REFRACTORY), c))
    lib = net.lib

    def filled(shape, dtype, value):
        return torch.full(shape, value, dtype=dtype, device="cuda")

    nan = float("nan")
    outputs = {"feats": filled((N_CLIPS, n_out), torch.float32, nan),
               "sm": filled((N_CLIPS, N_STEPS, n), torch.uint8, 0xAB),
               "vt": filled((N_CLIPS, N_STEPS, n), torch.float32, nan),
               "stats": filled((N_CLIPS, 2), torch.int32, -1),
               "records": filled((N_CLIPS, N_STEPS // SEGMENT_STEPS, n_out, 4), torch.int32, -1),
               "state_out": filled((N_CLIPS, net.state_bytes()), torch.uint8, 0xCD),
               "ws": filled((2 * N_CLIPS,), torch.int32, -1)}
    sentinels = {name: t.clone() for name, t in outputs.items()}
    spikes = torch.zeros((N_CLIPS, c, N_STEPS), dtype=torch.uint8, device="cuda")
    state_in = torch.zeros((N_CLIPS, net.state_bytes()), dtype=torch.uint8, device="cuda")
    counts = torch.full((N_CLIPS,), N_STEPS // SEGMENT_STEPS, dtype=torch.int32, device="cuda")
    key_ids, nine = np.array([0], dtype=np.int32), np.array([9], dtype=np.int32)
    assert state_in.data_ptr() % 16 == 0 and counts.data_ptr() % 4 == 0
    good = dict(spikes=spikes.data_ptr(), n_clips=N_CLIPS, n_steps=N_STEPS, segment_steps=SEGMENT_STEPS, first_step=0,
                state_in=state_in.data_ptr(), counts=counts.data_ptr(), key_ids=key_ids.ctypes.data, n_keys=1, wpc=0,
                ws_bytes=lib.lsm_reservoir_order_workspace(N_CLIPS), stream=torch.cuda.current_stream().cuda_stream,
                **{name: t.data_ptr() for name, t in outputs.items()})
    special = {("state_in", "misaligned"): state_in.data_ptr() + 8, ("counts", "misaligned"): counts.data_ptr() + 2,
               ("key_ids", "nine"): nine.ctypes.data}

    def call(export, values):
        args = [values[name] for name in ["spikes", "n_clips", "n_steps"] + PARAMS[export]]
        return getattr(lib, export)(net._handle, *args)

    for bad, message, exports in BOTH_BAD:
        for export in exports:
            assert set(bad) <= set(["spikes", "n_clips", "n_steps"] + PARAMS[export]), (export, bad)
            assert lib.lsm_reservoir_set_kernel(None, 0) == -1              # another message, so a stale one cannot pass
            rc = call(export, {**good, **{name: special.get((name, v), v) for name, v in bad.items()}})
            assert rc == -1 and message in lib.lsm_last_error(), (export, bad, rc, lib.lsm_last_error())
    # an empty batch is accepted before its buffers are looked at
    empty = {**good, **dict.fromkeys(["spikes", "state_in", "counts", "ws", *outputs]), "n_clips": 0, "ws_bytes": 0}
    for export in PARAMS:
        # lsm_reservoir_run and _run_ordered want a key even then; the others refuse a key without a features buffer
        values = empty if "first_step" not in PARAMS[export] else {**empty, "key_ids": None, "n_keys": 0}
        assert call(export, values) == 0, (export, lib.lsm_last_error())
    torch.cuda.synchronize()
    for name, t in outputs.items():
        assert torch.equal(t.view(torch.uint8), sentinels[name].view(torch.uint8)), f"{name} was written"
    _lib.check(call("lsm_reservoir_run", good), "lsm_reservoir_run")         # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert not torch.isnan(outputs["feats"]).any()
