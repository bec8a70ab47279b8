"""bench.py's driver contract on the GPU box: one JSON line with the required keys and sane values, the roofline and
cpu_baseline objects of --full, the outputs of --dump-outputs (tiny K so the test stays short)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, full=True):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2",
                          *(["--full"] if full else []), *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _fractions(obj, path=""):
    """Every (path, value) in the line whose key says it is a fraction."""
    if isinstance(obj, dict):
        for k, v in obj.items():
            if isinstance(v, (dict, list)):
                yield from _fractions(v, f"{path}.{k}")
            elif "frac" in k and v is not None:
                yield f"{path}.{k}", v
    elif isinstance(obj, list):
        for i, v in enumerate(obj):
            yield from _fractions(v, f"{path}[{i}]")


def _check_fractions(d):
    """a fraction above 1 is not evidence -- every `*frac*` of the line lies in [0, 1], and the duration
    `roofline.frac` is built on cannot exceed what a launch takes inside the overlapped region."""
    found = list(_fractions(d))
    assert len(found) >= 4, found
    for path, v in found:
        assert 0.0 <= v <= 1.0, (path, v)
    r = d["roofline"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert abs(r["achieved"] - r["bytes_per_clip"] * d["config"]["clips_per_gpu"] / (r["kernel_ms"] * 1e-3) / 1e9) \
        < 1e-3 * r["achieved"] + 0.02
    assert "lone launch" in r["kernel_ms_source"] and r["bound_by"]
    assert abs(r["launches_in_flight"] - r["in_region_kernel_ms"] / d["ms_per_step"]) < 0.02


def test_bench_line_contract():
    d = _run("--batch", "64")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "clips/s" and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    # `bound` is what bounds the kernel (cfg2: one clip's dependency chain, the table sits in L2), the figures
    # achieved / peak / frac are the streamed-bytes MODEL against the HBM peak, and the measured share travels beside it
    assert r["bound"] == "latency" and r["model"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    assert "hbm_frac_measured" in r and r["hbm_frac_measured"] is None          # no counter passes for a 64-clip batch
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and r["kernel_ms"] > 0
    _check_fractions(d)
    # the figure of the round-2 protocol (no 40 ms of priming) travels beside the headline
    u = d["unprimed"]
    assert u["value"] > 0 and abs(u["value"] - 64 / (u["ms_per_step"] * 1e-3)) / u["value"] < 1e-3 and "round-2" in u["protocol"]
    # the line says where `traffic` comes from (never a silent null), and carries the gather ceiling
    assert r["traffic"] is None and r["traffic_source"].startswith("none:") and "cfg2_B64_dense" in r["traffic_source"]
    assert r["gather_ceiling"] == 16800.0 and 4e6 < r["weight_table_bytes"] < 4.5e6      # 1000 x 1024 x 4: L2 resident
    g = r["row_gather"]
    assert g["rows_per_launch"] > 0 and g["mean_row_bytes"] == 4096.0 and g["requested_over_memory_side"] is None
    assert g["requested_bytes"] == g["rows_per_launch"] * 4096 and g["gbs_lone_launch"] > 0
    assert not any("frac" in k for k in g)              # a request rate is not a fraction of the memory-side ceiling
    assert r["memory_side_frac"] is None
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["unit"] == "clips/s" and c["value"] > 0 and c["sample"]
    assert d["value"] / c["value"] > 100           # north star: >= 100x the CPU reference at 1 GPU


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    """Without --full the run does only what the headline needs: no unprimed pass, roofline or CPU baseline in the line.
    --dump-outputs writes the feature rows of the last timed step; the inputs are seeded, so the serial path (one
    stream) writes the same rows as the overlapped one."""
    d = _run("--batch", "64", "--dump-outputs", str(tmp_path / "overlapped"), full=False)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 6 and d["warmup"] == 2 and d["unit"] == "clips/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert not {"unprimed", "roofline", "cpu_baseline"} & set(d)
    assert "unprimed pass" not in d["config"]["prime"]
    feats = np.load(tmp_path / "overlapped" / "features.npy")
    assert feats.dtype == np.float32 and feats.shape == (64, 5 * 400) and np.isfinite(feats).all()
    assert abs(feats[:, :400].sum(axis=1).mean() - d["config"]["mean_output_spikes_per_clip"]) < 1e-3
    assert sorted(os.listdir(tmp_path / "overlapped")) == ["features.npy"]
    _run("--batch", "64", "--streams", "1", "--dump-outputs", str(tmp_path / "serial"), full=False)
    np.testing.assert_array_equal(np.load(tmp_path / "serial" / "features.npy"), feats)


def test_bench_line_names_the_committed_traffic_file_at_the_headline_shape():
    d = _run("--no-cpu-baseline")                       # cfg2 at its own batch: the shape profiles/lif_traffic.json holds
    r = d["roofline"]
    assert r["traffic"] > 0 and "profiles/lif_traffic.json[cfg2_B256_dense]" in r["traffic_source"]
    assert "not measured in this run" in r["traffic_source"]
    assert 0 < r["memory_side_frac"] < 1 and r["memory_side_gbs_lone_launch"] > 0
    # the counter traffic of a launch over its duration over the HBM peak: a few percent at cfg2, far below the model's frac
    assert 0 < r["hbm_frac_measured"] < 0.1 < r["frac"] and r["bound"] == "latency"
    assert abs(r["hbm_frac_measured"] - r["traffic"] / (r["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-4
    assert "unprimed pass" in d["config"]["prime"] and d["config"]["setup_s"]["build_reservoir_s"] > 0
    _check_fractions(d)
    # `frac` rests on the lone launch: not longer than a launch takes while others overlap it, nor than a step of the
    # overlapped path times the launches in flight; the in-region figure and the wall-clock figure
    # travel beside it
    assert r["launches_in_flight"] > 1 and r["kernel_ms"] <= r["in_region_kernel_ms"] * 1.02
    assert r["kernel_ms"] <= d["ms_per_step"] * r["launches_in_flight"] * 1.02
    assert abs(r["pipeline_frac"] - r["in_region_frac"] * r["launches_in_flight"]) < 0.01 * r["pipeline_frac"] + 1e-4
    assert r["frac"] >= r["in_region_frac"]
    assert d["config"]["reservoir_launch_order"] == "batch order"          # 256 clips: one per compute unit
    assert d["config"]["hw_queues"] == 12 and d["config"]["streams"] == 6 and d["config"]["fe_streams"] == 5


def test_bench_stages_and_serial_mode():
    d = _run("--batch", "64", "--stage", "reservoir", "--no-cpu-baseline", "--streams", "1")
    _check_fractions(d)
    assert "cpu_baseline" not in d and d["config"]["stage"] == "reservoir" and d["config"]["pipeline"] == "serial"
    d = _run("--batch", "64", "--stage", "frontend", "--no-cpu-baseline")
    assert "roofline" not in d and d["value"] > 0


@pytest.mark.parametrize("config,batch", [("cfg4", "256"), ("cfg5", "512")])
def test_fractions_of_the_large_configs_stay_within_one(config, batch):
    """The ring-row kernel's gather figures charge a spike the bytes it requests, not the padded table: no fraction
    of the cfg4 / cfg5 lines exceeds 1 (r03's cfg5 line read 1.22).  Batches at which SURVEY.md 8(d)'s streamed model
    is a lower bound at all: T*|W|/B grows without limit as B shrinks, while an event-driven kernel gathers a clip's own
    rows whatever B is (at 64 clips the model charges cfg5 640 MB per clip)."""
    d = _run("--config", config, "--batch", batch, "--no-cpu-baseline", "--steps", "3", "--warmup", "1")
    _check_fractions(d)
    r = d["roofline"]
    # cfg4 (uniform leak, 128 channels, 32 blocks of 128 neurons) runs the pair-block form of the ring rows, cfg5 the quads
    assert r["kernel"] == ("lif_pair_kernel" if config == "cfg4" else "lif_ring_kernel")
    assert r["bound"] == ("latency" if config == "cfg4" else "gather") and r["model"] == "hbm"
    assert r["row_gather"]["mean_row_bytes"] * d["config"]["num_neurons"] <= r["weight_table_bytes"]
    assert r["row_gather"]["gbs_lone_launch"] > 0


def test_a_rank_started_by_the_launcher_inherits_what_rccl_needs():
    """VERDICT r4 #4a: the first run with more than one rank must not be the first time the launcher's environment is
    looked at.  `bench.py --gpus 1` through its OWN launcher (LSM_BENCH_FORCE_SPAWN=1) with the distributed code path
    forced (LSM_BENCH_FORCE_DIST=1: process group over RCCL, broadcast, all-gather, barrier -- with one rank): the rank
    process must carry HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC, what RCCL between processes needs on this driver) and
    GPU_MAX_HW_QUEUES=16 (pipeline streams + the exchange), and the line must hold the exchange and fence records."""
    env = {k: v for k, v in os.environ.items() if k not in ("HSA_ENABLE_IPC_MODE_LEGACY", "GPU_MAX_HW_QUEUES", "RANK",
                                                            "WORLD_SIZE", "LOCAL_RANK")}
    env.update(LSM_BENCH_FORCE_SPAWN="1", LSM_BENCH_FORCE_DIST="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                          "--batch", "64", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600,
                         cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["rank_env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert d["rank_env"]["GPU_MAX_HW_QUEUES"] == "16" and d["config"]["hw_queues"] == 16
    assert d["rank_env"]["MASTER_ADDR"] == "127.0.0.1" and d["rank_env"]["WORLD_SIZE"] == "1"
    x = d["exchange"]
    assert x["mode"] == "once" and x["exchange_ms"] is not None and x["digest"] is not None      # the default exchange
    assert x["exchange_bytes"] == 6 * 64 * 2000 * 4
    assert set(d["fences"]) >= {"start_barrier_ms", "start_synchronize_ms", "end_barrier_ms", "end_synchronize_ms"}
    # the rank's set-up times reach the parent's stderr, tagged with the rank (VERDICT r4 #4b, #4c)
    assert "[rank 0] bench.py[rank 0/1]: set-up cfg2: build_reservoir" in out.stderr, out.stderr[-1500:]


def test_chunked_exchange_over_two_gpus_equals_the_single_exchange():
    """the chunked exchange (all-gathers on a stream of their own while later steps run) against the product's
    single exchange, over RCCL with two ranks on two GPUs: same gathered rows (digest).  Skipped on a one-GPU box -- which
    is why 'once' is the default until this has run."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    digests = {}
    for mode in ("once", "chunked"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2",
                              "--batch", "64", "--full", "--no-cpu-baseline", "--exchange", mode], capture_output=True,
                             text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert d["n_gpus"] == 2 and d["exchange"]["mode"] == mode
        digests[mode] = d["exchange"]["digest"]
    assert digests["once"] == digests["chunked"] and digests["once"] is not None
