"""GPU: bench.py as the driver runs it -- the JSON contract at N=1, and `--gpus 2` spawning two ranks by itself
(gloo rehearsal: a one-GPU box cannot host two RCCL ranks, so the ranks share device 0 and the collectives go over gloo;
on an 8-GPU node the same code path runs with backend nccl = RCCL)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=900, tmp=None):
    """-> the full report (written to a file by bench.py), after checking the stdout contract: the LAST stdout line is ONE compact JSON
    object of < 6 000 bytes (the driver parses that line and keeps an ~8 KB tail; a 21 KB line left BENCH_r05.parsed = null)."""
    import tempfile
    env = dict(os.environ, **(env_extra or {}))
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    full = os.path.join(tmp or tempfile.mkdtemp(), "bench_full.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full-out", full] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out_lines = r.stdout.strip().splitlines()
    lines = [l for l in out_lines if l.startswith("{")]
    assert len(lines) == 1 and out_lines[-1] == lines[0], r.stdout[-2000:]
    assert len(lines[0].encode()) < 6000, len(lines[0])
    compact = json.loads(lines[0])
    with open(full) as f:
        res = json.load(f)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "rccl_ranks"):
        assert k in compact, k
        if k != "config":
            assert compact[k] == res[k] or abs(compact[k] - res[k]) <= 1e-4 * abs(res[k]), k      # (floats are cut to 5 significant digits)
    assert set(compact["config"]) >= {"workload", "frames_per_step_per_gpu", "timed_region"}
    res["_compact"] = compact
    return res


def test_bench_contract_n1():
    res = _run(["--full", "--steps", "6", "--warmup", "2", "--profile-steps", "2", "--also-batch", "2", "--model", "vits", "--no-cpu-baseline"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "roofline_warp", "parity_class", "batched", "ingest_rank0", "rccl_ranks"):
        assert k in res, k
    assert res["n_gpus"] == 1 and res["steps"] == 6 and res["dtype"] == "bf16" and res["vs_baseline"] is None
    c = res["_compact"]                            # what the driver parses: headline + roofline + parity + one number per sub-run
    for k in ("roofline", "roofline_warp", "parity_class", "batched", "depth_l1_vs_ref", "depth_max_vs_ref", "warp_max_lsb", "kernels", "full_report"):
        assert k in c, k
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in c["roofline"], k
    assert abs(c["roofline"]["frac"] - res["roofline"]["frac"]) < 1e-4 and c["batched"]["roofline"]["frac"] > 0
    assert abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
    rf = res["roofline"]
    assert rf["bound"] in ("mfma", "hbm") and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    pc = res["parity_class"]                       # the engines that meet the 1e-3 gate: split precision (fast) and fp32
    assert pc["dtype"] == "bf16x3" and 0 < pc["fp32_engine"]["value"] < pc["value"] < res["value"]
    # the parity half of BASELINE.json's metric, from the committed reference fixtures (vits_r518, warp): the headline bf16 engine inside
    # the reference's own bf16 class, the parity-class engine inside north_star's 1e-3, the warp within 1 LSB
    assert 0 < res["depth_l1_vs_ref"] <= 0.00287 and res["depth_max_vs_ref"] <= 0.0357 and res["warp_max_lsb"] <= 1, res["parity"]
    assert pc["depth_max_vs_ref"] <= 1e-3 and res["parity"]["bf16x3"]["depth_l1_vs_ref"] <= 1e-4


def test_bench_plain_run_is_the_headline_alone():
    """The driver's plain command on the default workload: the headline and nothing after it (every other measurement is --full's)."""
    res = _run(["--gpus", "1", "--steps", "6", "--warmup", "2"])
    assert set(res) - {"_compact"} == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                       "vs_baseline", "dtype", "data", "rccl_ranks", "hip_force_dev_kernarg", "config"}
    assert res["metric"] == "stereo frames/sec @1080p DepthAnything-v2-ViT-B" and res["dtype"] == "bf16" and res["steps"] == 6
    assert abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]


def test_bench_spawns_its_own_ranks():
    res = _run(["--full", "--gpus", "2", "--steps", "4", "--warmup", "1", "--model", "vits", "--no-profile", "--no-cpu-baseline"],
               {"D2S_DIST_BACKEND": "gloo"})
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2
    assert res["ingest_rank0"]["frames_per_step"] == 2 and res["ingest_rank0"]["value"] > 0
    assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]


def test_bench_two_ranks_over_rccl():
    """`bench.py --gpus 2` over backend nccl (= RCCL) on two real devices: rank spawn, HSA_ENABLE_IPC_MODE_LEGACY=0, the rank
    count by all-reduce, the isend / irecv frame exchange of the rank-0-ingest leg.  Needs two visible GPUs (the driver's
    multi-GPU boxes); the one-GPU rehearsal of the same code path is test_bench_spawns_its_own_ranks above."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip(f"{torch.cuda.device_count()} ROCm device(s) visible: two RCCL ranks need two (covered over gloo above)")
    res = _run(["--full", "--gpus", "2", "--steps", "6", "--warmup", "2", "--model", "vits", "--no-profile", "--no-cpu-baseline"])
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2
    assert res["ingest_rank0"]["frames_per_step"] == 2 and res["ingest_rank0"]["value"] > 0
    assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]


def test_bench_refuses_more_ranks_than_gpus():
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, cwd=REPO,
                       env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "D2S_DIST_BACKEND")})
    assert r.returncode != 0 and "visible" in (r.stderr + r.stdout)
