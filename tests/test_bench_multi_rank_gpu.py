"""SURVEY.md 8(e) / VERDICT r03 #7: `bench.py --gpus 2` end to end as the driver launches it (one process per rank under
torch.distributed.run), rehearsed on the ONE GPU of the test box: FHIP_BENCH_SHARE_GPU=1 puts both ranks on cuda:0 and the collectives on gloo,
so the N > 1 code path -- model broadcast from rank 0, barriers, max-over-ranks timing, config 5's global batch of 512 split over the ranks,
the shard check -- runs for real.  Its throughput numbers mean nothing and are not asserted."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env, tmp_path):
    detail = str(tmp_path / "detail.json")
    out = subprocess.run(cmd + ["--detail-out", detail], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return out, detail


def _line(out, only_line=False):
    lines = [ln for ln in out.stdout.splitlines() if (ln.strip() if only_line else ln.startswith("{"))]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-2000:]  # rank 0 prints ONE JSON line, the other ranks none
    assert len(lines[0].encode()) <= 8192, len(lines[0])  # the driver must be able to parse it
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu(cuda, tmp_path):
    from feathercnn_amd import model_zoo
    env = dict(os.environ, FHIP_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-steady", "--no-cpu-baseline", "--full"]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out)
    d = json.load(open(detail))
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["warmup"] == 1 and r["scaling"] == "weak" and r["value"] > 0
    assert r["config"]["global_batch"] == 64 and r["config"]["per_gpu_batch"] == 32            # VGG-16, 32 per GPU, weak
    g512 = d["nets"]["resnet50_global512"]
    assert g512["global_batch"] == 512 and g512["scaling"] == "strong" and g512["per_gpu_batch"] == 256
    assert d["nets"]["resnet50"]["scaling"] == "weak" and d["nets"]["resnet50"]["global_batch"] == 128
    # the one collective of the path: the .bin of the headline net, broadcast once from rank 0
    assert r["weight_broadcast"]["bytes"] == len(model_zoo.MODELS["vgg16"]()[1])
    # rank 1's results on its shard equal rank 0's on the same images (src/layers/conv_layer.h:107: images are independent)
    sc = r["shard_check"]
    assert sc["ok"] and sc["global_batch"] == 5 and sc["shares"] == [3, 2] and sc["max_norm_err"] <= 1e-5, sc
    assert "cpu_baseline" not in r and r["roofline"]["frac"] > 0 and len(r["roofline"]["frac_passes"]) >= 5


@pytest.mark.gpu
def test_bench_gpus_flag_starts_the_ranks_itself(cuda, tmp_path):
    """plain `python bench.py --gpus 2` -- no torch.distributed.run in front -- must start two ranks by itself (launch_ranks) and
    print one JSON line with n_gpus == 2; the same one-GPU rehearsal switch.  The compact per-net summary sits inside `config` and `roofline`,
    and both scaling efficiencies of config 5 are in the line with their definitions."""
    from feathercnn_amd import model_zoo
    env = dict(os.environ, FHIP_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-steady", "--no-cpu-baseline", "--full"]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out, only_line=True)  # the launcher's stdout is rank 0's JSON line and nothing else
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["value"] > 0
    assert r["shard_check"]["ok"] and r["weight_broadcast"]["bytes"] == len(model_zoo.MODELS["vgg16"]()[1])
    other = r["config"]["other_nets"]
    assert other["resnet50_g512"]["img_s"] > 0 and other["resnet50_b64"]["img_s"] > 0 and other["resnet50_g512_one_gpu"]["img_s"] > 0
    assert other["resnet50_b64_one_gpu"]["img_s"] > 0 and other["vgg16_b32_one_gpu"]["img_s"] > 0
    sc = other["resnet50_scaling"]
    assert sc["strong_eff"] > 0 and sc["weak_eff"] > 0 and sc["predicted_strong_eff_at_8_gpus"] > 0 and sc["strong_def"] and sc["weak_def"]
    assert r["roofline"]["also"]["vgg16_b32"][0]["kernel"] == "tile_gemm"
    assert json.load(open(detail))["nets"]["resnet50_global512"]["expected_from_1gpu"]["n_gpus"] == 2


@pytest.mark.gpu
def test_bench_eight_ranks_rehearsal_on_one_gpu(cuda, tmp_path):
    """the REAL 8-rank shape -- launcher, port choice, eight per-rank arenas, config 5 split 64 per rank, the 17-image ragged
    shard check, the line size -- one rank per GPU over RCCL.  (The name is kept from its first form, which put all eight ranks on one GPU:
    eight rank processes plus the test and the launcher hold one device at once, more than a shared test machine admits.)  On one GPU,
    test_bench_three_ranks_rehearsal_on_one_gpu rehearses an N > 2 run within that bound; tests/test_bench_report_cpu.py checks the N = 8
    line and tests/test_distributed_cpu.py the 8-way shard arithmetic."""
    import torch
    have = torch.cuda.device_count()
    if have < 8:
        pytest.skip(f"needs 8 GPUs, found {have}")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FHIP_BENCH_SHARE_GPU", None)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--no-steady", "--no-cpu-baseline", "--full"]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out, only_line=True)
    assert r["n_gpus"] == 8 and r["scaling"] == "weak" and r["value"] > 0 and r["config"]["global_batch"] == 256
    sc = r["shard_check"]
    assert sc["ok"] and sc["global_batch"] == 17 and sum(sc["shares"]) == 17 and len(sc["shares"]) == 8 and sc["max_norm_err"] <= 1e-5, sc
    other = r["config"]["other_nets"]
    assert other["resnet50_g512"]["per_gpu_batch"] == 64 and other["resnet50_g512"]["img_s"] > 0   # config 5 as the 8-GPU node will run it
    assert other["resnet50_b64"]["per_gpu_batch"] == 64 and other["resnet50_g512_one_gpu"]["per_gpu_batch"] == 512
    s8 = other["resnet50_scaling"]
    assert s8["n_gpus"] == 8 and s8["strong_eff"] > 0 and s8["weak_eff"] > 0
    d = json.load(open(detail))
    assert d["nets"]["resnet50_global512"]["global_batch"] == 512 and d["nets"]["resnet50"]["global_batch"] == 512


@pytest.mark.gpu
def test_bench_three_ranks_rehearsal_on_one_gpu(cuda, tmp_path):
    """An N > 2 run rehearsed on one GPU (FHIP_BENCH_SHARE_GPU=1, every rank on cuda:0, collectives over gloo) with a process count a shared
    machine admits (the test, the torch.distributed.run agent and three ranks): three per-rank arenas, config 5's 512 images split RAGGED
    over the ranks (171 / 171 / 170), the 7-image ragged shard check, both scaling efficiencies, and the line."""
    env = dict(os.environ, FHIP_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "2", "--warmup", "1", "--no-steady", "--no-cpu-baseline", "--full"]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out)
    assert r["n_gpus"] == 3 and r["steps"] == 2 and r["scaling"] == "weak" and r["value"] > 0 and r["config"]["global_batch"] == 96
    sc = r["shard_check"]
    assert sc["ok"] and sc["global_batch"] == 7 and sc["shares"] == [3, 2, 2] and sc["max_norm_err"] <= 1e-5, sc
    other = r["config"]["other_nets"]
    assert other["resnet50_g512"]["per_gpu_batch"] == 171 and other["resnet50_g512"]["img_s"] > 0   # rank 0's share of config 5
    assert other["resnet50_b64"]["per_gpu_batch"] == 64 and other["resnet50_g512_one_gpu"]["per_gpu_batch"] == 512
    s3 = other["resnet50_scaling"]
    assert s3["n_gpus"] == 3 and s3["strong_eff"] > 0 and s3["weak_eff"] > 0
    d = json.load(open(detail))
    assert d["nets"]["resnet50_global512"]["global_batch"] == 512 and d["nets"]["resnet50"]["global_batch"] == 192


@pytest.mark.gpu
def test_bench_gpus_flag_must_agree_with_the_launcher(cuda):
    """--gpus 4 under a launcher that started 2 ranks: refused before anything is measured (the flag can never disagree with the run)."""
    env = dict(os.environ, FHIP_BENCH_SHARE_GPU="1", WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    assert out.returncode != 0 and "must agree" in out.stderr


@pytest.mark.gpu
def test_bench_single_rank_line_is_compact_and_complete(cuda, tmp_path):
    """The N = 1 form of the driver's command with --full (shortened: headline net only, no CPU leg): ONE stdout line of at most 8 KiB that json.loads, with the contract keys,
    `roofline` carrying the spread of its 7 attribution passes, and everything long in the detail side file the line names."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FHIP_BENCH_SHARE_GPU"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--headline-only", "--no-steady", "--no-cpu-baseline", "--full"]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out, only_line=True)
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0 and r["dtype"] == "f32" and r["vs_baseline"] is None
    assert r["config"]["net"] == "vgg16" and r["config"]["per_gpu_batch"] == 32 and r["detail"] == detail
    ro = r["roofline"]
    assert ro["bound"] == "mfma" and len(ro["frac_passes"]) == 7 and ro["frac_min"] <= ro["frac"] <= ro["frac_max"] and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 2e-3
    d = json.load(open(detail))
    assert len(d["tables"]["vgg16"]) >= 15 and d["rooflines"]["vgg16"][0]["note"]


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_only(cuda, tmp_path):
    """The driver's plain command (no --full): the headline net alone is timed -- its contract keys and `config` in ONE line, and none of what
    --full adds (other nets, roofline, CPU baseline, calibration).  --dump-outputs still writes the array of every net --full times."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FHIP_BENCH_SHARE_GPU"):
        env.pop(k, None)
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)]
    out, detail = _run(cmd, env, tmp_path)
    r = _line(out, only_line=True)
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0 and r["ms_per_step"] > 0 and r["dtype"] == "f32"
    assert r["metric"] == "images/sec fp32 forward @224x224" and r["unit"] == "images/s" and r["higher_is_better"] is True
    assert r["config"]["net"] == "vgg16" and r["config"]["per_gpu_batch"] == 32 and r["config"]["workload"] and r["config"]["other_nets"] == {}
    assert not {"roofline", "cpu_baseline", "mfma_calibration", "shard_check"} & set(r)
    assert list(json.load(open(detail))["nets"]) == ["vgg16"]
    assert sorted(os.listdir(dump)) == ["mobilenet_v1.npy", "resnet50.npy", "resnet50_global512.npy", "vgg16.npy"]


@pytest.mark.gpu
def test_bench_dump_outputs_are_what_the_timed_net_computed(cuda, tmp_path):
    """--dump-outputs: the .npy bench.py writes is the output blob of its last timed step -- the same numbers a caller gets from a Net of the
    same model, settings and seeded input (MobileNet-V1 runs as two sub-batch replicas: the dump is the whole batch)."""
    import numpy as np
    import torch

    from feathercnn_amd import model_zoo
    from feathercnn_amd.net import Net
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FHIP_BENCH_SHARE_GPU"):
        env.pop(k, None)
    dump = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--net", "mobilenet_v1", "--batch", "4",
           "--no-steady", "--no-cpu-baseline", "--dump-outputs", str(dump)]
    out, _ = _run(cmd, env, tmp_path)
    r = _line(out, only_line=True)
    assert r["steps"] == 2 and r["config"]["per_gpu_batch"] == 4
    assert os.listdir(dump) == ["mobilenet_v1.npy"]
    got = np.load(dump / "mobilenet_v1.npy")
    assert got.dtype == np.float32 and got.shape == (4, 1000, 1, 1)
    p, b, i, o = model_zoo.MODELS["mobilenet_v1"]()
    gen = torch.Generator(device=cuda)
    gen.manual_seed(4321)  # benchkit.timing.measure_net's input of rank 0
    x = torch.rand((4, 3, 224, 224), device=cuda, generator=gen) * 2 - 1
    net = Net(fusion=3, graph=True, tuned=True, concurrency=True, sub_batches=2)  # what bench.py builds by default
    net.LoadParam(p)
    net.LoadWeights(b)
    net.FeedInput(i, x)
    net.Forward()
    want = net.Extract(o)
    net.close()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    np.testing.assert_allclose(got.reshape(4, -1).sum(axis=1), 1.0, atol=1e-3)
