"""Multi-GPU row on the one GPU of the test box: the library's RCCL entry points at world 1, and the
dataset driver (items sharded over ranks, lock-step groups, one all-gather) against one-by-one searches."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_comm_allgather_world1():
    """tstar_comm_unique_id / tstar_comm_create / tstar_allgather_i32 / tstar_comm_destroy through the C ABI: RCCL is
    dlopen'ed (the copy torch already carries), a 1-rank communicator is created on the current device and the gather of
    a padded keyframe buffer returns it unchanged, on the caller's stream."""
    from tstar_amd import _lib
    lib = _lib.load()
    idbuf = C.create_string_buffer(128)
    _lib.check(lib.tstar_comm_unique_id(idbuf), "tstar_comm_unique_id")
    assert any(idbuf.raw)
    h = C.c_void_p()
    _lib.check(lib.tstar_comm_create(C.byref(h), idbuf.raw, 1, 0), "tstar_comm_create")
    try:
        send = torch.tensor([[3, 17, 99, -1], [5, 6, 7, 8]], dtype=torch.int32, device="cuda")
        recv = torch.full((1, 2, 4), -7, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            _lib.check(lib.tstar_allgather_i32(h, send.data_ptr(), recv.data_ptr(), send.numel(), st.cuda_stream), "tstar_allgather_i32")
        st.synchronize()
        assert torch.equal(recv[0], send)
        assert lib.tstar_allgather_i32(h, send.data_ptr(), recv.data_ptr(), 0, None) == 1          # TSTAR_ERR_ARG
        assert lib.tstar_comm_create(C.byref(C.c_void_p()), idbuf.raw, 2, 2) == 1                   # rank out of range
    finally:
        lib.tstar_comm_destroy(h)


def test_dataset_driver_equals_one_by_one_searches(tmp_path):
    """examples/run_dataset.py (the reference's run_TStar_onDataset.py loop, sharded + lock-step) writes the reference's
    result JSON; every item's keyframes and distribution must equal a plain one-by-one search of that item with the same
    per-item sampler seed (results independent of grouping and rank count)."""
    from tstar_amd.interface_heuristic import initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.sharding import item_seed
    out = tmp_path / "res.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), "--items", "5", "--nframes", "240",
                        "--lockstep", "3", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    assert len(res) == 5
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import run_dataset as RD
    h = initialize_heuristic("owl-vit", synthetic_seed=0, max_batch=64)
    for i, item in enumerate(res):
        assert set(item) >= {"video_path", "grounding_objects", "keyframe_timestamps", "keyframe_distribution"}
        t_, c_ = RD.QUESTIONS[i % 4]
        assert item["grounding_objects"] == {"target_objects": t_, "cue_objects": c_}
        s = TStarSearcher(item["video_path"], h, list(t_), list(c_), search_nframes=8, image_grid_shape=(4, 4),
                          search_budget=1000, confidence_threshold=0.6, rng=np.random.RandomState(item_seed(2025, i)),
                          keep_visual_history=False)
        _, ts = s.search()
        assert [float(t) for t in ts] == item["keyframe_timestamps"], i
        assert s.P_history[-1] == item["keyframe_distribution"]


def test_configs2_haystack32_full_size():
    """BASELINE configs[2] at its own size on the one GPU of the test box: 32 distinct 3600-frame procedural videos
    (80 GB of HBM), 4 cycled questions, lock-step groups of 4, through run_sharded at world 1 (the N-rank driver of
    run_TStar_onDataset.py:195-211 sharded; item i -> rank i % world).  Every item's keyframes / score distribution / P
    must equal its one-by-one search (per-item sampler seed: results independent of grouping and rank count), and two
    items with different questions are teacher-forced through the CPU oracle searcher (oracle/replay.py): sampled
    seconds, score history and keyframes bit-exact."""
    import bench as B
    from oracle import replay
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.lockstep import search_lockstep
    from tstar_amd.sharding import run_sharded
    from tstar_amd.video import synthetic_video
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 100 * 2 ** 30:
        pytest.skip("needs 100 GB of free HBM for 32 resident 3600-frame videos")
    n_items, g, K = 32, 16, 8
    h = OWLInterface(synthetic_seed=0, max_batch=256)
    items = [dict(id=i, store=synthetic_video(B.N_FRAMES, B.FRAME_H, B.FRAME_W, seed=1000 + i), targets=B.QUESTIONS[i % 4][0],
                  cues=B.QUESTIONS[i % 4][1], seed=2025 + i) for i in range(n_items)]
    grouped = {}

    def group(ids):
        ss = [B.make_searcher(h, items[i], g, K) for i in ids]
        res = search_lockstep(ss)
        for i, s_, r in zip(ids, ss, res):
            grouped[i] = (s_, [int(t) for t in r[1]])
        return [grouped[i][1] for i in ids]

    rows = run_sharded(n_items, None, 1, 0, search_group=group, group_size=4)
    assert len(rows) == n_items and all(len(r) == K and r == sorted(r) for r in rows)
    assert len({tuple(r) for r in rows}) > 20                   # distinct videos / seeds: not one answer repeated
    replayed = 0
    for i in range(n_items):
        it = items[i]
        teacher = i in (1, 6)                                   # questions 1 and 2 (one target + cues / one target + one cue)
        rec = replay.Recorder(h, keep_images=False) if teacher else None
        try:
            s = B.make_searcher(h, it, g, K)
            log = []
            orig = s.sample_frames
            s.sample_frames = lambda num, _o=orig, _l=log: (lambda r: (_l.append(list(r[0])), r)[1])(_o(num))
            _, ts = s.search()
        finally:
            if rec:
                rec.restore()
        solo = [int(t) for t in ts]
        sg = grouped[i][0]
        assert solo == rows[i], (i, solo, rows[i])
        assert np.array_equal(s.score_distribution, sg.score_distribution) and s.P_history[-1] == sg.P_history[-1], i
        assert s.frames_scored == sg.frames_scored and s.iterations == sg.iterations
        if teacher:
            ref, ts_ref = replay.replay_through_oracle(rec.calls, h.texts, it["targets"], it["cues"], s.total_frame_num, g, K, 1000, 0.6,
                                                       it["seed"])
            assert [int(t) for t in ts_ref] == solo, i
            assert [x["secs"] for x in ref.trace] == log, i
            assert np.array_equal(s.score_distribution, ref.score), i
            replayed += 1
    assert replayed == 2
    del items, grouped
    torch.cuda.empty_cache()


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _bench_line(cmd, env):
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_equals_one_rank():
    """bench.py's N > 1 path as the driver launches it (torch.distributed.run, one process per rank), with two ranks
    sharing the box's one GPU over gloo (TSTAR_BENCH_BACKEND=gloo; on an 8-GPU node the same code runs over RCCL):
    item i on rank i % 2, one all-gather of the keyframe rows inside the timed region.  The gathered rows must be the
    1-rank run's rows for the same 4 items (sampler seeds are a function of the item id only)."""
    common = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-grid4", "--no-verify", "--max-batch", "64"]
    env = dict(os.environ, TSTAR_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    two = _bench_line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                       "--master-port", str(_free_port()), "bench.py", "--gpus", "2"] + common, env)
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["config"]["workload_kind"] == "haystack"
    assert two["config"]["items_total"] == 4 and two["config"]["gathered_keyframe_rows"] == 4
    assert two["config"]["collective_backend"] == "gloo" and "gloo" in two["config"]["collective_path"]
    assert two["value"] > 0 and two["roofline"]["launches_timed"] > 0 and two["roofline"]["algorithmic_bytes_per_launch"] > 0
    one = _bench_line([sys.executable, "bench.py", "--workload", "haystack", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-grid4",
                       "--no-verify", "--max-batch", "64"], dict(os.environ))
    assert one["n_gpus"] == 1 and one["config"]["gathered_keyframe_rows"] == 4
    assert one["config"]["gathered_keyframes"] == two["config"]["gathered_keyframes"]
    assert all(len(r) == 8 for r in one["config"]["gathered_keyframes"])
    assert "t0_boottime_ns" in one["config"]["timed_region"] and one["config"]["timed_region"]["t1_monotonic_ns"] > one["config"]["timed_region"]["t0_monotonic_ns"]


def _launcher_free_env():
    return {k: v for k, v in os.environ.items()
            if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_PORT", "TSTAR_BENCH_BACKEND")}


def test_bench_gpus2_typed_as_is_spawns_its_ranks():
    """`python bench.py --gpus 2 ...` with NO launcher around it (WORLD_SIZE unset) -- the way the docstring advertises the
    command and the way a driver that reuses its N = 1 invocation would call it -- starts two ranks itself
    (bench.self_spawn: torch.distributed.run on 127.0.0.1) and prints ONE line with n_gpus = 2.  On a 1-GPU box the
    two ranks share the device and gather over gloo; with two or more GPUs visible the same command goes over RCCL
    (next test)."""
    two = _bench_line([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-grid4",
                       "--no-verify", "--max-batch", "64"], _launcher_free_env())
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["config"]["items_total"] == 4
    assert two["config"]["gathered_keyframe_rows"] == 4 and all(len(r) == 8 for r in two["config"]["gathered_keyframes"])
    if torch.cuda.device_count() < 2:
        assert two["config"]["collective_backend"] == "gloo"
    else:
        assert two["config"]["collective_backend"] == "nccl" and "ncclAllGather" in two["config"]["collective_path"]


@pytest.mark.skipif(torch.cuda.device_count() != 1, reason="the duplicate-GPU failure needs ranks that share one device")
def test_rccl_that_cannot_come_up_falls_back_to_a_gloo_gather():
    """Round 6: with the RCCL gather asked for (TSTAR_BENCH_BACKEND=nccl) and two ranks on ONE GPU, ncclCommInitRank fails ("Duplicate GPU
    detected").  torch.distributed is the gloo control plane only, so nothing has to be torn down: the library's communicator is reported
    unavailable on every rank, the one gather goes over gloo, and the line comes out with the collective that actually ran.  (The previous
    torch-level fallback -- destroy the nccl process group, re-init gloo on the next port -- hung under torch.distributed.run.)"""
    env = dict(_launcher_free_env(), TSTAR_BENCH_BACKEND="nccl")
    two = _bench_line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                       "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-grid4",
                       "--no-verify", "--max-batch", "64"], env)
    c = two["config"]
    assert two["n_gpus"] == 2 and c["gathered_keyframe_rows"] == 4 and all(len(r) == 8 for r in c["gathered_keyframes"])
    assert c["collective_backend"] == "gloo" and "RCCL communicator was unavailable" in c["collective_path"] and "ncclCommInitRank" in c["collective_path"]
    assert c["control_plane"] == "torch.distributed over gloo"


def test_bench_gpus8_rehearsal_on_one_gpu():
    """Round 6 (review item 3): the 8-rank launch the driver's SCALE run makes, rehearsed on THIS box -- `python bench.py --gpus 8 ...` typed as
    is starts 8 ranks through torch.distributed.run; with one GPU visible they share the device and gather over gloo (on an 8-GPU node the same
    command puts one rank on each GPU and gathers through ncclAllGather).  One line, n_gpus = 8, the 8 gathered rows equal to the 1-rank run's
    rows for the same 8 items, the per-rank host budget and HBM figures present, and the whole launch -- 8 processes, 8 detector handles,
    8 x the spline workers -- well inside two minutes."""
    import time
    t0 = time.perf_counter()
    eight = _bench_line([sys.executable, "bench.py", "--gpus", "8", "--steps", "1", "--warmup", "1", "--max-batch", "16", "--no-cpu-baseline",
                         "--no-grid4", "--no-verify"], _launcher_free_env())
    wall = time.perf_counter() - t0
    c = eight["config"]
    assert eight["n_gpus"] == 8 and eight["scaling"] == "weak" and c["items_total"] == 8 and c["gathered_keyframe_rows"] == 8
    assert len(c["host_cpu_sec_per_video_by_rank"]) == 8 and all(v > 0 for v in c["host_cpu_sec_per_video_by_rank"])
    assert len(c["hbm_used_gib_by_rank"]) == 8 and all(1.0 < v < 288.0 for v in c["hbm_used_gib_by_rank"])
    assert all(len(r) == 8 for r in c["gathered_keyframes"]) and eight["value"] > 0
    if torch.cuda.device_count() < 8:
        assert c["collective_backend"] == "gloo" and "gloo" in c["collective_path"]
    assert wall < 240.0, wall                     # review target 120 s on a warm box; the bound leaves room for a cold page cache
    print(f"8-rank rehearsal: wall {wall:.1f} s, hbm {max(c['hbm_used_gib_by_rank']):.1f} GiB on the shared device, "
          f"host cpu/video by rank {[round(v, 2) for v in c['host_cpu_sec_per_video_by_rank']]}")
    one = _bench_line([sys.executable, "bench.py", "--workload", "haystack", "--steps", "8", "--warmup", "1", "--max-batch", "16", "--no-cpu-baseline",
                       "--no-grid4", "--no-verify"], _launcher_free_env())
    assert one["config"]["gathered_keyframes"] == c["gathered_keyframes"]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: real RCCL between two ranks")
def test_bench_gpus2_over_rccl():
    """On a multi-GPU box: the plain `python bench.py --gpus 2` command, one rank per GPU, the keyframe rows collected by
    ONE ncclAllGather on the library's own RCCL communicator (tstar_allgather_i32) with two ranks, and the gathered rows
    equal to a 1-rank run of the same four items."""
    common = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-grid4", "--no-verify", "--max-batch", "64"]
    two = _bench_line([sys.executable, "bench.py", "--gpus", "2"] + common, _launcher_free_env())
    assert two["n_gpus"] == 2 and two["config"]["collective_backend"] == "nccl"
    assert "ncclAllGather" in two["config"]["collective_path"] and "2 ranks" in two["config"]["collective_path"]
    one = _bench_line([sys.executable, "bench.py", "--workload", "haystack", "--steps", "4", "--warmup", "1", "--no-cpu-baseline",
                       "--no-grid4", "--no-verify", "--max-batch", "64"], _launcher_free_env())
    assert one["config"]["gathered_keyframes"] == two["config"]["gathered_keyframes"]
    assert len(two["config"]["host_cpu_sec_per_video_by_rank"]) == 2


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: one JSON line with the headline keys and
    none of the --full records, and DIR holds what the last timed search returned to its caller (float32 / float64, 64 MB at most):
    its keyframe time stamps (= the last gathered keyframe row), the K frames, the searcher's score and keyframe distributions.
    Two runs with the same arguments write the same arrays."""
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        runs.append((_bench_line([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                                 dict(os.environ)), out))
    d, out = runs[0]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline"):
        assert k in d, k
    c = d["config"]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["value"] > 1000
    assert "frames scored/sec" in d["metric"] and "3 bf16 terms" in d["dtype"]
    assert abs(d["ms_per_step"] * 1e-3 - c["sec_per_video"]) < 1e-9 and len(c["gathered_keyframes"]) == 3
    assert "cpu_baseline" not in d and not {"grid4", "drop_in", "other_configs", "f32_native"} & set(c)
    assert c["keyframes_verified"] is None and c["single_search_alone_latency_sec"] is None
    names = ("keyframe_timestamps", "keyframes", "score_distribution", "keyframe_distribution")
    assert sorted(p.name for p in out.iterdir()) == sorted(n + ".npy" for n in names)
    arrs = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert [int(t) for t in arrs["keyframe_timestamps"]] == c["gathered_keyframes"][-1]
    kf = arrs["keyframes"]
    assert kf.shape == (8, 360, 640, 3) and kf.dtype == np.float32 and kf.min() >= 0 and kf.max() <= 255 and np.array_equal(kf, np.round(kf))
    assert arrs["score_distribution"].shape == arrs["keyframe_distribution"].shape == (3600,) and arrs["score_distribution"].max() > 0
    for n in names:
        assert np.array_equal(arrs[n], np.load(runs[1][1] / (n + ".npy"))), n


def test_bench_line_contract():
    """`python bench.py --full --steps K --warmup W` at N = 1: exactly one JSON line on stdout with the
    contract's keys, the roofline and cpu_baseline objects, self-consistent figures (value = frames / time, the time shares
    below 1, achieved below the peak) and the keyframes of the timed region verified through the oracle."""
    d = _bench_line([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "3", "--no-grid4"],
                    dict(os.environ))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "frames/s" and "3 bf16 terms" in d["dtype"] and d["dtype"].startswith("f32") and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "frames scored/sec" in d["metric"] and "configs[1]" in d["config"]["workload"] and "model" not in d["config"]
    c, r, b = d["config"], d["roofline"], d["cpu_baseline"]
    assert abs(d["ms_per_step"] * 1e-3 - c["sec_per_video"]) < 1e-9 and d["value"] > 1000
    assert c["keyframes_verified"] is True and len(c["keyframes_rank0_step0"]) == 8 and c["lockstep_groups_alternating"] == 2
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "launches_timed", "launches_total",
              "avg_launch_ms", "time_share_of_step", "achieved_algorithmic"):
        assert k in r, k
    # round 5: the headline runs the f32x3 mode (exact three-term operands on the bf16 matrix pipe): priced against the dense bf16 peak,
    # executed = 6 x algorithmic
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0 and 0.4 < r["frac"] < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and abs(r["achieved"] - 6.0 * r["achieved_algorithmic"]) < 1e-6 * r["achieved"]
    # round 6: one definition per number -- executed vs algorithmic fraction, the scheme's ceiling, and a traffic ratio only across ONE
    # launch population (this 3-step run is not the 16-step population of the PMC collection: null, with the reason)
    assert r["frac_executed"] == r["frac"] and r["executed_over_algorithmic"] == 6.0 and abs(r["scheme_ceiling_tflops"] - 2500.0 / 6) < 1e-9
    assert abs(r["frac_algorithmic"] - r["achieved_algorithmic"] / r["peak"]) < 1e-12 and abs(r["frac_algorithmic"] * 6.0 - r["frac"]) < 1e-9
    assert abs(r["achieved_algorithmic"] / r["scheme_ceiling_tflops"] - r["frac"]) < 1e-9 and "executed" in r["frac_definition"]
    assert r["traffic"] is None and r["traffic_over_algorithmic"] is None and ("population" in r["traffic_note"] or "PMC" in r["traffic_note"])
    assert c["population"]["steps"] == 3 and c["population"]["weights"] == "f32x3" and c["population"]["lockstep"] == 8
    assert abs(r["gemm_plus_attention_time_share_of_step"] - r["time_share_of_step"] - r["attention_kernel"]["time_share_of_step"]) < 1e-12
    assert r["launches_total"] >= r["launches_timed"] * (r["timed_every_nth_launch"] - 1) and r["launches_timed"] > 0
    assert 0.5 < r["time_share_of_step"] + r["attention_kernel"]["time_share_of_step"] < 1.0
    assert "attention_x3" in r["attention_kernel"]["kernel"]
    assert b["kind"] == "port" and b["cores"] >= 1 and 1 < b["value"] < d["value"] and b["unit"] == "frames/s" and b["sample"]
    # round 6: the reference's per-call debug PNG (interface_heuristic.py:248-256) reported separately, never inside `value`
    png = b["png_write_sec_per_call"]
    assert png["grid"] > png["verify"] > 0 and png["grid_image"] == "3200x1520" and png["verify_image"] == "600x285"
    assert b["with_png"]["sec_per_video"] > b["sec_per_video"] and b["with_png"]["value"] < b["value"] and "decord" in b["decode_note"]
    # round 6: what an UNCHANGED TStarFramework gets (default-constructed heuristic, one 4x4 search alone, history ON), both modes
    di = c["drop_in"]
    assert "error" not in di, di
    for m in ("f32", "f32x3"):
        assert 0.05 < di[m]["sec_per_video"] < 5 and di[m]["grid_calls"] == 63 and di[m]["history_entries"] >= 63 and len(di[m]["keyframes"]) == 8
        assert di[m]["max_batch"] == 32
    assert di["f32"]["env"]["TSTAR_WEIGHTS_DTYPE"] is None and di["f32x3"]["env"]["TSTAR_WEIGHTS_DTYPE"] == "f32x3"
    assert di["sec_per_video"] == di["f32x3"]["sec_per_video"] < di["f32"]["sec_per_video"]
    # round 4: the host budget of a rank (what predicts the 8-rank curve), the visual-history statement, and the other BASELINE
    # configs observed through the same line
    assert c["visual_history"] is False and c["host_cores"] >= 1 and 0 < c["host_cpu_sec_per_video"] < 60 and c["host_cpu_busy_cores"] > 0
    oc = c["other_configs"]
    assert len(oc) == 3
    for name, rec in oc.items():
        assert "error" not in rec, (name, rec)
        assert rec["keyframes_verified"] is True and rec["value"] > 1000 and 0 < rec["roofline"]["frac"] < 1, (name, rec)
    y = [v for k, v in oc.items() if "configs[3]" in k][0]
    assert y["roofline"]["bound"] == "valu" and "configs[3]" in y["workload"]
    assert "VALU" in y["dtype"] and "no MFMA" in y["dtype"] and "bf16" not in y["dtype"] and y["roofline"]["executed_over_algorithmic"] == 1.0
    c5 = [v for k, v in oc.items() if "configs[4]" in k][0]
    assert "14400-frame" in c5["workload"] and "search_nframes=32" in c5["workload"] and "bf16" in c5["dtype"]
    nat = [v for k, v in oc.items() if "native f32" in k][0]
    assert nat["dtype"] == "f32" and nat["roofline"]["peak"] == 157.3
    # the native-f32 figure of the same workload stays in the line next to the headline
    assert c["f32_native"]["value"] == nat["value"] and c["f32_native"]["keyframes_verified"] is True and c["f32_native"]["headline_over_native"] > 1.0
