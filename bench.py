#!/usr/bin/env python
"""bench.py -- T* keyframe-search hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

(with N > 1 and no launcher around it, i.e. WORLD_SIZE unset, the command starts its own N ranks through
torch.distributed.run on 127.0.0.1 -- self_spawn(); under the driver's launcher it is one of the ranks.)

One "step" = one complete keyframe search (TStarSearcher.search(): iterative sampling, grid
scoring, verification, distribution updates, final K=8 keyframes) over one 3600-frame
synthetic video that is already resident in HBM -- BASELINE.json configs[1]: "Same single
video on 1xMI355X, HIP OWL-ViT-B/32 scorer, batch=256 frames/iter" (grid 16x16).  With N > 1
(one rank per GPU; torch.distributed over gloo as the control plane, the one data collective over RCCL) the workload is BASELINE configs[2]'s shape: every
step is its own (video, question) item -- a distinct procedural video, one of four questions --
item i on rank i % N (weak scaling, no data-path collective), and the final keyframe indices are
all-gathered once inside the timed region through the library's own RCCL entry point
(tstar_allgather_i32).  --workload haystack32 runs exactly configs[2] (32 items).  Within a rank, items advance in
lock-step groups of --lockstep (default 8): iteration t of every item of the group shares one
detector batch, each image scored against its own question (tstar_amd/lockstep.py); results are
bit-identical to one-by-one searches.

Prints ONE JSON line on rank 0.  value = candidate frames scored / s over all ranks; a frame
is scored each time it contributes a confidence to the searcher: g*g per grid call + 1 per
verification call.  Weights are seeded synthetic OWL-ViT-B/32 (no checkpoint
offline), data synthetic.

A plain run does only what that line's headline needs: set up, warm up, time --steps searches, write
--dump-outputs DIR (the last timed search's results as .npy; the same arguments give the same inputs),
print the line.  --full adds everything else, all of it after the timed region: the single-search
latency, the oracle replay of the timed keyframes, config.grid4, config.drop_in, config.other_configs
and the CPU baseline.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROF_STRIDE = 5
BF16_MFMA_PEAK_TFLOPS = 2500.0        # dense bf16 MFMA peak (same guide)
FP32_MFMA_PEAK_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
N_FRAMES, FRAME_H, FRAME_W = 3600, 360, 640
TARGETS, CUES = ["couch"], ["tv", "chair"]
# questions of the haystack workload (BASELINE configs[2]: independent (video, question) items); item i asks QUESTIONS[i % 4]
QUESTIONS = [(["couch"], ["tv", "chair"]), (["dog"], ["leash", "park bench"]), (["red car"], ["road"]),
             (["laptop", "mug"], ["desk"])]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps = searched videos per rank; default 16 (two lock-step groups of 8), 48 with --heuristic yolo (two groups of 24)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=int, default=16, help="grid side g (g*g frames per iteration)")
    ap.add_argument("--max-batch", type=int, default=512,
                    help="detector images per forward chunk (workspace size; NOT the 256 frames per iteration of configs[1], which is the 16x16 grid): "
                         "a lock-step group of 8 verifies ~360 frames per iteration, one chunk at 512 instead of 256 + ~104 "
                         "(11.81 k vs 11.69 k frames/s same-box, profiles/r05_owl_maxbatch_sweep.log)")
    ap.add_argument("--yolo-max-batch", type=int, default=76,
                    help="YOLO-World backend: detector images per forward chunk.  Sized for the chip, not a power of two: the halo conv "
                         "kernel holds 3 workgroups per CU (768 slots) and a 40x40 / 256-channel layer is 20 B workgroups, an 80x80 / 128 "
                         "layer 40 B, a 160x160 / 64 layer 80 B -- B = 38 fills exactly 1 / 2 / 4 rounds, 76 twice that (B = 32 leaves a "
                         "sixth of the slots idle: 84.7 vs 91.8 / 98.3 TFLOP/s per forward, tools/yolo_batch_sweep.py); with 24 searches "
                         "in lock-step an iteration verifies about 228 frames = three chunks of 76 (+ a small remainder)")
    ap.add_argument("--nframes", type=int, default=N_FRAMES)
    ap.add_argument("--search-nframes", type=int, default=8)
    ap.add_argument("--weights", choices=["f32", "bf16", "bf16_exact", "f32x3"], default="f32x3",
                    help="f32x3 (default since round 5) = the fp32 checkpoint on the bf16 matrix pipe with every GEMM / attention operand carried as THREE "
                         "exact bf16 terms (all 24 significand bits), the six partial products with i + j <= 2, f32 accumulation: error vs float64 no "
                         "larger than the native f32 MFMA kernels' (asserted in tests/test_gpu_kernels.py), detector parity at the same 5e-5 bound; "
                         "f32 = the native v_mfma_f32_32x32x2_f32 tiles of rounds 1-4 (reported beside the headline as config.f32_native); "
                         "bf16 = BASELINE config 5 (bf16-rounded weights on the bf16 matrix pipe, f32 activations as two bf16 terms: "
                         "2 MFMA products per algorithmic product); with --nframes 14400 --grid 15 --search-nframes 32 this is "
                         "configs[4].  bf16_exact = the same weights with the activations split exactly into three terms (3 products)."
                         )
    ap.add_argument("--concurrency", type=int, default=1,
                    help="independent searches in flight per GPU (host threads, one HIP stream + one scorer "
                         "workspace each); 2 fills kernel tails and gives ~+5 %% throughput, but overlapping "
                         "launches inflate per-launch durations, so the roofline leg is reported at 1")
    ap.add_argument("--lockstep", type=int, default=0,
                    help="independent (video, question) items advanced in lock-step per detector batch "
                         "(tstar_amd.lockstep; results identical to one-by-one searches); 1 = one at a time; default 8 "
                         "with the OWL-ViT backend (round 5, f32x3 mode: 11.70 k frames/s against 11.51 k at 4 in a same-box sweep, "
                         "profiles/r05_owl_pipeline_sweep.log; rounds 1-4 used 4), 24 with YOLO-World (its grid forwards run at B = the group size: 57 TFLOP/s at 8, "
                         "72 at 16, 84 at 24, and an iteration's ~228 verification frames fill three full chunks of 76: 12.3 k frames/s "
                         "against 12.05 k at 16 and 12.15 k at 31 in a same-box A/B; --steps defaults to 48 there)")
    ap.add_argument("--pipeline", type=int, default=2,
                    help="lock-step groups alternating on the GPU (tstar_amd.lockstep.search_lockstep_groups): while the detector runs "
                         "one group's verification batch the host does the other group's bookkeeping; one stream of detector work, "
                         "results identical to running the groups one after another; 1 = one group at a time")
    ap.add_argument("--heuristic", choices=["owl", "yolo"], default="owl",
                    help="detector backend: owl = OWL-ViT-B/32 (configs[1], the headline); yolo = YOLO-World-v2-L on the f32 VALU, no "
                         "MFMA (BASELINE configs[3]; parity of that model is unpinned: its source is not in the reference tree)")
    ap.add_argument("--workload", choices=["auto", "single", "haystack", "haystack32"], default="auto",
                    help="single = BASELINE configs[1]: every step searches the SAME resident video with its own sampler seed; "
                         "haystack = configs[2] shape: every step is its own (video, question) item -- a distinct procedural "
                         "video and one of 4 questions, item i on rank i %% world, --steps items per rank (weak scaling); "
                         "haystack32 = exactly configs[2]: 32 items in total over the ranks (--steps is ignored); "
                         "auto = single on 1 GPU, haystack on more")
    ap.add_argument("--questions", choices=["auto", "same", "cycle"], default="auto",
                    help="haystack items ask: same = the configs[1] question for every item (per-item work as in `single`, so "
                         "the 1/2/4/8-GPU weak-scaling points are comparable); cycle = 4 different questions (several query sets "
                         "resident, 1-2 targets each; with the synthetic weights most cells then list a target and 3-4x more frames "
                         "go through verification); auto = same for haystack, cycle for haystack32")
    ap.add_argument("--no-verify", action="store_true", help="skip the post-run oracle replay of step 0's keyframes")
    ap.add_argument("--no-grid4", action="store_true",
                    help="skip the config.grid4 sub-record (the reference's DEFAULT 4x4 grid, where 'sec/video' is what a user of "
                         "the reference sees: one solo search and 16 videos in lock-step, untimed by the driver)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip config.other_configs: after the timed region of the DEFAULT line (N = 1, OWL-ViT, f32x3, configs[1]) bench.py runs "
                         "itself three more times -- configs[3] (YOLO-World, 48 steps), configs[4] (bf16 weights, 14400 frames, K = 32, grid 15) "
                         "and configs[1] on the native f32 MFMA tiles (config.f32_native) -- and embeds value / roofline / keyframes_verified of each, so that the driver "
                         "observes them too (about +70 s, none of it inside the timed region)")
    ap.add_argument("--no-drop-in", action="store_true",
                    help="skip config.drop_in: what a user of the UNCHANGED TStarFramework gets -- the heuristic default-constructed by "
                         "initialize_heuristic('owl-vit') (mode from TSTAR_WEIGHTS_DTYPE), ONE search alone at the reference's 4x4 grid, K = 8, "
                         "visual history ON, the process-global numpy generator -- in the native-f32 and the f32x3 mode (about +8 s, untimed)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", choices=["full", "sample"], default="full",
                    help="full (default) = besides the sampled figure, ONE complete reference-faithful search of the workload is run and MEASURED on the "
                         "host cores (about 25-40 s at configs[1]; OWL-ViT backend, single-video workload); cpu_baseline.value is then the measured one "
                         "and the sampled extrapolation stays beside it; sample = the bounded sample only (rounds 1-4)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="budget for the CPU baseline sample")
    ap.add_argument("--full", action="store_true",
                    help="also run everything the headline figure does not need, after the timed region: the single-search latency, the oracle "
                         "replay of the timed keyframes (config.keyframes_verified), config.grid4, config.drop_in, config.other_configs and the CPU "
                         "baseline.  The --no-* options above switch single parts of it off.  Without --full a run sets up, warms up, times "
                         "--steps searches, writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed region, write what the last timed search returned to its caller (rank 0) as DIR/<name>.npy: "
                         "keyframe_timestamps (float64 [K]), keyframes (the K frames, float32 [K, H, W, 3]; a fixed seeded sample of "
                         "its elements when the whole would pass 64 MB), score_distribution and keyframe_distribution (the searcher's "
                         "score_distribution and P, float64 [nframes]).  The same arguments give the same inputs, run after run")
    args = ap.parse_args()
    if args.lockstep <= 0:
        args.lockstep = 24 if args.heuristic == "yolo" else 8
    if args.steps is None:
        args.steps = 48 if args.heuristic == "yolo" else 16
    return args


def make_searcher(heuristic, item, g, k=8):
    """``item``: dict(store=FrameStore, targets=, cues=, seed=sampler seed)."""
    from tstar_amd.interface_searcher import TStarSearcher
    return TStarSearcher(video_path=item["store"], heuristic=heuristic, target_objects=list(item["targets"]),
                         cue_objects=list(item["cues"]), search_nframes=k, image_grid_shape=(g, g), search_budget=1000,
                         confidence_threshold=0.6, rng=np.random.RandomState(item["seed"]), keep_visual_history=False)


def run_group(heuristic, items, g, k=8):
    """One lock-step group of independent (video, question) searches (a single search when len(items) == 1)."""
    return run_groups(heuristic, [items], g, k)[0]


def run_groups(heuristic, groups, g, k=8):
    """Lock-step groups of independent (video, question) searches, the groups alternating on the GPU
    (tstar_amd.lockstep.search_lockstep_groups); per group [(searcher, time_stamps, keyframes)]."""
    from tstar_amd.lockstep import search_lockstep_groups
    sss = [[make_searcher(heuristic, it, g, k) for it in items] for items in groups]
    if len(sss) == 1 and len(sss[0]) == 1:
        s_ = sss[0][0]
        frames, ts = s_.search()
        return [[(s_, ts, frames)]]
    res = search_lockstep_groups(sss)
    return [[(s_, r[1], r[0]) for s_, r in zip(ss, rr)] for ss, rr in zip(sss, res)]


def verify_keyframes(heuristic, item, g, k, timed_keyframes):
    """Post-run check (outside the timed region): item 0 of rank 0 is searched once more ALONE with a recorder on the
    scorer; its keyframes must equal the ones the timed (lock-step) run produced, and the recorded confidences replayed
    through the CPU oracle searcher (oracle/replay.py: the reference's loop restated, pinned by goldens) must yield the
    same sampled seconds and the same keyframes.  Returns (verified, detail)."""
    from oracle import replay
    rec = replay.Recorder(heuristic, keep_images=False)
    try:
        s = make_searcher(heuristic, item, g, k)
        log = []
        orig = s.sample_frames
        s.sample_frames = lambda num: (lambda r: (log.append(list(r[0])), r)[1])(orig(num))
        _, ts = s.search()
    finally:
        rec.restore()
    solo = [int(t) for t in ts]
    ref, ts_ref = replay.replay_through_oracle(rec.calls, heuristic.texts, item["targets"], item["cues"], s.total_frame_num, g, k,
                                               1000, 0.6, item["seed"])
    ok = (solo == list(timed_keyframes) and [int(t) for t in ts_ref] == solo and [it["secs"] for it in ref.trace] == log
          and np.array_equal(s.score_distribution, ref.score))
    return ok, {"timed": list(timed_keyframes), "solo_rerun": solo, "oracle_replay": [int(t) for t in ts_ref],
                "iterations": len(log), "verification_calls": int(sum(len(it["verify"]) for it in ref.trace))}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, last):
    """--dump-outputs: what the last timed search handed its caller, as float32 / float64 .npy files (rank 0).  ``last`` is one entry of
    run_many's result, (searcher, time_stamps, seconds, keyframes).  The searcher's state arrays are read after the timed region (a caller
    reads them the same way once search() has returned).  Keyframes past DUMP_MAX_BYTES are cut to a fixed seeded sample of elements."""
    s_, ts, _, frames = last
    arrays = {"keyframe_timestamps": np.asarray(ts, dtype=np.float64),
              "score_distribution": np.asarray(s_.score_distribution, dtype=np.float64),
              "keyframe_distribution": np.asarray(s_.P, dtype=np.float64)}
    budget = (DUMP_MAX_BYTES - sum(a.nbytes for a in arrays.values())) // 4
    kf = np.asarray(frames).reshape(-1)
    if kf.size > budget:
        kf = kf[np.sort(np.random.RandomState(0).randint(0, kf.size, budget))]
    else:
        kf = np.asarray(frames)
    arrays["keyframes"] = kf.astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def grid4_record(heuristic, store, nframes, k):
    """The reference's DEFAULT configuration (TStarFramework.py:34-35: grid 4x4, 16 frames per iteration, <= 63 iterations
    per video) on the same video and question, outside the driver-timed region: one search ALONE (the latency a single
    user sees) and 16 searches in lock-step (SURVEY.md 8d's "16 grid images of 4x4 per launch")."""
    import torch
    g = 4
    item = lambda seed: dict(store=store, targets=TARGETS, cues=CUES, seed=seed)
    run_group(heuristic, [item(30_000)], g, k)                         # first-use costs of the 380x800 shapes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solo = run_group(heuristic, [item(30_001)], g, k)
    torch.cuda.synchronize()
    t_solo = time.perf_counter() - t0
    t0 = time.perf_counter()
    # two lock-step groups of 16 alternating on the GPU (tstar_amd.lockstep.search_lockstep_groups)
    grps = run_groups(heuristic, [[item(31_000 + 16 * j + i) for i in range(16)] for j in range(2)], g, k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    grp = [x for gr in grps for x in gr]
    nv = len(grp)
    frames = sum(s_.frames_scored for s_, *_ in grp)
    return {"grid": "4x4 (16 frames/iter, the reference default)", "lockstep16_frames_per_s": frames / dt, "lockstep16_sec_per_video": dt / nv,
            "lockstep16_videos": nv, "lockstep16_groups_alternating": 2,
            "solo_sec_per_video": t_solo, "solo_frames_per_s": solo[0][0].frames_scored / t_solo,
            "grid_calls_per_video": sum(s_.iterations for s_, *_ in grp) / nv,
            "verify_calls_per_video": sum(s_.detector_calls - s_.iterations for s_, *_ in grp) / nv,
            "solo_bound": "kernel throughput at small batch: per iteration a B ~ 9.5 verification forward (M ~ 5500: 146-186 TFLOP/s algorithmic on its GEMMs, "
                          "~0.62 ms an image against 0.55 ms in the lock-step bench) and a B = 1 grid forward (M = 577: 120-456 wave tiles per GEMM for 1024 SIMDs, "
                          "2.06 ms alone), 63 iterations, 670 detector images.  Round 5 ran them back to back on one stream (593 ms of kernels in a 580 ms "
                          "search); since round 6 the NEXT iteration's grid forward runs BESIDE the verification batch on its own stream and detector workspace "
                          "(tstar_owl_score_lane) and the next verification batch is queued behind the running one before its results are read "
                          "(tstar_amd/lockstep.py: speculate / verify_ahead): 0.571 -> 0.510 s same-box (profiles/r06_solo_grid4_ab.md).  The verification "
                          "batch's own kernels already fill most of the 512 block slots, so the small forward mostly shares the chip with them; what is left "
                          "is tile efficiency at M = 577 / M ~ 5500, which only split-K would change -- and split-K makes result bits depend on the batch size"}


def drop_in_record(store, k):
    """What the 2-line import swap of INTEGRATION.md gives an UNCHANGED ``TStarFramework`` (review item 1b of round 5), outside the timed region:
    the heuristic built by the reference's own call ``initialize_heuristic("owl-vit")`` -- no keyword arguments (TStarFramework.py:171-187, 207); the
    arithmetic mode comes from ``TSTAR_WEIGHTS_DTYPE``, the offline stand-in for the checkpoint from ``TSTAR_SYNTHETIC_SEED`` -- and the searcher built
    with the keywords of TStarFramework.py:97-107 at ITS defaults (4x4 grid, K = 8, threshold 0.6, budget 1000): ONE search alone, the visual history
    kept (image_grid_iters / detect_annotot_iters filled, as TStarFramework reads them at :152-157), the process-global numpy generator."""
    import torch
    from tstar_amd.interface_heuristic import initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    saved = {k_: os.environ.get(k_) for k_ in ("TSTAR_WEIGHTS_DTYPE", "TSTAR_SYNTHETIC_SEED", "TSTAR_MAX_BATCH")}
    out = {"what": "initialize_heuristic('owl-vit') with no keyword arguments + TStarSearcher(video_path=, target_objects=, cue_objects=, search_nframes=8, "
                   "image_grid_shape=(4, 4), output_dir=, confidence_threshold=0.6, search_budget=1000, heuristic=): ONE search alone, visual history ON, "
                   "global numpy generator seeded once (np.random.seed(2025)); mode selected by TSTAR_WEIGHTS_DTYPE (unset = f32)",
           "grid": "4x4 (16 frames/iter, the reference default)"}
    try:
        for mode in ("f32", "f32x3"):
            os.environ["TSTAR_SYNTHETIC_SEED"] = "0"
            os.environ.pop("TSTAR_MAX_BATCH", None)
            if mode == "f32":
                os.environ.pop("TSTAR_WEIGHTS_DTYPE", None)           # the library default
            else:
                os.environ["TSTAR_WEIGHTS_DTYPE"] = mode
            h = initialize_heuristic("owl-vit")
            assert h.weights_dtype == mode

            def one(seed):
                np.random.seed(seed)
                s_ = TStarSearcher(video_path=store, target_objects=list(TARGETS), cue_objects=list(CUES), search_nframes=k, image_grid_shape=(4, 4),
                                   output_dir=None, confidence_threshold=0.6, search_budget=1000, heuristic=h)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames, ts = s_.search()
                torch.cuda.synchronize()
                return s_, [float(t) for t in ts], time.perf_counter() - t0

            one(1)                                                      # first-use costs of this handle's shapes
            s_, ts, dt = one(2025)
            out[mode] = {"sec_per_video": dt, "frames_per_s": s_.frames_scored / dt, "frames_scored": s_.frames_scored, "grid_calls": s_.iterations,
                         "verify_calls": s_.detector_calls - s_.iterations, "history_entries": len(s_.image_grid_iters), "keyframes": ts,
                         "max_batch": h.scorer.max_batch, "env": {"TSTAR_WEIGHTS_DTYPE": os.environ.get("TSTAR_WEIGHTS_DTYPE")}}
            del s_, h
            torch.cuda.empty_cache()
    finally:
        for k_, v in saved.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v
    out["sec_per_video"] = out["f32x3"]["sec_per_video"]
    return out


def match_traffic(population, alg_bytes_run, stem, profiles_dir=None):
    """The PMC traffic figure of the dominant kernel for THIS run, or the reason there is none:
    -> (bytes per launch, bytes / the collection's own algorithmic bytes, source file, note).  ``stem``: file name after the round tag; a
    round may hold several collections of one mode (``<tag>_<stem>.json``, ``<tag>_<stem>_steps20.json`` ...: one per launch population).
    The newest round's file whose population is this run's (same flags that shape the launches, and its own algorithmic bytes per launch
    within 5 % of this run's) is quoted; otherwise the first reason met in the newest round -- a per-launch byte count of one population
    divided by another's algorithmic bytes is not a ratio of anything (round 5 printed 0.28x ... 1.83x that way)."""
    import glob
    profiles_dir = profiles_dir or os.path.join(ROOT, "profiles")
    first_note = None
    for tag in ("r06", "r05", "r04", "r03", "r02", "r01"):
        for tp in sorted(glob.glob(os.path.join(profiles_dir, f"{tag}_{stem}*.json"))):
            rel = os.path.relpath(tp, os.path.dirname(profiles_dir))
            try:
                with open(tp) as f:
                    tj = json.load(f)
            except Exception as e:
                first_note = first_note or (rel, f"unreadable: {e!r}")
                continue
            pop, ab = tj.get("population"), tj.get("algorithmic_bytes_per_launch")
            if not pop or not ab:
                first_note = first_note or (rel, "the newest PMC collection predates round 6 and does not record its launch population: not comparable")
                continue
            diff = sorted(k_ for k_ in population if pop.get(k_) != population[k_])
            if diff:
                first_note = first_note or (rel, "launch population differs from the PMC collection's in " +
                                            ", ".join(f"{k_} ({population[k_]!r} here, {pop.get(k_)!r} there)" for k_ in diff))
                continue
            if not alg_bytes_run or abs(ab / alg_bytes_run - 1.0) > 0.05:
                first_note = first_note or (rel, f"algorithmic bytes per launch differ: {alg_bytes_run:.4g} here, {ab:.4g} in the PMC collection")
                continue
            return tj["bytes_per_launch_corrected"], tj["bytes_per_launch_corrected"] / ab, rel, "same launch population as this run"
        if first_note:
            break                         # an older round's kernels are not this round's
    if first_note:
        return None, None, first_note[0], first_note[1]
    return None, None, None, "no PMC collection under profiles/"


def lockstep_group_sizes(n, L, PL):
    """Sizes of the lock-step groups `n` items are run in: groups of at most about L items, balanced (5 items at L = 4 -> 3 + 2, not
    4 + 1), their count a multiple of the alternation depth PL when n allows it -- a count that is not leaves the last group without a
    partner to alternate with (the driver's --steps 20 at L = 8 ran 7 + 7 alternating, then 6 alone).  Fewer, somewhat larger groups
    are preferred (20 -> 10 + 10) while they stay within 1.5 L and 31 items; else one more round of smaller ones."""
    if n <= 0:
        return []
    ng = (n + L - 1) // L
    if PL > 1 and ng % PL and n > 1:
        lo = ng // PL * PL
        ng = lo if lo >= PL and (n + lo - 1) // lo <= min(31, L + L // 2) else min(lo + PL, n)
    return [n // ng + (1 if k < n % ng else 0) for k in range(ng)]


def cpu_baseline(args, stats):
    """Reference-faithful CPU path (oracle = "port") on the host cores: one grid call and a few
    verification calls are timed, then extrapolated to the GPU run's call mix."""
    import torch
    from oracle import cpu_pipeline, owl_ref, resize_ref, searcher_ref
    from tstar_amd import weights as W
    from tstar_amd.tokenizer import encode_queries
    from tstar_amd.video import synthetic_frames_numpy
    g = args.grid
    det = cpu_pipeline.CpuOwlDetector(W.synthetic_state_dict(0), faithful=True)
    texts = [[o] for o in TARGETS + CUES] + [[" "]]
    ids, am = encode_queries(texts)
    det.reparameterize_object_list(TARGETS, CUES, ids, am)
    o2w = {**{t: 1.0 for t in TARGETS}, **{c: 0.5 for c in CUES}}
    n = g * g
    secs = list(np.arange(0, args.nframes, args.nframes // n)[:n])
    frames = synthetic_frames_numpy(secs, args.nframes, FRAME_H, FRAME_W, seed=0)    # "decoded" frames, untimed
    # The frame -> grid / verification-size resizes are cv2.resize calls in the reference (~1 ms per frame);
    # cv2 is not in this image and the numpy restatement of it takes ~50 ms per frame, so those images are
    # prepared UNTIMED (this favours the CPU).  Timed per detector call: Pillow bicubic to 768x768 (the real
    # library when importable), rescale/normalise, [text tower,] vision tower + heads, post-process, grid-cell
    # aggregation.
    grid_img = resize_ref.frames_to_grid(list(frames), g, g)
    nver = min(n, 64)
    ver_imgs = [resize_ref.cv_bilinear_resize(frames[i], 600, 285) for i in range(nver)]
    names = det.texts

    def call(d, img, rows, cols):
        xyxy, lab, conf, _ = d.inference_detector(img, library_speed=True)
        return searcher_ref.image_grid_score(xyxy, lab, conf, names, o2w, img.shape[0], img.shape[1], rows, cols)

    call(det, ver_imgs[0], 1, 1)                     # untimed warm-up (thread pools, first-touch allocations)
    # thread count: torch's default (all hardware threads) is far from the fastest on a many-core host for
    # batch-1 forwards; probe a few counts on one verification call each and keep the best for BOTH baselines
    nt_all = torch.get_num_threads()
    best_nt, best_t = nt_all, None
    for nt in sorted({min(c, nt_all) for c in (8, 16, 32, 64, nt_all)}):
        torch.set_num_threads(nt)
        call(det, ver_imgs[0], 1, 1)
        t0 = time.perf_counter()
        call(det, ver_imgs[1 % nver], 1, 1)
        t_ = time.perf_counter() - t0
        if best_t is None or t_ < best_t:
            best_nt, best_t = nt, t_
    torch.set_num_threads(best_nt)
    t0 = time.perf_counter()
    call(det, grid_img, g, g)
    t_grid = time.perf_counter() - t0
    nv, t_ver = 0, 0.0
    deadline = time.perf_counter() + max(1.0, args.cpu_seconds - t_grid)
    while nv < nver and time.perf_counter() < deadline:
        t0 = time.perf_counter()
        call(det, ver_imgs[nv], 1, 1)
        t_ver += time.perf_counter() - t0
        nv += 1
    t_ver /= max(nv, 1)
    per_video = stats["grid_calls"] * t_grid + stats["verify_calls"] * t_ver
    frames_scored = stats["grid_calls"] * n + stats["verify_calls"]
    png = png_write_cost(grid_img, ver_imgs[0])
    # CPU(O) of SURVEY 8d: the same restatement with this build's own call structure (text tower cached,
    # verification frames batched) -- what the CPU does when only the arithmetic, not the reference's call
    # pattern, is kept
    det_o = cpu_pipeline.CpuOwlDetector(W.synthetic_state_dict(0), faithful=False)
    det_o.reparameterize_object_list(TARGETS, CUES, ids, am)
    det_o.query_embeds()
    t0 = time.perf_counter()
    call(det_o, grid_img, g, g)
    t_grid_o = time.perf_counter() - t0
    t_ver_o, vb = None, 1
    for b_ in (1, 8):                                # best of: one frame per forward, eight per forward
        b_ = min(b_, nver)
        reps = 3 if b_ == 1 else 1
        t0 = time.perf_counter()
        for r_ in range(reps):
            px = np.stack([det_o.preprocess(ver_imgs[(r_ + i) % nver], library_speed=True) for i in range(b_)])
            owl_ref.detect(px, det_o.query_embeds(), det_o.wv, 285, 600, query_mask=det_o.ids[:, 0] > 0)
        t_b = (time.perf_counter() - t0) / (b_ * reps)
        if t_ver_o is None or t_b < t_ver_o:
            t_ver_o, vb = t_b, b_
    per_video_o = stats["grid_calls"] * t_grid_o + stats["verify_calls"] * t_ver_o
    grid4 = None
    if stats.get("grid4"):
        # CPU(R) at the reference's default 4x4 grid: one 380x800 grid call timed, verification calls as above
        g4 = stats["grid4"]
        grid4_img = resize_ref.frames_to_grid(list(frames[:16]), 4, 4)
        call(det, grid4_img, 4, 4)
        t0 = time.perf_counter()
        call(det, grid4_img, 4, 4)
        t_g4 = time.perf_counter() - t0
        pv4 = g4["grid_calls_per_video"] * t_g4 + g4["verify_calls_per_video"] * t_ver
        png4 = png_write_cost(grid4_img, ver_imgs[0])
        t_png4 = g4["grid_calls_per_video"] * png4["grid"] + g4["verify_calls_per_video"] * png4["verify"]
        grid4 = {"value": (g4["grid_calls_per_video"] * 16 + g4["verify_calls_per_video"]) / pv4, "unit": "frames/s", "sec_per_video": pv4,
                 "png_write_sec_per_call": png4, "with_png_sec_per_video": pv4 + t_png4,
                 "sample": f"1 grid call (16 frames, {t_g4:.3f} s) + the verification calls timed above ({t_ver:.3f} s each), extrapolated to "
                           f"{g4['grid_calls_per_video']:.1f} grid + {g4['verify_calls_per_video']:.1f} verification calls per video"}
    return {
        "value": frames_scored / per_video, "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
        "sample": f"1 grid call ({n} frames, {t_grid:.3f} s) + {nv} verification calls ({t_ver:.3f} s each) of the same "
                  f"workload, reference-faithful (text tower per call, batch-1 verification), extrapolated to the GPU "
                  f"run's call mix ({stats['grid_calls']} grid + {stats['verify_calls']} verification calls per video); "
                  f"{best_nt} torch threads (fastest of 8/16/32/64/{nt_all} on this host); "
                  f"the cv2.resize steps (not importable here) are prepared untimed",
        "sec_per_video": per_video, "grid4": grid4,
        # the reference's per-call debug PNG (interface_heuristic.py:248-256) reported SEPARATELY, never part of `value`
        "png_write_sec_per_call": png,
        "decode_note": "the reference re-opens the video with decord.VideoReader on EVERY read_frame_batch call (interface_searcher.py:168) and decodes the "
                       "sampled frames on the CPU; neither the re-open nor the decode is in this baseline (decord is not importable here and the frames are "
                       "synthesised off the clock, as they are resident in HBM before the GPU timer starts): both omissions favour the CPU figure",
        "own_batching": {"value": frames_scored / per_video_o, "unit": "frames/s", "sec_per_video": per_video_o,
                         "sample": f"1 grid call ({t_grid_o:.3f} s, cached query embeddings) + verification forwards of {vb} "
                                   f"frame(s) ({t_ver_o:.3f} s per frame; best of batch 1 and 8), same extrapolation"},
    }


def png_write_cost(grid_img, ver_img):
    """Seconds per call of the reference's unconditional debug block (interface_heuristic.py:248-256): ``Image.fromarray(annotated_image[:, :, ::-1])
    .save("./annotated_image.png")`` of the image every detector call scored -- the grid image (95 g x 200 g) or one 600x285 verification frame --
    with Pillow's default PNG settings, into a scratch directory.  Best of three writes each."""
    import tempfile
    from PIL import Image
    out = {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "annotated_image.png")
        for name, img in (("grid", grid_img), ("verify", ver_img)):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                Image.fromarray(img[:, :, ::-1]).save(path)
                t_ = time.perf_counter() - t0
                best = t_ if best is None or t_ < best else best
            out[name] = best
            out[name + "_image"] = f"{img.shape[1]}x{img.shape[0]}"
    return out


def cpu_baseline_full(args, seed, nthreads, deadline_s=150.0):
    """CPU(R) of SURVEY.md 8d MEASURED, not extrapolated: ONE complete reference-faithful search of the bench workload on the host
    cores -- the reference's loop (oracle.searcher_ref.SearcherRef: sampler, grid scoring, window spread, FITPACK fit, per-target
    verification, final weighted draw) driving one detector call per grid image / per verification frame, text tower on every call,
    batch-1 verification forwards (oracle.cpu_pipeline, faithful=True; Pillow's own bicubic for the 768x768 preprocess).  The clock
    covers every statement of that search except (i) producing the "decoded" frames (the GPU run has them resident in HBM before its
    timer starts) and (ii) the frame -> 200x95 / 600x285 resizes in the oracle's bit-exact numpy restatement of cv2.resize
    (~50 ms a frame; cv2 is not importable here): those are re-done on the same frames with Pillow's BILINEAR (a C resize of the
    cost class of cv2's) INSIDE the clock.  Returns None if the search does not finish within ``deadline_s``."""
    import torch
    from PIL import Image
    from oracle import cpu_pipeline, resize_ref, searcher_ref
    from tstar_amd import weights as W
    from tstar_amd.tokenizer import encode_queries
    from tstar_amd.video import synthetic_frames_numpy
    g = args.grid
    torch.set_num_threads(nthreads)
    det = cpu_pipeline.CpuOwlDetector(W.synthetic_state_dict(0), faithful=True)
    texts = [[o] for o in TARGETS + CUES] + [[" "]]
    ids, am = encode_queries(texts)
    det.reparameterize_object_list(TARGETS, CUES, ids, am)
    o2w = {**{t: 1.0 for t in TARGETS}, **{c: 0.5 for c in CUES}}
    excl = [0.0]           # seconds taken OFF the clock
    t_res = [0.0]          # Pillow resize seconds (on the clock)
    calls = {"grid": 0, "verify": 0}
    t_start = time.perf_counter()

    class TooSlow(Exception):
        pass

    def score_fn(kind, secs, rows, cols):
        if time.perf_counter() - t_start - excl[0] > deadline_s:
            raise TooSlow()
        t0 = time.perf_counter()
        frames = synthetic_frames_numpy(list(secs), args.nframes, FRAME_H, FRAME_W, seed=0)
        if kind == "grid":
            img = resize_ref.frames_to_grid(list(frames), rows, cols)
        else:
            img = resize_ref.cv_bilinear_resize(frames[0], 600, 285)
        excl[0] += time.perf_counter() - t0
        t0 = time.perf_counter()                                      # the library-speed stand-in for the reference's cv2.resize calls + tiling
        size = (200, 95) if kind == "grid" else (600, 285)
        small = [np.asarray(Image.fromarray(f).resize(size, Image.BILINEAR)) for f in frames]
        if kind == "grid":
            np.concatenate([np.concatenate(small[r * cols:(r + 1) * cols], axis=1) for r in range(rows)], axis=0)
        t_res[0] += time.perf_counter() - t0
        calls[kind] += 1
        px = det.preprocess(img, library_speed=True)[None]
        from oracle import owl_ref
        out = owl_ref.detect(px, det.query_embeds(), det.wv, img.shape[0], img.shape[1], query_mask=det.ids[:, 0] > 0)
        sc, lab, box = out["kept"][0]
        return searcher_ref.image_grid_score(box, lab, sc, det.texts, o2w, img.shape[0], img.shape[1], rows, cols)

    try:
        ref = searcher_ref.SearcherRef(args.nframes, 1.0, TARGETS, CUES, score_fn, np.random.RandomState(seed), search_nframes=args.search_nframes,
                                       image_grid_shape=(g, g), search_budget=1000, confidence_threshold=0.6)
        ts = ref.search()
    except TooSlow:
        return None
    t_cpu = time.perf_counter() - t_start - excl[0]
    frames_scored = calls["grid"] * g * g + calls["verify"]
    return {"value": frames_scored / t_cpu, "unit": "frames/s", "sec_per_video": t_cpu, "measured": "full",
            "grid_calls": calls["grid"], "verify_calls": calls["verify"], "frames_scored": frames_scored, "keyframes": [int(t) for t in ts],
            "resize_sec_pillow_bilinear": t_res[0], "off_clock_sec_frames_and_numpy_resize": excl[0], "cores": nthreads,
            "what": f"ONE complete reference-faithful search of the workload on the host (sampler seed {seed}): {calls['grid']} grid + {calls['verify']} "
                    f"verification detector calls, text tower per call, batch-1 verification, the searcher's own numpy / FITPACK statements, "
                    f"{nthreads} torch threads; clock = everything except frame synthesis and the numpy restatement of cv2.resize, whose "
                    f"work is re-done on the clock with Pillow BILINEAR ({t_res[0]:.2f} s)"}


def cpu_baseline_yolo(args, stats):
    """CPU statement of the YOLO-World backend (oracle/yolo_ref.py, torch on the host cores; kind "port": the real model's
    source is not in the reference tree) timed per detector call the way the reference makes them -- one image per call,
    letterbox + forward + NMS + the cell loop -- on one grid image and a few verification frames, extrapolated to the GPU
    run's call mix.  The frame -> grid / 600x285 resizes (cv2 in the reference) are prepared untimed."""
    import torch
    from oracle import resize_ref, searcher_ref, yolo_ref
    from tstar_amd import yolo_world as YW
    from tstar_amd.video import synthetic_frames_numpy
    g = args.grid
    n = g * g
    sd = YW.synthetic_state_dict(0, "l")
    rs = np.random.RandomState(0)
    txt = rs.standard_normal((len(TARGETS) + len(CUES) + 1, 512)).astype(np.float32)
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    texts = [[o] for o in TARGETS + CUES] + [[" "]]
    o2w = {**{t: 1.0 for t in TARGETS}, **{c: 0.5 for c in CUES}}
    secs = list(np.arange(0, args.nframes, args.nframes // n)[:n])
    frames = synthetic_frames_numpy(secs, args.nframes, FRAME_H, FRAME_W, seed=0)
    grid_img = resize_ref.frames_to_grid(list(frames), g, g)
    nver = min(n, 32)
    ver_imgs = [resize_ref.cv_bilinear_resize(frames[i], 600, 285) for i in range(nver)]

    def call(img, rows, cols):
        r = yolo_ref.detect(sd, [img], txt)[0]
        return searcher_ref.image_grid_score(r["xyxy"], r["labels"], r["scores"], texts, o2w, img.shape[0], img.shape[1], rows, cols)

    call(ver_imgs[0], 1, 1)
    nt_all = torch.get_num_threads()
    best_nt, best_t = nt_all, None
    for nt in sorted({min(c, nt_all) for c in (8, 16, 32, 64, nt_all)}):
        torch.set_num_threads(nt)
        call(ver_imgs[0], 1, 1)
        t0 = time.perf_counter()
        call(ver_imgs[1 % nver], 1, 1)
        t_ = time.perf_counter() - t0
        if best_t is None or t_ < best_t:
            best_nt, best_t = nt, t_
    torch.set_num_threads(best_nt)
    t0 = time.perf_counter()
    call(grid_img, g, g)
    t_grid = time.perf_counter() - t0
    nv, t_ver = 0, 0.0
    deadline = time.perf_counter() + max(1.0, args.cpu_seconds - t_grid)
    while nv < nver and time.perf_counter() < deadline:
        t0 = time.perf_counter()
        call(ver_imgs[nv], 1, 1)
        t_ver += time.perf_counter() - t0
        nv += 1
    t_ver /= max(nv, 1)
    per_video = stats["grid_calls"] * t_grid + stats["verify_calls"] * t_ver
    frames_scored = stats["grid_calls"] * n + stats["verify_calls"]
    return {"value": frames_scored / per_video, "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 grid call ({n} frames, {t_grid:.3f} s) + {nv} verification calls ({t_ver:.3f} s each) of the same workload through "
                      f"the CPU statement of YOLO-World-v2-L (torch conv2d on the host cores; letterbox incl. a numpy area resize, forward, "
                      f"NMS, cell loop), extrapolated to the GPU run's call mix ({stats['grid_calls']} grid + {stats['verify_calls']} "
                      f"verification calls per video); {best_nt} torch threads (fastest of 8/16/32/64/{nt_all}); cv2.resize steps untimed",
            "sec_per_video": per_video}


def other_configs():
    """BASELINE configs[3], configs[4] and configs[1] in the native-f32 mode, each as its own bench.py process AFTER this line's timed region
    (fresh process = its own warm-up, barriers and timed region; nothing shared with the headline).  Summaries only."""
    import subprocess
    runs = {
        "configs[3] yolo": ["--heuristic", "yolo", "--steps", "48"],
        "configs[4] bf16 weights, 14400 frames, K=32, grid 15": ["--weights", "bf16", "--nframes", "14400", "--grid", "15", "--search-nframes", "32", "--steps", "16"],
        "configs[1] on the native f32 MFMA tiles (the headline mode of rounds 1-4)": ["--weights", "f32", "--steps", "16"],
    }
    out = {}
    # the children are plain 1-GPU runs of their own: no launcher variables, none of this process's TSTAR_* overrides
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")
           and not k.startswith("TSTAR_")}
    for name, flags in runs.items():
        t1 = time.perf_counter()
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-grid4", "--no-other-configs",
               "--no-drop-in"] + flags
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[name] = {"error": (r.stderr or r.stdout)[-400:], "rc": r.returncode}
                continue
            j = json.loads(line[-1])
            out[name] = {"value": j["value"], "unit": j["unit"], "steps": j["steps"], "ms_per_step": j["ms_per_step"], "dtype": j["dtype"],
                         "sec_per_video": j["config"]["sec_per_video"], "single_search_alone_latency_sec": j["config"]["single_search_alone_latency_sec"],
                         "keyframes_verified": j["config"]["keyframes_verified"], "host_cpu_sec_per_video": j["config"]["host_cpu_sec_per_video"],
                         "roofline": {k: j["roofline"].get(k) for k in ("kernel", "bound", "achieved", "achieved_algorithmic", "peak", "unit", "frac", "frac_algorithmic", "executed_over_algorithmic",
                                                                            "scheme_ceiling_tflops", "time_share_of_step")},
                         "workload": j["config"]["workload"], "command": "python bench.py " + " ".join(cmd[2:]), "wall_s": time.perf_counter() - t1}
        except Exception as e:                                  # a sub-run must never take the headline line down
            out[name] = {"error": repr(e)}
    return out


def self_spawn(n):
    """`python bench.py --gpus N` typed as is (no launcher, WORLD_SIZE unset): start the N ranks ourselves -- the command the
    driver uses, torch.distributed.run with one process per GPU on 127.0.0.1 -- and hand its exit code back; rank 0's ONE JSON
    line goes to our stdout.  On a box with fewer than N visible GPUs the ranks share devices and the collectives go over gloo
    (TSTAR_BENCH_BACKEND), so the command still returns a (meaningless for scaling, labelled) line instead of an error."""
    import socket
    import subprocess
    import torch
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    env["MASTER_ADDR"] = "127.0.0.1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")        # torch.distributed.run would set 1: the host side (numpy, spline fits) is not the ranks' bottleneck but needs more than that
    ndev = torch.cuda.device_count()
    if ndev < n and "TSTAR_BENCH_BACKEND" not in env:
        print(f"bench.py: {ndev} GPU(s) visible for --gpus {n}: ranks share devices, collectives over gloo", file=sys.stderr)
        env["TSTAR_BENCH_BACKEND"] = "gloo"
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py")] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_spawn(args.gpus))
    # the searcher prints progress like the reference ("Found target ...", sampler warnings): keep stdout
    # clean for the ONE JSON line
    # ... and at the file-descriptor level too: RCCL prints a version banner and gloo its connection notes with C stdio
    # straight to fd 1, which would land next to the JSON line
    sys.stdout.flush()
    real_fd = os.dup(1)
    os.dup2(2, 1)
    real_stdout = os.fdopen(real_fd, "w")
    sys.stdout = sys.stderr
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    # One rank per GPU.  The path has ONE collective that carries data -- the all-gather of the keyframe rows -- and it goes over RCCL / xGMI
    # through the library's own communicator (tstar_comm_* / tstar_allgather_i32: the C-ABI entry a non-Python host would use), bootstrapped
    # over torch.distributed.  torch.distributed itself is only the control plane (barriers, the max-over-ranks of three doubles, the
    # communicator's unique id) and runs over gloo: no second RCCL communicator in the process, and nothing to tear down and re-create when
    # RCCL cannot come up -- round 6 found that the old "init nccl, on failure destroy and re-init gloo on another port" fallback HUNG under
    # torch.distributed.run (its agent store lives on the original port).  If the library's communicator cannot be created (ranks sharing a
    # GPU: "Duplicate GPU detected"; RCCL not loadable; a hang caught by the watchdog) the rows are gathered over gloo and the line says so
    # (config.collective_backend / collective_path).  TSTAR_BENCH_BACKEND=gloo skips RCCL outright (N ranks on a 1-GPU box).
    backend = os.environ.get("TSTAR_BENCH_BACKEND", "nccl")
    local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    cdev = "cpu"

    from tstar_amd import _lib
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd import sharding as _shard
    from tstar_amd.sharding import close_comm, gather_keyframes, interleave_by_item
    _shard.PREFER_RCCL = backend == "nccl"
    from tstar_amd.video import synthetic_video
    lib = _lib.load()

    import queue
    import threading
    conc = max(1, min(args.concurrency, args.steps))
    if args.heuristic == "yolo":
        from tstar_amd.interface_heuristic import YoloWorldInterface
        heuristics = [YoloWorldInterface(synthetic_seed=0, scale="l", max_batch=args.yolo_max_batch, device=f"cuda:{local_rank}")
                      for _ in range(conc)]
    else:
        heuristics = [OWLInterface(synthetic_seed=0, max_batch=args.max_batch, device=f"cuda:{local_rank}",
                                   weights_dtype=args.weights) for _ in range(conc)]
    streams = [torch.cuda.Stream() for _ in range(conc)]
    g = args.grid
    workload = args.workload
    if workload == "auto":
        workload = "single" if world == 1 else "haystack"
    if workload == "haystack32":
        args.steps = (32 - rank + world - 1) // world            # item i -> rank i % world; 32 items in total
        n_items_total = 32
    else:
        n_items_total = args.steps * world
    shared_store = synthetic_video(args.nframes, FRAME_H, FRAME_W, seed=0) if workload == "single" else None
    cycle_questions = args.questions == "cycle" or (args.questions == "auto" and workload == "haystack32")

    def make_item(item_id, sampler_seed, store_seed=None):
        """One (video, question) item; its decoded video is built in HBM here, before any timed region."""
        if workload == "single":
            return dict(id=item_id, store=shared_store, targets=TARGETS, cues=CUES, seed=sampler_seed)
        t_, c_ = QUESTIONS[item_id % len(QUESTIONS)] if cycle_questions else (TARGETS, CUES)
        return dict(id=item_id, store=synthetic_video(args.nframes, FRAME_H, FRAME_W, seed=1000 + (item_id if store_seed is None else store_seed)),
                    targets=t_, cues=c_, seed=sampler_seed)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run_many(items):
        """Run one search per item, `conc` lock-step groups at a time; returns per-search (searcher, timestamps, seconds, keyframes)."""
        q = queue.Queue()
        L = max(1, min(args.lockstep, 31))
        PL = max(1, args.pipeline)
        while PL > 1 and PL * L > 63:             # query-set slots of one detector handle (include/tstar_hip.h)
            PL -= 1
        # groups of at most L items, balanced (5 items at L = 4 -> 3 + 2, not 4 + 1); PL consecutive groups alternate on the
        # GPU (tstar_amd.lockstep)
        sizes = lockstep_group_sizes(len(items), L, PL)
        ng = len(sizes)
        starts = [sum(sizes[:k]) for k in range(ng)]
        for k in range(0, ng, PL):
            q.put((starts[k], [items[starts[j]:starts[j] + sizes[j]] for j in range(k, min(k + PL, ng))]))
        out = [None] * len(items)
        errs = []

        def worker(w):
            torch.cuda.set_device(local_rank)
            try:
                with torch.cuda.stream(streams[w]):
                    while True:
                        try:
                            i, sd = q.get_nowait()
                        except queue.Empty:
                            break
                        t1 = time.perf_counter()
                        grps = run_groups(heuristics[w], sd, g, args.search_nframes)
                        torch.cuda.synchronize()
                        for j, (s_, ts_, fr_) in enumerate([x for grp in grps for x in grp]):
                            out[i + j] = (s_, ts_, time.perf_counter() - t1, fr_)
            except Exception as e:                      # surface worker failures in the main thread
                errs.append(e)

        if conc == 1:
            worker(0)
        else:
            th = [threading.Thread(target=worker, args=(w,)) for w in range(conc)]
            [t_.start() for t_ in th]
            [t_.join() for t_ in th]
        if errs:
            raise errs[0]
        return out

    # untimed warm-up: at least one FULL lock-step group, so the timed region meets no first-use cost
    # (kernel attributes, resample tables, workspace growth) at its own batch sizes
    n_warm = 0 if args.warmup <= 0 else max(args.warmup, min(args.lockstep, 31) * conc,
                                            min(min(args.lockstep, 31) * max(1, args.pipeline), 16) * conc)   # OWL: two full groups of 8
    # this rank's timed items: item id k * world + rank (item i -> rank i % world); the sampler seed is a function of the
    # item id only, so results do not depend on the rank count.  Videos are resident in HBM before the timer starts.
    items = [make_item(k * world + rank, 2025 + k * world + rank) for k in range(args.steps)]
    warm_items = [dict(items[w % len(items)], seed=10_000 + rank * 1000 + w) for w in range(n_warm)] if items else []
    run_many(warm_items)
    # latency of ONE search running alone (the "sec/video to 8 keyframes" half of the metric, untimed; --full only):
    solo_latency = None
    if args.full and n_warm > 0 and items:
        # a search alone runs other batch shapes than a lock-step group (its own verification batches): one untimed run
        # first, like the warm-up of the groups, so that the figure carries no first-use cost
        run_group(heuristics[0], [dict(items[0], seed=19_000 + rank)], g, args.search_nframes)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_group(heuristics[0], [dict(items[0], seed=20_000 + rank)], g, args.search_nframes)
        torch.cuda.synchronize()
        solo_latency = time.perf_counter() - t1
    if world > 1:                      # create the library's RCCL communicator before the timer (a one-off, like NCCL init)
        gather_keyframes([[0]], world)
    barrier()
    # time one GEMM / attention / conv launch out of every 5 consecutive ones with HIP event pairs, at a position that
    # changes from block to block (csrc/prof.hip: no aliasing with the launch pattern); timing all of them costs 2.2 %
    _lib.check(lib.tstar_prof_enable(0 if os.environ.get('TSTAR_BENCH_NO_PROF') else PROF_STRIDE))

    def stamp(which):
        """Mark one end of the timed region for trace tools: an empty marker kernel on the launch stream (the window on the
        GPU's own timeline, tools/rocpd_window.py) plus the host clocks a profiler may use for its timestamps."""
        _lib.check(lib.tstar_prof_mark(which, _lib.stream_ptr()))
        return {f"t{which}_realtime_ns": time.time_ns(), f"t{which}_monotonic_ns": time.monotonic_ns(),
                f"t{which}_boottime_ns": time.clock_gettime_ns(time.CLOCK_BOOTTIME)}

    from tstar_amd import spline_pool as _sp

    def host_cpu_seconds():
        """user + system CPU seconds consumed so far by this rank's process (all threads) and by its FITPACK worker processes."""
        pool = _sp._pool
        return time.process_time() + (pool.cpu_seconds() if pool is not None else 0.0)

    if _sp._pool is None and _sp.get_pool() is not None:      # no warm-up ran: start the spline workers now and let them finish their
        xs = np.arange(8.0)                                   # imports (one fit each), so that their start-up CPU is not the timed region's
        _sp._pool.fit_many([(xs, xs * 0.5)] * len(_sp._pool), 0.5)
    barrier()
    timed_region = stamp(0)
    cpu0 = host_cpu_seconds()
    t0 = time.perf_counter()
    res = run_many(items)
    frames = sum(r[0].frames_scored for r in res)
    grid_calls = sum(r[0].iterations for r in res)
    verify_calls = sum(r[0].detector_calls - r[0].iterations for r in res)
    images = sum(r[0].device_images_scored for r in res)
    keys = [[int(t) for t in r[1]] for r in res]
    latency = sum(r[2] for r in res) / max(len(res), 1)
    # RCCL all-gather of the keyframe indices (N > 1), rows back in item order
    all_keys = gather_keyframes(keys, world, pad_to=(n_items_total + world - 1) // world)
    from tstar_amd import sharding as _sh
    collective_path = _sh.LAST_GATHER_PATH        # which way the timed gather went (RCCL through the C ABI on a GPU job)
    if world > 1:
        all_keys = interleave_by_item(all_keys, n_items_total, world)
    torch.cuda.synchronize()
    timed_region.update(stamp(1))
    barrier()
    dt = time.perf_counter() - t0
    host_cpu = host_cpu_seconds() - cpu0
    t = torch.tensor([dt, float(frames), float(images)], dtype=torch.float64, device=cdev)
    if world > 1:
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dt, frames_all, images_all = tmax[0].item(), t[1].item(), t[2].item()
        free_b, total_b = torch.cuda.mem_get_info()
        hc = [torch.zeros(2, dtype=torch.float64, device=cdev) for _ in range(world)]
        dist.all_gather(hc, torch.tensor([host_cpu / max(args.steps, 1), (total_b - free_b) / 2 ** 30], dtype=torch.float64, device=cdev))
        host_cpu_by_rank = [float(x[0].item()) for x in hc]
        hbm_by_rank = [float(x[1].item()) for x in hc]
    else:
        frames_all, images_all = float(frames), float(images)
        host_cpu_by_rank = [host_cpu / max(args.steps, 1)]
        free_b, total_b = torch.cuda.mem_get_info()
        hbm_by_rank = [(total_b - free_b) / 2 ** 30]

    # roofline of the dominant kernel (gemm_f32_kernel): HIP events on the launch stream, this rank
    n_l, ms, fl = C.c_longlong(0), C.c_double(0), C.c_double(0)
    _lib.check(lib.tstar_prof_read(0, C.byref(n_l), C.byref(ms), C.byref(fl)))
    if args.heuristic == "yolo":                  # dominant kernels of the YOLO-World backend: the VALU convolutions (category 2)
        _lib.check(lib.tstar_prof_read(2, C.byref(n_l), C.byref(ms), C.byref(fl)))
    by = C.c_double(0)
    _lib.check(lib.tstar_prof_read_bytes(2 if args.heuristic == "yolo" else 0, C.byref(by)))
    a_l, a_ms, a_fl = C.c_longlong(0), C.c_double(0), C.c_double(0)
    _lib.check(lib.tstar_prof_read(1, C.byref(a_l), C.byref(a_ms), C.byref(a_fl)))
    # every launch of the two categories (sampled or not): count and algorithmic flops, exact.  A category's time share is
    # all-launch flops / (sampled flops / sampled ms) / wall: launch durations span 13 us .. 4 ms, so sampled ms x stride
    # carries the +-5 % error of a 1-in-5 sample of them, while flops / ms is nearly the same for every large launch
    n_all, fl_all, a_all, a_fl_all = C.c_longlong(0), C.c_double(0), C.c_longlong(0), C.c_double(0)
    _lib.check(lib.tstar_prof_read_totals(2 if args.heuristic == "yolo" else 0, C.byref(n_all), C.byref(fl_all)))
    _lib.check(lib.tstar_prof_read_totals(1, C.byref(a_all), C.byref(a_fl_all)))
    _lib.check(lib.tstar_prof_enable(0))
    share = lambda f_all, f_s, ms_s: (f_all / (f_s / (ms_s * 1e-3)) / dt / max(conc, 1)) if f_s > 0 and ms_s > 0 else 0.0
    achieved = fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
    # HBM-side traffic of the same kernel: rocprofv3 PMC passes of this command cannot run inside the
    # timed process, so the per-launch figure measured with `tools/rocpd_traffic.py` is read from the
    # committed summary (profiles/); None if it has not been collected.
    # The figure is quoted ONLY when that collection ran this run's launch population (same flags that shape the launches, and its
    # own algorithmic bytes per launch within 5 % of this run's): a per-launch byte count of one population divided by another's
    # algorithmic bytes is not a ratio of anything (round 5 printed 0.28x ... 1.83x that way).
    population = {"heuristic": args.heuristic, "weights": (args.weights if args.heuristic == "owl" else "f32-valu"), "steps": args.steps,
                  "lockstep": max(1, min(args.lockstep, 31)), "pipeline": max(1, args.pipeline),
                  "max_batch": args.yolo_max_batch if args.heuristic == "yolo" else args.max_batch, "grid": args.grid, "nframes": args.nframes,
                  "search_nframes": args.search_nframes, "workload_kind": workload, "n_gpus": world, "concurrency": conc}
    alg_bytes_run = by.value / max(n_l.value, 1)

    read_traffic = lambda stem: match_traffic(population, alg_bytes_run, stem)

    # the newest collection of THIS mode (tools/collect_profiles.sh); files without a mode suffix are the native-f32 kernels'
    sfx = {"f32": "", "f32x3": "_f32x3", "bf16": "_bf16", "bf16_exact": "_bf16_exact"}[args.weights]
    traffic, traffic_ratio, traffic_src, traffic_note = read_traffic("pmc_gemm_traffic" + sfx)

    # f32 weights: native f32 MFMA, algorithmic = executed flops.  bf16 weights: each algorithmic product is
    # three bf16 MFMA products (exact activation split), priced against the dense bf16 peak.
    bound = "mfma"
    if args.heuristic == "yolo":
        gemm_kernel, peak, exec_mult, bound = "conv_valu_kernel + conv_sw_kernel (implicit-GEMM convolutions, v_pk_fma_f32, no MFMA)", FP32_MFMA_PEAK_TFLOPS, 1.0, "valu"
        traffic, traffic_ratio, traffic_src, traffic_note = read_traffic("yolo_pmc_conv_traffic")      # tools/collect_yolo_profiles.sh
    elif args.weights == "bf16":
        gemm_kernel, peak, exec_mult = "gemm_bf16w2_wide_kernel / gemm_f32_kernel<WMODE=3> (2 x v_mfma_f32_32x32x16_bf16 per K=16)", BF16_MFMA_PEAK_TFLOPS, 2.0
    elif args.weights == "bf16_exact":
        gemm_kernel, peak, exec_mult = "gemm_f32_kernel<WMODE=1> (3 x v_mfma_f32_32x32x16_bf16 per K=16)", BF16_MFMA_PEAK_TFLOPS, 3.0
    elif args.weights == "f32x3":
        gemm_kernel, peak, exec_mult = ("gemm_bf16w2_wide_kernel<WMODE=4> / gemm_f32_kernel<WMODE=4> (gemm_tile_x3: 6 x v_mfma_f32_32x32x16_bf16 per K=16, "
                                        "weight planes global -> VGPR in fragment order a full K step ahead, software-pipelined per wave)"), BF16_MFMA_PEAK_TFLOPS, 6.0
    else:
        gemm_kernel, peak, exec_mult = "gemm_f32_kernel (v_mfma_f32_32x32x2_f32)", FP32_MFMA_PEAK_TFLOPS, 1.0
    if rank == 0 and args.dump_outputs and res:
        dump_outputs(args.dump_outputs, res[-1])
    # post-run parity check of the keyframes this run produced (rank 0, step 0): solo re-run + oracle replay, untimed (--full)
    verified, verify_detail = None, None
    if rank == 0 and args.full and not args.no_verify and items:
        verified, verify_detail = verify_keyframes(heuristics[0], items[0], g, args.search_nframes, keys[0])
    wl_name = {"single": "configs[1]", "haystack": "configs[2] shape (weak scaling: --steps items per rank)",
               "haystack32": "configs[2]"}[workload]
    if args.heuristic == "yolo":
        wl_name = "configs[3]" if workload == "single" else wl_name + " with the configs[3] backend"
    if args.weights not in ("f32", "f32x3") or args.nframes != N_FRAMES:
        wl_name = "variant of " + wl_name
    det_name = ("YOLO-World-v2-L (seeded synthetic weights, f32 VALU kernels, no MFMA; score > 0.12, top-50)" if args.heuristic == "yolo"
                else f"OWL-ViT-B/32 {args.weights} weights (seeded synthetic)")
    if workload == "single":
        wl_what = (f"ONE {args.nframes}-frame {FRAME_H}x{FRAME_W} synthetic RGB video resident in HBM, 1 question (targets {TARGETS}, "
                   f"cues {CUES}), every step = one full search of it with its own sampler seed")
    else:
        wl_what = (f"{n_items_total} independent (video, question) items, item i on rank i % {world}: each its own {args.nframes}-frame "
                   f"{FRAME_H}x{FRAME_W} procedural RGB video resident in HBM (seed 1000 + i) and "
                   + (f"one of {len(QUESTIONS)} questions, cycled ({'; '.join('/'.join(t) + ' | ' + '/'.join(c) for t, c in QUESTIONS)})"
                      if cycle_questions else f"the configs[1] question (targets {TARGETS}, cues {CUES})")
                   + "; every step = one item's full search")
    if rank == 0:
        out = {
            "metric": "candidate frames scored/sec (whole node) + sec/video to 8 keyframes, 1h@1fps",
            "value": frames_all / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 VALU (v_pk_fma_f32 implicit-GEMM convolutions), no MFMA" if args.heuristic == "yolo" else
                      {"f32": "f32", "bf16": "f32 activations (two round-to-nearest bf16 terms) x bf16 weights, exact products, f32 accumulate",
                       "bf16_exact": "f32 activations x bf16 weights (exact 3-term split on the bf16 MFMA pipe)",
                       "f32x3": "f32 held exactly as 3 bf16 terms per operand: every GEMM and vision-attention operand (activations, weights, Q, K, V, softmax "
                                "probabilities) = three round-to-nearest bf16 terms carrying all 24 significand bits; the 6 partial products with i + j <= 2 "
                                "(each exact) on v_mfma_f32_32x32x16_bf16, f32 accumulate -- error vs float64 <= the native f32 MFMA kernels' (tests); "
                                "LayerNorm, softmax statistics, epilogues and head tails plain f32"}[args.weights]),
            "data": "synthetic",
            "config": {
                # the data-path collective that actually ran: "nccl" = ncclAllGather on the library's RCCL communicator, "gloo" = torch.distributed
                # over gloo (asked for with TSTAR_BENCH_BACKEND=gloo, or the fallback: collective_path says why); the control plane is gloo
                "collective_backend": (("nccl" if "ncclAllGather" in (collective_path or "") else "gloo") if world > 1 else None),
                "collective_path": collective_path, "control_plane": ("torch.distributed over gloo" if world > 1 else None),
                "workload": f"{wl_name}: {wl_what}; {det_name}, grid {g}x{g} = "
                            f"{g * g} frames/iter, search_nframes={args.search_nframes}, threshold 0.6, budget 1000",
                "workload_kind": workload, "items_total": n_items_total, "population": population,
                "sec_per_video": dt / args.steps, "videos_per_rank": args.steps, "searches_in_flight_per_gpu": conc, "lockstep_items_per_batch": max(1, min(args.lockstep, 31)),
                "lockstep_groups_alternating": max(1, args.pipeline),
                "mean_search_latency_sec": latency, "single_search_alone_latency_sec": solo_latency,
                # what predicts the 8-rank curve: CPU seconds (user + sys) of this rank's process AND its spline worker processes over
                # the timed region, per video; host_cores = hardware threads this process may run on (its affinity mask)
                "host_cpu_sec_per_video": host_cpu / max(args.steps, 1), "host_cpu_busy_cores": host_cpu / dt,
                "host_cpu_sec_per_video_by_rank": host_cpu_by_rank,
                # HBM in use on each rank's DEVICE at the end of the timed region (hipMemGetInfo: weights + workspaces + resident videos + torch's
                # cache; ranks that share a device -- the 1-GPU rehearsal of an N-rank launch -- all report that device's total)
                "hbm_used_gib_by_rank": hbm_by_rank,
                "host_cores": _sp.host_threads(), "host_spline_workers": (len(_sp._pool) if _sp._pool is not None else 0),
                # the per-iteration annotated grid images / frames the reference keeps unconditionally (interface_searcher.py:469-474)
                # are NOT produced in the timed region (keep_visual_history=False); with them a search costs +2-4 %
                "visual_history": False,
                "grid_calls_per_video": grid_calls / args.steps, "verify_calls_per_video": verify_calls / args.steps,
                "detector_images_per_video": images / args.steps, "max_batch": args.yolo_max_batch if args.heuristic == "yolo" else args.max_batch,
                "keyframes_rank0_step0": keys[0], "gathered_keyframe_rows": len(all_keys), "gathered_keyframes": all_keys,
                "keyframes_verified": verified, "keyframes_verification": verify_detail,
                # both ends of the timed region: marker kernels prof_mark_begin_kernel / prof_mark_end_kernel were enqueued on
                # the launch stream at these instants (a kernel trace is cut between them: tools/rocpd_window.py)
                "timed_region": timed_region,
            },
            "roofline": {
                "kernel": gemm_kernel, "bound": bound, "achieved": achieved * exec_mult,
                "peak": peak, "unit": "TFLOP/s", "frac": achieved * exec_mult / peak,
                # ONE definition per number (review item 2 of round 5).  `achieved` / `frac` price the flops the matrix (or vector) pipe
                # EXECUTES: `executed_over_algorithmic` hardware products per algorithmic multiply-add (6 in the f32x3 scheme, 2 / 3 in the
                # bf16-weight modes, 1 for native f32 and the VALU convolutions).  `achieved_algorithmic` / `frac_algorithmic` price the
                # 2*M*N*K flops of SURVEY 8d against the same peak.  `scheme_ceiling_tflops` = peak / executed_over_algorithmic is the
                # most algorithmic TFLOP/s this scheme can reach on this pipe; achieved_algorithmic / scheme_ceiling == frac.
                "frac_definition": "executed flops (achieved = executed_over_algorithmic x achieved_algorithmic) / peak; equals achieved_algorithmic / scheme_ceiling_tflops",
                "frac_executed": achieved * exec_mult / peak, "frac_algorithmic": achieved / peak,
                "achieved_algorithmic": achieved, "executed_over_algorithmic": exec_mult, "scheme_ceiling_tflops": peak / exec_mult,
                "traffic": traffic, "traffic_over_algorithmic": traffic_ratio,
                "traffic_unit": "bytes per launch (L2 fabric side: FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes)",
                "traffic_source": traffic_src, "traffic_note": traffic_note,
                "launches_timed": n_l.value, "timed_every_nth_launch": PROF_STRIDE, "avg_launch_ms": ms.value / max(n_l.value, 1),
                "avg_launch_gflop": fl.value / max(n_l.value, 1) / 1e9,
                # every operand read once, the result written once (GEMM: A + W + C + residual + bias rows; conv: input
                # channels + output channels + weights + fused residual / gate), averaged over the same sampled launches
                "algorithmic_bytes_per_launch": alg_bytes_run,
                "launches_total": n_all.value, "gflop_total": fl_all.value / 1e9,
                "time_share_of_step": share(fl_all.value, fl.value, ms.value),
                "gemm_plus_attention_time_share_of_step": share(fl_all.value, fl.value, ms.value) + share(a_fl_all.value, a_fl.value, a_ms.value),
                "attention_kernel": {"kernel": "attention_x3_kernel (6 x v_mfma_f32_32x32x16_bf16 per step, exact three-term operands)" if args.weights == "f32x3"
                                     else ("attention_split_kernel" if args.weights in ("bf16", "bf16_exact") else "attention_f32_kernel"),
                                     "achieved_algorithmic": (a_fl.value / (a_ms.value * 1e-3) / 1e12) if a_ms.value > 0 else 0.0,
                                     "executed_over_algorithmic": 6.0 if args.weights == "f32x3" else (3.0 if args.weights in ("bf16", "bf16_exact") else 1.0),
                                         "launches_timed": a_l.value, "launches_total": a_all.value,
                                         "time_share_of_step": share(a_fl_all.value, a_fl.value, a_ms.value)},
            },
        }
        if args.heuristic == "yolo":
            out["roofline"].pop("attention_kernel", None)
            out["roofline"]["peak_note"] = "f32 VALU spec peak (v_pk_fma_f32 rate); a tiled f32 VALU GEMM sustains about a third of it on this part (MI355X guide: 52 TFLOP/s)"
        g4rec = None
        full = world == 1 and args.full                      # the records below are not the headline's: --full only
        if full and not args.no_grid4 and args.heuristic == "owl" and workload == "single" and g != 4:
            g4rec = grid4_record(heuristics[0], shared_store, args.nframes, args.search_nframes)
            out["config"]["grid4"] = g4rec
        if full and not args.no_drop_in and args.heuristic == "owl" and workload == "single":
            try:
                out["config"]["drop_in"] = drop_in_record(shared_store, args.search_nframes)
            except Exception as e:                                  # an extra record must never take the headline line down
                out["config"]["drop_in"] = {"error": repr(e)}
        if (full and not args.no_other_configs and args.heuristic == "owl" and args.weights == "f32x3" and workload == "single"
                and args.nframes == N_FRAMES and g == 16 and args.search_nframes == 8):
            out["config"]["other_configs"] = other_configs()
            # the native-f32 figure of the same workload beside the headline (what rounds 1-4 reported as `value`)
            nat = [v for k_, v in out["config"]["other_configs"].items() if "native f32" in k_]
            if nat and "error" not in nat[0]:
                out["config"]["f32_native"] = {"value": nat[0]["value"], "unit": nat[0]["unit"], "ms_per_step": nat[0]["ms_per_step"],
                                               "roofline_frac_of_157.3_TFLOPs": nat[0]["roofline"]["frac"], "keyframes_verified": nat[0]["keyframes_verified"],
                                               "headline_over_native": out["value"] / nat[0]["value"]}
        if full and not args.no_cpu_baseline:
            stats_ = {"grid_calls": grid_calls / args.steps, "verify_calls": verify_calls / args.steps, "grid4": g4rec}
            out["cpu_baseline"] = cpu_baseline_yolo(args, stats_) if args.heuristic == "yolo" else cpu_baseline(args, stats_)
            if args.cpu_baseline == "full" and args.heuristic == "owl" and workload == "single":
                cb = out["cpu_baseline"]
                full = cpu_baseline_full(args, items[0]["seed"], cb["cores"])
                if full is not None:
                    sampled = {k_: cb[k_] for k_ in ("value", "unit", "sample", "sec_per_video")}
                    cb.update({"value": full["value"], "sec_per_video": full["sec_per_video"], "measured": "full", "sample": full["what"],
                               "full_search": full, "sampled_extrapolation": sampled, "measured_over_sampled": full["value"] / sampled["value"]})
                else:
                    cb["measured"] = "sampled (the full search did not finish within its 150 s bound)"
            else:
                out["cpu_baseline"]["measured"] = "sampled"
            cb = out["cpu_baseline"]
            if cb.get("png_write_sec_per_call"):
                pg = cb["png_write_sec_per_call"]
                gc_, vc_ = ((cb["full_search"]["grid_calls"], cb["full_search"]["verify_calls"]) if cb.get("full_search")
                            else (stats_["grid_calls"], stats_["verify_calls"]))
                fr_ = gc_ * g * g + vc_
                t_png = gc_ * pg["grid"] + vc_ * pg["verify"]
                cb["with_png"] = {"sec_per_video": cb["sec_per_video"] + t_png, "value": fr_ / (cb["sec_per_video"] + t_png), "unit": "frames/s",
                                  "png_sec_per_video": t_png,
                                  "what": f"cpu_baseline.sec_per_video + {gc_:.0f} grid-image PNG writes ({pg['grid']:.3f} s each, {pg['grid_image']}) + {vc_:.0f} "
                                          f"verification-frame PNG writes ({pg['verify']:.4f} s each): what the reference's loop costs WITH its per-call "
                                          "./annotated_image.png; reported beside `value`, not in it (this build writes no such file)"}
            out["config"]["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
            di = out["config"].get("drop_in")
            if di and "error" not in di and cb.get("grid4"):
                for m_ in ("f32", "f32x3"):
                    di[m_]["speedup_vs_cpu_baseline_grid4"] = di[m_]["frames_per_s"] / cb["grid4"]["value"]
                di["cpu_baseline_grid4_sec_per_video"] = cb["grid4"]["sec_per_video"]
            if g4rec and out["cpu_baseline"].get("grid4"):
                g4rec["speedup_vs_cpu_baseline_lockstep16"] = g4rec["lockstep16_frames_per_s"] / out["cpu_baseline"]["grid4"]["value"]
                g4rec["speedup_vs_cpu_baseline_solo"] = g4rec["solo_frames_per_s"] / out["cpu_baseline"]["grid4"]["value"]
        print(json.dumps(out), file=real_stdout, flush=True)
    if world > 1:
        dist.barrier()
        from tstar_amd import sharding as _sh2
        if _sh2.COMM_TIMED_OUT:
            # a helper thread may still sit inside ncclCommInitRank (it cannot be cancelled): the line is out, leave without running
            # RCCL's / torch's teardown, which could wait for that thread's communicator
            real_stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        close_comm()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
