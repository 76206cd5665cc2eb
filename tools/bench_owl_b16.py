#!/usr/bin/env python
"""OWL-ViT B/16 against B/32 on one MI355X: detector images/s, one configs[1]-shaped search, FLOP per image.

  python tools/bench_owl_b16.py --out profiles/b16_measure.json              # everything below, one JSON
  python tools/bench_owl_b16.py --only-b16-256                               # one B/16 f32x3 batch of 256 (for a kernel trace)

* detector: ``OwlScorer.score`` on B in {1, 256} grid-sized images (1520 x 3200, the 16 x 16 grid of the bench) for B/32 and
  B/16 in the f32 and f32x3 modes; warm-up calls first, then device-event timing over the timed calls;
* search: ``TStarSearcher`` with a B/16 synthetic heuristic on the configs[1] shape (N = 3600, 16 x 16 grid, K = 8, budget
  1000, threshold 0.6, sampler seed 2025) -- frames scored per second and seconds per video (wall clock, device synchronised);
* FLOP per image from the shapes (GEMMs 2 M N K, attention 4 T^2 D per layer: S = Q K^T and O = P V).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flops_per_image(g):
    D, FF, L = 768, 3072, 12
    T = g.ntok
    gemm_layer = 2.0 * T * (3 * D * D + D * D + 2 * D * FF)         # qkv, out-proj, fc1, fc2
    attn_layer = 4.0 * T * T * D
    patch = 2.0 * g.npatch * D * g.patch_k
    heads = 2.0 * g.npatch * (512 * D + 2 * D * D + 4 * D)         # class head dense0, box head dense0 / dense1 / dense2
    total = L * (gemm_layer + attn_layer) + patch + heads
    return dict(total=total, gemm_per_layer=gemm_layer, attention_per_layer=attn_layer, patch_embed=patch, heads=heads,
                attention_fraction=L * attn_layer / total)


def time_detector(torch, scorer, B, warmup, reps):
    g = torch.Generator(device="cuda").manual_seed(B)
    imgs = torch.randint(0, 256, (B, 1520, 3200, 3), dtype=torch.uint8, device="cuda", generator=g)
    for _ in range(warmup):
        scorer.score(imgs, 16, 16)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        scorer.score(imgs, 16, 16)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return dict(B=B, ms_per_call=ms, images_per_s=B / (ms / 1e3), reps=reps, warmup=warmup)


def make_scorer(W, OwlScorer, geometry, mode, max_batch):
    sd = W.synthetic_state_dict(0, geometry=geometry)
    s = OwlScorer(W.pack_blob(sd, W.vision_spec(geometry)), W.pack_blob(sd, W.text_spec()), max_batch=max_batch, weights_mode=mode,
                  patch_size=geometry.patch_size)
    from tstar_amd.tokenizer import encode_queries
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    s.set_queries(ids, am, [1.0, 0.5, 0.5, 0.5])
    return s


def run_search(torch, np, mode, runs):
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    h = OWLInterface(synthetic_seed=0, max_batch=256, patch_size=16, weights_dtype=mode)
    store = synthetic_video(3600, seed=0)
    out = []
    for r in range(runs + 1):                                        # run 0 warms up (tables, lane 1, spline workers)
        s = TStarSearcher(store, h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(16, 16), search_budget=1000,
                          confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ts = s.search()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r > 0:
            out.append(dict(s_per_video=dt, frames_scored=s.frames_scored, frames_per_s=s.frames_scored / dt, iterations=s.iterations,
                            keyframes=[float(t) for t in ts]))
    del h
    return dict(mode=mode, N=3600, grid=16, K=8, budget=1000, seed=2025, runs=out,
                median_s_per_video=float(np.median([o["s_per_video"] for o in out])),
                median_frames_per_s=float(np.median([o["frames_per_s"] for o in out])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--search-runs", type=int, default=2)
    ap.add_argument("--only-b16-256", action="store_true", help="one warm-up and one timed B/16 f32x3 call at B = 256, nothing else")
    args = ap.parse_args()
    import numpy as np
    import torch
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0),
               flops_per_image={g.name: flops_per_image(g) for g in (W.B32, W.B16)})
    if args.only_b16_256:
        s = make_scorer(W, OwlScorer, W.B16, "f32x3", 256)
        res["detector"] = [dict(geometry="B/16", mode="f32x3", **time_detector(torch, s, 256, 1, 1))]
    else:
        det = []
        for geom in (W.B32, W.B16):
            for mode in ("f32", "f32x3"):
                s = make_scorer(W, OwlScorer, geom, mode, 256)
                for B in (1, 256):
                    r = dict(geometry=geom.name, mode=mode, **time_detector(torch, s, B, args.warmup, args.reps if B > 1 else 20))
                    r["tflops_algorithmic"] = r["images_per_s"] * res["flops_per_image"][geom.name]["total"] / 1e12
                    det.append(r)
                    print(json.dumps(r), flush=True)
                s.close()
                del s
                torch.cuda.empty_cache()
        res["detector"] = det
        res["search_b16"] = run_search(torch, np, "f32x3", args.search_runs)
        print(json.dumps(res["search_b16"]), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
