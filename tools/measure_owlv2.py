#!/usr/bin/env python
"""OWLv2 B/16 on one MI355X, beside OWL-ViT B/16 at the same input size (960 x 960, T = 3601: the same forward FLOP).

  python tools/measure_owlv2.py --out profiles/owlv2_measure          # writes <out>.json and <out>.md
        [--this-bench FILE ... --parent-bench FILE ...]                # outputs of `bench.py --gpus 1 --steps 16 --warmup 2` of this
                                                                       # commit and of its parent, run alternated in the same session

* detector: ``OwlScorer.score`` images/s of both families at B = 16 and B = 164 (the chunk limit at 3600 patches) in f32x3 and
  f32, the two sides alternated, ``--rounds`` repeats each: the spread of the repeats is reported beside the gap;
* pre-processing alone (``debug_preprocess``, device events): the direct form on 285 x 600 frames and the filtered form on
  1520 x 3200 grid images, beside OWL-ViT's bicubic pair at the same output size, and against the bytes floor (the u8 source in
  once, 960 * 960 * 3 float32 = 11.06 MB of im2col out per image);
* pre-processing share of the OWLv2 forward at B = 16;
* one reference-default 4 x 4 solo search with a synthetic OWLv2 heuristic.
A gap between the two families larger than the reported spread wants a per-kernel look: run one family per process under
``rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python -c "..."`` (the scorer of ``make_scorer(family, 164,
"f32x3")`` on ``images(torch, 164, 285, 600, 164)``) and compare the two ``kernel_stats.csv`` by kernel name.
Synthetic weights throughout: detection QUALITY with real OWLv2 weights is not measured (no checkpoint is on disk)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E, vendor figure: the floor below is bytes / this


def event_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make_scorer(family, max_batch, mode):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    from tstar_amd.tokenizer import encode_queries
    g = W.OWLV2_B16 if family == "owlv2" else W.with_input_size(W.B16, (960, 960))
    sd = W.synthetic_state_dict(0, geometry=g)
    s = OwlScorer(W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.text_spec(g)), max_batch=max_batch, weights_mode=mode,
                  patch_size=16, input_size=(960, 960), family=family)
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    s.set_queries(ids, am, [1.0, 0.5, 0.5, 0.5])
    return s


def images(torch, B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)


def detector(torch, np, mode, rounds):
    scorers = {f: make_scorer(f, 164, mode) for f in ("owlvit", "owlv2")}
    out = []
    for B, reps in ((16, 4), (164, 1)):
        imgs = images(torch, B, 285, 600, B)
        runs = {f: [] for f in scorers}
        for r in range(rounds + 1):                                  # round 0 warms both sides up
            for f, s in (list(scorers.items())[::-1] if r % 2 else scorers.items()):      # alternated, and the order too
                ms = event_ms(torch, lambda: s.score(imgs, 1, 1), 0 if r else 1, reps)
                if r:
                    runs[f].append(B / (ms / 1e3))
        row = dict(mode=mode, B=B, images_per_s=runs)
        for f in runs:
            row[f + "_median"] = float(np.median(runs[f]))
            row[f + "_spread"] = float((max(runs[f]) - min(runs[f])) / np.median(runs[f]))
        row["owlv2_over_owlvit"] = row["owlv2_median"] / row["owlvit_median"]
        out.append(row)
        print(json.dumps(row), flush=True)
    for s in scorers.values():
        s.close()
    torch.cuda.empty_cache()
    return out


def preprocessing(torch, np, rounds):
    scorers = {f: make_scorer(f, 16, "f32x3") for f in ("owlvit", "owlv2")}
    out = []
    B = 16
    for H, W, form in ((285, 600, "direct"), (1520, 3200, "filtered")):
        imgs = images(torch, B, H, W, H)
        runs = {f: [] for f in scorers}
        for r in range(rounds + 1):
            for f, s in (list(scorers.items())[::-1] if r % 2 else scorers.items()):
                ms = event_ms(torch, lambda: s.debug_preprocess(imgs), 0 if r else 2, 10)
                if r:
                    runs[f].append(ms * 1e3 / B)
        assert scorers["owlv2"].preprocess_form() == (0 if form == "direct" else 1)
        bytes_per_image = H * W * 3 + 960 * 960 * 3 * 4
        us = {f: float(np.median(v)) for f, v in runs.items()}
        row = dict(source=[H, W], form=form, B=B, us_per_image=us, us_per_image_runs=runs, bytes_per_image=bytes_per_image,
                   floor_us=bytes_per_image / (HBM_PEAK_GBS * 1e3), owlv2_gb_per_s=bytes_per_image / us["owlv2"] / 1e3)
        out.append(row)
        print(json.dumps(row), flush=True)
    # share of the forward: the same B = 16 frames through score()
    imgs = images(torch, B, 285, 600, 16)
    fwd = event_ms(torch, lambda: scorers["owlv2"].score(imgs, 1, 1), 1, 4) * 1e3 / B
    share = dict(B=B, forward_us_per_image=fwd, preprocess_us_per_image=out[0]["us_per_image"]["owlv2"],
                 share=out[0]["us_per_image"]["owlv2"] / fwd)
    imgs = images(torch, B, 1520, 3200, 17)
    fwd = event_ms(torch, lambda: scorers["owlv2"].score(imgs, 1, 1), 1, 4) * 1e3 / B
    share_grid = dict(B=B, forward_us_per_image=fwd, preprocess_us_per_image=out[1]["us_per_image"]["owlv2"],
                      share=out[1]["us_per_image"]["owlv2"] / fwd)
    print(json.dumps(dict(share_frames=share, share_grid_images=share_grid)), flush=True)
    for s in scorers.values():
        s.close()
    torch.cuda.empty_cache()
    return out, share, share_grid


def search(torch, np, runs):
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    h = OWLInterface(model_name_or_path="google/owlv2-base-patch16-ensemble", synthetic_seed=0, max_batch=164, weights_dtype="f32x3")
    store = synthetic_video(3600, seed=0)
    out = []
    for r in range(runs + 1):                                        # run 0 warms up (tables, lane 1, spline workers)
        s = TStarSearcher(store, h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(4, 4), search_budget=1000,
                          confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.search()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r > 0:
            out.append(dict(s_per_video=dt, frames_scored=s.frames_scored, iterations=s.iterations))
    res = dict(N=3600, grid=4, K=8, budget=1000, seed=2025, runs=out, median_s_per_video=float(np.median([o["s_per_video"] for o in out])))
    print(json.dumps(res), flush=True)
    del h
    torch.cuda.empty_cache()
    return res


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f if ln.startswith("{")]
    return json.loads(lines[-1])


def write_md(res, path):
    L = ["# OWLv2 B/16 on one MI355X", "",
         f"Device: {res['device']}.  Written by `tools/measure_owlv2.py`; the JSON next to this file holds every figure.  Synthetic "
         "weights throughout: detection quality with real OWLv2 weights is NOT measured (no checkpoint is on disk).", "",
         "## Detector at 960 x 960 (T = 3601), 285 x 600 images: OWLv2 against OWL-ViT B/16 with `input_size=(960, 960)`", "",
         "The two sides run the same forward FLOP; they differ in the pre-processing kernels only.  Alternated in one session, the order of the two sides reversed every round.", "",
         "| mode | B | OWL-ViT B/16 images/s (spread) | OWLv2 images/s (spread) | OWLv2 / OWL-ViT |", "|---|---|---|---|---|"]
    for d in res["detector"]:
        L.append(f"| {d['mode']} | {d['B']} | {d['owlvit_median']:.1f} ({100 * d['owlvit_spread']:.1f} %) | {d['owlv2_median']:.1f} "
                 f"({100 * d['owlv2_spread']:.1f} %) | {d['owlv2_over_owlvit']:.3f} |")
    L += ["", "Spread = (max - min) / median over the repeats of one side.", "",
          "## Pre-processing alone (B = 16, output 960 x 960, device events)", "",
          "| source | OWLv2 form | OWLv2 us/image | bicubic pair us/image | bytes/image | floor at 8 TB/s, us | OWLv2 GB/s |", "|---|---|---|---|---|---|---|"]
    for p in res["preprocessing"]:
        L.append(f"| {p['source'][0]} x {p['source'][1]} | {p['form']} | {p['us_per_image']['owlv2']:.1f} | {p['us_per_image']['owlvit']:.1f} | "
                 f"{p['bytes_per_image'] / 1e6:.2f} MB | {p['floor_us']:.2f} | {p['owlv2_gb_per_s']:.0f} |")
    for name, s in (("285 x 600 frames", res["share_frames"]), ("1520 x 3200 grid images", res["share_grid_images"])):
        L += ["", f"Share of the OWLv2 forward at B = 16 in f32x3, {name}: {s['preprocess_us_per_image']:.1f} us of "
              f"{s['forward_us_per_image']:.0f} us per image = {100 * s['share']:.2f} %."]
    if "search" in res:
        s = res["search"]
        L += ["", "## Reference-default 4 x 4 solo search, synthetic OWLv2 heuristic (f32x3, 3600-frame synthetic video, K = 8)", "",
              f"{s['median_s_per_video']:.3f} s per video (median of {len(s['runs'])}; {s['runs'][-1]['frames_scored']} frames scored in "
              f"{s['runs'][-1]['iterations']} iterations)."]
    if res.get("bench"):
        b = res["bench"]
        L += ["", "## `bench.py --gpus 1 --steps 16 --warmup 2` (OWL-ViT B/32 default): this commit against its parent, alternated", "",
              "| run | parent | this commit |", "|---|---|---|"]
        for i, (p, t) in enumerate(zip(b["parent"], b["this"])):
            L.append(f"| {i + 1} | {p:.1f} | {t:.1f} |")
        L += ["", f"Mean ratio this / parent: {b['ratio']:.4f} (the README states +- 3 % board-to-board for this figure)."]
    L += ["", res.get("notes", ""), ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="path without extension: <out>.json and <out>.md are written")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--search-runs", type=int, default=2)
    ap.add_argument("--this-bench", nargs="*", default=[])
    ap.add_argument("--parent-bench", nargs="*", default=[])
    ap.add_argument("--notes", default="", help="a paragraph appended to the .md (what a profile run explained, if a gap needed it)")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), notes=args.notes)
    res["preprocessing"], res["share_frames"], res["share_grid_images"] = preprocessing(torch, np, args.rounds)
    res["detector"] = [d for mode in ("f32x3", "f32") for d in detector(torch, np, mode, args.rounds)]
    res["search"] = search(torch, np, args.search_runs)
    if args.this_bench and args.parent_bench:
        t = [last_json_line(p)["value"] for p in args.this_bench]
        p = [last_json_line(q)["value"] for q in args.parent_bench]
        res["bench"] = dict(this=t, parent=p, ratio=float(np.mean(t) / np.mean(p)))
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".json", "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        write_md(res, args.out + ".md")


if __name__ == "__main__":
    main()
