#!/usr/bin/env python
"""What a smaller detector input buys on one MI355X: OWL-ViT B/32 at 768 x 768 against 448 x 768 and 384 x 800 (f32x3 mode).

  python tools/bench_owl_input_size.py --out profiles/owl_input_size_measure          # writes <out>.json and <out>.md
  python tools/bench_owl_input_size.py --part default --out DIR/name                  # only the default-size figures (the
        part that is also run from a checkout of the parent commit, in the same session on the same board: the two JSON files
        are then passed back with --parent-json / --parent-bench / --this-bench for the regression table)

* detector: ``OwlScorer.score`` at B = 256 and B = 10 on verification-sized images (285 x 600), per input size: images/s
  (device events), and the per-kernel figures of the library's own event profiler (GEMM and attention: algorithmic TFLOP/s);
* attention alone at T = 337 (448 x 768: ten full key tiles + one masked tile of 17 keys) against T = 577 (eighteen full
  tiles + the folded straggler key), the three kernels at B = 256: algorithmic TFLOP/s, and the time per key tile;
* searches: the configs[1] shape (N = 3600, 16 x 16 grid, K = 8, budget 1000, threshold 0.6, seed 2025) and a reference-
  default 4 x 4 solo search, at 448 x 768 against 768 x 768;
* default-size regression: the T = 577 attention microbenchmark of this tree (and, given the files, the parent's and the
  headline ``bench.py`` lines of both).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(768, 768), (448, 768), (384, 800)]


def flops_per_image(ntok, npatch, patch_k=3072):
    D, FF, L = 768, 3072, 12
    gemm_layer = 2.0 * ntok * (3 * D * D + D * D + 2 * D * FF)
    attn_layer = 4.0 * ntok * ntok * D
    patch = 2.0 * npatch * D * patch_k
    heads = 2.0 * npatch * (512 * D + 2 * D * D + 4 * D)
    total = L * (gemm_layer + attn_layer) + patch + heads
    return dict(total=total, attention_fraction=L * attn_layer / total)


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


def make_scorer(size, max_batch, mode="f32x3"):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    from tstar_amd.tokenizer import encode_queries
    kw = {} if size is None else dict(input_size=size)          # None: no keyword at all (runs on the parent commit too)
    sd = W.synthetic_state_dict(0)
    if size is None:
        vb = W.pack_blob(sd, W.vision_spec())
    else:
        g = W.with_input_size(W.B32, size)
        vb = W.pack_blob(sd, W.vision_spec(g), g)
    s = OwlScorer(vb, W.pack_blob(sd, W.text_spec()), max_batch=max_batch, weights_mode=mode, **kw)
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    s.set_queries(ids, am, [1.0, 0.5, 0.5, 0.5])
    return s


def prof_read(lib, cat):
    from tstar_amd import _lib
    n, ms, fl = C.c_longlong(0), C.c_double(0), C.c_double(0)
    _lib.check(lib.tstar_prof_read(cat, C.byref(n), C.byref(ms), C.byref(fl)))
    return dict(launches=n.value, ms=ms.value, tflops=(fl.value / (ms.value * 1e-3) / 1e12) if ms.value > 0 else 0.0)


def detector(torch, size, warmup, reps):
    from tstar_amd import _lib
    lib = _lib.load()
    s = make_scorer(size, 256)
    ntok = s.num_patches + 1
    fl = flops_per_image(ntok, s.num_patches)
    out = []
    for B in (256, 10):
        g = torch.Generator(device="cuda").manual_seed(B)
        imgs = torch.randint(0, 256, (B, 285, 600, 3), dtype=torch.uint8, device="cuda", generator=g)
        ms = event_ms(torch, lambda: s.score(imgs, 1, 1), warmup, reps if B > 10 else 4 * reps)
        _lib.check(lib.tstar_prof_enable(1))                        # a second, separately timed pass: every launch bracketed by events
        for _ in range(2):
            s.score(imgs, 1, 1)
        torch.cuda.synchronize()
        gemm, attn = prof_read(lib, 0), prof_read(lib, 1)
        _lib.check(lib.tstar_prof_enable(0))
        out.append(dict(input_size=list(size or (768, 768)), tokens=ntok, B=B, ms_per_call=ms, images_per_s=B / (ms / 1e3),
                        tflops_algorithmic=B / (ms / 1e3) * fl["total"] / 1e12, gflop_per_image=fl["total"] / 1e9,
                        attention_fraction_of_flop=fl["attention_fraction"], gemm_kernels=gemm, attention_kernel=attn))
        print(json.dumps(out[-1]), flush=True)
    s.close()
    del s
    torch.cuda.empty_cache()
    return out


def attention_alone(torch, Ts, B=256, heads=12):
    from tstar_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for T in Ts:
        qkv = torch.randn(B * T, 3 * heads * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
        o = torch.empty(B * T, heads * 64, device="cuda")
        calls = {"f32": lambda: lib.tstar_attention_f32(qkv.data_ptr(), o.data_ptr(), B, T, heads, 0, None, st),
                 "split": lambda: lib.tstar_attention_split(qkv.data_ptr(), o.data_ptr(), B, T, heads, st),
                 "x3": lambda: lib.tstar_attention_x3(qkv.data_ptr(), o.data_ptr(), B, T, heads, st)}
        for name, f in calls.items():
            ms = event_ms(torch, lambda: _lib.check(f()), 3, 20)
            tiles = (T + 31) // 32 if T % 32 != 1 else T // 32       # key tiles on the matrix pipe (T = 32 n + 1: the last key is VALU work)
            out.append(dict(kernel=name, T=T, B=B, heads=heads, ms=ms, tflops_algorithmic=4.0 * B * heads * T * T * 64 / ms / 1e9,
                            key_tiles=tiles, masked_tile_keys=(T % 32 if T % 32 not in (0, 1) else 0),
                            us_per_key_tile_and_query_block=ms * 1e3 / tiles / ((T + 127) // 128)))
            print(json.dumps(out[-1]), flush=True)
    return out


def search(torch, np, size, grid, nframes, budget, runs, label):
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    kw = {} if size is None else dict(input_size=size)
    h = OWLInterface(synthetic_seed=0, max_batch=256, weights_dtype="f32x3", **kw)
    store = synthetic_video(nframes, seed=0)
    out = []
    for r in range(runs + 1):                                        # run 0 warms up (tables, lane 1, spline workers)
        s = TStarSearcher(store, h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(grid, grid), search_budget=budget,
                          confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ts = s.search()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r > 0:
            out.append(dict(s_per_video=dt, frames_scored=s.frames_scored, iterations=s.iterations, keyframes=[float(t) for t in ts]))
    del h
    torch.cuda.empty_cache()
    res = dict(search=label, input_size=list(size or (768, 768)), N=nframes, grid=grid, K=8, budget=budget, seed=2025, runs=out,
               median_s_per_video=float(np.median([o["s_per_video"] for o in out])))
    print(json.dumps(res), flush=True)
    return res


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f if ln.startswith("{")]
    return json.loads(lines[-1])


def write_md(res, path):
    L = ["# OWL-ViT B/32 input size on one MI355X (f32x3 mode)", "",
         f"Device: {res['device']}.  Written by `tools/bench_owl_input_size.py`; the JSON next to this file holds every figure.", ""]
    if "detector" in res:
        L += ["## Detector, 285 x 600 images", "",
              "| input | tokens | B | images/s | x 768x768 | GFLOP/image | TFLOP/s (alg.) | GEMM kernels TFLOP/s | attention kernel TFLOP/s |",
              "|---|---|---|---|---|---|---|---|---|"]
        base = {d["B"]: d["images_per_s"] for d in res["detector"] if d["input_size"] == [768, 768]}
        for d in res["detector"]:
            L.append(f"| {d['input_size'][0]}x{d['input_size'][1]} | {d['tokens']} | {d['B']} | {d['images_per_s']:.0f} | "
                     f"{d['images_per_s'] / base[d['B']]:.2f} | {d['gflop_per_image']:.1f} | {d['tflops_algorithmic']:.0f} | "
                     f"{d['gemm_kernels']['tflops']:.0f} | {d['attention_kernel']['tflops']:.0f} |")
        L.append("")
    if "attention" in res:
        L += ["## Attention alone, B = 256, 12 heads", "",
              "| kernel | T | key tiles (masked keys in the last) | ms | TFLOP/s (alg.) | us per key tile and 128-query block |", "|---|---|---|---|---|---|"]
        for a in res["attention"]:
            L.append(f"| {a['kernel']} | {a['T']} | {a['key_tiles']} ({a['masked_tile_keys']}) | {a['ms']:.3f} | {a['tflops_algorithmic']:.1f} | "
                     f"{a['us_per_key_tile_and_query_block']:.2f} |")
        L += ["", "T = 337 runs 11 key tiles for 10.53 tiles of keys: the masked tile issues a full tile of MFMAs for 17 keys, so the "
              "algorithmic rate is at most 337 / 352 = 0.957 of what the same kernel reaches on full tiles, before the shorter "
              "loop (11 iterations against 18 for the same prologue and epilogue) and the three query blocks of 128 for 337 queries "
              "(2.63 blocks of work) are counted.", ""]
    if "searches" in res:
        L += ["## Searches (3600-frame synthetic video, K = 8, threshold 0.6, seed 2025)", "",
              "| search | input | s per video (median) | frames scored | iterations | detector images | ms per detector image |",
              "|---|---|---|---|---|---|---|"]
        for s in res["searches"]:
            r = s["runs"][-1]
            images = r["iterations"] + r["frames_scored"] - r["iterations"] * s["grid"] ** 2       # one grid image per iteration + the verification frames
            L.append(f"| {s['search']} | {s['input_size'][0]}x{s['input_size'][1]} | {s['median_s_per_video']:.3f} | {r['frames_scored']} | "
                     f"{r['iterations']} | {images} | {s['median_s_per_video'] * 1e3 / images:.2f} |")
        L += ["", "With synthetic weights the scores at two input sizes differ, so the two searches of a row pair do not verify the same "
              "frames (fewer cells pass the threshold at 448 x 768 here): seconds per video mixes the cheaper forward with the shorter "
              "verification batches.  The last column divides them out; it still contains the grid images' resampling from 1520 x 3200 "
              "and, in the solo search, the per-iteration host work that no input size changes.", ""]
    if "default_regression" in res:
        R = res["default_regression"]
        L += ["## Default size (768 x 768): this commit against its parent, same session, same board", "",
              "| figure | parent | this commit | ratio |", "|---|---|---|---|"]
        for row in R["rows"]:
            ratio = f"{row['this'] / row['parent']:.3f}" if row.get("parent") else "-"
            parent = f"{row['parent']:.1f}" if row.get("parent") else "-"
            L.append(f"| {row['figure']} | {parent} | {row['this']:.1f} | {ratio} |")
        L += ["", R.get("note", ""), ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="path without extension: <out>.json and <out>.md are written")
    ap.add_argument("--part", choices=["all", "default"], default="all")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search-runs", type=int, default=3)
    ap.add_argument("--root", default=None, help="import tstar_amd from this checkout instead (a built tree of the parent commit, with --part default)")
    ap.add_argument("--parent-json", default=None, help="<out>.json of `--part default` run from a checkout of the parent commit")
    ap.add_argument("--parent-bench", default=None, help="output of the parent's `bench.py --gpus 1 --steps K --warmup W`")
    ap.add_argument("--this-bench", default=None, help="output of this commit's bench.py, same command")
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), mode="f32x3")
    if args.part == "default":
        res["attention"] = attention_alone(torch, [577])
        res["detector"] = detector(torch, None, args.warmup, args.reps)
    else:
        res["detector"] = [d for size in SIZES for d in detector(torch, size, args.warmup, args.reps)]
        res["attention"] = attention_alone(torch, [577, 337])
        res["searches"] = []
        for label, grid in (("configs[1]: 16 x 16 grid, budget 1000", 16), ("reference default: 4 x 4 grid, solo", 4)):
            for size in ((768, 768), (448, 768)):
                res["searches"].append(search(torch, np, size, grid, 3600, 1000, args.search_runs, label))
        rows = []
        this_attn = {a["kernel"]: a for a in res["attention"] if a["T"] == 577}
        parent = json.load(open(args.parent_json)) if args.parent_json else None
        p_attn = {a["kernel"]: a for a in parent["attention"]} if parent else {}
        for k in ("f32", "split", "x3"):
            rows.append(dict(figure=f"attention {k}, T = 577, B = 256: TFLOP/s", this=this_attn[k]["tflops_algorithmic"],
                             parent=p_attn.get(k, {}).get("tflops_algorithmic")))
        if parent:
            pd = {d["B"]: d for d in parent["detector"]}
            for d in res["detector"]:
                if d["input_size"] == [768, 768]:
                    rows.append(dict(figure=f"detector 768x768, B = {d['B']}: images/s", this=d["images_per_s"], parent=pd[d["B"]]["images_per_s"]))
        if args.this_bench:
            tb = last_json_line(args.this_bench)
            pb = last_json_line(args.parent_bench) if args.parent_bench else None
            rows.append(dict(figure=f"bench.py --gpus 1 --steps {tb['steps']} --warmup {tb['warmup']}: frames/s", this=tb["value"],
                             parent=pb["value"] if pb else None))
        res["default_regression"] = dict(rows=rows, note="The README states a +- 3 % board-to-board spread for the headline figure; "
                                         "ratios inside 0.97 .. 1.03 are agreement.")
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".json", "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        write_md(res, args.out + ".md")


if __name__ == "__main__":
    main()
