#!/usr/bin/env python
"""Dataset run in the shape of the reference's LVHaystackBench/run_TStar_onDataset.py:149-213, on MI355X:
items are sharded over the ranks (one process per GPU), each rank advances its items in lock-step
groups, the keyframe indices are all-gathered (RCCL) and rank 0 writes the reference's result JSON
(video_path, grounding_objects, keyframe_timestamps, keyframe_distribution).

Grounding (question -> target / cue objects) is a remote VLM call in the reference and is out of scope
here: every item carries its objects.  Videos are synthetic:// URLs (BASELINE configs[2]: the real
LV-Haystack split needs network) unless --videos names files: anything tstar_amd.video.open_video reads --
a Motion-JPEG .avi, a .mjpeg stream, a folder of .jpg frames (--video-fps for the latter two), .y4m, ...

  python examples/run_dataset.py --items 8 --out /tmp/results.json
  python examples/run_dataset.py --videos clips/a.avi clips/b_frames/ --video-fps 1
  python examples/run_dataset.py --query-image mug=shots/my_mug.png --query-image dog=shots/rex.jpg
  python examples/run_dataset.py --query-image mug=shots/desk.png@120,40,260,210
  python examples/run_dataset.py --items 4 --questions-per-video 4 --feature-cache 2400
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/run_dataset.py --items 32
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUESTIONS = [(["couch"], ["tv", "chair"]), (["dog"], ["leash", "park bench"]), (["red car"], ["road"]),
             (["laptop", "mug"], ["desk"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--nframes", type=int, default=600)
    ap.add_argument("--search-nframes", type=int, default=8)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--lockstep", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default="./output/tstar_results.json")
    ap.add_argument("--owl-model", default="google/owlvit-base-patch32",
                    help="OWL-ViT or OWLv2 checkpoint (name or directory; OWL-ViT B/32 or B/16, OWLv2 B/16); when none is on disk, seeded "
                         "synthetic weights: B/32, or OWLv2 B/16 for a name containing 'owlv2' (e.g. google/owlv2-base-patch16-ensemble)")
    ap.add_argument("--owl-input-size", default=None, metavar="HxW",
                    help="detector input size, e.g. 448x768 (each side a multiple of the patch size; default: the checkpoint's 768x768, "
                         "or TSTAR_INPUT_SIZE)")
    ap.add_argument("--videos", nargs="+", default=None,
                    help="video files / JPEG frame folders to search instead of synthetic videos (one item each; overrides --items)")
    ap.add_argument("--video-fps", type=float, default=None,
                    help="frame rate of JPEG frame folders (default 1) and .mjpeg streams (default 25) among --videos")
    ap.add_argument("--jpeg-entropy", choices=("host", "device"), default=None,
                    help="where Motion-JPEG / JPEG-folder videos are entropy-decoded (default: TSTAR_JPEG_ENTROPY, else host); "
                         "'device' keeps the Huffman decode off the rank's CPUs")
    ap.add_argument("--jpeg-resident", nargs="?", type=int, const=0, default=None, metavar="N",
                    help="keep Motion-JPEG / JPEG-folder videos compressed in HBM and decode frames on demand into a pool of N slots "
                         "(default 512; sets TSTAR_JPEG_RESIDENT / TSTAR_JPEG_POOL): same results from a fraction of the memory")
    ap.add_argument("--jpeg-scale", type=int, choices=(1, 2, 4, 8), default=None, metavar="N",
                    help="decode Motion-JPEG / JPEG-folder videos at 1/N size (2, 4 or 8; sets TSTAR_JPEG_SCALE), byte for byte Pillow's "
                         "draft: the store shrinks by N * N, and the search sees the smaller frames (boxes are in their pixels)")
    ap.add_argument("--jpeg-recode", type=int, default=None, metavar="N",
                    help="with --jpeg-resident: re-code the compressed videos losslessly at open with a restart interval of N MCUs "
                         "(1..65535; sets TSTAR_JPEG_RECODE), so that fetches decode one lane per interval: same pixels, same results")
    ap.add_argument("--jpeg-recode-optimize", action="store_true",
                    help="with --jpeg-recode: write the re-coded frames with optimised Huffman tables, one set per group of frames "
                         "(sets TSTAR_JPEG_RECODE_OPTIMIZE): a smaller arena, same pixels, same results")
    ap.add_argument("--query-image", action="append", default=[], metavar="NAME=PATH[@x0,y0,x1,y1]",
                    help="example image of an object (repeatable): every target / cue object called NAME is searched for by the "
                         "image-guided query embedded from PATH instead of by its text; @x0,y0,x1,y1 (pixels of that image) "
                         "means only that region of it")
    ap.add_argument("--questions-per-video", type=int, default=1,
                    help="items per synthetic video: the reference's dataset asks many questions of one video (each with its own objects)")
    ap.add_argument("--feature-cache", type=int, default=None, metavar="N",
                    help="keep the detector's frame records of up to N verification frames on the device (default: TSTAR_FEATURE_CACHE, "
                         "else off): later questions about a video skip the vision tower for frames an earlier one verified; same results")
    ap.add_argument("--keyframe-jpegs", default=None, metavar="DIR",
                    help="write the K keyframes of each item as DIR/<item>/<second>.jpg, encoded on the device from the resident store "
                         "(Pillow's default JPEG bytes; the reference's keyframe writer, TStarFramework.py:136-146)")
    ap.add_argument("--save-mjpeg", default=None, metavar="DIR",
                    help="write each opened video once as DIR/<name>.avi (Motion-JPEG, quality 90, 1 frame per second), skipped when the "
                         "file is there: a later run passes those files as --videos and opens them through the device decode path")
    ap.add_argument("--jpeg-optimize", action="store_true",
                    help="write the JPEGs of --keyframe-jpegs and --save-mjpeg with Huffman tables built from each frame's own statistics "
                         "(Pillow's optimize=True, byte for byte): smaller files, the same pixels")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    from tstar_amd.interface_heuristic import initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.lockstep import search_lockstep_groups
    from tstar_amd.results import make_result, save_results
    from tstar_amd.sharding import gather_keyframes, interleave_by_item, item_seed, shard_items

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        # torch.distributed is only the control plane (gloo); the one data collective -- the all-gather of keyframe rows -- goes over RCCL
        # through the library's own communicator (tstar_amd.sharding), or over gloo with TSTAR_BENCH_BACKEND=gloo / when RCCL cannot come up
        from tstar_amd import sharding as _shard
        _shard.PREFER_RCCL = os.environ.get("TSTAR_BENCH_BACKEND", "nccl") == "nccl"
        dist.init_process_group("gloo")

    if args.jpeg_entropy is not None:
        os.environ["TSTAR_JPEG_ENTROPY"] = args.jpeg_entropy       # the searcher opens paths itself: the variable reaches it too
    if args.jpeg_resident is not None:
        os.environ["TSTAR_JPEG_RESIDENT"] = "1"
        if args.jpeg_resident > 0:
            os.environ["TSTAR_JPEG_POOL"] = str(args.jpeg_resident)
    if args.jpeg_scale is not None:
        os.environ["TSTAR_JPEG_SCALE"] = str(args.jpeg_scale)
    if args.jpeg_recode is not None:
        if args.jpeg_resident is None:
            ap.error("--jpeg-recode re-codes the arena of a compressed-resident store: it needs --jpeg-resident")
        os.environ["TSTAR_JPEG_RECODE"] = str(args.jpeg_recode)
    if args.jpeg_recode_optimize:
        if args.jpeg_recode is None:
            ap.error("--jpeg-recode-optimize optimises the tables of a re-coded arena: it needs --jpeg-recode")
        os.environ["TSTAR_JPEG_RECODE_OPTIMIZE"] = "1"
    per_video = max(1, args.questions_per_video)
    paths = args.videos if args.videos else [f"synthetic://n={args.nframes},seed={100 + i // per_video}" for i in range(args.items * per_video)]
    items = [{"video_path": p, "targets": QUESTIONS[i % 4][0], "cues": QUESTIONS[i % 4][1]} for i, p in enumerate(paths)]
    stores = {}

    def video_of(i):
        """What the searcher gets: ONE resident FrameStore per distinct video_path of this rank -- a video asked several questions is
        decoded once, and the detector's frame records (--feature-cache) are keyed by the store."""
        from tstar_amd.video import open_video
        p = items[i]["video_path"]
        if p not in stores:
            if args.video_fps is not None and (os.path.isdir(p) or p.lower().endswith((".mjpeg", ".mjpg"))):
                stores[p] = open_video(p, fps=args.video_fps, jpeg_entropy=args.jpeg_entropy)
            else:
                stores[p] = open_video(p)
            if args.save_mjpeg:
                import re
                os.makedirs(args.save_mjpeg, exist_ok=True)
                out = os.path.join(args.save_mjpeg, re.sub(r"[^A-Za-z0-9._-]+", "_", os.path.splitext(os.path.basename(p.rstrip("/")))[0] or "video") + ".avi")
                if not os.path.exists(out):
                    stores[p].save_mjpeg(out, quality=90, optimize=args.jpeg_optimize)
        return stores[p]

    owl_kw = {}
    if args.owl_input_size is not None:
        try:
            owl_kw["input_size"] = tuple(int(v) for v in args.owl_input_size.lower().split("x"))
        except ValueError:
            ap.error(f"--owl-input-size must look like HEIGHTxWIDTH, not {args.owl_input_size!r}")
    if args.feature_cache is not None:
        owl_kw["feature_cache_frames"] = args.feature_cache
    heuristic = initialize_heuristic("owl-vit", model_name_or_path=args.owl_model, synthetic_seed=0, max_batch=64,
                                     device=f"cuda:{local}", **owl_kw)
    query_images = {}
    for spec in args.query_image:
        name, sep, path = spec.partition("=")
        box = None
        head, at, tail = path.rpartition("@")
        if at and tail.count(",") == 3:
            try:
                box = tuple(float(v) for v in tail.split(","))
                path = head
            except ValueError:
                ap.error(f"--query-image: the box of {spec!r} must be four numbers x0,y0,x1,y1")
        if not sep or not name.strip() or not path:
            ap.error(f"--query-image must look like NAME=PATH or NAME=PATH@x0,y0,x1,y1, not {spec!r}")
        query_images[name.strip()] = path if box is None else (path, box)
    if query_images:
        heuristic.set_query_images(query_images)
    mine = shard_items(len(items), world, rank)
    uses = {}                                          # items of this rank that still need each video
    for i in mine:
        uses[items[i]["video_path"]] = uses.get(items[i]["video_path"], 0) + 1
    rows, dists = [], {}
    # two lock-step groups alternate on the GPU: one group's host bookkeeping runs under the other's verification batch
    L = max(1, min(args.lockstep, 31))
    for g0 in range(0, len(mine), 2 * L):
        groups = [mine[g1:g1 + L] for g1 in range(g0, min(g0 + 2 * L, len(mine)), L)]
        sss = [[TStarSearcher(video_of(i), heuristic, list(items[i]["targets"]), list(items[i]["cues"]),
                              search_nframes=args.search_nframes, image_grid_shape=(args.grid, args.grid),
                              search_budget=1000, confidence_threshold=0.6,
                              rng=np.random.RandomState(item_seed(args.seed, i)), keep_visual_history=False) for i in group]
               for group in groups]
        for group, ss, res in zip(groups, sss, search_lockstep_groups(sss)):
            for i, s, (frames, ts) in zip(group, ss, res):
                rows.append([int(t) for t in ts])
                if args.keyframe_jpegs:
                    d = os.path.join(args.keyframe_jpegs, f"{i:05d}")
                    os.makedirs(d, exist_ok=True)
                    for t, data in zip(rows[-1], video_of(i).jpeg_frames(rows[-1], optimize=args.jpeg_optimize)):
                        with open(os.path.join(d, f"{t}.jpg"), "wb") as f:
                            f.write(data)
                dists[i] = s.P_history[-1] if s.P_history else []
                uses[items[i]["video_path"]] -= 1
                if uses[items[i]["video_path"]] == 0:      # the last question about this video: its frames (and frame records) can go
                    stores.pop(items[i]["video_path"], None)
    gathered = gather_keyframes(rows, world, pad_to=(len(items) + world - 1) // world)
    if world > 1:
        gathered = interleave_by_item(gathered, len(items), world)
        parts = [None] * world                         # the per-second distributions (N floats per item) ride along
        dist.all_gather_object(parts, dists)
        dists = {k: v for d in parts for k, v in d.items()}
    if heuristic.feature_cache is not None:
        st = heuristic.feature_cache_stats()
        print(f"rank {rank}: feature cache {st['used']}/{st['slots']} records, {st['hits']} hits, {st['misses']} misses, {st['uncached']} uncached")
    if rank == 0:
        results = [make_result(it["video_path"], it["targets"], it["cues"], [float(t) for t in gathered[i]], dists.get(i, []))
                   for i, it in enumerate(items)]
        save_results(results, args.out)
        print(f"{len(results)} items -> {args.out}; item 0 keyframes {results[0]['keyframe_timestamps']}")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
