#!/usr/bin/env python
"""HF's image-guided post-process on one MI355X: what the HIP kernel costs beside HF's own CPU method.

  python tools/measure_image_guided_post.py --out profiles/image_guided_post_measure.md [--reps 20]
        [--this-bench FILE ... --parent-bench FILE ...]      # outputs of `bench.py --gpus 1 --steps 16 --warmup 2` of this commit and
                                                             # of its parent, run alternated in the same session

* ``tstar_image_guided_postprocess`` (h_scale_xy NULL: nothing but the launch is enqueued) between two HIP events, at np = 576 /
  B = 1, np = 3600 / B = 1 and np = 3600 / B = 16, threshold 0, nms_threshold 0.3, on two inputs: boxes that do not touch, so every
  candidate stays live and the sweep takes np - 1 steps (the worst case), and the scores / boxes of a real forward of the
  synthetic checkpoint (``OwlScorer.score(..., want_logits=True)`` against an image query at that patch count);
* HF's ``post_process_image_guided_detection`` on the same tensors on the CPU (host clock), when transformers is importable;
* ``OWLInterface.detect_image_guided`` end to end at B = 16 (host clock: upload, forward, post-process, download).
Warm-up calls first, then the median and the range of ``--reps`` timings.  Not on the search loop: no threshold is set."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fmt(ts, unit="ms"):
    return f"{statistics.median(ts):.3f} {unit} (min {min(ts):.3f}, max {max(ts):.3f})"


def event_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def host_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def disjoint_inputs(np_, B):
    import numpy as np
    import image_guided_post_util as G
    out = [G.make_image("disjoint", np_, np.random.RandomState(100 + b)) for b in range(B)]
    logits = np.stack([o[0] for o in out])
    return G.scores_of(logits[..., None]), np.stack([o[1] for o in out]), logits[..., None]


def forward_inputs(torch, np_, B):
    """Scores / boxes of a real forward: a synthetic B/32 checkpoint at the input size with np patches, an image query."""
    import numpy as np
    import image_query_util as U
    from tstar_amd.interface_heuristic import OWLInterface
    side = {576: (768, 768), 3600: (1920, 1920)}[np_]
    h = OWLInterface(synthetic_seed=0, max_batch=2, weights_dtype="f32x3", input_size=side)
    assert h.scorer.num_patches == np_
    example = U.example_images(41, 1, 120, 168)[0]
    r = h.scorer.embed_image_queries(torch.from_numpy(example[None]).cuda())
    h.scorer.set_query_embeds(r.embeds[:1], [1], [1.0], slot=1)
    nf = min(B, 2)                                               # two forwards' worth of images, repeated to B
    imgs = torch.from_numpy(U.example_images(50, nf, 360, 640)).cuda()
    sc = h.scorer.score(imgs, 1, 1, want_logits=True, image_sets=[1] * nf)
    torch.cuda.synchronize()
    reps = [-(-B // nf)] + [1, 1]
    out = tuple(np.tile(t.cpu().numpy(), reps[:t.dim()])[:B] for t in (sc.scores, sc.boxes_cxcywh, sc.logits))
    del h
    return out


def kernel_table(torch, lines, reps):
    import numpy as np
    import image_guided_post_util as G
    from tstar_amd import _lib
    lib = _lib.load()
    try:
        import transformers  # noqa: F401
        have_hf = True
    except ImportError:
        have_hf = False
    lines += ["## The post-process kernel (`tstar_image_guided_postprocess`, threshold 0, nms_threshold 0.3) beside HF's CPU method", "",
              "| input | np | B | kept per image | HIP kernel (two HIP events) | HF `post_process_image_guided_detection`, CPU | ratio |", "|---|---|---|---|---|---|---|"]
    for kind in ("disjoint", "forward"):
        for np_, B in ((576, 1), (3600, 1), (3600, 16)):
            scores, boxes, logits = disjoint_inputs(np_, B) if kind == "disjoint" else forward_inputs(torch, np_, B)
            d_s, d_b = torch.from_numpy(scores).cuda(), torch.from_numpy(boxes).cuda()
            a, x = torch.empty((B, np_), device="cuda"), torch.empty((B, np_, 4), device="cuda")
            k, cnt = torch.empty((B, np_), dtype=torch.uint8, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")

            def call():
                _lib.check(lib.tstar_image_guided_postprocess(d_s.data_ptr(), d_b.data_ptr(), B, np_, 0.0, 0.3, None, a.data_ptr(), x.data_ptr(),
                                                              k.data_ptr(), cnt.data_ptr(), _lib.stream_ptr()))

            t_dev = event_ms(torch, call, 3, reps)
            kept = cnt.cpu().numpy()
            want = G.host_entry(scores, boxes, 0.0, 0.3, None)
            assert np.array_equal(kept, want[3]) and np.array_equal(k.cpu().numpy(), want[2]) and G.same_bits(a.cpu().numpy(), want[0])
            if have_hf:
                t_hf = host_ms(lambda: G.hf_post_process(logits, boxes, 0.0, 0.3, None), 1, max(3, reps // 4))
                hf, ratio = fmt(t_hf), f"{statistics.median(t_hf) / statistics.median(t_dev):.0f} x"
            else:
                hf, ratio = "not measured (transformers is not importable)", "-"
            lines.append(f"| {kind} | {np_} | {B} | {int(kept.min())} .. {int(kept.max())} | {fmt(t_dev)} | {hf} | {ratio} |")
    lines += ["", "`disjoint`: a grid of boxes that do not touch; every candidate stays live, so the sweep takes np - 1 steps of one barrier each "
              "(the worst case; the rows not kept are those whose alpha is not above 0, score below a tenth of the best: none is suppressed).  "
              "`forward`: scores and boxes of a forward of the synthetic B/32 checkpoint at 768 x 768 (576 patches) and "
              "1920 x 1920 (3600 patches) against an image query.  One workgroup per image: B = 1 runs on one compute unit, B = 16 on sixteen.  "
              "The kernel's outputs were checked against the host entry in the same run.", ""]


def end_to_end(torch, lines, reps):
    import image_query_util as U
    from tstar_amd.interface_heuristic import OWLInterface
    h = OWLInterface(synthetic_seed=0, max_batch=16, weights_dtype="f32x3")
    example = U.example_images(41, 1, 120, 168)[0]
    targets = list(U.example_images(50, 16, 360, 640))
    t = host_ms(lambda: h.detect_image_guided(targets, example), 2, max(5, reps // 2))
    res = h.detect_image_guided(targets, example)
    kept = [len(r["patches"]) for r in res]
    lines += ["## `OWLInterface.detect_image_guided` end to end", "",
              f"B/32 at 768 x 768, f32x3, synthetic weights, one 120 x 168 example, sixteen 360 x 640 target images (host clock: example "
              f"embedding, upload, forward, post-process kernel, download): {fmt(t)}; kept per image {min(kept)} .. {max(kept)} of 576.", ""]
    del h


def bench_lines(lines, this_files, parent_files):
    def load(files):
        out = []
        for f in files:
            with open(f) as fh:
                for ln in fh:
                    ln = ln.strip()
                    if ln.startswith("{"):
                        out.append(json.loads(ln))
        return out

    def key(r):
        for k in ("value", "items_per_s", "throughput"):
            if k in r:
                return float(r[k])
        return None

    this, parent = load(this_files), load(parent_files)
    lines += ["## `bench.py --gpus 1 --steps 16 --warmup 2`, this commit and its parent alternated in one session", ""]
    for name, rs in (("this commit", this), ("parent", parent)):
        vals = [key(r) for r in rs if key(r) is not None]
        lines.append(f"- {name}: " + (", ".join(f"{v:.3f}" for v in vals) + f" (median {statistics.median(vals):.3f})" if vals else "no result line"))
    vt, vp = [key(r) for r in this if key(r) is not None], [key(r) for r in parent if key(r) is not None]
    if vt and vp:
        lines.append(f"- ratio of the medians: {statistics.median(vt) / statistics.median(vp):.4f} (the README states +- 3 % between runs)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_guided_post_measure.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--this-bench", nargs="*", default=[])
    ap.add_argument("--parent-bench", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_image_guided_post.py needs a HIP device: a CPU run measures nothing")
    lines = ["# Image-guided post-process: measurements", "",
             f"`tools/measure_image_guided_post.py --reps {args.reps}` on {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; one device; nothing else of this "
             f"project running on it).  Kernel times lie between two HIP events around the enqueued launch, after 3 warm-up calls; median "
             f"of {args.reps} (min, max).  CPU times are host-clock medians on the machine's CPU, torch {torch.__version__}.", ""]
    kernel_table(torch, lines, args.reps)
    end_to_end(torch, lines, args.reps)
    if args.this_bench or args.parent_bench:
        bench_lines(lines, args.this_bench, args.parent_bench)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
