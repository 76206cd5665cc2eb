#!/usr/bin/env python
"""Image-guided queries on one MI355X: what registering example images costs, and how far the device is from HF.

  python tools/measure_image_query.py --out profiles/image_query_measure.md
        [--this-bench FILE ... --parent-bench FILE ...]      # outputs of `bench.py --gpus 1 --steps 16 --warmup 2` of this commit and
                                                             # of its parent, run alternated in the same session

* ``OWLInterface.set_query_images`` for 1 and 8 example images at the default 768 x 768 B/32 in f32x3 (host clock around the
  call, which ends in a stream synchronise), and the text install of as many queries (``install_queries``) for scale;
* the selection kernel alone through ``tstar_image_query_select`` at np = 576 and 3600, n = 1 and 8 (host clock around the call:
  it allocates its staging buffer, launches, copies five small arrays back and synchronises -- the launcher's time, not the
  kernel's), against the bytes it has to read (the class embeddings once for the mean; the selected rows again);
* the deviations from HF's CPU ``image_guided_detection`` on HF-initialised checkpoints (the cases and bounds of
  tests/test_gpu_image_query.py::test_checkpoint_image_guided_matches_hf), when transformers is importable.
Nothing here is on the search loop's critical path: an example image costs one detector forward per question.  Synthetic or
HF-initialised weights throughout: detection QUALITY with real weights is not measured (no checkpoint is on disk)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_ms(torch, fn, warmup, reps):
    """Median and (min, max) of ``reps`` host-clock timings of ``fn``, which must end in a device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f})"


def registry_times(torch, lines, reps):
    import numpy as np
    from tstar_amd.interface_heuristic import OWLInterface
    h = OWLInterface(synthetic_seed=0, max_batch=32, weights_dtype="f32x3")
    rs = np.random.RandomState(0)
    lines += ["## Registering example images (B/32 at 768 x 768, f32x3, synthetic weights, 360 x 640 examples)", "",
              "| example images | `set_query_images` | `install_queries` of as many text queries (+ blank) |", "|---|---|---|"]
    for n in (1, 8):
        imgs = {f"object {i}": rs.randint(0, 256, (360, 640, 3)).astype(np.uint8) for i in range(n)}
        names = list(imgs)
        t_img = host_ms(torch, lambda: h.set_query_images(imgs), 2, reps)
        h.clear_query_images()
        t_txt = host_ms(torch, lambda: h.install_queries(1, names, []), 2, reps)
        lines.append(f"| {n} | {fmt(t_img)} | {fmt(t_txt)} |")
    lines.append("")
    del h


def kernel_times(torch, lines, reps):
    import numpy as np
    import image_query_util as U
    from tstar_amd import _lib
    lib = _lib.load()
    lines += ["## The selection launcher alone (`tstar_image_query_select`: staging allocation, one launch, five copies back, synchronise)", "",
              "| np | n | rows selected per image | time per call | class-embedding bytes read at least | that over 8 TB/s |", "|---|---|---|---|---|---|"]
    for np_ in (576, 3600):
        for n in (1, 8):
            # case 7 (identical boxes): every row selected, the most mean_sim work
            cls, boxes, exp = U.make_case(7, np_, np.random.RandomState(np_), np_ // 2)
            d_cls = torch.from_numpy(np.tile(cls, (n, 1))).cuda()
            d_box = torch.from_numpy(np.tile(boxes, (n, 1))).cuda()
            emb, box = np.zeros((n, 512), np.float32), np.zeros((n, 4), np.float32)
            best, nsel, status = (np.zeros(n, np.int32) for _ in range(3))

            def call():
                _lib.check(lib.tstar_image_query_select(d_cls.data_ptr(), d_box.data_ptr(), n, np_, emb.ctypes.data, best.ctypes.data,
                                                        box.ctypes.data, nsel.ctypes.data, status.ctypes.data, _lib.stream_ptr()))

            t = host_ms(torch, call, 3, reps)
            assert (best == exp["best"]).all() and (nsel == np_).all()
            nbytes = n * np_ * 512 * 4 * 2
            lines.append(f"| {np_} | {n} | {np_} | {fmt(t)} | {nbytes / 1e6:.2f} MB | {nbytes / 8e12 * 1e6:.2f} us |")
    lines += ["", "One workgroup per example image: a call with n = 1 runs on one of the 256 compute units, so its time is that unit's "
              "latency over np rows, not the memory system's rate.", ""]


def hf_deviations(torch, lines):
    try:
        import transformers  # noqa: F401
    except ImportError:
        lines += ["## Deviation from HF", "", "not measured: transformers is not importable here", ""]
        return
    import image_query_util as U
    from tstar_amd.interface_heuristic import OWLInterface
    lines += ["## Deviation from HF's CPU `image_guided_detection` (HF-initialised checkpoints, heads shrunk; two example and two target images)", "",
              "| geometry | input | weights | HF threshold margin | HF mean_sim gap | best index against HF | query box bits against `score` | max abs qn - HF | max abs sigmoid(logit) - HF | "
              "max abs box - HF (px) |", "|---|---|---|---|---|---|---|---|---|---|"]
    cache, models = {}, {}
    for g, mode in U.E2E_CASES:
        if g not in models:
            d = tempfile.mkdtemp(prefix=f"image_query_{g}_")
            models[g] = (d, U.make_checkpoint(g, d))
        d, model = models[g]
        ref = U.reference_for(g, model, "bf16" if mode == "bf16" else "f32", cache)
        margin, gap = U.assert_hf_margins(ref)
        size = U.GEOMETRIES[g][2]
        h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode, input_size=size)
        dev = U.device_image_guided(h, g, ref)
        same = all(int(dev["result"].best[b]) == p["best"] for b, p in enumerate(ref["per_image"]))
        lines.append(f"| {g} | {size[0]} x {size[1]} | {mode} | {margin:.2e} | {gap:.2e} | {'equal' if same else 'DIFFERS'} | "
                     f"{'equal' if dev['query_boxes_are_the_scorers_bits'] else 'DIFFER'} | {dev['emb_err']:.2e} | {dev['prob_err']:.2e} | "
                     f"{dev['box_err']:.2e} |")
        del h
    lines += ["", "Bounds of the test: 1e-5, 1e-3, 1e-2 px.", ""]


def bench_lines(lines, this_files, parent_files):
    def read(files):
        out = []
        for f in files:
            with open(f) as fh:
                for line in fh:
                    line = line.strip()
                    if line.startswith("{") and line.endswith("}"):
                        out.append(json.loads(line))
        return out
    this, parent = read(this_files), read(parent_files)
    if not this and not parent:
        return
    lines += ["## `bench.py --gpus 1 --steps 16 --warmup 2`, this commit and its parent alternated in one session", ""]
    for name, rows in (("this commit", this), ("parent", parent)):
        for r in rows:
            keys = [k for k in ("value", "unit", "ms_per_step") if k in r]
            lines.append(f"* {name}: " + (", ".join(f"{k} = {r[k]}" for k in keys) if keys else json.dumps(r)[:300]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_query_measure.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--this-bench", nargs="*", default=[])
    ap.add_argument("--parent-bench", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_image_query.py needs a HIP device: a CPU run measures nothing")
    lines = ["# Image-guided queries: measurements on one MI355X", "",
             f"`tools/measure_image_query.py --reps {args.reps}`: host clock around calls that end in a stream synchronise, after warm-up; median of "
             f"{args.reps} repeats with the smallest and largest.  Detection quality with real weights is NOT measured: no checkpoint is on disk.", ""]
    registry_times(torch, lines, args.reps)
    kernel_times(torch, lines, args.reps)
    hf_deviations(torch, lines)
    bench_lines(lines, args.this_bench, args.parent_bench)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
