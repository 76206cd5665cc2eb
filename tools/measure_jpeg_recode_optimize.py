"""The re-coded arena with optimised Huffman tables against the standard-table one on one MI355X
-> profiles/jpeg_recode_optimize_measure.md / .json.

The question of DESIGN.md 8m: ``open_video(path, resident="jpeg", recode_blocks=8, recode_optimize=True)`` codes every group of
frames with ONE set of tables built from the group's own symbol counts.  What does the arena save, what does the open pay, and does
a fetch read the optimised arena as fast as the standard-table one?

Four files: the two standard marker-free files of DESIGN.md 8k (3 600 x 360x640 and 600 x 1080x1920 of the synthetic video, Pillow
quality 85, 4:2:0) and the same pictures written by Pillow with ``optimize=True``.  For each, against the SAME run's
``recode_blocks=8`` without ``recode_optimize``, alternated, medians of --repeats:

* arena bytes and ``recode_stats``; open wall seconds and host CPU-seconds
* the scan stage of the first chunk from HIP events: standard tables, shared tables (all stages), and the new steps alone
  (counts + group sums; group tables)
* cold fetches of 16 / 64 / 256 frames
* the 4 x 4 solo and the 16 x 16 throughput search (tools/measure_jpeg_recode.py's), which must return the same keyframes
* ``recode_mjpeg(optimize=True)`` against ``optimize=False``: seconds and bytes

Every frame of the optimised store is checked against the decoded store's.

    python tools/measure_jpeg_recode_optimize.py [--scale 0.1] [--no-search] [--no-throughput-search] [--bench-log LOG]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_jpeg_ingest import CASES, timed, write_avi  # noqa: E402
from measure_jpeg_recode import bench_lines, searches  # noqa: E402
from measure_jpeg_resident import fetch_times, med_spread  # noqa: E402

INTERVAL = 8
STORES = ("decoded", "recoded", "optimized")
RESIDENT = STORES[1:]


def make_avi(path, n, H, W, optimize, threads=16):
    from PIL import Image
    from tstar_amd.video import synthetic_video
    frames = synthetic_video(n, H, W, seed=21).frames.cpu().numpy()

    def enc(i):
        b = io.BytesIO()
        Image.fromarray(frames[i]).save(b, "JPEG", quality=85, subsampling=2, optimize=optimize)
        return b.getvalue()

    with ThreadPoolExecutor(threads) as ex:
        jpegs = list(ex.map(enc, range(n)))
    write_avi(path, jpegs, W, H, 1)
    return sum(len(j) for j in jpegs)


def open_store(kind, path):
    from tstar_amd.video import open_video
    if kind == "decoded":
        return open_video(path, jpeg_entropy="device")
    return open_video(path, resident="jpeg", recode_blocks=INTERVAL, recode_optimize=kind == "optimized")


def opens(path, repeats):
    import torch
    wall, cpu = {k: [] for k in STORES}, {k: [] for k in STORES}
    stores = {}
    for r in range(repeats + 1):                                     # run 0 warms up (library load, pinned pools)
        for kind in (STORES if r % 2 == 0 else STORES[::-1]):
            stores.pop(kind, None)
            torch.cuda.empty_cache()
            st, w, c = timed(lambda: open_store(kind, path))
            stores[kind] = st
            if r:
                wall[kind].append(w)
                cpu[kind].append(c)
    return stores, {k: dict(wall_s=med_spread(wall[k]), cpu_s=med_spread(cpu[k])) for k in STORES}


def scan_times(path, reps=5):
    """The scan stage of the file's first chunk (at most 256 frames), HIP events, ms: the standard tables; the shared tables, all
    stages; and the new steps alone through the stages of tstar_jpeg_encode_scan_grp."""
    import torch
    from tstar_amd import _lib, jpeg, jpeg_recode as JR
    src = jpeg.open_source(path)
    try:
        files = [src.read(i) for i in range(min(256, src.n_frames))]
    finally:
        src.close()
    geom = JR.covered(files[0])
    run = JR.runner_for(files, geom, "cuda")
    part = run.read(0)
    ticket = run.submit(0, part, torch.cuda.current_stream())
    assert run.collect(ticket) == []
    n = len(part)
    slot = (2 * max(map(len, part)) + 4096 + 15) // 16 * 16
    out = {"frames": n}

    def ms(fn):
        t = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                t.append(e0.elapsed_time(e1))
        return med_spread(t)

    std = JR.DeviceRecoder(geom, "cuda", INTERVAL)
    bufs = std._buffers(n, slot)
    out["standard"] = ms(lambda: std._scan(run.d_coef, 0, n, slot, bufs, True))
    rec = JR.DeviceRecoder(geom, "cuda", INTERVAL, optimize=True, shared=True)
    group, k = JR.make_groups(np.ones(n, dtype=bool), rec.group_frames)
    rec.groups = SimpleNamespace(group=group, n=k, d_hist=torch.empty((k, 4 * 257), dtype=torch.int32, device="cuda"),
                                 d_specs=torch.empty((k, 4 * 276), dtype=torch.uint8, device="cuda"))
    bufs = rec._buffers(n, slot)
    out["shared"] = ms(lambda: rec._scan(run.d_coef, 0, n, slot, bufs, True))
    lib, W, H, hs, vs = _lib.load(), *geom[:2], *geom[3:]
    span = np.zeros((k, 2), dtype=np.int32)
    _lib.check(lib.tstar_jpeg_encode_group_spans(group.ctypes.data, n, k, W, H, hs, vs, span.ctypes.data), "tstar_jpeg_encode_group_spans")
    d_gs = torch.from_numpy(np.concatenate([group, span.reshape(-1)])).cuda()
    work = bufs.work

    def stage(stages):
        _lib.check(lib.tstar_jpeg_encode_scan_grp(run.d_coef.data_ptr(), n, W, H, hs, vs, INTERVAL, group.ctypes.data, span.ctypes.data, d_gs.data_ptr(),
                                                  d_gs.data_ptr() + 4 * n, k, stages, rec.groups.d_hist.data_ptr(), rec.groups.d_specs.data_ptr(), None, slot, None,
                                                  None, work.data_ptr(), work.numel(), _lib.stream_ptr()), "tstar_jpeg_encode_scan_grp")

    out["counts_and_group_sums"] = ms(lambda: stage(1))
    out["group_tables"] = ms(lambda: stage(2))
    out["groups"] = k
    return out


def recode_files(path, tmp, repeats):
    """recode_mjpeg to a .mjpeg stream with and without optimize: seconds (alternated, medians) and bytes."""
    from tstar_amd import jpeg_encode as JE
    t, size, stats = {False: [], True: []}, {}, {}
    for r in range(repeats + 1):
        for opt in ((False, True) if r % 2 == 0 else (True, False)):
            dst = os.path.join(tmp, f"recode-{int(opt)}.mjpeg")
            st = {}
            t0 = time.perf_counter()
            JE.recode_mjpeg(path, dst, restart_blocks=INTERVAL, stats=st, optimize=opt)
            if r:
                t[opt].append(time.perf_counter() - t0)
            size[opt], stats[opt] = os.path.getsize(dst), st
            os.remove(dst)
    return dict(standard=dict(seconds=med_spread(t[False]), bytes=size[False], stats=stats[False]),
                optimized=dict(seconds=med_spread(t[True]), bytes=size[True], stats=stats[True]))


def write_md(res, path):
    L = ["# The re-coded arena with optimised Huffman tables against the standard-table one on one MI355X", "",
         f"Device: {res['device']}.  Written by `tools/measure_jpeg_recode_optimize.py`; the JSON next to this file holds every run.  Medians of "
         f"{res['repeats']} alternated runs (searches: {res['pairs']} alternated rounds).  Files: the synthetic video, Pillow quality 85, 4:2:0, "
         "no restart markers, written with the standard tables and (`-opt`) with Pillow's `optimize=True`.  decoded = "
         f"`open_video(path, jpeg_entropy=\"device\")`; recoded = `open_video(path, resident=\"jpeg\", recode_blocks={INTERVAL})`; optimized = the "
         "same with `recode_optimize=True`.", ""]
    L += ["## Open: wall time, host CPU-seconds, arena bytes", "",
          "| file | store | open wall s [min .. max] | host CPU s | arena MB | arena / file | arena / recoded | recoded / kept | groups x quant sets |",
          "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for k in STORES:
            o = c["open"][k]
            a = c["arena_bytes"].get(k)
            head = f"| {c['name']} | {k} | {o['wall_s']['median']:.3f} [{o['wall_s']['min']:.3f} .. {o['wall_s']['max']:.3f}] | {o['cpu_s']['median']:.3f} | "
            if a is None:
                L.append(head + "- | - | - | - | - |")
                continue
            rs = c["recode_stats"][k]
            L.append(head + f"{a / 1e6:.1f} | {a / c['frame_bytes']:.4f} | {a / c['arena_bytes']['recoded']:.4f} | {rs['recoded']} / {rs['kept']} | "
                     f"{rs.get('table_sets', '-')} |")
    L += ["", "## The scan stage of the first chunk (HIP events, medians, ms)", "",
          "| file | frames | groups | standard tables | shared tables, all stages | counts + group sums alone | group tables alone |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        s = c["scan_ms"]
        L.append(f"| {c['name']} | {s['frames']} | {s['groups']} | {s['standard']['median']:.3f} | {s['shared']['median']:.3f} | "
                 f"{s['counts_and_group_sums']['median']:.3f} | {s['group_tables']['median']:.3f} |")
    L += ["", "## Cold fetch (`lease` of n seconds, none resident; HIP events, medians, ms)", "",
          "| file | n | recoded | optimized | optimized / recoded |", "|---|---|---|---|---|"]
    for c in res["cases"]:
        for i, f in enumerate(c["fetch"]["recoded"]):
            ms = {k: c["fetch"][k][i]["cold_s"]["median"] * 1e3 for k in RESIDENT}
            L.append(f"| {c['name']} | {f['frames']} | {ms['recoded']:.2f} | {ms['optimized']:.2f} | {ms['optimized'] / ms['recoded']:.2f} |")
    if any(c.get("searches") for c in res["cases"]):
        L += ["", "## Searches (f32x3 synthetic OWL heuristic, K = 8, seed 2025; median [min .. max] s)", "",
              "| file | search | decoded | recoded | optimized | optimized / recoded | same keyframes |", "|---|---|---|---|---|---|---|"]
        for c in res["cases"]:
            for s in c.get("searches", []):
                t = s["times"]
                cell = lambda k: f"{t[k]['median']:.3f} [{t[k]['min']:.3f} .. {t[k]['max']:.3f}]"          # noqa: E731
                L.append(f"| {c['name']} | {s['search']} | {cell('decoded')} | {cell('recoded')} | {cell('optimized')} | "
                         f"{t['optimized']['median'] / t['recoded']['median']:.3f} | {s['same_keyframes']} |")
    L += ["", f"## `recode_mjpeg(restart_blocks={INTERVAL})` to a .mjpeg stream: per-frame tables against the standard tables", "",
          "| file | bytes in | standard: s, bytes, out / in | optimize=True: s, bytes, out / in | kept |", "|---|---|---|---|---|"]
    for c in res["cases"]:
        f = c["recode_mjpeg"]
        a, b = f["standard"], f["optimized"]
        L.append(f"| {c['name']} | {c['frame_bytes']} | {a['seconds']['median']:.2f}, {a['bytes']}, {a['bytes'] / c['frame_bytes']:.4f} | "
                 f"{b['seconds']['median']:.2f}, {b['bytes']}, {b['bytes'] / c['frame_bytes']:.4f} | {b['stats'].get('kept', 0)} |")
    if res.get("bench"):
        b = res["bench"]
        med = {k: float(np.median([r["frames_per_s"] for r in b[k]])) for k in b}
        L += ["", "## `bench.py --gpus 1 --steps 16 --warmup 1`: the parent commit and this commit, alternated in one session", "",
              "`bench.py` does not touch the re-coding path; the line has to stay inside the +- 3 % board spread README states.", "",
              "| tree | frames/s, run by run | median | ms per step, run by run |", "|---|---|---|---|"]
        for k in ("parent", "this"):
            fps = " / ".join("%.0f" % r["frames_per_s"] for r in b[k])
            ms = " / ".join("%.2f" % r["ms_per_step"] for r in b[k])
            L.append(f"| {k} | {fps} | {med[k]:.0f} | {ms} |")
        L += ["", f"This commit's median differs from the parent's by {100 * (med['this'] / med['parent'] - 1):+.2f} %."]
    L += [""] + res.get("notes", [])
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_recode_optimize_measure"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsal)")
    ap.add_argument("--bench-log", default=None, help="a log of alternated bench.py runs of the parent and of this commit (bench_lines)")
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--no-throughput-search", action="store_true", help="leave the 16 x 16 search out")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, pairs=args.pairs, interval=INTERVAL, cases=[])
    if args.bench_log:
        res["bench"] = bench_lines(args.bench_log)
    h = None
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(32, int(n * args.scale))
            for optimize in (False, True):
                label = name + ("-opt" if optimize else "")
                path = os.path.join(tmp, f"{label}.avi")
                frame_bytes = make_avi(path, n, H, W, optimize)
                stores, op = opens(path, args.repeats)
                case = dict(name=label, frames=n, frame_bytes=frame_bytes, open=op,
                            arena_bytes={k: stores[k].pool_stats()["arena_bytes"] for k in RESIDENT},
                            recode_stats={k: stores[k].recode_stats for k in RESIDENT},
                            split={k: stores[k].entropy_split_stats for k in STORES})
                assert case["arena_bytes"]["optimized"] < case["arena_bytes"]["recoded"], f"{label}: the optimised arena is not smaller"
                want = stores["decoded"].frames
                for s0 in range(0, n, 256):                              # not one pixel changes
                    secs = list(range(s0, min(n, s0 + 256)))
                    assert np.array_equal(stores["optimized"].host_frames(secs), want[s0:s0 + len(secs)].cpu().numpy()), f"{label}: frames {s0}.."
                case["same_pixels"] = True
                case["scan_ms"] = scan_times(path)
                case["fetch"] = {k: fetch_times(stores[k], reps=max(3, args.repeats)) for k in RESIDENT}
                case["recode_mjpeg"] = recode_files(path, tmp, args.repeats)
                print(json.dumps(case), flush=True)
                if not args.no_search:
                    if h is None:
                        from tstar_amd.interface_heuristic import OWLInterface
                        h = OWLInterface(synthetic_seed=0, max_batch=256, weights_dtype="f32x3")
                    case["searches"] = [searches(stores, h, 4, 1000, args.pairs, "reference default: 4 x 4 grid, solo")]
                    if not args.no_throughput_search:
                        case["searches"].append(searches(stores, h, 16, 1000, args.pairs, "configs[1]: 16 x 16 grid, budget 1000"))
                res["cases"].append(case)
                with open(args.out + ".json", "w") as f:                 # after every file: a run cut short keeps what it measured
                    json.dump(res, f, indent=1)
                write_md(res, args.out + ".md")
                del stores, want
                torch.cuda.empty_cache()
                os.remove(path)
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
