"""The re-coded arena against the plain compressed-resident store on one MI355X -> profiles/jpeg_recode_measure.md / .json.

The question of DESIGN.md 8k: ``open_video(path, resident="jpeg", recode_blocks=8)`` re-codes a marker-free file's arena losslessly
with a restart interval at open.  Does the store then read like the store of a file that was WRITTEN with ``restart_blocks=8``
(profiles/jpeg_restart_measure.md), and what does the open pay for it?

For the two standard files without restart markers (3 600 x 360x640 and 600 x 1080x1920 of the synthetic video, Pillow quality 85,
4:2:0; tools/bench_jpeg_ingest.py's ``make_avi``), four stores, alternated, medians of --repeats:

* ``decoded``   open_video(path, jpeg_entropy="device")
* ``plain``     open_video(path, resident="jpeg")                      -- what the parent commit serves
* ``recoded``   open_video(path, resident="jpeg", recode_blocks=8)
* ``written8``  open_video(path8, resident="jpeg"), path8 = the same pictures written by Pillow with restart_marker_blocks=8

open wall time and host CPU-seconds, arena bytes, what the open cut; a cold fetch of 16 / 64 / 256 frames from the three resident
stores; the reference-default 4 x 4 solo search and the 16 x 16 throughput search on all four (tools/measure_jpeg_resident.py's
method and code).  The re-coded store's frames are checked against the decoded store's, all of them.

    python tools/measure_jpeg_recode.py [--scale 0.1] [--no-search] [--bench-log LOG]

``--bench-log``: the ``bench.py`` lines of the parent commit and of this one, which the caller ran alternately (``bench_lines``), go
into the profile too.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_jpeg_ingest import CASES, make_avi, timed  # noqa: E402
from measure_jpeg_resident import fetch_times, med_spread  # noqa: E402

INTERVAL = 8
STORES = ("decoded", "plain", "recoded", "written8")
RESIDENT = STORES[1:]


def open_store(kind, path, path8):
    from tstar_amd.video import open_video
    if kind == "decoded":
        return open_video(path, jpeg_entropy="device")
    if kind == "plain":
        return open_video(path, resident="jpeg")
    if kind == "recoded":
        return open_video(path, resident="jpeg", recode_blocks=INTERVAL)
    return open_video(path8, resident="jpeg")


def opens(path, path8, repeats):
    import torch
    wall, cpu = {k: [] for k in STORES}, {k: [] for k in STORES}
    stores = {}
    for r in range(repeats + 1):                                     # run 0 warms up (library load, pinned pools)
        for kind in (STORES if r % 2 == 0 else STORES[::-1]):
            stores.pop(kind, None)
            torch.cuda.empty_cache()
            st, w, c = timed(lambda: open_store(kind, path, path8))
            stores[kind] = st
            if r:
                wall[kind].append(w)
                cpu[kind].append(c)
    return stores, {k: dict(wall_s=med_spread(wall[k]), cpu_s=med_spread(cpu[k])) for k in STORES}


def searches(stores, h, grid, budget, pairs, label):
    import torch
    from tstar_amd.interface_searcher import TStarSearcher
    t = {k: [] for k in stores}
    keys = {}
    for r in range(pairs + 1):                                       # pair 0 warms up
        for k in (list(stores) if r % 2 == 0 else list(stores)[::-1]):
            s = TStarSearcher(stores[k], h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(grid, grid), search_budget=budget,
                              confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ts = s.search()
            torch.cuda.synchronize()
            if r:
                t[k].append(time.perf_counter() - t0)
            keys[k] = [float(x) for x in ts]
            last = dict(frames_scored=s.frames_scored, iterations=s.iterations)
    res = dict(search=label, grid=grid, budget=budget, **last, times={k: med_spread(v) for k, v in t.items()},
               same_keyframes=len({tuple(v) for v in keys.values()}) == 1)
    print(json.dumps(res), flush=True)
    return res


def optimised_growth(frames=32):
    """Bytes of files Pillow wrote with OPTIMISED Huffman tables (quality 85, 4:2:0, no markers) before and after the re-coding, which
    always writes the standard tables: the host twin on ``frames`` frames of each size (byte counts; no GPU involved)."""
    import io
    from PIL import Image
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import synthetic_frames_numpy
    out = []
    for name, n, H, W in CASES:
        pics = synthetic_frames_numpy(list(range(0, n, max(1, n // frames)))[:frames], n, H, W, seed=21)
        files = []
        for pic in pics:
            b = io.BytesIO()
            Image.fromarray(pic).save(b, "JPEG", quality=85, subsampling=2, optimize=True)
            files.append(b.getvalue())
        stats = {}
        JE.recode_frames(files, restart_blocks=INTERVAL, device=False, stats=stats)
        out.append(dict(name=name, frames=len(files), **stats))
    return out


def bench_lines(log):
    """``bench.py --gpus 1 --steps 16 --warmup 1`` of the parent commit and of this one, run alternately in one session by the caller
    (``bench.py`` does not touch the re-coding path): a log of ``== parent run 1`` / ``== this run 1`` headings, each followed by that
    run's JSON result line -> {"parent": [...], "this": [...]} of (frames/s, ms per step)."""
    out, who = {"parent": [], "this": []}, None
    with open(log) as f:
        for line in f:
            if line.startswith("=="):
                who = line.split()[1]
            elif line.startswith("{") and who in out:
                j = json.loads(line)
                out[who].append(dict(frames_per_s=j["value"], ms_per_step=j["ms_per_step"]))
    return out


def write_md(res, path):
    L = ["# The re-coded arena against the plain compressed-resident store on one MI355X", "",
         f"Device: {res['device']}.  Written by `tools/measure_jpeg_recode.py`; the JSON next to this file holds every run.  Medians of "
         f"{res['repeats']} alternated runs (searches: {res['pairs']} alternated rounds).  Files: the synthetic video, Pillow quality 85, 4:2:0, "
         "no restart markers.  decoded = `open_video(path, jpeg_entropy=\"device\")`; plain = `open_video(path, resident=\"jpeg\")`; recoded = "
         f"`open_video(path, resident=\"jpeg\", recode_blocks={INTERVAL})`; written8 = the plain resident open of the same pictures written by "
         f"Pillow with `restart_marker_blocks={INTERVAL}` (the layout the re-coding aims at).", ""]
    L += ["## Open: wall time, host CPU-seconds, arena bytes, what the store's fetches cut", "",
          "| file | store | open wall s [min .. max] | host CPU s | arena MB | arena / plain | recoded / kept | segments a fetch cuts | rounds |",
          "|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for k in STORES:
            o = c["open"][k]
            a = c["arena_bytes"].get(k)
            rs = c["recode_stats"] if k == "recoded" else None
            sp = c["split"].get(k, {})
            L.append(f"| {c['name']} | {k} | {o['wall_s']['median']:.3f} [{o['wall_s']['min']:.3f} .. {o['wall_s']['max']:.3f}] | "
                     f"{o['cpu_s']['median']:.3f} | {a / 1e6:.1f} | {a / c['arena_bytes']['plain']:.4f} | "
                     f"{(str(rs['recoded']) + ' / ' + str(rs['kept'])) if rs else '-'} | {sp.get('split', '-')} | {sp.get('rounds_max', '-')} |"
                     if a is not None else
                     f"| {c['name']} | {k} | {o['wall_s']['median']:.3f} [{o['wall_s']['min']:.3f} .. {o['wall_s']['max']:.3f}] | "
                     f"{o['cpu_s']['median']:.3f} | - | - | - | - | - |")
    L += ["", "## Cold fetch (`lease` of n seconds, none resident; HIP events, medians, ms)", "",
          "| file | n | plain | recoded | written8 | recoded / plain | recoded / written8 |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for i, f in enumerate(c["fetch"]["plain"]):
            ms = {k: c["fetch"][k][i]["cold_s"]["median"] * 1e3 for k in RESIDENT}
            L.append(f"| {c['name']} | {f['frames']} | {ms['plain']:.2f} | {ms['recoded']:.2f} | {ms['written8']:.2f} | "
                     f"{ms['recoded'] / ms['plain']:.2f} | {ms['recoded'] / ms['written8']:.2f} |")
    L += ["", "## Searches (f32x3 synthetic OWL heuristic, K = 8, seed 2025; median [min .. max] s)", "",
          "| file | search | decoded | plain | recoded | written8 | over decoded: plain / recoded / written8 | same keyframes |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for s in c.get("searches", []):
            t = s["times"]
            cell = lambda k: f"{t[k]['median']:.3f} [{t[k]['min']:.3f} .. {t[k]['max']:.3f}]"          # noqa: E731
            d = t["decoded"]["median"]
            L.append(f"| {c['name']} | {s['search']} | {cell('decoded')} | {cell('plain')} | {cell('recoded')} | {cell('written8')} | "
                     f"{t['plain']['median'] / d:.3f} / {t['recoded']['median'] / d:.3f} / {t['written8']['median'] / d:.3f} | {s['same_keyframes']} |")
    if res.get("optimised_growth"):
        L += ["", f"## A source with optimised Huffman tables grows (host twin, `recode_frames(restart_blocks={INTERVAL})`; byte counts)", "",
              "| file | frames | re-coded / kept | bytes in | bytes out | out / in |", "|---|---|---|---|---|---|"]
        for g in res["optimised_growth"]:
            L.append(f"| {g['name']} | {g['frames']} | {g.get('recoded', 0)} / {g.get('kept', 0)} | {g['bytes_in']} | {g['bytes_out']} | "
                     f"{g['bytes_out'] / g['bytes_in']:.4f} |")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_recode_measure"))
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
    res["optimised_growth"] = optimised_growth()
    print(json.dumps(res["optimised_growth"]), flush=True)
    h = None
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(32, int(n * args.scale))
            path, path8 = os.path.join(tmp, f"{name}.avi"), os.path.join(tmp, f"{name}-rst{INTERVAL}.avi")
            make_avi(path, n, H, W)
            make_avi(path8, n, H, W, restart_blocks=INTERVAL)
            stores, op = opens(path, path8, args.repeats)
            rec = stores["recoded"]
            case = dict(name=name, frames=n, file_bytes=os.path.getsize(path), file8_bytes=os.path.getsize(path8), open=op,
                        arena_bytes={k: stores[k].pool_stats()["arena_bytes"] for k in RESIDENT}, recode_stats=rec.recode_stats,
                        split={k: stores[k].entropy_split_stats for k in STORES})
            want = stores["decoded"].frames
            for s0 in range(0, n, 256):                              # not one pixel changes
                secs = list(range(s0, min(n, s0 + 256)))
                assert np.array_equal(rec.host_frames(secs), want[s0:s0 + len(secs)].cpu().numpy()), f"{name}: frames {s0}.."
            case["same_pixels"] = True
            print(json.dumps(case), flush=True)
            case["fetch"] = {k: fetch_times(stores[k], reps=max(3, args.repeats)) for k in RESIDENT}
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
            del stores, rec, want
            torch.cuda.empty_cache()
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
