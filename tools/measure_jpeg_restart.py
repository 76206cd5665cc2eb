"""Restart-coded Motion-JPEG against marker-free files on one MI355X -> profiles/jpeg_restart_measure.md / .json.

The question of DESIGN.md 8i: a frame without restart markers is one long segment, which the device entropy decoder cuts and
decodes in rounds; a frame with markers is many short segments of one lane each, one launch.  Does writing the files with
``save_mjpeg(restart_rows=1)`` or ``restart_blocks=8`` make a cold fetch from the compressed-resident store cheaper?

For the two stores of tools/bench_jpeg_ingest.py (3 600 x 360x640 and 600 x 1080x1920 of the synthetic video), at quality 75 and
90, three ways of writing the file -- no markers, ``restart_rows=1``, ``restart_blocks=8`` -- alternated, medians of --repeats:

* encode time of all frames (``FrameStore.jpeg_frames``, tools/bench_jpeg_encode.py's method: wall time around the call, and the
  two stages by HIP events in a second call), file bytes, and the arena bytes of the compressed-resident store;
* open time of the written .avi with host entropy, device entropy and ``resident="jpeg"``, and what the device mode cut;
* on the resident store a cold fetch of 16 / 64 / 256 frames and the reference-default 4 x 4 solo search, against the decoded
  store of the marker-free file (tools/measure_jpeg_resident.py's method and code).

``--encode-vs TREE`` first runs tools/bench_jpeg_encode.py of another built checkout (the parent commit) and of this one as child
processes, alternated, and reports the marker-free encode of both: that path launches the same kernels and must read inside the
spread of the other tree's runs.

    python tools/measure_jpeg_restart.py [--scale 0.1] [--encode-vs ../parent] [--only-fetch rows]    (--only-fetch: for a kernel trace)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_jpeg_ingest import CASES, timed  # noqa: E402
from measure_jpeg_resident import fetch_times, med_spread  # noqa: E402

VARIANTS = {"none": {}, "rows": dict(restart_rows=1), "blocks": dict(restart_blocks=8)}
LABEL = {"none": "no markers", "rows": "restart_rows=1", "blocks": "restart_blocks=8"}


def encode_vs(tree, rounds, scale):
    """tools/bench_jpeg_encode.py of `tree` and of this checkout, alternated child processes -> per case the runs of both."""
    out = {"other": {}, "this": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for which, root in (("other", tree), ("this", ROOT)) if r % 2 == 0 else (("this", ROOT), ("other", tree)):
                base = os.path.join(tmp, f"{which}{r}")
                subprocess.run([sys.executable, os.path.join(root, "tools", "bench_jpeg_encode.py"), "--out", base, "--scale", str(scale)],
                               check=True, cwd=root, stdout=subprocess.DEVNULL)
                print(f"encode-vs round {r}: {which} done", flush=True)
                with open(base + ".json") as f:
                    for row in json.load(f):
                        out[which].setdefault(row["case"], []).append({k: row[k] for k in ("device_wall_s", "block_ms", "entropy_ms", "same_bytes")})
    res = []
    for case in out["this"]:
        row = dict(case=case)
        for which in ("other", "this"):
            for k in ("device_wall_s", "block_ms", "entropy_ms"):
                row[f"{which}_{k}"] = med_spread([v[k] for v in out[which][case]])
        o, t = row["other_entropy_ms"], row["this_entropy_ms"]
        row["entropy_inside_other_spread"] = bool(o["min"] <= t["median"] <= o["max"])
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def encode_all(store, quality, repeats):
    """All frames of the store, the three ways alternated -> per variant wall / stage times, and the files of the last run."""
    from tstar_amd import jpeg_encode as JE
    secs = list(range(store.num_seconds))
    runs = {v: dict(wall=[], block_ms=[], entropy_ms=[], retried=[]) for v in VARIANTS}
    files = {}
    for r in range(repeats + 1):                                     # run 0 warms up
        order = list(VARIANTS) if r % 2 == 0 else list(VARIANTS)[::-1]
        for v in order:
            files[v], wall, _ = timed(lambda: store.jpeg_frames(secs, quality, **VARIANTS[v]))
            stats = {}
            timed(lambda: JE.encode_frames((store, secs), quality, stats=stats, **VARIANTS[v]))
            if r:
                runs[v]["wall"].append(wall)
                for k in ("block_ms", "entropy_ms", "retried"):
                    runs[v][k].append(stats[k])
            if v != "none":
                runs[v]["counters"] = {k: stats[k] for k in JE.RESTART_COUNTERS}
    return {v: dict(wall_s=med_spread(d["wall"]), block_ms=med_spread(d["block_ms"]), entropy_ms=med_spread(d["entropy_ms"]),
                    retried=d["retried"][-1], counters=d.get("counters")) for v, d in runs.items()}, files


def opens(paths, repeats):
    import torch
    from tstar_amd.video import open_video
    modes = {"host": dict(jpeg_entropy="host"), "device": dict(jpeg_entropy="device"), "resident": dict(resident="jpeg")}
    t = {(v, m): [] for v in paths for m in modes}
    stores, split = {}, {}
    for r in range(repeats + 1):
        for v in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
            for m, kw in modes.items():
                stores.pop((v, m), None)
                torch.cuda.empty_cache()
                st, wall, _ = timed(lambda: open_video(paths[v], **kw))
                if r:
                    t[(v, m)].append(wall)
                if m == "host":
                    del st
                else:
                    stores[(v, m)] = st
                    split[(v, m)] = dict(st.entropy_split_stats or {}, **{"entropy_" + k: n for k, n in (st.entropy_stats or {}).items()})
    return stores, {f"{v}/{m}": med_spread(x) for (v, m), x in t.items()}, {f"{v}/{m}": s for (v, m), s in split.items()}


def searches(stores, h, pairs):
    """The reference-default 4 x 4 solo search on every store, alternated; the same keyframes from each."""
    import torch
    from tstar_amd.interface_searcher import TStarSearcher
    t = {k: [] for k in stores}
    keys = {}
    for r in range(pairs + 1):
        for k in (list(stores) if r % 2 == 0 else list(stores)[::-1]):
            s = TStarSearcher(stores[k], h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(4, 4), search_budget=1000,
                              confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ts = s.search()
            torch.cuda.synchronize()
            if r:
                t[k].append(time.perf_counter() - t0)
            keys[k] = [float(x) for x in ts]
            last = dict(frames_scored=s.frames_scored, iterations=s.iterations)
    res = dict(times={k: med_spread(v) for k, v in t.items()}, keyframes=keys, **last)
    print(json.dumps(res), flush=True)
    return res


def write_md(res, path):
    L = ["# Restart-coded Motion-JPEG against marker-free files on one MI355X", "",
         f"Device: {res['device']}.  Written by `tools/measure_jpeg_restart.py`; the JSON next to this file holds every run.  Medians of "
         f"{res['repeats']} alternated runs (searches: {res['pairs']}).  The files are `FrameStore.save_mjpeg`'s frames of the synthetic video, "
         "4:2:0; decoded = `open_video(path, jpeg_entropy=\"device\")` of the marker-free file, resident = `open_video(path, resident=\"jpeg\")` "
         "with the default pool.", ""]
    if res.get("encode_vs"):
        L += ["## Marker-free encode: this commit against the other checkout (`tools/bench_jpeg_encode.py`, alternated child processes)", "",
              "| case | other wall s | this wall s | other entropy stage ms [min .. max] | this entropy stage ms [min .. max] | this median inside the other's spread |",
              "|---|---|---|---|---|---|"]
        for r in res["encode_vs"]:
            o, t = r["other_entropy_ms"], r["this_entropy_ms"]
            L.append(f"| {r['case']} | {r['other_device_wall_s']['median']:.3f} | {r['this_device_wall_s']['median']:.3f} | "
                     f"{o['median']:.2f} [{o['min']:.2f} .. {o['max']:.2f}] | {t['median']:.2f} [{t['min']:.2f} .. {t['max']:.2f}] | {r['entropy_inside_other_spread']} |")
        L.append("")
    L += ["## Bytes and encode time (all frames, `FrameStore.jpeg_frames`)", "",
          "| store | quality | file | file MB | against no markers | arena MB | markers per frame | encode wall s | block stage ms | entropy stage ms | retried |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for v in VARIANTS:
            e = c["encode"][v]
            mk = e["counters"]["rst"] / c["frames"] if e["counters"] else 0
            L.append(f"| {c['name']} | {c['quality']} | {LABEL[v]} | {c['file_bytes'][v] / 1e6:.1f} | {c['file_bytes'][v] / c['file_bytes']['none']:.4f} | "
                     f"{c['arena_bytes'][v] / 1e6:.1f} | {mk:.0f} | {e['wall_s']['median']:.3f} | {e['block_ms']['median']:.2f} | {e['entropy_ms']['median']:.2f} | {e['retried']} |")
    L += ["", "## Open time (s) and what the device mode cut", "", "| store | quality | file | host | device | resident | segments cut (device) | rounds |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for v in VARIANTS:
            o, s = c["open"], c["split"][f"{v}/device"]
            L.append(f"| {c['name']} | {c['quality']} | {LABEL[v]} | {o[f'{v}/host']['median']:.3f} | {o[f'{v}/device']['median']:.3f} | "
                     f"{o[f'{v}/resident']['median']:.3f} | {s.get('split')} | {s.get('rounds_max')} |")
    L += ["", "## Cold fetch from the resident store (`lease` of n seconds, none resident; HIP events, medians, ms)", "",
          "| store | quality | n | no markers | restart_rows=1 | restart_blocks=8 | rows / none | blocks / none |", "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for i, f in enumerate(c["fetch"]["none"]):
            ms = {v: c["fetch"][v][i]["cold_s"]["median"] * 1e3 for v in VARIANTS}
            L.append(f"| {c['name']} | {c['quality']} | {f['frames']} | {ms['none']:.2f} | {ms['rows']:.2f} | {ms['blocks']:.2f} | "
                     f"{ms['rows'] / ms['none']:.2f} | {ms['blocks'] / ms['none']:.2f} |")
    L += ["", "## Reference-default 4 x 4 solo search (f32x3 synthetic OWL heuristic, K = 8, seed 2025; median [min .. max] s)", "",
          "| store | quality | decoded store | resident, no markers | resident, restart_rows=1 | resident, restart_blocks=8 | over decoded: none / rows / blocks | same keyframes |",
          "|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        if not c.get("search"):
            continue
        t = c["search"]["times"]
        cell = lambda k: f"{t[k]['median']:.3f} [{t[k]['min']:.3f} .. {t[k]['max']:.3f}]"          # noqa: E731
        d = t["decoded"]["median"]
        same = len({tuple(k) for k in c["search"]["keyframes"].values()}) == 1
        L.append(f"| {c['name']} | {c['quality']} | {cell('decoded')} | {cell('none')} | {cell('rows')} | {cell('blocks')} | "
                 f"{t['none']['median'] / d:.3f} / {t['rows']['median'] / d:.3f} / {t['blocks']['median'] / d:.3f} | {same} |")
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_restart_measure"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsal)")
    ap.add_argument("--qualities", default="75,90")
    ap.add_argument("--encode-vs", default=None, help="another built checkout whose marker-free encode is compared with this one's")
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--only-fetch", choices=tuple(VARIANTS), default=None,
                    help="40 cold fetches of 16 frames from the first store written that way, quality 75, and nothing else (for a kernel trace)")
    args = ap.parse_args()
    res = dict(repeats=args.repeats, pairs=args.pairs, cases=[])
    if args.encode_vs:                                 # child processes first, before this one opens the device
        res["encode_vs"] = encode_vs(os.path.abspath(args.encode_vs), max(2, args.repeats), args.scale)
    import torch
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import open_video, synthetic_video
    torch.cuda.set_device(0)
    res["device"] = torch.cuda.get_device_name(0)
    h = None
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(32, int(n * args.scale))
            store = synthetic_video(n, H, W, seed=21)
            for q in (int(v) for v in args.qualities.split(",")):
                if args.only_fetch:
                    path = os.path.join(tmp, "trace.avi")
                    store.save_mjpeg(path, quality=q, **VARIANTS[args.only_fetch])
                    st = open_video(path, resident="jpeg")
                    for r in range(40):
                        st.flush()
                        st.lease(list(range((16 * r) % (n - 15), (16 * r) % (n - 15) + 16))).done()
                    torch.cuda.synchronize()
                    return
                enc, files = encode_all(store, q, args.repeats)
                paths = {}
                for v in VARIANTS:
                    paths[v] = os.path.join(tmp, f"{name}-{q}-{v}.avi")
                    JE.write_mjpeg_file(paths[v], files[v], W, H)
                case = dict(name=name, frames=n, quality=q, encode=enc, file_bytes={v: sum(len(f) for f in files[v]) for v in VARIANTS})
                del files
                stores, case["open"], case["split"] = opens(paths, args.repeats)
                case["arena_bytes"] = {v: stores[(v, "resident")].pool_stats()["arena_bytes"] for v in VARIANTS}
                want = stores[("none", "device")].frames
                for v in VARIANTS:                    # the markers change the entropy coding, not a pixel
                    assert torch.equal(stores[(v, "device")].frames, want), v
                print(json.dumps(case), flush=True)
                case["fetch"] = {v: fetch_times(stores[(v, "resident")], reps=max(3, args.repeats)) for v in VARIANTS}
                if not args.no_search:
                    if h is None:
                        from tstar_amd.interface_heuristic import OWLInterface
                        h = OWLInterface(synthetic_seed=0, max_batch=256, weights_dtype="f32x3")
                    case["search"] = searches(dict(decoded=stores[("none", "device")], **{v: stores[(v, "resident")] for v in VARIANTS}), h, args.pairs)
                res["cases"].append(case)
                del stores, want
                torch.cuda.empty_cache()
            del store
            torch.cuda.empty_cache()
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    write_md(res, args.out + ".md")
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
