"""The compressed-resident JPEG store against the decoded store on one MI355X -> profiles/jpeg_resident_measure.md / .json.

The two files of tools/bench_jpeg_ingest.py (3 600 x 360x640 and 600 x 1080x1920 Motion-JPEG AVI, quality 85, 4:2:0, no restart
markers), each opened as a decoded store (``open_video(path, jpeg_entropy="device")``: the parent's unchanged path) and as a
compressed-resident one (``resident="jpeg"``, the default pool of 512 slots):

* HBM bytes: the decoded store against arena + pool (and the fetch workspace, which the pool figure does not include);
* open time, medians of --repeats alternating runs;
* fetch time of 16, 64 and 256 frames, cold (no frame resident) and with every frame resident: HIP events around ``lease`` and
  the host's wall time inside the call;
* a reference-default 4 x 4 solo search and a 16 x 16 throughput search (budget 1000) on each store with a synthetic f32x3 OWL
  heuristic: --pairs alternated pairs, medians and spread, and that both stores gave the same keyframes.

    python tools/measure_jpeg_resident.py [--scale 0.1] [--only-search resident]      (--only-search: for a rocprofv3 --kernel-trace --stats run)
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


def med_spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), runs=[float(x) for x in v])


def open_both(path, repeats):
    import torch
    from tstar_amd.video import open_video
    opens = {"decoded": [], "resident": []}
    stores = {}
    for r in range(repeats + 1):                                     # run 0 warms up (library load, pinned pools)
        for kind in ("decoded", "resident"):
            stores.pop(kind, None)
            torch.cuda.empty_cache()
            st, wall, _ = timed((lambda: open_video(path, jpeg_entropy="device")) if kind == "decoded" else (lambda: open_video(path, resident="jpeg")))
            stores[kind] = st
            if r:
                opens[kind].append(wall)
    return stores, {k: med_spread(v) for k, v in opens.items()}


def workspace_bytes(st):
    return sum(int(t.numel() * t.element_size()) for t in (st._d_batch, st._d_coef, st._d_planes, st._d_status, st._d_ws))


def fetch_times(st, reps=5):
    """lease(secs) of n frames: cold = none of them resident (the pool flushed first), warm = the same request again."""
    import torch
    out = []
    N = st.num_seconds
    for n in (16, 64, 256):
        if n > N or n > st.pool_frames:
            continue
        cold, warm, cold_host, warm_host = [], [], [], []
        for r in range(reps + 1):
            base = (r * n) % (N - n + 1)
            secs = list(range(base, base + n))
            st.flush()
            for which, ev_l, host_l in (("cold", cold, cold_host), ("warm", warm, warm_host)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                before = st.pool_stats()["misses"]
                e0.record()
                t0 = time.perf_counter()
                lease = st.lease(secs)
                host = time.perf_counter() - t0
                e1.record()
                lease.done()
                torch.cuda.synchronize()
                missed = st.pool_stats()["misses"] - before
                assert missed == (n if which == "cold" else 0), (which, missed)
                if r:
                    ev_l.append(e0.elapsed_time(e1) * 1e-3)
                    host_l.append(host)
        out.append(dict(frames=n, cold_s=med_spread(cold), warm_s=med_spread(warm), cold_host_s=med_spread(cold_host),
                        warm_host_s=med_spread(warm_host)))
        print(json.dumps(out[-1]), flush=True)
    assert st.fetch_errors() == 0
    return out


def searches(stores, h, grid, budget, pairs, label):
    import torch
    from tstar_amd.interface_searcher import TStarSearcher
    t = {"decoded": [], "resident": []}
    keys = {}
    for r in range(pairs + 1):                                       # pair 0 warms up
        for kind in (("decoded", "resident") if r % 2 == 0 else ("resident", "decoded")):
            s = TStarSearcher(stores[kind], h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(grid, grid), search_budget=budget,
                              confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ts = s.search()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            keys.setdefault(kind, [float(v) for v in ts])
            assert keys[kind] == [float(v) for v in ts]
            if r:
                t[kind].append(dt)
            last = dict(frames_scored=s.frames_scored, iterations=s.iterations)
    res = dict(search=label, grid=grid, budget=budget, **last, decoded_s=med_spread(t["decoded"]), resident_s=med_spread(t["resident"]),
               same_keyframes=keys["decoded"] == keys["resident"], pool=stores["resident"].pool_stats())
    res["resident_over_decoded"] = res["resident_s"]["median"] / res["decoded_s"]["median"]
    res["decoded_spread_rel"] = (res["decoded_s"]["max"] - res["decoded_s"]["min"]) / res["decoded_s"]["median"]
    print(json.dumps(res), flush=True)
    return res


def write_md(res, path):
    L = ["# Compressed-resident JPEG store against the decoded store on one MI355X", "",
         f"Device: {res['device']}.  Written by `tools/measure_jpeg_resident.py`; the JSON next to this file holds every run.  Decoded = "
         "`open_video(path, jpeg_entropy=\"device\")`, resident = `open_video(path, resident=\"jpeg\")` with the default pool of 512 slots.", ""]
    L += ["## HBM and open time", "", "| file | frames | file MB | decoded store MB | arena MB | pool MB | fetch workspace MB | arena + pool / decoded | open decoded s | open resident s |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        m = c["memory"]
        L.append(f"| {c['name']} | {c['frames']} | {c['file_bytes'] / 1e6:.1f} | {m['decoded'] / 1e6:.0f} | {m['arena'] / 1e6:.1f} | {m['pool'] / 1e6:.0f} | "
                 f"{m['workspace'] / 1e6:.0f} | {(m['arena'] + m['pool']) / m['decoded']:.3f} | {c['open']['decoded']['median']:.3f} | {c['open']['resident']['median']:.3f} |")
    L += ["", "## Fetch (`lease` of n seconds; HIP events around the call, host wall time inside it; medians)", "",
          "| file | n | cold ms | cold, host ms | ms per frame cold | every frame resident ms | resident, host ms |", "|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for f in c.get("fetch", []):
            L.append(f"| {c['name']} | {f['frames']} | {f['cold_s']['median'] * 1e3:.2f} | {f['cold_host_s']['median'] * 1e3:.2f} | "
                     f"{f['cold_s']['median'] * 1e3 / f['frames']:.3f} | {f['warm_s']['median'] * 1e3:.3f} | {f['warm_host_s']['median'] * 1e3:.3f} |")
    L += ["", f"## Searches (f32x3 synthetic OWL heuristic, K = 8, seed 2025; {res['pairs']} alternated pairs, median [min .. max] s)", "",
          "| file | search | iterations | frames scored | decoded s | resident s | resident / decoded | spread of the decoded runs | same keyframes | hits / misses / evictions |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cases"]:
        for s in c.get("searches", []):
            d, r, p = s["decoded_s"], s["resident_s"], s["pool"]
            L.append(f"| {c['name']} | {s['search']} | {s['iterations']} | {s['frames_scored']} | {d['median']:.3f} [{d['min']:.3f} .. {d['max']:.3f}] | "
                     f"{r['median']:.3f} [{r['min']:.3f} .. {r['max']:.3f}] | {s['resident_over_decoded']:.3f} | {s['decoded_spread_rel'] * 100:.1f} % | "
                     f"{s['same_keyframes']} | {p['hits']} / {p['misses']} / {p['evictions']} |")
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_resident_measure"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsal)")
    ap.add_argument("--only-search", choices=("decoded", "resident"), default=None,
                    help="four 4 x 4 searches on the first file's store of that kind and nothing else (for a kernel trace)")
    args = ap.parse_args()
    import torch
    from tstar_amd.interface_heuristic import OWLInterface
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pairs=args.pairs, repeats=args.repeats, cases=[])
    h = OWLInterface(synthetic_seed=0, max_batch=256, weights_dtype="f32x3")
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(32, int(n * args.scale))
            path = os.path.join(tmp, f"{name}.avi")
            make_avi(path, n, H, W)
            if args.only_search:
                from tstar_amd.video import open_video
                st = open_video(path, jpeg_entropy="device") if args.only_search == "decoded" else open_video(path, resident="jpeg")
                searches({"decoded": st, "resident": st}, h, 4, 1000, 1, f"{args.only_search} only")        # 4 searches: 2 "pairs" on the one store
                return
            stores, opens = open_both(path, args.repeats)
            dec, st = stores["decoded"], stores["resident"]
            ps = st.pool_stats()
            case = dict(name=name, frames=n, file_bytes=os.path.getsize(path), open=opens, decode_stats=st.decode_stats,
                        memory=dict(decoded=int(dec.frames.numel()), arena=ps["arena_bytes"], pool=ps["pool_bytes"], workspace=workspace_bytes(st)))
            print(json.dumps(case), flush=True)
            case["fetch"] = fetch_times(st)
            case["searches"] = [searches(stores, h, 4, 1000, args.pairs, "reference default: 4 x 4 grid, solo"),
                                searches(stores, h, 16, 1000, args.pairs, "configs[1]: 16 x 16 grid, budget 1000")]
            res["cases"].append(case)
            del stores, dec, st
            torch.cuda.empty_cache()
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    write_md(res, args.out + ".md")
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
