"""JPEG decode at 1/2, 1/4, 1/8 size against the full-size decode on one MI355X -> profiles/jpeg_scale_measure.md / .json.

The two files of tools/bench_jpeg_ingest.py (3 600 x 360x640 and 600 x 1080x1920 Motion-JPEG AVI, quality 85, 4:2:0, no restart
markers), each opened with ``jpeg_scale`` 1, 2, 4, 8 -- scale 1 is the baseline, the code path without the keyword:

* open wall time and host CPU-seconds in host-entropy mode, in device-entropy mode and as a compressed-resident store, medians
  of --repeats runs in which the scales alternate;
* store / pool bytes, which must be N * ceil(H / s) * ceil(W / s) * 3 (pool: slots instead of N);
* the reconstruct kernels alone (tstar_jpeg_reconstruct_scaled over one resident chunk of coefficients, HIP events), with the
  coefficient bytes they read per second as a share of the achievable HBM rate: the coefficient layout is that of the full-size
  decode at every scale, so this is the floor of the stage;
* a cold 16-frame fetch on the resident store (HIP events around ``lease``);
* a reference-default 4 x 4 solo search and a 16 x 16 throughput search (budget 1000) on the decoded store with a synthetic
  f32x3 OWL heuristic.  A search on a scaled store sees other pixels than one on the full-size store: the keyframes may differ.

    python tools/measure_jpeg_scale.py [--scale 0.1]
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

from bench_jpeg_ingest import CASES, HBM_ACHIEVABLE, make_avi, timed  # noqa: E402

SCALES = (1, 2, 4, 8)
MODES = ("host entropy", "device entropy", "resident")


def med_spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), runs=[float(x) for x in v])


def _open(path, mode, s):
    from tstar_amd.video import open_video
    kw = {} if s == 1 else {"jpeg_scale": s}                           # scale 1: the call as it was before the keyword
    if mode == "resident":
        return open_video(path, resident="jpeg", **kw)
    return open_video(path, jpeg_entropy="host" if mode == "host entropy" else "device", **kw)


def opens(path, H, W, repeats):
    """-> {mode: {scale: {wall_s, cpu_s, bytes}}}; the byte counts are asserted against the ceil formula."""
    import torch
    out = {m: {s: dict(wall=[], cpu=[]) for s in SCALES} for m in MODES}
    for r in range(repeats + 1):                                       # run 0 warms up
        for mode in MODES:
            for s in (SCALES if r % 2 == 0 else SCALES[::-1]):
                torch.cuda.empty_cache()
                st, wall, cpu = timed(lambda: _open(path, mode, s))
                per = -(-H // s) * -(-W // s) * 3
                if mode == "resident":
                    nbytes = st.pool_stats()["pool_bytes"]
                    assert nbytes == (st.pool_frames + st.pool_stats()["exceptions"]) * per, (mode, s, nbytes)
                else:
                    nbytes = int(st.frames.numel())
                    assert nbytes == st.num_seconds * per, (mode, s, nbytes)
                assert st.decode_stats["pillow"] == 0
                out[mode][s]["bytes"] = nbytes
                if r:
                    out[mode][s]["wall"].append(wall)
                    out[mode][s]["cpu"].append(cpu)
                del st
    return {m: {s: dict(wall_s=med_spread(v["wall"]), cpu_s=med_spread(v["cpu"]), bytes=v["bytes"]) for s, v in d.items()} for m, d in out.items()}


def kernels(path, reps=20):
    """The reconstruct stage alone over one chunk of resident coefficients -> {scale: seconds per frame, share of HBM}."""
    import torch
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    src = jpeg.avi_mjpeg(path)
    try:
        rc, geom, _ = jpeg.probe(src.read(0))
        assert rc == 0
        blocks, _ = jpeg._sizes(geom)
        n = max(1, min(64, src.n_frames, (48 << 20) // (blocks * 128)))
        coef = np.empty((n, blocks * 64), dtype=np.int16)
        quant = np.empty((n, 192), dtype=np.uint16)
        status, _ = jpeg.entropy_batch([src.read(i) for i in range(n)], geom, coef, quant)
        assert not status.any()
    finally:
        src.close()
    d_coef, d_quant = torch.from_numpy(coef).cuda(), torch.from_numpy(quant.view(np.int16)).cuda()
    out = {}
    for s in SCALES:
        ow, oh, plane_bytes, covered = jpeg.scaled_sizes(geom, s)
        assert covered
        planes = torch.empty(n * plane_bytes, dtype=torch.uint8, device="cuda")
        rgb = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        times = []
        for r in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.tstar_jpeg_reconstruct_scaled(d_coef.data_ptr(), d_quant.data_ptr(), n, *geom, s, planes.data_ptr(), rgb.data_ptr(),
                                                         _lib.stream_ptr()), "tstar_jpeg_reconstruct_scaled")
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(e0.elapsed_time(e1) * 1e-3)
        t = float(np.median(times))
        traffic = blocks * 128 + 2 * plane_bytes + oh * ow * 3          # coefficients in, planes out and in again, RGB out
        out[s] = dict(frames=n, seconds=t, us_per_frame=t / n * 1e6, coef_bytes_per_frame=blocks * 128, traffic_bytes_per_frame=traffic,
                      coef_share_of_achievable_hbm=blocks * 128 * n / t / HBM_ACHIEVABLE, traffic_share_of_achievable_hbm=traffic * n / t / HBM_ACHIEVABLE)
    return out


def fetch16(path, reps=5):
    """A cold lease of 16 seconds on the resident store at every scale (HIP events around the call)."""
    import torch
    out = {}
    for s in SCALES:
        st = _open(path, "resident", s)
        ts = []
        for r in range(reps + 1):
            base = (r * 16) % (st.num_seconds - 15)
            st.flush()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            lease = st.lease(list(range(base, base + 16)))
            e1.record()
            lease.done()
            torch.cuda.synchronize()
            if r:
                ts.append(e0.elapsed_time(e1) * 1e-3)
        assert st.fetch_errors() == 0
        out[s] = med_spread(ts)
        del st
    return out


def searches(path, h, grid, budget, repeats, label):
    import torch
    from tstar_amd.interface_searcher import TStarSearcher
    stores = {s: _open(path, "device entropy", s) for s in SCALES}
    t, keys, last = {s: [] for s in SCALES}, {}, {}
    for r in range(repeats + 1):
        for s in (SCALES if r % 2 == 0 else SCALES[::-1]):
            se = TStarSearcher(stores[s], h, ["couch"], ["tv", "chair"], search_nframes=8, image_grid_shape=(grid, grid), search_budget=budget,
                               confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, ts = se.search()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            keys.setdefault(s, [float(v) for v in ts])
            assert keys[s] == [float(v) for v in ts]
            if r:
                t[s].append(dt)
            last[s] = dict(frames_scored=se.frames_scored, iterations=se.iterations)
    res = dict(search=label, grid=grid, budget=budget,
               scales={s: dict(seconds=med_spread(t[s]), **last[s], same_keyframes_as_full_size=keys[s] == keys[1]) for s in SCALES})
    print(json.dumps(res), flush=True)
    return res


def write_md(res, path):
    L = ["# JPEG decode at 1/2, 1/4, 1/8 size against the full-size decode on one MI355X", "",
         f"Device: {res['device']}; the host entropy stage runs on {min(16, res['cpus_allowed'])} threads.  Written by `tools/measure_jpeg_scale.py`; the JSON next to this file holds every "
         f"run.  Scale 1 is `open_video` without the keyword: the baseline every column is read against.  Medians of {res['repeats']} runs in "
         "which the scales alternate.", ""]
    for c in res["cases"]:
        L += [f"## {c['name']}, {c['frames']} frames, {c['file_bytes'] / 1e6:.1f} MB file", "",
              "| mode | scale | store / pool MB | open wall s [min .. max] | host CPU-s | wall against scale 1 |", "|---|---|---|---|---|---|"]
        for m in MODES:
            for s in SCALES:
                v, base = c["open"][m][s], c["open"][m][1]
                w = v["wall_s"]
                L.append(f"| {m} | 1/{s} | {v['bytes'] / 1e6:.1f} | {w['median']:.3f} [{w['min']:.3f} .. {w['max']:.3f}] | {v['cpu_s']['median']:.2f} | "
                         f"{w['median'] / base['wall_s']['median']:.2f} |")
        L += ["", "Reconstruct kernels alone (HIP events over one chunk of resident coefficients):", "",
              "| scale | us per frame | against scale 1 | coefficient bytes read / s, share of 6.3 TB/s | all traffic, share |", "|---|---|---|---|---|"]
        k1 = c["kernels"][1]
        for s in SCALES:
            k = c["kernels"][s]
            L.append(f"| 1/{s} | {k['us_per_frame']:.2f} | {k['us_per_frame'] / k1['us_per_frame']:.2f} | "
                     f"{100 * k['coef_share_of_achievable_hbm']:.1f} % | {100 * k['traffic_share_of_achievable_hbm']:.1f} % |")
        L += ["", "Cold fetch of 16 frames on the resident store (gather + entropy + reconstruct, HIP events around `lease`):", "",
              "| scale | ms [min .. max] |", "|---|---|"]
        for s in SCALES:
            f = c["fetch16"][s]
            L.append(f"| 1/{s} | {f['median'] * 1e3:.2f} [{f['min'] * 1e3:.2f} .. {f['max'] * 1e3:.2f}] |")
        L += ["", "Searches on the decoded store (f32x3 synthetic OWL heuristic, K = 8, seed 2025):", "",
              "| search | scale | s [min .. max] | against scale 1 | iterations | frames scored | keyframes of the full-size search |", "|---|---|---|---|---|---|---|"]
        for se in c["searches"]:
            b = se["scales"][1]["seconds"]["median"]
            for s in SCALES:
                v = se["scales"][s]
                w = v["seconds"]
                L.append(f"| {se['search']} | 1/{s} | {w['median']:.3f} [{w['min']:.3f} .. {w['max']:.3f}] | {w['median'] / b:.2f} | {v['iterations']} | "
                         f"{v['frames_scored']} | {v['same_keyframes_as_full_size']} |")
        L.append("")
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_scale_measure"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsal)")
    args = ap.parse_args()
    import torch
    from tstar_amd.interface_heuristic import OWLInterface
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), cpus_allowed=len(os.sched_getaffinity(0)), repeats=args.repeats, cases=[])
    h = OWLInterface(synthetic_seed=0, max_batch=256, weights_dtype="f32x3")
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(32, int(n * args.scale))
            path = os.path.join(tmp, f"{name}.avi")
            make_avi(path, n, H, W)
            case = dict(name=name, frames=n, file_bytes=os.path.getsize(path), open=opens(path, H, W, args.repeats))
            print(json.dumps(case), flush=True)
            case["kernels"] = kernels(path)
            print(json.dumps(case["kernels"]), flush=True)
            case["fetch16"] = fetch16(path)
            print(json.dumps(case["fetch16"]), flush=True)
            case["searches"] = [searches(path, h, 4, 1000, args.repeats, "reference default: 4 x 4 grid, solo")]
            if n >= 256:                                               # a 16 x 16 grid is 256 frames: a rehearsal file may be shorter
                case["searches"].append(searches(path, h, 16, 1000, args.repeats, "configs[1]: 16 x 16 grid, budget 1000"))
            res["cases"].append(case)
            torch.cuda.empty_cache()
            with open(args.out + ".json", "w") as f:                  # after every case: a run that is cut short leaves what it measured
                json.dump(res, f, indent=1)
    write_md(res, args.out + ".md")
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
