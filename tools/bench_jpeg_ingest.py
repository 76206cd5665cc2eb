#!/usr/bin/env python
"""Measure the JPEG decode front end on one MI355X: Motion-JPEG AVI -> resident RGB store.

For a 3 600-frame 360x640 and a 600-frame 1080x1920 AVI (4:2:0, quality 85, the synthetic video, one frame per second so
that every frame is wanted) it reports wall time, frames/s and host CPU-seconds (time.process_time: all threads of the
process) of

  device   tstar_amd.video.open_video: host entropy stage on the thread pool + HIP reconstruction kernels
  pillow   what a user would otherwise write: Pillow decode on a 16-thread pool + the same chunked pinned upload

alternating in the same run, after a warm-up of each, and checks that both stores hold the same bytes.  It also times the
two halves of the device path on their own: the entropy stage (host clock) and the kernels of one resident chunk (HIP
events), with the kernels' bytes/s against the achievable-HBM figure of the microarchitecture guide.

  python tools/bench_jpeg_ingest.py --out profiles/jpeg_ingest_measure          # writes .md and .json
  python tools/bench_jpeg_ingest.py --entropy device                            # the same, with the entropy stage on the GPU
  python tools/bench_jpeg_ingest.py --entropy compare                           # host against device entropy, the split path on and
                                                                                # off (TSTAR_JPEG_SPLIT_BYTES=0) -> profiles/jpeg_split_entropy_measure
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_jpeg_ingest.py --kernels-only     # kernel times, a run of its own

No GPU -> error (a CPU timing says nothing about this).
"""
import argparse
import io
import json
import os
import struct
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12          # B/s, MI355X_MICROARCH.md (achievable, not the 8 TB/s peak)
CASES = [("360x640", 3600, 360, 640), ("1080x1920", 600, 1080, 1920)]
MODES = ("host", "device", "device, split off")          # --entropy compare


def write_avi(path, frames, W, H, rate):
    """The plainest AVI 1.0 an MJPG stream fits in: hdrl (avih, one strl), movi of 00dc chunks, idx1."""
    def chunk(cid, payload):
        return cid + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)

    def lst(kind, body):
        return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body

    n = len(frames)
    avih = struct.pack("<10I16x", 1000000 // rate, 0, 0, 0x10, n, 0, 1, max(map(len, frames)), W, H)
    strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, 1, rate, 0, n, 0, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    movi, index, pos = [], [], 4
    for fr in frames:
        c = chunk(b"00dc", fr)
        index.append(struct.pack("<4sIII", b"00dc", 0x10, pos, len(fr)))
        movi.append(c)
        pos += len(c)
    body = (b"AVI " + lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
            + lst(b"movi", b"".join(movi)) + chunk(b"idx1", b"".join(index)))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def make_avi(path, n, H, W, threads=16, restart_blocks=0):
    """restart_blocks > 0: a restart marker every that many MCUs."""
    from PIL import Image
    from tstar_amd.video import synthetic_video
    frames = synthetic_video(n, H, W, seed=21).frames.cpu().numpy()

    def enc(i):
        b = io.BytesIO()
        kw = {"restart_marker_blocks": restart_blocks} if restart_blocks else {}
        Image.fromarray(frames[i]).save(b, "JPEG", quality=85, subsampling=2, **kw)
        return b.getvalue()

    with ThreadPoolExecutor(threads) as ex:
        jpegs = list(ex.map(enc, range(n)))
    write_avi(path, jpegs, W, H, 1)
    return sum(len(j) for j in jpegs)


def pillow_baseline(path, chunk=64, threads=16):
    """Pillow decode on a thread pool + chunked upload through two pinned buffers on a side stream."""
    import torch
    from PIL import Image
    from tstar_amd import jpeg
    src = jpeg.avi_mjpeg(path)
    try:
        want = jpeg.wanted_frames(src.n_frames, src.fps)
        with Image.open(io.BytesIO(src.read(0))) as im:
            W, H = im.size
        store = torch.empty((len(want), H, W, 3), dtype=torch.uint8, device="cuda")
        pinned = [torch.empty((chunk, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        done = [None, None]
        side = torch.cuda.Stream()

        def dec(args):
            dst, fi = args
            with Image.open(io.BytesIO(src.read(fi))) as im:
                dst[...] = np.asarray(im.convert("RGB"))

        with ThreadPoolExecutor(threads) as ex:
            for ci, s0 in enumerate(range(0, len(want), chunk)):
                b = ci & 1
                if done[b] is not None:
                    done[b].synchronize()
                idx = want[s0:s0 + chunk]
                host = pinned[b].numpy()
                list(ex.map(dec, [(host[j], fi) for j, fi in enumerate(idx)]))
                with torch.cuda.stream(side):
                    store[s0:s0 + len(idx)].copy_(pinned[b][:len(idx)], non_blocking=True)
                    done[b] = torch.cuda.Event()
                    done[b].record(side)
        side.synchronize()
        return store
    finally:
        src.close()


def timed(fn):
    import torch
    torch.cuda.synchronize()
    w0, c0 = time.perf_counter(), time.process_time()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - w0, time.process_time() - c0


def halves(path, reps=20):
    """Entropy stage alone (host clock over every frame) and the kernels alone (HIP events, one resident chunk)."""
    import torch
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    src = jpeg.avi_mjpeg(path)
    try:
        n_all = src.n_frames
        rc, geom, _ = jpeg.probe(src.read(0))
        assert rc == 0
        blocks, plane_bytes = jpeg._sizes(geom)
        W, H = geom[0], geom[1]
        chunk = max(1, min(64, (48 << 20) // (blocks * 128)))
        coef = np.empty((chunk, blocks * 64), dtype=np.int16)
        quant = np.empty((chunk, 192), dtype=np.uint16)
        read_s = ent_w = ent_c = 0.0
        for s0 in range(0, n_all, chunk):
            t0 = time.perf_counter()
            datas = [src.read(i) for i in range(s0, min(n_all, s0 + chunk))]
            t1, c1 = time.perf_counter(), time.process_time()
            status, _ = jpeg.entropy_batch(datas, geom, coef, quant)
            ent_w += time.perf_counter() - t1
            ent_c += time.process_time() - c1
            read_s += t1 - t0
            assert not status.any()
        n = min(chunk, n_all)
        # Successive launches walk over `sets` separate copies of the chunk's buffers, 1 GiB in all: a single chunk's working set
        # (~110 MB) would sit in the 256 MB Infinity Cache and the rate would not be an HBM rate.
        set_bytes = n * (blocks * 128 + 384 + plane_bytes + W * H * 3)
        sets = max(2, -(-(1 << 30) // set_bytes))
        d_coef = [torch.from_numpy(coef).cuda() for _ in range(sets)]
        d_quant = [torch.from_numpy(quant.view(np.int16)).cuda() for _ in range(sets)]
        planes = [torch.empty((chunk, plane_bytes), dtype=torch.uint8, device="cuda") for _ in range(sets)]
        rgb = [torch.empty((chunk, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(sets)]

        def run(k):
            k %= sets
            _lib.check(lib.tstar_jpeg_reconstruct(d_coef[k].data_ptr(), d_quant[k].data_ptr(), n, *geom, planes[k].data_ptr(),
                                                  rgb[k].data_ptr(), _lib.stream_ptr()), "tstar_jpeg_reconstruct")
        for k in range(sets):
            run(k)
        reps = max(reps, 2 * sets)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            run(k)
        e1.record()
        torch.cuda.synchronize()
        dev_s = e0.elapsed_time(e1) * 1e-3 / reps
        # bytes the algorithm needs per frame: coefficients + tables in, planes out and in again, RGB out
        per_frame = blocks * 128 + 384 + 2 * plane_bytes + W * H * 3
        return dict(chunk=n, buffer_sets=sets, launches_timed=reps, entropy_wall_s=ent_w, entropy_cpu_s=ent_c, file_read_s=read_s, frames=n_all,
                    kernels_s_per_chunk=dev_s, kernels_s_all_frames=dev_s / n * n_all, bytes_per_frame=per_frame,
                    kernels_bytes_per_s=per_frame * n / dev_s, share_of_achievable_hbm=per_frame * n / dev_s / HBM_ACHIEVABLE,
                    h2d_bytes_per_frame=blocks * 128 + 384, threads=int(lib.tstar_jpeg_threads(0)))
    finally:
        src.close()


def device_entropy_figures(path, reps=10):
    """What the device entropy path moves and how long its kernel takes: upload bytes per frame over every chunk of the
    file (compressed bytes + records, as load_jpeg sends them), and the launch (coefficient clear + kernel) of the first chunk
    by HIP events."""
    import torch
    from tstar_amd import _lib, jpeg
    src = jpeg.avi_mjpeg(path)
    try:
        n_all = src.n_frames
        rc, geom, _ = jpeg.probe(src.read(0))
        assert rc == 0
        blocks, _ = jpeg._sizes(geom)
        chunk = jpeg.device_entropy_chunk(blocks, n_all)
        up = segs = host_routed = 0
        t_plan = c_plan = 0.0
        first = None
        for s0 in range(0, n_all, chunk):
            datas = [src.read(i) for i in range(s0, min(n_all, s0 + chunk))]
            t0, c0 = time.perf_counter(), time.process_time()
            batch = jpeg.DeviceBatch(datas, geom)
            t_plan += time.perf_counter() - t0
            c_plan += time.process_time() - c0
            up += batch.nbytes
            segs += len(batch.plan.segments)
            host_routed += int(batch.plan.route.sum())
            if first is None:
                first = batch
        n = len(first.datas)
        host = np.zeros(first.nbytes, dtype=np.uint8)
        first.fill(host)
        d_buf = torch.from_numpy(host).cuda()
        d_coef = torch.empty((n, blocks * 64), dtype=torch.int16, device="cuda")
        d_status = torch.empty(len(first.plan.segments), dtype=torch.int32, device="cuda")
        first.launch(d_buf, d_coef, d_status, geom, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert not d_status.cpu().numpy().any()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            first.launch(d_buf, d_coef, d_status, geom, _lib.stream_ptr())
        e1.record()
        torch.cuda.synchronize()
        per_chunk = e0.elapsed_time(e1) * 1e-3 / reps
        # the split launcher on the same resident chunk: the defaults, then a sweep of each argument around them
        nseg = len(first.plan.segments)
        d_info = torch.empty(nseg, dtype=torch.int32, device="cuda")

        def split_launch(sub, min_split, rounds, reps):
            ws = torch.empty(jpeg.split_workspace_bytes(first.total, nseg, sub) // 8, dtype=torch.int64, device="cuda")
            run = lambda: first.launch_split(d_buf, d_coef, d_status, d_info, ws, geom, _lib.stream_ptr(), sub, min_split, rounds)  # noqa: E731
            run()
            torch.cuda.synchronize()
            assert not d_status.cpu().numpy().any()
            info = d_info.cpu().numpy()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps, info

        sub0, min0, rounds0 = jpeg.SPLIT_SUB_BYTES, jpeg.SPLIT_MIN_BYTES, jpeg.SPLIT_MAX_ROUNDS
        split_s, info = split_launch(sub0, min0, rounds0, reps)
        hist = {str(int(k)): int(v) for k, v in zip(*np.unique(info, return_counts=True))}
        sweep = []
        for sub, min_split, rounds in ([(sb, min0, rounds0) for sb in (32, 64, 128, 256, 512)] + [(sub0, ms, rounds0) for ms in (256, 4096, 16384)]
                                       + [(sub0, min0, r) for r in (8, 16, 96)]):
            t, inf = split_launch(sub, min_split, rounds, 3)
            sweep.append(dict(sub_bytes=sub, min_split_bytes=min_split, max_rounds=rounds, s_per_chunk=t, split=int((inf != 0).sum()),
                              abandoned=int((inf < 0).sum()), rounds_max=int(inf.max(initial=0))))
        return dict(split_kernel_s_per_chunk=split_s, split_kernel_s_all_frames=split_s / n * n_all, split_rounds_histogram=hist,
                    split_sweep=sweep, split_defaults=dict(sub_bytes=sub0, min_split_bytes=min0, max_rounds=rounds0),
                    chunk=n, frames=n_all, segments_per_frame=segs / n_all, host_routed=host_routed, table_sets_first_chunk=len(first.plan.table_sets),
                    h2d_bytes_per_frame=up / n_all, h2d_bytes_per_frame_host_mode=blocks * 128 + 384, plan_wall_s=t_plan, plan_cpu_s=c_plan,
                    entropy_kernel_s_per_chunk=per_chunk, entropy_kernel_s_all_frames=per_chunk / n * n_all, launches_timed=reps)
    finally:
        src.close()


def compare_entropy(args):
    """Host against device entropy through open_video, the device mode with the split path on (the default) and off
    (TSTAR_JPEG_SPLIT_BYTES=0: one lane per segment, the device mode before the split path), alternating in one process; the host
    mode is the baseline."""
    import torch
    from tstar_amd.video import open_video
    props = torch.cuda.get_device_properties(0)
    res = {"board": f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')})", "cpus_allowed": len(os.sched_getaffinity(0)), "cases": {}}
    cases = [(name, n, H, W, 0) for name, n, H, W in CASES] + [("360x640, restart per MCU row", 3600, 360, 640, 640 // 16)]
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, n, H, W, restart) in enumerate(cases):
            n = max(8, int(n * args.scale))
            path = os.path.join(tmp, f"case{k}.avi")
            jpeg_bytes = make_avi(path, n, H, W, restart_blocks=restart)
            print(f"[{name}] {n} frames, {jpeg_bytes / n / 1024:.1f} KiB/frame", flush=True)
            case = {"frames": n, "jpeg_bytes_per_frame": jpeg_bytes / n, "host": [], "device": [], "device, split off": []}

            def open_mode(mode):
                os.environ.pop("TSTAR_JPEG_SPLIT_BYTES", None)
                if mode == "device, split off":
                    os.environ["TSTAR_JPEG_SPLIT_BYTES"] = "0"
                try:
                    return open_video(path, jpeg_entropy="host" if mode == "host" else "device")
                finally:
                    os.environ.pop("TSTAR_JPEG_SPLIT_BYTES", None)

            a, b, b0 = (open_mode(m) for m in MODES)                                                   # warm-up of all
            case["same_bytes"] = bool(torch.equal(a.frames, b.frames) and torch.equal(a.frames, b0.frames))
            case["entropy_stats"] = b.entropy_stats
            case["entropy_split_stats"] = b.entropy_split_stats
            del a, b, b0
            for _ in range(args.repeats):
                for mode in MODES:
                    st, w, c = timed(lambda: open_mode(mode))
                    case[mode].append({"wall_s": w, "cpu_s": c, "frames_per_s": n / w})
                    del st
            for mode in MODES:
                case[mode + "_median"] = {m: float(np.median([r[m] for r in case[mode]])) for m in ("wall_s", "cpu_s", "frames_per_s")}
            case["figures"] = device_entropy_figures(path)
            res["cases"][name] = case
            print(json.dumps({name: {k2: case[k2] for k2 in ("host_median", "device_median", "device, split off_median", "same_bytes", "entropy_split_stats", "figures")}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(args.out + ".md", "w") as f:
        f.write(f"# JPEG ingest: entropy stage on the host against on the device ({res['board']}, {res['cpus_allowed']} CPUs allowed)\n\n"
                "`tools/bench_jpeg_ingest.py --entropy compare`; Motion-JPEG AVI -> resident store through `open_video`, 4:2:0, quality 85, "
                f"synthetic video, every frame wanted. Medians of {args.repeats} runs of each mode, alternating in one process after one warm-up of "
                "each; the host mode is the behaviour before the device stage existed and is the baseline; `device, split off` is the device "
                "mode with `TSTAR_JPEG_SPLIT_BYTES=0` (one lane per segment). CPU-seconds = `time.process_time` "
                "(all threads).\n\n| case | entropy on | wall s | frames/s | host CPU-s | H2D bytes/frame | segments/frame |\n|---|---|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            g = c["figures"]
            for mode in MODES:
                m = c[mode + "_median"]
                h2d = g["h2d_bytes_per_frame_host_mode"] if mode == "host" else g["h2d_bytes_per_frame"]
                f.write(f"| {name} x {c['frames']} | {mode} | {m['wall_s']:.3f} | {m['frames_per_s']:.0f} | {m['cpu_s']:.2f} | {h2d:.0f} | "
                        f"{g['segments_per_frame']:.0f} |\n")
        f.write("\nAll runs:\n\n")
        for name, c in res["cases"].items():
            for mode in MODES:
                f.write(f"- {name}, {mode}: wall " + ", ".join(f"{r['wall_s']:.3f}" for r in c[mode]) + " s; CPU "
                        + ", ".join(f"{r['cpu_s']:.2f}" for r in c[mode]) + f" s; stores byte-equal: {c['same_bytes']}; {c['entropy_stats']}; "
                        f"split on: {c['entropy_split_stats']}\n")
        f.write("\n## The entropy kernel alone\n\n| case | frames per chunk | segments (lanes) per chunk | clear + kernel, one chunk s (HIP events) | "
                "all frames s | planning on the host, all frames: wall s (CPU-s) |\n|---|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            g = c["figures"]
            f.write(f"| {name} | {g['chunk']} | {g['segments_per_frame'] * g['chunk']:.0f} | {g['entropy_kernel_s_per_chunk']:.4f} | "
                    f"{g['entropy_kernel_s_all_frames']:.3f} | {g['plan_wall_s']:.3f} ({g['plan_cpu_s']:.2f}) |\n")
        f.write("\nOne lane decodes one segment, so a file without restart markers gives one lane per frame; the kernel time is that of "
                f"the slowest lane. The launch is timed over {next(iter(res['cases'].values()))['figures']['launches_timed']} repeats on a resident chunk.\n")
        d = next(iter(res["cases"].values()))["figures"]["split_defaults"]
        f.write(f"\n## The split launcher alone (sub_bytes {d['sub_bytes']}, min_split_bytes {d['min_split_bytes']}, max_rounds {d['max_rounds']})\n\n"
                "The same resident chunk through `tstar_jpeg_entropy_split_device` (clear + every launch of the call, HIP events). seg_info "
                "histogram of that chunk: `0` one lane, `r` converged in round r, `-1` abandoned.\n\n"
                "| case | one chunk s | all frames s | one lane per segment, all frames s | seg_info: segments |\n|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            g = c["figures"]
            hist = ", ".join(f"{k}: {v}" for k, v in sorted(g["split_rounds_histogram"].items(), key=lambda kv: int(kv[0])))
            f.write(f"| {name} | {g['split_kernel_s_per_chunk']:.5f} | {g['split_kernel_s_all_frames']:.4f} | {g['entropy_kernel_s_all_frames']:.4f} | {hist} |\n")
        f.write("\nSweep, one argument at a time around the defaults (3 launches each; s per chunk):\n\n| case | sub_bytes | min_split_bytes | "
                "max_rounds | one chunk s | split | abandoned | rounds_max |\n|---|---|---|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            for r in c["figures"]["split_sweep"]:
                f.write(f"| {name} | {r['sub_bytes']} | {r['min_split_bytes']} | {r['max_rounds']} | {r['s_per_chunk']:.5f} | {r['split']} | "
                        f"{r['abandoned']} | {r['rounds_max']} |\n")
    print("wrote", args.out + ".md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="path stem of the .md / .json written (default: profiles/jpeg_ingest_measure, or "
                                                "profiles/jpeg_split_entropy_measure with --entropy compare)")
    ap.add_argument("--entropy", choices=("host", "device", "compare"), default="host",
                    help="where the device path entropy-decodes; 'compare' measures both modes against each other instead of against Pillow")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (rehearsal)")
    ap.add_argument("--kernels-only", action="store_true", help="only run the kernels of one chunk per case (for a rocprofv3 run)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_ingest needs an MI355X: a CPU timing says nothing about this path")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_split_entropy_measure" if args.entropy == "compare" else "jpeg_ingest_measure")
    if args.entropy == "compare":
        return compare_entropy(args)
    from tstar_amd import video
    open_video = lambda p: video.open_video(p, jpeg_entropy=args.entropy)      # noqa: E731
    props = torch.cuda.get_device_properties(0)
    res = {"board": f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')})", "cpus_allowed": len(os.sched_getaffinity(0)), "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in CASES:
            n = max(8, int(n * args.scale))
            path = os.path.join(tmp, name + ".avi")
            t0 = time.perf_counter()
            jpeg_bytes = make_avi(path, n, H, W)
            print(f"[{name}] {n} frames, {jpeg_bytes / n / 1024:.1f} KiB/frame, made in {time.perf_counter() - t0:.1f} s", flush=True)
            if args.kernels_only:
                print(json.dumps(halves(path, reps=10)), flush=True)
                continue
            case = {"frames": n, "jpeg_bytes_per_frame": jpeg_bytes / n, "device": [], "pillow": []}
            a = open_video(path)                       # warm-up of both paths (code objects, pinned allocations, page cache)
            b = pillow_baseline(path)
            case["same_bytes"] = bool(torch.equal(a.frames, b))
            case["decode_stats"] = a.decode_stats
            del a, b
            for _ in range(args.repeats):              # alternating, same run, same box
                st, w, c = timed(lambda: open_video(path))
                case["device"].append({"wall_s": w, "cpu_s": c, "frames_per_s": n / w})
                del st
                st, w, c = timed(lambda: pillow_baseline(path))
                case["pillow"].append({"wall_s": w, "cpu_s": c, "frames_per_s": n / w})
                del st
            case["halves"] = halves(path)
            for k in ("device", "pillow"):
                case[k + "_median"] = {m: float(np.median([r[m] for r in case[k]])) for m in ("wall_s", "cpu_s", "frames_per_s")}
            res["cases"][name] = case
            print(json.dumps({name: {k: case[k] for k in ("device_median", "pillow_median", "same_bytes")}}), flush=True)
    if args.kernels_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(args.out + ".md", "w") as f:
        f.write(f"# JPEG ingest: Motion-JPEG AVI -> resident store ({res['board']}, {res['cpus_allowed']} CPUs allowed)\n\n"
                "`tools/bench_jpeg_ingest.py`; 4:2:0, quality 85, synthetic video, every frame wanted (1 fps). Medians of "
                f"{args.repeats} alternating runs after one warm-up of each path; CPU-seconds = `time.process_time` (all threads).\n\n"
                "| case | path | wall s | frames/s | host CPU-s | CPU-s per 1000 frames |\n|---|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            for k, label in (("device", "entropy on host + HIP kernels"), ("pillow", "Pillow x16 threads + pinned upload")):
                m = c[k + "_median"]
                f.write(f"| {name} x {c['frames']} | {label} | {m['wall_s']:.3f} | {m['frames_per_s']:.0f} | {m['cpu_s']:.2f} | "
                        f"{1000 * m['cpu_s'] / c['frames']:.2f} |\n")
        f.write("\nAll runs:\n\n")
        for name, c in res["cases"].items():
            for k in ("device", "pillow"):
                f.write(f"- {name} {k}: wall " + ", ".join(f"{r['wall_s']:.3f}" for r in c[k]) + " s; CPU "
                        + ", ".join(f"{r['cpu_s']:.2f}" for r in c[k]) + f" s; stores byte-equal: {c['same_bytes']}\n")
        f.write("\n## The two halves of the device path\n\n| case | entropy stage, all frames: wall s (CPU-s, threads) | reading the frames from the file s | "
                "kernels, all frames s (HIP events) | kernel traffic B/frame | kernels B/s | share of 6.3 TB/s achievable HBM |\n|---|---|---|---|---|---|---|\n")
        for name, c in res["cases"].items():
            h = c["halves"]
            f.write(f"| {name} | {h['entropy_wall_s']:.3f} ({h['entropy_cpu_s']:.2f}, {h['threads']}) | {h['file_read_s']:.3f} | "
                    f"{h['kernels_s_all_frames']:.4f} | {h['bytes_per_frame']} | {h['kernels_bytes_per_s']:.3e} | "
                    f"{100 * h['share_of_achievable_hbm']:.1f} % |\n")
        f.write("\nKernel traffic counts what the algorithm needs: coefficients and tables in, u8 planes out and in again, RGB out. "
                "The kernels are timed on chunks already resident in HBM, successive launches cycling over separate copies of the "
                "buffers (1 GiB in all, buffer_sets in the .json) so that the 256 MB Infinity Cache cannot serve them; the host-to-device copy of the coefficients "
                "(2 B per padded sample, see h2d_bytes_per_frame in the .json) is part of the end-to-end wall time only.\n")
    print("wrote", args.out + ".md")


if __name__ == "__main__":
    main()
