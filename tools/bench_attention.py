"""Attention kernel alone (vision shape: T = 577, 12 heads) at a few batch sizes; used by tools/pmc_attention_counters.sh.
    python tools/bench_attention.py [--kernel f32|x3] [--order 0|1] [--alternate N] [B ...]
--kernel x3: attention_x3_kernel (the f32x3 mode's); --order: its block order (0 linear, 1 XCD groups; default: the library's
choice, TSTAR_AX3_XCD_OFF in the environment gives 0); --alternate N: N rounds of order 0 then order 1 in ONE process (x3 only)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tstar_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", choices=["f32", "x3"], default="f32")
ap.add_argument("--order", type=int, choices=[0, 1], default=None)
ap.add_argument("--alternate", type=int, default=0)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("B", type=int, nargs="*")
args = ap.parse_args()

lib = _lib.load()
s = torch.cuda.current_stream().cuda_stream


def launcher(qkv, out, B, order):
    if args.kernel == "f32":
        return lambda: _lib.check(lib.tstar_attention_f32(qkv.data_ptr(), out.data_ptr(), B, 577, 12, 0, None, s))
    if order is None:
        return lambda: _lib.check(lib.tstar_attention_x3(qkv.data_ptr(), out.data_ptr(), B, 577, 12, s))
    return lambda: _lib.check(lib.tstar_attention_x3_order(qkv.data_ptr(), out.data_ptr(), B, 577, 12, order, s))


def timed(f, it):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


for B in args.B or [16, 64, 256]:
    M = B * 577
    qkv = torch.randn(M, 2304, device="cuda")
    out = torch.empty(M, 768, device="cuda")
    runs = [(r, o) for r in range(args.alternate) for o in (0, 1)] if args.alternate and args.kernel == "x3" else [(0, args.order)]
    for r, order in runs:
        ms = timed(launcher(qkv, out, B, order), args.iters)
        tag = "" if args.kernel == "f32" else f" x3 order={'lib' if order is None else order} round={r}"
        print(f"attn{tag} B={B:3d} {ms:8.3f} ms  {4.0 * B * 12 * 577 * 577 * 64 / ms / 1e9:8.1f} TFLOP/s", flush=True)
