"""Golden output digests of gemm_f32 (csrc/gemm_f32.hip) for tests/test_gpu_gemm_same_bits.py.
    python tools/record_gemm_bits.py --root PARENT_TREE [--out tests/golden/gemm_bits.json]
Loads the library BUILT IN `PARENT_TREE` (a checkout of the commit whose bits are the reference, built with its own
`python -m tstar_amd.build`), runs every case of MODES x SHAPES x EPILOGUES with the launcher's own tile choice (tile_cfg -1), checks that
every other tile_cfg the plan accepts gives the same bytes, and writes the SHA-256 of the output bytes.
Record from the parent of a change to the kernel, never from the changed kernel itself: the test then shows that the bits did not move.
The inputs are made here (seeded numpy) and the test imports them from this file, so both sides see the same arrays."""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_bits.json")

# name -> (TSTAR_WEIGHTS_* of tstar_gemm_plan, the diagnostic entry that converts W on every call)
MODES = {"f32": (0, "tstar_gemm_f32_cfg"), "bf16": (1, "tstar_gemm_bf16w2"), "bf16_exact": (3, "tstar_gemm_bf16w"), "f32x3": (4, "tstar_gemm_f32x3")}
# (M, N, K)
SHAPES = [(1, 128, 32),        # one row, one K tile
          (300, 256, 96),      # two full panels + 44 ragged rows, odd K-tile count (the peeled tile of the 64x64 ring)
          (577, 768, 768),     # one image's tokens: out-proj (two-term mode: N = 768)
          (130, 768, 3072),    # fc2's long loop
          (257, 2304, 768)]    # qkv's width, one row past two panels
EPILOGUES = {"bias": (0, False), "bias_res_inplace": (0, True), "qgelu": (1, False), "gelu": (2, False)}     # act, residual read and written in place


def case_key(M: int, N: int, K: int) -> str:
    return f"{M},{N},{K}"


def make_inputs(M: int, N: int, K: int):
    """A [M, K], W [N, K], bias [N], residual [M, N] float32: the wide-dynamic-range Gaussian operands of test_gemm_f32x3 (every 7th row
    scaled by 1e-3, every 5th column by 37, W by K**-0.5)."""
    rs = np.random.RandomState(9000 + 7 * M + 3 * N + K)
    A = rs.standard_normal((M, K)).astype(np.float32)
    A[::7] *= np.float32(1e-3)
    A[:, ::5] *= np.float32(37.0)
    W = (rs.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    b = rs.standard_normal(N).astype(np.float32)
    R = rs.standard_normal((M, N)).astype(np.float32)
    return A, W, b, R


def tile_cfgs(mode: str, M: int):
    cfgs = (-1, 0, 1, 2, 3, 17, 16 + (M + 127) // 128) + ((4, 5) if mode in ("bf16", "f32x3") else ()) + ((6,) if mode == "bf16" else ())
    return tuple(dict.fromkeys(cfgs))


def accepted_cfgs(lib, mode: str, M: int, N: int):
    """The tile_cfg values tstar_gemm_plan accepts for the mode's converting entry (which holds a fragment-packed plane where N % 256 == 0)."""
    out, plan = [], (ctypes.c_int * 4)()
    for cfg in tile_cfgs(mode, M):
        rc = lib.tstar_gemm_plan(MODES[mode][0], M, N, N, 0, cfg, int(mode == "bf16" and N % 256 == 0), plan)
        assert rc in (0, 1), rc
        if rc == 0:
            out.append(cfg)
    return out


def device_inputs(torch, M: int, N: int, K: int):
    return tuple(torch.from_numpy(x).cuda() for x in make_inputs(M, N, K))


def run_case(lib, check, torch, dev, mode: str, M: int, N: int, K: int, epilogue: str, cfg: int) -> str:
    dA, dW, db, dR = dev
    act, res = EPILOGUES[epilogue]
    dC = dR.clone() if res else torch.full((M, N), -7.0, dtype=torch.float32, device="cuda")
    entry = MODES[mode][1]
    check(getattr(lib, entry)(dA.data_ptr(), dW.data_ptr(), dC.data_ptr(), db.data_ptr(), dC.data_ptr() if res else None, M, N, K, act, cfg,
                              torch.cuda.current_stream().cuda_stream), entry)
    torch.cuda.synchronize()
    return hashlib.sha256(dC.cpu().numpy().astype("<f4", copy=False).tobytes()).hexdigest()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="tree whose built library is recorded (the parent commit's)")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    from tstar_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))) == root, _lib.__file__
    lib = _lib.load()
    digests = {}
    for M, N, K in SHAPES:
        dev = device_inputs(torch, M, N, K)
        for mode in MODES:
            for ep in EPILOGUES:
                got = {cfg: run_case(lib, _lib.check, torch, dev, mode, M, N, K, ep, cfg) for cfg in accepted_cfgs(lib, mode, M, N)}
                assert len(set(got.values())) == 1, f"tile forms disagree in the recorded tree: {mode} {(M, N, K)} {ep} {got}"
                digests.setdefault(mode, {}).setdefault(case_key(M, N, K), {})[ep] = got[-1]
                print(mode, case_key(M, N, K), ep, got[-1], f"({len(got)} tile_cfg)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "SHA-256 of gemm_f32 outputs (float32, little-endian, [M, N]) per weight mode, shape 'M,N,K' and epilogue; "
                           "inputs: tools/record_gemm_bits.py make_inputs",
                   "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
