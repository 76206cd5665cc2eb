"""Golden output digests of attention_x3_kernel for tests/test_gpu_attention_x3_same_bits.py.
    python tools/record_attention_x3_bits.py --root PARENT_TREE [--out tests/golden/attention_x3_bits.json]
Loads the library BUILT IN `PARENT_TREE` (a checkout of the commit whose bits are the reference, built with its own
`python -m tstar_amd.build`), runs every case of CASES x INPUT_KINDS in both block orders and writes the SHA-256 of the output bytes.
Record from the parent of a change to the kernel, never from the changed kernel itself: the test then shows that the bits did not move.
The inputs are made here (seeded numpy) and the test imports them from this file, so both sides see the same arrays."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_x3_bits.json")

# (B, heads, T)
CASES = [(2, 2, 577),      # paired loop + peeled tiles + straggler key
         (3, 2, 97),       # 3 tiles, no paired loop, odd group padding
         (2, 1, 337),      # masked last tile, odd tile count
         (1, 2, 64),       # no straggler, no mask
         (1, 1, 33),       # one tile + straggler
         (1, 1, 1),        # straggler only
         (2, 12, 129)]     # second query block nearly empty
INPUT_KINDS = ("plain", "late_max")
ORDERS = (0, 1)            # linear, XCD groups


def case_key(B: int, heads: int, T: int) -> str:
    return f"{B},{heads},{T}"


def make_qkv(B: int, heads: int, T: int, kind: str) -> np.ndarray:
    """[B * T, 3 * heads * 64] float32.  late_max: every query of a head shares a component u and the LAST key of the last key tile
    the matrix pipe handles is 3 u, so that each query meets its largest score (about 24 against at most 8 elsewhere) in that tile
    and the alpha rescale of the output runs there."""
    rs = np.random.RandomState(7000 + 101 * T + 11 * heads + B + (50000 if kind == "late_max" else 0))
    D = heads * 64
    qkv = rs.standard_normal((B * T, 3 * D)).astype(np.float32)
    if kind == "late_max":
        key = T - 2 if T % 32 == 1 else T - 1          # T = 32 n + 1: key T - 1 is the straggler, folded in after the tiles
        x = qkv.reshape(B, T, 3, heads, 64)
        u = rs.standard_normal((B, heads, 64)).astype(np.float32)
        x[:, :, 0] += u[:, None]
        if key >= 0:
            x[:, key, 1] = 3.0 * u
    return qkv


def run_case(lib, check, torch, B: int, heads: int, T: int, kind: str, order: int) -> str:
    qkv = torch.from_numpy(make_qkv(B, heads, T, kind)).cuda()
    out = torch.full((B * T, heads * 64), -7.0, dtype=torch.float32, device="cuda")
    check(lib.tstar_attention_x3_order(qkv.data_ptr(), out.data_ptr(), B, T, heads, order, torch.cuda.current_stream().cuda_stream),
          "tstar_attention_x3_order")
    torch.cuda.synchronize()
    return hashlib.sha256(out.cpu().numpy().astype("<f4", copy=False).tobytes()).hexdigest()


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
    for B, heads, T in CASES:
        digests[case_key(B, heads, T)] = {kind: {str(o): run_case(lib, _lib.check, torch, B, heads, T, kind, o) for o in ORDERS}
                                          for kind in INPUT_KINDS}
        print(case_key(B, heads, T), digests[case_key(B, heads, T)], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "SHA-256 of attention_x3 outputs (float32, little-endian, [B * T, heads * 64]) per case 'B,heads,T', "
                           "input kind and block order; inputs: tools/record_attention_x3_bits.py make_qkv",
                   "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
