"""Compiled form of attention_x3_kernel<false>: what the compiler made of the key loop.
    python tools/attention_x3_isa.py [--lab] [--keep FILE] [extra hipcc flags ...]
Compiles tstar_amd/csrc/attention_x3.hip (--lab: tools/lab/attn_lab.hip) to gfx950 assembly with build.py's own flags and prints, for
every loop of the kernel, its MFMAs, its other VALU instructions and the packed f32 arithmetic between its first and last MFMA, then
the kernel's register / scratch metadata.  tests/test_attention_x3_compiled_form.py asserts on the same figures."""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tstar_amd import build as B  # noqa: E402

KERNEL = "attention_x3_kernelILb0EE"
PACKED_F32 = ("v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")
LIB_SRC = os.path.join(B.CSRC, "attention_x3.hip")
LAB_SRC = os.path.join(ROOT, "tools", "lab", "attn_lab.hip")


def flags(src: str = "attention_x3.hip") -> list:
    """build.py's device flags for `src` (the lab is built with those of attention_x3.hip, whose kernel it includes)"""
    return list(B.FLAGS) + list(B.PER_FILE.get(src, []))


def compile_asm(src: str = LIB_SRC, extra=()) -> str:
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = [B._hipcc()] + flags() + list(extra) + ["--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        with open(out) as f:
            return f.read()


def kernel_body(asm: str, kernel: str = KERNEL) -> list:
    """instruction and label lines of the kernel's function, in order"""
    lines = asm.splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\w*" + kernel + r"\w*:", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = []
    for ln in lines[start + 1:end]:
        s = ln.split(";")[0].strip()
        if s and not s.startswith("."):
            body.append(s)
        elif re.match(r"^\.LBB\d+_\d+:", s):
            body.append(s)
    return body


def loops(body: list) -> list:
    """[first, last] line ranges of the natural loops: a label and the last branch back to it"""
    where = {s[:-1]: i for i, s in enumerate(body) if s.endswith(":")}
    found = {}
    for i, s in enumerate(body):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)$", s)
        if m and m.group(1) in where and where[m.group(1)] < i:
            found[where[m.group(1)]] = i
    return sorted(found.items())


def loop_stats(body: list) -> list:
    out = []
    for a, b in loops(body):
        ins = [s.split()[0] for s in body[a:b + 1] if not s.endswith(":")]
        mf = [i for i, op in enumerate(ins) if op.startswith("v_mfma")]
        inner = ins[mf[0]:mf[-1] + 1] if mf else []
        out.append({
            "mfma": len(mf),
            "valu": sum(1 for op in ins if op.startswith("v_") and not op.startswith("v_mfma")),
            "packed_f32": sum(1 for op in ins if op in PACKED_F32),
            "packed_f32_between_mfma": sum(1 for op in inner if op in PACKED_F32),
            "scratch": sum(1 for op in ins if op.startswith("scratch_")),
            "instructions": len(ins),
        })
    return out


def metadata(asm: str, kernel: str = KERNEL) -> dict:
    """the kernel's entry of the amdhsa.kernels note"""
    md = {}
    blocks = re.split(r"\n\s+- \.agpr_count:", asm)
    for blk in blocks[1:]:
        if re.search(r"\.name:\s+_Z\w*" + kernel, blk):
            for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "sgpr_count"):
                m = re.search(r"\." + key + r":\s+(\d+)", blk)
                md[key] = int(m.group(1)) if m else None
            return md
    raise RuntimeError("kernel metadata not found")


def whole_kernel(body: list) -> dict:
    ins = [s.split()[0] for s in body if not s.endswith(":")]
    return {"packed_f32": sum(1 for op in ins if op in PACKED_F32), "scratch": sum(1 for op in ins if op.startswith("scratch_")),
            "mfma": sum(1 for op in ins if op.startswith("v_mfma")), "instructions": len(ins)}


if __name__ == "__main__":
    argv = sys.argv[1:]
    src = LIB_SRC
    keep = None
    if "--lab" in argv:
        argv.remove("--lab")
        src = LAB_SRC
    if "--keep" in argv:
        i = argv.index("--keep")
        keep = argv[i + 1]
        del argv[i:i + 2]
    asm = compile_asm(src, argv)
    if keep:
        with open(keep, "w") as f:
            f.write(asm)
    body = kernel_body(asm)
    print("flags:", " ".join(flags() + argv))
    for st in loop_stats(body):
        print("loop:", st)
    print("kernel:", whole_kernel(body))
    print("metadata:", metadata(asm))
