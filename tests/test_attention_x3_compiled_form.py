"""What the compiler makes of attention_x3_kernel<false> (host test: cross-compiles to gfx950 assembly, no GPU).

The key loop is bound by VALU issue, and beside MFMAs a packed f32 instruction issues slower than its two scalar halves; registers
spilled to scratch cost launches their scratch set-up.  So, with build.py's own flags for attention_x3.hip: no packed f32 arithmetic
between the first and last MFMA of any loop, 96 MFMAs in the two-tile steady loop, no spill, no scratch, at most 256 registers
(two blocks per CU).  tools/lab/attn_lab, built with the same flags, must compile the same loops."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attention_x3_isa", os.path.join(ROOT, "tools", "attention_x3_isa.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


def _have_hipcc():
    return any(c and os.path.exists(c) for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"))


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="hipcc not found")


@pytest.fixture(scope="module")
def lib_asm():
    return isa.compile_asm(isa.LIB_SRC)


def test_build_applies_the_flag_to_the_library_file():
    from tstar_amd import build as B
    assert "-fno-slp-vectorize" in B.PER_FILE["attention_x3.hip"]
    assert isa.flags() == B.FLAGS + B.PER_FILE["attention_x3.hip"]


def test_key_loops_hold_no_packed_f32(lib_asm):
    stats = isa.loop_stats(isa.kernel_body(lib_asm))
    with_mfma = [s for s in stats if s["mfma"]]
    print(stats)
    assert with_mfma, "no loop with MFMAs found"
    assert with_mfma[0]["mfma"] == 96, "the steady loop covers two key tiles of 48 MFMAs"
    assert all(s["mfma"] == 96 for s in with_mfma)                      # the peeled loop: every variant of a tile once
    for s in with_mfma:
        assert s["packed_f32_between_mfma"] == 0, s
        assert s["scratch"] == 0, s
    # the steady loop is the MFMA loop with the least other work: none of the peeled form's masks and branches
    assert with_mfma[0]["valu"] == min(s["valu"] for s in with_mfma)


def test_no_spill_no_scratch_two_blocks_per_cu(lib_asm):
    md = isa.metadata(lib_asm)
    print(md, isa.whole_kernel(isa.kernel_body(lib_asm)))
    assert md["vgpr_spill_count"] == 0
    assert md["sgpr_spill_count"] == 0
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_count"] <= 256
    assert isa.whole_kernel(isa.kernel_body(lib_asm))["scratch"] == 0


def test_lab_compiles_the_same_loops(lib_asm):
    import re
    lab_asm = isa.compile_asm(isa.LAB_SRC)

    def body(asm):                                                       # block labels carry the function's number in its file
        return [re.sub(r"\.LBB\d+_", ".LBB_", s) for s in isa.kernel_body(asm)]
    assert body(lab_asm) == body(lib_asm), "the lab's kernel is not the library's, instruction for instruction"
    assert isa.metadata(lab_asm) == isa.metadata(lib_asm)
