"""CPU: the YOLO-World layer program's checker (csrc/yolo_program.h) through tstar_yolo_check_program -- every check
tstar_yolo_create makes of its arguments, without a GPU -- the promise that what the checker accepts the conv planner serves, and
the stand-alone sanitizer program over extreme words."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yolo_ops_util as OU  # noqa: E402
from tstar_amd import yolo_world as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = ("s", "m", "l", "x", "xl")


@pytest.fixture(scope="module")
def accepted():
    """name -> program: the built programs of the five scales (seeded weights) and the crafted programs of yolo_ops_util."""
    progs = {f"scale_{s}": Y.build_program(Y.synthetic_state_dict(0, s), s) for s in SCALES}
    progs["conv"] = OU.conv_program(OU.CONV_CASES)[0]
    progs["gate"] = OU.gate_program()[0]
    progs["move"] = OU.move_program()[0]
    progs["crafted"] = OU.crafted_program()
    return progs


def test_built_and_crafted_programs_are_accepted(accepted):
    from tstar_amd.yolo import check_program
    for name, prog in accepted.items():
        for max_batch in (1, OU.MAX_BATCH, 76, 1024):
            check_program(prog, max_batch)


def test_refused_programs():
    """Every row of the shared table is refused with the message tstar_yolo_create gives on the GPU machines."""
    from tstar_amd import _lib
    from tstar_amd.yolo import check_program
    rows = OU.refused_programs()
    assert len(rows) == 16 and len({name for name, _, _ in rows}) == 16
    for name, prog, msg in rows:
        with pytest.raises(_lib.TStarHipError, match=msg):
            check_program(prog, 1)


def test_shape_of_the_call_and_oversized_buffers():
    from tstar_amd import _lib
    from tstar_amd.yolo import check_program
    prog = OU.crafted_program()
    for bad in (0, 1025, -1):
        with pytest.raises(_lib.TStarHipError, match="max_batch must be in 1..1024"):
            check_program(prog, bad)
    with pytest.raises(_lib.TStarHipError, match="bad input buffer"):
        check_program(dict(prog, input_buf=len(prog["bufs"])), 1)
    with pytest.raises(_lib.TStarHipError, match="must be 640 x 640 x 3"):
        check_program(dict(prog, input_buf=1), 1)
    with pytest.raises(_lib.TStarHipError, match="bad program shape"):
        check_program(dict(prog, ops=prog["ops"][:, :23]), 1)
    with pytest.raises(_lib.TStarHipError, match="bad buffer shape"):
        check_program(OU.crafted_program(lambda ops, bufs: bufs.__setitem__((3, Y.BUF_W), 0)), 1)
    # max_batch * H * W is the kernels' int pixel count: 2^31 - 1 pixels pass, 2^31 do not.  Buffer 3 is the first conv's output
    # (9 x 6): its map no longer matches, so with a legal size the refusal moves on to the op
    big = np.iinfo(np.int32).max

    def sized(H, W):
        return OU.crafted_program(lambda ops, bufs: bufs.__setitem__((3, slice(0, 2)), (H, W)))
    with pytest.raises(_lib.TStarHipError, match="malformed op 0"):
        check_program(sized(big, 1), 1)
    with pytest.raises(_lib.TStarHipError, match="buffer too large for the kernels' 32-bit pixel index"):
        check_program(sized(big, 2), 1)
    with pytest.raises(_lib.TStarHipError, match="buffer too large for the kernels' 32-bit pixel index"):
        check_program(sized(big, big), 1)
    with pytest.raises(_lib.TStarHipError, match="buffer too large for the kernels' 32-bit pixel index"):
        check_program(sized(1 << 11, 1 << 10), 1024)                # 2^31 exactly
    with pytest.raises(_lib.TStarHipError, match="malformed op 0"):
        check_program(sized((1 << 11) - 1, 1 << 10), 1024)
    # the input buffer itself: 1024 x 640 x 640 < 2^31
    check_program(prog, 1024)


def test_every_accepted_conv_op_has_a_plan(accepted):
    """Checker within planner: what tstar_yolo_create accepts, launch_conv serves at the first forward -- for every conv op of every
    accepted program, at B = 1 and B = max_batch, for max_batch 1, 76 and 1024 (1024 puts the zero quad of the large maps beyond
    the scalar-weight forms' 32-bit offsets), under the default policy."""
    import ctypes as C
    from tstar_amd import _lib
    lib = _lib.load()
    out = (C.c_int * 3)()
    seen = set()
    for name, prog in accepted.items():
        ops, bufs = prog["ops"], prog["bufs"]
        for o in ops[ops[:, Y.W_KIND] == Y.OP_CONV]:
            src, dst = bufs[o[Y.W_SRC]], bufs[o[Y.W_DST]]
            seen.add(tuple(int(v) for v in (o[Y.W_CIN], src[Y.BUF_C], o[Y.W_SRC_OFF], src[Y.BUF_H], src[Y.BUF_W], o[Y.W_COUT], dst[Y.BUF_C],
                                            o[Y.W_DST_OFF], o[Y.W_KS], o[Y.W_STRIDE], o[Y.W_MODE])))
    assert len(seen) > 300
    n = 0
    for op in sorted(seen):
        for max_batch in (1, 76, 1024):
            for B in {1, max_batch}:
                rc = lib.tstar_yolo_conv_plan(*op, B, max_batch, 0, out)
                assert rc == 0 and out[1] >= 1 and out[2] >= 1, (op, B, max_batch, lib.tstar_last_error())
                n += 1
    assert n == len(seen) * 5


def small_program():
    """One op of every kind on small buffers: a residual conv, a direct-form conv, an attention op with its gated conv, a pool and an
    up-copy.  -> (program, n_anchor, number of ops)."""
    b, levels, x = OU._new_builder()
    rs = np.random.RandomState(5)
    cat, tmp = b.buf(6, 5, 48), b.buf(6, 5, 16)
    b.conv(None, cat, 0, tmp, 0, raw=(rs.standard_normal((16, 16, 3, 3)), rs.standard_normal(16)))
    b.conv(None, tmp, 0, cat, 16, mode=Y.MODE_RESIDUAL, aux=cat, aux_off=0, raw=(rs.standard_normal((16, 16, 1, 1)), None))
    rgb, stem = b.buf(12, 10, 3), b.buf(6, 5, 16)
    b.conv(None, rgb, 0, stem, 0, stride=2, raw=(rs.standard_normal((16, 3, 3, 3)), rs.standard_normal(16)))
    gate = b.buf(6, 5, 2)
    b.guides.append(dict(embed=16, heads=2, w_off=b.put(rs.standard_normal((16, Y.TEXT_DIM))), b_off=b.put(np.zeros(16)), bias_off=b.put(np.zeros(2))))
    b.attn(cat, 16, 16, gate, 2, 0)
    b.conv(None, cat, 0, cat, 32, act=Y.ACT_NONE, mode=Y.MODE_ATTN_MUL, aux=gate, raw=(rs.standard_normal((16, 16, 3, 3)), None))
    b.pool5(cat, 0, 16, 16)
    up = b.buf(12, 10, 16)
    b.upcopy(stem, 0, 16, up, 0, 2)
    return Y.program_from_builder(b, levels, x), 16, len(b.ops)


def test_program_sanitizer_program(tmp_path):
    """csrc/yolo_program_check_main.cpp, built with -fsanitize=address,undefined (a stand-alone CPU program; nothing is loaded into
    python, nothing of the GPU is involved): INT_MIN, -1, 0 and INT_MAX in every word of every op, buffer, attention-layer and level
    row of a small valid program, one at a time, and the blob cut to every prefix length, on exact-size heap blocks.  Every call
    returns a program or a message, and the sanitizers report nothing."""
    from tstar_amd.yolo import check_program
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    prog, n_anchor, n_ops = small_program()
    check_program(prog, 2)
    path = str(tmp_path / "program.bin")
    tables = [np.ascontiguousarray(prog[k], dtype=np.int32) for k in ("ops", "bufs", "guides", "levels")]
    blob = np.ascontiguousarray(prog["blob"], dtype=np.float32)
    with open(path, "wb") as f:
        np.array([blob.size] + [len(t) for t in tables] + [prog["input_buf"], 2, n_anchor, n_ops], dtype=np.int32).tofile(f)
        for t in tables:
            t.tofile(f)
        blob.tofile(f)
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "yolo_program_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           os.path.join(csrc, "yolo_program_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    words = sum(t.size for t in tables)
    f = dict(kv.split("=") for kv in r.stdout.split())
    assert int(f["ops"]) == n_ops and int(f["n_anchor"]) == n_anchor and int(f["differ"]) == 0, r.stdout
    assert int(f["need"]) == blob.size and int(f["cuts"]) == blob.size + 1, r.stdout
    assert int(f["decoded"]) + int(f["refused"]) == 4 * words + 8 + blob.size + 1, r.stdout
    # every cut prefix is a refusal; the whole blob and any value in the 9 unused words of an op decode
    assert int(f["refused"]) >= blob.size and int(f["decoded"]) >= 1 + 4 * (Y.OP_WORDS - 15) * n_ops, r.stdout
