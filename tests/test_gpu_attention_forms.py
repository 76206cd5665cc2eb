"""GPU: the three attention kernels (csrc/attention_f32.hip, attention_split.hip, attention_x3.h) on crafted operands whose answer has a
closed form (tests/attention_forms_util.py), in every form a T selects: straggler key / masked / unmasked last key tile, last query block
with idle waves / with one query / as the f32 kernel's 16-query tail workgroup, mode 1, and TSTAR_ATTN_T16=0 in one child process.

Every launch here reads its qkv from the middle of a larger allocation whose 64 rows behind the last image are NaN, and writes into the
middle of a larger buffer with 64 sentinel rows on either side: an over-read shows up as a NaN, an out-of-range write as a changed
sentinel, neither as a fault.  tests/test_attention_forms_reference.py shows that these checks cannot pass vacuously.

$TSTAR_ATTN_FORMS_REPORT, when set, names a file that gets one JSON line per (check, kernel, T): rows compared bit for bit, rows compared
by the 2^-22 bound, the graded family's largest error beside its bound."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import attention_forms_util as U

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = U.GUARD_ROWS


def _lib():
    from tstar_amd import _lib
    return _lib, _lib.load()


def _report(**row):
    print("ATTN_FORMS " + json.dumps(row))
    path = os.environ.get("TSTAR_ATTN_FORMS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _sentinel_rows(n, cols):
    return torch.full((n, cols), U.SENTINEL, dtype=torch.int32, device="cuda")


def run_kernel(kernel, qkv, B, T, heads, mode=0, key_mask=None):
    """qkv [B * T, 3 D] float32 (numpy; may hold NaN) -> out [B * T, D] float32 (numpy).  The guards described above are checked here."""
    mod, lib = _lib()
    D = heads * U.HD
    rows = B * T
    big = torch.full((G + rows + G, 3 * D), float("nan"), dtype=torch.float32, device="cuda")
    big[G:G + rows] = torch.from_numpy(np.ascontiguousarray(qkv, np.float32)).cuda()
    obuf = _sentinel_rows(G + rows + G, D)
    dq, do = big[G:G + rows], obuf[G:G + rows]
    assert dq.is_contiguous() and do.is_contiguous()
    st = torch.cuda.current_stream().cuda_stream
    if kernel == "f32":
        dkm = torch.from_numpy(np.ascontiguousarray(key_mask, np.uint8)).cuda() if mode == 1 else None
        rc = lib.tstar_attention_f32(dq.data_ptr(), do.data_ptr(), B, T, heads, mode, dkm.data_ptr() if mode == 1 else None, st)
    else:
        assert mode == 0
        rc = getattr(lib, U.ENTRY[kernel])(dq.data_ptr(), do.data_ptr(), B, T, heads, st)
    mod.check(rc, U.ENTRY[kernel])
    torch.cuda.synchronize()
    o = obuf.cpu().numpy()
    assert (o[:G] == U.SENTINEL).all(), f"{kernel} T={T}: wrote in front of the output"
    assert (o[G + rows:] == U.SENTINEL).all(), f"{kernel} T={T}: wrote behind the output"
    return o[G:G + rows].view(np.float32)


def _all_written(out, kernel, T):
    assert not (out.view(np.int32) == U.SENTINEL).any(), f"{kernel} T={T}: an output element was never written"


def indicator_case(kernel, T, B, heads, mode=0, t16=True):
    """Every round of the case's indicator launches against the closed form.  -> (bitwise rows, bounded rows)."""
    km = U.mode1_key_masks(T) if mode == 1 else None
    nbit = nbnd = 0
    for rnd in range(len(U.rounds(B, heads, mode))):
        hd = U.launch_heads("indicator", T, B, heads, rnd, mode)
        out = run_kernel(kernel, U.pack_qkv(hd, T, B, heads), B, T, heads, mode, km)
        _all_written(out, kernel, T)
        for (b, h), x in hd.items():
            exp = U.expected_indicator(x, U.valid_matrix(T, mode, km[b] if mode == 1 else None))
            a, c = U.check_indicator(U.head_rows(out, b, h, T, heads), exp, f"{kernel} T={T} mode={mode} round {rnd} image {b} head {h}")
            nbit, nbnd = nbit + a, nbnd + c
    key, query = U.forms(kernel, T, mode, t16)
    _report(check="indicator", kernel=kernel, T=T, mode=mode, t16=bool(t16), key_form=key, query_form=query, bitwise_rows=nbit, bound_rows=nbnd)
    return nbit, nbnd


def graded_case(kernel, T, B, heads, t16=True):
    hd = U.launch_heads("graded", T, B, heads)
    out = run_kernel(kernel, U.pack_qkv(hd, T, B, heads), B, T, heads)
    _all_written(out, kernel, T)
    worst, bound = 0.0, None
    for (b, h), x in hd.items():
        err, bound = U.graded_error(U.head_rows(out, b, h, T, heads), x, U.valid_matrix(T), kernel)
        worst = max(worst, err)
    key, query = U.forms(kernel, T, 0, t16)
    _report(check="graded", kernel=kernel, T=T, mode=0, t16=bool(t16), key_form=key, query_form=query, max_err=worst, bound=bound)
    assert worst <= bound, f"{kernel} T={T}: graded family off by {worst:.3e}, bound {bound:.3e}"
    return worst, bound


CASE_IDS = [f"T{T}" for T, _, _ in U.CASES]


@pytest.mark.parametrize("T,B,heads", U.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kernel", U.KERNELS)
def test_indicator_closed_form(kernel, T, B, heads):
    """Means over tied keys: bit for bit at power-of-two counts, within 2^-22 mean |V| otherwise; guards intact, nothing unwritten."""
    assert os.environ.get("TSTAR_ATTN_T16", "1") != "0", "this process must run the tail workgroup (the knob-off form has its own child)"
    nbit, nbnd = indicator_case(kernel, T, B, heads)
    assert nbit > 0 and nbit + nbnd == T * B * heads * len(U.rounds(B, heads))


@pytest.mark.parametrize("T,B,heads", U.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kernel", U.KERNELS)
def test_graded_family(kernel, T, B, heads):
    """Weights 2^(-1.44 j) with the top level late: float64 reference, the existing bounds (2e-5 / 2e-4) times max |V|."""
    graded_case(kernel, T, B, heads)


@pytest.mark.parametrize("T", U.MODE1_T)
def test_mode1_indicator(T):
    """Causal + key-padding mask over more than one key tile and query block: every prefix mean, lengths 1 .. T, a mask with holes."""
    nbit, nbnd = indicator_case("f32", T, U.MODE1_B, U.MODE1_HEADS, mode=1)
    assert nbit > 0 and nbit + nbnd == T * U.MODE1_B * U.MODE1_HEADS * len(U.rounds(U.MODE1_B, U.MODE1_HEADS, 1))


@pytest.mark.parametrize("T", U.MODE1_T)
def test_mode1_gaussian(T):
    B, heads = U.MODE1_B, U.MODE1_HEADS
    rs = np.random.RandomState(7000 + T)
    qkv = rs.standard_normal((B * T, 3 * heads * U.HD)).astype(np.float32)
    km = U.mode1_key_masks(T)
    out = run_kernel("f32", qkv, B, T, heads, 1, km)
    x = qkv.reshape(B, T, 3, heads, U.HD)
    worst = 0.0
    for b in range(B):
        valid = U.valid_matrix(T, 1, km[b])
        rows = valid.any(1)
        assert rows.all()
        for h in range(heads):
            ref = U.attention64(x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h], valid)
            got = U.head_rows(out, b, h, T, heads)
            assert np.isfinite(got[rows]).all()
            worst = max(worst, float(np.abs(got[rows] - ref[rows]).max()))
    _report(check="mode1_gaussian", kernel="f32", T=T, mode=1, max_err=worst, bound=2e-5)
    assert worst < 2e-5, worst


@pytest.mark.parametrize("T,B,heads", U.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kernel", U.KERNELS)
def test_poisoned_neighbours(kernel, T, B, heads):
    """Three images; all but one (image, head) NaN in Q, K and V, the rows behind the last image NaN as everywhere in this file.  The clean
    (image, head) comes out finite, equal to the closed form and bit-identical to the all-clean launch, at every image position and head."""
    B = 3
    hd = U.launch_heads("indicator", T, B, heads)
    clean = run_kernel(kernel, U.pack_qkv(hd, T, B, heads), B, T, heads)
    _all_written(clean, kernel, T)
    for (b, h), x in hd.items():
        qkv = np.full((B, T, 3, heads, U.HD), np.nan, np.float32)
        qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = x.Q, x.K, x.V
        out = run_kernel(kernel, qkv.reshape(B * T, -1), B, T, heads)
        got = U.head_rows(out, b, h, T, heads)
        assert np.isfinite(got).all(), f"{kernel} T={T}: image {b} head {h} picked up a neighbour's NaN"
        assert np.array_equal(got.view(np.int32), U.head_rows(clean, b, h, T, heads).view(np.int32)), (kernel, T, b, h)
        U.check_indicator(got, U.expected_indicator(x, U.valid_matrix(T)), f"{kernel} T={T} poisoned, image {b} head {h}")


def child_main():
    """The TSTAR_ATTN_T16=0 child: the f32 kernel's indicator and graded checks at T = 65 and 193 through the generic last block."""
    assert os.environ.get("TSTAR_ATTN_T16") == "0"
    for T in U.T16_OFF_T:
        assert U.forms("f32", T, t16=False)[1] == "inactive_waves"
        indicator_case("f32", T, 2, 2, t16=False)
        graded_case("f32", T, 2, 2, t16=False)
    torch.cuda.synchronize()
    print("CHILD_OK")


def test_t16_off_child():
    """TSTAR_ATTN_T16 is read once per process, so the knob-off form runs in one fresh child, started after this process's own work is
    done; nothing is started after a child that failed."""
    torch.cuda.synchronize()
    env = dict(os.environ, TSTAR_ATTN_T16="0", PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--t16-off-child"], env=env, capture_output=True, text=True, timeout=240)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    print(f"child took {time.time() - t0:.1f} s")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--t16-off-child"]
    child_main()
