"""gemm_f32 (csrc/gemm_f32.hip) on operands whose result is exact in any accumulation order (tests/gemm_forms_util.py; the family and
the case table are checked without a GPU in tests/test_gemm_forms_reference.py): every weight mode, every tile_cfg tstar_gemm_plan
accepts, every epilogue the forward launches -- bits against an int64 sum, never a tolerance.

 * a mode's arithmetic: which term products it forms, which plane meets which, every K slice used once (a dropped a0 w2, a doubled
   a1 w1 or a skipped K = 16 step moves an integer; a change of order cannot);
 * epilogues: none, bias, bias + residual from a separate buffer, bias + residual IN PLACE (res == C, what run_encoder launches);
 * the row guard: 64 rows behind M hold a NaN pattern that must come back untouched;
 * crafted rows (ties of the first rounding, exact bfloat16 values, zeros) in every tile form, the tie rows reproduced against an
   identity block;
 * the pre-packed entries a handle uses (tstar_pack_f32x3 + tstar_gemm_f32x3_pre, tstar_gemm_bf16w_pre) against the converting ones,
   the plane made once per case;
 * QGELU / GELU on an exact pre-activation value: the same bits from every mode and kind, and the derived bounds against float64.
Observed on MI355X: profiles/gemm_forms_tests.md.
"""
import numpy as np
import pytest

import gemm_forms_util as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tstar_amd import _lib
    return _lib.load()


def _check(rc):
    from tstar_amd import _lib
    _lib.check(rc)


def _st():
    return torch.cuda.current_stream().cuda_stream


_DATA = {}


def case_data(name):
    """Operands of a case, made once: numpy, device copies, the bf16 plane (torch's round-to-nearest)."""
    if name not in _DATA:
        ops = G.make_operands(name)
        d = dict(ops=ops, dev={k: torch.from_numpy(v).cuda() for k, v in ops.items()})
        d["dev"]["W_f32"] = torch.from_numpy(G.weights_for("f32", ops["W"])).cuda()
        wb = d["dev"]["W"].to(torch.bfloat16)
        assert np.array_equal(wb.float().cpu().numpy(), G.bf16_rn(ops["W"]))
        d["dev"]["Wb"] = wb
        _DATA.clear()                                                         # one case resident at a time
        _DATA[name] = d
    return _DATA[name]


def _bits(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def new_c(M, N):
    """[M + GUARD_ROWS, N] float32 filled with the sentinel NaN."""
    return torch.full((M + G.GUARD_ROWS, N), G.SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def launch(lib, mode, dA, dW, dC, dbias, dres, M, N, K, act, cfg, pre=None):
    """The converting entry of the mode, or (pre = a plane) the pre-packed one."""
    b, r = (dbias.data_ptr() if dbias is not None else None), (dres.data_ptr() if dres is not None else None)
    if pre is None:
        return getattr(lib, G.ENTRY[mode])(dA.data_ptr(), dW.data_ptr(), dC.data_ptr(), b, r, M, N, K, act, cfg, _st())
    if mode == "f32x3":
        return lib.tstar_gemm_f32x3_pre(dA.data_ptr(), pre.data_ptr(), dC.data_ptr(), b, r, M, N, K, act, cfg, _st())
    return lib.tstar_gemm_bf16w_pre(dA.data_ptr(), pre.data_ptr(), dC.data_ptr(), b, r, M, N, K, act, 2 if mode == "bf16" else 3, cfg, _st())


def run_epilogue(lib, mode, dev, dW, M, N, K, epilogue, cfg, pre=None):
    """-> the int32 view of C's M rows; asserts the guard rows."""
    dC = new_c(M, N)
    dbias = dev["bias"] if epilogue != "none" else None
    dres = None
    if epilogue == "bias_res":
        dres = dev["res"]
    elif epilogue == "bias_res_inplace":
        dC[:M] = dev["res"]
        dres = dC
    _check(launch(lib, mode, dev["A"], dW, dC, dbias, dres, M, N, K, 0, cfg, pre))
    torch.cuda.synchronize()
    ci = dC.view(torch.int32)
    assert bool((ci[M:] == G.SENTINEL).all()), "rows behind M were written"
    return ci[:M]


def accepted_cfgs(lib, mode, M, N, wq=None):
    """(tile_cfg, kind) for what the plan accepts; what it refuses is skipped by its answer."""
    out = []
    for cfg in G.tile_cfgs(mode, M):
        plan = G.gemm_plan(lib, mode, M, N, cfg, wq)
        if plan is not None:
            out.append((cfg, plan[0]))
    return out


def pack_plane(lib, mode, dev, N, K):
    if mode == "f32x3":
        wp = torch.empty(N * K * 6, dtype=torch.uint8, device="cuda")
        _check(lib.tstar_pack_f32x3(dev["W"].data_ptr(), wp.data_ptr(), N, K, _st()))
        return wp
    return dev["Wb"] if mode in ("bf16", "bf16_exact") else None


@pytest.mark.parametrize("mode", list(G.MODES))
@pytest.mark.parametrize("name", list(G.CASES))
def test_exact_bits_in_every_form(lib, name, mode):
    """Every tile_cfg the plan accepts x every epilogue, converting and pre-packed entry: the int64 sum's bits.
    (M = 1 is the tie row alone: it pins the split, the clamped staging rows and the guard; a product missing from the six shows in the
    sixteen cases that hold family rows -- tried: profiles/gemm_forms_tests.md.)"""
    M, N, K = G.CASES[name]
    d = case_data(name)
    ops, dev = d["ops"], d["dev"]
    dW = dev["W_f32"] if mode == "f32" else dev["W"]
    plane = pack_plane(lib, mode, dev, N, K)                                  # once, as a handle does
    want = {e: _bits(G.expected(mode, ops, e)) for e in ("none", "bias", "bias_res")}
    want["bias_res_inplace"] = want["bias_res"]
    kinds = set()
    for cfg, kind in accepted_cfgs(lib, mode, M, N):
        kinds.add(kind)
        got = {}
        for e in G.EPILOGUES:
            got[e] = run_epilogue(lib, mode, dev, dW, M, N, K, e, cfg)
            bad = int((got[e] != want[e]).sum())
            assert bad == 0, f"{name} {mode} tile_cfg {cfg} (kind {kind}) {e}: {bad} of {M * N} elements differ from the exact sum"
        assert torch.equal(got["bias_res_inplace"], got["bias_res"])
    if plane is not None:
        for cfg, kind in accepted_cfgs(lib, mode, M, N, wq=0):
            for e in G.EPILOGUES:
                pre = run_epilogue(lib, mode, dev, dW, M, N, K, e, cfg, pre=plane)
                assert torch.equal(pre, want[e]), f"{name} {mode} pre-packed, tile_cfg {cfg} (kind {kind}) {e}"
    assert G.GRID_64 in kinds and (M < 128 or G.HYBRID in kinds)
    if name == G.IDENTITY_CASE and mode != "bf16":
        tie = G.rows_of(M, "tie")
        a = _bits(ops["A"][tie][:, :128])
        for cfg, _ in accepted_cfgs(lib, mode, M, N):
            c = run_epilogue(lib, mode, dev, dW, M, N, K, "none", cfg)
            assert torch.equal(c[tie][:, :128], a), f"tie rows not reassembled: {mode} tile_cfg {cfg}"


@pytest.mark.parametrize("name", list(G.CASES))
def test_activations_same_bits_in_every_form(lib, name):
    """Operands of the (0,0) pattern: the pre-activation v is one exact number in all four modes, so QGELU(v) and GELU(v) must be the
    same bits from every mode and kind; against float64, |QGELU - want| <= 2^-17 |want| and |GELU - want| <= 2^-21 |v| (derivations:
    profiles/gemm_forms_tests.md)."""
    M, N, K = G.CASES[name]
    ops = G.activation_operands(case_data(name)["ops"])
    dA, dW, dbias = (torch.from_numpy(ops[k]).cuda() for k in ("A", "W", "bias"))
    v32 = G.expected("f32", ops, "bias")
    v = v32.astype(np.float64)
    for act, ref64 in ((1, G.qgelu64), (2, G.gelu64)):
        first = None
        for mode in G.MODES:
            for cfg, kind in accepted_cfgs(lib, mode, M, N):
                dC = new_c(M, N)
                _check(launch(lib, mode, dA, dW, dC, dbias, None, M, N, K, act, cfg))
                torch.cuda.synchronize()
                ci = dC.view(torch.int32)
                assert bool((ci[M:] == G.SENTINEL).all())
                first = ci[:M].clone() if first is None else first
                assert torch.equal(ci[:M], first), f"{name} act {act}: {mode} tile_cfg {cfg} (kind {kind}) differs from f32 tile_cfg -1"
        got = first.cpu().numpy().view(np.float32).astype(np.float64)
        want = ref64(v)
        err = np.abs(got - want)
        if act == 1:
            nz = want != 0
            assert (err[~nz] == 0).all()
            worst = float((err[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
            print(f"GEMM_FORMS_ACT {name} qgelu max |err| / |want| = {worst:.3e} (bound {G.QGELU_REL:.3e}), max |v| = {np.abs(v).max():.3f}")
            assert (err <= G.QGELU_REL * np.abs(want)).all(), worst
        else:
            nz = v != 0
            assert (err[~nz] == 0).all()
            worst = float((err[nz] / np.abs(v[nz])).max()) if nz.any() else 0.0
            print(f"GEMM_FORMS_ACT {name} gelu max |err| / |v| = {worst:.3e} (bound {G.GELU_ABS_PER_V:.3e}), max |v| = {np.abs(v).max():.3f}")
            assert (err <= G.GELU_ABS_PER_V * np.abs(v)).all(), worst
