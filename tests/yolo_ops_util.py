"""Crafted single-op programs for the YOLO-World layer ops (csrc/yolo.hip, csrc/yolo_conv.hip), their float64 references, the per-output error
bound and the poison rules.  Used by tests/test_yolo_ops_reference.py (no GPU), tests/test_gpu_yolo_ops.py and
tests/yolo_ops_probe.py; the programs tstar_yolo_create must refuse (REFUSED, below) by tests/test_yolo_program_host.py (no GPU)
and tests/test_gpu_errors.py.  numpy only at import time.

References
----------
Plain float64 numpy over the same NHWC buffers and channel offsets the kernels see:
  conv_ref     k = 1 / 3, stride 1 / 2, pad k // 2, bias, none / SiLU, then plain | + residual (after the activation) |
               * gate[p, ch // (cout / heads)]
  pool_ref     5 x 5 / stride 1 / -inf padded max pool, written in place at a channel offset
  upcopy_ref   dst[b, y, x, doff + c] = src[b, y // f, x // f, soff + c], f = 1 / 2
  gate_ref     sigmoid(max_n <e, guide_n> / sqrt(hc) + bias), guide = W t + b

The bound (u = 2^-24, the unit roundoff of float32)
---------------------------------------------------
Every conv kernel accumulates one output as a sequential fmaf chain over K = k * k * cin products and then adds the bias.
A chain of K fused multiply-adds has relative error factors (1 + d)^j, j <= K, on its terms (each fmaf rounds once), the
bias add one more on everything, so

    |t_hat - t| <= ((1 + u)^(K + 1) - 1) * (sum |x * w| + |bias|)  ~  (K + 1) * u * (sum |x * w| + |bias|)   =: E_pre

(first order; the second-order remainder is below (K u)^2 / 2 < 2e-9 of it for K <= 1000).  The reference evaluates
sum |x| * |w| in float64.  The bound does not depend on the order of the sum, so it also covers the direct form.

SiLU, silu(t) = t / (1 + exp(-t)): |silu'| <= 1.0999 everywhere, so the pre-activation error contributes at most 1.1 * E_pre.
The device evaluates it as v / (1.0f + __expf(-v)): the fast exponential is exp2 of v * log2(e) on the hardware's exp2 unit,
the division may be a hardware reciprocal and a multiply.  No accuracy figure for either unit is documented in the ROCm
headers or the guides at hand, so the allowance is DERIVED from 1-ulp (2 u relative) exp2 and reciprocal units plus the
argument rounding, and then doubled:
    argument y = v * log2(e): the constant and the product round (2 u relative), |dy| <= 2 u |y|, which moves exp2(y) by
        ln 2 * |dy| = 2 u |v| relative;                     exp2 unit: 2 u          -> exp:   2 u (1 + |v|)
    1 + exp: one rounding, u, and the exp error weighs at most exp / (1 + exp) < 1    -> denom: 2 u (1 + |v|) + u
    reciprocal unit 2 u, final multiply u                                                -> silu:  2 u (1 + |v|) + 4 u
 <= 6 u (1 + |v|) relative; doubled: SILU_C = 12, allowance SILU_C * u * (1 + |t|) * |silu(t)|.  Crafted pre-activations
stay within |t| <= 8 (asserted), so the argument-rounding term is at most 9 of the (1 + |t|).

Residual: one more rounding of the sum, u * |out|.  Gate multiply: the activation error scales by |gate| and the product
rounds once, u * |out|.

The gate op gets the same treatment with K = hc: E_pre = (hc + 1) * u * (max_n sum |e * g_n| / sqrt(hc) + |bias|) (the max
of perturbed values moves by at most the largest perturbation), |sigmoid'| <= 1/4, and the same exp / reciprocal allowance
SILU_C * u * (1 + |v|) * sigmoid(v).  The guide vectors the device multiplies with are themselves computed on the device
(guide_fc_kernel, a 512-term fmaf chain plus bias), so each carries dg_c <= 513 * u * (sum |W_c * t| + |b_c|), which adds
sum_c |e_c| * dg_c / sqrt(hc) to E_pre.

Pool and up-copy move values: compared bit for bit.

Poison
------
Before a run every element of every buffer of a case that the op must not read -- source channels outside
[src_off, src_off + cin), every image at index >= B -- and the whole destination hold SENTINEL, a quiet NaN with a payload.
After the run every element outside [dst_off, dst_off + cout) x the first B images must hold the bits it held before (the
sentinel, or the residual operand where that lives in the destination buffer), and no output may be NaN: the kernels mask
by select or by reading the zero quad, never by multiplying, so a NaN that is never selected cannot leak.
"""
from __future__ import annotations

import math
import os
import sys
import zlib
from typing import Dict, List, NamedTuple, Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tstar_amd import yolo_world as Y  # noqa: E402

U = 2.0 ** -24
SILU_C = 12.0
MAX_BATCH = 3
T_MAX = 8.0
SENTINEL_BITS = 0x7FC0BEEF
SENTINEL = np.array([SENTINEL_BITS], dtype=np.uint32).view(np.float32)[0]

# The policy environments: those of test_gpu_yolo.py::test_conv_kernels_bit_identical plus the wide tile.
POLICY_VARS = ("TSTAR_YOLO_SW", "TSTAR_YOLO_SW_P", "TSTAR_YOLO_SW_MIN", "TSTAR_YOLO_TM", "TSTAR_YOLO_TM_MIN", "TSTAR_YOLO_TN", "TSTAR_YOLO_HALO",
               "TSTAR_YOLO_HALO_NCH", "TSTAR_YOLO_HALO8_MAX", "TSTAR_YOLO_HALO8_MIN")
ENVS = [("tile128", {"TSTAR_YOLO_SW": "0", "TSTAR_YOLO_TM": "8", "TSTAR_YOLO_HALO": "0"}),
        ("tile64", {"TSTAR_YOLO_SW": "0", "TSTAR_YOLO_TM": "4", "TSTAR_YOLO_HALO": "0"}),
        ("sw8", {"TSTAR_YOLO_SW": "1", "TSTAR_YOLO_SW_P": "8", "TSTAR_YOLO_HALO": "0"}),
        ("sw4", {"TSTAR_YOLO_SW": "1", "TSTAR_YOLO_SW_P": "4", "TSTAR_YOLO_HALO": "0"}),
        ("halo16", {"TSTAR_YOLO_HALO": "2", "TSTAR_YOLO_HALO_NCH": "16"}),
        ("halo8", {"TSTAR_YOLO_HALO": "2", "TSTAR_YOLO_HALO_NCH": "8"}),
        ("policy", {}),
        ("wide", {"TSTAR_YOLO_SW": "0", "TSTAR_YOLO_HALO": "0", "TSTAR_YOLO_TN": "8"})]

# The form a row's family names, per environment.  Rows are small, so wherever no override forces a form the default
# policy leaves them on the 64-pixel tile; a family is eligible for the forms named in its column and for no later one
# (tile rows have cout % 16 != 0, sw rows are not 3x3 / stride-1 on a map the halo patches tile).
FORM_OF = {
    "tile":   dict(tile128="tile128", tile64="tile64", sw8="tile64", sw4="tile64", halo16="tile64", halo8="tile64", policy="tile64", wide="wide"),
    "sw":     dict(tile128="tile128", tile64="tile64", sw8="sw8", sw4="sw4", halo16="tile64", halo8="tile64", policy="tile64", wide="wide"),
    "halo_a": dict(tile128="tile128", tile64="tile64", sw8="sw8", sw4="sw4", halo16="halo_a16", halo8="halo_a8", policy="tile64", wide="wide"),
    "halo_b": dict(tile128="tile128", tile64="tile64", sw8="sw8", sw4="sw4", halo16="halo_b16", halo8="halo_b8", policy="tile64", wide="wide"),
    "direct": {name: "direct" for name, _ in ENVS},
}
ALL_FORMS = ("tile64", "tile128", "wide", "sw8", "sw4", "halo_a16", "halo_a8", "halo_b16", "halo_b8", "direct")
BIT_IDENTICAL_FAMILIES = ("tile", "sw", "halo_a", "halo_b")       # the direct form has its own accumulation order


def child_env(env: Dict[str, str]) -> Dict[str, str]:
    e = dict(os.environ, **env)
    for k in POLICY_VARS:
        if k not in env:
            e.pop(k, None)
    return e


# ------------------------------------------------------------------------------------------ conv cases
class ConvCase(NamedTuple):
    name: str
    family: str
    k: int
    s: int
    H: int
    W: int
    cin: int
    cout: int
    B: int
    src_c: int
    src_off: int
    dst_c: int
    dst_off: int
    act: int            # Y.ACT_NONE / Y.ACT_SILU
    mode: str           # "plain" | "res" (aux = dst buffer at aux_off) | "gate" (aux = its own [.., heads] buffer)
    heads: int
    aux_off: int
    same_buf: bool      # source and destination are ONE buffer of dst_c channels, disjoint channel ranges

    @property
    def Ho(self):
        return (self.H + 2 * (self.k // 2) - self.k) // self.s + 1

    @property
    def Wo(self):
        return (self.W + 2 * (self.k // 2) - self.k) // self.s + 1

    @property
    def K(self):
        return self.k * self.k * self.cin

    @property
    def M(self):
        return self.B * self.Ho * self.Wo


def _c(name, family, k, s, H, W, cin, cout, B, src=None, dst=None, act=Y.ACT_NONE, mode="plain", heads=0, aux_off=0, same_buf=False):
    src_c, src_off = src or (cin, 0)
    dst_c, dst_off = dst or (cout, 0)
    if same_buf:
        src_c = dst_c
    return ConvCase(name, family, k, s, H, W, cin, cout, B, src_c, src_off, dst_c, dst_off, act, mode, heads, aux_off, same_buf)


SILU = Y.ACT_SILU


def _conv_cases() -> List[ConvCase]:
    c: List[ConvCase] = []
    # ---- tile forms (64-pixel, 128-pixel, wide): cout % 16 != 0 keeps them off the scalar-weight forms
    c += [_c("t_map1_k1", "tile", 1, 1, 1, 1, 16, 4, 1, dst=(96, 8)),
          _c("t_map1_k3", "tile", 3, 1, 1, 1, 32, 20, 2, dst=(128, 8)),
          _c("t_map1_k3_b3", "tile", 3, 1, 1, 1, 16, 72, 3, dst=(192, 8)),
          _c("t_m63", "tile", 1, 1, 3, 7, 16, 4, 3, dst=(96, 8)),
          _c("t_m64", "tile", 1, 1, 4, 8, 32, 20, 2, dst=(128, 8)),
          _c("t_m65", "tile", 3, 1, 5, 13, 16, 72, 1, dst=(192, 8)),
          _c("t_m127", "tile", 3, 1, 1, 127, 16, 20, 1, dst=(128, 8)),
          _c("t_m128", "tile", 3, 1, 8, 8, 32, 4, 2, dst=(96, 8)),
          _c("t_m129", "tile", 1, 1, 1, 43, 32, 72, 3, dst=(192, 8)),
          _c("t_s2_7x5", "tile", 3, 2, 7, 5, 16, 20, 3, dst=(128, 8)),
          _c("t_s2_8x8", "tile", 3, 2, 8, 8, 32, 72, 2, dst=(192, 8)),
          _c("t_13x9_srcoff", "tile", 3, 1, 13, 9, 32, 20, 2, src=(80, 16), dst=(128, 8)),
          _c("t_cout132", "tile", 1, 1, 5, 5, 16, 132, 1, dst=(140, 4)),
          _c("t_silu", "tile", 3, 1, 6, 5, 16, 20, 2, dst=(128, 8), act=SILU),
          _c("t_res_silu", "tile", 3, 1, 9, 6, 16, 20, 2, dst=(96, 8), act=SILU, mode="res", aux_off=40),
          _c("t_gate4_same", "tile", 3, 1, 6, 7, 32, 20, 3, src=(64, 0), dst=(64, 36), mode="gate", heads=5, same_buf=True),
          _c("t_gate2_silu", "tile", 1, 1, 7, 6, 16, 20, 2, dst=(128, 8), act=SILU, mode="gate", heads=10)]
    # ---- scalar-weight forms (8 and 4 pixels per lane): cout % 16 == 0, never 3x3 / stride 1 on a halo-tileable map
    c += [_c("s_m1", "sw", 1, 1, 1, 1, 16, 16, 1),
          _c("s_m255", "sw", 1, 1, 5, 17, 32, 48, 3, dst=(64, 8)),
          _c("s_m256", "sw", 3, 1, 16, 16, 16, 80, 1, dst=(96, 8)),
          _c("s_m257", "sw", 3, 1, 1, 257, 16, 16, 1, dst=(32, 8)),
          _c("s_m511", "sw", 1, 1, 7, 73, 16, 80, 1, dst=(96, 12)),
          _c("s_m512", "sw", 1, 1, 16, 16, 32, 16, 2, src=(48, 8)),
          _c("s_m513", "sw", 3, 1, 9, 19, 16, 48, 3, dst=(64, 4)),
          _c("s_s2_15x11", "sw", 3, 2, 15, 11, 16, 48, 3, dst=(64, 8)),
          _c("s_s2_k1_9x7", "sw", 1, 2, 9, 7, 32, 16, 2, src=(40, 4)),
          _c("s_silu", "sw", 3, 1, 7, 9, 16, 16, 2, act=SILU),
          _c("s_res_silu", "sw", 3, 1, 11, 7, 32, 48, 2, dst=(128, 16), act=SILU, mode="res", aux_off=72),
          _c("s_gate16_silu", "sw", 1, 1, 9, 13, 16, 48, 3, dst=(64, 8), act=SILU, mode="gate", heads=3),
          _c("s_gate2", "sw", 3, 1, 5, 9, 16, 16, 2, mode="gate", heads=8),
          _c("s_same", "sw", 3, 1, 10, 6, 32, 16, 3, src=(96, 0), dst=(96, 48), same_buf=True)]
    # ---- halo forms, patch A (8 x 40, never across images)
    c += [_c("ha_8x40", "halo_a", 3, 1, 8, 40, 16, 16, 1, dst=(32, 8)),
          _c("ha_16x80", "halo_a", 3, 1, 16, 80, 48, 48, 2, src=(64, 8), dst=(64, 8)),
          _c("ha_24x120", "halo_a", 3, 1, 24, 120, 16, 96, 3, dst=(112, 8)),
          _c("ha_res_silu", "halo_a", 3, 1, 8, 40, 16, 48, 2, dst=(128, 8), act=SILU, mode="res", aux_off=64),
          _c("ha_gate16", "halo_a", 3, 1, 8, 40, 16, 96, 3, mode="gate", heads=6),
          _c("ha_same_silu", "halo_a", 3, 1, 8, 40, 48, 16, 2, src=(80, 4), dst=(80, 56), act=SILU, same_buf=True)]
    # ---- halo forms, patch B (16 x 20 over the row-stacked batch): no boundary (16 rows), one boundary per patch, a ragged last
    # patch, a ragged last patch that also holds a boundary (17 and 23 rows at B = 2, 3)
    for H, W, cin, cout in ((16, 20, 16, 16), (17, 20, 48, 48), (20, 20, 16, 96), (23, 60, 16, 48), (20, 40, 48, 16)):
        for B in (1, 2, 3):
            c.append(_c(f"hb_{H}x{W}_b{B}", "halo_b", 3, 1, H, W, cin, cout, B, src=(cin + 16, 8), dst=(cout + 16, 8)))
    c += [_c("hb_res_silu", "halo_b", 3, 1, 17, 20, 16, 16, 2, dst=(64, 4), act=SILU, mode="res", aux_off=40),
          _c("hb_gate4", "halo_b", 3, 1, 20, 20, 16, 48, 3, mode="gate", heads=12),
          _c("hb_gate2_silu", "halo_b", 3, 1, 17, 20, 16, 16, 3, act=SILU, mode="gate", heads=8)]
    # ---- direct form: cin % 16 != 0 (or input channels not 16-byte aligned); no fused modes
    c += [_c("d_stem_9x7", "direct", 3, 2, 9, 7, 3, 16, 3, dst=(96, 8)),
          _c("d_k1_cout48", "direct", 1, 1, 7, 9, 3, 48, 2),
          _c("d_cin8_cout64", "direct", 3, 1, 6, 5, 8, 64, 3, act=SILU),
          _c("d_off1_of4", "direct", 3, 1, 5, 5, 3, 16, 1, src=(4, 1)),
          _c("d_two_blocks", "direct", 3, 1, 20, 20, 3, 16, 3, dst=(32, 16)),
          _c("d_s2_cout48", "direct", 3, 2, 11, 13, 3, 48, 3, dst=(64, 12), act=SILU)]
    return c


CONV_CASES = _conv_cases()
MODE_CODE = {"plain": Y.MODE_PLAIN, "res": Y.MODE_RESIDUAL, "gate": Y.MODE_ATTN_MUL}


def check_case_table():
    """Structural rules that make FORM_OF a plain table (not a second statement of the policy)."""
    names = [c.name for c in CONV_CASES]
    assert len(set(names)) == len(names)
    for c in CONV_CASES:
        assert 1 <= c.B <= MAX_BATCH and c.cout % 4 == 0 and c.dst_off % 4 == 0 and c.dst_c % 4 == 0, c
        assert c.src_off + c.cin <= c.src_c and c.dst_off + c.cout <= c.dst_c, c
        tiled = c.cin % 16 == 0 and c.src_c % 4 == 0 and c.src_off % 4 == 0
        halo = tiled and c.cout % 16 == 0 and c.k == 3 and c.s == 1
        halo_a = halo and c.H % 8 == 0 and c.W % 40 == 0
        halo_b = halo and not halo_a and c.W % 20 == 0 and c.H >= 16
        assert (c.family == "direct") == (not tiled), c
        if c.family == "tile":
            assert c.cout % 16 != 0, c
        if c.family in ("sw", "halo_a", "halo_b"):
            assert c.cout % 16 == 0 and (c.family == "halo_a") == halo_a and (c.family == "halo_b") == halo_b, c
        if c.mode != "plain":
            assert c.family != "direct", c
        if c.mode == "gate":
            assert c.heads >= 1 and c.cout % c.heads == 0, c
        if c.mode == "res":
            assert c.aux_off % 4 == 0 and (c.aux_off + c.cout <= c.dst_off or c.aux_off >= c.dst_off + c.cout) and c.aux_off + c.cout <= c.dst_c, c
        if c.same_buf:
            assert c.s == 1 and c.src_c == c.dst_c and (c.src_off + c.cin <= c.dst_off or c.src_off >= c.dst_off + c.cout), c


def _rs(name: str, salt: int = 0) -> np.random.RandomState:
    return np.random.RandomState((zlib.crc32(name.encode()) + 7919 * salt) & 0x7FFFFFFF)


class ConvData(NamedTuple):
    w: np.ndarray                 # f32 [cout, cin, k, k]  (OIHW, as _Builder.conv(raw=...) takes it)
    b: np.ndarray                 # f32 [cout]
    src: np.ndarray               # f32 [MAX_BATCH, H, W, src_c], poisoned (None when same_buf)
    dst: np.ndarray               # f32 [MAX_BATCH, Ho, Wo, dst_c], sentinel (+ residual operand / source channels)
    aux: Optional[np.ndarray]     # f32 [MAX_BATCH, Ho, Wo, heads] for the gate


def sentinel_array(shape) -> np.ndarray:
    a = np.empty(shape, np.float32)
    a.view(np.uint32)[...] = SENTINEL_BITS
    return a


def conv_data(c: ConvCase) -> ConvData:
    rs = _rs(c.name)
    w = (rs.uniform(-1.0, 1.0, (c.cout, c.cin, c.k, c.k)) * (2.0 / math.sqrt(c.K))).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, c.cout).astype(np.float32)
    x = rs.uniform(-1.0, 1.0, (c.B, c.H, c.W, c.cin)).astype(np.float32)
    dst = sentinel_array((MAX_BATCH, c.Ho, c.Wo, c.dst_c))
    if c.same_buf:
        src = None
        dst[:c.B, :, :, c.src_off:c.src_off + c.cin] = x
    else:
        src = sentinel_array((MAX_BATCH, c.H, c.W, c.src_c))
        src[:c.B, :, :, c.src_off:c.src_off + c.cin] = x
    aux = None
    if c.mode == "res":
        dst[:c.B, :, :, c.aux_off:c.aux_off + c.cout] = rs.uniform(-1.0, 1.0, (c.B, c.Ho, c.Wo, c.cout)).astype(np.float32)
    elif c.mode == "gate":
        aux = sentinel_array((MAX_BATCH, c.Ho, c.Wo, c.heads))
        aux[:c.B] = rs.uniform(0.1, 1.0, (c.B, c.Ho, c.Wo, c.heads)).astype(np.float32)
    return ConvData(w, b, src, dst, aux)


def case_inputs(c: ConvCase, d: ConvData):
    """(x [B,H,W,cin], residual [B,Ho,Wo,cout] or None, gate [B,Ho,Wo,heads] or None) as float32 views of the buffers."""
    buf = d.dst if c.same_buf else d.src
    x = buf[:c.B, :, :, c.src_off:c.src_off + c.cin]
    r = d.dst[:c.B, :, :, c.aux_off:c.aux_off + c.cout] if c.mode == "res" else None
    g = d.aux[:c.B] if c.mode == "gate" else None
    return x, r, g


def _im2col(x: np.ndarray, k: int, s: int) -> np.ndarray:
    """[B,H,W,C] -> [B,Ho,Wo,k,k,C] with zero padding k // 2."""
    B, H, W, Cc = x.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((B, H + 2 * p, W + 2 * p, Cc), x.dtype)
    xp[:, p:p + H, p:p + W] = x
    out = np.empty((B, Ho, Wo, k, k, Cc), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out[:, :, :, ky, kx] = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
    return out


def silu(t):
    return t / (1.0 + np.exp(-t))


def conv_ref(x, w, b, k, s, act, residual=None, gate=None, dtype=np.float64, res_before_act=False, gate_head=None):
    """x [B,H,W,cin], w [cout,cin,k,k], b [cout] or None -> (out [B,Ho,Wo,cout], bound, pre-activation t), all in ``dtype``
    arithmetic (float64: the reference; float32: the CPU stand-in of test (b)).  ``res_before_act`` and ``gate_head`` (a map
    channel -> head) build the mutants of the sensitivity test."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    cout, cin = w.shape[:2]
    cols = _im2col(x, k, s)
    Bn, Ho, Wo = cols.shape[:3]
    A = cols.reshape(Bn * Ho * Wo, k * k * cin)
    Wm = w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout)
    bias = np.zeros(cout, dtype) if b is None else np.asarray(b, dtype)
    t = A @ Wm + bias
    mag = np.abs(A).astype(np.float64) @ np.abs(Wm).astype(np.float64) + np.abs(bias).astype(np.float64)
    bound = (k * k * cin + 1) * U * mag
    t = t.reshape(Bn, Ho, Wo, cout)
    bound = bound.reshape(Bn, Ho, Wo, cout)
    if residual is not None and res_before_act:
        t = t + np.asarray(residual, dtype)
    v = t
    if act == Y.ACT_SILU:
        v = silu(t)
        bound = 1.1 * bound + SILU_C * U * (1.0 + np.abs(t)) * np.abs(v)
    if residual is not None and not res_before_act:
        v = v + np.asarray(residual, dtype)
        bound = bound + U * np.abs(v)
    if gate is not None:
        g = np.asarray(gate, dtype)
        heads = g.shape[-1]
        head = (np.arange(cout) // (cout // heads)) if gate_head is None else np.asarray(gate_head)
        gg = g[..., head]
        v = v * gg
        bound = bound * np.abs(gg) + U * np.abs(v)
    return v, np.asarray(bound, np.float64), t


def case_reference(c: ConvCase, d: ConvData, dtype=np.float64, **mut):
    x, r, g = case_inputs(c, d)
    return conv_ref(x, d.w, d.b, c.k, c.s, c.act, r, g, dtype, **mut)


def conv_mutants(c: ConvCase, d: ConvData):
    """name -> output of a subtly wrong conv (float64).  Each must stand out of the bound by a factor of 10 somewhere."""
    x, r, g = case_inputs(c, d)
    out = {}
    w = d.w.copy()
    w[:, :, c.k // 2, c.k // 2] = 0                                   # the centre tap: the one every map size reads
    out["tap_zeroed"] = conv_ref(x, w, d.b, c.k, c.s, c.act, r, g)[0]
    w = d.w.copy()
    w[:, -1] = 0
    out["last_cin_dropped"] = conv_ref(x, w, d.b, c.k, c.s, c.act, r, g)[0]
    w = d.w.copy()
    flat = w[-1].transpose(1, 2, 0).reshape(-1)                       # (ky, kx, ci): the kernels' k order
    w[-1] = np.roll(flat, 1).reshape(c.k, c.k, c.cin).transpose(2, 0, 1)
    out["last_cout_shifted"] = conv_ref(x, w, d.b, c.k, c.s, c.act, r, g)[0]
    if c.mode == "gate":
        cph = c.cout // c.heads
        if c.heads > 1:
            out["gate_next_head"] = conv_ref(x, d.w, d.b, c.k, c.s, c.act, r, g, gate_head=(np.arange(c.cout) // cph + 1) % c.heads)[0]
        if cph < 4:
            out["gate_head_of_quad"] = conv_ref(x, d.w, d.b, c.k, c.s, c.act, r, g, gate_head=(np.arange(c.cout) // 4 * 4) // cph)[0]
    if c.mode == "res" and c.act == Y.ACT_SILU:
        out["residual_before_act"] = conv_ref(x, d.w, d.b, c.k, c.s, c.act, r, g, res_before_act=True)[0]
    if c.act == Y.ACT_SILU:
        out["no_activation"] = conv_ref(x, d.w, d.b, c.k, c.s, Y.ACT_NONE, r, g)[0]
    return out


# ------------------------------------------------------------------------------------------ programs
def _new_builder():
    b = Y._Builder({})
    x = b.buf(Y.IMG_SIZE, Y.IMG_SIZE, 3)                               # tstar_yolo_create wants the 640 x 640 x 3 input ...
    e, r = b.buf(4, 4, Y.TEXT_DIM), b.buf(4, 4, 4 * Y.REG_MAX)         # ... and one head level; no op writes these
    levels = [[e, r, 4, 8, b.put([1.0, 0.0]), 0, 0, 0]]
    return b, levels, x


def conv_program(cases: List[ConvCase]):
    """One program holding one conv op per case, each on buffers of its own.  -> (program dict, per case dict(op, src, dst, aux))."""
    b, levels, x = _new_builder()
    where = []
    for c in cases:
        d = conv_data(c)
        dst = b.buf(c.Ho, c.Wo, c.dst_c)
        src = dst if c.same_buf else b.buf(c.H, c.W, c.src_c)
        aux = dst if c.mode == "res" else b.buf(c.Ho, c.Wo, c.heads) if c.mode == "gate" else -1
        b.conv(None, src, c.src_off, dst, c.dst_off, stride=c.s, act=c.act, mode=MODE_CODE[c.mode], aux=aux, aux_off=c.aux_off if c.mode == "res" else 0,
               raw=(d.w, d.b))
        where.append(dict(op=len(b.ops) - 1, src=src, dst=dst, aux=aux))
    return Y.program_from_builder(b, levels, x), where


def plan_of_case(c: ConvCase, env_policy: bool):
    from tstar_amd.yolo import conv_plan
    return conv_plan(c.cin, c.src_c, c.src_off, c.H, c.W, c.cout, c.dst_c, c.dst_off, c.k, c.s, MODE_CODE[c.mode], c.B, MAX_BATCH, env_policy)


def check_conv_output(c: ConvCase, d: ConvData, got: np.ndarray):
    """got: the destination buffer after the run, f32 [MAX_BATCH, Ho, Wo, dst_c].  Asserts the poison rules; returns the largest
    error / bound ratio against the float64 reference."""
    ref, bound, t = case_reference(c, d)
    assert np.abs(t).max() <= T_MAX, (c.name, np.abs(t).max())
    out = got[:c.B, :, :, c.dst_off:c.dst_off + c.cout]
    assert not np.isnan(out).any(), f"{c.name}: NaN in the output (poison leaked, or an output was never written)"
    keep = np.ones(got.shape, bool)
    keep[:c.B, :, :, c.dst_off:c.dst_off + c.cout] = False
    same = got.view(np.uint32) == d.dst.view(np.uint32)
    assert same[keep].all(), f"{c.name}: {int((~same[keep]).sum())} elements outside the output range were overwritten"
    ratio = np.abs(out.astype(np.float64) - ref) / bound
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ pool / up-copy
class PoolCase(NamedTuple):
    name: str
    H: int
    W: int
    C: int
    ld: int
    soff: int
    doff: int


POOL_CASES = [PoolCase("p_1x1", 1, 1, 4, 12, 4, 8), PoolCase("p_3x3", 3, 3, 36, 80, 0, 40), PoolCase("p_5x4", 5, 4, 4, 16, 8, 0),
              PoolCase("p_20x20", 20, 20, 36, 76, 4, 40), PoolCase("p_5x4_c36", 5, 4, 36, 72, 36, 0)]


class UpCase(NamedTuple):
    name: str
    Hs: int
    Ws: int
    C: int
    f: int
    sld: int
    soff: int
    dld: int
    doff: int


UP_CASES = [UpCase("u_f1_3x5", 3, 5, 8, 1, 16, 4, 24, 12), UpCase("u_f2_3x5", 3, 5, 12, 2, 20, 8, 16, 4), UpCase("u_f2_1x1", 1, 1, 4, 2, 4, 0, 8, 4),
            UpCase("u_f2_7x9", 7, 9, 36, 2, 40, 4, 44, 8), UpCase("u_f1_1x7", 1, 7, 4, 1, 8, 4, 4, 0)]


def pool_ref(buf: np.ndarray, soff: int, doff: int, C: int) -> np.ndarray:
    """buf f32 [B,H,W,ld] -> the buffer after the in-place 5x5 / stride 1 / -inf padded max pool of channels [soff, soff + C) into
    [doff, doff + C).  Exact (max moves values)."""
    B, H, W, _ = buf.shape
    x = buf[..., soff:soff + C]
    xp = np.full((B, H + 4, W + 4, C), -np.inf, buf.dtype)
    xp[:, 2:2 + H, 2:2 + W] = x
    m = np.full((B, H, W, C), -np.inf, buf.dtype)
    for dy in range(5):
        for dx in range(5):
            m = np.maximum(m, xp[:, dy:dy + H, dx:dx + W])
    out = buf.copy()
    out[..., doff:doff + C] = m
    return out


def upcopy_ref(src: np.ndarray, soff: int, C: int, f: int) -> np.ndarray:
    """src [B,Hs,Ws,sld] -> [B,Hs*f,Ws*f,C]: dst[b,y,x,c] = src[b,y//f,x//f,soff+c]."""
    B, Hs, Ws, _ = src.shape
    yy, xx = np.arange(Hs * f) // f, np.arange(Ws * f) // f
    return src[:, yy][:, :, xx][..., soff:soff + C]


def pool_data(c: PoolCase, B: int) -> np.ndarray:
    buf = sentinel_array((MAX_BATCH, c.H, c.W, c.ld))
    buf[:B, :, :, c.soff:c.soff + c.C] = _rs(c.name).standard_normal((B, c.H, c.W, c.C)).astype(np.float32)
    return buf


def up_data(c: UpCase, B: int):
    src = sentinel_array((MAX_BATCH, c.Hs, c.Ws, c.sld))
    src[:B, :, :, c.soff:c.soff + c.C] = _rs(c.name).standard_normal((B, c.Hs, c.Ws, c.C)).astype(np.float32)
    return src, sentinel_array((MAX_BATCH, c.Hs * c.f, c.Ws * c.f, c.dld))


def move_program():
    """One program with every pool and up-copy case.  -> (program, pool buffer ids, (src, dst) ids of the up-copies)."""
    b, levels, x = _new_builder()
    pools, ups = [], []
    for c in POOL_CASES:
        buf = b.buf(c.H, c.W, c.ld)
        b.pool5(buf, c.soff, c.C, c.doff)
        pools.append(buf)
    for c in UP_CASES:
        s, d = b.buf(c.Hs, c.Ws, c.sld), b.buf(c.Hs * c.f, c.Ws * c.f, c.dld)
        b.upcopy(s, c.soff, c.C, d, c.doff, c.f)
        ups.append((s, d))
    return Y.program_from_builder(b, levels, x), pools, ups


# ------------------------------------------------------------------------------------------ gate op
class GateCase(NamedTuple):
    name: str
    H: int
    W: int
    heads: int
    hc: int
    ld: int
    off: int


# HW * heads around one 256-thread block: 5 x 17 x 3 = 255, 2 x 43 x 3 = 258, 4 x 8 x 8 = 256, 3 x 11 x 8 = 264, 16 x 16 x 1 = 256
GATE_CASES = [GateCase("g_hc32_h1", 16, 16, 1, 32, 40, 8), GateCase("g_hc32_h3_255", 5, 17, 3, 32, 96, 0), GateCase("g_hc32_h3_258", 2, 43, 3, 32, 100, 4),
              GateCase("g_hc32_h8_256", 4, 8, 8, 32, 256, 0), GateCase("g_hc32_h8_264", 3, 11, 8, 32, 260, 4),
              GateCase("g_hc32_unaligned", 3, 5, 3, 32, 99, 2),          # the scalar branch through the alignment test
              GateCase("g_hc8_h1", 7, 9, 1, 8, 12, 4), GateCase("g_hc8_h3", 5, 17, 3, 8, 24, 0), GateCase("g_hc8_h8", 3, 11, 8, 8, 68, 4),
              GateCase("g_hc20_h1", 1, 1, 1, 20, 20, 0), GateCase("g_hc20_h3", 2, 43, 3, 20, 64, 3), GateCase("g_hc20_h8", 4, 8, 8, 20, 160, 0)]
GATE_SETS = {0: 5, 1: 32, 2: 1}                                        # query set -> Q
GATE_RUNS = [(3, [0, 1, 2]), (3, [1, 0, 0]), (2, [2, 1]), (1, [1]), (2, None)]   # (B, per-image sets; None = set 0 for all)


def gate_text(q_set: int) -> np.ndarray:
    t = _rs("gate_text", q_set).standard_normal((GATE_SETS[q_set], Y.TEXT_DIM))
    return (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)


class GateData(NamedTuple):
    W: np.ndarray        # f32 [embed, 512]
    b: np.ndarray        # f32 [embed]
    bias: np.ndarray     # f32 [heads]
    emb: np.ndarray      # f32 [MAX_BATCH, H, W, ld], channels outside [off, off + embed) poisoned


def gate_data(c: GateCase) -> GateData:
    rs = _rs(c.name)
    embed = c.heads * c.hc
    emb = sentinel_array((MAX_BATCH, c.H, c.W, c.ld))
    emb[..., c.off:c.off + embed] = rs.uniform(-1.0, 1.0, (MAX_BATCH, c.H, c.W, embed)).astype(np.float32)
    return GateData(rs.standard_normal((embed, Y.TEXT_DIM)).astype(np.float32), (0.1 * rs.standard_normal(embed)).astype(np.float32),
                    (0.3 * rs.standard_normal(c.heads)).astype(np.float32), emb)


def gate_ref(e, text, Wg, bg, bias, heads, dtype=np.float64):
    """e [P, embed] (one image's pixels), text [Q, 512] -> (gate [P, heads], bound [P, heads], pre-sigmoid v)."""
    e, text, Wg, bg, bias = (np.asarray(a, dtype) for a in (e, text, Wg, bg, bias))
    P, embed = e.shape
    hc = embed // heads
    guide = text @ Wg.T + bg                                                           # [Q, embed]
    dguide = (Y.TEXT_DIM + 1) * U * (np.abs(text).astype(np.float64) @ np.abs(Wg.T).astype(np.float64) + np.abs(bg))
    eh = e.reshape(P, heads, hc)
    gh = guide.reshape(-1, heads, hc)
    d = np.einsum("pmc,nmc->pnm", eh, gh)
    ea = np.abs(eh).astype(np.float64)
    mag = np.einsum("pmc,nmc->pnm", ea, np.abs(gh).astype(np.float64)).max(axis=1)
    carried = np.einsum("pmc,nmc->pnm", ea, dguide.reshape(-1, heads, hc)).max(axis=1)
    inv = dtype(1.0) / np.sqrt(dtype(hc))
    v = d.max(axis=1) * inv + bias
    s = 1.0 / (1.0 + np.exp(-v))
    pre = (hc + 1) * U * (mag / math.sqrt(hc) + np.abs(bias).astype(np.float64)) + carried / math.sqrt(hc)
    bound = 0.25 * pre + SILU_C * U * (1.0 + np.abs(v)) * s
    return s, np.asarray(bound, np.float64), v


def gate_program():
    b, levels, x = _new_builder()
    where = []
    for c in GATE_CASES:
        d = gate_data(c)
        embed = c.heads * c.hc
        src, dst = b.buf(c.H, c.W, c.ld), b.buf(c.H, c.W, c.heads)
        gid = len(b.guides)
        b.guides.append(dict(embed=embed, heads=c.heads, w_off=b.put(d.W), b_off=b.put(d.b), bias_off=b.put(d.bias)))
        b.attn(src, c.off, embed, dst, c.heads, gid)
        where.append((src, dst))
    return Y.program_from_builder(b, levels, x), where


# ------------------------------------------------------------------------------------------ programs the checker refuses
def crafted_program(mutate=None):
    """Ops 0 / 1 / 2: a residual conv, a gated conv (20 channels, 10 heads), a direct-form conv (cin = 3, cout = 16), with
    ``mutate(ops, bufs)`` applied to copies of the raw tables."""
    prog, _ = conv_program([c for c in CONV_CASES if c.name in ("t_res_silu", "t_gate2_silu", "d_stem_9x7")])
    prog = dict(prog, ops=prog["ops"].copy(), bufs=prog["bufs"].copy())
    if mutate:
        mutate(prog["ops"], prog["bufs"])
    return prog


def _mutated(prog, op_words=(), buf_words=()):
    """``prog`` with ops[i, word] = value for every (i, word, value) and bufs[ops[i, which], word] += delta for every
    (i, which, word, delta)."""
    ops, bufs = prog["ops"].copy(), prog["bufs"].copy()
    for i, word, value in op_words:
        ops[i, word] = value
    for i, which, word, delta in buf_words:
        bufs[ops[i, which], word] += delta
    return dict(prog, ops=ops, bufs=bufs)


def _lds_72k_program():
    """The direct form's 64 KB of weights: cin = 8, k = 3, cout = 256 is 72 KB."""
    b, levels, x = _new_builder()
    s, d = b.buf(4, 4, 8), b.buf(4, 4, 256)
    b.conv(None, s, 0, d, 0, act=Y.ACT_NONE, raw=(np.zeros((256, 8, 3, 3), np.float32), None))
    return Y.program_from_builder(b, levels, x)


def refused_programs():
    """[(name, program, regex the error must match)]: shapes that used to fail at the first forward (in the launcher) or not at
    all.  The regexes are those tests/test_gpu_errors.py has always asserted."""
    crafted = crafted_program()
    rows = []

    def conv_row(name, op, msg, op_words=(), buf_words=()):
        rows.append((name, _mutated(crafted, op_words, buf_words), f"malformed op {op}.*{msg}"))

    conv_row("cout_6", 0, "multiples of 4", [(0, Y.W_COUT, 6)])                                        # cout % 4
    conv_row("dst_off_2", 0, "multiples of 4", [(0, Y.W_DST_OFF, 2)])                                  # dst_off % 4
    conv_row("mode_3", 0, "unknown conv mode", [(0, Y.W_MODE, 3)])
    conv_row("res_off_2", 0, "residual channels", [(0, Y.W_AUX_OFF, 42)])                              # residual offset % 4
    conv_row("res_past_end", 0, "residual channels", [(0, Y.W_AUX_OFF, 80)])                           # 80 + 20 > 96
    conv_row("gate_heads", 1, "divide evenly among the heads", buf_words=[(1, Y.W_AUX, Y.BUF_C, -2)]) # 20 channels over 8 heads
    conv_row("gate_off", 1, "divide evenly among the heads", [(1, Y.W_AUX_OFF, 4)])
    conv_row("gate_map", 1, "output's map size", buf_words=[(1, Y.W_AUX, Y.BUF_H, 1)])                # gate buffer of another map size
    conv_row("direct_res", 2, "no fused residual",
             [(2, Y.W_MODE, Y.MODE_RESIDUAL), (2, Y.W_AUX, int(crafted["ops"][2, Y.W_DST])), (2, Y.W_AUX_OFF, 32)])
    conv_row("direct_cout", 2, "cout % 16 == 0", [(2, Y.W_COUT, 12)])      # direct form needs cout % 16 (12 keeps the blob ranges valid)
    rows.append(("direct_72k", _lds_72k_program(), "malformed op 0.*64 KB of LDS"))
    # attention op: embed / heads must be the guide's, the gate buffer the source's map
    gprog, _ = gate_program()
    rows.append(("attn_embed", _mutated(gprog, [(0, Y.W_EMBED, 16)]), "differ from the op's attention layer"))
    rows.append(("attn_heads", _mutated(gprog, [(0, Y.W_HEADS, 2)]), "malformed op 0"))
    rows.append(("attn_map", _mutated(gprog, buf_words=[(0, Y.W_DST, Y.BUF_W, 1)]), "gate buffer must have the source's map size"))
    # pool / up-copy of no channels
    mprog, _, _ = move_program()
    for i in (0, len(POOL_CASES)):
        rows.append((f"move_{i}_no_channels", _mutated(mprog, [(i, Y.W_C, 0)]), f"malformed op {i}"))
    return rows
