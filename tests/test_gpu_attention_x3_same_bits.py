"""attention_x3_kernel against output digests recorded from the commit BEFORE its compiled form was changed (scalar f32 VALU in the
key loop, no scratch): un-packing an add or moving a value out of scratch changes no result bit, so every digest must still match,
in both block orders.  Cases, inputs and the recorder: tools/record_attention_x3_bits.py (goldens: tests/golden/attention_x3_bits.json)."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_attention_x3_bits", os.path.join(ROOT, "tools", "record_attention_x3_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)["digests"]


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(rec.case_key(*c) for c in rec.CASES)
    for c in golden.values():
        assert sorted(c) == sorted(rec.INPUT_KINDS)
        for k in c.values():
            assert sorted(k) == sorted(str(o) for o in rec.ORDERS)


@pytest.mark.parametrize("kind", rec.INPUT_KINDS)
@pytest.mark.parametrize("B,heads,T", rec.CASES)
def test_same_bits_as_recorded(golden, B, heads, T, kind):
    from tstar_amd import _lib
    lib = _lib.load()
    for order in rec.ORDERS:
        got = rec.run_case(lib, _lib.check, torch, B, heads, T, kind, order)
        assert got == golden[rec.case_key(B, heads, T)][kind][str(order)], f"output bits changed: {(B, heads, T)} {kind} order {order}"


def test_late_max_inputs_rescale_in_the_last_tile():
    """the late_max inputs do what they are for: every query's largest score sits at the marked key of the last tile"""
    import numpy as np
    B, heads, T = 2, 2, 577
    x = rec.make_qkv(B, heads, T, "late_max").reshape(B, T, 3, heads, 64).astype(np.float64)
    s = np.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / 8.0
    assert (s.argmax(-1) == T - 2).all()
    assert (T - 2) // 32 == T // 32 - 1                                 # the last of the 18 key tiles
