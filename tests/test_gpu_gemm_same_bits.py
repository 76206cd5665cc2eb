"""gemm_f32 against output digests recorded from the commit BEFORE a kernel change: a change that claims "same bits" must leave every
digest where it is, in every weight mode, epilogue and tile form -- the check inside one build (every tile_cfg equals the others) cannot
see a reorder that moves the bits of all tiles alike.  Cases, inputs and the recorder: tools/record_gemm_bits.py (goldens:
tests/golden/gemm_bits.json)."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_gemm_bits", os.path.join(ROOT, "tools", "record_gemm_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)["digests"]


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(rec.MODES)
    for shapes in golden.values():
        assert sorted(shapes) == sorted(rec.case_key(*s) for s in rec.SHAPES)
        for eps in shapes.values():
            assert sorted(eps) == sorted(rec.EPILOGUES)
            assert all(len(d) == 64 and int(d, 16) >= 0 for d in eps.values())
    assert len(rec.MODES) * len(rec.SHAPES) * len(rec.EPILOGUES) == 80


@pytest.mark.parametrize("mode", list(rec.MODES))
@pytest.mark.parametrize("M,N,K", rec.SHAPES)
def test_same_bits_as_recorded(golden, M, N, K, mode):
    from tstar_amd import _lib
    lib = _lib.load()
    dev = rec.device_inputs(torch, M, N, K)
    cfgs = rec.accepted_cfgs(lib, mode, M, N)
    assert -1 in cfgs and len(cfgs) >= 6
    for ep in rec.EPILOGUES:
        want = golden[mode][rec.case_key(M, N, K)][ep]
        for cfg in cfgs:
            got = rec.run_case(lib, _lib.check, torch, dev, mode, M, N, K, ep, cfg)
            assert got == want, f"output bits changed: {mode} {(M, N, K)} {ep} tile_cfg {cfg}"
