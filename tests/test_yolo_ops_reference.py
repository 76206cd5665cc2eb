"""CPU: the float64 references, the error bound and the case table of the YOLO layer-op tests (tests/yolo_ops_util.py)
checked without a GPU: (a) each reference against an independent torch statement, (b) a float32 CPU evaluation stays inside the
bound, (c) the cases tell subtly wrong kernels apart, (d) the policy puts every case on the form its row names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_ops_util as OU
from tstar_amd import yolo_world as Y

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [c.name for c in OU.CONV_CASES]


def test_case_table_is_well_formed():
    OU.check_case_table()
    fams = {c.family for c in OU.CONV_CASES}
    assert fams == set(OU.FORM_OF)
    for fam in ("tile", "sw", "halo_a", "halo_b"):          # every fused mode on every family that has them
        modes = {(c.mode, c.act) for c in OU.CONV_CASES if c.family == fam}
        assert {m for m, _ in modes} == {"plain", "res", "gate"} and ("res", Y.ACT_SILU) in modes, fam
    cph = {c.cout // c.heads for c in OU.CONV_CASES if c.mode == "gate"}
    assert {16, 4, 2} <= cph
    assert {c.B for c in OU.CONV_CASES} == {1, 2, 3}


# ------------------------------------------------------------------------------------------ (a) references vs torch
@pytest.mark.parametrize("case", OU.CONV_CASES, ids=IDS)
def test_conv_reference_equals_torch(case):
    d = OU.conv_data(case)
    x, r, g = OU.case_inputs(case, d)
    ref, bound, t = OU.case_reference(case, d)
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    y = F.conv2d(xt, torch.from_numpy(d.w).double(), torch.from_numpy(d.b).double(), stride=case.s, padding=case.k // 2)
    if case.act == Y.ACT_SILU:
        y = F.silu(y)
    if r is not None:
        y = y + torch.from_numpy(np.ascontiguousarray(r)).double().permute(0, 3, 1, 2)
    if g is not None:
        gt = torch.from_numpy(np.ascontiguousarray(g)).double().permute(0, 3, 1, 2)
        y = y * gt.repeat_interleave(case.cout // case.heads, dim=1)
    y = y.permute(0, 2, 3, 1).numpy()
    assert y.shape == ref.shape == (case.B, case.Ho, case.Wo, case.cout)
    assert np.abs(y - ref).max() < 1e-12
    assert np.abs(t).max() <= OU.T_MAX and (bound > 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("case", OU.POOL_CASES, ids=[c.name for c in OU.POOL_CASES])
def test_pool_reference_equals_torch(case):
    buf = OU.pool_data(case, OU.MAX_BATCH)
    ref = OU.pool_ref(buf, case.soff, case.doff, case.C)
    x = torch.from_numpy(np.ascontiguousarray(buf[..., case.soff:case.soff + case.C])).permute(0, 3, 1, 2)
    y = F.max_pool2d(x, 5, 1, 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ref[..., case.doff:case.doff + case.C], y)
    keep = np.ones(buf.shape, bool)
    keep[..., case.doff:case.doff + case.C] = False
    assert np.array_equal(ref.view(np.uint32)[keep], buf.view(np.uint32)[keep])


@pytest.mark.parametrize("case", OU.UP_CASES, ids=[c.name for c in OU.UP_CASES])
def test_upcopy_reference_equals_torch(case):
    src, _ = OU.up_data(case, OU.MAX_BATCH)
    ref = OU.upcopy_ref(src, case.soff, case.C, case.f)
    x = torch.from_numpy(np.ascontiguousarray(src[..., case.soff:case.soff + case.C])).permute(0, 3, 1, 2)
    y = F.interpolate(x, scale_factor=case.f, mode="nearest").permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ref, y) and ref.shape == (OU.MAX_BATCH, case.Hs * case.f, case.Ws * case.f, case.C)


@pytest.mark.parametrize("case", OU.GATE_CASES, ids=[c.name for c in OU.GATE_CASES])
def test_gate_reference_equals_torch_and_float32_stays_inside(case):
    d = OU.gate_data(case)
    embed = case.heads * case.hc
    for q_set in OU.GATE_SETS:
        text = OU.gate_text(q_set)
        e = d.emb[0, :, :, case.off:case.off + embed].reshape(-1, embed)
        ref, bound, v = OU.gate_ref(e, text, d.W, d.b, d.bias, case.heads)
        guide = torch.from_numpy(text).double() @ torch.from_numpy(d.W).double().t() + torch.from_numpy(d.b).double()
        dots = torch.einsum("pmc,nmc->pnm", torch.from_numpy(np.ascontiguousarray(e)).double().reshape(-1, case.heads, case.hc),
                            guide.reshape(-1, case.heads, case.hc))
        y = torch.sigmoid(dots.max(dim=1).values / case.hc ** 0.5 + torch.from_numpy(d.bias).double()).numpy()
        assert np.abs(y - ref).max() < 1e-12 and np.abs(v).max() <= OU.T_MAX
        f32, _, _ = OU.gate_ref(e, text, d.W, d.b, d.bias, case.heads, dtype=np.float32)
        assert f32.dtype == np.float32
        ratio = (np.abs(f32.astype(np.float64) - ref) / bound).max()
        assert ratio < 1.0, ratio


# ------------------------------------------------------------------------------------------ (b) float32 stays inside the bound
@pytest.mark.parametrize("case", OU.CONV_CASES, ids=IDS)
def test_float32_evaluation_stays_inside_the_bound(case):
    d = OU.conv_data(case)
    ref, bound, _ = OU.case_reference(case, d)
    f32, _, _ = OU.case_reference(case, d, dtype=np.float32)
    assert f32.dtype == np.float32
    ratio = (np.abs(f32.astype(np.float64) - ref) / bound).max()
    assert ratio < 1.0, ratio


# ------------------------------------------------------------------------------------------ (c) sensitivity
@pytest.mark.parametrize("case", OU.CONV_CASES, ids=IDS)
def test_cases_tell_wrong_kernels_apart(case):
    d = OU.conv_data(case)
    ref, bound, _ = OU.case_reference(case, d)
    muts = OU.conv_mutants(case, d)
    want = {"tap_zeroed", "last_cin_dropped", "last_cout_shifted"}
    if case.mode == "gate" and case.heads > 1:
        want.add("gate_next_head")
    if case.mode == "gate" and case.cout // case.heads < 4:
        want.add("gate_head_of_quad")
    if case.mode == "res" and case.act == Y.ACT_SILU:
        want.add("residual_before_act")
    if case.act == Y.ACT_SILU:
        want.add("no_activation")
    assert set(muts) == want
    for name, m in muts.items():
        assert (np.abs(m - ref) / bound).max() > 10.0, name


def test_gate_cases_tell_a_wrong_head_apart():
    for case in OU.GATE_CASES:
        if case.heads == 1:
            continue
        d = OU.gate_data(case)
        embed = case.heads * case.hc
        e = d.emb[0, :, :, case.off:case.off + embed].reshape(-1, embed)
        text = OU.gate_text(0)
        ref, bound, _ = OU.gate_ref(e, text, d.W, d.b, d.bias, case.heads)
        wrong, _, _ = OU.gate_ref(e, text, d.W, d.b, np.roll(d.bias, 1), case.heads)          # the bias of the neighbouring head
        assert (np.abs(wrong - ref) / bound).max() > 10.0, case.name
        rolled = np.roll(e.reshape(-1, case.heads, case.hc), 1, axis=1).reshape(-1, embed)      # the channels of the neighbouring head
        wrong, _, _ = OU.gate_ref(rolled, text, d.W, d.b, d.bias, case.heads)
        assert (np.abs(wrong - ref) / bound).max() > 10.0, case.name


# ------------------------------------------------------------------------------------------ (d) reach
def test_every_form_is_reached_by_the_case_table():
    """One child interpreter per policy environment (the library reads the overrides once per process): the plan entry puts every
    case on the form its row's family names under that environment, and every form is reached by at least three cases."""
    code = ("import json, sys; sys.path.insert(0, %r); import yolo_ops_util as OU; "
            "print('PLAN', json.dumps({c.name: OU.plan_of_case(c, True)[0] for c in OU.CONV_CASES}))" % HERE)
    reached = {f: set() for f in OU.ALL_FORMS}
    for name, env in OU.ENVS:
        p = subprocess.run([sys.executable, "-c", code], env=OU.child_env(env), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        plan = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("PLAN ")][0][5:])
        for c in OU.CONV_CASES:
            assert plan[c.name] == OU.FORM_OF[c.family][name], (name, c.name, plan[c.name])
            reached[plan[c.name]].add(c.name)
    assert all(len(v) >= 3 for v in reached.values()), {f: len(v) for f, v in reached.items()}
