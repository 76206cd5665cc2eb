"""GPU: the YOLO-World layer ops one at a time on crafted single-op programs (tests/yolo_ops_util.py), each kernel form
against a float64 reference under a derived per-output bound, with poisoned surroundings, and the form that ran asserted.

Conv cases run in one child interpreter per policy environment (tests/yolo_ops_probe.py); pool, up-copy and gate cases run
in-process.  The largest error / bound ratio per case and form is written to $TSTAR_YOLO_OPS_RATIOS when that is set
(profiles/yolo_ops_error_ratios.md is such a run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yolo_ops_util as OU
from tstar_amd import yolo_world as Y

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _write_ratios(sections):
    path = os.environ.get("TSTAR_YOLO_OPS_RATIOS")
    if not path:
        return
    have = {}
    if os.path.exists(path):
        for block in open(path).read().split("\n## ")[1:]:
            have[block.split("\n", 1)[0]] = block.split("\n", 1)[1].rstrip("\n")
    have.update(sections)
    with open(path, "w") as f:
        f.write("# YOLO layer ops: largest |device - float64 reference| / bound per case\n\n"
                "Written by tests/test_gpu_yolo_ops.py (bound: tests/yolo_ops_util.py).  1.0 is the bound; pool and up-copy are compared bit for bit.\n")
        for k in sorted(have):
            f.write(f"\n## {k}\n{have[k]}\n")


def test_conv_forms_on_crafted_programs(tmp_path):
    """Per case and policy environment: the launcher reports the form the plan names (and the row's family names); the output is
    within the bound of the float64 reference; nothing outside [dst_off, dst_off + cout) x the first B images changed and no output
    is NaN although everything the op must not read is NaN; the tile, scalar-weight and halo forms agree bit for bit."""
    probe = os.path.join(HERE, "yolo_ops_probe.py")
    runs = {}
    for name, env in OU.ENVS:                                 # one child at a time; nothing is started after one that failed
        path = str(tmp_path / f"{name}.npz")
        p = subprocess.run([sys.executable, probe, path], env=OU.child_env(env), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "PROBE_OK" in p.stdout, (name, p.returncode, p.stdout[-1000:], p.stderr[-3000:])
        runs[name] = np.load(path)
        code = ("import json, sys; sys.path.insert(0, %r); import yolo_ops_util as OU; "
                "print('PLAN', json.dumps({c.name: OU.plan_of_case(c, True)[0] for c in OU.CONV_CASES}))" % HERE)
        q = subprocess.run([sys.executable, "-c", code], env=OU.child_env(env), capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, q.stderr[-2000:]
        runs[name + "/plan"] = json.loads([ln for ln in q.stdout.splitlines() if ln.startswith("PLAN ")][0][5:])
    failures, lines, reached = [], [], {f: 0 for f in OU.ALL_FORMS}
    worst = 0.0
    for c in OU.CONV_CASES:
        d = OU.conv_data(c)
        by_form = {}
        for name, _ in OU.ENVS:
            form = str(runs[name]["form/" + c.name])
            got = runs[name]["out/" + c.name]
            if form != runs[name + "/plan"][c.name] or form != OU.FORM_OF[c.family][name]:
                failures.append(f"{c.name} [{name}]: ran {form}, planned {runs[name + '/plan'][c.name]}, row names {OU.FORM_OF[c.family][name]}")
            try:
                ratio = OU.check_conv_output(c, d, got)
            except AssertionError as e:
                failures.append(f"{c.name} [{name} -> {form}]: {e}")
                continue
            print(f"{c.name:16s} {name:8s} {form:9s} error / bound = {ratio:.4f}")
            if ratio >= 1.0:
                failures.append(f"{c.name} [{name} -> {form}]: error / bound = {ratio:.3f}")
            by_form.setdefault(form, []).append((ratio, got))
        for form, rs in by_form.items():
            reached[form] += 1
            worst = max(worst, max(r for r, _ in rs))
            lines.append(f"| {c.name} | {form} | {c.K} | {max(r for r, _ in rs):.4f} |")
        if c.family in OU.BIT_IDENTICAL_FAMILIES:
            outs = [(f, g) for f, rs in by_form.items() for _, g in rs]
            for f, g in outs[1:]:
                if not np.array_equal(g.view(np.uint32), outs[0][1].view(np.uint32)):
                    failures.append(f"{c.name}: forms {outs[0][0]} and {f} differ in bits")
    _write_ratios({"conv (case, form, K, largest ratio over the environments that ran the form)":
                   "\n| case | form | K | max error / bound |\n|---|---|---|---|\n" + "\n".join(lines)})
    assert not failures, "\n".join(failures)
    assert all(n >= 3 for n in reached.values()), reached
    print(f"largest conv error / bound: {worst:.4f}")


def _detector(prog):
    from tstar_amd.yolo import YoloDetector
    return YoloDetector.from_program(prog, max_batch=OU.MAX_BATCH)


def _poison_tail(a, B):
    a = a.copy()
    a[B:].view(np.uint32)[...] = OU.SENTINEL_BITS
    return a


@pytest.mark.parametrize("B", [1, 2, 3])
def test_pool_and_upcopy_move_bits(B):
    """pool5_kernel and upcopy_kernel on odd maps and channel offsets: the written channels equal the reference bit for bit and
    every other element (other channels, images >= B) keeps its bits."""
    prog, pools, ups = OU.move_program()
    det = _detector(prog)
    pd = [OU.pool_data(c, B) for c in OU.POOL_CASES]
    ud = [OU.up_data(c, B) for c in OU.UP_CASES]
    for buf, a in zip(pools, pd):
        det.write_buffer(buf, torch.from_numpy(a).cuda(), OU.MAX_BATCH)
    for (s, d), (sa, da) in zip(ups, ud):
        det.write_buffer(s, torch.from_numpy(sa).cuda(), OU.MAX_BATCH)
        det.write_buffer(d, torch.from_numpy(da).cuda(), OU.MAX_BATCH)
    forms = det.run_ops(B)
    assert (forms == -1).all()
    for c, buf, a in zip(OU.POOL_CASES, pools, pd):
        got = det.read_buffer(buf, OU.MAX_BATCH).cpu().numpy()
        want = a.copy()
        want[:B] = OU.pool_ref(a[:B], c.soff, c.doff, c.C)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c.name
        assert not np.isnan(got[:B, :, :, c.doff:c.doff + c.C]).any(), c.name
    for c, (s, d), (sa, da) in zip(OU.UP_CASES, ups, ud):
        got = det.read_buffer(d, OU.MAX_BATCH).cpu().numpy()
        want = da.copy()
        want[:B, :, :, c.doff:c.doff + c.C] = OU.upcopy_ref(sa[:B], c.soff, c.C, c.f)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c.name
        assert not np.isnan(got[:B, :, :, c.doff:c.doff + c.C]).any(), c.name
    det.close()


def test_gate_op_against_reference():
    """attn_kernel (both branches: 32 channels per head as float4, any other head width or alignment as scalars) and
    guide_fc_kernel: per image the query set the batch names, gates within the bound of the float64 reference, rows of images >= B
    untouched, NaN outside the read channels and in images >= B never reaches an output."""
    prog, where = OU.gate_program()
    det = _detector(prog)
    for q_set, Q in OU.GATE_SETS.items():
        det.set_text_feats(OU.gate_text(q_set), [1.0] * Q, slot=q_set)
    data = [OU.gate_data(c) for c in OU.GATE_CASES]
    lines, failures = [], []
    for B, sets in OU.GATE_RUNS:
        for c, d, (src, dst) in zip(OU.GATE_CASES, data, where):
            det.write_buffer(src, torch.from_numpy(_poison_tail(d.emb, B)).cuda(), OU.MAX_BATCH)
            det.write_buffer(dst, torch.from_numpy(OU.sentinel_array((OU.MAX_BATCH, c.H, c.W, c.heads))).cuda(), OU.MAX_BATCH)
        det.run_ops(B, image_sets=sets)
        for c, d, (src, dst) in zip(OU.GATE_CASES, data, where):
            got = det.read_buffer(dst, OU.MAX_BATCH).cpu().numpy()
            embed = c.heads * c.hc
            if not (got[B:].view(np.uint32) == OU.SENTINEL_BITS).all():
                failures.append(f"{c.name} B={B}: rows of images >= B were written")
            worst = 0.0
            for b in range(B):
                text = OU.gate_text(sets[b] if sets is not None else 0)
                ref, bound, v = OU.gate_ref(d.emb[b, :, :, c.off:c.off + embed].reshape(-1, embed), text, d.W, d.b, d.bias, c.heads)
                g = got[b].reshape(-1, c.heads)
                if np.isnan(g).any():
                    failures.append(f"{c.name} B={B} image {b}: NaN in the gate")
                    continue
                worst = max(worst, float((np.abs(g.astype(np.float64) - ref) / bound).max()))
            print(f"{c.name:18s} B={B} sets={sets} error / bound = {worst:.4f}")
            lines.append(f"| {c.name} | {c.hc} | {c.heads} | {B} | {sets} | {worst:.4f} |")
            if worst >= 1.0:
                failures.append(f"{c.name} B={B} sets={sets}: error / bound = {worst:.3f}")
    _write_ratios({"gate op (attn_kernel + guide_fc_kernel)": "\n| case | hc | heads | B | query sets | max error / bound |\n|---|---|---|---|---|---|\n" + "\n".join(lines)})
    det.close()
    assert not failures, "\n".join(failures)
