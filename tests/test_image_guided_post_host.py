"""Image-guided detection's post-process, host side (no GPU): ``tstar_image_guided_postprocess_host`` -- the statements the device
kernel shares through csrc/image_guided_post_core.h -- against HF's own ``post_process_image_guided_detection`` bit for bit; the
general-box form of the query selection's restatement against HF's statements; the stand-alone checker under the sanitizers; and
the C surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_guided_post_util as G
import image_query_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = G.build_cases()


def test_the_case_list_covers_what_it_must():
    """Every np and both batch sizes, each kind of input, the three NMS thresholds, a threshold above every score, sizes given and
    not: no case of the list may be lost."""
    kinds = {k for c in CASES for k in c["kinds"]}
    assert kinds == {"random", "disjoint", "clusters", "chain", "straddle", "degenerate", "allzero"}
    for n in G.NP_LIST:
        assert {c["B"] for c in CASES if c["np"] == n} >= {1, 3}, n
        assert {k for c in CASES if c["np"] == n for k in c["kinds"]} >= {"random", "clusters", "degenerate", "allzero"}, n
    assert {c["nms"] for c in CASES} == {0.0, 0.3, 1.0}
    assert any(c["threshold"] > 1 for c in CASES) and any(0 < c["threshold"] < 1 for c in CASES)
    assert {c["sizes"] is None for c in CASES} == {True, False}
    assert any(c["np"] == 3600 and c["B"] == 3 for c in CASES)
    # the straddle really sits on the threshold: IoU == float32(0.3) and its two neighbours
    got = [G.iou_row(G.corners(np.stack(p)), 0)[1] for p in G._straddle_pairs()]
    assert got == [G.NMS, np.nextafter(G.NMS, np.float32(0)), np.nextafter(G.NMS, np.float32(1))]


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_host_entry_is_hfs_post_process_bit_for_bit(case):
    """HF's method on the crafted logits / boxes, then the host entry on sigmoid(max logit): the kept rows' alphas and scaled boxes
    have HF's bits, in patch order, and ``n_kept`` is HF's count; an image HF drops has an empty entry.  The numpy restatement
    (which the GPU tests use for the kept SET, HF returning only the compacted rows) agrees with both on every row."""
    G.assert_unambiguous(case)                                    # first: HF alone is unambiguous on these inputs
    hf = G.hf_post_process(case["logits"], case["boxes"], case["threshold"], case["nms"], case["sizes"])
    scores = G.scores_of(case["logits"])
    alphas, xyxy, keep, n_kept = G.host_entry(scores, case["boxes"], case["threshold"], case["nms"], G.scale_of(case["sizes"]))
    assert set(np.unique(keep)) <= {0, 1}
    rest = G.restated(case)
    for b in range(case["B"]):
        m = keep[b].astype(bool)
        assert n_kept[b] == m.sum() == len(hf[b][0]), (b, n_kept[b], len(hf[b][0]))
        assert G.same_bits(alphas[b][m], hf[b][0]), b
        assert G.same_bits(xyxy[b][m], hf[b][1]), b
        r = rest[b]
        assert np.array_equal(m, r["keep"]) and G.same_bits(alphas[b], r["alphas"]) and G.same_bits(xyxy[b], r["boxes"]), b
        assert not alphas[b][~m].any()
        if case["kinds"][b] == "allzero":
            assert r["dropped"] and n_kept[b] == 0
    if case["threshold"] > 1:
        assert not n_kept.any()


def test_host_entry_refuses_bad_arguments():
    from tstar_amd import _lib
    lib = _lib.load()
    s, b = np.full((1, 4), 0.5, np.float32), np.full((1, 4, 4), 0.25, np.float32)
    a, x, k, n = np.full((1, 4), -1, np.float32), np.full((1, 4, 4), -1, np.float32), np.full((1, 4), 9, np.uint8), np.full(1, -5, np.int32)

    def call(sp=s.ctypes.data, B=1, n_=4, ap=a.ctypes.data):
        return lib.tstar_image_guided_postprocess_host(sp, b.ctypes.data, B, n_, 0.0, 0.3, None, ap, x.ctypes.data, k.ctypes.data, n.ctypes.data)

    for kw in (dict(sp=None), dict(ap=None), dict(B=0), dict(n_=0), dict(n_=3601)):
        assert call(**kw) == 1, kw
        assert lib.tstar_last_error()
    assert (a == -1).all() and (x == -1).all() and (k == 9).all() and n[0] == -5
    assert call() == 0 and n[0] == 1                              # four identical boxes: one survives


# ----------------------------------------------------------------------------------------- the general-box restatement
@pytest.mark.parametrize("family", ["owlvit", "owlv2"])
def test_general_box_restatement_against_hf_statements(family):
    """The oracle of the GPU query-box test: at the unit box it is ``image_query_util``'s restatement and HF's statements bit for
    bit on every crafted case; at other boxes HF's ``box_iou`` / ``generalized_box_iou``, which are general, give the same
    values, threshold and selected set."""
    module, _ = U.hf_modules()[family]
    for np_ in (1, 12, 65, 576):
        for label, cls, boxes, q, r in G.box_cases(np_):
            values, used_giou, thr, selected = G.hf_statements_box(module, boxes, q)
            where = (family, np_, label)
            assert used_giou == r["used_giou"] and thr == r["thr"], where
            assert G.same_bits(values, r["values"]) and np.array_equal(selected, r["selected"]), where
            if np.array_equal(q, G.UNIT):
                v1, g1, t1, s1 = U.hf_statements(module, boxes)
                assert G.same_bits(v1, r["values"]) and g1 == used_giou and t1 == thr and np.array_equal(s1, selected), where


def test_general_box_restatement_is_hfs_embed_image_query_at_the_unit_box(tmp_path):
    """On HF-made ``class_embeds`` / ``pred_boxes`` (an HF-initialised B/32 model's forward of two example images): the
    restatement at the unit box selects HF's rows and HF's best index."""
    model = U.make_checkpoint("b32", str(tmp_path))
    q, t = U.query_and_target_images()
    ref = U.hf_image_guided("b32", model, q, t)
    U.assert_hf_margins(ref)
    for i, p in enumerate(ref["per_image"]):
        r = G.select_box(p["class_embeds"], p["boxes"], G.UNIT)
        assert G.same_bits(r["values"], p["values"]) and r["thr"] == p["thr"] and r["used_giou"] == p["used_giou"], i
        assert np.array_equal(r["selected"], p["selected"]) and r["best"] == p["best"], i
        ru = U.select(p["class_embeds"], p["boxes"])
        assert r["best"] == ru["best"] and np.array_equal(r["selected"], ru["selected"])


# ------------------------------------------------------------------------------------------- the checker under sanitizers
def test_core_under_address_and_ub_sanitizers(tmp_path):
    """csrc/image_guided_post_check_main.cpp with the host entry, built with -fsanitize=address,undefined (a stand-alone CPU
    program; nothing is loaded into python, nothing of the GPU is involved): every crafted case from a file (exact-size heap
    blocks; the tool compares with the expected outputs written beside them, word for word), then its own hostile inputs -- NaN
    and infinite scores and boxes, huge and negative thresholds, np at both limits, arguments the entry must refuse."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "image_guided_post_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           os.path.join(csrc, "image_guided_post_host.cpp"), os.path.join(csrc, "image_guided_post_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for i, case in enumerate(CASES):
        scale = G.scale_of(case["sizes"])
        rest = G.restated(case)
        p = tmp_path / f"case{i:03d}.bin"
        with open(p, "wb") as f:
            f.write(np.array([case["B"], case["np"], 0 if scale is None else 1], np.int32).tobytes())
            f.write(np.array([case["threshold"], case["nms"]], np.float32).tobytes())
            f.write(G.scores_of(case["logits"]).tobytes())
            f.write(case["boxes"].tobytes())
            if scale is not None:
                f.write(scale.tobytes())
            f.write(np.stack([x["alphas"] for x in rest]).tobytes())
            f.write(np.stack([x["boxes"] for x in rest]).tobytes())
            f.write(np.stack([x["keep"] for x in rest]).astype(np.uint8).tobytes())
            f.write(np.array([x["n_kept"] for x in rest], np.int32).tobytes())
        # a truncated copy: the tool must refuse the file, not read past its end
        if i % 7 == 0:
            t = tmp_path / f"case{i:03d}_truncated.bin"
            t.write_bytes(p.read_bytes()[:-(1 + i)])
            files.append(str(t))
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) + 1, r.stdout[-2000:]
    n_trunc = sum("_truncated" in f for f in files)
    assert sum(ln.endswith(" refused=truncated") for ln in lines) == n_trunc
    assert sum(ln.endswith(" differ=0") for ln in lines) == len(CASES)
    assert lines[-1].startswith("hostile ") and lines[-1].endswith(" bad=0") and int(lines[-1].split(" runs=")[1].split()[0]) >= 40


# ------------------------------------------------------------------------------------------------------------ the surface
def test_c_surface_declares_the_new_entries():
    from tstar_amd import _lib, build
    with open(os.path.join(ROOT, "include", "tstar_hip.h")) as f:
        header = f.read()
    sig = {"tstar_image_guided_postprocess": 12, "tstar_image_guided_postprocess_host": 11, "tstar_image_query_select_box": 11,
           "tstar_owl_embed_image_queries_box": 12}
    for name, nargs in sig.items():
        assert f"int {name}(" in header and len(_lib.SIGNATURES[name][1]) == nargs, name
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in sig) and lib.tstar_abi_version() == 3
    assert "image_guided_post.hip" in build.sources() and "image_guided_post_host.cpp" in build.sources()
    for src in ("image_guided_post.hip", "image_guided_post_host.cpp", "image_query.hip"):
        assert "-ffp-contract=off" in build.PER_FILE[src], src


def test_query_box_in_pixels_becomes_relative_or_raises():
    """``OWLInterface``'s conversion of a pixel box: float32(x) / float32(W), and ValueError naming the object for an empty, an
    inverted or an outside box (host logic: no device is touched)."""
    from tstar_amd.interface_heuristic import OWLInterface
    b = OWLInterface._relative_box((40, 24, 136, 104), 120, 168, "set_query_images: 'mug'")
    assert b.dtype == np.float32 and np.array_equal(b, G.relative_box((40, 24, 136, 104), 120, 168))
    for bad in ((40, 24, 40, 104), (136, 24, 40, 104), (40, 24, 169, 104), (-1, 0, 10, 10), (0, 0, 10, 121), (1, 2, 3), (0, 0, float("nan"), 5)):
        with pytest.raises(ValueError, match="'mug'"):
            OWLInterface._relative_box(bad, 120, 168, "set_query_images: 'mug'")
