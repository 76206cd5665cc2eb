"""Image-guided queries, host side: the numpy restatement of tests/image_query_util.py pinned against HF's own statements (both
families), the crafted cases of the selection kernel checked against it, the C surface, and the registry's name handling."""
import os
import re

import numpy as np
import pytest

import image_query_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_sets():
    """(cls, boxes) sets: uniform boxes, exact ties, zero-area boxes that drive the GIoU fallback, empty selections."""
    out = []
    for np_ in (1, 5, 64, 577):
        for k in range(40):
            rs = np.random.RandomState(7000 + 100 * np_ + k)
            cls = (rs.standard_normal((np_, U.PROJ)) * rs.uniform(0.2, 5.0, (np_, 1))).astype(np.float32)
            kind = k % 5
            if kind == 0:
                boxes = rs.uniform(0, 1, (np_, 4))
            elif kind == 1:                       # a grid of exactly representable boxes: ties at the maximum
                boxes = np.concatenate([np.full((np_, 2), 0.5), rs.choice([0.25, 0.5, 1.0], (np_, 2))], axis=1)
            elif kind == 2:                       # boxes reaching far outside
                boxes = np.concatenate([rs.uniform(-0.5, 1.5, (np_, 2)), rs.uniform(0, 2, (np_, 2))], axis=1)
            elif kind == 3:                       # zero-area boxes inside: every IoU 0, GIoU 0
                boxes = np.concatenate([rs.uniform(0.3, 0.7, (np_, 2)), rs.uniform(0, 0.5, (np_, 1)), np.zeros((np_, 1))], axis=1)
            else:                                 # zero-height boxes over the edge: every GIoU negative, empty selection
                boxes = np.concatenate([np.full((np_, 1), 0.9), rs.uniform(0.2, 0.8, (np_, 1)), rs.uniform(0.5, 1.0, (np_, 1)),
                                        np.zeros((np_, 1))], axis=1)
            out.append((cls, boxes.astype(np.float32)))
    return out


def _all_sets():
    sets = _random_sets()
    for np_ in U.CASE_NP:
        sets += [(c, b) for _, c, b, _ in U.build_cases(np_)]
    return sets


@pytest.mark.parametrize("family", ["owlvit", "owlv2"])
def test_restatement_is_hfs_selection_bit_for_bit(family):
    """IoU / GIoU values, the fallback decision, the threshold and the selected set equal HF's statements bit for bit; the best
    index equals HF's ``embed_image_query`` (float32 ``mean_sim``) wherever the float64 gap is at least 1e-3 of the largest
    |mean_sim| among the selected rows."""
    module, model_class = U.hf_modules()[family]
    compared = 0
    for cls, boxes in _all_sets():
        r = U.select(cls, boxes)
        values, used_giou, thr, selected = U.hf_statements(module, boxes)
        assert used_giou == r["used_giou"]
        assert np.array_equal(values.view(np.uint32), r["values"].view(np.uint32))
        assert np.float32(thr).view(np.uint32) == np.float32(r["thr"]).view(np.uint32)
        assert np.array_equal(selected, r["selected"])
        emb, best = U.hf_embed_image_query(model_class, cls, boxes)
        if r["n_selected"] == 0:
            assert emb is None and best == -1 and r["status"] == U.STATUS_EMPTY
            continue
        assert r["selected"][best]
        if r["gap"] >= 1e-3 * r["scale"]:
            compared += 1
            # identical rows tie exactly in float64 (the restatement takes the first); HF's float32 einsum gives them sums that differ in
            # the last bits by where the row falls in the BLAS kernel's blocking (it changes with the thread count), so its argmin may
            # name a later copy: another index must be a bit-identical row, and the embedding below is the same either way
            assert best == r["best"] or np.array_equal(cls[best].view(np.uint32), cls[r["best"]].view(np.uint32)), (best, r["best"])
            assert np.array_equal(emb.view(np.uint32), cls[r["best"]].view(np.uint32))
    assert compared > 150


def test_crafted_cases_are_what_they_claim():
    """Every numbered case of the kernel test gives, by the restatement, the outcome it was built for, with the planted
    ``mean_sim`` gap at least 64 x the error bound (so the GPU test may ask for the exact index)."""
    for np_ in U.CASE_NP:
        labels = [c[0][0] for c in U.build_cases(np_)]
        assert set(labels) == set("1467" if np_ == 1 else "12345678"), (np_, labels)
        for label, cls, boxes, exp in U.build_cases(np_):
            r = U.select(cls, boxes)
            where = (np_, label)
            assert r["status"] == exp["status"] and r["n_selected"] == exp["n_selected"] and r["best"] == exp["best"], where
            if "thr" in exp:
                assert np.float32(r["thr"]).view(np.uint32) == np.float32(exp["thr"]).view(np.uint32), where
            if exp["status"] == U.STATUS_GIOU:
                assert r["used_giou"] and np.all(r["iou"] == 0), where
            if label.startswith("5"):
                assert (r["giou"] < 0).sum() == np_ // 2 and not r["selected"][r["giou"] < 0].any(), where
            if label.startswith("6"):
                assert np.all(r["giou"] < 0), where
            if "twin" in exp:
                assert r["mean_sim"][exp["twin"]] == r["mean_sim"][exp["best"]] and exp["twin"] > exp["best"], where
            if r["n_selected"] > 1:
                assert r["gap"] >= 64 * U.mean_sim_bound(cls, r["selected"]), (where, r["gap"], U.mean_sim_bound(cls, r["selected"]))
    # the threshold straddle really has rows one ulp on either side of the threshold
    _, cls, boxes, exp = [c for c in U.build_cases(64) if c[0].startswith("3")][0]
    r = U.select(cls, boxes)
    thr = np.float32(np.float32(1.0 - 2.0 / 1024.0) * np.float32(0.8))
    assert (r["values"] == np.nextafter(thr, np.float32(0))).any() and (r["values"] == thr).any()
    assert not r["selected"][r["values"] == np.nextafter(thr, np.float32(0))].any() and r["selected"][r["values"] == thr].all()


def test_c_surface_declares_the_image_query_entries():
    from tstar_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tstar_hip.h")).read()
    declared = set(re.findall(r"\b(tstar_[a-z0-9_]+)\s*\(", hdr))
    new = {"tstar_owl_embed_image_queries", "tstar_image_query_select"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["tstar_owl_embed_image_queries"][1]) == 11 and len(_lib.SIGNATURES["tstar_image_query_select"][1]) == 10
    assert lib.tstar_abi_version() == 3


def test_selection_kernel_is_built_without_contraction():
    from tstar_amd import build
    assert "image_query.hip" in build.sources()
    assert "-ffp-contract=off" in build.PER_FILE["image_query.hip"]


def test_registry_rows_and_refusals():
    """The name handling of the registry without a device: which rows of a texts list an example image stands for."""
    from tstar_amd.interface_heuristic import OWLInterface, YoloWorldInterface
    h = OWLInterface.__new__(OWLInterface)
    h._query_images = {}
    texts = [["mug"], ["this person"], ["desk"], [" "]]
    assert h._image_overrides(texts) is None                                     # an empty registry changes nothing
    e = np.arange(512, dtype=np.float32)
    h._query_images = {"this person": e, " ": e + 1, "": e + 2}
    ov = h._image_overrides(texts)
    assert list(ov) == [1] and ov[1] is e                                        # never the trailing blank query
    assert h._image_overrides([["mug"], [" "]]) is None
    h.clear_query_images()
    assert h._query_images == {} and h.query_image_info == {}
    y = YoloWorldInterface.__new__(YoloWorldInterface)
    with pytest.raises(NotImplementedError, match="image-guided"):
        y.set_query_images({"mug": np.zeros((8, 8, 3), np.uint8)})
