"""OWLv2 support, the parts that need no GPU: the numpy restatement of HF's ``Owlv2ImageProcessorPil`` against the processor
itself, ``box_bias`` / interpolated positions against HF's tensors, checkpoint recognition and refusals, the weight blob, and the
pre-processing policy (``tstar_owlv2_preprocess_plan``: windows that hold every tap, LDS within 160 KiB, impossible factors)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import owlv2_util as U
from tstar_amd import weights as W


# --------------------------------------------------------------------------------------------------------------- processor
@pytest.mark.parametrize("src,size", U.PROCESSOR_CASES)
def test_restatement_is_hfs_processor_bit_for_bit(src, size):
    H, Wd = src
    img = np.random.RandomState(H * 3 + Wd).randint(0, 256, (H, Wd, 3)).astype(np.uint8)
    if src == (131, 131):
        img = np.maximum(img, 9)                      # a square source is not padded: the lower clip bound is table[9], not 0
    for normalize in (False, True):
        want = U.hf_pixels(img, size, normalize)
        got = U.preprocess_restated(img, size, normalize)
        assert want.shape == got.shape == (3,) + tuple(size)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (src, size, normalize)


def test_gaussian_weights_are_scipys():
    from scipy.ndimage import _filters
    from tstar_amd.owl import owlv2_axis_radius, owlv2_gaussian_half
    for S, out in [(3200, 960), (200, 64), (800, 96), (4000, 64), (600, 480), (600, 960)]:
        sigma, lw = U.axis_sigma(S, out)
        assert owlv2_axis_radius(S, out) == lw
        half = owlv2_gaussian_half(S, out)
        if lw <= 0:
            assert half.tolist() == [1.0]
            continue
        want = _filters._gaussian_kernel1d(sigma, 0, lw)
        assert np.array_equal(half.view(np.uint64), want[:lw + 1].view(np.uint64)), (S, out)


def test_library_axis_tables():
    """The taps the kernels read are the restatement's, bit for bit; the library's own Gaussian weights (libm's exp) agree with
    numpy's to the last bit or the one before it (2^-52 relative: one ulp of exp) -- OwlScorer installs numpy's."""
    from tstar_amd import _lib
    lib = _lib.load()
    for S, out in [(3200, 960), (600, 480), (800, 64), (200, 96), (200, 64), (23, 64), (37, 64), (131, 96), (4320, 960)]:
        sigma, lw = U.axis_sigma(S, out)
        i0, i1 = np.zeros(out, np.int32), np.zeros(out, np.int32)
        t, gw = np.zeros(out), np.zeros(max(lw, 0) + 1)
        _lib.check(lib.tstar_owlv2_axis_tables(S, out, i0.ctypes.data, i1.ctypes.data, t.ctypes.data, gw.ctypes.data, gw.size))
        a, b, c = U.zoom_taps(S, out)
        assert np.array_equal(a, i0) and np.array_equal(b, i1) and np.array_equal(c.view(np.uint64), t.view(np.uint64)), (S, out)
        if lw > 0:
            want = U.gaussian_weights(sigma, lw)[:lw + 1]
            assert np.all(np.abs(gw - want) <= want * 2.0 ** -51), (S, out)
        else:
            assert gw.tolist() == [1.0]


# ----------------------------------------------------------------------------------------------------- box bias, positions
@pytest.fixture(scope="module")
def hf_model():
    return U.make_hf_model(seed=1)


@pytest.mark.parametrize("size", [(960, 960), (64, 96)])
def test_box_bias_and_positions_are_hfs(hf_model, size):
    import torch
    g = W.with_input_size(W.OWLV2_B16, size)
    assert (g.gh, g.gw) == (size[0] // 16, size[1] // 16) and g.family == "owlv2" and g.checkpoint == W.OWLV2_B16
    want = hf_model.compute_box_bias(g.gh, g.gw).numpy()
    got = W.compute_box_bias(g)
    assert got.shape == want.shape == (g.npatch, 4) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    emb = hf_model.owlv2.vision_model.embeddings
    with torch.no_grad():
        want = emb.interpolate_pos_encoding(torch.zeros(1, g.ntok, 768), size[0], size[1])
        want = want.reshape(g.ntok, 768).numpy()
    got = W.interpolate_pos_emb(emb.position_embedding.weight.detach().numpy(), g)
    assert got.shape == (g.ntok, 768) and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ geometry
def _cfg(image=960, patch=16, **vision):
    return {"model_type": "owlv2", "vision_config": dict({"image_size": image, "patch_size": patch}, **vision)}


def test_geometry_constants_and_defaults():
    assert W.OWLV2_B16 == W.OwlGeometry(960, 16, family="owlv2") != W.OwlGeometry(960, 16)
    assert (W.OWLV2_B16.grid, W.OWLV2_B16.npatch, W.OWLV2_B16.ntok, W.OWLV2_B16.patch_k) == (60, 3600, 3601, 768)
    assert W.B32 == W.OwlGeometry(768, 32) == W.OwlGeometry(768, 32, 768, 768, "owlvit") and W.B16.family == "owlvit"
    assert W.with_input_size(W.OWLV2_B16, (320, 480)) == W.OwlGeometry(960, 16, 320, 480, "owlv2")
    assert W.with_input_size(W.OWLV2_B16, (320, 480)).checkpoint == W.OWLV2_B16
    for bad in [(968, 960), (976, 960), (0, 16)]:
        with pytest.raises(ValueError):
            W.with_input_size(W.OWLV2_B16, bad)
    assert W.SUPPORTED_TEXT.startswith("OWL-ViT B/32 and B/16 (image 768") and "OWLv2" in W.SUPPORTED_TEXT
    assert W.geometry_for_family("owlv2") == W.OWLV2_B16 and W.geometry_for_family("owlvit", 16) == W.B16


def test_config_recognition_and_refusals():
    assert W.geometry_of_config(_cfg()) == W.OWLV2_B16
    assert W.geometry_of_config(_cfg(hidden_size=768, num_hidden_layers=12)) == W.OWLV2_B16
    refused = [
        {"model_type": "owlv2"},                                   # configuration_owlv2.py's own defaults: image 768, patch 16
        _cfg(768, 16), _cfg(960, 32), _cfg(1008, 14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16),
        _cfg(hidden_size=1024), dict(_cfg(), projection_dim=768), dict(_cfg(), text_config={"hidden_size": 768}),
    ]
    for cfg in refused:
        with pytest.raises(ValueError, match="owlv2"):
            W.geometry_of_config(cfg)
    with pytest.raises(ValueError):                              # image 960 belongs to OWLv2 alone
        W.geometry_of_config({"model_type": "owlvit", "vision_config": {"image_size": 960, "patch_size": 16}})
    with pytest.raises(ValueError, match="model_type"):
        W.geometry_of_config({"model_type": "clip"})


def test_state_dict_and_checkpoint_recognition(tmp_path):
    from safetensors.numpy import save_file
    pe, pos = "vision_model.embeddings.patch_embedding.weight", "vision_model.embeddings.position_embedding.weight"
    v2 = {"owlv2." + pe: (768, 3, 16, 16), "owlv2." + pos: (3601, 768)}
    assert W.geometry_of_state_dict(v2) == W.OWLV2_B16 and W.family_of_state_dict(v2) == "owlv2"
    assert W.geometry_of_state_dict({"owlvit." + pe: (768, 3, 16, 16), "owlvit." + pos: (2305, 768)}) == W.B16
    for bad in [{"owlv2." + pe: (768, 3, 16, 16), "owlv2." + pos: (2305, 768)},          # OWLv2 at image 768
                {"owlv2." + pe: (768, 3, 32, 32), "owlv2." + pos: (901, 768)},
                {"owlv2." + pe: (1024, 3, 14, 14), "owlv2." + pos: (5185, 1024)}]:
        with pytest.raises(ValueError, match="owlv2"):
            W.geometry_of_state_dict(bad)
    with pytest.raises(ValueError):
        W.geometry_of_state_dict({"clip." + pe: (768, 3, 16, 16)})
    # a checkpoint directory: config + safetensors header; a config that disagrees with the weights
    d = tmp_path / "ckpt"
    d.mkdir()
    save_file({"owlv2." + pe: np.zeros((768, 3, 16, 16), np.float32), "owlv2." + pos: np.zeros((3601, 768), np.float32)},
              str(d / "model.safetensors"))
    assert W.geometry_of_checkpoint(str(d)) == W.OWLV2_B16                    # no config: the tensors decide
    (d / "config.json").write_text(json.dumps(_cfg()))
    assert W.geometry_of_checkpoint(str(d)) == W.OWLV2_B16
    (d / "config.json").write_text(json.dumps({"model_type": "owlvit", "vision_config": {"patch_size": 16}}))
    with pytest.raises(ValueError, match="config.json says"):
        W.geometry_of_checkpoint(str(d))
    (d / "config.json").write_text(json.dumps(_cfg(768, 16)))
    with pytest.raises(ValueError, match="owlv2"):
        W.geometry_of_checkpoint(str(d))


def test_synthetic_weights_and_blob_round_trip():
    g = W.OWLV2_B16
    sd = W.synthetic_state_dict(3, geometry=g)
    assert all(k.startswith(("owlv2.", "class_head.", "box_head.", "objectness_head.", "layer_norm.")) or k == "box_bias" for k in sd)
    assert sd["owlv2.vision_model.embeddings.position_embedding.weight"].shape == (3601, 768)
    assert sd["objectness_head.dense2.weight"].shape == (1, 768) and sd["objectness_head.dense2.bias"].shape == (1,)
    assert W.geometry_of_state_dict(sd) == g
    vspec, tspec = W.vision_spec(g), W.text_spec(g)
    names = [n for n, _, _ in vspec]
    assert names[-6:] == ["obj0_w", "obj0_b", "obj1_w", "obj1_b", "obj2_w", "obj2_b"] and names[-7] == "box_bias"
    assert W.spec_size(vspec) == W.spec_size(W.vision_spec(W.with_input_size(W.B16, (960, 960)))) + 2 * (768 * 768 + 768) + 768 + 1
    blob = W.pack_blob(sd, vspec, g)
    back = W.unpack_blob(blob, vspec)
    for n, k in [("obj0_w", "objectness_head.dense0.weight"), ("obj1_b", "objectness_head.dense1.bias"), ("obj2_w", "objectness_head.dense2.weight"),
                 ("obj2_b", "objectness_head.dense2.bias"), ("box2_w", "box_head.dense2.weight"),
                 ("pos_emb", "owlv2.vision_model.embeddings.position_embedding.weight")]:
        assert np.array_equal(back[n].reshape(-1), sd[k].reshape(-1)), n
    assert np.array_equal(back["box_bias"], W.compute_box_bias(g))
    tb = W.unpack_blob(W.pack_blob(sd, tspec), tspec)
    assert np.array_equal(tb["text_proj"], sd["owlv2.text_projection.weight"])
    # a run at another size: positions resampled, box_bias for the run's grid, the objectness head untouched
    g2 = W.with_input_size(g, (64, 96))
    b2 = W.unpack_blob(W.pack_blob(sd, W.vision_spec(g2), g2), W.vision_spec(g2))
    assert b2["pos_emb"].shape == (25, 768) and b2["box_bias"].shape == (24, 4) and np.array_equal(b2["obj1_w"], back["obj1_w"])
    # the text tower's stream does not depend on the family's prefix; bf16 rounding covers the objectness matrices
    vit = W.synthetic_state_dict(3, "text")
    assert np.array_equal(vit["owlvit.text_projection.weight"], sd["owlv2.text_projection.weight"])
    r = W.round_weights_to_bf16(sd)
    assert np.array_equal(r["objectness_head.dense0.weight"], W.to_bf16_values(sd["objectness_head.dense0.weight"]))
    assert np.array_equal(r["objectness_head.dense0.bias"], sd["objectness_head.dense0.bias"])
    from tstar_amd import _lib
    lib = _lib.load()
    assert lib.tstar_owl_vision_blob_floats_family(1, 960, 960, 16) == blob.size
    assert lib.tstar_owl_vision_blob_floats_family(0, 960, 960, 16) == lib.tstar_owl_vision_blob_floats_in(960, 960, 16)
    assert lib.tstar_owl_vision_blob_floats_family(1, 960, 960, 32) == 0 and lib.tstar_owl_vision_blob_floats_family(2, 960, 960, 16) == 0
    assert lib.tstar_abi_version() == 3


# -------------------------------------------------------------------------------------------------------------------- policy
def _plan(lib, H, Wd, oh, ow):
    p = (C.c_int * 10)()
    rc = lib.tstar_owlv2_preprocess_plan(H, Wd, oh, ow, p)
    return rc, dict(zip(("form", "tile_h", "tile_w", "win_h", "win_w", "lds", "grid_x", "grid_y", "radius_y", "radius_x"), list(p)))


SIDES = [23, 37, 64, 95, 131, 200, 301, 600, 960, 1000, 1520, 2161, 3200, 4320]
OUTS = [(64, 64), (64, 96), (96, 64), (160, 160), (320, 480), (480, 960), (960, 960), (960, 64)]


def test_plan_windows_hold_every_tap_and_fit_lds():
    """Sources 23 .. 4320 on the longer side (both orientations), outputs 64 .. 960: either the plan is refused (an impossible
    factor, checked below) or it declares, for every tile of either axis, a window that holds every sample the restatement reads
    for the tile's outputs, no larger than win_h x win_w, within 160 KiB of LDS."""
    from tstar_amd import _lib
    lib = _lib.load()
    seen = set()
    for S in SIDES:
        for oh, ow in OUTS:
            for H, Wd in ((S, max(1, S * 9 // 16)), (max(1, S * 9 // 16), S), (S, S)):
                rc, p = _plan(lib, H, Wd, oh, ow)
                ry, rx = U.axis_sigma(S, oh)[1], U.axis_sigma(S, ow)[1]
                if rc != 0:
                    assert max(ry, rx) >= 20, (H, Wd, oh, ow)          # only a large shrink factor may be refused
                    seen.add("refused")
                    continue
                assert (p["radius_y"], p["radius_x"]) == (ry, rx)
                assert p["form"] == (0 if ry < 0 and rx < 0 else 1) and 0 < p["lds"] <= 160 * 1024
                seen.add(p["form"])
                if p["form"] == 0:
                    continue
                assert p["grid_y"] * p["tile_h"] >= oh > (p["grid_y"] - 1) * p["tile_h"]
                assert p["grid_x"] * p["tile_w"] >= ow > (p["grid_x"] - 1) * p["tile_w"]
                for out, tile, radius, win in ((oh, p["tile_h"], ry, p["win_h"]), (ow, p["tile_w"], rx, p["win_w"])):
                    w2 = (C.c_int * 2)()
                    tiles = range(-(-out // tile))
                    if len(tiles) > 12:                           # every tile at the edges, a spread in between
                        tiles = sorted(set(list(tiles[:4]) + list(tiles[-4:]) + list(tiles[::max(1, len(tiles) // 7)])))
                    for k in tiles:
                        assert lib.tstar_owlv2_axis_window(S, out, tile, k, radius, w2) == 0
                        lo, n = w2[0], w2[1]
                        a, b = U.axis_reads(S, out, k * tile, min((k + 1) * tile, out))
                        assert 0 <= lo <= a and b <= lo + n - 1 <= S - 1 and n <= win, (S, out, tile, k, lo, n, a, b, win)
    assert seen == {0, 1, "refused"}


def test_impossible_factors_are_refused():
    from tstar_amd import _lib
    lib = _lib.load()
    for H, Wd, oh, ow in [(4320, 4320, 64, 64), (4320, 2430, 64, 96), (1, 1, 64, 64), (600, 600, 60, 64), (0, 5, 64, 64)]:
        rc, _ = _plan(lib, H, Wd, oh, ow)
        assert rc == 1 and lib.tstar_last_error(), (H, Wd, oh, ow)
    assert _plan(lib, 4320, 2430, 960, 960)[0] == 0 and _plan(lib, 23, 37, 64, 64)[0] == 0
