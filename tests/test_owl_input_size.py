"""OWL-ViT at an input size other than the checkpoint's 768 x 768, host side: the position table and ``box_bias`` packed for
the run geometry against HF's own ``interpolate_pos_encoding`` / ``compute_box_bias`` (bit for bit), blob sizes against the
library, and the sizes / settings that are refused before the device is touched."""
import numpy as np
import pytest

import owl_input_size_util as U

SIZES = [(32, (448, 768)), (32, (384, 800)), (32, (352, 640)), (16, (384, 800))]
_MODELS = {}


def _model(patch):
    if patch not in _MODELS:
        _MODELS[patch] = U.make_hf_model(patch, seed=3)
    return _MODELS[patch]


def _packed(patch, size):
    from tstar_amd import weights as W
    g = W.with_input_size(W.geometry_for_patch(patch), size)
    sd = {k: v.numpy() for k, v in _model(patch).state_dict().items()}
    spec = W.vision_spec(g)
    return g, W.unpack_blob(W.pack_blob(sd, spec, g), spec)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("patch,size", SIZES)
def test_pos_emb_is_hfs_interpolation_bit_for_bit(patch, size):
    import torch
    g, w = _packed(patch, size)
    assert (g.gh, g.gw) == (size[0] // patch, size[1] // patch) and g.npatch == g.gh * g.gw and g.ntok == g.npatch + 1
    emb = _model(patch).owlvit.vision_model.embeddings
    with torch.no_grad():
        ref = emb.interpolate_pos_encoding(torch.zeros(1, g.ntok, 768), size[0], size[1])[0].numpy()
    assert w["pos_emb"].shape == ref.shape == (g.ntok, 768)
    assert np.array_equal(_bits(w["pos_emb"]), _bits(ref))
    assert np.array_equal(_bits(w["pos_emb"][0]), _bits(emb.position_embedding.weight.detach().numpy()[0]))     # row 0 kept


@pytest.mark.parametrize("patch", [32, 16])
def test_pos_emb_at_the_checkpoint_size_is_the_stored_table(patch):
    from tstar_amd import weights as W
    g, w = _packed(patch, (768, 768))
    assert g == W.geometry_for_patch(patch) and g in (W.B32, W.B16)
    stored = _model(patch).owlvit.vision_model.embeddings.position_embedding.weight.detach().numpy()
    assert np.array_equal(_bits(w["pos_emb"]), _bits(stored))
    sd = {k: v.numpy() for k, v in _model(patch).state_dict().items()}
    assert np.array_equal(W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.vision_spec(g)))            # the blob of the parent commit


@pytest.mark.parametrize("patch,size", SIZES + [(32, (768, 768)), (16, (768, 768))])
def test_box_bias_is_hfs_bit_for_bit(patch, size):
    from tstar_amd import weights as W
    g, w = _packed(patch, size)
    ref = _model(patch).compute_box_bias(g.gh, g.gw).numpy()
    assert w["box_bias"].shape == ref.shape == (g.npatch, 4)
    assert np.array_equal(_bits(w["box_bias"]), _bits(ref))
    assert np.array_equal(_bits(W.compute_box_bias(g)), _bits(ref))


def test_geometry_keeps_its_meaning_at_the_default():
    from tstar_amd import weights as W
    assert W.OwlGeometry(768, 32) == W.B32 == W.OwlGeometry(768, 32, 768, 768) == W.with_input_size(W.B32, None)
    assert W.with_input_size(W.B32, (768, 768)) == W.B32 and hash(W.with_input_size(W.B16, (768, 768))) == hash(W.B16)
    g = W.with_input_size(W.B32, (448, 768))
    assert g != W.B32 and g.checkpoint == W.B32 and g.grid == 24 and (g.gh, g.gw, g.npatch, g.ntok) == (14, 24, 336, 337)
    assert g.patch_k == 3072 and g.name == "B/32" and g.input_size == (448, 768)
    assert W.with_input_size(g, None) == W.B32                                  # the size belongs to the run, not to the checkpoint
    big = W.with_input_size(W.B16, (960, 960))
    assert big.npatch == 3600 and big.ntok == 3601


@pytest.mark.parametrize("patch,size", SIZES + [(32, (768, 768)), (16, (768, 768)), (16, (960, 960)), (32, (32, 32))])
def test_spec_sizes_equal_the_library(patch, size):
    from tstar_amd import _lib, weights as W
    lib = _lib.load()
    g = W.with_input_size(W.geometry_for_patch(patch), size)
    n = lib.tstar_owl_vision_blob_floats_in(size[0], size[1], patch)
    assert n == W.spec_size(W.vision_spec(g)) > 0
    if size == (768, 768):
        assert n == lib.tstar_owl_vision_blob_floats_ex(768, patch)


def test_library_refuses_what_python_refuses():
    from tstar_amd import _lib
    lib = _lib.load()
    for h, w, p in [(450, 768, 32), (0, 768, 32), (32 * 61, 32 * 61, 32), (448, 768, 14), (-32, 64, 32), (976, 976, 16)]:
        assert lib.tstar_owl_vision_blob_floats_in(h, w, p) == 0, (h, w, p)
    assert lib.tstar_owl_vision_blob_floats_ex(840, 14) == 0
    assert b"input size" in lib.tstar_last_error() or b"geometry" in lib.tstar_last_error()


@pytest.mark.parametrize("size", [(450, 768), (0, 768), (32 * 61, 32 * 61)])
def test_invalid_sizes_raise_before_the_device(size, monkeypatch):
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface, initialize_heuristic
    from tstar_amd.owl import OwlScorer
    monkeypatch.delenv("TSTAR_INPUT_SIZE", raising=False)
    with pytest.raises(ValueError, match="multiple of the patch size"):
        W.with_input_size(W.B32, size)
    with pytest.raises(ValueError, match="multiple of the patch size"):
        W.vision_spec(W.with_input_size(W.B32, size))
    with pytest.raises(ValueError, match="multiple of the patch size"):
        OwlScorer(np.zeros(4, np.float32), None, max_batch=1, input_size=size)          # raised before the blob or a device is looked at
    with pytest.raises(ValueError, match="multiple of the patch size"):
        OWLInterface(synthetic_seed=0, max_batch=1, input_size=size)
    with pytest.raises(ValueError, match="multiple of the patch size"):
        initialize_heuristic("owl-vit", synthetic_seed=0, max_batch=1, input_size=size)
    monkeypatch.setenv("TSTAR_INPUT_SIZE", f"{size[0]}x{size[1]}")
    with pytest.raises(ValueError, match="multiple of the patch size"):
        OWLInterface(synthetic_seed=0, max_batch=1)


@pytest.mark.parametrize("text", ["448", "448x", "x768", "448x768x3", "big", "448*768", "44.8x768", "-448x768"])
def test_malformed_environment_setting_raises(text, monkeypatch):
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface
    monkeypatch.setenv("TSTAR_INPUT_SIZE", text)
    with pytest.raises(ValueError, match="TSTAR_INPUT_SIZE"):
        W.input_size_from_env()
    with pytest.raises(ValueError, match="TSTAR_INPUT_SIZE"):
        OWLInterface(synthetic_seed=0, max_batch=1)


def test_keyword_wins_over_the_environment(monkeypatch):
    from tstar_amd import weights as W
    monkeypatch.delenv("TSTAR_INPUT_SIZE", raising=False)
    assert W.resolve_input_size(None) is None
    monkeypatch.setenv("TSTAR_INPUT_SIZE", "")
    assert W.resolve_input_size(None) is None
    monkeypatch.setenv("TSTAR_INPUT_SIZE", "384x800")
    assert W.resolve_input_size(None) == (384, 800) and W.input_size_from_env() == (384, 800)
    assert W.resolve_input_size((448, 768)) == (448, 768)
    monkeypatch.setenv("TSTAR_INPUT_SIZE", "not a size")                         # never parsed when the keyword is given
    assert W.resolve_input_size((448, 768)) == (448, 768)
    with pytest.raises(ValueError):
        W.resolve_input_size(None)
