"""OWL-ViT B/16 support on the host side (no GPU): checkpoint geometry detection, the B/16 weight blob, ``box_bias`` at grid
48 against HF's own buffer, refusal of unsupported geometries, and B/32 defaults that stay exactly as they were."""
import json
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def b16_dir(tmp_path_factory):
    """An HF-initialised ``OwlViTForObjectDetection`` with patch 16 saved by ``save_pretrained`` (config.json +
    model.safetensors): what ``google/owlvit-base-patch16`` looks like on disk, made offline."""
    import torch
    import transformers
    d = str(tmp_path_factory.mktemp("owlvit_b16"))
    torch.manual_seed(0)
    m = transformers.OwlViTForObjectDetection(transformers.OwlViTConfig(vision_config={"patch_size": 16})).eval()
    m.save_pretrained(d, safe_serialization=True)
    return d, m


def test_checkpoint_geometry_and_blob(b16_dir):
    from tstar_amd import _lib, weights as W
    d, _ = b16_dir
    g = W.geometry_of_checkpoint(d)
    assert g == W.B16 and (g.grid, g.npatch, g.ntok, g.patch_k) == (48, 2304, 2305, 768)
    assert W.geometry_of_checkpoint(os.path.join(d, "model.safetensors")) == W.B16
    sd = W.load_safetensors_state_dict(os.path.join(d, "model.safetensors"))
    assert "box_bias" not in sd                                  # transformers 5.x: a non-persistent buffer
    blob = W.pack_blob(sd, W.vision_spec(W.B16))
    back = W.unpack_blob(blob, W.vision_spec(W.B16))
    assert back["patch_w"].shape == (768, 768) and back["pos_emb"].shape == (2305, 768) and back["box_bias"].shape == (2304, 4)
    for name, _, hf_names in W.vision_spec(W.B16):               # every entry comes back as the tensors it was packed from
        want = W.compute_box_bias(W.B16) if name == "box_bias" else np.concatenate([sd[h].reshape(-1) for h in hf_names])
        assert np.array_equal(back[name].reshape(-1), want.reshape(-1)), name
    lib = _lib.load()
    assert lib.tstar_owl_vision_blob_floats_ex(768, 16) == blob.size == W.spec_size(W.vision_spec(W.B16))
    assert lib.tstar_owl_vision_blob_floats_ex(768, 32) == lib.tstar_owl_vision_blob_floats() == W.spec_size(W.vision_spec())
    assert lib.tstar_owl_vision_blob_floats_ex(840, 14) == 0
    with pytest.raises(ValueError, match="expected"):
        W.pack_blob(sd, W.vision_spec())                         # B/16 weights do not fit the B/32 layout


def test_box_bias_grid48_matches_hf(b16_dir):
    from tstar_amd import weights as W
    _, m = b16_dir
    hf48 = m.box_bias.numpy()
    assert hf48.shape == (2304, 4)
    ours = W.compute_box_bias(W.B16)
    assert ours.dtype == np.float32 and np.array_equal(ours.view(np.uint32), hf48.view(np.uint32))
    assert np.array_equal(m.compute_box_bias(48, 48).numpy().view(np.uint32), ours.view(np.uint32))
    b32 = W.compute_box_bias()                                   # the default stays the 24 x 24 B/32 buffer
    assert b32.shape == (576, 4)
    assert np.array_equal(b32.view(np.uint32), m.compute_box_bias(24, 24).numpy().view(np.uint32))
    assert np.array_equal(b32, W.compute_box_bias(W.B32))


def _config(vision=None, text=None, **top):
    c = {"model_type": "owlvit", "projection_dim": 512, "vision_config": dict(vision or {}), "text_config": dict(text or {})}
    c.update(top)
    return c


def test_unsupported_geometries_raise(tmp_path):
    from tstar_amd import weights as W
    l14 = _config(vision=dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=840,
                              patch_size=14),
                  text=dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12), projection_dim=768)
    (tmp_path / "config.json").write_text(json.dumps(l14))
    with pytest.raises(ValueError, match=r"unsupported OWL-ViT geometry \(vision hidden 1024.*patch 14.*supported: OWL-ViT B/32 and B/16"):
        W.geometry_of_checkpoint(str(tmp_path))                  # no weights needed: the config alone is refused
    with pytest.raises(ValueError, match="owlv2"):
        W.geometry_of_config(dict(_config(), model_type="owlv2"))
    with pytest.raises(ValueError, match="patch 8"):
        W.geometry_of_config(_config(vision=dict(patch_size=8)))
    with pytest.raises(ValueError, match="image 960"):
        W.geometry_of_config(_config(vision=dict(image_size=960)))
    with pytest.raises(ValueError, match="projection 768"):
        W.geometry_of_config(_config(projection_dim=768))
    with pytest.raises(ValueError, match="not supported"):
        W.geometry_for_patch(14)
    assert W.geometry_of_config(_config()) == W.B32                 # a config that leaves the defaults out is B/32
    assert W.geometry_of_config(_config(vision=dict(patch_size=16))) == W.B16


def test_config_disagreeing_with_the_weights_raises(b16_dir, tmp_path):
    import shutil
    from tstar_amd import weights as W
    d, _ = b16_dir
    shutil.copy(os.path.join(d, "model.safetensors"), tmp_path / "model.safetensors")
    cfg = json.load(open(os.path.join(d, "config.json")))
    cfg["vision_config"]["patch_size"] = 32
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match=r"config.json says B/32 .* but the weights are B/16"):
        W.geometry_of_checkpoint(str(tmp_path))
    os.remove(tmp_path / "config.json")
    assert W.geometry_of_checkpoint(str(tmp_path)) == W.B16        # without a config the tensor shapes decide
    # shapes that disagree with each other
    with pytest.raises(ValueError, match="position_embedding"):
        W.geometry_of_state_dict({W._PATCH_KEY: (768, 3, 16, 16), W._POS_KEY: (577, 768)})
    with pytest.raises(ValueError, match="patch_embedding"):
        W.geometry_of_state_dict({W._PATCH_KEY: (768, 3, 14, 14), W._POS_KEY: (3601, 768)})


def test_b32_defaults_unchanged():
    from tstar_amd import weights as W
    assert W.vision_spec() == W.vision_spec(W.B32)
    assert (W.PATCH, W.GRID, W.NPATCH, W.NTOK) == (32, 24, 576, 577)
    assert (W.B32.grid, W.B32.npatch, W.B32.ntok, W.B32.patch_k) == (W.GRID, W.NPATCH, W.NTOK, 3 * W.PATCH * W.PATCH)
    a = W.synthetic_state_dict(0)
    b = W.synthetic_state_dict(0, geometry=W.B32)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert np.array_equal(W.pack_blob(a, W.vision_spec()), W.pack_blob(b, W.vision_spec(W.B32)))
    assert W.geometry_of_state_dict(a) == W.B32


def test_b16_synthetic_weights():
    """Seeded synthetic B/16 weights: the B/16 shapes, the text tower identical to B/32's (its own stream), blob size right."""
    from tstar_amd import weights as W
    s16 = W.synthetic_state_dict(0, geometry=W.B16)
    assert s16["owlvit.vision_model.embeddings.patch_embedding.weight"].shape == (768, 3, 16, 16)
    assert s16["owlvit.vision_model.embeddings.position_embedding.weight"].shape == (2305, 768)
    assert W.geometry_of_state_dict(s16) == W.B16
    t32 = W.synthetic_state_dict(0, "text")
    for k, v in t32.items():
        assert np.array_equal(s16[k], v), k
    assert W.pack_blob(s16, W.vision_spec(W.B16)).size == W.spec_size(W.vision_spec(W.B16))
