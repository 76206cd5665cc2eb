// Device-side view of the OWL-ViT parameter blobs (B/32 and B/16).  Entry order mirrors
// tstar_amd/weights.py vision_spec()/text_spec() one to one; the host blob is packed,
// the device copy pads every entry to 64 floats so all rows stay 16-byte aligned.
#pragma once
#include <stddef.h>

namespace tstar {

// B/32 numbers (the default geometry); a handle's own geometry is an OwlGeom
constexpr int V_D = 768, V_FF = 3072, V_LAYERS = 12, V_HEADS = 12, V_NP = 576, V_NTOK = 577, V_PATCH_K = 3072;
constexpr int T_D = 512, T_FF = 2048, T_LAYERS = 12, T_HEADS = 8, T_LEN = 16, T_VOCAB = 49408, PROJ = 512;

// Patch geometry of the vision tower: every supported checkpoint shares the widths above and differs only here.  image / grid
// describe the CHECKPOINT (its position table is grid x grid); in_h x in_w is the input size of the RUN (a property of the
// handle; the checkpoint's own 768 x 768 unless the handle was created with another one), gh x gw its patch grid, np = gh gw
// the patches and ntok = np + 1 the tokens per image.
constexpr int V_MAX_NP = 3600;
struct OwlGeom {
    int image = 768, patch = 32, grid = 24, np = V_NP, ntok = V_NTOK, patch_k = V_PATCH_K;
    int in_h = 768, in_w = 768, gh = 24, gw = 24;
    int family = 0;              // TSTAR_OWL_FAMILY_OWLVIT (0) or TSTAR_OWL_FAMILY_OWLV2 (1: image 960, patch 16, an objectness head)
};
// the run geometry of a (input_h, input_w) input at patch 32 / 16, or false when the size is not supported: each side a
// positive multiple of the patch size, at most V_MAX_NP patches
inline bool owl_geom_input(int input_h, int input_w, int patch_size, OwlGeom* g) {
    if (patch_size != 32 && patch_size != 16) return false;
    if (input_h <= 0 || input_w <= 0 || input_h % patch_size || input_w % patch_size) return false;
    if ((long long)(input_h / patch_size) * (input_w / patch_size) > V_MAX_NP) return false;
    g->image = 768; g->patch = patch_size; g->grid = 768 / patch_size;
    g->in_h = input_h; g->in_w = input_w; g->gh = input_h / patch_size; g->gw = input_w / patch_size;
    g->np = g->gh * g->gw; g->ntok = g->np + 1; g->patch_k = 3 * patch_size * patch_size;
    return true;
}
// the run geometry of a handle of `family`: 0 = OWL-ViT (owl_geom_input), 1 = OWLv2 B/16 (checkpoint image 960, patch 16 only)
inline bool owl_geom_family(int family, int input_h, int input_w, int patch_size, OwlGeom* g) {
    if (family == 0) return owl_geom_input(input_h, input_w, patch_size, g);
    if (family != 1 || patch_size != 16 || !owl_geom_input(input_h, input_w, patch_size, g)) return false;
    g->image = 960; g->grid = 60; g->family = 1;
    return true;
}
// the geometry of (image_size, patch_size), or false when it is not supported (B/32 and B/16: image 768, patch 32 / 16)
inline bool owl_geom(int image_size, int patch_size, OwlGeom* g) {
    if (image_size != 768 || (patch_size != 32 && patch_size != 16)) return false;
    return owl_geom_input(image_size, image_size, patch_size, g);
}

struct LayerW {
    const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct VisionW {
    const float *patch_w, *class_emb, *pos_emb, *pre_ln_w, *pre_ln_b;
    LayerW layers[V_LAYERS];
    const float *post_ln_w, *post_ln_b, *det_ln_w, *det_ln_b;
    const float *cls_w, *cls_b, *shift_w, *shift_b, *scale_w, *scale_b;
    const float *box0_w, *box0_b, *box1_w, *box1_b, *box2_w, *box2_b, *box_bias;
    const float *obj0_w, *obj0_b, *obj1_w, *obj1_b, *obj2_w, *obj2_b;      // OWLv2 only (objectness_head), null otherwise
};

struct TextW {
    const float *tok_emb, *tpos_emb;
    LayerW layers[T_LAYERS];
    const float *final_ln_w, *final_ln_b, *text_proj;
};

// `take(n)` returns the pointer for the next entry of n floats.
template <class Take>
void map_layer(LayerW& l, int d, int ff, Take&& take) {
    l.ln1_w = take((size_t)d); l.ln1_b = take((size_t)d);
    l.qkv_w = take((size_t)3 * d * d); l.qkv_b = take((size_t)3 * d);
    l.out_w = take((size_t)d * d); l.out_b = take((size_t)d);
    l.ln2_w = take((size_t)d); l.ln2_b = take((size_t)d);
    l.fc1_w = take((size_t)ff * d); l.fc1_b = take((size_t)ff);
    l.fc2_w = take((size_t)d * ff); l.fc2_b = take((size_t)d);
}

template <class Take>
void map_vision(VisionW& w, const OwlGeom& g, Take&& take) {
    w.patch_w = take((size_t)V_D * g.patch_k);
    w.class_emb = take(V_D);
    w.pos_emb = take((size_t)g.ntok * V_D);
    w.pre_ln_w = take(V_D); w.pre_ln_b = take(V_D);
    for (int i = 0; i < V_LAYERS; ++i) map_layer(w.layers[i], V_D, V_FF, take);
    w.post_ln_w = take(V_D); w.post_ln_b = take(V_D);
    w.det_ln_w = take(V_D); w.det_ln_b = take(V_D);
    w.cls_w = take((size_t)PROJ * V_D); w.cls_b = take(PROJ);
    w.shift_w = take(V_D); w.shift_b = take(1);
    w.scale_w = take(V_D); w.scale_b = take(1);
    w.box0_w = take((size_t)V_D * V_D); w.box0_b = take(V_D);
    w.box1_w = take((size_t)V_D * V_D); w.box1_b = take(V_D);
    w.box2_w = take((size_t)4 * V_D); w.box2_b = take(4);
    w.box_bias = take((size_t)g.np * 4);
    if (g.family == 1) {
        w.obj0_w = take((size_t)V_D * V_D); w.obj0_b = take(V_D);
        w.obj1_w = take((size_t)V_D * V_D); w.obj1_b = take(V_D);
        w.obj2_w = take(V_D); w.obj2_b = take(1);
    }
}

template <class Take>
void map_text(TextW& w, Take&& take) {
    w.tok_emb = take((size_t)T_VOCAB * T_D);
    w.tpos_emb = take((size_t)T_LEN * T_D);
    for (int i = 0; i < T_LAYERS; ++i) map_layer(w.layers[i], T_D, T_FF, take);
    w.final_ln_w = take(T_D); w.final_ln_b = take(T_D);
    w.text_proj = take((size_t)PROJ * T_D);
}

}  // namespace tstar
