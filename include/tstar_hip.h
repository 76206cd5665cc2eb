/* tstar_hip.h -- C ABI of libtstar_hip.so: the MI355X (gfx950) implementation of the
 * T* keyframe-search hot path.
 *
 * The reference (mll-lab-nu/TStar) has NO native plug-in ABI: its plug-in surface is two
 * duck-typed Python classes, HeuristicInterface/OWLInterface
 * (TStar/interface_heuristic.py:28-37, 200-280) and TStarSearcher
 * (TStar/interface_searcher.py:14-538).  tstar_amd/ keeps that Python surface and binds
 * the entry points below with ctypes (tstar_amd/_lib.py); INTEGRATION.md shows the
 * binding a maintainer of the reference would add.  Each entry point names the reference
 * code it replaces.
 *
 * Conventions
 *   - plain C types only; "d_" pointers are DEVICE pointers (HBM) owned by the caller,
 *     "h_" pointers are host pointers; nothing is retained past the call unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     enqueued on it; no entry point synchronises unless stated.
 *   - return value 0 = OK; otherwise an error code (TSTAR_ERR_*), with a human-readable
 *     message from tstar_last_error() (thread-local).
 *   - integer/byte outputs are bit-exact restatements of the reference arithmetic;
 *     floating-point outputs match the CPU oracle within 1e-3 (observed ~1e-6).
 */
#ifndef TSTAR_HIP_H
#define TSTAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSTAR_OK 0
#define TSTAR_ERR_ARG 1
#define TSTAR_ERR_HIP 2
#define TSTAR_ERR_STATE 3

#define TSTAR_OWL_NPATCH 576   /* 24 x 24 patches of a 768 x 768 detector image */
#define TSTAR_OWL_QDIM 512
#define TSTAR_OWL_TEXT_LEN 16
#define TSTAR_OWL_MAX_QUERIES 32
#define TSTAR_OWL_MAX_SETS 64      /* independent query sets (questions) resident at once */

const char* tstar_last_error(void);
int tstar_abi_version(void);
/* number of float32 values expected in the vision / text weight blobs (layout:
 * tstar_amd/weights.py vision_spec()/text_spec(), mirrored in csrc/owl_weights.h) */
size_t tstar_owl_vision_blob_floats(void);
size_t tstar_owl_text_blob_floats(void);

/* ------------------------------------------------------------------ detector (D-rows) */
typedef struct tstar_owl tstar_owl;

/* Replaces OWLInterface.__init__/load_model_and_tokenizer + model.to(device)
 * (interface_heuristic.py:201-210).  Copies the float32 blobs to HBM and allocates the
 * activation workspace for `max_batch` detector images per pass (larger batches are
 * processed in chunks).  h_text_blob may be NULL (then only tstar_owl_set_query_embeds
 * can install queries).  h_norm_lut: 3*256 float32, the rescale+normalise value of every
 * (channel, u8) pair, computed by the host with the reference's arithmetic
 * (HF image_transforms.py rescale/normalize via image_processing_pil_owlvit.py).
 * weights_mode:
 *   TSTAR_WEIGHTS_F32 (0): float32 weights, exact-f32 MFMA (v_mfma_f32_32x32x2_f32) -- the reference's
 *     arithmetic and the mode every headline number is quoted in.
 *   TSTAR_WEIGHTS_BF16 (1) (BASELINE config 5, "bf16 ViT weights"): every GEMM weight matrix is also kept
 *     as bfloat16 (round to nearest even; exact if the blob already holds bf16 values) and the GEMMs run
 *     on the bf16 matrix pipe.  A bf16 weight is exact in ONE term; the float32 activations are carried as TWO
 *     round-to-nearest bf16 terms a_hi + a_lo (16 significand bits, |a - a_hi - a_lo| <= 2^-17 |a|):
 *     C += a_lo*w + a_hi*w, exact products, f32 accumulation -- 2 MFMA products per algorithmic product.
 *     Detector scores stay within 1e-3 of a float32 run on the same rounded weights (tests state the measured
 *     bound, ~1e-5).  The text tower is the exception: its GEMMs (once per query set, M <= 512 rows) run with the exact
 *     three-term split of mode 3 on the same bf16 plane, so the query embeddings, which enter every score, are the
 *     float32-class embeddings of the rounded checkpoint.  The vision tower's attention runs on the bf16 pipe as well in modes 1 and 3 (f32-split
 *     operands: two bf16 terms each, 3 products, f32 accumulation).
 *   (2, TSTAR_WEIGHTS_F32_SPLIT of ABI 2 -- both operands as two bf16 terms, 16 significand bits -- is retired and
 *     refused; TSTAR_WEIGHTS_F32X3 below carries all 24 bits.)
 *   TSTAR_WEIGHTS_BF16_EXACT (3): bf16 weights with the activations split EXACTLY into three bf16 terms
 *     (8 + 8 + 8 significand bits, truncation split; 3 MFMA products): the f32-accumulated product of the f32
 *     activations with the bf16 weights, f32-roundoff class (round 1-2's bf16 mode, kept selectable).
 *   TSTAR_WEIGHTS_F32X3 (4) (ABI 3): float32 checkpoints on the bf16 matrix pipe WITHOUT dropping an operand bit: every
 *     weight and every activation is split exactly into three round-to-nearest bfloat16 terms (8 + 8 + 8 significand
 *     bits, signed remainders; weights once at creation, packed in MFMA-fragment order, 6 bytes per weight) and
 *     C += a0 w2 + a1 w1 + a0 w1 + a2 w0 + a1 w0 + a0 w0 per K = 16 step -- the six partial products with ka + kw <= 2,
 *     each exact, f32 accumulation.  The three products left out are <= 2^-24 |a w| each and zero-mean; measured
 *     against float64 the result is no further away than the exact-f32 MFMA tile's (tests assert it on every shape
 *     they run; the nine-product form has the same error to four digits).  1.3-1.45x the f32 tile's rate on the batch
 *     shapes.  Attention, LayerNorm and the heads' tails stay float32.  Opt-in; the headline is quoted in mode 0.
 * ABI note (tstar_abi_version() == 3): since ABI 2 mode 1 means TWO-term activations (it was the exact three-term split,
 * now mode 3), TSTAR_OWL_MAX_SETS went 32 -> 64, mode 2 was retired and mode 4 added. */
#define TSTAR_WEIGHTS_F32 0
#define TSTAR_WEIGHTS_BF16 1
#define TSTAR_WEIGHTS_BF16_EXACT 3
#define TSTAR_WEIGHTS_F32X3 4
int tstar_owl_create(tstar_owl** out, const float* h_vision_blob, size_t n_vision,
                     const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch,
                     int weights_mode);
/* Added entries (tstar_abi_version() stays 3).  The same for a vision tower of patch geometry (image_size, patch_size):
 * (768, 32) = OWL-ViT B/32 (what tstar_owl_create builds: 24 x 24 = 576 patches, 577 tokens) or (768, 16) = B/16
 * (48 x 48 = 2304 patches, 2305 tokens, patch-embed K = 768); every other geometry is refused before anything is
 * allocated.  Both share every width (vision 768 / 3072 / 12 layers / 12 heads, the text tower, projection 512).  The
 * vision blob holds tstar_owl_vision_blob_floats_ex(image_size, patch_size) floats.  A forward runs in chunks of at most
 * 1024 images at B/32 and 256 at B/16 (no chunk holds more token rows than B/32's 1024 images, so every activation
 * workspace stays below 2^31 elements); a larger max_batch is accepted and its batches are scored chunk by chunk. */
int tstar_owl_create_ex(tstar_owl** out, int image_size, int patch_size, const float* h_vision_blob, size_t n_vision,
                        const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode);
/* floats of a vision blob of that geometry (0 if it is not supported) */
size_t tstar_owl_vision_blob_floats_ex(int image_size, int patch_size);
/* Added entries (tstar_abi_version() stays 3).  The same for a handle that runs its checkpoint at the INPUT SIZE (input_h,
 * input_w) pixels instead of the checkpoint's own 768 x 768 (HF: forward(..., interpolate_pos_encoding=True) behind an image
 * processor of that size): images are resampled (Pillow bicubic) to input_h x input_w, the patch grid is gh x gw = input_h / P x
 * input_w / P, np = gh gw detections and np + 1 tokens per image.  Each side must be a positive multiple of patch_size (32 or
 * 16) and np at most 3600; anything else is refused before anything is allocated.  The size is fixed for the handle's life.
 * The vision blob holds tstar_owl_vision_blob_floats_in(input_h, input_w, patch_size) floats: the layout of tstar_owl_create_ex
 * with pos_emb [np + 1, 768] (the checkpoint's table resampled to gh x gw, row 0 kept) and box_bias [np, 4] (for the gh x gw
 * grid) -- tstar_amd/weights.py pack_blob builds both as HF does.  (768, 768, P) is tstar_owl_create_ex(768, P): same bits.
 * A forward chunk never holds more token rows than 1024 images of 577 tokens. */
int tstar_owl_create_in(tstar_owl** out, int input_h, int input_w, int patch_size, const float* h_vision_blob, size_t n_vision,
                        const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode);
/* floats of a vision blob for that input size (0 if it is not supported) */
size_t tstar_owl_vision_blob_floats_in(int input_h, int input_w, int patch_size);
/* np, the detections per image of the handle's geometry (576 at B/32, 2304 at B/16, gh x gw at another input size; -1 for a
 * NULL handle) */
/* OWLv2 (an added entry; tstar_abi_version() stays 3).  tstar_owl_create_in for a model family: TSTAR_OWL_FAMILY_OWLVIT (0) IS
 * tstar_owl_create_in.  TSTAR_OWL_FAMILY_OWLV2 (1): an OWLv2 B/16 handle (checkpoint image 960, patch 16; patch_size must be 16; the
 * input size follows the same rule, default 960 x 960 = 3600 patches).  Its vision blob has the v2 layout -- the OWL-ViT layout followed
 * by the objectness head: obj0_w [768,768], obj0_b [768], obj1_w [768,768], obj1_b [768], obj2_w [768], obj2_b [1] --
 * tstar_owl_vision_blob_floats_family(1, ...) floats; its normalisation argument is mean[3], std[3] (float32) instead of the 3 x 256
 * table: pre-processing is HF's Owlv2ImageProcessorPil in float (pad to a square, Gaussian anti-aliasing, linear zoom, clip, normalise),
 * bit for bit; boxes are scaled by max(H, W) as HF's post-processing does.  Every refusal happens before anything is allocated. */
#define TSTAR_OWL_FAMILY_OWLVIT 0
#define TSTAR_OWL_FAMILY_OWLV2 1
int tstar_owl_create_family(tstar_owl** out, int family, int input_h, int input_w, int patch_size, const float* h_vision_blob,
                            size_t n_vision, const float* h_text_blob, size_t n_text, const float* h_norm, int max_batch,
                            int weights_mode);
size_t tstar_owl_vision_blob_floats_family(int family, int input_h, int input_w, int patch_size);
int tstar_owl_num_patches(tstar_owl* h);
int tstar_owl_destroy(tstar_owl* h);

/* Replaces the text half of processor(...)+model(...) that the reference recomputes on every
 * detector call (interface_heuristic.py:234,239 -> HF modeling_owlvit.py:945-958, 631-663):
 * runs the CLIP text tower once for Q queries (ids/mask int32 [Q,16]) and keeps the
 * L2-normalised query embeddings resident.  h_class_weight float64 [Q] = object2weight of each
 * query's name (interface_searcher.py:88-91,136; Python floats in the reference, and the
 * confidence score * weight is formed in float64 as under the reference's pinned numpy 1.26).  `query_set` (0..TSTAR_OWL_MAX_SETS-1) is the slot the queries are stored
 * in: several (video, question) items can be resident at once and every image of a tstar_owl_score call
 * names the slot it is scored against (the reference keeps exactly one query set, = slot 0).
 * Synchronises `stream`. */
int tstar_owl_set_queries(tstar_owl* h, int query_set, const int32_t* h_input_ids, const int32_t* h_attention_mask,
                          const double* h_class_weight, int Q, void* stream);
/* Several query sets in ONE text-tower forward (a lock-step group installs the questions of all its items at once): h_sets
 * [n_sets] slots, h_Q [n_sets] queries per set, ids / attention masks [sum Q][16] and class weights [sum Q] concatenated in
 * set order.  Same kernels as tstar_owl_set_queries on more rows; results are bit-identical to one call per set.  Synchronises. */
int tstar_owl_set_queries_many(tstar_owl* h, int n_sets, const int32_t* h_sets, const int32_t* h_Q, const int32_t* h_ids,
                               const int32_t* h_am, const double* h_w, void* stream);
/* Same, from precomputed L2-normalised embeddings float32 [Q,512] and query mask u8 [Q]. */
int tstar_owl_set_query_embeds(tstar_owl* h, int query_set, const float* h_query_embeds, const uint8_t* h_query_mask,
                               const double* h_class_weight, int Q, void* stream);
/* Replaces only the per-query class weights (TStarSearcher sets object2weight AFTER it has
 * reparameterised the heuristic, interface_searcher.py:87-91). */
int tstar_owl_set_class_weights(tstar_owl* h, int query_set, const double* h_class_weight, int Q, void* stream);
/* Copies the resident (L2-normalised, pre-class-head) query embeddings float32 [Q,512] to the host. */
int tstar_owl_get_query_embeds(tstar_owl* h, int query_set, float* h_out, int Q, void* stream);

/* Replaces OWLInterface.inference_detector (interface_heuristic.py:232-246: HF preprocess,
 * both towers' forward, post_process_grounded_object_detection(threshold=0.005)) AND the
 * detection->grid-cell loop of TStarSearcher.imageGridScoreFunction
 * (interface_searcher.py:129-150) for B images of identical size in one call.
 *   d_images      u8  [B,H,W,3] RGB (the grid image, or a verification frame)
 * np = tstar_owl_num_patches(h): 576 for a B/32 handle, 2304 for B/16; detections come in patch order.
 *   h_image_query_set  i32 [B] (host) query set of every image, or NULL (all images use set 0)
 *   d_scores      f32 [B,np]    sigmoid(max_q logit)            (dense: not thresholded)
 *   d_labels      i32 [B,np]    argmax_q logit
 *   d_boxes_xyxy  f32 [B,np,4]  pixels of the passed image
 *   d_cell_conf   f64 [B,rows*cols]  max over detections with score > 0.005 of
 *                                    float64(score) * class_weight[label], row-major cells; 0 if none
 *   d_cell_mask   u32 [B,rows*cols]  bit q set <=> a kept detection with label q fell in the cell
 *   d_n_kept      i32 [B]       number of detections with score > 0.005 (may be NULL)
 *   d_logits      f32 [B,np,Q]  raw logits (may be NULL; needs the same Q for every image)
 *   d_boxes_cxcywh f32 [B,np,4] pred_boxes (may be NULL)
 */
int tstar_owl_score(tstar_owl* h, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                    const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, double* d_cell_conf,
                    uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_boxes_cxcywh, void* stream);
/* Round 6 (an added entry point; tstar_abi_version() stays 3).  The same call on workspace `lane` (0 .. TSTAR_OWL_LANES - 1).  tstar_owl_score is lane 0, the handle's own workspace of
 * max_batch images.  Lane 1 is a second, SMALL workspace (forward chunks of min(max_batch, max(TSTAR_OWL_AUX_BATCH, B)) images; allocated on
 * first use and grown when a larger batch arrives, which synchronises the device once): a call on lane 1 shares no mutable state with a call on lane 0, so the two may be
 * enqueued on DIFFERENT streams and execute concurrently -- TStarSearcher queues the NEXT iteration's grid forward (one image: 120-456
 * wave tiles per GEMM for 1024 SIMDs) on lane 1 beside the verification batch of the iteration before (interface_searcher.py:444-491:
 * the loop the reference runs strictly one call after another).  Calls on ONE lane must stay ordered (one stream, or events), as
 * before.  Results do not depend on the lane: same kernels, same tile choices, same bits. */
#define TSTAR_OWL_LANES 2
#define TSTAR_OWL_AUX_BATCH 4
int tstar_owl_score_lane(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                         const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy,
                         double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits,
                         float* d_boxes_cxcywh, void* stream);

/* tstar_owl_score_lane with one more nullable output (an added entry): d_objectness f32 [B, np] = HF's objectness_logits of an OWLv2
 * handle (the objectness head: two GELU layers through the handle's GEMM path, then a 768-dot).  Computed only when the pointer is
 * non-NULL, after everything else, so no other output changes; TSTAR_ERR_ARG on an OWL-ViT handle.  NULL: tstar_owl_score_lane. */
int tstar_owl_score_lane_obj(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                             const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy,
                             double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits,
                             float* d_boxes_cxcywh, float* d_objectness, void* stream);

/* tstar_owl_score_lane_obj WITHOUT the box outputs, for images scored as a 1 x 1 grid (an added entry; tstar_abi_version() stays 3).
 * With one cell the boxes cannot reach cell_conf / cell_mask / n_kept: the cell of a detection is its clamped box centre's, which is
 * cell 0, and everything else comes from the class head.  That is the searcher's verification call: the reference's
 * verify_and_remove_target (TStar/interface_searcher.py:382-420) reads the detections' confidence and class names only.  The entry
 * skips the box head's two 768 x 768 GELU layers, the box tail of the row kernel and both box stores; the launches of the class head
 * are the same, so d_scores, d_labels, d_cell_conf, d_cell_mask, d_n_kept, d_logits and d_objectness hold the bits of the full entry
 * in every weights mode.  Arguments as tstar_owl_score_lane_obj minus d_boxes_xyxy and d_boxes_cxcywh; TSTAR_ERR_ARG (nothing
 * launched) when grid_rows * grid_cols != 1: a larger grid needs the box centres. */
int tstar_owl_score_cells(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                          const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, double* d_cell_conf,
                          uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_objectness, void* stream);

/* Frame records (added entries; tstar_abi_version() stays 3).  Everything a score call computes for an image up to the query loop
 * of its last kernel reads the image and the checkpoint only.  A RECORD keeps exactly that for the np patches of one image, in the
 * form the kernel holds before the loop, so that a later question about the same image costs a pass over the record instead of the
 * vision tower:
 *   cn  f32 [np][512]  the class-head row after the division by sqrt(sum) + 1e-6
 *   ss  f32 [np][2]    the shift branch, and the scale branch after ELU + 1
 *   box f32 [np][4]    the box head's sigmoid outputs cx, cy, w, h, relative (pixels are made at scoring time)
 * np * 518 * 4 bytes (1.19 MB at B/32 768 x 768); OWLv2's objectness is not recorded.  A handle owns at most one pool of records,
 * addressed by slot 0 .. n_slots - 1; which image lives in which slot is the caller's bookkeeping (tstar_amd.feature_cache).
 *
 * tstar_owl_records_frame_bytes: the bytes of one record of that geometry (arguments as tstar_owl_vision_blob_floats_family); pure, no
 *   GPU; 0 with an error for an unsupported geometry.  In the pool records lie that far apart, rounded up to 16 bytes.
 * tstar_owl_records_reserve: allocate the pool (zero-filled), once: it lives until tstar_owl_destroy.  A second call with the same
 *   n_slots does nothing; with another size it returns TSTAR_ERR_STATE.
 * tstar_owl_records_slots: the pool's slot count (0 before a pool is reserved).
 * tstar_owl_score_records: ONE path for hits and misses.  First the n_miss images d_miss_images u8 [n_miss,H,W,3] go through the
 *   forward in workspace `lane` (the usual chunks) and record i is written to slot h_miss_slots[i] (host, [n_miss]; any order, any
 *   gaps, all different).  Then B images are scored as a 1 x 1 grid FROM records: image b from slot h_slots[b] (host, [B]; a slot
 *   may repeat, and may be one just filled) against query set h_image_query_set[b] (host, [B], or NULL: set 0), boxes scaled to an
 *   image of box_w x box_h pixels as tstar_owl_score scales them to its (W, H).  Outputs as tstar_owl_score_cells, plus the nullable
 *   d_boxes_xyxy / d_boxes_cxcywh f32 [B,np,4]; every output holds the bits tstar_owl_score_lane_obj gives for the same images in the
 *   batch that filled their records.  n_miss may be 0 (d_miss_images and h_miss_slots may then be NULL); B may be 0 (records are
 *   filled, nothing is scored, the outputs may be NULL).  TSTAR_ERR_ARG, with nothing launched, for: a slot outside the pool,
 *   n_miss < 0, no pool, d_objectness != NULL, a query set without queries (the text of tstar_owl_score).
 * ORDER: the pool is one piece of mutable state.  All record calls of a handle must be ordered on ONE stream (or by events), whatever
 * their lane; a call on the other lane that does not touch records (tstar_owl_score_lane) may still run beside them. */
size_t tstar_owl_records_frame_bytes(int family, int input_h, int input_w, int patch_size);
int tstar_owl_records_reserve(tstar_owl* h, int n_slots);
int tstar_owl_records_slots(tstar_owl* h);
int tstar_owl_score_records(tstar_owl* h, int lane, const uint8_t* d_miss_images, int n_miss, int H, int W, const int32_t* h_miss_slots,
                            int B, const int32_t* h_slots, const int32_t* h_image_query_set, int box_w, int box_h, float* d_scores,
                            int32_t* d_labels, double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits,
                            float* d_objectness, float* d_boxes_xyxy, float* d_boxes_cxcywh, void* stream);

/* OWLv2 pre-processing policy (added entries; pure: no GPU, nothing launched).  plan10 = { form, tile_h, tile_w, win_h, win_w, LDS bytes
 * per workgroup, grid.x, grid.y, radius_y, radius_x } for a u8 image H x W resized to out_h x out_w (multiples of 16): form 0 = direct
 * (no axis shrinks: four taps per output pixel straight from the source), 1 = filtered (a workgroup owns tile_h x tile_w output pixels and
 * holds their source window, at most win_h x win_w samples, in LDS); radius = the Gaussian's radius per axis, -1 = the axis is skipped.
 * TSTAR_ERR_ARG where a score call would refuse the same image: the window of the smallest tile must fit 160 KiB of LDS.
 * tstar_owlv2_axis_window: the window [lo, lo + n) = lo_n2 of tile k of an axis (S = max(H, W) samples -> out, `tile` outputs per tile).
 * tstar_owlv2_axis_tables: the float64 tables of an axis as the kernels read them: taps (i0, i1, t) per output index and the Gaussian's
 * left half gw[radius - k] (k = distance from the centre; one entry 1.0 when the axis is skipped).
 * tstar_owlv2_set_axis_weights: install the Gaussian's left half (n = radius + 1 float64 values, gw[radius - k] for distance k) of the axis
 * (S -> out) of a handle, replacing the library's own (computed with libm's exp).  HF's processor computes them with numpy, whose exp can
 * differ from libm's in the last bit; tstar_amd.owl.OwlScorer installs numpy's before the first image of a new (S, out), so its
 * pre-processing has the processor's bits on the machine it runs on. */
int tstar_owlv2_set_axis_weights(tstar_owl* h, int S, int out, const double* gw, int n);
int tstar_owlv2_preprocess_plan(int H, int W, int out_h, int out_w, int* plan10);
int tstar_owlv2_axis_window(int S, int out, int tile, int k, int radius, int* lo_n2);
int tstar_owlv2_axis_tables(int S, int out, int32_t* i0, int32_t* i1, double* t, double* gw, int gw_cap);
/* the form (0 / 1) of the last OWLv2 pre-processing launch of `lane`, -1 before the first */
int tstar_owlv2_last_preprocess_form(tstar_owl* h, int lane);

/* Diagnostics for parity tests: the preprocessed u8 images (after bicubic; 768 x 768, or the handle's input_h x input_w)
 * and their patch-embed A operand can be read back.  d_out_patches is [B*np, 3*P*P] for the handle's
 * patch size P: [B*576, 3072] at B/32, [B*2304, 768] at B/16 (row b*np + (y/P)*G + x/P, column c*P*P + (y%P)*P + x%P). */
/* On an OWLv2 handle there is no u8 stage: d_out_u8 must be NULL (TSTAR_ERR_ARG otherwise); d_out_patches is [B*np, 768]. */
int tstar_owl_debug_preprocess(tstar_owl* h, const uint8_t* d_images, int B, int H, int W,
                               uint8_t* d_out_u8 /* [B,input_h,input_w,3] */, float* d_out_patches /* [B*np,3*P*P] */,
                               void* stream);

/* Diagnostics for kernel tests of the detector TAIL (everything after the encoder): the launchers tstar_owl_score runs, with the
 * same arguments, on caller-supplied device tensors.  Added entries (no ABI bump).
 *
 * tstar_owl_debug_heads: detect_rows on d_feats [B*np,768] (image feats after the detection LayerNorm), d_cls [B*np,512] (the class
 * head's dense0 output) and d_boxh [B*np,768] (the box head after dense1 + GELU), with the handle's head weights, box_bias, installed
 * query sets and masks; np = tstar_owl_num_patches(h).  (H, W): the image size the boxes are scaled to -- by (W, H) on an OWL-ViT
 * handle, by max(H, W) on both axes on an OWLv2 handle.  h_image_query_set (host, [B]), d_logits [B*np,Q] (needs one Q for every
 * image) and d_boxes_cxcywh [B*np,4] may be NULL.  d_obj_hidden [B*np,768] with d_objectness [B*np] (both or neither; OWLv2 handle
 * only): row_dot768 with the handle's objectness dense2.  B in 1..max_batch. */
int tstar_owl_debug_heads(tstar_owl* h, const float* d_feats, const float* d_cls, const float* d_boxh, int B, int H, int W,
                          const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, float* d_logits,
                          float* d_boxes_cxcywh, const float* d_obj_hidden, float* d_objectness, void* stream);
/* write_cls_rows (when write_cls != 0: token row 0 of every image = class embedding + position row 0, in place) and then
 * merge_cls_ln on d_x [B*ntok,768] (ntok = np + 1) with the handle's post-LayerNorm / detection-LayerNorm weights:
 * d_feats [B*np,768] = LN_det(LN_post(x[b,1+p]) * LN_post(x[b,0])).  B in 1..max_batch. */
int tstar_owl_debug_merge(tstar_owl* h, float* d_x, int B, int write_cls, float* d_feats, void* stream);
/* The vision tower's entry as the forward runs it, in lane 0's workspace (an added entry; tstar_abi_version() stays 3): the patch
 * embedding GEMM on d_patches [B*np, patch_k] (the handle's weight plane of its weights mode, its -- possibly resampled -- position
 * table, token rows 1..np of every image), then write_cls_rows (token row 0).  stage 0 stops there; stage 1 also runs the
 * pre-LayerNorm IN PLACE, as the forward does.  The token rows are copied to d_x [B*ntok, 768].  B in 1..the images of one forward
 * chunk (min(max_batch, chunk limit)); any other stage is refused. */
int tstar_owl_debug_embed(tstar_owl* h, const float* d_patches, int B, int stage, float* d_x, void* stream);
/* The text tower as tstar_owl_set_queries runs it, in the handle's workspace, WITHOUT installing a query set (an added entry;
 * tstar_abi_version() stays 3).  h_ids, h_am: HOST [Q,16] as for tstar_owl_set_queries.  stage 0: h_out (HOST) [Q*16, 512] = the token +
 * position embedding rows; stage 1: h_out [Q, 512] = the rows of the final LayerNorm at every sequence's first maximum id (what the
 * text projection reads).  Refuses what tstar_owl_set_queries refuses, and any other stage.  Synchronises the stream. */
int tstar_owl_debug_text(tstar_owl* h, const int32_t* h_ids, const int32_t* h_am, int Q, int stage, float* h_out, void* stream);
/* cell_reduce without a handle: d_scores [B,np], d_labels [B,np] (0..31; rows with score <= thr are not read), d_boxes_xyxy [B,np,4]
 * -> d_cell_conf f64 [B,rows*cols], d_cell_mask u32 [B,rows*cols], d_n_kept [B] exactly as tstar_owl_score writes them.
 * h_weights: HOST float64 [n_sets,32] class weights; h_image_set: HOST [B] weight row of every image, or NULL (row 0).  W, H: the
 * image size in pixels.  At most 4096 cells.  Synchronises the stream.  Box centres are >= 0 (a sigmoid times a size). */
int tstar_cell_reduce(const float* d_scores, const int32_t* d_labels, const float* d_boxes_xyxy, const double* h_weights, int n_sets,
                      const int32_t* h_image_set, int B, int np, int W, int H, int grid_rows, int grid_cols, float thr,
                      double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, void* stream);

/* Image-guided (one-shot) queries (added entries; tstar_abi_version() stays 3): HF's image_guided_detection up to the query vector,
 * OwlViTForObjectDetection.embed_image_query (Owlv2ForObjectDetection's is the same statements).  An example image is pre-processed
 * and run through the vision tower exactly like a target image; with class_embeds [np,512] (the class head's dense0 output, not
 * normalised) and pred_boxes [np,4] (cxcywh): IoU of every box with the unit box [0,0,1,1] in float32 (generalized IoU instead when
 * EVERY IoU is 0), thr = max * 0.8, the selected rows are those with value >= thr; among them the one whose class embedding has the
 * smallest dot product with the mean class embedding of ALL rows (lowest index on a tie) is the query: class_embeds[best].  Install it
 * with tstar_owl_set_query_embeds (which normalises by ||.|| + 1e-6 as the class head does) with query mask 1.
 *
 * tstar_owl_embed_image_queries: d_images u8 [n,H,W,3] on the device -> HOST arrays h_embeds f32 [n,512], h_best i32 [n] (row of the
 * chosen patch), h_boxes_cxcywh f32 [n,4] (its pred_box: the bits tstar_owl_score returns as d_boxes_cxcywh for that image),
 * h_n_selected i32 [n], h_status i32 [n]: 0 = IoU, 1 = the GIoU fallback was used, 2 = empty selection (the largest GIoU is negative;
 * HF produces no query for such an image): embedding and box zeros, best -1, and the call still returns TSTAR_OK.  Runs in lane 0 (as
 * the text tower does; keep it ordered with lane-0 score calls) in chunks of the handle's chunk limit; OWL-ViT and OWLv2 handles,
 * any input size, every weights mode; installed queries are not touched.  Refuses bad arguments before anything is launched.
 * Synchronises the stream.
 *
 * tstar_image_query_select: the selection alone, without a handle, on caller tensors d_cls f32 [n*np,512] (16-byte aligned) and
 * d_boxes_cxcywh f32 [n*np,4] (w, h >= 0, no NaN), np in 1..3600; the launcher tstar_owl_embed_image_queries calls.  One workgroup
 * per image; image i reads rows i*np .. (i+1)*np - 1 and nothing else.  Synchronises the stream. */
int tstar_owl_embed_image_queries(tstar_owl* h, const uint8_t* d_images, int n, int H, int W, float* h_embeds, int32_t* h_best,
                                  float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream);
int tstar_image_query_select(const float* d_cls, const float* d_boxes_cxcywh, int n, int np, float* h_embeds, int32_t* h_best,
                             float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream);

/* Query boxes (added entries; tstar_abi_version() stays 3): the same selection against a per-example query box instead of the unit
 * box -- "this region of the example" -- with HF's box_iou / generalized_box_iou in their general form: area_q = (x1-x0)(y1-y0),
 * inter from max of the top-left and min of the bottom-right corners clamped at 0, union = (area_q + area_p) - inter, iou = inter /
 * union; the GIoU fallback uses the enclosing box of the two.  Boxes are (x0, y0, x1, y1), relative, float32.
 * tstar_image_query_select_box: tstar_image_query_select plus d_boxes_q f32 [n,4] on the DEVICE (NULL: unit boxes).
 * tstar_owl_embed_image_queries_box: tstar_owl_embed_image_queries plus h_query_boxes f32 [n,4] on the HOST (NULL: unit boxes).
 * With NULL or unit boxes both return the bits of the entries above, which are calls of these with NULL. */
int tstar_owl_embed_image_queries_box(tstar_owl* h, const uint8_t* d_images, int n, int H, int W, const float* h_query_boxes,
                                      float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status,
                                      void* stream);
int tstar_image_query_select_box(const float* d_cls, const float* d_boxes_cxcywh, const float* d_boxes_q, int n, int np, float* h_embeds,
                                 int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream);

/* HF's post_process_image_guided_detection (added entries; tstar_abi_version() stays 3), bit for bit in float32.  Per image:
 * d_scores f32 [B,np] (the sigmoid of the max logit over the queries: what tstar_owl_score returns as d_scores), d_boxes_cxcywh
 * f32 [B,np,4] (relative) -> d_alphas f32 [B,np], d_boxes_xyxy f32 [B,np,4] (corners cx -+ 0.5 w, cy -+ 0.5 h, scaled by (sx, sy, sx,
 * sy)), d_keep u8 [B,np] (alpha > 0; HF returns these rows, in patch order), d_n_kept i32 [B].  When nms_threshold < 1: greedy NMS in
 * descending score order (equal scores: lowest index first; torch's argsort leaves ties open), a candidate with score 0 is skipped, a
 * live candidate i zeroes every j != i with inter / ((area_i + area_j) - inter) > nms_threshold (a NaN IoU suppresses nothing).  An
 * image with no non-zero score left has all-zero alphas and keeps nothing (HF drops it from its result list; here its entry is
 * empty).  Otherwise scores < threshold become 0, m = max + 1e-6f, alpha = clip((s - m * 0.1f) / (m * 0.9f), 0, 1).
 * h_scale_xy: HOST f32 [B,2] (sx, sy) per image, or NULL (no scaling, HF's target_sizes=None; the call is then asynchronous,
 * otherwise it synchronises the stream).  One workgroup per image, no atomics; np in 1..3600, TSTAR_ERR_ARG beyond with nothing
 * launched.  tstar_image_guided_postprocess_host: the same statements on HOST arrays (no device is touched), scale_xy NULL or [B,2]. */
int tstar_image_guided_postprocess(const float* d_scores, const float* d_boxes_cxcywh, int B, int np, float threshold, float nms_threshold,
                                   const float* h_scale_xy, float* d_alphas, float* d_boxes_xyxy, uint8_t* d_keep, int32_t* d_n_kept,
                                   void* stream);
int tstar_image_guided_postprocess_host(const float* scores, const float* boxes_cxcywh, int B, int np, float threshold, float nms_threshold,
                                        const float* scale_xy, float* alphas, float* boxes_xyxy, uint8_t* keep, int32_t* n_kept);

/* ------------------------------------------------------------------ second detector backend: YOLO-World (D13)
 * Replaces YoloWorldInterface (interface_heuristic.py:39-190; wired at TStarFramework.py:178-184) -- the mmdet test
 * pipeline (keep-ratio resize to 640, letterbox pad 114, /255, channel swap), model.test_step (YOLOv8 CSPDarknet,
 * text-guided PAFPN, BN-contrastive head, DFL decode, class-aware NMS) and the wrapper's `score > 0.12`, top-50
 * (:148-152) -- with f32 VALU kernels (no MFMA, BASELINE configs[3]).  The model source is NOT in the reference tree
 * (dangling symlink): the architecture is restated from the published design, parity against the real model is
 * UNPINNED; oracle/yolo_ref.py is the independent CPU statement the tests compare against.
 *
 * The network is handed over as data (tstar_amd/yolo_world.py build_program): a float32 blob (BatchNorm folded), a
 * table of ops [n_ops][24] int32 over NHWC buffers [n_bufs][3] = (H, W, C), the max-sigmoid attention layers
 * [n_guides][5] = (embed, heads, guide_fc weight / bias offsets, per-head bias offset) and the head levels
 * [n_levels][8] = (embedding buffer, DFL buffer, map size, stride, offset of (exp(logit_scale), bias), 0, 0, 0).
 *
 * The words of an op (csrc/yolo_program.h is the definition, W_* in tstar_amd/yolo_world.py the mirror; unused words are 0):
 *   word        0  1    2        3      4    5        6       7      8       9    10     11     12    13   14
 *   conv        0  src  src_off  cin    dst  dst_off  cout    ks     stride  act  w_off  b_off  mode  aux  aux_off
 *   pool 5x5    1  buf  src_off  C      buf  dst_off
 *   up-copy     2  src  src_off  C      dst  dst_off  factor
 *   attention   3  src  src_off  embed  dst  0        heads   guide
 * src / dst / buf / aux are buffer indices, the offsets channel offsets inside them (channel concatenation is free), w_off / b_off float
 * offsets into the blob (weights [cout][ks][ks][cin]; b_off < 0: no bias).  conv: ks 1 | 3, stride 1 | 2, pad ks / 2, act 0 none | 1 SiLU,
 * mode 0 plain | 1 + residual read at channel aux_off of buffer aux | 2 * gate, buffer aux being [.., heads] (aux_off 0).  pool: 5 x 5 /
 * stride 1 max pool in place.  up-copy: factor 1 copies, 2 upsamples (nearest).  attention: the max-sigmoid gate of attention layer
 * `guide` (whose embed and heads words 3 and 6 repeat), one row of heads per source pixel into buffer dst.
 * tstar_yolo_create refuses, as "malformed op N" plus the reason, every op the kernels cannot serve; a buffer must hold fewer than 2^31
 * pixels at max_batch images. */
typedef struct tstar_yolo tstar_yolo;
int tstar_yolo_create(tstar_yolo** out, const float* h_blob, size_t n_blob, const int32_t* h_ops, int n_ops, int op_words,
                      const int32_t* h_bufs, int n_bufs, const int32_t* h_guides, int n_guides, const int32_t* h_levels,
                      int n_levels, int input_buf, int max_batch);
/* Diagnostic (an added entry; tstar_abi_version() stays 3): every check tstar_yolo_create makes of its arguments, without a GPU and
 * without creating anything.  TSTAR_OK, or TSTAR_ERR_ARG with the message tstar_yolo_create would give. */
int tstar_yolo_check_program(const float* h_blob, size_t n_blob, const int32_t* h_ops, int n_ops, int op_words, const int32_t* h_bufs,
                             int n_bufs, const int32_t* h_guides, int n_guides, const int32_t* h_levels, int n_levels, int input_buf,
                             int max_batch);
int tstar_yolo_destroy(tstar_yolo* h);
int tstar_yolo_num_anchors(tstar_yolo* h);
/* model.reparameterize(texts) (interface_heuristic.py:93): the cached CLIP text features float32 [Q,512] of query set
 * `query_set` (as the text backbone returns them: L2-normalised) + the searcher's class weights float64 [Q].  Synchronises. */
int tstar_yolo_set_text_feats(tstar_yolo* h, int query_set, const float* h_text, const double* h_class_weight, int Q, void* stream);
int tstar_yolo_set_class_weights(tstar_yolo* h, int query_set, const double* h_class_weight, int Q, void* stream);
/* inference_detector (:136-168) for B equally sized images u8 [B,H,W,3] (+ the searcher's detection -> cell loop,
 * interface_searcher.py:129-150, when d_cell_conf is given):
 *   d_det_scores f32 [B,max_dets], d_det_labels i32 [B,max_dets] (-1 = empty), d_det_boxes f32 [B,max_dets,4] xyxy pixels of
 *   the passed image, descending score; d_n_det i32 [B]; d_cell_conf f64 / d_cell_mask u32 [B,rows*cols] (may both be NULL);
 *   d_dense_scores f32 [B,8400,Q] / d_dense_boxes f32 [B,8400,4] (diagnostics, may be NULL). */
int tstar_yolo_detect(tstar_yolo* h, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                      const int32_t* h_image_query_set, float score_threshold, int max_dets, float* d_det_scores,
                      int32_t* d_det_labels, float* d_det_boxes, int32_t* d_n_det, double* d_cell_conf, uint32_t* d_cell_mask,
                      float* d_dense_scores, float* d_dense_boxes, void* stream);
/* Diagnostic (an added entry; tstar_abi_version() stays 3): the tail of tstar_yolo_detect -- DFL decode + contrastive scores + candidate
 * collection per head level, the nms_pre cut / sort / class-aware NMS / wrapper threshold / top-k, the dense copies and the
 * cell loop; the same launch sequence, one internal function -- on caller-supplied head tensors instead of the network's:
 * HOST arrays of n_levels DEVICE pointers, level l holding the embedding f32 [B * size_l^2, 512] and the DFL logits
 * f32 [B * size_l^2, 64] (side * 16 + bin; sides left, top, right, bottom), rows in image-major, row-major anchor order.
 * n_levels must equal the handle's; H, W only set the letterbox geometry and the clamp.  Everything else as in detect. */
int tstar_yolo_postprocess(tstar_yolo* h, const float* const* d_level_embed, const float* const* d_level_dfl, int n_levels, int B, int H,
                           int W, int grid_rows, int grid_cols, const int32_t* h_image_query_set, float score_threshold, int max_dets,
                           float* d_det_scores, int32_t* d_det_labels, float* d_det_boxes, int32_t* d_n_det, double* d_cell_conf,
                           uint32_t* d_cell_mask, float* d_dense_scores, float* d_dense_boxes, void* stream);

/* Diagnostics (added entries; tstar_abi_version() stays 3): the layer ops of a handle on caller data.  A handle's program may be any op
 * table tstar_yolo_create accepts (tests hand it crafted single-op programs); these entries run the code tstar_yolo_detect runs.
 * tstar_yolo_buffer_copy copies B images' worth of floats (B * H * W * C of activation buffer `buf`, NHWC) between d_data (device) and the
 * buffer: to_buffer != 0 writes the buffer, 0 reads it; 1 <= B <= max_batch, so the zero quad kept behind every buffer is out of reach.
 * Enqueues only.
 * tstar_yolo_run_ops runs the op table on the buffers as they stand (no preprocessing, no tail) for images 0 .. B - 1
 * (1 <= B <= max_batch), with the per-image query sets of tstar_yolo_detect (read only when the program has attention layers);
 * h_forms (host int32 [n_ops] or null) receives, per conv op, the kernel form that was launched (-1 for the other ops) -- the value the
 * launcher switched on.  Synchronises. */
#define TSTAR_YOLO_FORM_TILE64 0   /* LDS-tiled, 64 pixels x 64 channels per workgroup */
#define TSTAR_YOLO_FORM_TILE128 1  /* LDS-tiled, 128 pixels x 64 channels */
#define TSTAR_YOLO_FORM_WIDE 2     /* LDS-tiled, 128 pixels x 128 channels */
#define TSTAR_YOLO_FORM_SW8 3      /* scalar weights, 8 pixels per lane */
#define TSTAR_YOLO_FORM_SW4 4      /* scalar weights, 4 pixels per lane */
#define TSTAR_YOLO_FORM_HALO_A16 5 /* halo tile, 8 x 40 patches, 16 channels per wave */
#define TSTAR_YOLO_FORM_HALO_A8 6  /* halo tile, 8 x 40 patches, 8 channels per wave */
#define TSTAR_YOLO_FORM_HALO_B16 7 /* halo tile, 16 x 20 patches over the row-stacked batch, 16 channels per wave */
#define TSTAR_YOLO_FORM_HALO_B8 8  /* halo tile, 16 x 20 patches over the row-stacked batch, 8 channels per wave */
#define TSTAR_YOLO_FORM_DIRECT 9   /* direct small-K form */
int tstar_yolo_buffer_copy(tstar_yolo* h, int buf, float* d_data, int B, int to_buffer, void* stream);
int tstar_yolo_run_ops(tstar_yolo* h, int B, const int32_t* h_image_query_set, int32_t* h_forms, void* stream);
/* The launch plan of one conv op (pure: needs no GPU and launches nothing): a k x k / stride conv (pad k / 2) reading cin channels at
 * src_off of an H x W x src_ld buffer, writing cout channels at dst_off of a dst_ld-channel buffer, for B images of a handle created with
 * max_batch; mode 0 plain / 1 residual / 2 gate.  env_policy 0: the default policy; 1: with the TSTAR_YOLO_* overrides of this process (read
 * once).  plan3 = { form, mt, nt }: mt x nt workgroups of 256 threads (direct form: mt blocks of nt threads).  TSTAR_ERR_ARG where the
 * launcher refuses the layer. */
int tstar_yolo_conv_plan(int cin, int src_ld, int src_off, int H, int W, int cout, int dst_ld, int dst_off, int ks, int stride, int mode, int B,
                         int max_batch, int env_policy, int* plan3);

/* ------------------------------------------------------------------ ingest (S1-S3, S8) */
/* The resident decoded video d_video is u8 [N,H,W,3] RGB (nv12 = 0) or NV12 u8 [N, H*3/2, W] (nv12 = 1:
 * luma plane + interleaved half-resolution UV plane, converted on the fly, BT.601 limited range, nearest
 * chroma -- half the bytes per frame).
 * Replaces read_frame_batch + cv2.resize(800x380) + create_image_grid's cv2.resize(200x95) +
 * hstack/vstack (interface_searcher.py:157-169, 362, 186-188): gathers rows*cols frames by index
 * and writes the grid image u8 [rows*95, cols*200, 3]. */
int tstar_frames_to_grid(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx,
                         int grid_rows, int grid_cols, uint8_t* d_grid, int nv12, void* stream);
/* Replaces read_frame_batch + cv2.resize (interface_searcher.py:402-403; any target size):
 * out u8 [n,out_h,out_w,3]. */
int tstar_frames_resize(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n,
                        int out_w, int out_h, uint8_t* d_out, int nv12, void* stream);
/* Decode front end for RAW 4:2:0 containers (compressed streams need rocDecode / FFmpeg, which this
 * build does not have): n planar I420 frames (Y, U, V planes back to back, H*W*3/2 bytes each) already copied to the
 * device -> the resident NV12 store layout u8 [n, H*3/2, W] the ingest kernels read.  Replaces the decode half of
 * read_frame_batch (interface_searcher.py:157-169) for such files. */
int tstar_i420_to_nv12(const uint8_t* d_i420, int n, int H, int W, uint8_t* d_nv12, void* stream);
/* Decode front end for JPEG frames (Motion-JPEG AVI / .mjpeg streams, folders of .jpg): replaces the decode half of
 * read_frame_batch (interface_searcher.py:157-169) for such files.  Baseline / extended sequential Huffman, 8-bit, one
 * interleaved scan, grayscale or YCbCr with luma sampling 1x1, 2x1 or 2x2 (hs, vs) and chroma 1x1.  The entropy stage runs
 * on the host (serial per scan), everything after it on the device; the result is byte-equal to libjpeg-turbo's default
 * decode (accurate integer IDCT, fancy upsampling).  The host entries touch no HIP state and work without a device.
 *
 * Frame status / return value of tstar_jpeg_probe: 0 decodable here, 1 malformed or truncated, 2 a JPEG this decoder does
 * not cover (progressive, arithmetic, CMYK, other sampling: hand it to a general decoder), 3 geometry differs from the batch.
 * Layouts for a geometry (W, H, ncomp, hs, vs): coefficients int16 [blocks][64] in natural order, component after
 * component, block-raster within the component, padded to whole MCUs; tables u16 [3][64] per frame, natural order. */
/* Header walk: info5 = {W, H, ncomp, hs, vs}. */
int tstar_jpeg_probe(const uint8_t* data, size_t len, int32_t* info5);
/* One past the EOI of the JPEG starting at data[pos], by walking marker segments and the stuffed entropy data; 0 if broken. */
size_t tstar_jpeg_frame_end(const uint8_t* data, size_t len, size_t pos);
/* out2 = {blocks per frame, bytes of the per-frame plane workspace}. */
int tstar_jpeg_sizes(int W, int H, int ncomp, int hs, int vs, size_t* out2);
/* Threads a batch uses: min(16, CPUs the process may run on, asked when > 0). */
int tstar_jpeg_threads(int asked);
/* Entropy-decode n independent frames on a thread pool into caller memory (pinned for the device path): coef int16
 * [n][blocks][64], quant u16 [n][3][64], status i32 [n].  Returns 0 when every frame decoded, else TSTAR_ERR_STATE with the
 * first failing frame's message in tstar_last_error(); never reads or writes outside the given buffers. */
int tstar_jpeg_entropy_batch(const uint8_t* const* datas, const size_t* lens, int n, int W, int H, int ncomp, int hs, int vs,
                             int16_t* coef, uint16_t* quant, int threads, int32_t* status);
/* Scalar host reference of tstar_jpeg_reconstruct (same integers): rgb u8 [n,H,W,3] in host memory. */
int tstar_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* quant, int n, int W, int H, int ncomp, int hs, int vs,
                                uint8_t* rgb, int threads);
/* Device stage: dequantise + inverse DCT + range limit -> u8 planes (d_planes: n * plane-workspace bytes), then chroma
 * upsampling + YCbCr -> RGB into d_rgb u8 [n,H,W,3] (typically store[s0 : s0 + n]).  d_coef / d_quant 16-byte aligned. */
int tstar_jpeg_reconstruct(const int16_t* d_coef, const uint16_t* d_quant, int n, int W, int H, int ncomp, int hs, int vs,
                           uint8_t* d_planes, uint8_t* d_rgb, void* stream);
/* ---- Baseline JPEG ENCODE: RGB u8 frames -> the bytes Pillow's Image.fromarray(frame).save(buf, "JPEG", quality=q, subsampling=s)
 * writes, for quality 1..100 and luma sampling (hs, vs) = (2,2) 4:2:0, (2,1) 4:2:2, (1,1) 4:4:4.  Two stages share the decoder's
 * coefficient layout (above, 3 components): frames -> int16 coefficients, coefficients -> the stuffed bytes of the scan (from
 * behind SOS to EOI).  The header (SOI .. SOS, 623 bytes) is the same for every frame of a call.  Per-frame status: 0 written,
 * 1 the slot is too short (nothing of the frame is written; its length is then a lower bound), 2 a coefficient no 8-bit baseline
 * JPEG can code.  The _host entries touch no HIP state.  counters (optional, u64 [5], added to): ZRL symbols, blocks without
 * EOB, stuffed bytes, right-edge dummy blocks, bottom-edge dummy blocks. */
/* Pure plan for n frames whose scans go into slots of slot_bytes: out8 = {blocks per frame, coefficient bytes per frame, bytes
 * that hold any scan (2 * ceil(blocks * 1660 / 8) + 2: the longest codes everywhere, every byte stuffed, EOI), header bytes,
 * workspace bytes, workgroups of the block stage, workgroups per frame of the entropy stage, of the stuffing passes}. */
int tstar_jpeg_encode_plan(int W, int H, int hs, int vs, int n, size_t slot_bytes, size_t* out8);
/* SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS -> out (cap bytes), *len = 623.  TSTAR_ERR_ARG / 4 (cap short, nothing written). */
int tstar_jpeg_encode_header(int W, int H, int quality, int hs, int vs, uint8_t* out, size_t cap, size_t* len);
/* Block stage on the host: frames u8 [N,H,W,3], idx i32 [n] -> coef int16 [n][blocks][64]; quant (optional) u16 [3][64]. */
int tstar_jpeg_encode_blocks_host(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                                  int16_t* coef, uint16_t* quant, int threads, uint64_t* counters);
/* Scan stage on the host: coef -> out u8 [n][slot_bytes], lengths u32 [n], status i32 [n]. */
int tstar_jpeg_encode_scan_host(const int16_t* coef, int n, int W, int H, int hs, int vs, uint8_t* out, size_t slot_bytes,
                                uint32_t* lengths, int32_t* status, int threads, uint64_t* counters);
/* Whole files on the host (header + scan) into slots of slot_bytes; never writes past a slot, a short slot is left as it was. */
int tstar_jpeg_encode_host(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                           uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads, uint64_t* counters);
/* Block stage on the device: d_frames u8 [N,H,W,3] (a resident store), d_idx i32 [n] device memory (read in place, no staging
 * copy; an index outside 0..N-1 is clamped) -> d_coef (16-byte aligned); h_quant (optional, HOST) u16 [3][64]. */
int tstar_jpeg_encode_blocks(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                             int16_t* d_coef, uint16_t* h_quant, void* stream);
/* Scan stage on the device: d_coef -> d_out u8 [n][slot_bytes], d_lengths u32 [n], d_status i32 [n]; d_workspace: 16-byte
 * aligned device memory of the plan's workspace bytes.  Nothing is written past a slot; no host synchronisation. */
int tstar_jpeg_encode_scan(const int16_t* d_coef, int n, int W, int H, int hs, int vs, uint8_t* d_out, size_t slot_bytes,
                           uint32_t* d_lengths, int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Both stages: frames by index -> scans, lengths, status (d_coef: n * coefficient bytes of scratch). */
int tstar_jpeg_encode(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                      int16_t* d_coef, uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths, int32_t* d_status, void* d_workspace,
                      size_t workspace_bytes, void* stream);
/* ---- The same encoder with RESTART INTERVALS: what Pillow writes with restart_marker_blocks= / restart_marker_rows=.  restart is
 * the interval in MCUs, 0..65535 (0: none; the entries above are these with 0: the same bytes from the same launches).  With an
 * interval the header carries DRI (FF DD 00 04 hi lo) directly before SOS (629 bytes), and behind every full interval but the
 * last the scan fills the current byte with one-bits (a byte that becomes 0xFF is stuffed like any other), holds RSTn (FF D0 +
 * n mod 8, never stuffed) and starts every DC predictor from 0; an interval of at least the frame's MCUs writes DRI and no
 * marker.  Restart counters of their own (optional, added to; u64 [3] on the host, u32 [n][3] per frame on the device, zeroed by
 * the call): markers, intervals in front of a marker that ended byte-aligned, padded bytes that came out as 0xFF (on the device
 * the last is counted by the stuffing pass, so it stays 0 for a frame that pass never visits: one far too large for its slot). */
/* out8 as tstar_jpeg_encode_plan with the bound on a scan grown by 4 bytes per marker (the padding adds less than one data
 * byte, which stuffing can double; the marker's two bytes are never stuffed) and the workspace by the interval tables;
 * out2 (optional) = {interval, markers per frame = (MCUs - 1) / interval}. */
int tstar_jpeg_encode_plan_rst(int W, int H, int hs, int vs, int n, size_t slot_bytes, int restart, size_t* out8, size_t* out2);
int tstar_jpeg_encode_header_rst(int W, int H, int quality, int hs, int vs, int restart, uint8_t* out, size_t cap, size_t* len);
int tstar_jpeg_encode_scan_host_rst(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, int threads, uint64_t* counters, uint64_t* rst_counters);
int tstar_jpeg_encode_host_rst(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                               int restart, uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads,
                               uint64_t* counters, uint64_t* rst_counters);
/* d_workspace: the bytes tstar_jpeg_encode_plan_rst names for this interval; d_rst_counters: optional device u32 [n][3]. */
int tstar_jpeg_encode_scan_rst(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* d_out, size_t slot_bytes,
                               uint32_t* d_lengths, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                               uint32_t* d_rst_counters, void* stream);
int tstar_jpeg_encode_rst(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                          int restart, int16_t* d_coef, uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths, int32_t* d_status,
                          void* d_workspace, size_t workspace_bytes, uint32_t* d_rst_counters, void* stream);
/* ---- The same encoder with OPTIMISED HUFFMAN TABLES: what Pillow writes with optimize=True (libjpeg's optimize_coding), with or
 * without a restart interval.  Every frame is coded with four tables built from its own symbol counts (jchuff.c: the counts of
 * encode_mcu_gather, the tables of jpeg_gen_optimal_table), so the header differs from frame to frame in content and in length:
 * its four DHT segments (DC 0, AC 0, DC 1, AC 1, a segment each, all four always) carry the frame's tables.  A table travels as a
 * SPEC of 276 bytes: bits u8 [16] (codes of length 1..16), vals u8 [256] (the first nvals are the symbols), nvals u16, status u16
 * (0 ok; 1 a code longer than 32 bits before limiting, libjpeg's JERR_HUFF_CLEN_OVERFLOW; 2 no symbol).  Per-frame status 3: one of
 * the frame's tables overflowed; nothing of the frame is written and its length is 0.  A block is bounded by 1665 bits (a DC code
 * may be 16 bits long), which the plan's sizes hold.  The entries above are untouched: the same bytes from the same launches. */
/* optimize 0 / 1.  out8, out2 as tstar_jpeg_encode_plan_rst (optimize = 1: the larger bound, the longest header 1299 / 1305, the
 * workspace grown by the counts and the code tables); out3 (optional) = {optimize, byte offset in the workspace of the counts
 * u32 [n][4][257] (tables in DHT order; [256] stays 0), byte offset of the code tables [n][4] {u16 code [256], u8 len [256]}}: both
 * hold the last call's values when tstar_jpeg_encode_scan_opt returns. */
int tstar_jpeg_encode_plan_opt(int W, int H, int hs, int vs, int n, size_t slot_bytes, int restart, int optimize, size_t* out8, size_t* out2,
                               size_t* out3);
/* The table procedure alone, pure: freq u32 [256] (sum at most 1000000000) -> spec (276 bytes, above), code u16 [256] and len u8 [256]
 * (optional: the canonical codes; len 0 = no code), steps (optional: how often the limiting to 16 bits ran). */
int tstar_jpeg_huff_optimal(const uint32_t* freq, uint8_t* spec, uint16_t* code, uint8_t* len, int32_t* steps);
/* The header of one frame from its four specs (4 x 276 bytes, each with status 0) -> out, *len (at most 1299, 1305 with DRI). */
int tstar_jpeg_encode_header_opt(int W, int H, int quality, int hs, int vs, int restart, const uint8_t* specs, uint8_t* out, size_t cap,
                                 size_t* len);
/* Scan stage on the host with optimised tables: as tstar_jpeg_encode_scan_host_rst; specs u8 [n][4][276] out; hist (optional) u32
 * [n][4][257] out, the counts. */
int tstar_jpeg_encode_scan_host_opt(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, uint8_t* specs, uint32_t* hist, int threads, uint64_t* counters,
                                    uint64_t* rst_counters);
/* Whole files on the host with optimised tables (each frame's own header + scan), as tstar_jpeg_encode_host_rst. */
int tstar_jpeg_encode_host_opt(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                               int restart, uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads,
                               uint64_t* counters, uint64_t* rst_counters);
/* Scan stage on the device with optimised tables: counts -> tables -> the launches of tstar_jpeg_encode_scan_rst coding with the
 * frame's tables; nothing is read back in between.  d_specs: device u8 [n][4][276] out; d_workspace: the bytes
 * tstar_jpeg_encode_plan_opt names with optimize = 1. */
int tstar_jpeg_encode_scan_opt(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* d_out, size_t slot_bytes,
                               uint32_t* d_lengths, int32_t* d_status, uint8_t* d_specs, void* d_workspace, size_t workspace_bytes,
                               uint32_t* d_rst_counters, void* stream);
/* The two stages in front of that scan alone, for tests and measurements: stages 1 the counts (zeroed, then gathered), 2 the tables
 * from the counts as they lie in the workspace (so a caller may put counts of its own there), 3 both.  slot_bytes: the value the
 * workspace was planned with (it places the counts and the code tables). */
int tstar_jpeg_encode_tables(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, size_t slot_bytes, int stages,
                             uint8_t* d_specs, void* d_workspace, size_t workspace_bytes, void* stream);
/* Entropy stage on the device.  The unit of parallel work is a SEGMENT: a run of MCUs that starts at a byte boundary with
 * zero DC predictors (one restart interval; a frame without DRI is one segment).  The planner below cuts frames into
 * segments on the host, the kernel decodes one segment per lane into the coefficient layout above, and
 * tstar_jpeg_reconstruct runs on the result unchanged.  Flat little-endian records, no pointers:
 *   segment     6 x u32  {frame, byte begin, byte end (offset of the terminating marker), first MCU, MCU count, last (0 / 1)}
 *   frame       4 x i32  {table set (-1: routed to the host decoder), first segment, segment count, 0}
 *   table set   9016 bytes (six Huffman tables, quantisation rows, zigzag order, energy limits; csrc/jpeg_entropy_core.h)
 * Segment status: 0 OK, 1 malformed, 2 uncovered (the codes above); a frame's status is that of its first segment, in
 * stream order, that is not OK.
 *
 * Planner (host only, no HIP state): frame i is datas[i][0 .. lens[i]) and sits at byte_offsets[i] of the byte buffer the
 * segments will index (offset + length must stay below 2^32).  route i32 [n]: 0 device, 1 host -- a frame whose header,
 * tables or geometry tstar_jpeg_entropy_batch would not accept as they are, or whose framing (RSTn in order mod 8, their
 * count, EOI behind the last segment) is not exactly what the sequential decoder expects; that decoder's result is then
 * authoritative.  frames [n], quant u16 [n][192] (zero rows for host-routed frames), table sets deduplicated by content and
 * segments go to caller buffers of cap_sets / cap_segments records.  out5 = {table sets, segments, bytes of a table set,
 * bytes of a segment, bytes of a frame record}.  Returns 4 when a capacity is too small: out5 holds the counts needed, route /
 * frames / quant are already filled, table sets and segments were not written. */
int tstar_jpeg_plan_segments(const uint8_t* const* datas, const size_t* lens, const uint64_t* byte_offsets, int n, int W, int H,
                             int ncomp, int hs, int vs, int32_t* route, void* frames, uint16_t* quant, void* table_sets,
                             int cap_sets, void* segments, int cap_segments, size_t* out5);
/* Launcher on caller tensors: clears d_coef int16 [n_frames][blocks][64], then one lane per segment writes coefficients
 * and d_seg_status i32 [n_segments].  Every read is bounded by the segment's byte range inside d_bytes[0 .. total_bytes),
 * every store by the segment's frame's region of d_coef; a record that points outside the batch is status 1 and touches
 * nothing.  Refuses bad arguments before any launch. */
int tstar_jpeg_entropy_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                              int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                              int vs, int16_t* d_coef, int32_t* d_seg_status, void* stream);
/* The same arguments in host memory, the same decode core, segment by segment on the CPU. */
int tstar_jpeg_entropy_segments_host(const uint8_t* bytes, size_t total_bytes, const void* segments, const void* table_sets,
                                     int n_sets, const void* frames, int n_frames, int n_segments, int W, int H, int ncomp,
                                     int hs, int vs, int16_t* coef, int32_t* seg_status);
/* The split path: the same result for frames WITHOUT restart markers at many lanes per scan (self-synchronising parallel
 * Huffman decoding: Weissenberger & Schmidt, ICPP 2018).  A segment of at least min_split_bytes bytes (0: none, which is
 * tstar_jpeg_entropy_device's work exactly) is cut into sub-sequences of sub_bytes bytes, one lane each.  A decoder state is
 * the bit position, the block within the MCU, the zigzag index and the AC energy of the open block.
 *   rounds   round 0 starts every sub-sequence from a blank state at its own byte boundary (behind the 00 when that byte is the
 *            00 of an FF 00 pair), round r from the exit state its predecessor recorded in round r - 1; the first sub-sequence
 *            of a segment always starts at the segment start.  Nothing is stored but exit states, block counts and DC sums.  A
 *            segment has converged in the first round that changes none of its exits; after round max_rounds a segment that
 *            has not is abandoned.
 *   scan     per segment, exclusive, over (blocks completed, DC sums): first block and predictors of every sub-sequence.
 *   write    converged segments: one lane per sub-sequence stores coefficients under every check of the one-lane decoder.
 *            Every other segment (shorter than min_split_bytes, abandoned): one lane per segment, as before.
 *   redo     a cut segment whose write pass reports anything but OK is decoded again by one lane, and that status stands; were
 *            it OK the segment reports 2 (uncovered), which never happens.  Coefficients of a frame whose status is not 0 are
 *            unspecified and must not be read: the caller runs such a frame through the host decoder.
 * d_seg_info i32 [n_segments]: 0 one lane, r > 0 cut and converged in round r, -1 cut and abandoned.  d_seg_status and d_coef
 * are tstar_jpeg_entropy_device's, value for value.  TSTAR_JPEG_SUB_BYTES_MIN is the smallest legal sub_bytes (a symbol with
 * its magnitude bits is at most 27 bits; a state that lies behind a whole sub-sequence passes through it unchanged);
 * sub_bytes is a multiple of 4, max_rounds in 1 .. TSTAR_JPEG_SPLIT_MAX_ROUNDS.  The workspace is caller memory, 8-byte
 * aligned, of the size the query returns (0: bad arguments; no HIP work; it depends on the byte count, not on the records).
 * The launcher queues max_rounds + 5 launches (none of the rounds when min_split_bytes is 0) on the stream and never synchronises: order between the phases comes from the
 * kernel boundaries, no lane waits on another workgroup, every loop is bounded by the bits of its sub-sequence plus one
 * symbol, reads stay inside the segment's byte range and stores inside the frame's coefficient region and the workspace.
 * Refuses bad arguments before any launch.  The host mirror takes the same arguments in host memory, runs the same core in
 * the same round order and gives the same coefficients, statuses and seg_info. */
#define TSTAR_JPEG_SUB_BYTES_MIN 8
#define TSTAR_JPEG_SPLIT_MAX_ROUNDS 65536
size_t tstar_jpeg_split_workspace_bytes(size_t total_bytes, int n_segments, int sub_bytes);
int tstar_jpeg_entropy_split_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                                    int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                                    int vs, int sub_bytes, int min_split_bytes, int max_rounds, void* d_workspace,
                                    size_t workspace_bytes, int16_t* d_coef, int32_t* d_seg_status, int32_t* d_seg_info, void* stream);
int tstar_jpeg_entropy_split_host(const uint8_t* bytes, size_t total_bytes, const void* segments, const void* table_sets, int n_sets,
                                  const void* frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs, int vs,
                                  int sub_bytes, int min_split_bytes, int max_rounds, void* workspace, size_t workspace_bytes,
                                  int16_t* coef, int32_t* seg_status, int32_t* seg_info);
/* Compressed-resident store (added entries; tstar_abi_version() stays 3).  A file's wanted frames stay on the device as they are
 * on disk, in an ARENA, next to what the planner said about each: d_off u64 [n_entries] (the arena may exceed 4 GiB; a frame
 * may start at any byte), d_len u32 [n_entries], d_quant u16 [n_entries][192] (16-byte aligned), frame records whose
 * first_segment indexes d_segments, and segments whose begin / end count from the frame's first byte.  A FETCH of m arena
 * frames (repeats allowed) builds the buffer the entropy launchers take, without the host touching a compressed byte:
 *   bytes     the frames end to end, each at a 16-byte-aligned start, padded with zeros; total_bytes < 2^32
 *   quant     u16 [m][192] | frame records [m] | segments [n_segments], rebased to the batch (offsets from the size query)
 * Descriptor, 6 x u32 per frame, written by the host from the counts it kept when the file was opened: {arena frame, byte offset
 * in the batch, bytes, first segment in the batch, segments, 0}.  The launcher checks the HOST copy before any launch (ids,
 * exact tiling of the bytes and of the segment list, capacities, the 2^32 bound) and refuses what fails; the kernel reads the
 * DEVICE copy and checks each frame against the arena's own records again: one that disagrees is copied as zeros with a frame
 * record without a table set and segments that name no frame (status 1, nothing touched).  No load leaves a frame's arena
 * range, no store the batch buffer; one launch, no synchronisation.  The host mirror takes everything in host memory and
 * gives the same buffer word for word. */
/* Pure: bytes of the batch buffer for m frames (total_bytes: the sum of their lengths, each rounded up to 16) and n_segments
 * segments; out3 (optional) = byte offsets of {quant rows, frame records, segments}.  0: not a batch. */
size_t tstar_jpeg_gather_bytes(size_t total_bytes, int m, int n_segments, size_t* out3);
int tstar_jpeg_gather(const uint8_t* d_arena, size_t arena_bytes, const uint64_t* d_off, const uint32_t* d_len, const uint16_t* d_quant,
                      const void* d_frames, const void* d_segments, int n_entries, int n_arena_segments, const void* h_desc,
                      const void* d_desc, int m, size_t total_bytes, int n_segments, uint8_t* d_batch, size_t batch_bytes, void* stream);
int tstar_jpeg_gather_host(const uint8_t* arena, size_t arena_bytes, const uint64_t* off, const uint32_t* len, const uint16_t* quant,
                           const void* frames, const void* segments, int n_entries, int n_arena_segments, const void* desc, int m,
                           size_t total_bytes, int n_segments, uint8_t* batch, size_t batch_bytes);
/* tstar_jpeg_reconstruct with frame j written to d_pool[d_slots[j]] (d_pool u8 [pool_frames,H,W,3]; d_slots i32 [m], device
 * memory, read in place).  A slot outside 0 .. pool_frames - 1 is skipped: nothing of that frame is written. */
int tstar_jpeg_reconstruct_slots(const int16_t* d_coef, const uint16_t* d_quant, int m, int W, int H, int ncomp, int hs, int vs,
                                 uint8_t* d_planes, uint8_t* d_pool, int pool_frames, const int32_t* d_slots, void* stream);
/* Decode at 1/2, 1/4 or 1/8 size (added entries; tstar_abi_version() stays 3): the scaled decode of libjpeg-turbo, byte for byte what
 * Pillow's Image.draft gives.  scale 1, 2, 4 or 8; scale 1 is the entry without _scaled, argument for argument.  The entropy
 * stages, the coefficients and the tables are those of the full-size decode; only the inverse DCT and the chroma stage change.
 * With k = 8 / scale, every luma block goes through a k x k inverse DCT on its low-frequency corner (jidctred.c).  4:2:0 chroma
 * takes a 2k x 2k one, which makes its planes as large as the picture: nothing is upsampled.  4:2:2 chroma takes k x k and is
 * upsampled horizontally, by the triangle filter for k >= 2 and by replication for k = 1.  The picture is ow x oh =
 * ceil(W / scale) x ceil(H / scale).  NOT COVERED at a scale: 4:2:2 at scale 2 or 4 whose scaled chroma row, ceil(W * k / 16)
 * samples, is at most 2 samples long (the libjpeg quirk that excludes W <= 4 at full size); such frames go to a general decoder.
 * out4 = {ow, oh, bytes of the per-frame plane workspace at this scale, covered (1 / 0)}; TSTAR_ERR_ARG for a geometry the
 * full-size entries refuse or another scale. */
int tstar_jpeg_sizes_scaled(int W, int H, int ncomp, int hs, int vs, int scale, size_t* out4);
/* tstar_jpeg_reconstruct_host / tstar_jpeg_reconstruct / tstar_jpeg_reconstruct_slots with rgb u8 [n,oh,ow,3] (d_pool u8
 * [pool_frames,oh,ow,3]) and d_planes of n times the scaled plane-workspace bytes; alignment and argument rules as theirs.
 * TSTAR_ERR_ARG, before anything is written or launched, for another scale or a geometry that is not covered at this scale. */
int tstar_jpeg_reconstruct_scaled_host(const int16_t* coef, const uint16_t* quant, int n, int W, int H, int ncomp, int hs, int vs,
                                       int scale, uint8_t* rgb, int threads);
int tstar_jpeg_reconstruct_scaled(const int16_t* d_coef, const uint16_t* d_quant, int n, int W, int H, int ncomp, int hs, int vs,
                                  int scale, uint8_t* d_planes, uint8_t* d_rgb, void* stream);
int tstar_jpeg_reconstruct_slots_scaled(const int16_t* d_coef, const uint16_t* d_quant, int m, int W, int H, int ncomp, int hs, int vs,
                                        int scale, uint8_t* d_planes, uint8_t* d_pool, int pool_frames, const int32_t* d_slots,
                                        void* stream);
/* Lossless RE-CODING with a restart interval (added entries; tstar_abi_version() stays 3): the JPEG counterpart of
 * `jpegtran -restart`.  A batch of baseline frames of one geometry goes through the device entropy runner (coefficients in HBM),
 * through tstar_jpeg_encode_scan_rst (scans with the standard Huffman tables in fixed-size slots, per-frame length and status) and
 * through the assembly below, which builds a PIECE of a new arena and its records on the device.  Not a pixel changes: the
 * coefficients and the quantisation tables are the source's.
 * Header of a re-coded frame: the layout of tstar_jpeg_encode_header_rst with the DQT entries given (quant u16 [3][64], natural
 * order, rows Y / Cb / Cr, values 1..65535).  Equal chroma rows share table 1, else Cr takes table 2; a table with a value above
 * 255 is written with 16-bit entries and the frame header becomes SOF1, as libjpeg writes it.  At most 890 bytes; for the rows of
 * a quality the bytes are tstar_jpeg_encode_header_rst's.  TSTAR_ERR_ARG / 4 (cap short, nothing written). */
int tstar_jpeg_encode_header_tables(int W, int H, const uint16_t* quant, int hs, int vs, int restart, uint8_t* out, size_t cap, size_t* len);
/* Assembly.  Descriptor, 8 x u32 per frame j of the piece, written by the host once lengths and statuses are known:
 * {kind (0 re-coded: header row + the scan in slot j; 1 kept: the source bytes as they are), header row, frame of the source batch
 * (its quant row; for a kept frame its records), kept: byte offset and bytes in the source batch, table set of the output's frame
 * record (i32; -1: a kept frame without one), first segment in the output's list, segments (re-coded: ceil(n_mcu / restart);
 * kept: the source frame record's count)}.  Headers: u8 [n_headers][1024] with their lengths.  Slots: 16-byte aligned, slot_bytes a
 * multiple of 16.  The source batch is what the entropy launchers took: bytes, quant rows (16-byte aligned), frame records,
 * segments.  Output: the frames end to end from d_out[0] (no padding, as an arena packs them; out_bytes is the capacity, below
 * 2^32) and ONE record buffer, 16-byte aligned, of the size the layout query returns (0: not a piece; out5 = byte offsets of)
 *   off u64 [m + 1] (off[m]: the piece's bytes) | len u32 [m] | quant u16 [m][192] | frame records [m] | segments [n_segments]
 * which hold what tstar_jpeg_plan_segments says about the output bytes, field for field (begin / end from d_out[0], frame = j).
 * The launcher checks the HOST copy of the descriptor before any launch and refuses what fails; the kernels read the DEVICE copy
 * and check every frame against device memory again: a frame that fails takes no bytes and gets a record without a table set and
 * segments that name no frame.  No load leaves a slot, a header row or a kept frame's source range, no store the frame's range
 * below out_bytes or the record buffer.  longest: the most bytes a frame takes (it sizes the grid only).  Three launches, no
 * synchronisation.  The host mirror takes everything in host memory and gives the same bytes and records word for word. */
size_t tstar_jpeg_recode_layout(int m, int n_segments, size_t* out5);
int tstar_jpeg_recode_assemble(const void* h_desc, const void* d_desc, int m, int n_segments, const uint8_t* d_headers,
                               const uint32_t* d_header_len, int n_headers, const uint8_t* d_slots, size_t slot_bytes,
                               const uint32_t* d_scan_len, int restart, int n_mcu, const uint8_t* d_src_bytes, size_t src_total,
                               const uint16_t* d_src_quant, const void* d_src_frames, const void* d_src_segments, int n_src_frames,
                               int n_src_segments, uint8_t* d_rec, size_t rec_bytes, uint8_t* d_out, size_t out_bytes, size_t longest,
                               void* stream);
int tstar_jpeg_recode_assemble_host(const void* desc, int m, int n_segments, const uint8_t* headers, const uint32_t* header_len,
                                    int n_headers, const uint8_t* slots, size_t slot_bytes, const uint32_t* scan_len, int restart,
                                    int n_mcu, const uint8_t* src_bytes, size_t src_total, const uint16_t* src_quant,
                                    const void* src_frames, const void* src_segments, int n_src_frames, int n_src_segments, uint8_t* rec,
                                    size_t rec_bytes, uint8_t* out, size_t out_bytes);
/* ---- Re-coding with OPTIMISED HUFFMAN TABLES (added entries; tstar_abi_version() stays 3): the counterpart of
 * `jpegtran -optimize -restart N`.  Two modes.  PER FRAME: tstar_jpeg_encode_scan_opt on the decoder's coefficients, every frame
 * under a header of its own.  SHARED: the frames of a GROUP are coded with ONE set of four tables, built by the same procedure from
 * the SUM of their symbol counts (the DC predictors restart with every frame, so the sum over frames is exact); a compressed-resident
 * arena then needs one decoder table set per group and quantisation set instead of one per frame.
 * Header: the layout of tstar_jpeg_encode_header_tables (the source's DQT entries, SOF0 or SOF1) with the four tables of `specs`
 * (4 x 276 bytes, each with status 0) in the DHT segments.  At most 1566 bytes; for the rows of a quality the bytes are
 * tstar_jpeg_encode_header_opt's.  restart 0: no DRI. */
int tstar_jpeg_encode_header_tables_opt(int W, int H, const uint16_t* quant, int hs, int vs, int restart, const uint8_t* specs, uint8_t* out,
                                        size_t cap, size_t* len);
/* Groups.  group i32 [n]: the group of every frame of the batch, -1 for a frame that is not coded (status 3, length 0); group
 * numbers start at 0 and rise by one in frame order, so a group's frames are consecutive but for such frames.  A group holds at
 * most 1000000000 / (64 * blocks) frames, at least 1 (the first entry returns that number; 0: unsupported geometry): a block emits
 * at most 64 symbols, so a group's counts stay within what tstar_jpeg_huff_optimal is defined for and the u32 bins cannot wrap.
 * The second entry checks the groups and writes span i32 [n_groups][2], the first frame of every group and the frame behind its
 * last, which the device entry wants next to the groups. */
int tstar_jpeg_encode_group_frames(int W, int H, int hs, int vs);
int tstar_jpeg_encode_group_spans(const int32_t* group, int n, int n_groups, int W, int H, int hs, int vs, int32_t* span);
/* Scan stage with shared tables.  stages, a sum of: 1 the frames' counts (tstar_jpeg_encode_scan_opt's histogram launch) and their
 * sums per group into group_hist u32 [n_groups][4][257], added in frame order by a kernel that stores every bin once (no atomics);
 * 2 the groups' tables from group_hist AS IT IS (so a caller may put counts of its own there) into specs u8 [n_groups][4][276] and,
 * on the device, the code tables of the workspace; 4 the scans, coded with the tables stage 2 left (host: rebuilt from specs).  A
 * frame of a group one of whose tables has a status reports 3 with length 0, unless its walk met a coefficient without a code (2).
 * The device entry takes the groups and spans twice, in host memory (checked before any launch) and in device memory (read by the
 * kernels, which treat a group outside 0 .. n_groups - 1 as -1 and clip a span to the n frames).  Workspace: the bytes
 * tstar_jpeg_encode_plan_opt names with optimize = 1 for these n and slot_bytes.  No synchronisation. */
int tstar_jpeg_encode_scan_host_grp(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, const int32_t* group,
                                    int n_groups, int stages, uint32_t* group_hist, uint8_t* specs, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, int threads);
int tstar_jpeg_encode_scan_grp(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, const int32_t* h_group,
                               const int32_t* h_span, const int32_t* d_group, const int32_t* d_span, int n_groups, int stages,
                               uint32_t* d_group_hist, uint8_t* d_specs, uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths,
                               int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* The assembly with header rows of header_pitch bytes (a multiple of 16 in 16..65536 that holds the piece's longest header; rows 16-byte
 * aligned) and restart 0..65535 (0: no interval, a re-coded frame is one segment; so is one whose interval is not shorter than the
 * frame).  Everything else, bytes and records included, is tstar_jpeg_recode_assemble's. */
int tstar_jpeg_recode_assemble_opt(const void* h_desc, const void* d_desc, int m, int n_segments, const uint8_t* d_headers,
                                   size_t header_pitch, const uint32_t* d_header_len, int n_headers, const uint8_t* d_slots,
                                   size_t slot_bytes, const uint32_t* d_scan_len, int restart, int n_mcu, const uint8_t* d_src_bytes,
                                   size_t src_total, const uint16_t* d_src_quant, const void* d_src_frames, const void* d_src_segments,
                                   int n_src_frames, int n_src_segments, uint8_t* d_rec, size_t rec_bytes, uint8_t* d_out,
                                   size_t out_bytes, size_t longest, void* stream);
int tstar_jpeg_recode_assemble_host_opt(const void* desc, int m, int n_segments, const uint8_t* headers, size_t header_pitch,
                                        const uint32_t* header_len, int n_headers, const uint8_t* slots, size_t slot_bytes,
                                        const uint32_t* scan_len, int restart, int n_mcu, const uint8_t* src_bytes, size_t src_total,
                                        const uint16_t* src_quant, const void* src_frames, const void* src_segments, int n_src_frames,
                                        int n_src_segments, uint8_t* rec, size_t rec_bytes, uint8_t* out, size_t out_bytes);
/* Native-resolution RGB u8 [n,H,W,3] of NV12 frames (the keyframes pop_frames hands back, :379-380). */
int tstar_nv12_to_rgb(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n,
                      uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------ searcher state (S-rows)
 * Device-resident float64 state of one TStarSearcher (interface_searcher.py:73-75):
 * score_distribution, non_visiting_frames, P, plus the sampler's working arrays.  All
 * kernels are single-workgroup and reproduce numpy's operation order (pairwise sum,
 * sequential cumsum, 'linear' percentile); see csrc/searcher.hip for the line map. */
typedef struct tstar_searcher tstar_searcher;
int tstar_searcher_create(tstar_searcher** out, int n_frames, double init_score, double init_p);
int tstar_searcher_destroy(tstar_searcher* s);
/* update_frame_distribution up to the spline fit (interface_searcher.py:302-313, 260-261):
 * for the n sampled seconds (draw order) and their cell confidences d_conf f64 [n] (device,
 * cell i <-> sample i): mark visited, write scores, top-25 % window spread; returns the
 * visited frames (ascending) and their scores to the host for the FITPACK fit.  Synchronises. */
int tstar_searcher_apply_grid(tstar_searcher* s, const int32_t* h_secs, const double* d_conf, int n,
                              int* h_n_visited, int32_t* h_vis_x, double* h_vis_y, void* stream);
/* update_top_25_with_window alone (interface_searcher.py:215-241) on the device score array: np.percentile(h_conf, 75),
 * then for every sample with conf >= threshold, in the given order and in place, score[f + o] = max(score[f + o],
 * score[f] / (|o| + 1)) for |o| <= window.  Synchronises. */
int tstar_searcher_window_spread(tstar_searcher* s, const int32_t* h_secs, const double* h_conf, int n, int window,
                                 void* stream);
/* the visited frames (non_visiting == 0, ascending) and their scores (interface_searcher.py:260-261).  Synchronises. */
int tstar_searcher_visited(tstar_searcher* s, int* h_n_visited, int32_t* h_vis_x, double* h_vis_y, void* stream);
/* spline_keyframe_distribution after the fit (interface_searcher.py:266-274): evaluates the
 * B-spline (t, c, k) from scipy's UnivariateSpline at 0..N-1 (FITPACK splev, ext=0), clamps at
 * 1/N, sigmoid, normalises -> P. */
int tstar_searcher_set_spline(tstar_searcher* s, const double* h_t, const double* h_c, int n_knots, int k, void* stream);
/* sample_frames' weights (interface_searcher.py:345-352) with add = num/N, and the cdf of
 * np.random.choice; *h_fallback = 1 if the unvisited mask was dropped.  Synchronises. */
int tstar_searcher_sampler_prep(tstar_searcher* s, int num, double add, int* h_fallback, void* stream);
/* pop_frames' weights (interface_searcher.py:369) and their cdf.  *h_nnz = count_nonzero(p > 0) and *h_sum =
 * score.sum(): what numpy's choice() validates before drawing ("probabilities contain NaN" when the sum is 0 or NaN,
 * "Fewer non-zero entries in p than size").  Synchronises. */
int tstar_searcher_pop_prep(tstar_searcher* s, int* h_nnz, double* h_sum, void* stream);
/* cdf.searchsorted(x, 'right') for k host-drawn uniforms (the MT19937 stream stays on the host,
 * numpy legacy RandomState.choice).  Synchronises. */
int tstar_searcher_draw(tstar_searcher* s, const double* h_x, int k, int32_t* h_idx, void* stream);
/* choice()'s retry step: p[found] = 0, cdf recomputed. */
int tstar_searcher_exclude(tstar_searcher* s, const int32_t* h_found, int m, void* stream);
/* verification overwrites (interface_searcher.py:407): score[secs[i]] = vals[i], in order. */
int tstar_searcher_set_scores(tstar_searcher* s, const int32_t* h_secs, const double* h_vals, int m, void* stream);
/* store_score_distribution (interface_searcher.py:207-213): P, score_distribution and non_visiting_frames
 * copied to h_out f64 [3, N] (in that order) with ONE synchronisation. */
int tstar_searcher_read_state(tstar_searcher* s, double* h_out, void* stream);
/* overwrite a state array from the host (the reference's attributes are plain numpy arrays a caller may assign):
 * 0 score_distribution, 1 non_visiting_frames, 2 P -- e.g. P computed on the host by the reference's own numpy/scipy
 * calls (bit-identical by construction; tstar_searcher_set_spline is the device-side alternative).  Synchronises. */
int tstar_searcher_write(tstar_searcher* s, int which, const double* h_in, void* stream);
/* copy a state array to the host: 0 score, 1 non_visiting, 2 P, 3 sampler p, 4 cdf.  Synchronises. */
int tstar_searcher_read(tstar_searcher* s, int which, double* h_out, void* stream);

/* ------------------------------------------------------------------ multi-GPU
 * The path shards over independent (video, question) items with no data-path collective; the ONE exchange is an
 * all-gather of every rank's final keyframe indices -- what the sequential loop of
 * LVHaystackBench/run_TStar_onDataset.py:195-205 accumulates in `results`.  One process per GPU; RCCL over xGMI.
 * Bootstrap like NCCL's: rank 0 calls tstar_comm_unique_id and hands the TSTAR_COMM_ID_BYTES bytes to every rank by
 * any out-of-band channel (a file, a TCP store, MPI, torch.distributed's store); then EVERY rank calls
 * tstar_comm_create (collective; binds the current HIP device).  RCCL is dlopen'ed on first use (the copy a host
 * such as PyTorch-ROCm already carries is reused); TSTAR_RCCL_LIB overrides the library name. */
#define TSTAR_COMM_ID_BYTES 128
typedef struct tstar_comm tstar_comm;
/* binds RCCL in THIS process without touching any other rank (0 = usable).  tstar_comm_create is collective, so hosts
 * call this on every rank and agree on the outcome first: a rank that cannot load RCCL must not leave the others
 * blocked inside ncclCommInitRank. */
int tstar_comm_available(void);
int tstar_comm_unique_id(void* h_id /* TSTAR_COMM_ID_BYTES bytes */);
int tstar_comm_create(tstar_comm** out, const void* h_id, int world, int rank);
int tstar_comm_destroy(tstar_comm* c);
/* d_recv int32 [world * count] = concatenation over ranks (rank order) of every rank's d_send int32 [count] (both on
 * the device; pad short rows with -1).  Enqueued on `stream`; does not synchronise. */
int tstar_allgather_i32(tstar_comm* c, const int32_t* d_send, int32_t* d_recv, int count, void* stream);

/* ------------------------------------------------------------------ downstream selection (8f)
 * Replaces the score-based branch of extract_frames (LVHaystackBench/val_qa_results.py:90-110): the k
 * highest-probability seconds of a per-second distribution d_P f64 [N] (device) inside
 * [clip_start, clip_end), returned in ascending order (host int32 [k]); NaN -> 0, all-zero -> uniform; the clip is
 * normalised in float32 (numpy's pairwise sum, then an f32 divide) BEFORE ranking, as the reference does, so
 * division-induced ties are reproduced; ties resolve to the lowest index.  Synchronises. */
int tstar_topk_seconds(const double* d_P, int N, int clip_start, int clip_end, int k, int32_t* h_out, void* stream);

/* Replaces pairwise_ssim / ssim_torch (LVHaystackBench/val_tstar_results.py:48-95): SSIM of every
 * (ground-truth, predicted) keyframe pair, frames u8 [G,H,W,3] / [P,H,W,3] on the device, 11x11 Gaussian
 * window (host float32 [121], sigma 1.5) -> d_out f64 [G,P].  Keeps the reference's HWC-as-CHW layout
 * quirk (the window slides over the (W, colour) plane of each row).  Synchronises. */
int tstar_ssim_pairwise(const uint8_t* d_gt, int G, const uint8_t* d_pred, int P, int H, int W,
                        const float* h_window, double* d_out, void* stream);

/* Replaces OWLInterface.bbox_visualization (interface_heuristic.py:259-267) for images that are already on the
 * device: paints the 1-px box of every kept detection (score > 0.005) of image b -- d_boxes_xyxy [B,576,4] and
 * d_scores [B,576] as written by tstar_owl_score -- onto d_images u8 [B,H,W,3] in place. */
int tstar_draw_boxes(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, void* stream);
/* The same for np detections per image (d_boxes_xyxy [B,np,4], d_scores [B,np]; np = tstar_owl_num_patches of the handle
 * that scored them).  Added entry; tstar_draw_boxes is this with np = 576. */
int tstar_draw_boxes_np(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, int np,
                        void* stream);

/* ------------------------------------------------------------------ kernel-level diagnostics
 * (used by tests/ and bench.py to check and time individual kernels) */
/* C[M,N] = act(A[M,K] * W[N,K]^T + bias) (+ residual); act: 0 none, 1 quick-gelu, 2 gelu(erf) */
int tstar_gemm_f32(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                   int M, int N, int K, int act, void* stream);
/* same with the block tile forced: 0 = 128x128, 1 = 64x128, 2 = 64x64, 3 = hybrid (128x128 + 64x128 tail);
 * -1 = the launcher's choice; 16 + n = hybrid with the first n row tiles of 128 rows big (tile-policy sweeps) */
int tstar_gemm_f32_cfg(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                       int M, int N, int K, int act, int tile_cfg, void* stream);
/* bf16-weight GEMM (diagnostic): W is rounded to bfloat16 on the device, A is split exactly; synchronises */
int tstar_gemm_bf16w(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                     int M, int N, int K, int act, int tile_cfg, void* stream);
/* bf16-weight GEMM with two-term activations (diagnostic; tile_cfg 4 forces the 128x256 tile, 5 forbids it, 6 (round 6; needs N % 256 == 0 and
 * M >= 128) forces the 128x256 tile whose weight fragments stream global -> VGPR from a fragment-packed plane -- what the library picks by itself
 * for the N = 768 layers; every choice returns the same bits) */
int tstar_gemm_bf16w2(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                      int M, int N, int K, int act, int tile_cfg, void* stream);
/* bf16-weight GEMM on weights that are ALREADY bfloat16 on the device (d_Wb: [N, K] bf16); a_terms 2 or 3; enqueues only
 * (microbenchmarks) */
int tstar_gemm_bf16w_pre(const float* d_A, const void* d_Wb, float* d_C, const float* d_bias, const float* d_residual,
                         int M, int N, int K, int act, int a_terms, int tile_cfg, void* stream);
/* f32x3 GEMM (diagnostic): W is packed into three exact bf16 planes on the device, A is split on the fly, six products
 * (TSTAR_WEIGHTS_F32X3); N % 128 == 0, K % 32 == 0; tile_cfg as above, 4 forces the 128x256 tile, 5 forbids it; synchronises */
int tstar_gemm_f32x3(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                     int M, int N, int K, int act, int tile_cfg, void* stream);
/* the same in two steps for microbenchmarks: pack once (d_Wp: 6 * N * K bytes on the device), then enqueue-only GEMMs on the packed planes */
int tstar_pack_f32x3(const float* d_W, void* d_Wp, int N, int K, void* stream);
int tstar_gemm_f32x3_pre(const float* d_A, const void* d_Wp, float* d_C, const float* d_bias, const float* d_residual,
                         int M, int N, int K, int act, int tile_cfg, void* stream);
/* The tile plan the GEMM launcher makes for a problem (an added entry; tstar_abi_version() stays 3).  Pure integer arithmetic: needs no
 * GPU and launches nothing.  weights_mode: a TSTAR_WEIGHTS_* value; ldc and patch_np (0 = none) as the launch passes them (the patch
 * embedding writes token rows: ldc = N, patch_np = patches per image); tile_cfg as above; has_packed_w2: the two-term mode's
 * fragment-packed weight plane exists.  plan4 = { kind, m_split, blocks, dynamic LDS bytes per block }; kind 0 / 1 / 2 = a pure grid of
 * 128x128 / 64x128 / 64x64 tiles, 3 = hybrid (rows [0, m_split) in 128x128 tiles, the rest 64x128), 4 = wide (128x256 + 64x128 tail),
 * 5 = wide with the weights streamed global -> VGPR.  TSTAR_ERR_ARG where tstar_gemm_* would refuse the same arguments. */
int tstar_gemm_plan(int weights_mode, int M, int N, int ldc, int patch_np, int tile_cfg, int has_packed_w2, int* plan4);
/* The patch-embedding form of the GEMM, which no other tstar_gemm_* entry can ask for (an added entry; tstar_abi_version() stays 3):
 * d_X [B*(np+1), N] token row b*(np+1) + 1 + p = d_A [B*np, K] row (b*np + p) x d_W[N, K]^T + d_pos [np+1, N] row (1 + p); the
 * class-token rows b*(np+1) are not written.  weights_mode: a TSTAR_WEIGHTS_* value; the bf16 / fragment-packed / three-plane
 * weights are made from d_W as tstar_gemm_bf16w / tstar_gemm_bf16w2 / tstar_gemm_f32x3 make them.  tile_cfg as above.  Refuses
 * (TSTAR_ERR_ARG, nothing launched) what tstar_gemm_plan(weights_mode, B*np, N, N, np, tile_cfg, two-term mode && N % 256 == 0)
 * refuses, and K % 32 != 0.  Synchronises the stream. */
int tstar_gemm_patch_embed(const float* d_A, const float* d_W, float* d_X, const float* d_pos, int B, int np, int N, int K,
                           int weights_mode, int tile_cfg, void* stream);
/* The launch plan tstar_frames_resize (op 0: n frames -> out_w x out_h = ow x oh) or tstar_frames_to_grid (op 1: n = grid_rows * grid_cols,
 * ow x oh = the 200 x 95 cell) makes (an added entry; tstar_abi_version() stays 3).  Pure: needs no GPU and launches nothing.
 * out_aligned4 / video_aligned4: the output / frame-store pointer is a multiple of 4; generic, nv12_lds, grid_px: the values of
 * TSTAR_INGEST_GENERIC (default 0), TSTAR_NV12_LDS (default 1) and TSTAR_GRID_PX (default 1).  plan6 = { kind, pixels per lane, grid.x,
 * grid.y, dynamic LDS bytes, LDS row pitch in dwords }; kind 0 = generic kernels, 1 = RGB fast path, 2 = NV12 per tap, 3 = NV12 through LDS
 * (resize only).  TSTAR_ERR_ARG where the launchers refuse the same n / ow / oh. */
int tstar_ingest_plan(int op, int nv12, int H, int W, int n, int ow, int oh, int out_aligned4, int video_aligned4, int generic,
                      int nv12_lds, int grid_px, int* plan6);
int tstar_layernorm_f32(const float* d_x, float* d_y, const float* d_w, const float* d_b, int rows, int D, void* stream);
/* qkv [B*T, 3*heads*64] -> out [B*T, heads*64]; mode 0 full, 1 causal + key mask u8 [B,T] */
int tstar_attention_f32(const float* d_qkv, float* d_out, int B, int T, int heads, int mode,
                        const uint8_t* d_key_mask, void* stream);

/* full attention with f32-split operands on the bf16 matrix pipe (what the bf16-pipe weights modes use) */
int tstar_attention_split(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream);
/* full attention with EXACT operands on the bf16 matrix pipe: Q, K, V and the probabilities as three bf16 terms each, six
 * products per MFMA step, f32 accumulation (what TSTAR_WEIGHTS_F32X3 uses for the vision tower; replaces the fp32
 * softmax(Q K^T / 8) V of HF modeling_owlvit.py:377-402 behind TStar/interface_heuristic.py:237-239) */
int tstar_attention_x3(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream);
/* The same with the block order given (diagnostics / A-B runs; added entries): order 1 = the query tiles of one (image, head), which
 * stage the same K / V rows, run back to back on ONE XCD (what tstar_attention_x3 does unless TSTAR_AX3_XCD_OFF is set in the
 * environment), 0 = linear block ids, query tile fastest.  Every block computes the same tile either way: the output bits are equal.
 * tstar_xcd_group_block (pure, no GPU): the logical block (group * gsize + member) that hardware block bid of the order-1 grid of
 * tstar_xcd_groups_grid(ngroups, gsize) blocks computes, -1 for a padding block that exits at once, -2 for a bad argument. */
int tstar_attention_x3_order(const float* d_qkv, float* d_out, int B, int T, int heads, int order, void* stream);
int tstar_xcd_group_block(int bid, int ngroups, int gsize);
int tstar_xcd_groups_grid(int ngroups, int gsize);

/* Per-kernel timing with HIP events recorded on the launch stream, for bench.py's roofline leg.
 * category 0 = gemm_f32_kernel, 1 = attention_f32_kernel, 2 = conv_valu_kernel (YOLO-World backend).  enable(n > 0) resets the counters and times ONE of every
 * n consecutive launches of each category, at a position that varies from block to block (n = 1: all; a fixed phase would alias with periodic launch patterns);
 * read() synchronises the recorded events and returns launches / total ms / total algorithmic flops. */
int tstar_prof_enable(int on);
int tstar_prof_read(int category, long long* launches, double* total_ms, double* total_flops);
/* algorithmic HBM bytes of the launches tstar_prof_read counted (operands read once, results written once) */
int tstar_prof_read_bytes(int category, double* total_bytes);
/* EVERY launch of the category since enable(), sampled or not: their number and their algorithmic flops (exact; with the
 * sampled launches' flops / ms this gives the category's time without the sampling error of a 1-in-n sample of durations) */
int tstar_prof_read_totals(int category, long long* launches_all, double* flops_all);
/* trace markers: enqueue an empty kernel named prof_mark_begin_kernel (which = 0) / prof_mark_end_kernel (1) on `stream`,
 * so that a rocprofv3 kernel trace can be cut to the bracketed region on the GPU's own timeline */
int tstar_prof_mark(int which, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSTAR_HIP_H */
