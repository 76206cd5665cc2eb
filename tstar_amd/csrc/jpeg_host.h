// Baseline JPEG decode front end, host half (HIP-free: also compiled alone by the CPU sanitizer build).
//
// Split of the work (DESIGN.md "JPEG decode stage"): the entropy stage below turns one JPEG into int16 coefficient
// blocks + quantisation tables; dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB are data-parallel and
// run either in jpeg.hip (device) or in jpeg_reconstruct_host (the scalar reference, same integers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace tstar {

// status of one frame (also the return value of the single-frame calls)
enum {
    JPEG_OK = 0,
    JPEG_MALFORMED = 1,      // broken or truncated stream: an error, never a partial picture
    JPEG_UNCOVERED = 2,      // a JPEG this decoder does not cover (progressive, arithmetic, CMYK / RGB, other sampling) or does
                             // not vouch for (stray bytes or no EOI after the last block, a block beyond the energy bound)
    JPEG_GEOMETRY = 3,       // decodable, but width / height / components / sampling differ from the batch's geometry
};

// Geometry shared by every frame of a batch.  hs, vs: luma sampling factors (1x1, 2x1 or 2x2; chroma is always 1x1).
struct JpegGeom {
    int W, H, ncomp, hs, vs;
    int mcux() const { return (W + 8 * hs - 1) / (8 * hs); }
    int mcuy() const { return (H + 8 * vs - 1) / (8 * vs); }
    // blocks per row / column of component c, padded to whole MCUs
    int bw(int c) const { return mcux() * (c == 0 ? hs : 1); }
    int bh(int c) const { return mcuy() * (c == 0 ? vs : 1); }
    // true (unpadded) sample size of component c: ceil(W * h_c / hmax)
    int cw(int c) const { return c == 0 ? W : (W + hs - 1) / hs; }
    int ch(int c) const { return c == 0 ? H : (H + vs - 1) / vs; }
    size_t blocks() const {
        size_t b = 0;
        for (int c = 0; c < ncomp; ++c) b += (size_t)bw(c) * bh(c);
        return b;
    }
    size_t block_offset(int c) const {
        size_t b = 0;
        for (int k = 0; k < c; ++k) b += (size_t)bw(k) * bh(k);
        return b;
    }
    size_t plane_bytes() const { return blocks() * 64; }          // u8 planes of whole blocks
    // Subsampled chroma at most 2 samples wide (W <= 4) is excluded: libjpeg replicates such rows instead of running the
    // triangle filter, and frames that small go to the general decoder.
    bool valid() const {
        return W > 0 && H > 0 && W <= 16384 && H <= 16384 && (ncomp == 1 || ncomp == 3) &&
               ((hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2) && cw(1) > 2));
    }
};

// How the colour stage of a scaled decode reads chroma
enum {
    JPEG_CHROMA_FULL = 0,            // the chroma planes are as large as the picture (grayscale, 4:4:4, scaled 4:2:0)
    JPEG_CHROMA_FANCY_H2V1 = 1,      // half width, libjpeg's triangle filter (upsample_at with hs 2, vs 1)
    JPEG_CHROMA_REPLICATE_H2V1 = 2,  // half width, every sample twice
};

// A decode of geometry g at 1/scale size (scale 1, 2, 4, 8), as libjpeg-turbo does it: every block of component c goes through
// an inverse DCT of output size kc(c) x kc(c) on its low-frequency corner.  Luma takes k = 8 / scale.  4:2:0 chroma takes 2k
// (libjpeg scales it up in the IDCT instead of upsampling: at scale 2 that is the full 8 x 8 transform), so its plane is as
// large as the picture and nothing is upsampled; 4:2:2 chroma stays at k (the vertical condition fails) and is upsampled
// horizontally, by the triangle filter for k >= 2 and by replication for k = 1, where libjpeg turns fancy upsampling off.
// Planes: component after component, whole blocks, rows of pitch(c) bytes (a multiple of 4), each plane a multiple of 8 bytes.
// Scale 1 is the full-size decode: its entries delegate to JpegGeom's own code, and kc / chroma_mode below describe scales 2, 4, 8.
struct JpegScaledGeom {
    JpegGeom g;
    int scale;
    bool scale_ok() const { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }
    int k() const { return 8 / scale; }
    int kc(int c) const { return (c > 0 && g.hs == 2 && g.vs == 2 && scale > 1) ? 2 * k() : k(); }
    int ow() const { return (g.W + scale - 1) / scale; }
    int oh() const { return (g.H + scale - 1) / scale; }
    // true sample size of component c at this scale: ceil(W * h_c * kc / (hmax * 8))
    int cw(int c) const { return c == 0 ? ow() : (g.W * kc(c) + 8 * g.hs - 1) / (8 * g.hs); }
    int ch(int c) const { return c == 0 ? oh() : (g.H * kc(c) + 8 * g.vs - 1) / (8 * g.vs); }
    int pitch(int c) const { return (g.bw(c) * kc(c) + 3) & ~3; }
    size_t plane_size(int c) const { return ((size_t)pitch(c) * g.bh(c) * kc(c) + 7) & ~(size_t)7; }
    size_t plane_offset(int c) const {
        size_t b = 0;
        for (int j = 0; j < c; ++j) b += plane_size(j);
        return b;
    }
    size_t plane_bytes() const { return plane_offset(g.ncomp); }
    int chroma_mode() const {
        if (g.ncomp == 1 || g.hs == 1 || kc(1) != k()) return JPEG_CHROMA_FULL;
        return k() >= 2 ? JPEG_CHROMA_FANCY_H2V1 : JPEG_CHROMA_REPLICATE_H2V1;
    }
    // Not covered at this scale (the frame goes to the general decoder): the triangle filter over a chroma row of at most 2
    // samples, the libjpeg quirk JpegGeom::valid() excludes at full size.
    bool covered() const {
        return scale_ok() && g.valid() && (scale == 1 || chroma_mode() != JPEG_CHROMA_FANCY_H2V1 || cw(1) > 2);
    }
};

// Header walk only.  JPEG_OK: *g filled.  JPEG_UNCOVERED: g->W, g->H filled when a frame header was seen (else 0).
int jpeg_probe(const uint8_t* data, size_t len, JpegGeom* g, char* err, size_t errlen);

// Entropy-decode one frame of geometry g: coef int16 [g.blocks()][64] (natural order, component after component,
// block-raster within the component, padded to whole MCUs), quant u16 [3][64] (natural order; unused rows zero).
int jpeg_entropy(const uint8_t* data, size_t len, const JpegGeom& g, int16_t* coef, uint16_t* quant, char* err, size_t errlen);

// Byte offset one past the EOI of the JPEG that starts at data[pos] (found by walking marker segments and the stuffed
// entropy data), or 0 when the stream is broken / ends first.
size_t jpeg_frame_end(const uint8_t* data, size_t len, size_t pos);

// Segments for the entropy stage on the device (records and decode core: jpeg_entropy_core.h).  Walks the header and, once,
// the entropy data of n frames of geometry g; frame i sits at byte_offsets[i] of the byte buffer the segments index.
// route[i] = 0: frames[i], quant row i, its table set and its segments are filled; 1: the frame goes to jpeg_entropy, whose
// result is authoritative (header, tables or geometry it would not accept as they are, or framing that is not exactly what
// it expects).  Table sets (deduplicated by content) and segments are appended to *sets / *segments.  Returns false when an
// offset does not fit the segments' 32 bits.
struct JpegTableSet;
struct JpegSegment;
struct JpegFrameDesc;
bool jpeg_plan_segments(const uint8_t* const* datas, const size_t* lens, const uint64_t* byte_offsets, int n, const JpegGeom& g,
                        int32_t* route, JpegFrameDesc* frames, uint16_t* quant, std::vector<JpegTableSet>* sets,
                        std::vector<JpegSegment>* segments);

// The device kernel's decode core on the CPU, segment by segment: clears coef [n_frames][g.blocks() * 64], then writes it
// and seg_status [n_segments].  False on a null argument or unsupported geometry.
bool jpeg_entropy_segments_host(const uint8_t* bytes, size_t total_bytes, const JpegSegment* segments, const JpegTableSet* tables,
                                int n_sets, const JpegFrameDesc* frames, int n_frames, int n_segments, const JpegGeom& g,
                                int16_t* coef, int32_t* seg_status);

// The split path (jpeg_entropy_core.h "sub-sequences"): segments of at least min_split_bytes bytes (0: none) are cut into
// sub-sequences of sub_bytes bytes that are decoded side by side; rounds 0 .. max_rounds bring their entry states to the
// sequential decoder's, a scan hands out block indices and DC predictors, a write pass stores the coefficients.  Every
// other segment, and every cut one the write pass does not return OK for, is decoded by decode_segment, whose status
// stands (coefficients of a frame that is not OK are never read: the host decoder replaces the frame).  seg_info [n_segments]:
// 0 one lane, r > 0 cut and converged in round r, -1 cut and abandoned after max_rounds.  The workspace is caller memory of
// jpeg_split_workspace_bytes bytes (0: bad arguments), 8-byte aligned.  This is the CPU mirror of the device launcher:
// the same core in the same round order.
constexpr int kJpegSplitMaxRounds = 65536;        // TSTAR_JPEG_SPLIT_MAX_ROUNDS (include/tstar_hip.h)
size_t jpeg_split_workspace_bytes(size_t total_bytes, int n_segments, int sub_bytes);
bool jpeg_split_args_ok(size_t total_bytes, int n_segments, int sub_bytes, int min_split_bytes, int max_rounds, const void* workspace,
                        size_t workspace_bytes);
bool jpeg_entropy_split_host(const uint8_t* bytes, size_t total_bytes, const JpegSegment* segments, const JpegTableSet* tables,
                             int n_sets, const JpegFrameDesc* frames, int n_frames, int n_segments, const JpegGeom& g, int sub_bytes,
                             int min_split_bytes, int max_rounds, void* workspace, size_t workspace_bytes, int16_t* coef,
                             int32_t* seg_status, int32_t* seg_info);

// Scalar reference of the device stage: coefficients + tables -> RGB u8 [H][W][3].  scratch: g.plane_bytes() bytes.
void jpeg_reconstruct_host(const JpegGeom& g, const int16_t* coef, const uint16_t* quant, uint8_t* scratch, uint8_t* rgb);
// The same at 1/scale size (scale 2, 4, 8; sg.covered()): RGB u8 [sg.oh()][sg.ow()][3], byte-equal to libjpeg-turbo's scaled
// decode (Pillow's Image.draft).  scratch: sg.plane_bytes() bytes.
void jpeg_reconstruct_scaled_host(const JpegScaledGeom& sg, const int16_t* coef, const uint16_t* quant, uint8_t* scratch, uint8_t* rgb);

// threads a batch may use: min(16, CPUs this process is allowed to run on); `asked` > 0 lowers it further
int jpeg_thread_allowance(int asked);

}  // namespace tstar
