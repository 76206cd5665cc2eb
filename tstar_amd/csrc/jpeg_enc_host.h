// Baseline JPEG encoder, host half (HIP-free: also compiled alone by the CPU sanitizer build).  The twin of jpeg_enc.hip:
// the same two stages on the same integers (jpeg_enc_math.h), byte-equal to Pillow's
// Image.fromarray(frame).save(buf, "JPEG", quality=q, subsampling=s).
//
//   stage 1  RGB u8 frames -> int16 coefficients in the DECODER's layout (jpeg_host.h: [g.blocks()][64], natural order,
//            component after component, block raster, padded to whole MCUs; g.ncomp = 3)
//   stage 2  coefficients -> the stuffed entropy-coded bytes of the one interleaved scan, ending in EOI
//   header   SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS: the same for every frame of a call
//
// Capacity rule of a scan buffer: jpeg_enc_max_scan_bytes(g) always fits.  It is 2 * ceil(blocks * kMaxBlockBits / 8) + 2:
// the longest codes of the four tables on every coefficient, every byte of it stuffed, plus EOI.  A caller that gives
// less gets JPEG_ENC_SHORT for the frames that do not fit, and nothing is written for them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_enc_math.h"
#include "jpeg_host.h"

namespace tstar {

enum {
    JPEG_ENC_OK = 0,
    JPEG_ENC_SHORT = 1,          // the buffer's capacity is short of this frame: nothing of the frame was written
    JPEG_ENC_BAD_COEF = 2,       // a coefficient outside what 8-bit baseline JPEG can code (scan stage fed foreign data)
    JPEG_ENC_HUFF_OVERFLOW = 3,  // optimised tables only: a code would be longer than 32 bits before limiting (libjpeg's
                                 // JERR_HUFF_CLEN_OVERFLOW); nothing of the frame is written
};

// counters of the scan stage (optional out-array of the host entries)
enum { JPEG_ENC_N_ZRL = 0, JPEG_ENC_N_NO_EOB = 1, JPEG_ENC_N_STUFFED = 2, JPEG_ENC_N_DUMMY_RIGHT = 3, JPEG_ENC_N_DUMMY_BOTTOM = 4, JPEG_ENC_N_COUNTERS = 5 };

constexpr int kJpegEncHeaderBytes = 623;      // 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14
constexpr int kJpegEncDriBytes = 6;           // FF DD 00 04 hi lo, directly before SOS when the scan has a restart interval

// Restart intervals (every entry below that takes `restart`: MCUs per interval, 0 = none, at most kJpegEncMaxRestart -- the
// DRI segment holds 16 bits).  What a scan with an interval holds: jpeg_enc_math.h, "scan order".  Counters of their
// own (optional, added to): markers written; intervals in front of a marker that ended on a byte boundary (no padding);
// padded bytes in front of a marker that came out as 0xFF (and were stuffed like any data byte).
constexpr int kJpegEncMaxRestart = 65535;
enum { JPEG_ENC_R_RST = 0, JPEG_ENC_R_PAD_FREE = 1, JPEG_ENC_R_PAD_FF = 2, JPEG_ENC_R_COUNTERS = 3 };
inline bool jpeg_enc_restart_ok(int restart) { return restart >= 0 && restart <= kJpegEncMaxRestart; }
inline int jpeg_enc_header_bytes(int restart) { return kJpegEncHeaderBytes + (restart > 0 ? kJpegEncDriBytes : 0); }

// Optimised tables (every entry below that takes `optimize`: 0 the four Annex K tables, 1 tables built from each frame's own symbol
// counts, Pillow's optimize=True; the procedure: jpeg_enc_math.h, "optimised tables").  The header then differs from frame to frame,
// in content and in length: its four DHT segments carry the frame's tables, each 2 + 2 + 17 + symbols bytes.
constexpr int kJpegEncHeaderDhtAt = 177;      // SOI, APP0, DQT x 2, SOF0: the bytes in front of the first DHT
constexpr int kJpegEncDhtMax = 2 + 2 + 17 + 256;
constexpr int kJpegEncHeaderOptMax = kJpegEncHeaderDhtAt + 4 * kJpegEncDhtMax + 14;        // without DRI
constexpr int kJpegEncSpecBytes = (int)sizeof(jpegenc::HuffSpecWide);                        // 276
static_assert(kJpegEncSpecBytes == 276, "HuffSpecWide is handed out as 276 bytes");
inline int jpeg_enc_header_bytes(int restart, int optimize) {
    return optimize ? kJpegEncHeaderOptMax + (restart > 0 ? kJpegEncDriBytes : 0) : jpeg_enc_header_bytes(restart);
}

// what the encoder covers: 3 components, luma sampling 2x2 / 2x1 / 1x1, 1 <= W, H <= 16384 (JpegGeom::valid() is the DECODER's
// coverage and is narrower: it leaves pictures with subsampled chroma at most 2 samples wide to Pillow)
bool jpeg_enc_geom_ok(const JpegGeom& g);
size_t jpeg_enc_max_scan_bytes(const JpegGeom& g);
// With a restart interval the bound grows by 4 bytes per marker: the padding in front of a marker adds less than one data byte
// (which stuffing can double), the marker itself two bytes that are never stuffed.
size_t jpeg_enc_restart_markers(const JpegGeom& g, int restart);
size_t jpeg_enc_max_scan_bytes(const JpegGeom& g, int restart);
// With optimised tables a block's bound is kMaxBlockBitsOpt: a DC code may then be 16 bits long.
size_t jpeg_enc_max_scan_bytes(const JpegGeom& g, int restart, int optimize);

// Launch plan of the device encoder (jpeg_enc.hip), pure: no HIP call, no global state; integers in, integers out.  The
// workspace of a chunk of n frames whose scans go into slots of slot_bytes bytes holds, 16-byte aligned one after another:
//   meta  u32 [n][4]          bits of the scan, unstuffed bytes, 0xFF bytes among them, flags
//   bits  u32 [n][blocks]     bit length of every block in scan order, then (scanned in place) its bit offset
//   raw   u32 [n][raw_words]  the unstuffed stream, big-endian words; min(slot_bytes, the bound) bytes: unstuffed bytes never
//                             exceed stuffed ones, so a frame that does not fit here does not fit its slot either
//   ff    u32 [n][ff_chunks]  0xFF bytes per chunk of kJpegEncStuffChunk raw bytes, then (scanned in place) the count before it
// and, with a restart interval only (the unstuffed stream then holds the padding and the markers too):
//   seg   u32 [n][markers + 1]  padded bits of every interval with its marker, then (scanned in place) its first bit
//   mark  u32 [n][markers]      byte offset of every marker in the unstuffed stream; bit 31: the byte in front of it is padded
// and, with optimised tables only:
//   hist   u32 [n][4][257]      symbol counts of the frame's four tables (DC luma, AC luma, DC chroma, AC chroma); [256] stays 0
//   codes  HuffCodes [n][4]     the code / length arrays the two passes of the bits kernel code with
constexpr int kJpegEncStuffChunk = 64;
struct JpegEncPlan {
    const char* error;          // non-null: the launchers refuse these arguments
    size_t blocks, coef_bytes, max_scan_bytes, header_bytes, workspace_bytes;
    size_t raw_words, ff_chunks;                       // per frame
    size_t off_meta, off_bits, off_raw, off_ff;        // byte offsets inside the workspace
    unsigned block_wgs;         // block stage: workgroups of 32 blocks over all frames
    unsigned entropy_wgs_x;     // entropy stage: workgroups of 256 blocks per frame (grid y = n)
    unsigned stuff_wgs_x;       // stuffing passes: workgroups of 256 chunks per frame (grid y = n)
    int restart;                // MCUs per restart interval, 0: none (then markers, off_seg and off_mark are 0)
    size_t markers;             // per frame
    size_t off_seg, off_mark;
    int optimize;               // 1: optimised tables (else off_hist and off_codes are 0)
    size_t off_hist, off_codes;
};
JpegEncPlan plan_jpeg_encode(const JpegGeom& g, int n, size_t slot_bytes, int restart = 0, int optimize = 0);

// quant u16 [3][64], natural order, rows Y / Cb / Cr (the decoder's table layout); quality 1..100
void jpeg_enc_quant(int quality, uint16_t* quant);
// the header of every frame of geometry g at this quality, with DRI in front of SOS when restart > 0: exactly
// jpeg_enc_header_bytes(restart) bytes
void jpeg_enc_header(const JpegGeom& g, int quality, int restart, uint8_t* out);
// the same layout with the DQT entries given (quant u16 [3][64], natural order, rows Y / Cb / Cr, every value 1..65535), for a
// file that is re-coded losslessly: two tables when the chroma rows are equal (what the header above writes), else three; a table
// with a value above 255 takes 16-bit entries and turns SOF0 into SOF1, as libjpeg writes it.  -> the bytes written, at most
// kJpegEncHeaderTablesMax.  For jpeg_enc_quant(quality)'s rows the bytes are jpeg_enc_header's.
constexpr int kJpegEncHeaderTablesMax = kJpegEncHeaderBytes + kJpegEncDriBytes + 69 + 3 * 64;       // a third table, 16-bit entries
size_t jpeg_enc_header_tables(const JpegGeom& g, const uint16_t* quant, int restart, uint8_t* out);
// the header of ONE frame coded with the four tables of `specs` (DC luma, AC luma, DC chroma, AC chroma): the layout above with
// these tables in the DHT segments -> the bytes written, at most jpeg_enc_header_bytes(restart, 1)
size_t jpeg_enc_header_opt(const JpegGeom& g, int quality, int restart, const jpegenc::HuffSpecWide* specs, uint8_t* out);
// both: the DQT entries of jpeg_enc_header_tables AND the four tables of jpeg_enc_header_opt, for a file that is re-coded losslessly
// with tables of its own -> the bytes written, at most kJpegEncHeaderTablesOptMax
constexpr int kJpegEncHeaderTablesOptMax = kJpegEncHeaderOptMax + kJpegEncDriBytes + 69 + 3 * 64;
size_t jpeg_enc_header_tables_opt(const JpegGeom& g, const uint16_t* quant, int restart, const jpegenc::HuffSpecWide* specs, uint8_t* out);

// stage 1, one frame: rgb u8 [H][W][3] -> coef int16 [g.blocks()][64]; dummy2 (optional) += {right-edge, bottom-edge} dummy blocks
void jpeg_enc_blocks(const uint8_t* rgb, const JpegGeom& g, const uint16_t* quant, int16_t* coef, uint64_t* dummy2);
// the scan order of g's coefficient layout, for the host twin and the kernels alike
inline jpegenc::ScanGeom scan_geom(const JpegGeom& g) {
    return jpegenc::ScanGeom{g.hs, g.vs, g.mcux(), g.mcuy(), g.bw(0), (int)g.block_offset(1), (int)g.block_offset(2)};
}
// stage 2, one frame, with a restart interval of `restart` MCUs: -> *len = the bytes the scan takes (with EOI), written to out
// only when they fit cap.  counters (optional, JPEG_ENC_N_*) and rst_counters (optional, JPEG_ENC_R_*) are added to, for frames
// that fit and frames that do not alike.
int jpeg_enc_scan(const int16_t* coef, const JpegGeom& g, int restart, uint8_t* out, size_t cap, size_t* len, uint64_t* counters,
                  uint64_t* rst_counters);

// Optimised tables, one frame.  The counts of the symbols the scan's walk emits, in its order (so the DC counts depend on the
// interval): hist u32 [4][257], overwritten.  -> JPEG_ENC_OK or JPEG_ENC_BAD_COEF.
int jpeg_enc_gather(const int16_t* coef, const JpegGeom& g, int restart, uint32_t* hist);
// gather, the four tables, the scan coded with them.  specs [4] out (always written; a spec's status names an overflow);
// hist (optional) u32 [4][257] out.  -> JPEG_ENC_*; with JPEG_ENC_HUFF_OVERFLOW *len is 0 and nothing is written.
int jpeg_enc_scan_opt(const int16_t* coef, const JpegGeom& g, int restart, uint8_t* out, size_t cap, size_t* len, jpegenc::HuffSpecWide* specs,
                      uint32_t* hist, uint64_t* counters, uint64_t* rst_counters);

// Shared tables: the frames of a GROUP are coded with ONE set of four tables, built from the sum of their symbol counts (the DC
// predictors restart with every frame, so the sum over frames is exact).  A group holds at most jpeg_enc_group_frames(blocks)
// frames: a block emits at most 64 symbols, so the sums stay within kHuffMaxCount and the u32 bins cannot wrap.
inline int jpeg_enc_group_frames(size_t blocks) {
    const size_t n = (size_t)jpegenc::kHuffMaxCount / (blocks * 64);
    return n < 1 ? 1 : (n > 0x7fffffff ? 0x7fffffff : (int)n);
}
// group i32 [n]: the group of every frame, -1 for a frame that is not coded (status JPEG_ENC_HUFF_OVERFLOW, length 0); the frames
// of a group are consecutive but for such frames, and group numbers do not decrease.  -> nullptr, or what is wrong; span i32
// [n_groups][2] out (optional): first frame and the frame behind the last of every group.
const char* jpeg_enc_groups_check(const int32_t* group, int n, int n_groups, size_t blocks, int32_t* span);

}  // namespace tstar
