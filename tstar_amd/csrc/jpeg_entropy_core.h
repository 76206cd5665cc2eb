// Baseline JPEG entropy decode.  A SEGMENT is a run of MCUs that starts at a byte boundary with zero DC predictors (one
// restart interval, or a whole scan without DRI); a long segment may be cut into SUB-SEQUENCES of sub_bytes bytes, one lane
// each.  There is one symbol loop, walk_sub, in two forms:
//   walk_sub<false> (count form)  from a guessed or recorded state to the sub-sequence's limit: writes no coefficient, reports
//                                 the exit state, the blocks completed and the DC sums;
//   walk_sub<true>  (write form)  from a TRUE state with block index and predictors: stores coefficients under every check;
// and decode_segment, a wrapper: the write form from the segment's start state to its end, one lane per segment.
// One core for both sides: g++ compiles this file as plain C++ (jpeg_host.cpp: jpeg_entropy_segments_host,
// jpeg_entropy_split_host, the sanitizer checkers), hipcc as __host__ __device__ (jpeg_entropy.hip).  Everything the decoder
// looks at lives in flat, pointer-free records (JpegTableSet, JpegSegment, JpegFrameDesc) that may sit in host memory, global
// memory or LDS.
//
// This code parses untrusted bytes, on the device next to other people's work:
//   - every byte read is inside the segment's [begin, end), which segment_table_set first checks against the byte buffer;
//   - every coefficient store is inside the segment's frame's own region of the coefficient buffer;
//   - the symbol loop is bounded by the bits it may read (a symbol consumes at least one real bit or is an error).
// The checks of a block are those of decode_block in jpeg_host.cpp, which stays the yardstick: DC category <= 11 and DC
// range, AC category <= 10, run past 63, ZRL past 64, the energy bound, every table index before use.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_host.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TSTAR_JPEG_HD __host__ __device__
#else
#define TSTAR_JPEG_HD
#endif

namespace tstar {

// One Huffman table.  fast: 9-bit prefix -> (length << 8) | symbol, 0 when the code is longer than 9 bits.  Codes of
// length l > 9: code <= maxcode[l] (-1: none) selects vals[code + delta[l]], delta[l] = valptr[l] - mincode[l].
struct JpegHuffFlat {
    uint16_t fast[512];
    int32_t maxcode[18];
    int32_t delta[17];
    int32_t nvals;
    uint8_t vals[256];
};

// What the frames of a batch share by content: table h[2 * c] is component c's DC table, h[2 * c + 1] its AC table (the
// table of a symbol is picked by index, not by branch), the quantisation rows in natural order, the energy limit of a
// block of each component (computed on the host in double) and the zigzag order.
struct JpegTableSet {
    JpegHuffFlat h[6];
    uint16_t quant[192];
    uint8_t zigzag[64];
    int64_t limit[3];
};

struct JpegSegment {
    uint32_t frame;              // index into the frame descriptors and the coefficient buffer
    uint32_t begin, end;         // byte range in the batch's byte buffer; end = offset of the terminating marker's FF
    uint32_t first_mcu, n_mcu;
    uint32_t last;               // 1: the frame's last segment (bits left over are UNCOVERED, not MALFORMED)
};

struct JpegFrameDesc {
    int32_t table_set;           // -1: the frame was routed to the host decoder and has no segment
    int32_t first_segment, n_segments;
    int32_t reserved;
};

static_assert(sizeof(JpegHuffFlat) == 1424 && sizeof(JpegTableSet) == 9016 && sizeof(JpegSegment) == 24 && sizeof(JpegFrameDesc) == 16,
              "the flat records are part of the C ABI (include/tstar_hip.h)");

// The part of JpegGeom the decoder needs, as plain numbers (JpegGeom's methods are host code).
struct JpegSegGeom {
    uint32_t mcux, n_mcu;        // MCUs per row, MCUs per frame
    uint32_t ncomp, hs, vs;
    uint32_t bw0, bw1;           // blocks per row of luma / of a chroma component
    uint32_t off1, off2;         // first block of components 1 and 2 within a frame
    uint32_t per_frame;          // int16 elements of a frame's coefficient region (blocks * 64 < 2^32 for every valid geometry)
};

inline JpegSegGeom jpeg_seg_geom(const JpegGeom& g) {
    JpegSegGeom s;
    s.mcux = (uint32_t)g.mcux();
    s.n_mcu = (uint32_t)g.mcux() * (uint32_t)g.mcuy();
    s.ncomp = (uint32_t)g.ncomp; s.hs = (uint32_t)g.hs; s.vs = (uint32_t)g.vs;
    s.bw0 = (uint32_t)g.bw(0);
    s.bw1 = g.ncomp == 3 ? (uint32_t)g.bw(1) : 0;
    s.off1 = g.ncomp == 3 ? (uint32_t)g.block_offset(1) : 0;
    s.off2 = g.ncomp == 3 ? (uint32_t)g.block_offset(2) : 0;
    s.per_frame = (uint32_t)(g.blocks() * 64);
    return s;
}

namespace jpegcore {

// MSB-first bit reader over [p, end): removes FF00 stuffing, stops at a marker (an FF followed by anything but 00) or at
// end.  Bits past that point read as zero so that table look-ahead is safe; CONSUMING one of them is the error.  It also
// knows where its unread bits sit in the raw bytes: ff has one bit per byte pushed, newest lowest, set when that byte was
// an FF followed by its stuffed 00.
struct BitReader {
    const uint8_t* d;
    uint32_t p, end;
    uint64_t acc;
    int nbits, fake;             // the lowest `fake` bits of acc are padding
    uint32_t ff;
    bool at_marker;

    TSTAR_JPEG_HD BitReader(const uint8_t* bytes, uint32_t at, uint32_t stop)
        : d(bytes), p(at), end(stop), acc(0), nbits(0), fake(0), ff(0), at_marker(false) {}
    // at most 8 rounds; afterwards nbits > 56: enough for one code (<= 16 bits) and its magnitude field (<= 11)
    TSTAR_JPEG_HD void fill() {
        while (nbits <= 56) {
            unsigned b = 0, stuffed = 0;
            if (!at_marker) {
                if (p >= end) {
                    at_marker = true;
                } else {
                    const unsigned x = d[p];
                    if (x != 0xFF) {
                        b = x;
                        ++p;
                    } else if (p + 1 < end && d[p + 1] == 0x00) {
                        b = 0xFF;
                        stuffed = 1;
                        p += 2;
                    } else {
                        at_marker = true;                           // p stays on the FF
                    }
                }
            }
            if (at_marker) fake += 8;
            acc = (acc << 8) | b;
            ff = (ff << 1) | stuffed;
            nbits += 8;
        }
    }
    TSTAR_JPEG_HD unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1)); }
    TSTAR_JPEG_HD bool skip(int n) {
        nbits -= n;
        return nbits >= fake;
    }
    // the next unread bit (no padding bit has been consumed: nbits >= fake): byte offset and bit within it
    TSTAR_JPEG_HD void where(uint32_t* byte, uint32_t* bit) const {
        const uint32_t real = (uint32_t)(nbits - fake), nb = (real + 7) >> 3, nf = (uint32_t)fake >> 3;
        const uint32_t stuffed = (uint32_t)__builtin_popcount((ff >> nf) & ((1u << nb) - 1));       // nb <= 8, nf <= 8
        *byte = p - nb - stuffed;
        *bit = (8 - (real & 7)) & 7;
    }
};

// One symbol of table t (the reader is filled): the fast table, then the long-code path of 10 to 16 bits.  -1: no code of
// any length matches, a table index out of range, or the data ends inside the code.
template <class Table>
TSTAR_JPEG_HD inline int huff_decode(BitReader& br, const Table* t) {
    const unsigned f = t->fast[br.peek(9)];
    if (f) {
        if (!br.skip((int)(f >> 8))) return -1;
        return (int)(f & 255);
    }
    int32_t code = (int32_t)br.peek(10);
    int l = 10;
    while (l <= 16 && code > t->maxcode[l]) {
        ++l;
        if (l <= 16) code = (int32_t)br.peek(l);
    }
    if (l > 16) return -1;
    const int idx = code + t->delta[l];
    if (idx < 0 || idx >= t->nvals || idx > 255) return -1;
    if (!br.skip(l)) return -1;
    return t->vals[idx];
}

// Everything a launch (or the host loop) hands to every segment.
struct SegmentBatch {
    const uint8_t* bytes;
    uint64_t total_bytes;
    const JpegSegment* segments;
    const JpegTableSet* tables;
    const JpegFrameDesc* frames;
    uint32_t n_sets, n_frames, n_segments;
    JpegSegGeom g;
    int16_t* coef;               // [n_frames][g.per_frame]
    int32_t* seg_status;         // [n_segments]
};

// The one place that checks an entry point's arguments and fills the batch (host code, like jpeg_seg_geom) -> nullptr, or
// what is wrong, for the entry point to report under its own name.  total_bytes is the callee's to check.
inline const char* segment_batch(const uint8_t* bytes, size_t total_bytes, const void* segments, const void* tables, int n_sets,
                                 const void* frames, int n_frames, int n_segments, const JpegGeom& g, int16_t* coef,
                                 int32_t* seg_status, SegmentBatch* b) {
    if (!bytes || !segments || !tables || !frames || !coef || !seg_status) return "null argument";
    if (n_sets <= 0 || n_frames <= 0 || n_segments <= 0) return "empty batch";
    if (!g.valid()) return "unsupported geometry";
    b->bytes = bytes; b->total_bytes = total_bytes;
    b->segments = (const JpegSegment*)segments; b->tables = (const JpegTableSet*)tables; b->frames = (const JpegFrameDesc*)frames;
    b->n_sets = (uint32_t)n_sets; b->n_frames = (uint32_t)n_frames; b->n_segments = (uint32_t)n_segments;
    b->g = jpeg_seg_geom(g);
    b->coef = coef; b->seg_status = seg_status;
    return nullptr;
}

// The segment list is checked like the stream: a record that points outside the batch is MALFORMED and touches nothing.
// Returns the table set of a usable segment, -1 otherwise.
TSTAR_JPEG_HD inline int segment_table_set(const SegmentBatch& b, const JpegSegment& s) {
    if (s.frame >= b.n_frames) return -1;
    if (s.begin > s.end || s.end > b.total_bytes) return -1;
    if (s.n_mcu == 0 || s.first_mcu >= b.g.n_mcu || s.n_mcu > b.g.n_mcu - s.first_mcu) return -1;
    const int32_t ts = b.frames[s.frame].table_set;
    if (ts < 0 || (uint32_t)ts >= b.n_sets) return -1;
    return ts;
}

// ------------------------------------------------------------------------------------------------ sub-sequences
// A long segment is cut into SUB-SEQUENCES of sub_bytes bytes, one lane each (self-synchronising Huffman decoding:
// Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).  A decoder STATE is where the next
// symbol starts (byte offset in the batch's byte buffer and bit within that byte; the byte is never the 00 of an FF 00
// pair), the block within the MCU j, the zigzag index k and the AC energy of the open block.  Sub-sequence i of a segment
// decodes from an entry state to the first symbol that starts at or behind its byte limit and records that exit state;
// started from a guess, it falls into step with the true symbol sequence after some symbols, so rounds in which every
// sub-sequence starts from its predecessor's last exit reach the sequential decoder's states.
//
// walk_sub<false> (count form) writes no coefficient: it reports the exit state, the blocks completed and the sum of the DC
// differences of each component (mod 2^32).  A bad code is no error there, only "no exit state".  It cannot check the DC
// range or the energy of a block (both need the predictors) and does not try.
// walk_sub<true> (write form) is the same walk from a TRUE entry state with the predictors and the block index in front of
// it: it stores coefficients and applies every check of a block.  The energy of a block is the AC terms as they come plus
// the DC term when the block completes; the DC of a block opened in an earlier sub-sequence is the entry predictor of its
// component, so the energy check needs no second pass.  The sub-sequence in which the segment's last block completes
// checks the padding in front of the marker; sub-sequences behind it have nothing to do.
constexpr uint32_t kSubBytesMin = 8;           // TSTAR_JPEG_SUB_BYTES_MIN (include/tstar_hip.h)
constexpr uint32_t kSubValid = 1u << 14;       // SubState::pk = bit | j << 3 | k << 7 | kSubValid

struct SubState {
    uint32_t pos, pk;
    int64_t energy;
};

TSTAR_JPEG_HD inline bool sub_state_equal(const SubState& a, const SubState& b) { return a.pos == b.pos && a.pk == b.pk && a.energy == b.energy; }

struct SubCount {
    uint32_t blocks, dc0, dc1, dc2;
};

// Where sub-sequence i > 0 of a segment starts when nothing is known: its own first byte, or the byte behind it when that
// first byte is the 00 of an FF 00 pair (in entropy data an FF is always followed by 00).  at < end.
TSTAR_JPEG_HD inline SubState sub_blank_state(const uint8_t* bytes, uint32_t begin, uint32_t at) {
    SubState s;
    s.pos = (at > begin && bytes[at - 1] == 0xFF && bytes[at] == 0x00) ? at + 1 : at;
    s.pk = kSubValid;
    s.energy = 0;
    return s;
}

// What a write-form walk knows beyond the entry state.
struct SubWrite {
    uint32_t first_mcu, seg_blocks;            // the segment's first MCU and its blocks (n_mcu * blocks of an MCU)
    uint32_t first_block;                      // blocks of the segment completed in front of this sub-sequence
    int pred0, pred1, pred2;
    bool last_sub, last_seg;                   // the segment's last sub-sequence; the frame's last segment
    int16_t* coef;                             // the FRAME's region
};

// One sub-sequence: symbols from `in` (a valid state with begin <= pos <= end) up to the first one that starts at or
// behind byte `lim` (<= end).  Reads stay inside [begin, end); the loop is bounded by the bits of [in.pos, lim) plus one
// symbol (write form of the segment's last sub-sequence: lim = end).
// One loop; an iteration decodes one Huffman symbol and its magnitude bits and refills the reader.  Which table (DC when
// k == 0, else AC, of the block's component), which predictor and which destination are picked by data, so lanes that sit
// at different places of different streams run the same instructions.  Tables may be in LDS or global memory (Tables is the
// pointer type the caller hands in).
//   count form: *out = the exit state (pk == 0: none), *cnt the blocks completed and DC sums; returns JPEG_OK.
//   write form: returns the status; *out and *cnt are not written.
template <bool kWrite, class Tables>
TSTAR_JPEG_HD inline int walk_sub(const uint8_t* bytes, uint32_t end, uint32_t lim, Tables T, const JpegSegGeom& g, const SubState& in,
                                  const SubWrite* w, SubState* out, SubCount* cnt) {
    const uint32_t luma = g.hs * g.vs, bpm = g.ncomp == 3 ? luma + 2 : 1;
    uint32_t j = (in.pk >> 3) & 15;
    int k = (int)((in.pk >> 7) & 127);
    int64_t energy = in.energy;                                                 // AC terms of the open block
    if (kWrite) {
        if (w->first_block >= w->seg_blocks) return JPEG_OK;                    // behind the segment's last block: nothing to do
        if (j != w->first_block % bpm) return JPEG_MALFORMED;                   // never with a true state
    }
    if (j >= bpm || k > 63) {                                                   // never with a state this code recorded
        if (!kWrite) { out->pos = 0; out->pk = 0; out->energy = 0; cnt->blocks = cnt->dc0 = cnt->dc1 = cnt->dc2 = 0; }
        return JPEG_MALFORMED;
    }
    BitReader br(bytes, in.pos, end);
    br.fill();
    bool bad = !br.skip((int)(in.pk & 7));                                      // the bits of the first byte in front of the state
    uint32_t left = 0, mx = 0, my = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;                                        // three scalars: an indexed array would live in scratch
    if (kWrite) {
        left = w->seg_blocks - w->first_block;
        const uint32_t m = w->first_mcu + w->first_block / bpm;
        mx = m % g.mcux; my = m / g.mcux;
        pred0 = w->pred0; pred1 = w->pred1; pred2 = w->pred2;
        // the sequential decoder never carries a predictor outside the DC range: an earlier sub-sequence has refused the segment
        if (pred0 < -2048 || pred0 > 2047 || pred1 < -2048 || pred1 > 2047 || pred2 < -2048 || pred2 > 2047) return JPEG_MALFORMED;
    }
    uint32_t blocks = 0, dc0 = 0, dc1 = 0, dc2 = 0;
    const bool to_end = kWrite && w->last_sub;                                  // runs into the end of the data
    uint64_t budget = (in.pos <= lim ? 8ull * (lim - in.pos) : 0) + 1;     // a state already behind lim is its own exit
    int status = JPEG_OK;
    bool have_exit = false;
    uint32_t xb = 0, xbit = 0;
    while (!bad && budget != 0) {
        --budget;
        br.fill();
        if (!to_end) {
            br.where(&xb, &xbit);
            if (xb >= lim) { have_exit = true; break; }
        }
        const uint32_t c = j < luma ? 0u : j - luma + 1;
        uint64_t blk = 0;
        if (kWrite) {                                                           // where this block lives: block (bx, by) of component c's raster
            const uint32_t u = c == 0 ? j % g.hs : 0u, v = c == 0 ? j / g.hs : 0u;
            const uint32_t nh = c == 0 ? g.hs : 1u, nv = c == 0 ? g.vs : 1u;
            const uint32_t bw = c == 0 ? g.bw0 : g.bw1;
            const uint32_t base = c == 0 ? 0u : (c == 1 ? g.off1 : g.off2);
            blk = ((uint64_t)base + (uint64_t)(my * nv + v) * bw + (mx * nh + u)) * 64;
            if (blk + 64 > g.per_frame) { status = JPEG_MALFORMED; break; }    // never with a checked segment: the store bound
        }
        const bool dc = k == 0;
        const int sym = huff_decode(br, &T->h[2 * c + (dc ? 0 : 1)]);
        if (sym < 0) { status = JPEG_MALFORMED; break; }                        // bad code or data ends inside a code
        const int r = dc ? 0 : sym >> 4, s = dc ? sym : sym & 15;
        if (s > (dc ? 11 : 10)) { status = JPEG_MALFORMED; break; }            // magnitude category
        bool done = false;
        if (!dc && s == 0) {
            if (r == 15) {
                k += 16;
                if (k > 64) { status = JPEG_MALFORMED; break; }                 // zero run past the end of the block
                done = k == 64;
            } else if (r != 0) {
                status = JPEG_MALFORMED;                                        // end-of-band run in a sequential scan
                break;
            } else {
                done = true;                                                    // EOB: the rest stays zero
            }
        } else {
            k += r;
            if (k > 63) { status = JPEG_MALFORMED; break; }                    // coefficient index past the end of the block
            int val = 0;
            if (s) {
                const int bits = (int)br.peek(s);
                if (!br.skip(s)) { status = JPEG_MALFORMED; break; }           // data ends inside a value
                val = bits < (1 << (s - 1)) ? bits - (1 << s) + 1 : bits;       // T.81 F.2.2.1 EXTEND
            }
            int nat = 0;
            if (dc) {
                dc0 += c == 0 ? (uint32_t)val : 0u;
                dc1 += c == 1 ? (uint32_t)val : 0u;
                dc2 += c == 2 ? (uint32_t)val : 0u;
                if (kWrite) {
                    val += c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                    if (val < -2048 || val > 2047) { status = JPEG_MALFORMED; break; }     // DC out of the 8-bit range
                    pred0 = c == 0 ? val : pred0;
                    pred1 = c == 1 ? val : pred1;
                    pred2 = c == 2 ? val : pred2;
                }
                energy = 0;
            } else {
                nat = T->zigzag[k] & 63;                                       // the table is data too: the store stays in the block
                const int q = (int)T->quant[64 * c + (uint32_t)nat];
                energy += (int64_t)(val * q) * (val * q);
            }
            if (kWrite) w->coef[blk + (uint32_t)nat] = (int16_t)val;
            ++k;
            done = k == 64;
        }
        if (done) {
            if (kWrite) {
                const int d = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);       // this block's DC, wherever the block was opened
                const int q = (int)T->quant[64 * c];
                if (energy + (int64_t)(d * q) * (d * q) > T->limit[c]) { status = JPEG_UNCOVERED; break; }   // more than 8-bit samples can carry
            }
            k = 0;
            energy = 0;
            ++blocks;
            if (++j == bpm) {
                j = 0;
                if (kWrite && ++mx == g.mcux) { mx = 0; ++my; }
            }
            if (kWrite && --left == 0) break;
        }
    }
    if (!kWrite) {
        cnt->blocks = blocks; cnt->dc0 = dc0; cnt->dc1 = dc1; cnt->dc2 = dc2;
        out->pos = 0; out->pk = 0; out->energy = 0;
        if (have_exit) {
            out->pos = xb;
            out->pk = xbit | j << 3 | (uint32_t)k << 7 | kSubValid;
            out->energy = energy;
        }
        return JPEG_OK;
    }
    if (bad) return JPEG_MALFORMED;
    if (status != JPEG_OK) return status;
    if (left != 0) return w->last_sub ? JPEG_MALFORMED : (have_exit ? JPEG_OK : JPEG_MALFORMED);
    // every block of the segment is decoded: less than a byte of padding may be left in front of the marker
    br.fill();
    if (!br.at_marker || br.nbits - br.fake >= 8) return w->last_seg ? JPEG_UNCOVERED : JPEG_MALFORMED;
    return JPEG_OK;
}

// The start of a segment is a true state: its first byte, block 0, no open block.
TSTAR_JPEG_HD inline SubState sub_start_state(uint32_t begin) {
    SubState s;
    s.pos = begin; s.pk = kSubValid; s.energy = 0;
    return s;
}

// One lane per segment: MCUs [first_mcu, first_mcu + n_mcu) of one frame out of bytes[begin, end) into coef (the FRAME's
// region, g.per_frame elements, already zero) -> JPEG_OK / JPEG_MALFORMED / JPEG_UNCOVERED.  The caller has checked
// begin <= end <= size of bytes and 0 < n_mcu, first_mcu + n_mcu <= g.n_mcu (segment_table_set).  The write form from the
// segment's start state, as the segment's only and last sub-sequence.
template <class Tables>
TSTAR_JPEG_HD inline int decode_segment(const uint8_t* bytes, uint32_t begin, uint32_t end, Tables T, const JpegSegGeom& g,
                                        uint32_t first_mcu, uint32_t n_mcu, bool last, int16_t* coef) {
    SubWrite w;
    w.first_mcu = first_mcu; w.seg_blocks = n_mcu * (g.ncomp == 3 ? g.hs * g.vs + 2 : 1); w.first_block = 0;
    w.pred0 = w.pred1 = w.pred2 = 0;
    w.last_sub = true; w.last_seg = last;
    w.coef = coef;
    return walk_sub<true>(bytes, end, end, T, g, sub_start_state(begin), &w, (SubState*)nullptr, (SubCount*)nullptr);
}

// The caller-sized workspace of a split call, structure of arrays over `cap` sub-sequences and n segments:
//   per sub-sequence  exit state, two copies (round r reads copy (r - 1) & 1 and writes copy r & 1): pos, pk, energy;
//                     changed in that round, two copies; blocks, dc0..2 (count form); first block, pred0..2 (scan)
//   per segment       sub-sequences (0: not split), first sub-sequence, the last round that changed an exit;
//   one word          sub-sequences in all.
struct SplitWs {
    int64_t* energy[2];
    uint32_t *pos[2], *pk[2], *chg[2];
    uint32_t *blocks, *dc0, *dc1, *dc2, *first_block, *pred0, *pred1, *pred2;
    uint32_t *n_sub, *sub_first, *last_changed, *total;
    uint32_t cap;
};

// cap: no list of disjoint segments inside total_bytes has more sub-sequences
TSTAR_JPEG_HD inline uint64_t split_cap(uint64_t total_bytes, uint64_t n_segments, uint32_t sub_bytes) {
    return total_bytes / sub_bytes + n_segments;
}
TSTAR_JPEG_HD inline uint64_t split_ws_bytes(uint64_t cap, uint64_t n_segments) { return (cap * (16 + 14 * 4) + n_segments * 12 + 16 + 7) & ~7ull; }

inline SplitWs split_ws_carve(void* base, uint64_t cap, uint64_t n_segments) {
    SplitWs w;
    int64_t* e = (int64_t*)base;                                                // base is 8-byte aligned
    w.energy[0] = e; w.energy[1] = e + cap;
    uint32_t* u = (uint32_t*)(e + 2 * cap);
    uint32_t** lanes[14] = {&w.pos[0], &w.pos[1], &w.pk[0], &w.pk[1], &w.chg[0], &w.chg[1], &w.blocks, &w.dc0, &w.dc1, &w.dc2,
                            &w.first_block, &w.pred0, &w.pred1, &w.pred2};
    for (int i = 0; i < 14; ++i) { *lanes[i] = u; u += cap; }
    w.n_sub = u; u += n_segments;
    w.sub_first = u; u += n_segments;
    w.last_changed = u; u += n_segments;
    w.total = u;
    w.cap = (uint32_t)cap;
    return w;
}

TSTAR_JPEG_HD inline SubState split_ws_load(const SplitWs& w, uint32_t copy, uint32_t lane) {
    SubState s;
    s.pos = w.pos[copy][lane]; s.pk = w.pk[copy][lane]; s.energy = w.energy[copy][lane];
    return s;
}
TSTAR_JPEG_HD inline void split_ws_store(const SplitWs& w, uint32_t copy, uint32_t lane, const SubState& s) {
    w.pos[copy][lane] = s.pos; w.pk[copy][lane] = s.pk; w.energy[copy][lane] = s.energy;
}

// Is segment s cut into sub-sequences, and into how many?  0: one lane.
TSTAR_JPEG_HD inline uint32_t split_n_sub(const SegmentBatch& b, const JpegSegment& s, uint32_t sub_bytes, uint32_t min_split_bytes) {
    if (min_split_bytes == 0 || segment_table_set(b, s) < 0) return 0;
    const uint32_t len = s.end - s.begin;
    if (len < min_split_bytes) return 0;
    return (len - 1) / sub_bytes + 1;
}

// Same entry as last round, same exit: after round 0 the segment's first sub-sequence (at lane `first`), and one whose
// predecessor's exit did not change in the round before, copy their exit and are done.  Returns whether `lane` was one.
TSTAR_JPEG_HD inline bool split_round_copies(const SplitWs& w, uint32_t round, uint32_t first, uint32_t lane) {
    const uint32_t in = (round + 1) & 1, o = round & 1;
    if (round == 0 || (lane != first && w.chg[in][lane - 1] != 0)) return false;
    split_ws_store(w, o, lane, split_ws_load(w, in, lane));
    w.chg[o][lane] = 0;
    return true;
}

// Sub-sequence `lane` (i of segment `si`) in round `round`: round 0 starts from nothing, a later round from the exit its
// predecessor recorded in the round before, and only when that exit changed then.  Returns whether its own exit changed.
template <class Tables>
TSTAR_JPEG_HD inline bool split_round_lane(const SegmentBatch& b, const SplitWs& w, uint32_t sub_bytes, uint32_t round, uint32_t si,
                                           uint32_t lane, Tables T) {
    const JpegSegment s = b.segments[si];
    const uint32_t i = lane - w.sub_first[si], n = w.n_sub[si];
    const uint32_t in = (round + 1) & 1, o = round & 1;
    if (split_round_copies(w, round, w.sub_first[si], lane)) return false;
    const uint32_t at = s.begin + i * sub_bytes;
    SubState e;
    if (i == 0) {
        e = sub_start_state(s.begin);
    } else if (round == 0) {
        e = sub_blank_state(b.bytes, s.begin, at);
    } else {
        e = split_ws_load(w, in, lane - 1);
        if (!(e.pk & kSubValid) || e.pos < s.begin || e.pos > s.end) e = sub_blank_state(b.bytes, s.begin, at);
    }
    const uint32_t lim = i + 1 == n ? s.end : at + sub_bytes;
    SubState x;
    SubCount c;
    walk_sub<false>(b.bytes, s.end, lim, T, b.g, e, (const SubWrite*)nullptr, &x, &c);
    const bool changed = round == 0 || !sub_state_equal(split_ws_load(w, in, lane), x);
    split_ws_store(w, o, lane, x);
    w.chg[o][lane] = changed ? 1u : 0u;
    w.blocks[lane] = c.blocks; w.dc0[lane] = c.dc0; w.dc1[lane] = c.dc1; w.dc2[lane] = c.dc2;
    if (changed && round != 0) w.last_changed[si] = round;                     // every writer of a round stores the same value
    return changed;
}

// seg_info of a split segment after rounds 0 .. max_rounds: the first round that changed none of its exits, or -1
TSTAR_JPEG_HD inline int32_t split_seg_info(const SplitWs& w, uint32_t si, uint32_t max_rounds) {
    if (w.n_sub[si] == 0) return 0;
    const uint32_t r = w.last_changed[si] + 1;
    return r <= max_rounds ? (int32_t)r : -1;
}

// Sub-sequence `lane` of converged segment si in the write pass -> its status
template <class Tables>
TSTAR_JPEG_HD inline int split_write_lane(const SegmentBatch& b, const SplitWs& w, uint32_t sub_bytes, uint32_t max_rounds, uint32_t si,
                                          uint32_t lane, Tables T) {
    const JpegSegment s = b.segments[si];
    const uint32_t i = lane - w.sub_first[si], n = w.n_sub[si], f = max_rounds & 1;
    const uint32_t luma = b.g.hs * b.g.vs, bpm = b.g.ncomp == 3 ? luma + 2 : 1;
    const SubState e = i == 0 ? sub_start_state(s.begin) : split_ws_load(w, f, lane - 1);
    SubWrite sw;
    sw.first_mcu = s.first_mcu; sw.seg_blocks = s.n_mcu * bpm; sw.first_block = w.first_block[lane];
    sw.pred0 = (int)w.pred0[lane]; sw.pred1 = (int)w.pred1[lane]; sw.pred2 = (int)w.pred2[lane];
    sw.last_sub = i + 1 == n; sw.last_seg = s.last != 0;
    sw.coef = b.coef + (size_t)s.frame * b.g.per_frame;
    if (sw.first_block >= sw.seg_blocks) return JPEG_OK;
    if (!(e.pk & kSubValid) || e.pos < s.begin || e.pos > s.end) return JPEG_MALFORMED;   // the predecessor met a bad code
    const uint32_t lim = sw.last_sub ? s.end : s.begin + (i + 1) * sub_bytes;
    return walk_sub<true>(b.bytes, s.end, lim, T, b.g, e, &sw, (SubState*)nullptr, (SubCount*)nullptr);
}

}  // namespace jpegcore
}  // namespace tstar
