// Baseline JPEG entropy decode of one SEGMENT: a run of MCUs that starts at a byte boundary with zero DC predictors (one
// restart interval, or a whole scan without DRI).  One core for both sides: g++ compiles this file as plain C++
// (jpeg_host.cpp: jpeg_entropy_segments_host, the sanitizer checker), hipcc as __host__ __device__ (jpeg_entropy.hip: one
// lane per segment).  Everything the decoder looks at lives in flat, pointer-free records (JpegTableSet, JpegSegment,
// JpegFrameDesc) that may sit in host memory, global memory or LDS.
//
// This code parses untrusted bytes, on the device next to other people's work:
//   - every byte read is inside the segment's [begin, end), which segment_table_set first checks against the byte buffer;
//   - every coefficient store is inside the segment's frame's own region of the coefficient buffer;
//   - the symbol loop is bounded by the bits of the segment (a symbol consumes at least one real bit or is an error).
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
// end.  Bits past that point read as zero so that table look-ahead is safe; CONSUMING one of them is the error.
struct BitReader {
    const uint8_t* d;
    uint32_t p, end;
    uint64_t acc;
    int nbits, fake;             // the lowest `fake` bits of acc are padding
    bool at_marker;

    // at most 8 rounds; afterwards nbits > 56: enough for one code (<= 16 bits) and its magnitude field (<= 11)
    TSTAR_JPEG_HD void fill() {
        while (nbits <= 56) {
            unsigned b = 0;
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
                        p += 2;
                    } else {
                        at_marker = true;                           // p stays on the FF
                    }
                }
            }
            if (at_marker) fake += 8;
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    TSTAR_JPEG_HD unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1)); }
    TSTAR_JPEG_HD bool skip(int n) {
        nbits -= n;
        return nbits >= fake;
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

// MCUs [first_mcu, first_mcu + n_mcu) of one frame out of bytes[begin, end) into coef (the FRAME's region, g.per_frame
// elements, already zero) -> JPEG_OK / JPEG_MALFORMED / JPEG_UNCOVERED.  The caller has checked begin <= end <= size of bytes
// and first_mcu + n_mcu <= g.n_mcu.
//
// One loop; an iteration decodes one Huffman symbol and its magnitude bits and refills the reader.  Which table (DC when
// k == 0, else AC, of the block's component), which predictor and which destination are picked by data, so lanes that sit
// at different places of different streams run the same instructions.  Tables may be in LDS or global memory (Tables is the
// pointer type the caller hands in).
template <class Tables>
TSTAR_JPEG_HD inline int decode_segment(const uint8_t* bytes, uint32_t begin, uint32_t end, Tables T, const JpegSegGeom& g,
                                        uint32_t first_mcu, uint32_t n_mcu, bool last, int16_t* coef) {
    BitReader br;
    br.d = bytes; br.p = begin; br.end = end; br.acc = 0; br.nbits = 0; br.fake = 0; br.at_marker = false;
    const uint32_t luma = g.hs * g.vs, bpm = g.ncomp == 3 ? luma + 2 : 1;      // blocks of an MCU; luma first
    uint32_t left = n_mcu;                                                      // MCUs not finished yet
    uint32_t mx = first_mcu % g.mcux, my = first_mcu / g.mcux;
    uint32_t j = 0;                                                             // block within the MCU
    int pred0 = 0, pred1 = 0, pred2 = 0;                                        // three scalars: an indexed array would live in scratch
    int k = 0;
    int64_t energy = 0;
    // a symbol consumes at least one real bit, so this many iterations read any segment to its end
    uint64_t budget = 8ull * (end - begin) + 1;
    int status = JPEG_OK;
    while (left != 0 && budget != 0) {
        --budget;
        // where this block lives: component c, block (bx, by) of the component's raster
        const uint32_t c = j < luma ? 0u : j - luma + 1;
        const uint32_t u = c == 0 ? j % g.hs : 0u, v = c == 0 ? j / g.hs : 0u;
        const uint32_t nh = c == 0 ? g.hs : 1u, nv = c == 0 ? g.vs : 1u;
        const uint32_t bw = c == 0 ? g.bw0 : g.bw1;
        const uint32_t base = c == 0 ? 0u : (c == 1 ? g.off1 : g.off2);
        const uint64_t blk = ((uint64_t)base + (uint64_t)(my * nv + v) * bw + (mx * nh + u)) * 64;
        if (blk + 64 > g.per_frame) { status = JPEG_MALFORMED; break; }        // never with a checked segment: the store bound
        br.fill();
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
                val += c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                if (val < -2048 || val > 2047) { status = JPEG_MALFORMED; break; }     // DC out of the 8-bit range
                pred0 = c == 0 ? val : pred0;
                pred1 = c == 1 ? val : pred1;
                pred2 = c == 2 ? val : pred2;
                energy = 0;
            } else {
                nat = T->zigzag[k] & 63;                                       // the table is data too: the store stays in the block
            }
            coef[blk + (uint32_t)nat] = (int16_t)val;
            const int q = (int)T->quant[64 * c + (uint32_t)nat];
            energy += (int64_t)(val * q) * (val * q);
            ++k;
            done = k == 64;
        }
        if (done) {
            if (energy > T->limit[c]) { status = JPEG_UNCOVERED; break; }      // more energy than 8-bit samples can carry
            k = 0;
            if (++j == bpm) {
                j = 0;
                --left;
                if (++mx == g.mcux) { mx = 0; ++my; }
            }
        }
    }
    if (status != JPEG_OK) return status;
    if (left != 0) return JPEG_MALFORMED;                                       // budget spent: not reachable, kept as the loop's bound
    // every block of the segment is decoded: less than a byte of padding may be left in front of the marker
    br.fill();
    if (!br.at_marker || br.nbits - br.fake >= 8) return last ? JPEG_UNCOVERED : JPEG_MALFORMED;
    return JPEG_OK;
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

}  // namespace jpegcore
}  // namespace tstar
