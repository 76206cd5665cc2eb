// The integer arithmetic of the baseline JPEG encoder, stated once for the host twin (jpeg_enc_host.cpp) and the kernels
// (jpeg_enc.hip): libjpeg-turbo as Pillow drives it -- 16-bit fixed-point RGB -> YCbCr, the h2v2 / h2v1 box downsamplers with
// their alternating bias, libjpeg's accurate integer forward DCT (Loeffler-Ligtenberg-Moschytz, the twelve constants x 2^13
// that jpeg_math.h::idct8 uses), the rounding quantiser, the quality -> table rule, the four Annex K Huffman tables as
// code / length arrays, the symbol walk of one block, and the tables Pillow's optimize=True builds from a frame's own symbol
// counts.  Geometry and coefficient layout are JpegGeom's (jpeg_host.h).
#pragma once
#include <stdint.h>

#include "jpeg_math.h"

namespace tstar {
namespace jpegenc {

// ---------------------------------------------------------------------------------------------- colour (FIX(x) = int(x * 65536 + 0.5))
TSTAR_JHD int rgb_to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
TSTAR_JHD int rgb_to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
TSTAR_JHD int rgb_to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
// c: 0 Y, 1 Cb, 2 Cr
TSTAR_JHD int rgb_to_comp(int c, int r, int g, int b) { return c == 0 ? rgb_to_y(r, g, b) : (c == 1 ? rgb_to_cb(r, g, b) : rgb_to_cr(r, g, b)); }

// ---------------------------------------------------------------------------------------------- edges and downsampling
// Bias of the box filters by OUTPUT column: h2v2 1, 2, 1, 2, ...; h2v1 0, 1, 0, 1, ...
TSTAR_JHD int h2v2_bias(int ox) { return 1 + (ox & 1); }
TSTAR_JHD int h2v1_bias(int ox) { return ox & 1; }

// Output row of a component that a block row reads: luma replicates the last picture row; chroma replicates the last
// DOWNSAMPLED row (ch = ceil(H / vs) of them), whose own input rows are replicated only up to the next multiple of vs.
TSTAR_JHD int comp_row(int c, int oy, int H, int vs) {
    const int rows = c == 0 ? H : (H + vs - 1) / vs;
    return oy < rows ? oy : rows - 1;
}

// Sample (oy, ox) of component c (block coordinates times 8 plus the position inside the block; any non-negative value: the
// edges are replicated by clamping the coordinate) of an RGB u8 frame [H][W][3].  The plain statement; the kernel's vector
// path computes the same integers.
TSTAR_JHD int sample_at(const uint8_t* rgb, int W, int H, int hs, int vs, int c, int oy, int ox) {
    const int fh = c == 0 ? 1 : hs, fv = c == 0 ? 1 : vs;
    oy = comp_row(c, oy, H, vs);
    int sum = 0;
    for (int j = 0; j < fv; ++j) {
        const int y = jpegmath::clampi(oy * fv + j, 0, H - 1);
        for (int i = 0; i < fh; ++i) {
            const int x = jpegmath::clampi(ox * fh + i, 0, W - 1);
            const uint8_t* p = rgb + ((size_t)y * W + x) * 3;
            sum += rgb_to_comp(c, p[0], p[1], p[2]);
        }
    }
    if (fh == 1) return sum;
    return fv == 2 ? (sum + h2v2_bias(ox)) >> 2 : (sum + h2v1_bias(ox)) >> 1;
}

// ---------------------------------------------------------------------------------------------- forward DCT
// One 8-point pass of jfdctint.c.  Row pass (first): even outputs 0 / 4 shifted LEFT by 2, the rest descaled by 13 - 2.
// Column pass: outputs 0 / 4 descaled by 2, the rest by 13 + 2.  The result of both is 8 x the true DCT.
template <bool ROWPASS>
TSTAR_JHD void fdct8(const int32_t d[8], int32_t out[8]) {
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int odd = ROWPASS ? 13 - 2 : 13 + 2;
    if (ROWPASS) {
        out[0] = (t10 + t11) * 4;
        out[4] = (t10 - t11) * 4;
    } else {
        out[0] = jpegmath::descale((uint32_t)(t10 + t11), 2);
        out[4] = jpegmath::descale((uint32_t)(t10 - t11), 2);
    }
    int32_t z1 = (t12 + t13) * 4433;
    out[2] = jpegmath::descale((uint32_t)(z1 + t13 * 6270), odd);
    out[6] = jpegmath::descale((uint32_t)(z1 - t12 * 15137), odd);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    out[7] = jpegmath::descale((uint32_t)(a4 + z1 + z3), odd);
    out[5] = jpegmath::descale((uint32_t)(a5 + z2 + z4), odd);
    out[3] = jpegmath::descale((uint32_t)(a6 + z2 + z3), odd);
    out[1] = jpegmath::descale((uint32_t)(a7 + z1 + z4), odd);
}

// ---------------------------------------------------------------------------------------------- quantisation
// v: a DCT output (8 x the true coefficient); q: the table entry (1..255)
TSTAR_JHD int quantise(int v, int q) {
    const int d = 8 * q;
    const int a = v < 0 ? -v : v;
    const int r = (a + (d >> 1)) / d;
    return v < 0 ? -r : r;
}

// Annex K.1 / K.2, natural order
struct StdTables {
    uint8_t q[2][64];
    uint8_t zigzag[64];          // zigzag[k] = natural index of the k-th coefficient of the scan
};
constexpr StdTables kStd = {
    {{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
     {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}},
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}};

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): quality 1..100 -> table t (0 luma, 1 chroma), natural order
TSTAR_JHD int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
TSTAR_JHD int quant_entry(int std_value, int scale) { return jpegmath::clampi((std_value * scale + 50) / 100, 1, 255); }

// ---------------------------------------------------------------------------------------------- Huffman tables (Annex K.3 - K.6)
struct HuffSpec {
    uint8_t bits[16];            // codes of length 1..16
    uint8_t vals[162];
    int nvals;
};
struct HuffCodes {
    uint16_t code[256];
    uint8_t len[256];            // 0: the table has no code for this symbol
};
struct EncTables {
    HuffSpec spec[4];            // DC luma, AC luma, DC chroma, AC chroma (the order of the DHT segments)
    HuffCodes codes[4];
};

constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

// canonical code assignment (Annex C): codes of one length count up, the next length continues from twice the last + 2
constexpr HuffCodes make_codes(const HuffSpec& s) {
    HuffCodes h = {};
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1]; ++i, ++k) {
            h.code[s.vals[k]] = (uint16_t)code++;
            h.len[s.vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
    return h;
}
constexpr EncTables make_tables() {
    EncTables t = {{kDcLuma, kAcLuma, kDcChroma, kAcChroma}, {}};
    for (int i = 0; i < 4; ++i) t.codes[i] = make_codes(t.spec[i]);
    return t;
}

// Bits a block can take at most with these tables and 8-bit samples: a DC symbol of 11 + 11 bits and 63 AC symbols of
// 16 + 10 bits (no ZRL fits between them).  Stuffing can double the bytes.
constexpr int kMaxBlockBits = 22 + 63 * 26;

// ---------------------------------------------------------------------------------------------- symbols of one block
// size category of a value: the bit length of |v|
TSTAR_JHD int category(int v) {
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}
// magnitude bits: v for v >= 0, the low n bits of v - 1 otherwise
TSTAR_JHD unsigned magnitude_bits(int v, int n) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// what a block's walk saw (the host twin sums them; the tests prove their inputs reach each path)
struct BlockEvents {
    int zrl, no_eob, bad;        // ZRL symbols; 1 when coefficient 63 is non-zero; 1 when a value has no code (outside 8-bit JPEG)
};

// The symbol walk of one block: coef [64] natural order, pred the quantised DC of the previous block of the component,
// dc / ac the component's code tables.  put(code, len) is called for every code and every run of magnitude bits (len 1..16),
// MSB first.  Both sides run this walk: a counting put gives the block's length, a writing put its bits.
template <class Put>
TSTAR_JHD BlockEvents encode_block(const int16_t* coef, int pred, const HuffCodes& dc, const HuffCodes& ac, const uint8_t* zigzag, Put&& put) {
    BlockEvents ev = {0, 0, 0};
    const int diff = (int)coef[0] - pred;
    int n = category(diff);
    if (n > 11) { ev.bad = 1; n = 11; }
    put((unsigned)dc.code[n], (int)dc.len[n]);
    if (n) put(magnitude_bits(diff, n), n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = coef[zigzag[k]];
        if (v == 0) { ++run; continue; }
        while (run > 15) {
            put((unsigned)ac.code[0xF0], (int)ac.len[0xF0]);
            run -= 16;
            ++ev.zrl;
        }
        int s = category(v);
        if (s > 10) { ev.bad = 1; s = 10; }
        const int sym = (run << 4) | s;
        put((unsigned)ac.code[sym], (int)ac.len[sym]);
        put(magnitude_bits(v, s), s);
        run = 0;
    }
    if (run > 0) put((unsigned)ac.code[0], (int)ac.len[0]);
    else ev.no_eob = 1;
    return ev;
}

// ---------------------------------------------------------------------------------------------- optimised tables
// Pillow's optimize=True (libjpeg's optimize_coding): every frame is coded with four tables built from its own symbol counts.
// The procedure is jchuff.c's: encode_mcu_gather / htest_one_block for the counts, jpeg_gen_optimal_table for the tables.

// The gathering form of encode_block's walk: count(ac, symbol) for every code the walk above would put (ac: 0 the DC table of
// the component, 1 its AC table); magnitude bits have no symbol.  Out-of-range values are clamped as above.
template <class Count>
TSTAR_JHD BlockEvents gather_block(const int16_t* coef, int pred, const uint8_t* zigzag, Count&& count) {
    BlockEvents ev = {0, 0, 0};
    int n = category((int)coef[0] - pred);
    if (n > 11) { ev.bad = 1; n = 11; }
    count(0, n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = coef[zigzag[k]];
        if (v == 0) { ++run; continue; }
        while (run > 15) {
            count(1, 0xF0);
            run -= 16;
            ++ev.zrl;
        }
        int s = category(v);
        if (s > 10) { ev.bad = 1; s = 10; }
        count(1, (run << 4) | s);
        run = 0;
    }
    if (run > 0) count(1, 0);
    else ev.no_eob = 1;
    return ev;
}

// A table as the DHT segment carries it, for any alphabet of up to 256 symbols (the standard tables' HuffSpec stops at 162).
// 276 bytes, no padding: the layout the C ABI hands out.
struct HuffSpecWide {
    uint8_t bits[16];            // codes of length 1..16
    uint8_t vals[256];           // the first nvals are the symbols, by code length and then by value
    uint16_t nvals;
    uint16_t status;             // HUFF_*
};
enum { HUFF_OK = 0, HUFF_CLEN_OVERFLOW = 1, HUFF_EMPTY = 2 };        // libjpeg's JERR_HUFF_CLEN_OVERFLOW; a histogram without a symbol
constexpr int kHuffSymbols = 257;                    // 256 symbols and the reserved one, which keeps the all-ones code unused
constexpr int kHuffMaxClen = 32;                     // libjpeg's MAX_CLEN
constexpr uint32_t kHuffMaxCount = 1000000000u;      // libjpeg's search starts from this value: larger counts are never found

// With a 16-bit DC code a block takes at most (16 + 11) + 63 * (16 + 10) bits.
constexpr int kMaxBlockBitsOpt = 27 + 63 * 26;

// Code sizes as jpeg_gen_optimal_table finds them: repeat { c1 = the smallest non-zero count, ties to the LARGEST index; c2 the
// same among the others; count[c1] += count[c2], count[c2] = 0 } until one tree is left; a symbol's size is its depth in the
// tree of merges.  libjpeg bumps the sizes of both chains at every merge; here every merge makes a node with two parent links
// and the depth is read by walking them, which is what the table kernel does with one leaf per lane.
// freq [256] (their sum at most kHuffMaxCount); size [257] out (0: absent; [256] the reserved symbol's) -> the largest size.
TSTAR_JHD int huff_code_sizes(const uint32_t* freq, uint8_t* size) {
    uint32_t f[kHuffSymbols];
    uint16_t node[kHuffSymbols], parent[2 * kHuffSymbols];
    for (int i = 0; i < kHuffSymbols; ++i) { f[i] = i < 256 ? freq[i] : 1u; node[i] = (uint16_t)i; }
    for (int i = 0; i < 2 * kHuffSymbols; ++i) parent[i] = 0xFFFF;
    for (int next = kHuffSymbols;; ++next) {
        int c1 = -1, c2 = -1;
        for (int i = 0; i < kHuffSymbols; ++i)
            if (f[i] && (c1 < 0 || f[i] <= f[c1])) c1 = i;
        for (int i = 0; i < kHuffSymbols; ++i)
            if (f[i] && i != c1 && (c2 < 0 || f[i] <= f[c2])) c2 = i;
        if (c2 < 0) break;
        f[c1] += f[c2];
        f[c2] = 0;
        parent[node[c1]] = parent[node[c2]] = (uint16_t)next;
        node[c1] = (uint16_t)next;
    }
    int deepest = 0;
    for (int i = 0; i < kHuffSymbols; ++i) {
        int d = 0;
        if (i == 256 || freq[i])
            for (int p = i; parent[p] != 0xFFFF; p = parent[p]) ++d;
        size[i] = (uint8_t)d;                         // at most 256
        if (d > deepest) deepest = d;
    }
    return deepest;
}

// bits [33] (index = code length, [0] unused) counted from sizes of at most 32 -> limited to 16 as libjpeg does it: a pair of
// the longest codes gives one code a bit shorter, and the longest shorter code becomes the prefix of two; then the reserved
// symbol's code, one of the longest, is taken out.
TSTAR_JHD void huff_limit_bits(int* bits, int* steps) {
    int n = 0;
    for (int i = kHuffMaxClen; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) --j;
            bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
            ++n;
        }
    int i = 16;
    while (i > 0 && bits[i] == 0) --i;
    bits[i] -= 1;
    if (steps) *steps = n;
}

// rank of symbol j (size[j] > 0) in the order of huffval: symbols by unlimited code size, then by value
TSTAR_JHD int huff_rank(const uint8_t* size, int j) {
    int r = 0;
    for (int i = 0; i < 256; ++i) r += size[i] && (size[i] < size[j] || (size[i] == size[j] && i < j));
    return r;
}

// canonical codes of a wide spec (make_codes' rule); every symbol without a code gets length 0
TSTAR_JHD void huff_assign_codes(const HuffSpecWide& s, HuffCodes& h) {
    for (int i = 0; i < 256; ++i) { h.code[i] = 0; h.len[i] = 0; }
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1]; ++i, ++k) {
            h.code[s.vals[k]] = (uint16_t)code++;
            h.len[s.vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

// The whole procedure, pure: freq [256] -> spec (bits, huffval, status) and codes.  A status other than HUFF_OK leaves an empty
// spec and no code.  steps (optional): how often the limiting loop ran.
TSTAR_JHD int huff_optimal(const uint32_t* freq, HuffSpecWide& spec, HuffCodes& codes, int* steps) {
    for (int i = 0; i < 16; ++i) spec.bits[i] = 0;
    for (int i = 0; i < 256; ++i) spec.vals[i] = 0;
    spec.nvals = 0;
    spec.status = HUFF_OK;
    if (steps) *steps = 0;
    uint8_t size[kHuffSymbols];
    int present = 0;
    for (int i = 0; i < 256; ++i) present += freq[i] != 0;
    if (!present) spec.status = HUFF_EMPTY;
    else if (huff_code_sizes(freq, size) > kHuffMaxClen) spec.status = HUFF_CLEN_OVERFLOW;
    if (spec.status == HUFF_OK) {
        int bits[kHuffMaxClen + 1];
        for (int i = 0; i <= kHuffMaxClen; ++i) bits[i] = 0;
        for (int i = 0; i < kHuffSymbols; ++i)
            if (size[i]) ++bits[size[i]];
        huff_limit_bits(bits, steps);
        for (int i = 0; i < 16; ++i) spec.bits[i] = (uint8_t)bits[i + 1];
        for (int j = 0; j < 256; ++j)
            if (size[j]) spec.vals[huff_rank(size, j)] = (uint8_t)j;
        spec.nvals = (uint16_t)present;
    }
    huff_assign_codes(spec, codes);
    return spec.status;
}

// ---------------------------------------------------------------------------------------------- scan order
// The k-th block of a frame's interleaved scan (MCU after MCU; inside it the Y blocks row-major, then Cb, Cr): its component,
// its index in the coefficient layout, and the index of the block whose DC it is predicted from (-1: none, predictor 0).
//
// A scan with a restart interval of R MCUs (R >= 1; 0: none) is cut behind every R-th MCU but the last: the entropy coder fills
// the current byte with one-bits, RSTn follows (FF D0 + n mod 8, n counting the markers of the scan from 0) and every component's
// DC predictor starts from 0 again: the first block of a component in an interval has no predecessor.  The scan then holds
// (MCUs - 1) / R markers and one interval more.
struct ScanGeom {
    int hs, vs, mcux, mcuy, bw0;           // bw0: luma blocks per row of the padded layout
    int off1, off2;                        // first Cb / Cr block of the layout
    TSTAR_JHD int per_mcu() const { return hs * vs + 2; }
    TSTAR_JHD int blocks() const { return mcux * mcuy * per_mcu(); }
};
TSTAR_JHD int luma_block(const ScanGeom& g, int m, int j) {
    const int mx = m % g.mcux, my = m / g.mcux;
    return (my * g.vs + j / g.hs) * g.bw0 + mx * g.hs + j % g.hs;
}
TSTAR_JHD void scan_block(const ScanGeom& g, int k, int interval, int* comp, int* block, int* pred_block) {
    const int ny = g.hs * g.vs, m = k / (ny + 2), j = k % (ny + 2);
    if (j < ny) {
        *comp = 0;
        *block = luma_block(g, m, j);
        *pred_block = j > 0 ? luma_block(g, m, j - 1) : (m > 0 ? luma_block(g, m - 1, ny - 1) : -1);
    } else {
        *comp = 1 + j - ny;
        const int off = *comp == 1 ? g.off1 : g.off2;
        *block = off + m;
        *pred_block = m > 0 ? off + m - 1 : -1;
    }
    if (interval > 0 && m % interval == 0 && (j == 0 || j >= ny)) *pred_block = -1;
}
// Bits an interval's end adds to the scan at most: 7 pad bits and the 16 of the marker
constexpr int kRestartBits = 7 + 16;

// Dummy luma blocks (beyond the real ceil(W / 8) x ceil(H / 8) blocks, inside the last MCU column / row): AC zero, DC that of
// a REAL block in the same MCU.  A right-edge dummy takes the block to its left.  Every block of a bottom-edge dummy row takes
// the block that precedes the row in the MCU's order, the last block of the row above, which may be a right-edge dummy itself
// and then stands for the block left of it.  Returns the real block's index, or -1 when (by, bx) is a real block.
TSTAR_JHD int dummy_source(int by, int bx, int real_bw, int real_bh, int hs, int bw0, int* kind) {
    if (by >= real_bh) {
        int sx = bx / hs * hs + hs - 1;
        if (sx >= real_bw) --sx;
        *kind = 1;
        return (by - 1) * bw0 + sx;
    }
    if (bx >= real_bw) {
        *kind = 0;
        return by * bw0 + bx - 1;
    }
    return -1;
}

}  // namespace jpegenc
}  // namespace tstar
