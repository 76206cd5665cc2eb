// Baseline JPEG: host entropy stage (marker walk + sequential Huffman decode) and the scalar reference of the
// reconstruction.  HIP-free.  This file parses untrusted bytes: every read goes through a bounds-checked cursor, every
// table index and run length is checked before use, and a broken stream is an error, never a partial picture.
#include "jpeg_host.h"
#include "jpeg_entropy_core.h"
#include "jpeg_math.h"

#include <math.h>
#include <sched.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

namespace tstar {

void set_error(const std::string& msg);          // capi.hip (or the stand-alone checker): thread-local last error

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU T.81 Annex K.3 typical Huffman tables (frames of AVI MJPG streams commonly carry no DHT)
const uint8_t kStdDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kStdDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kStdAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kStdAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kStdAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kStdAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct Huff {
    bool present = false;
    uint16_t fast[512];            // 9-bit prefix -> (length << 8) | symbol, 0 when the code is longer than 9 bits
    int32_t maxcode[18];           // largest code of each length (-1: none); [17] is a sentinel
    int32_t valptr[17], mincode[17];
    uint8_t vals[256];
    int nvals = 0;

    // bits[1..16] = number of codes of each length.  False when the counts do not describe a prefix code.
    bool build(const uint8_t* bits16, const uint8_t* v, int n) {
        int total = 0;
        for (int l = 0; l < 16; ++l) total += bits16[l];
        if (total != n || n > 256) return false;
        memcpy(vals, v, (size_t)n);
        nvals = n;
        memset(fast, 0, sizeof(fast));
        int32_t code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            const int cnt = bits16[l - 1];
            valptr[l] = k;
            mincode[l] = code;
            if (code + cnt > (1 << l)) return false;               // more codes than this length has room for
            for (int i = 0; i < cnt; ++i, ++k, ++code) {
                if (l <= 9) {
                    const int first = code << (9 - l), span = 1 << (9 - l);
                    for (int j = 0; j < span; ++j) fast[first + j] = (uint16_t)((l << 8) | vals[k]);
                }
            }
            maxcode[l] = cnt ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        present = true;
        return true;
    }
};

struct Component {
    int id = 0, h = 0, v = 0, tq = 0, td = 0, ta = 0;
};

struct Header {
    bool have_sof = false, progressive = false, arithmetic = false, lossless_or_other = false;
    int precision = 0, W = 0, H = 0, ncomp = 0;
    Component comp[4];
    uint16_t quant[4][64];          // natural order
    bool have_quant[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart_interval = 0;
    size_t scan_data = 0;           // offset of the entropy-coded segment of the first scan
    bool scan_all_components = false;
    bool jfif = false, adobe = false;   // APP0 "JFIF" / APP14 "Adobe" seen: libjpeg picks the colour space from them
    int adobe_transform = 0;
};

struct Err {
    char* buf;
    size_t len;
    int fail(int code, const char* msg) const {
        if (buf && len) snprintf(buf, len, "%s", msg);
        return code;
    }
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Walk the marker segments up to and including the first SOS header.
int parse_header(const uint8_t* d, size_t len, Header& h, const Err& e) {
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return e.fail(JPEG_MALFORMED, "no SOI marker");
    size_t p = 2;
    for (;;) {
        if (p + 2 > len) return e.fail(JPEG_MALFORMED, "truncated before the scan");
        if (d[p] != 0xFF) return e.fail(JPEG_MALFORMED, "marker expected");
        while (p < len && d[p] == 0xFF) ++p;                       // fill bytes
        if (p >= len) return e.fail(JPEG_MALFORMED, "truncated inside a marker");
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;       // no payload
        if (m == 0xD9) return e.fail(JPEG_MALFORMED, "EOI before any scan");
        if (m == 0x00) return e.fail(JPEG_MALFORMED, "stuffed byte outside entropy data");
        if (p + 2 > len) return e.fail(JPEG_MALFORMED, "truncated segment length");
        const int L = be16(d + p);
        if (L < 2 || p + (size_t)L > len) return e.fail(JPEG_MALFORMED, "segment length runs past the end of the data");
        const uint8_t* s = d + p + 2;
        const int n = L - 2;
        p += (size_t)L;
        if (m == 0xDB) {                                            // DQT
            int q = 0;
            while (q < n) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (pq > 1 || tq > 3) return e.fail(JPEG_MALFORMED, "DQT: bad precision or table index");
                const int need = 1 + 64 * (pq + 1);
                if (q + need > n) return e.fail(JPEG_MALFORMED, "DQT: bad length");
                for (int k = 0; k < 64; ++k)
                    h.quant[tq][kZigzag[k]] = pq ? (uint16_t)be16(s + q + 1 + 2 * k) : s[q + 1 + k];
                h.have_quant[tq] = true;
                q += need;
            }
        } else if (m == 0xC4) {                                     // DHT
            int q = 0;
            while (q < n) {
                if (q + 17 > n) return e.fail(JPEG_MALFORMED, "DHT: bad length");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return e.fail(JPEG_MALFORMED, "DHT: bad class or table index");
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += s[q + 1 + l];
                if (cnt > 256 || q + 17 + cnt > n) return e.fail(JPEG_MALFORMED, "DHT: bad length");
                Huff& t = tc ? h.ac[th] : h.dc[th];
                if (!t.build(s + q + 1, s + q + 17, cnt)) return e.fail(JPEG_MALFORMED, "DHT: code lengths do not form a prefix code");
                q += 17 + cnt;
            }
        } else if (m == 0xDD) {                                     // DRI
            if (n != 2) return e.fail(JPEG_MALFORMED, "DRI: bad length");
            h.restart_interval = be16(s);
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {          // SOFn (0xC4 handled above)
            if (h.have_sof) return e.fail(JPEG_MALFORMED, "second frame header");
            if (n < 6) return e.fail(JPEG_MALFORMED, "SOF: bad length");
            h.precision = s[0];
            h.H = be16(s + 1);
            h.W = be16(s + 3);
            h.ncomp = s[5];
            if (h.ncomp < 1 || h.ncomp > 4 || n != 6 + 3 * h.ncomp) return e.fail(JPEG_MALFORMED, "SOF: bad length or component count");
            if (h.W == 0 || h.H == 0) return e.fail(JPEG_MALFORMED, "SOF: zero width or height");
            for (int c = 0; c < h.ncomp; ++c) {
                Component& k = h.comp[c];
                k.id = s[6 + 3 * c];
                k.h = s[7 + 3 * c] >> 4;
                k.v = s[7 + 3 * c] & 15;
                k.tq = s[8 + 3 * c];
                if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return e.fail(JPEG_MALFORMED, "SOF: bad sampling factor or table index");
            }
            h.have_sof = true;
            if (m == 0xC2) h.progressive = true;
            else if (m >= 0xC9) h.arithmetic = true;
            else if (m != 0xC0 && m != 0xC1) h.lossless_or_other = true;
            if (h.precision != 8) {
                // 12-bit samples: no decoder on either side of the bit-equality reads them; report as broken input
                return e.fail(JPEG_MALFORMED, "SOF: only 8-bit samples are supported");
            }
        } else if (m == 0xDA) {                                     // SOS
            if (!h.have_sof) return e.fail(JPEG_MALFORMED, "scan before the frame header");
            if (n < 1) return e.fail(JPEG_MALFORMED, "SOS: bad length");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return e.fail(JPEG_MALFORMED, "SOS: bad length or component count");
            h.scan_all_components = (ns == h.ncomp);
            for (int i = 0; i < ns; ++i) {
                const int id = s[1 + 2 * i], td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (td > 3 || ta > 3) return e.fail(JPEG_MALFORMED, "SOS: bad table index");
                if (h.scan_all_components) {
                    if (h.comp[i].id != id) return e.fail(JPEG_MALFORMED, "SOS: component order differs from the frame header");
                    h.comp[i].td = td;
                    h.comp[i].ta = ta;
                }
            }
            h.scan_data = p;
            return JPEG_OK;
        }
        else if (m == 0xE0 && n >= 14 && memcmp(s, "JFIF\0", 5) == 0) {
            h.jfif = true;
        } else if (m == 0xEE && n >= 12 && memcmp(s, "Adobe", 5) == 0) {
            h.adobe = true;
            h.adobe_transform = s[11];
        }
        // other APPn, COM and anything else with a length: skipped
    }
}

// What of a parsed header this decoder covers; the rest is left to a general decoder.
int classify(const Header& h, JpegGeom* g, const Err& e) {
    g->W = h.W; g->H = h.H; g->ncomp = h.ncomp; g->hs = 0; g->vs = 0;
    if (h.progressive) return e.fail(JPEG_UNCOVERED, "progressive JPEG");
    if (h.arithmetic) return e.fail(JPEG_UNCOVERED, "arithmetic-coded JPEG");
    if (h.lossless_or_other) return e.fail(JPEG_UNCOVERED, "not a baseline / extended sequential JPEG");
    if (h.ncomp != 1 && h.ncomp != 3) return e.fail(JPEG_UNCOVERED, "neither grayscale nor three components");
    if (!h.scan_all_components) return e.fail(JPEG_UNCOVERED, "more than one scan");
    if (h.ncomp == 3) {
        if (h.comp[1].h != 1 || h.comp[1].v != 1 || h.comp[2].h != 1 || h.comp[2].v != 1) return e.fail(JPEG_UNCOVERED, "chroma sampling other than 1x1");
        // three components are YCbCr only where libjpeg would say so (jdapimin.c, default_decompress_parms): a JFIF marker
        // settles it; else an Adobe marker with transform 0 means RGB whatever the ids; else the ids 'R','G','B' mean RGB
        const bool rgb = !h.jfif && (h.adobe ? h.adobe_transform == 0
                                             : (h.comp[0].id == 'R' && h.comp[1].id == 'G' && h.comp[2].id == 'B'));
        if (rgb) return e.fail(JPEG_UNCOVERED, "RGB-coded JPEG");
        g->hs = h.comp[0].h;
        g->vs = h.comp[0].v;
    } else {
        g->hs = g->vs = 1;                                          // a single component is never interleaved: its factors do not matter
    }
    if (!g->valid())
        return e.fail(JPEG_UNCOVERED, "luma sampling other than 1x1, 2x1 or 2x2, subsampled chroma at most 2 samples wide, or a picture above 16384 pixels a side");
    return JPEG_OK;
}

// MSB-first bit reader over the entropy-coded segment: removes FF00 stuffing, stops at a marker.  Bits past the marker
// (or the end of the data) read as zero so that table look-ahead is safe; CONSUMING one of them is the error.
struct BitReader {
    const uint8_t* d;
    size_t p, len;
    uint64_t acc = 0;
    int nbits = 0, fake = 0;       // the lowest `fake` bits of acc are padding
    bool at_marker = false;

    void fill() {
        while (nbits <= 56) {
            unsigned b = 0;
            if (!at_marker) {
                if (p >= len) {
                    at_marker = true;
                } else if (d[p] != 0xFF) {
                    b = d[p++];
                } else if (p + 1 < len && d[p + 1] == 0x00) {
                    b = 0xFF;
                    p += 2;
                } else {
                    at_marker = true;                               // p stays on the FF
                }
            }
            if (at_marker) fake += 8;
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1)); }
    bool skip(int n) {
        nbits -= n;
        return nbits >= fake;
    }
    void reset() { acc = 0; nbits = 0; fake = 0; at_marker = false; }
};

inline int huff_decode(BitReader& br, const Huff& t) {
    br.fill();
    const unsigned f = t.fast[br.peek(9)];
    if (f) {
        if (!br.skip((int)(f >> 8))) return -1;
        return (int)(f & 255);
    }
    int32_t code = (int32_t)br.peek(10);
    int l = 10;
    while (l <= 16 && code > t.maxcode[l]) {
        ++l;
        if (l <= 16) code = (int32_t)br.peek(l);
    }
    if (l > 16) return -1;                                          // no code of any length matches
    const int idx = t.valptr[l] + (code - t.mincode[l]);
    if (idx < 0 || idx >= t.nvals) return -1;
    if (!br.skip(l)) return -1;
    return t.vals[idx];
}

// s-bit magnitude field -> signed value (T.81 F.2.2.1 EXTEND)
inline bool receive_extend(BitReader& br, int s, int* out) {
    br.fill();
    const int v = (int)br.peek(s);
    if (!br.skip(s)) return false;
    *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

// The DCT of JPEG is orthonormal, so the coefficients of a block of 8-bit samples (level-shifted to [-128, 127]) have a
// Euclidean norm of at most 8 * 128 = 1024; quantisation moves each by at most half its step.  A block beyond
// 1024 + |q| / 2 (+ 16 for the encoder's own rounding) cannot come from a picture.  Decoders disagree on such data
// (libjpeg-turbo's SIMD inverse DCT keeps 16-bit intermediates that wrap or saturate, the C one does not), so it is an error
// here rather than one more picture nobody agrees on.  Inside the bound no 16-bit intermediate overflows.
const char kEnergyMsg[] = "block carries more energy than 8-bit samples can";

int64_t energy_limit(const uint16_t* q) {
    double n2 = 0;
    for (int k = 0; k < 64; ++k) n2 += (double)q[k] * q[k];
    const double b = 1024.0 + 16.0 + 0.5 * sqrt(n2) + 1.0;
    return (int64_t)(b * b);
}

const char* decode_block(BitReader& br, const Huff& dc, const Huff& ac, const uint16_t* q, int64_t limit, int* pred, int16_t* blk) {
    const int t = huff_decode(br, dc);
    if (t < 0) return "bad Huffman code or data ends inside a DC code";
    if (t > 11) return "DC magnitude category above 11";
    int diff = 0;
    if (t && !receive_extend(br, t, &diff)) return "data ends inside a DC value";
    *pred += diff;
    if (*pred < -2048 || *pred > 2047) return "DC coefficient out of the 8-bit range";
    blk[0] = (int16_t)*pred;
    int64_t energy = (int64_t)(*pred * (int)q[0]) * (*pred * (int)q[0]);
    int k = 1;
    while (k < 64) {
        const int rs = huff_decode(br, ac);
        if (rs < 0) return "bad Huffman code or data ends inside an AC code";
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r == 15) {
                k += 16;
                if (k > 64) return "zero run past the end of the block";
                continue;
            }
            if (r != 0) return "end-of-band run in a sequential scan";
            break;
        }
        if (s > 10) return "AC magnitude category above 10";
        k += r;
        if (k > 63) return "coefficient index past the end of the block";
        int v;
        if (!receive_extend(br, s, &v)) return "data ends inside an AC value";
        const int nat = kZigzag[k];
        blk[nat] = (int16_t)v;
        energy += (int64_t)(v * (int)q[nat]) * (v * (int)q[nat]);
        ++k;
    }
    if (energy > limit) return kEnergyMsg;
    return nullptr;
}

void std_tables(Header& h) {
    // a frame with no DHT at all gets the Annex K tables; a frame that defines some tables is taken at its word
    bool any = false;
    for (int i = 0; i < 4; ++i) any = any || h.dc[i].present || h.ac[i].present;
    if (any) return;
    h.dc[0].build(kStdDcLumBits, kStdDcVals, 12);
    h.dc[1].build(kStdDcChrBits, kStdDcVals, 12);
    h.ac[0].build(kStdAcLumBits, kStdAcLumVals, 162);
    h.ac[1].build(kStdAcChrBits, kStdAcChrVals, 162);
}

}  // namespace

int jpeg_probe(const uint8_t* data, size_t len, JpegGeom* g, char* err, size_t errlen) {
    const Err e{err, errlen};
    *g = JpegGeom{0, 0, 0, 0, 0};
    if (!data) return e.fail(JPEG_MALFORMED, "null data");
    std::vector<Header> hv(1);
    const int rc = parse_header(data, len, hv[0], e);
    if (rc != JPEG_OK) return rc;
    return classify(hv[0], g, e);
}

int jpeg_entropy(const uint8_t* data, size_t len, const JpegGeom& g, int16_t* coef, uint16_t* quant, char* err, size_t errlen) {
    const Err e{err, errlen};
    if (!data || !coef || !quant || !g.valid()) return e.fail(JPEG_MALFORMED, "null argument or unsupported geometry");
    std::vector<Header> hv(1);                                     // ~10 KB of tables: off the worker's stack
    Header& h = hv[0];
    int rc = parse_header(data, len, h, e);
    if (rc != JPEG_OK) return rc;
    JpegGeom got;
    rc = classify(h, &got, e);
    if (rc != JPEG_OK) return rc;
    if (got.W != g.W || got.H != g.H || got.ncomp != g.ncomp || got.hs != g.hs || got.vs != g.vs)
        return e.fail(JPEG_GEOMETRY, "size, component count or sampling differs from the batch's");
    std_tables(h);
    for (int c = 0; c < g.ncomp; ++c) {
        const Component& k = h.comp[c];
        if (!h.have_quant[k.tq]) return e.fail(JPEG_MALFORMED, "component names a quantisation table that was never defined");
        if (!h.dc[k.td].present || !h.ac[k.ta].present) return e.fail(JPEG_MALFORMED, "scan names a Huffman table that was never defined");
    }
    memset(quant, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < g.ncomp; ++c) memcpy(quant + 64 * c, h.quant[h.comp[c].tq], 64 * sizeof(uint16_t));
    memset(coef, 0, g.blocks() * 64 * sizeof(int16_t));

    const int mcux = g.mcux(), mcuy = g.mcuy();
    int16_t* base[3];
    int bw[3], nh[3], nv[3];
    int64_t limit[3];
    for (int c = 0; c < g.ncomp; ++c) {
        limit[c] = energy_limit(quant + 64 * c);
        base[c] = coef + g.block_offset(c) * 64;
        bw[c] = g.bw(c);
        nh[c] = c == 0 ? g.hs : 1;
        nv[c] = c == 0 ? g.vs : 1;
    }
    BitReader br{data, h.scan_data, len};
    int pred[3] = {0, 0, 0};
    const int ri = h.restart_interval;
    int until_restart = ri, next_rst = 0;
    const size_t n_mcu = (size_t)mcux * mcuy;
    for (size_t m = 0; m < n_mcu; ++m) {
        if (ri && until_restart == 0) {
            // byte-align: what is left of the current byte is padding; then exactly RSTn must follow
            br.fill();
            if (!br.at_marker || br.nbits - br.fake >= 8) return e.fail(JPEG_MALFORMED, "entropy data where a restart marker should be");
            size_t p = br.p;
            while (p + 1 < len && data[p] == 0xFF && data[p + 1] == 0xFF) ++p;
            if (p + 1 >= len || data[p] != 0xFF || data[p + 1] != 0xD0 + next_rst) return e.fail(JPEG_MALFORMED, "missing or out-of-order restart marker");
            br.p = p + 2;
            br.reset();
            next_rst = (next_rst + 1) & 7;
            until_restart = ri;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = (int)(m / mcux), mx = (int)(m % mcux);
        for (int c = 0; c < g.ncomp; ++c) {
            const Huff& dc = h.dc[h.comp[c].td];
            const Huff& ac = h.ac[h.comp[c].ta];
            for (int v = 0; v < nv[c]; ++v)
                for (int u = 0; u < nh[c]; ++u) {
                    const size_t b = (size_t)(my * nv[c] + v) * bw[c] + (size_t)(mx * nh[c] + u);
                    const char* msg = decode_block(br, dc, ac, quant + 64 * c, limit[c], &pred[c], base[c] + b * 64);
                    // beyond the energy bound the stream may still be one a lenient decoder reads: its call, not an error here
                    if (msg) return e.fail(msg == kEnergyMsg ? JPEG_UNCOVERED : JPEG_MALFORMED, msg);
                }
        }
        --until_restart;
    }
    // Every block is decoded.  A scan that ends cleanly here -- less than a byte of padding, then EOI -- is ours; one with
    // bytes left over or without its EOI (some cameras write such frames) is left to the general decoder, which may read it.
    br.fill();
    if (!br.at_marker || br.nbits - br.fake >= 8) return e.fail(JPEG_UNCOVERED, "entropy data left after the last block");
    size_t p = br.p;
    while (p + 1 < len && data[p] == 0xFF && data[p + 1] == 0xFF) ++p;
    if (p + 1 >= len || data[p] != 0xFF || data[p + 1] != 0xD9) return e.fail(JPEG_UNCOVERED, "no EOI after the last block");
    return JPEG_OK;
}

size_t jpeg_frame_end(const uint8_t* d, size_t len, size_t pos) {
    if (!d || pos + 4 > len || d[pos] != 0xFF || d[pos + 1] != 0xD8) return 0;
    size_t p = pos + 2;
    for (;;) {
        if (p + 2 > len || d[p] != 0xFF) return 0;
        while (p < len && d[p] == 0xFF) ++p;
        if (p >= len) return 0;
        const int m = d[p++];
        if (m == 0xD9) return p;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0x00 || p + 2 > len) return 0;
        const int L = be16(d + p);
        if (L < 2 || p + (size_t)L > len) return 0;
        p += (size_t)L;
        if (m != 0xDA) continue;
        // entropy-coded data: runs to the next FF that is followed by neither 00 (stuffing) nor RSTn
        for (;;) {
            const void* f = memchr(d + p, 0xFF, len - p);
            if (!f) return 0;
            p = (size_t)((const uint8_t*)f - d);
            if (p + 1 >= len) return 0;
            const int x = d[p + 1];
            if (x == 0x00 || (x >= 0xD0 && x <= 0xD7)) { p += 2; continue; }
            if (x == 0xFF) { p += 1; continue; }
            break;                                                  // a marker: back to the segment walk
        }
    }
}

namespace {

void flatten(const Huff& t, JpegHuffFlat* f) {
    memcpy(f->fast, t.fast, sizeof(f->fast));
    f->maxcode[0] = -1;
    f->delta[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        f->maxcode[l] = t.maxcode[l];
        f->delta[l] = t.valptr[l] - t.mincode[l];
    }
    f->maxcode[17] = t.maxcode[17];
    f->nvals = t.nvals;
    memcpy(f->vals, t.vals, (size_t)t.nvals);
}

// One frame: false = route it to jpeg_entropy.  On true, *ts is the frame's table set, quant its rows and segs its
// segments with frame-local byte offsets.
bool plan_frame(const uint8_t* d, size_t len, const JpegGeom& g, Header& h, JpegTableSet* ts, uint16_t* quant,
                std::vector<JpegSegment>& segs) {
    const Err e{nullptr, 0};
    if (!d || parse_header(d, len, h, e) != JPEG_OK) return false;
    JpegGeom got;
    if (classify(h, &got, e) != JPEG_OK) return false;
    if (got.W != g.W || got.H != g.H || got.ncomp != g.ncomp || got.hs != g.hs || got.vs != g.vs) return false;
    std_tables(h);
    for (int c = 0; c < g.ncomp; ++c) {
        const Component& k = h.comp[c];
        if (!h.have_quant[k.tq] || !h.dc[k.td].present || !h.ac[k.ta].present) return false;
    }
    memset((void*)ts, 0, sizeof(*ts));                              // padding and unused tables too: sets are compared by content
    memset(quant, 0, 192 * sizeof(uint16_t));
    for (int c = 0; c < g.ncomp; ++c) {
        const Component& k = h.comp[c];
        memcpy(quant + 64 * c, h.quant[k.tq], 64 * sizeof(uint16_t));
        ts->limit[c] = energy_limit(quant + 64 * c);
        flatten(h.dc[k.td], &ts->h[2 * c]);
        flatten(h.ac[k.ta], &ts->h[2 * c + 1]);
    }
    memcpy(ts->quant, quant, sizeof(ts->quant));
    memcpy(ts->zigzag, kZigzag, 64);

    // the entropy data, once: a segment ends at the first FF that is not followed by 00 (where the bit reader stops)
    const size_t n_mcu = (size_t)g.mcux() * g.mcuy(), ri = (size_t)h.restart_interval;
    const size_t n_seg = ri ? (n_mcu + ri - 1) / ri : 1;
    size_t p = h.scan_data;
    for (size_t i = 0; i < n_seg; ++i) {
        const size_t begin = p;
        for (;;) {
            const void* f = p < len ? memchr(d + p, 0xFF, len - p) : nullptr;
            if (!f) return false;                                   // the data ends without a marker
            p = (size_t)((const uint8_t*)f - d);
            if (p + 1 >= len) return false;
            if (d[p + 1] != 0x00) break;
            p += 2;
        }
        const size_t end = p;
        while (p + 1 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;       // fill bytes in front of the marker
        if (p + 1 >= len) return false;
        const bool last = i + 1 == n_seg;
        if (d[p + 1] != (last ? 0xD9 : 0xD0 + (int)(i & 7))) return false;  // RSTn in order, EOI behind the last segment
        p += 2;
        JpegSegment s;
        s.frame = 0;
        s.begin = (uint32_t)begin;
        s.end = (uint32_t)end;
        s.first_mcu = (uint32_t)(ri ? i * ri : 0);
        s.n_mcu = (uint32_t)(ri && (i + 1) * ri < n_mcu ? ri : n_mcu - s.first_mcu);
        s.last = last ? 1u : 0u;
        segs.push_back(s);
    }
    return true;
}

}  // namespace

bool jpeg_plan_segments(const uint8_t* const* datas, const size_t* lens, const uint64_t* byte_offsets, int n, const JpegGeom& g,
                        int32_t* route, JpegFrameDesc* frames, uint16_t* quant, std::vector<JpegTableSet>* sets,
                        std::vector<JpegSegment>* segments) {
    std::vector<Header> hv(1);                                     // ~10 KB of tables: off the stack
    std::vector<JpegTableSet> one(1);
    std::vector<JpegSegment> segs;
    for (int i = 0; i < n; ++i) {
        if (byte_offsets[i] + (uint64_t)lens[i] >= 0xffffffffull) return false;
        hv[0] = Header();
        segs.clear();
        uint16_t* q = quant + 192 * (size_t)i;
        JpegFrameDesc& fd = frames[i];
        fd.table_set = -1; fd.first_segment = 0; fd.n_segments = 0; fd.reserved = 0;
        if (!plan_frame(datas[i], lens[i], g, hv[0], &one[0], q, segs)) {
            memset(q, 0, 192 * sizeof(uint16_t));
            route[i] = 1;
            continue;
        }
        route[i] = 0;
        size_t k = 0;
        while (k < sets->size() && memcmp((const void*)&(*sets)[k], (const void*)&one[0], sizeof(JpegTableSet)) != 0) ++k;
        if (k == sets->size()) sets->push_back(one[0]);
        fd.table_set = (int32_t)k;
        fd.first_segment = (int32_t)segments->size();
        fd.n_segments = (int32_t)segs.size();
        for (JpegSegment s : segs) {
            s.frame = (uint32_t)i;
            s.begin += (uint32_t)byte_offsets[i];
            s.end += (uint32_t)byte_offsets[i];
            segments->push_back(s);
        }
    }
    return true;
}

bool jpeg_entropy_segments_host(const uint8_t* bytes, size_t total_bytes, const JpegSegment* segments, const JpegTableSet* tables,
                                int n_sets, const JpegFrameDesc* frames, int n_frames, int n_segments, const JpegGeom& g,
                                int16_t* coef, int32_t* seg_status) {
    jpegcore::SegmentBatch b;
    if (jpegcore::segment_batch(bytes, total_bytes, segments, tables, n_sets, frames, n_frames, n_segments, g, coef, seg_status, &b) ||
        total_bytes == 0 || total_bytes >= 0xffffffffull)
        return false;
    memset(coef, 0, (size_t)n_frames * b.g.per_frame * sizeof(int16_t));
    for (int i = 0; i < n_segments; ++i) {
        const JpegSegment s = segments[i];
        const int ts = jpegcore::segment_table_set(b, s);
        seg_status[i] = ts < 0 ? (int)JPEG_MALFORMED
                               : jpegcore::decode_segment(bytes, s.begin, s.end, tables + ts, b.g, s.first_mcu, s.n_mcu, s.last != 0,
                                                          coef + (size_t)s.frame * b.g.per_frame);
    }
    return true;
}

size_t jpeg_split_workspace_bytes(size_t total_bytes, int n_segments, int sub_bytes) {
    if (total_bytes == 0 || total_bytes >= 0xffffffffull || n_segments <= 0 || sub_bytes < (int)jpegcore::kSubBytesMin || sub_bytes % 4 != 0)
        return 0;
    const uint64_t cap = jpegcore::split_cap(total_bytes, (uint64_t)n_segments, (uint32_t)sub_bytes);
    if (cap >= 0x7fffffffull - 1024) return 0;
    return (size_t)jpegcore::split_ws_bytes(cap, (uint64_t)n_segments);
}

bool jpeg_split_args_ok(size_t total_bytes, int n_segments, int sub_bytes, int min_split_bytes, int max_rounds, const void* workspace,
                        size_t workspace_bytes) {
    const size_t need = jpeg_split_workspace_bytes(total_bytes, n_segments, sub_bytes);
    return need != 0 && min_split_bytes >= 0 && max_rounds >= 1 && max_rounds <= kJpegSplitMaxRounds && workspace &&
           (uintptr_t)workspace % 8 == 0 && workspace_bytes >= need;
}

bool jpeg_entropy_split_host(const uint8_t* bytes, size_t total_bytes, const JpegSegment* segments, const JpegTableSet* tables,
                             int n_sets, const JpegFrameDesc* frames, int n_frames, int n_segments, const JpegGeom& g, int sub_bytes,
                             int min_split_bytes, int max_rounds, void* workspace, size_t workspace_bytes, int16_t* coef,
                             int32_t* seg_status, int32_t* seg_info) {
    using namespace jpegcore;
    SegmentBatch b;
    if (segment_batch(bytes, total_bytes, segments, tables, n_sets, frames, n_frames, n_segments, g, coef, seg_status, &b) || !seg_info ||
        !jpeg_split_args_ok(total_bytes, n_segments, sub_bytes, min_split_bytes, max_rounds, workspace, workspace_bytes))
        return false;
    const uint32_t sub = (uint32_t)sub_bytes, rounds = (uint32_t)max_rounds, nseg = (uint32_t)n_segments;
    const uint64_t cap = split_cap(total_bytes, nseg, sub);
    const SplitWs w = split_ws_carve(workspace, cap, nseg);
    memset(coef, 0, (size_t)n_frames * b.g.per_frame * sizeof(int16_t));
    // the layout: which segments are cut, and where their sub-sequences sit in the workspace
    uint64_t at = 0;
    *w.total = 0;
    for (uint32_t si = 0; si < nseg; ++si) {
        const uint32_t n = split_n_sub(b, segments[si], sub, (uint32_t)min_split_bytes);
        const bool fits = n != 0 && at + n <= cap;
        w.n_sub[si] = fits ? n : 0;
        w.sub_first[si] = (uint32_t)(at < 0xffffffffull ? at : 0xffffffffull);
        w.last_changed[si] = 0;
        at += n;
        if (fits) *w.total = (uint32_t)at;
    }
    // (a) the rounds, in the kernels' order: every sub-sequence of round r reads what round r - 1 recorded
    // Only sub-sequences a round can touch are visited: the successor of one whose exit changed in the round before (it walks
    // again), and one whose own exit changed in one of the two rounds before (its other copy and flag are brought up to
    // date).  For every other one the round is a copy of equal words, so the result is the kernels' word for word.
    {
        const uint32_t total = *w.total;
        std::vector<uint32_t> seg_of(total), stamp(total, 0xffffffffu), prev, prev2, cur, todo;
        for (uint32_t si = 0; si < nseg; ++si)
            for (uint32_t i = 0; i < w.n_sub[si]; ++i) seg_of[w.sub_first[si] + i] = si;
        for (uint32_t lane = 0; lane < total; ++lane) prev.push_back(lane);     // round 0 changes every exit
        for (uint32_t r = 0; r <= rounds && !(prev.empty() && prev2.empty()); ++r) {
            todo.clear();
            auto want = [&](uint32_t lane) {
                if (stamp[lane] != r) { stamp[lane] = r; todo.push_back(lane); }
            };
            if (r == 0) {
                todo = prev;
            } else {
                for (uint32_t lane : prev) {
                    want(lane);
                    const uint32_t si = seg_of[lane];
                    if (lane + 1 < w.sub_first[si] + w.n_sub[si]) want(lane + 1);
                }
                for (uint32_t lane : prev2) want(lane);
            }
            cur.clear();
            for (uint32_t lane : todo) {
                const uint32_t si = seg_of[lane];
                if (split_round_lane(b, w, sub, r, si, lane, tables + segment_table_set(b, segments[si]))) cur.push_back(lane);
            }
            if (r != 0) prev2.swap(prev);
            prev.swap(cur);
        }
    }
    // (b) first block and predictors of every sub-sequence of a converged segment
    for (uint32_t si = 0; si < nseg; ++si) {
        seg_info[si] = split_seg_info(w, si, rounds);
        if (seg_info[si] <= 0) continue;
        seg_status[si] = JPEG_OK;
        uint64_t blocks = 0;
        uint32_t d0 = 0, d1 = 0, d2 = 0;
        for (uint32_t lane = w.sub_first[si]; lane < w.sub_first[si] + w.n_sub[si]; ++lane) {
            w.first_block[lane] = (uint32_t)(blocks < 0xffffffffull ? blocks : 0xffffffffull);
            w.pred0[lane] = d0; w.pred1[lane] = d1; w.pred2[lane] = d2;
            blocks += w.blocks[lane]; d0 += w.dc0[lane]; d1 += w.dc1[lane]; d2 += w.dc2[lane];
        }
    }
    // (c) the write pass of the converged segments
    for (uint32_t si = 0; si < nseg; ++si) {
        if (seg_info[si] <= 0) continue;
        for (uint32_t i = 0; i < w.n_sub[si]; ++i)
            if (split_write_lane(b, w, sub, rounds, si, w.sub_first[si] + i, tables + segment_table_set(b, segments[si])) != JPEG_OK)
                seg_status[si] = JPEG_MALFORMED;
    }
    // (c) every other segment and (d) the refused ones again, by one lane: that status stands
    for (uint32_t si = 0; si < nseg; ++si) {
        const bool redo = seg_info[si] > 0;
        if (redo && seg_status[si] == JPEG_OK) continue;
        const JpegSegment s = segments[si];
        const int ts = segment_table_set(b, s);
        int st = ts < 0 ? (int)JPEG_MALFORMED
                        : decode_segment(bytes, s.begin, s.end, tables + ts, b.g, s.first_mcu, s.n_mcu, s.last != 0,
                                         coef + (size_t)s.frame * b.g.per_frame);
        if (redo && st == JPEG_OK) st = JPEG_UNCOVERED;                         // the write pass refused what one lane accepts: never
        seg_status[si] = st;
    }
    return true;
}

namespace {

// dequantise + inverse DCT of output size k x k (8, 4, 2, 1) + range limit of one block -> k rows of k pixels at dst
void idct_block(const int16_t* b, const uint16_t* q, int k, uint8_t* dst, int pitch) {
    using namespace jpegmath;
    if (k == 1) {
        dst[0] = range_limit(idct1((uint32_t)((int32_t)b[0] * (int32_t)q[0])));
        return;
    }
    const int shift1 = k == 8 ? 11 : (k == 4 ? 12 : 13), shift2 = shift1 + 7;
    const auto pass = [k](const uint32_t* x, int32_t* o, int shift) {
        if (k == 8) idct8(x, o, shift);
        else if (k == 4) idct4(x, o, shift);
        else idct2(x, o, shift);
    };
    int32_t ws[64];
    for (int col = 0; col < 8; ++col) {
        if (!idct_reads(k, col)) continue;
        uint32_t x[8];
        int32_t o[8];
        for (int i = 0; i < 8; ++i) x[i] = (uint32_t)((int32_t)b[8 * i + col] * (int32_t)q[8 * i + col]);
        pass(x, o, shift1);
        for (int i = 0; i < k; ++i) ws[8 * i + col] = o[i];
    }
    for (int row = 0; row < k; ++row) {
        uint32_t x[8];
        int32_t o[8];
        for (int i = 0; i < 8; ++i) x[i] = idct_reads(k, i) ? (uint32_t)ws[8 * row + i] : 0u;
        pass(x, o, shift2);
        for (int i = 0; i < k; ++i) dst[(size_t)row * pitch + i] = range_limit(o[i]);
    }
}

// every block of a component -> its plane (whole blocks of k x k pixels, rows of `pitch` bytes)
void idct_plane(const int16_t* blocks, const uint16_t* q, int bw, int bh, int k, uint8_t* out, int pitch) {
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx)
            idct_block(blocks + ((size_t)by * bw + bx) * 64, q, k, out + (size_t)by * k * pitch + bx * k, pitch);
}

}  // namespace

void jpeg_reconstruct_host(const JpegGeom& g, const int16_t* coef, const uint16_t* quant, uint8_t* scratch, uint8_t* rgb) {
    using namespace jpegmath;
    const uint8_t* plane[3] = {nullptr, nullptr, nullptr};
    int pitch[3] = {0, 0, 0};
    for (int c = 0; c < g.ncomp; ++c) {
        uint8_t* out = scratch + g.block_offset(c) * 64;
        plane[c] = out;
        pitch[c] = g.bw(c) * 8;
        idct_plane(coef + g.block_offset(c) * 64, quant + 64 * c, g.bw(c), g.bh(c), 8, out, pitch[c]);
    }
    for (int y = 0; y < g.H; ++y) {
        uint8_t* dst = rgb + (size_t)y * g.W * 3;
        const uint8_t* yr = plane[0] + (size_t)y * pitch[0];
        if (g.ncomp == 1) {
            for (int x = 0; x < g.W; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = yr[x];
            continue;
        }
        for (int x = 0; x < g.W; ++x) {
            const int cb = upsample_at(plane[1], pitch[1], g.cw(1), g.ch(1), g.hs, g.vs, x, y);
            const int cr = upsample_at(plane[2], pitch[2], g.cw(2), g.ch(2), g.hs, g.vs, x, y);
            ycc_to_rgb(yr[x], cb, cr, dst + 3 * x);
        }
    }
}

void jpeg_reconstruct_scaled_host(const JpegScaledGeom& sg, const int16_t* coef, const uint16_t* quant, uint8_t* scratch, uint8_t* rgb) {
    using namespace jpegmath;
    const JpegGeom& g = sg.g;
    const uint8_t* plane[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < g.ncomp; ++c) {
        uint8_t* out = scratch + sg.plane_offset(c);
        plane[c] = out;
        idct_plane(coef + g.block_offset(c) * 64, quant + 64 * c, g.bw(c), g.bh(c), sg.kc(c), out, sg.pitch(c));
    }
    const int ow = sg.ow(), oh = sg.oh(), mode = sg.chroma_mode();
    for (int y = 0; y < oh; ++y) {
        uint8_t* dst = rgb + (size_t)y * ow * 3;
        const uint8_t* yr = plane[0] + (size_t)y * sg.pitch(0);
        if (g.ncomp == 1) {
            for (int x = 0; x < ow; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = yr[x];
            continue;
        }
        for (int x = 0; x < ow; ++x) {
            const int cb = chroma_at(plane[1], sg.pitch(1), sg.cw(1), sg.ch(1), mode, x, y);
            const int cr = chroma_at(plane[2], sg.pitch(2), sg.cw(2), sg.ch(2), mode, x, y);
            ycc_to_rgb(yr[x], cb, cr, dst + 3 * x);
        }
    }
}

int jpeg_thread_allowance(int asked) {
    int n = 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n < 1) n = 1;
    if (n > 16) n = 16;
    if (asked > 0 && asked < n) n = asked;
    return n;
}

namespace {

// run fn(i) for i in [0, n) on up to `threads` workers (frames are independent)
template <class F>
void parallel_frames(int n, int threads, F fn) {
    const int t = jpeg_thread_allowance(threads) < n ? jpeg_thread_allowance(threads) : n;
    if (t <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    pool.reserve((size_t)t);
    for (int w = 0; w < t; ++w)
        pool.emplace_back([&] {
            for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
        });
    for (auto& th : pool) th.join();
}

bool geom_from_args(int W, int H, int ncomp, int hs, int vs, JpegGeom* g) {
    *g = JpegGeom{W, H, ncomp, hs, vs};
    return g->valid();
}

}  // namespace
}  // namespace tstar

// ---------------------------------------------------------------------------------------------- C ABI (include/tstar_hip.h)
using namespace tstar;

extern "C" {

int tstar_jpeg_probe(const uint8_t* data, size_t len, int32_t* info5) {
    char msg[160] = "";
    JpegGeom g;
    if (!info5) { set_error("tstar_jpeg_probe: null argument"); return JPEG_MALFORMED; }
    const int rc = jpeg_probe(data, len, &g, msg, sizeof(msg));
    info5[0] = g.W; info5[1] = g.H; info5[2] = g.ncomp; info5[3] = g.hs; info5[4] = g.vs;
    if (rc != JPEG_OK) set_error(std::string("tstar_jpeg_probe: ") + msg);
    return rc;
}

size_t tstar_jpeg_frame_end(const uint8_t* data, size_t len, size_t pos) { return jpeg_frame_end(data, len, pos); }

int tstar_jpeg_sizes(int W, int H, int ncomp, int hs, int vs, size_t* out2) {
    JpegGeom g;
    if (!out2 || !geom_from_args(W, H, ncomp, hs, vs, &g)) { set_error("tstar_jpeg_sizes: null argument or unsupported geometry"); return 1; }
    out2[0] = g.blocks();
    out2[1] = g.plane_bytes();
    return 0;
}

int tstar_jpeg_threads(int asked) { return jpeg_thread_allowance(asked); }

int tstar_jpeg_sizes_scaled(int W, int H, int ncomp, int hs, int vs, int scale, size_t* out4) {
    const JpegScaledGeom sg{JpegGeom{W, H, ncomp, hs, vs}, scale};
    if (!out4 || !sg.scale_ok() || !sg.g.valid()) {
        set_error("tstar_jpeg_sizes_scaled: null argument, unsupported geometry or a scale other than 1, 2, 4, 8");
        return 1;
    }
    out4[0] = (size_t)sg.ow();
    out4[1] = (size_t)sg.oh();
    out4[2] = scale == 1 ? sg.g.plane_bytes() : sg.plane_bytes();
    out4[3] = sg.covered() ? 1 : 0;
    return 0;
}

int tstar_jpeg_entropy_batch(const uint8_t* const* datas, const size_t* lens, int n, int W, int H, int ncomp, int hs, int vs,
                             int16_t* coef, uint16_t* quant, int threads, int32_t* status) {
    JpegGeom g;
    if (!datas || !lens || !coef || !quant || !status || n <= 0 || !geom_from_args(W, H, ncomp, hs, vs, &g)) {
        set_error("tstar_jpeg_entropy_batch: null argument, n <= 0 or unsupported geometry");
        return 1;
    }
    const size_t per = g.blocks() * 64;
    std::vector<std::string> msgs((size_t)n);
    parallel_frames(n, threads, [&](int i) {
        char msg[160] = "";
        status[i] = jpeg_entropy(datas[i], lens[i], g, coef + per * (size_t)i, quant + 192 * (size_t)i, msg, sizeof(msg));
        if (status[i] != JPEG_OK) msgs[(size_t)i] = msg;
    });
    for (int i = 0; i < n; ++i)
        if (status[i] != JPEG_OK) {
            set_error("tstar_jpeg_entropy_batch: frame " + std::to_string(i) + " of the batch: " + msgs[(size_t)i]);
            return 3;
        }
    return 0;
}

int tstar_jpeg_plan_segments(const uint8_t* const* datas, const size_t* lens, const uint64_t* byte_offsets, int n, int W, int H,
                             int ncomp, int hs, int vs, int32_t* route, void* frames, uint16_t* quant, void* table_sets,
                             int cap_sets, void* segments, int cap_segments, size_t* out5) {
    JpegGeom g;
    if (!datas || !lens || !byte_offsets || !route || !frames || !quant || !out5 || n <= 0 || cap_sets < 0 || cap_segments < 0 ||
        (cap_sets > 0 && !table_sets) || (cap_segments > 0 && !segments) || !geom_from_args(W, H, ncomp, hs, vs, &g)) {
        set_error("tstar_jpeg_plan_segments: null argument, n <= 0 or unsupported geometry");
        return 1;
    }
    struct { std::vector<JpegTableSet> sets; std::vector<JpegSegment> segments; } plan;
    if (!jpeg_plan_segments(datas, lens, byte_offsets, n, g, route, (JpegFrameDesc*)frames, quant, &plan.sets, &plan.segments)) {
        set_error("tstar_jpeg_plan_segments: a frame ends beyond the 32-bit byte offsets of a segment");
        return 1;
    }
    out5[0] = plan.sets.size();
    out5[1] = plan.segments.size();
    out5[2] = sizeof(JpegTableSet);
    out5[3] = sizeof(JpegSegment);
    out5[4] = sizeof(JpegFrameDesc);
    if (plan.sets.size() > (size_t)cap_sets || plan.segments.size() > (size_t)cap_segments) {
        set_error("tstar_jpeg_plan_segments: " + std::to_string(plan.sets.size()) + " table sets and " +
                  std::to_string(plan.segments.size()) + " segments do not fit the given buffers");
        return 4;
    }
    if (!plan.sets.empty()) memcpy(table_sets, (const void*)plan.sets.data(), plan.sets.size() * sizeof(JpegTableSet));
    if (!plan.segments.empty()) memcpy(segments, plan.segments.data(), plan.segments.size() * sizeof(JpegSegment));
    return 0;
}

int tstar_jpeg_entropy_segments_host(const uint8_t* bytes, size_t total_bytes, const void* segments, const void* table_sets,
                                     int n_sets, const void* frames, int n_frames, int n_segments, int W, int H, int ncomp,
                                     int hs, int vs, int16_t* coef, int32_t* seg_status) {
    JpegGeom g;
    if (!geom_from_args(W, H, ncomp, hs, vs, &g) ||
        !jpeg_entropy_segments_host(bytes, total_bytes, (const JpegSegment*)segments, (const JpegTableSet*)table_sets, n_sets,
                                    (const JpegFrameDesc*)frames, n_frames, n_segments, g, coef, seg_status)) {
        set_error("tstar_jpeg_entropy_segments_host: null argument, empty batch or unsupported geometry");
        return 1;
    }
    return 0;
}

size_t tstar_jpeg_split_workspace_bytes(size_t total_bytes, int n_segments, int sub_bytes) {
    return jpeg_split_workspace_bytes(total_bytes, n_segments, sub_bytes);
}

int tstar_jpeg_entropy_split_host(const uint8_t* bytes, size_t total_bytes, const void* segments, const void* table_sets, int n_sets,
                                  const void* frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs, int vs,
                                  int sub_bytes, int min_split_bytes, int max_rounds, void* workspace, size_t workspace_bytes,
                                  int16_t* coef, int32_t* seg_status, int32_t* seg_info) {
    JpegGeom g;
    if (!geom_from_args(W, H, ncomp, hs, vs, &g) ||
        !jpeg_entropy_split_host(bytes, total_bytes, (const JpegSegment*)segments, (const JpegTableSet*)table_sets, n_sets,
                                 (const JpegFrameDesc*)frames, n_frames, n_segments, g, sub_bytes, min_split_bytes, max_rounds, workspace,
                                 workspace_bytes, coef, seg_status, seg_info)) {
        set_error("tstar_jpeg_entropy_split_host: null argument, empty batch, unsupported geometry, sub_bytes below " +
                  std::to_string(jpegcore::kSubBytesMin) + " or no multiple of 4, max_rounds outside 1.." +
                  std::to_string(kJpegSplitMaxRounds) + ", or a workspace that is misaligned or too small");
        return 1;
    }
    return 0;
}

int tstar_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* quant, int n, int W, int H, int ncomp, int hs, int vs,
                                uint8_t* rgb, int threads) {
    JpegGeom g;
    if (!coef || !quant || !rgb || n <= 0 || !geom_from_args(W, H, ncomp, hs, vs, &g)) {
        set_error("tstar_jpeg_reconstruct_host: null argument, n <= 0 or unsupported geometry");
        return 1;
    }
    const size_t per = g.blocks() * 64, frame = (size_t)W * H * 3;
    parallel_frames(n, threads, [&](int i) {
        std::vector<uint8_t> scratch(g.plane_bytes());
        jpeg_reconstruct_host(g, coef + per * (size_t)i, quant + 192 * (size_t)i, scratch.data(), rgb + frame * (size_t)i);
    });
    return 0;
}

int tstar_jpeg_reconstruct_scaled_host(const int16_t* coef, const uint16_t* quant, int n, int W, int H, int ncomp, int hs, int vs,
                                       int scale, uint8_t* rgb, int threads) {
    if (scale == 1) return tstar_jpeg_reconstruct_host(coef, quant, n, W, H, ncomp, hs, vs, rgb, threads);
    const JpegScaledGeom sg{JpegGeom{W, H, ncomp, hs, vs}, scale};
    if (!coef || !quant || !rgb || n <= 0 || !sg.covered()) {
        set_error("tstar_jpeg_reconstruct_scaled_host: null argument, n <= 0, a scale other than 1, 2, 4, 8 or a geometry that is not "
                  "covered at this scale");
        return 1;
    }
    const size_t per = sg.g.blocks() * 64, frame = (size_t)sg.ow() * sg.oh() * 3;
    parallel_frames(n, threads, [&](int i) {
        std::vector<uint8_t> scratch(sg.plane_bytes());
        jpeg_reconstruct_scaled_host(sg, coef + per * (size_t)i, quant + 192 * (size_t)i, scratch.data(), rgb + frame * (size_t)i);
    });
    return 0;
}

}  // extern "C"
