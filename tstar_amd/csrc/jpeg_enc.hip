// Baseline JPEG encoder, device half: RGB u8 frames of a resident store, gathered by an index list -> per frame the stuffed
// entropy-coded bytes of one interleaved scan (the header is the same for every frame and is joined on the host).  The
// integers are those of jpeg_enc_math.h, shared with the host twin (jpeg_enc_host.cpp): byte-equal to libjpeg-turbo as
// Pillow drives it.  Layouts, the workspace and the capacity rule: jpeg_enc_host.h.
//
//   block stage    jpeg_enc_blocks_kernel    colour conversion, chroma downsampling, level shift, forward DCT, quantisation
//                                            -> int16 coefficients in the decoder's layout
//                  jpeg_enc_dummy_dc_kernel  DC of the dummy luma blocks of the last MCU column / row (a lookup of a real block)
//   entropy stage  jpeg_enc_bits_kernel<0>   bit length of every block's codes (one lane per block, scan order)
//                                            [R] the DC predictor is cut at every interval
//                  jpeg_enc_offsets_kernel   exclusive sum per frame -> bit offsets, the scan's size, whether it can fit
//                                            [R] a second sum, of every interval's bits rounded up to a byte plus its marker's 16:
//                                            a block starts at its interval's first bit plus the bits before it inside the
//                                            interval; the byte offset of every marker goes into a sorted table
//                  jpeg_enc_bits_kernel<1>   the same walk again, writing the bits into the zeroed unstuffed stream: whole words
//                                            stored, the two boundary words of a block merged by atomicOr (commutative: the
//                                            result does not depend on the order of arrival)
//                                            [R] the lane of an interval's last block also writes the one-bits that fill its byte
//                                            and the marker, so the unstuffed stream holds both
//   stuffing       jpeg_enc_ff_kernel<0>     0xFF bytes per chunk of 64 unstuffed bytes
//                  jpeg_enc_lengths_kernel   exclusive sum per frame -> where each chunk lands, the frame's length and status
//                  jpeg_enc_ff_kernel<1>     scatter with FF 00, one-bits in the last byte, EOI; only into slots that fit
//                                            [R] both passes: a chunk's lane finds its first marker in the table by bisection; the
//                                            marker's FF is neither counted nor followed by 00 (its second byte, D0..D7, is no
//                                            0xFF anyway)
//
// [R]: only with a restart interval (jpeg_enc_math.h, "scan order").  The interval is an argument of the one scan launcher; the
// kernels of the entropy stage and the stuffing passes take it as the compile-time parameter RST, so a scan without markers runs
// none of the [R] steps and its kernels get no RestartArgs at all (RestartOf<false> is empty: there is nothing they could read).
// Where the four code tables of a frame come from is the bits kernel's third compile-time parameter TAB, handled the same way:
// TAB_STD reads the Annex K tables in constant memory and gets an empty StdTables.
//
// With optimised tables (Pillow's optimize=True; jpeg_enc_math.h, "optimised tables") two stages run in front of the entropy stage
// and the two bits passes code with the frame's own tables; nothing is read back in between, and a scan with the standard tables
// launches none of this:
//   tables         jpeg_enc_hist_kernel      the symbols of the block walk counted into the frame's four histograms [4][257]
//                  jpeg_enc_tables_kernel    one wave per (frame, table): histogram -> HuffSpecWide (what the DHT segment needs) and
//                                            HuffCodes (what the bits kernel needs), or a status
//   entropy stage  jpeg_enc_bits_kernel<WRITE, RST, TAB_FRAME>  the same lane body behind a staging of the frame's four code tables
//                                            into LDS
//   status         jpeg_enc_table_status_kernel<TAB_FRAME>  a frame with a table that has a status (never written) reports
//                                            JPEG_ENC_HUFF_OVERFLOW
//
// With SHARED tables (tstar_jpeg_encode_scan_grp: the re-coding of a compressed-resident arena) the frames of a GROUP are coded with one
// set of tables built from the sum of their counts; the launches above with
//   tables         jpeg_enc_group_sum_kernel   behind the histogram launch: one lane per bin adds the group's frames in frame order and
//                                              stores the sum once (no atomics)
//                  jpeg_enc_tables_kernel      one wave per (GROUP, table), on the sums
//                  jpeg_enc_group_flag_kernel  the frames of a group with a status, and the frames without a group, are never written
//   entropy stage  jpeg_enc_bits_kernel<WRITE, RST, TAB_GROUP>  stages the tables of the frame's group (frame -> table-row indirection)
//   status         jpeg_enc_table_status_kernel<TAB_GROUP>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/tstar_hip.h"
#include "common.h"
#include "jpeg_enc_host.h"

namespace tstar {

namespace {

__constant__ jpegenc::EncTables kDevTables = jpegenc::make_tables();
__constant__ uint8_t kDevZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kBlocksPerWg = 32;       // 256 threads: 8 lanes per 8x8 block
constexpr int kRowPitch = 9;           // LDS dwords per block row, 72 per block: the bank argument of jpeg.hip's IDCT kernel
constexpr int kBlockPitch = 72;

struct EncQuant { uint16_t q[3][64]; };                       // by value in the kernel arguments (384 bytes)

struct BlockArgs {
    const uint8_t* frames;      // [N][H][W][3]
    const int32_t* idx;         // [n]
    int16_t* coef;              // [n][blocks][64]
    int N, H, W, hs, vs;
    int bw[3], bh[3];           // padded blocks of each component
    int off[3];                 // first block of each component in a frame's layout
    int real_bw, real_bh;       // luma blocks that hold picture
    int blocks;                 // per frame
    int dwords;                 // 1: frames and rows are dword-aligned (4 | W and an aligned store)
    size_t total_blocks;
};

// npx (8 or 16) consecutive pixels of a row starting at x0 -> R | G << 8 | B << 16 each.  Inside the picture and dword-aligned
// (x0 is a multiple of 8, so 3 * x0 of 24): 3 * npx / 4 dword loads.  Otherwise byte loads with the column clamped.
template <int NPX>
__device__ __forceinline__ void load_span(const uint8_t* __restrict__ row, int x0, int W, int dwords, uint32_t (&px)[NPX]) {
    if (dwords && x0 + NPX <= W) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(row + 3 * (size_t)x0);
        uint32_t w[NPX * 3 / 4];
#pragma unroll
        for (int k = 0; k < NPX * 3 / 4; ++k) w[k] = p[k];
#pragma unroll
        for (int k = 0; k < NPX / 4; ++k) {
            px[4 * k] = w[3 * k] & 0xffffffu;
            px[4 * k + 1] = (w[3 * k] >> 24) | ((w[3 * k + 1] & 0xffffu) << 8);
            px[4 * k + 2] = (w[3 * k + 1] >> 16) | ((w[3 * k + 2] & 0xffu) << 16);
            px[4 * k + 3] = w[3 * k + 2] >> 8;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const int x = x0 + k < W ? x0 + k : W - 1;
            const uint8_t* p = row + 3 * (size_t)x;
            px[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
    }
}

__device__ __forceinline__ int comp_of(int c, uint32_t px) {
    return jpegenc::rgb_to_comp(c, (int)(px & 255), (int)((px >> 8) & 255), (int)(px >> 16));
}

// One workgroup = 32 consecutive blocks of the chunk (frame after frame, a frame's blocks in layout order).
//   rows    lane (block, r) gathers the 8 samples of row r of its block (luma: 8 pixels of one picture row; subsampled chroma:
//           16 pixels of one or two rows, box-filtered), subtracts 128, runs the row pass in registers and parks it in LDS;
//   cols    lane (block, c) runs the column pass on column c, quantises and writes back in place;
//   store   lane (block, r) packs row r to eight int16 and stores them as one 16-byte vector (a wave writes 1 KiB contiguous).
// Dummy luma blocks are written as zeros here; jpeg_enc_dummy_dc_kernel fills their DC.
__global__ __launch_bounds__(256) void jpeg_enc_blocks_kernel(BlockArgs a, EncQuant eq) {
    __shared__ int32_t ws[kBlocksPerWg * kBlockPitch];
    const int t = threadIdx.x, bl = t >> 3, r = t & 7;
    const size_t gb = (size_t)blockIdx.x * kBlocksPerWg + bl;
    const bool live = gb < a.total_blocks;
    int c = 0, by = 0, bx = 0;
    size_t f = 0;
    bool real = false;
    if (live) {
        f = gb / (size_t)a.blocks;
        const int g = (int)(gb % (size_t)a.blocks);
        c = g >= a.off[2] ? 2 : (g >= a.off[1] ? 1 : 0);
        const int gi = g - a.off[c];
        by = gi / a.bw[c];
        bx = gi % a.bw[c];
        real = c != 0 || (by < a.real_bh && bx < a.real_bw);
    }
    int32_t* mine = ws + bl * kBlockPitch;
    if (live && real) {
        int fi = a.idx[f];
        fi = fi < 0 ? 0 : (fi >= a.N ? a.N - 1 : fi);          // the entry checks what the host can see; a bad index never leaves the store
        const uint8_t* frame = a.frames + (size_t)fi * a.H * a.W * 3;
        int32_t d[8];
        if (c == 0 || a.hs == 1) {
            const int y = by * 8 + r < a.H ? by * 8 + r : a.H - 1;
            uint32_t px[8];
            load_span<8>(frame + (size_t)y * a.W * 3, bx * 8, a.W, a.dwords, px);
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = comp_of(c, px[k]) - 128;
        } else {
            const int oy = jpegenc::comp_row(c, by * 8 + r, a.H, a.vs);
            int32_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < a.vs; ++j) {
                const int y = oy * a.vs + j < a.H ? oy * a.vs + j : a.H - 1;
                uint32_t px[16];
                load_span<16>(frame + (size_t)y * a.W * 3, bx * 16, a.W, a.dwords, px);
#pragma unroll
                for (int k = 0; k < 8; ++k) sum[k] += comp_of(c, px[2 * k]) + comp_of(c, px[2 * k + 1]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int ox = bx * 8 + k;
                d[k] = (a.vs == 2 ? (sum[k] + jpegenc::h2v2_bias(ox)) >> 2 : (sum[k] + jpegenc::h2v1_bias(ox)) >> 1) - 128;
            }
        }
        int32_t o[8];
        jpegenc::fdct8<true>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) mine[r * kRowPitch + k] = o[k];
    }
    __syncthreads();
    if (live && real) {
        const int col = r;
        int32_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = mine[k * kRowPitch + col];
        jpegenc::fdct8<false>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) mine[k * kRowPitch + col] = jpegenc::quantise(o[k], (int)eq.q[c][k * 8 + col]);
    }
    __syncthreads();
    if (live) {
        uint4 v = {0, 0, 0, 0};
        if (real) {
            const int32_t* row = mine + r * kRowPitch;
            v.x = ((uint32_t)row[0] & 0xffffu) | ((uint32_t)row[1] << 16);
            v.y = ((uint32_t)row[2] & 0xffffu) | ((uint32_t)row[3] << 16);
            v.z = ((uint32_t)row[4] & 0xffffu) | ((uint32_t)row[5] << 16);
            v.w = ((uint32_t)row[6] & 0xffffu) | ((uint32_t)row[7] << 16);
        }
        *reinterpret_cast<uint4*>(a.coef + gb * 64 + r * 8) = v;
    }
}

// one lane per luma block of the chunk: a dummy block copies the DC of the real block jpegenc::dummy_source names
__global__ __launch_bounds__(256) void jpeg_enc_dummy_dc_kernel(int16_t* __restrict__ coef, int blocks, int bw0, int bh0, int real_bw,
                                                                int real_bh, int hs, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int per = bw0 * bh0;
    const size_t f = i / (size_t)per;
    const int g = (int)(i % (size_t)per), by = g / bw0, bx = g % bw0;
    int kind;
    const int src = jpegenc::dummy_source(by, bx, real_bw, real_bh, hs, bw0, &kind);
    if (src < 0) return;
    int16_t* fc = coef + f * (size_t)blocks * 64;
    fc[(size_t)g * 64] = fc[(size_t)src * 64];
}

// ------------------------------------------------------------------------------------------------ entropy stage
enum { META_BITS = 0, META_BYTES = 1, META_FF = 2, META_FLAGS = 3 };
enum { FLAG_BAD_COEF = 1, FLAG_SKIP = 2 };          // SKIP: the unstuffed bytes alone exceed the slot; nothing of the frame is written

struct EntropyArgs {
    const int16_t* coef;
    uint32_t* meta;             // [n][4]
    uint32_t* bits;             // [n][blocks]
    uint32_t* raw;              // [n][raw_words]
    jpegenc::ScanGeom sg;
    int blocks;
    uint32_t raw_words;
};

struct CountPut {
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(unsigned, int len) { n += (uint32_t)len; }
};

// Writes the bits of one block at bit offset `pos` of a big-endian word stream.  A word is stored whole when every bit of it
// is this block's; the first and the last word of the block, which neighbours share, are merged by atomicOr into the zeroed
// buffer.  Nothing is written at or beyond word `limit`.
struct WritePut {
    uint32_t* words;
    uint32_t w, limit;
    uint64_t acc = 0;
    int nb;
    bool first = true;
    __device__ __forceinline__ WritePut(uint32_t* words_, uint32_t pos, uint32_t limit_) : words(words_), w(pos >> 5), limit(limit_), nb((int)(pos & 31)) {}
    __device__ __forceinline__ void emit(uint32_t v) {
        if (w < limit) {
            if (first) atomicOr(words + w, v);
            else words[w] = v;
        }
        first = false;
        ++w;
    }
    __device__ __forceinline__ void operator()(unsigned code, int len) {
        acc = (acc << len) | code;
        nb += len;
        if (nb >= 32) {
            nb -= 32;
            emit((uint32_t)(acc >> nb));
            acc &= (1ull << nb) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nb && w < limit) atomicOr(words + w, (uint32_t)(acc << (32 - nb)));
    }
    __device__ __forceinline__ int bits_in_byte() const { return nb & 7; }       // of the position behind the last put
};

constexpr uint32_t kMarkPadded = 0x80000000u;          // a byte offset is below 2^29: bit offsets fit 32 bits

struct RestartArgs {
    uint32_t* seg;              // [n][markers + 1]
    uint32_t* mark;             // [n][markers]
    uint32_t* counters;         // [n][3] (JPEG_ENC_R_*) or null
    int interval;               // MCUs
    int seg_blocks;             // blocks of a full interval
    uint32_t markers;           // per frame
};
struct NoRestart {};            // what the RST = false forms get in its place: no member, so no read of one compiles
template <bool RST>
using RestartOf = std::conditional_t<RST, RestartArgs, NoRestart>;

// grid (ceil(blocks / 256), n): lane k of frame f walks the k-th block of the scan.  The DC predictor is the quantised DC of the
// previous block of the component, a lookup in the coefficients.  RST, WRITE: block k of interval s starts at seg[s] + bits[k] -
// bits[first block of s]; the lane of the last block of an interval that a marker follows appends up to 7 one-bits and the
// marker's 16.
// codes: the four code tables of the frame (the Annex K ones in constant memory, or the frame's own, staged in LDS)
template <int WRITE, bool RST>
__device__ __forceinline__ void bits_lane(const EntropyArgs& a, const RestartOf<RST>& r, const jpegenc::HuffCodes* codes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (k >= a.blocks) return;
    uint32_t* meta = a.meta + (size_t)f * 4;
    if (WRITE && meta[META_FLAGS]) return;
    int interval = 0;
    if constexpr (RST) interval = r.interval;
    int c, b, pb;
    jpegenc::scan_block(a.sg, k, interval, &c, &b, &pb);
    const int16_t* fc = a.coef + (size_t)f * a.blocks * 64;
    const int pred = pb < 0 ? 0 : fc[(size_t)pb * 64];
    const jpegenc::HuffCodes& dc = codes[c ? 2 : 0];
    const jpegenc::HuffCodes& ac = codes[c ? 3 : 1];
    if (WRITE) {
        const uint32_t* bits = a.bits + (size_t)f * a.blocks;
        [[maybe_unused]] uint32_t s = 0, first = 0;
        uint32_t pos = bits[k];
        if constexpr (RST) {
            s = (uint32_t)(k / r.seg_blocks);
            first = s * (uint32_t)r.seg_blocks;
            pos = r.seg[(size_t)f * (r.markers + 1) + s] + bits[k] - bits[first];
        }
        WritePut put(a.raw + (size_t)f * a.raw_words, pos, a.raw_words);
        jpegenc::encode_block(fc + (size_t)b * 64, pred, dc, ac, kDevZigzag, put);
        if constexpr (RST) {
            if (s < r.markers && (uint32_t)k + 1 == first + (uint32_t)r.seg_blocks) {
                const int fill = (8 - put.bits_in_byte()) & 7;
                if (fill) put((1u << fill) - 1u, fill);
                put(0xFFD0u | (s & 7u), 16);
            }
        }
        put.finish();
    } else {
        CountPut put;
        const jpegenc::BlockEvents ev = jpegenc::encode_block(fc + (size_t)b * 64, pred, dc, ac, kDevZigzag, put);
        a.bits[(size_t)f * a.blocks + k] = put.n;
        if (ev.bad) atomicOr(meta + META_FLAGS, (uint32_t)FLAG_BAD_COEF);
    }
}

// ------------------------------------------------------------------------------------------------ table source
// The frames of a group are coded with ONE set of four tables, built from the sum of their counts.  group i32 [n]: a frame's group
// (-1: not coded); span i32 [n_groups][2]: the first frame of a group and the frame behind its last.  Both come from the host, which
// has checked its copy (jpeg_enc_groups_check); the kernels still trust neither: a group outside 0 .. n_groups - 1 counts as -1, a
// span is clipped to the n frames.
struct GroupArgs {
    const int32_t* group;       // [n]
    const int32_t* span;        // [n_groups][2]
    uint32_t* hist;             // [n_groups][4][257]
    int n_groups;
};
struct OwnRow {};               // what TAB_FRAME gets in its place: row f of a table array belongs to frame f

// Where the four code tables of a frame come from: the Annex K ones in constant memory, row f of an array in HBM (the frame's own), or
// the row of the frame's group.  RowsOf<TAB> maps a frame to its row (-1: none, only with groups); TablesOf<TAB> is what the bits
// kernel gets: nothing at all, the codes pointer, or the codes pointer and the groups.
constexpr int TAB_STD = 0, TAB_FRAME = 1, TAB_GROUP = 2;
template <int TAB>
using RowsOf = std::conditional_t<TAB == TAB_GROUP, GroupArgs, OwnRow>;
template <class F>
__device__ __forceinline__ F table_row(const OwnRow&, F f) { return f; }        // as it is: an unsigned index stays one
__device__ __forceinline__ int table_row(const GroupArgs& ga, int f) {
    const int g = ga.group[f];
    return g >= 0 && g < ga.n_groups ? g : -1;
}
struct StdTables {};            // no member, as NoRestart
template <int TAB>
struct RowTables {
    const jpegenc::HuffCodes* codes;                    // [rows][4]
    [[no_unique_address]] RowsOf<TAB> rows;
};
template <int TAB>
using TablesOf = std::conditional_t<TAB == TAB_STD, StdTables, RowTables<TAB>>;

constexpr int kHist = jpegenc::kHuffSymbols;           // 257 bins per table
constexpr uint32_t kTableWords = 4 * sizeof(jpegenc::HuffCodes) / 4;       // 768 dwords: a frame's four code tables

// TAB_FRAME, TAB_GROUP: the workgroup stages the four tables of its frame's row in LDS (4 x 768 bytes) once.  A frame without a group
// stages tables without a code (every length 0); it is flagged and never written.
template <int WRITE, bool RST, int TAB>
__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(EntropyArgs a, RestartOf<RST> r, TablesOf<TAB> t) {
    if constexpr (TAB == TAB_STD) {
        bits_lane<WRITE, RST>(a, r, kDevTables.codes);
    } else {
        __shared__ alignas(16) jpegenc::HuffCodes tab[4];
        const auto row = table_row(t.rows, blockIdx.y);         // uniform over the workgroup
        const bool none = TAB == TAB_GROUP && (int)row < 0;
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(t.codes + (size_t)(none ? 0 : row) * 4);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
        for (uint32_t i = threadIdx.x; i < kTableWords; i += 256) dst[i] = none ? 0u : src[i];
        __syncthreads();
        bits_lane<WRITE, RST>(a, r, tab);
    }
}

// ------------------------------------------------------------------------------------------------ optimised tables
// blocks -> histogram -> tables -> bits (count) -> offsets -> bits (write) -> stuffing; nothing is read back in between.

// grid (ceil(blocks / 1024), n): a workgroup walks 1024 consecutive blocks of one frame's scan, four per lane, and counts their
// symbols into histograms in LDS; the bins that are not zero are then added to the frame's (zeroed) hist [4][257].  Neighbouring
// lanes meet on the same few bins (EOB, the small DC categories) at the same instruction, and LDS atomics on one address take
// turns: the workgroup keeps kHistCopies copies of the four histograms, lane l counts into copy l mod kHistCopies (their bins lie
// in different banks: a copy is 1028 dwords), and the flush sums them.
constexpr int kHistCopies = 8;
constexpr int kHistBlocksPerWg = 1024;
__global__ __launch_bounds__(256) void jpeg_enc_hist_kernel(EntropyArgs a, int interval, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kHistCopies * 4 * kHist];
    const int f = blockIdx.y;
    for (int i = threadIdx.x; i < kHistCopies * 4 * kHist; i += 256) h[i] = 0;
    __syncthreads();
    const int16_t* fc = a.coef + (size_t)f * a.blocks * 64;
    uint32_t* copy = h + (threadIdx.x % kHistCopies) * 4 * kHist;
    for (int j = 0; j < kHistBlocksPerWg / 256; ++j) {
        const int k = blockIdx.x * kHistBlocksPerWg + j * 256 + (int)threadIdx.x;
        if (k >= a.blocks) break;
        int c, b, pb;
        jpegenc::scan_block(a.sg, k, interval, &c, &b, &pb);
        const int pred = pb < 0 ? 0 : fc[(size_t)pb * 64];
        uint32_t* mine = copy + (c ? 2 : 0) * kHist;
        jpegenc::gather_block(fc + (size_t)b * 64, pred, kDevZigzag, [&](int ac, int sym) { atomicAdd(mine + ac * kHist + sym, 1u); });
    }
    __syncthreads();
    uint32_t* fh = hist + (size_t)f * 4 * kHist;
    for (int i = threadIdx.x; i < 4 * kHist; i += 256) {
        uint32_t sum = 0;
#pragma unroll
        for (int r = 0; r < kHistCopies; ++r) sum += h[r * 4 * kHist + i];
        if (sum) atomicAdd(fh + i, sum);
    }
}

// smallest key of the wave (64 lanes), in every lane
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// grid (4, n), one wave: table t of frame f from its histogram (jpegenc::huff_optimal's result, found in parallel).
//   merges  lane l holds the counts of symbols l, l + 64, ... (five registers; 256 is the reserved symbol, count 1).  The two
//           smallest of a merge are wave minima of the key count << 9 | 511 - index (ties go to the LARGEST index, as libjpeg's
//           upward scan with <= leaves them); every lane learns both and updates its own registers, lane 0 records the merge
//           as a node with two parent links.
//   depths  one leaf per lane walks its links to the root: the code size.  A size above 32 is the overflow status.
//   table   lane 0 counts and limits the lengths (32 steps); every lane ranks its symbols for huffval (size, then value);
//           lane 0 assigns the canonical codes.  Spec and codes leave LDS as dwords.
__global__ __launch_bounds__(64) void jpeg_enc_tables_kernel(const uint32_t* __restrict__ hist, jpegenc::HuffSpecWide* __restrict__ specs,
                                                             jpegenc::HuffCodes* __restrict__ codes, uint32_t* __restrict__ meta) {
    __shared__ uint16_t node[kHist], parent[2 * kHist];
    __shared__ uint8_t size[kHist + 3];
    __shared__ int bits[jpegenc::kHuffMaxClen + 1];
    __shared__ alignas(16) jpegenc::HuffSpecWide spec;
    __shared__ alignas(16) jpegenc::HuffCodes tab;
    const int lane = threadIdx.x, t = blockIdx.x, f = blockIdx.y;
    const uint32_t* fh = hist + ((size_t)f * 4 + t) * kHist;
    uint32_t cnt[5];
    uint32_t present = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        cnt[j] = i < 256 ? fh[i] : (i == 256 ? 1u : 0u);
        if (cnt[j]) present |= 1u << j;
        if (i < kHist) node[i] = (uint16_t)i;
    }
    for (int i = lane; i < 2 * kHist; i += 64) parent[i] = 0xFFFF;
    for (int i = lane; i < (int)(sizeof(spec) / 4); i += 64) reinterpret_cast<uint32_t*>(&spec)[i] = 0;
    for (int i = lane; i < (int)(sizeof(tab) / 4); i += 64) reinterpret_cast<uint32_t*>(&tab)[i] = 0;
    if (lane <= jpegenc::kHuffMaxClen) bits[lane] = 0;
    __syncthreads();
    constexpr uint64_t kNone = ~0ull;
    for (int next = kHist;; ++next) {
        uint64_t k1 = kNone;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (cnt[j]) {
                const uint64_t key = ((uint64_t)cnt[j] << 9) | (uint64_t)(511 - (lane + 64 * j));
                k1 = key < k1 ? key : k1;
            }
        k1 = wave_min_u64(k1);
        const int c1 = 511 - (int)(k1 & 511u);
        uint64_t k2 = kNone;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (cnt[j] && lane + 64 * j != c1) {
                const uint64_t key = ((uint64_t)cnt[j] << 9) | (uint64_t)(511 - (lane + 64 * j));
                k2 = key < k2 ? key : k2;
            }
        k2 = wave_min_u64(k2);
        if (k2 == kNone) break;                        // one tree is left (wave-uniform)
        const int c2 = 511 - (int)(k2 & 511u);
        const uint32_t sum = (uint32_t)(k1 >> 9) + (uint32_t)(k2 >> 9);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (lane + 64 * j == c1) cnt[j] = sum;
            if (lane + 64 * j == c2) cnt[j] = 0;
        }
        if (lane == 0) {                               // at most 256 merges: next stays below 2 * 257
            parent[node[c1]] = (uint16_t)next;
            parent[node[c2]] = (uint16_t)next;
            node[c1] = (uint16_t)next;
        }
    }
    __syncthreads();
    int deepest = 0, symbols = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        int d = 0;
        if (present & (1u << j))
            for (int p = i; parent[p] != 0xFFFF; p = parent[p]) ++d;
        if (i < kHist) size[i] = (uint8_t)d;           // at most 256
        deepest = d > deepest ? d : deepest;
        symbols += i < 256 && (present & (1u << j));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(deepest, d, 64);
        deepest = o > deepest ? o : deepest;
        symbols += __shfl_xor(symbols, d, 64);
    }
    __syncthreads();
    const int status = symbols == 0 ? jpegenc::HUFF_EMPTY : (deepest > jpegenc::kHuffMaxClen ? jpegenc::HUFF_CLEN_OVERFLOW : jpegenc::HUFF_OK);
    if (status == jpegenc::HUFF_OK) {                  // wave-uniform
        if (lane == 0) {
            for (int i = 0; i < kHist; ++i)
                if (size[i]) ++bits[size[i]];
            jpegenc::huff_limit_bits(bits, nullptr);
            for (int i = 0; i < 16; ++i) spec.bits[i] = (uint8_t)bits[i + 1];
            spec.nvals = (uint16_t)symbols;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lane + 64 * j;
            if (present & (1u << j)) spec.vals[jpegenc::huff_rank(size, i)] = (uint8_t)i;
        }
        __syncthreads();
        if (lane == 0) jpegenc::huff_assign_codes(spec, tab);
    } else if (lane == 0) {
        spec.status = (uint16_t)status;
        if (meta) atomicOr(meta + (size_t)f * 4 + META_FLAGS, (uint32_t)FLAG_SKIP);        // the frame is never written (null: f is a group)
    }
    __syncthreads();
    uint32_t* so = reinterpret_cast<uint32_t*>(specs + (size_t)f * 4 + t);
    uint32_t* co = reinterpret_cast<uint32_t*>(codes + (size_t)f * 4 + t);
    for (int i = lane; i < (int)(sizeof(spec) / 4); i += 64) so[i] = reinterpret_cast<const uint32_t*>(&spec)[i];
    for (int i = lane; i < (int)(sizeof(tab) / 4); i += 64) co[i] = reinterpret_cast<const uint32_t*>(&tab)[i];
}

// one lane per frame, behind the stuffing passes: a frame with a table that has a status reports it, with length 0; a frame without
// a group reports JPEG_ENC_HUFF_OVERFLOW whatever lies in its coefficients
template <int TAB>
__global__ __launch_bounds__(256) void jpeg_enc_table_status_kernel(const jpegenc::HuffSpecWide* __restrict__ specs, RowsOf<TAB> rows, uint32_t* lengths,
                                                                    int32_t* status, int n) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int row = table_row(rows, f);
    const bool none = TAB == TAB_GROUP && row < 0;
    bool bad = false;
    if (!none)
        for (int t = 0; t < 4; ++t) bad |= specs[(size_t)row * 4 + t].status != jpegenc::HUFF_OK;
    if (none || (bad && status[f] != JPEG_ENC_BAD_COEF)) {
        lengths[f] = 0;
        status[f] = JPEG_ENC_HUFF_OVERFLOW;
    }
}

// ------------------------------------------------------------------------------------------------ shared tables (groups of frames)
// grid (ceil(4 * 257 / 256), n_groups): lane i adds bin i of the group's frames IN FRAME ORDER into a register and stores the sum once:
// no atomic, no bin that two workgroups share (a video's EOB bin would otherwise take tens of thousands of atomics on one word),
// and the integer sum is the same in every run.  Four loads are in flight per lane; neighbouring lanes read neighbouring words.
__global__ __launch_bounds__(256) void jpeg_enc_group_sum_kernel(const uint32_t* __restrict__ hist, GroupArgs ga, int n) {
    const int i = blockIdx.x * 256 + (int)threadIdx.x, g = blockIdx.y;
    if (i >= 4 * kHist) return;
    int f0 = ga.span[2 * g], f1 = ga.span[2 * g + 1];
    f0 = f0 < 0 ? 0 : f0;
    f1 = f1 > n ? n : f1;
    uint32_t sum = 0;
    int f = f0;
    for (; f + 4 <= f1; f += 4) {
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ga.group[f + j] == g ? hist[(size_t)(f + j) * 4 * kHist + i] : 0u;
        sum += v[0]; sum += v[1]; sum += v[2]; sum += v[3];
    }
    for (; f < f1; ++f)
        if (ga.group[f] == g) sum += hist[(size_t)f * 4 * kHist + i];
    ga.hist[(size_t)g * 4 * kHist + i] = sum;
}

// one lane per frame, behind the tables: a frame without a group, or of a group one of whose tables has a status, is never written
__global__ __launch_bounds__(256) void jpeg_enc_group_flag_kernel(const jpegenc::HuffSpecWide* __restrict__ specs, GroupArgs ga, uint32_t* meta, int n) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int g = table_row(ga, f);
    bool bad = g < 0;
    if (!bad)
        for (int t = 0; t < 4; ++t) bad |= specs[(size_t)g * 4 + t].status != jpegenc::HUFF_OK;
    if (bad) atomicOr(meta + (size_t)f * 4 + META_FLAGS, (uint32_t)FLAG_SKIP);
}

// In-place exclusive sum of data[0 .. count) by one workgroup of 256 lanes, tiles of 1024 with a running carry; every lane
// returns the total.  Wave sums by shuffles, the four waves' sums through LDS.
__device__ uint32_t workgroup_exclusive_scan(uint32_t* data, uint32_t count) {
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < count; base += 1024) {
        const uint32_t i0 = base + (uint32_t)t * 4;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < count ? data[i0 + j] : 0u;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        uint32_t run = before + inc - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < count) data[i0 + j] = run;
            run += v[j];
        }
        __syncthreads();
        if (t == 255) carry_s = before + inc;
        __syncthreads();
    }
    return carry_s;
}

// grid (n): block lengths -> bit offsets; the scan's bits and unstuffed bytes; frames whose unstuffed bytes and EOI alone
// exceed the slot are marked and never written.
// RST: after the first sum bits[k] is the bits in front of block k without any padding; an interval that a marker follows takes
// its bits rounded up to a byte plus 16, the last one its bits alone; the second sum makes seg[s] the first bit of interval s.
// Marker s sits 16 bits in front of seg[s + 1].
template <bool RST>
__global__ __launch_bounds__(256) void jpeg_enc_offsets_kernel(uint32_t* bits, uint32_t* meta, int blocks, uint32_t slot_bytes, RestartOf<RST> r) {
    const int f = blockIdx.x, t = threadIdx.x;
    uint32_t* fb = bits + (size_t)f * blocks;
    uint32_t total = workgroup_exclusive_scan(fb, (uint32_t)blocks);              // < 2^32 by the plan's bound, padding and markers included
    [[maybe_unused]] uint32_t pad_free = 0;
    if constexpr (RST) {
        __shared__ uint32_t pad_free_s;
        uint32_t* seg = r.seg + (size_t)f * (r.markers + 1);
        uint32_t* mark = r.mark + (size_t)f * r.markers;
        const uint32_t data_bits = total;
        if (t == 0) pad_free_s = 0;
        __syncthreads();                               // every lane has the first total before the second sum starts its carry
        auto interval_bits = [&](uint32_t s) {
            const uint32_t first = s * (uint32_t)r.seg_blocks, next = first + (uint32_t)r.seg_blocks;
            return (next < (uint32_t)blocks ? fb[next] : data_bits) - fb[first];
        };
        for (uint32_t s = (uint32_t)t; s <= r.markers; s += 256) {
            const uint32_t d = interval_bits(s);
            seg[s] = s < r.markers ? ((d + 7u) & ~7u) + 16u : d;
        }
        __syncthreads();
        total = workgroup_exclusive_scan(seg, r.markers + 1);
        uint32_t aligned = 0;
        for (uint32_t s = (uint32_t)t; s < r.markers; s += 256) {
            const uint32_t d = interval_bits(s);
            mark[s] = ((seg[s + 1] - 16u) >> 3) | ((d & 7u) ? kMarkPadded : 0u);
            aligned += (d & 7u) == 0;
        }
        if (aligned) atomicAdd(&pad_free_s, aligned);
        __syncthreads();
        pad_free = pad_free_s;
    }
    if (t == 0) {
        uint32_t* m = meta + (size_t)f * 4;
        const uint32_t nbytes = (total >> 3) + ((total & 7u) ? 1u : 0u);
        m[META_BITS] = total;
        m[META_BYTES] = nbytes;
        if ((uint64_t)nbytes + 2 > slot_bytes) atomicOr(m + META_FLAGS, (uint32_t)FLAG_SKIP);
        if constexpr (RST) {
            if (r.counters) {
                r.counters[(size_t)f * JPEG_ENC_R_COUNTERS + JPEG_ENC_R_RST] = r.markers;
                r.counters[(size_t)f * JPEG_ENC_R_COUNTERS + JPEG_ENC_R_PAD_FREE] = pad_free;
            }
        }
    }
}

struct StuffArgs {
    const uint32_t* raw;
    uint32_t* meta;
    uint32_t* ff;               // [n][ff_chunks]
    uint8_t* out;               // [n][slot_bytes]
    uint32_t* lengths;
    int32_t* status;
    uint32_t raw_words, ff_chunks, slot_bytes;
};

// byte i of the unstuffed stream (i < nbytes); the last byte's unused low bits are ones
__device__ __forceinline__ uint32_t raw_byte(const uint32_t* raw, uint32_t i, uint32_t nbytes, uint32_t total_bits) {
    uint32_t b = (raw[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
    if (i + 1 == nbytes && (total_bits & 7u)) b |= (1u << (8 - (total_bits & 7u))) - 1u;
    return b;
}

// grid (ceil(ff_chunks / 256), n): one lane per chunk of 64 unstuffed bytes.  SCATTER = 0 counts its 0xFF bytes; SCATTER = 1
// writes the chunk at its place in the slot (its raw offset plus the 0xFF bytes before it) and, from the lane of the last
// chunk, EOI.  A frame whose status is not 0 is left alone, so every write lands inside [0, length) <= slot_bytes.
// RST: the unstuffed stream holds the markers, and byte mark[i] of it is a marker's FF, which is neither counted nor stuffed; the
// count pass also counts the padded bytes in front of a marker that came out as 0xFF.
template <int SCATTER, bool RST>
__global__ __launch_bounds__(256) void jpeg_enc_ff_kernel(StuffArgs a, RestartOf<RST> r) {
    const uint32_t chunk = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    const uint32_t* m = a.meta + (size_t)f * 4;
    if (m[META_FLAGS]) return;
    const uint32_t nbytes = m[META_BYTES], total_bits = m[META_BITS];
    const uint32_t begin = chunk * (uint32_t)kJpegEncStuffChunk;
    if (chunk >= a.ff_chunks || begin >= nbytes) return;
    const uint32_t end = begin + kJpegEncStuffChunk < nbytes ? begin + kJpegEncStuffChunk : nbytes;
    const uint32_t* raw = a.raw + (size_t)f * a.raw_words;
    [[maybe_unused]] const uint32_t* mark = nullptr;
    [[maybe_unused]] uint32_t mi = 0, next = 0xffffffffu;                          // the next marker and its table entry; no byte has offset 2^31 - 1
    if constexpr (RST) {
        mark = r.mark + (size_t)f * r.markers;
        uint32_t lo = 0, hi = r.markers;               // the first marker at or behind `begin`
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((mark[mid] & ~kMarkPadded) < begin) lo = mid + 1;
            else hi = mid;
        }
        mi = lo;
        if (mi < r.markers) next = mark[mi];
    }
    if (!SCATTER) {
        uint32_t n = 0;
        [[maybe_unused]] uint32_t pad_ff = 0;
        for (uint32_t i = begin; i < end; ++i) {
            if constexpr (RST) {
                if (i == (next & ~kMarkPadded)) {
                    if ((next & kMarkPadded) && raw_byte(raw, i - 1, nbytes, total_bits) == 255u) ++pad_ff;
                    ++mi;
                    next = mi < r.markers ? mark[mi] : 0xffffffffu;
                    continue;
                }
            }
            n += raw_byte(raw, i, nbytes, total_bits) == 255u;
        }
        a.ff[(size_t)f * a.ff_chunks + chunk] = n;
        if constexpr (RST) {
            if (pad_ff && r.counters) atomicAdd(r.counters + (size_t)f * JPEG_ENC_R_COUNTERS + JPEG_ENC_R_PAD_FF, pad_ff);
        }
    } else {
        if (a.status[f] != JPEG_ENC_OK) return;
        uint8_t* out = a.out + (size_t)f * a.slot_bytes;
        const uint32_t len = a.lengths[f];
        uint32_t o = begin + a.ff[(size_t)f * a.ff_chunks + chunk];
        for (uint32_t i = begin; i < end; ++i) {
            const uint32_t b = raw_byte(raw, i, nbytes, total_bits);
            if (o < len) out[o] = (uint8_t)b;
            ++o;
            if constexpr (RST) {
                if (i == (next & ~kMarkPadded)) {
                    ++mi;
                    next = mi < r.markers ? mark[mi] : 0xffffffffu;
                    continue;
                }
            }
            if (b == 255u) {
                if (o < len) out[o] = 0;
                ++o;
            }
        }
        if (end == nbytes && o + 2 == len) {
            out[o] = 0xFF;
            out[o + 1] = 0xD9;
        }
    }
}

// grid (n): chunk counts -> the count before each chunk; the frame's length (with EOI) and status
__global__ __launch_bounds__(256) void jpeg_enc_lengths_kernel(StuffArgs a) {
    const int f = blockIdx.x;
    uint32_t* m = a.meta + (size_t)f * 4;
    const uint32_t flags = m[META_FLAGS], nbytes = m[META_BYTES];
    uint32_t total = 0;
    if (!flags) {
        const uint32_t chunks = (nbytes + kJpegEncStuffChunk - 1) / kJpegEncStuffChunk;
        total = workgroup_exclusive_scan(a.ff + (size_t)f * a.ff_chunks, chunks < a.ff_chunks ? chunks : a.ff_chunks);
    }
    if (threadIdx.x == 0) {
        m[META_FF] = total;
        const uint64_t len = (uint64_t)nbytes + total + 2;
        if (flags & FLAG_BAD_COEF) {
            a.lengths[f] = 0;
            a.status[f] = JPEG_ENC_BAD_COEF;
        } else if (flags || len > a.slot_bytes) {
            // a skipped frame's 0xFF bytes were never counted: its length is a lower bound, which is all a short status promises
            a.lengths[f] = (uint32_t)(len > 0xffffffffull ? 0xffffffffull : len);
            a.status[f] = JPEG_ENC_SHORT;
        } else {
            a.lengths[f] = (uint32_t)len;
            a.status[f] = JPEG_ENC_OK;
        }
    }
}

}  // namespace

int jpeg_encode_blocks_u8(const uint8_t* frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, const JpegGeom& g,
                          int16_t* coef, hipStream_t s) {
    const JpegEncPlan p = plan_jpeg_encode(g, n, 2);
    TSTAR_REQUIRE(!p.error, std::string("jpeg_encode_blocks_u8: ") + (p.error ? p.error : ""));
    TSTAR_REQUIRE(N >= 1 && quality >= 1 && quality <= 100, "jpeg_encode_blocks_u8: empty store or quality outside 1..100");
    TSTAR_REQUIRE((uintptr_t)coef % 16 == 0, "jpeg_encode_blocks_u8: the coefficient buffer needs 16-byte alignment");
    BlockArgs a;
    a.frames = frames; a.idx = d_idx; a.coef = coef;
    a.N = N; a.H = H; a.W = W; a.hs = g.hs; a.vs = g.vs;
    for (int c = 0; c < 3; ++c) { a.bw[c] = g.bw(c); a.bh[c] = g.bh(c); a.off[c] = (int)g.block_offset(c); }
    a.real_bw = (W + 7) / 8; a.real_bh = (H + 7) / 8;
    a.blocks = (int)p.blocks;
    a.dwords = (W % 4 == 0 && (uintptr_t)frames % 4 == 0) ? 1 : 0;
    a.total_blocks = (size_t)n * p.blocks;
    EncQuant eq;
    jpeg_enc_quant(quality, &eq.q[0][0]);
    hipLaunchKernelGGL(jpeg_enc_blocks_kernel, dim3(p.block_wgs), dim3(256), 0, s, a, eq);
    TSTAR_HIP_CHECK(hipGetLastError());
    if (g.hs * g.vs > 1 && (g.bw(0) > a.real_bw || g.bh(0) > a.real_bh)) {
        const size_t total = (size_t)n * g.bw(0) * g.bh(0);
        hipLaunchKernelGGL(jpeg_enc_dummy_dc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, coef, a.blocks, g.bw(0), g.bh(0),
                           a.real_bw, a.real_bh, g.hs, total);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    return TSTAR_OK;
}

namespace {

// the six launches of the scan stage, with (RST) or without the interval-only steps, coding with the tables of TAB; tables that
// can have a status (specs: theirs) get the status launch behind them
template <bool RST, int TAB>
int launch_scan(const JpegEncPlan& p, int n, const EntropyArgs& e, const StuffArgs& a, const RestartOf<RST>& r, const TablesOf<TAB>& t,
                const jpegenc::HuffSpecWide* specs, hipStream_t s) {
    const dim3 egrid(p.entropy_wgs_x, (unsigned)n), sgrid(p.stuff_wgs_x, (unsigned)n);
    hipLaunchKernelGGL((jpeg_enc_bits_kernel<0, RST, TAB>), egrid, dim3(256), 0, s, e, r, t);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel<RST>, dim3((unsigned)n), dim3(256), 0, s, e.bits, e.meta, e.blocks, a.slot_bytes, r);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((jpeg_enc_bits_kernel<1, RST, TAB>), egrid, dim3(256), 0, s, e, r, t);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((jpeg_enc_ff_kernel<0, RST>), sgrid, dim3(256), 0, s, a, r);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_lengths_kernel, dim3((unsigned)n), dim3(256), 0, s, a);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((jpeg_enc_ff_kernel<1, RST>), sgrid, dim3(256), 0, s, a, r);
    TSTAR_HIP_CHECK(hipGetLastError());
    if constexpr (TAB != TAB_STD) {
        hipLaunchKernelGGL(jpeg_enc_table_status_kernel<TAB>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, specs, t.rows, a.lengths, a.status, n);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    return TSTAR_OK;
}

// the two stages in front of an optimised scan: 1 counts (into the zeroed histograms), 2 tables (from the histograms as they are)
// ga: stage 1 also sums the counts of every group's frames, stage 2 makes the tables of the GROUPS from those sums and flags the frames
int launch_tables(const JpegEncPlan& p, int n, const EntropyArgs& e, int restart, jpegenc::HuffSpecWide* specs, uint8_t* ws, int stages,
                  hipStream_t s, const GroupArgs* ga = nullptr) {
    TSTAR_REQUIRE((uintptr_t)specs % 4 == 0, "jpeg encode: the specs need 4-byte alignment");
    uint32_t* hist = (uint32_t*)(ws + p.off_hist);
    if (stages & 1) {
        TSTAR_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * 4 * kHist * sizeof(uint32_t), s));
        hipLaunchKernelGGL(jpeg_enc_hist_kernel, dim3((unsigned)((p.blocks + kHistBlocksPerWg - 1) / kHistBlocksPerWg), (unsigned)n), dim3(256), 0, s, e,
                           restart, hist);
        TSTAR_HIP_CHECK(hipGetLastError());
        if (ga) {
            hipLaunchKernelGGL(jpeg_enc_group_sum_kernel, dim3((4 * kHist + 255) / 256, (unsigned)ga->n_groups), dim3(256), 0, s, hist, *ga, n);
            TSTAR_HIP_CHECK(hipGetLastError());
        }
    }
    if ((stages & 2) && ga) {
        hipLaunchKernelGGL(jpeg_enc_tables_kernel, dim3(4, (unsigned)ga->n_groups), dim3(64), 0, s, ga->hist, specs,
                           (jpegenc::HuffCodes*)(ws + p.off_codes), (uint32_t*)nullptr);
        TSTAR_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(jpeg_enc_group_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, specs, *ga, e.meta, n);
        TSTAR_HIP_CHECK(hipGetLastError());
    } else if (stages & 2) {
        hipLaunchKernelGGL(jpeg_enc_tables_kernel, dim3(4, (unsigned)n), dim3(64), 0, s, hist, specs, (jpegenc::HuffCodes*)(ws + p.off_codes), e.meta);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    return TSTAR_OK;
}
// Where the code tables of a scan come from and which of its steps run.  specs null: the Annex K tables.  Else device HuffSpecWide out:
// [n][4], every frame coded with tables of its own; with ga [n_groups][4], every frame with the tables of its group.  stages: 1 counts,
// 2 tables (made from the histograms as they are), 4 scans (with the codes the workspace holds); the Annex K tables have the scans only.
struct TableSource {
    jpegenc::HuffSpecWide* specs = nullptr;
    const GroupArgs* ga = nullptr;
    int stages = 4;
};
}  // namespace

// The scan stage with a restart interval of `restart` MCUs (0: none), for the entry `who`: the one place that checks the plan and the
// workspace and fills the kernels' arguments.  d_rst_counters: optional u32 [n][3], zeroed here.  Without stage 4 nothing of out,
// lengths and status is used, and of the workspace only the flags are zeroed.
int jpeg_encode_scan_u8(const char* who, const int16_t* coef, int n, const JpegGeom& g, int restart, uint8_t* out, size_t slot_bytes,
                        uint32_t* lengths, int32_t* status, void* workspace, size_t workspace_bytes, uint32_t* d_rst_counters, hipStream_t s,
                        const TableSource& t = {}) {
    const JpegEncPlan p = plan_jpeg_encode(g, n, slot_bytes, restart, t.specs ? 1 : 0);
    TSTAR_REQUIRE(!p.error, std::string(who) + ": " + (p.error ? p.error : ""));
    TSTAR_REQUIRE((uintptr_t)workspace % 16 == 0 && workspace_bytes >= p.workspace_bytes,
                  std::string(who) + ": the workspace is misaligned or smaller than the plan's workspace_bytes");
    uint8_t* ws = (uint8_t*)workspace;
    EntropyArgs e;
    e.coef = coef;
    e.meta = (uint32_t*)(ws + p.off_meta);
    e.bits = (uint32_t*)(ws + p.off_bits);
    e.raw = (uint32_t*)(ws + p.off_raw);
    e.sg = scan_geom(g);
    e.blocks = (int)p.blocks;
    e.raw_words = (uint32_t)p.raw_words;
    StuffArgs a;
    a.raw = e.raw; a.meta = e.meta;
    a.ff = (uint32_t*)(ws + p.off_ff);
    a.out = out; a.lengths = lengths; a.status = status;
    a.raw_words = (uint32_t)p.raw_words; a.ff_chunks = (uint32_t)p.ff_chunks; a.slot_bytes = (uint32_t)slot_bytes;
    const bool scans = (t.stages & 4) != 0;
    // meta (flags) and the unstuffed stream start from zero: the stream is assembled by OR
    TSTAR_HIP_CHECK(hipMemsetAsync(e.meta, 0, (size_t)n * 4 * sizeof(uint32_t), s));
    if (scans) TSTAR_HIP_CHECK(hipMemsetAsync(e.raw, 0, (size_t)n * p.raw_words * sizeof(uint32_t), s));
    if (scans && d_rst_counters) TSTAR_HIP_CHECK(hipMemsetAsync(d_rst_counters, 0, (size_t)n * JPEG_ENC_R_COUNTERS * sizeof(uint32_t), s));
    if (t.specs && (t.stages & 3)) RC(launch_tables(p, n, e, restart, t.specs, ws, t.stages & 3, s, t.ga));
    if (!scans) return TSTAR_OK;
    if (t.ga && !(t.stages & 2)) {                         // the scans alone: the flags are those of the tables that were kept
        hipLaunchKernelGGL(jpeg_enc_group_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t.specs, *t.ga, e.meta, n);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    const jpegenc::HuffCodes* codes = (const jpegenc::HuffCodes*)(ws + p.off_codes);        // read with specs only
    auto launch = [&](auto rst, const auto& r) {
        constexpr bool RST = decltype(rst)::value;
        if (t.ga) return launch_scan<RST, TAB_GROUP>(p, n, e, a, r, {codes, *t.ga}, t.specs, s);
        if (t.specs) return launch_scan<RST, TAB_FRAME>(p, n, e, a, r, {codes, {}}, t.specs, s);
        return launch_scan<RST, TAB_STD>(p, n, e, a, r, {}, nullptr, s);
    };
    if (restart == 0) return launch(std::false_type{}, NoRestart{});
    RestartArgs r;
    r.seg = (uint32_t*)(ws + p.off_seg);
    r.mark = (uint32_t*)(ws + p.off_mark);
    r.counters = d_rst_counters;
    r.interval = restart;
    r.seg_blocks = restart * e.sg.per_mcu();           // at most 65535 * 6; at least the frame's blocks when there is no marker
    r.markers = (uint32_t)p.markers;
    return launch(std::true_type{}, r);
}

}  // namespace tstar

using namespace tstar;

extern "C" {

int tstar_jpeg_encode_blocks(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                             int16_t* d_coef, uint16_t* h_quant, void* stream) {
    TSTAR_REQUIRE(d_frames && d_idx && d_coef, "tstar_jpeg_encode_blocks: null argument");
    const JpegGeom g{W, H, 3, hs, vs};
    RC(jpeg_encode_blocks_u8(d_frames, N, H, W, d_idx, n, quality, g, d_coef, (hipStream_t)stream));
    if (h_quant) jpeg_enc_quant(quality, h_quant);
    return TSTAR_OK;
}

// the two entries without an interval forward to the _rst entries with interval 0 and no counters, as on the host side
int tstar_jpeg_encode_scan(const int16_t* d_coef, int n, int W, int H, int hs, int vs, uint8_t* d_out, size_t slot_bytes,
                           uint32_t* d_lengths, int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
    TSTAR_REQUIRE(d_coef && d_out && d_lengths && d_status && d_workspace, "tstar_jpeg_encode_scan: null argument");
    return tstar_jpeg_encode_scan_rst(d_coef, n, W, H, hs, vs, 0, d_out, slot_bytes, d_lengths, d_status, d_workspace, workspace_bytes, nullptr,
                                      stream);
}

int tstar_jpeg_encode(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                      int16_t* d_coef, uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths, int32_t* d_status, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
    TSTAR_REQUIRE(d_frames && d_idx && d_coef && d_out && d_lengths && d_status && d_workspace, "tstar_jpeg_encode: null argument");
    return tstar_jpeg_encode_rst(d_frames, N, H, W, d_idx, n, quality, hs, vs, 0, d_coef, d_out, slot_bytes, d_lengths, d_status, d_workspace,
                                 workspace_bytes, nullptr, stream);
}

int tstar_jpeg_encode_scan_rst(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* d_out, size_t slot_bytes,
                               uint32_t* d_lengths, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                               uint32_t* d_rst_counters, void* stream) {
    TSTAR_REQUIRE(d_coef && d_out && d_lengths && d_status && d_workspace, "tstar_jpeg_encode_scan_rst: null argument");
    return jpeg_encode_scan_u8("tstar_jpeg_encode_scan_rst", d_coef, n, JpegGeom{W, H, 3, hs, vs}, restart, d_out, slot_bytes, d_lengths, d_status,
                               d_workspace, workspace_bytes, d_rst_counters, (hipStream_t)stream);
}

int tstar_jpeg_encode_scan_opt(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* d_out, size_t slot_bytes,
                               uint32_t* d_lengths, int32_t* d_status, uint8_t* d_specs, void* d_workspace, size_t workspace_bytes,
                               uint32_t* d_rst_counters, void* stream) {
    TSTAR_REQUIRE(d_coef && d_out && d_lengths && d_status && d_specs && d_workspace, "tstar_jpeg_encode_scan_opt: null argument");
    return jpeg_encode_scan_u8("tstar_jpeg_encode_scan_opt", d_coef, n, JpegGeom{W, H, 3, hs, vs}, restart, d_out, slot_bytes, d_lengths, d_status,
                               d_workspace, workspace_bytes, d_rst_counters, (hipStream_t)stream, {(jpegenc::HuffSpecWide*)d_specs, nullptr, 7});
}

int tstar_jpeg_encode_tables(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, size_t slot_bytes, int stages,
                             uint8_t* d_specs, void* d_workspace, size_t workspace_bytes, void* stream) {
    TSTAR_REQUIRE(d_coef && d_specs && d_workspace && stages >= 1 && stages <= 3, "tstar_jpeg_encode_tables: null argument or stages outside 1..3");
    return jpeg_encode_scan_u8("tstar_jpeg_encode_tables", d_coef, n, JpegGeom{W, H, 3, hs, vs}, restart, nullptr, slot_bytes, nullptr, nullptr,
                               d_workspace, workspace_bytes, nullptr, (hipStream_t)stream, {(jpegenc::HuffSpecWide*)d_specs, nullptr, stages});
}

// Shared tables: frame f is coded with the four tables of group h_group[f] (d_group: the same array on the device; -1: the frame is
// not coded), built from the sum of the group's counts.  h_span / d_span: i32 [n_groups][2] from tstar_jpeg_encode_group_spans.  stages: 1 counts the frames' symbols and sums them per group into
// d_group_hist; 2 makes the groups' tables from d_group_hist as it is (d_specs, and the codes in the workspace); 4 codes the scans
// with the codes the workspace holds.  The workspace is tstar_jpeg_encode_plan_opt's (optimize 1) for these n and slot_bytes.
int tstar_jpeg_encode_scan_grp(const int16_t* d_coef, int n, int W, int H, int hs, int vs, int restart, const int32_t* h_group,
                               const int32_t* h_span, const int32_t* d_group, const int32_t* d_span, int n_groups, int stages, uint32_t* d_group_hist, uint8_t* d_specs,
                               uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths, int32_t* d_status, void* d_workspace,
                               size_t workspace_bytes, void* stream) {
    TSTAR_REQUIRE(d_coef && h_group && h_span && d_group && d_span && d_group_hist && d_specs && d_workspace && stages >= 1 && stages <= 7,
                  "tstar_jpeg_encode_scan_grp: null argument or stages outside 1..7");
    TSTAR_REQUIRE(!(stages & 4) || (d_out && d_lengths && d_status), "tstar_jpeg_encode_scan_grp: null argument");
    TSTAR_REQUIRE((uintptr_t)d_group % 4 == 0 && (uintptr_t)d_span % 4 == 0 && (uintptr_t)d_group_hist % 4 == 0,
                  "tstar_jpeg_encode_scan_grp: misaligned group arrays");
    const JpegGeom g{W, H, 3, hs, vs};
    const JpegEncPlan p = plan_jpeg_encode(g, n, slot_bytes, restart, 1);
    TSTAR_REQUIRE(!p.error, std::string("tstar_jpeg_encode_scan_grp: ") + (p.error ? p.error : ""));
    std::vector<int32_t> span((size_t)2 * (n_groups > 0 ? n_groups : 1));
    const char* bad = jpeg_enc_groups_check(h_group, n, n_groups, p.blocks, span.data());
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_encode_scan_grp: ") + (bad ? bad : ""));
    TSTAR_REQUIRE(memcmp(span.data(), h_span, span.size() * sizeof(int32_t)) == 0,
                  "tstar_jpeg_encode_scan_grp: the spans are not those of the groups (tstar_jpeg_encode_group_spans)");
    GroupArgs ga;
    ga.group = d_group; ga.span = d_span; ga.hist = d_group_hist; ga.n_groups = n_groups;
    return jpeg_encode_scan_u8("tstar_jpeg_encode_scan_grp", d_coef, n, g, restart, d_out, slot_bytes, d_lengths, d_status, d_workspace,
                               workspace_bytes, nullptr, (hipStream_t)stream, {(jpegenc::HuffSpecWide*)d_specs, &ga, stages});
}

int tstar_jpeg_encode_rst(const uint8_t* d_frames, int N, int H, int W, const int32_t* d_idx, int n, int quality, int hs, int vs,
                          int restart, int16_t* d_coef, uint8_t* d_out, size_t slot_bytes, uint32_t* d_lengths, int32_t* d_status,
                          void* d_workspace, size_t workspace_bytes, uint32_t* d_rst_counters, void* stream) {
    TSTAR_REQUIRE(d_frames && d_idx && d_coef && d_out && d_lengths && d_status && d_workspace, "tstar_jpeg_encode_rst: null argument");
    const JpegGeom g{W, H, 3, hs, vs};
    TSTAR_REQUIRE(jpeg_enc_restart_ok(restart), "tstar_jpeg_encode_rst: restart interval outside 0..65535 MCUs");
    RC(jpeg_encode_blocks_u8(d_frames, N, H, W, d_idx, n, quality, g, d_coef, (hipStream_t)stream));
    return jpeg_encode_scan_u8("tstar_jpeg_encode_rst", d_coef, n, g, restart, d_out, slot_bytes, d_lengths, d_status, d_workspace, workspace_bytes,
                               d_rst_counters, (hipStream_t)stream);
}

}  // extern "C"
