// Searcher ingest (ingest.hip): launchers and the launch plan (internal).
#pragma once
#include "common.h"

namespace tstar {

// OpenCV-style fixed-point bilinear resize (11-bit coefficients), gather by frame index.
// mode 0: frames[idx[i]] (H,W) -> out[i] (oh,ow)
int bilinear_gather_u8(const uint8_t* video, int H, int W, const int* d_idx, int n, int ow, int oh, uint8_t* out,
                       int nv12, hipStream_t s);
// frames[idx[i]] -> (4*ch x 4*cw) -> (ch x cw) -> tile (i / cols, i % cols) of grid [rows*ch, cols*cw, 3]
int frames_to_grid_u8(const uint8_t* video, int H, int W, const int* d_idx, int rows, int cols, int cw, int ch,
                      uint8_t* grid, int nv12, hipStream_t s);
// n planar I420 frames [H*3/2*W bytes each: Y, U, V planes] -> NV12 [n, H*3/2, W]
int i420_to_nv12_u8(const uint8_t* in, int n, int H, int W, uint8_t* out, hipStream_t s);
// frames[idx[i]] NV12 [H*3/2, W] -> RGB u8 [n,H,W,3] (BT.601 limited range, nearest chroma)
int nv12_to_rgb_u8(const uint8_t* video, int H, int W, const int* d_idx, int n, uint8_t* out, hipStream_t s);

// ---- which kernel form a launch gets (plan_ingest: the whole policy of the two launchers above)
enum IngestOp { INGEST_RESIZE = 0, INGEST_GRID = 1 };        // bilinear_gather_u8 / frames_to_grid_u8 (n = rows * cols, ow x oh = the cell)
enum IngestKind {
    INGEST_GENERIC = 0,     // one lane per pixel over all frames, plain tap tables; any shape, both formats
    INGEST_RGB_FAST = 1,    // fused tables, one frame per blockIdx.y; px pixels per lane
    INGEST_NV12_TAP = 2,    // the same for NV12 stores, every tap converted (px = 1 on the grid)
    INGEST_NV12_LDS = 3,    // resize only: an 8 x 128 output tile's source region converted once into LDS, px = 4
};
// the environment switches, read once by the launchers (ingest_overrides) and passed in
struct IngestOverrides {
    bool generic = false;   // TSTAR_INGEST_GENERIC=1: no RGB_FAST / NV12_TAP form (before / after counter runs)
    bool nv12_lds = true;   // TSTAR_NV12_LDS=0: no NV12_LDS form (same-session A/Bs)
    int grid_px = 1;        // TSTAR_GRID_PX=4: four pixels per lane in the RGB grid kernel where the cell allows it
};
struct IngestPlan {
    const char* error;      // non-null: the launcher refuses these arguments
    IngestKind kind;
    int px;                 // output pixels per lane (4 or 1)
    unsigned grid_x, grid_y;
    int lds_bytes, lds_pitch;   // NV12_LDS: dynamic LDS per block and its row pitch in dwords; else 0
};
// Pure: no HIP call, no global state; integers in, integers out (the NV12_LDS region size comes from the tap indices).
IngestPlan plan_ingest(int op, bool nv12, int H, int W, int n, int ow, int oh, bool out_aligned4, bool video_aligned4,
                       const IngestOverrides& o);

}  // namespace tstar
