// pyramid.h -- zoom-pyramid detection: the plan, the integer bilinear zoom and the mapping of a zoom pass back into the frame, shared
// by the kernels (kernels.hip zoom_tile_kernel / pyr_gather_kernel) and the host entry points rf_pyramid_plan / rf_pyramid_map_face /
// rf_pyramid_merge_host / rf_zoom_host (capi.cpp).  A frame is detected at 1x (the passes of its tile plan) and as net-sized tiles
// of the frame enlarged 2x and 4x, so that faces below the smallest anchor reach the net at a size it knows; the faces of all passes
// are moved into source-frame pixels and merged by the voting merge of tta.h (DESIGN.md "Zoom-pyramid detection").  The zoom is
// integer arithmetic; the mapping is tile_map_face followed by one exact fp32 multiply and one fp32 subtract per coordinate, never
// contracted, so host and device agree bit for bit with each other and with tests/pyramid_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/retinaface_amd.h"
#include "tile.h"
#include "tta.h"

namespace rf {

constexpr int kPyrMaxPasses = 1024;                 // passes of one frame's plan, all levels together
constexpr size_t kPyrMaxZoomBytes = (size_t)RF_PYRAMID_MAX_ZOOM_BYTES;      // zoom tiles of one call (256-byte-aligned each)
constexpr int kPyrLevels[3] = {1, 2, 4};            // bit b of rf_pyramid_spec.levels selects zoom kPyrLevels[b]
static_assert(sizeof(rf_pyramid_spec) == 28, "rf_pyramid_spec is 28 bytes");

// a validated rf_pyramid_spec with its defaults applied
struct PyrSpec {
    int levels = 3, vote = 1;
    TileSpec tile;                                  // overlap, edge, full_frame, max_faces
};

// One pass of a frame's plan as the gather kernel sees it: pass p of frame `frame` is the window [x0, x0 + tw) x [y0, y0 + th) of the
// frame enlarged z times, whose size is rows x cols (the VIRTUAL frame: z * the frame's); z = 1 && full != 0: the full-frame pass
// (coordinates are multiplied by `scale`).  frame < 0: nothing to gather.
struct PyrEntry {
    int32_t frame, z, x0, y0, tw, th, rows, cols, p, full;
    float scale;
};

// Host: check a caller's spec against the net size and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is
// wrong with it.
inline const char *pyr_spec_resolve(const rf_pyramid_spec *in, int net_h, int net_w, int default_max_faces, PyrSpec *out) {
    PyrSpec r;
    rf_tile_spec ts = {(uint32_t)sizeof(rf_tile_spec), 0, 0, 0, 0};
    if (in) {
        if (in->struct_size != sizeof(rf_pyramid_spec)) return "rf_pyramid_spec.struct_size mismatch";
        if (in->levels < 0 || in->levels > 7) return "levels must be 0 or in [1, 7]";
        if (in->vote < 0 || in->vote > 2) return "vote must be 0, 1 or 2";
        if (in->levels) r.levels = in->levels;
        r.vote = in->vote != 2;
        ts.overlap = in->overlap; ts.edge = in->edge; ts.full_frame = in->full_frame; ts.max_faces = in->max_faces;
    }
    if (const char *bad = tile_spec_resolve(&ts, net_h, net_w, default_max_faces, &r.tile)) return bad;
    *out = r;
    return nullptr;
}

// Host: the plan of a rows x cols frame (rows, cols > 0) appended to *out as entries of frame `frame`: the 1x passes of the tile plan
// (its full-frame pass included), then the tiles of the 2x and of the 4x virtual frame, row-major, without a full-frame pass.
// Returns the number of passes, or -1 when there are more than kPyrMaxPasses.  *zoom_bytes grows by the bytes the zoom tiles take
// as dense frames at 256-byte-aligned offsets.
inline int pyr_plan(const PyrSpec &sp, int rows, int cols, int net_h, int net_w, int frame, std::vector<PyrEntry> *out, size_t *zoom_bytes) {
    int passes = 0;
    for (int b = 0; b < 3; b++) {
        if (!(sp.levels >> b & 1)) continue;
        const int z = kPyrLevels[b], vr = rows * z, vc = cols * z;
        TileSpec ts = sp.tile;
        if (z > 1) ts.full_frame = 0;
        int nx = 0, ny = 0, full = 0;
        const int n = tile_plan_shape(ts, vr, vc, net_h, net_w, &nx, &ny, &full);
        if (n < 0 || passes + n > kPyrMaxPasses) return -1;
        for (int t = 0; t < n; t++) {
            const TileEntry te = tile_plan_entry(vr, vc, net_h, net_w, nx, ny, t, frame);
            PyrEntry e;
            e.frame = frame; e.z = z; e.x0 = te.x0; e.y0 = te.y0; e.tw = te.tw; e.th = te.th; e.rows = vr; e.cols = vc;
            e.p = passes + t; e.full = te.full; e.scale = te.scale;
            if (out) out->push_back(e);
            if (z > 1 && zoom_bytes) *zoom_bytes += ((size_t)te.tw * te.th * 3 + 255) / 256 * 256;
        }
        passes += n;
    }
    return passes;
}

// One axis of the zoom: output index X of an axis of source length n enlarged z times (2 or 4) lies at source coordinate
// (2X + 1 - z) / 2z (half-pixel centres).  *i0 / *i1: the two source indices, clamped to the axis; *w: the weight of i1 in units of
// 1 / D, D = 2z.
__host__ __device__ inline void pyr_zoom_axis(int X, int z, int n, int *i0, int *i1, int *w) {
    const int lg = z == 2 ? 2 : 3;                  // log2 D
    const int num = 2 * X + 1 - z;
    const int f = num >> lg;                        // floor(num / D): an arithmetic shift, also for num < 0
    *w = num - f * (1 << lg);                       // (a multiply: f is -1 at the first pixels, and shifting a negative left is undefined)
    *i0 = f < 0 ? 0 : f > n - 1 ? n - 1 : f;
    *i1 = f + 1 < 0 ? 0 : f + 1 > n - 1 ? n - 1 : f + 1;
}

// The per-pixel arithmetic of the zoom: pixel (X, Y) of the rows x cols BGR frame `src` (row pitch `step`) enlarged z times, three
// bytes.  Reads nothing outside the frame.
__host__ __device__ inline void pyr_zoom_pixel(const uint8_t *src, int rows, int cols, size_t step, int z, int X, int Y, uint8_t *bgr) {
    const int D = 2 * z, sh = z == 2 ? 4 : 6;       // 2 * log2 D
    int x0, x1, wx, y0, y1, wy;
    pyr_zoom_axis(X, z, cols, &x0, &x1, &wx);
    pyr_zoom_axis(Y, z, rows, &y0, &y1, &wy);
    const uint8_t *r0 = src + (size_t)y0 * step, *r1 = src + (size_t)y1 * step;
    for (int c = 0; c < 3; c++) {
        const int a = r0[3 * x0 + c], b = r0[3 * x1 + c], cc = r1[3 * x0 + c], d = r1[3 * x1 + c];
        const int acc = ((D - wx) * a + wx * b) * (D - wy) + ((D - wx) * cc + wx * d) * wy;
        bgr[c] = (uint8_t)((acc + D * D / 2) >> sh);
    }
}

// Edge rule and mapping of one face of a pass.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]), they may alias.  A 1x pass
// is tile_map_face; a zoom pass applies its edge rule in tile coordinates against the virtual frame, moves the face into the
// virtual frame and then into the source frame: v * (1 / z) - (z - 1) / 2z, the pixel-centre correspondence (both constants
// exact).  Returns false when the edge rule drops the face (out is then untouched).
__host__ __device__ inline bool pyr_map_face(const PyrEntry &e, int edge, const float *in, float *out) {
#pragma clang fp contract(off)
    TileEntry t;
    t.frame = e.frame; t.x0 = e.x0; t.y0 = e.y0; t.tw = e.tw; t.th = e.th; t.rows = e.rows; t.cols = e.cols; t.t = e.p; t.full = e.full;
    t.scale = e.scale;
    if (!tile_map_face(t, edge, in, out)) return false;
    if (e.z > 1) {
        const float inv = e.z == 2 ? 0.5f : 0.25f, off = e.z == 2 ? 0.25f : 0.375f;
        for (int i = 1; i < 15; i++) out[i] = out[i] * inv - off;
    }
    return true;
}

}  // namespace rf
