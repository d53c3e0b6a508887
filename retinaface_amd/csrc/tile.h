// tile.h -- the plan, edge rule and mapping of tiled detection, shared by the kernel (kernels.hip tile_gather_kernel) and the host
// entry points rf_tile_plan / rf_tile_map_face (capi.cpp).  A frame larger than the net is cut into net-sized tiles that overlap,
// every tile is detected at 1:1 (plus, optionally, the whole frame shrunk as one more pass), the faces of all passes are moved into
// source-frame pixels and merged by one more greedy NMS (DESIGN.md "Tiled detection").  Everything here is integer arithmetic or a
// single fp32 operation per coordinate, never contracted, so host and device agree bit for bit with each other and with
// tests/tile_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"

namespace rf {

constexpr int kTileDefaultEdge = 8;
constexpr int kTileMaxPasses = 1024;       // passes of one frame's plan (tiles + the full-frame pass)
constexpr int kTileMergeCap = 4096;        // surviving candidates per frame the merge holds (one workgroup's LDS, as launch_nms)
constexpr int kTileMaxFaces = 4096;
static_assert(sizeof(rf_tile_spec) == 20, "rf_tile_spec is 20 bytes");

// a validated rf_tile_spec with its defaults applied
struct TileSpec {
    int overlap = 0, edge = kTileDefaultEdge, full_frame = 1, max_faces = 0;
};

// One pass of a frame's plan as the gather kernel sees it: tile t of frame `frame` covers [x0, x0 + tw) x [y0, y0 + th) of a
// rows x cols frame; full != 0: the full-frame pass (coordinates are multiplied by `scale` instead).  frame < 0: nothing to gather.
struct TileEntry {
    int32_t frame, x0, y0, tw, th, rows, cols, t, full;
    float scale;
};

// Host: check a caller's spec against the net size and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is
// wrong with it.
inline const char *tile_spec_resolve(const rf_tile_spec *in, int net_h, int net_w, int default_max_faces, TileSpec *out) {
    if (net_h <= 0 || net_w <= 0) return "net size must be positive";
    const int nmin = net_h < net_w ? net_h : net_w;
    TileSpec r;
    r.overlap = nmin / 4;
    r.max_faces = default_max_faces;
    if (in) {
        if (in->struct_size != sizeof(rf_tile_spec)) return "rf_tile_spec.struct_size mismatch";
        if (in->overlap >= nmin) return "overlap must be smaller than min(net_h, net_w)";
        if (in->edge >= nmin / 2) return "edge must be smaller than min(net_h, net_w) / 2";      // a wider band would drop every face of an interior tile
        if (in->full_frame < 0 || in->full_frame > 2) return "full_frame must be 0, 1 or 2";
        if (in->max_faces < 0 || in->max_faces > kTileMaxFaces) return "max_faces must be 0 or in [1, 4096]";
        if (in->overlap) r.overlap = in->overlap < 0 ? 0 : in->overlap;
        if (in->edge) r.edge = in->edge < 0 ? 0 : in->edge;
        r.full_frame = in->full_frame != 2;
        if (in->max_faces) r.max_faces = in->max_faces;
    }
    if (r.max_faces < 1 || r.max_faces > kTileMaxFaces) return "max_faces must be in [1, 4096]";
    *out = r;
    return nullptr;
}

// one axis of the plan: length L, net size N, overlap ov (< N)
__host__ __device__ inline int tile_axis_count(int L, int N, int ov) { return L <= N ? 1 : (L - ov + (N - ov) - 1) / (N - ov); }
__host__ __device__ inline int tile_axis_origin(int L, int N, int n, int i) { return n <= 1 ? 0 : (int)((long long)i * (L - N) / (n - 1)); }
__host__ __device__ inline int tile_axis_size(int L, int N) { return L <= N ? L : N; }

// `scale` of the full-frame pass: rf_frame_scale (engine.h frame_scale computes the same float)
__host__ __device__ inline float tile_frame_scale(int rows, int cols, int net_h, int net_w) {
    const float sw = (float)cols / (float)net_w, sh = (float)rows / (float)net_h;
    const float sc = sw > sh ? sw : sh;
    return sc > 1.f ? sc : 1.f;
}

// The plan of a rows x cols frame (rows, cols >= 0): passes (tiles row-major, then the full-frame pass), -1 when there are more
// than kTileMaxPasses.  *nx / *ny: tiles per axis; *has_full: whether the full-frame pass exists.
inline int tile_plan_shape(const TileSpec &sp, int rows, int cols, int net_h, int net_w, int *nx, int *ny, int *has_full) {
    *nx = tile_axis_count(cols, net_w, sp.overlap);
    *ny = tile_axis_count(rows, net_h, sp.overlap);
    *has_full = sp.full_frame && (rows > net_h || cols > net_w);
    const long passes = (long)*nx * *ny + *has_full;
    return passes > kTileMaxPasses ? -1 : (int)passes;
}

// pass t of that plan (t < passes) as a table entry of frame `frame`
inline TileEntry tile_plan_entry(int rows, int cols, int net_h, int net_w, int nx, int ny, int t, int frame) {
    TileEntry e;
    memset(&e, 0, sizeof(e));
    e.frame = frame; e.rows = rows; e.cols = cols; e.t = t;
    e.scale = 1.f;
    if (t >= nx * ny) {
        e.full = 1; e.tw = cols; e.th = rows;
        e.scale = tile_frame_scale(rows, cols, net_h, net_w);
        return e;
    }
    e.x0 = tile_axis_origin(cols, net_w, nx, t % nx);
    e.y0 = tile_axis_origin(rows, net_h, ny, t / nx);
    e.tw = tile_axis_size(cols, net_w);
    e.th = tile_axis_size(rows, net_h);
    return e;
}

// Edge rule and mapping of one face of a pass.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]: the head of rf_face and of
// Candidate), they may alias.  Returns false when the edge rule drops the face (out is then untouched).
__host__ __device__ inline bool tile_map_face(const TileEntry &e, int edge, const float *in, float *out) {
#pragma clang fp contract(off)
    if (e.full) {
        out[0] = in[0];
        for (int i = 1; i < 15; i++) out[i] = in[i] * e.scale;
        return true;
    }
    const float x1 = in[1], y1 = in[2], x2 = in[3], y2 = in[4];
    if (e.x0 > 0 && x1 < (float)edge) return false;
    if (e.y0 > 0 && y1 < (float)edge) return false;
    if (e.x0 + e.tw < e.cols && x2 > (float)(e.tw - 1 - edge)) return false;
    if (e.y0 + e.th < e.rows && y2 > (float)(e.th - 1 - edge)) return false;
    const float fx = (float)e.x0, fy = (float)e.y0;
    out[0] = in[0];
    out[1] = x1 + fx; out[2] = y1 + fy; out[3] = x2 + fx; out[4] = y2 + fy;
    for (int i = 0; i < 5; i++) { out[5 + i] = in[5 + i] + fx; out[10 + i] = in[10 + i] + fy; }
    return true;
}

}  // namespace rf
