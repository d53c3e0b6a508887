// roi.h -- region detection: the plan of a frame's regions, the atlas views they are packed into and the mapping of a view's faces back
// into the frame, shared by the kernels (kernels.hip roi_atlas_kernel / pass_gather_kernel<RoiMap>) and the host entry points
// rf_roi_plan / rf_roi_from_faces / rf_roi_map_face / rf_roi_atlas_host / rf_roi_merge_host (capi.cpp).  A caller names up to 256
// regions of a frame; a view of the net's size is cut into grid x grid cells, region r goes to cell r mod grid^2 of pass r / grid^2 and
// is shown there at the largest of five power-of-two steps (x4 .. x1/4) at which it fits, centred, with the real pixels around it;
// the faces of all passes are moved into source-frame pixels, each kept only by the region that holds its centre, and merged by the
// voting merge of tta.h (DESIGN.md "Region detection").  The pixels are integer arithmetic; the mapping is one fp32 add and at most
// one exact fp32 multiply and one fp32 add per coordinate, never contracted, so host and device agree bit for bit with each other
// and with tests/roi_ref.py.
//
// Tracked region detection (DESIGN.md "Tracked region detection"; tests/roi_track_ref.py): the regions of a frame are planned from a
// tracker's table, on the device by roi_track_cells_kernel and on the host by rf_roi_cells_from_tracks, both through roi_track_cell
// below.  Slot = region: region r of an image is slot r of the image's stream, so every image has roi_passes(max_tracks, grid) passes
// whatever the table holds, and neither the host nor the launch grid ever needs a count from the device.  A caller who wants one pass
// per frame creates the tracker with max_tracks <= grid^2.  A slot that yields no region (a free slot, a box roi_from_face refuses) gets
// the VOID record -- every field zero, flags = RF_ROI_VOID: its cell is zero pixels, addresses no source byte and drops every face.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "motion.h"
#include "pyramid.h"
#include "tta.h"

namespace rf {

static_assert(sizeof(rf_roi) == 16 && sizeof(rf_roi_cell) == 32 && sizeof(rf_roi_spec) == 24, "rf_roi 16, rf_roi_cell 32, rf_roi_spec 24 bytes");

constexpr int kRoiMaxRegions = RF_ROI_MAX_REGIONS;      // regions of one frame
constexpr int kRoiMaxSide = 16384, kRoiMaxOrigin = 1 << 20;
constexpr int kRoiMaxW = 4096, kRoiMaxH = 3072;          // a view, as for dewarped views

// a validated rf_roi_spec with its defaults applied
struct RoiSpec {
    int grid = 4, max_zoom = 2, vote = 0, max_faces = 0;
};

// A region in its cell: the region, its level (log2 of the step: 2, 1, 0, -1, -2), the cell's origin (x0, y0) in level pixels and
// RF_ROI_CROPPED.  The public record is the engine's.
using RoiCell = rf_roi_cell;

// One pass of a call as the gather kernel sees it: pass `pass` of frame `frame` (a rows x cols SOURCE frame), a net_w x net_h view of
// grid x grid cells of which the first `used` hold the regions pass * grid^2 .. + used - 1, whose records are `cells` (device memory
// for the kernels, host memory for the host entry points).  frame < 0: nothing to gather.
struct RoiEntry {
    int32_t frame, pass, rows, cols, grid, used, net_w, net_h;
    const RoiCell *cells;
};

// Host: a caller's spec, checked, with its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *roi_spec_resolve(const rf_roi_spec *in, int default_max_faces, RoiSpec *out) {
    RoiSpec r;
    r.max_faces = default_max_faces;
    if (in) {
        if (in->struct_size != sizeof(rf_roi_spec)) return "rf_roi_spec.struct_size mismatch";
        if (in->grid != 0 && in->grid != 1 && in->grid != 2 && in->grid != 4) return "grid must be 0, 1, 2 or 4";
        if (in->max_zoom != 0 && in->max_zoom != 1 && in->max_zoom != 2 && in->max_zoom != 4) return "max_zoom must be 0, 1, 2 or 4";
        if (in->vote < 0 || in->vote > 2) return "vote must be 0, 1 or 2";
        if (in->max_faces < 0 || in->max_faces > kTtaMaxFaces) return "max_faces must be 0 or in [1, 4096]";
        if (in->reserved != 0) return "reserved must be 0";
        if (in->grid) r.grid = in->grid;
        if (in->max_zoom) r.max_zoom = in->max_zoom;
        r.vote = in->vote == 1;
        if (in->max_faces) r.max_faces = in->max_faces;
    }
    if (r.max_faces < 1 || r.max_faces > kTtaMaxFaces) return "max_faces must be in [1, 4096]";
    *out = r;
    return nullptr;
}

// Host: the cell rule of a view.  Returns nullptr, or what is wrong.
inline const char *roi_check_view(int view_w, int view_h, int grid) {
    if (view_w < 4 || view_h < 1 || view_w > kRoiMaxW || view_h > kRoiMaxH) return "a view is at least 4 x 1 and at most 4096 x 3072 pixels";
    if (view_w % grid || view_h % grid || (view_w / grid) % 4) return "the view must divide into grid x grid cells whose width is a multiple of 4";
    return nullptr;
}

inline bool roi_valid(const rf_roi &r) {
    return r.w >= 1 && r.w <= kRoiMaxSide && r.h >= 1 && r.h <= kRoiMaxSide && r.x >= -kRoiMaxOrigin && r.x <= kRoiMaxOrigin &&
           r.y >= -kRoiMaxOrigin && r.y <= kRoiMaxOrigin;
}

// the smallest level among a view's cells (0 when none is below x1): what the atlas launch sizes its staging memory by
inline int roi_min_level(const RoiCell *cells, int used) {
    int m = 0;
    for (int k = 0; k < used; k++) m = cells[k].level < m ? cells[k].level : m;
    return m;
}

// the void record, and the region (four zeros) that stands for it where an entry point takes regions
__host__ __device__ inline RoiCell roi_void_cell() {
    RoiCell c;
    c.roi.x = c.roi.y = c.roi.w = c.roi.h = 0;
    c.level = c.x0 = c.y0 = 0;
    c.flags = RF_ROI_VOID;
    return c;
}
__host__ __device__ inline bool roi_cell_is_void(const RoiCell &c) { return (c.flags & RF_ROI_VOID) != 0; }
inline bool roi_is_void(const rf_roi &r) { return r.x == 0 && r.y == 0 && r.w == 0 && r.h == 0; }

inline int roi_passes(int regions, int grid) { return (regions + grid * grid - 1) / (grid * grid); }

__host__ __device__ inline int roi_floordiv(long long a, int b) {      // b > 0
    const long long q = a / b;
    return (int)(a % b < 0 ? q - 1 : q);
}

// ---- the plan
// The cell of one (valid) region in cells of cw x ch pixels: the largest step not above max_zoom at which it fits; none: x1/4, the cell
// shows the region's centre, RF_ROI_CROPPED.
__host__ __device__ inline RoiCell roi_plan(const rf_roi &r, int cw, int ch, int max_zoom) {
    RoiCell c;
    c.roi = r;
    c.flags = 0;
    int level = -3;
    for (int l = 2; l >= -2; l--) {
        if (l > 0 && (1 << l) > max_zoom) continue;
        const bool fits = l >= 0 ? ((long long)r.w << l) <= cw && ((long long)r.h << l) <= ch
                                 : r.w <= ((long long)cw << -l) && r.h <= ((long long)ch << -l);
        if (fits) { level = l; break; }
    }
    if (level == -3) { level = -2; c.flags = RF_ROI_CROPPED; }
    c.level = level;
    const long long cx2 = 2ll * r.x + r.w, cy2 = 2ll * r.y + r.h;          // twice the centre
    if (level >= 0) {
        c.x0 = roi_floordiv(cx2 * (1 << level) - cw, 2);
        c.y0 = roi_floordiv(cy2 * (1 << level) - ch, 2);
    } else {
        const int k = 1 << -level;
        c.x0 = roi_floordiv(cx2 - (long long)k * cw, 2 * k);
        c.y0 = roi_floordiv(cy2 - (long long)k * ch, 2 * k);
    }
    return c;
}

// ---- the pixel rule
// Pixel (X, Y) of the rows x cols BGR frame `src` (row pitch `step`) at `level`: x2 / x4 pyr_zoom_pixel (half-pixel centres, clamped
// at the border), x1 the frame, x1/2 / x1/4 the rounded mean of the k x k source block with source coordinates clamped into the frame
// (the level is ceil(cols / k) x ceil(rows / k)).  A pixel outside the level image is 0 and addresses nothing.
__host__ __device__ inline void roi_level_pixel(const uint8_t *src, int rows, int cols, size_t step, int level, int X, int Y, uint8_t *bgr) {
    bgr[0] = bgr[1] = bgr[2] = 0;
    if (X < 0 || Y < 0) return;
    if (level > 0) {
        if (X >= (cols << level) || Y >= (rows << level)) return;
        pyr_zoom_pixel(src, rows, cols, step, 1 << level, X, Y, bgr);
    } else if (level == 0) {
        if (X >= cols || Y >= rows) return;
        const uint8_t *p = src + (size_t)Y * step + (size_t)3 * X;
        bgr[0] = p[0]; bgr[1] = p[1]; bgr[2] = p[2];
    } else {
        const int s = -level, k = 1 << s;
        if (X >= (cols + k - 1) >> s || Y >= (rows + k - 1) >> s) return;
        int acc[3] = {0, 0, 0};
        for (int dy = 0; dy < k; dy++) {
            const int y = (Y << s) + dy < rows ? (Y << s) + dy : rows - 1;
            const uint8_t *row = src + (size_t)y * step;
            for (int dx = 0; dx < k; dx++) {
                const int x = (X << s) + dx < cols ? (X << s) + dx : cols - 1;
                acc[0] += row[3 * x]; acc[1] += row[3 * x + 1]; acc[2] += row[3 * x + 2];
            }
        }
        for (int c = 0; c < 3; c++) bgr[c] = (uint8_t)((acc[c] + (k * k >> 1)) >> (2 * s));
    }
}

// pixel (i, j) of a region's cell
__host__ __device__ inline void roi_cell_pixel(const uint8_t *src, int rows, int cols, size_t step, const RoiCell &c, int i, int j, uint8_t *bgr) {
    roi_level_pixel(src, rows, cols, step, c.level, c.x0 + i, c.y0 + j, bgr);
}

// Host: one view of view_w x view_h pixels (roi_check_view) whose first `used` cells are `cells`, written as view_w * 3 bytes per row
// at dst + y * dst_step; bytes beyond a row are untouched, the cells behind `used` and the void cells are zero.
inline void roi_atlas_host(const uint8_t *src, int rows, int cols, int step, const RoiCell *cells, int used, int grid, int view_w,
                           int view_h, uint8_t *dst, int dst_step) {
    const int cw = view_w / grid, ch = view_h / grid;
    for (int y = 0; y < view_h; y++) {
        uint8_t *d = dst + (size_t)y * dst_step;
        for (int x = 0; x < view_w; x++) {
            const int c = (y / ch) * grid + x / cw;
            if (c < used && !roi_cell_is_void(cells[c])) roi_cell_pixel(src, rows, cols, (size_t)step, cells[c], x % cw, y % ch, d + 3 * x);
            else d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = 0;
        }
    }
}

// ---- the face rule
// One face of a pass.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]), they may alias.  The face's cell is the one its box
// centre lies in (compares against the cell borders: a NaN lands in cell 0 and fails the last test); a cell without a region, or a
// void one, drops it.  Every coordinate: one fp32 add of the integer x0 - cell_x (y0 - cell_y), then for a zoom * (1 / z) - (z - 1) / 2z, for a shrink
// * k + (k - 1) / 2 (all constants exact).  Kept only when the mapped centre lies inside the region; *region: its index in the frame.
__host__ __device__ inline bool roi_map_face(const RoiEntry &e, const float *in, float *out, int *region) {
#pragma clang fp contract(off)
    const int cw = e.net_w / e.grid, ch = e.net_h / e.grid;
    const float cx = (in[1] + in[3]) * 0.5f, cy = (in[2] + in[4]) * 0.5f;
    int ci = 0, cj = 0;
    for (int k = 1; k < e.grid; k++) {
        ci += cx >= (float)(k * cw);
        cj += cy >= (float)(k * ch);
    }
    const int cell = cj * e.grid + ci;
    if (cell >= e.used) return false;
    const RoiCell c = e.cells[cell];
    if (roi_cell_is_void(c)) return false;
    const float ax = (float)(c.x0 - ci * cw), ay = (float)(c.y0 - cj * ch);
    float mul = 1.f, add = 0.f;
    switch (c.level) {
    case 2: mul = 0.25f; add = -0.375f; break;
    case 1: mul = 0.5f; add = -0.25f; break;
    case -1: mul = 2.f; add = 0.5f; break;
    case -2: mul = 4.f; add = 1.5f; break;
    default: break;
    }
    float o[15];
    o[0] = in[0];
    for (int i = 1; i < 15; i++) {
        const bool isx = i == 1 || i == 3 || (i >= 5 && i < 10);
        float v = in[i] + (isx ? ax : ay);
        if (c.level != 0) { v = v * mul; v = v + add; }
        o[i] = v;
    }
    const float mx = (o[1] + o[3]) * 0.5f, my = (o[2] + o[4]) * 0.5f;
    const float lx = (float)c.roi.x, hx = (float)(c.roi.x + c.roi.w), ly = (float)c.roi.y, hy = (float)(c.roi.y + c.roi.h);
    if (!(mx >= lx && mx < hx && my >= ly && my < hy)) return false;
    for (int i = 0; i < 15; i++) out[i] = o[i];
    *region = e.pass * e.grid * e.grid + cell;
    return true;
}

// ---- regions from faces
// The region of one face: the box times coord_scale (one fp32 multiply per coordinate), grown on every side by margin_q8 / 256 of
// its longer side (doubles), lower edges floored, upper edges ceiled, the sides held to [1, 16384].  False for a box that is not
// finite, is empty or starts beyond +-2^20.
__host__ __device__ inline bool roi_from_face(const float *face, float coord_scale, int margin_q8, rf_roi *out) {
#pragma clang fp contract(off)
    double b[4];
    for (int i = 0; i < 4; i++) {
        const float v = face[1 + i] * coord_scale;
        if (!(v >= -(float)kRoiMaxOrigin && v <= (float)kRoiMaxOrigin)) return false;      // a NaN fails both
        b[i] = (double)v;
    }
    if (!(b[2] >= b[0]) || !(b[3] >= b[1])) return false;
    const double sw = b[2] - b[0], sh = b[3] - b[1];
    const double side = sw > sh ? sw : sh;
    const double m = side * (double)margin_q8 / 256.0;
    const double x1 = floor(b[0] - m), y1 = floor(b[1] - m), x2 = ceil(b[2] + m), y2 = ceil(b[3] + m);
    if (x1 < -(double)kRoiMaxOrigin || y1 < -(double)kRoiMaxOrigin) return false;
    double w = x2 - x1, h = y2 - y1;
    w = w < 1 ? 1 : w > kRoiMaxSide ? kRoiMaxSide : w;
    h = h < 1 ? 1 : h > kRoiMaxSide ? kRoiMaxSide : h;
    out->x = (int32_t)x1; out->y = (int32_t)y1; out->w = (int32_t)w; out->h = (int32_t)h;
    return true;
}

// ---- regions from tracks
// The cell of one track slot: void for a free slot; otherwise the region of the box the next frame step matches against -- `last` for
// a plain tracker (m null), track_step_motion's pred[s] for one with motion -- grown by margin_q8 / 256 (0 = 64, as at the C ABI) at
// coord scale 1 (tracks live in source pixels), planned into a cell of cw x ch pixels; void when roi_from_face refuses the box.
__host__ __device__ inline RoiCell roi_track_cell(const rf_track &t, const rf_track_motion *m, const MotionSpec &ms, int margin_q8, int cw,
                                                  int ch, int max_zoom) {
    if (t.id == 0) return roi_void_cell();
    float f[5];
    f[0] = 0.f;
    const float last[4] = {t.last.x1, t.last.y1, t.last.x2, t.last.y2};
    if (m) motion_predict_box(last, m->vx, m->vy, m->samples, motion_frames_ahead(t.missed, 1, ms.horizon), f + 1);
    else { f[1] = last[0]; f[2] = last[1]; f[3] = last[2]; f[4] = last[3]; }
    rf_roi r;
    if (!roi_from_face(f, 1.f, margin_q8 ? margin_q8 : 64, &r)) return roi_void_cell();
    return roi_plan(r, cw, ch, max_zoom);
}

// Host: the cells of a stream's table (max_tracks slots; motion null: a plain tracker) -- the code roi_track_cells_kernel runs
inline void roi_cells_from_tracks(const rf_track *table, const rf_track_motion *motion, const MotionSpec &ms, int max_tracks, int margin_q8,
                                  int cw, int ch, int max_zoom, RoiCell *cells) {
    for (int s = 0; s < max_tracks; s++) cells[s] = roi_track_cell(table[s], motion ? motion + s : nullptr, ms, margin_q8, cw, ch, max_zoom);
}

}  // namespace rf
