// redact.h -- face redaction, shared by the kernels (kernels.hip redact_*_kernel), the host entry points rf_redact_region /
// rf_redact_host (capi.cpp) and the engine.  A face's box grows by a margin and becomes an integer REGION; a region's MASK is its
// rectangle or the ellipse inscribed in it; PIXELATE replaces every pixel a region owns by the rounded mean of its CELL, FILL by a
// constant (DESIGN.md "Face redaction"); with RedactSpec::blur a PIXELATE region's pixels take the box-BLURRED frame instead (DESIGN.md
// "Blur redaction").  The floating-point part (redact_region_make) is fp32 with one rounding per operation (never
// contracted); everything after it is integer arithmetic, so host and device agree bit for bit with each other and with
// tests/redact_ref.py / tests/redact_blur_ref.py.  The host runs the pieces below in sequential loops (redact_host_frame); the kernels run the same pieces one
// thread per pixel or per span of bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/retinaface_amd.h"

namespace rf {

constexpr int kRedactMaxRegions = 1024;    // regions per image
constexpr int kRedactMaxCells = 64;        // cells across the longer side of a region
constexpr int kRedactMaxBlurRadius = 64;   // box radius of a blurred region, min(c, 64)
constexpr int kRedactMaxBlurPasses = 3;    // box passes per axis
static_assert(sizeof(rf_redact_spec) == 32, "rf_redact_spec is 32 bytes");

// a validated rf_redact_spec with its defaults applied
struct RedactSpec {
    int mode = RF_REDACT_PIXELATE, shape = RF_REDACT_RECT;
    int cells = 8;
    float margin = 0.2f;
    uint8_t fill[4] = {0, 0, 0, 0};        // B, G, R, unused
    int max_regions = 256;
    int coast = 0;                         // as the caller gave it: 0 = the tracker's max_missed, negative = none (redact_coast)
    int blur = 0;                          // 0 = cell means; 1..3 = box passes per axis of the blur (PIXELATE only)
};

// A region: the unclipped rectangle [ux0, ux1) x [uy0, uy1), its intersection with the frame [cx0, cx1) x [cy0, cy1) (empty when
// cx1 <= cx0 or cy1 <= cy0) and the cell edge c.  An invalid region is all zero: it owns no pixel.
struct RedactRegion { int32_t ux0, uy0, ux1, uy1, cx0, cy0, cx1, cy1, c, valid, pad_[2]; };
static_assert(sizeof(RedactRegion) == 48, "RedactRegion is 48 bytes");

__host__ __device__ inline bool redact_finite(float x) { return x == x && x - x == 0.f; }

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  default_regions: what max_regions 0 means (the engine's
// max_detections; clamped to 1024 here).  Returns nullptr, or what is wrong with it.
inline const char *redact_spec_resolve(const rf_redact_spec *in, int default_regions, RedactSpec *out) {
    RedactSpec r;
    r.max_regions = default_regions < 1 ? 1 : default_regions > kRedactMaxRegions ? kRedactMaxRegions : default_regions;
    if (in) {
        if (in->struct_size != sizeof(rf_redact_spec)) return "rf_redact_spec.struct_size mismatch";
        if (in->mode != RF_REDACT_PIXELATE && in->mode != RF_REDACT_FILL) return "mode must be RF_REDACT_PIXELATE or RF_REDACT_FILL";
        if (in->shape != RF_REDACT_RECT && in->shape != RF_REDACT_ELLIPSE) return "shape must be RF_REDACT_RECT or RF_REDACT_ELLIPSE";
        if (in->cells < 0 || in->cells > kRedactMaxCells) return "cells must be 0 or in [1, 64]";
        if (!redact_finite(in->margin) || in->margin > 1.f) return "margin must be finite and <= 1 (0 = 0.2, negative = 0)";
        if (in->max_regions < 0 || in->max_regions > kRedactMaxRegions) return "max_regions must be 0 or in [1, 1024]";
        if (in->blur > kRedactMaxBlurPasses) return "blur must be 0 (cell means) or 1, 2, 3 (box passes per axis)";
        if (in->blur && in->mode != RF_REDACT_PIXELATE) return "blur needs RF_REDACT_PIXELATE";
        r.mode = in->mode; r.shape = in->shape;
        if (in->cells) r.cells = in->cells;
        if (in->margin != 0.f) r.margin = in->margin < 0.f ? 0.f : in->margin;
        r.fill[0] = in->fill[0]; r.fill[1] = in->fill[1]; r.fill[2] = in->fill[2];
        if (in->max_regions) r.max_regions = in->max_regions;
        r.coast = in->coast;
        r.blur = in->blur;
    }
    *out = r;
    return nullptr;
}

// the largest `missed` of a live track that is still redacted (0: none), from the spec's coast and the tracker's max_missed
inline int redact_coast(int coast, int max_missed) { return coast == 0 ? max_missed : coast < 0 ? 0 : coast; }

__host__ __device__ inline float redact_clamp(float e) { return e < -4096.f ? -4096.f : e > 8192.f ? 8192.f : e; }

// The region of a box (x1, y1, x2, y2) in a rows x cols frame.  Steps 1-5 of the definition: scale (one multiply, a scale of 1
// included), validity, margin (one multiply and one add or subtract each), clamp and floor, clip.
//   The clamp to [-4096, 8192] bounds everything that follows: W, H <= 12289, so in the ellipse test |a| <= 2 W, |b| <= 2 H and each of
//   a*a*H*H, b*b*W*W, W*W*H*H is below 4 * 12289^4 < 2^57: their sums stay inside int64.  A cell's pixel set lies inside the frame,
//   which holds at most 4096 x 3072 = 12 582 912 pixels, so a channel sum is at most 255 * 12 582 912 < 2^32: a uint32 holds it.
//   A box whose width or height overflows fp32 (finite corners, infinite difference) is invalid like a non-finite corner.
__host__ __device__ inline RedactRegion redact_region_make(const float *box, float scale, float margin, int cells, int rows, int cols) {
#pragma clang fp contract(off)
    RedactRegion r;
    r.ux0 = r.uy0 = r.ux1 = r.uy1 = r.cx0 = r.cy0 = r.cx1 = r.cy1 = r.c = r.valid = 0;
    r.pad_[0] = r.pad_[1] = 0;
    const float bx1 = box[0] * scale, by1 = box[1] * scale, bx2 = box[2] * scale, by2 = box[3] * scale;
    const float w = bx2 - bx1, h = by2 - by1;
    if (!(redact_finite(bx1) && redact_finite(by1) && redact_finite(bx2) && redact_finite(by2))) return r;
    if (!(redact_finite(w) && redact_finite(h) && w >= 0.f && h >= 0.f)) return r;
    const float mw = margin * w, mh = margin * h;
    const float ex1 = redact_clamp(bx1 - mw), ex2 = redact_clamp(bx2 + mw);
    const float ey1 = redact_clamp(by1 - mh), ey2 = redact_clamp(by2 + mh);
    r.ux0 = (int)floorf(ex1); r.ux1 = (int)floorf(ex2) + 1;
    r.uy0 = (int)floorf(ey1); r.uy1 = (int)floorf(ey2) + 1;
    r.cx0 = r.ux0 > 0 ? r.ux0 : 0; r.cx1 = r.ux1 < cols ? r.ux1 : cols;
    r.cy0 = r.uy0 > 0 ? r.uy0 : 0; r.cy1 = r.uy1 < rows ? r.uy1 : rows;
    const int W = r.ux1 - r.ux0, H = r.uy1 - r.uy0;
    r.c = ((W > H ? W : H) + cells - 1) / cells;
    r.valid = 1;
    return r;
}

__host__ __device__ inline bool redact_clip_empty(const RedactRegion &r) { return !r.valid || r.cx1 <= r.cx0 || r.cy1 <= r.cy0; }

// whether the region's mask covers pixel (x, y); the ellipse is the one inscribed in the UNCLIPPED rectangle, at pixel centres, exact
__host__ __device__ inline bool redact_covers(const RedactRegion &r, int shape, int x, int y) {
    if (!r.valid || x < r.cx0 || x >= r.cx1 || y < r.cy0 || y >= r.cy1) return false;
    if (shape == RF_REDACT_RECT) return true;
    const long long W = r.ux1 - r.ux0, H = r.uy1 - r.uy0;
    const long long a = 2ll * x + 1 - ((long long)r.ux0 + r.ux1), b = 2ll * y + 1 - ((long long)r.uy0 + r.uy1);
    return a * a * H * H + b * b * W * W <= W * W * H * H;
}

// cells across / down the region's own grid (anchored at the unclipped corner)
__host__ __device__ inline int redact_cells_x(const RedactRegion &r) { return (r.ux1 - r.ux0 + r.c - 1) / r.c; }
__host__ __device__ inline int redact_cells_y(const RedactRegion &r) { return (r.uy1 - r.uy0 + r.c - 1) / r.c; }

// the pixel set of cell (gx, gy): its c x c square, cut by the unclipped rectangle and the frame: [x0, x1) x [y0, y1), maybe empty
__host__ __device__ inline void redact_cell_rect(const RedactRegion &r, int gx, int gy, int *x0, int *y0, int *x1, int *y1) {
    const int ax0 = r.ux0 + gx * r.c, ay0 = r.uy0 + gy * r.c;
    const int ax1 = ax0 + r.c, ay1 = ay0 + r.c;
    *x0 = ax0 > r.cx0 ? ax0 : r.cx0; *x1 = ax1 < r.cx1 ? ax1 : r.cx1;
    *y0 = ay0 > r.cy0 ? ay0 : r.cy0; *y1 = ay1 < r.cy1 ? ay1 : r.cy1;
}

// a cell's value from its channel sums and pixel count (n >= 1), packed B | G << 8 | R << 16
__host__ __device__ inline uint32_t redact_cell_value(uint32_t sb, uint32_t sg, uint32_t sr, uint32_t n) {
    const uint32_t h = n / 2;       // sum + h < 2^32: sum <= 255 n and n <= 12 582 912
    return ((sb + h) / n) | (((sg + h) / n) << 8) | (((sr + h) / n) << 16);
}

// ---- blur (RedactSpec::blur passes per axis).  A region's box radius; c >= 1 for every valid region, so rho >= 1.
__host__ __device__ inline int redact_blur_radius(const RedactRegion &r) { return r.c < kRedactMaxBlurRadius ? r.c : kRedactMaxBlurRadius; }
// the index a tap reads on an axis of length L >= 1: the border is replicated
__host__ __device__ inline int redact_blur_clamp(int i, int L) { return i < 0 ? 0 : i >= L ? L - 1 : i; }
// The rounded mean of the 2 rho + 1 taps of a pass.  sum <= 255 * 129 = 32 895, sum + rho <= 32 959 < 2^15: 16 bits hold every sum.
// The division is a multiplication by magic = redact_blur_magic(rho) = 2^24 / n + 1, n = 2 rho + 1 <= 129: with e = magic * n - 2^24
// (0 < e <= n) the product's quotient is exact while v * e < 2^24, and v * e <= 32 959 * 129 < 2^23.  (tests/csrc/test_redact_blur_host.cpp
// compares it with `/` for every rho and every v.)
__host__ __device__ inline uint32_t redact_blur_magic(int rho) { return (1u << 24) / (uint32_t)(2 * rho + 1) + 1u; }
__host__ __device__ inline uint32_t redact_blur_mean(uint32_t sum, int rho, uint32_t magic) { return ((sum + (uint32_t)rho) * magic) >> 24; }

// Host: one 1-D pass of radius rho over `count` lines of length L; element i of line k is at in[k * line + i * stride] (out likewise;
// out != in).  A running sum: O(1) per element.
inline void redact_blur_pass_host(const uint8_t *in, uint8_t *out, int count, size_t line, int L, size_t stride, int rho) {
    const uint32_t magic = redact_blur_magic(rho);
    for (int k = 0; k < count; k++) {
        const uint8_t *a = in + (size_t)k * line;
        uint8_t *o = out + (size_t)k * line;
        uint32_t s = 0;
        for (int d = -rho; d <= rho; d++) s += a[(size_t)redact_blur_clamp(d, L) * stride];
        for (int i = 0; i < L; i++) {
            o[(size_t)i * stride] = (uint8_t)redact_blur_mean(s, rho, magic);
            s += a[(size_t)redact_blur_clamp(i + rho + 1, L) * stride];
            s -= a[(size_t)redact_blur_clamp(i - rho, L) * stride];
        }
    }
}

// Host: B(orig, rho, passes) on the clipped rectangle of region r, dense (cx1 - cx0) * 3 bytes per row, into `out`.  A value depends on
// originals at most passes * rho away, so the window blurred is the rectangle grown by that halo and cut by the frame: a pass
// replicates the window's border, which is the frame's wherever the rectangle is nearer than the halo to it, and what a cut elsewhere
// spoils stays outside the rectangle (pass k spoils k * rho pixels from such a cut).
inline void redact_blur_host_region(const RedactRegion &r, int passes, const uint8_t *orig, int rows, int cols, size_t step,
                                    std::vector<uint8_t> &w0, std::vector<uint8_t> &w1, std::vector<uint8_t> &out) {
    const int rho = redact_blur_radius(r), halo = passes * rho;
    const int wx0 = r.cx0 - halo > 0 ? r.cx0 - halo : 0, wx1 = r.cx1 + halo < cols ? r.cx1 + halo : cols;
    const int wy0 = r.cy0 - halo > 0 ? r.cy0 - halo : 0, wy1 = r.cy1 + halo < rows ? r.cy1 + halo : rows;
    const int ww = wx1 - wx0, wh = wy1 - wy0;
    const size_t pitch = (size_t)ww * 3;
    w0.resize(pitch * wh); w1.resize(pitch * wh);
    for (int y = 0; y < wh; y++) memcpy(w0.data() + (size_t)y * pitch, orig + (size_t)(wy0 + y) * step + (size_t)3 * wx0, pitch);
    uint8_t *a = w0.data(), *b = w1.data();
    for (int p = 0; p < passes; p++) {                            // along x: 3 * wh lines (row, channel) of length ww
        for (int ch = 0; ch < 3; ch++) redact_blur_pass_host(a + ch, b + ch, wh, pitch, ww, 3, rho);
        uint8_t *t = a; a = b; b = t;
    }
    for (int p = 0; p < passes; p++) {                            // along y: 3 * ww lines (one per byte of a row) of length wh
        redact_blur_pass_host(a, b, (int)pitch, 1, wh, pitch, rho);
        uint8_t *t = a; a = b; b = t;
    }
    const size_t op = (size_t)(r.cx1 - r.cx0) * 3;
    out.resize(op * (r.cy1 - r.cy0));
    for (int y = r.cy0; y < r.cy1; y++) memcpy(out.data() + (size_t)(y - r.cy0) * op, a + (size_t)(y - wy0) * pitch + (size_t)3 * (r.cx0 - wx0), op);
}

// Host: a whole frame in place.  regions: the image's list, already cut at max_regions.  pixels: one count per region, or nullptr.
// Every read is of the original bytes: the cell values are formed before the first write, and a blur reads a copy of the frame made
// before the first write.
inline void redact_host_frame(const RedactSpec &sp, uint8_t *bgr, int rows, int cols, size_t step, const RedactRegion *regions, int nreg,
                              int32_t *pixels) {
    std::vector<std::vector<uint32_t>> value((size_t)nreg);
    const bool blur = sp.mode == RF_REDACT_PIXELATE && sp.blur > 0;
    std::vector<uint8_t> orig, w0, w1, blurred;
    if (blur && nreg > 0 && rows > 0 && cols > 0) {
        orig.resize((size_t)rows * cols * 3);
        for (int y = 0; y < rows; y++) memcpy(orig.data() + (size_t)y * cols * 3, bgr + (size_t)y * step, (size_t)cols * 3);
    }
    if (sp.mode == RF_REDACT_PIXELATE && !blur)
        for (int q = 0; q < nreg; q++) {
            const RedactRegion &r = regions[q];
            if (redact_clip_empty(r)) continue;
            const int gw = redact_cells_x(r), gh = redact_cells_y(r);
            value[q].assign((size_t)gw * gh, 0);
            for (int gy = 0; gy < gh; gy++)
                for (int gx = 0; gx < gw; gx++) {
                    int x0, y0, x1, y1;
                    redact_cell_rect(r, gx, gy, &x0, &y0, &x1, &y1);
                    if (x1 <= x0 || y1 <= y0) continue;
                    uint32_t s[3] = {0, 0, 0};
                    for (int y = y0; y < y1; y++) {
                        const uint8_t *p = bgr + (size_t)y * step + (size_t)3 * x0;
                        for (int x = x0; x < x1; x++, p += 3) { s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; }
                    }
                    value[q][(size_t)gy * gw + gx] = redact_cell_value(s[0], s[1], s[2], (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0));
                }
        }
    const uint32_t fill = (uint32_t)sp.fill[0] | ((uint32_t)sp.fill[1] << 8) | ((uint32_t)sp.fill[2] << 16);
    for (int q = 0; q < nreg; q++) {
        const RedactRegion &r = regions[q];
        int32_t owned = 0;
        if (!redact_clip_empty(r)) {
            const int gw = redact_cells_x(r);
            if (blur) redact_blur_host_region(r, sp.blur, orig.data(), rows, cols, (size_t)cols * 3, w0, w1, blurred);
            for (int y = r.cy0; y < r.cy1; y++)
                for (int x = r.cx0; x < r.cx1; x++) {
                    if (!redact_covers(r, sp.shape, x, y)) continue;
                    bool lower = false;
                    for (int o = 0; o < q && !lower; o++) lower = redact_covers(regions[o], sp.shape, x, y);
                    if (lower) continue;
                    uint32_t v;
                    if (blur) {
                        const uint8_t *b = blurred.data() + ((size_t)(y - r.cy0) * (r.cx1 - r.cx0) + (x - r.cx0)) * 3;
                        v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
                    } else {
                        v = sp.mode == RF_REDACT_FILL ? fill : value[q][(size_t)((y - r.uy0) / r.c) * gw + (x - r.ux0) / r.c];
                    }
                    uint8_t *p = bgr + (size_t)y * step + (size_t)3 * x;
                    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
                    owned++;
                }
        }
        if (pixels) pixels[q] = owned;
    }
}

}  // namespace rf
