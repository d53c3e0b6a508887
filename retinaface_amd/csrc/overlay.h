// overlay.h -- boxes, landmarks and labels drawn into frames, shared by the kernels (kernels.hip overlay_*_kernel), the host entry
// points rf_overlay_region / rf_overlay_host (capi.cpp) and the engine.  A face becomes a REGION record: the floored box, five disc
// centres, a plate of digits and a colour; overlay_paint says which PRIMITIVE of a region covers a pixel; a pixel is painted by the
// lowest-indexed region that covers it, blended once against its original bytes (DESIGN.md "Overlays").  The floating-point part
// (overlay_region_make) is fp32 with one rounding per operation (never contracted); everything after it is integer arithmetic, so host
// and device agree bit for bit with each other and with tests/overlay_ref.py.  The host runs the pieces below in sequential loops
// (overlay_host_frame); the draw kernel runs the same pieces one thread per pixel of a primitive.
#pragma once
#include "redact.h"

namespace rf {

constexpr int kOverlayMaxThickness = 16, kOverlayMaxRadius = 16, kOverlayMaxFont = 8, kOverlayMaxDigits = 6;
static_assert(sizeof(rf_overlay_spec) == 40, "rf_overlay_spec is 40 bytes");

// a validated rf_overlay_spec with its defaults applied
struct OverlaySpec {
    int thickness = 2;
    int radius = 2;                        // negative: no discs
    int alpha = 255;
    int label = RF_OVERLAY_LABEL_NONE;
    int font = 2;
    int color_by_id = 0;
    uint32_t box = 0xff0000u, point = 0x00ff00u, text = 0xffffffu;      // B | G << 8 | R << 16
    int max_regions = 256;
    int coast = 0;                         // as RedactSpec::coast (redact_coast)
};

// A region.  (x0, y0, x1, y1): the floored box; (bx0 .. by1): the inclusive bounding rectangle of everything the region paints, not
// clipped; flags: kOverlayValid, kOverlayCoasting, bit 8 + k: point k has a disc; ndig digits, digit j in bits 4 j .. 4 j + 3 of
// `digits`; (plx, ply): the plate's top left pixel.  An invalid region is all zero: it paints nothing.
struct OverlayRegion {
    int32_t x0, y0, x1, y1, bx0, by0, bx1, by1;
    int32_t flags, ndig;
    uint32_t digits;
    int32_t plx, ply;
    uint32_t colour;
    int32_t cx[5], cy[5];
};
static_assert(sizeof(OverlayRegion) == 96, "OverlayRegion is 96 bytes");
enum { kOverlayValid = 1, kOverlayCoasting = 2, kOverlayDisc0 = 256 };
// what overlay_paint returns: 0 = nothing, else the primitive that wins at the pixel (glyph > plate > disc, lower k first > outline)
enum { kPaintNone = 0, kPaintOutline = 1, kPaintDisc = 2 /* + k, k = 0 .. 4 */, kPaintPlate = 7, kPaintGlyph = 8 };

inline uint32_t overlay_pack(const uint8_t *c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  default_regions as redact_spec_resolve.  Returns nullptr,
// or what is wrong with it.
inline const char *overlay_spec_resolve(const rf_overlay_spec *in, int default_regions, OverlaySpec *out) {
    OverlaySpec r;
    r.max_regions = default_regions < 1 ? 1 : default_regions > kRedactMaxRegions ? kRedactMaxRegions : default_regions;
    if (in) {
        if (in->struct_size != sizeof(rf_overlay_spec)) return "rf_overlay_spec.struct_size mismatch";
        if (in->thickness < 0 || in->thickness > kOverlayMaxThickness) return "thickness must be 0 or in [1, 16]";
        if (in->radius > kOverlayMaxRadius) return "radius must be <= 16 (0 = 2, negative = no landmarks)";
        if (in->colors_set > 1) return "colors_set must be 0 or 1";
        if (in->color_by_id > 1) return "color_by_id must be 0 or 1";
        if (in->label != RF_OVERLAY_LABEL_NONE && in->label != RF_OVERLAY_LABEL_SCORE && in->label != RF_OVERLAY_LABEL_ID)
            return "label must be RF_OVERLAY_LABEL_NONE, _SCORE or _ID";
        if (in->font_scale < 0 || in->font_scale > kOverlayMaxFont) return "font_scale must be 0 or in [1, 8]";
        if (in->max_regions < 0 || in->max_regions > kRedactMaxRegions) return "max_regions must be 0 or in [1, 1024]";
        if (in->thickness) r.thickness = in->thickness;
        if (in->radius) r.radius = in->radius < 0 ? -1 : in->radius;
        if (in->alpha) r.alpha = in->alpha;
        r.label = in->label;
        if (in->font_scale) r.font = in->font_scale;
        r.color_by_id = in->color_by_id;
        const uint32_t b = overlay_pack(in->box), p = overlay_pack(in->point), t = overlay_pack(in->text);
        if (in->colors_set || b) r.box = b;
        if (in->colors_set || p) r.point = p;
        if (in->colors_set || t) r.text = t;
        if (in->max_regions) r.max_regions = in->max_regions;
        r.coast = in->coast;
    }
    *out = r;
    return nullptr;
}

// palette[id & 7], B | G << 8 | R << 16
__host__ __device__ inline uint32_t overlay_palette(int k) {
    switch (k & 7) {
        case 0: return 0xff0000u;
        case 1: return 0x00ff00u;
        case 2: return 0x0000ffu;
        case 3: return 0xffff00u;
        case 4: return 0xff00ffu;
        case 5: return 0x00ffffu;
        case 6: return 0xff8000u;
        default: return 0x0080ffu;
    }
}

// row gy (0 = top) of digit d's 5 x 7 glyph, bit 4 = the leftmost column
__host__ __device__ inline uint32_t overlay_glyph_row(int d, int gy) {
    // seven 5-bit rows per digit, row 0 in the low bits
    const unsigned long long g[10] = {
        0x0Eull | 0x11ull << 5 | 0x13ull << 10 | 0x15ull << 15 | 0x19ull << 20 | 0x11ull << 25 | 0x0Eull << 30,
        0x04ull | 0x0Cull << 5 | 0x04ull << 10 | 0x04ull << 15 | 0x04ull << 20 | 0x04ull << 25 | 0x0Eull << 30,
        0x0Eull | 0x11ull << 5 | 0x01ull << 10 | 0x02ull << 15 | 0x04ull << 20 | 0x08ull << 25 | 0x1Full << 30,
        0x1Full | 0x02ull << 5 | 0x04ull << 10 | 0x02ull << 15 | 0x01ull << 20 | 0x11ull << 25 | 0x0Eull << 30,
        0x02ull | 0x06ull << 5 | 0x0Aull << 10 | 0x12ull << 15 | 0x1Full << 20 | 0x02ull << 25 | 0x02ull << 30,
        0x1Full | 0x10ull << 5 | 0x1Eull << 10 | 0x01ull << 15 | 0x01ull << 20 | 0x11ull << 25 | 0x0Eull << 30,
        0x06ull | 0x08ull << 5 | 0x10ull << 10 | 0x1Eull << 15 | 0x11ull << 20 | 0x11ull << 25 | 0x0Eull << 30,
        0x1Full | 0x01ull << 5 | 0x02ull << 10 | 0x04ull << 15 | 0x08ull << 20 | 0x08ull << 25 | 0x08ull << 30,
        0x0Eull | 0x11ull << 5 | 0x11ull << 10 | 0x0Eull << 15 | 0x11ull << 20 | 0x11ull << 25 | 0x0Eull << 30,
        0x0Eull | 0x11ull << 5 | 0x11ull << 10 | 0x0Full << 15 | 0x01ull << 20 | 0x02ull << 25 | 0x0Cull << 30,
    };
    return (uint32_t)(g[d] >> (5 * gy)) & 31u;
}

__host__ __device__ inline int overlay_plate_w(const OverlaySpec &sp, int ndig) { return sp.font + 6 * sp.font * ndig; }
__host__ __device__ inline int overlay_plate_h(const OverlaySpec &sp) { return 9 * sp.font; }

// The region of a face (15 floats: score, box, px[5], py[5]) with track id `id` (0: none).  coasting: a track drawn where it coasts: no
// discs, a dashed outline.  The clamp to [-4096, 8192] bounds everything that follows: with o <= 8, a plate at most 72 rows tall and
// 296 pixels wide and r <= 16 every coordinate of the record lies within [-4200, 8500], and a squared disc distance below 2^28.
__host__ __device__ inline OverlayRegion overlay_region_make(const OverlaySpec &sp, const float *face, long long id, float scale, bool coasting) {
#pragma clang fp contract(off)
    OverlayRegion r;
    r.x0 = r.y0 = r.x1 = r.y1 = r.bx0 = r.by0 = r.bx1 = r.by1 = r.flags = r.ndig = r.plx = r.ply = 0;
    r.digits = 0; r.colour = 0;
    for (int k = 0; k < 5; k++) r.cx[k] = r.cy[k] = 0;
    const float bx1 = face[1] * scale, by1 = face[2] * scale, bx2 = face[3] * scale, by2 = face[4] * scale;
    const float w = bx2 - bx1, h = by2 - by1;
    if (!(redact_finite(bx1) && redact_finite(by1) && redact_finite(bx2) && redact_finite(by2))) return r;
    if (!(redact_finite(w) && redact_finite(h) && w >= 0.f && h >= 0.f)) return r;
    r.x0 = (int)floorf(redact_clamp(bx1)); r.y0 = (int)floorf(redact_clamp(by1));
    r.x1 = (int)floorf(redact_clamp(bx2)); r.y1 = (int)floorf(redact_clamp(by2));
    r.flags = kOverlayValid | (coasting ? kOverlayCoasting : 0);
    const int o = sp.thickness / 2;
    r.bx0 = r.x0 - o; r.by0 = r.y0 - o; r.bx1 = r.x1 + o; r.by1 = r.y1 + o;
    r.colour = sp.color_by_id && id > 0 ? overlay_palette((int)(id & 7)) : sp.box;
    if (!coasting && sp.radius >= 0)
        for (int k = 0; k < 5; k++) {
            const float px = face[5 + k] * scale, py = face[10 + k] * scale;
            if (!(redact_finite(px) && redact_finite(py))) continue;
            r.cx[k] = (int)floorf(redact_clamp(px)); r.cy[k] = (int)floorf(redact_clamp(py));
            r.flags |= kOverlayDisc0 << k;
            if (r.cx[k] - sp.radius < r.bx0) r.bx0 = r.cx[k] - sp.radius;
            if (r.cx[k] + sp.radius > r.bx1) r.bx1 = r.cx[k] + sp.radius;
            if (r.cy[k] - sp.radius < r.by0) r.by0 = r.cy[k] - sp.radius;
            if (r.cy[k] + sp.radius > r.by1) r.by1 = r.cy[k] + sp.radius;
        }
    if (sp.label == RF_OVERLAY_LABEL_SCORE) {
        const float p = face[0] * 100.f;
        const int v = !(p == p) || p <= 0.f ? 0 : p >= 99.f ? 99 : (int)p;
        r.ndig = 2; r.digits = (uint32_t)(v / 10) | ((uint32_t)(v % 10) << 4);
    } else if (sp.label == RF_OVERLAY_LABEL_ID && id > 0) {
        int v = (int)(id % 1000000), n = 1;
        for (int q = v; q >= 10; q /= 10) n++;
        r.ndig = n;
        for (int j = n - 1; j >= 0; j--, v /= 10) r.digits |= (uint32_t)(v % 10) << (4 * j);
    }
    if (r.ndig) {
        const int top = r.y0 - o - overlay_plate_h(sp);
        r.plx = r.x0 - o; r.ply = top < 0 ? r.y0 - o : top;
        const int px1 = r.plx + overlay_plate_w(sp, r.ndig) - 1, py1 = r.ply + overlay_plate_h(sp) - 1;
        if (r.ply < r.by0) r.by0 = r.ply;
        if (px1 > r.bx1) r.bx1 = px1;
        if (py1 > r.by1) r.by1 = py1;
    }
    return r;
}

// Which primitive of the region covers pixel (x, y) (any integers; the frame clips elsewhere): kPaintNone, or the highest-priority one.
__host__ __device__ inline int overlay_paint(const OverlaySpec &sp, const OverlayRegion &r, int x, int y) {
    if (!(r.flags & kOverlayValid) || x < r.bx0 || x > r.bx1 || y < r.by0 || y > r.by1) return kPaintNone;
    if (r.ndig) {
        const int u = x - r.plx, v = y - r.ply, f = sp.font;
        if (u >= 0 && v >= 0 && u < overlay_plate_w(sp, r.ndig) && v < overlay_plate_h(sp)) {
            const int uu = u - f, vv = v - f;
            if (uu >= 0 && vv >= 0 && vv < 7 * f) {
                const int j = uu / (6 * f), gx = (uu - j * 6 * f) / f, gy = vv / f;
                if (gx < 5 && ((overlay_glyph_row((int)(r.digits >> (4 * j)) & 15, gy) >> (4 - gx)) & 1u)) return kPaintGlyph;
            }
            return kPaintPlate;
        }
    }
    const int rad = sp.radius;
    for (int k = 0; k < 5; k++) {
        if (!(r.flags & (kOverlayDisc0 << k))) continue;
        const int dx = x - r.cx[k], dy = y - r.cy[k];
        if (dx >= -rad && dx <= rad && dy >= -rad && dy <= rad && dx * dx + dy * dy <= rad * rad) return kPaintDisc + k;
    }
    const int t = sp.thickness, o = t / 2;
    const int ox0 = r.x0 - o, oy0 = r.y0 - o, ox1 = r.x1 + o, oy1 = r.y1 + o;
    if (x < ox0 || x > ox1 || y < oy0 || y > oy1) return kPaintNone;
    if (x >= ox0 + t && x <= ox1 - t && y >= oy0 + t && y <= oy1 - t) return kPaintNone;
    if ((r.flags & kOverlayCoasting) && ((((x - ox0) + (y - oy0)) / (2 * t)) & 1)) return kPaintNone;
    return kPaintOutline;
}

// the colour primitive `code` of region r paints with
__host__ __device__ inline uint32_t overlay_colour(const OverlaySpec &sp, const OverlayRegion &r, int code) {
    return code == kPaintGlyph ? sp.text : code >= kPaintDisc && code < kPaintPlate ? sp.point : r.colour;
}

// one byte blended: (orig * (255 - a) + colour * a + 127) / 255; the sum is below 2^16
__host__ __device__ inline uint8_t overlay_blend(uint32_t orig, uint32_t colour, int a) {
    return (uint8_t)((orig * (uint32_t)(255 - a) + colour * (uint32_t)a + 127u) / 255u);
}
__host__ __device__ inline void overlay_put(uint8_t *p, uint32_t colour, int a) {
    p[0] = overlay_blend(p[0], colour & 255u, a);
    p[1] = overlay_blend(p[1], (colour >> 8) & 255u, a);
    p[2] = overlay_blend(p[2], colour >> 16, a);
}

// The PIECES of a region, the rectangles the draw kernel deals out: 0 top, 1 bottom, 2 left and 3 right strip of the outline (disjoint,
// together all of O minus the inner rectangle), 4 + k the square around disc k, 9 the plate.  Inclusive, unclipped; x1 < x0 or y1 < y0:
// the region has no such piece.  The piece of a painted pixel is the one that holds the primitive overlay_paint names for it.
constexpr int kOverlayPieces = 10;
__host__ __device__ inline void overlay_piece_rect(const OverlaySpec &sp, const OverlayRegion &r, int piece, int *x0, int *y0, int *x1, int *y1) {
    *x0 = *y0 = 0; *x1 = *y1 = -1;
    if (!(r.flags & kOverlayValid)) return;
    const int t = sp.thickness, o = t / 2;
    const int ox0 = r.x0 - o, oy0 = r.y0 - o, ox1 = r.x1 + o, oy1 = r.y1 + o;
    if (piece == 0) { *x0 = ox0; *x1 = ox1; *y0 = oy0; *y1 = oy0 + t - 1 < oy1 ? oy0 + t - 1 : oy1; }
    else if (piece == 1) { *x0 = ox0; *x1 = ox1; *y0 = oy1 - t + 1 > oy0 + t ? oy1 - t + 1 : oy0 + t; *y1 = oy1; }
    else if (piece == 2) { *x0 = ox0; *x1 = ox0 + t - 1 < ox1 ? ox0 + t - 1 : ox1; *y0 = oy0 + t; *y1 = oy1 - t; }
    else if (piece == 3) { *x0 = ox1 - t + 1 > ox0 + t ? ox1 - t + 1 : ox0 + t; *x1 = ox1; *y0 = oy0 + t; *y1 = oy1 - t; }
    else if (piece < 9) {
        const int k = piece - 4;
        if (!(r.flags & (kOverlayDisc0 << k))) return;
        *x0 = r.cx[k] - sp.radius; *x1 = r.cx[k] + sp.radius; *y0 = r.cy[k] - sp.radius; *y1 = r.cy[k] + sp.radius;
    } else if (r.ndig) {
        *x0 = r.plx; *x1 = r.plx + overlay_plate_w(sp, r.ndig) - 1; *y0 = r.ply; *y1 = r.ply + overlay_plate_h(sp) - 1;
    }
}
// whether primitive `code` belongs to `piece` (an outline pixel lies in exactly one strip: the strips are disjoint)
__host__ __device__ inline bool overlay_piece_holds(int piece, int code) {
    return piece < 4 ? code == kPaintOutline : piece < 9 ? code == kPaintDisc + (piece - 4) : code >= kPaintPlate;
}

// Host: a whole frame in place.  regions: the image's list, already cut at max_regions.  pixels: one count per region, or nullptr.
// A painted pixel is written once and its value depends on its own original bytes alone, so no copy of the frame is needed.
inline void overlay_host_frame(const OverlaySpec &sp, uint8_t *bgr, int rows, int cols, size_t step, const OverlayRegion *regions, int nreg,
                               int32_t *pixels) {
    for (int q = 0; q < nreg; q++) {
        const OverlayRegion &r = regions[q];
        int32_t painted = 0;
        if (r.flags & kOverlayValid) {
            const int x0 = r.bx0 > 0 ? r.bx0 : 0, x1 = r.bx1 < cols - 1 ? r.bx1 : cols - 1;
            const int y0 = r.by0 > 0 ? r.by0 : 0, y1 = r.by1 < rows - 1 ? r.by1 : rows - 1;
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) {
                    const int code = overlay_paint(sp, r, x, y);
                    if (!code) continue;
                    bool lower = false;
                    for (int o = 0; o < q && !lower; o++) lower = overlay_paint(sp, regions[o], x, y) != kPaintNone;
                    if (lower) continue;
                    overlay_put(bgr + (size_t)y * step + (size_t)3 * x, overlay_colour(sp, r, code), sp.alpha);
                    painted++;
                }
        }
        if (pixels) pixels[q] = painted;
    }
}

}  // namespace rf
