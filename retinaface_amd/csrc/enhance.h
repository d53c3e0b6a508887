// enhance.h -- low-light enhancement: contrast-limited adaptive histogram equalisation of luma (CLAHE) over a grid of tiles, applied as a
// hue-preserving gain, shared by the kernels (kernels.hip enhance_lut_kernel / enhance_apply_kernel) and the host entry point
// rf_enhance_host (capi.cpp).  Every step is exact integer arithmetic in uint32 (DESIGN.md "Low-light detection" holds the definition,
// tests/enhance_ref.py restates it in numpy), so host, device and reference agree to the byte:
//      luma     Y = (77 R + 150 G + 29 B + 128) >> 8 of a BGR pixel
//      tiles    ceil(rows / T) x ceil(cols / T); tile (j, i) covers rows [jT, min((j + 1)T, rows)) and columns likewise, n >= 1 pixels
//      tile LUT h = the tile's luma histogram, c its inclusive prefix sum, p99 = the smallest v with 100 c[v] >= 99 n.
//               p99 >= dark_below: the tile is lit, LUT = identity, flag 0.  Otherwise flag 1 and
//               lim = max(1, (clip n) >> 16); ex = sum max(h[v] - lim, 0); h[v] = min(h[v], lim) + ex / 256 + (v < ex % 256);
//               LUT[v] = max(v, (2 * 255 * c[v] + n) / (2 n)) with c the prefix sum of the new h
//      pixel    per axis, D = 2T: p = 2y + 1 - T, q = floor(p / D), a0 = clamp(q, 0, nt - 1), a1 = clamp(q + 1, 0, nt - 1),
//               w = p < 0 ? 0 : p mod D (tile centres are the nominal ones, also for ragged edge tiles);
//               v = L[j0][i0][Y](D - wy)(D - wx) + L[j0][i1][Y](D - wy)wx + L[j1][i0][Y]wy(D - wx) + L[j1][i1][Y]wy wx,
//               Yn = (2v + D^2) / (2 D^2)
//      gain     Yn == Y: the three bytes are copied.  Otherwise c -> min(255, (2 c Yn + Yd) / (2 Yd)) with Yd = max(Y, 1).  The division
//               is a multiply-high by M = floor((2^32 - 1) / (2 Yd)) + 1 (enh_div_magic): exact for every numerator below 2^17
//               (tests/csrc/test_enhance_host.cpp enumerates the domain against the plain division).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/retinaface_amd.h"

namespace rf {

static_assert(sizeof(rf_enhance_spec) == 16, "rf_enhance_spec is 16 bytes");

constexpr int kEnhanceMaxTiles = 262144;        // tiles of one call: 64 MB of LUTs

// a validated rf_enhance_spec with its defaults applied
struct EnhanceSpec {
    int tile = 64, clip = 2048, dark_below = 64;
    int log2_tile() const { return tile == 16 ? 4 : tile == 32 ? 5 : tile == 64 ? 6 : 7; }
};

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *enhance_spec_resolve(const rf_enhance_spec *in, EnhanceSpec *out) {
    EnhanceSpec r;
    if (in) {
        if (in->struct_size != sizeof(rf_enhance_spec)) return "rf_enhance_spec.struct_size mismatch";
        if (in->tile != 0 && in->tile != 16 && in->tile != 32 && in->tile != 64 && in->tile != 128) return "tile must be 0, 16, 32, 64 or 128";
        if (in->clip != 0 && (in->clip < 256 || in->clip > 65535)) return "clip must be 0 or in [256, 65535]";
        if (in->dark_below < 0 || in->dark_below > 256) return "dark_below must be in [0, 256]";
        if (in->tile) r.tile = in->tile;
        if (in->clip) r.clip = in->clip;
        if (in->dark_below) r.dark_below = in->dark_below;
    }
    *out = r;
    return nullptr;
}

__host__ __device__ inline int enh_tiles(int extent, int log2_tile) { return (extent + (1 << log2_tile) - 1) >> log2_tile; }

__host__ __device__ inline uint32_t enh_luma(uint32_t b, uint32_t g, uint32_t r) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// one axis of the interpolation: the two tiles pixel y lies between and the weight of the second, of D = 2T
__host__ __device__ inline void enh_axis(int y, int log2_tile, int nt, int *a0, int *a1, int *w) {
    const int T = 1 << log2_tile, p = 2 * y + 1 - T;
    const int q = p >> (log2_tile + 1);                      // arithmetic shift: the floor towards minus infinity
    *a0 = q < 0 ? 0 : q > nt - 1 ? nt - 1 : q;
    *a1 = q + 1 < 0 ? 0 : q + 1 > nt - 1 ? nt - 1 : q + 1;
    *w = p < 0 ? 0 : p & (2 * T - 1);
}

// the four LUT values of a pixel, blended
__host__ __device__ inline uint32_t enh_blend(uint32_t l00, uint32_t l01, uint32_t l10, uint32_t l11, int wy, int wx, int log2_tile) {
    const uint32_t D = 2u << log2_tile, uy = (uint32_t)wy, ux = (uint32_t)wx;
    const uint32_t v = l00 * (D - uy) * (D - ux) + l01 * (D - uy) * ux + l10 * uy * (D - ux) + l11 * uy * ux;      // <= 255 D^2 < 2^24
    return (2u * v + D * D) >> (2 * log2_tile + 3);          // / (2 D^2), D^2 = 2^(2 log2_tile + 2)
}

// floor(num / den) == enh_div(num, enh_div_magic(den)) for den in [2, 510] and num < 2^17: M = 2^32 / den + e with 0 <= e <= 1, so
// num M / 2^32 exceeds num / den by less than 2^-15 < 1 / den and cannot reach the next integer
__host__ __device__ inline uint32_t enh_div_magic(uint32_t den) { return 0xffffffffu / den + 1u; }
__host__ __device__ inline uint32_t enh_div(uint32_t num, uint32_t magic) { return (uint32_t)(((uint64_t)num * magic) >> 32); }

// one channel through the gain Yn / Yd, magic = enh_div_magic(2 Yd)
__host__ __device__ inline uint32_t enh_gain(uint32_t c, uint32_t yn, uint32_t yd, uint32_t magic) {
    const uint32_t q = enh_div(2u * c * yn + yd, magic);
    return q > 255u ? 255u : q;
}

// the LUT of a tile of n pixels from its luma histogram h; returns the flag
inline int enh_tile_lut(const uint32_t *h, uint32_t n, const EnhanceSpec &sp, uint8_t *lut) {
    uint32_t c = 0;
    int p99 = 255;
    for (int v = 0; v < 256; v++) {
        c += h[v];
        if (100u * c >= 99u * n) { p99 = v; break; }
    }
    if (p99 >= sp.dark_below) {
        for (int v = 0; v < 256; v++) lut[v] = (uint8_t)v;
        return 0;
    }
    const uint32_t raw = ((uint32_t)sp.clip * n) >> 16, lim = raw < 1u ? 1u : raw;
    uint32_t ex = 0;
    for (int v = 0; v < 256; v++)
        if (h[v] > lim) ex += h[v] - lim;
    c = 0;
    for (int v = 0; v < 256; v++) {
        c += (h[v] < lim ? h[v] : lim) + ex / 256u + ((uint32_t)v < ex % 256u ? 1u : 0u);
        const uint32_t e = (2u * 255u * c + n) / (2u * n);
        lut[v] = (uint8_t)(e > (uint32_t)v ? e : (uint32_t)v);
    }
    return 1;
}

// Host: the enhancement of the rows x cols BGR frame src (row pitch step) written as cols * 3 bytes per row at dst + y * dst_step (bytes
// beyond them are untouched).  dst may be src with the same pitch: the LUTs are finished before a pixel is written.  Returns the number
// of flagged tiles.
inline int enhance_host(const EnhanceSpec &sp, const uint8_t *src, int rows, int cols, int step, uint8_t *dst, int dst_step) {
    const int lt = sp.log2_tile(), T = sp.tile, ny = enh_tiles(rows, lt), nx = enh_tiles(cols, lt);
    std::vector<uint8_t> luts((size_t)ny * nx * 256);
    int flagged = 0;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            uint32_t h[256];
            memset(h, 0, sizeof(h));
            const int y1 = (j + 1) * T < rows ? (j + 1) * T : rows, x1 = (i + 1) * T < cols ? (i + 1) * T : cols;
            for (int y = j * T; y < y1; y++) {
                const uint8_t *s = src + (size_t)y * step;
                for (int x = i * T; x < x1; x++) h[enh_luma(s[3 * x], s[3 * x + 1], s[3 * x + 2])]++;
            }
            flagged += enh_tile_lut(h, (uint32_t)(y1 - j * T) * (uint32_t)(x1 - i * T), sp, &luts[((size_t)j * nx + i) * 256]);
        }
    for (int y = 0; y < rows; y++) {
        int j0, j1, wy;
        enh_axis(y, lt, ny, &j0, &j1, &wy);
        const uint8_t *s = src + (size_t)y * step;
        uint8_t *d = dst + (size_t)y * dst_step;
        for (int x = 0; x < cols; x++) {
            int i0, i1, wx;
            enh_axis(x, lt, nx, &i0, &i1, &wx);
            const uint32_t b = s[3 * x], g = s[3 * x + 1], r = s[3 * x + 2], Y = enh_luma(b, g, r);
            const uint32_t yn = enh_blend(luts[((size_t)j0 * nx + i0) * 256 + Y], luts[((size_t)j0 * nx + i1) * 256 + Y],
                                          luts[((size_t)j1 * nx + i0) * 256 + Y], luts[((size_t)j1 * nx + i1) * 256 + Y], wy, wx, lt);
            if (yn == Y) { d[3 * x] = (uint8_t)b; d[3 * x + 1] = (uint8_t)g; d[3 * x + 2] = (uint8_t)r; continue; }
            const uint32_t yd = Y < 1u ? 1u : Y, m = enh_div_magic(2u * yd);
            d[3 * x] = (uint8_t)enh_gain(b, yn, yd, m); d[3 * x + 1] = (uint8_t)enh_gain(g, yn, yd, m); d[3 * x + 2] = (uint8_t)enh_gain(r, yn, yd, m);
        }
    }
    return flagged;
}

}  // namespace rf
