// change.h -- change regions: the blocks of a frame that differ from a per-stream reference image, the 8-connected components of those
// blocks and the regions (roi.h) they turn into, shared by the kernels (kernels.hip change_blocks_kernel / change_regions_kernel) and
// the host entry point rf_change_step_host (capi.cpp).  DESIGN.md "Change regions" holds the definition, tests/change_ref.py restates
// it in numpy.  Everything up to the regions is integer arithmetic, so host, device and reference agree byte for byte.
//
// The block value is S = sum of 29 b + 150 g + 77 r over the block's pixels inside the frame: 256 x luma WITHOUT the per-pixel rounding
// of face_luma (quality.h), whose (.. + 128) >> 8 would cost an unpack per pixel; the sum over packed BGR bytes is three 4-byte dot
// products per twelve bytes with rotated weight words (change_weights) and no unpacking.  S fits 32 bits: 65280 * 1024 < 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "roi.h"

namespace rf {

static_assert(sizeof(rf_change_spec) == 32 && sizeof(rf_change_info) == 16, "rf_change_spec 32, rf_change_info 16 bytes");

constexpr int kChangeMaxBlocks = 16384;       // bw * bh of a changer
constexpr int kChangeMaxRegions = 64;
constexpr int kChangeMaxStreams = 1024;
constexpr int kChangeNone = 0xffff;           // the label of an unmarked block

// a validated rf_change_spec with its defaults applied
struct ChangeSpec {
    int block = 16, log2_block = 4, thr_q4 = 128, adapt_shift = 0, dilate = 1, min_blocks = 2, max_regions = 16;
};

// Host: a caller's spec, checked, with its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *change_spec_resolve(const rf_change_spec *in, ChangeSpec *out) {
    ChangeSpec r;
    if (in) {
        if (in->struct_size != sizeof(rf_change_spec)) return "rf_change_spec.struct_size mismatch";
        if (in->block != 0 && in->block != 8 && in->block != 16 && in->block != 32) return "block must be 0, 8, 16 or 32";
        if (in->thr_q4 < 0 || in->thr_q4 > 65535) return "thr_q4 must be in [1, 65535] (0 = 128)";
        if (in->adapt_shift < 0 || in->adapt_shift > 8) return "adapt_shift must be in [0, 8]";
        if (in->dilate < 0 || in->dilate > 2) return "dilate must be 0, 1 or 2";
        if (in->min_blocks < 0 || in->min_blocks > 65535) return "min_blocks must be in [1, 65535] (0 = 2)";
        if (in->max_regions < 0 || in->max_regions > kChangeMaxRegions) return "max_regions must be in [1, 64] (0 = 16)";
        if (in->reserved != 0) return "reserved must be 0";
        if (in->block) r.block = in->block;
        if (in->thr_q4) r.thr_q4 = in->thr_q4;
        r.adapt_shift = in->adapt_shift;
        r.dilate = in->dilate != 2;
        if (in->min_blocks) r.min_blocks = in->min_blocks;
        if (in->max_regions) r.max_regions = in->max_regions;
    }
    r.log2_block = r.block == 8 ? 3 : r.block == 16 ? 4 : 5;
    *out = r;
    return nullptr;
}

// Host: the block grid of a rows x cols frame.  Returns nullptr, or what is wrong.
inline const char *change_check_shape(int rows, int cols, const ChangeSpec &sp, int *bw, int *bh) {
    if (rows <= 0 || cols <= 0 || rows > 4096 * 3072 / cols) return "rows x cols must be in (0, 4096x3072]";
    const long long w = (cols + sp.block - 1) >> sp.log2_block, h = (rows + sp.block - 1) >> sp.log2_block;
    if (w * h > kChangeMaxBlocks) return "the block grid must not exceed 16384 blocks";
    *bw = (int)w; *bh = (int)h;
    return nullptr;
}

// ---- the block sum
// the weight word of a dword whose first byte is channel `phase` (0 = b, 1 = g, 2 = r) of its pixel
__host__ __device__ inline uint32_t change_weights(int phase) {
    return phase == 0 ? 0x1d4d961du : phase == 1 ? 0x961d4d96u : 0x4d961d4du;      // 29, 150, 77 rotated
}
// acc + the four byte products of a and b
__host__ __device__ inline uint32_t change_dot4(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int k = 0; k < 4; k++) acc += ((a >> (8 * k)) & 0xffu) * ((b >> (8 * k)) & 0xffu);
    return acc;
#endif
}
// the weighted sum of n packed bytes whose first is channel `phase`: dwords through change_dot4, the last n mod 4 bytes one by one
inline uint32_t change_bytes_sum(const uint8_t *p, int n, int phase) {
    uint32_t acc = 0;
    int k = 0;
    for (; k + 4 <= n; k += 4) {
        uint32_t w;
        memcpy(&w, p + k, 4);
        acc = change_dot4(w, change_weights((phase + k) % 3), acc);
    }
    for (; k < n; k++) acc += p[k] * (change_weights((phase + k) % 3) & 0xffu);
    return acc;
}
// Host: S of block (bx, by) of the rows x cols BGR frame `src` (row pitch `step`); *npix: its pixels inside the frame
inline uint32_t change_block_sum(const uint8_t *src, int rows, int cols, size_t step, int B, int bx, int by, int *npix) {
    const int x0 = bx * B, y0 = by * B, w = cols - x0 < B ? cols - x0 : B, h = rows - y0 < B ? rows - y0 : B;
    uint32_t acc = 0;
    for (int y = 0; y < h; y++) acc += change_bytes_sum(src + (size_t)(y0 + y) * step + (size_t)3 * x0, 3 * w, 0);
    *npix = w * h;
    return acc;
}

// ---- the step rule
// One block of a step that does not seed: whether it changed, and its new reference value.  |S - ref| <= 65280 * 1024 < 2^27 and
// 16 * thr_q4 * npix <= 16 * 65535 * 1024 < 2^30: both sides fit 32 bits; the shift is arithmetic and floors.
__host__ __device__ inline bool change_step_block(uint32_t S, int npix, int thr_q4, int adapt_shift, int32_t *ref) {
    const int32_t d = (int32_t)S - *ref;
    const bool changed = (long long)(d < 0 ? -d : d) > 16ll * thr_q4 * npix;
    *ref += d >> adapt_shift;
    return changed;
}

// ---- components
// whether block (x, y) is marked after the dilation (8-neighbourhood, one block) of the bw x bh mask
__host__ __device__ inline bool change_dilated(const uint8_t *mask, int bw, int bh, int x, int y, int dilate) {
    if (!dilate) return mask[y * bw + x] != 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int xx = x + dx, yy = y + dy;
            if (xx >= 0 && yy >= 0 && xx < bw && yy < bh && mask[yy * bw + xx]) return true;
        }
    return false;
}

// one component: its label (the smallest raster index in it), its number of marked blocks and its bounding box in blocks
struct ChangeComp {
    int label, count, bx0, by0, bx1, by1;
};

// Host: the 8-connected components of the marked blocks of `marked` (bw x bh bytes, after dilation), by flood fill in raster order, so
// they come out in ascending label.  labels: bw * bh uint16 (kChangeNone: unmarked); stack: bw * bh ints of scratch; comps: room
// for bw * bh records.  Returns their number.
inline int change_label_host(const uint8_t *marked, int bw, int bh, uint16_t *labels, int *stack, ChangeComp *comps) {
    const int nb = bw * bh;
    for (int i = 0; i < nb; i++) labels[i] = (uint16_t)kChangeNone;
    int nc = 0;
    for (int i = 0; i < nb; i++) {
        if (!marked[i] || labels[i] != kChangeNone) continue;
        ChangeComp c = {i, 0, bw, bh, -1, -1};
        int top = 0;
        stack[top++] = i;
        labels[i] = (uint16_t)i;
        while (top) {
            const int j = stack[--top], x = j % bw, y = j / bw;
            c.count++;
            c.bx0 = x < c.bx0 ? x : c.bx0; c.bx1 = x > c.bx1 ? x : c.bx1;
            c.by0 = y < c.by0 ? y : c.by0; c.by1 = y > c.by1 ? y : c.by1;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int xx = x + dx, yy = y + dy;
                    if (xx < 0 || yy < 0 || xx >= bw || yy >= bh) continue;
                    const int k = yy * bw + xx;
                    if (!marked[k] || labels[k] != kChangeNone) continue;
                    labels[k] = (uint16_t)i;
                    stack[top++] = k;
                }
        }
        comps[nc++] = c;
    }
    return nc;
}

// ---- the selection
// whether component a comes before b: count descending, then label ascending
__host__ __device__ inline bool change_before(int count_a, int label_a, int count_b, int label_b) {
    return count_a != count_b ? count_a > count_b : label_a < label_b;
}

// Host: the components with count >= min_blocks in selection order, the first max_regions of them, into `kept`; returns their number
inline int change_select_host(const ChangeComp *comps, int nc, int min_blocks, int max_regions, ChangeComp *kept) {
    int n = 0;
    for (int k = 0; k < max_regions; k++) {
        int best = -1;
        for (int i = 0; i < nc; i++) {
            if (comps[i].count < min_blocks) continue;
            if (n && !change_before(kept[n - 1].count, kept[n - 1].label, comps[i].count, comps[i].label)) continue;      // taken already
            if (best < 0 || change_before(comps[i].count, comps[i].label, comps[best].count, comps[best].label)) best = i;
        }
        if (best < 0) break;
        kept[n++] = comps[best];
    }
    return n;
}

// ---- component -> region -> cell
// The pixel rectangle of a component's box, as a face box through roi_from_face at coord scale 1 with margin_q8 (0 = 64), planned into
// a cell of cw x ch pixels.  *region: the rf_roi (zeros with the void record, which roi_from_face's refusal gives; it never refuses a
// rectangle inside a frame).
__host__ __device__ inline RoiCell change_region(int bx0, int by0, int bx1, int by1, int B, int rows, int cols, int margin_q8, int cw, int ch,
                                                 int max_zoom, rf_roi *region) {
    const int x2 = (bx1 + 1) * B < cols ? (bx1 + 1) * B : cols, y2 = (by1 + 1) * B < rows ? (by1 + 1) * B : rows;
    const float f[5] = {0.f, (float)(bx0 * B), (float)(by0 * B), (float)x2, (float)y2};
    rf_roi r;
    if (!roi_from_face(f, 1.f, margin_q8 ? margin_q8 : 64, &r)) {
        region->x = region->y = region->w = region->h = 0;
        return roi_void_cell();
    }
    *region = r;
    return roi_plan(r, cw, ch, max_zoom);
}

// ---- the whole step on the host (rf_change_step_host): the code the two kernels run
// ref: bw * bh values in and out; *counter in and out; mask: bw * bh bytes out (the changed blocks BEFORE dilation; zero on the seeding
// step); regions / cells: max_regions records out (zeros / the void record behind `kept`); info out.
inline void change_step_host(const ChangeSpec &sp, const uint8_t *src, int rows, int cols, size_t step, int bw, int bh, int32_t *ref,
                             int64_t *counter, int margin_q8, int cw, int ch, int max_zoom, uint8_t *mask, rf_roi *regions, RoiCell *cells,
                             rf_change_info *info) {
    const int nb = bw * bh, B = sp.block;
    const bool seed = *counter == 0;
    int changed = 0;
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            int npix;
            const uint32_t S = change_block_sum(src, rows, cols, step, B, bx, by, &npix);
            const int i = by * bw + bx;
            if (seed) { ref[i] = (int32_t)S; mask[i] = 0; }
            else { mask[i] = change_step_block(S, npix, sp.thr_q4, sp.adapt_shift, &ref[i]) ? 1 : 0; changed += mask[i]; }
        }
    *counter += 1;
    for (int k = 0; k < sp.max_regions; k++) {
        regions[k].x = regions[k].y = regions[k].w = regions[k].h = 0;
        cells[k] = roi_void_cell();
    }
    info->changed_blocks = changed; info->components = 0; info->kept = 0; info->flags = seed ? 1 : 0;
    if (seed || !changed) return;
    uint8_t *marked = new uint8_t[(size_t)nb];
    uint16_t *labels = new uint16_t[(size_t)nb];
    int *stack = new int[(size_t)nb];
    ChangeComp *comps = new ChangeComp[(size_t)nb];
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++) marked[y * bw + x] = change_dilated(mask, bw, bh, x, y, sp.dilate) ? 1 : 0;
    const int nc = change_label_host(marked, bw, bh, labels, stack, comps);
    ChangeComp kept[kChangeMaxRegions];
    const int n = change_select_host(comps, nc, sp.min_blocks, sp.max_regions, kept);
    for (int k = 0; k < n; k++)
        cells[k] = change_region(kept[k].bx0, kept[k].by0, kept[k].bx1, kept[k].by1, B, rows, cols, margin_q8, cw, ch, max_zoom, &regions[k]);
    info->components = nc; info->kept = n;
    delete[] marked; delete[] labels; delete[] stack; delete[] comps;
}

}  // namespace rf
