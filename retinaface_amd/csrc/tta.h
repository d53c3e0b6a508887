// tta.h -- flip test-time augmentation: the mapping of a mirrored pass back into the frame, and the voting merge, shared by the
// kernels (kernels.hip tta_gather_kernel / vote_merge_kernel) and the host entry points rf_tta_map_face / rf_tta_merge_host
// (capi.cpp).  A frame is detected as it is (pass 0) and mirrored left-right (pass 1); the faces of pass 1 are moved back with one
// fp32 subtract per x coordinate and a left/right landmark swap; the faces of both passes are merged by the detector's greedy NMS
// on a total order, and each kept head becomes the score-weighted mean of the candidates it suppressed (DESIGN.md "Flip test-time
// augmentation").  Every step is a single fp32 operation, or a double accumulation whose order is fixed, never contracted, so host
// and device agree bit for bit with each other and with tests/tta_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/retinaface_amd.h"
#include "tile.h"

namespace rf {

constexpr int kTtaMergeCap = 4096;         // candidates per frame the merge holds (one workgroup's LDS, as launch_nms)
constexpr int kTtaMaxFaces = 4096;
static_assert(sizeof(rf_tta_spec) == 16, "rf_tta_spec is 16 bytes");

// a validated rf_tta_spec with its defaults applied
struct TtaSpec {
    int flip = 1, vote = 1, max_faces = 0;
    int passes() const { return flip ? 2 : 1; }
};

// One pass of a call as the gather kernel sees it: pass `pass` (0: the frame, 1: the frame mirrored) of frame `frame`, a
// rows x cols frame whose results are multiplied by `scale` (rf_frame_scale: tile_frame_scale).  frame < 0: nothing to gather.
struct TtaEntry {
    int32_t frame, rows, cols, pass;
    float scale;
};

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *tta_spec_resolve(const rf_tta_spec *in, int default_max_faces, TtaSpec *out) {
    TtaSpec r;
    r.max_faces = default_max_faces;
    if (in) {
        if (in->struct_size != sizeof(rf_tta_spec)) return "rf_tta_spec.struct_size mismatch";
        if (in->flip < 0 || in->flip > 2) return "flip must be 0, 1 or 2";
        if (in->vote < 0 || in->vote > 2) return "vote must be 0, 1 or 2";
        if (in->max_faces < 0 || in->max_faces > kTtaMaxFaces) return "max_faces must be 0 or in [1, 4096]";
        r.flip = in->flip != 2;
        r.vote = in->vote != 2;
        if (in->max_faces) r.max_faces = in->max_faces;
    }
    if (r.max_faces < 1 || r.max_faces > kTtaMaxFaces) return "max_faces must be in [1, 4096]";
    *out = r;
    return nullptr;
}

// The mapping of one face of a pass.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]: the head of rf_face and of
// Candidate), they may alias.  One multiply by the scale per coordinate (also when it is 1); for the mirrored pass one subtract
// from (float)(cols - 1) per x coordinate, the box sides and the landmark pairs (eyes, mouth corners) changing places.
__host__ __device__ inline void tta_map_face(const TtaEntry &e, const float *in, float *out) {
#pragma clang fp contract(off)
    float f[15];
    f[0] = in[0];
    for (int i = 1; i < 15; i++) f[i] = in[i] * e.scale;
    if (e.pass == 1) {
        const float c = (float)(e.cols - 1);
        const float x1 = c - f[3], x2 = c - f[1];
        const float p0 = c - f[6], p1 = c - f[5], p2 = c - f[7], p3 = c - f[9], p4 = c - f[8];
        const float y0 = f[11], y1 = f[10], y3 = f[14], y4 = f[13];
        f[1] = x1; f[3] = x2;
        f[5] = p0; f[6] = p1; f[7] = p2; f[8] = p3; f[9] = p4;
        f[10] = y0; f[11] = y1; f[13] = y3; f[14] = y4;
    }
    for (int i = 0; i < 15; i++) out[i] = f[i];
}

// nms_kernel's suppression expression: does the kept box a (area1 = its +1-pixel area) suppress box b at threshold thr
__host__ __device__ inline bool tta_suppresses(float ax1, float ay1, float ax2, float ay2, float area1, float bx1, float by1, float bx2,
                                               float by2, float thr) {
#pragma clang fp contract(off)
    const float x = fmaxf(ax1, bx1);
    const float y = fmaxf(ay1, by1);
    const float w = fminf(ax2, bx2) - x + 1;
    const float h = fminf(ay2, by2) - y + 1;
    if (w <= 0 || h <= 0) return false;
    const float area2 = (bx2 - bx1 + 1) * (by2 - by1 + 1);
    const float inter = w * h;
    return inter / (area1 + area2 - inter) > thr;
}
__host__ __device__ inline float tta_area(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
    return (x2 - x1 + 1) * (y2 - y1 + 1);
}

// One step of the vote: acc + s * v in double.  The product of two floats is exact in double (24 + 24 significant bits), so a
// fused multiply-add and a multiply followed by an add round the same value once: contraction cannot change a bit here.
__host__ __device__ inline double tta_vote_add(double acc, float s, float v) {
#pragma clang fp contract(off)
    return acc + (double)s * (double)v;
}
__host__ __device__ inline double tta_vote_first(float s, float v) { return (double)s * (double)v; }
__host__ __device__ inline float tta_vote_result(double acc, double sw) { return (float)(acc / sw); }

// Host: the merge of one frame's mapped candidates (15 floats each; g: the tie-break index of each).  Writes the first
// min(heads, cap) merged faces, their member counts and their g; returns the true number of heads.
inline int tta_merge_candidates(const std::vector<float> &cand, const std::vector<int> &g, float thr, bool vote, int cap, float *out,
                                int *votes, int *head_g) {
    const int n = (int)g.size();
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[i] = i;
    auto bits = [&](int i) { uint32_t b; memcpy(&b, &cand[(size_t)i * 15], 4); return b; };
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        const uint32_t sa = bits(a), sb = bits(b);
        return sa != sb ? sa > sb : g[a] < g[b];
    });
    std::vector<char> alive((size_t)n, 1);
    int heads = 0;
    for (int i = 0; i < n; i++) {
        if (!alive[i]) continue;
        const float *h = &cand[(size_t)order[i] * 15];
        const float area1 = tta_area(h[1], h[2], h[3], h[4]);
        double acc[15];
        const bool emit = heads < cap;
        acc[0] = (double)h[0];
        for (int q = 1; q < 15; q++) acc[q] = tta_vote_first(h[0], h[q]);
        int members = 1;
        for (int j = i + 1; j < n; j++) {
            if (!alive[j]) continue;
            const float *m = &cand[(size_t)order[j] * 15];
            if (!tta_suppresses(h[1], h[2], h[3], h[4], area1, m[1], m[2], m[3], m[4], thr)) continue;
            alive[j] = 0;
            members++;
            acc[0] = acc[0] + (double)m[0];
            for (int q = 1; q < 15; q++) acc[q] = tta_vote_add(acc[q], m[0], m[q]);
        }
        if (emit) {
            float *o = out + (size_t)heads * 15;
            o[0] = h[0];
            for (int q = 1; q < 15; q++) o[q] = vote ? tta_vote_result(acc[q], acc[0]) : h[q];
            if (votes) votes[heads] = members;
            if (head_g) head_g[heads] = g[order[i]];
        }
        heads++;
    }
    return heads;
}

}  // namespace rf
