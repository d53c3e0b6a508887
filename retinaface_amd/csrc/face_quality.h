// face_quality.h -- the arithmetic of face quality records and gates, shared by the kernels (kernels.hip face_quality_kernel) and the
// host entry points rf_face_pose / rf_face_gate_eval (capi.cpp).  A record is a few exact numbers of one aligned face (DESIGN.md
// "Face quality"): integer sums over the luma of its crop (independent of the order they are reduced in) and landmark numbers in IEEE
// double, + - * / only, in the order written here, never contracted -- so host and device agree bit for bit with each other and with
// tests/face_quality_ref.py.  A gate turns a record into the flags that decide whether the face is packed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/retinaface_amd.h"
#include "align.h"
#include "face_batch.h"

namespace rf {

static_assert(sizeof(rf_face_quality) == 64, "rf_face_quality is 64 bytes");

// a validated rf_face_gate: every threshold widened to double; 0 = that gate is off
struct FaceGate {
    double min_sharpness = 0.0, min_iod = 0.0, max_abs_yaw = 0.0, max_sin2_roll = 0.0, min_covered = 0.0, min_luma = 0.0, max_luma = 0.0;
};

// Y of one u8 BGR pixel
__host__ __device__ inline unsigned face_luma(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }

// The landmark numbers of a face whose similarity is t (align_estimate with the same px, py, cs, S): iod2, yaw, sin2_roll into *q.
// An invalid face gets zeros.  Nothing else of *q is touched.
__host__ __device__ inline void face_pose(const float *px, const float *py, float cs, const AlignXform &t, rf_face_quality *q) {
#pragma clang fp contract(off)
    if (!t.valid) { q->iod2 = q->yaw = q->sin2_roll = 0.0; return; }
    const double c = (double)cs;
    const double p0x = (double)px[0] * c, p0y = (double)py[0] * c, p1x = (double)px[1] * c, p1y = (double)py[1] * c;
    const double p2x = (double)px[2] * c, p2y = (double)py[2] * c;
    const double ex = p1x - p0x, ey = p1y - p0y;
    const double iod2 = ex * ex + ey * ey;
    const double mx = (p0x + p1x) / 2.0, my = (p0y + p1y) / 2.0;
    q->iod2 = iod2;
    q->yaw = ((p2x - mx) * ex + (p2y - my) * ey) / iod2;
    q->sin2_roll = t.fwd[3] * t.fwd[3] / (t.fwd[0] * t.fwd[0] + t.fwd[3] * t.fwd[3]);
}

// the integer sums of a record -> its sharpness (the variance of the Laplacian over the (S - 2)^2 interior pixels)
__host__ __device__ inline double face_quality_finish(long long sum_lap, long long sum_lap2, int S) {
#pragma clang fp contract(off)
    const long long n = (long long)(S - 2) * (S - 2);
    const long long num = n * sum_lap2 - sum_lap * sum_lap;      // <= 7.0e16 at S = 512
    return (double)num / ((double)n * (double)n);
}

// The flags gate g gives record q of crop size S (`invalid`: the face has no similarity).  Written so that NaN and infinity fail.
__host__ __device__ inline int face_gate_eval(const FaceGate &g, const rf_face_quality &q, int invalid, int S) {
#pragma clang fp contract(off)
    const double area = (double)(S * S);
    int f = invalid ? RF_GATE_INVALID : 0;
    if (g.min_sharpness != 0.0 && !(q.sharpness >= g.min_sharpness)) f |= RF_GATE_SHARPNESS;
    if (g.min_iod != 0.0 && !(q.iod2 >= g.min_iod * g.min_iod)) f |= RF_GATE_IOD;
    if (g.max_abs_yaw != 0.0 && !(q.yaw >= -g.max_abs_yaw && q.yaw <= g.max_abs_yaw)) f |= RF_GATE_YAW;
    if (g.max_sin2_roll != 0.0 && !(q.sin2_roll <= g.max_sin2_roll)) f |= RF_GATE_ROLL;
    if (g.min_covered != 0.0 && !((double)q.covered >= g.min_covered * area)) f |= RF_GATE_COVERED;
    if (g.min_luma != 0.0 && !((double)q.sum_luma >= g.min_luma * area)) f |= RF_GATE_DARK;
    if (g.max_luma != 0.0 && !((double)q.sum_luma <= g.max_luma * area)) f |= RF_GATE_BRIGHT;
    return f;
}

// Host: check a caller's gate and widen it.  Returns nullptr, or what is wrong with it.
inline const char *face_gate_resolve(const rf_face_gate *g, FaceGate *out) {
    if (!g) return "face gate is null";
    if (g->struct_size != sizeof(rf_face_gate)) return "rf_face_gate.struct_size mismatch";
    const float v[7] = {g->min_sharpness, g->min_iod, g->max_abs_yaw, g->max_sin2_roll, g->min_covered, g->min_luma, g->max_luma};
    for (float x : v)
        if (!face_batch_finite(x) || x < 0.f) return "face gate fields must be finite and >= 0";
    if (g->min_covered > 1.f) return "min_covered is a fraction: at most 1";
    out->min_sharpness = (double)v[0]; out->min_iod = (double)v[1]; out->max_abs_yaw = (double)v[2]; out->max_sin2_roll = (double)v[3];
    out->min_covered = (double)v[4]; out->min_luma = (double)v[5]; out->max_luma = (double)v[6];
    return nullptr;
}

}  // namespace rf
