// align.h -- the transform half of 5-point face alignment, shared by the kernel (kernels.hip align_kernel) and the host entry point
// rf_align_matrix (capi.cpp): the least-squares similarity without reflection that maps a face's five landmarks onto the
// usual 112-pixel recognition template scaled to the crop size.  The definition (DESIGN.md "Face alignment") fixes every
// rounding: IEEE double, + - * / only, in the order written here, no contraction into FMA -- host and device therefore agree
// bit for bit with each other and with tests/align_ref.py.
#pragma once
#include <hip/hip_runtime.h>

namespace rf {

constexpr int kAlignMinCrop = 16, kAlignMaxCrop = 512;      // crop edge S the entry points accept
constexpr int kAlignMaxFaces = 4096;                        // crop slots per image (= the largest max_detections)

struct AlignXform {
    double fwd[6];                     // source -> crop, row major 2 x 3; all zero for an invalid face
    double ia, ib;                     // inverse rotation / scale (crop -> source)
    double mpx, mpy, mqx, mqy;         // landmark mean (source pixels), template mean (crop pixels)
    int valid;
};

// px / py: the five landmarks in rf_face order (left eye, right eye, nose, mouth left, mouth right); cs: the coordinate scale
// (1, or rf_frame_scale for a frame the engine shrank); S: crop edge.  Returns t->valid.
__host__ __device__ inline int align_estimate(const float *px, const float *py, float cs, int S, AlignXform *t) {
#pragma clang fp contract(off)
    const double tx[5] = {38.2946, 73.5318, 56.0252, 41.5493, 70.7299};
    const double ty[5] = {51.6963, 51.5014, 71.7366, 92.3655, 92.2041};
    const double c = (double)cs, k = (double)S / 112.0;
    double sx[5], sy[5], qx[5], qy[5];
    double mpx = 0.0, mpy = 0.0, mqx = 0.0, mqy = 0.0;
    for (int i = 0; i < 5; i++) {
        sx[i] = (double)px[i] * c; sy[i] = (double)py[i] * c;
        qx[i] = tx[i] * k; qy[i] = ty[i] * k;
        mpx = mpx + sx[i]; mpy = mpy + sy[i]; mqx = mqx + qx[i]; mqy = mqy + qy[i];
    }
    mpx = mpx / 5.0; mpy = mpy / 5.0; mqx = mqx / 5.0; mqy = mqy / 5.0;
    double sxx = 0.0, sxy = 0.0, n2 = 0.0;
    for (int i = 0; i < 5; i++) {
        const double a = sx[i] - mpx, b = sy[i] - mpy, cc = qx[i] - mqx, d = qy[i] - mqy;
        sxx = sxx + (a * cc + b * d);
        sxy = sxy + (a * d - b * cc);
        n2 = n2 + (a * a + b * b);
    }
    const double A = sxx / n2, B = sxy / n2, D = A * A + B * B;
    const double big = 1.7976931348623157e308;               // finite and > 0 (NaN fails both comparisons)
    t->valid = (n2 > 0.0 && n2 <= big && D > 0.0 && D <= big) ? 1 : 0;
    if (!t->valid) {
        for (int i = 0; i < 6; i++) t->fwd[i] = 0.0;
        t->ia = t->ib = t->mpx = t->mpy = t->mqx = t->mqy = 0.0;
        return 0;
    }
    t->fwd[0] = A; t->fwd[1] = -B; t->fwd[2] = mqx - (A * mpx - B * mpy);
    t->fwd[3] = B; t->fwd[4] = A;  t->fwd[5] = mqy - (B * mpx + A * mpy);
    t->ia = A / D; t->ib = -B / D;
    t->mpx = mpx; t->mpy = mpy; t->mqx = mqx; t->mqy = mqy;
    return 1;
}

// The supersampling factor per axis of an antialiased crop (DESIGN.md "Antialiased face crops"): R = source pixels per crop pixel,
// squared; the smallest power of two k <= aa_max (1, 2, 4 or 8) with sub-sample spacing sqrt(R) / k <= sqrt(2) source pixels.
// An invalid face has k = 1.
__host__ __device__ inline int align_aa_factor(const AlignXform &t, int aa_max) {
#pragma clang fp contract(off)
    if (!t.valid) return 1;
    const double a2 = t.ia * t.ia, b2 = t.ib * t.ib;
    const double R = a2 + b2;
    int k = 1;
    while (k < aa_max && (double)(k * k) * 2.0 < R) k *= 2;
    return k;
}

}  // namespace rf
