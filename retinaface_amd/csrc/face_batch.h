// face_batch.h -- the value half of recogniser-ready face batches, shared by the kernel (kernels.hip face_batch_kernel) and the
// host entry points rf_face_value_table / rf_face_batch_plan (capi.cpp).  A face batch is the aligned crops of one call as one
// dense tensor in the recogniser's layout and number format (DESIGN.md "Face batches"): an output element is a function of the
// u8 crop value q (align.h + the sampling of align_kernel define it) and the output channel c alone, the 256-entry map below.
// Every rounding is fixed -- one fp32 subtract, one fp32 multiply, never contracted, then round-to-nearest-even to half -- so host
// and device agree bit for bit with each other and with tests/face_batch_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "align.h"

namespace rf {

constexpr int kFaceBatchDefaultCrop = 112;
constexpr int kFaceDefaultAaMax = 4;
constexpr size_t kFaceSpecSizeV1 = 48;                                 // rf_face_batch_spec up to and including capacity: antialias = 0
static_assert(sizeof(rf_face_batch_spec) == 56, "rf_face_batch_spec is 56 bytes");

// aa_max as a caller gives it (0 = the default) -> 1, 2, 4 or 8; 0 for anything else
inline int face_aa_max_resolve(int aa_max) {
    if (aa_max == 0) return kFaceDefaultAaMax;
    return (aa_max == 1 || aa_max == 2 || aa_max == 4 || aa_max == 8) ? aa_max : 0;
}

// a validated rf_face_batch_spec with its defaults applied
struct FaceBatchSpec {
    int crop = kFaceBatchDefaultCrop, format = RF_FACES_U8_HWC, rgb = 0;
    float mean[3] = {127.5f, 127.5f, 127.5f}, scale[3] = {1.f / 128.f, 1.f / 128.f, 1.f / 128.f};      // per OUTPUT channel
    int max_faces = 0, capacity = 0;
    int antialias = 0, aa_max = 4;                                     // supersampled sampling (align_aa_factor) and its largest factor
    __host__ __device__ int elem_bytes() const { return format == RF_FACES_F32_CHW ? 4 : format == RF_FACES_F16_CHW ? 2 : 1; }
    size_t bytes_per_face() const { return (size_t)3 * crop * crop * elem_bytes(); }
};

// the map itself: u8 crop value q -> the fp32 output value of a channel with this mean and scale
__host__ __device__ inline float face_value_f32(unsigned q, float mean, float scale) {
#pragma clang fp contract(off)
    const float d = (float)q - mean;
    return d * scale;
}
template <typename E> __host__ __device__ inline E face_value(unsigned q, float mean, float scale);
template <> __host__ __device__ inline uint8_t face_value<uint8_t>(unsigned q, float, float) { return (uint8_t)q; }
template <> __host__ __device__ inline float face_value<float>(unsigned q, float mean, float scale) { return face_value_f32(q, mean, scale); }
template <> __host__ __device__ inline _Float16 face_value<_Float16>(unsigned q, float mean, float scale) {
    return (_Float16)face_value_f32(q, mean, scale);                  // IEEE half, round to nearest even
}

inline bool face_batch_finite(float v) { return v == v && v - v == 0.f; }

// Host: check a caller's spec and apply its defaults (crop 0 = 112, all-zero scale = (v - 127.5) / 128, max_faces 0 =
// default_max_faces, aa_max 0 = 4).  struct_size is the current size or the one before antialias / aa_max were appended (they are 0
// then): only that many bytes of the caller's struct are read.  Returns nullptr, or what is wrong with it.
inline const char *face_batch_resolve(const rf_face_batch_spec *in, int default_max_faces, FaceBatchSpec *out) {
    if (!in) return "face batch spec is null";
    if (in->struct_size != sizeof(rf_face_batch_spec) && in->struct_size != kFaceSpecSizeV1) return "rf_face_batch_spec.struct_size mismatch";
    rf_face_batch_spec local;
    memset(&local, 0, sizeof(local));
    memcpy(&local, in, in->struct_size);
    const rf_face_batch_spec *s = &local;
    if (s->antialias != 0 && s->antialias != 1) return "antialias must be 0 or 1";
    if (!face_aa_max_resolve(s->aa_max)) return "aa_max must be 0, 1, 2, 4 or 8";
    if (s->crop_size != 0 && (s->crop_size < kAlignMinCrop || s->crop_size > kAlignMaxCrop)) return "crop_size must be 0 or in [16, 512]";
    if (s->format != RF_FACES_U8_HWC && s->format != RF_FACES_F16_CHW && s->format != RF_FACES_F32_CHW) return "unknown face format";
    if (s->max_faces < 0 || s->max_faces > kAlignMaxFaces) return "max_faces must be 0 or in [1, 4096]";
    if (s->capacity < 1) return "capacity must be >= 1";
    for (int c = 0; c < 3; c++)
        if (!face_batch_finite(s->mean[c]) || !face_batch_finite(s->scale[c])) return "mean / scale must be finite";
    FaceBatchSpec r;
    r.crop = s->crop_size ? s->crop_size : kFaceBatchDefaultCrop;
    r.format = s->format;
    r.rgb = s->rgb ? 1 : 0;
    if (s->scale[0] != 0.f || s->scale[1] != 0.f || s->scale[2] != 0.f)
        for (int c = 0; c < 3; c++) { r.mean[c] = s->mean[c]; r.scale[c] = s->scale[c]; }
    r.max_faces = s->max_faces ? s->max_faces : default_max_faces;
    if (r.max_faces < 1 || r.max_faces > kAlignMaxFaces) return "max_faces must be in [1, 4096]";
    r.capacity = s->capacity;
    r.antialias = s->antialias;
    r.aa_max = face_aa_max_resolve(s->aa_max);
    *out = r;
    return nullptr;
}

// Host: packed offsets of a call -- offsets[i + 1] = offsets[i] + min(counts[i], limit); returns the total, -1 for a negative count.
// offsets may be nullptr.  The scan kernel computes the same numbers on the device from the counts the NMS kernel wrote.
inline long face_batch_offsets(const int *counts, int n, int limit, int *offsets) {
    long total = 0;
    if (offsets) offsets[0] = 0;
    for (int i = 0; i < n; i++) {
        if (counts[i] < 0) return -1;
        total += counts[i] < limit ? counts[i] : limit;
        if (offsets) offsets[i + 1] = (int)total;
    }
    return total;
}

}  // namespace rf
