// track.h -- the frame step of face tracks, shared by the kernel (kernels.hip track_kernel) and the host entry point rf_track_step
// (capi.cpp).  A stream keeps a table of track slots between calls; one frame step associates the faces of one image with the live
// tracks (greedy in score order, by the detector's own NMS overlap), keeps each track's best shot, ages and ends the tracks nobody
// claimed and opens tracks for the faces left over (DESIGN.md "Face tracks").  Everything here is integer arithmetic, fp32 with one
// rounding per operation (never contracted) or an IEEE double comparison, so host and device agree bit for bit with each other and with
// tests/track_ref.py.  The host runs the pieces below in a sequential loop (track_step); the kernel runs the same pieces one thread per
// slot.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"

namespace rf {

constexpr int kTrackMaxTracks = 256;       // slots per stream (one thread each)
constexpr int kTrackMaxFaces = 256;        // faces of one image a frame step looks at
constexpr int kTrackMaxStreams = 1024;
static_assert(sizeof(rf_track_spec) == 24, "rf_track_spec is 24 bytes");
static_assert(sizeof(rf_track) == 176, "rf_track is 176 bytes");
static_assert(sizeof(rf_track_tag) == 24, "rf_track_tag is 24 bytes");

// a validated rf_track_spec with its defaults applied
struct TrackSpec {
    int max_tracks = 64;
    float min_iou = 0.3f;
    int max_missed = 10, min_hits = 3;
    float new_score = 0.f;
};

// what a stream keeps in front of its table in device memory
struct TrackHeader { int64_t frames, next_id; };

// step results beyond the tags (bits of track_step's return value and of the kernel's per-image status word)
enum { kTrackOverflow = 1, kTrackEndedCut = 2 };

inline bool track_finite(float x) { return x == x && x - x == 0.f; }

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *track_spec_resolve(const rf_track_spec *in, TrackSpec *out) {
    TrackSpec r;
    if (in) {
        if (in->struct_size != sizeof(rf_track_spec)) return "rf_track_spec.struct_size mismatch";
        if (in->max_tracks < 0 || in->max_tracks > kTrackMaxTracks) return "max_tracks must be 0 or in [1, 256]";
        if (!track_finite(in->min_iou) || in->min_iou < 0.f || in->min_iou > 1.f) return "min_iou must be finite and in (0, 1] (0 = 0.3)";
        if (!track_finite(in->new_score) || in->new_score < 0.f) return "new_score must be finite and >= 0";
        if (in->max_tracks) r.max_tracks = in->max_tracks;
        if (in->min_iou != 0.f) r.min_iou = in->min_iou;
        if (in->max_missed) r.max_missed = in->max_missed < 0 ? 0 : in->max_missed;
        if (in->min_hits) r.min_hits = in->min_hits < 0 ? 1 : in->min_hits;
        r.new_score = in->new_score;
    }
    *out = r;
    return nullptr;
}

// map: 15 floats (score, x1, y1, x2, y2, px[5], py[5]); one fp32 multiply per coordinate, a scale of 1 included
__host__ __device__ inline void track_map_face(const float *in, float scale, float *out) {
#pragma clang fp contract(off)
    out[0] = in[0];
    for (int i = 1; i < 15; i++) out[i] = in[i] * scale;
}

// The overlap of a face's box with a track's last box (x1, y1, x2, y2 each): the expression of nms_kernel's suppression sweep with
// the face in the place of the kept box.  0 when the boxes do not meet.
__host__ __device__ inline float track_iou(const float *face, const float *last) {
#pragma clang fp contract(off)
    const float area1 = (face[2] - face[0] + 1) * (face[3] - face[1] + 1);
    const float x = fmaxf(face[0], last[0]);
    const float y = fmaxf(face[1], last[1]);
    const float w = fminf(face[2], last[2]) - x + 1;
    const float h = fminf(face[3], last[3]) - y + 1;
    if (w <= 0 || h <= 0) return 0.f;
    const float area2 = (last[2] - last[0] + 1) * (last[3] - last[1] + 1);
    const float inter = w * h;
    return inter / (area1 + area2 - inter);
}

// The match key of slot `slot` for a face: 0 = not eligible; otherwise larger = better.  An eligible overlap is a positive float, so
// its bit order is its numeric order; the low word breaks ties to the lowest slot.  The maximum over the slots is the definition.
__host__ __device__ inline unsigned long long track_match_key(bool available, float iou, float min_iou, int slot) {
    if (!available || !(iou >= min_iou)) return 0ull;
    unsigned int bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(iou);
#else
    memcpy(&bits, &iou, 4);
#endif
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)slot);
}
__host__ __device__ inline int track_key_slot(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull)); }

__host__ __device__ inline void track_set_face(rf_face *dst, const float *f) {
    dst->score = f[0]; dst->x1 = f[1]; dst->y1 = f[2]; dst->x2 = f[3]; dst->y2 = f[4];
    for (int i = 0; i < 5; i++) { dst->px[i] = f[5 + i]; dst->py[i] = f[10 + i]; }
}

// a matched track takes the (mapped) face of frame f
__host__ __device__ inline void track_match_update(rf_track *t, const float *face, long long f, int min_hits) {
    track_set_face(&t->last, face);
    t->last_frame = f;
    t->hits += 1;
    t->missed = 0;
    if (t->hits >= min_hits) t->flags |= RF_TRACK_CONFIRMED;
}

// a free slot becomes the track `id`, opened by the (mapped) face of frame f
__host__ __device__ inline void track_open(rf_track *t, long long id, const float *face, long long f, int min_hits) {
    t->id = id;
    t->first_frame = f; t->last_frame = f; t->best_frame = -1;
    t->best_value = 0.0;
    t->hits = 1; t->missed = 0; t->flags = 1 >= min_hits ? RF_TRACK_CONFIRMED : 0; t->reserved = 0;
    track_set_face(&t->last, face);
    rf_face z;
    z.score = 0.f; z.x1 = z.y1 = z.x2 = z.y2 = 0.f;
    for (int i = 0; i < 5; i++) z.px[i] = z.py[i] = 0.f;
    t->best = z;
}

// The best shot: q = the face's quality record or nullptr (then every face is eligible and its value is its score).  Returns
// RF_TRACK_BEST when the face became the track's best shot, else 0.
__host__ __device__ inline int track_best_update(rf_track *t, const float *face, long long f, const rf_face_quality *q) {
    if (q && q->flags != 0) return 0;
    const double value = q ? q->sharpness : (double)face[0];
    if (!(t->best_frame < 0 || value > t->best_value)) return 0;
    t->best_frame = f;
    t->best_value = value;
    track_set_face(&t->best, face);
    return RF_TRACK_BEST;
}

// the tag of a face tracked by slot `slot` in frame f; extra: RF_TRACK_NEW / RF_TRACK_BEST as they apply
__host__ __device__ inline rf_track_tag track_tag(const rf_track *t, int slot, long long f, int min_hits, int extra) {
    rf_track_tag g;
    g.id = t->id; g.slot = slot; g.hits = t->hits;
    const long long age = f - t->first_frame + 1;
    g.age = (int32_t)(age < 2147483647ll ? age : 2147483647ll);
    g.flags = extra | (t->hits >= min_hits ? RF_TRACK_CONFIRMED : 0);
    return g;
}
__host__ __device__ inline rf_track_tag track_tag_untracked(int extra) {
    rf_track_tag g;
    g.id = 0; g.slot = -1; g.hits = 0; g.age = 0; g.flags = RF_TRACK_UNTRACKED | extra;
    return g;
}
__host__ __device__ inline rf_track_tag track_tag_zero() {
    rf_track_tag g;
    g.id = 0; g.slot = 0; g.hits = 0; g.age = 0; g.flags = 0;
    return g;
}

// ageing of a live track nobody claimed; true: it ends in this frame
__host__ __device__ inline bool track_age(rf_track *t, int max_missed) {
    t->missed += 1;
    return t->missed > max_missed;
}

// Host: one frame step, sequential.  faces: `count` records of `stride_floats` floats in score order (unmapped); m = the faces the step
// looks at (<= kTrackMaxFaces, <= count); quality: nullptr or m records.  tags: m records (the caller tags the faces beyond m).
// Returns kTrackOverflow | kTrackEndedCut as they apply.
inline int track_step(const TrackSpec &sp, rf_track *table, int64_t *frames, int64_t *next_id, const float *faces, int stride_floats,
                      int m, float scale, const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended, int cap_ended,
                      int *ended_count) {
    const int T = sp.max_tracks;
    const long long f = *frames;
    *frames = f + 1;
    float mapped[kTrackMaxFaces][15];
    bool claimed[kTrackMaxTracks] = {};
    int slot_of[kTrackMaxFaces];
    int best_of[kTrackMaxFaces];
    for (int k = 0; k < m; k++) track_map_face(faces + (size_t)k * stride_floats, scale, mapped[k]);
    for (int k = 0; k < m; k++) {
        unsigned long long best = 0;
        for (int s = 0; s < T; s++) {
            const rf_track &t = table[s];
            const bool avail = t.id != 0 && !claimed[s];
            const float iou = avail ? track_iou(mapped[k] + 1, &t.last.x1) : 0.f;
            const unsigned long long key = track_match_key(avail, iou, sp.min_iou, s);
            if (key > best) best = key;
        }
        slot_of[k] = -1; best_of[k] = 0;
        if (!best) continue;
        const int s = track_key_slot(best);
        claimed[s] = true;
        slot_of[k] = s;
        track_match_update(&table[s], mapped[k], f, sp.min_hits);
        best_of[k] = track_best_update(&table[s], mapped[k], f, quality ? quality + k : nullptr);
        tags[k] = track_tag(&table[s], s, f, sp.min_hits, best_of[k]);
    }
    int n_ended = 0;
    for (int s = 0; s < T; s++) {
        rf_track &t = table[s];
        if (t.id == 0 || claimed[s]) continue;
        if (!track_age(&t, sp.max_missed)) continue;
        if (n_ended < cap_ended && ended) ended[n_ended] = t;
        n_ended++;
        memset(&t, 0, sizeof(t));
    }
    if (ended_count) *ended_count = n_ended;
    int status = n_ended > cap_ended ? kTrackEndedCut : 0;
    int s_free = 0;
    for (int k = 0; k < m; k++) {
        if (slot_of[k] >= 0) continue;
        if (!(mapped[k][0] >= sp.new_score)) { tags[k] = track_tag_untracked(0); continue; }
        while (s_free < T && table[s_free].id != 0) s_free++;
        if (s_free >= T) { tags[k] = track_tag_untracked(RF_TRACK_OVERFLOW); status |= kTrackOverflow; continue; }
        rf_track &t = table[s_free];
        track_open(&t, (*next_id)++, mapped[k], f, sp.min_hits);
        const int b = track_best_update(&t, mapped[k], f, quality ? quality + k : nullptr);
        tags[k] = track_tag(&t, s_free, f, sp.min_hits, RF_TRACK_NEW | b);
    }
    return status;
}

}  // namespace rf
