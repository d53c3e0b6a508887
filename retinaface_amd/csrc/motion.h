// motion.h -- motion-predicted face tracks, shared by the kernels (kernels.hip track_motion_kernel, the coasting variant of
// redact_regions_kernel) and the host entry points rf_track_step_motion / rf_track_predict (capi.cpp).  A tracker with motion keeps one
// rf_track_motion per track slot: a velocity of the box centre, smoothed exponentially over the matches.  The frame step is track.h's with
// two changes -- a face is matched against the track's PREDICTED box, and a matched track updates its velocity -- and redaction coasts
// at the predicted box (DESIGN.md "Motion-predicted tracks").  Everything here is fp32 with one rounding per operation (never contracted)
// or integer arithmetic, so host and device agree bit for bit with each other and with tests/motion_ref.py.  The host runs the pieces
// below in a sequential loop (track_step_motion); the kernel runs the same pieces one thread per slot.
#pragma once
#include "track.h"

namespace rf {

static_assert(sizeof(rf_motion_spec) == 16, "rf_motion_spec is 16 bytes");
static_assert(sizeof(rf_track_motion) == 16, "rf_track_motion is 16 bytes");

constexpr int kMotionMaxHorizon = 65536;
constexpr int kMotionMaxSamples = 1 << 30;

// a validated rf_motion_spec with its defaults applied; horizon 0 = never extrapolate (the caller's negative)
struct MotionSpec {
    float alpha;
    int horizon;
};

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *motion_spec_resolve(const rf_motion_spec *in, MotionSpec *out) {
    MotionSpec r = {0.5f, 8};
    if (in) {
        if (in->struct_size != sizeof(rf_motion_spec)) return "rf_motion_spec.struct_size mismatch";
        if (in->reserved != 0) return "rf_motion_spec.reserved must be 0";
        if (!track_finite(in->alpha) || in->alpha < 0.f || in->alpha > 1.f) return "alpha must be finite and in (0, 1] (0 = 0.5)";
        if (in->horizon > kMotionMaxHorizon) return "horizon must be in [1, 65536] (0 = 8, negative = never extrapolate)";
        if (in->alpha != 0.f) r.alpha = in->alpha;
        if (in->horizon) r.horizon = in->horizon < 0 ? 0 : in->horizon;
    }
    *out = r;
    return nullptr;
}

// frames a box is extrapolated: min(missed + ahead, horizon); ahead is 0 or 1, missed >= 0
__host__ __device__ inline int motion_frames_ahead(int missed, int ahead, int horizon) {
    return missed < horizon - ahead ? missed + ahead : horizon;
}

// The predicted box (x1, y1, x2, y2) of a track h frames ahead.  samples == 0 or h == 0: `last`, the same bytes.
__host__ __device__ inline void motion_predict_box(const float *last, float vx, float vy, int samples, int h, float *box) {
#pragma clang fp contract(off)
    if (samples == 0 || h == 0) { box[0] = last[0]; box[1] = last[1]; box[2] = last[2]; box[3] = last[3]; return; }
    const float dx = vx * (float)h, dy = vy * (float)h;
    box[0] = last[0] + dx; box[1] = last[1] + dy; box[2] = last[2] + dx; box[3] = last[3] + dy;
}

// the predicted face: the box as above, the landmarks moved with it, the score copied
__host__ __device__ inline void motion_predict_face(const rf_face *last, const rf_track_motion *m, int h, rf_face *out) {
#pragma clang fp contract(off)
    *out = *last;
    if (m->samples == 0 || h == 0) return;
    const float dx = m->vx * (float)h, dy = m->vy * (float)h;
    out->x1 = last->x1 + dx; out->y1 = last->y1 + dy; out->x2 = last->x2 + dx; out->y2 = last->y2 + dy;
    for (int i = 0; i < 5; i++) { out->px[i] = last->px[i] + dx; out->py[i] = last->py[i] + dy; }
}

// A matched track's velocity, before `last` is overwritten: box = the new mapped box, last = the old one (x1, y1, x2, y2 each),
// missed = the track's missed count before the match.
__host__ __device__ inline void motion_update(float *vx, float *vy, int *samples, const float *box, const float *last, int missed, float alpha) {
#pragma clang fp contract(off)
    float rx = (box[0] + box[2]) * 0.5f - (last[0] + last[2]) * 0.5f;
    float ry = (box[1] + box[3]) * 0.5f - (last[1] + last[3]) * 0.5f;
    if (missed != 0) {                                           // x / 1 is x, bit for bit: the usual match needs no division
        const float dt = (float)((unsigned int)missed + 1u);     // missed >= 0: no overflow, one conversion
        rx = rx / dt;
        ry = ry / dt;
    }
    float nx = rx, ny = ry;
    if (*samples != 0) {
        nx = *vx + alpha * (rx - *vx);
        ny = *vy + alpha * (ry - *vy);
    }
    const bool ok = nx == nx && nx - nx == 0.f && ny == ny && ny - ny == 0.f;            // track_finite
    *vx = ok ? nx : 0.f;
    *vy = ok ? ny : 0.f;
    *samples = ok ? (*samples < kMotionMaxSamples ? *samples + 1 : kMotionMaxSamples) : 0;
}

// Host: track_step with motion records, sequential; arguments as there, motion: max_tracks records.
inline int track_step_motion(const TrackSpec &sp, const MotionSpec &ms, rf_track *table, rf_track_motion *motion, int64_t *frames,
                             int64_t *next_id, const float *faces, int stride_floats, int m, float scale, const rf_face_quality *quality,
                             rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_count) {
    const int T = sp.max_tracks;
    const long long f = *frames;
    *frames = f + 1;
    float mapped[kTrackMaxFaces][15];
    float pred[kTrackMaxTracks][4];
    bool claimed[kTrackMaxTracks] = {};
    int slot_of[kTrackMaxFaces];
    for (int k = 0; k < m; k++) track_map_face(faces + (size_t)k * stride_floats, scale, mapped[k]);
    for (int s = 0; s < T; s++) {
        const rf_track &t = table[s];
        if (t.id == 0) { pred[s][0] = pred[s][1] = pred[s][2] = pred[s][3] = 0.f; continue; }
        motion_predict_box(&t.last.x1, motion[s].vx, motion[s].vy, motion[s].samples, motion_frames_ahead(t.missed, 1, ms.horizon), pred[s]);
    }
    for (int k = 0; k < m; k++) {
        unsigned long long best = 0;
        for (int s = 0; s < T; s++) {
            const bool avail = table[s].id != 0 && !claimed[s];
            const float iou = avail ? track_iou(mapped[k] + 1, pred[s]) : 0.f;
            const unsigned long long key = track_match_key(avail, iou, sp.min_iou, s);
            if (key > best) best = key;
        }
        slot_of[k] = -1;
        if (!best) continue;
        const int s = track_key_slot(best);
        claimed[s] = true;
        slot_of[k] = s;
        motion_update(&motion[s].vx, &motion[s].vy, &motion[s].samples, mapped[k] + 1, &table[s].last.x1, table[s].missed, ms.alpha);
        motion[s].reserved = 0;
        track_match_update(&table[s], mapped[k], f, sp.min_hits);
        const int b = track_best_update(&table[s], mapped[k], f, quality ? quality + k : nullptr);
        tags[k] = track_tag(&table[s], s, f, sp.min_hits, b);
    }
    int n_ended = 0;
    for (int s = 0; s < T; s++) {
        rf_track &t = table[s];
        if (t.id == 0 || claimed[s]) continue;
        if (!track_age(&t, sp.max_missed)) continue;
        if (n_ended < cap_ended && ended) ended[n_ended] = t;
        n_ended++;
        memset(&t, 0, sizeof(t));
        memset(&motion[s], 0, sizeof(rf_track_motion));
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
        memset(&motion[s_free], 0, sizeof(rf_track_motion));
        const int b = track_best_update(&t, mapped[k], f, quality ? quality + k : nullptr);
        tags[k] = track_tag(&t, s_free, f, sp.min_hits, RF_TRACK_NEW | b);
    }
    return status;
}

}  // namespace rf
