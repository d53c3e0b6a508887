// shot.h -- the decisions of the best-shot gallery, shared by the kernels (kernels.hip shot_deliver_kernel / shot_keep_kernel) and the
// host entry point rf_shot_resolve (capi.cpp).  A tracker with a gallery keeps, per track slot, the face-batch crop of the track's best
// shot and an rf_shot record; a track that ends is handed that crop (DESIGN.md "Best-shot gallery").  Which bytes a shot consists of is
// the face batch's business (align.h, face_batch.h); what is decided here is WHERE a delivered shot comes from and WHO owns a slot after
// a launch.  Everything is integer arithmetic on frame indices and ids (no floats occur, so there is nothing to contract), so host and
// device agree with each other and with tests/shot_ref.py.  The host runs the pieces below in a sequential loop (shot_resolve); the
// kernels run the same pieces one workgroup per delivered shot / per slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "align.h"
#include "track.h"

namespace rf {

static_assert(sizeof(rf_shot) == 64, "rf_shot is 64 bytes");

// the frame index of the stream's image `ord` of a launch that carried n of its images and left its frame counter at frames_after
__host__ __device__ inline long long shot_first_frame(long long frames_after, int n) { return frames_after - (long long)n; }

// Where the shot of an ended track comes from: it has none (every face it had was gated), it was taken before this launch (the slot's
// stored entry), or its best frame is one of the launch's own images (sampled from that frame: the keep launch has not run for it).
__host__ __device__ inline int shot_source_kind(long long best_frame, long long first_frame) {
    if (best_frame < 0) return RF_SHOT_NONE;
    return best_frame < first_frame ? RF_SHOT_STORED : RF_SHOT_LAUNCH;
}

// the stored record of a track's shot: ids are unique per stream, and the frame must be the track's best frame
__host__ __device__ inline bool shot_record_is(const rf_shot *r, long long id, long long best_frame) {
    return id != 0 && r->id == id && r->frame == best_frame;
}

// the face of a frame that a track's shot was taken from: its tag has the track's id and carries RF_TRACK_BEST
__host__ __device__ inline bool shot_tag_is(const rf_track_tag *g, long long id) { return id != 0 && g->id == id && (g->flags & RF_TRACK_BEST) != 0; }

// The image of the launch (ordinal among the stream's n images) whose face owns the slot of track t after the launch; -1: the launch
// leaves the slot alone (free slot, no best shot, or a best shot from before the launch).
__host__ __device__ inline int shot_owner_ordinal(const rf_track *t, long long first_frame, int n) {
    if (t->id == 0 || t->best_frame < first_frame) return -1;            // first_frame >= 0, so best_frame -1 is covered
    const long long o = t->best_frame - first_frame;
    return o < (long long)n ? (int)o : -1;
}

// faces of an image whose tags the frame step wrote
__host__ __device__ inline int shot_tagged(int count, int faces_per_image, int max_faces) {
    int m = count < 0 ? 0 : count;
    if (m > faces_per_image) m = faces_per_image;
    if (m > max_faces) m = max_faces;
    return m < kTrackMaxFaces ? m : kTrackMaxFaces;
}

__host__ __device__ inline void shot_record_set(rf_shot *r, long long id, long long frame, const double *fwd) {
    r->id = id; r->frame = frame;
    for (int i = 0; i < 6; i++) r->matrix[i] = fwd ? fwd[i] : 0.0;
}

// Host: one stream's n images of one launch, sequential (the header's rf_shot_resolve).  Returns the number of delivered shots.
inline int shot_resolve(int T, int n, const rf_track_tag *tags, int cap_per_image, const int *counts, const rf_track *ended, int cap_ended,
                        const int *ended_counts, long long first_frame, const rf_face *faces, const float *coord_scale, int crop,
                        rf_shot *records, int32_t *source, int32_t *owner) {
    rf_shot before[kTrackMaxTracks];
    memcpy(before, records, (size_t)T * sizeof(rf_shot));
    // the table's (id, best_frame) per slot as the tags tell it: a BEST tag sets it, a delivered track frees it
    rf_track now[kTrackMaxTracks];
    int32_t own[kTrackMaxTracks][2];
    memset(now, 0, sizeof(now));
    for (int s = 0; s < T; s++) own[s][0] = own[s][1] = -1;
    int delivered = 0;
    auto keep = [&](int i, int k, const rf_track_tag &g) {
        if (g.slot < 0 || g.slot >= T) return;
        now[g.slot].id = g.id; now[g.slot].best_frame = first_frame + i;
        own[g.slot][0] = i; own[g.slot][1] = k;
    };
    for (int i = 0; i < n; i++) {
        const int m = shot_tagged(counts[i], cap_per_image, kTrackMaxFaces);
        const rf_track_tag *g = tags + (size_t)i * cap_per_image;
        for (int k = 0; k < m; k++)                                   // matched faces first: the frame step's order
            if ((g[k].flags & RF_TRACK_BEST) && !(g[k].flags & RF_TRACK_NEW) && g[k].id != 0) keep(i, k, g[k]);
        const int ne = ended_counts[i] < cap_ended ? ended_counts[i] : cap_ended;
        for (int e = 0; e < cap_ended; e++) {
            int32_t *src = source ? source + ((size_t)i * cap_ended + e) * 3 : nullptr;
            if (e >= ne) { if (src) src[0] = src[1] = src[2] = -1; continue; }
            const rf_track &t = ended[(size_t)i * cap_ended + e];
            int kind = shot_source_kind(t.best_frame, first_frame), a = 0, b = 0;
            if (kind == RF_SHOT_STORED) {
                a = -1;
                for (int s = 0; s < T; s++)
                    if (shot_record_is(&before[s], t.id, t.best_frame)) { a = s; break; }
                if (a < 0) kind = RF_SHOT_NONE, a = 0;
            } else if (kind == RF_SHOT_LAUNCH) {
                a = (int)(t.best_frame - first_frame); b = -1;
                if (a < n) {
                    const int ma = shot_tagged(counts[a], cap_per_image, kTrackMaxFaces);
                    for (int k = 0; k < ma; k++)
                        if (shot_tag_is(tags + (size_t)a * cap_per_image + k, t.id)) { b = k; break; }
                }
                if (b < 0) kind = RF_SHOT_NONE, a = 0, b = 0;
            }
            if (src) { src[0] = kind; src[1] = a; src[2] = b; }
            delivered++;
            for (int s = 0; s < T; s++) {                             // the slot is free now
                if (now[s].id == t.id) { now[s].id = 0; now[s].best_frame = -1; own[s][0] = own[s][1] = -1; }
                if (records[s].id == t.id) memset(&records[s], 0, sizeof(rf_shot));
            }
        }
        for (int k = 0; k < m; k++)
            if ((g[k].flags & RF_TRACK_BEST) && (g[k].flags & RF_TRACK_NEW) && g[k].id != 0) keep(i, k, g[k]);
    }
    for (int s = 0; s < T; s++) {
        const int o = shot_owner_ordinal(&now[s], first_frame, n);
        if (owner) { owner[2 * s] = o < 0 ? -1 : own[s][0]; owner[2 * s + 1] = o < 0 ? -1 : own[s][1]; }
        if (o < 0) continue;
        AlignXform xf;
        const rf_face *f = faces ? faces + (size_t)own[s][0] * cap_per_image + own[s][1] : nullptr;
        if (f) align_estimate(f->px, f->py, coord_scale ? coord_scale[own[s][0]] : 1.f, crop, &xf);
        shot_record_set(&records[s], now[s].id, now[s].best_frame, f ? xf.fwd : nullptr);
    }
    return delivered;
}

}  // namespace rf
