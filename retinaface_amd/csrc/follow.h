// follow.h -- followed face tracks, shared by the kernels (kernels.hip follow_keep_kernel / follow_search_kernel / follow_step_kernel)
// and the host entry points rf_follow_geometry / rf_follow_template / rf_follow_search / rf_track_step_follow_key / rf_track_step_follow
// (capi.cpp).  A tracker with follow keeps, per track slot, a 32 x 32 template of luma cell means taken at the track's box on a key
// frame and an rf_track_follow record; on a frame without detections a block-matching search over the new frame's luma moves the box by
// whole cells (DESIGN.md "Followed tracks").  Everything is integer arithmetic, except one fp32 add per coordinate of a moved box (never
// contracted), so host and device agree bit for bit with each other and with tests/follow_ref.py.  The host runs the pieces below in a
// sequential loop; the kernels run the same pieces one workgroup per slot (template, search) and one thread per slot (step).
#pragma once
#include "face_quality.h"
#include "track.h"

namespace rf {

static_assert(sizeof(rf_follow_spec) == 20, "rf_follow_spec is 20 bytes");
static_assert(sizeof(rf_track_follow) == 32, "rf_track_follow is 32 bytes");

constexpr int kFollowG = 32;                       // the template is G x G cells
constexpr int kFollowCells = kFollowG * kFollowG;  // bytes of a template
constexpr int kFollowMaxRadius = 16;
constexpr int kFollowMaxRun = 65536;
constexpr int kFollowWin = kFollowG + 2 * kFollowMaxRadius;      // cells per side of the largest search window (64: 4 KB)

// a validated rf_follow_spec with its defaults applied
struct FollowSpec {
    int radius, max_mad, max_run;
};

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *follow_spec_resolve(const rf_follow_spec *in, FollowSpec *out) {
    FollowSpec r = {8, 16, 8};
    if (in) {
        if (in->struct_size != sizeof(rf_follow_spec)) return "rf_follow_spec.struct_size mismatch";
        if (in->reserved != 0) return "rf_follow_spec.reserved must be 0";
        if (in->radius < 0 || in->radius > kFollowMaxRadius) return "radius must be in [1, 16] (0 = 8)";
        if (in->max_mad < 0 || in->max_mad > 255) return "max_mad must be in [1, 255] (0 = 16)";
        if (in->max_run < 0 || in->max_run > kFollowMaxRun) return "max_run must be in [1, 65536] (0 = 8)";
        if (in->radius) r.radius = in->radius;
        if (in->max_mad) r.max_mad = in->max_mad;
        if (in->max_run) r.max_run = in->max_run;
    }
    *out = r;
    return nullptr;
}

// one frame: u8 BGR, row y at ptr + y * step
struct FollowFrame {
    const uint8_t *ptr;
    int rows, cols, step;
};

// the lattice of a box: cell edge q and the origin of cell (0, 0); valid = 0: the box has none
struct FollowGeom {
    int valid, q, ox, oy;
};

__host__ __device__ inline int follow_floordiv2(int v) { return v >> 1; }      // arithmetic shift: floor for negative v too

// floor of a finite coordinate clamped to [-4096, 8192]
__host__ __device__ inline int follow_floor(float v) {
    const float c = v < -4096.f ? -4096.f : (v > 8192.f ? 8192.f : v);
    return (int)floorf(c);
}

// box: x1, y1, x2, y2 in source-frame pixels
__host__ __device__ inline FollowGeom follow_geometry(const float *box) {
    FollowGeom g = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++)
        if (!(box[i] == box[i] && box[i] - box[i] == 0.f)) return g;         // track_finite
    const int ix1 = follow_floor(box[0]), iy1 = follow_floor(box[1]), ix2 = follow_floor(box[2]), iy2 = follow_floor(box[3]);
    const int W = ix2 - ix1 + 1, H = iy2 - iy1 + 1;
    if (W < 1 || H < 1) return g;
    const int side = W > H ? W : H;
    int q = (side + kFollowG - 1) / kFollowG;
    if (q < 1) q = 1;
    g.valid = 1; g.q = q;
    g.ox = follow_floordiv2(ix1 + ix2 + 1 - kFollowG * q);
    g.oy = follow_floordiv2(iy1 + iy2 + 1 - kFollowG * q);
    return g;
}

__host__ __device__ inline int follow_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The value of the cell whose top-left pixel is (cx, cy): the rounded mean luma of its q x q pixels, every coordinate clamped into the
// frame.  rows, cols >= 1; q <= 385, so the sum stays below 2^26.
__host__ __device__ inline unsigned follow_cell(const FollowFrame &fd, int cx, int cy, int q) {
    unsigned sum = 0;
    for (int y = 0; y < q; y++) {
        const uint8_t *row = fd.ptr + (size_t)follow_clampi(cy + y, fd.rows - 1) * (size_t)fd.step;
        for (int x = 0; x < q; x++) {
            const uint8_t *p = row + (size_t)follow_clampi(cx + x, fd.cols - 1) * 3;
            sum += face_luma(p[0], p[1], p[2]);
        }
    }
    const unsigned n = (unsigned)(q * q);
    return (sum + n / 2u) / n;
}

// the key a candidate competes with: smaller wins
__host__ __device__ inline unsigned long long follow_key(unsigned sad, int du, int dv, int R) {
    return ((unsigned long long)sad << 32) | ((unsigned long long)(unsigned)(du * du + dv * dv) << 16) |
           (unsigned long long)(unsigned)((dv + R) * (2 * R + 1) + du + R);
}
constexpr unsigned long long kFollowNoKey = ~0ull;
__host__ __device__ inline void follow_key_decode(unsigned long long key, int R, int *sad, int *du, int *dv) {
    const int idx = (int)(key & 0xFFFFull);
    *sad = (int)(key >> 32);
    *dv = idx / (2 * R + 1) - R;
    *du = idx % (2 * R + 1) - R;
}

// a candidate may win only if the centre of the moved lattice lies inside the frame
__host__ __device__ inline bool follow_eligible(int ox, int oy, int q, int du, int dv, int rows, int cols) {
    const int cx = ox + du * q + (kFollowG / 2) * q, cy = oy + dv * q + (kFollowG / 2) * q;
    return cx >= 0 && cx < cols && cy >= 0 && cy < rows;
}

__host__ __device__ inline bool follow_frame_empty(const FollowFrame &fd) { return fd.ptr == nullptr || fd.rows <= 0 || fd.cols <= 0; }

// what a search says about one slot: state 0 = not attempted, 1 = attempted, no eligible candidate, 2 = (sad, du, dv) is the winner
struct FollowResult {
    int32_t state, sad, du, dv;
};

// a slot is searched when its record is valid, its run is not used up and the frame has pixels
__host__ __device__ inline bool follow_attempted(const rf_track_follow &r, int max_run, const FollowFrame &fd) {
    return r.valid != 0 && r.run < max_run && !follow_frame_empty(fd);
}

// Host: the template of a lattice, G x G bytes
inline void follow_template(const FollowFrame &fd, int q, int ox, int oy, uint8_t *tpl) {
    for (int j = 0; j < kFollowG; j++)
        for (int i = 0; i < kFollowG; i++) tpl[j * kFollowG + i] = (uint8_t)follow_cell(fd, ox + i * q, oy + j * q, q);
}

// Host: the search of one slot, sequential.  tpl: G x G bytes.
inline FollowResult follow_search(const FollowFrame &fd, const uint8_t *tpl, int q, int ox, int oy, int R) {
    const int Wc = kFollowG + 2 * R;
    uint8_t win[kFollowWin * kFollowWin];
    for (int j = 0; j < Wc; j++)
        for (int i = 0; i < Wc; i++) win[j * Wc + i] = (uint8_t)follow_cell(fd, ox + (i - R) * q, oy + (j - R) * q, q);
    unsigned long long best = kFollowNoKey;
    for (int dv = -R; dv <= R; dv++)
        for (int du = -R; du <= R; du++) {
            if (!follow_eligible(ox, oy, q, du, dv, fd.rows, fd.cols)) continue;
            unsigned sad = 0;
            for (int j = 0; j < kFollowG; j++)
                for (int i = 0; i < kFollowG; i++) {
                    const int a = tpl[j * kFollowG + i], b = win[(j + dv + R) * Wc + i + du + R];
                    sad += (unsigned)(a > b ? a - b : b - a);
                }
            const unsigned long long key = follow_key(sad, du, dv, R);
            if (key < best) best = key;
        }
    FollowResult r = {1, -1, 0, 0};
    if (best != kFollowNoKey) { r.state = 2; follow_key_decode(best, R, &r.sad, &r.du, &r.dv); }
    return r;
}

__host__ __device__ inline bool follow_accepted(const FollowResult &r, int max_mad) { return r.state == 2 && r.sad <= max_mad * kFollowCells; }

// an accepted search moves the track's last face and the slot's lattice by whole cells
__host__ __device__ inline void follow_move(rf_face *last, rf_track_follow *rec, const FollowResult &r) {
#pragma clang fp contract(off)
    const int mx = r.du * rec->q, my = r.dv * rec->q;
    const float fx = (float)mx, fy = (float)my;
    last->x1 = last->x1 + fx; last->x2 = last->x2 + fx;
    last->y1 = last->y1 + fy; last->y2 = last->y2 + fy;
    for (int i = 0; i < 5; i++) { last->px[i] = last->px[i] + fx; last->py[i] = last->py[i] + fy; }
    rec->ox += mx; rec->oy += my;
    rec->run += 1;
    rec->sad = r.sad; rec->dx = mx; rec->dy = my;
}

// a slot that was not moved: its record says why (the winner's SAD, or -1 without one)
__host__ __device__ inline void follow_reject(rf_track_follow *rec, const FollowResult &r) {
    rec->sad = r.state == 2 ? r.sad : -1;
    rec->dx = 0; rec->dy = 0;
}

__host__ __device__ inline rf_track_follow follow_record_zero() {
    rf_track_follow z;
    z.valid = z.run = z.q = z.ox = z.oy = z.sad = z.dx = z.dy = 0;
    return z;
}
__host__ __device__ inline rf_track_follow follow_record_key(const FollowGeom &g) {
    rf_track_follow r = follow_record_zero();
    if (g.valid) { r.valid = 1; r.q = g.q; r.ox = g.ox; r.oy = g.oy; }
    return r;
}

// Host: a key step, sequential.  track_step's arguments plus the frame, max_tracks records and max_tracks x 1024 template bytes.  A
// frame without pixels has no faces.
inline int track_step_follow_key(const TrackSpec &sp, rf_track *table, rf_track_follow *records, uint8_t *templates, int64_t *frames,
                                 int64_t *next_id, const FollowFrame &fd, const float *faces, int stride_floats, int m, float scale,
                                 const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_count) {
    if (follow_frame_empty(fd)) m = 0;
    const int st = track_step(sp, table, frames, next_id, faces, stride_floats, m, scale, quality, tags, ended, cap_ended, ended_count);
    for (int s = 0; s < sp.max_tracks; s++)
        if (table[s].id == 0) records[s] = follow_record_zero();
    for (int k = 0; k < m; k++) {
        const int s = tags[k].slot;
        if (s < 0 || s >= sp.max_tracks || (tags[k].flags & RF_TRACK_UNTRACKED)) continue;
        const FollowGeom g = follow_geometry(&table[s].last.x1);
        records[s] = follow_record_key(g);
        if (g.valid) follow_template(fd, g.q, g.ox, g.oy, templates + (size_t)s * kFollowCells);
    }
    return st;
}

// Host: a follow step, sequential.  out / tags: the first min(*count, cap) accepted slots in ascending order; *count the true number.
inline int track_step_follow(const TrackSpec &sp, const FollowSpec &fs, rf_track *table, rf_track_follow *records, const uint8_t *templates,
                             int64_t *frames, const FollowFrame &fd, rf_face *out, rf_track_tag *tags, int cap, int *count, rf_track *ended,
                             int cap_ended, int *ended_count) {
    const long long f = *frames;
    *frames = f + 1;
    int n_out = 0, n_ended = 0;
    for (int s = 0; s < sp.max_tracks; s++) {
        rf_track &t = table[s];
        if (t.id == 0) continue;
        FollowResult r = {0, -1, 0, 0};
        if (follow_attempted(records[s], fs.max_run, fd))
            r = follow_search(fd, templates + (size_t)s * kFollowCells, records[s].q, records[s].ox, records[s].oy, fs.radius);
        if (follow_accepted(r, fs.max_mad)) {
            follow_move(&t.last, &records[s], r);
            if (n_out < cap) { out[n_out] = t.last; tags[n_out] = track_tag(&t, s, f, sp.min_hits, RF_TRACK_FOLLOWED); }
            n_out++;
            continue;
        }
        follow_reject(&records[s], r);
        if (!track_age(&t, sp.max_missed)) continue;
        if (n_ended < cap_ended && ended) ended[n_ended] = t;
        n_ended++;
        memset(&t, 0, sizeof(t));
        records[s] = follow_record_zero();
    }
    if (count) *count = n_out;
    if (ended_count) *ended_count = n_ended;
    return (n_out > cap ? kTrackOverflow : 0) | (n_ended > cap_ended ? kTrackEndedCut : 0);
}

}  // namespace rf
