// Host-only test of retinaface_amd/csrc/motion.h (and track.h under it), meant to run under -fsanitize=address,undefined
// (tests/test_motion_host.py::test_host_step_under_address_and_ub_sanitizers): a few hundred seeded random frames -- walkers that move,
// vanish and come back, empty frames, tables of 1, 5, 64 and 256 slots that overflow, non-finite boxes -- go through
// track_step_motion with exactly-sized heap buffers, and every live track's predicted face is formed.  A negative horizon must leave
// the bytes of track_step.  No GPU, no library: the headers are compiled into the program.
//   clang++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//           -o test_motion_host tests/csrc/test_motion_host.cpp && ./test_motion_host
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/motion.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Walker { float x, y, vx, vy, size; int hidden; };

static rf_face make_face(float score, float x, float y, float w) {
    rf_face f;
    f.score = score; f.x1 = x; f.y1 = y; f.x2 = x + w; f.y2 = y + 1.2f * w;
    for (int i = 0; i < 5; i++) { f.px[i] = x + 0.2f * (float)i * w; f.py[i] = y + 0.25f * (float)i * w; }
    return f;
}

static void run(unsigned seed, int max_tracks, int max_missed, float alpha, int horizon, int n_people, int n_frames) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    rf_track_spec ts = {sizeof(rf_track_spec), max_tracks, 0.f, max_missed, 2, 0.f};
    rf_motion_spec mspec = {sizeof(rf_motion_spec), alpha, horizon, 0};
    rf::TrackSpec sp;
    rf::MotionSpec ms;
    CHECK(rf::track_spec_resolve(&ts, &sp) == nullptr && rf::motion_spec_resolve(&mspec, &ms) == nullptr);
    const int T = sp.max_tracks;
    std::vector<rf_track> table((size_t)T), plain((size_t)T);
    std::vector<rf_track_motion> motion((size_t)T);
    memset((void *)table.data(), 0, table.size() * sizeof(rf_track));
    memset((void *)plain.data(), 0, plain.size() * sizeof(rf_track));
    memset((void *)motion.data(), 0, motion.size() * sizeof(rf_track_motion));
    int64_t frames = 0, next_id = 1, pframes = 0, pnext = 1;
    std::vector<Walker> people((size_t)n_people);
    for (Walker &w : people) w = Walker{600.f * u(rng), 600.f * u(rng), 28.f * u(rng) - 14.f, 28.f * u(rng) - 14.f, 24.f + 66.f * u(rng), 0};
    for (int t = 0; t < n_frames; t++) {
        std::vector<rf_face> faces;
        for (Walker &w : people) {
            w.x += w.vx; w.y += w.vy;
            if (w.hidden == 0 && u(rng) < 0.12f) w.hidden = 1 + (int)(u(rng) * 4.f);
            if (w.hidden > 0) { w.hidden--; continue; }
            faces.push_back(make_face(0.5f + 0.5f * u(rng), w.x, w.y, w.size));
        }
        if (t % 37 == 36) faces.clear();
        if (t % 41 == 7 && !faces.empty()) faces[0].x2 = std::numeric_limits<float>::infinity();
        if (t % 43 == 9 && !faces.empty()) faces[0].y1 = std::numeric_limits<float>::quiet_NaN();
        if (t % 47 == 11) faces.push_back(make_face(0.4f, 1.2e38f, 0.f, 1.2e38f));           // x1 + x2 overflows
        const int m = (int)faces.size();
        // score order is the caller's business; the step does not depend on it being sorted
        std::vector<rf_track_tag> tags((size_t)m), ptags((size_t)m);
        const int cap_ended = t % 3;                                                          // 0: no ended buffer at all
        std::vector<rf_track> ended((size_t)cap_ended), pended((size_t)cap_ended);
        int ne = -1, pne = -1;
        const float scale = t % 5 == 4 ? 1.5f : 1.f;
        const int st = rf::track_step_motion(sp, ms, table.data(), motion.data(), &frames, &next_id, (const float *)faces.data(), 15, m, scale,
                                             nullptr, tags.data(), cap_ended ? ended.data() : nullptr, cap_ended, &ne);
        CHECK(ne >= 0 && (st & ~(rf::kTrackOverflow | rf::kTrackEndedCut)) == 0);
        for (int s = 0; s < T; s++) {
            if (table[(size_t)s].id == 0) {
                CHECK(motion[(size_t)s].vx == 0.f && motion[(size_t)s].vy == 0.f && motion[(size_t)s].samples == 0);
                continue;
            }
            CHECK(rf::track_finite(motion[(size_t)s].vx) && rf::track_finite(motion[(size_t)s].vy));
            for (int ahead = 0; ahead < 2; ahead++) {
                rf_face out;
                const int h = rf::motion_frames_ahead(table[(size_t)s].missed, ahead, ms.horizon);
                CHECK(h >= 0 && h <= (ms.horizon > 0 ? ms.horizon : 0));
                rf::motion_predict_face(&table[(size_t)s].last, &motion[(size_t)s], h, &out);
                if (h == 0 || motion[(size_t)s].samples == 0) CHECK(memcmp(&out, &table[(size_t)s].last, sizeof(rf_face)) == 0);
            }
        }
        if (horizon < 0) {                                                                    // the plain tracker's bytes
            const int pst = rf::track_step(sp, plain.data(), &pframes, &pnext, (const float *)faces.data(), 15, m, scale, nullptr, ptags.data(),
                                           cap_ended ? pended.data() : nullptr, cap_ended, &pne);
            CHECK(pst == st && pne == ne && pframes == frames && pnext == next_id);
            CHECK(memcmp(table.data(), plain.data(), table.size() * sizeof(rf_track)) == 0);
            if (m) CHECK(memcmp(tags.data(), ptags.data(), (size_t)m * sizeof(rf_track_tag)) == 0);
            const int have = ne < cap_ended ? ne : cap_ended;
            if (have) CHECK(memcmp(ended.data(), pended.data(), (size_t)have * sizeof(rf_track)) == 0);
        }
    }
    CHECK(frames == n_frames && next_id > 1);
}

int main() {
    run(1, 64, 2, 0.5f, 8, 12, 120);
    run(2, 1, 1, 1.0f, 1, 3, 80);
    run(3, 5, -1, 0.3f, 3, 9, 120);
    run(4, 256, 4, 0.f, 0, 250, 60);
    run(5, 64, 3, 0.5f, -1, 20, 120);
    run(6, 8, 0, 1.0f, 65536, 14, 100);
    // the spec's refusals
    rf::MotionSpec ms;
    rf_motion_spec bad = {sizeof(rf_motion_spec), 0.5f, 8, 1};
    CHECK(rf::motion_spec_resolve(&bad, &ms) != nullptr);
    bad.reserved = 0; bad.horizon = 65537;
    CHECK(rf::motion_spec_resolve(&bad, &ms) != nullptr);
    bad.horizon = 8; bad.alpha = std::numeric_limits<float>::quiet_NaN();
    CHECK(rf::motion_spec_resolve(&bad, &ms) != nullptr);
    CHECK(rf::motion_spec_resolve(nullptr, &ms) == nullptr && ms.alpha == 0.5f && ms.horizon == 8);
    // missed counts at the end of int: no overflow in the frames ahead or in dt
    CHECK(rf::motion_frames_ahead(2147483647, 1, 65536) == 65536 && rf::motion_frames_ahead(2147483647, 1, 0) == 0);
    float vx = 1.f, vy = 1.f;
    int samples = 1 << 30;
    const float a[4] = {0.f, 0.f, 10.f, 10.f}, b[4] = {4.f, 4.f, 14.f, 14.f};
    rf::motion_update(&vx, &vy, &samples, b, a, 2147483647, 0.5f);
    CHECK(samples == 1 << 30 && rf::track_finite(vx));
    std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
