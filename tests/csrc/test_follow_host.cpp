// Host-only test of retinaface_amd/csrc/follow.h (and track.h under it), meant to run under -fsanitize=address,undefined
// (tests/test_follow_host.py::test_host_steps_under_address_and_ub_sanitizers): a few hundred seeded random key and follow steps --
// walkers over frames of several shapes whose rows have slack and whose first byte sits at an odd address, boxes over every edge,
// larger than the frame, non-finite and far outside, empty frames, every radius -- with frames, tables, records, templates and the
// output and ended lists in exactly-sized heap buffers, so a read outside a frame or a write past a list is an error here.  No GPU, no
// library: the headers are compiled into the program.
//   clang++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//           -o test_follow_host tests/csrc/test_follow_host.cpp && ./test_follow_host
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/follow.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Walker { float x, y, vx, vy, size; };

static rf_face make_face(float score, float x, float y, float w) {
    rf_face f;
    f.score = score; f.x1 = x; f.y1 = y; f.x2 = x + w; f.y2 = y + 1.2f * w;
    for (int i = 0; i < 5; i++) { f.px[i] = x + 0.2f * (float)i * w; f.py[i] = y + 0.25f * (float)i * w; }
    return f;
}

// a frame in a heap buffer of exactly offset + (rows - 1) * step + cols * 3 bytes: one byte more would be outside it
struct Frame {
    std::vector<uint8_t> buf;
    rf::FollowFrame fd;
    Frame(std::mt19937 &rng, int rows, int cols, int slack, int shift) {
        const int step = cols * 3 + slack;
        buf.resize(1 + (size_t)(rows - 1) * step + (size_t)cols * 3);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols * 3; x++) buf[1 + (size_t)y * step + x] = (uint8_t)(((x / 3 + shift) * 7 + y * 5 + (int)(rng() & 15)) & 255);
        fd = rf::FollowFrame{buf.data() + 1, rows, cols, step};
    }
};

static void run(unsigned seed, int rows, int cols, int max_tracks, int max_missed, int radius, int max_mad, int max_run, int n_people, int n_frames) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    rf_track_spec ts = {sizeof(rf_track_spec), max_tracks, 0.f, max_missed, 2, 0.f};
    rf_follow_spec fspec = {sizeof(rf_follow_spec), radius, max_mad, max_run, 0};
    rf::TrackSpec sp;
    rf::FollowSpec fs;
    CHECK(rf::track_spec_resolve(&ts, &sp) == nullptr && rf::follow_spec_resolve(&fspec, &fs) == nullptr);
    const int T = sp.max_tracks;
    std::vector<rf_track> table((size_t)T);
    std::vector<rf_track_follow> records((size_t)T);
    std::vector<uint8_t> templates((size_t)T * rf::kFollowCells);
    memset((void *)table.data(), 0, table.size() * sizeof(rf_track));
    memset((void *)records.data(), 0, records.size() * sizeof(rf_track_follow));
    int64_t frames = 0, next_id = 1;
    std::vector<Walker> people((size_t)n_people);
    for (Walker &w : people)
        w = Walker{(float)cols * (1.4f * u(rng) - 0.2f), (float)rows * (1.4f * u(rng) - 0.2f), 6.f * u(rng) - 3.f, 6.f * u(rng) - 3.f, 8.f + 0.9f * (float)cols * u(rng) * u(rng)};
    for (int t = 0; t < n_frames; t++) {
        Frame frame(rng, rows, cols, t % 4 == 0 ? 0 : 1 + (int)(rng() % 9), t);
        const rf::FollowFrame none = {nullptr, 0, 0, 0};
        const rf::FollowFrame &fd = t % 29 == 28 ? none : frame.fd;
        const int cap_ended = t % 3;                                                          // 0: no ended buffer at all
        std::vector<rf_track> ended((size_t)cap_ended);
        int ne = -1;
        if (t % 4 == 0) {                                                                     // a key step
            std::vector<rf_face> faces;
            for (Walker &w : people) {
                w.x += 4.f * w.vx; w.y += 4.f * w.vy;
                if (u(rng) < 0.2f) continue;
                faces.push_back(make_face(0.5f + 0.5f * u(rng), w.x, w.y, w.size));
            }
            if (t % 16 == 4 && !faces.empty()) faces[0].x2 = std::numeric_limits<float>::infinity();
            if (t % 16 == 8 && !faces.empty()) faces[0].y1 = std::numeric_limits<float>::quiet_NaN();
            if (t % 16 == 12) faces.push_back(make_face(0.4f, -3.0e9f, 2.0e9f, 1.0e9f));      // clamped: far outside, no candidate is eligible
            if (t % 32 == 0) faces.push_back(make_face(0.45f, -30.f, -20.f, (float)cols + 80.f));   // larger than the frame
            const int m = (int)faces.size();
            std::vector<rf_track_tag> tags((size_t)m);
            const int st = rf::track_step_follow_key(sp, table.data(), records.data(), templates.data(), &frames, &next_id, fd,
                                                     (const float *)faces.data(), 15, m, 1.f, nullptr, tags.data(),
                                                     cap_ended ? ended.data() : nullptr, cap_ended, &ne);
            CHECK(ne >= 0 && (st & ~(rf::kTrackOverflow | rf::kTrackEndedCut)) == 0);
        } else {
            const int cap = t % 5 == 0 ? 0 : (t % 5 == 1 ? 1 : T);
            std::vector<rf_face> out((size_t)cap);
            std::vector<rf_track_tag> tags((size_t)cap);
            int count = -1;
            const int st = rf::track_step_follow(sp, fs, table.data(), records.data(), templates.data(), &frames, fd, cap ? out.data() : nullptr,
                                                 cap ? tags.data() : nullptr, cap, &count, cap_ended ? ended.data() : nullptr, cap_ended, &ne);
            CHECK(ne >= 0 && count >= 0 && count <= T && (st & ~(rf::kTrackOverflow | rf::kTrackEndedCut)) == 0);
            CHECK(((st & rf::kTrackOverflow) != 0) == (count > cap) && ((st & rf::kTrackEndedCut) != 0) == (ne > cap_ended));
            if (rf::follow_frame_empty(fd)) CHECK(count == 0);
            for (int j = 0; j < (count < cap ? count : cap); j++) CHECK((tags[(size_t)j].flags & RF_TRACK_FOLLOWED) && (j == 0 || tags[(size_t)j].slot > tags[(size_t)j - 1].slot));
        }
        for (int s = 0; s < T; s++) {
            const rf_track_follow &r = records[(size_t)s];
            if (table[(size_t)s].id == 0) { CHECK(r.valid == 0 && r.q == 0 && r.run == 0 && r.sad == 0); continue; }
            if (r.valid) CHECK(r.q >= 1 && r.q <= 385 && r.run >= 0 && r.run <= fs.max_run && r.sad >= -1 && r.sad <= 255 * rf::kFollowCells);
        }
    }
    CHECK(frames == n_frames);
}

int main() {
    run(1, 96, 128, 16, 2, 8, 40, 4, 10, 120);
    run(2, 37, 53, 1, 1, 1, 255, 1, 3, 80);
    run(3, 200, 240, 5, -1, 16, 16, 8, 9, 60);
    run(4, 64, 64, 256, 4, 3, 255, 65536, 40, 40);
    run(5, 1, 1, 8, 3, 16, 255, 3, 6, 60);
    run(6, 5, 300, 8, 0, 8, 100, 2, 8, 60);
    // the spec's defaults and refusals
    rf::FollowSpec fs;
    CHECK(rf::follow_spec_resolve(nullptr, &fs) == nullptr && fs.radius == 8 && fs.max_mad == 16 && fs.max_run == 8);
    rf_follow_spec bad = {sizeof(rf_follow_spec), 8, 16, 8, 1};
    CHECK(rf::follow_spec_resolve(&bad, &fs) != nullptr);
    bad.reserved = 0; bad.radius = 17;
    CHECK(rf::follow_spec_resolve(&bad, &fs) != nullptr);
    bad.radius = 16; bad.max_mad = 256;
    CHECK(rf::follow_spec_resolve(&bad, &fs) != nullptr);
    bad.max_mad = 255; bad.max_run = 65537;
    CHECK(rf::follow_spec_resolve(&bad, &fs) != nullptr);
    bad.max_run = 65536;
    CHECK(rf::follow_spec_resolve(&bad, &fs) == nullptr && fs.radius == 16 && fs.max_mad == 255 && fs.max_run == 65536);
    // the largest lattice: no overflow in the geometry, the key or the cell sum
    const float huge[4] = {-3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f};
    const rf::FollowGeom g = rf::follow_geometry(huge);
    CHECK(g.valid && g.q == 385 && g.ox == (-4096 + 8192 + 1 - 32 * 385) / 2 - 1);
    int sad, du, dv;
    rf::follow_key_decode(rf::follow_key(255u * rf::kFollowCells, -16, 16, 16), 16, &sad, &du, &dv);
    CHECK(sad == 255 * rf::kFollowCells && du == -16 && dv == 16);
    std::printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
