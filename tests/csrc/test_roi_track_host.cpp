// Host-only test of tracked region detection in retinaface_amd/csrc/roi.h (with track.h and motion.h), meant to run under
// -fsanitize=address,undefined (tests/test_roi_track_host.py::test_cells_and_void_atlases_under_address_and_ub_sanitizers): random
// tables -- free slots, boxes of every size in and around the frame, extreme floats (NaN, infinities, +-3e38, beyond +-2^20, inverted
// boxes), velocities up to +-1e30 with any sample count and missed count -- planned into exactly-sized cell buffers: a record written
// past max_tracks is a sanitizer report, an overflow in the fp64 -> int32 conversions or the origin arithmetic a UBSan report.  Every
// cell is checked against its definition: void (all zero, flags RF_ROI_VOID) exactly for the free slots and the boxes roi_from_face
// refuses, else roi_plan of roi_from_face of the box the next step matches against.  Then atlases whose cells mix void and real
// records go from pitched sources into pitched destinations in exactly-sized heap buffers (a void cell is zeros and reads nothing),
// and faces whose centres fall in void cells are dropped.  No GPU, no library: the headers are compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_roi_track_host tests/csrc/test_roi_track_host.cpp && ./test_roi_track_host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/roi.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static bool is_void(const rf::RoiCell &c) {
    return c.roi.x == 0 && c.roi.y == 0 && c.roi.w == 0 && c.roi.h == 0 && c.level == 0 && c.x0 == 0 && c.y0 == 0 && c.flags == RF_ROI_VOID;
}

static float pick(std::mt19937 &rng, bool extreme) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float wild[] = {nan, inf, -inf, 3e38f, -3e38f, 1e9f, -1e9f, 1048576.f, 1048577.f, -1048576.f, -1048577.f, 2e6f, 0.f, -0.f, 1e-30f};
    if (extreme) return wild[rng() % (sizeof(wild) / sizeof(wild[0]))];
    return (float)((int)(rng() % 8000) - 2000) * 0.25f;
}

static int table_case(int T, int grid, int net, int max_zoom, int margin_q8, bool with_motion, std::mt19937 &rng) {
    const int cw = net / grid, ch = net / grid;
    // exactly-sized heap buffers: slot T of any of them is outside
    std::unique_ptr<rf_track[]> table(new rf_track[T]);
    std::unique_ptr<rf_track_motion[]> motion(new rf_track_motion[T]);
    std::unique_ptr<rf::RoiCell[]> cells(new rf::RoiCell[T]);
    memset((void *)table.get(), 0, sizeof(rf_track) * T);
    memset((void *)motion.get(), 0, sizeof(rf_track_motion) * T);
    memset((void *)cells.get(), 0x77, sizeof(rf::RoiCell) * T);
    const rf::MotionSpec ms = {0.5f, (int)(rng() % 4) == 0 ? 0 : (int)(rng() % 9)};
    int voids = 0;
    for (int s = 0; s < T; s++) {
        rf_track &t = table[s];
        if (rng() % 4 == 0) continue;                                  // a free slot
        t.id = 1 + (long long)(rng() % 1000);
        t.missed = (int)(rng() % 5);
        const bool extreme = rng() % 5 == 0;
        const float x = pick(rng, extreme), y = pick(rng, extreme && (rng() & 1));
        const float w = extreme && (rng() & 1) ? pick(rng, true) : (float)(rng() % 700) * 0.5f - (rng() % 16 == 0 ? 40.f : 0.f);
        t.last.score = 0.9f; t.last.x1 = x; t.last.y1 = y; t.last.x2 = x + w; t.last.y2 = y + w * 1.25f;
        if (with_motion) {
            const float big[] = {0.f, 1.f, -3.5f, 1e30f, -1e30f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
            motion[s].vx = big[rng() % 7]; motion[s].vy = big[rng() % 3];
            motion[s].samples = (int)(rng() % 3);
        }
    }
    rf::roi_cells_from_tracks(table.get(), with_motion ? motion.get() : nullptr, ms, T, margin_q8, cw, ch, max_zoom, cells.get());
    for (int s = 0; s < T; s++) {
        const rf_track &t = table[s];
        const rf::RoiCell &c = cells[s];
        if (t.id == 0) { CHECK(is_void(c)); voids++; continue; }
        float f[5] = {0.f, t.last.x1, t.last.y1, t.last.x2, t.last.y2};
        if (with_motion) {
            const float last[4] = {t.last.x1, t.last.y1, t.last.x2, t.last.y2};
            rf::motion_predict_box(last, motion[s].vx, motion[s].vy, motion[s].samples, rf::motion_frames_ahead(t.missed, 1, ms.horizon), f + 1);
        }
        rf_roi r;
        if (!rf::roi_from_face(f, 1.f, margin_q8 ? margin_q8 : 64, &r)) { CHECK(is_void(c)); voids++; continue; }
        CHECK(rf::roi_valid(r));
        const rf::RoiCell want = rf::roi_plan(r, cw, ch, max_zoom);
        CHECK(memcmp(&want, &c, sizeof(c)) == 0 && !(c.flags & RF_ROI_VOID));
        // the region holds the box it was made from
        CHECK((double)r.x <= (double)f[1] && (double)r.y <= (double)f[2]);
        if (r.w < rf::kRoiMaxSide) CHECK((double)r.x + r.w >= (double)f[3]);
    }
    return voids;
}

static void atlas_case(int grid, int view_w, int view_h, int rows, int cols, int src_pad, int dst_pad, std::mt19937 &rng) {
    const int step = cols * 3 + src_pad, dstep = view_w * 3 + dst_pad, cw = view_w / grid, ch = view_h / grid, GG = grid * grid;
    std::vector<uint8_t> src((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &b : src) b = (uint8_t)(1 + rng() % 255);                // no zero byte: a zero pixel of the view was not read from the frame
    std::unique_ptr<rf::RoiCell[]> cells(new rf::RoiCell[GG]);
    for (int k = 0; k < GG; k++) {
        if ((rng() & 1) || k == 0) { cells[k] = rf::roi_void_cell(); continue; }
        const rf_roi r = {(int)(rng() % (unsigned)cols) - 4, (int)(rng() % (unsigned)rows) - 4, 1 + (int)(rng() % (unsigned)(2 * cols)), 1 + (int)(rng() % (unsigned)(2 * rows))};
        cells[k] = rf::roi_plan(r, cw, ch, 1 << (rng() % 3));
    }
    std::vector<uint8_t> dst((size_t)(view_h - 1) * dstep + (size_t)view_w * 3, 0xAB);
    rf::roi_atlas_host(src.data(), rows, cols, step, cells.get(), GG, grid, view_w, view_h, dst.data(), dstep);
    for (int y = 0; y + 1 < view_h; y++)
        for (int b = view_w * 3; b < dstep; b++) CHECK(dst[(size_t)y * dstep + b] == 0xAB);
    const rf::RoiEntry e{0, 0, rows, cols, grid, GG, view_w, view_h, cells.get()};
    for (int k = 0; k < GG; k++) {
        const int ox = (k % grid) * cw, oy = (k / grid) * ch;
        if (!rf::roi_cell_is_void(cells[k])) continue;
        for (int j = 0; j < ch; j++)
            for (int i = 0; i < 3 * cw; i++) CHECK(dst[(size_t)(oy + j) * dstep + 3 * ox + i] == 0);
        // faces whose centres fall in the void cell: its middle, its first pixel, the last float below its right and lower borders
        const float xs[] = {ox + cw / 2.f, (float)ox, std::nextafterf((float)(ox + cw), 0.f)}, ys[] = {oy + ch / 2.f, (float)oy, std::nextafterf((float)(oy + ch), 0.f)};
        for (int a = 0; a < 3; a++) {
            float f[15], o[15];
            for (int i = 0; i < 15; i++) f[i] = (i == 1 || i == 3 || (i >= 5 && i < 10)) ? xs[a] : ys[a];
            f[0] = 0.5f;
            int region = -1;
            CHECK(!rf::roi_map_face(e, f, o, &region) && region == -1);
        }
    }
}

int main() {
    std::mt19937 rng(20261021);
    int tables = 0, voids = 0;
    const int Ts[] = {1, 2, 16, 17, 64, 256}, grids[] = {1, 2, 4}, margins[] = {0, 1, 64, 640, 65535};
    for (int T : Ts)
        for (int g : grids)
            for (int rep = 0; rep < 6; rep++) {
                voids += table_case(T, g, 448, 1 << (rng() % 3), margins[rng() % 5], (rep & 1) != 0, rng);
                tables++;
            }
    const int views[][3] = {{2, 32, 16}, {4, 64, 48}, {4, 448, 448}}, sources[][2] = {{1, 1}, {2, 3}, {63, 65}, {129, 131}};
    int atlases = 0;
    for (auto &v : views)
        for (auto &s : sources)
            for (int rep = 0; rep < (v[1] > 64 ? 2 : 8); rep++) {
                atlas_case(v[0], v[1], v[2], s[0], s[1], 0, 0, rng);
                atlas_case(v[0], v[1], v[2], s[0], s[1], 7, 5, rng);
                atlases += 2;
            }
    CHECK(voids > 100);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok: %d tables (%d void cells), %d atlases\n", tables, voids, atlases);
    return 0;
}
