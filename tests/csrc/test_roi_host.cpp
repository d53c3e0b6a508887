// Host-only test of retinaface_amd/csrc/roi.h, meant to run under -fsanitize=address,undefined
// (tests/test_roi_host.py::test_plan_atlas_and_map_under_address_and_ub_sanitizers): a few hundred random plans -- regions of every size
// from 1 x 1 to 16384 x 16384 at origins out to +-2^20, inside, over the edges of and far outside sources of 1 x 1, 2 x 3, 63 x 65 and
// 129 x 131 pixels -- whose atlases go from pitched sources into pitched destinations in exactly-sized heap buffers: a byte read
// outside a source row's cols * 3 bytes or written outside a view row's view_w * 3 bytes is a sanitizer report, an overflow in the
// origin arithmetic a UBSan report.  Every plan is checked against its definition (the level fits, the next larger does not, the cell
// is centred), x1 cells against the frame itself, and roi_map_face at the extremes (NaN, infinities, +-1e9) and on faces that sit in
// their regions, which come back.  No GPU, no library: the header is compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_roi_host tests/csrc/test_roi_host.cpp && ./test_roi_host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/roi.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static rf_roi random_roi(std::mt19937 &rng, int rows, int cols, int kind) {
    rf_roi r;
    const int sides[] = {1, 2, 3, 7, 16, 28, 29, 56, 57, 112, 113, 224, 225, 448, 449, 1000, 16384};
    r.w = sides[rng() % 17]; r.h = sides[rng() % 17];
    switch (kind) {
    case 0: r.x = (int)(rng() % (unsigned)(cols + 60)) - 30; r.y = (int)(rng() % (unsigned)(rows + 60)) - 30; break;      // around the frame
    case 1: r.x = (rng() & 1) ? rf::kRoiMaxOrigin : -rf::kRoiMaxOrigin; r.y = (rng() & 1) ? rf::kRoiMaxOrigin : -rf::kRoiMaxOrigin; break;
    case 2: r.x = -r.w / 2; r.y = rows - r.h / 2; break;                                                                   // over a corner
    default: r.x = (int)(rng() % 4001) - 2000; r.y = (int)(rng() % 4001) - 2000; break;
    }
    return r;
}

static void check_plan(const rf_roi &r, const rf::RoiCell &c, int cw, int ch, int max_zoom) {
    CHECK(c.level >= -2 && c.level <= 2 && (c.level <= 0 || (1 << c.level) <= max_zoom));
    const auto fits = [&](int l) { return l >= 0 ? ((long long)r.w << l) <= cw && ((long long)r.h << l) <= ch : r.w <= ((long long)cw << -l) && r.h <= ((long long)ch << -l); };
    if (c.flags & RF_ROI_CROPPED) CHECK(c.level == -2 && !fits(-2));
    else {
        CHECK(fits(c.level));
        if (c.level < 2 && (c.level < 0 || (2 << c.level) <= max_zoom)) CHECK(!fits(c.level + 1));
    }
    // the region's centre, in level pixels, is within one pixel of the cell's centre
    const double z = c.level >= 0 ? (double)(1 << c.level) : 1.0 / (1 << -c.level);
    CHECK(std::fabs((r.x + r.w / 2.0) * z - (c.x0 + cw / 2.0)) <= 1.0);
    CHECK(std::fabs((r.y + r.h / 2.0) * z - (c.y0 + ch / 2.0)) <= 1.0);
}

static void atlas_case(int grid, int view_w, int view_h, int rows, int cols, int src_pad, int dst_pad, int max_zoom, std::mt19937 &rng) {
    const int step = cols * 3 + src_pad, dstep = view_w * 3 + dst_pad, cw = view_w / grid, ch = view_h / grid, GG = grid * grid;
    CHECK(rf::roi_check_view(view_w, view_h, grid) == nullptr);
    // the last row ends with its pixels: no padding behind it, so a read past cols * 3 of the last row leaves the buffer
    std::vector<uint8_t> src((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &b : src) b = (uint8_t)rng();
    const int used = 1 + (int)(rng() % (unsigned)GG);
    std::vector<rf::RoiCell> cells;
    for (int k = 0; k < used; k++) {
        const rf_roi r = random_roi(rng, rows, cols, (int)(rng() % 4));
        CHECK(rf::roi_valid(r));
        cells.push_back(rf::roi_plan(r, cw, ch, max_zoom));
        check_plan(r, cells.back(), cw, ch, max_zoom);
    }
    std::vector<uint8_t> dst((size_t)(view_h - 1) * dstep + (size_t)view_w * 3, 0xAB);
    rf::roi_atlas_host(src.data(), rows, cols, step, cells.data(), used, grid, view_w, view_h, dst.data(), dstep);
    for (int y = 0; y + 1 < view_h; y++)
        for (int b = view_w * 3; b < dstep; b++) CHECK(dst[(size_t)y * dstep + b] == 0xAB);
    for (int k = 0; k < GG; k++) {
        const int ox = (k % grid) * cw, oy = (k / grid) * ch;
        for (int j = 0; j < ch; j += 3)
            for (int i = 0; i < cw; i += 5) {
                const uint8_t *p = &dst[(size_t)(oy + j) * dstep + 3 * (ox + i)];
                if (k >= used) { CHECK(p[0] == 0 && p[1] == 0 && p[2] == 0); continue; }
                if (cells[k].level != 0) continue;
                const int X = cells[k].x0 + i, Y = cells[k].y0 + j;                     // x1: the frame itself, or 0 outside it
                const bool in = X >= 0 && Y >= 0 && X < cols && Y < rows;
                for (int c = 0; c < 3; c++) CHECK(p[c] == (in ? src[(size_t)Y * step + 3 * X + c] : 0));
            }
    }
    // faces through the same cells: the extremes, and one per region that sits on its centre and comes back inside it
    const rf::RoiEntry e{0, 3, rows, cols, grid, used, view_w, view_h, cells.data()};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float vals[] = {0.f, -16.f, (float)view_w, (float)view_w + 0.5f, 1e9f, -1e9f, 3e38f, -3e38f, inf, -inf, nan, 0.3f, (float)(view_h - 1), 55.5f};
    for (size_t a = 0; a < sizeof(vals) / sizeof(vals[0]); a++) {
        float f[15], o[15];
        for (int i = 0; i < 15; i++) f[i] = vals[(a + (size_t)i * 5) % (sizeof(vals) / sizeof(vals[0]))];
        f[0] = 0.75f;
        int region = -1;
        if (!rf::roi_map_face(e, f, o, &region)) continue;
        CHECK(o[0] == 0.75f && region >= 3 * GG && region < 3 * GG + used);
    }
    for (int k = 0; k < used; k++) {
        if (cells[k].flags & RF_ROI_CROPPED) continue;
        if (cells[k].roi.w < 8 || cells[k].roi.h < 8) continue;      // a cell pixel of a shrunk level spans up to 4 source pixels: a thinner region may miss it
        const float cx = (float)((k % grid) * cw) + cw / 2.f, cy = (float)((k / grid) * ch) + ch / 2.f;
        float f[15], o[15];
        for (int i = 0; i < 15; i++) f[i] = (i == 1 || i == 3 || (i >= 5 && i < 10)) ? cx : cy;
        f[0] = 0.5f; f[1] = cx - 0.25f; f[3] = cx + 0.25f; f[2] = cy - 0.25f; f[4] = cy + 0.25f;
        int region = -1;
        const bool kept = rf::roi_map_face(e, f, o, &region);
        if (std::abs(cells[k].roi.x) > 100000 || std::abs(cells[k].roi.y) > 100000) continue;      // fp32 spacing beyond 2^17 px: the centre may round out
        CHECK(kept && region == 3 * GG + k);
        if (kept) CHECK(o[1] >= (float)cells[k].roi.x - 4.f && o[3] <= (float)(cells[k].roi.x + cells[k].roi.w) + 4.f);
    }
}

static void from_face_case(std::mt19937 &rng) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float vals[] = {0.f, 10.5f, -3.25f, 400.f, 1e6f, -1e6f, 2e6f, 1e9f, -1e9f, 3e38f, inf, -inf, nan, 16383.f, 20000.f};
    const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
    for (int t = 0; t < 400; t++) {
        float f[15] = {0.9f};
        for (int i = 1; i < 5; i++) f[i] = vals[rng() % nv];
        rf_roi r;
        const float scale = (rng() & 1) ? 1.f : 2.857f;
        const int mq = (int)(rng() % 3) * 128;
        if (rf::roi_from_face(f, scale, mq ? mq : 64, &r)) CHECK(rf::roi_valid(r));
    }
    float f[15] = {0.9f, 10.5f, 20.25f, 50.5f, 70.25f};
    rf_roi r;
    CHECK(rf::roi_from_face(f, 1.f, 64, &r) && r.x == -2 && r.y == 7 && r.w == 65 && r.h == 76);
}

int main() {
    std::mt19937 rng(20261021);
    const int views[][3] = {{2, 32, 16}, {4, 64, 48}, {1, 16, 9}, {4, 448, 448}, {2, 448, 448}}, sources[][2] = {{1, 1}, {2, 3}, {63, 65}, {129, 131}};
    int plans = 0;
    for (auto &v : views)
        for (auto &s : sources)
            for (int rep = 0; rep < (v[1] > 64 ? 3 : 12); rep++) {
                const int mz = 1 << (rng() % 3);
                atlas_case(v[0], v[1], v[2], s[0], s[1], 0, 0, mz, rng);
                atlas_case(v[0], v[1], v[2], s[0], s[1], 7, 5, mz, rng);
                plans += 2;
            }
    from_face_case(rng);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok: %d atlases\n", plans);
    return 0;
}
