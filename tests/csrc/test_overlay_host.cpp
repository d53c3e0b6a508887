// Host-only test of retinaface_amd/csrc/overlay.h, meant to run under -fsanitize=address,undefined
// (tests/test_overlay_host.py::test_overlay_h_under_address_and_undefined_sanitizers): overlay_host_frame on noise frames held in
// exactly-sized heap buffers -- a dense frame, a 1 x 1 frame, a view at an odd pointer with a padded step between guard bytes --
// with regions across each of the four sides and corners, wholly outside, beyond the clamp, non-finite, with every spec extreme,
// against a naive per-pixel loop that follows the definition; and the pieces of a region against overlay_paint: every painted pixel
// lies in exactly one piece that holds its primitive, which is what lets the draw kernel write it from one thread.  No GPU, no
// library: the header is compiled into the program.
//   clang++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//           -o test_overlay_host tests/csrc/test_overlay_host.cpp && ./test_overlay_host
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/overlay.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Face { float v[15]; };

static Face face(float x1, float y1, float x2, float y2, float score = 0.9f) {
    Face f;
    const float w = x2 - x1, h = y2 - y1;
    const float fx[5] = {0.3f, 0.7f, 0.5f, 0.35f, 0.65f}, fy[5] = {0.35f, 0.35f, 0.55f, 0.75f, 0.75f};
    f.v[0] = score; f.v[1] = x1; f.v[2] = y1; f.v[3] = x2; f.v[4] = y2;
    for (int k = 0; k < 5; k++) { f.v[5 + k] = x1 + fx[k] * w; f.v[10 + k] = y1 + fy[k] * h; }
    return f;
}

// the definition, pixel by pixel, on a dense copy: for every pixel the first region that covers it paints it
static void naive(const rf::OverlaySpec &sp, std::vector<uint8_t> &dense, int rows, int cols, const std::vector<rf::OverlayRegion> &regs,
                  std::vector<int32_t> &pixels) {
    pixels.assign(regs.size(), 0);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++)
            for (size_t q = 0; q < regs.size(); q++) {
                const int code = rf::overlay_paint(sp, regs[q], x, y);
                if (!code) continue;
                const uint32_t c = rf::overlay_colour(sp, regs[q], code);
                uint8_t *p = &dense[((size_t)y * cols + x) * 3];
                for (int ch = 0; ch < 3; ch++) p[ch] = (uint8_t)((p[ch] * (255 - sp.alpha) + ((c >> (8 * ch)) & 255) * sp.alpha + 127) / 255);
                pixels[q]++;
                break;
            }
}

// every painted pixel of a region lies in exactly one piece that holds its primitive
static void check_pieces(const rf::OverlaySpec &sp, const rf::OverlayRegion &r) {
    if (!(r.flags & rf::kOverlayValid)) return;
    const int x0 = r.bx0 < -40 ? -40 : r.bx0, x1 = r.bx1 > 140 ? 140 : r.bx1, y0 = r.by0 < -40 ? -40 : r.by0, y1 = r.by1 > 140 ? 140 : r.by1;
    for (int y = y0 - 1; y <= y1 + 1; y++)
        for (int x = x0 - 1; x <= x1 + 1; x++) {
            const int code = rf::overlay_paint(sp, r, x, y);
            int holders = 0;
            for (int p = 0; p < rf::kOverlayPieces; p++) {
                int a, b, c, d;
                rf::overlay_piece_rect(sp, r, p, &a, &b, &c, &d);
                if (x >= a && x <= c && y >= b && y <= d && code && rf::overlay_piece_holds(p, code)) holders++;
            }
            if (holders != (code ? 1 : 0)) { CHECK(holders == (code ? 1 : 0)); return; }
        }
}

static void run(const rf::OverlaySpec &sp, int rows, int cols, size_t step, size_t lead, const std::vector<Face> &faces,
                const std::vector<long long> &ids, float scale, std::mt19937 &rng) {
    // the frame sits `lead` bytes into an exactly-sized buffer: the bytes before it, between its rows and after it are guards
    const size_t bytes = lead + (rows ? (size_t)(rows - 1) * step + (size_t)cols * 3 : 0);
    std::vector<uint8_t> buf(bytes);
    for (auto &b : buf) b = (uint8_t)rng();
    const std::vector<uint8_t> before = buf;
    std::vector<uint8_t> dense((size_t)rows * cols * 3);
    for (int y = 0; y < rows; y++) memcpy(&dense[(size_t)y * cols * 3], &buf[lead + (size_t)y * step], (size_t)cols * 3);
    std::vector<rf::OverlayRegion> regs;
    for (size_t k = 0; k < faces.size(); k++) {
        regs.push_back(rf::overlay_region_make(sp, faces[k].v, ids.empty() ? 0 : ids[k], scale, k % 5 == 4));
        check_pieces(sp, regs.back());
    }
    std::vector<int32_t> want, got(regs.size(), -1);
    naive(sp, dense, rows, cols, regs, want);
    rf::overlay_host_frame(sp, buf.data() + lead, rows, cols, step, regs.data(), (int)regs.size(), got.data());
    CHECK(got == want);
    bool same = true, guards = true;
    for (size_t i = 0; i < bytes; i++) {
        const size_t o = i - lead;
        const bool inside = i >= lead && rows && o % step < (size_t)cols * 3;
        if (inside) same = same && buf[i] == dense[(o / step) * cols * 3 + o % step];
        else guards = guards && buf[i] == before[i];
    }
    CHECK(same);
    CHECK(guards);
}

int main() {
    std::mt19937 rng(7);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<rf::OverlaySpec> specs(5);
    specs[1].thickness = 1; specs[1].radius = -1; specs[1].alpha = 1; specs[1].label = RF_OVERLAY_LABEL_ID; specs[1].font = 1;
    specs[2].thickness = 16; specs[2].radius = 16; specs[2].font = 8; specs[2].label = RF_OVERLAY_LABEL_ID; specs[2].color_by_id = 1;
    specs[3].thickness = 3; specs[3].radius = 5; specs[3].alpha = 128; specs[3].label = RF_OVERLAY_LABEL_SCORE; specs[3].font = 3;
    specs[4].thickness = 5; specs[4].label = RF_OVERLAY_LABEL_ID; specs[4].font = 2; specs[4].alpha = 200;
    const int shapes[4][2] = {{48, 64}, {1, 1}, {33, 31}, {7, 90}};
    for (const rf::OverlaySpec &sp : specs)
        for (const auto &s : shapes) {
            const int rows = s[0], cols = s[1];
            const float r = (float)rows, c = (float)cols;
            std::vector<Face> faces = {
                face(-8.f, 10.f, 6.f, 20.f), face(c - 5.f, 10.f, c + 9.f, 20.f), face(10.f, -6.f, 20.f, 4.f), face(10.f, r - 3.f, 20.f, r + 8.f),
                face(-4.f, -4.f, 7.f, 6.f), face(c - 6.f, -3.f, c + 5.f, 8.f), face(-5.f, r - 7.f, 6.f, r + 4.f), face(c - 7.f, r - 6.f, c + 3.f, r + 5.f),
                face(-50.f, -50.f, -20.f, -30.f), face(c + 10.f, 5.f, c + 30.f, 9.f), face(-20.f, -30.f, c + 40.f, r + 50.f),
                face(-1e9f, -5000.f, 1e9f, 9000.f), face(3e38f, 0.f, 3.3e38f, 4.f), face(-3e38f, 0.f, 3e38f, 4.f), face(nan, 1.f, 5.f, 5.f),
                face(1.f, 1.f, inf, 5.f), face(20.f, 5.f, 10.f, 9.f), face(7.f, 7.f, 7.f, 7.f), face(3.f, 3.f, 3.f, 30.f, nan), face(0.f, 0.f, c - 1.f, r - 1.f, 1.f)};
            faces[2].v[6] = nan; faces[3].v[12] = inf; faces[4].v[5] = 1e9f; faces[4].v[10] = -1e9f;
            std::vector<long long> ids;
            for (size_t k = 0; k < faces.size(); k++) ids.push_back(k % 4 == 0 ? 0 : k == 5 ? 999999 : k == 7 ? 1000000 : k == 9 ? -4 : (long long)k * 37);
            run(sp, rows, cols, (size_t)cols * 3, 0, faces, ids, 1.f, rng);                    // dense
            run(sp, rows, cols, (size_t)cols * 3 + 17, 5, faces, ids, 1.f, rng);               // an odd pointer, a padded odd step
            run(sp, rows, cols, (size_t)cols * 3 + 2, 1, faces, {}, 2.857143f, rng);
            run(sp, rows, cols, (size_t)cols * 3, 3, {faces[10], faces[0]}, {}, 3e38f, rng);   // a scale that overflows
        }
    run(specs[0], 0, 0, 0, 0, {face(1.f, 1.f, 5.f, 5.f)}, {}, 1.f, rng);
    // the spec: defaults, every refusal
    rf::OverlaySpec sp;
    CHECK(rf::overlay_spec_resolve(nullptr, 0, &sp) == nullptr && sp.max_regions == 1 && sp.thickness == 2 && sp.radius == 2 && sp.alpha == 255);
    rf_overlay_spec in;
    memset(&in, 0, sizeof(in));
    in.struct_size = sizeof(in);
    CHECK(rf::overlay_spec_resolve(&in, 5000, &sp) == nullptr && sp.max_regions == 1024 && sp.box == 0xff0000u && sp.point == 0x00ff00u && sp.text == 0xffffffu);
    in.colors_set = 1;
    CHECK(rf::overlay_spec_resolve(&in, 256, &sp) == nullptr && sp.box == 0 && sp.point == 0 && sp.text == 0);
    in.colors_set = 0; in.radius = -7; in.box[1] = 9;
    CHECK(rf::overlay_spec_resolve(&in, 256, &sp) == nullptr && sp.radius == -1 && sp.box == 0x000900u && sp.point == 0x00ff00u);
    rf_overlay_spec bad = in; bad.struct_size = 36; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.thickness = 17; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.thickness = -1; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.radius = 17; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.label = 3; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.font_scale = 9; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.max_regions = 1025; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.colors_set = 2; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    bad = in; bad.color_by_id = 2; CHECK(rf::overlay_spec_resolve(&bad, 256, &sp) != nullptr);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("overlay host ok\n");
    return 0;
}
