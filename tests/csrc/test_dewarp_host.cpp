// Host-only test of retinaface_amd/csrc/dewarp.h, meant to run under -fsanitize=address,undefined
// (tests/test_dewarp_host.py::test_warp_and_map_under_address_and_ub_sanitizers): dewarp_view_host over views of 16 x 16, 16 x 48,
// 80 x 48 and 448 x 448 and sources of 1 x 1, 2 x 3, 63 x 65 and 129 x 131, pitched sources and destinations in exactly-sized heap
// buffers -- a byte read outside a source row's cols * 3 bytes or written outside a view row's view_w * 3 bytes is a sanitizer report --
// over meshes that leave the frame on every side and sit at +-2^22 (the sums then touch 2^30: an int overflow is a UBSan report);
// an identity mesh returns the frame; dewarp_map_face at the extremes (NaN, infinities, +-1e9, the clamp borders) on the same meshes;
// the plan of the four lens models and its refusals.  No GPU, no library: the header is compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_dewarp_host tests/csrc/test_dewarp_host.cpp && ./test_dewarp_host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/dewarp.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// kind 0: nodes from 20 px outside to 20 px beyond the frame; 1: +-2^22; 2: the frame's corners exactly; 3: all negative
static std::vector<int32_t> make_mesh(int kind, int view_w, int view_h, int rows, int cols, std::mt19937 &rng) {
    const int nx = rf::dewarp_nodes_x(view_w), ny = rf::dewarp_nodes_y(view_h);
    std::vector<int32_t> m((size_t)nx * ny * 2);
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            int32_t *n = &m[2 * ((size_t)j * nx + i)];
            switch (kind) {
            case 0: n[0] = (int32_t)(rng() % ((cols + 40) * 256)) - 20 * 256; n[1] = (int32_t)(rng() % ((rows + 40) * 256)) - 20 * 256; break;
            case 1: n[0] = (rng() & 1) ? rf::kDewarpNodeMax : -rf::kDewarpNodeMax; n[1] = (rng() & 1) ? rf::kDewarpNodeMax : -rf::kDewarpNodeMax; break;
            case 2: n[0] = (int32_t)((long long)i * (cols - 1) * 256 / (nx - 1)); n[1] = (int32_t)((long long)j * (rows - 1) * 256 / (ny - 1)); break;
            default: n[0] = -(int32_t)(rng() % 700) - 1; n[1] = -(int32_t)(rng() % 700) - 1; break;
            }
        }
    return m;
}

static void warp_case(int view_w, int view_h, int rows, int cols, int src_pad, int dst_pad, std::mt19937 &rng) {
    const int step = cols * 3 + src_pad, dstep = view_w * 3 + dst_pad;
    // the last row ends with its pixels: no padding behind it, so a read past cols * 3 of the last row leaves the buffer
    std::vector<uint8_t> src((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &b : src) b = (uint8_t)rng();
    for (int kind = 0; kind < 4; kind++) {
        const std::vector<int32_t> mesh = make_mesh(kind, view_w, view_h, rows, cols, rng);
        CHECK(rf::dewarp_check_mesh(view_w, view_h, 1, mesh.data()) == nullptr);
        std::vector<uint8_t> dst((size_t)(view_h - 1) * dstep + (size_t)view_w * 3, 0xAB);
        rf::dewarp_view_host(mesh.data(), view_w, view_h, src.data(), rows, cols, step, dst.data(), dstep);
        for (int y = 0; y + 1 < view_h; y++)
            for (int b = view_w * 3; b < dstep; b++) CHECK(dst[(size_t)y * dstep + b] == 0xAB);
        // the faces of the extremes through the same mesh
        const rf::DewarpEntry e{0, 0, rows, cols, view_w, view_h, kind & 1 ? 2.5f : 1.f, 0, mesh.data()};
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float vals[] = {0.f, -16.f, -16.01f, (float)view_w + 15.f, (float)view_w + 16.5f, 1e9f, -1e9f, 3e38f, -3e38f, inf, -inf, nan, 0.3f, (float)(view_h - 1)};
        for (size_t a = 0; a < sizeof(vals) / sizeof(vals[0]); a++) {
            float f[15], o[15];
            for (int i = 0; i < 15; i++) f[i] = vals[(a + (size_t)i * 5) % (sizeof(vals) / sizeof(vals[0]))];
            f[0] = 0.75f;
            for (int edge = 0; edge <= 8; edge += 8) {
                if (!rf::dewarp_map_face(e, edge, f, o)) continue;
                CHECK(o[0] == 0.75f && o[1] <= o[3] && o[2] <= o[4]);
                for (int i = 1; i < 15; i++) CHECK(std::fabs(o[i]) <= 9.f * 16384.f);      // weights in [-1, 2] per axis: one cell at most
            }
        }
    }
}

static void identity_case(std::mt19937 &rng) {
    const int rows = 48, cols = 80;
    std::vector<uint8_t> src((size_t)rows * cols * 3), dst((size_t)rows * cols * 3);
    for (auto &b : src) b = (uint8_t)rng();
    std::vector<int32_t> mesh((size_t)6 * 4 * 2);
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 6; i++) { mesh[2 * (j * 6 + i)] = i * 16 * 256; mesh[2 * (j * 6 + i) + 1] = j * 16 * 256; }
    rf::dewarp_view_host(mesh.data(), cols, rows, src.data(), rows, cols, cols * 3, dst.data(), cols * 3);
    CHECK(src == dst);
    const rf::DewarpEntry e{0, 0, rows, cols, cols, rows, 1.f, 0, mesh.data()};
    float f[15] = {0.5f, 1.25f, 2.5f, 70.75f, 40.f, 0.f, 79.f, 95.f, -16.f, 33.5f, 0.f, 47.f, 63.f, -16.f, 7.25f}, o[15];
    CHECK(rf::dewarp_map_face(e, 0, f, o));
    CHECK(memcmp(f, o, sizeof(f)) == 0);                     // an identity mesh returns quarter-pixel faces, one cell beyond the view too
}

static void plan_case() {
    rf_dewarp_spec sp;
    memset(&sp, 0, sizeof(sp));
    sp.struct_size = sizeof(sp);
    sp.f = 0.98 * 1024 / 3.14159265358979323846; sp.cx = sp.cy = 511.5;
    sp.ring = 4; sp.ring_pitch = 55.0; sp.ring_hfov = 60.0;
    std::vector<int32_t> mesh(rf::dewarp_view_ints(448, 448) * 4);          // exactly what four views take
    for (int model = 0; model < 4; model++) {
        sp.model = model;
        sp.ring_pitch = model == RF_LENS_ORTHOGRAPHIC ? 30.0 : 55.0;
        int views = 0;
        CHECK(rf::dewarp_plan(sp, 448, 448, mesh.data(), &views) == nullptr && views == 4);
        CHECK(rf::dewarp_check_mesh(448, 448, 4, mesh.data()) == nullptr);
    }
    sp.model = RF_LENS_ORTHOGRAPHIC; sp.ring_pitch = 65.0;          // the top corners reach pi / 2
    CHECK(rf::dewarp_plan(sp, 448, 448, mesh.data(), nullptr) != nullptr);
    sp.model = RF_LENS_STEREOGRAPHIC; sp.ring_pitch = 179.0;
    CHECK(rf::dewarp_plan(sp, 448, 448, mesh.data(), nullptr) != nullptr);
    sp.model = RF_LENS_EQUIDISTANT; sp.ring_pitch = 55.0; sp.f = 1e5;
    CHECK(rf::dewarp_plan(sp, 448, 448, mesh.data(), nullptr) != nullptr);
}

int main() {
    std::mt19937 rng(20261020);
    const int views[][2] = {{16, 16}, {16, 48}, {80, 48}, {448, 448}}, sources[][2] = {{1, 1}, {2, 3}, {63, 65}, {129, 131}};
    for (auto &v : views)
        for (auto &s : sources) {
            warp_case(v[0], v[1], s[0], s[1], 0, 0, rng);
            warp_case(v[0], v[1], s[0], s[1], 7, 5, rng);
        }
    identity_case(rng);
    plan_case();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
