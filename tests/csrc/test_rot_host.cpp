// Host-only test of retinaface_amd/csrc/rot.h, meant to run under -fsanitize=address,undefined
// (tests/test_rot_host.py::test_rotate_and_map_under_address_and_ub_sanitizers): rot_rotate_host over the edge shapes (1, 2, 3, 5, 64, 65
// in both axes), every k, pitched sources and destinations in exactly-sized heap buffers -- a byte read or written outside a row's
// cols_k * 3 bytes is a sanitizer report -- checked against the index rule and by rotating back; rot_map_face on the frame corners and
// on quarter-pixel faces, which the mapping of the inverse pass returns exactly.  No GPU, no library: the header is compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_rot_host tests/csrc/test_rot_host.cpp && ./test_rot_host
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/rot.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void rotate_case(int rows, int cols, int k, int src_pad, int dst_pad, std::mt19937 &rng) {
    const int step = cols * 3 + src_pad;
    // the last row ends with its pixels: no padding behind it, so a read past cols * 3 of the last row leaves the buffer
    std::vector<uint8_t> src((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &b : src) b = (uint8_t)rng();
    const int dr = rf::rot_rows(k, rows, cols), dc = rf::rot_cols(k, rows, cols), dstep = dc * 3 + dst_pad;
    std::vector<uint8_t> dst((size_t)(dr - 1) * dstep + (size_t)dc * 3, 0xAB);
    rf::rot_rotate_host(src.data(), rows, cols, step, k, dst.data(), dstep);
    for (int y = 0; y < dr; y++) {
        for (int x = 0; x < dc; x++) {
            int sy, sx, by, bx;
            rf::rot_src_of_dst(k, rows, cols, y, x, &sy, &sx);
            rf::rot_dst_of_src(k, rows, cols, sy, sx, &by, &bx);
            CHECK(by == y && bx == x && sy >= 0 && sy < rows && sx >= 0 && sx < cols);
            CHECK(memcmp(&dst[(size_t)y * dstep + 3 * x], &src[(size_t)sy * step + 3 * sx], 3) == 0);
        }
        if (y + 1 < dr)
            for (int b = dc * 3; b < dstep; b++) CHECK(dst[(size_t)y * dstep + b] == 0xAB);
    }
    // turning the pass by the remaining quarter turns gives the frame back
    std::vector<uint8_t> back((size_t)rows * cols * 3);
    rf::rot_rotate_host(dst.data(), dr, dc, dstep, (4 - k) % 4, back.data(), cols * 3);
    for (int y = 0; y < rows; y++) CHECK(memcmp(&back[(size_t)y * cols * 3], &src[(size_t)y * step], (size_t)cols * 3) == 0);
}

static void map_case(int rows, int cols, std::mt19937 &rng) {
    std::uniform_int_distribution<int> q(-80, 4 * 4200);
    for (int k = 0; k < 4; k++) {
        const rf::RotEntry e{0, rows, cols, k, 1.f};
        const int pr = rf::rot_rows(k, rows, cols), pc = rf::rot_cols(k, rows, cols);
        const rf::RotEntry inv{0, pr, pc, (4 - k) % 4, 1.f};
        // the corners of the pass land on corners of the frame
        float f[15] = {0.9f, 0.f, 0.f, (float)(pc - 1), (float)(pr - 1)}, g[15];
        for (int i = 0; i < 5; i++) { f[5 + i] = i & 1 ? (float)(pc - 1) : 0.f; f[10 + i] = i & 2 ? (float)(pr - 1) : 0.f; }
        rf::rot_map_face(e, f, g);
        CHECK(g[0] == f[0] && g[1] == 0.f && g[2] == 0.f && g[3] == (float)(cols - 1) && g[4] == (float)(rows - 1));
        for (int i = 0; i < 5; i++)
            CHECK((g[5 + i] == 0.f || g[5 + i] == (float)(cols - 1)) && (g[10 + i] == 0.f || g[10 + i] == (float)(rows - 1)));
        // quarter-pixel coordinates, inside and outside the frame: the inverse pass's mapping returns the face (aliasing in and out)
        for (int t = 0; t < 50; t++) {
            float a[15], b[15];
            a[0] = 0.5f + (float)(t % 32) / 64.f;
            for (int i = 1; i < 15; i++) a[i] = (float)q(rng) / 4.f;
            if (a[1] > a[3]) std::swap(a[1], a[3]);
            if (a[2] > a[4]) std::swap(a[2], a[4]);
            memcpy(b, a, sizeof(a));
            rf::rot_map_face(inv, b, b);              // the face of pass k that maps to a
            CHECK(b[1] <= b[3] && b[2] <= b[4]);
            rf::rot_map_face(e, b, b);
            CHECK(memcmp(a, b, sizeof(a)) == 0);
        }
    }
}

int main() {
    std::mt19937 rng(22);
    const int edges[] = {1, 2, 3, 5, 64, 65};
    for (int rows : edges)
        for (int cols : edges)
            for (int k = 0; k < 4; k++) {
                rotate_case(rows, cols, k, 0, 0, rng);
                rotate_case(rows, cols, k, 7, 5, rng);
            }
    const int shapes[][2] = {{1, 1}, {7, 2}, {448, 448}, {300, 449}, {896, 1280}, {3072, 4096}};
    for (auto &s : shapes) map_case(s[0], s[1], rng);
    rf::RotSpec sp;
    rf_rot_spec raw = {sizeof(rf_rot_spec), 5, 1, 7};
    CHECK(rf::rot_spec_resolve(&raw, 256, &sp) == nullptr && sp.rots == 5 && sp.vote == 1 && sp.max_faces == 7 && sp.passes() == 2);
    raw.rots = 16;
    CHECK(rf::rot_spec_resolve(&raw, 256, &sp) != nullptr);
    CHECK(rf::rot_spec_resolve(nullptr, 256, &sp) == nullptr && sp.rots == 15 && sp.vote == 0 && sp.max_faces == 256);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
