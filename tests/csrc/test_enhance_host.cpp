// Host-only test of retinaface_amd/csrc/enhance.h, meant to run under -fsanitize=address,undefined
// (tests/test_enhance_host.py::test_enhance_under_address_and_ub_sanitizers): enhance_host over the edge shapes (1, 2, 5, 63, 64, 65, 129
// in both axes) and every tile size, pitched sources and destinations in exactly-sized heap buffers -- a byte read or written outside a
// row's cols * 3 bytes is a sanitizer report -- in place and out of place; the whole domain of the gain's division (Yd = 1..255, every
// numerator up to 2 * 255 * 255 + 255) against the plain integer division; the interpolation axis against its definition.  No GPU, no
// library: the header is compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_enhance_host tests/csrc/test_enhance_host.cpp && ./test_enhance_host
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/enhance.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void frame_case(int rows, int cols, int tile, int dark_below, int src_pad, int dst_pad, int gain_pct, std::mt19937 &rng) {
    rf_enhance_spec raw = {sizeof(rf_enhance_spec), tile, 0, dark_below};
    rf::EnhanceSpec sp;
    CHECK(rf::enhance_spec_resolve(&raw, &sp) == nullptr && sp.tile == tile && sp.clip == 2048);
    const int step = cols * 3 + src_pad, dstep = cols * 3 + dst_pad;
    // the last row ends with its pixels: no padding behind it, so an access past cols * 3 of the last row leaves the buffer
    std::vector<uint8_t> src((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &b : src) b = (uint8_t)((rng() & 255u) * (unsigned)gain_pct / 100u);
    const std::vector<uint8_t> keep = src;
    std::vector<uint8_t> dst((size_t)(rows - 1) * dstep + (size_t)cols * 3, 0xAB);
    const int flagged = rf::enhance_host(sp, src.data(), rows, cols, step, dst.data(), dstep);
    const int tiles = rf::enh_tiles(rows, sp.log2_tile()) * rf::enh_tiles(cols, sp.log2_tile());
    CHECK(flagged >= 0 && flagged <= tiles && src == keep);
    if (dark_below == 256) CHECK(flagged == tiles);
    bool same = true;
    for (int y = 0; y < rows; y++) {
        for (int x = 0; x < cols; x++) {
            const uint8_t *s = &src[(size_t)y * step + 3 * x], *d = &dst[(size_t)y * dstep + 3 * x];
            CHECK(d[0] >= s[0] && d[1] >= s[1] && d[2] >= s[2]);          // never darker
            same = same && !memcmp(s, d, 3);
        }
        if (y + 1 < rows)
            for (int b = cols * 3; b < dstep; b++) CHECK(dst[(size_t)y * dstep + b] == 0xAB);
    }
    if (flagged == 0) CHECK(same);
    // in place: the same bytes
    const int again = rf::enhance_host(sp, src.data(), rows, cols, step, src.data(), step);
    CHECK(again == flagged);
    for (int y = 0; y < rows; y++) CHECK(memcmp(&src[(size_t)y * step], &dst[(size_t)y * dstep], (size_t)cols * 3) == 0);
}

int main() {
    // the division of the gain: every divisor 2 Yd and every numerator 2 c Yn + Yd can reach, and beyond to 2^17
    for (uint32_t yd = 1; yd <= 255; yd++) {
        const uint32_t den = 2 * yd, m = rf::enh_div_magic(den);
        for (uint32_t num = 0; num < (1u << 17); num++)
            if (rf::enh_div(num, m) != num / den) { CHECK(rf::enh_div(num, m) == num / den); break; }
    }
    CHECK(2u * 255u * 255u + 255u < (1u << 17));
    for (uint32_t c = 0; c <= 255; c += 5)
        for (uint32_t yn = 0; yn <= 255; yn += 3)
            for (uint32_t yd = 1; yd <= 255; yd += 7) {
                const uint32_t q = (2 * c * yn + yd) / (2 * yd);
                CHECK(rf::enh_gain(c, yn, yd, rf::enh_div_magic(2 * yd)) == (q > 255 ? 255 : q));
            }
    // the axis: floor division towards minus infinity, clamps, zero weight in front of the first centre
    for (int lt = 4; lt <= 7; lt++) {
        const int T = 1 << lt, D = 2 * T;
        for (int extent : {1, T / 2, T, T + 1, 3 * T + 5}) {
            const int nt = (extent + T - 1) / T;
            CHECK(rf::enh_tiles(extent, lt) == nt);
            for (int y = 0; y < extent; y++) {
                const int p = 2 * y + 1 - T;
                int q = p / D;
                if (p % D < 0) q--;
                int a0, a1, w;
                rf::enh_axis(y, lt, nt, &a0, &a1, &w);
                CHECK(a0 == std::min(std::max(q, 0), nt - 1) && a1 == std::min(std::max(q + 1, 0), nt - 1) && w == (p < 0 ? 0 : p % D));
            }
        }
    }
    std::mt19937 rng(25);
    const int edges[] = {1, 2, 5, 63, 64, 65, 129};
    for (int rows : edges)
        for (int cols : edges) {
            frame_case(rows, cols, 64, 0, 0, 0, 6, rng);
            frame_case(rows, cols, 64, 256, 7, 5, 100, rng);
            frame_case(rows, cols, 16, 0, 5, 0, 12, rng);
            frame_case(rows, cols, 128, 256, 0, 3, 3, rng);
            frame_case(rows, cols, 32, 0, 1, 1, 100, rng);                 // lit: nothing is touched
        }
    // spec refusals and defaults
    rf::EnhanceSpec sp;
    CHECK(rf::enhance_spec_resolve(nullptr, &sp) == nullptr && sp.tile == 64 && sp.clip == 2048 && sp.dark_below == 64);
    const rf_enhance_spec bad[] = {{12, 0, 0, 0}, {16, 48, 0, 0}, {16, -16, 0, 0}, {16, 256, 0, 0}, {16, 0, 255, 0}, {16, 0, 65536, 0},
                                   {16, 0, -1, 0}, {16, 0, 0, 257}, {16, 0, 0, -1}};
    for (const rf_enhance_spec &b : bad) CHECK(rf::enhance_spec_resolve(&b, &sp) != nullptr);
    const rf_enhance_spec good = {16, 128, 65535, 256};
    CHECK(rf::enhance_spec_resolve(&good, &sp) == nullptr && sp.tile == 128 && sp.clip == 65535 && sp.dark_below == 256 && sp.log2_tile() == 7);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
