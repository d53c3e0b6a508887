// Host-only test of change regions in retinaface_amd/csrc/change.h (with roi.h), meant to run under -fsanitize=address,undefined
// (tests/test_change_host.py::test_steps_under_address_and_ub_sanitizers): random frames -- pitched, at odd addresses, full and
// one-pixel partial blocks, every block size -- and random masks stepped through change_step_host into exactly-sized heap buffers: a
// byte read past a row's cols * 3 bytes or past the last row, a value written past bw * bh or a record past max_regions is a sanitizer
// report, an overflow in the sums, the threshold product or the shift a UBSan report.  Every output is checked against its definition,
// computed here with plain loops: the sums per pixel, the step rule in 64 bits, the components by repeated relabelling, the
// selection by a full sort.  No GPU, no library: the headers are compiled in.
//   g++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o test_change_host tests/csrc/test_change_host.cpp && ./test_change_host
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/change.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static bool is_void(const rf::RoiCell &c) {
    return c.roi.x == 0 && c.roi.y == 0 && c.roi.w == 0 && c.roi.h == 0 && c.level == 0 && c.x0 == 0 && c.y0 == 0 && c.flags == RF_ROI_VOID;
}

struct Comp { int label, count, x0, y0, x1, y1; };

// the components of a marked grid by relabelling until nothing changes: slow and obviously right
static std::vector<Comp> slow_components(const std::vector<uint8_t> &marked, int bw, int bh) {
    std::vector<int> lab((size_t)bw * bh, -1);
    for (int i = 0; i < bw * bh; i++)
        if (marked[i]) lab[i] = i;
    for (bool moved = true; moved;) {
        moved = false;
        for (int y = 0; y < bh; y++)
            for (int x = 0; x < bw; x++) {
                if (lab[y * bw + x] < 0) continue;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int xx = x + dx, yy = y + dy;
                        if (xx < 0 || yy < 0 || xx >= bw || yy >= bh || lab[yy * bw + xx] < 0) continue;
                        if (lab[yy * bw + xx] < lab[y * bw + x]) { lab[y * bw + x] = lab[yy * bw + xx]; moved = true; }
                    }
            }
    }
    std::vector<Comp> out;
    for (int i = 0; i < bw * bh; i++) {
        if (lab[i] != i) continue;
        Comp c = {i, 0, bw, bh, -1, -1};
        for (int j = 0; j < bw * bh; j++)
            if (lab[j] == i) {
                c.count++;
                c.x0 = std::min(c.x0, j % bw); c.x1 = std::max(c.x1, j % bw);
                c.y0 = std::min(c.y0, j / bw); c.y1 = std::max(c.y1, j / bw);
            }
        out.push_back(c);
    }
    return out;
}

// one changer of rows x cols stepped `steps` times; mode 0: random bytes, 1: a random mask of bright blocks over a dark frame
static void run_case(int rows, int cols, const rf_change_spec &raw, int steps, int mode, int grid, int net, int margin_q8, std::mt19937 &rng) {
    rf::ChangeSpec sp;
    CHECK(rf::change_spec_resolve(&raw, &sp) == nullptr);
    int bw = 0, bh = 0;
    CHECK(rf::change_check_shape(rows, cols, sp, &bw, &bh) == nullptr);
    const int nb = bw * bh, B = sp.block, R = sp.max_regions, cw = net / grid, ch = net / grid;
    // exactly-sized heap buffers
    std::unique_ptr<int32_t[]> ref(new int32_t[nb]);
    std::unique_ptr<uint8_t[]> mask(new uint8_t[nb]);
    std::unique_ptr<rf_roi[]> regions(new rf_roi[R]);
    std::unique_ptr<rf::RoiCell[]> cells(new rf::RoiCell[R]);
    memset(ref.get(), 0x55, sizeof(int32_t) * nb);
    std::vector<long long> want_ref((size_t)nb, 0);
    int64_t counter = 0;
    for (int t = 0; t < steps; t++) {
        const int pad = (int)(rng() % 9), lead = (int)(rng() % 4);
        const size_t step = (size_t)cols * 3 + pad;
        const size_t bytes = lead + (size_t)(rows - 1) * step + (size_t)cols * 3;      // the last row has no padding behind it
        std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes]);
        memset(buf.get(), 0xAB, bytes);
        uint8_t *src = buf.get() + lead;
        std::vector<uint8_t> bright((size_t)nb, 0);
        for (int i = 0; i < nb; i++) bright[i] = mode == 1 && rng() % 5 == 0;
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < 3 * cols; x++)
                src[(size_t)y * step + x] = mode == 0 ? (uint8_t)(rng() & 255) : bright[(y / B) * bw + (x / 3) / B] ? (uint8_t)(200 + rng() % 56) : (uint8_t)(rng() % 8);
        memset(mask.get(), 0x77, nb);
        memset((void *)regions.get(), 0x77, sizeof(rf_roi) * R);
        memset((void *)cells.get(), 0x77, sizeof(rf::RoiCell) * R);
        rf_change_info info = {-1, -1, -1, -1};
        const bool seed = counter == 0;
        rf::change_step_host(sp, src, rows, cols, step, bw, bh, ref.get(), &counter, margin_q8, cw, ch, 2, mask.get(), regions.get(), cells.get(), &info);
        CHECK(counter == t + 1 && info.flags == (seed ? 1 : 0));
        // the definition, per pixel and in 64 bits
        std::vector<uint8_t> want_mask((size_t)nb, 0);
        int changed = 0;
        for (int by = 0; by < bh; by++)
            for (int bx = 0; bx < bw; bx++) {
                long long S = 0, npix = 0;
                for (int y = by * B; y < std::min(rows, (by + 1) * B); y++)
                    for (int x = bx * B; x < std::min(cols, (bx + 1) * B); x++) {
                        const uint8_t *p = src + (size_t)y * step + (size_t)3 * x;
                        S += 29 * p[0] + 150 * p[1] + 77 * p[2];
                        npix++;
                    }
                const int i = by * bw + bx;
                if (seed) want_ref[i] = S;
                else {
                    const long long d = S - want_ref[i];
                    want_mask[i] = (d < 0 ? -d : d) > 16ll * sp.thr_q4 * npix;
                    want_ref[i] += d >= 0 ? d >> sp.adapt_shift : -((-d + (1ll << sp.adapt_shift) - 1) >> sp.adapt_shift);      // floor
                    changed += want_mask[i];
                }
                CHECK(ref[i] == want_ref[i] && mask[i] == want_mask[i]);
            }
        CHECK(info.changed_blocks == changed);
        std::vector<Comp> comps;
        if (!seed && changed) {
            std::vector<uint8_t> marked((size_t)nb, 0);
            for (int y = 0; y < bh; y++)
                for (int x = 0; x < bw; x++) {
                    bool m = want_mask[y * bw + x];
                    if (sp.dilate)
                        for (int dy = -1; dy <= 1; dy++)
                            for (int dx = -1; dx <= 1; dx++)
                                if (x + dx >= 0 && y + dy >= 0 && x + dx < bw && y + dy < bh && want_mask[(y + dy) * bw + x + dx]) m = true;
                    marked[y * bw + x] = m;
                }
            comps = slow_components(marked, bw, bh);
        }
        CHECK(info.components == (int)comps.size());
        std::vector<Comp> sel;
        for (const Comp &c : comps)
            if (c.count >= sp.min_blocks) sel.push_back(c);
        std::sort(sel.begin(), sel.end(), [](const Comp &a, const Comp &b) { return a.count != b.count ? a.count > b.count : a.label < b.label; });
        if ((int)sel.size() > R) sel.resize(R);
        CHECK(info.kept == (int)sel.size());
        for (int k = 0; k < R; k++) {
            if (k >= (int)sel.size()) {
                CHECK(is_void(cells[k]) && regions[k].x == 0 && regions[k].y == 0 && regions[k].w == 0 && regions[k].h == 0);
                continue;
            }
            const Comp &c = sel[k];
            const float f[5] = {0.f, (float)(c.x0 * B), (float)(c.y0 * B), (float)std::min(cols, (c.x1 + 1) * B), (float)std::min(rows, (c.y1 + 1) * B)};
            rf_roi r;
            CHECK(rf::roi_from_face(f, 1.f, margin_q8 ? margin_q8 : 64, &r));
            const rf::RoiCell w = rf::roi_plan(r, cw, ch, 2);
            CHECK(memcmp(&regions[k], &r, sizeof(r)) == 0 && memcmp(&cells[k], &w, sizeof(w)) == 0);
        }
    }
}

int main() {
    std::mt19937 rng(20261021);
    int cases = 0;
    const int shapes[][3] = {{24, 40, 8}, {29, 45, 8}, {33, 33, 32}, {33, 50, 16}, {1, 1, 8}, {7, 200, 16}, {200, 5, 32}, {136, 136, 8}};
    for (const auto &s : shapes)
        for (int mode = 0; mode < 2; mode++)
            for (int a : {0, 1, 8})
                for (int dilate : {1, 2}) {
                    rf_change_spec raw;
                    memset(&raw, 0, sizeof(raw));
                    raw.struct_size = sizeof(raw);
                    raw.block = s[2]; raw.thr_q4 = mode == 0 ? 1 + (int)(rng() % 400) : 0; raw.adapt_shift = a; raw.dilate = dilate;
                    raw.min_blocks = (int)(rng() % 4); raw.max_regions = a == 0 ? 1 : a == 1 ? 0 : 64;
                    const int grid = 1 << (rng() % 3);
                    run_case(s[0], s[1], raw, 4, mode, grid, 448, (int)(rng() % 3) == 0 ? 0 : (int)(rng() % 65536), rng);
                    cases++;
                }
    // the grid limit, and a spec at its extremes
    rf_change_spec big;
    memset(&big, 0, sizeof(big));
    big.struct_size = sizeof(big);
    big.block = 8; big.thr_q4 = 65535; big.adapt_shift = 8; big.min_blocks = 65535; big.max_regions = 64;
    run_case(1024, 1024, big, 2, 0, 4, 448, 65535, rng);
    big.thr_q4 = 1; big.min_blocks = 1;
    run_case(1024, 1024, big, 2, 1, 4, 448, 0, rng);
    cases += 2;
    rf::ChangeSpec sp;
    int bw, bh;
    CHECK(rf::change_spec_resolve(&big, &sp) == nullptr && rf::change_check_shape(1024, 1025, sp, &bw, &bh) != nullptr);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
