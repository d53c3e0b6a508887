// Host-only test of the blur pieces of retinaface_amd/csrc/redact.h, meant to run under -fsanitize=address,undefined
// (tests/test_redact_blur_host.py::test_host_program_under_sanitizers): redact_host_frame with blur = 1, 2, 3 on small noise frames
// held in exactly-sized heap buffers -- regions across each of the four frame sides, a region larger than the frame, a radius larger
// than the frame, a 1 x 1 frame, a padded row step -- against a naive loop that follows the definition tap by tap; and
// redact_blur_mean against the division it replaces, for every radius and every sum.  The halo's index clamp is where an
// out-of-bounds read would be.  No GPU, no library: the header is compiled into the program.
//   clang++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -fsanitize=address,undefined \
//           -o test_redact_blur_host tests/csrc/test_redact_blur_host.cpp && ./test_redact_blur_host
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../retinaface_amd/csrc/redact.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// B(frame, rho, passes) of a dense rows x cols x 3 frame, tap by tap
static std::vector<uint8_t> naive_blur(const std::vector<uint8_t> &frame, int rows, int cols, int rho, int passes) {
    std::vector<uint8_t> a = frame, b(frame.size());
    const int n = 2 * rho + 1;
    for (int p = 0; p < passes; p++) {
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++)
                for (int ch = 0; ch < 3; ch++) {
                    int s = 0;
                    for (int d = -rho; d <= rho; d++) {
                        const int xx = x + d < 0 ? 0 : x + d >= cols ? cols - 1 : x + d;
                        s += a[((size_t)y * cols + xx) * 3 + ch];
                    }
                    b[((size_t)y * cols + x) * 3 + ch] = (uint8_t)((s + rho) / n);
                }
        a.swap(b);
    }
    for (int p = 0; p < passes; p++) {
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++)
                for (int ch = 0; ch < 3; ch++) {
                    int s = 0;
                    for (int d = -rho; d <= rho; d++) {
                        const int yy = y + d < 0 ? 0 : y + d >= rows ? rows - 1 : y + d;
                        s += a[((size_t)yy * cols + x) * 3 + ch];
                    }
                    b[((size_t)y * cols + x) * 3 + ch] = (uint8_t)((s + rho) / n);
                }
        a.swap(b);
    }
    return a;
}

// one frame (rows x cols, row step = cols * 3 + pad) with the given boxes: redact_host_frame against the naive loop + ownership
static void run(unsigned seed, int rows, int cols, int pad, int cells, int blur, int shape, const std::vector<std::vector<float>> &boxes) {
    std::mt19937 rng(seed);
    const size_t step = (size_t)cols * 3 + pad;
    // exactly sized: the last row has no padding behind it
    std::vector<uint8_t> buf((size_t)(rows - 1) * step + (size_t)cols * 3);
    for (auto &v : buf) v = (uint8_t)(rng() & 255);
    const std::vector<uint8_t> before = buf;
    std::vector<uint8_t> dense((size_t)rows * cols * 3);
    for (int y = 0; y < rows; y++) memcpy(dense.data() + (size_t)y * cols * 3, buf.data() + (size_t)y * step, (size_t)cols * 3);

    rf_redact_spec in;
    memset(&in, 0, sizeof(in));
    in.struct_size = sizeof(in); in.cells = cells; in.shape = shape; in.blur = (uint8_t)blur; in.margin = -1.f;
    rf::RedactSpec sp;
    CHECK(rf::redact_spec_resolve(&in, 256, &sp) == nullptr && sp.blur == blur);
    std::vector<rf::RedactRegion> regions;
    for (const auto &b : boxes) regions.push_back(rf::redact_region_make(b.data(), 1.f, sp.margin, sp.cells, rows, cols));
    std::vector<int32_t> pixels(regions.size(), -1);
    rf::redact_host_frame(sp, buf.data(), rows, cols, step, regions.data(), (int)regions.size(), pixels.data());

    std::vector<uint8_t> want = dense;
    std::vector<int> owner((size_t)rows * cols, -1);
    std::vector<int32_t> wpx(regions.size(), 0);
    for (size_t q = 0; q < regions.size(); q++) {
        const rf::RedactRegion &r = regions[q];
        if (rf::redact_clip_empty(r)) continue;
        const int rho = rf::redact_blur_radius(r);
        CHECK(rho >= 1 && rho <= rf::kRedactMaxBlurRadius);
        const std::vector<uint8_t> bl = naive_blur(dense, rows, cols, rho, blur);
        for (int y = r.cy0; y < r.cy1; y++)
            for (int x = r.cx0; x < r.cx1; x++) {
                if (!rf::redact_covers(r, shape, x, y) || owner[(size_t)y * cols + x] >= 0) continue;
                owner[(size_t)y * cols + x] = (int)q;
                wpx[q]++;
                memcpy(want.data() + ((size_t)y * cols + x) * 3, bl.data() + ((size_t)y * cols + x) * 3, 3);
            }
    }
    for (size_t q = 0; q < regions.size(); q++) CHECK(pixels[q] == wpx[q]);
    bool same = true, pad_kept = true;
    for (int y = 0; y < rows; y++) {
        if (memcmp(buf.data() + (size_t)y * step, want.data() + (size_t)y * cols * 3, (size_t)cols * 3) != 0) same = false;
        if (y + 1 < rows && pad && memcmp(buf.data() + (size_t)y * step + (size_t)cols * 3, before.data() + (size_t)y * step + (size_t)cols * 3, (size_t)pad) != 0)
            pad_kept = false;
    }
    CHECK(same);
    CHECK(pad_kept);
}

int main() {
    // the exact multiply against the division, every radius and every value a sum + rho can take
    for (int rho = 1; rho <= rf::kRedactMaxBlurRadius; rho++) {
        const uint32_t n = 2 * (uint32_t)rho + 1, magic = rf::redact_blur_magic(rho);
        bool ok = true;
        for (uint32_t s = 0; s <= 255u * n; s++) ok = ok && rf::redact_blur_mean(s, rho, magic) == (s + (uint32_t)rho) / n;
        CHECK(ok);
    }
    // refusals of the spec byte
    {
        rf_redact_spec in;
        memset(&in, 0, sizeof(in));
        in.struct_size = sizeof(in);
        rf::RedactSpec sp;
        in.blur = 4; CHECK(rf::redact_spec_resolve(&in, 256, &sp) != nullptr);
        in.blur = 255; CHECK(rf::redact_spec_resolve(&in, 256, &sp) != nullptr);
        in.blur = 1; in.mode = RF_REDACT_FILL; CHECK(rf::redact_spec_resolve(&in, 256, &sp) != nullptr);
        in.blur = 0; CHECK(rf::redact_spec_resolve(&in, 256, &sp) == nullptr && sp.blur == 0);
    }
    const int rows = 23, cols = 31;
    const std::vector<std::vector<float>> sides = {
        {-6.f, 5.f, 7.f, 14.f}, {25.f, 3.f, 40.f, 12.f}, {9.f, -5.f, 18.f, 4.f}, {12.f, 17.f, 22.f, 30.f},      // left, right, top, bottom
        {14.f, 8.f, 17.f, 11.f}, {-100.f, 5.f, -90.f, 9.f}};                                                     // inside; wholly outside
    const std::vector<std::vector<float>> huge = {{3.f, 4.f, 6.f, 7.f}, {-40.f, -30.f, 80.f, 70.f}};             // larger than the frame on every side
    unsigned seed = 1;
    for (int blur = 1; blur <= 3; blur++)
        for (int shape = 0; shape <= 1; shape++) {
            for (int cells : {1, 2, 8}) run(seed++, rows, cols, 5, cells, blur, shape, sides);      // cells = 1: rho = c up to 15
            run(seed++, rows, cols, 0, 1, blur, shape, huge);                                       // c = 121: rho = 64 > the frame
            run(seed++, rows, cols, 7, 3, blur, shape, huge);                                       // rho = 41 > the frame
            run(seed++, 1, 1, 0, 8, blur, shape, {{0.f, 0.f, 0.5f, 0.5f}});
            run(seed++, 1, 9, 0, 2, blur, shape, {{-2.f, 0.f, 20.f, 0.5f}});
            run(seed++, 9, 1, 3, 2, blur, shape, {{0.f, 2.f, 0.5f, 30.f}});
        }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
