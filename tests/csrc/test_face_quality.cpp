// test_face_quality.cpp -- RetinaFace::detectFaceBatchGated through the class header, and the host half of face quality.
//   test_face_quality host
//       rf_face_pose / rf_face_gate_eval on fixed faces: no GPU, no handle.  Built with -DRF_FACE_QUALITY_HEADER (a compiler that
//       knows _Float16: clang) and -fsanitize=address,undefined, face_quality.h itself is compiled into the program and checked
//       under the sanitizers against the library (the program links the library but starts no engine).
//   test_face_quality <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <crop> <format> <rgb> <capacity>
//                     <max_faces> <min_sharpness> <out.bin>
//       reads a raw BGR frame, runs it as a batch of {frame, empty, frame} behind a sharpness gate (min_sharpness < 0: no gate) and
//       writes what the call returned for tests/test_face_quality_gpu.py to compare with tests/face_quality_ref.py.
//   out.bin: int32 n | int32 truncated | (n + 1) int32 offsets | per image: int32 k, k x 15 float | int32 stride | n x stride records |
//            int32 faces | faces x 6 double | the tensor bytes
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "RetinaFace.h"
#ifdef RF_FACE_QUALITY_HEADER      // -DRF_FACE_QUALITY_HEADER: face_quality.h itself compiled into this (instrumented) program
#include "../../retinaface_amd/csrc/face_quality.h"

// the header's code, here under the sanitizers, against the library's: the same bits, and every bad gate refused
static int header_checks() {
    const float cs[3] = {1.f, 2.5f, 1280.f / 448.f};
    const int sizes[3] = {16, 112, 512};
    unsigned seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
    for (int it = 0; it < 300; it++) {
        rf_face f = {};
        for (int i = 0; i < 5; i++) { f.px[i] = rnd() * 1280.f; f.py[i] = rnd() * 896.f; }
        if (it % 50 == 0) { f.px[1] = f.px[0]; f.py[1] = f.py[0]; }                       // coincident eyes
        if (it % 75 == 1) for (int i = 0; i < 5; i++) { f.px[i] = 7.f; f.py[i] = 9.f; }   // no plane
        const int S = sizes[it % 3];
        const float c = cs[(it / 3) % 3];
        rf::AlignXform t;
        rf::align_estimate(f.px, f.py, c, S, &t);
        rf_face_quality a, b;
        memset(&a, 0, sizeof(a));
        rf::face_pose(f.px, f.py, c, t, &a);
        a.flags = t.valid ? 0 : RF_GATE_INVALID;
        if (rf_face_pose(&f, c, S, &b) != RF_OK || memcmp(&a, &b, sizeof(a)) != 0) return 21;
        a.sum_lap = (long long)(rnd() * 2000.f) - 1000; a.sum_lap2 = (long long)(rnd() * 1.0e9f); a.sum_luma = (long long)(rnd() * 255.f * S * S);
        a.covered = (int)(rnd() * S * S);
        a.sharpness = rf::face_quality_finish(a.sum_lap, a.sum_lap2, S);
        rf_face_gate g = {};
        g.struct_size = sizeof(g);
        g.min_sharpness = rnd() * 500.f; g.min_iod = rnd() * 400.f; g.max_abs_yaw = rnd(); g.max_sin2_roll = rnd() * 0.5f;
        g.min_covered = rnd(); g.min_luma = rnd() * 100.f; g.max_luma = 100.f + rnd() * 155.f;
        rf::FaceGate w;
        if (rf::face_gate_resolve(&g, &w) != nullptr) return 22;
        if (rf::face_gate_eval(w, a, !t.valid, S) != rf_face_gate_eval(&g, &a, S)) return 23;
    }
    if (rf::face_quality_finish(0, 270608040000LL, 512) != 1040400.0 || rf::face_luma(255, 255, 255) != 255 || rf::face_luma(0, 0, 0) != 0) return 24;
    rf_face_gate g = {};
    rf::FaceGate w;
    if (!rf::face_gate_resolve(nullptr, &w) || !rf::face_gate_resolve(&g, &w)) return 25;            // null; struct_size 0
    g.struct_size = sizeof(g);
    if (rf::face_gate_resolve(&g, &w)) return 26;                                                      // all off: fine
    float *fields[7] = {&g.min_sharpness, &g.min_iod, &g.max_abs_yaw, &g.max_sin2_roll, &g.min_covered, &g.min_luma, &g.max_luma};
    const float bad[4] = {-1.f, NAN, INFINITY, -INFINITY};
    for (float *p : fields)
        for (float v : bad) { *p = v; if (!rf::face_gate_resolve(&g, &w)) return 27; *p = 0.f; }
    g.min_covered = 1.0000001f;
    if (!rf::face_gate_resolve(&g, &w)) return 28;
    return 0;
}
#else
static int header_checks() { return 0; }
#endif

static int host_checks() {
    rf_face f = {};
    const float tx[5] = {38.2946f, 73.5318f, 56.0252f, 41.5493f, 70.7299f}, ty[5] = {51.6963f, 51.5014f, 71.7366f, 92.3655f, 92.2041f};
    for (int i = 0; i < 5; i++) { f.px[i] = tx[i] * 2.f + 10.f; f.py[i] = ty[i] * 2.f + 20.f; }
    rf_face_quality q;
    memset(&q, 0x55, sizeof(q));
    if (rf_face_pose(&f, 1.f, 112, &q) != RF_OK || q.flags != 0) return 1;
    if (!(std::fabs(q.iod2 - 4.0 * (35.2372 * 35.2372 + 0.1949 * 0.1949)) < 1e-2) || !(std::fabs(q.yaw) < 0.01) || !(q.sin2_roll < 1e-9)) return 2;
    if (q.covered != 0 || q.sum_luma != 0 || q.sum_lap != 0 || q.sum_lap2 != 0 || q.sharpness != 0.0) return 3;
    rf_face_gate g = {};
    g.struct_size = sizeof(g);
    g.min_iod = 80.f; g.max_abs_yaw = 0.25f;
    if (rf_face_gate_eval(&g, &q, 112) != RF_GATE_IOD) return 4;
    g.min_iod = 60.f;
    if (rf_face_gate_eval(&g, &q, 112) != 0 || rf_face_gate_eval(nullptr, &q, 112) != 0) return 5;
    g.min_luma = 1.f;
    if (rf_face_gate_eval(&g, &q, 112) != RF_GATE_DARK) return 6;
    g.min_luma = -1.f;
    if (rf_face_gate_eval(&g, &q, 112) != RF_ERR_INVALID_ARG) return 7;
    g.min_luma = 0.f; g.struct_size = 4;
    if (rf_face_gate_eval(&g, &q, 112) != RF_ERR_INVALID_ARG || rf_face_pose(&f, 1.f, 7, &q) != RF_ERR_INVALID_ARG) return 8;
    rf_face same = {};
    for (int i = 0; i < 5; i++) { same.px[i] = 100.f; same.py[i] = 50.f; }
    if (rf_face_pose(&same, 1.f, 0, &q) != RF_OK || q.flags != RF_GATE_INVALID || q.iod2 != 0.0 || q.yaw != 0.0 || q.sin2_roll != 0.0) return 9;
    g.struct_size = sizeof(g);
    if (rf_face_gate_eval(&g, &q, 0) != (RF_GATE_INVALID | RF_GATE_IOD)) return 10;
    if (int rc = header_checks()) return rc;
    printf("face quality host checks ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "host")) return host_checks();
    if (argc != 16) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]);
    rf_face_batch_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.crop_size = atoi(argv[9]); spec.format = atoi(argv[10]); spec.rgb = atoi(argv[11]); spec.capacity = atoi(argv[12]);
    spec.max_faces = atoi(argv[13]);
    rf_face_gate gate = {};
    gate.struct_size = sizeof(gate);
    gate.min_sharpness = (float)atof(argv[14]);
    const bool has_gate = gate.min_sharpness >= 0.f;
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        vector<uint8_t> tensor = det.detectFaceBatchGated(imgs, (float)atof(argv[8]), spec, has_gate ? &gate : nullptr);
        const int n = (int)imgs.size(), tr = det.faceBatchTruncated() ? 1 : 0, stride = det.faceBatchQualityStride();
        if ((int)det.faceBatchOffsets().size() != n + 1 || (int)det.lastBatchResult().size() != n ||
            det.faceBatchQuality().size() != (size_t)n * stride) { fprintf(stderr, "sizes disagree\n"); return 1; }
        FILE *out = fopen(argv[15], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        fwrite(&tr, sizeof(int), 1, out);
        fwrite(det.faceBatchOffsets().data(), sizeof(int), (size_t)n + 1, out);
        for (const vector<FaceDetectInfo> &faces : det.lastBatchResult()) {
            const int k = (int)faces.size();
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
        }
        fwrite(&stride, sizeof(int), 1, out);
        fwrite(det.faceBatchQuality().data(), sizeof(rf_face_quality), (size_t)n * stride, out);
        const int got = (int)(det.faceBatchMatrices().size() / 6);
        fwrite(&got, sizeof(int), 1, out);
        fwrite(det.faceBatchMatrices().data(), sizeof(double), (size_t)got * 6, out);
        fwrite(tensor.data(), 1, tensor.size(), out);
        fclose(out);
        printf("faces %d of %d truncated %d bytes %zu\n", got, det.faceBatchOffsets()[n], tr, tensor.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
