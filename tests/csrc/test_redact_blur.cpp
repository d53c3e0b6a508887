// test_redact_blur.cpp -- blur redaction through the class header: RetinaFace::detectRedacted with rf_redact_spec.blur set (the spec
// passes through; the class needs no new signature) on raw BGR frames, which it modifies in place; writes the blurred frames and the
// per-face pixel counts for tests/test_redact_blur_gpu.py to compare with the Python call's bytes and the reference.
//   usage: test_redact_blur <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames> <threshold> <blur> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.  out.bin: the n_frames redacted frames, then per image: int32 k, k x int32 pixels
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 10) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int nf = atoi(argv[6]);
    const size_t fb = (size_t)o.net_h * o.net_w * 3;
    if (nf < 1 || nf > 64) { fprintf(stderr, "1..64 frames\n"); return 2; }
    std::vector<unsigned char> px(fb * nf);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        rf_redact_spec sp = {};
        sp.struct_size = sizeof(sp);
        sp.blur = (uint8_t)atoi(argv[8]);
        vector<cv::Mat> imgs;
        for (int i = 0; i < nf; i++) imgs.push_back(cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * i));
        det.detectRedacted(imgs, (float)atof(argv[7]), &sp);
        FILE *out = fopen(argv[9], "wb");
        if (!out) return 2;
        fwrite(px.data(), 1, px.size(), out);
        for (int i = 0; i < nf; i++) {
            const vector<int32_t> &p = det.redactedPixels()[i];
            const int k = (int)p.size();
            if ((int)det.lastBatchResult()[i].size() != k) { fprintf(stderr, "sizes disagree\n"); return 1; }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(p.data(), sizeof(int32_t), k, out);
            printf("image %d: %d faces blurred\n", i, k);
        }
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
