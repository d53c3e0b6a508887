// test_overlay.cpp -- overlays through the class header: RetinaFace::detectOverlay on raw BGR frames, which it draws into in place, then
// RetinaFace::detectTrackedOverlay on the same frames in device memory, one after the other as the frames of ONE stream (so a face the
// detector drops coasts and is drawn dashed); writes the annotated frames and the per-region pixel counts of both for
// tests/test_overlay_gpu.py to compare with the Python calls' bytes.
//   usage: test_overlay <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames> <threshold> <label> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.  out.bin: the n_frames frames of detectOverlay, then per image int32 k,
//   k x int32 pixels; then the same for detectTrackedOverlay
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

static void put(FILE *out, const std::vector<unsigned char> &px, const vector<vector<int32_t>> &pixels) {
    fwrite(px.data(), 1, px.size(), out);
    for (const vector<int32_t> &p : pixels) {
        const int k = (int)p.size();
        fwrite(&k, sizeof(int), 1, out);
        fwrite(p.data(), sizeof(int32_t), k, out);
    }
}

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
    const std::vector<unsigned char> orig = px;
    void *dev = nullptr;
    try {
        RetinaFace det(model, o);
        rf_overlay_spec sp = {};
        sp.struct_size = sizeof(sp);
        sp.label = atoi(argv[8]);
        sp.color_by_id = 1;
        vector<cv::Mat> imgs;
        for (int i = 0; i < nf; i++) imgs.push_back(cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * i));
        det.detectOverlay(imgs, (float)atof(argv[7]), &sp);
        FILE *out = fopen(argv[9], "wb");
        if (!out) return 2;
        for (int i = 0; i < nf; i++)
            if (det.overlayPixels()[i].size() != det.lastBatchResult()[i].size()) { fprintf(stderr, "sizes disagree\n"); return 1; }
        put(out, px, det.overlayPixels());

        if (hipMalloc(&dev, fb) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
        rf_tracker trk = det.createTracker(1);
        vector<vector<int32_t>> pixels;
        for (int i = 0; i < nf; i++) {
            if (hipMemcpy(dev, orig.data() + fb * i, fb, hipMemcpyHostToDevice) != hipSuccess) return 1;
            det.detectTrackedOverlay({dev}, {o.net_h}, {o.net_w}, {o.net_w * 3}, trk, {0}, (float)atof(argv[7]), &sp);
            if (hipMemcpy(px.data() + fb * i, dev, fb, hipMemcpyDeviceToHost) != hipSuccess) return 1;
            if (det.lastTrackTags()[0].size() != det.lastBatchResult()[0].size()) { fprintf(stderr, "sizes disagree\n"); return 1; }
            pixels.push_back(det.overlayPixels()[0]);
            printf("frame %d: %d faces, %d regions drawn\n", i, (int)det.lastBatchResult()[0].size(), (int)pixels.back().size());
        }
        put(out, px, pixels);
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(dev);
    return 0;
}
