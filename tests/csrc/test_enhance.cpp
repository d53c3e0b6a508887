// test_enhance.cpp -- low-light detection through the class header: RetinaFace::detectEnhanced on a raw BGR frame, run as a batch of
// {frame, empty, frame}; writes what the call returned for tests/test_enhance_gpu.py to compare with the Python call's bytes.
//   usage: test_enhance <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <tile> <clip> <dark_below> <out.bin>
//   out.bin: int32 n | per image: int32 k, k x 15 float, int32 tiles enhanced
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 13) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]);
    rf_enhance_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.tile = atoi(argv[9]); spec.clip = atoi(argv[10]); spec.dark_below = atoi(argv[11]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    const std::vector<unsigned char> before = px;
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        det.detectEnhanced(imgs, (float)atof(argv[8]), &spec);
        const int n = (int)imgs.size();
        if ((int)det.lastBatchResult().size() != n || (int)det.tilesEnhanced().size() != n) { fprintf(stderr, "sizes disagree\n"); return 1; }
        if (px != before) { fprintf(stderr, "the frame was written\n"); return 1; }
        FILE *out = fopen(argv[12], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        for (int i = 0; i < n; i++) {
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[i];
            const int k = (int)faces.size();
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
            fwrite(&det.tilesEnhanced()[i], sizeof(int), 1, out);
            printf("image %d: %d faces, %d tiles enhanced\n", i, k, det.tilesEnhanced()[i]);
        }
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
