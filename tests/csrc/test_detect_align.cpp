// test_detect_align.cpp -- RetinaFace::detectAndAlign through the class header, the way a C++ caller of the reference's class would
// use it: reads a raw BGR frame, writes what the call returned for tests/test_gpu_align.py to compare with tests/align_ref.py.
//   usage: test_detect_align <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <crop> <out.bin>
//   out.bin: int32 k | k x 15 float (lastResult) | k x 6 double (alignMatrices) | k x crop x crop x 3 u8
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 11) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]), crop = atoi(argv[9]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> crops = det.detectAndAlign(img, (float)atof(argv[8]), crop);
        const vector<FaceDetectInfo> &faces = det.lastResult();
        const int k = (int)faces.size();
        if ((int)crops.size() != k || det.alignMatrices().size() != (size_t)k * 6) { fprintf(stderr, "sizes disagree\n"); return 1; }
        FILE *out = fopen(argv[10], "wb");
        if (!out) return 2;
        fwrite(&k, sizeof(int), 1, out);
        fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
        fwrite(det.alignMatrices().data(), sizeof(double), (size_t)k * 6, out);
        for (const cv::Mat &c : crops) {
            if (c.rows != crop || c.cols != crop || !c.isContinuous()) { fprintf(stderr, "bad crop\n"); return 1; }
            fwrite(c.data, 1, (size_t)crop * crop * 3, out);
        }
        fclose(out);
        printf("faces %d crop %d scale %.6f\n", k, crop, det.frameScale(img));
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
