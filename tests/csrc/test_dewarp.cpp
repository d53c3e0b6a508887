// test_dewarp.cpp -- fisheye detection through the class header: RetinaFace::createDewarper (a ring of views planned from an
// equidistant lens) and RetinaFace::detectDewarped on a raw square BGR frame, run as a batch of {frame, empty, frame}; writes what the call
// returned for tests/test_dewarp_gpu.py to compare with the Python call's bytes.
//   usage: test_dewarp <model_dir> <stem> <net_h> <net_w> <frame.raw> <size> <threshold> <f> <ring> <pitch> <hfov> <vote> <max_faces> <edge> <out.bin>
//   out.bin: int32 n | per image: int32 k, k x 15 float, k x int32 votes, k x int32 source view
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 16) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int size = atoi(argv[6]);
    rf_dewarp_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.model = RF_LENS_EQUIDISTANT;
    spec.f = atof(argv[8]); spec.cx = spec.cy = (size - 1) / 2.0;
    spec.ring = atoi(argv[9]); spec.ring_pitch = atof(argv[10]); spec.ring_hfov = atof(argv[11]);
    spec.vote = atoi(argv[12]); spec.max_faces = atoi(argv[13]); spec.edge = atoi(argv[14]);
    std::vector<unsigned char> px((size_t)size * size * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        rf_dewarper dw = det.createDewarper(size, size, spec);
        cv::Mat img(size, size, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        det.detectDewarped(imgs, dw, (float)atof(argv[7]), &spec);
        const int n = (int)imgs.size();
        if ((int)det.lastBatchResult().size() != n || (int)det.dewarpVotes().size() != n || (int)det.dewarpViews().size() != n) {
            fprintf(stderr, "sizes disagree\n");
            return 1;
        }
        FILE *out = fopen(argv[15], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        for (int i = 0; i < n; i++) {
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[i];
            const int k = (int)faces.size();
            if ((int)det.dewarpVotes()[i].size() != k || (int)det.dewarpViews()[i].size() != k) { fprintf(stderr, "sizes disagree\n"); return 1; }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
            fwrite(det.dewarpVotes()[i].data(), sizeof(int), k, out);
            fwrite(det.dewarpViews()[i].data(), sizeof(int), k, out);
            printf("image %d: %d faces\n", i, k);
        }
        fclose(out);
        rf_dewarper_destroy(dw);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
