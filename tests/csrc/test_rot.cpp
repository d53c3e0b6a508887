// test_rot.cpp -- rotation-robust detection through the class header: RetinaFace::detectRotated on a raw BGR frame, run as a batch of
// {frame, empty, frame}; writes what the call returned for tests/test_rot_gpu.py to compare with the Python call's bytes.
//   usage: test_rot <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <rots> <vote> <max_faces> <out.bin>
//   out.bin: int32 n | per image: int32 k, k x 15 float, k x int32 votes, k x int32 source rotation, int32 frame rotation, 4 float sums
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
    rf_rot_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.rots = atoi(argv[9]); spec.vote = atoi(argv[10]); spec.max_faces = atoi(argv[11]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        det.detectRotated(imgs, (float)atof(argv[8]), &spec);
        const int n = (int)imgs.size();
        if ((int)det.lastBatchResult().size() != n || (int)det.rotVotes().size() != n || (int)det.rotSources().size() != n ||
            (int)det.frameRotations().size() != n || (int)det.rotScores().size() != 4 * n) {
            fprintf(stderr, "sizes disagree\n");
            return 1;
        }
        FILE *out = fopen(argv[12], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        for (int i = 0; i < n; i++) {
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[i];
            const int k = (int)faces.size();
            if ((int)det.rotVotes()[i].size() != k || (int)det.rotSources()[i].size() != k) { fprintf(stderr, "sizes disagree\n"); return 1; }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
            fwrite(det.rotVotes()[i].data(), sizeof(int), k, out);
            fwrite(det.rotSources()[i].data(), sizeof(int), k, out);
            fwrite(&det.frameRotations()[i], sizeof(int), 1, out);
            fwrite(&det.rotScores()[(size_t)i * 4], sizeof(float), 4, out);
            printf("image %d: %d faces, rotation %d\n", i, k, det.frameRotations()[i]);
        }
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
