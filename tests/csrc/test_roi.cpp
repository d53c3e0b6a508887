// test_roi.cpp -- region detection through the class header: RetinaFace::detectRois on a raw BGR frame, run as a batch of
// {frame, empty, frame} with the regions read from a file (the first frame gets all of them, the third the first half), and
// RetinaFace::roisFromFaces over the first frame's result; writes what the calls returned for tests/test_roi_gpu.py to compare with the
// Python call's bytes.
//   usage: test_roi <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <rois.bin> <threshold> <grid> <max_zoom> <vote> <max_faces> <out.bin>
//   rois.bin: int32 x, y, w, h per region
//   out.bin: int32 n | per image: int32 k, k x 15 float, k x int32 votes, k x int32 region | int32 m, m x 4 int32: roisFromFaces of image 0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 15) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]);
    rf_roi_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.grid = atoi(argv[10]); spec.max_zoom = atoi(argv[11]); spec.vote = atoi(argv[12]); spec.max_faces = atoi(argv[13]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    std::vector<rf_roi> rois;
    f = fopen(argv[8], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
    rf_roi r;
    while (fread(&r, sizeof(r), 1, f) == 1) rois.push_back(r);
    fclose(f);
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        vector<vector<rf_roi>> lists = {rois, rois, vector<rf_roi>(rois.begin(), rois.begin() + rois.size() / 2)};
        det.detectRois(imgs, lists, (float)atof(argv[9]), &spec);
        const int n = (int)imgs.size();
        if ((int)det.lastBatchResult().size() != n || (int)det.roiVotes().size() != n || (int)det.roiRegions().size() != n) {
            fprintf(stderr, "sizes disagree\n");
            return 1;
        }
        FILE *out = fopen(argv[14], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        for (int i = 0; i < n; i++) {
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[i];
            const int k = (int)faces.size();
            if ((int)det.roiVotes()[i].size() != k || (int)det.roiRegions()[i].size() != k) { fprintf(stderr, "sizes disagree\n"); return 1; }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
            fwrite(det.roiVotes()[i].data(), sizeof(int), k, out);
            fwrite(det.roiRegions()[i].data(), sizeof(int), k, out);
            printf("image %d: %d faces\n", i, k);
        }
        const vector<rf_roi> next = RetinaFace::roisFromFaces(det.lastBatchResult()[0]);
        const int m = (int)next.size();
        fwrite(&m, sizeof(int), 1, out);
        fwrite(next.data(), sizeof(rf_roi), m, out);
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
