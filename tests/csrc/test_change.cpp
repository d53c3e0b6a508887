// test_change.cpp -- change regions through the class header: a tracker and a changer of one stream, a key call
// (RetinaFace::detectTracked) on the first raw BGR frame, then RetinaFace::detectChanged on the first frame (the changer seeds) and
// on the second (a newcomer); writes what the two calls returned for tests/test_change_gpu.py to compare with the Python calls' bytes.
//   usage: test_change <model_dir> <stem> <net_h> <net_w> <first.raw> <second.raw> <rows> <cols> <threshold> <max_tracks> <max_regions> <out.bin>
// Then RetinaFace::changeRegions on a second changer over the two frames in device memory (hipMalloc: the program links the HIP runtime).
//   out.bin: per call: int32 k, k x 15 float, k x int32 votes, k x int32 region, k x 24-byte tags, int32 S, S x 32-byte cells,
//            16 bytes of info; then per changeRegions call: int32 R, R x 32-byte cells, 16 bytes of info
#include <hip/hip_runtime_api.h>

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
    const int rows = atoi(argv[7]), cols = atoi(argv[8]);
    const float thr = (float)atof(argv[9]);
    rf_track_spec ts = {};
    ts.struct_size = sizeof(ts);
    ts.max_tracks = atoi(argv[10]);
    rf_change_spec cs = {};
    cs.struct_size = sizeof(cs);
    cs.max_regions = atoi(argv[11]);
    std::vector<unsigned char> px[2];
    for (int k = 0; k < 2; k++) {
        px[k].resize((size_t)rows * cols * 3);
        FILE *f = fopen(argv[5 + k], "rb");
        if (!f || fread(px[k].data(), 1, px[k].size(), f) != px[k].size()) { fprintf(stderr, "cannot read %s\n", argv[5 + k]); return 2; }
        fclose(f);
    }
    try {
        RetinaFace det(model, o);
        rf_tracker trk = det.createTracker(1, &ts);
        rf_changer chg = det.createChanger(rows, cols, 1, &cs);
        cv::Mat first(rows, cols, CV_8UC3, px[0].data()), second(rows, cols, CV_8UC3, px[1].data());
        det.detectTracked({first}, trk, {0}, thr);
        FILE *out = fopen(argv[12], "wb");
        if (!out) return 2;
        for (int call = 0; call < 2; call++) {
            det.detectChanged({call ? second : first}, chg, {0}, trk, thr);
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[0];
            const int k = (int)faces.size(), S = (int)det.trackedRoiCells()[0].size();
            if ((int)det.roiVotes()[0].size() != k || (int)det.roiRegions()[0].size() != k || (int)det.lastTrackTags()[0].size() != k ||
                det.changeInfo().size() != 1) {
                fprintf(stderr, "sizes disagree\n");
                return 1;
            }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
            fwrite(det.roiVotes()[0].data(), sizeof(int), k, out);
            fwrite(det.roiRegions()[0].data(), sizeof(int), k, out);
            fwrite(det.lastTrackTags()[0].data(), sizeof(rf_track_tag), k, out);
            fwrite(&S, sizeof(int), 1, out);
            fwrite(det.trackedRoiCells()[0].data(), sizeof(rf_roi_cell), S, out);
            fwrite(det.changeInfo().data(), sizeof(rf_change_info), 1, out);
            printf("call %d: %d faces, %d changed blocks\n", call, k, det.changeInfo()[0].changed_blocks);
        }
        rf_changer alone = det.createChanger(rows, cols, 1, &cs);
        for (int call = 0; call < 2; call++) {
            void *d = nullptr;
            if (hipMalloc(&d, px[call].size()) != hipSuccess || hipMemcpy(d, px[call].data(), px[call].size(), hipMemcpyHostToDevice) != hipSuccess) {
                fprintf(stderr, "no device memory\n");
                return 1;
            }
            const vector<vector<rf_roi_cell>> cells = det.changeRegions(alone, {d}, {cols * 3}, {0});
            (void)hipFree(d);
            const int R = (int)cells[0].size();
            if (cells.size() != 1 || det.changeInfo().size() != 1) { fprintf(stderr, "sizes disagree\n"); return 1; }
            fwrite(&R, sizeof(int), 1, out);
            fwrite(cells[0].data(), sizeof(rf_roi_cell), R, out);
            fwrite(det.changeInfo().data(), sizeof(rf_change_info), 1, out);
        }
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
