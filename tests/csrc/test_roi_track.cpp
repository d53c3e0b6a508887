// test_roi_track.cpp -- tracked region detection through the class header: a tracker of two streams and <max_tracks> slots, a key call
// (RetinaFace::detectTracked) on {frame, frame}, then two RetinaFace::detectTrackedRois calls on {frame, empty} -- the second stream
// ages -- on a raw BGR frame; writes what the region calls returned for tests/test_roi_track_gpu.py to compare with the Python calls'
// bytes.
//   usage: test_roi_track <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <max_tracks> <grid> <vote> <margin_q8> <out.bin>
//   out.bin: per region call: int32 n | per image: int32 k, k x 15 float, k x int32 votes, k x int32 slot, k x 24-byte tags,
//            int32 e, e x 176-byte ended tracks, int32 T, T x 32-byte cells
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 14) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]);
    const float thr = (float)atof(argv[8]);
    rf_track_spec ts = {};
    ts.struct_size = sizeof(ts);
    ts.max_tracks = atoi(argv[9]); ts.max_missed = 1;
    rf_roi_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.grid = atoi(argv[10]); spec.vote = atoi(argv[11]);
    const int margin_q8 = atoi(argv[12]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        rf_tracker trk = det.createTracker(2, &ts);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        det.detectTracked({img, img}, trk, {0, 1}, thr);
        FILE *out = fopen(argv[13], "wb");
        if (!out) return 2;
        for (int call = 0; call < 2; call++) {
            vector<cv::Mat> imgs = {img, cv::Mat()};
            det.detectTrackedRois(imgs, trk, {0, 1}, thr, &spec, margin_q8);
            const int n = (int)imgs.size();
            fwrite(&n, sizeof(int), 1, out);
            for (int i = 0; i < n; i++) {
                const vector<FaceDetectInfo> &faces = det.lastBatchResult()[i];
                const int k = (int)faces.size(), e = (int)det.lastEndedTracks()[i].size(), T = (int)det.trackedRoiCells()[i].size();
                if ((int)det.roiVotes()[i].size() != k || (int)det.roiRegions()[i].size() != k || (int)det.lastTrackTags()[i].size() != k) {
                    fprintf(stderr, "sizes disagree\n");
                    return 1;
                }
                fwrite(&k, sizeof(int), 1, out);
                fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
                fwrite(det.roiVotes()[i].data(), sizeof(int), k, out);
                fwrite(det.roiRegions()[i].data(), sizeof(int), k, out);
                fwrite(det.lastTrackTags()[i].data(), sizeof(rf_track_tag), k, out);
                fwrite(&e, sizeof(int), 1, out);
                fwrite(det.lastEndedTracks()[i].data(), sizeof(rf_track), e, out);
                fwrite(&T, sizeof(int), 1, out);
                fwrite(det.trackedRoiCells()[i].data(), sizeof(rf_roi_cell), T, out);
                printf("call %d image %d: %d faces, %d ended\n", call, i, k, e);
            }
        }
        fclose(out);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
