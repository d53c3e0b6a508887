// test_track.cpp -- face tracks through the class header: RetinaFace::createTracker + detectTracked on raw BGR frames, as two calls of
// three frames each on streams {0, 1, 0}; writes what the calls returned for tests/test_track_gpu.py to compare with the Python calls' bytes.
//   usage: test_track <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames (6)> <threshold> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.  out.bin: per image: int32 k, k x rf_track_tag, int32 e, e x rf_track
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 9) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int nf = atoi(argv[6]);
    const size_t fb = (size_t)o.net_h * o.net_w * 3;
    if (nf != 6) { fprintf(stderr, "six frames\n"); return 2; }
    std::vector<unsigned char> px(fb * nf);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        rf_tracker trk = det.createTracker(2);
        FILE *out = fopen(argv[8], "wb");
        if (!out) return 2;
        for (int call = 0; call < 2; call++) {
            vector<cv::Mat> imgs;
            for (int i = 0; i < 3; i++) imgs.push_back(cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * (3 * call + i)));
            det.detectTracked(imgs, trk, {0, 1, 0}, (float)atof(argv[7]));
            for (int i = 0; i < 3; i++) {
                const vector<rf_track_tag> &tags = det.lastTrackTags()[i];
                const vector<rf_track> &ended = det.lastEndedTracks()[i];
                const int k = (int)tags.size(), e = (int)ended.size();
                if ((int)det.lastBatchResult()[i].size() != k) { fprintf(stderr, "sizes disagree\n"); return 1; }
                fwrite(&k, sizeof(int), 1, out);
                fwrite(tags.data(), sizeof(rf_track_tag), k, out);
                fwrite(&e, sizeof(int), 1, out);
                fwrite(ended.data(), sizeof(rf_track), e, out);
                printf("call %d image %d: %d faces, %d tracks ended\n", call, i, k, e);
            }
        }
        fclose(out);
        rf_tracker_destroy(trk);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
