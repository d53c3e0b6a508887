// test_shot.cpp -- the best-shot gallery through the class header: RetinaFace::createTracker + enableShots + detectTrackShots on raw BGR
// frames, as two calls of three frames each on one stream, then flushShots; writes what the flush returned for tests/test_shot_gpu.py to
// compare with the Python calls' bytes.
//   usage: test_shot <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames (6)> <threshold> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.  out.bin: int32 k, k x rf_track, k shots (32 x 32 x 3 u8 BGR), k x rf_shot
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
        rf_tracker trk = det.createTracker(1);
        rf_face_batch_spec sp = {};
        sp.struct_size = sizeof(sp);
        sp.crop_size = 32; sp.format = RF_FACES_U8_HWC; sp.rgb = 0; sp.capacity = 1;
        const size_t bpf = det.enableShots(trk, sp);
        if (bpf != 32 * 32 * 3) { fprintf(stderr, "bytes per shot\n"); return 1; }
        for (int call = 0; call < 2; call++) {
            vector<cv::Mat> imgs;
            for (int i = 0; i < 3; i++) imgs.push_back(cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * (3 * call + i)));
            det.detectTrackShots(imgs, trk, {0, 0, 0}, (float)atof(argv[7]));
            for (int i = 0; i < 3; i++) {
                if (det.lastShotInfo()[i].size() != det.lastEndedTracks()[i].size() || det.lastShots()[i].size() != bpf * det.lastEndedTracks()[i].size()) {
                    fprintf(stderr, "sizes disagree\n");
                    return 1;
                }
                printf("call %d image %d: %d faces, %d tracks ended\n", call, i, (int)det.lastBatchResult()[i].size(), (int)det.lastEndedTracks()[i].size());
            }
        }
        vector<uint8_t> shots;
        vector<rf_shot> info;
        const vector<rf_track> ended = det.flushShots(trk, 0, &shots, &info);
        const int k = (int)ended.size();
        FILE *out = fopen(argv[8], "wb");
        if (!out) return 2;
        fwrite(&k, sizeof(int), 1, out);
        fwrite(ended.data(), sizeof(rf_track), k, out);
        fwrite(shots.data(), 1, shots.size(), out);
        fwrite(info.data(), sizeof(rf_shot), k, out);
        fclose(out);
        rf_tracker_destroy(trk);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
