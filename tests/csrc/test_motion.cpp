// test_motion.cpp -- motion-predicted tracks through the class header: RetinaFace::createTracker + enableMotion + detectTracked on raw
// BGR frames, one call per frame on stream 0; writes what the calls returned, the stream's motion records after every call and the
// predicted faces of its live tracks for tests/test_motion_gpu.py to compare with the Python calls' bytes.
//   usage: test_motion <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames> <threshold> <alpha> <horizon> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.
//   out.bin: per frame: int32 k, k x rf_track_tag, int32 T, T x rf_track_motion, int32 p, p x rf_face (predictTrack, ahead 1, of the
//            slots whose motion record has samples > 0, in slot order)
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
    o.precision = RF_PRECISION_FP16;                  // the engine the Python side of the test compares with
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int nf = atoi(argv[6]);
    const size_t fb = (size_t)o.net_h * o.net_w * 3;
    if (nf < 1 || nf > 64) { fprintf(stderr, "1 .. 64 frames\n"); return 2; }
    std::vector<unsigned char> px(fb * nf);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    rf_motion_spec ms = {};
    ms.struct_size = sizeof(ms);
    ms.alpha = (float)atof(argv[8]); ms.horizon = atoi(argv[9]);
    try {
        RetinaFace det(model, o);
        rf_tracker trk = det.createTracker(1);
        det.enableMotion(trk, &ms);
        bool twice = false;
        try { det.enableMotion(trk, &ms); } catch (const std::exception &) { twice = true; }
        if (!twice) { fprintf(stderr, "a second enableMotion was not refused\n"); return 1; }
        FILE *out = fopen(argv[10], "wb");
        if (!out) return 2;
        std::vector<rf_track> table(64);
        for (int t = 0; t < nf; t++) {
            vector<cv::Mat> imgs(1, cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * t));
            det.detectTracked(imgs, trk, {0}, (float)atof(argv[7]));
            const vector<rf_track_tag> &tags = det.lastTrackTags()[0];
            const int k = (int)tags.size();
            fwrite(&k, sizeof(int), 1, out);
            fwrite(tags.data(), sizeof(rf_track_tag), k, out);
            const vector<rf_track_motion> rec = det.readMotion(trk, 0);
            const int T = (int)rec.size();
            if (T != 64 || rf_tracker_read(trk, 0, table.data(), 64, nullptr, nullptr) != 64) { fprintf(stderr, "64 slots expected\n"); return 1; }
            fwrite(&T, sizeof(int), 1, out);
            fwrite(rec.data(), sizeof(rf_track_motion), T, out);
            std::vector<rf_face> pred;
            for (int s = 0; s < T; s++)
                if (table[s].id != 0 && rec[s].samples > 0) pred.push_back(RetinaFace::predictTrack(table[s], rec[s], 1, &ms));
            const int p = (int)pred.size();
            fwrite(&p, sizeof(int), 1, out);
            fwrite(pred.data(), sizeof(rf_face), p, out);
            printf("frame %d: %d faces, %d predicted tracks\n", t, k, p);
        }
        fclose(out);
        rf_tracker_destroy(trk);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
