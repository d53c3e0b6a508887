// test_follow.cpp -- followed tracks through the class header: RetinaFace::createTracker + enableFollow, then the key / follow schedule on
// raw BGR frames, one call per frame on stream 0: detectTrackFollow on every fourth frame, followTracks on the frames in between;
// writes the faces every call returned for tests/test_follow_gpu.py to compare with the Python calls' bytes.
//   usage: test_follow <model_dir> <stem> <net_h> <net_w> <frames.raw> <n_frames> <threshold> <out.bin>
//   frames.raw: n_frames dense net_h x net_w BGR frames.
//   out.bin: per frame: int32 k, k x rf_face (the detections of a key frame, the followed faces of the others)
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
    if (nf < 1 || nf > 64) { fprintf(stderr, "1 .. 64 frames\n"); return 2; }
    std::vector<unsigned char> px(fb * nf);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        rf_tracker trk = det.createTracker(1);
        det.enableFollow(trk);
        bool twice = false;
        try { det.enableFollow(trk); } catch (const std::exception &) { twice = true; }
        if (!twice) { fprintf(stderr, "a second enableFollow was not refused\n"); return 1; }
        bool plain = false;                           // the plain tracked call refuses such a tracker
        try { det.detectTracked(vector<cv::Mat>(1, cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data())), trk, {0}, 0.5f); } catch (const std::exception &) { plain = true; }
        if (!plain) { fprintf(stderr, "detectTracked on a tracker with follow was not refused\n"); return 1; }
        FILE *out = fopen(argv[8], "wb");
        if (!out) return 2;
        for (int t = 0; t < nf; t++) {
            vector<cv::Mat> imgs(1, cv::Mat(o.net_h, o.net_w, CV_8UC3, px.data() + fb * t));
            if (t % 4 == 0) det.detectTrackFollow(imgs, trk, {0}, (float)atof(argv[7]));
            else det.followTracks(imgs, trk, {0});
            const vector<FaceDetectInfo> &faces = det.lastBatchResult()[0];
            const int k = (int)faces.size();
            if ((int)det.lastTrackTags()[0].size() != k) { fprintf(stderr, "one tag per face expected\n"); return 1; }
            if (t % 4 != 0)
                for (const rf_track_tag &g : det.lastTrackTags()[0])
                    if (!(g.flags & RF_TRACK_FOLLOWED)) { fprintf(stderr, "a followed face without RF_TRACK_FOLLOWED\n"); return 1; }
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(rf_face), k, out);
            printf("frame %d: %d faces (%s)\n", t, k, t % 4 == 0 ? "key" : "followed");
        }
        fclose(out);
        rf_tracker_destroy(trk);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
