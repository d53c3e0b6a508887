// RetinaFace.cpp -- the reference's class surface (retinaface/RetinaFace.h:63-78) over the C ABI.
#include "../../include/RetinaFace.h"

#include <cstring>
#include <stdexcept>

static_assert(sizeof(FaceDetectInfo) == sizeof(rf_face) && sizeof(rf_face) == 15 * sizeof(float),
              "FaceDetectInfo must stay layout-compatible with the reference (RetinaFace.h:37-42)");

static void check(int status, rf_handle h, const char *what) {
    if (status == RF_OK || status == RF_ERR_TRUNCATED) return;
    throw std::runtime_error(std::string(what) + ": " + rf_last_error(h));
}

void RetinaFace::init(const string &model, const rf_options *options, const string &net, float nms) {
    network = net;
    nms_threshold = nms;
    rf_options o;
    if (options) o = *options; else { memset(&o, 0, sizeof(o)); }
    o.struct_size = sizeof(o);
    if (o.max_detections > 0) maxDet_ = o.max_detections;
    check(rf_create(model.c_str(), net.c_str(), nms, &o, &h_), nullptr, "RetinaFace");
    rf_get_net_size(h_, &netH_, &netW_, nullptr);
}

RetinaFace::RetinaFace(string &model, string net, float nms) { init(model, nullptr, net, nms); }
RetinaFace::RetinaFace(const string &model, const rf_options &options, string net, float nms) { init(model, &options, net, nms); }
RetinaFace::~RetinaFace() { rf_destroy(h_); }

void RetinaFace::detectBatchImages(vector<cv::Mat> imgs, float threshold) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    if (n == 0) return;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * maxDet_);
    check(rf_detect_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_,
                          counts.data()), h_, "RetinaFace::detectBatchImages");
    for (int i = 0; i < n; i++) {
        int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
    }
}

void RetinaFace::detectRedacted(vector<cv::Mat> &imgs, float threshold, const rf_redact_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    redactPixels_.assign(n, vector<int32_t>());
    if (n == 0) return;
    const int regions = spec && spec->max_regions > 0 ? spec->max_regions : (maxDet_ < 1024 ? maxDet_ : 1024);
    vector<const uint8_t *> ptrs(n);
    vector<uint8_t *> outs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = outs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<int32_t> pixels((size_t)n * regions);
    check(rf_detect_redact_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_, counts.data(),
                                 spec, outs.data(), steps.data(), pixels.data()), h_, "RetinaFace::detectRedacted");
    for (int i = 0; i < n; i++) {
        int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
        const int r = k < regions ? k : regions;
        redactPixels_[i].assign(pixels.begin() + (size_t)i * regions, pixels.begin() + (size_t)i * regions + r);
    }
}

void RetinaFace::detectOverlay(vector<cv::Mat> &imgs, float threshold, const rf_overlay_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    overlayPixels_.assign(n, vector<int32_t>());
    if (n == 0) return;
    const int regions = spec && spec->max_regions > 0 ? spec->max_regions : (maxDet_ < 1024 ? maxDet_ : 1024);
    vector<const uint8_t *> ptrs(n);
    vector<uint8_t *> outs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = outs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<int32_t> pixels((size_t)n * regions);
    check(rf_detect_overlay_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_, counts.data(),
                                  spec, outs.data(), steps.data(), pixels.data()), h_, "RetinaFace::detectOverlay");
    for (int i = 0; i < n; i++) {
        int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
        const int r = k < regions ? k : regions;
        overlayPixels_[i].assign(pixels.begin() + (size_t)i * regions, pixels.begin() + (size_t)i * regions + r);
    }
}

void RetinaFace::detectTrackedOverlay(const vector<void *> &deviceFrames, const vector<int> &rows, const vector<int> &cols,
                                      const vector<int> &steps, rf_tracker tracker, const vector<int> &streams, float threshold,
                                      const rf_overlay_spec *spec) {
    const int n = (int)deviceFrames.size();
    if ((int)rows.size() != n || (int)cols.size() != n || (int)steps.size() != n || (int)streams.size() != n)
        throw std::runtime_error("RetinaFace::detectTrackedOverlay: rows, cols, steps and one stream per frame");
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    trackTags_.assign(n, vector<rf_track_tag>());
    trackEnded_.assign(n, vector<rf_track>());
    overlayPixels_.assign(n, vector<int32_t>());
    if (n == 0) return;
    const int capEnded = 256;                          // a table holds at most 256 tracks: no list is ever cut
    const int regions = spec && spec->max_regions > 0 ? spec->max_regions : (maxDet_ < 1024 ? maxDet_ : 1024);
    vector<int> counts(n, 0), endedCounts(n, 0), regionCounts(n, 0);
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<rf_track_tag> tags((size_t)n * maxDet_);
    vector<rf_track> ended((size_t)n * capEnded);
    vector<int32_t> pixels((size_t)n * regions);
    check(rf_detect_track_overlay_batch_device(h_, deviceFrames.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(),
                                               maxDet_, counts.data(), tracker, streams.data(), tags.data(), ended.data(), capEnded,
                                               endedCounts.data(), spec, pixels.data(), regionCounts.data()), h_,
          "RetinaFace::detectTrackedOverlay");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
        trackTags_[i].assign(tags.begin() + (size_t)i * maxDet_, tags.begin() + (size_t)i * maxDet_ + k);
        const int e = endedCounts[i] < capEnded ? endedCounts[i] : capEnded;
        trackEnded_[i].assign(ended.begin() + (size_t)i * capEnded, ended.begin() + (size_t)i * capEnded + e);
        const int r = regionCounts[i] < regions ? regionCounts[i] : regions;
        overlayPixels_[i].assign(pixels.begin() + (size_t)i * regions, pixels.begin() + (size_t)i * regions + r);
    }
}

void RetinaFace::detectTiled(const vector<cv::Mat> &imgs, float threshold, const rf_tile_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    tileSrc_.assign(n, vector<int>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> src((size_t)n * cap, 0);
    check(rf_detect_tiled_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap,
                                counts.data(), src.data()), h_, "RetinaFace::detectTiled");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        tileSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

rf_tracker RetinaFace::createTracker(int nStreams, const rf_track_spec *spec) {
    rf_tracker t = nullptr;
    check(rf_tracker_create(h_, spec, nStreams, &t), h_, "RetinaFace::createTracker");
    return t;
}

void RetinaFace::detectTracked(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold) {
    const int n = (int)imgs.size();
    if ((int)streams.size() != n) throw std::runtime_error("RetinaFace::detectTracked: one stream per image");
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    trackTags_.assign(n, vector<rf_track_tag>());
    trackEnded_.assign(n, vector<rf_track>());
    if (n == 0) return;
    const int capEnded = 256;                          // a table holds at most 256 tracks: no list is ever cut
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), endedCounts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<rf_track_tag> tags((size_t)n * maxDet_);
    vector<rf_track> ended((size_t)n * capEnded);
    check(rf_detect_track_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_, counts.data(),
                                tracker, streams.data(), tags.data(), ended.data(), capEnded, endedCounts.data()), h_,
          "RetinaFace::detectTracked");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
        trackTags_[i].assign(tags.begin() + (size_t)i * maxDet_, tags.begin() + (size_t)i * maxDet_ + k);
        const int e = endedCounts[i] < capEnded ? endedCounts[i] : capEnded;
        trackEnded_[i].assign(ended.begin() + (size_t)i * capEnded, ended.begin() + (size_t)i * capEnded + e);
    }
}

void RetinaFace::enableFollow(rf_tracker tracker, const rf_follow_spec *spec) {
    check(rf_tracker_enable_follow(tracker, spec), h_, "RetinaFace::enableFollow");
}

// key = true: rf_detect_track_follow_batch; false: rf_track_follow_batch (the faces are the followed ones)
static void follow_call(rf_handle h, bool key, const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold, int cap,
                        vector<vector<FaceDetectInfo>> *batch, vector<vector<rf_track_tag>> *trackTags, vector<vector<rf_track>> *trackEnded) {
    const int n = (int)imgs.size();
    if ((int)streams.size() != n) throw std::runtime_error("RetinaFace: one stream per image");
    batch->assign(n, vector<FaceDetectInfo>());
    trackTags->assign(n, vector<rf_track_tag>());
    trackEnded->assign(n, vector<rf_track>());
    if (n == 0) return;
    const int capEnded = 256;                          // a table holds at most 256 tracks: no list is ever cut
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), endedCounts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<rf_track_tag> tags((size_t)n * cap);
    vector<rf_track> ended((size_t)n * capEnded);
    const int st = key ? rf_detect_track_follow_batch(h, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), cap,
                                                      counts.data(), tracker, streams.data(), tags.data(), ended.data(), capEnded, endedCounts.data())
                       : rf_track_follow_batch(h, tracker, ptrs.data(), rows.data(), cols.data(), steps.data(), n, streams.data(), faces.data(), cap,
                                               counts.data(), tags.data(), ended.data(), capEnded, endedCounts.data());
    check(st, h, key ? "RetinaFace::detectTrackFollow" : "RetinaFace::followTracks");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        (*batch)[i].resize(k);
        if (k) memcpy((*batch)[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        (*trackTags)[i].assign(tags.begin() + (size_t)i * cap, tags.begin() + (size_t)i * cap + k);
        const int e = endedCounts[i] < capEnded ? endedCounts[i] : capEnded;
        (*trackEnded)[i].assign(ended.begin() + (size_t)i * capEnded, ended.begin() + (size_t)i * capEnded + e);
    }
}

void RetinaFace::detectTrackFollow(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold) {
    follow_call(h_, true, imgs, tracker, streams, threshold, maxDet_, &lastBatch_, &trackTags_, &trackEnded_);
}

void RetinaFace::followTracks(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams) {
    follow_call(h_, false, imgs, tracker, streams, 0.f, 256, &lastBatch_, &trackTags_, &trackEnded_);
}

void RetinaFace::enableMotion(rf_tracker tracker, const rf_motion_spec *spec) {
    check(rf_tracker_enable_motion(tracker, spec), h_, "RetinaFace::enableMotion");
}

vector<rf_track_motion> RetinaFace::readMotion(rf_tracker tracker, int stream) {
    vector<rf_track_motion> rec(256);                  // a table holds at most 256 tracks
    const int k = rf_tracker_read_motion(tracker, stream, rec.data(), (int)rec.size());
    if (k < 0) check(k, h_, "RetinaFace::readMotion");
    rec.resize(k);
    return rec;
}

rf_face RetinaFace::predictTrack(const rf_track &track, const rf_track_motion &motion, int ahead, const rf_motion_spec *spec) {
    rf_face f;
    if (rf_track_predict(spec, &track, &motion, ahead, &f) != RF_OK)
        throw std::runtime_error("RetinaFace::predictTrack: a free slot, a bad spec or an ahead other than 0 or 1");
    return f;
}

size_t RetinaFace::enableShots(rf_tracker tracker, const rf_face_batch_spec &spec) {
    check(rf_tracker_enable_shots(tracker, &spec), h_, "RetinaFace::enableShots");
    const size_t S = spec.crop_size ? (size_t)spec.crop_size : 112;
    const size_t bytes = 3 * S * S * (spec.format == RF_FACES_F32_CHW ? 4 : spec.format == RF_FACES_F16_CHW ? 2 : 1);
    shotBytes_[tracker] = bytes;
    return bytes;
}

void RetinaFace::detectTrackShots(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold,
                                  const rf_face_gate *gate, int capEnded) {
    const int n = (int)imgs.size();
    if ((int)streams.size() != n) throw std::runtime_error("RetinaFace::detectTrackShots: one stream per image");
    if (!shotBytes_.count(tracker) || capEnded < 1) throw std::runtime_error("RetinaFace::detectTrackShots: enableShots() first, capEnded >= 1");
    const size_t bpf = shotBytes_[tracker];
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    trackTags_.assign(n, vector<rf_track_tag>());
    trackEnded_.assign(n, vector<rf_track>());
    shots_.assign(n, vector<uint8_t>());
    shotInfo_.assign(n, vector<rf_shot>());
    if (n == 0) return;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), endedCounts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<rf_track_tag> tags((size_t)n * maxDet_);
    vector<rf_track> ended((size_t)n * capEnded);
    vector<uint8_t> shots((size_t)n * capEnded * bpf);
    vector<rf_shot> info((size_t)n * capEnded);
    const int st = rf_detect_track_shots_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_,
                                               counts.data(), tracker, streams.data(), tags.data(), ended.data(), capEnded, endedCounts.data(),
                                               gate, nullptr, nullptr, shots.data(), info.data());
    check(st, h_, "RetinaFace::detectTrackShots");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
        trackTags_[i].assign(tags.begin() + (size_t)i * maxDet_, tags.begin() + (size_t)i * maxDet_ + k);
        if (endedCounts[i] > capEnded) throw std::runtime_error("RetinaFace::detectTrackShots: more tracks ended in one frame than capEnded");
        const size_t e = (size_t)endedCounts[i], at = (size_t)i * capEnded;
        trackEnded_[i].assign(ended.begin() + at, ended.begin() + at + e);
        shots_[i].assign(shots.begin() + at * bpf, shots.begin() + (at + e) * bpf);
        shotInfo_[i].assign(info.begin() + at, info.begin() + at + e);
    }
}

vector<rf_track> RetinaFace::flushShots(rf_tracker tracker, int stream, vector<uint8_t> *shots, vector<rf_shot> *info) {
    if (!shotBytes_.count(tracker)) throw std::runtime_error("RetinaFace::flushShots: enableShots() first");
    const size_t bpf = shotBytes_[tracker];
    const int cap = 256;                               // a table holds at most 256 tracks
    vector<rf_track> ended(cap);
    vector<uint8_t> px((size_t)cap * bpf);
    vector<rf_shot> rec(cap);
    const int k = rf_tracker_flush_shots(tracker, stream, ended.data(), cap, nullptr, nullptr, px.data(), rec.data());
    if (k < 0) check(k, h_, "RetinaFace::flushShots");
    ended.resize(k);
    if (shots) shots->assign(px.begin(), px.begin() + (size_t)k * bpf);
    if (info) info->assign(rec.begin(), rec.begin() + k);
    return ended;
}

void RetinaFace::detectTta(const vector<cv::Mat> &imgs, float threshold, const rf_tta_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    ttaVotes_.assign(n, vector<int>());
    ttaPasses_.assign(n, vector<int>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    check(rf_detect_tta_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap, counts.data(),
                              votes.data(), src.data()), h_, "RetinaFace::detectTta");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        ttaVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        ttaPasses_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

void RetinaFace::detectRotated(const vector<cv::Mat> &imgs, float threshold, const rf_rot_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    rotVotes_.assign(n, vector<int>());
    rotSrc_.assign(n, vector<int>());
    frameRot_.assign(n, -1);
    rotScore_.assign((size_t)n * 4, 0.f);
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    check(rf_detect_rot_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap, counts.data(),
                              votes.data(), src.data(), frameRot_.data(), rotScore_.data()), h_, "RetinaFace::detectRotated");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        rotVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        rotSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

rf_dewarper RetinaFace::createDewarper(int rows, int cols, const rf_dewarp_spec &spec, int viewW, int viewH) {
    const int vw = viewW > 0 ? viewW : netW_, vh = viewH > 0 ? viewH : netH_;
    if (vw < 16 || vh < 16 || vw > 4096 || vh > 3072) throw std::runtime_error("RetinaFace::createDewarper: bad view size");
    vector<int32_t> mesh((size_t)RF_DEWARP_MAX_VIEWS * (vw / 16 + 1) * (vh / 16 + 1) * 2);
    int views = 0;
    if (rf_dewarp_plan(&spec, vw, vh, mesh.data(), (int)mesh.size(), &views) != RF_OK)
        throw std::runtime_error("RetinaFace::createDewarper: the spec is not valid, or a view leaves what the lens images");
    rf_dewarper d = nullptr;
    check(rf_dewarper_create(h_, rows, cols, viewW, viewH, views, mesh.data(), &d), h_, "RetinaFace::createDewarper");
    return d;
}

void RetinaFace::detectDewarped(const vector<cv::Mat> &imgs, rf_dewarper dewarper, float threshold, const rf_dewarp_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    dewarpVotes_.assign(n, vector<int>());
    dewarpSrc_.assign(n, vector<int>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    check(rf_detect_dewarp_batch(dewarper, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap,
                                 counts.data(), votes.data(), src.data()), h_, "RetinaFace::detectDewarped");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        dewarpVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        dewarpSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

void RetinaFace::detectRois(const vector<cv::Mat> &imgs, const vector<vector<rf_roi>> &rois, float threshold, const rf_roi_spec *spec) {
    const int n = (int)imgs.size();
    if ((int)rois.size() != n) throw std::runtime_error("RetinaFace::detectRois: one list of regions per frame");
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    roiVotes_.assign(n, vector<int>());
    roiSrc_.assign(n, vector<int>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), roiCounts(n);
    vector<rf_roi> flat;
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
        roiCounts[i] = (int)rois[i].size();
        flat.insert(flat.end(), rois[i].begin(), rois[i].end());
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    check(rf_detect_roi_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, flat.data(), roiCounts.data(), threshold, spec,
                              faces.data(), cap, counts.data(), votes.data(), src.data()), h_, "RetinaFace::detectRois");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        roiVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        roiSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

void RetinaFace::detectTrackedRois(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold,
                                   const rf_roi_spec *spec, int margin_q8) {
    const int n = (int)imgs.size();
    if ((int)streams.size() != n) throw std::runtime_error("RetinaFace::detectTrackedRois: one stream per image");
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    roiVotes_.assign(n, vector<int>());
    roiSrc_.assign(n, vector<int>());
    trackTags_.assign(n, vector<rf_track_tag>());
    trackEnded_.assign(n, vector<rf_track>());
    roiCells_.assign(n, vector<rf_roi_cell>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_, capEnded = 256, maxTracks = 256;      // no list is ever cut
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), endedCounts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    int T = 0;                                         // the tracker's max_tracks: what rf_tracker_read returns for cap 0
    for (int i = 0; i < n && T == 0; i++)
        if (streams[i] >= 0) T = rf_tracker_read(tracker, streams[i], nullptr, 0, nullptr, nullptr);
    if (T < 0) check(T, h_, "RetinaFace::detectTrackedRois");
    if (T == 0 || T > maxTracks) T = maxTracks;
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    vector<rf_track_tag> tags((size_t)n * cap);
    vector<rf_track> ended((size_t)n * capEnded);
    vector<rf_roi_cell> cells((size_t)n * T);
    check(rf_detect_track_roi_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, margin_q8, faces.data(), cap,
                                    counts.data(), src.data(), votes.data(), cells.data(), nullptr, tracker, streams.data(), tags.data(),
                                    ended.data(), capEnded, endedCounts.data()), h_, "RetinaFace::detectTrackedRois");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        roiVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        roiSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
        trackTags_[i].assign(tags.begin() + (size_t)i * cap, tags.begin() + (size_t)i * cap + k);
        const int e = endedCounts[i] < capEnded ? endedCounts[i] : capEnded;
        trackEnded_[i].assign(ended.begin() + (size_t)i * capEnded, ended.begin() + (size_t)i * capEnded + e);
        roiCells_[i].assign(cells.begin() + (size_t)i * T, cells.begin() + (size_t)(i + 1) * T);
    }
}

rf_changer RetinaFace::createChanger(int rows, int cols, int nStreams, const rf_change_spec *spec) {
    rf_changer c = nullptr;
    check(rf_changer_create(h_, spec, rows, cols, nStreams, &c), h_, "RetinaFace::createChanger");
    changers_.push_back(ChangerShape{c, rows, cols, spec && spec->max_regions > 0 ? spec->max_regions : 16});      // (the header's default)
    return c;
}

vector<vector<rf_roi_cell>> RetinaFace::changeRegions(rf_changer changer, const vector<const void *> &dFrames, const vector<int> &steps,
                                                      const vector<int> &streams, const rf_roi_spec *spec, int margin_q8) {
    const int n = (int)dFrames.size();
    if ((int)streams.size() != n || (int)steps.size() != n) throw std::runtime_error("RetinaFace::changeRegions: one step and one stream per frame");
    const ChangerShape *cs = nullptr;
    for (const ChangerShape &c : changers_)
        if (c.changer == changer) cs = &c;
    if (!cs) throw std::runtime_error("RetinaFace::changeRegions: not a changer of this object");
    vector<int> rows(n), cols(n);
    for (int i = 0; i < n; i++) { rows[i] = dFrames[i] ? cs->rows : 0; cols[i] = dFrames[i] ? cs->cols : 0; }
    vector<rf_roi_cell> cells((size_t)n * cs->regions);
    changeInfo_.assign(n, rf_change_info{0, 0, 0, 0});
    vector<vector<rf_roi_cell>> out(n);
    if (n == 0) return out;
    check(rf_change_regions_device(h_, changer, dFrames.data(), rows.data(), cols.data(), steps.data(), streams.data(), n, margin_q8, spec,
                                   cells.data(), changeInfo_.data()), h_, "RetinaFace::changeRegions");
    for (int i = 0; i < n; i++) out[i].assign(cells.begin() + (size_t)i * cs->regions, cells.begin() + (size_t)(i + 1) * cs->regions);
    return out;
}

void RetinaFace::detectChanged(const vector<cv::Mat> &imgs, rf_changer changer, const vector<int> &streams, rf_tracker tracker, float threshold,
                               const rf_roi_spec *spec, int margin_q8) {
    const int n = (int)imgs.size();
    if ((int)streams.size() != n) throw std::runtime_error("RetinaFace::detectChanged: one stream per image");
    const ChangerShape *cs = nullptr;
    for (const ChangerShape &c : changers_)
        if (c.changer == changer) cs = &c;
    if (!cs) throw std::runtime_error("RetinaFace::detectChanged: not a changer of this object");
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    roiVotes_.assign(n, vector<int>());
    roiSrc_.assign(n, vector<int>());
    trackTags_.assign(n, vector<rf_track_tag>());
    trackEnded_.assign(n, vector<rf_track>());
    roiCells_.assign(n, vector<rf_roi_cell>());
    changeInfo_.assign(n, rf_change_info{0, 0, 0, 0});
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_, capEnded = 256;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0), endedCounts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    int T = 0;                                         // the tracker's max_tracks: what rf_tracker_read returns for cap 0
    if (tracker) {
        T = rf_tracker_read(tracker, 0, nullptr, 0, nullptr, nullptr);
        if (T < 0) check(T, h_, "RetinaFace::detectChanged");
    }
    const int S = T + cs->regions;
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    vector<rf_track_tag> tags((size_t)n * cap);
    vector<rf_track> ended((size_t)n * capEnded);
    vector<rf_roi_cell> cells((size_t)n * S);
    check(rf_detect_change_roi_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, margin_q8, faces.data(), cap,
                                     counts.data(), src.data(), votes.data(), cells.data(), nullptr, changer, changeInfo_.data(), tracker,
                                     streams.data(), tracker ? tags.data() : nullptr, tracker ? ended.data() : nullptr, tracker ? capEnded : 0,
                                     tracker ? endedCounts.data() : nullptr), h_, "RetinaFace::detectChanged");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        roiVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        roiSrc_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
        roiCells_[i].assign(cells.begin() + (size_t)i * S, cells.begin() + (size_t)(i + 1) * S);
        if (!tracker) continue;
        trackTags_[i].assign(tags.begin() + (size_t)i * cap, tags.begin() + (size_t)i * cap + k);
        const int e = endedCounts[i] < capEnded ? endedCounts[i] : capEnded;
        trackEnded_[i].assign(ended.begin() + (size_t)i * capEnded, ended.begin() + (size_t)i * capEnded + e);
    }
}

vector<rf_roi> RetinaFace::roisFromFaces(const vector<FaceDetectInfo> &faces, float coordScale, int margin_q8) {
    static_assert(sizeof(FaceDetectInfo) == sizeof(rf_face), "a FaceDetectInfo is an rf_face");
    vector<rf_roi> out(faces.size());
    const int k = rf_roi_from_faces((const rf_face *)faces.data(), (int)faces.size(), coordScale, margin_q8, out.data());
    if (k < 0) throw std::runtime_error("RetinaFace::roisFromFaces: bad coordScale or margin");
    out.resize((size_t)k);
    return out;
}

void RetinaFace::detectEnhanced(const vector<cv::Mat> &imgs, float threshold, const rf_enhance_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    tilesEnhanced_.assign(n, 0);
    if (n == 0) return;
    const int cap = maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    check(rf_detect_enhanced_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap,
                                   counts.data(), nullptr, nullptr, tilesEnhanced_.data()), h_, "RetinaFace::detectEnhanced");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
    }
}

void RetinaFace::detectPyramid(const vector<cv::Mat> &imgs, float threshold, const rf_pyramid_spec *spec) {
    const int n = (int)imgs.size();
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    pyrVotes_.assign(n, vector<int>());
    pyrPasses_.assign(n, vector<int>());
    if (n == 0) return;
    const int cap = spec && spec->max_faces > 0 ? spec->max_faces : maxDet_;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    vector<rf_face> faces((size_t)n * cap);
    vector<int> votes((size_t)n * cap, 0), src((size_t)n * cap, 0);
    check(rf_detect_pyramid_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, spec, faces.data(), cap,
                                  counts.data(), votes.data(), src.data()), h_, "RetinaFace::detectPyramid");
    for (int i = 0; i < n; i++) {
        const int k = counts[i] < cap ? counts[i] : cap;
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * cap], (size_t)k * sizeof(rf_face));
        pyrVotes_[i].assign(votes.begin() + (size_t)i * cap, votes.begin() + (size_t)i * cap + k);
        pyrPasses_[i].assign(src.begin() + (size_t)i * cap, src.begin() + (size_t)i * cap + k);
    }
}

void RetinaFace::detectPad32(const Mat &img, float threshold) {
    last_.clear();
    if (img.empty()) return;                       // RetinaFace.cpp:945-947
    const uint8_t *ptr = img.data;
    int rows = img.rows, cols = img.cols, step = (int)(size_t)img.step, count = 0;
    vector<rf_face> faces(maxDet_);
    check(rf_detect_batch_pad32(h_, &ptr, &rows, &cols, &step, 1, 0, threshold, faces.data(), maxDet_, &count), h_, "RetinaFace::detectPad32");
    int k = count < maxDet_ ? count : maxDet_;
    last_.resize(k);
    if (k) memcpy(last_.data(), faces.data(), (size_t)k * sizeof(rf_face));
}

void RetinaFace::detect(const Mat &img, float threshold, float /*scales: unused in the reference too*/) {
    last_.clear();
    if (img.empty()) return;                       // RetinaFace.cpp:578-580
    const uint8_t *ptr = img.data;
    int rows = img.rows, cols = img.cols, step = (int)(size_t)img.step, count = 0;
    vector<rf_face> faces(maxDet_);
    check(rf_detect_batch(h_, &ptr, &rows, &cols, &step, 1, threshold, faces.data(), maxDet_, &count), h_, "RetinaFace::detect");
    int k = count < maxDet_ ? count : maxDet_;
    last_.resize(k);
    if (k) memcpy(last_.data(), faces.data(), (size_t)k * sizeof(rf_face));
}

vector<cv::Mat> RetinaFace::detectAndAlign(const Mat &img, float threshold, int cropSize) {
    last_.clear();
    alignMats_.clear();
    vector<cv::Mat> crops;
    if (img.empty()) return crops;
    const uint8_t *ptr = img.data;
    int rows = img.rows, cols = img.cols, step = (int)(size_t)img.step, count = 0;
    if (cropSize < 16 || cropSize > 512) throw std::runtime_error("RetinaFace::detectAndAlign: cropSize must be in [16, 512]");
    const size_t cb = (size_t)cropSize * cropSize * 3;
    vector<rf_face> faces(maxDet_);
    vector<uint8_t> buf((size_t)maxDet_ * cb);
    vector<double> mats((size_t)maxDet_ * 6);
    check(rf_detect_align_batch(h_, &ptr, &rows, &cols, &step, 1, threshold, faces.data(), maxDet_, &count, cropSize, maxDet_, nullptr,
                                buf.data(), mats.data()), h_, "RetinaFace::detectAndAlign");
    int k = count < maxDet_ ? count : maxDet_;
    last_.resize(k);
    if (k) memcpy(last_.data(), faces.data(), (size_t)k * sizeof(rf_face));
    alignMats_.assign(mats.begin(), mats.begin() + (size_t)k * 6);
    for (int i = 0; i < k; i++) {
        cv::Mat m(cropSize, cropSize, CV_8UC3);
        memcpy(m.data, buf.data() + (size_t)i * cb, cb);
        crops.push_back(m);
    }
    return crops;
}

vector<uint8_t> RetinaFace::detectFaceBatch(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec) {
    return faceBatchCall(imgs, threshold, spec, false, nullptr);
}

vector<uint8_t> RetinaFace::detectFaceBatchGated(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec,
                                                 const rf_face_gate *gate) {
    return faceBatchCall(imgs, threshold, spec, true, gate);
}

vector<uint8_t> RetinaFace::faceBatchCall(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec, bool gated,
                                          const rf_face_gate *gate) {
    const int n = (int)imgs.size();
    faceQuality_.clear();
    faceQualityStride_ = 0;
    lastBatch_.assign(n, vector<FaceDetectInfo>());
    faceOffsets_.assign((size_t)n + 1, 0);
    faceMats_.clear();
    faceTruncated_ = false;
    vector<const uint8_t *> ptrs(n);
    vector<int> rows(n), cols(n), steps(n), counts(n, 0);
    for (int i = 0; i < n; i++) {
        ptrs[i] = imgs[i].empty() ? nullptr : imgs[i].data;
        rows[i] = imgs[i].rows; cols[i] = imgs[i].cols; steps[i] = (int)(size_t)imgs[i].step;
    }
    size_t bpf = 0;
    if (rf_face_batch_plan(&spec, nullptr, 0, nullptr, &bpf) < 0) throw std::runtime_error("RetinaFace::detectFaceBatch: bad rf_face_batch_spec");
    vector<rf_face> faces((size_t)n * maxDet_);
    vector<uint8_t> tensor((size_t)spec.capacity * bpf);
    vector<double> mats((size_t)spec.capacity * 6);
    if (gated) {
        faceQualityStride_ = spec.max_faces ? spec.max_faces : maxDet_;
        faceQuality_.assign((size_t)n * faceQualityStride_, rf_face_quality());
        check(rf_detect_face_batch_gated(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_,
                                         counts.data(), &spec, nullptr, tensor.data(), mats.data(), faceOffsets_.data(), gate,
                                         faceQuality_.data()), h_, "RetinaFace::detectFaceBatchGated");
    } else {
        check(rf_detect_face_batch(h_, ptrs.data(), rows.data(), cols.data(), steps.data(), n, threshold, faces.data(), maxDet_, counts.data(),
                                   &spec, nullptr, tensor.data(), mats.data(), faceOffsets_.data()), h_, "RetinaFace::detectFaceBatch");
    }
    for (int i = 0; i < n; i++) {
        int k = counts[i] < maxDet_ ? counts[i] : maxDet_;
        for (int j = k < faceQualityStride_ ? k : faceQualityStride_; j < faceQualityStride_; j++)
            faceQuality_[(size_t)i * faceQualityStride_ + j] = rf_face_quality();      // slots without a considered face
        lastBatch_[i].resize(k);
        if (k) memcpy(lastBatch_[i].data(), &faces[(size_t)i * maxDet_], (size_t)k * sizeof(rf_face));
    }
    const int total = faceOffsets_[n];
    faceTruncated_ = total > spec.capacity;
    const size_t got = (size_t)(faceTruncated_ ? spec.capacity : total);
    tensor.resize(got * bpf);
    faceMats_.assign(mats.begin(), mats.begin() + got * 6);
    return tensor;
}
