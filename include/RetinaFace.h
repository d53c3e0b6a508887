/*
 * RetinaFace.h -- drop-in for the reference's detector class (retinaface/RetinaFace.h:63-78): the same
 * constructor, detect() and detectBatchImages() signatures and the same public result PODs
 * (anchor_box, FacePts, FaceDetectInfo: retinaface/RetinaFace.h:15-42), implemented on the MI355X engine
 * behind include/retinaface_amd.h instead of TensorRT + NPP + CPU loops.
 *
 * Differences a caller can observe, all additive:
 *   - detect()/detectBatchImages() return void in the reference and drop their result
 *     (RetinaFace.cpp:726-747, :916-939); here the detections stay available through lastResult() /
 *     lastBatchResult() until the next call.  Coordinates are network-input pixels, as in the reference.
 *   - a second constructor takes rf_options (precision, net size, batch, model stem) -- the reference bakes
 *     these in at compile time / in prototxt line 7.
 *   - errors throw std::runtime_error instead of abort()/exit(0).
 *   - detectAndAlign() also returns each face as an aligned crop, the input of the recogniser that usually follows;
 *     detectFaceBatch() returns the faces of a batch of frames as one dense tensor in the recogniser's layout and number format.
 */
#ifndef RETINAFACE_H
#define RETINAFACE_H

#include <map>
#include <string>
#include <vector>

#if !defined(RF_NO_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define RF_HAVE_OPENCV 1
#endif
#endif
#ifndef RF_HAVE_OPENCV
#include "rf_mat.h"
#endif
#include "retinaface_amd.h"

using namespace cv;
using namespace std;

struct anchor_win { float x_ctr, y_ctr, w, h; };
struct anchor_box { float x1, y1, x2, y2; };
struct FacePts { float x[5]; float y[5]; };
struct FaceDetectInfo { float score; anchor_box rect; FacePts pts; };

struct anchor_cfg {
    int STRIDE = 0;
    vector<int> SCALES;
    int BASE_SIZE = 0;
    vector<float> RATIOS;
    int ALLOWED_BORDER = 0;
};

class RetinaFace {
public:
    RetinaFace(string &model, string network = "net3", float nms = 0.4);
    RetinaFace(const string &model, const rf_options &options, string network = "net3", float nms = 0.4);
    ~RetinaFace();
    RetinaFace(const RetinaFace &) = delete;
    RetinaFace &operator=(const RetinaFace &) = delete;

    void detectBatchImages(vector<cv::Mat> imgs, float threshold = 0.5);
    void detect(const Mat &img, float threshold = 0.5, float scales = 1.0);

    /* the reference's Caffe-build detect (`void detect(Mat img, ...)`, RetinaFace.cpp:943-1075; it cannot share the name with
       the TensorRT-build signature above, RetinaFace.h:70): no resize, pad to x32, run at that size; result in lastResult() */
    void detectPad32(const Mat &img, float threshold = 0.5);

    /* additive: detect() + the faces warped onto the five-landmark recognition template (rf_detect_align_batch): one
       cropSize x cropSize CV_8UC3 BGR crop per face of lastResult(), in the same order, sampled from `img` at its full
       resolution; alignMatrices() holds their forward matrices (source pixels -> crop pixels, 6 doubles each) */
    vector<cv::Mat> detectAndAlign(const Mat &img, float threshold = 0.5, int cropSize = 112);
    const vector<double> &alignMatrices() const { return alignMats_; }

    /* additive: detectBatchImages() + the faces it finds as ONE dense, packed, normalised tensor (rf_detect_face_batch): the bytes of
       min(total, spec.capacity) faces of 3 x S x S elements each in the spec's format; face k of image i is packed face
       faceBatchOffsets()[i] + k, faceBatchMatrices() holds 6 doubles per packed face.  Fills lastBatchResult().
       faceBatchTruncated(): more faces than spec.capacity (the first `capacity` are returned).
       spec.antialias = 1 supersamples faces that are larger in the frame than their crop (up to spec.aa_max sub-samples per axis);
       under detectFaceBatchGated() the luma numbers of the quality records are then those of the antialiased crop. */
    vector<uint8_t> detectFaceBatch(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec);
    const vector<int> &faceBatchOffsets() const { return faceOffsets_; }
    const vector<double> &faceBatchMatrices() const { return faceMats_; }
    bool faceBatchTruncated() const { return faceTruncated_; }

    /* additive: detectFaceBatch() behind a quality gate (rf_detect_face_batch_gated): only the faces the gate keeps are packed, the
       offsets count kept faces.  gate may be nullptr (every face is kept: the bytes of detectFaceBatch).  faceBatchQuality() holds
       n x faceBatchQualityStride() records: the record of face k of image i, kept or dropped, is [i * stride + k] for
       k < min(faces of image i, stride); the other records are zero. */
    vector<uint8_t> detectFaceBatchGated(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec,
                                         const rf_face_gate *gate);
    const vector<rf_face_quality> &faceBatchQuality() const { return faceQuality_; }
    int faceBatchQualityStride() const { return faceQualityStride_; }

    /* additive: tiled detection (rf_detect_tiled_batch): frames larger than the net are cut into overlapping net-sized tiles that are
       detected at 1:1 and merged on the device, so small faces in large frames are not shrunk away.  Fills lastBatchResult() with the
       merged faces in SOURCE-FRAME pixels (at most spec->max_faces per frame); tileSources() holds, per frame, the pass of the frame's
       plan (rf_tile_plan) each face came from.  spec may be nullptr (the defaults). */
    void detectTiled(const vector<cv::Mat> &imgs, float threshold = 0.5, const rf_tile_spec *spec = nullptr);
    const vector<vector<int>> &tileSources() const { return tileSrc_; }

    /* additive: flip test-time augmentation (rf_detect_tta_batch): every frame is also detected mirrored left-right, the mirrored faces
       are moved back and overlapping boxes are merged on the device into a score-weighted mean.  Fills lastBatchResult() with the merged
       faces in SOURCE-FRAME pixels (at most spec->max_faces per frame); ttaVotes() holds, per frame, how many candidates each face
       merged, ttaPasses() the pass (0: the frame, 1: mirrored) its head came from.  spec may be nullptr (the defaults). */
    void detectTta(const vector<cv::Mat> &imgs, float threshold = 0.5, const rf_tta_spec *spec = nullptr);
    const vector<vector<int>> &ttaVotes() const { return ttaVotes_; }
    const vector<vector<int>> &ttaPasses() const { return ttaPasses_; }

    /* additive: rotation-robust detection (rf_detect_rot_batch): every frame is also detected turned by one, two and three quarter turns
       (the copies are made on the device), the faces of all passes are moved back and merged on the device.  Fills lastBatchResult()
       with the merged faces in SOURCE-FRAME pixels (at most spec->max_faces per frame); rotVotes() holds, per frame, how many
       candidates each face merged, rotSources() the rotation (0..3) its head came from, frameRotations() per frame the quarter turns
       counter-clockwise that make it upright (-1: no face), rotScores() per frame the four score sums.  spec may be nullptr. */
    void detectRotated(const vector<cv::Mat> &imgs, float threshold = 0.5, const rf_rot_spec *spec = nullptr);
    const vector<vector<int>> &rotVotes() const { return rotVotes_; }
    const vector<vector<int>> &rotSources() const { return rotSrc_; }
    const vector<int> &frameRotations() const { return frameRot_; }
    const vector<float> &rotScores() const { return rotScore_; }

    /* additive: fisheye detection (rf_dewarper_create / rf_detect_dewarp_batch): createDewarper() makes a dewarper on this handle for
       rows x cols frames -- the meshes planned from spec (rf_dewarp_plan) at viewW x viewH (0: the net size) -- which the destructor
       frees; detectDewarped() detects every frame in the dewarper's views, made on the device, and merges the faces moved back through
       the meshes.  Fills lastBatchResult() with the merged faces in SOURCE-FRAME pixels (at most spec->max_faces per frame; only vote,
       max_faces and edge of spec are read, nullptr: the defaults); dewarpVotes() holds, per frame, how many candidates each face
       merged, dewarpViews() the view its head came from. */
    rf_dewarper createDewarper(int rows, int cols, const rf_dewarp_spec &spec, int viewW = 0, int viewH = 0);
    void detectDewarped(const vector<cv::Mat> &imgs, rf_dewarper dewarper, float threshold = 0.5, const rf_dewarp_spec *spec = nullptr);
    const vector<vector<int>> &dewarpVotes() const { return dewarpVotes_; }
    const vector<vector<int>> &dewarpViews() const { return dewarpSrc_; }

    /* additive: region detection (rf_detect_roi_batch): every frame is detected only in its regions (rois[i]: frame i's, at most 256),
       which are packed several to a net-sized view on the device; the faces are moved back and merged.  Fills lastBatchResult() with
       the merged faces in SOURCE-FRAME pixels (at most spec->max_faces per frame; nullptr: the defaults); roiVotes() holds, per frame,
       how many candidates each face merged, roiRegions() the region it came from.  roisFromFaces() turns a frame's faces into the
       regions of the next call (rf_roi_from_faces; margin_q8 0: a quarter of the longer side). */
    void detectRois(const vector<cv::Mat> &imgs, const vector<vector<rf_roi>> &rois, float threshold = 0.5, const rf_roi_spec *spec = nullptr);
    const vector<vector<int>> &roiVotes() const { return roiVotes_; }
    const vector<vector<int>> &roiRegions() const { return roiSrc_; }
    static vector<rf_roi> roisFromFaces(const vector<FaceDetectInfo> &faces, float coordScale = 1.f, int margin_q8 = 0);

    /* additive: tracked region detection (rf_detect_track_roi_batch): the regions of frame i are planned on the device from the table
       of stream streams[i] of `tracker` (slot r is region r; a free slot is a void cell; -1: no regions, no faces, no step), and the
       merged faces go straight into the frame step -- "key frame (detectTracked), then regions around the faces of the last frame"
       with no host step in between.  Fills lastBatchResult() (SOURCE-FRAME pixels), roiVotes(), roiRegions() (the slot whose region
       found the face), lastTrackTags(), lastEndedTracks() and trackedRoiCells() (per frame the max_tracks records the device
       planned).  margin_q8 0: a quarter of the longer side.  Each stream at most once per call. */
    void detectTrackedRois(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold = 0.5,
                           const rf_roi_spec *spec = nullptr, int margin_q8 = 0);
    const vector<vector<rf_roi_cell>> &trackedRoiCells() const { return roiCells_; }

    /* additive: change regions (rf_changer_create / rf_change_regions_device / rf_detect_change_roi_batch): createChanger() makes a
       changer on this handle for frames of rows x cols and nStreams streams (freed with the handle, or by rf_changer_destroy).
       changeRegions() runs the two kernels alone over frames in DEVICE memory: it steps the references and returns, per frame, the
       spec's max_regions cell records; changeInfo() holds the info records.  detectChanged() is the fused call over host frames: the
       references of streams[i] step, every frame is detected inside its change regions -- with a tracker (may be null) also inside
       the regions of its stream's track slots, region r < max_tracks being slot r -- and the merged faces go into the frame step.
       Fills lastBatchResult() (SOURCE-FRAME pixels), roiVotes(), roiRegions(), trackedRoiCells() (per frame the T + R records),
       changeInfo() and, with a tracker, lastTrackTags() and lastEndedTracks(). */
    rf_changer createChanger(int rows, int cols, int nStreams = 1, const rf_change_spec *spec = nullptr);
    vector<vector<rf_roi_cell>> changeRegions(rf_changer changer, const vector<const void *> &dFrames, const vector<int> &steps,
                                              const vector<int> &streams, const rf_roi_spec *spec = nullptr, int margin_q8 = 0);
    void detectChanged(const vector<cv::Mat> &imgs, rf_changer changer, const vector<int> &streams, rf_tracker tracker = nullptr,
                       float threshold = 0.5, const rf_roi_spec *spec = nullptr, int margin_q8 = 0);
    const vector<rf_change_info> &changeInfo() const { return changeInfo_; }

    /* additive: low-light detection (rf_detect_enhanced_batch): every frame is enhanced on the device (tile-adaptive contrast boost of
       dark tiles, rf_enhance_spec) and detected; the frames themselves are not written.  Fills lastBatchResult() with what the plain
       batch call returns for the enhanced frames; tilesEnhanced() holds, per frame, the number of tiles the enhancement touched
       (0: the detector saw the frame as it is).  spec may be nullptr. */
    void detectEnhanced(const vector<cv::Mat> &imgs, float threshold = 0.5, const rf_enhance_spec *spec = nullptr);
    const vector<int> &tilesEnhanced() const { return tilesEnhanced_; }

    /* additive: zoom-pyramid detection (rf_detect_pyramid_batch): every frame is detected at 1x and as net-sized tiles of the frame enlarged
       2x / 4x on the device, so that faces below the smallest anchor are found; the faces of all passes are moved back and merged as in
       detectTta().  Fills lastBatchResult() with the merged faces in SOURCE-FRAME pixels (at most spec->max_faces per frame);
       pyramidVotes() holds, per frame, how many candidates each face merged, pyramidPasses() the pass of the plan (rf_pyramid_plan) its
       head came from.  spec may be nullptr (the defaults: 1x and 2x). */
    void detectPyramid(const vector<cv::Mat> &imgs, float threshold = 0.5, const rf_pyramid_spec *spec = nullptr);
    const vector<vector<int>> &pyramidVotes() const { return pyrVotes_; }
    const vector<vector<int>> &pyramidPasses() const { return pyrPasses_; }

    /* additive: face tracks (rf_tracker_create / rf_detect_track_batch): createTracker() makes a tracker on this handle (spec may be
       nullptr: the defaults; the destructor frees it); detectTracked() is detectBatchImages() plus one frame step per image of stream
       streams[i] (-1: not tracked), with the tracks in source-frame pixels.  lastTrackTags()[i][k] is the tag of face k of
       lastBatchResult()[i]; lastEndedTracks()[i] the tracks that ended in image i's step. */
    rf_tracker createTracker(int nStreams = 1, const rf_track_spec *spec = nullptr);
    void detectTracked(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold = 0.5);
    const vector<vector<rf_track_tag>> &lastTrackTags() const { return trackTags_; }
    const vector<vector<rf_track>> &lastEndedTracks() const { return trackEnded_; }

    /* additive: motion-predicted tracks (rf_tracker_enable_motion): enableMotion() gives a tracker a velocity per track (spec may be
       nullptr: the defaults) before its first frame step; every tracked call then matches and coasts at the predicted boxes.
       readMotion() returns a stream's records, one per slot; predictTrack() is rf_track_predict: the face a live track is expected
       at, ahead = 0 (where redaction coasts) or 1 (where the next frame step matches). */
    void enableMotion(rf_tracker tracker, const rf_motion_spec *spec = nullptr);
    vector<rf_track_motion> readMotion(rf_tracker tracker, int stream);
    static rf_face predictTrack(const rf_track &track, const rf_track_motion &motion, int ahead = 1, const rf_motion_spec *spec = nullptr);

    /* additive: followed tracks (rf_tracker_enable_follow / rf_detect_track_follow_batch / rf_track_follow_batch): enableFollow() gives a
       tracker a luma template per track (spec may be nullptr: radius 8, max_mad 16, max_run 8); such a tracker is stepped with
       detectTrackFollow() on key frames -- detectTracked() plus the templates of the matched and opened tracks -- and with followTracks()
       on the frames in between, which runs no forward pass: every live track's box is moved to where a block-matching search finds its
       template in the new frame.  followTracks() fills lastBatchResult()[i] with the followed faces of stream streams[i] (slot order,
       the score copied), lastTrackTags()[i] with their tags (RF_TRACK_FOLLOWED) and lastEndedTracks()[i].  Each stream at most once per
       call. */
    void enableFollow(rf_tracker tracker, const rf_follow_spec *spec = nullptr);
    void detectTrackFollow(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold = 0.5);
    void followTracks(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams);

    /* additive: best-shot gallery (rf_tracker_enable_shots / rf_detect_track_shots_batch): enableShots() gives a tracker a gallery of
       face-batch crops (spec as detectFaceBatch(); capacity is not used) and returns the bytes of one shot; from then on the tracker is
       stepped with detectTrackShots(), which is detectTracked() plus the shots of the tracks that end: lastShots()[i] holds
       lastEndedTracks()[i].size() shots back to back, lastShotInfo()[i] their records.  With a gate the best shot goes by sharpness among
       the faces the gate keeps, otherwise by score.  capEnded: ended tracks reported per image (more than that throws).  flushShots()
       ends a stream's live tracks and returns them with their shots. */
    size_t enableShots(rf_tracker tracker, const rf_face_batch_spec &spec);
    void detectTrackShots(const vector<cv::Mat> &imgs, rf_tracker tracker, const vector<int> &streams, float threshold = 0.5,
                          const rf_face_gate *gate = nullptr, int capEnded = 64);
    const vector<vector<uint8_t>> &lastShots() const { return shots_; }
    const vector<vector<rf_shot>> &lastShotInfo() const { return shotInfo_; }
    vector<rf_track> flushShots(rf_tracker tracker, int stream, vector<uint8_t> *shots, vector<rf_shot> *info);

    /* additive: face redaction (rf_detect_redact_batch): detectBatchImages() plus redaction of the faces it finds, IN PLACE in the Mats'
       pixels (pixelate, blur -- rf_redact_spec.blur -- or fill, rectangle or ellipse: rf_redact_spec; nullptr = the defaults).  Fills
       lastBatchResult();
       redactedPixels()[i][k] is the number of pixels face k of image i owns. */
    void detectRedacted(vector<cv::Mat> &imgs, float threshold = 0.5, const rf_redact_spec *spec = nullptr);
    const vector<vector<int32_t>> &redactedPixels() const { return redactPixels_; }

    /* additive: overlays (rf_detect_overlay_batch / rf_detect_track_overlay_batch_device): what the reference's detect() ends with,
       cv::rectangle + cv::circle per face, on the device.  detectOverlay() is detectBatchImages() plus boxes, landmark discs and
       optional score labels drawn IN PLACE into the Mats' pixels (rf_overlay_spec; nullptr = the reference's look).
       detectTrackedOverlay() is the tracked call on frames that already live in device memory (pointer, rows, cols and row step per
       frame): ids as labels or colours, coasting tracks dashed; it fills lastBatchResult(), lastTrackTags() and lastEndedTracks().
       overlayPixels()[i][r] is the number of pixels region r of image i painted. */
    void detectOverlay(vector<cv::Mat> &imgs, float threshold = 0.5, const rf_overlay_spec *spec = nullptr);
    void detectTrackedOverlay(const vector<void *> &deviceFrames, const vector<int> &rows, const vector<int> &cols, const vector<int> &steps,
                              rf_tracker tracker, const vector<int> &streams, float threshold = 0.5, const rf_overlay_spec *spec = nullptr);
    const vector<vector<int32_t>> &overlayPixels() const { return overlayPixels_; }

    /* `scale` of RetinaFace.cpp:585-589: multiply lastResult() coordinates by it for source-frame pixels (:732-739, commented) */
    float frameScale(const Mat &img) const { return rf_frame_scale(h_, img.rows, img.cols); }

    /* additive accessors */
    const vector<FaceDetectInfo> &lastResult() const { return last_; }
    const vector<vector<FaceDetectInfo>> &lastBatchResult() const { return lastBatch_; }
    int netWidth() const { return netW_; }
    int netHeight() const { return netH_; }
    rf_handle handle() const { return h_; }

private:
    void init(const string &model, const rf_options *options, const string &network, float nms);
    rf_handle h_ = nullptr;
    int netW_ = 0, netH_ = 0, maxDet_ = 256;
    string network;
    float nms_threshold;
    vector<FaceDetectInfo> last_;
    vector<vector<FaceDetectInfo>> lastBatch_;
    vector<double> alignMats_;
    vector<int> faceOffsets_;
    vector<double> faceMats_;
    bool faceTruncated_ = false;
    vector<rf_face_quality> faceQuality_;
    int faceQualityStride_ = 0;
    vector<vector<int>> tileSrc_;
    vector<vector<int>> ttaVotes_, ttaPasses_;
    vector<vector<int>> pyrVotes_, pyrPasses_;
    vector<vector<int>> rotVotes_, rotSrc_;
    vector<vector<int>> dewarpVotes_, dewarpSrc_;
    vector<vector<int>> roiVotes_, roiSrc_;
    vector<int> tilesEnhanced_;
    vector<int> frameRot_;
    vector<float> rotScore_;
    vector<vector<rf_track_tag>> trackTags_;
    vector<vector<rf_roi_cell>> roiCells_;
    vector<rf_change_info> changeInfo_;
    struct ChangerShape { rf_changer changer; int rows, cols, regions; };
    vector<ChangerShape> changers_;
    vector<vector<rf_track>> trackEnded_;
    vector<vector<int32_t>> redactPixels_;
    vector<vector<int32_t>> overlayPixels_;
    map<rf_tracker, size_t> shotBytes_;
    vector<vector<uint8_t>> shots_;
    vector<vector<rf_shot>> shotInfo_;
    vector<uint8_t> faceBatchCall(const vector<cv::Mat> &imgs, float threshold, const rf_face_batch_spec &spec, bool gated,
                                  const rf_face_gate *gate);
};

#endif /* RETINAFACE_H */
