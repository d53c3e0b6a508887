// engine.h -- the device-side engine behind the C ABI: owns the stream, the packed weights, the NHWC
// activation buffers and the per-batch-size hipGraphs.  Replaces TrtRetinaFaceNet (trtretinafacenet.cpp:
// allocateMemory :146-210, doInference :48-102, blob_by_name :104-114) + the decode/NMS half of
// RetinaFace::detect (RetinaFace.cpp:666-726).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/retinaface_amd.h"
#include "kernels.h"
#include "plan.h"

namespace rf {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };

struct EngineOptions {
    int precision = RF_PRECISION_FP16;
    int net_h = 0, net_w = 0;
    int max_batch = 8;
    int device = -1;
    int max_candidates = 4096;
    int max_detections = 256;
    bool use_graph = true;
    int lanes = 3;                   // launches in flight (each lane has its own stream + buffers + graphs)
    int coalesce = 0;                // enqueued batches merged into one launch (max_batch * coalesce images; 0 = about 256 images of 448 x 448 per launch): the kernels are
                                     // persistent and pipeline tile t+1's loads under tile t's compute, which pays off once
                                     // a launch holds several tiles per resident workgroup (measured: 4 -> 16 = +8 %)
    bool keep_outputs = false;
    int copy_threads = 0;            // threads (caller's included) that stage host frames into pinned memory; 0 = min(8, cores / 4): measured best on a 256-thread host, 46 GB/s; more threads contend
    bool resize_bilinear = false;    // oversize frames: false = area average (the NPP build), true = cv::resize bilinear (the build without NPP)
    bool plan_cache = true;          // read / write <model_dir>/<stem>.<precision>.rfplan (packed weight image, weights.h)
    std::string plan_cache_path;     // explicit cache file instead (tests)
    std::vector<int> devices;        // more than one entry: one engine per device, batches sharded by image (multi.cpp)
    std::string model_stem = "mnet-deconv-0517";
};

struct ActInfo { void *ptr; int h, w, c; std::vector<float> scale; };      // scale: empty, or one per channel (int8)

struct OpInfo {
    std::string name;            // reference layer name(s) the launch covers
    std::string kernel;          // which kernel instance runs it, e.g. "dwpw<128,128,s1>" (joins profiles/*.json)
    double alg_elems_in = 0;     // per image: layer-wise input elements (SURVEY.md 8d "E")
    double alg_elems_out = 0;    // per image: layer-wise output elements
    double alg_u8_in = 0;        // per image: bytes read as u8 (the frame), not scaled by the element size
    double macs = 0;             // per image
    // per image: what the launch has to move through HBM at the very least GIVEN its fusion -- every tensor it reads from HBM once,
    // every tensor it writes once (weights: < 1 MB per launch, ignored).  `useful` HBM fraction = these bytes / time / peak.
    double hbm_elems_in = 0, hbm_elems_out = 0;
    std::function<void(hipStream_t, int)> launch;   // (stream, n_images)
};

// the constructor's `network` presets (RetinaFace.cpp:209-271): anchor ratios of a preset (empty = no anchors), and the base
// anchors of FPN level 0 / 1 / 2 (strides 32 / 16 / 8) for those ratios, 2 per ratio
bool network_preset(const std::string &network, std::vector<float> *ratios);
void preset_base_anchors(const std::vector<float> &ratios, int level, float out[][4]);

// host-only test hook: runs the host half of engine start-up (plan cache or model -> packed image); 1 = served from the cache
int plan_cache_probe(const std::string &model_dir, const EngineOptions &opt, size_t *arena_bytes);

// `scale` of RetinaFace.cpp:585-589 (rf_frame_scale): what network-input coordinates of a rows x cols frame are multiplied by to
// land in source-frame pixels; the alignment kernel applies the same float
inline float frame_scale(int rows, int cols, int net_h, int net_w) {
    const float sw = (float)cols / (float)net_w, sh = (float)rows / (float)net_h;
    const float sc = sw > sh ? sw : sh;
    return sc > 1.f ? sc : 1.f;
}

// Where the aligned crops of a call go (rf_align_batch_device / rf_detect_align_batch*): the crop of face k of image i is slot
// i * max_faces + k of d_crops (device) and / or crops (host), its forward matrix the 6 doubles at matrices + 6 * slot
struct AlignRequest {
    int crop = 112, max_faces = 0;
    uint8_t *d_crops = nullptr, *crops = nullptr;
    double *matrices = nullptr;
};

// Where the face batch of a call goes (rf_detect_face_batch* / rf_face_batch_device): packed face j is element block j of d_tensor
// (device) and / or tensor (host), its forward matrix the 6 doubles at matrices + 6 * j; offsets: n + 1 packed offsets (host)
struct FaceBatchRequest {
    FaceBatchSpec spec;
    uint8_t *d_tensor = nullptr, *tensor = nullptr;
    double *matrices = nullptr;
    int *offsets = nullptr;
    // the gated calls (face_quality.h): quality records of every considered face, only the faces whose flags are 0 are packed
    bool gated = false, has_gate = false;       // has_gate false: flags stay 0, every face is kept
    FaceGate gate;
    rf_face_quality *quality = nullptr;         // host, n * spec.max_faces records, or nullptr
};

// A tiled-detection call (tile.h; rf_detect_tiled_batch* / rf_tile_merge_device / rf_detect_tiled_face_batch_device): the validated
// spec, where the pass of each merged face goes, and the face batch that follows the merge on the device (nullptr = none)
struct TileRequest {
    TileSpec spec;
    int *src_tile = nullptr;                    // host, indexed like out, or nullptr
    const FaceBatchRequest *fb = nullptr;
};

// A flip-TTA call (tta.h; rf_detect_tta_batch* / rf_tta_merge_device): the validated spec and where the member count and the pass of
// each merged face go
struct TtaRequest {
    TtaSpec spec;
    int *votes = nullptr;                       // host, indexed like out, or nullptr
    int *src_pass = nullptr;
};

// A zoom-pyramid call (pyramid.h; rf_detect_pyramid_batch* / rf_pyramid_merge_device): the validated spec and where the member count
// and the pass of each merged face go
struct PyrRequest {
    PyrSpec spec;
    int *votes = nullptr;                       // host, indexed like out, or nullptr
    int *src_pass = nullptr;
};

// A rotation call (rot.h; rf_detect_rot_batch* / rf_rot_merge_device): the validated spec and where the member count and the rotation
// of each merged face go
struct RotRequest {
    RotSpec spec;
    int *votes = nullptr;                       // host, indexed like out, or nullptr
    int *src_rot = nullptr;
};

// A fisheye call (dewarp.h; rf_detect_dewarp_batch* / rf_dewarp_merge_device): the validated spec, the dewarper (what dewarper_create
// returned), where the member count and the view of each merged face go, and where the views go (device memory; nullptr: an
// engine-owned block)
struct DewarpRequest {
    DewarpSpec spec;
    void *dewarper = nullptr;
    int *votes = nullptr;                       // host, indexed like out, or nullptr
    int *src_view = nullptr;
    void *d_views = nullptr;                    // n * V * view_h * view_w * 3 bytes, dense, frame-major
};

// A region call (roi.h; rf_detect_roi_batch* / rf_roi_merge_device): the validated spec, the regions of the call's frames (frame-major,
// roi_counts[i] of frame i), where the member count and the region of each merged face go, and where the views go (device memory;
// nullptr: an engine-owned block)
struct RoiRequest {
    RoiSpec spec;
    const rf_roi *rois = nullptr;
    const int *roi_counts = nullptr;
    int *votes = nullptr;                       // host, indexed like out, or nullptr
    int *src_roi = nullptr;
    void *d_views = nullptr;                    // P * net_h * net_w * 3 bytes, dense, frame-major
};

// A tracked region call (roi.h; rf_detect_track_roi_batch* / rf_roi_track_cells_device): the validated spec, the margin the tracks'
// boxes are grown by (in 1/256ths; 0 = 64), where the member count and the slot of each merged face go, where the n * max_tracks cell
// records the device planned go (host, or nullptr) and where the views go (device memory; nullptr: an engine-owned block)
struct RoiTrackRequest {
    RoiSpec spec;
    int margin_q8 = 0;
    int *votes = nullptr;
    int *src_roi = nullptr;
    rf_roi_cell *cells = nullptr;
    void *d_views = nullptr;                    // P * net_h * net_w * 3 bytes, dense, frame-major; P: roi_passes(max_tracks, grid) per live tracked frame
};

// A change-region call (change.h; rf_change_regions_device / rf_detect_change_roi_batch*): the changer, the region spec and margin as
// for a tracked region call, the stream of each image, and where the results go -- cells: n * (T + R) records for the fused call
// (T: the tracker's max_tracks, 0 without one), n * R for the kernels alone; info: n records; each may be nullptr
struct ChangeRequest {
    void *changer = nullptr;
    RoiSpec spec;
    int margin_q8 = 0;
    const int *stream_of_image = nullptr;
    int *votes = nullptr;
    int *src_roi = nullptr;
    rf_roi_cell *cells = nullptr;
    rf_change_info *info = nullptr;
    void *d_views = nullptr;                    // P * net_h * net_w * 3 bytes, dense, frame-major; P: roi_passes(T + R, grid) per frame with pixels
};

// An enhanced detection call (enhance.h; rf_detect_enhanced_batch*): the validated spec, where the enhanced copies go (device memory;
// nullptr: an engine-owned block) and where the number of flagged tiles of each frame goes
struct EnhanceRequest {
    EnhanceSpec spec;
    void *const *d_enhanced = nullptr;
    const int *enhanced_steps = nullptr;        // nullptr: cols * 3
    int *tiles_enhanced = nullptr;              // host, n ints, or nullptr
};

// A tracked call (track.h; rf_track_update_device / rf_detect_track_*): the tracker (what tracker_create returned), the stream of every
// image (-1 = not tracked) and where tags, ended lists and their counts go (host; each may be nullptr)
struct TrackRequest {
    void *tracker = nullptr;
    const int *stream_of_image = nullptr;
    rf_track_tag *tags = nullptr;               // n * cap_per_image
    rf_track *ended = nullptr;                  // n * cap_ended
    int cap_ended = 0;
    int *ended_counts = nullptr;                // n
};

// The gallery half of a shot call (shot.h; rf_track_shots_device / rf_detect_track_shots_batch*): where the delivered shots (n * cap_ended
// faces of the gallery spec, device and / or host) and their records go; for the fused call the gate and the quality records
struct ShotRequest {
    uint8_t *d_shots = nullptr, *shots = nullptr;
    rf_shot *info = nullptr;
    bool gated = false, has_gate = false;       // gated: a gate or a quality buffer was given, the best shot goes by sharpness
    FaceGate gate;
    rf_face_quality *quality = nullptr;         // host, n * max_faces records (the gallery spec's max_faces), or nullptr
};

// A redacting call (redact.h; rf_redact_device / rf_detect_redact_batch* / rf_detect_track_redact_batch_device): the validated spec,
// the tracker whose coasting tracks are redacted too (nullptr = none) with the stream of every image, and where the per-region pixel
// counts (n * spec.max_regions) and the true region counts (n) go (host; each may be nullptr)
struct RedactRequest {
    RedactSpec spec;
    void *tracker = nullptr;
    const int *stream_of_image = nullptr;
    int32_t *pixels = nullptr;
    int *region_counts = nullptr;
    // An overlay call (overlay.h; rf_overlay_device / rf_detect_overlay_batch* / rf_detect_track_overlay_batch_device) is the same request
    // with `overlay` set: the same list of regions is drawn instead of redacted.  spec then carries the overlay's max_regions and coast
    // and is otherwise all defaults; ids (redact() only; host, as the faces; may be nullptr) are the faces' track ids.
    bool overlay = false;
    OverlaySpec ospec;
    const int64_t *ids = nullptr;
};

// What a fused call wants behind every detection launch, on the launch's stream and with no host synchronisation in between: the
// stages read faces and counts from the device-visible result block the launch has just written, and each frame's frame_scale is
// applied, so frames the engine shrank are sampled at full source resolution.  A null request: the stage is off.  The sets a call
// may carry are {align}, {face_batch}, {track}, {track, face_batch}, {track, shots}, {redact}, {track, redact} and {track, follow}.
//   align       the aligned crops of the faces found (AlignRequest).
//   face_batch  their face batch (face_batch.h): per launch a scan kernel packs the counts on the device and the tensor kernel
//               follows; gated, the quality kernel runs in front.  max_faces 0 in the spec has been replaced by the caller with
//               default_max_faces().  StageResult::overflow: more packed faces than the capacity.
//   track       the frame step of every image (track.h), which reads the call's quality records when face_batch is gated; the
//               track launches of a call wait for each other on the device.  StageResult::track_cut: a full table or a cut
//               ended list.
//   shots       with track, on a tracker that has a gallery: the gallery rules behind each track launch (shot.h).  The gate rides
//               in the request; gated, the quality launch of the gated face-batch path runs for the gallery spec.
//   redact      redaction (or, with `overlay`, drawing) of the faces found, in place in device-resident frames.  Host frames are
//               uploaded once, detected and redacted on that copy, and the copy goes to out_bgr[i] (rows of out_steps[i] bytes;
//               nullptr = dense).  With track (device frames only, the same tracker and streams in both requests) the launches
//               sit behind each track launch: the coasting regions are those of the table after this call's frame step.
//               StageResult::redact_cut: a region list was cut at max_regions.
struct StageCall {
    const AlignRequest *align = nullptr;
    const FaceBatchRequest *face_batch = nullptr;
    const TrackRequest *track = nullptr;
    const ShotRequest *shots = nullptr;
    const RedactRequest *redact = nullptr;
    bool follow = false;                        // with track alone, on a tracker that has follow: the keep launch behind each track launch (follow.h)
    uint8_t *const *out_bgr = nullptr;          // redact over host frames: where the redacted copies go
    const int *out_steps = nullptr;
};
struct StageResult { bool overflow = false, track_cut = false, redact_cut = false; };

class Engine {
public:
    // opt.devices.size() > 1 gives the image-sharding multi-device engine (multi.cpp), otherwise one single-device engine
    static std::unique_ptr<Engine> create(const std::string &model_dir, const std::string &network, float nms,
                                          const EngineOptions &opt);
    static std::unique_ptr<Engine> create_single(const std::string &model_dir, const std::string &network, float nms,
                                                 const EngineOptions &opt);
    virtual ~Engine() {}

    // frames on host / device; synchronous
    virtual void detect(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                        bool on_device, float threshold, rf_face *out, int cap_per_image, int *counts,
                        bool *truncated) = 0;
    // detect() + the stages of `stages` behind every detection launch (StageCall).  Single-device engines only.
    virtual void detect_staged(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *, bool *,
                               const StageCall &stages, StageResult *) {
        const char *what = stages.redact ? "face redaction is" : stages.track ? "face tracks are" : stages.face_batch ? "face batches are" : "face alignment is";
        throw Unsupported(std::string(what) + " not available on a multi-device handle");
    }
    // aligned crops of faces the caller supplies (faces[i * cap_per_image + k], k < counts[i]) from device-resident frames;
    // coord_scale: per image, nullptr = 1
    virtual void align(const void *const *, const int *, const int *, const int *, int, const rf_face *, int, const int *,
                       const float *, const AlignRequest &) {
        throw Unsupported("face alignment is not available on a multi-device handle");
    }
    // the face batch of faces the caller supplies, from device-resident frames
    virtual void face_batch(const void *const *, const int *, const int *, const int *, int, const rf_face *, int, const int *,
                            const float *, const FaceBatchRequest &, bool * /*overflow*/) {
        throw Unsupported("face batches are not available on a multi-device handle");
    }
    // Tiled detection: the frames are expanded into passes (ROI views + the shrunk full-frame pass) that go through detect()'s
    // ordinary launches; a gather launch behind each of them and one merge launch behind the last (ordered by events on the
    // device, no host wait) leave the merged faces in device memory, where rq.fb's face-batch launches read them.  *truncated: a
    // pass or the merge hit a cap; *overflow: rq.fb's capacity.  Single-device engines only.
    virtual void detect_tiled(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *,
                              bool *, const TileRequest &, bool * /*overflow*/) {
        throw Unsupported("tiled detection is not available on a multi-device handle");
    }
    // edge rule, mapping and merge of per-pass faces the caller supplies (faces[(first_pass[i] + t) * max_detections + k])
    virtual void tile_merge(const int *, const int *, int, const TileRequest &, const rf_face *, const int *, rf_face *, int, int *,
                            bool *) {
        throw Unsupported("tiled detection is not available on a multi-device handle");
    }
    // Flip test-time augmentation: every frame becomes two passes (itself and a mirrored copy made on the device in front of the
    // call's first launch) that go through detect()'s ordinary launches; a gather launch behind each of them and one voting merge
    // behind the last (ordered by events on the device, no host wait).  *truncated: a pass or the merge hit a cap.  Single-device
    // engines only.
    virtual void detect_tta(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *,
                            bool *, const TtaRequest &) {
        throw Unsupported("test-time augmentation is not available on a multi-device handle");
    }
    // mapping and merge of per-pass faces the caller supplies (faces[(i * passes + p) * max_detections + k])
    virtual void tta_merge(const int *, const int *, int, const TtaRequest &, const rf_face *, const int *, rf_face *, int, int *,
                           bool *) {
        throw Unsupported("test-time augmentation is not available on a multi-device handle");
    }
    // the mirror kernel on its own: a left-right mirrored copy of a device-resident frame
    virtual void mirror(const void *, int, int, int, void *, int) {
        throw Unsupported("test-time augmentation is not available on a multi-device handle");
    }
    // Rotation-robust detection: every frame becomes up to four passes (itself and copies turned by quarter turns, made on the device in
    // front of the call's first launch) that go through detect()'s ordinary launches; a gather launch behind each of them and one
    // voting merge behind the last (ordered by events on the device, no host wait).  *truncated: a pass or the merge hit a cap.
    // Single-device engines only.
    virtual void detect_rot(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *,
                            bool *, const RotRequest &) {
        throw Unsupported("rotation detection is not available on a multi-device handle");
    }
    // mapping and merge of per-pass faces the caller supplies (faces[(i * passes + p) * max_detections + j])
    virtual void rot_merge(const int *, const int *, int, const RotRequest &, const rf_face *, const int *, rf_face *, int, int *,
                           bool *) {
        throw Unsupported("rotation detection is not available on a multi-device handle");
    }
    // the rotate kernel on its own: a device-resident frame turned by k quarter turns counter-clockwise
    virtual void rotate(const void *, int, int, int, int, void *, int) {
        throw Unsupported("rotation detection is not available on a multi-device handle");
    }
    // Fisheye detection: a dewarper (the frame shape, the views' shape and meshes of one camera, uploaded once) lives on the handle;
    // every frame of a call becomes its V views, made by one kernel on the device in front of the call's first launch, which go through
    // detect()'s ordinary launches; a gather launch behind each of them and one voting merge behind the last (ordered by events on the
    // device, no host wait).  view_w / view_h 0: the net size.  *truncated: a pass or the merge hit a cap.  Single-device engines only.
    virtual void *dewarper_create(int /*rows*/, int /*cols*/, int /*view_w*/, int /*view_h*/, int /*views*/, const int32_t * /*mesh*/) {
        throw Unsupported("fisheye detection is not available on a multi-device handle");
    }
    virtual void dewarper_destroy(void *) {}
    // the dewarp kernel on its own: one view of a device-resident frame of the dewarper's shape
    virtual void dewarp(void *, int /*view*/, const void *, int, void *, int) {
        throw Unsupported("fisheye detection is not available on a multi-device handle");
    }
    // rows / cols (each may be null) of every frame must be the dewarper's, or 0 x 0 for an empty frame
    virtual void detect_dewarp(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *, bool *, const DewarpRequest &) {
        throw Unsupported("fisheye detection is not available on a multi-device handle");
    }
    // edge rule, mapping and merge of per-view faces the caller supplies (faces[(i * V + v) * max_detections + j])
    virtual void dewarp_merge(int, const DewarpRequest &, const rf_face *, const int *, rf_face *, int, int *, bool *) {
        throw Unsupported("fisheye detection is not available on a multi-device handle");
    }
    // Region detection: the regions of every frame are packed, grid x grid to a net-sized view, by one kernel on the device in front of
    // the call's first launch; the views go through detect()'s ordinary launches; a gather launch behind each of them and one voting
    // merge behind the last (ordered by events on the device, no host wait).  *truncated: a pass or the merge hit a cap.
    // Single-device engines only.
    virtual void detect_rois(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *, bool *, const RoiRequest &) {
        throw Unsupported("region detection is not available on a multi-device handle");
    }
    // face rule and merge of per-pass faces the caller supplies (faces[q * max_detections + j], q over the call's passes)
    virtual void roi_merge(const int *, const int *, int, const RoiRequest &, const rf_face *, const int *, rf_face *, int, int *, bool *) {
        throw Unsupported("region detection is not available on a multi-device handle");
    }
    // the atlas kernel on its own: all passes of n regions of a device-resident frame, pass p at d_dst + p * view_h * dst_step
    virtual void roi_atlas(const void *, int, int, int, const rf_roi *, int, const RoiSpec &, int, int, void *, int) {
        throw Unsupported("region detection is not available on a multi-device handle");
    }
    // Tracked region detection: the plan kernel alone (image i's max_tracks records at cells + i * max_tracks; stream -1: void records),
    // and the fused call -- regions planned on the device from the tracker's tables, the frame steps behind the merge
    virtual void roi_track_cells(const TrackRequest &, int, const RoiTrackRequest &, rf_roi_cell *) {
        throw Unsupported("region detection is not available on a multi-device handle");
    }
    virtual void detect_track_rois(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *, bool *,
                                   const RoiTrackRequest &, const TrackRequest &, bool *) {
        throw Unsupported("region detection is not available on a multi-device handle");
    }
    // Change regions (change.h): a changer of one frame shape and n_streams streams; its reset (stream -1: all, which also clears the
    // error state) and a host copy of a stream's reference, frame counter and last mask (each may be null; returns bw * bh); the two
    // kernels alone over frames in device memory (synchronous; they step the reference); and the fused call, whose TrackRequest has a
    // null tracker when no tracker takes part
    virtual void *changer_create(const ChangeSpec &, int /*rows*/, int /*cols*/, int /*n_streams*/) {
        throw Unsupported("change regions are not available on a multi-device handle");
    }
    virtual void changer_destroy(void *) {}
    virtual void changer_reset(void *, int /*stream*/) { throw Unsupported("change regions are not available on a multi-device handle"); }
    virtual int changer_read(void *, int /*stream*/, int32_t *, int64_t *, uint8_t *) {
        throw Unsupported("change regions are not available on a multi-device handle");
    }
    virtual void change_regions(const void *const *, const int *, const int *, const int *, int, const ChangeRequest &) {
        throw Unsupported("change regions are not available on a multi-device handle");
    }
    virtual void detect_change_rois(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *, bool *,
                                    const ChangeRequest &, const TrackRequest &, bool *) {
        throw Unsupported("change regions are not available on a multi-device handle");
    }
    // Low-light enhancement: the two enhance kernels over frames in device memory (synchronous), and the fused call -- the enhanced
    // copies made on the side stream in front of the call's first launch, detect() over them, no host wait in between.
    // Single-device engines only.
    virtual void enhance(const EnhanceSpec &, const void *const *, const int *, const int *, const int *, int, void *const *, const int *,
                         int *) {
        throw Unsupported("low-light enhancement is not available on a multi-device handle");
    }
    virtual void detect_enhanced(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *,
                                 bool *, const EnhanceRequest &) {
        throw Unsupported("low-light enhancement is not available on a multi-device handle");
    }
    // Zoom-pyramid detection: every frame becomes the passes of its pyramid plan -- 1x views, and tiles of the frame enlarged 2x / 4x
    // that a zoom kernel writes on the device in front of the call's first launch -- which go through detect()'s ordinary launches; a
    // gather launch behind each of them and one voting merge behind the last (ordered by events on the device, no host wait).
    // *truncated: a pass or the merge hit a cap.  Single-device engines only.
    virtual void detect_pyramid(const uint8_t *const *, const int *, const int *, const int *, int, bool, float, rf_face *, int, int *,
                                bool *, const PyrRequest &) {
        throw Unsupported("pyramid detection is not available on a multi-device handle");
    }
    // edge rule, mapping and merge of per-pass faces the caller supplies (faces[(first_pass[i] + p) * max_detections + k])
    virtual void pyramid_merge(const int *, const int *, int, const PyrRequest &, const rf_face *, const int *, rf_face *, int, int *,
                               bool *) {
        throw Unsupported("pyramid detection is not available on a multi-device handle");
    }
    // the zoom kernel on its own: a window of a device-resident frame enlarged 2x or 4x
    virtual void zoom(const void *, int, int, int, int, int, int, int, int, void *, int) {
        throw Unsupported("pyramid detection is not available on a multi-device handle");
    }
    // Face tracks: a tracker's state (n_streams tables) lives in device memory between calls; the track launch of a detection launch
    // follows it on its stream, the track launches of a call wait for each other on the device.  *cut: a full table or a cut ended
    // list.  Single-device engines only.
    virtual void *tracker_create(const TrackSpec &, int /*n_streams*/) { throw Unsupported("face tracks are not available on a multi-device handle"); }
    virtual void tracker_destroy(void *) {}
    virtual void tracker_reset(void *, int /*stream*/) { throw Unsupported("face tracks are not available on a multi-device handle"); }
    // host copy of a stream's table, frame counter and next id; flush: end its live tracks (returned instead of the table).  Returns
    // max_tracks, or the number of tracks ended.
    virtual int tracker_read(void *, int /*stream*/, rf_track *, int /*cap*/, int64_t *, int64_t *, bool /*flush*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // frame steps over faces the caller supplies (host memory)
    virtual void track_update(const TrackRequest &, int /*n*/, const rf_face *, int /*cap_per_image*/, const int * /*counts*/,
                              const float * /*coord_scale*/, const rf_face_quality *, int /*max_faces*/, bool * /*cut*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // hipEvent time of the track launch of the most recent track_update() (negative: none yet)
    virtual float track_last_launch_ms() const { return -1.f; }
    // Best-shot gallery (shot.h): a tracker may own n_streams x max_tracks face-batch crops and shot records in device memory; the two
    // shot launches follow each track launch on its stream and join the chain the track launches form.  Single-device engines only.
    virtual void tracker_enable_shots(void *, const FaceBatchSpec &) { throw Unsupported("face tracks are not available on a multi-device handle"); }
    // host copy of a stream's entries and records (zeros where the slot holds no shot); returns max_tracks
    virtual int tracker_read_shots(void *, int /*stream*/, uint8_t *, rf_shot *, int /*cap*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // tracker_read(flush) + the shots of the tracks it ends
    virtual int tracker_flush_shots(void *, int /*stream*/, rf_track *, int /*cap*/, int64_t *, int64_t *, uint8_t *, rf_shot *) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // Motion-predicted tracks (motion.h): a tracker may own n_streams x max_tracks motion records in device memory; every track launch
    // of such a tracker is the motion kernel's, and redaction coasts at the predicted boxes.  Single-device engines only.
    virtual void tracker_enable_motion(void *, const MotionSpec &) { throw Unsupported("face tracks are not available on a multi-device handle"); }
    // host copy of a stream's motion records; returns max_tracks
    virtual int tracker_read_motion(void *, int /*stream*/, rf_track_motion *, int /*cap*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // track_update() against device-resident frames + the gallery rules; max_faces is the gallery spec's
    virtual void track_shots(const TrackRequest &, const ShotRequest &, const void *const *, const int *, const int *, const int *, int /*n*/,
                             const rf_face *, int /*cap_per_image*/, const int * /*counts*/, const float * /*coord_scale*/,
                             const rf_face_quality *, bool * /*cut*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // hipEvent time of the two shot launches of the most recent track_shots() (negative: none yet)
    virtual float shot_last_launch_ms() const { return -1.f; }
    // Followed tracks (follow.h): a tracker may own n_streams x max_tracks follow records and templates in device memory.  A key step is
    // a track launch with the keep launch behind it on its stream (track_follow_update() over faces the caller supplies, or the fused
    // call with StageCall::follow); a follow step (track_follow()) is the search and step launches over frames alone: no detection.
    // Each stream appears at most once in such a call.  Single-device engines only.
    virtual void tracker_enable_follow(void *, const FollowSpec &) { throw Unsupported("face tracks are not available on a multi-device handle"); }
    // host copy of a stream's records and templates (zeros where the record is not valid); returns max_tracks
    virtual int tracker_read_follow(void *, int /*stream*/, rf_track_follow *, uint8_t *, int /*cap*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    virtual void track_follow_update(const TrackRequest &, const void *const *, const int *, const int *, const int *, int /*n*/, const rf_face *,
                                     int /*cap_per_image*/, const int * /*counts*/, const float * /*coord_scale*/, const rf_face_quality *,
                                     bool * /*cut*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // out / counts: the followed faces of every image (host); host frames are uploaded densely first
    virtual void track_follow(const TrackRequest &, const uint8_t *const *, const int *, const int *, const int *, int /*n*/, bool /*on_device*/,
                              rf_face *, int /*cap_per_image*/, int * /*counts*/, bool * /*cut*/) {
        throw Unsupported("face tracks are not available on a multi-device handle");
    }
    // hipEvent time of the search and step launches of the most recent track_follow() over device frames (negative: none yet)
    virtual float follow_last_launch_ms() const { return -1.f; }
    // Face redaction, in place in device-resident frames: regions of faces the caller supplies (host memory) and, with a tracker in
    // the request, of its streams' coasting tracks.  *cut: a region list was cut at max_regions.  Single-device engines only.
    virtual void redact(const void *const *, const int *, const int *, const int *, int, const rf_face *, int, const int *, const float *,
                        const RedactRequest &, bool * /*cut*/) {
        throw Unsupported("face redaction is not available on a multi-device handle");
    }
    // hipEvent time of the redaction launches of the most recent redact() (negative: none yet)
    virtual float redact_last_launch_ms() const { return -1.f; }
    // ... of the overlay launches of the most recent redact() with an overlay request
    virtual float overlay_last_launch_ms() const { return -1.f; }
    int default_max_faces() const { return opt_.max_detections; }
    // asynchronous: frames on host (staged through pinned memory before the call returns, unless the caller registered
    // them with host_register) or on the device
    virtual int enqueue(const void *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                        float threshold) = 0;
    virtual void wait(int ticket, rf_face *out, int cap_per_image, int *counts, bool *truncated) = 0;
    virtual int num_slots() const = 0;
    // pinned caller memory: register pins the range (hipHostRegisterPortable) and records it; adopt / forget only record /
    // drop a range another engine of the same handle pinned (multi-device handles pin once)
    virtual void host_register(const void *ptr, size_t bytes) = 0;
    virtual void host_unregister(const void *ptr) = 0;
    virtual void host_adopt(const void *ptr, size_t bytes) = 0;
    virtual void host_forget(const void *ptr) = 0;
    // drop what the engine remembers about where device frame pointers live (callers that free / re-home frame buffers)
    virtual void invalidate_residency() = 0;
    // device frames that arrived from another device since the handle was built, and the peer copies that carried them
    virtual void scatter_stats(long long *frames, long long *copies) const = 0;
    // super-batches launched since the handle was built and the images in them (added to what the arguments hold)
    virtual void launch_stats(long long *launches, long long *images) const = 0;

    virtual int last_anchor_indices(int image, int32_t *out, int cap) const = 0;
    virtual int last_candidate_counts(int *counts, int n) const = 0;
    virtual void last_timings(float *pre, float *infer, float *post, float *total) const = 0;
    virtual long get_output(const std::string &blob, int image, float *dst, size_t cap) = 0;
    virtual long debug_activation(const std::string &blob, int image, float *dst, size_t cap, int dims[3]) = 0;
    virtual int profile(const void *const *d_frames, int n, int iters, int cap, const char **names, const char **kernels,
                        float *avg_ms, double *alg_bytes, double *macs) = 0;
    // compulsory HBM bytes of every launch for n images (OpInfo::hbm_elems_*), in launch order; returns the number of launches
    virtual int compulsory_bytes(int n, int cap, double *bytes) = 0;

    int net_h() const { return net_h_; }
    int net_w() const { return net_w_; }
    int max_batch() const { return opt_.max_batch; }
    virtual int num_devices() const { return 1; }

protected:
    EngineOptions opt_;
    int net_h_ = 0, net_w_ = 0;
    float nms_threshold_ = 0.4f;
};

}  // namespace rf
