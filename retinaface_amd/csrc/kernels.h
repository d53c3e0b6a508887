// kernels.h -- launch API of the hand-written gfx950 kernels (kernels.hip).  Everything NHWC.
// T = rf::half_t (fp16 storage, fp32 accumulate, v_mfma_f32_16x16x32_f16) or float (fp32 storage,
// exact-f32 v_mfma_f32_16x16x4_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>

#include "align.h"
#include "enhance.h"
#include "face_batch.h"
#include "face_quality.h"
#include "overlay.h"
#include "redact.h"
#include "pyramid.h"
#include "rot.h"
#include "dewarp.h"
#include "roi.h"
#include "change.h"
#include "tile.h"
#include "tta.h"
#include "track.h"
#include "motion.h"
#include "shot.h"
#include "follow.h"

namespace rf {

typedef _Float16 half_t;

// a request the engine has no kernel instance / configuration for (C ABI: RF_ERR_UNSUPPORTED)
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };

// depthwise weights are stored in the activation type, except fp32 for int8 activations
template <typename T> struct DwWeightT { typedef T type; };
template <> struct DwWeightT<int8_t> { typedef float type; };

// The launch helpers keep per-device state (CU count, LDS attribute / occupancy of each kernel instance); the engine tells
// them which device the calling thread is bound to (engine.cpp DeviceGuard).
void bind_launch_device(int device);
// int8 engines: 0 when v_cvt_pk_u8_f32 on the bound device rounds to nearest even and saturates (what the requantising epilogues rely on),
// 1 when it does not (cached per device), -1 when the probe could not run (a runtime error: not cached)
int cvt_pk_u8_selfcheck();
// Test hooks (C ABI rf_debug_resident_cap / rf_debug_grid_log): cap the resident workgroups the persistent launches size their grids by
// (0 = off), and read back the (tiles, grid) pairs handed out since the cap was last set.  Process-wide, single-threaded use.
void debug_resident_cap(int workgroups);
int debug_grid_log(int cap, int *tiles, int *grid);
constexpr int kMaxDevices = 64;     // device ordinals a process may use (per-device launch state is sized by it; engine / multi.cpp enforce it)

// One input frame: CV_8UC3 BGR, row y at ptr + y*step (cv::Mat data/step; RetinaFace.cpp:594).
struct FrameDesc {
    const uint8_t *ptr;
    int rows, cols, step, pad_;
};

// Pre-NMS candidate written by the head kernel: the reference's FaceDetectInfo (RetinaFace.h:37-42) + the
// global anchor index that defines the NMS tie order.  64 bytes.
struct Candidate {
    float score;
    float x1, y1, x2, y2;
    float px[5], py[5];
    int32_t anchor;
};

// Per-launch scalars; they live in device memory (copied with the frame table) so a captured hipGraph stays valid.
struct RunParams {
    float threshold;       // keep iff conf > threshold   (RetinaFace.cpp:693)
    float nms_threshold;   // suppress iff IoU > nms      (RetinaFace.cpp:486)
    int32_t n_images;
    int32_t pad_;
};

// ---- K_a: preprocess (BGR u8 HWC -> RGB, top-left placement on a zero canvas; resizeconvertion.cu:46-63,
//      165-185, 279-316 with factor 1) fused with mobilenet0_conv0 (3x3 s2 p1 3->8) + BN + ReLU.
template <typename T>
void launch_conv0(hipStream_t s, const FrameDesc *frames, T *out, const float *w, const float *b, int n, int net_h,
                  int net_w);

// ---- K_a' (int8 engine): K_a fused with the first depthwise/pointwise block; conv0 on MFMA (hi+lo split weights), computed in fp16.
template <typename TO>
struct StemParams {
    const FrameDesc *frames; TO *out;              // out: [n][net_h/2][net_w/2][16], fp16 or int8
    const half_t *w0; const float *b0;             // conv0: 4 A fragments (hi/lo x k<32/k>=32), K = (ky,kx,BGRX) 36 -> 64
    const half_t *w0_raw = nullptr;                // ... for the raw-row staging (weights.h c0_raw_), nullptr = general path only
    const uint32_t *c0_tab = nullptr;              // conv0 pixel table of the raw path (measured slower; the engine passes nullptr = index arithmetic)
    const float *dw_w; const float *dw_b;          // depthwise taps [9][8], fp32
    const half_t *pw_w; const float *pw_b;         // pointwise 16 x 8 as one A fragment with K slots [hi | hi | lo | 0] (pack.h)
    const float *pw_m = nullptr;                   // int8 output: 1 / out_scale per channel (pw_b pre-divided)
    int n, net_h, net_w;
};
template <typename TO> void launch_stem(hipStream_t s, const StemParams<TO> &p);

// ---- K_a'' (fp16 engine): K_a' fused with the first stride-2 block (conv3 depthwise + conv4 pointwise): net / 4 map, 32 channels.
struct Stem2Params {
    const FrameDesc *frames; half_t *out;          // out: [n][net_h/4][net_w/4][32]
    const half_t *w0; const float *b0;
    const half_t *w0_raw = nullptr;                // conv0 fragments of the raw-row staging (weights.h c0_raw_): [2 parities][4][64][8]
    const float *dw0_w; const float *dw0_b; const half_t *pw0_w; const float *pw0_b;
    const uint32_t *dw1_mma; const float *dw1_b;   // conv3: taps as diagonal MFMA A fragments [5][64] dwords (pack.h), bias [16]
    const half_t *pw1_w; const float *pw1_b;       // conv4: 32 x 16 as hi | lo along K (k < 16: rn16(w), k >= 16: rn16(w - hi)), MFMA-fragment packed, bias [32]
    const uint32_t *c2_floor, *c3_floor;           // DC-centred conv2 / conv3 tiles: -mu per channel as packed fp16 pairs, [8] dwords each (the
                                                   // biases above are pre-adjusted on the host, weights.h)
    int n, net_h, net_w;
};
void launch_stem2(hipStream_t s, const Stem2Params &p);

// ---- K_b: depthwise 3x3 (+BN+ReLU) -> pointwise 1x1 (+BN+ReLU), the intermediate never leaves LDS.
//      has_dw = false gives a plain 1x1 conv (+bias, +ReLU): the FPN laterals.
template <typename T>
struct DwPwParams {
    const T *in; T *out;
    const typename DwWeightT<T>::type *dw_w;        // [9][cin] (fp32 when T = int8)
    const float *dw_b;    // [cin]
    const uint32_t *dw_mma = nullptr;   // fp16 engine: the depthwise taps as per-lane dwords of DIAGONAL MFMA A fragments,
                                        // [cin/16][5][64] (dw_mma_dword in pack.h): the stencil runs on the matrix cores
    const T *pw_w;        // MFMA-fragment packed (pack.h), k = cin
    const float *pw_b;    // [cout]
    const T *lat_w = nullptr; const float *lat_b = nullptr; T *lat_out = nullptr;   // optional fused FPN lateral (cout -> 64)
    const float *pw_m = nullptr, *lat_m = nullptr;   // int8: requantisation multipliers per output channel
    const float *dw_m = nullptr;                     // int8 depthwise on MFMA: per-channel scale of the 15-bit integer taps
    int n, hin, win, hout, wout;
    int cin, cout, stride;
    bool has_dw;
};
template <typename T> void launch_dwpw(hipStream_t s, const DwPwParams<T> &p);

// ---- K_b2 (fp16 engine): two backbone blocks, 32 -> 32 stride 1 then 32 -> 64 stride 2, in one launch; the map between them stays in LDS
struct DwPw2Params {
    const half_t *in; half_t *out;                 // in [n][hin][win][32], out [n][hin/2][win/2][64]
    const uint32_t *dwa_mma; const float *dwa_b; const half_t *pwa_w; const float *pwa_b;     // block A: diagonal dw fragments (pack.h), packed pw
    const uint32_t *dwb_mma; const float *dwb_b; const half_t *pwb_w; const float *pwb_b;     // block B
    int n, hin, win;
};
void launch_dwpw2(hipStream_t s, const DwPw2Params &p);

// ---- K_c: dense 3x3 p1 s1 conv as an implicit GEMM on MFMA (+bias +ReLU).  Optional fused input
//      "lateral + bilinear x2 upsample(coarser)" (Deconvolution k4 s2 p1 + Crop + Eltwise SUM,
//      prototxt :1553-1592) and an output split into two NHWC destinations (merged sibling convs).
template <typename T>
struct Conv3Params {
    const T *in; int in_ld, in_off;       // input pixel stride / channel offset (elements)
    const T *up;                          // nullptr, or coarser level [n][h/2][w/2][64]
    const T *w; const float *b;           // packed (k = 9*cin), bias[cout]
    const float *m = nullptr;             // int8: per-output-channel requantisation multiplier
    float a_lat = 1.f, a_up = 1.f;        // fused upsample+add: staged = lat * a_lat + up * a_up (int8 scale ratios)
    bool blend_fp32 = false;              // int8: blend in fp32 even where the packed-integer form applies (test knob RF_BLEND_FP32, read ONCE when the lane is built)
    T *out0; int ld0, off0, n0;           // output channels [0, n0)    -> out0[pixel*ld0 + off0 + c]
    T *out1; int ld1, off1;               // output channels [n0, cout) -> out1[pixel*ld1 + off1 + c - n0]
    int n, h, w_, cin, cout;
};
// `levels`: 1..3 parameter sets of the same (cin, cout) covered by ONE launch (the FPN levels of the SSH module)
template <typename T> void launch_conv3x3(hipStream_t s, const Conv3Params<T> *levels, int nlevels);

// ---- K_c2 (fp16 / int8 engines): the tail of the SSH context module -- conv_b (16 -> 32: context_conv2 || context_conv3_1) and conv_c
//      (16 -> 16: context_conv3_2 on context_conv3_1) -- in one launch; context_conv3_1 never leaves LDS; writes concat[32:64].
template <typename T>
struct SshTailParams {
    const T *in;                                   // context_conv1 output [n][h][w][16]
    const T *wb; const float *bb; const float *mb; // conv_b packed (k = 144), bias [32], int8 multipliers [32] or nullptr
    const T *wc; const float *bc; const float *mc; // conv_c packed, bias [16], multipliers [16] or nullptr
    T *cat;                                        // concat tensor [n][h][w][64]: channels 32..63 are written
    int n, h, w_;
};
template <typename T> void launch_ssh_tail(hipStream_t s, const SshTailParams<T> *levels, int nlevels);   // 1..3 FPN levels per launch

// ---- K_d: the three 1x1 heads of one stride as one 64->32 GEMM + 2-class softmax + anchor decode +
//      bbox / landmark regression + clip + threshold compaction (RetinaFace.cpp:666-724, 378-432, 179-199).
template <typename T>
struct HeadParams {
    const T *in;                          // [n][h][w][64] = rf_cX_det_concat_relu
    const T *w; const float *b;           // packed 16A x 64, bias[16A]: cls [0, 2A) (background A | foreground A), bbox [2A, 6A), landmark [6A, 16A)
    const float *m = nullptr;             // int8: per-channel dequantisation multiplier (w_scale * in_scale)
    int n, h, w_, stride, anchor_offset;  // anchor_offset = global index of (a=0, iy=0, ix=0) of this stride
    int num_anchors = 2;                  // A: anchors per cell, 2 ("net3") or 4 ("net3a"); 0 = a preset without anchors: no candidates
    float base[4][4];                     // the A base anchors of this stride (RetinaFace.cpp:34-103)
    int net_h, net_w;
    const RunParams *params;
    Candidate *cand; int *cand_count; int cap;
    float *dump_prob, *dump_bbox, *dump_lmk;   // optional NCHW fp32 copies of the 3 blobs (nullptr = off)
};
template <typename T> void launch_head(hipStream_t s, const HeadParams<T> *levels, int nlevels);   // 1..3 strides per launch

// ---- K_e: per-image sort (score desc, anchor index asc) + greedy NMS (RetinaFace.cpp:434-492); one
//      workgroup per image, everything in LDS.
struct NmsParams {
    const Candidate *cand; int *cand_count; int cap;         // cap: power of two <= 4096; counter is reset to 0 at the end
    const RunParams *params;
    Candidate *out; int *out_count; int *out_cand_count;     // out[img*max_det + k]; true kept / candidate counts
    int max_det;                                             // (out* may be pinned host memory: written over PCIe)
    int n;
};
void launch_nms(hipStream_t s, const NmsParams &p);

// Area-average downscale of an over-size frame onto the net-size u8 canvas (NPPI_INTER_SUPER stand-in,
// resizeconvertion.cu:298-311; closed-source NPP semantics -> "parity unpinned").
void launch_resize_area(hipStream_t s, const FrameDesc *src, uint8_t *dst, int n, int net_h, int net_w);
// The same step in the reference's build without NPP: cv::resize bilinear (RetinaFace.cpp:611-620), OpenCV's fixed-point algorithm.
void launch_resize_bilinear(hipStream_t s, const FrameDesc *src, uint8_t *dst, int n, int net_h, int net_w);

// ---- K_f: 5-point face alignment -- S x S x 3 u8 BGR crops of the source frames, warped onto the recognition template by the
//      similarity of align.h; one workgroup per (image, face slot, band of crop rows).  Every pointer is device-visible memory
//      (the fused call reads faces and counts straight from the pinned result block the NMS kernel wrote).
struct AlignParams {
    const FrameDesc *frames;              // [n] SOURCE frames (full resolution, before any shrink)
    const uint8_t *faces;                 // image i, face k: an rf_face at faces + (i * faces_per_image + k) * face_stride
    int face_stride, faces_per_image;     // bytes per record (rf_face 60, Candidate 64); records per image
    const int *counts;                    // [n] faces of each image (clamped to faces_per_image and max_faces here)
    const float *scale;                   // [n] coordinate scale per image (rf_frame_scale), nullptr = 1
    int n, max_faces, crop;               // crop slots per image; crop edge S (kAlignMinCrop..kAlignMaxCrop)
    int first_image;                      // slot of (image i, face k) = (first_image + i) * max_faces + k
    uint8_t *crops;                       // [slots][S][S][3], or nullptr
    double *mats;                         // [slots][6] forward matrices (source -> crop), or nullptr
};
void launch_align(hipStream_t s, const AlignParams &p);

// ---- K_g: face batches -- the aligned faces of a launch packed into one dense tensor in the recogniser's layout and number format
//      (face_batch.h; same transform and sampling as K_f).  launch_face_scan turns the per-image counts into packed offsets on
//      the device and advances the call's running base; launch_face_batch writes the tensor: one workgroup per (image, face,
//      band of crop rows), a workgroup whose packed face is at or beyond min(total, capacity) exits at once.
struct FaceScanParams {
    const FrameDesc *frames;              // [n]: an empty frame (ptr == nullptr) packs no faces
    const int *counts;                    // [n] faces of each image (clamped to faces_per_image and max_faces here)
    int n, faces_per_image, max_faces;
    int *running;                         // device int: packed faces of the call's earlier launches; advanced by this launch's total
    int first;                            // != 0: the call's first launch, the base is 0 whatever *running holds
    int *offsets;                         // [n + 1] out: packed index of each image's first face, offsets[n] = the next launch's base
};
void launch_face_scan(hipStream_t s, const FaceScanParams &p);

struct FaceBatchParams {
    const FrameDesc *frames;              // as AlignParams
    const uint8_t *faces;
    int face_stride, faces_per_image;
    const float *scale;
    const int *offsets;                   // [n + 1], what launch_face_scan wrote (not read when packed is set)
    int n, max_faces;
    FaceBatchSpec spec;                   // crop edge, format, channel order, mean / scale, capacity, antialias
    void *tensor;                         // [capacity] faces of 3 * S * S elements, aligned to the element size, or nullptr
    double *mats;                         // [capacity][6], or nullptr
    const int *packed = nullptr;          // gated: packed index of (image i, face k) at packed[i * max_faces + k], -1 = not packed
                                          // (what launch_face_gate_scan wrote); nullptr: offsets[i] + k
};
void launch_face_batch(hipStream_t s, const FaceBatchParams &p);
int face_batch_band_rows(int crop, int format);      // crop rows one workgroup covers (exposed for tests and DESIGN.md)

// ---- K_h: face quality (face_quality.h) -- one 64-byte record per considered face: integer sums over the luma of its crop (the
//      transform and sampling of K_f), landmark numbers, and the flags of the call's gate.  launch_face_gate_scan is the keep-mask
//      counterpart of launch_face_scan: it packs the faces whose flags are 0.
struct FaceQualityParams {
    const FrameDesc *frames;              // as AlignParams
    const uint8_t *faces;
    int face_stride, faces_per_image;
    const int *counts;                    // [n] faces of each image (clamped to faces_per_image and max_faces here)
    const float *scale;
    int n, max_faces, crop;
    int aa_max = 0;                       // 0: the plain crop; 1, 2, 4, 8: the antialiased crop with this largest factor (align_aa_factor)
    int has_gate;                         // 0: flags stay 0
    FaceGate gate;
    rf_face_quality *records;             // [n * max_faces] out: (image i, face k) at i * max_faces + k; considered faces only
};
void launch_face_quality(hipStream_t s, const FaceQualityParams &p);

struct FaceGateScanParams {
    const FrameDesc *frames;              // as FaceScanParams
    const int *counts;
    int n, faces_per_image, max_faces;
    const rf_face_quality *records;       // [n * max_faces], what launch_face_quality wrote
    int *running;                         // as FaceScanParams
    int first;
    int *offsets;                         // [n + 1] out: packed index of each image's first kept face
    int *packed;                          // [n * max_faces] out: packed index of every slot k < min(max_faces, faces_per_image), -1 = none
};
void launch_face_gate_scan(hipStream_t s, const FaceGateScanParams &p);
int face_quality_ring_rows(int crop);                // luma rows the quality kernel holds in LDS (exposed for tests and DESIGN.md)

// ---- K_i: the pass gather of tiled, TTA, pyramid, rotation and fisheye detection (tile.h, tta.h, pyramid.h, rot.h, dewarp.h) -- behind each detection
//      launch of such a call: one workgroup per pass (image of the launch) applies the mode's mapping (and, for tiles and the pyramid,
//      its edge rule) to the faces the NMS kernel kept and appends the survivors, as Candidate records whose `anchor` is the tie-break
//      index g = pass_id * rank_stride + k, to the candidate array of the pass's frame (an atomic counter per frame; the append order
//      does not matter: the merge sorts on a total order).  The merge is launch_nms (tiles) or launch_vote_merge on those arrays.
template <class Entry> struct PassGatherParams {
    const uint8_t *faces;                 // pass p, rank k: 15 floats at faces + (p * faces_per_pass + k) * face_stride
    int face_stride, faces_per_pass;      // bytes per record (rf_face 60, Candidate 64); records per pass
    const int *counts;                    // [n] faces of each pass (clamped to faces_per_pass here)
    const Entry *table;                   // [n] what each pass is (frame < 0: skipped)
    int n, edge, rank_stride;             // passes of this launch; the spec's edge (TTA and rotation ignore it; fisheye: view pixels); max_detections
    Candidate *cand; int *cand_count;     // per frame f: cand[f * cap + pos], pos from atomicAdd(cand_count + f); the counter keeps
    int cap;                              // counting past cap (the merge reports it), records at or beyond cap are not written
};
// What differs between the modes: keep() maps a face in place and says whether it survives, pass_id() is the entry's pass number.
struct TileMap {
    using Entry = TileEntry;
    __host__ __device__ static bool keep(const Entry &e, int edge, const float *in, float *out) { return tile_map_face(e, edge, in, out); }
    __host__ __device__ static int pass_id(const Entry &e) { return e.t; }
};
struct TtaMap {
    using Entry = TtaEntry;
    __host__ __device__ static bool keep(const Entry &e, int, const float *in, float *out) { tta_map_face(e, in, out); return true; }
    __host__ __device__ static int pass_id(const Entry &e) { return e.pass; }
};
struct PyrMap {
    using Entry = PyrEntry;
    __host__ __device__ static bool keep(const Entry &e, int edge, const float *in, float *out) { return pyr_map_face(e, edge, in, out); }
    __host__ __device__ static int pass_id(const Entry &e) { return e.p; }
};
struct RotMap {
    using Entry = RotEntry;
    __host__ __device__ static bool keep(const Entry &e, int, const float *in, float *out) { rot_map_face(e, in, out); return true; }
    __host__ __device__ static int pass_id(const Entry &e) { return e.k; }
};
struct DewarpMap {
    using Entry = DewarpEntry;
    __host__ __device__ static bool keep(const Entry &e, int edge, const float *in, float *out) { return dewarp_map_face(e, edge, in, out); }
    __host__ __device__ static int pass_id(const Entry &e) { return e.view; }
};
// region detection: the pass of a face does not name its region, so the rule reports it (keep_region in place of keep); pass_id is
// the first region of the pass, the id a face carries until its rule has named its own
struct RoiMap {
    using Entry = RoiEntry;
    __host__ __device__ static bool keep_region(const Entry &e, int, const float *in, float *out, int *region) { return roi_map_face(e, in, out, region); }
    __host__ __device__ static int pass_id(const Entry &e) { return e.pass * e.grid * e.grid; }
};
template <class Map> void launch_pass_gather(hipStream_t s, const PassGatherParams<typename Map::Entry> &p);      // the six above

// ---- K_j: face tracks (track.h) -- the frame steps of a launch's images: one workgroup per stream present in the launch walks that
//      stream's images in order, its table in LDS, one thread per slot.  Every pointer is device-visible memory (the fused calls read
//      faces and counts from the pinned result block the NMS kernel wrote, and the two tables below from pinned memory).
struct TrackStreamEntry { int32_t stream, first, n, pad_; };          // images[first .. first + n) are this stream's, in call order
struct TrackImageEntry {
    int32_t local;                        // index of the image among the launch's faces / counts
    int32_t image;                        // index of the image in the call (tags, ended lists, quality records)
    float scale;                          // coord_scale
    int32_t empty;                        // != 0: a frame without pixels, it has no faces whatever counts says
};
struct TrackArgs {                        // what track_kernel takes
    const TrackStreamEntry *streams; int n_streams;      // the grid
    const TrackImageEntry *images;
    const uint8_t *faces;                 // image i, face k: 15 floats at faces + (i * faces_per_image + k) * face_stride
    int face_stride, faces_per_image;
    const int *counts;                    // [launch images]
    const rf_face_quality *records;       // call image c, face k at records[c * max_faces + k], or nullptr: best shots by score
    int max_faces;                        // m = min(count, faces_per_image, max_faces, kTrackMaxFaces)
    TrackSpec spec;
    uint8_t *state;                       // stream s: TrackHeader + max_tracks rf_track at s * (16 + max_tracks * 176)
    rf_track_tag *tags; int tag_stride;   // call image c, face k < min(count, tag_stride) at tags[c * tag_stride + k]
    rf_track *ended; int cap_ended;       // call image c: ended[c * cap_ended + j]
    int *ended_counts;                    // [call images] the true number
    int *status;                          // [call images] kTrackOverflow or 0
};
// With a motion pointer (motion.h) launch_track runs track_motion_kernel, the same layout with each slot's velocity in registers;
// without one it runs track_kernel on the TrackArgs part alone.
struct TrackParams : TrackArgs {
    rf_track_motion *motion;              // stream s, slot t: motion[s * max_tracks + t], or nullptr: the plain frame step
    MotionSpec mspec;
};
void launch_track(hipStream_t s, const TrackParams &p);

// ---- K_l: best-shot gallery (shot.h) -- two launches behind launch_track on its stream, which read tags, ended lists, counts and the
//      table after the step from where the track kernel has just written them.  launch_shot_deliver: one workgroup per (delivered
//      shot, band of crop rows) copies the slot's stored entry, or samples the frame of this launch the shot was taken in, into the
//      call's shot block.  launch_shot_keep: one workgroup per (slot, band) whose final owner is a face of this launch samples that
//      face into the slot's entry.  Stream order between the two is what makes "deliver the old entry, then keep the new one" safe.
struct ShotParams {
    const TrackStreamEntry *streams; int n_streams;      // as TrackParams, the same tables
    const TrackImageEntry *images; int n_images;         // the tracked images of the launch: the sum of streams[].n
    const int32_t *entry_of;              // [n_images] index into streams of images[j]'s stream
    const FrameDesc *frames;              // [launch images] SOURCE frames, indexed by images[j].local
    const uint8_t *faces;                 // as TrackParams
    int face_stride, faces_per_image;
    const int *counts;
    int max_faces, max_tracks;
    const uint8_t *state;                 // the tables AFTER the launch's frame steps
    const rf_track_tag *tags; int tag_stride;
    const rf_track *ended; int cap_ended;
    const int *ended_counts;
    FaceBatchSpec spec;                   // the gallery's
    uint8_t *gallery; rf_shot *records;   // stream s, slot t: entry (s * max_tracks + t) of bytes_per_face, record likewise
    uint8_t *out; rf_shot *out_info;      // deliver: call image c, ended entry e at c * cap_ended + e; each may be nullptr
};
void launch_shot_deliver(hipStream_t s, const ShotParams &p);
void launch_shot_keep(hipStream_t s, const ShotParams &p);

// ---- K_m: followed tracks (follow.h).  In a follow call every stream has at most one image, so streams[z] has n == 1 and its image is
//      images[streams[z].first].  launch_follow_keep (a key step, behind launch_track on its stream): one workgroup per (stream of the
//      launch, slot) reads the table after the step; a free slot gets the zero record, a slot the step matched or opened (last_frame is
//      the step's frame: exactly the slots a tag of the image names) gets its template and record retaken.  launch_follow_search: one
//      workgroup of four waves per (stream, slot) writes one FollowResult to `results`; launch_follow_step: one workgroup per stream, one
//      thread per slot, applies them, ages and ends tracks and compacts the output and ended lists in slot order.
struct FollowParams {
    const TrackStreamEntry *streams; int n_streams;      // the grid; as TrackParams, the same tables
    const TrackImageEntry *images;
    const FrameDesc *frames;              // [launch images] SOURCE frames, indexed by images[j].local
    TrackSpec spec;
    FollowSpec fspec;
    uint8_t *state;                       // as TrackParams
    rf_track_follow *records;             // stream s, slot t: records[s * max_tracks + t]
    uint8_t *templates;                   // ... templates + (s * max_tracks + t) * 1024
    FollowResult *results;                // search -> step: stream entry z, slot t at results[z * max_tracks + t]
    rf_face *out; int cap_per_image;      // step: call image c, followed face j at out[c * cap_per_image + j]
    int *counts;                          // [call images] the true number of followed faces
    rf_track_tag *tags; int tag_stride;   // call image c: tags[c * tag_stride + j], j < min(count, tag_stride)
    rf_track *ended; int cap_ended;
    int *ended_counts;                    // [call images] the true number
    int *status;                          // [call images] kTrackOverflow (the output list was cut) or 0
};
void launch_follow_keep(hipStream_t s, const FollowParams &p);
void launch_follow_search(hipStream_t s, const FollowParams &p);
void launch_follow_step(hipStream_t s, const FollowParams &p);

// ---- K_k: face redaction (redact.h) -- in place in the frames of a launch, in three launches ordered on the stream.
//      launch_redact_regions: one workgroup per image turns its faces, and with a tracker its stream's coasting tracks, into region
//      records.  launch_redact_mean (PIXELATE without blur) reads the frames and writes every region's cell values; launch_redact_write reads
//      only those, the records and the spec and writes the pixels each region owns.  Every pointer is device-visible memory (the fused
//      calls read faces and counts from the pinned result block the NMS kernel wrote).
struct RedactArgs {                       // what the three kernels take
    const FrameDesc *frames;              // [n] SOURCE frames (full resolution); they are written
    const uint8_t *faces;                 // image i, face k: an rf_face at faces + (i * faces_per_image + k) * face_stride
    int face_stride, faces_per_image;
    const int *counts;                    // [n] faces of each image, clamped to count_cap here (the faces beyond it do not exist)
    int count_cap;
    const float *scale;                   // [n] coordinate scale per image, nullptr = 1
    int n, image0;                        // images of this launch; call index of its first image
    RedactSpec spec;
    const uint8_t *track_state;           // a tracker's state block (TrackParams::state), or nullptr
    int max_tracks, coast;                // its slots per stream; live tracks with 1 <= missed <= coast are redacted
    const int *streams;                   // [n] the stream of each image (-1: faces only), or nullptr
    RedactRegion *regions;                // call image c: regions[c * max_regions + r]
    int *nreg;                            // [call images] length of the list after the cut
    int *true_counts;                     // [call images] ... before the cut
    uint32_t *cell_values;                // region slot q = c * max_regions + r, cell (gx, gy): cell_values[(q * cells + gy) * cells + gx]
    int *pixels;                          // [call images * max_regions] pixels each region owns (zeroed by launch_redact_regions)
    uint8_t *shadow;                      // spec.blur only: call image c's blurred owned pixels, dense cols * 3 bytes per row, at
    const unsigned long long *shadow_off; //   shadow + shadow_off[c]; every byte has one writer (its pixel's owner)
};
// With a motion pointer launch_redact_regions runs the coasting-box variant of its kernel: a coasting track is redacted at its predicted
// box for h = min(missed, horizon) (motion.h) instead of where it was last seen.
struct RedactParams : RedactArgs {
    const rf_track_motion *motion;        // the tracker's motion records (TrackParams::motion), or nullptr
    int horizon;                          // MotionSpec::horizon
};
void launch_redact_regions(hipStream_t s, const RedactParams &p);
void launch_redact_mean(hipStream_t s, const RedactParams &p);
// spec.blur: takes the place of launch_redact_mean -- reads the frames and writes the blurred value of every owned pixel into the
// shadow; launch_redact_write then copies owned pixels from the shadow into the frame
void launch_redact_blur(hipStream_t s, const RedactParams &p);
void launch_redact_write(hipStream_t s, const RedactParams &p);

// ---- K_l: overlays (overlay.h) -- boxes, landmark discs and labels drawn in place into the frames of a launch, in two launches ordered
//      on the stream.  launch_overlay_regions: redaction's list (the same code: faces, then the stream's coasting tracks) as overlay
//      records; launch_overlay_draw paints them.  The RedactParams part means what it means there (spec.max_regions and coast are the
//      overlay's; regions, cell_values and shadow are unused).
struct OverlayParams : RedactParams {
    OverlaySpec ospec;
    OverlayRegion *oregions;              // call image c: oregions[c * max_regions + r]
    const uint8_t *ids;                   // launch image i, face k: an int64 at ids + (i * ids_per_image + k) * id_stride; nullptr = no ids
    int id_stride, ids_per_image;         // faces k >= ids_per_image have no id
    int ids_of_streams;                   // 1: the ids are the tags of a track launch, which an image of stream -1 does not have
};
void launch_overlay_regions(hipStream_t s, const OverlayParams &p);
void launch_overlay_draw(hipStream_t s, const OverlayParams &p);

// ---- K_j: flip test-time augmentation (tta.h).
//      mirror_rows: a dense left-right mirrored copy of a BGR frame (any source pitch and alignment), in front of a TTA call's launches.
//      The gather is launch_pass_gather<TtaMap>, g = pass * rank_stride + k.
//      vote_merge:  nms_kernel's sort and greedy walk over the gathered candidates of a frame, which also records the head that
//                   suppressed each candidate; a second sort groups the members by head and every kept head becomes the
//                   score-weighted mean of its members.  One workgroup per frame; re-arms the frame counters as launch_nms does.
struct MirrorParams {
    const uint8_t *src; int rows, cols, step;     // row y at src + y * step
    uint8_t *dst; int dst_step;                   // cols * 3 bytes per row are written
};
constexpr int kMirrorFramesPerLaunch = 16;       // frames of one launch: their descriptors travel as kernel arguments
void launch_mirror_rows(hipStream_t s, const MirrorParams *frames, int n);

struct VoteMergeParams {
    const Candidate *cand; int *cand_count; int cap;         // cap <= 4096; the counter is reset to 0 at the end
    const RunParams *params;                                 // nms_threshold
    Candidate *out; int *out_count; int *out_cand_count;     // out[img * max_det + k] (anchor: g of the head); true head / candidate counts
    int *votes;                                              // votes[img * max_det + k]: members of each returned head
    int max_det;
    int n;
};
void launch_vote_merge(hipStream_t s, const VoteMergeParams &p, bool vote);     // vote false: the heads keep their own coordinates

// ---- K_m: rotation-robust detection (rot.h).
//      rotate_frames: dense or pitched quarter-turn rotations (np.rot90(F, k)) of BGR frames (any source pitch and alignment), in
//                     front of a rotation call's launches.  k = 0 / 2: mirror_rows' 12-byte path; k = 1 / 3: an LDS-tiled transpose.
//      The gather is launch_pass_gather<RotMap>, g = k * rank_stride + j.
//      The merge is launch_vote_merge.
struct RotateParams {
    const uint8_t *src; int rows, cols, step;     // the SOURCE frame: row y at src + y * step
    int k;                                        // quarter turns counter-clockwise, 0..3
    uint8_t *dst; int dst_step;                   // rot_cols(k) * 3 bytes per row are written, rot_rows(k) rows
};
constexpr int kRotateFramesPerLaunch = 16;       // rotations of one launch: their descriptors travel as kernel arguments
void launch_rotate_frames(hipStream_t s, const RotateParams *frames, int n);

// ---- K_o: fisheye detection (dewarp.h).
//      dewarp_views: dewarped views of BGR frames (any source pitch and alignment) as dense or pitched frames, in front of a fisheye
//                    call's launches: the pixel rule of dewarp.h, a workgroup per 64 x 16 pixel tile of a view, its ten mesh nodes read
//                    once, four source taps per pixel gathered from global memory, rows stored 12 bytes per thread.
//      The gather is launch_pass_gather<DewarpMap> (dewarp_map_face: edge rule and mapping through the mesh), g = view * rank_stride + j.
//      The merge is launch_vote_merge.
struct DewarpParams {
    const uint8_t *src; int rows, cols, step;     // the SOURCE frame: row y at src + y * step
    const int32_t *mesh;                          // the VIEW's nodes, device memory
    int view_w, view_h;                           // multiples of 16
    uint8_t *dst; int dst_step;                   // view_w * 3 bytes per row are written, view_h rows
};
constexpr int kDewarpViewsPerLaunch = 16;        // views of one launch: their descriptors travel as kernel arguments
constexpr int kDewarpTileW = 64, kDewarpTileH = 16;
void launch_dewarp_views(hipStream_t s, const DewarpParams *views, int n);

// ---- K_p: region detection (roi.h).
//      roi_atlas:  the atlas views of a call (any source pitch and alignment) as dense or pitched frames, in front of a region call's
//                  launches: the pixel rule of roi.h, a workgroup per 64 x 16 pixel tile of ONE cell (the cell's record is uniform over
//                  the workgroup), a thread per four neighbouring pixels of a row, rows stored 12 bytes per thread.
//      The gather is launch_pass_gather<RoiMap> (roi_map_face: the face rule), g = region * rank_stride + j.
//      The merge is launch_vote_merge.
struct RoiAtlasParams {
    const uint8_t *src; int rows, cols, step;     // the SOURCE frame: row y at src + y * step
    const RoiCell *cells; int used;               // the view's first `used` cells, device memory; the others are zero
    int grid, view_w, view_h;                     // roi_check_view
    uint8_t *dst; int dst_step;                   // view_w * 3 bytes per row are written, view_h rows
    int min_level;                                // roi_min_level of the cells: 0, -1 or -2 (the launch sizes its LDS by it)
};
constexpr int kRoiViewsPerLaunch = 16;           // views of one launch: their descriptors travel as kernel arguments
constexpr int kRoiTileW = 64, kRoiTileH = 16;
void launch_roi_views(hipStream_t s, const RoiAtlasParams *views, int n);
//      roi_track_cells: the cell records of a tracked region call, planned from the tracker's tables (roi.h roi_track_cell): one thread
//                  per (image of the call, slot) writes image i's max_tracks records at cells + i * max_tracks; an image whose
//                  stream is < 0 (stream -1, or a frame without pixels: it has no passes) gets nothing written.  Views made from
//                  such records carry min_level = -2: the host cannot know their levels, so the launch is sized for x1/4.
struct RoiTrackCellsParams {
    const int32_t *streams; int n;                // [n] the stream whose table plans image i, or < 0; device-visible
    TrackSpec spec;
    const uint8_t *state;                         // as TrackArgs
    const rf_track_motion *motion;                // as TrackParams, or nullptr: a plain tracker
    MotionSpec mspec;
    int margin_q8, cw, ch, max_zoom;
    RoiCell *cells;                               // device memory, n * max_tracks records
    int stride;                                   // records between two images' blocks; 0: max_tracks (change regions follow the slots)
};
void launch_roi_track_cells(hipStream_t s, const RoiTrackCellsParams &p);

// ---- K_o: change regions (change.h), two launches ordered on the stream.
//      change_blocks:  one workgroup per (32 block columns of one block row, image): every byte of the frame is read once, 16 bytes per
//                      lane where a chunk lies inside the row and bytewise at a row's head and tail, summed with rotated-weight
//                      4-byte dot products into per-block LDS accumulators; then per block the step rule: the mask byte and the new
//                      reference value.
//      change_regions: one workgroup of 1024 threads per image: the mask dilated and labelled in LDS (label equivalence: link, then
//                      pointer jumping, until nothing changes), per-root counts, the selection, the boxes of the kept components, their cell records
//                      (image i's at cells + i * cell_stride + cell_first), the info record and the stream's frame counter.
//      An image whose stream is < 0 or whose src is null is not stepped: void records, zero info.
struct ChangeImage {
    const uint8_t *src; int32_t step, stream;     // row y at src + y * step
};
struct ChangeParams {
    const ChangeImage *images; int n;             // [n], device-visible
    ChangeSpec spec;
    int rows, cols, bw, bh;                       // the changer's shape and block grid
    int32_t *ref;                                 // per stream bw * bh values
    uint8_t *mask; int mask_pitch;                // per stream mask_pitch bytes, the first bw * bh used
    int64_t *frames;                              // per stream the frame counter; 0: the next step seeds
    int margin_q8, cw, ch, max_zoom;
    RoiCell *cells; int cell_stride, cell_first;  // device memory, 16-byte aligned
    rf_change_info *info;                         // [n], device memory
};
constexpr int kChangeSegBlocks = 32, kChangeThreads = 1024;
void launch_change_blocks(hipStream_t s, const ChangeParams &p);
void launch_change_regions(hipStream_t s, const ChangeParams &p);

// ---- K_k: zoom-pyramid detection (pyramid.h).
//      zoom_tile:  windows of frames enlarged 2x / 4x (integer bilinear, pyr_zoom_pixel) written as dense frames, in front of a
//                  pyramid call's launches; mirror_rows' store discipline.
//      The gather is launch_pass_gather<PyrMap> (pyr_map_face: edge rule and mapping), g = p * rank_stride + k.
//      The merge is launch_vote_merge.
struct ZoomParams {
    const uint8_t *src; int rows, cols, step;     // the source frame: row y at src + y * step
    int z, x0, y0, tw, th;                        // the window of the z rows x z cols frame
    uint8_t *dst; int dst_step;                   // tw * 3 bytes per row are written
};
constexpr int kZoomTilesPerLaunch = 16;          // tiles of one launch: their descriptors travel as kernel arguments
void launch_zoom_tiles(hipStream_t s, const ZoomParams *tiles, int n);

// ---- K_n: low-light enhancement (enhance.h), two launches ordered on the stream, up to sixteen frames each.
//      enhance_lut:   one workgroup per (tile, frame): the tile's luma histogram in per-wave LDS sub-histograms, p99, clip,
//                     redistribution, prefix scan -> 256 LUT bytes and a flag byte per tile; the frame's flag count by atomic add.
//      enhance_apply: one workgroup per block of at most 64 x 64 pixels inside one interpolation cell (the rectangle between four
//                     neighbouring tile centres): its four LUTs staged in LDS, mirror_rows' 12-byte load / store discipline.
//                     dst may be src exactly (same pointer and pitch).
struct EnhanceParams {
    const uint8_t *src; int rows, cols, step;     // the source frame: row y at src + y * step
    uint8_t *dst; int dst_step;                   // cols * 3 bytes per row are written
    uint8_t *luts;                                // [tiles_y * tiles_x][256], row-major tiles
    uint8_t *flags;                               // [tiles_y * tiles_x]
    int *count;                                   // the frame's flagged tiles; zero before enhance_lut runs
};
constexpr int kEnhanceFramesPerLaunch = 16;      // frames of one launch: their descriptors travel as kernel arguments
void launch_enhance_lut(hipStream_t s, const EnhanceSpec &sp, const EnhanceParams *frames, int n);
void launch_enhance_apply(hipStream_t s, const EnhanceSpec &sp, const EnhanceParams *frames, int n);

// LDS bytes / tile geometry chosen for a layer (exposed for tests and DESIGN.md tables)
struct TileInfo { int th, tw; size_t lds_bytes; int blocks_per_image; };
template <typename T> TileInfo dwpw_tile_info(int cin, int cout, int stride, bool has_dw, int hout, int wout);
template <typename T> TileInfo conv3x3_tile_info(int cin, int cout, int h, int w);

}  // namespace rf
