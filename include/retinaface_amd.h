/*
 * retinaface_amd.h -- C ABI of the MI355X-native RetinaFace detect() engine.
 *
 * The reference (clancylian/retinaface) has no C ABI and no plugin registry: its only public
 * surface for this path is the C++ class in retinaface/RetinaFace.h:63-78.  This header is the
 * boundary a binding for that class (or any FFI: ctypes / cgo / JNI) would sit on; every entry
 * point cites the reference interface it replaces.  include/RetinaFace.h re-creates the C++
 * class verbatim on top of it.  No torch / OpenCV / HIP types appear in any signature.
 *
 * Threading: one handle = one caller thread at a time (the reference is single-threaded and
 * not re-entrant either: shared staging buffers, RetinaFace.cpp:323-336).  The rule is enforced: a
 * call that enters while another thread's call on the same handle is in flight returns
 * RF_ERR_INVALID_ARG at once ("handle in use by another thread" from rf_last_error on the refused
 * thread) and leaves the call in flight undisturbed.  Different handles are independent.
 * Errors: every call returns RF_OK (0) or a negative rf_status; rf_last_error() gives text.
 * (The reference abort()s / exit(0)s / bare-throws instead: trtutility.h:9-16,
 * trtnetbase.cpp:201-204, RetinaFace.cpp:327-335.)
 */
#ifndef RETINAFACE_AMD_H
#define RETINAFACE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_ABI_VERSION 2

typedef enum rf_status {
    RF_OK = 0,
    RF_ERR_INVALID_ARG = -1,
    RF_ERR_IO = -2,             /* model file missing / unreadable */
    RF_ERR_MODEL = -3,          /* graph is not the mnet0.25 + FPN + SSH topology this engine implements */
    RF_ERR_HIP = -4,            /* a HIP runtime call failed (no GPU, OOM, launch failure) */
    RF_ERR_UNSUPPORTED = -5,    /* e.g. int8 requested without a calibration table */
    RF_ERR_TRUNCATED = -6       /* more candidates / detections than the configured caps; counts[] hold the true numbers */
} rf_status;

typedef enum rf_precision {
    RF_PRECISION_FP32 = 0,      /* fp32 storage, exact-f32 MFMA (parity reference path)            */
    RF_PRECISION_FP16 = 1,      /* fp16 storage, fp32 accumulate (reference: kHALF, trtnetbase.cpp:268-274) */
    RF_PRECISION_INT8 = 2       /* int8 storage + v_mfma_i32_16x16x64_i8 with the per-tensor activation scales of the
                                   TensorRT calibration table (trtnetbase.cpp:295-311), per-channel weight scales */
} rf_precision;

/* Result record: byte-identical to the reference's FaceDetectInfo (RetinaFace.h:15-42):
 * score, rect{x1,y1,x2,y2}, pts{x[5], y[5]} = 15 floats, coordinates in network-input pixels. */
typedef struct rf_face {
    float score;
    float x1, y1, x2, y2;
    float px[5];
    float py[5];
} rf_face;

/* Replaces the compile-time / hard-coded configuration of the reference:
 * precision (trtnetbase.cpp:268-274,295), net H x W (prototxt line 7 via trtnetbase.cpp:149-197),
 * maxBatchSize = 8 (trtretinafacenet.cpp:21), model stem (RetinaFace.cpp:276).
 * Zero-initialise, set struct_size = sizeof(rf_options), fill what you need; 0 = default. */
typedef struct rf_options {
    uint32_t struct_size;
    int32_t precision;          /* rf_precision; default RF_PRECISION_FP16 */
    int32_t net_h, net_w;       /* 0 = the prototxt / .rfw input dims; must be multiples of 32 */
    int32_t max_batch;          /* images per launch (default 8); larger batches are chunked */
    int32_t device;             /* HIP device ordinal + 1; 0 = the calling thread's current HIP device.  Calls may come from any
                                   thread: every entry point binds the engine's device for its duration and restores the caller's */
    int32_t max_candidates;     /* pre-NMS candidates kept per image (default 4096, power of two) */
    int32_t max_detections;     /* post-NMS faces returned per image (default 256) */
    int32_t use_graph;          /* 1 (default) = replay a captured hipGraph per batch size; 2 = off */
    int32_t keep_outputs;       /* 1 = also materialise the 9 NCHW fp32 head blobs for rf_get_output() */
    const char *model_stem;     /* default "mnet-deconv-0517" (RetinaFace.cpp:276) */
    int32_t lanes;              /* launches that may be in flight at once (default 3): each lane owns a stream, its
                                   activation buffers and its hipGraphs */
    int32_t coalesce;           /* rf_enqueue_batch_device() batches merged into ONE launch of up to max_batch*coalesce
                                   images (default: about 256 images of 448 x 448 worth of pixels per launch, clamped to [1, 256]; 1 = off).  A merged launch starts when it is full or when one of
                                   its tickets is waited for.  rf_num_slots() = lanes * coalesce. */
    /* ---- fields added in ABI 2 (a caller compiled against ABI 1 passes the shorter struct_size and gets the defaults) ---- */
    int32_t copy_threads;       /* host threads (the caller's included) that stage host frames into pinned memory; 0 = min(8, cores/4) */
    int32_t n_devices;          /* > 1: one engine per entry of devices[], every rf_detect_batch* call is sharded by image over them */
    const int32_t *devices;     /* HIP device ordinals (0-based; an ordinal may repeat); NULL / n_devices <= 1: `device` above */
    int32_t plan_cache;         /* 0 / 1 (default): keep the packed weight image next to the model as <stem>.<precision>.rfplan -- the
                                   analogue of the reference's serialized-engine cache (trtnetbase.cpp:205-243): later rf_create calls
                                   read it back (one file read + one hipMemcpy, no parse / BN fold / packing) as long as the model files'
                                   hash, the precision and the library build match; 2 = neither read nor write it */
    int32_t oversize_resize;    /* how a frame LARGER than the net is shrunk: 0 / 1 (default) = aspect-kept area average, the reference's
                                   NPP build (resizeconvertion.cu:298-311, NPPI_INTER_SUPER: closed source, semantics by definition);
                                   2 = cv::resize bilinear + one-sided zero padding, the reference's build without NPP
                                   (RetinaFace.cpp:585-620; OpenCV's published 8-bit fixed-point algorithm, bit-exact to the oracle's) */
} rf_options;

typedef struct rf_engine *rf_handle;

/* RetinaFace::RetinaFace(string &model, string network = "net3", float nms = 0.4)
 * (RetinaFace.h:66, RetinaFace.cpp:205-337).  model_dir holds either <stem>.rfw (this repo's packed
 * model, the analogue of the reference's serialized-engine cache, trtnetbase.cpp:205-243) or
 * <stem>.prototxt + <stem>.caffemodel (+ <stem>.table.int8).  `network` is the reference's preset name: "net3" (2 anchors per
 * cell, what the shipped models carry), "net3a" (ratios {1, 1.5}: 4 anchors per cell; needs a model whose heads have 8 / 16 / 40
 * channels, otherwise RF_ERR_MODEL -- the reference would read past its score blob), and the presets the reference constructs
 * without anchors ("ssh", "vgg", "net4" ... and unknown names): accepted, every detect call returns zero faces as there. */
int rf_create(const char *model_dir, const char *network, float nms_threshold,
              const rf_options *options, rf_handle *out_handle);

/* Host-only (no GPU): what the constructor's `network` preset means (RetinaFace.cpp:209-271).  Writes the base anchors
 * (x1, y1, x2, y2) of one stride (32, 16 or 8) in the reference's order -- ratios outer, scales inner -- and returns their count A:
 * 2 for "net3", 4 for "net3a", 0 for the presets the reference leaves without ratios / without an anchor configuration ("ssh",
 * "vgg", "net4", "net5", "net5a", "net6": they construct and then find no faces), RF_ERR_INVALID_ARG for a bad stride.
 * Names the reference does not know behave like "ssh" there (it prints "network setting error" and goes on): also 0. */
int rf_preset_anchors(const char *network, int stride, float *out4, int cap_boxes);

/* RetinaFace::~RetinaFace() (RetinaFace.cpp:339-345) -- unlike the reference this frees everything. */
void rf_destroy(rf_handle h);

/* Text of the last failure on this handle (h == NULL: last rf_create failure on this thread). */
const char *rf_last_error(rf_handle h);

/* TrtNetBase::getNetHeight/getNetWidth/getMaxBatchSize (trtnetbase.h) */
int rf_get_net_size(rf_handle h, int *net_h, int *net_w, int *max_batch);

/* void RetinaFace::detectBatchImages(vector<cv::Mat> imgs, float threshold = 0.5)
 * (RetinaFace.h:69, RetinaFace.cpp:749-940) and, with n == 1, RetinaFace::detect (RetinaFace.h:70,
 * RetinaFace.cpp:576-747).  Frames are HOST pointers to CV_8UC3 BGR pixels: bgr[i] + y*steps[i] is row y
 * (cv::Mat data/step).  Frames no larger than the net are placed top-left on a zero canvas
 * (resizeconvertion.cu:298-303 with the scale factor clamped to 1); larger frames are shrunk first
 * (options.oversize_resize: area average as in the NPP build, or bilinear as in the build without NPP).  Unlike the reference (which returns void and drops faceInfo, RetinaFace.cpp:726-747)
 * results are returned: out[i*cap_per_image + k], k < min(counts[i], cap_per_image), score-descending,
 * coordinates in network-input pixels (as in the reference).  A NULL/0x0 frame yields count 0
 * (img.empty() early return, RetinaFace.cpp:578-580).  n may exceed max_batch (the reference overruns its buffers there,
 * trtretinafacenet.cpp:21): the call is cut into chunks of max_batch images, and the chunks join launch sequences of up to
 * max_batch x options.coalesce images instead of being launched one by one. */
int rf_detect_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols,
                    const int *steps, int n, float threshold,
                    rf_face *out, int cap_per_image, int *counts);

/* The reference's Caffe-build detect (`void RetinaFace::detect(Mat img, ...)`, RetinaFace.cpp:943-1075): NO resize and no
 * fixed network size -- every frame is zero-padded right/bottom to the next multiple of 32 (:950-953), the net is reshaped
 * to that size (:965-966), anchors are regenerated for it (:1035) and boxes are clipped to the padded size (:1055).
 * Coordinates are therefore source-frame pixels.  The handle keeps one engine per distinct padded size it has seen (created
 * on first use, least-recently-used evicted beyond 8); frames of one call are grouped by size and results returned in call
 * order.  `on_device` != 0: the frame pointers are device pointers.  Size limit as in the reference: 4096 x 3072. */
int rf_detect_batch_pad32(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols,
                          const int *steps, int n, int on_device, float threshold,
                          rf_face *out, int cap_per_image, int *counts);

/* Factor by which the coordinates returned for a rows x cols frame must be multiplied to land in source-frame pixels:
 * max(cols / net_w, rows / net_h, 1) -- `scale` in RetinaFace.cpp:585-589; the reference's own mapping back is commented
 * out (:732-739), so results stay in network-input pixels and this is what a caller applies.  1.0 for frames that fit. */
float rf_frame_scale(rf_handle h, int rows, int cols);

/* Same, frames already resident in device memory (HBM) on the engine's device. */
int rf_detect_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols,
                           const int *steps, int n, float threshold,
                           rf_face *out, int cap_per_image, int *counts);

/* ---- Face alignment (no reference equivalent: the reference stops at detection; the step its users run next, an ArcFace-style
 * recogniser, takes crops warped onto a five-landmark template).  A crop is crop_size x crop_size x 3 u8 BGR, dense, row-major;
 * crop_size S is 16..512 (112 is the usual one).  DESIGN.md "Face alignment" holds the full definition; every result is
 * byte-exact against it (tests/align_ref.py restates it in numpy):
 *   template   x = {38.2946, 73.5318, 56.0252, 41.5493, 70.7299}, y = {51.6963, 51.5014, 71.7366, 92.3655, 92.2041} (left eye,
 *              right eye, nose, mouth left, mouth right: the order of rf_face.px / py), times S / 112;
 *   transform  the least-squares similarity without reflection from the landmarks times coord_scale onto the template, in IEEE
 *              double with + - * / in a fixed order and no fused multiply-add; a face whose landmarks do not span a plane
 *              (all equal, NaN, infinite) is INVALID: zero matrix, all-zero crop;
 *   sampling   crop pixel (u, v) is mapped back with the inverse similarity, the position rounded to 1/1024 pixel and the four
 *              neighbours blended in integers, (sum w * pix + 2^19) >> 20; taps outside the frame count as 0 (constant border);
 *              no half-pixel shift, no prefilter (cv::warpAffine-style bilinear).
 *
 * rf_align_matrix: host only, no GPU, no handle.  The forward matrix (source pixels -> crop pixels, row-major 2 x 3) of one face.
 * Returns 1 (valid), 0 (invalid face: fwd is all zero) or RF_ERR_INVALID_ARG (NULL argument, crop_size outside 16..512). */
int rf_align_matrix(const rf_face *face, float coord_scale, int crop_size, double fwd[6]);

/* Aligned crops of faces the CALLER supplies -- faces[i * cap_per_image + k], k < counts[i], e.g. the result of an earlier detect
 * call -- from frames resident on the engine's device.  coord_scale[i] multiplies image i's landmarks into source-frame pixels
 * (rf_frame_scale for results of rf_detect_batch*; NULL = 1 for all, which is also right for rf_detect_batch_pad32 results).
 * The crop of face k of image i is slot i * max_faces + k, for k < min(counts[i], max_faces); the other slots are unspecified.
 * d_crops (device memory on the engine's device) and crops (host memory) hold n * max_faces slots of 3 * S * S bytes, matrices
 * (host) n * max_faces * 6 doubles; each may be NULL.  max_faces is 1..4096.
 * Multi-device handles (options.n_devices > 1) return RF_ERR_UNSUPPORTED from this and the next two calls. */
int rf_align_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                          const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, int crop_size,
                          int max_faces, void *d_crops, uint8_t *crops, double *matrices);

/* rf_detect_batch_device + the aligned crops of what it finds, in one call: detection runs exactly as in rf_detect_batch_device
 * (out / counts / rf_last_anchor_indices are the same bytes), and the alignment launches follow each detection launch on its
 * stream with no host synchronisation in between -- they read the faces from the device-visible result block.  coord_scale is each
 * frame's rf_frame_scale, so a frame the engine shrank is sampled at its full source resolution.  n may exceed max_batch.
 * Slots, buffers and max_faces as above; faces beyond max_faces (score order) get no crop. */
int rf_detect_align_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, int crop_size, int max_faces,
                                 void *d_crops, uint8_t *crops, double *matrices);

/* The same with frames in HOST memory (rf_detect_batch's convention): they are uploaded once and both stages read that copy. */
int rf_detect_align_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, rf_face *out, int cap_per_image, int *counts, int crop_size, int max_faces,
                          void *d_crops, uint8_t *crops, double *matrices);

/* ---- Face batches: the aligned faces of one call as ONE dense tensor in a recogniser's layout and number format, written by the
 * engine directly (the u8 slot array of the calls above is never materialised).  DESIGN.md "Face batches" holds the definition;
 * every result is byte-exact against it (tests/face_batch_ref.py restates it in numpy):
 *   packed order  m_i = min(counts[i], max_faces); offsets[0] = 0, offsets[i+1] = offsets[i] + m_i; face k of image i is packed
 *                 face j = offsets[i] + k (images in call order, faces in score order); total = offsets[n].  The tensor holds the
 *                 packed faces j < min(total, capacity); nothing at or beyond that many faces is written.  total > capacity:
 *                 the call returns RF_ERR_TRUNCATED; detections, offsets (the true numbers) and the first `capacity` faces are valid.
 *                 (A detect call holds at most max_detections records per image: m_i is clamped to that as well.)
 *   value         q = the u8 value of crop pixel (u, v), source channel b of B, G, R, exactly as the crops above (0 everywhere
 *                 for an invalid face).  Output channel c takes source channel c (rgb == 0) or 2 - c (rgb == 1).
 *                 With spec.antialias == 1 (DESIGN.md "Antialiased face crops"; tests/face_aa_ref.py) q is supersampled instead:
 *                 with ia, ib the inverse similarity, R = ia * ia + ib * ib (source pixels per crop pixel, squared; IEEE double),
 *                 k = 1; while (k < aa_max && (double)(k * k) * 2.0 < R) k *= 2;  -- per face; rf_face_aa_factor returns it.
 *                 Sub-sample (i, j), i, j < k, sits at (u + (2i + 1 - k) / 2k, v + (2j + 1 - k) / 2k) and is sampled exactly as
 *                 the crop pixel above up to its unshifted sum a = sum w * pix (0 when out of range); with k = 2^m,
 *                 q = (sum over the k * k sub-samples of a + 2^(19 + 2m)) >> (20 + 2m).  k = 1 is the plain crop bit for bit.
 *                 RF_FACES_U8_HWC: q itself, layout [j][v][u][c]; mean / scale unused.
 *                 RF_FACES_F32_CHW: ((float)q - mean[c]) * scale[c], one fp32 subtract then one fp32 multiply, layout [j][c][v][u].
 *                 RF_FACES_F16_CHW: the same value converted to IEEE half, round to nearest even.
 *                 All three scale entries 0: mean 127.5 and scale 1/128 for every channel.
 *   matrices      packed the same way: matrices[j*6 .. j*6+5] holds the doubles rf_align_matrix gives for that face. */
typedef enum rf_face_format { RF_FACES_U8_HWC = 0, RF_FACES_F16_CHW = 1, RF_FACES_F32_CHW = 2 } rf_face_format;
typedef struct rf_face_batch_spec {
    uint32_t struct_size;   /* sizeof(rf_face_batch_spec), or 48: the struct up to and including capacity (antialias = 0) */
    int32_t crop_size;      /* 16..512, 0 = 112 */
    int32_t format;         /* rf_face_format */
    int32_t rgb;            /* 0 = frame order (BGR), 1 = RGB */
    float mean[3], scale[3];/* per OUTPUT channel */
    int32_t max_faces;      /* per image, 1..4096; 0 = the engine's max_detections */
    int32_t capacity;       /* packed faces the tensor holds, >= 1 */
    int32_t antialias;      /* 0 = off: the plain sampling and its bytes.  1 = supersampled sampling (value, above) */
    int32_t aa_max;         /* largest supersampling factor per axis: 1, 2, 4 or 8; 0 = 4.  Ignored (but still validated) when antialias == 0 */
} rf_face_batch_spec;

/* Host only, no GPU, no handle.  rf_face_batch_plan: what a call with these per-image counts packs -- fills offsets (n + 1 ints, may
 * be NULL) and bytes_per_face (may be NULL) and returns total (NOT clamped to capacity), or RF_ERR_INVALID_ARG for a bad
 * struct_size / crop_size / format / max_faces / capacity / antialias / aa_max, a non-finite mean or scale, or a negative count.
 * max_faces == 0 stands for the default max_detections (256) here.
 * rf_face_value_table: the 256 output values (q = 0..255) of output channel `channel` (0..2) in the spec's element type (u8, half
 * or float) -- the same code the kernel runs, compiled for the host. */
long rf_face_batch_plan(const rf_face_batch_spec *spec, const int *counts, int n, int *offsets, size_t *bytes_per_face);
int rf_face_value_table(const rf_face_batch_spec *spec, int channel, void *out256);

/* Host only, no GPU, no handle.  The supersampling factor k (1, 2, 4 or 8; 1 for an invalid face) a face gets under antialias == 1
 * with this aa_max -- the same code the kernel runs, compiled for the host.  crop_size 0 = 112, aa_max 0 = 4.  RF_ERR_INVALID_ARG for
 * a NULL face, a crop_size outside 16..512 or an aa_max other than 0, 1, 2, 4, 8. */
int rf_face_aa_factor(const rf_face *face, float coord_scale, int crop_size, int aa_max);

/* rf_detect_batch_device + the face batch of what it finds, in one call.  Detection runs exactly as in rf_detect_batch_device (out /
 * counts / rf_last_anchor_indices are the same bytes); the packing and the tensor launches follow each detection launch on its
 * stream with no host synchronisation in between, and each frame's rf_frame_scale is applied as in rf_detect_align_batch_device.
 * d_tensor: device memory on the engine's device, aligned to the element size, `capacity` faces; tensor: host memory of the same
 * size; matrices: host, capacity * 6 doubles; offsets: host, n + 1 ints.  Each may be NULL.  n may exceed max_batch.
 * A bad spec is refused before any state changes.  Multi-device handles return RF_ERR_UNSUPPORTED from these three calls. */
int rf_detect_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                void *d_tensor, void *tensor, double *matrices, int *offsets);

/* The same with frames in HOST memory (rf_detect_batch's convention). */
int rf_detect_face_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                         float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                         void *d_tensor, void *tensor, double *matrices, int *offsets);

/* The face batch of faces the CALLER supplies (the packed counterpart of rf_align_batch_device; faces, counts and coord_scale as
 * there).  RF_ERR_TRUNCATED when total > capacity. 
 * Work the caller has pending on the default stream when the call starts (a fill of d_out, say) is ordered in front of the call's writes
 * to d_out. */
int rf_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                         const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale,
                         const rf_face_batch_spec *spec, void *d_tensor, void *tensor, double *matrices, int *offsets);

/* ---- Face quality: a few exact numbers per aligned face, and face batches that pack only the faces that pass a gate on them, all on
 * the device (DESIGN.md "Face quality" holds the definition; tests/face_quality_ref.py restates it in numpy; nothing carries a tolerance).
 * For a face with crop size S (the crop is exactly the one of the calls above):
 *   luma          Y = (29 B + 150 G + 77 R + 128) >> 8 of the u8 BGR crop pixel;  sum_luma = the sum of Y over the S x S crop
 *   Laplacian     L = 4 Y(u,v) - Y(u-1,v) - Y(u+1,v) - Y(u,v-1) - Y(u,v+1) on 1 <= u, v <= S - 2; sum_lap, sum_lap2 = the sums of L, L^2
 *   sharpness     the variance of L: (double)(n sum_lap2 - sum_lap^2) / ((double)n (double)n), n = (S - 2)^2, the integers in int64
 *   covered       crop pixels sampled inside the frame (the in-range test of the crop holds and the top-left tap is a frame pixel)
 *   iod2          squared distance of the eyes in source pixels;  yaw: the nose's offset from the eyes' midpoint along the eye axis,
 *                 in eye distances (0 frontal, +-0.5 over an eye);  sin2_roll: sin^2 of the in-plane rotation
 * An invalid face (rf_align_matrix returns 0) has every number 0. */
typedef struct rf_face_quality {   /* 64 bytes */
    int32_t flags;                 /* 0 = kept; else OR of the RF_GATE_* that failed */
    int32_t covered;
    int64_t sum_luma, sum_lap, sum_lap2;
    double sharpness, iod2, yaw, sin2_roll;
} rf_face_quality;
enum { RF_GATE_INVALID = 1, RF_GATE_SHARPNESS = 2, RF_GATE_IOD = 4, RF_GATE_YAW = 8, RF_GATE_ROLL = 16, RF_GATE_COVERED = 32,
       RF_GATE_DARK = 64, RF_GATE_BRIGHT = 128 };
/* Every field: 0 = that gate is off.  Floats are widened to double before use; the comparisons are written so that NaN and infinity
 * fail; ALL failing bits are set.  With a gate, an invalid face always fails with RF_GATE_INVALID (and whatever its zeros fail). */
typedef struct rf_face_gate {
    uint32_t struct_size;          /* sizeof(rf_face_gate) */
    float min_sharpness;           /* fails if !(sharpness >= min) */
    float min_iod;                 /* source pixels; fails if !(iod2 >= (double)min * (double)min) */
    float max_abs_yaw;             /* fails if !(yaw >= -max && yaw <= max) */
    float max_sin2_roll;           /* fails if !(sin2_roll <= max) */
    float min_covered;             /* fraction of the crop; fails if !((double)covered >= (double)min * (double)(S * S)) */
    float min_luma, max_luma;      /* mean luma: (double)sum_luma against (double)x * (double)(S * S); RF_GATE_DARK / RF_GATE_BRIGHT */
} rf_face_gate;

/* Host only, no GPU, no handle -- the same code the kernel runs, compiled for the host.
 * rf_face_pose: zeroes *q, then fills iod2, yaw, sin2_roll, and flags = RF_GATE_INVALID for an invalid face.  crop_size 0 = 112.
 * rf_face_gate_eval: the flags the gate gives record q (q->flags & RF_GATE_INVALID marks an invalid face); a NULL gate gives 0.
 * RF_ERR_INVALID_ARG: a wrong struct_size, a negative or non-finite field, min_covered > 1, a crop_size outside 16..512. */
int rf_face_pose(const rf_face *face, float coord_scale, int crop_size, rf_face_quality *q);
int rf_face_gate_eval(const rf_face_gate *gate, const rf_face_quality *q, int crop_size);

/* The quality records of faces the CALLER supplies (arguments as rf_align_batch_device); no tensor is written.  quality: host,
 * n * max_faces records; face k < min(counts[i], max_faces) of image i is record i * max_faces + k, the other records are
 * unspecified.  gate may be NULL (flags 0).  A bad gate is refused before any state changes.
 * This call takes no spec: its records are always those of the PLAIN crop.  The records of the antialiased crop come from
 * rf_face_batch_gated_device with spec.antialias == 1 and d_tensor = tensor = NULL. */
int rf_face_quality_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                           const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, int crop_size,
                           int max_faces, const rf_face_gate *gate, rf_face_quality *quality);

/* The face-batch calls above behind a quality gate.  Face k of image i is CONSIDERED when k < m_i and KEPT when its flags are 0;
 * offsets[i+1] = offsets[i] + kept_i, the kept faces of an image stay in score order; tensor, matrices, total, capacity and
 * RF_ERR_TRUNCATED behave as above, counted over kept faces.  quality (host, n * max_faces records with the spec's max_faces, may
 * be NULL) receives the record of every considered face, kept or dropped, at i * max_faces + k.  A NULL gate keeps every face: the
 * tensor, matrices and offsets are the bytes of the ungated call.  Gating never changes out / counts / rf_last_anchor_indices.
 * With spec.antialias == 1 luma, sum_luma, sum_lap, sum_lap2 and sharpness are taken from the antialiased crop value; covered (still
 * the pixel centre's), iod2, yaw and sin2_roll are unchanged. */
int rf_face_batch_gated_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale,
                               const rf_face_batch_spec *spec, void *d_tensor, void *tensor, double *matrices, int *offsets,
                               const rf_face_gate *gate, rf_face_quality *quality);
int rf_detect_face_batch_gated_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                      void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                                      rf_face_quality *quality);
int rf_detect_face_batch_gated(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                               void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                               rf_face_quality *quality);

/* ---- Tiled detection: a frame LARGER than the net is cut into net-sized tiles that overlap, every tile is detected at 1:1, and the
 * faces of all tiles are moved into source-frame pixels and merged on the device (DESIGN.md "Tiled detection" holds the definition;
 * tests/tile_ref.py restates it in numpy; every result is byte-exact against it):
 *   plan     per axis, length L, net size N, overlap ov: L <= N: one tile (0, L); else n = ceil((L - ov) / (N - ov)) tiles of size N at
 *            o_i = floor(i * (L - N) / (n - 1)).  Tiles are row-major, t = ty * nx + tx, T = nx * ny; with full_frame on and a frame larger
 *            than the net in some dimension the whole frame, shrunk as rf_detect_batch_device shrinks it, is pass T.  A frame that fits
 *            the net has the plan "one tile, no extra pass".  More than 1024 passes: RF_ERR_INVALID_ARG.
 *   pass     the result of pass t is exactly what rf_detect_batch_device returns for the view {ptr + y0 * step + 3 * x0, th, tw, step}
 *            (the full-frame pass: for the whole frame) at the call's threshold: up to max_detections faces in score order, to
 *            the byte.  (As with rf_detect_batch_device itself, the last bits of a view's result depend on how it lies in memory --
 *            conv0 sums an aligned dense frame in another order than a view with a row pitch -- but not on what shares its launch:
 *            only a frame larger than the net is read from the resize canvas, a view that fits is read where it lies.)
 *   edge     in tile coordinates, fp32: face (x1, y1, x2, y2) of tile (x0, y0, tw, th) is dropped when  x0 > 0 && x1 < (float)edge,
 *            y0 > 0 && y1 < (float)edge,  x0 + tw < cols && x2 > (float)(tw - 1 - edge)  or  y0 + th < rows && y2 > (float)(th - 1 - edge):
 *            boxes that reach a tile side which is not a frame side.  The full-frame pass drops nothing.
 *   mapping  tile: one fp32 add of (float)x0 to every x coordinate (box and landmarks), of (float)y0 to every y coordinate;
 *            full-frame pass: one fp32 multiply of all 14 coordinates by rf_frame_scale(rows, cols).  Scores are unchanged.  Results are
 *            in SOURCE-FRAME pixels: their coord_scale for the alignment and face-batch calls is 1.
 *   merge    per frame, over the surviving faces of all passes: order by score descending (bit order), then g = t * max_detections + k
 *            ascending (k: the rank in the pass's result); greedy suppression exactly as the detector's NMS (+1-pixel areas, strict
 *            > nms_threshold of the handle).  counts[i] is the true number kept; out[i * cap_per_image + k] holds the first
 *            min(counts[i], cap_per_image, max_faces) in merge order; src_tile (may be NULL; same indexing) the pass each came from.
 *   caps     a pass whose own result was truncated contributes what it holds and the call returns RF_ERR_TRUNCATED; so does a frame
 *            with more than 4096 surviving candidates, whose faces are then unspecified (the other frames are valid); so does a
 *            merged list that max_faces or cap_per_image cut (counts[i] > min(max_faces, cap_per_image)), as rf_detect_batch reports
 *            a cut list: counts stay true and the faces returned are the first of the merge order.
 * A frame that fits the net gives the faces and counts of rf_detect_batch_device, byte for byte. */
typedef struct rf_tile_spec {
    uint32_t struct_size;   /* sizeof(rf_tile_spec) */
    int32_t overlap;        /* minimum overlap of neighbouring tiles in pixels, < min(net_h, net_w); 0 = min(net_h, net_w) / 4; negative = 0 px */
    int32_t edge;           /* width of the border band of the edge rule in pixels, < min(net_h, net_w) / 2; 0 = 8; negative = 0 */
    int32_t full_frame;     /* 0 / 1 = also run the whole frame shrunk as one more pass; 2 = off */
    int32_t max_faces;      /* merged faces kept per frame on the device, 1..4096; 0 = the engine's max_detections */
} rf_tile_spec;

/* Host only, no GPU, no handle -- the same code the kernel runs, compiled for the host.  spec may be NULL (all defaults; max_faces 0
 * stands for 256 here).
 * rf_tile_plan: the number of passes of a rows x cols frame at a net_h x net_w net, the full-frame pass included, or RF_ERR_INVALID_ARG
 * (bad spec, non-positive net size, negative or over-size frame, more than 1024 passes).  xywh (may be NULL) receives x0, y0, tw, th
 * of the first min(passes, cap_tiles) passes; the full-frame pass is reported as 0, 0, cols, rows.
 * rf_tile_map_face: edge rule and mapping of one face of pass t: 1 = kept, *out is the mapped face (out may equal in); 0 = dropped by the
 * edge rule; RF_ERR_INVALID_ARG as above or for t outside the plan. */
int rf_tile_plan(const rf_tile_spec *spec, int rows, int cols, int net_h, int net_w, int *xywh, int cap_tiles);
int rf_tile_map_face(const rf_tile_spec *spec, int rows, int cols, int net_h, int net_w, int t, const rf_face *in, rf_face *out);

/* Tiled detection of frames resident on the engine's device (frame limits as rf_detect_batch_device; a NULL / 0 x 0 frame yields count
 * 0).  The passes of all frames go through the engine's ordinary launches (chunked by max_batch, coalesced, spread over the lanes; the
 * shrunk full-frame passes share launches with the 1:1 tiles); a gather kernel behind each launch applies the edge rule and the
 * mapping, and one merge launch behind the call's last launch waits for them on the device -- no host synchronisation in between.
 * spec may be NULL.  A bad spec is refused before any state changes.  Multi-device handles return RF_ERR_UNSUPPORTED from this and
 * the next three calls.  rf_last_anchor_indices / rf_last_candidate_counts afterwards describe the call's PASSES, in plan order. */
int rf_detect_tiled_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, const rf_tile_spec *spec, rf_face *out, int cap_per_image, int *counts, int *src_tile);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, the tiles are views of that copy. */
int rf_detect_tiled_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, const rf_tile_spec *spec, rf_face *out, int cap_per_image, int *counts, int *src_tile);

/* Edge rule, mapping and merge of per-pass faces the CALLER supplies (host memory; the counterpart of rf_face_batch_device for this
 * stage): with first_pass[i] the running sum of the frames' plan sizes, pass t of frame i holds pass_counts[first_pass[i] + t] faces
 * (clamped to max_detections) at faces[(first_pass[i] + t) * max_detections + k].  No forward pass runs. */
int rf_tile_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_tile_spec *spec, const rf_face *faces,
                         const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *src_tile);

/* rf_detect_tiled_batch_device followed ON THE DEVICE by the face batch of the merged faces (rf_face_batch_gated_device's launches,
 * reading the merged faces and counts from device memory with coordinate scale 1): m_i = min(counts[i], fb_spec max_faces, tile_spec
 * max_faces).  tensor, matrices, offsets and quality are the bytes rf_face_batch_gated_device gives for the tiled call's out / counts
 * with coord_scale = NULL; gate = NULL and quality = NULL: those of rf_face_batch_device.  RF_ERR_TRUNCATED as in both calls. */
int rf_detect_tiled_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, const rf_tile_spec *tile_spec, rf_face *out, int cap_per_image, int *counts,
                                      int *src_tile, const rf_face_batch_spec *fb_spec, void *d_tensor, void *tensor, double *matrices,
                                      int *offsets, const rf_face_gate *gate, rf_face_quality *quality);

/* ---- Face tracks: stable ids and best shots across calls, kept in device memory (DESIGN.md "Face tracks" holds the definition;
 * tests/track_ref.py restates it in numpy; every result is byte-exact against it).  A tracker holds, per stream, a table of max_tracks
 * slots, a frame counter f (from 0) and a next id (from 1; ids never repeat until the stream is reset).  One FRAME STEP of a stream takes
 * the faces d_0 .. d_(m-1) of one image in score order, m = min(count, max_detections, max_faces, 256); faces at or beyond m get the tag
 * {0, -1, 0, 0, RF_TRACK_UNTRACKED}:
 *   map      all 14 coordinates times coord_scale (one fp32 multiply, also for a scale of 1); f = the counter, which then grows by one
 *   match    for k = 0 .. m-1 in order, over the live tracks no earlier face of this frame has claimed: the overlap of d_k's box with the
 *            track's `last` box, exactly the detector's NMS expression (w = min(x2) - max(x1) + 1, h likewise, 0 when w <= 0 || h <= 0,
 *            else inter / (area1 + area2 - inter) with +1-pixel areas; fp32, never contracted).  Eligible: iou >= min_iou (NaN fails).
 *            The face takes the eligible track with the largest overlap, ties to the lowest slot; that track gets last = d_k,
 *            last_frame = f, hits += 1, missed = 0
 *   best     of a matched or new track: with quality records the face is eligible when its record's flags == 0 and its value is the
 *            record's sharpness; without, every face is eligible with value (double)score.  It replaces the best shot when
 *            best_frame < 0 || value > best_value (strict: the earlier shot wins a tie); its tag then carries RF_TRACK_BEST
 *   age      live tracks nobody claimed: missed += 1; a track with missed > max_missed ENDS: its record goes to the image's ended list
 *            (ascending slot order) and its slot is freed (the whole record becomes zero; id 0 = free)
 *   open     the unmatched faces with score >= new_score, in score order, each take the lowest free slot (slots freed by `age` in this
 *            frame included): id = next_id++, hits = 1, missed = 0, first_frame = last_frame = f, best_frame = -1 and then `best`.
 *            A face below new_score is tagged RF_TRACK_UNTRACKED; with no free slot RF_TRACK_UNTRACKED | RF_TRACK_OVERFLOW and the
 *            call returns RF_ERR_TRUNCATED (everything else stays valid)
 *   tag      of a tracked face: the track's id and slot, its hits after this frame, age = (int32)min(f - first_frame + 1, INT32_MAX),
 *            flags = RF_TRACK_NEW | RF_TRACK_CONFIRMED (hits >= min_hits) | RF_TRACK_BEST as they apply.  rf_track.flags holds
 *            RF_TRACK_CONFIRMED once it applies, nothing else. */
typedef struct rf_track_spec {
    uint32_t struct_size;   /* sizeof(rf_track_spec) */
    int32_t max_tracks;     /* slots per stream, 1..256; 0 = 64 */
    float min_iou;          /* association threshold, finite and in (0, 1]; 0 = 0.3 */
    int32_t max_missed;     /* a track ends in the frame where missed > max_missed; 0 = 10; negative = 0 */
    int32_t min_hits;       /* matched frames before RF_TRACK_CONFIRMED is set; 0 = 3; negative = 1 */
    float new_score;        /* an unmatched face opens a track only if score >= new_score; finite and >= 0; 0 = every face */
} rf_track_spec;
typedef struct rf_track {   /* 176 bytes, no padding */
    int64_t id;             /* 0 = free slot */
    int64_t first_frame, last_frame, best_frame;    /* best_frame -1: no best shot yet */
    double best_value;
    int32_t hits, missed, flags, reserved;
    rf_face last, best;     /* in source-frame pixels (mapped) */
} rf_track;
typedef struct rf_track_tag { int64_t id; int32_t slot, hits, age, flags; } rf_track_tag;   /* 24 bytes */
enum { RF_TRACK_NEW = 1, RF_TRACK_CONFIRMED = 2, RF_TRACK_BEST = 4, RF_TRACK_UNTRACKED = 8, RF_TRACK_OVERFLOW = 16 };

/* Host only, no GPU, no handle -- the same code the kernel runs, compiled for the host.  One frame step on a caller-held table of
 * max_tracks records (all zero = empty) with its frame counter and next id (0 and 1 to start).  faces: count records in score order;
 * quality: NULL or one record per face k < min(count, max_faces); max_faces >= 1.  tags: count records.  ended (may be NULL with
 * cap_ended 0): the first min(*ended_count, cap_ended) ended tracks; *ended_count: the true number.  Returns 0, RF_ERR_TRUNCATED (a
 * full table or a cut ended list) or RF_ERR_INVALID_ARG (bad spec, NULL argument, negative count), which changes nothing. */
int rf_track_step(const rf_track_spec *spec, rf_track *table, int64_t *frames, int64_t *next_id, const rf_face *faces, int count,
                  float coord_scale, const rf_face_quality *quality, int max_faces, rf_track_tag *tags, rf_track *ended, int cap_ended,
                  int *ended_count);

/* A tracker lives on a handle; its state (n_streams tables) stays in device memory between calls.  n_streams is 1..1024.  A bad spec or
 * argument is refused before any state changes.  Multi-device handles return RF_ERR_UNSUPPORTED.  rf_destroy frees the trackers that are
 * left.  A tracked call that ends in an error (RF_ERR_TRUNCATED is not one) leaves the tracker's state unspecified: every later tracked
 * call returns RF_ERR_INVALID_ARG until rf_tracker_reset(tracker, -1). */
typedef struct rf_tracker_s *rf_tracker;
int rf_tracker_create(rf_handle h, const rf_track_spec *spec, int n_streams, rf_tracker *out_tracker);
void rf_tracker_destroy(rf_tracker tracker);
/* forget a stream's tracks, frame counter and ids (stream -1: all streams) */
int rf_tracker_reset(rf_tracker tracker, int stream);
/* Host copy of a stream's table (the first min(cap, max_tracks) slots; table may be NULL), frame counter and next id (may be NULL).
 * Returns max_tracks. */
int rf_tracker_read(rf_tracker tracker, int stream, rf_track *table, int cap, int64_t *frames, int64_t *next_id);
/* Ends every live track of the stream: they are returned slot-ascending (the first min(count, cap)) and their slots freed; the frame
 * counter and the next id stay.  Returns the number of tracks ended. */
int rf_tracker_flush(rf_tracker tracker, int stream, rf_track *ended, int cap, int64_t *frames, int64_t *next_id);

/* Frame steps over faces the CALLER supplies in host memory (faces[i * cap_per_image + k], k < counts[i]; the counterpart of
 * rf_tile_merge_device for this stage: no forward pass runs, no frames are needed).  stream_of_image[i] is 0 .. n_streams-1, or -1: that
 * image is not tracked (all-zero tags, empty ended list, no frame step).  Images of one stream are stepped in call order; streams are
 * independent.  coord_scale: per image, NULL = 1.  quality: NULL, or n * max_faces records (image i, face k at i * max_faces + k).
 * tags: n * cap_per_image records, tags[i * cap_per_image + k]; records at or beyond counts[i] are zero.  ended: n * cap_ended records,
 * image i's at ended + i * cap_ended (the first min(ended_counts[i], cap_ended)); a cut list returns RF_ERR_TRUNCATED. */
int rf_track_update_device(rf_handle h, rf_tracker tracker, const int *stream_of_image, int n, const rf_face *faces, int cap_per_image,
                           const int *counts, const float *coord_scale, const rf_face_quality *quality, int max_faces,
                           rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);

/* Measurement hook: the time of the track launch of the handle's most recent rf_track_update_device call, between two HIP events on its
 * stream (the upload and the copy-out are outside).  RF_ERR_INVALID_ARG before the first such call. */
int rf_track_last_launch_ms(rf_handle h, float *ms);

/* rf_detect_batch_device / rf_detect_batch + the frame step of every image, in one call: detection runs exactly as there (out / counts /
 * rf_last_anchor_indices are the same bytes); one track launch follows each detection launch on its stream and reads the faces from the
 * device-visible result block, the track launches of a call wait for each other on the device (a stream's images may sit in several
 * launches) -- no host synchronisation in between.  coord_scale is each frame's rf_frame_scale, so tracks live in source pixels; the
 * best shot goes by score.  A NULL / 0 x 0 frame is a frame with no faces: it ages its stream's tracks.  n may exceed max_batch.
 * There is no tracked form of the asynchronous tickets, of rf_detect_batch_pad32, of the tiled calls or of the alignment slot-array
 * calls: a tiled caller follows rf_detect_tiled_batch* with rf_track_update_device. */
int rf_detect_track_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                 const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);
int rf_detect_track_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                          const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);

/* rf_detect_face_batch_gated_device + the frame steps: tensor, matrices, offsets and quality are that call's bytes.  With a gate or a
 * quality buffer the track launch reads the call's quality records from device memory and the best shot goes by sharpness among the
 * faces whose flags are 0; otherwise by score.  max_faces is the spec's. */
int rf_detect_track_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                      void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                                      rf_face_quality *quality, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                                      rf_track *ended, int cap_ended, int *ended_counts);

/* ---- Best-shot gallery: every track slot keeps the pixels of its best shot in device memory, and a track hands them over when it ends
 * (DESIGN.md "Best-shot gallery" holds the definition; tests/shot_ref.py restates it in numpy; every result is byte-exact against it).
 * A tracker may own a gallery: n_streams x max_tracks entries of bytes_per_face (one face's tensor of rf_face_batch_device for the
 * gallery spec) and one rf_shot record per slot.  The frame step is rf_track_step's, tags / ended lists / counts / table are the bytes of
 * the plain tracked call, and two rules are added:
 *   keep     a face whose tag carries RF_TRACK_BEST sets its track's slot: the entry becomes exactly the bytes rf_face_batch_device
 *            writes for that face of that image (its own coordinates and coord_scale, not the mapped rf_track.best) with the gallery
 *            spec, the record becomes {id, f, matrix}
 *   deliver  every ended track that makes it into the image's ended list (the first min(ended_counts[i], cap_ended)) gets its shot at
 *            shots + (i * cap_ended + e) * bytes_per_face and its record at shot_info[i * cap_ended + e], the index of its rf_track in
 *            `ended`.  A track with best_frame < 0 (every face it had was gated) gets an all-zero shot and record.  Tracks cut from the
 *            list deliver nothing; shots and records beyond the delivered ones are not written.
 * Order within a frame is the tracker's: age (which ends tracks), then open -- a track that ends and one that opens in the same slot in
 * the same frame are both well defined: the ended track delivers the old entry, the slot then holds the new track's crop.  The entry of
 * a free slot, and of a live track with best_frame < 0, is unspecified in device memory; rf_tracker_read_shots / rf_tracker_flush_shots
 * return zeros for them. */
#define RF_SHOT_MAX_BYTES (1u << 30)
typedef struct rf_shot {    /* 64 bytes, no padding */
    int64_t id;             /* the track's id; 0 = no shot, the whole record is zero */
    int64_t frame;          /* the track's best_frame */
    double matrix[6];       /* rf_align_matrix of that face: the bytes the face-batch call writes to `matrices` */
} rf_shot;

/* Host only, no GPU, no handle -- the decisions of the two shot kernels, from the same code, for ONE stream's n images of one launch in
 * call order.  tags: n * cap_per_image (what the frame steps wrote), counts: n; ended / ended_counts: n * cap_ended / n; first_frame:
 * the stream's frame index of image 0; records: max_tracks shot records, before the launch on entry, after it on return (faces /
 * coord_scale / crop_size feed the matrix: faces n * cap_per_image or NULL = zero matrices, coord_scale n or NULL = 1).
 * source (may be NULL): 3 ints per ended-list entry (i * cap_ended + e): kind RF_SHOT_NONE (zero shot) / RF_SHOT_STORED (a = slot, b = 0)
 * / RF_SHOT_LAUNCH (a = image, b = face of this launch); entries beyond the delivered ones are {-1, -1, -1}.  owner (may be NULL):
 * 2 ints per slot, the (image, face) of this launch whose crop the slot holds afterwards, or {-1, -1}: the launch leaves it alone.  The
 * record of a delivered track is zeroed (its slot is free).  Returns the number of delivered shots, or RF_ERR_INVALID_ARG. */
enum { RF_SHOT_NONE = 0, RF_SHOT_STORED = 1, RF_SHOT_LAUNCH = 2 };
int rf_shot_resolve(int max_tracks, int n, const rf_track_tag *tags, int cap_per_image, const int *counts, const rf_track *ended,
                    int cap_ended, const int *ended_counts, int64_t first_frame, const rf_face *faces, const float *coord_scale,
                    int crop_size, rf_shot *records, int32_t *source, int32_t *owner);

/* Fixes the tracker's gallery for its lifetime: crop_size, format, rgb, mean, scale, antialias, aa_max and max_faces mean what they mean
 * in rf_face_batch_device; capacity is validated as there (>= 1) and otherwise unused.  RF_ERR_INVALID_ARG, before any state changes,
 * for a bad spec, a gallery above RF_SHOT_MAX_BYTES, a tracker that has stepped a frame (any stream's frame counter non-zero) or one
 * that has a gallery already.  Every tracked call without "shots" in its name then refuses the tracker (RF_ERR_INVALID_ARG, nothing
 * changes), so a gallery never goes stale; rf_tracker_read / rf_tracker_flush / rf_tracker_reset keep working (reset also zeroes the
 * stream's shot records). */
int rf_tracker_enable_shots(rf_tracker tracker, const rf_face_batch_spec *spec);
/* Host copy of the first min(cap, max_tracks) slots of a stream: entries (bytes_per_face each; may be NULL) and records (may be NULL).
 * A slot that is free, whose track has best_frame < 0 or whose record is not its track's reads as zeros.  Returns max_tracks. */
int rf_tracker_read_shots(rf_tracker tracker, int stream, void *shots, rf_shot *shot_info, int cap);
/* rf_tracker_flush + the shots of the tracks it ends, in the same order (the first min(count, cap); shots / shot_info may be NULL). */
int rf_tracker_flush_shots(rf_tracker tracker, int stream, rf_track *ended, int cap, int64_t *frames, int64_t *next_id, void *shots,
                           rf_shot *shot_info);

/* rf_track_update_device against frames resident on the device (those of rf_face_batch_device: any pointer and row step, NULL / 0 x 0 =
 * a frame with no faces), plus the gallery rules.  max_faces is the gallery spec's; quality: NULL (best by score) or n * max_faces
 * records.  d_shots (device) and shots (host) are n * cap_ended faces each, shot_info n * cap_ended records; each may be NULL.  A shots
 * block above RF_SHOT_MAX_BYTES is refused.  The tracker must have a gallery.  Dirty-tracker rules as above. */
int rf_track_shots_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                          int n, const int *stream_of_image, const rf_face *faces, int cap_per_image, const int *counts,
                          const float *coord_scale, const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended, int cap_ended,
                          int *ended_counts, void *d_shots, void *shots, rf_shot *shot_info);
/* Measurement hook: the time of the two shot launches of the handle's most recent rf_track_shots_device call, between two HIP events. */
int rf_shot_last_launch_ms(rf_handle h, float *ms);

/* rf_detect_batch_device / rf_detect_batch + the frame steps + the gallery rules in one call; detection runs exactly as there.  With a
 * gate or a quality buffer the quality launch of the gated face-batch path runs for the gallery spec with no tensor (the records are
 * the bytes of rf_face_quality_device for that spec) and the best shot goes by sharpness among the faces whose flags are 0; otherwise
 * by score.  The shot launches follow each track launch on its stream and join the chain the track launches form; frames larger than
 * the net are sampled at full resolution with rf_frame_scale.  The call produces no per-frame tensor.  There is no shot form of the
 * asynchronous tickets, of pad32, of the tiled, TTA and pyramid calls or of redaction, and none on multi-device handles. */
int rf_detect_track_shots_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                       float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                       const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                       const rf_face_gate *gate, rf_face_quality *quality, void *d_shots, void *shots, rf_shot *shot_info);
int rf_detect_track_shots_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                                float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                const rf_face_gate *gate, rf_face_quality *quality, void *d_shots, void *shots, rf_shot *shot_info);

/* ---- Face redaction: pixelate, blur or fill the faces of a frame IN PLACE, on the device (DESIGN.md "Face redaction" holds the definition;
 * tests/redact_ref.py restates it in numpy; every result is byte-exact against it).  Frames are CV_8UC3 BGR with any pointer and row step.
 *   region   of a face with box x1, y1, x2, y2 in a rows x cols frame, coord_scale s (fp32, one rounding per operation, never contracted):
 *            b = box * s (also for s = 1); w = bx2 - bx1, h = by2 - by1.  INVALID (owns no pixel) unless bx1, by1, bx2, by2, w, h are all
 *            finite and w >= 0, h >= 0.  ex1 = bx1 - margin * w, ex2 = bx2 + margin * w, ey likewise; each clamped to [-4096, 8192];
 *            ux0 = floor(ex1), ux1 = floor(ex2) + 1, uy likewise; W = ux1 - ux0, H = uy1 - uy0.  The clipped rectangle is its
 *            intersection with [0, cols) x [0, rows), which may be empty.
 *   mask     RECT: the clipped rectangle.  ELLIPSE: its pixels with a*a*H*H + b*b*W*W <= W*W*H*H, a = 2x + 1 - (ux0 + ux1),
 *            b = 2y + 1 - (uy0 + uy1), in int64: the ellipse inscribed in the UNCLIPPED rectangle, at pixel centres, exact.
 *   cells    c = (max(W, H) + cells - 1) / cells; pixel (x, y) lies in cell ((x - ux0) / c, (y - uy0) / c).  A cell's pixel set is its
 *            c x c square cut by the unclipped rectangle and the frame (not by the mask, not by ownership); its value per channel is
 *            (sum + n / 2) / n over that set, of the ORIGINAL bytes.  With c == 1 pixelation is the identity.
 *   list     of image i: its faces k < min(counts[i], max_regions) in score order; with a tracker, then the `last` boxes (scale 1) of
 *            its stream's live tracks with 1 <= missed <= coast in ascending slot order (with a motion tracker, rf_tracker_enable_motion,
 *            their predicted boxes instead); cut at max_regions.  A pixel is OWNED by the
 *            lowest-indexed region whose mask covers it.  The output equals the input except at owned pixels, which take their owner's
 *            cell value (PIXELATE) or fill (FILL).  Every read is of the original frame.
 *   blur     rf_redact_spec.blur = 1, 2 or 3 (PIXELATE only): an owned pixel takes the frame BLURRED instead of its cell's mean
 *            (DESIGN.md "Blur redaction"; tests/redact_blur_ref.py).  The radius of a region is rho = min(c, 64).  One 1-D pass of
 *            radius rho along an axis of length L maps u8 to u8 per channel: out[i] = (sum over d in [-rho, rho] of
 *            in[clamp(i + d, 0, L - 1)] + rho) / (2 rho + 1), integer division: the rounded mean with the border replicated.  The
 *            blurred frame is `blur` such passes along x on every row, then `blur` passes along y on every column (1: a box, 2: a
 *            triangle, 3: close to a Gaussian of sigma rho), every intermediate u8, of the ORIGINAL frame (of a view: the view --
 *            no byte outside cols * 3 of each row is read).  Region, mask, list, ownership and results are those above.  The blur
 *            is selected by this byte and not by a third `mode` because mode = 2 has always been refused and callers rely on that;
 *            blur > 3, or blur != 0 with RF_REDACT_FILL, is RF_ERR_INVALID_ARG like any bad spec.  blur = 0: exactly the above.
 *   results  pixels[i * max_regions + r] (may be NULL): the pixels region r owns; region_counts[i] (may be NULL): the length of the list
 *            before the cut (counts[i] + coasting tracks); a cut list returns RF_ERR_TRUNCATED. */
enum { RF_REDACT_PIXELATE = 0, RF_REDACT_FILL = 1 };
enum { RF_REDACT_RECT = 0, RF_REDACT_ELLIPSE = 1 };
typedef struct rf_redact_spec {   /* 32 bytes; a field of 0 means its default, a NULL spec all defaults */
    uint32_t struct_size;   /* sizeof(rf_redact_spec) */
    int32_t mode;           /* RF_REDACT_PIXELATE / RF_REDACT_FILL */
    int32_t shape;          /* RF_REDACT_RECT / RF_REDACT_ELLIPSE */
    int32_t cells;          /* cells across the longer side of a region, 1..64; 0 = 8 */
    float margin;           /* the box grows by this fraction of its width / height on each side; finite and <= 1; 0 = 0.2; negative = 0 */
    uint8_t fill[3];        /* B, G, R of RF_REDACT_FILL */
    uint8_t blur;           /* 0 = cell means; 1..3 (RF_REDACT_PIXELATE only) = box-blur passes per axis, radius min(c, 64) per region */
    int32_t max_regions;    /* regions per image, 1..1024; 0 = the engine's max_detections clamped to 1024 (256 without a handle) */
    int32_t coast;          /* with a tracker: also redact live tracks with 1 <= missed <= coast; 0 = the tracker's max_missed; negative = none */
} rf_redact_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.  rf_redact_region: out = ux0, uy0, ux1, uy1, the
 * clipped rectangle cx0, cy0, cx1, cy1 (cx1 <= cx0 or cy1 <= cy0: empty) and c; returns 1 (valid), 0 (invalid region: out is all zero)
 * or RF_ERR_INVALID_ARG (bad spec -- a bad spec->blur included --, NULL argument, rows or cols < 0).  With spec->blur set the region is
 * the same; its blur radius is min(c, 64). */
int rf_redact_region(const rf_redact_spec *spec, const rf_face *face, float coord_scale, int rows, int cols, int out[9]);
/* Redacts a whole frame in place in HOST memory (the CPU counterpart of rf_redact_device for one image without a tracker; a usable
 * fallback; spec->blur as on the device, same bytes).  pixels: min(count, max_regions) counts, may be NULL.  Returns 0, RF_ERR_TRUNCATED (count > max_regions: the first
 * max_regions faces were redacted) or RF_ERR_INVALID_ARG, which changes nothing. */
int rf_redact_host(const rf_redact_spec *spec, uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, int count,
                   float coord_scale, int32_t *pixels);

/* Redacts faces the CALLER supplies (host memory: faces[i * cap_per_image + k], k < counts[i] <= cap_per_image) in place in
 * device-resident frames (pixelated, blurred with spec->blur, or filled); no forward pass runs.  coord_scale: per image, NULL = 1 -- a tiled caller follows rf_detect_tiled_batch_device
 * with this call and coord_scale NULL (the tiled calls, the asynchronous tickets and rf_detect_batch_pad32 have no redacting form).
 * tracker may be NULL; with one, stream_of_image[i] names the stream whose coasting tracks (the tracker's CURRENT table) are redacted in
 * image i, -1 = faces only; a stream may appear at most once per call.  A NULL / 0 x 0 frame is skipped (no regions).  Refused before
 * any state changes: a bad spec, a NULL frame array, two frames of the call whose byte ranges overlap (RF_ERR_INVALID_ARG), a frame
 * resident on another GPU (RF_ERR_UNSUPPORTED: its staged copy would be redacted, not the frame), a multi-device handle
 * (RF_ERR_UNSUPPORTED). */
int rf_redact_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
                     int cap_per_image, const int *counts, const float *coord_scale, const rf_redact_spec *spec, rf_tracker tracker,
                     const int *stream_of_image, int32_t *pixels, int *region_counts);

/* Measurement hook: the time of the redaction launches of the handle's most recent rf_redact_device call, between two HIP events on its
 * stream (the upload and the copy-out are outside).  RF_ERR_INVALID_ARG before the first such call. */
int rf_redact_last_launch_ms(rf_handle h, float *ms);

/* rf_detect_batch_device + redaction of what it finds, in one call: detection runs exactly as there (out / counts /
 * rf_last_anchor_indices are the same bytes); the redaction launches follow each detection launch on its stream and read the faces from
 * the device-visible result block -- no host synchronisation in between.  coord_scale is each frame's rf_frame_scale, so an oversize
 * frame is redacted at its full source resolution.  n may exceed max_batch.  pixels: n * max_regions, may be NULL.  Refusals as above.
 * spec->blur selects the blur here and in the two calls below as in rf_redact_device. */
int rf_detect_redact_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                  float threshold, rf_face *out, int cap_per_image, int *counts, const rf_redact_spec *spec,
                                  int32_t *pixels);
/* Frames in host memory: uploaded once, detected and redacted on that copy; the redacted frames go to out_bgr[i] with rows of
 * out_steps[i] bytes (NULL = cols * 3), which may be the input buffers. */
int rf_detect_redact_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                           float threshold, rf_face *out, int cap_per_image, int *counts, const rf_redact_spec *spec,
                           uint8_t *const *out_bgr, const int *out_steps, int32_t *pixels);
/* rf_detect_track_batch_device + redaction: the redaction launches sit behind each track launch, so the coasting regions are those of
 * the table AFTER this call's frame step -- a face the detector misses in this frame stays covered where it was last seen.  Each stream
 * may appear at most once per call (RF_ERR_INVALID_ARG otherwise).  Tags, ended lists and the tracker's state are the bytes of the
 * unredacted tracked call. */
int rf_detect_track_redact_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                        float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                        const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                        const rf_redact_spec *spec, int32_t *pixels, int *region_counts);

/* ---- Overlays: draw the boxes, landmarks and labels of faces and tracks into frames IN PLACE, on the device -- what the reference's
 * detect() ends with (cv::rectangle(src, rect, Scalar(0,0,255), 2) and cv::circle(src, pt, 1, Scalar(0,255,0), 2) per face,
 * RetinaFace.cpp:1083-1091).  DESIGN.md "Overlays" holds the definition; tests/overlay_ref.py restates it in numpy; every result is
 * byte-exact against it.  Frames are CV_8UC3 BGR with any pointer and row step.  Integer-exact apart from the fp32 scaling (one
 * rounding per operation, never contracted).  With t = thickness, r = radius, f = font_scale, a = alpha:
 *   region   of a face with box x1, y1, x2, y2 at coord_scale s: b = box * s (also for s = 1); w = bx2 - bx1, h = by2 - by1.  INVALID (paints
 *            nothing) unless bx1, by1, bx2, by2, w, h are all finite and w >= 0, h >= 0.  Each coordinate is clamped to [-4096, 8192];
 *            x0 = floor(bx1), y0 = floor(by1), x1 = floor(bx2), y1 = floor(by2); o = t / 2 (integer division).  The outer rectangle is
 *            O = [x0 - o, x1 + o] x [y0 - o, y1 + o], inclusive.
 *   outline  the pixels of O that are not in [x0 - o + t, x1 + o - t] x [y0 - o + t, y1 + o - t] (when that inner rectangle is empty the
 *            outline is all of O).  The region of a COASTING track is dashed: only the pixels with
 *            ((x - (x0 - o)) + (y - (y0 - o))) / (2 t) even.
 *   discs    detected faces only (a coasting track has none; radius < 0: nobody has any).  Point k has the centre
 *            (floor(clamp(px[k] * s)), floor(clamp(py[k] * s))); a point with a non-finite product is skipped.  Its disc is the pixels
 *            with dx * dx + dy * dy <= r * r.
 *   label    n digits.  RF_OVERLAY_LABEL_SCORE: v = (int)(score * 100.f) clamped to 0..99, NaN -> 0, always two digits (of a coasting
 *            track: the score of its box).  RF_OVERLAY_LABEL_ID: the decimal digits of id mod 1 000 000 without leading zeros; no label
 *            when id <= 0 (faces tagged RF_TRACK_UNTRACKED and faces without ids included).  The plate is PW = f + 6 f n wide and
 *            PH = 9 f tall; its left edge is x0 - o, its rows are [y0 - o - PH, y0 - o - 1], or [y0 - o, y0 - o + PH - 1] when that top
 *            row is < 0.  Digit j, glyph bit (gx, gy) (gx 0..4 from the left, gy 0..6 from the top) covers the f x f square at
 *            plate-relative (f + 6 f j + f gx, f + f gy).  The glyphs are 5 x 7, rows top to bottom, most significant bit on the left:
 *              0: 0E 11 13 15 19 11 0E   1: 04 0C 04 04 04 04 0E   2: 0E 11 01 02 04 08 1F   3: 1F 02 04 02 01 11 0E   4: 02 06 0A 12 1F 02 02
 *              5: 1F 10 1E 01 01 11 0E   6: 06 08 10 1E 11 11 0E   7: 1F 01 02 04 08 08 08   8: 0E 11 11 0E 11 11 0E   9: 0E 11 11 0F 01 02 0C
 *   colour   of a region: `box`; with color_by_id and id > 0 the palette entry id & 7 of (0,0,255) (0,255,0) (255,0,0) (0,255,255)
 *            (255,0,255) (255,255,0) (0,128,255) (255,128,0) (B, G, R).  Plate and outline take the region's colour, glyph pixels `text`,
 *            discs `point`.
 *   list     of image i: exactly redaction's -- its faces k < min(counts[i], max_regions) in score order, then with a tracker its
 *            stream's live tracks with 1 <= missed <= coast in ascending slot order at `last` (with a motion tracker at the predicted
 *            box), their ids the tracks'; cut at max_regions.
 *   owner    within a region the priority is glyph > plate > disc (lower k first) > outline.  A pixel is painted by the lowest-indexed
 *            region that has any primitive covering it, and takes that region's highest-priority primitive there.
 *   value    out = (orig * (255 - a) + colour * a + 127) / 255 per channel, of the ORIGINAL byte.  Every painted pixel is painted once;
 *            every other byte of the frame and of its row padding is untouched.  Everything is clipped to [0, cols) x [0, rows).
 *   results  pixels[i * max_regions + r] (may be NULL): the pixels region r painted; region_counts[i] (may be NULL): the length of the
 *            list before the cut; a cut list returns RF_ERR_TRUNCATED.
 * There is no fused redact-plus-overlay call: a caller follows a redacting call with rf_overlay_device on the faces it returned. */
enum { RF_OVERLAY_LABEL_NONE = 0, RF_OVERLAY_LABEL_SCORE = 1, RF_OVERLAY_LABEL_ID = 2 };
typedef struct rf_overlay_spec {   /* 40 bytes; a field of 0 means its default, a NULL spec all defaults */
    uint32_t struct_size;   /* sizeof(rf_overlay_spec) */
    int32_t thickness;      /* of the outline, 1..16; 0 = 2 (the reference's) */
    int32_t radius;         /* of a landmark disc, 1..16; 0 = 2; negative = no landmarks */
    uint8_t box[3];         /* B, G, R of outline and plate; all zero (and colors_set 0) = (0, 0, 255), the reference's */
    uint8_t colors_set;     /* 1: box, point and text are taken as they are, so that all zero is black; 0 or 1 */
    uint8_t point[3];       /* of the discs; all zero = (0, 255, 0), the reference's */
    uint8_t alpha;          /* 1..255; 0 = 255 (opaque) */
    uint8_t text[3];        /* of the glyphs; all zero = (255, 255, 255) */
    uint8_t color_by_id;    /* 0 / 1: a region with id > 0 takes its colour from the palette */
    int32_t label;          /* RF_OVERLAY_LABEL_NONE / _SCORE / _ID */
    int32_t font_scale;     /* pixels per glyph bit, 1..8; 0 = 2 */
    int32_t max_regions;    /* as rf_redact_spec.max_regions */
    int32_t coast;          /* as rf_redact_spec.coast */
} rf_overlay_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.  rf_overlay_region: the record of one face with
 * track id `id` (0 = none): out = x0, y0, x1, y1, the bounding rectangle of everything it paints bx0, by0, bx1, by1 (inclusive,
 * unclipped), digit count n, the digits (digit j in bits 4 j .. 4 j + 3), plate left, plate top, colour (B | G << 8 | R << 16), a mask of the
 * points that have a disc, the five centres cx[5], cy[5]: 24 values.  Returns 1 (valid), 0 (invalid region: out is all zero) or
 * RF_ERR_INVALID_ARG (bad spec, NULL argument, rows or cols < 0). */
int rf_overlay_region(const rf_overlay_spec *spec, const rf_face *face, int64_t id, float coord_scale, int rows, int cols, int32_t out[24]);
/* Draws into a whole frame in place in HOST memory (the CPU counterpart of rf_overlay_device for one image without a tracker; a usable
 * fallback).  ids: one per face, or NULL = none.  pixels: min(count, max_regions) counts, may be NULL.  Returns 0, RF_ERR_TRUNCATED
 * (count > max_regions: the first max_regions faces were drawn) or RF_ERR_INVALID_ARG, which changes nothing. */
int rf_overlay_host(const rf_overlay_spec *spec, uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, const int64_t *ids,
                    int count, float coord_scale, int32_t *pixels);

/* Draws faces the CALLER supplies (host memory, as rf_redact_device; ids: NULL or ids[i * cap_per_image + k]) in place in
 * device-resident frames; no forward pass runs.  coord_scale: per image, NULL = 1.  tracker may be NULL; with one, stream_of_image[i]
 * names the stream whose coasting tracks (the tracker's CURRENT table) are drawn dashed in image i, -1 = faces only; a stream may appear
 * at most once per call.  A NULL / 0 x 0 frame is skipped.  Refused before any state changes, as by rf_redact_device: a bad spec, a
 * NULL frame array, two frames of the call whose byte ranges overlap (RF_ERR_INVALID_ARG), a frame resident on another GPU, a
 * multi-device handle (RF_ERR_UNSUPPORTED). */
int rf_overlay_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
                      const int64_t *ids, int cap_per_image, const int *counts, const float *coord_scale, const rf_overlay_spec *spec,
                      rf_tracker tracker, const int *stream_of_image, int32_t *pixels, int *region_counts);
/* Measurement hook: the time of the two overlay launches of the handle's most recent rf_overlay_device call, between two HIP events on
 * its stream (the upload and the copy-out are outside).  RF_ERR_INVALID_ARG before the first such call. */
int rf_overlay_last_launch_ms(rf_handle h, float *ms);

/* rf_detect_batch_device + the overlay of what it finds, in one call: detection runs exactly as there (out / counts /
 * rf_last_anchor_indices are the same bytes); the two overlay launches follow each detection launch on its stream and read the faces
 * from the device-visible result block -- no host synchronisation in between.  coord_scale is each frame's rf_frame_scale; faces have
 * no ids.  n may exceed max_batch.  pixels: n * max_regions, may be NULL.  Refusals as above. */
int rf_detect_overlay_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                   float threshold, rf_face *out, int cap_per_image, int *counts, const rf_overlay_spec *spec,
                                   int32_t *pixels);
/* Frames in host memory: uploaded once, detected and drawn into on that copy; the annotated frames go to out_bgr[i] with rows of
 * out_steps[i] bytes (NULL = cols * 3), which may be the input buffers. */
int rf_detect_overlay_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                            float threshold, rf_face *out, int cap_per_image, int *counts, const rf_overlay_spec *spec,
                            uint8_t *const *out_bgr, const int *out_steps, int32_t *pixels);
/* rf_detect_track_batch_device + overlay: the overlay launches sit behind each track launch; the id of a face is the one in the tag the
 * track launch wrote for it (an image of stream -1 has no ids), and the coasting tracks are those of the table AFTER this call's frame
 * step.  Each stream may appear at most once per call (RF_ERR_INVALID_ARG otherwise).  Tags, ended lists and the tracker's state are
 * the bytes of the tracked call without overlay. */
int rf_detect_track_overlay_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                         float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                         const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                         const rf_overlay_spec *spec, int32_t *pixels, int *region_counts);

/* ---- Motion-predicted face tracks: a tracker may keep a velocity per track slot and match and coast at the PREDICTED box, so a face
 * that moves while the detector drops it keeps its id and stays covered (DESIGN.md "Motion-predicted tracks" holds the definition;
 * tests/motion_ref.py restates it in numpy; every result is byte-exact against it).  All arithmetic is fp32 with one rounding per
 * operation, never contracted.  rf_track, rf_track_tag and rf_track.last (the last OBSERVED face) are what they were.
 *   record     one rf_track_motion per slot; a free slot and a newly opened track have the all-zero record
 *   predicted  face of a live track h frames ahead: samples == 0 or h == 0: `last`, the same bytes, no arithmetic.  Otherwise
 *              dx = vx * (float)h, dy = vy * (float)h; every x coordinate (x1, x2, px[0..4]) becomes x + dx, every y coordinate y + dy; the
 *              score is copied.  The box keeps its observed size.
 *   frame step rf_track_step's with two changes.  `match` compares d_k with the track's predicted box for h = min(missed + 1, horizon)
 *              (h = 0 with a negative horizon), taken once at the start of the image's step; expression, eligibility, tie rule and greedy
 *              order are unchanged.  A matched track updates its velocity before `last` is overwritten: dt = (float)(missed + 1) with
 *              missed from before the match; rx = ((nx1 + nx2) * 0.5f - (lx1 + lx2) * 0.5f) / dt, n the new mapped box, l the old `last`;
 *              ry likewise; samples == 0: v = r, else v = v + alpha * (r - v) (a subtract, a multiply, an add).  vx or vy not finite: the
 *              record becomes all zero; else samples = min(samples + 1, 1 << 30).  A slot that ends or is opened gets the zero record.
 *   redaction  the coasting entries of the region list (1 <= missed <= coast) use the predicted box for h = min(missed, horizon).
 * With a negative horizon tags, ended lists, counts and tables are the bytes of the plain tracker; only the records differ. */
typedef struct rf_motion_spec {
    uint32_t struct_size;   /* sizeof(rf_motion_spec) */
    float alpha;            /* weight of the newest velocity sample, finite and in (0, 1]; 0 = 0.5 */
    int32_t horizon;        /* most frames a box is extrapolated, 1..65536; 0 = 8; negative = never extrapolate */
    int32_t reserved;       /* must be 0 */
} rf_motion_spec;
typedef struct rf_track_motion { float vx, vy; int32_t samples; int32_t reserved; } rf_track_motion;   /* 16 bytes, no padding */

/* Host only, no GPU, no handle.  rf_track_step_motion: rf_track_step plus a caller-held array of max_tracks motion records (all zero to
 * start); mspec NULL = all defaults.  A bad mspec (wrong size, non-zero reserved, a field out of range) is RF_ERR_INVALID_ARG like any
 * other bad argument and changes nothing.
 * rf_track_predict: the predicted face of a live track for h = min(missed + ahead, horizon), ahead 0 (where redaction coasts) or 1 (where
 * the next frame step matches).  RF_ERR_INVALID_ARG for a free slot (id 0), a bad spec, another `ahead` or a NULL argument. */
int rf_track_step_motion(const rf_track_spec *spec, const rf_motion_spec *mspec, rf_track *table, rf_track_motion *motion, int64_t *frames,
                         int64_t *next_id, const rf_face *faces, int count, float coord_scale, const rf_face_quality *quality,
                         int max_faces, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_count);
int rf_track_predict(const rf_motion_spec *mspec, const rf_track *track, const rf_track_motion *motion, int ahead, rf_face *out);

/* Gives the tracker motion for its lifetime: every tracked call (rf_track_update_device, rf_detect_track_batch*,
 * rf_detect_track_face_batch_device, rf_track_shots_device, rf_detect_track_shots_batch*, rf_detect_track_redact_batch_device) then runs
 * the motion frame step, and rf_redact_device / rf_detect_track_redact_batch_device coast at the predicted boxes; their other outputs are
 * defined as before, from the tags the step produced.  Refused with RF_ERR_INVALID_ARG, changing nothing, for a bad spec, a tracker that
 * has stepped a frame (any stream's frame counter non-zero) or one that has motion already.  Composes with rf_tracker_enable_shots in
 * either order.  rf_tracker_reset, rf_tracker_flush and rf_tracker_flush_shots zero the records of the slots they free. */
int rf_tracker_enable_motion(rf_tracker tracker, const rf_motion_spec *mspec);
/* Host copy of the first min(cap, max_tracks) motion records of a stream.  Returns max_tracks; RF_ERR_INVALID_ARG without motion. */
int rf_tracker_read_motion(rf_tracker tracker, int stream, rf_track_motion *out, int cap);

/* ---- Followed face tracks: a tracker may keep, per track slot, a template of the face's luma taken on a KEY frame (a frame with
 * detections) and, on the frames in between, measure from the new frame's pixels -- without a forward pass -- where each tracked face
 * went: a block-matching search over luma cell means moves the track's box by whole cells (DESIGN.md "Followed tracks" holds the
 * definition; tests/follow_ref.py restates it in numpy; every result is byte-exact against it).  All arithmetic is integer, except one
 * fp32 add per coordinate of a moved box, never contracted.  G = 32; luma Y = (29 B + 150 G + 77 R + 128) >> 8.
 *   geometry   of a box (x1, y1, x2, y2; fp32, source-frame pixels): every coordinate must be finite and is clamped to [-4096, 8192];
 *              ix = floor(.), W = ix2 - ix1 + 1, H likewise; invalid unless W >= 1 and H >= 1.  Cell edge q = max(1, (max(W, H) + G - 1) / G),
 *              origin ox = floordiv(ix1 + ix2 + 1 - G q, 2), oy likewise.
 *   cell value at cell origin (cx, cy): (sum of Y over the q x q pixels (cx + x, cy + y) + q q / 2) / (q q), every pixel coordinate clamped
 *              into the frame (replicated border): nothing outside the frame is read, whatever the row step or base pointer.
 *   template   of a slot: the G x G cell values (u8, row-major) at (ox + i q, oy + j q).
 *   record     one rf_track_follow per slot; a free slot has the all-zero record.  dx, dy are pixels (du q, dv q).
 *   search     in a new frame, radius R: the window is the (G + 2R)^2 cell values at (ox + (i - R) q, oy + (j - R) q); for du, dv in [-R, R]
 *              SAD(du, dv) = sum |T[j][i] - Wn[j + dv + R][i + du + R]|.  A candidate is eligible only if the moved centre
 *              (ox + du q + 16 q, oy + dv q + 16 q) lies inside the frame.  The winner is the eligible candidate with the smallest 64-bit
 *              key SAD << 32 | (du^2 + dv^2) << 16 | ((dv + R)(2R + 1) + du + R): ties go to the smaller motion, then raster order, so a
 *              flat frame answers "did not move".  The winner is accepted when SAD <= max_mad G G.
 *   key step   rf_track_step, unchanged (a NULL / 0 x 0 frame has no faces); then every slot the step left free gets the zero record, and
 *              for every face the step tagged with slot >= 0 the slot's template is retaken from this image at the track's `last` box
 *              and its record becomes {1, 0, q, ox, oy, 0, 0, 0} -- the zero record for an invalid geometry.  Live tracks nobody
 *              matched keep template and record.
 *   follow step  f = the stream's frame counter, which advances by one.  Every live slot on its own: it is attempted when valid is set,
 *              run < max_run and the frame is not NULL / 0 x 0.  Accepted: every x coordinate of `last` (x1, x2, px[0..4]) gets one
 *              fp32 add of (float)(du q), every y coordinate of (float)(dv q); the score is copied; ox, oy move by the same integers;
 *              run += 1; sad, dx, dy are stored; hits, missed, last_frame and best are untouched.  Otherwise missed += 1, sad = the
 *              winner's SAD or -1 (no attempt, no eligible candidate), dx = dy = 0, and the track ends when missed > max_missed: ended
 *              list in ascending slot order, slot freed, record zeroed.  No tracks are opened.  The output list of the image is the
 *              accepted slots in ascending order: out = the moved `last`, tag as rf_track_step's for frame f with flag RF_TRACK_FOLLOWED.
 * The template is taken only at key steps: every search compares against the same key-frame template on a lattice that moves by whole
 * cells, so quantisation (at most q / 2 per axis) does not accumulate; max_run bounds how long appearance may drift. */
enum { RF_TRACK_FOLLOWED = 32 };
typedef struct rf_follow_spec {   /* 20 bytes; a field of 0 means its default, a NULL spec all defaults */
    uint32_t struct_size;   /* sizeof(rf_follow_spec) */
    int32_t radius;         /* search radius in cells, 1..16; 0 = 8 */
    int32_t max_mad;        /* largest accepted mean absolute difference per cell, 1..255; 0 = 16 */
    int32_t max_run;        /* most follow steps between two key steps, 1..65536; 0 = 8 */
    int32_t reserved;       /* must be 0 */
} rf_follow_spec;
typedef struct rf_track_follow { int32_t valid, run, q, ox, oy, sad, dx, dy; } rf_track_follow;   /* 32 bytes, no padding */

/* Host only, no GPU, no handle: the code the kernels run, compiled for the host.
 * rf_follow_geometry: out = {q, ox, oy}; returns 1 (valid), 0 (invalid: out is zero) or RF_ERR_INVALID_ARG (NULL argument).
 * rf_follow_template: the 1024 template bytes of the lattice (q, ox, oy) in a frame (rows of `step` bytes, step >= cols * 3).
 * rf_follow_search: out = {state, sad, du, dv}; state 1 = no eligible candidate (sad -1), 2 = the winner.  q 1..385, radius 1..16.
 * rf_track_step_follow_key / rf_track_step_follow: the two whole steps on a caller-held table, max_tracks records and
 * max_tracks x 1024 template bytes (all zero to start).  The follow step writes the first min(*count, cap) accepted faces and tags;
 * *count and *ended_count are the true numbers.  Returns as rf_track_step: 0, RF_ERR_TRUNCATED (a full table, a cut output or ended
 * list) or RF_ERR_INVALID_ARG, which changes nothing. */
int rf_follow_geometry(const float box[4], int32_t out[3]);
int rf_follow_template(const uint8_t *bgr, int rows, int cols, int step, int q, int ox, int oy, uint8_t *tpl);
int rf_follow_search(const uint8_t *bgr, int rows, int cols, int step, const uint8_t *tpl, int q, int ox, int oy, int radius, int32_t out[4]);
int rf_track_step_follow_key(const rf_track_spec *spec, rf_track *table, rf_track_follow *records, uint8_t *templates, int64_t *frames,
                             int64_t *next_id, const uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, int count,
                             float coord_scale, const rf_face_quality *quality, int max_faces, rf_track_tag *tags, rf_track *ended,
                             int cap_ended, int *ended_count);
int rf_track_step_follow(const rf_track_spec *spec, const rf_follow_spec *fspec, rf_track *table, rf_track_follow *records,
                         const uint8_t *templates, int64_t *frames, const uint8_t *bgr, int rows, int cols, int step, rf_face *out,
                         rf_track_tag *tags, int cap, int *count, rf_track *ended, int cap_ended, int *ended_count);

/* Gives the tracker follow for its lifetime: n_streams x max_tracks records and templates (1024 bytes each, at most RF_SHOT_MAX_BYTES in
 * all) in device memory.  Refused with RF_ERR_INVALID_ARG, changing nothing, for a bad spec, a tracker that has stepped a frame (any
 * stream's frame counter non-zero) or one that has follow already.  It does not compose yet: a tracker that has a gallery or motion is
 * refused here, and rf_tracker_enable_shots / rf_tracker_enable_motion refuse a tracker that has follow.  Every tracked call without
 * "follow" in its name then refuses the tracker (RF_ERR_INVALID_ARG, nothing changes): it would leave a template stale.  In a
 * follow call each stream may appear at most once (RF_ERR_INVALID_ARG otherwise); an image of stream -1 is skipped.
 * rf_tracker_reset and rf_tracker_flush zero the records of the slots they free. */
int rf_tracker_enable_follow(rf_tracker tracker, const rf_follow_spec *spec);
/* Host copy of the first min(cap, max_tracks) records and templates (1024 bytes per slot; zeros where the record is not valid) of a
 * stream; each may be NULL.  Returns max_tracks; RF_ERR_INVALID_ARG without follow. */
int rf_tracker_read_follow(rf_tracker tracker, int stream, rf_track_follow *records, uint8_t *templates, int cap);

/* Key steps.  rf_track_follow_update_device: rf_track_update_device over faces the caller supplies (host memory, in source-frame pixels
 * after coord_scale) plus the frames they were found in (device memory), with the keep rule behind the track launch; what a tiled
 * caller uses.  rf_detect_track_follow_batch_device / rf_detect_track_follow_batch: rf_detect_track_batch_device / rf_detect_track_batch
 * plus the keep rule, with no host synchronisation between detection and the keep launch; out, counts, tags, ended lists and the table
 * are the bytes of the plain tracked call. */
int rf_track_follow_update_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                                  int n, const int *stream_of_image, const rf_face *faces, int cap_per_image, const int *counts,
                                  const float *coord_scale, const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended,
                                  int cap_ended, int *ended_counts);
int rf_detect_track_follow_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                        float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                        const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);
int rf_detect_track_follow_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                 const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);
/* Follow steps: no forward pass runs.  Frames in device memory (rf_track_follow_device) or host memory (rf_track_follow_batch: uploaded
 * densely, as the redacting host call uploads them).  out / tags: image i's followed faces at out + i * cap_per_image (the first
 * min(counts[i], cap_per_image)); counts[i]: the true number.  A cut output or ended list returns RF_ERR_TRUNCATED. */
int rf_track_follow_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                           const int *stream_of_image, rf_face *out, int cap_per_image, int *counts, rf_track_tag *tags, rf_track *ended,
                           int cap_ended, int *ended_counts);
int rf_track_follow_batch(rf_handle h, rf_tracker tracker, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          const int *stream_of_image, rf_face *out, int cap_per_image, int *counts, rf_track_tag *tags, rf_track *ended,
                          int cap_ended, int *ended_counts);
/* Measurement hook: hipEvent time (ms) of the search and step launches of the most recent rf_track_follow_device call, on their stream
 * (the upload and the copy-out are outside).  RF_ERR_INVALID_ARG before the first such call. */
int rf_follow_last_launch_ms(rf_handle h, float *ms);

/* ---- Flip test-time augmentation with box voting: every frame is detected as it is and mirrored left-right, the mirrored faces are
 * moved back into the frame, and overlapping boxes of both passes are merged on the device into a score-weighted mean (DESIGN.md "Flip
 * test-time augmentation" holds the definition; tests/tta_ref.py restates it in numpy; every result is byte-exact against it):
 *   passes   pass 0 is the frame; pass 1 (flip on) the frame mirrored, M[y][x] = F[y][cols - 1 - x].  Over a call the passes are
 *            frame-major: f0, f0 mirrored, f1, f1 mirrored ...  The result of a pass is exactly what rf_detect_batch_device returns for
 *            that image at the call's threshold -- to the byte when that ONE call holds all passes of the TTA call in that order, the
 *            mirrors as dense frames of their own (the caveat of the tiled call's views: the last bits of an image's result depend on
 *            how it lies in memory, not on what shares its launch).  Frames larger than the net are shrunk as always, in both passes.  A NULL / 0 x 0 frame finds nothing.
 *   mapping  face k of pass p: all 14 coordinates get one fp32 multiply by rf_frame_scale(rows, cols) (also when it is 1).  For p = 1,
 *            with c = (float)(cols - 1): x1' = c - x2, x2' = c - x1, px'[i] = c - px[perm[i]], py'[i] = py[perm[i]], perm = {1, 0, 2, 4, 3}
 *            (left and right eye, left and right mouth corner change places): one fp32 subtract per x coordinate; y and the score are
 *            untouched.  Results are in SOURCE-FRAME pixels: their coord_scale for the alignment and face-batch calls is 1.
 *   merge    per frame, over the mapped faces of its passes: order by score descending (bit order), then g = p * max_detections + k
 *            ascending; greedy suppression exactly as the detector's NMS (+1-pixel areas, skipped when w <= 0 || h <= 0, strict
 *            > nms_threshold of the handle).  The CLUSTER of a kept head is the head and every candidate it suppresses.  vote off: the
 *            output is the heads.  vote on: a head keeps its score and g, and each of its 14 coordinates q becomes (float)(acc_q / sw),
 *            sw = sum (double)s_m, acc_q = sum (double)s_m * (double)v_mq over the members in the total order, head first, one double
 *            rounding per add (a product of two floats is exact in double).  A head without other members keeps its bytes.
 *   outputs  counts[i]: the true number of heads; out[i * cap_per_image + k]: the first min(counts[i], cap_per_image, max_faces) in
 *            merge order; votes (may be NULL; same indexing): the members of each; src_pass (may be NULL): g / max_detections of the head.
 *   caps     RF_ERR_TRUNCATED as for the tiled call: a pass whose own result was truncated, a frame with more than 4096 candidates
 *            (its faces are then unspecified, the other frames valid), a list that max_faces or cap_per_image cut.
 * There is no on-device minimum-votes filter: `votes` lets the caller choose. */
typedef struct rf_tta_spec {
    uint32_t struct_size;   /* sizeof(rf_tta_spec) */
    int32_t flip;           /* 0 / 1 = also detect the frame mirrored; 2 = off (one pass per frame) */
    int32_t vote;           /* 0 / 1 = kept boxes become the score-weighted mean of their cluster; 2 = off (plain greedy NMS) */
    int32_t max_faces;      /* merged faces kept per frame on the device, 1..4096; 0 = the engine's max_detections */
} rf_tta_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.
 * rf_tta_map_face: the mapping of one face of pass `pass` (0 or 1) of a rows x cols frame at a net_h x net_w net (out may equal in).
 * rf_tta_merge_host: mapping and merge of ONE frame: pass p holds pass_counts[p] faces (clamped to max_detections) at
 * faces[p * max_detections + k]; two passes, one with flip off.  spec may be NULL (max_faces 0 stands for max_detections).  *count is the
 * true number of heads; out / votes / src_pass (the last two may be NULL) receive the first min(*count, cap, max_faces).  Returns RF_OK,
 * RF_ERR_TRUNCATED (a pass count above max_detections, or a cut list) or RF_ERR_INVALID_ARG. */
int rf_tta_map_face(int rows, int cols, int net_h, int net_w, int pass, const rf_face *in, rf_face *out);
int rf_tta_merge_host(const rf_tta_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_pass);

/* The mirror kernel on its own: d_dst row y (at d_dst + y * dst_step, cols * 3 bytes; bytes beyond them are untouched) is row y of the
 * BGR frame d_src (row pitch `step`, any pointer alignment; ROI views are legal) mirrored left-right.  Synchronous. */
int rf_mirror_device(rf_handle h, const void *d_src, int rows, int cols, int step, void *d_dst, int dst_step);

/* TTA detection of frames resident on the engine's device (frame limits as rf_detect_batch_device).  The mirrored copies are made on
 * the device in front of the call's first detection launch; the passes of all frames go through the engine's ordinary launches; a
 * gather kernel behind each launch applies the mapping, and one merge launch behind the call's last launch waits for them on the device
 * -- no host synchronisation in between.  spec may be NULL.  A bad spec is refused before any state changes.  Multi-device handles
 * return RF_ERR_UNSUPPORTED from this call, the next two and rf_mirror_device.  rf_last_anchor_indices / rf_last_candidate_counts afterwards describe
 * the call's PASSES. */
int rf_detect_tta_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_tta_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                               int *src_pass);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely. */
int rf_detect_tta_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                        float threshold, const rf_tta_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass);

/* Mapping and merge of per-pass faces the CALLER supplies (host memory): with P = 2 (flip off: 1) passes per frame, pass p of frame i
 * holds pass_counts[i * P + p] faces (clamped to max_detections) at faces[(i * P + p) * max_detections + k].  No forward pass runs. */
int rf_tta_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_tta_spec *spec, const rf_face *faces,
                        const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass);

/* ---- Rotation-robust detection: the detector finds upright faces; a frame that arrives turned by a quarter, a half or three quarters
 * of a turn (phone video without its orientation tag, scans, ceiling cameras) loses faces and score.  A rotation call detects every
 * frame in up to four orientations, the rotated copies made on the device, moves the faces of all passes back into the frame and merges
 * them on the device with the merge of the TTA call; the same call tells which way is up (DESIGN.md "Rotation-robust detection" holds the
 * definition; tests/rot_ref.py restates it in numpy; every result is byte-exact against it):
 *   passes   pass k (k = 0..3) of a rows x cols frame F is F turned by k quarter turns counter-clockwise, np.rot90(F, k):
 *              k = 0: F itself;                       k = 1: D is cols x rows, D[y][x] = F[x][cols - 1 - y];
 *              k = 2: D[y][x] = F[rows - 1 - y][cols - 1 - x];     k = 3: D is cols x rows, D[y][x] = F[rows - 1 - x][y].
 *            rots is a bit mask of the k to run (0 = all four).  Over a call the passes are frame-major, ascending k.  A pass is an
 *            ordinary image of the call: a rotated pass larger than the net is shrunk as always, and its result is exactly what
 *            rf_detect_batch_device returns for that image at the call's threshold -- to the byte when that ONE call holds all passes of
 *            the rotation call in that order, the rotated copies as dense frames of their own (the caveat of the TTA call: the last
 *            bits of an image's result depend on how it lies in memory, not on what shares its launch).  A NULL / 0 x 0 frame finds nothing.  A pass that breaks a
 *            frame limit of rf_detect_batch_device: RF_ERR_INVALID_ARG, before any state changes.
 *   mapping  face j of pass k: all 14 coordinates get one fp32 multiply by rf_frame_scale(rows_k, cols_k), the PASS's own shape
 *            ((cols, rows) for odd k), also when it is 1.  Then, with c = (float)(cols - 1) and r = (float)(rows - 1) of the source
 *            frame, a point (x', y') of the pass becomes  k = 1: (c - y', x');  k = 2: (c - x', r - y');  k = 3: (y', r - x')  -- one fp32
 *            subtract where a coordinate flips.  Boxes: k = 1: x1 = c - y2', x2 = c - y1', y1 = x1', y2 = x2'; k = 2: x1 = c - x2',
 *            x2 = c - x1', y1 = r - y2', y2 = r - y1'; k = 3: x1 = y1', x2 = y2', y1 = r - x2', y2 = r - x1'.  The landmarks keep their
 *            index (a rotation keeps handedness: no left / right swap); the score is untouched.  Results are in SOURCE-FRAME pixels:
 *            their coord_scale for the alignment and face-batch calls is 1.
 *   merge    rf_tta_spec's merge over the mapped faces of a frame's passes, g = k * max_detections + j with k the ROTATION (not the
 *            ordinal of the pass); src_rot = g / max_detections is the rotation the head came from.  vote: 0 / 2 = off (the default: a
 *            sideways pass gives a poorer box and unreliable landmarks for the same face; the head, almost always from the upright
 *            pass, wins unaveraged), 1 = on.  max_faces, outputs and caps (RF_ERR_TRUNCATED) as for the TTA call.  With rots = 1 and
 *            vote off, out and counts are the bytes of the TTA call with flip off.
 *   orientation  two optional outputs: rot_score[i * 4 + k] = (float) of the double sum, in merge order, of the scores of frame i's
 *            emitted heads with src_rot == k; frame_rot[i] = the k with the largest sum (ties: the lowest k), -1 for a frame without a
 *            head.  Turning the frame by frame_rot quarter turns counter-clockwise makes it upright. */
typedef struct rf_rot_spec {
    uint32_t struct_size;   /* sizeof(rf_rot_spec) */
    int32_t rots;           /* bit k: run pass k; 1..15; 0 = 15 (all four) */
    int32_t vote;           /* 0 / 2 = off (plain greedy NMS over all passes); 1 = kept boxes become the score-weighted mean of their cluster */
    int32_t max_faces;      /* merged faces kept per frame on the device, 1..4096; 0 = the engine's max_detections */
} rf_rot_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.
 * rf_rot_map_face: the mapping of one face of pass k (0..3) of a rows x cols frame at a net_h x net_w net (out may equal in).
 * rf_rot_merge_host: mapping and merge of ONE frame: with P = popcount(rots) passes in ascending k, the p-th of them holds pass_counts[p]
 * faces (clamped to max_detections) at faces[p * max_detections + j].  spec may be NULL (max_faces 0 stands for max_detections).  *count is
 * the true number of heads; out / votes / src_rot (the last two may be NULL) receive the first min(*count, cap, max_faces); frame_rot (one
 * int) and rot_score (four floats) may be NULL.  Returns RF_OK, RF_ERR_TRUNCATED (a pass count above max_detections, or a cut list) or
 * RF_ERR_INVALID_ARG.
 * rf_rotate_host: pass k (0..3; 0 is a row copy) of the rows x cols BGR frame src (row pitch step), written as cols_k * 3 bytes per row
 * at dst + y * dst_step (bytes beyond them are untouched). */
int rf_rot_map_face(int rows, int cols, int net_h, int net_w, int k, const rf_face *in, rf_face *out);
int rf_rot_merge_host(const rf_rot_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_rot,
                      int *frame_rot, float *rot_score);
int rf_rotate_host(const uint8_t *src, int rows, int cols, int step, int k, uint8_t *dst, int dst_step);

/* The rotate kernel on its own: rf_rotate_host for a frame and a destination in device memory (any source pitch and pointer alignment;
 * ROI views are legal).  Synchronous. */
int rf_rotate_device(rf_handle h, const void *d_src, int rows, int cols, int step, int k, void *d_dst, int dst_step);

/* Rotation detection of frames resident on the engine's device (frame limits as rf_detect_batch_device).  The rotated copies are made
 * on the device in front of the call's first detection launch; the passes of all frames go through the engine's ordinary launches; a
 * gather kernel behind each launch applies the mapping, and one merge launch behind the call's last launch waits for them on the device
 * -- no host synchronisation in between.  spec may be NULL; votes, src_rot (indexed like out), frame_rot (n ints) and rot_score (n * 4
 * floats) may be NULL.  A bad spec is refused before any state changes.  Multi-device handles return RF_ERR_UNSUPPORTED from this call,
 * the next two and rf_rotate_device.  rf_last_anchor_indices / rf_last_candidate_counts afterwards describe the call's PASSES. */
int rf_detect_rot_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_rot_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                               int *src_rot, int *frame_rot, float *rot_score);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely. */
int rf_detect_rot_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                        float threshold, const rf_rot_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_rot,
                        int *frame_rot, float *rot_score);

/* Mapping and merge of per-pass faces the CALLER supplies (host memory): with P = popcount(rots) passes per frame in ascending k, the
 * p-th pass of frame i holds pass_counts[i * P + p] faces (clamped to max_detections) at faces[(i * P + p) * max_detections + j].  No
 * forward pass runs. */
int rf_rot_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_rot_spec *spec, const rf_face *faces,
                        const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_rot, int *frame_rot,
                        float *rot_score);

/* ---- Fisheye detection: under a ceiling or door camera with a fisheye lens a face sits on a circle around the lens centre, turned by its
 * azimuth and stretched by the lens; quarter turns do not undo a lens.  A fisheye call makes up to 16 dewarped VIEWS (virtual pan / tilt
 * cameras) of every frame on the device, detects them, moves the faces of all views back into the frame through the views' meshes and
 * merges them on the device with the merge of the TTA call (DESIGN.md "Fisheye detection" holds the definition; tests/dewarp_ref.py
 * restates it in numpy; every result is byte-exact against it):
 *   mesh     a dewarper holds V views (1..16) of view_w x view_h pixels, both multiples of 16, at most 4096 x 3072.  Each view has a mesh of
 *            (view_h / 16 + 1) x (view_w / 16 + 1) NODES: node (i, j) is the source position of view pixel (16 i, 16 j), two int32, x then
 *            y, in 1/256 px, |value| <= 2^22.  Layout: view-major, then row-major nodes, x and y interleaved.  The device only ever sees
 *            meshes; the lens trigonometry (rf_dewarp_plan) stays on the host, and a caller with their own calibration brings a mesh.
 *   pixel    exact integers, >> arithmetic.  View pixel (X, Y): cell (X >> 4, Y >> 4), u = X & 15, v = Y & 15; per coordinate
 *            S = n00 (16 - u)(16 - v) + n10 u (16 - v) + n01 (16 - u) v + n11 u v (fits int32); q = (S + 1024) >> 11 in 1/32 px;
 *            x0 = q >> 5, w = q & 31.  The byte is (sum of tap * wx' * wy' + 512) >> 10 over the four taps (x0, y0) .. (x0 + 1, y0 + 1)
 *            with weights 32 - w and w; a tap outside the rows x cols source reads as 0; the channels are independent.
 *   passes   frame-major, ascending view.  A view is an ordinary image of the call: its result is exactly what rf_detect_batch_device
 *            returns for it (the caveat of the rotation call holds: to the byte when ONE call holds all views as dense frames).  A NULL
 *            frame finds nothing; a frame whose shape is not the dewarper's: RF_ERR_INVALID_ARG before any state changes.
 *   mapping  face j of view v, on its 15 floats.  p = in * rf_frame_scale(view_h, view_w), one fp32 multiply.  pq = p * 256.0f, clamped to
 *            [-4096, 256 dim + 4096] (dim = view_w for x, view_h for y) with two compares, c = pq > lo ? pq : lo; c = c < hi ? c : hi, so a
 *            NaN becomes lo; q = (int)rintf(c).  cell = clamp(q >> 12, 0, cells - 1), u = q - 4096 cell: linear extrapolation over at most
 *            one cell beyond the view.  Node weights 4096 - u and u per axis, the sum in int64; r = (S + 2^23) >> 24 in 1/256 px; the
 *            result is (float)r * (1 / 256.f), exact.  Landmarks are mapped point by point; the score is untouched.  The box is the
 *            min / max, in integers, over eight mapped points: the four corners and the four edge midpoints, xm = (x1q + x2q) >> 1 -- so
 *            x1 <= x2 and y1 <= y2 stay.  Results are in SOURCE-FRAME pixels.
 *   edge     with edge > 0 a face whose SCALED box has x1 < edge, y1 < edge, x2 > view_w - 1 - edge or y2 > view_h - 1 - edge is dropped
 *            (its neighbour view sees it whole); 0, the default, drops nothing.
 *   merge    rf_tta_spec's merge over the mapped faces of a frame's views, g = view * max_detections + j; src_view = g / max_detections.
 *            vote: 0 / 2 = off (the default, as for rotation), 1 = on.  max_faces, outputs and caps (RF_ERR_TRUNCATED) as for the TTA call.
 *   plan     rf_dewarp_plan, host only, doubles.  The lens: model (r = f theta, 2 f sin(theta / 2), 2 f tan(theta / 2), f sin theta), f in
 *            px, the centre (cx, cy).  Views: yaw, pitch, roll, hfov in degrees; ring = N gives N views at yaw 360 j / N with one pitch and
 *            one hfov, roll 0.  The node of view pixel (X, Y): fv = (view_w / 2) / tan(hfov / 2); d = R ((X - (view_w - 1) / 2) / fv,
 *            (Y - (view_h - 1) / 2) / fv, 1) with R = Rz(yaw) Rx(pitch) Rz(roll); theta = atan2(hypot(dx, dy), dz), psi = atan2(dy, dx);
 *            s = (cx + r(theta) cos psi, cy + r(theta) sin psi); node = lrint(256 s).  At yaw 0 and pitch > 0 the view's centre lies above
 *            the lens centre and the view's up points away from it: where a standing person's head is under a ceiling camera.  Refused:
 *            a view that reaches theta >= pi (orthographic: pi / 2), a node beyond +-2^22. */
#define RF_DEWARP_MAX_VIEWS 16
#define RF_LENS_EQUIDISTANT 0
#define RF_LENS_EQUISOLID 1
#define RF_LENS_STEREOGRAPHIC 2
#define RF_LENS_ORTHOGRAPHIC 3
typedef struct rf_dewarp_view {
    double yaw, pitch, roll, hfov;   /* degrees */
} rf_dewarp_view;
typedef struct rf_dewarp_spec {
    uint32_t struct_size;   /* sizeof(rf_dewarp_spec) */
    int32_t model;          /* RF_LENS_* */
    double f, cx, cy;       /* focal length and lens centre, source pixels */
    int32_t views;          /* 1..16 explicit views in view[]; 0 with a ring */
    int32_t ring;           /* 1..16: that many views at equal yaw steps with ring_pitch and ring_hfov; 0 with explicit views */
    double ring_pitch, ring_hfov;
    rf_dewarp_view view[RF_DEWARP_MAX_VIEWS];
    int32_t vote;           /* 0 / 2 = off; 1 = kept boxes become the score-weighted mean of their cluster */
    int32_t max_faces;      /* merged faces kept per frame on the device, 1..4096; 0 = the engine's max_detections */
    int32_t edge;           /* the edge rule, view pixels, 0..1024; 0 = off */
    int32_t reserved_;
} rf_dewarp_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.
 * rf_dewarp_plan: the meshes of the spec's views at view_w x view_h (multiples of 16) into mesh, which holds cap_ints int32; *views
 * receives the number of views (each (view_h / 16 + 1) * (view_w / 16 + 1) * 2 ints).  RF_ERR_INVALID_ARG for a bad or refused spec or a
 * mesh that is too small.
 * rf_dewarp_host: one view, whose nodes are view_mesh, of the rows x cols BGR frame src (row pitch step), written as view_w * 3 bytes per
 * row at dst + y * dst_step (bytes beyond them are untouched).
 * rf_dewarp_map_face: edge rule and mapping of one face of the view whose nodes are view_mesh.  Returns 1 (kept, out written; out may
 * equal in), 0 (dropped by the edge rule) or RF_ERR_INVALID_ARG.
 * rf_dewarp_merge_host: mapping and merge of ONE frame: view v holds pass_counts[v] faces (clamped to max_detections) at
 * faces[v * max_detections + j]; mesh holds all views.  Only vote, max_faces and edge of spec are read; spec may be NULL.  *count is the
 * true number of heads; out / votes / src_view (the last two may be NULL) receive the first min(*count, cap, max_faces).  Returns RF_OK,
 * RF_ERR_TRUNCATED (a pass count above max_detections, or a cut list) or RF_ERR_INVALID_ARG. */
int rf_dewarp_plan(const rf_dewarp_spec *spec, int view_w, int view_h, int32_t *mesh, int cap_ints, int *views);
int rf_dewarp_host(const int32_t *view_mesh, int view_w, int view_h, const uint8_t *src, int rows, int cols, int step, uint8_t *dst,
                   int dst_step);
int rf_dewarp_map_face(const int32_t *view_mesh, int view_w, int view_h, int net_h, int net_w, int edge, const rf_face *in, rf_face *out);
int rf_dewarp_merge_host(const rf_dewarp_spec *spec, const int32_t *mesh, int view_w, int view_h, int views, int net_h, int net_w,
                         float nms_threshold, int max_detections, const rf_face *faces, const int *pass_counts, rf_face *out, int cap,
                         int *count, int *votes, int *src_view);

/* A dewarper: one camera's views on a handle -- the shape of its frames, the views' shape and their meshes, uploaded once.  view_w /
 * view_h 0 = the net size.  Refused (RF_ERR_INVALID_ARG): rows * cols outside (0, 4096 x 3072], a bad view shape or count, a NULL mesh, a
 * node beyond +-2^22.  Freed by rf_dewarper_destroy or with the handle; until the handle is destroyed, every call on a destroyed
 * dewarper returns RF_ERR_INVALID_ARG.  Multi-device handles return RF_ERR_UNSUPPORTED. */
typedef struct rf_dewarper_s *rf_dewarper;
int rf_dewarper_create(rf_handle h, int rows, int cols, int view_w, int view_h, int views, const int32_t *mesh, rf_dewarper *out_dewarper);
void rf_dewarper_destroy(rf_dewarper dewarper);

/* The dewarp kernel on its own: view `view` of a frame of the dewarper's shape in device memory (any source pitch and pointer
 * alignment) into a destination in device memory, view_w * 3 bytes per row at d_dst + y * dst_step.  Synchronous. */
int rf_dewarp_device(rf_dewarper dewarper, int view, const void *d_src, int step, void *d_dst, int dst_step);

/* Fisheye detection of frames resident on the engine's device.  rows and cols (each may be NULL: the dewarper's) name every frame's shape,
 * which must be the dewarper's (0 x 0 or a NULL pointer: an empty frame); steps may be NULL (dense).  The views are made by one kernel on the
 * device in front of the call's first detection launch; the views of all frames go through the engine's ordinary launches; a gather
 * kernel behind each launch applies the edge rule and the mapping, and one merge launch behind the call's last launch waits for them on the
 * device -- no host synchronisation in between.  Only vote, max_faces and edge of spec are read; spec may be NULL.  votes and src_view
 * (indexed like out) may be NULL.  d_views, when not NULL, is device memory of n * V * view_h * view_w * 3 bytes that receives the views as
 * dense frames, frame-major (a NULL frame's are left untouched): upright pixels for a recogniser.  The views' bytes and the faces do not
 * depend on it when it is 256-byte aligned, as a fresh allocation is.  rf_last_anchor_indices / rf_last_candidate_counts afterwards
 * describe the call's PASSES. */
int rf_detect_dewarp_batch_device(rf_dewarper dewarper, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                  float threshold, const rf_dewarp_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_view,
                                  void *d_views);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely. */
int rf_detect_dewarp_batch(rf_dewarper dewarper, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                           float threshold, const rf_dewarp_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_view);

/* Mapping and merge of per-view faces the CALLER supplies (host memory): view v of frame i holds pass_counts[i * V + v] faces (clamped to
 * max_detections) at faces[(i * V + v) * max_detections + j].  No forward pass runs. */
int rf_dewarp_merge_device(rf_dewarper dewarper, int n, const rf_dewarp_spec *spec, const rf_face *faces, const int *pass_counts,
                           rf_face *out, int cap_per_image, int *counts, int *votes, int *src_view);

/* ---- Region detection: run the detector only where told to.  The caller names up to 256 REGIONS of every frame (the last key frame's
 * faces grown by a margin, a person detector's boxes, a motion mask); a region call packs them, several to a net-sized VIEW, on the
 * device, detects the views, moves the faces back into the frame and merges them on the device with the merge of the TTA call: true
 * boxes, landmarks and scores for a fraction of the tiled call's passes (DESIGN.md "Region detection" holds the definition;
 * tests/roi_ref.py restates it in numpy; every result is byte-exact against it):
 *   region   rf_roi {x, y, w, h}, int32 source pixels: w, h in [1, 16384], |x|, |y| <= 2^20.  It may reach outside the frame or lie
 *            wholly outside it.  Each frame has its own list; the lists of a call are concatenated frame-major in `rois`,
 *            roi_counts[i] (0..256) entries for frame i.
 *   grid     a view of net_w x net_h is cut into grid x grid cells (grid 1, 2 or 4) of cw = net_w / grid by ch = net_h / grid pixels;
 *            net_w and net_h must divide evenly and cw must be a multiple of 4.  Region r of a frame goes to cell r mod grid^2
 *            (row-major) of pass r / grid^2.  A frame without regions has no pass and no faces; unused cells of the last pass are 0.
 *   step     each region is shown at one of five levels, x4, x2, x1, x1/2, x1/4 (rf_roi_cell.level = 2, 1, 0, -1, -2): the largest not
 *            above max_zoom with w z <= cw and h z <= ch.  None fits: x1/4, the cell shows the region's centre, flags = RF_ROI_CROPPED.
 *   level    x2 / x4: the pyramid call's zoom (half-pixel centres, clamped at the frame border); x1: the frame; x1/2, x1/4: the rounded
 *            box mean (sum + k^2 / 2) / k^2 of the k x k source block, source coordinates clamped into the frame, a level image of
 *            ceil(cols / k) x ceil(rows / k) pixels.
 *   cell     c2 = 2 x + w (twice the centre); the cell's origin in level pixels is x0 = floor((c2 z - cw) / 2) for z >= 1 and
 *            x0 = floor((c2 - k cw) / (2 k)) for a shrink by k; y0 likewise.  Cell pixel (i, j) is level pixel (x0 + i, y0 + j); a level
 *            pixel outside the level image is 0.  The cell is filled with the real pixels around the region, not with padding.
 *   faces    on the 15 floats of a face of a view.  Its cell is the one its box centre (x1 + x2) * 0.5f, (y1 + y2) * 0.5f lies in; a
 *            cell without a region drops it.  Every coordinate gets one fp32 add of the integer x0 - cell_x (y0 - cell_y), then for a
 *            zoom * (1 / z) - (z - 1) / 2z, for a shrink * k + (k - 1) / 2.  The face is kept only when its mapped centre lies in
 *            [x, x + w) x [y, y + h): a neighbour that shows up in a cell's context is its own region's business.  Scores are untouched.
 *   merge    rf_tta_spec's merge over the kept faces of a frame, g = region * max_detections + j; src_roi = g / max_detections.
 *            vote: 0 / 2 = off (the default), 1 = on.  max_faces, outputs and caps (RF_ERR_TRUNCATED) as for the TTA call. */
#define RF_ROI_MAX_REGIONS 256
#define RF_ROI_CROPPED 1
#define RF_ROI_VOID 2       /* a cell without a region: every other field 0 (tracked region detection, below) */
typedef struct rf_roi {
    int32_t x, y, w, h;
} rf_roi;
typedef struct rf_roi_cell {
    rf_roi roi;
    int32_t level;          /* log2 of the step: 2, 1, 0, -1, -2 */
    int32_t x0, y0;         /* the cell's origin in level pixels */
    int32_t flags;          /* RF_ROI_CROPPED, or RF_ROI_VOID alone */
} rf_roi_cell;
typedef struct rf_roi_spec {
    uint32_t struct_size;   /* sizeof(rf_roi_spec) */
    int32_t grid;           /* 1, 2 or 4; 0 = 4 */
    int32_t max_zoom;       /* 1, 2 or 4; 0 = 2 */
    int32_t vote;           /* 0 / 2 = off; 1 = kept boxes become the score-weighted mean of their cluster */
    int32_t max_faces;      /* merged faces kept per frame on the device, 1..4096; 0 = the engine's max_detections */
    int32_t reserved;       /* 0 */
} rf_roi_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.  Only grid and max_zoom of spec are read where
 * no merge happens; spec may be NULL.  view_w x view_h is the view's size (the net's in a region call).
 * rf_roi_plan: the cells of n regions (0..256) into cells[n]; *passes (may be NULL) receives ceil(n / grid^2).
 * rf_roi_from_faces: the regions of n faces: each box times coord_scale, grown on every side by margin_q8 / 256 of its longer side
 * (0 = 64, a quarter), lower edges floored, upper edges ceiled, sides held to [1, 16384].  Faces whose box is not finite, is empty or
 * lies beyond +-2^20 are skipped.  Returns the number of regions written to rois (at most n), so that one call's result can be handed
 * to the next call.
 * rf_roi_atlas_host: all passes of the regions of the rows x cols BGR frame src (row pitch step): pass p is written as view_w * 3 bytes
 * per row at dst + (p * view_h + y) * dst_step (bytes beyond a row are untouched).
 * rf_roi_map_face: the face rule for one face of pass `pass` of the n regions.  Returns 1 (kept, out written, *region (may be NULL) its
 * region; out may equal in), 0 (dropped) or RF_ERR_INVALID_ARG.
 * rf_roi_merge_host: mapping and merge of ONE frame: pass p holds pass_counts[p] faces (clamped to max_detections) at
 * faces[p * max_detections + j].  *count is the true number of heads; out / votes / src_roi (the last two may be NULL) receive the
 * first min(*count, cap, max_faces).  Returns RF_OK, RF_ERR_TRUNCATED (a pass count above max_detections, or a cut list) or
 * RF_ERR_INVALID_ARG. */
int rf_roi_plan(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, rf_roi_cell *cells, int *passes);
int rf_roi_from_faces(const rf_face *faces, int n, float coord_scale, int margin_q8, rf_roi *rois);
int rf_roi_atlas_host(const rf_roi_spec *spec, int view_w, int view_h, const uint8_t *src, int rows, int cols, int step, const rf_roi *rois,
                      int n, uint8_t *dst, int dst_step);
int rf_roi_map_face(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, int pass, const rf_face *in, rf_face *out,
                    int *region);
int rf_roi_merge_host(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_roi);

/* The atlas kernel on its own: all passes of the n regions of a frame in device memory (any source pitch and pointer alignment) into a
 * destination in device memory laid out as rf_roi_atlas_host's, at any view size that meets the cell rule.  Synchronous.  Multi-device
 * handles return RF_ERR_UNSUPPORTED from this call and the next three. */
int rf_roi_atlas_device(rf_handle h, const void *d_src, int rows, int cols, int step, const rf_roi *rois, int n, const rf_roi_spec *spec,
                        int view_w, int view_h, void *d_dst, int dst_step);

/* Region detection of frames resident on the engine's device (a NULL pointer or 0 x 0: an empty frame, which finds nothing; steps may be
 * NULL: dense).  The views of all frames are made by one kernel on the device in front of the call's first detection launch and go
 * through the engine's ordinary launches; a gather kernel behind each launch applies the face rule, and one merge launch behind the
 * call's last launch waits for them on the device -- no host synchronisation in between.  Everything is checked before any state
 * changes: a bad spec, a net that does not meet the cell rule, a region out of range, a count outside 0..256 are RF_ERR_INVALID_ARG.
 * votes and src_roi (indexed like out) may be NULL.  d_views, when not NULL, is device memory of P * net_h * net_w * 3 bytes, P the
 * call's passes (frame-major, ascending region; sum of ceil(roi_counts[i] / grid^2)), that receives the views as dense frames (a NULL
 * frame's are left untouched).  rf_last_anchor_indices / rf_last_candidate_counts afterwards describe the call's PASSES. */
int rf_detect_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               const rf_roi *rois, const int *roi_counts, float threshold, const rf_roi_spec *spec, rf_face *out,
                               int cap_per_image, int *counts, int *votes, int *src_roi, void *d_views);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely. */
int rf_detect_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, const rf_roi *rois,
                        const int *roi_counts, float threshold, const rf_roi_spec *spec, rf_face *out, int cap_per_image, int *counts,
                        int *votes, int *src_roi);

/* Face rule and merge of per-pass faces the CALLER supplies (host memory): the call's passes in the order above, pass q holds
 * pass_counts[q] faces (clamped to max_detections) at faces[q * max_detections + j].  No forward pass runs. */
int rf_roi_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_roi *rois, const int *roi_counts,
                        const rf_roi_spec *spec, const rf_face *faces, const int *pass_counts, rf_face *out, int cap_per_image, int *counts,
                        int *votes, int *src_roi);

/* ---- Tracked region detection: the regions of a frame are planned ON THE DEVICE from a tracker's table, and the merged faces go
 * straight into the frame step -- "key frame, then regions around the faces of the last frame" with no host synchronisation between the
 * table and the tags (DESIGN.md "Tracked region detection" holds the definition; tests/roi_track_ref.py restates it in numpy):
 *   slot = region   region r of an image is slot r of the image's stream, so every live tracked image has ceil(max_tracks / grid^2)
 *            passes whatever the table holds; pass p has min(grid^2, max_tracks - p grid^2) cells.  A caller who wants one pass per
 *            frame creates the tracker with max_tracks <= grid^2.
 *   cell     a free slot gets the VOID record (every field 0, flags = RF_ROI_VOID).  A live slot's box is its track's `last` box, or
 *            for a tracker with motion the predicted box the next frame step matches against; the region is rf_roi_from_faces' of that
 *            box at coord_scale 1 and margin_q8 (0 = 64), the cell rf_roi_plan's.  A box rf_roi_from_faces would skip: void.
 *   void     a void cell is zero pixels, addresses no source byte and drops every face whose centre falls in it.  rf_roi_atlas_host,
 *            rf_roi_atlas_device and rf_roi_map_face take the void region {0, 0, 0, 0} in their lists from this version on; rf_roi_plan
 *            and the region calls above refuse it as before and never produce a void record.
 *   step     after the merge one frame step per image (rf_track_step, or rf_track_step_motion) runs over the merged faces in merge
 *            order at coord_scale 1, m = min(count, max_faces, 256); nothing about the step changes -- a face found in slot s's region
 *            is not forced onto slot s.  src_roi[k] is the slot whose region found face k, tags[k].slot the slot that claimed it.
 *   frames   a NULL / 0 x 0 frame has no passes and no faces, its stream still takes a step and ages; an image of stream -1 has no
 *            regions, no faces and no step.  Each stream may appear at most once per call.
 * Refused before any state changes (RF_ERR_INVALID_ARG): a bad spec, a net that does not meet the cell rule, margin_q8 outside
 * [0, 65535], a stream twice in the call, a tracker with a shot gallery or with follow (they do not compose yet), a tracker in the
 * error state.  Multi-device handles: RF_ERR_UNSUPPORTED.
 *
 * rf_roi_cells_from_tracks (host only, no GPU, no handle): the max_tracks cell records of one stream's table -- the code the plan kernel
 * runs.  spec (may be NULL) is checked only; motion NULL: a plain tracker, else max_tracks records read with mspec (NULL: its defaults).
 * rf_roi_track_cells_device: the plan kernel alone over the tables of `tracker`: image i's max_tracks records at cells[i * max_tracks]
 * (an image of stream -1: void records).  Synchronous; changes nothing.
 * rf_detect_track_roi_batch_device / rf_detect_track_roi_batch: the fused call.  Frames, out, cap_per_image, counts, tracker,
 * stream_of_image, tags, ended, cap_ended, ended_counts as rf_detect_track_batch*; votes, src_roi (may be NULL) and d_views (may be NULL:
 * device memory of P * net_h * net_w * 3 bytes, P = ceil(max_tracks / grid^2) per live tracked frame, frame-major) as
 * rf_detect_roi_batch_device; cells (may be NULL) receives the n * max_tracks records the device planned (void for images without
 * passes).  Returns RF_ERR_TRUNCATED as the region call and the tracked calls do.  An error after the step was enqueued leaves the
 * tracker in the error state until it is reset. */
int rf_roi_cells_from_tracks(const rf_track_spec *spec, const rf_motion_spec *mspec, const rf_track *table, const rf_track_motion *motion,
                             int max_tracks, int margin_q8, int net_w, int net_h, const rf_roi_spec *roi_spec, rf_roi_cell *cells);
int rf_roi_track_cells_device(rf_handle h, rf_tracker tracker, const int *stream_of_image, int n, int margin_q8, const rf_roi_spec *roi_spec,
                              rf_roi_cell *cells);
int rf_detect_track_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                     float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                                     int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_tracker tracker,
                                     const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts);
int rf_detect_track_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                              const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts, int *src_roi, int *votes,
                              rf_roi_cell *cells, void *d_views, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                              rf_track *ended, int cap_ended, int *ended_counts);

/* ---- Change regions: a region exists above only where a track already is, so a face that enters the scene between two key frames is
 * seen by nothing until the next key frame.  A CHANGER keeps a small per-stream reference image in device memory -- one luma sum per
 * block of the frame -- and turns the blocks of a frame that differ from it into regions ON THE DEVICE; they go through the same atlas,
 * launches, gather and merge, alone or next to a tracker's regions in one call (DESIGN.md "Change regions" holds the definition;
 * tests/change_ref.py restates it in numpy; everything up to the regions is integer arithmetic and byte-exact against it):
 *   spec     a zero field means its default.  block B: 8, 16 or 32 (16).  thr_q4: 1..65535, the mean luma difference of a block in
 *            1/16 grey levels (128 = 8 grey levels).  adapt_shift a: 0..8 (0: the reference becomes the frame).  dilate: 0 / 1 = grow
 *            the mask by one block, 8-neighbourhood; 2 = off.  min_blocks: 1..65535 (2).  max_regions R: 1..64 (16).
 *   changer  made for one frame shape and n_streams (1..1024) streams, as a dewarper is made for one shape.  The block grid is
 *            bw = ceil(cols / B) by bh = ceil(rows / B), bw * bh <= 16384 (4K at B = 32, 1080p at B = 16); anything else is refused.
 *   value    S(block) = sum of 29 b + 150 g + 77 r over the block's pixels inside the frame (uint32).  This is 256 x luma WITHOUT the
 *            per-pixel rounding of the face-quality luma ((29 b + 150 g + 77 r + 128) >> 8): the sum is taken over the packed bytes
 *            with 4-byte dot products and never unpacks a pixel.
 *   step     each stream keeps ref[bh * bw] (int32) and a frame counter.  The first step after creation or reset SEEDS: ref = S, no
 *            block is changed, every cell is void, info.flags = 1.  Every other step, per block with npix pixels inside the frame:
 *            changed = |S - ref| > 16 * thr_q4 * npix, then ref += (S - ref) >> a (arithmetic, floors).
 *   regions  the mask is dilated as the spec says; the 8-connected sets of marked blocks are the components: label = the smallest
 *            raster index, count = marked blocks after dilation, box = bounding box in blocks.  Components with count < min_blocks
 *            are dropped, the rest ordered by count descending, then label ascending, the first R kept.  Kept component k: the pixel
 *            rectangle x = bx0 B, y = by0 B, x2 = min(cols, (bx1 + 1) B), y2 = min(rows, (by1 + 1) B) goes as a face box through
 *            rf_roi_from_faces' rule at coord_scale 1 and margin_q8 (0 = 64) and rf_roi_plan's into cell k.  Slots k >= kept, and every
 *            slot of a seeding step, get the void record.  A whole-frame change (lights, a moved camera) is one large region, which
 *            may be RF_ROI_CROPPED; info.changed_blocks is how a caller recognises it and runs a key frame instead.
 *   info     changed_blocks (before dilation), components (before the min_blocks drop), kept, flags (1: the step seeded).
 *   fused    every image with pixels has ceil((T + R) / grid^2) passes, T = the tracker's max_tracks (0 without one), T + R <= 256:
 *            region r < T is track slot r exactly as in tracked region detection, region T + k is change slot k; src_roi indexes that
 *            list and cells receives n * (T + R) records.  With a tracker the merged faces go into the frame step: a newcomer gets its
 *            id on the frame it appears in.  One index names the stream of both the changer and the tracker, whose n_streams must
 *            match; a stream may appear once per call.  A NULL / 0 x 0 frame has no passes and does not touch the reference (with a
 *            tracker its stream still steps and ages); stream -1: nothing happens for the image.
 * Refused before any state changes (RF_ERR_INVALID_ARG): a bad spec, a net that does not meet the cell rule, margin_q8 outside
 * [0, 65535], T + R > 256, mismatched stream counts, a stream twice in the call, a frame whose shape is not the changer's, a tracker
 * with a gallery or with follow, a changer or tracker in the error state.  Multi-device handles: RF_ERR_UNSUPPORTED.  An error after
 * the step was enqueued leaves the changer (and the tracker) in the error state until rf_changer_reset(changer, -1).
 *
 * rf_changer_create / rf_changer_destroy: as for a dewarper; freed with the handle at the latest.  rf_changer_reset: stream (-1: all)
 * seeds again.  rf_changer_read: the reference (bw * bh int32), the frame counter and the last mask (bw * bh bytes, the changed blocks
 * BEFORE dilation) of a stream; each may be NULL; returns bw * bh.
 * rf_change_step_host (host only, no GPU, no handle): one step of one stream -- the code the kernels run.  ref (bw * bh) and *counter
 * in and out; mask (bw * bh bytes), regions and cells (max_regions records each; zeros / void records behind info->kept) and info out.
 * rf_change_regions_device: the two kernels alone over frames in device memory; they STEP the reference.  Image i's R records at
 * cells[i * R], its info at info[i] (stream -1 or no pixels: void records, zero info).  Synchronous.
 * rf_detect_change_roi_batch_device / rf_detect_change_roi_batch: the fused call.  Arguments as rf_detect_track_roi_batch*; tracker
 * may be NULL (then tags, ended, ended_counts are not written); info (may be NULL) receives n records. */
typedef struct rf_change_spec {
    uint32_t struct_size;   /* sizeof(rf_change_spec) */
    int32_t block;
    int32_t thr_q4;
    int32_t adapt_shift;
    int32_t dilate;
    int32_t min_blocks;
    int32_t max_regions;
    int32_t reserved;       /* 0 */
} rf_change_spec;
typedef struct rf_change_info {
    int32_t changed_blocks, components, kept, flags;
} rf_change_info;
typedef struct rf_changer_s *rf_changer;
int rf_changer_create(rf_handle h, const rf_change_spec *spec, int rows, int cols, int n_streams, rf_changer *out_changer);
void rf_changer_destroy(rf_changer changer);
int rf_changer_reset(rf_changer changer, int stream);
int rf_changer_read(rf_changer changer, int stream, int32_t *ref, int64_t *frames, uint8_t *mask);
int rf_change_step_host(const rf_change_spec *spec, const uint8_t *bgr, int rows, int cols, int step, int32_t *ref, int64_t *counter,
                        int margin_q8, int net_w, int net_h, const rf_roi_spec *roi_spec, uint8_t *mask, rf_roi *regions, rf_roi_cell *cells,
                        rf_change_info *info);
int rf_change_regions_device(rf_handle h, rf_changer changer, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                             const int *stream_of_image, int n, int margin_q8, const rf_roi_spec *roi_spec, rf_roi_cell *cells,
                             rf_change_info *info);
int rf_detect_change_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                                      int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_changer changer, rf_change_info *info,
                                      rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended,
                                      int *ended_counts);
int rf_detect_change_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                               int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_changer changer, rf_change_info *info,
                               rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended,
                               int *ended_counts);

/* ---- Zoom-pyramid detection: the smallest anchors are 16 px, so faces below about 16 px are not seen in a frame that already fits the
 * net.  A pyramid call detects every frame at 1x (the passes of its tile plan) and as net-sized tiles of the frame ENLARGED 2x and / or 4x
 * on the device, moves the faces of all passes back into the frame and merges them with the voting merge of the TTA call (DESIGN.md
 * "Zoom-pyramid detection" holds the definition; tests/pyramid_ref.py restates it in numpy; every result is byte-exact against it):
 *   plan     three groups in this order: level 1x (levels bit 0): the passes of rf_tile_plan(rows, cols) in its order, its full-frame
 *            pass included; level 2x (bit 1): the tiles of the tile plan of a VIRTUAL 2 rows x 2 cols frame with full_frame off,
 *            row-major; level 4x (bit 2): the same for 4 rows x 4 cols.  overlap and edge are in net pixels at every level.  More than
 *            1024 passes per frame, or zoom tiles of more than RF_PYRAMID_MAX_ZOOM_BYTES in one call (each tile tw * th * 3 bytes rounded
 *            up to 256): RF_ERR_INVALID_ARG, before any state changes.  A NULL / 0 x 0 frame is one pass that finds nothing.
 *   zoom     Z = zoom(F, z), z = 2 or 4: bilinear with half-pixel centres, in integers.  Per axis of length n, output index X:
 *            D = 2z, num = 2X + 1 - z, i0 = floor(num / D), w = num - i0 * D, i1 = i0 + 1, then i0 and i1 are clamped to [0, n - 1].
 *            Per channel, a, b on row y0 and c, d on row y1:  acc = ((D - wx) a + wx b)(D - wy) + ((D - wx) c + wx d) wy,
 *            out = (acc + D * D / 2) >> (2 log2 D).  Zoom tile (X0, Y0, tw, th) is Z[Y0 : Y0 + th, X0 : X0 + tw]: the clamp is at the
 *            FRAME border, never at the tile border, so neighbouring tiles agree on their overlap.
 *   pass     the result of a pass is exactly what rf_detect_batch_device returns for that image at the call's threshold -- to the byte
 *            when that ONE call holds all passes of the pyramid call in plan order, 1x tiles as ROI views, zoom tiles as dense frames of
 *            their own (the caveat of the tiled call's views: the last bits of an image's result depend on how it lies in memory, not on what shares its launch).
 *   mapping  a 1x pass: rf_tile_map_face.  A zoom pass: the edge rule of rf_tile_map_face in tile coordinates against the virtual frame
 *            (z cols, z rows); then every x becomes (x + (float)X0) * inv - off, every y (y + (float)Y0) * inv - off, inv = 1 / z,
 *            off = (z - 1) / 2z (0.25 at 2x, 0.375 at 4x): the pixel-centre correspondence.  Scores are unchanged.  Results are in
 *            SOURCE-FRAME pixels: their coord_scale for the alignment and face-batch calls is 1.
 *   merge    rf_tta_spec's merge over the surviving faces of all passes of a frame, g = p * max_detections + k with p the pass index in
 *            the plan; outputs and caps as for the TTA call (src_pass = g / max_detections).
 * With levels = 1 and vote = 2 (off), out, counts and src_pass are the bytes of rf_detect_tiled_batch_device with the same overlap, edge,
 * full_frame and max_faces. */
#define RF_PYRAMID_MAX_ZOOM_BYTES (1u << 30)
typedef struct rf_pyramid_spec {
    uint32_t struct_size;   /* sizeof(rf_pyramid_spec) */
    int32_t levels;         /* bit 0: the 1x passes; bit 1: 2x zoom tiles; bit 2: 4x zoom tiles; 1..7; 0 = 3 (1x and 2x) */
    int32_t overlap;        /* as rf_tile_spec, in net pixels at every level */
    int32_t edge;           /* as rf_tile_spec, in net pixels at every level */
    int32_t full_frame;     /* as rf_tile_spec (level 1x only) */
    int32_t max_faces;      /* as rf_tile_spec */
    int32_t vote;           /* as rf_tta_spec.vote */
} rf_pyramid_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host.  spec may be NULL (all defaults; max_faces 0
 * stands for 256 in the first two, for max_detections in the third).
 * rf_pyramid_plan: the number of passes of a rows x cols frame at a net_h x net_w net, or RF_ERR_INVALID_ARG (bad spec, non-positive net
 * size, negative or over-size frame, more than 1024 passes, zoom tiles above RF_PYRAMID_MAX_ZOOM_BYTES).  zxywh (may be NULL) receives z, x0,
 * y0, tw, th of the first min(passes, cap_passes) passes, in the level's virtual pixels; a full-frame pass is 1, 0, 0, cols, rows.
 * rf_pyramid_map_face: edge rule and mapping of one face of pass p: 1 = kept, *out is the mapped face (out may equal in); 0 = dropped by
 * the edge rule; RF_ERR_INVALID_ARG as above or for p outside the plan.
 * rf_pyramid_merge_host: edge rule, mapping and merge of ONE frame: pass p holds pass_counts[p] faces (clamped to max_detections) at
 * faces[p * max_detections + k].  *count is the true number of heads; out / votes / src_pass (the last two may be NULL) receive the first
 * min(*count, cap, max_faces).  Returns RF_OK, RF_ERR_TRUNCATED (a pass count above max_detections, or a cut list) or RF_ERR_INVALID_ARG.
 * rf_zoom_host: the window [x0, x0 + tw) x [y0, y0 + th) of the rows x cols BGR frame src (row pitch step) enlarged z (2 or 4) times,
 * written as tw * 3 bytes per row at dst + y * dst_step (bytes beyond them are untouched).  The window lies inside the z rows x z cols
 * frame. */
int rf_pyramid_plan(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, int *zxywh, int cap_passes);
int rf_pyramid_map_face(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, int p, const rf_face *in, rf_face *out);
int rf_pyramid_merge_host(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                          const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_pass);
int rf_zoom_host(const uint8_t *src, int rows, int cols, int step, int z, int x0, int y0, int tw, int th, uint8_t *dst, int dst_step);

/* The zoom kernel on its own: rf_zoom_host for a frame and a destination in device memory (any source pitch and pointer alignment; ROI
 * views are legal).  Synchronous. */
int rf_zoom_device(rf_handle h, const void *d_src, int rows, int cols, int step, int z, int x0, int y0, int tw, int th, void *d_dst,
                   int dst_step);

/* Pyramid detection of frames resident on the engine's device (frame limits as rf_detect_batch_device).  The zoom tiles are made on the
 * device in front of the call's first detection launch; the passes of all frames go through the engine's ordinary launches; a gather
 * kernel behind each launch applies the edge rule and the mapping, and one merge launch behind the call's last launch waits for them
 * on the device -- no host synchronisation in between.  spec may be NULL.  A bad spec is refused before any state changes.
 * Multi-device handles return RF_ERR_UNSUPPORTED from this call, the next two and rf_zoom_device.  rf_last_anchor_indices /
 * rf_last_candidate_counts afterwards describe the call's PASSES, in plan order. */
int rf_detect_pyramid_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                   float threshold, const rf_pyramid_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                                   int *src_pass);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely. */
int rf_detect_pyramid_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                            float threshold, const rf_pyramid_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                            int *src_pass);

/* Edge rule, mapping and merge of per-pass faces the CALLER supplies (host memory): with first_pass[i] the running sum of the frames'
 * plan sizes, pass p of frame i holds pass_counts[first_pass[i] + p] faces (clamped to max_detections) at
 * faces[(first_pass[i] + p) * max_detections + k].  No forward pass runs. */
int rf_pyramid_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_pyramid_spec *spec, const rf_face *faces,
                            const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass);

/* Asynchronous form of rf_detect_batch_device for serving loops: enqueue returns as soon as the
 * batch is queued on the engine's stream (n <= max_batch); `ticket` identifies that batch until it has been
 * waited for.  rf_wait blocks until the batch has finished and copies its results; a ticket is waited for once
 * (a second rf_wait on it is RF_ERR_INVALID_ARG), in any order.  The engine merges consecutive enqueues into one
 * launch (options.coalesce; INTEGRATION.md states when a launch is closed) and overlaps launches on options.lanes
 * streams.
 * rf_num_slots() = lanes * coalesce is the number of outstanding tickets that keeps every lane busy with a full
 * launch, and the number a caller may always keep outstanding.  The ticket pool behind it holds
 * 4 * options.lanes * coalesce + 8 tickets: more than rf_num_slots() outstanding tickets are accepted up to that
 * pool size (a launch whose lane is needed again is collected into its tickets, which keep their results until they
 * are waited for), then rf_enqueue_batch* returns RF_ERR_INVALID_ARG ("too many outstanding tickets") and changes
 * nothing: every outstanding ticket still delivers its result. */
int rf_num_slots(rf_handle h);
int rf_enqueue_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols,
                            const int *steps, int n, float threshold, int *ticket);
int rf_wait(rf_handle h, int ticket, rf_face *out, int cap_per_image, int *counts);

/* Asynchronous form of rf_detect_batch: frames in HOST memory, exactly what the reference's callers hold (cv::Mat data / step,
 * RetinaFace.cpp:594, :760-782 upload them inside the call).  The frames are copied into the engine's pinned staging ring before
 * the call returns (the caller may reuse its buffers at once) by options.copy_threads host threads, cross PCIe as ONE DMA per
 * enqueue on the lane's stream, and that upload overlaps the compute of the super-batches already in flight on the other lanes.
 * Collect with rf_wait.  Frames inside a range registered with rf_host_register skip the staging copy: the DMA engine reads
 * them in place, so they must stay unchanged until the ticket has been waited for. */
int rf_enqueue_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols,
                     const int *steps, int n, float threshold, int *ticket);

/* Pin a caller-owned host range (a ring of camera / decoder buffers reused across calls) for in-place DMA, and release it.
 * rf_host_unregister first waits for every launch that may still read the range; rf_destroy releases what is left. */
int rf_host_register(rf_handle h, const void *ptr, size_t bytes);
int rf_host_unregister(rf_handle h, const void *ptr);

/* Where device frame pointers live (rf_detect_batch_device / rf_enqueue_batch_device on a node with several GPUs): the engine
 * asks the HIP runtime once per ALLOCATION and remembers the answer (own device / host-visible: read in place; another GPU:
 * peer copy over xGMI first); a remembered answer is re-checked against the runtime when it is older than 2 ms.  A caller that
 * FREES or RE-ALLOCATES frame buffers while the handle lives (hipFree + hipMalloc may hand the same address out on another
 * device) calls rf_invalidate_residency() after the free and before it passes pointers of the new allocation: the engine then
 * looks every pointer up afresh.  Frames passed to an outstanding ticket must stay allocated until rf_wait returns. */
int rf_invalidate_residency(rf_handle h);

/* Engines behind the handle: 1, or options.n_devices for an image-sharding multi-device handle. */
int rf_num_devices(rf_handle h);

/* The batch split in numbers (since rf_create, summed over the handle's engines): device frames that were found resident on ANOTHER
 * GPU and pulled over xGMI before their launch, and the hipMemcpyPeerAsync calls that carried them (frames that follow each other in
 * memory travel as one copy: a contiguous slice of a sharded batch = 1 copy; RF_SCATTER_PER_FRAME=1 in the environment = 1 per frame). */
int rf_scatter_stats(rf_handle h, long long *frames, long long *copies);

/* The coalescing scheduler in numbers (since rf_create, summed over the handle's engines): launches (super-batches) started by
 * synchronous calls, enqueues and waits, and the images in them.  Read-only. */
int rf_launch_stats(rf_handle h, long long *launches, long long *images);

/* Global anchor index (offset(stride) + a*h*w + iy*w + ix, strides 32,16,8) of each
 * detection of image `image` of the most recent completed batch, in the same order as out[]. */
int rf_last_anchor_indices(rf_handle h, int image, int32_t *out, int cap);
/* Number of above-threshold anchors (pre-NMS) per image of the most recent completed batch. */
int rf_last_candidate_counts(rf_handle h, int *counts, int n);

/* The reference's three timers (RetinaFace.cpp:757,836,840-842,846,920; README columns pre/infer/post),
 * measured with HIP events on the engine's stream for the most recent *synchronous* detect call.
 * Only filled when the call ran un-graphed (options.use_graph == 2); otherwise returns total only. */
int rf_last_timings(rf_handle h, float *pre_ms, float *infer_ms, float *post_ms, float *total_ms);

/* TrtRetinaFaceNet::blob_by_name(name)->result[image] (trtretinafacenet.cpp:104-114): one of the 9
 * output blobs ("face_rpn_cls_prob_reshape_stride32", "face_rpn_bbox_pred_stride16", ...) as NCHW fp32.
 * Requires options.keep_outputs = 1.  Returns the number of floats written (or needed if dst == NULL). */
long rf_get_output(rf_handle h, const char *blob_name, int image, float *dst, size_t cap_floats);

/* Test / profiling hooks (no reference equivalent).
 * rf_debug_activation: copy an internal NHWC activation of the last batch, converted to fp32, by the
 *   name of the reference blob it corresponds to (e.g. "mobilenet0_relu10_fwd", "rf_c2_aggr_relu").
 *   dims = {H, W, C}.  Returns floats written (or needed if dst == NULL), negative on error.  int8 engine: values are
 *   dequantised with the tensor's scale(s); "<blob>#raw" returns the stored quanta themselves (-127..127 as floats).
 * rf_profile: time every launch of the hot path on the engine's own stream with HIP events (each launch repeated
 *   back to back between one event pair so the event overhead is amortised), `iters` passes over a batch of n
 *   net-sized device frames; returns the number of launches, fills names (reference layers covered), kernels
 *   (kernel instance, e.g. "dwpw<128,128,s1>"; both up to cap entries, pointers owned by the engine), avg_ms, and
 *   the algorithmic bytes / MACs each launch covers (layer-wise input+output elements x element size). */
long rf_debug_activation(rf_handle h, const char *blob_name, int image, float *dst, size_t cap_floats,
                         int dims[3]);
int rf_profile(rf_handle h, const void *const *d_bgr, int n, int iters, int cap,
               const char **names, const char **kernels, float *avg_ms, double *alg_bytes, double *macs);
/* rf_profile_compulsory_bytes: for the same launches in the same order, the bytes each one has to move through HBM at the very
 *   least GIVEN its fusion, for n images -- every tensor it reads from HBM once + every tensor it writes once (weights ignored).
 *   bench.py's `useful` HBM fraction = these bytes / kernel time / peak (the layer-wise alg_bytes of rf_profile also count tensors
 *   that never leave LDS).  Returns the number of launches. */
int rf_profile_compulsory_bytes(rf_handle h, int n, int cap, double *bytes);
/* rf_debug_resident_cap: process-wide test hook for the persistent kernels' tile walk.  A persistent launch with more tiles than the
 *   chip keeps workgroups resident gets fewer workgroups than tiles, each walking several; with `workgroups` > 0 that resident count is
 *   replaced by `workgroups`, so small inputs walk as well (1 = one workgroup walks every tile).  0 (the default) = off, the production
 *   grids.  Launches that are not persistent keep their grids.  Only this call sets it: no environment variable does.  An engine that
 *   replays a captured graph keeps the grids it was captured with.  Also clears the log below.
 * rf_debug_grid_log: the (tiles, grid) pairs the persistent launches were given since the last rf_debug_resident_cap call, in call order
 *   (for a multi-level launch: all levels' tiles and the grid before it is shared out to the levels).  Writes up to `cap` pairs and returns
 *   how many were recorded; recording stops after 256.  Both are single-threaded test hooks: call them while no other thread launches. */
void rf_debug_resident_cap(int workgroups);
int rf_debug_grid_log(int cap, int *tiles, int *grid);
/* rf_debug_face_bands: test hook, host only (no handle, no GPU call).  The crop rows one workgroup of the face-crop kernels covers for
 *   `crop_size` in [16, 512] and `format` (RF_FACES_*) -- the band of rf_align_device, the face-batch calls and the gallery -- and the
 *   luma rows the quality kernel keeps in LDS for that crop size (each of its bands brings ring_rows - 2 new rows).  Either pointer may be
 *   NULL.  Returns RF_OK, or RF_ERR_INVALID_ARG for a crop size out of range or an unknown format. */
int rf_debug_face_bands(int crop_size, int format, int *band_rows, int *ring_rows);

/* Offline: pack <prototxt, caffemodel[, int8 table]> into a .rfw file (the analogue of the reference's
 * first-run engine serialisation, trtnetbase.cpp:231-243).  int8_table may be NULL. */
int rf_convert_model(const char *prototxt, const char *caffemodel, const char *int8_table,
                     const char *out_rfw);

/* Host-only test hook (runs without a GPU): BN-folded weights of one fused op of the plan compiled from
 * <model_dir>/<stem>.  op = "conv0", "dw<i>" / "pw<i>" (i = 0..12), "lateral<i>" (0..2), "aggr<i>" (0..1),
 * "ssh<i>.a" / ".b" / ".c" / ".head" (i = 0..2 for strides 32, 16, 8).  dims = {cout, k, k, cin/group};
 * w is [cout][k][k][cin/group], b is [cout].  Returns RF_OK or an error; pass NULL buffers to query dims. */
int rf_plan_folded(const char *model_dir, const char *stem, const char *op, float *w, size_t cap_w,
                   float *b, size_t cap_b, int dims[4]);

/* Host-only hook of the int8 calibration tool (tools/calibrate_int8.py --gptq; SURVEY 8f rank 3, reference INT8-Calibration-Tool/
 * calibrationtable.cpp:399-583 + TensorRT's own weight handling): one fused dense convolution of the int8 plan compiled from
 * <model_dir>/<stem> and the calibration table at `int8_table` (NULL: the one the model carries), BEFORE rounding: quanta[cout][ktot] = w * in_scale / row_scale (K order (ky, kx, c)),
 * in_scale[cin] (per input channel, as the engine applies it: a depthwise mid already carries the 127/255 of its 0..255 quanta),
 * row_scale[cout] (the weight grid), out_scale[cout] (1 for the heads).  dims = {cout, ktot, cin, input_is_u8_mid}.  op = the fused
 * op's name (reference layer names, '+'-joined when siblings are merged); op = "?<i>" enumerates: the i-th name comes back in `quanta`
 * (bytes) with its length in dims[0], RF_ERR_INVALID_ARG past the end.  NULL buffers are skipped. */
int rf_plan_int8_gemm(const char *model_dir, const char *stem, const char *int8_table, const char *op, float *quanta, size_t cap_q,
                      float *in_scale, size_t cap_in, float *row_scale, float *out_scale, size_t cap_out, int dims[4]);

/* Offline: <model_dir>/<stem> (an .rfw or prototxt + caffemodel) re-packed into out_rfw with a new calibration: int8_table (text,
 * the reference's format; NULL keeps the model's) and qweights ("<stem>.qweights.int8", the calibrated int8 weights tools/
 * calibrate_int8.py --gptq writes; NULL keeps the model's unless the table changed, which drops them).  The result is checked by
 * compiling and packing the int8 plan on the host; no GPU needed.  A scale that is not a positive finite number (zero, negative, NaN, inf)
 * is refused with RF_ERR_MODEL naming the tensor -- here for a table line or a scale the model carries, and by rf_create for an int8
 * engine; fp32 / fp16 engines never read the scales and still build from such a container. */
int rf_attach_calibration(const char *model_dir, const char *stem, const char *int8_table, const char *qweights, const char *out_rfw);

/* Host-only test hook: the host half of rf_create (plan cache or model -> packed weight image) for <model_dir>/<stem> at a
 * precision, with the cache file at cache_path (NULL = the default place).  Returns 1 when the image came from the cache, 0 when it was
 * built from the model (and the cache written), or a negative rf_status. */
int rf_plan_cache_probe(const char *model_dir, const char *stem, int precision, const char *cache_path, size_t *image_bytes);

int rf_abi_version(void);

/* ---- Low-light detection: a frame that is too dark (night streams, backlit doorways, a lit and an unlit half) loses its faces.  The
 * enhancement is contrast-limited adaptive histogram equalisation of luma (CLAHE) over a grid of tiles, applied as a hue-preserving gain;
 * only dark tiles are touched, and no pixel is ever darkened.  Exact integer arithmetic (DESIGN.md "Low-light detection" holds the
 * definition; tests/enhance_ref.py restates it in numpy; host and device results are byte-exact against it):
 *   luma     Y = (77 R + 150 G + 29 B + 128) >> 8 of a BGR pixel.
 *   tiles    ceil(rows / T) x ceil(cols / T); tile (j, i) covers rows [jT, min((j + 1)T, rows)) and columns likewise (n >= 1 pixels).
 *   LUT      h = the tile's luma histogram, c its inclusive prefix sum, p99 = the smallest v with 100 c[v] >= 99 n.  p99 >= dark_below:
 *            the tile is lit, its LUT is the identity.  Otherwise the tile is flagged and lim = max(1, (clip n) >> 16),
 *            ex = sum max(h[v] - lim, 0), h[v] = min(h[v], lim) + ex / 256 + (v < ex % 256 ? 1 : 0) (one redistribution pass),
 *            LUT[v] = max(v, (2 * 255 * c[v] + n) / (2 n)) with c the prefix sum of the new h.
 *   pixel    per axis, with D = 2T: p = 2y + 1 - T, q = floor(p / D), a0 = clamp(q, 0, nt - 1), a1 = clamp(q + 1, 0, nt - 1),
 *            w = p < 0 ? 0 : p mod D (tile centres are the nominal ones, also for ragged edge tiles).  With (j0, j1, wy) from y and
 *            (i0, i1, wx) from x: v = L[j0][i0][Y](D - wy)(D - wx) + L[j0][i1][Y](D - wy)wx + L[j1][i0][Y]wy(D - wx) + L[j1][i1][Y]wy wx,
 *            Yn = (2v + D^2) / (2 D^2).
 *   gain     Yn == Y: the three bytes are copied (so a frame of lit tiles comes back byte-identical).  Otherwise every channel c
 *            becomes min(255, (2 c Yn + Yd) / (2 Yd)) with Yd = max(Y, 1).
 * Appended after rf_abi_version: the ABI version stays 2. */
typedef struct rf_enhance_spec {
    uint32_t struct_size;   /* sizeof(rf_enhance_spec) */
    int32_t tile;           /* tile edge T in pixels: 16, 32, 64 or 128; 0 = 64 */
    int32_t clip;           /* contrast limit in 1/256ths of a tile's mean bin count, 256..65535; 0 = 2048 */
    int32_t dark_below;     /* a tile is enhanced only when its p99 luma is below this, 1..256 (256: every tile); 0 = 64 */
} rf_enhance_spec;

/* Host only, no GPU, no handle -- the same code the kernels run, compiled for the host: the enhancement of the rows x cols BGR frame src
 * (row pitch step) written as cols * 3 bytes per row at dst + y * dst_step (bytes beyond them are untouched).  dst may be src with the
 * same pitch.  spec may be NULL (all defaults); *tiles_enhanced (may be NULL) receives the number of flagged tiles.  A bad spec, pitch
 * or pointer: RF_ERR_INVALID_ARG. */
int rf_enhance_host(const rf_enhance_spec *spec, const uint8_t *src, int rows, int cols, int step, uint8_t *dst, int dst_step,
                    int *tiles_enhanced);

/* The two enhance kernels on their own, for n frames in device memory (any source pitch and pointer alignment; ROI views are legal;
 * steps / dst_steps may be NULL for cols * 3; a NULL / 0 x 0 frame is skipped).  d_dst[i] may be d_src[i] exactly (same pointer and
 * pitch): every LUT is finished before a pixel is written.  Any other overlap between a destination and a source or another destination of
 * the call is refused, as are a bad spec and a call with more than 262144 tiles in total (64 MB of LUTs; the LUT scratch grows on
 * demand) -- all with RF_ERR_INVALID_ARG before any state changes.  tiles_enhanced (n ints, may be NULL) receives the number of flagged
 * tiles of each frame.  Synchronous.  Multi-device handles return RF_ERR_UNSUPPORTED from this call and the next two. */
int rf_enhance_device(rf_handle h, const rf_enhance_spec *spec, const void *const *d_src, const int *rows, const int *cols,
                      const int *steps, int n, void *const *d_dst, const int *dst_steps, int *tiles_enhanced);

/* Enhancement and detection in one call, for frames resident on the engine's device (frame limits as rf_detect_batch_device).  The
 * enhance kernels run on the engine's side stream in front of the call's first detection launch and every launch of the call waits for
 * them on the device -- no host synchronisation in between.  The caller's frames are never written: the enhanced copies go to
 * d_enhanced[i] (row pitch enhanced_steps[i], NULL = cols * 3; overlap rules as rf_enhance_device, and d_enhanced[i] may not be the
 * frame itself) so that the alignment, face-batch, redaction and overlay calls can be given the pixels the detector saw; with
 * d_enhanced NULL they go to an engine-owned block.  out and counts are, to the byte, what rf_detect_batch_device returns at this
 * threshold for the enhanced frames as dense frames (the copies are dense in the engine's block; a caller's d_enhanced is read where it
 * lies, so pass dense 256-byte-aligned buffers where the last bits matter).  tiles_enhanced (n ints, may be NULL) as above: 0 means the
 * frame's copy equals the frame.  spec may be NULL. */
int rf_detect_enhanced_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                    float threshold, const rf_enhance_spec *spec, rf_face *out, int cap_per_image, int *counts,
                                    void *const *d_enhanced, const int *enhanced_steps, int *tiles_enhanced);

/* The same with frames in HOST memory (rf_detect_batch's convention): each frame is uploaded once, densely.  d_enhanced (device
 * memory) may be NULL; tiles_enhanced comes back either way. */
int rf_detect_enhanced_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                             float threshold, const rf_enhance_spec *spec, rf_face *out, int cap_per_image, int *counts,
                             void *const *d_enhanced, const int *enhanced_steps, int *tiles_enhanced);

#ifdef __cplusplus
}
#endif
#endif /* RETINAFACE_AMD_H */
