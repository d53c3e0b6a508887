// capi.cpp -- extern "C" boundary (include/retinaface_amd.h) over rf::Engine.  Exceptions never cross it.
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <list>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"
#include "weights.h"

namespace {
thread_local std::string g_create_error;
thread_local const void *g_busy_handle = nullptr;      // the handle this thread's last call was refused on (see guarded)
const char kBusyText[] = "handle in use by another thread (one handle = one caller thread at a time)";
}

struct rf_engine {
    std::unique_ptr<rf::Engine> eng;
    std::string error;
    std::atomic_flag in_call = ATOMIC_FLAG_INIT;       // set for the duration of every call that touches the engine's state
    // rf_detect_batch_pad32: one engine per padded frame size, most recently used first
    std::string model_dir, network;
    float nms = 0.4f;
    rf::EngineOptions opt;
    std::list<std::pair<std::pair<int, int>, std::unique_ptr<rf::Engine>>> pool;
    std::vector<rf_tracker_s *> trackers;              // rf_tracker_create: what rf_destroy still has to free
    std::vector<rf_dewarper_s *> dewarpers;            // rf_dewarper_create: likewise
    std::vector<rf_changer_s *> changers;              // rf_changer_create: likewise
    ~rf_engine();
};

// a changer: the handle it lives on and the engine's object (null once destroyed)
struct rf_changer_s {
    rf_engine *h;
    void *impl;
};

// a tracker: the handle it lives on and the engine's object
struct rf_tracker_s {
    rf_engine *h;
    void *impl;
};

// a dewarper: the handle it lives on, the engine's object (null once destroyed) and its number of views
struct rf_dewarper_s {
    rf_engine *h;
    void *impl;
    int views;
};

rf_engine::~rf_engine() {
    for (rf_tracker_s *t : trackers) delete t;         // the engine frees the device state with itself
    for (rf_dewarper_s *d : dewarpers) delete d;
    for (rf_changer_s *c : changers) delete c;
}

namespace {

// The boundary's contract is "one handle = one caller thread at a time" (include/retinaface_amd.h): lanes, tickets and staging buffers are
// unsynchronised by design.  A second thread entering while a call is in flight would corrupt them silently (the reference is equally
// unsafe, RetinaFace.cpp shared staging buffers -- but this library advertises a serving loop), so the entry points refuse it: the
// intruder gets RF_ERR_INVALID_ARG and rf_last_error() on ITS thread says why; the call in flight is not disturbed.
struct InCall {
    rf_engine *h;
    bool ok;
    explicit InCall(rf_engine *e) : h(e), ok(!e || !e->in_call.test_and_set(std::memory_order_acquire)) {}
    ~InCall() { if (h && ok) h->in_call.clear(std::memory_order_release); }
};

template <typename F> int guarded(rf_engine *h, F &&f) {
    InCall guard(h);
    if (!guard.ok) { g_busy_handle = h; return RF_ERR_INVALID_ARG; }
    if (h && g_busy_handle == h) g_busy_handle = nullptr;
    std::string &err = h ? h->error : g_create_error;
    try {
        return f();
    } catch (const rf::ArgError &e) { err = e.what(); return RF_ERR_INVALID_ARG;
    } catch (const rf::IoError &e) { err = e.what(); return RF_ERR_IO;
    } catch (const rf::ModelError &e) { err = e.what(); return RF_ERR_MODEL;
    } catch (const rf::HipError &e) { err = e.what(); return RF_ERR_HIP;
    } catch (const rf::Unsupported &e) { err = e.what(); return RF_ERR_UNSUPPORTED;
    } catch (const std::exception &e) { err = e.what(); return RF_ERR_INVALID_ARG; }
}

// guarded() for a call that can run into the engine's caps: f(bool *truncated) does all of the call's work and returns the status it
// would have without that flag (with h->error set where that is not RF_OK); a set flag wins over it.
template <typename F> int guarded_caps(rf_engine *h, F &&f) {
    return guarded(h, [&]() -> int {
        bool truncated = false;
        const int st = f(&truncated);
        if (truncated) { h->error = "more candidates / detections than the configured caps"; return RF_ERR_TRUNCATED; }
        return st;
    });
}

// What the four rf_*_merge_host calls share once the mapped candidates of their passes are gathered (group g = pass * max_detections
// + index): the merge, the heads emitted to the caller (at most min(cap, max_faces)), the true count, and the status.  *emitted: the
// number of heads written, for a caller that goes on with them.
int merge_host_emit(const std::vector<float> &cand, const std::vector<int> &g, float nms_threshold, bool vote, int cap, int max_faces,
                    int max_detections, bool truncated, rf_face *out, int *count, int *votes, int *src, int *emitted = nullptr) {
    const int limit = cap < max_faces ? cap : max_faces;
    std::vector<float> merged((size_t)limit * 15 + 1);
    std::vector<int> vt((size_t)limit + 1), hg((size_t)limit + 1);
    const int heads = rf::tta_merge_candidates(cand, g, nms_threshold, vote, limit, merged.data(), vt.data(), hg.data());
    *count = heads;
    const int k = heads < limit ? heads : limit;
    for (int j = 0; j < k; j++) {
        memset(&out[j], 0, sizeof(rf_face));
        memcpy(&out[j], &merged[(size_t)j * 15], 15 * sizeof(float));
        if (votes) votes[j] = vt[j];
        if (src) src[j] = hg[j] / max_detections;
    }
    if (emitted) *emitted = k;
    return truncated || heads > limit ? RF_ERR_TRUNCATED : RF_OK;
}


rf::AlignRequest align_request(int crop_size, int max_faces, void *d_crops, uint8_t *crops, double *matrices) {
    rf::AlignRequest rq;
    rq.crop = crop_size; rq.max_faces = max_faces;
    rq.d_crops = (uint8_t *)d_crops; rq.crops = crops; rq.matrices = matrices;
    return rq;
}

}  // namespace

extern "C" {

int rf_abi_version(void) { return RF_ABI_VERSION; }

int rf_create(const char *model_dir, const char *network, float nms_threshold, const rf_options *o, rf_handle *out) {
    return guarded(nullptr, [&]() -> int {
        if (!model_dir || !out) throw rf::ArgError("model_dir / out_handle is null");
        *out = nullptr;
        rf::EngineOptions eo;
        rf_options ocopy;
        if (o) {
            // ABI 1 callers pass the struct up to `coalesce`; the fields added later default to 0
            const size_t v1 = offsetof(rf_options, copy_threads);
            if (o->struct_size != sizeof(rf_options) && o->struct_size != v1) throw rf::ArgError("rf_options.struct_size mismatch");
            memset(&ocopy, 0, sizeof(ocopy));
            memcpy(&ocopy, o, o->struct_size);
            o = &ocopy;
            if (o->precision == RF_PRECISION_FP32 || o->precision == RF_PRECISION_FP16 || o->precision == RF_PRECISION_INT8)
                eo.precision = o->precision;
            else throw rf::ArgError("unknown precision");
            eo.net_h = o->net_h; eo.net_w = o->net_w;
            if (o->max_batch) eo.max_batch = o->max_batch;
            eo.device = o->device > 0 ? o->device - 1 : -1;
            if (o->max_candidates) eo.max_candidates = o->max_candidates;
            if (o->max_detections) eo.max_detections = o->max_detections;
            eo.use_graph = o->use_graph != 2;
            eo.keep_outputs = o->keep_outputs == 1;
            if (o->model_stem && *o->model_stem) eo.model_stem = o->model_stem;
            if (o->lanes) eo.lanes = o->lanes;
            if (o->coalesce) eo.coalesce = o->coalesce;
            eo.copy_threads = o->copy_threads;
            if (o->n_devices < 0 || (o->n_devices > 0 && !o->devices)) throw rf::ArgError("n_devices / devices mismatch");
            for (int i = 0; i < o->n_devices; i++) eo.devices.push_back(o->devices[i]);
            eo.plan_cache = o->plan_cache != 2;
            eo.resize_bilinear = o->oversize_resize == 2;
        }
        auto eng = rf::Engine::create(model_dir, network ? network : "net3", nms_threshold, eo);
        rf_engine *h = new rf_engine;
        h->eng = std::move(eng);
        h->model_dir = model_dir; h->network = network ? network : "net3"; h->nms = nms_threshold; h->opt = eo;
        *out = h;
        return RF_OK;
    });
}

int rf_preset_anchors(const char *network, int stride, float *out4, int cap_boxes) {
    if (!network || (stride != 32 && stride != 16 && stride != 8) || (cap_boxes > 0 && !out4)) return RF_ERR_INVALID_ARG;
    std::vector<float> ratios;
    (void)rf::network_preset(network, &ratios);
    float base[4][4] = {};
    rf::preset_base_anchors(ratios, stride == 32 ? 0 : stride == 16 ? 1 : 2, base);
    const int a = 2 * (int)ratios.size();
    for (int i = 0; i < a && i < cap_boxes; i++) memcpy(out4 + 4 * i, base[i], 4 * sizeof(float));
    return a;
}

void rf_destroy(rf_handle h) { delete h; }

const char *rf_last_error(rf_handle h) {
    if (h && g_busy_handle == h) return kBusyText;
    return h ? h->error.c_str() : g_create_error.c_str();
}

int rf_get_net_size(rf_handle h, int *net_h, int *net_w, int *max_batch) {
    if (!h) return RF_ERR_INVALID_ARG;
    if (net_h) *net_h = h->eng->net_h();
    if (net_w) *net_w = h->eng->net_w();
    if (max_batch) *max_batch = h->eng->max_batch();
    return RF_OK;
}

static int detect_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps,
                         int n, bool on_device, float thr, rf_face *out, int cap, int *counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        h->eng->detect(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr);
        return RF_OK;
    });
}

int rf_detect_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                    float threshold, rf_face *out, int cap_per_image, int *counts) {
    return detect_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts);
}

int rf_detect_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                           int n, float threshold, rf_face *out, int cap_per_image, int *counts) {
    return detect_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts);
}

namespace {
constexpr size_t kPoolEngines = 8;

rf::Engine *pool_engine(rf_engine *h, int hs, int ws) {
    const std::pair<int, int> key(hs, ws);
    for (auto it = h->pool.begin(); it != h->pool.end(); ++it)
        if (it->first == key) {
            h->pool.splice(h->pool.begin(), h->pool, it);
            return h->pool.front().second.get();
        }
    rf::EngineOptions eo = h->opt;
    eo.net_h = hs; eo.net_w = ws;
    eo.lanes = 1; eo.coalesce = 1; eo.keep_outputs = false;
    if (!eo.devices.empty()) { eo.device = eo.devices[0]; eo.devices.clear(); }     // per-size engines live on the first device
    // activations scale with the frame: keep a pooled engine's footprint near max_batch x 448^2 worth of pixels
    const long px = (long)hs * ws, budget = (long)std::max(eo.max_batch, 1) * 448 * 448;
    eo.max_batch = (int)std::max(1L, std::min((long)eo.max_batch, budget / px));
    if (h->pool.size() >= kPoolEngines) h->pool.pop_back();
    h->pool.emplace_front(key, rf::Engine::create(h->model_dir, h->network, h->nms, eo));
    return h->pool.front().second.get();
}
}  // namespace

int rf_detect_batch_pad32(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          int on_device, float threshold, rf_face *out, int cap_per_image, int *counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *truncated) -> int {
        if (n < 0 || (n > 0 && (!bgr || !rows || !cols || !counts))) throw rf::ArgError("null argument");
        std::vector<char> done(n, 0);
        for (int i = 0; i < n; i++) {
            if (done[i]) continue;
            if (!bgr[i] || rows[i] <= 0 || cols[i] <= 0) { counts[i] = 0; done[i] = 1; continue; }    // img.empty(), :945-947
            if (rows[i] > 4096 * 3072 / std::max(cols[i], 1)) throw rf::ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
            const int hs = (rows[i] + 31) / 32 * 32, ws = (cols[i] + 31) / 32 * 32;                   // :950-951
            std::vector<int> idx;
            for (int j = i; j < n; j++)
                if (!done[j] && bgr[j] && rows[j] > 0 && cols[j] > 0 && (rows[j] + 31) / 32 * 32 == hs && (cols[j] + 31) / 32 * 32 == ws)
                    idx.push_back(j);
            rf::Engine &eng = *pool_engine(h, hs, ws);
            const int m = (int)idx.size();
            std::vector<const uint8_t *> f(m);
            std::vector<int> r(m), c(m), st(m), cnt(m);
            for (int k = 0; k < m; k++) { f[k] = bgr[idx[k]]; r[k] = rows[idx[k]]; c[k] = cols[idx[k]]; st[k] = steps ? steps[idx[k]] : cols[idx[k]] * 3; }
            std::vector<rf_face> tmp((size_t)m * std::max(cap_per_image, 0));
            bool cut = false;
            eng.detect(f.data(), r.data(), c.data(), st.data(), m, on_device != 0, threshold, out ? tmp.data() : nullptr, cap_per_image,
                       cnt.data(), &cut);
            *truncated = *truncated || cut;
            for (int k = 0; k < m; k++) {
                counts[idx[k]] = cnt[k];
                if (out)
                    memcpy(out + (size_t)idx[k] * cap_per_image, tmp.data() + (size_t)k * cap_per_image,
                           sizeof(rf_face) * (size_t)std::min(cnt[k], cap_per_image));
                done[idx[k]] = 1;
            }
        }
        return RF_OK;
    });
}

float rf_frame_scale(rf_handle h, int rows, int cols) {
    if (!h || rows <= 0 || cols <= 0) return 1.f;
    return rf::frame_scale(rows, cols, h->eng->net_h(), h->eng->net_w());     // RetinaFace.cpp:585-589
}

int rf_align_matrix(const rf_face *face, float coord_scale, int crop_size, double fwd[6]) {
    if (!face || !fwd || crop_size < rf::kAlignMinCrop || crop_size > rf::kAlignMaxCrop) return RF_ERR_INVALID_ARG;
    rf::AlignXform t;
    rf::align_estimate(face->px, face->py, coord_scale, crop_size, &t);
    memcpy(fwd, t.fwd, sizeof(t.fwd));
    return t.valid;
}

namespace {
int detect_align_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                        bool on_device, float thr, rf_face *out, int cap, int *counts, const rf::AlignRequest &rq) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::StageCall sc;
        rf::StageResult res;
        sc.align = &rq;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        return RF_OK;
    });
}
}  // namespace

int rf_align_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                          const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, int crop_size,
                          int max_faces, void *d_crops, uint8_t *crops, double *matrices) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        h->eng->align(d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale,
                      align_request(crop_size, max_faces, d_crops, crops, matrices));
        return RF_OK;
    });
}

int rf_detect_align_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, int crop_size, int max_faces,
                                 void *d_crops, uint8_t *crops, double *matrices) {
    return detect_align_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts,
                               align_request(crop_size, max_faces, d_crops, crops, matrices));
}

int rf_detect_align_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, rf_face *out, int cap_per_image, int *counts, int crop_size, int max_faces,
                          void *d_crops, uint8_t *crops, double *matrices) {
    return detect_align_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts,
                               align_request(crop_size, max_faces, d_crops, crops, matrices));
}

namespace {
// a caller's spec, checked and with its defaults applied, and the buffers of the call
void face_batch_request(const rf_face_batch_spec *spec, int default_max_faces, void *d_tensor, void *tensor, double *matrices,
                        int *offsets, rf::FaceBatchRequest *rq) {
    if (const char *bad = rf::face_batch_resolve(spec, default_max_faces, &rq->spec)) throw rf::ArgError(bad);
    rq->d_tensor = (uint8_t *)d_tensor; rq->tensor = (uint8_t *)tensor; rq->matrices = matrices; rq->offsets = offsets;
}

const char kFaceOverflow[] = "more packed faces than the face batch's capacity";

int detect_face_batch_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                             bool on_device, float thr, rf_face *out, int cap, int *counts, const rf_face_batch_spec *spec,
                             void *d_tensor, void *tensor, double *matrices, int *offsets) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::FaceBatchRequest rq;
        face_batch_request(spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.face_batch = &rq;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.overflow) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

long rf_face_batch_plan(const rf_face_batch_spec *spec, const int *counts, int n, int *offsets, size_t *bytes_per_face) {
    rf::FaceBatchSpec sp;
    if (rf::face_batch_resolve(spec, 256, &sp) || n < 0 || (n > 0 && !counts)) return RF_ERR_INVALID_ARG;
    long total = 0;
    for (int i = 0; i < n; i++) {                       // checked before anything is written
        if (counts[i] < 0) return RF_ERR_INVALID_ARG;
        total += std::min(counts[i], sp.max_faces);
    }
    if (total > 0x7fffffffL) return RF_ERR_INVALID_ARG;
    rf::face_batch_offsets(counts, n, sp.max_faces, offsets);
    if (bytes_per_face) *bytes_per_face = sp.bytes_per_face();
    return total;
}

int rf_face_value_table(const rf_face_batch_spec *spec, int channel, void *out256) {
    rf::FaceBatchSpec sp;
    rf_face_batch_spec any;
    if (!spec || !out256 || channel < 0 || channel > 2) return RF_ERR_INVALID_ARG;
    if (spec->struct_size != sizeof(any) && spec->struct_size != rf::kFaceSpecSizeV1) return RF_ERR_INVALID_ARG;
    memset(&any, 0, sizeof(any));
    memcpy(&any, spec, spec->struct_size);                       // only the bytes the caller's struct has
    if (any.capacity == 0) any.capacity = 1;                     // the table does not depend on it
    if (rf::face_batch_resolve(&any, 256, &sp)) return RF_ERR_INVALID_ARG;
    const float m = sp.mean[channel], k = sp.scale[channel];
    for (unsigned q = 0; q < 256; q++) {
        if (sp.format == RF_FACES_U8_HWC) ((uint8_t *)out256)[q] = rf::face_value<uint8_t>(q, m, k);
        else if (sp.format == RF_FACES_F16_CHW) ((_Float16 *)out256)[q] = rf::face_value<_Float16>(q, m, k);
        else ((float *)out256)[q] = rf::face_value<float>(q, m, k);
    }
    return RF_OK;
}

int rf_face_aa_factor(const rf_face *face, float coord_scale, int crop_size, int aa_max) {
    if (!face) return RF_ERR_INVALID_ARG;
    const int S = crop_size ? crop_size : rf::kFaceBatchDefaultCrop, kmax = rf::face_aa_max_resolve(aa_max);
    if (S < rf::kAlignMinCrop || S > rf::kAlignMaxCrop || !kmax) return RF_ERR_INVALID_ARG;
    rf::AlignXform t;
    rf::align_estimate(face->px, face->py, coord_scale, S, &t);
    return rf::align_aa_factor(t, kmax);
}

int rf_detect_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                void *d_tensor, void *tensor, double *matrices, int *offsets) {
    return detect_face_batch_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts,
                                    spec, d_tensor, tensor, matrices, offsets);
}

int rf_detect_face_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                         float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                         void *d_tensor, void *tensor, double *matrices, int *offsets) {
    return detect_face_batch_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, spec, d_tensor, tensor,
                                    matrices, offsets);
}

int rf_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                         const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale,
                         const rf_face_batch_spec *spec, void *d_tensor, void *tensor, double *matrices, int *offsets) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::FaceBatchRequest rq;
        face_batch_request(spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &rq);
        bool over = false;
        h->eng->face_batch(d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, rq, &over);
        if (over) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- face quality and gated face batches (face_quality.h)
namespace {
// the gate half of a gated request; a bad gate is refused here, before the engine is touched
void face_gate_request(const rf_face_gate *gate, rf_face_quality *quality, rf::FaceBatchRequest *rq) {
    rq->gated = true;
    rq->has_gate = gate != nullptr;
    if (gate)
        if (const char *bad = rf::face_gate_resolve(gate, &rq->gate)) throw rf::ArgError(bad);
    rq->quality = quality;
}

int detect_face_batch_gated_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                                   bool on_device, float thr, rf_face *out, int cap, int *counts, const rf_face_batch_spec *spec,
                                   void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                                   rf_face_quality *quality) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::FaceBatchRequest rq;
        face_batch_request(spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &rq);
        face_gate_request(gate, quality, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.face_batch = &rq;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.overflow) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_face_pose(const rf_face *face, float coord_scale, int crop_size, rf_face_quality *q) {
    if (!face || !q) return RF_ERR_INVALID_ARG;
    const int S = crop_size ? crop_size : rf::kFaceBatchDefaultCrop;
    if (S < rf::kAlignMinCrop || S > rf::kAlignMaxCrop) return RF_ERR_INVALID_ARG;
    rf::AlignXform t;
    const int ok = rf::align_estimate(face->px, face->py, coord_scale, S, &t);
    memset(q, 0, sizeof(*q));
    rf::face_pose(face->px, face->py, coord_scale, t, q);
    q->flags = ok ? 0 : RF_GATE_INVALID;
    return RF_OK;
}

int rf_face_gate_eval(const rf_face_gate *gate, const rf_face_quality *q, int crop_size) {
    if (!q) return RF_ERR_INVALID_ARG;
    const int S = crop_size ? crop_size : rf::kFaceBatchDefaultCrop;
    if (S < rf::kAlignMinCrop || S > rf::kAlignMaxCrop) return RF_ERR_INVALID_ARG;
    if (!gate) return 0;
    rf::FaceGate g;
    if (rf::face_gate_resolve(gate, &g)) return RF_ERR_INVALID_ARG;
    return rf::face_gate_eval(g, *q, (q->flags & RF_GATE_INVALID) != 0, S);
}

int rf_face_quality_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                           const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, int crop_size,
                           int max_faces, const rf_face_gate *gate, rf_face_quality *quality) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (!quality) throw rf::ArgError("quality is null");
        rf::FaceBatchRequest rq;                       // no tensor, no matrices: the records alone
        rq.spec.crop = crop_size ? crop_size : rf::kFaceBatchDefaultCrop;
        rq.spec.max_faces = max_faces;
        rq.spec.capacity = 1;
        face_gate_request(gate, quality, &rq);
        bool over = false;
        h->eng->face_batch(d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, rq, &over);
        return RF_OK;
    });
}

int rf_face_batch_gated_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale,
                               const rf_face_batch_spec *spec, void *d_tensor, void *tensor, double *matrices, int *offsets,
                               const rf_face_gate *gate, rf_face_quality *quality) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::FaceBatchRequest rq;
        face_batch_request(spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &rq);
        face_gate_request(gate, quality, &rq);
        bool over = false;
        h->eng->face_batch(d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, rq, &over);
        if (over) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int rf_detect_face_batch_gated_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                      void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                                      rf_face_quality *quality) {
    return detect_face_batch_gated_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image,
                                          counts, spec, d_tensor, tensor, matrices, offsets, gate, quality);
}

int rf_detect_face_batch_gated(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                               void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                               rf_face_quality *quality) {
    return detect_face_batch_gated_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, spec, d_tensor,
                                          tensor, matrices, offsets, gate, quality);
}

// ---- tiled detection (tile.h)
int rf_tile_plan(const rf_tile_spec *spec, int rows, int cols, int net_h, int net_w, int *xywh, int cap_tiles) {
    rf::TileSpec sp;
    if (rf::tile_spec_resolve(spec, net_h, net_w, 256, &sp) || rows < 0 || cols < 0 || cap_tiles < 0) return RF_ERR_INVALID_ARG;
    if (cols > 0 && rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    int nx = 0, ny = 0, full = 0;
    const int passes = rf::tile_plan_shape(sp, rows, cols, net_h, net_w, &nx, &ny, &full);
    if (passes < 0) return RF_ERR_INVALID_ARG;
    for (int t = 0; xywh && t < passes && t < cap_tiles; t++) {
        const rf::TileEntry e = rf::tile_plan_entry(rows, cols, net_h, net_w, nx, ny, t, 0);
        xywh[4 * t] = e.x0; xywh[4 * t + 1] = e.y0; xywh[4 * t + 2] = e.tw; xywh[4 * t + 3] = e.th;
    }
    return passes;
}

int rf_tile_map_face(const rf_tile_spec *spec, int rows, int cols, int net_h, int net_w, int t, const rf_face *in, rf_face *out) {
    rf::TileSpec sp;
    if (!in || !out || rf::tile_spec_resolve(spec, net_h, net_w, 256, &sp) || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    if (cols > 0 && rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    int nx = 0, ny = 0, full = 0;
    const int passes = rf::tile_plan_shape(sp, rows, cols, net_h, net_w, &nx, &ny, &full);
    if (passes < 0 || t < 0 || t >= passes) return RF_ERR_INVALID_ARG;
    const rf::TileEntry e = rf::tile_plan_entry(rows, cols, net_h, net_w, nx, ny, t, 0);
    float f[15];
    memcpy(f, in, sizeof(f));
    if (!rf::tile_map_face(e, sp.edge, f, f)) return 0;
    memcpy(out, f, sizeof(f));
    return 1;
}

namespace {
// a caller's tile spec, checked against the handle's net size and with its defaults applied; refused before the engine is touched
void tile_request(rf_handle h, const rf_tile_spec *spec, int *src_tile, rf::TileRequest *rq) {
    if (const char *bad = rf::tile_spec_resolve(spec, h->eng->net_h(), h->eng->net_w(), h->eng->default_max_faces(), &rq->spec))
        throw rf::ArgError(bad);
    rq->src_tile = src_tile;
}

int detect_tiled_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                        float thr, const rf_tile_spec *spec, rf_face *out, int cap, int *counts, int *src_tile) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::TileRequest rq;
        tile_request(h, spec, src_tile, &rq);
        bool over = false;
        h->eng->detect_tiled(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq, &over);
        return RF_OK;
    });
}
}  // namespace

int rf_detect_tiled_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, const rf_tile_spec *spec, rf_face *out, int cap_per_image, int *counts, int *src_tile) {
    return detect_tiled_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts,
                               src_tile);
}

int rf_detect_tiled_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, const rf_tile_spec *spec, rf_face *out, int cap_per_image, int *counts, int *src_tile) {
    return detect_tiled_common(h, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, src_tile);
}

int rf_tile_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_tile_spec *spec, const rf_face *faces,
                         const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *src_tile) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::TileRequest rq;
        tile_request(h, spec, src_tile, &rq);
        h->eng->tile_merge(rows, cols, n, rq, faces, pass_counts, out, cap_per_image, counts, tr);
        return RF_OK;
    });
}

int rf_detect_tiled_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, const rf_tile_spec *tile_spec, rf_face *out, int cap_per_image, int *counts,
                                      int *src_tile, const rf_face_batch_spec *fb_spec, void *d_tensor, void *tensor, double *matrices,
                                      int *offsets, const rf_face_gate *gate, rf_face_quality *quality) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::TileRequest rq;
        tile_request(h, tile_spec, src_tile, &rq);
        rf::FaceBatchRequest fb;
        face_batch_request(fb_spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &fb);
        if (gate || quality) face_gate_request(gate, quality, &fb);
        rq.fb = &fb;
        bool over = false;
        h->eng->detect_tiled((const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tr, rq, &over);
        if (over) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- face tracks (track.h)
int rf_track_step(const rf_track_spec *spec, rf_track *table, int64_t *frames, int64_t *next_id, const rf_face *faces, int count,
                  float coord_scale, const rf_face_quality *quality, int max_faces, rf_track_tag *tags, rf_track *ended, int cap_ended,
                  int *ended_count) {
    rf::TrackSpec sp;
    if (rf::track_spec_resolve(spec, &sp)) return RF_ERR_INVALID_ARG;
    if (!table || !frames || !next_id || !ended_count || count < 0 || max_faces < 1 || cap_ended < 0) return RF_ERR_INVALID_ARG;
    if (count > 0 && (!faces || !tags)) return RF_ERR_INVALID_ARG;
    if (cap_ended > 0 && !ended) return RF_ERR_INVALID_ARG;
    const int m = std::min(std::min(count, max_faces), rf::kTrackMaxFaces);
    const int st = rf::track_step(sp, table, frames, next_id, (const float *)faces, (int)(sizeof(rf_face) / sizeof(float)), m, coord_scale,
                                  quality, tags, ended, cap_ended, ended_count);
    for (int k = m; k < count; k++) tags[k] = rf::track_tag_untracked(0);
    return st ? RF_ERR_TRUNCATED : RF_OK;
}

namespace {
const char kTrackCut[] = "a track table is full or an ended list was cut";

void track_request(rf_handle h, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended,
                   int *ended_counts, rf::TrackRequest *rq) {
    if (!tracker || tracker->h != h) throw rf::ArgError("not a tracker of this handle");
    rq->tracker = tracker->impl;
    rq->stream_of_image = stream_of_image;
    rq->tags = tags; rq->ended = ended; rq->cap_ended = cap_ended; rq->ended_counts = ended_counts;
}

int detect_track_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                        float thr, rf_face *out, int cap, int *counts, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                        rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.track = &rq;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_tracker_create(rf_handle h, const rf_track_spec *spec, int n_streams, rf_tracker *out_tracker) {
    rf::TrackSpec sp;
    if (out_tracker) *out_tracker = nullptr;
    const char *bad = rf::track_spec_resolve(spec, &sp);               // spec and range first: refused without a GPU
    if (!bad && (n_streams < 1 || n_streams > rf::kTrackMaxStreams)) bad = "n_streams must be in [1, 1024]";
    if (!h || !out_tracker) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (bad) throw rf::ArgError(bad);
        void *impl = h->eng->tracker_create(sp, n_streams);
        rf_tracker_s *t = new rf_tracker_s{h, impl};
        h->trackers.push_back(t);
        *out_tracker = t;
        return RF_OK;
    });
}

void rf_tracker_destroy(rf_tracker tracker) {
    if (!tracker) return;
    rf_engine *h = tracker->h;
    (void)guarded(h, [&]() -> int {
        h->eng->tracker_destroy(tracker->impl);
        h->trackers.erase(std::remove(h->trackers.begin(), h->trackers.end(), tracker), h->trackers.end());
        delete tracker;
        return RF_OK;
    });
}

int rf_tracker_reset(rf_tracker tracker, int stream) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { tracker->h->eng->tracker_reset(tracker->impl, stream); return RF_OK; });
}

int rf_tracker_read(rf_tracker tracker, int stream, rf_track *table, int cap, int64_t *frames, int64_t *next_id) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { return tracker->h->eng->tracker_read(tracker->impl, stream, table, cap, frames, next_id, false); });
}

int rf_tracker_flush(rf_tracker tracker, int stream, rf_track *ended, int cap, int64_t *frames, int64_t *next_id) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { return tracker->h->eng->tracker_read(tracker->impl, stream, ended, cap, frames, next_id, true); });
}

int rf_track_update_device(rf_handle h, rf_tracker tracker, const int *stream_of_image, int n, const rf_face *faces, int cap_per_image,
                           const int *counts, const float *coord_scale, const rf_face_quality *quality, int max_faces,
                           rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        bool cut = false;
        h->eng->track_update(rq, n, faces, cap_per_image, counts, coord_scale, quality, max_faces ? max_faces : h->eng->default_max_faces(), &cut);
        if (cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int rf_track_last_launch_ms(rf_handle h, float *ms) {
    if (!h || !ms) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        const float v = h->eng->track_last_launch_ms();
        if (v < 0.f) throw rf::ArgError("no rf_track_update_device call has been timed on this handle");
        *ms = v;
        return RF_OK;
    });
}

int rf_detect_track_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                 const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tracker,
                               stream_of_image, tags, ended, cap_ended, ended_counts);
}

int rf_detect_track_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                          const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, tracker, stream_of_image, tags,
                               ended, cap_ended, ended_counts);
}

int rf_detect_track_face_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, rf_face *out, int cap_per_image, int *counts, const rf_face_batch_spec *spec,
                                      void *d_tensor, void *tensor, double *matrices, int *offsets, const rf_face_gate *gate,
                                      rf_face_quality *quality, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                                      rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::FaceBatchRequest fb;
        face_batch_request(spec, h->eng->default_max_faces(), d_tensor, tensor, matrices, offsets, &fb);
        if (gate || quality) face_gate_request(gate, quality, &fb);
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.face_batch = &fb; sc.track = &rq;
        h->eng->detect_staged((const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tr, sc, &res);
        if (res.overflow) { h->error = kFaceOverflow; return RF_ERR_TRUNCATED; }
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- best-shot gallery (shot.h)
int rf_shot_resolve(int max_tracks, int n, const rf_track_tag *tags, int cap_per_image, const int *counts, const rf_track *ended,
                    int cap_ended, const int *ended_counts, int64_t first_frame, const rf_face *faces, const float *coord_scale,
                    int crop_size, rf_shot *records, int32_t *source, int32_t *owner) {
    if (max_tracks < 1 || max_tracks > rf::kTrackMaxTracks || n < 0 || cap_per_image < 1 || cap_ended < 0 || first_frame < 0 || !records)
        return RF_ERR_INVALID_ARG;
    if (n > 0 && (!tags || !counts || !ended_counts)) return RF_ERR_INVALID_ARG;
    if (cap_ended > 0 && n > 0 && !ended) return RF_ERR_INVALID_ARG;
    if (faces && (crop_size < rf::kAlignMinCrop || crop_size > rf::kAlignMaxCrop)) return RF_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (counts[i] < 0 || ended_counts[i] < 0) return RF_ERR_INVALID_ARG;
    return rf::shot_resolve(max_tracks, n, tags, cap_per_image, counts, ended, cap_ended, ended_counts, first_frame, faces, coord_scale,
                            crop_size, records, source, owner);
}

namespace {
void shot_request(const rf_face_gate *gate, rf_face_quality *quality, void *d_shots, void *shots, rf_shot *shot_info, rf::ShotRequest *sq) {
    sq->d_shots = (uint8_t *)d_shots; sq->shots = (uint8_t *)shots; sq->info = shot_info;
    sq->gated = gate || quality;
    sq->has_gate = gate != nullptr;
    if (gate)
        if (const char *bad = rf::face_gate_resolve(gate, &sq->gate)) throw rf::ArgError(bad);
    sq->quality = quality;
}

int detect_track_shots_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                              float thr, rf_face *out, int cap, int *counts, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                              rf_track *ended, int cap_ended, int *ended_counts, const rf_face_gate *gate, rf_face_quality *quality,
                              void *d_shots, void *shots, rf_shot *shot_info) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        rf::ShotRequest sq;
        shot_request(gate, quality, d_shots, shots, shot_info, &sq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.track = &rq; sc.shots = &sq;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_tracker_enable_shots(rf_tracker tracker, const rf_face_batch_spec *spec) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    rf_engine *h = tracker->h;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::FaceBatchSpec sp;
        if (const char *bad = rf::face_batch_resolve(spec, h->eng->default_max_faces(), &sp)) throw rf::ArgError(bad);
        h->eng->tracker_enable_shots(tracker->impl, sp);
        return RF_OK;
    });
}

// ---- motion-predicted tracks (motion.h)
int rf_track_step_motion(const rf_track_spec *spec, const rf_motion_spec *mspec, rf_track *table, rf_track_motion *motion, int64_t *frames,
                         int64_t *next_id, const rf_face *faces, int count, float coord_scale, const rf_face_quality *quality,
                         int max_faces, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_count) {
    rf::TrackSpec sp;
    rf::MotionSpec ms;
    if (rf::track_spec_resolve(spec, &sp) || rf::motion_spec_resolve(mspec, &ms)) return RF_ERR_INVALID_ARG;
    if (!table || !motion || !frames || !next_id || !ended_count || count < 0 || max_faces < 1 || cap_ended < 0) return RF_ERR_INVALID_ARG;
    if (count > 0 && (!faces || !tags)) return RF_ERR_INVALID_ARG;
    if (cap_ended > 0 && !ended) return RF_ERR_INVALID_ARG;
    const int m = std::min(std::min(count, max_faces), rf::kTrackMaxFaces);
    const int st = rf::track_step_motion(sp, ms, table, motion, frames, next_id, (const float *)faces, (int)(sizeof(rf_face) / sizeof(float)), m,
                                         coord_scale, quality, tags, ended, cap_ended, ended_count);
    for (int k = m; k < count; k++) tags[k] = rf::track_tag_untracked(0);
    return st ? RF_ERR_TRUNCATED : RF_OK;
}

int rf_track_predict(const rf_motion_spec *mspec, const rf_track *track, const rf_track_motion *motion, int ahead, rf_face *out) {
    rf::MotionSpec ms;
    if (rf::motion_spec_resolve(mspec, &ms)) return RF_ERR_INVALID_ARG;
    if (!track || !motion || !out || (ahead != 0 && ahead != 1) || track->id == 0 || track->missed < 0) return RF_ERR_INVALID_ARG;
    rf_face f;
    rf::motion_predict_face(&track->last, motion, rf::motion_frames_ahead(track->missed, ahead, ms.horizon), &f);
    *out = f;
    return RF_OK;
}

int rf_tracker_enable_motion(rf_tracker tracker, const rf_motion_spec *mspec) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    rf_engine *h = tracker->h;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::MotionSpec ms;
        if (const char *bad = rf::motion_spec_resolve(mspec, &ms)) throw rf::ArgError(bad);
        h->eng->tracker_enable_motion(tracker->impl, ms);
        return RF_OK;
    });
}

int rf_tracker_read_motion(rf_tracker tracker, int stream, rf_track_motion *out, int cap) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { return tracker->h->eng->tracker_read_motion(tracker->impl, stream, out, cap); });
}

// ---- followed tracks (follow.h)
namespace {
// a host frame as follow.h takes it; false: a frame that cannot be read (a NULL / 0 x 0 frame is legal: it has no pixels)
bool follow_frame_arg(const uint8_t *bgr, int rows, int cols, int step, rf::FollowFrame *fd) {
    if (rows < 0 || cols < 0) return false;
    if (!bgr || rows == 0 || cols == 0) { *fd = rf::FollowFrame{nullptr, 0, 0, 0}; return true; }
    if (rows > 4096 * 3072 / cols || step < cols * 3) return false;
    *fd = rf::FollowFrame{bgr, rows, cols, step};
    return true;
}
}  // namespace

int rf_follow_geometry(const float box[4], int32_t out[3]) {
    if (!box || !out) return RF_ERR_INVALID_ARG;
    const rf::FollowGeom g = rf::follow_geometry(box);
    out[0] = g.valid ? g.q : 0; out[1] = g.valid ? g.ox : 0; out[2] = g.valid ? g.oy : 0;
    return g.valid;
}

int rf_follow_template(const uint8_t *bgr, int rows, int cols, int step, int q, int ox, int oy, uint8_t *tpl) {
    rf::FollowFrame fd;
    if (!tpl || !follow_frame_arg(bgr, rows, cols, step, &fd) || rf::follow_frame_empty(fd) || q < 1 || q > 385) return RF_ERR_INVALID_ARG;
    if (ox < -(1 << 20) || ox > (1 << 20) || oy < -(1 << 20) || oy > (1 << 20)) return RF_ERR_INVALID_ARG;
    rf::follow_template(fd, q, ox, oy, tpl);
    return RF_OK;
}

int rf_follow_search(const uint8_t *bgr, int rows, int cols, int step, const uint8_t *tpl, int q, int ox, int oy, int radius, int32_t out[4]) {
    rf::FollowFrame fd;
    if (!tpl || !out || !follow_frame_arg(bgr, rows, cols, step, &fd) || rf::follow_frame_empty(fd) || q < 1 || q > 385) return RF_ERR_INVALID_ARG;
    if (radius < 1 || radius > rf::kFollowMaxRadius) return RF_ERR_INVALID_ARG;
    if (ox < -(1 << 20) || ox > (1 << 20) || oy < -(1 << 20) || oy > (1 << 20)) return RF_ERR_INVALID_ARG;
    const rf::FollowResult r = rf::follow_search(fd, tpl, q, ox, oy, radius);
    out[0] = r.state; out[1] = r.sad; out[2] = r.du; out[3] = r.dv;
    return RF_OK;
}

int rf_track_step_follow_key(const rf_track_spec *spec, rf_track *table, rf_track_follow *records, uint8_t *templates, int64_t *frames,
                             int64_t *next_id, const uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, int count,
                             float coord_scale, const rf_face_quality *quality, int max_faces, rf_track_tag *tags, rf_track *ended,
                             int cap_ended, int *ended_count) {
    rf::TrackSpec sp;
    rf::FollowFrame fd;
    if (rf::track_spec_resolve(spec, &sp) || !follow_frame_arg(bgr, rows, cols, step, &fd)) return RF_ERR_INVALID_ARG;
    if (!table || !records || !templates || !frames || !next_id || !ended_count || count < 0 || max_faces < 1 || cap_ended < 0) return RF_ERR_INVALID_ARG;
    if (count > 0 && (!faces || !tags)) return RF_ERR_INVALID_ARG;
    if (cap_ended > 0 && !ended) return RF_ERR_INVALID_ARG;
    if (rf::follow_frame_empty(fd)) count = 0;                               // a frame without pixels has no faces, as on the device
    const int m = std::min(std::min(count, max_faces), rf::kTrackMaxFaces);
    const int st = rf::track_step_follow_key(sp, table, records, templates, frames, next_id, fd, (const float *)faces,
                                             (int)(sizeof(rf_face) / sizeof(float)), m, coord_scale, quality, tags, ended, cap_ended, ended_count);
    for (int k = m; k < count; k++) tags[k] = rf::track_tag_untracked(0);
    return st ? RF_ERR_TRUNCATED : RF_OK;
}

int rf_track_step_follow(const rf_track_spec *spec, const rf_follow_spec *fspec, rf_track *table, rf_track_follow *records,
                         const uint8_t *templates, int64_t *frames, const uint8_t *bgr, int rows, int cols, int step, rf_face *out,
                         rf_track_tag *tags, int cap, int *count, rf_track *ended, int cap_ended, int *ended_count) {
    rf::TrackSpec sp;
    rf::FollowSpec fs;
    rf::FollowFrame fd;
    if (rf::track_spec_resolve(spec, &sp) || rf::follow_spec_resolve(fspec, &fs) || !follow_frame_arg(bgr, rows, cols, step, &fd)) return RF_ERR_INVALID_ARG;
    if (!table || !records || !templates || !frames || !count || !ended_count || cap < 0 || cap_ended < 0) return RF_ERR_INVALID_ARG;
    if (cap > 0 && (!out || !tags)) return RF_ERR_INVALID_ARG;
    if (cap_ended > 0 && !ended) return RF_ERR_INVALID_ARG;
    for (int s = 0; s < sp.max_tracks; s++)                                  // a record the steps did not write is refused, not searched
        if (records[s].valid && (records[s].q < 1 || records[s].q > 385 || records[s].ox < -(1 << 20) || records[s].ox > (1 << 20) ||
                                 records[s].oy < -(1 << 20) || records[s].oy > (1 << 20)))
            return RF_ERR_INVALID_ARG;
    const int st = rf::track_step_follow(sp, fs, table, records, templates, frames, fd, out, tags, cap, count, ended, cap_ended, ended_count);
    return st ? RF_ERR_TRUNCATED : RF_OK;
}

int rf_tracker_enable_follow(rf_tracker tracker, const rf_follow_spec *spec) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    rf_engine *h = tracker->h;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::FollowSpec fs;
        if (const char *bad = rf::follow_spec_resolve(spec, &fs)) throw rf::ArgError(bad);
        h->eng->tracker_enable_follow(tracker->impl, fs);
        return RF_OK;
    });
}

int rf_tracker_read_follow(rf_tracker tracker, int stream, rf_track_follow *records, uint8_t *templates, int cap) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { return tracker->h->eng->tracker_read_follow(tracker->impl, stream, records, templates, cap); });
}

int rf_track_follow_update_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                                  int n, const int *stream_of_image, const rf_face *faces, int cap_per_image, const int *counts,
                                  const float *coord_scale, const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended,
                                  int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        bool cut = false;
        h->eng->track_follow_update(rq, d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, quality, &cut);
        if (cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

namespace {
int detect_track_follow_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                               float thr, rf_face *out, int cap, int *counts, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                               rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.track = &rq; sc.follow = true;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int track_follow_common(rf_handle h, rf_tracker tracker, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                        bool on_device, const int *stream_of_image, rf_face *out, int cap_per_image, int *counts, rf_track_tag *tags,
                        rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        bool cut = false;
        h->eng->track_follow(rq, frames, rows, cols, steps, n, on_device, out, cap_per_image, counts, &cut);
        if (cut) { h->error = "a followed list or an ended list was cut"; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_detect_track_follow_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                        float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                        const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_follow_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tracker,
                                      stream_of_image, tags, ended, cap_ended, ended_counts);
}

int rf_detect_track_follow_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                                 float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                 const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_follow_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, tracker, stream_of_image, tags,
                                      ended, cap_ended, ended_counts);
}

int rf_track_follow_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                           const int *stream_of_image, rf_face *out, int cap_per_image, int *counts, rf_track_tag *tags, rf_track *ended,
                           int cap_ended, int *ended_counts) {
    return track_follow_common(h, tracker, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, stream_of_image, out, cap_per_image, counts,
                               tags, ended, cap_ended, ended_counts);
}

int rf_track_follow_batch(rf_handle h, rf_tracker tracker, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                          const int *stream_of_image, rf_face *out, int cap_per_image, int *counts, rf_track_tag *tags, rf_track *ended,
                          int cap_ended, int *ended_counts) {
    return track_follow_common(h, tracker, bgr, rows, cols, steps, n, false, stream_of_image, out, cap_per_image, counts, tags, ended,
                               cap_ended, ended_counts);
}

int rf_follow_last_launch_ms(rf_handle h, float *ms) {
    if (!h || !ms) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        const float v = h->eng->follow_last_launch_ms();
        if (v < 0.f) throw rf::ArgError("no rf_track_follow_device call has been timed on this handle");
        *ms = v;
        return RF_OK;
    });
}

int rf_tracker_read_shots(rf_tracker tracker, int stream, void *shots, rf_shot *shot_info, int cap) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int { return tracker->h->eng->tracker_read_shots(tracker->impl, stream, (uint8_t *)shots, shot_info, cap); });
}

int rf_tracker_flush_shots(rf_tracker tracker, int stream, rf_track *ended, int cap, int64_t *frames, int64_t *next_id, void *shots,
                           rf_shot *shot_info) {
    if (!tracker) return RF_ERR_INVALID_ARG;
    return guarded(tracker->h, [&]() -> int {
        return tracker->h->eng->tracker_flush_shots(tracker->impl, stream, ended, cap, frames, next_id, (uint8_t *)shots, shot_info);
    });
}

int rf_track_shots_device(rf_handle h, rf_tracker tracker, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                          int n, const int *stream_of_image, const rf_face *faces, int cap_per_image, const int *counts,
                          const float *coord_scale, const rf_face_quality *quality, rf_track_tag *tags, rf_track *ended, int cap_ended,
                          int *ended_counts, void *d_shots, void *shots, rf_shot *shot_info) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("face tracks are not available on a multi-device handle");
        rf::TrackRequest rq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &rq);
        rf::ShotRequest sq;
        shot_request(nullptr, nullptr, d_shots, shots, shot_info, &sq);
        bool cut = false;
        h->eng->track_shots(rq, sq, d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, quality, &cut);
        if (cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int rf_shot_last_launch_ms(rf_handle h, float *ms) {
    if (!h || !ms) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        const float v = h->eng->shot_last_launch_ms();
        if (v < 0.f) throw rf::ArgError("no rf_track_shots_device call has been timed on this handle");
        *ms = v;
        return RF_OK;
    });
}

int rf_detect_track_shots_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                       float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                       const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                       const rf_face_gate *gate, rf_face_quality *quality, void *d_shots, void *shots, rf_shot *shot_info) {
    return detect_track_shots_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tracker,
                                     stream_of_image, tags, ended, cap_ended, ended_counts, gate, quality, d_shots, shots, shot_info);
}

int rf_detect_track_shots_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                                float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                const rf_face_gate *gate, rf_face_quality *quality, void *d_shots, void *shots, rf_shot *shot_info) {
    return detect_track_shots_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, tracker, stream_of_image, tags,
                                     ended, cap_ended, ended_counts, gate, quality, d_shots, shots, shot_info);
}

// ---- face redaction (redact.h)
int rf_redact_region(const rf_redact_spec *spec, const rf_face *face, float coord_scale, int rows, int cols, int out[9]) {
    rf::RedactSpec sp;
    if (rf::redact_spec_resolve(spec, 256, &sp) || !face || !out || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    const rf::RedactRegion r = rf::redact_region_make(&face->x1, coord_scale, sp.margin, sp.cells, rows, cols);
    const int v[9] = {r.ux0, r.uy0, r.ux1, r.uy1, r.cx0, r.cy0, r.cx1, r.cy1, r.c};
    memcpy(out, v, sizeof(v));
    return r.valid;
}

int rf_redact_host(const rf_redact_spec *spec, uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, int count,
                   float coord_scale, int32_t *pixels) {
    rf::RedactSpec sp;
    if (rf::redact_spec_resolve(spec, 256, &sp) || count < 0 || (count > 0 && !faces) || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    const bool empty = !bgr || rows == 0 || cols == 0;
    if (!empty && (step < cols * 3 || rows > 4096 * 3072 / cols)) return RF_ERR_INVALID_ARG;
    const int m = empty ? 0 : std::min(count, sp.max_regions);
    std::vector<rf::RedactRegion> regions((size_t)m);
    for (int k = 0; k < m; k++) regions[k] = rf::redact_region_make(&faces[k].x1, coord_scale, sp.margin, sp.cells, rows, cols);
    if (empty) { if (pixels) for (int k = 0; k < std::min(count, sp.max_regions); k++) pixels[k] = 0; }
    else rf::redact_host_frame(sp, bgr, rows, cols, (size_t)step, regions.data(), m, pixels);
    return count > sp.max_regions ? RF_ERR_TRUNCATED : RF_OK;
}

namespace {
const char kRedactCut[] = "a region list was cut at max_regions";

// the spec, refused before any state changes; the tracker (may be NULL) must live on this handle
void redact_request(rf_handle h, const rf_redact_spec *spec, rf_tracker tracker, const int *stream_of_image, int32_t *pixels, int *region_counts,
                    rf::RedactRequest *rq) {
    if (h->eng->num_devices() > 1) throw rf::Unsupported("face redaction is not available on a multi-device handle");
    const char *bad = rf::redact_spec_resolve(spec, h->eng->default_max_faces(), &rq->spec);
    if (bad) throw rf::ArgError(bad);
    if (tracker && tracker->h != h) throw rf::ArgError("not a tracker of this handle");
    rq->tracker = tracker ? tracker->impl : nullptr;
    rq->stream_of_image = tracker ? stream_of_image : nullptr;
    rq->pixels = pixels; rq->region_counts = region_counts;
}
}  // namespace

int rf_redact_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
                     int cap_per_image, const int *counts, const float *coord_scale, const rf_redact_spec *spec, rf_tracker tracker,
                     const int *stream_of_image, int32_t *pixels, int *region_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::RedactRequest rq;
        redact_request(h, spec, tracker, stream_of_image, pixels, region_counts, &rq);
        bool cut = false;
        h->eng->redact((const void *const *)d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, rq, &cut);
        if (cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int rf_redact_last_launch_ms(rf_handle h, float *ms) {
    if (!h || !ms) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        const float v = h->eng->redact_last_launch_ms();
        if (v < 0.f) throw rf::ArgError("no rf_redact_device call has been timed on this handle");
        *ms = v;
        return RF_OK;
    });
}

namespace {
int detect_redact_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                         float thr, rf_face *out, int cap, int *counts, const rf_redact_spec *spec, uint8_t *const *out_bgr, const int *out_steps,
                         int32_t *pixels) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RedactRequest rq;
        redact_request(h, spec, nullptr, nullptr, pixels, nullptr, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.redact = &rq; sc.out_bgr = out_bgr; sc.out_steps = out_steps;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.redact_cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_detect_redact_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                                  rf_face *out, int cap_per_image, int *counts, const rf_redact_spec *spec, int32_t *pixels) {
    return detect_redact_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, spec,
                                nullptr, nullptr, pixels);
}

int rf_detect_redact_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                           rf_face *out, int cap_per_image, int *counts, const rf_redact_spec *spec, uint8_t *const *out_bgr,
                           const int *out_steps, int32_t *pixels) {
    return detect_redact_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, spec, out_bgr, out_steps, pixels);
}

int rf_detect_track_redact_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                        float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                        const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                        const rf_redact_spec *spec, int32_t *pixels, int *region_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RedactRequest rq;
        redact_request(h, spec, tracker, stream_of_image, pixels, region_counts, &rq);
        rf::TrackRequest trq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &trq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.track = &trq; sc.redact = &rq;
        h->eng->detect_staged((const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tr, sc, &res);
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        if (res.redact_cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- overlays (overlay.h)
int rf_overlay_region(const rf_overlay_spec *spec, const rf_face *face, int64_t id, float coord_scale, int rows, int cols, int32_t out[24]) {
    rf::OverlaySpec sp;
    if (rf::overlay_spec_resolve(spec, 256, &sp) || !face || !out || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    const rf::OverlayRegion r = rf::overlay_region_make(sp, &face->score, id, coord_scale, false);
    const int32_t v[24] = {r.x0, r.y0, r.x1, r.y1, r.bx0, r.by0, r.bx1, r.by1, r.ndig, (int32_t)r.digits, r.plx, r.ply, (int32_t)r.colour,
                           (r.flags >> 8) & 31, r.cx[0], r.cx[1], r.cx[2], r.cx[3], r.cx[4], r.cy[0], r.cy[1], r.cy[2], r.cy[3], r.cy[4]};
    memcpy(out, v, sizeof(v));
    return r.flags & rf::kOverlayValid;
}

int rf_overlay_host(const rf_overlay_spec *spec, uint8_t *bgr, int rows, int cols, int step, const rf_face *faces, const int64_t *ids,
                    int count, float coord_scale, int32_t *pixels) {
    rf::OverlaySpec sp;
    if (rf::overlay_spec_resolve(spec, 256, &sp) || count < 0 || (count > 0 && !faces) || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    const bool empty = !bgr || rows == 0 || cols == 0;
    if (!empty && (step < cols * 3 || rows > 4096 * 3072 / cols)) return RF_ERR_INVALID_ARG;
    const int m = std::min(count, sp.max_regions);
    if (empty) { if (pixels) for (int k = 0; k < m; k++) pixels[k] = 0; }
    else {
        std::vector<rf::OverlayRegion> regions((size_t)m);
        for (int k = 0; k < m; k++) regions[k] = rf::overlay_region_make(sp, &faces[k].score, ids ? ids[k] : 0, coord_scale, false);
        rf::overlay_host_frame(sp, bgr, rows, cols, (size_t)step, regions.data(), m, pixels);
    }
    return count > sp.max_regions ? RF_ERR_TRUNCATED : RF_OK;
}

namespace {
// the spec, refused before any state changes; an overlay call travels as a redaction request with `overlay` set (engine.h)
void overlay_request(rf_handle h, const rf_overlay_spec *spec, rf_tracker tracker, const int *stream_of_image, int32_t *pixels, int *region_counts,
                     rf::RedactRequest *rq) {
    if (h->eng->num_devices() > 1) throw rf::Unsupported("overlays are not available on a multi-device handle");
    const char *bad = rf::overlay_spec_resolve(spec, h->eng->default_max_faces(), &rq->ospec);
    if (bad) throw rf::ArgError(bad);
    if (tracker && tracker->h != h) throw rf::ArgError("not a tracker of this handle");
    rq->overlay = true;
    rq->spec.max_regions = rq->ospec.max_regions; rq->spec.coast = rq->ospec.coast;
    rq->tracker = tracker ? tracker->impl : nullptr;
    rq->stream_of_image = tracker ? stream_of_image : nullptr;
    rq->pixels = pixels; rq->region_counts = region_counts;
}

int detect_overlay_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                          float thr, rf_face *out, int cap, int *counts, const rf_overlay_spec *spec, uint8_t *const *out_bgr, const int *out_steps,
                          int32_t *pixels) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RedactRequest rq;
        overlay_request(h, spec, nullptr, nullptr, pixels, nullptr, &rq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.redact = &rq; sc.out_bgr = out_bgr; sc.out_steps = out_steps;
        h->eng->detect_staged(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, sc, &res);
        if (res.redact_cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_overlay_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
                      const int64_t *ids, int cap_per_image, const int *counts, const float *coord_scale, const rf_overlay_spec *spec,
                      rf_tracker tracker, const int *stream_of_image, int32_t *pixels, int *region_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::RedactRequest rq;
        overlay_request(h, spec, tracker, stream_of_image, pixels, region_counts, &rq);
        rq.ids = ids;
        bool cut = false;
        h->eng->redact((const void *const *)d_bgr, rows, cols, steps, n, faces, cap_per_image, counts, coord_scale, rq, &cut);
        if (cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

int rf_overlay_last_launch_ms(rf_handle h, float *ms) {
    if (!h || !ms) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        const float v = h->eng->overlay_last_launch_ms();
        if (v < 0.f) throw rf::ArgError("no rf_overlay_device call has been timed on this handle");
        *ms = v;
        return RF_OK;
    });
}

int rf_detect_overlay_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                                   rf_face *out, int cap_per_image, int *counts, const rf_overlay_spec *spec, int32_t *pixels) {
    return detect_overlay_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, spec,
                                 nullptr, nullptr, pixels);
}

int rf_detect_overlay_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                            rf_face *out, int cap_per_image, int *counts, const rf_overlay_spec *spec, uint8_t *const *out_bgr,
                            const int *out_steps, int32_t *pixels) {
    return detect_overlay_common(h, bgr, rows, cols, steps, n, false, threshold, out, cap_per_image, counts, spec, out_bgr, out_steps, pixels);
}

int rf_detect_track_overlay_batch_device(rf_handle h, void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                         float threshold, rf_face *out, int cap_per_image, int *counts, rf_tracker tracker,
                                         const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts,
                                         const rf_overlay_spec *spec, int32_t *pixels, int *region_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RedactRequest rq;
        overlay_request(h, spec, tracker, stream_of_image, pixels, region_counts, &rq);
        rf::TrackRequest trq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &trq);
        rf::StageCall sc;
        rf::StageResult res;
        sc.track = &trq; sc.redact = &rq;
        h->eng->detect_staged((const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, out, cap_per_image, counts, tr, sc, &res);
        if (res.track_cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        if (res.redact_cut) { h->error = kRedactCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- flip test-time augmentation (tta.h)
int rf_tta_map_face(int rows, int cols, int net_h, int net_w, int pass, const rf_face *in, rf_face *out) {
    if (!in || !out || rows <= 0 || cols <= 0 || net_h <= 0 || net_w <= 0 || pass < 0 || pass > 1) return RF_ERR_INVALID_ARG;
    if (rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    rf::TtaEntry e{0, rows, cols, pass, rf::tile_frame_scale(rows, cols, net_h, net_w)};
    float f[15];
    memcpy(f, in, sizeof(f));
    rf::tta_map_face(e, f, f);
    memcpy(out, f, sizeof(f));
    return RF_OK;
}

int rf_tta_merge_host(const rf_tta_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_pass) {
    rf::TtaSpec sp;
    if (max_detections < 1 || max_detections > rf::kTtaMaxFaces || rf::tta_spec_resolve(spec, max_detections, &sp)) return RF_ERR_INVALID_ARG;
    if (!faces || !pass_counts || !count || cap < 0 || (cap > 0 && !out) || rows < 0 || cols < 0 || net_h <= 0 || net_w <= 0)
        return RF_ERR_INVALID_ARG;
    if (cols > 0 && rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    for (int p = 0; p < sp.passes(); p++)
        if (pass_counts[p] < 0) return RF_ERR_INVALID_ARG;
    bool truncated = false;
    std::vector<float> cand;
    std::vector<int> g;
    if (rows > 0 && cols > 0) {
        for (int p = 0; p < sp.passes(); p++) {
            const rf::TtaEntry e{0, rows, cols, p, rf::tile_frame_scale(rows, cols, net_h, net_w)};
            if (pass_counts[p] > max_detections) truncated = true;
            for (int k = 0; k < pass_counts[p] && k < max_detections; k++) {
                float f[15];
                memcpy(f, &faces[(size_t)p * max_detections + k], sizeof(f));
                rf::tta_map_face(e, f, f);
                cand.insert(cand.end(), f, f + 15);
                g.push_back(p * max_detections + k);
            }
        }
    }
    return merge_host_emit(cand, g, nms_threshold, sp.vote != 0, cap, sp.max_faces, max_detections, truncated, out, count, votes, src_pass);
}

namespace {
// a caller's TTA spec with its defaults applied; refused before the engine is touched
void tta_request(rf_handle h, const rf_tta_spec *spec, int *votes, int *src_pass, rf::TtaRequest *rq) {
    if (const char *bad = rf::tta_spec_resolve(spec, h->eng->default_max_faces(), &rq->spec)) throw rf::ArgError(bad);
    rq->votes = votes;
    rq->src_pass = src_pass;
}

int detect_tta_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                      float thr, const rf_tta_spec *spec, rf_face *out, int cap, int *counts, int *votes, int *src_pass) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::TtaRequest rq;
        tta_request(h, spec, votes, src_pass, &rq);
        h->eng->detect_tta(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq);
        return RF_OK;
    });
}
}  // namespace

int rf_mirror_device(rf_handle h, const void *d_src, int rows, int cols, int step, void *d_dst, int dst_step) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        h->eng->mirror(d_src, rows, cols, step, d_dst, dst_step);
        return RF_OK;
    });
}

int rf_detect_tta_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_tta_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                               int *src_pass) {
    return detect_tta_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts, votes,
                             src_pass);
}

int rf_detect_tta_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                        float threshold, const rf_tta_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass) {
    return detect_tta_common(h, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, votes, src_pass);
}

int rf_tta_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_tta_spec *spec, const rf_face *faces,
                        const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::TtaRequest rq;
        tta_request(h, spec, votes, src_pass, &rq);
        h->eng->tta_merge(rows, cols, n, rq, faces, pass_counts, out, cap_per_image, counts, tr);
        return RF_OK;
    });
}

// ---- rotation-robust detection (rot.h)
namespace {
// the orientation outputs of one frame from its emitted heads (merge order): the double sum of the scores per rotation, the rotation
// with the largest sum (ties: the lowest), -1 without a head
void rot_orientation(const rf_face *faces, const int *src_rot, int emitted, int *frame_rot, float *rot_score) {
    double sum[4] = {0, 0, 0, 0};
    int seen[4] = {0, 0, 0, 0};
    for (int j = 0; j < emitted; j++) {
        const int k = src_rot[j];
        if (k < 0 || k > 3) continue;
        sum[k] = sum[k] + (double)faces[j].score;
        seen[k] = 1;
    }
    int best = -1;
    for (int k = 0; k < 4; k++)
        if (seen[k] && (best < 0 || sum[k] > sum[best])) best = k;
    if (frame_rot) *frame_rot = best;
    if (rot_score)
        for (int k = 0; k < 4; k++) rot_score[k] = (float)sum[k];
}
}  // namespace

int rf_rot_map_face(int rows, int cols, int net_h, int net_w, int k, const rf_face *in, rf_face *out) {
    if (!in || !out || rows <= 0 || cols <= 0 || net_h <= 0 || net_w <= 0 || k < 0 || k > 3) return RF_ERR_INVALID_ARG;
    if (rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    rf::RotEntry e{0, rows, cols, k, rf::tile_frame_scale(rf::rot_rows(k, rows, cols), rf::rot_cols(k, rows, cols), net_h, net_w)};
    float f[15];
    memcpy(f, in, sizeof(f));
    rf::rot_map_face(e, f, f);
    memcpy(out, f, sizeof(f));
    return RF_OK;
}

int rf_rot_merge_host(const rf_rot_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_rot,
                      int *frame_rot, float *rot_score) {
    rf::RotSpec sp;
    if (max_detections < 1 || max_detections > rf::kTtaMaxFaces || rf::rot_spec_resolve(spec, max_detections, &sp)) return RF_ERR_INVALID_ARG;
    if (!faces || !pass_counts || !count || cap < 0 || (cap > 0 && !out) || rows < 0 || cols < 0 || net_h <= 0 || net_w <= 0)
        return RF_ERR_INVALID_ARG;
    if (cols > 0 && rows > 4096 * 3072 / cols) return RF_ERR_INVALID_ARG;
    for (int p = 0; p < sp.passes(); p++)
        if (pass_counts[p] < 0) return RF_ERR_INVALID_ARG;
    bool truncated = false;
    std::vector<float> cand;
    std::vector<int> g;
    if (rows > 0 && cols > 0) {
        int p = 0;
        for (int k = 0; k < 4; k++) {
            if (!(sp.rots >> k & 1)) continue;
            const rf::RotEntry e{0, rows, cols, k, rf::tile_frame_scale(rf::rot_rows(k, rows, cols), rf::rot_cols(k, rows, cols), net_h, net_w)};
            if (pass_counts[p] > max_detections) truncated = true;
            for (int j = 0; j < pass_counts[p] && j < max_detections; j++) {
                float f[15];
                memcpy(f, &faces[(size_t)p * max_detections + j], sizeof(f));
                rf::rot_map_face(e, f, f);
                cand.insert(cand.end(), f, f + 15);
                g.push_back(k * max_detections + j);
            }
            p++;
        }
    }
    std::vector<int> own;                        // the orientation outputs need the rotation of every head
    if (!src_rot) { own.resize((size_t)cap + 1); src_rot = own.data(); }
    int emitted = 0;
    const int st = merge_host_emit(cand, g, nms_threshold, sp.vote != 0, cap, sp.max_faces, max_detections, truncated, out, count, votes,
                                   src_rot, &emitted);
    rot_orientation(out, src_rot, emitted, frame_rot, rot_score);
    return st;
}

int rf_rotate_host(const uint8_t *src, int rows, int cols, int step, int k, uint8_t *dst, int dst_step) {
    if (rows < 0 || cols < 0 || k < 0 || k > 3) return RF_ERR_INVALID_ARG;
    if (rows == 0 || cols == 0) return RF_OK;
    if (!src || !dst || rows > 4096 * 3072 / cols || step < cols * 3 || dst_step < rf::rot_cols(k, rows, cols) * 3) return RF_ERR_INVALID_ARG;
    rf::rot_rotate_host(src, rows, cols, step, k, dst, dst_step);
    return RF_OK;
}

namespace {
// a caller's rotation spec with its defaults applied; refused before the engine is touched
void rot_request(rf_handle h, const rf_rot_spec *spec, int *votes, int *src_rot, rf::RotRequest *rq) {
    if (const char *bad = rf::rot_spec_resolve(spec, h->eng->default_max_faces(), &rq->spec)) throw rf::ArgError(bad);
    rq->votes = votes;
    rq->src_rot = src_rot;
}

// the orientation outputs of a finished call, from what it wrote for the caller
void rot_orient_call(const rf::RotRequest &rq, int n, const rf_face *out, int cap, const int *counts, const int *src_rot, int *frame_rot,
                     float *rot_score) {
    if (!frame_rot && !rot_score) return;
    for (int i = 0; i < n; i++) {
        const bool have = out && src_rot;
        const int emitted = have ? std::min(std::min(counts[i], rq.spec.max_faces), cap) : 0;
        rot_orientation(have ? out + (size_t)i * cap : nullptr, have ? src_rot + (size_t)i * cap : nullptr, emitted,
                        frame_rot ? frame_rot + i : nullptr, rot_score ? rot_score + (size_t)i * 4 : nullptr);
    }
}

int detect_rot_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                      float thr, const rf_rot_spec *spec, rf_face *out, int cap, int *counts, int *votes, int *src_rot, int *frame_rot,
                      float *rot_score) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RotRequest rq;
        std::vector<int> own;                    // the orientation outputs need the rotation of every head
        if (!src_rot && (frame_rot || rot_score) && n > 0 && cap > 0) { own.assign((size_t)n * cap, 0); src_rot = own.data(); }
        rot_request(h, spec, votes, src_rot, &rq);
        h->eng->detect_rot(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq);
        rot_orient_call(rq, n, src_rot ? out : nullptr, cap, counts, src_rot, frame_rot, rot_score);
        return RF_OK;
    });
}
}  // namespace

int rf_rotate_device(rf_handle h, const void *d_src, int rows, int cols, int step, int k, void *d_dst, int dst_step) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        h->eng->rotate(d_src, rows, cols, step, k, d_dst, dst_step);
        return RF_OK;
    });
}

int rf_detect_rot_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_rot_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                               int *src_rot, int *frame_rot, float *rot_score) {
    return detect_rot_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts, votes,
                             src_rot, frame_rot, rot_score);
}

int rf_detect_rot_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                        float threshold, const rf_rot_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_rot,
                        int *frame_rot, float *rot_score) {
    return detect_rot_common(h, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, votes, src_rot, frame_rot,
                             rot_score);
}

int rf_rot_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_rot_spec *spec, const rf_face *faces,
                        const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_rot, int *frame_rot,
                        float *rot_score) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::RotRequest rq;
        std::vector<int> own;
        if (!src_rot && (frame_rot || rot_score) && n > 0 && cap_per_image > 0) { own.assign((size_t)n * cap_per_image, 0); src_rot = own.data(); }
        rot_request(h, spec, votes, src_rot, &rq);
        h->eng->rot_merge(rows, cols, n, rq, faces, pass_counts, out, cap_per_image, counts, tr);
        rot_orient_call(rq, n, src_rot ? out : nullptr, cap_per_image, counts, src_rot, frame_rot, rot_score);
        return RF_OK;
    });
}

// ---- fisheye detection (dewarp.h)
int rf_dewarp_plan(const rf_dewarp_spec *spec, int view_w, int view_h, int32_t *mesh, int cap_ints, int *views) {
    if (!spec || !mesh || cap_ints < 0 || spec->struct_size != sizeof(rf_dewarp_spec)) return RF_ERR_INVALID_ARG;
    if (view_w < 16 || view_h < 16 || (view_w & 15) || (view_h & 15) || view_w > rf::kDewarpMaxW || view_h > rf::kDewarpMaxH) return RF_ERR_INVALID_ARG;
    rf_dewarp_view vw[rf::kDewarpMaxViews];
    const int V = rf::dewarp_spec_views(*spec, vw);
    if (!V || rf::dewarp_view_ints(view_w, view_h) * (size_t)V > (size_t)cap_ints) return RF_ERR_INVALID_ARG;
    if (rf::dewarp_plan(*spec, view_w, view_h, mesh, views)) return RF_ERR_INVALID_ARG;
    return RF_OK;
}

int rf_dewarp_host(const int32_t *view_mesh, int view_w, int view_h, const uint8_t *src, int rows, int cols, int step, uint8_t *dst,
                   int dst_step) {
    if (rf::dewarp_check_mesh(view_w, view_h, 1, view_mesh)) return RF_ERR_INVALID_ARG;
    if (!src || !dst || rows <= 0 || cols <= 0 || rows > 4096 * 3072 / cols || step < cols * 3 || dst_step < view_w * 3) return RF_ERR_INVALID_ARG;
    rf::dewarp_view_host(view_mesh, view_w, view_h, src, rows, cols, step, dst, dst_step);
    return RF_OK;
}

int rf_dewarp_map_face(const int32_t *view_mesh, int view_w, int view_h, int net_h, int net_w, int edge, const rf_face *in, rf_face *out) {
    if (!in || !out || net_h <= 0 || net_w <= 0 || edge < 0 || edge > 1024 || rf::dewarp_check_mesh(view_w, view_h, 1, view_mesh)) return RF_ERR_INVALID_ARG;
    rf::DewarpEntry e{0, 0, 0, 0, view_w, view_h, rf::tile_frame_scale(view_h, view_w, net_h, net_w), 0, view_mesh};
    float f[15];
    memcpy(f, in, sizeof(f));
    if (!rf::dewarp_map_face(e, edge, f, f)) return 0;
    memcpy(out, f, sizeof(f));
    return 1;
}

int rf_dewarp_merge_host(const rf_dewarp_spec *spec, const int32_t *mesh, int view_w, int view_h, int views, int net_h, int net_w,
                         float nms_threshold, int max_detections, const rf_face *faces, const int *pass_counts, rf_face *out, int cap,
                         int *count, int *votes, int *src_view) {
    rf::DewarpSpec sp;
    if (max_detections < 1 || max_detections > rf::kTtaMaxFaces || rf::dewarp_spec_resolve(spec, max_detections, &sp)) return RF_ERR_INVALID_ARG;
    if (!faces || !pass_counts || !count || cap < 0 || (cap > 0 && !out) || net_h <= 0 || net_w <= 0) return RF_ERR_INVALID_ARG;
    if (rf::dewarp_check_mesh(view_w, view_h, views, mesh)) return RF_ERR_INVALID_ARG;
    for (int v = 0; v < views; v++)
        if (pass_counts[v] < 0) return RF_ERR_INVALID_ARG;
    bool truncated = false;
    std::vector<float> cand;
    std::vector<int> g;
    const float scale = rf::tile_frame_scale(view_h, view_w, net_h, net_w);
    for (int v = 0; v < views; v++) {
        const rf::DewarpEntry e{0, v, 0, 0, view_w, view_h, scale, 0, mesh + (size_t)v * rf::dewarp_view_ints(view_w, view_h)};
        if (pass_counts[v] > max_detections) truncated = true;
        for (int j = 0; j < pass_counts[v] && j < max_detections; j++) {
            float f[15];
            memcpy(f, &faces[(size_t)v * max_detections + j], sizeof(f));
            if (!rf::dewarp_map_face(e, sp.edge, f, f)) continue;
            cand.insert(cand.end(), f, f + 15);
            g.push_back(v * max_detections + j);
        }
    }
    return merge_host_emit(cand, g, nms_threshold, sp.vote != 0, cap, sp.max_faces, max_detections, truncated, out, count, votes, src_view);
}

int rf_dewarper_create(rf_handle h, int rows, int cols, int view_w, int view_h, int views, const int32_t *mesh, rf_dewarper *out_dewarper) {
    if (out_dewarper) *out_dewarper = nullptr;
    if (!h || !out_dewarper) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        void *impl = h->eng->dewarper_create(rows, cols, view_w, view_h, views, mesh);
        rf_dewarper_s *d = new rf_dewarper_s{h, impl, views};
        h->dewarpers.push_back(d);
        *out_dewarper = d;
        return RF_OK;
    });
}

void rf_dewarper_destroy(rf_dewarper dewarper) {
    if (!dewarper) return;
    rf_engine *h = dewarper->h;
    (void)guarded(h, [&]() -> int {
        h->eng->dewarper_destroy(dewarper->impl);
        dewarper->impl = nullptr;          // the record stays until rf_destroy, so that a call on a destroyed dewarper is refused, not undefined
        return RF_OK;
    });
}

int rf_dewarp_device(rf_dewarper dewarper, int view, const void *d_src, int step, void *d_dst, int dst_step) {
    if (!dewarper) return RF_ERR_INVALID_ARG;
    return guarded(dewarper->h, [&]() -> int {
        dewarper->h->eng->dewarp(dewarper->impl, view, d_src, step, d_dst, dst_step);
        return RF_OK;
    });
}

namespace {
// a caller's fisheye spec with its defaults applied; refused before the engine is touched
void dewarp_request(rf_dewarper dw, const rf_dewarp_spec *spec, int *votes, int *src_view, void *d_views, rf::DewarpRequest *rq) {
    if (const char *bad = rf::dewarp_spec_resolve(spec, dw->h->eng->default_max_faces(), &rq->spec)) throw rf::ArgError(bad);
    rq->dewarper = dw->impl;
    rq->votes = votes; rq->src_view = src_view; rq->d_views = d_views;
}

int detect_dewarp_common(rf_dewarper dw, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                         bool on_device, float thr, const rf_dewarp_spec *spec, rf_face *out, int cap, int *counts, int *votes,
                         int *src_view, void *d_views) {
    if (!dw) return RF_ERR_INVALID_ARG;
    rf_engine *h = dw->h;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::DewarpRequest rq;
        dewarp_request(dw, spec, votes, src_view, d_views, &rq);
        h->eng->detect_dewarp(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq);
        return RF_OK;
    });
}
}  // namespace

int rf_detect_dewarp_batch_device(rf_dewarper dewarper, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                  float threshold, const rf_dewarp_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                                  int *src_view, void *d_views) {
    return detect_dewarp_common(dewarper, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts,
                                votes, src_view, d_views);
}

int rf_detect_dewarp_batch(rf_dewarper dewarper, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                           float threshold, const rf_dewarp_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                           int *src_view) {
    return detect_dewarp_common(dewarper, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, votes, src_view, nullptr);
}

int rf_dewarp_merge_device(rf_dewarper dewarper, int n, const rf_dewarp_spec *spec, const rf_face *faces, const int *pass_counts,
                           rf_face *out, int cap_per_image, int *counts, int *votes, int *src_view) {
    if (!dewarper) return RF_ERR_INVALID_ARG;
    rf_engine *h = dewarper->h;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::DewarpRequest rq;
        dewarp_request(dewarper, spec, votes, src_view, nullptr, &rq);
        h->eng->dewarp_merge(n, rq, faces, pass_counts, out, cap_per_image, counts, tr);
        return RF_OK;
    });
}

// ---- region detection (roi.h)
namespace {
// the host entry points' common checks: the spec (max_faces irrelevant where nothing is merged), the view and the regions
// (allow_void: the entry point takes the void region, four zeros, which stands for the void record)
int roi_host_args(const rf_roi_spec *spec, int default_max_faces, int view_w, int view_h, const rf_roi *rois, int n, rf::RoiSpec *sp,
                  bool allow_void = false) {
    if (rf::roi_spec_resolve(spec, default_max_faces, sp)) return RF_ERR_INVALID_ARG;
    if (rf::roi_check_view(view_w, view_h, sp->grid)) return RF_ERR_INVALID_ARG;
    if (n < 0 || n > rf::kRoiMaxRegions || (n > 0 && !rois)) return RF_ERR_INVALID_ARG;
    for (int r = 0; r < n; r++)
        if (!rf::roi_valid(rois[r]) && !(allow_void && rf::roi_is_void(rois[r]))) return RF_ERR_INVALID_ARG;
    return RF_OK;
}

void roi_cells_of(const rf::RoiSpec &sp, int view_w, int view_h, const rf_roi *rois, int n, std::vector<rf::RoiCell> *cells) {
    cells->resize((size_t)n);
    for (int r = 0; r < n; r++)
        (*cells)[r] = rf::roi_is_void(rois[r]) ? rf::roi_void_cell() : rf::roi_plan(rois[r], view_w / sp.grid, view_h / sp.grid, sp.max_zoom);
}
}  // namespace

int rf_roi_plan(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, rf_roi_cell *cells, int *passes) {
    rf::RoiSpec sp;
    if (roi_host_args(spec, 1, view_w, view_h, rois, n, &sp) || (n > 0 && !cells)) return RF_ERR_INVALID_ARG;
    std::vector<rf::RoiCell> c;
    roi_cells_of(sp, view_w, view_h, rois, n, &c);
    if (n) memcpy(cells, c.data(), (size_t)n * sizeof(rf_roi_cell));
    if (passes) *passes = rf::roi_passes(n, sp.grid);
    return RF_OK;
}

int rf_roi_from_faces(const rf_face *faces, int n, float coord_scale, int margin_q8, rf_roi *rois) {
    if (n < 0 || (n > 0 && (!faces || !rois)) || margin_q8 < 0 || margin_q8 > 65536 || !(coord_scale > 0.f) || !(coord_scale <= 65536.f)) return RF_ERR_INVALID_ARG;
    int k = 0;
    for (int i = 0; i < n; i++) {
        float f[15];
        memcpy(f, &faces[i], sizeof(f));
        if (rf::roi_from_face(f, coord_scale, margin_q8 ? margin_q8 : 64, &rois[k])) k++;
    }
    return k;
}

int rf_roi_atlas_host(const rf_roi_spec *spec, int view_w, int view_h, const uint8_t *src, int rows, int cols, int step, const rf_roi *rois,
                      int n, uint8_t *dst, int dst_step) {
    rf::RoiSpec sp;
    if (roi_host_args(spec, 1, view_w, view_h, rois, n, &sp, true)) return RF_ERR_INVALID_ARG;
    if (!src || !dst || rows <= 0 || cols <= 0 || rows > 4096 * 3072 / cols || step < cols * 3 || dst_step < view_w * 3) return RF_ERR_INVALID_ARG;
    std::vector<rf::RoiCell> c;
    roi_cells_of(sp, view_w, view_h, rois, n, &c);
    const int GG = sp.grid * sp.grid;
    for (int p = 0; p < rf::roi_passes(n, sp.grid); p++)
        rf::roi_atlas_host(src, rows, cols, step, c.data() + (size_t)p * GG, std::min(GG, n - p * GG), sp.grid, view_w, view_h,
                           dst + (size_t)p * view_h * dst_step, dst_step);
    return RF_OK;
}

int rf_roi_map_face(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, int pass, const rf_face *in, rf_face *out,
                    int *region) {
    rf::RoiSpec sp;
    if (!in || !out || roi_host_args(spec, 1, view_w, view_h, rois, n, &sp, true)) return RF_ERR_INVALID_ARG;
    if (pass < 0 || pass >= rf::roi_passes(n, sp.grid)) return RF_ERR_INVALID_ARG;
    std::vector<rf::RoiCell> c;
    roi_cells_of(sp, view_w, view_h, rois, n, &c);
    const int GG = sp.grid * sp.grid;
    const rf::RoiEntry e{0, pass, 0, 0, sp.grid, std::min(GG, n - pass * GG), view_w, view_h, c.data() + (size_t)pass * GG};
    float f[15];
    memcpy(f, in, sizeof(f));
    int r = 0;
    if (!rf::roi_map_face(e, f, f, &r)) return 0;
    memcpy(out, f, sizeof(f));
    if (region) *region = r;
    return 1;
}

int rf_roi_merge_host(const rf_roi_spec *spec, int view_w, int view_h, const rf_roi *rois, int n, float nms_threshold, int max_detections,
                      const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_roi) {
    rf::RoiSpec sp;
    if (max_detections < 1 || max_detections > rf::kTtaMaxFaces || roi_host_args(spec, max_detections, view_w, view_h, rois, n, &sp)) return RF_ERR_INVALID_ARG;
    const int P = rf::roi_passes(n, sp.grid), GG = sp.grid * sp.grid;
    if (!count || cap < 0 || (cap > 0 && !out) || (P > 0 && (!faces || !pass_counts))) return RF_ERR_INVALID_ARG;
    for (int p = 0; p < P; p++)
        if (pass_counts[p] < 0) return RF_ERR_INVALID_ARG;
    std::vector<rf::RoiCell> c;
    roi_cells_of(sp, view_w, view_h, rois, n, &c);
    bool truncated = false;
    std::vector<float> cand;
    std::vector<int> g;
    for (int p = 0; p < P; p++) {
        const rf::RoiEntry e{0, p, 0, 0, sp.grid, std::min(GG, n - p * GG), view_w, view_h, c.data() + (size_t)p * GG};
        if (pass_counts[p] > max_detections) truncated = true;
        for (int j = 0; j < pass_counts[p] && j < max_detections; j++) {
            float f[15];
            memcpy(f, &faces[(size_t)p * max_detections + j], sizeof(f));
            int r = 0;
            if (!rf::roi_map_face(e, f, f, &r)) continue;
            cand.insert(cand.end(), f, f + 15);
            g.push_back(r * max_detections + j);
        }
    }
    const int limit = cap < sp.max_faces ? cap : sp.max_faces;
    std::vector<float> merged((size_t)limit * 15 + 1);
    std::vector<int> vt((size_t)limit + 1), hg((size_t)limit + 1);
    const int heads = rf::tta_merge_candidates(cand, g, nms_threshold, sp.vote != 0, limit, merged.data(), vt.data(), hg.data());
    *count = heads;
    const int emitted = heads < limit ? heads : limit;
    for (int j = 0; j < emitted; j++) {
        memset(&out[j], 0, sizeof(rf_face));
        memcpy(&out[j], &merged[(size_t)j * 15], 15 * sizeof(float));
        if (votes) votes[j] = vt[j];
        if (src_roi) src_roi[j] = hg[j] / max_detections;
    }
    return truncated || heads > limit ? RF_ERR_TRUNCATED : RF_OK;
}

int rf_roi_atlas_device(rf_handle h, const void *d_src, int rows, int cols, int step, const rf_roi *rois, int n, const rf_roi_spec *spec,
                        int view_w, int view_h, void *d_dst, int dst_step) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::RoiSpec sp;
        if (const char *bad = rf::roi_spec_resolve(spec, h->eng->default_max_faces(), &sp)) throw rf::ArgError(bad);
        h->eng->roi_atlas(d_src, rows, cols, step, rois, n, sp, view_w, view_h, d_dst, dst_step);
        return RF_OK;
    });
}

namespace {
// a caller's region spec with its defaults applied; refused before the engine is touched
void roi_request(rf_handle h, const rf_roi_spec *spec, const rf_roi *rois, const int *roi_counts, int *votes, int *src_roi, void *d_views,
                 rf::RoiRequest *rq) {
    if (const char *bad = rf::roi_spec_resolve(spec, h->eng->default_max_faces(), &rq->spec)) throw rf::ArgError(bad);
    rq->rois = rois; rq->roi_counts = roi_counts;
    rq->votes = votes; rq->src_roi = src_roi; rq->d_views = d_views;
}

int detect_roi_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                      const rf_roi *rois, const int *roi_counts, float thr, const rf_roi_spec *spec, rf_face *out, int cap, int *counts,
                      int *votes, int *src_roi, void *d_views) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::RoiRequest rq;
        roi_request(h, spec, rois, roi_counts, votes, src_roi, d_views, &rq);
        bool tr = false;
        h->eng->detect_rois(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, &tr, rq);
        if (tr) { h->error = "more candidates / detections than the configured caps"; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_detect_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                               const rf_roi *rois, const int *roi_counts, float threshold, const rf_roi_spec *spec, rf_face *out,
                               int cap_per_image, int *counts, int *votes, int *src_roi, void *d_views) {
    return detect_roi_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, rois, roi_counts, threshold, spec, out, cap_per_image,
                             counts, votes, src_roi, d_views);
}

int rf_detect_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, const rf_roi *rois,
                        const int *roi_counts, float threshold, const rf_roi_spec *spec, rf_face *out, int cap_per_image, int *counts,
                        int *votes, int *src_roi) {
    return detect_roi_common(h, bgr, rows, cols, steps, n, false, rois, roi_counts, threshold, spec, out, cap_per_image, counts, votes, src_roi,
                             nullptr);
}

// ---- tracked region detection (roi.h roi_track_cell)
int rf_roi_cells_from_tracks(const rf_track_spec *spec, const rf_motion_spec *mspec, const rf_track *table, const rf_track_motion *motion,
                             int max_tracks, int margin_q8, int net_w, int net_h, const rf_roi_spec *roi_spec, rf_roi_cell *cells) {
    rf::TrackSpec ts;
    rf::MotionSpec ms;
    rf::RoiSpec sp;
    if (rf::track_spec_resolve(spec, &ts) || rf::motion_spec_resolve(mspec, &ms) || rf::roi_spec_resolve(roi_spec, 1, &sp)) return RF_ERR_INVALID_ARG;
    if (rf::roi_check_view(net_w, net_h, sp.grid)) return RF_ERR_INVALID_ARG;
    if (max_tracks < 1 || max_tracks > rf::kTrackMaxTracks || margin_q8 < 0 || margin_q8 > 65535 || !table || !cells) return RF_ERR_INVALID_ARG;
    rf::roi_cells_from_tracks(table, motion, ms, max_tracks, margin_q8, net_w / sp.grid, net_h / sp.grid, sp.max_zoom, cells);
    return RF_OK;
}

int rf_roi_track_cells_device(rf_handle h, rf_tracker tracker, const int *stream_of_image, int n, int margin_q8, const rf_roi_spec *roi_spec,
                              rf_roi_cell *cells) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("region detection is not available on a multi-device handle");
        rf::RoiTrackRequest rq;
        if (const char *bad = rf::roi_spec_resolve(roi_spec, h->eng->default_max_faces(), &rq.spec)) throw rf::ArgError(bad);
        rq.margin_q8 = margin_q8;
        rf::TrackRequest trq;
        track_request(h, tracker, stream_of_image, nullptr, nullptr, 0, nullptr, &trq);
        h->eng->roi_track_cells(trq, n, rq, cells);
        return RF_OK;
    });
}

namespace {
int detect_track_roi_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                            float thr, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap, int *counts, int *src_roi, int *votes,
                            rf_roi_cell *cells, void *d_views, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                            rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        if (h->eng->num_devices() > 1) throw rf::Unsupported("region detection is not available on a multi-device handle");
        rf::RoiTrackRequest rq;
        if (const char *bad = rf::roi_spec_resolve(roi_spec, h->eng->default_max_faces(), &rq.spec)) throw rf::ArgError(bad);
        rq.margin_q8 = margin_q8;
        rq.votes = votes; rq.src_roi = src_roi; rq.cells = cells; rq.d_views = d_views;
        rf::TrackRequest trq;
        track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &trq);
        bool cut = false;
        h->eng->detect_track_rois(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq, trq, &cut);
        if (cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_detect_track_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                     float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                                     int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_tracker tracker,
                                     const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_roi_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, roi_spec, margin_q8, out, cap_per_image,
                                   counts, src_roi, votes, cells, d_views, tracker, stream_of_image, tags, ended, cap_ended, ended_counts);
}

int rf_detect_track_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n, float threshold,
                              const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts, int *src_roi, int *votes,
                              rf_roi_cell *cells, void *d_views, rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags,
                              rf_track *ended, int cap_ended, int *ended_counts) {
    return detect_track_roi_common(h, bgr, rows, cols, steps, n, false, threshold, roi_spec, margin_q8, out, cap_per_image, counts, src_roi, votes,
                                   cells, d_views, tracker, stream_of_image, tags, ended, cap_ended, ended_counts);
}

// ---- change regions (change.h)
int rf_changer_create(rf_handle h, const rf_change_spec *spec, int rows, int cols, int n_streams, rf_changer *out_changer) {
    rf::ChangeSpec sp;
    if (out_changer) *out_changer = nullptr;
    const char *bad = rf::change_spec_resolve(spec, &sp);             // spec, shape and range first: refused without a GPU
    int bw = 0, bh = 0;
    if (!bad) bad = rf::change_check_shape(rows, cols, sp, &bw, &bh);
    if (!bad && (n_streams < 1 || n_streams > rf::kChangeMaxStreams)) bad = "n_streams must be in [1, 1024]";
    if (!h || !out_changer) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        if (bad) throw rf::ArgError(std::string("changer: ") + bad);
        void *impl = h->eng->changer_create(sp, rows, cols, n_streams);
        rf_changer_s *c = new rf_changer_s{h, impl};
        h->changers.push_back(c);
        *out_changer = c;
        return RF_OK;
    });
}

void rf_changer_destroy(rf_changer changer) {
    if (!changer) return;
    rf_engine *h = changer->h;
    (void)guarded(h, [&]() -> int {
        h->eng->changer_destroy(changer->impl);
        changer->impl = nullptr;           // the record stays until rf_destroy, so that a call on a destroyed changer is refused, not undefined
        return RF_OK;
    });
}

int rf_changer_reset(rf_changer changer, int stream) {
    if (!changer) return RF_ERR_INVALID_ARG;
    return guarded(changer->h, [&]() -> int { changer->h->eng->changer_reset(changer->impl, stream); return RF_OK; });
}

int rf_changer_read(rf_changer changer, int stream, int32_t *ref, int64_t *frames, uint8_t *mask) {
    if (!changer) return RF_ERR_INVALID_ARG;
    return guarded(changer->h, [&]() -> int { return changer->h->eng->changer_read(changer->impl, stream, ref, frames, mask); });
}

int rf_change_step_host(const rf_change_spec *spec, const uint8_t *bgr, int rows, int cols, int step, int32_t *ref, int64_t *counter,
                        int margin_q8, int net_w, int net_h, const rf_roi_spec *roi_spec, uint8_t *mask, rf_roi *regions, rf_roi_cell *cells,
                        rf_change_info *info) {
    rf::ChangeSpec sp;
    rf::RoiSpec rs;
    int bw = 0, bh = 0;
    if (rf::change_spec_resolve(spec, &sp) || rf::roi_spec_resolve(roi_spec, 1, &rs)) return RF_ERR_INVALID_ARG;
    if (rf::change_check_shape(rows, cols, sp, &bw, &bh) || rf::roi_check_view(net_w, net_h, rs.grid)) return RF_ERR_INVALID_ARG;
    if (!bgr || step < cols * 3 || margin_q8 < 0 || margin_q8 > 65535 || !ref || !counter || *counter < 0 || !mask || !regions || !cells || !info)
        return RF_ERR_INVALID_ARG;
    rf::change_step_host(sp, bgr, rows, cols, (size_t)step, bw, bh, ref, counter, margin_q8, net_w / rs.grid, net_h / rs.grid, rs.max_zoom, mask,
                         regions, cells, info);
    return RF_OK;
}

namespace {
void change_request(rf_handle h, rf_changer changer, const rf_roi_spec *roi_spec, int margin_q8, const int *stream_of_image, rf::ChangeRequest *rq) {
    if (h->eng->num_devices() > 1) throw rf::Unsupported("change regions are not available on a multi-device handle");
    if (!changer || changer->h != h || !changer->impl) throw rf::ArgError("not a changer of this handle");
    if (const char *bad = rf::roi_spec_resolve(roi_spec, h->eng->default_max_faces(), &rq->spec)) throw rf::ArgError(bad);
    rq->changer = changer->impl;
    rq->margin_q8 = margin_q8;
    rq->stream_of_image = stream_of_image;
}
}  // namespace

int rf_change_regions_device(rf_handle h, rf_changer changer, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                             const int *stream_of_image, int n, int margin_q8, const rf_roi_spec *roi_spec, rf_roi_cell *cells,
                             rf_change_info *info) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::ChangeRequest rq;
        change_request(h, changer, roi_spec, margin_q8, stream_of_image, &rq);
        rq.cells = cells; rq.info = info;
        h->eng->change_regions(d_bgr, rows, cols, steps, n, rq);
        return RF_OK;
    });
}

namespace {
int detect_change_roi_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                             float thr, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap, int *counts, int *src_roi, int *votes,
                             rf_roi_cell *cells, void *d_views, rf_changer changer, rf_change_info *info, rf_tracker tracker,
                             const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended, int *ended_counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::ChangeRequest rq;
        change_request(h, changer, roi_spec, margin_q8, stream_of_image, &rq);
        rq.votes = votes; rq.src_roi = src_roi; rq.cells = cells; rq.info = info; rq.d_views = d_views;
        rf::TrackRequest trq;
        if (tracker) track_request(h, tracker, stream_of_image, tags, ended, cap_ended, ended_counts, &trq);
        bool cut = false;
        h->eng->detect_change_rois(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq, trq, &cut);
        if (cut) { h->error = kTrackCut; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}
}  // namespace

int rf_detect_change_roi_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                      float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                                      int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_changer changer, rf_change_info *info,
                                      rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended,
                                      int *ended_counts) {
    return detect_change_roi_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, roi_spec, margin_q8, out, cap_per_image,
                                    counts, src_roi, votes, cells, d_views, changer, info, tracker, stream_of_image, tags, ended, cap_ended,
                                    ended_counts);
}

int rf_detect_change_roi_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                               float threshold, const rf_roi_spec *roi_spec, int margin_q8, rf_face *out, int cap_per_image, int *counts,
                               int *src_roi, int *votes, rf_roi_cell *cells, void *d_views, rf_changer changer, rf_change_info *info,
                               rf_tracker tracker, const int *stream_of_image, rf_track_tag *tags, rf_track *ended, int cap_ended,
                               int *ended_counts) {
    return detect_change_roi_common(h, bgr, rows, cols, steps, n, false, threshold, roi_spec, margin_q8, out, cap_per_image, counts, src_roi, votes,
                                    cells, d_views, changer, info, tracker, stream_of_image, tags, ended, cap_ended, ended_counts);
}

int rf_roi_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_roi *rois, const int *roi_counts,
                        const rf_roi_spec *spec, const rf_face *faces, const int *pass_counts, rf_face *out, int cap_per_image, int *counts,
                        int *votes, int *src_roi) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::RoiRequest rq;
        roi_request(h, spec, rois, roi_counts, votes, src_roi, nullptr, &rq);
        bool tr = false;
        h->eng->roi_merge(rows, cols, n, rq, faces, pass_counts, out, cap_per_image, counts, &tr);
        if (tr) { h->error = "more candidates / detections than the configured caps"; return RF_ERR_TRUNCATED; }
        return RF_OK;
    });
}

// ---- low-light enhancement (enhance.h)
int rf_enhance_host(const rf_enhance_spec *spec, const uint8_t *src, int rows, int cols, int step, uint8_t *dst, int dst_step,
                    int *tiles_enhanced) {
    rf::EnhanceSpec sp;
    if (rf::enhance_spec_resolve(spec, &sp) || rows < 0 || cols < 0) return RF_ERR_INVALID_ARG;
    if (tiles_enhanced) *tiles_enhanced = 0;
    if (rows == 0 || cols == 0) return RF_OK;
    if (!src || !dst || rows > 4096 * 3072 / cols || step < cols * 3 || dst_step < cols * 3) return RF_ERR_INVALID_ARG;
    if (dst != src || dst_step != step) {       // the frame itself is the one legal overlap
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)(rows - 1) * step + (size_t)cols * 3;
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)(rows - 1) * dst_step + (size_t)cols * 3;
        if (s0 < d1 && d0 < s1) return RF_ERR_INVALID_ARG;
    }
    const int flagged = rf::enhance_host(sp, src, rows, cols, step, dst, dst_step);
    if (tiles_enhanced) *tiles_enhanced = flagged;
    return RF_OK;
}

int rf_enhance_device(rf_handle h, const rf_enhance_spec *spec, const void *const *d_src, const int *rows, const int *cols,
                      const int *steps, int n, void *const *d_dst, const int *dst_steps, int *tiles_enhanced) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        rf::EnhanceSpec sp;
        if (const char *bad = rf::enhance_spec_resolve(spec, &sp)) throw rf::ArgError(bad);
        h->eng->enhance(sp, d_src, rows, cols, steps, n, d_dst, dst_steps, tiles_enhanced);
        return RF_OK;
    });
}

namespace {
int detect_enhanced_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                           bool on_device, float thr, const rf_enhance_spec *spec, rf_face *out, int cap, int *counts,
                           void *const *d_enhanced, const int *enhanced_steps, int *tiles_enhanced) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::EnhanceRequest rq;
        if (const char *bad = rf::enhance_spec_resolve(spec, &rq.spec)) throw rf::ArgError(bad);
        rq.d_enhanced = d_enhanced; rq.enhanced_steps = enhanced_steps; rq.tiles_enhanced = tiles_enhanced;
        h->eng->detect_enhanced(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq);
        return RF_OK;
    });
}
}  // namespace

int rf_detect_enhanced_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                    float threshold, const rf_enhance_spec *spec, rf_face *out, int cap_per_image, int *counts,
                                    void *const *d_enhanced, const int *enhanced_steps, int *tiles_enhanced) {
    return detect_enhanced_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts,
                                  d_enhanced, enhanced_steps, tiles_enhanced);
}

int rf_detect_enhanced_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                             float threshold, const rf_enhance_spec *spec, rf_face *out, int cap_per_image, int *counts,
                             void *const *d_enhanced, const int *enhanced_steps, int *tiles_enhanced) {
    return detect_enhanced_common(h, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, d_enhanced,
                                  enhanced_steps, tiles_enhanced);
}

// ---- zoom-pyramid detection (pyramid.h)
namespace {
// the plan of one frame for the host-only entry points: false = refused
bool pyr_host_plan(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, int default_max_faces, rf::PyrSpec *sp,
                   std::vector<rf::PyrEntry> *entries) {
    if (net_h <= 0 || net_w <= 0 || rows < 0 || cols < 0 || rf::pyr_spec_resolve(spec, net_h, net_w, default_max_faces, sp)) return false;
    if (cols > 0 && rows > 4096 * 3072 / cols) return false;
    entries->clear();
    if (rows == 0 || cols == 0) {                      // an empty frame: one pass that finds nothing
        rf::PyrEntry e;
        memset(&e, 0, sizeof(e));
        e.frame = -1; e.z = 1; e.scale = 1.f;
        entries->push_back(e);
        return true;
    }
    size_t zoom_bytes = 0;
    if (rf::pyr_plan(*sp, rows, cols, net_h, net_w, 0, entries, &zoom_bytes) < 0) return false;
    return zoom_bytes <= rf::kPyrMaxZoomBytes;
}
}  // namespace

int rf_pyramid_plan(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, int *zxywh, int cap_passes) {
    rf::PyrSpec sp;
    std::vector<rf::PyrEntry> entries;
    if (cap_passes < 0 || !pyr_host_plan(spec, rows, cols, net_h, net_w, 256, &sp, &entries)) return RF_ERR_INVALID_ARG;
    const int passes = (int)entries.size();
    for (int p = 0; zxywh && p < passes && p < cap_passes; p++) {
        const rf::PyrEntry &e = entries[p];
        zxywh[5 * p] = e.z; zxywh[5 * p + 1] = e.x0; zxywh[5 * p + 2] = e.y0; zxywh[5 * p + 3] = e.tw; zxywh[5 * p + 4] = e.th;
    }
    return passes;
}

int rf_pyramid_map_face(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, int p, const rf_face *in, rf_face *out) {
    rf::PyrSpec sp;
    std::vector<rf::PyrEntry> entries;
    if (!in || !out || !pyr_host_plan(spec, rows, cols, net_h, net_w, 256, &sp, &entries)) return RF_ERR_INVALID_ARG;
    if (p < 0 || p >= (int)entries.size() || entries[p].frame < 0) return RF_ERR_INVALID_ARG;
    float f[15];
    memcpy(f, in, sizeof(f));
    if (!rf::pyr_map_face(entries[p], sp.tile.edge, f, f)) return 0;
    memcpy(out, f, sizeof(f));
    return 1;
}

int rf_pyramid_merge_host(const rf_pyramid_spec *spec, int rows, int cols, int net_h, int net_w, float nms_threshold, int max_detections,
                          const rf_face *faces, const int *pass_counts, rf_face *out, int cap, int *count, int *votes, int *src_pass) {
    rf::PyrSpec sp;
    std::vector<rf::PyrEntry> entries;
    if (max_detections < 1 || max_detections > rf::kTtaMaxFaces) return RF_ERR_INVALID_ARG;
    if (!pyr_host_plan(spec, rows, cols, net_h, net_w, max_detections, &sp, &entries)) return RF_ERR_INVALID_ARG;
    if (!faces || !pass_counts || !count || cap < 0 || (cap > 0 && !out)) return RF_ERR_INVALID_ARG;
    const int P = (int)entries.size();
    for (int p = 0; p < P; p++)
        if (pass_counts[p] < 0) return RF_ERR_INVALID_ARG;
    bool truncated = false;
    std::vector<float> cand;
    std::vector<int> g;
    for (int p = 0; p < P; p++) {
        if (pass_counts[p] > max_detections) truncated = true;
        if (entries[p].frame < 0) continue;
        for (int k = 0; k < pass_counts[p] && k < max_detections; k++) {
            float f[15];
            memcpy(f, &faces[(size_t)p * max_detections + k], sizeof(f));
            if (!rf::pyr_map_face(entries[p], sp.tile.edge, f, f)) continue;
            cand.insert(cand.end(), f, f + 15);
            g.push_back(p * max_detections + k);
        }
    }
    return merge_host_emit(cand, g, nms_threshold, sp.vote != 0, cap, sp.tile.max_faces, max_detections, truncated, out, count, votes,
                           src_pass);
}

int rf_zoom_host(const uint8_t *src, int rows, int cols, int step, int z, int x0, int y0, int tw, int th, uint8_t *dst, int dst_step) {
    if (rows < 0 || cols < 0 || tw < 0 || th < 0 || (z != 2 && z != 4)) return RF_ERR_INVALID_ARG;
    if (rows == 0 || cols == 0 || tw == 0 || th == 0) return RF_OK;
    if (!src || !dst || rows > 4096 * 3072 / cols || step < cols * 3 || dst_step < tw * 3) return RF_ERR_INVALID_ARG;
    if (x0 < 0 || y0 < 0 || x0 > z * cols - tw || y0 > z * rows - th) return RF_ERR_INVALID_ARG;
    for (int y = 0; y < th; y++)
        for (int x = 0; x < tw; x++)
            rf::pyr_zoom_pixel(src, rows, cols, (size_t)step, z, x0 + x, y0 + y, dst + (size_t)y * dst_step + (size_t)3 * x);
    return RF_OK;
}

namespace {
// a caller's pyramid spec with its defaults applied; refused before the engine is touched
void pyr_request(rf_handle h, const rf_pyramid_spec *spec, int *votes, int *src_pass, rf::PyrRequest *rq) {
    if (const char *bad = rf::pyr_spec_resolve(spec, h->eng->net_h(), h->eng->net_w(), h->eng->default_max_faces(), &rq->spec))
        throw rf::ArgError(bad);
    rq->votes = votes;
    rq->src_pass = src_pass;
}

int detect_pyramid_common(rf_handle h, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                          bool on_device, float thr, const rf_pyramid_spec *spec, rf_face *out, int cap, int *counts, int *votes,
                          int *src_pass) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::PyrRequest rq;
        pyr_request(h, spec, votes, src_pass, &rq);
        h->eng->detect_pyramid(frames, rows, cols, steps, n, on_device, thr, out, cap, counts, tr, rq);
        return RF_OK;
    });
}
}  // namespace

int rf_zoom_device(rf_handle h, const void *d_src, int rows, int cols, int step, int z, int x0, int y0, int tw, int th, void *d_dst,
                   int dst_step) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        h->eng->zoom(d_src, rows, cols, step, z, x0, y0, tw, th, d_dst, dst_step);
        return RF_OK;
    });
}

int rf_detect_pyramid_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps, int n,
                                   float threshold, const rf_pyramid_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                                   int *src_pass) {
    return detect_pyramid_common(h, (const uint8_t *const *)d_bgr, rows, cols, steps, n, true, threshold, spec, out, cap_per_image, counts,
                                 votes, src_pass);
}

int rf_detect_pyramid_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                            float threshold, const rf_pyramid_spec *spec, rf_face *out, int cap_per_image, int *counts, int *votes,
                            int *src_pass) {
    return detect_pyramid_common(h, bgr, rows, cols, steps, n, false, threshold, spec, out, cap_per_image, counts, votes, src_pass);
}

int rf_pyramid_merge_device(rf_handle h, const int *rows, const int *cols, int n, const rf_pyramid_spec *spec, const rf_face *faces,
                            const int *pass_counts, rf_face *out, int cap_per_image, int *counts, int *votes, int *src_pass) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        rf::PyrRequest rq;
        pyr_request(h, spec, votes, src_pass, &rq);
        h->eng->pyramid_merge(rows, cols, n, rq, faces, pass_counts, out, cap_per_image, counts, tr);
        return RF_OK;
    });
}

int rf_num_slots(rf_handle h) { return h ? h->eng->num_slots() : RF_ERR_INVALID_ARG; }

int rf_enqueue_batch_device(rf_handle h, const void *const *d_bgr, const int *rows, const int *cols, const int *steps,
                            int n, float threshold, int *ticket) {
    if (!h || !ticket) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { *ticket = h->eng->enqueue(d_bgr, rows, cols, steps, n, true, threshold); return RF_OK; });
}

int rf_enqueue_batch(rf_handle h, const uint8_t *const *bgr, const int *rows, const int *cols, const int *steps, int n,
                     float threshold, int *ticket) {
    if (!h || !ticket) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int {
        *ticket = h->eng->enqueue((const void *const *)bgr, rows, cols, steps, n, false, threshold);
        return RF_OK;
    });
}

int rf_host_register(rf_handle h, const void *ptr, size_t bytes) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { h->eng->host_register(ptr, bytes); return RF_OK; });
}

int rf_host_unregister(rf_handle h, const void *ptr) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { h->eng->host_unregister(ptr); return RF_OK; });
}

int rf_invalidate_residency(rf_handle h) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { h->eng->invalidate_residency(); return RF_OK; });
}

int rf_num_devices(rf_handle h) { return h ? h->eng->num_devices() : RF_ERR_INVALID_ARG; }

int rf_scatter_stats(rf_handle h, long long *frames, long long *copies) {
    if (!h || !frames || !copies) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { *frames = 0; *copies = 0; h->eng->scatter_stats(frames, copies); return RF_OK; });
}

int rf_launch_stats(rf_handle h, long long *launches, long long *images) {
    if (!h || !launches || !images) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { *launches = 0; *images = 0; h->eng->launch_stats(launches, images); return RF_OK; });
}

int rf_wait(rf_handle h, int ticket, rf_face *out, int cap_per_image, int *counts) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded_caps(h, [&](bool *tr) -> int {
        h->eng->wait(ticket, out, cap_per_image, counts, tr);
        return RF_OK;
    });
}

int rf_last_anchor_indices(rf_handle h, int image, int32_t *out, int cap) {
    if (!h || (cap > 0 && !out)) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { return h->eng->last_anchor_indices(image, out, cap); });
}

int rf_last_candidate_counts(rf_handle h, int *counts, int n) {
    if (!h || !counts) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { return h->eng->last_candidate_counts(counts, n); });
}

int rf_last_timings(rf_handle h, float *pre_ms, float *infer_ms, float *post_ms, float *total_ms) {
    if (!h) return RF_ERR_INVALID_ARG;
    h->eng->last_timings(pre_ms, infer_ms, post_ms, total_ms);
    return RF_OK;
}

long rf_get_output(rf_handle h, const char *blob_name, int image, float *dst, size_t cap_floats) {
    if (!h || !blob_name) return RF_ERR_INVALID_ARG;
    long r = 0;
    int st = guarded(h, [&]() -> int { r = h->eng->get_output(blob_name, image, dst, cap_floats); return RF_OK; });
    return st == RF_OK ? r : st;
}

long rf_debug_activation(rf_handle h, const char *blob_name, int image, float *dst, size_t cap_floats, int dims[3]) {
    if (!h || !blob_name) return RF_ERR_INVALID_ARG;
    long r = 0;
    int st = guarded(h, [&]() -> int { r = h->eng->debug_activation(blob_name, image, dst, cap_floats, dims); return RF_OK; });
    return st == RF_OK ? r : st;
}

void rf_debug_resident_cap(int workgroups) { rf::debug_resident_cap(workgroups); }

int rf_debug_grid_log(int cap, int *tiles, int *grid) {
    if (cap < 0 || (cap > 0 && (!tiles || !grid))) return RF_ERR_INVALID_ARG;
    return rf::debug_grid_log(cap, tiles, grid);
}

int rf_debug_face_bands(int crop_size, int format, int *band_rows, int *ring_rows) {
    if (crop_size < rf::kAlignMinCrop || crop_size > rf::kAlignMaxCrop) return RF_ERR_INVALID_ARG;
    if (format != RF_FACES_U8_HWC && format != RF_FACES_F16_CHW && format != RF_FACES_F32_CHW) return RF_ERR_INVALID_ARG;
    if (band_rows) *band_rows = rf::face_batch_band_rows(crop_size, format);
    if (ring_rows) *ring_rows = rf::face_quality_ring_rows(crop_size);
    return RF_OK;
}

int rf_profile(rf_handle h, const void *const *d_bgr, int n, int iters, int cap, const char **names, const char **kernels,
               float *avg_ms, double *alg_bytes, double *macs) {
    if (!h || !d_bgr) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { return h->eng->profile(d_bgr, n, iters, cap, names, kernels, avg_ms, alg_bytes, macs); });
}

int rf_profile_compulsory_bytes(rf_handle h, int n, int cap, double *bytes) {
    if (!h) return RF_ERR_INVALID_ARG;
    return guarded(h, [&]() -> int { return h->eng->compulsory_bytes(n, cap, bytes); });
}

int rf_convert_model(const char *prototxt, const char *caffemodel, const char *int8_table, const char *out_rfw) {
    return guarded(nullptr, [&]() -> int {
        if (!prototxt || !caffemodel || !out_rfw) throw rf::ArgError("null path");
        rf::Model m = rf::load_prototxt(prototxt);
        rf::attach_caffemodel(m, caffemodel);
        if (int8_table && *int8_table) rf::attach_int8_table(m, int8_table);
        (void)rf::compile_plan(m);      // refuse to pack a graph the engine cannot run
        rf::save_rfw(m, out_rfw);
        return RF_OK;
    });
}

int rf_plan_cache_probe(const char *model_dir, const char *stem, int precision, const char *cache_path, size_t *image_bytes) {
    return guarded(nullptr, [&]() -> int {
        if (!model_dir) throw rf::ArgError("null argument");
        rf::EngineOptions eo;
        eo.precision = precision;
        if (stem && *stem) eo.model_stem = stem;
        if (cache_path && *cache_path) eo.plan_cache_path = cache_path;
        return rf::plan_cache_probe(model_dir, eo, image_bytes);
    });
}

int rf_plan_folded(const char *model_dir, const char *stem, const char *op, float *w, size_t cap_w, float *b,
                   size_t cap_b, int dims[4]) {
    return guarded(nullptr, [&]() -> int {
        if (!model_dir || !op) throw rf::ArgError("null argument");
        rf::Model m = rf::load_model_dir(model_dir, stem && *stem ? stem : "mnet-deconv-0517");
        rf::Plan p = rf::compile_plan(m);
        std::string name = op;
        const rf::FoldedConv *f = nullptr;
        auto idx = [&](const std::string &prefix, int limit) -> int {
            if (name.compare(0, prefix.size(), prefix) != 0) return -1;
            int i = std::atoi(name.c_str() + prefix.size());
            return i >= 0 && i < limit ? i : -1;
        };
        int i;
        // "dw<i>.eq" / "pw<i>.eq": block i as the fp16 engine packs it, after the per-channel depthwise equalisation (weights.h)
        rf::FoldedConv eq_dw, eq_pw;
        if (name.size() > 3 && name.compare(name.size() - 3, 3, ".eq") == 0) {
            const bool want_dw = name.compare(0, 2, "dw") == 0;
            name.resize(name.size() - 3);
            if ((i = idx(want_dw ? "dw" : "pw", 13)) < 0) throw rf::ArgError("unknown plan op '" + std::string(op) + "'");
            eq_dw = p.blocks[i].dw;
            eq_pw = p.blocks[i].pw;
            rf::WeightPack<rf::half_t>::equalize_depthwise(eq_dw, eq_pw);
            f = want_dw ? &eq_dw : &eq_pw;
        } else
        if (name == "conv0") f = &p.conv0;
        else if ((i = idx("dw", 13)) >= 0 && name.find('.') == std::string::npos) f = &p.blocks[i].dw;
        else if ((i = idx("pw", 13)) >= 0) f = &p.blocks[i].pw;
        else if ((i = idx("lateral", 3)) >= 0) f = &p.lateral[i];
        else if ((i = idx("aggr", 2)) >= 0) f = &p.aggr[i];
        else if ((i = idx("ssh", 3)) >= 0) {
            std::string tail = name.substr(name.find('.') == std::string::npos ? name.size() : name.find('.'));
            if (tail == ".a") f = &p.ssh[i].conv_a;
            else if (tail == ".b") f = &p.ssh[i].conv_b;
            else if (tail == ".c") f = &p.ssh[i].conv_c;
            else if (tail == ".head") f = &p.ssh[i].head;
        }
        // "stem2.<c0|c2|c3|c4|floor2|floor3>": the constants of the fp16 engine's first launch (stem2_kernel) that exist only inside the packed
        // image, read back from the image WeightPack<half_t>::pack emits: c0 = conv0 weights + the offset-folded MFMA bias; c2 = conv2 weights +
        // the bias centred by mu2; c3 = the equalised conv3 taps as the packed halves + its centred bias; c4 = the equalised conv4 weights + its
        // bias with W mu3 folded in; floor2 / floor3 = the per-channel floors -mu2 / -mu3 of the two DC-centred tiles (in w and in b)
        rf::FoldedConv s2;
        if (!f && name.compare(0, 6, "stem2.") == 0 && p.blocks.size() >= 2) {
            rf::WeightPack<rf::half_t> wp;
            wp.pack(p);                                // host only: nothing is uploaded
            const std::vector<unsigned char> &img = wp.arena_.host();
            auto floats = [&](size_t off, int n) { std::vector<float> v(n); memcpy(v.data(), img.data() + off, (size_t)n * 4); return v; };
            auto halves = [&](size_t off, int n) {
                std::vector<float> v(n);
                for (int j = 0; j < n; j++) { rf::half_t h; memcpy(&h, img.data() + off + 2 * (size_t)j, 2); v[j] = (float)h; }
                return v;
            };
            const std::string t = name.substr(6);
            rf::FoldedConv dwq = p.blocks[1].dw, pwq = p.blocks[1].pw;
            rf::WeightPack<rf::half_t>::equalize_depthwise(dwq, pwq);
            if (t == "c0") { s2 = p.conv0; s2.b = floats(wp.c0_b_mma_, 8); f = &s2; }
            else if (t == "c2") { s2 = p.blocks[0].pw; s2.b = floats(wp.stem2_c2_b_, 16); f = &s2; }
            else if (t == "c3") {
                s2 = dwq;
                const std::vector<float> taps = halves(wp.stem2_dw_.w, 9 * 16);          // [tap][channel]
                for (int ch = 0; ch < 16; ch++)
                    for (int tp = 0; tp < 9; tp++) s2.w[(size_t)ch * 9 + tp] = taps[(size_t)tp * 16 + ch];
                s2.b = floats(wp.stem2_dw_.b, 16);
                f = &s2;
            }
            else if (t == "c4") { s2 = pwq; s2.b = floats(wp.stem2_pw_.b, 32); f = &s2; }
            else if (t == "floor2" || t == "floor3") {
                s2.cout = 16; s2.cin = 1; s2.k = 1; s2.group = 1;
                s2.w = halves(t == "floor2" ? wp.stem2_c2_floor_ : wp.stem2_c3_floor_, 16);
                s2.b = s2.w;
                f = &s2;
            }
        }
        if (!f) throw rf::ArgError("unknown plan op '" + name + "'");
        if (dims) { dims[0] = f->cout; dims[1] = f->k; dims[2] = f->k; dims[3] = f->cin / f->group; }
        if (w) { if (cap_w < f->w.size()) throw rf::ArgError("w too small"); memcpy(w, f->w.data(), f->w.size() * 4); }
        if (b) { if (cap_b < f->b.size()) throw rf::ArgError("b too small"); memcpy(b, f->b.data(), f->b.size() * 4); }
        return RF_OK;
    });
}

int rf_attach_calibration(const char *model_dir, const char *stem, const char *int8_table, const char *qweights, const char *out_rfw) {
    return guarded(nullptr, [&]() -> int {
        if (!model_dir || !out_rfw) throw rf::ArgError("null argument");
        rf::Model m = rf::load_model_dir(model_dir, stem && *stem ? stem : "mnet-deconv-0517");
        if (int8_table && *int8_table) {
            rf::attach_int8_table(m, int8_table);
            m.int8_qweights.clear();                   // calibrated weights belong to the table they were chosen under
        }
        if (qweights && *qweights) rf::attach_int8_qweights(m, qweights);
        rf::Plan p = rf::compile_plan(m);              // refuses a model the engine could not run
        if (!m.int8_scales.empty()) {
            rf::WeightPack<int8_t> wp;
            wp.pack(p);                                // ... and a table / weight file that does not fit it (missing tensors, wrong shapes)
        }
        rf::save_rfw(m, out_rfw);
        return RF_OK;
    });
}

int rf_plan_int8_gemm(const char *model_dir, const char *stem, const char *int8_table, const char *op, float *quanta, size_t cap_q,
                      float *in_scale, size_t cap_in, float *row_scale, float *out_scale, size_t cap_out, int dims[4]) {
    return guarded(nullptr, [&]() -> int {
        if (!model_dir || !op) throw rf::ArgError("null argument");
        rf::Model m = rf::load_model_dir(model_dir, stem && *stem ? stem : "mnet-deconv-0517");
        if (int8_table && *int8_table) rf::attach_int8_table(m, int8_table);
        m.int8_qweights.clear();                       // the grid and the unrounded quanta do not depend on an earlier calibration
        rf::Plan p = rf::compile_plan(m);
        rf::WeightPack<int8_t> wp;
        std::map<std::string, rf::WeightPack<int8_t>::GemmRecord> rec;
        wp.record_ = &rec;
        wp.pack(p);                                    // host only: nothing is uploaded
        auto it = rec.find(op);
        if (it == rec.end()) {
            // "?<i>": enumerate -- the i-th fused dense conv's name is returned through `dims` as its length and (when quanta != NULL) its bytes
            if (op[0] == '?') {
                size_t i = (size_t)std::atoi(op + 1);
                if (i >= rec.size()) return RF_ERR_INVALID_ARG;
                auto jt = rec.begin();
                std::advance(jt, (long)i);
                if (dims) dims[0] = (int)jt->first.size();
                if (quanta) { if (cap_q * 4 < jt->first.size()) throw rf::ArgError("name buffer too small"); memcpy(quanta, jt->first.data(), jt->first.size()); }
                return RF_OK;
            }
            throw rf::ArgError("the int8 plan has no fused dense conv '" + std::string(op) + "'");
        }
        const auto &r = it->second;
        if (dims) { dims[0] = r.cout; dims[1] = r.ktot; dims[2] = r.cin; dims[3] = r.in_u8; }
        if (quanta) { if (cap_q < r.quanta.size()) throw rf::ArgError("quanta too small"); memcpy(quanta, r.quanta.data(), r.quanta.size() * 4); }
        if (in_scale) { if (cap_in < r.in_scale.size()) throw rf::ArgError("in_scale too small"); memcpy(in_scale, r.in_scale.data(), r.in_scale.size() * 4); }
        if (row_scale) { if (cap_out < r.row_scale.size()) throw rf::ArgError("row_scale too small"); memcpy(row_scale, r.row_scale.data(), r.row_scale.size() * 4); }
        if (out_scale) { if (cap_out < r.out_scale.size()) throw rf::ArgError("out_scale too small"); memcpy(out_scale, r.out_scale.data(), r.out_scale.size() * 4); }
        return RF_OK;
    });
}

}  // extern "C"
