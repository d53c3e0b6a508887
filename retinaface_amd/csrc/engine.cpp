// engine.cpp -- see engine.h.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <thread>

#include "copier.h"
#include "knobs.h"
#include "net.h"
#include "pack.h"
#include "residency.h"
#include "staging.h"

namespace rf {

#define RF_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            throw HipError(std::string(#expr) + " failed: " + hipGetErrorString(e_));                  \
    } while (0)

namespace {

// RF_HOST_TRACE=1 (probe): where the HOST time of a call goes -- per-stage wall-clock sums, printed when the engine is destroyed
struct HostTrace {
    bool on = knob(K_HOST_TRACE) != 0;
    double sum[8] = {};
    long n[8] = {};
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void add(int k, double t0) { if (on) { sum[k] += now() - t0; n[k]++; } }
    void report(const char *tag) const {
        if (!on) return;
        static const char *names[8] = {"detect() total", "submit: checks + table fill", "launch: table H2D enqueue", "launch: graph / kernel launches",
                                       "launch: event record", "harvest: event synchronize", "harvest: copy records", "wait: copy out"};
        for (int k = 0; k < 8; k++)
            if (n[k]) fprintf(stderr, "[rf host trace %s] %-32s %9.2f us avg over %ld\n", tag, names[k], sum[k] / n[k], n[k]);
    }
};

// The HIP current device is per host thread and defaults to 0: every entry point binds the calling thread to the engine's
// device for the duration of the call and puts the caller's device back (rf_options.device may differ from it, and the
// caller may use another thread per call -- the header only promises one caller thread AT A TIME).
class DeviceGuard {
public:
    explicit DeviceGuard(int dev) : dev_(dev) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = dev;
        if (prev_ != dev_) (void)hipSetDevice(dev_);
        bind_launch_device(dev_);
    }
    ~DeviceGuard() {
        if (prev_ != dev_) { (void)hipSetDevice(prev_); bind_launch_device(prev_); }
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
private:
    int dev_, prev_ = 0;
};

// one base anchor of generate_anchors(base_size 16, ratios {.., ratio, ..}, scales {.., scale, ..}) -- RetinaFace.cpp:9-103, with
// the reference's float / double rounding points (`0.5 * (w - 1)` is double arithmetic stored to float; sqrt / round on floats)
void base_anchor(int scale, float ratio, float out[4]) {
    float w = 15.f - 0.f + 1, h = 15.f - 0.f + 1;                                   // _whctrs of (0, 0, 15, 15)
    float xc = 0.f + 0.5 * (w - 1), yc = 0.f + 0.5 * (h - 1);
    float size = w * h, sc = size / ratio;                                          // _ratio_enum, :34-51
    float w2 = std::round(std::sqrt(sc)), h2 = std::round(w2 * ratio);
    float rx1 = xc - 0.5 * (w2 - 1), ry1 = yc - 0.5 * (h2 - 1), rx2 = xc + 0.5 * (w2 - 1), ry2 = yc + 0.5 * (h2 - 1);
    w = rx2 - rx1 + 1; h = ry2 - ry1 + 1;                                           // _scale_enum, :53-68
    xc = rx1 + 0.5 * (w - 1); yc = ry1 + 0.5 * (h - 1);
    w = w * scale; h = h * scale;
    out[0] = xc - 0.5 * (w - 1); out[1] = yc - 0.5 * (h - 1);
    out[2] = xc + 0.5 * (w - 1); out[3] = yc + 0.5 * (h - 1);
}

}  // namespace

// The reference constructor's `network` presets (RetinaFace.cpp:209-271).  Only fmc == 3 presets get an anchor configuration
// (strides 32 / 16 / 8, scales {32,16} {8,4} {2,1}, base 16) and only "net3" / "net3a" give it ratios: "ssh" / "vgg" set pixel
// means that are never applied and leave `_ratio` empty, net4 / net5 / net5a / net6 print "please reconfig anchor_cfg", any
// other name prints "network setting error" -- all of those construct fine and then find no faces, because post-processing
// loops over zero anchors.  Returns false for names the reference does not know (its behaviour is the same as for "ssh").
bool network_preset(const std::string &network, std::vector<float> *ratios) {
    ratios->clear();
    if (network == "net3") { *ratios = {1.0f}; return true; }
    if (network == "net3a") { *ratios = {1.0f, 1.5f}; return true; }
    for (const char *k : {"ssh", "vgg", "net4", "net5", "net5a", "net6"})
        if (network == k) return true;
    return false;
}

void preset_base_anchors(const std::vector<float> &ratios, int level, float out[][4]) {
    static const int scales[3][2] = {{32, 16}, {8, 4}, {2, 1}};
    int a = 0;
    for (float r : ratios)                              // generate_anchors: ratios outer, scales inner (:86-91)
        for (int s = 0; s < 2; s++) base_anchor(scales[level][s], r, out[a++]);
}

namespace {

// One lane = one independent copy of everything a batch touches while in flight: stream(s), activation buffers,
// candidate buffers, pinned host descriptor / result blocks and the captured hipGraphs.  Batches on different
// lanes overlap on the GPU (most kernels of a batch-8 pass fill only a fraction of the 256 CUs); weights are shared.
constexpr int kMaxCoalesce = 256;       // enqueues merged into one launch: a batch-1 caller still fills a 256-image super-batch

// Everything the engine knows about its element type (filled by make_engine<T>): the scheduler, staging and result paths are the
// same code for fp32, fp16 and int8.
struct NetKind {
    size_t elem_bytes = 0;
    const char *tag = "";                                          // RF_HOST_TRACE report
    bool cvt_selfcheck = false;                                    // int8: the requantising epilogues' rounding probe runs at create
    void (*to_float)(const void *raw, size_t n, float *dst) = nullptr;      // stored elements -> float (debug_activation)
    Arena *arena = nullptr;                                        // the weight image of the pack that build_net's closure owns
    int head_a = 2;                                                // anchors per cell the model's heads carry
    std::function<void(const Plan &, const NetSite &, LaneNet *)> build_net;
};

// The open pass call: tiled, TTA, pyramid, rotation, fisheye and region detection turn a call's frames into passes that go through detect()'s ordinary
// launches, in call order, so image i of a launch is pass next_pass + i.  What differs between the modes is bound when the call is
// opened (the two callables); the launch path (launch_lane_passes) does not know which mode it serves.
constexpr size_t kPassEntryMax = std::max(std::max(std::max(sizeof(TileEntry), sizeof(TtaEntry)), std::max(sizeof(PyrEntry), sizeof(RotEntry))), sizeof(DewarpEntry));
static_assert(sizeof(RoiEntry) <= kPassEntryMax, "a region pass is no larger than the largest pass entry: its cell records travel in a block of their own");
struct PassCall {
    // gather(stream, faces, face_stride, counts, table, n): the mode's gather over the n passes of one launch (table: their entries)
    using Gather = std::function<void(hipStream_t, const uint8_t *, int, const int *, const void *, int)>;
    // merge(stream, d_params): the call's merge, behind the gather of its last launch
    using Merge = std::function<void(hipStream_t, const RunParams *)>;
    bool on = false;
    const char *name = "";                // the mode, as the two error messages spell it
    std::vector<uint8_t> table;           // the call's pass table: `total` entries of entry_bytes
    size_t entry_bytes = 0;
    int total = 0, next_pass = 0;
    std::vector<int> lanes_used;          // lanes that carried a launch of the call other than its last
    hipEvent_t inputs_ready = nullptr;    // recorded behind the side-stream copies the call's launches read; null: the call made none.
                                          // Every launch waits for it, pass call or not (detect_enhanced() sets it with `on` false)
    Gather gather;
    Merge merge;
};

class EngineImpl final : public Engine {
public:
    // `plan` may be a skeleton (no weights): everything weight-related comes packed in the WeightPack behind `kind` (built from
    // the model or read from the plan cache, weights.h)
    EngineImpl(const Plan &plan, NetKind kind, float nms, const EngineOptions &opt, const std::vector<float> &ratios)
        : kind_(std::move(kind)) {
        opt_ = opt;
        nms_threshold_ = nms;
        ratios_ = ratios;
        na_ = 2 * (int)ratios.size();              // anchors per cell: 2 scales x the preset's ratios; 0 = nothing to decode
        net_h_ = opt.net_h > 0 ? opt.net_h : plan.net_h;
        net_w_ = opt.net_w > 0 ? opt.net_w : plan.net_w;
        if (net_h_ <= 0 || net_w_ <= 0 || net_h_ % 32 || net_w_ % 32)
            throw ArgError("network input size must be a positive multiple of 32 (got " + std::to_string(net_h_) + "x" +
                           std::to_string(net_w_) + ")");
        if (opt_.max_batch < 1) throw ArgError("max_batch must be >= 1");
        int mc = opt_.max_candidates;
        if (mc < 64 || mc > 4096 || (mc & (mc - 1))) throw ArgError("max_candidates must be a power of two in [64, 4096]");
        if (opt_.max_detections < 1 || opt_.max_detections > 4096) throw ArgError("max_detections must be in [1, 4096]");
        if (opt_.lanes < 1 || opt_.lanes > 16) throw ArgError("lanes must be in [1, 16]");
        // default super-batch: ~256 images of 448 x 448 worth of pixels per launch whatever the batch size (measured: 8 x 32 and 32 x 8 beat 8 x 16 / 32 x 4 by
        // 2-4 %; every persistent kernel then has several tiles per resident workgroup)
        if (opt_.coalesce == 0)
            opt_.coalesce = (int)std::max<long>(1, std::min<long>(kMaxCoalesce, 256L * 448 * 448 / ((long)std::max(opt_.max_batch, 1) * net_h_ * net_w_)));
        if (opt_.coalesce < 1 || opt_.coalesce > kMaxCoalesce) throw ArgError("coalesce must be in [1, 256]");
        if (opt_.copy_threads < 0 || opt_.copy_threads > 64) throw ArgError("copy_threads must be in [0, 64]");
        cap_images_ = opt_.max_batch * opt_.coalesce;
        // every lane owns activation buffers for a full super-batch (~13 MB per 448 x 448 image in fp16): refuse sizes that can only
        // end in an out-of-memory error three allocations later
        if ((long)cap_images_ * net_h_ * net_w_ > 2048L * 448 * 448)
            throw ArgError("max_batch x coalesce = " + std::to_string(cap_images_) + " images per launch: more than 2048 images of 448 x 448 worth of pixels");
        tickets_.resize(4 * opt_.lanes * opt_.coalesce + 8);
        if (opt_.device >= 0) device_ = opt_.device;
        else RF_HIP(hipGetDevice(&device_));
        int ndev = 0;
        RF_HIP(hipGetDeviceCount(&ndev));
        if (device_ < 0 || device_ >= ndev) throw ArgError("device ordinal " + std::to_string(device_) + " out of range (" + std::to_string(ndev) + " devices)");
        if (device_ >= kMaxDevices) throw ArgError("device ordinal " + std::to_string(device_) + ": at most " + std::to_string(kMaxDevices) + " devices per process");
        // device frames are checked for residency whenever another device exists they could live on (RF_FORCE_SCATTER: test knob,
        // treats every device frame as foreign so the scatter path runs on a one-GPU box)
        force_scatter_ = knob(K_FORCE_SCATTER) != 0;
        scatter_per_frame_ = knob(K_SCATTER_PER_FRAME) != 0;
        stage_pieces_ = knob(K_SYNC_SPLIT) == 0 ? 1 : knob(K_SYNC_PIECES);      // RF_SYNC_PIECES: measurement knob of the A/B
        check_residency_ = ndev > 1 || force_scatter_;
        DeviceGuard guard(device_);                  // the caller's current device is put back when construction ends
        if (kind_.cvt_selfcheck) {
            const int chk = cvt_pk_u8_selfcheck();
            if (chk < 0) throw HipError("int8: the v_cvt_pk_u8_f32 rounding probe could not run on this device (allocation, launch or copy failed)");
            if (chk > 0) throw Unsupported("int8: v_cvt_pk_u8_f32 on this device does not round to nearest even / saturate as the requantising epilogues assume");
        }
        try { kind_.arena->upload(); } catch (const std::exception &e) { throw HipError(e.what()); }
        // Lanes are built on first use: a caller that only makes synchronous calls of <= max_batch images keeps re-using lane 0 and
        // never pays for the other lanes' activation buffers (~13 MB per 448 x 448 image in fp16 x the super-batch size).  Lane 0
        // is built now; if its buffers do not fit the device (a small or shared GPU) the super-batch is halved until they do.
        plan_ = plan;
        for (auto *f : {&plan_.conv0, &plan_.lateral[0], &plan_.lateral[1], &plan_.lateral[2], &plan_.aggr[0], &plan_.aggr[1]}) { f->w.clear(); f->w.shrink_to_fit(); }
        lanes_.resize(opt_.lanes);
        for (;;) {
            try { ensure_lane(0); break; }
            catch (const HipError &) {
                if (opt_.coalesce == 1) throw;
                opt_.coalesce = std::max(1, opt_.coalesce / 2);
                cap_images_ = opt_.max_batch * opt_.coalesce;
            }
        }
        // RF_PREBUILD_LANES=1: build every lane now (allocation, first eager run and graph capture happen at create time instead of
        // in the middle of the asynchronous steady state: one latency spike per lane less for latency-sensitive callers).  A lane
        // that does not fit is dropped, as on first use.  num_slots() may therefore be smaller than lanes x coalesce: callers read it
        // after rf_create, and again if an enqueue ever fails with RF_ERR_HIP.
        if (knob(K_PREBUILD_LANES)) {
            for (int l = 1; l < (int)lanes_.size(); l++) {
                try { ensure_lane(l); }
                catch (const HipError &) { lanes_.resize(l); break; }
            }
        }
        const int hw = (int)std::thread::hardware_concurrency();
        const int helpers = opt_.copy_threads > 0 ? opt_.copy_threads - 1 : std::max(0, std::min(8, hw / 4) - 1);
        copier_.reset(new ParallelCopier(helpers, true));       // non-temporal stores into the staging block
    }

    ~EngineImpl() override {
        DeviceGuard guard(device_);
        trace_.report(kind_.tag);
        for (auto &r : registered_) if (r.owned) (void)hipHostUnregister((void *)r.base);
        for (auto &l : lanes_) free_lane(l);
        for (void *p : dev_allocs_) (void)hipFree(p);
        for (void *p : host_allocs_) (void)hipHostFree(p);
        if (align_stream_) { (void)hipStreamSynchronize(align_stream_); (void)hipStreamDestroy(align_stream_); }
        for (DeviceScratch *b : {&align_crops_, &align_mats_, &align_tab_, &fb_state_, &fq_records_, &fq_packed_, &fq_offsets_, &tile_cand_, &tile_count_, &tile_out_,
                                 &tile_outcount_, &tile_tab_, &pass_frames_, &tta_cand_, &tta_count_, &tta_mirror_, &pyr_zoom_, &rot_copies_, &dewarp_views_, &roi_cells_, &roi_views_, &enh_luts_, &enh_frames_,
                                 &red_regions_, &red_counts_, &red_cells_, &red_frames_, &red_shadow_, &fol_results_}) b->release();
        for (HostScratch *b : {&trk_tags_, &trk_ended_, &trk_counts_, &enh_counts_, &roi_cells_pin_, &tta_out_, &tta_votes_, &tta_outcount_, &shot_out_, &shot_info_, &fol_out_}) b->release();
        for (auto &t : trackers_) t->release();
        for (auto &d : dewarpers_) d->mesh.release();
        for (auto &c : changers_) c->release();
        for (hipEvent_t e : trk_ev_) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : shot_ev_) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : fol_ev_) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : red_ev_) if (e) (void)hipEventDestroy(e);
        if (inputs_ready_) (void)hipEventDestroy(inputs_ready_);
        if (caller_ready_) (void)hipEventDestroy(caller_ready_);
        kind_.arena->release();
        for (auto &e : prof_ev_) (void)hipEventDestroy(e);
    }

    // ------------------------------------------------------------------------------------------ API
    void detect(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts))) throw ArgError("null argument");
        if (cap_per_image < 0 || (cap_per_image > 0 && !out)) throw ArgError("out is null");
        DeviceGuard guard(device_);
        const double t_detect = trace_.on ? HostTrace::now() : 0.0;
        struct AtExit { HostTrace &t; double t0; ~AtExit() { t.add(0, t0); } } at_exit{trace_, t_detect};
        *truncated = false;
        // every frame is checked before the first chunk is launched: a bad frame in a later chunk must not leave earlier
        // chunks in flight with nobody waiting for them
        for (int i = 0; i < n; i++) check_frame(frames[i], rows[i], cols[i], steps ? steps[i] : cols[i] * 3);
        std::vector<int> all_cand;
        std::vector<std::vector<int32_t>> all_anchor;
        // a synchronous call keeps up to `lanes` chunks of max_batch images in flight and collects them in order
        std::vector<std::pair<int, int>> inflight;      // (ticket, base)
        auto collect = [&]() {
            int ticket = inflight.front().first, base = inflight.front().second;
            inflight.erase(inflight.begin());
            bool tr = false;
            wait_impl(ticket, out ? out + (size_t)base * cap_per_image : nullptr, cap_per_image, counts + base, &tr);
            *truncated = *truncated || tr;
            all_cand.insert(all_cand.end(), last_cand_counts_.begin(), last_cand_counts_.end());
            for (int i = 0; i < last_n_; i++) all_anchor.push_back(std::move(last_anchor_[i]));
        };
        const bool timed = !opt_.use_graph;             // the eager engine measures the pre / infer / post split
        // A call of MORE than max_batch images (round 5): its chunks are not launched one by one (eight dependent 32-image launch sequences for
        // a 256-image call: each latency-bound, 1.07 ms) but join super-batches like enqueued tickets do -- one launch sequence per
        // max_batch x coalesce images (0.8 ms for the same call); the last, partial one is launched by the first wait.
        const bool coalesce_chunks = !timed && n > opt_.max_batch && opt_.coalesce > 1;
        const int max_inflight = coalesce_chunks ? (int)lanes_.size() * opt_.coalesce : (int)lanes_.size();
        try {
            for (int base = 0; base < n; base += opt_.max_batch) {
                int m = std::min(opt_.max_batch, n - base);
                std::vector<int> st(m);
                for (int i = 0; i < m; i++) st[i] = steps ? steps[base + i] : cols[base + i] * 3;
                if ((int)inflight.size() >= max_inflight || (timed && !inflight.empty())) collect();      // (>=: pick_lane() may have dropped lanes that did not fit)
                int ticket = submit(frames + base, rows + base, cols + base, st.data(), m, on_device, threshold, !coalesce_chunks);
                inflight.emplace_back(ticket, base);
            }
            while (!inflight.empty()) collect();
        } catch (...) {
            // hand every ticket of this call back to the pool (results dropped) before the error leaves
            for (auto &tb : inflight) {
                try { bool tr = false; wait_impl(tb.first, nullptr, 0, nullptr, &tr); } catch (...) { tickets_[tb.first].state = Ticket::FREE; }
            }
            throw;
        }
        if (n > opt_.max_batch) last_first_image_ = -1000000;   // blob accessors are per-launch: not valid for chunked calls
        last_n_ = n;                         // the "most recent completed batch" of a chunked call is the whole call
        last_cand_counts_.swap(all_cand);
        last_anchor_.swap(all_anchor);
    }

    int enqueue(const void *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                float threshold) override {
        if (n < 1 || n > opt_.max_batch) throw ArgError("enqueue: n must be in [1, max_batch]");
        if (!frames || !rows || !cols) throw ArgError("null argument");
        DeviceGuard guard(device_);
        std::vector<int> st(n);
        for (int i = 0; i < n; i++) {
            st[i] = steps ? steps[i] : cols[i] * 3;
            check_frame((const uint8_t *)frames[i], rows[i], cols[i], st[i]);
        }
        return submit((const uint8_t *const *)frames, rows, cols, st.data(), n, on_device, threshold, false);
    }

    void wait(int ticket, rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        if (cap_per_image < 0 || (cap_per_image > 0 && !out)) throw ArgError("wait: out is null");
        DeviceGuard guard(device_);
        wait_impl(ticket, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- face alignment
    static void check_align_request(const AlignRequest &rq) {
        if (rq.crop < kAlignMinCrop || rq.crop > kAlignMaxCrop) throw ArgError("crop_size must be in [16, 512]");
        if (rq.max_faces < 1 || rq.max_faces > kAlignMaxFaces) throw ArgError("max_faces must be in [1, 4096]");
    }

    // device blocks of an alignment call over n images: the caller's crops or scratch for the host copy, scratch for the matrices
    void align_open(const AlignRequest &rq, int n, uint8_t **d_crops, double **d_mats) {
        *d_crops = rq.d_crops;
        if (!rq.d_crops && rq.crops) *d_crops = align_crops_.reserve((size_t)n * rq.max_faces * rq.crop * rq.crop * 3);
        *d_mats = rq.matrices ? (double *)align_mats_.reserve((size_t)n * rq.max_faces * 6 * sizeof(double)) : nullptr;
    }

    void align(const void *const *frames, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
               int cap_per_image, const int *counts, const float *coord_scale, const AlignRequest &rq) override {
        check_align_request(rq);
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts || !faces))) throw ArgError("null argument");
        if (cap_per_image < 1) throw ArgError("cap_per_image must be >= 1");
        if ((long)n * rq.max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 crop slots in one call");
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int fpi = std::min(cap_per_image, rq.max_faces);          // records per image that travel to the device
        // one table: frames | counts | scales | faces (60-byte records)
        HostTable tb;
        const size_t o_fd = tb.add((size_t)n * sizeof(FrameDesc)), o_cnt = tb.add((size_t)n * sizeof(int)), o_sc = tb.add((size_t)n * sizeof(float)),
                     o_face = tb.add((size_t)n * fpi * sizeof(rf_face));
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        float *sc = (float *)(tab + o_sc);
        const std::vector<char> empty = table_frames((FrameDesc *)(tab + o_fd), frames, rows, cols, steps, n, "align");
        for (int i = 0; i < n; i++) {
            cnt[i] = empty[i] ? 0 : std::max(0, std::min(counts[i], fpi));
            sc[i] = coord_scale ? coord_scale[i] : 1.f;
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        uint8_t *d_crops = nullptr;
        double *d_mats = nullptr;
        align_open(rq, n, &d_crops, &d_mats);
        if (!d_crops && !d_mats) return;
        table_upload(d_tab, tb);
        for (int base = 0; base < n; base += kAlignImagesPerLaunch) {
            AlignParams ap;
            ap.frames = (const FrameDesc *)(d_tab + o_fd) + base;
            ap.faces = d_tab + o_face + (size_t)base * fpi * sizeof(rf_face);
            ap.face_stride = (int)sizeof(rf_face); ap.faces_per_image = fpi;
            ap.counts = (const int *)(d_tab + o_cnt) + base;
            ap.scale = (const float *)(d_tab + o_sc) + base;
            ap.n = std::min(kAlignImagesPerLaunch, n - base); ap.max_faces = rq.max_faces; ap.crop = rq.crop;
            ap.first_image = base;
            ap.crops = d_crops; ap.mats = d_mats;
            launch_align(align_stream_, ap);
        }
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
        align_copy_out(rq, d_crops, d_mats, n, cnt, rq.max_faces);
    }

    // -------------------------------------------------------------------------------- face batches
    static void check_face_batch_request(const FaceBatchRequest &rq) {
        const FaceBatchSpec &sp = rq.spec;
        if (sp.crop < kAlignMinCrop || sp.crop > kAlignMaxCrop) throw ArgError("crop_size must be in [16, 512]");
        if (sp.max_faces < 1 || sp.max_faces > kAlignMaxFaces) throw ArgError("max_faces must be in [1, 4096]");
        if (sp.capacity < 1) throw ArgError("capacity must be >= 1");
        if (rq.d_tensor && ((uintptr_t)rq.d_tensor & (uintptr_t)(sp.elem_bytes() - 1))) throw ArgError("d_tensor is not aligned to its element size");
    }

    // device blocks of a face-batch call: the caller's tensor or scratch for the host copy, scratch for the matrices
    void face_batch_open(const FaceBatchRequest &rq, uint8_t **d_tensor, double **d_mats) {
        const size_t cap = (size_t)rq.spec.capacity;
        *d_tensor = rq.d_tensor;
        if (!rq.d_tensor && rq.tensor) *d_tensor = align_crops_.reserve(cap * rq.spec.bytes_per_face());
        *d_mats = rq.matrices ? (double *)align_mats_.reserve(cap * 6 * sizeof(double)) : nullptr;
        if (!fb_state_.ptr) RF_HIP(hipMemset(fb_state_.reserve(256), 0, 256));
    }

    // device blocks of a gated call: quality records and packed indices per face slot, the call's packed offsets
    void face_gate_open(const FaceBatchRequest &rq, int n) {
        const size_t slots = (size_t)std::max(n, 1) * rq.spec.max_faces;
        fq_records_.reserve(slots * sizeof(rf_face_quality));
        fq_packed_.reserve(slots * sizeof(int));
        fq_offsets_.reserve(((size_t)n + 1) * sizeof(int));
    }

    // results of a finished gated call: the device's offsets (the host cannot derive them from counts), the packed faces that exist,
    // the records of the considered slots (counts[i] clamped to limit).  A record block that is small or at least half
    // considered travels as one copy instead of one per image.
    void face_gated_copy_out(const FaceBatchRequest &rq, const uint8_t *d_tensor, const double *d_mats, const int *counts, int n, int limit,
                             bool *overflow) {
        std::vector<int> off((size_t)n + 1, 0);
        if (n > 0) RF_HIP(hipMemcpy(off.data(), fq_offsets_.ptr, off.size() * sizeof(int), hipMemcpyDeviceToHost));
        if (rq.offsets) memcpy(rq.offsets, off.data(), off.size() * sizeof(int));
        const long total = off[n];
        const size_t written = (size_t)std::min<long>(total, rq.spec.capacity);
        *overflow = total > rq.spec.capacity;
        if (written) {
            if (rq.tensor && d_tensor) RF_HIP(hipMemcpy(rq.tensor, d_tensor, written * rq.spec.bytes_per_face(), hipMemcpyDeviceToHost));
            if (rq.matrices && d_mats) RF_HIP(hipMemcpy(rq.matrices, d_mats, written * 6 * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (!rq.quality || n == 0) return;
        const size_t mf = (size_t)rq.spec.max_faces, all = (size_t)n * mf;
        size_t considered = 0;
        for (int i = 0; i < n; i++) considered += (size_t)std::max(0, std::min(counts[i], limit));
        if (!considered) return;
        const rf_face_quality *d_rec = (const rf_face_quality *)fq_records_.ptr;
        if (all * sizeof(rf_face_quality) <= (1u << 20) || considered * 2 >= all) {
            RF_HIP(hipMemcpy(rq.quality, d_rec, all * sizeof(rf_face_quality), hipMemcpyDeviceToHost));
            return;
        }
        for (int i = 0; i < n; i++) {
            const int m = std::max(0, std::min(counts[i], limit));
            if (m) RF_HIP(hipMemcpy(rq.quality + i * mf, d_rec + i * mf, (size_t)m * sizeof(rf_face_quality), hipMemcpyDeviceToHost));
        }
    }

    // results of a finished face-batch call to the caller's host buffers: the packed faces that exist, nothing behind them
    void face_batch_copy_out(const FaceBatchRequest &rq, const uint8_t *d_tensor, const double *d_mats, const int *counts, int n, int limit,
                             bool *overflow) {
        std::vector<int> off((size_t)n + 1, 0);
        const long total = face_batch_offsets(counts, n, limit, off.data());
        if (rq.offsets) memcpy(rq.offsets, off.data(), off.size() * sizeof(int));
        const size_t written = (size_t)std::min<long>(total, rq.spec.capacity);
        *overflow = total > rq.spec.capacity;
        if (!written) return;
        if (rq.tensor && d_tensor) RF_HIP(hipMemcpy(rq.tensor, d_tensor, written * rq.spec.bytes_per_face(), hipMemcpyDeviceToHost));
        if (rq.matrices && d_mats) RF_HIP(hipMemcpy(rq.matrices, d_mats, written * 6 * sizeof(double), hipMemcpyDeviceToHost));
    }

    // The face-batch launches over n images of ONE table of faces, in stream order: (gated: the quality kernel,) the scan that packs
    // the counts and advances the call's running base, the tensor kernel.  Shared by the standalone call, the launches behind a
    // detection launch and the fused tiled call: they differ only in where frames, faces, counts and scales live.
    struct FaceSeq {
        const FrameDesc *frames; const uint8_t *faces; int face_stride, faces_per_image;
        const int *counts; const float *scale;           // scale: nullptr = 1
        int n, image0;                                   // images of this launch; index of its first image in the call (records / packed / gated offsets)
        bool first;                                      // the call's first launch
        int *offsets;                                    // [n + 1] device ints the scan writes
        hipEvent_t wait_before_scan = nullptr;           // the scan of the call's previous launch, on another stream
        hipEvent_t record_after_scan = nullptr;
    };
    void launch_face_seq(hipStream_t st, const FaceBatchRequest &rq, const FaceSeq &q, uint8_t *d_tensor, double *d_mats) {
        const FaceBatchSpec &spec = rq.spec;
        const int *packed = nullptr;
        if (rq.gated) {
            // quality kernel first: it needs nothing of the call's earlier launches and runs while their scans finish
            const size_t slot0 = (size_t)q.image0 * spec.max_faces;
            FaceQualityParams qp;
            qp.frames = q.frames;
            qp.faces = q.faces;
            qp.face_stride = q.face_stride; qp.faces_per_image = q.faces_per_image;
            qp.counts = q.counts;
            qp.scale = q.scale;
            qp.n = q.n; qp.max_faces = spec.max_faces; qp.crop = spec.crop;
            qp.aa_max = spec.antialias ? spec.aa_max : 0;
            qp.has_gate = rq.has_gate ? 1 : 0; qp.gate = rq.gate;
            qp.records = (rf_face_quality *)fq_records_.ptr + slot0;
            launch_face_quality(st, qp);
            if (q.wait_before_scan) RF_HIP(hipStreamWaitEvent(st, q.wait_before_scan, 0));
            FaceGateScanParams gp;
            gp.frames = q.frames; gp.counts = q.counts;
            gp.n = q.n; gp.faces_per_image = q.faces_per_image; gp.max_faces = spec.max_faces;
            gp.records = qp.records;
            gp.running = (int *)fb_state_.ptr; gp.first = q.first;
            gp.offsets = q.offsets;
            gp.packed = (int *)fq_packed_.ptr + slot0;
            launch_face_gate_scan(st, gp);
            packed = gp.packed;
        } else {
            if (q.wait_before_scan) RF_HIP(hipStreamWaitEvent(st, q.wait_before_scan, 0));
            FaceScanParams sp;
            sp.frames = q.frames;
            sp.counts = q.counts;
            sp.n = q.n; sp.faces_per_image = q.faces_per_image; sp.max_faces = spec.max_faces;
            sp.running = (int *)fb_state_.ptr; sp.first = q.first;
            sp.offsets = q.offsets;
            launch_face_scan(st, sp);
        }
        if (q.record_after_scan) RF_HIP(hipEventRecord(q.record_after_scan, st));
        if (!d_tensor && !d_mats) return;
        FaceBatchParams bp;
        bp.frames = q.frames;
        bp.faces = q.faces;
        bp.face_stride = q.face_stride; bp.faces_per_image = q.faces_per_image;
        bp.scale = q.scale;
        bp.offsets = q.offsets; bp.packed = packed;
        bp.n = q.n; bp.max_faces = spec.max_faces;
        bp.spec = spec;
        bp.tensor = d_tensor; bp.mats = d_mats;
        launch_face_batch(st, bp);
    }

    void face_batch(const void *const *frames, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces,
                    int cap_per_image, const int *counts, const float *coord_scale, const FaceBatchRequest &rq, bool *overflow) override {
        check_face_batch_request(rq);
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts || !faces))) throw ArgError("null argument");
        if (cap_per_image < 1) throw ArgError("cap_per_image must be >= 1");
        if ((long)n * rq.spec.max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 faces in one call");
        for (int i = 0; i < n; i++)
            if (counts[i] < 0) throw ArgError("negative face count");
        *overflow = false;
        if (n == 0) { if (rq.offsets) rq.offsets[0] = 0; return; }
        DeviceGuard guard(device_);
        if (rq.gated) face_gate_open(rq, n);
        const int fpi = std::min(cap_per_image, rq.spec.max_faces);     // records per image that travel to the device
        // one table: frames | counts | scales | offsets (written by the scan) | faces (60-byte records)
        const int per = std::min(n, kAlignImagesPerLaunch);
        HostTable tb;
        const size_t o_fd = tb.add((size_t)n * sizeof(FrameDesc)), o_cnt = tb.add((size_t)n * sizeof(int)), o_sc = tb.add((size_t)n * sizeof(float)),
                     o_off = tb.add(((size_t)per + 1) * sizeof(int)), o_face = tb.add((size_t)n * fpi * sizeof(rf_face));
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        float *sc = (float *)(tab + o_sc);
        const std::vector<char> empty = table_frames((FrameDesc *)(tab + o_fd), frames, rows, cols, steps, n, "face batch");
        for (int i = 0; i < n; i++) {
            cnt[i] = empty[i] ? 0 : std::min(counts[i], fpi);
            sc[i] = coord_scale ? coord_scale[i] : 1.f;
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        uint8_t *d_tensor = nullptr;
        double *d_mats = nullptr;
        face_batch_open(rq, &d_tensor, &d_mats);
        if (d_tensor || d_mats || rq.gated) {
            table_upload(d_tab, tb);
            // The caller's tensor: what the caller has pending on it on the default stream (a fill, say) comes first -- the side
            // stream does not wait for the default stream by itself, and a late fill would land on top of the tensor kernel's output.
            if (rq.d_tensor) {
                if (!caller_ready_) RF_HIP(hipEventCreateWithFlags(&caller_ready_, hipEventDisableTiming));
                RF_HIP(hipEventRecord(caller_ready_, nullptr));
                RF_HIP(hipStreamWaitEvent(align_stream_, caller_ready_, 0));
            }
            for (int base = 0; base < n; base += per) {          // one stream: the scans and the tensor launches run in order
                FaceSeq q;
                q.frames = (const FrameDesc *)(d_tab + o_fd) + base;
                q.faces = d_tab + o_face + (size_t)base * fpi * sizeof(rf_face);
                q.face_stride = (int)sizeof(rf_face); q.faces_per_image = fpi;
                q.counts = (const int *)(d_tab + o_cnt) + base;
                q.scale = (const float *)(d_tab + o_sc) + base;
                q.n = std::min(per, n - base); q.image0 = base;
                q.first = base == 0;
                q.offsets = rq.gated ? (int *)fq_offsets_.ptr + base : (int *)(d_tab + o_off);
                launch_face_seq(align_stream_, rq, q, d_tensor, d_mats);
            }
            RF_HIP(hipGetLastError());
            RF_HIP(hipStreamSynchronize(align_stream_));
        }
        if (rq.gated) face_gated_copy_out(rq, d_tensor, d_mats, cnt, n, rq.spec.max_faces, overflow);
        else face_batch_copy_out(rq, d_tensor, d_mats, cnt, n, rq.spec.max_faces, overflow);
    }

    // -------------------------------------------------------------------------------- pass calls
    // What tiled, TTA, pyramid, rotation and fisheye detection share (PassCall).  a..d: the arrays the entry point needs when n > 0.
    static void pass_check_args(int n, const void *a, const void *b, const void *c, const void *d, rf_face *out, int cap_per_image, int max_faces) {
        static_assert(kTileMaxFaces == 4096 && kTtaMaxFaces == 4096, "the message below names the bound");
        if (n < 0 || (n > 0 && (!a || !b || !c || !d))) throw ArgError("null argument");
        if (cap_per_image < 0 || (cap_per_image > 0 && !out)) throw ArgError("out is null");
        if (max_faces < 1 || max_faces > 4096) throw ArgError("max_faces must be in [1, 4096]");
    }

    // the row pitch of each frame of a call (default cols * 3), every frame checked
    std::vector<int> checked_steps(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n) const {
        std::vector<int> st((size_t)std::max(n, 1));
        for (int i = 0; i < n; i++) {
            st[i] = steps ? steps[i] : cols[i] * 3;
            check_frame(frames[i], rows[i], cols[i], st[i]);
        }
        return st;
    }

    // Where the passes of a call read frame i (null: not a live frame): the caller's device frame, or host frames uploaded once,
    // densely, each at a 256-byte-aligned offset of one block (st[i] becomes cols * 3).  One block serves the four modes: their calls
    // are synchronous and never overlap.
    template <class Live>
    std::vector<const uint8_t *> pass_frame_bases(const uint8_t *const *frames, const int *rows, const int *cols, std::vector<int> &st, int n,
                                                  bool on_device, Live live) {
        std::vector<const uint8_t *> base((size_t)n, nullptr);
        if (on_device) {
            for (int i = 0; i < n; i++) base[i] = live(i) ? frames[i] : nullptr;
            return base;
        }
        size_t bytes = 0;
        std::vector<size_t> off((size_t)n, 0);
        for (int i = 0; i < n; i++)
            if (live(i)) { off[i] = bytes; bytes += align256((size_t)rows[i] * cols[i] * 3); }
        uint8_t *d = pass_frames_.reserve(bytes);
        for (int i = 0; i < n; i++) {
            if (!live(i)) continue;
            RF_HIP(hipMemcpy2D(d + off[i], (size_t)cols[i] * 3, frames[i], (size_t)st[i], (size_t)cols[i] * 3, (size_t)rows[i], hipMemcpyHostToDevice));
            base[i] = d + off[i];
            st[i] = cols[i] * 3;
        }
        return base;
    }

    // the passes of a call as detect() takes them: views of the frames or of the copies made for the call (an empty pass stays null / 0)
    struct PassViews {
        std::vector<const uint8_t *> ptr;
        std::vector<int> rows, cols, step;
        explicit PassViews(int P) : ptr((size_t)P, nullptr), rows((size_t)P, 0), cols((size_t)P, 0), step((size_t)P, 0) {}
        void set(int q, const uint8_t *p, int r, int c, int s) { ptr[q] = p; rows[q] = r; cols[q] = c; step[q] = s; }
    };

    // the event behind the mirrored / zoomed / rotated / dewarped copies a call has just launched on the side stream (PassCall::inputs_ready)
    hipEvent_t record_inputs_ready() {
        if (!inputs_ready_) RF_HIP(hipEventCreateWithFlags(&inputs_ready_, hipEventDisableTiming));
        RF_HIP(hipGetLastError());
        RF_HIP(hipEventRecord(inputs_ready_, align_stream_));
        return inputs_ready_;
    }

    // the mode's gather into a candidate block set (cand, count: read when it runs, after the set has been opened)
    template <class Map, class Block> PassCall::Gather gather_into(int edge, const Block &cand, const Block &count, int cap) {
        return [this, edge, &cand, &count, cap](hipStream_t st, const uint8_t *faces, int face_stride, const int *counts, const void *table, int n) {
            PassGatherParams<typename Map::Entry> gp;
            gp.faces = faces; gp.face_stride = face_stride; gp.faces_per_pass = opt_.max_detections;
            gp.counts = counts; gp.table = (const typename Map::Entry *)table;
            gp.n = n; gp.edge = edge; gp.rank_stride = opt_.max_detections;
            gp.cand = (Candidate *)cand.ptr; gp.cand_count = (int *)count.ptr; gp.cap = cap;
            launch_pass_gather<Map>(st, gp);
        };
    }

    // Open a pass call and run it: a super-batch of earlier enqueues has been started (launch_pending()), so every launch detect()
    // makes now carries passes of this call only.  `dirty` is the flag of the block set the call gathers into: set until the call has
    // ended well, so that an error in between makes the next open zero the counters.  Returns detect()'s truncated.
    template <class Entry>
    bool run_passes(const char *name, const std::vector<Entry> &entries, const PassViews &v, float threshold, hipEvent_t inputs_ready,
                    PassCall::Gather gather, PassCall::Merge merge, bool &dirty) {
        const int P = (int)entries.size();
        passes_.name = name;
        passes_.table.assign((const uint8_t *)entries.data(), (const uint8_t *)(entries.data() + P));
        passes_.entry_bytes = sizeof(Entry);
        passes_.total = P; passes_.next_pass = 0;
        passes_.lanes_used.clear();
        passes_.inputs_ready = inputs_ready;
        passes_.gather = std::move(gather); passes_.merge = std::move(merge);
        passes_.on = true;
        dirty = true;
        struct Off { PassCall &c; ~Off() { c.on = false; c.inputs_ready = nullptr; } } off_guard{passes_};
        std::vector<int> pass_counts((size_t)P);
        bool tr = false;
        detect(v.ptr.data(), v.rows.data(), v.cols.data(), v.step.data(), P, true, threshold, nullptr, 0, pass_counts.data(), &tr);
        passes_.on = false;
        if (passes_.next_pass != P) throw HipError(std::string(name) + ": the merge was not launched");
        // every launch of the call has been waited for; the merge (and what it carries) ran in front of the last one's `done`
        dirty = false;
        return tr;
    }

    // The stand-alone merge of a mode: gather and merge over faces the caller brings, max_detections per pass.  One table -- run
    // parameters | pass table | counts | faces (60-byte records) -- crosses in one copy on the side stream, which the host waits for.
    // `open` opens the block set the gather writes, `dirty` is that set's flag (run_passes).
    template <class Entry, class Open>
    void merge_passes(const std::vector<Entry> &entries, int n, const rf_face *faces, const int *pass_counts, bool *truncated, Open open,
                      const PassCall::Gather &gather, const PassCall::Merge &merge, bool &dirty) {
        const int P = (int)entries.size(), md = opt_.max_detections;
        for (int p = 0; p < P; p++)
            if (pass_counts[p] < 0) throw ArgError("negative face count");
        const size_t o_tab = 256, o_cnt = o_tab + align256((size_t)P * sizeof(Entry)), o_face = o_cnt + align256((size_t)P * sizeof(int)),
                     total = o_face + (size_t)P * md * sizeof(rf_face);
        align_host_.assign(total, 0);
        *(RunParams *)align_host_.data() = RunParams{0.f, nms_threshold_, n, 0};
        memcpy(align_host_.data() + o_tab, entries.data(), (size_t)P * sizeof(Entry));
        int *cnt = (int *)(align_host_.data() + o_cnt);
        for (int p = 0; p < P; p++) {
            cnt[p] = std::min(pass_counts[p], md);
            if (pass_counts[p] > md) *truncated = true;
            if (cnt[p]) memcpy(align_host_.data() + o_face + (size_t)p * md * sizeof(rf_face), faces + (size_t)p * md, (size_t)cnt[p] * sizeof(rf_face));
        }
        uint8_t *d_tab = align_tab_.reserve(total);
        open();
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        dirty = true;
        RF_HIP(hipMemcpyAsync(d_tab, align_host_.data(), total, hipMemcpyHostToDevice, align_stream_));
        gather(align_stream_, d_tab + o_face, (int)sizeof(rf_face), (const int *)(d_tab + o_cnt), d_tab + o_tab, P);
        merge(align_stream_, (const RunParams *)d_tab);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
        dirty = false;
    }

    // -------------------------------------------------------------------------------- tiled detection
    // The plans of a call's frames as one pass table (frames in call order, passes in plan order); first[i]: frame i's first pass.
    // A NULL / empty frame is one pass that gathers nothing (frame = -1).  `have_ptrs` false: tile_merge(), which has no pixels.
    void tile_build_passes(const TileSpec &sp, const uint8_t *const *frames, bool have_ptrs, const int *rows, const int *cols, int n,
                           std::vector<TileEntry> *entries, std::vector<int> *first) const {
        entries->clear();
        first->assign((size_t)n + 1, 0);
        for (int i = 0; i < n; i++) {
            (*first)[i] = (int)entries->size();
            const bool empty = (have_ptrs && !frames[i]) || rows[i] <= 0 || cols[i] <= 0;
            if (empty) {
                TileEntry e;
                memset(&e, 0, sizeof(e));
                e.frame = -1; e.scale = 1.f;
                entries->push_back(e);
                continue;
            }
            if (rows[i] > 4096 * 3072 / cols[i]) throw ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
            int nx = 0, ny = 0, full = 0;
            const int passes = tile_plan_shape(sp, rows[i], cols[i], net_h_, net_w_, &nx, &ny, &full);
            if (passes < 0) throw ArgError("tiled detection: a frame's plan has more than 1024 passes");
            for (int t = 0; t < passes; t++) entries->push_back(tile_plan_entry(rows[i], cols[i], net_h_, net_w_, nx, ny, t, i));
        }
        (*first)[n] = (int)entries->size();
    }

    // device blocks of a tiled call, sized once and reused: per frame kTileMergeCap candidate records and their counter, max_faces
    // merged records, kept / candidate counts.  The counters are zero between calls (the merge re-arms them as the NMS kernel re-arms
    // the heads'); a new block, or a call that ended in an error, is zeroed here.
    void tile_open(int n, const TileSpec &sp) {
        const size_t nf = (size_t)std::max(n, 1);
        tile_cand_.reserve(nf * kTileMergeCap * sizeof(Candidate));
        const uint8_t *before = tile_count_.ptr;
        tile_count_.reserve(nf * sizeof(int));
        if (tile_count_.ptr != before) tile_dirty_ = true;
        tile_out_.reserve(nf * sp.max_faces * sizeof(Candidate));
        tile_outcount_.reserve(2 * nf * sizeof(int));
        if (tile_dirty_) {
            RF_HIP(hipDeviceSynchronize());
            RF_HIP(hipMemset(tile_count_.ptr, 0, tile_count_.cap));
            RF_HIP(hipDeviceSynchronize());
            tile_dirty_ = false;
        }
    }

    // the merge: the detector's own NMS kernel over the gathered candidates, one workgroup per frame (`anchor` holds g)
    void tile_launch_merge(hipStream_t st, int n, const TileSpec &sp, const RunParams *d_params) {
        NmsParams np;
        np.cand = (const Candidate *)tile_cand_.ptr; np.cand_count = (int *)tile_count_.ptr; np.cap = kTileMergeCap;
        np.params = d_params;
        np.out = (Candidate *)tile_out_.ptr; np.out_count = (int *)tile_outcount_.ptr; np.out_cand_count = (int *)tile_outcount_.ptr + n;
        np.max_det = sp.max_faces;
        np.n = n;
        launch_nms(st, np);
    }

    // results of a finished tiled call (the host has waited for its last launch): true counts, the first min(count, max_faces,
    // cap_per_image) faces of each frame, the pass each came from
    void tile_copy_out(int n, const TileRequest &rq, rf_face *out, int cap_per_image, int *counts, bool *truncated) {
        if (n == 0) return;
        std::vector<int> hc(2 * (size_t)n);
        RF_HIP(hipMemcpy(hc.data(), tile_outcount_.ptr, hc.size() * sizeof(int), hipMemcpyDeviceToHost));
        const int mf = rq.spec.max_faces;
        const size_t block = (size_t)n * mf;
        size_t used = 0;
        for (int i = 0; i < n; i++) {
            counts[i] = hc[i];
            if (hc[n + i] > kTileMergeCap || hc[i] > mf) *truncated = true;
            if (out && std::min(hc[i], mf) > cap_per_image) *truncated = true;
            used += (size_t)std::min(std::min(hc[i], mf), out ? cap_per_image : 0);
        }
        if (!used) return;
        const Candidate *d_out = (const Candidate *)tile_out_.ptr;
        const bool whole = block * sizeof(Candidate) <= (1u << 20) || 2 * used >= block;
        tile_host_.resize(block);
        if (whole) RF_HIP(hipMemcpy(tile_host_.data(), d_out, block * sizeof(Candidate), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            const int k = std::min(std::min(hc[i], mf), cap_per_image);
            if (k <= 0) continue;
            Candidate *src = tile_host_.data() + (size_t)i * mf;
            if (!whole) RF_HIP(hipMemcpy(src, d_out + (size_t)i * mf, (size_t)k * sizeof(Candidate), hipMemcpyDeviceToHost));
            for (int j = 0; j < k; j++) {
                memcpy(&out[(size_t)i * cap_per_image + j], &src[j], sizeof(rf_face));
                if (rq.src_tile) rq.src_tile[(size_t)i * cap_per_image + j] = src[j].anchor / opt_.max_detections;
            }
        }
    }

    void detect_tiled(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                      float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const TileRequest &rq,
                      bool *overflow) override {
        *truncated = false;
        *overflow = false;
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, rq.spec.max_faces);
        if (rq.fb) {
            check_face_batch_request(*rq.fb);
            if ((long)n * rq.fb->spec.max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 faces in one call");
        }
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        std::vector<TileEntry> entries;
        std::vector<int> first;
        tile_build_passes(rq.spec, frames, true, rows, cols, n, &entries, &first);
        if (n == 0) { if (rq.fb && rq.fb->offsets) rq.fb->offsets[0] = 0; return; }
        DeviceGuard guard(device_);
        // the passes are views of the frames (host frames: of their one dense copy)
        const std::vector<const uint8_t *> base =
            pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return entries[first[i]].frame >= 0; });
        PassViews v((int)entries.size());
        tile_fd_.assign((size_t)n, FrameDesc{nullptr, 0, 0, 0, 0});
        for (int i = 0; i < n; i++) {
            if (base[i]) tile_fd_[i] = FrameDesc{base[i], rows[i], cols[i], st[i], 0};
            for (int p = first[i]; p < first[i + 1]; p++) {
                const TileEntry &e = entries[p];
                if (e.frame >= 0) v.set(p, base[i] + (size_t)e.y0 * st[i] + (size_t)3 * e.x0, e.th, e.tw, st[i]);
            }
        }
        launch_pending();
        tile_open(n, rq.spec);
        uint8_t *d_tensor = nullptr;
        double *d_mats = nullptr;
        if (rq.fb) {
            face_batch_open(*rq.fb, &d_tensor, &d_mats);
            if (rq.fb->gated) face_gate_open(*rq.fb, n);
            fq_offsets_.reserve(((size_t)n + 1) * sizeof(int));
            // the frame table of those launches is known now: it is on the device before the call's first launch
            RF_HIP(hipMemcpy(tile_tab_.reserve((size_t)n * sizeof(FrameDesc)), tile_fd_.data(), (size_t)n * sizeof(FrameDesc), hipMemcpyHostToDevice));
        }
        // behind the merge, for the fused call, the face-batch launches over the merged faces
        const TileSpec sp = rq.spec;
        const FaceBatchRequest *fb = rq.fb;
        auto merge = [=](hipStream_t s, const RunParams *d_params) {
            tile_launch_merge(s, n, sp, d_params);
            if (fb) launch_tiled_face_batch(s, n, *fb, sp.max_faces, d_tensor, d_mats);
        };
        *truncated = run_passes("tiled detection", entries, v, threshold, nullptr,
                                gather_into<TileMap>(sp.edge, tile_cand_, tile_count_, kTileMergeCap), merge, tile_dirty_);
        tile_copy_out(n, rq, out, cap_per_image, counts, truncated);
        if (rq.fb) {
            const int limit = std::min(rq.fb->spec.max_faces, rq.spec.max_faces);
            if (rq.fb->gated) face_gated_copy_out(*rq.fb, d_tensor, d_mats, counts, n, limit, overflow);
            else face_batch_copy_out(*rq.fb, d_tensor, d_mats, counts, n, limit, overflow);
        }
    }

    void tile_merge(const int *rows, const int *cols, int n, const TileRequest &rq, const rf_face *faces, const int *pass_counts,
                    rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        *truncated = false;
        pass_check_args(n, rows, cols, counts, faces && pass_counts ? faces : nullptr, out, cap_per_image, rq.spec.max_faces);
        std::vector<TileEntry> entries;
        std::vector<int> first;
        tile_build_passes(rq.spec, nullptr, false, rows, cols, n, &entries, &first);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const TileSpec sp = rq.spec;
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tile_open(n, sp); },
                     gather_into<TileMap>(sp.edge, tile_cand_, tile_count_, kTileMergeCap),
                     [=](hipStream_t s, const RunParams *d_params) { tile_launch_merge(s, n, sp, d_params); }, tile_dirty_);
        tile_copy_out(n, rq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- flip test-time augmentation
    // The passes of a call's frames as one table, frame-major (frame i: pass 0, then with flip on pass 1).  A NULL / empty frame
    // keeps its passes, which gather nothing (frame = -1).  `have_ptrs` false: tta_merge(), which has no pixels.
    void tta_build_passes(const TtaSpec &sp, const uint8_t *const *frames, bool have_ptrs, const int *rows, const int *cols, int n,
                          std::vector<TtaEntry> *entries) const {
        entries->clear();
        for (int i = 0; i < n; i++) {
            const bool empty = (have_ptrs && !frames[i]) || rows[i] <= 0 || cols[i] <= 0;
            if (!empty && rows[i] > 4096 * 3072 / cols[i]) throw ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
            for (int p = 0; p < sp.passes(); p++) {
                TtaEntry e;
                e.frame = empty ? -1 : i; e.rows = empty ? 0 : rows[i]; e.cols = empty ? 0 : cols[i]; e.pass = p;
                e.scale = empty ? 1.f : tile_frame_scale(rows[i], cols[i], net_h_, net_w_);
                entries->push_back(e);
            }
        }
    }

    // blocks of a TTA call, sized once and reused (as tile_open): in device memory, per frame kTtaMergeCap candidate records and
    // their counter; in pinned host memory, which the merge kernel writes straight into as the NMS kernel writes its result block
    // (nothing reads the merged faces on the device, so no copy follows the call), max_faces merged records and member counts
    // and the head / candidate counts.  The counters are zero between calls (the merge re-arms them); a new block, or a call that
    // ended in an error, is zeroed here.
    void tta_open(int n, const TtaSpec &sp) {
        const size_t nf = (size_t)std::max(n, 1);
        tta_cand_.reserve(nf * kTtaMergeCap * sizeof(Candidate));
        const uint8_t *before = tta_count_.ptr;
        tta_count_.reserve(nf * sizeof(int));
        if (tta_count_.ptr != before) tta_dirty_ = true;
        tta_out_.reserve(nf * sp.max_faces * sizeof(Candidate));
        tta_votes_.reserve(nf * sp.max_faces * sizeof(int));
        tta_outcount_.reserve(2 * nf * sizeof(int));
        if (tta_dirty_) {
            RF_HIP(hipDeviceSynchronize());
            RF_HIP(hipMemset(tta_count_.ptr, 0, tta_count_.cap));
            RF_HIP(hipDeviceSynchronize());
            tta_dirty_ = false;
        }
    }

    void tta_launch_merge(hipStream_t st, int n, const TtaSpec &sp, const RunParams *d_params) {
        VoteMergeParams vp;
        vp.cand = (const Candidate *)tta_cand_.ptr; vp.cand_count = (int *)tta_count_.ptr; vp.cap = kTtaMergeCap;
        vp.params = d_params;
        vp.out = (Candidate *)tta_out_.ptr; vp.out_count = (int *)tta_outcount_.ptr; vp.out_cand_count = (int *)tta_outcount_.ptr + n;
        vp.votes = (int *)tta_votes_.ptr;
        vp.max_det = sp.max_faces;
        vp.n = n;
        launch_vote_merge(st, vp, sp.vote != 0);
    }

    // results of a finished TTA call (the host has waited for its last launch, so the pinned blocks hold them): true counts, the
    // first min(count, max_faces, cap_per_image) faces of each frame, their member counts and passes
    void tta_copy_out(int n, const TtaRequest &rq, rf_face *out, int cap_per_image, int *counts, bool *truncated) {
        const int *hc = (const int *)tta_outcount_.ptr;
        const int mf = rq.spec.max_faces;
        for (int i = 0; i < n; i++) {
            counts[i] = hc[i];
            if (hc[n + i] > kTtaMergeCap || hc[i] > mf) *truncated = true;
            if (out && std::min(hc[i], mf) > cap_per_image) *truncated = true;
            const int k = out ? std::min(std::min(hc[i], mf), cap_per_image) : 0;
            const Candidate *src = (const Candidate *)tta_out_.ptr + (size_t)i * mf;
            const int *vt = (const int *)tta_votes_.ptr + (size_t)i * mf;
            for (int j = 0; j < k; j++) {
                memcpy(&out[(size_t)i * cap_per_image + j], &src[j], sizeof(rf_face));
                if (rq.votes) rq.votes[(size_t)i * cap_per_image + j] = vt[j];
                if (rq.src_pass) rq.src_pass[(size_t)i * cap_per_image + j] = src[j].anchor / opt_.max_detections;
            }
        }
    }

    void mirror(const void *d_src, int rows, int cols, int step, void *d_dst, int dst_step) override {
        if (rows < 0 || cols < 0) throw ArgError("negative frame size");
        if (rows == 0 || cols == 0) return;
        if (!d_dst || dst_step < cols * 3) throw ArgError("mirror: null destination or dst_step < cols * 3");
        check_frame((const uint8_t *)d_src, rows, cols, step);
        if (!d_src) throw ArgError("null argument");
        DeviceGuard guard(device_);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        const MirrorParams mp{(const uint8_t *)d_src, rows, cols, step, (uint8_t *)d_dst, dst_step};
        launch_mirror_rows(align_stream_, &mp, 1);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
    }

    // the voting merge of a TTA, pyramid or rotation call over n frames
    PassCall::Merge vote_merge_of(int n, const TtaSpec &sp) {
        return [=](hipStream_t s, const RunParams *d_params) { tta_launch_merge(s, n, sp, d_params); };
    }

    void detect_tta(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                    float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const TtaRequest &rq) override {
        *truncated = false;
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, rq.spec.max_faces);
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        std::vector<TtaEntry> entries;
        tta_build_passes(rq.spec, frames, true, rows, cols, n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int PP = rq.spec.passes();
        const std::vector<const uint8_t *> base =
            pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return entries[(size_t)i * PP].frame >= 0; });
        launch_pending();
        // The mirrored copies: dense, each at a 256-byte-aligned offset of one block (what a freshly allocated dense frame looks
        // like to conv0's staging), made on the side stream; every lane that launches a pass of the call waits for them on the device.
        PassViews v((int)entries.size());
        hipEvent_t mirrored = nullptr;
        std::vector<MirrorParams> mp;
        size_t bytes = 0;
        for (int i = 0; i < n; i++)
            if (base[i]) bytes += align256((size_t)rows[i] * cols[i] * 3);
        uint8_t *d_mirror = rq.spec.flip ? tta_mirror_.reserve(bytes) : nullptr;
        for (int i = 0; i < n; i++) {
            if (!base[i]) continue;
            v.set(i * PP, base[i], rows[i], cols[i], st[i]);
            if (!rq.spec.flip) continue;
            mp.push_back(MirrorParams{base[i], rows[i], cols[i], st[i], d_mirror, cols[i] * 3});
            v.set(i * PP + 1, d_mirror, rows[i], cols[i], cols[i] * 3);
            d_mirror += align256((size_t)rows[i] * cols[i] * 3);
        }
        if (rq.spec.flip) {
            if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
            launch_mirror_rows(align_stream_, mp.data(), (int)mp.size());
            mirrored = record_inputs_ready();
        }
        tta_open(n, rq.spec);
        *truncated = run_passes("test-time augmentation", entries, v, threshold, mirrored,
                                gather_into<TtaMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, rq.spec), tta_dirty_);
        tta_copy_out(n, rq, out, cap_per_image, counts, truncated);
    }

    void tta_merge(const int *rows, const int *cols, int n, const TtaRequest &rq, const rf_face *faces, const int *pass_counts,
                   rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        *truncated = false;
        pass_check_args(n, rows, cols, counts, faces, out, cap_per_image, rq.spec.max_faces);
        if (n > 0 && !pass_counts) throw ArgError("null argument");
        std::vector<TtaEntry> entries;
        tta_build_passes(rq.spec, nullptr, false, rows, cols, n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tta_open(n, rq.spec); },
                     gather_into<TtaMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, rq.spec), tta_dirty_);
        tta_copy_out(n, rq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- zoom-pyramid detection
    // The pyramid plans of a call's frames as one pass table (frames in call order, passes in plan order); first[i]: frame i's first
    // pass; *zoom_bytes: what the zoom tiles of the call take.  A NULL / empty frame is one pass that gathers nothing (frame = -1).
    // `have_ptrs` false: pyramid_merge(), which has no pixels.  Throws before any state has changed.
    void pyr_build_passes(const PyrSpec &sp, const uint8_t *const *frames, bool have_ptrs, const int *rows, const int *cols, int n,
                          std::vector<PyrEntry> *entries, std::vector<int> *first, size_t *zoom_bytes) const {
        entries->clear();
        first->assign((size_t)n + 1, 0);
        *zoom_bytes = 0;
        for (int i = 0; i < n; i++) {
            (*first)[i] = (int)entries->size();
            const bool empty = (have_ptrs && !frames[i]) || rows[i] <= 0 || cols[i] <= 0;
            if (empty) {
                PyrEntry e;
                memset(&e, 0, sizeof(e));
                e.frame = -1; e.z = 1; e.scale = 1.f;
                entries->push_back(e);
                continue;
            }
            if (rows[i] > 4096 * 3072 / cols[i]) throw ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
            if (pyr_plan(sp, rows[i], cols[i], net_h_, net_w_, i, entries, zoom_bytes) < 0)
                throw ArgError("pyramid detection: a frame's plan has more than 1024 passes");
            if (*zoom_bytes > kPyrMaxZoomBytes) throw ArgError("pyramid detection: the zoom tiles of the call need more than 1 GiB");
        }
        (*first)[n] = (int)entries->size();
    }

    // the blocks of a pyramid call are those of a TTA call (tta_open): the two calls never overlap, and the merge is the same launch
    static TtaSpec pyr_merge_spec(const PyrSpec &sp) {
        TtaSpec t;
        t.flip = 0; t.vote = sp.vote; t.max_faces = sp.tile.max_faces;
        return t;
    }
    static TtaRequest pyr_merge_request(const PyrRequest &rq) {
        TtaRequest t;
        t.spec = pyr_merge_spec(rq.spec); t.votes = rq.votes; t.src_pass = rq.src_pass;
        return t;
    }

    void zoom(const void *d_src, int rows, int cols, int step, int z, int x0, int y0, int tw, int th, void *d_dst, int dst_step) override {
        if (rows < 0 || cols < 0 || tw < 0 || th < 0) throw ArgError("negative frame or window size");
        if (z != 2 && z != 4) throw ArgError("zoom: z must be 2 or 4");
        if (rows == 0 || cols == 0 || tw == 0 || th == 0) return;
        check_frame((const uint8_t *)d_src, rows, cols, step);
        if (!d_src) throw ArgError("null argument");
        if (x0 < 0 || y0 < 0 || x0 > z * cols - tw || y0 > z * rows - th) throw ArgError("zoom: the window leaves the enlarged frame");
        if (!d_dst || dst_step < tw * 3) throw ArgError("zoom: null destination or dst_step < tw * 3");
        DeviceGuard guard(device_);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        const ZoomParams zp{(const uint8_t *)d_src, rows, cols, step, z, x0, y0, tw, th, (uint8_t *)d_dst, dst_step};
        launch_zoom_tiles(align_stream_, &zp, 1);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
    }

    void detect_pyramid(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                        float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const PyrRequest &rq) override {
        *truncated = false;
        const TtaRequest mrq = pyr_merge_request(rq);
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, mrq.spec.max_faces);
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        std::vector<PyrEntry> entries;
        std::vector<int> first;
        size_t zoom_bytes = 0;
        pyr_build_passes(rq.spec, frames, true, rows, cols, n, &entries, &first, &zoom_bytes);
        if (n == 0) return;
        DeviceGuard guard(device_);
        // the 1x passes are views of the frames (host frames: of their one dense copy), the zoom kernel reads the same
        const std::vector<const uint8_t *> base =
            pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return entries[first[i]].frame >= 0; });
        launch_pending();
        // The zoom tiles: dense, each at a 256-byte-aligned offset of one growing block (what a freshly allocated dense frame looks
        // like to conv0's staging), made on the side stream; every lane that launches a pass of the call waits for them on the device.
        const int P = (int)entries.size();
        PassViews v(P);
        uint8_t *d_zoom = zoom_bytes ? pyr_zoom_.reserve(zoom_bytes) : nullptr;
        std::vector<ZoomParams> zp;
        size_t zoff = 0;
        for (int q = 0; q < P; q++) {
            const PyrEntry &e = entries[q];
            if (e.frame < 0) continue;
            const int i = e.frame;
            if (e.z == 1) {
                v.set(q, base[i] + (size_t)e.y0 * st[i] + (size_t)3 * e.x0, e.th, e.tw, st[i]);
                continue;
            }
            uint8_t *dst = d_zoom + zoff;
            zoff += align256((size_t)e.tw * e.th * 3);
            zp.push_back(ZoomParams{base[i], rows[i], cols[i], st[i], e.z, e.x0, e.y0, e.tw, e.th, dst, e.tw * 3});
            v.set(q, dst, e.th, e.tw, e.tw * 3);
        }
        hipEvent_t zoomed = nullptr;
        if (!zp.empty()) {
            if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
            launch_zoom_tiles(align_stream_, zp.data(), (int)zp.size());
            zoomed = record_inputs_ready();
        }
        tta_open(n, mrq.spec);
        *truncated = run_passes("pyramid detection", entries, v, threshold, zoomed,
                                gather_into<PyrMap>(rq.spec.tile.edge, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    void pyramid_merge(const int *rows, const int *cols, int n, const PyrRequest &rq, const rf_face *faces, const int *pass_counts,
                       rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        *truncated = false;
        const TtaRequest mrq = pyr_merge_request(rq);
        pass_check_args(n, rows, cols, counts, faces, out, cap_per_image, mrq.spec.max_faces);
        if (n > 0 && !pass_counts) throw ArgError("null argument");
        std::vector<PyrEntry> entries;
        std::vector<int> first;
        size_t zoom_bytes = 0;
        pyr_build_passes(rq.spec, nullptr, false, rows, cols, n, &entries, &first, &zoom_bytes);
        if (n == 0) return;
        DeviceGuard guard(device_);
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tta_open(n, mrq.spec); },
                     gather_into<PyrMap>(rq.spec.tile.edge, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- rotation-robust detection
    // The passes of a call's frames as one table, frame-major, ascending k over the rotations of the spec.  A NULL / empty frame keeps
    // its passes, which gather nothing (frame = -1).  `have_ptrs` false: rot_merge(), which has no pixels.  Throws before any state
    // has changed.
    void rot_build_passes(const RotSpec &sp, const uint8_t *const *frames, bool have_ptrs, const int *rows, const int *cols, int n,
                          std::vector<RotEntry> *entries) const {
        entries->clear();
        for (int i = 0; i < n; i++) {
            const bool empty = (have_ptrs && !frames[i]) || rows[i] <= 0 || cols[i] <= 0;
            if (!empty && rows[i] > 4096 * 3072 / cols[i]) throw ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
            for (int k = 0; k < 4; k++) {
                if (!(sp.rots >> k & 1)) continue;
                RotEntry e;
                e.frame = empty ? -1 : i; e.rows = empty ? 0 : rows[i]; e.cols = empty ? 0 : cols[i]; e.k = k;
                e.scale = 1.f;
                if (!empty) {
                    const int rk = rot_rows(k, rows[i], cols[i]), ck = rot_cols(k, rows[i], cols[i]);
                    if (rk > 4096 * 3072 / ck) throw ArgError("a rotated pass is larger than 4096x3072 (RetinaFace.cpp:325)");
                    e.scale = tile_frame_scale(rk, ck, net_h_, net_w_);
                }
                entries->push_back(e);
            }
        }
    }

    // the blocks of a rotation call are those of a TTA call (tta_open): the two calls never overlap, and the merge is the same launch
    static TtaSpec rot_merge_spec(const RotSpec &sp) {
        TtaSpec t;
        t.flip = 0; t.vote = sp.vote; t.max_faces = sp.max_faces;
        return t;
    }
    static TtaRequest rot_merge_request(const RotRequest &rq) {
        TtaRequest t;
        t.spec = rot_merge_spec(rq.spec); t.votes = rq.votes; t.src_pass = rq.src_rot;
        return t;
    }

    void rotate(const void *d_src, int rows, int cols, int step, int k, void *d_dst, int dst_step) override {
        if (rows < 0 || cols < 0) throw ArgError("negative frame size");
        if (k < 0 || k > 3) throw ArgError("rotate: k must be in [0, 3]");
        if (rows == 0 || cols == 0) return;
        if (!d_dst || dst_step < rot_cols(k, rows, cols) * 3) throw ArgError("rotate: null destination or dst_step < cols_k * 3");
        check_frame((const uint8_t *)d_src, rows, cols, step);
        if (!d_src) throw ArgError("null argument");
        DeviceGuard guard(device_);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        const RotateParams rp{(const uint8_t *)d_src, rows, cols, step, k, (uint8_t *)d_dst, dst_step};
        launch_rotate_frames(align_stream_, &rp, 1);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
    }

    void detect_rot(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                    float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const RotRequest &rq) override {
        *truncated = false;
        const TtaRequest mrq = rot_merge_request(rq);
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, mrq.spec.max_faces);
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        std::vector<RotEntry> entries;
        rot_build_passes(rq.spec, frames, true, rows, cols, n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int PP = rq.spec.passes();
        const std::vector<const uint8_t *> base =
            pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return entries[(size_t)i * PP].frame >= 0; });
        launch_pending();
        // The rotated copies: dense, each at a 256-byte-aligned offset of one block (what a freshly allocated dense frame looks like to
        // conv0's staging), made on the side stream; every lane that launches a pass of the call waits for them on the device.
        const int P = (int)entries.size();
        size_t copy_bytes = 0;
        for (int i = 0; i < n; i++)
            if (base[i]) copy_bytes += align256((size_t)rows[i] * cols[i] * 3) * (size_t)__builtin_popcount((unsigned)rq.spec.rots & 14u);
        uint8_t *d_copies = copy_bytes ? rot_copies_.reserve(copy_bytes) : nullptr;
        PassViews v(P);
        std::vector<RotateParams> rp;
        size_t coff = 0;
        for (int q = 0; q < P; q++) {
            const RotEntry &e = entries[q];
            if (e.frame < 0) continue;
            const int i = e.frame, rk = rot_rows(e.k, rows[i], cols[i]), ck = rot_cols(e.k, rows[i], cols[i]);
            if (e.k == 0) {
                v.set(q, base[i], rk, ck, st[i]);
                continue;
            }
            uint8_t *dst = d_copies + coff;
            coff += align256((size_t)rows[i] * cols[i] * 3);
            rp.push_back(RotateParams{base[i], rows[i], cols[i], st[i], e.k, dst, ck * 3});
            v.set(q, dst, rk, ck, ck * 3);
        }
        hipEvent_t rotated = nullptr;
        if (!rp.empty()) {
            if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
            launch_rotate_frames(align_stream_, rp.data(), (int)rp.size());
            rotated = record_inputs_ready();
        }
        tta_open(n, mrq.spec);
        *truncated = run_passes("rotation detection", entries, v, threshold, rotated,
                                gather_into<RotMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    void rot_merge(const int *rows, const int *cols, int n, const RotRequest &rq, const rf_face *faces, const int *pass_counts,
                   rf_face *out, int cap_per_image, int *counts, bool *truncated) override {
        *truncated = false;
        const TtaRequest mrq = rot_merge_request(rq);
        pass_check_args(n, rows, cols, counts, faces, out, cap_per_image, mrq.spec.max_faces);
        if (n > 0 && !pass_counts) throw ArgError("null argument");
        std::vector<RotEntry> entries;
        rot_build_passes(rq.spec, nullptr, false, rows, cols, n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tta_open(n, mrq.spec); },
                     gather_into<RotMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- fisheye detection
private:
    struct Dewarper;
public:
    void *dewarper_create(int rows, int cols, int view_w, int view_h, int views, const int32_t *mesh) override {
        if (rows <= 0 || cols <= 0 || rows > 4096 * 3072 / cols) throw ArgError("dewarper: rows x cols must be in (0, 4096x3072]");
        if (view_w < 0 || view_h < 0) throw ArgError("dewarper: negative view size");
        if (!view_w) view_w = net_w_;
        if (!view_h) view_h = net_h_;
        if (const char *bad = dewarp_check_mesh(view_w, view_h, views, mesh)) throw ArgError(std::string("dewarper: ") + bad);
        DeviceGuard guard(device_);
        std::unique_ptr<Dewarper> d(new Dewarper);
        d->rows = rows; d->cols = cols; d->view_w = view_w; d->view_h = view_h; d->views = views;
        const size_t bytes = d->view_ints() * (size_t)views * sizeof(int32_t);
        d->mesh.reserve(bytes);
        try { RF_HIP(hipMemcpy(d->mesh.ptr, mesh, bytes, hipMemcpyHostToDevice)); } catch (...) { d->mesh.release(); throw; }
        dewarpers_.push_back(std::move(d));
        return dewarpers_.back().get();
    }
    void dewarper_destroy(void *p) override {
        for (size_t i = 0; i < dewarpers_.size(); i++)
            if (dewarpers_[i].get() == p) {
                DeviceGuard guard(device_);
                if (align_stream_) (void)hipStreamSynchronize(align_stream_);
                dewarpers_[i]->mesh.release();
                dewarpers_.erase(dewarpers_.begin() + i);
                return;
            }
    }
    Dewarper &dewarper_of(void *p) {
        for (auto &d : dewarpers_)
            if (d.get() == p) return *d;
        throw ArgError("not a dewarper of this handle");
    }

    // The passes of a call's frames as one table, frame-major, ascending view.  A NULL frame keeps its passes, which gather nothing
    // (frame = -1).  frames null: dewarp_merge(), which has no pixels.  rows: 0 for an empty frame.
    void dewarp_build_passes(const Dewarper &dw, const uint8_t *const *frames, const int *rows, int n, std::vector<DewarpEntry> *entries) const {
        entries->clear();
        const float scale = tile_frame_scale(dw.view_h, dw.view_w, net_h_, net_w_);
        for (int i = 0; i < n; i++) {
            const bool empty = frames && (!frames[i] || rows[i] == 0);
            for (int v = 0; v < dw.views; v++) {
                DewarpEntry e;
                memset(&e, 0, sizeof(e));
                e.frame = empty ? -1 : i; e.view = v; e.rows = dw.rows; e.cols = dw.cols; e.view_w = dw.view_w; e.view_h = dw.view_h;
                e.scale = scale; e.mesh = dw.view_mesh(v);
                entries->push_back(e);
            }
        }
    }

    // the blocks of a fisheye call are those of a TTA call (tta_open): the two calls never overlap, and the merge is the same launch
    static TtaRequest dewarp_merge_request(const DewarpRequest &rq) {
        TtaRequest t;
        t.spec.flip = 0; t.spec.vote = rq.spec.vote; t.spec.max_faces = rq.spec.max_faces;
        t.votes = rq.votes; t.src_pass = rq.src_view;
        return t;
    }

    void dewarp(void *p, int view, const void *d_src, int step, void *d_dst, int dst_step) override {
        Dewarper &dw = dewarper_of(p);
        if (view < 0 || view >= dw.views) throw ArgError("dewarp: view out of range");
        if (!d_dst || dst_step < dw.view_w * 3) throw ArgError("dewarp: null destination or dst_step < view_w * 3");
        check_frame((const uint8_t *)d_src, dw.rows, dw.cols, step);
        if (!d_src) throw ArgError("null argument");
        DeviceGuard guard(device_);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        const DewarpParams dp{(const uint8_t *)d_src, dw.rows, dw.cols, step, dw.view_mesh(view), dw.view_w, dw.view_h, (uint8_t *)d_dst, dst_step};
        launch_dewarp_views(align_stream_, &dp, 1);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
    }

    void detect_dewarp(const uint8_t *const *frames, const int *frame_rows, const int *frame_cols, const int *steps, int n, bool on_device,
                       float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const DewarpRequest &rq) override {
        *truncated = false;
        Dewarper &dw = dewarper_of(rq.dewarper);
        const TtaRequest mrq = dewarp_merge_request(rq);
        pass_check_args(n, frames, frames, frames, counts, out, cap_per_image, mrq.spec.max_faces);
        std::vector<int> rows((size_t)std::max(n, 1), dw.rows), cols((size_t)std::max(n, 1), dw.cols);
        for (int i = 0; i < n; i++) {
            const int r = frame_rows ? frame_rows[i] : dw.rows, c = frame_cols ? frame_cols[i] : dw.cols;
            if (!frames[i] || (r == 0 && c == 0)) { rows[i] = cols[i] = 0; continue; }      // an empty frame
            if (r != dw.rows || c != dw.cols) throw ArgError("fisheye detection: a frame's shape is not the dewarper's");
        }
        std::vector<int> st = checked_steps(frames, rows.data(), cols.data(), steps, n);
        std::vector<DewarpEntry> entries;
        dewarp_build_passes(dw, frames, rows.data(), n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int V = dw.views;
        const std::vector<const uint8_t *> base =
            pass_frame_bases(frames, rows.data(), cols.data(), st, n, on_device, [&](int i) { return entries[(size_t)i * V].frame >= 0; });
        launch_pending();
        // The views: dense frames, frame-major, in the caller's block or in one of the engine's -- a view is a multiple of 768 bytes, so
        // each starts 256-byte aligned (what a freshly allocated dense frame looks like to conv0's staging); made on the side stream,
        // every lane that launches a pass of the call waits for them on the device.
        const int P = (int)entries.size();
        const size_t vb = dw.view_bytes();
        uint8_t *d_views = rq.d_views ? (uint8_t *)rq.d_views : dewarp_views_.reserve(vb * (size_t)P);
        PassViews v(P);
        std::vector<DewarpParams> dp;
        for (int q = 0; q < P; q++) {
            const DewarpEntry &e = entries[q];
            if (e.frame < 0) continue;
            uint8_t *dst = d_views + vb * (size_t)q;
            dp.push_back(DewarpParams{base[e.frame], dw.rows, dw.cols, st[e.frame], e.mesh, dw.view_w, dw.view_h, dst, dw.view_w * 3});
            v.set(q, dst, dw.view_h, dw.view_w, dw.view_w * 3);
        }
        hipEvent_t dewarped = nullptr;
        if (!dp.empty()) {
            if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
            launch_dewarp_views(align_stream_, dp.data(), (int)dp.size());
            dewarped = record_inputs_ready();
        }
        tta_open(n, mrq.spec);
        *truncated = run_passes("fisheye detection", entries, v, threshold, dewarped,
                                gather_into<DewarpMap>(rq.spec.edge, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    void dewarp_merge(int n, const DewarpRequest &rq, const rf_face *faces, const int *pass_counts, rf_face *out, int cap_per_image,
                      int *counts, bool *truncated) override {
        *truncated = false;
        Dewarper &dw = dewarper_of(rq.dewarper);
        const TtaRequest mrq = dewarp_merge_request(rq);
        pass_check_args(n, faces, faces, counts, pass_counts, out, cap_per_image, mrq.spec.max_faces);
        std::vector<DewarpEntry> entries;
        dewarp_build_passes(dw, nullptr, nullptr, n, &entries);
        if (n == 0) return;
        DeviceGuard guard(device_);
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tta_open(n, mrq.spec); },
                     gather_into<DewarpMap>(rq.spec.edge, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- region detection
    // The regions of a call, checked, as cell records (frame-major, the call's order) and as one pass table, frame-major, ascending
    // region: frame i's passes are ceil(roi_counts[i] / grid^2) views of the net's size.  Entries point into `d_cells`, the address
    // the records will have on the device.  A NULL frame keeps its passes, which gather nothing (frame = -1).  frames null:
    // roi_merge(), which has no pixels.
    void roi_build_passes(const RoiRequest &rq, const uint8_t *const *frames, const int *rows, const int *cols, int n,
                          std::vector<RoiCell> *cells, std::vector<RoiEntry> *entries, std::vector<int> *first_cell) const {
        const int G = rq.spec.grid, GG = G * G;
        if (const char *bad = roi_check_view(net_w_, net_h_, G)) throw ArgError(std::string("region detection: ") + bad);
        if (n > 0 && !rq.roi_counts) throw ArgError("null argument");
        cells->clear(); entries->clear(); first_cell->clear();
        size_t total = 0;
        for (int i = 0; i < n; i++) {
            if (rq.roi_counts[i] < 0 || rq.roi_counts[i] > kRoiMaxRegions) throw ArgError("region detection: a frame has 0 to 256 regions");
            total += (size_t)rq.roi_counts[i];
        }
        if (total && !rq.rois) throw ArgError("null argument");
        for (size_t r = 0; r < total; r++)
            if (!roi_valid(rq.rois[r])) throw ArgError("region detection: a region's w, h must be in [1, 16384], |x|, |y| at most 2^20");
        const int cw = net_w_ / G, ch = net_h_ / G;
        const rf_roi *roi = rq.rois;
        for (int i = 0; i < n; i++) {
            const int R = rq.roi_counts[i];
            const bool empty = frames && (!frames[i] || rows[i] <= 0 || cols[i] <= 0);
            for (int p = 0; p < roi_passes(R, G); p++) {
                RoiEntry e;
                memset(&e, 0, sizeof(e));
                e.frame = empty ? -1 : i; e.pass = p; e.rows = rows[i]; e.cols = cols[i]; e.grid = G; e.used = std::min(GG, R - p * GG);
                e.net_w = net_w_; e.net_h = net_h_;
                first_cell->push_back((int)cells->size() + p * GG);
                entries->push_back(e);
            }
            for (int r = 0; r < R; r++) cells->push_back(roi_plan(roi[r], cw, ch, rq.spec.max_zoom));
            roi += R;
        }
    }

    // The cell records of a call in device memory: staged in a pinned host block and copied on the side stream (in front of the atlas
    // kernel and of inputs_ready, as a dewarper's meshes are in front of its first call); the entries then point at them.  Every
    // caller has the side stream waited for before it returns (the call's last launch waits for inputs_ready; merge_passes
    // synchronises), so the pinned block is free again at the next call.
    void roi_upload_cells(const std::vector<RoiCell> &cells, std::vector<RoiEntry> &entries, const std::vector<int> &first_cell) {
        const size_t bytes = std::max<size_t>(cells.size(), 1) * sizeof(RoiCell);
        uint8_t *pin = roi_cells_pin_.reserve(bytes);
        const RoiCell *d = (const RoiCell *)roi_cells_.reserve(bytes);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        if (!cells.empty()) {
            memcpy(pin, cells.data(), cells.size() * sizeof(RoiCell));
            RF_HIP(hipMemcpyAsync(roi_cells_.ptr, pin, cells.size() * sizeof(RoiCell), hipMemcpyHostToDevice, align_stream_));
        }
        for (size_t q = 0; q < entries.size(); q++) entries[q].cells = d + first_cell[q];
    }

    // the blocks of a region call are those of a TTA call (tta_open): the two calls never overlap, and the merge is the same launch
    static TtaRequest roi_merge_request(const RoiRequest &rq) {
        TtaRequest t;
        t.spec.flip = 0; t.spec.vote = rq.spec.vote; t.spec.max_faces = rq.spec.max_faces;
        t.votes = rq.votes; t.src_pass = rq.src_roi;
        return t;
    }

    void roi_atlas(const void *d_src, int rows, int cols, int step, const rf_roi *rois, int n, const RoiSpec &sp, int view_w, int view_h,
                   void *d_dst, int dst_step) override {
        if (const char *bad = roi_check_view(view_w, view_h, sp.grid)) throw ArgError(std::string("region atlas: ") + bad);
        if (n < 0 || n > kRoiMaxRegions || (n > 0 && !rois)) throw ArgError("region atlas: 0 to 256 regions");
        for (int r = 0; r < n; r++)                                // (four zeros: the void region, whose cell is the void record)
            if (!roi_valid(rois[r]) && !roi_is_void(rois[r])) throw ArgError("region atlas: a region's w, h must be in [1, 16384], |x|, |y| at most 2^20");
        if (!d_dst || dst_step < view_w * 3) throw ArgError("region atlas: null destination or dst_step < view_w * 3");
        check_frame((const uint8_t *)d_src, rows, cols, step);
        if (!d_src || rows <= 0 || cols <= 0) throw ArgError("null argument");
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int GG = sp.grid * sp.grid, P = roi_passes(n, sp.grid);
        std::vector<RoiCell> cells;
        for (int r = 0; r < n; r++)
            cells.push_back(roi_is_void(rois[r]) ? roi_void_cell() : roi_plan(rois[r], view_w / sp.grid, view_h / sp.grid, sp.max_zoom));
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        const RoiCell *d = (const RoiCell *)roi_cells_.reserve(cells.size() * sizeof(RoiCell));
        RF_HIP(hipMemcpy(roi_cells_.ptr, cells.data(), cells.size() * sizeof(RoiCell), hipMemcpyHostToDevice));
        std::vector<RoiAtlasParams> ap;
        for (int p = 0; p < P; p++)
            ap.push_back(RoiAtlasParams{(const uint8_t *)d_src, rows, cols, step, d + (size_t)p * GG, std::min(GG, n - p * GG), sp.grid, view_w, view_h,
                                        (uint8_t *)d_dst + (size_t)p * view_h * dst_step, dst_step,
                                        roi_min_level(cells.data() + (size_t)p * GG, std::min(GG, n - p * GG))});
        launch_roi_views(align_stream_, ap.data(), P);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
    }

    void detect_rois(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device, float threshold,
                     rf_face *out, int cap_per_image, int *counts, bool *truncated, const RoiRequest &rq) override {
        *truncated = false;
        const TtaRequest mrq = roi_merge_request(rq);
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, mrq.spec.max_faces);
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        std::vector<RoiCell> cells;
        std::vector<RoiEntry> entries;
        std::vector<int> first_cell;
        roi_build_passes(rq, frames, rows, cols, n, &cells, &entries, &first_cell);
        for (int i = 0; i < n; i++) counts[i] = 0;
        const int P = (int)entries.size();
        if (P == 0) return;                                       // no frame has a region: no pass, no faces
        DeviceGuard guard(device_);
        std::vector<char> live((size_t)n, 0);
        for (const RoiEntry &e : entries)
            if (e.frame >= 0) live[e.frame] = 1;
        const std::vector<const uint8_t *> base = pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return live[i] != 0; });
        launch_pending();
        // The views: dense frames, frame-major, in the caller's block or in one of the engine's -- a view of the net's size is a multiple
        // of 768 bytes, so each starts 256-byte aligned; made on the side stream behind the copy of the cell records, every lane that
        // launches a pass of the call waits for them on the device.
        const size_t vb = (size_t)net_w_ * net_h_ * 3;
        uint8_t *d_views = rq.d_views ? (uint8_t *)rq.d_views : roi_views_.reserve(vb * (size_t)P);
        bool any_live = false;
        for (char l : live) any_live = any_live || l;
        if (any_live) roi_upload_cells(cells, entries, first_cell);      // (the passes of NULL frames never read their records)
        PassViews v(P);
        std::vector<RoiAtlasParams> ap;
        for (int q = 0; q < P; q++) {
            const RoiEntry &e = entries[q];
            if (e.frame < 0) continue;
            uint8_t *dst = d_views + vb * (size_t)q;
            ap.push_back(RoiAtlasParams{base[e.frame], e.rows, e.cols, st[e.frame], e.cells, e.used, e.grid, net_w_, net_h_, dst, net_w_ * 3,
                                        roi_min_level(cells.data() + first_cell[q], e.used)});
            v.set(q, dst, net_h_, net_w_, net_w_ * 3);
        }
        hipEvent_t packed = nullptr;
        if (!ap.empty()) {
            launch_roi_views(align_stream_, ap.data(), (int)ap.size());
            packed = record_inputs_ready();
        }
        tta_open(n, mrq.spec);
        *truncated = run_passes("region detection", entries, v, threshold, packed,
                                gather_into<RoiMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    void roi_merge(const int *rows, const int *cols, int n, const RoiRequest &rq, const rf_face *faces, const int *pass_counts, rf_face *out,
                   int cap_per_image, int *counts, bool *truncated) override {
        *truncated = false;
        const TtaRequest mrq = roi_merge_request(rq);
        pass_check_args(n, rows, cols, counts, rq.roi_counts, out, cap_per_image, mrq.spec.max_faces);
        for (int i = 0; i < n; i++)
            if (rows[i] < 0 || cols[i] < 0) throw ArgError("negative frame size");
        std::vector<RoiCell> cells;
        std::vector<RoiEntry> entries;
        std::vector<int> first_cell;
        roi_build_passes(rq, nullptr, rows, cols, n, &cells, &entries, &first_cell);
        if (!entries.empty() && (!faces || !pass_counts)) throw ArgError("null argument");
        for (int i = 0; i < n; i++) counts[i] = 0;
        if (entries.empty()) return;
        DeviceGuard guard(device_);
        roi_upload_cells(cells, entries, first_cell);             // on the side stream, in front of the table's copy and the gather
        merge_passes(entries, n, faces, pass_counts, truncated, [&] { tta_open(n, mrq.spec); },
                     gather_into<RoiMap>(0, tta_cand_, tta_count_, kTtaMergeCap), vote_merge_of(n, mrq.spec), tta_dirty_);
        tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
    }

    // -------------------------------------------------------------------------------- tracked region detection
private:
    struct Tracker;
public:
    // The arguments of a tracked region call, checked before any state changes: the cell rule, the margin, the tracker (no gallery, no
    // follow, not in the error state: track_check), and every stream at most once -- the cells of a call are planned before any of its
    // steps runs, so a second image of a stream would be planned from a table the first has yet to step.
    Tracker &roi_track_check(const TrackRequest &trq, int n, const RoiTrackRequest &rq) {
        if (const char *bad = roi_check_view(net_w_, net_h_, rq.spec.grid)) throw ArgError(std::string("region detection: ") + bad);
        if (rq.margin_q8 < 0 || rq.margin_q8 > 65535) throw ArgError("region detection: margin_q8 must be in [0, 65535]");
        if (n < 0) throw ArgError("null argument");
        Tracker &t = track_check(trq, n);
        std::vector<int> seen;
        for (int i = 0; i < n; i++)
            if (trq.stream_of_image[i] >= 0) seen.push_back(trq.stream_of_image[i]);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) throw ArgError("tracked region detection: a stream appears more than once in the call");
        return t;
    }

    // The track-cells launch of a call on the side stream: streams[i] (device-visible) = the stream whose table plans image i, or -1
    // (stream -1, a frame without pixels); image i's records at d + i * stride (0: max_tracks).
    void roi_track_cells_launch(const Tracker &t, const RoiSpec &spec, int margin_q8, const int32_t *streams, int n, RoiCell *d, int stride) {
        RoiTrackCellsParams cp;
        memset((void *)&cp, 0, sizeof(cp));
        cp.streams = streams; cp.n = n;
        cp.spec = t.spec;
        cp.state = t.state.ptr;
        if (t.has_motion) { cp.motion = (const rf_track_motion *)t.motion.ptr; cp.mspec = t.motion_spec; }
        cp.margin_q8 = margin_q8; cp.cw = net_w_ / spec.grid; cp.ch = net_h_ / spec.grid; cp.max_zoom = spec.max_zoom;
        cp.cells = d; cp.stride = stride;
        launch_roi_track_cells(align_stream_, cp);
        RF_HIP(hipGetLastError());
    }

    // the planned records of a finished call to the host: what the kernel wrote, the void record for the images it skipped
    void roi_track_cells_out(const RoiCell *d_cells, const int *plans, int n, int T, rf_roi_cell *cells) {
        if (!cells || n == 0) return;
        RF_HIP(hipMemcpy(cells, d_cells, (size_t)n * T * sizeof(RoiCell), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++)
            if (plans[i] < 0)
                for (int s = 0; s < T; s++) cells[(size_t)i * T + s] = roi_void_cell();
    }

    void roi_track_cells(const TrackRequest &trq, int n, const RoiTrackRequest &rq, rf_roi_cell *cells) override {
        Tracker &t = roi_track_check(trq, n, rq);
        if (n > 0 && !cells) throw ArgError("null argument");
        if (n == 0) return;
        DeviceGuard guard(device_);
        int32_t *plans = (int32_t *)roi_cells_pin_.reserve((size_t)n * sizeof(int32_t));
        for (int i = 0; i < n; i++) plans[i] = trq.stream_of_image[i];
        RoiCell *d = (RoiCell *)roi_cells_.reserve((size_t)n * t.spec.max_tracks * sizeof(RoiCell));
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        roi_track_cells_launch(t, rq.spec, rq.margin_q8, plans, n, d, 0);
        RF_HIP(hipStreamSynchronize(align_stream_));
        roi_track_cells_out(d, plans, n, t.spec.max_tracks, cells);
    }

    // A seventh user of the pass-call skeleton: detect_slot_rois() below without a changer.
    void detect_track_rois(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device, float threshold,
                           rf_face *out, int cap_per_image, int *counts, bool *truncated, const RoiTrackRequest &rq, const TrackRequest &trq,
                           bool *cut) override {
        ChangeRequest crq;
        crq.spec = rq.spec; crq.margin_q8 = rq.margin_q8; crq.stream_of_image = trq.stream_of_image;
        crq.votes = rq.votes; crq.src_roi = rq.src_roi; crq.cells = rq.cells; crq.d_views = rq.d_views;
        detect_slot_rois("tracked region detection", frames, rows, cols, steps, n, on_device, threshold, out, cap_per_image, counts, truncated, crq, trq, cut);
    }

    // -------------------------------------------------------------------------------- change regions
private:
    struct Changer;
public:
    void *changer_create(const ChangeSpec &spec, int rows, int cols, int n_streams) override {
        if (n_streams < 1 || n_streams > kChangeMaxStreams) throw ArgError("changer: n_streams must be in [1, 1024]");
        int bw = 0, bh = 0;
        if (const char *bad = change_check_shape(rows, cols, spec, &bw, &bh)) throw ArgError(std::string("changer: ") + bad);
        DeviceGuard guard(device_);
        std::unique_ptr<Changer> c(new Changer);
        c->spec = spec; c->rows = rows; c->cols = cols; c->bw = bw; c->bh = bh; c->n_streams = n_streams;
        try {
            c->ref.reserve((size_t)n_streams * bw * bh * sizeof(int32_t));
            c->mask.reserve((size_t)n_streams * c->mask_pitch());
            c->frames.reserve((size_t)n_streams * sizeof(int64_t));
            changer_reset_impl(*c, -1);
        } catch (...) { c->release(); throw; }
        changers_.push_back(std::move(c));
        return changers_.back().get();
    }
    void changer_destroy(void *p) override {
        for (size_t i = 0; i < changers_.size(); i++)
            if (changers_[i].get() == p) {
                DeviceGuard guard(device_);
                if (align_stream_) (void)hipStreamSynchronize(align_stream_);
                changers_[i]->release();
                changers_.erase(changers_.begin() + i);
                return;
            }
    }
    Changer &changer_of(void *p) {
        for (auto &c : changers_)
            if (c.get() == p) return *c;
        throw ArgError("not a changer of this handle");
    }
    // a stream's (or every stream's) empty state: counter 0 (the next step seeds), reference and mask zero
    void changer_reset_impl(Changer &c, int stream) {
        const int first = stream < 0 ? 0 : stream, count = stream < 0 ? c.n_streams : 1;
        const size_t nb = (size_t)c.bw * c.bh;
        RF_HIP(hipMemset(c.ref.ptr + (size_t)first * nb * sizeof(int32_t), 0, (size_t)count * nb * sizeof(int32_t)));
        RF_HIP(hipMemset(c.mask.ptr + (size_t)first * c.mask_pitch(), 0, (size_t)count * c.mask_pitch()));
        RF_HIP(hipMemset(c.frames.ptr + (size_t)first * sizeof(int64_t), 0, (size_t)count * sizeof(int64_t)));
        RF_HIP(hipDeviceSynchronize());
    }
    void changer_reset(void *p, int stream) override {
        Changer &c = changer_of(p);
        if (stream < -1 || stream >= c.n_streams) throw ArgError("stream out of range");
        DeviceGuard guard(device_);
        changer_reset_impl(c, stream);
        if (stream < 0) c.dirty = false;
    }
    int changer_read(void *p, int stream, int32_t *ref, int64_t *frames, uint8_t *mask) override {
        Changer &c = changer_of(p);
        if (stream < 0 || stream >= c.n_streams) throw ArgError("stream out of range");
        if (c.dirty) throw ArgError("the changer's last call failed: reset it first");
        DeviceGuard guard(device_);
        const size_t nb = (size_t)c.bw * c.bh;
        if (ref) RF_HIP(hipMemcpy(ref, c.ref.ptr + (size_t)stream * nb * sizeof(int32_t), nb * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (frames) RF_HIP(hipMemcpy(frames, c.frames.ptr + (size_t)stream * sizeof(int64_t), sizeof(int64_t), hipMemcpyDeviceToHost));
        if (mask) RF_HIP(hipMemcpy(mask, c.mask.ptr + (size_t)stream * c.mask_pitch(), nb, hipMemcpyDeviceToHost));
        return (int)nb;
    }

    // The arguments of a change-region call, checked before any state changes: the changer, the cell rule, the margin, the streams
    // (each at most once: two images of a stream would step one reference from two workgroups), the shape of every frame that will be
    // stepped and, with a tracker, T + R and the stream counts.  frames null: no frame is looked at.
    Changer &change_check(const ChangeRequest &rq, const void *const *frames, const int *rows, const int *cols, int n, const Tracker *t) {
        Changer &c = changer_of(rq.changer);
        if (c.dirty) throw ArgError("the changer's last call failed: reset it first");
        if (const char *bad = roi_check_view(net_w_, net_h_, rq.spec.grid)) throw ArgError(std::string("region detection: ") + bad);
        if (rq.margin_q8 < 0 || rq.margin_q8 > 65535) throw ArgError("region detection: margin_q8 must be in [0, 65535]");
        if (n < 0 || (n > 0 && !rq.stream_of_image)) throw ArgError("stream_of_image is null");
        if (t && t->spec.max_tracks + c.spec.max_regions > kRoiMaxRegions) throw ArgError("change regions: max_tracks + max_regions must not exceed 256");
        if (t && t->n_streams != c.n_streams) throw ArgError("change regions: the tracker and the changer must have the same number of streams");
        std::vector<int> seen;
        for (int i = 0; i < n; i++) {
            const int s = rq.stream_of_image[i];
            if (s < -1 || s >= c.n_streams) throw ArgError("stream_of_image: stream out of range");
            if (s < 0) continue;
            seen.push_back(s);
            if (frames && frames[i] && rows[i] > 0 && cols[i] > 0 && (rows[i] != c.rows || cols[i] != c.cols))
                throw ArgError("change regions: a frame's shape is not the changer's");
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) throw ArgError("change regions: a stream appears more than once in the call");
        return c;
    }

    // The two launches of a step on the side stream.  images: the pinned table (src null or stream < 0: the image is not stepped);
    // image i's records at d_cells + i * stride + first, its info at d_info + i.
    void change_launch(const Changer &c, const ChangeRequest &rq, const ChangeImage *images, int n, RoiCell *d_cells, int stride, int first,
                       rf_change_info *d_info) {
        ChangeParams cp;
        memset((void *)&cp, 0, sizeof(cp));
        cp.images = images; cp.n = n;
        cp.spec = c.spec;
        cp.rows = c.rows; cp.cols = c.cols; cp.bw = c.bw; cp.bh = c.bh;
        cp.ref = (int32_t *)c.ref.ptr; cp.mask = c.mask.ptr; cp.mask_pitch = (int)c.mask_pitch(); cp.frames = (int64_t *)c.frames.ptr;
        cp.margin_q8 = rq.margin_q8; cp.cw = net_w_ / rq.spec.grid; cp.ch = net_h_ / rq.spec.grid; cp.max_zoom = rq.spec.max_zoom;
        cp.cells = d_cells; cp.cell_stride = stride; cp.cell_first = first;
        cp.info = d_info;
        launch_change_blocks(align_stream_, cp);
        launch_change_regions(align_stream_, cp);
        RF_HIP(hipGetLastError());
    }

    void change_regions(const void *const *d_frames, const int *rows, const int *cols, const int *steps, int n, const ChangeRequest &rq) override {
        if (n < 0 || (n > 0 && (!d_frames || !rows || !cols))) throw ArgError("null argument");
        const std::vector<int> st = checked_steps((const uint8_t *const *)d_frames, rows, cols, steps, n);
        Changer &c = change_check(rq, d_frames, rows, cols, n, nullptr);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int R = c.spec.max_regions;
        ChangeImage *images = (ChangeImage *)roi_cells_pin_.reserve((size_t)n * sizeof(ChangeImage));
        for (int i = 0; i < n; i++) {
            const bool live = rq.stream_of_image[i] >= 0 && d_frames[i] && rows[i] > 0 && cols[i] > 0;
            images[i] = ChangeImage{live ? (const uint8_t *)d_frames[i] : nullptr, st[i], live ? rq.stream_of_image[i] : -1};
        }
        const size_t o_info = align256((size_t)n * R * sizeof(RoiCell));
        uint8_t *d = roi_cells_.reserve(o_info + (size_t)n * sizeof(rf_change_info));
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        c.dirty = true;                                // until the results are back
        change_launch(c, rq, images, n, (RoiCell *)d, R, 0, (rf_change_info *)(d + o_info));
        RF_HIP(hipStreamSynchronize(align_stream_));
        if (rq.cells) RF_HIP(hipMemcpy(rq.cells, d, (size_t)n * R * sizeof(RoiCell), hipMemcpyDeviceToHost));
        if (rq.info) RF_HIP(hipMemcpy(rq.info, d + o_info, (size_t)n * sizeof(rf_change_info), hipMemcpyDeviceToHost));
        c.dirty = false;
    }

    // An eighth user of the pass-call skeleton.
    void detect_change_rois(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device, float threshold,
                            rf_face *out, int cap_per_image, int *counts, bool *truncated, const ChangeRequest &rq, const TrackRequest &trq,
                            bool *cut) override {
        if (!rq.changer) throw ArgError("not a changer of this handle");
        detect_slot_rois("change region detection", frames, rows, cols, steps, n, on_device, threshold, out, cap_per_image, counts, truncated, rq, trq, cut);
    }

    // The one body of the tracked region call (no changer: R = 0) and of the change-region call (a changer, the tracker optional).
    // Every image with pixels has roi_passes(T + R, grid) passes: records 0 .. T - 1 of its block are the tracker's slots, T .. T + R - 1
    // the change slots.  On the side stream, in order: the blocks kernel and the regions kernel (with a changer), the track-cells kernel
    // (with a tracker), the atlas launches (their `cells` are device addresses those launches fill; sized for the x1/4 level, which the
    // host cannot rule out), inputs_ready.  Then the passes with the region gather, and behind the vote merge, on its stream, the
    // track launch over the merged faces (source pixels, score order) in the merge's device-visible output blocks.  The calls are
    // synchronous, so the tables the plan kernels read are settled when the call starts.  An error after the step was enqueued leaves
    // the changer and the tracker in the error state.
    void detect_slot_rois(const char *what, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                          float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const ChangeRequest &rq,
                          const TrackRequest &trq, bool *cut) {
        *truncated = false;
        *cut = false;
        TtaRequest mrq;
        mrq.spec.flip = 0; mrq.spec.vote = rq.spec.vote; mrq.spec.max_faces = rq.spec.max_faces;
        mrq.votes = rq.votes; mrq.src_pass = rq.src_roi;
        pass_check_args(n, frames, rows, cols, counts, out, cap_per_image, mrq.spec.max_faces);
        const bool tracked = trq.tracker || !rq.changer;
        if (tracked && cap_per_image < 1 && trq.tags) throw ArgError("cap_per_image must be >= 1");
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n);
        RoiTrackRequest prq;
        prq.spec = rq.spec; prq.margin_q8 = rq.margin_q8;
        Tracker *t = tracked ? &roi_track_check(trq, n, prq) : nullptr;
        Changer *c = rq.changer ? &change_check(rq, (const void *const *)frames, rows, cols, n, t) : nullptr;
        for (int i = 0; i < n; i++) counts[i] = 0;
        if (n == 0) return;
        const int T = t ? t->spec.max_tracks : 0, R = c ? c->spec.max_regions : 0, S = T + R, G = rq.spec.grid, GG = G * G, PP = roi_passes(S, G);
        std::vector<char> empty((size_t)n);
        DeviceGuard guard(device_);
        // the pinned block: plans | stream table | image table | change images; the device block: records | info
        const size_t o_str = align256((size_t)n * sizeof(int32_t)), o_img = o_str + align256((size_t)n * sizeof(TrackStreamEntry));
        const size_t o_chg = o_img + align256((size_t)n * sizeof(TrackImageEntry));
        uint8_t *pin = roi_cells_pin_.reserve(o_chg + (size_t)n * sizeof(ChangeImage));
        int32_t *plans = (int32_t *)pin;
        for (int i = 0; i < n; i++) {
            empty[i] = !frames[i] || rows[i] <= 0 || cols[i] <= 0;
            plans[i] = empty[i] ? -1 : rq.stream_of_image[i];
        }
        const std::vector<const uint8_t *> base = pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return plans[i] >= 0; });
        launch_pending();
        const size_t rec_bytes = (size_t)n * S * sizeof(RoiCell), o_info = align256(rec_bytes), info_bytes = (size_t)n * sizeof(rf_change_info);
        RoiCell *d_cells = (RoiCell *)roi_cells_.reserve(c ? o_info + info_bytes : rec_bytes);
        const rf_change_info *d_info = (const rf_change_info *)((const uint8_t *)d_cells + o_info);
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        if (c) {
            ChangeImage *images = (ChangeImage *)(pin + o_chg);
            for (int i = 0; i < n; i++) images[i] = ChangeImage{plans[i] >= 0 ? base[i] : nullptr, st[i], plans[i]};
            c->dirty = true;                           // until the results are back
            change_launch(*c, rq, images, n, d_cells, S, T, (rf_change_info *)((uint8_t *)d_cells + o_info));
        }
        if (t) roi_track_cells_launch(*t, rq.spec, rq.margin_q8, plans, n, d_cells, c ? S : 0);
        TrackStreamEntry *se = (TrackStreamEntry *)(pin + o_str);
        TrackImageEntry *ie = (TrackImageEntry *)(pin + o_img);
        const std::vector<float> scale((size_t)n, 1.f);
        const int ns = t ? track_build_table(trq.stream_of_image, 0, n, scale.data(), empty.data(), se, ie) : 0;
        // the passes: PP per image with pixels, frame-major
        std::vector<RoiEntry> entries;
        for (int i = 0; i < n; i++) {
            if (plans[i] < 0) continue;
            for (int p = 0; p < PP; p++) {
                RoiEntry e;
                memset(&e, 0, sizeof(e));
                e.frame = i; e.pass = p; e.rows = rows[i]; e.cols = cols[i]; e.grid = G; e.used = std::min(GG, S - p * GG);
                e.net_w = net_w_; e.net_h = net_h_;
                e.cells = d_cells + (size_t)i * S + (size_t)p * GG;
                entries.push_back(e);
            }
        }
        const int P = (int)entries.size();
        const size_t vb = (size_t)net_w_ * net_h_ * 3;
        uint8_t *d_views = rq.d_views ? (uint8_t *)rq.d_views : roi_views_.reserve(vb * (size_t)std::max(P, 1));
        PassViews v(P);
        std::vector<RoiAtlasParams> ap;
        for (int q = 0; q < P; q++) {
            const RoiEntry &e = entries[q];
            uint8_t *dst = d_views + vb * (size_t)q;
            ap.push_back(RoiAtlasParams{base[e.frame], e.rows, e.cols, st[e.frame], e.cells, e.used, e.grid, net_w_, net_h_, dst, net_w_ * 3, -2});
            v.set(q, dst, net_h_, net_w_, net_w_ * 3);
        }
        hipEvent_t packed = nullptr;
        if (P) {
            launch_roi_views(align_stream_, ap.data(), P);
            packed = record_inputs_ready();
        }
        tta_open(n, mrq.spec);
        TrackParams tp;
        memset((void *)&tp, 0, sizeof(tp));
        if (t) {
            track_open_call(*t, trq, n, cap_per_image);
            tp = track_params(*t);
            tp.streams = se; tp.n_streams = ns;
            tp.images = ie;
            tp.faces = tta_out_.ptr; tp.face_stride = (int)sizeof(Candidate); tp.faces_per_image = mrq.spec.max_faces;
            tp.counts = (const int *)tta_outcount_.ptr;
            tp.records = nullptr;
            tp.max_faces = mrq.spec.max_faces;
            t->dirty = true;                           // until track_copy_out() has run
        }
        if (P) {
            const TtaSpec msp = mrq.spec;
            auto merge = [=](hipStream_t s, const RunParams *d_params) {
                tta_launch_merge(s, n, msp, d_params);
                if (ns > 0) launch_track(s, tp);
            };
            *truncated = run_passes(what, entries, v, threshold, packed, gather_into<RoiMap>(0, tta_cand_, tta_count_, kTtaMergeCap), merge, tta_dirty_);
            tta_copy_out(n, mrq, out, cap_per_image, counts, truncated);
        } else {                                       // no image has a pass: the streams of the frames without pixels still step and age
            RF_HIP(hipStreamSynchronize(align_stream_));
            if (ns > 0) launch_track(align_stream_, tp);
            RF_HIP(hipGetLastError());
            RF_HIP(hipStreamSynchronize(align_stream_));
        }
        if (t) track_copy_out(*t, trq, n, cap_per_image, counts, cut);
        roi_track_cells_out(d_cells, plans, n, S, rq.cells);
        if (c) {
            if (rq.info) RF_HIP(hipMemcpy(rq.info, d_info, info_bytes, hipMemcpyDeviceToHost));
            c->dirty = false;
        }
    }


    // -------------------------------------------------------------------------------- low-light enhancement
    // The frames of an enhancement as the kernels take them, checked: destinations and pitches, the tile limit, and overlap -- a
    // destination may be its own source exactly (same pointer and pitch, `in_place`), and touches no other source or destination of
    // the call.  src[i] null with rows, cols > 0 (host frames that are yet to be uploaded): not compared.  Nothing has changed when
    // this throws.
    std::vector<EnhanceParams> enhance_frames(const EnhanceSpec &sp, const uint8_t *const *src, const int *rows, const int *cols,
                                              const std::vector<int> &st, int n, const std::vector<uint8_t *> &dst,
                                              const std::vector<int> &dst_st, const std::vector<char> &live, bool in_place) const {
        std::vector<EnhanceParams> fp((size_t)n);
        long long tiles = 0;
        const int lt = sp.log2_tile();
        for (int i = 0; i < n; i++) {
            memset(&fp[i], 0, sizeof(EnhanceParams));
            if (!live[i]) continue;
            if (!dst[i] || dst_st[i] < cols[i] * 3) throw ArgError("enhance: null destination or destination step < cols * 3");
            fp[i] = EnhanceParams{src[i], rows[i], cols[i], st[i], dst[i], dst_st[i], nullptr, nullptr, nullptr};
            tiles += (long long)enh_tiles(rows[i], lt) * enh_tiles(cols[i], lt);
            if (tiles > kEnhanceMaxTiles) throw ArgError("enhance: more than 262144 tiles in one call");
        }
        auto extent = [&](const uint8_t *p, int i, int step) { return (size_t)(rows[i] - 1) * step + (size_t)cols[i] * 3 + (uintptr_t)p; };
        auto meet = [](uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; };
        for (int i = 0; i < n; i++) {
            if (!live[i]) continue;
            const uintptr_t d0 = (uintptr_t)dst[i], d1 = extent(dst[i], i, dst_st[i]);
            for (int j = 0; j < n; j++) {
                if (!live[j]) continue;
                if (src[j] && meet(d0, d1, (uintptr_t)src[j], extent(src[j], j, st[j])) &&
                    !(in_place && i == j && dst[i] == src[i] && dst_st[i] == st[i]))
                    throw ArgError("enhance: a destination overlaps a source frame (only the frame itself, same pointer and pitch, is legal)");
                if (j < i && meet(d0, d1, (uintptr_t)dst[j], extent(dst[j], j, dst_st[j]))) throw ArgError("enhance: two destinations overlap");
            }
        }
        return fp;
    }

    // The two launches on the side stream: the LUT scratch (LUTs | flags | one counter per frame) grows on demand.  Returns the
    // counters (device), complete when the side stream has run what this enqueued.
    const int *enhance_launch(const EnhanceSpec &sp, std::vector<EnhanceParams> &fp) {
        const int n = (int)fp.size(), lt = sp.log2_tile();
        size_t tiles = 0;
        for (const EnhanceParams &p : fp)
            if (p.rows > 0) tiles += (size_t)enh_tiles(p.rows, lt) * enh_tiles(p.cols, lt);
        const size_t o_flags = tiles * 256, o_cnt = align256(o_flags + tiles);
        uint8_t *d = enh_luts_.reserve(o_cnt + (size_t)n * sizeof(int));
        size_t t0 = 0;
        for (int i = 0; i < n; i++) {
            if (fp[i].rows <= 0) continue;
            fp[i].luts = d + t0 * 256; fp[i].flags = d + o_flags + t0; fp[i].count = (int *)(d + o_cnt) + i;
            t0 += (size_t)enh_tiles(fp[i].rows, lt) * enh_tiles(fp[i].cols, lt);
        }
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        RF_HIP(hipMemsetAsync(d + o_cnt, 0, (size_t)n * sizeof(int), align_stream_));
        launch_enhance_lut(align_stream_, sp, fp.data(), n);
        launch_enhance_apply(align_stream_, sp, fp.data(), n);
        RF_HIP(hipGetLastError());
        return (const int *)(d + o_cnt);
    }

    void enhance(const EnhanceSpec &sp, const void *const *d_src, const int *rows, const int *cols, const int *steps, int n,
                 void *const *d_dst, const int *dst_steps, int *tiles_enhanced) override {
        if (n < 0 || (n > 0 && (!d_src || !rows || !cols || !d_dst))) throw ArgError("null argument");
        std::vector<int> st = checked_steps((const uint8_t *const *)d_src, rows, cols, steps, n), dst_st((size_t)n, 0);
        std::vector<uint8_t *> dst((size_t)n, nullptr);
        std::vector<char> live((size_t)n, 0);
        bool any = false;
        for (int i = 0; i < n; i++) {
            if (rows[i] < 0 || cols[i] < 0) throw ArgError("negative frame size");
            live[i] = d_src[i] && rows[i] > 0 && cols[i] > 0;
            any = any || live[i];
            dst[i] = (uint8_t *)d_dst[i]; dst_st[i] = dst_steps ? dst_steps[i] : cols[i] * 3;
            if (tiles_enhanced) tiles_enhanced[i] = 0;
        }
        std::vector<EnhanceParams> fp = enhance_frames(sp, (const uint8_t *const *)d_src, rows, cols, st, n, dst, dst_st, live, true);
        if (!any) return;
        DeviceGuard guard(device_);
        const int *d_counts = enhance_launch(sp, fp);
        RF_HIP(hipStreamSynchronize(align_stream_));
        if (tiles_enhanced) RF_HIP(hipMemcpy(tiles_enhanced, d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    }

    // Enhancement and detection in one call: the enhanced copies are made on the side stream in front of the call's first launch, every
    // launch waits for them on its lane stream (PassCall::inputs_ready, DESIGN.md section 24 rule 1), and detect() runs over the copies
    // as ordinary device frames -- no host wait between the two.
    void detect_enhanced(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                         float threshold, rf_face *out, int cap_per_image, int *counts, bool *truncated, const EnhanceRequest &rq) override {
        *truncated = false;
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts))) throw ArgError("null argument");
        if (cap_per_image < 0 || (cap_per_image > 0 && !out)) throw ArgError("out is null");
        std::vector<int> st = checked_steps(frames, rows, cols, steps, n), dst_st((size_t)n, 0);
        std::vector<uint8_t *> dst((size_t)n, nullptr);
        std::vector<char> live((size_t)n, 0);
        std::vector<const uint8_t *> cmp((size_t)n, nullptr);         // host frames are not compared with device destinations
        size_t own_bytes = 0;
        bool any = false;
        for (int i = 0; i < n; i++) {
            live[i] = frames[i] && rows[i] > 0 && cols[i] > 0;
            any = any || live[i];
            if (on_device) cmp[i] = frames[i];
            if (rq.tiles_enhanced) rq.tiles_enhanced[i] = 0;
            if (!live[i]) continue;
            if (rq.d_enhanced) { dst[i] = (uint8_t *)rq.d_enhanced[i]; dst_st[i] = rq.enhanced_steps ? rq.enhanced_steps[i] : cols[i] * 3; }
            else { dst[i] = (uint8_t *)(uintptr_t)(256 + own_bytes); dst_st[i] = cols[i] * 3; own_bytes += align256((size_t)rows[i] * cols[i] * 3); }
        }
        // an engine-owned destination is an offset (+ 256, so that it is not null) until the block exists: offsets never overlap
        std::vector<EnhanceParams> fp = enhance_frames(rq.spec, cmp.data(), rows, cols, st, n, dst, dst_st, live, false);
        if (!any) {
            detect(frames, rows, cols, st.data(), n, on_device, threshold, out, cap_per_image, counts, truncated);
            return;
        }
        DeviceGuard guard(device_);
        const std::vector<const uint8_t *> base = pass_frame_bases(frames, rows, cols, st, n, on_device, [&](int i) { return live[i] != 0; });
        launch_pending();
        uint8_t *own = rq.d_enhanced ? nullptr : enh_frames_.reserve(own_bytes);
        PassViews v(n);
        for (int i = 0; i < n; i++) {
            if (!live[i]) continue;
            fp[i].src = base[i]; fp[i].step = st[i];
            if (own) fp[i].dst = own + ((uintptr_t)dst[i] - 256);
            v.set(i, fp[i].dst, rows[i], cols[i], fp[i].dst_step);
        }
        int *h_counts = rq.tiles_enhanced ? (int *)enh_counts_.reserve((size_t)n * sizeof(int)) : nullptr;
        const int *d_counts = enhance_launch(rq.spec, fp);
        passes_.inputs_ready = record_inputs_ready();
        struct Clear { hipEvent_t &e; ~Clear() { e = nullptr; } } clear{passes_.inputs_ready};
        // the counters travel to pinned memory behind the event, while the detection runs
        if (h_counts) RF_HIP(hipMemcpyAsync(h_counts, d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, align_stream_));
        detect(v.ptr.data(), v.rows.data(), v.cols.data(), v.step.data(), n, true, threshold, out, cap_per_image, counts, truncated);
        RF_HIP(hipStreamSynchronize(align_stream_));
        if (h_counts) memcpy(rq.tiles_enhanced, h_counts, (size_t)n * sizeof(int));
    }

    // -------------------------------------------------------------------------------- face tracks
    void *tracker_create(const TrackSpec &spec, int n_streams) override {
        if (n_streams < 1 || n_streams > kTrackMaxStreams) throw ArgError("n_streams must be in [1, 1024]");
        if (spec.max_tracks < 1 || spec.max_tracks > kTrackMaxTracks) throw ArgError("max_tracks must be in [1, 256]");
        DeviceGuard guard(device_);
        std::unique_ptr<Tracker> t(new Tracker);
        t->spec = spec; t->n_streams = n_streams;
        t->state.reserve((size_t)n_streams * t->stream_bytes());
        try { tracker_reset_impl(*t, -1); } catch (...) { t->release(); throw; }
        trackers_.push_back(std::move(t));
        return trackers_.back().get();
    }
    void tracker_destroy(void *p) override {
        for (size_t i = 0; i < trackers_.size(); i++)
            if (trackers_[i].get() == p) {
                DeviceGuard guard(device_);
                trackers_[i]->release();
                trackers_.erase(trackers_.begin() + i);
                return;
            }
    }
    void tracker_reset(void *p, int stream) override {
        Tracker &t = tracker_of(p);
        if (stream < -1 || stream >= t.n_streams) throw ArgError("stream out of range");
        DeviceGuard guard(device_);
        tracker_reset_impl(t, stream);
        if (stream < 0) t.dirty = false;
    }
    int tracker_read(void *p, int stream, rf_track *table, int cap, int64_t *frames, int64_t *next_id, bool flush) override {
        Tracker &t = tracker_of(p);
        if (stream < 0 || stream >= t.n_streams) throw ArgError("stream out of range");
        if (cap < 0 || (cap > 0 && !table)) throw ArgError("table is null");
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        DeviceGuard guard(device_);
        std::vector<uint8_t> img(t.stream_bytes());
        uint8_t *d = t.state.ptr + (size_t)stream * t.stream_bytes();
        RF_HIP(hipMemcpy(img.data(), d, img.size(), hipMemcpyDeviceToHost));
        const TrackHeader *hd = (const TrackHeader *)img.data();
        rf_track *tr = (rf_track *)(img.data() + sizeof(TrackHeader));
        if (frames) *frames = hd->frames;
        if (next_id) *next_id = hd->next_id;
        if (!flush) {
            if (cap > 0) memcpy(table, tr, (size_t)std::min(cap, t.spec.max_tracks) * sizeof(rf_track));
            return t.spec.max_tracks;
        }
        int ended = 0;
        for (int s = 0; s < t.spec.max_tracks; s++) {
            if (tr[s].id == 0) continue;
            if (ended < cap) table[ended] = tr[s];
            ended++;
            memset(&tr[s], 0, sizeof(rf_track));
        }
        if (ended) RF_HIP(hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice));
        if (ended && t.has_motion) {                                   // every live slot was freed: the stream's records are all zero now
            RF_HIP(hipMemset(t.motion.ptr + (size_t)stream * t.motion_bytes(), 0, t.motion_bytes()));
            RF_HIP(hipDeviceSynchronize());
        }
        if (ended && t.has_follow) {
            RF_HIP(hipMemset(t.follow_records.ptr + (size_t)stream * t.follow_bytes(), 0, t.follow_bytes()));
            RF_HIP(hipDeviceSynchronize());
        }
        return ended;
    }

    void track_update(const TrackRequest &rq, int n, const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale,
                      const rf_face_quality *quality, int max_faces, bool *cut) override {
        *cut = false;
        if (n < 0 || (n > 0 && (!faces || !counts))) throw ArgError("null argument");
        if (cap_per_image < 1) throw ArgError("cap_per_image must be >= 1");
        if (max_faces < 1 || max_faces > kAlignMaxFaces) throw ArgError("max_faces must be in [1, 4096]");
        for (int i = 0; i < n; i++)
            if (counts[i] < 0) throw ArgError("negative face count");
        Tracker &t = track_check(rq, n);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int fpi = std::min(std::min(cap_per_image, max_faces), kTrackMaxFaces);      // records per image that travel to the device
        const int mq = std::min(max_faces, kTrackMaxFaces);                                 // quality records per image that do
        // one table: streams | images | counts | quality records | faces (60-byte records)
        HostTable tb;
        const size_t o_se = tb.add((size_t)n * sizeof(TrackStreamEntry)), o_img = tb.add((size_t)n * sizeof(TrackImageEntry)),
                     o_cnt = tb.add((size_t)n * sizeof(int)), o_q = tb.add(quality ? (size_t)n * mq * sizeof(rf_face_quality) : 0),
                     o_face = tb.add((size_t)n * fpi * sizeof(rf_face));
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        std::vector<float> scale(n);
        std::vector<char> empty(n, 0);
        for (int i = 0; i < n; i++) {
            cnt[i] = counts[i];            // the true count: the kernel clamps it, and tags the faces beyond the clamp
            scale[i] = coord_scale ? coord_scale[i] : 1.f;
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        if (quality) table_records(tab + o_q, mq, quality, max_faces, sizeof(rf_face_quality), cnt, std::min(fpi, mq), n);
        const int ns = track_build_table(rq.stream_of_image, 0, n, scale.data(), empty.data(), (TrackStreamEntry *)(tab + o_se),
                                         (TrackImageEntry *)(tab + o_img));
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        track_open_call(t, rq, n, cap_per_image);
        t.dirty = true;
        table_upload(d_tab, tb);
        TrackParams tp = track_params(t);
        tp.streams = (const TrackStreamEntry *)(d_tab + o_se); tp.n_streams = ns;
        tp.images = (const TrackImageEntry *)(d_tab + o_img);
        tp.faces = d_tab + o_face; tp.face_stride = (int)sizeof(rf_face); tp.faces_per_image = fpi;
        tp.counts = (const int *)(d_tab + o_cnt);
        tp.records = quality ? (const rf_face_quality *)(d_tab + o_q) : nullptr;
        tp.max_faces = mq;
        timed_launch(trk_ev_, trk_launch_ms_, [&] { launch_track(align_stream_, tp); });
        track_copy_out(t, rq, n, cap_per_image, counts, cut);
    }
    float track_last_launch_ms() const override { return trk_launch_ms_; }

    // -------------------------------------------------------------------------------- best-shot gallery
    void tracker_enable_shots(void *p, const FaceBatchSpec &spec) override {
        Tracker &t = tracker_of(p);
        FaceBatchRequest probe;
        probe.spec = spec;
        check_face_batch_request(probe);
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        if (t.has_shots) throw ArgError("the tracker has a shot gallery already");
        if (t.has_follow) throw ArgError("the tracker has follow: a gallery does not compose with it yet");
        const size_t entries = (size_t)t.n_streams * t.spec.max_tracks;
        if (entries * spec.bytes_per_face() > (size_t)RF_SHOT_MAX_BYTES) throw ArgError("shot gallery: more than RF_SHOT_MAX_BYTES");
        DeviceGuard guard(device_);
        std::vector<TrackHeader> hd((size_t)t.n_streams);
        RF_HIP(hipMemcpy2D(hd.data(), sizeof(TrackHeader), t.state.ptr, t.stream_bytes(), sizeof(TrackHeader), (size_t)t.n_streams, hipMemcpyDeviceToHost));
        for (const TrackHeader &h : hd)
            if (h.frames != 0) throw ArgError("shot gallery: the tracker has stepped a frame already");
        try {
            t.gallery.reserve(entries * spec.bytes_per_face());
            RF_HIP(hipMemset(t.shot_records.reserve(entries * sizeof(rf_shot)), 0, entries * sizeof(rf_shot)));
            RF_HIP(hipDeviceSynchronize());
        } catch (...) { t.gallery.release(); t.shot_records.release(); throw; }
        t.shot_spec = spec;
        t.has_shots = true;
    }

    // -------------------------------------------------------------------------------- motion-predicted tracks
    void tracker_enable_motion(void *p, const MotionSpec &spec) override {
        Tracker &t = tracker_of(p);
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        if (t.has_motion) throw ArgError("the tracker has motion already");
        if (t.has_follow) throw ArgError("the tracker has follow: motion does not compose with it yet");
        DeviceGuard guard(device_);
        std::vector<TrackHeader> hd((size_t)t.n_streams);
        RF_HIP(hipMemcpy2D(hd.data(), sizeof(TrackHeader), t.state.ptr, t.stream_bytes(), sizeof(TrackHeader), (size_t)t.n_streams, hipMemcpyDeviceToHost));
        for (const TrackHeader &h : hd)
            if (h.frames != 0) throw ArgError("motion: the tracker has stepped a frame already");
        const size_t bytes = (size_t)t.n_streams * t.motion_bytes();
        try {
            RF_HIP(hipMemset(t.motion.reserve(bytes), 0, bytes));
            RF_HIP(hipDeviceSynchronize());
        } catch (...) { t.motion.release(); throw; }
        t.motion_spec = spec;
        t.has_motion = true;
    }
    int tracker_read_motion(void *p, int stream, rf_track_motion *out, int cap) override {
        Tracker &t = tracker_of(p);
        if (!t.has_motion) throw ArgError("the tracker has no motion (rf_tracker_enable_motion)");
        if (stream < 0 || stream >= t.n_streams) throw ArgError("stream out of range");
        if (cap < 0 || (cap > 0 && !out)) throw ArgError("out is null");
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        DeviceGuard guard(device_);
        const int m = std::min(cap, t.spec.max_tracks);
        if (m > 0) RF_HIP(hipMemcpy(out, t.motion.ptr + (size_t)stream * t.motion_bytes(), (size_t)m * sizeof(rf_track_motion), hipMemcpyDeviceToHost));
        return t.spec.max_tracks;
    }

    // a stream's table and shot records on the host
    void shot_read_state(Tracker &t, int stream, std::vector<uint8_t> *img, std::vector<rf_shot> *rec) {
        const int T = t.spec.max_tracks;
        img->resize(t.stream_bytes());
        rec->resize((size_t)T);
        RF_HIP(hipMemcpy(img->data(), t.state.ptr + (size_t)stream * t.stream_bytes(), img->size(), hipMemcpyDeviceToHost));
        RF_HIP(hipMemcpy(rec->data(), t.shot_records.ptr + (size_t)stream * T * sizeof(rf_shot), (size_t)T * sizeof(rf_shot), hipMemcpyDeviceToHost));
    }
    // the shot of slot `slot` of a stream to the host: zeros unless the slot's track has a best shot and the record is that shot's
    void shot_fetch(Tracker &t, int stream, int slot, const rf_track &tr, const rf_shot &rec, uint8_t *shot, rf_shot *info) {
        const size_t bpf = t.shot_spec.bytes_per_face();
        const bool ok = tr.id != 0 && tr.best_frame >= 0 && shot_record_is(&rec, tr.id, tr.best_frame);
        if (info) { if (ok) *info = rec; else memset((void *)info, 0, sizeof(rf_shot)); }
        if (!shot) return;
        if (ok) RF_HIP(hipMemcpy(shot, t.gallery.ptr + ((size_t)stream * t.spec.max_tracks + slot) * bpf, bpf, hipMemcpyDeviceToHost));
        else memset(shot, 0, bpf);
    }
    Tracker &shot_tracker(void *p, int stream) {
        Tracker &t = tracker_of(p);
        if (!t.has_shots) throw ArgError("the tracker has no shot gallery (rf_tracker_enable_shots)");
        if (stream < 0 || stream >= t.n_streams) throw ArgError("stream out of range");
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        return t;
    }

    int tracker_read_shots(void *p, int stream, uint8_t *shots, rf_shot *info, int cap) override {
        Tracker &t = shot_tracker(p, stream);
        if (cap < 0) throw ArgError("cap is negative");
        const int T = t.spec.max_tracks, m = std::min(cap, T);
        if (m == 0 || (!shots && !info)) return T;
        DeviceGuard guard(device_);
        std::vector<uint8_t> img;
        std::vector<rf_shot> rec;
        shot_read_state(t, stream, &img, &rec);
        const rf_track *tr = (const rf_track *)(img.data() + sizeof(TrackHeader));
        const size_t bpf = t.shot_spec.bytes_per_face();
        for (int s = 0; s < m; s++) shot_fetch(t, stream, s, tr[s], rec[s], shots ? shots + (size_t)s * bpf : nullptr, info ? info + s : nullptr);
        return T;
    }

    int tracker_flush_shots(void *p, int stream, rf_track *ended, int cap, int64_t *frames, int64_t *next_id, uint8_t *shots, rf_shot *info) override {
        Tracker &t = shot_tracker(p, stream);
        if (cap < 0 || (cap > 0 && !ended)) throw ArgError("table is null");
        DeviceGuard guard(device_);
        std::vector<uint8_t> img;
        std::vector<rf_shot> rec;
        shot_read_state(t, stream, &img, &rec);
        const rf_track *tr = (const rf_track *)(img.data() + sizeof(TrackHeader));
        const size_t bpf = t.shot_spec.bytes_per_face();
        int e = 0;
        for (int s = 0; s < t.spec.max_tracks; s++) {                  // the order of tracker_read(flush): slot ascending
            if (tr[s].id == 0) continue;
            if (e < cap) shot_fetch(t, stream, s, tr[s], rec[s], shots ? shots + (size_t)e * bpf : nullptr, info ? info + e : nullptr);
            e++;
        }
        const int count = tracker_read(p, stream, ended, cap, frames, next_id, true);
        const size_t rb = (size_t)t.spec.max_tracks * sizeof(rf_shot);
        RF_HIP(hipMemset(t.shot_records.ptr + (size_t)stream * rb, 0, rb));
        RF_HIP(hipDeviceSynchronize());
        return count;
    }

    // the arguments of a shot call, checked before any state changes; opens the call-level blocks
    void shot_check(const Tracker &t, const ShotRequest &sq, int n, int cap_ended) {
        if (sq.d_shots && ((uintptr_t)sq.d_shots & (uintptr_t)(t.shot_spec.elem_bytes() - 1))) throw ArgError("d_shots is not aligned to its element size");
        if ((sq.d_shots || sq.shots) && (size_t)std::max(n, 0) * std::max(cap_ended, 0) * t.shot_spec.bytes_per_face() > (size_t)RF_SHOT_MAX_BYTES)
            throw ArgError("n x cap_ended shots: more than RF_SHOT_MAX_BYTES");
    }
    void shot_open_call(const Tracker &t, const ShotRequest &sq, int n, int cap_ended) {
        const size_t slots = (size_t)std::max(n, 1) * std::max(cap_ended, 1);
        call_.shot.d_out = sq.d_shots;
        call_.shot.host = sq.shots != nullptr; call_.shot.info = sq.info != nullptr;
        if (call_.shot.host) shot_out_.reserve(slots * t.shot_spec.bytes_per_face());
        if (call_.shot.info) shot_info_.reserve(slots * sizeof(rf_shot));
        call_.shot.last_streams = 0;
    }
    // The two shot launches behind a track launch on stream st (what is common to both is in sp): deliver to the caller's device block
    // and / or the pinned call-level block the kernel writes straight into, then keep.
    void shot_launches(hipStream_t st, ShotParams sp) {
        const Tracker &t = *call_.trk.tr;
        sp.max_tracks = t.spec.max_tracks;
        sp.state = t.state.ptr;
        sp.tags = (const rf_track_tag *)trk_tags_.ptr; sp.tag_stride = call_.trk.tag_stride;
        sp.ended = (const rf_track *)trk_ended_.ptr; sp.cap_ended = call_.trk.cap_ended;
        sp.ended_counts = (const int *)trk_counts_.ptr;
        sp.spec = t.shot_spec;
        sp.max_faces = call_.trk.max_faces;
        sp.gallery = t.gallery.ptr; sp.records = (rf_shot *)t.shot_records.ptr;
        sp.out_info = call_.shot.info ? (rf_shot *)shot_info_.ptr : nullptr;
        if (call_.shot.host || !call_.shot.d_out) {
            sp.out = call_.shot.host ? shot_out_.ptr : nullptr;
            launch_shot_deliver(st, sp);
            sp.out_info = nullptr;
        }
        if (call_.shot.d_out) {
            sp.out = call_.shot.d_out;
            launch_shot_deliver(st, sp);
        }
        launch_shot_keep(st, sp);
        RF_HIP(hipGetLastError());
    }
    // the delivered shots of a finished call, from the pinned blocks the deliver kernel wrote, to the caller's host buffers
    void shot_copy_out(const Tracker &t, const TrackRequest &rq, const ShotRequest &sq, int n) {
        if (!sq.shots && !sq.info) return;
        const size_t bpf = t.shot_spec.bytes_per_face();
        const int *cs = (const int *)trk_counts_.ptr;
        for (int i = 0; i < n; i++) {
            if (rq.stream_of_image[i] < 0) continue;
            const size_t have = (size_t)std::max(0, std::min(cs[i], rq.cap_ended)), at = (size_t)i * rq.cap_ended;
            if (!have) continue;
            if (sq.shots) memcpy(sq.shots + at * bpf, shot_out_.ptr + at * bpf, have * bpf);
            if (sq.info) memcpy((void *)(sq.info + at), shot_info_.ptr + at * sizeof(rf_shot), have * sizeof(rf_shot));
        }
    }

    void track_shots(const TrackRequest &rq, const ShotRequest &sq, const void *const *frames, const int *rows, const int *cols, const int *steps,
                     int n, const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, const rf_face_quality *quality,
                     bool *cut) override {
        *cut = false;
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !faces || !counts))) throw ArgError("null argument");
        if (cap_per_image < 1) throw ArgError("cap_per_image must be >= 1");
        for (int i = 0; i < n; i++)
            if (counts[i] < 0) throw ArgError("negative face count");
        Tracker &t = track_check(rq, n, true);
        shot_check(t, sq, n, rq.cap_ended);
        const int max_faces = t.shot_spec.max_faces;
        const int fpi = std::min(std::min(cap_per_image, max_faces), kTrackMaxFaces);      // records per image that travel to the device
        const int mq = std::min(max_faces, kTrackMaxFaces);                                 // quality records per image that do
        // one table: streams | images | counts | stream entry of each image | frames | quality records | faces (60-byte records)
        HostTable tb;
        const size_t o_se = tb.add((size_t)n * sizeof(TrackStreamEntry)), o_img = tb.add((size_t)n * sizeof(TrackImageEntry)),
                     o_cnt = tb.add((size_t)n * sizeof(int)), o_ent = tb.add((size_t)n * sizeof(int32_t)), o_fd = tb.add((size_t)n * sizeof(FrameDesc)),
                     o_q = tb.add(quality ? (size_t)n * mq * sizeof(rf_face_quality) : 0), o_face = tb.add((size_t)n * fpi * sizeof(rf_face));
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        std::vector<float> scale((size_t)n);
        const std::vector<char> empty = table_frames((FrameDesc *)(tab + o_fd), frames, rows, cols, steps, n, "shots");
        for (int i = 0; i < n; i++) {
            cnt[i] = empty[i] ? 0 : counts[i];      // the true count: the kernel clamps it, and tags the faces beyond the clamp; a frame
            scale[i] = coord_scale ? coord_scale[i] : 1.f;      // without pixels has no faces
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        if (quality) table_records(tab + o_q, mq, quality, max_faces, sizeof(rf_face_quality), cnt, std::min(fpi, mq), n);
        if (n == 0) return;
        DeviceGuard guard(device_);
        TrackStreamEntry *se = (TrackStreamEntry *)(tab + o_se);
        const int ns = track_build_table(rq.stream_of_image, 0, n, scale.data(), empty.data(), se, (TrackImageEntry *)(tab + o_img));
        int32_t *ent = (int32_t *)(tab + o_ent);
        int n_img = 0;
        for (int z = 0; z < ns; z++)
            for (int j = 0; j < se[z].n; j++) ent[n_img++] = z;
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        track_open_call(t, rq, n, cap_per_image);
        shot_open_call(t, sq, n, rq.cap_ended);
        t.dirty = true;
        table_upload(d_tab, tb);
        TrackParams tp = track_params(t);
        tp.streams = (const TrackStreamEntry *)(d_tab + o_se); tp.n_streams = ns;
        tp.images = (const TrackImageEntry *)(d_tab + o_img);
        tp.faces = d_tab + o_face; tp.face_stride = (int)sizeof(rf_face); tp.faces_per_image = fpi;
        tp.counts = (const int *)(d_tab + o_cnt);
        tp.records = quality ? (const rf_face_quality *)(d_tab + o_q) : nullptr;
        tp.max_faces = mq;
        call_.trk.max_faces = mq;
        launch_track(align_stream_, tp);
        RF_HIP(hipGetLastError());
        ShotParams sp;
        memset((void *)&sp, 0, sizeof(sp));
        sp.streams = tp.streams; sp.n_streams = ns;
        sp.images = tp.images; sp.n_images = n_img;
        sp.entry_of = (const int32_t *)(d_tab + o_ent);
        sp.frames = (const FrameDesc *)(d_tab + o_fd);
        sp.faces = tp.faces; sp.face_stride = tp.face_stride; sp.faces_per_image = fpi;
        sp.counts = tp.counts;
        timed_launch(shot_ev_, shot_launch_ms_, [&] { if (ns > 0) shot_launches(align_stream_, sp); });
        track_copy_out(t, rq, n, cap_per_image, cnt, cut);
        shot_copy_out(t, rq, sq, n);
    }
    float shot_last_launch_ms() const override { return shot_launch_ms_; }

    // -------------------------------------------------------------------------------- followed tracks
    void tracker_enable_follow(void *p, const FollowSpec &spec) override {
        Tracker &t = tracker_of(p);
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        if (t.has_follow) throw ArgError("the tracker has follow already");
        if (t.has_shots || t.has_motion) throw ArgError("follow does not compose with a shot gallery or motion yet");
        const size_t entries = (size_t)t.n_streams * t.spec.max_tracks;
        if (entries * kFollowCells > (size_t)RF_SHOT_MAX_BYTES) throw ArgError("follow: more than RF_SHOT_MAX_BYTES of templates");
        DeviceGuard guard(device_);
        std::vector<TrackHeader> hd((size_t)t.n_streams);
        RF_HIP(hipMemcpy2D(hd.data(), sizeof(TrackHeader), t.state.ptr, t.stream_bytes(), sizeof(TrackHeader), (size_t)t.n_streams, hipMemcpyDeviceToHost));
        for (const TrackHeader &h : hd)
            if (h.frames != 0) throw ArgError("follow: the tracker has stepped a frame already");
        try {
            RF_HIP(hipMemset(t.follow_templates.reserve(entries * kFollowCells), 0, entries * kFollowCells));
            RF_HIP(hipMemset(t.follow_records.reserve(entries * sizeof(rf_track_follow)), 0, entries * sizeof(rf_track_follow)));
            RF_HIP(hipDeviceSynchronize());
        } catch (...) { t.follow_templates.release(); t.follow_records.release(); throw; }
        t.follow_spec = spec;
        t.has_follow = true;
    }
    int tracker_read_follow(void *p, int stream, rf_track_follow *records, uint8_t *templates, int cap) override {
        Tracker &t = tracker_of(p);
        if (!t.has_follow) throw ArgError("the tracker has no follow (rf_tracker_enable_follow)");
        if (stream < 0 || stream >= t.n_streams) throw ArgError("stream out of range");
        if (cap < 0) throw ArgError("cap is negative");
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        const int T = t.spec.max_tracks, m = std::min(cap, T);
        if (m == 0 || (!records && !templates)) return T;
        DeviceGuard guard(device_);
        std::vector<rf_track_follow> rec((size_t)m);
        RF_HIP(hipMemcpy(rec.data(), t.follow_records.ptr + (size_t)stream * t.follow_bytes(), (size_t)m * sizeof(rf_track_follow), hipMemcpyDeviceToHost));
        if (records) memcpy(records, rec.data(), (size_t)m * sizeof(rf_track_follow));
        if (templates) {
            RF_HIP(hipMemcpy(templates, t.follow_templates.ptr + (size_t)stream * T * kFollowCells, (size_t)m * kFollowCells, hipMemcpyDeviceToHost));
            for (int s = 0; s < m; s++)
                if (!rec[s].valid) memset(templates + (size_t)s * kFollowCells, 0, kFollowCells);
        }
        return T;
    }
    // what every follow launch takes from the tracker and the open call's result blocks
    FollowParams follow_params(const Tracker &t) const {
        FollowParams fp;
        memset((void *)&fp, 0, sizeof(fp));
        fp.spec = t.spec; fp.fspec = t.follow_spec;
        fp.state = t.state.ptr;
        fp.records = (rf_track_follow *)t.follow_records.ptr;
        fp.templates = t.follow_templates.ptr;
        fp.tags = (rf_track_tag *)trk_tags_.ptr; fp.tag_stride = call_.trk.tag_stride;
        fp.ended = (rf_track *)trk_ended_.ptr; fp.cap_ended = call_.trk.cap_ended;
        fp.ended_counts = (int *)trk_counts_.ptr;
        fp.status = (int *)trk_counts_.ptr + std::max(call_.trk.n, 1);
        return fp;
    }

    // a key step over faces the caller supplies: track_update() against device-resident frames + the keep launch
    void track_follow_update(const TrackRequest &rq, const void *const *frames, const int *rows, const int *cols, const int *steps, int n,
                             const rf_face *faces, int cap_per_image, const int *counts, const float *coord_scale, const rf_face_quality *quality,
                             bool *cut) override {
        *cut = false;
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !faces || !counts))) throw ArgError("null argument");
        if (cap_per_image < 1) throw ArgError("cap_per_image must be >= 1");
        for (int i = 0; i < n; i++)
            if (counts[i] < 0) throw ArgError("negative face count");
        Tracker &t = track_check(rq, n, false, true);
        const int max_faces = opt_.max_detections;
        const int fpi = std::min(std::min(cap_per_image, max_faces), kTrackMaxFaces);      // records per image that travel to the device
        const int mq = std::min(max_faces, kTrackMaxFaces);                                 // quality records per image that do
        // one table: streams | images | counts | frames | quality records | faces (60-byte records)
        HostTable tb;
        const size_t o_se = tb.add((size_t)n * sizeof(TrackStreamEntry)), o_img = tb.add((size_t)n * sizeof(TrackImageEntry)),
                     o_cnt = tb.add((size_t)n * sizeof(int)), o_fd = tb.add((size_t)n * sizeof(FrameDesc)),
                     o_q = tb.add(quality ? (size_t)n * mq * sizeof(rf_face_quality) : 0), o_face = tb.add((size_t)n * fpi * sizeof(rf_face));
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        std::vector<float> scale((size_t)n);
        const std::vector<char> empty = table_frames((FrameDesc *)(tab + o_fd), frames, rows, cols, steps, n, "follow");
        for (int i = 0; i < n; i++) {
            cnt[i] = empty[i] ? 0 : counts[i];      // a frame without pixels has no faces
            scale[i] = coord_scale ? coord_scale[i] : 1.f;
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        if (quality) table_records(tab + o_q, mq, quality, max_faces, sizeof(rf_face_quality), cnt, std::min(fpi, mq), n);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int ns = track_build_table(rq.stream_of_image, 0, n, scale.data(), empty.data(), (TrackStreamEntry *)(tab + o_se),
                                         (TrackImageEntry *)(tab + o_img));
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        track_open_call(t, rq, n, cap_per_image);
        t.dirty = true;
        table_upload(d_tab, tb);
        TrackParams tp = track_params(t);
        tp.streams = (const TrackStreamEntry *)(d_tab + o_se); tp.n_streams = ns;
        tp.images = (const TrackImageEntry *)(d_tab + o_img);
        tp.faces = d_tab + o_face; tp.face_stride = (int)sizeof(rf_face); tp.faces_per_image = fpi;
        tp.counts = (const int *)(d_tab + o_cnt);
        tp.records = quality ? (const rf_face_quality *)(d_tab + o_q) : nullptr;
        tp.max_faces = mq;
        launch_track(align_stream_, tp);
        RF_HIP(hipGetLastError());
        FollowParams fp = follow_params(t);
        fp.streams = tp.streams; fp.n_streams = ns;
        fp.images = tp.images;
        fp.frames = (const FrameDesc *)(d_tab + o_fd);
        launch_follow_keep(align_stream_, fp);
        RF_HIP(hipGetLastError());
        RF_HIP(hipStreamSynchronize(align_stream_));
        track_copy_out(t, rq, n, cap_per_image, cnt, cut);
    }

    // a follow step: the search and step launches over the frames alone
    void track_follow(const TrackRequest &rq, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
                      rf_face *out, int cap_per_image, int *counts, bool *cut) override {
        *cut = false;
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts))) throw ArgError("null argument");
        if (cap_per_image < 0 || (cap_per_image > 0 && !out)) throw ArgError("out is null");
        if ((long)n * std::max(cap_per_image, 1) > (1L << 24)) throw ArgError("n x cap_per_image: more than 2^24 faces in one call");
        Tracker &t = track_check(rq, n, false, true);
        if (!on_device)
            for (int i = 0; i < n; i++) check_frame(frames[i], rows[i], cols[i], steps ? steps[i] : cols[i] * 3);
        // one table: streams | images | frames
        HostTable tb;
        const size_t o_se = tb.add((size_t)n * sizeof(TrackStreamEntry)), o_img = tb.add((size_t)n * sizeof(TrackImageEntry)),
                     o_fd = tb.add((size_t)n * sizeof(FrameDesc));
        DeviceGuard guard(device_);
        std::vector<const uint8_t *> dev;
        std::vector<int> dense;
        if (!on_device && n > 0) {                     // the dense upload of the redacting host call; nothing is copied back
            dev = redact_upload(frames, rows, cols, steps, n, nullptr, nullptr);
            dense.resize((size_t)n);
            for (int i = 0; i < n; i++) dense[i] = cols[i] * 3;
            frames = dev.data(); steps = dense.data();
        }
        uint8_t *tab = table_open(tb);
        const std::vector<char> empty = table_frames((FrameDesc *)(tab + o_fd), (const void *const *)frames, rows, cols, steps, n, on_device ? "follow" : nullptr);
        if (n == 0) return;
        const std::vector<float> scale((size_t)n, 1.f);
        const int ns = track_build_table(rq.stream_of_image, 0, n, scale.data(), empty.data(), (TrackStreamEntry *)(tab + o_se),
                                         (TrackImageEntry *)(tab + o_img));
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        track_open_call(t, rq, n, cap_per_image);
        // followed faces of the call | their counts, pinned: the step kernel writes them; an image no workgroup serves has none
        const size_t o_cnt = align256((size_t)n * std::max(cap_per_image, 1) * sizeof(rf_face));
        uint8_t *h_out = fol_out_.reserve(o_cnt + (size_t)n * sizeof(int));
        int *h_cnt = (int *)(h_out + o_cnt);
        memset(h_cnt, 0, (size_t)n * sizeof(int));
        memset(trk_counts_.ptr, 0, (size_t)n * 2 * sizeof(int));
        t.dirty = true;
        table_upload(d_tab, tb);
        FollowParams fp = follow_params(t);
        fp.streams = (const TrackStreamEntry *)(d_tab + o_se); fp.n_streams = ns;
        fp.images = (const TrackImageEntry *)(d_tab + o_img);
        fp.frames = (const FrameDesc *)(d_tab + o_fd);
        fp.results = (FollowResult *)fol_results_.reserve((size_t)std::max(ns, 1) * t.spec.max_tracks * sizeof(FollowResult));
        fp.out = (rf_face *)h_out; fp.cap_per_image = cap_per_image;
        fp.counts = h_cnt;
        float ms = -1.f;
        timed_launch(fol_ev_, ms, [&] { launch_follow_search(align_stream_, fp); launch_follow_step(align_stream_, fp); });
        if (on_device) fol_launch_ms_ = ms;
        for (int i = 0; i < n; i++) {
            counts[i] = h_cnt[i];
            const int have = std::min(h_cnt[i], cap_per_image);
            if (have > 0) memcpy((void *)(out + (size_t)i * cap_per_image), h_out + (size_t)i * cap_per_image * sizeof(rf_face), (size_t)have * sizeof(rf_face));
        }
        track_copy_out(t, rq, n, cap_per_image, counts, cut);
    }
    float follow_last_launch_ms() const override { return fol_launch_ms_; }

    // -------------------------------------------------------------------------------- face redaction
    // The arguments of a redacting call, checked before any state changes: the tracker and its streams (each at most once per call:
    // the coasting regions of a stream belong to one frame), the frames (in-place writes: no two frames of a call may share a byte,
    // and a frame resident on another device would be redacted in its staged copy, not where the caller holds it).
    void *redact_check(const RedactRequest &rq, const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                          bool on_device) {
        if (n < 0 || (n > 0 && (!frames || !rows || !cols))) throw ArgError("null argument");
        if (rq.spec.max_regions < 1 || rq.spec.max_regions > kRedactMaxRegions) throw ArgError("max_regions must be in [1, 1024]");
        if ((size_t)std::max(n, 1) * rq.spec.max_regions * rq.spec.cells * rq.spec.cells > ((size_t)1 << 28))
            throw ArgError("n x max_regions x cells^2: more than 2^28 cells in one call");
        const std::string who = rq.overlay ? "overlay" : "redaction", verb = rq.overlay ? "drawn into" : "redacted";
        auto *t = rq.tracker ? &tracker_of(rq.tracker) : nullptr;
        if (t) {
            if (t->dirty) throw ArgError("the tracker's last call failed: reset it first");
            if (n > 0 && !rq.stream_of_image) throw ArgError("stream_of_image is null");
            std::vector<int> seen;
            for (int i = 0; i < n; i++) {
                const int st = rq.stream_of_image[i];
                if (st < -1 || st >= t->n_streams) throw ArgError("stream_of_image: stream out of range");
                if (st >= 0) seen.push_back(st);
            }
            std::sort(seen.begin(), seen.end());
            if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) throw ArgError(who + ": a stream appears more than once in the call");
        }
        std::vector<std::pair<uintptr_t, uintptr_t>> span;
        for (int i = 0; i < n; i++) {
            const int st = steps ? steps[i] : cols[i] * 3;
            check_frame(frames[i], rows[i], cols[i], st);
            if (!frames[i] || rows[i] <= 0 || cols[i] <= 0) continue;
            if (on_device && check_residency_) {
                const int where = foreign_device_of(frames[i]);
                if (where >= 0 && where != device_) throw Unsupported(who + ": a frame is resident on another device (its staged copy would be " + verb + ", not the frame)");
            }
            span.emplace_back((uintptr_t)frames[i], (uintptr_t)frames[i] + (size_t)(rows[i] - 1) * st + (size_t)cols[i] * 3);
        }
        std::sort(span.begin(), span.end());
        for (size_t j = 1; j < span.size(); j++)
            if (span[j].first < span[j - 1].second) throw ArgError(who + ": two frames of the call overlap in memory");
        return t;
    }

    // device blocks of a redacting call, sized once and reused; the region counts (after | before the cut) and the owned-pixel counts
    // share one block, so the results of a call come back in one copy.  A blurring call also gets its shadow: behind a table of one
    // offset per call image, rows x cols x 3 bytes for every frame of the call -- sized from what the host knows, whatever the faces
    // turn out to be; the block grows to the largest call seen.  (No launch of an earlier call is in flight: every redacting call
    // waits for its last launch before it returns.)
    void redact_open(const RedactRequest &rq, void *tracker, int n, const uint8_t *const *frames, const int *rows, const int *cols) {
        const size_t slots = (size_t)std::max(n, 1) * rq.spec.max_regions;
        if (rq.overlay) ov_regions_.reserve(slots * sizeof(OverlayRegion));
        else red_regions_.reserve(slots * sizeof(RedactRegion));
        red_counts_.reserve(((size_t)std::max(n, 1) * 2 + slots) * sizeof(int));
        if (!rq.overlay && rq.spec.mode == RF_REDACT_PIXELATE && !rq.spec.blur) red_cells_.reserve(slots * rq.spec.cells * rq.spec.cells * sizeof(uint32_t));
        if (rq.spec.blur && n > 0) {
            red_shadow_off_.assign((size_t)n, 0);
            size_t bytes = align256((size_t)n * sizeof(unsigned long long));
            for (int i = 0; i < n; i++) {
                red_shadow_off_[i] = bytes;
                if (frames[i] && rows[i] > 0 && cols[i] > 0) bytes += align256((size_t)rows[i] * cols[i] * 3);
            }
            uint8_t *d = red_shadow_.reserve(bytes);
            RF_HIP(hipMemcpy(d, red_shadow_off_.data(), (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice));
        }
        call_.red.spec = rq.spec; call_.red.tr = tracker ? &tracker_of(tracker) : nullptr; call_.red.stream_of_image = rq.stream_of_image;
        call_.red.n = n;
        call_.red.overlay = rq.overlay; call_.red.ospec = rq.ospec;
    }
    // (the overlay part stays zero in a redacting call, whose launches take the RedactParams part alone)
    OverlayParams redact_params() const {
        OverlayParams rp;
        memset((void *)&rp, 0, sizeof(rp));
        rp.spec = call_.red.spec;
        if (call_.red.overlay) { rp.ospec = call_.red.ospec; rp.oregions = (OverlayRegion *)ov_regions_.ptr; }
        if (call_.red.tr) {
            rp.track_state = call_.red.tr->state.ptr;
            rp.max_tracks = call_.red.tr->spec.max_tracks;
            rp.coast = redact_coast(call_.red.spec.coast, call_.red.tr->spec.max_missed);
            if (call_.red.tr->has_motion) { rp.motion = (const rf_track_motion *)call_.red.tr->motion.ptr; rp.horizon = call_.red.tr->motion_spec.horizon; }
        }
        rp.regions = (RedactRegion *)red_regions_.ptr;
        rp.nreg = (int *)red_counts_.ptr; rp.true_counts = (int *)red_counts_.ptr + std::max(call_.red.n, 1);
        rp.cell_values = (uint32_t *)red_cells_.ptr;
        rp.pixels = (int *)red_counts_.ptr + 2 * std::max(call_.red.n, 1);
        if (call_.red.spec.blur) { rp.shadow = red_shadow_.ptr; rp.shadow_off = (const unsigned long long *)red_shadow_.ptr; }
        return rp;
    }
    void redact_launch(hipStream_t st, const OverlayParams &rp) const {
        if (call_.red.overlay) {
            launch_overlay_regions(st, rp);
            launch_overlay_draw(st, rp);
            return;
        }
        launch_redact_regions(st, rp);
        if (rp.spec.blur) launch_redact_blur(st, rp);
        else launch_redact_mean(st, rp);
        launch_redact_write(st, rp);
    }
    // results of a finished redacting call (the host has waited for its last launch)
    void redact_copy_out(const RedactRequest &rq, int n, bool *cut) {
        if (n == 0) return;
        const size_t px = rq.pixels ? (size_t)n * rq.spec.max_regions : 0;
        red_host_.resize(2 * (size_t)n + px);
        RF_HIP(hipMemcpy(red_host_.data(), red_counts_.ptr, red_host_.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            if (red_host_[n + i] > rq.spec.max_regions) *cut = true;
            if (rq.region_counts) rq.region_counts[i] = red_host_[n + i];
        }
        if (px) memcpy(rq.pixels, red_host_.data() + 2 * (size_t)n, px * sizeof(int));
    }

    void redact(const void *const *frames, const int *rows, const int *cols, const int *steps, int n, const rf_face *faces, int cap_per_image,
                const int *counts, const float *coord_scale, const RedactRequest &rq, bool *cut) override {
        *cut = false;
        if (n < 0 || (n > 0 && (!counts || (!faces && cap_per_image > 0)))) throw ArgError("null argument");
        if (cap_per_image < 0) throw ArgError("cap_per_image must be >= 0");
        for (int i = 0; i < n; i++)
            if (counts[i] < 0 || counts[i] > cap_per_image) throw ArgError("counts[i] must be in [0, cap_per_image]");
        void *t = redact_check(rq, (const uint8_t *const *)frames, rows, cols, steps, n, true);
        if (n == 0) return;
        DeviceGuard guard(device_);
        const int fpi = std::max(1, std::min(cap_per_image, rq.spec.max_regions));      // records per image that travel to the device
        // one table: frames | counts | scales | streams | faces (60-byte records) | with ids, one int64 per face
        const bool with_ids = rq.overlay && rq.ids;
        HostTable tb;
        const size_t o_fd = tb.add((size_t)n * sizeof(FrameDesc)), o_cnt = tb.add((size_t)n * sizeof(int)), o_sc = tb.add((size_t)n * sizeof(float)),
                     o_st = tb.add((size_t)n * sizeof(int)), o_face = tb.add((size_t)n * fpi * sizeof(rf_face)),
                     o_id = with_ids ? tb.add((size_t)n * fpi * sizeof(int64_t)) : 0;
        uint8_t *tab = table_open(tb);
        int *cnt = (int *)(tab + o_cnt);
        float *sc = (float *)(tab + o_sc);
        int *strm = (int *)(tab + o_st);
        table_frames((FrameDesc *)(tab + o_fd), frames, rows, cols, steps, n, nullptr);      // checked by redact_check()
        for (int i = 0; i < n; i++) {
            cnt[i] = counts[i];             // the true count: the kernel cuts the list and reports its length
            sc[i] = coord_scale ? coord_scale[i] : 1.f;
            strm[i] = t ? rq.stream_of_image[i] : -1;
        }
        table_records(tab + o_face, fpi, faces, cap_per_image, sizeof(rf_face), cnt, fpi, n);
        if (with_ids) table_records(tab + o_id, fpi, rq.ids, cap_per_image, sizeof(int64_t), cnt, fpi, n);
        uint8_t *d_tab = align_tab_.reserve(tb.end);
        redact_open(rq, t, n, (const uint8_t *const *)frames, rows, cols);
        table_upload(d_tab, tb);
        OverlayParams rp = redact_params();
        rp.frames = (const FrameDesc *)(d_tab + o_fd);
        rp.faces = d_tab + o_face; rp.face_stride = (int)sizeof(rf_face); rp.faces_per_image = fpi;
        if (with_ids) { rp.ids = d_tab + o_id; rp.id_stride = (int)sizeof(int64_t); rp.ids_per_image = fpi; }
        rp.counts = (const int *)(d_tab + o_cnt); rp.count_cap = 0x7fffffff;
        rp.scale = (const float *)(d_tab + o_sc);
        rp.streams = t ? (const int *)(d_tab + o_st) : nullptr;
        rp.n = n; rp.image0 = 0;
        timed_launch(red_ev_, rq.overlay ? ov_launch_ms_ : red_launch_ms_, [&] { redact_launch(align_stream_, rp); });
        redact_copy_out(rq, n, cut);
    }
    float redact_last_launch_ms() const override { return red_launch_ms_; }
    float overlay_last_launch_ms() const override { return ov_launch_ms_; }

    // -------------------------------------------------------------------------------- stage calls
    // Host frames of a redacting call, uploaded once, densely, each at a 256-byte-aligned offset of one block: detection and redaction run
    // on that copy (dev[i], rows of cols * 3 bytes), which goes to out_bgr[i] when the call has ended
    std::vector<const uint8_t *> redact_upload(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n,
                                               uint8_t *const *out_bgr, const int *out_steps) {
        std::vector<const uint8_t *> dev((size_t)n, nullptr);
        size_t bytes = 0;
        std::vector<size_t> off((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            if (!frames[i] || rows[i] <= 0 || cols[i] <= 0) continue;
            if (out_bgr && !out_bgr[i]) throw ArgError("out_bgr[i] is null");      // (out_bgr null: a follow step, nothing goes back)
            if (out_bgr && out_steps && out_steps[i] < cols[i] * 3) throw ArgError("out_steps[i] smaller than cols*3");
            off[i] = bytes; bytes += align256((size_t)rows[i] * cols[i] * 3);
        }
        uint8_t *d = red_frames_.reserve(bytes);
        for (int i = 0; i < n; i++) {
            if (!frames[i] || rows[i] <= 0 || cols[i] <= 0) continue;
            RF_HIP(hipMemcpy2D(d + off[i], (size_t)cols[i] * 3, frames[i], steps ? (size_t)steps[i] : (size_t)cols[i] * 3, (size_t)cols[i] * 3,
                               (size_t)rows[i], hipMemcpyHostToDevice));
            dev[i] = d + off[i];
        }
        return dev;
    }

    // The fused calls (StageCall): detect() with the call's stages armed behind every launch (launch_pending()).  Everything a stage
    // needs is bound when the call opens; the launch path does not know which of the eight calls it serves.
    void detect_staged(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device, float threshold,
                       rf_face *out, int cap_per_image, int *counts, bool *truncated, const StageCall &sc, StageResult *res) override {
        *res = StageResult{};
        const AlignRequest *al = sc.align;
        const FaceBatchRequest *fb = sc.face_batch;
        const TrackRequest *trq = sc.track;
        const ShotRequest *sq = sc.shots;
        const RedactRequest *rq = sc.redact;
        static const int kSets[8] = {1, 2, 4, 4 | 2, 4 | 8, 16, 4 | 16, 4 | 32};
        const int set = (al ? 1 : 0) | (fb ? 2 : 0) | (trq ? 4 : 0) | (sq ? 8 : 0) | (rq ? 16 : 0) | (sc.follow ? 32 : 0);
        if (std::find(kSets, kSets + 8, set) == kSets + 8) throw ArgError("stage call: not a set of stages that run together");
        // every check before any state changes; a call with two defects reports the one it always has
        if (al) check_align_request(*al);
        if (fb) check_face_batch_request(*fb);
        if (n < 0 || (n > 0 && (!frames || !rows || !cols || !counts))) throw ArgError("null argument");
        if ((trq || rq) && (cap_per_image < 0 || (cap_per_image > 0 && !out))) throw ArgError("out is null");      // (otherwise detect() refuses it)
        if (al && (long)n * al->max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 crop slots in one call");
        if (fb && (long)n * fb->spec.max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 faces in one call");
        if (rq && !trq) {
            if (rq->tracker) throw ArgError("redaction: the tracked form is detect_track_redact");
            if (!on_device && n > 0 && !sc.out_bgr) throw ArgError("out_bgr is null");
        } else if (rq) {
            if (!rq->tracker || rq->tracker != trq->tracker || rq->stream_of_image != trq->stream_of_image) throw ArgError("redaction: not the tracked call's tracker");
            if (!on_device) throw ArgError("redaction: the tracked call takes frames in device memory");
        }
        Tracker *t = trq ? &track_check(*trq, n, sq != nullptr, sc.follow) : nullptr;
        // shots: the quality launch of the gated face-batch path, for the gallery spec, no tensor; it runs only under a gate, the frame
        // steps read max_faces from it either way
        FaceBatchRequest shot_fb;
        if (sq) {
            shot_check(*t, *sq, n, trq->cap_ended);
            shot_fb.spec = t->shot_spec;
            shot_fb.spec.capacity = std::max(1, n) * shot_fb.spec.max_faces;
            shot_fb.gated = sq->gated; shot_fb.has_gate = sq->has_gate; shot_fb.gate = sq->gate; shot_fb.quality = sq->quality;
            if ((long)n * shot_fb.spec.max_faces > (1L << 24)) throw ArgError("n x max_faces: more than 2^24 faces in one call");
            if (sq->gated) fb = &shot_fb;
        }
        const FaceBatchRequest *records_of = sq ? &shot_fb : fb;      // whose quality records and max_faces the frame steps read
        if (rq) redact_check(*rq, frames, rows, cols, steps, n, on_device);
        DeviceGuard guard(device_);
        std::vector<const uint8_t *> dev;
        std::vector<int> dense;
        const bool uploaded = rq && !on_device;
        if (uploaded) {
            dev = redact_upload(frames, rows, cols, steps, n, sc.out_bgr, sc.out_steps);
            dense.resize((size_t)std::max(n, 1));
            for (int i = 0; i < n; i++) dense[i] = cols[i] * 3;
            frames = dev.data(); steps = dense.data(); on_device = true;
        }
        // a super-batch of earlier enqueues that is still being assembled starts now: from here on every launch carries images of
        // this call only, in call order, so image i of a launch is image call_.next_image + i of the call for every stage
        launch_pending();
        call_.who = trq ? "face tracks" : rq ? "redaction" : fb ? "face batch" : "face alignment";
        call_.n = n; call_.next_image = 0;
        if (al) { call_.align.rq = *al; align_open(*al, n, &call_.align.d_crops, &call_.align.d_mats); }
        // full tags: the shot kernels find faces by their tags, and an overlay reads every face's id from its tag, whatever the caller's cap is
        if (trq) track_open_call(*t, *trq, n, cap_per_image, sq || (rq && rq->overlay));
        if (sq) shot_open_call(*t, *sq, n, trq->cap_ended);
        if (fb) {
            call_.fb.rq = *fb;
            face_batch_open(*fb, &call_.fb.d_tensor, &call_.fb.d_mats);
            if (fb->gated) face_gate_open(*fb, n);
            call_.fb.first = true; call_.fb.prev_scan = nullptr;
        }
        if (trq) {
            call_.trk.records = records_of && records_of->gated ? (const rf_face_quality *)fq_records_.ptr : nullptr;
            call_.trk.max_faces = records_of ? records_of->spec.max_faces : kTrackMaxFaces;
        }
        if (rq) redact_open(*rq, trq ? rq->tracker : nullptr, n, frames, rows, cols);
        if (t) t->dirty = true;                        // until track_copy_out() has run: an error in between leaves the tracker refused
        struct Disarm { StageOpen &c; ~Disarm() { c.disarm(); } } disarm{call_};
        call_.align.on = al && (call_.align.d_crops || call_.align.d_mats);
        call_.fb.on = fb != nullptr;
        call_.trk.on = trq && n > 0; call_.shot.on = sq && n > 0; call_.red.on = rq && n > 0; call_.follow.on = sc.follow && n > 0;
        const bool armed = call_.armed();
        detect(frames, rows, cols, steps, n, on_device, threshold, out, cap_per_image, counts, truncated);
        call_.disarm();
        if (armed && call_.next_image != n)
            throw HipError(rq ? "redaction: a launch of the call was not redacted" : std::string(call_.who) + ": a launch of the call was not served");
        // every launch of the call has been waited for (its `done` event follows the launches of its stages); an empty frame has count 0
        if (al) align_copy_out(*al, call_.align.d_crops, call_.align.d_mats, n, counts, opt_.max_detections);
        if (fb) {
            const int limit = std::min(fb->spec.max_faces, opt_.max_detections);
            bool over = false;
            if (fb->gated) face_gated_copy_out(*fb, call_.fb.d_tensor, call_.fb.d_mats, counts, n, limit, &over);
            else face_batch_copy_out(*fb, call_.fb.d_tensor, call_.fb.d_mats, counts, n, limit, &over);
            res->overflow = over && !sq;
        }
        if (trq) track_copy_out(*t, *trq, n, cap_per_image, counts, &res->track_cut);
        if (sq) shot_copy_out(*t, *trq, *sq, n);
        if (rq) redact_copy_out(*rq, n, &res->redact_cut);
        if (uploaded)
            for (int i = 0; i < n; i++)
                if (dev[i]) RF_HIP(hipMemcpy2D(sc.out_bgr[i], sc.out_steps ? (size_t)sc.out_steps[i] : (size_t)cols[i] * 3, dev[i], (size_t)cols[i] * 3,
                                               (size_t)cols[i] * 3, (size_t)rows[i], hipMemcpyDeviceToHost));
    }

    void host_register(const void *ptr, size_t bytes) override {
        if (!ptr || !bytes) throw ArgError("host_register: null / empty range");
        DeviceGuard guard(device_);
        RF_HIP(hipHostRegister((void *)ptr, bytes, hipHostRegisterPortable));
        registered_.push_back(HostRange{(uintptr_t)ptr, bytes, true});
    }
    void host_adopt(const void *ptr, size_t bytes) override {
        if (!ptr || !bytes) throw ArgError("host_register: null / empty range");
        registered_.push_back(HostRange{(uintptr_t)ptr, bytes, false});
    }
    void host_unregister(const void *ptr) override { drop_range(ptr, true); }
    void host_forget(const void *ptr) override { drop_range(ptr, false); }
    void invalidate_residency() override { residency_.clear(); }
    void scatter_stats(long long *frames, long long *copies) const override { *frames += scattered_frames_; *copies += peer_copies_; }
    void launch_stats(long long *launches, long long *images) const override { *launches += launches_; *images += launched_images_; }

    // tickets the caller may keep outstanding before it has to wait: every lane can hold a full super-batch
    int num_slots() const override { return (int)lanes_.size() * opt_.coalesce; }

    int last_anchor_indices(int image, int32_t *out, int cap) const override {
        if (image < 0 || image >= last_n_) throw ArgError("image index out of range");
        if (cap > 0 && !out) throw ArgError("null argument");
        int n = (int)last_anchor_[image].size();
        for (int i = 0; i < std::min(n, cap); i++) out[i] = last_anchor_[image][i];
        return n;
    }
    int last_candidate_counts(int *counts, int n) const override {
        if (n > 0 && !counts) throw ArgError("null argument");
        for (int i = 0; i < std::min(n, last_n_); i++) counts[i] = last_cand_counts_[i];
        return last_n_;
    }
    void last_timings(float *pre, float *infer, float *post, float *total) const override {
        if (pre) *pre = have_split_ ? t_pre_ : -1.f;
        if (infer) *infer = have_split_ ? t_infer_ : -1.f;
        if (post) *post = have_split_ ? t_post_ : -1.f;
        if (total) *total = have_split_ ? t_total_ : -1.f;
    }

    long get_output(const std::string &blob, int image, float *dst, size_t cap) override {
        if (!opt_.keep_outputs) throw ArgError("rf_get_output needs options.keep_outputs = 1");
        DeviceGuard guard(device_);
        static const char *kinds[3] = {"face_rpn_cls_prob_reshape_stride", "face_rpn_bbox_pred_stride",
                                       "face_rpn_landmark_pred_stride"};
        const int chans[3] = {2 * kind_.head_a, 4 * kind_.head_a, 10 * kind_.head_a};
        Lane &l = lanes_[last_lane_];
        for (int si = 0; si < 3; si++)
            for (int k = 0; k < 3; k++) {
                if (blob != std::string(kinds[k]) + std::to_string(kStrides[si])) continue;
                if (image < 0 || image >= last_n_ || last_first_image_ < 0) throw ArgError("image index out of range");
                size_t hw = (size_t)(net_h_ / kStrides[si]) * (net_w_ / kStrides[si]);
                size_t cnt = hw * chans[k];
                if (!dst) return (long)cnt;
                if (cap < cnt) throw ArgError("destination too small");
                RF_HIP(hipStreamSynchronize(l.stream));
                RF_HIP(hipMemcpy(dst, l.d_dump[si][k] + (size_t)(last_first_image_ + image) * cnt, cnt * sizeof(float),
                                 hipMemcpyDeviceToHost));
                return (long)cnt;
            }
        throw ArgError("unknown output blob '" + blob + "'");
    }

    long debug_activation(const std::string &blob, int image, float *dst, size_t cap, int dims[3]) override {
        DeviceGuard guard(device_);
        Lane &l = lanes_[last_lane_];
        if (blob == "input_canvas") {
            // the net-sized u8 BGR canvas an OVERSIZE frame was scaled onto (valid when the last launch had one)
            if (image < 0 || image >= last_n_ || last_first_image_ < 0) throw ArgError("image index out of range");
            const size_t cnt = (size_t)net_h_ * net_w_ * 3;
            if (dims) { dims[0] = net_h_; dims[1] = net_w_; dims[2] = 3; }
            if (!dst) return (long)cnt;
            if (cap < cnt) throw ArgError("destination too small");
            RF_HIP(hipStreamSynchronize(l.stream));
            std::vector<uint8_t> tmp(cnt);
            RF_HIP(hipMemcpy(tmp.data(), l.d_canvas + (size_t)(last_first_image_ + image) * cnt, cnt, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; i++) dst[i] = (float)tmp[i];
            return (long)cnt;
        }
        // "<blob>#raw": the stored values themselves (int8 engine: the quanta, not multiplied by the tensor's scale)
        bool raw = false;
        std::string key = blob;
        if (key.size() > 4 && key.compare(key.size() - 4, 4, "#raw") == 0) { raw = true; key.resize(key.size() - 4); }
        auto it = l.acts.find(key);
        if (it == l.acts.end()) throw ArgError("unknown activation '" + key + "'");
        const ActInfo &ai = it->second;
        if (image < 0 || image >= last_n_ || last_first_image_ < 0) throw ArgError("image index out of range");
        size_t cnt = (size_t)ai.h * ai.w * ai.c;
        if (dims) { dims[0] = ai.h; dims[1] = ai.w; dims[2] = ai.c; }
        if (!dst) return (long)cnt;
        if (cap < cnt) throw ArgError("destination too small");
        RF_HIP(hipStreamSynchronize(l.stream));
        const size_t eb = kind_.elem_bytes;
        std::vector<uint8_t> tmp(cnt * eb);
        RF_HIP(hipMemcpy(tmp.data(), (const uint8_t *)ai.ptr + (size_t)(last_first_image_ + image) * cnt * eb, cnt * eb, hipMemcpyDeviceToHost));
        kind_.to_float(tmp.data(), cnt, dst);
        if (!raw && !ai.scale.empty())
            for (size_t i = 0; i < cnt; i++) dst[i] *= ai.scale[i % ai.c];      // NHWC: channel = i % c
        return (long)cnt;
    }

    int profile(const void *const *d_frames, int n, int iters, int cap, const char **names, const char **kernels,
                float *avg_ms, double *alg_bytes, double *macs) override {
        if (n < 1 || n > cap_images_ || iters < 1) throw ArgError("profile: bad n / iters");
        DeviceGuard guard(device_);
        launch_pending();
        Lane &l = lanes_[0];
        harvest(l);
        RF_HIP(hipStreamSynchronize(l.stream));
        const int mb = cap_images_;
        for (int i = 0; i < n; i++) l.h_frames[mb + i] = FrameDesc{(const uint8_t *)d_frames[i], net_h_, net_w_, net_w_ * 3, 0};
        *l.h_params = RunParams{0.5f, nms_threshold_, n, 0};
        RF_HIP(hipMemcpyAsync(l.d_frames, l.h_frames, l.table_bytes, hipMemcpyHostToDevice, l.stream));
        size_t nops = l.ops.size();
        while (prof_ev_.size() < 2 * nops) { hipEvent_t e; RF_HIP(hipEventCreate(&e)); prof_ev_.push_back(e); }
        // Every launch is timed on the engine's own stream as `kReps` back-to-back repetitions between one HIP event
        // pair (a single launch between two events would mostly measure the ~6 us event/launch overhead); the result is
        // the average duration per launch including its launch boundary.  A full pass runs first in launch order so
        // every kernel sees the real producer's data.
        constexpr int kReps = 8;
        const size_t kh = nops - 2, kn = nops - 1;     // heads, NMS: producer / consumer of the candidate counters
        std::vector<double> sum(nops, 0.0);
        for (int it = -1; it < iters; it++) {          // one untimed warm-up pass
            for (size_t k = 0; k < kh; k++) {
                l.ops[k].launch(l.stream, n);           // real predecessor state for the ops that follow
                RF_HIP(hipEventRecord(prof_ev_[2 * k], l.stream));
                for (int r = 0; r < kReps; r++) l.ops[k].launch(l.stream, n);
                RF_HIP(hipEventRecord(prof_ev_[2 * k + 1], l.stream));
            }
            // NMS re-arms the counters the heads fill, so the two are repeated as a pair; the heads are also repeated
            // alone (candidates pile up, one NMS drains them afterwards) and NMS = pair - heads.
            RF_HIP(hipEventRecord(prof_ev_[2 * kh], l.stream));
            for (int r = 0; r < kReps; r++) { l.ops[kh].launch(l.stream, n); l.ops[kn].launch(l.stream, n); }
            RF_HIP(hipEventRecord(prof_ev_[2 * kh + 1], l.stream));
            RF_HIP(hipEventRecord(prof_ev_[2 * kn], l.stream));
            for (int r = 0; r < kReps; r++) l.ops[kh].launch(l.stream, n);
            RF_HIP(hipEventRecord(prof_ev_[2 * kn + 1], l.stream));
            l.ops[kn].launch(l.stream, n);
            RF_HIP(hipStreamSynchronize(l.stream));
            RF_HIP(hipGetLastError());
            if (it < 0) continue;
            for (size_t k = 0; k < nops; k++) {
                float ms = 0;
                RF_HIP(hipEventElapsedTime(&ms, prof_ev_[2 * k], prof_ev_[2 * k + 1]));
                if (k < kh) sum[k] += ms / kReps;
                else if (k == kh) sum[kn] += ms / kReps;      // pair, fixed up below
                else sum[kh] += ms / kReps;                   // heads alone
            }
        }
        sum[kn] = std::max(sum[kn] - sum[kh], 0.0);
        for (size_t k = 0; k < nops && (int)k < cap; k++) {
            if (names) names[k] = l.ops[k].name.c_str();
            if (kernels) kernels[k] = l.ops[k].kernel.c_str();
            if (avg_ms) avg_ms[k] = (float)(sum[k] / iters);
            if (alg_bytes) alg_bytes[k] = n * (l.ops[k].alg_u8_in + kind_.elem_bytes * (l.ops[k].alg_elems_in + l.ops[k].alg_elems_out));
            if (macs) macs[k] = n * l.ops[k].macs;
        }
        return (int)nops;
    }

    int compulsory_bytes(int n, int cap, double *bytes) override {
        if (n < 0 || (cap > 0 && !bytes)) throw ArgError("null argument");
        const Lane &l = lanes_[0];
        for (size_t k = 0; k < l.ops.size() && (int)k < cap; k++)
            bytes[k] = n * (l.ops[k].alg_u8_in + kind_.elem_bytes * (l.ops[k].hbm_elems_in + l.ops[k].hbm_elems_out));
        return (int)l.ops.size();
    }

private:
    struct Lane : LaneNet {                   // + the ops, activations and dump buffers build_net fills (net.h)
        bool built = false;
        std::vector<void *> dev_allocs, host_allocs;      // what build_lane allocated for this lane
        hipStream_t stream = nullptr;
        unsigned long long launch_seq = 0;    // order of this lane's last launch among all launches of the engine (pick_lane)
        // host-frame uploads from the pinned staging block alternate between the lane's stream and a second one (a second SDMA
        // engine); the launch waits for both
        hipStream_t copy2 = nullptr;
        hipEvent_t copy2_done = nullptr;
        bool copy2_used = false;
        unsigned uploads = 0;
        hipEvent_t time_ev[4] = {nullptr, nullptr, nullptr, nullptr};
        hipEvent_t done = nullptr;
        std::map<int, hipGraphExec_t> graphs;
        std::set<int> warmed;
        // pinned host staging of the per-launch table: [0,mb) source frames, [mb,2mb) what the stem reads, then RunParams;
        // ONE small H2D copy per launch puts it in HBM (a launch covers up to max_batch*coalesce images, so the copy is
        // amortised; reading it from the kernels over PCIe instead cost every workgroup a PCIe round trip)
        FrameDesc *h_frames = nullptr;
        RunParams *h_params = nullptr;
        FrameDesc *d_frames = nullptr;
        size_t table_bytes = 0;
        int *h_counts = nullptr;              // [2*max_batch]: kept counts, candidate counts
        Candidate *h_out = nullptr;           // [max_batch*max_det]
        // device
        RunParams *d_params = nullptr;
        int *d_cand_count = nullptr;
        Candidate *d_cand = nullptr;
        uint8_t *d_canvas = nullptr;
        // host frames: pinned staging block + its device twin (allocated on first use); a super-batch's frames are packed into
        // it back to back and cross PCIe as one DMA per enqueue
        uint8_t *h_stage = nullptr, *d_stage = nullptr;
        size_t stage_cap = 0, stage_used = 0;
        float *h_align_scale = nullptr;       // the stage hooks (lane_view): pinned, per image of the launch its frame_scale (allocated on first use)
        int *d_face_off = nullptr;            // the face-batch stage: packed offsets of the launch's images, written by its scan kernel (first use)
        hipEvent_t face_scan_done = nullptr;  // ... recorded behind that scan: the call's next launch (another lane) waits for it on the device
        uint8_t *h_pass_tab = nullptr;        // pass calls: pinned, per image of the launch the pass it is, in the mode's entry type (allocated on first use)
        hipEvent_t pass_done = nullptr;       // ... recorded behind the launch's gather: the call's merge (another lane) waits for it on the device
        uint8_t *h_track_tab = nullptr;       // the track stage: pinned, the launch's stream table and image table (allocated on first use)
        hipEvent_t track_done = nullptr;      // ... recorded behind the launch's track kernel: the call's next track launch (another lane) waits for it
        int32_t *h_shot_tab = nullptr;        // the shot stage: pinned, per tracked image of the launch its stream entry (allocated on first use)
        hipEvent_t shot_done = nullptr;       // ... recorded behind the launch's keep kernel: with a gallery the call's next track launch waits for this one
        int *h_red_streams = nullptr;         // the redaction stage behind a track launch: pinned, per image of the launch its stream (allocated on first use)
        bool busy = false;                    // a launched super-batch whose results have not been harvested yet
        int n_images = 0;                     // images of the super-batch being assembled / in flight on this lane
        float threshold = 0.f;
        bool need_resize = false, timed = false;
        std::vector<int> tickets;             // tickets riding on that super-batch
        std::vector<char> empty;              // per image: img.empty() (count forced to 0)
    };

    // One enqueue() / detect chunk.  Several tickets are coalesced into one launch ("super-batch") of up to
    // max_batch * coalesce images: the launch count per image -- what bounds throughput at batch 8 -- drops accordingly.
    struct Ticket {
        enum State { FREE, PENDING, LAUNCHED, DONE };
        State state = FREE;
        int lane = 0, first_image = 0, n = 0;
        bool timed = false;
        std::vector<int> kept, ncand, first_record;
        std::vector<Candidate> records;
    };

    // ------------------------------------------------------------------------------------------ build
    template <typename U> U *dalloc(size_t count) {
        void *p = nullptr;
        RF_HIP(hipMalloc(&p, std::max<size_t>(count * sizeof(U), 256)));
        (building_ ? building_->dev_allocs : dev_allocs_).push_back(p);
        return (U *)p;
    }
    template <typename U> U *halloc(size_t count) {
        void *p = nullptr;
        RF_HIP(hipHostMalloc(&p, std::max<size_t>(count * sizeof(U), 256), hipHostMallocDefault));
        (building_ ? building_->host_allocs : host_allocs_).push_back(p);
        memset(p, 0, std::max<size_t>(count * sizeof(U), 256));
        return (U *)p;
    }

    void free_lane(Lane &l) {
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        for (auto &kv : l.graphs) (void)hipGraphExecDestroy(kv.second);
        for (hipEvent_t &e : l.time_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.copy2_done) (void)hipEventDestroy(l.copy2_done);
        if (l.face_scan_done) (void)hipEventDestroy(l.face_scan_done);
        if (l.pass_done) (void)hipEventDestroy(l.pass_done);
        if (l.track_done) (void)hipEventDestroy(l.track_done);
        if (l.shot_done) (void)hipEventDestroy(l.shot_done);
        if (l.copy2) { (void)hipStreamSynchronize(l.copy2); (void)hipStreamDestroy(l.copy2); }
        if (l.d_stage) (void)hipFree(l.d_stage);
        if (l.h_stage) (void)hipHostFree(l.h_stage);
        if (l.stream) (void)hipStreamDestroy(l.stream);
        for (void *p : l.dev_allocs) (void)hipFree(p);
        for (void *p : l.host_allocs) (void)hipHostFree(p);
        l = Lane();
    }

    // build lane k if it has not been used yet; a failed build releases what it had allocated and rethrows
    void ensure_lane(int k) {
        Lane &l = lanes_[k];
        if (l.built) return;
        building_ = &l;
        try { build_lane(l, plan_); }
        catch (...) { building_ = nullptr; (void)hipGetLastError(); free_lane(l); throw; }
        building_ = nullptr;
        l.built = true;
    }

    // Which lane opens the next super-batch: an idle lane that exists (a synchronous caller therefore stays on lane 0), else a
    // lane that has not been built yet (if its buffers do not fit the device any more the engine simply runs with fewer lanes),
    // else the oldest busy one (its results are harvested first).
    int pick_lane() {
        const int L = (int)lanes_.size();
        for (int k = 0; k < L; k++) {
            const int l = (next_lane_ + k) % L;
            if (lanes_[l].built && !lanes_[l].busy) return l;
        }
        for (int l = 0; l < L; l++)
            if (!lanes_[l].built) {
                try { ensure_lane(l); return l; }
                catch (const HipError &) { if (l == 0) throw; lanes_.resize(l); next_lane_ %= l; break; }      // lanes l.. were never built: drop them
            }
        // every lane is busy: the one launched longest ago (its results are harvested first; next_lane_ is not it once idle lanes
        // have been preferred out of order)
        int oldest = 0;
        for (int l = 1; l < (int)lanes_.size(); l++)
            if (lanes_[l].launch_seq < lanes_[oldest].launch_seq) oldest = l;
        return oldest;
    }

    void build_lane(Lane &L, const Plan &plan) {
        const int mb = cap_images_;           // images per launch: max_batch * coalesce
        const int H = net_h_, W = net_w_;
        RF_HIP(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        for (auto &e : L.time_ev) RF_HIP(hipEventCreate(&e));
        RF_HIP(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        RF_HIP(hipStreamCreateWithFlags(&L.copy2, hipStreamNonBlocking));
        RF_HIP(hipEventCreateWithFlags(&L.copy2_done, hipEventDisableTiming));

        L.table_bytes = 2 * mb * sizeof(FrameDesc) + sizeof(RunParams);
        unsigned char *htab = halloc<unsigned char>(L.table_bytes);
        unsigned char *dtab = dalloc<unsigned char>(L.table_bytes);
        L.h_frames = (FrameDesc *)htab;
        L.h_params = (RunParams *)(htab + 2 * mb * sizeof(FrameDesc));
        L.d_frames = (FrameDesc *)dtab;
        L.d_params = (RunParams *)(dtab + 2 * mb * sizeof(FrameDesc));
        const size_t hdr = ((2 * mb * sizeof(int) + 255) / 256) * 256;
        unsigned char *res = halloc<unsigned char>(hdr + (size_t)mb * opt_.max_detections * sizeof(Candidate));
        L.h_counts = (int *)res;
        L.h_out = (Candidate *)(res + hdr);
        L.d_cand_count = dalloc<int>(mb);
        RF_HIP(hipMemset(L.d_cand_count, 0, mb * sizeof(int)));
        L.d_cand = dalloc<Candidate>((size_t)mb * opt_.max_candidates);
        L.d_canvas = dalloc<uint8_t>((size_t)mb * H * W * 3);

        NetSite site;
        site.mb = mb; site.net_h = H; site.net_w = W;
        site.frames = L.d_frames + mb;
        site.d_params = L.d_params;
        site.d_cand = L.d_cand; site.d_cand_count = L.d_cand_count;
        site.h_out = L.h_out; site.h_counts = L.h_counts;
        site.max_candidates = opt_.max_candidates; site.max_detections = opt_.max_detections; site.num_anchors = na_;
        site.keep_outputs = opt_.keep_outputs;
        site.ratios = &ratios_;
        site.dalloc = [this](size_t bytes) { return (void *)dalloc<uint8_t>(bytes); };
        kind_.build_net(plan, site, &L);
    }

    // ------------------------------------------------------------------------------------------ run
    static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

    // The host table of a standalone call (align, face_batch, track_update, track_shots, redact): sections appended at 256-byte
    // alignment, filled in align_host_ and sent to align_tab_ in one copy on the side stream.
    struct HostTable {
        size_t end = 0;
        size_t add(size_t bytes) { const size_t at = align256(end); end = at + bytes; return at; }
    };
    uint8_t *table_open(const HostTable &tb) {
        align_host_.assign(tb.end, 0);
        return align_host_.data();
    }
    // The FrameDesc section; returns which frames have no pixels.  With `who` every frame is checked, and one that is resident on another
    // device refused under that prefix (nullptr: the caller has checked the frames).
    std::vector<char> table_frames(FrameDesc *fd, const void *const *frames, const int *rows, const int *cols, const int *steps, int n, const char *who) {
        std::vector<char> empty((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            const int st = steps ? steps[i] : cols[i] * 3;
            const uint8_t *p = (const uint8_t *)frames[i];
            if (who) check_frame(p, rows[i], cols[i], st);
            empty[i] = !p || rows[i] <= 0 || cols[i] <= 0;
            if (who && !empty[i] && check_residency_) {
                const int where = foreign_device_of(p);
                if (where >= 0 && where != device_) throw ArgError(std::string(who) + ": frame is resident on another device");
            }
            fd[i] = empty[i] ? FrameDesc{nullptr, 0, 0, 0, 0} : FrameDesc{p, rows[i], cols[i], st, 0};
        }
        return empty;
    }
    // A per-image record section (faces, quality records, ids): the first min(cnt[i], take) records of image i, `bytes` each, from the
    // caller's array (src_per records per image) to the table's (dst_per per image).
    static void table_records(uint8_t *dst, int dst_per, const void *src, int src_per, size_t bytes, const int *cnt, int take, int n) {
        for (int i = 0; i < n; i++) {
            const int c = std::min(cnt[i], take);
            if (c > 0) memcpy(dst + (size_t)i * dst_per * bytes, (const uint8_t *)src + (size_t)i * src_per * bytes, (size_t)c * bytes);
        }
    }
    void table_upload(uint8_t *d_tab, const HostTable &tb) {
        if (!align_stream_) RF_HIP(hipStreamCreateWithFlags(&align_stream_, hipStreamNonBlocking));
        RF_HIP(hipMemcpyAsync(d_tab, align_host_.data(), tb.end, hipMemcpyHostToDevice, align_stream_));
    }
    // a launch of a standalone call on the side stream between two events, waited for; *ms: its hipEvent time, or -1
    template <class Launch> void timed_launch(hipEvent_t (&ev)[2], float &ms, Launch launch) {
        if (!ev[0]) { RF_HIP(hipEventCreate(&ev[0])); RF_HIP(hipEventCreate(&ev[1])); }
        RF_HIP(hipEventRecord(ev[0], align_stream_));
        launch();
        RF_HIP(hipGetLastError());
        RF_HIP(hipEventRecord(ev[1], align_stream_));
        RF_HIP(hipStreamSynchronize(align_stream_));
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) ms = -1.f;
    }

    // img.empty() (RetinaFace.cpp:578-580) is legal and yields count 0; everything else must be a sane CV_8UC3 view
    void check_frame(const uint8_t *ptr, int rows, int cols, int step) const {
        if (!ptr || rows <= 0 || cols <= 0) return;
        if (rows > 4096 * 3072 / std::max(cols, 1)) throw ArgError("frame larger than 4096x3072 (RetinaFace.cpp:325)");
        if (step < cols * 3) throw ArgError("row step smaller than cols*3");
    }

    // Staging capacity of a lane: room for a full super-batch of net-sized frames, or for what one enqueue needs if that is more
    // (sized by the frames actually staged, not by cap_images x the largest frame ever seen).
    void ensure_stage(Lane &L, size_t need, bool device_only = false) {
        if (need <= L.stage_cap && (device_only || L.h_stage)) return;
        const size_t want = std::max(std::max(need, L.stage_cap), (size_t)cap_images_ * align256((size_t)net_h_ * net_w_ * 3));
        RF_HIP(hipStreamSynchronize(L.stream));
        if (L.d_stage) RF_HIP(hipFree(L.d_stage));
        if (L.h_stage) RF_HIP(hipHostFree(L.h_stage));
        L.d_stage = nullptr; L.h_stage = nullptr; L.stage_cap = 0;
        // frames scattered from other GPUs (peer copies) never touch host memory: no pinned mirror for a handle that only stages those
        if (!device_only) RF_HIP(hipHostMalloc((void **)&L.h_stage, want, hipHostMallocDefault));
        RF_HIP(hipMalloc((void **)&L.d_stage, want));
        L.stage_cap = want;
    }

    // Where a caller's "device" frame lives (rf_detect_batch_device / rf_enqueue_batch_device).  -1: readable in place by this
    // engine's kernels (its own device's memory, or pinned / managed host memory); >= 0: the ordinal of ANOTHER device of the
    // node -- the frame is then scattered to this device over xGMI before the launch (submit()).  Anything the runtime does not
    // know as device-accessible memory is refused here instead of faulting inside a kernel.
    // The answer is cached per allocation and re-validated every kResidencyTtlUs (residency.h).

    // one runtime lookup; returns false for host / managed memory (answer in *where, not cacheable)
    bool lookup_residency(const uint8_t *p, Residency *out) {
        hipPointerAttribute_t attr;
        memset(&attr, 0, sizeof(attr));
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
            (void)hipGetLastError();
            throw ArgError("device frame pointer is not known to the HIP runtime (host memory passed to a *_device entry point?)");
        }
        if (attr.type == hipMemoryTypeUnregistered) throw ArgError("device frame pointer is unregistered host memory");
        out->owner = attr.device;
        out->checked_us = HostTrace::now();
        if (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeManaged) { out->where = -1; out->base = 0; out->bytes = 0; return false; }
        out->where = attr.device == device_ ? (force_scatter_ ? device_ : -1) : attr.device;
        hipDeviceptr_t base = nullptr;
        size_t bytes = 0;
        if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)p) != hipSuccess || !base || !bytes) {
            (void)hipGetLastError();
            out->base = 0; out->bytes = 0;
            return false;                       // a device pointer whose allocation cannot be delimited is looked up every time
        }
        out->base = (uintptr_t)base; out->bytes = bytes;
        return true;
    }

    int foreign_device_of(const uint8_t *p) {
        return residency_.where((uintptr_t)p, [this](uintptr_t a, Residency *out) { return lookup_residency((const uint8_t *)a, out); }, HostTrace::now);
    }

    bool is_registered(const uint8_t *p, size_t bytes) const {
        for (const auto &r : registered_)
            if ((uintptr_t)p >= r.base && (uintptr_t)p + bytes <= r.base + r.bytes) return true;
        return false;
    }
    void drop_range(const void *ptr, bool unpin) {
        DeviceGuard guard(device_);
        for (size_t i = 0; i < registered_.size(); i++)
            if (registered_[i].base == (uintptr_t)ptr) {
                for (auto &l : lanes_) if (l.stream) RF_HIP(hipStreamSynchronize(l.stream));     // no DMA may still read it
                if (unpin && registered_[i].owned) RF_HIP(hipHostUnregister((void *)ptr));
                registered_.erase(registered_.begin() + i);
                return;
            }
        throw ArgError("host_unregister: range was not registered on this handle");
    }

    void wait_impl(int ticket, rf_face *out, int cap_per_image, int *counts, bool *truncated) {
        if (ticket < 0 || ticket >= (int)tickets_.size() || tickets_[ticket].state == Ticket::FREE)
            throw ArgError("wait: invalid ticket");
        Ticket &t = tickets_[ticket];
        if (t.state == Ticket::PENDING) launch_pending();          // its super-batch has not been launched yet
        if (t.state == Ticket::LAUNCHED) {
            // About to block on a running super-batch: a partial one queued behind it starts now and runs on its own lane
            // meanwhile (the tail of a burst overlaps instead of serialising).  When the waited batch has already finished
            // nothing is flushed -- in a steady pipeline the pending batch keeps filling up to max_batch x coalesce images.
            Lane &L = lanes_[t.lane];
            if (L.busy && hipEventQuery(L.done) == hipErrorNotReady) launch_pending();
            harvest(L);                                             // first waiter of a super-batch collects all of it
        }
        bool tr = false;
        last_lane_ = t.lane;
        last_first_image_ = t.first_image;
        last_n_ = t.n;
        last_cand_counts_.assign(t.n, 0);
        if ((int)last_anchor_.size() < t.n) last_anchor_.resize(t.n);      // per-image vectors keep their capacity across waits
        for (int i = 0; i < t.n; i++) {
            int kept = t.kept[i], ncand = t.ncand[i];
            last_cand_counts_[i] = ncand;
            if (ncand > opt_.max_candidates) tr = true;
            int avail = std::min(kept, opt_.max_detections);
            if (kept > opt_.max_detections) tr = true;
            if (counts) counts[i] = kept;
            int ncopy = out ? std::min(avail, cap_per_image) : 0;
            if (out && avail > cap_per_image) tr = true;
            const Candidate *src = t.records.data() + t.first_record[i];
            last_anchor_[i].resize(avail);
            for (int k = 0; k < avail; k++) last_anchor_[i][k] = src[k].anchor;
            for (int k = 0; k < ncopy; k++) memcpy(&out[(size_t)i * cap_per_image + k], &src[k], sizeof(rf_face));
        }
        if (t.timed) {
            Lane &s = lanes_[t.lane];
            float a = 0, b = 0, c = 0;
            (void)hipEventElapsedTime(&a, s.time_ev[0], s.time_ev[1]);
            (void)hipEventElapsedTime(&b, s.time_ev[1], s.time_ev[2]);
            (void)hipEventElapsedTime(&c, s.time_ev[2], s.time_ev[3]);
            t_pre_ = a; t_infer_ = b; t_post_ = c; t_total_ = a + b + c;
            have_split_ = true;
        }
        t.state = Ticket::FREE;
        if (truncated) *truncated = tr;
    }

    int alloc_ticket() {
        for (size_t k = 0; k < tickets_.size(); k++) {
            int id = (int)((next_ticket_ + k) % tickets_.size());
            if (tickets_[id].state == Ticket::FREE) { next_ticket_ = (id + 1) % (int)tickets_.size(); return id; }
        }
        throw ArgError("too many outstanding tickets: call rf_wait before enqueueing more");
    }

    // copy a finished super-batch's results out of the lane's pinned block into its tickets, so the lane can be reused
    void harvest(Lane &L) {
        if (!L.busy) return;
        double tt = trace_.on ? HostTrace::now() : 0.0;
        RF_HIP(hipEventSynchronize(L.done));
        trace_.add(5, tt);
        tt = trace_.on ? HostTrace::now() : 0.0;
        struct AtExit { HostTrace &t; double t0; ~AtExit() { t.add(6, t0); } } at_exit{trace_, tt};
        const int mb = cap_images_;
        for (int id : L.tickets) {
            Ticket &t = tickets_[id];
            t.kept.assign(t.n, 0); t.ncand.assign(t.n, 0); t.first_record.assign(t.n, 0);
            t.records.clear();
            for (int i = 0; i < t.n; i++) {
                const int img = t.first_image + i;
                if (L.empty[img]) continue;
                t.kept[i] = L.h_counts[img];
                t.ncand[i] = L.h_counts[mb + img];
                t.first_record[i] = (int)t.records.size();
                const int avail = std::min(t.kept[i], opt_.max_detections);
                const Candidate *src = L.h_out + (size_t)img * opt_.max_detections;
                t.records.insert(t.records.end(), src, src + avail);
            }
            t.state = Ticket::DONE;
        }
        L.tickets.clear();
        L.busy = false;
        L.n_images = 0;
    }

    void launch_pending() {
        if (pending_lane_ < 0) return;
        Lane &s = lanes_[pending_lane_];
        pending_lane_ = -1;
        const int n = s.n_images;
        if (n == 0) return;
        launches_++;
        launched_images_ += n;
        *s.h_params = RunParams{s.threshold, nms_threshold_, n, 0};
        if (s.need_resize) {
            // Only the frames that are larger than the net are read from the canvas.  A frame that fits keeps its own descriptor, as in a
            // launch without a resize: the stems choose their staging path (raw rows / general, different conv0 K order) from a frame's
            // pointer, pitch and width, so a fitting frame read from the canvas instead could differ in the last bits from the same frame in
            // a launch that holds no oversize frame -- an image's result must not depend on what it shares a launch with.
            const int mb = cap_images_;
            for (int i = 0; i < n; i++)
                if (s.h_frames[i].rows > net_h_ || s.h_frames[i].cols > net_w_)
                    s.h_frames[mb + i] = FrameDesc{s.d_canvas + (size_t)i * net_h_ * net_w_ * 3, net_h_, net_w_, net_w_ * 3, 0};
        }
        if (s.copy2_used) {             // uploads that went through the second copy stream: the launch waits for them
            RF_HIP(hipEventRecord(s.copy2_done, s.copy2));
            RF_HIP(hipStreamWaitEvent(s.stream, s.copy2_done, 0));
            s.copy2_used = false;
        }
        if (passes_.inputs_ready) RF_HIP(hipStreamWaitEvent(s.stream, passes_.inputs_ready, 0));      // the launch reads mirrored / zoomed / rotated / enhanced copies
        double tt = trace_.on ? HostTrace::now() : 0.0;
        RF_HIP(hipMemcpyAsync(s.d_frames, s.h_frames, s.table_bytes, hipMemcpyHostToDevice, s.stream));
        trace_.add(2, tt);
        tt = trace_.on ? HostTrace::now() : 0.0;
        if (s.need_resize) {
            if (opt_.resize_bilinear) launch_resize_bilinear(s.stream, s.d_frames, s.d_canvas, n, net_h_, net_w_);
            else launch_resize_area(s.stream, s.d_frames, s.d_canvas, n, net_h_, net_w_);
        }
        const bool eager_timed = s.timed;
        if (eager_timed) RF_HIP(hipEventRecord(s.time_ev[1], s.stream));
        if (opt_.use_graph && s.warmed.count(n)) {
            auto it = s.graphs.find(n);
            if (it == s.graphs.end()) it = s.graphs.emplace(n, capture(s, n)).first;
            RF_HIP(hipGraphLaunch(it->second, s.stream));
        } else {
            for (size_t k = 0; k < s.ops.size(); k++) {
                if (eager_timed && k == s.first_post) RF_HIP(hipEventRecord(s.time_ev[2], s.stream));
                s.ops[k].launch(s.stream, n);
            }
            s.warmed.insert(n);    // first run of a batch size is always eager: function attributes get set outside capture
        }
        RF_HIP(hipGetLastError());
        trace_.add(3, tt);
        tt = trace_.on ? HostTrace::now() : 0.0;
        if (eager_timed) RF_HIP(hipEventRecord(s.time_ev[3], s.stream));
        // the open call's stages: ordinary launches behind the graph, before `done`: nothing waits in between
        const bool staged = call_.armed();
        if (staged && (n > cap_images_ || call_.next_image + n > call_.n)) throw HipError(std::string(call_.who) + ": a launch carries images of another call");
        if (call_.align.on) launch_lane_align(s, n);
        if (call_.fb.on) launch_lane_face_batch(s, n);
        if (passes_.on) launch_lane_passes(s, n);
        if (call_.trk.on) launch_lane_track(s, n);
        if (call_.shot.on) launch_lane_shots(s);
        if (call_.follow.on) launch_lane_follow(s);
        if (call_.red.on) launch_lane_redact(s, n);
        if (staged) call_.next_image += n;
        RF_HIP(hipEventRecord(s.done, s.stream));
        trace_.add(4, tt);
        s.busy = true;
        s.launch_seq = ++launch_counter_;
        for (int id : s.tickets) tickets_[id].state = Ticket::LAUNCHED;
    }

    // What every stage hook binds from the lane into its kernel parameters: faces and counts from the pinned result block the NMS
    // kernel of the same stream has just written; where the struct has them, source frames from the launch's own frame table (the
    // first half: full-resolution frames, also when the stem reads a shrunk canvas) and each frame's coordinate scale from the pinned
    // per-lane array.
    template <class P> void lane_faces(P &p, const Lane &s) const {
        p.faces = (const uint8_t *)s.h_out;
        p.face_stride = (int)sizeof(Candidate); p.faces_per_image = opt_.max_detections;
        p.counts = s.h_counts;
    }
    void lane_view(TrackParams &p, const Lane &s) const { lane_faces(p, s); }
    void lane_view(ShotParams &p, const Lane &s) const { p.frames = s.d_frames; lane_faces(p, s); }
    template <class P> void lane_view(P &p, const Lane &s) const {      // AlignParams, FaceSeq, OverlayParams
        p.frames = s.d_frames;
        p.scale = s.h_align_scale;
        lane_faces(p, s);
    }

    // a per-lane block allocated on first use and owned by the lane (pinned host memory, or device memory), with the event of its stage
    template <class U> void lane_block(Lane &s, U *&block, size_t bytes, bool device = false, hipEvent_t *event = nullptr) {
        if (block) return;
        void *p = nullptr;
        if (device) { RF_HIP(hipMalloc(&p, std::max<size_t>(bytes, 256))); s.dev_allocs.push_back(p); }
        else { RF_HIP(hipHostMalloc(&p, std::max<size_t>(bytes, 256), hipHostMallocDefault)); s.host_allocs.push_back(p); }
        block = (U *)p;
        if (event) RF_HIP(hipEventCreateWithFlags(event, hipEventDisableTiming));
    }

    // the alignment launch of a super-batch of an aligning call
    void launch_lane_align(Lane &s, int n) {
        fill_lane_align_scale(s, n);
        AlignParams ap;
        lane_view(ap, s);
        ap.n = n; ap.max_faces = call_.align.rq.max_faces; ap.crop = call_.align.rq.crop;
        ap.first_image = call_.next_image;
        ap.crops = call_.align.d_crops; ap.mats = call_.align.d_mats;
        launch_align(s.stream, ap);
        RF_HIP(hipGetLastError());
    }

    // pinned per-lane array of each image's coordinate scale (rf_frame_scale)
    void fill_lane_align_scale(Lane &s, int n) {
        lane_block(s, s.h_align_scale, (size_t)cap_images_ * sizeof(float));
        for (int i = 0; i < n; i++) {
            const FrameDesc &f = s.h_frames[i];
            s.h_align_scale[i] = f.ptr ? frame_scale(f.rows, f.cols, net_h_, net_w_) : 1.f;
        }
    }

    // The face-batch launches of a super-batch of a face-batch call.  Packed offsets continue across the launches of a call through
    // ONE running base in device memory: this launch's scan waits (on the device: hipStreamWaitEvent) for the scan of the call's
    // previous launch, which ran on another lane's stream; the detection launches in front of it do not wait and keep overlapping.
    // No host wait anywhere.
    void launch_lane_face_batch(Lane &s, int n) {
        fill_lane_align_scale(s, n);
        lane_block(s, s.d_face_off, ((size_t)cap_images_ + 1) * sizeof(int), true, &s.face_scan_done);
        FaceSeq q;
        lane_view(q, s);
        q.n = n; q.image0 = call_.next_image;
        q.first = call_.fb.first;
        q.offsets = call_.fb.rq.gated ? (int *)fq_offsets_.ptr + call_.next_image : s.d_face_off;
        q.wait_before_scan = (call_.fb.prev_scan && call_.fb.prev_scan != s.face_scan_done) ? call_.fb.prev_scan : nullptr;
        q.record_after_scan = s.face_scan_done;
        launch_face_seq(s.stream, call_.fb.rq, q, call_.fb.d_tensor, call_.fb.d_mats);
        call_.fb.prev_scan = s.face_scan_done;
        call_.fb.first = false;
        RF_HIP(hipGetLastError());
    }

    // The pass-call launches of a super-batch of detect_tiled() / detect_tta() / detect_pyramid() / detect_rot(): the gather reads the
    // launch's faces and counts from the pinned result block the NMS kernel of the same stream has just written, and what each image
    // of the launch is from a pinned per-lane pass table.  A launch that is not the call's last records the lane's pass_done behind
    // its gather.  Behind the call's LAST launch this stream waits (on the device: hipStreamWaitEvent) for the gathers of the call's
    // other lanes, then runs the merge (for the fused tiled call also the face-batch launches over the merged faces).  The lane's
    // `done` event follows, so the host's ordinary wait for the last launch covers all of it.  No host wait anywhere.
    void launch_lane_passes(Lane &s, int n) {
        lane_block(s, s.h_pass_tab, (size_t)cap_images_ * kPassEntryMax, false, &s.pass_done);
        PassCall &c = passes_;
        if (n > cap_images_ || c.next_pass + n > c.total) throw HipError(std::string(c.name) + ": a launch carries images of another call");
        memcpy(s.h_pass_tab, c.table.data() + (size_t)c.next_pass * c.entry_bytes, (size_t)n * c.entry_bytes);
        c.gather(s.stream, (const uint8_t *)s.h_out, (int)sizeof(Candidate), s.h_counts, s.h_pass_tab, n);
        RF_HIP(hipGetLastError());
        c.next_pass += n;
        const int me = (int)(&s - lanes_.data());
        if (c.next_pass < c.total) {
            RF_HIP(hipEventRecord(s.pass_done, s.stream));
            if (std::find(c.lanes_used.begin(), c.lanes_used.end(), me) == c.lanes_used.end()) c.lanes_used.push_back(me);
            return;
        }
        for (int l : c.lanes_used)
            if (l != me && l < (int)lanes_.size() && lanes_[l].pass_done) RF_HIP(hipStreamWaitEvent(s.stream, lanes_[l].pass_done, 0));
        c.merge(s.stream, s.d_params);
        RF_HIP(hipGetLastError());
    }

    // the face-batch launches of the fused tiled call: face_batch()'s launches over the merged faces and counts in device memory
    // (Candidate records, max_faces per frame, coordinate scale 1), on the stream that has just run the merge
    void launch_tiled_face_batch(hipStream_t st, int n, const FaceBatchRequest &rq, int fpi, uint8_t *d_tensor, double *d_mats) {
        if (!(d_tensor || d_mats || rq.gated)) return;
        for (int base = 0; base < n; base += kAlignImagesPerLaunch) {
            FaceSeq q;
            q.frames = (const FrameDesc *)tile_tab_.ptr + base;      // uploaded by detect_tiled() before the call's first launch
            q.faces = tile_out_.ptr + (size_t)base * fpi * sizeof(Candidate);
            q.face_stride = (int)sizeof(Candidate); q.faces_per_image = fpi;
            q.counts = (const int *)tile_outcount_.ptr + base;
            q.scale = nullptr;
            q.n = std::min(kAlignImagesPerLaunch, n - base); q.image0 = base;
            q.first = base == 0;
            q.offsets = (int *)fq_offsets_.ptr + base;
            launch_face_seq(st, rq, q, d_tensor, d_mats);
        }
    }

    // The track launch of a super-batch of a tracked call: faces and counts as lane_view() binds them (and, for the fused face batch,
    // the quality records its quality kernel has just written), which images belong to which stream from a pinned per-lane table.  A
    // stream's images may sit in several launches on different lanes, and the state is one block in device memory, so the track
    // launches of a call form a chain: each waits (on the device: hipStreamWaitEvent) for the track launch of the call's previous
    // launch and records its own event.  The detection launches in front do not wait and keep overlapping.  The lane's `done` event
    // follows, so the host's ordinary wait covers it.  No host wait anywhere.
    void launch_lane_track(Lane &s, int n) {
        lane_block(s, s.h_track_tab, (size_t)cap_images_ * (sizeof(TrackStreamEntry) + sizeof(TrackImageEntry)), false, &s.track_done);
        std::vector<float> scale(n);
        std::vector<char> empty(n);
        for (int i = 0; i < n; i++) {
            const FrameDesc &f = s.h_frames[i];
            empty[i] = f.ptr ? 0 : 1;
            scale[i] = f.ptr ? frame_scale(f.rows, f.cols, net_h_, net_w_) : 1.f;
        }
        TrackStreamEntry *se = (TrackStreamEntry *)s.h_track_tab;
        TrackImageEntry *ie = (TrackImageEntry *)(se + cap_images_);
        const int ns = track_build_table(call_.trk.stream_of_image, call_.next_image, n, scale.data(), empty.data(), se, ie);
        call_.shot.last_streams = ns;
        if (ns == 0) return;
        if (call_.trk.prev && call_.trk.prev != s.track_done) RF_HIP(hipStreamWaitEvent(s.stream, call_.trk.prev, 0));
        TrackParams tp = track_params(*call_.trk.tr);
        tp.streams = se; tp.n_streams = ns;
        tp.images = ie;
        lane_view(tp, s);
        tp.records = call_.trk.records;
        tp.max_faces = call_.trk.max_faces;
        launch_track(s.stream, tp);
        RF_HIP(hipGetLastError());
        RF_HIP(hipEventRecord(s.track_done, s.stream));
        call_.trk.prev = s.track_done;
    }

    // The shot launches of a super-batch of a shot call, behind its track launch: the tables launch_lane_track() has just filled,
    // frames, faces and counts as lane_view() binds them.  The keep launch reads the table the NEXT track launch of the call
    // rewrites, and that launch's deliver reads the entries this keep writes, so with a gallery the chain runs through the event
    // recorded here: the call's next track launch waits for this keep launch, not only for the track launch in front of it.  The
    // lane's `done` event follows.  No host wait anywhere.
    void launch_lane_shots(Lane &s) {
        const int ns = call_.shot.last_streams;
        if (ns == 0) return;                          // no tracked image in this launch: launch_lane_track() launched nothing either
        lane_block(s, s.h_shot_tab, (size_t)cap_images_ * sizeof(int32_t), false, &s.shot_done);
        const TrackStreamEntry *se = (const TrackStreamEntry *)s.h_track_tab;
        int n_img = 0;
        for (int z = 0; z < ns; z++)
            for (int j = 0; j < se[z].n && n_img < cap_images_; j++) s.h_shot_tab[n_img++] = z;
        ShotParams sp;
        memset((void *)&sp, 0, sizeof(sp));
        sp.streams = se; sp.n_streams = ns;
        sp.images = (const TrackImageEntry *)(se + cap_images_); sp.n_images = n_img;
        sp.entry_of = s.h_shot_tab;
        lane_view(sp, s);
        shot_launches(s.stream, sp);
        RF_HIP(hipEventRecord(s.shot_done, s.stream));
        call_.trk.prev = s.shot_done;
    }

    // The keep launch of a super-batch of a key call on a tracker with follow, behind its track launch: the tables launch_lane_track()
    // has just filled and the launch's own frame table (full-resolution source frames).  Every stream appears once in the call, so the
    // table the keep launch reads is the one after this frame's step; the lane's track event is recorded again behind it, so the track
    // chain of the call runs through the keep launch.  The lane's `done` event follows.  No host wait anywhere.
    void launch_lane_follow(Lane &s) {
        const int ns = call_.shot.last_streams;
        if (ns == 0) return;                          // no tracked image in this launch: launch_lane_track() launched nothing either
        FollowParams fp = follow_params(*call_.trk.tr);
        fp.streams = (const TrackStreamEntry *)s.h_track_tab; fp.n_streams = ns;
        fp.images = (const TrackImageEntry *)(fp.streams + cap_images_);
        fp.frames = s.d_frames;
        launch_follow_keep(s.stream, fp);
        RF_HIP(hipGetLastError());
        RF_HIP(hipEventRecord(s.track_done, s.stream));
    }

    // The redaction launches of a super-batch of a redacting call: frames (the caller's, written in place), faces, counts and scales
    // as lane_view() binds them.  With a tracker the launches sit behind the lane's track launch: every stream appears at most once
    // in the call, so its table is the one after this frame's step.  Region records, cell values and pixel counts are indexed by the
    // image's place in the call: launches on different lanes write different slices.  The lane's `done` event follows.  No host
    // wait anywhere.
    void launch_lane_redact(Lane &s, int n) {
        fill_lane_align_scale(s, n);
        OverlayParams rp = redact_params();
        if (call_.red.tr) {
            if (call_.red.overlay && call_.trk.on) {         // the tags the lane's track launch has just written, pinned like the result block
                rp.ids = (const uint8_t *)trk_tags_.ptr + (size_t)call_.next_image * call_.trk.tag_stride * sizeof(rf_track_tag);
                rp.id_stride = (int)sizeof(rf_track_tag); rp.ids_per_image = call_.trk.tag_stride; rp.ids_of_streams = 1;
            }
            lane_block(s, s.h_red_streams, (size_t)cap_images_ * sizeof(int));
            for (int i = 0; i < n; i++) s.h_red_streams[i] = call_.red.stream_of_image[call_.next_image + i];
            rp.streams = s.h_red_streams;
        }
        lane_view(rp, s);
        rp.count_cap = opt_.max_detections;
        rp.n = n; rp.image0 = call_.next_image;
        redact_launch(s.stream, rp);
        RF_HIP(hipGetLastError());
    }

    // The stream table of images [image0, image0 + n) of a call: the streams present in order of first appearance, each with its
    // images in call order.  Returns the number of streams present (images of stream -1 appear nowhere).
    static int track_build_table(const int *stream_of_image, int image0, int n, const float *scale, const char *empty, TrackStreamEntry *se,
                                 TrackImageEntry *ie) {
        std::vector<int> order;
        for (int i = 0; i < n; i++)
            if (stream_of_image[image0 + i] >= 0) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return stream_of_image[image0 + a] < stream_of_image[image0 + b]; });
        int ns = 0;
        for (size_t j = 0; j < order.size(); j++) {
            const int i = order[j], st = stream_of_image[image0 + i];
            if (j == 0 || st != se[ns - 1].stream) se[ns++] = TrackStreamEntry{st, (int)j, 0, 0};
            se[ns - 1].n++;
            ie[j] = TrackImageEntry{i, image0 + i, scale[i], empty[i]};
        }
        return ns;
    }

    Tracker &tracker_of(void *p) {
        for (auto &t : trackers_)
            if (t.get() == p) return *t;
        throw ArgError("not a tracker of this handle");
    }
    // a stream's (or every stream's) empty state: no tracks, frame counter 0, next id 1
    void tracker_reset_impl(Tracker &t, int stream) {
        const size_t sb = t.stream_bytes();
        const int first = stream < 0 ? 0 : stream, count = stream < 0 ? t.n_streams : 1;
        std::vector<uint8_t> img((size_t)count * sb, 0);
        for (int i = 0; i < count; i++) *(TrackHeader *)(img.data() + (size_t)i * sb) = TrackHeader{0, 1};
        RF_HIP(hipMemcpy(t.state.ptr + (size_t)first * sb, img.data(), img.size(), hipMemcpyHostToDevice));
        if (t.has_shots) {
            const size_t rb = (size_t)t.spec.max_tracks * sizeof(rf_shot);
            RF_HIP(hipMemset(t.shot_records.ptr + (size_t)first * rb, 0, (size_t)count * rb));
            RF_HIP(hipDeviceSynchronize());
        }
        if (t.has_motion) {
            RF_HIP(hipMemset(t.motion.ptr + (size_t)first * t.motion_bytes(), 0, (size_t)count * t.motion_bytes()));
            RF_HIP(hipDeviceSynchronize());
        }
        if (t.has_follow) {
            RF_HIP(hipMemset(t.follow_records.ptr + (size_t)first * t.follow_bytes(), 0, (size_t)count * t.follow_bytes()));
            RF_HIP(hipDeviceSynchronize());
        }
    }
    // the arguments of a tracked call, checked before any state changes
    Tracker &track_check(const TrackRequest &rq, int n, bool shots = false, bool follow = false) {
        Tracker &t = tracker_of(rq.tracker);
        if (t.dirty) throw ArgError("the tracker's last call failed: reset it first");
        if (t.has_follow && !follow) throw ArgError("the tracker has follow: use the follow calls, this one would leave a template stale");
        if (!t.has_follow && follow) throw ArgError("the tracker has no follow (rf_tracker_enable_follow)");
        if (t.has_shots && !shots) throw ArgError("the tracker has a shot gallery: use the shot calls, this one would leave it stale");
        if (!t.has_shots && shots) throw ArgError("the tracker has no shot gallery (rf_tracker_enable_shots)");
        if (n > 0 && !rq.stream_of_image) throw ArgError("stream_of_image is null");
        if (rq.cap_ended < 0 || (rq.cap_ended > 0 && !rq.ended)) throw ArgError("ended is null");
        if ((long)n * std::max(rq.cap_ended, 1) > (1L << 24)) throw ArgError("n x cap_ended: more than 2^24 records in one call");
        for (int i = 0; i < n; i++)
            if (rq.stream_of_image[i] < -1 || rq.stream_of_image[i] >= t.n_streams) throw ArgError("stream_of_image: stream out of range");
        if (follow) {                                  // a stream's template belongs to one frame of the call
            std::vector<int> seen;
            for (int i = 0; i < n; i++)
                if (rq.stream_of_image[i] >= 0) seen.push_back(rq.stream_of_image[i]);
            std::sort(seen.begin(), seen.end());
            if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) throw ArgError("follow: a stream appears more than once in the call");
        }
        return t;
    }
    // call-level result blocks (pinned host memory): tags (tag_stride per image), ended lists, ended counts | status
    // (full_tags: the shot kernels find faces by their tags, so every face the step looks at gets one whatever the caller's cap is)
    void track_open_call(Tracker &t, const TrackRequest &rq, int n, int cap_per_image, bool full_tags = false) {
        call_.trk.tr = &t;
        call_.trk.stream_of_image = rq.stream_of_image;
        call_.trk.n = n; call_.trk.prev = nullptr;
        call_.trk.tag_stride = full_tags ? kTrackMaxFaces : std::max(0, std::min(cap_per_image, kTrackMaxFaces));
        call_.trk.cap_ended = rq.cap_ended;
        trk_tags_.reserve((size_t)std::max(n, 1) * std::max(call_.trk.tag_stride, 1) * sizeof(rf_track_tag));
        trk_ended_.reserve((size_t)std::max(n, 1) * std::max(rq.cap_ended, 1) * sizeof(rf_track));
        trk_counts_.reserve((size_t)std::max(n, 1) * 2 * sizeof(int));
    }
    TrackParams track_params(const Tracker &t) const {
        TrackParams tp;
        memset(&tp, 0, sizeof(tp));
        tp.spec = t.spec;
        tp.state = t.state.ptr;
        tp.tags = (rf_track_tag *)trk_tags_.ptr; tp.tag_stride = call_.trk.tag_stride;
        tp.ended = (rf_track *)trk_ended_.ptr; tp.cap_ended = call_.trk.cap_ended;
        tp.ended_counts = (int *)trk_counts_.ptr;
        tp.status = (int *)trk_counts_.ptr + std::max(call_.trk.n, 1);
        if (t.has_motion) { tp.motion = (rf_track_motion *)t.motion.ptr; tp.mspec = t.motion_spec; }
        return tp;
    }
    // Results of a finished tracked call, from the pinned blocks the kernel wrote; the host fills what the device never writes -- the
    // images of stream -1, the tags at or beyond the image's count and whatever lies behind an ended list.
    void track_copy_out(Tracker &t, const TrackRequest &rq, int n, int cap_per_image, const int *counts, bool *cut) {
        const int ts = call_.trk.tag_stride;
        const int *cs = (const int *)trk_counts_.ptr;
        const rf_track_tag *tags = (const rf_track_tag *)trk_tags_.ptr;
        const rf_track *ended = (const rf_track *)trk_ended_.ptr;
        for (int i = 0; i < n; i++) {
            const bool tracked = rq.stream_of_image[i] >= 0;
            const int ec = tracked ? cs[i] : 0;
            if (rq.ended_counts) rq.ended_counts[i] = ec;
            if (ec > rq.cap_ended || (tracked && cs[n + i])) *cut = true;
            if (rq.ended && rq.cap_ended > 0) {
                const int have = std::min(ec, rq.cap_ended);
                rf_track *dst = rq.ended + (size_t)i * rq.cap_ended;
                if (have) memcpy((void *)dst, ended + (size_t)i * rq.cap_ended, (size_t)have * sizeof(rf_track));
                memset((void *)(dst + have), 0, (size_t)(rq.cap_ended - have) * sizeof(rf_track));
            }
            if (!rq.tags) continue;
            rf_track_tag *dst = rq.tags + (size_t)i * cap_per_image;
            const int have = tracked ? std::max(0, std::min(std::min(counts[i], ts), cap_per_image)) : 0;      // what the kernel wrote
            if (have) memcpy((void *)dst, tags + (size_t)i * ts, (size_t)have * sizeof(rf_track_tag));
            for (int k = have; k < cap_per_image; k++) dst[k] = tracked && k < counts[i] ? track_tag_untracked(0) : track_tag_zero();
        }
        t.dirty = false;
    }

    // results of an alignment call to the caller's host buffers: per image the slots that hold faces (the others are unspecified)
    // (`limit`: the most faces per image the launch can have seen).  A block that is at least half full, and a small matrix block,
    // travel as one copy instead of one per image.
    void align_copy_out(const AlignRequest &rq, const uint8_t *d_crops, const double *d_mats, int n, const int *counts, int limit) {
        const size_t cb = (size_t)rq.crop * rq.crop * 3, mbytes = 6 * sizeof(double);
        const bool want_crops = rq.crops && d_crops, want_mats = rq.matrices && d_mats;
        if (!want_crops && !want_mats) return;
        std::vector<size_t> k(n);
        size_t used = 0;
        for (int i = 0; i < n; i++) used += k[i] = (size_t)std::max(0, std::min(std::min(counts[i], rq.max_faces), limit));
        if (!used) return;
        const size_t slots = (size_t)n * rq.max_faces;
        const bool crops_whole = 2 * used >= slots, mats_whole = crops_whole || slots * mbytes <= (1u << 20);
        if (want_crops && crops_whole) RF_HIP(hipMemcpy(rq.crops, d_crops, slots * cb, hipMemcpyDeviceToHost));
        if (want_mats && mats_whole) RF_HIP(hipMemcpy(rq.matrices, d_mats, slots * mbytes, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            const size_t slot = (size_t)i * rq.max_faces;
            if (!k[i]) continue;
            if (want_crops && !crops_whole) RF_HIP(hipMemcpy(rq.crops + slot * cb, d_crops + slot * cb, k[i] * cb, hipMemcpyDeviceToHost));
            if (want_mats && !mats_whole) RF_HIP(hipMemcpy(rq.matrices + slot * 6, d_mats + slot * 6, k[i] * mbytes, hipMemcpyDeviceToHost));
        }
    }

    // One enqueue / one chunk of a synchronous call joins the super-batch being assembled (or opens the next lane).  Everything
    // that can fail for a caller-side reason runs BEFORE any state changes: a thrown error leaves no half-open lane or ticket.
    int submit(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, int n, bool on_device,
               float threshold, bool sync_call) {
        const int mb = cap_images_;
        bool need_resize = false, all_registered = true;
        size_t stage_need = 0;
        std::vector<char> empty(n, 0);
        std::vector<size_t> off(n, 0);
        std::vector<int> src_dev(n, -1);          // device frames: >= 0 = resident on that OTHER device, staged by a peer copy
        for (int i = 0; i < n; i++) {
            check_frame(frames[i], rows[i], cols[i], steps[i]);
            empty[i] = !frames[i] || rows[i] <= 0 || cols[i] <= 0;      // img.empty(), RetinaFace.cpp:578-580
            if (empty[i]) continue;
            if (rows[i] > net_h_ || cols[i] > net_w_) need_resize = true;
            if (!on_device) {
                off[i] = stage_need;
                stage_need += align256((size_t)rows[i] * cols[i] * 3);
                all_registered = all_registered && is_registered(frames[i], (size_t)(rows[i] - 1) * steps[i] + (size_t)cols[i] * 3);
            } else if (check_residency_) {
                src_dev[i] = foreign_device_of(frames[i]);
                if (src_dev[i] >= 0) {            // the rows keep the caller's step: one contiguous span, one peer copy
                    off[i] = stage_need;
                    stage_need += align256((size_t)(rows[i] - 1) * steps[i] + (size_t)cols[i] * 3);
                }
            }
        }
        const bool eager_timed = sync_call && !opt_.use_graph;
        // a pending super-batch is closed when this chunk does not fit (images or staging bytes) or must not be mixed with it
        // (different threshold, timed eager run)
        if (pending_lane_ >= 0) {
            Lane &p = lanes_[pending_lane_];
            if (p.n_images + n > mb || p.threshold != threshold || eager_timed || p.timed ||
                (stage_need && p.stage_used + stage_need > p.stage_cap) ||
                (stage_need && !on_device && !p.h_stage))             // the open lane only has a device-side staging block (peer copies so far)
                launch_pending();
        }
        const int id = alloc_ticket();
        if (pending_lane_ < 0) {
            const int lane = pick_lane();
            Lane &s = lanes_[lane];
            harvest(s);                       // waits for the previous super-batch on this lane, if any
            if (stage_need) ensure_stage(s, stage_need, on_device);
            next_lane_ = (lane + 1) % (int)lanes_.size();
            s.n_images = 0;
            s.stage_used = 0;
            s.threshold = threshold;
            s.need_resize = false;
            s.timed = eager_timed;
            s.empty.assign(mb, 0);
            s.tickets.clear();
            pending_lane_ = lane;
            if (eager_timed) RF_HIP(hipEventRecord(s.time_ev[0], s.stream));
        }
        Lane &s = lanes_[pending_lane_];
        Ticket &t = tickets_[id];
        t.state = Ticket::PENDING; t.lane = pending_lane_; t.first_image = s.n_images; t.n = n; t.timed = eager_timed;
        // the launch's frame table (nothing below reads it before it is complete; a throw leaves n_images where it was)
        for (int i = 0; i < n; i++) {
            const int img = s.n_images + i;
            FrameDesc src{nullptr, 0, 0, 0, 0};
            s.empty[img] = empty[i];
            if (!empty[i]) {
                if (on_device && src_dev[i] < 0) src = FrameDesc{frames[i], rows[i], cols[i], steps[i], 0};
                else if (on_device) src = FrameDesc{s.d_stage + s.stage_used + off[i], rows[i], cols[i], steps[i], 0};
                else src = FrameDesc{s.d_stage + s.stage_used + off[i], rows[i], cols[i], cols[i] * 3, 0};
            }
            s.h_frames[img] = src;
            s.h_frames[mb + img] = src;       // replaced by the canvas in launch_pending() when a resize is needed
        }
        try {
            if (stage_need) {
                uint8_t *hbase = s.h_stage + s.stage_used, *dbase = s.d_stage + s.stage_used;
                hipStream_t up = s.stream;
                // staged (pageable) frames: measured 69-74 k -> 76-81 k images/s at 448 x 448 with the second stream (48.6 GB/s = 0.9 of
                // the box's pinned-copy rate); frames in rf_host_register'ed memory got SLOWER with it (75.6 k -> 69.4 k) and stay on one
                if (!on_device && !all_registered && (s.uploads++ & 1)) { up = s.copy2; s.copy2_used = true; }
                if (on_device) {
                    // the batch split of a multi-GPU node: frames resident on another device cross xGMI as one peer copy each
                    // (SDMA, on this lane's stream: it overlaps the compute of the super-batches in flight on the other lanes)
                    // Frames that follow each other in the source allocation AND in the staging block (dense rows, a span that is a
                    // multiple of the 256-byte staging alignment: every BASELINE shape) travel as ONE copy per run -- a contiguous slice of a
                    // sharded batch is one SDMA descriptor instead of 32 (round 6; RF_SCATTER_PER_FRAME=1 keeps one copy per frame for the A/B).
                    for (int i = 0; i < n; i++) {
                        if (empty[i] || src_dev[i] < 0) continue;
                        const FrameRun run = frame_run(frames, rows, cols, steps, empty.data(), off.data(), i, n, scatter_per_frame_,
                                                       [&](int a, int b) { return src_dev[a] == src_dev[b]; });
                        RF_HIP(hipMemcpyPeerAsync(dbase + off[i], device_, frames[i], src_dev[i], run.bytes, s.stream));
                        scattered_frames_ += run.end - i;
                        peer_copies_++;
                        i = run.end - 1;
                    }
                } else if (all_registered) {
                    // caller buffers pinned with rf_host_register: the DMA engine reads them in place.  Frames with dense rows
                    // that follow each other in memory (a ring of camera buffers) and in the staging block go as ONE copy.
                    upload_registered(frames, rows, cols, steps, empty, off, 0, n, dbase, up);
                } else {
                    // PIPELINED STAGING of a synchronous call (round 6): the reference's calling convention is ONE call
                    // that uploads, preprocesses and infers (RetinaFace.cpp:749-846), and through round 5 such a call ran staging copy, PCIe
                    // transfer and compute strictly one after the other (batch 8 at 448 x 448, C ABI: 0.285 ms = 0.06 + 0.10 + 0.13).  The frames
                    // are now staged and sent in pieces of ~kStagePieceBytes: while piece k crosses the bus the host stages piece k + 1.  Same
                    // stream, same bytes, same launch afterwards: results are byte-identical (RF_SYNC_SPLIT=0 = one piece, the A/B).
                    // Measured and rejected in the same round (profiles/r06_sync_host_call_ab.txt): sending the pieces on the copy stream and
                    // starting the STEM of each piece behind its event -- 4 events + 4 cross-stream waits + 4 eager launches + a second graph
                    // cost more host time (0.309 / 0.278 ms pageable / registered) than the 13 us stem they hid (0.285 / 0.224 ms unsplit).
                    const int pieces = (sync_call && stage_pieces_ > 1) ? (int)std::min<size_t>((size_t)stage_pieces_, std::max<size_t>(1, stage_need / kStagePieceBytes)) : 1;
                    if (pieces <= 1) {
                        copy_jobs_.clear();
                        for (int i = 0; i < n; i++)
                            if (!empty[i])
                                copy_jobs_.push_back(ParallelCopier::Job{hbase + off[i], frames[i], (size_t)cols[i] * 3, (size_t)rows[i], (size_t)steps[i]});
                        copier_->run(copy_jobs_);          // the caller's buffers are free again when this returns
                        RF_HIP(hipMemcpyAsync(dbase, hbase, stage_need, hipMemcpyHostToDevice, up));
                    } else {
                        // staging.h cuts the block into the pieces; while piece k crosses the bus the host stages piece k + 1
                        for (const StagePiece &pc : stage_piece_plan(frames, rows, cols, steps, empty.data(), off.data(), n, stage_need, pieces, hbase)) {
                            if (pc.jobs.empty()) continue;
                            copier_->run(pc.jobs);         // the caller's rows of this piece are free again when this returns
                            RF_HIP(hipMemcpyAsync(dbase + pc.sent, hbase + pc.sent, pc.end - pc.sent, hipMemcpyHostToDevice, up));
                        }
                        staged_pieces_ += pieces;
                    }
                }
            }
        } catch (...) {
            t.state = Ticket::FREE;
            throw;
        }
        s.stage_used += stage_need;
        s.need_resize = s.need_resize || need_resize;
        s.n_images += n;
        s.tickets.push_back(id);
        // launch now when full, when the caller is synchronous, or when coalescing is off
        if (s.n_images + 1 > mb || sync_call || opt_.coalesce == 1) launch_pending();
        return id;
    }

    // frames [a, b) of a chunk, in pinned caller memory, to their places in the device staging block: one DMA per run of dense frames that
    // follow each other in memory and in the block, a 2-D copy for frames with a row pitch
    void upload_registered(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, const std::vector<char> &empty,
                           const std::vector<size_t> &off, int a, int b, uint8_t *dbase, hipStream_t up) {
        for (int i = a; i < b; i++) {
            if (empty[i]) continue;
            if (steps[i] != cols[i] * 3) {
                RF_HIP(hipMemcpy2DAsync(dbase + off[i], (size_t)cols[i] * 3, frames[i], (size_t)steps[i], (size_t)cols[i] * 3,
                                        (size_t)rows[i], hipMemcpyHostToDevice, up));
                continue;
            }
            const FrameRun run = frame_run(frames, rows, cols, steps, empty.data(), off.data(), i, b, false, [](int, int) { return true; });
            RF_HIP(hipMemcpyAsync(dbase + off[i], frames[i], run.bytes, hipMemcpyHostToDevice, up));
            i = run.end - 1;
        }
    }

    hipGraphExec_t capture(Lane &L, int n) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        RF_HIP(hipStreamBeginCapture(L.stream, hipStreamCaptureModeThreadLocal));
        std::string err;
        try {
            for (size_t k = 0; k < L.ops.size(); k++) L.ops[k].launch(L.stream, n);
        } catch (const std::exception &e) { err = e.what(); }
        hipError_t end = hipStreamEndCapture(L.stream, &g);
        if (!err.empty() || end != hipSuccess || !g)
            throw HipError("hipGraph capture failed: " + (err.empty() ? std::string(hipGetErrorString(end)) : err));
        hipError_t inst = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (inst != hipSuccess) throw HipError(std::string("hipGraphInstantiate failed: ") + hipGetErrorString(inst));
        return ge;
    }

    // ------------------------------------------------------------------------------------------ state
    int device_ = 0;
    HostTrace trace_;
    bool check_residency_ = false, force_scatter_ = false, scatter_per_frame_ = false;
    int stage_pieces_ = 4;                    // most pieces a synchronous host-frame call is staged + sent in (RF_SYNC_SPLIT=0: one, as rounds 1-5; RF_SYNC_PIECES=n)
    static constexpr size_t kStagePieceBytes = 1200 << 10;      // ~2 frames of 448 x 448: 24 us on the bus, ~15 us of staging
    long staged_pieces_ = 0;
    long scattered_frames_ = 0;               // device frames that arrived from another device
    long peer_copies_ = 0;                    // ... in this many hipMemcpyPeerAsync calls (one per contiguous run of frames)
    long long launches_ = 0;                  // super-batches launched (launch_pending()) ...
    long long launched_images_ = 0;           // ... and the images in them
    std::vector<float> ratios_;                // the network preset's anchor ratios (empty: a preset without anchors)
    int na_ = 2;                               // anchors per cell the preset decodes (head_a_: what the model's heads carry)
    std::unique_ptr<ParallelCopier> copier_;
    std::vector<ParallelCopier::Job> copy_jobs_;
    struct HostRange { uintptr_t base; size_t bytes; bool owned; };
    std::vector<HostRange> registered_;       // rf_host_register ranges (pinned caller memory; owned = pinned by this engine)
    std::vector<hipEvent_t> prof_ev_;
    std::vector<void *> dev_allocs_, host_allocs_;

    NetKind kind_;
    Plan plan_;                               // skeleton (shapes, names): what build_lane needs when a lane is built later
    Lane *building_ = nullptr;
    std::vector<Lane> lanes_;
    int next_lane_ = 0, last_lane_ = 0, last_first_image_ = 0, pending_lane_ = -1;
    unsigned long long launch_counter_ = 0;
    ResidencyCache residency_;                // where the allocations behind device frame pointers live (foreign_device_of)
    int cap_images_ = 0;                      // images per launch = max_batch * coalesce
    std::vector<Ticket> tickets_;
    int next_ticket_ = 0;

    // face alignment: device scratch that grows to the largest call seen (every alignment call is synchronous, so nothing is in
    // flight on a block when it is replaced), and the side stream of the standalone calls
    struct DeviceScratch {
        uint8_t *ptr = nullptr; size_t cap = 0;
        uint8_t *reserve(size_t bytes) {
            if (bytes > cap) {
                if (ptr) (void)hipFree(ptr);
                ptr = nullptr; cap = 0;
                const size_t want = (std::max<size_t>(bytes, 4096) + 4095) / 4096 * 4096;
                RF_HIP(hipMalloc((void **)&ptr, want));
                cap = want;
            }
            return ptr;
        }
        void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; cap = 0; }
    };
    DeviceScratch align_crops_, align_mats_, align_tab_;
    std::vector<uint8_t> align_host_;
    hipStream_t align_stream_ = nullptr;
    static constexpr int kAlignImagesPerLaunch = 32768;       // grid.z limit of one launch
    // face batches: the running base of packed offsets (one device int)
    DeviceScratch fb_state_;
    // gated face batches: quality records and packed indices per face slot of the call, the call's packed offsets
    DeviceScratch fq_records_, fq_packed_, fq_offsets_;
    // pass calls: the one that is open, the device copy of its host frames, the event behind its side-stream copies
    PassCall passes_;
    DeviceScratch pass_frames_;
    hipEvent_t inputs_ready_ = nullptr;
    hipEvent_t caller_ready_ = nullptr;       // face_batch(): the default stream's work on a caller's tensor, recorded in front of the launches
    // tiled detection: per frame the gathered candidates and their counter, the merged records and counts, the frame table of the
    // fused face batch
    DeviceScratch tile_cand_, tile_count_, tile_out_, tile_outcount_, tile_tab_;
    bool tile_dirty_ = true;                  // the counters are not known to be zero (new block, or a call that ended in an error)
    std::vector<Candidate> tile_host_;
    std::vector<FrameDesc> tile_fd_;
    // flip test-time augmentation: per frame the gathered candidates and their counter, the mirrored copies; the merged records, member
    // counts and counts are tta_out_ / tta_votes_ / tta_outcount_ below.  Pyramid and rotation calls use the same blocks
    // (pyr_merge_spec, rot_merge_spec) and bring the zoom tiles / the rotated copies.
    DeviceScratch tta_cand_, tta_count_, tta_mirror_, pyr_zoom_, rot_copies_;
    // fisheye detection (dewarp.h): the dewarpers of this handle (a camera's shapes and its meshes in device memory) and the views of a
    // call; the call gathers into the TTA blocks too (dewarp_merge_spec)
    struct Dewarper {
        int rows = 0, cols = 0, view_w = 0, view_h = 0, views = 0;
        DeviceScratch mesh;                   // views x nodes_y x nodes_x x 2 int32
        size_t view_ints() const { return dewarp_view_ints(view_w, view_h); }
        size_t view_bytes() const { return (size_t)view_w * view_h * 3; }      // a multiple of 768: dense views stay 256-byte aligned
        const int32_t *view_mesh(int v) const { return (const int32_t *)mesh.ptr + (size_t)v * view_ints(); }
    };
    std::vector<std::unique_ptr<Dewarper>> dewarpers_;
    DeviceScratch dewarp_views_;
    // region detection (roi.h): the cell records of a call (device block; roi_cells_pin_ below stages them) and its views; the call gathers into the TTA
    // blocks too (roi_merge_request)
    DeviceScratch roi_cells_, roi_views_;
    // change regions (change.h): the changers of this handle -- per stream the reference image, the last mask (before dilation) and
    // the frame counter, in device memory; a call's records and info share roi_cells_
    struct Changer {
        ChangeSpec spec;
        int rows = 0, cols = 0, bw = 0, bh = 0, n_streams = 0;
        DeviceScratch ref, mask, frames;
        bool dirty = false;                   // a call on it ended in an error: refused until it is reset
        size_t mask_pitch() const { return align256((size_t)bw * bh); }
        void release() { ref.release(); mask.release(); frames.release(); }
    };
    std::vector<std::unique_ptr<Changer>> changers_;
    // low-light enhancement (enhance.h): LUTs | flags | per-frame counts of a call, and the enhanced copies of a fused call
    DeviceScratch enh_luts_, enh_frames_;
    bool tta_dirty_ = true;

    // face tracks: the trackers of this handle, the call-level result buffers and the request a tracked call has open
    struct Tracker {
        TrackSpec spec;
        int n_streams = 0;
        DeviceScratch state;                  // n_streams x (TrackHeader + max_tracks records)
        bool dirty = false;                   // a call on it ended in an error: refused until it is reset
        // the best-shot gallery (shot.h), fixed by tracker_enable_shots(): n_streams x max_tracks entries of the resolved spec's
        // bytes_per_face, and as many rf_shot records
        bool has_shots = false;
        FaceBatchSpec shot_spec;
        DeviceScratch gallery, shot_records;
        // motion (motion.h), fixed by tracker_enable_motion(): n_streams x max_tracks rf_track_motion records
        bool has_motion = false;
        MotionSpec motion_spec;
        DeviceScratch motion;
        size_t stream_bytes() const { return sizeof(TrackHeader) + (size_t)spec.max_tracks * sizeof(rf_track); }
        // follow (follow.h), fixed by tracker_enable_follow(): n_streams x max_tracks rf_track_follow records and 1024-byte templates
        bool has_follow = false;
        FollowSpec follow_spec;
        DeviceScratch follow_records, follow_templates;
        size_t motion_bytes() const { return (size_t)spec.max_tracks * sizeof(rf_track_motion); }
        size_t follow_bytes() const { return (size_t)spec.max_tracks * sizeof(rf_track_follow); }
        void release() { state.release(); gallery.release(); shot_records.release(); motion.release(); follow_records.release(); follow_templates.release(); }
    };
    std::vector<std::unique_ptr<Tracker>> trackers_;
    // (pinned host memory the kernel writes straight into, as the NMS kernel writes its result block: no copy after the call)
    struct HostScratch {
        uint8_t *ptr = nullptr; size_t cap = 0;
        uint8_t *reserve(size_t bytes) {
            if (bytes > cap) {
                if (ptr) (void)hipHostFree(ptr);
                ptr = nullptr; cap = 0;
                const size_t want = (std::max<size_t>(bytes, 4096) + 4095) / 4096 * 4096;
                RF_HIP(hipHostMalloc((void **)&ptr, want, hipHostMallocDefault));
                cap = want;
            }
            return ptr;
        }
        void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; cap = 0; }
    };
    HostScratch trk_tags_, trk_ended_, trk_counts_, enh_counts_, roi_cells_pin_;
    // best-shot gallery: the call-level blocks the deliver kernel writes (shots, records; indexed image * cap_ended + e), the events
    // around the shot launches of track_shots() (tools/shot_bench.py reads the time) and the request a shot call has open
    HostScratch shot_out_, shot_info_;
    hipEvent_t shot_ev_[2] = {nullptr, nullptr};
    float shot_launch_ms_ = -1.f;
    HostScratch tta_out_, tta_votes_, tta_outcount_;      // detect_tta() / tta_merge(): what the voting merge writes (see tta_open)
    // followed tracks: what the search launch hands to the step launch (device), the followed faces | their counts of a call (pinned,
    // the step kernel writes them) and the events around the two launches of track_follow() (tools/follow_bench.py reads the time)
    DeviceScratch fol_results_;
    HostScratch fol_out_;
    hipEvent_t fol_ev_[2] = {nullptr, nullptr};
    float fol_launch_ms_ = -1.f;
    hipEvent_t trk_ev_[2] = {nullptr, nullptr};   // around the track launch of track_update() (tools/track_bench.py reads the time)
    float trk_launch_ms_ = -1.f;
    hipEvent_t red_ev_[2] = {nullptr, nullptr};   // around the redaction launches of redact() (tools/redact_bench.py reads the time)
    float red_launch_ms_ = -1.f, ov_launch_ms_ = -1.f;

    // face redaction: region records, region counts (after | before the cut) + owned-pixel counts, and cell values of the call's
    // images, the device copy of host frames; the request a redacting call has open
    DeviceScratch red_regions_, red_counts_, red_cells_, red_frames_;
    DeviceScratch red_shadow_;                    // a blurring call: offset table | the blurred owned pixels of every frame of the call
    std::vector<unsigned long long> red_shadow_off_;
    std::vector<int> red_host_;
    DeviceScratch ov_regions_;                    // an overlay call's region records (overlay.h), in the place of red_regions_

    // The open stage call (detect_staged()): what each stage has bound for the call, and ONE cursor -- every launch between the open and
    // the end of the call carries images of this call only, in call order, so image i of a launch is image next_image + i of the call for
    // every stage.  What remains per stage is what really differs: the face batch's scan chain (first, prev_scan), the track chain
    // (prev) and the streams of the lane's last track launch (last_streams).  The standalone calls bind the same per-stage blocks
    // (track_params(), shot_launches() and redact_params() read them) and never arm a stage.
    struct StageOpen {
        const char *who = "";                 // the stage the call's launch errors name
        int n = 0, next_image = 0;
        struct { bool on = false; AlignRequest rq; uint8_t *d_crops = nullptr; double *d_mats = nullptr; } align;
        struct { bool on = false, first = true; FaceBatchRequest rq; uint8_t *d_tensor = nullptr; double *d_mats = nullptr; hipEvent_t prev_scan = nullptr; } fb;
        struct { bool on = false; Tracker *tr = nullptr; const int *stream_of_image = nullptr; int n = 0, tag_stride = 0, cap_ended = 0, max_faces = 0;
                 const rf_face_quality *records = nullptr; hipEvent_t prev = nullptr; } trk;
        struct { bool on = false; uint8_t *d_out = nullptr; bool host = false, info = false; int last_streams = 0; } shot;
        struct { bool on = false; } follow;   // the keep launch behind every track launch (launch_lane_follow())
        struct { bool on = false; RedactSpec spec; Tracker *tr = nullptr; const int *stream_of_image = nullptr; int n = 0; bool overlay = false;
                 OverlaySpec ospec; } red;
        bool armed() const { return align.on || fb.on || trk.on || shot.on || red.on || follow.on; }
        void disarm() { align.on = fb.on = trk.on = shot.on = red.on = follow.on = false; }
    } call_;

    int last_n_ = 0;
    std::vector<int> last_cand_counts_;
    std::vector<std::vector<int32_t>> last_anchor_;
    float t_pre_ = 0, t_infer_ = 0, t_post_ = 0, t_total_ = 0;
    bool have_split_ = false;
};

}  // namespace

std::string plan_cache_path(const std::string &model_dir, const std::string &stem, int precision) {
    static const char *names[3] = {"fp32", "fp16", "int8"};
    return model_dir + "/" + stem + "." + names[precision < 0 || precision > 2 ? 1 : precision] + ".rfplan";
}

// Host-only half of engine start-up: the packed weight image and the plan skeleton, from the plan cache when it matches the
// model files, otherwise from the model (and then the cache is (re)written, best effort: a read-only model directory is fine).
template <typename T>
void prepare_pack(const std::string &model_dir, const EngineOptions &opt, Plan *plan, WeightPack<T> *pack, bool *from_cache) {
    PlanCacheKey key;
    key.build = 1469598103934665603ull;
    for (const char *c = __DATE__ " " __TIME__ " " __FILE__; *c; c++) { key.build ^= (unsigned char)*c; key.build *= 1099511628211ull; }
    key.precision = opt.precision;
    const std::string path = opt.plan_cache_path.empty() ? plan_cache_path(model_dir, opt.model_stem, opt.precision) : opt.plan_cache_path;
    *from_cache = false;
    if (opt.plan_cache) {
        key.source_hash = model_source_hash(model_dir, opt.model_stem);        // throws IoError when the model is missing
        std::string bytes;
        if (read_file_if_exists(path, &bytes)) {
            try {
                if (load_plan_cache<T>(bytes, key, plan, pack)) { *from_cache = true; return; }
            } catch (const IoError &) { /* damaged cache file: rebuild below and overwrite it */ }
            *plan = Plan();
            *pack = WeightPack<T>();
        }
    }
    Model model = load_model_dir(model_dir, opt.model_stem);
    *plan = compile_plan(model);
    if (opt.precision == RF_PRECISION_INT8 && plan->int8_scales.empty())
        throw Unsupported("int8 precision needs a calibration table (<stem>.table.int8, or scales inside the .rfw)");
    pack->pack(*plan);
    if (opt.plan_cache) write_file_best_effort(path, save_plan_cache<T>(key, *plan, *pack));
}

template <typename T>
static std::unique_ptr<Engine> make_engine(const std::string &model_dir, const std::string &network, float nms, const EngineOptions &opt,
                                           const std::vector<float> &ratios) {
    Plan plan;
    WeightPack<T> pack;
    bool from_cache = false;
    prepare_pack<T>(model_dir, opt, &plan, &pack, &from_cache);       // host-only steps first: their errors do not need a GPU
    if (!ratios.empty() && 2 * (int)ratios.size() != plan.anchors_per_cell)
        // the reference would index past the end of the score blob here (RetinaFace.cpp:669-694 with _num_anchors != blob channels / 2)
        throw ModelError("network preset '" + network + "' decodes " + std::to_string(2 * ratios.size()) + " anchors per cell but the model's "
                         "heads carry " + std::to_string(plan.anchors_per_cell));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw HipError("no HIP device available");
    auto wp = std::make_shared<WeightPack<T>>(std::move(pack));
    NetKind kind;
    kind.elem_bytes = sizeof(T);
    kind.tag = sizeof(T) == 1 ? "int8" : sizeof(T) == 2 ? "fp16" : "fp32";
    kind.cvt_selfcheck = sizeof(T) == 1;
    kind.to_float = [](const void *raw, size_t n, float *dst) { for (size_t i = 0; i < n; i++) dst[i] = Cast<T>::to(((const T *)raw)[i]); };
    kind.arena = &wp->arena_;
    kind.head_a = wp->head_a_;
    kind.build_net = [wp](const Plan &p, const NetSite &site, LaneNet *net) { build_net<T>(p, *wp, site, net); };
    return std::unique_ptr<Engine>(new EngineImpl(plan, std::move(kind), nms, opt, ratios));
}

// test hook (host only): build / validate the plan cache of one model without creating an engine
int plan_cache_probe(const std::string &model_dir, const EngineOptions &opt, size_t *arena_bytes) {
    Plan plan;
    bool hit = false;
    switch (opt.precision) {
        case RF_PRECISION_FP16: { WeightPack<half_t> p; prepare_pack<half_t>(model_dir, opt, &plan, &p, &hit); if (arena_bytes) *arena_bytes = p.arena_.bytes(); break; }
        case RF_PRECISION_FP32: { WeightPack<float> p; prepare_pack<float>(model_dir, opt, &plan, &p, &hit); if (arena_bytes) *arena_bytes = p.arena_.bytes(); break; }
        case RF_PRECISION_INT8: { WeightPack<int8_t> p; prepare_pack<int8_t>(model_dir, opt, &plan, &p, &hit); if (arena_bytes) *arena_bytes = p.arena_.bytes(); break; }
        default: throw ArgError("unknown precision");
    }
    return hit ? 1 : 0;
}

std::unique_ptr<Engine> Engine::create_single(const std::string &model_dir, const std::string &network, float nms,
                                              const EngineOptions &opt) {
    std::vector<float> ratios;
    (void)network_preset(network, &ratios);       // unknown names behave like "ssh": constructed, no anchors (RetinaFace.cpp:237-239)
    switch (opt.precision) {
        case RF_PRECISION_FP16: return make_engine<half_t>(model_dir, network, nms, opt, ratios);
        case RF_PRECISION_FP32: return make_engine<float>(model_dir, network, nms, opt, ratios);
        case RF_PRECISION_INT8: return make_engine<int8_t>(model_dir, network, nms, opt, ratios);
        default: throw ArgError("unknown precision");
    }
}

}  // namespace rf
