// net.cpp -- see net.h.
#include "net.h"

#include "knobs.h"

namespace rf {

namespace {

// The launch closure of a parameter block that carries the image count: a copy of the block (of the three FPN levels' blocks)
// with n filled in.
template <typename P, typename F> std::function<void(hipStream_t, int)> with_n(const P &p, F launch) {
    return [p, launch](hipStream_t s, int n) { P q = p; q.n = n; launch(s, q); };
}
template <typename P, typename F> std::function<void(hipStream_t, int)> with_n3(const P (&lv)[3], F launch) {
    struct Levels { P p[3]; } c{{lv[0], lv[1], lv[2]}};
    return [c, launch](hipStream_t s, int n) { Levels q = c; for (auto &p : q.p) p.n = n; launch(s, q.p, 3); };
}

}  // namespace

template <typename T> void build_net(const Plan &plan, const WeightPack<T> &wp, const NetSite &site, LaneNet *net) {
    typedef typename DwWeightT<T>::type DWT;
    typedef typename WeightPack<T>::GemmW GemmW;
    constexpr size_t kNone = WeightPack<T>::kNone;
    const Arena &A = wp.arena_;
    LaneNet &L = *net;
    const int mb = site.mb;
    const int H = site.net_h, W = site.net_w;
    const double P = (double)H * W;
    auto act = [&](const std::string &name, int h, int w, int c) {
        T *p = (T *)site.dalloc((size_t)mb * h * w * c * sizeof(T));
        auto sc = wp.act_scale_.find(name);
        L.acts[name] = ActInfo{p, h, w, c, sc == wp.act_scale_.end() ? std::vector<float>() : sc->second};
        return p;
    };
    // activations: one buffer per reference blob that survives fusion (288 GB of HBM: nothing is recycled)
    int h = H / 2, w = W / 2;
    T *cur = nullptr;
    size_t first_block = 0;
    int c = 8;
    if constexpr (std::is_same<T, half_t>::value) {
        // fp16 engine: preprocess + conv0 + blocks 0 and 1 (conv1..conv4) are ONE launch (stem2_kernel): the 224^2 x 16 map of
        // the net never exists in HBM
        const auto &b0 = plan.blocks[0], &b1 = plan.blocks[1];
        const int h4 = H / 4, w4 = W / 4;
        T *out = act(b1.pw.out_blob, h4, w4, b1.pw.cout);
        Stem2Params sp;
        sp.frames = site.frames; sp.out = out;
        sp.w0 = A.ptr<half_t>(wp.c0_hi_); sp.b0 = A.ptr<float>(wp.c0_b_mma_);
        sp.w0_raw = A.ptr<half_t>(wp.c0_raw_);
        sp.dw0_w = A.ptr<float>(wp.stem_dw_.w); sp.dw0_b = A.ptr<float>(wp.stem_dw_.b);
        sp.pw0_w = A.ptr<half_t>(wp.stem_pw_.w); sp.pw0_b = A.ptr<float>(wp.stem2_c2_b_);
        sp.c2_floor = A.ptr<uint32_t>(wp.stem2_c2_floor_); sp.c3_floor = A.ptr<uint32_t>(wp.stem2_c3_floor_);
        sp.dw1_mma = A.ptr<uint32_t>(wp.stem2_dw_.mma); sp.dw1_b = A.ptr<float>(wp.stem2_dw_.b);
        sp.pw1_w = A.ptr<half_t>(wp.stem2_pw_.w); sp.pw1_b = A.ptr<float>(wp.stem2_pw_.b);
        sp.n = 0; sp.net_h = H; sp.net_w = W;
        OpInfo op;
        op.name = "pre+" + plan.conv0.name + "+" + b0.dw.name + "+" + b0.pw.name + "+" + b1.dw.name + "+" + b1.pw.name;
        op.kernel = "stem2";
        op.alg_u8_in = 3.0 * P;
        // layer-wise accounting: every covered layer's input + output elements, fused or not
        op.alg_elems_in = 8.0 * h * w + 8.0 * h * w + 16.0 * h * w + 16.0 * h4 * w4;                       // conv1, conv2, conv3, conv4 inputs
        op.alg_elems_out = 8.0 * h * w + 8.0 * h * w + 16.0 * h * w + 16.0 * h4 * w4 + 32.0 * h4 * w4;     // conv0 .. conv4 outputs
        op.macs = (plan.conv0.macs_per_out_pixel() + b0.dw.macs_per_out_pixel() + b0.pw.macs_per_out_pixel()) * h * w +
                  (b1.dw.macs_per_out_pixel() + b1.pw.macs_per_out_pixel()) * h4 * w4;
        op.hbm_elems_out = 32.0 * h4 * w4;                        // the frame in (alg_u8_in), the 32-channel net/4 map out
        op.launch = with_n(sp, launch_stem2);
        L.ops.push_back(op);
        cur = out; c = b1.pw.cout; first_block = 2; h = h4; w = w4;
        if (plan.blocks.size() > 3 && plan.blocks[2].dw.cout == 32 && plan.blocks[2].pw.cout == 32 &&
            plan.blocks[3].dw.stride == 2 && plan.blocks[3].pw.cout == 64) {
            // blocks 2 and 3 (conv5..conv8) as ONE launch (dwpw2_kernel): the 112^2 x 32 map between them stays in LDS
            const auto &ba = plan.blocks[2], &bb = plan.blocks[3];
            T *out2 = act(bb.pw.out_blob, h / 2, w / 2, bb.pw.cout);
            DwPw2Params dp;
            dp.in = cur; dp.out = out2;
            dp.dwa_mma = A.ptr<uint32_t>(wp.dw_w_[2].mma); dp.dwa_b = A.ptr<float>(wp.dw_w_[2].b);
            dp.pwa_w = A.ptr<half_t>(wp.pw_w_[2].w); dp.pwa_b = A.ptr<float>(wp.pw_w_[2].b);
            dp.dwb_mma = A.ptr<uint32_t>(wp.dw_w_[3].mma); dp.dwb_b = A.ptr<float>(wp.dw_w_[3].b);
            dp.pwb_w = A.ptr<half_t>(wp.pw_w_[3].w); dp.pwb_b = A.ptr<float>(wp.pw_w_[3].b);
            dp.n = 0; dp.hin = h; dp.win = w;
            OpInfo o2;
            o2.name = ba.dw.name + "+" + ba.pw.name + "+" + bb.dw.name + "+" + bb.pw.name;
            o2.kernel = "dwpw2<32,32,64>";
            const double pa = (double)h * w, pb = (double)(h / 2) * (w / 2);
            o2.alg_elems_in = 32.0 * pa + 32.0 * pa + 32.0 * pa + 32.0 * pb;          // dw A, pw A, dw B, pw B inputs (layer-wise)
            o2.alg_elems_out = 32.0 * pa + 32.0 * pa + 32.0 * pb + 64.0 * pb;
            o2.macs = (ba.dw.macs_per_out_pixel() + ba.pw.macs_per_out_pixel()) * pa + (bb.dw.macs_per_out_pixel() + bb.pw.macs_per_out_pixel()) * pb;
            o2.hbm_elems_in = 32.0 * pa; o2.hbm_elems_out = 64.0 * pb;
            o2.launch = with_n(dp, launch_dwpw2);
            L.ops.push_back(o2);
            cur = out2; c = bb.pw.cout; first_block = 4; h /= 2; w /= 2;
        }
    } else if constexpr (sizeof(T) == 1) {
        // int8 engine: preprocess + conv0 + the first depthwise/pointwise
        // block are ONE launch (stem_kernel); it computes in fp16 and stores its 16-channel output in the engine's storage type
        const auto &blk = plan.blocks[0];
        T *out = act(blk.pw.out_blob, h, w, blk.pw.cout);
        StemParams<T> sp;
        sp.frames = site.frames; sp.out = out;
        sp.w0 = A.ptr<half_t>(wp.c0_hi_); sp.b0 = A.ptr<float>(wp.c0_b_mma_);
        sp.w0_raw = A.ptr<half_t>(wp.c0_raw_);
        sp.dw_w = A.ptr<float>(wp.stem_dw_.w); sp.dw_b = A.ptr<float>(wp.stem_dw_.b);
        sp.pw_w = A.ptr<half_t>(wp.stem_pw_.w); sp.pw_b = A.ptr<float>(wp.stem_pw_.b);
        sp.pw_m = wp.mult_ptr(wp.stem_pw_);
        sp.n = 0; sp.net_h = H; sp.net_w = W;
        OpInfo op;
        op.name = "pre+" + plan.conv0.name + "+" + blk.dw.name + "+" + blk.pw.name;
        op.kernel = "stem";
        op.alg_u8_in = 3.0 * P;
        op.alg_elems_in = 8.0 * h * w + 8.0 * h * w;                       // dw input, pw input
        op.alg_elems_out = 8.0 * h * w + 8.0 * h * w + 16.0 * h * w;       // conv0, dw, pw outputs
        op.macs = (plan.conv0.macs_per_out_pixel() + blk.dw.macs_per_out_pixel() + blk.pw.macs_per_out_pixel()) * h * w;
        op.hbm_elems_out = 16.0 * h * w;
        op.launch = with_n(sp, launch_stem<T>);
        L.ops.push_back(op);
        cur = out; c = blk.pw.cout; first_block = 1;
    } else {
        cur = act(plan.conv0.out_blob, h, w, 8);
        OpInfo op;
        op.name = "pre+" + plan.conv0.name;
        op.kernel = "conv0";
        op.alg_u8_in = 3.0 * P;
        op.alg_elems_out = 8.0 * h * w;
        op.macs = plan.conv0.macs_per_out_pixel() * h * w;
        op.hbm_elems_out = 8.0 * h * w;
        const float *w0 = A.ptr<float>(wp.c0_w_), *b0 = A.ptr<float>(wp.c0_b_);
        const FrameDesc *fr = site.frames;
        T *o = cur;
        op.launch = [=](hipStream_t s, int n) { launch_conv0<T>(s, fr, o, w0, b0, n, H, W); };
        L.ops.push_back(op);
    }
    // FPN tap -> lateral index: block 4 (stride 8) -> lateral[2], block 10 (stride 16) -> [1], block 12 (stride 32) -> [0]
    T *lat[3] = {nullptr, nullptr, nullptr};
    for (size_t i = first_block; i < plan.blocks.size(); i++) {
        const auto &blk = plan.blocks[i];
        int ho = h / blk.dw.stride, wo = w / blk.dw.stride;
        T *out = act(blk.pw.out_blob, ho, wo, blk.pw.cout);
        if (dwpw_tile_info<T>(c, blk.pw.cout, blk.dw.stride, true, ho, wo).th == 0)
            throw ModelError("no kernel instance for depthwise/pointwise block " + blk.dw.name);
        DwPwParams<T> p;
        p.in = cur; p.out = out;
        p.dw_w = A.ptr<DWT>(wp.dw_w_[i].w); p.dw_b = A.ptr<float>(wp.dw_w_[i].b);
        if (wp.dw_w_[i].mma) p.dw_mma = A.ptr<uint32_t>(wp.dw_w_[i].mma);
        if (wp.dw_w_[i].m != kNone) p.dw_m = A.ptr<float>(wp.dw_w_[i].m);
        p.pw_w = A.ptr<T>(wp.pw_w_[i].w); p.pw_b = A.ptr<float>(wp.pw_w_[i].b); p.pw_m = wp.mult_ptr(wp.pw_w_[i]);
        p.n = 0; p.hin = h; p.win = w; p.hout = ho; p.wout = wo;
        p.cin = c; p.cout = blk.pw.cout; p.stride = blk.dw.stride; p.has_dw = true;
        OpInfo op;
        op.name = blk.dw.name + "+" + blk.pw.name;
        op.kernel = "dwpw<" + std::to_string(c) + "," + std::to_string(blk.pw.cout) + ",s" + std::to_string(blk.dw.stride) + ">";
        op.alg_elems_in = (double)c * h * w + (double)c * ho * wo;
        op.alg_elems_out = (double)c * ho * wo + (double)blk.pw.cout * ho * wo;
        op.macs = (blk.dw.macs_per_out_pixel() + blk.pw.macs_per_out_pixel()) * ho * wo;
        op.hbm_elems_in = (double)c * h * w; op.hbm_elems_out = (double)blk.pw.cout * ho * wo;
        const int li = i == 4 ? 2 : i == 10 ? 1 : i == 12 ? 0 : -1;
        if (li >= 0) {          // the lateral 1x1 is computed from this block's output tile while it is in LDS
            const FoldedConv &lf = plan.lateral[li];
            lat[li] = act(lf.out_blob, ho, wo, 64);
            p.lat_w = A.ptr<T>(wp.lat_w_[li].w); p.lat_b = A.ptr<float>(wp.lat_w_[li].b); p.lat_out = lat[li];
            p.lat_m = wp.mult_ptr(wp.lat_w_[li]);
            op.name += "+" + lf.name;
            op.kernel.insert(op.kernel.size() - 1, ",lat");
            op.alg_elems_in += (double)blk.pw.cout * ho * wo;
            op.alg_elems_out += 64.0 * ho * wo;
            op.hbm_elems_out += 64.0 * ho * wo;
            op.macs += lf.macs_per_out_pixel() * ho * wo;
        }
        op.launch = with_n(p, launch_dwpw<T>);
        L.ops.push_back(op);
        cur = out; h = ho; w = wo; c = blk.pw.cout;
    }
    // FPN: P3 = c3 lateral; P2 / P1 = aggr conv with "lateral + bilinear x2 upsample(coarser)" fused into its input staging
    T *feat[3];
    feat[0] = lat[0];
    for (int i = 0; i < 2; i++) {
        int fh = H / kStrides[i + 1], fw = W / kStrides[i + 1];
        feat[i + 1] = act(plan.aggr[i].out_blob, fh, fw, 64);
        Conv3Params<T> p;
        p.in = lat[i + 1]; p.in_ld = 64; p.in_off = 0; p.up = feat[i];
        p.w = A.ptr<T>(wp.aggr_w_[i].w); p.b = A.ptr<float>(wp.aggr_w_[i].b); p.m = wp.mult_ptr(wp.aggr_w_[i]);
        p.a_lat = wp.aggr_a_lat_[i]; p.a_up = wp.aggr_a_up_[i];
        p.blend_fp32 = knob(K_BLEND_FP32) != 0;            // read once per lane (not per launch)
        p.out0 = feat[i + 1]; p.ld0 = 64; p.off0 = 0; p.n0 = 64; p.out1 = nullptr; p.ld1 = 0; p.off1 = 0;
        p.n = 0; p.h = fh; p.w_ = fw; p.cin = 64; p.cout = 64;
        OpInfo op;
        op.name = std::string(i == 0 ? "rf_c3_upsampling" : "rf_c2_upsampling") + "+" + plan.aggr[i].name;
        {
            TileInfo ti = conv3x3_tile_info<T>(64, 64, fh, fw);
            op.kernel = "conv3x3<64,64," + std::to_string(ti.th) + "x" + std::to_string(ti.tw) + ",up>";
        }
        op.alg_elems_in = 64.0 * (fh / 2) * (fw / 2) + 64.0 * fh * fw;     // deconv input + conv input
        op.alg_elems_out = 64.0 * fh * fw + 64.0 * fh * fw;               // deconv output + conv output
        op.macs = plan.aggr[i].macs_per_out_pixel() * fh * fw + 16.0 * 64 * (fh / 2) * (fw / 2);
        op.hbm_elems_in = 64.0 * (fh / 2) * (fw / 2) + 64.0 * fh * fw; op.hbm_elems_out = 64.0 * fh * fw;
        op.launch = [p](hipStream_t s, int n) { Conv3Params<T> q = p; q.n = n; launch_conv3x3<T>(s, &q, 1); };
        L.ops.push_back(op);
    }
    // SSH context modules: each of the three merged convs is ONE launch covering strides 32, 16 and 8
    Conv3Params<T> lv_a[3], lv_b[3], lv_c[3];
    OpInfo op_a, op_b, op_c, op_h;
    // fp16 / int8: conv_b and conv_c of the context module are ONE launch (ssh_tail_kernel); context_conv3_1 stays in LDS
    constexpr bool fuse_tail = sizeof(T) <= 2;
    SshTailParams<T> tl[3];
    HeadParams<T> hl[3];
    int anchor_off = 0;
    for (int i = 0; i < 3; i++) {
        const SshModule &m = plan.ssh[i];
        int fh = H / kStrides[i], fw = W / kStrides[i];
        std::string pre = "rf_c" + std::to_string(3 - i) + "_det_";
        T *cat = act(pre + "concat_relu", fh, fw, 64);
        T *ctx1 = act(pre + "context_conv1_relu", fh, fw, 16);
        T *ctx31 = fuse_tail ? nullptr : act(pre + "context_conv3_1_relu", fh, fw, 16);
        auto fill = [&](Conv3Params<T> &p, OpInfo &op, const FoldedConv &f, const GemmW &gw, const T *in, int cin, T *o0,
                        int ld0, int off0, int n0, T *o1, int ld1, int off1, int nlayers) {
            p.in = in; p.in_ld = cin; p.in_off = 0; p.up = nullptr;
            p.w = A.ptr<T>(gw.w); p.b = A.ptr<float>(gw.b); p.m = wp.mult_ptr(gw);
            p.out0 = o0; p.ld0 = ld0; p.off0 = off0; p.n0 = n0; p.out1 = o1; p.ld1 = ld1; p.off1 = off1;
            p.n = 0; p.h = fh; p.w_ = fw; p.cin = cin; p.cout = f.cout;
            op.name += (op.name.empty() ? "" : " | ") + f.name;
            op.alg_elems_in += (double)nlayers * cin * fh * fw;   // each merged sibling reads the input once, layer-wise
            op.alg_elems_out += (double)f.cout * fh * fw;
            op.hbm_elems_in += (double)cin * fh * fw;              // merged siblings share ONE read of the input
            op.hbm_elems_out += (double)f.cout * fh * fw;
            op.macs += f.macs_per_out_pixel() * fh * fw;
        };
        fill(lv_a[i], op_a, m.conv_a, wp.ssh_w_[i][0], feat[i], 64, cat, 64, 0, 32, ctx1, 16, 0, 2);
        fill(lv_b[i], op_b, m.conv_b, wp.ssh_w_[i][1], ctx1, 16, cat, 64, 32, 16, ctx31, 16, 0, 2);
        fill(lv_c[i], op_c, m.conv_c, wp.ssh_w_[i][2], ctx31, 16, cat, 64, 48, 16, nullptr, 0, 0, 1);
        if constexpr (fuse_tail) {
            SshTailParams<T> &tp = tl[i];
            tp.in = ctx1; tp.cat = cat; tp.n = 0; tp.h = fh; tp.w_ = fw;
            tp.wb = A.ptr<T>(wp.ssh_w_[i][1].w); tp.bb = A.ptr<float>(wp.ssh_w_[i][1].b); tp.mb = wp.mult_ptr(wp.ssh_w_[i][1]);
            tp.wc = A.ptr<T>(wp.ssh_w_[i][2].w); tp.bc = A.ptr<float>(wp.ssh_w_[i][2].b); tp.mc = wp.mult_ptr(wp.ssh_w_[i][2]);
        }
        HeadParams<T> &hp = hl[i];
        hp.in = cat; hp.w = A.ptr<T>(wp.ssh_w_[i][3].w); hp.b = A.ptr<float>(wp.ssh_w_[i][3].b);
        hp.m = wp.mult_ptr(wp.ssh_w_[i][3]);
        hp.n = 0; hp.h = fh; hp.w_ = fw; hp.stride = kStrides[i]; hp.anchor_offset = anchor_off;
        hp.num_anchors = site.num_anchors;
        memset(hp.base, 0, sizeof(hp.base));
        preset_base_anchors(*site.ratios, i, hp.base);
        hp.net_h = H; hp.net_w = W; hp.params = site.d_params;
        hp.cand = site.d_cand; hp.cand_count = site.d_cand_count; hp.cap = site.max_candidates;
        hp.dump_prob = hp.dump_bbox = hp.dump_lmk = nullptr;
        if (site.keep_outputs) {
            const int chans[3] = {2 * wp.head_a_, 4 * wp.head_a_, 10 * wp.head_a_};
            for (int k = 0; k < 3; k++) L.d_dump[i][k] = (float *)site.dalloc((size_t)mb * chans[k] * fh * fw * sizeof(float));
            hp.dump_prob = L.d_dump[i][0]; hp.dump_bbox = L.d_dump[i][1]; hp.dump_lmk = L.d_dump[i][2];
        }
        op_h.name += (op_h.name.empty() ? "" : " | ") + m.head.name;
        op_h.alg_elems_in += 3.0 * 64 * fh * fw;
        op_h.alg_elems_out += 16.0 * wp.head_a_ * fh * fw;
        op_h.hbm_elems_in += 64.0 * fh * fw;                       // the concat tensor in; candidates out: a few KB
        op_h.macs += m.head.macs_per_out_pixel() * fh * fw;
        anchor_off += site.num_anchors * fh * fw;
    }
    op_a.launch = with_n3(lv_a, launch_conv3x3<T>);
    op_a.kernel = "conv3x3<64,48,8x8>";
    op_b.kernel = "conv3x3<16,32,8x8>";
    op_c.kernel = "conv3x3<16,16,8x8>";
    op_h.kernel = "head";
    L.ops.push_back(op_a);
    if constexpr (fuse_tail) {
        OpInfo op_t;
        op_t.name = op_b.name + " | " + op_c.name;
        op_t.kernel = "ssh_tail<16,32,16>";
        op_t.alg_elems_in = op_b.alg_elems_in + op_c.alg_elems_in;       // layer-wise accounting, fused or not
        op_t.alg_elems_out = op_b.alg_elems_out + op_c.alg_elems_out;
        op_t.macs = op_b.macs + op_c.macs;
        op_t.hbm_elems_in = op_b.hbm_elems_in;                 // context_conv1 in; context_conv3_1 stays in LDS
        op_t.hbm_elems_out = op_b.hbm_elems_out + op_c.hbm_elems_out - op_c.hbm_elems_in;      // concat[32:64]: 16 + 16 channels
        op_t.launch = with_n3(tl, launch_ssh_tail<T>);
        L.ops.push_back(op_t);
    } else {
        op_b.launch = with_n3(lv_b, launch_conv3x3<T>);
        op_c.launch = with_n3(lv_c, launch_conv3x3<T>);
        L.ops.push_back(op_b);
        L.ops.push_back(op_c);
    }
    L.first_post = L.ops.size();
    op_h.name += " +softmax+decode";
    op_h.launch = with_n3(hl, launch_head<T>);
    L.ops.push_back(op_h);
    {
        NmsParams np;
        np.cand = site.d_cand; np.cand_count = site.d_cand_count; np.cap = site.max_candidates; np.params = site.d_params;
        np.out = site.h_out; np.out_count = site.h_counts; np.out_cand_count = site.h_counts + mb;
        np.max_det = site.max_detections; np.n = 0;
        OpInfo op;
        op.name = "sort+nms";
        op.kernel = "nms";
        op.launch = with_n(np, launch_nms);
        L.ops.push_back(op);
    }
}

template void build_net<float>(const Plan &, const WeightPack<float> &, const NetSite &, LaneNet *);
template void build_net<half_t>(const Plan &, const WeightPack<half_t> &, const NetSite &, LaneNet *);
template void build_net<int8_t>(const Plan &, const WeightPack<int8_t> &, const NetSite &, LaneNet *);

}  // namespace rf
