// net.h -- the only part of a lane that depends on the element type: Plan + WeightPack<T> -> the lane's launch list and the
// activation buffers behind it (net.cpp).  Streams, tables, staging, graphs and the scheduler are engine.cpp's and know no T.
#pragma once
#include "engine.h"
#include "weights.h"

namespace rf {

constexpr int kStrides[3] = {32, 16, 8};      // FPN levels 0 / 1 / 2

// what build_net fills in a lane
struct LaneNet {
    std::map<std::string, ActInfo> acts;
    std::vector<OpInfo> ops;              // launch order
    size_t first_post = 0;                // index of the first post-processing launch (heads)
    float *d_dump[3][3] = {};
};

// what the lane code allocated before the net is built, and the engine settings its launches carry
struct NetSite {
    int mb, net_h, net_w;                 // images per launch (max_batch * coalesce), network input size
    const FrameDesc *frames;              // the half of the lane's device frame table the stem reads
    RunParams *d_params;
    Candidate *d_cand, *h_out;
    int *d_cand_count, *h_counts;
    int max_candidates, max_detections, num_anchors;
    bool keep_outputs;
    const std::vector<float> *ratios;
    std::function<void *(size_t bytes)> dalloc;      // the lane's device allocator (the lane frees what it hands out)
};

template <typename T> void build_net(const Plan &plan, const WeightPack<T> &wp, const NetSite &site, LaneNet *net);

}  // namespace rf
