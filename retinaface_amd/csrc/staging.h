// staging.h -- host-only address arithmetic of the engine's frame uploads: which frames of a chunk travel as one copy, and how a
// synchronous host-frame call is cut into pipelined pieces.  (Header-only and HIP-free so tests/csrc/test_staging.cpp
// exercises exactly the code the engine runs.)  A chunk is frames[] / rows[] / cols[] / steps[] as the caller passed them, empty[]
// (img.empty()) and off[], each staged frame's byte offset in the lane's staging block.
#pragma once
#include <vector>

#include "copier.h"

namespace rf {

// Frames [i, end) travel as one copy of `bytes` bytes.
struct FrameRun { int end; size_t bytes; };

// The run that starts at the non-empty frame i of a chunk of n: frame i's span, plus every following frame as long as the frames
// have dense rows, come from the same source (same_source(i, j): the peer path's "resident on the same device") and follow each
// other in source memory AND in the staging block.  per_frame (RF_SCATTER_PER_FRAME): runs of one frame.
template <typename Same>
FrameRun frame_run(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, const char *empty, const size_t *off,
                   int i, int n, bool per_frame, Same same_source) {
    size_t run = (size_t)(rows[i] - 1) * steps[i] + (size_t)cols[i] * 3;
    int j = i + 1;
    if (!per_frame && steps[i] == cols[i] * 3)
        while (j < n && !empty[j] && same_source(i, j) && steps[j] == cols[j] * 3 && frames[j] == frames[i] + run && off[j] == off[i] + run)
            run += (size_t)rows[j] * cols[j] * 3, j++;
    return FrameRun{j, run};
}

// One piece of a pipelined upload: the rows to stage into the pinned block at hbase, then bytes [sent, end) of the block to send.
struct StagePiece { std::vector<ParallelCopier::Job> jobs; size_t sent, end; };

// Piece boundaries are byte positions of the staging block (stage_need bytes) cut at row granularity: a piece is whole frames
// and / or a row range of a frame, so ONE large frame (1280 x 896 = 3.4 MB) is pipelined as well.  A piece that gets no rows
// (its goal was reached by the row the piece before rounded up to) has no jobs and sent == end.
inline std::vector<StagePiece> stage_piece_plan(const uint8_t *const *frames, const int *rows, const int *cols, const int *steps, const char *empty,
                                                const size_t *off, int n, size_t stage_need, int pieces, uint8_t *hbase) {
    std::vector<StagePiece> plan(pieces);
    size_t sent = 0;
    int i = 0, r = 0;                          // next frame / next row of it to stage
    for (int pc = 0; pc < pieces; pc++) {
        const size_t goal = pc == pieces - 1 ? stage_need : stage_need * (pc + 1) / pieces;
        size_t end = sent;
        while (i < n && end < goal) {
            if (empty[i]) { i++; r = 0; continue; }
            const size_t rb = (size_t)cols[i] * 3, at = off[i] + (size_t)r * rb;
            int take = rows[i] - r;
            if (at + (size_t)take * rb > goal) take = (int)std::max<size_t>(1, (goal - std::min(goal, at) + rb - 1) / rb);
            take = std::min(take, rows[i] - r);
            plan[pc].jobs.push_back(ParallelCopier::Job{hbase + at, frames[i] + (size_t)r * steps[i], rb, (size_t)take, (size_t)steps[i]});
            end = at + (size_t)take * rb;
            r += take;
            if (r == rows[i]) { i++; r = 0; }
        }
        plan[pc].sent = sent;
        plan[pc].end = end;
        sent = end;
    }
    return plan;
}

}  // namespace rf
