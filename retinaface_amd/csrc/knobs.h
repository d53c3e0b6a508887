// knobs.h -- every RF_* environment knob of the library in ONE table (round 5; ADVICE r4: the knobs were ~30 function-local statics,
// each parsed where it was used, unknown values fell through to some variant silently).
//
// The semantic knobs change what the library does for a caller: RF_BLEND_FP32, RF_FORCE_SCATTER, RF_SCATTER_PER_FRAME,
// RF_SYNC_SPLIT, RF_PREBUILD_LANES, RF_HOST_TRACE.  They are looked up on every query (engines read them when they are built;
// tests toggle them between engines of one process).  RF_SYNC_PIECES is a measurement knob with a range: read once per process
// (std::call_once), an invalid value is reported on stderr and replaced by the default.
#pragma once

namespace rf {

enum Knob {
    K_BLEND_FP32,          // RF_BLEND_FP32: int8 aggregation convs blend in fp32 instead of packed integers (bit-identical; test knob)
    K_FORCE_SCATTER,       // RF_FORCE_SCATTER: treat every device frame as resident on another GPU (peer-copy path on a one-GPU box)
    K_SCATTER_PER_FRAME,   // RF_SCATTER_PER_FRAME: one peer copy per foreign frame (rounds 3-5) instead of one per contiguous run of frames (the split A/B of bench.py)
    K_SYNC_SPLIT,          // RF_SYNC_SPLIT=0: a synchronous host-frame call stages + uploads its frames in ONE piece (rounds 1-5) instead of pipelined pieces
    K_PREBUILD_LANES,      // RF_PREBUILD_LANES: build every lane at rf_create instead of on first use
    K_HOST_TRACE,          // RF_HOST_TRACE: per-stage host wall clock of the calls, printed when the engine is destroyed
    K_SYNC_PIECES,         // RF_SYNC_PIECES=1..64: most pieces a synchronous host-frame call is staged + sent in (default 4)
    K_COUNT
};

int knob(Knob k);
const char *knob_name(Knob k);

}  // namespace rf
