// knobs.cpp -- see knobs.h.
#include "knobs.h"

#include <cstdio>
#include <cstdlib>
#include <mutex>

namespace rf {

namespace {

constexpr int kPresence = -0x7ffffffe;     // the knob is "set or not": any value (even empty) counts as 1

struct Spec {
    const char *name;
    bool semantic;          // looked up on every query; otherwise parsed and range-checked once per process
    int def;
    int lo, hi;             // range of a knob that is not semantic; {kPresence, 0} = presence knob
};

// One row per knob, in the order of enum Knob.
const Spec kSpecs[K_COUNT] = {
    {"RF_BLEND_FP32", true, 0, kPresence, 0},
    {"RF_FORCE_SCATTER", true, 0, kPresence, 0},
    {"RF_SCATTER_PER_FRAME", true, 0, kPresence, 0},
    {"RF_SYNC_SPLIT", true, 1, 0, 1},
    {"RF_PREBUILD_LANES", true, 0, 0, 1},
    {"RF_HOST_TRACE", true, 0, kPresence, 0},
    {"RF_SYNC_PIECES", false, 4, 1, 64},
};

int g_value[K_COUNT];
std::once_flag g_once;

void parse_all() {
    for (int k = 0; k < K_COUNT; k++) {
        const Spec &s = kSpecs[k];
        g_value[k] = s.def;
        const char *e = getenv(s.name);
        if (!e || s.semantic) continue;
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end != '\0' || v < s.lo || v > s.hi) {
            fprintf(stderr, "[retinaface_amd] %s=%s is not a value this knob knows: using the default %d\n", s.name, e, s.def);
            continue;
        }
        g_value[k] = (int)v;
    }
}

}  // namespace

int knob(Knob k) {
    if (kSpecs[k].semantic) {
        const char *e = getenv(kSpecs[k].name);
        if (!e) return kSpecs[k].def;
        if (kSpecs[k].lo == kPresence) return 1;
        return atoi(e) != 0 ? 1 : 0;
    }
    std::call_once(g_once, parse_all);
    return g_value[k];
}
const char *knob_name(Knob k) { return kSpecs[k].name; }

}  // namespace rf
