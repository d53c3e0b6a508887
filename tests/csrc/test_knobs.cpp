// Host unit test of the RF_* knob table (retinaface_amd/csrc/knobs.cpp), compiled by tests/test_host.py.  The environment is set by the
// test; this program prints what knob() returns.
#include <cstdio>

#include "../../retinaface_amd/csrc/knobs.cpp"

int main() {
    using namespace rf;
    printf("RF_SYNC_PIECES %d\n", knob(K_SYNC_PIECES));
    printf("RF_SYNC_SPLIT %d\n", knob(K_SYNC_SPLIT));
    printf("RF_FORCE_SCATTER %d\n", knob(K_FORCE_SCATTER));
    printf("RF_PREBUILD_LANES %d\n", knob(K_PREBUILD_LANES));
    printf("RF_BLEND_FP32 %d\n", knob(K_BLEND_FP32));
    for (int k = 0; k < K_COUNT; k++)
        if (!knob_name((Knob)k) || knob_name((Knob)k)[0] != 'R') { printf("table row %d has no name\n", k); return 1; }
    return 0;
}
