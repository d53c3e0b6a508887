// rot.h -- rotation-robust detection: the quarter-turn rotations of a frame, the mapping of a rotated pass back into the frame, shared
// by the kernels (kernels.hip rotate_frames_kernel / rot_gather_kernel) and the host entry points rf_rot_map_face / rf_rot_merge_host /
// rf_rotate_host (capi.cpp).  Pass k (k = 0..3) of a rows x cols frame F is np.rot90(F, k), k quarter turns counter-clockwise:
//      k = 0: F itself
//      k = 1: D is cols x rows, D[y][x] = F[x][cols - 1 - y]
//      k = 2: D is rows x cols, D[y][x] = F[rows - 1 - y][cols - 1 - x]
//      k = 3: D is cols x rows, D[y][x] = F[rows - 1 - x][y]
// The faces of pass k are moved back with one fp32 multiply by the PASS's frame scale per coordinate and one fp32 subtract where a
// coordinate flips; the landmarks keep their index (a rotation keeps handedness).  The merge is the flip-TTA merge (tta.h), with
// g = k * max_detections + j (DESIGN.md "Rotation-robust detection").  Every step is a single fp32 operation, never contracted, so
// host and device agree bit for bit with each other and with tests/rot_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "tile.h"
#include "tta.h"

namespace rf {

static_assert(sizeof(rf_rot_spec) == 16, "rf_rot_spec is 16 bytes");

// a validated rf_rot_spec with its defaults applied
struct RotSpec {
    int rots = 15, vote = 0, max_faces = 0;
    int passes() const { return __builtin_popcount((unsigned)rots); }
};

// One pass of a call as the gather kernel sees it: rotation k of frame `frame`, a rows x cols SOURCE frame, whose results are
// multiplied by `scale` (rf_frame_scale of the pass's own shape: cols x rows for odd k).  frame < 0: nothing to gather.
struct RotEntry {
    int32_t frame, rows, cols, k;
    float scale;
};

// Host: check a caller's spec and apply its defaults; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *rot_spec_resolve(const rf_rot_spec *in, int default_max_faces, RotSpec *out) {
    RotSpec r;
    r.max_faces = default_max_faces;
    if (in) {
        if (in->struct_size != sizeof(rf_rot_spec)) return "rf_rot_spec.struct_size mismatch";
        if (in->rots < 0 || in->rots > 15) return "rots must be in [0, 15]";
        if (in->vote < 0 || in->vote > 2) return "vote must be 0, 1 or 2";
        if (in->max_faces < 0 || in->max_faces > kTtaMaxFaces) return "max_faces must be 0 or in [1, 4096]";
        r.rots = in->rots ? in->rots : 15;
        r.vote = in->vote == 1;
        if (in->max_faces) r.max_faces = in->max_faces;
    }
    if (r.max_faces < 1 || r.max_faces > kTtaMaxFaces) return "max_faces must be in [1, 4096]";
    *out = r;
    return nullptr;
}

// the shape of pass k of a rows x cols frame
__host__ __device__ inline int rot_rows(int k, int rows, int cols) { return (k & 1) ? cols : rows; }
__host__ __device__ inline int rot_cols(int k, int rows, int cols) { return (k & 1) ? rows : cols; }

// The pixel index rule, both ways: where pixel (sy, sx) of the rows x cols source lands in pass k, and which source pixel
// pixel (dy, dx) of pass k shows.
__host__ __device__ inline void rot_dst_of_src(int k, int rows, int cols, int sy, int sx, int *dy, int *dx) {
    switch (k & 3) {
    case 0: *dy = sy; *dx = sx; break;
    case 1: *dy = cols - 1 - sx; *dx = sy; break;
    case 2: *dy = rows - 1 - sy; *dx = cols - 1 - sx; break;
    default: *dy = sx; *dx = rows - 1 - sy; break;
    }
}
__host__ __device__ inline void rot_src_of_dst(int k, int rows, int cols, int dy, int dx, int *sy, int *sx) {
    switch (k & 3) {
    case 0: *sy = dy; *sx = dx; break;
    case 1: *sy = dx; *sx = cols - 1 - dy; break;
    case 2: *sy = rows - 1 - dy; *sx = cols - 1 - dx; break;
    default: *sy = rows - 1 - dx; *sx = dy; break;
    }
}

// Host: pass k of the rows x cols BGR frame src (row pitch step), written as rot_cols * 3 bytes per row at dst + y * dst_step; bytes
// beyond a row are untouched.  k = 0 is a row copy.
inline void rot_rotate_host(const uint8_t *src, int rows, int cols, int step, int k, uint8_t *dst, int dst_step) {
    const int dr = rot_rows(k, rows, cols), dc = rot_cols(k, rows, cols);
    for (int y = 0; y < dr; y++) {
        uint8_t *d = dst + (size_t)y * dst_step;
        if ((k & 3) == 0) {
            memcpy(d, src + (size_t)y * step, (size_t)dc * 3);
            continue;
        }
        for (int x = 0; x < dc; x++) {
            int sy, sx;
            rot_src_of_dst(k, rows, cols, y, x, &sy, &sx);
            const uint8_t *s = src + (size_t)sy * step + (size_t)sx * 3;
            d[3 * x] = s[0]; d[3 * x + 1] = s[1]; d[3 * x + 2] = s[2];
        }
    }
}

// The mapping of one face of a pass.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]: the head of rf_face and of
// Candidate), they may alias.  One multiply by the scale per coordinate (also when it is 1); then, with c = (float)(cols - 1) and
// r = (float)(rows - 1) of the source frame, a point (x', y') of the pass is
//      k = 1: (c - y', x')      k = 2: (c - x', r - y')      k = 3: (y', r - x')
// in the frame -- one subtract where a coordinate flips; the box corners change places so that x1 <= x2, y1 <= y2 stay.
__host__ __device__ inline void rot_map_face(const RotEntry &e, const float *in, float *out) {
#pragma clang fp contract(off)
    float f[15], o[15];
    f[0] = in[0];
    for (int i = 1; i < 15; i++) f[i] = in[i] * e.scale;
    for (int i = 0; i < 15; i++) o[i] = f[i];
    const float c = (float)(e.cols - 1), r = (float)(e.rows - 1);
    if (e.k == 1) {
        o[1] = c - f[4]; o[3] = c - f[2]; o[2] = f[1]; o[4] = f[3];
        for (int i = 0; i < 5; i++) { o[5 + i] = c - f[10 + i]; o[10 + i] = f[5 + i]; }
    } else if (e.k == 2) {
        o[1] = c - f[3]; o[3] = c - f[1]; o[2] = r - f[4]; o[4] = r - f[2];
        for (int i = 0; i < 5; i++) { o[5 + i] = c - f[5 + i]; o[10 + i] = r - f[10 + i]; }
    } else if (e.k == 3) {
        o[1] = f[2]; o[3] = f[4]; o[2] = r - f[3]; o[4] = r - f[1];
        for (int i = 0; i < 5; i++) { o[5 + i] = f[10 + i]; o[10 + i] = r - f[5 + i]; }
    }
    for (int i = 0; i < 15; i++) out[i] = o[i];
}

}  // namespace rf
