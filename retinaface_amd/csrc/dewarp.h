// dewarp.h -- fisheye detection: the dewarped views of a frame and the mapping of a view's faces back into the frame, shared by the
// kernels (kernels.hip dewarp_views_kernel / pass_gather_kernel<DewarpMap>) and the host entry points rf_dewarp_host /
// rf_dewarp_map_face / rf_dewarp_merge_host / rf_dewarp_plan (capi.cpp).  A dewarper holds V views of view_w x view_h pixels (both
// multiples of 16).  Each view has a MESH of (view_h / 16 + 1) x (view_w / 16 + 1) nodes: node (i, j) is the source position of view
// pixel (16 i, 16 j) as two int32, x then y, in 1/256 px, |value| <= 2^22; view-major, then row-major nodes.  The device only ever
// sees meshes: the trigonometry of the lens (dewarp_plan) stays on the host.  Between the nodes a pixel's source position is the
// bilinear blend of its cell's four nodes, in exact integers, and the pixel is the bilinear blend of four source taps with 5-bit
// weights; a face is moved back through the same mesh with 12-bit weights (DESIGN.md "Fisheye detection").  Integers everywhere,
// and where a float is touched a single uncontracted fp32 operation, so host and device agree bit for bit with each other and with
// tests/dewarp_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/retinaface_amd.h"
#include "tile.h"
#include "tta.h"

namespace rf {

static_assert(sizeof(rf_dewarp_spec) == 584, "rf_dewarp_spec is 584 bytes");

constexpr int kDewarpMaxViews = RF_DEWARP_MAX_VIEWS;
constexpr int kDewarpNodeMax = 1 << 22;         // |node| bound, 1/256 px: 16384 px
constexpr int kDewarpMaxW = 4096, kDewarpMaxH = 3072;

// the call-level part of a validated rf_dewarp_spec with its defaults applied
struct DewarpSpec {
    int vote = 0, max_faces = 0, edge = 0;
};

// One pass of a call as the gather kernel sees it: view `view` of frame `frame`, a rows x cols SOURCE frame, whose results are
// multiplied by `scale` (rf_frame_scale of the view's shape) and moved through `mesh`, the VIEW's nodes (device memory for the
// kernels, host memory for the host entry points).  frame < 0: nothing to gather.
struct DewarpEntry {
    int32_t frame, view, rows, cols, view_w, view_h;
    float scale;
    int32_t pad_;
    const int32_t *mesh;
};

__host__ __device__ inline int dewarp_nodes_x(int view_w) { return (view_w >> 4) + 1; }
__host__ __device__ inline int dewarp_nodes_y(int view_h) { return (view_h >> 4) + 1; }
inline size_t dewarp_view_ints(int view_w, int view_h) { return (size_t)dewarp_nodes_x(view_w) * dewarp_nodes_y(view_h) * 2; }

// Host: the call-level fields of a caller's spec; nullptr = all defaults.  Returns nullptr, or what is wrong with it.
inline const char *dewarp_spec_resolve(const rf_dewarp_spec *in, int default_max_faces, DewarpSpec *out) {
    DewarpSpec r;
    r.max_faces = default_max_faces;
    if (in) {
        if (in->struct_size != sizeof(rf_dewarp_spec)) return "rf_dewarp_spec.struct_size mismatch";
        if (in->vote < 0 || in->vote > 2) return "vote must be 0, 1 or 2";
        if (in->max_faces < 0 || in->max_faces > kTtaMaxFaces) return "max_faces must be 0 or in [1, 4096]";
        if (in->edge < 0 || in->edge > 1024) return "edge must be in [0, 1024]";
        r.vote = in->vote == 1;
        if (in->max_faces) r.max_faces = in->max_faces;
        r.edge = in->edge;
    }
    if (r.max_faces < 1 || r.max_faces > kTtaMaxFaces) return "max_faces must be in [1, 4096]";
    *out = r;
    return nullptr;
}

// Host: the shape of a dewarper and its mesh, checked.  Returns nullptr, or what is wrong.
inline const char *dewarp_check_mesh(int view_w, int view_h, int views, const int32_t *mesh) {
    if (views < 1 || views > kDewarpMaxViews) return "views must be in [1, 16]";
    if (view_w < 16 || view_h < 16 || (view_w & 15) || (view_h & 15) || view_w > kDewarpMaxW || view_h > kDewarpMaxH)
        return "view_w / view_h must be multiples of 16, at most 4096 x 3072";
    if (!mesh) return "mesh is null";
    const size_t total = dewarp_view_ints(view_w, view_h) * (size_t)views;
    for (size_t i = 0; i < total; i++)
        if (mesh[i] > kDewarpNodeMax || mesh[i] < -kDewarpNodeMax) return "a mesh node lies beyond +-2^22 (1/256 px)";
    return nullptr;
}

// ---- the pixel rule
// The source position of view pixel (X, Y) in 1/32 px.  nodes: the view's mesh; nx: nodes per mesh row.  S is the cell's bilinear
// blend with weights (16 - u, u) x (16 - v, v): |S| <= 2^22 * 256 = 2^30.
__host__ __device__ inline void dewarp_pixel_src(const int32_t *nodes, int nx, int X, int Y, int *qx, int *qy) {
    const int cx = X >> 4, cy = Y >> 4, u = X & 15, v = Y & 15;
    const int32_t *n0 = nodes + 2 * ((size_t)cy * nx + cx), *n1 = n0 + 2 * nx;
    const int w00 = (16 - u) * (16 - v), w10 = u * (16 - v), w01 = (16 - u) * v, w11 = u * v;
    const int sx = n0[0] * w00 + n0[2] * w10 + n1[0] * w01 + n1[2] * w11;
    const int sy = n0[1] * w00 + n0[3] * w10 + n1[1] * w01 + n1[3] * w11;
    *qx = (sx + 1024) >> 11;
    *qy = (sy + 1024) >> 11;
}

// The three bytes of the pixel whose source position is (qx, qy), 1/32 px: four taps with weights (32 - w, w) per axis, a tap outside
// the rows x cols source reads as 0, (sum + 512) >> 10 per channel.
__host__ __device__ inline void dewarp_sample(const uint8_t *src, int rows, int cols, int step, int qx, int qy, uint8_t *bgr) {
    const int x0 = qx >> 5, y0 = qy >> 5, wx = qx & 31, wy = qy & 31;
    const int w00 = (32 - wx) * (32 - wy), w10 = wx * (32 - wy), w01 = (32 - wx) * wy, w11 = wx * wy;
    if (x0 >= 0 && y0 >= 0 && x0 + 1 < cols && y0 + 1 < rows) {
        const uint8_t *p0 = src + (size_t)y0 * step + (size_t)3 * x0, *p1 = p0 + step;
        for (int c = 0; c < 3; c++) bgr[c] = (uint8_t)((p0[c] * w00 + p0[3 + c] * w10 + p1[c] * w01 + p1[3 + c] * w11 + 512) >> 10);
        return;
    }
    const bool xa = x0 >= 0 && x0 < cols, xb = x0 + 1 >= 0 && x0 + 1 < cols, ya = y0 >= 0 && y0 < rows, yb = y0 + 1 >= 0 && y0 + 1 < rows;
    if (!((xa || xb) && (ya || yb))) { bgr[0] = bgr[1] = bgr[2] = 0; return; }
    // only the taps inside are addressed
    const uint8_t *r0 = ya ? src + (size_t)y0 * step : nullptr, *r1 = yb ? src + (size_t)(y0 + 1) * step : nullptr;
    for (int c = 0; c < 3; c++) {
        const int t00 = xa && ya ? r0[3 * x0 + c] : 0, t10 = xb && ya ? r0[3 * (x0 + 1) + c] : 0;
        const int t01 = xa && yb ? r1[3 * x0 + c] : 0, t11 = xb && yb ? r1[3 * (x0 + 1) + c] : 0;
        bgr[c] = (uint8_t)((t00 * w00 + t10 * w10 + t01 * w01 + t11 * w11 + 512) >> 10);
    }
}

// Host: one view of the rows x cols BGR frame src (row pitch step), written as view_w * 3 bytes per row at dst + y * dst_step; bytes
// beyond a row are untouched.
inline void dewarp_view_host(const int32_t *nodes, int view_w, int view_h, const uint8_t *src, int rows, int cols, int step,
                             uint8_t *dst, int dst_step) {
    const int nx = dewarp_nodes_x(view_w);
    for (int y = 0; y < view_h; y++) {
        uint8_t *d = dst + (size_t)y * dst_step;
        for (int x = 0; x < view_w; x++) {
            int qx, qy;
            dewarp_pixel_src(nodes, nx, x, y, &qx, &qy);
            dewarp_sample(src, rows, cols, step, qx, qy, d + 3 * x);
        }
    }
}

// ---- the face rule
// A scaled view coordinate as an integer in 1/256 px, clamped to one cell beyond the view: [-4096, 256 dim + 4096].  The clamp is two
// compares, so that a NaN (every compare false) becomes the lower bound on the host and on the device alike.
__host__ __device__ inline int dewarp_quant(float p, int dim) {
#pragma clang fp contract(off)
    const float lo = -4096.f, hi = (float)(256 * dim + 4096);
    const float pq = p * 256.0f;
    float c = pq > lo ? pq : lo;
    c = c < hi ? c : hi;
    return (int)rintf(c);
}

// The source position, 1/256 px, of the view point (qx, qy) (dewarp_quant): the cell's bilinear blend with 12-bit weights, linearly
// extrapolated over at most one cell beyond the view.  Weights in [-4096, 8192], nodes within 2^22: |sum| < 2^50.
__host__ __device__ inline void dewarp_map_point(const DewarpEntry &e, int qx, int qy, int *rx, int *ry) {
    const int cells_x = e.view_w >> 4, cells_y = e.view_h >> 4, nx = cells_x + 1;
    int cx = qx >> 12, cy = qy >> 12;
    cx = cx < 0 ? 0 : cx > cells_x - 1 ? cells_x - 1 : cx;
    cy = cy < 0 ? 0 : cy > cells_y - 1 ? cells_y - 1 : cy;
    const long long u = qx - 4096 * cx, v = qy - 4096 * cy;
    const int32_t *n0 = e.mesh + 2 * ((size_t)cy * nx + cx), *n1 = n0 + 2 * nx;
    const long long w00 = (4096 - u) * (4096 - v), w10 = u * (4096 - v), w01 = (4096 - u) * v, w11 = u * v;
    const long long sx = n0[0] * w00 + n0[2] * w10 + n1[0] * w01 + n1[2] * w11;
    const long long sy = n0[1] * w00 + n0[3] * w10 + n1[1] * w01 + n1[3] * w11;
    *rx = (int)((sx + (1ll << 23)) >> 24);
    *ry = (int)((sy + (1ll << 23)) >> 24);
}

// Edge rule and mapping of one face of a view.  in / out: 15 floats (score, x1, y1, x2, y2, px[5], py[5]), they may alias.  One fp32
// multiply by the scale per coordinate; the edge rule on the scaled box; every landmark through dewarp_map_point; the box becomes the
// integer min / max over eight mapped points, its corners and edge midpoints (a straight edge of the view is a curve in the frame).
// Returns false for a face the edge rule drops (out is then not written).
__host__ __device__ inline bool dewarp_map_face(const DewarpEntry &e, int edge, const float *in, float *out) {
#pragma clang fp contract(off)
    float f[15];
    f[0] = in[0];
    for (int i = 1; i < 15; i++) f[i] = in[i] * e.scale;
    if (edge > 0) {
        const float lo = (float)edge, hx = (float)(e.view_w - 1 - edge), hy = (float)(e.view_h - 1 - edge);
        if (f[1] < lo || f[2] < lo || f[3] > hx || f[4] > hy) return false;
    }
    const float inv = 1.f / 256.f;
    const int x1 = dewarp_quant(f[1], e.view_w), y1 = dewarp_quant(f[2], e.view_h), x2 = dewarp_quant(f[3], e.view_w), y2 = dewarp_quant(f[4], e.view_h);
    const int xm = (x1 + x2) >> 1, ym = (y1 + y2) >> 1;
    const int bx[8] = {x1, xm, x2, x1, x2, x1, xm, x2}, by[8] = {y1, y1, y1, ym, ym, y2, y2, y2};
    int lox = 0, loy = 0, hix = 0, hiy = 0;
    for (int i = 0; i < 8; i++) {
        int rx, ry;
        dewarp_map_point(e, bx[i], by[i], &rx, &ry);
        if (i == 0) { lox = hix = rx; loy = hiy = ry; }
        lox = rx < lox ? rx : lox; hix = rx > hix ? rx : hix;
        loy = ry < loy ? ry : loy; hiy = ry > hiy ? ry : hiy;
    }
    float o[15];
    o[0] = f[0];
    o[1] = (float)lox * inv; o[2] = (float)loy * inv; o[3] = (float)hix * inv; o[4] = (float)hiy * inv;
    for (int i = 0; i < 5; i++) {
        int rx, ry;
        dewarp_map_point(e, dewarp_quant(f[5 + i], e.view_w), dewarp_quant(f[10 + i], e.view_h), &rx, &ry);
        o[5 + i] = (float)rx * inv; o[10 + i] = (float)ry * inv;
    }
    for (int i = 0; i < 15; i++) out[i] = o[i];
    return true;
}

// ---- the plan (host only, doubles)
// r(theta) of the four lens models; *limit: the theta the model cannot image
inline double dewarp_radius(int model, double f, double theta) {
    switch (model) {
    case RF_LENS_EQUISOLID: return 2.0 * f * sin(theta / 2.0);
    case RF_LENS_STEREOGRAPHIC: return 2.0 * f * tan(theta / 2.0);
    case RF_LENS_ORTHOGRAPHIC: return f * sin(theta);
    default: return f * theta;
    }
}

// the views of a spec: the ring preset or the explicit list.  Returns their number, 0 for a bad spec.
inline int dewarp_spec_views(const rf_dewarp_spec &sp, rf_dewarp_view *out) {
    if (sp.ring < 0 || sp.ring > kDewarpMaxViews || sp.views < 0 || sp.views > kDewarpMaxViews) return 0;
    if ((sp.ring > 0) == (sp.views > 0)) return 0;          // one of the two
    if (sp.ring > 0) {
        for (int j = 0; j < sp.ring; j++) out[j] = rf_dewarp_view{360.0 * j / sp.ring, sp.ring_pitch, 0.0, sp.ring_hfov};
        return sp.ring;
    }
    for (int j = 0; j < sp.views; j++) out[j] = sp.view[j];
    return sp.views;
}

// The meshes of a spec's views.  mesh: views * dewarp_view_ints(view_w, view_h) ints.  Returns nullptr, or why the plan is refused.
inline const char *dewarp_plan(const rf_dewarp_spec &sp, int view_w, int view_h, int32_t *mesh, int *views_out) {
    if (sp.struct_size != sizeof(rf_dewarp_spec)) return "rf_dewarp_spec.struct_size mismatch";
    if (sp.model < RF_LENS_EQUIDISTANT || sp.model > RF_LENS_ORTHOGRAPHIC) return "unknown lens model";
    if (!(sp.f > 0.0) || !(sp.f < 1e6) || !(fabs(sp.cx) < 1e6) || !(fabs(sp.cy) < 1e6)) return "f must be positive, f / cx / cy finite";
    if (view_w < 16 || view_h < 16 || (view_w & 15) || (view_h & 15) || view_w > kDewarpMaxW || view_h > kDewarpMaxH)
        return "view_w / view_h must be multiples of 16, at most 4096 x 3072";
    rf_dewarp_view vw[kDewarpMaxViews];
    const int V = dewarp_spec_views(sp, vw);
    if (!V) return "a spec has 1..16 views or a ring of 1..16, not both";
    const double pi = 3.14159265358979323846, rad = pi / 180.0;
    const double limit = sp.model == RF_LENS_ORTHOGRAPHIC ? pi / 2.0 : pi;
    const int nx = dewarp_nodes_x(view_w), ny = dewarp_nodes_y(view_h);
    for (int k = 0; k < V; k++) {
        const rf_dewarp_view &w = vw[k];
        if (!(w.hfov > 0.0) || !(w.hfov < 180.0) || !(fabs(w.yaw) <= 3600.0) || !(fabs(w.pitch) <= 3600.0) || !(fabs(w.roll) <= 3600.0))
            return "hfov must be in (0, 180) degrees, the angles finite";
        const double fv = (view_w / 2.0) / tan(w.hfov * rad / 2.0);
        const double cy_ = cos(w.yaw * rad), sy_ = sin(w.yaw * rad), cp = cos(w.pitch * rad), sp_ = sin(w.pitch * rad),
                     cr = cos(w.roll * rad), sr = sin(w.roll * rad);
        int32_t *out = mesh + (size_t)k * nx * ny * 2;
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                const double a = (16.0 * i - (view_w - 1) / 2.0) / fv, b = (16.0 * j - (view_h - 1) / 2.0) / fv;
                // Rz(roll), then Rx(pitch), then Rz(yaw)
                const double x1 = cr * a - sr * b, y1 = sr * a + cr * b, z1 = 1.0;
                const double x2 = x1, y2 = cp * y1 - sp_ * z1, z2 = sp_ * y1 + cp * z1;
                const double dx = cy_ * x2 - sy_ * y2, dy = sy_ * x2 + cy_ * y2, dz = z2;
                const double theta = atan2(hypot(dx, dy), dz), psi = atan2(dy, dx);
                if (!(theta < limit)) return "a view reaches an angle the lens model cannot image";
                const double r = dewarp_radius(sp.model, sp.f, theta);
                const double px = 256.0 * (sp.cx + r * cos(psi)), py = 256.0 * (sp.cy + r * sin(psi));
                if (!(fabs(px) <= (double)kDewarpNodeMax) || !(fabs(py) <= (double)kDewarpNodeMax)) return "a mesh node lies beyond +-2^22 (1/256 px)";
                out[2 * ((size_t)j * nx + i)] = (int32_t)lrint(px);
                out[2 * ((size_t)j * nx + i) + 1] = (int32_t)lrint(py);
            }
    }
    if (views_out) *views_out = V;
    return nullptr;
}

}  // namespace rf
