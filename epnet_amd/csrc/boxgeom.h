// boxgeom.h -- the pair geometry of rotated boxes that more than one feature needs (lib/utils/iou3d/src/iou3d_kernel.cu,
// iou3d_utils.py:21-53): BEV overlap / IoU, the fused 3-D IoU, the rotated NMS's per-box record, the ground-truth row count.
// box_overlap evaluates each polygon vertex's atan2 once and bubble-sorts on the stored angles (the reference recomputes two
// atan2 per comparison, :104-106, :188-196): the same deterministic function of the same arguments, hence the same swaps.
#pragma once
#include <math.h>

#include "common.h"
#include "cr_trig.h"

namespace epnet {

constexpr float kIouEps = 1e-8f;  // iou3d_kernel.cu:13

struct P2 {
    float x, y;
};

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {  // :38-40
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool rect_cross(P2 p1, P2 p2, P2 q1, P2 q2) {  // :42-48
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// check_in_box2d (:50-65) with the box's cos(-ry), sin(-ry) passed in
__device__ __forceinline__ bool in_box2d(const float *box, float ncos, float nsin, P2 p) {
    const float MARGIN = 1e-5f;
    const float center_x = (box[0] + box[2]) / 2;
    const float center_y = (box[1] + box[3]) / 2;
    const float rot_x = (p.x - center_x) * ncos + (p.y - center_y) * nsin + center_x;
    const float rot_y = -(p.x - center_x) * nsin + (p.y - center_y) * ncos + center_y;
    return rot_x > box[0] - MARGIN && rot_x < box[2] + MARGIN && rot_y > box[1] - MARGIN && rot_y < box[3] + MARGIN;
}

__device__ __forceinline__ bool seg_intersection(P2 p1, P2 p0, P2 q1, P2 q0, P2 &ans) {  // :67-96
    if (!rect_cross(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kIouEps) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__device__ __forceinline__ void rot_center(P2 center, float c, float s, P2 &p) {  // :98-102
    const float nx = (p.x - center.x) * c + (p.y - center.y) * s + center.x;
    const float ny = -(p.x - center.x) * s + (p.y - center.y) * c + center.y;
    p.x = nx;
    p.y = ny;
}

// per-box trigonometry: cos/sin of +ry (corner rotation) and of -ry (point-in-box test)
struct BoxTrig {
    float c, s, nc, ns;
};

__device__ __forceinline__ BoxTrig box_trig(float ry) {
    BoxTrig t;
    t.c = cr_cosf(ry);
    t.s = cr_sinf(ry);
    t.nc = cr_cosf(-ry);
    t.ns = cr_sinf(-ry);
    return t;
}

__device__ inline float box_overlap(const float *box_a, const float *box_b, BoxTrig ta, BoxTrig tb) {  // :108-212
    const float a_x1 = box_a[0], a_y1 = box_a[1], a_x2 = box_a[2], a_y2 = box_a[3];
    const float b_x1 = box_b[0], b_y1 = box_b[1], b_x2 = box_b[2], b_y2 = box_b[3];
    const P2 center_a = {(a_x1 + a_x2) / 2, (a_y1 + a_y2) / 2};
    const P2 center_b = {(b_x1 + b_x2) / 2, (b_y1 + b_y2) / 2};
    P2 ac[5] = {{a_x1, a_y1}, {a_x2, a_y1}, {a_x2, a_y2}, {a_x1, a_y2}, {0.f, 0.f}};
    P2 bc[5] = {{b_x1, b_y1}, {b_x2, b_y1}, {b_x2, b_y2}, {b_x1, b_y2}, {0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rot_center(center_a, ta.c, ta.s, ac[k]);
        rot_center(center_b, tb.c, tb.s, bc[k]);
    }
    ac[4] = ac[0];
    bc[4] = bc[0];

    P2 cp[24];  // the reference has 16 slots; two rectangles cannot produce more than 16 entries
    float ang[24];
    P2 pc = {0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            P2 r;
            if (seg_intersection(ac[i + 1], ac[i], bc[j + 1], bc[j], r)) {
                pc.x = pc.x + r.x;
                pc.y = pc.y + r.y;
                cp[cnt++] = r;
            }
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(box_a, ta.nc, ta.ns, bc[k])) {
            pc.x = pc.x + bc[k].x;
            pc.y = pc.y + bc[k].y;
            cp[cnt++] = bc[k];
        }
        if (in_box2d(box_b, tb.nc, tb.ns, ac[k])) {
            pc.x = pc.x + ac[k].x;
            pc.y = pc.y + ac[k].y;
            cp[cnt++] = ac[k];
        }
    }
    pc.x /= cnt;
    pc.y /= cnt;

    for (int i = 0; i < cnt; ++i) ang[i] = cr_atan2f(cp[i].y - pc.y, cp[i].x - pc.x);
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i)
            if (ang[i] > ang[i + 1]) {
                const P2 tp = cp[i];
                cp[i] = cp[i + 1];
                cp[i + 1] = tp;
                const float ta_ = ang[i];
                ang[i] = ang[i + 1];
                ang[i + 1] = ta_;
            }

    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k) {
        const float ax = cp[k].x - cp[0].x, ay = cp[k].y - cp[0].y;
        const float bx = cp[k + 1].x - cp[0].x, by = cp[k + 1].y - cp[0].y;
        area += ax * by - ay * bx;
    }
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const float *box_a, const float *box_b, BoxTrig ta, BoxTrig tb) {  // :214-221
    const float sa = (box_a[2] - box_a[0]) * (box_a[3] - box_a[1]);
    const float sb = (box_b[2] - box_b[0]) * (box_b[3] - box_b[1]);
    const float s_overlap = box_overlap(box_a, box_b, ta, tb);
    return s_overlap / fmaxf(sa + sb - s_overlap, kIouEps);
}

__device__ __forceinline__ float iou_normal(const float *a, const float *b) {  // :295-303
    const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
    const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
    const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
    const float interS = width * height;
    const float Sa = (a[2] - a[0]) * (a[3] - a[1]);
    const float Sb = (b[2] - b[0]) * (b[3] - b[1]);
    return interS / fmaxf(Sa + Sb - interS, kIouEps);
}

// ---- fused 3-D IoU (boxes_iou3d_gpu of lib/utils/iou3d/iou3d_utils.py:21-53 in ONE launch) -------------
// The reference builds the BEV boxes (kitti_utils.boxes3d_to_bev_torch :137-150), calls the overlap kernel and
// finishes with ~10 small torch kernels (height overlap, volumes, clamp, divide). Every step is an fp32
// elementwise op, reproduced here in the same order, so the values equal that composition.
// boxes: (.,7) [x, y, z, h, w, l, ry], y = bottom centre, camera coordinates.
__device__ __forceinline__ void bev_of(const float *b7, float *bev) {
    const float half_l = b7[5] / 2, half_w = b7[4] / 2;
    bev[0] = b7[0] - half_l;
    bev[1] = b7[2] - half_w;
    bev[2] = b7[0] + half_l;
    bev[3] = b7[2] + half_w;
    bev[4] = b7[6];
}

__device__ __forceinline__ float iou3d_pair(const float *a7, const float *b7) {
    float ba[5], bb[5];
    bev_of(a7, ba);
    bev_of(b7, bb);
    const float overlaps_bev = box_overlap(ba, bb, box_trig(ba[4]), box_trig(bb[4]));
    const float a_min = a7[1] - a7[3], a_max = a7[1], b_min = b7[1] - b7[3], b_max = b7[1];
    const float max_of_min = fmaxf(a_min, b_min), min_of_max = fminf(a_max, b_max);
    const float overlaps_h = fmaxf(min_of_max - max_of_min, 0.f);
    const float overlaps_3d = overlaps_bev * overlaps_h;
    const float vol_a = a7[3] * a7[4] * a7[5], vol_b = b7[3] * b7[4] * b7[5];
    return overlaps_3d / fmaxf(vol_a + vol_b - overlaps_3d, 1e-7f);
}

// The per-box record of the rotated NMS (box_rot_kernel, iou3d.hip), part of every NMS caller's workspace. Everything of a
// pair's overlap that depends on ONE box is computed once per box: the rotated corners (same expressions as box_overlap),
// their axis-aligned hull, cos / sin of -ry for the point-in-box test, the box area.
struct BoxRot {
    float x1, y1, x2, y2;      // the BEV box itself
    float nc, ns;              // cos(-ry), sin(-ry): check_in_box2d (:50-65)
    float cx[4], cy[4];        // corners after rotate_around_center (:98-102, :141-146)
    float minx, maxx, miny, maxy;
    float area, pad;
};
static_assert(sizeof(BoxRot) == 80, "BoxRot layout");

// 1 + the last row whose fp32 sum over all gc columns (ascending) is not 0; 0 without such a row. Every thread of the
// workgroup gets the result; s_red holds one int per wave.
__device__ __forceinline__ int count_gt_rows(int g, int gc, const float *__restrict__ gt, int *s_red) {
    int last = 0;
    for (int r = threadIdx.x; r < g; r += blockDim.x) {
        float sum = 0.f;
        for (int c = 0; c < gc; ++c) sum = sum + gt[(size_t)r * gc + c];
        if (sum != 0.f) last = r + 1;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = last;
    __syncthreads();
    int res = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) res = max(res, s_red[w]);
    __syncthreads();
    return res;
}

}  // namespace epnet
