// targets.hip -- the RPN training targets of a whole batch in one launch (include/epnet_ops.h, epnet_rpn_targets) for gfx950.
//
// The reference makes them in the loader, per scene, on a host core (lib/datasets/kitti_rcnn_dataset.py): data_augmentation
// (:698-755) rotates, scales and flips the cloud and its ground-truth boxes, generate_rpn_training_labels (:547-576) then runs
// two scipy Delaunay point-in-hull tests per box over all points. Here a workgroup of 256 threads takes 1024 consecutive points
// of one scene, four consecutive points per thread:
//
//   1. wave 0 derives the scene's augmented boxes, 64 at a time, into an LDS table of 64 bytes per box -- centre, cos / sin of
//      the heading, the half extents of the box and of the enlarged box, the four label values -- which every lane then reads
//      at the same address (broadcast); the workgroup with the scene's first points also writes gt_out. Meanwhile all waves
//      stage the tile's points into LDS with 16-byte coalesced loads (clamped index, no load under a condition);
//   2. every thread takes its four points out of LDS, augments them, puts them back, and the tile goes out to pts_out with
//      16-byte non-temporal stores that cover contiguous bytes per wave;
//   3. the box loop in ascending k, as the reference's loop: the class is decided by the last box whose enlarged form holds
//      the point, the regression row by the last box that holds it, independently;
//   4. the 28-byte regression rows are staged through the same LDS buffer and streamed out 16 bytes per lane, contiguous per
//      wave; the four class labels of a thread are one 16-byte store.
// No atomics, no scratch memory, no synchronisation with the host: the bits depend on the inputs alone.
//
// Arithmetic. The rotation is evaluated in double from the fp32 coordinates and the angle and rounded once, as
// rotate_pc_along_y's float64 np.dot does; everything else is fp32 in source order without contraction; cos / sin / atan2 are the
// parity definition's correctly rounded ones (via double). The membership test is pt_in_box3d's (roipool3d.hip) about the
// centre (x, y - h/2, z), with enlarge_box3d's extents (h, w, l + 2e about the same centre) for the ignore margin.
#include <math.h>

#include "common.h"
#include "cr_trig.h"

namespace epnet {
namespace targets {

constexpr int kThreads = 256;
constexpr int kPer = 4;                       // consecutive points per thread
constexpr int kTile = kThreads * kPer;        // points per workgroup
constexpr int kBoxChunk = 64;                 // boxes in the LDS table at a time (one per lane of wave 0)

typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

struct Aug {
    bool rot, flip;
    double c, s;      // of the scene's angle
    float scale;
};

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : v); }   // np.sign: 0 and NaN stay

// one ground-truth row through data_augmentation (stage 1), in its order: rotation, scaling, flip
__device__ __forceinline__ void augment_box(const Aug &a, float alpha, float g[7]) {
    constexpr float kPi = (float)M_PI;
    if (a.rot) {
        const double xd = (double)g[0], zd = (double)g[2];
        g[0] = (float)(xd * a.c - zd * a.s);
        g[2] = (float)(xd * a.s + zd * a.c);
        const float beta = cr_atan2f(g[2], g[0]);
        g[6] = ((sign_of(beta) * kPi) / 2.f + alpha) - beta;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = g[k] * a.scale;
    if (a.flip) {
        g[0] = -g[0];
        g[6] = sign_of(g[6]) * kPi - g[6];
    }
}

__device__ __forceinline__ void augment_point(const Aug &a, float &x, float &y, float &z) {
    if (a.rot) {
        const double xd = (double)x, zd = (double)z;
        x = (float)(xd * a.c - zd * a.s);
        z = (float)(xd * a.s + zd * a.c);
    }
    x = x * a.scale; y = y * a.scale; z = z * a.scale;
    if (a.flip) x = -x;
}

// grid (ceil(n / kTile), b); VEC: n % 4 == 0 and every pointer 16-byte aligned, so every tile of every scene is too
template <bool VEC>
__global__ __launch_bounds__(kThreads) void rpn_targets_kernel(int n, int g, float extra, const float *__restrict__ pts,
                                                               const float *__restrict__ gt, const float *__restrict__ gt_alpha,
                                                               const float *__restrict__ aug, float *__restrict__ pts_out,
                                                               float *__restrict__ gt_out, int *__restrict__ cls_label,
                                                               float *__restrict__ reg_label) {
    __shared__ f4 s_buf[kTile * 7 / 4];          // the tile's points (3 floats each), later its regression rows (7 floats each)
    __shared__ f4 s_box[kBoxChunk * 4];          // [cx cy cz -] [cos sin hl hh] [hw el eh ew] [h w l ry]
    __shared__ double s_cs[2];
    int wg_x, bs;
    xcd_scene_map(wg_x, bs);   // a scene's boxes pass through one XCD's L2
    const int t = threadIdx.x;
    const int tile0 = wg_x * kTile;
    const int np = n - tile0 < kTile ? n - tile0 : kTile;          // points of this tile
    const size_t p0 = (size_t)bs * (size_t)n + (size_t)tile0;      // first point, batch-wide
    float *s_f = reinterpret_cast<float *>(s_buf);

    // ---- the scene's draws (uniform over the workgroup)
    Aug a;
    a.rot = false; a.flip = false; a.c = 1.0; a.s = 0.0; a.scale = 1.f;
    float angle = 0.f;
    if (aug) {
        const float *row = aug + (size_t)bs * 4;
        a.rot = row[0] != 0.f; angle = row[1]; a.scale = row[2]; a.flip = row[3] != 0.f;
    }
    if (t < 64 && a.rot) {
        const double c = cos((double)angle), s = sin((double)angle);
        if (t == 0) { s_cs[0] = c; s_cs[1] = s; }
        a.c = c; a.s = s;                          // wave 0 needs them before the barrier
    }

    // ---- stage the tile's points: 3 * np floats from pts + 3 * p0
    {
        const float *src = pts + p0 * 3;
        if (VEC) {
            const int n4 = np * 3 / 4;             // np % 4 == 0
            const f4 *src4 = reinterpret_cast<const f4 *>(src);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = t + j * kThreads;
                s_buf[i] = src4[i < n4 ? i : n4 - 1];
            }
        } else {
            for (int i = t; i < np * 3; i += kThreads) s_f[i] = src[i];
        }
    }

    const float extra2 = 2.0f * extra;             // == (float)(2 * extra_width): a doubling is exact
    // derives boxes k0 .. k0 + 63 of the scene into the table (wave 0, lane = box)
    auto derive = [&](int k0) {
        const int k = k0 + t, kk = k < g ? k : g - 1;
        const float *row = gt + ((size_t)bs * g + kk) * 7;
        float b[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) b[c] = row[c];
        const float alpha = gt_alpha ? gt_alpha[(size_t)bs * g + kk] : 0.f;     // only the rotation reads it
        augment_box(a, alpha, b);
        if (gt_out && wg_x == 0 && k < g) {
            float *o = gt_out + ((size_t)bs * g + k) * 7;
#pragma unroll
            for (int c = 0; c < 7; ++c) o[c] = b[c];
        }
        const bool real = k < g && b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;   // a degenerate hull labels nothing
        const float cy = b[1] - b[3] / 2.f;
        float cosa, sina;
        cr_cossinf(b[6], cosa, sina);
        const float hh = b[3] * 0.5f, hw = b[4] * 0.5f, hl = b[5] * 0.5f;
        const float eh = (b[3] + extra2) * 0.5f, ew = (b[4] + extra2) * 0.5f, el = (b[5] + extra2) * 0.5f;
        // a negative extent fails every |.| <= test
        s_box[t * 4 + 0] = f4{b[0], cy, b[2], 0.f};
        s_box[t * 4 + 1] = f4{cosa, sina, real ? hl : -1.f, real ? hh : -1.f};
        s_box[t * 4 + 2] = f4{real ? hw : -1.f, real ? el : -1.f, real ? eh : -1.f, real ? ew : -1.f};
        s_box[t * 4 + 3] = f4{b[3], b[4], b[5], b[6]};
    };
    if (t < 64 && g > 0) derive(0);
    __syncthreads();
    if (a.rot) { a.c = s_cs[0]; a.s = s_cs[1]; }

    // ---- this thread's four points: out of LDS, augmented, back
    float px[kPer], py[kPer], pz[kPer];
    {
        const f4 v0 = s_buf[t * 3], v1 = s_buf[t * 3 + 1], v2 = s_buf[t * 3 + 2];
        px[0] = v0.x; py[0] = v0.y; pz[0] = v0.z; px[1] = v0.w; py[1] = v1.x; pz[1] = v1.y;
        px[2] = v1.z; py[2] = v1.w; pz[2] = v2.x; px[3] = v2.y; py[3] = v2.z; pz[3] = v2.w;
    }
    if (aug) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) augment_point(a, px[j], py[j], pz[j]);
    }
    if (pts_out) {
        s_buf[t * 3] = f4{px[0], py[0], pz[0], px[1]};
        s_buf[t * 3 + 1] = f4{py[1], pz[1], px[2], py[2]};
        s_buf[t * 3 + 2] = f4{pz[2], px[3], py[3], pz[3]};
        __syncthreads();
        float *dst = pts_out + p0 * 3;
        if (VEC) {
            const int n4 = np * 3 / 4;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = t + j * kThreads;
                if (i < n4) __builtin_nontemporal_store(s_buf[i], reinterpret_cast<f4 *>(dst) + i);
            }
        } else {
            for (int i = t; i < np * 3; i += kThreads) dst[i] = s_f[i];
        }
    }

    // ---- the boxes in ascending k: the last one decides
    int cls[kPer];
    float reg[kPer][7];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        cls[j] = 0;
#pragma unroll
        for (int c = 0; c < 7; ++c) reg[j][c] = 0.f;
    }
    for (int k0 = 0; k0 < g; k0 += kBoxChunk) {
        if (k0 > 0) {
            __syncthreads();                       // the previous chunk has been read by everyone
            if (t < 64) derive(k0);
            __syncthreads();
        }
        const int cnt = g - k0 < kBoxChunk ? g - k0 : kBoxChunk;
        for (int k = 0; k < cnt; ++k) {
            const f4 b0 = s_box[k * 4], b1 = s_box[k * 4 + 1], b2 = s_box[k * 4 + 2], b3 = s_box[k * 4 + 3];
            const float nsina = -b1.y;
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const float dx = px[j] - b0.x, dy = py[j] - b0.y, dz = pz[j] - b0.z;
                const float lx = dx * b1.x + dz * nsina;
                const float lz = dx * b1.y + dz * b1.x;
                const float ax = fabsf(lx), ay = fabsf(dy), az = fabsf(lz);
                const bool in_e = (ax <= b2.y) & (ay <= b2.z) & (az <= b2.w);
                const bool in_b = (ax <= b1.z) & (ay <= b1.w) & (az <= b2.x);
                cls[j] = in_e ? (in_b ? 1 : -1) : cls[j];
                reg[j][0] = in_b ? b0.x - px[j] : reg[j][0];     // centre - point as written: -(p - c) would give -0 at the centre
                reg[j][1] = in_b ? b0.y - py[j] : reg[j][1];
                reg[j][2] = in_b ? b0.z - pz[j] : reg[j][2];
                reg[j][3] = in_b ? b3.x : reg[j][3];
                reg[j][4] = in_b ? b3.y : reg[j][4];
                reg[j][5] = in_b ? b3.z : reg[j][5];
                reg[j][6] = in_b ? b3.w : reg[j][6];
            }
        }
    }

    // ---- class labels: one 16-byte store per thread
    {
        int *dst = cls_label + p0;
        if (VEC) {
            if (t * kPer < np) __builtin_nontemporal_store(i4{cls[0], cls[1], cls[2], cls[3]}, reinterpret_cast<i4 *>(dst) + t);
        } else {
#pragma unroll
            for (int j = 0; j < kPer; ++j)
                if (t * kPer + j < np) dst[t * kPer + j] = cls[j];
        }
    }

    // ---- regression rows through LDS: 28 consecutive floats per thread in, 16 contiguous bytes per lane out
    __syncthreads();                               // pts_out has left the buffer
    {
        const float *r = &reg[0][0];
#pragma unroll
        for (int q = 0; q < 7; ++q) s_buf[t * 7 + q] = f4{r[q * 4], r[q * 4 + 1], r[q * 4 + 2], r[q * 4 + 3]};
    }
    __syncthreads();
    {
        float *dst = reg_label + p0 * 7;
        if (VEC) {
            const int n4 = np * 7 / 4;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int i = t + j * kThreads;
                if (i < n4) __builtin_nontemporal_store(s_buf[i], reinterpret_cast<f4 *>(dst) + i);
            }
        } else {
            for (int i = t; i < np * 7; i += kThreads) dst[i] = s_f[i];
        }
    }
}

}  // namespace targets
}  // namespace epnet

using namespace epnet;

extern "C" int epnet_rpn_targets(int b, int n, int g, float extra_width, const float *pts, const float *gt_boxes3d,
                                 const float *gt_alpha, const float *aug, float *pts_out, float *gt_out, int *cls_label,
                                 float *reg_label, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && n >= 0 && g >= 0 && extra_width >= 0.f);
    if (b == 0 || n == 0) return EPNET_OK;
    const long long tiles = div_up64(n, targets::kTile);
    if (b > 65535 || tiles * b > 0x7fffffffll) return EPNET_ELIMIT;
    EPNET_REQUIRE(pts && cls_label && reg_label);
    EPNET_REQUIRE(g == 0 || (gt_boxes3d && (gt_alpha || !aug)));
    EPNET_REQUIRE(aug == nullptr || (pts_out && (g == 0 || gt_out)));
    EPNET_REQUIRE(pts_out != pts && (gt_out == nullptr || gt_out != gt_boxes3d));
    const bool vec = n % 4 == 0 && (((uintptr_t)pts | (uintptr_t)pts_out | (uintptr_t)cls_label | (uintptr_t)reg_label) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)b), block(targets::kThreads);
    if (vec)
        hipLaunchKernelGGL(targets::rpn_targets_kernel<true>, grid, block, 0, st, n, g, extra_width, pts, gt_boxes3d, gt_alpha, aug,
                           pts_out, gt_out, cls_label, reg_label);
    else
        hipLaunchKernelGGL(targets::rpn_targets_kernel<false>, grid, block, 0, st, n, g, extra_width, pts, gt_boxes3d, gt_alpha, aug,
                           pts_out, gt_out, cls_label, reg_label);
    return check_launch("rpn_targets");
}
