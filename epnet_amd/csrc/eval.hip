// eval.hip -- the KITTI result records of an evaluation batch for gfx950: save_kitti_format (tools/eval_rcnn.py:76-101) without
// the host. The reference copies the detections of a scene to the host, builds the eight corners of every box with a batched
// numpy matmul (kitti_utils.boxes3d_to_corners3d :66-103), projects them (Calibration.corners3d_to_img_boxes,
// calibration.py:106-124), clips and filters the image boxes and prints one text line per box with %.4f, which the AP evaluator
// parses again. Here one workgroup per scene does the same arithmetic per lane, compacts the valid rows in index order (wave
// ballot + prefix, as roipool3d.hip and proposal_bin_kernel) and writes the 13 numbers of each line as the doubles the text
// would parse to (r4.h). The contract is spelled out in include/epnet_ops.h.
#include <math.h>

#include "common.h"
#include "r4.h"

namespace epnet {

constexpr int kRecThreads = 256;
constexpr int kRecMaxM = 4096;
constexpr int kRecCols = 13;

__device__ __forceinline__ float rec_sign(float v) { return v > 0.f ? 1.0f : v < 0.f ? -1.0f : 0.0f; }

// np.clip: minimum(maximum(v, lo), hi), a NaN stays
__device__ __forceinline__ float rec_clip(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(kRecThreads) void kitti_records_kernel(int m, const float *__restrict__ boxes3d,
                                                                    const float *__restrict__ scores,
                                                                    const int *__restrict__ count, const float *__restrict__ P2,
                                                                    const int *__restrict__ img_shape,
                                                                    double *__restrict__ records, int *__restrict__ rec_count,
                                                                    float *__restrict__ bbox_raw, int *__restrict__ valid) {
    __shared__ int wave_cnt[kRecThreads / 64];
    __shared__ int base;
    const int scene = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    boxes3d += (size_t)scene * m * 7;
    scores += (size_t)scene * m;
    records += (size_t)scene * m * kRecCols;
    const int n_box = count ? min(max(count[scene], 0), m) : m;
    float P[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) P[r][q] = P2[(size_t)scene * 12 + r * 4 + q];
    const int img_h = img_shape[scene * 2], img_w = img_shape[scene * 2 + 1];
    const float x_hi = (float)(img_w - 1), y_hi = (float)(img_h - 1);
    const float w_bound = (float)((double)img_w * 0.8), h_bound = (float)((double)img_h * 0.8);  // img_shape[1] * 0.8 (:87)
    const float kPi = 3.14159265358979323846f;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < m; start += kRecThreads) {  // every wave runs every round (ballots over whole waves)
        const int i = start + threadIdx.x;
        bool ok = false;
        float box[4] = {0.f, 0.f, 0.f, 0.f};
        float b7[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float alpha = 0.f, score = 0.f;
        if (i < n_box) {
#pragma unroll
            for (int q = 0; q < 7; ++q) b7[q] = boxes3d[(size_t)i * 7 + q];
            score = scores[i];
            const float x = b7[0], y = b7[1], z = b7[2], h = b7[3], w = b7[4], l = b7[5], ry = b7[6];
            const float c = (float)cos((double)ry), s = (float)sin((double)ry);
            const float hl = l / 2.0f, hw = w / 2.0f;
            const float xc[8] = {hl, hl, -hl, -hl, hl, hl, -hl, -hl};
            const float zc[8] = {hw, -hw, -hw, hw, hw, -hw, -hw, hw};
            float u_lo = 0.f, u_hi = 0.f, v_lo = 0.f, v_hi = 0.f;
            bool u_nan = false, v_nan = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float yc = k < 4 ? 0.f : -h;
                const float X = x + (xc[k] * c + zc[k] * s);
                const float Y = y + yc;
                const float Z = z + (xc[k] * (-s) + zc[k] * c);
                float p[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) p[r] = ((X * P[r][0] + Y * P[r][1]) + Z * P[r][2]) + P[r][3];
                const float u = p[0] / p[2], v = p[1] / p[2];
                u_nan = u_nan || u != u;
                v_nan = v_nan || v != v;
                u_lo = k == 0 ? u : fminf(u_lo, u);
                u_hi = k == 0 ? u : fmaxf(u_hi, u);
                v_lo = k == 0 ? v : fminf(v_lo, v);
                v_hi = k == 0 ? v : fmaxf(v_hi, v);
            }
            const float kNan = __int_as_float(0x7fc00000);
            if (u_nan) u_lo = u_hi = kNan;  // np.min / np.max (calibration.py:118-119)
            if (v_nan) v_lo = v_hi = kNan;
            box[0] = rec_clip(u_lo, 0.f, x_hi);  // :80-83
            box[1] = rec_clip(v_lo, 0.f, y_hi);
            box[2] = rec_clip(u_hi, 0.f, x_hi);
            box[3] = rec_clip(v_hi, 0.f, y_hi);
            ok = (box[2] - box[0]) < w_bound && (box[3] - box[1]) < h_bound;  // :85-87; false with a NaN
            const float beta = (float)atan2((double)z, (double)x);  // :95-96
            alpha = ((-rec_sign(beta) * kPi) / 2.0f + beta) + ry;
        }
        if (i < m) {
            if (bbox_raw) {
#pragma unroll
                for (int q = 0; q < 4; ++q) bbox_raw[((size_t)scene * m + i) * 4 + q] = box[q];
            }
            if (valid) valid[(size_t)scene * m + i] = ok ? 1 : 0;
        }
        const unsigned long long mask = __ballot(ok);
        if (lane == 0) wave_cnt[wave] = (int)__popcll(mask);
        __syncthreads();
        if (ok) {
            int pos = base + popc_below(mask);
            for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
            double *row = records + (size_t)pos * kRecCols;  // pos <= i < m
            row[0] = r4(alpha);
#pragma unroll
            for (int q = 0; q < 4; ++q) row[1 + q] = r4(box[q]);
            row[5] = r4(b7[3]);
            row[6] = r4(b7[4]);
            row[7] = r4(b7[5]);
            row[8] = r4(b7[0]);
            row[9] = r4(b7[1]);
            row[10] = r4(b7[2]);
            row[11] = r4(b7[6]);
            row[12] = r4(score);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < kRecThreads / 64; ++w) t += wave_cnt[w];
            base += t;
        }
        __syncthreads();
    }
    const int total = base;
    if (threadIdx.x == 0) rec_count[scene] = total;
    for (long long e = (long long)total * kRecCols + threadIdx.x; e < (long long)m * kRecCols; e += kRecThreads) records[e] = 0.0;
}

}  // namespace epnet

using namespace epnet;

extern "C" int epnet_kitti_records(int b, int m, const float *boxes3d, const float *scores, const int *count, const float *P2,
                                   const int *img_shape, double *records, int *rec_count, float *bbox_raw, int *valid,
                                   epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && m >= 0);
    if (b == 0) return EPNET_OK;
    if (m < 1 || m > kRecMaxM || b > 65535) return EPNET_ELIMIT;
    EPNET_REQUIRE(boxes3d && scores && P2 && img_shape && records && rec_count);
    hipLaunchKernelGGL(kitti_records_kernel, dim3(b), dim3(kRecThreads), 0, (hipStream_t)stream, m, boxes3d, scores, count, P2,
                       img_shape, records, rec_count, bbox_raw, valid);
    return check_launch("kitti_records");
}
