// eval.hip -- the evaluation epoch for gfx950 (epnet_amd/eval_epoch.py): the KITTI result records of a batch and, below them,
// its recall counts.
//
// ---- KITTI result records: save_kitti_format (tools/eval_rcnn.py:76-101) without the host -------------------------------------
// The reference copies the detections of a scene to the host, builds the eight corners of every box with a batched
// numpy matmul (kitti_utils.boxes3d_to_corners3d :66-103), projects them (Calibration.corners3d_to_img_boxes,
// calibration.py:106-124), clips and filters the image boxes and prints one text line per box with %.4f, which the AP evaluator
// parses again. Here one workgroup per scene does the same arithmetic per lane, compacts the valid rows in index order (wave
// ballot + prefix, as roipool3d.hip and proposal_bin_kernel) and writes the 13 numbers of each line as the doubles the text
// would parse to (r4.h). The contract is spelled out in include/epnet_ops.h.
#include <math.h>

#include "boxgeom.h"
#include "common.h"
#include "cr_trig.h"
#include "dpp.h"
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
            float c, s;
            cr_cossinf(ry, c, s);
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
            const float beta = cr_atan2f(z, x);  // :95-96
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

// ---- evaluation recall (tools/eval_rcnn.py:598-632) ---------------------------------------------------------------------------
// The reference walks the scenes on the host: it trims the padded ground truth, calls boxes_iou3d_gpu for the refined boxes and
// for the ROIs, and reads `(gt_max_iou > thresh).sum().item()` ten times and the segmentation IoU once -- about a dozen syncs
// per scene. Here: (1) one workgroup per (scene, box set, ground-truth row) puts its lanes over the boxes, every IoU is
// iou3d_pair -- bit for bit epnet_boxes_iou3d's -- and the column maximum is folded across the wave on the vector ALU (dpp.h)
// and across the waves through LDS; (2) the segmentation counts are a grid-stride integer reduction into one partial per
// workgroup; (3) one workgroup per scene counts the thresholds, folds the rows for pred_max_iou and adds the epoch totals
// (integer atomics: the order does not matter), and workgroup 0 adds the segmentation partials. The cost is the latency of one
// rotated-box IoU per lane, not bytes. No value leaves the device.
constexpr int kEvalMaxM = 4096;
constexpr int kEvalMaxT = 8;
constexpr int kEvalSegBlocks = 256;  // most workgroups of the segmentation reduction (the partials' room in the workspace)

struct EvalThresholds {
    float v[kEvalMaxT];
};

// float <-> int, order preserving (its own inverse), every NaN on top: the maximum over these keys is the maximum that
// propagates a NaN, as torch.max does. -0.0 ranks below +0.0.
__device__ __forceinline__ int max_key(float v) {
    if (v != v) return 0x7fffffff;
    const int s = __float_as_int(v);
    return s >= 0 ? s : s ^ 0x7fffffff;
}
__device__ __forceinline__ float max_key_value(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ __launch_bounds__(256) void eval_iou_kernel(int m, int g, int gc, const float *__restrict__ pred,
                                                       const float *__restrict__ roi, const float *__restrict__ gt,
                                                       float *__restrict__ gt_max, float *__restrict__ mat) {
    __shared__ int s_red[4];
    __shared__ int s_key[4];
    const int j = blockIdx.x, set = blockIdx.y, scene = blockIdx.z;
    gt += (size_t)scene * g * gc;
    const float *boxes = (set == 0 ? pred : roi) + (size_t)scene * m * 7;
    const int num_gt = count_gt_rows(g, gc, gt, s_red);
    int key = (int)0x80000000;  // below every key
    if (j < num_gt) {  // uniform over the workgroup
        float b7[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) b7[q] = gt[(size_t)j * gc + q];
        for (int i = threadIdx.x; i < m; i += 256) {
            float a7[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) a7[q] = boxes[(size_t)i * 7 + q];
            const float v = iou3d_pair(a7, b7);
            key = max(key, max_key(v));
            if (mat && set == 0) mat[((size_t)scene * g + j) * m + i] = v;
        }
    }
    key = wave_max_all(key);  // all 64 lanes active
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int k = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
        gt_max[((size_t)scene * 2 + set) * g + j] = j < num_gt ? max_key_value(k) : 0.f;
    }
}

// one partial [correct, fg, pos] per workgroup (a few hundred KB of int32 per batch: plain coalesced loads)
__global__ __launch_bounds__(256) void eval_seg_kernel(long long total, const int *__restrict__ seg, const int *__restrict__ label,
                                                       long long *__restrict__ partial) {
    __shared__ long long s_sum[4][3];
    long long c = 0, f = 0, p = 0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int s = seg[e], l = label[e];
        c += (l > 0 && s == l) ? 1 : 0;
        f += l > 0 ? 1 : 0;
        p += s > 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c += __shfl_xor(c, off, 64);
        f += __shfl_xor(f, off, 64);
        p += __shfl_xor(p, off, 64);
    }
    if (lane_id() == 0) {
        s_sum[threadIdx.x >> 6][0] = c;
        s_sum[threadIdx.x >> 6][1] = f;
        s_sum[threadIdx.x >> 6][2] = p;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        partial[(size_t)blockIdx.x * 3 + threadIdx.x] = s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x] + s_sum[2][threadIdx.x] + s_sum[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void eval_finish_kernel(int m, int g, int gc, int nt, EvalThresholds thr, int have_roi,
                                                          const float *__restrict__ gt, const float *__restrict__ gt_max,
                                                          const float *__restrict__ mat, const long long *__restrict__ seg_partial,
                                                          int seg_blocks, int *__restrict__ scene_stats,
                                                          long long *__restrict__ seg_counts, unsigned long long *__restrict__ totals,
                                                          float *__restrict__ gt_max_pred, float *__restrict__ gt_max_roi,
                                                          float *__restrict__ pred_max_iou) {
    __shared__ int s_red[4];
    __shared__ int s_cnt[2][kEvalMaxT];
    const int scene = blockIdx.x;
    const int num_gt = count_gt_rows(g, gc, gt + (size_t)scene * g * gc, s_red);
    if (threadIdx.x < 2 * kEvalMaxT) s_cnt[threadIdx.x / kEvalMaxT][threadIdx.x % kEvalMaxT] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < g; j += 256) {
        const float vp = j < num_gt ? gt_max[((size_t)scene * 2 + 0) * g + j] : 0.f;
        const float vr = (have_roi && j < num_gt) ? gt_max[((size_t)scene * 2 + 1) * g + j] : 0.f;
        if (gt_max_pred) gt_max_pred[(size_t)scene * g + j] = vp;
        if (gt_max_roi) gt_max_roi[(size_t)scene * g + j] = vr;
        if (j < num_gt) {
            for (int t = 0; t < nt; ++t) {  // strict, fp32; a NaN maximum is above no threshold (:615, :625)
                if (vp > thr.v[t]) atomicAdd(&s_cnt[0][t], 1);
                if (have_roi && vr > thr.v[t]) atomicAdd(&s_cnt[1][t], 1);
            }
        }
    }
    __syncthreads();
    const int cols = 1 + 2 * nt;
    if ((int)threadIdx.x < cols) {
        const int t = threadIdx.x;
        const int v = t == 0 ? num_gt : (t <= nt ? s_cnt[0][t - 1] : s_cnt[1][t - 1 - nt]);
        scene_stats[(size_t)scene * cols + t] = v;
        if (totals && v != 0) atomicAdd(&totals[t], (unsigned long long)v);
    }
    if (pred_max_iou) {
        for (int i = threadIdx.x; i < m; i += 256) {
            int key = (int)0x80000000;
            for (int j = 0; j < num_gt; ++j) key = max(key, max_key(mat[((size_t)scene * g + j) * m + i]));
            pred_max_iou[(size_t)scene * m + i] = num_gt > 0 ? max_key_value(key) : 0.f;
        }
    }
    if (scene == 0 && seg_counts && threadIdx.x < 3) {
        long long sum = 0;
        for (int w = 0; w < seg_blocks; ++w) sum += seg_partial[(size_t)w * 3 + threadIdx.x];
        seg_counts[threadIdx.x] = sum;
    }
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

namespace {
struct EvalPlan {
    size_t off_seg, off_gt_max, off_mat, bytes;
};

EvalPlan eval_plan(int b, int m, int g) {
    EvalPlan p;
    const size_t sb = (size_t)b, sm = (size_t)m, sg = (size_t)g;
    Carver c;
    p.off_seg = c.take((size_t)kEvalSegBlocks * 3 * sizeof(long long));
    p.off_gt_max = c.take(sb * 2 * sg * sizeof(float));
    p.off_mat = c.take(sb * sg * sm * sizeof(float));
    p.bytes = c.off;
    return p;
}
}  // namespace

extern "C" size_t epnet_eval_recall_workspace_bytes(int b, int m, int g) {
    if (b <= 0 || b > 65535 || m < 1 || m > kEvalMaxM || g < 0) return 0;
    return eval_plan(b, m, g).bytes;
}

extern "C" int epnet_eval_recall(int b, int m, int g, int gc, int n, int nt, const float *thresholds, const float *pred_boxes3d,
                                 const float *roi_boxes3d, const float *gt_boxes3d, const int *seg_result, const int *rpn_cls_label,
                                 void *workspace, size_t workspace_bytes, int *scene_stats, int64_t *seg_counts, int64_t *totals,
                                 float *gt_max_pred, float *gt_max_roi, float *pred_max_iou, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && m >= 0 && n >= 0 && nt >= 0);
    if (b == 0) return EPNET_OK;
    if (m < 1 || m > kEvalMaxM || g < 0 || b > 65535 || nt > kEvalMaxT) return EPNET_ELIMIT;
    EPNET_REQUIRE(gc >= 7 && gc <= 16);
    EPNET_REQUIRE(pred_boxes3d && (gt_boxes3d || g == 0) && (thresholds || nt == 0) && workspace && scene_stats);
    if (seg_counts) {
        EPNET_REQUIRE(n == 0 || (seg_result && rpn_cls_label));
    } else {
        EPNET_REQUIRE(!seg_result && !rpn_cls_label);
    }
    const EvalPlan p = eval_plan(b, m, g);
    if (workspace_bytes < p.bytes) return EPNET_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    long long *seg_partial = (long long *)(ws + p.off_seg);
    float *gt_max = (float *)(ws + p.off_gt_max);
    float *mat = (float *)(ws + p.off_mat);
    EvalThresholds thr;
    for (int t = 0; t < kEvalMaxT; ++t) thr.v[t] = t < nt ? thresholds[t] : 0.f;
    int rc;
    if (g > 0) {
        hipLaunchKernelGGL(eval_iou_kernel, dim3(g, roi_boxes3d ? 2 : 1, b), dim3(256), 0, s, m, g, gc, pred_boxes3d, roi_boxes3d,
                           gt_boxes3d, gt_max, pred_max_iou ? mat : (float *)nullptr);
        rc = check_launch("eval_recall iou");
        if (rc) return rc;
    }
    int seg_blocks = 0;
    const long long total = (long long)b * n;
    if (seg_counts && total > 0) {
        seg_blocks = (int)(div_up64(total, 256 * 8) < kEvalSegBlocks ? div_up64(total, 256 * 8) : kEvalSegBlocks);
        hipLaunchKernelGGL(eval_seg_kernel, dim3(seg_blocks), dim3(256), 0, s, total, seg_result, rpn_cls_label, seg_partial);
        rc = check_launch("eval_recall seg");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(b), dim3(256), 0, s, m, g, gc, nt, thr, roi_boxes3d ? 1 : 0, gt_boxes3d,
                       (const float *)gt_max, (const float *)mat, (const long long *)seg_partial, seg_blocks, scene_stats,
                       (long long *)seg_counts, (unsigned long long *)totals, gt_max_pred, gt_max_roi, pred_max_iou);
    return check_launch("eval_recall finish");
}
