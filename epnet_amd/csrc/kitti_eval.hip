// kitti_eval.hip -- the KITTI AP evaluator's device side for gfx950: per-frame overlap blocks, the two matching passes and the
// fixed-order reduction of the precision / recall sums.
//
// Replaces tools/kitti_object_eval_python/rotate_iou.py:18-296 (a numba.cuda kernel) and eval.py:84-332 (numba CPU JIT:
// image_box_overlap, d3_box_overlap_kernel, compute_statistics_jit, fused_compute_statistics).
//
// Differences in structure, not in results:
//   * only the per-frame diagonal blocks are computed (the reference computes part x part matrices of 50 frames and slices
//     them, eval.py:334-408); all frames are ragged, addressed through offset arrays, nothing is padded;
//   * one wave works on one (frame, combination[, threshold]); the loop over ground truths stays sequential (assigned_detection
//     carries over), the loop over detections is a wave arg-reduction (DESIGN.md "The AP evaluator" shows why it selects the
//     same detection as eval.py:197-222);
//   * the DontCare pass (eval.py:246-259) is evaluated per detection: a detection leaves the false positives when ANY DontCare
//     box covers it, which is what the two nested loops count;
//   * per-frame partial sums, then one reduction in a fixed order: no atomics, the bits depend on the inputs alone.
// The rotated intersection is the evaluator's own algorithm in float32, source order (rotate_iou.py:18-261); it is NOT
// box_overlap of boxgeom.h, which differs on identical, edge-sharing and nested boxes. Its polygon (8 points) and sort keys
// live in LDS columns, one per lane: they are indexed at run time and would otherwise go to scratch memory.
#include <math.h>

#include "common.h"
#include "cr_cos.h"
#include "cr_trig.h"

namespace epnet {

namespace {

constexpr int kMaxDt = EPNET_KITTI_MAX_DT;
constexpr int kMaxGt = EPNET_KITTI_MAX_GT;
constexpr int kMaxDc = EPNET_KITTI_MAX_DC;
constexpr int kMaxCombos = EPNET_KITTI_MAX_COMBOS;
constexpr int kMaxThresh = EPNET_KITTI_MAX_THRESHOLDS;
constexpr int kDtSlots = kMaxDt / kWave;  // detections per lane: one bit each in the lane's masks
constexpr int kOvWavesPerFrame = 4;       // waves that share one frame's overlap block
constexpr int kPolyPts = 8;               // rotate_iou.py:236: intersection_corners holds 16 floats
constexpr double kNoDetection = -10000000.0;  // eval.py:181

// rotate_iou.py:205-229
__device__ __forceinline__ void rbbox_to_corners(float *corners, const float *rbbox) {
    const float angle = rbbox[4];
    const float a_cos = cr_cosf(angle);
    const float a_sin = cr_sinf(angle);
    const float center_x = rbbox[0], center_y = rbbox[1], x_d = rbbox[2], y_d = rbbox[3];
    const float cx[4] = {-x_d / 2, -x_d / 2, x_d / 2, x_d / 2};
    const float cy[4] = {-y_d / 2, y_d / 2, y_d / 2, -y_d / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        corners[2 * i] = a_cos * cx[i] + a_sin * cy[i] + center_x;
        corners[2 * i + 1] = -a_sin * cx[i] + a_cos * cy[i] + center_y;
    }
}

// rotate_iou.py:162-178 (inclusive on every side)
__device__ __forceinline__ bool point_in_quadrilateral(float pt_x, float pt_y, const float *corners) {
    const float ab0 = corners[2] - corners[0];
    const float ab1 = corners[3] - corners[1];
    const float ad0 = corners[6] - corners[0];
    const float ad1 = corners[7] - corners[1];
    const float ap0 = pt_x - corners[0];
    const float ap1 = pt_y - corners[1];
    const float abab = ab0 * ab0 + ab1 * ab1;
    const float abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1;
    const float adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

// rotate_iou.py:74-117, edge (a, b) of one box against edge (c, d) of the other
__device__ __forceinline__ bool line_segment_intersection(float a0, float a1, float b0, float b1, float c0, float c1, float d0,
                                                          float d1, float &x, float &y) {
    const float BA0 = b0 - a0;
    const float BA1 = b1 - a1;
    const float DA0 = d0 - a0;
    const float CA0 = c0 - a0;
    const float DA1 = d1 - a1;
    const float CA1 = c1 - a1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
    if (acd != bcd) {
        const bool abc = CA1 * BA0 > BA1 * CA0;
        const bool abd = DA1 * BA0 > BA1 * DA0;
        if (abc != abd) {
            const float DC0 = d0 - c0;
            const float DC1 = d1 - c1;
            const float ABBA = a0 * b1 - b0 * a1;
            const float CDDC = c0 * d1 - d0 * c1;
            const float DH = BA1 * DC0 - BA0 * DC1;
            const float Dx = ABBA * DC0 - BA0 * CDDC;
            const float Dy = ABBA * DC1 - BA1 * CDDC;
            x = Dx / DH;
            y = Dy / DH;
            return true;
        }
    }
    return false;
}

// rotate_iou.py:232-246: area of the intersection of two rotated boxes (x, y, x_d, y_d, angle). `pts` (2 * kPolyPts floats) and
// `key` (kPolyPts floats) are this lane's LDS columns, element k at [k * kWave]. The reference's arrays have room for 8 points;
// a ninth (possible only where corners coincide) would be written past them there, here it is dropped.
__device__ float rotated_inter(const float *rbbox1, const float *rbbox2, float *pts, float *key) {
    float c1[8], c2[8];
    rbbox_to_corners(c1, rbbox1);
    rbbox_to_corners(c2, rbbox2);
    int n = 0;
    // quadrilateral_intersection, :181-202
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (point_in_quadrilateral(c1[2 * i], c1[2 * i + 1], c2) && n < kPolyPts) {
            pts[(2 * n) * kWave] = c1[2 * i];
            pts[(2 * n + 1) * kWave] = c1[2 * i + 1];
            ++n;
        }
        if (point_in_quadrilateral(c2[2 * i], c2[2 * i + 1], c1) && n < kPolyPts) {
            pts[(2 * n) * kWave] = c2[2 * i];
            pts[(2 * n + 1) * kWave] = c2[2 * i + 1];
            ++n;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x, y;
            const int i1 = (i + 1) % 4, j1 = (j + 1) % 4;
            if (line_segment_intersection(c1[2 * i], c1[2 * i + 1], c1[2 * i1], c1[2 * i1 + 1], c2[2 * j], c2[2 * j + 1], c2[2 * j1],
                                          c2[2 * j1 + 1], x, y) && n < kPolyPts) {
                pts[(2 * n) * kWave] = x;
                pts[(2 * n + 1) * kWave] = y;
                ++n;
            }
        }
    }
    // sort_vertex_in_convex_polygon, :34-71
    if (n > 0) {
        float cx = 0.0f, cy = 0.0f;
        for (int i = 0; i < n; ++i) {
            cx += pts[(2 * i) * kWave];
            cy += pts[(2 * i + 1) * kWave];
        }
        cx /= (float)n;
        cy /= (float)n;
        for (int i = 0; i < n; ++i) {
            float v0 = pts[(2 * i) * kWave] - cx;
            float v1 = pts[(2 * i + 1) * kWave] - cy;
            const float d = sqrtf(v0 * v0 + v1 * v1);
            v0 = v0 / d;
            v1 = v1 / d;
            if (v1 < 0) v0 = -2 - v0;
            key[i * kWave] = v0;
        }
        for (int i = 1; i < n; ++i) {
            if (key[(i - 1) * kWave] > key[i * kWave]) {
                const float temp = key[i * kWave];
                const float tx = pts[(2 * i) * kWave];
                const float ty = pts[(2 * i + 1) * kWave];
                int j = i;
                while (j > 0 && key[(j - 1) * kWave] > temp) {
                    key[j * kWave] = key[(j - 1) * kWave];
                    pts[(2 * j) * kWave] = pts[(2 * j - 2) * kWave];
                    pts[(2 * j + 1) * kWave] = pts[(2 * j - 1) * kWave];
                    --j;
                }
                key[j * kWave] = temp;
                pts[(2 * j) * kWave] = tx;
                pts[(2 * j + 1) * kWave] = ty;
            }
        }
    }
    // area, :24-31: a fan from point 0
    float area_val = 0.0f;
    const float a0 = pts[0], a1 = pts[kWave];
    for (int i = 0; i < n - 2; ++i) {
        const float b0 = pts[(2 * i + 2) * kWave], b1 = pts[(2 * i + 3) * kWave];
        const float q0 = pts[(2 * i + 4) * kWave], q1 = pts[(2 * i + 5) * kWave];
        area_val += fabsf(((a0 - q0) * (b1 - q1) - (a1 - q1) * (b0 - q0)) / 2.0f);
    }
    return area_val;
}

// image_box_overlap, eval.py:85-111, boxes = the row (detection) box, query = the column box
__device__ __forceinline__ double image_overlap(const double *box, const double *q, int criterion) {
    const double qbox_area = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = fmin(box[2], q[2]) - fmax(box[0], q[0]);
    if (iw > 0) {
        const double ih = fmin(box[3], q[3]) - fmax(box[1], q[1]);
        if (ih > 0) {
            double ua;
            if (criterion == -1)
                ua = (box[2] - box[0]) * (box[3] - box[1]) + qbox_area - iw * ih;
            else if (criterion == 0)
                ua = (box[2] - box[0]) * (box[3] - box[1]);
            else
                ua = qbox_area;
            return iw * ih / ua;
        }
    }
    return 0.0;
}

// one frame per blockIdx.x, kOvWavesPerFrame waves of 64 over its rows x cols pairs; rows = detections, cols = ground truths
// (eval.py:467 passes (dt_annos, gt_annos), so `boxes` are the detections and `query_boxes` the ground truths)
__global__ __launch_bounds__(kWave) void kitti_overlaps_kernel(int metric, int criterion, const int *__restrict__ row_off,
                                                               const int *__restrict__ col_off, const int64_t *__restrict__ ov_off,
                                                               const double *__restrict__ rows, const double *__restrict__ cols,
                                                               double *__restrict__ out) {
    __shared__ float s_pts[2 * kPolyPts * kWave];
    __shared__ float s_key[kPolyPts * kWave];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int r0 = row_off[f], c0 = col_off[f];
    const int nr = row_off[f + 1] - r0, nc = col_off[f + 1] - c0;
    if (nr <= 0 || nc <= 0) return;
    const int64_t base = ov_off[f];
    const int64_t room = ov_off[f + 1] - base;  // never write past the caller's own block
    const int pairs = nr * nc;
    const int width = metric == 0 ? 4 : (metric == 1 ? 5 : 7);
    for (int p = blockIdx.y * kWave + lane; p < pairs && p < room; p += kOvWavesPerFrame * kWave) {
        const int j = p / nc, i = p - j * nc;
        const double *dt = rows + (int64_t)(r0 + j) * width;
        const double *gt = cols + (int64_t)(c0 + i) * width;
        double v;
        if (metric == 0) {
            v = image_overlap(dt, gt, criterion);
        } else if (metric == 1) {
            // rotate_iou.py:293: devRotateIoUEval(qbox, box): rbox1 is the query (ground-truth) box
            float b1[5], b2[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                b1[k] = (float)gt[k];
                b2[k] = (float)dt[k];
            }
            const float area1 = b1[2] * b1[3];
            const float area2 = b2[2] * b2[3];
            const float area_inter = rotated_inter(b1, b2, s_pts + lane, s_key + lane);
            v = (double)(area_inter / (area1 + area2 - area_inter));
        } else {
            // d3_box_overlap, eval.py:120-152: criterion-2 intersection of columns [0,2,3,5,6] in float32, the rest in float64;
            // the result goes back through the float32 array `rinc` (rotate_iou.py:332 returns float32)
            const float b1[5] = {(float)gt[0], (float)gt[2], (float)gt[3], (float)gt[5], (float)gt[6]};
            const float b2[5] = {(float)dt[0], (float)dt[2], (float)dt[3], (float)dt[5], (float)dt[6]};
            const float rinc = rotated_inter(b1, b2, s_pts + lane, s_key + lane);
            v = (double)rinc;
            if (rinc > 0) {
                const double iw = fmin(dt[1], gt[1]) - fmax(dt[1] - dt[4], gt[1] - gt[4]);
                if (iw > 0) {
                    const double area1 = dt[3] * dt[4] * dt[5];
                    const double area2 = gt[3] * gt[4] * gt[5];
                    const double inc = iw * (double)rinc;
                    const double ua = area1 + area2 - inc;
                    v = (double)(float)(inc / ua);
                } else {
                    v = 0.0;
                }
            }
        }
        out[base + p] = v;
    }
}

struct Combos {
    int difficulty[kMaxCombos];
    int num_thresholds[kMaxCombos];
    double min_overlap[kMaxCombos];
};

// (value, index) maximum over the wave, the lowest index among equal values; index -1 = nothing
__device__ __forceinline__ void wave_argmax(double &v, int &idx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, kWave);
        const int oi = __shfl_xor(idx, off, kWave);
        if (oi >= 0 && (idx < 0 || ov > v || (ov == v && oi < idx))) {
            v = ov;
            idx = oi;
        }
    }
}

__device__ __forceinline__ int wave_min_index(int idx) {  // the lowest index >= 0, -1 if none
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int oi = __shfl_xor(idx, off, kWave);
        if (oi >= 0 && (idx < 0 || oi < idx)) idx = oi;
    }
    return idx;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// compute_statistics_jit (eval.py:155-272) of one frame for one (difficulty, min_overlap[, threshold]), by one wave.
// Lane l owns detections l, l + 64, ...: bit k of its masks is detection l + 64 k. kFp = the reference's compute_fp.
template <bool kFp>
__device__ void match_frame(int lane, int nd, int ng, int ndc, const double *__restrict__ ov, const double *__restrict__ score,
                            const int *__restrict__ ign_gt, const int *__restrict__ ign_dt, double min_overlap, double thresh,
                            int metric, int compute_aos, const double *__restrict__ dt_bbox, const double *__restrict__ dc_bbox,
                            const double *__restrict__ gt_alpha, const double *__restrict__ dt_alpha, double *__restrict__ matched,
                            int &tp_out, int &fp_out, int &fn_out, double &sim_out) {
    const int slots = min((nd + kWave - 1) / kWave, kDtSlots);
    unsigned usable = 0;   // ignored_det != -1 and not below the threshold
    unsigned plain = 0;    // ignored_det == 0
    unsigned assigned = 0;
    for (int k = 0; k < slots; ++k) {
        const int j = lane + k * kWave;
        if (j < nd) {
            const int ig = ign_dt[j];
            const bool below = kFp && score[j] < thresh;  // eval.py:179
            if (ig != -1 && !below) usable |= 1u << k;
            if (ig == 0) plain |= 1u << k;
        }
    }
    int tp = 0, fn = 0;
    double sim = 0.0;
    for (int i = 0; i < ng; ++i) {
        const int ig = ign_gt[i];
        if (ig == -1) {
            if (!kFp && lane == 0) matched[i] = nan("");
            continue;
        }
        double best = kNoDetection;
        int best_j = -1;
        int first_ignored = -1;
        const unsigned open = usable & ~assigned;
        for (int k = 0; k < slots; ++k) {
            if (!((open >> k) & 1u)) continue;
            const int j = lane + k * kWave;
            const double o = ov[(int64_t)j * ng + i];
            if (!(o > min_overlap)) continue;
            if (!kFp) {
                const double s = score[j];
                if (s > best) {  // strict: the lowest index among equal scores
                    best = s;
                    best_j = j;
                }
            } else if ((plain >> k) & 1u) {
                if (best_j < 0 || o > best) {  // strict: the first index of the maximum overlap
                    best = o;
                    best_j = j;
                }
            } else if (first_ignored < 0) {
                first_ignored = j;
            }
        }
        wave_argmax(best, best_j);
        int det = best_j;
        if (kFp && det < 0) det = wave_min_index(first_ignored);
        double hit = nan("");
        if (det < 0) {
            if (ig == 0) ++fn;
        } else {
            if (!(ig == 1 || ign_dt[det] == 1)) {
                ++tp;
                hit = score[det];
                if (kFp && compute_aos) sim += (1.0 + cr_cos(gt_alpha[i] - dt_alpha[det])) / 2.0;  // eval.py:264, cos as numpy rounds it
            }
            if ((det & (kWave - 1)) == lane) assigned |= 1u << (det / kWave);
        }
        if (!kFp && lane == 0) matched[i] = hit;
    }
    tp_out = tp;
    fn_out = fn;
    sim_out = sim;
    fp_out = 0;
    if (kFp) {
        // eval.py:241-259: unassigned plain detections at or above the threshold, minus those a DontCare box covers
        const unsigned cand = usable & plain & ~assigned;
        int fp = 0;
        for (int k = 0; k < slots; ++k) {
            if (!((cand >> k) & 1u)) continue;
            const int j = lane + k * kWave;
            bool stuff = false;
            if (metric == 0) {
                for (int c = 0; c < ndc && !stuff; ++c) stuff = image_overlap(dt_bbox + (int64_t)j * 4, dc_bbox + (int64_t)c * 4, 0) > min_overlap;
            }
            if (!stuff) ++fp;
        }
        fp_out = wave_sum_i32(fp);
    }
}

// pass 1: grid (frames, combos), one wave each
__global__ __launch_bounds__(kWave) void kitti_match_kernel(int total_gt, int total_dt, Combos cb, const int *__restrict__ gt_off,
                                                            const int *__restrict__ dt_off, const int64_t *__restrict__ ov_off,
                                                            const double *__restrict__ overlaps, const double *__restrict__ dt_score,
                                                            const int *__restrict__ ign_gt, const int *__restrict__ ign_dt,
                                                            double *__restrict__ matched) {
    const int f = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int g0 = gt_off[f], d0 = dt_off[f];
    const int ng = min(max(gt_off[f + 1] - g0, 0), kMaxGt), nd = min(max(dt_off[f + 1] - d0, 0), kMaxDt);
    if (ng == 0) return;
    const int diff = cb.difficulty[c];
    int tp, fp, fn;
    double sim;
    match_frame<false>(lane, nd, ng, 0, overlaps + ov_off[f], dt_score + d0, ign_gt + (int64_t)diff * total_gt + g0,
                       ign_dt + (int64_t)diff * total_dt + d0, cb.min_overlap[c], 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                       matched + (int64_t)c * total_gt + g0, tp, fp, fn, sim);
}

// pass 2: grid (frames, tstride, combos), one wave each; partial (c, t, f) = tp, fp, fn and the similarity sum of frame f
__global__ __launch_bounds__(kWave) void kitti_pr_kernel(int frames, int total_gt, int total_dt, int tstride, int metric,
                                                         int compute_aos, Combos cb, const int *__restrict__ gt_off,
                                                         const int *__restrict__ dt_off, const int *__restrict__ dc_off,
                                                         const int64_t *__restrict__ ov_off, const double *__restrict__ overlaps,
                                                         const double *__restrict__ dt_score, const int *__restrict__ ign_gt,
                                                         const int *__restrict__ ign_dt, const double *__restrict__ dt_bbox,
                                                         const double *__restrict__ dc_bbox, const double *__restrict__ gt_alpha,
                                                         const double *__restrict__ dt_alpha, const double *__restrict__ thresholds,
                                                         int *__restrict__ part_cnt, double *__restrict__ part_sim) {
    const int f = blockIdx.x, t = blockIdx.y, c = blockIdx.z, lane = threadIdx.x;
    if (t >= cb.num_thresholds[c]) return;
    const int g0 = gt_off[f], d0 = dt_off[f], q0 = dc_off[f];
    const int ng = min(max(gt_off[f + 1] - g0, 0), kMaxGt), nd = min(max(dt_off[f + 1] - d0, 0), kMaxDt);
    const int ndc = min(max(dc_off[f + 1] - q0, 0), kMaxDc);
    const int diff = cb.difficulty[c];
    int tp, fp, fn;
    double sim;
    match_frame<true>(lane, nd, ng, ndc, overlaps + ov_off[f], dt_score + d0, ign_gt + (int64_t)diff * total_gt + g0,
                      ign_dt + (int64_t)diff * total_dt + d0, cb.min_overlap[c], thresholds[(int64_t)c * tstride + t], metric,
                      compute_aos, dt_bbox + (int64_t)d0 * 4, dc_bbox + (int64_t)q0 * 4, gt_alpha + g0, dt_alpha + d0, nullptr, tp,
                      fp, fn, sim);
    if (lane == 0) {
        const int64_t slot = ((int64_t)c * tstride + t) * frames + f;
        part_cnt[slot * 3 + 0] = tp;
        part_cnt[slot * 3 + 1] = fp;
        part_cnt[slot * 3 + 2] = fn;
        part_sim[slot] = sim;
    }
}

// one wave per (combination, threshold): lane l adds frames l, l + 64, ... in ascending order, then a fixed butterfly over the
// lanes -- the order of the additions depends on the number of frames alone
__global__ __launch_bounds__(kWave) void kitti_pr_reduce_kernel(int frames, int tstride, Combos cb, const int *__restrict__ part_cnt,
                                                                const double *__restrict__ part_sim, int *__restrict__ pr_counts,
                                                                double *__restrict__ pr_similarity) {
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int64_t out = (int64_t)c * tstride + t;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if (t < cb.num_thresholds[c]) {
        for (int f = lane; f < frames; f += kWave) {
            const int64_t slot = out * frames + f;
            tp += part_cnt[slot * 3 + 0];
            fp += part_cnt[slot * 3 + 1];
            fn += part_cnt[slot * 3 + 2];
            sim += part_sim[slot];
        }
    }
    tp = wave_sum_i32(tp);
    fp = wave_sum_i32(fp);
    fn = wave_sum_i32(fn);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sim += __shfl_xor(sim, off, kWave);
    if (lane == 0) {
        pr_counts[out * 3 + 0] = tp;
        pr_counts[out * 3 + 1] = fp;
        pr_counts[out * 3 + 2] = fn;
        pr_similarity[out] = sim;
    }
}

bool fill_combos(Combos &cb, int combos, int num_difficulty, const int *difficulty, const double *min_overlap, const int *num_thresholds,
                 int tstride) {
    for (int c = 0; c < kMaxCombos; ++c) {
        cb.difficulty[c] = 0;
        cb.num_thresholds[c] = 0;
        cb.min_overlap[c] = 0.0;
    }
    for (int c = 0; c < combos; ++c) {
        if (difficulty[c] < 0 || difficulty[c] >= num_difficulty) return false;
        if (!(min_overlap[c] >= 0.0)) return false;  // the reduction equals the loop for min_overlap >= 0 (max_overlap starts at 0)
        cb.difficulty[c] = difficulty[c];
        cb.min_overlap[c] = min_overlap[c];
        if (num_thresholds) {
            if (num_thresholds[c] < 0 || num_thresholds[c] > tstride) return false;
            cb.num_thresholds[c] = num_thresholds[c];
        }
    }
    return true;
}

}  // namespace

}  // namespace epnet

using namespace epnet;

extern "C" int epnet_kitti_overlaps(int metric, int criterion, int frames, int max_rows, int max_cols, const int *row_off,
                                    const int *col_off, const int64_t *ov_off, const double *row_boxes, const double *col_boxes,
                                    double *overlaps, epnet_stream_t stream) {
    EPNET_REQUIRE(metric >= 0 && metric <= 2 && frames >= 0 && max_rows >= 0 && max_cols >= 0);
    EPNET_REQUIRE(metric == 0 ? (criterion >= -1 && criterion <= 1) : criterion == -1);
    if (max_rows > kMaxDt || max_cols > (kMaxGt > kMaxDc ? kMaxGt : kMaxDc)) return EPNET_ELIMIT;
    if (frames == 0 || max_rows == 0 || max_cols == 0) return EPNET_OK;
    EPNET_REQUIRE(row_off && col_off && ov_off && row_boxes && col_boxes && overlaps);
    hipLaunchKernelGGL(kitti_overlaps_kernel, dim3(frames, kOvWavesPerFrame), dim3(kWave), 0, (hipStream_t)stream, metric, criterion,
                       row_off, col_off, ov_off, row_boxes, col_boxes, overlaps);
    return check_launch("epnet_kitti_overlaps");
}

extern "C" int epnet_kitti_match(int frames, int total_gt, int total_dt, int max_gt, int max_dt, int num_difficulty, int combos,
                                 const int *combo_difficulty, const double *combo_min_overlap, const int *gt_off, const int *dt_off,
                                 const int64_t *ov_off, const double *overlaps, const double *dt_score, const int *ignored_gt,
                                 const int *ignored_dt, double *matched, epnet_stream_t stream) {
    EPNET_REQUIRE(frames >= 0 && total_gt >= 0 && total_dt >= 0 && max_gt >= 0 && max_dt >= 0 && num_difficulty >= 1 && combos >= 0);
    if (combos > kMaxCombos || max_gt > kMaxGt || max_dt > kMaxDt) return EPNET_ELIMIT;
    if (frames == 0 || combos == 0 || total_gt == 0) return EPNET_OK;
    EPNET_REQUIRE(combo_difficulty && combo_min_overlap && gt_off && dt_off && ov_off && ignored_gt && matched);
    EPNET_REQUIRE(total_dt == 0 || (dt_score && ignored_dt));  // `overlaps` is empty when no frame has both
    Combos cb;
    EPNET_REQUIRE(fill_combos(cb, combos, num_difficulty, combo_difficulty, combo_min_overlap, nullptr, 0));
    hipLaunchKernelGGL(kitti_match_kernel, dim3(frames, combos), dim3(kWave), 0, (hipStream_t)stream, total_gt, total_dt, cb, gt_off,
                       dt_off, ov_off, overlaps, dt_score, ignored_gt, ignored_dt, matched);
    return check_launch("epnet_kitti_match");
}

extern "C" size_t epnet_kitti_pr_workspace_bytes(int frames, int combos, int tstride) {
    if (frames <= 0 || combos <= 0 || tstride <= 0 || combos > kMaxCombos || tstride > kMaxThresh) return 0;
    const size_t slots = (size_t)frames * combos * tstride;
    Carver c;  // the per-frame partial counts (3 ints per slot), then the partial similarities
    c.take(slots * 3 * sizeof(int));
    c.take(slots * sizeof(double));
    return c.off;
}

extern "C" int epnet_kitti_pr(int frames, int total_gt, int total_dt, int max_gt, int max_dt, int max_dc, int num_difficulty, int combos,
                              int tstride, int metric, int compute_aos, const int *combo_difficulty, const double *combo_min_overlap,
                              const int *combo_num_thresholds, const int *gt_off, const int *dt_off, const int *dc_off,
                              const int64_t *ov_off, const double *overlaps, const double *dt_score, const int *ignored_gt,
                              const int *ignored_dt, const double *dt_bbox, const double *dc_bbox, const double *gt_alpha,
                              const double *dt_alpha, const double *thresholds, void *workspace, size_t workspace_bytes,
                              int *pr_counts, double *pr_similarity, epnet_stream_t stream) {
    EPNET_REQUIRE(frames >= 0 && total_gt >= 0 && total_dt >= 0 && max_gt >= 0 && max_dt >= 0 && max_dc >= 0 && num_difficulty >= 1);
    EPNET_REQUIRE(combos >= 0 && tstride >= 0 && metric >= 0 && metric <= 2);
    if (combos > kMaxCombos || tstride > kMaxThresh || max_gt > kMaxGt || max_dt > kMaxDt || max_dc > kMaxDc) return EPNET_ELIMIT;
    if (combos == 0 || tstride == 0) return EPNET_OK;
    EPNET_REQUIRE(combo_difficulty && combo_min_overlap && combo_num_thresholds && thresholds && pr_counts && pr_similarity);
    EPNET_REQUIRE(frames == 0 || (gt_off && dt_off && dc_off && ov_off));
    EPNET_REQUIRE(total_gt == 0 || (ignored_gt && gt_alpha));
    EPNET_REQUIRE(total_dt == 0 || (dt_score && ignored_dt && dt_bbox && dt_alpha));
    EPNET_REQUIRE(max_dc == 0 || metric != 0 || dc_bbox);
    Combos cb;
    EPNET_REQUIRE(fill_combos(cb, combos, num_difficulty, combo_difficulty, combo_min_overlap, combo_num_thresholds, tstride));
    int *part_cnt = nullptr;
    double *part_sim = nullptr;
    if (frames > 0) {
        EPNET_REQUIRE(workspace);
        if (workspace_bytes < epnet_kitti_pr_workspace_bytes(frames, combos, tstride)) return EPNET_ENOMEM;
        const size_t slots = (size_t)frames * combos * tstride;
        Carver c;
        part_cnt = (int *)((char *)workspace + c.take(slots * 3 * sizeof(int)));
        part_sim = (double *)((char *)workspace + c.take(slots * sizeof(double)));
        hipLaunchKernelGGL(kitti_pr_kernel, dim3(frames, tstride, combos), dim3(kWave), 0, (hipStream_t)stream, frames, total_gt, total_dt,
                           tstride, metric, compute_aos != 0, cb, gt_off, dt_off, dc_off, ov_off, overlaps, dt_score, ignored_gt,
                           ignored_dt, dt_bbox, dc_bbox, gt_alpha, dt_alpha, thresholds, part_cnt, part_sim);
        const int rc = check_launch("epnet_kitti_pr");
        if (rc != EPNET_OK) return rc;
    }
    hipLaunchKernelGGL(kitti_pr_reduce_kernel, dim3(tstride, combos), dim3(kWave), 0, (hipStream_t)stream, frames, tstride, cb, part_cnt,
                       part_sim, pr_counts, pr_similarity);
    return check_launch("epnet_kitti_pr (reduce)");
}
