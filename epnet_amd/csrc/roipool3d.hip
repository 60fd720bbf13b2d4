// roipool3d.hip -- point-in-box ROI pooling for gfx950.
//
// Replaces roipool3dLauncher and its three kernels assign_pts_to_box3d / get_pooled_idx /
// roipool3d_forward (lib/utils/roipool3d/src/roipool3d_kernel.cu:97-237; pt_in_box3d :14-28) and,
// with the same result, forward_slow (:31-94, :197-206).
//
// The reference materialises a (B,N,M) int assignment tensor (cudaMalloc'ed per call), then one
// THREAD per box walks it with stride-M reads to pick the first S in-box points. Here one
// workgroup owns one (scene, box): its 4 waves scan 4 contiguous quarters of the cloud 64 points
// at a time, __ballot + mbcnt compact the hits in index order into LDS, the four lists are
// concatenated in quarter order (= global index order), truncated to S and padded cyclically
// (k % cnt, :152-158); the same workgroup then copies the S rows (xyz + C features) with
// lane-contiguous loads/stores. No scratch tensor, no device allocation, no extra launches.
//
// Predicate arithmetic: as pt_in_box3d, fp32 in source order without contraction; the double
// sub-expressions of the reference (h / 2.0, -l / 2.0, ...) are exact halvings, so their float
// forms compare identically; cos/sin per the parity definition (correctly rounded, via double).
#include <math.h>

#include "common.h"
#include "cr_trig.h"

namespace epnet {

constexpr int kRpThreads = 256;
constexpr int kRpWaves = kRpThreads / 64;

// CANON: the eval branch of RCNNNet.forward (lib/net/rcnn_net.py:151-164) in the same launch. boxes3d are the ROIs as given;
// the kernel enlarges them for the membership test (kitti_utils.enlarge_box3d :153-163 -- h, w, l + 2 extra, y + extra) and
// its copy phase writes the xyz columns in the ROI's own frame: minus the ROI centre, then rotate_pc_along_y_torch (:45-63)
// by ry. Every element of both outputs is written: an empty box gets the transform of the reference's zero rows and flag
// 1, a non-empty one flag 0.
//
// TRAIN (MODE 2): the tail of ProposalTargetLayer.forward (lib/rpn/proposal_target_layer.py:16-83) in the same launch. Membership
// and the choice of the S rows are CANON's on the ROI as given; the copy phase takes a sampled point through data_augmentation
// (:292-349: rotation about y, scale, flip) and the canonical transformation (:51-62) with the AUGMENTED ROI, the ROI and its
// ground-truth row go through data_augmentation's box rules (and the ground truth through the canonical step), and the labels
// of :64-73 come out of the same workgroup. Points, features, boxes, labels and the mask score are tensors of their own.
enum { kRpPlain = 0, kRpCanon = 1, kRpTrain = 2 };

struct RpTrain {
    const float *gt_of_rois, *roi_iou, *aug;  // (B,R,7), (B,R), (B,R,3) [angle, scale, flip] or NULL
    float *sampled_pts, *feature_out, *rois_out, *gt_out, *mask_score;
    int *cls_label, *reg_valid_mask;
    float reg_fg_thresh, cls_fg_thresh, cls_bg_thresh;
};

__device__ __forceinline__ float rp_sign(float v) { return v > 0.f ? 1.0f : v < 0.f ? -1.0f : 0.0f; }  // torch.sign

// data_augmentation's rules for one box row (:305-347), fp32 in source order: alpha from beta = atan2(z, x) before the
// rotation, the centre rotated, ry = sign(beta') * pi / 2 + alpha - beta', columns 0..5 times scale, x times flip and
// ry = sign(ry) * pi - ry on a flip
__device__ __forceinline__ void rp_augment_box(float *b, float ca, float sa, float scale, float flip) {
    const float kPi = 3.14159265358979323846f;
    const float beta = cr_atan2f(b[2], b[0]);
    const float alpha = ((-rp_sign(beta) * kPi) / 2.0f + beta) + b[6];
    const float x = b[0] * ca + b[2] * (-sa), z = b[0] * sa + b[2] * ca;
    b[0] = x;
    b[2] = z;
    const float beta2 = cr_atan2f(z, x);
    b[6] = ((rp_sign(beta2) * kPi) / 2.0f + alpha) - beta2;
#pragma unroll
    for (int q = 0; q < 6; ++q) b[q] = b[q] * scale;
    b[0] = b[0] * flip;
    const float keep = flip == 1.0f ? 1.0f : 0.0f, mirror = flip == -1.0f ? 1.0f : 0.0f;
    b[6] = keep * b[6] + mirror * (rp_sign(b[6]) * kPi - b[6]);
}

template <int MODE>
__global__ __launch_bounds__(kRpThreads) void roipool3d_kernel(int pts_num, int boxes_num, int feature_in_len,
                                                               int sampled_pts_num, float extra,
                                                               const float *__restrict__ xyz,
                                                               const float *__restrict__ boxes3d,
                                                               const float *__restrict__ pts_feature,
                                                               float *__restrict__ pooled_features,
                                                               int *__restrict__ pooled_empty_flag, RpTrain tr) {
    constexpr bool CANON = MODE != kRpPlain;  // the enlarged box decides membership
    extern __shared__ int lds[];  // [kRpWaves][S] per-wave hit lists, then [S] final list
    __shared__ int wave_cnt[kRpWaves];
    __shared__ float wave_sum[kRpWaves];
    const int S = sampled_pts_num;
    int *lists = lds;
    int *final_idx = lds + kRpWaves * S;

    const int box = blockIdx.x, bs = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    xyz += (size_t)bs * pts_num * 3;
    pts_feature += (size_t)bs * pts_num * feature_in_len;
    const float *bx = boxes3d + ((size_t)bs * boxes_num + box) * 7;

    const float cx = bx[0], cz = bx[2], angle = bx[6];
    const float extra2 = 2.0f * extra;  // == (float)(2 * extra_width): a doubling is exact
    const float bottom_y = CANON ? bx[1] + extra : bx[1];
    const float h = CANON ? bx[3] + extra2 : bx[3], w = CANON ? bx[4] + extra2 : bx[4], l = CANON ? bx[5] + extra2 : bx[5];
    const float max_dis = 10.0f;
    const float cy = (float)((double)bottom_y - (double)h / 2.0);
    const float hh = h * 0.5f, hw = w * 0.5f, hl = l * 0.5f;
    float cosa, sina;
    cr_cossinf(angle, cosa, sina);
    const float nsina = -sina;

    // phase 1: each wave compacts the hits of its quarter of the cloud
    const int chunks = (pts_num + 63) / 64;
    const int per_wave = (chunks + kRpWaves - 1) / kRpWaves;
    const int k_begin = wave * per_wave * 64;
    const int k_end = min(pts_num, (wave + 1) * per_wave * 64);
    int cnt = 0;
    int *mylist = lists + wave * S;
    // the scan is a chain of dependent loads, not arithmetic: 8 chunks of 64 points are requested together and then
    // compacted in index order (positions beyond S are dropped, so testing up to 448 points past the S-th hit
    // changes nothing)
    constexpr int kRpChunks = 8;
    for (int k0 = k_begin; k0 < k_end && cnt < S; k0 += 64 * kRpChunks) {
        float px[kRpChunks], py[kRpChunks], pz[kRpChunks];
        bool valid[kRpChunks];
#pragma unroll
        for (int u = 0; u < kRpChunks; ++u) {
            const int k = k0 + u * 64 + lane;
            valid[u] = k < k_end;
            const int kk = valid[u] ? k : k_begin;
            px[u] = xyz[kk * 3 + 0];
            py[u] = xyz[kk * 3 + 1];
            pz[u] = xyz[kk * 3 + 2];
        }
#pragma unroll
        for (int u = 0; u < kRpChunks; ++u) {
            const float x = px[u], y = py[u], z = pz[u];
            bool in = false;
            if (valid[u] && !((fabsf(x - cx) > max_dis) || (fabsf(y - cy) > hh) || (fabsf(z - cz) > max_dis))) {
                const float x_rot = (x - cx) * cosa + (z - cz) * nsina;
                const float z_rot = (x - cx) * sina + (z - cz) * cosa;
                in = (x_rot >= -hl) & (x_rot <= hl) & (z_rot >= -hw) & (z_rot <= hw);
            }
            const unsigned long long mask = __ballot(in);
            if (mask) {
                const int pos = cnt + popc_below(mask);
                if (in && pos < S) mylist[pos] = k0 + u * 64 + lane;
                cnt += (int)__popcll(mask);
            }
        }
    }
    if (cnt > S) cnt = S;
    if (lane == 0) wave_cnt[wave] = cnt;
    __syncthreads();

    // phase 2: concatenate in quarter order, truncate to S, pad cyclically
    int offs[kRpWaves + 1];
    offs[0] = 0;
#pragma unroll
    for (int i = 0; i < kRpWaves; ++i) offs[i + 1] = offs[i] + wave_cnt[i];
    const int total = min(offs[kRpWaves], S);
    const int row = 3 + feature_in_len;
    float *dst_base = pooled_features + ((size_t)bs * boxes_num + box) * S * row;
    const float roi_y = bx[1];  // the ROI's own y, not the enlarged box's
    if constexpr (MODE == kRpTrain) {
        const size_t roi_id = (size_t)bs * boxes_num + box;
        const int C = feature_in_len;
        float roi[7], gtb[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            roi[q] = bx[q];
            gtb[q] = tr.gt_of_rois[roi_id * 7 + q];
        }
        const bool has_aug = tr.aug != nullptr;
        float ca = 1.0f, sa = 0.0f, scale = 1.0f, flip = 1.0f;
        if (has_aug) {
            const float ang = tr.aug[roi_id * 3 + 0];
            scale = tr.aug[roi_id * 3 + 1];
            flip = tr.aug[roi_id * 3 + 2];
            cr_cossinf(ang, ca, sa);
            rp_augment_box(roi, ca, sa, scale, flip);
            rp_augment_box(gtb, ca, sa, scale, flip);
        }
        // canonical transformation (:51-62): the points turn by the augmented ry, the ground truth by ry mod 2 pi
        const float kTwoPi = 6.28318530717958647692f;
        float ry_mod = fmodf(roi[6], kTwoPi);
        if (ry_mod != 0.0f && ry_mod < 0.0f) ry_mod = ry_mod + kTwoPi;  // torch's remainder: the sign of the divisor
        float c2, s2;
        cr_cossinf(roi[6], c2, s2);
        if (threadIdx.x == 0) {
            float cm, sm;
            cr_cossinf(ry_mod, cm, sm);
            const float gx = gtb[0] - roi[0], gy = gtb[1] - roi[1], gz = gtb[2] - roi[2];
            float *go = tr.gt_out + roi_id * 7;
            go[0] = gx * cm + gz * (-sm);
            go[1] = gy;
            go[2] = gx * sm + gz * cm;
            go[3] = gtb[3];
            go[4] = gtb[4];
            go[5] = gtb[5];
            go[6] = gtb[6] - ry_mod;
#pragma unroll
            for (int q = 0; q < 7; ++q) tr.rois_out[roi_id * 7 + q] = roi[q];
            const float iou = tr.roi_iou[roi_id];
            const bool valid = total != 0;
            int cls = iou > tr.cls_fg_thresh ? 1 : 0;
            if (iou > tr.cls_bg_thresh && iou < tr.cls_fg_thresh) cls = -1;
            if (!valid) cls = -1;
            tr.cls_label[roi_id] = cls;
            tr.reg_valid_mask[roi_id] = (iou > tr.reg_fg_thresh && valid) ? 1 : 0;
            pooled_empty_flag[roi_id] = valid ? 0 : 1;
        }
        auto place = [&](float px, float py, float pz, float &ox, float &oy, float &oz) {
            if (has_aug) {
                const float x1 = px * ca + pz * (-sa), z1 = px * sa + pz * ca;
                px = (x1 * scale) * flip;
                py = py * scale;
                pz = z1 * scale;
            }
            const float dx = px - roi[0], dy = py - roi[1], dz = pz - roi[2];
            ox = dx * c2 + dz * (-s2);
            oy = dy;
            oz = dx * s2 + dz * c2;
        };
        float *pts_dst = tr.sampled_pts + roi_id * S * 3;
        float *feat_dst = tr.feature_out + roi_id * S * C;
        if (total == 0) {  // what the reference's zero rows become; features 0, mask score 0
            float ox, oy, oz;
            place(0.0f, 0.0f, 0.0f, ox, oy, oz);
            for (int s = threadIdx.x; s < S; s += kRpThreads) {
                pts_dst[(size_t)s * 3 + 0] = ox;
                pts_dst[(size_t)s * 3 + 1] = oy;
                pts_dst[(size_t)s * 3 + 2] = oz;
            }
            for (size_t e = threadIdx.x; e < (size_t)S * C; e += kRpThreads) feat_dst[e] = 0.0f;
            if (threadIdx.x == 0) tr.mask_score[roi_id] = 0.0f;
            return;
        }
        for (int s = threadIdx.x; s < S; s += kRpThreads) {
            const int r = s % total;
            int src = 0;
#pragma unroll
            for (int i = 0; i < kRpWaves; ++i)
                if (r >= offs[i] && r < offs[i + 1]) src = lists[i * S + (r - offs[i])];
            final_idx[s] = src;
        }
        __syncthreads();
        // points and the mask score: thread t takes rows t, t + 256, ...; the partial sums fold in a fixed order
        float part = 0.0f;
        for (int s = threadIdx.x; s < S; s += kRpThreads) {
            const int src = final_idx[s];
            float ox, oy, oz;
            place(xyz[(size_t)src * 3 + 0], xyz[(size_t)src * 3 + 1], xyz[(size_t)src * 3 + 2], ox, oy, oz);
            pts_dst[(size_t)s * 3 + 0] = ox;
            pts_dst[(size_t)s * 3 + 1] = oy;
            pts_dst[(size_t)s * 3 + 2] = oz;
            if (C > 0) part = part + pts_feature[(size_t)src * C];
        }
        part = wave_sum_f32(part);
        if (lane == 0) wave_sum[wave] = part;
        __syncthreads();
        if (threadIdx.x == 0) {
            float total_mask = 0.0f;
#pragma unroll
            for (int i = 0; i < kRpWaves; ++i) total_mask = total_mask + wave_sum[i];
            tr.mask_score[roi_id] = total_mask / (float)S;
        }
        // features: kRpRows rows per wave and step, lane-contiguous
        constexpr int kRpRowsT = 16;
        for (int s0 = wave * kRpRowsT; s0 < S; s0 += kRpWaves * kRpRowsT) {
            for (int e = lane; e < C; e += 64) {
                float v[kRpRowsT];
#pragma unroll
                for (int u = 0; u < kRpRowsT; ++u) v[u] = pts_feature[(size_t)final_idx[min(s0 + u, S - 1)] * C + e];
#pragma unroll
                for (int u = 0; u < kRpRowsT; ++u)
                    if (s0 + u < S) feat_dst[(size_t)(s0 + u) * C + e] = v[u];
            }
        }
        return;
    }
    if (total == 0) {
        if (threadIdx.x == 0) pooled_empty_flag[(size_t)bs * boxes_num + box] = 1;  // :146-148
        if (CANON) {
            // the reference's zero rows go through the subtraction and the rotation as well (rcnn_net.py:155-164)
            const float dx = 0.0f - cx, dy = 0.0f - roi_y, dz = 0.0f - cz;
            const float ox = dx * cosa + dz * nsina, oz = dx * sina + dz * cosa;
            for (int s = wave; s < S; s += kRpWaves)
                for (int e = lane; e < row; e += 64)
                    dst_base[(size_t)s * row + e] = e == 0 ? ox : e == 1 ? dy : e == 2 ? oz : 0.0f;
        }
        return;  // plain: rows of an empty box are left as the caller initialised them (:177-179)
    }
    if (CANON && threadIdx.x == 0) pooled_empty_flag[(size_t)bs * boxes_num + box] = 0;
    for (int s = threadIdx.x; s < S; s += kRpThreads) {
        const int r = s % total;
        int src = 0;
#pragma unroll
        for (int i = 0; i < kRpWaves; ++i)
            if (r >= offs[i] && r < offs[i + 1]) src = lists[i * S + (r - offs[i])];
        final_idx[s] = src;
    }
    __syncthreads();

    // phase 3: copy xyz + features of the S sampled points, one row per wave at a time
    // kRpRows rows per wave and step: their gathers are in flight together (the copy is a chain of dependent
    // loads -- list entry, then the row -- not a bandwidth problem at these sizes)
    constexpr int kRpRows = 16;
    for (int s0 = wave * kRpRows; s0 < S; s0 += kRpWaves * kRpRows) {
        for (int e = lane; e < row; e += 64) {
            float v[kRpRows];
#pragma unroll
            for (int u = 0; u < kRpRows; ++u) {
                const int src = final_idx[min(s0 + u, S - 1)];
                v[u] = e < 3 ? xyz[(size_t)src * 3 + e] : pts_feature[(size_t)src * feature_in_len + (e - 3)];
            }
#pragma unroll
            for (int u = 0; u < kRpRows; ++u) {
                float out = v[u];
                if (CANON && e < 64) {
                    // lanes 0 - 2 of the first pass hold x, y, z of the row (row >= 3, so they are always there); lanes 0
                    // and 2 each need both x and z: read across the wave, every lane computes, lanes 0 - 2 keep their column
                    const int bits = __float_as_int(out);
                    const float dx = __int_as_float(__builtin_amdgcn_readlane(bits, 0)) - cx;
                    const float dy = __int_as_float(__builtin_amdgcn_readlane(bits, 1)) - roi_y;
                    const float dz = __int_as_float(__builtin_amdgcn_readlane(bits, 2)) - cz;
                    const float ox = dx * cosa + dz * nsina, oz = dx * sina + dz * cosa;
                    out = e == 0 ? ox : e == 1 ? dy : e == 2 ? oz : out;
                }
                if (s0 + u < S) dst_base[(size_t)(s0 + u) * row + e] = out;
            }
        }
    }
}

}  // namespace epnet

using namespace epnet;

extern "C" size_t epnet_roipool3d_workspace_bytes(int, int, int) { return 0; }  // fused kernel: no scratch

template <int MODE>
static int roipool3d_launch(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num, float extra,
                            const float *xyz, const float *boxes3d, const float *pts_feature, float *pooled_features,
                            int *pooled_empty_flag, epnet_stream_t stream, RpTrain tr = RpTrain()) {
    EPNET_REQUIRE(batch_size >= 0 && pts_num >= 0 && boxes_num >= 0 && feature_in_len >= 0 && sampled_pts_num >= 0);
    if (batch_size == 0 || boxes_num == 0) return EPNET_OK;
    if (MODE == kRpTrain) {
        EPNET_REQUIRE(boxes3d && pooled_empty_flag && tr.gt_of_rois && tr.roi_iou && tr.rois_out && tr.gt_out && tr.cls_label &&
                      tr.reg_valid_mask && tr.mask_score);
        EPNET_REQUIRE(sampled_pts_num == 0 || (tr.sampled_pts && (tr.feature_out || feature_in_len == 0)));
    } else {
        EPNET_REQUIRE(boxes3d && pooled_empty_flag && (sampled_pts_num == 0 || pooled_features));
    }
    EPNET_REQUIRE(pts_num == 0 || (xyz && (pts_feature || feature_in_len == 0)));
    if (batch_size > 65535) return EPNET_ELIMIT;
    const size_t lds = (size_t)(kRpWaves + 1) * sampled_pts_num * sizeof(int);
    if (lds > 150 * 1024) return EPNET_ELIMIT;
    hipLaunchKernelGGL(roipool3d_kernel<MODE>, dim3(boxes_num, batch_size), dim3(kRpThreads), lds, (hipStream_t)stream, pts_num,
                       boxes_num, feature_in_len, sampled_pts_num, extra, xyz, boxes3d, pts_feature, pooled_features,
                       pooled_empty_flag, tr);
    return check_launch(MODE == kRpTrain ? "roipool3d_train" : MODE == kRpCanon ? "roipool3d_canonical" : "roipool3d");
}

extern "C" int epnet_roipool3d(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num,
                               const float *xyz, const float *boxes3d, const float *pts_feature, float *pooled_features,
                               int *pooled_empty_flag, void *, size_t, epnet_stream_t stream) {
    return roipool3d_launch<kRpPlain>(batch_size, pts_num, boxes_num, feature_in_len, sampled_pts_num, 0.0f, xyz, boxes3d,
                                   pts_feature, pooled_features, pooled_empty_flag, stream);
}

extern "C" int epnet_roipool3d_canonical(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num,
                                         float pool_extra_width, const float *xyz, const float *rois,
                                         const float *pts_feature, float *pooled_features, int *pooled_empty_flag,
                                         epnet_stream_t stream) {
    return roipool3d_launch<kRpCanon>(batch_size, pts_num, boxes_num, feature_in_len, sampled_pts_num, pool_extra_width, xyz, rois,
                                  pts_feature, pooled_features, pooled_empty_flag, stream);
}

extern "C" int epnet_roipool3d_train(int batch_size, int pts_num, int boxes_num, int feature_in_len, int sampled_pts_num,
                                     float pool_extra_width, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh,
                                     const float *xyz, const float *pts_feature, const float *rois, const float *gt_of_rois,
                                     const float *roi_iou, const float *aug, float *sampled_pts, float *pts_feature_out,
                                     float *rois_out, float *gt_out, int *cls_label, int *reg_valid_mask, float *mask_score,
                                     int *pooled_empty_flag, epnet_stream_t stream) {
    RpTrain tr;
    tr.gt_of_rois = gt_of_rois;
    tr.roi_iou = roi_iou;
    tr.aug = aug;
    tr.sampled_pts = sampled_pts;
    tr.feature_out = pts_feature_out;
    tr.rois_out = rois_out;
    tr.gt_out = gt_out;
    tr.mask_score = mask_score;
    tr.cls_label = cls_label;
    tr.reg_valid_mask = reg_valid_mask;
    tr.reg_fg_thresh = reg_fg_thresh;
    tr.cls_fg_thresh = cls_fg_thresh;
    tr.cls_bg_thresh = cls_bg_thresh;
    return roipool3d_launch<kRpTrain>(batch_size, pts_num, boxes_num, feature_in_len, sampled_pts_num, pool_extra_width, xyz, rois,
                                      pts_feature, (float *)nullptr, pooled_empty_flag, stream, tr);
}
