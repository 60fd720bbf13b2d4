// rcnn_targets.hip -- the RCNN training targets' box work for gfx950: ROI augmentation by noise and ROI sampling
// (lib/rpn/proposal_target_layer.py:85-275). Every IoU is iou3d_pair (boxgeom.h), bit for bit epnet_boxes_iou3d's.
#include <math.h>

#include "boxgeom.h"
#include "common.h"

namespace epnet {

// ---- ROI augmentation by noise (lib/rpn/proposal_target_layer.py:220-247, aug_roi_by_noise_torch) ----------
// The reference walks the sampled ROIs one by one on the host: per ROI up to aug_times tries, each a host coin
// (np.random.rand() < 0.2 keeps the ROI as it is), a noisy box built by five small torch kernels
// (random_aug_box3d :250-275), a single-pair boxes_iou3d_gpu (another ~15 launches) and a device->host read of the
// IoU for the loop condition -- up to 640 such round trips per scene. Here the random draws of ALL tries are
// the caller's tables (drawn on the device with no sync), every (ROI, try) IoU is evaluated by its own lane, and
// the first try whose IoU ends the reference's loop (`not (iou < pos_thresh)`) is found with one ballot:
// the same boxes and IoUs as the loop fed with draw [k][cnt] at try cnt of ROI k.
//   keep_draw (k, aug_times) u8: 1 = "keep the original ROI" (:232-234)
//   noise (k, aug_times, 7) f32: pos_shift[3], hwl_scale[3], angle_rot -- aug = [xyz + shift, hwl * scale, ry + rot] (:259,274)
__device__ __forceinline__ void aug_box_of(const float *roi, const float *nz, bool keep, float *aug) {
#pragma unroll
    for (int j = 0; j < 7; ++j) aug[j] = roi[j];
    if (!keep) {
#pragma unroll
        for (int j = 0; j < 3; ++j) aug[j] = roi[j] + nz[j];
#pragma unroll
        for (int j = 3; j < 6; ++j) aug[j] = roi[j] * nz[j];
        aug[6] = roi[6] + nz[6];
    }
}

// TP = tries per ROI rounded up to a power of two (<= 64): 64 / TP ROIs per wave, lane = (roi, try)
__global__ __launch_bounds__(256) void aug_roi_wave_kernel(int k, int aug_times, int tp, float pos_thresh,
                                                           float *__restrict__ rois, const float *__restrict__ gts,
                                                           const float *__restrict__ iou_src, const int *__restrict__ tries,
                                                           const unsigned char *__restrict__ keep_draw,
                                                           const float *__restrict__ noise, float *__restrict__ iou_out) {
    const int lane = lane_id();
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int per_wave = 64 / tp;
    const int grp = lane / tp, t = lane - grp * tp;
    const int r = wave * per_wave + grp;
    const int n_try = r < k ? (tries ? min(max(tries[r], 0), aug_times) : aug_times) : 0;
    const bool active = t < n_try;
    float roi[7], gt[7], aug[7], nz[7];
    bool keep = true;
    float iou = 0.f;
    if (active) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            roi[j] = rois[(size_t)r * 7 + j];
            gt[j] = gts[(size_t)r * 7 + j];
            nz[j] = noise[((size_t)r * aug_times + t) * 7 + j];
        }
        keep = keep_draw[(size_t)r * aug_times + t] != 0;
        aug_box_of(roi, nz, keep, aug);
        iou = iou3d_pair(aug, gt);
    }
    // the loop runs try t+1 only while temp_iou < pos_thresh (:231): a try ends it when that comparison is false
    const unsigned long long ends = __ballot(active && !(iou < pos_thresh));
    const unsigned long long group_mask = (tp == 64 ? ~0ull : ((1ull << tp) - 1)) << (grp * tp);
    const unsigned long long mine = ends & group_mask;
    const int last = mine ? (__builtin_ctzll(mine) - grp * tp) : (n_try - 1);
    __syncthreads();  // every lane has read its ROI before the winners overwrite rows (waves of a block share no ROI,
                      // lanes of a wave are in lockstep; the barrier only orders the stores after the loads)
    if (active && t == last) {
#pragma unroll
        for (int j = 0; j < 7; ++j) rois[(size_t)r * 7 + j] = aug[j];
        iou_out[r] = keep ? iou_src[r] : iou;  // :243-246
    }
    if (r < k && n_try == 0 && t == 0) iou_out[r] = iou_src[r];  // no try ran (cnt == 0, :243): box untouched
}

// any number of tries: one thread walks the loop of one ROI
__global__ __launch_bounds__(64) void aug_roi_serial_kernel(int k, int aug_times, float pos_thresh, float *__restrict__ rois,
                                                            const float *__restrict__ gts, const float *__restrict__ iou_src,
                                                            const int *__restrict__ tries,
                                                            const unsigned char *__restrict__ keep_draw,
                                                            const float *__restrict__ noise, float *__restrict__ iou_out) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= k) return;
    const int n_try = tries ? min(max(tries[r], 0), aug_times) : aug_times;
    float roi[7], gt[7], aug[7], nz[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        roi[j] = rois[(size_t)r * 7 + j];
        gt[j] = gts[(size_t)r * 7 + j];
        aug[j] = roi[j];
    }
    float temp_iou = 0.f;
    int cnt = 0;
    bool keep = true;
    while (temp_iou < pos_thresh && cnt < n_try) {
#pragma unroll
        for (int j = 0; j < 7; ++j) nz[j] = noise[((size_t)r * aug_times + cnt) * 7 + j];
        keep = keep_draw[(size_t)r * aug_times + cnt] != 0;
        aug_box_of(roi, nz, keep, aug);
        temp_iou = iou3d_pair(aug, gt);
        ++cnt;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) rois[(size_t)r * 7 + j] = aug[j];
    iou_out[r] = (cnt == 0 || keep) ? iou_src[r] : temp_iou;
}

// ---- RCNN training targets: ROI sampling (lib/rpn/proposal_target_layer.py:85-218, sample_rois_for_rcnn) ---------------------
// The reference walks the scenes on the host: three `nonzero` syncs per scene, np.random.permutation / torch.randint on the
// host, index uploads. Here: (0) one workgroup per scene counts the box rows; (1) the (ROI, ground truth) pairs of a scene are spread over the lanes of ceil(m / (256 / g))
// workgroups, every IoU is iou3d_pair -- bit for bit epnet_boxes_iou3d's -- and lands in the workspace matrix; (2) ONE
// workgroup per scene folds each row to its maximum and first arg-max, compacts the three class lists in ascending ROI
// index (ballot + prefix, as proposal_bin_kernel), ranks the foreground candidates by the caller's keys, fills the R slots
// from the caller's uniform draws and gathers the rows. No value leaves the device, nothing depends on a launch order.
constexpr int kSmpThreads = 1024;
constexpr int kSmpMaxM = 4096;
constexpr int kSmpMaxR = 1024;
// ROIs per workgroup of the IoU phase: as many as give every thread ONE pair when all g rows count (a pair is a long chain of
// dependent arithmetic -- about 20 us -- so the phase lasts as long as the longest thread's list of pairs)
static inline int smp_rois_per_block(int g) { return g >= 256 ? 1 : 256 / g; }

// one workgroup per scene reads the box table ONCE (the IoU phase has up to m workgroups per scene)
__global__ __launch_bounds__(256) void rcnn_count_gt_kernel(int g, int gc, const float *__restrict__ gt, int *__restrict__ num_gt_out) {
    __shared__ int s_red[4];
    const int scene = blockIdx.x;
    const int counted = count_gt_rows(g, gc, gt + (size_t)scene * g * gc, s_red);
    if (threadIdx.x == 0) num_gt_out[scene] = counted;
}

__global__ __launch_bounds__(256) void rcnn_iou_kernel(int m, int g, int gc, int rois_per_block, const float *__restrict__ rois,
                                                       const float *__restrict__ gt, float *__restrict__ iou_mat,
                                                       const int *__restrict__ num_gt_in) {
    const int scene = blockIdx.y, first = blockIdx.x * rois_per_block;
    rois += (size_t)scene * m * 7;
    gt += (size_t)scene * g * gc;
    iou_mat += (size_t)scene * m * g;
    const int num_gt = max(num_gt_in[scene], 1);  // a scene without ground truth: the zero row 0 alone, every IoU 0
    const int n_roi = min(rois_per_block, m - first);
    const long long pairs = (long long)n_roi * num_gt;
    for (long long p = threadIdx.x; p < pairs; p += 256) {
        const int i = first + (int)(p / num_gt), j = (int)(p % num_gt);
        float a7[7], b7[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            a7[q] = rois[(size_t)i * 7 + q];
            b7[q] = gt[(size_t)j * gc + q];
        }
        iou_mat[(size_t)i * g + j] = iou3d_pair(a7, b7);
    }
}

// pick(list, u) of include/epnet_ops.h: entry min((int)(u * (float)len), len - 1), entry 0 for a NaN or negative u
__device__ __forceinline__ int pick_pos(float u, int len) {
    const float p = u * (float)len;
    if (!(p >= 0.f)) return 0;
    return p >= (float)len ? len - 1 : (int)p;
}

// the maximum of a row and the FIRST column that reaches it; a NaN wins over every number and then stays
__device__ __forceinline__ float row_max_first(const float *__restrict__ row, int n, int &arg) {
    float best = row[0];
    arg = 0;
    for (int j = 1; j < n; ++j) {
        const float v = row[j];
        if (v > best || (v != v && best == best)) {
            best = v;
            arg = j;
        }
    }
    return best;
}

__global__ __launch_bounds__(kSmpThreads) void rcnn_select_kernel(
    int m, int g, int gc, int per_image, int fg_per_image, float fg_thresh, float bg_thresh, float bg_thresh_lo,
    double hard_bg_ratio, int aug_times, const float *__restrict__ rois, const float *__restrict__ gt,
    const float *__restrict__ fg_key, const float *__restrict__ slot_u, const float *__restrict__ iou_mat,
    const int *__restrict__ num_gt_in, float *__restrict__ max_overlaps, int *__restrict__ gt_assignment,
    float *__restrict__ batch_rois, float *__restrict__ batch_gt, float *__restrict__ iou_src, int *__restrict__ tries,
    float *__restrict__ roi_iou_direct, int *__restrict__ src_inds, int *__restrict__ scene_info) {
    __shared__ unsigned short lists[3][kSmpMaxM];  // fg, hard, easy: ROI indices in ascending order
    __shared__ unsigned long long keys[kSmpMaxM];
    __shared__ int slot_src[kSmpMaxR];
    __shared__ int wave_cnt[3][kSmpThreads / 64];
    __shared__ int base[3];
    const int scene = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    rois += (size_t)scene * m * 7;
    gt += (size_t)scene * g * gc;
    fg_key += (size_t)scene * m;
    slot_u += (size_t)scene * per_image;
    iou_mat += (size_t)scene * m * g;
    max_overlaps += (size_t)scene * m;
    gt_assignment += (size_t)scene * m;
    const int counted = num_gt_in[scene];
    const int num_gt = max(counted, 1);
    if (threadIdx.x < 3) base[threadIdx.x] = 0;
    __syncthreads();
    for (int start = 0; start < m; start += kSmpThreads) {
        const int i = start + threadIdx.x;
        bool in[3] = {false, false, false};
        if (i < m) {
            int arg;
            const float best = row_max_first(iou_mat + (size_t)i * g, num_gt, arg);
            max_overlaps[i] = best;
            gt_assignment[i] = arg;
            in[0] = best >= fg_thresh;                                   // :117
            in[1] = best < bg_thresh && best >= bg_thresh_lo;             // :123-124
            in[2] = best < bg_thresh_lo;                                  // :122
        }
        unsigned long long mk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mk[c] = __ballot(in[c]);
            if (lane == 0) wave_cnt[c][wave] = (int)__popcll(mk[c]);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (in[c]) {
                int before = base[c];
                for (int w = 0; w < wave; ++w) before += wave_cnt[c][w];
                lists[c][before + popc_below(mk[c])] = (unsigned short)i;
            }
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            int t = 0;
            for (int w = 0; w < kSmpThreads / 64; ++w) t += wave_cnt[threadIdx.x][w];
            base[threadIdx.x] += t;
        }
        __syncthreads();
    }
    const int fg_num = base[0], hard_num = base[1], easy_num = base[2], bg_num = hard_num + easy_num;
    const int which = fg_num > 0 ? (bg_num > 0 ? 0 : 1) : (bg_num > 0 ? 2 : 3);
    const int fg_this = which == 0 ? min(fg_per_image, fg_num) : which == 1 ? per_image : 0;
    if (which == 0) {
        // the fg_this smallest keys in ascending (key, ROI index) order: a counting rank over unique 64-bit keys
        for (int q = threadIdx.x; q < fg_num; q += kSmpThreads) {
            const unsigned roi = lists[0][q];
            keys[q] = ((unsigned long long)ordered_key(fg_key[roi]) << 32) | roi;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < fg_num; q += kSmpThreads) {
            const unsigned long long mine = keys[q];
            int rank = 0;
            for (int k = 0; k < fg_num; ++k) rank += keys[k] < mine ? 1 : 0;
            if (rank < fg_this) slot_src[rank] = (int)(unsigned)mine;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int *info = scene_info + (size_t)scene * 6;
        info[0] = counted;
        info[1] = fg_num;
        info[2] = hard_num;
        info[3] = easy_num;
        info[4] = fg_this;
        info[5] = which;
    }
    const int bg_tries = aug_times > 0 ? 1 : 0;  // :174
    for (int j = threadIdx.x; j < per_image; j += kSmpThreads) {
        const float u = slot_u[j];
        int src;
        if (which == 3) {
            src = pick_pos(u, m);
        } else if (which == 1) {
            src = lists[0][pick_pos(u, fg_num)];
        } else if (j < fg_this) {
            src = slot_src[j];
        } else if (hard_num > 0 && easy_num > 0) {  // :194-206
            const int hard_slots = (int)((double)(per_image - fg_this) * hard_bg_ratio);
            src = j - fg_this < hard_slots ? lists[1][pick_pos(u, hard_num)] : lists[2][pick_pos(u, easy_num)];
        } else if (hard_num > 0) {
            src = lists[1][pick_pos(u, hard_num)];
        } else {
            src = lists[2][pick_pos(u, easy_num)];
        }
        const size_t o = (size_t)scene * per_image + j;
        int assigned;  // folded again from the matrix of the IoU launch rather than read back from this launch's own stores
        const float ov = row_max_first(iou_mat + (size_t)src * g, num_gt, assigned);
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            batch_rois[o * 7 + q] = rois[(size_t)src * 7 + q];
            batch_gt[o * 7 + q] = gt[(size_t)assigned * gc + q];
        }
        iou_src[o] = ov;
        tries[o] = j < fg_this ? aug_times : bg_tries;
        if (roi_iou_direct) roi_iou_direct[o] = ov;
        if (src_inds) src_inds[o] = src;
    }
}

}  // namespace epnet

using namespace epnet;

// the noise loop over k ROIs: the wave form up to 64 tries, the serial form beyond (arguments already checked)
static int aug_roi_launch(int k, int aug_times, float pos_thresh, float *roi_boxes3d, const float *gt_boxes3d,
                          const float *iou3d_src, const int *tries, const unsigned char *keep_draw, const float *noise,
                          float *iou_of_rois, hipStream_t s) {
    if (aug_times >= 1 && aug_times <= 64 && 0.f < pos_thresh) {  // (the loop starts from temp_iou = 0, :225)
        int tp = 1;
        while (tp < aug_times) tp *= 2;
        const int per_wave = 64 / tp;
        const int waves = div_up(k, per_wave);
        hipLaunchKernelGGL(aug_roi_wave_kernel, dim3(div_up(waves, 4)), dim3(256), 0, s, k, aug_times, tp, pos_thresh,
                           roi_boxes3d, gt_boxes3d, iou3d_src, tries, keep_draw, noise, iou_of_rois);
    } else {
        hipLaunchKernelGGL(aug_roi_serial_kernel, dim3(div_up(k, 64)), dim3(64), 0, s, k, aug_times, pos_thresh, roi_boxes3d,
                           gt_boxes3d, iou3d_src, tries, keep_draw, noise, iou_of_rois);
    }
    return check_launch("aug_roi_by_noise");
}

extern "C" int epnet_aug_roi_by_noise(int k, int aug_times, float pos_thresh, float *roi_boxes3d, const float *gt_boxes3d,
                                      const float *iou3d_src, const int *tries, const unsigned char *keep_draw,
                                      const float *noise, float *iou_of_rois, epnet_stream_t stream) {
    EPNET_REQUIRE(k >= 0 && aug_times >= 0);
    if (k == 0) return EPNET_OK;
    EPNET_REQUIRE(roi_boxes3d && gt_boxes3d && iou3d_src && iou_of_rois);
    EPNET_REQUIRE(aug_times == 0 || (keep_draw && noise));
    return aug_roi_launch(k, aug_times, pos_thresh, roi_boxes3d, gt_boxes3d, iou3d_src, tries, keep_draw, noise, iou_of_rois,
                          (hipStream_t)stream);
}

namespace {
struct SamplePlan {
    size_t off_num_gt, off_mat, off_max, off_assign, off_tries, off_iou_src, bytes;
};

SamplePlan sample_plan(int b, int m, int g, int r) {
    SamplePlan p;
    const size_t sb = (size_t)b, sm = (size_t)m, sg = (size_t)g, sr = (size_t)r;
    Carver c;
    p.off_num_gt = c.take(sb * sizeof(int));
    p.off_mat = c.take(sb * sm * sg * sizeof(float));
    p.off_max = c.take(sb * sm * sizeof(float));
    p.off_assign = c.take(sb * sm * sizeof(int));
    p.off_tries = c.take(sb * sr * sizeof(int));
    p.off_iou_src = c.take(sb * sr * sizeof(float));
    p.bytes = c.off;
    return p;
}
}  // namespace

extern "C" size_t epnet_rcnn_sample_rois_workspace_bytes(int b, int m, int g, int r) {
    if (b <= 0 || b > 65535 || m < 1 || m > kSmpMaxM || g < 1 || r < 1 || r > kSmpMaxR) return 0;
    return sample_plan(b, m, g, r).bytes;
}

extern "C" int epnet_rcnn_sample_rois(int b, int m, int g, int gc, int r, int fg_per_image, float fg_thresh, float cls_bg_thresh,
                                      float cls_bg_thresh_lo, double hard_bg_ratio, int aug_times, const float *rois,
                                      const float *gt_boxes3d, const float *fg_key, const float *slot_u,
                                      const unsigned char *keep_draw, const float *noise, void *workspace,
                                      size_t workspace_bytes, float *batch_rois, float *batch_gt_of_rois, float *batch_roi_iou,
                                      int *scene_info, int *src_inds, float *iou_src, int *tries, float *max_overlaps,
                                      int *gt_assignment, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && m >= 0 && g >= 0 && r >= 0 && aug_times >= 0 && fg_per_image >= 0);
    if (b == 0) return EPNET_OK;
    if (m < 1 || m > kSmpMaxM || r < 1 || r > kSmpMaxR || g < 1 || b > 65535) return EPNET_ELIMIT;
    EPNET_REQUIRE(gc >= 7 && gc <= 16 && fg_per_image <= r);
    EPNET_REQUIRE(rois && gt_boxes3d && fg_key && slot_u && workspace && batch_rois && batch_gt_of_rois && batch_roi_iou && scene_info);
    EPNET_REQUIRE(aug_times == 0 || (keep_draw && noise));
    const SamplePlan p = sample_plan(b, m, g, r);
    if (workspace_bytes < p.bytes) return EPNET_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *num_gt = (int *)(ws + p.off_num_gt);
    float *mat = (float *)(ws + p.off_mat);
    float *mo = max_overlaps ? max_overlaps : (float *)(ws + p.off_max);
    int *as = gt_assignment ? gt_assignment : (int *)(ws + p.off_assign);
    int *tr = tries ? tries : (int *)(ws + p.off_tries);
    float *src_iou = iou_src ? iou_src : (float *)(ws + p.off_iou_src);
    const int per_block = smp_rois_per_block(g);
    hipLaunchKernelGGL(rcnn_count_gt_kernel, dim3(b), dim3(256), 0, s, g, gc, gt_boxes3d, num_gt);
    int rc = check_launch("rcnn_sample_rois count");
    if (rc) return rc;
    hipLaunchKernelGGL(rcnn_iou_kernel, dim3(div_up(m, per_block), b), dim3(256), 0, s, m, g, gc, per_block, rois, gt_boxes3d, mat,
                       (const int *)num_gt);
    rc = check_launch("rcnn_sample_rois iou");
    if (rc) return rc;
    hipLaunchKernelGGL(rcnn_select_kernel, dim3(b), dim3(kSmpThreads), 0, s, m, g, gc, r, fg_per_image, fg_thresh, cls_bg_thresh,
                       cls_bg_thresh_lo, hard_bg_ratio, aug_times, rois, gt_boxes3d, fg_key, slot_u, (const float *)mat,
                       (const int *)num_gt, mo, as, batch_rois, batch_gt_of_rois, src_iou, tr,
                       aug_times == 0 ? batch_roi_iou : (float *)nullptr, src_inds, scene_info);
    rc = check_launch("rcnn_sample_rois select");
    if (rc || aug_times == 0) return rc;
    // the noise loop (:158-179) over all b * r rows: foreground slots get aug_times tries, background slots one
    return aug_roi_launch(b * r, aug_times, fg_thresh, batch_rois, batch_gt_of_rois, src_iou, tr, keep_draw, noise, batch_roi_iou, s);
}
