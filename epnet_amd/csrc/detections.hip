// detections.hip -- the second-stage detections for gfx950 (tools/eval_rcnn.py:663-683). det.hip is the deterministic gradients.
// The reference walks the scenes on the host: `inds.sum() == 0` (a sync), boolean-mask indexing (a sync), a sort, nms_gpu (mask
// to the host, host sweep), more indexing. Here: (1) one workgroup per scene thresholds the scores, ranks the candidates --
// descending score, equal scores by ascending index -- and writes their BEV boxes in rank order; (2) the batched NMS of the
// proposal layer (nms.h) with the candidate counts read from device memory; (3) one kernel gathers the kept boxes and raw scores
// into the zero-padded results. No value leaves the device.
#include "common.h"
#include "nms.h"

namespace epnet {

constexpr int kDetThreads = 1024;
constexpr int kDetMaxM = 4096;

// ordered_key (common.h): float -> unsigned, order preserving; it fixes the order of the candidates below

// sel (b, m): ROI index of the candidate at each rank; counts (b): candidates; bev (b, m, 5) in rank order
__global__ __launch_bounds__(kDetThreads) void det_select_kernel(int m, float score_thresh, const float *__restrict__ boxes3d,
                                                                 const float *__restrict__ raw_scores,
                                                                 const float *__restrict__ norm_scores, int *__restrict__ sel,
                                                                 int *__restrict__ counts, float *__restrict__ bev) {
    __shared__ unsigned long long keys[kDetMaxM];
    __shared__ int s_count;
    const int scene = blockIdx.x, lane = lane_id();
    boxes3d += (size_t)scene * m * 7;
    raw_scores += (size_t)scene * m;
    norm_scores += (size_t)scene * m;
    sel += (size_t)scene * m;
    bev += (size_t)scene * m * 5;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    // candidates into LDS in any order: the key (score, then the LOWER index first) is unique, so the rank below does not
    // depend on where a key sits. Every wave runs the same number of rounds (ballot over whole waves).
    for (int start = 0; start < m; start += kDetThreads) {
        const int i = start + threadIdx.x;
        const int ic = min(i, m - 1);
        const float norm = norm_scores[ic], raw = raw_scores[ic];
        const bool cand = i < m && norm > score_thresh;
        const unsigned long long mask = __ballot(cand);
        if (mask) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_count, (int)__popcll(mask));
            base = __builtin_amdgcn_readfirstlane(base);
            if (cand) keys[base + popc_below(mask)] = ((unsigned long long)ordered_key(raw) << 32) | (unsigned)(~(unsigned)i);
        }
    }
    __syncthreads();
    const int c = s_count;
    if (threadIdx.x == 0) counts[scene] = c;
    // counting rank: the number of keys above mine
    for (int j0 = 0; j0 < c; j0 += kDetThreads) {
        const int j = j0 + threadIdx.x;
        const unsigned long long mine = keys[min(j, c - 1)];
        int rank = 0;
        for (int k = 0; k < c; ++k) rank += keys[k] > mine ? 1 : 0;
        if (j < c) {
            const int src = (int)(~(unsigned)mine);
            const float *p = boxes3d + (size_t)src * 7;
            const float half_l = p[5] / 2, half_w = p[4] / 2;
            sel[rank] = src;
            bev[rank * 5 + 0] = p[0] - half_l;
            bev[rank * 5 + 1] = p[2] - half_w;
            bev[rank * 5 + 2] = p[0] + half_l;
            bev[rank * 5 + 3] = p[2] + half_w;
            bev[rank * 5 + 4] = p[6];
        }
    }
}

__global__ __launch_bounds__(256) void det_emit_kernel(int m, const float *__restrict__ boxes3d,
                                                       const float *__restrict__ raw_scores, const int *__restrict__ sel,
                                                       const long long *__restrict__ keep, const int *__restrict__ num_keep,
                                                       float *__restrict__ det_boxes3d, float *__restrict__ det_scores,
                                                       int *__restrict__ det_count) {
    const int scene = blockIdx.x;
    const int kept = min(num_keep[scene], m);
    if (threadIdx.x == 0) det_count[scene] = kept;
    for (int j = threadIdx.x; j < m; j += 256) {
        float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        if (j < kept) {
            const int src = sel[(size_t)scene * m + (int)keep[(size_t)scene * m + j]];
#pragma unroll
            for (int q = 0; q < 7; ++q) row[q] = boxes3d[((size_t)scene * m + src) * 7 + q];
            sc = raw_scores[(size_t)scene * m + src];
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) det_boxes3d[((size_t)scene * m + j) * 7 + q] = row[q];
        det_scores[(size_t)scene * m + j] = sc;
    }
}

}  // namespace epnet

using namespace epnet;

namespace {
struct DetPlan {
    size_t off_counts, off_num_keep, off_sel, off_bev, off_rot, off_keep, off_mask, bytes;
};

DetPlan det_plan(int b, int m) {
    DetPlan p;
    const size_t g = (size_t)b, cap = (size_t)m;
    Carver c;
    p.off_counts = c.take(g * sizeof(int));
    p.off_num_keep = c.take(g * sizeof(int));
    p.off_sel = c.take(g * cap * sizeof(int));
    p.off_bev = c.take(g * cap * 5 * sizeof(float));
    p.off_rot = c.take(g * cap * sizeof(BoxRot));
    p.off_keep = c.take(g * cap * sizeof(long long));
    p.off_mask = c.take(g * cap * nms_mask_words(cap) * sizeof(unsigned long long));
    p.bytes = c.off;
    return p;
}
}  // namespace

extern "C" size_t epnet_rcnn_detections_workspace_bytes(int b, int m) {
    if (b <= 0 || m < 1 || m > kDetMaxM || b > 65535) return 0;
    return det_plan(b, m).bytes;
}

extern "C" int epnet_rcnn_detections(int b, int m, const float *boxes3d, const float *raw_scores, const float *norm_scores,
                                     float score_thresh, float nms_thresh, void *workspace, size_t workspace_bytes,
                                     float *det_boxes3d, float *det_scores, int *det_count, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && m >= 0);
    if (b == 0) return EPNET_OK;
    if (m < 1 || m > kDetMaxM || b > 65535) return EPNET_ELIMIT;
    EPNET_REQUIRE(boxes3d && raw_scores && norm_scores && workspace && det_boxes3d && det_scores && det_count);
    const DetPlan p = det_plan(b, m);
    if (workspace_bytes < p.bytes) return EPNET_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *counts = (int *)(ws + p.off_counts), *num_keep = (int *)(ws + p.off_num_keep), *sel = (int *)(ws + p.off_sel);
    float *bev = (float *)(ws + p.off_bev);
    BoxRot *rot = (BoxRot *)(ws + p.off_rot);
    long long *keep = (long long *)(ws + p.off_keep);
    unsigned long long *mask = (unsigned long long *)(ws + p.off_mask);
    hipLaunchKernelGGL(det_select_kernel, dim3(b), dim3(kDetThreads), 0, s, m, score_thresh, boxes3d, raw_scores, norm_scores, sel,
                       counts, bev);
    int rc = check_launch("rcnn_detections select");
    if (rc) return rc;
    rc = nms_groups(true, b, m, counts, bev, nms_thresh, rot, mask, keep, num_keep, s);
    if (rc) return rc;
    hipLaunchKernelGGL(det_emit_kernel, dim3(b), dim3(256), 0, s, m, boxes3d, raw_scores, sel, keep, num_keep, det_boxes3d,
                       det_scores, det_count);
    return check_launch("rcnn_detections emit");
}
