// proposals.hip -- the proposal layer for gfx950 (lib/rpn/proposal_layer.py:15-142).
// The reference walks the scenes on the host: boolean-mask indexing by distance bin (a sync each), top-K slices, NMS (mask
// to the host, host sweep), more slices, torch.cat, copy into the zero-padded result -- about ten host syncs per scene.
// Here: (1) one workgroup per scene walks the score-sorted order and compacts the members of each distance bin, in order,
// up to the bin's pre-NMS budget, and writes their BEV boxes (kitti_utils.boxes3d_to_bev_torch :137-150); (2) the NMS of
// all (scene, bin) groups runs as one batched mask + sweep with the group sizes read from device memory (nms.h); (3) one kernel
// gathers the first post-NMS survivors of bin 0, then of bin 1, into the zero-padded (b, post, 7) / (b, post) results.
// No value leaves the device. bins == 1 is score_based_proposal (:121-142): one bin that takes every box.
#include "common.h"
#include "nms.h"

namespace epnet {

constexpr int kBinThreads = 1024;

__device__ __forceinline__ int bin_of(float z, int bins) {  // nms_range_list = [0, 40, 80] (:65, :77-80)
    if (bins == 1) return 0;
    if (z > 0.f && z <= 40.f) return 0;
    if (z > 40.f && z <= 80.f) return 1;
    return -1;
}

// sel (b, 2, tot): positions IN THE SORTED ORDER of the members of each bin; counts (b*2): members kept for the NMS
__global__ __launch_bounds__(kBinThreads) void proposal_bin_kernel(int n, int bins, int pre0, int pre1, int cap,
                                                                   const float *__restrict__ proposals,
                                                                   const long long *__restrict__ order, int *__restrict__ sel,
                                                                   int *__restrict__ counts, float *__restrict__ bev) {
    __shared__ int wave_cnt[2][kBinThreads / 64];
    __shared__ int base[2];
    const int scene = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    const int tot = pre0 + pre1;
    proposals += (size_t)scene * n * 7;
    order += (size_t)scene * n;
    int *sel0 = sel + (size_t)scene * 2 * tot, *sel1 = sel0 + tot;
    if (threadIdx.x < 2) base[threadIdx.x] = 0;
    __syncthreads();
    for (int start = 0; start < n; start += kBinThreads) {
        const int i = start + threadIdx.x;
        int bin = -1;
        if (i < n) bin = bin_of(proposals[(size_t)order[i] * 7 + 2], bins);
        const unsigned long long m0 = __ballot(bin == 0), m1 = __ballot(bin == 1);
        if (lane == 0) {
            wave_cnt[0][wave] = __popcll(m0);
            wave_cnt[1][wave] = __popcll(m1);
        }
        __syncthreads();
        int before0 = base[0], before1 = base[1];
        for (int w = 0; w < wave; ++w) {
            before0 += wave_cnt[0][w];
            before1 += wave_cnt[1][w];
        }
        // bin 0 keeps pre0 + pre1 members: the tail serves bin 1 when that area holds no box at all (:92-100)
        if (bin == 0) {
            const int pos = before0 + popc_below(m0);
            if (pos < tot) sel0[pos] = i;
        } else if (bin == 1) {
            const int pos = before1 + popc_below(m1);
            if (pos < pre1) sel1[pos] = i;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t0 = 0, t1 = 0;
            for (int w = 0; w < kBinThreads / 64; ++w) {
                t0 += wave_cnt[0][w];
                t1 += wave_cnt[1][w];
            }
            base[0] += t0;
            base[1] += t1;
        }
        __syncthreads();
    }
    const int c0 = base[0], c1 = base[1];
    const int n0 = min(c0, pre0);
    int n1 = min(c1, pre1);
    if (bins == 2 && c1 == 0) {  // "this area doesn't have any points, so use rois of first area" (:92-100)
        n1 = max(min(c0, tot) - pre0, 0);
        for (int j = threadIdx.x; j < n1; j += kBinThreads) sel1[j] = sel0[pre0 + j];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[scene * 2] = n0;
        counts[scene * 2 + 1] = bins == 2 ? n1 : 0;
    }
    // BEV boxes of the members, in order: [x - l/2, z - w/2, x + l/2, z + w/2, ry]
    for (int bin = 0; bin < bins; ++bin) {
        const int cnt = bin ? n1 : n0;
        const int *src = bin ? sel1 : sel0;
        float *dst = bev + ((size_t)scene * 2 + bin) * cap * 5;
        for (int j = threadIdx.x; j < cnt; j += kBinThreads) {
            const float *p = proposals + (size_t)order[src[j]] * 7;
            const float half_l = p[5] / 2, half_w = p[4] / 2;
            dst[j * 5 + 0] = p[0] - half_l;
            dst[j * 5 + 1] = p[2] - half_w;
            dst[j * 5 + 2] = p[0] + half_l;
            dst[j * 5 + 3] = p[2] + half_w;
            dst[j * 5 + 4] = p[6];
        }
    }
}

__global__ __launch_bounds__(256) void proposal_emit_kernel(int n, int pre0, int pre1, int cap, int post0, int post1,
                                                            const float *__restrict__ proposals, const float *__restrict__ scores,
                                                            const long long *__restrict__ order, const int *__restrict__ sel,
                                                            const long long *__restrict__ keep, const int *__restrict__ num_keep,
                                                            float *__restrict__ ret_bbox3d, float *__restrict__ ret_scores,
                                                            int *__restrict__ ret_count) {
    const int scene = blockIdx.x;
    const int tot = pre0 + pre1, post = post0 + post1;
    const int k0 = min(num_keep[scene * 2], post0), k1 = min(num_keep[scene * 2 + 1], post1);
    if (threadIdx.x == 0 && ret_count) ret_count[scene] = k0 + k1;
    for (int j = threadIdx.x; j < post; j += 256) {
        float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        if (j < k0 + k1) {  // the kept boxes of bin 0, then those of bin 1 (torch.cat, :117-118)
            const int bin = j < k0 ? 0 : 1, pos = j < k0 ? j : j - k0;
            const int member = (int)keep[((size_t)scene * 2 + bin) * cap + pos];
            const long long src = order[(size_t)scene * n + sel[((size_t)scene * 2 + bin) * tot + member]];
#pragma unroll
            for (int q = 0; q < 7; ++q) row[q] = proposals[((size_t)scene * n + src) * 7 + q];
            sc = scores[(size_t)scene * n + src];
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) ret_bbox3d[((size_t)scene * post + j) * 7 + q] = row[q];
        ret_scores[(size_t)scene * post + j] = sc;
    }
}

}  // namespace epnet

using namespace epnet;

namespace {
struct ProposalPlan {
    int bins, pre0, pre1, post0, post1, cap, groups;
    size_t off_counts, off_num_keep, off_sel, off_bev, off_rot, off_keep, off_mask, bytes;
};

// pre / post budgets of the two distance bins: int(0.7 * total) and the rest (proposal_layer.py:66-69)
ProposalPlan proposal_plan(int b, int distance_based, int pre_nms_top_n, int post_nms_top_n) {
    ProposalPlan p;
    p.bins = distance_based ? 2 : 1;
    p.pre0 = distance_based ? (int)(pre_nms_top_n * 0.7) : pre_nms_top_n;
    p.pre1 = pre_nms_top_n - p.pre0;
    p.post0 = distance_based ? (int)(post_nms_top_n * 0.7) : post_nms_top_n;
    p.post1 = post_nms_top_n - p.post0;
    p.cap = p.pre0 > p.pre1 ? p.pre0 : p.pre1;
    if (p.cap < 1) p.cap = 1;
    p.groups = b * 2;
    const size_t g = (size_t)p.groups, cap = (size_t)p.cap, tot = (size_t)(p.pre0 + p.pre1);
    Carver c;
    p.off_counts = c.take(g * sizeof(int));
    p.off_num_keep = c.take(g * sizeof(int));
    p.off_sel = c.take(g * tot * sizeof(int));
    p.off_bev = c.take(g * cap * 5 * sizeof(float));
    p.off_rot = c.take(g * cap * sizeof(BoxRot));
    p.off_keep = c.take(g * cap * sizeof(long long));
    p.off_mask = c.take(g * cap * nms_mask_words(cap) * sizeof(unsigned long long));
    p.bytes = c.off;
    return p;
}
}  // namespace

extern "C" size_t epnet_rpn_proposals_workspace_bytes(int b, int distance_based, int pre_nms_top_n, int post_nms_top_n) {
    if (b <= 0 || pre_nms_top_n < 0 || post_nms_top_n < 0) return 0;
    return proposal_plan(b, distance_based, pre_nms_top_n, post_nms_top_n).bytes;
}

extern "C" int epnet_rpn_proposals(int b, int n, const float *proposals, const float *scores, const int64_t *order,
                                   int distance_based, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated,
                                   void *workspace, size_t workspace_bytes, float *ret_bbox3d, float *ret_scores, int *ret_count,
                                   epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && n >= 0 && pre_nms_top_n >= 0 && post_nms_top_n >= 0);
    if (b == 0 || post_nms_top_n == 0) return EPNET_OK;
    EPNET_REQUIRE(ret_bbox3d && ret_scores && workspace);
    EPNET_REQUIRE(n == 0 || (proposals && scores && order));
    const ProposalPlan p = proposal_plan(b, distance_based, pre_nms_top_n, post_nms_top_n);
    if (workspace_bytes < p.bytes) return EPNET_ENOMEM;
    if (b > 32767) return EPNET_ELIMIT;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *counts = (int *)(ws + p.off_counts), *num_keep = (int *)(ws + p.off_num_keep), *sel = (int *)(ws + p.off_sel);
    float *bev = (float *)(ws + p.off_bev);
    BoxRot *rot = (BoxRot *)(ws + p.off_rot);
    long long *keep = (long long *)(ws + p.off_keep);
    unsigned long long *mask = (unsigned long long *)(ws + p.off_mask);
    hipLaunchKernelGGL(proposal_bin_kernel, dim3(b), dim3(kBinThreads), 0, s, n, p.bins, p.pre0, p.pre1, p.cap, proposals,
                       (const long long *)order, sel, counts, bev);
    int rc = check_launch("rpn_proposals bin");
    if (rc) return rc;
    rc = nms_groups(rotated != 0, p.groups, p.cap, counts, bev, nms_thresh, rot, mask, keep, num_keep, s);
    if (rc) return rc;
    hipLaunchKernelGGL(proposal_emit_kernel, dim3(b), dim3(256), 0, s, n, p.pre0, p.pre1, p.cap, p.post0, p.post1, proposals, scores,
                       (const long long *)order, sel, keep, num_keep, ret_bbox3d, ret_scores, ret_count);
    return check_launch("rpn_proposals emit");
}
