// fps.hip -- furthest point sampling for gfx950.
//
// Replaces furthest_point_sampling_kernel / _launcher of the reference
// (pointnet2_lib/pointnet2/src/sampling_gpu.cu:94-253). One workgroup per scene, as there, but the
// M-1 dependent arg-max iterations are rebuilt around the CDNA4 execution model. Four kernels:
//
//   fps_wave_kernel      N <= 1024 (and the brute-force fallback): the scene lives in VGPRs; lane / slot order
//                        equals the reference's tie-break order, so the wave arg-max is a DPP max + ballot + ff1;
//   pruned::fps_*_kernel 1024 < N <= 16384: registers again, points in spatial order, exact bucket pruning
//                        (see fps_pruned.h) -- over a caller-built scene index or self-sorting;
//   fps_bigscene_kernel  16384 < N <= 65536: bucket summaries in registers, points re-read from the index;
//   fps_stream_kernel    anything else: xyz / temp re-read through L2.
// Common to all but the last: NO global memory access inside the round loop (the selected indices are buffered in
// LDS and flushed with coalesced stores), one barrier per round (the reference has 11 and a dependent global load).
//
// Tie-breaking. The reference's result depends on its block size bs = opt_n_threads(N)
// (cuda_utils.h:10-14): thread tid scans k = tid, tid+bs, ... keeping the FIRST maximum (strict
// '>', :136-137), and at every level of the shared-memory tree the LOWER slot wins a tie (:86-91).
// Among equal distances the winner is therefore the point with the smallest
//         rank(k) = (bitreverse_{log2 bs}(k mod bs), k div bs)      (lexicographic).
// Physical thread q of this kernel holds the reference thread tid = bitreverse(q), slot j holds
// k = tid + j*bs, so rank order == (q, j) order == (wave, lane, slot) order: the winner among tied
// lanes is the lowest set bit of a ballot, among tied waves the lowest wave, among tied slots the
// lowest slot. Squared distances are >= +0 and never NaN for finite inputs, so comparing their
// bit patterns for equality is comparing the floats.
//
// Arithmetic: d = dx*dx + dy*dy + dz*dz evaluated left to right in fp32 without contraction
// (-ffp-contract=off), then min with the running distance, as sampling_gpu.cu:133-135.
//
// This file: one translation unit. The kernel families are in fps_common.h, fps_wave.h, fps_pruned.h, fps_bigscene.h and
// fps_stream.h (included in that order: static LDS and symbols keep their places); fps_plan.h decides, as a pure function of
// the shape, the NULL pattern and the tuning knobs, which of them a call gets and what runs in front of and behind it; below are
// the small kernels around the sampling, fps_run, which carries a plan out, and the extern "C" entry points.
#include <math.h>

#include "fps_common.h"
#include "fps_wave.h"
#include "fps_pruned.h"
#include "fps_bigscene.h"
#include "fps_stream.h"
#include "fps_plan.h"

using namespace epnet;

// skip: per scene, "the first skip[b] points of xyz are an unambiguous furthest-point sequence" (scenes with skip[b] >= m are
// left alone: fps_prefix_kernel has written their samples); prefix_out: per scene, receives the number of leading rounds of
// THIS sampling whose maximum was unique (initialised by fps_prefix_kernel) where the kernel can tell. Both may be NULL.
// Scenes whose first m points are known to be the samples (skip[b] >= m): idx = 0 .. m-1, and the knowledge is passed on;
// the others: prefix_out starts at `init` (m where the sampling kernel reports ties by lowering it, 0 where it cannot tell)
__global__ __launch_bounds__(256) void fps_prefix_kernel(int m, const int *__restrict__ skip, int *__restrict__ idx,
                                                         int *__restrict__ prefix_out, int init) {
    const int bs = blockIdx.x;
    const int have = skip ? skip[bs] : 0;
    const bool known = have >= m;
    if (threadIdx.x == 0 && prefix_out) prefix_out[bs] = known ? have : init;
    // (a scene whose rounds do run rewrites its indices itself; the known prefix is the same there)
    for (int i = threadIdx.x; i < min(have, m); i += 256) idx[(size_t)bs * m + i] = i;
}

// rows of the (B,N,3) cloud picked by idx (B,M): the centres of an SA level
__global__ __launch_bounds__(256) void gather_centres_kernel(int n, int m, const float *__restrict__ xyz,
                                                             const int *__restrict__ idx, float *__restrict__ out) {
    const int bs = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;  // element of the (m, 3) output
    if (e >= m * 3) return;
    const int i = e / 3, a = e - i * 3;
    out[(size_t)bs * m * 3 + e] = xyz[((size_t)bs * n + idx[(size_t)bs * m + i]) * 3 + a];
}

// four centres per thread (one 16-byte load of indices, three 16-byte stores): a twelfth of the waves of the kernel above. The
// gather sits on the sampling chain behind the FPS of every level above 1024 points (fps_wave_kernel writes its centres itself),
// and beside the wide kernels of the pipelined stack what a small kernel waits for is wave slots (77 - 118 us for a copy that
// takes 8 alone)
__global__ __launch_bounds__(256) void gather_centres4_kernel(int n, int m, const float *__restrict__ xyz,
                                                              const int *__restrict__ idx, float *__restrict__ out) {
    const int bs = blockIdx.y;
    const int i4 = blockIdx.x * 256 + threadIdx.x;  // group of four centres
    if (i4 * 4 >= m) return;
    const int4 ids = reinterpret_cast<const int4 *>(idx + (size_t)bs * m)[i4];
    const float *src = xyz + (size_t)bs * n * 3;
    const float *p0 = src + (size_t)ids.x * 3, *p1 = src + (size_t)ids.y * 3, *p2 = src + (size_t)ids.z * 3, *p3 = src + (size_t)ids.w * 3;
    const float a0 = p0[0], a1 = p0[1], a2 = p0[2], b0 = p1[0], b1 = p1[1], b2 = p1[2];
    const float c0 = p2[0], c1 = p2[1], c2 = p2[2], d0 = p3[0], d1 = p3[1], d2 = p3[2];
    float4 *dst = reinterpret_cast<float4 *>(out + ((size_t)bs * m + (size_t)i4 * 4) * 3);
    dst[0] = make_float4(a0, a1, a2, b0);
    dst[1] = make_float4(b1, b2, c0, c1);
    dst[2] = make_float4(c2, d0, d1, d2);
}

static void launch_gather_centres(int b, int n, int m, const float *xyz, const int *idx, float *new_xyz, hipStream_t s) {
    if ((m & 3) == 0 && (((uintptr_t)idx | (uintptr_t)new_xyz) & 15) == 0)
        hipLaunchKernelGGL(gather_centres4_kernel, dim3(div_up(m / 4, 256), b), dim3(256), 0, s, n, m, xyz, idx, new_xyz);
    else
        hipLaunchKernelGGL(gather_centres_kernel, dim3(div_up(m * 3, 256), b), dim3(256), 0, s, n, m, xyz, idx, new_xyz);
}

// carries a plan out: every decision is fps_plan's. (The instantiations are named in the order pruned, wave, stream, bigscene,
// indexed, in which the compiler emits them.)
static int fps_run(const FpsPlan &p, int b, int n, int m, const float *xyz, void *index, float *temp, int *idx, float *new_xyz,
                   const int *prefix_in, int *prefix_out, void *next_index, hipStream_t s) {
    if (p.rc != EPNET_OK || p.family == kFpsNone) return p.rc;
    const int *skip = p.prefix_in ? prefix_in : nullptr;
    const float4 *sorted = (const float4 *)index;
    const dim3 grid(b);
    if (p.prefix_init >= 0) {   // the kernel chosen does not do the prologue itself
        hipLaunchKernelGGL(fps_prefix_kernel, grid, dim3(256), 0, s, m, skip, idx, prefix_out, p.prefix_init);
        if (int rc = check_launch("sampling prefix")) return rc;
    }
#define EPNET_FPS_CASE(K_, W_, P_, ...) \
    case (W_) * 64 + (P_): hipLaunchKernelGGL((K_<W_, P_>), grid, dim3(64 * W_), p.lds, s, __VA_ARGS__); break
#define EPNET_FPS_PRUNED(W_, P_) EPNET_FPS_CASE(pruned::fps_pruned_kernel, W_, P_, n, m, xyz, temp, idx, skip, prefix_out, p.prefix_cap)
#define EPNET_FPS_WAVE(W_, P_) \
    EPNET_FPS_CASE(fps_wave_kernel, W_, P_, n, m, p.lg_bs, xyz, temp, idx, skip, prefix_out, p.prologue_init, p.writes_centres ? new_xyz : nullptr)
#define EPNET_FPS_WAVES(W_) EPNET_FPS_WAVE(W_, 1); EPNET_FPS_WAVE(W_, 2); EPNET_FPS_WAVE(W_, 4); EPNET_FPS_WAVE(W_, 8); EPNET_FPS_WAVE(W_, 16)
#define EPNET_FPS_INDEXED(W_, P_)                                                                                                  \
    EPNET_FPS_CASE(pruned::fps_indexed_kernel, W_, P_, n, m, sorted, temp, idx, skip, prefix_out, xyz, p.prefix_cap, p.prologue_init, \
                   p.builds_next ? next_index : nullptr, new_xyz)
    const int wp = p.waves * 64 + p.ppt;
    switch (p.family) {
        case kFpsPruned:
            switch (wp) { EPNET_FPS_PRUNED(8, 8); EPNET_FPS_PRUNED(8, 16); EPNET_FPS_PRUNED(8, 32);
                          EPNET_FPS_PRUNED(4, 8); EPNET_FPS_PRUNED(4, 16); EPNET_FPS_PRUNED(4, 32); }
            break;
        case kFpsWave:
            switch (wp) { EPNET_FPS_WAVES(1); EPNET_FPS_WAVES(2); EPNET_FPS_WAVES(4); EPNET_FPS_WAVES(8); EPNET_FPS_WAVES(16); }
            break;
        case kFpsStream:
            hipLaunchKernelGGL(fps_stream_kernel, grid, dim3(64 * p.waves), 0, s, n, m, p.lg_bs, xyz, temp, idx, skip);
            break;
        case kFpsBigscene: {
            const int np = scene_index_np(n);
            hipLaunchKernelGGL(pruned::fps_bigscene_kernel<16>, grid, dim3(1024), 0, s, n, np, m, xyz, sorted,
                               (const float *)(sorted + (size_t)b * np), temp, scene_index_sampling_scratch(b, n, index), idx, skip);
            break;
        }
        case kFpsIndexed:
            switch (wp) { EPNET_FPS_INDEXED(4, 8); EPNET_FPS_INDEXED(4, 16); EPNET_FPS_INDEXED(4, 32); EPNET_FPS_INDEXED(8, 32); }
            break;
        case kFpsNone: break;
    }
#undef EPNET_FPS_INDEXED
#undef EPNET_FPS_WAVES
#undef EPNET_FPS_WAVE
#undef EPNET_FPS_PRUNED
#undef EPNET_FPS_CASE
    if (int rc = check_launch("furthest_point_sampling")) return rc;
    if (p.follow == kFpsIndexBuild) {
        const int np2 = scene_index_np(m);
        float4 *sorted2 = (float4 *)next_index;
        float *boxes2 = (float *)(sorted2 + (size_t)b * np2);
        return spatial_index_launch(b, m, np2, xyz, sorted2, boxes2, boxes2 + (size_t)b * (np2 / 64) * 6, s, n, idx, new_xyz);
    }
    if (p.follow == kFpsGather) {
        launch_gather_centres(b, n, m, xyz, idx, new_xyz, s);
        return check_launch("sample_centres gather");
    }
    return EPNET_OK;
}

// what every entry point does: describe the call, plan it, run the plan
static int fps_sample(FpsEntry entry, int b, int n, int m, const float *xyz, void *index, size_t index_bytes, float *temp, int *idx,
                      float *new_xyz, epnet_stream_t stream, const int *prefix_in = nullptr, int *prefix_out = nullptr,
                      int prefix_cap = 0x7fffffff, void *next_index = nullptr, size_t next_index_bytes = 0) {
    const FpsCall call = {entry, b, n, m, index_bytes, next_index_bytes, xyz != nullptr, index != nullptr, temp != nullptr,
                          idx != nullptr, new_xyz != nullptr, prefix_in != nullptr, prefix_out != nullptr, next_index != nullptr,
                          ((uintptr_t)next_index & 15) == 0, prefix_cap};
    const FpsKnobs knobs = {tuning(kFpsPrune), tuning(kFpsPruneMin), tuning(kFpsPwaves), tuning(kFpsWaves)};
    return fps_run(fps_plan(call, knobs), b, n, m, xyz, index, temp, idx, new_xyz, prefix_in, prefix_out, next_index, (hipStream_t)stream);
}

extern "C" int epnet_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idx,
                                             epnet_stream_t stream) {
    return fps_sample(kFpsEntryPlain, b, n, m, xyz, nullptr, 0, temp, idx, nullptr, stream);
}

extern "C" int epnet_furthest_point_sampling_indexed(int b, int n, int m, const float *xyz, void *index,
                                                     size_t index_bytes, float *temp, int *idx,
                                                     epnet_stream_t stream) {
    return fps_sample(kFpsEntryIndexed, b, n, m, xyz, index, index_bytes, temp, idx, nullptr, stream);
}

// furthest point sampling from a fresh state AND the gather of the selected coordinates, i.e. the head of an SA module
// (pointnet2_modules.py:39-45: furthest_point_sample, then gather_operation on the flipped cloud, flipped back):
// idx (B,M) and new_xyz (B,M,3) = xyz[b, idx[b,i], :]. temp: running-distance scratch (B,N) or NULL (then every
// distance starts at 1e10 as pointnet2_utils.py:26 sets it; allowed for 64 <= n <= 16384); index may be NULL.
extern "C" int epnet_sample_centres(int b, int n, int m, const float *xyz, void *index, size_t index_bytes,
                                    float *temp, int *idx, float *new_xyz, epnet_stream_t stream) {
    return fps_sample(kFpsEntryCentres, b, n, m, xyz, index, index_bytes, temp, idx, new_xyz, stream);
}

// epnet_sample_centres for the levels of a sampling PYRAMID (SA level l + 1 samples the centres of level l).
// Furthest point sampling is nested: as long as every round's maximum is unique, the first m' samples of a sequence are the
// furthest-point samples OF that sequence (the global maximiser over all points is itself one of the candidates; the running
// distances are the same fp32 values), so idx = 0 .. m'-1 -- bit for bit what the reference's kernel computes on the centres,
// whose tie-break only matters among equal maxima. prefix_in[b] (or NULL) = the number of leading rounds of the sampling that
// produced xyz in which the maximum was unique up to exact twins; scenes with prefix_in[b] >= m take the identity, the others run
// the rounds.
// prefix_out[b] (or NULL) receives the same knowledge about THIS sampling's output (0 where the kernel cannot tell), looked
// for during the first prefix_cap rounds only (<= 0: all rounds) -- the next level's sample count is all anybody will ask for.
extern "C" int epnet_sample_centres_chain(int b, int n, int m, const float *xyz, void *index, size_t index_bytes,
                                          float *temp, int *idx, float *new_xyz, const int *prefix_in, int *prefix_out,
                                          int prefix_cap, epnet_stream_t stream) {
    // (new_xyz may be NULL: the indices alone, the centres come from epnet_scene_index_build_gathered)
    return fps_sample(kFpsEntryChain, b, n, m, xyz, index, index_bytes, temp, idx, new_xyz, stream, prefix_in, prefix_out, prefix_cap);
}

// epnet_sample_centres_chain AND the scene index of the m centres (epnet_scene_index_build_gathered on idx: what the next level of
// the pyramid starts with) into next_index, a buffer of epnet_scene_index_bytes(b, m) bytes; 1024 <= m <= 16384, new_xyz required.
// For 8192 < n <= 16384, 1024 <= m <= 4096 and no prefix_in the sampling workgroup of a scene gathers its centres and builds their
// index itself, as the epilogue of its rounds -- no dispatch between the sampling and the next level's; every other shape runs the
// two launches, with the same results. (The order of the points INSIDE a grid cell of an index is unspecified either way.)
extern "C" int epnet_sample_centres_chain_index(int b, int n, int m, const float *xyz, void *index, size_t index_bytes,
                                                float *temp, int *idx, float *new_xyz, const int *prefix_in, int *prefix_out,
                                                int prefix_cap, void *next_index, size_t next_index_bytes,
                                                epnet_stream_t stream) {
    return fps_sample(kFpsEntryChainIndex, b, n, m, xyz, index, index_bytes, temp, idx, new_xyz, stream, prefix_in, prefix_out,
                      prefix_cap, next_index, next_index_bytes);
}
