// ball_query.hip -- radius neighbour search for gfx950.
//
// Replaces ball_query_kernel_fast / _launcher (pointnet2_lib/pointnet2/src/ball_query_gpu.cu:9-66).
// The reference walks all N points with ONE THREAD per centre (stride-3 scalar loads, divergent
// early exit). Here one 64-lane wave owns CPW centres: the block stages a tile of the interleaved
// (N,3) xyz array in LDS with coalesced loads, each lane tests one point of a 64-point chunk
// against the wave's centres (held in scalar registers), and __ballot + mbcnt give every hit its
// slot in index order -- so "the first nsample points with d2 < r2, in index order, padded with
// the first hit" (:29-43) is preserved exactly while the scan is 64 points wide. A wave stops
// scanning as soon as all its centres are full; the block leaves when all its waves have.
//
// d2 = (cx-x)*(cx-x) + (cy-y)*(cy-y) + (cz-z)*(cz-z) in source order, no contraction; strict '<'.

#include "common.h"
#include "dpp.h"
#include "spatial.h"

namespace epnet {

constexpr int kBqTile = 2048;     // points per LDS tile (24 KiB)
constexpr int kBqThreads = 256;   // 4 waves

template <int CPW>
__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(int n, int m, float radius2, int nsample,
                                                                const float *__restrict__ new_xyz,
                                                                const float *__restrict__ xyz,
                                                                int *__restrict__ idx) {
    __shared__ float tile[kBqTile * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bs = blockIdx.y;
    xyz += (size_t)bs * n * 3;
    new_xyz += (size_t)bs * m * 3;
    idx += (size_t)bs * m * nsample;

    const int c0 = (blockIdx.x * (kBqThreads / 64) + wave) * CPW;
    float cx[CPW], cy[CPW], cz[CPW];
    int cnt[CPW], first[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ci = c0 + i;
        const bool ok = ci < m;
        cx[i] = ok ? new_xyz[ci * 3 + 0] : 0.f;
        cy[i] = ok ? new_xyz[ci * 3 + 1] : 0.f;
        cz[i] = ok ? new_xyz[ci * 3 + 2] : 0.f;
        cnt[i] = ok ? 0 : nsample;  // out-of-range centres count as already full
        first[i] = 0;
    }

    for (int t0 = 0; t0 < n; t0 += kBqTile) {
        const int tn = min(kBqTile, n - t0);
        for (int e = threadIdx.x; e < tn * 3; e += kBqThreads) tile[e] = xyz[(size_t)t0 * 3 + e];
        __syncthreads();

        bool wave_done = true;
#pragma unroll
        for (int i = 0; i < CPW; ++i) wave_done = wave_done && (cnt[i] >= nsample);

        if (!wave_done) {
            for (int p0 = 0; p0 < tn; p0 += 64) {
                const int p = p0 + lane;
                const bool valid = p < tn;
                const float x = valid ? tile[p * 3 + 0] : 0.f;
                const float y = valid ? tile[p * 3 + 1] : 0.f;
                const float z = valid ? tile[p * 3 + 2] : 0.f;
                bool all_full = true;
#pragma unroll
                for (int i = 0; i < CPW; ++i) {
                    if (cnt[i] < nsample) {  // wave-uniform
                        const float dx = cx[i] - x, dy = cy[i] - y, dz = cz[i] - z;
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        const bool hit = valid && (d2 < radius2);
                        const unsigned long long mask = __ballot(hit);
                        if (mask) {
                            const int pos = cnt[i] + popc_below(mask);
                            if (hit && pos < nsample) idx[(size_t)(c0 + i) * nsample + pos] = t0 + p;
                            if (cnt[i] == 0) first[i] = t0 + p0 + (int)__builtin_ctzll(mask);
                            cnt[i] += (int)__popcll(mask);
                        }
                        all_full = all_full && (cnt[i] >= nsample);
                    }
                }
                if (all_full) {
                    wave_done = true;
                    break;
                }
            }
        }
        // barrier before the tile is overwritten; doubles as the block-wide "everyone full" vote
        if (__syncthreads_and(wave_done ? 1 : 0)) break;
    }

    // padding: slots [cnt, nsample) repeat the first hit (:35-39); an empty ball is all zeros
    // (the value the caller's zero fill leaves in the reference, pointnet2_utils.py:218)
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ci = c0 + i;
        if (ci < m && cnt[i] < nsample) {
            const int fill = cnt[i] > 0 ? first[i] : 0;
            for (int l = cnt[i] + lane; l < nsample; l += 64) idx[(size_t)ci * nsample + l] = fill;
        }
    }
}


// ---- indexed path ----------------------------------------------------------------------------------
//
// For the big levels (N from 2048 up to 65536) the scan is N*M pair tests although a ball only ever contains a
// handful of points. With caller-supplied scratch the query is split in two launches:
//   bq_index_kernel  one workgroup per scene sorts the points by grid cell (counting sort on an interleaved cell code)
//                    and writes them, with their ORIGINAL index, as float4 plus one bounding box per
//                    bucket of 64 consecutive sorted points;
//   bq_query_kernel  one wave per centre: the lanes test the buckets' boxes against the ball (the lower
//                    bound |clamp(c, box) - c|^2 uses the point-test expression, so by monotonicity of
//                    fp32 arithmetic no bucket holding a hit is ever skipped), the few surviving
//                    buckets are tested point by point, and every hit sets bit `original index` in an
//                    N-bit LDS bitmap. Reading the bitmap back in order yields exactly the reference's
//                    result: the first nsample hits in index order, padded with the first one.
// The point test is the same expression as above: d2 = (cx-x)*(cx-x) + (cy-y)*(cy-y) + (cz-z)*(cz-z).

// T threads, 2^BITS grid cells: <1024, 14> for big scenes; <256, 12> for n <= 4096, where 4096 cells are plenty and a
// workgroup of 4 waves with 18 KB of LDS finds room on a CU that the wide kernels of the pipelined stack occupy
#ifdef EPNET_BQ_STATS  // diagnostic build only (profiles/micro/bq_stats.py): per-wave counters of bq_query2_kernel
__device__ unsigned long long g_bq_stats[16];
#endif
#ifdef EPNET_IX_STATS  // diagnostic build only (profiles/micro/ix_stats.py): phase counters of the index build (wave 0)
__device__ unsigned long long g_ix_stats[8];
#endif

template <int kIxThreads, int BITS>
__global__ __launch_bounds__(kIxThreads) void bq_index_kernel(int n, int np, const float *__restrict__ xyz,
                                                              float4 *__restrict__ sorted, float *__restrict__ boxes,
                                                              float *__restrict__ qboxes, int n_src = 0,
                                                              const int *__restrict__ src_idx = nullptr,
                                                              float *__restrict__ gathered = nullptr) {
    extern __shared__ int s_hist[];  // cell histogram / running offsets, then the staging rows (spatial.h)
    __shared__ float s_box[6][16];
    __shared__ int s_part[16];
    // one workgroup per scene on the sampling chain of a level: beside the wide kernels of the pipelined stack (32 waves of a ball
    // query per CU) its waves would get a ninth of the issue slots -- a 23 us build took 204 us there
    __builtin_amdgcn_s_setprio(3);
#ifdef EPNET_IX_STATS
    unsigned long long *const ix_stats = g_ix_stats;
#else
    unsigned long long *const ix_stats = nullptr;
#endif
    // (the 256-thread kernel stages at most 512 rows: see scene_index_build_block)
    scene_index_build_block<kIxThreads, BITS, 16, kIxThreads == 256 ? 512 : 0, false>(s_hist, s_box, s_part, n, np, xyz, sorted, boxes, qboxes,
                                                                                      n_src, src_idx, gathered, ix_stats);
}

constexpr int kQThreads = 256;

// |clamp(c, box) - c|^2 < r^2, box = (min x, max x, min y, max y, min z, max z)
__device__ __forceinline__ bool box_near(const float *__restrict__ bx, float cx, float cy, float cz, float radius2) {
    const float2 bxx = *reinterpret_cast<const float2 *>(bx), byy = *reinterpret_cast<const float2 *>(bx + 2),
                 bzz = *reinterpret_cast<const float2 *>(bx + 4);
    const float px = __builtin_amdgcn_fmed3f(cx, bxx.x, bxx.y), py = __builtin_amdgcn_fmed3f(cy, byy.x, byy.y),
                pz = __builtin_amdgcn_fmed3f(cz, bzz.x, bzz.y);
    const float dx = cx - px, dy = cy - py, dz = cz - pz;
    return (dx * dx + dy * dy + dz * dz) < radius2;
}

// One wave per centre. Two levels of boxes: the lanes test the quad boxes (256 points each), then -- 16 candidate
// quads at a time -- the 4 bucket boxes of each candidate quad, then the 64 points of every near bucket. A ball holds
// a handful of points (median 1-2 on KITTI-like scenes), so the hits are appended to a 64-entry list and ordered
// by counting; only a ball with more than 64 hits takes a second walk through the N-bit bitmap.
// The K scales of an MSG level (same centres, same points, nested balls) share ONE walk: boxes are tested against
// the largest radius and every distance is computed once.
// DPL = bitmap dwords per lane = np / 2048 (np >= 2048)

// the candidate walk: visit(p, d2) for the 64 points p (one per lane) of every bucket whose box is nearer than r2
template <int DPL, typename F>
__device__ __forceinline__ void bq_walk(int lane, int np, float r2, float cx, float cy, float cz,
                                        const float4 *__restrict__ sorted, const float *__restrict__ boxes,
                                        const float *__restrict__ qboxes, int *quads, F &&visit) {
    // The kernel is bound by its chain of dependent loads (boxes -> boxes -> points), not by arithmetic: the rows of
    // up to 4 near buckets are requested together before any of them is tested.
    auto scan_buckets = [&](unsigned long long cand, auto &&bucket_of) {
        while (cand) {
            float4 p[4];
            int nb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cand) {
                    const int bb = bucket_of((int)__builtin_ctzll(cand));
                    cand &= cand - 1ull;
                    p[k] = sorted[(bb << 6) + lane];
                    nb = k + 1;
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nb) {
                    const float dx = cx - p[k].x, dy = cy - p[k].y, dz = cz - p[k].z;
                    visit(p[k], dx * dx + dy * dy + dz * dz);
                }
        }
    };
    if constexpr (DPL <= 2) {  // <= 64 buckets: one round over the bucket boxes, no second level
        const bool bnear = lane < (np >> 6) && box_near(boxes + lane * 6, cx, cy, cz, r2);
        scan_buckets(__ballot(bnear), [](int l) { return l; });
    } else {
        const int nq = np >> 8;
        for (int q0 = 0; q0 < nq; q0 += 64) {
            const int qd = q0 + lane;
            const bool qnear = qd < nq && box_near(qboxes + qd * 6, cx, cy, cz, r2);
            const unsigned long long qmask = __ballot(qnear);
            if (!qmask) continue;
            const int nqc = (int)__popcll(qmask);
            if (qnear) quads[popc_below(qmask)] = qd;
            __builtin_amdgcn_wave_barrier();
            for (int s0 = 0; s0 < nqc; s0 += 16) {
                const int slot = s0 + (lane >> 2);
                int bid = 0;
                bool bnear = false;
                if (slot < nqc) {
                    bid = quads[slot] * 4 + (lane & 3);
                    bnear = box_near(boxes + bid * 6, cx, cy, cz, r2);
                }
                scan_buckets(__ballot(bnear), [&](int l) { return __builtin_amdgcn_readlane(bid, l); });
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// <= 64 hits in `hits`: order them by original index (rank = number of smaller indices; they are distinct) and write
// "the first nsample in index order, padded with the first" (ball_query_gpu.cu:29-43); an empty ball is all zeros
__device__ __forceinline__ void bq_emit_list(int lane, const int *hits, int cnt, int nsample, int *__restrict__ out) {
    __builtin_amdgcn_wave_barrier();
    const int mine = lane < cnt ? hits[lane] : 0x7fffffff;
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += __builtin_amdgcn_readlane(mine, j) < mine ? 1 : 0;
    if (lane < cnt && rank < nsample) out[rank] = mine;
    int first = 0;
    if (cnt) first = __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(__ballot(lane < cnt && rank == 0)));
    for (int l = cnt + lane; l < nsample; l += 64) out[l] = first;
}

// ---- shared lists: the two scales of an MSG level (nested balls) keep ONE list per centre ----
// An entry is (original index << 1) | (also inside the smaller ball): the indices are distinct, so the entries order as their
// indices do, and the low bit says which of them the smaller scale wants.

// one centre, <= 64 entries in `hits`: both scales from one rank loop (the path of an odd list length above the pair bound)
__device__ __forceinline__ void bq_emit_shared(int lane, const int *hits, int cnt, int ns_big, int ns_small, int *__restrict__ out_big,
                                               int *__restrict__ out_small) {
    __builtin_amdgcn_wave_barrier();
    const bool valid = lane < cnt;
    const int mine = valid ? hits[lane] : 0x7fffffff;
    int rank = 0, rin = 0;   // smaller entries among all / among the inner ones
    for (int j = 0; j < cnt; ++j) {
        const int v = __builtin_amdgcn_readlane(mine, j);
        rank += v < mine ? 1 : 0;
        rin += v < mine ? (v & 1) : 0;
    }
    const bool inner = valid && (mine & 1);
    if (valid && rank < ns_big) out_big[rank] = mine >> 1;
    if (inner && rin < ns_small) out_small[rin] = mine >> 1;
    int first = 0;
    if (cnt) first = __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(__ballot(valid && rank == 0))) >> 1;
    for (int l = cnt + lane; l < ns_big; l += 64) out_big[l] = first;
    const unsigned long long im = __ballot(inner);
    const int cin = (int)__popcll(im);
    first = 0;
    if (cin) first = __builtin_amdgcn_readlane(mine, (int)__builtin_ctzll(__ballot(inner && rin == 0))) >> 1;
    for (int l = cin + lane; l < ns_small; l += 64) out_small[l] = first;
}

// the rows of one scale for the two centres of a wave from their ordered lists ord[2][32] (c0, c1 <= 32 entries): slot s of a row
// is entry s, beyond the list entry 0, of an empty ball 0 (ball_query_gpu.cu:29-43) -- the READING lane pads. NS = 16: both rows
// in one half wave; otherwise centre 0 in lanes 0-31 and centre 1 in lanes 32-63 (NS = 32: the whole wave stores). NS = 0: run-time ns.
template <int NS>
__device__ __forceinline__ void bq_store_rows(int lane, bool two, const int *ord, int c0, int c1, int ns_rt, int *__restrict__ row0,
                                              int *__restrict__ row1) {
    const int ns = NS ? NS : ns_rt;
    if (NS == 16 && lane >= 32) return;
    const int e = NS == 16 ? lane >> 4 : lane >> 5, s = NS == 16 ? lane & 15 : lane & 31;
    const int c = e ? c1 : c0;
    int v = ord[e * 32 + (s < c ? s : 0)];
    v = c ? v : 0;
    // (one masked store per row from its scalar base: selecting a 64-bit row address per lane costs more vector instructions)
    if (e == 0) {
        if (s < ns) row0[s] = v;
    } else if (two) {   // an odd tail has no second row
        if (s < ns) row1[s] = v;
    }
    if (NS == 0 && ns > 32 && (e == 0 || two)) {   // (beyond the 32 entries of this path: padding only)
        int *row = e ? row1 : row0;
        const int first = c ? ord[e * 32] : 0;
        for (int l = s + 32; l < ns; l += 32) row[l] = first;
    }
}

// ONE emission pass for the two centres of a wave, both lists at or below 32 entries: centre 0's list in lanes 0-31, centre 1's
// in lanes 32-63; one loop over the entries of the own half (broadcast LDS reads, four entries each) gives every entry its rank
// among all and among the inner entries of its list; the ordered lists go back through LDS and leave as one store per row.
// lists: 256 words, 16-byte aligned -- [0, 128) the two lists (64 apart), [128, 256) the ordered copies.
template <int NSB, int NSS>
__device__ __forceinline__ void bq_emit_pair(int lane, bool two, int *lists, int c0, int c1, int ns_big, int ns_small,
                                             int *__restrict__ big0, int *__restrict__ big1, int *__restrict__ small0,
                                             int *__restrict__ small1) {
    const int half = lane >> 5, sl = lane & 31;
    const int c = half ? c1 : c0;
    int *raw = lists + half * 64;
    const bool valid = sl < c;
    __builtin_amdgcn_wave_barrier();
    int mine = raw[sl];
    if (!valid) {   // the loop below reads whole groups of four
        mine = 0x7fffffff;
        raw[sl] = mine;
    }
    __builtin_amdgcn_wave_barrier();
    int rank = 0, rin = 0;
    const int nmax = max(c0, c1);
#pragma unroll 1
    for (int j = 0; j < nmax; j += 4) {
        const int4 v = *reinterpret_cast<const int4 *>(raw + j);
        rank += (v.x < mine ? 1 : 0) + (v.y < mine ? 1 : 0) + (v.z < mine ? 1 : 0) + (v.w < mine ? 1 : 0);
        rin += (v.x < mine ? v.x & 1 : 0) + (v.y < mine ? v.y & 1 : 0) + (v.z < mine ? v.z & 1 : 0) + (v.w < mine ? v.w & 1 : 0);
    }
    const bool inner = valid && (mine & 1);
    if (valid) lists[128 + half * 32 + rank] = mine >> 1;
    if (inner) lists[192 + half * 32 + rin] = mine >> 1;
    const unsigned long long im = __ballot(inner);
    __builtin_amdgcn_wave_barrier();
    bq_store_rows<NSB>(lane, two, lists + 128, c0, c1, ns_big, big0, big1);
    bq_store_rows<NSS>(lane, two, lists + 192, (int)__popc((unsigned)im), (int)__popc((unsigned)(im >> 32)), ns_small, small0, small1);
}

// 64 < cnt <= 64 * RM hits in `hits`, nsample <= 64: only the nsample SMALLEST original indices are wanted. They are found
// without a second walk: the indices are distinct integers below np, so count(hits < T) grows by at most one per unit of T and a
// binary search over T finds the threshold below which exactly nsample of them lie (the lanes hold the list in RM registers; a
// count is RM ballots); those are compacted to the head of the list, which bq_emit_list then orders.
template <int RM>
__device__ __forceinline__ int bq_select_smallest(int lane, int *hits, int cnt, int nsample, int np) {
    __builtin_amdgcn_wave_barrier();
    int key[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) key[r] = (r * 64 < cnt && r * 64 + lane < cnt) ? hits[r * 64 + lane] : 0x7fffffff;
    int lo = 0, hi = np;   // count(hits < lo) < nsample <= count(hits < hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        int c = 0;
#pragma unroll
        for (int r = 0; r < RM; ++r)
            if (r * 64 < cnt) c += (int)__popcll(__ballot(key[r] < mid));
        if (c >= nsample) hi = mid;
        else lo = mid;
    }
    __builtin_amdgcn_wave_barrier();
    int base = 0;
#pragma unroll
    for (int r = 0; r < RM; ++r)
        if (r * 64 < cnt) {
            const bool sel = key[r] < hi;
            const unsigned long long sm = __ballot(sel);
            if (sel) hits[base + popc_below(sm)] = key[r];
            base += (int)__popcll(sm);
        }
    return hi;   // every kept index is below, every dropped one at or above
}

// a crowded ball: every hit sets bit `original index` of an N-bit bitmap, which is then read back in order
template <int DPL>
__device__ __forceinline__ void bq_bitmap_search(int lane, int np, float r2, int nsample, float cx, float cy, float cz,
                                                 const float4 *__restrict__ sorted, const float *__restrict__ boxes,
                                                 const float *__restrict__ qboxes, int *__restrict__ out, unsigned *bits,
                                                 int *quads) {
#pragma unroll
    for (int w = 0; w < DPL; ++w) bits[lane * DPL + w] = 0u;
    __builtin_amdgcn_wave_barrier();
    bq_walk<DPL>(lane, np, r2, cx, cy, cz, sorted, boxes, qboxes, quads, [&](const float4 &p, float d2) {
        if (d2 < r2) {
            const int k = __float_as_int(p.w);
            atomicOr(&bits[k >> 5], 1u << (k & 31));
        }
    });
    __builtin_amdgcn_wave_barrier();
    // lane l owns bits [l*32*DPL, (l+1)*32*DPL)
    int bc = 0;
#pragma unroll 8
    for (int i = 0; i < DPL; ++i) bc += __popc(bits[lane * DPL + i]);
    const int incl = wave_inclusive_scan(bc);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    int pos = incl - bc;
    int mine_first = 0x7fffffff;
    if (bc > 0 && (pos < nsample || pos == 0)) {
#pragma unroll 1   // (unrolled, the (lane * DPL + i) * 32 of every copy of this walk in a kernel stay in registers over its common path)
        for (int i = 0; i < DPL; ++i) {
            unsigned ww = bits[lane * DPL + i];
            if (ww && mine_first == 0x7fffffff) mine_first = (lane * DPL + i) * 32 + (int)__builtin_ctz(ww);
            while (ww && pos < nsample) {
                const int bit = (int)__builtin_ctz(ww);
                ww &= ww - 1u;
                out[pos++] = (lane * DPL + i) * 32 + bit;
            }
            if (pos >= nsample) break;
        }
    }
    const unsigned long long have = __ballot(bc > 0);
    int first = 0;
    if (have) first = __builtin_amdgcn_readlane(mine_first, (int)__builtin_ctzll(have));
    for (int l = total + lane; l < nsample; l += 64) out[l] = first;
}

template <int K>
struct BqScales {
    float r2[K];   // radius * radius (ball_query_gpu.cu:23)
    int nsample[K];
    int *idx[K];   // (B, M, nsample[k])
};

// order (or NULL) / npc: the scene index of the CENTRES (npc entries per scene, the m real ones first): wave w then serves the
// w-th centre in that spatial order instead of centre w -- consecutive waves walk the same quads, buckets and rows, which are
// still in the CU's L1 / the XCD's L2 from the neighbour (FPS order scatters consecutive centres over the whole scene)
template <int DPL, int K>
__global__ __launch_bounds__(kQThreads) void bq_query_kernel(int np, int m, BqScales<K> sc,
                                                             const float *__restrict__ new_xyz,
                                                             const float4 *__restrict__ sorted,
                                                             const float *__restrict__ boxes,
                                                             const float *__restrict__ qboxes,
                                                             const float4 *__restrict__ order, int npc) {
    __shared__ unsigned s_bits[kQThreads / 64][64 * DPL];
    __shared__ int s_quads[kQThreads / 64][64];
    __shared__ int s_hits[kQThreads / 64][K][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int wg_x, bs;
    xcd_scene_map(wg_x, bs);   // a scene's index passes through one XCD's L2
    int ci = wg_x * (kQThreads / 64) + wave;
    if (ci >= m) return;  // wave-uniform; no block-level barrier below
    sorted += (size_t)bs * np;
    boxes += (size_t)bs * (np / 64) * 6;
    qboxes += (size_t)bs * (np / 256) * 6;
    float cx, cy, cz;
    if (order) {
        const float4 e = order[(size_t)bs * npc + ci];
        ci = __float_as_int(e.w);
        cx = e.x; cy = e.y; cz = e.z;
    } else {
        const float *c = new_xyz + ((size_t)bs * m + ci) * 3;
        cx = c[0]; cy = c[1]; cz = c[2];
    }
    float r2max = sc.r2[0];
#pragma unroll
    for (int k = 1; k < K; ++k) r2max = fmaxf(r2max, sc.r2[k]);
    int cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 0;
    bq_walk<DPL>(lane, np, r2max, cx, cy, cz, sorted, boxes, qboxes, s_quads[wave], [&](const float4 &p, float d2) {
        if (!__ballot(d2 < r2max)) return;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool hit = d2 < sc.r2[k];
            const unsigned long long hm = __ballot(hit);
            if (hm) {
                const int pos = cnt[k] + popc_below(hm);
                if (hit && pos < 64) s_hits[wave][k][pos] = __float_as_int(p.w);
                cnt[k] += (int)__popcll(hm);
            }
        }
    });
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int *out = sc.idx[k] + ((size_t)bs * m + ci) * sc.nsample[k];
        if (cnt[k] <= 64)
            bq_emit_list(lane, s_hits[wave][k], cnt[k], sc.nsample[k], out);
        else
            bq_bitmap_search<DPL>(lane, np, sc.r2[k], sc.nsample[k], cx, cy, cz, sorted, boxes, qboxes, out, s_bits[wave],
                                  s_quads[wave]);
    }
}

// xcd_scene_map in scalar registers, and for a power-of-two grid (every level of the pyramid) without its division: ~25 vector
// instructions, several of them quarter-rate, at the head of a kernel that is bound by the vector instructions it issues
__device__ __forceinline__ void xcd_scene_map_uniform(int &wg_x, int &bs) {
#ifndef EPNET_NO_XCD_MAP
    const int gx = (int)gridDim.x;
    if ((gx & (gx - 1)) == 0) {
        const int nwg = gx * (int)gridDim.y, orig = (int)blockIdx.y * gx + (int)blockIdx.x;
        const int xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
        const int wgid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
        bs = wgid >> __builtin_ctz(gx);
        wg_x = wgid & (gx - 1);
        return;
    }
#endif
    xcd_scene_map(wg_x, bs);
    wg_x = __builtin_amdgcn_readfirstlane(wg_x);
    bs = __builtin_amdgcn_readfirstlane(bs);
}

// TWO centres per wave. The search is a chain of dependent loads (quad boxes -> bucket boxes -> rows) and the chip
// holds at most 8 waves per SIMD, so a wave that walks the chain for two centres at once -- quad boxes loaded once
// and tested against both, the bucket boxes of centre 0 in lanes 0-31 and of centre 1 in lanes 32-63, one candidate
// row of each per step -- halves the latency per centre. Same results as bq_query_kernel.
// kStream (every nsample <= 64; the launcher takes it for scenes of more than 16384 points): no bitmap. A list that runs full
// during the walk is cut down to its nsample smallest indices on the spot and from then on only takes hits below the threshold
// of that cut (nothing at or above it can be among the first nsample in index order): ONE walk however crowded the ball, and
// 4 KB of LDS per wave instead of the N-bit bitmap's 8 KB at 65536 points, which held the kernel at half the waves a CU can
// keep (the walk is a chain of dependent loads: 0.54 -> 0.32 ms at 32 scenes of BASELINE config 5). The lists are looked at once
// per step of the walk (<= kRowsPerStep rows = kStepAppends appends per list).
// K == 2 without kStream: ONE list per centre for both scales (see "shared lists" above): the balls are nested, so a hit is
// appended once, with a bit for the smaller ball, and the four lists of a wave leave in one emission pass while both centres
// hold at most 32 hits. A centre above 64 hits takes the bitmap walk for both of its scales (its list has dropped entries the
// smaller scale may want as well). kStream keeps one list per scale: its cut threshold is per scale. kSpec: nsample = (16, 32)
// with r2[0] <= r2[1], the pyramid's pair, as compile-time constants.
template <int DPL, int K, bool kStream, bool kSpec = false>
__global__ __launch_bounds__(kQThreads) void bq_query2_kernel(int np, int m, BqScales<K> sc,
                                                              const float *__restrict__ new_xyz,
                                                              const float4 *__restrict__ sorted,
                                                              const float *__restrict__ boxes,
                                                              const float *__restrict__ qboxes,
                                                              const float4 *__restrict__ order, int npc) {
    constexpr int kRowsPerStep = 2;   // candidate rows of each centre per step of the walk (scan_pairs: p0, p2 | p1, p3)
    constexpr int CAP = kStream ? (K == 1 ? 512 : 256) : 64, kStepAppends = kRowsPerStep * 64;
    static_assert(CAP % 64 == 0, "the lists are selected and emitted in whole waves");
    static_assert(!kStream || CAP - kStepAppends >= 64,
                  "a cut list keeps nsample <= 64 entries (the launcher streams for nsample <= 64 only) and must take a step's appends");
    constexpr int kBitWords = kStream ? 0 : 64 * DPL;
    constexpr bool kShared = K == 2 && !kStream;
    static_assert(!kSpec || kShared, "the compile-time pair is one of the shared-list kernel");
    __shared__ __attribute__((aligned(16))) unsigned s_pool[kQThreads / 64][kBitWords + 2 * K * CAP];   // (the bitmap of a crowded ball,) the hit lists
    __shared__ int s_quads[kQThreads / 64][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int wg_x, bs;
    xcd_scene_map_uniform(wg_x, bs);   // a scene's index passes through one XCD's L2
    const int ci0 = (wg_x * (kQThreads / 64) + wave) * 2;
    if (ci0 >= m) return;  // wave-uniform; no block-level barrier below
    const bool two = ci0 + 1 < m;
    sorted += (size_t)bs * np;
    boxes += (size_t)bs * (np / 64) * 6;
    qboxes += (size_t)bs * (np / 256) * 6;
    float ax, ay, az, bx_, by_, bz_;
    int out0 = ci0, out1 = ci0 + 1;   // the rows of idx the two centres write
    if (order) {   // the two neighbours in the centres' spatial order (see bq_query_kernel): they mostly want the same rows
        const float4 e0 = order[(size_t)bs * npc + ci0], e1 = order[(size_t)bs * npc + ci0 + (two ? 1 : 0)];
        ax = e0.x; ay = e0.y; az = e0.z;
        bx_ = e1.x; by_ = e1.y; bz_ = e1.z;
        out0 = __float_as_int(e0.w);
        out1 = __float_as_int(e1.w);
    } else {
        const float *c0 = new_xyz + ((size_t)bs * m + ci0) * 3;
        const float *c1 = two ? c0 + 3 : c0;  // an odd tail repeats centre 0 (its second copy is never written)
        ax = c0[0]; ay = c0[1]; az = c0[2];
        bx_ = c1[0]; by_ = c1[1]; bz_ = c1[2];
    }
    // wave-uniform, but loaded per lane: into scalar registers (the kernel stays at or below 48 VGPRs -- eight waves of it then
    // leave 128 registers of every SIMD to the sampling chain's kernels it runs beside, which need 126)
    auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    ax = uniform(ax); ay = uniform(ay); az = uniform(az);
    bx_ = uniform(bx_); by_ = uniform(by_); bz_ = uniform(bz_);
    out0 = __builtin_amdgcn_readfirstlane(out0);
    out1 = __builtin_amdgcn_readfirstlane(out1);
    const int half = lane >> 5;  // which centre this lane serves in the bucket-box stage
    const float hx = half ? bx_ : ax, hy = half ? by_ : ay, hz = half ? bz_ : az;
    float r2max = sc.r2[0];
#pragma unroll
    for (int k = 1; k < K; ++k) r2max = fmaxf(r2max, sc.r2[k]);
    // (kShared) which scale is the larger ball: by r2, whichever order the caller passed (a NaN radius is an empty ball: the smaller)
    const bool big1 = kSpec || (kShared && (sc.r2[K - 1] >= sc.r2[0] || sc.r2[0] != sc.r2[0]));
    const float r2small = kShared ? (big1 ? sc.r2[0] : sc.r2[K - 1]) : r2max;
    if constexpr (kShared) r2max = big1 ? sc.r2[K - 1] : sc.r2[0];
    int cnt[2][K];    // hits so far (kStream: entries in the list; kShared: [e][0] only)
    int below[2][K];  // (kStream) the list only takes original indices below this
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            cnt[e][k] = 0;
            below[e][k] = 0x7fffffff;
        }
    int *hits_of = reinterpret_cast<int *>(s_pool[wave]) + kBitWords;
#ifdef EPNET_BQ_STATS
    const unsigned long long st_0 = __builtin_amdgcn_s_memtime();
    unsigned st_rows = 0;
    bool st_sel = false, st_again = false;
#endif

    auto visit = [&](int e, const float4 &p) {  // e is compile-time at the call sites
#ifdef EPNET_BQ_STATS
        ++st_rows;
#endif
        const float cx = e ? bx_ : ax, cy = e ? by_ : ay, cz = e ? bz_ : az;
        const float dx = cx - p.x, dy = cy - p.y, dz = cz - p.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        if constexpr (kShared) {
            const bool hit = d2 < r2max;
            const unsigned long long hm = __ballot(hit);
            if (!hm) return;
            const int pos = cnt[e][0] + popc_below(hm);
            if (hit && pos < 64) hits_of[e * 64 + pos] = (__float_as_int(p.w) << 1) | (d2 < r2small ? 1 : 0);
            cnt[e][0] += (int)__popcll(hm);
            return;
        }
        if (!__ballot(d2 < r2max)) return;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool hit = d2 < sc.r2[k] && (!kStream || __float_as_int(p.w) < below[e][k]);
            const unsigned long long hm = __ballot(hit);
            if (hm) {
                const int pos = cnt[e][k] + popc_below(hm);
                if (hit && pos < CAP) hits_of[(e * K + k) * CAP + pos] = __float_as_int(p.w);
                cnt[e][k] += (int)__popcll(hm);
            }
        }
    };
    // (kStream) between two steps of the walk: room for the next step's appends in every list
    auto make_room = [&]() {
        if constexpr (kStream) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (cnt[e][k] > CAP - kStepAppends) {
                        below[e][k] = bq_select_smallest<CAP / 64>(lane, hits_of + (e * K + k) * CAP, cnt[e][k], sc.nsample[k], np);
                        cnt[e][k] = sc.nsample[k];
#ifdef EPNET_BQ_STATS
                        st_sel = true;
#endif
                    }
        }
    };
    // one candidate row of each centre per step (both loads in flight together); bucket_of(e, bit)
    // lane's point of a bucket: the bucket is wave-uniform, so the row's base stays in scalar registers and the lane adds its 16 bytes
    auto row_of = [&](int bucket) { return (sorted + ((size_t)(unsigned)bucket << 6))[(unsigned)lane]; };
    auto scan_pairs = [&](unsigned long long cand0, unsigned long long cand1, auto &&bucket_of) {
        static_assert(kRowsPerStep == 2, "the step below loads two rows of each centre");
        while (cand0 | cand1) {
            make_room();
            // (no initial values: with a constant on the other edge the compiler folds what visit() first does to a row into the block
            // of its load, behind a wait for that load alone, and the four rows of a step arrive one after the other)
            float4 p0, p1, p2, p3;
            const bool h0 = cand0 != 0ull, h1 = cand1 != 0ull;
            if (h0) { p0 = row_of(bucket_of(0, (int)__builtin_ctzll(cand0))); cand0 &= cand0 - 1ull; }
            if (h1) { p1 = row_of(bucket_of(1, (int)__builtin_ctzll(cand1))); cand1 &= cand1 - 1ull; }
            const bool h2 = cand0 != 0ull, h3 = cand1 != 0ull;
            if (h2) { p2 = row_of(bucket_of(0, (int)__builtin_ctzll(cand0))); cand0 &= cand0 - 1ull; }
            if (h3) { p3 = row_of(bucket_of(1, (int)__builtin_ctzll(cand1))); cand1 &= cand1 - 1ull; }
            if (h0) visit(0, p0);
            if (h1) visit(1, p1);
            if (h2) visit(0, p2);
            if (h3) visit(1, p3);
            // every row of the step has arrived by now; saying so (s_waitcnt vmcnt(0)) keeps the compiler from assuming, on the way
            // round the loop, a load still in flight into p0 .. p3 and waiting before it reuses their registers for the next addresses
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
    };
    if constexpr (DPL <= 2) {  // <= 64 buckets: every bucket box once, tested against both centres
        bool n0 = false, n1 = false;
        if (lane < (np >> 6)) {
            n0 = box_near(boxes + lane * 6, ax, ay, az, r2max);
            n1 = box_near(boxes + lane * 6, bx_, by_, bz_, r2max);
        }
        scan_pairs(__ballot(n0), __ballot(n1), [](int, int bit) { return bit; });
    } else {
        const int nq = np >> 8;
        // every word of the two quad lists is a quad of this scene from here on (see the bucket-box pass)
        s_quads[wave][0][lane] = 0;
        s_quads[wave][1][lane] = 0;
        for (int q0 = 0; q0 < nq; q0 += 64) {
            const int qd = q0 + lane;
            // (a lane past the last quad tests the last one again and drops the answer: no branch around the loads, and the ballots
            // come straight from the compares; 24-bit multiplies: full rate)
            const float *qb = qboxes + __umul24(min(qd, nq - 1), 6);
            const bool n0 = box_near(qb, ax, ay, az, r2max) && qd < nq, n1 = box_near(qb, bx_, by_, bz_, r2max) && qd < nq;
            const unsigned long long qm0 = __builtin_amdgcn_ballot_w64(n0), qm1 = __builtin_amdgcn_ballot_w64(n1);   // (of a bool: no 0 / 1 round trip)
            if (!(qm0 | qm1)) continue;
            const int nq0 = (int)__popcll(qm0), nq1 = (int)__popcll(qm1);
            if (n0) s_quads[wave][0][popc_below(qm0)] = qd;
            if (n1) s_quads[wave][1][popc_below(qm1)] = qd;
            __builtin_amdgcn_wave_barrier();
            const int nmine = half ? nq1 : nq0;
            for (int s0 = 0; s0 < max(nq0, nq1); s0 += 8) {  // 8 candidate quads of each centre per round
                const int slot = s0 + ((lane & 31) >> 2);
                // no branch around the loads, and the ballot straight from the compare: a lane past its centre's list reads the list's
                // last entry again (one address for all of them) and drops the answer. The unsigned minimum leaves `slot` itself for
                // an EMPTY list -- a word of the list that holds a quad of this scene all the same: zero, or what an earlier round of
                // the walk left (the lists are initialised above)
                const unsigned sl = min((unsigned)slot, (unsigned)(nmine - 1));
                const int bid = s_quads[wave][half][sl] * 4 + (lane & 3);
                // (two ballots, each of its compare, and a scalar AND: the ballot of `near && mine` goes through a 0 / 1 register)
                const unsigned long long cand = __builtin_amdgcn_ballot_w64(box_near(boxes + __umul24(bid, 6), hx, hy, hz, r2max)) &
                                                __builtin_amdgcn_ballot_w64(slot < nmine);
                scan_pairs(cand & 0xFFFFFFFFull, cand >> 32,
                           [&](int e, int bit) { return __builtin_amdgcn_readlane(bid, bit + 32 * e); });
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
#ifdef EPNET_BQ_STATS
    const unsigned long long st_1 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (kShared) {
        const int ns0 = kSpec ? 16 : sc.nsample[0], ns1 = kSpec ? 32 : sc.nsample[K - 1];
        const int ns_big = big1 ? ns1 : ns0, ns_small = big1 ? ns0 : ns1;
        int *idx_big = big1 ? sc.idx[K - 1] : sc.idx[0], *idx_small = big1 ? sc.idx[0] : sc.idx[K - 1];
        const size_t row0 = (size_t)bs * m + out0, row1 = (size_t)bs * m + out1;
        const int c0 = cnt[0][0], c1 = cnt[1][0];
        if (c0 <= 32 && c1 <= 32) {   // (wave-uniform) the common path; an odd tail walked centre 0 twice and stores one row
            bq_emit_pair<kSpec ? 32 : 0, kSpec ? 16 : 0>(lane, two, hits_of, c0, c1, ns_big, ns_small, idx_big + row0 * ns_big,
                                                         idx_big + row1 * ns_big, idx_small + row0 * ns_small, idx_small + row1 * ns_small);
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (e == 1 && !two) break;
                const size_t row = e ? row1 : row0;
                if (cnt[e][0] <= 64) {
                    bq_emit_shared(lane, hits_of + e * 64, cnt[e][0], ns_big, ns_small, idx_big + row * ns_big, idx_small + row * ns_small);
                } else {
#ifdef EPNET_BQ_STATS
                    st_again = true;
#endif
                    const float cx = e ? bx_ : ax, cy = e ? by_ : ay, cz = e ? bz_ : az;
                    bq_bitmap_search<DPL>(lane, np, r2max, ns_big, cx, cy, cz, sorted, boxes, qboxes, idx_big + row * ns_big, s_pool[wave],
                                          s_quads[wave][0]);
                    bq_bitmap_search<DPL>(lane, np, r2small, ns_small, cx, cy, cz, sorted, boxes, qboxes, idx_small + row * ns_small,
                                          s_pool[wave], s_quads[wave][0]);
                }
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && !two) break;
            const float cx = e ? bx_ : ax, cy = e ? by_ : ay, cz = e ? bz_ : az;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                int *out = sc.idx[k] + ((size_t)bs * m + (e ? out1 : out0)) * sc.nsample[k];
                int *hits = hits_of + (e * K + k) * CAP;
                if constexpr (kStream) {
                    if (cnt[e][k] > 64) {   // (a list that was cut before holds nsample or more candidates: the same selection)
                        bq_select_smallest<CAP / 64>(lane, hits, cnt[e][k], sc.nsample[k], np);
                        cnt[e][k] = sc.nsample[k];
#ifdef EPNET_BQ_STATS
                        st_sel = true;
#endif
                    }
                    bq_emit_list(lane, hits, cnt[e][k], sc.nsample[k], out);
                } else {
                    if (cnt[e][k] <= 64) {
                        bq_emit_list(lane, hits, cnt[e][k], sc.nsample[k], out);
                    } else {
#ifdef EPNET_BQ_STATS
                        st_again = true;
#endif
                        bq_bitmap_search<DPL>(lane, np, sc.r2[k], sc.nsample[k], cx, cy, cz, sorted, boxes, qboxes, out, s_pool[wave],
                                              s_quads[wave][0]);
                    }
                }
            }
        }
    }
#ifdef EPNET_BQ_STATS
    {
        const unsigned long long st_3 = __builtin_amdgcn_s_memtime();
        if (lane == 0) {
            const int o = st_again ? 8 : (st_sel ? 4 : 0);   // plain waves / waves that selected / waves that walked again
            atomicAdd(&g_bq_stats[o + 0], 1ull);
            atomicAdd(&g_bq_stats[o + 1], st_1 - st_0);
            atomicAdd(&g_bq_stats[o + 2], st_3 - st_1);
            atomicAdd(&g_bq_stats[o + 3], (unsigned long long)st_rows);
            atomicMax(&g_bq_stats[12], st_3 - st_0);
        }
    }
#endif
}

}  // namespace epnet

using namespace epnet;

extern "C" int epnet_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                                const float *xyz, int *idx, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && n >= 0 && m >= 0 && nsample >= 0);
    if (b == 0 || m == 0 || nsample == 0) return EPNET_OK;
    EPNET_REQUIRE(new_xyz && xyz && idx);
    EPNET_REQUIRE(b <= 65535);
    const float radius2 = radius * radius;  // ball_query_gpu.cu:23
    hipStream_t s = (hipStream_t)stream;
    constexpr int waves = kBqThreads / 64;
    // few centres: one per wave so that the grid still covers the chip; many: two per wave to
    // halve the LDS reads per pair test
    if ((long long)m * b >= 8192) {
        dim3 grid(div_up(m, waves * 2), b);
        hipLaunchKernelGGL(ball_query_kernel<2>, grid, dim3(kBqThreads), 0, s, n, m, radius2, nsample, new_xyz, xyz, idx);
    } else {
        dim3 grid(div_up(m, waves), b);
        hipLaunchKernelGGL(ball_query_kernel<1>, grid, dim3(kBqThreads), 0, s, n, m, radius2, nsample, new_xyz, xyz, idx);
    }
    return check_launch("ball_query");
}


// shared with three_nn (interpolate.hip): cell-sorted float4 copy (x, y, z, original index) of n points padded
// to np (a multiple of 64) per scene, plus one box (6 floats) per 64 sorted points
int epnet::spatial_index_launch(int b, int n, int np, const float *xyz, float4 *sorted, float *boxes, float *qboxes,
                                hipStream_t s, int n_src, const int *src_idx, float *gathered) {
    if (n <= 4096) {
        constexpr int T = 256, cells = 1 << 12;
        // (+ the staging buffer of a quarter of the sorted scene, at most 512 points = 8 KB here; 64 KB below)
        const size_t stage = (np & 255) == 0 ? (size_t)(np / 4 < 512 ? np / 4 : 512) * sizeof(float4) : 0;
        hipLaunchKernelGGL((bq_index_kernel<T, 12>), dim3(b), dim3(T), (size_t)(cells + cells / (cells / T) + 64) * sizeof(int) + stage, s,
                           n, np, xyz, sorted, boxes, qboxes, n_src, src_idx, gathered);
    } else {
        constexpr int T = 1024, cells = 1 << 14;
        const size_t stage = (n <= T * 16 && (np & 255) == 0) ? (size_t)(np / 4) * sizeof(float4) : 0;   // (bigger scenes scatter straight to global memory)
        hipLaunchKernelGGL((bq_index_kernel<T, 14>), dim3(b), dim3(T), (size_t)(cells + cells / (cells / T) + 64) * sizeof(int) + stage, s,
                           n, np, xyz, sorted, boxes, qboxes, n_src, src_idx, gathered);
    }
    return check_launch("spatial index");
}

template <int K>
static int bq_query_launch(int b, int np, int m, const BqScales<K> &sc, const float *new_xyz, const float4 *sorted,
                           hipStream_t s, const float4 *order = nullptr, int npc = 0) {
    const float *boxes = (const float *)(sorted + (size_t)b * np);
    const float *qboxes = boxes + (size_t)b * (np / 64) * 6;
    // enough centres to fill the chip: two per wave (half the latency per centre); EPNET_BQ_PAIR=0/1 forces either
    const int pair_force = tuning(kBqPair);
    const bool pair = pair_force >= 0 ? pair_force != 0 : (long long)b * m >= 65536;
    if (pair) {
        dim3 grid(div_up(div_up(m, 2), kQThreads / 64), b);
        // streaming lists instead of the bitmap (see the kernel): where the bitmap costs occupancy, i.e. above 16384 points;
        // EPNET_BQ_STREAM=0/1 forces either (nsample <= 64 is a precondition of the streaming variant)
        const int stream_force = tuning(kBqStream);
        bool stream = stream_force >= 0 ? stream_force != 0 : np > 16384;
        for (int k = 0; k < K; ++k) stream = stream && sc.nsample[k] <= 64;
        // the pyramid's pair of scales with its sample counts as compile-time constants (see the kernel)
        const bool spec = K == 2 && !stream && sc.nsample[0] == 16 && sc.nsample[K - 1] == 32 && sc.r2[0] <= sc.r2[K - 1];
#define EPNET_BQ2(D_)                                                                                                                   \
    do {                                                                                                                                \
        if (stream)                                                                                                                     \
            hipLaunchKernelGGL((bq_query2_kernel<D_, K, true>), grid, dim3(kQThreads), 0, s, np, m, sc, new_xyz, sorted, boxes, qboxes,   \
                               order, npc);                                                                                             \
        else if (spec)                                                                                                                  \
            hipLaunchKernelGGL((bq_query2_kernel<D_, K, false, K == 2>), grid, dim3(kQThreads), 0, s, np, m, sc, new_xyz, sorted, boxes, \
                               qboxes, order, npc);                                                                                     \
        else                                                                                                                            \
            hipLaunchKernelGGL((bq_query2_kernel<D_, K, false>), grid, dim3(kQThreads), 0, s, np, m, sc, new_xyz, sorted, boxes,         \
                               qboxes, order, npc);                                                                                     \
    } while (0)
        switch (np / 2048) {
            case 1: EPNET_BQ2(1); break;
            case 2: EPNET_BQ2(2); break;
            case 4: EPNET_BQ2(4); break;
            case 8: EPNET_BQ2(8); break;
            case 16: EPNET_BQ2(16); break;
            default: EPNET_BQ2(32); break;
        }
#undef EPNET_BQ2
        return check_launch("ball_query query");
    }
    dim3 grid(div_up(m, kQThreads / 64), b);
#define EPNET_BQ(D_) hipLaunchKernelGGL((bq_query_kernel<D_, K>), grid, dim3(kQThreads), 0, s, np, m, sc, new_xyz, sorted, boxes, qboxes, order, npc)
    switch (np / 2048) {
        case 1: EPNET_BQ(1); break;
        case 2: EPNET_BQ(2); break;
        case 4: EPNET_BQ(4); break;
        case 8: EPNET_BQ(8); break;
        case 16: EPNET_BQ(16); break;
        default: EPNET_BQ(32); break;
    }
#undef EPNET_BQ
    return check_launch("ball_query query");
}

extern "C" size_t epnet_scene_index_bytes(int b, int n) { return scene_index_bytes(b, n); }

extern "C" int epnet_scene_index_build(int b, int n, const float *xyz, void *index, size_t index_bytes,
                                       epnet_stream_t stream) {
    const size_t need = scene_index_bytes(b, n);
    EPNET_REQUIRE(need != 0 && xyz && index);
    if (index_bytes < need) return EPNET_ENOMEM;
    if (((uintptr_t)index & 15) != 0) return EPNET_EINVAL;
    EPNET_REQUIRE(b <= 65535);
    const int np = scene_index_np(n);
    float4 *sorted = (float4 *)index;
    float *boxes = (float *)(sorted + (size_t)b * np);
    return spatial_index_launch(b, n, np, xyz, sorted, boxes, boxes + (size_t)b * (np / 64) * 6, (hipStream_t)stream);
}

// the scene index of the n points xyz_src[idx[0 .. n)] of every scene (rows of a cloud of n_src points: the centres a sampling has
// just picked), which are written to `gathered` (b, n, 3) in that order as well: gather_points + epnet_scene_index_build of an SA
// level's centres in one dispatch. 1024 <= n <= 16384.
extern "C" int epnet_scene_index_build_gathered(int b, int n_src, int n, const float *xyz_src, const int *idx, float *gathered,
                                                void *index, size_t index_bytes, epnet_stream_t stream) {
    const size_t need = scene_index_bytes(b, n);
    EPNET_REQUIRE(need != 0 && n <= 16384 && n_src >= 1 && xyz_src && idx && gathered && index);
    if (index_bytes < need) return EPNET_ENOMEM;
    if (((uintptr_t)index & 15) != 0) return EPNET_EINVAL;
    EPNET_REQUIRE(b <= 65535);
    const int np = scene_index_np(n);
    float4 *sorted = (float4 *)index;
    float *boxes = (float *)(sorted + (size_t)b * np);
    return spatial_index_launch(b, n, np, xyz_src, sorted, boxes, boxes + (size_t)b * (np / 64) * 6, (hipStream_t)stream, n_src, idx,
                                gathered);
}

extern "C" int epnet_ball_query_indexed(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                                        const float *xyz, const void *index, size_t index_bytes, int *idx,
                                        epnet_stream_t stream) {
    const size_t need = scene_index_bytes(b, n);
    if (need == 0 || !index || nsample <= 0 || m <= 0)
        return epnet_ball_query(b, n, m, radius, nsample, new_xyz, xyz, idx, stream);
    EPNET_REQUIRE(new_xyz && idx);
    if (index_bytes < need) return EPNET_ENOMEM;
    EPNET_REQUIRE(b <= 65535);
    const int np = scene_index_np(n);
    BqScales<1> sc;
    sc.r2[0] = radius * radius;  // ball_query_gpu.cu:23
    sc.nsample[0] = nsample;
    sc.idx[0] = idx;
    return bq_query_launch<1>(b, np, m, sc, new_xyz, (const float4 *)index, (hipStream_t)stream);
}

// the nscales ball queries of an MSG level (same centres, same points) in one launch: boxes are tested against the
// largest radius and every distance is computed once. idx[k]: (b, m, nsample[k]). Same results as nscales calls.
extern "C" int epnet_ball_query_indexed_multi(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                              const float *new_xyz, const float *xyz, const void *index,
                                              size_t index_bytes, int *const *idx, epnet_stream_t stream) {
    EPNET_REQUIRE(nscales >= 0 && (nscales == 0 || (radii && nsamples && idx)));
    const size_t need = scene_index_bytes(b, n);
    bool fused = nscales == 2 && need != 0 && index && m > 0 && nsamples[0] > 0 && nsamples[1] > 0;
    if (!fused) {
        for (int k = 0; k < nscales; ++k) {
            const int rc = epnet_ball_query_indexed(b, n, m, radii[k], nsamples[k], new_xyz, xyz, index, index_bytes, idx[k], stream);
            if (rc) return rc;
        }
        return EPNET_OK;
    }
    EPNET_REQUIRE(new_xyz && idx[0] && idx[1]);
    if (index_bytes < need) return EPNET_ENOMEM;
    EPNET_REQUIRE(b <= 65535);
    BqScales<2> sc;
    for (int k = 0; k < 2; ++k) {
        sc.r2[k] = radii[k] * radii[k];  // ball_query_gpu.cu:23
        sc.nsample[k] = nsamples[k];
        sc.idx[k] = idx[k];
    }
    return bq_query_launch<2>(b, scene_index_np(n), m, sc, new_xyz, (const float4 *)index, (hipStream_t)stream);
}

// the nscales (1 or 2) ball queries of a level with the centres served in THEIR spatial order: centre_index is the scene index of
// the m centres (new_xyz = the cloud it was built from, in that order). Same results as epnet_ball_query_indexed_multi.
extern "C" int epnet_ball_query_ordered(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                        const float *new_xyz, const float *xyz, const void *index, size_t index_bytes,
                                        const void *centre_index, size_t centre_index_bytes, int *const *idx,
                                        epnet_stream_t stream) {
    EPNET_REQUIRE(nscales >= 0 && (nscales == 0 || (radii && nsamples && idx)));
    const size_t need = scene_index_bytes(b, n), need_c = scene_index_bytes(b, m);
    bool ordered = (nscales == 1 || nscales == 2) && need != 0 && need_c != 0 && index && centre_index && m > 0;
    for (int k = 0; ordered && k < nscales; ++k) ordered = nsamples[k] > 0 && idx[k] != nullptr;
    // what the order buys is cache hits on the point rows: nothing up to 16384 points (the scene's rows stay in L2 whatever the order:
    // 256 scenes, 16384 x 4096: 0.458 = 0.455 ms; 4096 x 1024: 0.108 -> 0.125), 31 % at 65536 (6.68 -> 4.58 ms). EPNET_BQ_ORDERED=0/1 forces.
    const int force = tuning(kBqOrdered);
    if (force >= 0 ? force == 0 : n <= 16384) ordered = false;
    if (!ordered) return epnet_ball_query_indexed_multi(b, n, m, nscales, radii, nsamples, new_xyz, xyz, index, index_bytes, idx, stream);
    if (index_bytes < need || centre_index_bytes < need_c) return EPNET_ENOMEM;
    EPNET_REQUIRE(b <= 65535);
    const int np = scene_index_np(n), npc = scene_index_np(m);
    if (nscales == 1) {
        BqScales<1> sc;
        sc.r2[0] = radii[0] * radii[0];  // ball_query_gpu.cu:23
        sc.nsample[0] = nsamples[0];
        sc.idx[0] = idx[0];
        return bq_query_launch<1>(b, np, m, sc, new_xyz, (const float4 *)index, (hipStream_t)stream, (const float4 *)centre_index, npc);
    }
    BqScales<2> sc;
    for (int k = 0; k < 2; ++k) {
        sc.r2[k] = radii[k] * radii[k];
        sc.nsample[k] = nsamples[k];
        sc.idx[k] = idx[k];
    }
    return bq_query_launch<2>(b, np, m, sc, new_xyz, (const float4 *)index, (hipStream_t)stream, (const float4 *)centre_index, npc);
}

extern "C" size_t epnet_ball_query_workspace_bytes(int b, int n, int m) {
    if (n < 1024 || m <= 0) return 0;  // small or huge scenes: direct scan, no scratch
    return scene_index_bytes(b, n);
}

extern "C" int epnet_ball_query_ws(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                                   const float *xyz, int *idx, void *workspace, size_t workspace_bytes,
                                   epnet_stream_t stream) {
    const size_t need = epnet_ball_query_workspace_bytes(b, n, m);
    if (need == 0 || nsample <= 0) return epnet_ball_query(b, n, m, radius, nsample, new_xyz, xyz, idx, stream);
    EPNET_REQUIRE(new_xyz && xyz && idx && workspace);
    int rc = epnet_scene_index_build(b, n, xyz, workspace, workspace_bytes, stream);
    if (rc) return rc;
    return epnet_ball_query_indexed(b, n, m, radius, nsample, new_xyz, xyz, workspace, workspace_bytes, idx, stream);
}

#ifdef EPNET_BQ_STATS
extern "C" int epnet_debug_bq_stats(unsigned long long *host16) {
    (void)hipMemcpyFromSymbol(host16, HIP_SYMBOL(epnet::g_bq_stats), sizeof(unsigned long long) * 16);
    unsigned long long zero[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(epnet::g_bq_stats), zero, sizeof(zero));
    return 0;
}
#endif
#ifdef EPNET_IX_STATS
extern "C" int epnet_debug_ix_stats(unsigned long long *host8) {
    (void)hipMemcpyFromSymbol(host8, HIP_SYMBOL(epnet::g_ix_stats), sizeof(unsigned long long) * 8);
    unsigned long long zero[8] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(epnet::g_ix_stats), zero, sizeof(zero));
    return 0;
}
#endif
