// fps_pruned.h -- the spatially pruned sampling kernels: the shared rounds, the self-sorting kernel and the one over a scene index
// (with the next level's index build as its epilogue).
//
// Exact FPS with spatial pruning, for 1024 < N <= 16384. The points are sorted by grid cell (a scene index
// built beforehand, or an in-kernel counting sort on an interleaved cell code, spatial.h) and dealt in groups of
// 64 consecutive sorted points to (wave, slot) registers: group g is slot g/W of wave g%W, one point per lane.
// Every slot is split into 64/PPT buckets of PPT lanes; a bucket's summary (bounding box, maximum running
// distance bm) lives in one lane of the bucket itself. A new sample c can only lower distances in buckets whose
// box lies closer than their bm, so per round a wave
//   A. evaluates L = |clamp(c, box) - c|^2 for all its 64 buckets at once (one bucket per lane),
//   B. updates only the slots holding a bucket with L < bm (typically 0-3; the slot registers are addressed
//      with the gfx9 GPR-index mode, so there is one copy of the code and no branch tree),
//   C. reduces its bucket maxima; every thread holding the wave's maximum publishes its point (coordinates
//      into its record slot, (distance, rank, thread) into one 64-bit LDS atomic max),
//   D. after the single barrier reads the winning key and that thread's coordinates.
// Everything after the `active` mask stays on the vector ALU (DPP / permlane-swap reductions, lane
// masks instead of readlane -> SALU -> VALU round trips).
// Skipping is EXACT, not approximate: L_j is computed with the very expression used for point
// distances (dx*dx + dy*dy + dz*dz, fp32, no contraction) on the clamped point; fp32 subtraction,
// multiplication and addition are monotone, so every point of the bucket has d >= L_j >= bm_j >= its
// running distance and min(d, t) = t bit for bit. Tie-breaks cannot follow the lane order here (the
// layout is spatial): every maximum carries the reference rank of its point,
// rank(k) = (bitreverse10(k mod 1024) << 4) | (k div 1024)  (block size 1024 for every N > 1024),
// and equal distances are resolved by the smaller rank inside a bucket, between buckets and between
// waves -- exactly the winner of the reference's strided scan + shared-memory tree.
#pragma once
#include <type_traits>

#include "fps_common.h"

namespace epnet {
namespace pruned {

#ifndef EPNET_FPS_PRIO
#define EPNET_FPS_PRIO 3
#endif

#ifdef EPNET_FPS_STATS  // diagnostic build only (scratch/fps_stats.hip): phase cycle counters
__device__ unsigned long long g_stats[16];
#define EPNET_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define EPNET_ACC(slot, a, b) st_acc[slot] += (unsigned long long)((b) - (a))
#define EPNET_CNT(slot, v) st_acc[slot] += (unsigned long long)(v)
#define EPNET_STATS_BEGIN unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define EPNET_STATS_END if ((threadIdx.x & 63) == 0) for (int s_ = 0; s_ < 8; ++s_) atomicAdd(&g_stats[s_], st_acc[s_])
#else
#define EPNET_STAMP(var)
#define EPNET_ACC(slot, a, b)
#define EPNET_CNT(slot, v)
#define EPNET_STATS_BEGIN
#define EPNET_STATS_END
#endif

__device__ __forceinline__ unsigned rank14(int k) { return (bitrev_lg((unsigned)k & 1023u, 10) << 4) | ((unsigned)k >> 10); }
__device__ __forceinline__ int unrank14(unsigned r) { return (int)(bitrev_lg(r >> 4, 10) + ((r & 15u) << 10)); }

// max over aligned groups of G lanes (G = 8, 16 or 32), result in every lane of the group
template <int G>
__device__ __forceinline__ int group_max(int v) {
    v = max(v, dpp_i32<0xB1>(v));                  // quad_perm [1,0,3,2]
    v = max(v, dpp_i32<0x4E>(v));                  // quad_perm [2,3,0,1]
    v = max(v, dpp_i32<0x141>(v));                 // row_half_mirror: the other quad of the 8-lane half
    if (G >= 16) v = max(v, dpp_i32<0x140>(v));    // row_mirror: the other half of the row
    if (G >= 32) {
        const auto a = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        v = max((int)a[0], (int)a[1]);
    }
    return v;
}
template <int G>
__device__ __forceinline__ float group_minf(float v) {
    v = fminf(v, __int_as_float(dpp_i32<0xB1>(__float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_i32<0x4E>(__float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_i32<0x141>(__float_as_int(v))));
    if (G >= 16) v = fminf(v, __int_as_float(dpp_i32<0x140>(__float_as_int(v))));
    if (G >= 32) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fminf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    }
    return v;
}
template <int G>
__device__ __forceinline__ float group_maxf(float v) { return -group_minf<G>(-v); }

// data replicated with period P (a power of two <= 16) along the lanes: reduce over one period
template <int P>
__device__ __forceinline__ int period_max(int v) {
    if (P > 1) v = max(v, dpp_i32<0xB1>(v));
    if (P > 2) v = max(v, dpp_i32<0x4E>(v));
    if (P > 4) v = max(v, dpp_i32<0x124>(v));
    if (P > 8) v = max(v, dpp_i32<0x128>(v));
    return v;
}
template <int P>
__device__ __forceinline__ unsigned period_min(unsigned v) {
    if (P > 1) v = min(v, dpp_u32<0xB1>(v));
    if (P > 2) v = min(v, dpp_u32<0x4E>(v));
    if (P > 4) v = min(v, dpp_u32<0x124>(v));
    if (P > 8) v = min(v, dpp_u32<0x128>(v));
    return v;
}

// fold a 64-lane ballot over the 64/PPT parts of a slot: bit j set <=> some part of slot j is set
template <int PPT>
__device__ __forceinline__ unsigned fold_parts(unsigned long long a) {
    if (PPT <= 32) a |= a >> 32;
    if (PPT <= 16) a |= a >> 16;
    if (PPT <= 8) a |= a >> 8;
    return (unsigned)a & (PPT >= 32 ? 0xFFFFFFFFu : ((1u << PPT) - 1u));
}

constexpr int kIdxBufP = 1024;  // selected ranks buffered in LDS between flushes

// reference ranks of a thread's PPT points, two 16-bit ranks per register (0xFFFF = padding)
template <typename VH>
__device__ __forceinline__ unsigned rank_of(const VH &rk2, int j) {
    return ((unsigned)rk2[j >> 1] >> ((j & 1) << 4)) & 0xFFFFu;
}
template <typename VH>
__device__ __forceinline__ void set_rank(VH &rk2, int j, unsigned r) {  // j is a compile-time constant at the call sites
    rk2[j >> 1] = (j & 1) ? (int)(((unsigned)rk2[j >> 1] & 0xFFFFu) | (r << 16)) : (int)r;
}

// The M-1 rounds. W waves per scene (4: one per SIMD; 8 for N > 8192), PPT slots of 64 points per wave;
// thread (wave, lane) holds in slot j the point at sorted position ((j*kW + wave) << 6) | lane: coordinates,
// running distance t (bits; -1.0f = padding) and reference rank rk.
// A slot is split into 64/PPT parts of PPT lanes: these parts are the pruning buckets, and bucket
// (slot j, part p) is summarised in lane p*PPT + j -- a lane of the part itself, so a part's maximum
// reaches its summary lane with an in-row DPP reduction and a lane-id compare, no cross-lane move.
// Cross-wave arg-max: every thread holding its wave's maximum enters ONE 64-bit LDS atomic max on the key
// (distance bits << 32 | (0x3FFF - rank) << 10 | thread): the larger distance wins, equal distances go to the
// smaller reference rank -- and after the round's single barrier the winner is read back with two
// dependent LDS loads (key, then that thread's coordinates), no cross-lane reduction at all.
// LDS comes from the caller (s_key: 3 keys, s_rec: one record slot per thread and round parity, s_idx: kIdxBufP ints), so that a
// kernel with an epilogue of its own can lay the epilogue's LDS over them (fps_indexed_kernel).
template <int kW, int PPT, typename VF, typename VI, typename VH>
__device__ __forceinline__ void fps_rounds(unsigned long long *s_key, float4 (*s_rec)[64 * kW], int *s_idx, int m, const VF &x,
                                           const VF &y, const VF &z, VI &t, const VH &rk2,
                                           float cx, float cy, float cz, int *__restrict__ idxs,
                                           int *__restrict__ tie_free = nullptr, int known = 0,
                                           const float *__restrict__ xyz_in_order = nullptr, int detect_upto = 0x7fffffff) {
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    const int sub = lane & (PPT - 1);  // the slot this lane summarises (for its own part)
    const int kNeg1 = __float_as_int(-1.f);

    // ---- bucket summaries
    int bm = kNeg1;
    float lox = 0.f, hix = 0.f, loy = 0.f, hiy = 0.f, loz = 0.f, hiz = 0.f;
    for (int j = 0; j < PPT; ++j) {  // runtime loop, indexed registers: one copy of the code
        const float xj = x[j], yj = y[j], zj = z[j];
        const int tj = t[j];
        const bool real = tj != kNeg1;
        const float mnx = group_minf<PPT>(real ? xj : 3.4e38f), mxx = group_maxf<PPT>(real ? xj : -3.4e38f);
        const float mny = group_minf<PPT>(real ? yj : 3.4e38f), mxy = group_maxf<PPT>(real ? yj : -3.4e38f);
        const float mnz = group_minf<PPT>(real ? zj : 3.4e38f), mxz = group_maxf<PPT>(real ? zj : -3.4e38f);
        const int gm = group_max<PPT>(tj);  // -1 for an all-padding bucket: never active, never best
        if (sub == j) {
            const bool any = gm != kNeg1;
            bm = gm;
            lox = any ? mnx : 0.f; hix = any ? mxx : 0.f;
            loy = any ? mny : 0.f; hiy = any ? mxy : 0.f;
            loz = any ? mnz : 0.f; hiz = any ? mxz : 0.f;
        }
    }
    if (q < 3) s_key[q] = 0ull;
    if (q == 0) s_idx[0] = 0;  // rank 0 == point 0
    // `known` leading samples are given (points 0 .. known-1 of the cloud in its own order: a sampling pyramid's chain,
    // epnet_sample_centres_chain): their rounds need no selection, only the distance updates -- no cross-wave exchange, no barrier
    if (known > kIdxBufP || known > m || !xyz_in_order) known = 0;
    for (int i = q; i < known; i += 64 * kW) s_idx[i] = (int)rank14(i);
    __syncthreads();
    for (int it = 1; it < known; ++it) {
        const float px = __builtin_amdgcn_fmed3f(cx, lox, hix), py = __builtin_amdgcn_fmed3f(cy, loy, hiy),
                    pz = __builtin_amdgcn_fmed3f(cz, loz, hiz);
        const float bdx = px - cx, bdy = py - cy, bdz = pz - cz;
        const float L = bdx * bdx + bdy * bdy + bdz * bdz;
        unsigned active = fold_parts<PPT>(__ballot(__float_as_int(L) < bm));
        const float nx = xyz_in_order[it * 3 + 0], ny = xyz_in_order[it * 3 + 1], nz = xyz_in_order[it * 3 + 2];  // the next sample
        while (active) {
            const int j = (int)__builtin_ctz(active);
            active &= active - 1u;
            const float xj = x[j], yj = y[j], zj = z[j];
            const int told = t[j];
            __builtin_amdgcn_sched_barrier(0);
            const float dx = xj - cx, dy = yj - cy, dz = zj - cz;
            const float d = dx * dx + dy * dy + dz * dz;
            const int tj = min(__float_as_int(d), told);
            t[j] = tj;
            const int gm = group_max<PPT>(tj);
            bm = (sub == j) ? gm : bm;
        }
        cx = nx;
        cy = ny;
        cz = nz;
    }

    // a strictly serial chain: when it shares a SIMD with a wide kernel (software-pipelined SA stack), every
    // instruction it has ready should issue first
    __builtin_amdgcn_s_setprio(EPNET_FPS_PRIO);
    EPNET_STATS_BEGIN;
    EPNET_STAMP(t_loop0);
    // this wave's best point(s), recomputed only in rounds that update a bucket holding one of them
    bool stale = true;
    int wbest = kNeg1;
    unsigned long long hbuckets = 0ull;  // buckets (by summary lane) in which this lane holds the wave's maximum
    unsigned racc = 0xFFFFFFFFu;  // != ~0 in the lanes that publish
    float xa = 0.f, ya = 0.f, za = 0.f;
    int kb = 1;  // key slot of the round = it % 3
    // the first round in which the reference's tie-break decides WHICH COORDINATES are sampled: several points at the maximum
    // running distance that are not all exact twins of one another (or a maximum of zero: every point coincides with a sample).
    // Up to that round the sequence of sampled coordinates is a property of the coordinates alone (epnet_sample_centres_chain).
    // Exact twins -- the reference's loader pads short scenes by re-drawing rows, kitti_rcnn_dataset.py:338-342 -- tie at the
    // round one of them is picked, harmlessly: the others sit at distance 0 from then on and cannot be sampled while the
    // maximum is positive.
    bool wave_multi = false;  // several points of this wave hold its maximum
    int tied_v = 0x7fffffff;  // wave-uniform, kept scalar
    // one round; kTies: also look for a second holder of the round's maximum (only the rounds a later level can ask about pay
    // for that: the two instantiations of the body are run one after the other)
    auto round = [&](auto ties_tag, const int it) __attribute__((always_inline)) {
        constexpr bool kTies = decltype(ties_tag)::value;
        EPNET_STAMP(t0);
        // A. which buckets can change?
        const float px = __builtin_amdgcn_fmed3f(cx, lox, hix), py = __builtin_amdgcn_fmed3f(cy, loy, hiy),
                    pz = __builtin_amdgcn_fmed3f(cz, loz, hiz);
        const float bdx = px - cx, bdy = py - cy, bdz = pz - cz;
        const float L = bdx * bdx + bdy * bdy + bdz * bdz;
        const unsigned long long act64 = __ballot(__float_as_int(L) < bm);  // bit = summary lane of an active bucket
        unsigned active = fold_parts<PPT>(act64);
        EPNET_CNT(0, __popc(active));
        // distances only fall: the wave's maximum and its holders stand unless one of THEIR buckets is updated
        stale = stale || __ballot((hbuckets & act64) != 0ull) != 0ull;
        EPNET_STAMP(t1);
        // B. update the slots that contain one (handling two slots per iteration was measured: 20 % slower)
        while (active) {
            const int j = (int)__builtin_ctz(active);
            active &= active - 1u;
            const float xj = x[j], yj = y[j], zj = z[j];
            const int told = t[j];
            __builtin_amdgcn_sched_barrier(0);  // keep the indexed reads together: one GPR-index window
            const float dx = xj - cx, dy = yj - cy, dz = zj - cz;
            const float d = dx * dx + dy * dy + dz * dz;
            const int tj = min(__float_as_int(d), told);  // == fminf(d, temp[k]); padding stays at -1
            t[j] = tj;
            const int gm = group_max<PPT>(tj);
            bm = (sub == j) ? gm : bm;
        }
        EPNET_STAMP(t2);
        // C. this wave's maximum. EVERY lane holding it (usually exactly one) publishes its point: its own record
        // slot and the atomic key, which orders equal distances by reference rank -- no holder count, no second
        // reduction, whatever the number of ties
        if (stale) {
            stale = false;
            wbest = wave_max_all(bm);
            unsigned cand = fold_parts<PPT>(__ballot(bm == wbest));
            racc = 0xFFFFFFFFu;
            hbuckets = 0ull;
            do {
                const int j = (int)__builtin_ctz(cand);
                cand &= cand - 1u;
                const int tj = t[j];
                const float xj = x[j], yj = y[j], zj = z[j];
                const unsigned rw = (unsigned)rk2[j >> 1];
                __builtin_amdgcn_sched_barrier(0);  // one GPR-index window for the four slot registers
                const unsigned r = tj == wbest ? ((rw >> ((j & 1) << 4)) & 0xFFFFu) : 0xFFFFFFFFu;
                if (r != 0xFFFFFFFFu) hbuckets |= 1ull << ((lane & ~(PPT - 1)) | j);  // summary lane of (slot j, my part)
                const bool take = r < racc;  // a lane holding the maximum in two of its slots keeps the smaller rank
                racc = take ? r : racc;
                xa = take ? xj : xa;
                ya = take ? yj : ya;
                za = take ? zj : za;
            } while (cand);
            if (wbest == kNeg1) {  // a wave of padding only
                racc = 0xFFFFFFFFu;
                hbuckets = 0ull;
            }
            if (kTies) {
                // (hbuckets has one bit per slot in which the lane holds the maximum)
                const unsigned long long holders = __ballot(hbuckets != 0ull);
                wave_multi = (holders & (holders - 1ull)) != 0ull || __ballot((hbuckets & (hbuckets - 1ull)) != 0ull) != 0ull;
            }
        }
        const int buf = it & 1;
        if (racc != 0xFFFFFFFFu) {
            s_rec[buf][q] = make_float4(xa, ya, za, 0.f);
            const unsigned long long key =
                ((unsigned long long)(unsigned)wbest << 32) | (unsigned long long)(((0x3FFFu - racc) << 10) | (unsigned)q);
            __hip_atomic_fetch_max(&s_key[kb], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        EPNET_STAMP(t3);
        __syncthreads();
        EPNET_STAMP(t4);
        // D. the winner: key, then its thread's coordinates (both loads are wave-uniform broadcasts)
        const unsigned long long kfull = s_key[kb];
        const unsigned klo = (unsigned)kfull;
        const float4 rec = s_rec[buf][klo & 1023u];
        cx = rec.x;
        cy = rec.y;
        cz = rec.z;
        if (kTies) {
            // this wave's (exact, possibly cached) maximum equals the winner's distance and the winner is not its only holder: a
            // tie -- unless every other holder is an exact twin of the winner. The first test is what every round pays (a handful
            // of instructions; the twin rule computed branch-free on every round cost 0.1 us on each of the 1024 watched rounds of
            // the level-1 sampling: 2.05 -> 2.15 ms); the coordinates are compared behind a wave-uniform branch that only a round
            // with several holders takes.
            const bool mine = (int)((klo & 1023u) >> 6) == wave;
            const int wd = (int)(unsigned)(kfull >> 32);
            const bool suspect = (wbest == wd && (!mine || wave_multi)) || wd == 0;
            if (__builtin_amdgcn_readfirstlane(suspect ? 1 : 0)) {
                // every slot in which a lane holds the maximum (bit (lane's part | j) of hbuckets) against the winner's coordinates
                // (the winner's own slot compares equal to itself)
                bool differs = false;
                const unsigned mine_slots = (unsigned)((hbuckets >> (lane & ~(PPT - 1))) & ((1ull << PPT) - 1ull));   // (PPT <= 32)
                unsigned any_slots = mine_slots;   // slots in which ANY lane of the wave holds the maximum
                for (int off = 32; off >= 1; off >>= 1) any_slots |= (unsigned)__shfl_xor((int)any_slots, off, 64);
                // a runtime loop with indexed registers: one copy of the code, no registers beyond the round's own
#pragma unroll 1
                while (any_slots) {
                    const int j = (int)__builtin_ctz(any_slots);
                    any_slots &= any_slots - 1u;
                    const float xj = x[j], yj = y[j], zj = z[j];
                    __builtin_amdgcn_sched_barrier(0);
                    differs = differs || (((mine_slots >> j) & 1u) && (xj != cx || yj != cy || zj != cz));
                }
                if (wd == 0 || __ballot(differs)) tied_v = min(tied_v, it);
            }
        }
        const int kb2 = kb == 0 ? 2 : kb - 1;  // == (it + 2) % 3: last read in round it-1, next used in round it+2
        kb = kb == 2 ? 0 : kb + 1;
        if (wave == 0) {
            s_idx[it & (kIdxBufP - 1)] = (int)(0x3FFFu - (klo >> 10));  // all lanes, same word; converted at the flush
            if (lane == 0) s_key[kb2] = 0ull;
            if ((it & (kIdxBufP - 1)) == kIdxBufP - 1) {
                const int base = it - (kIdxBufP - 1);
                for (int e = lane; e < kIdxBufP; e += 64) idxs[base + e] = unrank14((unsigned)s_idx[e]);
            }
        }
        EPNET_STAMP(t5);
        EPNET_ACC(1, t0, t1); EPNET_ACC(2, t1, t2); EPNET_ACC(3, t2, t3); EPNET_ACC(4, t3, t4); EPNET_ACC(5, t4, t5);
    };
    int it0 = max(1, known);
    if (tie_free) {
        const int upto = min(m, detect_upto);
        for (; it0 < upto; ++it0) round(std::true_type{}, it0);
    }
    for (; it0 < m; ++it0) round(std::false_type{}, it0);
    EPNET_STAMP(t_loop1);
    EPNET_ACC(6, t_loop0, t_loop1);
    EPNET_STATS_END;
    if (tie_free && lane == 0) atomicMin(tie_free, min(min(tied_v, m), detect_upto));  // (initialised to m by the caller's launch sequence)
    if (wave == 0) {
        const int base = (m - 1) & ~(kIdxBufP - 1);
        for (int e = lane; base + e < m; e += 64) idxs[base + e] = unrank14((unsigned)s_idx[e]);
    }
}

// Self-contained kernel (no caller scratch): counting-sorts the scene by grid cell in LDS, then runs the rounds.
template <int kW, int PPT>
__global__ __launch_bounds__(64 * kW) void fps_pruned_kernel(int n, int m, const float *__restrict__ xyz,
                                                             float *__restrict__ temp, int *__restrict__ idxs,
                                                             const int *__restrict__ skip, int *__restrict__ prefix_out,
                                                             int prefix_cap) {
    if (skip && skip[blockIdx.x] >= m) return;
    typedef float vecf __attribute__((ext_vector_type(PPT)));
    typedef int veci __attribute__((ext_vector_type(PPT)));
    constexpr int kT = 64 * kW;
    extern __shared__ int s_dyn[];  // cell histogram, then the 16-bit point indices in cell order
    int *hist = s_dyn;
    unsigned short *perm = reinterpret_cast<unsigned short *>(s_dyn + kCells + kCells / (kCells / kT) + 64);
    __shared__ int s_part[16];
    __shared__ float s_box[6][16];
    __shared__ unsigned long long s_key[3];
    __shared__ float4 s_rec[2][64 * kW];
    __shared__ int s_idx[kIdxBufP];
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    xyz += (size_t)blockIdx.x * n * 3;
    if (temp) temp += (size_t)blockIdx.x * n;
    idxs += (size_t)blockIdx.x * m;

    // ---- spatial order: counting sort by grid cell (spatial.h); positions >= n are padding
    float lo[3], ext[3];
    block_bbox3(xyz, n, s_box, lo, ext);
    const CellGrid grid = make_cell_grid(lo, ext);
    cell_sort_lds(xyz, n, grid, hist, s_part, perm);

    // ---- sorted position p = (group << 6 | lane); group g of 64 sorted points -> (wave g % kW, slot g / kW)
    veci kk;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int p = ((j * kW + wave) << 6) | lane;
        kk[j] = p < n ? (int)perm[p] : -1;
    }
    typedef int vech __attribute__((ext_vector_type(PPT / 2)));
    vecf x, y, z;
    veci t;
    vech rk2;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int k = kk[j];
        if (k >= 0) {
            x[j] = xyz[k * 3 + 0];
            y[j] = xyz[k * 3 + 1];
            z[j] = xyz[k * 3 + 2];
            t[j] = __float_as_int(temp ? temp[k] : 1e10f);
            set_rank(rk2, j, rank14(k));
        } else {  // padding: distance pinned at -1
            x[j] = y[j] = z[j] = 0.f;
            t[j] = __float_as_int(-1.f);
            set_rank(rk2, j, 0xFFFFu);
        }
    }
    fps_rounds<kW, PPT>(s_key, s_rec, s_idx, m, x, y, z, t, rk2, xyz[0], xyz[1], xyz[2], idxs, prefix_out ? prefix_out + blockIdx.x : nullptr, 0,
                        nullptr, prefix_cap);
    if (temp) {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const unsigned r = rank_of(rk2, j);
            if (r != 0xFFFFu) temp[unrank14(r)] = __int_as_float(t[j]);
        }
    }
}

// The epilogue of fps_indexed_kernel: a function of its own (not inlined), so that its registers are allocated apart from the
// round loop's -- two sampling waves of 200 VGPRs plus two gather waves per SIMD is what the pipelined schedule rests on.
template <int kT, int BITS, int kPer, int kStage>
__device__ __attribute__((noinline)) void fps_index_epilogue(int *s_hist, float (*s_box)[16], int *s_part, int m, int np,
                                                             const float *xyz, float4 *sorted, float *boxes, float *qboxes, int n_src,
                                                             const int *src_idx, float *gathered) {
    scene_index_build_block<kT, BITS, kPer, kStage, true>(s_hist, s_box, s_part, m, np, xyz, sorted, boxes, qboxes, n_src, src_idx,
                                                          gathered);
}

// Same rounds over a scene index built beforehand (spatial.h: cell-sorted float4 copy x, y, z, original index;
// padding entries carry index -1). Needs no dynamic LDS, so it shares a CU with the bandwidth-bound kernels.
template <int kW, int PPT>
__global__ __launch_bounds__(64 * kW) void fps_indexed_kernel(int n, int m, const float4 *__restrict__ sorted,
                                                              float *__restrict__ temp, int *__restrict__ idxs,
                                                              const int *__restrict__ prefix_in,
                                                              int *__restrict__ prefix_out, const float *__restrict__ xyz,
                                                              int prefix_cap, int prologue_init, void *next_index,
                                                              float *__restrict__ new_xyz) {
    typedef float vecf __attribute__((ext_vector_type(PPT)));
    typedef int veci __attribute__((ext_vector_type(PPT)));
    constexpr int NP = 64 * kW * PPT;
    // ONE LDS array. The rounds' part: records, index buffer, keys, the first sample. The 512-thread kernel's epilogue (below) lays
    // the next level's index build over it once the rounds are through: histogram, staging rows, box and scan partials.
    constexpr bool kEpilogue = kW == 8;
    constexpr int kRecAt = 0, kIdxAt = kRecAt + 2 * 64 * kW * 16, kKeyAt = kIdxAt + kIdxBufP * 4, kFirstAt = kKeyAt + 32,
                  kRoundsBytes = kFirstAt + 16;
    constexpr int kIxBits = 12, kIxPer = 8, kIxStage = 512;   // 512 threads x 8 points: m <= 4096
    constexpr int kIxHistWords = (1 << kIxBits) + (1 << kIxBits) / ((1 << kIxBits) / (64 * kW)) + 64;
    constexpr int kStageAt = kIxHistWords * 4, kBoxAt = kStageAt + kIxStage * 16, kPartAt = kBoxAt + 6 * 16 * 4,
                  kIxBytes = kEpilogue ? kPartAt + 16 * 4 : 0;
    // what only the epilogue needs waits in LDS behind the rounds' part (the kernel has no scalar registers to spare across the round
    // loops: kept in SGPRs they were spilled to lanes of a 201st VGPR)
    constexpr int kArgsAt = kRoundsBytes;
    static_assert(kStageAt % 16 == 0 && kIxBytes <= 32768, "the sampling workgroup shares its CU with two 64 KB row gathers");
    static_assert(!kEpilogue || kArgsAt + 32 <= kIxBytes, "epilogue arguments");
    __shared__ __attribute__((aligned(16))) unsigned char s_lds[kRoundsBytes > kIxBytes ? kRoundsBytes : kIxBytes];
    unsigned long long *const s_key = reinterpret_cast<unsigned long long *>(s_lds + kKeyAt);
    float4(*const s_rec)[64 * kW] = reinterpret_cast<float4(*)[64 * kW]>(s_lds + kRecAt);
    int *const s_idx = reinterpret_cast<int *>(s_lds + kIdxAt);
    float *const s_first = reinterpret_cast<float *>(s_lds + kFirstAt);
    unsigned long long *const s_args = reinterpret_cast<unsigned long long *>(s_lds + kArgsAt);
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    const int known = prefix_in ? prefix_in[blockIdx.x] : 0;
    // the first m points ARE the samples?
    if (fps_prologue(m, prefix_in, idxs + (size_t)blockIdx.x * m, prefix_out, prologue_init)) return;
    sorted += (size_t)blockIdx.x * NP;
    if (temp) temp += (size_t)blockIdx.x * n;
    idxs += (size_t)blockIdx.x * m;
    typedef int vech __attribute__((ext_vector_type(PPT / 2)));
    vecf x, y, z;
    veci t;
    vech rk2;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const float4 v = sorted[((j * kW + wave) << 6) | lane];
        const int k = __float_as_int(v.w);
        if (k >= 0) {
            x[j] = v.x;
            y[j] = v.y;
            z[j] = v.z;
            t[j] = __float_as_int(temp ? temp[k] : 1e10f);
            set_rank(rk2, j, rank14(k));
            if (k == 0) {  // the first sample is point 0 (sampling_gpu.cu:118)
                s_first[0] = v.x;
                s_first[1] = v.y;
                s_first[2] = v.z;
            }
        } else {
            x[j] = y[j] = z[j] = 0.f;
            t[j] = __float_as_int(-1.f);
            set_rank(rk2, j, 0xFFFFu);
        }
    }
    if constexpr (kEpilogue) {
        if (q == 0) {
            s_args[0] = (unsigned long long)next_index;
            s_args[1] = (unsigned long long)new_xyz;
            s_args[2] = (unsigned long long)xyz;
            s_args[3] = (unsigned long long)(unsigned)n;
        }
    }
    __syncthreads();
    fps_rounds<kW, PPT>(s_key, s_rec, s_idx, m, x, y, z, t, rk2, s_first[0], s_first[1], s_first[2], idxs,
                        prefix_out ? prefix_out + blockIdx.x : nullptr, known, xyz ? xyz + (size_t)blockIdx.x * n * 3 : nullptr,
                        prefix_cap);
    if (temp) {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const unsigned r = rank_of(rk2, j);
            if (r != 0xFFFFu) temp[unrank14(r)] = __int_as_float(t[j]);
        }
    }
    if constexpr (kEpilogue) {
        // The next level's preparation, by the workgroup that has just picked its points: the m centres are gathered (new_xyz) and
        // their scene index is built (what epnet_scene_index_build_gathered does in a dispatch of its own): one dispatch less on the
        // sampling chain, and every scene starts as soon as ITS rounds end. Beside the wide kernels of the pipelined stack the build
        // costs this kernel about what it cost as a dispatch (0.06 ms). The priority stays raised, as in bq_index_kernel.
        // next_index != NULL (block-uniform) implies 1024 <= m <= 4096 and no prefix_in (fps_plan, held by its selftest).
        void *const next_index_ = (void *)s_args[0];
        if (next_index_) {
            float *const new_xyz_ = (float *)s_args[1];
            const float *const xyz_ = (const float *)s_args[2];
            const int n_ = (int)s_args[3];
            __threadfence_block();   // wave 0's last flush of idxs
            __syncthreads();         // ... and nobody reads the rounds' LDS (or the arguments above) any more
            const int np2 = m <= 2048 ? 2048 : 4096;   // scene_index_np(m)
            float4 *const sorted2 = reinterpret_cast<float4 *>(next_index_);
            float *const boxes2 = reinterpret_cast<float *>(sorted2 + (size_t)gridDim.x * np2);
            float *const qboxes2 = boxes2 + (size_t)gridDim.x * (np2 / 64) * 6;
            fps_index_epilogue<64 * kW, kIxBits, kIxPer, kIxStage>(
                reinterpret_cast<int *>(s_lds), reinterpret_cast<float(*)[16]>(s_lds + kBoxAt), reinterpret_cast<int *>(s_lds + kPartAt),
                m, np2, xyz_, sorted2, boxes2, qboxes2, n_, idxs - (size_t)blockIdx.x * m, new_xyz_);
        }
    }
}

}  // namespace pruned
}  // namespace epnet
