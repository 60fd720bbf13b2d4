// fps_bigscene.h -- sampling of scenes beyond the register file (16384 < N <= 65536), over a scene index.
#pragma once
#include "fps_pruned.h"

namespace epnet {
namespace pruned {

// The points stay in the index (L2-resident, <= 1 MB) and the running distances in the caller's temp buffer;
// only the bucket summaries live in registers: lane j of wave w owns bucket j * 16 + w (64 consecutive sorted points) -- its
// box (from the index), its maximum running distance bm and the rank and coordinates of the point holding it.
// A round tests all buckets against the new sample with the same exact lower bound, re-reads and updates only
// the active buckets (one wave per bucket, a coalesced 1 KB row of the index), and finds the arg-max over the
// summaries exactly as fps_rounds does (wave maximum, 64-bit LDS atomic key, one barrier).
// rank(k) = (bitreverse10(k mod 1024) << 6) | (k div 1024) -- 16 bits for k < 65536.
__device__ __forceinline__ unsigned rank16(int k) { return (bitrev_lg((unsigned)k & 1023u, 10) << 6) | ((unsigned)k >> 10); }
__device__ __forceinline__ int unrank16(unsigned r) { return (int)(bitrev_lg(r >> 6, 10) + ((r & 63u) << 10)); }

// kW waves per scene, every lane owning 1024 / (64 kW) buckets. Measured (65536 -> 16384, one scene / 256 scenes):
// 16 waves 0.88 / 1.18 us per round, 8 waves 1.11 / 1.47, 4 waves 1.50 / 1.97 -- the round is a chain of latencies through ONE
// wave (winner read-back -> box tests -> row load -> update + bucket maximum -> the wave's arg-max -> LDS atomic -> barrier), and
// a wave with four buckets per lane runs four box tests and up to four times the row updates back to back; the instructions
// the sixteen waves issue in total are not what bounds it: 16 it is.
template <int kW>
__global__ __launch_bounds__(64 * kW) void fps_bigscene_kernel(int n, int np, int m, const float *__restrict__ xyz,
                                                               const float4 *__restrict__ sorted,
                                                               const float *__restrict__ boxes,
                                                               float *__restrict__ temp, float *__restrict__ tsort,
                                                               int *__restrict__ idxs, const int *__restrict__ skip) {
    if (skip && skip[blockIdx.x] >= m) return;
    constexpr int kT = 64 * kW;
    constexpr int kBPL = 1024 / kT;   // buckets per lane (np <= 65536: at most 1024 buckets)
    constexpr int kLgW = kW == 16 ? 4 : (kW == 8 ? 3 : 2);
    static_assert(kW == 4 || kW == 8 || kW == 16, "bucket dealing assumes 4, 8 or 16 waves");
    __shared__ unsigned long long s_key[3];
    __shared__ float4 s_rec[2][kW];
    __shared__ int s_idx[kIdxBufP];
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    const int nb = np >> 6;
    xyz += (size_t)blockIdx.x * n * 3;
    sorted += (size_t)blockIdx.x * np;
    boxes += (size_t)blockIdx.x * nb * 6;
    temp += (size_t)blockIdx.x * n;
    tsort += (size_t)blockIdx.x * np;
    idxs += (size_t)blockIdx.x * m;
    const int kNeg1 = __float_as_int(-1.f);
    // Bucket e (= 0 .. 64 kBPL - 1) of this wave is bucket (e * kW + wave) of the scene; lane e % 64 keeps its summary in slot
    // e / 64. Consecutive buckets of the sorted order are spatial neighbours, and a new sample touches a handful of neighbouring
    // buckets -- dealt round-robin they land on different waves, which re-read them side by side instead of one wave working
    // through them one L2 round trip after the other
    auto bid = [&](int e) { return (e << kLgW) | wave; };

    float lox[kBPL], hix[kBPL], loy[kBPL], hiy[kBPL], loz[kBPL], hiz[kBPL];
    bool own[kBPL];
    int bm[kBPL];               // maximum running distance of my bucket (bits); -1: nothing real in it
    unsigned brank[kBPL];       // reference rank of the point holding it
    float bxx[kBPL], byy[kBPL], bzz[kBPL];
#pragma unroll
    for (int s_ = 0; s_ < kBPL; ++s_) {
        const int b_ = bid(s_ * 64 + lane);
        own[s_] = b_ < nb;
        lox[s_] = hix[s_] = loy[s_] = hiy[s_] = loz[s_] = hiz[s_] = 0.f;
        if (own[s_]) {
            const float *bx = boxes + b_ * 6;
            lox[s_] = bx[0]; hix[s_] = bx[1]; loy[s_] = bx[2]; hiy[s_] = bx[3]; loz[s_] = bx[4]; hiz[s_] = bx[5];
        }
        bm[s_] = kNeg1;
        brank[s_] = 0xFFFFu;
        bxx[s_] = byy[s_] = bzz[s_] = 0.f;
    }
    const int nmine = 64 * kBPL;   // bucket slots of this wave

    // The caller's running distances are indexed by ORIGINAL point number: a bucket's 64 values would be 64 cache lines.
    // The rounds keep them in SORTED order instead, in the sampling scratch at the tail of the scene index (one 256-byte
    // row per bucket, fetched beside the bucket's 1 KB row of the index); gathered on the way in, scattered back on the
    // way out. (The original index of a point rides in the .w of its index row: nothing per point is kept in registers --
    // a workgroup that holds few registers leaves the rest of the CU to the bandwidth-bound kernels beside it.)
    for (int e = 0; e < nmine; ++e) {
        const int pos = (bid(e) << 6) + lane;
        if (pos < n) tsort[pos] = temp[__float_as_int(sorted[pos].w)];
    }

    struct Row {
        float4 p;
        int t;
    };
    auto load_row = [&](int e) {
        Row r;
        const int pos = (bid(e) << 6) + lane;
        r.p = sorted[pos];
        r.t = pos < n ? __float_as_int(tsort[pos]) : kNeg1;
        return r;
    };
    // (re)computes the summary of bucket e of this wave from its row; with `update`, first lowers its distances by the sample c
    auto finish = [&](int e, Row r, bool update, float cx, float cy, float cz) {
        const int pos = (bid(e) << 6) + lane;
        const int k = __float_as_int(r.p.w);   // original index (padding rows: -1, never `real`)
        const bool real = pos < n;
        int t = r.t;
        if (real && update) {
            const float dx = r.p.x - cx, dy = r.p.y - cy, dz = r.p.z - cz;
            const float d = dx * dx + dy * dy + dz * dz;
            const int tn = min(__float_as_int(d), t);  // == fminf(d, temp[k])
            if (tn != t) tsort[pos] = __int_as_float(tn);
            t = tn;
        }
        const int mx = wave_max_all(t);
        const unsigned rk = (t == mx && real) ? rank16(k) : 0xFFFFFFFFu;
        unsigned long long holders = __ballot(rk != 0xFFFFFFFFu);
        unsigned rwin = 0xFFFFu;
        int wl = 0;
        if (holders) {
            if (holders & (holders - 1ull)) holders = __ballot(rk == wave_min_all(rk));  // several: the smallest rank
            wl = (int)__builtin_ctzll(holders);
            rwin = (unsigned)__builtin_amdgcn_readlane((int)rk, wl);
        }
        const float wx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.p.x), wl));
        const float wy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.p.y), wl));
        const float wz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.p.z), wl));
        const bool mine = lane == (e & 63);
        const int slot = e >> 6;   // wave-uniform
#pragma unroll
        for (int s_ = 0; s_ < kBPL; ++s_)
            if (mine && s_ == slot) {
                bm[s_] = mx;
                brank[s_] = rwin;
                bxx[s_] = wx; byy[s_] = wy; bzz[s_] = wz;
            }
    };

    for (int e = 0; e < nmine; ++e)
        if (bid(e) < nb) finish(e, load_row(e), false, 0.f, 0.f, 0.f);  // wave-uniform
    if (q < 3) s_key[q] = 0ull;
    if (q == 0) s_idx[0] = 0;  // rank 0 == point 0
    float cx = xyz[0], cy = xyz[1], cz = xyz[2];
    __syncthreads();

    __builtin_amdgcn_s_setprio(EPNET_FPS_PRIO);
    bool stale = true;
    int wbest = kNeg1;
    bool publisher = false;
    unsigned pub_rank = 0xFFFFu;
    float pub_x = 0.f, pub_y = 0.f, pub_z = 0.f;
    int kb = 1;
    for (int it = 1; it < m; ++it) {
        // A. which buckets can change?  (same fp32 expression as the point distance: exact)
        unsigned long long active[kBPL];
        bool any = false;
#pragma unroll
        for (int s_ = 0; s_ < kBPL; ++s_) {
            const float px = __builtin_amdgcn_fmed3f(cx, lox[s_], hix[s_]), py = __builtin_amdgcn_fmed3f(cy, loy[s_], hiy[s_]),
                        pz = __builtin_amdgcn_fmed3f(cz, loz[s_], hiz[s_]);
            const float bdx = px - cx, bdy = py - cy, bdz = pz - cz;
            const float L = bdx * bdx + bdy * bdy + bdz * bdz;
            active[s_] = __ballot(own[s_] && __float_as_int(L) < bm[s_]);
            any = any || active[s_] != 0ull;
        }
        stale = stale || any;
        // B. re-read and update them, two rows per trip to L2
#pragma unroll
        for (int s_ = 0; s_ < kBPL; ++s_) {
            unsigned long long act = active[s_];
            while (act) {
                const int e0 = s_ * 64 + (int)__builtin_ctzll(act);
                act &= act - 1ull;
                const bool two = act != 0ull;
                const int e1 = two ? s_ * 64 + (int)__builtin_ctzll(act) : e0;
                act &= act - 1ull;  // (no-op on 0)
                const Row r0 = load_row(e0);
                Row r1 = r0;
                if (two) r1 = load_row(e1);
                finish(e0, r0, true, cx, cy, cz);
                if (two) finish(e1, r1, true, cx, cy, cz);
            }
        }
        // C. this wave's best bucket (ties by rank)
        if (stale) {
            stale = false;
            int lmax = bm[0];
#pragma unroll
            for (int s_ = 1; s_ < kBPL; ++s_) lmax = max(lmax, bm[s_]);
            wbest = wave_max_all(lmax);
            // my best candidate among the slots that hold the wave's maximum: the smallest rank
            unsigned lrank = 0xFFFFFFFFu;
            float lx = 0.f, ly = 0.f, lz = 0.f;
#pragma unroll
            for (int s_ = 0; s_ < kBPL; ++s_) {
                const bool take = bm[s_] == wbest && bm[s_] != kNeg1 && brank[s_] < lrank;
                lrank = take ? brank[s_] : lrank;
                lx = take ? bxx[s_] : lx;
                ly = take ? byy[s_] : ly;
                lz = take ? bzz[s_] : lz;
            }
            unsigned long long cand = __ballot(lrank != 0xFFFFFFFFu);
            if (cand & (cand - 1ull)) {
                const unsigned rmin = wave_min_all(lrank);   // (every lane takes part: no short-circuit in front of it)
                cand = __ballot(lrank == rmin);
            }
            publisher = cand != 0ull && lane == (int)__builtin_ctzll(cand);
            pub_rank = lrank;
            pub_x = lx; pub_y = ly; pub_z = lz;
        }
        const int buf = it & 1;
        if (publisher) {
            s_rec[buf][wave] = make_float4(pub_x, pub_y, pub_z, 0.f);
            const unsigned long long key =
                ((unsigned long long)(unsigned)wbest << 32) | (unsigned long long)(((0xFFFFu - pub_rank) << 4) | (unsigned)wave);
            __hip_atomic_fetch_max(&s_key[kb], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        // D. the winner
        const unsigned klo = (unsigned)s_key[kb];
        const float4 rec = s_rec[buf][klo & 15u];
        cx = rec.x;
        cy = rec.y;
        cz = rec.z;
        const int kb2 = kb == 0 ? 2 : kb - 1;
        kb = kb == 2 ? 0 : kb + 1;
        if (wave == 0) {
            s_idx[it & (kIdxBufP - 1)] = (int)(0xFFFFu - (klo >> 4));
            if (lane == 0) s_key[kb2] = 0ull;
            if ((it & (kIdxBufP - 1)) == kIdxBufP - 1) {
                const int base = it - (kIdxBufP - 1);
                for (int e = lane; e < kIdxBufP; e += 64) idxs[base + e] = unrank16((unsigned)s_idx[e]);
            }
        }
    }
    if (wave == 0) {
        const int base = (m - 1) & ~(kIdxBufP - 1);
        for (int e = lane; base + e < m; e += 64) idxs[base + e] = unrank16((unsigned)s_idx[e]);
    }
    // the running distances back into the caller's order (a wave reads only what it wrote itself)
    __builtin_amdgcn_s_setprio(0);
    for (int e = 0; e < nmine; ++e) {
        const int pos = (bid(e) << 6) + lane;
        if (pos < n) temp[__float_as_int(sorted[pos].w)] = tsort[pos];
    }
}

}  // namespace pruned
}  // namespace epnet
