// fps_wave.h -- the register-resident sampling kernel for N <= 1024 (and the brute-force fallback up to 16384 points).
#pragma once
#include "fps_common.h"

namespace epnet {

// Register-resident kernel: W waves per scene, PPT point slots per thread. 64*W <= bs = 2^lg_bs,
// R = bs / (64*W), J = ceil(n / bs), R*J <= PPT.
template <int W, int PPT>
__global__ __launch_bounds__(64 * W) void fps_wave_kernel(int n, int m, int lg_bs, const float *__restrict__ xyz,
                                                          float *__restrict__ temp, int *__restrict__ idxs,
                                                          const int *__restrict__ skip, int *__restrict__ prefix_out = nullptr,
                                                          int prologue_init = -1, float *__restrict__ new_xyz = nullptr) {
    // new_xyz (or NULL): the centres xyz[idx] (b, m, 3), written here behind the indices -- the scene is in the cache, and a
    // gather of its own behind this kernel is a dispatch more on the sampling chain (see gather_centres4_kernel)
    if (new_xyz) new_xyz += (size_t)blockIdx.x * m * 3;
    // this scene's first m points are the samples already?
    if (fps_prologue(m, skip, idxs + (size_t)blockIdx.x * m, prefix_out, prologue_init)) {
        if (new_xyz) {
            const float *src = xyz + (size_t)blockIdx.x * n * 3;   // (known prefixes come with m <= n)
            for (int e = threadIdx.x; e < m * 3; e += blockDim.x) new_xyz[e] = src[e];
        }
        return;
    }
    __shared__ int s_val[2][16];     // per-wave maximum (bit pattern)
    __shared__ float4 s_rec[2][16];  // per-wave candidate: x, y, z, (q << 8 | slot) as int bits
    __shared__ int s_idx[kIdxBuf];
    constexpr int T = 64 * W;
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    const int bs = 1 << lg_bs;
    const int R = bs / T, J = (n + bs - 1) / bs;
    const int used = R * J;
    xyz += (size_t)blockIdx.x * n * 3;
    if (temp) temp += (size_t)blockIdx.x * n;
    idxs += (size_t)blockIdx.x * m;
    const int kNeg1 = __float_as_int(-1.f);

    float x[PPT], y[PPT], z[PPT];
    int t[PPT];  // running min squared distance, as bits
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        const int k = s < used ? fps_point_of(q, s, R, J, lg_bs) : n;
        if (k < n) {
            x[s] = xyz[k * 3 + 0];
            y[s] = xyz[k * 3 + 1];
            z[s] = xyz[k * 3 + 2];
            t[s] = __float_as_int(temp ? temp[k] : 1e10f);
        } else {  // padding slot: distance pinned at -1, never a maximum (slot 0 of every thread is real)
            x[s] = y[s] = z[s] = 0.f;
            t[s] = kNeg1;
        }
    }
    if (W > 1 && q < 32) s_val[q >> 4][q & 15] = kNeg1;
    if (q == 0) s_idx[0] = 0;  // code of (thread 0, slot 0) == point 0
    float x1 = xyz[0], y1 = xyz[1], z1 = xyz[2];
    __syncthreads();

    for (int it = 1; it < m; ++it) {
        int g[(PPT + 3) / 4];
        int best = kNeg1;
        if constexpr (PPT >= 8) {
#pragma unroll
            for (int gi = 0; gi < PPT / 4; ++gi) {
                int gm = kNeg1;
#pragma unroll
                for (int j = 4 * gi; j < 4 * gi + 4; ++j) {
                    const float dx = x[j] - x1, dy = y[j] - y1, dz = z[j] - z1;
                    const float d = dx * dx + dy * dy + dz * dz;
                    t[j] = min(__float_as_int(d), t[j]);  // == fminf(d, temp[k]) for d >= 0 (padding: -1 stays)
                    gm = max(gm, t[j]);
                }
                g[gi] = gm;
                best = max(best, gm);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                const float dx = x[j] - x1, dy = y[j] - y1, dz = z[j] - z1;
                const float d = dx * dx + dy * dy + dz * dz;
                t[j] = min(__float_as_int(d), t[j]);
                best = max(best, t[j]);
            }
            g[0] = best;
        }
        // wave arg-max: value by DPP, owner = lowest tied lane, slot = lowest tied slot of that lane
        const int wbest = wave_max_i32(best);
        const unsigned long long tied = __ballot(best == wbest);
        const int wl = (int)__builtin_ctzll(tied);
        int slot;
        float sx, sy, sz;
        find_slot<PPT>(t, x, y, z, g, wl, wbest, slot, sx, sy, sz);
        const int code = ((wave * 64 + wl) << 8) | slot;
        if constexpr (W == 1) {
            x1 = sx;
            y1 = sy;
            z1 = sz;
            s_idx[it & (kIdxBuf - 1)] = code;  // all 64 lanes, same word
        } else {
            const int buf = it & 1;
            if (lane == 0) {
                s_val[buf][wave] = wbest;
                s_rec[buf][wave] = make_float4(sx, sy, sz, __int_as_float(code));
            }
            __syncthreads();  // no global traffic is in flight here: this waits on LDS only
            // one LDS round trip: lane l < 16 fetches wave l's maximum AND record; the winner's record is
            // then picked out of the registers with readlane
            const int wv = s_val[buf][lane & 15];
            const float4 rec = s_rec[buf][lane & 15];
            const int bm = row16_max(wv);
            const unsigned long long wtied = __ballot(wv == bm) & 0xFFFFull;
            const int ww = (int)__builtin_ctzll(wtied);  // lowest tied wave
            x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.x), ww));
            y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.y), ww));
            z1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.z), ww));
            // every lane of wave 0 stores the (uniform) winner code: a store guarded by `q == 0` would let
            // the compiler sink the LDS load feeding the readlane into a single-lane region, where the
            // lane being read has not loaded anything
            const int wcode = __builtin_amdgcn_readlane(__float_as_int(rec.w), ww);
            if (wave == 0) s_idx[it & (kIdxBuf - 1)] = wcode;
        }
        if ((it & (kIdxBuf - 1)) == kIdxBuf - 1 && wave == 0) {  // buffer full: wave 0 (the writer) flushes it
            const int base = it - (kIdxBuf - 1);
            for (int e = lane; e < kIdxBuf; e += 64) {
                const int c = s_idx[e];
                const int k = fps_point_of(c >> 8, c & 0xFF, R, J, lg_bs);
                idxs[base + e] = k;
                if (new_xyz) {
                    float *dst = new_xyz + (size_t)(base + e) * 3;
                    dst[0] = xyz[k * 3 + 0];
                    dst[1] = xyz[k * 3 + 1];
                    dst[2] = xyz[k * 3 + 2];
                }
            }
        }
    }
    if (wave == 0) {
        const int base = (m - 1) & ~(kIdxBuf - 1);
        for (int e = lane; base + e < m; e += 64) {
            const int c = s_idx[e];
            const int k = fps_point_of(c >> 8, c & 0xFF, R, J, lg_bs);
            idxs[base + e] = k;
            if (new_xyz) {
                float *dst = new_xyz + (size_t)(base + e) * 3;
                dst[0] = xyz[k * 3 + 0];
                dst[1] = xyz[k * 3 + 1];
                dst[2] = xyz[k * 3 + 2];
            }
        }
    }
    if (temp) {
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const int k = s < used ? fps_point_of(q, s, R, J, lg_bs) : n;
            if (k < n) temp[k] = __int_as_float(t[s]);
        }
    }
}

}  // namespace epnet
