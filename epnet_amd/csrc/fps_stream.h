// fps_stream.h -- the generic sampling kernel (tiny clouds with a reference block < one wave; clouds beyond the register file),
// with the device counterpart of ref_block_lg's tie-break rank (fps_plan.h) for any block size.
#pragma once
#include "fps_common.h"

namespace epnet {

__device__ __forceinline__ unsigned fps_rank(int k, int lg) {
    return (bitrev_lg((unsigned)k & ((1u << lg) - 1u), lg) << 20) | ((unsigned)k >> lg);
}

__device__ __forceinline__ int fps_unrank(unsigned rank, int lg) {
    return (int)(bitrev_lg(rank >> 20, lg) + ((rank & 0xFFFFFu) << lg));
}

__device__ __forceinline__ long long wave_max_i64(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// xyz and temp re-read through L2 each iteration; arg-max on the 64-bit key
// (bits(d2) << 32) | (0x7fffffff - rank(k)), whose unique maximum is the reference's winner.
// blockDim.x is a multiple of the reference block size 2^lg_bs, so a thread's points share k mod bs.
__global__ __launch_bounds__(1024) void fps_stream_kernel(int n, int m, int lg_bs, const float *__restrict__ xyz,
                                                          float *__restrict__ temp, int *__restrict__ idxs,
                                                          const int *__restrict__ skip) {
    if (skip && skip[blockIdx.x] >= m) return;
    __shared__ long long red[2][16];
    const int BS = blockDim.x;
    const int q = threadIdx.x;
    const int lane = q & 63, wave = q >> 6;
    xyz += (size_t)blockIdx.x * n * 3;
    temp += (size_t)blockIdx.x * n;
    idxs += (size_t)blockIdx.x * m;
    if (q < 32) red[q >> 4][q & 15] = (long long)0x8000000000000000ull;
    if (q == 0) idxs[0] = 0;
    float x1 = xyz[0], y1 = xyz[1], z1 = xyz[2];
    __syncthreads();
    for (int it = 1; it < m; ++it) {
        float best = -1.f;
        int bestk = q;
        for (int k = q; k < n; k += BS) {
            const float dx = xyz[k * 3 + 0] - x1, dy = xyz[k * 3 + 1] - y1, dz = xyz[k * 3 + 2] - z1;
            const float d = dx * dx + dy * dy + dz * dz;
            const float d2 = fminf(d, temp[k]);
            temp[k] = d2;
            bestk = d2 > best ? k : bestk;
            best = d2 > best ? d2 : best;
        }
        // threads beyond n own no point: best = -1 sorts below every real distance (signed high word)
        const unsigned rank = fps_rank(bestk, lg_bs);
        long long key = ((long long)__float_as_int(best) << 32) | (long long)(0x7FFFFFFFu - rank);
        key = wave_max_i64(key);
        if (lane == 0) red[it & 1][wave] = key;
        __syncthreads();
        long long kk = red[it & 1][lane & 15];
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const long long o = __shfl_xor(kk, off, 64);
            kk = o > kk ? o : kk;
        }
        const unsigned wr = 0x7FFFFFFFu - (unsigned)(kk & 0xFFFFFFFFll);
        const int old = __builtin_amdgcn_readfirstlane(fps_unrank(wr, lg_bs));
        x1 = xyz[old * 3 + 0];
        y1 = xyz[old * 3 + 1];
        z1 = xyz[old * 3 + 2];
        if (q == 0) idxs[it] = old;
    }
}

}  // namespace epnet
