// fps_common.h -- what the furthest-point-sampling kernel families share (fps.hip has the overview): the tie-break rank's bit
// reversal, the wave-wide DPP maximum, the register-resident kernels' slot search, and the prologue that stands in for
// fps_prefix_kernel.
#pragma once
#include "common.h"
#include "dpp.h"
#include "spatial.h"

// clang exposes no builtin for v_writelane_b32; bind the LLVM intrinsic by name (value, lane, old)
extern "C" __device__ int epnet_llvm_writelane_i32(int, int, int) __asm("llvm.amdgcn.writelane.i32");

namespace epnet {

__device__ __forceinline__ int writelane_i32(int value, int lane, int old) {
    return epnet_llvm_writelane_i32(value, lane, old);
}

__device__ __forceinline__ unsigned bitrev_lg(unsigned v, int lg) {
    return lg == 0 ? 0u : (__brev(v) >> (32 - lg));
}

// ---- DPP helpers -------------------------------------------------------------------------------
// Distances are handled as their int32 bit patterns: for non-negative floats (and the -1.0f padding
// value, which is a negative int) signed integer order == float order and bit equality == float
// equality, and v_min_i32 / v_max3_i32 need none of the NaN-canonicalising v_max the compiler has to
// put in front of every fminf / fmaxf.
// wave-wide max, returned wave-uniform (scalar registers)
__device__ __forceinline__ int wave_max_i32(int v) {
    const int r = row16_max(v);
    const int a = __builtin_amdgcn_readlane(r, 0), b = __builtin_amdgcn_readlane(r, 16);
    const int c = __builtin_amdgcn_readlane(r, 32), d = __builtin_amdgcn_readlane(r, 48);
    return max(max(a, b), max(c, d));
}

constexpr int kIdxBuf = 4096;  // selected (thread, slot) codes buffered in LDS between flushes

// (thread q, slot s) -> point index. Thread q owns R = bs/T consecutive rank positions r = q*R + s/J
// (reference thread tid = bitreverse(r)) and, of each, the J = ceil(n/bs) points k = tid + j*bs.
__device__ __forceinline__ int fps_point_of(int q, int slot, int R, int J, int lg_bs) {
    const int r = q * R + slot / J;
    return (int)bitrev_lg((unsigned)r, lg_bs) + (slot % J) * (1 << lg_bs);
}

// first slot (lowest index) of lane `wl` whose distance equals `target`, and that point's coordinates
// -- all wave-uniform. Two-level search over groups of 4 slots for PPT >= 8.
template <int PPT>
__device__ __forceinline__ void find_slot(const int (&t)[PPT], const float (&x)[PPT], const float (&y)[PPT],
                                          const float (&z)[PPT], const int (&g)[(PPT + 3) / 4], int wl, int target,
                                          int &slot, float &sx, float &sy, float &sz) {
    slot = 0;
    sx = sy = sz = 0.f;
    if constexpr (PPT >= 8) {
        constexpr int NG = PPT / 4;
        int grp = 0;
#pragma unroll
        for (int gi = NG - 1; gi >= 0; --gi)
            if (__builtin_amdgcn_readlane(g[gi], wl) == target) grp = gi;  // wave-uniform
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
            if (grp == gi) {
#pragma unroll
                for (int j = 4 * gi + 3; j >= 4 * gi; --j)
                    if (__builtin_amdgcn_readlane(t[j], wl) == target) slot = j;
            }
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (slot == j) {
                sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[j]), wl));
                sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y[j]), wl));
                sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[j]), wl));
            }
    } else {
#pragma unroll
        for (int j = PPT - 1; j >= 0; --j)
            if (__builtin_amdgcn_readlane(t[j], wl) == target) {
                slot = j;
                sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[j]), wl));
                sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y[j]), wl));
                sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[j]), wl));
            }
    }
}

// What fps_prefix_kernel does for a scene, as the first thing of a sampling kernel (one workgroup per scene) that can do it
// itself -- one dispatch less on the sampling chain of every level, where a dispatch beside the wide kernels of the pipelined
// stack waits for wave slots (a 6 us prefix kernel was seen to take 77 us there). init < 0: a separate launch has done it.
// Returns whether the scene's first m points are its samples already.
__device__ __forceinline__ bool fps_prologue(int m, const int *__restrict__ skip, int *__restrict__ idx_scene,
                                             int *__restrict__ prefix_out, int init) {
    const int have = skip ? skip[blockIdx.x] : 0;
    if (init >= 0) {
        if (threadIdx.x == 0 && prefix_out) prefix_out[blockIdx.x] = have >= m ? have : init;
        // (a scene whose rounds do run rewrites its indices itself; the known prefix is the same there)
        for (int i = threadIdx.x; i < min(have, m); i += blockDim.x) idx_scene[i] = i;
    }
    return have >= m;
}

}  // namespace epnet
