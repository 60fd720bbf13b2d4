// satail.hip -- the tail of a set-abstraction level's shared MLP for inference on gfx950: the last 1x1 convolution with its
// batch norm folded into the weights, the ReLU and the neighbourhood max-pool in ONE kernel.
//
// In eval mode   max_s relu(bn(conv(x)))[c, p, s]  ==  relu(max_s (W' . x')[c, p, s] + b'[c])   exactly, because `+ b'` and relu
// are monotone: the (B, C, P, S) activation -- the largest tensor of the level -- is never written. The pool is the epilogue of
// one GEMM per scene, (P*S x K) . (K x C), whose rows are reduced in consecutive groups of S.
//
// The rule (include/epnet_ops.h, pinned bit for bit by tests/test_sa_tail_gpu.py): a[c, p, s] is ONE float32 fmaf chain over
// k = 0 .. K-1 ascending from +0, which is what v_mfma_f32_32x32x2_f32 computes when K is walked in order into one accumulator.
// So: no split-K, one accumulator per output; the independent accumulators of a wave belong to different channel tiles.
//
// Layout. x^T is the A operand: lane l holds x'[k0 + (l >> 5)][n0 + (l & 31)], a coalesced dword load of two 128-byte rows and no
// LDS transpose. w^T is the B operand, lane l: w[c0 + (l & 31)][k0 + (l >> 5)], read from a (32 k x channels) chunk that the
// workgroup stages through LDS (zeros where k >= K or c >= C: BOTH operands are padded, 0 * inf would be NaN). The result has the
// output channel on the lane (l & 31) and the tile's 32 columns in the 16 accumulator registers of the two half-waves,
// column = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5): a window of S <= 4 columns is register-local, S = 8, 16, 32 need one
// exchange with lane l ^ 32, and a window of 32 T columns is the running maximum over T consecutive tiles of the same wave.
// A workgroup is 4 waves on 4 neighbouring column spans (of all scenes in one row) and the same CT channel tiles; the next chunk's
// x and w are fetched into registers while the MFMAs of the current chunk run.
#include "common.h"

namespace epnet {

constexpr int kTailThreads = 256;
constexpr int kTailWaves = kTailThreads / kWave;
constexpr int kTailKC = 32;  // k values per staged chunk of w = 16 MFMA steps

typedef float tail_f32x16 __attribute__((ext_vector_type(16)));

// maximum that keeps a NaN (pool_max: a NaN in the window makes the output NaN)
__device__ __forceinline__ float tail_max(float a, float b) {
    const float m = fmaxf(a, b);
    return (a != a || b != b) ? __builtin_nanf("") : m;
}

// the value of lane l ^ 32
__device__ __forceinline__ float tail_other_half(float v) { return __shfl_xor(v, 32, kWave); }

template <int CT>
__global__ __launch_bounds__(kTailThreads) void sa_tail_kernel(int B, int K, int C, int P, int S, int T, int chan_blocks,
                                                               long long spans,
                                                               const float *__restrict__ x, const float *__restrict__ w,
                                                               const float *__restrict__ bias, const float *__restrict__ s_in,
                                                               const float *__restrict__ t_in, int relu_in,
                                                               float *__restrict__ y) {
    constexpr int CB = 32 * CT;      // channels per workgroup
    constexpr int kStride = CB + 1;  // LDS row stride: the transposing writes of the staging step spread over the banks
    __shared__ float ws[kTailKC * kStride];
    __shared__ float ss[kTailKC];
    __shared__ float tt[kTailKC];

    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int cblk = (int)(blockIdx.x % (unsigned)chan_blocks);
    const long long group = (long long)(blockIdx.x / (unsigned)chan_blocks);
    const int c0 = cblk * CB;
    const long long N = (long long)P * S;
    // the spans of all scenes in one row: wave `g` works on span g % spans of scene g / spans (a scene with fewer than four
    // spans -- the GroupAll level -- still fills the workgroup)
    const long long g = group * kTailWaves + wave;
    const bool active = g < (long long)B * spans;
    const int b = active ? (int)(g / spans) : 0;
    const long long span0 = active ? (g - (long long)b * spans) * 32 * T : N;  // first column of this wave's T tiles
    const float *xb = x + (size_t)b * K * N;
    float *yb = y + (size_t)b * C * P;
    const bool affine = s_in != nullptr;
    const int skk = threadIdx.x & 31, scc = threadIdx.x >> 5;  // this thread's part of the staging of w: k and first channel

    float run[CT] = {};  // running window maximum over the tiles (S >= 32)
    for (int t = 0; t < T; ++t) {
        const long long n = span0 + (long long)t * 32 + l31;  // this lane's column of x
        const bool n_ok = n < N;
        tail_f32x16 acc[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

        // the next chunk's operands are fetched into registers while the MFMAs of the current one run
        float xn[kTailKC / 2], wn[CB / 8], sn = 0.f, tn = 0.f;
        auto fetch = [&](int kc) {
#pragma unroll
            for (int j = 0; j < kTailKC / 2; ++j) {
                const int k = kc + 2 * j + half;
                xn[j] = (k < K && n_ok) ? xb[(size_t)k * N + n] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < CB / 8; ++i) {
                const int k = kc + skk, c = c0 + scc + 8 * i;
                wn[i] = (k < K && c < C) ? w[(size_t)c * K + k] : 0.f;
            }
            if (affine && threadIdx.x < kTailKC) {
                const int k = kc + (int)threadIdx.x;
                sn = k < K ? s_in[k] : 0.f;
                tn = k < K ? t_in[k] : 0.f;
            }
        };
        fetch(0);
        for (int kc = 0; kc < K; kc += kTailKC) {
            const int steps = min(kTailKC / 2, (K - kc + 1) / 2);
            __syncthreads();  // the previous chunk has been read
#pragma unroll
            for (int i = 0; i < CB / 8; ++i) ws[skk * kStride + scc + 8 * i] = wn[i];
            if (affine && threadIdx.x < kTailKC) {
                ss[threadIdx.x] = sn;
                tt[threadIdx.x] = tn;
            }
            __syncthreads();
            float xc[kTailKC / 2];
#pragma unroll
            for (int j = 0; j < kTailKC / 2; ++j) {
                const int kk = 2 * j + half;
                float v = xn[j];
                if (affine) v = __builtin_fmaf(v, ss[kk], tt[kk]);
                if (relu_in) v = (v > 0.f || v != v) ? v : 0.f;
                xc[j] = (kc + kk < K && n_ok) ? v : 0.f;  // the padding is of x', after the affine map
            }
            if (kc + kTailKC < K) fetch(kc + kTailKC);
            if (steps == kTailKC / 2) {
#pragma unroll
                for (int j = 0; j < kTailKC / 2; ++j)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[j], ws[(2 * j + half) * kStride + ct * 32 + l31], acc[ct], 0, 0, 0);
            } else {
#pragma unroll
                for (int j = 0; j < kTailKC / 2; ++j) {
                    if (j < steps) {
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[j], ws[(2 * j + half) * kStride + ct * 32 + l31], acc[ct], 0, 0, 0);
                    }
                }
            }
        }

        // epilogue: this lane holds channel c0 + 32 ct + l31 at the tile's columns (r & 3) + 8 (r >> 2) + 4 half
        const long long tile0 = span0 + (long long)t * 32;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int c = c0 + ct * 32 + l31;
            const bool c_ok = c < C;
            const float bc = (c_ok && bias) ? bias[c] : 0.f;
            float *yc = yb + (size_t)(c_ok ? c : 0) * P;
            auto emit = [&](long long col, float m) {  // col: first column of the window
                if (c_ok && col < N) {
                    const float v = m + bc;
                    yc[col / S] = (v > 0.f || v != v) ? v : 0.f;
                }
            };
            const tail_f32x16 a = acc[ct];
            if (S == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) emit(tile0 + (r & 3) + 8 * (r >> 2) + 4 * half, a[r]);
            } else if (S == 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) emit(tile0 + 2 * (i & 1) + 8 * (i >> 1) + 4 * half, tail_max(a[2 * i], a[2 * i + 1]));
            } else {
                float m4[4];  // columns 8 i + 4 half .. + 3
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    m4[i] = tail_max(tail_max(a[4 * i], a[4 * i + 1]), tail_max(a[4 * i + 2], a[4 * i + 3]));
                if (S == 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) emit(tile0 + 8 * i + 4 * half, m4[i]);
                } else if (S == 8) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float m = tail_max(m4[i], tail_other_half(m4[i]));
                        if (half == 0) emit(tile0 + 8 * i, m);
                    }
                } else if (S == 16) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        float m = tail_max(m4[2 * i], m4[2 * i + 1]);
                        m = tail_max(m, tail_other_half(m));
                        if (half == 0) emit(tile0 + 16 * i, m);
                    }
                } else {  // S = 32 T: one window per span
                    float m = tail_max(tail_max(m4[0], m4[1]), tail_max(m4[2], m4[3]));
                    m = tail_max(m, tail_other_half(m));
                    run[ct] = t == 0 ? m : tail_max(run[ct], m);
                    if (t == T - 1 && half == 0) emit(span0, run[ct]);
                }
            }
        }
    }
}

}  // namespace epnet

using namespace epnet;

extern "C" int epnet_sa_tail_f32(int b, int k, int c, int p, int s, const float *x, const float *w, const float *bias,
                                 const float *s_in, const float *t_in, int relu_in, float *y, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && k >= 1 && c >= 1 && p >= 0 && s >= 1);
    EPNET_REQUIRE((s_in == nullptr) == (t_in == nullptr));
    const bool small = s == 1 || s == 2 || s == 4 || s == 8 || s == 16;
    if (!small && s % 32 != 0) return EPNET_ELIMIT;
    const long long n = (long long)p * s;
    if (n > 0x7fffffffll || (long long)k * c > 0x7fffffffll) return EPNET_ELIMIT;
    if (b == 0 || p == 0) return EPNET_OK;
    EPNET_REQUIRE(x && w && y);
    const int t = small ? 1 : s / 32;
    const int ct = c <= 32 ? 1 : c <= 64 ? 2 : 4;
    const long long spans = div_up64(n, 32ll * t), groups = div_up64((long long)b * spans, kTailWaves);
    const int chan_blocks = div_up(c, 32 * ct);
    if (groups * chan_blocks > 0x7fffffffll) return EPNET_ELIMIT;
    const dim3 grid((unsigned)(groups * chan_blocks));
    hipStream_t st = (hipStream_t)stream;
#define EPNET_TAIL(CT_)                                                                                                       \
    hipLaunchKernelGGL((sa_tail_kernel<CT_>), grid, dim3(kTailThreads), 0, st, b, k, c, p, s, t, chan_blocks, spans, x, w, bias, \
                       s_in, t_in, relu_in, y)
    if (ct == 1) EPNET_TAIL(1);
    else if (ct == 2) EPNET_TAIL(2);
    else EPNET_TAIL(4);
#undef EPNET_TAIL
    return check_launch("sa_tail_f32");
}
