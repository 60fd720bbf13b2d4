// rows16.hip -- the SA / FP byte movers on 16-bit feature rows (fp16, bf16) for gfx950.
//
// One rule for every entry point: the result is the value the fp32 op gives on the inputs upcast to fp32,
// rounded ONCE to the 16-bit type -- to nearest, ties to even, denormals kept, overflow to inf, NaN stays NaN. All
// arithmetic is fp32 in the order the fp32 kernels document (group.hip, pool.hip, interpolate.hip), no contraction;
// coordinates, weights, bias and indices stay fp32 / int32. Pure moves (the max-pool, its gradient) carry the 16 bits of the
// element itself, so they are exact whatever the conversion instruction does.
//
// The kernels are the fp32 kernels' designs at half the bytes per feature element: rows staged in LDS as 16-bit (twice the rows
// per workgroup), 16-byte loads that cover 8 elements, four results packed into one 8-byte streaming store. The fp32 files are
// not touched: their kernels stay the same code objects.
#include "common.h"

namespace epnet {

typedef unsigned short u16;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kR16Threads = 256;
constexpr int kR16Chan = 16;               // channels per workgroup of the scalar kernels
constexpr int kR16LdsBudget = 64 * 1024;   // LDS per staged workgroup: two workgroups per CU, as group.hip
constexpr int kR16Unroll = 4;              // 16-byte loads in flight per thread of the pool kernel

// ---- conversions ----------------------------------------------------------------------------------------------------
// DT: EPNET_F16 or EPNET_BF16. up() is exact. down() rounds to nearest even: v_cvt_f16_f32 under the default rounding mode, and
// gfx950's v_cvt_pk_bf16_f32 for bf16 (-DEPNET_ROWS16_INT_CVT: the integer form of the same rounding).
template <int DT>
__device__ __forceinline__ float up(unsigned h) {   // the low 16 bits of h
    if constexpr (DT == EPNET_BF16) {
        return __uint_as_float(h << 16);
    } else {
        return (float)__builtin_bit_cast(_Float16, (u16)h);
    }
}

__device__ __forceinline__ unsigned bf16_bits_int(float f) {
    const unsigned u = __float_as_uint(f);
    if (f != f) return (u >> 16) | 0x40u;                    // quiet, sign and top payload bits kept
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;           // ties to even; carries into the exponent up to inf
}

template <int DT>
__device__ __forceinline__ unsigned down(float f) {  // 16 bits, upper half zero
    if constexpr (DT == EPNET_BF16) {
#ifdef EPNET_ROWS16_INT_CVT
        return bf16_bits_int(f);
#else
        return (unsigned)__builtin_bit_cast(u16, (__bf16)f);
#endif
    } else {
        return (unsigned)__builtin_bit_cast(u16, (_Float16)f);
    }
}

template <int DT>
__device__ __forceinline__ unsigned down2(float lo, float hi) {  // two results in one word, `lo` at the lower address
    if constexpr (DT == EPNET_BF16) {
#ifdef EPNET_ROWS16_INT_CVT
        return bf16_bits_int(lo) | (bf16_bits_int(hi) << 16);
#else
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
#endif
    } else {
        return down<DT>(lo) | (down<DT>(hi) << 16);
    }
}

__device__ __forceinline__ void store_stream8(u16 *dst, unsigned a, unsigned b) {
    const u32x2 v = {a, b};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x2 *>(dst));
}

// ---- group_linear ---------------------------------------------------------------------------------------------------
// out[b, co, m, s] = RN((z[b, co, idx] + (wx[co][0] * dx + wx[co][1] * dy + wx[co][2] * dz)) + bias[co]), group.hip's expression.
// `rows` whole rows of z in LDS as 16-bit; nsample % 4 == 0, idx 16-byte and out 8-byte aligned.
// grid: (tiles, row chunks, scenes); dynamic LDS: rows * n * 2 bytes.
template <int DT, bool BIAS>
__global__ __launch_bounds__(kR16Threads) void group_linear_h_lds_kernel(int c, int n, int npoints, int nsample, int rows, int tile,
                                                                         const u16 *__restrict__ z, const float *__restrict__ xyz,
                                                                         const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                                         const float *__restrict__ wx, const float *__restrict__ bias,
                                                                         u16 *__restrict__ out) {
    extern __shared__ u32x4 s_raw16[];
    u16 *s_rows = reinterpret_cast<u16 *>(s_raw16);
    const int bs = blockIdx.z;
    const int c0 = blockIdx.y * rows;
    const int nr = min(rows, c - c0);
    const int p = npoints * nsample;
    const u16 *src = z + ((size_t)bs * c + c0) * n;
    const int total = nr * n;
    if ((n & 7) == 0 && ((uintptr_t)src & 15) == 0) {
        const u32x4 *src8 = reinterpret_cast<const u32x4 *>(src);
        for (int e = threadIdx.x; e < total / 8; e += kR16Threads) s_raw16[e] = src8[e];
    } else {
        for (int e = threadIdx.x; e < total; e += kR16Threads) s_rows[e] = src[e];
    }
    __syncthreads();
    const int q_begin = blockIdx.x * tile, q_end = min(p, q_begin + tile);
    const int *ix = idx + (size_t)bs * p;
    const float *pts = xyz + (size_t)bs * n * 3;
    u16 *dst_base = out + ((size_t)bs * c + c0) * p;
    for (int q = q_begin + threadIdx.x * 4; q < q_end; q += kR16Threads * 4) {
        const int4 id = *reinterpret_cast<const int4 *>(ix + q);
        const float *ce = new_xyz + ((size_t)bs * npoints + q / nsample) * 3;  // nsample % 4 == 0: one centre per thread
        const float cx = ce[0], cy = ce[1], cz = ce[2];
        const float *p0 = pts + (size_t)id.x * 3, *p1 = pts + (size_t)id.y * 3, *p2 = pts + (size_t)id.z * 3, *p3 = pts + (size_t)id.w * 3;
        const float dx0 = p0[0] - cx, dy0 = p0[1] - cy, dz0 = p0[2] - cz;
        const float dx1 = p1[0] - cx, dy1 = p1[1] - cy, dz1 = p1[2] - cz;
        const float dx2 = p2[0] - cx, dy2 = p2[1] - cy, dz2 = p2[2] - cz;
        const float dx3 = p3[0] - cx, dy3 = p3[1] - cy, dz3 = p3[2] - cz;
        u16 *dst = dst_base + q;
        const u16 *row = s_rows;
#pragma unroll 2
        for (int r = 0; r < nr; ++r) {
            const float w0 = wx[(c0 + r) * 3], w1 = wx[(c0 + r) * 3 + 1], w2 = wx[(c0 + r) * 3 + 2];  // wave-uniform
            float v0 = up<DT>(row[id.x]) + (w0 * dx0 + w1 * dy0 + w2 * dz0);
            float v1 = up<DT>(row[id.y]) + (w0 * dx1 + w1 * dy1 + w2 * dz1);
            float v2 = up<DT>(row[id.z]) + (w0 * dx2 + w1 * dy2 + w2 * dz2);
            float v3 = up<DT>(row[id.w]) + (w0 * dx3 + w1 * dy3 + w2 * dz3);
            if constexpr (BIAS) {
                const float bv = bias[c0 + r];
                v0 += bv; v1 += bv; v2 += bv; v3 += bv;
            }
            store_stream8(dst, down2<DT>(v0, v1), down2<DT>(v2, v3));
            row += n;
            dst += p;
        }
    }
}

// any shape and alignment: one thread per position, kR16Chan channels per block row, z read through L1 / L2
template <int DT, bool BIAS>
__global__ __launch_bounds__(kR16Threads) void group_linear_h_scalar_kernel(int c, int n, int npoints, int nsample,
                                                                            const u16 *__restrict__ z, const float *__restrict__ xyz,
                                                                            const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                                            const float *__restrict__ wx, const float *__restrict__ bias,
                                                                            u16 *__restrict__ out) {
    const int bs = blockIdx.z;
    const int c0 = blockIdx.y * kR16Chan;
    const int p = npoints * nsample;
    const int q = blockIdx.x * kR16Threads + threadIdx.x;
    if (q >= p) return;
    const int id = idx[(size_t)bs * p + q];
    const float *pt = xyz + ((size_t)bs * n + id) * 3;
    const float *ce = new_xyz + ((size_t)bs * npoints + q / nsample) * 3;
    const float dx = pt[0] - ce[0], dy = pt[1] - ce[1], dz = pt[2] - ce[2];
    const int cend = min(c, c0 + kR16Chan);
    for (int ci = c0; ci < cend; ++ci) {
        float v = up<DT>(z[((size_t)bs * c + ci) * n + id]) + (wx[ci * 3] * dx + wx[ci * 3 + 1] * dy + wx[ci * 3 + 2] * dz);
        if constexpr (BIAS) v += bias[ci];
        out[((size_t)bs * c + ci) * p + q] = (u16)down<DT>(v);
    }
}

// ---- pool_max -------------------------------------------------------------------------------------------------------
// pool.hip's rule on the upcast values: NaN outranks everything; otherwise the larger value, then the lower position (-0 == +0
// is a tie). The winner travels as its own 16 bits.
template <int DT>
__device__ __forceinline__ bool pool_better16(unsigned vb, int i, unsigned bb, int bi) {
    const float v = up<DT>(vb), best = up<DT>(bb);
    const bool vn = v != v, bn = best != best;
    if (vn != bn) return vn;
    if (vn) return i < bi;
    return v > best || (v == best && i < bi);
}

// NS = nsample (power of two, 8..256): NS/8 lanes per row, 16 bytes = 8 elements per lane; x 16-byte aligned
template <int DT, int NS>
__global__ __launch_bounds__(kR16Threads) void pool_max_h_vec_kernel(long long rows, const u16 *__restrict__ x, u16 *__restrict__ out,
                                                                     int *__restrict__ arg) {
    constexpr int G = NS / 8;                       // lanes per row (1..32)
    constexpr int kRowsPerPass = kR16Threads / G;   // rows per block per load instruction
    const int sub = threadIdx.x % G;
    const long long row0 = (long long)blockIdx.x * (kRowsPerPass * kR16Unroll) + threadIdx.x / G;
    u32x4 v[kR16Unroll];
#pragma unroll
    for (int u = 0; u < kR16Unroll; ++u) {   // rows past the end re-read the last row (no load under a condition); not stored
        const long long r = min(row0 + (long long)u * kRowsPerPass, rows - 1);
        v[u] = *reinterpret_cast<const u32x4 *>(x + r * NS + sub * 8);
    }
#pragma unroll
    for (int u = 0; u < kR16Unroll; ++u) {
        const long long r = row0 + (long long)u * kRowsPerPass;
        const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        unsigned bb = w[0] & 0xffffu;
        int bi = sub * 8;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const unsigned e = (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu);
            if (pool_better16<DT>(e, sub * 8 + j, bb, bi)) { bb = e; bi = sub * 8 + j; }
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {  // groups are aligned runs of G lanes inside a wave
            const unsigned ob = (unsigned)__shfl_xor((int)bb, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (pool_better16<DT>(ob, oi, bb, bi)) { bb = ob; bi = oi; }
        }
        if (sub == 0 && r < rows) {
            out[r] = (u16)bb;
            if (arg) arg[r] = bi;
        }
    }
}

// any nsample, any alignment: one wave per row
template <int DT>
__global__ __launch_bounds__(kR16Threads) void pool_max_h_row_kernel(long long rows, int ns, const u16 *__restrict__ x,
                                                                     u16 *__restrict__ out, int *__restrict__ arg) {
    const int lane = lane_id();
    const long long r = (long long)blockIdx.x * (kR16Threads / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;   // whole waves leave together
    unsigned bb = 0;
    int bi = 0x7fffffff;  // "nothing yet": loses against any real element of equal value
    bool have = false;
    for (int i = lane; i < ns; i += 64) {
        const unsigned e = x[r * ns + i];
        if (!have || pool_better16<DT>(e, i, bb, bi)) { bb = e; bi = i; have = true; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned ob = (unsigned)__shfl_xor((int)bb, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        const bool oh = __shfl_xor((int)have, off, 64) != 0;
        if (oh && (!have || pool_better16<DT>(ob, oi, bb, bi))) { bb = ob; bi = oi; have = true; }
    }
    if (lane == 0) {
        out[r] = (u16)bb;
        if (arg) arg[r] = bi;
    }
}

// grad_x (rows, ns) = grad_out[row] at arg[row], zero elsewhere: a move of 16 bits, the same kernels for both types.
// ns % 8 == 0, grad_x 16-byte aligned: every element written once, 16 bytes per thread
__global__ __launch_bounds__(kR16Threads) void pool_max_grad_h_vec_kernel(long long rows, int ns, const u16 *__restrict__ grad_out,
                                                                          const int *__restrict__ arg, u16 *__restrict__ grad_x) {
    const int per_row = ns / 8;
    const long long octs = rows * per_row;
    for (long long q = (long long)blockIdx.x * kR16Threads + threadIdx.x; q < octs; q += (long long)gridDim.x * kR16Threads) {
        const long long r = q / per_row;
        const int i0 = (int)(q - r * per_row) * 8;
        const int a = arg[r] - i0;
        const unsigned g = grad_out[r];
        u32x4 o;
        o.x = (a == 0 ? g : 0u) | (a == 1 ? g << 16 : 0u);
        o.y = (a == 2 ? g : 0u) | (a == 3 ? g << 16 : 0u);
        o.z = (a == 4 ? g : 0u) | (a == 5 ? g << 16 : 0u);
        o.w = (a == 6 ? g : 0u) | (a == 7 ? g << 16 : 0u);
        __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(grad_x + q * 8));
    }
}

__global__ __launch_bounds__(kR16Threads) void pool_max_grad_h_kernel(long long rows, int ns, const u16 *__restrict__ grad_out,
                                                                      const int *__restrict__ arg, u16 *__restrict__ grad_x) {
    const long long total = rows * ns;
    for (long long e = (long long)blockIdx.x * kR16Threads + threadIdx.x; e < total; e += (long long)gridDim.x * kR16Threads) {
        const long long r = e / ns;
        grad_x[e] = (int)(e - r * ns) == arg[r] ? grad_out[r] : (u16)0;
    }
}

// ---- three_interpolate ----------------------------------------------------------------------------------------------
// out = RN(w0 * p[i0] + w1 * p[i1] + w2 * p[i2]), left to right (interpolate.hip).
// Staged: rows of `points` in LDS as 16-bit, four channels interleaved per known point ([m] x 8 bytes per group of four rows, as
// three_interpolate_lds4_kernel): one 8-byte LDS read serves four channel rows. rows % 4 == 0 (c % 4 == 0), m % 4 == 0, n % 4 == 0,
// points and out 8-byte aligned; dynamic LDS: rows * m * 2 bytes.
template <int DT, int U>   // unknowns per thread: 4 (8-byte stores), or 1 for the coarse levels (n < 1024)
__global__ __launch_bounds__(kR16Threads) void three_interpolate_h_lds4_kernel(int c, int m, int n, int rows, int tile,
                                                                               const u16 *__restrict__ points, const int *__restrict__ idx,
                                                                               const float *__restrict__ weight, u16 *__restrict__ out) {
    extern __shared__ u32x2 s_quad16[];  // [rows / 4][m]: the four channels of one known point
    int wg_x, wg_y, bs;
    xcd_scene_map3(wg_x, wg_y, bs);   // a scene's idx / weight rows are read by every row chunk: through one XCD's L2
    const int c0 = wg_y * rows;
    const int nr = min(rows, c - c0);  // multiple of 4
    const int groups = nr >> 2, m4 = m >> 2;
    const u16 *src = points + ((size_t)bs * c + c0) * m;
    for (int e = threadIdx.x; e < groups * m4; e += kR16Threads) {
        const int g = e / m4, j4 = e - g * m4;
        const u32x2 *row = reinterpret_cast<const u32x2 *>(src + (size_t)g * 4 * m) + j4;
        const u32x2 a = row[0], b4 = row[m4], cc = row[2 * m4], d = row[3 * m4];
        u32x2 *dst = s_quad16 + g * m + j4 * 4;
        u32x2 t;
        t.x = (a.x & 0xffffu) | (b4.x << 16); t.y = (cc.x & 0xffffu) | (d.x << 16); dst[0] = t;
        t.x = (a.x >> 16) | (b4.x & 0xffff0000u); t.y = (cc.x >> 16) | (d.x & 0xffff0000u); dst[1] = t;
        t.x = (a.y & 0xffffu) | (b4.y << 16); t.y = (cc.y & 0xffffu) | (d.y << 16); dst[2] = t;
        t.x = (a.y >> 16) | (b4.y & 0xffff0000u); t.y = (cc.y >> 16) | (d.y & 0xffff0000u); dst[3] = t;
    }
    __syncthreads();
    const int i_begin = wg_x * tile, i_end = min(n, i_begin + tile);
    u16 *dst_base = out + ((size_t)bs * c + c0) * n;
    for (int i0 = i_begin + threadIdx.x * U; i0 < i_end; i0 += kR16Threads * U) {
        int ix[U][3];
        float w[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ix[u][j] = idx[((size_t)bs * n + i0 + u) * 3 + j];
                w[u][j] = weight[((size_t)bs * n + i0 + u) * 3 + j];
            }
        const u32x2 *quad = s_quad16;
        u16 *dst = dst_base + i0;
        for (int g = 0; g < groups; ++g) {
            u32x2 v[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 3; ++j) v[u][j] = quad[ix[u][j]];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                float o[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float pv[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const unsigned word = ch < 2 ? v[u][j].x : v[u][j].y;
                        pv[j] = up<DT>((ch & 1) ? word >> 16 : word & 0xffffu);
                    }
                    o[u] = w[u][0] * pv[0] + w[u][1] * pv[1] + w[u][2] * pv[2];
                }
                if constexpr (U == 4) store_stream8(dst, down2<DT>(o[0], o[1]), down2<DT>(o[2], o[3]));
                else __builtin_nontemporal_store((u16)down<DT>(o[0]), dst);
                dst += n;
            }
            quad += m;
        }
    }
}

// any shape and alignment: one thread per unknown, kR16Chan channels per block row
template <int DT>
__global__ __launch_bounds__(kR16Threads) void three_interpolate_h_kernel(int c, int m, int n, const u16 *__restrict__ points,
                                                                          const int *__restrict__ idx, const float *__restrict__ weight,
                                                                          u16 *__restrict__ out) {
    int wg_x, wg_y, bs;
    xcd_scene_map3(wg_x, wg_y, bs);
    const int c0 = wg_y * kR16Chan;
    const int i = wg_x * kR16Threads + threadIdx.x;
    if (i >= n) return;
    const int *ix = idx + ((size_t)bs * n + i) * 3;
    const float *w = weight + ((size_t)bs * n + i) * 3;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    const int cend = min(c, c0 + kR16Chan);
    for (int ci = c0; ci < cend; ++ci) {
        const u16 *src = points + ((size_t)bs * c + ci) * m;
        const float v = w0 * up<DT>(src[i0]) + w1 * up<DT>(src[i1]) + w2 * up<DT>(src[i2]);
        out[((size_t)bs * c + ci) * n + i] = (u16)down<DT>(v);
    }
}

}  // namespace epnet

using namespace epnet;

#define EPNET_REQUIRE_DTYPE(dt) EPNET_REQUIRE((dt) == EPNET_F16 || (dt) == EPNET_BF16)

extern "C" int epnet_group_linear_h(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz,
                                    const void *z, const int *idx, const float *w_xyz, const float *bias, void *out, int dtype,
                                    epnet_stream_t stream) {
    EPNET_REQUIRE_DTYPE(dtype);
    EPNET_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0);
    const long long p = (long long)npoints * nsample;
    if (b == 0 || c == 0 || p == 0) return EPNET_OK;
    EPNET_REQUIRE(xyz && new_xyz && z && idx && w_xyz && out && n > 0);
    if (p > 0x7fffffffll || b > 65535 || div_up(c, kR16Chan) > 65535) return EPNET_ELIMIT;
    hipStream_t s = (hipStream_t)stream;
    const u16 *zz = (const u16 *)z;
    u16 *oo = (u16 *)out;
    const bool vec = nsample % 4 == 0 && (uintptr_t)idx % 16 == 0 && (uintptr_t)out % 8 == 0;
    if (vec && (size_t)n * 2 <= (size_t)kR16LdsBudget) {
        int rows = kR16LdsBudget / (n * 2);
        if (rows > c) rows = c;
        if (rows > 64) rows = 64;    // twice group.hip's 32: the same bytes of LDS
        const int max_tiles = (int)(p / 1024);
        // a problem too small to fill the chip with such workgroups (the coarse levels at a few scenes) is bound by the latency of
        // one workgroup, not by bytes: fewer rows each, more of them (measured: profiles/rows16_bench_ops.jsonl)
        while (rows > 16 && (long long)b * div_up(c, rows) * (max_tiles < 1 ? 1 : max_tiles) < 512) rows /= 2;
        const int chunks = div_up(c, rows);
        int tiles = div_up(1024, b * chunks);  // enough workgroups to fill the chip, tiles of at least 1024 positions
        if (tiles > max_tiles) tiles = max_tiles;
        if (tiles < 1) tiles = 1;
        int tile = (int)div_up64(p, tiles);
        tile = (tile + kR16Threads * 4 - 1) / (kR16Threads * 4) * (kR16Threads * 4);
        tiles = (int)div_up64(p, tile);
        if (chunks <= 65535) {
#define EPNET_GLH(DT_, B_)                                                                                                      \
    hipLaunchKernelGGL((group_linear_h_lds_kernel<DT_, B_>), dim3(tiles, chunks, b), dim3(kR16Threads), (size_t)rows * n * 2, s, c, n, \
                       npoints, nsample, rows, tile, zz, xyz, new_xyz, idx, w_xyz, bias, oo)
            if (dtype == EPNET_F16) { if (bias) EPNET_GLH(EPNET_F16, true); else EPNET_GLH(EPNET_F16, false); }
            else { if (bias) EPNET_GLH(EPNET_BF16, true); else EPNET_GLH(EPNET_BF16, false); }
#undef EPNET_GLH
            return check_launch("group_linear_h");
        }
    }
#define EPNET_GLH(DT_, B_)                                                                                                        \
    hipLaunchKernelGGL((group_linear_h_scalar_kernel<DT_, B_>), dim3((unsigned)div_up64(p, kR16Threads), div_up(c, kR16Chan), b),     \
                       dim3(kR16Threads), 0, s, c, n, npoints, nsample, zz, xyz, new_xyz, idx, w_xyz, bias, oo)
    if (dtype == EPNET_F16) { if (bias) EPNET_GLH(EPNET_F16, true); else EPNET_GLH(EPNET_F16, false); }
    else { if (bias) EPNET_GLH(EPNET_BF16, true); else EPNET_GLH(EPNET_BF16, false); }
#undef EPNET_GLH
    return check_launch("group_linear_h");
}

template <int DT>
static int launch_pool_max_h(long long rows, int nsample, const u16 *x, u16 *out, int *arg, hipStream_t s) {
    const bool vec = (nsample & (nsample - 1)) == 0 && nsample >= 8 && nsample <= 256 && ((uintptr_t)x & 15) == 0;
    if (vec) {
        const int g = nsample / 8;
        const long long per_block = (long long)(kR16Threads / g) * kR16Unroll;
        const long long blocks = div_up64(rows, per_block);
        if (blocks > 0x7fffffffll) return EPNET_ELIMIT;
#define EPNET_POOLH(NS_) \
    hipLaunchKernelGGL((pool_max_h_vec_kernel<DT, NS_>), dim3((unsigned)blocks), dim3(kR16Threads), 0, s, rows, x, out, arg)
        switch (nsample) {
            case 8: EPNET_POOLH(8); break;
            case 16: EPNET_POOLH(16); break;
            case 32: EPNET_POOLH(32); break;
            case 64: EPNET_POOLH(64); break;
            case 128: EPNET_POOLH(128); break;
            default: EPNET_POOLH(256); break;
        }
#undef EPNET_POOLH
    } else {
        const long long blocks = div_up64(rows, kR16Threads / 64);
        if (blocks > 0x7fffffffll) return EPNET_ELIMIT;
        hipLaunchKernelGGL((pool_max_h_row_kernel<DT>), dim3((unsigned)blocks), dim3(kR16Threads), 0, s, rows, nsample, x, out, arg);
    }
    return check_launch("pool_max_h");
}

extern "C" int epnet_pool_max_h(long long rows, int nsample, const void *x, void *out, int *arg, int dtype, epnet_stream_t stream) {
    EPNET_REQUIRE_DTYPE(dtype);
    EPNET_REQUIRE(rows >= 0 && nsample >= 1);
    if (rows == 0) return EPNET_OK;
    EPNET_REQUIRE(x && out);
    if (dtype == EPNET_F16) return launch_pool_max_h<EPNET_F16>(rows, nsample, (const u16 *)x, (u16 *)out, arg, (hipStream_t)stream);
    return launch_pool_max_h<EPNET_BF16>(rows, nsample, (const u16 *)x, (u16 *)out, arg, (hipStream_t)stream);
}

extern "C" int epnet_pool_max_grad_h(long long rows, int nsample, const void *grad_out, const int *arg, void *grad_x, int dtype,
                                     epnet_stream_t stream) {
    EPNET_REQUIRE_DTYPE(dtype);
    EPNET_REQUIRE(rows >= 0 && nsample >= 1);
    if (rows == 0) return EPNET_OK;
    EPNET_REQUIRE(grad_out && arg && grad_x);
    hipStream_t s = (hipStream_t)stream;
    const long long total = rows * nsample;
    if (nsample % 8 == 0 && ((uintptr_t)grad_x & 15) == 0) {
        const long long blocks = div_up64(total / 8, kR16Threads);
        hipLaunchKernelGGL(pool_max_grad_h_vec_kernel, dim3((unsigned)(blocks > 1048576 ? 1048576 : blocks)), dim3(kR16Threads), 0, s,
                           rows, nsample, (const u16 *)grad_out, arg, (u16 *)grad_x);
    } else {
        const long long blocks = div_up64(total, kR16Threads);
        hipLaunchKernelGGL(pool_max_grad_h_kernel, dim3((unsigned)(blocks > 1048576 ? 1048576 : blocks)), dim3(kR16Threads), 0, s, rows,
                           nsample, (const u16 *)grad_out, arg, (u16 *)grad_x);
    }
    return check_launch("pool_max_grad_h");
}

template <int DT>
static int launch_three_interpolate_h(int b, int c, int m, int n, const u16 *points, const int *idx, const float *weight, u16 *out,
                                      hipStream_t s) {
    const bool quad_ok = (c & 3) == 0 && (m & 3) == 0 && (n & 3) == 0 && m >= 4 && ((uintptr_t)points & 7) == 0 &&
                         ((uintptr_t)out & 7) == 0;
    if (quad_ok && (size_t)m * 8 <= (size_t)kR16LdsBudget) {
        const bool wide = n >= 1024;             // four unknowns per thread; below, a thread per unknown fills the workgroup
        int rows = kR16LdsBudget / (m * 2);
        if (rows > c) rows = c;
        if (rows > (wide ? 64 : 128)) rows = wide ? 64 : 128;   // twice interpolate.hip's 32 / 64: the same bytes of LDS
        rows &= ~3;
        const int max_tiles = wide ? max(1, n / 2048) : 1;
        // small problems: fewer rows per workgroup, more workgroups (as epnet_group_linear_h)
        while (rows > 16 && (long long)b * div_up(c, rows) * max_tiles < 512) rows = (rows / 2) & ~3;
        const int chunks = div_up(c, rows);
        int tiles = 1, tile = (n + kR16Threads - 1) / kR16Threads * kR16Threads;
        if (wide) {
            tiles = div_up(1024, b * chunks);
            if (tiles > max_tiles) tiles = max_tiles;
            if (tiles < 1) tiles = 1;
            tile = div_up(n, tiles);
            tile = (tile + 1023) / 1024 * 1024;
            tiles = div_up(n, tile);
        }
        if (rows >= 4 && chunks <= 65535) {
            if (wide)
                hipLaunchKernelGGL((three_interpolate_h_lds4_kernel<DT, 4>), dim3(tiles, chunks, b), dim3(kR16Threads),
                                   (size_t)rows * m * 2, s, c, m, n, rows, tile, points, idx, weight, out);
            else
                hipLaunchKernelGGL((three_interpolate_h_lds4_kernel<DT, 1>), dim3(tiles, chunks, b), dim3(kR16Threads),
                                   (size_t)rows * m * 2, s, c, m, n, rows, tile, points, idx, weight, out);
            return check_launch("three_interpolate_h");
        }
    }
    dim3 grid(div_up(n, kR16Threads), div_up(c, kR16Chan), b);
    hipLaunchKernelGGL((three_interpolate_h_kernel<DT>), grid, dim3(kR16Threads), 0, s, c, m, n, points, idx, weight, out);
    return check_launch("three_interpolate_h");
}

extern "C" int epnet_three_interpolate_h(int b, int c, int m, int n, const void *points, const int *idx, const float *weight, void *out,
                                         int dtype, epnet_stream_t stream) {
    EPNET_REQUIRE_DTYPE(dtype);
    EPNET_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0);
    if (b == 0 || c == 0 || n == 0) return EPNET_OK;
    EPNET_REQUIRE(points && idx && weight && out);
    if (b > 65535 || div_up(c, kR16Chan) > 65535) return EPNET_ELIMIT;
    if (dtype == EPNET_F16)
        return launch_three_interpolate_h<EPNET_F16>(b, c, m, n, (const u16 *)points, idx, weight, (u16 *)out, (hipStream_t)stream);
    return launch_three_interpolate_h<EPNET_BF16>(b, c, m, n, (const u16 *)points, idx, weight, (u16 *)out, (hipStream_t)stream);
}
