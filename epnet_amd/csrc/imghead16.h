// imghead16.h -- the 16-bit kernels of the image head at the points (float16 / bfloat16 maps; DESIGN.md section 4.12, contract:
// include/epnet_ops.h epnet_image_head_points_h). Included by imghead.hip after the float32 kernels: the counting sort
// (ih_hist / ih_scan / ih_scatter) is shared, it reads xy only.
//
//   1. ih_transpose16_kernel, once per level: F_l (B, C_l, P_l) in T -> pixel-major (B, P_l, Cp_l) in T, Cp_l = C_l rounded up
//      to the MFMA's K step of 32, the padding written as zeros (0 * inf of a neighbouring row would be a NaN).
//   3. ih_taps16_kernel: one workgroup per tile of 64 taps of one phase, one wave per 16 taps = one row block of
//      v_mfma_f32_16x16x32_{f16,bf16}. Stage 1, per level: (16 x Cp_l) x (Cp_l x R_l) with the A fragments straight from the
//      pixel-major rows (lane: 8 consecutive channels, one 16-byte load) and the B fragments from the fragment-ordered pack (a
//      wave's fragment is 1 KB contiguous); d rounded to T into LDS. Stage 2: (16 x sum R) x (sum R x q) from LDS and the packed
//      1x1 weight, relu(shift + .) into val. A wave reads only the rows of d it wrote. Every row of an MFMA result depends on its
//      own A row alone, so a tap's value does not depend on the tile it lands in.
//   4. ih_blend16_kernel: ih_blend_kernel with the result rounded once to T.
#pragma once

namespace epnet {

typedef unsigned short ih_u16;
typedef unsigned ih_u32x4 __attribute__((ext_vector_type(4)));
typedef float ih_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIhKStep = 32;      // K of the MFMA: the channel padding of the copies and the packs
constexpr int kIhNBlock = 16;     // N of the MFMA: the padding of R_l and q in the packs
constexpr int kIhDPad = 8;        // elements between the rows of d in LDS: rows 16 bytes off the 128-byte bank period
constexpr int kIhT16Pixels = 64;  // pixels per workgroup of the transpose

inline int ih_pad(int v, int to) { return (v + to - 1) / to * to; }

template <int DT>
__device__ __forceinline__ unsigned ih_down(float f) {  // round to nearest even, denormals kept, overflow to inf
    if constexpr (DT == EPNET_BF16) {
        return (unsigned)__builtin_bit_cast(ih_u16, (__bf16)f);
    } else {
        return (unsigned)__builtin_bit_cast(ih_u16, (_Float16)f);
    }
}

template <int DT>
__device__ __forceinline__ ih_f32x4 ih_mfma(ih_u32x4 a, ih_u32x4 b, ih_f32x4 acc) {
    if constexpr (DT == EPNET_BF16) {
        typedef __bf16 frag __attribute__((ext_vector_type(8)));
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), acc, 0, 0, 0);
    } else {
        typedef _Float16 frag __attribute__((ext_vector_type(8)));
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), acc, 0, 0, 0);
    }
}

struct IhLevel16 {
    const ih_u16 *rows;  // (B, hl * wl, cp) pixel-major copy of the map
    const ih_u16 *wd;    // (k, k, rp / 16, cp / 32, 64, 8): include/epnet_ops.h
    int cp, k, r, rp, roff, hl, wl;
};

struct IhLevels16 {
    IhLevel16 lv[kIhMaxLevels];
    int count, sum_rp, kmax;  // sum_rp: sum R rounded up to 32
};

// (B, c, p) -> (B, p, cp), channels c .. cp - 1 zero; grid (ceil(p / 64), cp / 32, B), 256 threads. PAIRS: `in` is 4-byte aligned
// and p is even, so every channel's plane is -- one 4-byte load per two pixels; else 2-byte loads.
template <bool PAIRS>
__global__ __launch_bounds__(kIhThreads) void ih_transpose16_kernel(int c, int cp, int p, const ih_u16 *__restrict__ in,
                                                                    ih_u16 *__restrict__ out) {
    __shared__ ih_u16 tile[32][kIhT16Pixels + 2];
    const int p0 = blockIdx.x * kIhT16Pixels, c0 = blockIdx.y * 32, tid = threadIdx.x;
    const ih_u16 *src = in + (size_t)blockIdx.z * c * p;
    ih_u16 *dst = out + (size_t)blockIdx.z * cp * p;
    if (PAIRS) {
        const int tx = tid & 31, ty = tid >> 5;
        for (int i = ty; i < 32; i += 8) {
            const int ci = c0 + i, pi = p0 + 2 * tx;
            unsigned v = 0;
            if (ci < c && pi < p) v = *reinterpret_cast<const unsigned *>(src + (size_t)ci * p + pi);  // p even: pi + 1 < p too
            tile[i][2 * tx] = (ih_u16)(v & 0xffffu);
            tile[i][2 * tx + 1] = (ih_u16)(v >> 16);
        }
    } else {
        const int tx = tid & 63, ty = tid >> 6;
        for (int i = ty; i < 32; i += 4) {
            const int ci = c0 + i, pi = p0 + tx;
            tile[i][tx] = (ci < c && pi < p) ? src[(size_t)ci * p + pi] : (ih_u16)0;
        }
    }
    __syncthreads();
    const int px = tid & 63, g = tid >> 6;  // 8 channels of one pixel per thread: one 16-byte store
    if (p0 + px < p) {
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (unsigned)tile[g * 8 + 2 * j][px] | ((unsigned)tile[g * 8 + 2 * j + 1][px] << 16);
        const ih_u32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<ih_u32x4 *>(dst + (size_t)(p0 + px) * cp + c0 + g * 8) = o;
    }
}

// grid: (points * 4) / 64 + 256 workgroups, as ih_taps_kernel; dynamic LDS: 64 * (sum_rp + 8) 16-bit elements
template <int DT>
__global__ __launch_bounds__(kIhThreads) void ih_taps16_kernel(IhLevels16 lv, int n, int h, int w, int q, int align_corners,
                                                               const float *__restrict__ xy, const ih_u16 *__restrict__ wf,
                                                               const float *__restrict__ shift, const int *__restrict__ offset,
                                                               const int *__restrict__ tileoff, const int *__restrict__ order,
                                                               float *__restrict__ val) {
    extern __shared__ ih_u16 d16[];  // (kIhTile, sum_rp + kIhDPad)
    __shared__ int s_bin, s_tile;
    __shared__ int s_tap[kIhTile], s_b[kIhTile], s_x[kIhTile], s_y[kIhTile];
    const int tid = threadIdx.x;
    int wg, unused;
    xcd_scene_map(wg, unused);
    if (tid == 0) s_bin = -1;
    __syncthreads();
    {
        const int lo = tileoff[tid], hi = tileoff[tid + 1];
        if (wg >= lo && wg < hi) {
            s_bin = tid;
            s_tile = wg - lo;
        }
    }
    __syncthreads();
    const int bin = s_bin;
    if (bin < 0) return;
    if (tid < kIhTile) {
        // a slot beyond the bin's end reads the pixel of the tile's first tap (always there) and is discarded
        const int first = offset[bin] + s_tile * kIhTile, mine = first + tid;
        const bool valid = mine < offset[bin + 1];
        const int id = order[valid ? mine : first];
        const int point = id >> 2;
        const Taps tp = taps_of(xy[(size_t)point * 2], xy[(size_t)point * 2 + 1], h, w, align_corners);
        int x, y;
        tap_pixel(tp, id & 3, x, y);
        s_tap[tid] = valid ? id : -1;
        s_b[tid] = point / n;
        s_x[tid] = x;
        s_y[tid] = y;
    }
    const int pitch = lv.sum_rp + kIhDPad;
    // the columns sum R .. sum_rp - 1 of d are K padding of stage 2: zeros (every level's own columns are written below)
    for (int i = tid; i < kIhTile * kIhKStep; i += kIhThreads) {
        const int slot = i / kIhKStep;
        d16[slot * pitch + lv.sum_rp - kIhKStep + (i - slot * kIhKStep)] = 0;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int arow = wave * 16 + (lane & 15), kq = lane >> 4;  // the A row this lane feeds, its 8-channel quarter of a K step
    const int py = bin / lv.kmax, px = bin - py * lv.kmax;     // the tile's phase under the largest kernel
    const int ab = s_b[arow], ax = s_x[arow], ay = s_y[arow];
    for (int l = 0; l < lv.count; ++l) {
        const IhLevel16 L = lv.lv[l];
        const int ksteps = L.cp / kIhKStep, nblocks = L.rp / kIhNBlock;
        const ih_u16 *row = L.rows + ((size_t)ab * L.hl * L.wl + (size_t)(ay / L.k) * L.wl + ax / L.k) * L.cp + kq * 8;
        const ih_u16 *slice = L.wd + (size_t)((py & (L.k - 1)) * L.k + (px & (L.k - 1))) * L.rp * L.cp + lane * 8;
        for (int nb = 0; nb < nblocks; ++nb) {
            const ih_u16 *bsrc = slice + (size_t)nb * ksteps * 512;
            ih_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < ksteps; ++ks) {
                const ih_u32x4 a = *reinterpret_cast<const ih_u32x4 *>(row + ks * kIhKStep);
                const ih_u32x4 bf = *reinterpret_cast<const ih_u32x4 *>(bsrc + ks * 512);
                acc = ih_mfma<DT>(a, bf, acc);
            }
            // result: column = lane & 15, rows = kq * 4 + i
            const int r = nb * kIhNBlock + (lane & 15);
            if (r < L.r) {
#pragma unroll
                for (int i = 0; i < 4; ++i) d16[(wave * 16 + kq * 4 + i) * pitch + L.roff + r] = (ih_u16)ih_down<DT>(acc[i]);
            }
        }
    }
    __syncthreads();
    const int ksteps2 = lv.sum_rp / kIhKStep, qblocks = (q + kIhNBlock - 1) / kIhNBlock;
    const ih_u16 *drow = d16 + arow * pitch + kq * 8;
    int ids[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ids[i] = s_tap[wave * 16 + kq * 4 + i];
    for (int qb = 0; qb < qblocks; ++qb) {
        const ih_u16 *bsrc = wf + (size_t)qb * ksteps2 * 512 + lane * 8;
        ih_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps2; ++ks) {
            const ih_u32x4 a = *reinterpret_cast<const ih_u32x4 *>(drow + ks * kIhKStep);
            const ih_u32x4 bf = *reinterpret_cast<const ih_u32x4 *>(bsrc + ks * 512);
            acc = ih_mfma<DT>(a, bf, acc);
        }
        const int c = qb * kIhNBlock + (lane & 15);
        if (c < q) {
            const float sh = shift[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (ids[i] < 0) continue;
                const float v = sh + acc[i];
                val[(size_t)ids[i] * q + c] = v < 0.f ? 0.f : v;
            }
        }
    }
}

// ih_blend_kernel, the sum rounded once to T; grid (ceil(n / 32), B); dynamic LDS: 32 * (4 q + 1) floats
template <int DT>
__global__ __launch_bounds__(kIhThreads) void ih_blend16_kernel(int n, int h, int w, int q, int align_corners,
                                                                const float *__restrict__ xy, const float *__restrict__ val,
                                                                ih_u16 *__restrict__ out) {
    extern __shared__ float v_lds16[];  // (32, 4 q + 1)
    __shared__ float s_w[kIhBlendPoints][4];
    __shared__ int s_in[kIhBlendPoints];
    const int bs = blockIdx.y, p0 = blockIdx.x * kIhBlendPoints, tid = threadIdx.x;
    const int np = min(kIhBlendPoints, n - p0), per = 4 * q;
    const float *src = val + ((size_t)bs * n + p0) * per;
    for (int i = tid; i < np * per; i += kIhThreads) {
        const int pp = i / per;
        v_lds16[pp * (per + 1) + (i - pp * per)] = src[i];
    }
    if (tid < np) {
        const size_t point = (size_t)bs * n + p0 + tid;
        const Taps tp = taps_of(xy[point * 2], xy[point * 2 + 1], h, w, align_corners);
        s_w[tid][0] = tp.nw;
        s_w[tid][1] = tp.ne;
        s_w[tid][2] = tp.sw;
        s_w[tid][3] = tp.se;
        int in = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int x, y;
            tap_pixel(tp, t, x, y);
            in |= inside(x, y, h, w) ? (1 << t) : 0;
        }
        s_in[tid] = in;
    }
    __syncthreads();
    for (int item = tid; item < kIhBlendPoints * q; item += kIhThreads) {
        const int pp = item & (kIhBlendPoints - 1), c = item / kIhBlendPoints;
        if (pp >= np) continue;
        const float *pv = v_lds16 + pp * (per + 1) + c;
        const int in = s_in[pp];
        float v = 0.f;
        v += (in & 1) ? pv[0] * s_w[pp][0] : 0.f;
        v += (in & 2) ? pv[q] * s_w[pp][1] : 0.f;
        v += (in & 4) ? pv[2 * q] * s_w[pp][2] : 0.f;
        v += (in & 8) ? pv[3 * q] * s_w[pp][3] : 0.f;
        out[((size_t)bs * q + c) * n + p0 + pp] = (ih_u16)ih_down<DT>(v);
    }
}

struct IhLayout16 {
    size_t rows[kIhMaxLevels], val, order, tables, total;
    int cp[kIhMaxLevels], rp[kIhMaxLevels];
    int sum_r, sum_rp, kmax;
};

// ih_layout's checks, with the 16-bit padded copies in place of the float32 ones
static int ih_layout16(int b, int n, int h, int w, int levels, const int *chans, const int *kernels, const int *reduce, int q,
                       IhLayout16 &lay) {
    IhLayout base;
    const int rc = ih_layout(b, n, h, w, levels, chans, kernels, reduce, q, base);
    if (rc != EPNET_OK) return rc;
    size_t at = 0;
    for (int l = 0; l < levels; ++l) {
        lay.cp[l] = ih_pad(chans[l], kIhKStep);
        lay.rp[l] = ih_pad(reduce[l], kIhNBlock);
        lay.rows[l] = at;
        at += ih_round((size_t)b * lay.cp[l] * (h / kernels[l]) * (w / kernels[l]) * sizeof(ih_u16));
    }
    lay.val = at;
    at += ih_round((size_t)4 * b * n * q * sizeof(float));
    lay.order = at;
    at += ih_round((size_t)4 * b * n * sizeof(int));
    lay.tables = at;
    at += ih_round((size_t)(2 * kIhBins + 2 * (kIhBins + 1)) * sizeof(int));
    lay.total = at;
    lay.sum_r = base.sum_r;
    lay.sum_rp = ih_pad(base.sum_r, kIhKStep);
    lay.kmax = base.kmax;
    return EPNET_OK;
}

template <int DT>
static int ih_launch16(int b, int n, int h, int w, int levels, const int *chans, const int *kernels, const int *reduce,
                       const IhLayout16 &lay, const void *const *maps, const void *const *weights16, int q, const void *wf16,
                       const float *shift, const float *xy, int align_corners, void *out, char *ws, hipStream_t s) {
    IhLevels16 lv;
    lv.count = levels;
    lv.sum_rp = lay.sum_rp;
    lv.kmax = lay.kmax;
    int roff = 0;
    for (int l = 0; l < levels; ++l) {
        IhLevel16 &L = lv.lv[l];
        L.rows = (const ih_u16 *)(ws + lay.rows[l]);
        L.wd = (const ih_u16 *)weights16[l];
        L.cp = lay.cp[l];
        L.k = kernels[l];
        L.r = reduce[l];
        L.rp = lay.rp[l];
        L.roff = roff;
        L.hl = h / L.k;
        L.wl = w / L.k;
        roff += L.r;
    }
    float *val = (float *)(ws + lay.val);
    int *order = (int *)(ws + lay.order);
    int *count = (int *)(ws + lay.tables), *cursor = count + kIhBins, *offset = cursor + kIhBins, *tileoff = offset + kIhBins + 1;
    int kshift = 0;
    while ((1 << kshift) < lay.kmax) ++kshift;
    const int kmask = lay.kmax - 1, points = b * n;

    for (int l = 0; l < levels; ++l) {
        const IhLevel16 &L = lv.lv[l];
        const int p = L.hl * L.wl;
        const dim3 grid(div_up(p, kIhT16Pixels), L.cp / 32, b);
        ih_u16 *dst = (ih_u16 *)(ws + lay.rows[l]);
        if ((((uintptr_t)maps[l]) & 3) == 0 && (p & 1) == 0)
            hipLaunchKernelGGL(ih_transpose16_kernel<true>, grid, dim3(kIhThreads), 0, s, chans[l], L.cp, p, (const ih_u16 *)maps[l], dst);
        else
            hipLaunchKernelGGL(ih_transpose16_kernel<false>, grid, dim3(kIhThreads), 0, s, chans[l], L.cp, p, (const ih_u16 *)maps[l], dst);
    }
    hipError_t e = hipMemsetAsync(count, 0, kIhBins * sizeof(int), s);
    if (e != hipSuccess) return record_hip_error(e, "image_head_points_h");
    const int point_blocks = div_up(points, kIhThreads);
    hipLaunchKernelGGL(ih_hist_kernel, dim3(point_blocks), dim3(kIhThreads), 0, s, points, h, w, kmask, kshift, align_corners, xy, count);
    hipLaunchKernelGGL(ih_scan_kernel, dim3(1), dim3(kIhBins), 0, s, count, cursor, offset, tileoff);
    hipLaunchKernelGGL(ih_scatter_kernel, dim3(point_blocks), dim3(kIhThreads), 0, s, points, h, w, kmask, kshift, align_corners, xy,
                       offset, cursor, order);
    const int tiles = (int)((4ll * points) / kIhTile) + kIhBins;
    const size_t d_bytes = (size_t)kIhTile * (lay.sum_rp + kIhDPad) * sizeof(ih_u16);
    hipLaunchKernelGGL(ih_taps16_kernel<DT>, dim3(tiles), dim3(kIhThreads), d_bytes, s, lv, n, h, w, q, align_corners, xy,
                       (const ih_u16 *)wf16, shift, offset, tileoff, order, val);
    hipLaunchKernelGGL(ih_blend16_kernel<DT>, dim3(div_up(n, kIhBlendPoints), b), dim3(kIhThreads),
                       (size_t)kIhBlendPoints * (4 * q + 1) * sizeof(float), s, n, h, w, q, align_corners, xy, val, (ih_u16 *)out);
    return check_launch("image_head_points_h");
}

}  // namespace epnet
