// imghead.hip -- LI-Fusion's image head evaluated at the points only, for gfx950 (inference).
//
// The end of the two-stream backbone (lib/net/pointnet2_msg.py:237-246) upsamples the four image maps to full resolution with
// kernel == stride transposed convolutions, concatenates them, applies a 1x1 convolution + batch norm + ReLU and then samples
// the result at the projected pixel of every point. In eval mode everything in front of the sampler is pointwise per output
// pixel, so only the pixels under the bilinear taps are evaluated here (contract: include/epnet_ops.h):
//
//   1. ih_transpose_kernel, once per level: F_l (B, C_l, P_l) -> pixel-major (B, P_l, C_l) in the workspace, through a 32 x 33
//      LDS tile. In NCHW a tap's input column is C_l loads a whole plane apart (960 cache lines per tap at the yaml's widths);
//      after the transpose it is one contiguous row of 256 B .. 2 KB. The maps are 59 MB per scene and most of the coarse cells
//      are touched anyway, so the copy is read once + written once at streaming speed.
//   2. counting sort of the 4 * B * n taps by phase (Y % K, X % K), K the largest kernel (the smaller kernels' phases are
//      functions of it): ih_hist_kernel -> ih_scan_kernel -> ih_scatter_kernel. The deconvolution weights differ per phase
//      (61 KB per phase at the yaml's widths); grouped, a workgroup reads one phase's slices once per tile of 64 taps instead
//      of once per tap. Integer atomics only; the order inside a bin is arbitrary and no result depends on it. Taps outside
//      the map are in no bin.
//   3. ih_taps_kernel: one workgroup per tile of 64 taps of one phase. Stage 1: d (tile, sum R) into LDS, one lane per
//      (tap, 4 reduced channels) walking the input row and the phase's (C_l, R_l) slice in ascending channel order. Stage 2:
//      relu(shift + wf . d), one lane per (tap, output channel), written to val (tap id, q). The grid is the shape's upper
//      bound on the tile count; workgroups beyond the data's count leave at once.
//   4. ih_blend_kernel: one lane per (point, channel), the four taps in the sampler's fixed order.
//
// Float16 / bfloat16 maps (epnet_image_head_points_h) take the same steps on 16-bit copies with the two products on MFMA:
// imghead16.h, included below; steps 2 is shared, the float32 kernels here are untouched by it.
#include "common.h"
#include "taps.h"

namespace epnet {

constexpr int kIhMaxLevels = 8;
constexpr int kIhBins = 256;     // phases of a 16 x 16 kernel
constexpr int kIhTile = 64;      // taps per workgroup of ih_taps_kernel
constexpr int kIhThreads = 256;
constexpr int kIhBlendPoints = 32;
constexpr int kIhMaxSumR = 240;  // kIhTile * sum R floats of LDS + the tile's tables <= 64 KB
constexpr int kIhMaxQ = 120;     // kIhBlendPoints * (4 q + 1) floats of LDS + the weights <= 64 KB

struct IhLevel {
    const float *rows;  // (B, hl * wl, c) pixel-major copy of the map
    const float *wd;    // (k, k, c, r)
    int c, k, r, roff, hl, wl;
};

struct IhLevels {
    IhLevel lv[kIhMaxLevels];
    int count, sum_r, kmax;
};

// (B, c, p) -> (B, p, c); grid (ceil(p / 32), ceil(c / 32), B), 256 threads = 32 x 8
__global__ __launch_bounds__(kIhThreads) void ih_transpose_kernel(int c, int p, const float *__restrict__ in, float *__restrict__ out) {
    __shared__ float tile[32][33];
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *src = in + (size_t)blockIdx.z * c * p;
    float *dst = out + (size_t)blockIdx.z * c * p;
    for (int i = ty; i < 32; i += 8) {
        const int ci = c0 + i, pi = p0 + tx;
        if (ci < c && pi < p) tile[i][tx] = src[(size_t)ci * p + pi];
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int pi = p0 + i, ci = c0 + tx;
        if (pi < p && ci < c) dst[(size_t)pi * c + ci] = tile[tx][i];
    }
}

// pixel of tap t (0 nw, 1 ne, 2 sw, 3 se) of a point
__device__ __forceinline__ void tap_pixel(const Taps &tp, int t, int &x, int &y) {
    x = tp.x0 + (t & 1);
    y = tp.y0 + (t >> 1);
}

// count[bin] += the in-bounds taps of that phase; grid ceil(B * n / 256)
__global__ __launch_bounds__(kIhThreads) void ih_hist_kernel(int points, int h, int w, int kmask, int kshift, int align_corners,
                                                             const float *__restrict__ xy, int *__restrict__ count) {
    __shared__ int hist[kIhBins];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int gid = blockIdx.x * kIhThreads + threadIdx.x;
    if (gid < points) {
        const Taps tp = taps_of(xy[(size_t)gid * 2], xy[(size_t)gid * 2 + 1], h, w, align_corners);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int x, y;
            tap_pixel(tp, t, x, y);
            if (inside(x, y, h, w)) atomicAdd(&hist[((y & kmask) << kshift) | (x & kmask)], 1);
        }
    }
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&count[threadIdx.x], hist[threadIdx.x]);
}

// exclusive scans of the counts (offset) and of the tile counts (tileoff), 257 entries each; clears the scatter's cursors
__global__ __launch_bounds__(kIhBins) void ih_scan_kernel(const int *__restrict__ count, int *__restrict__ cursor,
                                                         int *__restrict__ offset, int *__restrict__ tileoff) {
    __shared__ int a[kIhBins], t[kIhBins];
    const int tid = threadIdx.x;
    const int mine = count[tid], tiles = (mine + kIhTile - 1) / kIhTile;
    a[tid] = mine;
    t[tid] = tiles;
    __syncthreads();
    for (int step = 1; step < kIhBins; step <<= 1) {
        const int pa = tid >= step ? a[tid - step] : 0, pt = tid >= step ? t[tid - step] : 0;
        __syncthreads();
        a[tid] += pa;
        t[tid] += pt;
        __syncthreads();
    }
    offset[tid + 1] = a[tid];
    tileoff[tid + 1] = t[tid];
    if (tid == 0) {
        offset[0] = 0;
        tileoff[0] = 0;
    }
    cursor[tid] = 0;
}

// order[offset[bin] + ...] = tap id (point * 4 + t) of every in-bounds tap; a workgroup reserves its share of a bin with one
// atomic per bin and ranks its own taps in LDS
__global__ __launch_bounds__(kIhThreads) void ih_scatter_kernel(int points, int h, int w, int kmask, int kshift, int align_corners,
                                                                const float *__restrict__ xy, const int *__restrict__ offset,
                                                                int *__restrict__ cursor, int *__restrict__ order) {
    __shared__ int hist[kIhBins], base[kIhBins];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int gid = blockIdx.x * kIhThreads + threadIdx.x;
    int bin[4], rank[4];
    if (gid < points) {
        const Taps tp = taps_of(xy[(size_t)gid * 2], xy[(size_t)gid * 2 + 1], h, w, align_corners);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int x, y;
            tap_pixel(tp, t, x, y);
            bin[t] = inside(x, y, h, w) ? (((y & kmask) << kshift) | (x & kmask)) : -1;
            rank[t] = bin[t] >= 0 ? atomicAdd(&hist[bin[t]], 1) : 0;
        }
    }
    __syncthreads();
    base[threadIdx.x] = hist[threadIdx.x] ? offset[threadIdx.x] + atomicAdd(&cursor[threadIdx.x], hist[threadIdx.x]) : 0;
    __syncthreads();
    if (gid < points) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (bin[t] >= 0) order[base[bin[t]] + rank[t]] = gid * 4 + t;
    }
}

// grid: (points * 4) / 64 + 256 workgroups (every non-empty bin ends in at most one partial tile); dynamic LDS: 64 * sum R floats.
// VEC: every level has c % 4 == 0 and r % 4 == 0 and 16-byte aligned weights -- 128-bit loads of the row and the slice; the
// sums run in the same order either way.
template <bool VEC>
__global__ __launch_bounds__(kIhThreads) void ih_taps_kernel(IhLevels lv, int n, int h, int w, int q, int align_corners,
                                                             const float *__restrict__ xy, const float *__restrict__ wf,
                                                             const float *__restrict__ shift, const int *__restrict__ offset,
                                                             const int *__restrict__ tileoff, const int *__restrict__ order,
                                                             float *__restrict__ val) {
    extern __shared__ float d[];  // (kIhTile, sum_r)
    __shared__ int s_bin, s_tile;
    __shared__ int s_tap[kIhTile], s_b[kIhTile], s_x[kIhTile], s_y[kIhTile];
    const int tid = threadIdx.x;
    // consecutive tiles of a phase on one XCD: its slices pass through one L2
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
        const int first = offset[bin] + s_tile * kIhTile + tid;
        int id = -1, bs = 0, x = 0, y = 0;
        if (first < offset[bin + 1]) {
            id = order[first];
            const int point = id >> 2;
            bs = point / n;
            const Taps tp = taps_of(xy[(size_t)point * 2], xy[(size_t)point * 2 + 1], h, w, align_corners);
            tap_pixel(tp, id & 3, x, y);
        }
        s_tap[tid] = id;
        s_b[tid] = bs;
        s_x[tid] = x;
        s_y[tid] = y;
    }
    __syncthreads();
    const int sum_r = lv.sum_r;
    const int py = bin / lv.kmax, px = bin - py * lv.kmax;  // the tile's phase under the largest kernel
    for (int l = 0; l < lv.count; ++l) {
        const IhLevel L = lv.lv[l];
        const float *slice = L.wd + ((size_t)((py & (L.k - 1)) * L.k + (px & (L.k - 1)))) * L.c * L.r;
        if (VEC) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            const int groups = L.r >> 2;
            for (int item = tid; item < kIhTile * groups; item += kIhThreads) {
                const int slot = item / groups, rg = item - slot * groups;
                if (s_tap[slot] < 0) continue;
                const float *row = L.rows + ((size_t)s_b[slot] * L.hl * L.wl + (size_t)(s_y[slot] / L.k) * L.wl + s_x[slot] / L.k) * L.c;
                const float *wcol = slice + rg * 4;
                f4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int ci = 0; ci < L.c; ci += 4) {
                    const f4 f = *reinterpret_cast<const f4 *>(row + ci);
                    const f4 w0 = *reinterpret_cast<const f4 *>(wcol + (size_t)ci * L.r);
                    const f4 w1 = *reinterpret_cast<const f4 *>(wcol + (size_t)(ci + 1) * L.r);
                    const f4 w2 = *reinterpret_cast<const f4 *>(wcol + (size_t)(ci + 2) * L.r);
                    const f4 w3 = *reinterpret_cast<const f4 *>(wcol + (size_t)(ci + 3) * L.r);
                    acc += w0 * f.x;
                    acc += w1 * f.y;
                    acc += w2 * f.z;
                    acc += w3 * f.w;
                }
                float *dst = d + slot * sum_r + L.roff + rg * 4;
                dst[0] = acc.x;
                dst[1] = acc.y;
                dst[2] = acc.z;
                dst[3] = acc.w;
            }
        } else {
            for (int item = tid; item < kIhTile * L.r; item += kIhThreads) {
                const int slot = item / L.r, r = item - slot * L.r;
                if (s_tap[slot] < 0) continue;
                const float *row = L.rows + ((size_t)s_b[slot] * L.hl * L.wl + (size_t)(s_y[slot] / L.k) * L.wl + s_x[slot] / L.k) * L.c;
                float acc = 0.f;
                for (int ci = 0; ci < L.c; ++ci) acc += slice[(size_t)ci * L.r + r] * row[ci];
                d[slot * sum_r + L.roff + r] = acc;
            }
        }
    }
    __syncthreads();
    for (int item = tid; item < kIhTile * q; item += kIhThreads) {
        const int slot = item / q, c = item - slot * q;
        const int id = s_tap[slot];
        if (id < 0) continue;
        const float *wrow = wf + (size_t)c * sum_r;
        const float *drow = d + slot * sum_r;
        float acc = 0.f;
        for (int j = 0; j < sum_r; ++j) acc += wrow[j] * drow[j];
        const float v = shift[c] + acc;
        val[(size_t)id * q + c] = v < 0.f ? 0.f : v;
    }
}

// out[b, c, p] from val (tap id, q); grid (ceil(n / 32), B); dynamic LDS: 32 * (4 q + 1) floats
__global__ __launch_bounds__(kIhThreads) void ih_blend_kernel(int n, int h, int w, int q, int align_corners,
                                                              const float *__restrict__ xy, const float *__restrict__ val,
                                                              float *__restrict__ out) {
    extern __shared__ float v_lds[];  // (32, 4 q + 1): the odd row keeps the 32 points of a read on different banks
    __shared__ float s_w[kIhBlendPoints][4];
    __shared__ int s_in[kIhBlendPoints];
    const int bs = blockIdx.y, p0 = blockIdx.x * kIhBlendPoints, tid = threadIdx.x;
    const int np = min(kIhBlendPoints, n - p0), per = 4 * q;
    const float *src = val + ((size_t)bs * n + p0) * per;
    for (int i = tid; i < np * per; i += kIhThreads) {
        const int pp = i / per;
        v_lds[pp * (per + 1) + (i - pp * per)] = src[i];
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
        const float *pv = v_lds + pp * (per + 1) + c;
        const int in = s_in[pp];
        // a tap outside the map has no value in `val` (whatever the workspace held): selected away, never multiplied
        float v = 0.f;
        v += (in & 1) ? pv[0] * s_w[pp][0] : 0.f;
        v += (in & 2) ? pv[q] * s_w[pp][1] : 0.f;
        v += (in & 4) ? pv[2 * q] * s_w[pp][2] : 0.f;
        v += (in & 8) ? pv[3 * q] * s_w[pp][3] : 0.f;
        out[((size_t)bs * q + c) * n + p0 + pp] = v;
    }
}

struct IhLayout {
    size_t rows[kIhMaxLevels], val, order, tables, total;
    int sum_r, kmax;
};

static size_t ih_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// EPNET_OK and the workspace layout, or the code the entry point returns for these shapes
static int ih_layout(int b, int n, int h, int w, int levels, const int *chans, const int *kernels, const int *reduce, int q,
                     IhLayout &lay) {
    EPNET_REQUIRE(b >= 0 && n >= 0 && h > 0 && w > 0 && levels >= 1 && levels <= kIhMaxLevels && chans && kernels && reduce && q >= 1);
    int kmax = 1;
    long long sum_r = 0;
    for (int l = 0; l < levels; ++l) {
        const int k = kernels[l];
        EPNET_REQUIRE(chans[l] >= 1 && reduce[l] >= 1 && (k == 1 || k == 2 || k == 4 || k == 8 || k == 16));
        if (k > kmax) kmax = k;
        sum_r += reduce[l];
    }
    EPNET_REQUIRE(h % kmax == 0 && w % kmax == 0);
    if (sum_r > kIhMaxSumR || q > kIhMaxQ || b > 65535 || 4ll * b * n > 0x7fffffffll || (long long)h * w > 0x7fffffffll) return EPNET_ELIMIT;
    size_t at = 0;
    for (int l = 0; l < levels; ++l) {
        if (chans[l] > 65535 * 32) return EPNET_ELIMIT;
        lay.rows[l] = at;
        at += ih_round((size_t)b * chans[l] * (h / kernels[l]) * (w / kernels[l]) * sizeof(float));
    }
    lay.val = at;
    at += ih_round((size_t)4 * b * n * q * sizeof(float));
    lay.order = at;
    at += ih_round((size_t)4 * b * n * sizeof(int));
    lay.tables = at;  // count[256], cursor[256], offset[257], tileoff[257]
    at += ih_round((size_t)(2 * kIhBins + 2 * (kIhBins + 1)) * sizeof(int));
    lay.total = at;
    lay.sum_r = (int)sum_r;
    lay.kmax = kmax;
    return EPNET_OK;
}

}  // namespace epnet

#include "imghead16.h"

using namespace epnet;

extern "C" size_t epnet_image_head_points_workspace_bytes(int b, int n, int h, int w, int levels, const int *chans,
                                                          const int *kernels, const int *reduce, int q) {
    IhLayout lay;
    if (ih_layout(b, n, h, w, levels, chans, kernels, reduce, q, lay) != EPNET_OK || b == 0 || n == 0) return 0;
    return lay.total;
}

extern "C" int epnet_image_head_points(int b, int n, int h, int w, int levels, const int *chans, const int *kernels,
                                       const int *reduce, const float *const *maps, const float *const *weights, int q,
                                       const float *wf, const float *shift, const float *xy, int align_corners, float *out,
                                       void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    IhLayout lay;
    const int rc = ih_layout(b, n, h, w, levels, chans, kernels, reduce, q, lay);
    if (rc != EPNET_OK) return rc;
    if (b == 0 || n == 0) return EPNET_OK;
    EPNET_REQUIRE(maps && weights && wf && shift && xy && out);
    for (int l = 0; l < levels; ++l) EPNET_REQUIRE(maps[l] && weights[l]);
    if (!workspace || workspace_bytes < lay.total) return EPNET_ENOMEM;
    EPNET_REQUIRE(((uintptr_t)workspace & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    IhLevels lv;
    lv.count = levels;
    lv.sum_r = lay.sum_r;
    lv.kmax = lay.kmax;
    bool vec = true;
    int roff = 0;
    for (int l = 0; l < levels; ++l) {
        IhLevel &L = lv.lv[l];
        L.rows = (const float *)(ws + lay.rows[l]);
        L.wd = weights[l];
        L.c = chans[l];
        L.k = kernels[l];
        L.r = reduce[l];
        L.roff = roff;
        L.hl = h / L.k;
        L.wl = w / L.k;
        roff += L.r;
        vec = vec && (L.c % 4 == 0) && (L.r % 4 == 0) && (((uintptr_t)L.wd & 15) == 0);
    }
    float *val = (float *)(ws + lay.val);
    int *order = (int *)(ws + lay.order);
    int *count = (int *)(ws + lay.tables), *cursor = count + kIhBins, *offset = cursor + kIhBins, *tileoff = offset + kIhBins + 1;
    int kshift = 0;
    while ((1 << kshift) < lay.kmax) ++kshift;
    const int kmask = lay.kmax - 1, points = b * n;

    for (int l = 0; l < levels; ++l) {
        const IhLevel &L = lv.lv[l];
        const int p = L.hl * L.wl;
        hipLaunchKernelGGL(ih_transpose_kernel, dim3(div_up(p, 32), div_up(L.c, 32), b), dim3(kIhThreads), 0, s, L.c, p, maps[l],
                           (float *)(ws + lay.rows[l]));
    }
    hipError_t e = hipMemsetAsync(count, 0, kIhBins * sizeof(int), s);
    if (e != hipSuccess) return record_hip_error(e, "image_head_points");
    const int point_blocks = div_up(points, kIhThreads);
    hipLaunchKernelGGL(ih_hist_kernel, dim3(point_blocks), dim3(kIhThreads), 0, s, points, h, w, kmask, kshift, align_corners, xy, count);
    hipLaunchKernelGGL(ih_scan_kernel, dim3(1), dim3(kIhBins), 0, s, count, cursor, offset, tileoff);
    hipLaunchKernelGGL(ih_scatter_kernel, dim3(point_blocks), dim3(kIhThreads), 0, s, points, h, w, kmask, kshift, align_corners, xy,
                       offset, cursor, order);
    const int tiles = (int)((4ll * points) / kIhTile) + kIhBins;
    const size_t d_bytes = (size_t)kIhTile * lay.sum_r * sizeof(float);
    if (vec)
        hipLaunchKernelGGL(ih_taps_kernel<true>, dim3(tiles), dim3(kIhThreads), d_bytes, s, lv, n, h, w, q, align_corners, xy, wf, shift,
                           offset, tileoff, order, val);
    else
        hipLaunchKernelGGL(ih_taps_kernel<false>, dim3(tiles), dim3(kIhThreads), d_bytes, s, lv, n, h, w, q, align_corners, xy, wf, shift,
                           offset, tileoff, order, val);
    hipLaunchKernelGGL(ih_blend_kernel, dim3(div_up(n, kIhBlendPoints), b), dim3(kIhThreads),
                       (size_t)kIhBlendPoints * (4 * q + 1) * sizeof(float), s, n, h, w, q, align_corners, xy, val, out);
    return check_launch("image_head_points");
}

extern "C" size_t epnet_image_head_points_h_workspace_bytes(int b, int n, int h, int w, int levels, const int *chans,
                                                            const int *kernels, const int *reduce, int q) {
    IhLayout16 lay;
    if (ih_layout16(b, n, h, w, levels, chans, kernels, reduce, q, lay) != EPNET_OK || b == 0 || n == 0) return 0;
    return lay.total;
}

extern "C" int epnet_image_head_points_h(int b, int n, int h, int w, int levels, const int *chans, const int *kernels,
                                         const int *reduce, int dtype, const void *const *maps, const void *const *weights16, int q,
                                         const void *wf16, const float *shift, const float *xy, int align_corners, void *out,
                                         void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    IhLayout16 lay;
    const int rc = ih_layout16(b, n, h, w, levels, chans, kernels, reduce, q, lay);
    if (rc != EPNET_OK) return rc;
    EPNET_REQUIRE(dtype == EPNET_F16 || dtype == EPNET_BF16);
    if (b == 0 || n == 0) return EPNET_OK;
    EPNET_REQUIRE(maps && weights16 && wf16 && shift && xy && out);
    // maps and out: any 2-byte aligned address; the packs are read with 16-byte loads
    EPNET_REQUIRE(((uintptr_t)wf16 & 15) == 0 && ((uintptr_t)out & 1) == 0);
    for (int l = 0; l < levels; ++l) EPNET_REQUIRE(maps[l] && weights16[l] && ((uintptr_t)maps[l] & 1) == 0 && ((uintptr_t)weights16[l] & 15) == 0);
    if (!workspace || workspace_bytes < lay.total) return EPNET_ENOMEM;
    EPNET_REQUIRE(((uintptr_t)workspace & 15) == 0);
    if (dtype == EPNET_F16)
        return ih_launch16<EPNET_F16>(b, n, h, w, levels, chans, kernels, reduce, lay, maps, weights16, q, wf16, shift, xy, align_corners,
                                      out, (char *)workspace, (hipStream_t)stream);
    return ih_launch16<EPNET_BF16>(b, n, h, w, levels, chans, kernels, reduce, lay, maps, weights16, q, wf16, shift, xy, align_corners,
                                   out, (char *)workspace, (hipStream_t)stream);
}
