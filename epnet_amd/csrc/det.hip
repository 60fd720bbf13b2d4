// det.hip -- the deterministic gradients (include/epnet_ops.h, "*_det" entry points) for gfx950.
//
// Every scatter-add gradient of the library (gather_points, group_points, group_concat, three_interpolate, feature_gather)
// is  grad[ch][key(t)] += term(ch, t)  over the entries t of a scene. The default kernels add the terms with float atomics
// (global or LDS), so the summation order -- and the bits -- change from run to run. Here the scatter is inverted in the
// store-and-sum form instead, so that every (target, channel) element is folded by ONE lane in ascending entry order:
//
//   1. keys     key[t] = target of entry t (an entry whose target lies outside [0, n) is flagged and never summed),
//               val[t] = t;
//   2. sort     an LSD radix sort of (key, val) by key, 8 bits per pass, passes = bits of n - 1 (two for n <= 65536). Every
//               pass is a stable counting sort: per-tile digit counts, one exclusive scan per scene (digit-major, so that a
//               digit's tiles follow one another in entry order), and a scatter in which the 256 threads of a tile rank their
//               entries by wave ballots in entry order. So each target's run keeps ascending entry order: a stable
//               inverse index, built with integer LDS counters only;
//   3. bounds   start[j] = first sorted slot of target j (binary search), start[n] = end of the valid entries;
//   4. sum      thread = target j of kRows channel rows: acc = grad[ch][j] (the incoming value), then for the run of j in
//               order acc = acc + term, one fp32 add per term, and one plain store. The terms of a run are read through the
//               sorted values (entry t -> grad_out position t / DIV, weight[t]).
// A long run is not split into partial sums (that would break the sequential contract): a lane walks the whole run of its
// target. Run lengths are skewed, so a wave costs as much as its longest run.
//
// group_linear_grad_w is a full reduction over (scene, position) into (c, 3); its fixed order is
//   block partials:  tiles of kGwTile positions; thread q of a tile sums positions q, q + 256, ... of it in ascending order,
//                    the 64 lanes of a wave are combined by the xor butterfly 32, 16, ..., 1 and the four waves in order;
//   scene totals:    the tile partials of a scene added in ascending tile order (from 0);
//   total:           the scene totals added in ascending scene order (from 0), then grad_w = grad_w + total.
// Nothing in it depends on the stream, the tuning table, the XCD placement or anything but the shape.
// No float atomics, no host synchronisation, no allocation: the scratch is the caller's (*_det_workspace_bytes).
#include "common.h"
#include "taps.h"

namespace epnet {
namespace det {

constexpr int kThreads = 256;
constexpr int kRounds = 16;                    // entries of a sort tile per thread
constexpr int kTile = kThreads * kRounds;      // 4096 entries per sort workgroup
constexpr int kRadix = 256;                    // 8-bit digits
constexpr int kScanThreads = 1024;
constexpr int kRows = 8;                       // channel rows per sum thread (the run's entries are read once for all)
constexpr unsigned kBad = 0x80000000u;         // val flag: target outside [0, n), never summed
constexpr int kGwTile = kThreads * 16;         // group_linear_grad_w: positions per tile
constexpr int kGwRows = 8;

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

inline int passes_of(long long n) {
    int bits = 0;
    for (long long v = n - 1; v > 0; v >>= 1) ++bits;
    return (bits + 7) / 8;
}

// scratch of the scatter gradients: keys and values twice (ping-pong), the tile histograms, the run starts and -- for the
// sampler, whose tap weights are computed -- one weight per entry. Every part is 256-byte aligned.
struct Scratch {
    size_t keys[2], vals[2], hist, start, wt, total;
};

inline Scratch scratch_of(int b, long long p, long long n, bool own_weights) {
    Scratch s;
    const size_t bp = (size_t)b * (size_t)p * 4;
    const size_t nb = (size_t)div_up64(p, kTile);
    size_t off = 0;
    for (int k = 0; k < 2; ++k) {
        s.keys[k] = off; off += align_up(bp);
        s.vals[k] = off; off += align_up(bp);
    }
    s.hist = off; off += align_up((size_t)b * kRadix * nb * 4);
    s.start = off; off += align_up((size_t)b * (size_t)(n + 1) * 4);
    s.wt = off; off += own_weights ? align_up(bp) : 0;
    s.total = off;
    return s;
}

// ---- 1. keys ------------------------------------------------------------------------------------------------------
// an index array of p entries per scene (gather / group: target = idx[t]; three_interpolate: the (n, 3) neighbour array)
__global__ __launch_bounds__(kThreads) void keys_from_index_kernel(int p, int n, const int *__restrict__ idx,
                                                                   unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const int bs = blockIdx.y;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= p) return;
    const size_t o = (size_t)bs * p + t;
    const int j = idx[o];
    const bool ok = j >= 0 && j < n;
    keys[o] = ok ? (unsigned)j : 0u;
    vals[o] = (unsigned)t | (ok ? 0u : kBad);
}

// the sampler: entry 4q + k = tap k (nw, ne, sw, se) of point q, weight as taps_of computes it (sample.hip)
__global__ __launch_bounds__(kThreads) void keys_from_taps_kernel(int h, int w, int npts, int align_corners,
                                                                  const float *__restrict__ xy, unsigned *__restrict__ keys,
                                                                  unsigned *__restrict__ vals, float *__restrict__ wt) {
    const int bs = blockIdx.y;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= npts) return;
    const size_t i = (size_t)bs * npts + q;
    const Taps tp = taps_of(xy[i * 2], xy[i * 2 + 1], h, w, align_corners);
    const int xs[4] = {tp.x0, tp.x0 + 1, tp.x0, tp.x0 + 1}, ys[4] = {tp.y0, tp.y0, tp.y0 + 1, tp.y0 + 1};
    const float ws[4] = {tp.nw, tp.ne, tp.sw, tp.se};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = inside(xs[k], ys[k], h, w);
        const size_t o = i * 4 + k;
        keys[o] = ok ? (unsigned)((long long)ys[k] * w + xs[k]) : 0u;
        vals[o] = (unsigned)(q * 4 + k) | (ok ? 0u : kBad);
        wt[o] = ws[k];
    }
}

// ---- 2. stable radix sort ------------------------------------------------------------------------------------------
// grid (tiles, b): digit counts of one tile -> hist[scene][digit * tiles + tile]
__global__ __launch_bounds__(kThreads) void hist_kernel(int p, int shift, const unsigned *__restrict__ keys,
                                                        unsigned *__restrict__ hist) {
    __shared__ unsigned s_h[kRadix];
    const int bs = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned *k = keys + (size_t)bs * p;
    const long long t0 = (long long)tile * kTile;
    for (int r = 0; r < kRounds; ++r) {
        const long long t = t0 + r * kThreads + threadIdx.x;
        if (t < p) atomicAdd(&s_h[(k[t] >> shift) & (kRadix - 1)], 1u);
    }
    __syncthreads();
    hist[((size_t)bs * kRadix + threadIdx.x) * tiles + tile] = s_h[threadIdx.x];
}

// grid (b): exclusive scan of the len = 256 * tiles counts of a scene, in place
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int len, unsigned *__restrict__ hist) {
    __shared__ unsigned s_sum[kScanThreads];
    unsigned *h = hist + (size_t)blockIdx.x * len;
    const int seg = (len + kScanThreads - 1) / kScanThreads;
    const int i0 = threadIdx.x * seg, i1 = min(len, i0 + seg);
    unsigned sum = 0;
    for (int i = i0; i < i1; ++i) sum += h[i];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {   // inclusive Hillis-Steele scan of the segment sums
        const unsigned v = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = s_sum[threadIdx.x] - sum;
    for (int i = i0; i < i1; ++i) {
        const unsigned v = h[i];
        h[i] = run;
        run += v;
    }
}

// grid (tiles, b): the stable scatter of one tile. Round r places entries t0 + 256 r .. + 255 in entry order: inside a wave
// by ballot matching of the 8 digit bits, across the four waves through per-wave digit counts in LDS, across rounds and
// tiles through the running digit bases.
__global__ __launch_bounds__(kThreads) void scatter_kernel(int p, int shift, const unsigned *__restrict__ keys_in,
                                                           const unsigned *__restrict__ vals_in, unsigned *__restrict__ keys_out,
                                                           unsigned *__restrict__ vals_out, const unsigned *__restrict__ hist) {
    __shared__ unsigned s_base[kRadix];
    __shared__ unsigned s_wc[kThreads / 64][kRadix];
    const int bs = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    s_base[tid] = hist[((size_t)bs * kRadix + tid) * tiles + tile];
    const size_t so = (size_t)bs * p;
    const long long t0 = (long long)tile * kTile;
    for (int r = 0; r < kRounds; ++r) {
        const long long t = t0 + r * kThreads + tid;
        const bool valid = t < p;
        const unsigned key = valid ? keys_in[so + t] : 0u;
        const unsigned val = valid ? vals_in[so + t] : 0u;
        const unsigned d = (key >> shift) & (kRadix - 1);
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1u;
            const unsigned long long bb = __ballot(set);
            m &= set ? bb : ~bb;
        }
        if (!valid) m = 0;
        const unsigned rank = (unsigned)popc_below(m);
        const bool leader = valid && (63 - __builtin_clzll(m)) == lane;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s_wc[w][tid] = 0;
        __syncthreads();
        if (leader) s_wc[wave][d] = (unsigned)__popcll(m);
        __syncthreads();
        if (valid) {
            unsigned slot = s_base[d] + rank;
            for (int w = 0; w < wave; ++w) slot += s_wc[w][d];
            keys_out[so + slot] = key;
            vals_out[so + slot] = val;
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) add += s_wc[w][tid];
        s_base[tid] += add;
        __syncthreads();
    }
}

// ---- 3. run starts -------------------------------------------------------------------------------------------------
// grid (ceil((n + 1) / 256), b): start[j] = first sorted slot whose key >= j (start[n] = p)
__global__ __launch_bounds__(kThreads) void bounds_kernel(int p, int n, const unsigned *__restrict__ keys,
                                                          unsigned *__restrict__ start) {
    const int bs = blockIdx.y;
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j > n) return;
    const unsigned *k = keys + (size_t)bs * p;
    long long lo = 0, hi = p;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)k[mid] < j) lo = mid + 1; else hi = mid;
    }
    start[(size_t)bs * (n + 1) + j] = (unsigned)lo;
}

// ---- 4. the sequential fold ----------------------------------------------------------------------------------------
// grid (ceil(n / 256), ceil(c / kRows), b). DIV: entries per grad_out position (1 gather / group, 3 three_interpolate, 4 sampler).
// grad_out row ch of scene bs starts at grad_out + bs * gstride + ch * row; weights (W) have p per scene.
template <int DIV, bool W>
__global__ __launch_bounds__(kThreads) void sum_kernel(int c, int n, int p, int row, size_t gstride,
                                                       const float *__restrict__ grad_out, const float *__restrict__ weight,
                                                       const unsigned *__restrict__ vals, const unsigned *__restrict__ start,
                                                       float *__restrict__ grad) {
    const int bs = blockIdx.z;
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const int c0 = blockIdx.y * kRows, nr = min(kRows, c - c0);
    const unsigned *st = start + (size_t)bs * (n + 1) + j;
    const unsigned s0 = st[0], s1 = st[1];
    const unsigned *v = vals + (size_t)bs * p;
    const float *wt = W ? weight + (size_t)bs * p : nullptr;
    const float *go = grad_out + (size_t)bs * gstride + (size_t)c0 * row;
    float *g = grad + ((size_t)bs * c + c0) * n + j;
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = r < nr ? g[(size_t)r * n] : 0.f;
    for (unsigned s = s0; s < s1; ++s) {
        const unsigned t = v[s];
        if (t & kBad) continue;
        const unsigned pos = t / DIV;
        const float wv = W ? wt[t] : 1.f;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r < nr) {
                const float x = go[(size_t)r * row + pos];
                acc[r] = acc[r] + (W ? x * wv : x);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r)
        if (r < nr) g[(size_t)r * n] = acc[r];
}

// the whole scatter: keys are in s.keys[0] / s.vals[0] already. The caller has checked every limit (b, ceil(c / kRows), p, n)
// before its key launch, so that a refused shape launches nothing.
template <int DIV, bool W>
static int run_scatter(int b, int c, int n, int p, int row, size_t gstride, const float *grad_out, const float *weight,
                       float *grad, char *ws, const Scratch &s, hipStream_t st, const char *what) {
    const int tiles = (int)div_up64(p, kTile);
    const int passes = passes_of(n);
    int cur = 0;
    for (int pass = 0; pass < passes; ++pass) {
        unsigned *hist = (unsigned *)(ws + s.hist);
        hipLaunchKernelGGL(hist_kernel, dim3(tiles, b), dim3(kThreads), 0, st, p, pass * 8, (const unsigned *)(ws + s.keys[cur]), hist);
        hipLaunchKernelGGL(scan_kernel, dim3(b), dim3(kScanThreads), 0, st, kRadix * tiles, hist);
        hipLaunchKernelGGL(scatter_kernel, dim3(tiles, b), dim3(kThreads), 0, st, p, pass * 8, (const unsigned *)(ws + s.keys[cur]),
                           (const unsigned *)(ws + s.vals[cur]), (unsigned *)(ws + s.keys[cur ^ 1]), (unsigned *)(ws + s.vals[cur ^ 1]),
                           (const unsigned *)hist);
        const int rc = check_launch(what);
        if (rc) return rc;
        cur ^= 1;
    }
    unsigned *start = (unsigned *)(ws + s.start);
    hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)div_up64((long long)n + 1, kThreads), b), dim3(kThreads), 0, st, p, n,
                       (const unsigned *)(ws + s.keys[cur]), start);
    hipLaunchKernelGGL((sum_kernel<DIV, W>), dim3((unsigned)div_up64(n, kThreads), div_up(c, kRows), b), dim3(kThreads), 0, st, c, n,
                       p, row, gstride, grad_out, weight, (const unsigned *)(ws + s.vals[cur]), (const unsigned *)start, grad);
    return check_launch(what);
}

// the index-driven ops: p entries per scene, positions per grad_out row = p / DIV
template <int DIV, bool W>
static int index_scatter(int b, int c, int n, long long p, size_t gstride, const float *grad_out, const int *idx, const float *weight,
                         float *grad, void *workspace, size_t workspace_bytes, hipStream_t st, const char *what) {
    if (b == 0 || c == 0 || p == 0 || n == 0) return EPNET_OK;
    if (!(grad_out && idx && grad && (!W || weight))) return EPNET_EINVAL;
    if (p > 0x7fffffffll || b > 65535 || div_up(c, kRows) > 65535) return EPNET_ELIMIT;
    const Scratch s = scratch_of(b, p, n, false);
    if (!workspace || workspace_bytes < s.total) return EPNET_ENOMEM;
    if ((uintptr_t)workspace & 255) return EPNET_EINVAL;
    char *ws = (char *)workspace;
    hipLaunchKernelGGL(keys_from_index_kernel, dim3((unsigned)div_up64(p, kThreads), b), dim3(kThreads), 0, st, (int)p, n, idx,
                       (unsigned *)(ws + s.keys[0]), (unsigned *)(ws + s.vals[0]));
    const int rc = check_launch(what);
    if (rc) return rc;
    return run_scatter<DIV, W>(b, c, n, (int)p, (int)(p / DIV), gstride, grad_out, weight, grad, ws, s, st, what);
}

// ---- group_linear_grad_w ------------------------------------------------------------------------------------------
// grid (tiles, ceil(c / kGwRows), b): partial[bs][co][tile][k]
__global__ __launch_bounds__(kThreads) void gw_partial_kernel(int c, int n, int npoints, int nsample, int tiles,
                                                              const float *__restrict__ grad_out, const float *__restrict__ xyz,
                                                              const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                              float *__restrict__ partial) {
    __shared__ float s_part[kThreads / 64][kGwRows * 3];
    const int bs = blockIdx.z, tile = blockIdx.x;
    const int c0 = blockIdx.y * kGwRows;
    const int nr = min(kGwRows, c - c0);
    const int p = npoints * nsample;
    const int q_begin = tile * kGwTile, q_end = min(p, q_begin + kGwTile);
    const int *ix = idx + (size_t)bs * p;
    const float *pts = xyz + (size_t)bs * n * 3;
    const float *g = grad_out + ((size_t)bs * c + c0) * p;
    float acc[kGwRows][3];
#pragma unroll
    for (int r = 0; r < kGwRows; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
    for (int q = q_begin + threadIdx.x; q < q_end; q += kThreads) {
        const int id = ix[q];
        const float *pt = pts + (size_t)id * 3;
        const float *ce = new_xyz + ((size_t)bs * npoints + q / nsample) * 3;
        float gv[kGwRows];
#pragma unroll
        for (int r = 0; r < kGwRows; ++r) gv[r] = g[(size_t)min(r, nr - 1) * p + q];
        const float dx = pt[0] - ce[0], dy = pt[1] - ce[1], dz = pt[2] - ce[2];
#pragma unroll
        for (int r = 0; r < kGwRows; ++r) {
            if (r < nr) {
                acc[r][0] = acc[r][0] + gv[r] * dx;
                acc[r][1] = acc[r][1] + gv[r] * dy;
                acc[r][2] = acc[r][2] + gv[r] * dz;
            }
        }
    }
    const int lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < kGwRows; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = wave_sum_f32(acc[r][k]);
            if (lane == 0) s_part[wave][r * 3 + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < nr * 3) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) v = v + s_part[w][threadIdx.x];
        const int r = threadIdx.x / 3, k = threadIdx.x - r * 3;
        partial[(((size_t)bs * c + c0 + r) * tiles + tile) * 3 + k] = v;
    }
}

// grid (ceil(c * 3 / 256), b): scene totals, tiles in ascending order
__global__ __launch_bounds__(kThreads) void gw_scene_kernel(int c, int tiles, const float *__restrict__ partial,
                                                            float *__restrict__ scene) {
    const int bs = blockIdx.y;
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= c * 3) return;
    const int co = e / 3, k = e - co * 3;
    const float *pp = partial + ((size_t)bs * c + co) * tiles * 3 + k;
    float v = 0.f;
    for (int t = 0; t < tiles; ++t) v = v + pp[(size_t)t * 3];
    scene[(size_t)bs * c * 3 + e] = v;
}

// grid (ceil(c * 3 / 256)): scenes in ascending order, then added to grad_w
__global__ __launch_bounds__(kThreads) void gw_final_kernel(int b, int c, const float *__restrict__ scene, float *__restrict__ grad_w) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= c * 3) return;
    float v = 0.f;
    for (int bs = 0; bs < b; ++bs) v = v + scene[(size_t)bs * c * 3 + e];
    grad_w[e] = grad_w[e] + v;
}

inline size_t gw_bytes(int b, int c, long long p, size_t *scene_off) {
    const size_t tiles = (size_t)div_up64(p, kGwTile);
    const size_t part = align_up((size_t)b * c * tiles * 3 * 4);
    if (scene_off) *scene_off = part;
    return part + align_up((size_t)b * c * 3 * 4);
}

}  // namespace det
}  // namespace epnet

using namespace epnet;

// ---- workspace queries: functions of the shape alone -------------------------------------------------------------------
static size_t det_index_bytes(int b, long long p, long long n) {
    if (b <= 0 || p <= 0 || n <= 0) return 0;
    return det::scratch_of(b, p, n, false).total;
}

extern "C" size_t epnet_gather_points_grad_det_workspace_bytes(int b, int n, int npoints) {
    return det_index_bytes(b, npoints, n);
}

extern "C" size_t epnet_group_points_grad_det_workspace_bytes(int b, int n, int npoints, int nsample) {
    return det_index_bytes(b, (long long)npoints * nsample, n);
}

extern "C" size_t epnet_group_concat_grad_det_workspace_bytes(int b, int n, int npoints, int nsample) {
    return det_index_bytes(b, (long long)npoints * nsample, n);
}

extern "C" size_t epnet_three_interpolate_grad_det_workspace_bytes(int b, int n, int m) {
    return det_index_bytes(b, (long long)n * 3, m);
}

extern "C" size_t epnet_feature_gather_grad_det_workspace_bytes(int b, int h, int w, int n) {
    if (b <= 0 || h <= 0 || w <= 0 || n <= 0) return 0;
    return det::scratch_of(b, (long long)n * 4, (long long)h * w, true).total;
}

extern "C" size_t epnet_group_linear_grad_w_det_workspace_bytes(int b, int c, int npoints, int nsample) {
    const long long p = (long long)npoints * nsample;
    if (b <= 0 || c <= 0 || p <= 0) return 0;
    return det::gw_bytes(b, c, p, nullptr);
}

// ---- the entry points ----------------------------------------------------------------------------------------------------
extern "C" int epnet_gather_points_grad_det(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                                            float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0);
    return det::index_scatter<1, false>(b, c, n, npoints, (size_t)c * npoints, grad_out, idx, nullptr, grad_points, workspace,
                                        workspace_bytes, (hipStream_t)stream, "gather_points_grad_det");
}

extern "C" int epnet_group_points_grad_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                           float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0);
    const long long p = (long long)npoints * nsample;
    return det::index_scatter<1, false>(b, c, n, p, (size_t)c * (size_t)p, grad_out, idx, nullptr, grad_points, workspace,
                                        workspace_bytes, (hipStream_t)stream, "group_points_grad_det");
}

extern "C" int epnet_group_concat_grad_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                           float *grad_features, int use_xyz, void *workspace, size_t workspace_bytes,
                                           epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0);
    const long long p = (long long)npoints * nsample;
    if (b == 0 || c == 0 || p == 0 || n == 0) return EPNET_OK;
    EPNET_REQUIRE(grad_out);
    const int ch0 = use_xyz ? 3 : 0;
    return det::index_scatter<1, false>(b, c, n, p, (size_t)(ch0 + c) * (size_t)p, grad_out + (size_t)ch0 * p, idx, nullptr,
                                        grad_features, workspace, workspace_bytes, (hipStream_t)stream, "group_concat_grad_det");
}

extern "C" int epnet_three_interpolate_grad_det(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                                                float *grad_points, void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0);
    return det::index_scatter<3, true>(b, c, m, (long long)n * 3, (size_t)c * n, grad_out, idx, weight, grad_points, workspace,
                                       workspace_bytes, (hipStream_t)stream, "three_interpolate_grad_det");
}

extern "C" int epnet_feature_gather_grad_det(int b, int c, int h, int w, int n, int align_corners, const float *grad_out,
                                             const float *xy, float *grad_feature_map, void *workspace, size_t workspace_bytes,
                                             epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && h >= 0 && w >= 0 && n >= 0);
    if (b == 0 || n == 0 || c == 0) return EPNET_OK;
    EPNET_REQUIRE(grad_out && xy && grad_feature_map && h > 0 && w > 0);
    const long long hw = (long long)h * w, p = (long long)n * 4;
    if (b > 65535 || hw > 0x7fffffffll || p > 0x7fffffffll || div_up(c, det::kRows) > 65535) return EPNET_ELIMIT;
    const det::Scratch s = det::scratch_of(b, p, hw, true);
    if (!workspace || workspace_bytes < s.total) return EPNET_ENOMEM;
    if ((uintptr_t)workspace & 255) return EPNET_EINVAL;
    char *ws = (char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(det::keys_from_taps_kernel, dim3(div_up(n, det::kThreads), b), dim3(det::kThreads), 0, st, h, w, n,
                       align_corners, xy, (unsigned *)(ws + s.keys[0]), (unsigned *)(ws + s.vals[0]), (float *)(ws + s.wt));
    const int rc = check_launch("feature_gather_grad_det");
    if (rc) return rc;
    return det::run_scatter<4, true>(b, c, (int)hw, (int)p, n, (size_t)c * n, grad_out, (const float *)(ws + s.wt), grad_feature_map,
                                     ws, s, st, "feature_gather_grad_det");
}

extern "C" int epnet_group_linear_grad_w_det(int b, int c, int n, int npoints, int nsample, const float *grad_out, const float *xyz,
                                             const float *new_xyz, const int *idx, float *grad_w, void *workspace,
                                             size_t workspace_bytes, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && c >= 0 && n >= 0 && npoints >= 0 && nsample >= 0);
    const long long p = (long long)npoints * nsample;
    if (b == 0 || c == 0 || p == 0) return EPNET_OK;
    EPNET_REQUIRE(grad_out && xyz && new_xyz && idx && grad_w && n > 0);
    const int chunks = div_up(c, det::kGwRows);
    if (p > 0x7fffffffll || b > 65535 || chunks > 65535) return EPNET_ELIMIT;
    size_t scene_off = 0;
    const size_t need = det::gw_bytes(b, c, p, &scene_off);
    if (!workspace || workspace_bytes < need) return EPNET_ENOMEM;
    if ((uintptr_t)workspace & 255) return EPNET_EINVAL;
    const int tiles = (int)div_up64(p, det::kGwTile);
    float *partial = (float *)workspace;
    float *scene = (float *)((char *)workspace + scene_off);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(det::gw_partial_kernel, dim3(tiles, chunks, b), dim3(det::kThreads), 0, st, c, n, npoints, nsample, tiles,
                       grad_out, xyz, new_xyz, idx, partial);
    hipLaunchKernelGGL(det::gw_scene_kernel, dim3(div_up(c * 3, det::kThreads), b), dim3(det::kThreads), 0, st, c, tiles,
                       (const float *)partial, scene);
    hipLaunchKernelGGL(det::gw_final_kernel, dim3(div_up(c * 3, det::kThreads)), dim3(det::kThreads), 0, st, b, c,
                       (const float *)scene, grad_w);
    return check_launch("group_linear_grad_w_det");
}
