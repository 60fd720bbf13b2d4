// scan.hip -- the RPN inputs of a whole batch from the raw scans, with no host synchronisation (include/epnet_ops.h,
// epnet_scan_prepare and epnet_image_normalise) for gfx950.
//
// The reference does this per scene on a host core, in the first half of get_rpn_with_li_fusion
// (lib/datasets/kitti_rcnn_dataset.py:281-356): Calibration.lidar_to_rect and rect_to_img (lib/utils/calibration.py:51-70),
// get_valid_flag (:229-251), then every point at 40 m or farther plus a random subset of the nearer ones (:325-346) and a
// shuffle. Here the draws are device tables (one key per raw point, one slot permutation per scene), so that the subset is
// "the r smallest keys" and nothing is read back. Four launches, whatever the data:
//
//   1. classify, grid (tiles of 2048 raw points, scenes): 16-byte coalesced row loads, the transform, the view / scope test;
//      the wave ballots of `valid` and `valid and near` go to the workspace as 64-bit words, with the tile's V and F counts;
//   2. plan, one workgroup per scene: sums the tile counts, decides the case, q and r (the header's table) and finds the
//      r-th smallest candidate key by a four-pass 8-bit radix select -- integer LDS histograms over the keys whose bit is
//      set in the stored ballots -- which gives the threshold key and how many of the keys equal to it are admitted (in raw order);
//   3. count, grid as 1: per tile, the candidates below the threshold and those at it (popcounts of ballots);
//   4. emit, grid as 1: each workgroup sums the counts of the tiles before it, ranks its own points by mask popcounts,
//      re-reads the rows of the chosen points, transforms them again and writes them at slot_perm[position].
// No float atomics and no data-dependent launch: the bits depend on the inputs alone.
//
// Arithmetic: fp32 in source order without contraction, `/` correctly rounded (the conventions of epnet_kitti_records); the
// scope test compares (double)coordinate against the double bound.
#include "common.h"
#include "cr_trig.h"

namespace epnet {
namespace scan {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kIters = 8;                          // ballots per wave and tile
constexpr int kTile = kThreads * kIters;           // raw points per workgroup
constexpr int kWords = kTile / kWave;              // 64-bit mask words per tile
constexpr int kPlanThreads = 1024;
constexpr int kPlanUnroll = 8;                     // independent loads per thread in the plan's key passes
constexpr int kPlanInts = 8;                       // case, q, r, threshold key, admitted ties, candidate set, forced set, its size

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

enum Set { kNone = 0, kValid = 1, kNear = 2, kFar = 3 };

struct Scope {
    double v[6];
};

// where the pieces of the workspace start (bytes from its base); words = kWords * tiles per scene
struct Layout {
    size_t valid, near, tile_cnt, plan, tile_sel, total;
};

__host__ __device__ inline Layout layout(int b, int tiles, int cnt_ints = 2) {
    Layout l;
    const size_t words = (size_t)b * (size_t)tiles * kWords;
    l.valid = 0;
    l.near = l.valid + words * 8;
    l.tile_cnt = l.near + words * 8;
    l.plan = l.tile_cnt + (size_t)b * tiles * cnt_ints * sizeof(int);
    l.tile_sel = l.plan + (size_t)b * kPlanInts * sizeof(int);
    l.total = l.tile_sel + (size_t)b * tiles * 2 * sizeof(int);
    return l;
}

struct Calib {
    float m[4][3];   // the composite of V2C and R0
    float p[3][4];   // P2
    float w, h;
};

__device__ __forceinline__ Calib load_calib(const float *__restrict__ V2C, const float *__restrict__ R0, const float *__restrict__ P2,
                                            const int *__restrict__ img_shape, int bs) {
    Calib c;
    const float *v = V2C + (size_t)bs * 12, *r = R0 + (size_t)bs * 9, *p = P2 + (size_t)bs * 12;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[k][j] = (v[k] * r[j * 3] + v[4 + k] * r[j * 3 + 1]) + v[8 + k] * r[j * 3 + 2];
#pragma unroll
    for (int k = 0; k < 12; ++k) c.p[k / 4][k % 4] = p[k];
    c.h = (float)img_shape[(size_t)bs * 2];
    c.w = (float)img_shape[(size_t)bs * 2 + 1];
    return c;
}

struct Point {
    float x, y, z, u, v, depth;
};

__device__ __forceinline__ Point transform(const Calib &c, const f4 row) {
    Point q;
    q.x = ((row.x * c.m[0][0] + row.y * c.m[1][0]) + row.z * c.m[2][0]) + c.m[3][0];
    q.y = ((row.x * c.m[0][1] + row.y * c.m[1][1]) + row.z * c.m[2][1]) + c.m[3][1];
    q.z = ((row.x * c.m[0][2] + row.y * c.m[1][2]) + row.z * c.m[2][2]) + c.m[3][2];
    const float p0 = ((q.x * c.p[0][0] + q.y * c.p[0][1]) + q.z * c.p[0][2]) + c.p[0][3];
    const float p1 = ((q.x * c.p[1][0] + q.y * c.p[1][1]) + q.z * c.p[1][2]) + c.p[1][3];
    const float p2 = ((q.x * c.p[2][0] + q.y * c.p[2][1]) + q.z * c.p[2][2]) + c.p[2][3];
    q.u = p0 / q.z;          // the divisor is the rectified z, as calibration.py:68
    q.v = p1 / q.z;
    q.depth = p2 - c.p[2][3];
    return q;
}

__device__ __forceinline__ int clamp_raw(const int *__restrict__ num_raw, int bs, int p) {
    const int r = num_raw[bs];
    return r < 0 ? 0 : (r > p ? p : r);
}

__device__ __forceinline__ u64 set_word(int set, u64 valid, u64 near) {
    return set == kValid ? valid : (set == kNear ? near : (set == kFar ? (valid & ~near) : 0ull));
}

__device__ __forceinline__ int set_count(int set, int v, int f) {
    return set == kValid ? v : (set == kNear ? v - f : (set == kFar ? f : 0));
}

// ---- the variant with ground-truth database objects (epnet_scan_prepare_aug): the index space is the p raw rows, then e rows of
// pasted objects that are rectified already; a raw row inside one of the scene's removal boxes is not valid. AUG is a
// compile-time switch of the four kernels: with AUG == false they are the kernels of epnet_scan_prepare as they were, down to
// their arguments -- the AugArgs travel in a parameter pack that is empty then.
constexpr int kMaxRemove = 32;                     // EPNET_GT_AUG_MAX_ACCEPT

struct AugArgs {
    int p_raw, e, k_max, count_stride;             // num_remove[k * count_stride], num_extra[k * count_stride]
    const f4 *extra;                               // (b,e,4) [x, y, z, intensity], rectified
    const int *num_extra;
    const float *remove_boxes;                     // (b,k_max,7)
    const int *num_remove;
};

struct NoArgs {};

__device__ __forceinline__ NoArgs first_arg() { return NoArgs(); }
__device__ __forceinline__ const AugArgs &first_arg(const AugArgs &a) { return a; }

__device__ __forceinline__ int clamp_count(const int *__restrict__ counts, int at, int cap) {
    const int r = counts[at];
    return r < 0 ? 0 : (r > cap ? cap : r);
}

// the pixel of a rectified point: the second half of transform()
__device__ __forceinline__ Point project(const Calib &c, const f4 row) {
    Point q;
    q.x = row.x; q.y = row.y; q.z = row.z;
    const float p0 = ((q.x * c.p[0][0] + q.y * c.p[0][1]) + q.z * c.p[0][2]) + c.p[0][3];
    const float p1 = ((q.x * c.p[1][0] + q.y * c.p[1][1]) + q.z * c.p[1][2]) + c.p[1][3];
    const float p2 = ((q.x * c.p[2][0] + q.y * c.p[2][1]) + q.z * c.p[2][2]) + c.p[2][3];
    q.u = p0 / q.z;
    q.v = p1 / q.z;
    q.depth = p2 - c.p[2][3];
    return q;
}

// pt_in_box3d (roipool3d_kernel.cu:14-28) as roipool3d.hip evaluates it; s = [cx, cy, cz, hh, hw, hl, cosa, sina]
__device__ __forceinline__ void remove_box_setup(const float *__restrict__ bx, float *s) {
    const float h = bx[3];
    s[0] = bx[0]; s[1] = (float)((double)bx[1] - (double)h / 2.0); s[2] = bx[2];
    s[3] = h * 0.5f; s[4] = bx[4] * 0.5f; s[5] = bx[5] * 0.5f;
    cr_cossinf(bx[6], s[6], s[7]);
}

__device__ __forceinline__ bool in_remove_box(const float *s, float x, float y, float z) {
    const float max_dis = 10.0f;
    if ((fabsf(x - s[0]) > max_dis) || (fabsf(y - s[1]) > s[3]) || (fabsf(z - s[2]) > max_dis)) return false;
    const float nsina = -s[7];
    const float x_rot = (x - s[0]) * s[6] + (z - s[2]) * nsina;
    const float z_rot = (x - s[0]) * s[7] + (z - s[2]) * s[6];
    return (x_rot >= -s[5]) & (x_rot <= s[5]) & (z_rot >= -s[4]) & (z_rot <= s[4]);
}

// ---- 1. classify: grid (tiles, b)
template <bool AUG, typename... Aug>
__global__ __launch_bounds__(kThreads) void scan_classify_kernel(int p, int reduce_by_range, Scope scope, float near_depth,
                                                                 const f4 *__restrict__ pts, const int *__restrict__ num_raw,
                                                                 const float *__restrict__ V2C, const float *__restrict__ R0,
                                                                 const float *__restrict__ P2, const int *__restrict__ img_shape,
                                                                 u64 *__restrict__ ws_valid, u64 *__restrict__ ws_near,
                                                                 int *__restrict__ ws_tile_cnt, Aug... aug_pack) {
    const auto aug = first_arg(aug_pack...);
    constexpr int kC = AUG ? 3 : 2;                // counts per tile: valid, far and, AUG, removed
    __shared__ int s_cnt[kWaves][kC];
    __shared__ float s_box[AUG ? kMaxRemove : 1][8];
    int wg_x, bs;
    xcd_scene_map(wg_x, bs);
    const int tiles = (int)gridDim.x, t = threadIdx.x, wave = t >> 6;
    const Calib c = load_calib(V2C, R0, P2, img_shape, bs);
    int p_raw = p, n_extra = 0, n_remove = 0;      // AUG: p is the size of the index space, p_raw the raw rows of a scene
    const f4 *extra = nullptr;
    if constexpr (AUG) {
        p_raw = aug.p_raw;
        n_extra = aug.e > 0 ? clamp_count(aug.num_extra, bs * aug.count_stride, aug.e) : 0;
        n_remove = aug.k_max > 0 ? clamp_count(aug.num_remove, bs * aug.count_stride, aug.k_max) : 0;
        extra = aug.extra + (size_t)bs * (size_t)aug.e;
        if (t < n_remove) remove_box_setup(aug.remove_boxes + ((size_t)bs * aug.k_max + t) * 7, s_box[t]);
        __syncthreads();
    }
    const int raw = clamp_raw(num_raw, bs, p_raw);
    const f4 *rows = pts + (size_t)bs * (size_t)p_raw;
    const size_t word0 = ((size_t)bs * tiles + wg_x) * kWords;
    int cnt_v = 0, cnt_f = 0, cnt_r = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int i = wg_x * kTile + it * kThreads + t;
        const f4 row = rows[i < p_raw ? i : p_raw - 1];         // clamped: no load under a condition
        const Point q = transform(c, row);
        bool ok = i < raw && q.u >= 0.f && q.u < c.w && q.v >= 0.f && q.v < c.h && q.depth >= 0.f;
        if (reduce_by_range)
            ok = ok && (double)q.x >= scope.v[0] && (double)q.x <= scope.v[1] && (double)q.y >= scope.v[2] &&
                 (double)q.y <= scope.v[3] && (double)q.z >= scope.v[4] && (double)q.z <= scope.v[5];
        float z = q.z;
        if constexpr (AUG) {
            bool removed = false;
            if (ok)
                for (int k = 0; k < n_remove; ++k) removed = removed || in_remove_box(s_box[k], q.x, q.y, q.z);
            cnt_r += __popcll(__ballot(ok && removed));
            ok = ok && !removed;
            const int j = i - p_raw;                            // the extra row, when not negative
            if (aug.e > 0) {                                    // uniform
                const f4 xr = extra[j >= 0 && j < aug.e ? j : 0];
                if (j >= 0) { ok = j < n_extra; z = xr.z; }
            }
        }
        const u64 vb = __ballot(ok), nb = __ballot(ok && z < near_depth);
        if ((t & 63) == 0) {
            ws_valid[word0 + it * kWaves + wave] = vb;
            ws_near[word0 + it * kWaves + wave] = nb;
        }
        cnt_v += __popcll(vb);
        cnt_f += __popcll(vb & ~nb);
    }
    if ((t & 63) == 0) {
        s_cnt[wave][0] = cnt_v; s_cnt[wave][1] = cnt_f;
        if constexpr (AUG) s_cnt[wave][2] = cnt_r;
    }
    __syncthreads();
    if (t == 0) {
        int v = 0, f = 0, r = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            v += s_cnt[k][0]; f += s_cnt[k][1];
            if constexpr (AUG) r += s_cnt[k][2];
        }
        ws_tile_cnt[((size_t)bs * tiles + wg_x) * kC] = v;
        ws_tile_cnt[((size_t)bs * tiles + wg_x) * kC + 1] = f;
        if constexpr (AUG) ws_tile_cnt[((size_t)bs * tiles + wg_x) * kC + 2] = r;
    }
}

// ---- 2. plan: grid (b), one workgroup per scene
template <bool AUG, typename... Aug>
__global__ __launch_bounds__(kPlanThreads) void scan_plan_kernel(int p, int n, int tiles, const int *__restrict__ num_raw,
                                                                 const unsigned *__restrict__ keys, const u64 *__restrict__ ws_valid,
                                                                 const u64 *__restrict__ ws_near, const int *__restrict__ ws_tile_cnt,
                                                                 int *__restrict__ ws_plan, int *__restrict__ scene_info, Aug... aug_pack) {
    const auto aug = first_arg(aug_pack...);
    constexpr int kC = AUG ? 3 : 2;
    __shared__ int s_hist[256];
    __shared__ int s_sum[kC];
    __shared__ int s_pick[2];                      // the bin that holds the rem-th key, and the keys below that bin
    const int bs = blockIdx.x, t = threadIdx.x;
    if (t < kC) s_sum[t] = 0;
    __syncthreads();
    {
        int v = 0, f = 0, removed = 0;
        for (int k = t; k < tiles; k += kPlanThreads) {
            v += ws_tile_cnt[((size_t)bs * tiles + k) * kC];
            f += ws_tile_cnt[((size_t)bs * tiles + k) * kC + 1];
            if constexpr (AUG) removed += ws_tile_cnt[((size_t)bs * tiles + k) * kC + 2];
        }
        if (v) atomicAdd(&s_sum[0], v);
        if (f) atomicAdd(&s_sum[1], f);
        if constexpr (AUG)
            if (removed) atomicAdd(&s_sum[2], removed);
    }
    __syncthreads();
    const int V = s_sum[0], F = s_sum[1];
    int kase, q, r, cand, forced;
    if (V == 0) { kase = 4; q = 0; r = 0; cand = kNone; forced = kNone; }
    else if (V > n) {
        if (F <= n) { kase = 0; q = 1; r = n - F; cand = kNear; forced = kFar; }
        else { kase = 5; q = 0; r = n; cand = kFar; forced = kNone; }
    } else {
        kase = V == n ? 1 : (2 * V >= n ? 2 : 3);              // n <= 65536: no overflow
        q = kase == 3 ? n / V : 1;
        r = n - q * V;
        cand = kValid; forced = kValid;
    }
    // the r-th smallest (key, raw index) among the candidates: most significant byte first
    unsigned prefix = 0;
    int rem = r;
    if (r > 0) {
        const unsigned *kk = keys + (size_t)bs * (size_t)p;
        const size_t word0 = (size_t)bs * tiles * kWords;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (t < 256) s_hist[t] = 0;
            __syncthreads();
            // a wave's 64 points share one mask word; kPlanUnroll independent word and key loads in flight per thread (clamped
            // index, no load under a condition: one workgroup walks the scene, so the loop is bound by latency, not by bytes)
            for (int base = t; base < p; base += kPlanThreads * kPlanUnroll) {
                u64 word[kPlanUnroll];
                unsigned key[kPlanUnroll];
#pragma unroll
                for (int u = 0; u < kPlanUnroll; ++u) {
                    const int i = base + u * kPlanThreads, ii = i < p ? i : p - 1;
                    word[u] = set_word(cand, ws_valid[word0 + (ii >> 6)], ws_near[word0 + (ii >> 6)]);
                    key[u] = kk[ii];
                }
#pragma unroll
                for (int u = 0; u < kPlanUnroll; ++u) {
                    const int i = base + u * kPlanThreads;
                    const bool in = i < p && ((word[u] >> (i & 63)) & 1ull);
                    if (in && (pass == 0 || (key[u] >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&s_hist[(key[u] >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (t < 256) {
                int below = 0;
                for (int k = 0; k < t; ++k) below += s_hist[k];
                if (below < rem && rem <= below + s_hist[t]) { s_pick[0] = t; s_pick[1] = below; }
            }
            __syncthreads();
            prefix |= (unsigned)s_pick[0] << shift;
            rem -= s_pick[1];
            __syncthreads();
        }
    }
    if (t == 0) {
        int *pl = ws_plan + (size_t)bs * kPlanInts;
        pl[0] = kase; pl[1] = q; pl[2] = r; pl[3] = (int)prefix; pl[4] = r > 0 ? rem : 0; pl[5] = cand; pl[6] = forced;
        pl[7] = set_count(forced, V, F);
        if constexpr (AUG) {
            int *si = scene_info + (size_t)bs * 8;
            si[0] = clamp_raw(num_raw, bs, aug.p_raw); si[1] = V; si[2] = F; si[3] = kase; si[4] = r; si[5] = q;
            si[6] = s_sum[2];
            si[7] = aug.e > 0 ? clamp_count(aug.num_extra, bs * aug.count_stride, aug.e) : 0;
        } else {
            int *si = scene_info + (size_t)bs * 6;
            si[0] = clamp_raw(num_raw, bs, p); si[1] = V; si[2] = F; si[3] = kase; si[4] = r; si[5] = q;
        }
    }
}

// ---- 3. count: grid (tiles, b): the tile's candidates below the threshold key and at it
__global__ __launch_bounds__(kThreads) void scan_count_kernel(int p, const unsigned *__restrict__ keys, const u64 *__restrict__ ws_valid,
                                                              const u64 *__restrict__ ws_near, const int *__restrict__ ws_plan,
                                                              int *__restrict__ ws_tile_sel) {
    __shared__ int s_cnt[kWaves][2];
    int wg_x, bs;
    xcd_scene_map(wg_x, bs);
    const int tiles = (int)gridDim.x, t = threadIdx.x, wave = t >> 6;
    const int *pl = ws_plan + (size_t)bs * kPlanInts;
    const unsigned thr = (unsigned)pl[3];
    const int cand = pl[2] > 0 ? pl[5] : kNone;
    const unsigned *kk = keys + (size_t)bs * (size_t)p;
    const size_t word0 = ((size_t)bs * tiles + wg_x) * kWords;
    int less = 0, tie = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int i = wg_x * kTile + it * kThreads + t;
        const u64 word = set_word(cand, ws_valid[word0 + it * kWaves + wave], ws_near[word0 + it * kWaves + wave]);
        const bool in = (word >> (t & 63)) & 1ull;               // a set bit is a row below num_raw <= p
        const unsigned key = in ? kk[i] : 0u;
        less += __popcll(__ballot(in && key < thr));
        tie += __popcll(__ballot(in && key == thr));
    }
    if ((t & 63) == 0) { s_cnt[wave][0] = less; s_cnt[wave][1] = tie; }
    __syncthreads();
    if (t == 0) {
        int a = 0, e = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) { a += s_cnt[k][0]; e += s_cnt[k][1]; }
        ws_tile_sel[((size_t)bs * tiles + wg_x) * 2] = a;
        ws_tile_sel[((size_t)bs * tiles + wg_x) * 2 + 1] = e;
    }
}

struct Outputs {
    float *pts_rect, *pts_intensity, *pts_origin_xy, *pts_input;
    int *choice;
};

// writes list position `pos` of scene bs; a slot outside [0, n) (a slot_perm that is no permutation) writes nothing
__device__ __forceinline__ void put_row(const Outputs &o, const int *__restrict__ slot_perm, int bs, int n, int pos, const Point &q,
                                        float intensity, int raw_index) {
    if (pos >= n) return;
    const int slot = slot_perm ? slot_perm[(size_t)bs * n + pos] : pos;
    if ((unsigned)slot >= (unsigned)n) return;
    const size_t d = (size_t)bs * (size_t)n + (size_t)slot;
    o.pts_rect[d * 3] = q.x; o.pts_rect[d * 3 + 1] = q.y; o.pts_rect[d * 3 + 2] = q.z;
    o.pts_intensity[d] = intensity;
    o.pts_origin_xy[d * 2] = q.u; o.pts_origin_xy[d * 2 + 1] = q.v;
    if (o.pts_input) { o.pts_input[d * 4] = q.x; o.pts_input[d * 4 + 1] = q.y; o.pts_input[d * 4 + 2] = q.z; o.pts_input[d * 4 + 3] = intensity; }
    o.choice[d] = raw_index;
}

// ---- 4. emit: grid (tiles, b)
template <bool AUG, typename... Aug>
__global__ __launch_bounds__(kThreads) void scan_emit_kernel(int p, int n, const f4 *__restrict__ pts, const float *__restrict__ V2C,
                                                             const float *__restrict__ R0, const float *__restrict__ P2,
                                                             const int *__restrict__ img_shape, const unsigned *__restrict__ keys,
                                                             const int *__restrict__ slot_perm, const u64 *__restrict__ ws_valid,
                                                             const u64 *__restrict__ ws_near, const int *__restrict__ ws_tile_cnt,
                                                             const int *__restrict__ ws_plan, const int *__restrict__ ws_tile_sel,
                                                             Outputs o, Aug... aug_pack) {
    const auto aug = first_arg(aug_pack...);
    constexpr int kC = AUG ? 3 : 2;
    __shared__ int s_before[3];                    // forced, below the threshold, at the threshold: in the tiles before this one
    __shared__ u64 s_mask[3][kWords];
    __shared__ int s_pre[3][kWords];               // the same three counts in the words of this tile before word j
    int wg_x, bs;
    xcd_scene_map(wg_x, bs);
    const int tiles = (int)gridDim.x, t = threadIdx.x, wave = t >> 6;
    const int *pl = ws_plan + (size_t)bs * kPlanInts;
    const int kase = pl[0], q = pl[1], r = pl[2], admit = pl[4], forced = pl[6], forced_n = pl[7];
    const unsigned thr = (unsigned)pl[3];
    const int cand = r > 0 ? pl[5] : kNone;
    if (kase == 4) {                               // no valid point: zero rows, choice -1
        for (int j = wg_x * kThreads + t; j < n; j += tiles * kThreads) {
            const size_t d = (size_t)bs * (size_t)n + (size_t)j;
            o.pts_rect[d * 3] = 0.f; o.pts_rect[d * 3 + 1] = 0.f; o.pts_rect[d * 3 + 2] = 0.f;
            o.pts_intensity[d] = 0.f;
            o.pts_origin_xy[d * 2] = 0.f; o.pts_origin_xy[d * 2 + 1] = 0.f;
            if (o.pts_input) { o.pts_input[d * 4] = 0.f; o.pts_input[d * 4 + 1] = 0.f; o.pts_input[d * 4 + 2] = 0.f; o.pts_input[d * 4 + 3] = 0.f; }
            o.choice[d] = -1;
        }
        return;
    }
    if (t < 3) s_before[t] = 0;
    __syncthreads();
    {
        int a = 0, l = 0, e = 0;
        for (int k = t; k < wg_x; k += kThreads) {
            const size_t at = ((size_t)bs * tiles + k) * 2, at_cnt = ((size_t)bs * tiles + k) * kC;
            a += set_count(forced, ws_tile_cnt[at_cnt], ws_tile_cnt[at_cnt + 1]);
            l += ws_tile_sel[at];
            e += ws_tile_sel[at + 1];
        }
        if (a) atomicAdd(&s_before[0], a);
        if (l) atomicAdd(&s_before[1], l);
        if (e) atomicAdd(&s_before[2], e);
    }
    const unsigned *kk = keys + (size_t)bs * (size_t)p;
    const size_t word0 = ((size_t)bs * tiles + wg_x) * kWords;
    bool in_forced[kIters], is_less[kIters], is_tie[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int i = wg_x * kTile + it * kThreads + t, j = it * kWaves + wave;
        const u64 vw = ws_valid[word0 + j], nw = ws_near[word0 + j];
        const u64 fw = set_word(forced, vw, nw), cw = set_word(cand, vw, nw);
        const bool in = (cw >> (t & 63)) & 1ull;
        const unsigned key = in ? kk[i] : 0u;
        in_forced[it] = (fw >> (t & 63)) & 1ull;
        is_less[it] = in && key < thr;
        is_tie[it] = in && key == thr;
        const u64 lb = __ballot(is_less[it]), eb = __ballot(is_tie[it]);
        if ((t & 63) == 0) { s_mask[0][j] = fw; s_mask[1][j] = lb; s_mask[2][j] = eb; }
    }
    __syncthreads();
    if (t < 3 * kWords) {
        const int which = t / kWords, j = t - which * kWords;
        int sum = 0;
        for (int k = 0; k < j; ++k) sum += __popcll(s_mask[which][k]);
        s_pre[which][j] = sum;
    }
    __syncthreads();
    const Calib c = load_calib(V2C, R0, P2, img_shape, bs);
    int p_raw = p;
    if constexpr (AUG) p_raw = aug.p_raw;
    const f4 *rows = pts + (size_t)bs * (size_t)p_raw;
    // who is chosen, and the ballots of it, in a loop of their own: every ballot is taken with the whole wave active, before
    // the write loop below diverges
    bool chosen_it[kIters];
    u64 chosen_mask[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int j = it * kWaves + wave;
        const int tie_rank = s_before[2] + s_pre[2][j] + popc_below(s_mask[2][j]);
        chosen_it[it] = is_less[it] || (is_tie[it] && tie_rank < admit);
        chosen_mask[it] = __ballot(chosen_it[it]);
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int i = wg_x * kTile + it * kThreads + t, j = it * kWaves + wave;
        const int tie_before = s_before[2] + s_pre[2][j];
        const bool chosen = chosen_it[it];
        const u64 cb = chosen_mask[it];
        if (!(in_forced[it] || chosen)) continue;
        f4 row;
        Point pt;
        if (!AUG || i < p_raw) {
            row = rows[i];                                        // a set bit is a row below num_raw <= p
            pt = transform(c, row);
        } else if constexpr (AUG) {
            row = aug.extra[(size_t)bs * (size_t)aug.e + (size_t)(i - p_raw)];   // a set bit is a row below num_extra <= e
            pt = project(c, row);
        }
        const float intensity = row.w - 0.5f;
        if (in_forced[it]) {
            const int rank = s_before[0] + s_pre[0][j] + popc_below(s_mask[0][j]);
            for (int copy = 0; copy < q; ++copy) put_row(o, slot_perm, bs, n, copy * forced_n + rank, pt, intensity, i);
        }
        if (chosen) {
            const int taken_ties = tie_before < admit ? tie_before : admit;
            const int rank = (s_before[1] + s_pre[1][j] + taken_ties) + popc_below(cb);
            put_row(o, slot_perm, bs, n, q * forced_n + rank, pt, intensity, i);
        }
    }
}

// ---- image normalisation: grid (groups of 256 * 4 pixels of the output plane, b)
struct Norm {
    double mean[3], std[3];
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void image_normalise_kernel(int h_in, int w_in, int h_out, int w_out, const uint8_t *__restrict__ img,
                                                                   const int *__restrict__ img_shape, Norm nm, float *__restrict__ out) {
    __shared__ float s_tab[3][256];                // the 256 values a channel can take, rounded once from double
    const int t = threadIdx.x, bs = blockIdx.y;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_tab[c][t] = (float)((((double)t / 255.0) - nm.mean[c]) / nm.std[c]);
    __syncthreads();
    int hk = h_in, wk = w_in;
    if (img_shape) { hk = img_shape[(size_t)bs * 2]; wk = img_shape[(size_t)bs * 2 + 1]; }
    hk = hk < 0 ? 0 : (hk > h_in ? h_in : hk);     // never read past the given image
    wk = wk < 0 ? 0 : (wk > w_in ? w_in : wk);
    const int groups_x = (w_out + 3) / 4;
    const long long g = (long long)blockIdx.x * kThreads + t;
    if (g >= (long long)groups_x * h_out) return;
    const int y = (int)(g / groups_x), x0 = (int)(g - (long long)y * groups_x) * 4;
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        const bool in = y < hk && x < wk;
        const uint8_t *px = img + (((size_t)bs * h_in + (in ? y : 0)) * w_in + (in ? x : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = in ? s_tab[c][px[c]] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *dst = out + (((size_t)bs * 3 + c) * h_out + y) * (size_t)w_out + x0;
        if (VEC) {
            store_stream(dst, v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < w_out) dst[k] = v[c][k];
        }
    }
}

}  // namespace scan
}  // namespace epnet

using namespace epnet;

static bool scan_limits(int b, int p, int n) { return n >= 1 && n <= 65536 && p >= 1 && p <= 1048576 && b <= 65535; }

extern "C" size_t epnet_scan_prepare_workspace_bytes(int b, int p, int n) {
    if (b <= 0 || !scan_limits(b, p, n)) return 0;
    return scan::layout(b, div_up(p, scan::kTile)).total;
}

extern "C" int epnet_scan_prepare(int b, int p, int n, int reduce_by_range, const double *scope, float near_depth,
                                  const float *pts_lidar, const int *num_raw, const float *V2C, const float *R0, const float *P2,
                                  const int *img_shape, const int *keys, const int *slot_perm, void *workspace, size_t workspace_bytes,
                                  float *pts_rect, float *pts_intensity, float *pts_origin_xy, float *pts_input, int *choice,
                                  int *scene_info, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0);
    if (b == 0) return EPNET_OK;
    if (!scan_limits(b, p, n)) return EPNET_ELIMIT;
    EPNET_REQUIRE(pts_lidar && num_raw && V2C && R0 && P2 && img_shape && keys && workspace);
    EPNET_REQUIRE(pts_rect && pts_intensity && pts_origin_xy && choice && scene_info);
    EPNET_REQUIRE(scope || !reduce_by_range);
    EPNET_REQUIRE(((uintptr_t)pts_lidar & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    const int tiles = div_up(p, scan::kTile);
    const scan::Layout l = scan::layout(b, tiles);
    if (workspace_bytes < l.total) return EPNET_ENOMEM;
    scan::Scope sc;
    for (int k = 0; k < 6; ++k) sc.v[k] = scope ? scope[k] : 0.0;
    char *ws = (char *)workspace;
    scan::u64 *ws_valid = (scan::u64 *)(ws + l.valid), *ws_near = (scan::u64 *)(ws + l.near);
    int *ws_tile_cnt = (int *)(ws + l.tile_cnt), *ws_plan = (int *)(ws + l.plan), *ws_tile_sel = (int *)(ws + l.tile_sel);
    const scan::f4 *rows = (const scan::f4 *)pts_lidar;
    const unsigned *ukeys = (const unsigned *)keys;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)b), block(scan::kThreads);
    hipLaunchKernelGGL(scan::scan_classify_kernel<false>, grid, block, 0, st, p, reduce_by_range, sc, near_depth, rows, num_raw, V2C, R0, P2,
                       img_shape, ws_valid, ws_near, ws_tile_cnt);
    hipLaunchKernelGGL(scan::scan_plan_kernel<false>, dim3((unsigned)b), dim3(scan::kPlanThreads), 0, st, p, n, tiles, num_raw, ukeys,
                       ws_valid, ws_near, ws_tile_cnt, ws_plan, scene_info);
    hipLaunchKernelGGL(scan::scan_count_kernel, grid, block, 0, st, p, ukeys, ws_valid, ws_near, ws_plan, ws_tile_sel);
    const scan::Outputs o = {pts_rect, pts_intensity, pts_origin_xy, pts_input, choice};
    hipLaunchKernelGGL(scan::scan_emit_kernel<false>, grid, block, 0, st, p, n, rows, V2C, R0, P2, img_shape, ukeys, slot_perm, ws_valid,
                       ws_near, ws_tile_cnt, ws_plan, ws_tile_sel, o);
    return check_launch("scan_prepare");
}

static bool scan_aug_limits(int b, int p, int e, int n, int k_max) {
    return scan_limits(b, p, n) && e >= 0 && e <= 1048576 && p + e <= 1048576 && k_max >= 0 && k_max <= scan::kMaxRemove;
}

extern "C" size_t epnet_scan_prepare_aug_workspace_bytes(int b, int p, int e, int n) {
    if (b <= 0 || !scan_aug_limits(b, p, e, n, 0)) return 0;
    return scan::layout(b, div_up(p + e, scan::kTile), 3).total;
}

extern "C" int epnet_scan_prepare_aug(int b, int p, int e, int n, int k_max, int reduce_by_range, const double *scope, float near_depth,
                                      const float *pts_lidar, const int *num_raw, const float *V2C, const float *R0, const float *P2,
                                      const int *img_shape, const float *extra_pts, const int *num_extra, const float *remove_boxes,
                                      const int *num_remove, int count_stride, const int *keys, const int *slot_perm, void *workspace,
                                      size_t workspace_bytes, float *pts_rect, float *pts_intensity, float *pts_origin_xy,
                                      float *pts_input, int *choice, int *scene_info, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0);
    if (b == 0) return EPNET_OK;
    if (!scan_aug_limits(b, p, e, n, k_max)) return EPNET_ELIMIT;
    EPNET_REQUIRE(pts_lidar && num_raw && V2C && R0 && P2 && img_shape && keys && workspace);
    EPNET_REQUIRE(pts_rect && pts_intensity && pts_origin_xy && choice && scene_info);
    EPNET_REQUIRE(scope || !reduce_by_range);
    EPNET_REQUIRE(count_stride >= 1 && (e == 0 || (extra_pts && num_extra)) && (k_max == 0 || (remove_boxes && num_remove)));
    EPNET_REQUIRE(((uintptr_t)pts_lidar & 15) == 0 && ((uintptr_t)extra_pts & 15) == 0 && ((uintptr_t)workspace & 7) == 0);
    const int total = p + e, tiles = div_up(total, scan::kTile);
    const scan::Layout l = scan::layout(b, tiles, 3);
    if (workspace_bytes < l.total) return EPNET_ENOMEM;
    scan::Scope sc;
    for (int k = 0; k < 6; ++k) sc.v[k] = scope ? scope[k] : 0.0;
    char *ws = (char *)workspace;
    scan::u64 *ws_valid = (scan::u64 *)(ws + l.valid), *ws_near = (scan::u64 *)(ws + l.near);
    int *ws_tile_cnt = (int *)(ws + l.tile_cnt), *ws_plan = (int *)(ws + l.plan), *ws_tile_sel = (int *)(ws + l.tile_sel);
    const scan::f4 *rows = (const scan::f4 *)pts_lidar;
    const unsigned *ukeys = (const unsigned *)keys;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)b), block(scan::kThreads);
    scan::AugArgs aug;
    aug.p_raw = p; aug.e = e; aug.k_max = k_max; aug.count_stride = count_stride;
    aug.extra = (const scan::f4 *)extra_pts; aug.num_extra = num_extra; aug.remove_boxes = remove_boxes; aug.num_remove = num_remove;
    // the kernels' `p` is the size of the index space: raw rows, then extra rows
    hipLaunchKernelGGL(scan::scan_classify_kernel<true>, grid, block, 0, st, total, reduce_by_range, sc, near_depth, rows, num_raw, V2C, R0,
                       P2, img_shape, ws_valid, ws_near, ws_tile_cnt, aug);
    hipLaunchKernelGGL(scan::scan_plan_kernel<true>, dim3((unsigned)b), dim3(scan::kPlanThreads), 0, st, total, n, tiles, num_raw, ukeys,
                       ws_valid, ws_near, ws_tile_cnt, ws_plan, scene_info, aug);
    hipLaunchKernelGGL(scan::scan_count_kernel, grid, block, 0, st, total, ukeys, ws_valid, ws_near, ws_plan, ws_tile_sel);
    const scan::Outputs o = {pts_rect, pts_intensity, pts_origin_xy, pts_input, choice};
    hipLaunchKernelGGL(scan::scan_emit_kernel<true>, grid, block, 0, st, total, n, rows, V2C, R0, P2, img_shape, ukeys, slot_perm, ws_valid,
                       ws_near, ws_tile_cnt, ws_plan, ws_tile_sel, o, aug);
    return check_launch("scan_prepare_aug");
}

extern "C" int epnet_image_normalise(int b, int h_in, int w_in, int h_out, int w_out, const uint8_t *img, const int *img_shape,
                                     const double *mean, const double *std, float *out, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && h_in >= 1 && w_in >= 1 && h_out >= 1 && w_out >= 1);
    if (b == 0) return EPNET_OK;
    const long long groups = (long long)div_up(w_out, 4) * h_out;
    const long long wgs = div_up64(groups, scan::kThreads);
    if (b > 65535 || wgs > 0x7fffffffll || (long long)h_in * w_in > 0x7fffffffll / 3) return EPNET_ELIMIT;
    EPNET_REQUIRE(img && mean && std && out);
    scan::Norm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.std[c] = std[c]; }
    const bool vec = w_out % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)wgs, (unsigned)b), block(scan::kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(scan::image_normalise_kernel<true>, grid, block, 0, st, h_in, w_in, h_out, w_out, img, img_shape, nm, out);
    else
        hipLaunchKernelGGL(scan::image_normalise_kernel<false>, grid, block, 0, st, h_in, w_in, h_out, w_out, img, img_shape, nm, out);
    return check_launch("image_normalise");
}
