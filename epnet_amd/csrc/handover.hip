// handover.hip -- from the RPN heads to the proposal kernels in one call (include/epnet_ops.h: epnet_decode_bbox_target,
// epnet_score_order, epnet_rpn_handover) for gfx950.
//
// The reference decodes the boxes with about thirty small tensor kernels (lib/utils/bbox_transform.py:25-262), moves y to the
// bottom centre, sorts the scores and forms the segmentation mask and the point depths with stock ops
// (lib/rpn/proposal_layer.py:23-35, lib/net/point_rcnn.py:44-52). Here:
//
//   decode   one wave per 64 consecutive rows. The wave stages its 64 regression rows with 16-byte coalesced loads into LDS
//            (odd row stride: a lane reading its own row is conflict-free), every lane decodes its own row there -- soft-bin
//            mean or first arg-max bin per axis, y by offset or bin, the heading by arg-max bin or the two-sided weighted
//            mean, sizes from the anchor, the ROI rotation for 7-wide anchors -- and the 64 boxes leave through LDS as
//            coalesced rows. In the hand-over the same launch writes seg_mask = sigmoid(score) > thresh and pts_depth = |xyz|
//            from the score and the anchor row the lane holds anyway.
//   order    one workgroup per scene: the unique keys (ordered_key(score) << 32) | ~index of a scene in LDS, sorted
//            descending by a bitonic network: up to four strides >= 128 per pass over LDS (a thread holds the 2^m keys
//            they connect), strides 64 .. 1 in registers (two keys per lane, exchanged over the vector ALU). A unique key makes the sort stable by construction: equal scores
//            come out in ascending index, a NaN before every number, -0.0 == +0.0.
//   epnet_rpn_handover = decode (1 launch) + order (1 launch) + epnet_rpn_proposals unchanged (bin, [box rotation,] NMS mask,
//            NMS sweep, emit): 7 launches with the rotated NMS, 6 with the normal one, whatever the data.
// No float atomics, no allocation, no copy and no synchronisation: the bits depend on the inputs alone, and the calls record
// into a graph. Arithmetic: fp32 in source order without contraction; expf / sinf / cosf / fmodf are the accurate ones.
#include "common.h"
#include "dpp.h"

namespace epnet {
namespace handover {

constexpr int kMaxChannels = 255;      // 64 rows of stride (c | 1) floats stay within 64 KiB of LDS
constexpr int kOrderThreads = 1024;
constexpr int kOrderMaxN = 16384;      // keys of a scene: 128 KiB of the CU's 160 KiB
constexpr int kOrderMaxB = 65535;

struct Params {
    long long rows;
    int c, acols, nb, nby, nh, xz_fine, y_by_bin, ry_fine, avg, ry_bin, y_bottom, vec;
    float scope, bs, bs_half, y_scope, y_bs, y_bs_half, per_bin, per_bin_half, a_h, a_w, a_l, thresh;
};

// torch.remainder: the sign of the divisor
__device__ __forceinline__ float py_mod(float a, float b) {
    float r = fmodf(a, b);
    if (r != 0.f && ((r < 0.f) != (b < 0.f))) r = r + b;
    return r;
}

// torch.argmax over n logits of a row in LDS: the FIRST maximal one; a NaN counts as the maximum
__device__ __forceinline__ int first_argmax(const float *x, int n) {
    int best = 0;
    float top = x[0];
    for (int k = 1; k < n; ++k) {
        const float v = x[k];
        if (v > top || (v != v && top == top)) { top = v; best = k; }
    }
    return best;
}

// arg-max bin centre (+ the residual predicted for that bin), bbox_transform.py:48-72
__device__ __forceinline__ float hard_bin(const float *bins, const float *res, int n, float bs, float bs_half, float scope,
                                          bool with_residual) {
    const int which = first_argmax(bins, n);
    float pos = (float)which * bs + bs_half - scope;
    if (with_residual) pos = pos + res[which] * bs;
    return pos;
}

// soft-max weighted mean of (bin centre + that bin's residual), bbox_transform.py:73-106
__device__ __forceinline__ float soft_bin(const float *bins, const float *res, int n, float bs, float bs_half, float scope) {
    float m = bins[0];
    for (int k = 1; k < n; ++k) m = fmaxf(m, bins[k]);
    float se = 0.f;
    for (int k = 0; k < n; ++k) se = se + expf(bins[k] - m);
    float acc = 0.f;
    for (int k = 0; k < n; ++k) {
        const float centre = (float)k * bs + bs_half - scope;
        acc = acc + (centre + res[k] * bs) * (expf(bins[k] - m) / se);
    }
    return acc;
}

// grid ceil(rows / 64) workgroups of ONE wave; dynamic LDS: 64 rows of stride (c | 1) floats. scores / seg_mask / pts_depth
// are NULL outside the hand-over (pts_depth needs 3-wide anchors: the points themselves).
__global__ __launch_bounds__(64) void decode_kernel(Params p, const float *__restrict__ anchors, const float *__restrict__ pred_reg,
                                                    const float *__restrict__ scores, float *__restrict__ boxes,
                                                    float *__restrict__ seg_mask, float *__restrict__ pts_depth) {
    extern __shared__ __attribute__((aligned(16))) float s_tile[];
    const int lane = lane_id();
    const long long row0 = (long long)blockIdx.x * 64, row = row0 + lane;
    const bool in = row < p.rows;
    const int tile_rows = (int)(p.rows - row0 < 64 ? p.rows - row0 : 64);
    const int c = p.c, stride = c | 1;
    const int n = tile_rows * c;                    // floats of this wave's tile

    // ---- stage the tile: element e of the tile belongs to row e / c, column e % c, kept incrementally
    const float *src = pred_reg + (size_t)row0 * (size_t)c;
    if (p.vec) {
        int e = lane * 4, r = e / c, col = e - r * c;
        const int dr = 256 / c, dc = 256 - dr * c;
        for (; e + 3 < n; e += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(src + e);
            const float vv[4] = {v.x, v.y, v.z, v.w};
            int rr = r, cc = col;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s_tile[rr * stride + cc] = vv[k];
                if (++cc == c) { cc = 0; ++rr; }
            }
            r += dr; col += dc;
            if (col >= c) { col -= c; ++r; }
        }
        for (int i = (n & ~3) + lane; i < n; i += 64) { const int rr = i / c; s_tile[rr * stride + (i - rr * c)] = src[i]; }
    } else {
        for (int i = lane; i < n; i += 64) { const int rr = i / c; s_tile[rr * stride + (i - rr * c)] = src[i]; }
    }

    // ---- the lane's anchor row and, in the hand-over, its mask and depth
    float ax = 0.f, ay = 0.f, az = 0.f, a_ry = 0.f;
    if (in) {
        const float *a = anchors + (size_t)row * p.acols;
        ax = a[0]; ay = a[1]; az = a[2];
        if (p.acols == 7) a_ry = a[6];
        if (seg_mask) {
            const float prob = 1.f / (1.f + expf(-scores[row]));
            seg_mask[row] = prob > p.thresh ? 1.f : 0.f;   // a NaN score compares false
        }
        if (pts_depth) pts_depth[row] = sqrtf(ax * ax + ay * ay + az * az);
    }
    __syncthreads();

    float box[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
        const float *q = s_tile + lane * stride;      // this lane's row
        const int nb = p.nb, nh = p.nh;
        // ---- x, z
        float pos_x, pos_z;
        if (p.avg) {
            pos_x = soft_bin(q, q + 2 * nb, nb, p.bs, p.bs_half, p.scope);
            pos_z = soft_bin(q + nb, q + 3 * nb, nb, p.bs, p.bs_half, p.scope);
        } else {
            pos_x = hard_bin(q, q + 2 * nb, nb, p.bs, p.bs_half, p.scope, p.xz_fine != 0);
            pos_z = hard_bin(q + nb, q + 3 * nb, nb, p.bs, p.bs_half, p.scope, p.xz_fine != 0);
        }
        int cursor = p.xz_fine ? 4 * nb : 2 * nb;
        // ---- y (:108-124)
        float pos_y;
        if (p.y_by_bin) {
            pos_y = hard_bin(q + cursor, q + cursor + p.nby, p.nby, p.y_bs, p.y_bs_half, p.y_scope, true) + ay;
            cursor += 2 * p.nby;
        } else {
            pos_y = ay + q[cursor];
            cursor += 1;
        }
        // ---- heading (:126-238)
        const float *logit = q + cursor, *res = q + cursor + nh;
        cursor += 2 * nh;
        constexpr float kTwoPi = (float)(2.0 * M_PI), kPi = (float)M_PI, kQuarterPi = (float)(M_PI * 0.25);
        float ry;
        if (p.ry_bin) {
            // every bin proposes a heading; the bins fall on two sides (fine: either side of the ROI's own heading, coarse: the
            // first / second half turn); the answer is the probability-weighted mean over the likelier side
            float m = logit[0];
            for (int k = 1; k < nh; ++k) m = fmaxf(m, logit[k]);
            float se = 0.f;
            for (int k = 0; k < nh; ++k) se = se + expf(logit[k] - m);
            float mass_r = 0.f, mass_l = 0.f;
            for (int k = 0; k < nh; ++k) {
                const float each = p.ry_fine ? ((float)k * p.per_bin + p.per_bin_half) + res[k] * p.per_bin_half - kQuarterPi
                                             : py_mod((float)k * p.per_bin + res[k] * p.per_bin_half, kTwoPi);
                const bool right = p.ry_fine ? each >= 0.f : each <= kPi;
                const float prob = expf(logit[k] - m) / se;
                mass_r = mass_r + (right ? prob : 0.f);
                mass_l = mass_l + (right ? 0.f : prob);
            }
            mass_r = mass_r + 1e-7f;
            mass_l = mass_l + 1e-7f;
            float ry_r = 0.f, ry_l = 0.f;
            for (int k = 0; k < nh; ++k) {
                const float each = p.ry_fine ? ((float)k * p.per_bin + p.per_bin_half) + res[k] * p.per_bin_half - kQuarterPi
                                             : py_mod((float)k * p.per_bin + res[k] * p.per_bin_half, kTwoPi);
                const bool right = p.ry_fine ? each >= 0.f : each <= kPi;
                const float prob = expf(logit[k] - m) / se;
                ry_r = ry_r + (right ? each : 0.f) * ((right ? prob : 0.f) / mass_r);
                ry_l = ry_l + (right ? 0.f : each) * ((right ? 0.f : prob) / mass_l);
            }
            const float use_r = mass_r >= mass_l ? 1.f : 0.f;
            ry = ry_r * use_r + ry_l * (1.f - use_r);
            if (!p.ry_fine && ry > kPi) ry = ry - kTwoPi;
        } else {
            const int head = first_argmax(logit, nh);
            if (p.ry_fine) {       // a quarter turn split into bins around the ROI's own heading
                ry = ((float)head * p.per_bin + p.per_bin_half) + res[head] * p.per_bin_half - kQuarterPi;
            } else {               // the full turn, wrapped into (-pi, pi]
                ry = py_mod((float)head * p.per_bin + res[head] * p.per_bin_half, kTwoPi);
                if (ry > kPi) ry = ry - kTwoPi;
            }
        }
        // ---- size (:243-248) and back to scene coordinates (:250-262)
        const float h = q[cursor] * p.a_h + p.a_h, w = q[cursor + 1] * p.a_w + p.a_w, l = q[cursor + 2] * p.a_l + p.a_l;
        if (p.acols == 7) {
            const float cosa = cosf(-a_ry), sina = sinf(-a_ry);
            const float x = pos_x, z = pos_z;
            pos_x = x * cosa + z * (-sina);
            pos_z = x * sina + z * cosa;
            ry = ry + a_ry;
        }
        pos_x = pos_x + ax;
        pos_z = pos_z + az;
        if (p.y_bottom) pos_y = pos_y + h / 2.f;          // proposal_layer.py:31
        box[0] = pos_x; box[1] = pos_y; box[2] = pos_z; box[3] = h; box[4] = w; box[5] = l; box[6] = ry;
    }
    // ---- the 64 boxes leave through LDS as coalesced rows (stride >= 9 > 7: the tile holds them)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k) s_tile[lane * 7 + k] = box[k];
    __syncthreads();
    float *out = boxes + (size_t)row0 * 7;
    for (int i = lane; i < tile_rows * 7; i += 64) out[i] = s_tile[i];
}

// ---- per-scene stable descending order ---------------------------------------------------------------------------------------
// np = the power of two >= max(n, 128); the keys beyond n are 0, below every real key (ordered_key never returns 0), so they
// end up behind the n real ones. A bitonic network over np keys in LDS; no stride goes through LDS on its own:
//   strides >= 128: up to four consecutive strides per pass. A thread holds the 2^m keys whose indices differ in exactly those
//     stride bits (neighbouring lanes hold neighbouring keys: conflict-free) and runs the m stages in registers;
//   strides 64 .. 1: a wave holds 128 consecutive keys, two per lane; stride 64 is the lane's own pair, the others exchange
//     over the vector ALU (DPP quad / row moves, the gfx950 row and half swaps), not through the LDS pipe.
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
    const unsigned lo = dpp_u32<CTRL>((unsigned)v), hi = dpp_u32<CTRL>((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// which of the two candidates holds the value of lane ^ 4 / ^ 16 / ^ 32: found once per wave by moving the lane ids themselves
struct LanePick {
    bool ror4, first16, first32;
};

__device__ __forceinline__ LanePick lane_pick(int lane) {
    LanePick p;
    p.ror4 = dpp_i32<0x124>(lane) == (lane ^ 4);
    const auto a = __builtin_amdgcn_permlane16_swap((unsigned)lane, (unsigned)lane, false, false);
    p.first16 = (int)a[0] == (lane ^ 16);
    const auto b = __builtin_amdgcn_permlane32_swap((unsigned)lane, (unsigned)lane, false, false);
    p.first32 = (int)b[0] == (lane ^ 32);
    return p;
}

// the key held by lane ^ J
template <int J>
__device__ __forceinline__ unsigned long long partner_key(unsigned long long v, const LanePick &pick) {
    if (J == 1) return dpp_u64<0xB1>(v);          // quad_perm [1,0,3,2]
    if (J == 2) return dpp_u64<0x4E>(v);          // quad_perm [2,3,0,1]
    if (J == 8) return dpp_u64<0x128>(v);         // row_ror:8
    if (J == 4) {                                 // row_ror:4 for one half of the lanes, row_ror:12 for the other
        const unsigned long long x = dpp_u64<0x124>(v), y = dpp_u64<0x12C>(v);
        return pick.ror4 ? x : y;
    }
    const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    if (J == 16) {
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        return pick.first16 ? (((unsigned long long)h[0] << 32) | l[0]) : (((unsigned long long)h[1] << 32) | l[1]);
    }
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return pick.first32 ? (((unsigned long long)h[0] << 32) | l[0]) : (((unsigned long long)h[1] << 32) | l[1]);
}

// stride J <= 32 of phase k on the two keys of a lane (indices ia and ib = ia + 64); skipped when the phase starts below it
template <int J>
__device__ __forceinline__ void lane_step(unsigned long long &a, unsigned long long &b, int ia, int ib, int k, int lane,
                                          const LanePick &pick) {
    if (J >= k) return;                           // wave-uniform
    const unsigned long long pa = partner_key<J>(a, pick), pb = partner_key<J>(b, pick);
    const bool lower = (lane & J) == 0;
    // descending block: the lower index keeps the larger key
    const bool max_a = lower == ((ia & k) == 0), max_b = lower == ((ib & k) == 0);
    a = max_a ? (a > pa ? a : pa) : (a < pa ? a : pa);
    b = max_b ? (b > pb ? b : pb) : (b < pb ? b : pb);
}

// the M strides 2^(s+M-1) .. 2^s of phase k in one pass over LDS
template <int M>
__device__ __forceinline__ void lds_pass(unsigned long long *keys, int np, int k, int s) {
    constexpr int R = 1 << M;
    for (int t = threadIdx.x; t < (np >> M); t += kOrderThreads) {
        const int low = t & ((1 << s) - 1), high = t >> s;
        const int i0 = low + (high << (s + M));
        unsigned long long v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = keys[i0 + (r << s)];
        const bool desc = (i0 & k) == 0;          // bit k lies above every stride of its phase: the same for all R keys
#pragma unroll
        for (int q = M - 1; q >= 0; --q) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r & (1 << q)) continue;
                const unsigned long long x = v[r], y = v[r | (1 << q)];
                const bool sw = (x < y) == desc;
                v[r] = sw ? y : x;
                v[r | (1 << q)] = sw ? x : y;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) keys[i0 + (r << s)] = v[r];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kOrderThreads) void score_order_kernel(int n, int np, const float *__restrict__ scores,
                                                                    long long *__restrict__ order) {
    __shared__ unsigned long long keys[kOrderMaxN];
    const int scene = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6;
    const LanePick pick = lane_pick(lane);
    scores += (size_t)scene * n;
    order += (size_t)scene * n;
    for (int i = threadIdx.x; i < np; i += kOrderThreads)
        keys[i] = i < n ? (((unsigned long long)ordered_key(scores[i]) << 32) | (unsigned)(~(unsigned)i)) : 0ull;
    __syncthreads();
    int klog = 1;
    for (int k = 2; k <= np; k <<= 1, ++klog) {
        // strides k / 2 .. 128, at most four per pass
        for (int e = klog - 1; e >= 7;) {
            const int m = e - 6 < 4 ? e - 6 : 4, s = e - m + 1;
            if (m == 4) lds_pass<4>(keys, np, k, s);
            else if (m == 3) lds_pass<3>(keys, np, k, s);
            else if (m == 2) lds_pass<2>(keys, np, k, s);
            else lds_pass<1>(keys, np, k, s);
            e -= m;
        }
        // strides 64 .. 1 of this phase: a wave takes 128 consecutive keys, two per lane
        for (int base = wave * 128; base < np; base += (kOrderThreads / 64) * 128) {
            const int ia = base + lane, ib = ia + 64;
            unsigned long long a = keys[ia], b = keys[ib];
            if (k > 64) {
                const bool desc = (ia & k) == 0;        // k >= 128: the same for the lane's two keys
                if ((a < b) == desc) { const unsigned long long t = a; a = b; b = t; }
            }
            lane_step<32>(a, b, ia, ib, k, lane, pick);
            lane_step<16>(a, b, ia, ib, k, lane, pick);
            lane_step<8>(a, b, ia, ib, k, lane, pick);
            lane_step<4>(a, b, ia, ib, k, lane, pick);
            lane_step<2>(a, b, ia, ib, k, lane, pick);
            lane_step<1>(a, b, ia, ib, k, lane, pick);
            keys[ia] = a;
            keys[ib] = b;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += kOrderThreads) order[i] = (long long)(unsigned)(~(unsigned)keys[i]);
}

inline int validate(int anchor_cols, int channels, int bins_xz, int bins_y, int num_head_bin, int xz_fine, int y_by_bin,
                    int avg_by_bin) {
    EPNET_REQUIRE(anchor_cols == 3 || anchor_cols == 7);
    EPNET_REQUIRE(bins_xz >= 1 && num_head_bin >= 1 && channels >= 1 && (!y_by_bin || bins_y >= 1));
    EPNET_REQUIRE(!(avg_by_bin && !xz_fine));                            // the reference asserts (:54)
    const long long want = (xz_fine ? 4ll : 2ll) * bins_xz + (y_by_bin ? 2ll * bins_y : 1ll) + 2ll * num_head_bin + 3;
    EPNET_REQUIRE((long long)channels == want);
    return EPNET_OK;
}

inline int launch_decode(long long rows, int anchor_cols, const float *anchors, const float *pred_reg, int channels, int bins_xz,
                         int bins_y, double loc_scope, double loc_bin_size, double loc_y_scope, double loc_y_bin_size,
                         int num_head_bin, const float *anchor_size, int xz_fine, int y_by_bin, int ry_fine, int avg_by_bin,
                         int ry_with_bin, int y_to_bottom, const float *scores, float score_thresh, float *boxes, float *seg_mask,
                         float *pts_depth, hipStream_t s) {
    Params p;
    p.rows = rows; p.c = channels; p.acols = anchor_cols; p.nb = bins_xz; p.nby = bins_y; p.nh = num_head_bin;
    p.xz_fine = xz_fine ? 1 : 0; p.y_by_bin = y_by_bin ? 1 : 0; p.ry_fine = ry_fine ? 1 : 0; p.avg = avg_by_bin ? 1 : 0;
    p.ry_bin = ry_with_bin ? 1 : 0; p.y_bottom = y_to_bottom ? 1 : 0;
    p.vec = ((uintptr_t)pred_reg & 15) == 0;
    // the constants as torch forms them: Python doubles, rounded to fp32 where they meet a tensor
    const double per_bin = ry_fine ? (M_PI / 2) / num_head_bin : (2 * M_PI) / num_head_bin;
    p.scope = (float)loc_scope; p.bs = (float)loc_bin_size; p.bs_half = (float)(loc_bin_size / 2);
    p.y_scope = (float)loc_y_scope; p.y_bs = (float)loc_y_bin_size; p.y_bs_half = (float)(loc_y_bin_size / 2);
    p.per_bin = (float)per_bin; p.per_bin_half = (float)(per_bin / 2);
    p.a_h = anchor_size[0]; p.a_w = anchor_size[1]; p.a_l = anchor_size[2];   // host memory, by value from here on
    p.thresh = score_thresh;
    const size_t lds = (size_t)64 * (channels | 1) * sizeof(float);
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)div_up64(rows, 64)), dim3(64), lds, s, p, anchors, pred_reg, scores, boxes,
                       seg_mask, pts_depth);
    return check_launch("decode_bbox_target");
}

inline int launch_order(int b, int n, const float *scores, int64_t *order, hipStream_t s) {
    int np = 128;
    while (np < n) np <<= 1;
    hipLaunchKernelGGL(score_order_kernel, dim3(b), dim3(kOrderThreads), 0, s, n, np, scores, (long long *)order);
    return check_launch("score_order");
}

}  // namespace handover
}  // namespace epnet

using namespace epnet;

extern "C" int epnet_decode_bbox_target(long long rows, int anchor_cols, const float *anchors, const float *pred_reg, int channels,
                                        int bins_xz, int bins_y, double loc_scope, double loc_bin_size, double loc_y_scope,
                                        double loc_y_bin_size, int num_head_bin, const float *anchor_size, int xz_fine,
                                        int y_by_bin, int ry_fine, int avg_by_bin, int ry_with_bin, int y_to_bottom, float *boxes,
                                        epnet_stream_t stream) {
    EPNET_REQUIRE(rows >= 0);
    const int rc = handover::validate(anchor_cols, channels, bins_xz, bins_y, num_head_bin, xz_fine, y_by_bin, avg_by_bin);
    if (rc) return rc;
    if (rows == 0) return EPNET_OK;
    EPNET_REQUIRE(anchors && pred_reg && anchor_size && boxes);
    if (channels > handover::kMaxChannels || div_up64(rows, 64) > 0x7fffffffll) return EPNET_ELIMIT;
    return handover::launch_decode(rows, anchor_cols, anchors, pred_reg, channels, bins_xz, bins_y, loc_scope, loc_bin_size,
                                   loc_y_scope, loc_y_bin_size, num_head_bin, anchor_size, xz_fine, y_by_bin, ry_fine, avg_by_bin,
                                   ry_with_bin, y_to_bottom, nullptr, 0.f, boxes, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int epnet_score_order(int b, int n, const float *scores, int64_t *order, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && n >= 0);
    if (b == 0) return EPNET_OK;
    if (n < 1 || n > handover::kOrderMaxN || b > handover::kOrderMaxB) return EPNET_ELIMIT;
    EPNET_REQUIRE(scores && order);
    return handover::launch_order(b, n, scores, order, (hipStream_t)stream);
}

extern "C" size_t epnet_rpn_handover_workspace_bytes(int b, int n, int distance_based, int pre_nms_top_n, int post_nms_top_n) {
    if (b <= 0 || b > 32767 || n < 1 || n > handover::kOrderMaxN || pre_nms_top_n < 0 || post_nms_top_n < 0) return 0;
    const size_t rows = (size_t)b * (size_t)n;
    Carver c;  // the decoded boxes, the score order, then the proposal layer's own workspace
    c.take(rows * 7 * sizeof(float));
    c.take(rows * sizeof(int64_t));
    return c.off + epnet_rpn_proposals_workspace_bytes(b, distance_based, pre_nms_top_n, post_nms_top_n);
}

extern "C" int epnet_rpn_handover(int b, int n, int channels, const float *scores, const float *rpn_reg, const float *xyz,
                                  int bins_xz, int bins_y, double loc_scope, double loc_bin_size, double loc_y_scope,
                                  double loc_y_bin_size, int num_head_bin, const float *anchor_size, int xz_fine, int y_by_bin,
                                  int ry_fine, int avg_by_bin, int ry_with_bin, float score_thresh, int distance_based,
                                  int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated, void *workspace,
                                  size_t workspace_bytes, float *ret_bbox3d, float *ret_scores, int *ret_count, float *seg_mask,
                                  float *pts_depth, float *proposals, int64_t *order, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && n >= 0 && pre_nms_top_n >= 0 && post_nms_top_n >= 1);
    const int rc0 = handover::validate(3, channels, bins_xz, bins_y, num_head_bin, xz_fine, y_by_bin, avg_by_bin);
    if (rc0) return rc0;
    if (b == 0) return EPNET_OK;
    if (n < 1 || n > handover::kOrderMaxN || b > 32767 || channels > handover::kMaxChannels) return EPNET_ELIMIT;
    EPNET_REQUIRE(scores && rpn_reg && xyz && anchor_size && ret_bbox3d && ret_scores);
    const size_t need = epnet_rpn_handover_workspace_bytes(b, n, distance_based, pre_nms_top_n, post_nms_top_n);
    if (!workspace || workspace_bytes < need) return EPNET_ENOMEM;
    EPNET_REQUIRE(((uintptr_t)workspace & 15) == 0);
    const size_t rows = (size_t)b * (size_t)n;
    char *ws = (char *)workspace;
    Carver c;
    float *ws_proposals = (float *)(ws + c.take(rows * 7 * sizeof(float)));
    int64_t *ws_order = (int64_t *)(ws + c.take(rows * sizeof(int64_t)));
    if (!proposals) proposals = ws_proposals;
    if (!order) order = ws_order;
    hipStream_t s = (hipStream_t)stream;
    int rc = handover::launch_decode((long long)rows, 3, xyz, rpn_reg, channels, bins_xz, bins_y, loc_scope, loc_bin_size, loc_y_scope,
                                     loc_y_bin_size, num_head_bin, anchor_size, xz_fine, y_by_bin, ry_fine, avg_by_bin, ry_with_bin,
                                     1, scores, score_thresh, proposals, seg_mask, pts_depth, s);
    if (rc) return rc;
    rc = handover::launch_order(b, n, scores, order, s);
    if (rc) return rc;
    return epnet_rpn_proposals(b, n, proposals, scores, order, distance_based, pre_nms_top_n, post_nms_top_n, nms_thresh, rotated,
                               ws + c.off, workspace_bytes - c.off, ret_bbox3d, ret_scores, ret_count, stream);
}
