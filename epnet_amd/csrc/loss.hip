// loss.hip -- the RPN / RCNN training losses with their gradients in one call (include/epnet_ops.h, epnet_box_loss) for gfx950.
//
// The reference (lib/net/train_functions.py:92-284 over lib/utils/loss_utils.py:79-350) selects the foreground rows by boolean
// masks, branches on their count on the host and runs well over a hundred small torch kernels forward and as many backward.
// Here a row (a point of the RPN, a ROI of the RCNN stage) is one lane's work, forward and closed-form backward together:
//
//   1. count      grid of at most kCountBlocks workgroups over the labels alone: foreground / positive / negative / valid rows
//                 as INTEGER partial counts (the means' 1 / count scales every row gradient, so it has to be known first);
//   2. rows       one wave per 64 consecutive rows. The wave folds the count partials (integers: any order gives the same
//                 number), computes the classification term of its rows, and -- if its ballot of the mask is not empty -- stages
//                 its 64 regression rows with 16-byte coalesced loads into LDS (odd row stride: lane-per-row reads are
//                 conflict-free), lets every foreground lane work on its own row there (three softmaxes, the residual terms, the
//                 axis-aligned IoU with its clamps) and overwrite the row with the scaled gradient, background lanes with zeros,
//                 and streams the tile back out coalesced. A wave without a foreground row writes its zero rows and leaves.
//                 Per-wave sums of the 13 float terms (xor butterfly 32 .. 1) go to partial[wave][16];
//   3. finish     one workgroup: thread t adds the partials of waves t, t + 256, ... in ascending order, the 64 lanes of a wave
//                 are combined by the butterfly and the four waves in order; thread 0 divides by the counts and writes `terms`.
// No float atomics, no allocation, no copy and no synchronisation: the bits depend on the inputs and the shape alone, and the
// call records into a graph. Arithmetic: fp32 in source order without contraction, divisions are divisions, expf / logf /
// log1pf are the accurate ones (the file is compiled without fast-math).
#include "common.h"

namespace epnet {
namespace loss {

constexpr int kCountBlocks = 256;      // upper bound of the count grid (its partials are 4 ints each)
constexpr int kCountThreads = 256;
constexpr int kCountRows = 4096;       // rows per count workgroup before the grid is capped
constexpr int kPartial = 16;           // floats per wave in the partial table (13 used)
constexpr int kMaxBins = 32;           // per_loc_bin_num and num_head_bin: the 64-row tile has to fit 64 KB of LDS
constexpr int kFinishThreads = 256;

enum Term { tTotal, tLoss, tCls, tClsPos, tClsNeg, tReg, tLoc, tAngle, tSize, tIou, tXBin, tZBin, tXRes, tZRes, tYOffset, tRyBin,
            tRyRes, tBranch, tFg, tPos, tNeg, tValid, tSizeUnweighted, tIouUnweighted, tCount };
static_assert(tCount == EPNET_BOX_LOSS_TERMS, "terms");
enum Part { pCls, pClsPos, pClsNeg, pXBin, pZBin, pXRes, pZRes, pY, pRyBin, pRyRes, pSize, pIou, pBranch, pCount };

struct Params {
    long long rows;
    int c, nb, nh, ry_fine, iou_bin, cls_type, count_blocks, vec;
    float scope, bs, bs_half, shift_hi, apc, apc_half, alpha, one_minus_alpha, gamma, fg_weight, w_cls, w_reg, w_cls_total,
        w_reg_total, w_train, ce_weight;
};

inline int count_blocks_of(long long rows) {
    const long long b = div_up64(rows, kCountRows);
    return (int)(b < 1 ? 1 : (b > kCountBlocks ? kCountBlocks : b));
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// torch.remainder: the sign of the divisor
__device__ __forceinline__ float py_mod(float a, float b) {
    float r = fmodf(a, b);
    if (r != 0.f && ((r < 0.f) != (b < 0.f))) r = r + b;
    return r;
}

__device__ __forceinline__ float smooth_l1(float d, float &grad) {
    const float a = fabsf(d);
    grad = a < 1.f ? d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

// ---- 1. counts -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCountThreads) void count_kernel(long long rows, const int *__restrict__ cls_label,
                                                              const int *__restrict__ reg_mask, int *__restrict__ counts) {
    __shared__ int s_c[kCountThreads / 64][4];
    const long long per = (rows + gridDim.x - 1) / gridDim.x, chunk = (per + 63) / 64 * 64;   // rows per workgroup
    const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    int fg = 0, pos = 0, neg = 0, valid = 0;
    for (long long r = r0 + threadIdx.x; r < r1; r += kCountThreads) {
        const int l = cls_label[r];
        fg += (reg_mask ? reg_mask[r] > 0 : l > 0) ? 1 : 0;
        pos += l > 0 ? 1 : 0;
        neg += l == 0 ? 1 : 0;
        valid += l >= 0 ? 1 : 0;
    }
    fg = wave_sum_i32(fg); pos = wave_sum_i32(pos); neg = wave_sum_i32(neg); valid = wave_sum_i32(valid);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) { s_c[wave][0] = fg; s_c[wave][1] = pos; s_c[wave][2] = neg; s_c[wave][3] = valid; }
    __syncthreads();
    if (threadIdx.x < 4) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < kCountThreads / 64; ++w) v += s_c[w][threadIdx.x];
        counts[blockIdx.x * 4 + threadIdx.x] = v;
    }
}

__device__ __forceinline__ void total_counts(const Params &p, const int *__restrict__ counts, int &fg, int &pos, int &neg, int &valid) {
    fg = pos = neg = valid = 0;
    for (int i = lane_id(); i < p.count_blocks; i += 64) {
        const int4 v = reinterpret_cast<const int4 *>(counts)[i];
        fg += v.x; pos += v.y; neg += v.z; valid += v.w;
    }
    fg = wave_sum_i32(fg); pos = wave_sum_i32(pos); neg = wave_sum_i32(neg); valid = wave_sum_i32(valid);
}

// softmax statistics of n logits of a row in LDS: the maximum and the sum of exp(x - max)
__device__ __forceinline__ void softmax_stats(const float *x, int n, float &m, float &se) {
    m = x[0];
    for (int k = 1; k < n; ++k) m = fmaxf(m, x[k]);
    se = 0.f;
    for (int k = 0; k < n; ++k) se = se + expf(x[k] - m);
}

// one axis of the axis-aligned intersection: clamped length, d / d centre and d / d extent of the prediction
__device__ __forceinline__ float axis_overlap(float pc, float pe, float tc, float te, float &d_centre, float &d_extent) {
    const float p_hi = pc + pe / 2.f, t_hi = tc + te / 2.f, p_lo = pc - pe / 2.f, t_lo = tc - te / 2.f;
    const float raw = fminf(p_hi, t_hi) - fmaxf(p_lo, t_lo);
    const bool live = raw > 1e-3f;
    const float hi_p = p_hi < t_hi ? 1.f : 0.f, lo_p = p_lo > t_lo ? 1.f : 0.f;
    d_centre = live ? hi_p - lo_p : 0.f;
    d_extent = live ? (hi_p + lo_p) * 0.5f : 0.f;
    return live ? raw : 1e-3f;
}

// ---- 2. rows -------------------------------------------------------------------------------------------------------------
// grid ceil(rows / 64) workgroups of ONE wave; dynamic LDS: 64 rows of stride (c | 1) floats
__global__ __launch_bounds__(64) void rows_kernel(Params p, const float *__restrict__ cls_logit, const float *__restrict__ pred_reg,
                                                  const float *__restrict__ reg_label, const int *__restrict__ cls_label,
                                                  const int *__restrict__ reg_mask, const float *__restrict__ iou_branch,
                                                  const float *__restrict__ anchor, const int *__restrict__ counts,
                                                  float *__restrict__ grad_cls, float *__restrict__ grad_reg,
                                                  float *__restrict__ grad_branch, float *__restrict__ partial) {
    extern __shared__ float s_tile[];
    const int lane = lane_id();
    const long long wg = blockIdx.x;
    const long long row0 = wg * 64, row = row0 + lane;
    const bool in = row < p.rows;
    const int tile_rows = (int)(p.rows - row0 < 64 ? p.rows - row0 : 64);
    const int c = p.c, stride = c | 1;
    int n_fg, n_pos, n_neg, n_valid;
    total_counts(p, counts, n_fg, n_pos, n_neg, n_valid);
    const float denom = (float)(n_fg > 1 ? n_fg : 1);

    const int label = in ? cls_label[row] : -1;
    const bool fg = in && (reg_mask ? reg_mask[row] > 0 : label > 0);
    const float x = in ? cls_logit[row] : 0.f;
    const float prob = 1.f / (1.f + expf(-x));
    float part[pCount];
#pragma unroll
    for (int k = 0; k < pCount; ++k) part[k] = 0.f;

    // ---- classification, every row
    float g_cls = 0.f;
    const float t = label > 0 ? 1.f : 0.f;
    if (p.cls_type == 0) {            // sigmoid focal loss, weights (pos + neg) / max(sum pos, 1)
        const float w = (label >= 0 ? 1.f : 0.f) / (float)(n_pos > 1 ? n_pos : 1);
        const float ce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
        const float u = t * (1.f - prob) + (1.f - t) * prob;
        float mod, dmod;
        if (p.gamma == 2.f) { mod = u * u; dmod = 2.f * u; }
        else if (p.gamma != 0.f) { mod = powf(u, p.gamma); dmod = p.gamma * powf(u, p.gamma - 1.f); }
        else { mod = 1.f; dmod = 0.f; }
        const float aw = t * p.alpha + (1.f - t) * p.one_minus_alpha;
        const float per = in ? mod * aw * ce * w : 0.f;
        part[pCls] = per;
        part[pClsPos] = label > 0 ? per : 0.f;
        part[pClsNeg] = label == 0 ? per : 0.f;
        g_cls = p.w_cls_total * aw * w * (dmod * (1.f - 2.f * t) * prob * (1.f - prob) * ce + mod * (prob - t));
    } else if (p.cls_type == 1) {     // binary cross-entropy on the sigmoid, logs clamped at -100, rows with label -1 masked out
        const float valid = label >= 0 ? 1.f : 0.f;
        const float w = label > 0 ? p.fg_weight : 1.f;
        const float per = -w * (t * fmaxf(logf(prob), -100.f) + (1.f - t) * fmaxf(logf(1.f - prob), -100.f));
        const float norm = (float)(n_valid > 1 ? n_valid : 1);
        part[pCls] = in && label >= 0 ? per : 0.f;
        g_cls = p.w_cls_total * valid / norm * w * (prob - t) / fmaxf((1.f - prob) * prob, 1e-12f) * (prob * (1.f - prob));
    }

    const unsigned long long any_fg = __ballot(fg);
    const size_t tile_off = (size_t)row0 * (size_t)c;
    const int n = tile_rows * c;                    // floats of this wave's tile
    float g_branch = 0.f;
    if (any_fg == 0ull) {
        // no foreground row in this wave: zero rows, written coalesced
        float *out = grad_reg + tile_off;
        if (p.vec) {
            for (int i = lane * 4; i + 3 < n; i += 256) *reinterpret_cast<float4 *>(out + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = (n & ~3) + lane; i < n; i += 64) out[i] = 0.f;
        } else {
            for (int i = lane; i < n; i += 64) out[i] = 0.f;
        }
    } else {
        // ---- stage the tile: element e of the tile belongs to row e / c, column e % c, kept incrementally
        const float *src = pred_reg + tile_off;
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
        __syncthreads();
        float *q = s_tile + lane * stride;            // this lane's row
        if (!fg) {
            if (in) for (int k = 0; k < c; ++k) q[k] = 0.f;
        } else {
            const int nb = p.nb, nh = p.nh;
            const int o_xb = 0, o_zb = nb, o_xr = 2 * nb, o_zr = 3 * nb, o_y = 4 * nb, o_rb = 4 * nb + 1, o_rr = o_rb + nh, o_sz = o_rr + nh;
            const float *lb = reg_label + (size_t)row * 7;
            const float lx = lb[0], ly = lb[1], lz = lb[2], lh = lb[3], lw = lb[4], ll = lb[5], lry = lb[6];
            const float a_h = anchor[0], a_w = anchor[1], a_l = anchor[2];
            const float scale = p.w_reg_total / denom;
            // labels of the two location axes
            const float xs = fminf(fmaxf(lx + p.scope, 0.f), p.shift_hi), zs = fminf(fmaxf(lz + p.scope, 0.f), p.shift_hi);
            int xb = (int)floorf(xs / p.bs), zb = (int)floorf(zs / p.bs);
            xb = min(max(xb, 0), nb - 1); zb = min(max(zb, 0), nb - 1);
            const float x_res = xs - ((float)xb * p.bs + p.bs_half), z_res = zs - ((float)zb * p.bs + p.bs_half);
            const float x_resn = x_res / p.bs, z_resn = z_res / p.bs;
            // the heading label
            constexpr float kTwoPi = (float)(2.0 * M_PI), kPi = (float)M_PI, kHalfPi = (float)(M_PI * 0.5), kQuarterPi = (float)(M_PI * 0.25);
            float shift;
            if (p.ry_fine) {
                float ry = py_mod(lry, kTwoPi);
                if (ry > kHalfPi && ry < (float)(M_PI * 1.5)) ry = py_mod(ry + kPi, kTwoPi);
                shift = py_mod(ry + kHalfPi, kTwoPi);
                shift = fminf(fmaxf(shift - kQuarterPi, 1e-3f), (float)(M_PI * 0.5 - 1e-3));
            } else {
                shift = py_mod(py_mod(lry, kTwoPi) + p.apc_half, kTwoPi);
            }
            int rb = (int)floorf(shift / p.apc);
            rb = min(max(rb, 0), nh - 1);
            const float r_resn = (shift - ((float)rb * p.apc + p.apc_half)) / p.apc_half;

            float m_x, se_x, m_z, se_z, m_r, se_r;
            softmax_stats(q + o_xb, nb, m_x, se_x);
            softmax_stats(q + o_zb, nb, m_z, se_z);
            softmax_stats(q + o_rb, nh, m_r, se_r);
            part[pXBin] = logf(se_x) - (q[o_xb + xb] - m_x);
            part[pZBin] = logf(se_z) - (q[o_zb + zb] - m_z);
            part[pRyBin] = logf(se_r) - (q[o_rb + rb] - m_r);
            float d_xr, d_zr, d_y, d_rr, d_sz[3];
            part[pXRes] = smooth_l1(q[o_xr + xb] - x_resn, d_xr);
            part[pZRes] = smooth_l1(q[o_zr + zb] - z_resn, d_zr);
            part[pY] = smooth_l1(q[o_y] - ly, d_y);
            part[pRyRes] = smooth_l1(q[o_rr + rb] - r_resn, d_rr);
            const float sz0 = q[o_sz], sz1 = q[o_sz + 1], sz2 = q[o_sz + 2];
            float s_sum = smooth_l1(sz0 - (lh - a_h) / a_h, d_sz[0]);
            s_sum = s_sum + smooth_l1(sz1 - (lw - a_w) / a_w, d_sz[1]);
            s_sum = s_sum + smooth_l1(sz2 - (ll - a_l) / a_l, d_sz[2]);
            part[pSize] = s_sum;

            // ---- the IoU term: axis-aligned boxes, x <-> l, y <-> h, z <-> w
            const float ph = sz0 * a_h + a_h, pw = sz1 * a_w + a_w, pl = sz2 * a_l + a_l;
            float px, pz, tx, tz;
            if (p.iou_bin) {
                px = 0.f; pz = 0.f;
                for (int k = 0; k < nb; ++k) {
                    const float centre = (float)k * p.bs + p.bs_half - p.scope;
                    px = px + (centre + q[o_xr + k] * p.bs) * (expf(q[o_xb + k] - m_x) / se_x);
                    pz = pz + (centre + q[o_zr + k] * p.bs) * (expf(q[o_zb + k] - m_z) / se_z);
                }
                tx = ((float)xb * p.bs + p.bs_half - p.scope) + x_res;
                tz = ((float)zb * p.bs + p.bs_half - p.scope) + z_res;
            } else {
                px = q[o_xr + xb] * p.bs; pz = q[o_zr + zb] * p.bs;
                tx = x_res; tz = z_res;
            }
            float dix_c, dix_e, diy_c, diy_e, diz_c, diz_e;
            const float ix = axis_overlap(px, pl, tx, ll, dix_c, dix_e);
            const float iy = axis_overlap(q[o_y], ph, ly, lh, diy_c, diy_e);
            const float iz = axis_overlap(pz, pw, tz, lw, diz_c, diz_e);
            const float inter = ix * iy * iz;
            const float vol_raw = ph * pw * pl;
            const bool vol_live = vol_raw > 1e-3f;
            const float vol = vol_live ? vol_raw : 1e-3f;
            const float uni = vol + lh * lw * ll - inter;
            const float iou = inter / uni;
            const float v = prob * iou;
            const bool v_live = v > 1e-4f;
            part[pIou] = -logf(v_live ? v : 1e-4f);
            const float g_inter = v_live ? -(uni + inter) / (inter * uni) * p.ce_weight : 0.f;
            const float g_vol = v_live && vol_live ? 1.f / uni * p.ce_weight : 0.f;
            g_cls = g_cls + (v_live ? -(1.f - prob) * p.ce_weight : 0.f) * scale;
            const float g_ix = g_inter * iy * iz, g_iy = g_inter * ix * iz, g_iz = g_inter * ix * iy;
            const float g_h = g_iy * diy_e + g_vol * pw * pl, g_w = g_iz * diz_e + g_vol * ph * pl, g_l = g_ix * dix_e + g_vol * ph * pw;
            const float g_px = g_ix * dix_c, g_pz = g_iz * diz_c;
            if (iou_branch) {
                const float qb = iou_branch[row];
                const float qc = fminf(fmaxf(qb, 1e-4f), 0.9999f), tg = fminf(fmaxf(iou, 1e-4f), 0.9999f);
                part[pBranch] = -(tg * logf(qc) + (1.f - tg) * logf(1.f - qc));
                g_branch = scale * ((qb > 1e-4f && qb < 0.9999f) ? -(tg / qc - (1.f - tg) / (1.f - qc)) : 0.f);
            }
            // ---- the row's gradient replaces the row (every column is read before it is written)
            for (int k = 0; k < nb; ++k) {
                const float sx = expf(q[o_xb + k] - m_x) / se_x, sz = expf(q[o_zb + k] - m_z) / se_z;
                const float centre = (float)k * p.bs + p.bs_half - p.scope;
                const float ax = centre + q[o_xr + k] * p.bs, az = centre + q[o_zr + k] * p.bs;
                float gxb = sx - (k == xb ? 1.f : 0.f), gzb = sz - (k == zb ? 1.f : 0.f);
                float gxr = k == xb ? d_xr : 0.f, gzr = k == zb ? d_zr : 0.f;
                if (p.iou_bin) {
                    gxb = gxb + g_px * sx * (ax - px); gzb = gzb + g_pz * sz * (az - pz);
                    gxr = gxr + g_px * p.bs * sx; gzr = gzr + g_pz * p.bs * sz;
                } else {
                    gxr = gxr + (k == xb ? g_px * p.bs : 0.f); gzr = gzr + (k == zb ? g_pz * p.bs : 0.f);
                }
                q[o_xb + k] = gxb * scale; q[o_zb + k] = gzb * scale;
                q[o_xr + k] = gxr * scale; q[o_zr + k] = gzr * scale;
            }
            q[o_y] = (d_y + g_iy * diy_c) * scale;
            for (int k = 0; k < nh; ++k) {
                const float sr = expf(q[o_rb + k] - m_r) / se_r;
                q[o_rb + k] = (sr - (k == rb ? 1.f : 0.f)) * scale;
                q[o_rr + k] = (k == rb ? d_rr : 0.f) * scale;
            }
            q[o_sz] = (d_sz[0] + g_h * a_h) * scale;
            q[o_sz + 1] = (d_sz[1] + g_w * a_w) * scale;
            q[o_sz + 2] = (d_sz[2] + g_l * a_l) * scale;
        }
        __syncthreads();
        // ---- the tile goes out as it came in
        float *out = grad_reg + tile_off;
        if (p.vec) {
            int e = lane * 4, r = e / c, col = e - r * c;
            const int dr = 256 / c, dc = 256 - dr * c;
            for (; e + 3 < n; e += 256) {
                float vv[4];
                int rr = r, cc = col;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    vv[k] = s_tile[rr * stride + cc];
                    if (++cc == c) { cc = 0; ++rr; }
                }
                *reinterpret_cast<float4 *>(out + e) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                r += dr; col += dc;
                if (col >= c) { col -= c; ++r; }
            }
            for (int i = (n & ~3) + lane; i < n; i += 64) { const int rr = i / c; out[i] = s_tile[rr * stride + (i - rr * c)]; }
        } else {
            for (int i = lane; i < n; i += 64) { const int rr = i / c; out[i] = s_tile[rr * stride + (i - rr * c)]; }
        }
    }
    if (in) {
        grad_cls[row] = g_cls;
        if (grad_branch) grad_branch[row] = g_branch;
    }
    float *pp = partial + (size_t)wg * kPartial;
#pragma unroll
    for (int k = 0; k < pCount; ++k) {
        const float s = wave_sum_f32(part[k]);
        if (lane == 0) pp[k] = s;
    }
}

// ---- 3. finish -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(Params p, long long waves, const int *__restrict__ counts,
                                                                const float *__restrict__ partial, float *__restrict__ terms) {
    __shared__ float s_w[kFinishThreads / 64][pCount];
    float acc[pCount];
#pragma unroll
    for (int k = 0; k < pCount; ++k) acc[k] = 0.f;
    for (long long w = threadIdx.x; w < waves; w += kFinishThreads) {
        const float *pp = partial + (size_t)w * kPartial;
#pragma unroll
        for (int k = 0; k < pCount; ++k) acc[k] = acc[k] + pp[k];
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < pCount; ++k) {
        const float s = wave_sum_f32(acc[k]);
        if (lane_id() == 0) s_w[wave][k] = s;
    }
    int n_fg, n_pos, n_neg, n_valid;
    total_counts(p, counts, n_fg, n_pos, n_neg, n_valid);
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s[pCount];
#pragma unroll
    for (int k = 0; k < pCount; ++k) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kFinishThreads / 64; ++w) v = v + s_w[w][k];
        s[k] = v;
    }
    const float denom = (float)(n_fg > 1 ? n_fg : 1);
    float out[tCount];
    out[tFg] = (float)n_fg; out[tPos] = (float)n_pos; out[tNeg] = (float)n_neg; out[tValid] = (float)n_valid;
    out[tCls] = p.cls_type == 1 ? s[pCls] / (float)(n_valid > 1 ? n_valid : 1) : s[pCls];
    out[tClsPos] = s[pClsPos]; out[tClsNeg] = s[pClsNeg];
    out[tXBin] = s[pXBin] / denom; out[tZBin] = s[pZBin] / denom; out[tXRes] = s[pXRes] / denom; out[tZRes] = s[pZRes] / denom;
    out[tYOffset] = s[pY] / denom; out[tRyBin] = s[pRyBin] / denom; out[tRyRes] = s[pRyRes] / denom;
    out[tBranch] = s[pBranch] / denom;
    out[tSizeUnweighted] = s[pSize] / (3.f * denom);
    out[tSize] = 3.f * out[tSizeUnweighted];
    out[tIouUnweighted] = s[pIou] / denom;
    out[tIou] = p.ce_weight * out[tIouUnweighted];
    out[tLoc] = out[tXBin] + out[tZBin] + out[tXRes] + out[tZRes] + out[tYOffset];
    out[tAngle] = out[tRyBin] + out[tRyRes];
    out[tReg] = out[tLoc] + out[tAngle] + out[tSize] + out[tIou] + out[tBranch];
    out[tLoss] = out[tCls] * p.w_cls + out[tReg] * p.w_reg;
    out[tTotal] = out[tLoss] * p.w_train;
#pragma unroll
    for (int k = 0; k < tCount; ++k) terms[k] = out[k];
}

inline size_t workspace_bytes(long long rows) {
    return (size_t)kCountBlocks * 4 * sizeof(int) + (size_t)div_up64(rows, 64) * kPartial * sizeof(float);
}

}  // namespace loss
}  // namespace epnet

using namespace epnet;

extern "C" size_t epnet_box_loss_workspace_bytes(long long rows, int c) {
    if (rows <= 0 || c <= 0) return 0;
    return loss::workspace_bytes(rows);
}

extern "C" int epnet_box_loss(long long rows, int c, double loc_scope, double loc_bin_size, int num_head_bin, int ry_fine,
                              int iou_loss_type, int cls_loss_type, double focal_alpha, double focal_gamma, double fg_weight,
                              double w_cls, double w_reg, double w_train, double ce_weight, const float *cls_logit,
                              const float *pred_reg, const float *reg_label, const int *cls_label, const int *reg_mask,
                              const float *iou_branch_pred, const float *anchor, float *terms, float *grad_cls, float *grad_reg,
                              float *grad_iou_branch, void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    EPNET_REQUIRE(rows >= 0 && c > 0 && num_head_bin > 0 && loc_scope > 0 && loc_bin_size > 0);
    EPNET_REQUIRE(iou_loss_type == EPNET_LOSS_IOU_RAW || iou_loss_type == EPNET_LOSS_IOU_CLS_MASK_WITH_BIN);
    EPNET_REQUIRE(cls_loss_type == EPNET_LOSS_CLS_FOCAL || cls_loss_type == EPNET_LOSS_CLS_BCE || cls_loss_type == EPNET_LOSS_CLS_NONE);
    const double bins = loc_scope / loc_bin_size;
    EPNET_REQUIRE(bins >= 1 && bins < 1e6);
    const int nb = (int)bins * 2;                                        // per_loc_bin_num, loss_utils.py:113
    EPNET_REQUIRE((long long)c == 4ll * nb + 1 + 2ll * num_head_bin + 3);
    if (rows == 0) return EPNET_OK;
    EPNET_REQUIRE(cls_logit && pred_reg && reg_label && cls_label && anchor && terms && grad_cls && grad_reg);
    EPNET_REQUIRE((iou_branch_pred == nullptr) == (grad_iou_branch == nullptr));
    const long long waves = div_up64(rows, 64);
    if (nb > loss::kMaxBins || num_head_bin > loss::kMaxBins || waves > 0x7fffffffll) return EPNET_ELIMIT;
    if (!workspace || workspace_bytes < loss::workspace_bytes(rows)) return EPNET_ENOMEM;
    EPNET_REQUIRE(((uintptr_t)workspace & 15) == 0);
    loss::Params p;
    p.rows = rows; p.c = c; p.nb = nb; p.nh = num_head_bin; p.ry_fine = ry_fine ? 1 : 0;
    p.iou_bin = iou_loss_type == EPNET_LOSS_IOU_CLS_MASK_WITH_BIN; p.cls_type = cls_loss_type;
    p.count_blocks = loss::count_blocks_of(rows);
    p.vec = (((uintptr_t)pred_reg | (uintptr_t)grad_reg) & 15) == 0;
    // the constants as torch forms them: Python doubles, rounded to fp32 where they meet a tensor
    const double apc = ry_fine ? (M_PI / 2) / num_head_bin : (2 * M_PI) / num_head_bin;
    p.scope = (float)loc_scope; p.bs = (float)loc_bin_size; p.bs_half = (float)(loc_bin_size / 2);
    p.shift_hi = (float)(loc_scope * 2 - 1e-3);
    p.apc = (float)apc; p.apc_half = (float)(apc / 2);
    p.alpha = (float)focal_alpha; p.one_minus_alpha = (float)(1 - focal_alpha); p.gamma = (float)focal_gamma;
    p.fg_weight = (float)fg_weight; p.w_cls = (float)w_cls; p.w_reg = (float)w_reg; p.w_train = (float)w_train;
    p.w_cls_total = p.w_cls * p.w_train; p.w_reg_total = p.w_reg * p.w_train; p.ce_weight = (float)ce_weight;
    int *counts = (int *)workspace;
    float *partial = (float *)((char *)workspace + (size_t)loss::kCountBlocks * 4 * sizeof(int));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loss::count_kernel, dim3(p.count_blocks), dim3(loss::kCountThreads), 0, st, rows, cls_label, reg_mask, counts);
    const size_t lds = (size_t)64 * (c | 1) * sizeof(float);
    hipLaunchKernelGGL(loss::rows_kernel, dim3((unsigned)waves), dim3(64), lds, st, p, cls_logit, pred_reg, reg_label, cls_label,
                       reg_mask, iou_branch_pred, anchor, (const int *)counts, grad_cls, grad_reg, grad_iou_branch, partial);
    hipLaunchKernelGGL(loss::finish_kernel, dim3(1), dim3(loss::kFinishThreads), 0, st, p, waves, (const int *)counts,
                       (const float *)partial, terms);
    return check_launch("box_loss");
}
