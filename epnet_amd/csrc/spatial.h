// spatial.h -- Morton keys and an in-LDS bitonic sort, shared by the pruned FPS and ball-query kernels.
// The spatial order only decides WHICH work can be skipped; results never depend on it.
#pragma once
#include "common.h"
#include "dpp.h"
#include "scene_index_layout.h"

namespace epnet {

__device__ __forceinline__ unsigned spread10(unsigned v) {  // ..9876543210 -> ..9__8__7__6__5__4__3__2__1__0
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Morton code of p inside the cube [lo, lo + 1023/scale]^3 (one cell size for all axes)
__device__ __forceinline__ unsigned morton30(float px, float py, float pz, const float (&lo)[3], float scale) {
    const unsigned ix = (unsigned)fminf((px - lo[0]) * scale, 1023.f);
    const unsigned iy = (unsigned)fminf((py - lo[1]) * scale, 1023.f);
    const unsigned iz = (unsigned)fminf((pz - lo[2]) * scale, 1023.f);
    return spread10(ix) | (spread10(iy) << 1) | (spread10(iz) << 2);
}

// ascending bitonic sort of np (a power of two) 64-bit keys in LDS by all threads of the block;
// ends with a barrier
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long *keys, int np) {
    const int q = threadIdx.x, T = blockDim.x;
    for (int k2 = 2; k2 <= np; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = q; i < np / 2; i += T) {
                const int a = ((i & ~(j2 - 1)) << 1) | (i & (j2 - 1));
                const int b = a | j2;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool up = (a & k2) == 0;
                if ((ka > kb) == up) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            __syncthreads();
        }
}

// inclusive prefix sum over the 64 lanes (DPP row shifts + row broadcasts)
__device__ __forceinline__ int wave_inclusive_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);  // row_bcast15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);  // row_bcast31 -> rows 2, 3
    return v;
}

// bounding box of n points (xyz interleaved) by all threads of the block; s_box is 6 x 16 floats of LDS.
// On return lo[] / ext[] hold the minimum corner and the extents.
__device__ __forceinline__ void block_bbox3(const float *__restrict__ xyz, int n, float (*s_box)[16], float (&lo)[3],
                                            float (&ext)[3]) {
    const int q = threadIdx.x, T = blockDim.x, lane = q & 63, wave = q >> 6, nw = T >> 6;
    float hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    lo[0] = lo[1] = lo[2] = 3.4e38f;
    for (int k = q; k < n; k += T)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[k * 3 + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
        if (lane == 0) {
            s_box[a][wave] = lo[a];
            s_box[3 + a][wave] = hi[a];
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = s_box[a][0], h = s_box[3 + a][0];
        for (int w = 1; w < nw; ++w) {
            l = fminf(l, s_box[a][w]);
            h = fmaxf(h, s_box[3 + a][w]);
        }
        lo[a] = l;
        ext[a] = h - l;
    }
}

// ---- cell sort: counting sort of the points by a <= 14-bit interleaved cell code ---------------------
// A uniform grid (one cell size for all axes, power-of-two cell counts per axis, at most 2^14 cells in
// all) is laid over the scene; a point's code interleaves the bits of its cell coordinates, so that
// consecutive codes are neighbouring cells. One histogram pass, one scan, one scatter -- ~20x cheaper
// than a full Morton sort, and buckets of 64 consecutive points are just as compact at the scale of a
// cell. The order INSIDE a cell is whatever the LDS atomics produce: the layout only decides which work
// can be skipped, never a result. (kCellBits, kCells: scene_index_layout.h)

struct CellGrid {
    float lo[3];
    float inv;    // 1 / cell size
    int bits[3];  // log2(cells) per axis
};

__device__ __forceinline__ CellGrid make_cell_grid(const float (&lo)[3], const float (&ext)[3], int max_bits = kCellBits) {
    CellGrid g;
    const float big = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
    float cell = big > 0.f ? big / 64.f : 1.f;
    for (int iter = 0; iter < 8; ++iter) {
        int total = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int cells = (int)(ext[a] / cell) + 1;
            int b = 0;
            while ((1 << b) < cells && b < 6) ++b;
            g.bits[a] = b;
            total += b;
        }
        if (total <= max_bits) break;
        cell *= 1.26f;  // ~ one bit less in total every 3 iterations
    }
    g.lo[0] = lo[0]; g.lo[1] = lo[1]; g.lo[2] = lo[2];
    g.inv = 1.f / cell;
    return g;
}

__device__ __forceinline__ unsigned cell_code(const CellGrid &g, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    unsigned c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int hi = (1 << g.bits[a]) - 1;
        const int v = (int)((p[a] - g.lo[a]) * g.inv);
        c[a] = (unsigned)min(max(v, 0), hi);
    }
    unsigned code = 0;
    int pos = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (b < g.bits[a]) {
                code |= ((c[a] >> b) & 1u) << pos;
                ++pos;
            }
    return code;
}

// padded histogram index: thread-contiguous runs of `per` bins hit distinct LDS banks
__device__ __forceinline__ int hist_at(int b, int per_shift) { return b + (b >> per_shift); }
__device__ __forceinline__ int cell_hist_words(int threads) { return kCells + kCells / (kCells / threads) + 64; }

// perm[p] = index of the p-th point in cell order, p < n (perm has >= n entries; hist has
// cell_hist_words(blockDim.x) ints; s_part has 16 ints). blockDim.x must be a power of two <= 1024.
// All threads of the block call this; ends with a barrier.
__device__ __forceinline__ void cell_sort_lds(const float *__restrict__ xyz, int n, const CellGrid &g, int *hist,
                                              int *s_part, unsigned short *perm) {
    const int q = threadIdx.x, T = blockDim.x, lane = q & 63, wave = q >> 6, nw = T >> 6;
    const int per = kCells / T;  // bins per thread in the scan
    int per_shift = 0;
    while ((1 << per_shift) < per) ++per_shift;
    for (int i = q; i < cell_hist_words(T); i += T) hist[i] = 0;
    __syncthreads();
    for (int k = q; k < n; k += T)
        atomicAdd(&hist[hist_at((int)cell_code(g, xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2]), per_shift)], 1);
    __syncthreads();
    // exclusive scan: thread q owns bins [q*per, (q+1)*per)
    int sum = 0;
    for (int i = 0; i < per; ++i) sum += hist[hist_at(q * per + i, per_shift)];
    const int incl = wave_inclusive_scan(sum);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_part[w];
    (void)nw;
    for (int i = 0; i < per; ++i) {
        const int at = hist_at(q * per + i, per_shift);
        const int c = hist[at];
        hist[at] = base;
        base += c;
    }
    __syncthreads();
    for (int k = q; k < n; k += T) {
        const int pos = atomicAdd(&hist[hist_at((int)cell_code(g, xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2]), per_shift)], 1);
        perm[pos] = (unsigned short)k;
    }
    __syncthreads();
}

// ---- scene index (layout: scene_index_layout.h): the sampling kernel's scratch behind a scene of more than 16384 points
inline float *scene_index_sampling_scratch(int b, int n, void *index) {
    const size_t np = (size_t)scene_index_np(n);
    return (float *)((char *)index + (size_t)b * (np * sizeof(float4) + (np / 64 + np / 256) * 6 * sizeof(float)));
}

// ---- the index build of one scene by one workgroup (bq_index_kernel in ball_query.hip; the epilogue of a sampling kernel in
// fps.hip, which builds the NEXT level's index from the centres it has just picked) ------------------------------------
// kIxThreads threads, 2^BITS grid cells, kIxPerThread points per thread held in registers (kIxThreads * kIxPerThread >= n for the
// one-read path; kRegsOnly: the caller guarantees that, the re-reading paths are not compiled), kStageCap: rows of the staging
// buffer (0: a quarter of the scene). LDS comes from the caller: s_hist = (2^BITS + 2^BITS / per + 64) ints of histogram followed,
// 16-byte aligned, by the staging rows; s_box 6 x 16 floats, s_part 16 ints. All threads of the workgroup call it; blockIdx.x is
// the scene. src_idx / gathered (in-register path only): see bq_index_kernel.
#ifdef EPNET_IX_STATS  // diagnostic build only (profiles/micro/ix_stats.py): phase counters of the index build (wave 0)
#define EPNET_IX_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define EPNET_IX_STAMP(var)
#endif

template <int kIxThreads, int BITS, int kIxPerThread, int kStageCap, bool kRegsOnly>
__device__ __forceinline__ void scene_index_build_block(int *s_hist, float (*s_box)[16], int *s_part, int n, int np,
                                                        const float *__restrict__ xyz, float4 *__restrict__ sorted,
                                                        float *__restrict__ boxes, float *__restrict__ qboxes, int n_src,
                                                        const int *__restrict__ src_idx, float *__restrict__ gathered,
                                                        unsigned long long *ix_stats = nullptr) {
    constexpr int kCells = 1 << BITS;
    const int q = threadIdx.x, lane = q & 63, wave = q >> 6;
    // src_idx (n <= kIxThreads * kIxPerThread only): the scene's points are rows src_idx[0 .. n) of a cloud of n_src points -- the centres a
    // sampling has just picked -- and are written out in that order as well (gathered): the centre gather of an SA level and the
    // index build of the next one in one dispatch
    xyz += (size_t)blockIdx.x * (src_idx ? n_src : n) * 3;
    if (src_idx) {
        src_idx += (size_t)blockIdx.x * n;
        gathered += (size_t)blockIdx.x * n * 3;
    }
    sorted += (size_t)blockIdx.x * np;
    boxes += (size_t)blockIdx.x * (np / 64) * 6;
    // counting sort by cell, scattering the points (with their original index) straight to global memory.
    // Up to kIxPerThread points per thread the cloud is read ONCE into registers (bounding box, cell codes and the
    // scatter all work from there); bigger clouds re-read it per phase.
    constexpr int per = kCells / kIxThreads;
    constexpr int per_shift = per == 16 ? 4 : per == 8 ? 3 : per == 4 ? 2 : -1;
    static_assert(per_shift > 0, "scan layout");
    const bool in_regs = kRegsOnly || n <= kIxThreads * kIxPerThread;  // block-uniform
    float px[kIxPerThread], py[kIxPerThread], pz[kIxPerThread];
    float lo[3], ext[3];
    EPNET_IX_STAMP(t_0);
    if (in_regs) {
        float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
        // all of a thread's points are requested before the first one is used, and nothing below branches on `k < n`: with the
        // box update under an `if` every iteration was a basic block of its own and its load was waited for before the next
        // was issued -- 16 serial trips to HBM at the head of the sampling chain of every level
        int row[kIxPerThread];
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i) {
            const int k = q + i * kIxThreads;
            const int kk = k < n ? k : 0;
            row[i] = src_idx ? src_idx[kk] : kk;
        }
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i) {
            px[i] = xyz[row[i] * 3 + 0];
            py[i] = xyz[row[i] * 3 + 1];
            pz[i] = xyz[row[i] * 3 + 2];
        }
        if (src_idx) {
#pragma unroll
            for (int i = 0; i < kIxPerThread; ++i) {
                const int k = q + i * kIxThreads;
                if (k < n) {
                    gathered[k * 3 + 0] = px[i];
                    gathered[k * 3 + 1] = py[i];
                    gathered[k * 3 + 2] = pz[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i) {
            const bool ok = q + i * kIxThreads < n;
            mn[0] = fminf(mn[0], ok ? px[i] : 3.4e38f); mx[0] = fmaxf(mx[0], ok ? px[i] : -3.4e38f);
            mn[1] = fminf(mn[1], ok ? py[i] : 3.4e38f); mx[1] = fmaxf(mx[1], ok ? py[i] : -3.4e38f);
            mn[2] = fminf(mn[2], ok ? pz[i] : 3.4e38f); mx[2] = fmaxf(mx[2], ok ? pz[i] : -3.4e38f);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float l = wave_minf_all(mn[a]), h = wave_maxf_all(mx[a]);
            if (lane == 0) {
                s_box[a][wave] = l;
                s_box[3 + a][wave] = h;
            }
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = s_box[a][0], h = s_box[3 + a][0];
            for (int w = 1; w < kIxThreads / 64; ++w) {
                l = fminf(l, s_box[a][w]);
                h = fmaxf(h, s_box[3 + a][w]);
            }
            lo[a] = l;
            ext[a] = h - l;
        }
    } else {
        block_bbox3(xyz, n, s_box, lo, ext);
    }
    const CellGrid g = make_cell_grid(lo, ext, BITS);
    EPNET_IX_STAMP(t_1);
    for (int i = q; i < kCells + kCells / per + 64; i += kIxThreads) s_hist[i] = 0;
    __syncthreads();
    EPNET_IX_STAMP(t_2);
    // in_regs: the histogram pass keeps what its atomics return -- a point's rank inside its cell -- so the scatter below needs
    // no second round of atomics on the same (hot: a cell next to the sensor holds hundreds of points) words: 46 % of the kernel
    int code[kIxPerThread], rank[kIxPerThread];
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i) code[i] = hist_at((int)cell_code(g, px[i], py[i], pz[i]), per_shift);
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i)   // (a slot beyond n counts on one of the 64 spare words behind the histogram)
            rank[i] = atomicAdd(&s_hist[q + i * kIxThreads < n ? code[i] : kCells + kCells / per + lane], 1);
    } else {
        for (int k = q; k < n; k += kIxThreads)
            atomicAdd(&s_hist[hist_at((int)cell_code(g, xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2]), per_shift)], 1);
    }
    __syncthreads();
    EPNET_IX_STAMP(t_3);
    int sum = 0;
    for (int i = 0; i < per; ++i) sum += s_hist[hist_at(q * per + i, per_shift)];
    const int incl = wave_inclusive_scan(sum);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_part[w];
    for (int i = 0; i < per; ++i) {
        const int at = hist_at(q * per + i, per_shift);
        const int c = s_hist[at];
        s_hist[at] = base;
        base += c;
    }
    __syncthreads();
    EPNET_IX_STAMP(t_4);
    auto bucket_box = [&](int p, const float4 v) {  // one wave handles one bucket at a time (all 64 lanes active)
        const bool real = p < n;
        const float cx_ = canonical(v.x), cy_ = canonical(v.y), cz_ = canonical(v.z);   // (quiet NaNs drop out of the box, as with fminf)
        float mnx = real ? cx_ : 3.4e38f, mxx = real ? cx_ : -3.4e38f, mny = real ? cy_ : 3.4e38f, mxy = real ? cy_ : -3.4e38f,
              mnz = real ? cz_ : 3.4e38f, mxz = real ? cz_ : -3.4e38f;
        wave_box(mnx, mxx, mny, mxy, mnz, mxz);
        if (lane == 0) {
            float *bx = boxes + (p >> 6) * 6;
            const bool any = mnx <= mxx;  // an all-padding bucket gets a box no ball can reach
            bx[0] = any ? mnx : 3.0e38f; bx[1] = any ? mxx : 3.0e38f;
            bx[2] = any ? mny : 3.0e38f; bx[3] = any ? mxy : 3.0e38f;
            bx[4] = any ? mnz : 3.0e38f; bx[5] = any ? mxz : 3.0e38f;
        }
    };
    const bool staged = kRegsOnly || (in_regs && (np & 255) == 0);  // (three_nn's own index of a known set pads to 64 only: no whole-bucket quarters)
    if (staged) {
        // The sorted order goes through LDS, a quarter of the scene at a time: the points land in the staging buffer (scattered
        // 16-byte LDS writes), leave for global memory as whole rows (the scattered 16-byte global stores this replaces were
        // 46 % of the kernel: 4 M partial-line writes per 256 scenes) and give their bucket boxes on the way out (no read-back
        // of what was just written: another 20 %).
        float4 *s_stage = reinterpret_cast<float4 *>(s_hist + kCells + kCells / per + 64);
        int pos[kIxPerThread];
#pragma unroll
        for (int i = 0; i < kIxPerThread; ++i) pos[i] = s_hist[code[i]] + rank[i];   // start of the cell + rank inside it
        // a quarter of the scene per round; with kStageCap (the 256-thread kernel, a sampling kernel's epilogue) at most 512 points (8 KB): with 26 KB of LDS in all it still finds
        // room on a CU that holds two 64 KB workgroups of a row gather -- at 34 KB it waited for the whole gather to drain (260 us)
        // (a multiple of 64: np is a multiple of 256 here. A scene index has a power of two, three_nn's own index of a known set any
        // multiple of 64 -- 2304, 2816, 3328, 3840 are not whole rounds of 512: the last round is shorter)
        const int quarter = kStageCap ? min(np >> 2, kStageCap) : np >> 2;
        for (int h = 0; h * quarter < np; ++h) {
            const int base = h * quarter, len = min(quarter, np - base);
            for (int p = q; p < len; p += kIxThreads)   // padding rows: never inside a ball
                if (base + p >= n) s_stage[p] = make_float4(3.0e38f, 3.0e38f, 3.0e38f, __int_as_float(-1));
#pragma unroll
            for (int i = 0; i < kIxPerThread; ++i) {
                const int k = q + i * kIxThreads;
                if (k < n && (unsigned)(pos[i] - base) < (unsigned)quarter)
                    s_stage[pos[i] - base] = make_float4(px[i], py[i], pz[i], __int_as_float(k));
            }
            __syncthreads();
            for (int p = q; p < len; p += kIxThreads) {
                const float4 v = s_stage[p];
                sorted[base + p] = v;
                bucket_box(base + p, v);
            }
            __syncthreads();
        }
    } else {
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < kIxPerThread; ++i) {
                const int k = q + i * kIxThreads;
                if (k < n) sorted[s_hist[code[i]] + rank[i]] = make_float4(px[i], py[i], pz[i], __int_as_float(k));
            }
        } else {
            for (int k = q; k < n; k += kIxThreads) {
                const float x = xyz[k * 3 + 0], y = xyz[k * 3 + 1], z = xyz[k * 3 + 2];
                const int pos = atomicAdd(&s_hist[hist_at((int)cell_code(g, x, y, z), per_shift)], 1);
                sorted[pos] = make_float4(x, y, z, __int_as_float(k));
            }
        }
        for (int p = n + q; p < np; p += kIxThreads)  // padding: never inside a ball
            sorted[p] = make_float4(3.0e38f, 3.0e38f, 3.0e38f, __int_as_float(-1));
        __threadfence_block();
        __syncthreads();  // the scattered points are read back by other waves of this workgroup below
        for (int p = q; p < np; p += kIxThreads) bucket_box(p, sorted[p]);
    }
#ifdef EPNET_IX_STATS
    {
        EPNET_IX_STAMP(t_6);
        if (q == 0 && ix_stats) {
            atomicAdd(&ix_stats[0], t_1 - t_0); atomicAdd(&ix_stats[1], t_2 - t_1); atomicAdd(&ix_stats[2], t_3 - t_2);
            atomicAdd(&ix_stats[3], t_4 - t_3); atomicAdd(&ix_stats[4], t_6 - t_4);
            atomicAdd(&ix_stats[7], 1ull);
        }
    }
#endif
    if (!qboxes) return;
    // second level: one box per 4 consecutive buckets (256 sorted points)
    qboxes += (size_t)blockIdx.x * (np / 256) * 6;
    __threadfence_block();
    __syncthreads();
    for (int g = q; g < np / 256; g += kIxThreads) {
        float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
        for (int k = 0; k < 4; ++k) {
            const float *bx = boxes + (g * 4 + k) * 6;
            if (bx[0] < 3.0e38f)  // not an all-padding bucket
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    mn[a] = fminf(mn[a], bx[2 * a]);
                    mx[a] = fmaxf(mx[a], bx[2 * a + 1]);
                }
        }
        const bool any = mn[0] <= mx[0];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            qboxes[g * 6 + 2 * a] = any ? mn[a] : 3.0e38f;
            qboxes[g * 6 + 2 * a + 1] = any ? mx[a] : 3.0e38f;
        }
    }
}

// defined in ball_query.hip
// qboxes (one box per 4 buckets) may be NULL; src_idx / gathered (n <= 16384): see bq_index_kernel
int spatial_index_launch(int b, int n, int np, const float *xyz, float4 *sorted, float *boxes, float *qboxes, hipStream_t s,
                         int n_src = 0, const int *src_idx = nullptr, float *gathered = nullptr);

}  // namespace epnet
