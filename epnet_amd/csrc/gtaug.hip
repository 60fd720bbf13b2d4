// gtaug.hip -- ground-truth database augmentation of a whole batch with no host synchronisation (include/epnet_ops.h,
// epnet_gt_aug_place and epnet_gt_aug_points) for gfx950.
//
// The reference does this per scene on a host core, apply_gt_aug_to_one_scene (lib/datasets/kitti_rcnn_dataset.py:590-696): up to
// 100 tries of a database object, each placed on the road plane and tested against every box of the scene with two shapely
// polygons per pair, then one pts_in_boxes3d_cpu pass over the scene per accepted object. Here the draws are device tables and
// the work is two launches whatever the data:
//
//   place, one wave per scene: the tries run in the reference's order; the 64 lanes test one candidate against all current
//     boxes in parallel (float64 rectangle clip) and ballot; the current boxes -- the scene's boxes, then the accepted ones --
//     live in LDS as float64 rectangles. Its outputs say what was accepted, where its points go and which boxes clear points;
//   points, grid (row chunks, scenes): copies each accepted object's rows behind one another, lowered by the object's move.
//
// The removal of the scene's own points inside the accepted boxes and the sampling belong to epnet_scan_prepare_aug (scan.hip).
// Arithmetic: the placement in float64 rounded once to float32, the overlap decision in float64 on the float32 box values.
#include <math.h>

#include "common.h"

namespace epnet {
namespace gtaug {

constexpr int kMaxTries = EPNET_GT_AUG_MAX_TRIES;
constexpr int kMaxExisting = EPNET_GT_AUG_MAX_EXISTING;
constexpr int kMaxAccept = EPNET_GT_AUG_MAX_ACCEPT;
constexpr int kPointThreads = 256;

typedef float f4 __attribute__((ext_vector_type(4)));

struct Scope {
    double v[6];
};

// the BEV rectangle of a box in the corner order of kitti_utils.boxes3d_to_corners3d, its vertical interval and its area
struct Rect {
    double x[4], z[4], y0, y1, area;
    int solid;                                     // w != 0 and l != 0 (the reference's polygon is valid)
};

__device__ __forceinline__ Rect make_rect(float fx, float fy, float fz, float fh, float fw, float fl, float fry) {
    Rect r;
    const double x = fx, y = fy, z = fz, h = fh, w = fw, l = fl, ry = fry;
    const double c = cos(ry), s = sin(ry), hl = l / 2.0, hw = w / 2.0;
    const double dx[4] = {hl, hl, -hl, -hl}, dz[4] = {hw, -hw, -hw, hw};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.x[k] = (x + dx[k] * c) + dz[k] * s;
        r.z[k] = (z - dx[k] * s) + dz[k] * c;
    }
    r.y0 = y - h;
    r.y1 = y;
    r.area = fabs(w * l);
    r.solid = (fw != 0.f && fl != 0.f) ? 1 : 0;
    return r;
}

// area of the intersection of two rectangles: Sutherland-Hodgman clip of `a` by the four half-planes of `b`, shoelace sum
__device__ double clip_area(const Rect &a, const Rect &b) {
    double px[8], pz[8], qx[8], qz[8];
    int n = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) { px[k] = a.x[k]; pz[k] = a.z[k]; }
    double twice = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) twice += b.x[k] * b.z[(k + 1) & 3] - b.x[(k + 1) & 3] * b.z[k];
    const double sign = twice >= 0.0 ? 1.0 : -1.0;  // inside = left of a counter-clockwise edge
    for (int e = 0; e < 4; ++e) {
        const double ax = b.x[e], az = b.z[e], ex = b.x[(e + 1) & 3] - ax, ez = b.z[(e + 1) & 3] - az;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 < n ? i + 1 : 0;
            const double d0 = sign * (ex * (pz[i] - az) - ez * (px[i] - ax));
            const double d1 = sign * (ex * (pz[j] - az) - ez * (px[j] - ax));
            if (d0 >= 0.0 && m < 8) { qx[m] = px[i]; qz[m] = pz[i]; ++m; }
            if ((d0 >= 0.0) != (d1 >= 0.0) && m < 8) {
                const double t = d0 / (d0 - d1);
                qx[m] = px[i] + t * (px[j] - px[i]);
                qz[m] = pz[i] + t * (pz[j] - pz[i]);
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) { px[i] = qx[i]; pz[i] = qz[i]; }
    }
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        sum += px[i] * pz[j] - px[j] * pz[i];
    }
    return fabs(sum / 2.0);
}

// the reference's rejection: iou3d >= 1e-8 (kitti_utils.get_iou3d :198-238), cand = its `A`, cur = its `B`
__device__ bool overlaps(const Rect &cand, const Rect &cur) {
    const double h_overlap = fmin(cand.y1, cur.y1) - fmax(cand.y0, cur.y0);
    if (!(h_overlap > 0.0)) return false;
    const double bottom = (cand.solid && cur.solid) ? clip_area(cand, cur) : 0.0;
    const double overlap3d = bottom * h_overlap;
    const double union3d = (cand.area * (cand.y1 - cand.y0) + cur.area * (cur.y1 - cur.y0)) - overlap3d;
    return overlap3d / union3d >= 1e-8;
}

struct PlaceOut {
    int *acc_db;
    float *acc_box;
    double *acc_move;
    int *acc_row0;
    float *remove_boxes, *gt_out, *alpha_out;
    int *info;
};

// ---- place: grid (b), one wave per scene
__global__ __launch_bounds__(kWave) void place_kernel(int T, int a, int g, int k_max, int e, int D, int reduce_by_range, Scope scope,
                                                      const float *__restrict__ db_boxes, const float *__restrict__ db_alpha,
                                                      const int *__restrict__ db_npts, const int *__restrict__ apply,
                                                      const int *__restrict__ extra_num, const int *__restrict__ cand,
                                                      const float *__restrict__ all_boxes, const int *__restrict__ num_all,
                                                      const float *__restrict__ gt_boxes, const float *__restrict__ gt_alpha,
                                                      const int *__restrict__ num_gt, const double *__restrict__ road_plane, PlaceOut o) {
    __shared__ Rect s_cur[kMaxExisting + kMaxAccept];
    __shared__ float s_box[kMaxAccept][8];          // the placed box and alpha of each accepted object
    __shared__ double s_move[kMaxAccept];
    __shared__ int s_db[kMaxAccept], s_row0[kMaxAccept];
    const int bs = blockIdx.x, lane = threadIdx.x;
    const int na = min(max(num_all[bs], 0), a), ng = min(max(num_gt[bs], 0), g);
    const int applied = apply[bs] != 0 ? 1 : 0;
    const int extra = min(extra_num[bs], k_max - 1);   // cnt <= extra + 1 <= k_max bounds the accepted list
    int tries = 0, cnt = 0, acc = 0, rej_overlap = 0, rej_capacity = 0, rows = 0;
    if (applied) {
        for (int j = lane; j < na; j += kWave) {
            const float *bx = all_boxes + ((size_t)bs * a + j) * 7;
            s_cur[j] = make_rect(bx[0], bx[1], bx[2], bx[3], bx[4] + 0.5f, bx[5] + 0.5f, bx[6]);
        }
        __syncthreads();
        const double pa = road_plane[(size_t)bs * 4], pb = road_plane[(size_t)bs * 4 + 1], pc = road_plane[(size_t)bs * 4 + 2],
                     pd = road_plane[(size_t)bs * 4 + 3];
        int ncur = na;
        for (int t = 0; t < T; ++t) {              // every condition below is uniform over the wave
            if (cnt > extra) break;
            ++tries;
            const int d = cand[(size_t)bs * T + t];
            if (d < 0 || d >= D) continue;         // no such object: as a candidate out of range
            const float *bx = db_boxes + (size_t)d * 7;
            const float x = bx[0], y = bx[1], z = bx[2], h = bx[3], w = bx[4], l = bx[5], ry = bx[6];
            if (reduce_by_range &&
                !((double)x >= scope.v[0] && (double)x <= scope.v[1] && (double)y >= scope.v[2] && (double)y <= scope.v[3] &&
                  (double)z >= scope.v[4] && (double)z <= scope.v[5]))
                continue;
            const int npts = db_npts[d];
            if (npts < 5) continue;
            const double cur_height = ((-pd - pa * (double)x) - pc * (double)z) / pb;
            const double move = (double)y - cur_height;
            const float y_placed = (float)((double)y - move);
            ++cnt;
            const Rect mine = make_rect(x, y_placed, z, h, w + 0.5f, l + 0.5f, ry);
            bool hit = false;
            for (int j = lane; j < ncur; j += kWave) hit = hit || overlaps(mine, s_cur[j]);
            if (__ballot(hit) != 0ull) { ++rej_overlap; continue; }
            if (acc >= k_max || npts > e - rows) { ++rej_capacity; continue; }
            if (lane == 0) {
                s_cur[ncur] = mine;
                s_box[acc][0] = x; s_box[acc][1] = y_placed; s_box[acc][2] = z; s_box[acc][3] = h; s_box[acc][4] = w; s_box[acc][5] = l;
                s_box[acc][6] = ry; s_box[acc][7] = db_alpha[d];
                s_move[acc] = move; s_db[acc] = d; s_row0[acc] = rows;
            }
            __syncthreads();
            ++ncur; ++acc; rows += npts;
        }
    }
    __syncthreads();
    for (int k = lane; k < k_max; k += kWave) {
        const size_t at = (size_t)bs * k_max + k;
        const bool live = k < acc;
        o.acc_db[at] = live ? s_db[k] : -1;
        o.acc_move[at] = live ? s_move[k] : 0.0;
        o.acc_row0[at] = live ? s_row0[k] : 0;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const float v = live ? s_box[k][c] : 0.f;
            o.acc_box[at * 7 + c] = v;
            o.remove_boxes[at * 7 + c] = (c == 3 && live) ? v + 2.0f : v;
        }
    }
    const int out_rows = g + k_max;
    for (int r = lane; r < out_rows; r += kWave) {
        const size_t at = (size_t)bs * out_rows + r;
        const bool own = r < ng, added = !own && r - ng < acc;
        const float *src = gt_boxes + ((size_t)bs * g + (own ? r : 0)) * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c) o.gt_out[at * 7 + c] = own ? src[c] : (added ? s_box[r - ng][c] : 0.f);
        o.alpha_out[at] = own ? gt_alpha[(size_t)bs * g + r] : (added ? s_box[r - ng][7] : 0.f);
    }
    if (lane == 0) {
        int *info = o.info + (size_t)bs * 8;
        info[0] = applied; info[1] = extra_num[bs]; info[2] = tries; info[3] = cnt; info[4] = acc; info[5] = rej_overlap;
        info[6] = rej_capacity; info[7] = rows;
    }
}

// ---- points: grid (chunks of 256 extra rows, b)
template <bool VEC>
__global__ __launch_bounds__(kPointThreads) void points_kernel(int e, int k_max, int D, int S, const float *__restrict__ db_points,
                                                               const int *__restrict__ db_offsets, const int *__restrict__ acc_db,
                                                               const double *__restrict__ acc_move, const int *__restrict__ acc_row0,
                                                               const int *__restrict__ info, float *__restrict__ extra_pts) {
    __shared__ int s_row0[kMaxAccept + 1], s_src[kMaxAccept];
    __shared__ double s_move[kMaxAccept];
    int chunk, bs;
    xcd_scene_map(chunk, bs);
    const int t = threadIdx.x;
    const int acc = min(max(info[(size_t)bs * 8 + 4], 0), k_max), rows = min(max(info[(size_t)bs * 8 + 7], 0), e);
    if (t < acc) {
        const size_t at = (size_t)bs * k_max + t;
        const int d = min(max(acc_db[at], 0), D - 1);
        s_row0[t] = acc_row0[at];
        s_src[t] = db_offsets[d];
        s_move[t] = acc_move[at];
    }
    if (t == acc) s_row0[t] = rows;
    __syncthreads();
    const int r = chunk * kPointThreads + t;
    if (r >= e) return;
    float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
    if (r < rows && acc > 0) {
        int k = 0;
        while (k + 1 < acc && s_row0[k + 1] <= r) ++k;
        const size_t src = (size_t)min(max(s_src[k] + (r - s_row0[k]), 0), S - 1);   // never past the database
        if (VEC) {
            const f4 v = reinterpret_cast<const f4 *>(db_points)[src];
            x = v.x; y = v.y; z = v.z; w = v.w;
        } else {
            x = db_points[src * 4]; y = db_points[src * 4 + 1]; z = db_points[src * 4 + 2]; w = db_points[src * 4 + 3];
        }
        y = (float)((double)y - s_move[k]);
    }
    float *dst = extra_pts + ((size_t)bs * e + r) * 4;
    if (VEC) {
        const f4 v = {x, y, z, w};
        *reinterpret_cast<f4 *>(dst) = v;
    } else {
        dst[0] = x; dst[1] = y; dst[2] = z; dst[3] = w;
    }
}

}  // namespace gtaug
}  // namespace epnet

using namespace epnet;

static bool place_limits(int b, int T, int a, int g, int k_max, int e, int D, int extra_max) {
    return b <= 65535 && T >= 0 && T <= gtaug::kMaxTries && a >= 0 && a <= gtaug::kMaxExisting && g >= 0 && g <= 65536 && k_max >= 1 &&
           k_max <= gtaug::kMaxAccept && extra_max < k_max && e >= 0 && e <= 1048576 && D >= 1;
}

extern "C" int epnet_gt_aug_place(int b, int T, int a, int g, int k_max, int e, int D, int extra_max, int reduce_by_range,
                                  const double *scope, const float *db_boxes, const float *db_alpha, const int *db_npts,
                                  const int *apply, const int *extra_num, const int *cand, const float *all_boxes, const int *num_all,
                                  const float *gt_boxes, const float *gt_alpha, const int *num_gt, const double *road_plane,
                                  int *acc_db, float *acc_box, double *acc_move, int *acc_row0, float *remove_boxes, float *gt_out,
                                  float *alpha_out, int *info, epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0);
    if (b == 0) return EPNET_OK;
    if (!place_limits(b, T, a, g, k_max, e, D, extra_max)) return EPNET_ELIMIT;
    EPNET_REQUIRE(db_boxes && db_alpha && db_npts && apply && extra_num && (cand || T == 0) && num_all && num_gt && road_plane);
    EPNET_REQUIRE((all_boxes || a == 0) && ((gt_boxes && gt_alpha) || g == 0));
    EPNET_REQUIRE(acc_db && acc_box && acc_move && acc_row0 && remove_boxes && gt_out && alpha_out && info);
    EPNET_REQUIRE(scope || !reduce_by_range);
    gtaug::Scope sc;
    for (int k = 0; k < 6; ++k) sc.v[k] = scope ? scope[k] : 0.0;
    const gtaug::PlaceOut o = {acc_db, acc_box, acc_move, acc_row0, remove_boxes, gt_out, alpha_out, info};
    hipLaunchKernelGGL(gtaug::place_kernel, dim3((unsigned)b), dim3(kWave), 0, (hipStream_t)stream, T, a, g, k_max, e, D, reduce_by_range, sc,
                       db_boxes, db_alpha, db_npts, apply, extra_num, cand, all_boxes, num_all, gt_boxes, gt_alpha, num_gt, road_plane, o);
    return check_launch("gt_aug_place");
}

extern "C" int epnet_gt_aug_points(int b, int e, int k_max, int D, int S, const float *db_points, const int *db_offsets, const int *acc_db,
                                   const double *acc_move, const int *acc_row0, const int *info, float *extra_pts,
                                   epnet_stream_t stream) {
    EPNET_REQUIRE(b >= 0 && e >= 0);
    if (b == 0 || e == 0) return EPNET_OK;
    if (b > 65535 || e > 1048576 || k_max < 1 || k_max > gtaug::kMaxAccept || D < 1 || S < 1) return EPNET_ELIMIT;
    EPNET_REQUIRE(db_points && db_offsets && acc_db && acc_move && acc_row0 && info && extra_pts);
    const dim3 grid((unsigned)div_up(e, gtaug::kPointThreads), (unsigned)b), block(gtaug::kPointThreads);
    const bool vec = (((uintptr_t)db_points | (uintptr_t)extra_pts) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(gtaug::points_kernel<true>, grid, block, 0, (hipStream_t)stream, e, k_max, D, S, db_points, db_offsets, acc_db,
                           acc_move, acc_row0, info, extra_pts);
    else
        hipLaunchKernelGGL(gtaug::points_kernel<false>, grid, block, 0, (hipStream_t)stream, e, k_max, D, S, db_points, db_offsets, acc_db,
                           acc_move, acc_row0, info, extra_pts);
    return check_launch("gt_aug_points");
}
