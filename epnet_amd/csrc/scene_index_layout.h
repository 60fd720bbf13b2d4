// scene_index_layout.h -- sizes of the scene index and of the cell sort, free of HIP: what the host-side launch plans
// (fps_plan.h) share with the kernels of spatial.h.
#pragma once
#include <stddef.h>

namespace epnet {

// cells of the counting sort by grid cell (spatial.h, "cell sort")
constexpr int kCellBits = 14;
constexpr int kCells = 1 << kCellBits;

// ---- scene index: caller scratch shared by FPS, ball query and three_nn of one level ---------------------
// per scene: the points counting-sorted by cell as float4 (x, y, z, original index; padding = 3e38 / -1),
// padded to np = a power of two >= 2048, followed (after all scenes) by one box (6 floats) per 64 sorted points
// ("bucket") and then one box per 256 sorted points ("quad")
inline int scene_index_np(int n) {
    int np = 2048;
    while (np < n) np <<= 1;
    return np;
}
// scenes beyond 16384 points: np floats more per scene at the end -- scratch of the sampling kernel (its running distances
// in sorted order); nothing else reads or writes that tail
inline size_t scene_index_bytes(int b, int n) {
    if (b <= 0 || n < 1024 || n > 65536) return 0;
    const size_t np = (size_t)scene_index_np(n);
    return (size_t)b * (np * 16 + (np / 64 + np / 256) * 6 * sizeof(float) + (n > 16384 ? np * sizeof(float) : 0));
}

}  // namespace epnet
