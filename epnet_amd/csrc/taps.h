// taps.h -- bilinear taps of grid_sample (bilinear, zeros padding) shared by the sampler and its gradients (sample.hip, det.hip).
#pragma once
#include "common.h"

namespace epnet {

struct Taps {
    int x0, y0;            // north-west corner
    float nw, ne, sw, se;  // bilinear weights
};

__device__ __forceinline__ Taps taps_of(float x, float y, int h, int w, int align_corners) {
    float ix, iy;
    if (align_corners) {
        ix = ((x + 1.f) / 2.f) * (float)(w - 1);
        iy = ((y + 1.f) / 2.f) * (float)(h - 1);
    } else {
        ix = ((x + 1.f) * (float)w - 1.f) / 2.f;
        iy = ((y + 1.f) * (float)h - 1.f) / 2.f;
    }
    float fx = floorf(ix), fy = floorf(iy);
    // a tap can only be inside the map for -1 <= floor <= size - 1; anything else (far outside, infinite, NaN) is moved to
    // a corner that has no in-bounds tap, so that the int conversion below is always defined
    if (!(fx >= -1.f && fx <= (float)(w - 1) && fy >= -1.f && fy <= (float)(h - 1))) {
        fx = -2.f;
        fy = -2.f;
        ix = -2.f;
        iy = -2.f;
    }
    Taps t;
    t.x0 = (int)fx;
    t.y0 = (int)fy;
    const float x_e = fx + 1.f, y_s = fy + 1.f;
    t.nw = (x_e - ix) * (y_s - iy);
    t.ne = (ix - fx) * (y_s - iy);
    t.sw = (x_e - ix) * (iy - fy);
    t.se = (ix - fx) * (iy - fy);
    return t;
}

__device__ __forceinline__ bool inside(int x, int y, int h, int w) { return x >= 0 && y >= 0 && x < w && y < h; }

}  // namespace epnet
