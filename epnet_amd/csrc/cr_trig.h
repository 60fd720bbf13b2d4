// cr_trig.h -- the trigonometry of record (DESIGN.md "Parity definition"): correctly rounded float cos / sin / atan2 via the
// double-precision functions, the same definition the oracle uses. Host and device; every kernel and host op that rotates a
// box or takes a viewing angle calls these, so the definition has one place.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EPNET_HD __host__ __device__ __forceinline__
#else
#define EPNET_HD inline
#endif

namespace epnet {

EPNET_HD float cr_cosf(float x) { return (float)cos((double)x); }
EPNET_HD float cr_sinf(float x) { return (float)sin((double)x); }
// cos and sin of ONE angle, in one body: the two share their argument reduction, as they do when written out side by side
EPNET_HD void cr_cossinf(float x, float &c, float &s) {
    c = (float)cos((double)x);
    s = (float)sin((double)x);
}
EPNET_HD float cr_atan2f(float y, float x) { return (float)atan2((double)y, (double)x); }

}  // namespace epnet
