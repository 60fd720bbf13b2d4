// r4.h -- the value a float has after printf("%.4f") and strtod, without the text, host and device.
//
// save_kitti_format (tools/eval_rcnn.py:98-101) prints every number of a result line with %.4f and the evaluator parses the
// file again. For a float v: (double)v * 1e4 is exact -- a 24-bit significand times 10000 = 2^4 * 625 has at most 34
// significant bits -- so rint() in the default round-to-nearest-even mode picks the integer printf's exact decimal rounding
// picks, and the IEEE quotient of the two exact doubles is the double nearest to the printed decimal, which is what strtod
// returns. Non-finite values pass through; a small negative value gives -0.0, as "-0.0000" parses.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EPNET_R4_HD __host__ __device__ __forceinline__
#else
#define EPNET_R4_HD inline
#endif

namespace epnet {

EPNET_R4_HD double r4(float v) { return rint((double)v * 1e4) / 1e4; }

}  // namespace epnet
