// nms.h -- the batched NMS launcher of iou3d.hip and the sizes of the workspace parts it needs.
#pragma once
#include "boxgeom.h"

namespace epnet {

// mask words per row of the suppression bit-mask of `cap` boxes
inline size_t nms_mask_words(size_t cap) { return (cap + 63) / 64; }

// `groups` NMS problems of at most `cap` boxes each (boxes: (groups, cap, 5) BEV rows), the group sizes read from device memory
// (counts[group], clamped to cap); counts == NULL: one group of exactly cap boxes.
// rot: groups * cap BoxRot (rotated only); mask: groups * cap * nms_mask_words(cap) words; keep: (groups, cap); num_keep: (groups).
int nms_groups(bool rotated, int groups, int cap, const int *counts, const float *boxes, float thresh, BoxRot *rot,
               unsigned long long *mask, long long *keep, int *num_keep, hipStream_t s);

}  // namespace epnet
