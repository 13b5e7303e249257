// bbox_iou in the reference's operation order, shared by nms.hip (write_results, rtod_bbox_iou) and match.hip (the validator).
// Both files are compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: one rounding per operation.
#pragma once
#include "rtod_internal.h"

namespace rtod {

__device__ __forceinline__ float iou_ref(const f32x4 a, const f32x4 b) {
    // bbox_iou, src/util.py:138-151 — same operation order, fp32, one rounding per op
    const float ix1 = fmaxf(a[0], b[0]), iy1 = fmaxf(a[1], b[1]);
    const float ix2 = fminf(a[2], b[2]), iy2 = fminf(a[3], b[3]);
    const float iw = fmaxf((ix2 - ix1) + 1.0f, 0.0f);
    const float ih = fmaxf((iy2 - iy1) + 1.0f, 0.0f);
    const float inter = iw * ih;
    const float a1 = ((a[2] - a[0]) + 1.0f) * ((a[3] - a[1]) + 1.0f);
    const float a2 = ((b[2] - b[0]) + 1.0f) * ((b[3] - b[1]) + 1.0f);
    return inter / ((a1 + a2) - inter);
}

}  // namespace rtod
