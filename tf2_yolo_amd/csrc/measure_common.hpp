// Device helpers shared by the evaluation kernels: measure.hip (one image, one class) and measure_batch.hip (a batch of
// images, every class). The order of the rank and curve kernels is desc_order_key's (common.hpp).
#pragma once
#include "common.hpp"

namespace yolo {

// utils/tools.py:630-684 (mode 1) in fp64; a = ground truth, b = prediction
__device__ __forceinline__ double iou_xywh(const double* a, const double* b) {
  const double ahx = a[2] / 2., ahy = a[3] / 2., bhx = b[2] / 2., bhy = b[3] / 2.;
  const double aminx = a[0] - ahx, amaxx = a[0] + ahx, aminy = a[1] - ahy, amaxy = a[1] + ahy;
  const double bminx = b[0] - bhx, bmaxx = b[0] + bhx, bminy = b[1] - bhy, bmaxy = b[1] + bhy;
  const double iw = fmax(fmin(bmaxx, amaxx) - fmax(bminx, aminx), 0.);
  const double ih = fmax(fmin(bmaxy, amaxy) - fmax(bminy, aminy), 0.);
  const double inter = iw * ih;
  const double uni = b[2] * b[3] + a[2] * a[3] - inter;
  return inter / (uni + 1e-07);
}

}  // namespace yolo
