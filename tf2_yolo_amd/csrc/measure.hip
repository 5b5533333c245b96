// Detection evaluation on the device: the arithmetic of the reference's utils/measurement.py (create_score_mat :16-150,
// PRfunc :153-337) after decode / NMS -- matching detections to ground truth by IoU, counting true positives, and the
// cumulative precision / recall curve. Everything is fp64 and integer work, bit-exact against the reference's own outputs
// (tests/golden/measurement_golden.npz). No floating-point atomics; integer atomics on counters, atomicMin on ranks and
// "set to 1" flag stores only, so the results do not depend on the order in which workgroups run.
//
// ONE pipeline, stated for a data set: rows of B images, image-major with offsets (what yolo_decode_batch_write and
// yolo_nms_batch_select store), and every class at once. The entry points for one image or one class run the same kernels
// with the offset and count tables left out (null pointers): the kernels then take the one segment [0, n) and the counts
// that the call passes by value.
//
//   match   per detection the best-IoU ground truth of ITS image and ITS class (np.argmax: first maximum, index inside the
//           class subset) and IoU >= threshold; per class #detections, #ground truths, #matched detections (TPP),
//           #distinct matched ground truths (TP: per image, summed)                               (measurement.py:104-138)
//   rank    rank of every row inside its segment by key, descending (np.argsort(...)[::-1]). A TOTAL order, so that the
//           ranks of a segment are a permutation of 0 .. m-1 whatever the keys: the order key of NaN is +inf
//           (desc_order_key, common.hpp: argsort()[::-1] visits NaN first); equal order keys -- ties, which numpy leaves to
//           its unstable sort, -0.0 and 0.0, two NaNs, NaN and +inf -- put the later row first
//   curve   per class: sort the detections by joint confidence (the order of rank: every slot of the sorted flags is
//           written exactly once), then for every prefix the number of matched detections and of DISTINCT matched ground
//           truths -> precision (3 modes) and recall, plus the closing (0, last recall) point      (measurement.py:299-323)
//
//   yolo_match_batch        match for B images. Also gid, the ground truth's id inside its class over the whole data set:
//                           best_gt + the class's ground truths in earlier images of this call + gts_seen[class]; gts_seen
//                           advances by the call's counts
//   yolo_match_detections   B = 1: no offsets (the image is [0, ngt) and [0, ndet)), no gid and no gts_seen; the caller's
//                           gt_flags are the flag bytes, and the ground-truth counts come from the pass over the flags
//   yolo_rank_desc_images   rank with segment = (image, class): a row is compared against the rows of its own image only,
//                           so the work is the sum of the images' n^2, not the batch's
//   yolo_rank_desc          one image [0, n); the segment ids take the place of the classes: any ints, compared for
//                           equality only
//   yolo_pr_curves          curve of every class in one call: count and scan the classes, stable partition by class, rank
//                           inside each class, first detection of every matched ground truth, and one workgroup per class
//                           for the running (tpp, tp) scan
//   yolo_pr_curve           one class: the rows are that class already (no partition), n and num_gts by value
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

// the segment b of [0, nseg) with off[b] <= i < off[b + 1] (off ascending, off[0] <= i; empty segments are passed over)
__device__ __forceinline__ int segment_of(const int* __restrict__ off, int nseg, int i) {
  int lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// exclusive prefix count of a predicate over a 1024-thread workgroup (16 waves); *total = the workgroup's count.
// Every thread calls it; s_w: 16 ints of LDS, free again on return.
__device__ __forceinline__ int block_prefix_count(bool p, int* s_w, int* total) {
  const unsigned long long m = __ballot(p);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int in_wave = __popcll(m & ((1ULL << lane) - 1ULL));
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int v = s_w[k];
    before += (k < w) ? v : 0;
    all += v;
  }
  __syncthreads();
  *total = all;
  return before + in_wave;
}

// ---- match ------------------------------------------------------------------------------------------------------------
// cnt[b * C + c] = ground truths of class c in image b
__global__ void mb_gt_count_kernel(const double* __restrict__ gt, int ngt, const int* __restrict__ gt_off, int B, int C,
                                   int* __restrict__ cnt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ngt) return;
  const int c = (int)gt[(long long)j * 7 + 5];
  if (c < 0 || c >= C) return;
  atomicAdd(&cnt[(size_t)segment_of(gt_off, B, j) * C + c], 1);
}

// one thread per class: pre[b * C + c] = gts_seen[c] + ground truths of class c in the images before b; then the class's
// ground-truth count and gts_seen[c] advance by the call's total
__global__ void mb_scan_kernel(const int* __restrict__ cnt, int B, int C, int* __restrict__ pre,
                               long long* __restrict__ gts_seen, long long* __restrict__ counts) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long long seen = gts_seen[c];
  long long run = 0;
  for (int b = 0; b < B; ++b) {
    const size_t s = (size_t)b * C + c;
    pre[s] = (int)(seen + run);
    run += cnt[s];
  }
  counts[c * 4 + 1] += run;
  gts_seen[c] = seen + run;
}

// one thread per detection, the ground truths of an image are few. A class id outside [0, C) is matched against its own
// id and counted nowhere. det_off / gt_off null: one image, [0, ndet) and [0, ngt); pre null: the ids start at 0; gid null:
// not wanted. flags: zero on entry.
__global__ __launch_bounds__(256) void mb_match_kernel(const double* __restrict__ gt, int ngt, const int* __restrict__ gt_off,
                                                     const double* __restrict__ det, int ndet,
                                                     const int* __restrict__ det_off, int B, int C, double thr,
                                                     const int* __restrict__ pre, int* __restrict__ best_gt,
                                                     unsigned char* __restrict__ matched, double* __restrict__ best_iou,
                                                     int* __restrict__ gid, unsigned char* __restrict__ flags,
                                                     long long* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ndet) return;
  const int b = det_off ? segment_of(det_off, B, i) : 0;
  int g0 = gt_off ? gt_off[b] : 0, g1 = gt_off ? gt_off[b + 1] : ngt;
  if (g0 < 0) g0 = 0;
  if (g1 > ngt) g1 = ngt;
  const double* d = det + (long long)i * 7;
  const int c = (int)d[5];
  double best = -1.0;
  int arg = 0, arg_row = 0, k = 0;
  for (int j = g0; j < g1; ++j) {
    const double* g = gt + (long long)j * 7;
    if ((int)g[5] != c) continue;
    const double v = iou_xywh(g, d);
    if (v > best) {   // strict: the first maximum wins, like np.argmax
      best = v;
      arg = k;
      arg_row = j;
    }
    ++k;
  }
  const bool in_range = c >= 0 && c < C;
  const bool hit = k > 0 && best >= thr;
  best_gt[i] = (k > 0) ? arg : 0;
  matched[i] = hit ? 1 : 0;
  best_iou[i] = (k > 0) ? best : 0.0;
  if (gid) gid[i] = (k > 0) ? arg + ((in_range && pre) ? pre[(size_t)b * C + c] : 0) : 0;
  if (!in_range) return;
  atomicAdd((unsigned long long*)&counts[c * 4 + 0], 1ULL);
  if (hit) {
    atomicAdd((unsigned long long*)&counts[c * 4 + 2], 1ULL);
    flags[arg_row] = 1;   // a ground-truth row belongs to one image: the distinct count is per image
  }
}

// the flagged ground truths per class; count_gts: and the ground truths per class, where no mb_scan_kernel counted them
__global__ void mb_distinct_kernel(const double* __restrict__ gt, int ngt, int C, const unsigned char* __restrict__ flags,
                                   bool count_gts, long long* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ngt) return;
  const bool hit = flags[j];
  if (!hit && !count_gts) return;
  const int c = (int)gt[(long long)j * 7 + 5];
  if (c < 0 || c >= C) return;
  if (count_gts) atomicAdd((unsigned long long*)&counts[c * 4 + 1], 1ULL);
  if (hit) atomicAdd((unsigned long long*)&counts[c * 4 + 3], 1ULL);
}

// ---- rank -------------------------------------------------------------------------------------------------------------
// One workgroup ranks 256 rows: it walks, in tiles of 256, the images (segments of `off`) its rows lie in, and a row counts
// the rows of its own image and class that come before it. cls: any ints, compared for equality only (no value is
// reserved: a tile's unused slots are never read); null: one class. off null: one image [0, n). Rows at or past off[nseg]
// get no rank.
__global__ __launch_bounds__(256) void rank_desc_images_kernel(const double* __restrict__ key, const int* __restrict__ cls,
                                                             int n, const int* __restrict__ off, int nseg,
                                                             int* __restrict__ rank) {
  __shared__ double s_key[256];
  __shared__ int s_cls[256];
  __shared__ int s_range[2];
  const int nn = (off && off[nseg] < n) ? off[nseg] : n;
  const int w0 = blockIdx.x * 256;
  if (w0 >= nn) return;   // (the whole workgroup)
  const int i = w0 + threadIdx.x;
  const bool valid = i < nn;
  int lo = 0, hi = nn;
  if (valid && off) {
    const int b = segment_of(off, nseg, i);
    lo = off[b] < 0 ? 0 : off[b];
    hi = off[b + 1] > nn ? nn : off[b + 1];
  }
  if (threadIdx.x == 0) s_range[0] = lo;
  if (i == ((w0 + 255 < nn - 1) ? w0 + 255 : nn - 1)) s_range[1] = hi;
  __syncthreads();
  const int r0 = s_range[0], r1 = s_range[1];
  const double ki = valid ? desc_order_key(key[i]) : 0.0;
  const int ci = valid ? (cls ? cls[i] : 0) : 0;
  int r = 0;
  for (int base = r0; base < r1; base += 256) {
    const int j = base + threadIdx.x;
    s_key[threadIdx.x] = (j < r1) ? desc_order_key(key[j]) : 0.0;   // (a key: no NaN, so == and > below are a total order)
    s_cls[threadIdx.x] = (j < r1) ? (cls ? cls[j] : 0) : 0;
    __syncthreads();
    const int lim = (r1 - base < 256) ? (r1 - base) : 256;
    for (int t = 0; t < lim; ++t) {
      const int j2 = base + t;
      const bool before = (s_key[t] > ki) || (s_key[t] == ki && j2 > i);
      r += (j2 >= lo && j2 < hi && s_cls[t] == ci && before) ? 1 : 0;
    }
    __syncthreads();
  }
  if (valid) rank[i] = r;
}

// ---- curve ------------------------------------------------------------------------------------------------------------
__global__ void prc_count_kernel(const int* __restrict__ cls, int n, int C, int* __restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = cls[i];
  if (c >= 0 && c < C) atomicAdd(&cnt[c], 1);
}

// cls_off = exclusive scan of the class counts, gt_base = exclusive scan of the ground-truth counts (one thread: C is small)
__global__ void prc_offsets_kernel(const int* __restrict__ cnt, const long long* __restrict__ gts, int C,
                                   int* __restrict__ cls_off, long long* __restrict__ gt_base) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int run = 0;
  long long grun = 0;
  for (int c = 0; c < C; ++c) {
    cls_off[c] = run;
    gt_base[c] = grun;
    run += cnt[c];
    grun += gts[c] > 0 ? gts[c] : 0;
  }
  cls_off[C] = run;
  gt_base[C] = grun;
}

// workgroup c walks all rows in chunks of 1024 and copies those of class c, in their order, to cls_off[c] ...
__global__ __launch_bounds__(1024) void prc_partition_kernel(const double* __restrict__ joint, const int* __restrict__ gid,
                                                           const unsigned char* __restrict__ matched,
                                                           const int* __restrict__ cls, int n,
                                                           const int* __restrict__ cls_off, double* __restrict__ pj,
                                                           int* __restrict__ pg, unsigned char* __restrict__ pm,
                                                           int* __restrict__ pc) {
  __shared__ int s_w[16];
  const int c = blockIdx.x;
  const int first = cls_off[c], n_c = cls_off[c + 1] - first;
  if (n_c <= 0) return;
  int run = 0;
  for (int base = 0; base < n && run < n_c; base += 1024) {   // (run and n_c are the same in every thread)
    const int i = base + threadIdx.x;
    const bool mine = i < n && cls[i] == c;
    int total;
    const int at = run + block_prefix_count(mine, s_w, &total);
    if (mine && at < n_c) {
      const int p = first + at;
      pj[p] = joint[i];
      pg[p] = gid[i];
      pm[p] = matched[i];
      pc[p] = c;
    }
    run += total;
  }
}

__global__ void prc_fill_kernel(int* p, long long n, int v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// Where the classes are. yolo_pr_curves: tables on the device -- the rows of class c are [cls_off[c], cls_off[c + 1]) with pc
// = c, it has gts[c] ground truths, and the slot of its ground truth g in `first` is gt_base[c] + g. yolo_pr_curve: cls_off
// null and ONE class by value -- n rows from 0, num_gts ground truths, slots from 0.
struct PrcClasses {
  const int *cls_off, *pc;
  const long long *gts, *gt_base;
  int n;
  long long num_gts;
};
struct PrcSpan {
  int first, n;
  long long gts, gt_base;
};
__device__ __forceinline__ PrcSpan prc_span(const PrcClasses& k, int c) {
  if (!k.cls_off) return {0, k.n, k.num_gts, 0};
  return {k.cls_off[c], k.cls_off[c + 1] - k.cls_off[c], k.gts[c], k.gt_base[c]};
}

// row p of the partitioned rows: false past the last row; else its class's first row and the slot in `first` of its ground
// truth (-1: not matched, or an id outside the class's ground truths). Ranks are inside the class.
__device__ __forceinline__ bool prc_row(const PrcClasses& k, int C, long long gts_total, const int* pg, const unsigned char* pm,
                                        int p, int* first_row, long long* slot) {
  if (p >= (k.cls_off ? k.cls_off[C] : k.n)) return false;
  const PrcSpan s = prc_span(k, k.cls_off ? k.pc[p] : 0);
  const long long g = pg[p], at = s.gt_base + g;
  *first_row = s.first;
  *slot = (pm[p] && g >= 0 && g < s.gts && at < gts_total) ? at : -1;
  return true;
}
// first[slot] = smallest rank among the MATCHED detections of that ground truth; sorted_flags bit 0: matched
__global__ void prc_first_kernel(const int* __restrict__ rank, const int* __restrict__ pg, const unsigned char* __restrict__ pm,
                                 PrcClasses k, int C, long long gts_total, int* __restrict__ first,
                                 unsigned char* __restrict__ sorted_flags) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  int first_row;
  long long s;
  if (!prc_row(k, C, gts_total, pg, pm, p, &first_row, &s)) return;
  const int r = rank[p];
  if (s >= 0) atomicMin(&first[s], r);
  sorted_flags[first_row + r] = pm[p] ? 1 : 0;
}
// sorted_flags bit 1: the first detection of its ground truth
__global__ void prc_mark_kernel(const int* __restrict__ rank, const int* __restrict__ pg, const unsigned char* __restrict__ pm,
                                PrcClasses k, int C, long long gts_total, const int* __restrict__ first,
                                unsigned char* __restrict__ sorted_flags) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  int first_row;
  long long s;
  if (!prc_row(k, C, gts_total, pg, pm, p, &first_row, &s)) return;
  const int r = rank[p];
  if (s >= 0 && first[s] == r) sorted_flags[first_row + r] |= 2;
}

// workgroup c walks class c's sorted flags in chunks of 1024 with a running (tpp, tp) pair; its n_c + 1 points start at
// first row + c. A class without detections or without ground truths is left to the caller: nothing is written (and nothing
// divided) there.
__global__ __launch_bounds__(1024) void prc_scan_kernel(const unsigned char* __restrict__ sorted_flags, PrcClasses k, int mode,
                                                      double* __restrict__ precision, double* __restrict__ recall) {
  __shared__ int s_w[16];
  const int c = blockIdx.x;
  const PrcSpan s = prc_span(k, c);
  const int n = s.n;
  const long long num_gts = s.gts;
  if (n <= 0 || num_gts <= 0) return;
  const unsigned char* flags = sorted_flags + s.first;
  double* prec = precision + s.first + c;
  double* rec = recall + s.first + c;
  int run_a = 0, run_b = 0;   // (tpp, tp) of the chunks before this one, the same in every thread
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const unsigned char f = (i < n) ? flags[i] : 0;
    int tot_a, tot_b;
    const int a = block_prefix_count(f & 1, s_w, &tot_a) + (f & 1);          // inclusive
    const int b = block_prefix_count((f >> 1) & 1, s_w, &tot_b) + ((f >> 1) & 1);
    if (i < n) {
      const long long tpp = run_a + a, tp = run_b + b;
      const long long dets = i + 1, fp = dets - tpp;
      double p;
      if (mode == 0) p = (double)tpp / (double)dets;
      else if (mode == 1) p = (double)tp / (double)(tp + fp);
      else p = (double)tp / (double)dets;
      prec[i] = p;
      rec[i] = (double)tp / (double)num_gts;
      if (i == n - 1) {
        prec[n] = 0.0;
        rec[n] = (double)tp / (double)num_gts;
      }
    }
    run_a += tot_a;
    run_b += tot_b;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the largest B * class_num / n / ground-truth total the int indices of the kernels above hold
static const long long MB_MAX_CELLS = 1LL << 28;
static const long long MB_MAX_ROWS = 1LL << 30;

static bool match_batch_sizes_ok(int ngt, int ndet, int B, int class_num) {
  return ngt >= 0 && ndet >= 0 && B > 0 && class_num > 0 && (long long)B * class_num <= MB_MAX_CELLS && ngt <= MB_MAX_ROWS &&
         ndet <= MB_MAX_ROWS;
}
static bool pr_curves_sizes_ok(int n, int class_num, long long gts_total) {
  return n >= 0 && n <= MB_MAX_ROWS && class_num > 0 && class_num <= MB_MAX_CELLS && gts_total >= 0 && gts_total <= MB_MAX_ROWS;
}

// the five launches from rows that lie class by class (k, C classes, gts_total slots in `first`) to the curves
static void curve_launches(hipStream_t st, const double* pj, const int* pg, const unsigned char* pm, int n, const PrcClasses& k,
                           int C, long long gts_total, int mode, int* rank, int* first, unsigned char* flags, double* precision,
                           double* recall) {
  hipLaunchKernelGGL(rank_desc_images_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pj, (const int*)nullptr, n, k.cls_off, C,
                     rank);
  if (gts_total > 0)
    hipLaunchKernelGGL(prc_fill_kernel, dim3((unsigned)((gts_total + 255) / 256)), dim3(256), 0, st, first, gts_total, 0x7fffffff);
  hipLaunchKernelGGL(prc_first_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rank, pg, pm, k, C, gts_total, first, flags);
  hipLaunchKernelGGL(prc_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rank, pg, pm, k, C, gts_total, first, flags);
  hipLaunchKernelGGL(prc_scan_kernel, dim3(C), dim3(1024), 0, st, flags, k, mode, precision, recall);
}

}  // namespace yolo

using namespace yolo;

extern "C" size_t yolo_match_batch_workspace_bytes(int ngt, int B, int class_num) {
  if (!match_batch_sizes_ok(ngt, 0, B, class_num)) return 256;
  return align256((size_t)2 * B * class_num * sizeof(int)) + align256((size_t)ngt) + 256;
}

extern "C" int yolo_match_batch(const double* gt_rows, int ngt, const int* gt_off, const double* det_rows, int ndet,
                                const int* det_off, int B, int class_num, double iou_threshold, long long* gts_seen,
                                int* best_gt, unsigned char* matched, double* best_iou, int* gid, long long* class_counts,
                                void* workspace, size_t workspace_bytes, void* stream) {
  YOLO_REQUIRE(match_batch_sizes_ok(ngt, ndet, B, class_num), "match_batch: bad sizes");
  YOLO_REQUIRE(gt_off && det_off && gts_seen && class_counts && workspace, "match_batch: null pointer");
  YOLO_REQUIRE(ndet == 0 || (det_rows && best_gt && matched && best_iou && gid), "match_batch: null detection buffers");
  YOLO_REQUIRE(ngt == 0 || gt_rows, "match_batch: null ground-truth rows");
  const size_t need = yolo_match_batch_workspace_bytes(ngt, B, class_num);
  if (workspace_bytes < need) {
    set_error("match_batch: workspace %zu < %zu", workspace_bytes, need);
    return YOLO_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const size_t cells = (size_t)B * class_num;
  int* cnt = reinterpret_cast<int*>(workspace);
  int* pre = cnt + cells;
  unsigned char* flags = reinterpret_cast<unsigned char*>(workspace) + align256(2 * cells * sizeof(int));
  if (hipMemsetAsync(cnt, 0, cells * sizeof(int), st) != hipSuccess ||
      (ngt > 0 && hipMemsetAsync(flags, 0, (size_t)ngt, st) != hipSuccess)) {
    set_error("match_batch: memset failed");
    return YOLO_ERR_LAUNCH;
  }
  if (ngt > 0)
    hipLaunchKernelGGL(mb_gt_count_kernel, dim3((ngt + 255) / 256), dim3(256), 0, st, gt_rows, ngt, gt_off, B, class_num, cnt);
  hipLaunchKernelGGL(mb_scan_kernel, dim3((class_num + 255) / 256), dim3(256), 0, st, cnt, B, class_num, pre, gts_seen,
                     class_counts);
  if (ndet > 0)
    hipLaunchKernelGGL(mb_match_kernel, dim3((ndet + 255) / 256), dim3(256), 0, st, gt_rows, ngt, gt_off, det_rows, ndet,
                       det_off, B, class_num, iou_threshold, pre, best_gt, matched, best_iou, gid, flags, class_counts);
  if (ngt > 0 && ndet > 0)
    hipLaunchKernelGGL(mb_distinct_kernel, dim3((ngt + 255) / 256), dim3(256), 0, st, gt_rows, ngt, class_num, flags, false,
                       class_counts);
  return check_launch("match_batch");
}

// B = 1 of yolo_match_batch without its tables: gt_flags (the caller's, uninitialised) are zeroed on the stream, and
// mb_distinct_kernel counts the ground truths too, so it runs whenever there are any
extern "C" int yolo_match_detections(const double* gt_rows, int ngt, const double* det_rows, int ndet, int class_num,
                                     double iou_threshold, int* best_gt, unsigned char* matched, double* best_iou,
                                     unsigned char* gt_flags, long long* class_counts, void* stream) {
  YOLO_REQUIRE(ngt >= 0 && ndet >= 0 && class_num > 0 && class_counts, "match_detections: bad args");
  YOLO_REQUIRE(ndet == 0 || (det_rows && best_gt && matched && best_iou), "match_detections: null detection buffers");
  YOLO_REQUIRE(ngt == 0 || (gt_rows && gt_flags), "match_detections: null ground-truth buffers");
  hipStream_t st = as_stream(stream);
  if (ngt > 0 && hipMemsetAsync(gt_flags, 0, (size_t)ngt, st) != hipSuccess) {
    set_error("match_detections: memset failed");
    return YOLO_ERR_LAUNCH;
  }
  if (ndet > 0)
    hipLaunchKernelGGL(mb_match_kernel, dim3((ndet + 255) / 256), dim3(256), 0, st, gt_rows, ngt, (const int*)nullptr, det_rows,
                       ndet, (const int*)nullptr, 1, class_num, iou_threshold, (const int*)nullptr, best_gt, matched, best_iou,
                       (int*)nullptr, gt_flags, class_counts);
  if (ngt > 0)
    hipLaunchKernelGGL(mb_distinct_kernel, dim3((ngt + 255) / 256), dim3(256), 0, st, gt_rows, ngt, class_num, gt_flags, true,
                       class_counts);
  return check_launch("match_detections");
}

extern "C" int yolo_rank_desc_images(const double* key, const int* cls, int n, const int* img_off, int B, int* rank,
                                     void* stream) {
  YOLO_REQUIRE(n >= 0 && n <= MB_MAX_ROWS && B > 0, "rank_desc_images: bad sizes");
  if (n == 0) return YOLO_OK;
  YOLO_REQUIRE(key && img_off && rank, "rank_desc_images: null pointer");
  hipLaunchKernelGGL(rank_desc_images_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), key, cls, n, img_off, B,
                     rank);
  return check_launch("rank_desc_images");
}

// one image [0, n) without an offset table; the segment ids are the kernel's class ids
extern "C" int yolo_rank_desc(const double* key, const int* segment, int n, int* rank, void* stream) {
  YOLO_REQUIRE(n >= 0, "rank_desc: bad args");
  if (n == 0) return YOLO_OK;
  YOLO_REQUIRE(key && rank, "rank_desc: null pointer");
  hipLaunchKernelGGL(rank_desc_images_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), key, segment, n,
                     (const int*)nullptr, 1, rank);
  return check_launch("rank_desc");
}

namespace {
struct PrcWs {
  double* pj;
  long long* gt_base;
  int *cnt, *rank, *pg, *pc, *first;
  unsigned char *pm, *flags;
};
size_t prc_carve(int n, int class_num, long long gts_total, void* base, PrcWs* ws) {
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += align256(bytes);
    return reinterpret_cast<unsigned char*>(base) + here;
  };
  unsigned char* pj = take((size_t)n * sizeof(double));
  unsigned char* gt_base = take(((size_t)class_num + 1) * sizeof(long long));
  unsigned char* cnt = take((size_t)class_num * sizeof(int));
  unsigned char* rank = take((size_t)n * sizeof(int));
  unsigned char* pg = take((size_t)n * sizeof(int));
  unsigned char* pc = take((size_t)n * sizeof(int));
  unsigned char* first = take((size_t)gts_total * sizeof(int));
  unsigned char* pm = take((size_t)n);
  unsigned char* flags = take((size_t)n);
  if (ws) {
    ws->pj = reinterpret_cast<double*>(pj);
    ws->gt_base = reinterpret_cast<long long*>(gt_base);
    ws->cnt = reinterpret_cast<int*>(cnt);
    ws->rank = reinterpret_cast<int*>(rank);
    ws->pg = reinterpret_cast<int*>(pg);
    ws->pc = reinterpret_cast<int*>(pc);
    ws->first = reinterpret_cast<int*>(first);
    ws->pm = pm;
    ws->flags = flags;
  }
  return at + 256;
}
}  // namespace

extern "C" size_t yolo_pr_curves_workspace_bytes(int n, int class_num, long long gts_total) {
  if (!pr_curves_sizes_ok(n, class_num, gts_total)) return 256;
  return prc_carve(n, class_num, gts_total, nullptr, nullptr);
}

extern "C" int yolo_pr_curves(const double* joint, const int* gid, const unsigned char* matched, const int* cls, int n,
                              const long long* gts, int class_num, long long gts_total, int precision_mode, void* workspace,
                              size_t workspace_bytes, int* cls_off, double* precision, double* recall, void* stream) {
  YOLO_REQUIRE(pr_curves_sizes_ok(n, class_num, gts_total), "pr_curves: bad sizes");
  YOLO_REQUIRE(precision_mode >= 0 && precision_mode <= 2, "pr_curves: bad precision mode %d", precision_mode);
  YOLO_REQUIRE(gts && cls_off && workspace, "pr_curves: null pointer");
  YOLO_REQUIRE(n == 0 || (joint && gid && matched && cls && precision && recall), "pr_curves: null pointer");
  PrcWs ws;
  const size_t need = prc_carve(n, class_num, gts_total, workspace, &ws);
  if (workspace_bytes < need) {
    set_error("pr_curves: workspace %zu < %zu", workspace_bytes, need);
    return YOLO_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    if (hipMemsetAsync(cls_off, 0, sizeof(int) * ((size_t)class_num + 1), st) != hipSuccess) return YOLO_ERR_LAUNCH;
    return YOLO_OK;
  }
  if (hipMemsetAsync(ws.cnt, 0, sizeof(int) * (size_t)class_num, st) != hipSuccess) {
    set_error("pr_curves: memset failed");
    return YOLO_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(prc_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cls, n, class_num, ws.cnt);
  hipLaunchKernelGGL(prc_offsets_kernel, dim3(1), dim3(64), 0, st, ws.cnt, gts, class_num, cls_off, ws.gt_base);
  hipLaunchKernelGGL(prc_partition_kernel, dim3(class_num), dim3(1024), 0, st, joint, gid, matched, cls, n, cls_off, ws.pj,
                     ws.pg, ws.pm, ws.pc);
  const PrcClasses k = {cls_off, ws.pc, gts, ws.gt_base, 0, 0};
  curve_launches(st, ws.pj, ws.pg, ws.pm, n, k, class_num, gts_total, precision_mode, ws.rank, ws.first, ws.flags, precision,
                 recall);
  return check_launch("pr_curves");
}

extern "C" size_t yolo_pr_curve_workspace_bytes(int n, int num_gts) {
  if (n < 0) n = 0;
  if (num_gts < 0) num_gts = 0;
  return (size_t)(n + num_gts + 2) * sizeof(int) + (size_t)n + 256;
}

// one class of yolo_pr_curves without its tables: the caller's rows are the partitioned rows
extern "C" int yolo_pr_curve(const double* joint, const int* gt_id, const unsigned char* matched, int n, int num_gts,
                             int precision_mode, void* workspace, size_t workspace_bytes, double* precision,
                             double* recall, void* stream) {
  YOLO_REQUIRE(n > 0 && num_gts > 0, "pr_curve: needs at least one detection and one ground truth");
  YOLO_REQUIRE(joint && gt_id && matched && workspace && precision && recall, "pr_curve: null pointer");
  YOLO_REQUIRE(precision_mode >= 0 && precision_mode <= 2, "pr_curve: bad precision mode %d", precision_mode);
  YOLO_REQUIRE(workspace_bytes >= yolo_pr_curve_workspace_bytes(n, num_gts), "pr_curve: workspace too small");
  int* rank = reinterpret_cast<int*>(workspace);
  int* first = rank + n;
  unsigned char* flags = reinterpret_cast<unsigned char*>(first + num_gts + 2);
  const PrcClasses k = {nullptr, nullptr, nullptr, nullptr, n, num_gts};
  curve_launches(as_stream(stream), joint, gt_id, matched, n, k, 1, num_gts, precision_mode, rank, first, flags, precision,
                 recall);
  return check_launch("pr_curve");
}
