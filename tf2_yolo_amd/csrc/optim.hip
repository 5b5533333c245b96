// Optimizer kernels beyond the two in elementwise.hip: deterministic gradient norms, clip factors, and the update kernels of
// Adam (AMSGrad, clipping) and of SGD (momentum, Nesterov, clipping) that read every step-dependent scalar from device memory.
//
// All of them walk the flat buffers through one CHUNK TABLE built on the host (optimizers.build_chunk_table): chunk c covers
// elements [chunk_off[c], chunk_off[c] + chunk_len[c]) of variable chunk_var[c]; chunks never straddle two variables, never
// touch the padding between them, and the chunks of variable v are the consecutive indices [var_first[v], var_first[v + 1]).
// One workgroup per chunk: the work of a workgroup is a property of the table, not of the grid or of the clock.
//
// hyper (device float[8], refreshed by the host before every step):
//   [0] lr (Adam: the bias-corrected rate of the step)  [1] beta1  [2] beta2  [3] eps  [4] grad_scale  [5] momentum
//   [6] clip threshold (clipnorm / global_clipnorm / clipvalue)  [7] unused
#include <cmath>
#include "common.hpp"

// No implicit fused multiply-adds in this file: where a product and a sum are fused is written out (fmaf), so that the
// rounding of an update does not depend on what else the compiler finds around it. adam_update below spells the sequence
// the compiler makes of adam_kernel's expressions (elementwise.hip), which is what lets a clip factor of exactly 1 leave
// every bit as yolo_adam_step_dev would (tests/test_gpu_optim_kernels.py holds the two kernels against each other).
#pragma clang fp contract(off)

namespace yolo {

constexpr int OPT_THREADS = 256;
enum { CLIP_NONE = 0, CLIP_NORM = 1, CLIP_GLOBAL = 2, CLIP_VALUE = 3 };

// ---- stage 1: one workgroup per chunk -> one double. Products of floats are exact in double; the order of the additions is
// fixed by (thread index, wave tree, wave index), so a chunk's partial has one value whatever else runs.
__global__ __launch_bounds__(OPT_THREADS) void sqnorm_chunk_kernel(const float* __restrict__ g,
                                                                   const long long* __restrict__ chunk_off,
                                                                   const int* __restrict__ chunk_len,
                                                                   double* __restrict__ partial) {
  const long long off = chunk_off[blockIdx.x];
  const int len = chunk_len[blockIdx.x];
  const float* gc = g + off;
  const int n4 = (off & 3) == 0 ? len >> 2 : 0;   // (anchor boxes sit at offsets 2k: no 16-byte loads there)
  double s = 0.0;
  for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
    const f32x4 x = reinterpret_cast<const f32x4*>(gc)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)x[e] * (double)x[e];
  }
  for (int i = (n4 << 2) + threadIdx.x; i < len; i += OPT_THREADS) s += (double)gc[i] * (double)gc[i];
  s = wave_reduce_sum(s);
  __shared__ double wave_sum[OPT_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wave_sum[0];
#pragma unroll
    for (int w = 1; w < OPT_THREADS / 64; ++w) t += wave_sum[w];
    partial[blockIdx.x] = t;
  }
}

// x[first .. last) summed strictly in index order by one wave: 64 coalesced loads, then 64 additions in lane order (every lane
// computes the same sum). Lanes past the end add +0.0, which changes no sum of squares.
__device__ __forceinline__ double ordered_sum(const double* __restrict__ x, int first, int last) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int base = first; base < last; base += 64) {
    const double mine = base + lane < last ? x[base + lane] : 0.0;
#pragma unroll
    for (int l = 0; l < 64; ++l) s += __shfl(mine, l, 64);
  }
  return s;
}

// ---- stage 2: ONE workgroup. Wave w sums the partials of variables w, w + waves, ... in index order; then wave 0 sums the
// variables in order. (A few hundred variables, at most ~10^4 partials: a second launch for the last sum would cost more
// than it computes.)
constexpr int SUM_THREADS = 1024;
__global__ __launch_bounds__(SUM_THREADS) void sqnorm_sum_kernel(const double* __restrict__ partial,
                                                                 const int* __restrict__ var_first, int n_vars,
                                                                 double* __restrict__ var_sq, double* __restrict__ total_sq) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int v = wave; v < n_vars; v += SUM_THREADS / 64) {
    const double s = ordered_sum(partial, var_first[v], var_first[v + 1]);
    if (lane == 0) var_sq[v] = s;
  }
  __syncthreads();   // (var_sq was written by this workgroup: visible to it after the barrier)
  if (wave == 0) {
    const double t = ordered_sum(var_sq, 0, n_vars);
    if (lane == 0) *total_sq = t;
  }
}

// ---- clip factors: c = threshold / max(||gs * g||, threshold) in double, rounded once; exactly 1 at or below the threshold
__global__ void clip_factors_kernel(const double* __restrict__ var_sq, int n_vars, const double* __restrict__ total_a,
                                    const double* __restrict__ total_b, const float* __restrict__ hyper, int mode,
                                    float* __restrict__ factors, float* __restrict__ norm_out) {
  const double gs = fabs((double)hyper[4]);
  const double thr = (double)hyper[6];
  const double total = total_b != nullptr ? *total_a + *total_b : *total_a;   // parameters first, then anchors
  const double gnorm = gs * sqrt(total);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && norm_out != nullptr) *norm_out = (float)gnorm;
  if (mode == CLIP_GLOBAL) {
    if (i == 0) factors[0] = (float)(thr / fmax(gnorm, thr));
  } else if (i < n_vars) {
    factors[i] = (float)(thr / fmax(gs * sqrt(var_sq[i]), thr));
  }
}

// the gradient an update sees: (g * gs) * c, or clamp(g * gs, -t, +t)
struct ClipArgs {
  float gs, c, t;
  int value;
};
__device__ __forceinline__ float clipped(float g, const ClipArgs& k) {
  const float x = g * k.gs;
  return k.value ? fminf(fmaxf(x, -k.t), k.t) : x * k.c;
}
__device__ __forceinline__ ClipArgs clip_args(const float* __restrict__ hyper, const float* __restrict__ factors, int mode,
                                              int var) {
  ClipArgs k;
  k.gs = hyper[4];
  k.t = hyper[6];
  k.value = mode == CLIP_VALUE;
  k.c = mode == CLIP_NORM ? factors[var] : mode == CLIP_GLOBAL ? factors[0] : 1.f;
  return k;
}

// ---- Adam (optionally AMSGrad): the arithmetic of adam_kernel (elementwise.hip) on the clipped gradient
struct AdamArgs {
  float lr_t, b1, b2, eps;
};
template <bool AMSGRAD>
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float& vhat, float gg, const AdamArgs& h) {
  m = fmaf(h.b1, m, (1.f - h.b1) * gg);
  v = fmaf(h.b2, v, ((1.f - h.b2) * gg) * gg);
  if (AMSGRAD) {
    vhat = fmaxf(vhat, v);
    p -= (h.lr_t * m) / (sqrtf(vhat) + h.eps);
  } else {
    p -= (h.lr_t * m) / (sqrtf(v) + h.eps);
  }
}

template <bool AMSGRAD>
__global__ __launch_bounds__(OPT_THREADS) void adam_clip_kernel(float* __restrict__ p, float* __restrict__ g,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                float* __restrict__ vhat,
                                                                const long long* __restrict__ chunk_off,
                                                                const int* __restrict__ chunk_len,
                                                                const int* __restrict__ chunk_var,
                                                                const float* __restrict__ hyper,
                                                                const float* __restrict__ factors, int mode, int zero) {
  const long long off = chunk_off[blockIdx.x];
  const int len = chunk_len[blockIdx.x];
  const ClipArgs k = clip_args(hyper, factors, mode, chunk_var[blockIdx.x]);
  const AdamArgs h = {hyper[0], hyper[1], hyper[2], hyper[3]};
  const int n4 = (off & 3) == 0 ? len >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
    f32x4 pv = reinterpret_cast<f32x4*>(p + off)[i];
    f32x4 gv = reinterpret_cast<f32x4*>(g + off)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m + off)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v + off)[i];
    f32x4 hv = {0.f, 0.f, 0.f, 0.f};
    if (AMSGRAD) hv = reinterpret_cast<f32x4*>(vhat + off)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pp = pv[e], mm = mv[e], v1 = vv[e], hh = hv[e];   // (a vector element cannot bind to a reference)
      adam_update<AMSGRAD>(pp, mm, v1, hh, clipped(gv[e], k), h);
      pv[e] = pp;
      mv[e] = mm;
      vv[e] = v1;
      hv[e] = hh;
    }
    reinterpret_cast<f32x4*>(p + off)[i] = pv;
    reinterpret_cast<f32x4*>(m + off)[i] = mv;
    reinterpret_cast<f32x4*>(v + off)[i] = vv;
    if (AMSGRAD) reinterpret_cast<f32x4*>(vhat + off)[i] = hv;
    if (zero) reinterpret_cast<f32x4*>(g + off)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long long i = off + (n4 << 2) + threadIdx.x; i < off + len; i += OPT_THREADS) {
    float pp = p[i], mm = m[i], vv = v[i], hh = AMSGRAD ? vhat[i] : 0.f;
    adam_update<AMSGRAD>(pp, mm, vv, hh, clipped(g[i], k), h);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
    if (AMSGRAD) vhat[i] = hh;
    if (zero) g[i] = 0.f;
  }
}

// ---- SGD. KIND 0: p -= lr * gg (no accumulator). 1: a = mu * a - lr * gg; p += a. 2 (Nesterov): p += mu * a - lr * gg.
// (Keras ResourceApplyKerasMomentum.)
template <int KIND>
__device__ __forceinline__ void sgd_update(float& p, float& a, float gg, float lr, float mu) {
  if (KIND == 0) {
    p = fmaf(-lr, gg, p);     // (sgd_kernel's p -= (lr * gs) * g, fused the same way)
  } else {
    const float step = lr * gg;
    a = fmaf(mu, a, -step);
    if (KIND == 1) p += a;
    else p += fmaf(mu, a, -step);
  }
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void sgd_clip_kernel(float* __restrict__ p, float* __restrict__ g,
                                                               float* __restrict__ a,
                                                               const long long* __restrict__ chunk_off,
                                                               const int* __restrict__ chunk_len,
                                                               const int* __restrict__ chunk_var,
                                                               const float* __restrict__ hyper,
                                                               const float* __restrict__ factors, int mode, int zero) {
  const long long off = chunk_off[blockIdx.x];
  const int len = chunk_len[blockIdx.x];
  const ClipArgs k = clip_args(hyper, factors, mode, chunk_var[blockIdx.x]);
  const float lr = hyper[0], mu = hyper[5];
  const int n4 = (off & 3) == 0 ? len >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
    f32x4 pv = reinterpret_cast<f32x4*>(p + off)[i];
    f32x4 gv = reinterpret_cast<f32x4*>(g + off)[i];
    f32x4 av = {0.f, 0.f, 0.f, 0.f};
    if (KIND != 0) av = reinterpret_cast<f32x4*>(a + off)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pp = pv[e], aa = av[e];   // (a vector element cannot bind to a reference)
      sgd_update<KIND>(pp, aa, clipped(gv[e], k), lr, mu);
      pv[e] = pp;
      av[e] = aa;
    }
    reinterpret_cast<f32x4*>(p + off)[i] = pv;
    if (KIND != 0) reinterpret_cast<f32x4*>(a + off)[i] = av;
    if (zero) reinterpret_cast<f32x4*>(g + off)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (long long i = off + (n4 << 2) + threadIdx.x; i < off + len; i += OPT_THREADS) {
    float pp = p[i], aa = KIND != 0 ? a[i] : 0.f;
    sgd_update<KIND>(pp, aa, clipped(g[i], k), lr, mu);
    p[i] = pp;
    if (KIND != 0) a[i] = aa;
    if (zero) g[i] = 0.f;
  }
}

static bool clip_mode_ok(int mode, const float* factors) {
  return mode >= CLIP_NONE && mode <= CLIP_VALUE && ((mode != CLIP_NORM && mode != CLIP_GLOBAL) || factors != nullptr);
}

}  // namespace yolo

using namespace yolo;

extern "C" size_t yolo_grad_sqnorm_workspace_bytes(int n_chunks) {
  return sizeof(double) * (size_t)(n_chunks > 0 ? n_chunks : 1);
}

extern "C" int yolo_grad_sqnorm(const float* g, const long long* chunk_off, const int* chunk_len, int n_chunks,
                                const int* var_first, int n_vars, double* var_sq, double* total_sq, void* workspace,
                                size_t workspace_bytes, void* stream) {
  YOLO_REQUIRE(g && chunk_off && chunk_len && var_first && var_sq && total_sq && n_chunks > 0 && n_vars > 0,
               "grad_sqnorm: bad args");
  YOLO_REQUIRE(workspace && workspace_bytes >= yolo_grad_sqnorm_workspace_bytes(n_chunks),
               "grad_sqnorm: workspace of %zu bytes, need %zu", workspace_bytes, yolo_grad_sqnorm_workspace_bytes(n_chunks));
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(sqnorm_chunk_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, as_stream(stream), g, chunk_off, chunk_len,
                     partial);
  if (int rc = check_launch("sqnorm_chunk_kernel")) return rc;
  hipLaunchKernelGGL(sqnorm_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, as_stream(stream), partial, var_first, n_vars, var_sq,
                     total_sq);
  return check_launch("sqnorm_sum_kernel");
}

extern "C" int yolo_clip_factors(const double* var_sq, int n_vars, const double* total_sq, const double* total_sq_extra,
                                 const float* hyper, int mode, float* factors, float* norm_out, void* stream) {
  YOLO_REQUIRE(var_sq && total_sq && hyper && factors && n_vars > 0 && (mode == CLIP_NORM || mode == CLIP_GLOBAL),
               "clip_factors: bad args");
  const int threads = 256;
  const int blocks = mode == CLIP_GLOBAL ? 1 : (n_vars + threads - 1) / threads;
  hipLaunchKernelGGL(clip_factors_kernel, dim3(blocks), dim3(threads), 0, as_stream(stream), var_sq, n_vars, total_sq,
                     total_sq_extra, hyper, mode, factors, norm_out);
  return check_launch("clip_factors_kernel");
}

extern "C" int yolo_adam_step_clip(float* p, float* g, float* m, float* v, float* vhat, const long long* chunk_off,
                                   const int* chunk_len, const int* chunk_var, int n_chunks, const float* hyper,
                                   const float* factors, int clip_mode, int zero_grad, void* stream) {
  YOLO_REQUIRE(p && g && m && v && chunk_off && chunk_len && chunk_var && hyper && n_chunks > 0 &&
                   clip_mode_ok(clip_mode, factors),
               "adam_step_clip: bad args");
  if (vhat != nullptr)
    hipLaunchKernelGGL(adam_clip_kernel<true>, dim3(n_chunks), dim3(OPT_THREADS), 0, as_stream(stream), p, g, m, v, vhat,
                       chunk_off, chunk_len, chunk_var, hyper, factors, clip_mode, zero_grad);
  else
    hipLaunchKernelGGL(adam_clip_kernel<false>, dim3(n_chunks), dim3(OPT_THREADS), 0, as_stream(stream), p, g, m, v, vhat,
                       chunk_off, chunk_len, chunk_var, hyper, factors, clip_mode, zero_grad);
  return check_launch("adam_clip_kernel");
}

extern "C" int yolo_sgd_step_clip(float* p, float* g, float* accum, int nesterov, const long long* chunk_off,
                                  const int* chunk_len, const int* chunk_var, int n_chunks, const float* hyper,
                                  const float* factors, int clip_mode, int zero_grad, void* stream) {
  YOLO_REQUIRE(p && g && chunk_off && chunk_len && chunk_var && hyper && n_chunks > 0 && clip_mode_ok(clip_mode, factors) &&
                   (accum != nullptr || !nesterov),
               "sgd_step_clip: bad args");
  const dim3 grid(n_chunks), block(OPT_THREADS);
  if (accum == nullptr)
    hipLaunchKernelGGL(sgd_clip_kernel<0>, grid, block, 0, as_stream(stream), p, g, accum, chunk_off, chunk_len, chunk_var,
                       hyper, factors, clip_mode, zero_grad);
  else if (!nesterov)
    hipLaunchKernelGGL(sgd_clip_kernel<1>, grid, block, 0, as_stream(stream), p, g, accum, chunk_off, chunk_len, chunk_var,
                       hyper, factors, clip_mode, zero_grad);
  else
    hipLaunchKernelGGL(sgd_clip_kernel<2>, grid, block, 0, as_stream(stream), p, g, accum, chunk_off, chunk_len, chunk_var,
                       hyper, factors, clip_mode, zero_grad);
  return check_launch("sgd_clip_kernel");
}
