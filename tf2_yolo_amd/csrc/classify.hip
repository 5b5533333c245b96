// The classifier top (yolov3/models/darknet.py:38-40, yolov4/models/darknet.py:39-41, yolov1_5/models/darknet.py:18-19,
// yolov2/models/darknet.py:23-25): GlobalAveragePooling2D, Dense + softmax, categorical cross-entropy, categorical accuracy.
// fp32 storage, NHWC, wave64. Every sum below has ONE order, fixed by the shape alone: a lane walks its elements upwards, lanes
// are folded by wave_reduce_* (xor butterfly), waves through LDS in index order. No atomics anywhere, so a step that ends in
// this top is as bit-reproducible as one that ends in a detection head.
#include "common.hpp"

namespace yolo {

// ---- global average pooling ------------------------------------------------------------------------------------------------
// x [N][HW][C] -> g [N][C]. blockDim = (64, 4): the 64 lanes of a wave read 64 consecutive channels of one pixel (256 B, one
// line), wave y takes pixels y, y + 4, ...; the four partial sums meet in LDS and are added in the order 0, 1, 2, 3.
__global__ void __launch_bounds__(256) gap_fwd_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ g) {
  __shared__ double part[4][64];
  const int c = blockIdx.x * 64 + threadIdx.x;
  const long long n = blockIdx.y;
  double acc = 0.0;
  if (c < C) {
    const float* xn = x + n * HW * (long long)C + c;
    for (int p = threadIdx.y; p < HW; p += 4) acc += (double)xn[(long long)p * C];
  }
  part[threadIdx.y][threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.y == 0 && c < C) {
    const double s = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    g[n * C + c] = (float)(s / (double)HW);
  }
}

// dx [N][HW][C] (+)= dg [N][C] / HW: one thread per element, C innermost
__global__ void __launch_bounds__(256) gap_bwd_kernel(const float* __restrict__ dg, long long total, int HW, int C, float inv,
                                                      float* __restrict__ dx, int accumulate) {
  const long long per = (long long)HW * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per;
    const int c = (int)(i % C);
    const float v = dg[n * C + c] * inv;
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

// ---- Dense + softmax -------------------------------------------------------------------------------------------------------
constexpr int DENSE_NT = 8;   // rows of g per workgroup

// logits[n][k] = b[k] + sum_c g[n][c] W[k][c]. One wave per output column k (4 per workgroup), DENSE_NT rows of g per workgroup:
// the wave reads W[k][:] once, 256 B per instruction, and the rows of g (shared by every wave: cache hits) against it.
__global__ void __launch_bounds__(256) dense_fwd_kernel(const float* __restrict__ g, const float* __restrict__ W,
                                                        const float* __restrict__ b, int N, int C, int K,
                                                        float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n0 = blockIdx.y * DENSE_NT;
  if (k >= K) return;     // (whole waves leave: no barrier below)
  float acc[DENSE_NT];
#pragma unroll
  for (int j = 0; j < DENSE_NT; ++j) acc[j] = 0.f;
  const float* wk = W + (long long)k * C;
  for (int c = lane; c < C; c += 64) {
    const float w = wk[c];
#pragma unroll
    for (int j = 0; j < DENSE_NT; ++j)
      if (n0 + j < N) acc[j] = fmaf(g[(long long)(n0 + j) * C + c], w, acc[j]);
  }
#pragma unroll
  for (int j = 0; j < DENSE_NT; ++j) {
    const float s = wave_reduce_sum(acc[j]);
    if (lane == 0 && n0 + j < N) logits[(long long)(n0 + j) * K + k] = s + b[k];
  }
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// p[n][:] = softmax(z[n][:]) with the row maximum subtracted; one wave per row
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* __restrict__ z, int N, int K, float* __restrict__ p) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* zn = z + (long long)n * K;
  float m = -INFINITY;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, zn[k]);
  m = wave_reduce_max(m);
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += expf(zn[k] - m);
  s = wave_reduce_sum(s);
  const float inv = 1.f / s;
  for (int k = lane; k < K; k += 64) p[(long long)n * K + k] = expf(zn[k] - m) * inv;
}

// dz[n][:] = p ⊙ (dp − Σ_k p_k dp_k); one wave per row
__global__ void __launch_bounds__(256) softmax_bwd_rows_kernel(const float* __restrict__ dp, const float* __restrict__ p, int N,
                                                               int K, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* pn = p + (long long)n * K;
  const float* dn = dp + (long long)n * K;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s = fmaf(pn[k], dn[k], s);
  s = wave_reduce_sum(s);
  for (int k = lane; k < K; k += 64) dz[(long long)n * K + k] = pn[k] * (dn[k] - s);
}

// dW[k][c] += Σ_n dz[n][k] g[n][c] (n upwards), db[k] += Σ_n dz[n][k]: one thread per filter element, c innermost
__global__ void __launch_bounds__(256) dense_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ g, int N, int C,
                                                          int K, float* __restrict__ dW, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (c >= C) return;
  float acc = 0.f, accb = 0.f;
  for (int n = 0; n < N; ++n) {
    const float d = dz[(long long)n * K + k];
    acc = fmaf(d, g[(long long)n * C + c], acc);
    accb += d;
  }
  dW[(long long)k * C + c] += acc;
  if (c == 0) db[k] += accb;
}

// dg[n][c] = Σ_k dz[n][k] W[k][c]. blockDim = (64, DENSE_KS): lane = channel, wave y sums the y-th of DENSE_KS contiguous
// ranges of k upwards for DENSE_NT rows (a thousand classes are 63 steps per wave, not a thousand: the loop is a chain of
// dependent loads and the grid is small); the partial sums meet in LDS (32 KB) and are added in the order 0, 1, 2, ...
constexpr int DENSE_KS = 16;

__global__ void __launch_bounds__(64 * DENSE_KS) dense_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ W,
                                                                    int N, int C, int K, float* __restrict__ dg) {
  __shared__ float part[DENSE_KS][DENSE_NT][64];
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int n0 = blockIdx.y * DENSE_NT;
  const int kq = (K + DENSE_KS - 1) / DENSE_KS;
  const int k0 = threadIdx.y * kq, k1 = min(K, k0 + kq);
  float acc[DENSE_NT];
#pragma unroll
  for (int j = 0; j < DENSE_NT; ++j) acc[j] = 0.f;
  if (c < C) {
    for (int k = k0; k < k1; ++k) {
      const float w = W[(long long)k * C + c];
#pragma unroll
      for (int j = 0; j < DENSE_NT; ++j)
        if (n0 + j < N) acc[j] = fmaf(dz[(long long)(n0 + j) * K + k], w, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < DENSE_NT; ++j) part[threadIdx.y][j][threadIdx.x] = acc[j];
  __syncthreads();
  if (threadIdx.y == 0 && c < C) {
#pragma unroll
    for (int j = 0; j < DENSE_NT; ++j)
      if (n0 + j < N) {
        float s = part[0][j][threadIdx.x];
#pragma unroll
        for (int y = 1; y < DENSE_KS; ++y) s += part[y][j][threadIdx.x];
        dg[(long long)(n0 + j) * C + c] = s;
      }
  }
}

// ---- categorical cross-entropy on probabilities (Keras categorical_crossentropy, from_logits=False) ------------------------
// q = p / Σp, q̂ = clip(q, 1e-7, 1 - 1e-7), loss = mean_n(−Σ_k t log q̂). With m_k = [1e-7 <= q_k <= 1 - 1e-7] (the clip passes
// no gradient outside its range) and dq_k/dp_j = (δ_kj − q_k) / Σp:
//   dloss/dp[n][j] = −(t_j m_j / q̂_j − Σ_k t_k m_k q_k / q̂_k) / (Σp · N).
// ONE workgroup of 16 waves: wave w takes rows w, w + 16, ... and adds their losses upwards in double; the 16 sums meet in LDS.
constexpr float CCE_EPS = 1e-7f;

__global__ void __launch_bounds__(1024) cce_kernel(const float* __restrict__ t, const float* __restrict__ p, int N, int K,
                                                   double* __restrict__ loss_out, float* __restrict__ dpred, float grad_scale) {
  __shared__ double part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double loss = 0.0;
  for (int n = wave; n < N; n += 16) {
    const float* tn = t + (long long)n * K;
    const float* pn = p + (long long)n * K;
    double S = 0.0;
    for (int k = lane; k < K; k += 64) S += (double)pn[k];
    S = wave_reduce_sum(S);
    const float Sf = (float)S;
    double l = 0.0, corr = 0.0;
    for (int k = lane; k < K; k += 64) {
      const float q = pn[k] / Sf;
      const float qc = fminf(fmaxf(q, CCE_EPS), 1.f - CCE_EPS);
      const bool in = q >= CCE_EPS && q <= 1.f - CCE_EPS;
      l -= (double)tn[k] * log((double)qc);
      if (in) corr += (double)tn[k] * (double)(q / qc);
    }
    l = wave_reduce_sum(l);
    corr = wave_reduce_sum(corr);
    loss += l;
    if (dpred != nullptr) {
      const double f = (double)grad_scale / (S * (double)N);
      for (int k = lane; k < K; k += 64) {
        const float q = pn[k] / Sf;
        const float qc = fminf(fmaxf(q, CCE_EPS), 1.f - CCE_EPS);
        const bool in = q >= CCE_EPS && q <= 1.f - CCE_EPS;
        const double own = in ? (double)tn[k] / (double)qc : 0.0;
        dpred[(long long)n * K + k] = (float)(-(own - corr) * f);
      }
    }
  }
  if (lane == 0) part[wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < 16; ++w) s += part[w];
    loss_out[0] = s / (double)N;
    for (int i = 1; i < 8; ++i) loss_out[i] = 0.0;
  }
}

// first maximal index of a row (tf.argmax): a lane keeps the first of its own, lanes fold by (value, then lower index)
__device__ __forceinline__ int row_argmax(const float* __restrict__ r, int K, int lane) {
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const float v = r[k];
    if (v > best || idx == 0x7fffffff) {
      best = v;
      idx = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (oi != 0x7fffffff && (idx == 0x7fffffff || ov > best || (ov == best && oi < idx))) {
      best = ov;
      idx = oi;
    }
  }
  return idx;
}

__global__ void __launch_bounds__(1024) accuracy_kernel(const float* __restrict__ t, const float* __restrict__ p, int N, int K,
                                                        double* __restrict__ out) {
  __shared__ int part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int hits = 0;
  for (int n = wave; n < N; n += 16)
    hits += row_argmax(t + (long long)n * K, K, lane) == row_argmax(p + (long long)n * K, K, lane) ? 1 : 0;
  if (lane == 0) part[wave] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < 16; ++w) s += part[w];
    out[0] = (double)s / (double)N;
  }
}

// ---- BatchNormalization + activation over ANY channel count -----------------------------------------------------------------
// darknet19's class convolution (yolov2/models/darknet.py:23) is normalised over class_num channels -- 10 by default -- and the
// kernels of bn_act.hip walk their channels four or eight at a time. The tensor here is the last feature map times class_num
// (a few thousand pixels), so ONE workgroup per channel does everything: statistics in two passes in double (mean, then
// centred squares), the Keras moving-statistics update, scale / shift, and the activation. Thread t takes pixels t, t + 256,
// ... upwards, the 256 partial sums fold through LDS in a fixed tree.
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();          // (sh may still be read from the previous sum)
  sh[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ float act_any(float z, int act) { return act == YOLO_ACT_LEAKY ? (z > 0.f ? z : 0.1f * z) : z; }

// training != 0: batch statistics of y (the convolution WITHOUT its bias, as the other BatchNorm units: the bias cancels in
// y - mean and only the moving mean adds it back, mean_offset); else the moving statistics. scale / shift / save_* [C] are
// written for the backward pass; out = act(fma(scale, y, shift)).
__global__ void __launch_bounds__(256) bn_act_any_fwd_kernel(const float* __restrict__ y, long long P, int C,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                             const float* __restrict__ mean_offset, float eps, float momentum,
                                                             int unbiased, int training, int act, float* __restrict__ scale,
                                                             float* __restrict__ shift, float* __restrict__ save_mean,
                                                             float* __restrict__ save_invstd, float* __restrict__ out) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  double mean, var;
  if (training) {
    double s = 0.0;
    for (long long p = threadIdx.x; p < P; p += 256) s += (double)y[p * C + c];
    mean = block_sum_256(s, sh) / (double)P;
    double q = 0.0;
    for (long long p = threadIdx.x; p < P; p += 256) {
      const double d = (double)y[p * C + c] - mean;
      q += d * d;
    }
    var = block_sum_256(q, sh) / (double)P;
  } else {
    mean = (double)moving_mean[c];
    var = (double)moving_var[c];
  }
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const float sc = (float)((double)gamma[c] * invstd);
  const float sf = (float)((double)beta[c] - mean * (double)gamma[c] * invstd);
  for (long long p = threadIdx.x; p < P; p += 256) out[p * C + c] = act_any(fmaf(sc, y[p * C + c], sf), act);
  if (threadIdx.x == 0) {
    scale[c] = sc;
    shift[c] = sf;
    if (training) {
      save_mean[c] = (float)mean;
      save_invstd[c] = (float)invstd;
      const double fed = unbiased && P > 1 ? var * (double)P / (double)(P - 1) : var;
      const double off = mean_offset ? (double)mean_offset[c] : 0.0;
      moving_mean[c] = (float)((double)moving_mean[c] * momentum + (mean + off) * (1.0 - (double)momentum));
      moving_var[c] = (float)((double)moving_var[c] * momentum + fed * (1.0 - (double)momentum));
    }
  }
}

// dz = dout * act'(fma(scale, y, shift)); dbeta += Σ dz, dgamma += Σ dz x̂; dy = gamma invstd (dz − mean(dz) − x̂ mean(dz x̂))
__global__ void __launch_bounds__(256) bn_act_any_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dout,
                                                             long long P, int C, const float* __restrict__ gamma,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ save_mean,
                                                             const float* __restrict__ save_invstd, int act,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             float* __restrict__ dy) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  const float sc = scale[c], sf = shift[c], mean = save_mean[c], invstd = save_invstd[c];
  double s1 = 0.0, s2 = 0.0;
  for (long long p = threadIdx.x; p < P; p += 256) {
    const float v = y[p * C + c];
    const float z = fmaf(sc, v, sf);
    const float dz = (act == YOLO_ACT_LEAKY && !(z > 0.f)) ? 0.1f * dout[p * C + c] : dout[p * C + c];
    s1 += (double)dz;
    s2 += (double)dz * ((double)(v - mean) * (double)invstd);
  }
  s1 = block_sum_256(s1, sh);
  s2 = block_sum_256(s2, sh);
  const double m1 = s1 / (double)P, m2 = s2 / (double)P, gi = (double)gamma[c] * (double)invstd;
  for (long long p = threadIdx.x; p < P; p += 256) {
    const float v = y[p * C + c];
    const float z = fmaf(sc, v, sf);
    const float dz = (act == YOLO_ACT_LEAKY && !(z > 0.f)) ? 0.1f * dout[p * C + c] : dout[p * C + c];
    const double xh = (double)(v - mean) * (double)invstd;
    dy[p * C + c] = (float)(gi * ((double)dz - m1 - xh * m2));
  }
  if (threadIdx.x == 0) {
    dgamma[c] += (float)s2;
    dbeta[c] += (float)s1;
  }
}

}  // namespace yolo

using namespace yolo;

extern "C" int yolo_bn_act_any_fwd(const float* y, long long P, int C, const float* gamma, const float* beta,
                                   float* moving_mean, float* moving_var, const float* mean_offset, float eps, float momentum,
                                   int unbiased_moving_var, int training, int act, float* scale, float* shift,
                                   float* save_mean, float* save_invstd, float* out, void* stream) {
  YOLO_REQUIRE(y && gamma && beta && moving_mean && moving_var && scale && shift && out && P > 0 && C > 0 && C <= 65535,
               "bn_act_any_fwd: bad args");
  YOLO_REQUIRE(!training || (save_mean && save_invstd), "bn_act_any_fwd: training needs save_mean / save_invstd");
  YOLO_REQUIRE(act == YOLO_ACT_LINEAR || act == YOLO_ACT_LEAKY, "bn_act_any_fwd: linear or LeakyReLU only (act=%d)", act);
  hipLaunchKernelGGL(bn_act_any_fwd_kernel, dim3(C), dim3(256), 0, as_stream(stream), y, P, C, gamma, beta, moving_mean,
                     moving_var, mean_offset, eps, momentum, unbiased_moving_var, training, act, scale, shift, save_mean,
                     save_invstd, out);
  return check_launch("bn_act_any_fwd_kernel");
}

extern "C" int yolo_bn_act_any_bwd(const float* y, const float* dout, long long P, int C, const float* gamma,
                                   const float* scale, const float* shift, const float* save_mean, const float* save_invstd,
                                   int act, float* dgamma, float* dbeta, float* dy, void* stream) {
  YOLO_REQUIRE(y && dout && gamma && scale && shift && save_mean && save_invstd && dgamma && dbeta && dy && P > 0 && C > 0 &&
                   C <= 65535,
               "bn_act_any_bwd: bad args");
  YOLO_REQUIRE(act == YOLO_ACT_LINEAR || act == YOLO_ACT_LEAKY, "bn_act_any_bwd: linear or LeakyReLU only (act=%d)", act);
  hipLaunchKernelGGL(bn_act_any_bwd_kernel, dim3(C), dim3(256), 0, as_stream(stream), y, dout, P, C, gamma, scale, shift,
                     save_mean, save_invstd, act, dgamma, dbeta, dy);
  return check_launch("bn_act_any_bwd_kernel");
}

extern "C" int yolo_gap_fwd(const float* x, int N, int H, int W, int C, float* g, void* stream) {
  YOLO_REQUIRE(x && g && N > 0 && H > 0 && W > 0 && C > 0, "gap_fwd: bad args");
  YOLO_REQUIRE(N <= 65535 && (long long)H * W < (1LL << 31), "gap_fwd: N=%d exceeds the grid's second dimension", N);
  hipLaunchKernelGGL(gap_fwd_kernel, dim3((C + 63) / 64, N), dim3(64, 4), 0, as_stream(stream), x, H * W, C, g);
  return check_launch("gap_fwd_kernel");
}

extern "C" int yolo_gap_bwd(const float* dg, int N, int H, int W, int C, float* dx, int accumulate, void* stream) {
  YOLO_REQUIRE(dg && dx && N > 0 && H > 0 && W > 0 && C > 0 && (long long)H * W < (1LL << 31), "gap_bwd: bad args");
  const long long total = (long long)N * H * W * C;
  hipLaunchKernelGGL(gap_bwd_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(stream), dg, total, H * W, C,
                     1.f / (float)((long long)H * W), dx, accumulate);
  return check_launch("gap_bwd_kernel");
}

extern "C" int yolo_dense_softmax_fwd(const float* g, const float* W, const float* b, int N, int C, int K, float* logits,
                                      float* p, void* stream) {
  YOLO_REQUIRE(g && p && N > 0 && C > 0 && K > 0, "dense_softmax_fwd: bad args");
  YOLO_REQUIRE((W == nullptr) == (b == nullptr), "dense_softmax_fwd: kernel and bias come together or not at all");
  const float* z = g;
  if (W != nullptr) {
    YOLO_REQUIRE(logits != nullptr, "dense_softmax_fwd: the Dense form needs a logits buffer");
    YOLO_REQUIRE((N + DENSE_NT - 1) / DENSE_NT <= 65535, "dense_softmax_fwd: N=%d too large", N);
    hipLaunchKernelGGL(dense_fwd_kernel, dim3((K + 3) / 4, (N + DENSE_NT - 1) / DENSE_NT), dim3(256), 0, as_stream(stream), g, W,
                       b, N, C, K, logits);
    if (int rc = check_launch("dense_fwd_kernel")) return rc;
    z = logits;
  } else {
    YOLO_REQUIRE(K == C, "dense_softmax_fwd: without weights the softmax is over g itself (K=%d, C=%d)", K, C);
    YOLO_REQUIRE(logits == nullptr || logits == g, "dense_softmax_fwd: without weights the logits ARE g");
  }
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), z, N, K, p);
  return check_launch("softmax_rows_kernel");
}

extern "C" int yolo_dense_softmax_bwd(const float* dp, const float* p, const float* g, const float* W, int N, int C, int K,
                                      float* dz, float* dg, float* dW, float* db, void* stream) {
  YOLO_REQUIRE(dp && p && dg && N > 0 && C > 0 && K > 0, "dense_softmax_bwd: bad args");
  if (W == nullptr) {
    YOLO_REQUIRE(K == C && dW == nullptr && db == nullptr, "dense_softmax_bwd: without weights K == C and there is no dW / db");
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), dp, p, N, K, dg);
    return check_launch("softmax_bwd_rows_kernel");
  }
  YOLO_REQUIRE(g && dz && dW && db, "dense_softmax_bwd: the Dense form needs g, a dz workspace [N, K], dW and db");
  YOLO_REQUIRE(K <= 65535 && (N + DENSE_NT - 1) / DENSE_NT <= 65535, "dense_softmax_bwd: K=%d or N=%d too large", K, N);
  hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), dp, p, N, K, dz);
  if (int rc = check_launch("softmax_bwd_rows_kernel")) return rc;
  hipLaunchKernelGGL(dense_wgrad_kernel, dim3((C + 255) / 256, K), dim3(256), 0, as_stream(stream), dz, g, N, C, K, dW, db);
  if (int rc = check_launch("dense_wgrad_kernel")) return rc;
  hipLaunchKernelGGL(dense_dgrad_kernel, dim3((C + 63) / 64, (N + DENSE_NT - 1) / DENSE_NT), dim3(64, DENSE_KS), 0,
                     as_stream(stream), dz, W, N, C, K, dg);
  return check_launch("dense_dgrad_kernel");
}

extern "C" int yolo_cce_fwd_bwd(const float* t, const float* p, int N, int K, double* loss_out, float* dpred, float grad_scale,
                                void* stream) {
  YOLO_REQUIRE(t && p && loss_out && N > 0 && K > 0, "cce_fwd_bwd: bad args");
  hipLaunchKernelGGL(cce_kernel, dim3(1), dim3(1024), 0, as_stream(stream), t, p, N, K, loss_out, dpred, grad_scale);
  return check_launch("cce_kernel");
}

extern "C" int yolo_categorical_accuracy(const float* t, const float* p, int N, int K, double* out, void* stream) {
  YOLO_REQUIRE(t && p && out && N > 0 && K > 0, "categorical_accuracy: bad args");
  hipLaunchKernelGGL(accuracy_kernel, dim3(1), dim3(1024), 0, as_stream(stream), t, p, N, K, out);
  return check_launch("accuracy_kernel");
}
