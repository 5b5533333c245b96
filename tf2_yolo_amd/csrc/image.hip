// Network input from raw pixels: N packed uint8 RGB images of any sizes -> float32 NHWC [N, H, W, 3], resized into a target
// region per image (bilinear, half-pixel centres, no antialias: cv2.INTER_LINEAR / torch interpolate(align_corners=False)),
// padded outside it and rescaled, in one launch for the whole batch.
#include "common.hpp"

namespace yolo {

// one table entry per image (32 bytes; tf2_yolo_amd/images.py packs the same layout)
struct ImageEntry {
  long long off;        // byte offset of the image in the source buffer
  int sh, sw;           // source height and width
  int y0, x0, rh, rw;   // target region of the output
};
static_assert(sizeof(ImageEntry) == 32, "the host packs 32-byte entries");

// Source coordinate of region index v in integers (source extent n, region extent r): the position is
// (2 v + 1) n / (2 r) - 1/2 = ((2 v + 1) n - r) / (2 r), clamped to [0, n - 1]. n <= 16384 and r <= 4096 keep num under 2^28.
__device__ __forceinline__ void axis_taps(int v, int n, int r, int& lo, int& hi, float& f) {
  const int den = 2 * r;
  int num = (2 * v + 1) * n - r;
  num = max(0, min(num, (n - 1) * den));
  lo = num / den;
  hi = min(lo + 1, n - 1);
  f = (float)(num - lo * den) / (float)den;
}

// an entry the kernel may read pixels of: positive sizes within the limits and an extent inside the source buffer
__device__ __forceinline__ bool entry_ok(const ImageEntry& e, long long src_bytes) {
  if (e.sh <= 0 || e.sw <= 0 || e.rh <= 0 || e.rw <= 0) return false;
  if (e.sh > YOLO_IMAGE_MAX_SRC || e.sw > YOLO_IMAGE_MAX_SRC || e.rh > YOLO_IMAGE_MAX_DST || e.rw > YOLO_IMAGE_MAX_DST) return false;
  if (e.y0 < -YOLO_IMAGE_MAX_DST || e.y0 > YOLO_IMAGE_MAX_DST || e.x0 < -YOLO_IMAGE_MAX_DST || e.x0 > YOLO_IMAGE_MAX_DST) return false;
  const long long bytes = (long long)e.sh * e.sw * 3;
  return e.off >= 0 && e.off <= src_bytes && bytes <= src_bytes - e.off;
}

// V floats per work item (4: one float4 store; W * 3 % 4 == 0, so an item never crosses a row). items = N H W 3 / V.
template <int V>
__global__ void image_prepare_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                     const ImageEntry* __restrict__ tab, int H, int W, float rescale, float pad,
                                     float* __restrict__ out, unsigned items) {
  const unsigned row = (unsigned)W * 3u;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
    const unsigned e0 = i * V;
    const unsigned r = e0 / row;               // n H + y
    const unsigned xc0 = e0 - r * row;         // x 3 + c of the first float
    const unsigned n = r / (unsigned)H;
    const int y = (int)(r - n * (unsigned)H);
    const ImageEntry e = tab[n];
    const int v = y - e.y0;
    float res[V];
#pragma unroll
    for (int k = 0; k < V; ++k) res[k] = pad;
    if (entry_ok(e, src_bytes) && v >= 0 && v < e.rh) {
      const unsigned char* img = src + e.off;
      int ylo, yhi, xlo = 0, xhi = 0, px = -1;
      float fy, fx = 0.f;
      axis_taps(v, e.sh, e.rh, ylo, yhi, fy);
      const unsigned char* top = img + (size_t)ylo * e.sw * 3;
      const unsigned char* bot = img + (size_t)yhi * e.sw * 3;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int x = (int)((xc0 + k) / 3u), c = (int)((xc0 + k) - 3u * (unsigned)x);
        const int u = x - e.x0;
        if (u < 0 || u >= e.rw) continue;
        if (x != px) {
          axis_taps(u, e.sw, e.rw, xlo, xhi, fx);
          px = x;
        }
        const float a = (float)top[xlo * 3 + c], b = (float)top[xhi * 3 + c];
        const float p = (float)bot[xlo * 3 + c], q = (float)bot[xhi * 3 + c];
        const float t = a + fx * (b - a), s = p + fx * (q - p);
        res[k] = (t + fy * (s - t)) * rescale;
      }
    }
    if constexpr (V == 4) {
      f32x4 o = {res[0], res[1], res[2], res[3]};
      *reinterpret_cast<f32x4*>(out + e0) = o;
    } else {
      out[e0] = res[0];
    }
  }
}

}  // namespace yolo

using namespace yolo;

extern "C" int yolo_image_prepare(const unsigned char* src, long long src_bytes, const void* table, int N, int H, int W,
                                  float rescale, float pad_grey, float* out, void* stream) {
  YOLO_REQUIRE(src && table && out, "image_prepare: null pointer");
  YOLO_REQUIRE(N > 0 && H > 0 && W > 0 && src_bytes > 0, "image_prepare: sizes must be positive");
  YOLO_REQUIRE(H <= YOLO_IMAGE_MAX_DST && W <= YOLO_IMAGE_MAX_DST, "image_prepare: output sides over %d", YOLO_IMAGE_MAX_DST);
  YOLO_REQUIRE((long long)N * H * W * 3 < (1LL << 31), "image_prepare: more than 2^31 output values in one call");
  YOLO_REQUIRE((reinterpret_cast<size_t>(table) & 7) == 0, "image_prepare: the table must be 8-byte aligned");
  const float pad = pad_grey * rescale;
  const auto* tab = static_cast<const ImageEntry*>(table);
  const int vec = ((W * 3) % 4 == 0 && (reinterpret_cast<size_t>(out) & 15) == 0) ? 1 : 0;
  const unsigned items = (unsigned)((long long)N * H * W * 3 / (vec ? 4 : 1));   // work items: one per float4, else per float
  if (vec)
    hipLaunchKernelGGL(image_prepare_kernel<4>, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), src,
                       src_bytes, tab, H, W, rescale, pad, out, items);
  else
    hipLaunchKernelGGL(image_prepare_kernel<1>, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), src,
                       src_bytes, tab, H, W, rescale, pad, out, items);
  return check_launch("image_prepare_kernel");
}
