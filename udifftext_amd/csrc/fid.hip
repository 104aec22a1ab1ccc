// fid.hip — what the FID InceptionV3 needs on top of csrc/lpips.hip (include/udt_kernels.h, "FID"): rectangular convolutions on the
// same fp32 MFMA kernel, 3x3 pools with padding, the 299 x 299 input stage, the global average pool and the fp64 moments of the pool
// features.  Activations are fp32, channels-last with a pixel stride ld >= C, as in lpips.hip: a channel slice of a wider map is a
// pointer offset plus that map's ld, which is how a block's branches write their part of the concatenation.
//
// No floating-point atomics: every sum has one fixed order, so a result depends on the values alone.
#include "common.h"
#include "bilinear.h"
#include "conv_f32.h"

namespace {

// ---- udt_pool3_f32: one thread per output element, channel fastest; taps in row-major window order, those outside the image skipped
__global__ void __launch_bounds__(256) pool3_kernel(const float* __restrict__ x, float* __restrict__ out, long long total, int H, int W, int C,
                                                    int ldx, int ldo, int Ho, int Wo, int stride, int pad, int average) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long pixel = idx / C;
  const int ox = (int)(pixel % Wo);
  const long long t = pixel / Wo;
  const int oy = (int)(t % Ho);
  const long long n = t / Ho;
  const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
  float m = -INFINITY, s = 0.f;
  int taps = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iy = iy0 + dy, ix = ix0 + dx;
      if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
      const float v = x[((n * H + iy) * W + ix) * ldx + c];
      m = (v > m || v != v) ? v : m;                            // (a NaN wins, as in nn.MaxPool2d and udt_maxpool3s2_f32)
      s = __fadd_rn(s, v);
      ++taps;
    }
  out[pixel * ldo + c] = average ? __fdiv_rn(s, (float)taps) : m;   // (taps >= 1: pad <= 1 < 3)
}

// ---- udt_fid_input_f32: one thread per pixel of the 2 N output frames --------------------------------------------------------------
__global__ void __launch_bounds__(256) fid_input_kernel(const float* __restrict__ samples, const float* __restrict__ images,
                                                        float* __restrict__ out, long long total, int N, int H, int W, int S, int ldo,
                                                        int quantise) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % S);
  const long long rest = idx / S;
  const int oy = (int)(rest % S);
  const long long n2 = rest / S;
  const bool fake = n2 < N;
  const long long HW = (long long)H * W;
  const float* src = fake ? samples + n2 * 3 * HW : images + (n2 - N) * 3 * HW;
  const BlTap ty = bl_tap(oy, H, S), tx = bl_tap(ox, W, S);
  // the saved 8-bit value over 255 (ToTensor); every fp32 operation rounded on its own, as in udt_lpips_input_f32
  auto frame = [&](const float* plane, int y, int x) {
    const float s = plane[(long long)y * W + x];
    float v = fake ? __fmul_rn(s, 255.f) : __fmul_rn(__fmul_rn(__fadd_rn(s, 1.f), 0.5f), 255.f);
    v = fminf(fmaxf(v, 0.f), 255.f);
    if (quantise) v = truncf(v);
    return __fdiv_rn(v, 255.f);
  };
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* plane = src + c * HW;
    const float top = __builtin_fmaf(tx.w1, frame(plane, ty.i0, tx.i1), __fmul_rn(tx.w0, frame(plane, ty.i0, tx.i0)));
    const float bot = __builtin_fmaf(tx.w1, frame(plane, ty.i1, tx.i1), __fmul_rn(tx.w0, frame(plane, ty.i1, tx.i0)));
    const float r = __builtin_fmaf(ty.w1, bot, __fmul_rn(ty.w0, top));
    out[idx * ldo + c] = __fsub_rn(__fmul_rn(2.f, r), 1.f);
  }
}

// ---- udt_mean_pixels_f32: one thread per (image, channel); pixels added in ascending order, one division -----------------------------
__global__ void __launch_bounds__(256) mean_pixels_kernel(const float* __restrict__ x, float* __restrict__ out, long long total, long long P,
                                                          int C, int ldx, int ldo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long n = idx / C;
  const float* src = x + n * P * ldx + c;
  float s = 0.f;
  for (long long p = 0; p < P; ++p) s = __fadd_rn(s, src[p * ldx]);
  out[n * ldo + c] = __fdiv_rn(s, (float)P);
}

// ---- udt_moments_accum_f64 ---------------------------------------------------------------------------------------------------------------
// outer += X^T X on v_mfma_f64_16x16x4_f64, the FULL D x D matrix: wave (ti, tj) owns the 16 x 16 tile of rows i0 = 16 ti, columns
// j0 = 16 tj, and nobody else touches it.  The contraction index is the row r of X, four rows per instruction in ascending order:
// lane l supplies A[i = l & 15][k = l >> 4] = X[r0 + k][i0 + i] and B[k = l >> 4][j = l & 15] = X[r0 + k][j0 + j], each fp32 value
// converted exactly to fp64; a row >= n and a column >= D supply a ZERO that is not loaded.  The instruction's D operand is NOT laid
// out like the f32 forms': element g of lane l is row (l >> 4) + 4 g, column l & 15.
// The waves of tile column 0 also own sum[i0 .. i0 + 15]: lanes 0 .. 15 add their column's rows in ascending order.
// One read-modify-write of every output element per launch.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ void __launch_bounds__(256) moments_kernel(const float* __restrict__ x, double* __restrict__ sum, double* __restrict__ outer, int n,
                                                      int D, int ld, int tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ti = blockIdx.x, tj = (int)blockIdx.y * 4 + wave;
  if (tj >= tiles) return;                                     // (wave-uniform; no barrier follows)
  const int l15 = lane & 15, k = lane >> 4;
  const int ci = 16 * ti + l15, cj = 16 * tj + l15;
  const bool i_ok = ci < D, j_ok = cj < D;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < n; r0 += 4) {
    const int r = r0 + k;
    const bool r_ok = r < n;
    const double a = (r_ok && i_ok) ? (double)x[(long long)r * ld + ci] : 0.0;
    const double b = (r_ok && j_ok) ? (double)x[(long long)r * ld + cj] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  if (j_ok) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = 16 * ti + k + 4 * g;
      if (row < D) outer[(long long)row * D + cj] += acc[g];
    }
  }
  if (tj == 0 && lane < 16 && i_ok) {
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += (double)x[(long long)r * ld + ci];
    sum[ci] += s;
  }
}

}  // namespace

extern "C" int udt_conv2d_rect_f32(const float* x, const float* w, const float* bias, float* out, int32_t N, int32_t H, int32_t W,
                                   int32_t Cin, int32_t ld_x, int32_t Cout, int32_t ld_out, int32_t kh, int32_t kw, int32_t stride,
                                   int32_t pad_h, int32_t pad_w, int32_t relu, void* stream) {
  if (!x || !w || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || Cin > (1 << 20) || ld_x < Cin || ld_out < Cout) return UDT_ERR_BAD_SHAPE;
  if (kh < 1 || kh > 11 || kw < 1 || kw > 11 || stride < 1 || stride > 4) return UDT_ERR_BAD_SHAPE;
  if (pad_h < 0 || pad_h >= kh || pad_w < 0 || pad_w >= kw) return UDT_ERR_BAD_SHAPE;
  if (H + 2 * pad_h < kh || W + 2 * pad_w < kw) return UDT_ERR_BAD_SHAPE;                   // no output pixel
  udt_conv_f32::Params p;
  p.x = x; p.w = w; p.bias = bias; p.out = out;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.ldx = ld_x; p.Cout = Cout; p.ldo = ld_out; p.kh = kh; p.kw = kw; p.stride = stride;
  p.pad_h = pad_h; p.pad_w = pad_w; p.relu = relu != 0;
  return udt_conv_f32::launch(p, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int udt_pool3_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ld_x, int32_t ld_out,
                             int32_t stride, int32_t pad, int32_t average, void* stream) {
  if (!x || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 1 || W < 1 || C < 1 || ld_x < C || ld_out < C) return UDT_ERR_BAD_SHAPE;
  if (stride < 1 || stride > 2 || pad < 0 || pad > 1 || H + 2 * pad < 3 || W + 2 * pad < 3) return UDT_ERR_BAD_SHAPE;
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const long long total = (long long)N * Ho * Wo * C;
  if (total > (1LL << 38)) return UDT_ERR_BAD_SHAPE;                                         // (grid limit: 2^31 workgroups of 256)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(pool3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, total, (int)H, (int)W, (int)C, (int)ld_x,
                     (int)ld_out, Ho, Wo, (int)stride, (int)pad, (int)(average != 0));
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_fid_input_f32(const float* samples, const float* images, float* out, int32_t N, int32_t H, int32_t W, int32_t size,
                                 int32_t ld_out, int32_t quantise, void* stream) {
  if (!samples || !images || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 1 || W < 1 || size < 1 || size > 4096 || ld_out < 3) return UDT_ERR_BAD_SHAPE;
  const long long total = 2LL * N * size * size;
  if (total > (1LL << 38)) return UDT_ERR_BAD_SHAPE;                                         // (grid limit: 2^31 workgroups of 256)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(fid_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, samples, images, out, total, (int)N, (int)H,
                     (int)W, (int)size, (int)ld_out, (int)(quantise != 0));
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_mean_pixels_f32(const float* x, float* out, int32_t N, int64_t P, int32_t C, int32_t ld_x, int32_t ld_out, void* stream) {
  if (!x || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || P < 1 || P > (1LL << 24) || C < 1 || ld_x < C || ld_out < C) return UDT_ERR_BAD_SHAPE;   // (P exact as an fp32 divisor)
  const long long total = (long long)N * C;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(mean_pixels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, total, (long long)P, (int)C,
                     (int)ld_x, (int)ld_out);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_moments_accum_f64(const float* x, double* sum, double* outer, int32_t n, int32_t D, int32_t ld, void* stream) {
  if (!x || !sum || !outer) return UDT_ERR_BAD_ARG;
  if (n < 1 || D < 1 || D > (1 << 18) || ld < D) return UDT_ERR_BAD_SHAPE;                   // (D: 16384 x 4096 workgroups at most)
  const int tiles = (D + 15) / 16;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(1, s);
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)tiles, (unsigned)((tiles + 3) / 4)), dim3(256), 0, s, x, sum, outer, (int)n, (int)D,
                     (int)ld, tiles);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}
