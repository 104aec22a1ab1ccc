// lpips.hip — LPIPS-Alex in fp32 (include/udt_kernels.h, "LPIPS"): the input stage, an fp32 convolution on f32-input MFMA, the 3x3 / 2
// max-pool and the per-tap distance.  Activations are fp32, channels-last: pixel (n, y, x) of a [N, H, W, C] map starts at element
// ((n H + y) W + x) ld, ld >= C, and only its first C elements are read or written.
//
// Nothing here uses a floating-point atomic: every sum has one fixed order, so a result depends on the values alone — not on the
// run, not on the leading dimensions.
#include "common.h"
#include "conv_f32.h"

namespace {

// ---- udt_conv2d_f32 / udt_conv2d_rect_f32: implicit GEMM, rows = output pixels (n, oy, ox), columns = output channels,
// k = (ky kw + kx) Cin + c (conv_f32.h: one kernel behind both entry points) -------------------------------------------------------
// A 256-thread workgroup owns a 128-pixel x 64-channel tile; wave w owns pixels 32 w .. 32 w + 31 and all 64 channels in two
// v_mfma_f32_32x32x2_f32 accumulators (one wave per SIMD; the instruction's dependent latency equals its issue interval, so the
// accumulator count does not bound the issue rate).  What bounds this kernel is its LDS staging — one buffer and two barriers per
// chunk, nothing software-pipelined: it measures 40 % of the fp32 peak (profiles/lpips.txt).  K runs in chunks of 16: thread t gathers column t % 16 of the chunk for the 8 pixel
// rows and 4 weight rows t / 16 + 16 i into registers while the previous chunk is multiplied, then the tile goes through LDS as
// [k][row].  A tap outside the image, a pixel row >= M, a weight row >= Cout and a k >= K contribute a ZERO that is produced here:
// no address outside the operands is formed into a load.
constexpr int CV_BM = udt_conv_f32::BM, CV_BN = udt_conv_f32::BN, CV_BK = udt_conv_f32::BK;
constexpr int CV_LDA = CV_BM + 4, CV_LDB = CV_BN + 4;      // (+4: the 16 x 4 (k, row) pairs a wave writes at once fall into 64 distinct banks)
constexpr int CV_FLUSH = 8;                                // chunks per fused-multiply-add chain: 128 k, then the chain is added to the total
constexpr int CV_NOWHERE = -(1 << 28);                     // iy0 / ix0 of a pixel row >= M: no tap of it is inside any image

using ConvParams = udt_conv_f32::Params;

__global__ void __launch_bounds__(256) conv2d_f32_kernel(const ConvParams p) {
  __shared__ float As[CV_BK * CV_LDA];
  __shared__ float Bs[CV_BK * CV_LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = tid & 15, r0 = tid >> 4;
  const long long m0 = (long long)blockIdx.x * CV_BM;
  const int n0 = (int)blockIdx.y * CV_BN;

  long long pix[8];          // pixel index of tap (0, 0) of the row's window (may lie before the image: it is only used with a valid tap)
  int iy0[8], ix0[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const long long m = m0 + r0 + 16 * i;
    if (m < p.M) {
      const int ox = (int)(m % p.Wo);
      const long long t = m / p.Wo;
      const int oy = (int)(t % p.Ho);
      const long long n = t / p.Ho;
      iy0[i] = oy * p.stride - p.pad_h;
      ix0[i] = ox * p.stride - p.pad_w;
      pix[i] = (n * p.H + iy0[i]) * p.W + ix0[i];
    } else {
      iy0[i] = ix0[i] = CV_NOWHERE;
      pix[i] = 0;
    }
  }

  float ra[8], rb[4];
  auto gather = [&](int chunk) {
    const int k = chunk * CV_BK + kk;
    const bool k_ok = k < p.K;
    const int tap = k / p.Cin, ch = k - tap * p.Cin;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    const long long koff = (long long)ky * p.W + kx;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool ok = k_ok && (unsigned)(iy0[i] + ky) < (unsigned)p.H && (unsigned)(ix0[i] + kx) < (unsigned)p.W;
      ra[i] = ok ? p.x[(pix[i] + koff) * p.ldx + ch] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + r0 + 16 * i;
      rb[i] = n < p.Cout ? p.w[(long long)n * p.Kp + k] : 0.f;          // (k < Kp: the packed rows are zero from K on)
    }
  };

  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 acc0 = zero, acc1 = zero, tot0 = zero, tot1 = zero;
  const int l31 = lane & 31, h = lane >> 5;
  const int chunks = p.Kp / CV_BK;
  gather(0);
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();                                         // (the previous chunk's reads are done)
#pragma unroll
    for (int i = 0; i < 8; ++i) As[kk * CV_LDA + r0 + 16 * i] = ra[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) Bs[kk * CV_LDB + r0 + 16 * i] = rb[i];
    __syncthreads();
    if (c + 1 < chunks) gather(c + 1);
#pragma unroll
    for (int kp = 0; kp < CV_BK / 2; ++kp) {
      const float a = As[(2 * kp + h) * CV_LDA + 32 * wave + l31];
      const float b0 = Bs[(2 * kp + h) * CV_LDB + l31];
      const float b1 = Bs[(2 * kp + h) * CV_LDB + 32 + l31];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
    if ((c & (CV_FLUSH - 1)) == CV_FLUSH - 1 || c + 1 == chunks) {      // blocked summation: a chain ends after 128 k
      tot0 += acc0;
      tot1 += acc1;
      acc0 = zero;
      acc1 = zero;
    }
  }

  // accumulator element r of lane (l31, h): pixel row (r & 3) + 8 (r >> 2) + 4 h, channel column l31
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + 32 * j + l31;
    if (col >= p.Cout) continue;
    const float b = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m >= p.M) continue;
      float v = (j == 0 ? tot0[r] : tot1[r]) + b;
      if (p.relu) v = fmaxf(v, 0.f);
      p.out[m * p.ldo + col] = v;
    }
  }
}

// ---- udt_maxpool3s2_f32: one thread per output element, channel fastest; the maximum starts from the window's first element ------
__global__ void __launch_bounds__(256) maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ out, long long total, int H, int W,
                                                         int C, int ldx, int ldo, int Ho, int Wo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long pixel = idx / C;
  const int ox = (int)(pixel % Wo);
  const long long t = pixel / Wo;
  const int oy = (int)(t % Ho);
  const long long n = t / Ho;
  const float* src = x + ((n * H + 2 * oy) * W + 2 * ox) * ldx + c;
  float m = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float v = src[((long long)dy * W + dx) * ldx];
      m = (v > m || v != v) ? v : m;                            // (a NaN wins, as in nn.MaxPool2d)
    }
  out[pixel * ldo + c] = m;
}

// ---- udt_lpips_input_f32: one thread per pixel of the 2 N frames --------------------------------------------------------------------
__global__ void __launch_bounds__(256) lpips_input_kernel(const float* __restrict__ samples, const float* __restrict__ images,
                                                          const float* __restrict__ shift, const float* __restrict__ scale,
                                                          float* __restrict__ out, long long total, int N, long long HW, int ldo,
                                                          int quantise) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n2 = idx / HW, px = idx - n2 * HW;
  const bool fake = n2 < N;
  const float* src = (fake ? samples + n2 * 3 * HW : images + (n2 - N) * 3 * HW) + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = src[c * HW];
    // every product is rounded on its own (no contraction): these are the fp32 array operations of the reference's saving code
    float v = fake ? __fmul_rn(s, 255.f) : __fmul_rn(__fmul_rn(__fadd_rn(s, 1.f), 0.5f), 255.f);
    v = fminf(fmaxf(v, 0.f), 255.f);
    if (quantise) v = truncf(v);
    const float t = (float)((double)v / 127.5 - 1.0);
    out[idx * ldo + c] = __fdiv_rn(__fsub_rn(t, shift[c]), scale[c]);
  }
}

// ---- udt_lpips_layer_f32 ----------------------------------------------------------------------------------------------------------------
// sum over the wave, the same bits in every lane (the lanes of a rotate-and-add butterfly add in different orders: lane 0's sum is taken)
UDT_DEVINL float wave_sum_uniform(float v) {
  v = xor32_sum(xor16_sum(row16_sum(v)));
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

constexpr int LP_PIX = 64;                                  // pixels per workgroup: 16 consecutive ones per wave

// workgroup (blk, n): pixels 64 blk .. 64 blk + 63 of pair n -> partial[n nblk + blk]
__global__ void __launch_bounds__(256) lpips_layer_kernel(const float* __restrict__ f, const float* __restrict__ w, float* __restrict__ partial,
                                                          int N, long long P, int C, int ld) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n = blockIdx.y;
  const float* f0 = f + n * P * ld;
  const float* f1 = f + (n + N) * P * ld;
  float wsum = 0.f;
  for (int i = 0; i < LP_PIX / 4; ++i) {
    const long long px = (long long)blockIdx.x * LP_PIX + wave * (LP_PIX / 4) + i;
    if (px >= P) break;                                      // (wave-uniform)
    const float* a = f0 + px * ld;
    const float* b = f1 + px * ld;
    float s0 = 0.f, s1 = 0.f;
    for (int c = lane; c < C; c += 64) {
      s0 = __builtin_fmaf(a[c], a[c], s0);
      s1 = __builtin_fmaf(b[c], b[c], s1);
    }
    const float na = __fadd_rn(__fsqrt_rn(wave_sum_uniform(s0)), 1e-10f);
    const float nb = __fadd_rn(__fsqrt_rn(wave_sum_uniform(s1)), 1e-10f);
    float d = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float df = __fsub_rn(__fdiv_rn(a[c], na), __fdiv_rn(b[c], nb));
      d = __builtin_fmaf(__fmul_rn(w[c], df), df, d);
    }
    wsum += wave_sum_uniform(d);
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) partial[n * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per pair: lane l adds partials l, l + 64, ... in ascending order, then the wave sum; / P; written or added to out[n]
__global__ void __launch_bounds__(64) lpips_layer_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblk, float fP,
                                                               int accumulate) {
  const long long n = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < nblk; j += 64) s += partial[n * nblk + j];
  s = wave_sum_uniform(s);
  if (threadIdx.x == 0) {
    const float v = __fdiv_rn(s, fP);
    out[n] = accumulate ? __fadd_rn(out[n], v) : v;
  }
}

long long lpips_layer_blocks(long long P) { return (P + LP_PIX - 1) / LP_PIX; }

}  // namespace

int udt_conv_f32::launch(Params& p, hipStream_t s) {
  p.Ho = (p.H + 2 * p.pad_h - p.kh) / p.stride + 1;
  p.Wo = (p.W + 2 * p.pad_w - p.kw) / p.stride + 1;
  p.K = p.kh * p.kw * p.Cin;
  p.Kp = (p.K + CV_BK - 1) / CV_BK * CV_BK;
  p.M = (long long)p.N * p.Ho * p.Wo;
  const long long mt = (p.M + CV_BM - 1) / CV_BM, nt = (p.Cout + CV_BN - 1) / CV_BN;
  if (mt > 0x7fffffffLL || nt > 65535) return UDT_ERR_BAD_SHAPE;                            // grid limits
  UdtProfScope prof(0, s);
  hipLaunchKernelGGL(conv2d_f32_kernel, dim3((unsigned)mt, (unsigned)nt), dim3(256), 0, s, p);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_conv2d_f32(const float* x, const float* w, const float* bias, float* out, int32_t N, int32_t H, int32_t W, int32_t Cin,
                              int32_t ld_x, int32_t Cout, int32_t ld_out, int32_t ksize, int32_t stride, int32_t pad, int32_t relu,
                              void* stream) {
  if (!x || !w || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || Cin > (1 << 20) || ld_x < Cin || ld_out < Cout) return UDT_ERR_BAD_SHAPE;
  if (ksize < 1 || ksize > 11 || stride < 1 || stride > 4 || pad < 0 || pad >= ksize) return UDT_ERR_BAD_SHAPE;
  if (H + 2 * pad < ksize || W + 2 * pad < ksize) return UDT_ERR_BAD_SHAPE;                 // no output pixel
  ConvParams p;
  p.x = x; p.w = w; p.bias = bias; p.out = out;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.ldx = ld_x; p.Cout = Cout; p.ldo = ld_out; p.kh = p.kw = ksize; p.stride = stride;
  p.pad_h = p.pad_w = pad; p.relu = relu != 0;
  return udt_conv_f32::launch(p, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int udt_maxpool3s2_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ld_x, int32_t ld_out,
                                  void* stream) {
  if (!x || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 3 || W < 3 || C < 1 || ld_x < C || ld_out < C) return UDT_ERR_BAD_SHAPE;
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long long total = (long long)N * Ho * Wo * C;
  if (total > (1LL << 38)) return UDT_ERR_BAD_SHAPE;                                         // (grid limit: 2^31 workgroups of 256)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, total, (int)H, (int)W, (int)C,
                     (int)ld_x, (int)ld_out, Ho, Wo);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_lpips_input_f32(const float* samples, const float* images, const float* shift, const float* scale, float* out, int32_t N,
                                   int32_t H, int32_t W, int32_t ld_out, int32_t quantise, void* stream) {
  if (!samples || !images || !shift || !scale || !out) return UDT_ERR_BAD_ARG;
  if (N < 1 || H < 1 || W < 1 || ld_out < 3) return UDT_ERR_BAD_SHAPE;
  const long long HW = (long long)H * W, total = 2LL * N * HW;
  if (total > (1LL << 38)) return UDT_ERR_BAD_SHAPE;                                         // (grid limit: 2^31 workgroups of 256)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, samples, images, shift, scale, out, total,
                     (int)N, HW, (int)ld_out, (int)(quantise != 0));
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" size_t udt_lpips_layer_scratch_bytes(int32_t N, int64_t P) {
  if (N < 1 || P < 1) return 0;
  return (size_t)N * (size_t)lpips_layer_blocks(P) * sizeof(float);
}

extern "C" int udt_lpips_layer_f32(const float* feats, const float* w, float* out, int32_t N, int64_t P, int32_t C, int32_t ld,
                                   int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream) {
  if (!feats || !w || !out || !scratch) return UDT_ERR_BAD_ARG;
  if (N < 1 || N > 65535 || P < 1 || C < 1 || ld < C) return UDT_ERR_BAD_SHAPE;
  const long long nblk = lpips_layer_blocks(P);
  if (nblk > 0x7fffffffLL) return UDT_ERR_BAD_SHAPE;                                         // grid limit
  if (scratch_bytes < udt_lpips_layer_scratch_bytes(N, P)) return UDT_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)nblk, (unsigned)N), dim3(256), 0, s, feats, w, reinterpret_cast<float*>(scratch),
                     (int)N, (long long)P, (int)C, (int)ld);
  UDT_CHECK_LAUNCH();
  hipLaunchKernelGGL(lpips_layer_final_kernel, dim3((unsigned)N), dim3(64), 0, s, reinterpret_cast<const float*>(scratch), out, (int)nblk,
                     (float)P, (int)(accumulate != 0));
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}
