// ocr_backward.hip — the kernels of the OCR loss and of the reverse pass through the OCR scorer (PARSeq) that csrc/backward.hip does
// not already hold (reference sgm/modules/diffusionmodules/loss.py:178-190, sgm/modules/predictors/model.py:40-58):
//
//   udt_mattn_bwd          backward of udt_mattn_fwd (masked small attention): dq (optional), dk, dv
//   udt_gelu_fwd / _bwd    exact-erf GELU on stored pre-activations (the inference GEMM epilogue keeps none)
//   udt_ocr_ce_f32         clamped character cross entropy of every row and its seed d loss / d logits, one launch
//
// (udt_crop_resize_aa_bwd_f32, the adjoint of the scorer's input side, lives next to its forward in csrc/resample.hip: they share the
// tap rule.)  Nothing here uses atomics: every output element is written by exactly one thread, sums run in a fixed order, results are
// bit-identical from run to run.
#include "common.h"
#include <math.h>
#include <atomic>

namespace {
#include "tile_common.h"      // AttrOnce: the dynamic-LDS attribute, once per (kernel, device), thread-safe

// ---------------------------------------------------------------------------------------------------------------------
// masked small attention, backward.  One workgroup per (head, sample) — the unit of the forward — so dk / dv need no reduction across
// workgroups: K and V of the head sit in LDS as fp32 (row stride D + 1, as in the forward), the queries are walked in tiles of
// MB_TQ rows (Q, dO tile [MB_TQ][D + 1]; P and dS tile [MB_TQ][lk]), and every thread keeps its share of dk / dv — up to 4 pieces of
// 8 channels of one key — in registers over all tiles.  Per tile: (1) one wave per query recomputes the scores and the softmax as the
// forward does (lanes own keys), dP = dO V^T, delta = sum_l P dP, dS = P (dP - delta); (2) dv += P^T dO, dk += dS^T Q in the owners'
// registers, query rows in ascending order; (3) dq = scale dS K for the tile.  LDS at the largest shapes (lk D = 8192, lk = 256):
// 2 x 33 KB + 2 x 4 KB + 2 x 16 KB = 106 KB.
constexpr int MB_TQ = 16;        // query rows per tile
constexpr int MB_PIECES = 4;     // 8-channel pieces of dk / dv per thread: lk D / 8 <= 1024 = 4 x 256

struct MattnBwdParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const uint16_t* d_o;
  uint16_t* dq;
  uint16_t* dk;
  uint16_t* dv;
  const float* mask;
  const uint8_t* kpm;
  int heads, D, nq, lk;
  int ldq, ldk, ldv, lddo, lddq, lddk, lddv, ldmask;
  long long sq, sk, sv, sdo, sdq, sdk, sdv;
  float scale;
};

UDT_DEVINL uint16_t bf16_of(float x) { return (uint16_t)(pack_bf16x2(x, 0.f) & 0xffffu); }

__global__ void __launch_bounds__(256) mattn_bwd_kernel(const MattnBwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char msm[];
  const int D = p.D, RS = D + 1, lk = p.lk, D8 = D >> 3;
  float* ks = reinterpret_cast<float*>(msm);                 // [lk][D + 1]
  float* vs = ks + lk * RS;                                  // [lk][D + 1]
  float* qs = vs + lk * RS;                                  // [MB_TQ][D + 1]
  float* gs = qs + MB_TQ * RS;                               // [MB_TQ][D + 1]   (dO)
  float* pt = gs + MB_TQ * RS;                               // [MB_TQ][lk]      (P)
  float* dst = pt + MB_TQ * lk;                              // [MB_TQ][lk]      (dS)
  const int h = blockIdx.x, b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < lk * D; i += 256) {
    const int l = i / D, d = i - l * D;
    ks[l * RS + d] = bf16_bits_to_f32(p.k[(long long)b * p.sk + (long long)l * p.ldk + h * D + d]);
    vs[l * RS + d] = bf16_bits_to_f32(p.v[(long long)b * p.sv + (long long)l * p.ldv + h * D + d]);
  }
  // this thread's pieces of dk / dv: piece c = threadIdx.x + 256 j -> key c / D8, channels 8 (c % D8) .. + 7
  const int npieces = lk * D8;
  int pl[MB_PIECES], pd[MB_PIECES];
  float akv[MB_PIECES][8], avv[MB_PIECES][8];
#pragma unroll
  for (int j = 0; j < MB_PIECES; ++j) {
    const int c = (int)threadIdx.x + 256 * j;
    pl[j] = c < npieces ? c / D8 : -1;
    pd[j] = c < npieces ? (c - pl[j] * D8) * 8 : 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) akv[j][e] = avv[j][e] = 0.f;
  }

  for (int q0 = 0; q0 < p.nq; q0 += MB_TQ) {
    const int tq = min(MB_TQ, p.nq - q0);
    __syncthreads();                                         // (K, V staged; the previous tile's P / dS / Q / dO no longer read)
    for (int i = threadIdx.x; i < tq * D; i += 256) {
      const int r = i / D, d = i - r * D;
      qs[r * RS + d] = bf16_bits_to_f32(p.q[(long long)b * p.sq + (long long)(q0 + r) * p.ldq + h * D + d]);
      gs[r * RS + d] = bf16_bits_to_f32(p.d_o[(long long)b * p.sdo + (long long)(q0 + r) * p.lddo + h * D + d]);
    }
    __syncthreads();
    // (1) P and dS of the tile's rows: wave w takes rows w, w + 4, ...
    for (int r = wave; r < tq; r += 4) {
      const int qi = q0 + r;
      float sc[4], dp[4];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = lane + j * 64;
        float s = -INFINITY, g = 0.f;
        if (l < lk) {
          s = 0.f;
          for (int d = 0; d < D; ++d) {
            s += qs[r * RS + d] * ks[l * RS + d];
            g += gs[r * RS + d] * vs[l * RS + d];
          }
          s *= p.scale;
          if (p.mask) s += p.mask[(long long)qi * p.ldmask + l];
          if (p.kpm && p.kpm[(long long)b * lk + l]) s = -INFINITY;
        }
        sc[j] = s;
        dp[j] = g;
        mx = fmaxf(mx, s);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[j] = (mx == -INFINITY || sc[j] == -INFINITY) ? 0.f : __expf(sc[j] - mx);
        sum += sc[j];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float inv = sum > 0.f ? 1.0f / sum : 0.f;
      float delta = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[j] *= inv;
        delta += sc[j] * dp[j];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) delta += __shfl_xor(delta, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = lane + j * 64;
        if (l < lk) {
          pt[r * lk + l] = sc[j];
          dst[r * lk + l] = sc[j] * (dp[j] - delta);
        }
      }
    }
    __syncthreads();
    // (2) dv += P^T dO, dk += dS^T Q
#pragma unroll
    for (int j = 0; j < MB_PIECES; ++j) {
      if (pl[j] < 0) continue;
      for (int r = 0; r < tq; ++r) {
        const float pv = pt[r * lk + pl[j]], dsv = dst[r * lk + pl[j]];
        const float* gr = gs + r * RS + pd[j];
        const float* qr = qs + r * RS + pd[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          avv[j][e] = __builtin_fmaf(pv, gr[e], avv[j][e]);
          akv[j][e] = __builtin_fmaf(dsv, qr[e], akv[j][e]);
        }
      }
    }
    // (3) dq of the tile: piece c -> row c / D8, channels 8 (c % D8) .. + 7
    if (p.dq) {
      for (int c = threadIdx.x; c < tq * D8; c += 256) {
        const int r = c / D8, d0 = (c - r * D8) * 8;
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
        for (int l = 0; l < lk; ++l) {
          const float dsv = dst[r * lk + l];
          const float* kr = ks + l * RS + d0;
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = __builtin_fmaf(dsv, kr[e], a[e]);
        }
        uint16_t* o = p.dq + (long long)b * p.sdq + (long long)(q0 + r) * p.lddq + h * D + d0;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = bf16_of(a[e] * p.scale);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MB_PIECES; ++j) {
    if (pl[j] < 0) continue;
    uint16_t* ok = p.dk + (long long)b * p.sdk + (long long)pl[j] * p.lddk + h * D + pd[j];
    uint16_t* ov = p.dv + (long long)b * p.sdv + (long long)pl[j] * p.lddv + h * D + pd[j];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ok[e] = bf16_of(akv[j][e] * p.scale);
      ov[e] = bf16_of(avv[j][e]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// exact-erf GELU on stored pre-activations, 8 channels per thread.  erf by Abramowitz-Stegun 7.1.26 as gelu_erf_f (common.h).
// The pre-activations are fp32 — the GEMM's accumulators as they are (UDT_GEMM_OUT_F32) — so that the tape-mode forward rounds where the
// fused inference epilogue rounds: once, after the GELU.
UDT_DEVINL float erf_as7(float x) {
  const float z = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
  float poly = 1.061405429f;
  poly = poly * t - 1.453152027f;
  poly = poly * t + 1.421413741f;
  poly = poly * t - 0.284496736f;
  poly = poly * t + 0.254829592f;
  poly = poly * t;
  const float e = __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);
  return __builtin_copysignf(1.0f - poly * e, x);
}

template <bool BWD>
__global__ void __launch_bounds__(256) gelu_kernel(const float* __restrict__ a, const uint16_t* __restrict__ dy,
                                                   uint16_t* __restrict__ out, long long n8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + i * 8), a1 = *reinterpret_cast<const f32x4*>(a + i * 8 + 4);
  const float af[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
  float o[8];
  if constexpr (!BWD) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = gelu_erf_f(af[j]);
  } else {
    const u32x4 dv = *reinterpret_cast<const u32x4*>(dy + i * 8);
    float df[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { df[2 * j] = bf16_lo(dv[j]); df[2 * j + 1] = bf16_hi(dv[j]); }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float phi_c = 0.5f * (1.0f + erf_as7(af[j] * 0.70710678118654752f));
      const float pdf = 0.3989422804014327f * __expf(-0.5f * af[j] * af[j]);
      o[j] = df[j] * (phi_c + af[j] * pdf);
    }
  }
  const u32x4 pk = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
  *reinterpret_cast<u32x4*>(out + i * 8) = pk;
}

// ---------------------------------------------------------------------------------------------------------------------
// clamped character cross entropy and its seed.  One workgroup per row b; wave w takes the positions t = w, w + 4, ... and its lanes
// the classes (4 per lane).  The row is tiny (L <= 256 positions of <= 256 classes), so the log-sum-exp and the softmax are evaluated in
// fp64: the only rounding of a result is its conversion to fp32.  Thread 0 adds the characters' cross entropies in ascending order.
constexpr int CE_MAX = 256;

__global__ void __launch_bounds__(256) ocr_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets,
                                                     const int32_t* __restrict__ n_chars, const float* __restrict__ weight,
                                                     float* __restrict__ loss, float* __restrict__ d_logits, int L, int n_cls, int ld,
                                                     int T, int ld_d) {
  __shared__ double s_mx[CE_MAX], s_lse[CE_MAX], s_ce[CE_MAX];
  __shared__ int s_flow;
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = min(max(n_chars[b], 1), min(L, T));          // (validated on the host; clamped so that no address leaves the row)
  const float* row = logits + (long long)b * L * ld;
  for (int t = wave; t < n; t += 4) {
    const float* x = row + (long long)t * ld;
    double xv[4];
    double mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      xv[j] = c < n_cls ? (double)x[c] : -INFINITY;
      mx = fmax(mx, xv[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += (lane + 64 * j < n_cls) ? exp(xv[j] - mx) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
      const int tg = min(max(targets[(long long)b * T + t], 0), n_cls - 1);
      const double lse = log(sum);
      s_mx[t] = mx;
      s_lse[t] = lse;
      s_ce[t] = (lse + mx) - (double)x[tg];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int t = 0; t < n; ++t) acc += s_ce[t];
    const double mean = acc / (double)n;
    const bool flows = mean <= 1.0;                          // torch's clamp(max=1) rule; false for NaN as well
    s_flow = flows ? 1 : 0;
    loss[b] = (float)(flows ? mean : (mean > 1.0 ? 1.0 : mean));
  }
  __syncthreads();
  const bool flows = s_flow != 0;
  const double wn = (weight ? (double)weight[b] : 1.0) / (double)n;
  float* drow = d_logits + (long long)b * L * ld_d;
  for (int t = wave; t < L; t += 4) {
    const bool live = flows && t < n;
    const float* x = row + (long long)t * ld;
    const int tg = live ? min(max(targets[(long long)b * T + t], 0), n_cls - 1) : -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      if (c >= n_cls) continue;
      float g = 0.f;
      if (live) {
        const double sm = exp(((double)x[c] - s_mx[t]) - s_lse[t]);
        g = (float)(wn * (sm - (c == tg ? 1.0 : 0.0)));
      }
      drow[(long long)t * ld_d + c] = g;
    }
  }
}

}  // namespace

#define UDT_OCR_STREAM hipStream_t s = reinterpret_cast<hipStream_t>(stream); UdtProfScope prof(5, s)

extern "C" int udt_mattn_bwd(const void* q, const void* k, const void* v, const void* d_o, void* dq, void* dk, void* dv,
                             const float* mask, const uint8_t* kpm, int32_t batch, int32_t heads, int32_t head_dim, int32_t nq,
                             int32_t lk, int32_t ldq, int32_t ldk, int32_t ldv, int32_t lddo, int32_t lddq, int32_t lddk, int32_t lddv,
                             int32_t ldmask, int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t do_bstride,
                             int64_t dq_bstride, int64_t dk_bstride, int64_t dv_bstride, float scale, void* stream) {
  if (!q || !k || !v || !d_o || !dk || !dv) return UDT_ERR_BAD_ARG;
  if (batch <= 0 || heads <= 0 || nq <= 0 || lk <= 0 || lk > 256 || batch > 65535) return UDT_ERR_BAD_SHAPE;
  if (head_dim <= 0 || head_dim > 64 || head_dim % 8 != 0 || (long long)lk * head_dim > 8192 || (long long)nq * head_dim > 8192)
    return UDT_ERR_BAD_SHAPE;
  const int hd = heads * head_dim;
  if (ldq < hd || ldk < hd || ldv < hd || lddo < hd || lddk < hd || lddv < hd || (dq && lddq < hd)) return UDT_ERR_BAD_SHAPE;
  if (mask && ldmask < lk) return UDT_ERR_BAD_SHAPE;
  MattnBwdParams p;
  p.q = reinterpret_cast<const uint16_t*>(q);
  p.k = reinterpret_cast<const uint16_t*>(k);
  p.v = reinterpret_cast<const uint16_t*>(v);
  p.d_o = reinterpret_cast<const uint16_t*>(d_o);
  p.dq = reinterpret_cast<uint16_t*>(dq);
  p.dk = reinterpret_cast<uint16_t*>(dk);
  p.dv = reinterpret_cast<uint16_t*>(dv);
  p.mask = mask; p.kpm = kpm;
  p.heads = heads; p.D = head_dim; p.nq = nq; p.lk = lk;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv; p.ldmask = ldmask;
  p.sq = q_bstride; p.sk = k_bstride; p.sv = v_bstride; p.sdo = do_bstride; p.sdq = dq_bstride; p.sdk = dk_bstride; p.sdv = dv_bstride;
  p.scale = scale;
  const size_t smem = ((size_t)2 * lk * (head_dim + 1) + (size_t)2 * MB_TQ * (head_dim + 1) + (size_t)2 * MB_TQ * lk) * sizeof(float);
  UDT_OCR_STREAM;
  static AttrOnce attr;
  const hipError_t e = attr.ensure(reinterpret_cast<const void*>(mattn_bwd_kernel), 112 * 1024);
  if (e != hipSuccess) return udt_set_hip_error(e);
  hipLaunchKernelGGL(mattn_bwd_kernel, dim3(heads, batch), dim3(256), smem, s, p);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_gelu_fwd(const void* a, void* out, int64_t rows, int32_t C, void* stream) {
  if (!a || !out) return UDT_ERR_BAD_ARG;
  if (rows <= 0 || C <= 0 || C % 8 != 0 || rows * (C / 8) > 0x7fffffffLL * 256) return UDT_ERR_BAD_SHAPE;
  UDT_OCR_STREAM;
  const long long n8 = rows * (C / 8);
  hipLaunchKernelGGL(gelu_kernel<false>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(a), nullptr,
                     static_cast<uint16_t*>(out), n8);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_gelu_bwd(const void* a, const void* dy, void* da, int64_t rows, int32_t C, void* stream) {
  if (!a || !dy || !da) return UDT_ERR_BAD_ARG;
  if (rows <= 0 || C <= 0 || C % 8 != 0 || rows * (C / 8) > 0x7fffffffLL * 256) return UDT_ERR_BAD_SHAPE;
  UDT_OCR_STREAM;
  const long long n8 = rows * (C / 8);
  hipLaunchKernelGGL(gelu_kernel<true>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(a),
                     static_cast<const uint16_t*>(dy), static_cast<uint16_t*>(da), n8);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_ocr_ce_f32(const float* logits, const int32_t* targets, const int32_t* n_chars, const float* weight, float* loss,
                              float* d_logits, int32_t N, int32_t L, int32_t n_cls, int32_t ld, int32_t T, int32_t ld_d, void* stream) {
  if (!logits || !targets || !n_chars || !loss || !d_logits) return UDT_ERR_BAD_ARG;
  if (N <= 0 || L <= 0 || L > CE_MAX || n_cls <= 0 || n_cls > CE_MAX || ld < n_cls || ld_d < n_cls || T <= 0) return UDT_ERR_BAD_SHAPE;
  UDT_OCR_STREAM;
  hipLaunchKernelGGL(ocr_ce_kernel, dim3((unsigned)N), dim3(256), 0, s, logits, targets, n_chars, weight, loss, d_logits, L, n_cls, ld, T,
                     ld_d);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}
