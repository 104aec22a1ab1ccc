// attn512_bwd.hip — udt_attn512_bwd: flash-attention backward for ONE head of 512 dims, self-attention (the AutoencoderKL mid-block
// attention under autograd; forward: udt_attn512_fwd, attention.hip), and the two elementwise steps of the OCR term of the training
// loss (udt_denoised_f32, udt_seed_add_bf16).
//
// dQ, dK, dV from Q, K, V, O, dO, as udt_attn_bwd (backward.hip) does it for head_dim 64: two launches of one kernel template, S
// recomputed tile by tile (no [n, n] tensor anywhere), no atomics, every sum in a fixed order (two runs are bit-identical, and the
// result does not depend on strides).
//   launch 1 ("dq"):  owner = 32 queries.  Pass 1 walks the keys for LSE (log2 domain) and computes D = rowsum(dO o O) (as the
//                     diagonal of O dO^T, in the arithmetic of dP); both are stored for launch 2.  Pass 2 walks the keys again: dQ^T[d][q] += sum_k K^T[d][k] dS[k][q].
//   launch 2 ("dkv"): owner = 32 keys, streamed = queries with their LSE and D:
//                     dV^T[d][k] += sum_q dO^T[d][q] P[q][k],   dK^T[d][k] += sum_q Q^T[d][q] dS[q][k].
// The forward's decomposition carries over: a workgroup is four waves, wave w owns head dims [128 w, 128 w + 128).  The score tiles
// S = X Y^T and dP contract over all 512 dims, so every wave computes the partial product over its own quarter (8 MFMAs 32x32x16
// each), parks it in LDS, and every wave adds the four partials in the order 0, 1, 2, 3: all four hold the same fp32 tile.  The
// second products need only the wave's own quarter of the streamed tile (transposed) and of the accumulators (4 tiles of 32 dims x
// 32 owner rows = 64 fp32 registers per lane and result).
//
// Roundings: q, k, v, o, d_o are bf16 operands; scores S, dP, the softmax statistics (running max, sum, LSE), D and all accumulators
// are fp32; P = exp2(S c - LSE) and dS = P (dP - D) are rounded to bf16 ONCE, as operands of the second products (dS without the
// softmax scale: it multiplies the finished dQ / dK sums in fp32); dq, dk, dv are rounded to bf16 once when stored.
//
// Rows and keys past n are masked and never read.  LDS: 32 x 512 row-major images of the two streamed tensors (A fragments of the
// scores), their transposes (A fragments of the second products), and the partial-score exchange, which lies over the row-major
// images (dead once the score MFMAs have read them): 138 KiB, one workgroup per CU.
#include "common.h"
#include <atomic>

namespace {

struct Attn512BwdParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const uint16_t* o;
  const uint16_t* d_o;
  uint16_t* dq;
  uint16_t* dk;
  uint16_t* dv;
  float* lse;              // [batch][n], log2 domain: m + log2(sum)
  float* dsum;             // [batch][n]
  int n, tiles;
  int ldq, ldk, ldv, ldo, lddo, ldd;
  long long sq, sk, sv, so, sdo, sd;
  float scale, scale_log2e;
};

constexpr int B5_XP = 520;                         // row-major pitch (elements): 1040 B, rows shift by 4 banks
constexpr int B5_TP = 36;                          // transposed pitch (elements): 72 B, the 8-byte fragment reads of 32 rows hit 32 bank pairs
constexpr int B5_X_BYTES = 32 * B5_XP * 2;         // 33280
constexpr int B5_T_BYTES = 512 * B5_TP * 2;        // 36864
constexpr int B5_OFF_X2 = B5_X_BYTES;
constexpr int B5_OFF_X1T = 2 * B5_X_BYTES;
constexpr int B5_OFF_X2T = B5_OFF_X1T + B5_T_BYTES;
constexpr int B5_OFF_SC = B5_OFF_X2T + B5_T_BYTES; // lse[32], d[32] floats
constexpr int B5_SMEM = B5_OFF_SC + (32 + 32) * 4;
static_assert(4 * 2 * 16 * 64 * 4 <= 2 * B5_X_BYTES, "the partial-score exchange lies over the two row-major images");
static_assert(B5_SMEM <= 160 * 1024, "LDS of one CU");

UDT_DEVINL u32x4 b5_load16(const uint16_t* p, bool ok) {
  u32x4 z = {0u, 0u, 0u, 0u};
  if (ok) z = *reinterpret_cast<const u32x4*>(p);
  return z;
}

template <bool DKV>
__global__ void __launch_bounds__(256) attn512_bwd_kernel(const Attn512BwdParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char b5_smem[];
  uint16_t* x1 = reinterpret_cast<uint16_t*>(b5_smem);
  uint16_t* x2 = reinterpret_cast<uint16_t*>(b5_smem + B5_OFF_X2);
  float* part = reinterpret_cast<float*>(b5_smem);                   // [wave][S | dP][r / 4][lane][4], over x1 / x2
  uint16_t* x1t = reinterpret_cast<uint16_t*>(b5_smem + B5_OFF_X1T);
  uint16_t* x2t = reinterpret_cast<uint16_t*>(b5_smem + B5_OFF_X2T);
  float* sc_lse = reinterpret_cast<float*>(b5_smem + B5_OFF_SC);
  float* sc_d = sc_lse + 32;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int b = blockIdx.x / p.tiles;
  const int tile = blockIdx.x - b * p.tiles;
  const uint16_t* Q = p.q + (long long)b * p.sq;
  const uint16_t* K = p.k + (long long)b * p.sk;
  const uint16_t* V = p.v + (long long)b * p.sv;
  const uint16_t* O = p.o + (long long)b * p.so;
  const uint16_t* DO = p.d_o + (long long)b * p.sdo;
  float* LSE = p.lse + (long long)b * p.n;
  float* DS = p.dsum + (long long)b * p.n;
  const int orow = tile * 32 + l31;
  const bool ook = orow < p.n;
  const float c = p.scale_log2e;
  const int d0 = wave * 128;                       // this wave's quarter of the head

  // owner fragments (B operands of the scores): 8 consecutive dims at d0 + ks * 16 + hi * 8 of this lane's row
  const uint16_t* Y1 = DKV ? K : Q;
  const uint16_t* Y2 = DKV ? V : DO;
  const int ldy1 = DKV ? p.ldk : p.ldq, ldy2 = DKV ? p.ldv : p.lddo;
  bf16x8_t y1f[8], y2f[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    y1f[ks] = __builtin_bit_cast(bf16x8_t, b5_load16(Y1 + (long long)orow * ldy1 + d0 + ks * 16 + hi * 8, ook));
    y2f[ks] = __builtin_bit_cast(bf16x8_t, b5_load16(Y2 + (long long)orow * ldy2 + d0 + ks * 16 + hi * 8, ook));
  }
  const uint16_t* X1 = DKV ? Q : K;
  const uint16_t* X2 = DKV ? DO : V;
  const int ldx1 = DKV ? p.ldq : p.ldk, ldx2 = DKV ? p.lddo : p.ldv;
  const int nst = (p.n + 31) / 32;

  // one streamed tile (32 rows x 512 dims of X1 and X2) -> LDS, one tile ahead in registers.  A thread holds the same 8 dims of
  // two neighbouring rows (4 such units per thread and tensor), so that the transposed image is written a row PAIR (one dword) at a
  // time; a wave instruction covers 8 row pairs x 8 chunks (128 contiguous bytes of each row).
  u32x4 ra[4][2], rb[4][2];
  float rl = 0.f, rd = 0.f;
  auto unit = [&](int i, int& a, int& sch) {
    const int u = wave * 4 + i;
    a = (u & 1) * 8 + (lane >> 3);                 // row pair 0 .. 15
    sch = (u >> 1) * 8 + (lane & 7);               // 16-byte chunk 0 .. 63
  };
  auto gload = [&](int st, bool second) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int a, sch;
      unit(i, a, sch);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int s = st * 32 + 2 * a + e;
        const bool ok = st < nst && s < p.n;
        ra[i][e] = b5_load16(X1 + (long long)s * ldx1 + sch * 8, ok);
        rb[i][e] = b5_load16(X2 + (long long)s * ldx2 + sch * 8, ok && second);
      }
    }
    if (DKV && second) {
      const int s2 = st * 32 + (tid & 31);
      const bool ok2 = st < nst && s2 < p.n;
      rl = ok2 ? LSE[s2] : 0.f;
      rd = ok2 ? DS[s2] : 0.f;
    }
  };
  auto tstore = [&](uint16_t* xt, const u32x4& r0, const u32x4& r1, int a, int sch) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<uint32_t*>(xt + (sch * 8 + 2 * j) * B5_TP + 2 * a) = (r0[j] & 0xffffu) | (r1[j] << 16);
      *reinterpret_cast<uint32_t*>(xt + (sch * 8 + 2 * j + 1) * B5_TP + 2 * a) = (r0[j] >> 16) | (r1[j] & 0xffff0000u);
    }
  };
  auto lstore = [&](bool second) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int a, sch;
      unit(i, a, sch);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        *reinterpret_cast<u32x4*>(x1 + (2 * a + e) * B5_XP + sch * 8) = ra[i][e];
        if (second) *reinterpret_cast<u32x4*>(x2 + (2 * a + e) * B5_XP + sch * 8) = rb[i][e];
      }
      if (second) {
        tstore(x1t, ra[i][0], ra[i][1], a, sch);
        if (DKV) tstore(x2t, rb[i][0], rb[i][1], a, sch);
      }
    }
    if (DKV && second && tid < 32) {
      sc_lse[tid] = rl;
      sc_d[tid] = rd;
    }
  };
  // partial scores over this wave's 128 dims: acc[r] = sum_d X[i = 8 (r >> 2) + 4 hi + (r & 3)][d] Y[j = l31][d]
  auto scores = [&](const uint16_t* xs, const bf16x8_t (&yf)[8]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(xs + l31 * B5_XP + d0 + ks * 16 + hi * 8);
      acc = mfma32(a, yf[ks], acc);
    }
    return acc;
  };
  // the four waves' partial tiles -> their sum in the order 0, 1, 2, 3, in every wave.  The exchange buffer lies over x1 / x2: the
  // first barrier says that every wave has read its score fragments.
  auto exchange = [&](f32x16& s, f32x16& dp, bool two) {
    __syncthreads();
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const f32x4 sv = {s[r4 * 4], s[r4 * 4 + 1], s[r4 * 4 + 2], s[r4 * 4 + 3]};
      *reinterpret_cast<f32x4*>(part + (((wave * 2 + 0) * 4 + r4) * 64 + lane) * 4) = sv;
      if (two) {
        const f32x4 dv = {dp[r4 * 4], dp[r4 * 4 + 1], dp[r4 * 4 + 2], dp[r4 * 4 + 3]};
        *reinterpret_cast<f32x4*>(part + (((wave * 2 + 1) * 4 + r4) * 64 + lane) * 4) = dv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      f32x4 sv = *reinterpret_cast<const f32x4*>(part + (((0 * 2 + 0) * 4 + r4) * 64 + lane) * 4);
      f32x4 dv = {0.f, 0.f, 0.f, 0.f};
      if (two) dv = *reinterpret_cast<const f32x4*>(part + (((0 * 2 + 1) * 4 + r4) * 64 + lane) * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        sv += *reinterpret_cast<const f32x4*>(part + (((w * 2 + 0) * 4 + r4) * 64 + lane) * 4);
        if (two) dv += *reinterpret_cast<const f32x4*>(part + (((w * 2 + 1) * 4 + r4) * 64 + lane) * 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[r4 * 4 + e] = sv[e];
        dp[r4 * 4 + e] = dv[e];
      }
    }
  };
  // A fragment of a transposed tile: rows d = d0 + it * 32 + l31, the 8 streamed indices of k-step `half` in the order P / dS sit in
  auto tfrag = [&](const uint16_t* xt, int it, int half) {
    const uint16_t* base = xt + (d0 + it * 32 + l31) * B5_TP + 16 * half + 4 * hi;
    const u32x2 lo = *reinterpret_cast<const u32x2*>(base);
    const u32x2 hh = *reinterpret_cast<const u32x2*>(base + 8);
    const u32x4 v4 = {lo[0], lo[1], hh[0], hh[1]};
    return __builtin_bit_cast(bf16x8_t, v4);
  };
  auto pack8 = [](const float* f) {
    const u32x4 v4 = {pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
    return __builtin_bit_cast(bf16x8_t, v4);
  };

  float lse_o = 0.f, d_o_sum = 0.f;
  if constexpr (!DKV) {
    // ---- pass 1: LSE of this lane's query over all keys (the two half-waves see different keys: merged at the end), and D
    float m_run = -INFINITY, l_run = 0.f;
    gload(0, false);
    for (int st = 0; st < nst; ++st) {
      __syncthreads();
      lstore(false);
      __syncthreads();
      gload(st + 1, false);
      f32x16 s = scores(x1, y1f), unused;
      exchange(s, unused, false);
      float sv[16];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = st * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
        sv[r] = key < p.n ? s[r] * c : -INFINITY;
        mx = fmaxf(mx, sv[r]);
      }
      if (mx > -INFINITY) {
        const float m_new = fmaxf(m_run, mx);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += fast_exp2(sv[r] - m_new);
        l_run = l_run * fast_exp2(m_run - m_new) + sum;
        m_run = m_new;
      }
    }
    const float m_oth = __shfl_xor(m_run, 32), l_oth = __shfl_xor(l_run, 32);
    const float m_all = fmaxf(m_run, m_oth);
    float l_all = 0.f;
    if (m_run > -INFINITY) l_all += l_run * fast_exp2(m_run - m_all);
    if (m_oth > -INFINITY) l_all += l_oth * fast_exp2(m_oth - m_all);
    lse_o = m_all + __log2f(l_all);
    // D = rowsum(dO o O) as the diagonal of O_tile dO_tile^T, through the same MFMAs and the same exchange as dP = dO V^T: where
    // a row of P is one-hot at a key whose V row is the query's O row, dP - D cancels exactly, as it does in exact arithmetic
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int a, sch;
      unit(i, a, sch);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int s = tile * 32 + 2 * a + e;
        *reinterpret_cast<u32x4*>(x2 + (2 * a + e) * B5_XP + sch * 8) = b5_load16(O + (long long)s * p.ldo + sch * 8, s < p.n);
      }
    }
    __syncthreads();
    f32x16 dd = scores(x2, y2f), unused;
    exchange(dd, unused, false);
    float dsel = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (8 * (r >> 2) + 4 * hi + (r & 3) == l31) dsel = dd[r];
    const float doth = __shfl_xor(dsel, 32);
    d_o_sum = hi == ((l31 >> 2) & 1) ? dsel : doth;
    if (ook && wave == 0 && hi == 0) {
      LSE[orow] = lse_o;
      DS[orow] = d_o_sum;
    }
  }

  f32x16 acc1[4], acc2[4];             // dq: acc1 = dQ^T; dkv: acc1 = dK^T, acc2 = dV^T   ([32-dim tile of the quarter][...])
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[it][r] = acc2[it][r] = 0.f;

  gload(0, true);
  for (int st = 0; st < nst; ++st) {
    __syncthreads();
    lstore(true);
    __syncthreads();
    gload(st + 1, true);
    f32x16 s = scores(x1, y1f);
    f32x16 dp = scores(x2, y2f);
    exchange(s, dp, true);
    float pv[16], dsv[16];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      f32x4 ls = {lse_o, lse_o, lse_o, lse_o}, dd = {d_o_sum, d_o_sum, d_o_sum, d_o_sum};
      if constexpr (DKV) {
        ls = *reinterpret_cast<const f32x4*>(sc_lse + 8 * q4 + 4 * hi);
        dd = *reinterpret_cast<const f32x4*>(sc_d + 8 * q4 + 4 * hi);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = q4 * 4 + e;
        const int sidx = st * 32 + 8 * q4 + 4 * hi + e;
        const float pr = (sidx < p.n && ook) ? fast_exp2(s[r] * c - ls[e]) : 0.f;
        pv[r] = pr;
        dsv[r] = pr * (dp[r] - dd[e]);                          // (the softmax scale multiplies the finished dQ / dK sums)
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const bf16x8_t dsf = pack8(dsv + half * 8);
#pragma unroll
      for (int it = 0; it < 4; ++it) acc1[it] = mfma32(tfrag(x1t, it, half), dsf, acc1[it]);
      if constexpr (DKV) {
        const bf16x8_t pf = pack8(pv + half * 8);
#pragma unroll
        for (int it = 0; it < 4; ++it) acc2[it] = mfma32(tfrag(x2t, it, half), pf, acc2[it]);
      }
    }
  }
  if (ook) {
    uint16_t* o1 = (DKV ? p.dk : p.dq) + (long long)b * p.sd + (long long)orow * p.ldd + d0;
    uint16_t* o2 = p.dv + (long long)b * p.sd + (long long)orow * p.ldd + d0;
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int d = it * 32 + 8 * q4 + 4 * hi;
        const u32x2 a = {pack_bf16x2(acc1[it][q4 * 4] * p.scale, acc1[it][q4 * 4 + 1] * p.scale),
                         pack_bf16x2(acc1[it][q4 * 4 + 2] * p.scale, acc1[it][q4 * 4 + 3] * p.scale)};
        *reinterpret_cast<u32x2*>(o1 + d) = a;
        if constexpr (DKV) {
          const u32x2 bb = {pack_bf16x2(acc2[it][q4 * 4], acc2[it][q4 * 4 + 1]), pack_bf16x2(acc2[it][q4 * 4 + 2], acc2[it][q4 * 4 + 3])};
          *reinterpret_cast<u32x2*>(o2 + d) = bb;
        }
      }
  }
}

// ------------------------------------------------------------------------------------------------ OCR term: elementwise steps
// D[b, c, pix] = c_skip[b] noised[b, c, pix] + c_out[b] F[b, pix, c] for the 4 latent channels: F is the UNet head's fp32 NHWC output
// (ld floats per pixel), noised and D are fp32 NCHW.  One lane per pixel: one 16-byte load of F, four plane loads / stores that are
// contiguous across the wave.
__global__ void __launch_bounds__(256) denoised_kernel(const float* __restrict__ f, const float* __restrict__ noised,
                                                       const float* __restrict__ c_skip, const float* __restrict__ c_out,
                                                       float* __restrict__ out, int hw, int ld, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / hw);
  const int pix = (int)(i - (long long)b * hw);
  const float cs = c_skip[b], co = c_out[b];
  const f32x4 fv = *reinterpret_cast<const f32x4*>(f + i * ld);
  const long long base = (long long)b * 4 * hw + pix;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) out[base + (long long)ch * hw] = __builtin_fmaf(co, fv[ch], cs * noised[base + (long long)ch * hw]);
}

// seed[b, pix, c] += c_out[b] g[b, c, pix] for the 4 latent channels: the seed is the reverse pass's bf16 NHWC [B, hw, cpad] loss
// seed, g is fp32 NCHW; channels 4 .. cpad - 1 are left alone.  One lane per pixel, its 4 channels in one 8-byte load and store;
// fp32 arithmetic, one rounding to bf16.
__global__ void __launch_bounds__(256) seed_add_kernel(uint16_t* __restrict__ seed, const float* __restrict__ g,
                                                       const float* __restrict__ c_out, int hw, int cpad, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / hw);
  const int pix = (int)(i - (long long)b * hw);
  const float co = c_out[b];
  const float* gp = g + (long long)b * 4 * hw + pix;
  const float g0 = gp[0], g1 = gp[hw], g2 = gp[2 * (long long)hw], g3 = gp[3 * (long long)hw];
  u32x2* sp = reinterpret_cast<u32x2*>(seed + i * cpad);
  const u32x2 sv = *sp;
  const u32x2 r = {pack_bf16x2(__builtin_fmaf(co, g0, bf16_lo(sv[0])), __builtin_fmaf(co, g1, bf16_hi(sv[0]))),
                   pack_bf16x2(__builtin_fmaf(co, g2, bf16_lo(sv[1])), __builtin_fmaf(co, g3, bf16_hi(sv[1])))};
  *sp = r;
}

}  // namespace

extern "C" int udt_attn512_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                               float* lse_ws, float* dsum_ws, int32_t batch, int32_t n, int32_t ldq, int32_t ldk, int32_t ldv,
                               int32_t ldo, int32_t lddo, int32_t ldd, int64_t q_bstride, int64_t k_bstride, int64_t v_bstride,
                               int64_t o_bstride, int64_t do_bstride, int64_t d_bstride, float scale, void* stream) {
  if (!q || !k || !v || !o || !d_o || !dq || !dk || !dv || !lse_ws || !dsum_ws) return UDT_ERR_BAD_ARG;
  if (batch <= 0 || n < 1) return UDT_ERR_BAD_SHAPE;
  if (ldq % 8 != 0 || ldk % 8 != 0 || ldv % 8 != 0 || ldo % 8 != 0 || lddo % 8 != 0 || ldd % 8 != 0) return UDT_ERR_BAD_SHAPE;
  if (ldq < 512 || ldk < 512 || ldv < 512 || ldo < 512 || lddo < 512 || ldd < 512) return UDT_ERR_BAD_SHAPE;
  if ((q_bstride | k_bstride | v_bstride | o_bstride | do_bstride | d_bstride) % 8 != 0) return UDT_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o) |
       reinterpret_cast<uintptr_t>(d_o) | reinterpret_cast<uintptr_t>(dq) | reinterpret_cast<uintptr_t>(dk) |
       reinterpret_cast<uintptr_t>(dv)) & 15) return UDT_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(lse_ws) | reinterpret_cast<uintptr_t>(dsum_ws)) & 3) return UDT_ERR_BAD_ARG;
  Attn512BwdParams p;
  p.q = static_cast<const uint16_t*>(q); p.k = static_cast<const uint16_t*>(k); p.v = static_cast<const uint16_t*>(v);
  p.o = static_cast<const uint16_t*>(o); p.d_o = static_cast<const uint16_t*>(d_o);
  p.dq = static_cast<uint16_t*>(dq); p.dk = static_cast<uint16_t*>(dk); p.dv = static_cast<uint16_t*>(dv);
  p.lse = lse_ws; p.dsum = dsum_ws;
  p.n = n; p.tiles = (n + 31) / 32;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddo = lddo; p.ldd = ldd;
  p.sq = q_bstride; p.sk = k_bstride; p.sv = v_bstride; p.so = o_bstride; p.sdo = do_bstride; p.sd = d_bstride;
  p.scale = scale; p.scale_log2e = scale * 1.4426950408889634f;
  const long long units = (long long)batch * p.tiles;
  if (units > 0x7fffffffLL) return UDT_ERR_BAD_SHAPE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  static std::atomic<int> attr_done{0};
  if (!attr_done.load()) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn512_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, B5_SMEM);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(attn512_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, B5_SMEM);
    if (e != hipSuccess) return udt_set_hip_error(e);
    attr_done.store(1);
  }
  const dim3 grid((unsigned)units), blk(256);
  hipLaunchKernelGGL(attn512_bwd_kernel<false>, grid, blk, B5_SMEM, s, p);   /* LSE, D, dQ */
  UDT_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn512_bwd_kernel<true>, grid, blk, B5_SMEM, s, p);    /* dK, dV */
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_denoised_f32(const float* f, const float* noised, const float* c_skip, const float* c_out, float* out, int32_t B,
                                int32_t hw, int32_t ld, void* stream) {
  if (!f || !noised || !c_skip || !c_out || !out) return UDT_ERR_BAD_ARG;
  if (B <= 0 || hw <= 0 || ld < 4 || ld % 4 != 0) return UDT_ERR_BAD_SHAPE;
  if (reinterpret_cast<uintptr_t>(f) & 15) return UDT_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(noised) | reinterpret_cast<uintptr_t>(out)) & 3) return UDT_ERR_BAD_ARG;
  const long long total = (long long)B * hw;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(denoised_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f, noised, c_skip, c_out, out, hw, ld, total);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_seed_add_bf16(void* seed, const float* g, const float* c_out, int32_t B, int32_t hw, int32_t cpad, void* stream) {
  if (!seed || !g || !c_out) return UDT_ERR_BAD_ARG;
  if (B <= 0 || hw <= 0 || cpad < 4 || cpad % 4 != 0) return UDT_ERR_BAD_SHAPE;
  if (reinterpret_cast<uintptr_t>(seed) & 7) return UDT_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(g) & 3) return UDT_ERR_BAD_ARG;
  const long long total = (long long)B * hw;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(seed_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, static_cast<uint16_t*>(seed), g, c_out, hw,
                     cpad, total);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}
