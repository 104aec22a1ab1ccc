// conv_f32.h — the fp32 implicit-GEMM convolution of csrc/lpips.hip, shared by its two entry points: udt_conv2d_f32 (lpips.hip,
// square kernels) and udt_conv2d_rect_f32 (fid.hip, kh x kw kernels with a padding per axis).  One kernel serves both, so a square
// call computes the same bits through either.
#pragma once
#include "common.h"

namespace udt_conv_f32 {

constexpr int BM = 128, BN = 64, BK = 16;                  // workgroup tile: 128 pixels x 64 channels, K in chunks of 16

struct Params {
  const float* x; const float* w; const float* bias; float* out;
  int N, H, W, Cin, ldx, Cout, ldo, kh, kw, stride, pad_h, pad_w, relu, Ho, Wo, K, Kp;
  long long M;
};

// fills Ho, Wo, K, Kp, M from the geometry already in p, checks the grid limits and launches; the caller has validated the geometry
// (every count >= 1, ld_x >= Cin, ld_out >= Cout, 0 <= pad < kernel per axis, at least one output pixel).
// UDT_ERR_BAD_SHAPE (nothing launched): more than 2^31 - 1 row tiles or more than 65535 column tiles.
int launch(Params& p, hipStream_t stream);

}  // namespace udt_conv_f32
