// bilinear.h — the one coordinate rule of the library's bilinear resizes (udt_resize_bilinear_f32, udt_fid_input_f32):
// F.interpolate(mode="bilinear", align_corners=False).  Half-pixel centres, edge clamp: output i reads source coordinate
// ((2 i + 1) n_in - n_out) / (2 n_out), clamped below at 0 — kept as that integer fraction, so the two taps are exact and the
// weights are the fraction rounded to fp32 once.
#pragma once
#include "common.h"

struct BlTap { int i0, i1; float w0, w1; };
UDT_DEVINL BlTap bl_tap(int i, int n_in, int n_out) {
  const long long den = 2LL * n_out;
  long long num = (2LL * i + 1) * n_in - n_out;
  if (num < 0) num = 0;
  const long long q = num / den, r = num - q * den;
  BlTap t;
  t.i0 = (int)min(q, (long long)(n_in - 1));
  t.i1 = min(t.i0 + 1, n_in - 1);
  t.w1 = (float)((double)r / (double)den);
  t.w0 = (float)((double)(den - r) / (double)den);
  return t;
}
