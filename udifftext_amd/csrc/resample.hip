// resample.hip — the OCR scorer's input side: crop + antialiased bicubic resize + normalise, every box of every image in ONE launch.
//
//   udt_crop_resize_aa_f32 : test.py:81 (results[i, :, top:bottom, left:right]) + sgm/modules/predictors/model.py:24-29
//                            (torchvision Resize(BICUBIC, antialias=True) + Normalize(0.5, 0.5)), i.e. per box
//                            F.interpolate(crop[None], size, mode="bicubic", antialias=True, align_corners=False) * mul + add
//
// The resample is separable.  Along an axis of n_in input and n_out output samples, output i takes the taps
// lo <= j < hi with weight k((j - centre + 0.5) * inv) / (their sum), k the Keys cubic with a = -0.5 (ATen's value when antialiasing).
//
// Launch plan.  boxes is device data, so the grid is a function of (N, C, out_h, out_w) alone: one workgroup per
// (box, channel, 32 x 32 tile of the OUTPUT).  A box is unbounded up to the image, so neither it nor its row-resampled intermediate is
// assumed to fit in LDS: the workgroup walks the input rows its 32 output rows need in chunks of 64, resamples a chunk horizontally
// into its 32 output columns (64 x 32 fp32 = 8 KiB of LDS), and adds the chunk's share of the vertical pass to 4 accumulators per
// thread before the next chunk overwrites it.  No workspace, no host read, no allocation.
// Tap positions and the cubic are evaluated in fp64 (a tap's offset is a difference of two numbers as large as the box: in fp32 its
// cancellation error, times the cubic's slope, is larger than the whole fp32 accumulation error); the normalised weight is rounded to
// fp32 once, and products and sums are fp32.  A weight is evaluated once per 8 rows (horizontal) / once per tap (vertical).
#include "common.h"
#include "bilinear.h"

namespace {

constexpr int RS_COLS = 32;      // output columns of a workgroup's tile (the lanes of half a wave: 128-byte row segments)
constexpr int RS_ROWS = 32;      // output rows of a tile
constexpr int RS_GROUPS = 8;     // 256 threads = 32 columns x 8 row groups
constexpr int RS_CHUNK = 64;     // input rows resampled horizontally per pass
constexpr int RS_RPT = RS_CHUNK / RS_GROUPS;       // input rows per thread and chunk (8)
constexpr int RS_OPT = RS_ROWS / RS_GROUPS;        // outputs per thread (4)

struct RsAxis {                  // one axis of one box: n_in samples -> n_out
  double scale, support, inv;
};
UDT_DEVINL RsAxis rs_axis(int n_in, int n_out) {
  RsAxis a;
  a.scale = (double)n_in / (double)n_out;
  a.support = a.scale >= 1.0 ? 2.0 * a.scale : 2.0;
  a.inv = a.scale >= 1.0 ? 1.0 / a.scale : 1.0;
  return a;
}
UDT_DEVINL double rs_centre(const RsAxis& a, int i) {
#pragma clang fp contract(off)      // (the product is rounded before the support is subtracted: tap ranges as the float64 restatement)
  return a.scale * ((double)i + 0.5);
}
UDT_DEVINL int rs_lo(const RsAxis& a, double centre) { return max(0, (int)(centre - a.support + 0.5)); }
UDT_DEVINL int rs_hi(const RsAxis& a, double centre, int n_in) { return min(n_in, (int)(centre + a.support + 0.5)); }
// Keys cubic, a = -0.5
UDT_DEVINL double rs_cubic(double x) {
  const double ax = fabs(x);
  if (ax < 1.0) return (1.5 * ax - 2.5) * ax * ax + 1.0;
  if (ax < 2.0) return -0.5 * (((ax - 5.0) * ax + 8.0) * ax - 4.0);
  return 0.0;
}
// 1 / (sum of the raw weights of taps [lo, hi)); d0 = lo + 0.5 - centre
UDT_DEVINL double rs_rsum(double d0, double inv, int ntap) {
  double s = 0.0;
  for (int t = 0; t < ntap; ++t) s += rs_cubic((d0 + (double)t) * inv);
  return 1.0 / s;
}
// normalised weight of tap lo + t, rounded to fp32 once (the forward and the adjoint evaluate this one expression)
UDT_DEVINL float rs_weight(double d0, double inv, double rsum, int t) { return (float)(rs_cubic((d0 + (double)t) * inv) * rsum); }

__global__ void __launch_bounds__(256) crop_resize_aa_kernel(const float* __restrict__ img, const int32_t* __restrict__ boxes,
                                                             float* __restrict__ out, int B, int C, int H, int W, int out_h, int out_w,
                                                             int tiles_x, float mul, float add) {
  __shared__ float tmp[RS_CHUNK][RS_COLS];
  __shared__ int s_ylo[RS_ROWS], s_yhi[RS_ROWS];
  __shared__ double s_yd0[RS_ROWS], s_yrs[RS_ROWS];

  const int n = blockIdx.z, c = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lx = threadIdx.x & (RS_COLS - 1), g = threadIdx.x >> 5;
  const int ox = tx * RS_COLS + lx, oy0 = ty * RS_ROWS;

  // the box, clamped to the image and to at least one pixel: whatever boxes holds, every address read lies inside img
  const int32_t* bx = boxes + (long long)n * 5;
  const int b = min(max(bx[0], 0), B - 1);
  const int top = min(max(bx[1], 0), H - 1), bottom = min(max(bx[2], top + 1), H);
  const int left = min(max(bx[3], 0), W - 1), right = min(max(bx[4], left + 1), W);
  const int bh = bottom - top, bw = right - left;
  const float* src = img + (((long long)b * C + c) * H + top) * (long long)W + left;     // pixel (0, 0) of the box

  // vertical tap tables of the tile's 32 output rows (shared by the 32 columns)
  const RsAxis ay = rs_axis(bh, out_h);
  if (threadIdx.x < RS_ROWS) {
    const int oy = oy0 + (int)threadIdx.x;
    int lo = 0, hi = 0;
    double d0 = 0.0, rs = 0.0;
    if (oy < out_h) {
      const double cy = rs_centre(ay, oy);
      lo = rs_lo(ay, cy);
      hi = rs_hi(ay, cy, bh);
      d0 = (double)lo + 0.5 - cy;
      rs = rs_rsum(d0, ay.inv, hi - lo);
    }
    s_ylo[threadIdx.x] = lo;
    s_yhi[threadIdx.x] = hi;
    s_yd0[threadIdx.x] = d0;
    s_yrs[threadIdx.x] = rs;
  }
  // this thread's column: taps [xlo, xlo + nx) of a box row (nx = 0 for a column past out_w: it loads and stores nothing)
  const RsAxis ax = rs_axis(bw, out_w);
  int xlo = 0, nx = 0;
  double xd0 = 0.0, xrs = 0.0;
  if (ox < out_w) {
    const double cx = rs_centre(ax, ox);
    xlo = rs_lo(ax, cx);
    nx = rs_hi(ax, cx, bw) - xlo;
    xd0 = (double)xlo + 0.5 - cx;
    xrs = rs_rsum(xd0, ax.inv, nx);
  }
  __syncthreads();

  // input rows the tile needs: lo and hi grow with the output row
  const int last = min(RS_ROWS, out_h - oy0) - 1;
  const int row_begin = s_ylo[0], row_end = s_yhi[last];

  float vacc[RS_OPT];
#pragma unroll
  for (int m = 0; m < RS_OPT; ++m) vacc[m] = 0.f;

  for (int r0 = row_begin; r0 < row_end; r0 += RS_CHUNK) {
    // horizontal pass: rows r0 + g + 8 k (k = 0..7) of the box into this thread's column; a row past the tile's range repeats the
    // last one (an address inside the box) and is not read back below
    const float* rp[RS_RPT];
    float hacc[RS_RPT];
#pragma unroll
    for (int k = 0; k < RS_RPT; ++k) {
      rp[k] = src + (long long)min(r0 + g + RS_GROUPS * k, row_end - 1) * W + xlo;
      hacc[k] = 0.f;
    }
    for (int t = 0; t < nx; ++t) {
      const float w = rs_weight(xd0, ax.inv, xrs, t);
#pragma unroll
      for (int k = 0; k < RS_RPT; ++k) hacc[k] = __builtin_fmaf(w, rp[k][t], hacc[k]);
    }
#pragma unroll
    for (int k = 0; k < RS_RPT; ++k) tmp[g + RS_GROUPS * k][lx] = hacc[k];
    __syncthreads();
    // vertical pass over the chunk: output rows oy0 + g + 8 m (m = 0..3)
    const int r1 = min(r0 + RS_CHUNK, row_end);
#pragma unroll
    for (int m = 0; m < RS_OPT; ++m) {
      const int q = g + RS_GROUPS * m;
      const int lo = s_ylo[q];
      const int a = max(lo, r0), e = min(s_yhi[q], r1);
      const double d0 = s_yd0[q], rs = s_yrs[q];
      for (int r = a; r < e; ++r) {
        const float w = rs_weight(d0, ay.inv, rs, r - lo);
        vacc[m] = __builtin_fmaf(w, tmp[r - r0][lx], vacc[m]);
      }
    }
    __syncthreads();       // (the next chunk overwrites tmp)
  }

  if (ox < out_w) {
    float* dst = out + (((long long)n * C + c) * out_h) * (long long)out_w + ox;
#pragma unroll
    for (int m = 0; m < RS_OPT; ++m) {
      const int oy = oy0 + g + RS_GROUPS * m;
      if (oy < out_h) dst[(long long)oy * out_w] = __builtin_fmaf(mul, vacc[m], add);
    }
  }
}

// ---- the adjoint: d_img[b, c, y, x] = mul * sum_oy wy(oy, y - top) sum_ox wx(ox, x - left) d_out[n, c, oy, ox] for the box n of image b
// Gather form.  The taps [lo, hi) of an axis grow with the output index, so the outputs that read input sample j are one contiguous
// range [i0, i1): rs_out_range starts below it (from the real-valued inverse of the tap rule, two outputs of slack) and walks up with
// rs_lo / rs_hi themselves — the range is DEFINED by the forward's rule, not restated.
UDT_DEVINL void rs_out_range(const RsAxis& a, int n_in, int n_out, int j, int& i0, int& i1) {
  int i = (int)floor(((double)j - a.support) / a.scale - 0.5) - 2;
  i = min(max(i, 0), n_out);
  while (i < n_out && rs_hi(a, rs_centre(a, i), n_in) <= j) ++i;
  i0 = i;
  while (i < n_out && rs_lo(a, rs_centre(a, i)) <= j) ++i;
  i1 = i;
}
// weight of input sample j in output i of an axis (j inside i's taps)
UDT_DEVINL float rs_weight_of(const RsAxis& a, int n_in, int i, int j) {
  const double c = rs_centre(a, i);
  const int lo = rs_lo(a, c);
  const double d0 = (double)lo + 0.5 - c;
  return rs_weight(d0, a.inv, rs_rsum(d0, a.inv, rs_hi(a, c, n_in) - lo), j - lo);
}

constexpr int RB_COLS = 256;     // input columns of a workgroup: one row segment of one channel of one image

// Launch plan: one workgroup per (256-column segment, row y, image b * C + c) of d_img — a function of (B, C, H, W) alone.  The
// workgroup looks the image's box up in the table (the first row whose index is b; none: the segment is zero), its 256 threads
// evaluate the vertical weights of the outputs that read row y once (LDS, 256 outputs at a time), and every thread inside the box sums
// its column's outputs: per output column ox, inner = sum_oy wy d_out (ascending oy), acc += wx * inner (ascending ox).
__global__ void __launch_bounds__(RB_COLS) crop_resize_aa_bwd_kernel(const float* __restrict__ d_out, const int32_t* __restrict__ boxes,
                                                                     float* __restrict__ d_img, int B, int C, int H, int W, int N,
                                                                     int out_h, int out_w, float mul) {
  __shared__ float s_wy[RB_COLS];
  const int x = blockIdx.x * RB_COLS + (int)threadIdx.x, y = blockIdx.y;
  const int b = blockIdx.z / C, c = blockIdx.z - b * C;
  int n = -1;
  for (int i = 0; i < N; ++i)
    if (min(max(boxes[(long long)i * 5], 0), B - 1) == b) { n = i; break; }
  float* dst = d_img + (((long long)b * C + c) * H + y) * (long long)W;
  int top = 0, bottom = 0, left = 0, right = 0;
  if (n >= 0) {                                              // clamped exactly as the forward clamps it
    const int32_t* bx = boxes + (long long)n * 5;
    top = min(max(bx[1], 0), H - 1); bottom = min(max(bx[2], top + 1), H);
    left = min(max(bx[3], 0), W - 1); right = min(max(bx[4], left + 1), W);
  }
  if (n < 0 || y < top || y >= bottom) {                     // (uniform over the workgroup)
    if (x < W) dst[x] = 0.f;
    return;
  }
  const int bh = bottom - top, bw = right - left;
  const RsAxis ay = rs_axis(bh, out_h), ax = rs_axis(bw, out_w);
  int oy0, oy1;
  rs_out_range(ay, bh, out_h, y - top, oy0, oy1);
  const bool inside = x >= left && x < right;                // (x < W follows)
  int ox0 = 0, ox1 = 0;
  if (inside) rs_out_range(ax, bw, out_w, x - left, ox0, ox1);
  const float* src = d_out + ((long long)n * C + c) * out_h * (long long)out_w;
  float acc = 0.f;
  for (int c0 = oy0; c0 < oy1; c0 += RB_COLS) {
    const int cnt = min(RB_COLS, oy1 - c0);
    __syncthreads();                                         // (the previous chunk's weights are no longer read)
    if ((int)threadIdx.x < cnt) s_wy[threadIdx.x] = rs_weight_of(ay, bh, c0 + (int)threadIdx.x, y - top);
    __syncthreads();
    for (int ox = ox0; ox < ox1; ++ox) {
      const float wx = rs_weight_of(ax, bw, ox, x - left);
      float inner = 0.f;
      for (int k = 0; k < cnt; ++k) inner = __builtin_fmaf(s_wy[k], src[(long long)(c0 + k) * out_w + ox], inner);
      acc = __builtin_fmaf(wx, inner, acc);
    }
  }
  if (x < W) dst[x] = inside ? mul * acc : 0.f;
}

// ---- bilinear resize of fp32 planes (the character maps at image size: demo.py:109 cv2.resize, F.interpolate(mode="bilinear",
// align_corners=False)).  Half-pixel centres, edge clamp: output i reads source coordinate ((2 i + 1) n_in - n_out) / (2 n_out),
// clamped below at 0 — kept as that integer fraction, so the two taps are exact and the weights are the fraction rounded to fp32 once.
// (BlTap, bl_tap: bilinear.h, shared with the FID input stage)
// one thread per output element, x fastest
__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, long long total,
                                                              int h, int w, int H, int W) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % W);
  const long long rest = idx / W;
  const int oy = (int)(rest % H);
  const long long plane = rest / H;
  const BlTap ty = bl_tap(oy, h, H), tx = bl_tap(ox, w, W);
  const float* r0 = in + (plane * h + ty.i0) * (long long)w;
  const float* r1 = in + (plane * h + ty.i1) * (long long)w;
  const float top = __builtin_fmaf(tx.w1, r0[tx.i1], tx.w0 * r0[tx.i0]);
  const float bot = __builtin_fmaf(tx.w1, r1[tx.i1], tx.w0 * r1[tx.i0]);
  out[idx] = __builtin_fmaf(ty.w1, bot, ty.w0 * top);
}

}  // namespace

extern "C" int udt_resize_bilinear_f32(const float* in, float* out, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W,
                                       void* stream) {
  if (!in || !out) return UDT_ERR_BAD_ARG;
  if (planes <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return UDT_ERR_BAD_SHAPE;
  if (planes > (1LL << 40) / ((long long)H * W)) return UDT_ERR_BAD_SHAPE;                // (grid limit: 2^31 workgroups of 256)
  const long long total = (long long)planes * H * W;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, total, (int)h, (int)w,
                     (int)H, (int)W);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_crop_resize_aa_bwd_f32(const float* d_out, const int32_t* boxes, float* d_img, int B, int C, int H, int W, int N,
                                          int out_h, int out_w, float mul, void* stream) {
  if (!d_out || !boxes || !d_img) return UDT_ERR_BAD_ARG;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || N <= 0 || out_h <= 0 || out_w <= 0) return UDT_ERR_BAD_SHAPE;
  if (H > 65535 || (long long)B * C > 65535 || N > 65535) return UDT_ERR_BAD_SHAPE;      // grid limits
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(crop_resize_aa_bwd_kernel, dim3((unsigned)((W + RB_COLS - 1) / RB_COLS), (unsigned)H, (unsigned)(B * C)),
                     dim3(RB_COLS), 0, s, d_out, boxes, d_img, B, C, H, W, N, out_h, out_w, mul);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}

extern "C" int udt_crop_resize_aa_f32(const float* img, const int32_t* boxes, float* out, int B, int C, int H, int W, int N, int out_h,
                                      int out_w, float mul, float add, void* stream) {
  if (!img || !boxes || !out) return UDT_ERR_BAD_ARG;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || N <= 0 || out_h <= 0 || out_w <= 0) return UDT_ERR_BAD_SHAPE;
  const long long tiles_x = (out_w + RS_COLS - 1) / RS_COLS, tiles_y = (out_h + RS_ROWS - 1) / RS_ROWS;
  if (tiles_x * tiles_y > 0x7fffffffLL || C > 65535 || N > 65535) return UDT_ERR_BAD_SHAPE;      // grid limits
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  UdtProfScope prof(5, s);
  hipLaunchKernelGGL(crop_resize_aa_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)C, (unsigned)N), dim3(256), 0, s, img, boxes, out,
                     B, C, H, W, out_h, out_w, (int)tiles_x, mul, add);
  UDT_CHECK_LAUNCH();
  return UDT_OK;
}
