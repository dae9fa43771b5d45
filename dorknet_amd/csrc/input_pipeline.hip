// Device-side input pipeline (SURVEY.md section 8 f, row 4): the per-image preprocessing of
// data_loading/image_preprocessor.py:16-39 and the mixup of data_loading/image_data_loader.py:
// 101-111, for a whole batch on the GPU.  Byte / elementwise work, HBM-bound: one thread per
// output element, coalesced along the output's innermost dimension.
//
//   resize   cv2.resize(im, (OW, OH)) with INTER_LINEAR (the reference's default) for uint8:
//            OpenCV's 11-bit fixed-point algorithm (see resize_linear_u8_kernel), integer work,
//            bit-exact to oracle/pipeline.py's restatement.  cv2 is not in this image, so
//            agreement with cv2 itself is unpinned.
//   crop + cast + layout   im[r:r+OH, c:c+OW, :].astype(float32).transpose(2, 0, 1) - 128:
//            uint8 NHWC batch in, fp32 NCHW batch out (the layout the reference's X_batch has),
//            per-image crop offsets.  Exact.
//   mixup    X_mixed = p * X_m + (1 - p) * X and its mirror, for images and one-hot labels,
//            with p and 1 - p rounded to fp32 first as numpy does for a Python float times a
//            float32 array.  Exact.
//   augment  data_loading/image_augmentation.py:16-72: HSV perturbation, rotation, translation and
//            flip of a uint8 BGR batch in one pass, to uint8 NHWC or straight to fp32 NCHW (the cast
//            fused in); see augment_u8_kernel.  Bit-exact to tests/_augment_ref.py.
#include "dk_common.h"

// Built with -ffp-contract=off (__graft_entry__.EXTRA_FLAGS): every fp32 / fp64 operation is
// rounded on its own, as in the numpy restatement.

namespace dk {

// cv2.resize INTER_LINEAR for CV_8U, OpenCV 4.3 (opencv-python 4.3.0.36, the reference's pin),
// imgproc/src/resize.cpp, restated from its published algorithm:
//   scale = 1 / (O / L) (cv::resize's inv_scale, then 1/inv_scale);
//   x: fx = (float)((ox + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (sx, fx) = (0, 0);
//      sx >= L - 1 -> (sx, fx) = (L - 1, 0); weights (short) cvRound((1 - fx) * 2048), cvRound(fx * 2048)
//      (INTER_RESIZE_COEF_BITS = 11); outputs at or past the first sx + 1 >= L use src[sx] * 2048;
//   y: the same coordinate, rows sy and sy + 1 clipped to [0, H - 1], no weight clamping;
//   horizontal pass in int32: S = src[sx] * a0 + src[sx + C] * a1;
//   vertical pass FixedPtCast<int, uchar, 22>: (S0 * b0 + S1 * b1 + 2^21) >> 22, saturated to uint8;
//   an exact 2x downscale on both axes switches to INTER_AREA: (a + b + c + d + 2) >> 2 per 2x2 block;
//   the same size copies.
// Integer work, exact; the kernel and oracle/pipeline.py agree bit for bit.  OpenCV's x86 SIMD
// vertical pass (VResizeLinearVec_32s8u: >> 4, mulhi, (+2) >> 2) can round the bulk of a row
// differently in the last bit; cv2 is not installed here, so agreement with cv2 is unpinned.
struct CvAxis {
  int s0, s1;   // source indices of the two taps
  int a0, a1;   // weights (2048 = 1.0); (2048, 0) at and past the edge
};
__device__ __forceinline__ int cv_round(float v) { return (int)rintf(v); }

__device__ __forceinline__ CvAxis cv_axis_x(int o, double scale, int L) {
  float f = (float)((o + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  bool edge = false;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s + 1 >= L) {  // at or past xmax: src[sx] * ONE
    edge = true;
    if (s >= L - 1) {
      s = L - 1;
      f = 0.f;
    }
  }
  CvAxis a;
  a.s0 = s;
  a.s1 = min(s + 1, L - 1);
  if (edge) {
    a.a0 = 2048;
    a.a1 = 0;
  } else {
    a.a0 = cv_round((1.f - f) * 2048.f);
    a.a1 = cv_round(f * 2048.f);
  }
  return a;
}
__device__ __forceinline__ CvAxis cv_axis_y(int o, double scale, int L) {
  float f = (float)((o + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  CvAxis a;
  a.s0 = min(max(s, 0), L - 1);
  a.s1 = min(max(s + 1, 0), L - 1);
  a.a0 = cv_round((1.f - f) * 2048.f);
  a.a1 = cv_round(f * 2048.f);
  return a;
}

// mode 0: linear, 1: exact 2x area, 2: copy
__global__ void resize_linear_u8_kernel(const uint8_t* __restrict__ src, int N, int H, int W, int C, int OH, int OW,
                                        double scy, double scx, int mode, uint8_t* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over N * OH * OW
  if (i >= (long long)N * OH * OW) return;
  const int ox = (int)(i % OW);
  const long long t = i / OW;
  const int oy = (int)(t % OH);
  const int n = (int)(t / OH);
  const uint8_t* im = src + (size_t)n * H * W * C;
  uint8_t* out = dst + (size_t)i * C;
  if (mode == 2) {
    for (int c = 0; c < C; ++c) out[c] = im[((size_t)oy * W + ox) * C + c];
    return;
  }
  if (mode == 1) {
    const size_t p = ((size_t)(2 * oy) * W + 2 * ox) * C, q = p + (size_t)W * C;
    for (int c = 0; c < C; ++c) out[c] = (uint8_t)((im[p + c] + im[p + C + c] + im[q + c] + im[q + C + c] + 2) >> 2);
    return;
  }
  const CvAxis ax = cv_axis_x(ox, scx, W), ay = cv_axis_y(oy, scy, H);
  const uint8_t* r0 = im + (size_t)ay.s0 * W * C;
  const uint8_t* r1 = im + (size_t)ay.s1 * W * C;
  for (int c = 0; c < C; ++c) {
    const int S0 = r0[ax.s0 * C + c] * ax.a0 + r0[ax.s1 * C + c] * ax.a1;
    const int S1 = r1[ax.s0 * C + c] * ax.a0 + r1[ax.s1 * C + c] * ax.a1;
    const int v = (S0 * ay.a0 + S1 * ay.a1 + (1 << 21)) >> 22;
    out[c] = (uint8_t)min(max(v, 0), 255);
  }
}

__global__ void u8_nhwc_to_nchw_kernel(const uint8_t* __restrict__ src, int N, int H, int W, int C,
                                       const int* __restrict__ crop, int OH, int OW, float shift,
                                       float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over N * C * OH * OW (NCHW)
  if (i >= (long long)N * C * OH * OW) return;
  const int ox = (int)(i % OW);
  long long t = i / OW;
  const int oy = (int)(t % OH);
  t /= OH;
  const int c = (int)(t % C);
  const int n = (int)(t / C);
  // offsets clamped into the image (a bad offset cannot read out of bounds)
  const int r0 = crop ? min(max(crop[2 * n], 0), H - OH) : 0, c0 = crop ? min(max(crop[2 * n + 1], 0), W - OW) : 0;
  const uint8_t v = src[(((size_t)n * H + r0 + oy) * W + c0 + ox) * C + c];
  dst[i] = __fsub_rn((float)v, shift);
}

__global__ void mixup_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, float p, float q,
                             float* __restrict__ ab, float* __restrict__ ba) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i];
  ab[i] = __fadd_rn(__fmul_rn(p, y), __fmul_rn(q, x));  // p * X_m + (1 - p) * X
  ba[i] = __fadd_rn(__fmul_rn(p, x), __fmul_rn(q, y));  // p * X + (1 - p) * X_m
}

// Image augmentation (data_loading/image_augmentation.py:16-72), all four steps of the reference in one
// pass over a uint8 BGR batch; tests/_augment_ref.py restates them one after the other and pins this bit
// for bit.  For output pixel (y, x) of image n:
//   flip         x1 = flip ? W - 1 - x : x                       (im[:, ::-1, :], the last step)
//   translation  (x2, y2) = (x1 - tx, y - ty), 0 outside         (warpAffine by whole pixels: an exact
//                                                                 shifted copy with zero fill)
//   rotation     cv2.warpAffine INTER_LINEAR / BORDER_CONSTANT 0 at (x2, y2): the inverse matrix m (formed
//                on the host in double), X = (cvRound((m1 y + m2) 1024) + 16 + cvRound(m0 x 1024)) >> 5,
//                sx = X >> 5, fx = X & 31 (likewise Y), four taps weighted (32 - fx)(32 - fy) 32 ...,
//                (sum + 2^14) >> 15; a tap outside the image is 0
//   HSV          every tap inside the image is the perturbed source pixel: cvtColor BGR2HSV (uint8,
//                integer, hue range 180), three fp32 factors, clip, truncate, cvtColor HSV2BGR (fp32,
//                one rounding per operation: this file is built with -ffp-contract=off)
// One thread per output pixel, its three channels together: a wave writes 192 adjacent bytes (uint8
// NHWC out) or 256 adjacent bytes per channel plane (fp32 NCHW out).  The source is a crop window
// rows x cols at (row, col) of an H x W image, so the pipeline needs no crop copy.  blockIdx.y is the
// image (its parameters are uniform over a block), blockIdx.x * 256 + threadIdx.x the pixel within it.
struct AugParams {   // = dk_augment_params
  double m[6];
  float hsv[3];
  int tx, ty, flags;
};
static_assert(sizeof(AugParams) == sizeof(dk_augment_params), "parameter record layout");
enum : int { AUG_HSV = 1, AUG_ROTATE = 2, AUG_FLIP = 4 };

struct Bgr {
  int b, g, r;
};

// n / den rounded half to even (cvRound of the quotient: a tie is exact in double too)
__device__ __forceinline__ int div_round_even(int n, int den) {
  const int q = n / den, rem = n - q * den;
  return q + ((2 * rem > den || (2 * rem == den && (q & 1))) ? 1 : 0);
}

__device__ __forceinline__ float pick4(int k, float t0, float t1, float t2, float t3) {
  return k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3;
}

__device__ __forceinline__ int cv_sat_u8(float v) { return min(max((int)rintf(v), 0), 255); }

__device__ __forceinline__ Bgr hsv_perturb(Bgr p, const int* sdiv, const int* hdiv, float fh, float fs, float fv) {
  // BGR -> HSV, uint8
  const int v = max(max(p.b, p.g), p.r), vmin = min(min(p.b, p.g), p.r), d = v - vmin;
  const int s = (d * sdiv[v] + 2048) >> 12;
  const int h0 = v == p.r ? p.g - p.b : v == p.g ? p.b - p.r + 2 * d : p.r - p.g + 4 * d;
  int h = (h0 * hdiv[d] + 2048) >> 12;
  if (h < 0) h += 180;
  // scale in fp32, clip, truncate to uint8
  const int hi = (int)fminf(fminf(fmaxf(__fmul_rn((float)h, fh), 0.f), 255.f), 179.f);
  const int si = (int)fminf(fmaxf(__fmul_rn((float)s, fs), 0.f), 255.f);
  const int vi = (int)fminf(fmaxf(__fmul_rn((float)v, fv), 0.f), 255.f);
  // HSV -> BGR, fp32
  const float hf = __fmul_rn((float)hi, 6.f / 180.f), sf = __fmul_rn((float)si, 1.f / 255.f),
              vf = __fmul_rn((float)vi, 1.f / 255.f);
  float b = vf, g = vf, r = vf;
  if (si != 0) {
    const float sec = floorf(hf);
    float f = __fsub_rn(hf, sec);
    int k = (int)sec;
    if (k < 0 || k > 5) {
      k = 0;
      f = 0.f;
    }
    const float t0 = vf, t1 = __fmul_rn(vf, __fsub_rn(1.f, sf)), t2 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, f))),
                t3 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, __fsub_rn(1.f, f))));
    // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], two bits per sector
    const int sh = 2 * k;
    const int bsel = 1 | 1 << 2 | 3 << 4 | 0 << 6 | 0 << 8 | 2 << 10;
    const int gsel = 3 | 0 << 2 | 0 << 4 | 2 << 6 | 1 << 8 | 1 << 10;
    const int rsel = 0 | 2 << 2 | 1 << 4 | 1 << 6 | 3 << 8 | 0 << 10;
    b = pick4((bsel >> sh) & 3, t0, t1, t2, t3);
    g = pick4((gsel >> sh) & 3, t0, t1, t2, t3);
    r = pick4((rsel >> sh) & 3, t0, t1, t2, t3);
  }
  Bgr o;
  o.b = cv_sat_u8(__fmul_rn(b, 255.f));
  o.g = cv_sat_u8(__fmul_rn(g, 255.f));
  o.r = cv_sat_u8(__fmul_rn(r, 255.f));
  return o;
}

// cvRound to a 64-bit integer, clamped far outside any image (a NaN takes the low end)
__device__ __forceinline__ long long round_fix(double v) {
  const double lim = 1099511627776.0;  // 2^40
  return (long long)fmin(fmax(rint(v), -lim), lim);
}

template <bool F32>
__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ src, int N, int H, int W,
                                                         const int* __restrict__ crop, int rows, int cols,
                                                         const AugParams* __restrict__ params, float shift,
                                                         void* __restrict__ dst) {
  // the two division tables of BGR2HSV: sdiv[i] = cvRound((255 << 12) / i), hdiv[i] = cvRound((180 << 12) / 6 i)
  __shared__ int sdiv[256], hdiv[256];
  {
    const int t = threadIdx.x;  // blockDim.x == 256
    sdiv[t] = t ? div_round_even(255 << 12, t) : 0;
    hdiv[t] = t ? div_round_even(180 << 12, 6 * t) : 0;
  }
  __syncthreads();
  const int n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;  // over rows * cols (< 2^31 - 256: the entry points check)
  if (n >= N || i >= rows * cols) return;
  const int x = i % cols, y = i / cols;
  const AugParams& P = params[n];
  const int flags = P.flags;
  const float fh = P.hsv[0], fs = P.hsv[1], fv = P.hsv[2];
  // offsets clamped into the image (a bad offset cannot read out of bounds)
  const int r0 = crop ? min(max(crop[2 * n], 0), H - rows) : 0, c0 = crop ? min(max(crop[2 * n + 1], 0), W - cols) : 0;
  const uint8_t* im = src + (((size_t)n * H + r0) * W + c0) * 3;
  const size_t pitch = (size_t)W * 3;

  // the (perturbed) source pixel at (yy, xx) of the window, 0 outside it
  auto tap = [&](long long yy, long long xx) {
    Bgr p = {0, 0, 0};
    if (yy >= 0 && yy < rows && xx >= 0 && xx < cols) {
      const uint8_t* q = im + (size_t)yy * pitch + (size_t)xx * 3;
      p.b = q[0];
      p.g = q[1];
      p.r = q[2];
      if (flags & AUG_HSV) p = hsv_perturb(p, sdiv, hdiv, fh, fs, fv);
    }
    return p;
  };

  const long long x2 = (long long)((flags & AUG_FLIP) ? cols - 1 - x : x) - P.tx, y2 = (long long)y - P.ty;
  Bgr o = {0, 0, 0};
  if (x2 >= 0 && x2 < cols && y2 >= 0 && y2 < rows) {
    if (flags & AUG_ROTATE) {
      const double xd = (double)x2, yd = (double)y2;
      const long long X = (round_fix((P.m[1] * yd + P.m[2]) * 1024.0) + 16 + round_fix(P.m[0] * xd * 1024.0)) >> 5;
      const long long Y = (round_fix((P.m[4] * yd + P.m[5]) * 1024.0) + 16 + round_fix(P.m[3] * xd * 1024.0)) >> 5;
      // clamped next to the window: a tap that far out is 0 either way
      const long long sx = min(max(X >> 5, -2LL), (long long)cols), sy = min(max(Y >> 5, -2LL), (long long)rows);
      const int fx = (int)(X & 31), fy = (int)(Y & 31);
      const Bgr a = tap(sy, sx), b = tap(sy, sx + 1), c = tap(sy + 1, sx), d = tap(sy + 1, sx + 1);
      const int wa = (32 - fx) * (32 - fy) * 32, wb = fx * (32 - fy) * 32, wc = (32 - fx) * fy * 32, wd = fx * fy * 32;
      o.b = (a.b * wa + b.b * wb + c.b * wc + d.b * wd + 16384) >> 15;
      o.g = (a.g * wa + b.g * wb + c.g * wc + d.g * wd + 16384) >> 15;
      o.r = (a.r * wa + b.r * wb + c.r * wc + d.r * wd + 16384) >> 15;
    } else {
      o = tap(y2, x2);
    }
  }
  if constexpr (F32) {
    float* out = (float*)dst + ((size_t)n * 3 * rows + y) * cols + x;  // NCHW
    const size_t plane = (size_t)rows * cols;
    out[0] = __fsub_rn((float)o.b, shift);
    out[plane] = __fsub_rn((float)o.g, shift);
    out[2 * plane] = __fsub_rn((float)o.r, shift);
  } else {
    uint8_t* out = (uint8_t*)dst + ((size_t)n * rows * cols + i) * 3;  // NHWC
    out[0] = (uint8_t)o.b;
    out[1] = (uint8_t)o.g;
    out[2] = (uint8_t)o.r;
  }
}

// Device-resident image store: decoded uint8 HWC images of differing sizes back
// to back in one buffer, one record per image; a batch is an int32 table of (image, crop row, crop col).
// store_pixel is the one source-pixel function of every store entry: the pixel at (crop_row + oy,
// crop_col + ox) of that image resized to TH x TW -- what resize_linear_u8_kernel followed by the crop
// gives, computed for the crop window only.  The resize mode is per image: blockIdx.y is the image, so a
// block never diverges on it.
struct StoreImage {   // = dk_store_image
  long long offset;   // bytes from the start of the store
  int H, W;
};
static_assert(sizeof(StoreImage) == sizeof(dk_store_image), "store record layout");

struct Px4 {
  int v[4];   // channels past C are 0
};

__device__ __forceinline__ Px4 store_pixel(const uint8_t* __restrict__ data, const StoreImage* __restrict__ images,
                                           int count, int C, const int* __restrict__ rec, int TH, int TW, int OH,
                                           int OW, int oy, int ox) {
  // a bad table cannot read out of bounds: the image index and the crop offsets are clamped
  const StoreImage im = images[min(max(rec[0], 0), count - 1)];
  const int y = min(max(rec[1], 0), TH - OH) + oy, x = min(max(rec[2], 0), TW - OW) + ox;
  const int H = im.H, W = im.W;
  const uint8_t* src = data + im.offset;   // 64-bit: the store is meant to exceed 4 GB
  const size_t pitch = (size_t)W * C;
  Px4 o = {{0, 0, 0, 0}};
  if (H == TH && W == TW) {  // copy
    const uint8_t* p = src + (size_t)y * pitch + (size_t)x * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o.v[c] = p[c];
  } else if (H == 2 * TH && W == 2 * TW) {  // INTER_AREA for the exact 2x downscale of both axes
    const uint8_t* p = src + (size_t)(2 * y) * pitch + (size_t)(2 * x) * C;
    const uint8_t* q = p + pitch;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) o.v[c] = (p[c] + p[C + c] + q[c] + q[C + c] + 2) >> 2;
  } else {
    // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale, from this image's own size
    const double scy = 1.0 / ((double)TH / (double)H), scx = 1.0 / ((double)TW / (double)W);
    const CvAxis ax = cv_axis_x(x, scx, W), ay = cv_axis_y(y, scy, H);
    const uint8_t* r0 = src + (size_t)ay.s0 * pitch;
    const uint8_t* r1 = src + (size_t)ay.s1 * pitch;
    const size_t x0 = (size_t)ax.s0 * C, x1 = (size_t)ax.s1 * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        const int S0 = r0[x0 + c] * ax.a0 + r0[x1 + c] * ax.a1;
        const int S1 = r1[x0 + c] * ax.a0 + r1[x1 + c] * ax.a1;
        o.v[c] = min(max((S0 * ay.a0 + S1 * ay.a1 + (1 << 21)) >> 22, 0), 255);
      }
  }
  return o;
}

// OUT 0: uint8 NHWC [N][OH][OW][C] (the cropped image, for the augmenter); 1: fp32 NCHW [N][C][OH][OW];
// 2: bf16 channels-last [N][OH][OW][C], round-to-nearest-even of the fp32 value.  OUT 1 / 2: pixel - shift;
// with a partner table also the partner image's value xm, ab = p * xm + q * x and ba = p * x + q * xm,
// every product and sum rounded on its own as in mixup_kernel.  One thread per output pixel, all channels.
template <int OUT>
__global__ __launch_bounds__(256) void store_batch_kernel(const uint8_t* __restrict__ data,
                                                          const StoreImage* __restrict__ images, int count, int C,
                                                          const int* __restrict__ batch,
                                                          const int* __restrict__ partner, int N, int TH, int TW,
                                                          int OH, int OW, float shift, float p, float q,
                                                          void* __restrict__ ab, void* __restrict__ ba) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;  // over OH * OW (< 2^31 - 256: the entry points check)
  if (n >= N || i >= OH * OW) return;
  const int ox = i % OW, oy = i / OW;
  const Px4 a = store_pixel(data, images, count, C, batch + 3 * (size_t)n, TH, TW, OH, OW, oy, ox);
  if constexpr (OUT == 0) {
    uint8_t* out = (uint8_t*)ab + ((size_t)n * OH * OW + i) * C;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) out[c] = (uint8_t)a.v[c];
  } else {
    float x[4], y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = __fsub_rn((float)a.v[c], shift);
    const bool mix = partner != nullptr;
    if (mix) {
      const Px4 b = store_pixel(data, images, count, C, partner + 3 * (size_t)n, TH, TW, OH, OW, oy, ox);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float xm = __fsub_rn((float)b.v[c], shift);
        y[c] = __fadd_rn(__fmul_rn(p, x[c]), __fmul_rn(q, xm));   // p * X + (1 - p) * X_m
        x[c] = __fadd_rn(__fmul_rn(p, xm), __fmul_rn(q, x[c]));   // p * X_m + (1 - p) * X
      }
    }
    const size_t plane = (size_t)OH * OW;
    const size_t e = OUT == 1 ? (size_t)n * C * plane + i : ((size_t)n * plane + i) * C;
    const size_t step = OUT == 1 ? plane : 1;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) {
        if constexpr (OUT == 1) {
          ((float*)ab)[e + c * step] = x[c];
          if (mix) ((float*)ba)[e + c * step] = y[c];
        } else {
          st1((bf16_t*)ab + e + c * step, x[c]);
          if (mix) st1((bf16_t*)ba + e + c * step, y[c]);
        }
      }
  }
}

// One-hot rows of a batch's labels, mixed with the partner batch's as the images are:
// y_ab[n][c] = p * [c == lm] + q * [c == l] and its mirror; without a partner the plain one-hot row.
// A label outside [0, classes) matches no column: a zero row.
__global__ void onehot_mixup_kernel(const int* __restrict__ labels, const int* __restrict__ partner, long long total,
                                    int classes, float p, float q, float* __restrict__ y_ab,
                                    float* __restrict__ y_ba) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over N * classes
  if (i >= total) return;
  const int c = (int)(i % classes);
  const long long n = i / classes;
  const float e = labels[n] == c ? 1.f : 0.f;
  if (!partner) {
    y_ab[i] = e;
    return;
  }
  const float em = partner[n] == c ? 1.f : 0.f;
  y_ab[i] = __fadd_rn(__fmul_rn(p, em), __fmul_rn(q, e));
  y_ba[i] = __fadd_rn(__fmul_rn(p, e), __fmul_rn(q, em));
}

}  // namespace dk

using namespace dk;

static inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

DK_API int dk_resize_bilinear_u8(const uint8_t* src, int N, int H, int W, int C, int OH, int OW, uint8_t* dst,
                                 void* stream) {
  if (!src || !dst || N < 1 || H < 1 || W < 1 || C < 1 || OH < 1 || OW < 1) return DK_ERR_ARGS;
  // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale
  const double scy = 1.0 / ((double)OH / (double)H), scx = 1.0 / ((double)OW / (double)W);
  const int iy = (int)rint(scy), ix = (int)rint(scx);
  const double eps = 2.220446049250313e-16;  // DBL_EPSILON
  const bool area2 = fabs(scx - ix) < eps && fabs(scy - iy) < eps && ix == 2 && iy == 2;
  const int mode = (OH == H && OW == W) ? 2 : area2 ? 1 : 0;
  hipLaunchKernelGGL(resize_linear_u8_kernel, dim3(blocks256((long long)N * OH * OW)), dim3(256), 0,
                     as_stream(stream), src, N, H, W, C, OH, OW, scy, scx, mode, dst);
  return launch_status();
}

DK_API int dk_u8_nhwc_to_nchw_f32(const uint8_t* src, int N, int H, int W, int C, const int* crop_rc, int OH, int OW,
                                  float shift, float* dst, void* stream) {
  if (!src || !dst || N < 1 || C < 1 || OH < 1 || OW < 1 || OH > H || OW > W) return DK_ERR_ARGS;
  hipLaunchKernelGGL(u8_nhwc_to_nchw_kernel, dim3(blocks256((long long)N * C * OH * OW)), dim3(256), 0,
                     as_stream(stream), src, N, H, W, C, crop_rc, OH, OW, shift, dst);
  return launch_status();
}

DK_API int dk_mixup_f32(const float* a, const float* b, long long n, float p, float one_minus_p, float* ab, float* ba,
                        void* stream) {
  if (!a || !b || !ab || !ba || n < 0) return DK_ERR_ARGS;
  if (n == 0) return 0;
  hipLaunchKernelGGL(mixup_kernel, dim3(blocks256(n)), dim3(256), 0, as_stream(stream), a, b, n, p, one_minus_p, ab,
                     ba);
  return launch_status();
}

static inline bool augment_args_ok(const void* src, int N, int H, int W, int C, int OH, int OW, const void* params,
                                   const void* dst) {
  return src && dst && params && N >= 1 && C == 3 && OH >= 1 && OW >= 1 && OH <= H && OW <= W &&
         (long long)OH * OW <= 0x7fffffffLL - 256;  // the kernel's 32-bit pixel index
}

// grid.y is the image (at most 65535 per launch: larger batches take several launches)
template <bool F32>
static int launch_augment(const uint8_t* src, int N, int H, int W, const int* crop_rc, int OH, int OW,
                          const dk_augment_params* params, float shift, void* dst, void* stream) {
  const int kMaxY = 65535;
  const size_t out_image = (size_t)OH * OW * 3 * (F32 ? sizeof(float) : 1);
  for (int n0 = 0; n0 < N; n0 += kMaxY) {
    const int nb = N - n0 < kMaxY ? N - n0 : kMaxY;
    hipLaunchKernelGGL(augment_u8_kernel<F32>, dim3(blocks256((long long)OH * OW), nb), dim3(256), 0, as_stream(stream),
                       src + (size_t)n0 * H * W * 3, nb, H, W, crop_rc ? crop_rc + 2 * (size_t)n0 : nullptr, OH, OW,
                       reinterpret_cast<const AugParams*>(params) + n0, shift,
                       (void*)((uint8_t*)dst + (size_t)n0 * out_image));
  }
  return launch_status();
}

DK_API int dk_augment_u8(const uint8_t* src, int N, int H, int W, int C, const int* crop_rc, int OH, int OW,
                         const dk_augment_params* params, uint8_t* dst, void* stream) {
  if (!augment_args_ok(src, N, H, W, C, OH, OW, params, dst)) return DK_ERR_ARGS;
  return launch_augment<false>(src, N, H, W, crop_rc, OH, OW, params, 0.f, dst, stream);
}

DK_API int dk_augment_u8_to_nchw_f32(const uint8_t* src, int N, int H, int W, int C, const int* crop_rc, int OH, int OW,
                                     const dk_augment_params* params, float shift, float* dst, void* stream) {
  if (!augment_args_ok(src, N, H, W, C, OH, OW, params, dst)) return DK_ERR_ARGS;
  return launch_augment<true>(src, N, H, W, crop_rc, OH, OW, params, shift, dst, stream);
}

static inline bool store_args_ok(const void* data, const void* images, int count, int C, const void* batch, int N,
                                 int TH, int TW, int OH, int OW, const void* dst) {
  return data && images && batch && dst && count >= 1 && N >= 1 && C >= 1 && C <= 4 && OH >= 1 && OW >= 1 &&
         OH <= TH && OW <= TW && (long long)OH * OW <= 0x7fffffffLL - 256;  // the kernel's 32-bit pixel index
}

// grid.y is the output image (at most 65535 per launch: larger batches take several launches)
template <int OUT>
static int launch_store(const uint8_t* data, const dk_store_image* images, int count, int C, const int* batch,
                        const int* partner, int N, int TH, int TW, int OH, int OW, float shift, float p, float q,
                        void* ab, void* ba, void* stream) {
  const int kMaxY = 65535;
  const size_t out_image = (size_t)OH * OW * C * (OUT == 1 ? sizeof(float) : OUT == 2 ? sizeof(bf16_t) : 1);
  for (int n0 = 0; n0 < N; n0 += kMaxY) {
    const int nb = N - n0 < kMaxY ? N - n0 : kMaxY;
    hipLaunchKernelGGL(store_batch_kernel<OUT>, dim3(blocks256((long long)OH * OW), nb), dim3(256), 0,
                       as_stream(stream), data, reinterpret_cast<const StoreImage*>(images), count, C,
                       batch + 3 * (size_t)n0, partner ? partner + 3 * (size_t)n0 : nullptr, nb, TH, TW, OH, OW, shift,
                       p, q, (void*)((uint8_t*)ab + (size_t)n0 * out_image),
                       ba ? (void*)((uint8_t*)ba + (size_t)n0 * out_image) : nullptr);
  }
  return launch_status();
}

DK_API int dk_store_crop_u8(const uint8_t* data, const dk_store_image* images, int count, int C, const int* batch,
                            int N, int TH, int TW, int OH, int OW, uint8_t* dst, void* stream) {
  if (!store_args_ok(data, images, count, C, batch, N, TH, TW, OH, OW, dst)) return DK_ERR_ARGS;
  return launch_store<0>(data, images, count, C, batch, nullptr, N, TH, TW, OH, OW, 0.f, 0.f, 0.f, dst, nullptr,
                         stream);
}

DK_API int dk_store_batch_nchw_f32(const uint8_t* data, const dk_store_image* images, int count, int C,
                                   const int* batch, const int* partner, int N, int TH, int TW, int OH, int OW,
                                   float shift, float p, float one_minus_p, float* ab, float* ba, void* stream) {
  if (!store_args_ok(data, images, count, C, batch, N, TH, TW, OH, OW, ab) || (partner && !ba)) return DK_ERR_ARGS;
  return launch_store<1>(data, images, count, C, batch, partner, N, TH, TW, OH, OW, shift, p, one_minus_p, ab,
                         partner ? ba : nullptr, stream);
}

DK_API int dk_store_batch_nhwc_bf16(const uint8_t* data, const dk_store_image* images, int count, int C,
                                    const int* batch, const int* partner, int N, int TH, int TW, int OH, int OW,
                                    float shift, float p, float one_minus_p, uint16_t* ab, uint16_t* ba,
                                    void* stream) {
  if (!store_args_ok(data, images, count, C, batch, N, TH, TW, OH, OW, ab) || (partner && !ba)) return DK_ERR_ARGS;
  return launch_store<2>(data, images, count, C, batch, partner, N, TH, TW, OH, OW, shift, p, one_minus_p, ab,
                         partner ? ba : nullptr, stream);
}

DK_API int dk_onehot_mixup_f32(const int* labels, const int* partner, int N, int classes, float p, float one_minus_p,
                               float* y_ab, float* y_ba, void* stream) {
  if (!labels || !y_ab || N < 1 || classes < 1 || (partner && !y_ba)) return DK_ERR_ARGS;
  const long long total = (long long)N * classes;
  hipLaunchKernelGGL(onehot_mixup_kernel, dim3(blocks256(total)), dim3(256), 0, as_stream(stream), labels, partner,
                     total, classes, p, one_minus_p, y_ab, y_ba);
  return launch_status();
}
