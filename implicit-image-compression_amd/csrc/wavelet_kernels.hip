// wavelet_kernels.hip — the image-space composition of WaveletSiren (reference: implicit_image/models/wavelet_siren.py)
// and its adjoint, fp32, fixed summation order, no atomics.
//
// A WaveletSiren handle runs two SIREN sub-networks on the same n x n coefficient grid (n = (H + 5) / 2, the db3 / zero
// coefficient length of an H x H image).  LF predicts (Y_LL, Cb, Cr), HF predicts the detail bands (LH, HL, HH), both as
// p = z / 2 + 1 / 2.  The image is
//   Y      = inverse DWT (db3, mode "zero", pytorch_wavelets' SFB2D) of (LL, LH, HL, HH)             H x H
//   Cb, Cr = F.interpolate(LF[..., 1:3], scale_factor = H / n, mode="bilinear", align_corners=False)   H x H
//   RGB    = kornia's ycbcr_to_rgb: r = y + 1.403 (cr - 1/2), g = y - 0.714 (cr - 1/2) - 0.344 (cb - 1/2),
//            b = y + 1.773 (cb - 1/2)
// and the loss is mean((RGB - img)^2) over 3 H^2 values.
//
//   k_wv_compose   one thread per output pixel: prediction, residual, per-workgroup SSE partial and the image-space
//                  gradient dL/d(Y, Cb, Cr) (the colour transform's adjoint folded in)
//   k_wv_compose_eval  (sf_eval) the same pixel body with no prediction and no gradient store: the SSE partial and the
//                  exact integer partial of the 8-bit figure
//   k_wv_adjoint   one thread per coefficient (i, j): transposed synthesis taps over dL/dY, transposed bilinear
//                  footprint over dL/dCb, dL/dCr; the result times 1/2 (p = z/2 + 1/2) times the sub-networks' fp16
//                  pre-scale goes straight into each sub-network's dL/dout (Dlast, F-layout) or, when the coefficient
//                  grid takes more than one chunk, into an fp32 buffer
//   k_wv_inject    two-pass form: one chunk of that fp32 buffer -> Dlast
//   k_wv_render    (wavelet_render.hip) the inference form of k_wv_compose: a pixel window, fp32 and / or bytes, no loss
// With a sine output layer (outermost_linear=False) dL/dout is dL/dz of the last pre-activation: the sub-networks' training
// forward writes d sin(om z)/dz = om cos(om z) per coefficient and channel (FwdArgs::dfac), and k_wv_adjoint (one chunk) or
// k_wv_inject (two passes) multiplies by it before the single fp16 rounding.  The two-pass buffer holds dL/dp times dscale.
//
// Synthesis (pytorch_wavelets lowlevel.sfb1d, zero mode): per axis y[o] = sum_i lo[i] g0[o + 4 - 2 i] + hi[i] g1[o + 4 - 2 i]
// over 0 <= o + 4 - 2 i < 6 (conv_transpose with stride 2, padding L - 2 = 4), the column filter along the height first.
// For an even H every output row o reads the three coefficient rows i = o/2 .. o/2 + 2 (all inside [0, n)), with taps
// (o & 1) + 4, (o & 1) + 2, (o & 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace sf {

constexpr int kWvThreads = 256;

// db3 reconstruction filters as pytorch_wavelets holds them (pywt.Wavelet("db3").rec_lo / rec_hi rounded to fp32;
// tests/golden/wavelet_idwt.npz pins them)
__constant__ float kWvG0[6] = {0.33267055295008263f, 0.8068915093110925f, 0.45987750211849154f, -0.13501102001025458f,
                               -0.08544127388202666f, 0.03522629188570953f};
__constant__ float kWvG1[6] = {0.03522629188570953f, 0.08544127388202666f, -0.13501102001025458f, -0.45987750211849154f,
                               0.8068915093110925f, -0.33267055295008263f};

struct WvArgs {
  int H;                 // image side (even)
  int n;                 // coefficient side, H / 2 + 2
  float up;              // bilinear source-index scale: (float)(1.0 / (H / n)), torch's area_pixel_compute_scale
  const float* lf;       // [n*n][3] LF prediction p: Y_LL, Cb, Cr
  const float* hf;       // [n*n][3] HF prediction p: LH, HL, HH
  const float* img;      // [H*H][3] target (null: no residual)
  float* pred;           // [H*H][3] RGB prediction (null: not written)
  float* g;              // [H*H][3] dL/d(Y, Cb, Cr) (null: not written)
  float* sse_part;       // [gridDim.x of k_wv_compose]
  float gscale;          // d mean / d rgb = 2 / (3 H^2)
  float dscale;          // 1/2 (p = z/2 + 1/2) times the sub-networks' gradient pre-scale
  u32x4* dl_lf;          // single chunk: Dlast of LF / HF (F-layout, 16-bit float, two k-steps per 32-pixel block)
  u32x4* dl_hf;
  float* gl_lf;          // two-pass: [n*n][3] fp32 dL/dout (already scaled by dscale) of LF / HF
  float* gl_hf;
  const float* dfac_lf;  // one chunk, sine output layer: [n*n][3] d sin(om z)/dz of LF / HF (null: linear output)
  const float* dfac_hf;
};

// torch's bilinear source index (upsample_bilinear2d, align_corners=False): the same arithmetic serves the forward and,
// through wv_bilinear_weight, the adjoint, so that the adjoint is exactly the transpose
struct WvTap {
  int i0, i1;            // source rows / columns (i1 = i0 + 1, or i0 at the last one)
  float l0, l1;          // their weights
};
__device__ __forceinline__ WvTap wv_tap(int o, float up, int n) {
  float s = __fsub_rn(__fmul_rn(up, __fadd_rn((float)o, 0.5f)), 0.5f);
  if (s < 0.f) s = 0.f;
  WvTap t;
  t.i0 = (int)s;
  t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
  t.l1 = __fsub_rn(s, (float)t.i0);
  t.l0 = __fsub_rn(1.0f, t.l1);
  return t;
}
// weight of source index i in output o's footprint (both taps count when they coincide at the border)
__device__ __forceinline__ float wv_bilinear_weight(int o, int i, float up, int n) {
  const WvTap t = wv_tap(o, up, n);
  return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

__device__ __forceinline__ uint32_t wv_pack_f16(float a, float b) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  f2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, h2));
}

// One output pixel of the composition: RGB of pixel (r, c) of the H x H picture, stored at pred[p] (when given); with a
// target, the squared residual (returned) and dL/d(Y, Cb, Cr) at g[p] (when given).  lf / hf hold the coefficient rows
// [i0, ..) x columns [j0, ..) in rows of cc coefficients (the whole grid: i0 = j0 = 0, cc = n); n and up are those of the
// full picture.
// This is the body k_wv_compose and k_wv_render (wavelet_render.hip) share, and it is NOT inlined, on purpose: hipcc
// contracts a * b + c into fma and pairs operations into packed instructions depending on the code around them, and two
// inlined copies of the same expressions came out of the two kernels with different roundings (the render prediction
// differed from sf_forward's in the last bit).  One compiled body called by both is bit-identical by construction; the
// four values come back in registers.
struct WvPixel { float rgb[3]; float sse; };
__device__ __noinline__ WvPixel wv_compose_pixel(const float* lf, const float* hf, const float* img, float* pred, float* g,
                                                 float gscale, long p, int r, int c, int n, float up, int i0, int j0, int cc) {
  WvPixel out;
  float (&rgb)[3] = out.rgb;
  float sse = 0.f;
  // inverse DWT, gather form: 3 x 3 coefficients per band
  float y = 0.f;
#pragma unroll
  for (int ar = 0; ar < 3; ++ar) {
    const int i = (r >> 1) + ar - i0, kr = (r & 1) + 4 - 2 * ar;
    const float g0r = kWvG0[kr], g1r = kWvG1[kr];
    const float* lrow = lf + (size_t)i * cc * 3;
    const float* hrow = hf + (size_t)i * cc * 3;
#pragma unroll
    for (int ac = 0; ac < 3; ++ac) {
      const int j = (c >> 1) + ac - j0, kc = (c & 1) + 4 - 2 * ac;
      const float g0c = kWvG0[kc], g1c = kWvG1[kc];
      y += lrow[j * 3 + 0] * (g0r * g0c) + hrow[j * 3 + 0] * (g1r * g0c) + hrow[j * 3 + 1] * (g0r * g1c) +
           hrow[j * 3 + 2] * (g1r * g1c);
    }
  }
  // Cb, Cr: bilinear upsampling of LF channels 1, 2 (torch's operation order)
  const WvTap tr = wv_tap(r, up, n), tc = wv_tap(c, up, n);
  const float* q00 = lf + ((size_t)(tr.i0 - i0) * cc + (tc.i0 - j0)) * 3;
  const float* q01 = lf + ((size_t)(tr.i0 - i0) * cc + (tc.i1 - j0)) * 3;
  const float* q10 = lf + ((size_t)(tr.i1 - i0) * cc + (tc.i0 - j0)) * 3;
  const float* q11 = lf + ((size_t)(tr.i1 - i0) * cc + (tc.i1 - j0)) * 3;
  const float cb = tr.l0 * (tc.l0 * q00[1] + tc.l1 * q01[1]) + tr.l1 * (tc.l0 * q10[1] + tc.l1 * q11[1]);
  const float cr = tr.l0 * (tc.l0 * q00[2] + tc.l1 * q01[2]) + tr.l1 * (tc.l0 * q10[2] + tc.l1 * q11[2]);
  const float cbs = cb - 0.5f, crs = cr - 0.5f;
  rgb[0] = y + 1.403f * crs;
  rgb[1] = y - 0.714f * crs - 0.344f * cbs;
  rgb[2] = y + 1.773f * cbs;
  if (pred) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pred[p * 3 + k] = rgb[k];
  }
  if (img) {
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float e = rgb[k] - img[p * 3 + k];
      sse += e * e;
      d[k] = e * gscale;
    }
    if (g) {   // adjoint of the colour transform: dY, dCb, dCr
      g[p * 3 + 0] = d[0] + d[1] + d[2];
      g[p * 3 + 1] = 1.773f * d[2] - 0.344f * d[1];
      g[p * 3 + 2] = 1.403f * d[0] - 0.714f * d[1];
    }
  }
  out.sse = sse;
  return out;
}

__global__ __launch_bounds__(kWvThreads) void k_wv_compose(WvArgs a) {
  __shared__ float sRed[kWvThreads / 64];
  const long p = (long)blockIdx.x * kWvThreads + threadIdx.x;
  const int H = a.H, n = a.n;
  float sse = 0.f;
  if (p < (long)H * H) {
    const int r = (int)(p / H), c = (int)(p - (long)r * H);
    sse = wv_compose_pixel(a.lf, a.hf, a.img, a.pred, a.g, a.gscale, p, r, c, n, a.up, 0, 0, n).sse;
  }
  // workgroup SSE partial, fixed order: lanes by xor-shuffle, then waves 0..3
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sse += __shfl_xor(sse, o);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = sse;
  __syncthreads();
  if (threadIdx.x == 0 && a.sse_part) {
    float t = 0.f;
    for (int w = 0; w < kWvThreads / 64; ++w) t += sRed[w];
    a.sse_part[blockIdx.x] = t;
  }
}

// The EVAL form of k_wv_compose (sf_eval): the same compiled pixel body with no prediction and no gradient store, its SSE
// partial in the same order, and beside it the workgroup's integer partial of the 8-bit figure (eval_sq8 of the composed RGB
// the body returns, siren_kernels.hip).  A kernel of its own and not a template argument: k_wv_compose keeps its name
__global__ __launch_bounds__(kWvThreads) void k_wv_compose_eval(WvArgs a, unsigned long long* sse8_part) {
  __shared__ __attribute__((aligned(8))) float sRed[2 * (kWvThreads / 64)];   // (then the waves' 64-bit partials)
  const long p = (long)blockIdx.x * kWvThreads + threadIdx.x;
  const int H = a.H, n = a.n;
  float sse = 0.f;
  unsigned long long s8 = 0;
  if (p < (long)H * H) {
    const int r = (int)(p / H), c = (int)(p - (long)r * H);
    const WvPixel px = wv_compose_pixel(a.lf, a.hf, a.img, nullptr, nullptr, a.gscale, p, r, c, n, a.up, 0, 0, n);
    sse = px.sse;
#pragma unroll
    for (int k = 0; k < 3; ++k) s8 += eval_sq8(a.img[p * 3 + k], px.rgb[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sse += __shfl_xor(sse, o);
  if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = sse;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kWvThreads / 64; ++w) t += sRed[w];
    a.sse_part[blockIdx.x] = t;
  }
  eval_block_partial<kWvThreads / 64>(s8, sRed, sse8_part + blockIdx.x);
}

// dL/dout of one coefficient into a sub-network's Dlast: lane m of k-step 0 of block q / 32 (neurons 0..2 of lane half 0);
// every other element of the two pieces is the zero the training forward (no target) wrote there
__device__ __forceinline__ void wv_store_dlast(u32x4* dl, long q, float d0, float d1, float d2) {
  const long pb = q >> 5;
  const int m = (int)(q & 31);
  dl[(pb * 2) * 64 + m] = u32x4{wv_pack_f16(d0, d1), wv_pack_f16(d2, 0.f), 0u, 0u};
}

__global__ __launch_bounds__(kWvThreads) void k_wv_adjoint(WvArgs a) {
  const long q = (long)blockIdx.x * kWvThreads + threadIdx.x;
  const int H = a.H, n = a.n;
  if (q >= (long)n * n) return;
  const int i = (int)(q / n), j = (int)(q - (long)i * n);
  // synthesis adjoint: output rows r = 2 i - 4 + kr, columns c = 2 j - 4 + kc, inside the image
  float dll = 0.f, dlh = 0.f, dhl = 0.f, dhh = 0.f;
  const int kr0 = 4 - 2 * i > 0 ? 4 - 2 * i : 0, kr1 = H + 4 - 2 * i < 6 ? H + 4 - 2 * i : 6;
  const int kc0 = 4 - 2 * j > 0 ? 4 - 2 * j : 0, kc1 = H + 4 - 2 * j < 6 ? H + 4 - 2 * j : 6;
  for (int kr = kr0; kr < kr1; ++kr) {
    const int r = 2 * i - 4 + kr;
    const float* grow = a.g + (size_t)r * H * 3;
    float s0 = 0.f, s1 = 0.f;   // the row's sums against g0 / g1 along the width
    for (int kc = kc0; kc < kc1; ++kc) {
      const float gy = grow[(size_t)(2 * j - 4 + kc) * 3];
      s0 += gy * kWvG0[kc];
      s1 += gy * kWvG1[kc];
    }
    dll += kWvG0[kr] * s0;
    dlh += kWvG1[kr] * s0;
    dhl += kWvG0[kr] * s1;
    dhh += kWvG1[kr] * s1;
  }
  // bilinear adjoint: the output rows / columns whose footprint holds i / j.  The source index is monotone in the output
  // index, and these bounds (two outputs of margin on either side) contain every such output; the weight itself comes
  // from wv_tap, the forward's own arithmetic
  const float inv = 1.0f / a.up;
  int r0 = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 2, r1 = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2;
  int c0 = (int)floorf(((float)j - 0.5f) * inv - 0.5f) - 2, c1 = (int)ceilf(((float)j + 1.5f) * inv - 0.5f) + 2;
  r0 = r0 < 0 ? 0 : r0; c0 = c0 < 0 ? 0 : c0;
  r1 = r1 > H - 1 ? H - 1 : r1; c1 = c1 > H - 1 ? H - 1 : c1;
  float dcb = 0.f, dcr = 0.f;
  for (int r = r0; r <= r1; ++r) {
    const float wr = wv_bilinear_weight(r, i, a.up, n);
    if (wr == 0.f) continue;
    const float* grow = a.g + (size_t)r * H * 3;
    float sb = 0.f, sr = 0.f;
    for (int c = c0; c <= c1; ++c) {
      const float wc = wv_bilinear_weight(c, j, a.up, n);
      if (wc == 0.f) continue;
      sb += wc * grow[(size_t)c * 3 + 1];
      sr += wc * grow[(size_t)c * 3 + 2];
    }
    dcb += wr * sb;
    dcr += wr * sr;
  }
  const float s = a.dscale;
  if (a.dl_lf && a.dfac_lf) {
    const float* fl = a.dfac_lf + q * 3;
    const float* fh = a.dfac_hf + q * 3;
    wv_store_dlast(a.dl_lf, q, dll * s * fl[0], dcb * s * fl[1], dcr * s * fl[2]);
    wv_store_dlast(a.dl_hf, q, dlh * s * fh[0], dhl * s * fh[1], dhh * s * fh[2]);
  } else if (a.dl_lf) {
    wv_store_dlast(a.dl_lf, q, dll * s, dcb * s, dcr * s);
    wv_store_dlast(a.dl_hf, q, dlh * s, dhl * s, dhh * s);
  } else {
    a.gl_lf[q * 3 + 0] = dll * s; a.gl_lf[q * 3 + 1] = dcb * s; a.gl_lf[q * 3 + 2] = dcr * s;
    a.gl_hf[q * 3 + 0] = dlh * s; a.gl_hf[q * 3 + 1] = dhl * s; a.gl_hf[q * 3 + 2] = dhh * s;
  }
}

// two-pass form: coefficients [pix0, pix0 + px) of one sub-network's fp32 dL/dout into its (chunk-local) Dlast; dfac
// ([n*n][3], sine output layer, written by the chunk's training forward just before) or null
__global__ __launch_bounds__(kWvThreads) void k_wv_inject(const float* gl, const float* dfac, long pix0, long px, u32x4* dl) {
  const long t = (long)blockIdx.x * kWvThreads + threadIdx.x;
  if (t >= px) return;
  const float* s = gl + (pix0 + t) * 3;
  if (dfac) {
    const float* f = dfac + (pix0 + t) * 3;
    wv_store_dlast(dl, t, s[0] * f[0], s[1] * f[1], s[2] * f[2]);
  } else {
    wv_store_dlast(dl, t, s[0], s[1], s[2]);
  }
}

}  // namespace sf
