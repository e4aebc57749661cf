// fourier_kernels.hip — gfx950 kernels of the FourierNet fit (random-Fourier-feature encoding -> ReLU MLP -> sigmoid).
//
// Reference arithmetic being replaced (paths relative to the reference tree):
//   implicit_image/models/fourier.py:21-24      encoding [sin(2 pi x B), cos(2 pi x B)]
//   implicit_image/models/fourier.py:43-56      Linear -> ReLU stack, Linear -> Sigmoid
//   implicit_image/utils/train_helper.py:147-161 F.mse_loss + autograd backward
//
// Same "transposed" network orientation as the SIREN kernels (layout.h): rows = neurons, columns = pixels, one wave
// owns 32 pixels, every GEMM is v_mfma_f32_32x32x16_f16 (fp16 operands, fp32 accumulation), and the accumulator of
// layer l is the B operand of layer l+1 with the k order permuted by PI (layout.h).
//
// Scratch between kernels is NEURON-MAJOR fp16, [layer][neuron][chunk pixel] with row stride `cp` (the chunk's pixel
// capacity, a multiple of 256): the chain kernels read / write it with one 2-byte access per accumulator register
// (32 consecutive pixels per instruction), and the weight-gradient kernels, whose contraction runs over pixels, read
// it as 16-byte MFMA fragments (8 consecutive pixels of one neuron) without a transpose.
//
//   k_ff_fwd<WD, TRAIN>  encoding computed in registers from the coordinates (phase reduced in revolutions), every layer
//                        on MFMA with the weight image staged through LDS in k slices, residual, SSE partial,
//                        dL/dz_out = 2 (s - y) s (1 - s) / (3 H W) (pre-scaled, fp16).  TRAIN spills every ReLU output h_l.
//                        RENDER (inference only, sf_render / fourier_render.hip): the same chain and sigmoid without
//                        the target, the residual, dz, the scratch stores and the SSE reduction; fp32 and / or bytes.
//                        EVAL (sf_eval, BITS = kFfEvalBits): the evaluation form without the prediction store; its SSE
//                        partial and, beside it, the exact integer partial of the 8-bit figure (eval_sq8).
//   k_ff_bwd<WD>         data-gradient chain g_{l-1} = (W_l^T g_l) * [h_{l-1} > 0], l = L-1 .. 1, spilling every g_l.
//   k_ff_dw<NI, E0>      dW_l = g_l h_{l-1}^T and db_l = sum g_l over the workgroup's pixels into a per-workgroup slab
//                        (E0: layer 0, whose input, the encoding, is recomputed from the coordinates); k_reduce* of
//                        siren_kernels.hip sums the slabs in fixed order.
//   k_ff_images          fp16 weight images (forward A fragments of every layer, backward A fragments of layers >= 1).
// (included by siren_fit.hip after siren_kernels.hip: OpF16, rho, pi_perm, k_reduce*, k_adam)

namespace sf {

constexpr int kFfMaxLinear = 12;
constexpr int kFfThreads = 512;                 // 8 waves x 32 pixels = 256 pixels per chain workgroup
constexpr int kFfLdsPieces = 64;                // weight slice staged in LDS: 64 fragments x 1 KiB
constexpr size_t kFfLdsBytes = (size_t)kFfLdsPieces * 1024;
constexpr int ff_ksl(int WD) { return kFfLdsPieces / (WD / 32); }   // k-steps per staged slice

struct FfArgs {
  const float* gh; const float* gw;   // linspace coordinate vectors (rows, cols)
  int W;                              // image width
  long pix0, npix;                    // first pixel of the chunk, pixels of the image
  long cp;                            // row stride of the scratch planes (chunk capacity)
  const float* Btab;                  // encoding.B [2][MS/2], fp32 (xp / 2 pi = x @ B: revolutions)
  int MS, nlin;
  const u32x4* img;                   // fp16 weight images
  long img_f[kFfMaxLinear];           // forward image of layer l (offset in 16-byte units)
  long img_b[kFfMaxLinear];           // backward image of layer l >= 1
  const float* params;
  long off_b[kFfMaxLinear];
  _Float16* H;                        // [nlin-1][WD][cp] ReLU outputs
  _Float16* G;                        // [nlin-1][WD][cp] data gradients of the hidden layers
  _Float16* Z;                        // [3][cp] dL/dz of the output layer (pre-scaled)
  const float* tgt;                   // target image rows [npix][3] (may be null: prediction only)
  float* pred;                        // [npix][3] or null
  union {                             // RENDER only: [npix][3] samples or null (4-byte aligned)
    uint8_t* rgb8;                    //   BITS = 8:  bytes, min(max((int)(pred * 255), 0), 255)
    uint16_t* rgb16;                  //   BITS = 16: native-endian uint16_t, min(max((int)(pred * 65535), 0), 65535)
    unsigned long long* sse8_part;    // EVAL only, never null: one integer partial (eval_sq8) per workgroup, beside sse_part
  };
  float* sse_part;                    // one partial per workgroup
  float gscale;                       // gpre / (3 H W)
};

DEV int ff_lane_px(long p, const FfArgs& a, float& x0, float& x1) {
  const long q = p < a.npix ? p : a.npix - 1;
  const long r = q / a.W, c = q - r * a.W;
  x0 = a.gh[r];
  x1 = a.gw[c];
  return 0;
}

// sin / cos of 2 pi (x0 B0c + x1 B1c): the phase is formed and reduced in revolutions (fract), where v_sin / v_cos are
// accurate; map_scale 16 puts the raw argument near 300 rad
DEV float ff_feature(float x0, float x1, const float* Btab, int half, int f) {
  const bool is_cos = f >= half;
  const int c = is_cos ? f - half : f;
  const float t = __builtin_fmaf(x1, Btab[half + c], x0 * Btab[c]);
  const float fr = __builtin_amdgcn_fractf(t);
  return is_cos ? __builtin_amdgcn_cosf(fr) : __builtin_amdgcn_sinf(fr);
}

// stage fragments (tile nt < NT, k-step s0 + i, i < nks) of a weight image with KS k-steps per tile into LDS [nt][i]
template <int NT, int KSL>
DEV void ff_stage(u32x4* lds, const u32x4* src, int KS, int s0, int nks) {
  const int per_tile = nks * 64;
  const int total = NT * per_tile;
#pragma unroll 4
  for (int e = threadIdx.x; e < total; e += kFfThreads) {
    const int nt = e / per_tile, rem = e - nt * per_tile;
    lds[nt * KSL * 64 + rem] = src[((long)nt * KS + s0) * 64 + rem];
  }
}

// accumulators start from the layer's bias (row 32 nt + rho(t, h) of a [rows] vector; rows past `rows` are 0)
template <int NT>
DEV void ff_bias_init(f32x16 (&acc)[NT], const float* bias, int rows, int hh) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int row = 32 * nt + rho(t, hh);
      acc[nt][t] = row < rows ? bias[row] : 0.f;
    }
}

template <int NT>
DEV void ff_to_frags(const f32x16 (&acc)[NT], u32x4 (&fr)[2 * NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      u32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = OpF16::pack2(acc[nt][8 * q + 2 * k], acc[nt][8 * q + 2 * k + 1]);
      fr[2 * nt + q] = v;
    }
}

// fixed-order workgroup sum of one float per lane (butterfly inside the wave, waves added in order)
DEV float ff_block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < kFfThreads / 64; ++w) s += sh[w];
  return s;
}

// EVAL (sf_eval) is the evaluation form with no samples at all, BITS = kFfEvalBits: the kernel has no operand tag to wrap
// (OpEval), and a further template parameter would rename every existing instantiation
constexpr int kFfEvalBits = 0;
template <int WD, bool TRAIN, bool RENDER = false, int BITS = 8>
__global__ __launch_bounds__(kFfThreads) void k_ff_fwd(FfArgs a) {
  constexpr bool EVAL = BITS == kFfEvalBits;
  static_assert(!(TRAIN && RENDER), "the render form spills nothing");
  static_assert(BITS == 8 || (RENDER && BITS == 16) || (EVAL && !TRAIN && !RENDER),
                "BITS: the sample width of the RENDER form, 8 or 16; kFfEvalBits: the EVAL form");
  constexpr int NT = WD / 32, KS = WD / 16, KSL = ff_ksl(WD);
  extern __shared__ u32x4 lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, hh = lane >> 5;
  const long pl = (long)blockIdx.x * 256 + wave * 32 + m;   // chunk-local pixel of this lane's column
  const long p = a.pix0 + pl;
  const bool valid = p < a.npix;
  float x0, x1;
  ff_lane_px(p, a, x0, x1);

  f32x16 acc[NT];
  u32x4 fr[KS];
  // ---- layer 0: K = map_size, the encoding computed per k-step ----
  {
    const int KS0 = a.MS / 16, half = a.MS / 2;
    ff_bias_init<NT>(acc, a.params + a.off_b[0], WD, hh);
    for (int s0 = 0; s0 < KS0; s0 += KSL) {
      const int nks = KS0 - s0 < KSL ? KS0 - s0 : KSL;
      __syncthreads();
      ff_stage<NT, KSL>(lds, a.img + a.img_f[0], KS0, s0, nks);
      __syncthreads();
      for (int i = 0; i < nks; ++i) {
        const int s = s0 + i;
        u32x4 b;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          b[k] = OpF16::pack2(ff_feature(x0, x1, a.Btab, half, 16 * s + pi_perm(hh, 2 * k)),
                              ff_feature(x0, x1, a.Btab, half, 16 * s + pi_perm(hh, 2 * k + 1)));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = OpF16::mfma(lds[(nt * KSL + i) * 64 + lane], b, acc[nt]);
      }
    }
  }
  // ---- ReLU of layer l, then hidden layers l + 1 ----
  // scratch addressing: a wave-uniform plane base + a 32-bit element offset (WD * cp < 2^31: sf_fourier_create)
  const uint32_t cp32 = (uint32_t)a.cp, lane_off = (uint32_t)(4 * hh) * cp32 + (uint32_t)pl;
  for (int l = 0; l < a.nlin - 1; ++l) {
    _Float16* Hl = a.H + (size_t)l * WD * a.cp;
    uint32_t lo = lane_off;
    asm volatile("" : "+v"(lo));   // keeps the 16 x NT store offsets from being hoisted out of the layer loop (registers)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        acc[nt][t] = acc[nt][t] > 0.f ? acc[nt][t] : 0.f;
        if (TRAIN) Hl[(uint32_t)(32 * nt + rho(t, 0)) * cp32 + lo] = (_Float16)acc[nt][t];
      }
    ff_to_frags<NT>(acc, fr);
    if (l == a.nlin - 2) break;
    const u32x4* src = a.img + a.img_f[l + 1];
    ff_bias_init<NT>(acc, a.params + a.off_b[l + 1], WD, hh);
#pragma unroll
    for (int s0 = 0; s0 < KS; s0 += KSL) {
      constexpr int NKS = KS < KSL ? KS : KSL;
      __syncthreads();
      ff_stage<NT, KSL>(lds, src, KS, s0, NKS);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NKS; ++i)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = OpF16::mfma(lds[(nt * KSL + i) * 64 + lane], fr[s0 + i], acc[nt]);
    }
  }
  // ---- output layer (3 rows of a 32-row tile) + sigmoid + loss ----
  f32x16 o[1];
  ff_bias_init<1>(o, a.params + a.off_b[a.nlin - 1], 3, hh);
  __syncthreads();
  ff_stage<1, KSL>(lds, a.img + a.img_f[a.nlin - 1], KS, 0, KS);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < KS; ++s) o[0] = OpF16::mfma(lds[s * 64 + lane], fr[s], o[0]);
  if constexpr (RENDER) {
    // no target, no residual, no dz, no Z store, no workgroup sum: the sigmoid of k_ff_fwd<WD, false>, then bytes (BITS = 8)
    // or 16-bit samples (BITS = 16)
    RenderPx<BITS> mine;   // this lane's pixel (the upper lane half holds padded rows: never selected)
    if (hh == 0) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float z = o[0][t];
        const float sg = 1.0f / (1.0f + __expf(-z));
        if (valid && a.pred) a.pred[p * 3 + t] = sg;
        mine.put(t, sg);
      }
    }
    // (all 64 lanes: the gather is a cross-lane read.)  pix0 is a multiple of 256: the wave's first pixel is one of 32
    const long px0 = a.pix0 + (long)blockIdx.x * 256 + wave * 32;
    if (a.rgb8) render_store<BITS, 32>(a.rgb8, px0, a.npix, 3, mine, lane);   // (a.rgb16: the same member)
  } else if constexpr (EVAL) {
    // the residual and the sum of k_ff_fwd<WD, false> (the same expressions: the same SSE partial), the sigmoid used once
    // more for the integer partial; no prediction, no dz
    __shared__ __attribute__((aligned(8))) float sh_sse[2 * (kFfThreads / 64)];   // (then the waves' 64-bit partials)
    float sse = 0.f;
    unsigned long long s8 = 0;
    if (hh == 0 && valid) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float z = o[0][t];
        const float sg = 1.0f / (1.0f + __expf(-z));
        const float tg = a.tgt[p * 3 + t];
        const float r = sg - tg;
        // k_ff_fwd<WD, false> forms its sum as r0 * r0, then one fused multiply-add per further channel.  Written out: left
        // to itself the compiler pairs the three squares here into packed multiplies, which round before the add
        sse = t == 0 ? r * r : __builtin_fmaf(r, r, sse);
        s8 += eval_sq8(tg, sg);
      }
    }
    const float s = ff_block_sum(sse, sh_sse);
    if (threadIdx.x == 0) a.sse_part[blockIdx.x] = s;
    eval_block_partial<kFfThreads / 64>(s8, sh_sse, a.sse8_part + blockIdx.x);
  } else {
    __shared__ float sh_sse[kFfThreads / 64];
    float sse = 0.f;
    if (hh == 0) {   // rows 0..2 sit in registers 0..2 of the lower lane half
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float z = o[0][t];
        const float sg = 1.0f / (1.0f + __expf(-z));
        float dz = 0.f;
        if (valid) {
          if (a.pred) a.pred[p * 3 + t] = sg;
          if (a.tgt) {
            const float r = sg - a.tgt[p * 3 + t];
            sse += r * r;
            dz = 2.0f * r * sg * (1.0f - sg) * a.gscale;
          }
        }
        if (TRAIN) a.Z[(uint32_t)t * cp32 + (uint32_t)pl] = (_Float16)dz;
      }
    }
    const float s = ff_block_sum(sse, sh_sse);
    if (threadIdx.x == 0) a.sse_part[blockIdx.x] = s;
  }
}

// data-gradient chain, last layer first
template <int WD>
__global__ __launch_bounds__(kFfThreads) void k_ff_bwd(FfArgs a) {
  constexpr int NT = WD / 32, KS = WD / 16, KSL = ff_ksl(WD);
  extern __shared__ u32x4 lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, hh = lane >> 5;
  const long pl = (long)blockIdx.x * 256 + wave * 32 + m;
  f32x16 acc[NT];
  u32x4 fr[KS];
  // g_{L-1} = dL/dz_out: k-step 0 of a 16-row operand, rows 0..2 live (element j of half 0 is row PI(0, j) = j for j < 4)
  {
    u32x4 bz = {0u, 0u, 0u, 0u};
    if (hh == 0) {
      const uint32_t p32 = (uint32_t)pl, c32 = (uint32_t)a.cp;
      const float z0 = (float)a.Z[p32], z1 = (float)a.Z[c32 + p32], z2 = (float)a.Z[2 * c32 + p32];
      bz[0] = OpF16::pack2(z0, z1);
      bz[1] = OpF16::pack2(z2, 0.f);
    }
    __syncthreads();
    ff_stage<NT, KSL>(lds, a.img + a.img_b[a.nlin - 1], 1, 0, 1);
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = OpF16::mfma(lds[nt * KSL * 64 + lane], bz, f32x16{});
  }
  const uint32_t cp32 = (uint32_t)a.cp, lane_off = (uint32_t)(4 * hh) * cp32 + (uint32_t)pl;
  for (int l = a.nlin - 2; l >= 0; --l) {
    // g_l = acc * [h_l > 0]
    const _Float16* Hl = a.H + (size_t)l * WD * a.cp;
    _Float16* Gl = a.G + (size_t)l * WD * a.cp;
    uint32_t lo = lane_off;
    asm volatile("" : "+v"(lo));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const uint32_t idx = (uint32_t)(32 * nt + rho(t, 0)) * cp32 + lo;
        const float g = Hl[idx] > (_Float16)0 ? acc[nt][t] : 0.f;
        acc[nt][t] = g;
        Gl[idx] = (_Float16)g;
      }
    if (l == 0) break;   // layer 0 has no data gradient (B frozen, coordinates constant)
    ff_to_frags<NT>(acc, fr);
    const u32x4* src = a.img + a.img_b[l];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x16{};
#pragma unroll
    for (int s0 = 0; s0 < KS; s0 += KSL) {
      constexpr int NKS = KS < KSL ? KS : KSL;
      __syncthreads();
      ff_stage<NT, KSL>(lds, src, KS, s0, NKS);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NKS; ++i)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = OpF16::mfma(lds[(nt * KSL + i) * 64 + lane], fr[s0 + i], acc[nt]);
    }
  }
}

// weight gradient of one layer: contraction over the pixels [blockIdx.x * ppw, +ppw) of the chunk
struct FfDwArgs {
  const _Float16* A;     // g_l plane [rows][cp]
  int rows;              // live rows of the layer (3 for the output layer)
  const _Float16* Bm;    // h_{l-1} plane [in][cp] (null for layer 0: the encoding is recomputed)
  int in, n_it;          // input width, 32-column tiles
  int n_groups;          // (32-row tiles) x (column groups of NI tiles)
  long cp, n_px, ppw;
  float* slab;           // [gridDim.x][rows * in + rows]
  FfArgs e;              // coordinates / encoding (layer 0)
};

template <int NI, bool E0>
__global__ __launch_bounds__(256) void k_ff_dw(FfDwArgs a) {
  const int lane = threadIdx.x & 63, m = lane & 31, hh = lane >> 5;
  const int gid = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gid >= a.n_groups) return;
  const int n_cg = a.n_it / NI, ot = gid / n_cg, it0 = (gid - ot * n_cg) * NI;
  const long p_lo = (long)blockIdx.x * a.ppw;
  long p_hi = p_lo + a.ppw;
  if (p_hi > a.n_px) p_hi = a.n_px;
  const int row = 32 * ot + m;
  const bool row_live = row < a.rows;
  f32x16 acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x16{};
  float bsum = 0.f;
  const int half = a.e.MS / 2;
  for (long p = p_lo; p < p_hi; p += 16) {
    const long pk = p + 8 * hh;   // this lane's 8 pixels (k = 8 hh + j)
    u32x4 fa = {0u, 0u, 0u, 0u};
    if (row_live) fa = *reinterpret_cast<const u32x4*>(a.A + (long)row * a.cp + pk);
    if (it0 == 0) bsum += OpF16::sum2(fa[0]) + OpF16::sum2(fa[1]) + OpF16::sum2(fa[2]) + OpF16::sum2(fa[3]);
    u32x4 fb[NI];
    if constexpr (E0) {
      float x0[8], x1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) ff_lane_px(a.e.pix0 + pk + j, a.e, x0[j], x1[j]);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int f = 32 * (it0 + i) + m;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          fb[i][k] = OpF16::pack2(ff_feature(x0[2 * k], x1[2 * k], a.e.Btab, half, f),
                                  ff_feature(x0[2 * k + 1], x1[2 * k + 1], a.e.Btab, half, f));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) fb[i] = *reinterpret_cast<const u32x4*>(a.Bm + (long)(32 * (it0 + i) + m) * a.cp + pk);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = OpF16::mfma(fa, fb[i], acc[i]);
  }
  float* slab = a.slab + (long)blockIdx.x * ((long)a.rows * a.in + a.rows);
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int r = 32 * ot + rho(t, hh);
      if (r < a.rows) slab[(long)r * a.in + 32 * (it0 + i) + m] = acc[i][t];
    }
  bsum += __shfl_xor(bsum, 32);
  if (it0 == 0 && hh == 0 && row_live) slab[(long)a.rows * a.in + row] = bsum;
}

// fp16 weight images of every layer, one 16-byte fragment element (8 weights) per thread:
//   forward  (A of z = W x):    tile nt, k-step s, lane (r, h), elem j = W[32 nt + r][16 s + PI(h, j)]
//   backward (A of dx = W^T g): tile it, k-step s, lane (r, h), elem j = W[16 s + PI(h, j)][32 it + r]
// rows / columns past the layer's shape are zero (output layer: 3 rows padded to 32 / 16).
struct FfImgArgs {
  const float* params;
  int nlin;
  long off_w[kFfMaxLinear];
  int in[kFfMaxLinear], out[kFfMaxLinear];
  long start[2 * kFfMaxLinear + 1];   // segment 2l: forward image of layer l, 2l+1: backward image (empty for l = 0)
  u32x4* img;
};
__global__ void k_ff_images(FfImgArgs a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.start[2 * a.nlin]) return;
  int seg = 0;
  while (e >= a.start[seg + 1]) ++seg;
  const int l = seg >> 1;
  const bool bwd = seg & 1;
  const int in = a.in[l], out = a.out[l];
  const float* W = a.params + a.off_w[l];
  const long loc = e - a.start[seg];
  const int lane = (int)(loc & 63), r = lane & 31, hh = lane >> 5;
  const int KS = bwd ? (out + 15) / 16 : in / 16;
  const long tile = (loc >> 6) / KS;
  const int s = (int)((loc >> 6) - tile * KS);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 16 * s + pi_perm(hh, j);
    if (!bwd) {
      const long row = 32 * tile + r;
      v[j] = row < out ? W[row * in + k] : 0.f;
    } else {
      const long col = 32 * tile + r;
      v[j] = k < out ? W[(long)k * in + col] : 0.f;
    }
  }
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = OpF16::pack2(v[2 * k], v[2 * k + 1]);
  a.img[e] = o;
}

}  // namespace sf
