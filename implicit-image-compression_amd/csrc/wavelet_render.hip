// wavelet_render.hip — the inference-only path of WaveletSiren: sf_wavelet_render_create / sf_wavelet_render
// (include/siren_fit.h).
//
// A decoder needs the picture, not a training step.  One call draws a pixel window [row0, row1) x [col0, col1) of the
// H x H picture:
//   the coefficient window [i0, i1) x [j0, j1) that window reads (wv_coeff_span below)
//   -> the RENDER forward (siren_render.hip: k_fwd<WD> / k_fwd_pipe, pred only) of LF and of HF over that sub-grid, whose
//      coordinates are the slices [i0, i1) / [j0, j1) of the caller's two full coefficient-grid vectors
//   -> k_wv_render: k_wv_compose (wavelet_kernels.hip) without the target, the residual, the SSE partial and its workgroup
//      barrier, with bytes.  The per-pixel body (wv_compose_pixel) is ONE compiled function that both kernels call, so the
//      fp32 prediction is bit-identical to what
//      sf_forward writes on a WaveletSiren training handle, and a window is bit-identical to that region of the full
//      picture: coefficient (i, j) sees rows[i], cols[j] whatever the window (tests/test_gpu_wavelet_render.py).
//
// Bytes: u8 = min(max((int)(v * 255.0f), 0), 255), the product in fp32 and truncated toward zero (render_quant,
// decode.to_u8); 16-bit samples (sf_wavelet_render16, k_wv_render<16>): u16 = min(max((int)(v * 65535.0f), 0), 65535).  A wave
// owns 64 consecutive pixels of the dense rows x cols output; how it packs, gathers and stores their samples: the sample
// tail, beside render_store in siren_kernels.hip.
//
// This file is included at the end of siren_fit.hip, after siren_render.hip (one translation unit); the creator builds on
// wavelet_host.hip.

namespace sf {

struct WvRenderArgs {
  int H, n;              // FULL picture side, coefficient side
  float up;              // bilinear source-index scale of the full picture
  int row0, col0;        // pixel window origin
  int cols;              // pixel window width (row length of the dense outputs)
  long npx;              // pixels of the window
  int i0, j0, cc;        // coefficient window origin and row length of lf / hf
  const float* lf;       // [cr * cc][3]
  const float* hf;
  float* pred;           // [npx][3] or null
  union {                // [npx][3] samples or null (4-byte aligned)
    uint8_t* rgb8;       //   k_wv_render<8>:  bytes
    uint16_t* rgb16;     //   k_wv_render<16>: native-endian uint16_t
  };
};

template <int BITS>
__global__ __launch_bounds__(kWvThreads) void k_wv_render(WvRenderArgs a) {
  static_assert(BITS == 8 || BITS == 16, "BITS: the sample width, 8 or 16");
  const long p = (long)blockIdx.x * kWvThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  RenderPx<BITS> mine;   // this lane's pixel
  if (p < a.npx) {
    const int pr = (int)(p / a.cols);
    const int r = a.row0 + pr, c = a.col0 + (int)(p - (long)pr * a.cols);
    // (no target: no fetch, no residual; pred, when asked for, is the plain 12-byte store of k_wv_compose)
    const WvPixel px = wv_compose_pixel(a.lf, a.hf, nullptr, a.pred, nullptr, 0.f, p, r, c, a.n, a.up, a.i0, a.j0, a.cc);
#pragma unroll
    for (int k = 0; k < 3; ++k) mine.put(k, px.rgb[k]);
  }
  if (!a.rgb8) return;   // (uniform; a.rgb16 is the same member)
  // (all 64 lanes: the gather is a cross-lane read.)  The wave's first pixel is a multiple of 64
  render_store<BITS, 64>(a.rgb8, p - lane, a.npx, 3, mine, lane);
}

}  // namespace sf

namespace {

// wv_tap's source indices (wavelet_kernels.hip) on the host, operation for operation in fp32 (one rounding per
// statement: no contraction)
void wv_tap_host(int o, float up, int n, int* i0, int* i1) {
  const float a = (float)o + 0.5f;
  const float m = up * a;
  float s = m - 0.5f;
  if (s < 0.f) s = 0.f;
  *i0 = (int)s;
  *i1 = *i0 + (*i0 < n - 1 ? 1 : 0);
}
// Coefficient rows (or columns) [lo, hi) that output rows [o0, o1) of an H-row picture read.  Row o reads, for Y,
// coefficients o/2 .. o/2 + 2 (k_wv_compose's gather) and, for Cb / Cr, wv_tap(o).i0 and .i1; all are monotone in o, so
// the span is the minimum at o0 and the maximum at o1 - 1.  (Python mirror: implicit_image.decode.wavelet_coeff_span)
void wv_coeff_span(int o0, int o1, int H, int* lo, int* hi) {
  const int n = (H + 5) / 2;
  const float up = (float)(1.0 / ((double)H / (double)n));
  int a0, a1, b0, b1;
  wv_tap_host(o0, up, n, &a0, &a1);
  wv_tap_host(o1 - 1, up, n, &b0, &b1);
  *lo = std::min(o0 / 2, a0);
  *hi = std::max((o1 - 1) / 2 + 2, b1) + 1;
}

int create_wavelet_render(const sf_wavelet_render_config* cfg, sf_handle** out) {
  HandlePtr sub[2];
  int max_rows = 0, max_cols = 0, cr = 0, cc = 0;   // the largest pixel window, and the largest coefficient window of any such
  auto check = [&](Grid& g) -> int {
    SF_TRY(wavelet_check_network(cfg));
    SF_TRY(wavelet_check_image(cfg->height, cfg->height, cfg->chunk_pixels));
    const int H = cfg->height;
    max_rows = cfg->max_rows ? cfg->max_rows : H; max_cols = cfg->max_cols ? cfg->max_cols : H;
    if (max_rows < 1 || max_rows > H || max_cols < 1 || max_cols > H)
      return fail(SF_ERR_INVALID, "sf_wavelet_render_create: max_rows / max_cols must be 0 (the whole picture) or 1 .. height");
    auto max_span = [&](int len) {   // (the span's length depends on where it sits)
      int best = 0;
      for (int o = 0; o + len <= H; ++o) {
        int lo, hi;
        wv_coeff_span(o, o + len, H, &lo, &hi);
        best = std::max(best, hi - lo);
      }
      return best;
    };
    cr = max_span(max_rows); cc = max_span(max_cols);
    g = {H, H, 0, H};
    return wavelet_subs(wavelet_sub_config(cfg, cr, cc), true, sub);
  };
  auto init = [&](sf_engine* h, const Grid& g) -> int {
    wavelet_begin(h, sub, g.height);
    h->wv.max_rows = max_rows; h->wv.max_cols = max_cols;
    SF_TRY(alloc_state(h, false));
    SF_TRY(dev_alloc(h, h->wv.pred, (size_t)2 * cr * cc * 3 * 4));   // the one pair of coefficient buffers
    SF_TRY(dev_alloc(h, h->gh, (size_t)h->wv.n * 4));   // the caller's FULL coefficient-grid vectors
    SF_TRY(dev_alloc(h, h->gw, (size_t)h->wv.n * 4));
    for (int s = 0; s < 2; ++s) h->wv.sub[s]->params = h->params + s * h->wv.sub[s]->P;   // the two halves of the joint vector
    return SF_OK;
  };
  return create_with(cfg, out, (int32_t sf_wavelet_render_config::*)nullptr, Model::Wavelet, true, check, init);
}

// sf_wavelet_render (bits = 8) and sf_wavelet_render16 (bits = 16): one set of argument checks; the sub-networks are drawn by render_chunks
int wavelet_render_any(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, void* out, int bits, float* pred) {
  const std::string fn = bits == 16 ? "sf_wavelet_render16" : "sf_wavelet_render", on = bits == 16 ? "rgb16_dev" : "rgb8_dev";
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  if (h->model != Model::Wavelet)
    return fail(SF_ERR_INVALID, fn + ": not a WaveletSiren handle (sf_wavelet_render_create / sf_wavelet_create)");
  if (!out && !pred) return fail(SF_ERR_INVALID, fn + ": " + on + " and pred_dev are both NULL");
  if (((uintptr_t)out & 3u) != 0) return fail(SF_ERR_INVALID, fn + ": " + on + " must be 4-byte aligned");
  const int H = h->cfg.height;
  if (row0 < 0 || row1 > H || row0 >= row1 || col0 < 0 || col1 > H || col0 >= col1)
    return fail(SF_ERR_INVALID, fn + ": need 0 <= row0 < row1 <= height and 0 <= col0 < col1 <= height");
  if (h->render && (row1 - row0 > h->wv.max_rows || col1 - col0 > h->wv.max_cols))
    return fail(SF_ERR_INVALID, fn + ": the window is larger than the max_rows x max_cols the handle was created for");
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(refresh_images(h));
  int i0, i1, j0, j1;
  wv_coeff_span(row0, row1, H, &i0, &i1);
  wv_coeff_span(col0, col1, H, &j0, &j1);
  const int cr = i1 - i0, cc = j1 - j0;
  const long nn = (long)cr * cc;
  // the full coordinate vectors: a render handle keeps them itself, a training handle in its sub-networks
  const float* gh = h->render ? h->gh : h->wv.sub[0]->gh;
  const float* gw = h->render ? h->gw : h->wv.sub[0]->gw;
  float* const p_sub[2] = {h->wv.pred, h->wv.pred + nn * 3};
  // the sub-grid of this window: its rows / columns are slices of the full vectors, its row length is cc
  const PixelView window = {gh + i0, gw + j0, cc, nn};
  for (int s = 0; s < 2; ++s) SF_TRY(render_chunks(h->wv.sub[s], nullptr, 8, p_sub[s], &window));
  WvRenderArgs a = zeroed<WvRenderArgs>();
  a.H = H; a.n = h->wv.n; a.up = h->wv.up;
  a.row0 = row0; a.col0 = col0; a.cols = col1 - col0;
  a.npx = (long)(row1 - row0) * (col1 - col0);
  a.i0 = i0; a.j0 = j0; a.cc = cc;
  a.lf = p_sub[0]; a.hf = p_sub[1];
  a.pred = pred; a.rgb8 = (uint8_t*)out;   // (a.rgb16 of k_wv_render<16>: the same member)
  Launch L(h, K_WV_RENDER, 0, (double)a.npx * 3.0 * render_sample_bytes(out, bits, pred) + (double)nn * 24.0);
  const long n_wg = (a.npx + kWvThreads - 1) / kWvThreads;
  return bits == 16 ? launch(h, k_wv_render<16>, n_wg, kWvThreads, 0, a) : launch(h, k_wv_render<8>, n_wg, kWvThreads, 0, a);
}

}  // namespace

extern "C" {

int sf_wavelet_render_create(const sf_wavelet_render_config* cfg, sf_handle** out) try {
  return create_wavelet_render(cfg, out);
} SF_CATCH

int sf_wavelet_render(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, uint8_t* rgb8, float* pred) try {
  return wavelet_render_any(h, row0, row1, col0, col1, rgb8, 8, pred);
} SF_CATCH

}  // extern "C"

extern "C" {   // sf_wavelet_render at 16 bits per sample

int sf_wavelet_render16(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, uint16_t* rgb16, float* pred) try {
  return wavelet_render_any(h, row0, row1, col0, col1, rgb16, 16, pred);
} SF_CATCH

}  // extern "C"
