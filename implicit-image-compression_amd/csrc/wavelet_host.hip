// wavelet_host.hip — WaveletSiren on the host (kernels: wavelet_kernels.hip): the pass over the two SIREN sub-handles, what
// both creators share, sf_wavelet_create / sf_wavelet_debug.  Included by siren_fit.hip after siren_host.hip (create_handle).

namespace {

// the joint parameters changed: both sub-networks' weight images follow
int refresh_images_wavelet(sf_engine* h) {
  for (sf_engine* s : h->wv.sub) {
    s->images_dirty = true;
    SF_TRY(refresh_images(s));
  }
  h->images_dirty = false;
  return SF_OK;
}

// WaveletSiren pass.  One chunk (the coefficient grid fits one sweep of the sub-networks):
//   training forward of LF and HF (no target: phases, predictions, zero dL/dout) -> k_wv_compose -> k_wv_adjoint (dL/dout
//   straight into both Dlast) -> the backward chain of LF, then of HF (slab reductions into each half of the gradient).
// Two passes (more than one chunk): inference forward of both over every chunk -> compose -> adjoint into an fp32 buffer
//   -> per chunk and sub-network: training forward, k_wv_inject, backward.
// Then the fixed-order reduction of the compose partials into the handle's SSE.
// The sub-networks run through the SIREN chunk functions (siren_host.hip) and, for the inference forwards, the chunk loop; they
// launch through this handle's context, their weight images are refreshed here with this handle's, and the SSE partials
// their forwards write (they have no target: nothing reads them) go to the start of their own sse_part.
// eval8 (sf_eval): the sub-network forwards of an evaluation, then k_wv_compose_eval - no picture is written - and the
// reduction of both kinds of partials.
int run_pass_wavelet(sf_engine* h, bool train, float* pred, bool want_sse, bool eval8) {
  SF_TRY(refresh_images(h));
  sf_engine* const sub[2] = {h->wv.sub[0], h->wv.sub[1]};
  const long nn = sub[0]->npix, HH = h->npix;
  const bool one = nn <= sub[0]->chunk_px;
  float* const p_sub[2] = {h->wv.pred, h->wv.pred + nn * 3};
  int n_part[2] = {0, 0};
  for (int s = 0; s < 2; ++s)
    SF_TRY(train && one ? siren_fwd_chunk(sub[s], 0, true, p_sub[s], sub[s]->sse_part, n_part[s])
                        : run_chunks(sub[s], false, p_sub[s], false));
  WvArgs a = zeroed<WvArgs>();
  a.H = h->cfg.height; a.n = h->wv.n; a.up = h->wv.up;
  a.lf = p_sub[0]; a.hf = p_sub[1];
  a.img = h->img; a.pred = pred; a.g = train ? h->wv.g : nullptr;
  a.sse_part = h->sse_part;
  a.gscale = (float)(2.0 / (3.0 * h->n_total));
  a.dscale = 0.5f * sub[0]->gpre;
  a.dfac_lf = sub[0]->wv.dfac_out; a.dfac_hf = sub[1]->wv.dfac_out;   // (null for a linear output layer)
  auto wv_grid = [](long n) { return (unsigned)((n + kWvThreads - 1) / kWvThreads); };
  const unsigned n_cwg = wv_grid(HH);
  {
    Launch L(h, K_WV_COMPOSE, 0, (double)HH * 4.0 * (3.0 + (a.img ? 3.0 : 0.0) + (pred ? 3.0 : 0.0) + (train ? 3.0 : 0.0)));
    if (eval8) SF_TRY(launch(h, k_wv_compose_eval, n_cwg, kWvThreads, 0, a, h->sse8_part));
    else SF_TRY(launch(h, k_wv_compose, n_cwg, kWvThreads, 0, a));
  }
  if (eval8) return launch_eval_reduce(h, n_cwg);
  if (train) {
    if (one) { a.dl_lf = sub[0]->Dlast; a.dl_hf = sub[1]->Dlast; }
    else { a.gl_lf = h->wv.gl; a.gl_hf = h->wv.gl + nn * 3; }
    {
      Launch L(h, K_WV_ADJOINT, 0, (double)nn * (52.0 * 8.0 + (one ? 32.0 : 24.0)));
      SF_TRY(launch(h, k_wv_adjoint, wv_grid(nn), kWvThreads, 0, a));
    }
    if (one) {
      for (int s = 0; s < 2; ++s) SF_TRY(siren_bwd_chunk(sub[s], 0, sub[s]->sse_part, n_part[s]));
    } else {
      for (long c = 0; c < n_chunks(nn, sub[0]->chunk_px); ++c) {
        const Chunk k = chunk_at(c, nn, sub[0]->chunk_px);
        for (int s = 0; s < 2; ++s) {
          SF_TRY(siren_fwd_chunk(sub[s], c, true, nullptr, sub[s]->sse_part, n_part[s]));
          {
            Launch L(h, K_WV_INJECT, 0, (double)k.px * 28.0);
            SF_TRY(launch(h, k_wv_inject, wv_grid(k.px), kWvThreads, 0, h->wv.gl + (size_t)s * nn * 3, sub[s]->wv.dfac_out, k.pix0,
                          k.px, sub[s]->Dlast));
          }
          SF_TRY(siren_bwd_chunk(sub[s], c, sub[s]->sse_part, n_part[s]));
        }
      }
    }
  }
  if (want_sse || train) SF_TRY(launch_sse_reduce(h, n_cwg));
  return SF_OK;
}

// ---- WaveletSiren: what sf_wavelet_create and sf_wavelet_render_create (wavelet_render.hip) share ------------------
// the argument checks both creators word identically, in the order both run them
template <typename Config>
int wavelet_check_network(const Config* cfg) {
  if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256)
    return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128 or 256 for WaveletSiren (other widths: zero-pad on the host)");
  if (cfg->depth < 2 || cfg->depth > 16) return fail(SF_ERR_INVALID, "depth must be 2..16");
  if (cfg->compute_dtype != SF_F16) return fail(SF_ERR_INVALID, "WaveletSiren runs fp16 operands only (compute_dtype SF_F16)");
  return SF_OK;
}
int wavelet_check_image(int height, int width, int64_t chunk_pixels) {
  if (height != width || height < 2 || height % 2)
    return fail(SF_ERR_INVALID, "WaveletSiren needs an even, square image: the reference's inverse DWT (2n - 4 rows) and its "
                                "torch.cat of Y with the upsampled Cb / Cr stop matching otherwise");
  if ((double)height * (double)width >= 2147483648.0) return fail(SF_ERR_INVALID, "image too large");
  if (chunk_pixels < 0) return fail(SF_ERR_INVALID, "chunk_pixels must be >= 0");
  return SF_OK;
}
// config of the two sub-networks: SIRENs of the creator's shape on a rows x cols coefficient grid, scratch format 16
template <typename Config>
sf_config wavelet_sub_config(const Config* cfg, int rows, int cols) {
  sf_config sc = zeroed<sf_config>();
  sc.abi_version = SF_ABI_VERSION; sc.height = rows; sc.width = cols; sc.row_begin = 0; sc.row_end = rows;
  sc.in_features = 2; sc.out_features = 3; sc.hidden = cfg->hidden; sc.depth = cfg->depth;
  sc.first_omega_0 = cfg->first_omega_0; sc.hidden_omega_0 = cfg->hidden_omega_0; sc.outermost_linear = cfg->outermost_linear;
  sc.compute_dtype = SF_F16; sc.device = cfg->device; sc.stream = cfg->stream; sc.chunk_pixels = cfg->chunk_pixels;
  sc.scratch_format = 16;
  return sc;
}
// the two sub-networks (LF, HF; their flat state stays unallocated: the creator points it at slices of the joint vectors
// it allocates)
int wavelet_subs(const sf_config& sc, bool render, HandlePtr (&sub)[2]) {
  for (HandlePtr& s : sub) {
    sf_handle* e = nullptr;
    SF_TRY(create_handle(&sc, &e, render, true));   // (render: refuses rows * cols^2 >= 2^40: draw such a picture in bands)
    s.reset(e);
  }
  return SF_OK;
}
// ... and the handle itself, an H x H picture over them: from here on both launch through its launch context
void wavelet_begin(sf_engine* h, HandlePtr (&sub)[2], int H) {
  h->cfg = sub[0]->cfg;
  h->cfg.height = H; h->cfg.width = H; h->cfg.row_begin = 0; h->cfg.row_end = H;
  h->beta1_d = sub[0]->beta1_d; h->beta2_d = sub[0]->beta2_d;
  h->D = 2 * sub[0]->D; h->WD = sub[0]->WD;
  h->wv.n = (H + 5) / 2;   // pywt.dwt_coeff_len(H, 6, "zero")
  h->wv.up = (float)(1.0 / ((double)H / (double)h->wv.n));   // torch: scale_factor = H / n, source scale 1 / scale_factor
  h->P = 2 * sub[0]->P;
  for (int s = 0; s < 2; ++s) {
    h->wv.sub[s] = sub[s].release();
    h->wv.sub[s]->ctx = &h->own;
  }
}

}  // namespace

extern "C" {

// WaveletSiren handle: two SIREN sub-handles (sf_create, format 16) whose state buffers are slices of this handle's joint
// [LF | HF] vectors, so that sf_state_ptr, sf_get/set_*, sf_adam_step (one k_adam over the joint vector), sf_step and graph
// replay work unchanged; run_pass_wavelet drives the sub-handles around the composition kernels
int sf_wavelet_create(const sf_wavelet_config* cfg, sf_handle** out) try {
  HandlePtr sub[2];
  auto check = [&](Grid& g) -> int {
    if (cfg->out_features != 3) return fail(SF_ERR_INVALID, "out_features must be 3 (Y, Cb, Cr / the three detail bands)");
    if (cfg->wavelet_levels != 1)
      return fail(SF_ERR_INVALID, "wavelet_levels must be 1: the reference's single-level inverse DWT receives 3 * levels bands "
                                  "and fails for more");
    SF_TRY(wavelet_check_network(cfg));
    if (cfg->scratch_format != 0 && cfg->scratch_format != 16)
      return fail(SF_ERR_INVALID, "WaveletSiren runs scratch format 16 (0 = auto resolves to it): format 8 takes its fp8 delta "
                                  "scale from the fused residual, which a WaveletSiren pass does not form");
    SF_TRY(wavelet_check_image(cfg->height, cfg->width, cfg->chunk_pixels));
    const int H = cfg->height, n = (H + 5) / 2;
    sf_config sc = wavelet_sub_config(cfg, n, n);
    sc.beta1 = cfg->beta1; sc.beta2 = cfg->beta2; sc.eps = cfg->eps;
    g = {H, H, 0, H};
    return wavelet_subs(sc, false, sub);
  };
  auto init = [&](sf_engine* h, const Grid& g) -> int {
    wavelet_begin(h, sub, g.height);
    const long nn = h->wv.sub[0]->npix;
    const bool one = nn <= h->wv.sub[0]->chunk_px;
    h->chunk_px = one ? h->npix : 1;   // (sf_step's graph replay covers single-chunk fits only)
    const int64_t P0 = h->wv.sub[0]->P;
    // the sub-networks' dL/dout pre-scale comes from the 3 H^2 values of the full image (what the loss mean divides by)
    const float gpre = (float)exp2(ceil(log2(3.0 * h->n_total)) + 2.0);
    for (sf_engine* s : h->wv.sub) s->gpre = gpre;
    SF_TRY(alloc_state(h, true));
    SF_TRY(dev_alloc(h, h->wv.pred, (size_t)2 * nn * 3 * 4));
    SF_TRY(dev_alloc(h, h->wv.g, (size_t)h->npix * 3 * 4));
    if (!one) SF_TRY(dev_alloc(h, h->wv.gl, (size_t)2 * nn * 3 * 4));
    if (!cfg->outermost_linear) SF_TRY(dev_alloc(h, h->wv.dfac, (size_t)2 * nn * 3 * 4));
    SF_TRY(alloc_sse(h, (h->npix + kWvThreads - 1) / kWvThreads));
    for (int s = 0; s < 2; ++s) {   // the sub-handles' state: the two halves of the joint vectors
      sf_engine* e = h->wv.sub[s];
      e->params = h->params + s * P0; e->grads = h->grads + s * P0; e->m = h->m + s * P0; e->v = h->v + s * P0;
      e->mask = h->mask + s * P0;
      if (h->wv.dfac) e->wv.dfac_out = h->wv.dfac + (size_t)s * nn * 3;
    }
    return SF_OK;
  };
  return create_with(cfg, out, &sf_wavelet_config::in_features, Model::Wavelet, false, check, init);
} SF_CATCH

int sf_wavelet_debug(sf_handle* h, int32_t which, const float* in0, const float* in1, const float* img, float* out0,
                     float* out1) try {
  if (!h || !in0 || !out0 || !out1 || (which == 0 && !in1)) return fail(SF_ERR_INVALID, "null argument");
  if (h->render) return fail(SF_ERR_INVALID, "sf_wavelet_debug: a render handle (sf_wavelet_render_create) runs sf_wavelet_render only");
  if (h->model != Model::Wavelet) return fail(SF_ERR_INVALID, "sf_wavelet_debug: not a WaveletSiren handle (sf_wavelet_create)");
  if (which != 0 && which != 1) return fail(SF_ERR_INVALID, "sf_wavelet_debug: which must be 0 or 1");
  DevGuard dev_guard(h->cfg.device);
  WvArgs a = zeroed<WvArgs>();
  a.H = h->cfg.height; a.n = h->wv.n; a.up = h->wv.up;
  a.gscale = (float)(2.0 / (3.0 * h->n_total));
  a.dscale = 1.0f;
  if (which == 0) {
    a.lf = in0; a.hf = in1; a.img = img; a.pred = out0; a.g = img ? out1 : nullptr; a.sse_part = h->sse_part;
    return launch(h, k_wv_compose, (h->npix + kWvThreads - 1) / kWvThreads, kWvThreads, 0, a);
  }
  a.g = const_cast<float*>(in0); a.gl_lf = out0; a.gl_hf = out1;
  const long nn = (long)h->wv.n * h->wv.n;
  return launch(h, k_wv_adjoint, (nn + kWvThreads - 1) / kWvThreads, kWvThreads, 0, a);
} SF_CATCH

}  // extern "C"
