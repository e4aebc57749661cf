// fourier_host.hip — FourierNet on the host (kernels: fourier_kernels.hip): weight images, a chunk's forward and backward, the creator of training
// and render handles (fourier_render.hip), sf_fourier_create / sf_set_encoding.  Included by siren_fit.hip.

namespace {

// ---------------------------------------------------------------------------------------------------------
// FourierNet (fourier_kernels.hip): per chunk k_ff_fwd -> k_ff_bwd -> k_ff_dw per layer, each followed by the
// fixed-order slab reduction into the flat gradient; Adam, graph replay and the rest are shared with SIREN
// ---------------------------------------------------------------------------------------------------------
int refresh_images_fourier(sf_engine* h) {
  FfImgArgs a = zeroed<FfImgArgs>();
  a.params = h->params; a.nlin = h->D; a.img = h->ff.img;
  for (int l = 0; l < h->D; ++l) {
    a.off_w[l] = h->off_w[l];
    a.in[l] = l == 0 ? h->ff.MS : h->WD;
    a.out[l] = l == h->D - 1 ? h->cfg.out_features : h->WD;
    // segments in memory order: f0, (b0: empty), f1, b1, f2, b2, ...
    a.start[2 * l] = h->ff.img_f[l];
    a.start[2 * l + 1] = l == 0 ? h->ff.img_f[1] : h->ff.img_b[l];
  }
  a.start[2 * h->D] = h->ff.img_n;
  Launch L(h, K_IMAGES, 0, (double)h->ff.img_n * 16.0);
  SF_TRY(launch(h, k_ff_images, (h->ff.img_n + 255) / 256, 256, 0, a));
  h->images_dirty = false;
  return SF_OK;
}

// what every kernel of the FourierNet chain is given for the chunk at pixel pix0: coordinates, encoding, weight images,
// biases; the caller adds its planes and outputs (the RENDER form of k_ff_fwd touches none of H / G / Z / tgt / sse_part)
FfArgs ff_args_base(const sf_engine* h, long pix0) {
  FfArgs fa = zeroed<FfArgs>();
  fa.gh = h->gh; fa.gw = h->gw; fa.W = h->cfg.width; fa.pix0 = pix0; fa.npix = h->npix; fa.cp = h->chunk_px;
  fa.Btab = h->ff.B; fa.MS = h->ff.MS; fa.nlin = h->D; fa.img = h->ff.img; fa.params = h->params;
  for (int l = 0; l < h->D; ++l) { fa.img_f[l] = h->ff.img_f[l]; fa.img_b[l] = h->ff.img_b[l]; fa.off_b[l] = h->off_b[l]; }
  return fa;
}
// k_ff_fwd<WD, false>, k_ff_fwd<WD, true>, k_ff_bwd<WD>, k_ff_fwd<WD, false, true>, k_ff_fwd<WD, false, true, 16>,
// k_ff_fwd<WD, false, false, kFfEvalBits> (sf_eval)
enum FfKernel { kFfEval, kFfTrain, kFfBwd, kFfRender, kFfRender16, kFfEval8 };
int launch_ff(sf_engine* h, const FfArgs& a, int n_super, FfKernel which) {
  return with_width(h, [&](auto wd) {
    constexpr int WD = decltype(wd)::value;
    auto go = [&](auto kernel) { return launch(h, kernel, n_super, kFfThreads, kFfLdsBytes, a); };
    return which == kFfEval ? go(k_ff_fwd<WD, false>) : which == kFfTrain ? go(k_ff_fwd<WD, true>)
           : which == kFfBwd ? go(k_ff_bwd<WD>) : which == kFfRender ? go(k_ff_fwd<WD, false, true>)
           : which == kFfRender16 ? go(k_ff_fwd<WD, false, true, 16>) : go(k_ff_fwd<WD, false, false, kFfEvalBits>);
  });
}

// ... and for the forward and the backward of a training handle's chunk: the planes, the target, the outputs
FfArgs ff_chunk_args(const sf_engine* h, const Chunk& k, float* pred, float* sse_part) {
  FfArgs fa = ff_args_base(h, k.pix0);
  fa.H = h->ff.H; fa.G = h->ff.G; fa.Z = h->ff.Z;
  fa.tgt = h->img; fa.pred = pred; fa.sse_part = sse_part;
  fa.gscale = gscale(h);
  return fa;
}

// The forward of chunk c (k_ff_fwd), training or evaluation form: the prediction to pred (or null), the chunk's SSE partials
// to sse_part; n_part: how many it wrote (one per 256-pixel group).  sse8_part (sf_eval, with neither train nor pred): the
// EVAL form, which stores nothing but the two kinds of partials
int fourier_fwd_chunk(sf_engine* h, long c, bool train, float* pred, float* sse_part, int& n_part, unsigned long long* sse8_part = nullptr) {
  const int WD = h->WD, D = h->D, MS = h->ff.MS;
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  const double npx = (double)k.n_super * kSuper;
  FfArgs fa = ff_chunk_args(h, k, pred, sse_part);
  if (sse8_part) fa.sse8_part = sse8_part;
  const double f_hidden = (double)(D - 2) * WD * WD;
  n_part = k.n_super;
  Launch L(h, K_FWD, 2.0 * ((double)MS * WD + f_hidden + 32.0 * WD) * npx,
           npx * (12.0 + (train ? (D - 1) * WD * 2.0 + 6.0 : 0.0)));
  return launch_ff(h, fa, k.n_super, sse8_part ? kFfEval8 : train ? kFfTrain : kFfEval);
}

// The backward of chunk c after its training forward (which ran with the same sse_part and no prediction: the kernels receive
// the forward's argument struct): k_ff_bwd, then k_ff_dw per layer, last first, each followed by the slab reduction
int fourier_bwd_chunk(sf_engine* h, long c, float* sse_part) {
  const int WD = h->WD, D = h->D, MS = h->ff.MS;
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  const int n_super = k.n_super;
  const double npx = (double)n_super * kSuper;
  const FfArgs fa = ff_chunk_args(h, k, nullptr, sse_part);
  const double f_hidden = (double)(D - 2) * WD * WD;
  {
    Launch L(h, K_BWD_HIDDEN, 2.0 * (f_hidden + 16.0 * WD) * npx, npx * (6.0 + (D - 1) * WD * 4.0));
    SF_TRY(launch_ff(h, fa, n_super, kFfBwd));
  }
  // weight gradients, last layer first: per-workgroup slabs over contiguous pixel ranges, then k_reduce*
  int gx = (int)(npx / kSuper);
  if (gx > h->ff.dw_wgs) gx = h->ff.dw_wgs;
  long ppw = ((long)npx + gx - 1) / gx;
  ppw = (ppw + 15) / 16 * 16;
  gx = (int)(((long)npx + ppw - 1) / ppw);
  for (int l = D - 1; l >= 0; --l) {
    const bool last = l == D - 1;
    FfDwArgs da = zeroed<FfDwArgs>();
    da.rows = last ? h->cfg.out_features : WD;
    da.A = last ? h->ff.Z : h->ff.G + (size_t)l * WD * h->chunk_px;
    da.Bm = l == 0 ? nullptr : h->ff.H + (size_t)(l - 1) * WD * h->chunk_px;
    da.in = l == 0 ? MS : WD;
    da.n_it = da.in / 32;
    const int NI = da.n_it < 4 ? da.n_it : 4;
    da.n_groups = ((da.rows + 31) / 32) * (da.n_it / NI);
    da.cp = h->chunk_px; da.n_px = (long)npx; da.ppw = ppw; da.slab = h->slab; da.e = fa;
    {
      Launch L(h, l == 0 ? K_DW_FIRST : last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * 32.0 * ((da.rows + 31) / 32) * da.in * npx,
               npx * 2.0 * (32.0 * ((da.rows + 31) / 32) + (l == 0 ? 0.0 : da.in)));
      const dim3 grid(gx, (da.n_groups + 3) / 4);
      SF_TRY(with_bool(l == 0, [&](auto e0) {
        constexpr bool E0 = decltype(e0)::value;
        return NI == 1 ? launch(h, k_ff_dw<1, E0>, grid, 256, 0, da) : NI == 2 ? launch(h, k_ff_dw<2, E0>, grid, 256, 0, da)
                                                                               : launch(h, k_ff_dw<4, E0>, grid, 256, 0, da);
      }));
    }
    const long n = (long)da.rows * da.in + da.rows;
    Launch L(h, K_REDUCE, 0, (double)gx * n * 4.0);
    if (!last) {   // slab layout [W rows*in | b rows] == flat gradient layout of the layer
      const int n4 = (int)(n / 4);
      SF_TRY(launch(h, k_reduce_vec, (n4 + 7) / 8, 256, 0, h->slab, gx, n, n4, h->grads + h->off_w[l], c > 0, 1.0f / h->gpre,
                    nullptr, nullptr));
    } else {
      ReduceArgs ra = zeroed<ReduceArgs>();
      ra.slab = h->slab; ra.n_wg = gx; ra.slab_rows = da.rows; ra.slab_cols = da.in; ra.rows_out = da.rows; ra.cols_out = da.in;
      ra.mode = 0; ra.gW = h->grads + h->off_w[l]; ra.gb = h->grads + h->off_b[l]; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre;
      SF_TRY(launch_reduce(h, ra));
    }
  }
  return SF_OK;
}

// FourierNet handle: the same sf_engine, run by fourier_kernels.hip (the two chunk functions above); every other entry point is shared.
// sf_fourier_create and sf_fourier_render_create (fourier_render.hip): one validation, one geometry; a render handle
// allocates the parameters, the weight images (forward and backward: k_ff_images writes both, a few MB at most),
// encoding.B and the two coordinate vectors
int create_fourier(const sf_fourier_config* cfg, sf_handle** out, bool render) {
  auto check = [&](Grid& g) -> int {
    if (cfg->out_features != 3) return fail(SF_ERR_INVALID, "out_features must be 3 (the fused sigmoid / loss epilogue is RGB)");
    if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256)
      return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128 or 256 for FourierNet (other widths: zero-pad on the host)");
    if (cfg->map_size != 64 && cfg->map_size != 128 && cfg->map_size != 256 && cfg->map_size != 512)
      return fail(SF_ERR_INVALID, "map_size must be 64, 128, 256 or 512");
    if (cfg->n_linear < 2 || cfg->n_linear > kFfMaxLinear) return fail(SF_ERR_INVALID, "n_linear must be 2..12");
    if (cfg->compute_dtype != SF_F16) return fail(SF_ERR_INVALID, "FourierNet runs fp16 operands only (compute_dtype SF_F16)");
    if (cfg->height < 1 || cfg->width < 1) return fail(SF_ERR_INVALID, "bad image size");
    if ((double)cfg->height * (double)cfg->width >= 2147483648.0) return fail(SF_ERR_INVALID, "image too large: height * width must stay below 2^31");
    if (cfg->chunk_pixels < 0) return fail(SF_ERR_INVALID, "chunk_pixels must be >= 0");
    g = {cfg->height, cfg->width, 0, cfg->height};
    return SF_OK;
  };
  auto init = [&](sf_engine* h, const Grid&) -> int {
    h->cfg = zeroed<sf_config>();
    h->cfg.abi_version = cfg->abi_version;
    h->cfg.height = cfg->height; h->cfg.width = cfg->width; h->cfg.row_begin = 0; h->cfg.row_end = cfg->height;
    h->cfg.in_features = cfg->in_features; h->cfg.out_features = cfg->out_features; h->cfg.hidden = cfg->hidden;
    h->cfg.depth = cfg->n_linear; h->cfg.compute_dtype = cfg->compute_dtype;
    h->cfg.beta1 = cfg->beta1; h->cfg.beta2 = cfg->beta2; h->cfg.eps = cfg->eps;
    h->cfg.device = cfg->device; h->cfg.stream = cfg->stream; h->cfg.chunk_pixels = cfg->chunk_pixels;
    h->cfg.scratch_format = 16;
    adam_defaults(h);
    h->D = cfg->n_linear; h->WD = cfg->hidden; h->ff.MS = cfg->map_size;
    const int WD = h->WD, D = h->D, MS = h->ff.MS;
    layer_offsets(h, MS);   // layers.{2l}.weight, layers.{2l}.bias (encoding.B is frozen and lives outside)
    long img = 0;
    for (int l = 0; l < D; ++l) {   // the weight images, in 16-byte units: forward of every layer, backward of layers >= 1
      const int in = l == 0 ? MS : WD, outn = l == D - 1 ? cfg->out_features : WD;
      h->ff.img_f[l] = img; img += (long)((outn + 31) / 32) * (in / 16) * 64;
      if (l > 0) { h->ff.img_b[l] = img; img += (long)(in / 32) * ((outn + 15) / 16) * 64; }
    }
    h->ff.img_n = img;
    h->gpre = (float)exp2(ceil(log2((double)cfg->out_features * (double)cfg->height * (double)cfg->width)) + 2.0);
    // chunking: 4 Mi pixels, or fewer when the activation + gradient planes of a chunk would pass 16 GiB
    const double px_bytes = (double)(D - 1) * WD * 4.0 + 8.0;
    // (never more than 4 Mi: the kernels address a [WD][chunk] plane with 32-bit offsets)
    const long want = cfg->chunk_pixels > 0 ? (long)cfg->chunk_pixels : (long)fmin((double)(1L << 22), 17179869184.0 / px_bytes);
    const long chunk = chunk_pixels(std::min(want, 1L << 22), h->npix);
    h->chunk_px = chunk;
    h->ff.dw_wgs = 4 * h->dw_wg;
    long slab_row = (long)WD * MS + WD;
    if ((long)WD * WD + WD > slab_row) slab_row = (long)WD * WD + WD;
    SF_TRY(alloc_state(h, !render));   // (render: no gradient, moments or mask)
    SF_TRY(dev_alloc(h, h->ff.img, (size_t)h->ff.img_n * 16));
    SF_TRY(dev_alloc(h, h->ff.B, (size_t)cfg->in_features * (MS / 2) * 4));
    SF_TRY(dev_alloc(h, h->gh, (size_t)cfg->height * 4));
    SF_TRY(dev_alloc(h, h->gw, (size_t)cfg->width * 4));
    if (render) return SF_OK;   // no activation / gradient planes, slab or SSE partials: k_ff_fwd's RENDER form spills nothing
    SF_TRY(dev_alloc(h, h->ff.H, (size_t)(D - 1) * WD * chunk * 2));
    SF_TRY(dev_alloc(h, h->ff.G, (size_t)(D - 1) * WD * chunk * 2));
    SF_TRY(dev_alloc(h, h->ff.Z, (size_t)4 * chunk * 2));
    SF_TRY(dev_alloc(h, h->slab, (size_t)h->ff.dw_wgs * slab_row * 4));
    return alloc_sse(h, chunked_sse_parts(h));
  };
  return create_with(cfg, out, &sf_fourier_config::in_features, Model::Fourier, render, check, init);
}

}  // namespace

extern "C" {

int sf_fourier_create(const sf_fourier_config* cfg, sf_handle** out) try { return create_fourier(cfg, out, false); } SF_CATCH

int sf_set_encoding(sf_handle* h, const float* B_dev) try {
  if (!h || !B_dev) return fail(SF_ERR_INVALID, "null argument");
  if (h->model != Model::Fourier) return fail(SF_ERR_INVALID, "sf_set_encoding: not a FourierNet handle (sf_fourier_create / sf_fourier_render_create)");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(h->ff.B, B_dev, (size_t)h->cfg.in_features * (h->ff.MS / 2) * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
  h->ff.have_B = true;
  return SF_OK;
} SF_CATCH

}  // extern "C"
