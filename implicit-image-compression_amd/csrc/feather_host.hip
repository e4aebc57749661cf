// feather_host.hip — Feathermap (structured multi-hashing, feather_kernels.hip) on the host: materialisation and adjoint as
// the Adam step of siren_fit.hip calls them, the four sf_feather_* entry points of a training handle, and the two of a
// render handle (sf_feather_render_attach / sf_feather_render_load: the feather vector and k_fth_mat<true>, nothing of the
// adjoint).  Included by siren_fit.hip.

namespace {

// Feathermap: V = V1 V2 and W = scaler * V into the engine's flat parameters; the weight images follow at the next
// refresh_images
int feather_materialise(sf_engine* h) {
  const FthArgs& a = h->fth.args;
  const dim3 grid((unsigned)((a.rows_used + kFthTile - 1) / kFthTile), (unsigned)((a.n + kFthTile - 1) / kFthTile));
  Launch L(h, K_FTH_MAT, 2.0 * a.rows_used * a.n * a.m, 4.0 * (2.0 * a.n * a.m + 2.0 * a.P));
  SF_TRY(with_bool(h->render, [&](auto render) { return launch(h, k_fth_mat<decltype(render)::value>, grid, 256, 0, a); }));
  h->images_dirty = true;
  return SF_OK;
}

// What sf_feather_attach and sf_feather_render_attach share, under the caller's name fn: the depth, the logical layer sizes
// against the handle's, the segments of V.view(-1) on the handle's flat layout, n and m.  Fills a.seg, n, m, P, rows_used.
int feather_geometry(const sf_engine* h, const std::string& fn, int64_t n, int64_t m, int32_t n_layers,
                     const int32_t* logical_out, const int32_t* logical_in, FthArgs& a) {
  if (n_layers != h->D) return fail(SF_ERR_INVALID, fn + ": n_layers must equal the handle's depth");
  const int D = h->D;
  long P = 0;
  for (int l = 0; l < D; ++l) {
    const int in_p = l == 0 ? h->cfg.in_features : h->WD, out_p = l == D - 1 ? h->cfg.out_features : h->WD;
    const int in = logical_in[l], outn = logical_out[l];
    if (in < 1 || outn < 1 || in > in_p || outn > out_p || (l == 0 && in != in_p) || (l == D - 1 && outn != out_p))
      return fail(SF_ERR_INVALID, fn + ": logical layer sizes do not fit the handle");
    a.seg.start[2 * l] = P; a.seg.base[2 * l] = h->off_w[l]; a.seg.cols[2 * l] = in; a.seg.stride[2 * l] = in_p;
    P += (long)in * outn;
    a.seg.start[2 * l + 1] = P; a.seg.base[2 * l + 1] = h->off_b[l]; a.seg.cols[2 * l + 1] = outn;
    a.seg.stride[2 * l + 1] = outn;
    P += outn;
  }
  a.seg.nseg = 2 * D;
  a.seg.start[2 * D] = P;
  if (n < 1 || m < 1 || n > 46340 || m > n || n * n < P)
    return fail(SF_ERR_INVALID, fn + ": need 1 <= m <= n <= 46340 and n^2 >= the parameter count");
  a.n = (int)n; a.m = (int)m; a.P = P;
  a.rows_used = (int)((P + n - 1) / n);
  return SF_OK;
}

// Feathermap adjoint of the engine's dense gradient: dV1, dV2 and dscaler into fth_g (two launches)
int feather_adjoint(sf_engine* h) {
  const FthArgs& a = h->fth.args;
  {
    Launch L(h, K_FTH_GRAD, 2.0 * a.P, 4.0 * 4.0 * a.P);
    SF_TRY(launch(h, k_fth_grad, a.g_blocks + a.nchunks, 256, 0, a));
  }
  {
    const int t2 = (a.m + kFthTile - 1) / kFthTile * a.t2n;
    Launch L(h, K_FTH_DV, 2.0 * (double)a.n * a.m * (a.n + a.rows_used), 4.0 * ((double)a.n * a.n + 4.0 * a.n * a.m));
    SF_TRY(launch(h, k_fth_dv, a.t1 + t2 + 1, 256, 0, a));
  }
  h->fth.fresh = true;
  return SF_OK;
}

}  // namespace

extern "C" {

// ---- Feathermap (structured multi-hashing, feather_kernels.hip) ---------------------------------------------------
int sf_feather_attach(sf_handle* h, int64_t n, int64_t m, int32_t n_layers, const int32_t* logical_out,
                      const int32_t* logical_in) try {
  if (!h || !logical_out || !logical_in) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_attach");
  switch (h->model) {
    case Model::Siren: break;
    case Model::Fourier:
    case Model::Wavelet: return fail(SF_ERR_INVALID, "sf_feather_attach: Feathermap runs on SIREN handles only");
  }
  if (h->fth.attached) return fail(SF_ERR_INVALID, "sf_feather_attach: the handle already has a feather state");
  if (h->cfg.row_begin != 0 || h->cfg.row_end != h->cfg.height)
    return fail(SF_ERR_INVALID, "sf_feather_attach: Feathermap fits the whole image (no pixel split)");
  if (h->has_mask) return fail(SF_ERR_INVALID, "sf_feather_attach: the handle has a mask (Feathermap is dense)");
  FthArgs a = zeroed<FthArgs>();
  SF_TRY(feather_geometry(h, "sf_feather_attach", n, m, n_layers, logical_out, logical_in, a));
  const int D = h->D;
  const long P = a.P;
  std::vector<long> chunks;
  std::vector<int> chunk0;
  for (int k = 0; k < a.seg.nseg; ++k) {
    chunk0.push_back((int)(chunks.size() / 3));
    for (long b = a.seg.start[k]; b < a.seg.start[k + 1]; b += kFthChunk) {
      chunks.push_back(k); chunks.push_back(b); chunks.push_back(std::min(b + kFthChunk, a.seg.start[k + 1]));
    }
  }
  chunk0.push_back((int)(chunks.size() / 3));
  a.nchunks = (int)(chunks.size() / 3);
  a.g_blocks = (int)std::min<long>((P + 255) / 256, 8L * h->dw_wg);
  a.t1n = (a.m + kFthTile - 1) / kFthTile;
  a.t1 = (a.n + kFthTile - 1) / kFthTile * a.t1n;
  a.t2n = (a.n + kFthTile - 1) / kFthTile;
  const long nf = 2 * n * m + 2L * D;
  DevGuard dev_guard(h->cfg.device);
  // (a failure part-way leaves a handle without feather state: h->fth.attached stays false, nothing reads the fth_* fields, and
  //  what was allocated stays on the owned list until sf_destroy)
  if (dev_alloc(h, h->fth.p, nf * 4) || dev_alloc(h, h->fth.g, nf * 4) || dev_alloc(h, h->fth.m, nf * 4) ||
      dev_alloc(h, h->fth.v, nf * 4) || dev_alloc(h, h->fth.V, P * 4) || dev_alloc(h, h->fth.G, n * n * 4) ||
      dev_alloc(h, h->fth.part, (size_t)a.nchunks * 4) || dev_alloc(h, h->fth.chunks, chunks.size() * sizeof(long)) ||
      dev_alloc(h, h->fth.chunk0, chunk0.size() * sizeof(int))) {
    (void)hipGetLastError();
    return fail(SF_ERR_NOMEM, "hipMalloc failed (feather state)");
  }
  HIPCHK(hipMemcpy(h->fth.chunks, chunks.data(), chunks.size() * sizeof(long), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->fth.chunk0, chunk0.data(), chunk0.size() * sizeof(int), hipMemcpyHostToDevice));
  for (float* p : {h->fth.p, h->fth.g, h->fth.m, h->fth.v}) HIPCHK(hipMemsetAsync(p, 0, nf * 4, h->ctx->stream));
  HIPCHK(hipMemsetAsync(h->fth.V, 0, P * 4, h->ctx->stream)); HIPCHK(hipMemsetAsync(h->fth.G, 0, n * n * 4, h->ctx->stream));
  HIPCHK(hipMemsetAsync(h->params, 0, h->P * 4, h->ctx->stream));   // padded slots stay exactly 0
  a.fp = h->fth.p; a.fg = h->fth.g; a.V = h->fth.V; a.G = h->fth.G; a.W = h->params; a.dW = h->grads;
  a.chunks = h->fth.chunks; a.seg_chunk0 = h->fth.chunk0; a.part = h->fth.part;
  h->fth.args = a;
  h->fth.nf = nf;
  h->fth.attached = true;
  h->fth.fresh = false;
  if (h->graph.exec) { hipGraphExecDestroy(h->graph.exec); h->graph.exec = nullptr; }   // a captured step holds the dense Adam
  h->images_dirty = true;
  return SF_OK;
} SF_CATCH

int sf_feather_state_ptr(sf_handle* h, int32_t which, float** dev_ptr, int64_t* len) try {
  if (!h || !dev_ptr) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_state_ptr");
  if (!h->fth.attached) return fail(SF_ERR_STATE, "sf_feather_state_ptr: no feather state (sf_feather_attach)");
  float* ps[] = {h->fth.p, h->fth.g, h->fth.m, h->fth.v, h->fth.V};
  if (which < 0 || which > 4) return fail(SF_ERR_INVALID, "bad feather state selector");
  *dev_ptr = ps[which];
  if (len) *len = which == 4 ? h->fth.args.P : h->fth.nf;
  return SF_OK;
} SF_CATCH

int sf_feather_materialise(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_materialise");
  if (!h->fth.attached) return fail(SF_ERR_STATE, "sf_feather_materialise: no feather state (sf_feather_attach)");
  DevGuard dev_guard(h->cfg.device);
  return feather_materialise(h);
} SF_CATCH

int sf_feather_adjoint(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_adjoint");
  if (!h->fth.attached) return fail(SF_ERR_STATE, "sf_feather_adjoint: no feather state (sf_feather_attach)");
  DevGuard dev_guard(h->cfg.device);
  return feather_adjoint(h);
} SF_CATCH

// ---- inference: the feather vector on a render handle ---------------------------------------------------------------
int sf_feather_render_attach(sf_handle* h, int64_t n, int64_t m, int32_t n_layers, const int32_t* logical_out,
                             const int32_t* logical_in) try {
  if (!h || !logical_out || !logical_in) return fail(SF_ERR_INVALID, "null argument");
  if (!h->render)
    return fail(SF_ERR_INVALID, "sf_feather_render_attach: a training handle takes sf_feather_attach; this call is for a "
                                "handle from sf_render_create");
  switch (h->model) {
    case Model::Siren: break;
    case Model::Fourier:
    case Model::Wavelet:
      return fail(SF_ERR_INVALID, "sf_feather_render_attach: Feathermap runs on SIREN render handles (sf_render_create) only");
  }
  if (h->wide)
    return fail(SF_ERR_INVALID, "sf_feather_render_attach: a wide render handle (sf_wide_render_create) takes dense parameters; "
                                "the Feathermap render path is built for hidden 32 .. 256 (sf_render_create)");
  if (h->fth.attached) return fail(SF_ERR_INVALID, "sf_feather_render_attach: the handle already has a feather state");
  FthArgs a = zeroed<FthArgs>();
  SF_TRY(feather_geometry(h, "sf_feather_render_attach", n, m, n_layers, logical_out, logical_in, a));
  const long nf = 2 * n * m + 2L * h->D;
  DevGuard dev_guard(h->cfg.device);
  if (dev_alloc(h, h->fth.p, nf * 4)) {
    (void)hipGetLastError();
    return fail(SF_ERR_NOMEM, "hipMalloc failed (feather vector)");
  }
  HIPCHK(hipMemsetAsync(h->fth.p, 0, nf * 4, h->ctx->stream));
  HIPCHK(hipMemsetAsync(h->params, 0, h->P * 4, h->ctx->stream));   // padded slots stay exactly 0
  a.fp = h->fth.p; a.W = h->params;   // (every other pointer stays null: k_fth_mat<true> reads fp and writes W)
  h->fth.args = a;
  h->fth.nf = nf;
  h->fth.attached = true;
  h->fth.loaded = false;
  h->images_dirty = true;
  return SF_OK;
} SF_CATCH

int sf_feather_render_load(sf_handle* h, const float* feather_dev) try {
  if (!h || !feather_dev) return fail(SF_ERR_INVALID, "null argument");
  if (!h->render || !h->fth.attached)
    return fail(SF_ERR_STATE, "sf_feather_render_load: no feather state (sf_feather_render_attach on a handle from "
                              "sf_render_create)");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(h->fth.p, feather_dev, h->fth.nf * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
  SF_TRY(feather_materialise(h));
  h->fth.loaded = true;
  return SF_OK;
} SF_CATCH

}  // extern "C"
