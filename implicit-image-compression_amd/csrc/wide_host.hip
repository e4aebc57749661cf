// wide_host.hip — SIREN handles of hidden 512 / 1024 on the host: weight images, a chunk's forward and backward and the render
// loop of a wide render handle over the layer-at-a-time kernels of siren_wide.hip.  Included by siren_fit.hip after siren_host.hip, whose layer-0 and reduction launchers it shares.

namespace {

// ---------------------------------------------------------------------------------------------------------
// wide path (hidden 512 / 1024): layer-at-a-time kernels of siren_wide.hip
// ---------------------------------------------------------------------------------------------------------
// (a render handle has the forward images and the tables only: no transposed image, no fp8 scale)
int refresh_images_wide(sf_engine* h) {
  const int WD = h->WD, D = h->D, NBLK = WD / 256, KS = WD / 16;
  const bool f16 = h->cfg.compute_dtype == SF_F16;
  Launch L(h, K_IMAGES, 0, (double)(D - 2) * WD * WD * 8.0);
  {
    WTabArgs t = zeroed<WTabArgs>();
    t.params = h->params; t.depth = D; t.WD = WD; t.out_features = h->cfg.out_features;
    t.off_w0 = h->off_w[0]; t.off_b0 = h->off_b[0];
    for (int l = 0; l < D; ++l) t.off_b[l] = h->off_b[l];
    t.wscale = h->wscale; t.hscale = (float)((double)h->cfg.hidden_omega_0 / kTwoPi);
    t.l0tab = h->l0tab; t.bias = h->biasw;
    long n = (long)(D - 2) * WD;
    if (n < WD) n = WD;
    SF_TRY(launch(h, k_wtables, (n + 255) / 256, 256, 0, t));
  }
  if (h->d8 && h->lsc) SF_TRY(launch_fp8_scales(h));   // per-layer fp8 delta scales, as at width <= 256
  auto image = [&](int l, bool transpose, int OT, int n_ob, int n_chunk, float scale, uint16_t* dst) {
    WImgArgs a = zeroed<WImgArgs>();
    a.link = (transpose && h->d8 && h->lsc) ? h->lsc + l : nullptr;
    a.W = h->params + h->off_w[l];
    a.rows = l == D - 1 ? h->cfg.out_features : WD; a.cols = WD;
    a.transpose = transpose; a.OT = OT; a.n_ob = n_ob; a.n_chunk = n_chunk; a.scale = scale; a.f16 = f16; a.dst = dst;
    const long total = (long)n_ob * n_chunk * OT * 4 * 512;
    return launch(h, k_wimage, (total + 255) / 256, 256, 0, a);
  };
  for (int l = 1; l <= D - 2; ++l) {
    SF_TRY(image(l, false, 8, NBLK, KS / 4, (float)((double)h->cfg.hidden_omega_0 / kTwoPi), h->wf + (size_t)(l - 1) * WD * WD));
    if (!h->render) SF_TRY(image(l, true, 8, NBLK, KS / 4, l - 1 == 0 ? h->cfg.first_omega_0 : h->cfg.hidden_omega_0, h->wb + (size_t)(l - 1) * WD * WD));
  }
  SF_TRY(image(D - 1, false, 1, 1, KS / 4, h->wscale, h->wf_last));
  if (!h->render) SF_TRY(image(D - 1, true, 8, NBLK, 1, D - 2 == 0 ? h->cfg.first_omega_0 : h->cfg.hidden_omega_0, h->wb_last));
  h->images_dirty = false;
  return SF_OK;
}

// persistent grid of the wide GEMMs: one workgroup per CU, a multiple of 8 * n_ob (so XCD and output block are loop
// invariants), at most one workgroup per tile
unsigned wgemm_grid(const sf_engine* h, int n_ob, unsigned tiles) {
  const unsigned pg = (unsigned)(h->dw_wg / (8 * n_ob) * (8 * n_ob));
  return pg == 0 || pg > tiles ? tiles : pg;
}
// (render_bits: 0, or the sample width of a render handle's launch - the RENDER forms of MODE 0 and 1; eval8: the EVAL form
// of MODE 1, a.sse8_part set)
template <int MODE>
int launch_wgemm(sf_engine* h, const WGemmArgs& a, int n_super, int n_ob, int render_bits = 0, bool eval8 = false) {
  WGemmArgs b = a;
  b.n_super = n_super; b.n_ob = n_ob;
  const unsigned grid = (unsigned)((n_super + 7) / 8 * 8 * n_ob);
  if constexpr (MODE == 1) {
    if (render_bits)
      return with_bool(render_bits == 16, [&](auto wide) {
        constexpr int BITS = decltype(wide)::value ? 16 : 8;
        return with_op(h, [&](auto op) { return launch(h, k_wgemm<decltype(op), true, BITS>, grid, 512, WGemmLds::bytes, b); });
      });
    if (eval8) return with_op(h, [&](auto op) { return launch(h, k_wgemm<OpEval<decltype(op)>>, grid, 512, WGemmLds::bytes, b); });
    return with_op(h, [&](auto op) { return launch(h, k_wgemm<decltype(op)>, grid, 512, WGemmLds::bytes, b); });
  } else {
    if constexpr (MODE == 0) {
      if (render_bits)
        return with_op(h, [&](auto op) {
          return launch(h, k_wgemm2<0, decltype(op), false, false, false, true>, wgemm_grid(h, n_ob, grid), 512, WGemm2Lds::bytes, b);
        });
    }
    if constexpr (MODE == 2) {
      if (h->d8) {   // fp8 deltas (format 8): out always, in for every launch below the last layer's
        const unsigned pg8 = wgemm_grid(h, n_ob, grid);
        return a.fscale ? launch(h, k_wgemm2<2, OpF16, true, false, true>, pg8, 512, WGemm2Lds::bytes, b)
                        : launch(h, k_wgemm2<2, OpF16, true, true, true>, pg8, 512, WGemm2Lds::bytes, b);
      }
    }
    const size_t lds = WGemm2Lds::bytes;
    const unsigned pgrid = wgemm_grid(h, n_ob, grid);    // persistent: one workgroup per CU
    if (h->s8 && (MODE == 0 || b.Pprev))                    // phase bytes (format 12; fp16 only: sf_create)
      return launch(h, k_wgemm2<MODE, OpF16, true>, pgrid, 512, lds, b);
    return with_op(h, [&](auto op) { return launch(h, k_wgemm2<MODE, decltype(op)>, pgrid, 512, lds, b); });
  }
}

// What the last layer of a wide forward walk writes: the prediction (or null) and either the training / evaluation outputs -
// the chunk's SSE partials and, if train, dL/dout - or samples of `bits` bits at `samples` (or null)
struct WideOut { float* pred; float* sse_part; bool train; void* samples; int bits; unsigned long long* sse8_part = nullptr; };

// The forward walk of chunk k, layer at a time: k_wlayer0, k_wgemm2<0> per hidden layer, k_wgemm.  o.bits = 0: the training /
// evaluation forms under K_FWD - layer l writes its own phase and activation planes.  o.bits = 8 / 16: the RENDER forms
// under K_RENDER - activations only, through the handle's two planes in turn (layer l reads plane (l - 1) & 1 and writes
// plane l & 1)
int wide_fwd_walk(sf_engine* h, const Chunk& k, const WideOut& o) {
  const int WD = h->WD, D = h->D, KS = WD / 16, NBLK = WD / 256;
  const bool render = o.bits != 0;
  const int id = render ? K_RENDER : K_FWD;
  const double phase_bytes = render ? 0.0 : (h->s8 ? 1.0 : 2.0);   // charged per phase value; a RENDER form stores none
  const size_t blk_pieces = (size_t)(KS / 4) * 32;   // pieces of one [256 x WD] block of a hidden image
  const int n_super = k.n_super;
  const double npx = k.n_pb * 32.0;
  auto act = [&](int l) { return h->Abuf + (size_t)(render ? l & 1 : l) * h->a_stride; };
  {
    WL0Args a = zeroed<WL0Args>();
    a.gh = h->gh; a.gw = h->gw; a.W = h->cfg.width; a.row_begin = h->cfg.row_begin; a.pix0 = k.pix0; a.npix = h->npix;
    a.l0tab = h->l0tab; a.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi); a.KS = KS; a.n_pieces = k.n_pb * KS;
    if (!render) a.P = h->Pbuf;
    a.Act = act(0);
    Launch L(h, id, 4.0 * WD * npx, npx * (WD * (2.0 + phase_bytes)));
    const long n_wg = (a.n_pieces + 3) / 4;
    if (render) SF_TRY(with_op(h, [&](auto op) { return launch(h, k_wlayer0<decltype(op), false, true>, n_wg, 256, 0, a); }));
    else if (h->s8) SF_TRY(launch(h, k_wlayer0<OpF16, true>, (a.n_pieces / 2 + 3) / 4, 256, 0, a));
    else SF_TRY(with_op(h, [&](auto op) { return launch(h, k_wlayer0<decltype(op)>, n_wg, 256, 0, a); }));
  }
  for (int l = 1; l <= D - 2; ++l) {
    WGemmArgs a = zeroed<WGemmArgs>();
    a.A = reinterpret_cast<const u32x4*>(h->wf + (size_t)(l - 1) * WD * WD);
    a.a_block_pieces = (long)blk_pieces; a.n_chunk = KS / 4;
    a.Bin = act(l - 1); a.ks_in = KS;
    a.bias = h->biasw + (size_t)(l - 1) * WD;
    if (!render) {
      a.sc = (float)((double)h->cfg.hidden_omega_0 / kTwoPi / (double)h->wscale);
      a.Out = h->Pbuf + (size_t)l * h->p_stride;
    }
    a.OutAct = act(l); a.ks_out = KS; a.kp_out = WD / 32;
    Launch L(h, id, 2.0 * WD * WD * npx, npx * (WD * (2.0 + phase_bytes + 2.0 * NBLK)));
    SF_TRY(launch_wgemm<0>(h, a, n_super, NBLK, o.bits));
  }
  WGemmArgs a = zeroed<WGemmArgs>();
  a.A = reinterpret_cast<const u32x4*>(h->wf_last);
  a.a_block_pieces = (long)KS; a.n_chunk = KS / 4;
  a.Bin = act(D - 2); a.ks_in = KS;
  a.bias = h->biasw + (size_t)(D - 2) * WD; a.sc = 1.0f / h->wscale;
  a.pred = o.pred; a.nout = h->cfg.out_features; a.pix0 = k.pix0; a.npix = h->npix;
  if (!h->cfg.outermost_linear) a.last_om_rev = (float)((double)h->cfg.hidden_omega_0 / kTwoPi);
  if (render) {
    a.rgb8 = (uint8_t*)o.samples;   // (a.rgb16 of the 16-bit form: the same member)
  } else {
    a.img = h->img; a.gscale = gscale(h);
    a.sse_part = o.sse_part; a.Dlast = o.train ? h->Dlast : nullptr;
    if (o.sse8_part) a.sse8_part = o.sse8_part;   // the EVAL form of k_wgemm
    if (!h->cfg.outermost_linear) a.last_om = h->cfg.hidden_omega_0;
  }
  const double out_bytes = render ? h->cfg.out_features * render_sample_bytes(o.samples, o.bits, o.pred) : 12.0 + 64.0;
  Launch L(h, id, 2.0 * h->cfg.out_features * WD * npx, npx * (WD * 2.0 + out_bytes));
  return launch_wgemm<1>(h, a, n_super, 1, o.bits, o.sse8_part != nullptr);
}

// The forward of chunk c, training or evaluation form: the prediction to pred (or null), the chunk's SSE partials to sse_part;
// n_part: how many it wrote (one per 256-pixel group)
int wide_fwd_chunk(sf_engine* h, long c, bool train, float* pred, float* sse_part, int& n_part, unsigned long long* sse8_part = nullptr) {
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  n_part = k.n_super;
  return wide_fwd_walk(h, k, {pred, sse_part, train, nullptr, 0, sse8_part});
}

// The render loop of a wide render handle (sf_wide_render_create; its images are current): every chunk's RENDER walk, to pred
// and / or to samples of `bits` bits at out (either may be null)
int wide_render_chunks(sf_engine* h, void* out, int bits, float* pred) {
  for (long c = 0; c < n_chunks(h->npix, h->chunk_px); ++c)
    SF_TRY(wide_fwd_walk(h, chunk_at(c, h->npix, h->chunk_px), {pred, nullptr, false, out, bits}));
  return SF_OK;
}

// The backward of chunk c after its training forward: per layer, last first, k_wdw (weight gradient, every block in one launch)
// -> k_wreduce -> k_wgemm2<2> (data gradient); then layer 0 in 256-neuron blocks (k_dw0 -> k_reduce).  sse_part, n_part: the
// forward's partials of this chunk, from which k_wchunk_scale forms the chunk's fp8 factor
int wide_bwd_chunk(sf_engine* h, long c, const float* sse_part, int n_part) {
  const int WD = h->WD, D = h->D, KS = WD / 16, NBLK = WD / 256;
  const size_t blk_pieces = (size_t)(KS / 4) * 32;
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  const int n_super = k.n_super;
  const long n_pb = k.n_pb;
  const double npx = n_pb * 32.0;
  const int n_wg = (int)(n_pb < (long)h->dw_wg ? n_pb : (long)h->dw_wg);
  if (h->d8)   // fp8 deltas: this chunk's power-of-two factor from its own residual
    SF_TRY(launch(h, k_wchunk_scale, 1, 256, 0, sse_part, n_part,
                  1.0 / ((double)h->cfg.out_features * (double)k.px), gscale(h), h->gpre, kFp8Target, h->scale_dev));
  for (int l = D - 1; l >= 1; --l) {
    const bool last = l == D - 1;
    const bool dl8 = h->d8 && !last;                      // this layer's incoming deltas are fp8 byte pieces
    const u32x4* Dl = last ? h->Dlast : h->Dbuf + (size_t)l * h->d_stride;
    const u32x4* Pprev = h->Pbuf + (size_t)(l - 1) * h->p_stride;
    const double rows = last ? h->cfg.out_features : WD;
    {   // weight gradient: every [256 x 256] (last layer: [32 x 256]) block in one launch, blockIdx.y = block
      const int nby = (last ? 1 : NBLK) * NBLK;
      int gx = h->dw_wg / nby / 8 * 8;            // multiple of 8: same-pixel workgroups share an XCD
      if (gx < 8) gx = 8;
      if ((long)gx > n_pb) gx = (int)n_pb;
      WDwArgs a = zeroed<WDwArgs>();
      a.D = Dl; a.ksd_total = last ? 2 : (dl8 ? WD / 32 : KS); a.P = h->Abuf + (size_t)(l - 1) * h->a_stride; a.ksp_total = KS; a.nblk_i = NBLK;
      a.n_pb = n_pb; a.slab = h->slab;
      {
        Launch L(h, last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * rows * WD * npx, npx * ((last ? 64.0 : WD * 2.0) + WD * 2.0));
        const dim3 grid(gx, nby);
        if (dl8) SF_TRY(launch(h, k_wdw<256, OpF16, true>, grid, 512, WDwLds<256, true>::bytes, a));
        else SF_TRY(with_op(h, [&](auto op) {
          using OP = decltype(op);
          return last ? launch(h, k_wdw<32, OP>, grid, 512, WDwLds<32, false>::bytes, a) : launch(h, k_wdw<256, OP>, grid, 512, WDwLds<256, false>::bytes, a);
        }));
      }
      WReduceArgs r = zeroed<WReduceArgs>();
      r.slab = h->slab; r.n_wg = gx; r.slab_rows = last ? 32 : 256; r.rows_out = last ? h->cfg.out_features : 256;
      r.nblk_i = NBLK; r.gW = h->grads + h->off_w[l]; r.ldw = WD; r.gb = h->grads + h->off_b[l];
      r.accumulate = c > 0; r.scale = 1.0f / h->gpre;
      if (dl8) { r.s1 = h->scale_dev; r.s2 = h->lsc + 16 + l; }
      const int n = r.rows_out * 256 + r.rows_out;
      Launch L(h, K_REDUCE, 0, (double)gx * nby * n * 4.0);
      SF_TRY(launch(h, k_wreduce, dim3((n + 255) / 256, nby), 256, 0, r));
    }
    // data gradient: delta_{l-1} = (delta_l W_l) * omega cos(P_{l-1})
    WGemmArgs a = zeroed<WGemmArgs>();
    a.A = last ? reinterpret_cast<const u32x4*>(h->wb_last) : reinterpret_cast<const u32x4*>(h->wb + (size_t)(l - 1) * WD * WD);
    a.a_block_pieces = last ? 32 : (long)blk_pieces; a.n_chunk = last ? 1 : KS / 4;
    a.Bin = Dl; a.ks_in = last ? 2 : KS;
    a.Out = h->Dbuf + (size_t)(l - 1) * h->d_stride; a.ks_out = KS; a.kp_out = WD / 32; a.Pprev = Pprev;
    a.fscale = (h->d8 && last) ? h->scale_dev : nullptr;
    Launch L(h, last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * rows * WD * npx,
             npx * ((last ? 64.0 : WD * 2.0 * NBLK) + WD * (h->s8 ? 3.0 : 4.0)));
    SF_TRY(launch_wgemm<2>(h, a, n_super, NBLK));
  }
  for (int jb = 0; jb < NBLK; ++jb) {   // layer 0: contraction of delta_0 with the coordinates
    Dw0Args da = zeroed<Dw0Args>();
    fill_grid(h, k.pix0, da);
    da.D = h->Dbuf; da.ks_total = KS; da.ks_off = 16 * jb; da.n_pb = n_pb; da.slab = h->slab;
    {
      Launch L(h, K_DW_FIRST, 4.0 * 256 * npx, (h->d8 ? 256.0 : 512.0) * npx);
      SF_TRY(launch_dw_first_t<256>(h, da, n_wg));
    }
    ReduceArgs ra = zeroed<ReduceArgs>();
    ra.slab = h->slab; ra.n_wg = n_wg; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre; ra.scale_dev = nullptr;
    if (h->d8) { ra.scale_dev = h->scale_dev; ra.scale2_dev = h->lsc + 16; }     // 1 / (chunk factor * gpre), 1 / cumulative layer scale
    ra.gW = h->grads + h->off_w[0] + 512 * jb; ra.gb = h->grads + h->off_b[0] + 256 * jb;
    ra.slab_rows = 256; ra.slab_cols = 32; ra.rows_out = 256; ra.cols_out = 2; ra.mode = 1;
    Launch L(h, K_REDUCE, 0, (double)n_wg * (256 * 3) * 4.0);
    SF_TRY(launch_reduce(h, ra));
  }
  return SF_OK;
}

}  // namespace
