// siren_host.hip — SIREN handles of hidden width <= 256 on the host: the forward, backward, layer-0 and reduction launchers
// (kernels: siren_kernels.hip, siren_s8.hip, siren_s8h.hip), weight images, the forward and the backward of a chunk, the scratch formats, and create_handle
// behind sf_create, sf_render_create (siren_render.hip) and the WaveletSiren sub-handles.  Included by siren_fit.hip.

namespace {

// 8-bit scratch: dL/dout is stored as residual * 2^10 in fp16 (residuals of 6e-8 .. 64 stay normal numbers); the
// adaptive part of the gradient pre-scale is applied by k_bwd8<LAST> (siren_s8.hip)
static constexpr float kResScale = 1024.0f;

// per-layer fp8 delta scales (link[16] | inv[16] | norms in h->lsc), rebuilt with the weight images
int launch_fp8_scales(sf_engine* h) {
  Fp8ScaleArgs f = zeroed<Fp8ScaleArgs>();
  f.params = h->params; f.depth = h->D; f.WD = h->WD; f.out_features = h->cfg.out_features;
  for (int l = 0; l < h->D; ++l) f.off_w[l] = h->off_w[l];
  f.om_first = h->cfg.first_omega_0; f.om_hidden = h->cfg.hidden_omega_0; f.link = h->lsc; f.inv = h->lsc + 16;
  f.nrm = reinterpret_cast<double*>(h->lsc + 32);
  SF_TRY(launch(h, k_fp8_norms, h->D - 1, 1024, 0, f));
  return launch(h, k_fp8_links, 1, 64, 0, f);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
size_t fwd_lds_bytes(int WD) { return (size_t)FwdGeom(WD).PIECES * 1024 + (size_t)WD * 16 + 64; }
// k_fwd_pipe: weight image halves + layer-0 image + SSE partials
size_t fwd_pipe_lds_bytes() { return (size_t)FwdGeom(256).PIECES * 1024 + (size_t)(256 / 32) * 1024 + 64; }

// hidden = 256, depth >= 3 run the persistent pipeline kernel (k_fwd_pipe): one workgroup per CU walks the chunk
bool fwd_is_pipe(const sf_engine* h) { return h->WD == 256 && h->D >= 3 && !h->wide; }
// forward workgroups of a chunk with n_super 256-pixel groups (= the chunk's SSE partials)
int fwd_grid(const sf_engine* h, int n_super) { return fwd_is_pipe(h) && n_super > h->dw_wg ? h->dw_wg : n_super; }

// hidden = 256, depth >= 3: the hand-scheduled software pipeline over all layers (k_fwd_pipe)
int launch_fwd_pipe(sf_engine* h, const FwdArgs& a, int n_wg, bool train, bool eval8) {
  const size_t lds = fwd_pipe_lds_bytes();
  const bool f16 = h->cfg.compute_dtype == SF_F16;
  if (f16 && train && h->s8) return launch(h, k_fwd_pipe<OpF16, true, true>, n_wg, 512, lds, a);
  return with_op(h, [&](auto op) {
    using OP = decltype(op);
    if (eval8) return launch(h, k_fwd_pipe<OpEval<OP>, false, false>, n_wg, 512, lds, a);
    return train ? launch(h, k_fwd_pipe<OP, true, false>, n_wg, 512, lds, a) : launch(h, k_fwd_pipe<OP, false, false>, n_wg, 512, lds, a);
  });
}
// the forward of a chunk on n_wg workgroups (fwd_grid): phase bytes (fp16 operands only), training or evaluation form;
// eval8 (never with train): the EVAL form, a.sse8_part set
int launch_fwd(sf_engine* h, const FwdArgs& a, int n_wg, bool train, bool eval8 = false) {
  if (fwd_is_pipe(h)) return launch_fwd_pipe(h, a, n_wg, train, eval8);
  return with_width(h, [&](auto wd) {
    constexpr int WD = decltype(wd)::value;
    const size_t lds = fwd_lds_bytes(WD);
    if (h->cfg.compute_dtype == SF_F16 && train && h->s8) return launch(h, k_fwd<WD, OpF16, true, true>, n_wg, 512, lds, a);
    return with_op(h, [&](auto op) {
      using OP = decltype(op);
      if (eval8) return launch(h, k_fwd<WD, OpEval<OP>, false>, n_wg, 512, lds, a);
      return train ? launch(h, k_fwd<WD, OP, true>, n_wg, 512, lds, a) : launch(h, k_fwd<WD, OP, false>, n_wg, 512, lds, a);
    });
  });
}

// what every forward of a SIREN handle (width <= 256) is given for the chunk that starts at local pixel pix0: coordinates,
// geometry, weight images and scales; the caller adds its outputs (scratch, target, prediction, partials)
FwdArgs fwd_args_base(const sf_engine* h, const PixelView& v, long pix0, int n_super) {
  FwdArgs fa = zeroed<FwdArgs>();
  fill_pixels(h, v, pix0, fa);
  fa.gh = v.gh; fa.gw = v.gw; fa.depth = h->D;
  fa.l0tab = h->l0tab; fa.l0img = reinterpret_cast<const u32x4*>(h->l0img);
  fa.wf = reinterpret_cast<const u32x4*>(h->wf);
  fa.wf_last = reinterpret_cast<const u32x4*>(h->wf_last);
  fa.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
  fa.sc_hidden = (float)((double)h->cfg.hidden_omega_0 / kTwoPi / (double)h->wscale);
  fa.sc_last = 1.0f / h->wscale;
  if (!h->cfg.outermost_linear) { fa.last_om = h->cfg.hidden_omega_0; fa.last_om_rev = (float)((double)h->cfg.hidden_omega_0 / kTwoPi); }
  fa.nout = h->cfg.out_features;
  fa.n_super = n_super;
  return fa;
}

// ---- backward --------------------------------------------------------------------------------------------------------
// fused backward of one layer, 16-bit scratch (k_bwd; its cases and their geometry: BwdCase, siren_kernels.hip): last = the
// out_features(<=3, padded to 32)-row layer; p0 = its input layer is layer 0, whose phases are re-derived from the coordinates.
int launch_bwd(sf_engine* h, bool last, bool p0, const BwdLayerArgs& a, int n_wg) {
  return with_width(h, [&](auto wd) {
    return with_bool(last, p0, [&](auto l, auto p) {
      return with_op(h, [&](auto op) {
        constexpr int WD = decltype(wd)::value;
        constexpr bool LAST = decltype(l)::value, P0 = decltype(p)::value;
        using C = BwdCase<WD, LAST, P0>;
        return launch(h, k_bwd<WD, LAST, P0, decltype(op)>, n_wg, C::threads, C::Lds::bytes, a);
      });
    });
  });
}

// 8-bit scratch path (k_bwd8; its cases: Bwd8Case, siren_s8.hip): fp16 operands only.  h->d8: fp8 deltas (scratch_format 8);
// else phase bytes with 16-bit float deltas (scratch_format 12).
int launch_bwd8(sf_engine* h, bool last, bool p0, const Bwd8Args& a, int n_wg) {
  return with_width(h, [&](auto wd) {
    return with_bool(last, p0, [&](auto l, auto p) {
      return with_bool(h->d8, [&](auto d) {
        constexpr int WD = decltype(wd)::value;
        constexpr bool LAST = decltype(l)::value, P0 = decltype(p)::value, D8 = decltype(d)::value;
        // fp8 deltas at width 256, every layer below the last: the slot-per-MFMA pipeline (siren_s8h.hip).  The forward of such
        // a layer is k_fwd_pipe, which spills layer 0's phase bytes too, so siren_bwd_chunk never asks for the P0 form here.
        if constexpr (WD == 256 && !LAST && D8) {
          return P0 ? fail(SF_ERR_INVALID, "launch_bwd8: no P0 form below the last layer")
                    : launch(h, k_bwd8h<kBwd8hPark>, n_wg, 512, Bwd8hLds<kBwd8hPark>::bytes, a);
        } else {
          using C = Bwd8Case<WD, LAST, P0, D8>;
          return launch(h, k_bwd8<WD, LAST, P0, D8>, n_wg, C::threads, C::Lds::bytes, a);
        }
      });
    });
  });
}

// weight gradient of layer 0 (no data gradient needed): contraction of delta_0 with the coordinates
template <int JW>
int launch_dw0(sf_engine* h, const Dw0Args& a, int n_wg) {
  return with_op(h, [&](auto op) { return launch(h, k_dw0<JW, decltype(op)>, n_wg, JW * 2, Dw0Lds<JW>::bytes, a); });
}
// ... from fp8 deltas (k_dw0_8; ring depth: Dw0Lds8, siren_s8.hip)
template <int JW>
int launch_dw0_8(sf_engine* h, const Dw0Args& a, int n_wg) {
  return launch(h, k_dw0_8<JW>, n_wg, JW * 2, Dw0Lds8<JW>::bytes, a);
}
template <int JW>
int launch_dw_first_t(sf_engine* h, const Dw0Args& a, int n_wg) {
  return h->d8 ? launch_dw0_8<JW>(h, a, n_wg) : launch_dw0<JW>(h, a, n_wg);
}
int launch_dw_first(sf_engine* h, const Dw0Args& a, int n_wg) {
  return with_width(h, [&](auto wd) { return launch_dw_first_t<decltype(wd)::value>(h, a, n_wg); });
}
// the fixed-order slab reduction of one layer's weight and bias gradient into the flat gradient
int launch_reduce(sf_engine* h, const ReduceArgs& ra) {
  return launch(h, k_reduce, (ra.rows_out * ra.cols_out + ra.rows_out + 15) / 16, 256, 0, ra);
}

// algorithmic GEMM FLOPs per pixel: forward 2*P_w, backward 4*P_w - 4*WD
double flops_fwd_px(const sf_engine* h) {
  const double W = h->WD;
  return 2.0 * (2 * W + (h->D - 2) * W * W + h->cfg.out_features * W);
}

// the 16-bit weight images, the layer-0 table / image (and, format 8, the per-layer delta scales) of a width <= 256
ImgArgs images_args(const sf_engine* h) {
  ImgArgs a = zeroed<ImgArgs>();
  a.params = h->params;
  a.depth = h->D;
  a.WD = h->WD;
  a.out_features = h->cfg.out_features;
  for (int l = 0; l < h->D; ++l) {
    a.off_w[l] = h->off_w[l];
    a.off_b[l] = h->off_b[l];
  }
  a.wscale = h->wscale;
  a.hscale = (float)((double)h->cfg.hidden_omega_0 / kTwoPi);
  a.om_first = h->cfg.first_omega_0; a.om_hidden = h->cfg.hidden_omega_0;
  a.fwd_is_f16 = h->cfg.compute_dtype == SF_F16;
  a.wf = h->wf; a.wf_last = h->wf_last; a.wb = h->wb; a.wb_last = h->wb_last;
  a.l0tab = h->l0tab;
  a.l0img = h->l0img; a.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
  return a;
}
// threads of k_images: one per element of the hidden images, at least the small tables
long images_count(const sf_engine* h) {
  long n = (long)(h->D - 2) * h->WD * h->WD;
  const long n_min = (long)h->WD / 16 * 64 * 8;  // also covers the small tables
  if (n < n_min) n = n_min;
  if (n < 1024) n = 1024;
  return n;
}
int refresh_images_siren(sf_engine* h) {
  ImgArgs a = images_args(h);
  const long n = images_count(h);
  Launch L(h, K_IMAGES, 0, (double)n * 8);
  if (h->d8 && h->lsc) {   // per-layer delta scales first: k_images folds them into the backward images
    SF_TRY(launch_fp8_scales(h));
    a.link = h->lsc;
  }
  SF_TRY(launch(h, k_images, (n + 255) / 256, 256, 0, a));
  h->images_dirty = false;
  return SF_OK;
}

// ---- the arguments of a chunk's kernels, each built in one place: siren_fwd_chunk / siren_bwd_chunk launch them one fit at a
// time, sf_step_many (many_host.hip) files them in tables of B fits -------------------------------------------------------
// the forward of chunk k (fwd_args_base plus its outputs); sse8_part non-null: the EVAL form
FwdArgs fwd_chunk_args(const sf_engine* h, const Chunk& k, bool train, float* pred, float* sse_part, unsigned long long* sse8_part) {
  FwdArgs fa = fwd_args_base(h, own_view(h), k.pix0, k.n_super);
  fa.P = h->Pbuf; fa.p_stride = h->p_stride; fa.Dlast = h->Dlast;
  fa.dfac = train ? h->wv.dfac_out : nullptr;
  fa.img = h->img;
  fa.gscale = h->d8 ? kResScale : gscale(h);
  fa.pred = pred;
  fa.sse_part = sse_part;
  if (sse8_part) fa.sse8_part = sse8_part;
  return fa;
}
double fwd_chunk_bytes(const sf_engine* h, const Chunk& k, bool train) {
  return k.n_pb * 32.0 * (4.0 * h->cfg.out_features + (train ? (h->D - 2) * h->WD * (h->s8 ? 1.0 : 2.0) + (h->s8 ? 32.0 : 64.0) : 0.0));
}
// workgroups of the layer kernels of a chunk (at most one per CU) and the pixel blocks each walks
struct BwdGrid { int n_wg; long pb_per_wg; };
BwdGrid bwd_grid(const sf_engine* h, const Chunk& k) {
  const int PBS = 2;   // k_dw stages two pixel blocks at a time; k_bwd accepts any block count
  int n_wg = (int)((k.n_pb + PBS - 1) / PBS);
  if (n_wg > h->dw_wg) n_wg = h->dw_wg;
  long pb_per_wg = (k.n_pb + n_wg - 1) / n_wg;
  pb_per_wg = (pb_per_wg + PBS - 1) / PBS * PBS;
  n_wg = (int)((k.n_pb + pb_per_wg - 1) / pb_per_wg);
  return {n_wg, pb_per_wg};
}
// what Bwd8Args and BwdLayerArgs share for layer l >= 1: deltas in and out, phases of the layer below, the backward image
template <typename Args>
void fill_bwd_layer(const sf_engine* h, const Chunk& k, int l, Args& ba) {
  const bool last = l == h->D - 1;
  const size_t img_pieces = (size_t)h->WD * h->WD / 8;
  fill_grid(h, k.pix0, ba);
  ba.D = last ? h->Dlast : h->Dbuf + (size_t)l * h->d_stride;
  ba.P = h->Pbuf + (size_t)(l - 1) * h->p_stride;
  ba.Dout = h->Dbuf + (size_t)(l - 1) * h->d_stride;
  ba.wb = last ? reinterpret_cast<const u32x4*>(h->wb_last)
               : reinterpret_cast<const u32x4*>(h->wb) + (size_t)(l - 1) * img_pieces;
  ba.n_pb = k.n_pb; ba.slab = h->slab; ba.l0tab = h->l0tab;
  ba.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
}
// k_bwd of layer l >= 1 (16-bit scratch)
BwdLayerArgs bwd_layer_args(const sf_engine* h, const Chunk& k, int l, const BwdGrid& g) {
  BwdLayerArgs ba = zeroed<BwdLayerArgs>();
  fill_bwd_layer(h, k, l, ba);
  ba.pb_per_wg = (int)g.pb_per_wg;
  return ba;
}
double bwd_layer_bytes(const sf_engine* h, const Chunk& k, int l) {
  return k.n_pb * 32.0 * ((l == h->D - 1 ? 64.0 : h->WD * 2.0) + h->WD * (l - 1 == 0 ? 2.0 : 4.0));
}
// k_dw0 / k_dw0_8 and their workgroups
Dw0Args dw0_args(const sf_engine* h, const Chunk& k) {
  Dw0Args da = zeroed<Dw0Args>();
  fill_grid(h, k.pix0, da);
  da.D = h->Dbuf; da.ks_total = h->WD / 16; da.ks_off = 0; da.n_pb = k.n_pb; da.slab = h->slab;
  return da;
}
int dw0_grid(const sf_engine* h, const Chunk& k) {
  const long cap0 = (h->d8 && h->WD == 256) ? 2L * h->dw_wg : (long)h->dw_wg;      // k_dw0_8<256>: two workgroups per CU
  return (int)(k.n_pb < cap0 ? k.n_pb : cap0);
}
// the slab reduction of layer l after a kernel of n_wg workgroups, chunk c (accumulating from the second chunk on)
ReduceArgs reduce_args(const sf_engine* h, long c, int l, int n_wg) {
  const int WD = h->WD;
  const bool last = l == h->D - 1;
  ReduceArgs ra = zeroed<ReduceArgs>();
  ra.slab = h->slab; ra.n_wg = n_wg; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre;
  if (h->d8) {   // last layer: dW from the statically scaled residual; layers below: the chunk's adaptive pre-scale
    ra.scale = (float)(1.0 / ((double)kResScale * (double)h->cfg.out_features * h->n_total));
    ra.scale_dev = last ? nullptr : h->scale_dev;
    ra.scale2_dev = (last || !h->lsc) ? nullptr : h->lsc + 16 + l;
  }
  ra.gW = h->grads + h->off_w[l]; ra.gb = h->grads + h->off_b[l];
  // a layer above 0: rows x WD weight gradient from slabs of (last: 32, else WD) rows
  ra.slab_rows = last ? 32 : WD; ra.slab_cols = WD; ra.rows_out = last ? h->cfg.out_features : WD; ra.cols_out = WD; ra.mode = 0;
  if (l == 0) { ra.slab_rows = WD; ra.slab_cols = 32; ra.rows_out = WD; ra.cols_out = 2; ra.mode = 1; }
  return ra;
}
// values a reduction of layer l writes; a hidden layer's slab layout is the flat gradient's [W | b]: k_reduce_vec
int reduce_count(const ReduceArgs& ra) { return ra.rows_out * ra.cols_out + ra.rows_out; }
bool reduce_is_vec(const sf_engine* h, int l) { return l > 0 && l != h->D - 1; }

// The forward of chunk c of a SIREN handle of width <= 256, training or evaluation form (k_fwd / k_fwd_pipe): the prediction
// to pred (or null), the chunk's SSE partials to sse_part; n_part: how many it wrote (fwd_grid).  sse8_part (sf_eval, with
// neither train nor pred): the EVAL form, which stores nothing but the two kinds of partials
int siren_fwd_chunk(sf_engine* h, long c, bool train, float* pred, float* sse_part, int& n_part, unsigned long long* sse8_part = nullptr) {
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  const FwdArgs fa = fwd_chunk_args(h, k, train, pred, sse_part, sse8_part);
  n_part = fwd_grid(h, k.n_super);
  Launch L(h, K_FWD, flops_fwd_px(h) * (k.n_pb * 32.0), fwd_chunk_bytes(h, k, train));
  return launch_fwd(h, fa, n_part, train, sse8_part != nullptr);
}

// The backward of chunk c after its training forward: k_bwd(last) -> k_bwd(hidden l = depth-2 .. 1) -> k_dw0, each followed by
// the fixed-order slab reduction into the flat fp32 gradient (accumulating from the second chunk on).  sse_part, n_part: the
// forward's partials of this chunk, from which the fp8 form of k_bwd8 takes the chunk's scale
int siren_bwd_chunk(sf_engine* h, long c, const float* sse_part, int n_part) {
  const int WD = h->WD, D = h->D;
  const Chunk k = chunk_at(c, h->npix, h->chunk_px);
  const long n_pb = k.n_pb;
  const double npx = n_pb * 32.0;
  // backward, last layer first; every layer kernel is followed by the fixed-order slab reduction
  const int PBS = 2;
  const BwdGrid g = bwd_grid(h, k);
  const int n_wg = g.n_wg;
  for (int l = D - 1; l >= 0; --l) {
    const bool last = l == D - 1;
    const double rows = last ? h->cfg.out_features : WD;
    ReduceArgs ra = reduce_args(h, c, l, n_wg);
    if (l > 0 && h->s8) {
      // layer 1: with fp8 deltas at width 256 the pipeline forward also spills layer 0's phase bytes, so this layer runs the
      // hidden-layer kernel (k_bwd8h) like the others; else the form that re-derives the layer-0 phases from the coordinates
      const bool l0_bytes = h->d8 && WD == 256 && fwd_is_pipe(h), p0 = l - 1 == 0 && !(l0_bytes && !last);
      Bwd8Args ba = zeroed<Bwd8Args>();
      fill_bwd_layer(h, k, l, ba);
      ba.sse_part = sse_part; ba.n_part = n_part;
      ba.inv_chunk_values = 1.0 / ((double)h->cfg.out_features * (double)k.px);
      ba.n_values = (double)h->cfg.out_features * h->n_total;
      ba.res_scale = kResScale; ba.target = kFp8Target; ba.scale_out = h->scale_dev;
      ba.zeros = reinterpret_cast<const u32x4*>(h->pad8); ba.dump = reinterpret_cast<u32x4*>(h->pad8 + 8192);
      // hidden 256: the last-layer kernel keeps two workgroups per CU (its slab rows are 32 wide: the slab has room)
      if (last && !p0 && WD == 256 && h->d8) ra.n_wg = (int)std::min<long>((n_pb + PBS - 1) / PBS, 2L * h->dw_wg);
      const double db = h->d8 ? 1.0 : 2.0;   // bytes per delta
      Launch L(h, last ? K_BWD_LAST : (p0 ? K_BWD_L1 : K_BWD_HIDDEN), 4.0 * rows * WD * npx,
               npx * ((last ? 32.0 : WD * db) + WD * db + (p0 ? 0.0 : WD * 1.0)));
      SF_TRY(launch_bwd8(h, last, p0, ba, ra.n_wg));
    } else if (l > 0) {
      const bool p0 = l - 1 == 0;
      const BwdLayerArgs ba = bwd_layer_args(h, k, l, g);
      Launch L(h, last ? K_BWD_LAST : (p0 ? K_BWD_L1 : K_BWD_HIDDEN), 4.0 * rows * WD * npx, bwd_layer_bytes(h, k, l));
      SF_TRY(launch_bwd(h, last, p0, ba, n_wg));
    } else {
      const Dw0Args da = dw0_args(h, k);
      ra.n_wg = dw0_grid(h, k);
      Launch L(h, K_DW_FIRST, 4.0 * WD * npx, WD * (h->d8 ? 1.0 : 2.0) * npx);
      SF_TRY(launch_dw_first(h, da, ra.n_wg));
    }
    const int n = reduce_count(ra);
    Launch L(h, K_REDUCE, 0, (double)n_wg * n * 4.0);
    if (reduce_is_vec(h, l))   // slab layout == flat gradient layout [W | b]
      SF_TRY(launch(h, k_reduce_vec, (n / 4 + 7) / 8, 256, 0, h->slab, n_wg, n, n / 4, h->grads + h->off_w[l], ra.accumulate,
                    ra.scale, ra.scale_dev, ra.scale2_dev));
    else SF_TRY(launch_reduce(h, ra));
  }
  return SF_OK;
}

// what the forward reads, on a training and on a render handle alike: the forward weight images (width <= 256; the wide
// path has its own blocked images), the layer-0 table / image and the two coordinate vectors
int alloc_forward_inputs(sf_engine* h) {
  const int WD = h->WD, D = h->D;
  if (!h->wide) {
    SF_TRY(dev_alloc(h, h->wf, (size_t)(D - 2 > 0 ? D - 2 : 1) * FwdGeom(WD).PIECES * 1024));
    SF_TRY(dev_alloc(h, h->wf_last, (size_t)(WD / 16 + 1) * 1024));
  }
  SF_TRY(dev_alloc(h, h->l0tab, (size_t)WD * 16));
  if (WD == 256) SF_TRY(dev_alloc(h, h->l0img, (size_t)(WD / 32) * 1024));
  SF_TRY(dev_alloc(h, h->gh, (size_t)h->cfg.height * 4));
  return dev_alloc(h, h->gw, (size_t)h->cfg.width * 4);
}

// layer strides of the phase / delta scratch for the handle's current format
void set_scratch_strides(sf_engine* h) {
  const long chunk = h->chunk_px;
  const int WD = h->WD;
  h->p_stride = chunk / 32 * (h->s8 ? WD / 32 : WD / 16) * 64 + 37 * 64;
  h->d_stride = chunk / 32 * (h->d8 ? WD / 32 : WD / 16) * 64 + 37 * 64;
  h->a_stride = chunk / 32 * (WD / 16) * 64 + 37 * 64;
}
// sf_create and sf_render_create (siren_render.hip): one validation, one geometry; a render handle allocates the forward's
// inputs only.  sub_network: the handle is one of the two SIRENs of a WaveletSiren handle, which points params / grads / m /
// v / mask at slices of its own joint vectors - nothing is allocated for them here.  wide_render: the caller is
// sf_wide_render_create (siren_render.hip), the one creator that takes hidden 512 / 1024 for a render handle: the blocked forward
// images of the wide path and TWO activation planes, which the layers use in turn
int create_handle(const sf_config* cfg, sf_handle** out, bool render, bool sub_network = false, bool wide_render = false) {
  auto check = [&](Grid& g) -> int {
    if (cfg->out_features < 1 || cfg->out_features > 3) return fail(SF_ERR_INVALID, "out_features must be 1..3");
    if (cfg->depth < 2 || cfg->depth > 16) return fail(SF_ERR_INVALID, "depth must be 2..16");
    if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256 && cfg->hidden != 512 &&
        cfg->hidden != 1024)
      return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128, 256, 512 or 1024 in this build");
    if (cfg->hidden > 256 && cfg->depth < 3) return fail(SF_ERR_INVALID, "hidden > 256 needs depth >= 3");
    if (render && cfg->hidden > 256 && !wide_render)
      return fail(SF_ERR_INVALID, "sf_render_create: the render kernel is not built for the wide path (hidden 512 / 1024): "
                                  "run the model's own forward on the host side");
    if (cfg->compute_dtype != SF_BF16 && cfg->compute_dtype != SF_F16)
      return fail(SF_ERR_INVALID, "compute_dtype must be SF_BF16 or SF_F16");
    if (cfg->height < 1 || cfg->width < 1) return fail(SF_ERR_INVALID, "bad image size");
    if (cfg->scratch_format != 0 && cfg->scratch_format != 8 && cfg->scratch_format != 12 && cfg->scratch_format != 16)
      return fail(SF_ERR_INVALID, "scratch_format must be 0 (auto), 8, 12 or 16");
    if ((cfg->scratch_format == 8 || cfg->scratch_format == 12) && cfg->compute_dtype != SF_F16)
      return fail(SF_ERR_INVALID, "scratch_format 8 / 12 need compute_dtype SF_F16");
    int r0 = cfg->row_begin, r1 = cfg->row_end;
    if (r0 == 0 && r1 == 0) r1 = cfg->height;
    if (r0 < 0 || r1 > cfg->height || r0 >= r1) return fail(SF_ERR_INVALID, "bad row range");
    // the layer-0 / layer-1 gradient kernels decode (row, col) of a local pixel p as row = (p * ceil(2^40 / W)) >> 40,
    // exact while p * W < 2^40, i.e. local_rows * W^2 < 2^40 (an unsharded 8192 x 8192 grid sits at 2^39)
    if ((double)(r1 - r0) * (double)cfg->width * (double)cfg->width >= 1099511627776.0)
      return fail(SF_ERR_INVALID, "grid too large for one handle: (row_end - row_begin) * width^2 must stay below 2^40 "
                                  "(shard the rows over more handles)");
    g = {cfg->height, cfg->width, r0, r1};
    return SF_OK;
  };
  auto init = [&](sf_engine* h, const Grid& g) -> int {
    h->cfg = *cfg;
    h->cfg.row_begin = g.row_begin;
    h->cfg.row_end = g.row_end;
    adam_defaults(h);
    h->D = cfg->depth;
    h->WD = cfg->hidden;
    h->wide = cfg->hidden > 256;
    {
      // auto (fp16 operands, hidden <= 256): phase bytes always; fp8 deltas (format 8) when the image has >= 2^20 pixels - a
      // gradient then sums the zero-mean fp8 rounding over >= 10^6 terms (within the 0.05 dB criterion on every reference
      // fixture even at 2^16 pixels) and the backward kernels are bandwidth-bound; smaller fits are
      // launch-latency-bound and keep 16-bit deltas (format 12).  A masked fit is moved to format 16 by sf_set_masks.
      int fmt = cfg->scratch_format;
      h->fmt_auto = fmt == 0;
      const bool mega = (double)cfg->height * (double)cfg->width >= 1048576.0;
      // (wider than 256: the layer-at-a-time kernels take the byte formats where bandwidth matters - from 2^20 pixels; fp8 deltas up to
      // width 512, where a reference-minted fixture at 2^20 pixels pins them (tests/golden/plateau_ns_512x4_1024.npz: -0.0002 dB);
      // phase bytes only above)
      if (fmt == 0) fmt = cfg->compute_dtype != SF_F16 ? 16 : h->wide ? (mega ? (cfg->hidden <= 512 ? 8 : 12) : 16) : (mega ? 8 : 12);
      if (render) { fmt = 16; h->fmt_auto = false; }   // no scratch at all: nothing of the byte formats applies
      h->cfg.scratch_format = fmt;
      h->s8 = fmt == 8 || fmt == 12;
      h->d8 = fmt == 8;
    }
    layer_offsets(h, 2);   // named_parameters() order (siren.py:90-118)
    // fp16 forward images are scaled by 2^8 so that small weights stay normal numbers
    h->wscale = cfg->compute_dtype == SF_F16 ? 256.0f : 1.0f;
    // fp16 backward operands: dL/dout = resid/(3N) is pre-scaled by 2^k ~ 4*3N so the deltas sit around 1
    // (fp16 normal range 6e-5..65504); every gradient is multiplied back by 2^-k in the slab reduction
    if (cfg->compute_dtype == SF_F16) h->gpre = (float)exp2(ceil(log2((double)cfg->out_features * (double)cfg->height * (double)cfg->width)) + 2.0);
    // chunking
    // default: 4 Mi pixels at width <= 256 (29 GB of scratch at 256x8); the same scratch budget for wider layers
    // (a wide render handle: 2^18 pixels at 512, 2^17 at 1024 - 256 MiB per activation plane)
    const long chunk_auto = render && h->wide ? (1L << 18) / (cfg->hidden / 512) : (1L << 22) / (h->wide ? cfg->hidden / 256 : 1);
    const long chunk = chunk_pixels(cfg->chunk_pixels > 0 ? cfg->chunk_pixels : chunk_auto, h->npix);
    h->chunk_px = chunk;
    const int WD = h->WD, D = h->D;
    // layer stride of the scratch tensors, padded so that the three streams a kernel touches at once are
    // not a power of two apart (HBM channel aliasing)
    // (8-bit scratch: one piece per 32-neuron tile instead of one per 16-neuron k-step)
    set_scratch_strides(h);

    if (!sub_network) SF_TRY(alloc_state(h, !render));
    SF_TRY(alloc_forward_inputs(h));
    const size_t img_elems = (size_t)(D - 2 > 0 ? D - 2 : 1) * WD * WD;
    auto alloc_wide_forward = [&]() -> int {   // blocked forward images of siren_wide.hip and the pre-scaled biases
      SF_TRY(dev_alloc(h, h->wf, img_elems * 2));
      SF_TRY(dev_alloc(h, h->wf_last, (size_t)(WD / 16) * 1024));
      return dev_alloc(h, h->biasw, ((size_t)(D - 2) * WD + 32) * 4);
    };
    // a render handle: parameters, forward weight images, layer-0 table / image, the two coordinate vectors; wide: and two
    // activation planes - layer l reads plane (l - 1) & 1 and writes plane l & 1 (wide_render_chunks, wide_host.hip)
    if (render) {
      if (h->wide) { SF_TRY(alloc_wide_forward()); SF_TRY(dev_alloc(h, h->Abuf, (size_t)2 * h->a_stride * 16)); }
      return SF_OK;
    }
    SF_TRY(dev_alloc(h, h->wb, img_elems * 2));
    if (h->wide) {   // ... and the backward ones
      SF_TRY(alloc_wide_forward());
      SF_TRY(dev_alloc(h, h->wb_last, (size_t)(WD / 256) * 32 * 1024));
    } else {
      SF_TRY(dev_alloc(h, h->wb_last, (size_t)WD / 32 * 64 * 16));
    }
    SF_TRY(dev_alloc(h, h->Pbuf, (size_t)(D - 1) * h->p_stride * 16));
    SF_TRY(dev_alloc(h, h->Dbuf, (size_t)(D - 1) * h->d_stride * 16));
    if (h->wide) SF_TRY(dev_alloc(h, h->Abuf, (size_t)(D - 1) * h->a_stride * 16));
    SF_TRY(dev_alloc(h, h->Dlast, (size_t)chunk / 32 * 2 * 64 * 16));
    { const size_t sw = WD > 256 ? 256 : WD; SF_TRY(dev_alloc(h, h->slab, (size_t)h->dw_wg * (sw * sw + sw) * 4 + 4096)); }
    SF_TRY(alloc_sse(h, chunked_sse_parts(h)));
    SF_TRY(dev_alloc(h, h->scale_dev, 16));
    SF_TRY(dev_alloc(h, h->pad8, 16384));
    SF_TRY(dev_alloc(h, h->lsc, 32 * 4 + 16 * 8));
    if (hipMemset(h->pad8, 0, 16384) != hipSuccess) return fail(SF_ERR_NOMEM, "hipMemset failed");
    const float sc[2] = {(float)((double)h->gpre / ((double)cfg->out_features * h->n_total)), 1.0f / h->gpre};
    if (hipMemcpy(h->scale_dev, sc, sizeof(sc), hipMemcpyHostToDevice) != hipSuccess) return fail(SF_ERR_HIP, "hipMemcpy(scale) failed");
    return SF_OK;
  };
  return create_with(cfg, out, &sf_config::in_features, Model::Siren, render, check, init);
}

// An auto-format handle that receives a mask leaves the 8-bit scratch: fp8 deltas under one scale per chunk underflow in
// a 90 %-sparse network, and topology updates rank small gradients that phase bytes blur.
// (the new buffers are allocated BEFORE anything of the handle changes: a failed hipMalloc leaves the handle exactly as it
//  was - format, strides and scratch - and returns SF_ERR_NOMEM)
int switch_scratch_format(sf_engine* h, int fmt) {
  hipStreamSynchronize(h->ctx->stream);
  const sf_config cfg0 = h->cfg;
  const bool s8_0 = h->s8, d8_0 = h->d8;
  h->cfg.scratch_format = fmt;
  h->s8 = fmt == 8 || fmt == 12;
  h->d8 = fmt == 8;
  set_scratch_strides(h);
  u32x4 *newP = nullptr, *newD = nullptr;
  if (dev_alloc(h, newP, (size_t)(h->D - 1) * h->p_stride * 16) || dev_alloc(h, newD, (size_t)(h->D - 1) * h->d_stride * 16)) {
    dev_free(h, newP);
    (void)hipGetLastError();
    h->cfg = cfg0; h->s8 = s8_0; h->d8 = d8_0;
    set_scratch_strides(h);
    return fail(SF_ERR_NOMEM, "hipMalloc failed while moving the scratch to format 16 (the handle keeps its format)");
  }
  if (h->graph.exec) { hipGraphExecDestroy(h->graph.exec); h->graph.exec = nullptr; }
  dev_free(h, h->Pbuf);
  dev_free(h, h->Dbuf);
  h->Pbuf = newP; h->Dbuf = newD;
  h->images_dirty = true;      // (the backward images carry the fp8 per-layer scales only under format 8)
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_create(const sf_config* cfg, sf_handle** out) try { return create_handle(cfg, out, false); } SF_CATCH

}  // extern "C"
