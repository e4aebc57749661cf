// siren_render.hip — the inference-only path of the engine: sf_render_create / sf_render (include/siren_fit.h).
// (sf_render on a FourierNet handle: render_fourier, fourier_render.hip.)
//
// A decoder needs the picture, not a training step.  The kernels are the RENDER instantiations of k_fwd<WD> and k_fwd_pipe
// (siren_kernels.hip): the evaluation forward (no phase stores, so the pipeline's counted waits are those of TRAIN = false)
// without the target fetch, the residual, the SSE partial and its workgroup reduction, and with fwd_render_out below as the
// last-layer epilogue.  Up to the fp32 prediction nothing differs from the training forward - the same weight images, the
// same MFMA chain, the same v_sin_f32 - so sf_render's pred is bit-identical to sf_forward's (tests/test_gpu_render.py).
//
// Bytes: u8 = min(max((int)(pred * 255.0f), 0), 255), the product in fp32 and truncated toward zero - the reference's
// (pred * 255).int() (implicit_image/utils/train_helper.py:52, eval_epoch), clamped to what a file can hold.  16-bit samples
// (sf_render16, BITS = 16): u16 = min(max((int)(pred * 65535.0f), 0), 65535), the same statement one sample width up - it
// inverts the loader's raw / (2^16 - 1).  How a wave packs, gathers and stores the samples of its 32 pixels: the sample
// tail, beside render_store in siren_kernels.hip.
//
// This file is included at the end of siren_fit.hip (one translation unit, as every kernel file of the library); the host
// part builds on siren_host.hip (create_handle, fwd_args_base, the forward geometry).

namespace sf {

// The 32-pixel stores of fwd_render_out below (k_fwd, k_fwd_pipe, k_wgemm): what render_store<BITS, 32> (siren_kernels.hip,
// where the tail is explained) does, as it was written before that template.  This one call site keeps them: with the
// template here a Feathermap decode leg measured above the parent's spread twice, so the device
// code of these kernels is byte for byte the parent's.
// The byte form.  mine: the lane's pixel of the block starting at pixel px0, channel c in byte c (lanes 0..31; the upper half
// is never selected).  Called by all 64 lanes; rgb8 + px0 * nout is dword aligned (the entry point checks the base,
// 32 | px0).
DEV void render_store_block(uint8_t* rgb8, long px0, long npix, int nout, uint32_t mine, int lane) {
  const long left = npix - px0;
  const int nbytes = left >= 32 ? 32 * nout : (left > 0 ? (int)left * nout : 0);   // bytes of the block inside the picture
  uint32_t word = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * lane + j;                            // byte k of the block = pixel k / nout, channel k % nout
    const int src = nout == 3 ? k / 3 : (nout == 2 ? k >> 1 : k);
    const int ch = k - src * nout;
    const uint32_t v = (uint32_t)__shfl((int)mine, src & 31);   // (lanes >= 8 * nout gather nothing they store)
    word |= ((v >> (8 * ch)) & 0xffu) << (8 * j);
  }
  if (lane < 8 * nout) {
    uint8_t* blk = rgb8 + px0 * nout;
    if (4 * lane + 4 <= nbytes) {
      reinterpret_cast<uint32_t*>(blk)[lane] = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * lane + j < nbytes) blk[4 * lane + j] = (uint8_t)(word >> (8 * j));
    }
  }
}

// Sample k (= pixel k / nout, channel k % nout) of a wave's block of 16-bit samples, gathered from the lane that holds the
// pixel: v0 = channel 0 | channel 1 << 16, v1 = channel 2.  lanes: the pixels of the block (32); called by all 64 lanes, two
// ds_bpermute.
DEV uint32_t render_sample16(uint32_t v0, uint32_t v1, int k, int nout, int lanes) {
  const int src = nout == 3 ? k / 3 : (nout == 2 ? k >> 1 : k);
  const int ch = k - src * nout;
  const uint32_t lo = (uint32_t)__shfl((int)v0, src & (lanes - 1)), hi = (uint32_t)__shfl((int)v1, src & (lanes - 1));
  return ch == 2 ? hi : (lo >> (16 * ch)) & 0xffffu;
}
// Stores dword d of a wave's block of 16-bit samples (samples 2d, 2d + 1 = word) when the output holds both, the low half
// as one 2-byte store when it holds only the first (the ragged end of an output with an odd sample count), else nothing.
// blk: the block's first sample, dword aligned; nsamp: samples of the block inside the output.
DEV void render_store_dword16(uint16_t* blk, int d, int nsamp, uint32_t word) {
  if (2 * d + 2 <= nsamp) reinterpret_cast<uint32_t*>(blk)[d] = word;
  else if (2 * d < nsamp) blk[2 * d] = (uint16_t)word;
}

// render_store_block for 16-bit samples.  mine0 / mine1: the lane's pixel of the block starting at pixel px0 (lanes 0..31;
// the upper half is never selected).  Called by all 64 lanes; rgb16 + px0 * nout is dword aligned (the entry point checks
// the base, 32 | px0): lane d < 16 * nout stores dword d.
DEV void render_store_block16(uint16_t* rgb16, long px0, long npix, int nout, uint32_t mine0, uint32_t mine1, int lane) {
  const long left = npix - px0;
  const int nsamp = left >= 32 ? 32 * nout : (left > 0 ? (int)left * nout : 0);   // samples of the block inside the picture
  const uint32_t s0 = render_sample16(mine0, mine1, 2 * lane, nout, 32);        // (lanes >= 16 * nout gather nothing they store)
  const uint32_t s1 = render_sample16(mine0, mine1, 2 * lane + 1, nout, 32);
  if (lane < 16 * nout) render_store_dword16(rgb16 + px0 * nout, lane, nsamp, s0 | (s1 << 16));
}

template <int BITS>
DEV void fwd_render_out(const FwdArgs& a, const f32x16& acc, long pix, long pb, bool valid, int lane, int h) {
  const int nout = a.nout;
  RenderPx<BITS> mine;   // this lane's pixel (lanes of the upper half hold padded rows: never selected)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (c >= nout) break;
    // exactly fwd_residual's prediction
    float o = acc[c] * a.sc_last;
    if (a.last_om_rev != 0.f) {
      const float tt = o * a.last_om_rev;
      o = __builtin_amdgcn_sinf(tt);
    }
    const float p = o * 0.5f + 0.5f;  // siren.py:131
    if (a.pred && h == 0 && valid) a.pred[pix * nout + c] = p;
    mine.put(c, p);
  }
  if (!a.rgb8) return;   // (a.rgb16: the same member)
  const long px0 = a.pix0 + pb * 32;   // the block's first pixel: a multiple of 32
  if constexpr (BITS == 16) render_store_block16(a.rgb16, px0, a.npix, nout, mine.v0, mine.v1, lane);
  else render_store_block(a.rgb8, px0, a.npix, nout, mine.v0, lane);
}

}  // namespace sf

namespace {

// the kernel family sf_forward picks for the handle (fwd_is_pipe), in its RENDER form, on n_wg workgroups (fwd_grid);
// bits: 8 (a.rgb8) or 16 (a.rgb16) per sample
int launch_render(sf_engine* h, const FwdArgs& a, int n_wg, int bits) {
  return with_bool(bits == 16, [&](auto wide) {
    constexpr int BITS = decltype(wide)::value ? 16 : 8;
    return with_op(h, [&](auto op) {
      using OP = decltype(op);
      if (fwd_is_pipe(h))
        return launch(h, k_fwd_pipe<OP, false, false, true, BITS>, n_wg, 512, fwd_pipe_lds_bytes(), a);
      return with_width(h, [&](auto wd) {
        constexpr int WD = decltype(wd)::value;
        return launch(h, k_fwd<WD, OP, false, false, true, BITS>, n_wg, 512, fwd_lds_bytes(WD), a);
      });
    });
  });
}

// The render loop of a SIREN handle of width <= 256 (its images are current): the RENDER forward of every chunk, to pred and /
// or to samples of `bits` bits at out (either may be null).  window: the pixels drawn when they are not the handle's own grid
// (sf_wavelet_render: a coefficient window on a sub-handle)
int render_chunks(sf_engine* h, void* out, int bits, float* pred, const PixelView* window = nullptr) {
  const PixelView v = window ? *window : own_view(h);
  for (long c = 0; c < n_chunks(v.npix, h->chunk_px); ++c) {
    const Chunk k = chunk_at(c, v.npix, h->chunk_px);
    const int n_super = k.n_super;
    FwdArgs fa = fwd_args_base(h, v, k.pix0, n_super);
    fa.pred = pred;
    fa.rgb8 = (uint8_t*)out;   // (a.rgb16 of the 16-bit forms: the same member)
    Launch L(h, K_RENDER, flops_fwd_px(h) * n_super * (double)kSuper,
             n_super * (double)kSuper * h->cfg.out_features * render_sample_bytes(out, bits, pred));
    SF_TRY(launch_render(h, fa, fwd_grid(h, n_super), bits));
  }
  return SF_OK;
}

// fourier_render.hip, included last: the RENDER form of k_ff_fwd (out: bits / 8 bytes per sample)
int render_fourier(sf_engine* h, void* out, int bits, float* pred);

// sf_render / sf_render16 (wide = false) and sf_wide_render / sf_wide_render16 (wide = true) at bits = 8 / 16: one set of
// argument checks.  The entry points differ in the handles they refuse - the wide ones draw the one kind of handle that
// sf_wide_render_create makes and send any other to the entry point that draws it - and in the draw
int render_any(sf_handle* h, void* out, int bits, float* pred, bool wide) {
  const std::string fn = std::string(wide ? "sf_wide_render" : "sf_render") + (bits == 16 ? "16" : "");
  const std::string on = bits == 16 ? "rgb16_dev" : "rgb8_dev";
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  if (!out && !pred) return fail(SF_ERR_INVALID, fn + ": " + on + " and pred_dev are both NULL");
  if (wide) {
    if (!(h->model == Model::Siren && h->wide && h->render)) {
      const char* use = h->model == Model::Wavelet ? "sf_wavelet_render draws a WaveletSiren handle"
                        : h->model == Model::Fourier ? "sf_render draws a FourierNet handle"
                        : h->wide ? "a training handle of hidden 512 / 1024 (sf_create) evaluates through sf_forward"
                                  : "sf_render draws a SIREN handle of hidden width 32 .. 256";
      return fail(SF_ERR_INVALID, fn + ": built for the wide render handle of sf_wide_render_create (hidden 512 / 1024); " + use);
    }
  } else {
    if (h->model == Model::Wavelet && h->render)
      return fail(SF_ERR_INVALID, fn + ": a WaveletSiren render handle (sf_wavelet_render_create) is drawn by sf_wavelet_render" +
                                      (bits == 16 ? "16" : ""));
    if (h->wide || h->model == Model::Wavelet)
      return fail(SF_ERR_INVALID, fn + ": built for SIREN handles of hidden width 32 .. 256 (sf_create / sf_render_create) "
                                       "and FourierNet handles (sf_fourier_create / sf_fourier_render_create)");
  }
  if (((uintptr_t)out & 3u) != 0) return fail(SF_ERR_INVALID, fn + ": " + on + " must be 4-byte aligned");
  if (h->render && h->fth.attached && !h->fth.loaded)   // (never a wide handle: sf_feather_render_attach refuses it)
    return fail(SF_ERR_STATE, fn + ": sf_feather_render_load has not been called (the handle has a feather state and no weights yet)");
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  if (h->model == Model::Fourier) return render_fourier(h, out, bits, pred);   // (wide = false: refused above otherwise)
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(refresh_images(h));
  return wide ? wide_render_chunks(h, out, bits, pred) : render_chunks(h, out, bits, pred);
}

}  // namespace

extern "C" {

int sf_render_create(const sf_config* cfg, sf_handle** out) try { return create_handle(cfg, out, true); } SF_CATCH

int sf_render(sf_handle* h, uint8_t* rgb8, float* pred) try { return render_any(h, rgb8, 8, pred, false); } SF_CATCH
int sf_render16(sf_handle* h, uint16_t* rgb16, float* pred) try { return render_any(h, rgb16, 16, pred, false); } SF_CATCH

int sf_wide_render_create(const sf_config* cfg, sf_handle** out) try {
  if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if ((cfg->hidden != 512 && cfg->hidden != 1024) || cfg->depth < 3)
    return fail(SF_ERR_INVALID, "sf_wide_render_create: built for hidden 512 / 1024 with depth >= 3 (the layer-at-a-time kernels); "
                                "sf_render_create makes the render handle of hidden 32 .. 256");
  return create_handle(cfg, out, true, false, true);
} SF_CATCH
int sf_wide_render(sf_handle* h, uint8_t* rgb8, float* pred) try { return render_any(h, rgb8, 8, pred, true); } SF_CATCH
int sf_wide_render16(sf_handle* h, uint16_t* rgb16, float* pred) try { return render_any(h, rgb16, 16, pred, true); } SF_CATCH

}  // extern "C"
