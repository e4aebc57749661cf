// fourier_render.hip — the inference-only path of FourierNet: sf_fourier_render_create, and sf_render on a FourierNet handle
// (include/siren_fit.h).
//
// A decoder needs the picture, not a training step.  The kernel is the RENDER instantiation of k_ff_fwd<WD>
// (fourier_kernels.hip): the evaluation forward - the encoding in registers, the MFMA chain, the weight staging and the
// sigmoid are the source lines of k_ff_fwd<WD, false> - without the target fetch, the residual, dz, the Z / H stores, the
// workgroup sum with its barrier and the SSE partial, and with bytes from the last-layer epilogue.  So sf_render's pred is
// bit-identical to sf_forward's on a FourierNet training handle (tests/test_gpu_fourier_render.py), and a window or a
// band is bit-identical to that region of the full picture: pixel (r, c) sees rows[r], cols[c] whatever the grid.
//
// Bytes: u8 = min(max((int)(pred * 255.0f), 0), 255), fwd_render_out's formula; sf_render16 runs the BITS = 16 form:
// u16 = min(max((int)(pred * 65535.0f), 0), 65535).  How a wave packs, gathers and stores the samples of its 32 pixels: the
// sample tail, beside render_store in siren_kernels.hip.
//
// A render handle (create_fourier(.., render = true), fourier_host.hip) holds the parameters, the weight images, encoding.B
// and the two coordinate vectors: none of the [D-1][WD][chunk] activation / gradient planes, the slab, gradients, Adam
// moments, mask or SSE partials of sf_fourier_create.
//
// This file is included at the end of siren_fit.hip, after siren_render.hip (one translation unit); ff_args_base, launch_ff
// and create_fourier are fourier_host.hip's.

namespace {

// sf_render / sf_render16 on a FourierNet handle (render or training), after their argument checks: chunked as
// a FourierNet pass.  out: bits / 8 bytes per sample
int render_fourier(sf_engine* h, void* out, int bits, float* pred) {
  if (!h->ff.have_B) return fail(SF_ERR_STATE, "sf_set_encoding has not been called");
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(refresh_images(h));
  const int WD = h->WD, D = h->D, MS = h->ff.MS;
  for (long c = 0; c < n_chunks(h->npix, h->chunk_px); ++c) {
    const Chunk k = chunk_at(c, h->npix, h->chunk_px);
    const double npx = (double)k.n_super * kSuper;
    FfArgs fa = ff_args_base(h, k.pix0);
    fa.pred = pred; fa.rgb8 = (uint8_t*)out;   // (a.rgb16 of the 16-bit form: the same member)
    Launch L(h, K_FF_RENDER, 2.0 * ((double)MS * WD + (double)(D - 2) * WD * WD + 32.0 * WD) * npx,
             npx * 3.0 * render_sample_bytes(out, bits, pred));
    SF_TRY(launch_ff(h, fa, k.n_super, bits == 16 ? kFfRender16 : kFfRender));
  }
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_fourier_render_create(const sf_fourier_config* cfg, sf_handle** out) try { return create_fourier(cfg, out, true); } SF_CATCH

}  // extern "C"
