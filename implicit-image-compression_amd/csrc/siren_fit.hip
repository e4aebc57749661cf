// siren_fit.hip — the one translation unit of the library: the kernel files, the host core (engine.h), one host file per
// model and one for the topology updates (mask_host.hip), the model-independent entry points of the C ABI (include/siren_fit.h), the three render paths - in this order,
// which is the order of the non-template kernels in the code object.
//
// One sf_engine == one per-image fit on one HIP stream.  A training step is, per pixel chunk:
//   k_fwd -> k_bwd(last) -> k_bwd(hidden l = depth-2 .. 1) -> k_dw0, each followed by the fixed-order slab
//   reduction into the flat fp32 gradient; then k_adam (+mask) and k_images (16-bit weight images).
// Every `interval` steps of a masked fit the topology changes: sf_mask_update (kernels siren_mask.hip, host mask_host.hip),
// two more launches, or sf_mask_prune_global (same files), six.
// The sequence mirrors one `train_epoch` of the reference (implicit_image/utils/train_helper.py:132-185)
// for the full-batch grid (implicit_image/compress.py:137-138).
#include "siren_kernels.hip"
#include "siren_s8.hip"
#include "siren_s8h.hip"
#include "siren_wide.hip"
#include "siren_kmeans.hip"
#include "fourier_kernels.hip"
#include "feather_kernels.hip"
#include "wavelet_kernels.hip"
#include "siren_mask.hip"
#include "siren_quant.hip"
#include "siren_many.hip"

#include "engine.h"

// Every template kernel of the library, in the order the code object holds them.  The compiler emits instantiations in the
// order of their first use, so this list - their first use - keeps the device code byte for byte what it was measured as,
// however the host code below is arranged: a host-only change leaves the sha256 of the device object alone.  A kernel the
// launch code asks for and this list lacks is still built (behind these); one listed and never launched would be built too.
// A row names a kernel by its case; the geometry of a case is stated once, beside the kernel (BwdCase, Bwd8Case, Dw0Lds8).
#define SF_K(...) reinterpret_cast<const void*>(&__VA_ARGS__)
[[maybe_unused]] static const void* const kKernelOrder[] = {
    SF_K(k_fwd_pipe<OpF16, true, true, false>), SF_K(k_fwd_pipe<OpF16, true, false, false>),
    SF_K(k_fwd_pipe<OpF16, false, false, false>), SF_K(k_fwd_pipe<OpBF16, true, false, false>),
    SF_K(k_fwd_pipe<OpBF16, false, false, false>), SF_K(k_bwd<32, true, true, OpF16>),
    SF_K(k_bwd<32, true, true, OpBF16>), SF_K(k_bwd<32, true, false, OpF16>), SF_K(k_bwd<32, true, false, OpBF16>),
    SF_K(k_bwd<32, false, true, OpF16>), SF_K(k_bwd<32, false, true, OpBF16>), SF_K(k_bwd<32, false, false, OpF16>),
    SF_K(k_bwd<32, false, false, OpBF16>), SF_K(k_bwd<64, true, true, OpF16>), SF_K(k_bwd<64, true, true, OpBF16>),
    SF_K(k_bwd<64, true, false, OpF16>), SF_K(k_bwd<64, true, false, OpBF16>), SF_K(k_bwd<64, false, true, OpF16>),
    SF_K(k_bwd<64, false, true, OpBF16>), SF_K(k_bwd<64, false, false, OpF16>), SF_K(k_bwd<64, false, false, OpBF16>),
    SF_K(k_bwd<128, true, true, OpF16>), SF_K(k_bwd<128, true, true, OpBF16>), SF_K(k_bwd<128, true, false, OpF16>),
    SF_K(k_bwd<128, true, false, OpBF16>), SF_K(k_bwd<128, false, true, OpF16>),
    SF_K(k_bwd<128, false, true, OpBF16>), SF_K(k_bwd<128, false, false, OpF16>),
    SF_K(k_bwd<128, false, false, OpBF16>), SF_K(k_bwd<256, true, true, OpF16>), SF_K(k_bwd<256, true, true, OpBF16>),
    SF_K(k_bwd<256, true, false, OpF16>), SF_K(k_bwd<256, true, false, OpBF16>), SF_K(k_bwd<256, false, true, OpF16>),
    SF_K(k_bwd<256, false, true, OpBF16>), SF_K(k_bwd<256, false, false, OpF16>),
    SF_K(k_bwd<256, false, false, OpBF16>), SF_K(k_bwd8<32, true, true, false>), SF_K(k_bwd8<32, true, false, false>),
    SF_K(k_bwd8<32, false, true, false>), SF_K(k_bwd8<32, false, false, false>), SF_K(k_bwd8<64, true, true, false>),
    SF_K(k_bwd8<64, true, false, false>), SF_K(k_bwd8<64, false, true, false>), SF_K(k_bwd8<64, false, false, false>),
    SF_K(k_bwd8<128, true, true, false>), SF_K(k_bwd8<128, true, false, false>),
    SF_K(k_bwd8<128, false, true, false>), SF_K(k_bwd8<128, false, false, false>),
    SF_K(k_bwd8<256, true, true, false>), SF_K(k_bwd8<256, true, false, false>),
    SF_K(k_bwd8<256, false, true, false>), SF_K(k_bwd8<256, false, false, false>), SF_K(k_bwd8h<kBwd8hPark>),
    SF_K(k_bwd8<32, true, true, true>), SF_K(k_bwd8<32, true, false, true>), SF_K(k_bwd8<32, false, true, true>),
    SF_K(k_bwd8<32, false, false, true>), SF_K(k_bwd8<64, true, true, true>), SF_K(k_bwd8<64, true, false, true>),
    SF_K(k_bwd8<64, false, true, true>), SF_K(k_bwd8<64, false, false, true>), SF_K(k_bwd8<128, true, true, true>),
    SF_K(k_bwd8<128, true, false, true>), SF_K(k_bwd8<128, false, true, true>), SF_K(k_bwd8<128, false, false, true>),
    SF_K(k_bwd8<256, true, true, true>), SF_K(k_bwd8<256, true, false, true>), SF_K(k_dw0_8<32>), SF_K(k_dw0_8<64>),
    SF_K(k_dw0_8<128>), SF_K(k_dw0_8<256>), SF_K(k_dw0<32, OpF16>), SF_K(k_dw0<32, OpBF16>), SF_K(k_dw0<64, OpF16>),
    SF_K(k_dw0<64, OpBF16>), SF_K(k_dw0<128, OpF16>), SF_K(k_dw0<128, OpBF16>),
    SF_K(k_fwd<32, OpF16, true, true, false>), SF_K(k_fwd<32, OpF16, true, false, false>),
    SF_K(k_fwd<32, OpF16, false, false, false>), SF_K(k_fwd<32, OpBF16, true, false, false>),
    SF_K(k_fwd<32, OpBF16, false, false, false>), SF_K(k_fwd<64, OpF16, true, true, false>),
    SF_K(k_fwd<64, OpF16, true, false, false>), SF_K(k_fwd<64, OpF16, false, false, false>),
    SF_K(k_fwd<64, OpBF16, true, false, false>), SF_K(k_fwd<64, OpBF16, false, false, false>),
    SF_K(k_fwd<128, OpF16, true, true, false>), SF_K(k_fwd<128, OpF16, true, false, false>),
    SF_K(k_fwd<128, OpF16, false, false, false>), SF_K(k_fwd<128, OpBF16, true, false, false>),
    SF_K(k_fwd<128, OpBF16, false, false, false>), SF_K(k_fwd<256, OpF16, true, true, false>),
    SF_K(k_fwd<256, OpF16, true, false, false>), SF_K(k_fwd<256, OpF16, false, false, false>),
    SF_K(k_fwd<256, OpBF16, true, false, false>), SF_K(k_fwd<256, OpBF16, false, false, false>),
    SF_K(k_wlayer0<OpF16, true>), SF_K(k_wlayer0<OpF16, false>), SF_K(k_wlayer0<OpBF16, false>),
    SF_K(k_wgemm2<0, OpF16, true, false, false>), SF_K(k_wgemm2<0, OpF16, false, false, false>),
    SF_K(k_wgemm2<0, OpBF16, false, false, false>), SF_K(k_wgemm<OpF16>), SF_K(k_wgemm<OpBF16>),
    SF_K(k_wdw<32, OpF16, false>), SF_K(k_wdw<32, OpBF16, false>), SF_K(k_wdw<256, OpF16, true>),
    SF_K(k_wdw<256, OpF16, false>), SF_K(k_wdw<256, OpBF16, false>), SF_K(k_wgemm2<2, OpF16, true, false, true>),
    SF_K(k_wgemm2<2, OpF16, true, true, true>), SF_K(k_wgemm2<2, OpF16, true, false, false>),
    SF_K(k_wgemm2<2, OpF16, false, false, false>), SF_K(k_wgemm2<2, OpBF16, false, false, false>),
    SF_K(k_dw0<256, OpF16>), SF_K(k_dw0<256, OpBF16>), SF_K(k_ff_fwd<32, false, false>),
    SF_K(k_ff_fwd<32, true, false>), SF_K(k_ff_bwd<32>), SF_K(k_ff_fwd<64, false, false>),
    SF_K(k_ff_fwd<64, true, false>), SF_K(k_ff_bwd<64>), SF_K(k_ff_fwd<128, false, false>),
    SF_K(k_ff_fwd<128, true, false>), SF_K(k_ff_bwd<128>), SF_K(k_ff_fwd<256, false, false>),
    SF_K(k_ff_fwd<256, true, false>), SF_K(k_ff_bwd<256>), SF_K(k_ff_dw<1, true>), SF_K(k_ff_dw<2, true>),
    SF_K(k_ff_dw<4, true>), SF_K(k_ff_dw<1, false>), SF_K(k_ff_dw<2, false>), SF_K(k_ff_dw<4, false>),
    SF_K(k_fwd_pipe<OpF16, false, false, true>), SF_K(k_fwd_pipe<OpBF16, false, false, true>),
    SF_K(k_fwd<32, OpF16, false, false, true>), SF_K(k_fwd<32, OpBF16, false, false, true>),
    SF_K(k_fwd<64, OpF16, false, false, true>), SF_K(k_fwd<64, OpBF16, false, false, true>),
    SF_K(k_fwd<128, OpF16, false, false, true>), SF_K(k_fwd<128, OpBF16, false, false, true>),
    SF_K(k_fwd<256, OpF16, false, false, true>), SF_K(k_fwd<256, OpBF16, false, false, true>),
    SF_K(k_ff_fwd<32, false, true>), SF_K(k_ff_fwd<64, false, true>), SF_K(k_ff_fwd<128, false, true>),
    SF_K(k_ff_fwd<256, false, true>), SF_K(k_fth_mat<false>), SF_K(k_fth_mat<true>),
    SF_K(k_wlayer0<OpF16, false, true>), SF_K(k_wlayer0<OpBF16, false, true>),
    SF_K(k_wgemm2<0, OpF16, false, false, false, true>), SF_K(k_wgemm2<0, OpBF16, false, false, false, true>),
    SF_K(k_wgemm<OpF16, true, 8>), SF_K(k_wgemm<OpF16, true, 16>), SF_K(k_wgemm<OpBF16, true, 8>),
    SF_K(k_wgemm<OpBF16, true, 16>), SF_K(k_prune_file<false>), SF_K(k_prune_file<true>),
    // sf_step_many (siren_many.hip): behind everything that was there before it
    SF_K(k_fwd_many<32>), SF_K(k_fwd_many<64>), SF_K(k_fwd_many<128>), SF_K(k_bwd_many<32, true, true>),
    SF_K(k_bwd_many<32, true, false>), SF_K(k_bwd_many<32, false, true>), SF_K(k_bwd_many<32, false, false>),
    SF_K(k_bwd_many<64, true, true>), SF_K(k_bwd_many<64, true, false>), SF_K(k_bwd_many<64, false, true>),
    SF_K(k_bwd_many<64, false, false>), SF_K(k_bwd_many<128, true, true>), SF_K(k_bwd_many<128, true, false>),
    SF_K(k_bwd_many<128, false, true>), SF_K(k_bwd_many<128, false, false>), SF_K(k_dw0_many<32>), SF_K(k_dw0_many<64>),
    SF_K(k_dw0_many<128>),
};
#undef SF_K

#include "siren_host.hip"
#include "wide_host.hip"
#include "fourier_host.hip"
#include "wavelet_host.hip"
#include "feather_host.hip"
#include "mask_host.hip"

namespace {

// the weight images of any handle follow its parameters
int refresh_images(sf_engine* h) {
  if (!h->images_dirty) return SF_OK;
  switch (h->model) {
    case Model::Siren: return h->wide ? refresh_images_wide(h) : refresh_images_siren(h);
    case Model::Fourier: return refresh_images_fourier(h);
    case Model::Wavelet: return refresh_images_wavelet(h);
  }
  __builtin_unreachable();
}

// The chunk loop of every training / evaluation pass of a SIREN or FourierNet handle (its images are current): per chunk the
// model's forward and, if train, its backward, the chunks' SSE partials one after the other in h->sse_part; then their
// fixed-order reduction.  (A WaveletSiren handle runs its two SIREN sub-handles instead: run_pass_wavelet.)
int run_chunks(sf_engine* h, bool train, float* pred, bool want_sse, bool eval8) {
  long sse_off = 0;
  for (long c = 0; c < n_chunks(h->npix, h->chunk_px); ++c) {
    float* const part = h->sse_part + sse_off;
    unsigned long long* const part8 = eval8 ? h->sse8_part + sse_off : nullptr;   // non-null: the EVAL form
    int n_part = 0;
    switch (h->model) {
      case Model::Siren:
        SF_TRY(h->wide ? wide_fwd_chunk(h, c, train, pred, part, n_part, part8) : siren_fwd_chunk(h, c, train, pred, part, n_part, part8));
        if (train) SF_TRY(h->wide ? wide_bwd_chunk(h, c, part, n_part) : siren_bwd_chunk(h, c, part, n_part));
        break;
      case Model::Fourier:
        SF_TRY(fourier_fwd_chunk(h, c, train, pred, part, n_part, part8));
        if (train) SF_TRY(fourier_bwd_chunk(h, c, part));
        break;
      case Model::Wavelet: __builtin_unreachable();   // run_pass
    }
    sse_off += n_part;
  }
  if (eval8) return launch_eval_reduce(h, sse_off);
  if (want_sse || train) SF_TRY(launch_sse_reduce(h, sse_off));
  return SF_OK;
}

int run_pass(sf_engine* h, bool train, float* pred, bool want_sse, bool eval8) {
  if (h->render) return fail(SF_ERR_INVALID, "a render handle (sf_render_create) runs sf_render only");
  if (train) h->fth.fresh = false;
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  if ((train || want_sse) && !h->img) return fail(SF_ERR_STATE, "sf_set_target has not been called");
  switch (h->model) {   // the model's own checks, before anything is launched
    case Model::Wavelet: return run_pass_wavelet(h, train, pred, want_sse, eval8);
    case Model::Fourier:
      if (!h->ff.have_B) return fail(SF_ERR_STATE, "sf_set_encoding has not been called");
      break;
    case Model::Siren:
      if (train && (!h->Pbuf || !h->Dbuf)) return fail(SF_ERR_STATE, "the handle has no backward scratch");   // (never a null store on the GPU)
  }
  SF_TRY(refresh_images(h));
  return run_chunks(h, train, pred, want_sse, eval8);
}

int read_sse(sf_engine* h, double* out) {
  HIPCHK(hipMemcpyAsync(out, h->sse_dev, sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
  HIPCHK(hipStreamSynchronize(h->ctx->stream));
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_abi_version(void) { return SF_ABI_VERSION; }
const char* sf_last_error(void) { return g_err.c_str(); }

int sf_destroy(sf_handle* h) try {
  if (h) destroy(h);
  return SF_OK;
} SF_CATCH

int sf_num_params(const sf_handle* h, int64_t* n) try {
  if (!h || !n) return fail(SF_ERR_INVALID, "null argument");
  *n = h->P;
  return SF_OK;
} SF_CATCH
int sf_scratch_format(const sf_handle* h, int32_t* format) try {
  if (!h || !format) return fail(SF_ERR_INVALID, "null argument");
  *format = h->cfg.scratch_format;
  return SF_OK;
} SF_CATCH
int sf_param_offset(const sf_handle* h, int32_t layer, int64_t* w, int64_t* b) try {
  if (!h || layer < 0 || layer >= h->D) return fail(SF_ERR_INVALID, "bad layer");
  const sf_engine* s = h;
  int64_t base = 0;
  switch (h->model) {
    case Model::Siren:
    case Model::Fourier: break;
    case Model::Wavelet: {   // layers 0 .. depth-1: LF, then HF in the second half of the flat vector
      const bool hf = layer >= h->wv.sub[0]->D;
      s = h->wv.sub[hf];
      if (hf) { base = h->wv.sub[0]->P; layer -= h->wv.sub[0]->D; }
    }
  }
  if (w) *w = base + s->off_w[layer];
  if (b) *b = base + s->off_b[layer];
  return SF_OK;
} SF_CATCH

// one flat fp32 vector of the handle (P values) to or from the caller's device buffer, on the handle's stream
static int copy_state(sf_engine* h, float* dst, const float* src) {
  if (!h || !dst || !src) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(dst, src, h->P * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
  return SF_OK;
}
int sf_set_params(sf_handle* h, const float* p) try {
  SF_NO_FEATHER_RENDER(h, "sf_set_params");
  int rc = copy_state(h, h ? h->params : nullptr, p);
  if (!rc) h->images_dirty = true;
  return rc;
} SF_CATCH
int sf_get_params(sf_handle* h, float* p) try { return copy_state(h, p, h ? h->params : nullptr); } SF_CATCH
int sf_get_grads(sf_handle* h, float* p) try {
  SF_NO_RENDER(h, "sf_get_grads");
  return copy_state(h, p, h ? h->grads : nullptr);
} SF_CATCH
int sf_set_grads(sf_handle* h, const float* p) try {
  SF_NO_RENDER(h, "sf_set_grads");
  if (h) h->fth.fresh = false;
  return copy_state(h, h ? h->grads : nullptr, p);
} SF_CATCH
int sf_set_masks(sf_handle* h, const float* p) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_masks");
  DevGuard dev_guard(h->cfg.device);
  if (!p) { h->has_mask = false; return SF_OK; }
  if (h->fth.attached) return fail(SF_ERR_INVALID, "sf_set_masks: a Feathermap handle is dense (masking.dense: True)");
  if (h->fmt_auto && h->cfg.scratch_format != 16) {
    const int rs = switch_scratch_format(h, 16);
    if (rs) return rs;
  }
  int rc = copy_state(h, h->mask, p);
  if (!rc) h->has_mask = true;
  return rc;
} SF_CATCH
int sf_get_adam_state(sf_handle* h, float* m, float* v, int64_t* step) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_get_adam_state");
  DevGuard dev_guard(h->cfg.device);
  if (m) { int rc = copy_state(h, m, h->m); if (rc) return rc; }
  if (v) { int rc = copy_state(h, v, h->v); if (rc) return rc; }
  if (step) *step = h->step;
  return SF_OK;
} SF_CATCH
int sf_set_adam_state(sf_handle* h, const float* m, const float* v, int64_t step) try {
  if (!h || step < 0) return fail(SF_ERR_INVALID, "bad argument");
  SF_NO_RENDER(h, "sf_set_adam_state");
  DevGuard dev_guard(h->cfg.device);
  if (m) { int rc = copy_state(h, h->m, m); if (rc) return rc; }
  if (v) { int rc = copy_state(h, h->v, v); if (rc) return rc; }
  h->step = step;
  return SF_OK;
} SF_CATCH
int sf_state_ptr(sf_handle* h, int32_t which, float** p) try {
  if (!h || !p) return fail(SF_ERR_INVALID, "null argument");
  if (h->render && which >= 1 && which <= 4) return refuse_render("sf_state_ptr");
  switch (which) {
    case 0: *p = h->params; return SF_OK;
    case 1: *p = h->grads; return SF_OK;
    case 2: *p = h->m; return SF_OK;
    case 3: *p = h->v; return SF_OK;
    case 4: *p = h->mask; return SF_OK;
  }
  return fail(SF_ERR_INVALID, "bad state selector");
} SF_CATCH

int sf_sse_ptr(sf_handle* h, double** p) try {
  if (!h || !p) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_sse_ptr");
  *p = h->sse_dev;
  return SF_OK;
} SF_CATCH

int sf_sse8_ptr(sf_handle* h, uint64_t** p) try {
  if (!h || !p) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_sse8_ptr");
  *p = reinterpret_cast<uint64_t*>(sse8_dev(h));
  return SF_OK;
} SF_CATCH

int sf_debug_scratch(sf_handle* h, int32_t which, void** p, int64_t* bytes) try {
  if (!h || !p || !bytes) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_debug_scratch");
  switch (h->model) {
    case Model::Siren: break;
    case Model::Fourier: return fail(SF_ERR_INVALID, "sf_debug_scratch: a FourierNet handle has no phase / delta scratch");
    case Model::Wavelet: return fail(SF_ERR_INVALID, "sf_debug_scratch: the scratch of a WaveletSiren handle lives in its sub-networks");
  }
  const int D = h->D;
  switch (which) {
    case 0: *p = h->Pbuf; *bytes = (int64_t)(D - 1) * h->p_stride * 16; return SF_OK;
    case 1: *p = h->Dbuf; *bytes = (int64_t)(D - 1) * h->d_stride * 16; return SF_OK;
    case 2: *p = h->Dlast; *bytes = (int64_t)(h->chunk_px / 32) * (h->s8 ? 1 : 2) * 64 * 16; return SF_OK;
    case 3: { const size_t sw = h->WD > 256 ? 256 : h->WD; *p = h->slab; *bytes = (int64_t)h->dw_wg * (sw * sw + sw) * 4; return SF_OK; }
  }
  return fail(SF_ERR_INVALID, "bad scratch selector");
} SF_CATCH

int sf_params_changed(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_FEATHER_RENDER(h, "sf_params_changed");
  h->images_dirty = true;
  return SF_OK;
} SF_CATCH

// the two coordinate vectors of a handle (the caller holds the device)
static int set_coords(sf_engine* h, const float* rows, const float* cols) {
  switch (h->model) {
    case Model::Siren:
    case Model::Fourier: break;
    case Model::Wavelet:
      if (h->render) {   // kept whole and unchecked: sf_wavelet_render points the sub-networks at slices of them
        HIPCHK(hipMemcpyAsync(h->gh, rows, (size_t)h->wv.n * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
        HIPCHK(hipMemcpyAsync(h->gw, cols, (size_t)h->wv.n * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
      } else {           // both sub-networks run on the n x n coefficient grid (wavelet_siren.py:76-80)
        for (sf_engine* s : h->wv.sub) SF_TRY(set_coords(s, rows, cols));
      }
      h->have_coords = true;
      return SF_OK;
  }
  HIPCHK(hipMemcpyAsync(h->gh, rows, (size_t)h->cfg.height * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
  HIPCHK(hipMemcpyAsync(h->gw, cols, (size_t)h->cfg.width * 4, hipMemcpyDeviceToDevice, h->ctx->stream));
  // The forward indexes these vectors; the gradient kernels of layer 0 / layer 1 re-derive the coordinate of a
  // pixel as i/(n-1) instead of loading it.  Both agree only for get_grid()'s linspace(0,1,n) (data.py:82-83):
  // anything else is rejected here instead of training on inconsistent coordinates.  A render handle only indexes them
  // (a window of a grid is a slice of the two vectors), so it takes whatever it is given.
  if (!h->render) {
    std::vector<float> hv((size_t)h->cfg.height + h->cfg.width);
    HIPCHK(hipMemcpyAsync(hv.data(), h->gh, (size_t)h->cfg.height * 4, hipMemcpyDeviceToHost, h->ctx->stream));
    HIPCHK(hipMemcpyAsync(hv.data() + h->cfg.height, h->gw, (size_t)h->cfg.width * 4, hipMemcpyDeviceToHost, h->ctx->stream));
    HIPCHK(hipStreamSynchronize(h->ctx->stream));
    auto is_linspace = [](const float* v, int n) {
      for (int i = 0; i < n; ++i) {
        const float ref = n > 1 ? (float)((double)i / (double)(n - 1)) : 0.f;
        if (!(fabsf(v[i] - ref) <= 2e-6f)) return false;
      }
      return true;
    };
    if (!is_linspace(hv.data(), h->cfg.height) || !is_linspace(hv.data() + h->cfg.height, h->cfg.width))
      return fail(SF_ERR_INVALID, "sf_set_coords: rows / cols must be torch.linspace(0, 1, n) (data.py:82-83)");
  }
  h->have_coords = true;
  return SF_OK;
}
int sf_set_coords(sf_handle* h, const float* rows, const float* cols) try {
  if (!h || !rows || !cols) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  return set_coords(h, rows, cols);
} SF_CATCH
int sf_set_target(sf_handle* h, const float* img) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_target");
  h->img = img;
  return SF_OK;
} SF_CATCH

int sf_forward(sf_handle* h, float* pred, double* sse_out) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  const bool want = sse_out != nullptr;
  int rc = run_pass(h, false, pred, want);
  if (rc) return rc;
  if (want) return read_sse(h, sse_out);
  return SF_OK;
} SF_CATCH

// eval_epoch's sums in one pass that stores no prediction (include/siren_fit.h): every refusal first, with this entry point's
// name; then the handle's integer partials (first call), the EVAL forms of the forwards through run_pass, and one copy of the
// two words behind sse_dev
int sf_eval(sf_handle* h, double* sse_out, uint64_t* sse8_out) try {
  if (!h) return fail(SF_ERR_INVALID, "sf_eval: null argument");
  SF_NO_RENDER(h, "sf_eval");
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_eval: sf_set_coords has not been called");
  if (!h->img) return fail(SF_ERR_STATE, "sf_eval: sf_set_target has not been called");
  if (h->model == Model::Fourier && !h->ff.have_B) return fail(SF_ERR_STATE, "sf_eval: sf_set_encoding has not been called");
  DevGuard dev_guard(h->cfg.device);
  if (!h->sse8_part) SF_TRY(dev_alloc(h, h->sse8_part, (size_t)h->n_sse * 8));   // (before any launch: no EVAL kernel sees a null pointer)
  SF_TRY(run_pass(h, false, nullptr, true, true));
  if (!sse_out && !sse8_out) return SF_OK;
  struct { double sse; uint64_t sse8; } both;   // the two words behind sse_dev: one copy, one synchronise
  HIPCHK(hipMemcpyAsync(&both, h->sse_dev, sizeof(both), hipMemcpyDeviceToHost, h->ctx->stream));
  HIPCHK(hipStreamSynchronize(h->ctx->stream));
  if (sse_out) *sse_out = both.sse;
  if (sse8_out) *sse8_out = both.sse8;
  return SF_OK;
} SF_CATCH

int sf_forward_backward(sf_handle* h, double* sse_out) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_forward_backward");
  DevGuard dev_guard(h->cfg.device);
  int rc = run_pass(h, true, nullptr, true);
  if (rc) return rc;
  if (sse_out) return read_sse(h, sse_out);
  return SF_OK;
} SF_CATCH

// one optimiser step on the gradient the handle holds, then the weight images of the new parameters (refresh = false: they
// stay marked dirty - the caller rewrites the weights before the next pass, which refreshes them)
// k_adam on the handle's flat state, without the per-step scalars (adam_scalars, or a device table of them)
static AdamArgs adam_args(const sf_engine* h) {
  AdamArgs a = zeroed<AdamArgs>();
  a.p = h->params; a.g = h->grads; a.m = h->m; a.v = h->v; a.mask = h->has_mask ? h->mask : nullptr;
  a.n = h->P;
  a.beta1 = h->cfg.beta1; a.beta2 = h->cfg.beta2; a.eps = h->cfg.eps;
  // torch forms 1 - beta in double and hands the kernel the rounded float (0.1f, 0.001f); 1.0f - beta in fp32 is
  // 0.100000024 / 0.000999987
  a.omb1 = (float)(1.0 - h->beta1_d); a.omb2 = (float)(1.0 - h->beta2_d);
  return a;
}
// {step_size, bc2_sqrt} of the handle's Adam step number t (from 1) at learning rate lr, formed in double as torch does
static void adam_scalars(const sf_engine* h, double t, float lr, float* out2) {
  const double bc1 = 1.0 - pow(h->beta1_d, t), bc2 = 1.0 - pow(h->beta2_d, t);
  out2[0] = (float)((double)lr / bc1);
  out2[1] = (float)sqrt(bc2);
}
static int adam_step(sf_engine* h, float lr, bool refresh = true) {
  h->step += 1;
  AdamArgs a = adam_args(h);
  if (h->ctx->replay) { a.tab = h->graph.step_tab; a.iter = h->graph.iter_dev; }
  float sc[2];
  adam_scalars(h, (double)h->step, lr, sc);
  a.step_size = sc[0];
  a.bc2_sqrt = sc[1];
  if (h->fth.attached) {   // adjoint -> Adam on [V1 | V2 | scalers] -> materialise: four launches
    if (!h->fth.fresh) SF_TRY(feather_adjoint(h));
    a.p = h->fth.p; a.g = h->fth.g; a.m = h->fth.m; a.v = h->fth.v; a.mask = nullptr; a.n = h->fth.nf;
    {
      Launch L(h, K_FTH_ADAM, 0, (double)h->fth.nf * 28);
      SF_TRY(launch(h, k_adam, (h->fth.nf + 255) / 256, 256, 0, a));
    }
    SF_TRY(feather_materialise(h));
    return refresh_images(h);
  }
  {
    Launch L(h, K_ADAM, 0, (double)h->P * 28);
    SF_TRY(launch(h, k_adam, (h->P + 255) / 256, 256, 0, a));
  }
  h->images_dirty = true;
  return refresh ? refresh_images(h) : SF_OK;
}
int sf_adam_step(sf_handle* h, float lr) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_adam_step");
  DevGuard dev_guard(h->cfg.device);
  return adam_step(h, lr);
} SF_CATCH

// ---- graph replay -----------------------------------------------------------------------------------------
// One training step (forward, backward, reductions, Adam, weight images) is captured ONCE into a hipGraph on an
// engine-owned stream and replayed n times; the only per-step scalars (Adam's bias-corrected step size, computed
// on the host in double exactly as sf_adam_step does) are read from a device table indexed by a device counter.
static int graph_prepare(sf_engine* h, int n) {
  if (!h->graph.stream) {
    HIPCHK(hipStreamCreateWithFlags(&h->graph.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->graph.ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->graph.ev_out, hipEventDisableTiming));
    SF_TRY(dev_alloc(h, h->graph.iter_dev, 16));
    HIPCHK(hipMemset(h->graph.iter_dev, 0, 16));   // [0] replay step index, [2] constant 0 (eager table index)
  }
  if (n > h->graph.tab_cap) {
    dev_free(h, h->graph.step_tab);
    dev_free(h, h->graph.loss_tab);
    h->graph.step_tab = nullptr; h->graph.loss_tab = nullptr; h->graph.tab_cap = 0;
    SF_TRY(dev_alloc(h, h->graph.step_tab, (size_t)n * 8));
    SF_TRY(dev_alloc(h, h->graph.loss_tab, (size_t)n * 8));
    h->graph.tab_cap = n;
    if (h->graph.exec) { hipGraphExecDestroy(h->graph.exec); h->graph.exec = nullptr; }   // the graph holds the old table pointers
  }
  return SF_OK;
}

// n SSE values of the loss table as the MSE per step, read on the handle's current stream (which it waits for)
static int read_losses(sf_engine* h, int n, float* loss_out) {
  std::vector<double> sse((size_t)n);
  HIPCHK(hipMemcpyAsync(sse.data(), h->graph.loss_tab, (size_t)n * 8, hipMemcpyDeviceToHost, h->ctx->stream));
  HIPCHK(hipStreamSynchronize(h->ctx->stream));
  for (int i = 0; i < n; ++i) loss_out[i] = (float)(sse[i] / ((double)h->cfg.out_features * (double)h->npix));
  return SF_OK;
}

static int step_replay(sf_engine* h, const float* lr, int n, float* loss_out) {
  SF_TRY(graph_prepare(h, n));
  std::vector<float> tab((size_t)n * 2);
  for (int i = 0; i < n; ++i) adam_scalars(h, (double)(h->step + i + 1), lr[i], &tab[2 * i]);
  hipStream_t user = h->ctx->stream;
  HIPCHK(hipEventRecord(h->graph.ev_in, user));
  HIPCHK(hipStreamWaitEvent(h->graph.stream, h->graph.ev_in, 0));
  h->ctx->stream = h->graph.stream;
  struct Restore { sf_engine* h; hipStream_t s; ~Restore() { h->ctx->stream = s; h->ctx->replay = false; } } restore{h, user};
  HIPCHK(hipMemcpyAsync(h->graph.step_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->graph.stream));
  HIPCHK(hipStreamSynchronize(h->graph.stream));            // `tab` is pageable host memory: keep it alive until copied
  HIPCHK(hipMemsetAsync(h->graph.iter_dev, 0, 4, h->graph.stream));
  SF_TRY(refresh_images(h));                             // parameters edited since the last pass
  if (!h->graph.exec || h->graph.img != h->img || h->graph.mask != h->has_mask) {
    if (h->graph.exec) { hipGraphExecDestroy(h->graph.exec); h->graph.exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(h->graph.stream, hipStreamCaptureModeRelaxed));
    h->ctx->replay = true;
    const int64_t step0 = h->step;
    int rc = run_pass(h, true, nullptr, true);
    if (!rc) rc = adam_step(h, 0.f);
    if (!rc) rc = launch(h, k_tick, 1, 1, 0, h->graph.iter_dev);   // (h->ctx->stream is the capturing stream here)
    h->step = step0;
    h->ctx->replay = false;
    const hipError_t e = hipStreamEndCapture(h->graph.stream, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(SF_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t e2 = hipGraphInstantiate(&h->graph.exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e2 != hipSuccess) { h->graph.exec = nullptr; return fail(SF_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
    h->graph.img = h->img; h->graph.mask = h->has_mask;
  }
  for (int i = 0; i < n; ++i) HIPCHK(hipGraphLaunch(h->graph.exec, h->graph.stream));
  h->step += n;
  h->images_dirty = false;
  if (loss_out) SF_TRY(read_losses(h, n, loss_out));   // (on the replay stream)
  HIPCHK(hipEventRecord(h->graph.ev_out, h->graph.stream));
  HIPCHK(hipStreamWaitEvent(user, h->graph.ev_out, 0));
  return SF_OK;
}

// The eager run of n steps, for sf_step and sf_quant_step: per step `before` (if given), the pass, `after` (if given), Adam at
// lr[i] (refresh: adam_step's).  With `table` there is no host sync per step: every step's SSE goes to a device table, read back
// once at the end; without it a loss to report is read from the handle's scalar after each pass.
using StepHook = std::function<int()>;
static int eager_steps(sf_engine* h, const float* lr, int n, float* loss_out, bool table, bool refresh,
                       const StepHook& before = nullptr, const StepHook& after = nullptr) {
  if (table) SF_TRY(graph_prepare(h, n));
  for (int i = 0; i < n; ++i) {
    if (before) SF_TRY(before());
    h->graph.loss_dst = table ? h->graph.loss_tab + i : nullptr;
    const int rc = run_pass(h, true, nullptr, true);
    h->graph.loss_dst = nullptr;
    if (rc) return rc;
    if (loss_out && !table) {
      double sse = 0;
      SF_TRY(read_sse(h, &sse));
      loss_out[i] = (float)(sse / ((double)h->cfg.out_features * (double)h->npix));
    }
    if (after) SF_TRY(after());
    SF_TRY(adam_step(h, lr[i], refresh));
  }
  return table ? read_losses(h, n, loss_out) : SF_OK;
}

int sf_step(sf_handle* h, const float* lr, int32_t n_steps, float* loss_out) try {
  if (!h || !lr || n_steps < 0) return fail(SF_ERR_INVALID, "bad argument");
  SF_NO_RENDER(h, "sf_step");
  DevGuard dev_guard(h->cfg.device);
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  if (!h->img) return fail(SF_ERR_STATE, "sf_set_target has not been called");
  if (h->graph.want && n_steps >= 2 && !h->ctx->prof && h->npix <= h->chunk_px) return step_replay(h, lr, n_steps, loss_out);
  return eager_steps(h, lr, n_steps, loss_out, loss_out && n_steps > 1, true);   // (a single loss: from the scalar)
} SF_CATCH

int sf_set_graph_replay(sf_handle* h, int32_t on) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_graph_replay");
  h->graph.want = on != 0;
  return SF_OK;
} SF_CATCH

// (the launch context of a WaveletSiren handle is its sub-handles' too: their launches are its records)
int sf_profile_enable(sf_handle* h, int32_t on) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  if (!on) SF_TRY(prof_flush(h->ctx));
  h->ctx->prof = on != 0;
  return SF_OK;
} SF_CATCH
int sf_profile_reset(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(prof_flush(h->ctx));
  LaunchCtx& c = *h->ctx;
  for (int i = 0; i < K_COUNT; ++i) { c.ms[i] = 0; c.n[i] = 0; c.flops[i] = 0; c.bytes[i] = 0; }
  return SF_OK;
} SF_CATCH
int sf_profile_num_kernels(const sf_handle* h, int32_t* n) try {
  if (!h || !n) return fail(SF_ERR_INVALID, "null argument");
  *n = K_COUNT;
  return SF_OK;
} SF_CATCH
int sf_profile_get(sf_handle* h, int32_t idx, const char** name, double* total_ms, int64_t* launches,
                   double* flops_per_launch, double* bytes_per_launch) try {
  if (!h || idx < 0 || idx >= K_COUNT) return fail(SF_ERR_INVALID, "bad kernel index");
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(prof_flush(h->ctx));
  const double ms = h->ctx->ms[idx], fl = h->ctx->flops[idx], by = h->ctx->bytes[idx];
  const int64_t cnt = h->ctx->n[idx];
  if (name) *name = kKernelNames[idx];
  if (total_ms) *total_ms = ms;
  if (launches) *launches = cnt;
  const double nl = cnt > 0 ? (double)cnt : 1.0;
  if (flops_per_launch) *flops_per_launch = fl / nl;
  if (bytes_per_launch) *bytes_per_launch = by / nl;
  return SF_OK;
} SF_CATCH

/* k-means weight quantisation of one tensor on the handle's stream, no host synchronisation (siren_kmeans.hip) */
int sf_kmeans_fit(sf_handle* h, const float* w_dev, int64_t n, float* centers_dev, int32_t K, int32_t iter_limit, float tol,
                  float* centroids_dev, int32_t centroids_cap, int32_t* n_centroids_dev, int64_t* labels_dev,
                  float* new_weight_dev) try {
  if (!h || !w_dev || !centers_dev || !centroids_dev) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_kmeans_fit");
  if (n <= 0 || K < 2 || K >= kKmMaxK || centroids_cap < K + 1 || iter_limit < 0)
    return fail(SF_ERR_INVALID, "sf_kmeans_fit: need n > 0, 2 <= K < 512, centroids_cap >= K + 1, iter_limit >= 0");
  DevGuard dev_guard(h->cfg.device);
  if (!h->km_ws) {
    if (dev_alloc(h, h->km_ws, sizeof(KmWs))) return fail(SF_ERR_NOMEM, "hipMalloc failed (k-means workspace)");
    HIPCHK(hipMemsetAsync(h->km_ws, 0, sizeof(KmWs), h->ctx->stream));
  }
  long blocks = (n + 255) / 256;
  const long cap = 4L * h->dw_wg;
  if (blocks > cap) blocks = cap;
  SF_TRY(launch(h, k_km_init, 1, kKmMaxK, 0, centers_dev, K, n, h->km_ws));
  for (int it = 0; it < iter_limit; ++it) {
    SF_TRY(launch(h, k_km_assign, blocks, 256, 0, w_dev, n, centers_dev, K, h->km_ws));
    SF_TRY(launch(h, k_km_update, 1, kKmMaxK, 0, centers_dev, K, h->km_ws, tol));
  }
  SF_TRY(launch(h, k_km_finish, 1, kKmMaxK, 0, centers_dev, K, h->km_ws, centroids_dev, centroids_cap, n_centroids_dev));
  if (labels_dev || new_weight_dev)
    SF_TRY(launch(h, k_km_predict, blocks, 256, 0, w_dev, n, centroids_dev, h->km_ws, (long long*)labels_dev, new_weight_dev));
  return SF_OK;
} SF_CATCH

/* test aid: throws inside the boundary on purpose (0: std::bad_alloc, 1: std::runtime_error, 2: a non-std exception) */
int sf_debug_throw(int32_t kind) try {
  if (kind == 0) throw std::bad_alloc();
  if (kind == 1) throw std::runtime_error("sf_debug_throw");
  if (kind == 2) throw 42;
  return SF_OK;
} SF_CATCH

}  // extern "C"

#include "quant_host.hip"
#include "many_host.hip"
#include "siren_render.hip"
#include "wavelet_render.hip"
#include "fourier_render.hip"
