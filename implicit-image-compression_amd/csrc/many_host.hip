// many_host.hip — sf_step_many: n_steps training steps of B fits of one shape, every kernel of a step launched once for all of
// them (kernels: siren_many.hip).  The arguments of every launch are the ones siren_fwd_chunk / siren_bwd_chunk / adam_step /
// refresh_images_siren build for one fit (the same functions build them), filed in tables of B rows in a device block of the
// first handle.  Layout of that block, filled by ONE asynchronous copy per call from a pinned staging block:
//   [step counter, 64 B] [FwdArgs x B] [per layer l = D-1 .. 1: BwdLayerArgs x B, then ReduceArgs x B (last layer) or
//   ReduceVecArgs x B (hidden)] [Dw0Args x B] [ReduceArgs x B (layer 0)] [SseArgs x B] [AdamArgs x B] [ImgArgs x B]
//   [{step_size, bc2_sqrt} x n_steps x B]            ... and behind what the copy fills:   [loss table: double x n_steps x B]
// Shared by the members: the stream, the step counter (k_tick after every step), the grids.  Per fit: every pointer, the
// Adam scalars of its own step count and learning-rate column, its column of the loss table.
// Included by siren_fit.hip after quant_host.hip.

namespace {

int many_refuse(int code, int b, const std::string& what) {
  return fail(code, "sf_step_many: member " + std::to_string(b) + ": " + what);
}

// every refusal of sf_step_many, before anything is launched, allocated or changed
int many_check(sf_engine* const* h, int n_fits, const float* lr, int n_steps) {
  if (!h || !lr) return fail(SF_ERR_INVALID, "sf_step_many: null argument");
  if (n_fits < 1 || n_fits > SF_STEP_MANY_MAX)
    return fail(SF_ERR_INVALID, "sf_step_many: n_fits must be 1.." + std::to_string(SF_STEP_MANY_MAX) + ", got " + std::to_string(n_fits));
  if (n_steps < 0) return fail(SF_ERR_INVALID, "sf_step_many: n_steps < 0");
  for (int b = 0; b < n_fits; ++b) {
    const sf_engine* m = h[b];
    if (!m) return many_refuse(SF_ERR_INVALID, b, "null handle");
    for (int c = 0; c < b; ++c)
      if (h[c] == m) return many_refuse(SF_ERR_INVALID, b, "the same handle as member " + std::to_string(c));
    if (m->render) return many_refuse(SF_ERR_INVALID, b, "a render handle (sf_render_create) holds no training state");
    if (m->model != Model::Siren) return many_refuse(SF_ERR_INVALID, b, "a FourierNet or WaveletSiren handle (SIREN handles only)");
    if (m->fth.attached) return many_refuse(SF_ERR_INVALID, b, "a Feathermap handle");
    if (m->WD > 128) return many_refuse(SF_ERR_INVALID, b, "hidden " + std::to_string(m->WD) + " (the batched kernels are built for 32, 64 and 128)");
    if (m->cfg.compute_dtype != SF_F16) return many_refuse(SF_ERR_INVALID, b, "compute_dtype must be SF_F16");
    if (m->cfg.scratch_format != 16)
      return many_refuse(SF_ERR_INVALID, b, "scratch format " + std::to_string(m->cfg.scratch_format) + " (the batched kernels are those of format 16)");
    if (m->npix > m->chunk_px) return many_refuse(SF_ERR_INVALID, b, "more than one pixel chunk");
    if (m->cfg.row_begin != 0 || m->cfg.row_end != m->cfg.height) return many_refuse(SF_ERR_INVALID, b, "a row range other than the whole picture");
    if (!m->have_coords) return many_refuse(SF_ERR_STATE, b, "sf_set_coords has not been called");
    if (!m->img) return many_refuse(SF_ERR_STATE, b, "sf_set_target has not been called");
    const sf_config &x = m->cfg, &y = h[0]->cfg;
    const char* diff = x.height != y.height || x.width != y.width            ? "height / width"
                       : x.hidden != y.hidden || x.depth != y.depth         ? "hidden / depth"
                       : x.out_features != y.out_features                   ? "out_features"
                       : x.first_omega_0 != y.first_omega_0 || x.hidden_omega_0 != y.hidden_omega_0 ? "the omegas"
                       : (x.outermost_linear != 0) != (y.outermost_linear != 0) ? "outermost_linear"
                       : x.beta1 != y.beta1 || x.beta2 != y.beta2 || x.eps != y.eps ? "betas / eps"
                       : x.device != y.device                               ? "device"
                       : m->ctx->stream != h[0]->ctx->stream                ? "stream"
                                                                            : nullptr;
    if (diff) return many_refuse(SF_ERR_INVALID, b, std::string("differs from member 0 in ") + diff);
  }
  return SF_OK;
}

// offsets of the device block of one call (bytes; every table 64-byte aligned)
struct ManyLayout {
  size_t fwd = 0, bwd[16] = {0}, red[16] = {0}, dw0 = 0, sse = 0, adam = 0, img = 0, steps = 0, filled = 0, loss = 0, total = 0;
};
ManyLayout many_layout(const sf_engine* h0, int B, int n_steps) {
  ManyLayout o;
  size_t at = 64;   // the step counter
  auto take = [&](size_t bytes) { const size_t r = at; at += (bytes + 63) / 64 * 64; return r; };
  o.fwd = take(sizeof(FwdArgs) * B);
  for (int l = h0->D - 1; l >= 1; --l) {
    o.bwd[l] = take(sizeof(BwdLayerArgs) * B);
    o.red[l] = take((reduce_is_vec(h0, l) ? sizeof(ReduceVecArgs) : sizeof(ReduceArgs)) * B);
  }
  o.dw0 = take(sizeof(Dw0Args) * B);
  o.red[0] = take(sizeof(ReduceArgs) * B);
  o.sse = take(sizeof(SseArgs) * B);
  o.adam = take(sizeof(AdamArgs) * B);
  o.img = take(sizeof(ImgArgs) * B);
  o.steps = take(sizeof(float) * 2 * n_steps * B);
  o.filled = at;
  o.loss = take(sizeof(double) * n_steps * B);
  o.total = at;
  return o;
}

template <int WD>
int many_launch_bwd(sf_engine* h0, bool last, bool p0, const BwdLayerArgs* tab, dim3 grid) {
  return with_bool(last, p0, [&](auto l, auto p) {
    constexpr bool LAST = decltype(l)::value, P0 = decltype(p)::value;
    using C = BwdCase<WD, LAST, P0>;
    return launch(h0, k_bwd_many<WD, LAST, P0>, grid, C::threads, C::Lds::bytes, tab);
  });
}

// the launches of n_steps steps on the filled block; images_first: some member's weight images trail its parameters
template <int WD>
int many_run(sf_engine* const* h, int B, int n_steps, const ManyLayout& o, bool images_first) {
  sf_engine* const h0 = h[0];
  char* const dev = h0->many.dev;
  const int D = h0->D;
  const Chunk k = chunk_at(0, h0->npix, h0->chunk_px);
  const double npx = k.n_pb * 32.0, nb = (double)B;
  const BwdGrid g = bwd_grid(h0, k);
  const unsigned y = (unsigned)B;
  int* const counter = reinterpret_cast<int*>(dev);
  const long n_img = images_count(h0);
  auto images = [&]() {
    Launch L(h0, K_IMAGES, 0, nb * (double)n_img * 8);
    return launch(h0, k_images_many, dim3((unsigned)((n_img + 255) / 256), y), 256, 0, reinterpret_cast<const ImgArgs*>(dev + o.img));
  };
  if (images_first) SF_TRY(images());
  for (int s = 0; s < n_steps; ++s) {
    {
      Launch L(h0, K_FWD, nb * flops_fwd_px(h0) * npx, nb * fwd_chunk_bytes(h0, k, true));
      SF_TRY(launch(h0, k_fwd_many<WD>, dim3((unsigned)fwd_grid(h0, k.n_super), y), 512, fwd_lds_bytes(WD),
                    reinterpret_cast<const FwdArgs*>(dev + o.fwd)));
    }
    for (int l = D - 1; l >= 0; --l) {
      const bool last = l == D - 1, p0 = l - 1 == 0;
      const ReduceArgs ra = reduce_args(h0, 0, l, l > 0 ? g.n_wg : dw0_grid(h0, k));   // (the geometry; the pointers are per fit)
      if (l > 0) {
        Launch L(h0, last ? K_BWD_LAST : (p0 ? K_BWD_L1 : K_BWD_HIDDEN), nb * 4.0 * ra.rows_out * WD * npx, nb * bwd_layer_bytes(h0, k, l));
        SF_TRY(many_launch_bwd<WD>(h0, last, p0, reinterpret_cast<const BwdLayerArgs*>(dev + o.bwd[l]), dim3((unsigned)g.n_wg, y)));
      } else {
        Launch L(h0, K_DW_FIRST, nb * 4.0 * WD * npx, nb * WD * 2.0 * npx);
        SF_TRY(launch(h0, k_dw0_many<WD>, dim3((unsigned)ra.n_wg, y), WD * 2, Dw0Lds<WD>::bytes, reinterpret_cast<const Dw0Args*>(dev + o.dw0)));
      }
      const int n = reduce_count(ra);
      Launch L(h0, K_REDUCE, 0, nb * (double)g.n_wg * n * 4.0);
      if (reduce_is_vec(h0, l))
        SF_TRY(launch(h0, k_reduce_vec_many, dim3((unsigned)((n / 4 + 7) / 8), y), 256, 0, reinterpret_cast<const ReduceVecArgs*>(dev + o.red[l])));
      else
        SF_TRY(launch(h0, k_reduce_many, dim3((unsigned)((n + 15) / 16), y), 256, 0, reinterpret_cast<const ReduceArgs*>(dev + o.red[l])));
    }
    {
      Launch L(h0, K_SSE, 0, nb * (double)fwd_grid(h0, k.n_super) * 4);
      SF_TRY(launch(h0, k_sse_reduce_many, dim3(1, y), 256, 0, reinterpret_cast<const SseArgs*>(dev + o.sse)));
    }
    {
      Launch L(h0, K_ADAM, 0, nb * (double)h0->P * 28);
      SF_TRY(launch(h0, k_adam_many, dim3((unsigned)((h0->P + 255) / 256), y), 256, 0, reinterpret_cast<const AdamArgs*>(dev + o.adam)));
    }
    SF_TRY(images());
    SF_TRY(launch(h0, k_tick, 1, 1, 0, counter));
  }
  return SF_OK;
}

// the staging block of this call, filled: every table and the per-step scalars (the counter's 64 bytes are zeros)
void many_fill(sf_engine* const* h, int B, const float* lr, int n_steps, const ManyLayout& o, char* host) {
  sf_engine* const h0 = h[0];
  char* const dev = h0->many.dev;
  const int D = h0->D;
  memset(host, 0, o.filled);
  int* const counter = reinterpret_cast<int*>(dev);
  for (int b = 0; b < B; ++b) {
    const sf_engine* m = h[b];
    const Chunk k = chunk_at(0, m->npix, m->chunk_px);
    const BwdGrid g = bwd_grid(m, k);
    auto row = [&](size_t off, const auto& v) { memcpy(host + off + sizeof(v) * b, &v, sizeof(v)); };
    row(o.fwd, fwd_chunk_args(m, k, true, nullptr, m->sse_part, nullptr));
    for (int l = D - 1; l >= 0; --l) {
      const ReduceArgs ra = reduce_args(m, 0, l, l > 0 ? g.n_wg : dw0_grid(m, k));
      if (l > 0) row(o.bwd[l], bwd_layer_args(m, k, l, g));
      else row(o.dw0, dw0_args(m, k));
      if (reduce_is_vec(m, l)) {
        const int n = reduce_count(ra);
        ReduceVecArgs rv = zeroed<ReduceVecArgs>();
        rv.slab = m->slab; rv.n_wg = g.n_wg; rv.stride = n; rv.n4 = n / 4; rv.out = m->grads + m->off_w[l];
        rv.accumulate = ra.accumulate; rv.scale = ra.scale; rv.scale_dev = ra.scale_dev; rv.scale2_dev = ra.scale2_dev;
        row(o.red[l], rv);
      } else {
        row(o.red[l], ra);
      }
    }
    SseArgs sa = zeroed<SseArgs>();
    sa.part = m->sse_part; sa.n = fwd_grid(m, k.n_super); sa.out = m->sse_dev;
    sa.loss_tab = reinterpret_cast<double*>(dev + o.loss) + (size_t)b * n_steps; sa.iter = counter;
    row(o.sse, sa);
    AdamArgs aa = adam_args(m);
    aa.tab = reinterpret_cast<const float*>(dev + o.steps) + (size_t)b * n_steps * 2; aa.iter = counter;
    row(o.adam, aa);
    row(o.img, images_args(m));
    float* const st = reinterpret_cast<float*>(host + o.steps) + (size_t)b * n_steps * 2;
    for (int s = 0; s < n_steps; ++s) adam_scalars(m, (double)(m->step + s + 1), lr[(size_t)s * B + b], st + 2 * s);
  }
}

// the device block (grown when a call needs more) and a staging block whose last copy has left it
int many_blocks(sf_engine* h0, const ManyLayout& o, char*& host, int& slot) {
  sf_engine::Many& m = h0->many;
  if (m.dev_cap < o.total) {
    dev_free(h0, m.dev);   // (hipFree waits for the device: no earlier call still reads the old block)
    m.dev = nullptr; m.dev_cap = 0;
    SF_TRY(dev_alloc(h0, m.dev, o.total));
    m.dev_cap = o.total;
  }
  slot = m.turn;
  m.turn ^= 1;
  if (m.pending[slot]) {   // the copy of the call before the last one: long done unless the caller runs far ahead of the device
    HIPCHK(hipEventSynchronize(m.ev[slot]));
    m.pending[slot] = false;
  }
  if (!m.ev[slot]) HIPCHK(hipEventCreateWithFlags(&m.ev[slot], hipEventDisableTiming));
  if (m.host_cap[slot] < o.filled) {
    if (m.host[slot]) { hipHostFree(m.host[slot]); m.host[slot] = nullptr; m.host_cap[slot] = 0; }
    void* p = nullptr;
    if (hipHostMalloc(&p, o.filled, hipHostMallocDefault) != hipSuccess) return fail(SF_ERR_NOMEM, "sf_step_many: hipHostMalloc failed");
    m.host[slot] = static_cast<char*>(p);
    m.host_cap[slot] = o.filled;
  }
  host = m.host[slot];
  return SF_OK;
}

}  // namespace

extern "C" {

int sf_step_many(sf_handle* const* h, int32_t n_fits, const float* lr, int32_t n_steps, float* loss_out) try {
  SF_TRY(many_check(h, n_fits, lr, n_steps));
  if (n_steps == 0) return SF_OK;
  sf_engine* const h0 = h[0];
  DevGuard dev_guard(h0->cfg.device);
  const ManyLayout o = many_layout(h0, n_fits, n_steps);
  char* host = nullptr;
  int slot = 0;
  SF_TRY(many_blocks(h0, o, host, slot));
  many_fill(h, n_fits, lr, n_steps, o, host);
  hipStream_t stream = h0->ctx->stream;
  HIPCHK(hipMemcpyAsync(h0->many.dev, host, o.filled, hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(h0->many.ev[slot], stream));
  h0->many.pending[slot] = true;
  bool images_first = false;
  for (int b = 0; b < n_fits; ++b) images_first = images_first || h[b]->images_dirty;
  for (int b = 0; b < n_fits; ++b) h[b]->images_dirty = true;   // (until the last launch below is out: a failure leaves them to be rebuilt)
  const int rc = h0->WD == 32 ? many_run<32>(h, n_fits, n_steps, o, images_first)
                 : h0->WD == 64 ? many_run<64>(h, n_fits, n_steps, o, images_first)
                                : many_run<128>(h, n_fits, n_steps, o, images_first);
  if (rc) return rc;
  for (int b = 0; b < n_fits; ++b) { h[b]->step += n_steps; h[b]->images_dirty = false; }
  if (!loss_out) return SF_OK;
  std::vector<double> sse((size_t)n_fits * n_steps);
  HIPCHK(hipMemcpyAsync(sse.data(), h0->many.dev + o.loss, sse.size() * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const double n_values = (double)h0->cfg.out_features * (double)h0->npix;
  for (int b = 0; b < n_fits; ++b)
    for (int s = 0; s < n_steps; ++s) loss_out[(size_t)s * n_fits + b] = (float)(sse[(size_t)b * n_steps + s] / n_values);
  return SF_OK;
} SF_CATCH

}  // extern "C"
