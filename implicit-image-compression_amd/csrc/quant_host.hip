// quant_host.hip — the quantise phase of a fit (siren_quant.hip states what it computes) on the host: the three entry points
// sf_quant_pass, sf_quant_nudge and sf_quant_step, and what they share under the caller's name - the refusals, the layer table,
// the launches.  Every refusal comes before anything is allocated or launched.  Included by siren_fit.hip behind the
// model-independent entry points (sf_quant_step is their eager_steps with the pass before and the nudge after each step's pass).

namespace {

// what every entry point of the quantise phase refuses, and the layer table of those it takes
int quant_args(sf_engine* h, const sf_quant_args* a, const std::string& fn, KmqArgs& k, long& n_max, double& bytes) {
  if (!h || !a || !a->layers) return fail(SF_ERR_INVALID, fn + ": null argument");
  if (a->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, fn + ": abi_version mismatch");
  SF_NO_RENDER(h, fn.c_str());
  switch (h->model) {
    case Model::Siren: break;
    case Model::Fourier: return fail(SF_ERR_INVALID, fn + ": the quantise phase of a FourierNet handle stays on the host");
    case Model::Wavelet: return fail(SF_ERR_INVALID, fn + ": the quantise phase of a WaveletSiren handle stays on the host");
  }
  if (h->fth.attached) return fail(SF_ERR_INVALID, fn + ": a Feathermap handle has no quantise phase (its weights are materialised)");
  if (a->K < 2 || a->K >= kKmMaxK) return fail(SF_ERR_INVALID, fn + ": need 2 <= K < 512");
  if (a->iter_limit < 0) return fail(SF_ERR_INVALID, fn + ": iter_limit must be >= 0");
  if (a->n_layers < 1 || a->n_layers > h->D || a->n_layers > kKmqMaxLayers)
    return fail(SF_ERR_INVALID, fn + ": n_layers must be 1 .. depth");
  n_max = 0;
  bytes = 0;
  for (int j = 0; j < a->n_layers; ++j) {
    const sf_quant_layer& q = a->layers[j];
    if (q.layer < 0 || q.layer >= h->D || (j > 0 && q.layer <= a->layers[j - 1].layer))
      return fail(SF_ERR_INVALID, fn + ": layers must be ascending indices in [0, depth)");
    if (!q.centers_dev || !q.centroids_dev || !q.labels_dev)
      return fail(SF_ERR_INVALID, fn + ": null argument (centers_dev, centroids_dev and labels_dev of every layer)");
    KmqLayer& y = k.l[j];
    y.off = h->off_w[q.layer];
    y.n = (int)(h->off_b[q.layer] - h->off_w[q.layer]);
    y.centers = q.centers_dev; y.cent = q.centroids_dev; y.n_cent = q.n_centroids_dev;
    y.labels = reinterpret_cast<long long*>(q.labels_dev);
    n_max = std::max(n_max, (long)y.n);
    bytes += (double)y.n * 4;
  }
  k.L = a->n_layers; k.K = a->K; k.tol = a->tol; k.lr = a->nudge_lr;
  k.params = h->params; k.grads = h->grads;
  return SF_OK;
}

// guess, <= iter_limit x (assign, update), finish, predict into the parameters: 3 + 2 * iter_limit launches
int quant_pass(sf_engine* h, KmqArgs& k, int iter_limit, long n_max, double bytes) {
  if (!h->kmq_ws) {
    SF_TRY(dev_alloc(h, h->kmq_ws, sizeof(KmWs) * kKmqMaxLayers));
    HIPCHK(hipMemsetAsync(h->kmq_ws, 0, sizeof(KmWs) * kKmqMaxLayers, h->ctx->stream));
  }
  k.ws = h->kmq_ws;
  // the walk of a layer as sf_kmeans_fit sizes it, shared among the layers: at most four workgroups per compute unit in all
  const long per_layer = std::max(1L, std::min((n_max + 255) / 256, 4L * h->dw_wg / k.L));
  const dim3 walk((unsigned)per_layer, (unsigned)k.L);
  {
    Launch L(h, K_KMQ_GUESS, 0, bytes);
    SF_TRY(launch(h, k_kmq_guess, k.L, kKmqThreads, 0, k));
  }
  for (int it = 0; it < iter_limit; ++it) {
    {
      Launch L(h, K_KMQ_ASSIGN, 0, bytes);
      SF_TRY(launch(h, k_kmq_assign, walk, 256, 0, k));
    }
    Launch L(h, K_KMQ_UPDATE, 0, (double)k.L * k.K * 16);
    SF_TRY(launch(h, k_kmq_update, k.L, kKmqThreads, 0, k));
  }
  {
    Launch L(h, K_KMQ_FINISH, 0, (double)k.L * k.K * 8);
    SF_TRY(launch(h, k_kmq_finish, k.L, kKmqThreads, 0, k));
  }
  {
    Launch L(h, K_KMQ_PREDICT, 0, bytes * 4);   // (the weight read and written, the 8-byte label)
    SF_TRY(launch(h, k_kmq_predict, walk, 256, 0, k));
  }
  h->images_dirty = true;                       // the weights changed under the images
  return SF_OK;
}

int quant_nudge(sf_engine* h, const KmqArgs& k, double bytes) {
  Launch L(h, K_KMQ_NUDGE, 0, bytes * 4);       // (the gradient twice, the 8-byte label)
  return launch(h, k_kmq_nudge, k.L, kKmqThreads, 0, k);
}

}  // namespace

extern "C" {

/* the pre-pass of the quantise phase for every listed layer on the handle's stream: no host synchronisation */
int sf_quant_pass(sf_handle* h, const sf_quant_args* a) try {
  KmqArgs k = zeroed<KmqArgs>();
  long n_max;
  double bytes;
  SF_TRY(quant_args(h, a, "sf_quant_pass", k, n_max, bytes));
  DevGuard dev_guard(h->cfg.device);
  return quant_pass(h, k, a->iter_limit, n_max, bytes);
} SF_CATCH

/* the centroid nudge after a backward for every listed layer: one launch, no host synchronisation */
int sf_quant_nudge(sf_handle* h, const sf_quant_args* a) try {
  KmqArgs k = zeroed<KmqArgs>();
  long n_max;
  double bytes;
  SF_TRY(quant_args(h, a, "sf_quant_nudge", k, n_max, bytes));
  DevGuard dev_guard(h->cfg.device);
  return quant_nudge(h, k, bytes);
} SF_CATCH

/* n_steps x (pass, forward_backward, nudge, Adam), eagerly; the losses through the loss table, read once at the end */
int sf_quant_step(sf_handle* h, const sf_quant_args* a, const float* lr, int32_t n_steps, float* loss_out) try {
  KmqArgs k = zeroed<KmqArgs>();
  long n_max;
  double bytes;
  SF_TRY(quant_args(h, a, "sf_quant_step", k, n_max, bytes));
  if (!lr || n_steps < 0) return fail(SF_ERR_INVALID, "sf_quant_step: bad argument (lr, n_steps)");
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_quant_step: sf_set_coords has not been called");
  if (!h->img) return fail(SF_ERR_STATE, "sf_quant_step: sf_set_target has not been called");
  DevGuard dev_guard(h->cfg.device);
  // (refresh = false: the next pass - of this call, of an eval - rewrites the weights first: one refresh)
  return eager_steps(h, lr, n_steps, loss_out, loss_out && n_steps > 0, false,
                     [&] { return quant_pass(h, k, a->iter_limit, n_max, bytes); }, [&] { return quant_nudge(h, k, bytes); });
} SF_CATCH

}  // extern "C"
