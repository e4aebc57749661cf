// mask_host.hip — the topology updates of a masked fit (siren_mask.hip states what they compute) on the host: the three entry
// points sf_mask_update, sf_mask_prune_global and sf_mask_update_snfs, and what they share under the caller's name - the refusals, the walk over
// the layers, the state pointers, the epilogue.  An entry point keeps its own argument checks and its launches; the order
// of the checks is: the shared refusals, its own, the layers.  Included by siren_fit.hip.

namespace {

static_assert(sizeof(MaskRow) == sizeof(sf_mask_layer_stats), "MaskRow is sf_mask_layer_stats");
static_assert(sizeof(SnfsRow) == sizeof(sf_mask_snfs_stats), "SnfsRow is sf_mask_snfs_stats");

// what every topology update refuses before it looks at its own arguments (A: an argument struct of the ABI)
template <class A>
int mask_refuse(const sf_engine* h, const A* a, const std::string& fn) {
  if (!h || !a || !a->layers) return fail(SF_ERR_INVALID, "null argument");
  if (a->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, "abi_version mismatch");
  SF_NO_RENDER(h, fn.c_str());
  switch (h->model) {
    case Model::Siren: break;
    case Model::Fourier: return fail(SF_ERR_INVALID, fn + ": a FourierNet handle takes no mask");
    case Model::Wavelet: return fail(SF_ERR_INVALID, fn + ": topology updates of a WaveletSiren handle stay on the host");
  }
  if (h->fth.attached) return fail(SF_ERR_INVALID, fn + ": a Feathermap handle is dense (masking.dense: True)");
  if (!h->has_mask) return fail(SF_ERR_STATE, fn + ": sf_set_masks has not been called");
  return SF_OK;
}

// a->layers (ascending layer indices) into k.off / k.n, with the scalars every update takes; bytes: the size of the listed
// weights, n_max: the largest of them
template <class A>
int mask_layers(const sf_engine* h, const A* a, const std::string& fn, MaskArgs& k, double& bytes, int& n_max) {
  if (a->n_layers < 1 || a->n_layers > h->D || a->n_layers > kMaskMaxLayers)
    return fail(SF_ERR_INVALID, fn + ": n_layers must be 1 .. depth");
  bytes = 0;
  n_max = 0;
  for (int j = 0; j < a->n_layers; ++j) {
    const int l = a->layers[j];
    if (l < 0 || l >= h->D || (j > 0 && l <= a->layers[j - 1]))
      return fail(SF_ERR_INVALID, fn + ": layers must be ascending indices in [0, depth)");
    k.off[j] = h->off_w[l];
    k.n[j] = (int)(h->off_b[l] - h->off_w[l]);
    n_max = std::max(n_max, k.n[j]);
    bytes += (double)k.n[j] * 4;
  }
  k.L = a->n_layers; k.rate = a->prune_rate; k.dense = a->dense_gradients != 0;
  return SF_OK;
}

// the handle's state into k, and the statistics rows - the caller's, or the handle's own (`own`, allocated on first use) -
// into rows
template <class Row>
int mask_bind(sf_engine* h, void* stats_dev, Row*& own, MaskArgs& k, Row*& rows) {
  if (!stats_dev && !own) SF_TRY(dev_alloc(h, own, sizeof(Row) * (kMaskMaxLayers + 1)));
  k.w = h->params; k.g = h->grads; k.m = h->m; k.v = h->v; k.k = h->mask;
  rows = stats_dev ? reinterpret_cast<Row*>(stats_dev) : own;
  return SF_OK;
}

// after the launches: the weights changed under the images and under a materialised Feathermap
void mask_done(sf_engine* h) {
  h->images_dirty = true;
  h->fth.fresh = false;
}

}  // namespace

extern "C" {

/* one RigL topology update of the masked layers on the handle's stream: two launches, no host synchronisation */
int sf_mask_update(sf_handle* h, const sf_mask_update_args* a) try {
  const char* fn = "sf_mask_update";
  SF_TRY(mask_refuse(h, a, fn));
  if (a->growth != 0 && a->growth != 1) return fail(SF_ERR_INVALID, "sf_mask_update: growth must be 0 (none) or 1 (absolute gradient)");
  MaskArgs k = zeroed<MaskArgs>();
  double bytes;
  int n_max;
  SF_TRY(mask_layers(h, a, fn, k, bytes, n_max));
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(mask_bind(h, a->stats_dev, h->mask_rows, k, k.rows));
  k.growth = a->growth;
  {
    Launch L(h, K_MASK, 0, bytes * 12);   // (about a dozen L2-resident reads of every masked layer)
    SF_TRY(launch(h, k_mask_count, k.L, kMaskThreads, 0, k));
    SF_TRY(launch(h, k_mask_update, k.L, kMaskThreads, 0, k));
  }
  mask_done(h);
  return SF_OK;
} SF_CATCH

/* one global-magnitude topology update (masking=Pruning) of the masked layers on the handle's stream: six launches whatever
 * the depth and the number of trials, no host synchronisation */
int sf_mask_prune_global(sf_handle* h, const sf_mask_prune_global_args* a) try {
  const char* fn = "sf_mask_prune_global";
  SF_TRY(mask_refuse(h, a, fn));
  if (!(std::isfinite(a->threshold) && a->threshold > 0.0))
    return fail(SF_ERR_INVALID, "sf_mask_prune_global: threshold must be finite and > 0");
  if (!(a->increment > 0.0 && a->increment < 1.0)) return fail(SF_ERR_INVALID, "sf_mask_prune_global: increment must lie in (0, 1)");
  if (!(std::isfinite(a->tolerance) && a->tolerance >= 0.0))
    return fail(SF_ERR_INVALID, "sf_mask_prune_global: tolerance must be finite and >= 0");
  if (a->target < 0) return fail(SF_ERR_INVALID, "sf_mask_prune_global: target must be >= 0");
  PruneArgs p = zeroed<PruneArgs>();
  MaskArgs& k = p.m;
  double bytes;
  int n_max;
  SF_TRY(mask_layers(h, a, fn, k, bytes, n_max));
  if (h->P > 0x7fffffff) return fail(SF_ERR_INVALID, "sf_mask_prune_global: more than 2^31 - 1 parameters");
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(mask_bind(h, a->stats_dev, h->mask_rows, k, k.rows));
  if (!h->prune_ws) SF_TRY(dev_alloc(h, h->prune_ws, sizeof(PruneWs)));
  if (!h->prune_keys) SF_TRY(dev_alloc(h, h->prune_keys, (size_t)h->P * 4));
  p.ws = h->prune_ws; p.keys = h->prune_keys; p.cap = (int)h->P;
  p.target = a->target; p.threshold = a->threshold; p.increment = a->increment; p.tolerance = a->tolerance;
  // strides per layer: 16 elements per thread of the largest layer, at most four workgroups per compute unit in all
  const int per_layer = std::max(1, std::min((n_max + kMaskThreads * 16 - 1) / (kMaskThreads * 16), 4 * h->dw_wg / k.L));
  const dim3 grid(k.L, per_layer);
  {
    Launch L(h, K_MASK_PRUNE, 0, bytes * 12);   // (the weights three times, the keys, the five state vectors once)
    HIPCHK(hipMemsetAsync(h->prune_ws->hist, 0, sizeof(h->prune_ws->hist), h->ctx->stream));
    SF_TRY(launch(h, k_mask_count, k.L, kMaskThreads, 0, k));
    SF_TRY(launch(h, k_prune_file<false>, grid, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_prune_scan, 1, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_prune_file<true>, grid, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_prune_search, 1, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_prune_apply, grid, kMaskThreads, 0, p));
  }
  mask_done(h);
  return SF_OK;
} SF_CATCH

/* one SNFS topology update (momentum growth, momentum redistribution) of the masked layers on the handle's stream: three
 * launches whatever the depth and the number of water-filling rounds, no host synchronisation */
int sf_mask_update_snfs(sf_handle* h, const sf_mask_update_snfs_args* a) try {
  const char* fn = "sf_mask_update_snfs";
  SF_TRY(mask_refuse(h, a, fn));
  if (a->growth != 1 && a->growth != 2)
    return fail(SF_ERR_INVALID, "sf_mask_update_snfs: growth must be 1 (absolute gradient) or 2 (momentum)");
  if (a->statistic != 0 && a->statistic != 1)
    return fail(SF_ERR_INVALID, "sf_mask_update_snfs: statistic must be 0 (non-zero count) or 1 (momentum)");
  if (!(std::isfinite(a->adjusted_growth) && a->adjusted_growth >= 0.0))
    return fail(SF_ERR_INVALID, "sf_mask_update_snfs: adjusted_growth must be finite and >= 0");
  SnfsArgs p = zeroed<SnfsArgs>();
  MaskArgs& k = p.m;
  double bytes;
  int n_max;
  SF_TRY(mask_layers(h, a, fn, k, bytes, n_max));
  DevGuard dev_guard(h->cfg.device);
  SF_TRY(mask_bind(h, a->stats_dev, h->snfs_rows, k, p.rows));
  k.growth = a->growth;
  p.adjusted_growth = a->adjusted_growth;
  p.statistic = a->statistic;
  {
    Launch L(h, K_MASK_SNFS, 0, bytes * 20);   // (about twenty L2-resident reads of every masked layer)
    SF_TRY(launch(h, k_snfs_stat, k.L, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_snfs_prune, k.L, kMaskThreads, 0, p));
    SF_TRY(launch(h, k_snfs_grow, k.L, kMaskThreads, 0, p));
  }
  mask_done(h);
  return SF_OK;
} SF_CATCH

}  // extern "C"
