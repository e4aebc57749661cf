// siren_mask.hip — the RigL topology update on the device, no host synchronisation (sf_mask_update).
//
// Reference being replaced (paths relative to the reference tree, implicit_image/pipeline/masking/):
//   core.py:425-464   gather_statistics: live / dead counts of every mask, the non-zero share of every layer
//   core.py:250-269   adjust_prune_rate: a layer less than 20 % sparse that holds more than an equal share is pruned by no
//                     more than its own sparsity
//   funcs/prune.py:24-51  magnitude_prune: the ceil(rate * live) smallest |w| among the live weights go
//   funcs/grow.py:58-97   abs_grad_growth: as many come back where |dL/dw| of a masked-out weight is largest, at w = 0
//   core.py:271-289   apply_mask, reset_momentum, apply_mask_gradients
// The host mirror walks the layers in Python: two torch.sort per layer and about eight blocking reads.  Here: two launches
// whatever the depth, one workgroup per masked layer (blockIdx.x runs over the layers).
//
// The contract (per masked layer j, a flat slice of n elements; counts are integers, rates IEEE double):
//   1. live = #{k == 1}, dead = #{k == 0}, nnz = #{w != 0}; S = sum of nnz over the layers               (k_mask_count)
//   2. share = nnz / S, frac_dead = dead / n; rate = min(frac_dead, r) if frac_dead < 0.2 && (1.0 / L) / share < 1.0, else r
//   3. drop = ceil(rate * live)
//   4. drop > 0: the dead + drop elements smallest in (|w_i|, i) get k = 0; removed = live - sum k
//   5. growth 1, unless every k of the layer is 1: c_i = |g_i| * (1 - k_i) in fp32, the `removed` elements largest in c_i
//      (ties: the lower index) get k = 1 and w = +0.0
//   6. w *= k (a product: a pruned negative weight becomes -0.0); dense_gradients == 0: also m *= k, v *= k, g *= k
//   7. the statistics row: the counts before, removed, the counts after, rate
// S == 0 leaves the state alone and sets the status row.
//
// Selection is an exact radix select, not a sort: bits(a) orders like a for a non-negative float a, so four 8-bit histogram
// passes from the top digit find the boundary key and how many of its ties belong to the selection; one more pass ranks
// those ties by index (each wave owns a contiguous segment: a ballot prefix inside a 64-element step, a running count
// along the segment, a scan over the waves) and only when the boundary splits a group of ties.  Growth is the same code on
// the complemented key.  The one key that piles up - |w| = 0 of the dead weights, c = 0 of the live ones - is counted in
// registers and kept out of the histogram.  Every count is an integer (LDS integer atomics commute): the result does not
// depend on the order in which waves arrive.  Every loop runs a trip count derived from n and the wave index, so every
// barrier is reached by every thread of the workgroup.
// (included by siren_fit.hip)

namespace sf {

constexpr int kMaskThreads = 1024;
constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kMaskMaxLayers = 16;

struct MaskRow {                  // sf_mask_layer_stats (include/siren_fit.h); row [n_layers] is the status row
  long long live_before, dead_before, nnz_before, removed, live_after, dead_after, nnz_after;
  double prune_rate;
};

struct MaskArgs {
  float *w, *g, *m, *v, *k;
  MaskRow* rows;
  long long off[kMaskMaxLayers];  // flat offset of each masked layer's weight
  int n[kMaskMaxLayers];
  int L;
  double rate;
  int growth, dense;
};

struct MaskSel {                  // the answer of one radix select (LDS)
  unsigned T;                     // the boundary key: every smaller key is selected
  int take;                       // ... and the first `take` of the `ties` elements that equal it, by index
  int ties;
};

struct MaskLds {
  int hist[256];
  int heavy;
  unsigned prefix;
  int krem;
  int done;
  MaskSel sel;
  int wave_cnt[kMaskWaves];
  int acc[4];
};

// one wave-wide addition per distinct digit of a 64-element step (the top digit of a float takes a handful of values)
__device__ __forceinline__ void mask_hist_add(int* hist, unsigned digit, bool valid, int lane) {
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned d = (unsigned)__shfl((int)digit, leader);
    const unsigned long long same = __ballot(valid && digit == d);
    if (lane == leader) atomicAdd(&hist[d], __popcll(same));
    todo &= ~same;
  }
}

// key of element i: prune, the bits of |w|; grow, the complement of the bits of |g| * (1 - k) - smallest key first both times
template <bool GROW>
__device__ __forceinline__ unsigned mask_key(const float* x, const float* k, int i) {
  if (GROW) return ~__float_as_uint(__fmul_rn(fabsf(x[i]), __fsub_rn(1.0f, k[i])));
  return __float_as_uint(x[i]) & 0x7fffffffu;
}

// The K-th smallest key of n (1 <= K <= n) and the number of its ties inside the selection -> s.sel.  x: the weights
// (prune) or the gradients (grow).  H, the heavy key, is the smallest possible key when pruning and the largest when growing.
template <bool GROW>
__device__ void mask_select(const float* x, const float* k, int n, int K, MaskLds& s) {
  const unsigned H = GROW ? 0xffffffffu : 0u;
  const int t = threadIdx.x, lane = t & 63;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = t; i < 256; i += kMaskThreads) s.hist[i] = 0;
    if (t == 0 && pass == 0) { s.heavy = 0; s.done = 0; s.prefix = 0; }
    __syncthreads();
    const bool done = s.done != 0;
    const unsigned prefix = s.prefix;
    if (!done) {
      int heavy = 0;
      for (int base = t - lane; base < n; base += kMaskThreads) {
        const int i = base + lane;
        const bool in = i < n;
        const unsigned key = in ? mask_key<GROW>(x, k, i) : H;
        if (pass == 0) {
          heavy += in && key == H;
          mask_hist_add(s.hist, key >> 24, in && key != H, lane);
        } else if (in && key != H && (key >> (shift + 8)) == prefix) {
          atomicAdd(&s.hist[(key >> shift) & 255u], 1);
        }
      }
      if (pass == 0 && heavy) atomicAdd(&s.heavy, heavy);
    }
    __syncthreads();
    if (t == 0 && !done) {
      int krem = pass == 0 ? K : s.krem;
      bool stop = false;
      if (pass == 0) {
        const int heavy = s.heavy;
        if (!GROW) {
          if (K <= heavy) { s.sel.T = H; s.sel.take = K; s.sel.ties = heavy; stop = true; }
          else krem = K - heavy;
        } else if (K > n - heavy) {
          s.sel.T = H; s.sel.take = K - (n - heavy); s.sel.ties = heavy; stop = true;
        }
      }
      if (stop) {
        s.done = 1;
      } else {
        int cum = 0, d = 0;
        for (; d < 255; ++d) {
          const int c = s.hist[d];
          if (cum + c >= krem) break;
          cum += c;
        }
        s.prefix = (prefix << 8) | (unsigned)d;
        s.krem = krem - cum;
        if (pass == 3) { s.sel.T = s.prefix; s.sel.take = krem - cum; s.sel.ties = s.hist[d]; }
      }
    }
    __syncthreads();
  }
}

// Ranks of the boundary's ties: when the selection takes only some of them, wave_base = how many lie in the segments of
// the waves before this one.  Every wave owns the contiguous segment [wave * seg, (wave + 1) * seg) of the layer.
template <bool GROW>
__device__ int mask_tie_base(const float* x, const float* k, int n, int seg, MaskLds& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const MaskSel sel = s.sel;
  if (sel.take >= sel.ties) return 0;                         // (uniform: every tie is selected, no rank is needed)
  int cnt = 0;
  const int end = min(n, (wave + 1) * seg);
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    cnt += __popcll(__ballot(i < end && mask_key<GROW>(x, k, i) == sel.T));
  }
  if (lane == 0) s.wave_cnt[wave] = cnt;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s.wave_cnt[w];
  return before;
}

// live / dead / non-zero counts of every masked layer -> its row (the "after" fields start as a copy); status row cleared
__global__ __launch_bounds__(kMaskThreads) void k_mask_count(MaskArgs a) {
  __shared__ int acc[3];
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int n = a.n[j];
  const float* __restrict__ w = a.w + a.off[j];
  const float* __restrict__ k = a.k + a.off[j];
  if (t < 3) acc[t] = 0;
  __syncthreads();
  int live = 0, dead = 0, nnz = 0;
  for (int base = t - lane; base < n; base += kMaskThreads) {
    const int i = base + lane;
    const bool in = i < n;
    const float kv = in ? k[i] : -1.0f, wv = in ? w[i] : 0.0f;
    live += __popcll(__ballot(kv == 1.0f));
    dead += __popcll(__ballot(kv == 0.0f));
    nnz += __popcll(__ballot(wv != 0.0f));
  }
  if (lane == 0) { atomicAdd(&acc[0], live); atomicAdd(&acc[1], dead); atomicAdd(&acc[2], nnz); }
  __syncthreads();
  if (t == 0) {
    MaskRow r;
    r.live_before = r.live_after = acc[0];
    r.dead_before = r.dead_after = acc[1];
    r.nnz_before = r.nnz_after = acc[2];
    r.removed = 0;
    r.prune_rate = 0.0;
    a.rows[j] = r;
    if (j == 0) {
      MaskRow z;
      z.live_before = z.dead_before = z.nnz_before = z.removed = z.live_after = z.dead_after = z.nnz_after = 0;
      z.prune_rate = 0.0;
      a.rows[a.L] = z;
    }
  }
}

// steps 2 - 7 of the contract for layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_mask_update(MaskArgs a) {
  __shared__ MaskLds s;
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = a.n[j];
  float* w = a.w + a.off[j];
  float* g = a.g + a.off[j];
  float* k = a.k + a.off[j];
  long long S = 0;
  for (int l = 0; l < a.L; ++l) S += a.rows[l].nnz_before;
  if (S == 0) {                                               // (uniform over the grid: nothing is touched)
    if (j == 0 && t == 0) a.rows[a.L].live_before = 1;
    return;
  }
  const long long live0 = a.rows[j].live_before, dead0 = a.rows[j].dead_before, nnz0 = a.rows[j].nnz_before;
  const double share = (double)nnz0 / (double)S, frac_dead = (double)dead0 / (double)n;
  const bool capped = frac_dead < 0.2 && (1.0 / (double)a.L) / share < 1.0;
  const double rate = capped ? fmin(frac_dead, a.rate) : a.rate;
  const double dropd = ceil(rate * (double)live0);
  const int seg = ((n + kMaskWaves - 1) / kMaskWaves + 63) / 64 * 64;
  const int end = min(n, (wave + 1) * seg);
  if (t < 4) s.acc[t] = 0;
  __syncthreads();

  // 4. prune
  int removed = 0;
  if (dropd > 0.0) {
    const int K = (int)fmin((double)dead0 + dropd, (double)n);
    mask_select<false>(w, k, n, K, s);
    const int before = mask_tie_base<false>(w, k, n, seg, s);
    const MaskSel sel = s.sel;
    const bool all = sel.take >= sel.ties;
    int run = before, gone = 0;
    for (int base = wave * seg; base < end; base += 64) {
      const int i = base + lane;
      const bool in = i < end;
      const unsigned key = in ? mask_key<false>(w, k, i) : 0xffffffffu;
      const bool tie = in && key == sel.T;
      const unsigned long long tb = __ballot(tie);
      const int rank = run + __popcll(tb & ((1ull << lane) - 1ull));
      run += __popcll(tb);
      const bool pick = in && (key < sel.T || (tie && (all || rank < sel.take)));
      const bool was_live = pick && k[i] == 1.0f;
      if (pick) k[i] = 0.0f;
      gone += __popcll(__ballot(was_live));
    }
    if (lane == 0 && gone) atomicAdd(&s.acc[0], gone);
    __syncthreads();                                          // (the new k of every wave is visible to the growth below)
    removed = s.acc[0];
  }

  // 5. grow
  const bool grow = a.growth == 1 && removed > 0;   // (removed > 0: not every k of the layer is 1)
  int before = 0;
  if (grow) {
    mask_select<true>(g, k, n, min(removed, n), s);
    before = mask_tie_base<true>(g, k, n, seg, s);
  }
  const MaskSel sel = s.sel;
  const bool all = sel.take >= sel.ties;

  // 5. (the picks) + 6. apply + the counts of 7.
  const bool sparse_grads = a.dense == 0;
  float* m = a.m + a.off[j];
  float* v = a.v + a.off[j];
  int run = before, live = 0, dead = 0, nnz = 0;
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    const bool in = i < end;
    float kv = in ? k[i] : -1.0f, wv = in ? w[i] : 0.0f;
    const float gv = in ? g[i] : 0.0f;
    if (grow) {
      const unsigned key = in ? ~__float_as_uint(__fmul_rn(fabsf(gv), __fsub_rn(1.0f, kv))) : 0xffffffffu;
      const bool tie = in && key == sel.T;
      const unsigned long long tb = __ballot(tie);
      const int rank = run + __popcll(tb & ((1ull << lane) - 1ull));
      run += __popcll(tb);
      if (in && (key < sel.T || (tie && (all || rank < sel.take)))) {
        kv = 1.0f;
        wv = 0.0f;
        k[i] = 1.0f;
      }
    }
    if (in) {
      wv = __fmul_rn(wv, kv);
      w[i] = wv;
      if (sparse_grads) {
        m[i] = __fmul_rn(m[i], kv);
        v[i] = __fmul_rn(v[i], kv);
        g[i] = __fmul_rn(gv, kv);
      }
    }
    live += __popcll(__ballot(kv == 1.0f));
    dead += __popcll(__ballot(kv == 0.0f));
    nnz += __popcll(__ballot(in && wv != 0.0f));
  }
  if (lane == 0) { atomicAdd(&s.acc[1], live); atomicAdd(&s.acc[2], dead); atomicAdd(&s.acc[3], nnz); }
  __syncthreads();
  if (t == 0) {
    MaskRow& r = a.rows[j];
    r.removed = removed;
    r.live_after = s.acc[1];
    r.dead_after = s.acc[2];
    r.nnz_after = s.acc[3];
    r.prune_rate = rate;
  }
}

}  // namespace sf
