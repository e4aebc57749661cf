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
// A device helper that holds a barrier or a wave-wide ballot is left early only on a condition that is uniform over the
// workgroup (the wave), and says so.
// (included by siren_fit.hip; the two entry points are in mask_host.hip)

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
  int acc[4];                     // live, dead, non-zero after the update; the live weights the prune removed
};

struct MaskLayer {                // the state of one masked layer
  float *w, *g, *m, *v, *k;
  int n;
};

__device__ __forceinline__ MaskLayer mask_layer(const MaskArgs& a, int j) {
  const long long o = a.off[j];
  return {a.w + o, a.g + o, a.m + o, a.v + o, a.k + o, a.n[j]};
}

// step 2 of the contract: the rate of layer j (n elements) of L, from the counts of its row; S the non-zeros of all layers
__device__ __forceinline__ double mask_rate(const MaskRow* rows, int j, int n, int L, long long S, double r) {
  const double share = (double)rows[j].nnz_before / (double)S, frac_dead = (double)rows[j].dead_before / (double)n;
  const bool capped = frac_dead < 0.2 && (1.0 / (double)L) / share < 1.0;
  return capped ? fmin(frac_dead, r) : r;
}

// The count-and-commit form of every kernel that counts: a lane tallies its own elements, the wave adds its lanes up once,
// and lane 0 adds the wave's sums to acc[0 .. 2] (live, dead, non-zero) in LDS.  The caller zeroes acc behind a barrier
// before and reads it behind one after; every lane of a wave reaches commit (a wave-wide shuffle).
struct MaskTally {
  int live, dead, nnz;
  __device__ __forceinline__ void add(float wv, float kv) {
    live += kv == 1.0f;
    dead += kv == 0.0f;
    nnz += wv != 0.0f;
  }
  __device__ __forceinline__ void commit(int* acc, int lane) {
    for (int d = 32; d > 0; d >>= 1) {
      live += __shfl_down(live, d);
      dead += __shfl_down(dead, d);
      nnz += __shfl_down(nnz, d);
    }
    if (lane == 0) { atomicAdd(&acc[0], live); atomicAdd(&acc[1], dead); atomicAdd(&acc[2], nnz); }
  }
};

// step 6 of the contract for element i, whose weight wv, gradient gv (read only with sparse gradients) and new mask value kv
// the caller holds, and its share of the counts of step 7.  Products: a pruned negative weight becomes -0.0.
__device__ __forceinline__ void mask_apply(const MaskLayer& p, int i, float wv, float gv, float kv, bool sparse_grads,
                                           MaskTally& c) {
  wv = __fmul_rn(wv, kv);
  p.w[i] = wv;
  if (sparse_grads) {
    p.m[i] = __fmul_rn(p.m[i], kv);
    p.v[i] = __fmul_rn(p.v[i], kv);
    p.g[i] = __fmul_rn(gv, kv);
  }
  c.add(wv, kv);
}

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

// key of an element: prune, the bits of |w|; grow, the complement of the bits of |g| * (1 - k) - smallest key first both times
template <bool GROW>
__device__ __forceinline__ unsigned mask_key(float x, float k) {
  if (GROW) return ~__float_as_uint(__fmul_rn(fabsf(x), __fsub_rn(1.0f, k)));
  return __float_as_uint(x) & 0x7fffffffu;
}
template <bool GROW>
__device__ __forceinline__ unsigned mask_key(const float* x, const float* k, int i) {
  return mask_key<GROW>(x[i], GROW ? k[i] : 0.0f);
}

// The tie-ranked pick of one 64-element step of a wave's segment: every key below the boundary, and the boundary's ties up to
// rank sel.take (all: every tie).  run: the ties before this step, advanced by the step's.  A wave-wide ballot: every lane
// of the wave calls it, `in` false where the lane has no element.
__device__ __forceinline__ bool mask_pick(unsigned key, bool in, const MaskSel& sel, bool all, int& run, int lane) {
  const bool tie = in && key == sel.T;
  const unsigned long long tb = __ballot(tie);
  const int rank = run + __popcll(tb & ((1ull << lane) - 1ull));
  run += __popcll(tb);
  return in && (key < sel.T || (tie && (all || rank < sel.take)));
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
  const int j = blockIdx.x, t = threadIdx.x;
  const MaskLayer p = mask_layer(a, j);
  if (t < 3) acc[t] = 0;
  __syncthreads();
  MaskTally c{};
  for (int i = t; i < p.n; i += kMaskThreads) c.add(p.w[i], p.k[i]);
  c.commit(acc, t & 63);
  __syncthreads();
  if (t == 0) {
    MaskRow r{};
    r.live_before = r.live_after = acc[0];
    r.dead_before = r.dead_after = acc[1];
    r.nnz_before = r.nnz_after = acc[2];
    a.rows[j] = r;
    if (j == 0) a.rows[a.L] = MaskRow{};
  }
}

// steps 2 - 7 of the contract for layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_mask_update(MaskArgs a) {
  __shared__ MaskLds s;
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const MaskLayer p = mask_layer(a, j);
  const int n = p.n;
  long long S = 0;
  for (int l = 0; l < a.L; ++l) S += a.rows[l].nnz_before;
  if (S == 0) {                                               // (uniform over the grid: nothing is touched)
    if (j == 0 && t == 0) a.rows[a.L].live_before = 1;
    return;
  }
  const long long live0 = a.rows[j].live_before, dead0 = a.rows[j].dead_before;
  const double rate = mask_rate(a.rows, j, n, a.L, S, a.rate);
  const double dropd = ceil(rate * (double)live0);
  const int seg = ((n + kMaskWaves - 1) / kMaskWaves + 63) / 64 * 64;
  const int end = min(n, (wave + 1) * seg);
  if (t < 4) s.acc[t] = 0;
  __syncthreads();

  // 4. prune
  int removed = 0;
  if (dropd > 0.0) {
    const int K = (int)fmin((double)dead0 + dropd, (double)n);
    mask_select<false>(p.w, p.k, n, K, s);
    int run = mask_tie_base<false>(p.w, p.k, n, seg, s), gone = 0;
    const MaskSel sel = s.sel;
    const bool all = sel.take >= sel.ties;
    for (int base = wave * seg; base < end; base += 64) {
      const int i = base + lane;
      const bool in = i < end;
      const bool pick = mask_pick(in ? mask_key<false>(p.w, p.k, i) : 0xffffffffu, in, sel, all, run, lane);
      const bool was_live = pick && p.k[i] == 1.0f;
      if (pick) p.k[i] = 0.0f;
      gone += __popcll(__ballot(was_live));
    }
    if (lane == 0 && gone) atomicAdd(&s.acc[3], gone);
    __syncthreads();                                          // (the new k of every wave is visible to the growth below)
    removed = s.acc[3];
  }

  // 5. grow
  const bool grow = a.growth == 1 && removed > 0;   // (removed > 0: not every k of the layer is 1)
  int run = 0;
  if (grow) {
    mask_select<true>(p.g, p.k, n, min(removed, n), s);
    run = mask_tie_base<true>(p.g, p.k, n, seg, s);
  }
  const MaskSel sel = s.sel;
  const bool all = sel.take >= sel.ties;

  // 5. (the picks) + 6. apply + the counts of 7.
  const bool sparse_grads = a.dense == 0;
  MaskTally c{};
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    const bool in = i < end;
    float kv = in ? p.k[i] : -1.0f, wv = in ? p.w[i] : 0.0f;
    const float gv = in ? p.g[i] : 0.0f;
    // (grow is uniform over the workgroup: every lane of the wave reaches the pick's ballot or none does)
    if (grow && mask_pick(in ? mask_key<true>(gv, kv) : 0xffffffffu, in, sel, all, run, lane)) {
      kv = 1.0f;
      wv = 0.0f;
      p.k[i] = 1.0f;
    }
    if (in) mask_apply(p, i, wv, gv, kv, sparse_grads, c);
  }
  c.commit(s.acc, lane);
  __syncthreads();
  if (t == 0) {
    MaskRow& r = a.rows[j];
    r.removed = removed;
    r.live_after = s.acc[0];
    r.dead_after = s.acc[1];
    r.nnz_after = s.acc[2];
    r.prune_rate = rate;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// sf_mask_prune_global — the global-magnitude update of masking=Pruning on the device, no host synchronisation.
//
// Reference being replaced: funcs/prune.py:54-104 global_magnitude_prune (one |w| threshold over all masked layers, nudged
// multiplicatively until the number of weights it removes is within `tolerance` of the target or the count has stalled ten
// times) inside core.py:713-801 truncate_weights with growth_mode none.  The host mirror sorts every masked weight and reads
// one count back per trial - hundreds of blocking reads per update.  Here: six launches whatever the depth and however
// many trials the search takes.
//
// The contract (counts exact integers; threshold arithmetic IEEE double, round to nearest, no contraction):
//   1. per listed layer j: live_j, dead_j, nnz_j as step 1 above; S = sum nnz_j, alive = sum live_j.  S == 0: status 1,
//      nothing else is touched
//   2. rate_j as step 2 above with r = prune_rate (bookkeeping only)
//   3. target <= 0: no search - the masks keep their values, removed = 0, trials = 0, the threshold is unchanged
//   4. slack = target * tolerance; step = increment; removed = previous = stalled = 0
//      while |removed - target| > slack:
//        a. removed = alive - #{ i in the listed layers : |w_i| > f32(threshold) }   (an fp32 comparison over every element,
//           dead ones included; f32: the double rounded to nearest-even); trials += 1
//        b. stalled = stalled + 1 if removed == previous else 0
//        c. stalled == 10: break
//        d. previous = removed
//        e. removed > target * (1.0 + tolerance): threshold *= 1.0 - step; step *= 0.99
//           else removed < target * (1.0 - tolerance): threshold *= 1.0 + step; step *= 0.99
//      a 4097th trial is never evaluated (kPruneTrialCap): status 2, nothing else is touched
//   5. a search ran: k_i = |w_i| > f32(threshold) ? 1 : 0 with the final threshold
//   6. w_i *= k_i (a product); dense_gradients == 0: also m_i *= k_i, v_i *= k_i, g_i *= k_i
//   7. row j: the counts before, removed = live_before - live_after, the counts after, rate_j;
//      status row: status, trials, alive, the search's last `removed`, target, 0, 0, bits of the final threshold (double)
//
// bits(|w|) orders like |w|, so "how many keys exceed the threshold's key" needs no sort: k_prune_file<false> counts the keys by
// their top 16 bits (integer atomics), k_prune_scan turns the counts into bucket offsets, k_prune_file<true> files every key
// under its bucket (in any order: only counts are taken), and k_prune_search - one workgroup - runs the trials: the
// buckets above the threshold's come from the prefix, the threshold's own bucket is counted cooperatively, and a trial
// whose fp32 threshold did not move reuses the last count.  Keys 0 (never above a threshold) and NaN (never above one in
// an fp32 comparison) are filed nowhere.  One lane does the double arithmetic of a trial; the loop's continue / stop
// decision is one LDS word that every thread reads behind a barrier, so every barrier is reached by every thread.
// k_prune_apply (steps 5 - 7) adds its integer counts to the rows with 64-bit integer atomics.

constexpr int kPruneTrialCap = 4096;
constexpr int kPruneBins = 1 << 16;               // key >> 15: the 8 exponent bits and the top 8 mantissa bits
constexpr unsigned kPruneInf = 0x7f800000u;

struct PruneCtl {                 // what the search leaves for k_prune_apply
  int mode;                       // 0 nothing is touched (S == 0, cap reached), 1 no search: the masks keep their values, 2 a search ran
  unsigned tkey;                  // bits of f32(final threshold)
};

struct PruneWs {                  // the scratch of one handle (allocated on the first sf_mask_prune_global)
  int hist[kPruneBins];           // keys per bucket; the cursors of k_prune_file<true> afterwards
  int start[kPruneBins + 1];      // exclusive prefix of hist: bucket b is keys[start[b] .. start[b + 1])
  PruneCtl ctl;
};

struct PruneArgs {
  MaskArgs m;                     // w, g, m, v, k, rows, off, n, L, rate, dense (growth unused)
  PruneWs* ws;
  unsigned* keys;                 // cap entries
  int cap;
  int pad;
  long long target;
  double threshold, increment, tolerance;
};

__device__ __forceinline__ bool prune_filed(unsigned key) { return key != 0u && key <= kPruneInf; }

// blockIdx.x: the layer, blockIdx.y: a stride over its elements.  SCATTER false: hist[bucket] += 1; true: the key goes to
// the next free slot of its bucket (hist holds the cursors, k_prune_scan set them to the bucket starts)
template <bool SCATTER>
__global__ __launch_bounds__(kMaskThreads) void k_prune_file(PruneArgs a) {
  const MaskLayer p = mask_layer(a.m, blockIdx.x);
  for (int i = blockIdx.y * kMaskThreads + threadIdx.x; i < p.n; i += gridDim.y * kMaskThreads) {
    const unsigned key = mask_key<false>(p.w, p.k, i);
    if (!prune_filed(key)) continue;
    const int pos = atomicAdd(&a.ws->hist[key >> 15], 1);
    if (SCATTER && pos >= 0 && pos < a.cap) a.keys[pos] = key;
  }
}

// exclusive prefix of the 65 536 bucket counts -> start (and into hist, as the scatter's cursors); one workgroup
__global__ __launch_bounds__(kMaskThreads) void k_prune_scan(PruneArgs a) {
  __shared__ int part[kMaskThreads];
  constexpr int kPer = kPruneBins / kMaskThreads;
  const int t = threadIdx.x;
  int* hist = a.ws->hist;
  int sum = 0;
  for (int i = 0; i < kPer; ++i) sum += hist[t * kPer + i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kMaskThreads; d <<= 1) {                // (Hillis-Steele, inclusive)
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int i = 0; i < kPer; ++i) {
    const int c = hist[t * kPer + i];
    a.ws->start[t * kPer + i] = run;
    hist[t * kPer + i] = run;
    run += c;
  }
  if (t == kMaskThreads - 1) a.ws->start[kPruneBins] = run;
}

struct PruneLds {
  int go;                         // the loop's decision: 1 another trial is evaluated (never written after the loop)
  int touch;                      // after the loop: the state is updated (a status of 0 with something to do)
  int recount;                    // ... and its fp32 threshold differs from the last one's
  unsigned tkey;
  int lo, hi;                     // the threshold's bucket in keys
  int cnt;                        // keys of that bucket above the threshold
  long long above;                // keys in the buckets above it
};

// steps 2 - 4 and the status row; one workgroup
__global__ __launch_bounds__(kMaskThreads) void k_prune_search(PruneArgs a) {
  __shared__ PruneLds s;
  const int t = threadIdx.x, lane = t & 63, L = a.m.L;
  MaskRow* rows = a.m.rows;
  const int* start = a.ws->start;
  long long S = 0, alive = 0;
  for (int l = 0; l < L; ++l) { S += rows[l].nnz_before; alive += rows[l].live_before; }
  const long long target = a.target;
  const int mode = S == 0 ? 0 : target <= 0 ? 1 : 2;
  // the search's state lives in thread 0
  const double tgt = (double)target, tol = a.tolerance;
  const double slack = __dmul_rn(tgt, tol);
  const double hi_bound = __dmul_rn(tgt, __dadd_rn(1.0, tol)), lo_bound = __dmul_rn(tgt, __dsub_rn(1.0, tol));
  double thr = a.threshold, step = a.increment;
  long long removed = 0, previous = 0, last_count = 0;
  int stalled = 0, trials = 0, status = S == 0 ? 1 : 0;
  unsigned last_tkey = 0xffffffffu;
  auto aim = [&]() {                                          // (thread 0) the next trial's threshold as a key and a bucket
    const unsigned tkey = __float_as_uint(__double2float_rn(thr));
    s.tkey = tkey;
    s.recount = tkey != last_tkey;
    if (tkey != last_tkey) {
      const int b = (int)(tkey >> 15);                        // (thr > 0: the sign bit is clear, b < kPruneBins)
      s.lo = start[b];
      s.hi = start[b + 1];
      s.above = (long long)start[kPruneBins] - start[b + 1];
      if (tkey > kPruneInf) { s.lo = s.hi = 0; s.above = 0; }  // (unreachable for a finite double; nothing exceeds a NaN)
    }
    s.cnt = 0;
  };
  if (t == 0) {
    s.go = mode == 2 && fabs((double)(removed - target)) > slack;
    if (s.go) aim();
  }
  for (int it = 0; it <= kPruneTrialCap; ++it) {
    __syncthreads();
    if (!s.go) break;                                         // (one LDS word, read by every thread behind the barrier)
    if (s.recount) {
      const unsigned tkey = s.tkey;
      const int hi = s.hi;
      int c = 0;
      for (int i = s.lo + t; i < hi; i += kMaskThreads) c += a.keys[i] > tkey;
      for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
      if (lane == 0 && c) atomicAdd(&s.cnt, c);
    }
    __syncthreads();
    if (t == 0) {
      if (trials == kPruneTrialCap) {                         // the cap: the search is abandoned
        status = 2;
        s.go = 0;
      } else {
        if (s.recount) { last_count = s.above + s.cnt; last_tkey = s.tkey; }
        removed = alive - last_count;                                                        // a.
        ++trials;
        stalled = removed == previous ? stalled + 1 : 0;                                     // b.
        if (stalled == 10) {                                                                 // c.
          s.go = 0;
        } else {
          previous = removed;                                                                // d.
          const double r = (double)removed;
          if (r > hi_bound) { thr = __dmul_rn(thr, __dsub_rn(1.0, step)); step = __dmul_rn(step, 0.99); }        // e.
          else if (r < lo_bound) { thr = __dmul_rn(thr, __dadd_rn(1.0, step)); step = __dmul_rn(step, 0.99); }
          s.go = fabs((double)(removed - target)) > slack;
          if (s.go) aim();
        }
      }
    }
  }
  // (every thread left the loop at its first barrier)
  const bool touch = mode != 0 && status == 0;                // (thread 0 only knows status; the others use ctl below)
  if (t == 0) {
    a.ws->ctl.mode = touch ? mode : 0;
    a.ws->ctl.tkey = __float_as_uint(__double2float_rn(thr));
    MaskRow z{};
    z.live_before = status;
    z.dead_before = trials;
    z.nnz_before = alive;
    z.removed = removed;
    z.live_after = target;
    z.prune_rate = status == 0 ? thr : a.threshold;
    rows[L] = z;
    s.touch = touch;
  }
  __syncthreads();
  if (t < L && s.touch) {                                        // 2. the rates; the "after" counts restart for k_prune_apply
    rows[t].prune_rate = mask_rate(rows, t, a.m.n[t], L, S, a.m.rate);
    rows[t].removed = rows[t].live_before;
    rows[t].live_after = rows[t].dead_after = rows[t].nnz_after = 0;
  }
}

// steps 5 - 7 for a stride (blockIdx.y) of layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_prune_apply(PruneArgs a) {
  __shared__ int acc[3];
  const int mode = a.ws->ctl.mode;
  if (mode == 0) return;                                      // (uniform over the grid)
  const unsigned tkey = a.ws->ctl.tkey;
  const int j = blockIdx.x, t = threadIdx.x;
  const MaskLayer p = mask_layer(a.m, j);
  const bool sparse_grads = a.m.dense == 0;
  if (t < 3) acc[t] = 0;
  __syncthreads();
  MaskTally c{};
  for (int i = blockIdx.y * kMaskThreads + t; i < p.n; i += gridDim.y * kMaskThreads) {
    const float wv = p.w[i];
    float kv = p.k[i];
    if (mode == 2) {
      const unsigned key = mask_key<false>(wv, kv);
      kv = key > tkey && key <= kPruneInf ? 1.0f : 0.0f;
      p.k[i] = kv;
    }
    mask_apply(p, i, wv, sparse_grads ? p.g[i] : 0.0f, kv, sparse_grads, c);
  }
  c.commit(acc, t & 63);
  __syncthreads();
  if (t == 0) {
    MaskRow& r = a.m.rows[j];
    using u64 = unsigned long long;
    atomicAdd(reinterpret_cast<u64*>(&r.live_after), (u64)acc[0]);
    atomicAdd(reinterpret_cast<u64*>(&r.dead_after), (u64)acc[1]);
    atomicAdd(reinterpret_cast<u64*>(&r.nnz_after), (u64)acc[2]);
    atomicAdd(reinterpret_cast<u64*>(&r.removed), (u64)(-(long long)acc[0]));
  }
}

}  // namespace sf
