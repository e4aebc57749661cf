// siren_mask.hip — the RigL topology update on the device, no host synchronisation (sf_mask_update); below
// it the SNFS update (sf_mask_update_snfs) and the global-magnitude update (sf_mask_prune_global), each under its own header.
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
// those ties by index (each wave owns a contiguous segment, mask_seg: a ballot prefix inside a 64-element step, a running count
// along the segment, a scan over the waves) and only when the boundary splits a group of ties.  Growth is the same code on
// the complemented key.  The one key that piles up - |w| = 0 of the dead weights, c = 0 of the live ones - is counted in
// registers and kept out of the histogram.  Every count is an integer (LDS integer atomics commute): the result does not
// depend on the order in which waves arrive.  Every loop runs a trip count derived from n and the wave index, so every
// barrier is reached by every thread of the workgroup.
// A device helper that holds a barrier or a wave-wide ballot is left early only on a condition that is uniform over the
// workgroup (the wave), and says so.
// (included by siren_fit.hip; the three entry points are in mask_host.hip)

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

// step 2 of the contract: the rate of a layer of n elements, `dead` of them masked out, one of L, that holds `share` of
// the statistic (sf_mask_update, sf_mask_prune_global: of the non-zeros; sf_mask_update_snfs: of its redistribution statistic)
__device__ __forceinline__ double mask_rate(double share, long long dead, int n, int L, double r) {
  const double frac_dead = (double)dead / (double)n;
  const bool capped = frac_dead < 0.2 && (1.0 / (double)L) / share < 1.0;
  return capped ? fmin(frac_dead, r) : r;
}
__device__ __forceinline__ double mask_rate(const MaskRow* rows, int j, int n, int L, long long S, double r) {
  return mask_rate((double)rows[j].nnz_before / (double)S, rows[j].dead_before, n, L, r);
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

// Adam's momentum of one weight as Masking.get_momentum_for_weight forms it, m / (sqrt(v) + 1e-8): three IEEE fp32
// operations, each rounded to nearest.  Written as operators under `fp contract(off)` and with sqrtf, not as the _rn
// intrinsics: the toolchain's __fsqrt_rn is the approximate hardware square root (one ulp), and its _rn arithmetic forms are
// plain operators that the translation unit's default contraction may fuse with a neighbour.
__device__ __forceinline__ float mask_momentum(float m, float v) {
#pragma clang fp contract(off)
  const float root = sqrtf(v);
  const float den = root + 1e-8f;
  return m / den;
}

// The key sources of the selection helpers below: key(i) of element i, smallest first.  kHeavy: the one key that piles up
// (it is counted in registers, not in the histogram) - the smallest possible key when pruning, the largest when growing.
struct KeyAbsW {                  // prune: the bits of |w|
  const float* w;
  static constexpr unsigned kHeavy = 0u;
  static constexpr bool kGrow = false;
  __device__ __forceinline__ unsigned key(int i) const { return mask_key<false>(w[i], 0.0f); }
};
struct KeyGrad {                  // grow by |gradient|: the complement of the bits of |g| * (1 - k)
  const float *g, *k;
  static constexpr unsigned kHeavy = 0xffffffffu;
  static constexpr bool kGrow = true;
  __device__ __forceinline__ unsigned key(int i) const { return mask_key<true>(g[i], k[i]); }
};
struct KeyMom {                   // grow by |momentum|: the complement of the bits of |mom * (1 - k)|, mom from m and v on the fly
  const float *m, *v, *k;
  static constexpr unsigned kHeavy = 0xffffffffu;
  static constexpr bool kGrow = true;
  __device__ __forceinline__ unsigned key(int i) const {
    return ~(__float_as_uint(__fmul_rn(mask_momentum(m[i], v[i]), __fsub_rn(1.0f, k[i]))) & 0x7fffffffu);
  }
};

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

// The K-th smallest key of n (1 <= K <= n) and the number of its ties inside the selection -> s.sel.  src: the key source
// (KeyAbsW, KeyGrad, KeyMom).
template <class Src>
__device__ void mask_select(const Src& src, int n, int K, MaskLds& s) {
  constexpr unsigned H = Src::kHeavy;
  constexpr bool GROW = Src::kGrow;
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
        const unsigned key = in ? src.key(i) : H;
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
template <class Src>
__device__ int mask_tie_base(const Src& src, int n, int seg, MaskLds& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const MaskSel sel = s.sel;
  if (sel.take >= sel.ties) return 0;                         // (uniform: every tie is selected, no rank is needed)
  int cnt = 0;
  const int end = min(n, (wave + 1) * seg);
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    cnt += __popcll(__ballot(i < end && src.key(i) == sel.T));
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

// every wave owns the contiguous segment [wave * seg, (wave + 1) * seg) of a layer of n elements, seg a multiple of 64
__device__ __forceinline__ int mask_seg(int n) { return ((n + kMaskWaves - 1) / kMaskWaves + 63) / 64 * 64; }

// steps 3 and 4 of the contract for the layer p, live0 of its elements live and dead0 masked out: -> removed.  The caller
// zeroed s.acc[3] behind a barrier.  (Left early only on the rate: uniform over the workgroup.)
__device__ int mask_prune(const MaskLayer& p, long long live0, long long dead0, double rate, int seg, MaskLds& s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = p.n;
  const double dropd = ceil(rate * (double)live0);
  if (!(dropd > 0.0)) return 0;
  const int end = min(n, (wave + 1) * seg);
  const int K = (int)fmin((double)dead0 + dropd, (double)n);
  const KeyAbsW src{p.w};
  mask_select(src, n, K, s);
  int run = mask_tie_base(src, n, seg, s), gone = 0;
  const MaskSel sel = s.sel;
  const bool all = sel.take >= sel.ties;
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    const bool in = i < end;
    const bool pick = mask_pick(in ? src.key(i) : 0xffffffffu, in, sel, all, run, lane);
    const bool was_live = pick && p.k[i] == 1.0f;
    if (pick) p.k[i] = 0.0f;
    gone += __popcll(__ballot(was_live));
  }
  if (lane == 0 && gone) atomicAdd(&s.acc[3], gone);
  __syncthreads();                                            // (the new k of every wave is visible to the growth that follows)
  return s.acc[3];
}

// bits of |mom_i| of the SNFS statistic (sf_mask_update_snfs, below)
__device__ __forceinline__ unsigned snfs_abs_mom(float m, float v) { return __float_as_uint(mask_momentum(m, v)) & 0x7fffffffu; }

// Step 5 (budget > 0: the `budget` elements smallest in src's key get k = 1, and w = +0.0 where zero_grown), step 6 and the
// counts of step 7 -> s.acc[0 .. 2], which the caller zeroed behind a barrier and reads behind one.  seen(i): what the caller
// wants of element i once its state is final (k_mask_update: nothing).  (budget: uniform over the workgroup.)
template <class Src, class Seen>
__device__ void mask_grow_apply(const MaskLayer& p, const Src& src, int budget, bool zero_grown, bool sparse_grads, int seg,
                                MaskLds& s, Seen seen) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = p.n;
  const int end = min(n, (wave + 1) * seg);
  const bool grow = budget > 0;
  int run = 0;
  if (grow) {
    mask_select(src, n, min(budget, n), s);
    run = mask_tie_base(src, n, seg, s);
  }
  const MaskSel sel = s.sel;
  const bool all = sel.take >= sel.ties;
  MaskTally c{};
  for (int base = wave * seg; base < end; base += 64) {
    const int i = base + lane;
    const bool in = i < end;
    float kv = in ? p.k[i] : -1.0f, wv = in ? p.w[i] : 0.0f;
    const float gv = in ? p.g[i] : 0.0f;
    // (grow is uniform over the workgroup: every lane of the wave reaches the pick's ballot or none does)
    if (grow && mask_pick(in ? src.key(i) : 0xffffffffu, in, sel, all, run, lane)) {
      kv = 1.0f;
      if (zero_grown) wv = 0.0f;
      p.k[i] = 1.0f;
    }
    if (in) {
      mask_apply(p, i, wv, gv, kv, sparse_grads, c);
      seen(i);
    }
  }
  c.commit(s.acc, lane);
}

// steps 2 - 7 of the contract for layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_mask_update(MaskArgs a) {
  __shared__ MaskLds s;
  const int j = blockIdx.x, t = threadIdx.x;
  const MaskLayer p = mask_layer(a, j);
  const int n = p.n;
  long long S = 0;
  for (int l = 0; l < a.L; ++l) S += a.rows[l].nnz_before;
  if (S == 0) {                                               // (uniform over the grid: nothing is touched)
    if (j == 0 && t == 0) a.rows[a.L].live_before = 1;
    return;
  }
  const double rate = mask_rate(a.rows, j, n, a.L, S, a.rate);
  const int seg = mask_seg(n);
  if (t < 4) s.acc[t] = 0;
  __syncthreads();
  const int removed = mask_prune(p, a.rows[j].live_before, a.rows[j].dead_before, rate, seg, s);      // 3., 4.
  // 5. (growth 1, removed > 0: not every k of the layer is 1), 6. and the counts of 7.
  mask_grow_apply(p, KeyGrad{p.g, p.k}, a.growth == 1 ? removed : 0, true, a.dense == 0, seg, s, [](int) {});
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
// sf_mask_update_snfs — the update of masking=SNFS on the device (magnitude pruning, growth by |momentum| or |gradient|, the
// regrowth redistributed by the mean |momentum| of the live weights), no host synchronisation.
//
// Reference being replaced: core.py:713-801 truncate_weights with core.py:425-464 gather_statistics,
// funcs/redistribute.py:18-37 momentum_redistribution, core.py:299-360 calc_redistributed_densities, funcs/grow.py:25-55
// momentum_growth, core.py:474-493 get_momentum_for_weight.  Three launches whatever the depth and however many rounds the
// water-filling takes, one workgroup per masked layer.
//
// The contract (counts exact integers; every double operation IEEE round to nearest, none contracted; mom_i =
// m_i / (sqrt(v_i) + 1e-8f) as three fp32 operations rounded to nearest, mask_momentum above):
//   1. live_j, dead_j, nnz_j as step 1 of sf_mask_update                                                      (k_snfs_stat)
//   2. statistic 0: stat_j = (double)nnz_j.  statistic 1, a_i = |mom_i|: amax_j = the largest a_i over EVERY element of the
//      layer (an integer max on the bits); a non-finite a_i or live_j == 0 -> status 3.  e: amax_j < 2^e (frexp; of 1.0 when
//      amax_j == 0), ln the least with n + 1 <= 2^ln, s = 60 - ln - e; A_j = sum over k_i == 1 of llrint((double)a_i * 2^s), a
//      64-bit integer sum (it cannot overflow: every term is at most 2^(60 - ln), there are fewer than 2^ln);
//      stat_j = ((double)A_j * 2^-s) / (double)live_j.  An integer sum: any order gives the same bits
//      norm = sum of stat_j in layer order from 0.0; status 3 if any layer asked for it, else status 1 if norm == 0: the
//      state is untouched.  share_j = stat_j / norm                                                          (k_snfs_prune)
//   3. rate_j: step 2 of sf_mask_update with share_j; drop_j = ceil(rate_j * live_j); the prune of step 4 there -> removed_j
//   4. statistic 0: budget_j = removed_j.  statistic 1 (calc_redistributed_densities): R = sum removed_j,
//      pool = (double)R + adjusted_growth, cap_j = 0.99 * (double)(dead_j + removed_j), budget_j = rint(share_j * pool) (half to
//      even), share = 0; at most 1000 rounds of { excess = 0; for j ascending: want = budget_j + share; if want > cap_j:
//      excess += want - cap_j, want = cap_j; budget_j = want; then share = excess / (double)L; stop unless excess > 0 }.
//      grown_j = (int)budget_j, truncated.  Thread 0 of EVERY workgroup of k_snfs_grow runs these doubles from the same rows:
//      the same operations in the same order, so the same bits                                                (k_snfs_grow)
//   5. grown_j > 0.  growth 2: c_i = |mom_i * (1 - k_i)| (an fp32 product, k after the prune), the grown_j elements largest
//      in c_i, ties to the lower index, get k_i = 1; w_i is NOT written (a weight pruned in 3 and grown here keeps its
//      value).  growth 1: step 5 of sf_mask_update with grown_j in place of removed (w_i = +0.0)
//   6. step 6 of sf_mask_update
//   7. row j (SnfsRow, 12 words): the eight words of sf_mask_update's row; stat_j; budget_j, the double before truncation;
//      grown_j; stat_after_j = step 2 over the state steps 5 and 6 left (statistic 1: NaN when no weight is live)
//      status row: [0] status (0, 1, 3) [1] rounds [2] R [3] sum grown_j [7] pool [8] norm [11] the norm after: the sum of
//      the stat_after_j that are not NaN, in layer order; every other word 0.  Status 1 or 3: rows j hold the counts before,
//      copied to the counts after, and zeros; the status row its status and zeros.
// The norm after needs every layer's row: the workgroup that finishes last (an arrival count in word [6] of the status row,
// device-scope atomics and fences, put back to 0) sums them.  No float is ever added atomically.

constexpr unsigned kMaskInf = 0x7f800000u;

struct SnfsRow {                  // sf_mask_snfs_stats (include/siren_fit.h); row [n_layers] is the status row
  long long live_before, dead_before, nnz_before, removed, live_after, dead_after, nnz_after;
  double prune_rate, stat_before, budget;
  long long grown;                // (between k_snfs_stat and k_snfs_grow: 1 where the layer asks for status 3)
  double stat_after;
};

struct SnfsArgs {
  MaskArgs m;                     // w, g, m, v, k, off, n, L, rate, growth, dense (rows unused)
  SnfsRow* rows;
  double adjusted_growth;
  int statistic;
};

struct SnfsLds {
  unsigned amax;                  // bits of the largest |mom| of the layer
  unsigned long long A;           // the fixed-point sum
  double budget[kMaskMaxLayers], cap[kMaskMaxLayers];
  int grown[kMaskMaxLayers];
};

// the wave's largest value -> LDS (an integer max: any order gives the same word); every lane of the wave calls it
__device__ __forceinline__ void snfs_commit_max(unsigned amax, unsigned* dst, int lane) {
  for (int d = 32; d > 0; d >>= 1) amax = max(amax, (unsigned)__shfl_down((int)amax, d));
  if (lane == 0 && amax) atomicMax(dst, amax);
}

// Step 2's statistic of the layer p whose largest |mom| has the bits amax (finite) and that has live > 0 live weights.
// Every thread of the workgroup calls it (barriers); q.A was zeroed behind a barrier.
__device__ double snfs_stat(const MaskLayer& p, unsigned amax, long long live, SnfsLds& q) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, lane = t & 63;
  const float top = __uint_as_float(amax);
  int e = 0, ln = 0;
  frexpf(top > 0.f ? top : 1.f, &e);                             // top < 2^e
  while ((1L << ln) < (long)p.n + 1) ++ln;                       // n < 2^ln
  const int sh = 60 - ln - e;
  const double scale = ldexp(1.0, sh);
  long long sum = 0;
  for (int i = t; i < p.n; i += kMaskThreads) {
    if (p.k[i] != 1.0f) continue;
    const double a = (double)__uint_as_float(snfs_abs_mom(p.m[i], p.v[i]));
    sum += __double2ll_rn(a * scale);                            // (a power of two: the product is exact)
  }
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  if (lane == 0 && sum) atomicAdd(&q.A, (unsigned long long)sum);
  __syncthreads();
  const double total = (double)(long long)q.A;
  const double unscaled = total * ldexp(1.0, -sh);
  return unscaled / (double)live;
}

// steps 1 and 2 (the statistic) for layer blockIdx.x -> its row; the status row cleared
__global__ __launch_bounds__(kMaskThreads) void k_snfs_stat(SnfsArgs a) {
  __shared__ SnfsLds q;
  __shared__ int acc[3];
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const MaskLayer p = mask_layer(a.m, j);
  const bool stat = a.statistic == 1;
  if (t < 3) acc[t] = 0;
  if (t == 0) { q.amax = 0; q.A = 0; }
  __syncthreads();
  MaskTally c{};
  unsigned amax = 0;
  for (int i = t; i < p.n; i += kMaskThreads) {
    c.add(p.w[i], p.k[i]);
    if (stat) amax = max(amax, snfs_abs_mom(p.m[i], p.v[i]));
  }
  c.commit(acc, lane);
  snfs_commit_max(amax, &q.amax, lane);
  __syncthreads();
  const long long live = acc[0];
  const bool bad = stat && (q.amax >= kMaskInf || live == 0);
  double value = (double)acc[2];
  if (stat && !bad) value = snfs_stat(p, q.amax, live, q);      // (uniform over the workgroup)
  if (t == 0) {
    SnfsRow r{};
    r.live_before = r.live_after = live;
    r.dead_before = r.dead_after = acc[1];
    r.nnz_before = r.nnz_after = acc[2];
    r.stat_before = bad ? 0.0 : value;
    r.grown = bad;
    a.rows[j] = r;
    if (j == 0) a.rows[a.m.L] = SnfsRow{};
  }
}

// the norm and the status of step 2, the shares, step 3 for layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_snfs_prune(SnfsArgs a) {
  __shared__ MaskLds s;
  const int j = blockIdx.x, t = threadIdx.x, L = a.m.L;
  const MaskLayer p = mask_layer(a.m, j);
  SnfsRow* rows = a.rows;
  bool bad = false;
  double norm = 0.0;
  {
#pragma clang fp contract(off)
    for (int l = 0; l < L; ++l) {
      bad |= rows[l].grown != 0;
      norm = norm + rows[l].stat_before;
    }
  }
  const int status = bad ? 3 : norm == 0.0 ? 1 : 0;
  if (status) {                                               // (uniform over the grid: nothing is touched)
    if (j == 0 && t == 0) rows[L].live_before = status;
    return;
  }
  const double share = rows[j].stat_before / norm;
  const double rate = mask_rate(share, rows[j].dead_before, p.n, L, a.m.rate);
  if (t < 4) s.acc[t] = 0;
  __syncthreads();
  const int removed = mask_prune(p, rows[j].live_before, rows[j].dead_before, rate, mask_seg(p.n), s);
  if (t == 0) {                                               // (fields no other workgroup of this kernel reads)
    rows[j].removed = removed;
    rows[j].prune_rate = rate;
    if (j == 0) rows[L].stat_before = norm;
  }
}

// step 4 (thread 0): the budgets of all L layers from the rows -> q.budget, q.grown; block 0 also fills the status row
__device__ void snfs_budgets(const SnfsArgs& a, SnfsLds& q, bool report) {
#pragma clang fp contract(off)
  const int L = a.m.L;
  SnfsRow* rows = a.rows;
  long long R = 0, total = 0;
  for (int l = 0; l < L; ++l) R += rows[l].removed;
  const double pool = (double)R + a.adjusted_growth;
  int rounds = 0;
  if (a.statistic == 0) {
    for (int l = 0; l < L; ++l) q.budget[l] = (double)rows[l].removed;
  } else {
    const double norm = rows[L].stat_before;
    for (int l = 0; l < L; ++l) {
      const double share_l = rows[l].stat_before / norm;
      const double asked = share_l * pool;
      q.budget[l] = rint(asked);
      q.cap[l] = 0.99 * (double)(rows[l].dead_before + rows[l].removed);
    }
    double share = 0.0;
    while (rounds < 1000) {
      double excess = 0.0;
      for (int l = 0; l < L; ++l) {
        double want = q.budget[l] + share;
        const double c = q.cap[l];
        if (want > c) {
          const double over = want - c;
          excess = excess + over;
          want = c;
        }
        q.budget[l] = want;
      }
      share = excess / (double)L;
      ++rounds;
      if (!(excess > 0.0)) break;
    }
  }
  for (int l = 0; l < L; ++l) {
    q.grown[l] = (int)q.budget[l];
    total += q.grown[l];
  }
  if (report) {
    SnfsRow& z = rows[L];
    z.dead_before = rounds;
    z.nnz_before = R;
    z.removed = total;
    z.prune_rate = pool;
  }
}

// steps 4 - 7 for layer blockIdx.x
__global__ __launch_bounds__(kMaskThreads) void k_snfs_grow(SnfsArgs a) {
  __shared__ MaskLds s;
  __shared__ SnfsLds q;
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63, L = a.m.L;
  const MaskLayer p = mask_layer(a.m, j);
  SnfsRow* rows = a.rows;
  if (rows[L].live_before != 0) {                             // (status 1 or 3, uniform over the grid: nothing is touched)
    if (t == 0) { rows[j].stat_before = 0.0; rows[j].grown = 0; }
    return;
  }
  const bool stat = a.statistic == 1;
  if (t < 4) s.acc[t] = 0;
  if (t == 0) {
    q.amax = 0; q.A = 0;
    snfs_budgets(a, q, j == 0);
  }
  __syncthreads();
  const int grown = q.grown[j], seg = mask_seg(p.n);
  const bool sparse_grads = a.m.dense == 0;
  unsigned amax = 0;                                          // the lane's largest |mom| bits over the state the pass leaves
  auto seen = [&](int i) { if (stat) amax = max(amax, snfs_abs_mom(p.m[i], p.v[i])); };
  if (a.m.growth == 2) mask_grow_apply(p, KeyMom{p.m, p.v, p.k}, grown, false, sparse_grads, seg, s, seen);
  else mask_grow_apply(p, KeyGrad{p.g, p.k}, grown, true, sparse_grads, seg, s, seen);
  snfs_commit_max(amax, &q.amax, lane);
  __syncthreads();                                            // (the counts, the largest |mom|, the state every wave left)
  const long long live = s.acc[0];
  double after = (double)s.acc[2];
  if (stat) after = live == 0 ? __longlong_as_double(0x7ff8000000000000ll) : snfs_stat(p, q.amax, live, q);      // (uniform)
  if (t == 0) {
    SnfsRow& r = rows[j];
    r.live_after = live;
    r.dead_after = s.acc[1];
    r.nnz_after = s.acc[2];
    r.budget = q.budget[j];
    r.grown = grown;
    using u64 = unsigned long long;
    __hip_atomic_store(reinterpret_cast<u64*>(&r.stat_after), (u64)__double_as_longlong(after), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the norm after: the workgroup that arrives last sums every layer's stat_after in layer order
    __threadfence();
    u64* arrived = reinterpret_cast<u64*>(&rows[L].nnz_after);
    if (atomicAdd(arrived, (u64)1) == (u64)(L - 1)) {
#pragma clang fp contract(off)
      __threadfence();
      double norm = 0.0;
      for (int l = 0; l < L; ++l) {
        const double v = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<u64*>(&rows[l].stat_after), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (v == v) norm = norm + v;
      }
      rows[L].stat_after = norm;
      __hip_atomic_store(arrived, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
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
    const unsigned key = mask_key<false>(p.w[i], 0.0f);
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
