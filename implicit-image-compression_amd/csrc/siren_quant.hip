// siren_quant.hip — the quantise phase of a fit on the device (sf_quant_pass / sf_quant_nudge / sf_quant_step, quant_host.hip).
//
// Reference being replaced (paths relative to the reference tree):
//   implicit_image/pipeline/quant/kmeans.py:66-72,110-150  the forward-pre-hook of every quantised Linear: find_centroids from a
//                                                          linspace(min, max, 2^bits - 1) guess, the codebook weights written back
//   implicit_image/pipeline/quant/kmeans.py:163-181        the backward hook: centroids -= lr * scatter_add(labels, dL/dW)
// The k-means itself is siren_kmeans.hip's, through the same device functions (km_init / km_assign / km_update / km_finish /
// km_predict): the same arithmetic, so a layer gets the bits sf_kmeans_fit gives it.  What is new here is the batching: ONE
// launch serves every quantised layer (blockIdx.y, or blockIdx.x where a layer is one workgroup) from a layer table in the
// kernel arguments, every layer with its own workspace row, and the guess and the nudge, which were torch ops with two host
// reads per layer.  A pass is 3 + 2 * iter_limit launches whatever the depth, the nudge is one.
// (included by siren_fit.hip)

namespace sf {

constexpr int kKmqMaxLayers = 16;    // (the layers of a handle: sf_engine::off_w)
constexpr int kKmqThreads = 512;     // one workgroup per layer where a layer is one workgroup (= kKmMaxK: km_update, km_finish)

struct KmqLayer {
  long off;                 // the layer's weights in the flat params / grads
  int n;
  float* centers;           // [K] the guess, then the Lloyd centres
  float* cent;              // [K + 1] centroids, zero padded
  int* n_cent;              // may be null
  long long* labels;        // [n]
};
struct KmqArgs {
  KmqLayer l[kKmqMaxLayers];
  int L, K;
  float tol, lr;
  float* params;
  const float* grads;
  KmWs* ws;                 // [L] one row per layer: a layer's done / empty flag is its own
};

// The guess of every layer and k_km_init's work.  min / max over the layer's non-zero weights (+inf / -inf without one), then
// torch.linspace(min, max, K) as ATen's device kernel forms it in fp32: step = (end - start) / (K - 1), entry i is
// start + step * i below K / 2 and end - step * (K - 1 - i) from there on, each one fused multiply-add.  Without a non-zero
// weight both ends come out non-finite and km_init marks the layer's call empty.
__global__ __launch_bounds__(kKmqThreads) void k_kmq_guess(KmqArgs a) {
  const KmqLayer& y = a.l[blockIdx.x];
  const float* w = a.params + y.off;
  __shared__ float smin[kKmqThreads], smax[kKmqThreads];
  const int t = threadIdx.x;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = t; i < y.n; i += kKmqThreads) {
    const float x = w[i];
    if (x != 0.0f) { mn = fminf(mn, x); mx = fmaxf(mx, x); }
  }
  smin[t] = mn; smax[t] = mx;
  __syncthreads();
  for (int s = kKmqThreads / 2; s > 0; s >>= 1) {
    if (t < s) { smin[t] = fminf(smin[t], smin[t + s]); smax[t] = fmaxf(smax[t], smax[t + s]); }
    __syncthreads();
  }
  const float start = smin[0], end = smax[0];
  const float step = __fdiv_rn(__fsub_rn(end, start), (float)(a.K - 1));
  for (int i = t; i < a.K; i += kKmqThreads)
    y.centers[i] = i < a.K / 2 ? __fmaf_rn(step, (float)i, start) : __fmaf_rn(-step, (float)(a.K - 1 - i), end);
  __syncthreads();          // (km_init reads centers[0] and centers[K - 1] back: the workgroup's own stores)
  km_init(y.centers, a.K, y.n, a.ws + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_kmq_assign(KmqArgs a) {
  const KmqLayer& y = a.l[blockIdx.y];
  if ((long)blockIdx.x * 256 >= y.n) return;                       // (a smaller layer than the grid was sized for)
  km_assign(a.params + y.off, y.n, y.centers, a.K, a.ws + blockIdx.y, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kKmqThreads) void k_kmq_update(KmqArgs a) {
  km_update(a.l[blockIdx.x].centers, a.K, a.ws + blockIdx.x, a.tol);
}

__global__ __launch_bounds__(kKmqThreads) void k_kmq_finish(KmqArgs a) {
  const KmqLayer& y = a.l[blockIdx.x];
  km_finish(y.centers, a.K, a.ws + blockIdx.x, y.cent, a.K + 1, y.n_cent);
}

// labels of all weights of every layer, the codebook weights straight into the flat parameters
__global__ __launch_bounds__(256) void k_kmq_predict(KmqArgs a) {
  const KmqLayer& y = a.l[blockIdx.y];
  if ((long)blockIdx.x * 256 >= y.n) return;
  float* w = a.params + y.off;
  km_predict(w, y.n, y.cent, a.ws + blockIdx.y, y.labels, w, blockIdx.x, gridDim.x);
}

// centroids[k] -= lr * sum of dL/dW over the weights labelled k, one workgroup per layer.  The segment sums are 64-bit
// fixed-point integer adds (they commute: the result does not depend on the order of arrival, unlike the float atomics of
// scatter_add_), in the unit 2^(60 - ln - e) with n < 2^ln and max|g| < 2^e - the way km_init sizes its unit, the maximum
// from an integer max over the bits of |g|.  A sum is rounded once to float; then c - lr * dw in fp32, two roundings.
__global__ __launch_bounds__(kKmqThreads) void k_kmq_nudge(KmqArgs a) {
  const KmqLayer& y = a.l[blockIdx.x];
  const float* g = a.grads + y.off;
  __shared__ unsigned long long ssum[kKmMaxK];
  __shared__ unsigned gmax;
  const int t = threadIdx.x, C = a.K + 1;
  for (int i = t; i < kKmMaxK; i += kKmqThreads) ssum[i] = 0ull;
  if (t == 0) gmax = 0u;
  __syncthreads();
  unsigned m = 0u;
  for (int i = t; i < y.n; i += kKmqThreads) m = max(m, __float_as_uint(g[i]) & 0x7fffffffu);   // (bits of |g| order as |g| does)
  atomicMax(&gmax, m);
  __syncthreads();
  const float gm = __uint_as_float(gmax);
  int e = 0;
  frexpf(gm > 0.f && gm < __builtin_inff() ? gm : 1.f, &e);       // gm < 2^e
  int ln = 0;
  while ((1L << ln) < (long)y.n + 1) ++ln;                         // n < 2^ln
  const double scale = ldexp(1.0, 60 - ln - e), inv_scale = ldexp(1.0, -(60 - ln - e));
  for (int i = t; i < y.n; i += kKmqThreads) {
    const long long k = y.labels[i];
    if (k < 0 || k >= C) continue;                                 // (never with labels k_kmq_predict wrote)
    atomicAdd(&ssum[k], (unsigned long long)(long long)llrint((double)g[i] * scale));
  }
  __syncthreads();
  for (int k = t; k < C; k += kKmqThreads) {
#pragma clang fp contract(off)                                     // (two roundings, as the host path's two torch ops: never one fma)
    const float dw = (float)((double)(long long)ssum[k] * inv_scale);
    const float step = a.lr * dw;
    y.cent[k] = y.cent[k] - step;
  }
}

}  // namespace sf
