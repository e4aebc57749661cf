// feather_kernels.hip — gfx950 kernels of Feathermap (structured multi-hashing) on top of the SIREN engine.
//
// Reference arithmetic being replaced (paths relative to the reference tree):
//   implicit_image/pipeline/feathermap/feathernet.py:260-274   V = V1 @ V2, W_k = scaler_k * V.view(-1)[seg_k]
//   autograd of the above                                      dV1 = G V2^T, dV2 = V1^T G, dscaler_k = sum_seg dL/dW * V
//   torch.optim.Adam over named_parameters()                   k_adam of siren_kernels.hip on [V1 | V2 | scalers]
//
// V is n x n (row-major); its first P entries, in the reference's named_modules order, are the P logical weights and
// biases of the SIREN, the n^2 - P tail is unused.  Segment k of V.view(-1) is one weight or bias tensor; its logical
// element j sits at engine flat index base_k + (j / cols_k) * stride_k + j % cols_k, so a zero-padded engine width
// (hidden 96 -> 128) maps each logical row onto a strided engine row and the padded slots are never written.
//
// Every product is fp32 in, fp32 accumulated, in a fixed order (no atomics): 64 x 64 output tiles on the VALU, 16-deep
// k slices staged in LDS, each output summed over k in ascending order by one thread.  The scalar gradients are summed
// in fixed 64 Ki-element chunks (k_fth_grad) whose partials are added in chunk order (last block of k_fth_dv).
//
//   k_fth_mat    V = V1 V2 (rows that hold logical entries only); writes V[0, P) and W = scaler * V into the engine;
//                its RENDER form (sf_feather_render_load) writes W alone: the unscaled V is the adjoint's operand only
//   k_fth_grad   G = scaler * dL/dW mapped onto V's layout (the tail stays 0), plus per-chunk partials of dscaler
//   k_fth_dv     dV1 = G V2^T and dV2 = V1^T G into the feather gradient; one extra block reduces the partials
// (included by siren_fit.hip after siren_kernels.hip: DEV, k_adam)

namespace sf {

constexpr int kFthMaxSeg = 32;        // 2 x 16 layers
constexpr int kFthTile = 64;          // output tile edge
constexpr int kFthKT = 16;            // k slice staged in LDS
constexpr int kFthPitch = kFthTile + 4;
constexpr long kFthChunk = 65536;     // elements per scalar-gradient partial

struct FthSeg {
  int nseg;
  long start[kFthMaxSeg + 1];   // logical start of each segment in V.view(-1); start[nseg] = P
  long base[kFthMaxSeg];        // engine flat offset of the segment's first element
  int cols[kFthMaxSeg];         // logical row length (in_features of a weight, out_features of a bias)
  int stride[kFthMaxSeg];       // engine row stride
};

struct FthArgs {
  FthSeg seg;
  int n, m;
  long P;
  int rows_used;                // ceil(P / n): rows of V that hold logical entries
  const float* fp;              // feather parameters [V1 n*m | V2 m*n | scalers nseg]
  float* fg;                    // feather gradient, same layout
  float* V;                     // [P] unscaled V of the last materialisation (never touched by k_fth_mat<true>)
  float* G;                     // [n*n] scaler * dL/dW on V's layout (tail zero)
  float* W;                     // engine flat parameters
  const float* dW;              // engine flat gradient
  const long* chunks;           // [nchunks][3]: segment, first, end (logical indices)
  const int* seg_chunk0;        // [nseg + 1]: first chunk of each segment
  float* part;                  // [nchunks]
  int nchunks;
  int g_blocks;                 // k_fth_grad: blocks that form G (the rest sum the chunks)
  int t1, t1n;                  // k_fth_dv: dV1 tiles (t1n along the columns); the dV2 tiles follow
  int t2n;                      // dV2 tiles along the columns
};

struct FthSegLds {
  long start[kFthMaxSeg + 1];
  long base[kFthMaxSeg];
  int cols[kFthMaxSeg], stride[kFthMaxSeg];
  float scal[kFthMaxSeg];
};

DEV void fth_seg_load(FthSegLds& s, const FthArgs& a) {
  const int t = threadIdx.x;
  if (t <= a.seg.nseg) s.start[t] = a.seg.start[t];
  if (t < a.seg.nseg) {
    s.base[t] = a.seg.base[t]; s.cols[t] = a.seg.cols[t]; s.stride[t] = a.seg.stride[t];
    s.scal[t] = a.fp[2L * a.n * a.m + t];
  }
  __syncthreads();
}

// segment of logical index i < P (binary search over the segment starts)
DEV int fth_seg_of(const FthSegLds& s, int nseg, long i) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s.start[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

DEV long fth_engine_index(const FthSegLds& s, int k, long i) {
  const long j = i - s.start[k];
  const long r = j / s.cols[k];
  return s.base[k] + r * s.stride[k] + (j - r * s.cols[k]);
}

// C[64 x 64] tile (tm, tn) of A[M x K] B[K x N]; A(r, k) = A[r*sar + k*sak], B(k, c) = B[k*sbk + c*sbc].
// Thread (ty, tx) = (tid / 16, tid % 16) owns rows 4ty..4ty+3 and columns 4tx..4tx+3 of the tile; acc is summed over k
// in ascending order.
DEV void fth_tile(const float* A, long sar, long sak, const float* B, long sbk, long sbc, int M, int N, int K, int tm,
                  int tn, float (&acc)[4][4], float* As, float* Bs) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int r0 = tm * kFthTile, c0 = tn * kFthTile;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < K; k0 += kFthKT) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int e = tid + 256 * t;
      int rr, kk, cc, kb;
      if (sak == 1) { kk = e & 15; rr = e >> 4; } else { rr = e & 63; kk = e >> 6; }
      if (sbc == 1) { cc = e & 63; kb = e >> 6; } else { kb = e & 15; cc = e >> 4; }
      const int r = r0 + rr, ka = k0 + kk, c = c0 + cc, kbb = k0 + kb;
      As[kk * kFthPitch + rr] = (r < M && ka < K) ? A[(long)r * sar + (long)ka * sak] : 0.f;
      Bs[kb * kFthPitch + cc] = (c < N && kbb < K) ? B[(long)kbb * sbk + (long)c * sbc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kFthKT; ++kk) {
      const float4 av = *reinterpret_cast<const float4*>(&As[kk * kFthPitch + 4 * ty]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[kk * kFthPitch + 4 * tx]);
      const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
    }
    __syncthreads();
  }
}

// grid: (ceil(rows_used / 64), ceil(n / 64)), 256 threads.  RENDER: the inference form - the same product, mapping and one
// multiply by the scalar, so W is bit-identical; it reads a.fp and a.seg and writes a.W, nothing else of a
template <bool RENDER>
__global__ void __launch_bounds__(256) k_fth_mat(FthArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kFthKT * kFthPitch];
  __shared__ __attribute__((aligned(16))) float Bs[kFthKT * kFthPitch];
  __shared__ FthSegLds s;
  fth_seg_load(s, a);
  const int n = a.n, m = a.m;
  float acc[4][4];
  fth_tile(a.fp, m, 1, a.fp + (long)n * m, n, 1, a.rows_used, n, m, blockIdx.x, blockIdx.y, acc, As, Bs);
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = blockIdx.x * kFthTile + 4 * ty + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = blockIdx.y * kFthTile + 4 * tx + j;
      const long e = (long)r * n + c;
      if (r < n && c < n && e < a.P) {
        const int k = fth_seg_of(s, a.seg.nseg, e);
        if constexpr (!RENDER) a.V[e] = acc[i][j];
        a.W[fth_engine_index(s, k, e)] = s.scal[k] * acc[i][j];
      }
    }
  }
}

// blocks [0, g_blocks): G; blocks [g_blocks, g_blocks + nchunks): one dscaler partial each.  256 threads.
__global__ void __launch_bounds__(256) k_fth_grad(FthArgs a) {
  __shared__ FthSegLds s;
  __shared__ float red[256];
  fth_seg_load(s, a);
  const int b = blockIdx.x;
  if (b < a.g_blocks) {
    for (long e = (long)b * 256 + threadIdx.x; e < a.P; e += (long)a.g_blocks * 256) {
      const int k = fth_seg_of(s, a.seg.nseg, e);
      a.G[e] = s.scal[k] * a.dW[fth_engine_index(s, k, e)];
    }
    return;
  }
  const long* ch = a.chunks + 3L * (b - a.g_blocks);
  const int k = (int)ch[0];
  float sum = 0.f;
  for (long e = ch[1] + threadIdx.x; e < ch[2]; e += 256) sum = fmaf(a.dW[fth_engine_index(s, k, e)], a.V[e], sum);
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.part[b - a.g_blocks] = red[0];
}

// blocks [0, t1): dV1 tiles; [t1, t1 + t2): dV2 tiles; the last block: dscaler from the partials.  256 threads.
__global__ void __launch_bounds__(256) k_fth_dv(FthArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kFthKT * kFthPitch];
  __shared__ __attribute__((aligned(16))) float Bs[kFthKT * kFthPitch];
  const int n = a.n, m = a.m;
  const int b = blockIdx.x;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  float acc[4][4];
  if (b < a.t1) {   // dV1[n x m] = G[n x n] V2^T, V2^T(c, j) = V2[j * n + c]
    const int tm = b / a.t1n, tn = b % a.t1n;
    fth_tile(a.G, n, 1, a.fp + (long)n * m, 1, n, n, m, n, tm, tn, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = tm * kFthTile + 4 * ty + i, c = tn * kFthTile + 4 * tx + j;
        if (r < n && c < m) a.fg[(long)r * m + c] = acc[i][j];
      }
    return;
  }
  const int b2 = b - a.t1;
  const int t2 = ((m + kFthTile - 1) / kFthTile) * a.t2n;
  if (b2 < t2) {    // dV2[m x n] = V1^T[m x n] G[n x n], V1^T(j, r) = V1[r * m + j]; rows of G past rows_used are zero
    const int tm = b2 / a.t2n, tn = b2 % a.t2n;
    fth_tile(a.fp, 1, m, a.G, n, 1, m, n, a.rows_used, tm, tn, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = tm * kFthTile + 4 * ty + i, c = tn * kFthTile + 4 * tx + j;
        if (r < m && c < n) a.fg[(long)n * m + (long)r * n + c] = acc[i][j];
      }
    return;
  }
  const int k = threadIdx.x;
  if (k < a.seg.nseg) {
    float sum = 0.f;
    for (int c = a.seg_chunk0[k]; c < a.seg_chunk0[k + 1]; ++c) sum += a.part[c];
    a.fg[2L * n * m + k] = sum;
  }
}

}  // namespace sf
