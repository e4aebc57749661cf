// siren_many.hip — the kernels of a single-chunk training step in scratch format 16 (hidden 32 / 64 / 128, fp16 operands) for B
// fits of one shape in ONE launch each (sf_step_many, many_host.hip).  The pattern is siren_quant.hip's: the arithmetic is the
// single-fit device function (fwd_body, bwd_body, dw0_body, reduce_body, reduce_vec_body, sse_reduce_body, adam_body,
// images_body - siren_kernels.hip), and the kernel here only picks its fit.  The grid is (the single kernel's grid, B); block
// size and dynamic LDS are the single kernel's; blockIdx.x / gridDim.x mean inside the body what they mean in the single
// kernel.  Workgroup (x, y) copies row y of a device table of argument structs into a local struct - the address is uniform
// over the workgroup, so the copy is scalar loads and the struct lives in scalar registers like a kernel argument - and calls
// the body with it.  A fit therefore computes bit for bit what its own launch computes.
// Included by siren_fit.hip after siren_quant.hip.

namespace sf {

template <int WD>
__global__ __launch_bounds__(512) void k_fwd_many(const FwdArgs* __restrict__ table) {
  const FwdArgs a = table[blockIdx.y];
  fwd_body<WD, OpF16, true>(a);
}

template <int WD, bool LAST, bool P0>
__global__ __launch_bounds__((BwdCase<WD, LAST, P0>::threads)) void k_bwd_many(const BwdLayerArgs* __restrict__ table) {
  const BwdLayerArgs a = table[blockIdx.y];
  bwd_body<WD, LAST, P0, OpF16>(a);
}

template <int JW>
__global__ __launch_bounds__(JW * 2) void k_dw0_many(const Dw0Args* __restrict__ table) {
  const Dw0Args a = table[blockIdx.y];
  dw0_body<JW, OpF16>(a);
}

__global__ __launch_bounds__(256) void k_reduce_many(const ReduceArgs* __restrict__ table) {
  const ReduceArgs a = table[blockIdx.y];
  reduce_body(a);
}

// (k_reduce_vec takes its arguments loose; a table needs them as a struct)
struct ReduceVecArgs {
  const float* slab;
  int n_wg, n4;
  long stride;
  float* out;
  int accumulate;
  float scale;
  const float* scale_dev;
  const float* scale2_dev;
};
__global__ __launch_bounds__(256) void k_reduce_vec_many(const ReduceVecArgs* __restrict__ table) {
  const ReduceVecArgs a = table[blockIdx.y];
  reduce_vec_body(a.slab, a.n_wg, a.stride, a.n4, a.out, a.accumulate, a.scale, a.scale_dev, a.scale2_dev);
}

// (k_sse_reduce likewise.  loss_tab: this fit's column of the call's loss table, indexed by the call's step counter)
struct SseArgs {
  const float* part;
  int n;
  double* out;
  double* loss_tab;
  const int* iter;
};
__global__ void k_sse_reduce_many(const SseArgs* __restrict__ table) {
  const SseArgs a = table[blockIdx.y];
  sse_reduce_body(a.part, a.n, a.out, a.loss_tab, a.iter);
}

// (a.tab: this fit's {step_size, bc2_sqrt} per step of the call; a.iter: the call's step counter)
__global__ void k_adam_many(const AdamArgs* __restrict__ table) {
  const AdamArgs a = table[blockIdx.y];
  adam_body(a);
}

// (ImgArgs holds the layer offsets as arrays indexed at run time: the body reads them from the table row itself, as k_images
//  reads them from its kernel-argument segment - a local copy of the struct would be indexed in scratch memory)
__global__ void k_images_many(const ImgArgs* __restrict__ table) { images_body(table[blockIdx.y]); }

}  // namespace sf
