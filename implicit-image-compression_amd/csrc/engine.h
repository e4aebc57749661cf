// engine.h — the host core, once: error plumbing, the handle (sf_engine), the launch context and the one kernel launch, chunk
// geometry, device memory, what every creator shares.  Included by siren_fit.hip after the kernel files (one translation unit).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/siren_fit.h"

using namespace sf;

static thread_local std::string g_err;

// sf_config carries the Adam betas as floats; torch.optim.Adam computes 1 - beta and beta^t on the Python double
// (0.9, not 0.89999997615...).  The double meant is recovered as the shortest decimal that rounds to the float.
static double shortest_double(float f) {
  char buf[64];
  for (int digits = 1; digits <= 9; ++digits) {
    snprintf(buf, sizeof(buf), "%.*g", digits, (double)f);
    const double d = strtod(buf, nullptr);
    if ((float)d == f) return d;
  }
  return (double)f;
}
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(SF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)
#define SF_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)
// No exception crosses the C ABI (include/siren_fit.h): every entry point is a function-try-block.  std::bad_alloc becomes
// SF_ERR_NOMEM with a message short enough for the small-string buffer (no allocation on that path), anything else
// SF_ERR_INVALID with the exception's text.
static int fail_nomem() noexcept {
  try { g_err.assign("out of memory"); } catch (...) {}
  return SF_ERR_NOMEM;
}
#define SF_CATCH catch (const std::bad_alloc&) { return fail_nomem(); } \
  catch (const std::exception& e) { try { return fail(SF_ERR_INVALID, std::string("unexpected exception: ") + e.what()); } catch (...) { return fail_nomem(); } } \
  catch (...) { try { return fail(SF_ERR_INVALID, "unexpected exception"); } catch (...) { return fail_nomem(); } }

// an argument struct of a kernel, every member zero
template <typename T>
T zeroed() { T a; memset(&a, 0, sizeof(a)); return a; }

// the kernels take phases in revolutions: omega / 2 pi, formed in double
static constexpr double kTwoPi = 6.283185307179586476925286766559;

// (k_bwd_layer1: the backward of layer 1, whose input phases are re-derived from the coordinates - another kernel form than
//  the hidden layers', so it gets its own line in the per-kernel report)
// (k_feather_*: the Feathermap update of sf_adam_step on a handle with sf_feather_attach, feather_kernels.hip)
enum KernelId { K_FWD = 0, K_BWD_HIDDEN, K_BWD_LAST, K_DW_FIRST, K_REDUCE, K_SSE, K_ADAM, K_IMAGES, K_BWD_L1,
                K_FTH_GRAD, K_FTH_DV, K_FTH_ADAM, K_FTH_MAT, K_WV_COMPOSE, K_WV_ADJOINT, K_WV_INJECT, K_MASK, K_MASK_PRUNE, K_MASK_SNFS,
                K_KMQ_GUESS, K_KMQ_ASSIGN, K_KMQ_UPDATE, K_KMQ_FINISH, K_KMQ_PREDICT, K_KMQ_NUDGE, K_RENDER, K_WV_RENDER, K_FF_RENDER, K_COUNT };
// (k_wv_*: the image-space composition of a WaveletSiren handle and its adjoint, wavelet_kernels.hip)
// (k_mask_update: the two kernels of one sf_mask_update, siren_mask.hip; k_mask_prune_global: the kernels of one
//  sf_mask_prune_global, same file; k_mask_snfs: the three kernels of one sf_mask_update_snfs, same file)
// (k_kmq_*: the batched kernels of the quantise phase, siren_quant.hip - one record per launch, so the profile counts launches)
static const char* kKernelNames[K_COUNT] = {"k_fwd",    "k_bwd_hidden", "k_bwd_last", "k_dw_first",
                                            "k_reduce", "k_sse",        "k_adam",     "k_images", "k_bwd_layer1",
                                            "k_feather_grad", "k_feather_dv", "k_feather_adam", "k_feather_mat",
                                            "k_wv_compose", "k_wv_adjoint", "k_wv_inject", "k_mask_update", "k_mask_prune_global", "k_mask_snfs",
                                            "k_kmq_guess", "k_kmq_assign", "k_kmq_update", "k_kmq_finish", "k_kmq_predict", "k_kmq_nudge",
                                            "k_render", "k_wv_render", "k_ff_render"};

struct ProfRec {
  int id;
  hipEvent_t e0, e1;
};

// Every entry point runs with the handle's device current and restores the caller's device on return: a
// process may drive engines on several GPUs, or change torch.cuda.current_device after sf_create.
struct DevGuard {
  int prev = -1, want = -1;
  explicit DevGuard(int device) : want(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) hipSetDevice(want);
  }
  ~DevGuard() {
    if (prev >= 0 && prev != want) hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

// the network a handle fits, fixed by its creator (`wide`, `render` and an attached Feathermap are flags beside it)
enum class Model { Siren, Fourier, Wavelet };

// Where and how a handle launches: the stream, whether the launches belong to a captured step, the profiler.  Every handle
// owns one; the sub-handles of a WaveletSiren handle use their parent's (wavelet_begin), so its stream - the capturing one
// while a step is captured - is theirs, and their launches are its profile records.
struct LaunchCtx {
  hipStream_t stream = nullptr;
  bool replay = false;      // launches issued now belong to a replayed step: per-step scalars come from device tables
  bool prof = false;
  std::vector<ProfRec> recs;         // launches not yet timed (prof_flush)
  std::vector<hipEvent_t> ev_pool;   // recycled timing events (creating two per launch costs more than a small kernel)
  double ms[K_COUNT] = {0};
  int64_t n[K_COUNT] = {0};
  double flops[K_COUNT] = {0}, bytes[K_COUNT] = {0};
};

struct sf_engine {
  sf_config cfg;
  Model model = Model::Siren;
  int D = 0, WD = 0;
  int64_t P = 0;
  int64_t off_w[16], off_b[16];
  LaunchCtx own;
  LaunchCtx* ctx = &own;      // the context in use: its own, or (sub-handle of a WaveletSiren handle) the parent's
  std::vector<void*> owned;   // every device buffer this handle allocated (dev_alloc); sf_destroy frees exactly these
  long npix = 0;          // local pixels
  double n_total = 0;     // H*W of the full image
  // state
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *mask = nullptr;
  bool has_mask = false;
  int64_t step = 0;
  double beta1_d = 0.9, beta2_d = 0.999;   // the Python doubles behind cfg.beta1/beta2 (shortest decimal that rounds to the float)
  // images
  uint16_t *wf = nullptr, *wf_last = nullptr, *wb = nullptr, *wb_last = nullptr;
  f32x4* l0tab = nullptr;
  uint16_t* l0img = nullptr;   // layer 0 as MFMA fragments (hidden 256: k_fwd_pipe)
  float* lsc = nullptr;        // fp8 deltas: link[16] | inv[16] (k_fp8_norms + k_fp8_links), rebuilt with the weight images
  float* biasw = nullptr;   // wide path: pre-scaled fp32 biases of layers 1..D-1
  bool wide = false;        // SIREN, hidden > 256: layer-at-a-time kernels (siren_wide.hip, wide_host.hip)
  bool images_dirty = true;
  float wscale = 1.f;
  float gpre = 1.f;       // power-of-two pre-scale of dL/dout (fp16 backward operands), undone in k_reduce*
  bool s8 = false;        // phase bytes (scratch_format 8 and 12): k_fwd<.., S8> + the kernels of siren_s8.hip
  bool d8 = false;        // fp8 deltas under a per-chunk adaptive pre-scale (scratch_format 8)
  bool fmt_auto = false;  // scratch_format was 0 at sf_create: the engine picks it, and moves to 16 when a mask is set
  long d_stride = 0;      // pieces per layer in the delta scratch (p_stride: phases)
  long a_stride = 0;      // wide path: pieces per layer in the activation scratch (always 16-bit)
  KmWs* km_ws = nullptr;        // sf_kmeans_fit workspace (allocated on first use)
  KmWs* kmq_ws = nullptr;       // sf_quant_pass: one workspace row per layer (allocated on first use)
  MaskRow* mask_rows = nullptr; // sf_mask_update without stats_dev: its statistics rows (allocated on first use)
  SnfsRow* snfs_rows = nullptr; // sf_mask_update_snfs without stats_dev: its statistics rows (allocated on first use)
  PruneWs* prune_ws = nullptr;  // sf_mask_prune_global: bucket counts, offsets, the search's answer (allocated on first use)
  unsigned* prune_keys = nullptr;   // ... and the keys filed by bucket, one per weight of the handle
  char* pad8 = nullptr;         // k_bwd8h: 1 KiB of zeros, then (at +8 KiB) an 8 KiB dump
  float* scale_dev = nullptr;   // {gpre / n_values_total, 1 / gpre} as the kernels read them (adaptive when s8)
  // data
  float *gh = nullptr, *gw = nullptr;
  bool have_coords = false;
  const float* img = nullptr;
  // scratch
  long chunk_px = 0;
  long p_stride = 0;  // pieces per layer
  u32x4 *Pbuf = nullptr, *Dbuf = nullptr, *Dlast = nullptr;
  u32x4* Abuf = nullptr;   // wide path: activations sin(phase) of every hidden layer (16-bit float, F-layout)
  float* slab = nullptr;
  int dw_wg = 0;
  float* sse_part = nullptr;
  long n_sse = 0;         // partials sse_part holds (alloc_sse)
  double* sse_dev = nullptr;   // the pass's SSE and, in the word behind it, sf_eval's integer sum (one copy reads both)
  unsigned long long* sse8_part = nullptr;   // sf_eval: the integer partials of the EVAL forms, n_sse of them (allocated on first use)
  // render handle (sf_render_create, siren_render.hip; sf_fourier_render_create, fourier_render.hip; sf_wavelet_render_create,
  // wavelet_render.hip): parameters, forward images and coordinates only - no gradient, no optimiser state, no mask, no
  // backward scratch; every training entry point refuses it.  sf_feather_render_attach (feather_host.hip) adds the feather
  // vector of a Feathermap fit to a SIREN one (fth.p, fth.args): its parameters are then what sf_feather_render_load
  // materialises, and sf_set_params / sf_params_changed are refused
  bool render = false;
  // graph replay of whole training steps (sf_step): small fits are bound by launch latency, not by the kernels
  struct Graph {
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraphExec_t exec = nullptr;
    const float* img = nullptr;   // the target and mask state the captured step holds
    bool mask = false;
    bool want = false;            // sf_set_graph_replay
    double* loss_dst = nullptr;   // eager multi-step sf_step: where k_sse_reduce also stores this step's SSE
    float* step_tab = nullptr;
    double* loss_tab = nullptr;
    int* iter_dev = nullptr;
    int tab_cap = 0;
  } graph;
  // sf_step_many with this handle as its first member (many_host.hip): the device block of a call - step counter, argument
  // tables, per-step scalars, loss table - and two pinned staging blocks it is filled from, used in turn (ev[i]: the copy out
  // of block i has been issued and may still be pending)
  struct Many {
    char* dev = nullptr;
    size_t dev_cap = 0;
    char* host[2] = {nullptr, nullptr};
    size_t host_cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    int turn = 0;
  } many;
  // Model::Fourier (fourier_host.hip, fourier_kernels.hip): D = number of Linear layers, WD = hidden width.  A render handle
  // keeps the parameters, img, B and the two coordinate vectors
  struct Fourier {
    int MS = 0;                   // map_size (encoding width)
    float* B = nullptr;           // encoding.B [in_features][MS/2] (sf_set_encoding)
    bool have_B = false;
    u32x4* img = nullptr;         // fp16 weight images (forward of every layer, backward of layers >= 1)
    long img_f[kFfMaxLinear] = {0}, img_b[kFfMaxLinear] = {0}, img_n = 0;   // offsets / size in 16-byte units
    _Float16 *H = nullptr, *G = nullptr, *Z = nullptr;   // [D-1][WD][chunk] ReLU outputs, gradients; [3][chunk] dL/dz
    int dw_wgs = 0;               // max weight-gradient workgroups along the pixels (slab rows)
  } ff;
  // Feathermap (sf_feather_attach, feather_host.hip): the weights are materialised from [V1 | V2 | scalers], and
  // sf_adam_step runs adjoint -> Adam on the feather vector -> materialise instead of Adam on W.  A render handle
  // (sf_feather_render_attach) holds args and p alone: every other pointer stays null and nothing launched on it reads one
  struct Feather {
    bool attached = false;
    bool fresh = false;           // g holds the adjoint of the current dL/dW (cleared by every training pass)
    bool loaded = false;          // render handle: sf_feather_render_load has materialised W at least once
    FthArgs args;
    long nf = 0;                  // 2 n m + 2 D
    float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
    float *V = nullptr, *G = nullptr, *part = nullptr;
    long* chunks = nullptr;
    int* chunk0 = nullptr;
  } fth;
  // Model::Wavelet (wavelet_host.hip, wavelet_kernels.hip): two SIREN sub-handles whose parameter, gradient, moment and mask
  // buffers are slices of this handle's (never on the sub-handles' owned lists); this handle owns the composition, the
  // loss and the optimiser.  A render handle (wavelet_render.hip) has two render sub-handles on the joint parameter vector,
  // pred as the one pair of coefficient buffers of the largest window, and gh / gw the caller's FULL coefficient-grid
  // vectors, which every sf_wavelet_render call slices
  struct Wavelet {
    sf_engine* sub[2] = {nullptr, nullptr};   // LF, HF
    int n = 0;                    // coefficient side
    float up = 0.f;               // bilinear source-index scale
    float* pred = nullptr;        // [2][n*n][3] sub-network predictions
    float* g = nullptr;           // [H*H][3] dL/d(Y, Cb, Cr)
    float* gl = nullptr;          // two-pass only: [2][n*n][3] fp32 dL/dout of the sub-networks
    float* dfac = nullptr;        // outermost_linear=False only: [2][n*n][3] d sin(om z)/dz of the sub-networks' outputs
    int max_rows = 0, max_cols = 0;   // render handle: the largest pixel window one call draws
    // on a sub-handle (a Model::Siren handle), sine output layer: its slice of dfac (FwdArgs::dfac of training forwards)
    float* dfac_out = nullptr;
  } wv;
};

namespace {

// Timing scope of one profile record: while it lives, what the handle launches lies between two events (when profiling).
// Several kernels under one scope are one record (k_fp8_norms + k_fp8_links + k_images under K_IMAGES).
struct Launch {
  LaunchCtx* c;
  bool on;
  ProfRec r;
  Launch(sf_engine* h_, int id, double flops, double bytes) : c(h_->ctx), on(c->prof) {
    if (!on) return;
    r.id = id;
    auto get = [&](hipEvent_t* e) {
      if (!c->ev_pool.empty()) { *e = c->ev_pool.back(); c->ev_pool.pop_back(); }
      else hipEventCreate(e);
    };
    get(&r.e0);
    get(&r.e1);
    hipEventRecord(r.e0, c->stream);
    c->flops[id] += flops;   // totals; sf_profile_get reports the per-launch average
    c->bytes[id] += bytes;
  }
  ~Launch() {
    if (!on) return;
    hipEventRecord(r.e1, c->stream);
    try { c->recs.push_back(r); } catch (...) {}   // out of memory: this record is lost, its two events with it
  }
  Launch(const Launch&) = delete;
  Launch& operator=(const Launch&) = delete;
};
// bytes a render launch is charged per output sample: 4 for the fp32 prediction, bits / 8 for the sample, each when asked for
double render_sample_bytes(const void* out, int bits, const float* pred) { return (pred ? 4.0 : 0.0) + (out ? bits / 8.0 : 0.0); }

int prof_flush(LaunchCtx* c) {
  if (c->recs.empty()) return SF_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& r : c->recs) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.e0, r.e1);
    c->ms[r.id] += ms;
    c->n[r.id] += 1;
    c->ev_pool.push_back(r.e0);
    c->ev_pool.push_back(r.e1);
  }
  c->recs.clear();
  return SF_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is set once per (device, kernel): the call costs microseconds and the
// small fits are launch-latency bound (14 launches in 73 us at 64x4)
template <typename K>
int set_lds(K kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const void* fn = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({dev, fn});
  if (it != done.end() && it->second >= bytes) return SF_OK;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done[{dev, fn}] = bytes;
  return SF_OK;
}

// The one kernel launch of the library: the kernel's dynamic-LDS limit (set_lds), the launch on the handle's stream, the
// launch error.  The kernel is named once per call site, so the limit cannot go to one kernel and the launch to another.
template <typename... P, typename... A>
int launch(sf_engine* h, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
  if (lds) SF_TRY(set_lds(kernel, lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, h->ctx->stream, static_cast<P>(args)...);
  HIPCHK(hipGetLastError());
  return SF_OK;
}

// The one hidden-width dispatch (width <= 256), the one operand-type dispatch and a run-time bool as a type: f receives
// std::integral_constant<int, WD>, an OpF16 / OpBF16 tag or std::true_type / std::false_type, so one generic lambda stands for
// the kernel instantiations of all of them.
template <typename F>
int with_width(const sf_engine* h, F&& f) {
  using std::integral_constant;
  const int w = h->WD;
  return w == 32    ? f(integral_constant<int, 32>{})
         : w == 64  ? f(integral_constant<int, 64>{})
         : w == 128 ? f(integral_constant<int, 128>{})
         : w == 256 ? f(integral_constant<int, 256>{})
                    : fail(SF_ERR_INVALID, "unsupported hidden width");
}
template <typename F>
int with_op(const sf_engine* h, F&& f) { return h->cfg.compute_dtype == SF_F16 ? f(OpF16{}) : f(OpBF16{}); }
template <typename F>
int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F>
int with_bool(bool b0, bool b1, F&& f) {
  return with_bool(b0, [&](auto x) { return with_bool(b1, [&](auto y) { return f(x, y); }); });
}

// ---- what the argument structs of the chunked kernels share ---------------------------------------------------------
// One chunk of a handle's local pixels: first pixel, length, 256-pixel groups, 32-pixel blocks
struct Chunk {
  long pix0, px;
  int n_super;
  long n_pb;
};
long n_chunks(long npix, long chunk_px) { return (npix + chunk_px - 1) / chunk_px; }
Chunk chunk_at(long c, long npix, long chunk_px) {
  Chunk k;
  k.pix0 = c * chunk_px;   // a multiple of 256: every wave's 32-pixel block starts on a dword of a byte picture
  k.px = std::min(chunk_px, npix - k.pix0);
  k.n_super = (int)((k.px + kSuper - 1) / kSuper);
  k.n_pb = (long)k.n_super * kWavesFwd;
  return k;
}
// The pixels a handle's kernels walk: the two coordinate vectors, the row length, the pixel count.  Its own grid, or
// (sf_wavelet_render on a sub-handle) the coefficient window of one call
struct PixelView { const float *gh, *gw; int W; long npix; };
PixelView own_view(const sf_engine* h) { return {h->gh, h->gw, h->cfg.width, h->npix}; }
// pixel geometry of the chunk at local pixel pix0, for any argument struct that decodes (row, col) from a pixel index
template <typename Args>
void fill_pixels(const sf_engine* h, const PixelView& v, long pix0, Args& a) {
  a.pix0 = pix0; a.npix = v.npix; a.W = v.W; a.row_begin = h->cfg.row_begin;
  a.w_magic = ((1ULL << 40) + (unsigned long long)v.W - 1) / (unsigned long long)v.W;
}
// ... and for the backward structs, which also re-derive the coordinates from (row, col)
template <typename Args>
void fill_grid(const sf_engine* h, long pix0, Args& a) {
  fill_pixels(h, own_view(h), pix0, a);
  a.inv_hm1 = h->cfg.height > 1 ? 1.0f / (float)(h->cfg.height - 1) : 0.f;
  a.inv_wm1 = h->cfg.width > 1 ? 1.0f / (float)(h->cfg.width - 1) : 0.f;
}
// dL/dout = residual * gscale: the mean over all values of the image, under the power-of-two pre-scale
float gscale(const sf_engine* h) { return (float)((double)h->gpre / ((double)h->cfg.out_features * h->n_total)); }

// the fixed-order sum of a pass's SSE partials into the handle's scalar (and this step's slot of the loss table)
int launch_sse_reduce(sf_engine* h, long n_parts) {
  Launch L(h, K_SSE, 0, (double)n_parts * 4);
  return launch(h, k_sse_reduce, 1, 256, 0, h->sse_part, n_parts, h->sse_dev, h->ctx->replay ? h->graph.loss_tab : h->graph.loss_dst,
                h->ctx->replay ? h->graph.iter_dev : h->graph.iter_dev + 2);
}

// ---------------------------------------------------------------------------------------------------------
// building and freeing a handle: the steps every creator shares
// ---------------------------------------------------------------------------------------------------------
// Device memory of a handle.  dev_alloc is the library's one hipMalloc: it records the buffer on h->owned and stores it in
// the typed field, and sf_destroy frees that list - a new buffer is one dev_alloc line and cannot be leaked.  A view into
// another handle's buffer (the state of a WaveletSiren's sub-networks) is a plain assignment and never on a list.
template <typename T>
int dev_alloc(sf_engine* h, T*& field, size_t bytes) {
  h->owned.push_back(nullptr);   // the slot first: a std::bad_alloc of the list must not strand a device buffer
  const hipError_t e = hipMalloc(&h->owned.back(), bytes ? bytes : 16);
  if (e != hipSuccess) {
    h->owned.pop_back();
    return fail(SF_ERR_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  field = static_cast<T*>(h->owned.back());
  return SF_OK;
}
// frees one owned buffer and forgets it: for the buffers that get replaced (scratch of another format, longer step tables)
void dev_free(sf_engine* h, void* p) {
  const auto it = std::find(h->owned.begin(), h->owned.end(), p);
  if (!p || it == h->owned.end()) return;
  hipFree(p);
  h->owned.erase(it);
}
// frees a handle with everything it has: the events of the launch context it owns (a sub-handle launches through its
// parent's and has none), its sub-handles, the replay graph and stream, every dev_alloc buffer
void destroy(sf_engine* h) {
  DevGuard dev_guard(h->cfg.device);
  hipStreamSynchronize(h->ctx->stream);
  for (auto& r : h->own.recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  for (hipEvent_t e : h->own.ev_pool) hipEventDestroy(e);
  for (sf_engine* s : h->wv.sub) if (s) destroy(s);
  if (h->graph.exec) hipGraphExecDestroy(h->graph.exec);
  if (h->graph.stream) { hipStreamSynchronize(h->graph.stream); hipStreamDestroy(h->graph.stream); hipEventDestroy(h->graph.ev_in); hipEventDestroy(h->graph.ev_out); }
  for (int i = 0; i < 2; ++i) {
    if (h->many.host[i]) hipHostFree(h->many.host[i]);
    if (h->many.ev[i]) hipEventDestroy(h->many.ev[i]);
  }
  for (void* p : h->owned) hipFree(p);
  delete h;
}
// a handle under construction: an early return (or an exception) destroys it with everything it owns so far
struct HandleDeleter { void operator()(sf_engine* h) const { destroy(h); } };
using HandlePtr = std::unique_ptr<sf_engine, HandleDeleter>;

// the device of a new handle exists and is a gfx950 (the creator makes it current with a DevGuard afterwards)
template <typename Config>
int check_device(const Config* cfg, hipDeviceProp_t& prop) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SF_ERR_NO_DEVICE, "no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(SF_ERR_INVALID, "bad device ordinal");
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SF_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950");
  return SF_OK;
}
// What every creator does around its own work, in the order its refusals come: the null, ABI and in_features checks (a
// configuration without the member passes nullptr); check(grid) - the model's argument checks, which also name the picture
// and the handle's rows (the WaveletSiren creators build their two sub-handles there, which run their own checks and the
// device's); the device; the new handle with its model, stream, pixel counts and workgroup budget; init(h, grid) - the
// configuration, geometry and allocations.  A failure anywhere leaves *out null and nothing allocated.
struct Grid { int height = 0, width = 0, row_begin = 0, row_end = 0; };
template <typename Config, typename Check, typename Init>
int create_with(const Config* cfg, sf_handle** out, int32_t Config::*in_features, Model model, bool render, Check&& check,
                Init&& init) {
  if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, "abi_version mismatch");
  if (in_features && cfg->*in_features != 2) return fail(SF_ERR_INVALID, "in_features must be 2 (coordinate grid)");
  Grid g;
  SF_TRY(check(g));
  hipDeviceProp_t prop;
  SF_TRY(check_device(cfg, prop));
  DevGuard dev_guard(cfg->device);   // the caller's current device is restored on return
  HandlePtr owner(new sf_engine());
  sf_engine* h = owner.get();
  h->model = model;
  h->render = render;
  h->own.stream = (hipStream_t)cfg->stream;
  h->npix = (long)(g.row_end - g.row_begin) * g.width;
  h->n_total = (double)g.height * (double)g.width;
  h->dw_wg = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  SF_TRY(init(h, g));
  *out = owner.release();
  return SF_OK;
}
// flat parameter offsets of h->D Linear layers in named_parameters() order (weight [out][in], then bias), and their sum P;
// fan_in0: what the first layer reads - the coordinate pair (2) or the encoding (map_size)
void layer_offsets(sf_engine* h, int fan_in0) {
  int64_t off = 0;
  for (int l = 0; l < h->D; ++l) {
    const int in = l == 0 ? fan_in0 : h->WD, outn = l == h->D - 1 ? h->cfg.out_features : h->WD;
    h->off_w[l] = off; off += (int64_t)in * outn;
    h->off_b[l] = off; off += outn;
  }
  h->P = off;
}
// Adam: all-zero betas / eps mean torch.optim.Adam's defaults; the doubles behind the float betas (shortest_double)
void adam_defaults(sf_engine* h) {
  sf_config& c = h->cfg;
  if (c.beta1 == 0.f && c.beta2 == 0.f && c.eps == 0.f) { c.beta1 = 0.9f; c.beta2 = 0.999f; c.eps = 1e-8f; }
  h->beta1_d = shortest_double(c.beta1);
  h->beta2_d = shortest_double(c.beta2);
}
// the flat fp32 state of a handle, zeroed on its stream: parameters and, on a training handle, gradient, Adam moments and mask
int alloc_state(sf_engine* h, bool train) {
  const size_t bytes = (size_t)h->P * 4;
  SF_TRY(dev_alloc(h, h->params, bytes));
  if (train) for (float** p : {&h->grads, &h->m, &h->v, &h->mask}) SF_TRY(dev_alloc(h, *p, bytes));
  for (float* p : {h->params, h->grads, h->m, h->v}) if (p) hipMemsetAsync(p, 0, bytes, h->ctx->stream);
  return SF_OK;
}
// chunk length of a handle: whole 256-pixel groups, at most the padded local image
long round_super(long px) { return (px + kSuper - 1) / kSuper * kSuper; }
long chunk_pixels(long want, long npix) { return std::min(round_super(want), round_super(npix)); }
// SSE partials of a chunked pass (one per 256-pixel group, then one per chunk) and the scalar they reduce to
long chunked_sse_parts(const sf_engine* h) {
  return round_super(h->npix) / kSuper + (h->npix + h->chunk_px - 1) / h->chunk_px + 8;
}
int alloc_sse(sf_engine* h, long n_sse) {
  h->n_sse = n_sse + 64;
  SF_TRY(dev_alloc(h, h->sse_part, (size_t)h->n_sse * 4));
  return dev_alloc(h, h->sse_dev, 16);
}
// sf_eval: where its integer sum lands, and the fixed-order sums of both kinds of partials of an EVAL pass
unsigned long long* sse8_dev(const sf_engine* h) { return reinterpret_cast<unsigned long long*>(h->sse_dev + 1); }
int launch_eval_reduce(sf_engine* h, long n_parts) {
  Launch L(h, K_SSE, 0, (double)n_parts * 12);
  return launch(h, k_eval_reduce, 1, 256, 0, h->sse_part, h->sse8_part, n_parts, h->sse_dev, sse8_dev(h));
}

// the model dispatch of siren_fit.hip: the weight images, the one loop over a handle's chunks (forward; if train, backward;
// the SSE reduction), and the pass - its checks, the images, then that loop or run_pass_wavelet.  eval8 (sf_eval, never with
// train or pred): the EVAL forms of the forwards, their integer partials in h->sse8_part beside the SSE partials, both reduced
int refresh_images(sf_engine* h);
int run_chunks(sf_engine* h, bool train, float* pred, bool want_sse, bool eval8 = false);
int run_pass(sf_engine* h, bool train, float* pred, bool want_sse, bool eval8 = false);

// training entry points on a render handle: an argument error, before anything is touched
int refuse_render(const char* fn) {
  return fail(SF_ERR_INVALID, std::string(fn) + ": a render handle (sf_render_create) holds parameters and forward images "
                                                "only - no gradient, optimiser state, mask or backward scratch");
}
#define SF_NO_RENDER(h, fn) do { if ((h) && (h)->render) return refuse_render(fn); } while (0)
// writing W on a render handle with a feather state (sf_feather_render_attach): W is what the feather vector materialises to
int refuse_feather_render(const char* fn) {
  return fail(SF_ERR_INVALID, std::string(fn) + ": the parameters of a feather render handle (sf_feather_render_attach) belong "
                                                "to its feather vector - load that with sf_feather_render_load");
}
#define SF_NO_FEATHER_RENDER(h, fn) do { if ((h) && (h)->render && (h)->fth.attached) return refuse_feather_render(fn); } while (0)

}  // namespace
