// siren_fit.hip — C ABI (include/siren_fit.h) and host-side orchestration of the gfx950 kernels.
//
// One sf_engine == one per-image fit on one HIP stream.  A training step is, per pixel chunk:
//   k_fwd -> k_bwd(last) -> k_bwd(hidden l = depth-2 .. 1) -> k_dw0, each followed by the fixed-order slab
//   reduction into the flat fp32 gradient; then k_adam (+mask) and k_images (16-bit weight images).
// The sequence mirrors one `train_epoch` of the reference (implicit_image/utils/train_helper.py:132-185)
// for the full-batch grid (implicit_image/compress.py:137-138).
#include "siren_kernels.hip"
#include "siren_s8.hip"
#include "siren_s8h.hip"
#include "siren_wide.hip"
#include "siren_kmeans.hip"
#include "fourier_kernels.hip"
#include "feather_kernels.hip"
#include "wavelet_kernels.hip"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
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

// hidden 256, 16-bit scratch (k_bwd): 8 waves (two per SIMD), all weight rows in registers, 5 x 32 KiB ring = 160 KiB: 96 KiB
// in flight; the P0 variant needs more registers and keeps the 4-wave / 4-slot form
constexpr int kBwd16P0WC = 2;
constexpr int kBwd16NB = 5;
constexpr int kBwd16P0NB = 4;
constexpr int kBwd8hPark = 4;   // k_bwd8h: k-steps of every wave's stationary W^T rows parked in LDS

// Every template kernel of the library, in the order the code object holds them.  The compiler emits instantiations in the
// order of their first use, so this list - their first use - keeps the device code byte for byte what it was measured as,
// however the host code below is arranged: a host-only change leaves the sha256 of the device object alone.  A kernel the
// launch code asks for and this list lacks is still built (behind these); one listed and never launched would be built too.
#define SF_K(...) reinterpret_cast<const void*>(&__VA_ARGS__)
[[maybe_unused]] static const void* const kKernelOrder[] = {
    SF_K(k_fwd_pipe<OpF16, true, true, kFwdPD, false>), SF_K(k_fwd_pipe<OpF16, true, false, kFwdPD, false>),
    SF_K(k_fwd_pipe<OpF16, false, false, kFwdPD, false>), SF_K(k_fwd_pipe<OpBF16, true, false, kFwdPD, false>),
    SF_K(k_fwd_pipe<OpBF16, false, false, kFwdPD, false>), SF_K(k_bwd<32, 32, 1, 1, true, true, OpF16, 8>),
    SF_K(k_bwd<32, 32, 1, 1, true, true, OpBF16, 8>), SF_K(k_bwd<32, 32, 1, 1, true, false, OpF16, 8>),
    SF_K(k_bwd<32, 32, 1, 1, true, false, OpBF16, 8>), SF_K(k_bwd<32, 32, 1, 1, false, true, OpF16, 8>),
    SF_K(k_bwd<32, 32, 1, 1, false, true, OpBF16, 8>), SF_K(k_bwd<32, 32, 1, 1, false, false, OpF16, 8>),
    SF_K(k_bwd<32, 32, 1, 1, false, false, OpBF16, 8>), SF_K(k_bwd<32, 64, 1, 2, true, true, OpF16, 8>),
    SF_K(k_bwd<32, 64, 1, 2, true, true, OpBF16, 8>), SF_K(k_bwd<32, 64, 1, 2, true, false, OpF16, 8>),
    SF_K(k_bwd<32, 64, 1, 2, true, false, OpBF16, 8>), SF_K(k_bwd<64, 64, 2, 1, false, true, OpF16, 8>),
    SF_K(k_bwd<64, 64, 2, 1, false, true, OpBF16, 8>), SF_K(k_bwd<64, 64, 2, 1, false, false, OpF16, 8>),
    SF_K(k_bwd<64, 64, 2, 1, false, false, OpBF16, 8>), SF_K(k_bwd<32, 128, 1, 4, true, true, OpF16, 8>),
    SF_K(k_bwd<32, 128, 1, 4, true, true, OpBF16, 8>), SF_K(k_bwd<32, 128, 1, 4, true, false, OpF16, 8>),
    SF_K(k_bwd<32, 128, 1, 4, true, false, OpBF16, 8>), SF_K(k_bwd<128, 128, 2, 2, false, true, OpF16, 8>),
    SF_K(k_bwd<128, 128, 2, 2, false, true, OpBF16, 8>), SF_K(k_bwd<128, 128, 2, 2, false, false, OpF16, 8>),
    SF_K(k_bwd<128, 128, 2, 2, false, false, OpBF16, 8>), SF_K(k_bwd<32, 256, 1, 8, true, true, OpF16, 8>),
    SF_K(k_bwd<32, 256, 1, 8, true, true, OpBF16, 8>), SF_K(k_bwd<32, 256, 1, 8, true, false, OpF16, 8>),
    SF_K(k_bwd<32, 256, 1, 8, true, false, OpBF16, 8>),
    SF_K(k_bwd<256, 256, 2, kBwd16P0WC, false, true, OpF16, kBwd16P0NB>),
    SF_K(k_bwd<256, 256, 2, kBwd16P0WC, false, true, OpBF16, kBwd16P0NB>),
    SF_K(k_bwd<256, 256, 2, 4, false, false, OpF16, kBwd16NB>),
    SF_K(k_bwd<256, 256, 2, 4, false, false, OpBF16, kBwd16NB>),
    SF_K(k_bwd8<32, 32, 1, 1, true, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 32, 1, 1, true, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 32, 1, 1, false, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 32, 1, 1, false, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 64, 1, 2, true, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 64, 1, 2, true, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<64, 64, 2, 1, false, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<64, 64, 2, 1, false, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 128, 1, 4, true, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 128, 1, 4, true, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<128, 128, 2, 2, false, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<128, 128, 2, 2, false, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 256, 1, 8, true, true, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<32, 256, 1, 8, true, false, OpF16, 8, 0, 0, false>),
    SF_K(k_bwd8<256, 256, 2, 4, false, true, OpF16, 5, 4, 0, false>),
    SF_K(k_bwd8<256, 256, 2, 4, false, false, OpF16, 5, 2, 3, false>), SF_K(k_bwd8h<kBwd8hPark>),
    SF_K(k_bwd8<32, 32, 1, 1, true, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 32, 1, 1, true, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 32, 1, 1, false, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 32, 1, 1, false, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 64, 1, 2, true, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 64, 1, 2, true, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<64, 64, 2, 1, false, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<64, 64, 2, 1, false, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 128, 1, 4, true, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 128, 1, 4, true, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<128, 128, 2, 2, false, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<128, 128, 2, 2, false, false, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 256, 1, 8, true, true, OpF16, 8, 0, 0, true>),
    SF_K(k_bwd8<32, 256, 1, 8, true, false, OpF16, 4, 0, 4, true>),
    SF_K(k_dw0_8<32, OpF16, 8>),
    SF_K(k_dw0_8<64, OpF16, 8>), SF_K(k_dw0_8<128, OpF16, 8>), SF_K(k_dw0_8<256, OpF16, 4>), SF_K(k_dw0<32, OpF16>),
    SF_K(k_dw0<32, OpBF16>), SF_K(k_dw0<64, OpF16>), SF_K(k_dw0<64, OpBF16>), SF_K(k_dw0<128, OpF16>),
    SF_K(k_dw0<128, OpBF16>), SF_K(k_fwd<32, OpF16, true, true, false>), SF_K(k_fwd<32, OpF16, true, false, false>),
    SF_K(k_fwd<32, OpF16, false, false, false>), SF_K(k_fwd<32, OpBF16, true, false, false>),
    SF_K(k_fwd<32, OpBF16, false, false, false>), SF_K(k_fwd<64, OpF16, true, true, false>),
    SF_K(k_fwd<64, OpF16, true, false, false>), SF_K(k_fwd<64, OpF16, false, false, false>),
    SF_K(k_fwd<64, OpBF16, true, false, false>), SF_K(k_fwd<64, OpBF16, false, false, false>),
    SF_K(k_fwd<128, OpF16, true, true, false>), SF_K(k_fwd<128, OpF16, true, false, false>),
    SF_K(k_fwd<128, OpF16, false, false, false>), SF_K(k_fwd<128, OpBF16, true, false, false>),
    SF_K(k_fwd<128, OpBF16, false, false, false>), SF_K(k_fwd<256, OpF16, true, true, false>),
    SF_K(k_fwd<256, OpF16, true, false, false>), SF_K(k_fwd<256, OpF16, false, false, false>),
    SF_K(k_fwd<256, OpBF16, true, false, false>), SF_K(k_fwd<256, OpBF16, false, false, false>),
    SF_K(k_wlayer0<OpF16, true>), SF_K(k_wlayer0<OpF16, false>), SF_K(k_wlayer0<OpBF16, false>),
    SF_K(k_wgemm2<0, OpF16, true, false, false>), SF_K(k_wgemm2<0, OpF16, false, false, false>),
    SF_K(k_wgemm2<0, OpBF16, false, false, false>), SF_K(k_wgemm<1, OpF16>), SF_K(k_wgemm<1, OpBF16>),
    SF_K(k_wdw<32, OpF16, false>), SF_K(k_wdw<32, OpBF16, false>), SF_K(k_wdw<256, OpF16, true>),
    SF_K(k_wdw<256, OpF16, false>), SF_K(k_wdw<256, OpBF16, false>), SF_K(k_wgemm2<2, OpF16, true, false, true>),
    SF_K(k_wgemm2<2, OpF16, true, true, true>), SF_K(k_wgemm2<2, OpF16, true, false, false>),
    SF_K(k_wgemm2<2, OpF16, false, false, false>), SF_K(k_wgemm2<2, OpBF16, false, false, false>),
    SF_K(k_dw0<256, OpF16>), SF_K(k_dw0<256, OpBF16>), SF_K(k_ff_fwd<32, false, false>), SF_K(k_ff_fwd<32, true, false>),
    SF_K(k_ff_bwd<32>), SF_K(k_ff_fwd<64, false, false>), SF_K(k_ff_fwd<64, true, false>), SF_K(k_ff_bwd<64>),
    SF_K(k_ff_fwd<128, false, false>), SF_K(k_ff_fwd<128, true, false>), SF_K(k_ff_bwd<128>),
    SF_K(k_ff_fwd<256, false, false>), SF_K(k_ff_fwd<256, true, false>), SF_K(k_ff_bwd<256>), SF_K(k_ff_dw<1, true>),
    SF_K(k_ff_dw<2, true>), SF_K(k_ff_dw<4, true>), SF_K(k_ff_dw<1, false>), SF_K(k_ff_dw<2, false>),
    SF_K(k_ff_dw<4, false>), SF_K(k_fwd_pipe<OpF16, false, false, kFwdPD, true>),
    SF_K(k_fwd_pipe<OpBF16, false, false, kFwdPD, true>), SF_K(k_fwd<32, OpF16, false, false, true>),
    SF_K(k_fwd<32, OpBF16, false, false, true>), SF_K(k_fwd<64, OpF16, false, false, true>),
    SF_K(k_fwd<64, OpBF16, false, false, true>), SF_K(k_fwd<128, OpF16, false, false, true>),
    SF_K(k_fwd<128, OpBF16, false, false, true>), SF_K(k_fwd<256, OpF16, false, false, true>),
    SF_K(k_fwd<256, OpBF16, false, false, true>), SF_K(k_ff_fwd<32, false, true>), SF_K(k_ff_fwd<64, false, true>),
    SF_K(k_ff_fwd<128, false, true>), SF_K(k_ff_fwd<256, false, true>),
};
#undef SF_K

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

// the kernels take phases in revolutions: omega / 2 pi, formed in double
static constexpr double kTwoPi = 6.283185307179586476925286766559;

// 8-bit scratch: dL/dout is stored as residual * 2^10 in fp16 (residuals of 6e-8 .. 64 stay normal numbers); the
// adaptive part of the gradient pre-scale is applied by k_bwd8<LAST> (siren_s8.hip)
static constexpr float kResScale = 1024.0f;

// (k_bwd_layer1: the backward of layer 1, whose input phases are re-derived from the coordinates - another kernel form than
//  the hidden layers', so it gets its own line in the per-kernel report)
// (k_feather_*: the Feathermap update of sf_adam_step on a handle with sf_feather_attach, feather_kernels.hip)
enum KernelId { K_FWD = 0, K_BWD_HIDDEN, K_BWD_LAST, K_DW_FIRST, K_REDUCE, K_SSE, K_ADAM, K_IMAGES, K_BWD_L1,
                K_FTH_GRAD, K_FTH_DV, K_FTH_ADAM, K_FTH_MAT, K_WV_COMPOSE, K_WV_ADJOINT, K_WV_INJECT, K_RENDER, K_WV_RENDER, K_FF_RENDER, K_COUNT };
// (k_wv_*: the image-space composition of a WaveletSiren handle and its adjoint, wavelet_kernels.hip)
static const char* kKernelNames[K_COUNT] = {"k_fwd",    "k_bwd_hidden", "k_bwd_last", "k_dw_first",
                                            "k_reduce", "k_sse",        "k_adam",     "k_images", "k_bwd_layer1",
                                            "k_feather_grad", "k_feather_dv", "k_feather_adam", "k_feather_mat",
                                            "k_wv_compose", "k_wv_adjoint", "k_wv_inject", "k_render", "k_wv_render", "k_ff_render"};

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

struct sf_engine {
  sf_config cfg;
  int D = 0, WD = 0;
  int64_t P = 0;
  int64_t off_w[16], off_b[16];
  hipStream_t stream = nullptr;
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
  bool wide = false;        // hidden > 256: layer-at-a-time kernels (siren_wide.hip)
  bool images_dirty = true;
  float wscale = 1.f;
  float gpre = 1.f;       // power-of-two pre-scale of dL/dout (fp16 backward operands), undone in k_reduce*
  bool s8 = false;        // phase bytes (scratch_format 8 and 12): k_fwd<.., S8> + the kernels of siren_s8.hip
  bool d8 = false;        // fp8 deltas under a per-chunk adaptive pre-scale (scratch_format 8)
  bool fmt_auto = false;  // scratch_format was 0 at sf_create: the engine picks it, and moves to 16 when a mask is set
  long d_stride = 0;      // pieces per layer in the delta scratch (p_stride: phases)
  long a_stride = 0;      // wide path: pieces per layer in the activation scratch (always 16-bit)
  KmWs* km_ws = nullptr;        // sf_kmeans_fit workspace (allocated on first use)
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
  double* sse_dev = nullptr;
  // graph replay of whole training steps (sf_step): small fits are bound by launch latency, not by the kernels
  hipStream_t gstream = nullptr;
  hipEvent_t gev_in = nullptr, gev_out = nullptr;
  hipGraphExec_t gexec = nullptr;
  const float* g_img = nullptr;
  bool g_mask = false;
  bool replay = false;      // launches issued now belong to a replayed step: per-step scalars come from device tables
  bool want_replay = false; // sf_set_graph_replay
  double* loss_dst = nullptr;   // eager multi-step sf_step: where k_sse_reduce also stores this step's SSE
  float* step_tab = nullptr;
  double* loss_tab = nullptr;
  int* iter_dev = nullptr;
  int tab_cap = 0;
  // profiling
  bool prof = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> ev_pool;   // recycled timing events (creating two per launch costs more than a small kernel)
  double prof_ms[K_COUNT] = {0};
  int64_t prof_n[K_COUNT] = {0};
  double prof_flops[K_COUNT] = {0}, prof_bytes[K_COUNT] = {0};
  // FourierNet handle (sf_fourier_create, fourier_kernels.hip): D = number of Linear layers, WD = hidden width
  bool fourier = false;
  int MS = 0;                   // map_size (encoding width)
  float* ffB = nullptr;         // encoding.B [in_features][MS/2] (sf_set_encoding)
  bool have_B = false;
  u32x4* ffimg = nullptr;       // fp16 weight images (forward of every layer, backward of layers >= 1)
  long ff_img_f[kFfMaxLinear] = {0}, ff_img_b[kFfMaxLinear] = {0}, ff_img_n = 0;   // offsets / size in 16-byte units
  _Float16 *ffH = nullptr, *ffG = nullptr, *ffZ = nullptr;   // [D-1][WD][chunk] ReLU outputs, gradients; [3][chunk] dL/dz
  int ff_dw_wgs = 0;            // max weight-gradient workgroups along the pixels (slab rows)
  // Feathermap (sf_feather_attach, feather_kernels.hip): the weights are materialised from [V1 | V2 | scalers], and
  // sf_adam_step runs adjoint -> Adam on the feather vector -> materialise instead of Adam on W
  bool feather = false;
  bool fth_fresh = false;       // fth_g holds the adjoint of the current dL/dW (cleared by every training pass)
  FthArgs fth;
  long fth_nf = 0;              // 2 n m + 2 D
  float *fth_p = nullptr, *fth_g = nullptr, *fth_m = nullptr, *fth_v = nullptr;
  float *fth_V = nullptr, *fth_G = nullptr, *fth_part = nullptr;
  long* fth_chunks = nullptr;
  int* fth_chunk0 = nullptr;
  // WaveletSiren (sf_wavelet_create, wavelet_kernels.hip): two SIREN sub-handles whose parameter, gradient, moment and
  // mask buffers are slices of this handle's (never on the sub-handles' owned lists); this handle owns the composition,
  // the loss and the optimiser
  bool wavelet = false;
  sf_engine* wv_sub[2] = {nullptr, nullptr};   // LF, HF
  bool ext_dout = false;        // sub-handle: the training forward runs without a target, dL/dout comes from k_wv_adjoint
  int wv_n = 0;                 // coefficient side
  float wv_up = 0.f;            // bilinear source-index scale
  float* wv_pred = nullptr;     // [2][n*n][3] sub-network predictions
  float* wv_g = nullptr;        // [H*H][3] dL/d(Y, Cb, Cr)
  float* wv_gl = nullptr;       // two-pass only: [2][n*n][3] fp32 dL/dout of the sub-networks
  float* wv_dfac = nullptr;     // outermost_linear=False only: [2][n*n][3] d sin(om z)/dz of the sub-networks' outputs
  float* dfac_out = nullptr;    // sub-handle, sine output layer: its slice of wv_dfac (FwdArgs::dfac of training forwards)
  // (a FourierNet render handle, sf_fourier_render_create / fourier_render.hip, sets fourier and render: parameters, ffimg,
  //  ffB and the two coordinate vectors)
  // render handle (sf_render_create, siren_render.hip): parameters, forward images and coordinates only - no gradient, no
  // optimiser state, no mask, no backward scratch; every training entry point refuses it
  bool render = false;
  // WaveletSiren render handle (sf_wavelet_render_create, wavelet_render.hip): wavelet and render both set.  Two render
  // sub-handles on the joint parameter vector, wv_pred as the one pair of coefficient buffers of the largest window, and
  // gh / gw the caller's FULL coefficient-grid vectors, which every sf_wavelet_render call slices
  int wv_max_rows = 0, wv_max_cols = 0;   // the largest pixel window one call draws
};

namespace {

// Timing scope of one profile record: while it lives, what the handle launches lies between two events (when profiling).
// Several kernels under one scope are one record (k_fp8_norms + k_fp8_links + k_images under K_IMAGES).
struct Launch {
  sf_engine* h;
  bool on;
  ProfRec r;
  Launch(sf_engine* h_, int id, double flops, double bytes) : h(h_), on(h_->prof) {
    if (!on) return;
    r.id = id;
    auto get = [&](hipEvent_t* e) {
      if (!h->ev_pool.empty()) { *e = h->ev_pool.back(); h->ev_pool.pop_back(); }
      else hipEventCreate(e);
    };
    get(&r.e0);
    get(&r.e1);
    hipEventRecord(r.e0, h->stream);
    h->prof_flops[id] += flops;   // totals; sf_profile_get reports the per-launch average
    h->prof_bytes[id] += bytes;
  }
  ~Launch() {
    if (!on) return;
    hipEventRecord(r.e1, h->stream);
    try { h->recs.push_back(r); } catch (...) {}   // out of memory: this record is lost, its two events with it
  }
  Launch(const Launch&) = delete;
  Launch& operator=(const Launch&) = delete;
};

int prof_flush(sf_engine* h) {
  if (h->recs.empty()) return SF_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  for (auto& r : h->recs) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.e0, r.e1);
    h->prof_ms[r.id] += ms;
    h->prof_n[r.id] += 1;
    h->ev_pool.push_back(r.e0);
    h->ev_pool.push_back(r.e1);
  }
  h->recs.clear();
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
  hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, static_cast<P>(args)...);
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
// pixel geometry of the chunk at local pixel pix0, for any argument struct that decodes (row, col) from a pixel index
template <typename Args>
void fill_pixels(const sf_engine* h, long pix0, Args& a) {
  a.pix0 = pix0; a.npix = h->npix; a.W = h->cfg.width; a.row_begin = h->cfg.row_begin;
  a.w_magic = ((1ULL << 40) + (unsigned long long)h->cfg.width - 1) / (unsigned long long)h->cfg.width;
}
// ... and for the backward structs, which also re-derive the coordinates from (row, col)
template <typename Args>
void fill_grid(const sf_engine* h, long pix0, Args& a) {
  fill_pixels(h, pix0, a);
  a.inv_hm1 = h->cfg.height > 1 ? 1.0f / (float)(h->cfg.height - 1) : 0.f;
  a.inv_wm1 = h->cfg.width > 1 ? 1.0f / (float)(h->cfg.width - 1) : 0.f;
}
// dL/dout = residual * gscale: the mean over all values of the image, under the power-of-two pre-scale
float gscale(const sf_engine* h) { return (float)((double)h->gpre / ((double)h->cfg.out_features * h->n_total)); }

// the fixed-order sum of a pass's SSE partials into the handle's scalar (and this step's slot of the loss table)
int launch_sse_reduce(sf_engine* h, long n_parts) {
  Launch L(h, K_SSE, 0, (double)n_parts * 4);
  return launch(h, k_sse_reduce, 1, 256, 0, h->sse_part, n_parts, h->sse_dev, h->replay ? h->loss_tab : h->loss_dst,
                h->replay ? h->iter_dev : h->iter_dev + 2);
}
// per-layer fp8 delta scales (link[16] | inv[16] | norms in h->lsc), rebuilt with the weight images
int launch_fp8_scales(sf_engine* h) {
  Fp8ScaleArgs f;
  memset(&f, 0, sizeof(f));
  f.params = h->params; f.depth = h->D; f.WD = h->WD; f.out_features = h->cfg.out_features;
  for (int l = 0; l < h->D; ++l) f.off_w[l] = h->off_w[l];
  f.om_first = h->cfg.first_omega_0; f.om_hidden = h->cfg.hidden_omega_0; f.link = h->lsc; f.inv = h->lsc + 16;
  f.nrm = reinterpret_cast<double*>(h->lsc + 32);
  SF_TRY(launch(h, k_fp8_norms, h->D - 1, 1024, 0, f));
  return launch(h, k_fp8_links, 1, 64, 0, f);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
size_t fwd_lds_bytes(int WD) { return (size_t)FwdGeom(WD).PIECES * 1024 + (size_t)WD * 16 + 64; }
// k_fwd_pipe: weight image halves + layer-0 image + SSE partials
size_t fwd_pipe_lds_bytes() { return (size_t)FwdGeom(256).PIECES * 1024 + (size_t)(256 / 32) * 1024 + 64; }

// hidden = 256, depth >= 3 run the persistent pipeline kernel (k_fwd_pipe): one workgroup per CU walks the chunk
bool fwd_is_pipe(const sf_engine* h) { return h->WD == 256 && h->D >= 3 && !h->wide; }
// forward workgroups of a chunk with n_super 256-pixel groups (= the chunk's SSE partials)
int fwd_grid(const sf_engine* h, int n_super) { return fwd_is_pipe(h) && n_super > h->dw_wg ? h->dw_wg : n_super; }

// hidden = 256, depth >= 3: the hand-scheduled software pipeline over all layers (k_fwd_pipe)
int launch_fwd_pipe(sf_engine* h, const FwdArgs& a, int n_wg, bool train) {
  const size_t lds = fwd_pipe_lds_bytes();
  const bool f16 = h->cfg.compute_dtype == SF_F16;
  if (f16 && train && h->s8) return launch(h, k_fwd_pipe<OpF16, true, true>, n_wg, 512, lds, a);
  return with_op(h, [&](auto op) {
    using OP = decltype(op);
    return train ? launch(h, k_fwd_pipe<OP, true, false>, n_wg, 512, lds, a) : launch(h, k_fwd_pipe<OP, false, false>, n_wg, 512, lds, a);
  });
}
// the forward of a chunk on n_wg workgroups (fwd_grid): phase bytes (fp16 operands only), training or evaluation form
int launch_fwd(sf_engine* h, const FwdArgs& a, int n_wg, bool train) {
  if (fwd_is_pipe(h)) return launch_fwd_pipe(h, a, n_wg, train);
  return with_width(h, [&](auto wd) {
    constexpr int WD = decltype(wd)::value;
    const size_t lds = fwd_lds_bytes(WD);
    if (h->cfg.compute_dtype == SF_F16 && train && h->s8) return launch(h, k_fwd<WD, OpF16, true, true>, n_wg, 512, lds, a);
    return with_op(h, [&](auto op) {
      using OP = decltype(op);
      return train ? launch(h, k_fwd<WD, OP, true>, n_wg, 512, lds, a) : launch(h, k_fwd<WD, OP, false>, n_wg, 512, lds, a);
    });
  });
}

// what every forward of a SIREN handle (width <= 256) is given for the chunk that starts at local pixel pix0: coordinates,
// geometry, weight images and scales; the caller adds its outputs (scratch, target, prediction, partials)
FwdArgs fwd_args_base(const sf_engine* h, long pix0, int n_super) {
  FwdArgs fa;
  memset(&fa, 0, sizeof(fa));
  fill_pixels(h, pix0, fa);
  fa.gh = h->gh; fa.gw = h->gw; fa.depth = h->D;
  fa.l0tab = h->l0tab; fa.l0img = reinterpret_cast<const u32x4*>(h->l0img);
  fa.wf = reinterpret_cast<const u32x4*>(h->wf);
  fa.wf_last = reinterpret_cast<const u32x4*>(h->wf_last);
  fa.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
  fa.sc_hidden = (float)((double)h->cfg.hidden_omega_0 / kTwoPi / (double)h->wscale);
  fa.sc_last = 1.0f / h->wscale;
  if (!h->cfg.outermost_linear) { fa.last_om = h->cfg.hidden_omega_0; fa.last_om_rev = (float)((double)h->cfg.hidden_omega_0 / kTwoPi); }
  fa.nout = h->cfg.out_features;
  fa.n_super = n_super;
  return fa;
}

// ---- backward --------------------------------------------------------------------------------------------------------
// The one tile table of the fused layer backward, <JW, IW, WR, WC> of (width, last): the last layer's out_features (<= 3,
// padded to 32) rows against one wave per 32 inputs; a hidden layer's WD x WD block on 1, 2, 4 or 8 waves.
template <int WD, bool LAST>
struct BwdTile {
  static constexpr int JW = LAST ? 32 : WD, IW = WD;
  static constexpr int WR = LAST || WD == 32 ? 1 : 2, WC = LAST ? WD / 32 : WD == 32 ? 1 : WD / 64;
};

// 16-bit scratch (k_bwd).  Ring depths are chosen to fill the 160 KiB of LDS.
template <int WD, bool LAST, bool P0, typename OP>
int launch_bwd16(sf_engine* h, const BwdLayerArgs& a, int n_wg) {
  using T = BwdTile<WD, LAST>;
  constexpr bool H256 = WD == 256 && !LAST;
  constexpr int WC = H256 && P0 ? kBwd16P0WC : T::WC, NB = H256 ? (P0 ? kBwd16P0NB : kBwd16NB) : 8;   // (the constants at the kernel list)
  // NB-slot block ring + (when the stationary weight rows do not fit in registers) their parked part
  // + (P0) the layer-0 table
  constexpr int JW = T::JW, IW = T::IW, WR = T::WR, NWV = WR * WC, XT = (IW / 32) / NWV, KSX = LAST ? 1 : JW / 16;
  constexpr int WSP = (XT * KSX > 24) ? (P0 ? 3 : 4) : 0;
  const size_t lds = (size_t)NB * (JW / 16 + IW / 16) * 1024 + (size_t)NWV * XT * WSP * 1024 + (P0 ? (size_t)IW * 16 : 0);
  return launch(h, k_bwd<JW, IW, WR, WC, LAST, P0, OP, NB>, n_wg, NWV * 64, lds, a);
}
// fused backward of one layer: last = the out_features(<=3, padded to 32)-row layer; p0 = its input layer is
// layer 0, whose phases are re-derived from the coordinates.
int launch_bwd(sf_engine* h, bool last, bool p0, const BwdLayerArgs& a, int n_wg) {
  return with_width(h, [&](auto wd) {
    return with_bool(last, p0, [&](auto l, auto p) {
      return with_op(h, [&](auto op) { return launch_bwd16<decltype(wd)::value, decltype(l)::value, decltype(p)::value, decltype(op)>(h, a, n_wg); });
    });
  });
}

// 8-bit scratch path (siren_s8.hip, k_bwd8): fp16 operands only.  D8: fp8 deltas (scratch_format 8); else phase bytes with
// 16-bit float deltas (scratch_format 12).  Ring depth NB, parked W^T k-steps PARK and phase-ring depth NBP:
struct Ring8 { int NB, PARK, NBP; };
template <int WD, bool LAST, bool P0, bool D8>
constexpr Ring8 bwd8_ring() {
  static_assert(WD != 256 || !D8 || LAST, "fp8 deltas, width 256, below the last layer: k_bwd8h (launch_bwd8)");
  if (WD != 256) return {8, 0, 0};
  // Ring depths / parked W^T k-steps of the 256-wide 8-wave forms are the combinations hipcc allocates WITHOUT a scratch
  // reload inside the block loop (a reload's vmcnt(0) also waits for every LDS-DMA in flight, i.e. it serialises the loop on
  // HBM latency): DESIGN.md section 4.
  if (!D8) {
    if (LAST) return {8, 0, 0};
    // hidden: 5 delta slots (80 KiB) + 3 phase slots (24) + sines (32) + 2 parked k-steps (16) + sin/cos table (1) = 153 KiB
    // layer 1 (P0, no phase ring): 5 delta slots + sines + 4 parked k-steps + layer-0 table = 148 KiB
    return P0 ? Ring8{5, 4, 0} : Ring8{5, 2, 3};
  }
  // 8 waves (two per SIMD); the ring slots hold the fp8 bytes (8 KiB per block): phase W converts in registers, phase X
  // reads a 16-bit image expanded once per block (2 x 16 KiB).
  // last layer: 3 MFMAs per block, bound by the latency of a step once its delta output is bytes - rings of 4 slots
  // (72 KiB) let two workgroups share a CU (2.30 instead of 2.60 ms per step; with 16-bit deltas the kernel is
  // HBM-bound at 5.4 TB/s and the shallower rings cost 0.3 ms: format 12 keeps one workgroup per CU)
  // (every layer below the last runs k_bwd8h: launch_bwd8)
  return P0 ? Ring8{8, 0, 0} : Ring8{4, 0, 4};
}
template <int WD, bool LAST, bool P0, bool D8>
int launch_bwd8_k(sf_engine* h, const Bwd8Args& a, int n_wg) {
  using T = BwdTile<WD, LAST>;
  constexpr int NB = bwd8_ring<WD, LAST, P0, D8>().NB, PARK = bwd8_ring<WD, LAST, P0, D8>().PARK, NBP = bwd8_ring<WD, LAST, P0, D8>().NBP;
  constexpr size_t lds = bwd8_lds_bytes<T::JW, T::IW, T::WR * T::WC, LAST, P0, NB, PARK, NBP, D8>();
  static_assert(lds <= 160 * 1024, "k_bwd8 LDS budget");
  return launch(h, k_bwd8<T::JW, T::IW, T::WR, T::WC, LAST, P0, OpF16, NB, PARK, NBP, D8>, n_wg, T::WR * T::WC * 64, lds, a);
}
int launch_bwd8h(sf_engine* h, const Bwd8Args& a, int n_wg) {
  constexpr size_t lds = bwd8h_lds_bytes<kBwd8hPark>();
  static_assert(lds <= 160 * 1024, "k_bwd8h LDS budget");
  return launch(h, k_bwd8h<kBwd8hPark>, n_wg, 512, lds, a);
}
int launch_bwd8(sf_engine* h, bool last, bool p0, const Bwd8Args& a, int n_wg) {
  return with_width(h, [&](auto wd) {
    return with_bool(last, p0, [&](auto l, auto p) {
      return with_bool(h->d8, [&](auto d) {
        constexpr int WD = decltype(wd)::value;
        constexpr bool LAST = decltype(l)::value, P0 = decltype(p)::value, D8 = decltype(d)::value;
        // fp8 deltas at width 256, every layer below the last: the slot-per-MFMA pipeline (siren_s8h.hip).  The forward of such
        // a layer is k_fwd_pipe, which spills layer 0's phase bytes too, so run_pass never asks for the P0 form here.
        if constexpr (WD == 256 && !LAST && D8) return P0 ? fail(SF_ERR_INVALID, "launch_bwd8: no P0 form below the last layer") : launch_bwd8h(h, a, n_wg);
        else return launch_bwd8_k<WD, LAST, P0, D8>(h, a, n_wg);
      });
    });
  });
}

// weight gradient of layer 0 (no data gradient needed): contraction of delta_0 with the coordinates
template <int JW>
int launch_dw0(sf_engine* h, const Dw0Args& a, int n_wg) {
  const size_t lds = (size_t)8 * (JW / 16) * 1024 + 512;   // ring + coordinate table
  return with_op(h, [&](auto op) { return launch(h, k_dw0<JW, decltype(op)>, n_wg, JW * 2, lds, a); });
}
// ... from fp8 deltas: two MFMAs per wave and block behind a workgroup barrier: bound by the latency of a step.  At width
// 256 a 4-slot ring (64.5 KiB) lets two workgroups share a CU.
constexpr int dw0_8_ring(int JW) { return JW == 256 ? 4 : 8; }
template <int JW>
int launch_dw0_8(sf_engine* h, const Dw0Args& a, int n_wg) {
  constexpr int NB = dw0_8_ring(JW);
  const size_t lds = (size_t)(NB * (JW / 32) + 2 * (JW / 16)) * 1024 + 512;   // byte ring + two fp16 images + coordinate table
  return launch(h, k_dw0_8<JW, OpF16, NB>, n_wg, JW * 2, lds, a);
}
template <int JW>
int launch_dw_first_t(sf_engine* h, const Dw0Args& a, int n_wg) {
  return h->d8 ? launch_dw0_8<JW>(h, a, n_wg) : launch_dw0<JW>(h, a, n_wg);
}
int launch_dw_first(sf_engine* h, const Dw0Args& a, int n_wg) {
  return with_width(h, [&](auto wd) { return launch_dw_first_t<decltype(wd)::value>(h, a, n_wg); });
}
// the fixed-order slab reduction of one layer's weight and bias gradient into the flat gradient
int launch_reduce(sf_engine* h, const ReduceArgs& ra) {
  return launch(h, k_reduce, (ra.rows_out * ra.cols_out + ra.rows_out + 15) / 16, 256, 0, ra);
}

// WaveletSiren: the sub-handles launch on the handle's current stream (graph capture swaps it) and report to its profiler
void wv_sync(sf_engine* h) {
  for (sf_engine* s : h->wv_sub) {
    s->stream = h->stream;
    s->prof = h->prof;
    s->replay = h->replay;
  }
}

// algorithmic GEMM FLOPs per pixel: forward 2*P_w, backward 4*P_w - 4*WD
double flops_fwd_px(const sf_engine* h) {
  const double W = h->WD;
  return 2.0 * (2 * W + (h->D - 2) * W * W + h->cfg.out_features * W);
}
// ---------------------------------------------------------------------------------------------------------
// wide path (hidden 512 / 1024): layer-at-a-time kernels of siren_wide.hip
// ---------------------------------------------------------------------------------------------------------
int refresh_images_wide(sf_engine* h) {
  if (!h->images_dirty) return SF_OK;
  const int WD = h->WD, D = h->D, NBLK = WD / 256, KS = WD / 16;
  const bool f16 = h->cfg.compute_dtype == SF_F16;
  Launch L(h, K_IMAGES, 0, (double)(D - 2) * WD * WD * 8.0);
  {
    WTabArgs t;
    memset(&t, 0, sizeof(t));
    t.params = h->params; t.depth = D; t.WD = WD; t.out_features = h->cfg.out_features;
    t.off_w0 = h->off_w[0]; t.off_b0 = h->off_b[0];
    for (int l = 0; l < D; ++l) t.off_b[l] = h->off_b[l];
    t.wscale = h->wscale; t.hscale = (float)((double)h->cfg.hidden_omega_0 / kTwoPi);
    t.l0tab = h->l0tab; t.bias = h->biasw;
    long n = (long)(D - 2) * WD;
    if (n < WD) n = WD;
    SF_TRY(launch(h, k_wtables, (n + 255) / 256, 256, 0, t));
  }
  if (h->d8 && h->lsc) SF_TRY(launch_fp8_scales(h));   // per-layer fp8 delta scales, as at width <= 256
  auto image = [&](int l, bool transpose, int OT, int n_ob, int n_chunk, float scale, uint16_t* dst) {
    WImgArgs a;
    memset(&a, 0, sizeof(a));
    a.link = (transpose && h->d8 && h->lsc) ? h->lsc + l : nullptr;
    a.W = h->params + h->off_w[l];
    a.rows = l == D - 1 ? h->cfg.out_features : WD; a.cols = WD;
    a.transpose = transpose; a.OT = OT; a.n_ob = n_ob; a.n_chunk = n_chunk; a.scale = scale; a.f16 = f16; a.dst = dst;
    const long total = (long)n_ob * n_chunk * OT * 4 * 512;
    return launch(h, k_wimage, (total + 255) / 256, 256, 0, a);
  };
  for (int l = 1; l <= D - 2; ++l) {
    SF_TRY(image(l, false, 8, NBLK, KS / 4, (float)((double)h->cfg.hidden_omega_0 / kTwoPi), h->wf + (size_t)(l - 1) * WD * WD));
    SF_TRY(image(l, true, 8, NBLK, KS / 4, l - 1 == 0 ? h->cfg.first_omega_0 : h->cfg.hidden_omega_0, h->wb + (size_t)(l - 1) * WD * WD));
  }
  SF_TRY(image(D - 1, false, 1, 1, KS / 4, h->wscale, h->wf_last));
  SF_TRY(image(D - 1, true, 8, NBLK, 1, D - 2 == 0 ? h->cfg.first_omega_0 : h->cfg.hidden_omega_0, h->wb_last));
  h->images_dirty = false;
  return SF_OK;
}

// persistent grid of the wide GEMMs: one workgroup per CU, a multiple of 8 * n_ob (so XCD and output block are loop
// invariants), at most one workgroup per tile
unsigned wgemm_grid(const sf_engine* h, int n_ob, unsigned tiles) {
  const unsigned pg = (unsigned)(h->dw_wg / (8 * n_ob) * (8 * n_ob));
  return pg == 0 || pg > tiles ? tiles : pg;
}
template <int MODE>
int launch_wgemm(sf_engine* h, const WGemmArgs& a, int n_super, int n_ob) {
  WGemmArgs b = a;
  b.n_super = n_super; b.n_ob = n_ob;
  const unsigned grid = (unsigned)((n_super + 7) / 8 * 8 * n_ob);
  if constexpr (MODE == 1) {
    return with_op(h, [&](auto op) { return launch(h, k_wgemm<1, decltype(op)>, grid, 512, (size_t)4 * 4 * 1024 + 64, b); });
  } else {
    if constexpr (MODE == 2) {
      if (h->d8) {   // fp8 deltas (format 8): out always, in for every launch below the last layer's
        const size_t lds8 = (size_t)4 * 32 * 1024;
        const unsigned pg8 = wgemm_grid(h, n_ob, grid);
        return a.fscale ? launch(h, k_wgemm2<2, OpF16, true, false, true>, pg8, 512, lds8, b)
                        : launch(h, k_wgemm2<2, OpF16, true, true, true>, pg8, 512, lds8, b);
      }
    }
    const size_t lds = (size_t)4 * 32 * 1024;
    const unsigned pgrid = wgemm_grid(h, n_ob, grid);    // persistent: one workgroup per CU
    if (h->s8 && (MODE == 0 || b.Pprev))                    // phase bytes (format 12; fp16 only: sf_create)
      return launch(h, k_wgemm2<MODE, OpF16, true>, pgrid, 512, lds, b);
    return with_op(h, [&](auto op) { return launch(h, k_wgemm2<MODE, decltype(op)>, pgrid, 512, lds, b); });
  }
}
int run_pass_wide(sf_engine* h, bool train, float* pred, bool want_sse) {
  SF_TRY(refresh_images_wide(h));
  const int WD = h->WD, D = h->D, KS = WD / 16, NBLK = WD / 256;
  const bool f16 = h->cfg.compute_dtype == SF_F16;
  const float sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
  const float sc_hidden = (float)((double)h->cfg.hidden_omega_0 / kTwoPi / (double)h->wscale);
  const size_t blk_pieces = (size_t)(KS / 4) * 32;   // pieces of one [256 x WD] block of a hidden image
  long sse_off = 0;
  for (long c = 0; c < n_chunks(h->npix, h->chunk_px); ++c) {
    const Chunk k = chunk_at(c, h->npix, h->chunk_px);
    const int n_super = k.n_super;
    const long n_pb = k.n_pb;
    const double npx = n_pb * 32.0;
    // ---- forward ----
    {
      WL0Args a;
      memset(&a, 0, sizeof(a));
      a.gh = h->gh; a.gw = h->gw; a.W = h->cfg.width; a.row_begin = h->cfg.row_begin; a.pix0 = k.pix0; a.npix = h->npix;
      a.l0tab = h->l0tab; a.sc_first = sc_first; a.KS = KS; a.n_pieces = n_pb * KS; a.P = h->Pbuf; a.Act = h->Abuf;
      Launch L(h, K_FWD, 4.0 * WD * npx, npx * (WD * (h->s8 ? 3.0 : 4.0)));
      if (h->s8) SF_TRY(launch(h, k_wlayer0<OpF16, true>, (a.n_pieces / 2 + 3) / 4, 256, 0, a));
      else SF_TRY(with_op(h, [&](auto op) { return launch(h, k_wlayer0<decltype(op)>, (a.n_pieces + 3) / 4, 256, 0, a); }));
    }
    for (int l = 1; l <= D - 2; ++l) {
      WGemmArgs a;
      memset(&a, 0, sizeof(a));
      a.A = reinterpret_cast<const u32x4*>(h->wf + (size_t)(l - 1) * WD * WD);
      a.a_block_pieces = (long)blk_pieces; a.n_chunk = KS / 4;
      a.Bin = h->Abuf + (size_t)(l - 1) * h->a_stride; a.ks_in = KS;
      a.bias = h->biasw + (size_t)(l - 1) * WD; a.sc = sc_hidden;
      a.Out = h->Pbuf + (size_t)l * h->p_stride; a.OutAct = h->Abuf + (size_t)l * h->a_stride; a.ks_out = KS; a.kp_out = WD / 32;
      Launch L(h, K_FWD, 2.0 * WD * WD * npx, npx * (WD * ((h->s8 ? 3.0 : 4.0) + 2.0 * NBLK)));
      SF_TRY(launch_wgemm<0>(h, a, n_super, NBLK));
    }
    {
      WGemmArgs a;
      memset(&a, 0, sizeof(a));
      a.A = reinterpret_cast<const u32x4*>(h->wf_last);
      a.a_block_pieces = (long)KS; a.n_chunk = KS / 4;
      a.Bin = h->Abuf + (size_t)(D - 2) * h->a_stride; a.ks_in = KS;
      a.bias = h->biasw + (size_t)(D - 2) * WD; a.sc = 1.0f / h->wscale;
      a.img = h->img; a.pred = pred; a.nout = h->cfg.out_features;
      a.gscale = gscale(h);
      a.sse_part = h->sse_part + sse_off; a.Dlast = train ? h->Dlast : nullptr; a.pix0 = k.pix0; a.npix = h->npix;
      if (!h->cfg.outermost_linear) { a.last_om = h->cfg.hidden_omega_0; a.last_om_rev = (float)((double)h->cfg.hidden_omega_0 / kTwoPi); }
      sse_off += n_super;
      Launch L(h, K_FWD, 2.0 * h->cfg.out_features * WD * npx, npx * (WD * 2.0 + 12.0 + 64.0));
      SF_TRY(launch_wgemm<1>(h, a, n_super, 1));
    }
    if (!train) continue;
    // ---- backward ----
    const int n_wg = (int)(n_pb < (long)h->dw_wg ? n_pb : (long)h->dw_wg);
    if (h->d8)   // fp8 deltas: this chunk's power-of-two factor from its own residual
      SF_TRY(launch(h, k_wchunk_scale, 1, 256, 0, h->sse_part + sse_off - n_super, n_super,
                    1.0 / ((double)h->cfg.out_features * (double)k.px), gscale(h), h->gpre, kFp8Target, h->scale_dev));
    for (int l = D - 1; l >= 1; --l) {
      const bool last = l == D - 1;
      const bool dl8 = h->d8 && !last;                      // this layer's incoming deltas are fp8 byte pieces
      const u32x4* Dl = last ? h->Dlast : h->Dbuf + (size_t)l * h->d_stride;
      const u32x4* Pprev = h->Pbuf + (size_t)(l - 1) * h->p_stride;
      const double rows = last ? h->cfg.out_features : WD;
      {   // weight gradient: every [256 x 256] (last layer: [32 x 256]) block in one launch, blockIdx.y = block
        const int nby = (last ? 1 : NBLK) * NBLK;
        int gx = h->dw_wg / nby / 8 * 8;            // multiple of 8: same-pixel workgroups share an XCD
        if (gx < 8) gx = 8;
        if ((long)gx > n_pb) gx = (int)n_pb;
        WDwArgs a;
        memset(&a, 0, sizeof(a));
        a.D = Dl; a.ksd_total = last ? 2 : (dl8 ? WD / 32 : KS); a.P = h->Abuf + (size_t)(l - 1) * h->a_stride; a.ksp_total = KS; a.nblk_i = NBLK;
        a.n_pb = n_pb; a.slab = h->slab;
        {
          Launch L(h, last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * rows * WD * npx, npx * ((last ? 64.0 : WD * 2.0) + WD * 2.0));
          const dim3 grid(gx, nby);
          const size_t lds = (size_t)4 * ((last ? 2 : 16) + 16) * 1024;
          if (dl8) SF_TRY(launch(h, k_wdw<256, OpF16, true>, grid, 512, (size_t)4 * (8 + 16) * 1024, a));
          else SF_TRY(with_op(h, [&](auto op) {
            using OP = decltype(op);
            return last ? launch(h, k_wdw<32, OP>, grid, 512, lds, a) : launch(h, k_wdw<256, OP>, grid, 512, lds, a);
          }));
        }
        WReduceArgs r;
        memset(&r, 0, sizeof(r));
        r.slab = h->slab; r.n_wg = gx; r.slab_rows = last ? 32 : 256; r.rows_out = last ? h->cfg.out_features : 256;
        r.nblk_i = NBLK; r.gW = h->grads + h->off_w[l]; r.ldw = WD; r.gb = h->grads + h->off_b[l];
        r.accumulate = c > 0; r.scale = 1.0f / h->gpre;
        if (dl8) { r.s1 = h->scale_dev; r.s2 = h->lsc + 16 + l; }
        const int n = r.rows_out * 256 + r.rows_out;
        Launch L(h, K_REDUCE, 0, (double)gx * nby * n * 4.0);
        SF_TRY(launch(h, k_wreduce, dim3((n + 255) / 256, nby), 256, 0, r));
      }
      // data gradient: delta_{l-1} = (delta_l W_l) * omega cos(P_{l-1})
      WGemmArgs a;
      memset(&a, 0, sizeof(a));
      a.A = last ? reinterpret_cast<const u32x4*>(h->wb_last) : reinterpret_cast<const u32x4*>(h->wb + (size_t)(l - 1) * WD * WD);
      a.a_block_pieces = last ? 32 : (long)blk_pieces; a.n_chunk = last ? 1 : KS / 4;
      a.Bin = Dl; a.ks_in = last ? 2 : KS;
      a.Out = h->Dbuf + (size_t)(l - 1) * h->d_stride; a.ks_out = KS; a.kp_out = WD / 32; a.Pprev = Pprev;
      a.fscale = (h->d8 && last) ? h->scale_dev : nullptr;
      Launch L(h, last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * rows * WD * npx,
               npx * ((last ? 64.0 : WD * 2.0 * NBLK) + WD * (h->s8 ? 3.0 : 4.0)));
      SF_TRY(launch_wgemm<2>(h, a, n_super, NBLK));
    }
    for (int jb = 0; jb < NBLK; ++jb) {   // layer 0: contraction of delta_0 with the coordinates
      Dw0Args da;
      memset(&da, 0, sizeof(da));
      fill_grid(h, k.pix0, da);
      da.D = h->Dbuf; da.ks_total = KS; da.ks_off = 16 * jb; da.n_pb = n_pb; da.slab = h->slab;
      {
        Launch L(h, K_DW_FIRST, 4.0 * 256 * npx, (h->d8 ? 256.0 : 512.0) * npx);
        SF_TRY(launch_dw_first_t<256>(h, da, n_wg));
      }
      ReduceArgs ra;
      memset(&ra, 0, sizeof(ra));
      ra.slab = h->slab; ra.n_wg = n_wg; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre; ra.scale_dev = nullptr;
      if (h->d8) { ra.scale_dev = h->scale_dev; ra.scale2_dev = h->lsc + 16; }     // 1 / (chunk factor * gpre), 1 / cumulative layer scale
      ra.gW = h->grads + h->off_w[0] + 512 * jb; ra.gb = h->grads + h->off_b[0] + 256 * jb;
      ra.slab_rows = 256; ra.slab_cols = 32; ra.rows_out = 256; ra.cols_out = 2; ra.mode = 1;
      Launch L(h, K_REDUCE, 0, (double)n_wg * (256 * 3) * 4.0);
      SF_TRY(launch_reduce(h, ra));
    }
  }
  if (want_sse || train) SF_TRY(launch_sse_reduce(h, sse_off));
  return SF_OK;
}

// ---------------------------------------------------------------------------------------------------------
// FourierNet (fourier_kernels.hip): per chunk k_ff_fwd -> k_ff_bwd -> k_ff_dw per layer, each followed by the
// fixed-order slab reduction into the flat gradient; Adam, graph replay and the rest are shared with SIREN
// ---------------------------------------------------------------------------------------------------------
int refresh_images_fourier(sf_engine* h) {
  FfImgArgs a;
  memset(&a, 0, sizeof(a));
  a.params = h->params; a.nlin = h->D; a.img = h->ffimg;
  for (int l = 0; l < h->D; ++l) {
    a.off_w[l] = h->off_w[l];
    a.in[l] = l == 0 ? h->MS : h->WD;
    a.out[l] = l == h->D - 1 ? h->cfg.out_features : h->WD;
    // segments in memory order: f0, (b0: empty), f1, b1, f2, b2, ...
    a.start[2 * l] = h->ff_img_f[l];
    a.start[2 * l + 1] = l == 0 ? h->ff_img_f[1] : h->ff_img_b[l];
  }
  a.start[2 * h->D] = h->ff_img_n;
  Launch L(h, K_IMAGES, 0, (double)h->ff_img_n * 16.0);
  SF_TRY(launch(h, k_ff_images, (h->ff_img_n + 255) / 256, 256, 0, a));
  h->images_dirty = false;
  return SF_OK;
}

// the weight images of any handle follow its parameters
int refresh_images(sf_engine* h) {
  if (!h->images_dirty) return SF_OK;
  if (h->wide) return refresh_images_wide(h);
  if (h->fourier) return refresh_images_fourier(h);
  if (h->wavelet) {   // the joint parameters changed: both sub-networks' weight images follow
    wv_sync(h);
    for (sf_engine* s : h->wv_sub) {
      s->images_dirty = true;
      SF_TRY(refresh_images(s));
    }
    h->images_dirty = false;
    return SF_OK;
  }
  ImgArgs a;
  memset(&a, 0, sizeof(a));
  a.params = h->params;
  a.depth = h->D;
  a.WD = h->WD;
  a.out_features = h->cfg.out_features;
  for (int l = 0; l < h->D; ++l) {
    a.off_w[l] = h->off_w[l];
    a.off_b[l] = h->off_b[l];
  }
  a.wscale = h->wscale;
  a.hscale = (float)((double)h->cfg.hidden_omega_0 / kTwoPi);
  a.om_first = h->cfg.first_omega_0; a.om_hidden = h->cfg.hidden_omega_0;
  a.fwd_is_f16 = h->cfg.compute_dtype == SF_F16;
  a.wf = h->wf; a.wf_last = h->wf_last; a.wb = h->wb; a.wb_last = h->wb_last;
  a.l0tab = h->l0tab;
  a.l0img = h->l0img; a.sc_first = (float)((double)h->cfg.first_omega_0 / kTwoPi);
  long n = (long)(h->D - 2) * h->WD * h->WD;
  const long n_min = (long)h->WD / 16 * 64 * 8;  // also covers the small tables
  if (n < n_min) n = n_min;
  if (n < 1024) n = 1024;
  Launch L(h, K_IMAGES, 0, (double)n * 8);
  if (h->d8 && h->lsc) {   // per-layer delta scales first: k_images folds them into the backward images
    SF_TRY(launch_fp8_scales(h));
    a.link = h->lsc;
  }
  SF_TRY(launch(h, k_images, (n + 255) / 256, 256, 0, a));
  h->images_dirty = false;
  return SF_OK;
}

// what every kernel of the FourierNet chain is given for the chunk at pixel pix0: coordinates, encoding, weight images,
// biases; the caller adds its planes and outputs (the RENDER form of k_ff_fwd touches none of H / G / Z / tgt / sse_part)
FfArgs ff_args_base(const sf_engine* h, long pix0) {
  FfArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.gh = h->gh; fa.gw = h->gw; fa.W = h->cfg.width; fa.pix0 = pix0; fa.npix = h->npix; fa.cp = h->chunk_px;
  fa.Btab = h->ffB; fa.MS = h->MS; fa.nlin = h->D; fa.img = h->ffimg; fa.params = h->params;
  for (int l = 0; l < h->D; ++l) { fa.img_f[l] = h->ff_img_f[l]; fa.img_b[l] = h->ff_img_b[l]; fa.off_b[l] = h->off_b[l]; }
  return fa;
}
// k_ff_fwd<WD, false>, k_ff_fwd<WD, true>, k_ff_bwd<WD>, k_ff_fwd<WD, false, true>, k_ff_fwd<WD, false, true, 16>
enum FfKernel { kFfEval, kFfTrain, kFfBwd, kFfRender, kFfRender16 };
int launch_ff(sf_engine* h, const FfArgs& a, int n_super, FfKernel which) {
  return with_width(h, [&](auto wd) {
    constexpr int WD = decltype(wd)::value;
    auto go = [&](auto kernel) { return launch(h, kernel, n_super, kFfThreads, kFfLdsBytes, a); };
    return which == kFfEval ? go(k_ff_fwd<WD, false>) : which == kFfTrain ? go(k_ff_fwd<WD, true>)
           : which == kFfBwd ? go(k_ff_bwd<WD>) : which == kFfRender ? go(k_ff_fwd<WD, false, true>)
                             : go(k_ff_fwd<WD, false, true, 16>);
  });
}

int run_pass_fourier(sf_engine* h, bool train, float* pred, bool want_sse) {
  if (!h->have_B) return fail(SF_ERR_STATE, "sf_set_encoding has not been called");
  SF_TRY(refresh_images(h));
  const int WD = h->WD, D = h->D, MS = h->MS;
  long sse_off = 0;
  for (long c = 0; c < n_chunks(h->npix, h->chunk_px); ++c) {
    const Chunk k = chunk_at(c, h->npix, h->chunk_px);
    const int n_super = k.n_super;
    const double npx = (double)n_super * kSuper;
    FfArgs fa = ff_args_base(h, k.pix0);
    fa.H = h->ffH; fa.G = h->ffG; fa.Z = h->ffZ;
    fa.tgt = h->img; fa.pred = pred; fa.sse_part = h->sse_part + sse_off;
    fa.gscale = gscale(h);
    sse_off += n_super;
    const double f_hidden = (double)(D - 2) * WD * WD;
    {
      Launch L(h, K_FWD, 2.0 * ((double)MS * WD + f_hidden + 32.0 * WD) * npx,
               npx * (12.0 + (train ? (D - 1) * WD * 2.0 + 6.0 : 0.0)));
      SF_TRY(launch_ff(h, fa, n_super, train ? kFfTrain : kFfEval));
    }
    if (!train) continue;
    {
      Launch L(h, K_BWD_HIDDEN, 2.0 * (f_hidden + 16.0 * WD) * npx, npx * (6.0 + (D - 1) * WD * 4.0));
      SF_TRY(launch_ff(h, fa, n_super, kFfBwd));
    }
    // weight gradients, last layer first: per-workgroup slabs over contiguous pixel ranges, then k_reduce*
    int gx = (int)(npx / kSuper);
    if (gx > h->ff_dw_wgs) gx = h->ff_dw_wgs;
    long ppw = ((long)npx + gx - 1) / gx;
    ppw = (ppw + 15) / 16 * 16;
    gx = (int)(((long)npx + ppw - 1) / ppw);
    for (int l = D - 1; l >= 0; --l) {
      const bool last = l == D - 1;
      FfDwArgs da;
      memset(&da, 0, sizeof(da));
      da.rows = last ? h->cfg.out_features : WD;
      da.A = last ? h->ffZ : h->ffG + (size_t)l * WD * h->chunk_px;
      da.Bm = l == 0 ? nullptr : h->ffH + (size_t)(l - 1) * WD * h->chunk_px;
      da.in = l == 0 ? MS : WD;
      da.n_it = da.in / 32;
      const int NI = da.n_it < 4 ? da.n_it : 4;
      da.n_groups = ((da.rows + 31) / 32) * (da.n_it / NI);
      da.cp = h->chunk_px; da.n_px = (long)npx; da.ppw = ppw; da.slab = h->slab; da.e = fa;
      {
        Launch L(h, l == 0 ? K_DW_FIRST : last ? K_BWD_LAST : K_BWD_HIDDEN, 2.0 * 32.0 * ((da.rows + 31) / 32) * da.in * npx,
                 npx * 2.0 * (32.0 * ((da.rows + 31) / 32) + (l == 0 ? 0.0 : da.in)));
        const dim3 grid(gx, (da.n_groups + 3) / 4);
        SF_TRY(with_bool(l == 0, [&](auto e0) {
          constexpr bool E0 = decltype(e0)::value;
          return NI == 1 ? launch(h, k_ff_dw<1, E0>, grid, 256, 0, da) : NI == 2 ? launch(h, k_ff_dw<2, E0>, grid, 256, 0, da)
                                                                                 : launch(h, k_ff_dw<4, E0>, grid, 256, 0, da);
        }));
      }
      const long n = (long)da.rows * da.in + da.rows;
      Launch L(h, K_REDUCE, 0, (double)gx * n * 4.0);
      if (!last) {   // slab layout [W rows*in | b rows] == flat gradient layout of the layer
        const int n4 = (int)(n / 4);
        SF_TRY(launch(h, k_reduce_vec, (n4 + 7) / 8, 256, 0, h->slab, gx, n, n4, h->grads + h->off_w[l], c > 0, 1.0f / h->gpre,
                      nullptr, nullptr));
      } else {
        ReduceArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.slab = h->slab; ra.n_wg = gx; ra.slab_rows = da.rows; ra.slab_cols = da.in; ra.rows_out = da.rows; ra.cols_out = da.in;
        ra.mode = 0; ra.gW = h->grads + h->off_w[l]; ra.gb = h->grads + h->off_b[l]; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre;
        SF_TRY(launch_reduce(h, ra));
      }
    }
  }
  if (want_sse || train) SF_TRY(launch_sse_reduce(h, sse_off));
  return SF_OK;
}

int run_pass_wavelet(sf_engine* h, bool train, float* pred, bool want_sse);
// phases (WaveletSiren sub-handles only; every other pass runs both): bit 0 the forward of each chunk, bit 1 the backward;
// chunks [c_begin, c_end) (c_end < 0: to the last)
enum { kPassFwd = 1, kPassBwd = 2, kPassAll = 3 };
int run_pass(sf_engine* h, bool train, float* pred, bool want_sse, int phases = kPassAll, long c_begin = 0,
             long c_end = -1) {
  if (h->render) return fail(SF_ERR_INVALID, "a render handle (sf_render_create) runs sf_render only");
  if (train) h->fth_fresh = false;
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  if (((train && !h->ext_dout) || want_sse) && !h->img) return fail(SF_ERR_STATE, "sf_set_target has not been called");
  if (h->wavelet) return run_pass_wavelet(h, train, pred, want_sse);
  if (h->fourier) return run_pass_fourier(h, train, pred, want_sse);
  if (train && (!h->Pbuf || !h->Dbuf)) return fail(SF_ERR_STATE, "the handle has no backward scratch");   // (never a null store on the GPU)
  if (h->wide) return run_pass_wide(h, train, pred, want_sse);
  SF_TRY(refresh_images(h));
  const int WD = h->WD, D = h->D;
  long sse_off = 0;
  for (long c = c_begin; c < (c_end < 0 ? n_chunks(h->npix, h->chunk_px) : c_end); ++c) {
    const Chunk k = chunk_at(c, h->npix, h->chunk_px);
    const long n_pb = k.n_pb;
    const double npx = n_pb * 32.0;
    FwdArgs fa = fwd_args_base(h, k.pix0, k.n_super);
    fa.P = h->Pbuf; fa.p_stride = h->p_stride; fa.Dlast = h->Dlast;
    fa.dfac = train ? h->dfac_out : nullptr;
    fa.img = h->img;
    fa.gscale = h->d8 ? kResScale : gscale(h);
    fa.pred = pred;
    fa.sse_part = h->sse_part + sse_off;
    const int n_fwd_wg = fwd_grid(h, k.n_super);
    sse_off += n_fwd_wg;
    if (phases & kPassFwd) {
      Launch L(h, K_FWD, flops_fwd_px(h) * npx,
               npx * (4.0 * h->cfg.out_features + (train ? (D - 2) * WD * (h->s8 ? 1.0 : 2.0) + (h->s8 ? 32.0 : 64.0) : 0.0)));
      SF_TRY(launch_fwd(h, fa, n_fwd_wg, train));
    }
    if (!train || !(phases & kPassBwd)) continue;
    // backward, last layer first; every layer kernel is followed by the fixed-order slab reduction
    const int PBS = 2;   // k_dw stages two pixel blocks at a time; k_bwd accepts any block count
    int n_wg = (int)((n_pb + PBS - 1) / PBS);
    if (n_wg > h->dw_wg) n_wg = h->dw_wg;
    long pb_per_wg = (n_pb + n_wg - 1) / n_wg;
    pb_per_wg = (pb_per_wg + PBS - 1) / PBS * PBS;
    n_wg = (int)((n_pb + pb_per_wg - 1) / pb_per_wg);
    const size_t img_pieces = (size_t)WD * WD / 8;
    // what Bwd8Args and BwdLayerArgs share for layer l >= 1: deltas in and out, phases of the layer below, the backward image
    auto fill_layer = [&](auto& ba, int l) {
      const bool last = l == D - 1;
      memset(&ba, 0, sizeof(ba));
      fill_grid(h, k.pix0, ba);
      ba.D = last ? h->Dlast : h->Dbuf + (size_t)l * h->d_stride;
      ba.P = h->Pbuf + (size_t)(l - 1) * h->p_stride;
      ba.Dout = h->Dbuf + (size_t)(l - 1) * h->d_stride;
      ba.wb = last ? reinterpret_cast<const u32x4*>(h->wb_last)
                   : reinterpret_cast<const u32x4*>(h->wb) + (size_t)(l - 1) * img_pieces;
      ba.n_pb = n_pb; ba.slab = h->slab; ba.l0tab = h->l0tab; ba.sc_first = fa.sc_first;
    };
    for (int l = D - 1; l >= 0; --l) {
      const bool last = l == D - 1;
      const double rows = last ? h->cfg.out_features : WD;
      ReduceArgs ra;
      memset(&ra, 0, sizeof(ra));
      ra.slab = h->slab; ra.n_wg = n_wg; ra.accumulate = c > 0; ra.scale = 1.0f / h->gpre;
      if (h->d8) {   // last layer: dW from the statically scaled residual; layers below: the chunk's adaptive pre-scale
        ra.scale = (float)(1.0 / ((double)kResScale * (double)h->cfg.out_features * h->n_total));
        ra.scale_dev = last ? nullptr : h->scale_dev;
        ra.scale2_dev = (last || !h->lsc) ? nullptr : h->lsc + 16 + l;
      }
      ra.gW = h->grads + h->off_w[l]; ra.gb = h->grads + h->off_b[l];
      // a layer above 0: rows x WD weight gradient from slabs of (last: 32, else WD) rows
      ra.slab_rows = last ? 32 : WD; ra.slab_cols = WD; ra.rows_out = (int)rows; ra.cols_out = WD; ra.mode = 0;
      if (l > 0 && h->s8) {
        // layer 1: with fp8 deltas at width 256 the pipeline forward also spills layer 0's phase bytes, so this layer runs the
        // hidden-layer kernel (k_bwd8h) like the others; else the form that re-derives the layer-0 phases from the coordinates
        const bool l0_bytes = h->d8 && WD == 256 && fwd_is_pipe(h), p0 = l - 1 == 0 && !(l0_bytes && !last);
        Bwd8Args ba;
        fill_layer(ba, l);
        ba.sse_part = fa.sse_part; ba.n_part = n_fwd_wg;
        ba.inv_chunk_values = 1.0 / ((double)h->cfg.out_features * (double)k.px);
        ba.n_values = (double)h->cfg.out_features * h->n_total;
        ba.res_scale = kResScale; ba.target = kFp8Target; ba.scale_out = h->scale_dev;
        ba.zeros = reinterpret_cast<const u32x4*>(h->pad8); ba.dump = reinterpret_cast<u32x4*>(h->pad8 + 8192);
        // hidden 256: the last-layer kernel keeps two workgroups per CU (its slab rows are 32 wide: the slab has room)
        if (last && !p0 && WD == 256 && h->d8) ra.n_wg = (int)std::min<long>((n_pb + PBS - 1) / PBS, 2L * h->dw_wg);
        const double db = h->d8 ? 1.0 : 2.0;   // bytes per delta
        Launch L(h, last ? K_BWD_LAST : (p0 ? K_BWD_L1 : K_BWD_HIDDEN), 4.0 * rows * WD * npx,
                 npx * ((last ? 32.0 : WD * db) + WD * db + (p0 ? 0.0 : WD * 1.0)));
        SF_TRY(launch_bwd8(h, last, p0, ba, ra.n_wg));
      } else if (l > 0) {
        const bool p0 = l - 1 == 0;
        BwdLayerArgs ba;
        fill_layer(ba, l);
        ba.pb_per_wg = (int)pb_per_wg;
        Launch L(h, last ? K_BWD_LAST : (p0 ? K_BWD_L1 : K_BWD_HIDDEN), 4.0 * rows * WD * npx,
                 npx * ((last ? 64.0 : WD * 2.0) + WD * (p0 ? 2.0 : 4.0)));
        SF_TRY(launch_bwd(h, last, p0, ba, n_wg));
      } else {
        Dw0Args da;
        memset(&da, 0, sizeof(da));
        fill_grid(h, k.pix0, da);
        da.D = h->Dbuf; da.ks_total = WD / 16; da.ks_off = 0; da.n_pb = n_pb; da.slab = h->slab;
        const long cap0 = (h->d8 && WD == 256) ? 2L * h->dw_wg : (long)h->dw_wg;      // k_dw0_8<256>: two workgroups per CU
        ra.n_wg = (int)(n_pb < cap0 ? n_pb : cap0);
        ra.slab_rows = WD; ra.slab_cols = 32; ra.rows_out = WD; ra.cols_out = 2; ra.mode = 1;
        Launch L(h, K_DW_FIRST, 4.0 * WD * npx, WD * (h->d8 ? 1.0 : 2.0) * npx);
        SF_TRY(launch_dw_first(h, da, ra.n_wg));
      }
      const int n = ra.rows_out * ra.cols_out + ra.rows_out;
      Launch L(h, K_REDUCE, 0, (double)n_wg * n * 4.0);
      if (l > 0 && !last)   // slab layout == flat gradient layout [W | b]
        SF_TRY(launch(h, k_reduce_vec, (n / 4 + 7) / 8, 256, 0, h->slab, n_wg, n, n / 4, h->grads + h->off_w[l], ra.accumulate,
                      ra.scale, ra.scale_dev, ra.scale2_dev));
      else SF_TRY(launch_reduce(h, ra));
    }
  }
  if ((want_sse || train) && !h->ext_dout) SF_TRY(launch_sse_reduce(h, sse_off));
  return SF_OK;
}

// WaveletSiren pass.  One chunk (the coefficient grid fits one sweep of the sub-networks):
//   training forward of LF and HF (no target: phases, predictions, zero dL/dout) -> k_wv_compose -> k_wv_adjoint (dL/dout
//   straight into both Dlast) -> the backward chain of LF, then of HF (slab reductions into each half of the gradient).
// Two passes (more than one chunk): inference forward of both over every chunk -> compose -> adjoint into an fp32 buffer
//   -> per chunk and sub-network: training forward, k_wv_inject, backward.
// Then the fixed-order reduction of the compose partials into the handle's SSE.
int run_pass_wavelet(sf_engine* h, bool train, float* pred, bool want_sse) {
  SF_TRY(refresh_images(h));   // (also points the sub-handles at the current stream)
  wv_sync(h);
  sf_engine* const sub[2] = {h->wv_sub[0], h->wv_sub[1]};
  const long nn = sub[0]->npix, HH = h->npix;
  const bool one = nn <= sub[0]->chunk_px;
  float* const p_sub[2] = {h->wv_pred, h->wv_pred + nn * 3};
  for (int s = 0; s < 2; ++s)
    SF_TRY(train && one ? run_pass(sub[s], true, p_sub[s], false, kPassFwd) : run_pass(sub[s], false, p_sub[s], false));
  WvArgs a;
  memset(&a, 0, sizeof(a));
  a.H = h->cfg.height; a.n = h->wv_n; a.up = h->wv_up;
  a.lf = p_sub[0]; a.hf = p_sub[1];
  a.img = h->img; a.pred = pred; a.g = train ? h->wv_g : nullptr;
  a.sse_part = h->sse_part;
  a.gscale = (float)(2.0 / (3.0 * h->n_total));
  a.dscale = 0.5f * sub[0]->gpre;
  a.dfac_lf = sub[0]->dfac_out; a.dfac_hf = sub[1]->dfac_out;   // (null for a linear output layer)
  auto wv_grid = [](long n) { return (unsigned)((n + kWvThreads - 1) / kWvThreads); };
  const unsigned n_cwg = wv_grid(HH);
  {
    Launch L(h, K_WV_COMPOSE, 0, (double)HH * 4.0 * (3.0 + (a.img ? 3.0 : 0.0) + (pred ? 3.0 : 0.0) + (train ? 3.0 : 0.0)));
    SF_TRY(launch(h, k_wv_compose, n_cwg, kWvThreads, 0, a));
  }
  if (train) {
    if (one) { a.dl_lf = sub[0]->Dlast; a.dl_hf = sub[1]->Dlast; }
    else { a.gl_lf = h->wv_gl; a.gl_hf = h->wv_gl + nn * 3; }
    {
      Launch L(h, K_WV_ADJOINT, 0, (double)nn * (52.0 * 8.0 + (one ? 32.0 : 24.0)));
      SF_TRY(launch(h, k_wv_adjoint, wv_grid(nn), kWvThreads, 0, a));
    }
    if (one) {
      for (int s = 0; s < 2; ++s) SF_TRY(run_pass(sub[s], true, nullptr, false, kPassBwd));
    } else {
      for (long c = 0; c < n_chunks(nn, sub[0]->chunk_px); ++c) {
        const Chunk k = chunk_at(c, nn, sub[0]->chunk_px);
        for (int s = 0; s < 2; ++s) {
          SF_TRY(run_pass(sub[s], true, nullptr, false, kPassFwd, c, c + 1));
          {
            Launch L(h, K_WV_INJECT, 0, (double)k.px * 28.0);
            SF_TRY(launch(h, k_wv_inject, wv_grid(k.px), kWvThreads, 0, h->wv_gl + (size_t)s * nn * 3, sub[s]->dfac_out, k.pix0,
                          k.px, sub[s]->Dlast));
          }
          SF_TRY(run_pass(sub[s], true, nullptr, false, kPassBwd, c, c + 1));
        }
      }
    }
  }
  if (want_sse || train) SF_TRY(launch_sse_reduce(h, n_cwg));
  return SF_OK;
}

int read_sse(sf_engine* h, double* out) {
  HIPCHK(hipMemcpyAsync(out, h->sse_dev, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SF_OK;
}

// Feathermap: V = V1 V2 and W = scaler * V into the engine's flat parameters; the weight images follow at the next
// refresh_images
int feather_materialise(sf_engine* h) {
  const FthArgs& a = h->fth;
  const dim3 grid((unsigned)((a.rows_used + kFthTile - 1) / kFthTile), (unsigned)((a.n + kFthTile - 1) / kFthTile));
  Launch L(h, K_FTH_MAT, 2.0 * a.rows_used * a.n * a.m, 4.0 * (2.0 * a.n * a.m + 2.0 * a.P));
  SF_TRY(launch(h, k_fth_mat, grid, 256, 0, a));
  h->images_dirty = true;
  return SF_OK;
}

// Feathermap adjoint of the engine's dense gradient: dV1, dV2 and dscaler into fth_g (two launches)
int feather_adjoint(sf_engine* h) {
  const FthArgs& a = h->fth;
  {
    Launch L(h, K_FTH_GRAD, 2.0 * a.P, 4.0 * 4.0 * a.P);
    SF_TRY(launch(h, k_fth_grad, a.g_blocks + a.nchunks, 256, 0, a));
  }
  {
    const int t2 = (a.m + kFthTile - 1) / kFthTile * a.t2n;
    Launch L(h, K_FTH_DV, 2.0 * (double)a.n * a.m * (a.n + a.rows_used), 4.0 * ((double)a.n * a.n + 4.0 * a.n * a.m));
    SF_TRY(launch(h, k_fth_dv, a.t1 + t2 + 1, 256, 0, a));
  }
  h->fth_fresh = true;
  return SF_OK;
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
// a handle under construction: an early return (or an exception) destroys it with everything it owns so far
struct HandleDeleter { void operator()(sf_engine* h) const { sf_destroy(h); } };
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
// Adam: all-zero betas / eps mean torch.optim.Adam's defaults; the doubles behind the float betas (shortest_double)
void adam_defaults(sf_engine* h) {
  sf_config& c = h->cfg;
  if (c.beta1 == 0.f && c.beta2 == 0.f && c.eps == 0.f) { c.beta1 = 0.9f; c.beta2 = 0.999f; c.eps = 1e-8f; }
  h->beta1_d = shortest_double(c.beta1);
  h->beta2_d = shortest_double(c.beta2);
}
// the flat fp32 state of a training handle: parameters, gradient and Adam moments (zeroed on the handle's stream), mask
int alloc_train_state(sf_engine* h) {
  const size_t bytes = (size_t)h->P * 4;
  for (float** p : {&h->params, &h->grads, &h->m, &h->v, &h->mask}) SF_TRY(dev_alloc(h, *p, bytes));
  for (float* p : {h->params, h->grads, h->m, h->v}) hipMemsetAsync(p, 0, bytes, h->stream);
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
  SF_TRY(dev_alloc(h, h->sse_part, (size_t)(n_sse + 64) * 4));
  return dev_alloc(h, h->sse_dev, 8);
}
// what the forward reads, on a training and on a render handle alike: the forward weight images (width <= 256; the wide
// path has its own blocked images), the layer-0 table / image and the two coordinate vectors
int alloc_forward_inputs(sf_engine* h) {
  const int WD = h->WD, D = h->D;
  if (!h->wide) {
    SF_TRY(dev_alloc(h, h->wf, (size_t)(D - 2 > 0 ? D - 2 : 1) * FwdGeom(WD).PIECES * 1024));
    SF_TRY(dev_alloc(h, h->wf_last, (size_t)(WD / 16 + 1) * 1024));
  }
  SF_TRY(dev_alloc(h, h->l0tab, (size_t)WD * 16));
  if (WD == 256) SF_TRY(dev_alloc(h, h->l0img, (size_t)(WD / 32) * 1024));
  SF_TRY(dev_alloc(h, h->gh, (size_t)h->cfg.height * 4));
  return dev_alloc(h, h->gw, (size_t)h->cfg.width * 4);
}

}  // namespace

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

// layer strides of the phase / delta scratch for the handle's current format
static void set_scratch_strides(sf_engine* h) {
  const long chunk = h->chunk_px;
  const int WD = h->WD;
  h->p_stride = chunk / 32 * (h->s8 ? WD / 32 : WD / 16) * 64 + 37 * 64;
  h->d_stride = chunk / 32 * (h->d8 ? WD / 32 : WD / 16) * 64 + 37 * 64;
  h->a_stride = chunk / 32 * (WD / 16) * 64 + 37 * 64;
}
// sf_create and sf_render_create (siren_render.hip): one validation, one geometry; a render handle allocates the forward's
// inputs only.  sub_network: the handle is one of the two SIRENs of a WaveletSiren handle, which points params / grads / m /
// v / mask at slices of its own joint vectors - nothing is allocated for them here
static int create_handle(const sf_config* cfg, sf_handle** out, bool render, bool sub_network = false) {
  if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, "abi_version mismatch");
  if (cfg->in_features != 2) return fail(SF_ERR_INVALID, "in_features must be 2 (coordinate grid)");
  if (cfg->out_features < 1 || cfg->out_features > 3) return fail(SF_ERR_INVALID, "out_features must be 1..3");
  if (cfg->depth < 2 || cfg->depth > 16) return fail(SF_ERR_INVALID, "depth must be 2..16");
  if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256 && cfg->hidden != 512 &&
      cfg->hidden != 1024)
    return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128, 256, 512 or 1024 in this build");
  if (cfg->hidden > 256 && cfg->depth < 3) return fail(SF_ERR_INVALID, "hidden > 256 needs depth >= 3");
  if (render && cfg->hidden > 256)
    return fail(SF_ERR_INVALID, "sf_render_create: the render kernel is not built for the wide path (hidden 512 / 1024): "
                                "run the model's own forward on the host side");
  if (cfg->compute_dtype != SF_BF16 && cfg->compute_dtype != SF_F16)
    return fail(SF_ERR_INVALID, "compute_dtype must be SF_BF16 or SF_F16");
  if (cfg->height < 1 || cfg->width < 1) return fail(SF_ERR_INVALID, "bad image size");
  if (cfg->scratch_format != 0 && cfg->scratch_format != 8 && cfg->scratch_format != 12 && cfg->scratch_format != 16)
    return fail(SF_ERR_INVALID, "scratch_format must be 0 (auto), 8, 12 or 16");
  if ((cfg->scratch_format == 8 || cfg->scratch_format == 12) && cfg->compute_dtype != SF_F16)
    return fail(SF_ERR_INVALID, "scratch_format 8 / 12 need compute_dtype SF_F16");
  int r0 = cfg->row_begin, r1 = cfg->row_end;
  if (r0 == 0 && r1 == 0) r1 = cfg->height;
  if (r0 < 0 || r1 > cfg->height || r0 >= r1) return fail(SF_ERR_INVALID, "bad row range");
  // the layer-0 / layer-1 gradient kernels decode (row, col) of a local pixel p as row = (p * ceil(2^40 / W)) >> 40,
  // exact while p * W < 2^40, i.e. local_rows * W^2 < 2^40 (an unsharded 8192 x 8192 grid sits at 2^39)
  if ((double)(r1 - r0) * (double)cfg->width * (double)cfg->width >= 1099511627776.0)
    return fail(SF_ERR_INVALID, "grid too large for one handle: (row_end - row_begin) * width^2 must stay below 2^40 "
                                "(shard the rows over more handles)");
  hipDeviceProp_t prop;
  SF_TRY(check_device(cfg, prop));
  DevGuard dev_guard(cfg->device);   // the caller's current device is restored on return

  HandlePtr owner(new sf_engine());
  sf_engine* h = owner.get();
  h->cfg = *cfg;
  h->cfg.row_begin = r0;
  h->cfg.row_end = r1;
  adam_defaults(h);
  h->D = cfg->depth;
  h->WD = cfg->hidden;
  h->wide = cfg->hidden > 256;
  h->render = render;
  {
    // auto (fp16 operands, hidden <= 256): phase bytes always; fp8 deltas (format 8) when the image has >= 2^20 pixels - a
    // gradient then sums the zero-mean fp8 rounding over >= 10^6 terms (within the 0.05 dB criterion on every reference
    // fixture even at 2^16 pixels) and the backward kernels are bandwidth-bound; smaller fits are
    // launch-latency-bound and keep 16-bit deltas (format 12).  A masked fit is moved to format 16 by sf_set_masks.
    int fmt = cfg->scratch_format;
    h->fmt_auto = fmt == 0;
    const bool mega = (double)cfg->height * (double)cfg->width >= 1048576.0;
    // (wider than 256: the layer-at-a-time kernels take the byte formats where bandwidth matters - from 2^20 pixels; fp8 deltas up to
    // width 512, where a reference-minted fixture at 2^20 pixels pins them (tests/golden/plateau_ns_512x4_1024.npz: -0.0002 dB);
    // phase bytes only above)
    if (fmt == 0) fmt = cfg->compute_dtype != SF_F16 ? 16 : h->wide ? (mega ? (cfg->hidden <= 512 ? 8 : 12) : 16) : (mega ? 8 : 12);
    if (render) { fmt = 16; h->fmt_auto = false; }   // no scratch at all: nothing of the byte formats applies
    h->cfg.scratch_format = fmt;
    h->s8 = fmt == 8 || fmt == 12;
    h->d8 = fmt == 8;
  }
  h->stream = (hipStream_t)cfg->stream;
  h->npix = (long)(r1 - r0) * cfg->width;
  h->n_total = (double)cfg->height * (double)cfg->width;
  // flat parameter offsets: named_parameters() order (siren.py:90-118)
  int64_t off = 0;
  for (int l = 0; l < h->D; ++l) {
    const int in = l == 0 ? 2 : h->WD, outn = l == h->D - 1 ? cfg->out_features : h->WD;
    h->off_w[l] = off; off += (int64_t)in * outn;
    h->off_b[l] = off; off += outn;
  }
  h->P = off;
  // fp16 forward images are scaled by 2^8 so that small weights stay normal numbers
  h->wscale = cfg->compute_dtype == SF_F16 ? 256.0f : 1.0f;
  // fp16 backward operands: dL/dout = resid/(3N) is pre-scaled by 2^k ~ 4*3N so the deltas sit around 1
  // (fp16 normal range 6e-5..65504); every gradient is multiplied back by 2^-k in the slab reduction
  if (cfg->compute_dtype == SF_F16) h->gpre = (float)exp2(ceil(log2((double)cfg->out_features * (double)cfg->height * (double)cfg->width)) + 2.0);
  // chunking
  // default: 4 Mi pixels at width <= 256 (29 GB of scratch at 256x8); the same scratch budget for wider layers
  const long chunk = chunk_pixels(cfg->chunk_pixels > 0 ? cfg->chunk_pixels : (1L << 22) / (h->wide ? cfg->hidden / 256 : 1), h->npix);
  h->chunk_px = chunk;
  const int WD = h->WD, D = h->D;
  // layer stride of the scratch tensors, padded so that the three streams a kernel touches at once are
  // not a power of two apart (HBM channel aliasing)
  // (8-bit scratch: one piece per 32-neuron tile instead of one per 16-neuron k-step)
  set_scratch_strides(h);

  h->dw_wg = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

  if (render) {   // parameters, forward weight images, layer-0 table / image, the two coordinate vectors
    if (!sub_network) {
      SF_TRY(dev_alloc(h, h->params, h->P * 4));
      hipMemsetAsync(h->params, 0, h->P * 4, h->stream);
    }
    SF_TRY(alloc_forward_inputs(h));
    *out = owner.release();
    return SF_OK;
  }
  if (!sub_network) SF_TRY(alloc_train_state(h));
  SF_TRY(alloc_forward_inputs(h));
  const size_t img_elems = (size_t)(D - 2 > 0 ? D - 2 : 1) * WD * WD;
  SF_TRY(dev_alloc(h, h->wb, img_elems * 2));
  if (h->wide) {   // blocked images of siren_wide.hip
    SF_TRY(dev_alloc(h, h->wf, img_elems * 2));
    SF_TRY(dev_alloc(h, h->wf_last, (size_t)(WD / 16) * 1024));
    SF_TRY(dev_alloc(h, h->wb_last, (size_t)(WD / 256) * 32 * 1024));
    SF_TRY(dev_alloc(h, h->biasw, ((size_t)(D - 2) * WD + 32) * 4));
  } else {
    SF_TRY(dev_alloc(h, h->wb_last, (size_t)WD / 32 * 64 * 16));
  }
  SF_TRY(dev_alloc(h, h->Pbuf, (size_t)(D - 1) * h->p_stride * 16));
  SF_TRY(dev_alloc(h, h->Dbuf, (size_t)(D - 1) * h->d_stride * 16));
  if (h->wide) SF_TRY(dev_alloc(h, h->Abuf, (size_t)(D - 1) * h->a_stride * 16));
  SF_TRY(dev_alloc(h, h->Dlast, (size_t)chunk / 32 * 2 * 64 * 16));
  { const size_t sw = WD > 256 ? 256 : WD; SF_TRY(dev_alloc(h, h->slab, (size_t)h->dw_wg * (sw * sw + sw) * 4 + 4096)); }
  SF_TRY(alloc_sse(h, chunked_sse_parts(h)));
  SF_TRY(dev_alloc(h, h->scale_dev, 16));
  SF_TRY(dev_alloc(h, h->pad8, 16384));
  SF_TRY(dev_alloc(h, h->lsc, 32 * 4 + 16 * 8));
  if (hipMemset(h->pad8, 0, 16384) != hipSuccess) return fail(SF_ERR_NOMEM, "hipMemset failed");
  const float sc[2] = {(float)((double)h->gpre / ((double)cfg->out_features * h->n_total)), 1.0f / h->gpre};
  if (hipMemcpy(h->scale_dev, sc, sizeof(sc), hipMemcpyHostToDevice) != hipSuccess) return fail(SF_ERR_HIP, "hipMemcpy(scale) failed");
  *out = owner.release();
  return SF_OK;
}
// ---- WaveletSiren: what sf_wavelet_create and sf_wavelet_render_create (wavelet_render.hip) share ------------------
// the argument checks both creators word identically, in the order both run them
template <typename Config>
static int wavelet_check_network(const Config* cfg) {
  if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256)
    return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128 or 256 for WaveletSiren (other widths: zero-pad on the host)");
  if (cfg->depth < 2 || cfg->depth > 16) return fail(SF_ERR_INVALID, "depth must be 2..16");
  if (cfg->compute_dtype != SF_F16) return fail(SF_ERR_INVALID, "WaveletSiren runs fp16 operands only (compute_dtype SF_F16)");
  return SF_OK;
}
static int wavelet_check_image(int height, int width, int64_t chunk_pixels) {
  if (height != width || height < 2 || height % 2)
    return fail(SF_ERR_INVALID, "WaveletSiren needs an even, square image: the reference's inverse DWT (2n - 4 rows) and its "
                                "torch.cat of Y with the upsampled Cb / Cr stop matching otherwise");
  if ((double)height * (double)width >= 2147483648.0) return fail(SF_ERR_INVALID, "image too large");
  if (chunk_pixels < 0) return fail(SF_ERR_INVALID, "chunk_pixels must be >= 0");
  return SF_OK;
}
// config of the two sub-networks: SIRENs of the creator's shape on a rows x cols coefficient grid, scratch format 16
template <typename Config>
static sf_config wavelet_sub_config(const Config* cfg, int rows, int cols) {
  sf_config sc;
  memset(&sc, 0, sizeof(sc));
  sc.abi_version = SF_ABI_VERSION; sc.height = rows; sc.width = cols; sc.row_begin = 0; sc.row_end = rows;
  sc.in_features = 2; sc.out_features = 3; sc.hidden = cfg->hidden; sc.depth = cfg->depth;
  sc.first_omega_0 = cfg->first_omega_0; sc.hidden_omega_0 = cfg->hidden_omega_0; sc.outermost_linear = cfg->outermost_linear;
  sc.compute_dtype = SF_F16; sc.device = cfg->device; sc.stream = cfg->stream; sc.chunk_pixels = cfg->chunk_pixels;
  sc.scratch_format = 16;
  return sc;
}
// the two sub-networks (LF, HF; their flat state stays unallocated: the creator points it at slices of the joint vectors
// it allocates), then the handle itself with the geometry of an H x H picture
static int wavelet_begin(const sf_config& sc, bool render, int H, HandlePtr& owner) {
  HandlePtr sub[2];
  for (HandlePtr& s : sub) {
    sf_handle* e = nullptr;
    SF_TRY(create_handle(&sc, &e, render, true));   // (render: refuses rows * cols^2 >= 2^40: draw such a picture in bands)
    s.reset(e);
  }
  owner.reset(new sf_engine());
  sf_engine* h = owner.get();
  h->wavelet = true;
  h->render = render;
  h->cfg = sub[0]->cfg;
  h->cfg.height = H; h->cfg.width = H; h->cfg.row_begin = 0; h->cfg.row_end = H;
  h->beta1_d = sub[0]->beta1_d; h->beta2_d = sub[0]->beta2_d;
  h->D = 2 * sc.depth; h->WD = sc.hidden;
  h->dw_wg = sub[0]->dw_wg;
  h->stream = (hipStream_t)sc.stream;
  h->npix = (long)H * H;
  h->n_total = (double)H * (double)H;
  h->wv_n = (H + 5) / 2;   // pywt.dwt_coeff_len(H, 6, "zero")
  h->wv_up = (float)(1.0 / ((double)H / (double)h->wv_n));   // torch: scale_factor = H / n, source scale 1 / scale_factor
  h->P = 2 * sub[0]->P;
  h->wv_sub[0] = sub[0].release(); h->wv_sub[1] = sub[1].release();
  return SF_OK;
}

extern "C" {

int sf_abi_version(void) { return SF_ABI_VERSION; }
const char* sf_last_error(void) { return g_err.c_str(); }

int sf_create(const sf_config* cfg, sf_handle** out) try { return create_handle(cfg, out, false); } SF_CATCH

// FourierNet handle: the same sf_engine, run by fourier_kernels.hip (run_pass_fourier); every other entry point is shared.
// sf_fourier_create and sf_fourier_render_create (fourier_render.hip): one validation, one geometry; a render handle
// allocates the parameters, the weight images (forward and backward: k_ff_images writes both, a few MB at most),
// encoding.B and the two coordinate vectors
static int create_fourier(const sf_fourier_config* cfg, sf_handle** out, bool render) {
  if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, "abi_version mismatch");
  if (cfg->in_features != 2) return fail(SF_ERR_INVALID, "in_features must be 2 (coordinate grid)");
  if (cfg->out_features != 3) return fail(SF_ERR_INVALID, "out_features must be 3 (the fused sigmoid / loss epilogue is RGB)");
  if (cfg->hidden != 32 && cfg->hidden != 64 && cfg->hidden != 128 && cfg->hidden != 256)
    return fail(SF_ERR_INVALID, "hidden must be 32, 64, 128 or 256 for FourierNet (other widths: zero-pad on the host)");
  if (cfg->map_size != 64 && cfg->map_size != 128 && cfg->map_size != 256 && cfg->map_size != 512)
    return fail(SF_ERR_INVALID, "map_size must be 64, 128, 256 or 512");
  if (cfg->n_linear < 2 || cfg->n_linear > kFfMaxLinear) return fail(SF_ERR_INVALID, "n_linear must be 2..12");
  if (cfg->compute_dtype != SF_F16) return fail(SF_ERR_INVALID, "FourierNet runs fp16 operands only (compute_dtype SF_F16)");
  if (cfg->height < 1 || cfg->width < 1) return fail(SF_ERR_INVALID, "bad image size");
  if ((double)cfg->height * (double)cfg->width >= 2147483648.0) return fail(SF_ERR_INVALID, "image too large: height * width must stay below 2^31");
  if (cfg->chunk_pixels < 0) return fail(SF_ERR_INVALID, "chunk_pixels must be >= 0");
  hipDeviceProp_t prop;
  SF_TRY(check_device(cfg, prop));
  DevGuard dev_guard(cfg->device);

  HandlePtr owner(new sf_engine());
  sf_engine* h = owner.get();
  h->fourier = true;
  h->render = render;
  memset(&h->cfg, 0, sizeof(h->cfg));
  h->cfg.abi_version = cfg->abi_version;
  h->cfg.height = cfg->height; h->cfg.width = cfg->width; h->cfg.row_begin = 0; h->cfg.row_end = cfg->height;
  h->cfg.in_features = cfg->in_features; h->cfg.out_features = cfg->out_features; h->cfg.hidden = cfg->hidden;
  h->cfg.depth = cfg->n_linear; h->cfg.compute_dtype = cfg->compute_dtype;
  h->cfg.beta1 = cfg->beta1; h->cfg.beta2 = cfg->beta2; h->cfg.eps = cfg->eps;
  h->cfg.device = cfg->device; h->cfg.stream = cfg->stream; h->cfg.chunk_pixels = cfg->chunk_pixels;
  h->cfg.scratch_format = 16;
  adam_defaults(h);
  h->D = cfg->n_linear; h->WD = cfg->hidden; h->MS = cfg->map_size;
  h->stream = (hipStream_t)cfg->stream;
  h->npix = (long)cfg->height * cfg->width;
  h->n_total = (double)cfg->height * (double)cfg->width;
  const int WD = h->WD, D = h->D, MS = h->MS;
  // flat parameters: layers.{2l}.weight, layers.{2l}.bias (encoding.B is frozen and lives outside)
  int64_t off = 0;
  long img = 0;
  for (int l = 0; l < D; ++l) {
    const int in = l == 0 ? MS : WD, outn = l == D - 1 ? cfg->out_features : WD;
    h->off_w[l] = off; off += (int64_t)in * outn;
    h->off_b[l] = off; off += outn;
    h->ff_img_f[l] = img; img += (long)((outn + 31) / 32) * (in / 16) * 64;
    if (l > 0) { h->ff_img_b[l] = img; img += (long)(in / 32) * ((outn + 15) / 16) * 64; }
  }
  h->P = off;
  h->ff_img_n = img;
  h->gpre = (float)exp2(ceil(log2((double)cfg->out_features * (double)cfg->height * (double)cfg->width)) + 2.0);
  // chunking: 4 Mi pixels, or fewer when the activation + gradient planes of a chunk would pass 16 GiB
  const double px_bytes = (double)(D - 1) * WD * 4.0 + 8.0;
  // (never more than 4 Mi: the kernels address a [WD][chunk] plane with 32-bit offsets)
  const long want = cfg->chunk_pixels > 0 ? (long)cfg->chunk_pixels : (long)fmin((double)(1L << 22), 17179869184.0 / px_bytes);
  const long chunk = chunk_pixels(std::min(want, 1L << 22), h->npix);
  h->chunk_px = chunk;
  h->dw_wg = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  h->ff_dw_wgs = 4 * h->dw_wg;
  long slab_row = (long)WD * MS + WD;
  if ((long)WD * WD + WD > slab_row) slab_row = (long)WD * WD + WD;
  if (render) {   // no gradient, moments or mask
    SF_TRY(dev_alloc(h, h->params, h->P * 4));
    hipMemsetAsync(h->params, 0, h->P * 4, h->stream);
  } else {
    SF_TRY(alloc_train_state(h));
  }
  SF_TRY(dev_alloc(h, h->ffimg, (size_t)h->ff_img_n * 16));
  SF_TRY(dev_alloc(h, h->ffB, (size_t)cfg->in_features * (MS / 2) * 4));
  SF_TRY(dev_alloc(h, h->gh, (size_t)cfg->height * 4));
  SF_TRY(dev_alloc(h, h->gw, (size_t)cfg->width * 4));
  if (render) {   // no activation / gradient planes, slab or SSE partials: k_ff_fwd's RENDER form spills nothing
    *out = owner.release();
    return SF_OK;
  }
  SF_TRY(dev_alloc(h, h->ffH, (size_t)(D - 1) * WD * chunk * 2));
  SF_TRY(dev_alloc(h, h->ffG, (size_t)(D - 1) * WD * chunk * 2));
  SF_TRY(dev_alloc(h, h->ffZ, (size_t)4 * chunk * 2));
  SF_TRY(dev_alloc(h, h->slab, (size_t)h->ff_dw_wgs * slab_row * 4));
  SF_TRY(alloc_sse(h, chunked_sse_parts(h)));
  *out = owner.release();
  return SF_OK;
}
int sf_fourier_create(const sf_fourier_config* cfg, sf_handle** out) try { return create_fourier(cfg, out, false); } SF_CATCH

// WaveletSiren handle: two SIREN sub-handles (sf_create, format 16) whose state buffers are slices of this handle's joint
// [LF | HF] vectors, so that sf_state_ptr, sf_get/set_*, sf_adam_step (one k_adam over the joint vector), sf_step and graph
// replay work unchanged; run_pass_wavelet drives the sub-handles around the composition kernels
int sf_wavelet_create(const sf_wavelet_config* cfg, sf_handle** out) try {
  if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SF_ABI_VERSION) return fail(SF_ERR_INVALID, "abi_version mismatch");
  if (cfg->in_features != 2) return fail(SF_ERR_INVALID, "in_features must be 2 (coordinate grid)");
  if (cfg->out_features != 3) return fail(SF_ERR_INVALID, "out_features must be 3 (Y, Cb, Cr / the three detail bands)");
  if (cfg->wavelet_levels != 1)
    return fail(SF_ERR_INVALID, "wavelet_levels must be 1: the reference's single-level inverse DWT receives 3 * levels bands "
                                "and fails for more");
  SF_TRY(wavelet_check_network(cfg));
  if (cfg->scratch_format != 0 && cfg->scratch_format != 16)
    return fail(SF_ERR_INVALID, "WaveletSiren runs scratch format 16 (0 = auto resolves to it): format 8 takes its fp8 delta "
                                "scale from the fused residual, which a WaveletSiren pass does not form");
  SF_TRY(wavelet_check_image(cfg->height, cfg->width, cfg->chunk_pixels));
  const int H = cfg->height, n = (H + 5) / 2;
  sf_config sc = wavelet_sub_config(cfg, n, n);
  sc.beta1 = cfg->beta1; sc.beta2 = cfg->beta2; sc.eps = cfg->eps;
  HandlePtr owner;
  SF_TRY(wavelet_begin(sc, false, H, owner));
  DevGuard dev_guard(cfg->device);
  sf_engine* h = owner.get();
  const long nn = h->wv_sub[0]->npix;
  const bool one = nn <= h->wv_sub[0]->chunk_px;
  h->chunk_px = one ? h->npix : 1;   // (sf_step's graph replay covers single-chunk fits only)
  const int64_t P0 = h->wv_sub[0]->P;
  // the sub-networks' dL/dout pre-scale comes from the 3 H^2 values of the full image (what the loss mean divides by)
  const float gpre = (float)exp2(ceil(log2(3.0 * h->n_total)) + 2.0);
  for (sf_engine* s : h->wv_sub) { s->gpre = gpre; s->ext_dout = true; }
  SF_TRY(alloc_train_state(h));
  SF_TRY(dev_alloc(h, h->wv_pred, (size_t)2 * nn * 3 * 4));
  SF_TRY(dev_alloc(h, h->wv_g, (size_t)h->npix * 3 * 4));
  if (!one) SF_TRY(dev_alloc(h, h->wv_gl, (size_t)2 * nn * 3 * 4));
  if (!cfg->outermost_linear) SF_TRY(dev_alloc(h, h->wv_dfac, (size_t)2 * nn * 3 * 4));
  SF_TRY(alloc_sse(h, (h->npix + kWvThreads - 1) / kWvThreads));
  for (int s = 0; s < 2; ++s) {   // the sub-handles' state: the two halves of the joint vectors
    sf_engine* e = h->wv_sub[s];
    e->params = h->params + s * P0; e->grads = h->grads + s * P0; e->m = h->m + s * P0; e->v = h->v + s * P0;
    e->mask = h->mask + s * P0;
    if (h->wv_dfac) e->dfac_out = h->wv_dfac + (size_t)s * nn * 3;
  }
  *out = owner.release();
  return SF_OK;
} SF_CATCH

int sf_wavelet_debug(sf_handle* h, int32_t which, const float* in0, const float* in1, const float* img, float* out0,
                     float* out1) try {
  if (!h || !in0 || !out0 || !out1 || (which == 0 && !in1)) return fail(SF_ERR_INVALID, "null argument");
  if (h->render) return fail(SF_ERR_INVALID, "sf_wavelet_debug: a render handle (sf_wavelet_render_create) runs sf_wavelet_render only");
  if (!h->wavelet) return fail(SF_ERR_INVALID, "sf_wavelet_debug: not a WaveletSiren handle (sf_wavelet_create)");
  if (which != 0 && which != 1) return fail(SF_ERR_INVALID, "sf_wavelet_debug: which must be 0 or 1");
  DevGuard dev_guard(h->cfg.device);
  WvArgs a;
  memset(&a, 0, sizeof(a));
  a.H = h->cfg.height; a.n = h->wv_n; a.up = h->wv_up;
  a.gscale = (float)(2.0 / (3.0 * h->n_total));
  a.dscale = 1.0f;
  if (which == 0) {
    a.lf = in0; a.hf = in1; a.img = img; a.pred = out0; a.g = img ? out1 : nullptr; a.sse_part = h->sse_part;
    return launch(h, k_wv_compose, (h->npix + kWvThreads - 1) / kWvThreads, kWvThreads, 0, a);
  }
  a.g = const_cast<float*>(in0); a.gl_lf = out0; a.gl_hf = out1;
  const long nn = (long)h->wv_n * h->wv_n;
  return launch(h, k_wv_adjoint, (nn + kWvThreads - 1) / kWvThreads, kWvThreads, 0, a);
} SF_CATCH

int sf_set_encoding(sf_handle* h, const float* B_dev) try {
  if (!h || !B_dev) return fail(SF_ERR_INVALID, "null argument");
  if (!h->fourier) return fail(SF_ERR_INVALID, "sf_set_encoding: not a FourierNet handle (sf_fourier_create / sf_fourier_render_create)");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(h->ffB, B_dev, (size_t)h->cfg.in_features * (h->MS / 2) * 4, hipMemcpyDeviceToDevice, h->stream));
  h->have_B = true;
  return SF_OK;
} SF_CATCH

int sf_destroy(sf_handle* h) try {
  if (!h) return SF_OK;
  DevGuard dev_guard(h->cfg.device);
  hipStreamSynchronize(h->stream);
  for (auto& r : h->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
  for (sf_engine* s : h->wv_sub) if (s) sf_destroy(s);
  if (h->gexec) hipGraphExecDestroy(h->gexec);
  if (h->gstream) { hipStreamSynchronize(h->gstream); hipStreamDestroy(h->gstream); hipEventDestroy(h->gev_in); hipEventDestroy(h->gev_out); }
  for (void* p : h->owned) hipFree(p);
  delete h;
  return SF_OK;
} SF_CATCH

int sf_num_params(const sf_handle* h, int64_t* n) try {
  if (!h || !n) return fail(SF_ERR_INVALID, "null argument");
  *n = h->P;
  return SF_OK;
} SF_CATCH
int sf_scratch_format(const sf_handle* h, int32_t* format) try {
  if (!h || !format) return fail(SF_ERR_INVALID, "null argument");
  *format = h->cfg.scratch_format;
  return SF_OK;
} SF_CATCH
int sf_param_offset(const sf_handle* h, int32_t layer, int64_t* w, int64_t* b) try {
  if (!h || layer < 0 || layer >= h->D) return fail(SF_ERR_INVALID, "bad layer");
  if (h->wavelet) {   // layers 0 .. depth-1: LF, then HF in the second half of the flat vector
    const sf_engine* s = h->wv_sub[layer >= h->wv_sub[0]->D];
    const int64_t base = layer >= h->wv_sub[0]->D ? h->wv_sub[0]->P : 0;
    const int l = layer >= h->wv_sub[0]->D ? layer - h->wv_sub[0]->D : layer;
    if (w) *w = base + s->off_w[l];
    if (b) *b = base + s->off_b[l];
    return SF_OK;
  }
  if (w) *w = h->off_w[layer];
  if (b) *b = h->off_b[layer];
  return SF_OK;
} SF_CATCH

// training entry points on a render handle: an argument error, before anything is touched
static int refuse_render(const char* fn) {
  return fail(SF_ERR_INVALID, std::string(fn) + ": a render handle (sf_render_create) holds parameters and forward images "
                                                "only - no gradient, optimiser state, mask or backward scratch");
}
#define SF_NO_RENDER(h, fn) do { if ((h) && (h)->render) return refuse_render(fn); } while (0)

static int copy_in(sf_engine* h, float* dst, const float* src) {
  if (!h || !src) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(dst, src, h->P * 4, hipMemcpyDeviceToDevice, h->stream));
  return SF_OK;
}
static int copy_out(sf_engine* h, float* dst, const float* src) {
  if (!h || !dst) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  HIPCHK(hipMemcpyAsync(dst, src, h->P * 4, hipMemcpyDeviceToDevice, h->stream));
  return SF_OK;
}
int sf_set_params(sf_handle* h, const float* p) try {
  int rc = copy_in(h, h ? h->params : nullptr, p);
  if (!rc) h->images_dirty = true;
  return rc;
} SF_CATCH
int sf_get_params(sf_handle* h, float* p) try { return copy_out(h, p, h ? h->params : nullptr); } SF_CATCH
int sf_get_grads(sf_handle* h, float* p) try {
  SF_NO_RENDER(h, "sf_get_grads");
  return copy_out(h, p, h ? h->grads : nullptr);
} SF_CATCH
int sf_set_grads(sf_handle* h, const float* p) try {
  SF_NO_RENDER(h, "sf_set_grads");
  if (h) h->fth_fresh = false;
  return copy_in(h, h ? h->grads : nullptr, p);
} SF_CATCH
// An auto-format handle that receives a mask leaves the 8-bit scratch: fp8 deltas under one scale per chunk underflow in
// a 90 %-sparse network, and topology updates rank small gradients that phase bytes blur.
// (the new buffers are allocated BEFORE anything of the handle changes: a failed hipMalloc leaves the handle exactly as it
//  was - format, strides and scratch - and returns SF_ERR_NOMEM)
static int switch_scratch_format(sf_engine* h, int fmt) {
  hipStreamSynchronize(h->stream);
  const sf_config cfg0 = h->cfg;
  const bool s8_0 = h->s8, d8_0 = h->d8;
  h->cfg.scratch_format = fmt;
  h->s8 = fmt == 8 || fmt == 12;
  h->d8 = fmt == 8;
  set_scratch_strides(h);
  u32x4 *newP = nullptr, *newD = nullptr;
  if (dev_alloc(h, newP, (size_t)(h->D - 1) * h->p_stride * 16) || dev_alloc(h, newD, (size_t)(h->D - 1) * h->d_stride * 16)) {
    dev_free(h, newP);
    (void)hipGetLastError();
    h->cfg = cfg0; h->s8 = s8_0; h->d8 = d8_0;
    set_scratch_strides(h);
    return fail(SF_ERR_NOMEM, "hipMalloc failed while moving the scratch to format 16 (the handle keeps its format)");
  }
  if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
  dev_free(h, h->Pbuf);
  dev_free(h, h->Dbuf);
  h->Pbuf = newP; h->Dbuf = newD;
  h->images_dirty = true;      // (the backward images carry the fp8 per-layer scales only under format 8)
  return SF_OK;
}
int sf_set_masks(sf_handle* h, const float* p) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_masks");
  DevGuard dev_guard(h->cfg.device);
  if (!p) { h->has_mask = false; return SF_OK; }
  if (h->feather) return fail(SF_ERR_INVALID, "sf_set_masks: a Feathermap handle is dense (masking.dense: True)");
  if (h->fmt_auto && h->cfg.scratch_format != 16) {
    const int rs = switch_scratch_format(h, 16);
    if (rs) return rs;
  }
  int rc = copy_in(h, h->mask, p);
  if (!rc) h->has_mask = true;
  return rc;
} SF_CATCH
int sf_get_adam_state(sf_handle* h, float* m, float* v, int64_t* step) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_get_adam_state");
  DevGuard dev_guard(h->cfg.device);
  if (m) { int rc = copy_out(h, m, h->m); if (rc) return rc; }
  if (v) { int rc = copy_out(h, v, h->v); if (rc) return rc; }
  if (step) *step = h->step;
  return SF_OK;
} SF_CATCH
int sf_set_adam_state(sf_handle* h, const float* m, const float* v, int64_t step) try {
  if (!h || step < 0) return fail(SF_ERR_INVALID, "bad argument");
  SF_NO_RENDER(h, "sf_set_adam_state");
  DevGuard dev_guard(h->cfg.device);
  if (m) { int rc = copy_in(h, h->m, m); if (rc) return rc; }
  if (v) { int rc = copy_in(h, h->v, v); if (rc) return rc; }
  h->step = step;
  return SF_OK;
} SF_CATCH
int sf_state_ptr(sf_handle* h, int32_t which, float** p) try {
  if (!h || !p) return fail(SF_ERR_INVALID, "null argument");
  if (h->render && which >= 1 && which <= 4) return refuse_render("sf_state_ptr");
  switch (which) {
    case 0: *p = h->params; return SF_OK;
    case 1: *p = h->grads; return SF_OK;
    case 2: *p = h->m; return SF_OK;
    case 3: *p = h->v; return SF_OK;
    case 4: *p = h->mask; return SF_OK;
  }
  return fail(SF_ERR_INVALID, "bad state selector");
} SF_CATCH

int sf_sse_ptr(sf_handle* h, double** p) try {
  if (!h || !p) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_sse_ptr");
  *p = h->sse_dev;
  return SF_OK;
} SF_CATCH

int sf_debug_scratch(sf_handle* h, int32_t which, void** p, int64_t* bytes) try {
  if (!h || !p || !bytes) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_debug_scratch");
  if (h->fourier) return fail(SF_ERR_INVALID, "sf_debug_scratch: a FourierNet handle has no phase / delta scratch");
  if (h->wavelet) return fail(SF_ERR_INVALID, "sf_debug_scratch: the scratch of a WaveletSiren handle lives in its sub-networks");
  const int D = h->D;
  switch (which) {
    case 0: *p = h->Pbuf; *bytes = (int64_t)(D - 1) * h->p_stride * 16; return SF_OK;
    case 1: *p = h->Dbuf; *bytes = (int64_t)(D - 1) * h->d_stride * 16; return SF_OK;
    case 2: *p = h->Dlast; *bytes = (int64_t)(h->chunk_px / 32) * (h->s8 ? 1 : 2) * 64 * 16; return SF_OK;
    case 3: { const size_t sw = h->WD > 256 ? 256 : h->WD; *p = h->slab; *bytes = (int64_t)h->dw_wg * (sw * sw + sw) * 4; return SF_OK; }
  }
  return fail(SF_ERR_INVALID, "bad scratch selector");
} SF_CATCH

int sf_params_changed(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  h->images_dirty = true;
  return SF_OK;
} SF_CATCH

int sf_set_coords(sf_handle* h, const float* rows, const float* cols) try {
  if (!h || !rows || !cols) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  if (h->wavelet && h->render) {   // kept whole and unchecked: sf_wavelet_render points the sub-networks at slices of them
    HIPCHK(hipMemcpyAsync(h->gh, rows, (size_t)h->wv_n * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->gw, cols, (size_t)h->wv_n * 4, hipMemcpyDeviceToDevice, h->stream));
    h->have_coords = true;
    return SF_OK;
  }
  if (h->wavelet) {   // both sub-networks run on the n x n coefficient grid (wavelet_siren.py:76-80)
    wv_sync(h);
    for (sf_engine* s : h->wv_sub) {
      const int rc = sf_set_coords(s, rows, cols);
      if (rc) return rc;
    }
    h->have_coords = true;
    return SF_OK;
  }
  HIPCHK(hipMemcpyAsync(h->gh, rows, (size_t)h->cfg.height * 4, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->gw, cols, (size_t)h->cfg.width * 4, hipMemcpyDeviceToDevice, h->stream));
  // The forward indexes these vectors; the gradient kernels of layer 0 / layer 1 re-derive the coordinate of a
  // pixel as i/(n-1) instead of loading it.  Both agree only for get_grid()'s linspace(0,1,n) (data.py:82-83):
  // anything else is rejected here instead of training on inconsistent coordinates.  A render handle only indexes them
  // (a window of a grid is a slice of the two vectors), so it takes whatever it is given.
  if (!h->render) {
    std::vector<float> hv((size_t)h->cfg.height + h->cfg.width);
    HIPCHK(hipMemcpyAsync(hv.data(), h->gh, (size_t)h->cfg.height * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hv.data() + h->cfg.height, h->gw, (size_t)h->cfg.width * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    auto is_linspace = [](const float* v, int n) {
      for (int i = 0; i < n; ++i) {
        const float ref = n > 1 ? (float)((double)i / (double)(n - 1)) : 0.f;
        if (!(fabsf(v[i] - ref) <= 2e-6f)) return false;
      }
      return true;
    };
    if (!is_linspace(hv.data(), h->cfg.height) || !is_linspace(hv.data() + h->cfg.height, h->cfg.width))
      return fail(SF_ERR_INVALID, "sf_set_coords: rows / cols must be torch.linspace(0, 1, n) (data.py:82-83)");
  }
  h->have_coords = true;
  return SF_OK;
} SF_CATCH
int sf_set_target(sf_handle* h, const float* img) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_target");
  h->img = img;
  return SF_OK;
} SF_CATCH

int sf_forward(sf_handle* h, float* pred, double* sse_out) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  const bool want = sse_out != nullptr;
  const float* keep = h->img;
  int rc = run_pass(h, false, pred, want);
  h->img = keep;
  if (rc) return rc;
  if (want) return read_sse(h, sse_out);
  return SF_OK;
} SF_CATCH

int sf_forward_backward(sf_handle* h, double* sse_out) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_forward_backward");
  DevGuard dev_guard(h->cfg.device);
  int rc = run_pass(h, true, nullptr, true);
  if (rc) return rc;
  if (sse_out) return read_sse(h, sse_out);
  return SF_OK;
} SF_CATCH

int sf_adam_step(sf_handle* h, float lr) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_adam_step");
  DevGuard dev_guard(h->cfg.device);
  h->step += 1;
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  if (h->replay) { a.tab = h->step_tab; a.iter = h->iter_dev; }
  a.p = h->params; a.g = h->grads; a.m = h->m; a.v = h->v; a.mask = h->has_mask ? h->mask : nullptr;
  a.n = h->P;
  a.beta1 = h->cfg.beta1; a.beta2 = h->cfg.beta2; a.eps = h->cfg.eps;
  // torch forms 1 - beta in double and hands the kernel the rounded float (0.1f, 0.001f); 1.0f - beta in fp32 is
  // 0.100000024 / 0.000999987
  a.omb1 = (float)(1.0 - h->beta1_d); a.omb2 = (float)(1.0 - h->beta2_d);
  const double bc1 = 1.0 - pow(h->beta1_d, (double)h->step);
  const double bc2 = 1.0 - pow(h->beta2_d, (double)h->step);
  a.step_size = (float)((double)lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  if (h->feather) {   // adjoint -> Adam on [V1 | V2 | scalers] -> materialise: four launches
    if (!h->fth_fresh) { const int rc = feather_adjoint(h); if (rc) return rc; }
    a.p = h->fth_p; a.g = h->fth_g; a.m = h->fth_m; a.v = h->fth_v; a.mask = nullptr; a.n = h->fth_nf;
    {
      Launch L(h, K_FTH_ADAM, 0, (double)h->fth_nf * 28);
      SF_TRY(launch(h, k_adam, (h->fth_nf + 255) / 256, 256, 0, a));
    }
    SF_TRY(feather_materialise(h));
    return refresh_images(h);
  }
  {
    Launch L(h, K_ADAM, 0, (double)h->P * 28);
    SF_TRY(launch(h, k_adam, (h->P + 255) / 256, 256, 0, a));
  }
  h->images_dirty = true;
  return refresh_images(h);
} SF_CATCH


// ---- graph replay -----------------------------------------------------------------------------------------
// One training step (forward, backward, reductions, Adam, weight images) is captured ONCE into a hipGraph on an
// engine-owned stream and replayed n times; the only per-step scalars (Adam's bias-corrected step size, computed
// on the host in double exactly as sf_adam_step does) are read from a device table indexed by a device counter.
static int graph_prepare(sf_engine* h, int n) {
  if (!h->gstream) {
    HIPCHK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->gev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->gev_out, hipEventDisableTiming));
    SF_TRY(dev_alloc(h, h->iter_dev, 16));
    HIPCHK(hipMemset(h->iter_dev, 0, 16));   // [0] replay step index, [2] constant 0 (eager table index)
  }
  if (n > h->tab_cap) {
    dev_free(h, h->step_tab);
    dev_free(h, h->loss_tab);
    h->step_tab = nullptr; h->loss_tab = nullptr; h->tab_cap = 0;
    SF_TRY(dev_alloc(h, h->step_tab, (size_t)n * 8));
    SF_TRY(dev_alloc(h, h->loss_tab, (size_t)n * 8));
    h->tab_cap = n;
    if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }   // the graph holds the old table pointers
  }
  return SF_OK;
}

static int step_replay(sf_engine* h, const float* lr, int n, float* loss_out) {
  int rc = graph_prepare(h, n);
  if (rc) return rc;
  std::vector<float> tab((size_t)n * 2);
  for (int i = 0; i < n; ++i) {
    const double t = (double)(h->step + i + 1);
    const double bc1 = 1.0 - pow(h->beta1_d, t), bc2 = 1.0 - pow(h->beta2_d, t);
    tab[2 * i] = (float)((double)lr[i] / bc1);
    tab[2 * i + 1] = (float)sqrt(bc2);
  }
  hipStream_t user = h->stream;
  HIPCHK(hipEventRecord(h->gev_in, user));
  HIPCHK(hipStreamWaitEvent(h->gstream, h->gev_in, 0));
  h->stream = h->gstream;
  struct Restore { sf_engine* h; hipStream_t s; ~Restore() { h->stream = s; h->replay = false; } } restore{h, user};
  HIPCHK(hipMemcpyAsync(h->step_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->gstream));
  HIPCHK(hipStreamSynchronize(h->gstream));            // `tab` is pageable host memory: keep it alive until copied
  HIPCHK(hipMemsetAsync(h->iter_dev, 0, 4, h->gstream));
  rc = refresh_images(h);                                // parameters edited since the last pass
  if (rc) return rc;
  if (!h->gexec || h->g_img != h->img || h->g_mask != h->has_mask) {
    if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(h->gstream, hipStreamCaptureModeRelaxed));
    h->replay = true;
    const int64_t step0 = h->step;
    rc = run_pass(h, true, nullptr, true);
    if (!rc) rc = sf_adam_step(h, 0.f);
    if (!rc) rc = launch(h, k_tick, 1, 1, 0, h->iter_dev);   // (h->stream is the capturing stream here)
    h->step = step0;
    h->replay = false;
    const hipError_t e = hipStreamEndCapture(h->gstream, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(SF_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t e2 = hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e2 != hipSuccess) { h->gexec = nullptr; return fail(SF_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
    h->g_img = h->img; h->g_mask = h->has_mask;
  }
  for (int i = 0; i < n; ++i) HIPCHK(hipGraphLaunch(h->gexec, h->gstream));
  h->step += n;
  h->images_dirty = false;
  if (loss_out) {
    std::vector<double> sse((size_t)n);
    HIPCHK(hipMemcpyAsync(sse.data(), h->loss_tab, (size_t)n * 8, hipMemcpyDeviceToHost, h->gstream));
    HIPCHK(hipStreamSynchronize(h->gstream));
    for (int i = 0; i < n; ++i) loss_out[i] = (float)(sse[i] / ((double)h->cfg.out_features * (double)h->npix));
  }
  HIPCHK(hipEventRecord(h->gev_out, h->gstream));
  HIPCHK(hipStreamWaitEvent(user, h->gev_out, 0));
  return SF_OK;
}

int sf_step(sf_handle* h, const float* lr, int32_t n_steps, float* loss_out) try {
  if (!h || !lr || n_steps < 0) return fail(SF_ERR_INVALID, "bad argument");
  SF_NO_RENDER(h, "sf_step");
  DevGuard dev_guard(h->cfg.device);
  if (!h->have_coords) return fail(SF_ERR_STATE, "sf_set_coords has not been called");
  if (!h->img) return fail(SF_ERR_STATE, "sf_set_target has not been called");
  if (h->want_replay && n_steps >= 2 && !h->prof && h->npix <= h->chunk_px) return step_replay(h, lr, n_steps, loss_out);
  if (loss_out && n_steps > 1) {
    // eager, but without a host sync per step: every step's SSE goes to a device table, read back once
    int rc = graph_prepare(h, n_steps);
    if (rc) return rc;
    for (int i = 0; i < n_steps && !rc; ++i) {
      h->loss_dst = h->loss_tab + i;
      rc = run_pass(h, true, nullptr, true);
      h->loss_dst = nullptr;
      if (!rc) rc = sf_adam_step(h, lr[i]);
    }
    if (rc) return rc;
    std::vector<double> sse((size_t)n_steps);
    HIPCHK(hipMemcpyAsync(sse.data(), h->loss_tab, (size_t)n_steps * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_steps; ++i) loss_out[i] = (float)(sse[i] / ((double)h->cfg.out_features * (double)h->npix));
    return SF_OK;
  }
  for (int i = 0; i < n_steps; ++i) {
    int rc = run_pass(h, true, nullptr, true);
    if (rc) return rc;
    if (loss_out) {
      double sse = 0;
      rc = read_sse(h, &sse);
      if (rc) return rc;
      loss_out[i] = (float)(sse / ((double)h->cfg.out_features * (double)h->npix));
    }
    rc = sf_adam_step(h, lr[i]);
    if (rc) return rc;
  }
  return SF_OK;
} SF_CATCH

int sf_set_graph_replay(sf_handle* h, int32_t on) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_set_graph_replay");
  h->want_replay = on != 0;
  return SF_OK;
} SF_CATCH

int sf_profile_enable(sf_handle* h, int32_t on) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  if (!on) { int rc = prof_flush(h); if (rc) return rc; }
  h->prof = on != 0;
  for (sf_engine* s : h->wv_sub) if (s) { int rc = sf_profile_enable(s, on); if (rc) return rc; }
  return SF_OK;
} SF_CATCH
int sf_profile_reset(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  DevGuard dev_guard(h->cfg.device);
  int rc = prof_flush(h);
  if (rc) return rc;
  for (int i = 0; i < K_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; h->prof_flops[i] = 0; h->prof_bytes[i] = 0; }
  for (sf_engine* s : h->wv_sub) if (s) { rc = sf_profile_reset(s); if (rc) return rc; }
  return SF_OK;
} SF_CATCH
int sf_profile_num_kernels(const sf_handle* h, int32_t* n) try {
  if (!h || !n) return fail(SF_ERR_INVALID, "null argument");
  *n = K_COUNT;
  return SF_OK;
} SF_CATCH
int sf_profile_get(sf_handle* h, int32_t idx, const char** name, double* total_ms, int64_t* launches,
                   double* flops_per_launch, double* bytes_per_launch) try {
  if (!h || idx < 0 || idx >= K_COUNT) return fail(SF_ERR_INVALID, "bad kernel index");
  DevGuard dev_guard(h->cfg.device);
  int rc = prof_flush(h);
  if (rc) return rc;
  double ms = h->prof_ms[idx], fl = h->prof_flops[idx], by = h->prof_bytes[idx];
  int64_t cnt = h->prof_n[idx];
  for (sf_engine* s : h->wv_sub) {   // WaveletSiren: the sub-networks' launches count as the handle's
    if (!s) continue;
    rc = prof_flush(s);
    if (rc) return rc;
    ms += s->prof_ms[idx]; fl += s->prof_flops[idx]; by += s->prof_bytes[idx]; cnt += s->prof_n[idx];
  }
  if (name) *name = kKernelNames[idx];
  if (total_ms) *total_ms = ms;
  if (launches) *launches = cnt;
  const double nl = cnt > 0 ? (double)cnt : 1.0;
  if (flops_per_launch) *flops_per_launch = fl / nl;
  if (bytes_per_launch) *bytes_per_launch = by / nl;
  return SF_OK;
} SF_CATCH

/* k-means weight quantisation of one tensor on the handle's stream, no host synchronisation (siren_kmeans.hip) */
int sf_kmeans_fit(sf_handle* h, const float* w_dev, int64_t n, float* centers_dev, int32_t K, int32_t iter_limit, float tol,
                  float* centroids_dev, int32_t centroids_cap, int32_t* n_centroids_dev, int64_t* labels_dev,
                  float* new_weight_dev) try {
  if (!h || !w_dev || !centers_dev || !centroids_dev) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_kmeans_fit");
  if (n <= 0 || K < 1 || K >= kKmMaxK || centroids_cap < K + 1 || iter_limit < 0)
    return fail(SF_ERR_INVALID, "sf_kmeans_fit: need n > 0, 1 <= K < 512, centroids_cap >= K + 1");
  DevGuard dev_guard(h->cfg.device);
  if (!h->km_ws) {
    if (dev_alloc(h, h->km_ws, sizeof(KmWs))) return fail(SF_ERR_NOMEM, "hipMalloc failed (k-means workspace)");
    HIPCHK(hipMemsetAsync(h->km_ws, 0, sizeof(KmWs), h->stream));
  }
  long blocks = (n + 255) / 256;
  const long cap = 4L * h->dw_wg;
  if (blocks > cap) blocks = cap;
  SF_TRY(launch(h, k_km_init, 1, kKmMaxK, 0, centers_dev, K, n, h->km_ws));
  for (int it = 0; it < iter_limit; ++it) {
    SF_TRY(launch(h, k_km_assign, blocks, 256, 0, w_dev, n, centers_dev, K, h->km_ws));
    SF_TRY(launch(h, k_km_update, 1, kKmMaxK, 0, centers_dev, K, h->km_ws, tol));
  }
  SF_TRY(launch(h, k_km_finish, 1, kKmMaxK, 0, centers_dev, K, h->km_ws, centroids_dev, centroids_cap, n_centroids_dev));
  if (labels_dev || new_weight_dev)
    SF_TRY(launch(h, k_km_predict, blocks, 256, 0, w_dev, n, centroids_dev, h->km_ws, (long long*)labels_dev, new_weight_dev));
  return SF_OK;
} SF_CATCH

// ---- Feathermap (structured multi-hashing, feather_kernels.hip) ---------------------------------------------------
int sf_feather_attach(sf_handle* h, int64_t n, int64_t m, int32_t n_layers, const int32_t* logical_out,
                      const int32_t* logical_in) try {
  if (!h || !logical_out || !logical_in) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_attach");
  if (h->fourier || h->wavelet) return fail(SF_ERR_INVALID, "sf_feather_attach: Feathermap runs on SIREN handles only");
  if (h->feather) return fail(SF_ERR_INVALID, "sf_feather_attach: the handle already has a feather state");
  if (h->cfg.row_begin != 0 || h->cfg.row_end != h->cfg.height)
    return fail(SF_ERR_INVALID, "sf_feather_attach: Feathermap fits the whole image (no pixel split)");
  if (h->has_mask) return fail(SF_ERR_INVALID, "sf_feather_attach: the handle has a mask (Feathermap is dense)");
  if (n_layers != h->D) return fail(SF_ERR_INVALID, "sf_feather_attach: n_layers must equal the handle's depth");
  FthArgs a;
  memset(&a, 0, sizeof(a));
  const int D = h->D;
  long P = 0;
  for (int l = 0; l < D; ++l) {
    const int in_p = l == 0 ? h->cfg.in_features : h->WD, out_p = l == D - 1 ? h->cfg.out_features : h->WD;
    const int in = logical_in[l], outn = logical_out[l];
    if (in < 1 || outn < 1 || in > in_p || outn > out_p || (l == 0 && in != in_p) || (l == D - 1 && outn != out_p))
      return fail(SF_ERR_INVALID, "sf_feather_attach: logical layer sizes do not fit the handle");
    a.seg.start[2 * l] = P; a.seg.base[2 * l] = h->off_w[l]; a.seg.cols[2 * l] = in; a.seg.stride[2 * l] = in_p;
    P += (long)in * outn;
    a.seg.start[2 * l + 1] = P; a.seg.base[2 * l + 1] = h->off_b[l]; a.seg.cols[2 * l + 1] = outn;
    a.seg.stride[2 * l + 1] = outn;
    P += outn;
  }
  a.seg.nseg = 2 * D;
  a.seg.start[2 * D] = P;
  if (n < 1 || m < 1 || n > 46340 || m > n || n * n < P)
    return fail(SF_ERR_INVALID, "sf_feather_attach: need 1 <= m <= n <= 46340 and n^2 >= the parameter count");
  a.n = (int)n; a.m = (int)m; a.P = P;
  a.rows_used = (int)((P + n - 1) / n);
  std::vector<long> chunks;
  std::vector<int> chunk0;
  for (int k = 0; k < a.seg.nseg; ++k) {
    chunk0.push_back((int)(chunks.size() / 3));
    for (long b = a.seg.start[k]; b < a.seg.start[k + 1]; b += kFthChunk) {
      chunks.push_back(k); chunks.push_back(b); chunks.push_back(std::min(b + kFthChunk, a.seg.start[k + 1]));
    }
  }
  chunk0.push_back((int)(chunks.size() / 3));
  a.nchunks = (int)(chunks.size() / 3);
  a.g_blocks = (int)std::min<long>((P + 255) / 256, 8L * h->dw_wg);
  a.t1n = (a.m + kFthTile - 1) / kFthTile;
  a.t1 = (a.n + kFthTile - 1) / kFthTile * a.t1n;
  a.t2n = (a.n + kFthTile - 1) / kFthTile;
  const long nf = 2 * n * m + 2L * D;
  DevGuard dev_guard(h->cfg.device);
  // (a failure part-way leaves a handle without feather state: h->feather stays false, nothing reads the fth_* fields, and
  //  what was allocated stays on the owned list until sf_destroy)
  if (dev_alloc(h, h->fth_p, nf * 4) || dev_alloc(h, h->fth_g, nf * 4) || dev_alloc(h, h->fth_m, nf * 4) ||
      dev_alloc(h, h->fth_v, nf * 4) || dev_alloc(h, h->fth_V, P * 4) || dev_alloc(h, h->fth_G, n * n * 4) ||
      dev_alloc(h, h->fth_part, (size_t)a.nchunks * 4) || dev_alloc(h, h->fth_chunks, chunks.size() * sizeof(long)) ||
      dev_alloc(h, h->fth_chunk0, chunk0.size() * sizeof(int))) {
    (void)hipGetLastError();
    return fail(SF_ERR_NOMEM, "hipMalloc failed (feather state)");
  }
  HIPCHK(hipMemcpy(h->fth_chunks, chunks.data(), chunks.size() * sizeof(long), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->fth_chunk0, chunk0.data(), chunk0.size() * sizeof(int), hipMemcpyHostToDevice));
  for (float* p : {h->fth_p, h->fth_g, h->fth_m, h->fth_v}) HIPCHK(hipMemsetAsync(p, 0, nf * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->fth_V, 0, P * 4, h->stream)); HIPCHK(hipMemsetAsync(h->fth_G, 0, n * n * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->params, 0, h->P * 4, h->stream));   // padded slots stay exactly 0
  a.fp = h->fth_p; a.fg = h->fth_g; a.V = h->fth_V; a.G = h->fth_G; a.W = h->params; a.dW = h->grads;
  a.chunks = h->fth_chunks; a.seg_chunk0 = h->fth_chunk0; a.part = h->fth_part;
  h->fth = a;
  h->fth_nf = nf;
  h->feather = true;
  h->fth_fresh = false;
  if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }   // a captured step holds the dense Adam
  h->images_dirty = true;
  return SF_OK;
} SF_CATCH

int sf_feather_state_ptr(sf_handle* h, int32_t which, float** dev_ptr, int64_t* len) try {
  if (!h || !dev_ptr) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_state_ptr");
  if (!h->feather) return fail(SF_ERR_STATE, "sf_feather_state_ptr: no feather state (sf_feather_attach)");
  float* ps[] = {h->fth_p, h->fth_g, h->fth_m, h->fth_v, h->fth_V};
  if (which < 0 || which > 4) return fail(SF_ERR_INVALID, "bad feather state selector");
  *dev_ptr = ps[which];
  if (len) *len = which == 4 ? h->fth.P : h->fth_nf;
  return SF_OK;
} SF_CATCH

int sf_feather_materialise(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_materialise");
  if (!h->feather) return fail(SF_ERR_STATE, "sf_feather_materialise: no feather state (sf_feather_attach)");
  DevGuard dev_guard(h->cfg.device);
  return feather_materialise(h);
} SF_CATCH

int sf_feather_adjoint(sf_handle* h) try {
  if (!h) return fail(SF_ERR_INVALID, "null argument");
  SF_NO_RENDER(h, "sf_feather_adjoint");
  if (!h->feather) return fail(SF_ERR_STATE, "sf_feather_adjoint: no feather state (sf_feather_attach)");
  DevGuard dev_guard(h->cfg.device);
  return feather_adjoint(h);
} SF_CATCH

/* test aid: throws inside the boundary on purpose (0: std::bad_alloc, 1: std::runtime_error, 2: a non-std exception) */
int sf_debug_throw(int32_t kind) try {
  if (kind == 0) throw std::bad_alloc();
  if (kind == 1) throw std::runtime_error("sf_debug_throw");
  if (kind == 2) throw 42;
  return SF_OK;
} SF_CATCH

}  // extern "C"

#include "siren_render.hip"
#include "wavelet_render.hip"
#include "fourier_render.hip"
