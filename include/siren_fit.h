/*
 * siren_fit.h — C ABI of libsiren_fit.so, the MI355X (gfx950) SIREN fitting engine.
 *
 * One handle == one per-image fit == one HIP stream on one device.  The library replaces
 * the arithmetic of ONE hot path of varun19299/implicit-image-compression (citations are
 * relative to the reference tree):
 *
 *   implicit_image/data.py:78-88              get_grid         -> sf_set_coords (two 1-D linspace vectors)
 *   implicit_image/models/siren.py:56-68      SineLayer.forward \
 *   implicit_image/models/siren.py:123-134    Siren.forward      > sf_forward / sf_forward_backward
 *   implicit_image/utils/train_helper.py:147-161  mse_loss + backward (autograd) /
 *   implicit_image/utils/train_helper.py:166-177  optimiser step (torch.optim.Adam, conf/optim/adam.yaml)
 *   implicit_image/pipeline/masking/core.py:271-279,671-702  Masking.step -> apply_mask   -> sf_adam_step
 *   implicit_image/pipeline/masking/core.py:713-801 (+ funcs/prune.py:24-51, funcs/grow.py:58-97, core.py:250-269)
 *                                                 update_connections of RigL              -> sf_mask_update
 *   implicit_image/utils/train_helper.py:41-59    eval_epoch (fwd, MSE)                   -> sf_forward
 *   implicit_image/utils/train_helper.py:52       (pred * 255).int()   -> sf_render / sf_wavelet_render (8-bit samples);
 *                                                 one sample width up: sf_render16 / sf_wavelet_render16 (pred * 65535)
 *
 * Conventions
 *   - every function returns 0 on success, a negative sf_status otherwise; the message is
 *     available from sf_last_error() (never throws, never exits);
 *   - pointers named *_dev are DEVICE pointers owned by the caller (e.g. torch tensor.data_ptr());
 *     the engine never frees them.  sf_set_target BORROWS its pointer: the image must stay
 *     alive and unchanged until the next sf_set_target or sf_destroy;
 *   - "flat" parameter order is the reference's named_parameters() order
 *     (layers.0.linear.weight, layers.0.linear.bias, layers.1.linear.weight, ...), weights in
 *     nn.Linear layout [out][in] row-major, fp32;
 *   - all work is enqueued on the handle's stream; functions that return host scalars
 *     (loss_out / sse_out != NULL) synchronise that stream, the others do not;
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef SIREN_FIT_H_
#define SIREN_FIT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_ABI_VERSION 3   /* 3: FourierNet handles (sf_fourier_create, sf_set_encoding) */

typedef enum sf_status {
  SF_OK = 0,
  SF_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
  SF_ERR_HIP = -2,         /* a HIP runtime call failed                */
  SF_ERR_NO_DEVICE = -3,   /* no gfx950 device visible                 */
  SF_ERR_STATE = -4,       /* call order violated (e.g. step before set_target) */
  SF_ERR_NOMEM = -5
} sf_status;

/* arithmetic type of the hidden-layer GEMM operands (accumulation is always fp32,
 * layer 0 and all optimiser state are always fp32) */
typedef enum sf_dtype {
  SF_BF16 = 0,   /* bf16 operands, 1 MFMA per product                                  */
  SF_F16 = 1,    /* fp16 operands (11-bit significand), gradients pre-scaled            */
  SF_BF16X3 = 2  /* forward operands split hi+lo in bf16 (3 MFMAs per forward product)  */
} sf_dtype;

typedef struct sf_config {
  int32_t abi_version;      /* SF_ABI_VERSION                                            */
  int32_t height, width;    /* full image H, W: the loss mean is over 3*H*W (train_helper.py:151) */
  int32_t row_begin, row_end; /* rows [row_begin,row_end) fitted by THIS handle (pixel-split); 0,H = all */
  int32_t in_features;      /* 2  (siren.py:74)  */
  int32_t out_features;     /* 3  (siren.py:75)  */
  int32_t hidden;           /* mlp.hidden_size after the small-dense scaling (siren.py:88) */
  int32_t depth;            /* number of Linear layers incl. first and last (siren.py:90-118) */
  float first_omega_0;      /* conf/mlp/siren.yaml:5 */
  float hidden_omega_0;     /* conf/mlp/siren.yaml:6 */
  int32_t outermost_linear; /* 1: last layer has no sine (siren.py:114) */
  int32_t compute_dtype;    /* sf_dtype */
  float beta1, beta2, eps;  /* Adam (torch.optim.Adam defaults 0.9, 0.999, 1e-8) */
  int32_t device;           /* HIP device ordinal */
  void* stream;             /* hipStream_t to enqueue on (NULL = the device's null stream) */
  int64_t chunk_pixels;     /* pixels processed per kernel sweep (0 = auto) */
  int32_t scratch_format;   /* width of the two tensors the backward re-reads from HBM (phases, deltas):
                             * 16 = unorm16 phases + 16-bit float deltas (round-1 format);
                             * 12 = phase BYTES + 16-bit float deltas;
                             *  8 = phase bytes + fp8 e4m3 deltas under one power-of-two scale per pixel chunk (from the
                             *      chunk's residual) times one per layer (from the layer's weight norm);
                             *  0 = auto, SF_F16 only (8 and 12 need fp16 operands; else 16): hidden <= 256: 8 for images of
                             *      >= 2^20 pixels, 12 below; hidden > 256: from 2^20 pixels 8 up to hidden 512 and 12 above
                             *      (8 is accepted there when asked for), 16 below.  An auto handle moves to 16 when sf_set_masks sets a mask
                             *      (sparse networks: DESIGN.md section 2)                                             */
} sf_config;

typedef struct sf_engine sf_handle;

/* FourierNet (reference implicit_image/models/fourier.py): encoding [sin(2 pi x B), cos(2 pi x B)] of width map_size,
 * then Linear(map_size, hidden) + ReLU, (n_linear - 2) x [Linear(hidden, hidden) + ReLU], Linear(hidden, 3) + Sigmoid.
 * The handle is an ordinary sf_handle: every call below works on it, with these differences
 *   - the flat parameter vector holds the Linear layers only (layers.{2l}.weight, layers.{2l}.bias); encoding.B is frozen
 *     and goes in through sf_set_encoding, once per bind, before the first pass;
 *   - sf_scratch_format reports 16; sf_debug_scratch returns SF_ERR_INVALID; the whole image is fitted (no pixel split);
 *   - sf_render draws it (bytes and / or fp32), on a training handle and on the inference-only handle of
 *     sf_fourier_render_create, which takes this config too (height / width: the picture to render; the Adam fields are
 *     ignored). */
typedef struct sf_fourier_config {
  int32_t abi_version;      /* SF_ABI_VERSION                              */
  int32_t height, width;    /* image H, W: the loss mean is over 3*H*W     */
  int32_t in_features;      /* 2                                           */
  int32_t out_features;     /* 3                                           */
  int32_t map_size;         /* 64, 128, 256 or 512 (fourier.py:13)         */
  int32_t hidden;           /* 32, 64, 128 or 256 (Small_Dense widths: zero-pad on the host) */
  int32_t n_linear;         /* Linear layers, 2..12 (depth 8 of conf/mlp/fourier.yaml = 7)  */
  int32_t compute_dtype;    /* SF_F16 only                                 */
  float beta1, beta2, eps;  /* Adam                                        */
  int32_t device;           /* HIP device ordinal                          */
  void* stream;             /* hipStream_t (NULL = null stream)            */
  int64_t chunk_pixels;     /* pixels per kernel sweep (0 = auto)          */
} sf_fourier_config;

/* WaveletSiren (reference implicit_image/models/wavelet_siren.py): two SIRENs, LF (Y_LL, Cb, Cr) and HF (the detail bands
 * LH, HL, HH), on one n x n coefficient grid, n = (H + 5) / 2; the image is the db3 / zero-mode inverse DWT for Y, bilinear
 * upsampling of Cb and Cr, and YCbCr -> RGB (wavelet_kernels.hip).  The handle is an ordinary sf_handle: every call above
 * and below works on it, with these differences
 *   - the flat vector is [LF layers | HF layers] in the reference's named_parameters() order (LF_siren.layers.{i}.linear.*,
 *     then HF_siren.*); sf_param_offset numbers the layers 0 .. 2 depth - 1 the same way;
 *   - sf_set_coords takes the two linspace(0, 1, n) vectors of the coefficient grid; sf_set_target the H x H x 3 image;
 *     sf_forward writes the H x H x 3 RGB prediction and the SSE over 3 H^2 values;
 *   - sf_scratch_format reports 16; sf_debug_scratch and sf_feather_attach return SF_ERR_INVALID. */
typedef struct sf_wavelet_config {
  int32_t abi_version;      /* SF_ABI_VERSION                                              */
  int32_t height, width;    /* image H = W, even (the reference's shapes stop matching otherwise) */
  int32_t in_features;      /* 2                                                           */
  int32_t out_features;     /* 3                                                           */
  int32_t hidden;           /* 32, 64, 128 or 256 (Small_Dense widths: zero-pad on the host) */
  int32_t depth;            /* Linear layers of each sub-network, 2..16                    */
  int32_t wavelet_levels;   /* 1                                                           */
  float first_omega_0, hidden_omega_0;
  int32_t outermost_linear;
  int32_t compute_dtype;    /* SF_F16 only                                                 */
  float beta1, beta2, eps;  /* Adam                                                        */
  int32_t device;           /* HIP device ordinal                                          */
  void* stream;             /* hipStream_t (NULL = null stream)                            */
  int64_t chunk_pixels;     /* coefficient-grid pixels per sweep of a sub-network (0 = auto, 4 Mi): a grid of more
                             * pixels than one chunk runs in two passes */
  int32_t scratch_format;   /* 0 (auto) or 16                                              */
} sf_wavelet_config;

/* lifecycle */
int sf_create(const sf_config* cfg, sf_handle** out);
int sf_destroy(sf_handle* h);
int sf_fourier_create(const sf_fourier_config* cfg, sf_handle** out);
int sf_wavelet_create(const sf_wavelet_config* cfg, sf_handle** out);
/* test aid: one composition kernel of a WaveletSiren handle on caller buffers, enqueued on the handle's stream.
 * which 0 (k_wv_compose): in0 / in1 the LF / HF predictions [n*n][3], img [H*H][3] (may be NULL) -> out0 the RGB prediction
 *   [H*H][3], out1 dL/d(Y, Cb, Cr) [H*H][3] (written when img is given; the SSE partials stay in the handle);
 * which 1 (k_wv_adjoint, unscaled): in0 dL/d(Y, Cb, Cr) [H*H][3] -> out0 / out1 dL/dp of LF / HF [n*n][3] (fp32) */
int sf_wavelet_debug(sf_handle* h, int32_t which, const float* in0, const float* in1, const float* img, float* out0,
                     float* out1);
int sf_set_encoding(sf_handle* h, const float* B_dev /* [in_features][map_size/2] fp32, copied */);
const char* sf_last_error(void);            /* thread-local message of the last failure */
int sf_abi_version(void);

/* shapes */
int sf_num_params(const sf_handle* h, int64_t* n_params);          /* P, length of every flat vector */
int sf_scratch_format(const sf_handle* h, int32_t* format);        /* the format in use (8 / 12 / 16): what 0 resolved to */
int sf_param_offset(const sf_handle* h, int32_t layer, int64_t* weight_off, int64_t* bias_off);

/* model state: flat fp32 vectors of length P on the device */
int sf_set_params(sf_handle* h, const float* flat_dev);
int sf_get_params(sf_handle* h, float* flat_dev);
int sf_set_masks(sf_handle* h, const float* flat_dev);   /* 0/1 per parameter (1 for biases); NULL = dense */
int sf_get_grads(sf_handle* h, float* flat_dev);         /* dense gradient of the last forward_backward   */
int sf_set_grads(sf_handle* h, const float* flat_dev);   /* e.g. after an all-reduce over ranks           */
int sf_get_adam_state(sf_handle* h, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t* step);
int sf_set_adam_state(sf_handle* h, const float* exp_avg_dev, const float* exp_avg_sq_dev, int64_t step);
/* direct device views of engine-owned state (valid until sf_destroy); which: 0 params, 1 grads,
 * 2 exp_avg, 3 exp_avg_sq, 4 masks */
int sf_state_ptr(sf_handle* h, int32_t which, float** dev_ptr);
/* device address of the engine's sum-of-squared-residuals scalar (double) that the last sf_forward /
 * sf_forward_backward wrote on the handle's stream: pixel-split ranks all-reduce it together with the gradient
 * view instead of synchronising for the host value */
int sf_sse_ptr(sf_handle* h, double** dev_ptr);
/* test / debugging aid: device address and size in bytes of an engine scratch tensor of the last pass.
 * which: 0 phases (all layers, layer stride = bytes / (depth-1)), 1 deltas, 2 dL/dout, 3 per-workgroup slabs */
int sf_debug_scratch(sf_handle* h, int32_t which, void** dev_ptr, int64_t* bytes);
/* 1-D k-means quantisation of one weight tensor on the handle's stream, NO host synchronisation.  Replaces
 * pipeline/quant/kmeans.py:110-150 (find_centroids) + kmeans_helper.py:59-115 (kmeans_fit / kmeans_predict).
 *   w_dev [n]            the weights (device); zeros are excluded from the fit, included in the prediction
 *   centers_dev [K]      in: the initial guess - torch.linspace(min, max, K) over the non-zero weights, K = 2^bits - 1
 *                        (kmeans.py:125-131); out: the Lloyd centres after <= iter_limit iterations (tol on (sum |dc|)^2)
 *   centroids_dev [cap]  out: {0} U centres -> unique -> ordered by |c|, zero padded (cap >= K + 1)
 *   n_centroids_dev      out (device int, may be NULL): how many of them are real
 *   labels_dev [n]       out (may be NULL): argmin of the squared distance, first index wins (int64, as torch.argmin)
 *   new_weight_dev [n]   out (may be NULL): centroids[labels]
 * Needs n > 0, 2 <= K < 512, cap >= K + 1, iter_limit >= 0 (SF_ERR_INVALID otherwise, nothing is launched).
 * PRECONDITION: every non-zero weight is at most max(|centers[0]|, |centers[K-1]|) in magnitude.  The 64-bit fixed-point
 * unit of the segment sums is sized from those two ends; the linspace guess gives it for K >= 2 (for K = 1 the guess is the
 * minimum alone, which is why K = 1 is refused).  A guess that does not bracket the weights overflows the sums.
 * EMPTY CALL: a guess whose first or last entry is not finite - torch.linspace(inf, -inf, K), what the masked min / max
 * give for a tensor without a non-zero weight - is decided on the device, without a host read: centers_dev is left as it
 * is, centroids = {+0.0} (n_centroids 1, zero padded), every label 0, every new weight +0.0.  (The reference raises on
 * the empty .min(); INTEGRATION.md section 4 records the departure.) */
int sf_kmeans_fit(sf_handle* h, const float* w_dev, int64_t n, float* centers_dev, int32_t K, int32_t iter_limit, float tol,
                  float* centroids_dev, int32_t centroids_cap, int32_t* n_centroids_dev, int64_t* labels_dev,
                  float* new_weight_dev);
/* The quantise phase of a fit on the handle's stream (csrc/siren_quant.hip, quant_host.hip): what KmeansQuant's forward-pre
 * and backward hooks do per quantised Linear (pipeline/quant/kmeans.py:66-72,110-150,163-181), batched over the layers - one
 * launch serves all of them - and without a device-to-host copy or a host synchronisation.
 *   layers [n_layers]    ascending layer indices of the handle, each with its caller-owned device buffers:
 *     centers_dev [K]        out: the guess, then the Lloyd centres (what the single-tensor call leaves in centers_dev)
 *     centroids_dev [K + 1]  out: the centroids, zero padded; the nudge updates them in place
 *     n_centroids_dev        out (device int, may be NULL): how many of them are real
 *     labels_dev [n]         out: int64 labels of the layer's weights; the nudge reads them
 *   K = 2^bits - 1, iter_limit, tol: as the single-tensor call takes them; nudge_lr: the learning rate of the nudge
 * sf_quant_pass: per layer the guess on the device - min / max over the non-zero weights, then the K entries of
 *   torch.linspace(min, max, K) in ATen's fp32 form: step = (max - min) / (K - 1), entry i = fma(step, i, min) below K / 2 and
 *   fma(-step, K - 1 - i, max) from there on; a layer without a non-zero weight gets non-finite ends, the EMPTY CALL above -,
 *   <= iter_limit Lloyd iterations, the centroids, the labels, and the codebook weights centroids[labels] written straight
 *   into the handle's parameters (the weight images are marked dirty).  The arithmetic is the single-tensor call's, bit for
 *   bit.  3 + 2 * iter_limit launches whatever n_layers.
 * sf_quant_nudge: centroids[k] -= nudge_lr * (sum of the handle's dL/dW over the weights labelled k), all K + 1 entries.  The
 *   segment sums are 64-bit fixed-point integer adds in the unit 2^(60 - ln - e), n < 2^ln, max|g| < 2^e (1 for a zero or
 *   non-finite maximum): the result does not depend on the order of arrival.  A sum is rounded once to float, then
 *   c - nudge_lr * dw in fp32 (two roundings).  One launch.
 * sf_quant_step: n_steps x (pass, forward_backward, nudge, Adam with lr[i]), launch by launch (never the graph replay of
 *   sf_step); loss_out (host, may be NULL) receives the MSE of every step through the device loss table, read once at the
 *   end - the call's only synchronisation, none with NULL.
 * SF_ERR_INVALID before anything is launched or written: a null pointer, a wrong abi_version, a render handle, a FourierNet
 * or WaveletSiren handle, an attached Feathermap, n_layers outside 1 .. depth, a layer index out of range or not ascending,
 * K < 2 or K >= 512, iter_limit < 0; sf_quant_step without coordinates or a target: SF_ERR_STATE.  Every hidden width of
 * sf_create is served (the flat layout is the same at 512 / 1024). */
typedef struct sf_quant_layer {
  int32_t layer;
  float* centers_dev;
  float* centroids_dev;
  int32_t* n_centroids_dev;
  int64_t* labels_dev;
} sf_quant_layer;
typedef struct sf_quant_args {
  int32_t abi_version;      /* SF_ABI_VERSION */
  int32_t n_layers;
  const sf_quant_layer* layers;
  int32_t K, iter_limit;
  float tol, nudge_lr;
} sf_quant_args;
int sf_quant_pass(sf_handle* h, const sf_quant_args* a);
int sf_quant_nudge(sf_handle* h, const sf_quant_args* a);
int sf_quant_step(sf_handle* h, const sf_quant_args* a, const float* lr, int32_t n_steps, float* loss_out);
/* One RigL topology update (Masking.update_connections of the reference: pipeline/masking/core.py:713-801 with
 * funcs/prune.py:24-51 magnitude_prune, funcs/grow.py:58-97 abs_grad_growth, core.py:250-269 adjust_prune_rate) on the
 * handle's stream: two launches whatever the depth, NO device-to-host copy and no host synchronisation (csrc/siren_mask.hip).
 * The state is the handle's flat fp32 vectors: params w, grads g, Adam m and v, masks k (0/1, sf_set_masks).
 *   layers [n_layers]  host array: the engine layer indices, ascending, whose WEIGHT is masked (biases never are;
 *                      sparse_init=random leaves the first layer out)
 *   prune_rate         the current rate r of the decay schedule
 *   growth             0 none, 1 absolute gradient
 *   dense_gradients    0: the moments and the gradient are masked too
 *   stats_dev          device, n_layers rows + one status row, may be NULL
 * Per masked layer j, a flat slice of n elements (counts are exact integers, rate arithmetic is IEEE double):
 *   1. live = #{k == 1}, dead = #{k == 0}, nnz = #{w != 0};  S = sum of nnz over the listed layers
 *   2. share = nnz / S, frac_dead = dead / n;  rate = min(frac_dead, r) if frac_dead < 0.2 && (1.0 / n_layers) / share < 1.0,
 *      else r
 *   3. drop = ceil(rate * live)
 *   4. drop > 0: the dead + drop elements smallest in (|w_i|, i), lexicographically, get k_i = 0;  removed = live - sum k
 *   5. growth 1, unless every k_i of the layer is 1 after pruning: c_i = |g_i| * (1 - k_i) as an fp32 product; the `removed`
 *      elements largest in c_i, ties to the lower index, get k_i = 1 and w_i = +0.0
 *   6. w_i *= k_i (a product, as on the host: a pruned negative weight becomes -0.0); dense_gradients == 0: also m_i *= k_i,
 *      v_i *= k_i, g_i *= k_i.  The weight images are marked dirty
 *   7. row j: live, dead, nnz before; removed; live, dead, nnz after; rate
 * S == 0 leaves the state untouched and sets live_before of the status row (row n_layers, otherwise all zero) to 1.
 * Ties: the host's torch.sort orders equal keys arbitrarily; here the lower index comes first.  The two agree whenever the
 * value at the selection boundary is unique.
 * SF_ERR_INVALID / SF_ERR_STATE, before anything is launched: a null pointer, a wrong abi_version, a render handle, a
 * FourierNet or WaveletSiren handle, a handle with Feathermap attached, no masks set (SF_ERR_STATE), a layer index out of
 * range or not ascending, a growth mode other than 0 or 1.  Hidden 512 / 1024 handles are supported (the same flat layout). */
typedef struct sf_mask_layer_stats {
  int64_t live_before, dead_before, nnz_before, removed, live_after, dead_after, nnz_after;
  double prune_rate;
} sf_mask_layer_stats;
typedef struct sf_mask_update_args {
  int32_t abi_version, n_layers;
  const int32_t* layers;
  double prune_rate;
  int32_t growth, dense_gradients;
  sf_mask_layer_stats* stats_dev;
} sf_mask_update_args;
int sf_mask_update(sf_handle* h, const sf_mask_update_args* a);
/* One global-magnitude topology update (masking=Pruning: Masking.update_connections of the reference with
 * funcs/prune.py:54-104 global_magnitude_prune and growth_mode none) on the handle's stream: six launches whatever the depth
 * and however many trials the threshold search takes, NO device-to-host copy and no host synchronisation (csrc/siren_mask.hip).
 * The state is the handle's flat fp32 vectors, as for sf_mask_update.
 *   layers [n_layers]  host array: the engine layer indices, ascending, whose WEIGHT is masked
 *   target             ceil(prune_rate * baseline_nonzero): how many live weights the threshold should remove
 *   prune_rate         the current rate r of the decay schedule (bookkeeping of step 2 only)
 *   threshold          the threshold the search starts from (Masking.prune_threshold)
 *   increment          the first relative nudge (Masking.increment), tolerance: the relative slack (Masking.tolerance)
 *   dense_gradients    0: the moments and the gradient are masked too
 *   stats_dev          device, n_layers rows + one status row, may be NULL
 * Counts are exact integers; all threshold arithmetic is IEEE double, round to nearest, no FMA contraction, no fast-math:
 *   1. per listed layer j: live_j = #{k == 1}, dead_j = #{k == 0}, nnz_j = #{w != 0}; S = sum nnz_j, alive = sum live_j.
 *      S == 0 leaves the state untouched and sets status 1
 *   2. rate_j: step 2 of sf_mask_update with r = prune_rate
 *   3. target <= 0: no search - the masks keep their values, removed = 0, trials = 0, the threshold is unchanged; steps 6 and 7 run
 *   4. slack = target * tolerance; step = increment; removed = previous = stalled = 0
 *      while |removed - target| > slack:
 *        a. removed = alive - #{ i in the listed layers : |w_i| > f32(threshold) }; trials += 1
 *           (f32: the double rounded to fp32, to nearest-even; an fp32 `>` over every element, dead ones included)
 *        b. stalled = stalled + 1 if removed == previous else 0
 *        c. if stalled == 10: break                (before any nudge)
 *        d. previous = removed
 *        e. if   removed > target * (1.0 + tolerance): threshold *= 1.0 - step; step *= 0.99
 *           elif removed < target * (1.0 - tolerance): threshold *= 1.0 + step; step *= 0.99
 *      (target converts to double exactly.)  The loop evaluates at most 4096 trials (kPruneTrialCap): a search that would
 *      evaluate one more sets status 2 and leaves masks, state and threshold untouched.  The loop itself stalls long before
 *      
 *   5. a search ran: k_i = |w_i| > f32(threshold) ? 1 : 0 for every element of the listed layers, with the final threshold
 *   6. w_i *= k_i (a product: a pruned negative weight becomes -0.0); dense_gradients == 0: also m_i *= k_i, v_i *= k_i,
 *      g_i *= k_i.  The weight images are marked dirty
 *   7. row j: live, dead, nnz before; removed = live_before - live_after; live, dead, nnz after; rate_j.
 *      The status row (row n_layers), as eight 64-bit words in the order of the sf_mask_layer_stats fields:
 *        [0] live_before = status (0 done, 1 S == 0, 2 trial cap)   [1] dead_before = trials   [2] nnz_before = alive
 *        [3] removed = the last count the search evaluated (0 without a search: what the host function returns)
 *        [4] live_after = target   [5] dead_after = 0   [6] nnz_after = 0
 *        [7] prune_rate = the final threshold, a double (status 1 or 2: the threshold passed in)
 *      With status 1 or 2 rows 0 .. n_layers - 1 hold the counts before, copied to the counts after, removed 0, rate 0.
 * There is no tie rule: the mask is a function of each value alone, so the device result equals the host path's bit for bit.
 * SF_ERR_INVALID / SF_ERR_STATE, before anything is launched: everything sf_mask_update refuses (a null pointer, a wrong
 * abi_version, a render handle, a FourierNet or WaveletSiren handle, a handle with Feathermap attached, no masks set
 * (SF_ERR_STATE), a layer index out of range or not ascending), a threshold that is not finite and > 0, an increment outside
 * (0, 1), a negative or non-finite tolerance, a negative target.  The first call allocates 4 bytes per parameter of key
 * scratch on the handle (freed with it). */
typedef struct sf_mask_prune_global_args {
  int32_t abi_version, n_layers;
  const int32_t* layers;
  int64_t target;
  double prune_rate, threshold, increment, tolerance;
  int32_t dense_gradients;
  sf_mask_layer_stats* stats_dev;
} sf_mask_prune_global_args;
int sf_mask_prune_global(sf_handle* h, const sf_mask_prune_global_args* a);
/* One SNFS topology update (masking=SNFS: Masking.update_connections of the reference with magnitude_prune, growth by
 * |momentum| (funcs/grow.py:25-55) or |gradient|, and the regrowth redistributed by a per-layer statistic: core.py:425-464
 * gather_statistics, funcs/redistribute.py:18-37, core.py:299-360 calc_redistributed_densities) on the handle's stream: three
 * launches whatever the depth and however many rounds the redistribution takes, NO device-to-host copy and no host
 * synchronisation (csrc/siren_mask.hip).  The state is the handle's flat fp32 vectors, as for sf_mask_update.
 *   layers [n_layers]  host array: the engine layer indices, ascending, whose WEIGHT is masked
 *   prune_rate         the current rate r of the decay schedule
 *   adjusted_growth    Masking.adjusted_growth: what the pool of regrown weights holds beyond the weights removed, >= 0
 *   growth             1 absolute gradient, 2 momentum
 *   statistic          0 the non-zero count (redistribution none / nonzero), 1 the mean |momentum| of the live weights
 *   dense_gradients    0: the moments and the gradient are masked too
 *   stats_dev          device, n_layers rows + one status row of sf_mask_snfs_stats, may be NULL
 * Counts are exact integers; every double operation is IEEE round to nearest and none is contracted into an FMA;
 * mom_i = m_i / (sqrt(v_i) + 1e-8f) is three fp32 operations, each rounded to nearest (get_momentum_for_weight under Adam).
 *   1. per listed layer j (n elements): live_j, dead_j, nnz_j as step 1 of sf_mask_update
 *   2. statistic 0: stat_j = (double)nnz_j.  statistic 1, with a_i = |mom_i|:
 *        amax_j = the largest a_i over EVERY element of the layer (an integer max on the bits); a non-finite a_i, or
 *        live_j == 0, gives status 3 and leaves the state untouched (the host's round(nan) raises)
 *        e: amax_j < 2^e (frexp; that of 1.0 when amax_j == 0); ln: the least with n + 1 <= 2^ln; s = 60 - ln - e
 *        A_j = sum over k_i == 1 of llrint((double)a_i * 2^s), a 64-bit integer: no order of summation changes it, and it
 *        cannot overflow (every term is at most 2^(60 - ln) and there are fewer than 2^ln of them)
 *        stat_j = ((double)A_j * 2^-s) / (double)live_j
 *      norm = sum of stat_j in layer order from 0.0; norm == 0 gives status 1 and leaves the state untouched (the host's
 *      "Total variance is zero!"); status 3 comes first.  share_j = stat_j / norm
 *   3. rate_j: step 2 of sf_mask_update with this share_j; drop_j = ceil(rate_j * live_j); the prune of step 4 there: the
 *      dead_j + drop_j elements smallest in (|w_i|, i) get k_i = 0 -> removed_j
 *   4. statistic 0: budget_j = removed_j.  statistic 1 (calc_redistributed_densities, literally): R = sum removed_j,
 *      pool = (double)R + adjusted_growth, cap_j = 0.99 * (double)(dead_j + removed_j), budget_j = rint(share_j * pool), half to
 *      even, share = 0; then at most 1000 rounds: excess = 0; for j ascending { want = budget_j + share; if want > cap_j
 *      { excess += want - cap_j; want = cap_j }; budget_j = want }; share = excess / (double)n_layers; the loop ends after a
 *      round whose excess is not > 0.  Each of these is one double operation, in this order.  grown_j = (int)budget_j, truncated
 *   5. grown_j > 0.  growth 2: c_i = |mom_i * (1 - k_i)| as an fp32 product with k after the prune; the grown_j elements
 *      largest in c_i, ties to the lower index, get k_i = 1.  w_i is NOT written: a weight pruned in step 3 and grown here
 *      keeps its value, as momentum_growth leaves it.  growth 1: step 5 of sf_mask_update with grown_j in place of removed
 *      (w_i = +0.0)
 *   6. step 6 of sf_mask_update: w_i *= k_i; dense_gradients == 0: also m_i, v_i, g_i.  The weight images are marked dirty
 *   7. row j: the eight words of sf_mask_layer_stats with the same meaning; stat_before = stat_j; budget = budget_j, the
 *      double before truncation; grown = grown_j; stat_after = step 2's statistic over the state steps 5 and 6 left (statistic
 *      1: NaN when no weight of the layer is live; gather_statistics leaves such a layer out of the norm).
 *      The status row (row n_layers), as twelve 64-bit words in the order of the sf_mask_snfs_stats fields:
 *        [0] status (0 done, 1 norm == 0, 3 no statistic)   [1] the rounds of step 4 (0 with statistic 0)   [2] R
 *        [3] sum of grown_j   [7] pool, a double   [8] norm, a double   [11] the norm after: the stat_after that are not NaN
 *        summed in layer order, a double; every other word 0
 *      With status 1 or 3 rows 0 .. n_layers - 1 hold the counts before, copied to the counts after, and zeros; the status
 *      row holds the status and zeros.
 * With growth 1 and statistic 0 the five state vectors equal sf_mask_update's bit for bit.  Ties are broken as there.
 * SF_ERR_INVALID / SF_ERR_STATE, before anything is launched: everything sf_mask_update refuses, a growth other than 1 or
 * 2, a statistic other than 0 or 1, an adjusted_growth that is negative or not finite. */
typedef struct sf_mask_snfs_stats {
  int64_t live_before, dead_before, nnz_before, removed, live_after, dead_after, nnz_after;
  double prune_rate;
  double stat_before, budget;
  int64_t grown;
  double stat_after;
} sf_mask_snfs_stats;
typedef struct sf_mask_update_snfs_args {
  int32_t abi_version, n_layers;
  const int32_t* layers;
  double prune_rate, adjusted_growth;
  int32_t growth;            /* 1 absolute gradient, 2 momentum */
  int32_t statistic;         /* 0 non-zero count, 1 momentum */
  int32_t dense_gradients;
  sf_mask_snfs_stats* stats_dev;
} sf_mask_update_snfs_args;
int sf_mask_update_snfs(sf_handle* h, const sf_mask_update_snfs_args* a);
/* test aid for the "never throws" promise above: raises inside the library on purpose (0: std::bad_alloc -> SF_ERR_NOMEM,
 * 1: std::runtime_error, 2: a non-std exception -> SF_ERR_INVALID); every entry point is a function-try-block */
int sf_debug_throw(int32_t kind);
/* tell the engine that the caller wrote the parameters through the sf_state_ptr(…,0) view */
int sf_params_changed(sf_handle* h);

/* data: the two linspace vectors of get_grid (data.py:82-83) and the target image rows.  rows / cols must be
 * torch.linspace(0, 1, n) to within 2e-6 (the layer-0 gradient kernels re-derive coordinates as i/(n-1));
 * anything else returns SF_ERR_INVALID */
int sf_set_coords(sf_handle* h, const float* rows_dev /*[height]*/, const float* cols_dev /*[width]*/);
int sf_set_target(sf_handle* h, const float* img_dev /*[(row_end-row_begin)*width*3], borrowed*/);

/* the hot path */
/* forward only (eval_epoch): pred_dev may be NULL; sse_out (host) = sum of squared residuals over
 * this handle's rows (double), NULL = do not synchronise */
int sf_forward(sf_handle* h, float* pred_dev, double* sse_out);
/* one evaluation pass over the handle's rows: no prediction is written.  *sse_out: the double sf_forward reports, bit for
 * bit.  *sse8_out: sum over the handle's pixels and channels of ((int)(255 t) - (int)(255 p))^2, exact.  Both NULL: the pass is
 * enqueued and nothing is read; the sums stay where sf_sse_ptr / sf_sse8_ptr point.  Otherwise ONE copy and ONE synchronise.
 *   - t: the fp32 target, p: the fp32 prediction sf_forward would store; the products in fp32, truncated toward zero and NOT
 *     clamped - eval_epoch's (x * 255).int() (train_helper.py), not the samples of sf_render.  The squares are summed in
 *     64-bit integers (per lane, per workgroup, then one fixed-order reduction), so the sum is exact and deterministic;
 *   - the pass runs the EVAL forms of the forward kernels: they store the two kinds of per-workgroup partials and nothing
 *     else (the sub-network forwards of a WaveletSiren handle still fill its coefficient predictions, as sf_forward's do).
 *     The integer partials live in a buffer of the handle, allocated at the first call;
 *   - every training handle takes it: SIREN of every width (with Feathermap attached, with a pixel-split row range),
 *     FourierNet, WaveletSiren.  Parameters, gradients, moments, masks and what a following sf_step computes are untouched;
 *   - refused before anything is allocated or launched, "sf_eval" in the message: a null handle (SF_ERR_INVALID, no GPU
 *     touched), a render handle (SF_ERR_INVALID), no coordinates, no target, FourierNet without sf_set_encoding
 *     (SF_ERR_STATE).
 * sf_sse8_ptr: device address of the integer sum the last sf_eval wrote (the word behind sf_sse_ptr's double). */
int sf_eval(sf_handle* h, double* sse_out, uint64_t* sse8_out);
int sf_sse8_ptr(sf_handle* h, uint64_t** dev_ptr);
/* forward + loss + backward: leaves the dense gradient (already scaled by 1/(3*H*W)) in the
 * engine; sse_out as above */
int sf_forward_backward(sf_handle* h, double* sse_out);
/* Inference only (csrc/siren_render.hip): what a decoder needs and nothing of a training step.
 * sf_render_create takes sf_create's config and validation (height / width: the picture to render, any size) for hidden
 * 32 / 64 / 128 / 256 and allocates the parameters, the forward weight images, the layer-0 table / image and the two
 * coordinate vectors - no gradient, Adam moments, mask, phase / delta scratch or slabs (hidden 512 / 1024: SF_ERR_INVALID,
 * the render kernel is not built for the wide path; sf_wide_render_create below makes that handle).  On such a handle sf_set_params, sf_get_params, sf_params_changed,
 * sf_set_coords (any two vectors: a window of a grid is a slice of them), sf_num_params, sf_param_offset, sf_state_ptr(0),
 * sf_destroy and the profiling calls work; every training entry point returns SF_ERR_INVALID.
 * sf_fourier_render_create (csrc/fourier_render.hip) is the same for FourierNet: sf_fourier_create's config, validation and
 * geometry; it allocates the parameters, the fp16 weight images, encoding.B and the two coordinate vectors - none of the
 * [n_linear - 1][hidden][chunk] activation / gradient planes, slabs, gradient, Adam moments, mask or SSE partials.  The same
 * calls work on it, plus sf_set_encoding; every training entry point returns SF_ERR_INVALID.
 * sf_render writes rows [row_begin, row_end) of the handle - a SIREN render handle, an ordinary SIREN training handle of
 * hidden <= 256, a FourierNet render handle or a FourierNet training handle (WaveletSiren: sf_wavelet_render) - on the
 * handle's stream, no host synchronisation.  A call before sf_set_coords (FourierNet: or before sf_set_encoding) returns
 * SF_ERR_STATE.  Either output may be NULL, not both:
 *   pred_dev [npix][out_features] fp32, bit-identical to what sf_forward writes for the same parameters and coordinates;
 *   rgb8_dev [npix][out_features] bytes (4-byte aligned), u8 = min(max((int)(pred * 255.0f), 0), 255): the product in fp32,
 *            truncated toward zero (eval_epoch's (pred * 255).int(), train_helper.py:52), clamped to what a file can hold.
 * sf_render16 is sf_render at 16 bits per sample - the same handles, refusals, stream and pred_dev, the same kernels with a
 * 16-bit store epilogue:
 *   rgb16_dev [npix][out_features] native-endian uint16_t (4-byte aligned: a base that is only 2-byte aligned is refused),
 *            u16 = min(max((int)(pred * 65535.0f), 0), 65535): the product in fp32, truncated toward zero - the inverse of
 *            the loader's raw / (2^16 - 1).  A NaN prediction gives 0, as in the byte form. */
int sf_render_create(const sf_config* cfg, sf_handle** out);
int sf_render(sf_handle* h, uint8_t* rgb8_dev, float* pred_dev);
int sf_render16(sf_handle* h, uint16_t* rgb16_dev, float* pred_dev);
int sf_fourier_render_create(const sf_fourier_config* cfg, sf_handle** out);
/* Inference only, SIREN of hidden 512 / 1024 (the RENDER forms of the layer-at-a-time kernels, csrc/siren_wide.hip).
 * sf_wide_render_create takes sf_create's config and validation for hidden 512 / 1024 with depth >= 3 (any other width:
 * SF_ERR_INVALID, sf_render_create makes that handle) and allocates the parameters, the blocked forward weight images with
 * their biases, the layer-0 table, the two coordinate vectors and TWO activation planes of chunk_pixels x hidden 16-bit
 * values, which the layers use in turn - no gradient, Adam moments, mask, transposed images, phase / delta planes, per-layer
 * activation planes or slabs.  chunk_pixels = 0 means 2^18 pixels at hidden 512 and 2^17 at 1024 (256 MiB per plane);
 * scratch_format is ignored.  On such a handle the calls listed for sf_render_create work and every training entry point,
 * sf_render, sf_render16 and sf_feather_render_attach return SF_ERR_INVALID.
 * sf_wide_render / sf_wide_render16 are sf_render / sf_render16 for this handle: rows [row_begin, row_end) on the handle's
 * stream, no host synchronisation, pred_dev bit-identical to what sf_forward writes on a training handle of any
 * scratch_format with the same parameters and coordinates, the samples by the same formulas, the same NULL, alignment and
 * sf_set_coords checks.  Any other handle returns SF_ERR_INVALID with the entry point that draws it in the message. */
int sf_wide_render_create(const sf_config* cfg, sf_handle** out);
int sf_wide_render(sf_handle* h, uint8_t* rgb8_dev, float* pred_dev);
int sf_wide_render16(sf_handle* h, uint16_t* rgb16_dev, float* pred_dev);
/* Inference only, WaveletSiren (csrc/wavelet_render.hip).  sf_wavelet_render_create validates what sf_wavelet_create
 * validates and allocates the joint parameter vector [LF | HF], two render sub-handles (parameters as views into it, forward
 * weight images, layer-0 table / image), the two FULL coefficient-grid vectors and ONE pair of fp32 coefficient buffers
 * sized for the coefficient window of a max_rows x max_cols pixel window - no gradient, Adam moments, mask, phase / delta
 * scratch, slabs or image-space gradient.  On such a handle sf_set_params, sf_get_params, sf_params_changed, sf_num_params,
 * sf_param_offset, sf_state_ptr(0), sf_set_coords, sf_destroy and the profiling calls work as on a WaveletSiren training
 * handle; every training entry point, sf_render and sf_set_target return SF_ERR_INVALID.  sf_set_coords takes the two
 * linspace(0, 1, n) vectors of the FULL coefficient grid (n = (height + 5) / 2; unchecked, as on a SIREN render handle) and
 * keeps them: coefficient (i, j) is evaluated at rows[i], cols[j] whatever the window, so a window is bit-identical to the
 * same region of the full picture. */
typedef struct sf_wavelet_render_config {
  int32_t abi_version;      /* SF_ABI_VERSION                                                            */
  int32_t height;           /* side H of the FULL picture (even, square): fixes n and the bilinear scale */
  int32_t max_rows, max_cols; /* the largest pixel window one sf_wavelet_render call will draw (0 = H)   */
  int32_t hidden, depth;    /* as sf_wavelet_config                                                      */
  float first_omega_0, hidden_omega_0;
  int32_t outermost_linear;
  int32_t compute_dtype;    /* SF_F16 only                                                               */
  int32_t device;           /* HIP device ordinal                                                        */
  void* stream;             /* hipStream_t (NULL = null stream)                                          */
  int64_t chunk_pixels;     /* coefficient-grid pixels per sweep of a sub-network (0 = auto)             */
} sf_wavelet_render_config;
int sf_wavelet_render_create(const sf_wavelet_render_config* cfg, sf_handle** out);
/* Draws pixel rows [row0, row1) x columns [col0, col1) of the H x H picture on the handle's stream, no host
 * synchronisation: the RENDER forward of LF and HF over the coefficient window those pixels read (Y: rows o/2 .. o/2 + 2 of
 * output row o; Cb / Cr: the two bilinear source rows; likewise for columns), then k_wv_render.  h is a WaveletSiren render
 * handle or a WaveletSiren training handle (sf_wavelet_create, which uses its own prediction buffers).  Either output may be
 * NULL, not both, dense [row1 - row0][col1 - col0][3]:
 *   pred_dev fp32, bit-identical to what sf_forward writes for those pixels on a training handle with the same parameters;
 *   rgb8_dev bytes (4-byte aligned), u8 = min(max((int)(pred * 255.0f), 0), 255) as sf_render.
 * Empty windows, windows outside [0, H) or larger than max_rows x max_cols return SF_ERR_INVALID; a call before
 * sf_set_coords returns SF_ERR_STATE.
 * sf_wavelet_render16 is the same call at 16 bits per sample: rgb16_dev native-endian uint16_t (4-byte aligned),
 * u16 = min(max((int)(pred * 65535.0f), 0), 65535) as sf_render16. */
int sf_wavelet_render(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, uint8_t* rgb8_dev,
                      float* pred_dev);
int sf_wavelet_render16(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, uint16_t* rgb16_dev,
                        float* pred_dev);
/* Adam (+ mask) on the current gradient with learning rate lr; refreshes the low-precision weight images */
int sf_adam_step(sf_handle* h, float lr);
/* n_steps x (forward_backward + adam_step) with learning rates lr[0..n_steps) (host array);
 * loss_out (host, may be NULL) receives the MSE of every step (length n_steps) */
int sf_step(sf_handle* h, const float* lr, int32_t n_steps, float* loss_out);
/* n_steps training steps of n_fits fits of ONE shape, every kernel of a step launched once for all of them (grid: the single
 * fit's grid x n_fits; csrc/siren_many.hip).  lr: host [n_steps][n_fits]; loss_out: host [n_steps][n_fits] or NULL.
 * For every member b the call is sf_step on h[b] with column b of lr and of loss_out, bit for bit: parameters, gradient,
 * both moments, the step counter, the reported losses, and whatever a later call on the member computes.  The launches per
 * step do not depend on n_fits; they are eager launches on the members' common stream (no graph capture); the call
 * synchronises with the host once, to read the losses, and not at all with loss_out NULL.  The argument tables, the per-step
 * scalars and the step counter live in device memory of h[0]; the profile records of the call are h[0]'s, one per launch.
 * Members may differ in parameters, target, mask (set or not), step count and learning rate.
 * Refused before anything is launched, allocated or changed on any handle, with "sf_step_many" and the offending member's
 * index in the message - SF_ERR_INVALID: a null argument, n_fits < 1 or > SF_STEP_MANY_MAX, n_steps < 0, the same handle
 * twice, a render handle, a FourierNet or WaveletSiren handle, a Feathermap handle, hidden > 128, compute_dtype other than
 * SF_F16, a scratch format other than 16 at the time of the call, more than one chunk, a row range other than the whole
 * picture, members that differ in height, width, hidden, depth, out_features, the omegas, outermost_linear, betas, eps,
 * device or stream; SF_ERR_STATE: coordinates or target not set. */
#define SF_STEP_MANY_MAX 64
int sf_step_many(sf_handle* const* h, int32_t n_fits, const float* lr, int32_t n_steps, float* loss_out);
/* sf_step execution mode for single-chunk fits: 0 (default) = one stream launch per kernel, 1 = capture one
 * training step into a hipGraph and replay it n_steps times.  Results are bit-identical; which is faster is a
 * property of the runtime (measured on ROCm 7.2 / MI355X: eager 73 us/step vs replay 87 us/step at SIREN 64x4
 * on 256x256), so replay stays opt-in. */
int sf_set_graph_replay(sf_handle* h, int32_t on);

/* Feathermap (reference implicit_image/pipeline/feathermap/feathernet.py): structured multi-hashing of a SIREN handle.
 * The P logical weights and biases, in flat order, are the first P entries of V = V1 V2 (V1 [n][m], V2 [m][n], fp32,
 * row-major), each tensor k scaled by its own scalar: W_k = scaler_k * V.view(-1)[seg_k].  The feather vector is
 * [V1 | V2 | scaler of layers.0.weight, layers.0.bias, layers.1.weight, ...], length 2 n m + 2 depth (the reference's
 * named_parameters() order).  After sf_feather_attach
 *   - sf_adam_step (and with it sf_step and graph replay) runs adjoint -> Adam on the feather vector -> materialise, in four
 *     launches; sf_get_grads still returns dL/dW of the last pass;
 *   - sf_set_masks with a mask returns SF_ERR_INVALID (Feathermap is dense), as does attaching to a pixel-split or
 *     FourierNet handle;
 *   - the parameters are W: sf_feather_materialise rewrites them from the feather vector (padded slots stay 0). */
/* logical_out / logical_in [n_layers]: each Linear's logical size (a width the engine zero-pads maps onto strided rows) */
int sf_feather_attach(sf_handle* h, int64_t n, int64_t m, int32_t n_layers, const int32_t* logical_out,
                      const int32_t* logical_in);
/* which: 0 feather params, 1 grads, 2 exp_avg, 3 exp_avg_sq (length 2nm + 2 depth), 4 unscaled V[0, P) of the last
 * materialisation (length P) */
int sf_feather_state_ptr(sf_handle* h, int32_t which, float** dev_ptr, int64_t* len);
/* V = V1 V2 and W = scaler * V into the parameters (call after editing the feather vector; enqueued, no sync) */
int sf_feather_materialise(sf_handle* h);
/* dV1, dV2 and the scalar gradients from the current dL/dW into the feather gradient (sf_adam_step reuses them) */
int sf_feather_adjoint(sf_handle* h);
/* Inference only: the feather vector on a render handle.  sf_feather_render_attach works on a SIREN handle from
 * sf_render_create (a training handle - which takes sf_feather_attach -, a FourierNet or WaveletSiren render handle, a second
 * attach and any bad size return SF_ERR_INVALID).  It validates what sf_feather_attach validates (n_layers, the logical sizes,
 * 1 <= m <= n <= 46340, n^2 >= P), allocates the feather vector (2 n m + 2 depth floats) and nothing else - no gradient,
 * moments, unscaled V, G, partials or chunk tables - and zeroes the parameters, so padded slots stay exactly 0.
 * sf_feather_render_load copies the vector on the handle's stream and materialises W = scaler * (V1 V2) with the inference
 * form of the training handle's kernel (the same fixed-order product, no store of the unscaled V): W, and with it the
 * picture, is bit-identical to a training handle's with the same vector.  No host synchronisation; before attach it returns
 * SF_ERR_STATE.  On an attached handle sf_render / sf_render16 before the first load return SF_ERR_STATE, sf_set_params and
 * sf_params_changed return SF_ERR_INVALID (the parameters belong to the feather vector), and sf_get_params (W),
 * sf_state_ptr(0), sf_set_coords, sf_num_params, sf_param_offset, the profiling calls (the materialisation counts under
 * k_feather_mat) and sf_destroy work as on any render handle. */
int sf_feather_render_attach(sf_handle* h, int64_t n, int64_t m, int32_t n_layers, const int32_t* logical_out,
                             const int32_t* logical_in);
int sf_feather_render_load(sf_handle* h, const float* feather_dev /* [2 n m + 2 depth] fp32, copied */);

/* measurement: per-kernel HIP-event timing on the handle's stream */
int sf_profile_enable(sf_handle* h, int32_t on);
int sf_profile_reset(sf_handle* h);
int sf_profile_num_kernels(const sf_handle* h, int32_t* n);
int sf_profile_get(sf_handle* h, int32_t idx, const char** name, double* total_ms, int64_t* launches,
                   double* flops_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* SIREN_FIT_H_ */
