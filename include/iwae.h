/*
 * iwae.h -- C ABI of libiwae_hip.so, the MI355X (gfx950) IWAE train-step and
 * k-sample NLL hot path.
 *
 * This is the drop-in boundary for the reference's model API
 * (/root/reference/flexible_IWAE.py, "F:" below).  The reference has no native
 * code and no FFI: its "interface" is the Python class Flexible_Model.  Each
 * entry point below replaces the TensorFlow op sequence behind one method of
 * that class; the Python facade iwae_replication_project_amd.Flexible_Model
 * binds them with ctypes (see INTEGRATION.md for the binding a maintainer of
 * the reference would add).
 *
 * Conventions
 *  - Every function returns 0 on success, a negative IWAE_E* code on error;
 *    iwae_last_error(h) then holds a message.  Nothing throws across the ABI.
 *  - Tensors are plain float32.  Pointers marked [dev] are device (HBM)
 *    pointers; [host] are host pointers.  The caller owns all inputs/outputs;
 *    the handle owns weights, Adam state, workspace and RNG state.
 *  - Device work is enqueued on the handle's HIP stream (iwae_set_stream) and
 *    is asynchronous w.r.t. the host, except functions documented as
 *    synchronous (parameter/gradient/state copies to/from host).
 *  - One handle per GPU / rank; a handle is not thread-safe.
 *  - Noise: eps == NULL -> on-device Philox4x32-10 (key = iwae_set_seed,
 *    counter advanced once per forward pass).  Otherwise eps[] holds one
 *    [dev] buffer per stochastic layer in the reference's sample-major layout
 *    [k][B][d_i] (F:59 qh1Ix.sample(n), F:68 .sample()); CIWAE takes 2*L
 *    buffers: draw 1 feeds the VAE term, draw 2 the IWAE term (F:383).
 *  - Internally rows are image-major (row = b*k + s).  Outputs documented as
 *    [B][k] use that layout.
 */
#ifndef IWAE_H
#define IWAE_H

#ifdef __cplusplus
extern "C" {
#endif

#define IWAE_MAX_LAYERS 8

/* error codes */
#define IWAE_OK 0
#define IWAE_EINVAL (-1)   /* bad argument / unknown loss (reference: UnboundLocalError at F:242) */
#define IWAE_EHIP (-2)     /* HIP runtime error */
#define IWAE_ENOMEM (-3)

/* loss ids: Flexible_Model.train_step dispatch F:228-F:241, plus MIWAE/PIWAE
 * (IWAE_replication.pdf p7 s2.4 / Rainforth et al.), absent from the code. */
enum iwae_loss_id {
  IWAE_LOSS_VAE = 0,        /* -get_L        F:229, F:419 */
  IWAE_LOSS_IWAE = 1,       /* -get_L_k      F:231, F:354 */
  IWAE_LOSS_VAE_V1 = 2,     /* -get_L_V1     F:233, F:434 */
  IWAE_LOSS_L_ALPHA = 3,    /* -get_L_alpha  F:235, F:386 */
  IWAE_LOSS_L_POWER_P = 4,  /* -get_L_power_p F:237, F:405 */
  IWAE_LOSS_L_MEDIAN = 5,   /* -get_L_median F:239, F:373 */
  IWAE_LOSS_CIWAE = 6,      /* -get_L_CIWAE  F:241, F:382 */
  IWAE_LOSS_MIWAE = 7,      /* MIWAE(k1,k2), PDF p7 */
  IWAE_LOSS_PIWAE = 8,      /* decoder: IWAE_{k1 k2}, encoder: MIWAE(k1,k2) */
  /* Path-gradient estimators of the IWAE bound.  Loss value and decoder
   * gradient are IWAE's.  The encoder's gradient is that of
   * sum_{b,s} a_enc[s][b] log w[s][b] taken through the sampling path
   * h_i = mu_i + s_i eps_i only (the encoder's parameters inside the densities
   * log q held fixed), with sm = softmax_k(log w) per image: */
  IWAE_LOSS_IWAE_STL = 9,   /* a_enc = sm / B     "sticking the landing", Roeder et al. 2017 (biased for k > 1) */
  IWAE_LOSS_IWAE_DREG = 10  /* a_enc = sm^2 / B   doubly reparameterised, Tucker et al. 2019 (unbiased) */
};

/* Architecture knobs of Flexible_Model.__init__ (F:178-F:180). */
typedef struct iwae_config {
  int n_stochastic;                         /* len(n_hidden_encoder) */
  int x_dim;                                /* 784 (F:57, F:94) */
  int n_hidden_encoder[IWAE_MAX_LAYERS];
  int n_latent_encoder[IWAE_MAX_LAYERS];
  int n_hidden_decoder[IWAE_MAX_LAYERS];
  int n_latent_decoder[IWAE_MAX_LAYERS];
} iwae_config;

/* Loss knobs of Flexible_Model (loss_function, k, p, alpha, beta; F:179-F:217)
 * plus the MIWAE/PIWAE split k = k1*k2 (sample s = j*k1 + i, j < k2). */
typedef struct iwae_loss_config {
  int loss;
  int k;
  float p;
  float alpha;
  float beta;
  int k1;
  int k2;
} iwae_loss_config;

typedef struct iwae_handle iwae_handle;

/* --- lifetime ------------------------------------------------------------ */
/* Replaces Flexible_Model.__init__ (F:178-F:218).  Weights are zero until
 * iwae_set_params (the reference draws Glorot weights lazily inside Keras;
 * the facade draws them on the host and uploads them).  NULL on error. */
iwae_handle* iwae_create(const iwae_config* cfg, int device);
const char* iwae_create_error(void);
void iwae_destroy(iwae_handle* h);
const char* iwae_last_error(const iwae_handle* h);
/* Enqueue on this stream (hipStream_t); NULL = the handle's own stream. */
int iwae_set_stream(iwae_handle* h, void* hip_stream);
/* Waits for the handle's stream, then reports kernel failures as iwae_status. */
int iwae_synchronize(iwae_handle* h);
/* IWAE_EHIP (with iwae_last_error naming the kernel) once a kernel of this
 * handle has reported a failure it could not recover from -- an in-launch
 * wait of the combined image-row backward + update launch (tcu_kernel) that
 * ran out of spins, so that train step's gradients and Adam update were
 * computed from stale data -- else IWAE_OK.  Reads a host-mapped word the
 * kernel writes: no synchronization, so call it after the step's results were
 * read (or after iwae_synchronize).  Sticky until iwae_set_params; the train
 * entry points also return it before enqueueing more work. */
int iwae_status(iwae_handle* h);
int iwae_set_seed(iwae_handle* h, unsigned long long seed);
/* Noise stream of this handle (one per rank): the Philox key becomes
 * splitmix64(seed ^ splitmix64(stream)) for stream != 0 (stream 0: the seed
 * itself), so ranks that share a seed still draw independent noise -- the iid
 * draws of F:59 qh1Ix.sample(n) / F:68 .sample() hold across the ranks of a
 * data-parallel step or a sample-sharded NLL.  Each stream keeps its own
 * Philox counter position: switching away and back continues where the stream
 * stopped (its noise is never replayed), re-selecting the current stream is a
 * no-op, and iwae_set_seed restarts every stream from counter 0. */
int iwae_set_noise_stream(iwae_handle* h, unsigned long long stream);
/* 1 = capture the Philox train step in a hipGraph per shape and replay it. */
int iwae_set_graphs(iwae_handle* h, int enable);
/* Tuning knobs (A/B measurements and tests; none changes the arithmetic
 * beyond summation order / which of two parity-tested kernel paths runs).
 * They replace the environment switches of earlier builds: the release
 * library reads no environment variables.  Setting one drops the handle's
 * captured graphs and engine plans. */
enum iwae_knob {
  IWAE_KNOB_ENGINE = 1,        /* train step on the row-chain engine (default 1) */
  IWAE_KNOB_TC_IMG = 2,        /* ... first encoder layer's l2 / head as image-row jobs above 32 images (1) */
  IWAE_KNOB_TC_IMGBWD = 3,     /* ... its backward as an image-row job at small batches too (1) */
  IWAE_KNOB_TC_FOLD0 = 4,      /* ... its l2 / head folded into the forward jobs (0) */
  IWAE_KNOB_TC_XCD = 5,        /* XCD-aware job placement of the engine launches (1) */
  IWAE_KNOB_TC_BOUND = 6,      /* the bound inside the engine's backward launch (1) */
  IWAE_KNOB_TC_RT = 7,         /* 16-row tiles per engine workgroup below WIDE_ROWS: 1, 2 or 4 (1) */
  IWAE_KNOB_UPD = 8,           /* fused weight-gradient + Adam + FX update launch (1) */
  IWAE_KNOB_UPD_ROWS = 9,      /* ... up to this many sample rows per step (4096) */
  IWAE_KNOB_UPD_SLABS = 11,    /* beyond UPD_ROWS: its split-K gradient pass into the Adam slabs (1) */
  IWAE_KNOB_UPD_SLAB_WG = 12,  /* ... sample-row workgroups of that pass (512) */
  IWAE_KNOB_DW_TARGET = 13,    /* split-K workgroups per layer of the grouped weight-gradient GEMMs (768) */
  IWAE_KNOB_SMALLM_ROWS = 14,  /* few-row first-layer launches up to this many images, <= 32 (32) */
  IWAE_KNOB_OUT_X3_ROWS = 15,  /* row-block path: bf16x3 output layer from this many sample rows (8192) */
  IWAE_KNOB_MG_WAVES = 16,     /* NLL kernel workgroup: 8 waves / 64 rows or 4 waves / 32 rows (8) */
  IWAE_KNOB_NLL_ROWS = 17,     /* sample rows per NLL chunk (2^20) */
  IWAE_KNOB_WIDE_ROWS = 18,    /* engine: 32 / 64-row workgroups from this many sample rows (4097) */
  IWAE_KNOB_DW_WIDE = 19,      /* beyond UPD_ROWS: weight gradients on the 208 x 128-block kernel (1) */
  IWAE_KNOB_LD_ALIGN = 20,     /* workspace row strides: multiples of 4, 8, 16 or 32 floats (4) */
  IWAE_KNOB_NRING = 21,        /* NLL: the weight-ring kernel where its model shapes apply (1) */
  IWAE_KNOB_NRING_TRAIN = 22,  /* train-step forward on the weight-ring kernel (1) ... */
  IWAE_KNOB_NRING_TRAIN_ROWS = 23, /* ... from this many sample rows (4096) */
  IWAE_KNOB_NRING_BWD = 24,        /* ... and the output MLP's backward on the weight ring too: 0 off, 1 on the
                                      step's stream, 2 on a side stream beside the engine's backward launch,
                                      3 the encoder / prior backward on the ring as well (2-layer shape) (3) */
  IWAE_KNOB_WIDE_RT = 25           /* row tiles of 16 per workgroup of the engine's backward launches from
                                      WIDE_ROWS: 1, 2 or 4 (2; the forward launch: 4) */,
  IWAE_KNOB_UPD_WAVES = 26,        /* update kernel workgroup: 16 waves (four per SIMD, each a quarter of a tile's
                                      columns for one k step), 8 or 4 (16; the combined launch of TCU always 8) */
  IWAE_KNOB_NLL_IMGS = 27,         /* images per NLL chunk where the call passes chunk 0 (iwae_nll_eps too);
                                      with NLL_ROWS < imgs * k the chunk's samples split into sample chunks (0: auto) */
  IWAE_KNOB_DW_WG = 28,            /* workgroups the DW_WIDE weight-gradient pass balances its row chunks over (256) */
  IWAE_KNOB_PIWAE_ONE = 29         /* PIWAE on the engine: one unit-weight backward chain for both weightings (1);
                                      0: the chain twice (IWAE_{k1 k2}, then MIWAE for the encoder) */,
  IWAE_KNOB_DW_ALPHA = 30,         /* DW_WIDE pass cost model: a k step's fixed cost in MFMA tiles (150) */
  IWAE_KNOB_IMG_ROWS_FWD = 31,     /* image-row job I (first encoder layer's l2 / head): images per workgroup,
                                      <= 16 (0: auto, ceil(B / 256)) */
  IWAE_KNOB_IMG_ROWS_BWD = 32,     /* image-row job I' (its backward): images per workgroup (0: auto) */
  IWAE_KNOB_X_DIRECT = 33,         /* 1: a large-batch engine step's input GEMM reads the caller's x (default); 0: staged copy */
  IWAE_KNOB_TCU = 34,              /* the first encoder layer's image-row backward (job I') and the fused update in one
                                      launch, its tiles of that layer waiting in-launch for job I' (1) */
  IWAE_KNOB_UPD_APPLY = 35,       /* beyond UPD_ROWS: the gradient pass's slabs summed, Adam and the FX / GX copies
                                      in one update-kernel launch instead of the Adam and FX-refresh launches (1) */
  IWAE_KNOB_TCU_WAIT_TEST = 41,   /* fault injection for tests (0): every in-launch wait of the TCU launch waits
                                      for one producer more than exists, with a short spin bound, so it gives up and
                                      the failure must surface through iwae_status (results of that step invalid) */
  IWAE_KNOB_TCU_WT = 42,          /* the TCU launch's hand-off write-through where every waiting tile is one
                                      reduction iteration (1): job I' stores its outputs sc1 and adds to the counter
                                      without a release fence, the waiting tiles poll and load dZ sc1 without an
                                      acquire; 0: release / acquire fences */
  IWAE_KNOB_NLL_GROUP = 43        /* fused evaluation entries (iwae_nll, iwae_posterior / iwae_impute, iwae_score,
                                      iwae_score_grad): images per pass of the first encoder layer, whole chunks of
                                      them, in [1, 2^20] (16384: three GEMM launches and the copy of x per ~16 K
                                      images instead of per chunk, ~2 % of a k = 5000 NLL) */
  /* 10, 36-40: removed variants measured slower (64 x 32 update tiles, a short
     first graph, the chained / paired first-encoder-layer launches, dw_kernel
     cost-model terms); iwae_set_tuning rejects them with IWAE_EINVAL */
};
int iwae_set_tuning(iwae_handle* h, int knob, long long value);
/* Store policy of what a launch leaves to later launches, a bit mask (default
 * 5).  A launch's end writes back whatever its stores left dirty in the L2s,
 * and the next launch waits for it.  Bit 1: the forward, bit 2: the backward
 * 16-row engine launch store write-through (sc1); bit 4: the fused update's
 * sample-row tiles, bit 8: its one-iteration tiles too; bit 16: a sample-row
 * tile's workgroup, bit 32: the forward's job E / O1 workgroups, which end
 * before the launch does, write their XCD's L2 back as their last act
 * (agent-scope release).  16-row engine plans and the fused / combined update
 * routes only; results do not change by a bit.  Measured at B = 20, k = 50:
 * bits 1 and 4 win, the others lose.  Like a tuning knob (and not
 * one of the enum only because that list is closed): for A/B measurements and
 * tests; setting it drops the handle's captured graphs and engine plans. */
int iwae_set_store_policy(iwae_handle* h, int mask);
/* Matrix-product precision of the tiled GEMM kernels: 1 (default) bf16x3 --
 * a.b = a_hi b_hi + a_hi b_lo + a_lo b_hi with hi = bf16(x), lo = bf16(x - hi),
 * f32 accumulate on v_mfma_f32_16x16x32_bf16 (the engine, ring, update and
 * weight-gradient kernels; the tiled GEMMs also 32x32x16_bf16), ~2^-16
 * relative per product, 5.3x the f32-MFMA rate; 0 exact f32 on
 * v_mfma_f32_16x16x4_f32 (the tiled GEMMs, row-block and few-row kernels; the
 * tiled GEMMs' largest tile also 32x32x2_f32). */
int iwae_set_precision(iwae_handle* h, int mode);
/* Kernel path: 0 auto (train step on the bf16x3 row-chain engine where it
 * applies -- every loss but VAE_V1 / IWAE_STL / IWAE_DREG and L_power_p with
 * p < 0 (whose row weights amplify the bf16x3 rounding), up to 3 stochastic
 * layers, layer widths whose plan fits 160 KB of LDS at 16 rows per workgroup
 * (hidden widths up to about 1200) -- else the f32 fused row-block kernels up
 * to 65536 sample rows, 4 stochastic layers and layer widths of 511, else
 * layer-wise GEMMs), 1 layer-wise only, 2 fused row-block kernels whenever the
 * depth and widths allow, 3 the engine (as auto).  A path that does not apply
 * to the model is never an error: the next one in that order runs. */
int iwae_set_path(iwae_handle* h, int path);

/* --- parameters (synchronous host copies) --------------------------------- */
/* Flat float32 in Keras trainable_weights order: encoder then decoder, per
 * Stochastic_layer l1,l2,lmu,lstd (F:26-F:29), decoder prior layers then the
 * output Sequential (F:86-F:96); per Dense kernel [in][out] then bias [out]. */
long long iwae_num_params(const iwae_handle* h);
int iwae_set_params(iwae_handle* h, const float* host, long long n);
int iwae_get_params(iwae_handle* h, float* host, long long n);
/* Gradient of the LOSS (-bound) from the last iwae_forward_backward, same order. */
int iwae_get_grads(iwae_handle* h, float* host, long long n);

/* --- optimizer: Keras Adam (E:36-E:40), TF ResourceApplyAdam semantics ----- */
int iwae_set_adam(iwae_handle* h, float lr, float beta1, float beta2, float epsilon);
int iwae_get_adam_state(iwae_handle* h, float* m_host, float* v_host, long long n,
                        long long* step);
int iwae_set_adam_state(iwae_handle* h, const float* m_host, const float* v_host,
                        long long n, long long step);

/* --- training (device pointers, stream-ordered) --------------------------- */
/* Flexible_Model.train_step (F:221-F:247): forward, loss, backward, Adam.
 * x [dev] is [B][x_dim], every pixel in [0,1] (here and in every entry that
 * takes images).  log p(x|h) is TFP's Bernoulli log_prob (F:126-F:128): pixels
 * that are exactly 0 or 1 take its one-log form log(x ? p : 1 - p), any other
 * value the two-log form x log p + (1 - x) log(1 - p), the same function.  The
 * kernels decide between the two per group of pixels, not per pixel -- a
 * wave's column tile of 16, 32 or 64 sample rows, or a workgroup's 128 rows --
 * so a binarised image takes either form depending on its neighbours in the
 * batch; results agree to float32 rounding, not bit for bit.  Pixels outside
 * [0,1] and NaN are not supported (a missing pixel goes through the masked
 * entries).  loss_dev [dev, may be NULL] receives the scalar loss (= -bound,
 * the value train_step returns in {loss: ...}). */
int iwae_train_step(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
                    const float* const* eps, int n_eps, float* loss_dev);
/* fit's batch loop (E:82 -> F:221-F:247 per batch): nsteps consecutive train
 * steps with device Philox noise on the batches x + i*B*x_dim, i < nsteps
 * (x [dev] holds nsteps*B images); loss_dev [dev, may be NULL] receives
 * nsteps losses.  Same arithmetic as nsteps iwae_train_step calls; with graphs
 * on, consecutive steps replay from captured graphs of up to 32 steps (no
 * launch gap between them). */
int iwae_train_steps(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, int nsteps,
                     float* loss_dev);
/* Capture, without launching anything, every graph an iwae_train_steps call
 * with these arguments would capture (its chunk lengths: up to 32 steps
 * each), so that the call itself only replays; the parameters, Adam
 * state and noise position are untouched.  Data parallelism with the library
 * communicator included (each captured step carries its all-reduces). */
int iwae_train_steps_prepare(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, int nsteps);
/* The same without the Adam update (gradient kept on device).  For data
 * parallelism: forward_backward -> all-reduce(grad buffer) -> apply_adam. */
int iwae_forward_backward(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
                          const float* const* eps, int n_eps, float* loss_dev);
/* Device gradient buffer (internal padded layout, elementwise-summable).  The
 * caller may bind its own buffer (e.g. a torch tensor used for RCCL). */
int iwae_grad_buffer(iwae_handle* h, float** grad_dev, long long* n);
int iwae_bind_grad_buffer(iwae_handle* h, float* grad_dev, long long n);
/* Gradient signal-to-noise harness (the SNR of
 * Rainforth et al. 2018 discussed at PDF p7): accumulates the current gradient
 * buffer (after iwae_forward_backward) into sum_dev += g, sumsq_dev += g^2.
 * Both are device buffers of iwae_grad_buffer's n floats, internal layout;
 * iwae_export_internal converts such a buffer to the Keras weight order. */
int iwae_grad_moments(iwae_handle* h, float* sum_dev, float* sumsq_dev);
int iwae_export_internal(iwae_handle* h, const float* internal_dev, float* host, long long n);
/* Adam over the gradient buffer times grad_scale.  grad_scale <= 0 (data
 * parallel, after iwae_dp_init): 1 / the buffer's tail element, i.e. the
 * all-reduced sum of the ranks' batch sizes (see iwae_dp_init).  The scaled
 * gradient is written back, so iwae_get_grads returns what Adam used. */
int iwae_apply_adam(iwae_handle* h, float grad_scale);

/* --- data parallelism (SURVEY s8(e), configs[4]) --------------------------- */
/* Make this handle rank `rank` of `world`.  Effects:
 *  - noise stream = rank (iwae_set_noise_stream): per-rank iid Philox noise;
 *  - iwae_forward_backward writes B_local * grad into the gradient buffer and
 *    B_local into its tail element n (the buffer then needs n + 4 floats: the
 *    handle's own one has them; a bound one must too), so one sum all-reduce of
 *    n + 4 floats yields sum_r B_r g_r and B_global = sum_r B_r, and
 *    iwae_apply_adam(h, 0) steps with the exact global batch-mean gradient
 *    (each rank's loss is its local batch mean, F:369) for unequal shards too;
 *  - rccl_unique_id != NULL (128 bytes of ncclGetUniqueId from rank 0, see
 *    iwae_dp_unique_id): the library creates an RCCL communicator over xGMI and
 *    iwae_train_step then runs forward_backward -> ncclAllReduce(sum) on the
 *    handle's stream -> Adam as one step (one hipGraph when graphs are on).
 *    With NULL, the caller reduces the buffer itself between
 *    iwae_forward_backward and iwae_apply_adam(h, 0); iwae_train_step then
 *    returns IWAE_EINVAL.
 * world == 1 with NULL restores single-process behaviour.  A failed call
 * (bad rank / world, a bound gradient buffer, RCCL init) changes nothing. */
int iwae_dp_unique_id(void* out128);
int iwae_dp_init(iwae_handle* h, int rank, int world, const void* rccl_unique_id);
/* Broadcast parameters, Adam moments and the Adam step from rank 0 over the
 * library communicator (needs iwae_dp_init with an RCCL id); synchronous. */
int iwae_dp_broadcast_state(iwae_handle* h);
/* The data-parallel world of the handle: *world = iwae_dp_init's world (1 when
 * never called), *comm_ranks = the rank count of the library's RCCL
 * communicator (ncclCommCount), 0 without one.  bench.py reports both. */
int iwae_dp_world(const iwae_handle* h, int* world, int* comm_ranks);

/* --- evaluation ----------------------------------------------------------- */
/* get_log_weights (F:327-F:351): lw [dev] [B][k] (image-major). */
int iwae_log_weights(iwae_handle* h, const float* x, int B, int k,
                     const float* const* eps, int n_eps, float* lw);
/* The bound (= -loss) of lc on x without a backward pass: get_L, get_L_k,
 * get_L_CIWAE, get_L_power_p, get_L_median, get_L_alpha, get_L_V1 (F:354-F:460).
 * value_dev [dev] receives one float. */
int iwae_bound(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
               const float* const* eps, int n_eps, float* value_dev);
/* E_q(h|x)[log p(x|h)] with Keras BCE (get_E_qhIx_log_pxIh, F:304-F:325). */
int iwae_e_log_px(iwae_handle* h, const float* x, int B, int k,
                  const float* const* eps, int n_eps, float* value_dev);
/* k-sample log p(x) estimate per image (get_NLL = -mean of it, F:463-F:464).
 * Images are processed in chunks of `chunk` images (0 = auto) so that
 * chunk*k rows fit the workspace; out_logpx [dev] is [N]. */
int iwae_nll(iwae_handle* h, const float* x, int N, int k, int chunk, float* out_logpx);
/* Log-sum-exp partials for sample-sharded NLL: over k_local Philox samples per
 * image, out_m[i] = max_s lw, out_s[i] = sum_s exp(lw - out_m[i]) ([dev], [N]).
 * Partials from several ranks merge as M = max m, S = sum s*exp(m-M),
 * log p(x) = M + log S - log(k_total). */
int iwae_nll_partials(iwae_handle* h, const float* x, int N, int k_local, int chunk,
                      float* out_m, float* out_s);
/* Same as iwae_nll with injected noise (parity tests): eps[i] is [k][N][d_i].
 * Where the fused NLL kernel applies (bf16x3 precision, not iwae_set_path(h, 1),
 * at most 4 stochastic layers -- 24 stages -- and layer widths whose plan
 * fits 160 KB of LDS) it runs, chunk by chunk, on the caller's noise.  Where it
 * does not, the call is not an error: all N * k sample rows run as ONE forward
 * pass on the row-block or layer-wise kernels (no chunking: the workspace
 * grows to N * k rows), with the same result. */
int iwae_nll_eps(iwae_handle* h, const float* x, int N, int k, const float* const* eps,
                 int n_eps, float* out_logpx);

/* --- evaluation statistics (get_training_statistics, F:496-F:526) --------- */
/* get_levels_of_units_activity (F:264-F:281): out_means[i] [dev] [N][d_i] =
 * mean over n samples of q(h|x) of h_i (one encoder pass per sample, as the
 * reference's n calls of encoder(x, 1)).  eps (optional) is [n][N][d_i] per
 * layer.  Variances and PCA eigenvalues of these means are host arithmetic. */
int iwae_encoder_means(iwae_handle* h, const float* x, int N, int n, const float* const* eps,
                       int n_eps, float* const* out_means, int n_out);
/* reconstructed_x_probs + get_reconstruction_loss (F:249-F:262, generate_x
 * F:106-F:119): probs [dev] [B][ld_probs] (or NULL), loss_dev [dev] one float
 * = mean_B sum_784 Keras BCE (or NULL).  eps (optional): L encoder buffers
 * [1][B][d_i], then L-1 prior buffers [1][B][d_{L-2-j}] in generation order. */
int iwae_reconstruct(iwae_handle* h, const float* x, int B, const float* const* eps, int n_eps,
                     float* probs, int ld_probs, float* loss_dev);
/* Decoder.generate_x (F:107-F:119) and ancestral sampling from the prior.
 * n rows.  h_top [dev] [n][d_L] or NULL (then h_L ~ N(0, I)).  eps (optional):
 * h_top given: L-1 prior buffers [1][n][d_{L-2-j}] in generation order (as
 * iwae_reconstruct's); h_top NULL: one [1][n][d_L] buffer for h_L first, then
 * those.  u [dev] [n][x_dim] uniforms for the pixel draws, or NULL (Philox).
 * probs / pixels [dev] [n][ld] (ld >= x_dim, multiple of 4, 16-byte aligned),
 * either may be NULL, not both.  h_out (optional): L buffers [n][d_i] in
 * encoder order h_1..h_L.  Weights, Adam state and captured graphs untouched.
 * Each prior layer samples h = eps (exp(zs) + 1e-6) + mu (F:113-F:114); probs =
 * sigmoid(logit) (1 - 1e-6) + 1e-7 (F:101-F:102); pixels = (u < probs) as 0.0 /
 * 1.0.  Columns [x_dim, ld) of the outputs are not written; ld <= 2^22.  One fused launch
 * (gen_kernel: activations in LDS, bf16x3 products) when the model fits 160 KB
 * of LDS; layer-wise launches otherwise and under iwae_set_precision(h, 0) or
 * iwae_set_path(h, 1).  Device noise: Philox layer ids IWAE_MAX_LAYERS + j for
 * prior layer j (iwae_reconstruct's), IWAE_MAX_LAYERS + L - 1 for h_L,
 * 2 * IWAE_MAX_LAYERS for the pixels, row = the generated row; both paths draw
 * the same stream, and every call advances the noise position once.  n == 0
 * succeeds and launches nothing; the handle's sticky error (iwae_status) is
 * returned before any work is enqueued. */
int iwae_generate(iwae_handle* h, int n, const float* h_top, const float* const* eps, int n_eps,
                  const float* u, float* probs, int ld_probs, float* pixels, int ld_pixels,
                  float* const* h_out, int n_out);
/* Dynamic binarisation (the stochastic "MNIST" setting, PDF p7 s3.1): gather
 * the caller's grey-level rows and draw every pixel ~ Bernoulli(grey level),
 * one streaming launch.  Every pointer is a device pointer.  x [n_src][x_dim]
 * grey levels; perm: n int64 row indices into x (what torch.randperm gives), or
 * NULL: the identity, which needs n <= n_src; 0 <= n <= 2^24.  Output row i is
 * drawn from source row perm[i]:
 *   out[i][j] = (u_ij < x[perm[i]][j] || x[perm[i]][j] >= 1) ? 1.0f : 0.0f,
 * so NaN, 0 and negative grey levels give 0.  The x >= 1 clause: the uniform
 * of a Philox word c is ((float)c + 0.5f) * 2^-32, which rounds to exactly 1.0f
 * for c >= 0xFFFFFF80 (about 3e-8 of the draws); with the clause a grey level
 * of 1 always gives 1 and a 0/1 image set comes back bit for bit.  An index
 * outside [0, n_src) gives a row of zeros (a select: nothing outside x is ever
 * read).  out [n][ld_out] follows iwae_generate's rules: x_dim <= ld_out <=
 * 2^22, a multiple of 4, 16-byte aligned, columns [x_dim, ld_out) not written;
 * out == x is legal when perm is NULL and ld_out == x_dim (a thread reads its
 * own column quad before it writes it).  u [n][x_dim]: uniforms in [0, 1)
 * (parity tests), or NULL: Philox on the handle's key (seed and current noise
 * stream), layer id 2 * IWAE_MAX_LAYERS + 3, row = the OUTPUT row i, column
 * quad j / 4 as the counter's group and j % 4 the value within it
 * (iwae_generate's pixel layout).  Every call with n > 0 advances the noise
 * position once (with u given as well); n == 0 succeeds, launches nothing and
 * leaves the position alone.  x is loaded as float4 when x_dim is a multiple
 * of 4 and x is 16-byte aligned, by scalar loads otherwise, with the same
 * result.  Weights, Adam state, captured graphs, engine plans and the workspace
 * are untouched.  The handle's sticky error (iwae_status) is returned before
 * any work is enqueued; IWAE_EINVAL: x or out NULL, n or n_src negative, n >
 * 2^24, n > n_src without perm, a bad ld_out or a misaligned out, or n *
 * ceil(x_dim / 4) >= 2^32 - 255 (the launch's thread count).  After iwae_dp_init
 * the current noise stream is the rank, so ranks binarise their shards
 * independently. */
int iwae_binarize(iwae_handle* h, const float* x, long long n_src, const long long* perm,
                  int n, const float* u, float* out, int ld_out);
/* The importance-weighted posterior q_IW of an IWAE (Cremer, Morningstar &
 * Duvenaud 2017): k samples of q(h|x) reweighted by their self-normalised
 * importance weights.  For image b, lw[b][s] (s < k) are the log weights of
 * iwae_nll / iwae_nll_eps (F:327-F:351), m = max_s lw, e_s = exp(lw_s - m),
 * w~_s = e_s / sum e.  Every pointer is a device pointer; every output is
 * optional, but not all of them NULL:
 *   weights [N][k] (image-major): w~;
 *   logpx [N]: m + log sum e - log k (iwae_nll's value);  ess [N]: (sum e)^2 / sum e^2;
 *   h_mean[i] [N][d_i], encoder order h_1..h_L (n_mean 0 or L): sum_s w~_s h_{i,s};
 *   probs [N][ld_probs]: sum_s w~_s p(x | h_{1,s}), p = sigmoid(logit) (1 - 1e-6) +
 *     1e-7 (F:126) of the ENCODER's h_1 of that sample (the one log w is made
 *     of; iwae_reconstruct re-draws the lower latents from the prior instead).
 *     iwae_generate's rules: x_dim <= ld_probs <= 2^22, a multiple of 4, 16-byte
 *     aligned, columns [x_dim, ld) not written;
 *   h_sir[i] [N][d_i] (n_sir 0 or L): the latents of ONE resampled sample per
 *     image (sampling-importance-resampling), s* = min{ j : sum_{s <= j} w~_s >
 *     u_b } clamped to k - 1, the sum taken in sample order in f32.  u [N]:
 *     uniforms in [0, 1), or NULL: Philox, layer id 2 * IWAE_MAX_LAYERS + 1,
 *     row = the image's index in its chunk.
 * Noise: eps NULL (n_eps 0) is iwae_nll's device stream (same seed, base,
 * chunk-local rows, one advance per chunk); else L buffers [k][N][d_i] as for
 * iwae_nll_eps.  Images run in chunks of `chunk` images (0: IWAE_KNOB_NLL_IMGS,
 * else floor(nll_rows / k), at least 1); a chunk holds ALL k samples of its
 * images; k <= 2^20.  Per chunk: the NLL's forward and log-sum-exp, a small
 * weights kernel, then a second, weighted pass over the same rows -- fused
 * (post_kernel: the rows recomputed in LDS from the same noise, bf16x3) where
 * the fused NLL kernel applies and the second pass's plan fits 160 KB of LDS;
 * else, and under iwae_set_precision(h, 0) or iwae_set_path(h, 1), weighted
 * sums over the rows the layer-wise forward left in memory (there a chunk's
 * probabilities stay within 256 MB).  A path that does not apply is never an
 * error.  Deterministic.  Weights, Adam state, captured graphs and engine
 * plans are untouched; the handle's sticky error (iwae_status) is returned
 * before any work is enqueued. */
int iwae_posterior(iwae_handle* h, const float* x, int N, int k, int chunk,
                   const float* const* eps, int n_eps, const float* u,
                   float* const* h_mean, int n_mean, float* probs, int ld_probs,
                   float* const* h_sir, int n_sir,
                   float* weights, float* ess, float* logpx);
/* Imputation of missing pixels (Mattei & Frellsen 2019, MIWAE): iwae_posterior
 * under the likelihood of the OBSERVED pixels alone.  mask [N][x_dim] (device,
 * required: NULL is IWAE_EINVAL, an all-observed call is iwae_posterior's):
 * non-zero = observed, 0 = missing.  The encoder sees x (.) mask (zero
 * imputation); missing entries of x are selected away, never multiplied, so
 * any value there (NaN, Inf) gives the bits a 0 gives.  The log weights are
 *   lw[b][s] = log p(h) + sum_j [mask_bj != 0] log Bern(x_bj | p_j(h_{1,s}))
 *              - log q(h | x (.) mask),   p = sigmoid(logit) (1 - 1e-6) + 1e-7 (F:126),
 * and weights, ess, logpx (the k-sample estimate of log p(x_obs)), h_mean and
 * h_sir are iwae_posterior's, formed from them; N, k, chunk, eps, n_eps, u,
 * n_mean, n_sir follow its conventions (k <= 2^20, eps [k][N][d_i], u [N]).
 *   x_mean [N][ld_mean]: the single imputation: x_bj where observed (copied bit
 *     for bit), sum_s w~_s p_j(h_{1,s}) where missing;
 *   x_draw [N][ld_draw]: one multiple-imputation draw: x_bj where observed,
 *     (u_pix[b][j] < p_j(h_{1,s*})) as 0.0 / 1.0 where missing, s* the SIR
 *     sample of h_sir (the same u_b, whether or not h_sir is asked for).
 *     u_pix [N][x_dim]: uniforms in [0, 1), or NULL: Philox, layer id
 *     2 * IWAE_MAX_LAYERS + 2, row = the image's index in its chunk, column
 *     quad j / 4 as the counter's group and j % 4 the value within it
 *     (iwae_generate's pixel layout), the base the chunk's first pass drew with.
 * Both follow iwae_generate's ld rules (x_dim <= ld <= 2^22, a multiple of 4,
 * 16-byte aligned; columns [x_dim, ld) not written).  Every output is optional,
 * not all of them NULL.  Repeat the call with another u / u_pix for more draws.
 * Per chunk: the images staged twice by select (mask ? x : 0 for the encoder,
 * mask ? x : -1 for the likelihood), the first pass on the masked
 * instantiation of mega_fwd_kernel where iwae_posterior's fused path applies
 * (the weight-ring kernel is not used, whatever k) or, elsewhere and under
 * iwae_set_precision(h, 0) / iwae_set_path(h, 1), layer-wise with the output
 * Dense's logits stored (at most 256 MB per chunk) and a masked row sum; then
 * iwae_posterior's weights kernel and second pass unchanged, and the fill /
 * draw epilogues (the draw's output MLP runs on the layer-wise GEMMs: N rows).
 * A path that does not apply is never an error.  Deterministic.  Weights, Adam
 * state, captured graphs and engine plans are untouched; the handle's sticky
 * error (iwae_status) is returned before any work is enqueued. */
int iwae_impute(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                const float* const* eps, int n_eps, const float* u, const float* u_pix,
                float* x_mean, int ld_mean, float* x_draw, int ld_draw,
                float* const* h_mean, int n_mean, float* const* h_sir, int n_sir,
                float* weights, float* ess, float* logpx);
/* Training with missing pixels (Mattei & Frellsen 2019, MIWAE proper): the
 * train step, forward + backward and forward-only bound of incomplete images,
 * under iwae_impute's semantics.  Arguments as iwae_train_step /
 * iwae_forward_backward / iwae_bound, with mask [B][x_dim] (device, required:
 * NULL is IWAE_EINVAL) after x: non-zero = observed, 0 = missing.  The encoder
 * sees x (.) mask; missing entries of x are selected away, never multiplied,
 * so any value there (NaN, Inf) gives the bits a 0 gives.  The log weights are
 *   lw[s][b] = log p(h) + sum_j [mask_bj != 0] log Bern(x_bj | p_j(h_{1,s}))
 *              - log q(h | x (.) mask),
 * and every loss id (path-gradient estimators included) is its function of
 * these lw; the Keras-BCE term of L_alpha / VAE_V1 (F:317-F:323) sums the
 * observed pixels only, VAE_V1's analytic KL is unchanged.  The loss is the
 * batch mean over images, not renormalised by the number of observed pixels;
 * an image with every pixel missing is legal (its likelihood term is 0).
 * Per call one staging launch writes the images twice by select (mask ? x : 0
 * for the first encoder layer, its backward and its weight gradient; mask ? x
 * : -1 for the likelihood) -- no launch reads the caller's x -- and the output
 * Dense runs the pixel-masked Bernoulli epilogue of the tiled GEMM, which
 * selects a missing pixel's log-probability, Keras-BCE term and dLoss/dlogit
 * to 0, so the pixel is absent from the bound, every backward chain and the
 * weight gradients.  Paths: the fused row-block kernels or the layer-wise ones
 * by iwae_set_path's rules; the row-chain engine and the weight-ring kernels
 * are never used.  With device noise and iwae_set_graphs(h, 1) a single step
 * is captured and replayed (the staging stays outside the graph, so later
 * calls may pass other x / mask buffers).  After iwae_dp_init with world > 1:
 * IWAE_EINVAL (masked data-parallel steps are not built).  The handle's sticky
 * error (iwae_status) is returned before any work is enqueued. */
int iwae_train_step_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask, int B,
                           const float* const* eps, int n_eps, float* loss_dev);
int iwae_forward_backward_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask,
                                 int B, const float* const* eps, int n_eps, float* loss_dev);
int iwae_bound_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask, int B,
                      const float* const* eps, int n_eps, float* value_dev);
/* Densities of caller-supplied latents: Decoder.get_log_pxIh / get_log_ph /
 * get_log_pxh (F:123-F:145), Decoder.call's probabilities (F:100-F:105) and the
 * encoder's log q (F:60 / F:70) at latents the caller chose -- prior samples,
 * another model's samples, a resampled or perturbed set, the state of an MCMC
 * chain.  Every pointer is a device pointer.  lat[i] is [k][N][d_i], sample-
 * major (the reference's layout of h_i and this ABI's of eps); n_lat must equal
 * L.  Row (b, s) is scored at h_i = lat[i][(s N + b) d_i ..]:
 *   log_q[b][s]  = log N(h_1; enc_0(x_b)) + sum_{i>=1} log N(h_{i+1}; enc_i(h_i))
 *   log_ph[b][s] = log N(h_L; 0, 1) + sum_j log N(h_{L-1-j}; dec_j(h_{L-j}))
 *   log_px[b][s] = sum_pixels log Bern(x_b | p(h_1)),  p = sigmoid(logit) (1 - 1e-6) + 1e-7
 * each [N][k] (image-major, as iwae_log_weights' lw), so log_ph + log_px -
 * log_q is the row's log weight; probs [N k][ld_probs], row b k + s: p(h_1) of
 * that row (iwae_generate's ld rules: x_dim <= ld <= 2^22, a multiple of 4,
 * 16-byte aligned, columns [x_dim, ld) not written).  Every output is optional,
 * not all of them NULL; x may be NULL when neither log_q nor log_px is asked
 * for.  Work an absent output needs is left out of the launch (log_ph alone
 * runs no encoder and no output-MLP stage), and a present output's value does
 * not depend on which others are present, bit for bit.  Each density is
 * evaluated at the caller's float32 latent; the bf16 hi / lo split of a latent
 * feeds the matrix products only.  Images run in chunks of `chunk` images (0:
 * IWAE_KNOB_NLL_IMGS, else floor(nll_rows / k), at least 1); a chunk holds all
 * k rows of its images; k <= 2^20, a chunk at most 2^30 rows; the result does
 * not depend on chunk, bit for bit.  Paths: one score_kernel launch per chunk
 * (mega_fwd_kernel's pipeline and LDS plan with every head a density head,
 * the latents' tiles loaded by its prologue; the weight-ring kernel is not
 * used, whatever k) where iwae_posterior's fused first pass applies; else, and
 * under iwae_set_precision(h, 0) or iwae_set_path(h, 1), layer-wise: one
 * gather launch of the latents into the workspace's rows, then per layer the
 * GEMMs and the density kernel, the output MLP with the Bernoulli epilogue and
 * its row sums; probs: the output Dense's logits stored into the caller's
 * buffer and turned into probabilities in place.  A path that does not apply
 * is never an error.  Rows are independent: non-finite latents in one row give
 * non-finite outputs for that row only.  Nothing is drawn and the noise
 * position stays; weights, Adam state, captured graphs and engine plans are
 * untouched; the handle's sticky error (iwae_status) is returned before any
 * work is enqueued.  IWAE_EINVAL: every output NULL, x NULL with log_q or
 * log_px asked for, n_lat != L, a NULL lat[i], N <= 0 or k <= 0, k or the chunk
 * above the limits, a bad ld_probs or a misaligned probs. */
int iwae_score(iwae_handle* h, const float* x, int N, int k, int chunk,
               const float* const* lat, int n_lat,
               float* log_q, float* log_ph, float* log_px,
               float* probs, int ld_probs);
/* iwae_score for incomplete images: the densities of iwae_impute's and
 * iwae_train_step_masked's model, p(x_obs, h) and q(h | x_obs).  mask is
 * [N][x_dim] on the device, non-zero = observed, 0 = missing; every other
 * argument, limit and output layout is iwae_score's.  The encoder sees x (.)
 * mask, so log_q is log q(h | x (.) mask); log_px[b][s] = sum over the pixels j
 * with mask[b][j] != 0 of log Bern(x_bj | p_j(h_1)); log_ph does not change;
 * probs stay the probabilities of EVERY pixel, observed or not (a caller fills
 * the missing pixels from them).  Missing entries of x are selected away and
 * never multiplied: whatever they hold (NaN, Inf) gives the bits a 0 there
 * gives.  An image with every pixel missing is legal; its log_px is exactly 0.
 * Staging: where iwae_score copies a chunk's (fused: a first-layer group's)
 * images into the workspace, this call runs one impute_stage_kernel launch that
 * writes two copies by select, mask ? x : 0 (the first encoder layer's input)
 * and mask ? x : -1 (the likelihood's pixels: a negative pixel is a missing
 * one); the mask rows advance with the chunk.  Kernels: fused, the masked
 * instantiation of score_kernel (mg_bern's masked form: a missing pixel is the
 * factor 1 of a binarised product and the term 0 of a fractional sum) on
 * iwae_score's plan and LDS layout, wherever iwae_score's fused path applies;
 * layer-wise, iwae_score's launches with the output Dense's masked Bernoulli
 * epilogue (the tiled GEMM's, as iwae_bound_masked) reading the -1 copy.  The
 * weight-ring kernel is never used.  There are no float atomics, the call is
 * deterministic, its result does not depend on chunk, bit for bit, and an
 * all-observed mask gives iwae_score's bits on either path.  State and error
 * rules are iwae_score's, and: IWAE_EINVAL for mask NULL and for x NULL (a call
 * that needs no images has no use for a mask). */
int iwae_score_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                      const float* const* lat, int n_lat,
                      float* log_q, float* log_ph, float* log_px,
                      float* probs, int ld_probs);
/* Gradients of the scored densities with respect to the latents (what HMC, AIS
 * and per-image optimisation of latents move by).  x, N, k, chunk, lat and the
 * value outputs log_q / log_ph / log_px ([N][k], optional) are iwae_score's,
 * with its limits (k <= 2^20, a chunk at most 2^30 rows, a chunk holds all k
 * rows of its images).  coef is a HOST array (c_q, c_ph, c_px); grad is 0 or L
 * device buffers [k][N][d_i], sample-major like lat.  For row (b, s), layer i:
 *   grad[i] = c_q dlog q(h|x)/dh_i + c_ph dlog p(h)/dh_i + c_px dlog p(x|h_1)/dh_i
 * at the caller's float32 latents: (0, 1, 1) the posterior score (HMC), (0, 1,
 * beta) tempered AIS from the prior, (1 - beta, beta, beta) AIS from q, (-1, 1,
 * 1) dlog w/dh, a unit vector one term alone.  Terms, with z = (t - mu) / s,
 * s = exp(zs) + 1e-6 and t a head's target latent: -z / s with respect to the
 * target; dmu = z / s, dzs = (z^2 - 1)(s - 1e-6) / s into the head's outputs,
 * carried back through head -> l2 -> l1 (tanh' = 1 - y^2) to the latent the
 * chain reads.  log q: h_1 gets its target term only (mu_0, s_0 depend on x);
 * chain i >= 1 gives h_{i+1} its target term and h_i the chain's dX.  log p(h):
 * -h_L, and each prior chain's target term and dX.  log p(x|h_1): dlogit_j =
 * (x_j / p_j - (1 - x_j) / (1 - p_j)) (1 - 1e-6) sigma_j (1 - sigma_j) with p =
 * sigma (1 - 1e-6) + 1e-7, back through the output MLP to h_1; zero for i > 1.
 * A term whose coefficient is exactly 0 contributes nothing (not even a NaN)
 * and its chains are left out unless its value output is asked for: then its
 * forward alone runs.  With n_grad 0 the call is a scoring call.  x may be
 * NULL when c_q = c_px = 0 (or n_grad is 0) and neither log_q nor log_px is
 * asked for.  Each grad[i] is written in full, never accumulated into; grad[i]
 * MUST NOT alias any lat[j] (the latents are read while gradients are stored).
 * Paths.  Fused: one sg_kernel launch per chunk wherever iwae_score's fused
 * path applies and the gradient plan fits 160 KiB of LDS at some row tile
 * (64, 32 or 16 rows per workgroup): score_kernel's prologue and density heads;
 * the 2L - 1 chains are independent, so each runs forward and straight back with
 * its y1 / y2 in LDS, the head epilogue turning (mu, zs, target) into the
 * density, the target gradient and dP, and three backward-data stages on the
 * fragment-major transposed weight copies (products bf16x3 on
 * v_mfma_f32_16x16x32_bf16; the heads read the caller's float32 target, the
 * hi / lo copies of a latent feed products only).  The output chain's dlogit
 * enters dY2 = dlogit W3^T as slabs of 256 pixels, each dY2 tile accumulated by
 * one wave in slab order.  Per row, f32 gradient tiles in LDS collect the
 * addends in the fixed order c_q T^q_1 and -c_ph h_L (prologue), then per
 * encoder chain i >= 1 c_q T^q_{i+1} and c_q X^q_i, per prior chain c_ph T^p
 * and c_ph X^p, then c_px X^o (T: target term, X: a chain's dX, the coefficient
 * applied at the head), and are stored to grad.  Layer-wise (under
 * iwae_set_precision(h, 0) or iwae_set_path(h, 1), or when the fused plan does
 * not fit; never an error), one pass per chunk: iwae_score's gather launch and
 * forward GEMMs, per chain the head gradients (sg_dens_kernel) and three
 * backward-data GEMMs (no weight gradient), the output Dense's Bernoulli
 * epilogue with the constant row weight c_px writing c_px dlogit (a chunk's
 * dlogits: at most 256 MB) and three backward-data GEMMs, then one scatter
 * launch that forms c_q T^q_i + c_q X^q_i + c_ph T^p_i + c_ph X^p_i + X^o_i -
 * c_ph h_L left to right (absent addends skipped); its values are iwae_score's
 * layer-wise launches.  On either path there are no float atomics, the call is
 * deterministic, and its result does not depend on chunk, bit for bit.  The
 * value outputs need not be bit-equal to iwae_score's.
 * Rows are independent: non-finite latents in one row give non-finite outputs
 * for that row only.  Nothing is drawn and the noise position stays; weights,
 * Adam state, captured graphs and engine plans are untouched (the backward rows
 * are a workspace of the call's own); the sticky error (iwae_status) is
 * returned before any work is enqueued.  IWAE_EINVAL: nothing asked for, coef
 * NULL or non-finite, n_lat != L, n_grad not 0 or L, a NULL lat[i] or grad[i],
 * x NULL where it is needed, N <= 0 or k <= 0, k or the chunk above the
 * limits. */
int iwae_score_grad(iwae_handle* h, const float* x, int N, int k, int chunk,
                    const float* const* lat, int n_lat,
                    const float coef[3],
                    float* const* grad, int n_grad,
                    float* log_q, float* log_ph, float* log_px);
/* iwae_score_grad for incomplete images: mask ([N][x_dim], device, non-zero =
 * observed) and the semantics are iwae_score_masked's; every other argument,
 * limit and output is iwae_score_grad's.  log q is log q(h | x (.) mask) (its
 * gradient with respect to the latents follows); log p(x|h_1) sums the observed
 * pixels only and the dlogit of a missing pixel is 0, so an image with every
 * pixel missing has log_px exactly 0 and d log p(x|h)/dh exactly 0; log p(h) and
 * its gradient do not change.  Missing entries of x are selected away, never
 * multiplied: NaN or Inf there gives the bits a 0 gives.  Staging is
 * iwae_score_masked's (one impute_stage_kernel launch per chunk or first-layer
 * group: mask ? x : 0 for the encoder, mask ? x : -1 for the likelihood).
 * Kernels: fused, the masked instantiation of sg_kernel on iwae_score_grad's
 * plan and LDS layout -- in the output stage a pixel whose staged value is
 * negative adds 0 to the row's log p(x|h) and stores a 0 dlogit, by a select on
 * values computed for every pixel; the 256-pixel slabs, the one-wave-per-dY2-
 * tile accumulation and the addend order are iwae_score_grad's; layer-wise,
 * iwae_score_grad's launches with the masked Bernoulli epilogue writing c_px
 * dlogit (a chunk's dlogits: at most 256 MB).  The weight-ring kernel is never
 * used.  There are no float atomics, the call is deterministic, its result
 * does not depend on chunk, bit for bit, and an all-observed mask gives
 * iwae_score_grad's bits on either path.  State and error rules are
 * iwae_score_grad's, and: IWAE_EINVAL for mask NULL and for x NULL. */
int iwae_score_grad_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                           const float* const* lat, int n_lat,
                           const float coef[3],
                           float* const* grad, int n_grad,
                           float* log_q, float* log_ph, float* log_px);
/* Annealed importance sampling on the latents (Neal 2001; Wu et al. 2017): a
 * whole annealing schedule of Metropolis-adjusted HMC transitions, enqueued on
 * the handle's stream with no host synchronization (only a workspace that has
 * to grow waits).  Every chain is one (image b, sample s) row; all layers move
 * jointly, the mass matrix is the identity.  lat (required, L device buffers
 * [k][N][d_i], sample-major) is the chains' state, updated IN PLACE; x
 * (required), N, k and chunk are iwae_score's, with its limits, and N k <=
 * 2^30 chains.  betas is a HOST array of n_temps + 1 finite values in [0, 1],
 * in any order: ascending from 0 to 1 is AIS, descending from 1 the reverse
 * chain (bidirectional Monte Carlo), constant 1 plain HMC on p(h|x).  The
 * transition at beta moves under c_q log q(h|x) + c_ph log p(h) + c_px log
 * p(x|h_1), iwae_score_grad's coefficient forms: init 0 (from the prior) (0,
 * 1, beta) with Delta = log p(x|h_1); init 1 (from q) (1 - beta, beta, beta)
 * with Delta = log p(h) + log p(x|h_1) - log q(h|x).  Transition t = 1 ..
 * n_temps, beta = betas[t], per chain with its own step eps:
 *   1. one iwae_score_grad pass at the state: g, the values, U_old = -(c_q
 *      log q + c_ph log p(h) + c_px log p(x|h)) (a term whose coefficient is 0
 *      is left out) and Delta;
 *   2. log_w += (betas[t] - betas[t-1]) Delta;
 *   3. momenta r ~ N(0, I); H_old = U_old + |r|^2 / 2; r += eps/2 g; the
 *      proposal q = state + eps r;
 *   4. n_leapfrog passes at q; after each but the last r += eps g, q += eps r
 *      (two half kicks merged); after the last r += eps/2 g, H_new = U(q) +
 *      |r|^2 / 2; accept iff log u < H_old - H_new (a NaN rejects);
 *   5. on accept state <- q and the chain's accept count goes up by one; a
 *      rejected chain keeps its bits;
 *   6. eps <- clamp(eps (accept ? adapt_inc : adapt_dec), step_min, step_max)
 *      in float32 (adapt_inc = adapt_dec = 1: a fixed step).
 * That is n_leapfrog + 1 gradient passes per transition, each on the path
 * iwae_score_grad would take (fused or layer-wise, never an error), and
 * between them one launch of iwae_ais.hip: ais_begin_kernel (steps 2, 3),
 * ais_step_kernel (the merged kick and drift, float4 where d_i is a multiple
 * of 4), ais_end_kernel (the last kick, the decision, steps 5 and 6); begin
 * and end give a chain 16 lanes while every d_i <= 64 and a wave otherwise,
 * and sum |r|^2 per lane in layer, then column order and over the group by a
 * fixed butterfly.  After the last transition ais_finish_kernel forms, per
 * image in a fixed order, logpx = logsumexp_s log_w - log k and ess = (sum
 * e)^2 / sum e^2 with e = exp(log_w - max).  Per-chain arrays are image-major
 * [N][k]: step_io (NULL: every chain starts at cfg->step; else read and
 * written), log_w, accepts (accepted transitions, as float); logpx, ess [N];
 * each of the four outputs is optional.  accumulate = 0: log_w and accepts
 * start at 0; 1: they are added to the caller's values (with log_w NULL the
 * weights behind logpx / ess start at 0 either way), and a call on the
 * lat, step_io, log_w and accepts a previous call left, over the rest of the
 * schedule (its first beta the previous call's last), continues that chain:
 * two such calls give bit for bit what one call over the whole schedule
 * gives, with injected and with device noise.  Noise: mom is NULL / 0, or
 * n_temps * L device buffers [k][N][d_i], mom[(t - 1) L + i] transition t's
 * momenta of layer i; u is NULL, or [n_temps][N][k] uniforms in (0, 1).
 * Absent, momenta of layer i are philox_normal4 under layer id 2
 * IWAE_MAX_LAYERS + 4 + i (column quad j / 4, value j % 4) and the accept
 * uniform is value 0 of quad 0 of philox_uniform4 under layer id 2
 * IWAE_MAX_LAYERS + 12, both at row b k + s over the whole call and base =
 * the handle's noise position + t - 1 on the current key.  The noise position
 * advances once per transition, by n_temps per call, whether or not noise was
 * injected.  There are no float atomics, every element is written by one
 * thread, the call is deterministic and its result does not depend on chunk,
 * bit for bit.  Rows are independent: a chain whose latents are not finite
 * never accepts, stays put, and its neighbours are unaffected.  Weights, Adam
 * state, the train arena, captured graphs and engine plans are untouched (the
 * chains' momenta, proposals, gradients and values are a workspace of the
 * call's own, which only grows); the sticky error (iwae_status) is returned
 * before any work is enqueued.  IWAE_EINVAL, with nothing launched: cfg,
 * betas, lat or x NULL, a NULL lat[i], n_lat != L, n_mom not 0 or n_temps * L
 * or a NULL buffer among them, init not 0 or 1, n_temps < 1 or above 2^24,
 * n_leapfrog < 1, a beta that is not finite or outside [0, 1], step not
 * finite or <= 0, adapt_inc or adapt_dec not finite or <= 0, step_min >
 * step_max, N <= 0 or k <= 0, k, the chunk or N k above the limits. */
typedef struct iwae_ais_config {
  int init;         /* 0: from the prior, 1: from q(h|x) */
  int n_temps;      /* T >= 1; betas holds T + 1 host floats; T <= 2^24 */
  int n_leapfrog;   /* >= 1 */
  int accumulate;   /* 0: log_w and accepts start at 0; 1: added to the caller's values */
  float step;       /* every chain's initial step where step_io is NULL; > 0 */
  float adapt_inc, adapt_dec, step_min, step_max;   /* 1, 1: fixed step */
} iwae_ais_config;
int iwae_ais(iwae_handle* h, const float* x, int N, int k, int chunk,
             float* const* lat, int n_lat,
             const iwae_ais_config* cfg, const float* betas,
             const float* const* mom, int n_mom,
             const float* u,
             float* step_io,
             float* log_w, float* accepts,
             float* logpx, float* ess);
/* iwae_ais on incomplete images: annealing towards p(h | x_obs), so logpx
 * estimates log p(x_obs).  mask ([N][x_dim], device, non-zero = observed) and
 * the semantics are iwae_score_masked's: log q is log q(h | x (.) mask), log
 * p(x|h_1) sums the observed pixels, a missing pixel's dlogit is 0, log p(h)
 * does not change, missing entries of x are selected away (NaN or Inf there
 * gives the bits a 0 gives), an all-missing image is legal.  Every other
 * argument, limit, output, noise rule and the transition itself are iwae_ais's;
 * each of the n_leapfrog + 1 gradient passes of a transition is an
 * iwae_score_grad_masked pass with the same mask (its two staged copies, mask
 * ? x : 0 for the encoder and mask ? x : -1 for the likelihood, then the masked
 * sg_kernel or the masked layer-wise launches), between them iwae_ais's own
 * begin / step / end launches.  The weight-ring kernel is never used.
 * There are no float atomics, the call is deterministic, its result does not
 * depend on chunk, bit for bit, and an all-observed mask gives iwae_ais's bits.
 * Continuation: with accumulate = 1 a call on the lat, step_io, log_w and
 * accepts a previous call left, with the same x and mask and over the rest of
 * the schedule, gives bit for bit what one call over the whole schedule gives,
 * with injected and with device noise.  State, noise-position and error rules
 * (nothing launched on an error) are iwae_ais's, and: IWAE_EINVAL for mask
 * NULL (x NULL is iwae_ais's own error). */
int iwae_ais_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                    float* const* lat, int n_lat,
                    const iwae_ais_config* cfg, const float* betas,
                    const float* const* mom, int n_mom,
                    const float* u,
                    float* step_io,
                    float* log_w, float* accepts,
                    float* logpx, float* ess);
/* Per-image variational refinement ("local" optimisation of q; Cremer, Li &
 * Duvenaud 2018): Adam ascent on the parameters of one diagonal Gaussian per
 * image over all latent layers jointly, q*(h) = prod_i N(h_i; m_i,
 * diag(exp(ls_i))^2), enqueued on the handle's stream with no host
 * synchronization (only a workspace that has to grow waits).  mean[i],
 * logstd[i] (required, n_par = L device buffers [N][d_i], encoder order h_1 ..
 * h_L) are updated IN PLACE; x (required), N, k and chunk are iwae_score's,
 * with its limits, and N k <= 2^30 rows.  With k samples per image, row (b,
 * s): h_i = fmaf(exp(ls_i), eps_i, m_i) in float32 (the value the gradient
 * pass sees), log q* = sum_ij (-eps^2 / 2 - ls_ij) - D / 2 log 2 pi with D =
 * sum d_i, log w = log p(h) + log p(x|h_1) - log q*.  objective 0 (ELBO): the
 * value is mean_s log w_s and a_s = 1 / k; objective 1 (IWAE_k): logsumexp_s
 * log w_s - log k and a_s = softmax_s(log w).  With g = d(log p(h) + log
 * p(x|h_1)) / dh (iwae_score_grad under (0, 1, 1)) the total reparameterised
 * gradients are G^m_ij = sum_s a_s g_sij and G^ls_ij = (sum_s a_s g_sij
 * eps_sij) exp(ls_ij) + 1, both summed in one fixed order.  Update n = step0
 * + 1 .. step0 + n_iters, per parameter p with gradient G, in the train
 * step's Adam form: m1 += (1 - beta1) (G - m1); m2 += (1 - beta2) (G^2 - m2);
 * p += lr_n m1 / (sqrt(m2) + epsilon), lr_n = lr sqrt(1 - beta2^n) / (1 -
 * beta1^n) formed on the host in double; then ls is clamped to [logstd_min,
 * logstd_max].  After the n_iters updates one optional evaluation pass draws
 * fresh samples at the final parameters and scores them (no gradient); it
 * runs when any of lat_out / log_w / logpx / ess is asked for, and n_iters =
 * 0 only evaluates the q* the caller supplies.  P = n_iters + (1 with an
 * evaluation pass) passes draw noise: eps is NULL / 0, or P L device buffers
 * [k][N][d_i], eps[p L + i] pass p's noise of layer i; absent, the noise of
 * layer i is philox_normal4 under layer id 2 IWAE_MAX_LAYERS + 13 + i (column
 * quad j / 4, value j % 4) at row b k + s over the whole call and base = the
 * handle's noise position + p on the current key.  The noise position
 * advances by P per call, whether or not noise was injected.  adam is NULL /
 * 0 (the moments live in the call's workspace), or 4 L device buffers [N][d_i]:
 * adam[4 i], adam[4 i + 1] the first and second moment of mean_i, adam[4 i +
 * 2], adam[4 i + 3] those of logstd_i.  With step0 = 0 the moments start at
 * zero and the buffers' contents are ignored; with step0 > 0 they are read,
 * and a second call on the mean, logstd and adam a first call left, with
 * step0 = the first call's n_iters, continues that run: its noise is the next
 * passes of the same device stream (or the next injected buffers) and its
 * result is bit for bit what one call over all iterations gives, provided
 * the first call ran no evaluation pass.  Outputs, all optional: bound
 * [n_iters][N], the objective's value at the parameters before update t on
 * iteration t's samples; lat_out[i] [k][N][d_i] (n_lat 0 or L), the
 * evaluation pass's samples; log_w [N][k], image-major; logpx = logsumexp_s
 * log_w - log k and ess = (sum e)^2 / sum e^2 with e = exp(log_w - max), [N].
 * Per call n_iters gradient passes and, with an evaluation, one scoring pass,
 * each on the path iwae_score_grad would take (fused or layer-wise, never an
 * error), and between them n_iters + 1 launches of iwae_refine.hip:
 * refine_begin_kernel (pass 0's samples), refine_step_kernel (an iteration's
 * weights, gradients, Adam update and the next pass's samples in one launch),
 * refine_end_kernel (the last update and the evaluation's samples);
 * refine_finish_kernel forms the evaluation's outputs and moves the noise
 * position.  One workgroup owns an image; there are no float atomics, every
 * element is written by one thread, the call is deterministic and its result
 * does not depend on chunk, bit for bit.  Rows are independent: an image whose
 * parameters are not finite has non-finite outputs and its neighbours are
 * unaffected.  Weights, the model's Adam state, the train arena, captured
 * graphs and engine plans are untouched (the samples, their noise, gradients
 * and values are a workspace of the call's own, which only grows); the sticky
 * error (iwae_status) is returned before any work is enqueued.  IWAE_EINVAL,
 * with nothing launched: cfg, x, mean or logstd NULL or a NULL buffer among
 * them, n_par != L, n_eps not 0 or P L, n_adam not 0 or 4 L, n_lat not 0 or L,
 * a NULL buffer among eps / adam / lat_out, objective not 0 or 1, n_iters < 0
 * or above 2^24, step0 < 0 or above 2^30, step0 > 0 without adam, n_iters = 0
 * with no evaluation output, lr or epsilon not finite or <= 0, beta1 or beta2
 * outside [0, 1), logstd_min > logstd_max or either not finite, N <= 0 or k <=
 * 0, k, the chunk or N k above the limits. */
typedef struct iwae_refine_config {
  int objective;     /* 0 ELBO, 1 IWAE_k */
  int n_iters;       /* >= 0, <= 2^24 */
  int step0;         /* Adam steps already taken (continuation); >= 0 */
  float lr, beta1, beta2, epsilon;
  float logstd_min, logstd_max;
} iwae_refine_config;                       /* 36 bytes */
int iwae_refine(iwae_handle* h, const float* x, int N, int k, int chunk,
                float* const* mean, float* const* logstd, int n_par,
                const iwae_refine_config* cfg,
                const float* const* eps, int n_eps,
                float* const* adam, int n_adam,
                float* bound, float* const* lat_out, int n_lat,
                float* log_w, float* logpx, float* ess);
/* iwae_refine on incomplete images: q*(h) is fitted to p(h | x_obs), and the
 * evaluation's logpx is a bound on log p(x_obs).  mask ([N][x_dim], device,
 * non-zero = observed) and the semantics are iwae_score_masked's: log p(x|h_1)
 * sums the observed pixels, a missing pixel's dlogit is 0, log p(h) does not
 * change, missing entries of x are selected away (NaN or Inf there gives the
 * bits a 0 gives), an all-missing image is legal (its q* moves under the prior
 * alone).  Every other argument, limit, output, noise rule and the update are
 * iwae_refine's; each gradient pass and the evaluation's scoring pass is an
 * iwae_score_grad_masked pass under (0, 1, 1) with the same mask (its two
 * staged copies, mask ? x : 0 for the encoder and mask ? x : -1 for the
 * likelihood, then the masked sg_kernel or the masked layer-wise launches),
 * between them iwae_refine's own launches.  The weight-ring kernel is never
 * used.  There are no float atomics, the call is deterministic, its result
 * does not depend on chunk, bit for bit, and an all-observed mask gives
 * iwae_refine's bits.  Continuation: a second call on the mean, logstd and
 * adam a first call left, with the same x and mask and step0 = the first
 * call's n_iters, gives bit for bit what one call over all iterations gives,
 * provided the first call ran no evaluation pass.  State, noise-position and
 * error rules (nothing launched on an error) are iwae_refine's, and:
 * IWAE_EINVAL for mask NULL (x NULL is iwae_refine's own error). */
int iwae_refine_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                       float* const* mean, float* const* logstd, int n_par,
                       const iwae_refine_config* cfg,
                       const float* const* eps, int n_eps,
                       float* const* adam, int n_adam,
                       float* bound, float* const* lat_out, int n_lat,
                       float* log_w, float* logpx, float* ess);
/* Encoder.call (F:56-F:75): k samples of q(h|x) per image, with device noise
 * (eps NULL, n_eps 0) or injected eps[i] [k][N][d_i].  lat_out[i] [k][N][d_i],
 * sample-major (n_lat 0 or L); log_q [N][k]; loc_top / scale_top: the
 * parameters of distributions[-1] (F:75), [N][d_1] when L = 1 and [k][N][d_L]
 * otherwise, scale = exp(zs) + 1e-6.  Every output is optional, not all of
 * them NULL.  Chunks as iwae_score's.  The rows have to reach memory, so the
 * call runs on the layer-wise kernels whatever the path: per encoder layer the
 * three GEMMs and the sampling kernel, then one relayout launch ([rows][ld] ->
 * [k][N][d]); no decoder work.  With device noise the noise position advances
 * once per chunk, as a forward pass's does, and Philox is addressed as the
 * layer-wise forward does (row in chunk, layer id i, column quad): a layer-wise
 * iwae_log_weights call of the same seed, N and k (one chunk) weighs exactly
 * these samples.  State and error rules are iwae_score's otherwise (x is
 * required). */
int iwae_encode(iwae_handle* h, const float* x, int N, int k, int chunk,
                const float* const* eps, int n_eps,
                float* const* lat_out, int n_lat, float* log_q,
                float* loc_top, float* scale_top);
/* The aggregate posterior q(h_1) = 1/M sum_m q(h_1 | x_m) (Hoffman & Johnson
 * 2016) at R query latents lat1 [R][d_1] [dev].  Only the first stochastic
 * layer is pairwise: q(h_1..h_L) = q(h_1) prod_i q(h_{i+1} | h_i), so this one
 * entry serves every depth; the other terms are iwae_encode's and iwae_score's.
 * Reference components (mu_m, s_m), m < M:
 *  - x_ref [M][x_dim] [dev] given: the first encoder layer's parameters of
 *    image m, s = exp(zs) + 1e-6, from the layer-0 launches the layer-wise
 *    encoder makes on image rows (l1, l2, head); nothing is sampled, no later
 *    layer and no decoder work runs.  The walk is the evaluation entries' chunk
 *    walker with k = 1 and chunk images per pass (0: automatic).  loc / scale
 *    [M][d_1] [dev], if non-NULL, receive the parameters; for L = 1 they are the
 *    bits iwae_encode returns as loc_top / scale_top for the same x, path and
 *    precision.
 *  - x_ref NULL: loc and scale are required inputs (the aggregate of any
 *    diagonal-Gaussian family, e.g. iwae_refine's q* with scale =
 *    exp(logstd)); chunk is ignored.  A scale <= 0 or not finite gives
 *    non-finite results for the rows it touches; it is not checked on the host.
 * Float32, in difference form (never h^2 a - 2 h b + c, which cancels at the
 * small scales of a trained encoder):
 *   t(r,m,j) = -1/2 z^2 - log s_mj - 1/2 log 2 pi,  z = (h_rj - mu_mj) (1 / s_mj)
 *   J(r,m)   = sum_j t(r,m,j), in column order
 *   log_q_agg[r]    = logsumexp_m J(r,m) - log M            [R]
 *   log_q_dim[r][j] = logsumexp_m t(r,m,j) - log M          [R][d_1]
 * and with own_period = P > 0 row r's own image is o = r mod P (sample-major
 * [k][N][d_1] latents with x_ref = x: P = N):
 *   log_q_own[r] = J(r,o) [R],  log_q_own_dim[r][j] = t(r,o,j) [R][d_1];
 * P = 0: the two own outputs must be NULL.  Every output is optional, not all
 * of them NULL.  1 / s and log s are formed once per call by a prep launch
 * into [M][d_1] workspace.  Launches: agg_joint_kernel for log_q_agg,
 * agg_dim_kernel (the expensive one: one exp per (r, m, j)) only for
 * log_q_dim, one own-term launch.  When the query rows are too few to fill the
 * device the references are split into segments: with W the workgroups one
 * pass over all references takes (ceil(R / 64) joint; ceil(ceil(R / 4)
 * min(d_1, 256) / 256) ceil(d_1 / 256) per unit) and T the references per tile
 * (64 joint; min(128, 4096 / min(d_1, 256)) per unit), W >= 1024 gives one
 * segment, else ceil(1024 / W) segments, at most 1024 and at most one per
 * tile, of equal length rounded up to whole tiles; each writes (max, sum)
 * partials and a merge launch combines them in segment order, M* = max m, S =
 * sum s exp(m - M*) (iwae_nll_partials' rule).  The partial workspace is
 * bounded by the rule itself, so R needs no slicing: a split call has W < 1024
 * workgroups of at most 64 rows (joint) or 1024 (row, unit) pairs (per unit)
 * and fewer than 1024 / W + 1 segments, so its partials (2 segments floats per
 * row joint, 2 segments d_1 per row per unit) stay below 2^18 floats (1 MiB)
 * and 2^22 floats (16 MiB); an unsplit call writes none.  The split is a
 * function of (R, M, d_1) alone, so two calls with different R need not agree
 * to the last bit; one call is deterministic run to run and its result does
 * not depend on chunk, bit for bit.  No float atomics, every output element
 * has one writer, every reduction a fixed order.  Rows are independent: a
 * non-finite latent poisons its own row only.  A float4 path serves d_1 % 4 ==
 * 0 with 16-byte aligned lat1 and loc, a scalar path with the same bits
 * everything else, down to d_1 = 1.
 * Everything is enqueued on the handle's stream with no host synchronisation
 * unless a workspace has to grow.  Nothing is drawn and the noise position
 * stays; weights, Adam state, captured graphs and engine plans are untouched
 * (as for iwae_encode, an x_ref call whose chunk outgrows the handle's
 * activation workspace regrows it, and the next train step re-captures; its
 * result is the same).
 * IWAE_EINVAL, nothing launched (after the sticky iwae_status error, returned
 * first): every output NULL; lat1 NULL; R < 1 or R > 2^30; M < 1 or M > 2^24;
 * x_ref NULL with loc or scale NULL; P < 0 or P > M; P = 0 with an own output
 * asked for.
 * Out of scope: pixel masks (an x_ref with a mask), sharding M over GPUs, and
 * minibatch-weighted / stratified estimators for an x_ref that subsamples a
 * larger data set. */
int iwae_aggregate(iwae_handle* h,
                   const float* x_ref, int M, int chunk,
                   float* loc, float* scale,
                   const float* lat1, long long R,
                   int own_period,
                   float* log_q_agg,
                   float* log_q_dim,
                   float* log_q_own,
                   float* log_q_own_dim);
/* get_NLL_without_inactive_units (F:466-F:494): like iwae_nll / iwae_nll_eps
 * with every sampled h_i multiplied by masks[i] ([dev], d_i floats of 0/1). */
int iwae_nll_masked(iwae_handle* h, const float* x, int N, int k, const float* const* eps,
                    int n_eps, const float* const* masks, int n_masks, float* out_logpx);

/* --- reweighted wake-sleep ------------------------------------------------- */
/* Reweighted wake-sleep (Bornschein & Bengio 2015; Le et al. 2019): k samples
 * per image, n_dream dream pairs, and the two encoder coefficients.  (1, 0) is
 * wake-wake, (0, 1) wake-sleep, (0.5, 0.5) Bornschein & Bengio's mix. */
typedef struct iwae_ws_config { int k; int n_dream; float c_wake, c_sleep; } iwae_ws_config;
/* One reweighted wake-sleep step on x [B][x_dim] [dev].  Wake forward:
 * iwae_log_weights' pass with k samples (device noise: eps NULL, n_eps 0; or
 * injected eps[i] [k][B][d_i], n_eps = L, as iwae_train_step takes them),
 * giving h_i, lw and sm = softmax_s(lw) per image.  Three values, float32:
 *   L_theta = -(1/B) sum_b (logsumexp_s lw_bs - log k), the IWAE loss: the
 *             bits of an IWAE_LOSS_IWAE iwae_train_step / iwae_forward_backward
 *             on the same noise and path, and of -iwae_bound wherever a train
 *             step's forward and a bound's use the same products (every GEMM
 *             under iwae_set_precision(h, 0));
 *   L_wake  = -(1/B) sum_b sum_s sm_bs log q(h_bs | x_b), sm and h constants;
 *   L_sleep = -(1/n) sum_j log q(h^j | x^j) over the n = n_dream dream pairs.
 * Gradient buffer: the decoder's parameters get grad L_theta (exactly an
 * IWAE_LOSS_IWAE step's), the encoder's c_wake grad L_wake + c_sleep grad
 * L_sleep: per head -a z/s on mu and -a (z^2 - 1)(s - 1e-6)/s on zs, row
 * weight a = c_wake sm_bs / B (wake rows) or c_sleep / n (dream rows), through
 * head -> l2 -> l1 into that layer's weight gradients only: the latent a
 * layer reads is data, there is no dL/dh into another layer.  A coefficient
 * of exactly 0 leaves its phase out of every launch (not even a NaN of it
 * reaches the encoder's gradient) and its value is reported as 0.
 * Dreams: dream_x [n][x_dim] [dev] (the encoder's input) with dream_lat[i]
 * [n][d_i] [dev], encoder order h_1 .. h_L, n_dream_lat = L; or both NULL
 * (n_dream_lat 0) with n_dream > 0: the step dreams its own from the current
 * weights by one internal iwae_generate(n, h_top NULL, device noise, pixels
 * and h_out), bit for bit that call's result at that noise position, on the
 * generation path that call takes.  With c_sleep == 0 dream buffers are never
 * read.  The noise position advances once for the wake forward and once more
 * iff the step dreamt its own.
 * values_dev [dev], 3 floats (L_theta, L_wake, L_sleep), may be NULL.
 * iwae_wake_sleep_step then applies the handle's Adam to the whole buffer (the
 * Adam launch an f32 row-block or layer-wise train step ends in);
 * iwae_wake_sleep_grad leaves the gradient in the buffer (iwae_get_grads,
 * iwae_apply_adam) and the Adam state untouched.
 * Paths: chosen as IWAE_LOSS_IWAE_STL's are, over B k + n_dream rows: the f32
 * row-block kernels (rb_bwd_kernel's GM_FIT jobs; the dream rows' encoder
 * forward on rb_fwd_kernel with the target-given density epilogue), else the
 * layer-wise GEMMs (gauss_bwd_enc_kernel's GM_FIT launches), never an error;
 * never the bf16x3 engine, the fused update or the weight ring.
 * iwae_set_graphs does not apply: every launch is enqueued on the handle's
 * stream, with no host synchronisation unless a workspace grows (before
 * anything is enqueued).  No float atomics; deterministic.  The dream rows
 * lie behind the wake rows in the train step's workspace, which grows to
 * B + n_dream image rows and B k + n_dream sample rows; captured train-step
 * graphs and engine plans survive a call that does not grow it.
 * IWAE_EINVAL, nothing launched and the noise position untouched (after the
 * sticky iwae_status error, returned first): cfg or x NULL; k < 1 or B < 1; a
 * coefficient negative or not finite; both 0; c_sleep > 0 with n_dream < 1;
 * c_sleep == 0 with n_dream != 0; only one of dream_x and dream_lat; n_dream_lat
 * not L with dream_lat and not 0 without; a NULL dream_lat[i]; a wrong n_eps
 * or a NULL eps[i]; B k + n_dream above 2^30; a data-parallel world > 1. */
int iwae_wake_sleep_step(iwae_handle* h, const iwae_ws_config* cfg, const float* x, int B,
                         const float* const* eps, int n_eps,
                         const float* dream_x, const float* const* dream_lat, int n_dream_lat,
                         float* values_dev);
int iwae_wake_sleep_grad(iwae_handle* h, const iwae_ws_config* cfg, const float* x, int B,
                         const float* const* eps, int n_eps,
                         const float* dream_x, const float* const* dream_lat, int n_dream_lat,
                         float* values_dev);

/* --- thermodynamic variational objective ----------------------------------- */
/* Thermodynamic variational objective (TVO; Masrani, Le & Wood 2019): k samples
 * per image and a partition of n_part temperature intervals. */
typedef struct iwae_tvo_config { int k; int n_part; } iwae_tvo_config;
/* One TVO step on x [B][x_dim] [dev].  betas [host], n_part + 1 floats: the
 * partition 0 = betas[0] < betas[1] < ... < betas[n_part] = 1, 1 <= n_part <=
 * 64; it travels in the launch's arguments (no device copy).  Wake forward:
 * iwae_log_weights' pass with k samples (device noise: eps NULL, n_eps 0; or
 * injected eps[i] [k][B][d_i], n_eps = L, as iwae_train_step takes them),
 * giving h_i and lw_s = log p(h) + log p(x | h_1) - log q(h | x) per image.
 * With D_j = betas[j+1] - betas[j], wn^(j) = softmax_s(betas[j] lw_s) (taken
 * after subtracting betas[j] max_s lw) and m_j = sum_s wn^(j)_s lw_s,
 * j = 0 .. n_part, per image:
 *   lower = sum_{j<n_part} D_j m_j        (left Riemann sum: the TVO),
 *   upper = sum_{j<n_part} D_j m_{j+1}    (right Riemann sum),
 *   iwae  = logsumexp_s lw_s - log k,     lower <= iwae <= upper,
 *   a_theta_s = sum_{j<n_part} D_j wn^(j)_s [1 + betas[j] (lw_s - m_j)]
 *             = d lower / d lw_s,                          sum_s a_theta_s = 1,
 *   a_phi_s   = sum_{j<n_part} D_j wn^(j)_s [(1 - betas[j]) (lw_s - m_j) - 1],
 *                                                          sum_s a_phi_s = -1
 * (a_phi: the covariance estimator of the paper's eq. 9-10 at fixed samples;
 * it needs no reparameterisation and can be negative).  n_part = 1 makes lower
 * the k-sample ELBO mean_s lw and a_theta = 1 / k; k = 1 gives a_theta = 1,
 * a_phi = -1.  Three values, float32, the negated batch means:
 *   L_tvo = -(1/B) sum_b lower_b >= L_iwae = -(1/B) sum_b iwae_b
 *                                >= L_upper = -(1/B) sum_b upper_b.
 * Gradient buffer, of L_tvo at fixed samples: the decoder's parameters get
 * -(1/B) sum_bs a_theta_bs grad [log p(h_bs) + log p(x_b | h_1,bs)] (the row
 * weight -a_theta / B where an IWAE step has dL/dlw and dpx; no dL/dh
 * stages); the encoder's get the gradient of -(1/B) sum_bs a_phi_bs
 * log q(h_bs | x_b) with a_phi and h constants: per head -a z/s on mu and
 * -a (z^2 - 1)(s - 1e-6)/s on zs with row weight a = a_phi_bs / B, the GM_FIT
 * regression of iwae_wake_sleep_step (linear in a, of either sign), per layer
 * into that layer's weight gradients only.
 * values_dev [dev], 3 floats (L_tvo, L_upper, L_iwae), may be NULL.
 * iwae_tvo_step then applies the handle's Adam to the whole buffer;
 * iwae_tvo_grad leaves the gradient in the buffer (iwae_get_grads,
 * iwae_apply_adam) and the Adam state untouched.  The noise position advances
 * once.
 * Launches: the wake forward, tvo_kernel (one wave per image, fixed reduction
 * orders, no float atomics: the values, both sets of row weights, the noise
 * position and Adam's tick in one launch), the decoder backward and its weight
 * gradients, one GM_FIT backward per encoder layer and their weight gradients,
 * Adam.  Paths: chosen as iwae_wake_sleep_step's are, over B k rows: the f32
 * row-block kernels, else the layer-wise GEMMs, never an error; never the
 * bf16x3 engine, the fused update or the weight ring.  iwae_set_graphs does not
 * apply: every launch is enqueued on the handle's stream, with no host
 * synchronisation unless the workspace grows (before anything is enqueued);
 * captured train-step graphs and engine plans survive a call that does not
 * grow it.  Deterministic.
 * IWAE_EINVAL, nothing launched and the noise position untouched (after the
 * sticky iwae_status error, returned first): cfg, betas or x NULL; k < 1 or
 * B < 1; n_part outside [1, 64]; a beta not finite, betas not strictly
 * ascending, betas[0] != 0 or betas[n_part] != 1; a wrong n_eps or a NULL
 * eps[i]; B k above 2^30; a data-parallel world > 1. */
int iwae_tvo_step(iwae_handle* h, const iwae_tvo_config* cfg, const float* betas,
                  const float* x, int B, const float* const* eps, int n_eps, float* values_dev);
int iwae_tvo_grad(iwae_handle* h, const iwae_tvo_config* cfg, const float* betas,
                  const float* x, int B, const float* const* eps, int n_eps, float* values_dev);
/* The same kernel on caller log weights lw [N][k] [dev] (iwae_log_weights',
 * iwae_ais' or iwae_refine's, say): per image lower, upper, iwae [N] [dev] and
 * per row a_theta, a_phi [N][k] [dev] as defined above, unscaled; each output
 * may be NULL, not all.  betas [host], n_part + 1 floats.  k <= 2^20 (staged
 * in LDS up to 1024, re-read beyond), N k <= 2^30.  One tvo_kernel launch on
 * the handle's stream; nothing is drawn; weights, Adam state, graphs, plans
 * and the noise position are untouched.  An image whose lw holds a NaN or an
 * infinity gets NaN in each of its outputs; its neighbours are untouched.
 * IWAE_EINVAL, nothing launched (after the sticky iwae_status error): lw or
 * betas NULL; N < 1; k outside [1, 2^20]; n_part or betas as above; N k above
 * 2^30; every output NULL. */
int iwae_tvo_weights(iwae_handle* h, const float* lw, int N, int k, const float* betas, int n_part,
                     float* lower, float* upper, float* iwae, float* a_theta, float* a_phi);

/* --- diagnostics ---------------------------------------------------------- */
/* C[M][N] = A[M][K] @ B[K][N] (all [dev], row-major, leading dims given) via
 * the f32 MFMA GEMM used on the hot path (unit-test entry). */
int iwae_debug_gemm(iwae_handle* h, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, int M, int N, int K);
/* Bytes of device workspace currently allocated by the handle. */
double iwae_workspace_bytes(const iwae_handle* h);
/* Launch counters (tests): what = 0 fused k-sample NLL kernel (mega_fwd_kernel)
 * launches, 1 those of them fed injected noise, 2 train-engine (tc_kernel)
 * launches issued (a captured step counts once, at capture), 3 NLL chunks run
 * by the weight-ring kernel (nring_kernel, a subset of 0), 4 train-step
 * forwards run by it in train mode, 5 train-step output-MLP backwards run by
 * the weight-ring backward kernel (nrb_kernel), 6 encoder / prior backwards
 * run by nre_kernel, 7 train-step graphs captured (iwae_train_step,
 * iwae_train_steps, iwae_train_steps_prepare; bench.py asserts it stays flat
 * across its timed region), 8 in-launch waits of the combined image-row
 * backward + update launch that gave up (synchronous; 0 unless the GPU was
 * shared with a kernel that held CUs for ~1 s, or IWAE_KNOB_TCU_WAIT_TEST;
 * each also sets the error iwae_status reports), 9 such combined launches
 * issued (a captured step counts once, at capture), 10 fused generation
 * launches (gen_kernel) issued by iwae_generate; IWAE_STL / IWAE_DREG steps
 * (a captured step counts once, at capture): 11 path-gradient encoder jobs
 * issued on rb_bwd_kernel (path and density jobs), 12 path-gradient launches
 * of gauss_bwd_enc_kernel (path and density); 13 row-block forward launches
 * (rb_fwd_kernel: train steps and evaluation passes on the fused row-block
 * path; none on the engine's small-batch steps or the layer-wise path), 14
 * fused update launches (update_kernel: weight gradients, Adam and the
 * fragment-major copies) issued, or recorded for the combined launch of id 9,
 * by a train step (a captured step counts once, at capture; 0 on the row-block
 * and layer-wise paths, whose steps end in the GEMM + Adam launches); 15
 * bound_kernel launches issued by train steps and forward-only bounds (a
 * captured step counts once, at capture; none where the engine's backward
 * launch computes the bound itself), 16 those of them with more than one
 * workgroup (more than 64 images and more than 8192 sample rows); 17 fused
 * second passes of iwae_posterior (post_kernel launches, one per chunk), 18
 * its layer-wise second passes (one per chunk; both also count iwae_impute's
 * second passes); 19 masked fused first passes of iwae_impute (masked
 * mega_fwd_kernel launches, one per chunk; not counted under 0), 20 its
 * masked layer-wise first passes (one per chunk); 21 pixel-masked Bernoulli
 * output launches (the tiled GEMM's masked epilogue) issued by
 * iwae_train_step_masked / iwae_forward_backward_masked / iwae_bound_masked (a
 * captured step counts once, at capture); 22 binarize_kernel launches issued by
 * iwae_binarize (one per call with n > 0); 23 fused iwae_score launches
 * (score_kernel, one per chunk), 24 its layer-wise passes (one per chunk); 25
 * fused score-gradient launches of iwae_score_grad (sg_kernel, one per chunk),
 * 26 its layer-wise score-gradient passes (one per chunk); 27 AIS transitions
 * run by iwae_ais, 28 its begin / step / end launches (n_temps (n_leapfrog +
 * 1) per call; the finish launch is not counted); 29 refinement iterations
 * run by iwae_refine, 30 its begin / step / end launches (n_iters + 1 per
 * call; the finish launch is not counted); pixel-masked calls
 * (iwae_score_masked, iwae_score_grad_masked and the passes iwae_ais_masked /
 * iwae_refine_masked run), one per chunk and not counted under 23-26: 31
 * masked fused score_kernel launches, 32 masked layer-wise score passes, 33
 * masked fused sg_kernel launches, 34 masked layer-wise score-gradient passes
 * (iwae_ais_masked and iwae_refine_masked count under 27-30 as their
 * siblings do); iwae_wake_sleep_step / iwae_wake_sleep_grad: 35 calls that
 * enqueued work, 36 GM_FIT jobs issued on rb_bwd_kernel (one per encoder
 * layer of a row-block call), 37 GM_FIT launches of gauss_bwd_enc_kernel (one
 * per encoder layer of a layer-wise call), 38 dream generations the step ran
 * itself (also counted under 10 where gen_kernel ran them); iwae_aggregate: 39
 * calls that enqueued work, 40 agg_joint_kernel launches (one per call that
 * asks for log_q_agg), 41 agg_dim_kernel launches (one per call that asks for
 * log_q_dim); TVO: 42 iwae_tvo_step / iwae_tvo_grad calls that enqueued work,
 * 43 tvo_kernel launches (one per step, grad or iwae_tvo_weights call; a
 * step's GM_FIT launches also count under 36 / 37, one per encoder layer);
 * -1 for an unknown id. */
long long iwae_debug_count(const iwae_handle* h, int what);
/* Live kernel timing: bracket every launch of one kernel class with HIP events
 * on the handle's stream -- a GEMM class (kind: 0 forward, 1 backward-data,
 * 2 backward-weight; epi: 0 store, 1 tanh, 2 Bernoulli, 3 tanh-grad) or the
 * train engine's forward (kind 10) / backward (kind 11) launch (epi ignored),
 * or a memory-bound launch of the train step: 12 Adam, 13 bound, 14 FX refresh
 * (replay only; their "FLOP" outputs are the launch's algorithmic HBM bytes);
 * 15 the fused update launch, 16 the combined job I' + update launch
 * (tcu_kernel; replay only, its FLOP output 0: the caller prices it);
 * kind = -1 disables.
 * Disables hipGraph replay while active.  iwae_profile_read synchronizes and
 * returns the summed kernel milliseconds, the algorithmic FLOPs of those
 * launches (2*rows*fan_in*fan_out each) and the launch count. */
int iwae_profile_gemm(iwae_handle* h, int kind, int epi);
int iwae_profile_read(iwae_handle* h, double* total_ms, double* total_flop, long long* launches);
/* Re-launch the last recorded launch of the profiled GEMM class n times back to
 * back between two HIP events on the handle's stream (steady-state kernel time,
 * comparable with rocprofv3's per-dispatch duration); synchronous. */
int iwae_profile_replay(iwae_handle* h, int n, double* total_ms, double* total_flop);

#ifdef __cplusplus
}
#endif
#endif /* IWAE_H */
