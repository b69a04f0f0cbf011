// Host side of libiwae_hip.so: model plan, HBM workspace, forward / backward
// orchestration of the IWAE hot path, Adam, NLL chunking, hipGraph replay and
// the extern "C" ABI declared in include/iwae.h.
//
// Reference call stacks mirrored here (F: = /root/reference/flexible_IWAE.py):
//   train_step        F:221-F:247 -> get_log_weights F:327-F:351 -> bound -> tape.gradient -> Adam
//   get_NLL           F:463-F:464 -> get_L_k with k = 5000
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/iwae.h"
#include "iwae_kernels.h"

using namespace iwae;

namespace {

thread_local std::string g_create_error;

inline int r4(int x) { return (x + 3) & ~3; }
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

struct DenseL {
  int fin = 0, fout = 0, ldw = 0;
  long long off = 0;           // into the internal parameter buffer
  long long f_off = 0, g_off = 0;  // split copies F [fout][ldF], G [fin][ldG] (bf16 hi / lo)
  int ldF = 0, ldG = 0;
  long long size() const { return (long long)(fin + 1) * ldw; }
  int max_splits = 1, splits = 1;
  int cap_splits = 1;                  // slabs allocated (>= max_splits: the large-batch weight-gradient pass may use more)
  long long slab_off = 0;
  int rows_kind = 1;           // 0: image rows (encoder layer 0), 1: sample rows
  int head_d = 0;              // a stochastic layer's (mu | zs) head: its latent width
  // fragment-major split copies FX / GX (FxSeg)
  long long fx_off = 0, gx_off = 0;
  int fx_tiles = 0, fx_steps = 0, gx_tiles = 0, gx_steps = 0;
};

struct StochL {
  int fin, H, d;
  int l1, l2, head;            // dense indices
};

struct Mat {
  float* p = nullptr;
  int ld = 0;
};

struct LayerBufs {
  Mat y1, y2, P, dP, dY2, dY1;
  Mat dPq;                     // path-gradient losses, encoder layers >= 1: dP of the density chain (layer-wise path)
};

struct KerasDense {
  int di, col0, width;
};

struct DevState {
  AdamState adam;
  uint64_t rng[2];             // [0] next forward's Philox counter, [1] last forward's
  unsigned tickets[4];         // 0: bound, 1: lse, 2: adam
  unsigned upd_ctr[2];         // the fused update's image hand-off (UpdArgs::ctr), zero between launches
  float scalars[8];            // 0: loss, 1: bound value, 2: KL (V1)
};

// Resolved loss plan (train_step dispatch, F:228-F:241)
struct Plan {
  int loss = IWAE_LOSS_IWAE;
  int B = 0, Bimg = 0, Bsplit = 0, kS = 0;
  int mode_a = BM_IWAE, mode_b = BM_NONE, mode2 = BM_NONE;
  float w_a = 1.f, w_b = 0.f;
  float p = 1.f;
  int k1 = 0, k2 = 0;
  int need_bce = 0;
  float bce_w = 0.f, wa = 1.f, wb = 0.f;
  int dpx_const = 0;
  float dpx_val = 0.f;
  int kl = 0;                  // VAE_V1 analytic KL on the last encoder layer
  int piwae = 0;               // two backward passes: dlw / dpx for the decoder, dlw2 / dpx2 (mode2) for the encoder
  int path = 0;                // IWAE_STL / IWAE_DREG: the encoder's gradient through the sampling path only
  int pix = 0;                 // pixel-masked call (MIWAE): x_in holds mask ? x : 0, x_lik mask ? x : -1
};

// Tuning knobs (iwae_set_tuning; ids, ranges and the measurements behind the
// defaults: include/iwae.h).
struct Tune {
  int engine = 1;                    // train step on the row-chain engine when it applies
  int engine_img = 1;                // ... with the first encoder layer's l2 / head on its image-row jobs
  int engine_img_bwd = 1;            // ... their backward on the image-row job at small batches too
  int engine_fold0 = 0;              // ... its l2 / head folded into the forward jobs at small batches
  int tc_xcd = 1;                    // XCD-aware job placement of the engine launches
  int tc_bound = 1;                  // the train step's bound inside the engine's backward launch
  int tc_rt = 1;                     // row tiles of 16 per engine workgroup below wide_rows
  long long wide_rows = 4097;        // sample rows from which the engine runs 32 / 64-row workgroups
  int wide_rt = 2;                   // engine row tiles per workgroup of the backward launches from
                                     // wide_rows (1, 2 or 4; the forward launch: 4)
  int img_rows_fwd = 0, img_rows_bwd = 0;   // image-row jobs I / I': rows per workgroup (0: auto)
  int x_direct = 1;                  // large-batch engine step: the input GEMM reads the caller's x (gemm_direct)
  int piwae_one = 1;                 // PIWAE: one unit-weight backward chain serves both weightings
  int upd = 1;                       // fused weight-gradient + Adam + FX update launch
  long long upd_rows = 4096;         // ... up to this many sample rows per step
  int upd_slabs = 1;                 // ... and beyond upd_rows its split-K gradient pass into the slabs
  long long upd_slab_wg = 512;       // sample-row workgroups of that pass
  int upd_waves = 16;                // update kernel workgroups: 16 waves (four per SIMD), 8 or 4
  int upd_apply = 1;                 // large batches: the update kernel sums the slabs, Adam, FX / GX (one launch)
  int tcu = 1;                       // job I' and the fused update in one launch (tcu_kernel) where it fits
  int tcu_wt = 1;                    // the combined launch's hand-off write-through (launch_tcu decides)
  int tcu_wait_test = 0;             // fault injection: every combined-launch wait gives up
  int st_wt = 5;                     // store policy of what a launch leaves to later launches (iwae_set_store_policy bits;
                                     // 1 + 4: B = 20 step 0.0977 -> 0.0957 ms, profiles/store_policy_ab.txt)
  int dw_wide = 1;                   // the slab pass run by the 208 x 128-block weight-gradient kernel (iwae_dwgrad.hip;
                                     // B = 512: 107 vs 152 us for the update kernel's pass, step 0.513 -> 0.473 ms)
  long long dw_target = 768;         // split-K target workgroups per layer of the grouped weight-gradient GEMMs
  int dw_wg = 256;                   // large-batch weight-gradient pass: workgroups its row chunks aim at
  int dw_alpha = 150;                // ... its cost model: a k step's fixed cost in MFMA tiles (measured: a
                                     // k step costs ~2 us whatever its tiles; alpha 0 / 45 / 90 / 200: 174 / 127 / 108 / 106 us)
  int smallm_rows = 32;              // first encoder layer on the few-row launches up to this many images (0: never)
  long long out_x3_rows = 8192;      // sample rows from which a train step runs the output layer's GEMMs on bf16x3 (0: never)
  int ld_align = 4;                  // workspace row strides: multiples of this many floats (4 or 32)
  int mg_waves = 8;                  // mega_fwd_kernel workgroup: 8 waves (64 rows) or 4 (32 rows, 2 per CU)
  long long nll_rows = 1LL << 20;    // sample rows per NLL chunk (measured fastest: 2^17-2^20 within 10 %)
  int nll_imgs = 0;                  // images per NLL chunk when the caller passes chunk 0 (0: nll_rows / k)
  int nll_group = 16384;             // fused evaluation paths: images per pass of the first encoder layer (ChunkWalk)
  int nring = 1;                     // NLL: the weight-ring kernel (nring_kernel) where its shapes apply
  int nring_train = 1;               // train-step forward on it (train mode) ...
  long long nr_train_rows = 4096;    // ... from this many sample rows
  int nring_bwd = 3;                 // large-batch train step: the output MLP's backward on nrb_kernel
                                     // (2: on the side stream beside the engine's backward launch;
                                     // 3: then the encoder / prior backward on nre_kernel too)
};

// the input-layer launch of a captured train step: it reads the caller's x
// directly and is re-pointed at each call's x (hipGraphExecKernelNodeSetParams)
struct XLaunch {
  int kind = 0;                      // 0: smallm_kernel (SmArgs), 1: gemm_kernel (GemmArgs)
  SmArgs sm{};
  GemmArgs gm{};
};

// Valid only during a train step or its capture (do_train, do_train_steps);
// StepScope puts every field back to these values when the call leaves.
struct StepState {
  bool in_train_step = false;        // weight-operand GEMMs of a train step stay exact f32
  bool out_x3 = false;               // ... except the output layer's two GEMMs of a large-batch step (bf16x3)
  const float* x_user = nullptr;     // caller's x read directly by the first kernel
  float* loss_out = nullptr;         // loss destination (part of the graph key)
  bool capturing = false;
  hipGraphNode_t cap_x_node = nullptr;   // the captured input-layer launch and its arguments
  XLaunch cap_x_args{};
  bool piwae_ks = false;             // the weight gradients apply the per-layer PIWAE weighting
  bool defer_launch = false;         // tc_run / run_update record their launch in Pending instead
};

// the launches recorded under defer_launch, issued by launch_pending
struct Pending {
  bool tc_have = false, upd_have = false;
  TcArgs tc{};
  int tc_rt = 1;
  size_t tc_lds = 0;
  UpdArgs upd{};
  unsigned upd_mask = 0;             // update jobs that read job I''s output (the first encoder layer's)
  int upd_cons = 0;                  // their tiles
};

// live kernel timing (HIP events around every launch of one GEMM class)
struct Prof {
  int kind = -1, epi = -1;
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  double flop = 0.0;
  // last launch of the profiled GEMM class (replayed back to back by iwae_profile_replay)
  bool have = false;
  GemmArgs args{};
  GemmKind k = GEMM_FWD; GemmEpi e = EPI_STORE;
  int tile = 0, splits = 1; bool ks = false;
  double flop1 = 0.0;
  bool is_tc = false;                // the recorded launch is an engine launch (kind 10 / 11)
  // memory-bound launches (kind 12 Adam, 13 bound, 14 FX refresh): the
  // launch as a closure and its algorithmic bytes (reported in place of FLOP)
  std::function<hipError_t(hipStream_t)> mem;
  float* scratch = nullptr;          // side-effect targets of a replayed bound launch
  float* adam = nullptr;             // parameters / m / v copies a replayed Adam launch updates
  size_t adam_bytes = 0;
  TcArgs tc{};
  int tc_rt = 1;
  size_t tc_lds = 0;
};

// launch counters (iwae_debug_count)
struct Counters {
  long long mega = 0, mega_eps = 0;  // 0, 1: mega_fwd_kernel launches (all / injected noise)
  long long tc = 0;                  // 2: train-engine launches (tc_kernel)
  long long nring = 0;               // 3: nring_kernel launches
  long long nring_train = 0;         // 4: ... of them train-step forwards
  long long nrb = 0, nre = 0;        // 5, 6: nrb_kernel / nre_kernel launches
  long long captures = 0;            // 7: train-step graphs captured (single and multi-step)
  long long tcu = 0;                 // 9: combined job I' + update launches (tcu_kernel)
  long long gen = 0;                 // 10: fused generation launches (gen_kernel)
  long long path_rb = 0;             // 11: path-gradient encoder jobs issued on rb_bwd_kernel (path and density jobs)
  long long path_gauss = 0;          // 12: path-gradient launches of gauss_bwd_enc_kernel (path and density)
  long long rb_fwd = 0;              // 13: row-block forward launches (rb_fwd_kernel)
  long long upd = 0;                 // 14: fused update launches issued or recorded by run_update
  long long bound = 0, bound_multi = 0;  // 15, 16: bound_kernel launches (all / with more than one workgroup)
  long long post = 0, post_lw = 0;       // 17, 18: iwae_posterior second passes: post_kernel launches / layer-wise passes
  long long imp = 0, imp_lw = 0;         // 19, 20: iwae_impute first passes: masked mega_fwd_kernel launches / layer-wise passes
  long long bern_mask = 0;               // 21: pixel-masked Bernoulli output launches (EPI_BERN_MASK) of train steps and bounds
  long long binarize = 0;                // 22: binarize_kernel launches (iwae_binarize)
  long long score = 0, score_lw = 0;     // 23, 24: iwae_score chunks: score_kernel launches / layer-wise passes
  long long sgrad = 0, sgrad_lw = 0;     // 25, 26: iwae_score_grad chunks: sg_kernel launches / layer-wise passes
  long long ais = 0, ais_launch = 0;     // 27, 28: iwae_ais transitions / their begin, step and end launches
  long long refine = 0, refine_launch = 0;   // 29, 30: iwae_refine iterations / its begin, step and end launches
  long long score_pix = 0, score_pix_lw = 0;   // 31, 32: pixel-masked iwae_score chunks: masked score_kernel launches / layer-wise passes
  long long sgrad_pix = 0, sgrad_pix_lw = 0;   // 33, 34: pixel-masked iwae_score_grad chunks: masked sg_kernel launches / layer-wise passes
  long long ws = 0;                      // 35: wake-sleep calls that enqueued work
  long long ws_rb = 0, ws_gauss = 0;     // 36, 37: GM_FIT jobs issued on rb_bwd_kernel / GM_FIT launches of gauss_bwd_enc_kernel
  long long ws_dream = 0;                // 38: dream generations a wake-sleep step ran itself
  long long agg = 0;                     // 39: iwae_aggregate calls that enqueued work
  long long agg_joint = 0, agg_dim = 0;  // 40, 41: agg_joint_kernel / agg_dim_kernel launches
  long long tvo = 0, tvo_launch = 0;     // 42, 43: TVO step / grad calls that enqueued work / tvo_kernel launches (weights calls too)
};

// row-chain train engine plan (device resident, per shape; iwae_train.hip)
struct TcRec {
  TcPlan* dev = nullptr;
  int rt = 1, nb[kTcMaxJobs] = {};
  int row_step = 0;                  // rows per workgroup (image-row launches; 0: 16 rt)
  size_t lds = 0;
  int acc_off = 0;                   // float offset of the per-row accumulators in LDS
  bool prepad = false;               // every op's output in a buffer of its own, padding written up front (TcJob::pre)
  double flop = 0.0;                 // algorithmic FLOPs of one launch (weight products, no bias rows)
  unsigned kinds = 0;                // op kinds of the plan's jobs (TcArgs::kinds)
};

// a captured train step (or several: iwae_train_steps)
struct GraphRec {
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  // one input-layer launch per captured step that reads the caller's x (a
  // single train step: one entry, or none when x was staged)
  std::vector<hipGraphNode_t> xs_node;
  std::vector<XLaunch> xs_args;
  std::vector<const float*> xs_cap;
  // multi-step graphs: the last node, the losses' copy, re-pointed at each call's loss_dev
  hipGraphNode_t loss_node = nullptr;
  float* loss_cap = nullptr;
};

}  // namespace

// A grow-only device workspace of one evaluation entry (floats).  reserve
// (below) leaves it holding at least `floats`: a larger one is allocated after
// the stream has drained (queued kernels may still read the old one), and
// zeroed where asked (force: whatever it holds now).  What it held is gone
// when it grows.
struct GrowWs {
  float* p = nullptr;
  size_t floats = 0;
  int reserve(iwae_handle* h, size_t need, bool zero = false, bool force = false);
};

// Offsets into such a workspace, each on a 64-float boundary.
struct WsLayout {
  size_t floats = 0;
  size_t take(size_t n) {
    const size_t o = floats;
    floats += (n + 63) & ~size_t(63);
    return o;
  }
};

struct iwae_handle {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t side_stream = nullptr;   // second branch of a train step (the fused update's sample-row tiles)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  iwae_config cfg{};
  int L = 0, xdim = 0;
  std::vector<DenseL> dense;
  std::vector<StochL> enc, dec;
  int o1 = -1, o2 = -1, o3 = -1;
  std::vector<KerasDense> keras;
  long long nparam_int = 0, nparam_keras = 0;
  int n_cu = 256;                    // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  // modes (iwae_set_path / _precision / _graphs) and knobs (iwae_set_tuning)
  int path = 0;                      // 0 auto, 1 layer-wise kernels, 2 fused row-block kernels
  int x3 = 1;                        // tiled GEMMs: 1 bf16x3 products (default), 0 exact f32 MFMA
  int nll_fused = 1;                 // NLL: fused k-sample forward (mega_fwd_kernel) when it fits
  bool use_graphs = false;
  Tune tune;
  // per-call state
  StepState step;
  Pending pend;
  Prof prof;
  Counters count;
  // persistent device state
  float* params = nullptr;
  size_t params_bytes = 0;   // allocation incl. the zero tail the row-block weight fetch may over-read
  float* adam_m = nullptr;
  float* adam_v = nullptr;
  float* grad_own = nullptr;
  float* grad = nullptr;
  __bf16* wsplit_hi = nullptr;       // split weight copies (WSplitSeg); lo = hi + wsplit_elems
  __bf16* wsplit_lo = nullptr;
  long long wsplit_elems = 0;
  long long params_version = 1, wsplit_version = 0;   // split copies current iff equal
  __bf16* fx_hi = nullptr;           // fragment-major split copies (FxSeg); lo = hi + fx_elems
  __bf16* fx_lo = nullptr;
  long long fx_elems = 0;
  long long fx_version = 0;
  bool adam_splits = false;          // the Adam launch being built also rewrites the split copies
  DevState* ds = nullptr;
  uint64_t seed = 0x5eed5eedULL;       // Philox key actually used (derived from user_seed, noise_stream)
  uint64_t user_seed = 0x5eed5eedULL;
  uint64_t noise_stream = 0;
  std::map<uint64_t, uint64_t> stream_pos;   // saved Philox counter of the streams not selected
  NrUnit* nr_units = nullptr;        // nring_kernel's unit table (device, built once: FX offsets are fixed per model)
  NrUnit* nrb_units = nullptr;       // nrb_kernel's
  NrUnit* nre_units = nullptr;       // nre_kernel's (nring_bwd 3: the encoder / prior backward on the ring too)
  unsigned* tcu_ctr = nullptr;       // tcu_kernel's in-launch counters (UpdWait::ctr; zero between launches)
  unsigned* err_host = nullptr;      // host-mapped error word a kernel sets when an in-launch wait gives up
  unsigned* err_dev = nullptr;       // ... its device address (UpdWait::err)
  // the evaluation entries' workspaces: each its own allocation, so the arena and what was captured over it
  // stay as they are
  GrowWs post_ws;                    // iwae_posterior's (weights, SIR indices, partial sums, probabilities, a chunk's
                                     // injected noise) and iwae_encode's (a chunk's injected noise)
  GrowWs sg_ws;                      // iwae_score_grad's backward rows (layer-wise path): zeroed when it grows, laid
  int sg_rows = 0;                   // out for sg_rows rows (padding columns stay zero)
  GrowWs ais_ws;                     // iwae_ais's chains (momenta, proposals, gradients per layer; H_old, the value
                                     // terms, and the weights / steps the caller did not give)
  GrowWs refine_ws;                  // iwae_refine's samples (latents, noise, gradients per layer; the value terms,
                                     // the weights, and the Adam moments the caller did not give)
  GrowWs ws_ws;                      // iwae_wake_sleep_step's own dreams (pixels [n][r4(x_dim)], then h_1 .. h_L
                                     // [n][d_i]) and its three values when the caller wants none
  GrowWs agg_ws;                     // iwae_aggregate's reference components ([M][d_1]: 1 / s and the log term, and
                                     // mu / s where the caller takes none) and its split partials
  float* loss_slots = nullptr;       // multi-step graphs: step j's loss (kGraphSteps floats), then
                                     // [kGraphSteps, 2 kGraphSteps): where a graph's copy node writes
                                     // when the call wants no losses
  // data parallelism (iwae_dp_init)
  int dp_rank = 0, dp_world = 1;
  bool dp_weighted = false;            // forward_backward writes B_local * grad and B_local at grad[nparam_int]
  ncclComm_t comm = nullptr;           // library-owned RCCL communicator (or null: the caller reduces)
  // workspace
  char* arena = nullptr;
  size_t arena_bytes = 0;
  int cap_img = 0, cap_rows = 0;
  bool cap_train = false;
  bool cap_path = false;             // the workspace holds the path-gradient losses' buffers (dh_encq, dPq)
  Mat x_in;
  Mat x_lik;                         // pixel-masked calls: the likelihood's copy of the images, mask ? x : -1
  std::vector<LayerBufs> eb, db;
  LayerBufs ob;                      // output MLP: y1 = o1, y2 = o2, P = g
  std::vector<Mat> h, eps_st, dh_out, dh_prior, dh_dec, dh_enc;
  std::vector<Mat> dh_encq;          // path-gradient losses: dL/dh[i] through the density of q(h[i+1] | h[i])
  float *logq = nullptr, *logp = nullptr, *lw = nullptr, *dlw = nullptr, *dpx = nullptr;
  float *dlw2 = nullptr, *dpx2 = nullptr, *contrib = nullptr, *part = nullptr, *part2 = nullptr;
  float *run_m = nullptr, *run_s = nullptr;
  float* ebern = nullptr;            // engine: per-row Bernoulli log-likelihood, [rows][4] (cols 1-3 zero)
  float* ebce = nullptr;             // engine: per-row Keras-BCE log-likelihood (L_alpha), same layout
  float* ones = nullptr;             // [rows] of 1.0 (the fused update's row scale of unscaled dZ)
  int ldpart = 0, npart = 0;
  float* slabs = nullptr;
  float* fslab = nullptr;            // split-K partials of the first encoder layer (fused path)
  int fslab_S = 0;
  float* oslab = nullptr;            // split-K slabs of the output layer's dX (fused path)
  int oslab_S = 0;
  bool masked = false;               // active-unit masks in force (iwae_nll_masked only)
  const float* mask[IWAE_MAX_LAYERS] = {};
  std::map<std::vector<long long>, TcRec> tc_plans;     // engine plans per shape
  int tc_fit[2] = {-1, -1};          // whether the engine's plans fit the LDS (tc_fits; [1]: with fold0), -1 unknown
  std::map<std::vector<long long>, GraphRec> graphs;    // captured train steps per graph key
};

// Resets the handle's per-step state when a train-step call leaves, on every
// exit.  (The flags engine_train_body sets -- piwae_ks, defer_launch, the
// pending launches -- are read only by the launches of that same step, and
// nothing runs between its return and the driver's: one guard at the drivers
// restores what the body's own guards used to.)
struct StepScope {
  iwae_handle* h;
  ~StepScope() {
    h->step = StepState();
    h->pend.tc_have = h->pend.upd_have = false;
  }
};

#define HIPCHK(expr)                                                           \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      h->err = std::string(#expr) + " -> " + hipGetErrorString(_e);            \
      return IWAE_EHIP;                                                        \
    }                                                                          \
  } while (0)

#define CHK(expr)                                                              \
  do {                                                                         \
    int _r = (expr);                                                           \
    if (_r != IWAE_OK) return _r;                                              \
  } while (0)

static int fail(iwae_handle* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

int GrowWs::reserve(iwae_handle* h, size_t need, bool zero, bool force) {
  if (need <= floats && !force) return IWAE_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p) (void)hipFree(p);
  p = nullptr;
  floats = 0;
  HIPCHK(hipMalloc(&p, need * sizeof(float)));
  if (zero) HIPCHK(hipMemsetAsync(p, 0, need * sizeof(float), h->stream));
  floats = need;
  return IWAE_OK;
}

// ------------------------------------------------------------------ plan
static int add_dense(iwae_handle* h, int fin, int fout, int rows_kind) {
  DenseL d;
  d.fin = fin; d.fout = fout; d.ldw = r4(fout); d.off = h->nparam_int; d.rows_kind = rows_kind;
  h->nparam_int += d.size();
  d.ldF = (fin + 1 + 31) & ~31;
  d.ldG = (fout + 31) & ~31;
  d.f_off = h->wsplit_elems;
  h->wsplit_elems += (long long)fout * d.ldF;
  d.g_off = h->wsplit_elems;
  h->wsplit_elems += (long long)fin * d.ldG;
  h->wsplit_elems = (h->wsplit_elems + 63) & ~63LL;
  h->dense.push_back(d);
  return (int)h->dense.size() - 1;
}

static StochL add_stoch(iwae_handle* h, int fin, int H, int d, int rows_kind) {
  StochL s{fin, H, d, 0, 0, 0};
  s.l1 = add_dense(h, fin, H, rows_kind);
  s.l2 = add_dense(h, H, H, rows_kind);
  s.head = add_dense(h, H, 2 * d, rows_kind);   // [lmu | lstd] concatenated along N
  h->dense[s.head].head_d = d;
  h->keras.push_back({s.l1, 0, H});
  h->keras.push_back({s.l2, 0, H});
  h->keras.push_back({s.head, 0, d});
  h->keras.push_back({s.head, d, d});
  return s;
}
static void destroy_graph(GraphRec& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
}

// drop every captured train step: something they captured (a kernel argument,
// a path decision) is about to change
static void invalidate_graphs(iwae_handle* h) {
  for (auto& kv : h->graphs) destroy_graph(kv.second);
  h->graphs.clear();
}

// drop the engine plans (built per shape for the current knobs; they point into the arena)
static void invalidate_tc_plans(iwae_handle* h) {
  for (auto& kv : h->tc_plans) (void)hipFree(kv.second.dev);
  h->tc_plans.clear();
}

static void free_workspace(iwae_handle* h) {
  invalidate_graphs(h);
  invalidate_tc_plans(h);
  if (h->arena) (void)hipFree(h->arena);
  h->arena = nullptr;
  h->arena_bytes = 0;
  h->cap_img = h->cap_rows = 0;
  h->cap_train = false;
  h->cap_path = false;
}

// (path: a train step of a path-gradient loss, which needs dh_encq / dPq too)
static int ensure_capacity(iwae_handle* h, int Bimg, int rows, bool train, bool path = false) {
  if (h->arena && Bimg <= h->cap_img && rows <= h->cap_rows && (!train || h->cap_train) && (!path || h->cap_path))
    return IWAE_OK;
  HIPCHK(hipStreamSynchronize(h->stream));
  Bimg = std::max(Bimg, h->cap_img);
  rows = std::max(rows, h->cap_rows);
  train = train || h->cap_train;
  path = path || h->cap_path;
  free_workspace(h);
  // ---- layout pass (offsets in floats, 64-float aligned)
  size_t off = 0;
  auto take = [&](size_t n) {
    size_t o = off;
    off += (n + 63) & ~size_t(63);
    return o;
  };
  struct Pending { Mat* m; size_t o; };
  std::vector<std::pair<float**, size_t>> vecs;
  std::vector<Pending> mats;
  const int la = h->tune.ld_align;
  auto mat = [&](Mat& m, int nrows, int width) {
    m.ld = (width + la - 1) / la * la;
    mats.push_back({&m, take((size_t)nrows * m.ld)});
  };
  auto vec = [&](float*& p, size_t n) { vecs.push_back({&p, take(n)}); };
  const int L = h->L;
  h->eb.assign(L, LayerBufs());
  h->db.assign(std::max(L - 1, 0), LayerBufs());
  h->h.assign(L, Mat());
  h->eps_st.assign(L, Mat());
  h->dh_out.assign(1, Mat());
  h->dh_prior.assign(L, Mat());
  h->dh_dec.assign(L, Mat());
  h->dh_enc.assign(L, Mat());
  h->dh_encq.assign(L, Mat());
  mat(h->x_in, Bimg, h->xdim + 1);
  for (int i = 0; i < L; ++i) {
    const StochL& s = h->enc[i];
    const int R = i == 0 ? Bimg : rows;
    mat(h->eb[i].y1, R, s.H + 1);
    mat(h->eb[i].y2, R, s.H + 1);
    mat(h->eb[i].P, R, 2 * s.d + 1);
    if (train) {
      mat(h->eb[i].dP, R, 2 * s.d);
      mat(h->eb[i].dY2, R, s.H);
      mat(h->eb[i].dY1, R, s.H);
    }
    mat(h->h[i], rows, s.d + 1);
    if (train) mat(h->eps_st[i], rows, s.d);
  }
  for (int i = 0; i < L - 1; ++i) {
    const StochL& s = h->dec[i];
    mat(h->db[i].y1, rows, s.H + 1);
    mat(h->db[i].y2, rows, s.H + 1);
    mat(h->db[i].P, rows, 2 * s.d + 1);
    if (train) {
      mat(h->db[i].dP, rows, 2 * s.d);
      mat(h->db[i].dY2, rows, s.H);
      mat(h->db[i].dY1, rows, s.H);
    }
  }
  const int Hd = h->dense[h->o1].fout;
  mat(h->ob.y1, rows, Hd + 1);
  mat(h->ob.y2, rows, Hd + 1);
  if (train) {
    mat(h->ob.P, rows, h->xdim);   // g = dLoss/dlogit factor
    mat(h->ob.dY2, rows, Hd);
    mat(h->ob.dY1, rows, Hd);
    const int d0 = h->enc[0].d;
    mat(h->dh_out[0], rows, d0);
    for (int i = 0; i < L; ++i) {
      const int di = h->enc[i].d;
      if (i <= L - 2) { mat(h->dh_prior[i], rows, di); mat(h->dh_enc[i], rows, di); }
      if (i >= 1) mat(h->dh_dec[i], rows, di);
      if (path && i <= L - 2) mat(h->dh_encq[i], rows, di);
      if (path && i >= 1) mat(h->eb[i].dPq, rows, 2 * di);
    }
  }
  h->npart = (int)cdiv(h->xdim, 32);
  h->ldpart = r4(h->npart);
  vec(h->part, (size_t)rows * h->ldpart);
  vec(h->part2, (size_t)rows * h->ldpart);
  vec(h->logq, rows); vec(h->logp, rows); vec(h->lw, rows);
  vec(h->dlw, rows); vec(h->dpx, rows); vec(h->dlw2, rows); vec(h->dpx2, rows);
  vec(h->contrib, Bimg); vec(h->run_m, Bimg); vec(h->run_s, Bimg);
  vec(h->ebern, (size_t)rows * 4);
  vec(h->ebce, (size_t)rows * 4);
  vec(h->ones, rows);
  h->fslab_S = (int)std::min<long long>(16, cdiv(h->xdim + 1, 64));
  vec(h->fslab, (size_t)h->fslab_S * Bimg * r4(h->enc[0].H + 1));
  if (train && rows <= 65536) {
    h->oslab_S = 4;
    vec(h->oslab, (size_t)h->oslab_S * rows * r4(Hd));
  } else {
    h->oslab_S = 0;
  }
  size_t slab_total = 0;
  if (train) {
    for (auto& d : h->dense) {
      const long long R = d.rows_kind == 0 ? Bimg : rows;
      const long long tiles = cdiv(d.fin + 1, 64) * cdiv(d.fout, 64);
      long long S = std::max(1LL, cdiv(h->tune.dw_target, tiles));   // split-K target workgroups per layer
      // at most 16 slabs (the Adam kernel sums up to 16 with all loads in flight;
      // more slabs only add write + read traffic at large batch)
      S = std::min(S, std::min(16LL, std::max(1LL, cdiv(R, 64))));
      d.max_splits = (int)S;
      // the large-batch weight-gradient pass (run_dw) balances its workgroups with up to 32 row chunks
      d.cap_splits = (int)std::max<long long>(S, std::min(32LL, std::max(1LL, cdiv(R, 32))));
      d.slab_off = (long long)slab_total;
      slab_total += (size_t)((d.size() * d.cap_splits + 63) & ~63LL);
    }
  }
  size_t slab_base = take(slab_total);
  // (last, so every other buffer keeps its offset: a few images, always there,
  // so a pixel-masked call never regrows the arena under a captured graph)
  mat(h->x_lik, Bimg, h->xdim + 1);
  const size_t bytes = off * sizeof(float);
  HIPCHK(hipMalloc(&h->arena, bytes));
  h->arena_bytes = bytes;
  HIPCHK(hipMemsetAsync(h->arena, 0, bytes, h->stream));
  float* base = reinterpret_cast<float*>(h->arena);
  for (auto& pm : mats) pm.m->p = base + pm.o;
  for (auto& pv : vecs) *pv.first = base + pv.second;
  h->slabs = train ? base + slab_base : nullptr;
  // ones columns of every Dense input (bias folded into W_aug's last row)
  HIPCHK(launch_fill_col(h->stream, h->x_in.p, Bimg, h->x_in.ld, h->xdim, 1.f));
  for (int i = 0; i < L; ++i) {
    const int R = i == 0 ? Bimg : rows;
    HIPCHK(launch_fill_col(h->stream, h->eb[i].y1.p, R, h->eb[i].y1.ld, h->enc[i].H, 1.f));
    HIPCHK(launch_fill_col(h->stream, h->eb[i].y2.p, R, h->eb[i].y2.ld, h->enc[i].H, 1.f));
    HIPCHK(launch_fill_col(h->stream, h->h[i].p, rows, h->h[i].ld, h->enc[i].d, 1.f));
  }
  for (int i = 0; i < L - 1; ++i) {
    HIPCHK(launch_fill_col(h->stream, h->db[i].y1.p, rows, h->db[i].y1.ld, h->dec[i].H, 1.f));
    HIPCHK(launch_fill_col(h->stream, h->db[i].y2.p, rows, h->db[i].y2.ld, h->dec[i].H, 1.f));
  }
  HIPCHK(launch_fill_col(h->stream, h->ob.y1.p, rows, h->ob.y1.ld, Hd, 1.f));
  HIPCHK(launch_fill_col(h->stream, h->ob.y2.p, rows, h->ob.y2.ld, Hd, 1.f));
  HIPCHK(launch_fill_col(h->stream, h->ones, rows, 1, 0, 1.f));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->cap_img = Bimg;
  h->cap_rows = rows;
  h->cap_train = train;
  h->cap_path = train && path;
  return IWAE_OK;
}

// --------------------------------------------------------------- GEMMs
// pre-split B operand (weights) for a bf16x3 GEMM: only outside the train step
static bool use_split_b(const iwae_handle* h) { return h->x3 && !h->step.in_train_step; }
// split-weight (bf16x3) operand for Dense d: every tiled GEMM outside the train
// step; inside it only the output layer of a large-batch step, whose split copy
// the step refreshes first (run_wsplit_seg)
static bool split_b_for(const iwae_handle* h, const DenseL& d) {
  return use_split_b(h) || (h->step.out_x3 && &d == &h->dense[h->o3]);
}

static int choose_tile(long long M, long long N, int splits) {
  return (cdiv(M, 128) * cdiv(N, 128) * splits >= 512) ? 1 : 0;
}

static bool prof_match(iwae_handle* h, GemmKind kind, GemmEpi epi) {
  return h->prof.kind == (int)kind && h->prof.epi == (int)epi;
}

static void prof_note(iwae_handle* h, GemmKind kind, GemmEpi epi, int tile, int splits, bool ks, const GemmArgs& a,
                      double flop) {
  if (!prof_match(h, kind, epi)) return;
  h->prof.have = true; h->prof.args = a; h->prof.k = kind; h->prof.e = epi;
  h->prof.tile = tile; h->prof.splits = splits; h->prof.ks = ks; h->prof.flop1 = flop;
}

static int prof_begin(iwae_handle* h, GemmKind kind, GemmEpi epi, double flop) {
  if (!prof_match(h, kind, epi)) return IWAE_OK;
  if (h->prof.used + 2 > h->prof.ev.size()) {
    for (int i = 0; i < 256; ++i) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      h->prof.ev.push_back(e);
    }
  }
  HIPCHK(hipEventRecord(h->prof.ev[h->prof.used], h->stream));
  h->prof.flop += flop;
  return IWAE_OK;
}

static int prof_end(iwae_handle* h, GemmKind kind, GemmEpi epi) {
  if (!prof_match(h, kind, epi)) return IWAE_OK;
  HIPCHK(hipEventRecord(h->prof.ev[h->prof.used + 1], h->stream));
  h->prof.used += 2;
  return IWAE_OK;
}

static int gemm_fwd(iwae_handle* h, GemmEpi epi, const Mat& X, int rows, const DenseL& d, Mat& Y,
                    GemmArgs extra = GemmArgs{}) {
  GemmArgs a = extra;
  a.x3 = split_b_for(h, d) ? 1 : 0;       // weight operand: exact f32 inside the train step (but see out_x3)
  a.A = X.p; a.lda = X.ld;
  a.B = h->params + d.off; a.ldb = d.ldw;
  a.C = Y.p; a.ldc = Y.ld;
  a.M = rows; a.N = d.fout; a.K = d.fin + 1;
  a.kchunk = a.K;
  a.c_split_stride = 0;
  if (split_b_for(h, d)) { a.Bhi = h->wsplit_hi + d.f_off; a.Blo = h->wsplit_lo + d.f_off; a.ldbx = d.ldF; }
  CHK(prof_begin(h, GEMM_FWD, epi, 2.0 * rows * d.fout * d.fin));
  prof_note(h, GEMM_FWD, epi, choose_tile(a.M, a.N, 1), 1, false, a, 2.0 * rows * d.fout * d.fin);
  HIPCHK(launch_gemm(h->stream, GEMM_FWD, epi, choose_tile(a.M, a.N, 1), 1, false, a));
  CHK(prof_end(h, GEMM_FWD, epi));
  return IWAE_OK;
}

// dX[rows][fin] = dZ[rows][fout] . W[:fin]^T  (optionally * rowscale, * (1-Y^2))
static int gemm_bwd_data(iwae_handle* h, const Mat& dZ, int rows, const DenseL& d, Mat& dX,
                         const Mat* Y, const float* rowscale) {
  GemmArgs a{};
  a.x3 = split_b_for(h, d) ? 1 : 0;       // weight operand: exact f32 inside the train step (but see out_x3)
  a.A = dZ.p; a.lda = dZ.ld;
  a.B = h->params + d.off; a.ldb = d.ldw;
  a.C = dX.p; a.ldc = dX.ld;
  a.M = rows; a.N = d.fin; a.K = d.fout;
  a.kchunk = a.K;
  a.rowscale = rowscale;
  if (split_b_for(h, d)) { a.Bhi = h->wsplit_hi + d.g_off; a.Blo = h->wsplit_lo + d.g_off; a.ldbx = d.ldG; }
  GemmEpi epi = EPI_STORE;
  if (Y) { a.aux = Y->p; a.ldaux = Y->ld; epi = EPI_TANH_GRAD; }
  CHK(prof_begin(h, GEMM_BWD_DATA, epi, 2.0 * rows * d.fout * d.fin));
  HIPCHK(launch_gemm(h->stream, GEMM_BWD_DATA, epi, choose_tile(a.M, a.N, 1), 1, false, a));
  CHK(prof_end(h, GEMM_BWD_DATA, epi));
  return IWAE_OK;
}

// slabs of dW_aug[fin+1][fout] = X_aug[rows][fin+1]^T . dZ[rows][fout], split over rows (the slab count: d.splits)
static GemmArgs bwd_weight_args(const iwae_handle* h, const Mat& X, const Mat& dZ, int rows, DenseL& d,
                                const float* kscale) {
  GemmArgs a{};
  a.x3 = h->x3;
  a.A = X.p; a.lda = X.ld;
  a.B = dZ.p; a.ldb = dZ.ld;
  a.C = h->slabs + d.slab_off; a.ldc = d.ldw;
  a.M = d.fin + 1; a.N = d.fout; a.K = rows;
  const long long S = std::min<long long>(d.max_splits, std::max(1LL, cdiv(rows, 64)));
  a.kchunk = (int)(cdiv(cdiv(rows, S), 64) * 64);
  d.splits = (int)cdiv(rows, a.kchunk);
  a.c_split_stride = d.size(); a.kscale = kscale;
  return a;
}
static int gemm_bwd_weight(iwae_handle* h, const Mat& X, const Mat& dZ, int rows, DenseL& d, const float* kscale) {
  const GemmArgs a = bwd_weight_args(h, X, dZ, rows, d, kscale);
  CHK(prof_begin(h, GEMM_BWD_WEIGHT, EPI_STORE, 2.0 * rows * d.fout * (d.fin + 1)));
  HIPCHK(launch_gemm(h->stream, GEMM_BWD_WEIGHT, EPI_STORE, 0, d.splits, kscale != nullptr, a));
  CHK(prof_end(h, GEMM_BWD_WEIGHT, EPI_STORE));
  return IWAE_OK;
}

static int stoch_fwd(iwae_handle* h, const StochL& s, const Mat& in, int rows, LayerBufs& b) {
  CHK(gemm_fwd(h, EPI_TANH, in, rows, h->dense[s.l1], b.y1));
  CHK(gemm_fwd(h, EPI_TANH, b.y1, rows, h->dense[s.l2], b.y2));
  CHK(gemm_fwd(h, EPI_STORE, b.y2, rows, h->dense[s.head], b.P));
  return IWAE_OK;
}

static int stoch_bwd(iwae_handle* h, const StochL& s, const Mat& in, int rows, LayerBufs& b, bool do_dw,
                     Mat* dx) {
  CHK(gemm_bwd_data(h, b.dP, rows, h->dense[s.head], b.dY2, &b.y2, nullptr));
  if (do_dw) CHK(gemm_bwd_weight(h, b.y2, b.dP, rows, h->dense[s.head], nullptr));
  CHK(gemm_bwd_data(h, b.dY2, rows, h->dense[s.l2], b.dY1, &b.y1, nullptr));
  if (do_dw) CHK(gemm_bwd_weight(h, b.y1, b.dY2, rows, h->dense[s.l2], nullptr));
  if (dx) CHK(gemm_bwd_data(h, b.dY1, rows, h->dense[s.l1], *dx, nullptr, nullptr));
  if (do_dw) CHK(gemm_bwd_weight(h, in, b.dY1, rows, h->dense[s.l1], nullptr));
  return IWAE_OK;
}

// dX-only pass of an encoder layer's density chain (path-gradient losses):
// b.dPq through the three transposed layers into dx, no weight gradients.
// b.dY2 / b.dY1 are its scratch: stoch_bwd's weight-gradient GEMMs, their only
// readers, are ahead of it on the stream.
static int stoch_bwd_dx(iwae_handle* h, const StochL& s, int rows, LayerBufs& b, Mat& dx) {
  CHK(gemm_bwd_data(h, b.dPq, rows, h->dense[s.head], b.dY2, &b.y2, nullptr));
  CHK(gemm_bwd_data(h, b.dY2, rows, h->dense[s.l2], b.dY1, &b.y1, nullptr));
  CHK(gemm_bwd_data(h, b.dY1, rows, h->dense[s.l1], dx, nullptr, nullptr));
  return IWAE_OK;
}

// ------------------------------------------------------------ loss plan
static int make_plan(iwae_handle* h, const iwae_loss_config* lc, int B, Plan& P) {
  if (!lc) return fail(h, IWAE_EINVAL, "loss config is NULL");
  if (B <= 0) return fail(h, IWAE_EINVAL, "batch must be positive");
  if (lc->k <= 0) return fail(h, IWAE_EINVAL, "k must be positive");
  P = Plan();
  P.loss = lc->loss;
  P.B = B; P.Bimg = B; P.Bsplit = B; P.kS = lc->k;
  P.p = lc->p;
  switch (lc->loss) {
    case IWAE_LOSS_VAE: P.mode_a = BM_VAE; break;
    case IWAE_LOSS_IWAE: P.mode_a = BM_IWAE; break;
    // value and decoder gradient of IWAE; the encoder's through the sampling
    // path only, weighted by the softmax (STL) or its square (DReG: a second
    // pass on dlw2 / dpx2, PIWAE's structure)
    case IWAE_LOSS_IWAE_STL: P.mode_a = BM_IWAE; P.path = 1; break;
    case IWAE_LOSS_IWAE_DREG: P.mode_a = BM_IWAE; P.mode2 = BM_SM2; P.piwae = 1; P.path = 1; break;
    case IWAE_LOSS_L_POWER_P:
      if (!(lc->p > 0.f) && !(lc->p < 0.f)) return fail(h, IWAE_EINVAL, "L_power_p needs p != 0");
      P.mode_a = BM_POWER; break;
    case IWAE_LOSS_L_MEDIAN:
      if (lc->k > 1024) return fail(h, IWAE_EINVAL, "L_median supports k <= 1024");
      P.mode_a = BM_MEDIAN; break;
    case IWAE_LOSS_MIWAE:
    case IWAE_LOSS_PIWAE:
      if (lc->k1 <= 0 || lc->k2 <= 0 || lc->k1 * lc->k2 != lc->k)
        return fail(h, IWAE_EINVAL, "MIWAE/PIWAE need k1*k2 == k");
      if (lc->k > 1024) return fail(h, IWAE_EINVAL, "MIWAE/PIWAE support k <= 1024");
      P.k1 = lc->k1; P.k2 = lc->k2;
      if (lc->loss == IWAE_LOSS_MIWAE) {
        P.mode_a = BM_MIWAE;
      } else {
        P.mode_a = BM_IWAE; P.mode2 = BM_MIWAE; P.piwae = 1;
      }
      break;
    case IWAE_LOSS_CIWAE:
      P.Bimg = 2 * B; P.Bsplit = B;
      P.mode_a = BM_VAE; P.w_a = lc->beta;            // beta * get_L      (F:383)
      P.mode_b = BM_IWAE; P.w_b = 1.f - lc->beta;     // (1-beta) * get_L_k
      break;
    case IWAE_LOSS_L_ALPHA:
      P.mode_a = BM_VAE; P.w_a = lc->alpha;            // alpha * L          (F:401)
      P.need_bce = 1; P.bce_w = 1.f - lc->alpha;       // (1-alpha) * E_q log p(x|h)
      P.wa = lc->alpha; P.wb = 1.f - lc->alpha;
      P.dpx_const = 1; P.dpx_val = -1.f / ((float)lc->k * (float)B);
      break;
    case IWAE_LOSS_VAE_V1:
      P.mode_a = BM_NONE; P.w_a = 0.f;
      P.need_bce = 1; P.bce_w = 1.f;                   // E_q log p(x|h) (F:456) - KL (F:458)
      P.wa = 0.f; P.wb = 1.f;
      P.dpx_const = 1; P.dpx_val = -1.f / ((float)lc->k * (float)B);
      P.kl = 1;
      break;
    default:
      return fail(h, IWAE_EINVAL, "unknown loss_function id " + std::to_string(lc->loss));
  }
  return IWAE_OK;
}

// ------------------------------------------------------------- forward
struct EpsSet {
  const float* a[IWAE_MAX_LAYERS];
  const float* b[IWAE_MAX_LAYERS];
};

static int parse_eps(iwae_handle* h, const Plan& P, const float* const* eps, int n_eps, EpsSet& E) {
  std::memset(&E, 0, sizeof(E));
  if (!eps || n_eps == 0) return IWAE_OK;
  const int need = (P.Bimg != P.Bsplit) ? 2 * h->L : h->L;
  if (n_eps != need)
    return fail(h, IWAE_EINVAL, "expected " + std::to_string(need) + " eps buffers, got " +
                                   std::to_string(n_eps));
  for (int i = 0; i < h->L; ++i) {
    E.a[i] = eps[i];
    if (P.Bimg != P.Bsplit) E.b[i] = eps[h->L + i];
    if (!E.a[i] || (P.Bimg != P.Bsplit && !E.b[i])) return fail(h, IWAE_EINVAL, "NULL eps buffer");
  }
  return IWAE_OK;
}

// Encoder + prior + output layer.  Leaves part/logp/logq (and g when train).
static bool use_fused(const iwae_handle* h, const Plan& P);
static int fused_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool train);

// Layer-wise encoder (F:56-F:75): h[i] sampled, log q into h->logq.  With
// active-unit masks set (get_NLL_without_inactive_units, F:466-F:483) each
// sample is multiplied by its layer's mask before log q and the next layer.
static int encoder_fwd(iwae_handle* h, const Plan& P, const EpsSet& E, bool train) {
  const int L = h->L, kS = P.kS, M = P.Bimg * kS;
  CHK(stoch_fwd(h, h->enc[0], h->x_in, P.Bimg, h->eb[0]));
  for (int i = 0; i < L; ++i) {
    if (i > 0) CHK(stoch_fwd(h, h->enc[i], h->h[i - 1], M, h->eb[i]));
    GaussArgs g{};
    g.P = h->eb[i].P.p; g.ldP = h->eb[i].P.ld; g.prow_div = i == 0 ? kS : 1; g.d = h->enc[i].d;
    g.H = h->h[i].p; g.ldH = h->h[i].ld;
    g.eps_a = E.a[i]; g.eps_b = E.b[i];
    g.kS = kS; g.Bsplit = P.Bsplit; g.Bimg = P.Bimg;
    g.seed = h->seed; g.rng_base = &h->ds->rng[0]; g.layer = i;
    g.out = h->logq; g.accumulate = i > 0; g.M = M;
    if (train) { g.eps_out = h->eps_st[i].p; g.ld_eps_out = h->eps_st[i].ld; }
    g.mask = h->masked ? h->mask[i] : nullptr;
    HIPCHK(launch_gauss_fwd(h->stream, 0, g));
  }
  return IWAE_OK;
}

// Layer-wise prior log p(h) of the M sampled rows into h->logp, or out (F:134-F:142)
static int prior_fwd(iwae_handle* h, int M, float* out = nullptr) {
  const int L = h->L;
  if (!out) out = h->logp;
  {
    GaussArgs g{};
    g.d = h->enc[L - 1].d; g.H = h->h[L - 1].p; g.ldH = h->h[L - 1].ld;
    g.out = out; g.accumulate = 0; g.M = M;
    HIPCHK(launch_gauss_fwd(h->stream, 2, g));
  }
  for (int i = 0; i < L - 1; ++i) {
    CHK(stoch_fwd(h, h->dec[i], h->h[L - 1 - i], M, h->db[i]));
    GaussArgs g{};
    g.P = h->db[i].P.p; g.ldP = h->db[i].P.ld; g.prow_div = 1; g.d = h->dec[i].d;
    g.H = h->h[L - 2 - i].p; g.ldH = h->h[L - 2 - i].ld;
    g.out = out; g.accumulate = 1; g.M = M;
    HIPCHK(launch_gauss_fwd(h->stream, 1, g));
  }
  return IWAE_OK;
}

static int layerwise_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool train);
static int forward_core(iwae_handle* h, const Plan& P, const EpsSet& E, bool train) {
  if (use_fused(h, P)) return fused_forward(h, P, E, train);
  return layerwise_forward(h, P, E, train);
}

static int layerwise_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool train) {
  const int kS = P.kS, M = P.Bimg * kS;
  CHK(encoder_fwd(h, P, E, train));
  CHK(prior_fwd(h, M));
  // output MLP + Bernoulli (F:89-F:96, F:123-F:129)
  CHK(gemm_fwd(h, EPI_TANH, h->h[0], M, h->dense[h->o1], h->ob.y1));
  CHK(gemm_fwd(h, EPI_TANH, h->ob.y1, M, h->dense[h->o2], h->ob.y2));
  {
    GemmArgs ex{};
    // (a pixel-masked call: the -1 copy and the epilogue that selects by it)
    const Mat& xl = P.pix ? h->x_lik : h->x_in;
    ex.aux = xl.p; ex.ldaux = xl.ld; ex.x_row_div = kS;
    ex.part = h->part; ex.part2 = h->part2; ex.ldpart = h->ldpart;
    ex.wa = P.wa; ex.wb = P.wb;
    ex.store_g = train ? 1 : 0;
    ex.need_bce = P.need_bce;
    Mat gm = h->ob.P;
    if (!train) { gm.p = nullptr; gm.ld = 0; }
    CHK(gemm_fwd(h, P.pix ? EPI_BERN_MASK : EPI_BERN, h->ob.y2, M, h->dense[h->o3], gm, ex));
    if (P.pix) h->count.bern_mask++;
  }
  return IWAE_OK;
}

// Layer-wise first pass of iwae_impute: forward_core's encoder and prior on
// x_in (already mask ? x : 0), the output Dense storing its logits in Z, then
// the masked Bernoulli row sums where lse_kernel reads a row's likelihood term
// ([rows][4], one partial).  No GEMM instantiation of the train step changes.
static int impute_layerwise_fwd(iwae_handle* h, const Plan& P, const EpsSet& E, const float* mask, Mat Z, float* part,
                                bool to_probs) {
  const int M = P.Bimg * P.kS;
  CHK(encoder_fwd(h, P, E, false));
  CHK(prior_fwd(h, M));
  CHK(gemm_fwd(h, EPI_TANH, h->h[0], M, h->dense[h->o1], h->ob.y1));
  CHK(gemm_fwd(h, EPI_TANH, h->ob.y1, M, h->dense[h->o2], h->ob.y2));
  CHK(gemm_fwd(h, EPI_STORE, h->ob.y2, M, h->dense[h->o3], Z));
  HIPCHK(launch_impute_rowsum(h->stream, Z.p, Z.ld, M, P.kS, h->x_in.p, h->x_in.ld, mask, h->xdim, part,
                              to_probs ? 1 : 0));
  return IWAE_OK;
}

static BoundArgs make_bound_args(iwae_handle* h, const Plan& P, bool train, float sign, float* value_out,
                                 bool adam_tick, bool engine) {
  BoundArgs b{};
  b.part = h->part; b.part2 = P.need_bce ? h->part2 : nullptr; b.ldpart = h->ldpart; b.npart = h->npart;
  b.logp = h->logp; b.logq = h->logq;
  if (engine) {                     // row totals (cols 0-1 summed)
    b.part = h->ebern; b.ldpart = 4; b.npart = 1;
    b.part2 = P.need_bce ? h->ebce : nullptr;
  }
  b.lw = h->lw; b.contrib = h->contrib;
  b.dlw = train ? h->dlw : nullptr; b.dpx = train ? h->dpx : nullptr;
  b.dlw2 = (train && P.piwae) ? h->dlw2 : nullptr; b.dpx2 = (train && P.piwae) ? h->dpx2 : nullptr;
  b.kS = P.kS; b.Bimg = P.Bimg; b.Bsplit = P.Bsplit;
  b.mode_a = P.mode_a; b.w_a = P.w_a; b.mode_b = P.mode_b; b.w_b = P.w_b; b.mode2 = P.mode2;
  b.p = P.p; b.k1 = P.k1; b.k2 = P.k2;
  b.bce_w = P.bce_w; b.dpx_const = P.dpx_val; b.dpx_is_const = P.dpx_const;
  b.loss = value_out; b.loss_sign = sign;
  b.loss_add = nullptr;
  if (P.kl) {
    // training loss = -(E - KL) = -E + KL ; bound value = E - KL  (F:459)
    b.loss_add = &h->ds->scalars[2];
    b.loss_add_coef = sign > 0 ? -1.f : 1.f;
  }
  b.ticket = &h->ds->tickets[0]; b.rng_base = &h->ds->rng[0];
  b.adam_step = adam_tick ? &h->ds->adam.t : nullptr;
  return b;
}

static int run_bound(iwae_handle* h, const Plan& P, bool train, float sign, float* value_out,
                     bool adam_tick = false, bool engine = false) {
  if (P.kl) {
    const int Lm1 = h->L - 1;
    const int rows = Lm1 == 0 ? P.Bimg : P.Bimg * P.kS;
    HIPCHK(launch_kl_v1(h->stream, h->eb[Lm1].P.p, h->eb[Lm1].P.ld, h->enc[Lm1].d, rows,
                        &h->ds->scalars[2]));
  }
  const BoundArgs b = make_bound_args(h, P, train, sign, value_out, adam_tick, engine);
  HIPCHK(launch_bound(h->stream, b));
  h->count.bound++;
  if (bound_grid(b) > 1) h->count.bound_multi++;
  if (h->prof.kind == 13 && !h->prof.have) {
    // replays write the loss, Philox base and Adam step into scratch instead
    if (!h->prof.scratch) HIPCHK(hipMalloc(&h->prof.scratch, 64 * sizeof(float)));
    HIPCHK(hipMemsetAsync(h->prof.scratch, 0, 64 * sizeof(float), h->stream));
    BoundArgs r = b;
    r.loss = h->prof.scratch;
    r.rng_base = reinterpret_cast<uint64_t*>(h->prof.scratch + 8);
    r.adam_step = b.adam_step ? reinterpret_cast<decltype(b.adam_step)>(h->prof.scratch + 16) : nullptr;
    r.ticket = reinterpret_cast<unsigned*>(h->prof.scratch + 24);
    h->prof.mem = [r](hipStream_t st) { return launch_bound(st, r); };
    const double rows = (double)P.Bimg * P.kS;
    // logq, logp, the row's 4 partial-sum floats in; lw, dlw, dpx out; contrib per image
    h->prof.flop1 = rows * (2 + 4 + 1 + (b.dlw ? 1 : 0) + (b.dpx ? 1 : 0)) * 4.0 + (double)P.Bimg * 4.0;
    h->prof.have = true;
  }
  return IWAE_OK;
}

// --------------------------------------------------------------- backward
static int decoder_bwd(iwae_handle* h, const Plan& P, const float* dlw, const float* dpx, bool do_dw,
                       bool do_dx) {
  const int L = h->L, M = P.Bimg * P.kS;
  // output MLP: dlogit = dpx[row] * g
  CHK(gemm_bwd_data(h, h->ob.P, M, h->dense[h->o3], h->ob.dY2, &h->ob.y2, dpx));
  if (do_dw) CHK(gemm_bwd_weight(h, h->ob.y2, h->ob.P, M, h->dense[h->o3], dpx));
  CHK(gemm_bwd_data(h, h->ob.dY2, M, h->dense[h->o2], h->ob.dY1, &h->ob.y1, nullptr));
  if (do_dw) CHK(gemm_bwd_weight(h, h->ob.y1, h->ob.dY2, M, h->dense[h->o2], nullptr));
  if (do_dx) CHK(gemm_bwd_data(h, h->ob.dY1, M, h->dense[h->o1], h->dh_out[0], nullptr, nullptr));
  if (do_dw) CHK(gemm_bwd_weight(h, h->h[0], h->ob.dY1, M, h->dense[h->o1], nullptr));
  // decoder prior layers p(h_t | h_src)
  for (int i = 0; i < L - 1; ++i) {
    const int t = L - 2 - i, src = L - 1 - i;
    GaussBwdArgs g{};
    g.P = h->db[i].P.p; g.ldP = h->db[i].P.ld; g.prow_div = 1; g.d = h->dec[i].d;
    g.H = h->h[t].p; g.ldH = h->h[t].ld;
    g.dlw = dlw;
    g.dP = h->db[i].dP.p; g.lddP = h->db[i].dP.ld;
    g.dh_out = h->dh_prior[t].p; g.ldh_out = h->dh_prior[t].ld;
    g.M = M;
    HIPCHK(launch_gauss_bwd(h->stream, 1, g));
    CHK(stoch_bwd(h, h->dec[i], h->h[src], M, h->db[i], do_dw, do_dx ? &h->dh_dec[src] : nullptr));
  }
  return IWAE_OK;
}

static int encoder_bwd(iwae_handle* h, const Plan& P, const float* dlw) {
  const int L = h->L, kS = P.kS, M = P.Bimg * kS;
  for (int i = L - 1; i >= 0; --i) {
    GaussBwdArgs g{};
    g.P = h->eb[i].P.p; g.ldP = h->eb[i].P.ld; g.prow_div = i == 0 ? kS : 1; g.d = h->enc[i].d;
    g.H = h->h[i].p; g.ldH = h->h[i].ld;
    g.eps_rows = h->eps_st[i].p; g.ld_eps = h->eps_st[i].ld;
    int n = 0;
    if (i == 0) { g.src[n] = h->dh_out[0].p; g.ldsrc[n++] = h->dh_out[0].ld; }
    if (i <= L - 2) {
      g.src[n] = h->dh_prior[i].p; g.ldsrc[n++] = h->dh_prior[i].ld;
      g.src[n] = h->dh_enc[i].p; g.ldsrc[n++] = h->dh_enc[i].ld;
    }
    if (i >= 1) { g.src[n] = h->dh_dec[i].p; g.ldsrc[n++] = h->dh_dec[i].ld; }
    if (P.path && i <= L - 2) { g.src[n] = h->dh_encq[i].p; g.ldsrc[n++] = h->dh_encq[i].ld; }
    g.nsrc = n;
    g.std_normal = i == L - 1;
    g.dlw = dlw;
    g.grad_mode = P.path ? GM_PATH : GM_TOTAL;
    if (P.path) h->count.path_gauss++;
    if (P.kl && i == L - 1) {
      g.kl_coef = 1.f;   // dLoss/dKL_mean for loss = -(E - KL)
      g.kl_rows = (L == 1) ? P.Bimg : M;
    }
    g.dP = h->eb[i].dP.p; g.lddP = h->eb[i].dP.ld;
    g.M = M;
    HIPCHK(launch_gauss_bwd(h->stream, 0, g));
    const Mat& in = i == 0 ? h->x_in : h->h[i - 1];
    const int rows = i == 0 ? P.Bimg : M;
    CHK(stoch_bwd(h, h->enc[i], in, rows, h->eb[i], true, i > 0 ? &h->dh_enc[i - 1] : nullptr));
    if (P.path && i > 0) {
      // q(h_i | h_{i-1}) depends on h_{i-1} through (mu, s) too: that is a path
      // of the layer below, so the density partials still send their dX down
      GaussBwdArgs q{};
      q.P = g.P; q.ldP = g.ldP; q.prow_div = 1; q.d = g.d;
      q.H = g.H; q.ldH = g.ldH; q.eps_rows = g.eps_rows; q.ld_eps = g.ld_eps;
      q.dlw = dlw;
      q.grad_mode = GM_DENSITY;
      q.dP = h->eb[i].dPq.p; q.lddP = h->eb[i].dPq.ld;
      q.M = M;
      HIPCHK(launch_gauss_bwd(h->stream, 0, q));
      h->count.path_gauss++;
      CHK(stoch_bwd_dx(h, h->enc[i], M, h->eb[i], h->dh_encq[i - 1]));
    }
  }
  return IWAE_OK;
}

// refresh the split (bf16 hi / lo) weight copies from the f32 parameters
static int run_wsplit(iwae_handle* h) {
  WSplitArgs a{};
  a.param = h->params; a.hi = h->wsplit_hi; a.lo = h->wsplit_lo;
  long long mx = 0;
  for (size_t i = 0; i < h->dense.size(); ++i) {
    const DenseL& d = h->dense[i];
    WSplitSeg& g = a.seg[i];
    g.off = d.off; g.fin = d.fin; g.fout = d.fout; g.ldw = d.ldw;
    g.f_off = d.f_off; g.g_off = d.g_off; g.ldF = d.ldF; g.ldG = d.ldG;
    mx = std::max(mx, (long long)(d.fin + 1) * d.fout);
  }
  a.nseg = (int)h->dense.size();
  HIPCHK(launch_wsplit(h->stream, a, mx));
  return IWAE_OK;
}

// refresh one Dense layer's split copy (the train step's output layer, on the
// step's stream, so a captured graph re-splits after every Adam update);
// the other layers' copies stay stale until ensure_wsplit
static int run_wsplit_seg(iwae_handle* h, int di) {
  WSplitArgs a{};
  a.param = h->params; a.hi = h->wsplit_hi; a.lo = h->wsplit_lo;
  const DenseL& d = h->dense[di];
  WSplitSeg& g = a.seg[0];
  g.off = d.off; g.fin = d.fin; g.fout = d.fout; g.ldw = d.ldw;
  g.f_off = d.f_off; g.g_off = d.g_off; g.ldF = d.ldF; g.ldG = d.ldG;
  a.nseg = 1;
  HIPCHK(launch_wsplit(h->stream, a, (long long)(d.fin + 1) * d.fout));
  h->wsplit_version = -1;
  return IWAE_OK;
}

static int ensure_wsplit(iwae_handle* h) {
  if (h->wsplit_version == h->params_version) return IWAE_OK;
  CHK(run_wsplit(h));
  h->wsplit_version = h->params_version;
  return IWAE_OK;
}

// refresh the fragment-major copies of every Dense layer but the input layer
// (the engine runs every other layer, the first encoder layer's l2 and head on
// image rows)
static int run_fx(iwae_handle* h) {
  FxArgs a{};
  a.param = h->params; a.hi = h->fx_hi; a.lo = h->fx_lo;
  long long tot = 0;
  for (size_t i = 0; i < h->dense.size(); ++i) {
    const DenseL& d = h->dense[i];
    if ((int)i == h->enc[0].l1) continue;      // the 785-wide input layer: few-row f32 path only
    FxSeg& g = a.seg[a.nseg++];
    g.off = d.off; g.fin = d.fin; g.fout = d.fout; g.ldw = d.ldw;
    g.fx_off = d.fx_off; g.fx_tiles = d.fx_tiles; g.fx_steps = d.fx_steps; g.head_d = d.head_d;
    g.gx_off = d.gx_off; g.gx_tiles = d.gx_tiles; g.gx_steps = d.gx_steps;
    g.start = tot;      // block aligned: a workgroup never straddles two segments
    tot += ((((long long)d.fx_tiles * d.fx_steps + (long long)d.gx_tiles * d.gx_steps) * 64 + 255) / 256) * 256;
  }
  a.total = tot;
  HIPCHK(launch_fx_refresh(h->stream, a));
  if (h->prof.kind == 14 && !h->prof.have) {
    h->prof.mem = [a](hipStream_t st) { return launch_fx_refresh(st, a); };
    double chunks = 0.0;                  // 8 parameters in, 8 bf16 per plane out
    for (int i = 0; i < a.nseg; ++i)
      chunks += ((double)a.seg[i].fx_tiles * a.seg[i].fx_steps + (double)a.seg[i].gx_tiles * a.seg[i].gx_steps) * 64;
    h->prof.flop1 = chunks * (8 * 4.0 + 2 * 16.0);
    h->prof.have = true;
  }
  return IWAE_OK;
}

static int ensure_fx(iwae_handle* h) {
  if (h->fx_version == h->params_version) return IWAE_OK;
  CHK(run_fx(h));
  h->fx_version = h->params_version;
  return IWAE_OK;
}

// Profiling replays (iwae_profile_replay) repeat a step's update on scratch
// copies, so the model is untouched: *base = prof.adam holds the parameters, m
// and v (n floats each, copied here on the step's stream) and extra_bytes behind
// them (the fragment-major copies: room only, the replayed launch rewrites them).
static int prof_state_copy(iwae_handle* h, size_t extra_bytes, float** base) {
  const size_t pb = (size_t)h->nparam_int * sizeof(float);
  if (h->prof.adam_bytes < 3 * pb + extra_bytes) {
    if (h->prof.adam) HIPCHK(hipFree(h->prof.adam));
    h->prof.adam = nullptr;
    HIPCHK(hipMalloc(&h->prof.adam, 3 * pb + extra_bytes));
    h->prof.adam_bytes = 3 * pb + extra_bytes;
  }
  HIPCHK(hipMemcpyAsync(h->prof.adam, h->params, pb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->prof.adam + h->nparam_int, h->adam_m, pb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->prof.adam + 2 * h->nparam_int, h->adam_v, pb, hipMemcpyDeviceToDevice, h->stream));
  *base = h->prof.adam;
  return IWAE_OK;
}
// (a replayed update launch's state: with the fragment-major copies)
static int prof_state_copy(iwae_handle* h, UpdArgs& r) {
  float* s = nullptr;
  CHK(prof_state_copy(h, (size_t)h->fx_elems * 2 * sizeof(__bf16), &s));
  r.param = s; r.m = s + h->nparam_int; r.v = s + 2 * h->nparam_int;
  r.fx_hi = reinterpret_cast<__bf16*>(s + 3 * h->nparam_int); r.fx_lo = r.fx_hi + h->fx_elems;
  return IWAE_OK;
}

struct AdamMode {   // what one adam_kernel launch does
  bool read_slabs = false;           // sum the weight-gradient slabs (DenseL::splits of them) into the gradient buffer first
  bool do_adam = false;              // then step Adam (else the gradient buffer is all it writes)
  float scale = 1.f;                 // gradient scale (0: AdamState's) ...
  const float* scale_dev = nullptr;  // ... or 1 / *scale_dev (data parallel: the all-reduced batch total)
  float* tail = nullptr;             // data parallel: *tail = scale (this rank's batch size)
  bool tick = false;                 // advance the Adam step count first (inside a train step the bound launch has)
  // the end of a step: the slabs summed into the gradient buffer, then (adam) the update
  static AdamMode from_slabs(bool adam) { return {true, adam}; }
  // data parallel: the slabs summed into b_local * g, b_local into the buffer's tail
  static AdamMode weighted_slab_sum(float b_local, float* tail) { return {true, false, b_local, nullptr, tail}; }
  // the update from the gradient buffer times scale, or times 1 / *total (data parallel: the summed buffer's tail)
  static AdamMode from_grad(float scale) { return {false, true, scale}; }
  static AdamMode from_grad_over(const float* total) { return {false, true, 0.f, total}; }
  // a call of its own (iwae_apply_adam): no bound launch has advanced the step count
  AdamMode own_tick() const { return {read_slabs, do_adam, scale, scale_dev, tail, true}; }
};

static int run_adam(iwae_handle* h, const AdamMode& mode) {
  const bool read_slabs = mode.read_slabs, do_adam = mode.do_adam;
  AdamArgs a{};
  a.scale_dev = mode.scale_dev; a.tail = mode.tail; a.tail_val = mode.scale;
  a.param = h->params; a.m = h->adam_m; a.v = h->adam_v; a.grad = h->grad; a.slabs = h->slabs;
  // the engine reads the split copies: its steps rewrite them with every update,
  // other paths refresh them lazily (ensure_wsplit)
  const bool splits = do_adam && h->adam_splits;
  a.whi = splits ? h->wsplit_hi : nullptr; a.wlo = splits ? h->wsplit_lo : nullptr;
  if (do_adam) h->params_version++;
  if (splits) h->wsplit_version = h->params_version;
  long long mx = 0;
  for (size_t i = 0; i < h->dense.size(); ++i) {
    const DenseL& d = h->dense[i];
    a.seg[i].off = d.off; a.seg[i].n = d.size(); a.seg[i].slab_off = d.slab_off;
    a.seg[i].splits = read_slabs ? d.splits : 0;
    a.seg[i].fin = d.fin; a.seg[i].fout = d.fout; a.seg[i].ldw = d.ldw;
    a.seg[i].f_off = d.f_off; a.seg[i].g_off = d.g_off; a.seg[i].ldF = d.ldF; a.seg[i].ldG = d.ldG;
    mx = std::max(mx, d.size());
  }
  a.nseg = (int)h->dense.size();
  a.write_grad = true; a.do_adam = do_adam; a.read_slabs = read_slabs;
  a.state = &h->ds->adam; a.ticket = &h->ds->tickets[2];
  a.grad_scale_override = mode.scale; a.tick = mode.tick;
  HIPCHK(launch_adam(h->stream, a, mx));
  if (h->prof.kind == 12 && do_adam && !h->prof.have) {
    AdamArgs r = a;
    r.tick = false;                  // replays repeat this step's update (same t)
    // ... on scratch copies of the parameters and moments: the model is untouched
    float* s = nullptr;
    CHK(prof_state_copy(h, 0, &s));
    r.param = s; r.m = s + h->nparam_int; r.v = s + 2 * h->nparam_int;
    // (the gradient buffer is rewritten with the same values)
    h->prof.mem = [r, mx](hipStream_t st) { return launch_adam(st, r, mx); };
    double bytes = 0.0;
    for (int i = 0; i < a.nseg; ++i)      // p, m, v in; p, m, v, g out; the slabs in
      bytes += (double)a.seg[i].n * 4.0 * (7 + (read_slabs ? a.seg[i].splits : 1));
    h->prof.flop1 = bytes;
    h->prof.have = true;
  }
  return IWAE_OK;
}

static int copy_x(iwae_handle* h, const Plan& P, const float* x) {
  const size_t wbytes = (size_t)h->xdim * sizeof(float);
  HIPCHK(hipMemcpy2DAsync(h->x_in.p, (size_t)h->x_in.ld * sizeof(float), x, wbytes, wbytes, P.B,
                          hipMemcpyDeviceToDevice, h->stream));
  if (P.Bimg != P.B) {
    HIPCHK(hipMemcpy2DAsync(h->x_in.p + (size_t)P.B * h->x_in.ld, (size_t)h->x_in.ld * sizeof(float), x,
                            wbytes, wbytes, P.B, hipMemcpyDeviceToDevice, h->stream));
  }
  return IWAE_OK;
}

// copy_x of a pixel-masked call (mask [B][x_dim], non-zero = observed), by
// select: x_in = mask ? x : 0 for every reader of the image (first encoder
// layer, its backward and weight gradient), x_lik = mask ? x : -1 for the
// masked Bernoulli epilogue.  One launch per copy of the batch (CIWAE: two).
static int stage_masked(iwae_handle* h, const Plan& P, const float* x, const float* mask) {
  for (int r0 = 0; r0 < P.Bimg; r0 += P.B)
    HIPCHK(launch_impute_stage(h->stream, x, mask, P.B, h->xdim, h->x_in.p + (size_t)r0 * h->x_in.ld, h->x_in.ld,
                               h->x_lik.p + (size_t)r0 * h->x_lik.ld, h->x_lik.ld));
  return IWAE_OK;
}

// pixel-masked entry points: the checks they share
static int check_masked(iwae_handle* h, const float* mask) {
  if (!mask) return fail(h, IWAE_EINVAL, "mask is NULL");
  if (h->dp_world > 1)
    return fail(h, IWAE_EINVAL, "pixel-masked steps and bounds are not built for data parallelism (world > 1)");
  return IWAE_OK;
}

// The node the capture on the handle's stream enqueued last (null unless it
// is exactly one): the launch or copy just issued, kept to re-point on replay.
static int last_captured_node(iwae_handle* h, hipGraphNode_t* node) {
  hipStreamCaptureStatus cs;
  unsigned long long cid;
  hipGraph_t cg;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  HIPCHK(hipStreamGetCaptureInfo_v2(h->stream, &cs, &cid, &cg, &deps, &nd));
  *node = nd == 1 ? deps[0] : nullptr;
  return IWAE_OK;
}

// ------------------------------------------------------- fused row-block path
constexpr int kRbMaxWidth = 512;   // widest LDS row the row-block kernels accept

static int rb_width_ok(const iwae_handle* h) {
  for (const auto& d : h->dense) {
    if (&d == &h->dense[h->enc[0].l1] || &d == &h->dense[h->o3]) continue;   // run as GEMMs
    if (d.fin + 1 > kRbMaxWidth || d.fout + 1 > kRbMaxWidth) return 0;
  }
  return 1;
}

static bool use_fused(const iwae_handle* h, const Plan& P) {
  if (h->path == 1 || h->L > kRbMaxJobs || h->masked) return false;
  if (!rb_width_ok(h)) return false;
  if (h->path == 2) return true;
  return (long long)P.Bimg * P.kS <= 65536;
}

// LDS image row stride: the widest padded operand of any stage, + 4 floats
// (rows then start 4 banks apart: the 16x4 MFMA A-fragment reads and the
// epilogue writes are bank-conflict free)
static int rb_ld(const iwae_handle* h, bool bwd) {
  int w = 0;
  for (const auto& d : h->dense) {
    const bool first = &d == &h->dense[h->enc[0].l1], out = &d == &h->dense[h->o3];
    if (!first) w = std::max(w, d.fin + 1);
    if (!out) w = std::max(w, d.fout + 1);
  }
  // (the backward stages pad to 64 at least, the forward ones to 32: a model
  // whose every width is below 32 needs the wider backward row, else the
  // padding of one LDS row lands in the next)
  return rb_k_pad(std::min(w, kRbMaxWidth), bwd) + 4;
}

// every row-block forward launch goes through here (iwae_debug_count id 13)
static int run_rb_fwd(iwae_handle* h, RbFwdLaunch& Lf) {
  HIPCHK(launch_rb_fwd(h->stream, Lf));
  h->count.rb_fwd++;
  return IWAE_OK;
}

static RbStage rb_fwd_stage(iwae_handle* h, int di, int act, Mat* out) {
  const DenseL& d = h->dense[di];
  RbStage s{};
  s.W = h->params + d.off; s.ldw = d.ldw; s.K = d.fin + 1; s.N = d.fout; s.act = act;
  s.W_bytes = (unsigned)(h->params_bytes - (size_t)d.off * sizeof(float));
  if (out) { s.out_g = out->p; s.ld_out = out->ld; }
  return s;
}

static RbStage rb_bwd_stage(iwae_handle* h, int di, const Mat* y, Mat* out) {
  const DenseL& d = h->dense[di];
  RbStage s{};
  s.W = h->params + d.off; s.ldw = d.ldw; s.K = d.fout; s.N = d.fin; s.act = y ? 2 : 0;
  s.W_bytes = (unsigned)(h->params_bytes - (size_t)d.off * sizeof(float));
  if (y) { s.y = y->p; s.ldy = y->ld; }
  if (out) { s.out_g = out->p; s.ld_out = out->ld; }
  return s;
}

static RbNoise rb_noise(iwae_handle* h, const Plan& P, const EpsSet& E, int layer) {
  RbNoise n{};
  n.eps_a = E.a[layer]; n.eps_b = E.b[layer];
  n.kS = P.kS; n.Bsplit = P.Bsplit; n.Bimg = P.Bimg;
  n.seed = h->seed; n.layer = layer;
  return n;
}

// few-row Dense layer (per-image first encoder layer of a small batch)
static SmArgs smallm_args(iwae_handle* h, const Mat& A, int rows, const DenseL& d, bool bwd, int act, const Mat* Y,
                          Mat& C) {
  SmArgs a{};
  a.A = A.p; a.lda = A.ld;
  a.W = h->params + d.off; a.ldw = d.ldw; a.bt = bwd ? 1 : 0;
  a.C = C.p; a.ldc = C.ld;
  a.M = rows; a.N = bwd ? d.fin : d.fout; a.K = bwd ? d.fout : d.fin + 1;
  a.act = act;
  if (Y) { a.Y = Y->p; a.ldy = Y->ld; }
  return a;
}
static int smallm(iwae_handle* h, const Mat& A, int rows, const DenseL& d, bool bwd, int act, const Mat* Y, Mat& C) {
  HIPCHK(launch_smallm(h->stream, smallm_args(h, A, rows, d, bwd, act, Y, C)));
  return IWAE_OK;
}
static bool smallm_ok(const iwae_handle* h, int rows) {
  if (rows > std::min(h->tune.smallm_rows, 32)) return false;      // (0: never the few-row launches)
  for (int di : {h->enc[0].l1, h->enc[0].l2, h->enc[0].head})
    if (h->dense[di].fin + 1 > 1024 || h->dense[di].fout > 1024) return false;
  return true;
}

// Number of partial slabs the first encoder Dense writes into fslab when only
// that launch runs (enc0_forward(l1_only), the train engine's image-row job
// sums them).
// The split-K GEMM's k chunk (a multiple of 64): at most fslab_S slabs, and
// no more than one round of the chip needs (64 x 64 tiles x slabs <= 256
// workgroups).  B = 512: 7 slabs of 128 in 224 workgroups instead of 13 of 64
// in 416 -- the GEMM 13.2 -> 9.9 us, job I's slab sum 26.0 -> 24.8 us
// (profiles/r06g_input_gemm_slabs_ab.txt); the NLL chunks (<= 256 images) keep 13.
static long long enc0_kchunk(const iwae_handle* h, int Bimg) {
  const DenseL& d1 = h->dense[h->enc[0].l1];
  const long long K = d1.fin + 1, tiles = cdiv(d1.fout, 64) * cdiv(Bimg, 64);
  const long long S = std::max(1LL, std::min<long long>(h->fslab_S, 256 / std::max(1LL, tiles)));
  return cdiv(cdiv(K, S), 64) * 64;
}
static int enc0_nslab(const iwae_handle* h, int Bimg) {
  const DenseL& d1 = h->dense[h->enc[0].l1];
  if (smallm_ok(h, Bimg)) return (int)std::min<long long>(std::min(4, h->fslab_S), cdiv(d1.fin + 1, 128));
  return (int)cdiv(d1.fin + 1, enc0_kchunk(h, Bimg));
}

// First encoder layer on the images (Stochastic_layer 0, F:58): y1, y2 and
// its head (mu | zs) P0, per image.  l1_only: just the input Dense, as
// pre-activation partial slabs in fslab (enc0_nslab of them).
static int enc0_forward(iwae_handle* h, const Plan& P, bool l1_only = false) {
  if (smallm_ok(h, P.Bimg)) {
    // (1') first encoder layer on the images: three N-split few-row launches
    const StochL& S0 = h->enc[0];
    const DenseL& d1 = h->dense[S0.l1];
    const int ksl = (int)std::min<long long>(std::min(4, h->fslab_S), cdiv(d1.fin + 1, 128));
    // input layer: from the caller's x when given (it also fills x_in for the
    // later readers: Bernoulli epilogue, weight gradient), else from x_in
    SmArgs a{};
    if (h->step.x_user) {
      a.A = h->step.x_user; a.lda = h->xdim;
      a.a_ones = h->xdim; a.a_bytes = (unsigned)((size_t)P.Bimg * h->xdim * sizeof(float));
      a.a_copy = h->x_in.p; a.a_copy_ld = h->x_in.ld;
    } else {
      a.A = h->x_in.p; a.lda = h->x_in.ld;
    }
    a.W = h->params + d1.off; a.ldw = d1.ldw;
    a.M = P.Bimg; a.N = d1.fout; a.K = d1.fin + 1;
    if (ksl > 1 || l1_only) {
      // the wide input layer split over K into partial slabs (more workgroups);
      // the second layer sums them, applies tanh and stores y1 while staging
      a.C = h->fslab; a.ldc = h->eb[0].y1.ld;
      a.kslabs = ksl; a.c_slab = (long long)P.Bimg * a.ldc;
    } else {
      a.C = h->eb[0].y1.p; a.ldc = h->eb[0].y1.ld;
      a.act = 1;
    }
    HIPCHK(launch_smallm(h->stream, a));
    if (h->step.capturing && h->step.x_user) {
      // remember the launch that reads x: replays re-point it at the caller's next x
      CHK(last_captured_node(h, &h->step.cap_x_node));
      h->step.cap_x_args.kind = 0;
      h->step.cap_x_args.sm = a;
    }
    if (l1_only) return IWAE_OK;
    const DenseL& d2 = h->dense[S0.l2];
    SmArgs b{};
    if (ksl > 1) {
      b.A = h->fslab; b.lda = a.ldc;
      b.a_slabs = ksl; b.a_slab = a.c_slab; b.a_act = 1; b.a_out = h->eb[0].y1.p; b.a_ldo = h->eb[0].y1.ld;
      b.W = h->params + d2.off; b.ldw = d2.ldw;
      b.C = h->eb[0].y2.p; b.ldc = h->eb[0].y2.ld;
      b.M = P.Bimg; b.N = d2.fout; b.K = d2.fin + 1;
      b.act = 1;
    } else {
      b = smallm_args(h, h->eb[0].y1, P.Bimg, d2, false, 1, nullptr, h->eb[0].y2);
    }
    const SmArgs hd = smallm_args(h, h->eb[0].y2, P.Bimg, h->dense[S0.head], false, 0, nullptr, h->eb[0].P);
    HIPCHK(launch_smallm(h->stream, b));
    HIPCHK(launch_smallm(h->stream, hd));
  } else
  // (1) first encoder Dense (K = 785) as a split-K GEMM into partial slabs
  {
    const DenseL& d = h->dense[h->enc[0].l1];
    GemmArgs a{};
    a.x3 = h->step.in_train_step ? 0 : h->x3;
    a.A = h->x_in.p; a.lda = h->x_in.ld;
    a.B = h->params + d.off; a.ldb = d.ldw;
    a.C = h->fslab; a.ldc = h->eb[0].y1.ld;
    a.M = P.Bimg; a.N = d.fout; a.K = d.fin + 1;
    if (use_split_b(h)) { a.Bhi = h->wsplit_hi + d.f_off; a.Blo = h->wsplit_lo + d.f_off; a.ldbx = d.ldF; }
    a.kchunk = (int)enc0_kchunk(h, P.Bimg);
    const int S = (int)cdiv(a.K, a.kchunk);
    a.c_split_stride = (long long)P.Bimg * a.ldc;
    if (h->step.x_user) {
      // the caller's x with a virtual ones column; the column-0 workgroups
      // fill x_in for the later readers (ring forward pixels, weight gradients)
      a.A = h->step.x_user; a.lda = h->xdim;
      a.a_ones = h->xdim; a.a_copy = h->x_in.p; a.a_copy_ld = h->x_in.ld;
    }
    CHK(prof_begin(h, GEMM_FWD, EPI_STORE, 2.0 * P.Bimg * d.fout * d.fin));
    HIPCHK(launch_gemm(h->stream, GEMM_FWD, EPI_STORE, 0, S, false, a));
    CHK(prof_end(h, GEMM_FWD, EPI_STORE));
    if (h->step.capturing && h->step.x_user) {
      CHK(last_captured_node(h, &h->step.cap_x_node));
      h->step.cap_x_args.kind = 1;
      h->step.cap_x_args.gm = a;
    }
    if (l1_only) return IWAE_OK;
    // (2) rest of encoder layer 0 on the images: tanh(sum) -> l2 -> head (P0)
    RbFwdLaunch Lf{};
    Lf.ld_lds = rb_ld(h, false);
    Lf.rng_base = &h->ds->rng[0];
    RbFwdJob& J = Lf.job[0];
    J.rows = P.Bimg; J.rpb = 4;
    J.pr_slabs = h->fslab; J.pr_nslab = S; J.pr_ld = a.ldc; J.pr_H = d.fout; J.pr_stride = a.c_split_stride;
    J.pr_y = h->eb[0].y1.p; J.pr_ldy = h->eb[0].y1.ld;
    J.nst = 2;
    J.st[0] = rb_fwd_stage(h, h->enc[0].l2, 1, &h->eb[0].y2);
    J.st[1] = rb_fwd_stage(h, h->enc[0].head, 0, &h->eb[0].P);
    Lf.njobs = 1;
    CHK(run_rb_fwd(h, Lf));
  }
  return IWAE_OK;
}

static int fused_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool train) {
  const int L = h->L, kS = P.kS, M = P.Bimg * kS;
  CHK(enc0_forward(h, P));
  // (3) encoder layers 1..L-1 (layer 1 samples h1 from P0 in its prologue)
  for (int i = 1; i < L; ++i) {
    RbFwdLaunch Lf{};
    Lf.ld_lds = rb_ld(h, false);
    Lf.rng_base = &h->ds->rng[0];
    RbFwdJob& J = Lf.job[0];
    J.rows = M; J.rpb = 16;
    if (i == 1) {
      J.pro_sample = 1;
      J.ps_P = h->eb[0].P.p; J.ps_ldP = h->eb[0].P.ld; J.ps_div = kS; J.ps_d = h->enc[0].d;
      J.ps_h = h->h[0].p; J.ps_ldh = h->h[0].ld;
      J.ps_eps = train ? h->eps_st[0].p : nullptr; J.ps_ldeps = train ? h->eps_st[0].ld : 0;
      J.ps_noise = rb_noise(h, P, E, 0);
    } else {
      J.in = h->h[i - 1].p; J.ld_in = h->h[i - 1].ld;
      J.logq_acc = 1;
    }
    const StochL& S = h->enc[i];
    J.nst = 3;
    J.st[0] = rb_fwd_stage(h, S.l1, 1, &h->eb[i].y1);
    J.st[1] = rb_fwd_stage(h, S.l2, 1, &h->eb[i].y2);
    J.st[2] = rb_fwd_stage(h, S.head, 0, &h->eb[i].P);
    J.epi = 1; J.ep_d = S.d; J.ep_noise = rb_noise(h, P, E, i);
    J.ep_h = h->h[i].p; J.ep_ldh = h->h[i].ld;
    J.ep_eps = train ? h->eps_st[i].p : nullptr; J.ep_ldeps = train ? h->eps_st[i].ld : 0;
    J.logq = h->logq;
    Lf.njobs = 1;
    CHK(run_rb_fwd(h, Lf));
  }
  // (4) decoder prior layers and the output MLP's two hidden layers
  {
    RbFwdLaunch Lf{};
    Lf.ld_lds = rb_ld(h, false);
    Lf.rng_base = &h->ds->rng[0];
    int nj = 0;
    if (L >= 2) {
      RbFwdJob& J = Lf.job[nj++];
      J.rows = M; J.rpb = 16;
      J.in = h->h[L - 1].p; J.ld_in = h->h[L - 1].ld;
      J.pro_stdnormal = 1;                                   // log N(h_L; 0, 1)
      const StochL& S = h->dec[0];
      J.nst = 3;
      J.st[0] = rb_fwd_stage(h, S.l1, 1, &h->db[0].y1);
      J.st[1] = rb_fwd_stage(h, S.l2, 1, &h->db[0].y2);
      J.st[2] = rb_fwd_stage(h, S.head, 0, &h->db[0].P);
      J.epi = 2; J.ep_d = S.d; J.ep_tgt = h->h[L - 2].p; J.ep_ldtgt = h->h[L - 2].ld;
      J.logp = h->logp;
    }
    {
      RbFwdJob& J = Lf.job[nj++];
      J.rows = M; J.rpb = 16;
      if (L == 1) {
        J.pro_sample = 1;
        J.ps_P = h->eb[0].P.p; J.ps_ldP = h->eb[0].P.ld; J.ps_div = kS; J.ps_d = h->enc[0].d;
        J.ps_h = h->h[0].p; J.ps_ldh = h->h[0].ld;
        J.ps_eps = train ? h->eps_st[0].p : nullptr; J.ps_ldeps = train ? h->eps_st[0].ld : 0;
        J.ps_noise = rb_noise(h, P, E, 0);
        J.pro_stdnormal = 1;
        J.logq = h->logq; J.logp = h->logp;
      } else {
        J.in = h->h[0].p; J.ld_in = h->h[0].ld;
      }
      J.nst = 2;
      J.st[0] = rb_fwd_stage(h, h->o1, 1, &h->ob.y1);
      J.st[1] = rb_fwd_stage(h, h->o2, 1, &h->ob.y2);
    }
    Lf.njobs = nj;
    CHK(run_rb_fwd(h, Lf));
  }
  // deeper decoder layers (L >= 3) accumulate into log p one launch at a time
  for (int i = 1; i < L - 1; ++i) {
    RbFwdLaunch Lf{};
    Lf.ld_lds = rb_ld(h, false);
    RbFwdJob& J = Lf.job[0];
    J.rows = M; J.rpb = 16;
    J.in = h->h[L - 1 - i].p; J.ld_in = h->h[L - 1 - i].ld;
    const StochL& S = h->dec[i];
    J.nst = 3;
    J.st[0] = rb_fwd_stage(h, S.l1, 1, &h->db[i].y1);
    J.st[1] = rb_fwd_stage(h, S.l2, 1, &h->db[i].y2);
    J.st[2] = rb_fwd_stage(h, S.head, 0, &h->db[i].P);
    J.epi = 2; J.ep_d = S.d; J.ep_tgt = h->h[L - 2 - i].p; J.ep_ldtgt = h->h[L - 2 - i].ld;
    J.logp = h->logp; J.logp_acc = 1;
    Lf.njobs = 1;
    CHK(run_rb_fwd(h, Lf));
  }
  // (5) output layer 200 -> 784 with the fused Bernoulli epilogue
  {
    GemmArgs ex{};
    // (a pixel-masked call: the -1 copy and the epilogue that selects by it)
    const Mat& xl = P.pix ? h->x_lik : h->x_in;
    ex.aux = xl.p; ex.ldaux = xl.ld; ex.x_row_div = kS;
    ex.part = h->part; ex.part2 = h->part2; ex.ldpart = h->ldpart;
    ex.wa = P.wa; ex.wb = P.wb;
    ex.store_g = train ? 1 : 0;
    ex.need_bce = P.need_bce;
    Mat gm = h->ob.P;
    if (!train) { gm.p = nullptr; gm.ld = 0; }
    CHK(gemm_fwd(h, P.pix ? EPI_BERN_MASK : EPI_BERN, h->ob.y2, M, h->dense[h->o3], gm, ex));
    if (P.pix) h->count.bern_mask++;
  }
  return IWAE_OK;
}

// decoder backward: output MLP + prior layers (which: 1 = weights' dZ only, 2 = dh only, 3 = both)
static int fused_decoder_bwd(iwae_handle* h, const Plan& P, const float* dlw, const float* dpx, bool need_dh) {
  const int L = h->L, M = P.Bimg * P.kS;
  if (L > kRbMaxJobs) return fail(h, IWAE_EINVAL, "fused path supports up to 4 stochastic layers");
  // output layer dX = (dpx * g) W3^T (1 - y2^2), split over K = 784 into slabs
  // that the row-block prologue sums (the epilogue is linear: applied per slab)
  int oS = 1;
  {
    const DenseL& d = h->dense[h->o3];
    GemmArgs a{};
    a.x3 = split_b_for(h, d) ? 1 : 0;
    a.A = h->ob.P.p; a.lda = h->ob.P.ld;
    a.B = h->params + d.off; a.ldb = d.ldw;
    a.M = M; a.N = d.fin; a.K = d.fout;
    a.rowscale = dpx; a.aux = h->ob.y2.p; a.ldaux = h->ob.y2.ld;
    if (split_b_for(h, d)) { a.Bhi = h->wsplit_hi + d.g_off; a.Blo = h->wsplit_lo + d.g_off; a.ldbx = d.ldG; }
    const long long tiles = cdiv(M, 64) * cdiv(d.fin, 64);
    if (h->oslab && h->oslab_S > 1 && tiles < 256) {
      oS = (int)std::min<long long>(h->oslab_S, cdiv(256, tiles));
      a.kchunk = (int)(cdiv(cdiv(a.K, oS), 64) * 64);
      oS = (int)cdiv(a.K, a.kchunk);
    }
    if (oS > 1) {
      a.C = h->oslab; a.ldc = h->ob.dY2.ld;
      a.c_split_stride = (long long)M * a.ldc;
    } else {
      a.kchunk = a.K;
      a.C = h->ob.dY2.p; a.ldc = h->ob.dY2.ld;
    }
    CHK(prof_begin(h, GEMM_BWD_DATA, EPI_TANH_GRAD, 2.0 * M * d.fout * d.fin));
    // large batches: 128x128 tiles (B=512, k=50: 1.132 vs 1.158 ms per step)
    const int tile = (oS == 1 && M >= 8192) ? 1 : 0;
    HIPCHK(launch_gemm(h->stream, GEMM_BWD_DATA, EPI_TANH_GRAD, tile, oS, false, a));
    CHK(prof_end(h, GEMM_BWD_DATA, EPI_TANH_GRAD));
  }
  RbBwdLaunch Lb{};
  Lb.ld_lds = rb_ld(h, true);
  int nj = 0;
  {
    RbBwdJob& J = Lb.job[nj++];
    J.rows = M; J.rpb = 16; J.pro = 0;
    if (oS > 1) {
      J.dz_in = h->oslab; J.ld_dz_in = h->ob.dY2.ld; J.dz_nslab = oS; J.dz_stride = (long long)M * h->ob.dY2.ld;
      J.dz_out = h->ob.dY2.p;
    } else {
      J.dz_in = h->ob.dY2.p; J.ld_dz_in = h->ob.dY2.ld; J.dz_nslab = 1;
    }
    J.nst = need_dh ? 2 : 1;
    J.st[0] = rb_bwd_stage(h, h->o2, &h->ob.y1, &h->ob.dY1);
    if (need_dh) J.st[1] = rb_bwd_stage(h, h->o1, nullptr, &h->dh_out[0]);
  }
  for (int i = 0; i < L - 1 && nj < kRbMaxJobs; ++i) {
    const int t = L - 2 - i, src = L - 1 - i;
    const StochL& S = h->dec[i];
    RbBwdJob& J = Lb.job[nj++];
    J.rows = M; J.rpb = 16; J.pro = 2;
    J.P = h->db[i].P.p; J.ldP = h->db[i].P.ld; J.d = S.d;
    J.H = h->h[t].p; J.ldH = h->h[t].ld; J.dlw = dlw;
    J.dP_out = h->db[i].dP.p; J.ld_dP = h->db[i].dP.ld;
    J.dh_out = h->dh_prior[t].p; J.ld_dh = h->dh_prior[t].ld;
    J.nst = need_dh ? 3 : 2;
    J.st[0] = rb_bwd_stage(h, S.head, &h->db[i].y2, &h->db[i].dY2);
    J.st[1] = rb_bwd_stage(h, S.l2, &h->db[i].y1, &h->db[i].dY1);
    if (need_dh) J.st[2] = rb_bwd_stage(h, S.l1, nullptr, &h->dh_dec[src]);
  }
  Lb.njobs = nj;
  HIPCHK(launch_rb_bwd(h->stream, Lb));
  return IWAE_OK;
}

// encoder backward, layers top .. 0 (top < 0: all)
static int fused_encoder_bwd(iwae_handle* h, const Plan& P, const float* dlw, int top = -1) {
  const int L = h->L, kS = P.kS, M = P.Bimg * kS;
  for (int i = top < 0 ? L - 1 : top; i >= 0; --i) {
    const StochL& S = h->enc[i];
    RbBwdLaunch Lb{};
    Lb.ld_lds = rb_ld(h, true);
    RbBwdJob& J = Lb.job[0];
    J.pro = i == 0 ? 3 : 1;
    J.rows = i == 0 ? P.Bimg : M;
    J.rpb = i == 0 ? 1 : 16;
    J.kS = kS;
    J.P = h->eb[i].P.p; J.ldP = h->eb[i].P.ld; J.d = S.d;
    J.H = h->h[i].p; J.ldH = h->h[i].ld;
    J.eps = h->eps_st[i].p; J.ld_eps = h->eps_st[i].ld;
    J.dlw = dlw;
    int n = 0;
    if (i == 0) { J.src[n] = h->dh_out[0].p; J.ldsrc[n++] = h->dh_out[0].ld; }
    if (i <= L - 2) {
      J.src[n] = h->dh_prior[i].p; J.ldsrc[n++] = h->dh_prior[i].ld;
      J.src[n] = h->dh_enc[i].p; J.ldsrc[n++] = h->dh_enc[i].ld;
    }
    if (i >= 1) { J.src[n] = h->dh_dec[i].p; J.ldsrc[n++] = h->dh_dec[i].ld; }
    if (P.path && i <= L - 2) { J.src[n] = h->dh_encq[i].p; J.ldsrc[n++] = h->dh_encq[i].ld; }
    J.nsrc = n;
    J.std_normal = i == L - 1;
    J.gmode = P.path ? GM_PATH : GM_TOTAL;
    if (P.kl && i == L - 1) { J.kl_coef = 1.f; J.kl_rows = (L == 1) ? P.Bimg : M; }
    J.dP_out = h->eb[i].dP.p; J.ld_dP = h->eb[i].dP.ld;
    const bool sm0 = i == 0 && smallm_ok(h, P.Bimg);
    J.nst = i == 0 ? (sm0 ? 0 : 2) : 3;
    if (!sm0) {
      J.st[0] = rb_bwd_stage(h, S.head, &h->eb[i].y2, &h->eb[i].dY2);
      J.st[1] = rb_bwd_stage(h, S.l2, &h->eb[i].y1, &h->eb[i].dY1);
    }
    if (i > 0) J.st[2] = rb_bwd_stage(h, S.l1, nullptr, &h->dh_enc[i - 1]);
    Lb.njobs = 1;
    if (P.path) h->count.path_rb++;
    if (P.path && i > 0) {
      // the density job, beside the path job: the layer's density partials
      // through the same three transposed layers, storing only the final dX
      // (dh_encq[i - 1]) -- dP / dY2 / dY1 stay the path job's (weight_grads)
      RbBwdJob& Q = Lb.job[1];
      Q.pro = 1; Q.rows = M; Q.rpb = 16; Q.kS = kS;
      Q.P = J.P; Q.ldP = J.ldP; Q.d = J.d;
      Q.H = J.H; Q.ldH = J.ldH; Q.eps = J.eps; Q.ld_eps = J.ld_eps;
      Q.dlw = dlw;
      Q.gmode = GM_DENSITY;
      Q.nst = 3;
      Q.st[0] = rb_bwd_stage(h, S.head, &h->eb[i].y2, nullptr);
      Q.st[1] = rb_bwd_stage(h, S.l2, &h->eb[i].y1, nullptr);
      Q.st[2] = rb_bwd_stage(h, S.l1, nullptr, &h->dh_encq[i - 1]);
      Lb.njobs = 2;
      h->count.path_rb++;
    }
    HIPCHK(launch_rb_bwd(h->stream, Lb));
    if (sm0) {
      // first encoder layer's head and l2 backward as N-split few-row launches
      CHK(smallm(h, h->eb[0].dP, P.Bimg, h->dense[S.head], true, 2, &h->eb[0].y2, h->eb[0].dY2));
      CHK(smallm(h, h->eb[0].dY2, P.Bimg, h->dense[S.l2], true, 2, &h->eb[0].y1, h->eb[0].dY1));
    }
  }
  return IWAE_OK;
}

// One weight-gradient job of a train step: dW_aug of Dense layer di = A_aug^T (ks . dZ) over rows.
enum WGroup { WG_ENC0, WG_ENC, WG_DEC, WG_OUT };   // first encoder layer (image rows), encoder, decoder, output MLP
// sets of groups: the two passes of PIWAE's fused step; the data-parallel step's two all-reduce buckets
enum WGroups : unsigned {
  WG_ALL = 15, WG_ENCODER = 1u << WG_ENC0 | 1u << WG_ENC, WG_DECODER = 1u << WG_DEC | 1u << WG_OUT,
  WG_OUT_ONLY = 1u << WG_OUT, WG_BUT_OUT = WG_ALL & ~WG_OUT_ONLY,
};
struct WJob { int di; const Mat* A; const Mat* dZ; int rows; const float* ks; WGroup grp; };   // ks: dZ's row scale, or null

// The step's weight-gradient jobs in their natural order: the encoder layers
// ascending, the decoder layers ascending, the output MLP, each layer as l1,
// l2, head (three jobs).  Row scales: the output layer's dZ is g, scaled by
// dpx; under piwae_unit every layer's dZ takes its own weighting (see
// engine_train_body), but the first encoder layer's image-row dZ, weighted
// already.  The three consumers (weight_grads, run_update's slab pass, run_dw)
// each choose a layer's slab count and leave it in DenseL::splits, which the launch
// that sums the slabs reads: run_adam (read_slabs) or run_update's apply from the slabs.
static std::vector<WJob> layer_jobs(const iwae_handle* h, const Plan& P, WGroups groups = WG_ALL) {
  const int L = h->L, M = P.Bimg * P.kS;
  const float* const unit_ks[] = {nullptr, h->dlw2, h->dlw, h->dpx};      // piwae_unit's weighting by WGroup
  std::vector<WJob> js;
  auto layer = [&](const StochL& S, const Mat* in, const LayerBufs& b, int rows, WGroup grp) {
    if (!(groups >> grp & 1u)) return;
    const float* ks = h->step.piwae_ks ? unit_ks[grp] : nullptr;
    js.push_back({S.l1, in, &b.dY1, rows, ks, grp});
    js.push_back({S.l2, &b.y1, &b.dY2, rows, ks, grp});
    js.push_back({S.head, &b.y2, grp == WG_OUT ? &b.P : &b.dP, rows, grp == WG_OUT ? h->dpx : ks, grp});
  };
  layer(h->enc[0], &h->x_in, h->eb[0], P.Bimg, WG_ENC0);
  for (int i = 1; i < L; ++i) layer(h->enc[i], &h->h[i - 1], h->eb[i], M, WG_ENC);
  for (int i = 0; i < L - 1; ++i) layer(h->dec[i], &h->h[L - 1 - i], h->db[i], M, WG_DEC);
  layer({0, 0, 0, h->o1, h->o2, h->o3}, &h->h[0], h->ob, M, WG_OUT);      // the output MLP as one layer (head dZ: ob.P)
  return js;
}

// weight-gradient jobs (X_aug^T dZ, split over rows) in grouped launches
static int weight_grad_jobs(iwae_handle* h, const std::vector<WJob>& js) {
  for (size_t b = 0; b < js.size(); b += kMaxGroup) {
    GemmGroup gg{};
    for (size_t q = b; q < std::min(js.size(), b + kMaxGroup); ++q) {
      const WJob& w = js[q];
      DenseL& d = h->dense[w.di];
      gg.g[gg.n] = bwd_weight_args(h, *w.A, *w.dZ, w.rows, d, w.ks);
      gg.splits[gg.n++] = d.splits;
    }
    HIPCHK(launch_gemm_group_bwd_weight(h->stream, gg));
  }
  return IWAE_OK;
}

// ... of the groups' layers
static int weight_grads(iwae_handle* h, const Plan& P, WGroups groups) {
  return weight_grad_jobs(h, layer_jobs(h, P, groups));
}

// Fused update (iwae_update.hip): every weight gradient over all the step's rows,
// the gradient buffer, Adam and the FX / GX copies in one launch (data
// parallel: the gradient pass only, B_local-weighted, before the all-reduce),
// bf16x3 products, and up to upd_rows sample rows (one workgroup reduces a
// tile over all rows: beyond that the split-K GEMM + Adam launches parallelise
// better).
static bool upd_tiles_ok(const iwae_handle* h) {
  long long tiles = 0;
  for (const DenseL& d : h->dense) tiles += cdiv(d.fin + 1, 64) * cdiv(d.fout, 64);
  return tiles <= kUpdMaxTiles && (int)h->dense.size() <= kUpdMaxJobs;
}
static bool use_update(const iwae_handle* h, const Plan& P) {
  return h->tune.upd && h->x3 && (long long)P.Bimg * P.kS <= h->tune.upd_rows && upd_tiles_ok(h);
}

// slabs: larger batches (beyond upd_rows), the gradient pass only, split over
// rows into the split-K slabs the Adam launch sums (the weight-gradient GEMMs'
// role); about two workgroups per CU of sample-row tiles
static bool use_update_slabs(const iwae_handle* h, const Plan& P) {
  return h->tune.upd_slabs && h->x3 && h->slabs && (long long)P.Bimg * P.kS > h->tune.upd_rows &&
         (int)h->dense.size() <= kUpdMaxJobs;
}

struct UpdMode {   // what one launch of the update kernel does
  enum Kind { FUSED, DP_GRADS, SLAB_PASS, APPLY_GRAD, APPLY_SLABS } kind = FUSED;
  bool adam = false;                 // FUSED: step Adam and rewrite the FX / GX copies (else the gradients only)
  WGroups bucket = WG_ALL; hipStream_t st = nullptr;   // DP_GRADS: the layers of the pass, its stream (null: the step's)
  const float* total = nullptr;      // APPLY_GRAD: the all-reduced batch total
  // every weight gradient, the gradient buffer, (adam) Adam and the FX / GX copies
  static UpdMode fused(bool adam) { return {FUSED, adam}; }
  // data parallel before the all-reduce: B_local * g only, B_local into the tail with the bucket that holds it
  static UpdMode dp_grads(WGroups bucket, hipStream_t st) { return {DP_GRADS, false, bucket, st}; }
  static UpdMode slab_pass() { return {SLAB_PASS}; }      // (use_update_slabs) the gradient pass only, into the split-K slabs
  // data parallel after the all-reduce: no reduction, Adam + FX / GX from the summed buffer times 1 / *total
  static UpdMode apply_grad(const float* total) { return {APPLY_GRAD, false, WG_ALL, nullptr, total}; }
  // the slabs of a gradient pass summed (DenseL::splits of them), then Adam + FX / GX
  static UpdMode apply_slabs() { return {APPLY_SLABS}; }
};

static int run_update(iwae_handle* h, const Plan& P, const UpdMode& mode) {
  const hipStream_t st = mode.st ? mode.st : h->stream;
  const int M = P.Bimg * P.kS;
  const bool slabs = mode.kind == UpdMode::SLAB_PASS, from_slabs = mode.kind == UpdMode::APPLY_SLABS;
  const bool apply = mode.kind == UpdMode::APPLY_GRAD || from_slabs;
  std::vector<WJob> js = layer_jobs(h, P, mode.bucket);
  if ((int)js.size() > kUpdMaxJobs) return fail(h, IWAE_EINVAL, "fused update: too many layers");
  // the long reductions first (dispatched first)
  std::stable_sort(js.begin(), js.end(), [](const WJob& x, const WJob& y) { return x.rows > y.rows; });
  UpdArgs a{};
  int tiles = 0, nsplit = 1;
  double flop = 0.0;
  if (slabs) {
    long long st_tiles = 0;                      // sample-row tiles: nsplit of them per CU pair
    for (const WJob& w : js)
      if (w.rows == M) st_tiles += cdiv(h->dense[w.di].fin + 1, 64) * cdiv(h->dense[w.di].fout, 64);
    const long long target = h->tune.upd_slab_wg;     // sample-row workgroups of the pass
    nsplit = (int)std::max(1LL, (target + st_tiles / 2) / std::max(1LL, st_tiles));
  }
  for (const WJob& w : js) {
    DenseL& d = h->dense[w.di];
    UpdJob& J = a.job[a.njobs++];
    J.A = w.A->p; J.lda = w.A->ld; J.B = w.dZ->p; J.ldb = w.dZ->ld; J.ks = w.ks ? w.ks : h->ones; J.rows = w.rows;
    J.off = d.off; J.fin = d.fin; J.fout = d.fout; J.ldw = d.ldw;
    const bool fx = w.di != h->enc[0].l1;       // the input layer has no fragment-major copies
    J.fx_off = fx ? d.fx_off : -1; J.fx_steps = d.fx_steps; J.head_d = d.head_d;
    J.gx_off = d.gx_off; J.gx_steps = d.gx_steps;
    J.tn = 64;
    J.tiles_m = (int)cdiv(d.fin + 1, 64); J.tiles_n = (int)cdiv(d.fout, J.tn);
    J.tile0 = tiles;
    J.nsplit = 1;
    if (slabs) {
      // row chunks of whole reduction iterations (128 rows), at most the layer's slab count
      long long S = std::min<long long>(w.rows == M ? nsplit : 1, d.max_splits);
      const long long chunk = cdiv(cdiv(w.rows, S), kUpdRowsPerIter) * kUpdRowsPerIter;
      S = cdiv(w.rows, chunk);
      J.nsplit = (int)S; J.chunk = (int)chunk; J.slab_stride = d.size();
      J.off = d.slab_off; J.fx_off = -1; J.tn = 64;
      J.tiles_n = (int)cdiv(d.fout, 64);
      d.splits = (int)S;
    }
    if (from_slabs) {
      // apply from the gradient pass's slabs: B, chunk, slab_stride name them
      J.B = h->slabs + d.slab_off; J.chunk = d.splits; J.slab_stride = d.size();
    }
    tiles += J.tiles_m * J.tiles_n * J.nsplit;
    if (!slabs) {
      if (tiles > kUpdMaxTiles) return fail(h, IWAE_EINVAL, "fused update: too many tiles");
      for (int q = J.tile0; q < tiles; ++q) a.tile_job[q] = (unsigned char)(a.njobs - 1);
    }
    flop += 2.0 * w.rows * (d.fin + 1) * d.fout;
  }
  a.ntiles = tiles;
  int heavy = 0;                                // the jobs are sorted by rows: the sample-row jobs' tiles first
  for (int j = 0; j < a.njobs; ++j)
    if (a.job[j].rows == js[0].rows) heavy = a.job[j].tile0 + a.job[j].tiles_m * a.job[j].tiles_n * a.job[j].nsplit;
  a.nheavy = heavy;
  a.per_xcd = (int)cdiv(heavy, 8);
  a.per_xcd2 = (int)cdiv(tiles - heavy, 8);
  a.param = h->params; a.m = h->adam_m; a.v = h->adam_v; a.grad = h->grad;
  a.fx_hi = h->fx_hi; a.fx_lo = h->fx_lo;
  a.state = &h->ds->adam;
  a.gscale = a.tail_val = 1.f;
  switch (mode.kind) {
    case UpdMode::FUSED:
      a.do_adam = mode.adam ? 1 : 0;
      // store policy (bits 4, 8, 16 of the knob: heavy tiles, light tiles, the heavy tiles' release)
      a.st_wt = ((h->tune.st_wt & 4) ? kUpdStHeavy : 0) | ((h->tune.st_wt & 8) ? kUpdStLight : 0) |
                ((h->tune.st_wt & 16) ? kUpdStRelease : 0);
      break;
    case UpdMode::DP_GRADS:
      a.gscale = a.tail_val = (float)P.B;
      a.tail = (mode.bucket & WG_OUT_ONLY) ? h->grad + h->nparam_int : nullptr;
      break;
    case UpdMode::SLAB_PASS: a.search = 1; a.grad = h->slabs; break;
    case UpdMode::APPLY_GRAD: a.do_adam = 1; a.apply = 1; a.scale_dev = mode.total; break;
    case UpdMode::APPLY_SLABS: a.do_adam = 1; a.apply = 2; break;
  }
  a.waves = h->tune.upd_waves;
  h->count.upd++;
  if (h->step.defer_launch && st == h->stream && !slabs && !apply) {
    // recorded for a combined launch (tcu_kernel) with job I': the first
    // encoder layer's jobs are the ones that wait for it
    h->pend.upd = a; h->pend.upd_have = true;
    h->pend.upd_mask = 0; h->pend.upd_cons = 0;
    for (int j = 0; j < a.njobs; ++j) {
      if (js[j].grp == WG_ENC0) {
        h->pend.upd_mask |= 1u << j;
        h->pend.upd_cons += a.job[j].tiles_m * a.job[j].tiles_n;
      }
    }
  } else {
    HIPCHK(launch_update(st, a));
  }
  if (a.do_adam) h->params_version++;
  if (h->prof.kind == 15 && a.do_adam && !h->prof.have) {
    // replays repeat this step's update on scratch copies of the parameters,
    // moments and fragment-major copies: the model is untouched
    UpdArgs r = a;
    CHK(prof_state_copy(h, r));
    h->prof.mem = [r](hipStream_t st) { return launch_update(st, r); };
    h->prof.flop1 = flop;
    h->prof.have = true;
  }
  return IWAE_OK;
}

// Large-batch weight gradients (iwae_dwgrad.hip): every layer's X_aug^T dZ in
// blocks of up to 208 x 128 (13 x 8 MFMA tiles) split over row chunks into the
// slabs adam_kernel sums.  Blocks of one layer are as even as the tile counts
// allow; row chunks are sized so every workgroup has about the same MFMA work
// (about one workgroup per CU: 96 KiB of LDS each), at most cap_splits slabs per
// layer; work items are ordered chunk-major so one row chunk's blocks share an
// XCD (and its L2).
static int run_dw(iwae_handle* h, const Plan& P) {
  const int L = h->L;
  // the output MLP first, then the decoder layers ascending, then the encoder
  // layers descending, each layer as head, l2, l1
  const std::vector<WJob> nat = layer_jobs(h, P);
  std::vector<WJob> js;
  auto layer = [&](int t) { for (int q = 2; q >= 0; --q) js.push_back(nat[3 * t + q]); };
  layer(2 * L - 1);
  for (int i = 0; i < L - 1; ++i) layer(L + i);
  for (int i = L - 1; i >= 0; --i) layer(i);
  if ((int)js.size() > kDwMaxJobs) return fail(h, IWAE_EINVAL, "weight-gradient pass: too many layers");
  DwArgs a;
  std::memset(&a, 0, sizeof(a));
  double W = 0.0;
  std::vector<double> cost(js.size(), 0.0);        // MFMA tiles of one block per k step
  for (size_t q = 0; q < js.size(); ++q) {
    const DenseL& d = h->dense[js[q].di];
    DwJob& J = a.job[q];
    J.M = d.fin + 1; J.N = d.fout;
    J.mt = (int)cdiv(J.M, 16); J.nt = (int)cdiv(J.N, 16);
    // blocks of up to 13 x 8 MFMA tiles ("tall"), or 8 x 16 ("wide": a narrow
    // layer's outputs up to 256 in one block, so each row chunk is read once)
    J.wide = J.mt <= 8 && J.nt > 8 ? 1 : 0;
    J.nib = (int)cdiv(J.mt, J.wide ? 8 : 13); J.mtb = (int)cdiv(J.mt, J.nib);
    J.njb = (int)cdiv(J.nt, J.wide ? 16 : 8); J.ntb = (int)cdiv(J.nt, J.njb);
    // a k step's cost in tile units: its MFMA tiles + a fixed cost
    cost[q] = (double)J.mtb * J.ntb + (double)h->tune.dw_alpha;
    W += cost[q] * J.nib * J.njb * (double)cdiv(js[q].rows, 32);
  }
  // block-k-steps of tiles per workgroup; the grid must not exceed one workgroup
  // per CU (8 XCDs x 32): a second round would double the pass
  double target = W / (double)h->tune.dw_wg;
  auto chunk_of = [&](size_t q) {          // job q's row chunk at this target: whole 32-row k steps
    long long S = std::llround((double)cdiv(js[q].rows, 32) * cost[q] / std::max(target, 1.0));
    S = std::max(1LL, std::min<long long>(S, h->dense[js[q].di].cap_splits));
    return cdiv(cdiv(js[q].rows, S), 32) * 32;
  };
  for (int tries = 0; tries < 64; ++tries) {
    long long n = 0;
    for (size_t q = 0; q < js.size(); ++q) n += (long long)a.job[q].nib * a.job[q].njb * cdiv(js[q].rows, chunk_of(q));
    if (n <= h->tune.dw_wg) break;
    target *= 1.02;
  }
  int items = 0;
  for (size_t q = 0; q < js.size(); ++q) {
    const WJob& w = js[q];
    DenseL& d = h->dense[w.di];
    DwJob& J = a.job[q];
    J.A = w.A->p; J.lda = w.A->ld; J.B = w.dZ->p; J.ldb = w.dZ->ld; J.ks = w.ks ? w.ks : h->ones;
    J.scaled = w.ks ? 1 : 0;                   // (unscaled dZ: no row-scale loads)
    J.rows = w.rows;
    J.out = h->slabs + d.slab_off; J.ldo = d.ldw; J.slab_stride = d.size();
    const long long chunk = chunk_of(q);
    J.nsplit = d.splits = (int)cdiv(w.rows, chunk); J.chunk = (int)chunk;
    J.item0 = items;
    items += J.nib * J.njb * J.nsplit;
  }
  a.njobs = (int)js.size();
  a.nitems = items;
  a.per_xcd = (int)cdiv(items, 8);
  HIPCHK(launch_dw(h->stream, a));
  return IWAE_OK;
}

// ------------------------------------------------ row-chain train engine
// Train step = first encoder layer (per image, enc0_forward) -> engine forward
// (jobs E, O) -> bound -> engine backward (jobs O', E') -> first encoder layer
// backward -> grouped weight gradients -> Adam (which also rewrites the split
// copies the engine reads).  See iwae_train.hip.
constexpr int kTcMaxLayers = 3;      // op-table capacity: 4 ops per stochastic layer and direction

static bool tc_fits(const iwae_handle* h, const Plan& P);

static bool use_engine(const iwae_handle* h, const Plan& P) {
  if (!h->tune.engine || !h->x3 || h->path == 1 || h->path == 2 || h->masked) return false;
  if (P.kl) return false;       // VAE_V1's analytic KL: fused row-block path
  if (P.path) return false;     // IWAE_STL / IWAE_DREG: the engine's Gaussian backward has no gradient modes
  if (P.pix) return false;      // pixel-masked steps: the engine's and the ring's Bernoulli epilogues know no mask
  // L_power_p with p < 0: the row weights softmax(p lw) sit on each image's smallest
  // log-weights, the ones of the largest magnitude, and scale the engine's bf16x3
  // rounding of lw by |p| (3 layers, p = -1.5: gradient 1.7e-4 off float64 against
  // 3e-6 on the f32 row-block kernels, which run instead)
  if (P.mode_a == BM_POWER && P.p < 0.f) return false;
  if (h->L > kTcMaxLayers || h->enc[0].d > 2048) return false;   // (image-row backward: d / 4 column quads)
  const long long rows = (long long)P.Bimg * P.kS;
  if (rows > (1LL << 18)) return false;
  // the engine and the ring kernels address each activation / gradient matrix
  // through one buffer resource (32-bit byte offsets, range < 2^31): every
  // matrix they write must stay below 2 GiB, else the row-block path runs
  long long w = h->xdim;
  for (const DenseL& d : h->dense) w = std::max<long long>(w, std::max(d.fout, d.fin + 1));
  w = (w + 31) / 32 * 32;
  if (rows * w * (long long)sizeof(float) >= (1LL << 31)) return false;
  // layers too wide for the engine's LDS plan at 16 rows per workgroup: the
  // row-block kernels (up to kRbMaxWidth) or the layer-wise ones run
  return tc_fits(h, P);
}

struct TcBuild {
  TcJob J;
  std::vector<int> width;
  struct Need { int op, buf, w; };
  std::vector<Need> needs;           // every need() by the op it was made for (the op added last)
  TcBuild() : width(kTcMaxBufs, 0) { std::memset(&J, 0, sizeof(J)); }
  void need(int b, int w) {
    if (b < 0) return;
    width[b] = std::max(width[b], w);
    needs.push_back({J.nop - 1, b, w});
  }
  TcOp& add(int kind) {
    TcOp& o = J.op[J.nop++];
    std::memset(&o, 0, sizeof(o));
    o.kind = kind;
    o.in_buf = o.out_buf = -1;
    return o;
  }
};

static void tc_w(iwae_handle* h, TcOp& o, int di, bool bwd) {
  const DenseL& d = h->dense[di];
  const long long off = bwd ? d.gx_off : d.fx_off;
  o.Whi = h->fx_hi + off;
  o.Wlo = h->fx_lo + off;
  o.W_bytes = (unsigned)((h->fx_elems - off) * (long long)sizeof(__bf16));
  o.ldk = bwd ? d.ldG : d.ldF;
  o.K = bwd ? d.fout : d.fin + 1;
  o.N = bwd ? d.fin : d.fout;
}
// Dense op with an LDS output read by an op of padded width next_k
static TcOp& tc_dense_op(iwae_handle* h, TcBuild& B, int kind, int di, bool bwd, int in, int out, int next_k) {
  TcOp& o = B.add(kind);
  tc_w(h, o, di, bwd);
  o.in_buf = in; o.out_buf = out; o.next_k = next_k; o.ones = bwd ? 0 : 1;
  B.need(in, o.ldk);
  B.need(out, next_k);
  return o;
}
static TcOp& tc_head_op(iwae_handle* h, TcBuild& B, int kind, int di, int in, int out, int d, int next_k) {
  TcOp& o = tc_dense_op(h, B, kind, di, false, in, out, next_k);
  o.d = d;
  o.N = 8 * ((d + 3) / 4);                   // [mu quad | zs quad] groups of 8
  B.need(out, 16 * ((o.N + 15) / 16) / 2);   // latent columns the epilogue writes
  return o;
}

// LDS layout of one job for RT row tiles: every buffer = hi and lo planes of
// [16 RT][ld] bf16 with a row stride of 8 mod 16 dwords (conflict-free
// fragment reads), then the per-row accumulators.  Returns the bytes.
static size_t tc_layout(TcBuild& B, int rt) {
  const int R = 16 * rt;
  int off = 0;
  for (int b = 0; b < kTcMaxBufs; ++b) {
    if (B.width[b] == 0) continue;
    int sdw = (std::max(B.width[b], 32) + 1) / 2;
    while (sdw % 16 != 8) ++sdw;
    B.J.buf_ld[b] = 2 * sdw;
    B.J.buf_off[b] = off;
    off += 2 * R * B.J.buf_ld[b];
  }
  return (size_t)off * sizeof(__bf16);
}

// The same job with every op's LDS output in a buffer of its own (the ops'
// readers renamed; widths from the ops' own needs): no op then writes a buffer
// another op's padding lives in, so all padding can be written before the
// job's first barrier.  False when the job needs more than kTcMaxBufs buffers.
static bool tc_unshare(const TcBuild& B, TcBuild& U) {
  U = B;
  std::fill(U.width.begin(), U.width.end(), 0);
  U.needs.clear();
  int cur[kTcMaxBufs], n = 0;         // the buffer that holds what the job's buffer b holds now
  for (int b = 0; b < kTcMaxBufs; ++b) cur[b] = -1;
  for (int s = 0; s < B.J.nop; ++s) {
    const TcOp& o = B.J.op[s];
    TcOp& u = U.J.op[s];
    if (o.in_buf >= 0) {
      if (cur[o.in_buf] < 0) {          // (scratch nothing wrote: job I's reduction)
        if (n >= kTcMaxBufs) return false;
        cur[o.in_buf] = n++;
      }
      u.in_buf = cur[o.in_buf];
    }
    if (o.out_buf >= 0) {
      if (n >= kTcMaxBufs || o.out_buf == o.in_buf) return false;
      u.out_buf = cur[o.out_buf] = n++;
    }
    for (const TcBuild::Need& q : B.needs) {
      if (q.op != s) continue;
      const int nb = q.buf == o.in_buf ? u.in_buf : q.buf == o.out_buf ? u.out_buf : -1;
      if (nb < 0) return false;
      U.width[nb] = std::max(U.width[nb], q.w);
    }
  }
  return true;
}

// The first encoder layer's l2 and head folded into a forward sample-row job
// (small batches): every workgroup sums the input Dense's slabs of its images,
// runs l2 and the head on those image rows and stores P0, which the job's
// SAMPLE0 then reads (full barrier).  Buffers 0 / 1 are dead before SAMPLE0.
static void tc_fold_first_layer(iwae_handle* h, const Plan& P, TcBuild& B) {
  const StochL& S0 = h->enc[0];
  auto ldF = [&](int di) { return h->dense[di].ldF; };
  TcOp& ls = B.add(TC_LOADSLAB);
  ls.img = 1;
  ls.N = h->dense[S0.l1].fout; ls.out_buf = 0; ls.next_k = ldF(S0.l2);
  ls.y = h->fslab; ls.ld_y = h->eb[0].y1.ld;
  ls.nslab = enc0_nslab(h, P.Bimg); ls.slab_stride = (long long)P.Bimg * h->eb[0].y1.ld;
  ls.out = h->eb[0].y1.p; ls.ld_out = h->eb[0].y1.ld;
  B.need(0, ls.next_k);
  TcOp& a = tc_dense_op(h, B, TC_TANH, S0.l2, false, 0, 1, ldF(S0.head));
  a.img = 1;
  a.out = h->eb[0].y2.p; a.ld_out = h->eb[0].y2.ld;
  TcOp& c = tc_head_op(h, B, TC_HEADP, S0.head, 1, -1, S0.d, 0);
  c.img = 1;
  c.out = h->eb[0].P.p; c.ld_out = h->eb[0].P.ld;
}

static bool use_fold0(const iwae_handle* h, const Plan& P) {
  return h->tune.engine_fold0 && smallm_ok(h, P.Bimg) && h->L >= 1;
}

// The engine's launches.  The value is part of the plan key (tc_key).
enum TcLaunch : int {
  TCL_FWD = 0, TCL_BWD = 1,          // sample-row forward (jobs E, O) / backward (jobs O', E')
  TCL_IMG_FWD = 2, TCL_IMG_BWD = 3,  // first encoder layer's image-row forward (job I) / backward (job I')
  TCL_BWD_ENC = 4,                   // PIWAE's encoder pass: the backward chain on the MIWAE weighting
  TCL_BWD_NO_OUT = 5,                // the backward without job O' (nrb_kernel runs it)
};

static std::vector<long long> tc_key(const Plan& P, TcLaunch which) {
  return {which, P.Bimg, P.Bsplit, P.kS};
}

// wide workgroups (32 / 64 sample rows, two-set weight pipeline) for large batches
static bool tc_wide(const iwae_handle* h, const Plan& P, TcLaunch which) {
  return which != TCL_IMG_FWD && which != TCL_IMG_BWD && (long long)P.Bimg * P.kS >= h->tune.wide_rows;
}

// The jobs of launch `which` (see tc_prepare_one): op tables and the buffer
// widths the LDS layout needs.  Reads the handle only.
static std::vector<TcBuild> tc_build_jobs(iwae_handle* h, const Plan& P, TcLaunch which) {
  const int L = h->L, kS = P.kS;
  const bool wide = tc_wide(h, P, which);
  std::vector<TcBuild> jobs;
  const bool fold0 = which == TCL_FWD && use_fold0(h, P);
  auto ldF = [&](int di) { return h->dense[di].ldF; };
  auto ldG = [&](int di) { return h->dense[di].ldG; };
  if (which == TCL_FWD) {
    // job E: h1 (kept, buffer 0 .. L-2 hold h_0 .. h_{L-2}), P = L-1 (also h_{L-1}), Q = L
    if (L >= 2) {
      TcBuild B;
      const int bP = L - 1, bQ = L;
      auto hbuf = [&](int i) { return i == L - 1 ? bP : i; };
      if (fold0) tc_fold_first_layer(h, P, B);
      TcOp& s0 = B.add(TC_SAMPLE0);
      s0.gsync = fold0;
      s0.d = h->enc[0].d; s0.layer = 0; s0.acc = 1; s0.stdnormal = 0;
      s0.P = h->eb[0].P.p; s0.ld_P = h->eb[0].P.ld; s0.P_div = kS;
      s0.h = h->h[0].p; s0.ld_h = h->h[0].ld; s0.eps = h->eps_st[0].p; s0.ld_eps = h->eps_st[0].ld;
      s0.out_buf = hbuf(0); s0.next_k = ldF(h->enc[1].l1);
      B.need(s0.out_buf, s0.next_k);
      for (int i = 1; i < L; ++i) {
        const StochL& S = h->enc[i];
        TcOp& a = tc_dense_op(h, B, TC_TANH, S.l1, false, hbuf(i - 1), bP, ldF(S.l2));
        a.out = h->eb[i].y1.p; a.ld_out = h->eb[i].y1.ld;
        TcOp& b = tc_dense_op(h, B, TC_TANH, S.l2, false, bP, bQ, ldF(S.head));
        b.out = h->eb[i].y2.p; b.ld_out = h->eb[i].y2.ld;
        const int nk = i < L - 1 ? ldF(h->enc[i + 1].l1) : ldF(h->dec[0].l1);
        TcOp& c = tc_head_op(h, B, TC_SAMPLE, S.head, bQ, hbuf(i), S.d, nk);
        c.layer = i; c.acc = 1; c.stdnormal = i == L - 1;
        c.h = h->h[i].p; c.ld_h = h->h[i].ld; c.eps = h->eps_st[i].p; c.ld_eps = h->eps_st[i].ld;
        c.out = h->eb[i].P.p; c.ld_out = h->eb[i].P.ld;
      }
      for (int j = 0; j < L - 1; ++j) {
        const StochL& D = h->dec[j];
        TcOp& a = tc_dense_op(h, B, TC_TANH, D.l1, false, hbuf(L - 1 - j), bQ, ldF(D.l2));
        a.out = h->db[j].y1.p; a.ld_out = h->db[j].y1.ld;
        TcOp& b = tc_dense_op(h, B, TC_TANH, D.l2, false, bQ, bP, ldF(D.head));
        b.out = h->db[j].y2.p; b.ld_out = h->db[j].y2.ld;
        TcOp& c = tc_head_op(h, B, TC_PRIOR, D.head, bP, -1, D.d, 0);
        c.h = h->h[L - 2 - j].p; c.ld_h = h->h[L - 2 - j].ld;
        c.out = h->db[j].P.p; c.ld_out = h->db[j].P.ld;
      }
      B.J.logq = h->logq; B.J.logp = h->logp;
      jobs.push_back(B);
    }
    // jobs O1, O2: h1 again (same draw), output MLP, Bernoulli over a column
    // range each (the 784-wide output layer is the chain's longest op: both jobs
    // recompute the two 200-wide layers, O1 alone stores them)
    // (only while the launch leaves CUs idle: at large batch the recomputed
    // 200-wide layers cost more than the split saves)
    const int ntile = (h->dense[h->o3].fout + 15) / 16;
    const int nsplit = ntile >= 16 && (long long)P.Bimg * kS <= 2048 ? 2 : 1;
    for (int part = 0; part < nsplit; ++part) {
      const bool first = part == 0;
      TcBuild B;
      if (fold0) tc_fold_first_layer(h, P, B);
      TcOp& s0 = B.add(TC_SAMPLE0);
      s0.gsync = fold0;
      s0.d = h->enc[0].d; s0.layer = 0; s0.acc = L == 1 && first; s0.stdnormal = L == 1;
      s0.P = h->eb[0].P.p; s0.ld_P = h->eb[0].P.ld; s0.P_div = kS;
      if (L == 1 && first) {
        s0.h = h->h[0].p; s0.ld_h = h->h[0].ld; s0.eps = h->eps_st[0].p; s0.ld_eps = h->eps_st[0].ld;
      }
      s0.out_buf = 0; s0.next_k = ldF(h->o1);
      B.need(0, s0.next_k);
      TcOp& a = tc_dense_op(h, B, TC_TANH, h->o1, false, 0, 1, ldF(h->o2));
      if (first) { a.out = h->ob.y1.p; a.ld_out = h->ob.y1.ld; }
      // (y2 over h1's buffer, dead after o1: the 64-row layout fits the LDS)
      TcOp& b = tc_dense_op(h, B, TC_TANH, h->o2, false, 1, 0, ldF(h->o3));
      if (first) { b.out = h->ob.y2.p; b.ld_out = h->ob.y2.ld; }
      TcOp& c = tc_dense_op(h, B, TC_BERN, h->o3, false, 0, -1, 0);
      c.out = h->ob.P.p; c.ld_out = h->ob.P.ld;
      // tiles [t0, t1): t1 caps N (whole tiles), t0 offsets each wave's first tile
      const int t0 = part * (ntile / nsplit), t1 = part + 1 == nsplit ? ntile : (part + 1) * (ntile / nsplit);
      c.t0 = t0;
      if (t1 < ntile) c.N = 16 * t1;
      B.J.bern = h->ebern; B.J.ld_bern = 4; B.J.bern_col = part; B.J.bern_ncol = nsplit;
      B.J.bce = P.need_bce ? h->ebce : nullptr;
      if (L == 1 && first) { B.J.logq = h->logq; B.J.logp = h->logp; }
      jobs.push_back(B);
    }
    // wide launches (large batches): the output job, the longest, dispatched first
    if (wide && jobs.size() == 2) std::swap(jobs[0], jobs[1]);
  } else if (which == TCL_IMG_FWD) {
    // job I: y1 = tanh(sum of the input Dense's slabs) -> l2 tanh -> head: P0 = (mu | zs)
    TcBuild B;
    const StochL& S0 = h->enc[0];
    TcOp& ls = B.add(TC_LOADSLAB);
    ls.N = h->dense[S0.l1].fout; ls.out_buf = 0; ls.next_k = ldF(S0.l2);
    ls.y = h->fslab; ls.ld_y = h->eb[0].y1.ld;
    ls.nslab = enc0_nslab(h, P.Bimg); ls.slab_stride = (long long)P.Bimg * h->eb[0].y1.ld;
    ls.out = h->eb[0].y1.p; ls.ld_out = h->eb[0].y1.ld;
    B.need(0, ls.next_k);
    TcOp& a = tc_dense_op(h, B, TC_TANH, S0.l2, false, 0, 1, ldF(S0.head));
    a.out = h->eb[0].y2.p; a.ld_out = h->eb[0].y2.ld;
    TcOp& c = tc_head_op(h, B, TC_HEADP, S0.head, 1, -1, S0.d, 0);
    c.out = h->eb[0].P.p; c.ld_out = h->eb[0].P.ld;
    jobs.push_back(B);
  } else if (which == TCL_IMG_BWD) {
    // job I': dP0 summed over each image's samples -> head^T (1 - y2^2) -> l2^T (1 - y1^2)
    TcBuild B;
    const StochL& S0 = h->enc[0];
    TcOp& g = B.add(TC_GBWD0);
    g.d = S0.d; g.out_buf = 0; g.in_buf = 2; g.next_k = ldG(S0.head); g.stdnormal = L == 1;
    g.P = h->eb[0].P.p; g.ld_P = h->eb[0].P.ld;
    g.h = h->h[0].p; g.ld_h = h->h[0].ld;
    g.eps = h->eps_st[0].p; g.ld_eps = h->eps_st[0].ld;
    int n = 0;
    g.src[n] = h->dh_out[0].p; g.ld_src[n++] = h->dh_out[0].ld;
    if (L >= 2) {
      g.src[n] = h->dh_prior[0].p; g.ld_src[n++] = h->dh_prior[0].ld;
      g.src[n] = h->dh_enc[0].p; g.ld_src[n++] = h->dh_enc[0].ld;
    }
    g.nsrc = n;
    g.out = h->eb[0].dP.p; g.ld_out = h->eb[0].dP.ld;
    B.need(0, std::max(g.next_k, 2 * S0.d));
    B.need(2, 256);                            // reduction scratch: [16][32][8] floats
    TcOp& a = tc_dense_op(h, B, TC_TGRAD, S0.head, true, 0, 1, ldG(S0.l2));
    a.y = h->eb[0].y2.p; a.ld_y = h->eb[0].y2.ld; a.out = h->eb[0].dY2.p; a.ld_out = h->eb[0].dY2.ld;
    TcOp& b = tc_dense_op(h, B, TC_TGRAD, S0.l2, true, 1, -1, 0);
    b.y = h->eb[0].y1.p; b.ld_y = h->eb[0].y1.ld; b.out = h->eb[0].dY1.p; b.ld_out = h->eb[0].dY1.ld;
    jobs.push_back(B);
  } else {
    // TCL_BWD: the backward launch.  TCL_BWD_ENC (PIWAE's encoder pass): the same
    // chain run on the MIWAE weighting, storing only what the encoder's
    // backward reads (dL/dh, the encoder layers' dZ): the decoder layers' dZ
    // of the IWAE pass stay for their weight gradients.  TCL_BWD_NO_OUT: TCL_BWD
    // without job O' (nrb_kernel runs it)
    const bool dec_out = which != TCL_BWD_ENC;
    // job O': (dpx g) W3^T (1 - y2^2) -> W2^T (1 - y1^2) -> W1^T = dL/dh1 (output MLP part)
    if (which != TCL_BWD_NO_OUT) {
      TcBuild B;
      TcOp& g = B.add(TC_LOADG);
      g.out_buf = 0; g.N = h->xdim; g.next_k = ldG(h->o3);
      g.y = h->ob.P.p; g.ld_y = h->ob.P.ld;
      B.need(0, g.next_k);
      TcOp& a = tc_dense_op(h, B, TC_TGRAD, h->o3, true, 0, 1, ldG(h->o2));
      a.y = h->ob.y2.p; a.ld_y = h->ob.y2.ld; a.out = dec_out ? h->ob.dY2.p : nullptr; a.ld_out = h->ob.dY2.ld;
      // (dY1 over g's buffer, dead after the output layer's op)
      TcOp& b = tc_dense_op(h, B, TC_TGRAD, h->o2, true, 1, 0, ldG(h->o1));
      b.y = h->ob.y1.p; b.ld_y = h->ob.y1.ld; b.out = dec_out ? h->ob.dY1.p : nullptr; b.ld_out = h->ob.dY1.ld;
      TcOp& c = tc_dense_op(h, B, TC_LIN, h->o1, true, 0, -1, 0);
      c.out = h->dh_out[0].p; c.ld_out = h->dh_out[0].ld;
      jobs.push_back(B);
    }
    // job E': decoder prior layers, then encoder layers L-1 .. 1 (row-local chain)
    if (L >= 2) {
      TcBuild B;
      for (int j = 0; j < L - 1; ++j) {
        const int t = L - 2 - j, src = L - 1 - j;
        const StochL& D = h->dec[j];
        TcOp& g = B.add(TC_GBWD_PRIOR);
        g.d = D.d; g.out_buf = 0; g.next_k = ldG(D.head);
        g.P = h->db[j].P.p; g.ld_P = h->db[j].P.ld;
        g.h = h->h[t].p; g.ld_h = h->h[t].ld;
        g.out = dec_out ? h->db[j].dP.p : nullptr; g.ld_out = h->db[j].dP.ld;
        g.dh = h->dh_prior[t].p; g.ld_dh = h->dh_prior[t].ld;
        B.need(0, std::max(g.next_k, 2 * D.d));
        TcOp& a = tc_dense_op(h, B, TC_TGRAD, D.head, true, 0, 1, ldG(D.l2));
        a.y = h->db[j].y2.p; a.ld_y = h->db[j].y2.ld; a.out = dec_out ? h->db[j].dY2.p : nullptr;
        a.ld_out = h->db[j].dY2.ld;
        TcOp& b = tc_dense_op(h, B, TC_TGRAD, D.l2, true, 1, 0, ldG(D.l1));
        b.y = h->db[j].y1.p; b.ld_y = h->db[j].y1.ld; b.out = dec_out ? h->db[j].dY1.p : nullptr;
        b.ld_out = h->db[j].dY1.ld;
        TcOp& c = tc_dense_op(h, B, TC_LIN, D.l1, true, 0, -1, 0);
        c.out = h->dh_dec[src].p; c.ld_out = h->dh_dec[src].ld;
      }
      for (int i = L - 1; i >= 1; --i) {
        const StochL& S = h->enc[i];
        TcOp& g = B.add(TC_GBWD_ENC);
        g.d = S.d; g.out_buf = 0; g.next_k = ldG(S.head); g.stdnormal = i == L - 1;
        g.P = h->eb[i].P.p; g.ld_P = h->eb[i].P.ld;
        g.h = h->h[i].p; g.ld_h = h->h[i].ld;
        g.eps = h->eps_st[i].p; g.ld_eps = h->eps_st[i].ld;
        int n = 0;
        g.src[n] = h->dh_dec[i].p; g.ld_src[n++] = h->dh_dec[i].ld;
        if (i <= L - 2) {
          g.src[n] = h->dh_prior[i].p; g.ld_src[n++] = h->dh_prior[i].ld;
          g.src[n] = h->dh_enc[i].p; g.ld_src[n++] = h->dh_enc[i].ld;
        }
        g.nsrc = n;
        g.out = h->eb[i].dP.p; g.ld_out = h->eb[i].dP.ld;
        B.need(0, std::max(g.next_k, 2 * S.d));
        TcOp& a = tc_dense_op(h, B, TC_TGRAD, S.head, true, 0, 1, ldG(S.l2));
        a.y = h->eb[i].y2.p; a.ld_y = h->eb[i].y2.ld; a.out = h->eb[i].dY2.p; a.ld_out = h->eb[i].dY2.ld;
        TcOp& b = tc_dense_op(h, B, TC_TGRAD, S.l2, true, 1, 0, ldG(S.l1));
        b.y = h->eb[i].y1.p; b.ld_y = h->eb[i].y1.ld; b.out = h->eb[i].dY1.p; b.ld_out = h->eb[i].dY1.ld;
        TcOp& c = tc_dense_op(h, B, TC_LIN, S.l1, true, 0, -1, 0);
        c.out = h->dh_enc[i - 1].p; c.ld_out = h->dh_enc[i - 1].ld;
      }
      jobs.push_back(B);
    }
  }
  return jobs;
}

// LDS bytes of one launch's jobs at rt row tiles: the widest job's buffers,
// then the per-row accumulators (log q, log p, [4][8 waves] partials, the
// in-launch bound's dL/dlw and dpx); acc_off: their float offset
static size_t tc_lds_bytes(std::vector<TcBuild>& jobs, int rt, int* acc_off = nullptr) {
  size_t mx = 0;
  for (auto& B : jobs) mx = std::max(mx, tc_layout(B, rt));
  const int off = (int)((mx + 15) / 16 * 4);          // floats, 16-byte aligned
  if (acc_off) *acc_off = off;
  return (size_t)off * sizeof(float) + (size_t)(4 + 4 * 8) * 16 * rt * sizeof(float);
}

// The ops' hot records (TcHot) of a job whose LDS layout is final: everything
// the op loop and a Dense op's prologue need, resolved here once per plan so
// the kernel computes nothing about an op from its TcOp fields.
static void tc_resolve_hot(TcJob& J, bool prepad) {
  auto reads_global = [](const TcOp& o) { return o.kind == TC_PRIOR || o.kind == TC_GBWD_ENC || o.gsync != 0; };
  for (int s = 0; s < kTcMaxOps; ++s) std::memset(&J.hot[s], 0, sizeof(TcHot));
  std::memset(J.pre, 0, sizeof(J.pre));
  J.npre = 0;
  for (int s = 0; s < J.nop; ++s) {
    const TcOp& o = J.op[s];
    TcHot& H = J.hot[s];
    const TcOp* nx = s + 1 < J.nop ? &J.op[s + 1] : nullptr;
    H.flags = (uint32_t)o.kind | (o.img ? kTcHotImg : 0u) | (o.ones ? kTcHotOnes : 0u);
    // LDS-only barrier unless the next op reads what this launch stored (or none follows)
    if (!nx || reads_global(*nx)) H.flags |= kTcHotFullSync;
    else if (nx->kind <= TC_LAST_DENSE) H.flags |= kTcHotNextDense;
    if (o.kind > TC_LAST_DENSE) continue;
    const uint64_t whi = (uint64_t)(uintptr_t)o.Whi, wlo = (uint64_t)(uintptr_t)o.Wlo;
    H.whi_lo = (uint32_t)whi; H.whi_hi = (uint32_t)(whi >> 32);
    H.wlo_lo = (uint32_t)wlo; H.wlo_hi = (uint32_t)(wlo >> 32);
    H.W_bytes = o.W_bytes;
    const int ob = o.out_buf >= 0 ? o.out_buf : o.in_buf;
    H.in_off = (uint32_t)J.buf_off[o.in_buf]; H.in_ld = (uint32_t)J.buf_ld[o.in_buf];
    H.out_off = (uint32_t)J.buf_off[ob]; H.out_ld = (uint32_t)J.buf_ld[ob];
    // zero padding [width, next_k) of the output the op writes before its tiles
    const int width = o.kind == TC_SAMPLE ? o.d : o.N;
    if (o.out_buf >= 0 && o.next_k > width) H.pad = (uint32_t)width | ((uint32_t)o.next_k << 16);
    if (prepad && H.pad) {               // written before the job's first barrier instead
      J.pre[J.npre++] = TcPad{H.out_off, H.out_ld, H.pad, (uint32_t)(o.ones ? 1 : 0)};
      H.pad = 0;
    }
    const int nch = (o.ldk + 127) / 128;     // k chunks of 4 k steps (TC_KS) of 32
    H.kt = (uint32_t)(o.ldk >> 5) | ((uint32_t)nch << 16);
    H.ntile = (uint32_t)((o.N + 15) >> 4);
    H.t0 = (uint32_t)o.t0;
    H.N = (uint32_t)o.N;
  }
}

constexpr size_t kTcLdsBytes = 160 * 1024;

// Whether every launch of an engine step has a plan that fits the LDS at the
// smallest workgroup (one 16-row tile).  It depends on the layer widths and,
// through fold0, on whether the batch takes the few-row launches: decided
// once per model for each, so use_engine() can decline the engine (the step
// then runs on the row-block or the layer-wise kernels) instead of failing in
// tc_prepare_one.  (TCL_BWD_ENC and TCL_BWD_NO_OUT run subsets of TCL_BWD's jobs.)
static bool tc_fits(const iwae_handle* ch, const Plan& P) {
  iwae_handle* h = const_cast<iwae_handle*>(ch);     // (the builders only read it)
  if ((int)h->eb.size() < h->L) return true;          // no workspace yet: decided at the first step
  int& fit = h->tc_fit[use_fold0(h, P) ? 1 : 0];
  if (fit < 0) {
    fit = 1;
    for (TcLaunch which : {TCL_FWD, TCL_BWD, TCL_IMG_FWD, TCL_IMG_BWD}) {
      std::vector<TcBuild> jobs = tc_build_jobs(h, P, which);
      if (tc_lds_bytes(jobs, 1) > kTcLdsBytes) fit = 0;
    }
  }
  return fit == 1;
}

// Plans of this shape, built once and uploaded (the launches: TcLaunch; the
// image-row forward runs after the first encoder layer's input Dense).
static int tc_prepare_one(iwae_handle* h, const Plan& P, TcLaunch which) {
  const auto key = tc_key(P, which);
  if (h->tc_plans.count(key)) return IWAE_OK;
  const int kS = P.kS;
  const bool wide = tc_wide(h, P, which);
  std::vector<TcBuild> jobs = tc_build_jobs(h, P, which);
  if ((int)jobs.size() > kTcMaxJobs) return fail(h, IWAE_EINVAL, "engine: too many jobs");
  // rows per workgroup: the largest tile count the LDS allows, fewer for small batches
  const bool img = which == TCL_IMG_FWD || which == TCL_IMG_BWD;
  const long long rows = img ? (long long)P.Bimg : (long long)P.Bimg * kS;
  // image rows: one image per workgroup (latency-bound chains of a few rows), up to 256 workgroups
  // (knobs img_rows_fwd / img_rows_bwd: rows per workgroup of job I / I' instead)
  int row_step = img ? (int)std::max<long long>(1, cdiv(P.Bimg, 256)) : 0;
  if (which == TCL_IMG_FWD && h->tune.img_rows_fwd > 0) row_step = h->tune.img_rows_fwd;
  if (which == TCL_IMG_BWD && h->tune.img_rows_bwd > 0) row_step = h->tune.img_rows_bwd;
  // rows per workgroup: 16 (four-set pipeline) below wide_rows, else the
  // widest the LDS allows (two-set pipeline)
  const int want = wide ? (which == TCL_FWD ? 4 : h->tune.wide_rt) : h->tune.tc_rt;
  TcRec rec;
  for (int rt : {4, 2, 1}) {
    if (rt > want) continue;
    int acc_off = 0;
    size_t lds = tc_lds_bytes(jobs, rt, &acc_off);
    if (lds <= kTcLdsBytes) {
      // 16-row plans that still fit with a buffer per op output: padding off
      // the op chain (never a reason not to fit: the shared layout stays
      // otherwise).  The backward launch's bound then stages its images' log
      // weights in the row reduction's scratch ([4][8 waves][16] floats).
      std::vector<TcBuild> own(jobs.size());
      bool ok = rt == 1 && (which == TCL_FWD || img || 8 * r4(kS) <= 4 * 8 * 16);
      for (size_t j = 0; ok && j < jobs.size(); ++j) ok = tc_unshare(jobs[j], own[j]);
      if (ok) {
        int acc2 = 0;
        const size_t lds2 = tc_lds_bytes(own, rt, &acc2);
        if (lds2 <= kTcLdsBytes) {
          jobs = own; lds = lds2; acc_off = acc2;
          rec.prepad = true;
        }
      }
      rec.rt = rt;
      rec.lds = lds;
      rec.acc_off = acc_off;
      TcPlan plan;
      std::memset(&plan, 0, sizeof(plan));
      plan.njobs = (int)jobs.size();
      plan.acc_off = acc_off;
      for (size_t j = 0; j < jobs.size(); ++j) {
        plan.job[j] = jobs[j].J;
        tc_resolve_hot(plan.job[j], rec.prepad);
        for (int o = 0; o < jobs[j].J.nop; ++o) rec.kinds |= 1u << jobs[j].J.op[o].kind;
      }
      HIPCHK(hipMalloc(&rec.dev, sizeof(TcPlan)));
      HIPCHK(hipMemcpy(rec.dev, &plan, sizeof(TcPlan), hipMemcpyHostToDevice));
      const int nb = (int)cdiv(rows, row_step > 0 ? row_step : 16 * rt);
      rec.row_step = row_step;
      for (size_t j = 0; j < jobs.size(); ++j) {
        rec.nb[j] = nb;
        for (int o = 0; o < jobs[j].J.nop; ++o) {
          const TcOp& op = jobs[j].J.op[o];
          if (op.kind > TC_LAST_DENSE) continue;
          const int kin = op.kind == TC_TGRAD || op.kind == TC_LIN ? op.K : op.K - 1;
          const int nout = op.kind == TC_SAMPLE || op.kind == TC_PRIOR ? 2 * op.d : op.N;
          // (a folded image-row op: its images once, however many workgroups recompute them)
          if (op.img) { if (j == 0) rec.flop += 2.0 * (double)P.Bimg * kin * nout; continue; }
          rec.flop += 2.0 * (double)rows * kin * nout;
        }
      }
      h->tc_plans[key] = rec;
      return IWAE_OK;
    }
  }
  return fail(h, IWAE_EINVAL, "engine: layer widths exceed the LDS");
}

static int tc_prepare(iwae_handle* h, const Plan& P) {
  CHK(tc_prepare_one(h, P, TCL_IMG_FWD));
  CHK(tc_prepare_one(h, P, TCL_IMG_BWD));
  CHK(tc_prepare_one(h, P, TCL_FWD));
  if (P.piwae) CHK(tc_prepare_one(h, P, TCL_BWD_ENC));
  return tc_prepare_one(h, P, TCL_BWD);
}

// dlw / dpx: the bound's weighting the launch reads (default: the bound's
// first one; PIWAE's encoder pass: the MIWAE one, dlw2 / dpx2)
static int tc_run(iwae_handle* h, const Plan& P, const EpsSet& E, TcLaunch which, const BoundArgs* bnd = nullptr,
                  const float* dlw = nullptr, const float* dpx = nullptr, bool unit = false) {
  auto it = h->tc_plans.find(tc_key(P, which));
  if (it == h->tc_plans.end()) return fail(h, IWAE_EINVAL, "engine plan missing");
  const TcRec& rec = it->second;
  TcArgs a;
  std::memset(&a, 0, sizeof(a));
  a.plan = rec.dev;
  a.kinds = rec.kinds;
  int tot = 0;
  for (int j = 0; j < kTcMaxJobs; ++j) {
    a.block_start[j] = tot;
    tot += rec.nb[j];
  }
  a.block_start[kTcMaxJobs] = tot;
  a.rows = (which == TCL_IMG_FWD || which == TCL_IMG_BWD) ? P.Bimg : P.Bimg * P.kS; a.kS = P.kS;
  a.row_step = rec.row_step;
  // XCD-aware placement: the XCDs split over the jobs in proportion to their
  // workgroups, so each XCD's L2 fetches one job's weight copies (a launch that
  // fills more than the chip keeps the plain order)
  int njobs = 0;
  for (int j = 0; j < kTcMaxJobs; ++j) njobs += rec.nb[j] > 0;
  if (h->tune.tc_xcd && njobs > 1 && tot <= 256) {
    int cnt[kTcMaxJobs] = {};
    for (int q = 0; q < kTcMaxJobs; ++q) cnt[q] = rec.nb[q] > 0;      // one XCD per job first
    for (int x = njobs; x < 8; ++x) {                                   // then the most loaded job
      int best = -1;
      for (int q = 0; q < kTcMaxJobs; ++q)
        if (cnt[q] > 0 && (best < 0 || (double)rec.nb[q] / cnt[q] > (double)rec.nb[best] / cnt[best])) best = q;
      ++cnt[best];
    }
    int slots = 0;
    for (int q = 0, x = 0; q < kTcMaxJobs; ++q) {
      a.xcd_count[q] = cnt[q];
      for (int r = 0; r < cnt[q]; ++r, ++x) { a.xcd_job[x] = q; a.xcd_rank[x] = r; }
      if (cnt[q] > 0) slots = std::max(slots, (int)cdiv(rec.nb[q], cnt[q]));
    }
    a.xcd_slots = slots;
  }
  a.x = h->x_in.p; a.ldx = h->x_in.ld;
  a.seed = h->seed; a.rng_base = &h->ds->rng[0];
  for (int i = 0; i < h->L && i < 8; ++i) { a.eps_a[i] = E.a[i]; a.eps_b[i] = E.b[i]; }
  a.Bsplit = P.Bsplit; a.Bimg = P.Bimg;
  a.dlw = dlw ? dlw : h->dlw; a.dpx = dpx ? dpx : h->dpx; a.wa = P.wa;
  a.wb = P.wb; a.need_bce = P.need_bce;
  a.unit_w = unit ? 1 : 0;
  if (rec.rt == 1) {
    // store policy (16-row plans): bit 1 the forward launches, 2 the backward
    // ones write-through; 32: the forward's jobs before its last (E and O1,
    // which end before O2) write their XCD's L2 back as they end
    const bool fwd = which == TCL_FWD || which == TCL_IMG_FWD;
    a.st_wt = (h->tune.st_wt & (fwd ? 1 : 2)) != 0;
    if (which == TCL_FWD && (h->tune.st_wt & 32) && njobs > 1) a.rel_jobs = (1u << (njobs - 1)) - 1u;
  }
  a.bnd_block = -1;
  if (bnd) {
    // the bound in this (backward) launch: its rows' dL/dlw per workgroup, the
    // whole bound in one extra workgroup (it advances the Philox base, which
    // this launch does not read: nothing samples in the backward)
    a.bnd = *bnd;
    a.bnd_rows = 1;
    a.bnd_block = h->tune.tc_xcd && a.xcd_slots > 0 ? 8 * a.xcd_slots : tot;
    a.bnd_ld = r4(P.kS);
    a.bnd_lds = rec.acc_off + (2 + 4 * 8) * 16 * rec.rt;
    a.bnd_stage = rec.prepad ? rec.acc_off + 2 * 16 * rec.rt : 0;
    a.rng_base = nullptr;
  }
  const bool prof = (which == TCL_FWD || which == TCL_BWD) && h->prof.kind == 10 + which;
  h->count.tc++;
  if (h->step.defer_launch) {
    // recorded for a combined launch (tcu_kernel); launch_pending issues it
    h->pend.tc = a; h->pend.tc_rt = rec.rt; h->pend.tc_lds = rec.lds; h->pend.tc_have = true;
    return IWAE_OK;
  }
  if (prof) {
    if (h->prof.used + 2 > h->prof.ev.size()) {
      for (int i = 0; i < 256; ++i) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->prof.ev.push_back(e);
      }
    }
    HIPCHK(hipEventRecord(h->prof.ev[h->prof.used], h->stream));
  }
  HIPCHK(launch_tc(h->stream, a, rec.rt, rec.lds));
  if (prof) {
    HIPCHK(hipEventRecord(h->prof.ev[h->prof.used + 1], h->stream));
    h->prof.used += 2;
    h->prof.flop += rec.flop;
    h->prof.have = true; h->prof.is_tc = true;
    h->prof.tc = a; h->prof.tc_rt = rec.rt; h->prof.tc_lds = rec.lds; h->prof.flop1 = rec.flop;
    if (bnd) {
      // replays write the loss, Philox base and Adam step into scratch
      if (!h->prof.scratch) HIPCHK(hipMalloc(&h->prof.scratch, 64 * sizeof(float)));
      h->prof.tc.bnd.loss = h->prof.scratch;
      h->prof.tc.bnd.rng_base = reinterpret_cast<uint64_t*>(h->prof.scratch + 8);
      h->prof.tc.bnd.adam_step = bnd->adam_step ? reinterpret_cast<long long*>(h->prof.scratch + 16) : nullptr;
    }
  }
  return IWAE_OK;
}

static float* train_loss_ptr(iwae_handle* h) { return h->step.loss_out ? h->step.loss_out : &h->ds->scalars[0]; }

// End of a train step / forward_backward: sum the weight-gradient slabs into the
// gradient buffer and (adam) step.  Data parallel (iwae_dp_init): the buffer gets
// B_local * g and B_local in its tail element; with the library communicator the
// n + 4 floats are summed over the ranks right here (ncclAllReduce on the step's
// stream, inside the captured graph) and Adam scales by 1 / sum_r B_r.
// sum count floats of the gradient buffer from offset over the ranks, in place, on the step's stream
static int allreduce_grad(iwae_handle* h, long long offset, long long count, const char* what) {
  if (ncclAllReduce(h->grad + offset, h->grad + offset, (size_t)count, ncclFloat32, ncclSum, h->comm, h->stream) !=
      ncclSuccess)
    return fail(h, IWAE_EHIP, std::string("ncclAllReduce of the gradient") + what + " failed");
  return IWAE_OK;
}

// Data parallel: the slabs summed into B_local * g (B_local in the tail), then
// (all_reduce: a step that applies Adam) the n + 4 floats summed over the ranks.
static int dp_reduce_slabs(iwae_handle* h, const Plan& P, bool all_reduce) {
  CHK(run_adam(h, AdamMode::weighted_slab_sum((float)P.B, h->grad + h->nparam_int)));
  if (!all_reduce) return IWAE_OK;
  if (!h->comm) return fail(h, IWAE_EINVAL, "data parallel without a library communicator");
  return allreduce_grad(h, 0, h->nparam_int + 4, "");
}

static int finish_step(iwae_handle* h, const Plan& P, bool adam) {
  if (!h->dp_weighted) return run_adam(h, AdamMode::from_slabs(adam));
  CHK(dp_reduce_slabs(h, P, adam));
  return adam ? run_adam(h, AdamMode::from_grad_over(h->grad + h->nparam_int)) : IWAE_OK;
}

// The bound inside the engine's backward launch (no bound launch): up to 256
// samples per image (an image's log weights staged per wave in the op buffers'
// LDS, which must hold 8 of them plus the spare workgroup's 64 floats).
static bool piwae_unit(const iwae_handle* h, const Plan& P, bool ring);
// (PIWAE with the unit-weight chain: the launch's rows need no weighting, and
// the spare workgroup writes both weightings, dlw / dpx and dlw2 / dpx2, for
// the weight gradients and the image-row job)
static bool use_tc_bound(iwae_handle* h, const Plan& P, bool ring) {
  // (one spare workgroup runs the whole bound: up to 64 images, 8 per wave)
  if (!h->tune.tc_bound || P.kS > 256 || P.Bimg > 64 || P.need_bce || P.kl || h->prof.kind == 13) return false;
  if (P.piwae && !piwae_unit(h, P, ring)) return false;
  auto it = h->tc_plans.find(tc_key(P, TCL_BWD));
  if (it == h->tc_plans.end()) return false;
  return (long long)it->second.acc_off >= 64 + 8LL * r4(P.kS);
}

static bool nring_train_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool& ran);
static bool nring_plan(iwae_handle* h, NrLaunch& R);
static bool nrb_plan(iwae_handle* h, NrbLaunch& R);
static bool nring_train_backward(iwae_handle* h, const Plan& P, bool fwd_ring, bool& ran, hipStream_t st);
static bool nre_plan(iwae_handle* h, NreLaunch& R);
static bool nring_train_backward_enc(iwae_handle* h, const Plan& P, bool& ran);

// PIWAE (PDF p7) on the engine with ONE backward chain: every quantity of the
// backward is linear in a row's weight (dL/dlw for the log q / prior terms, dpx
// for the Bernoulli term), so the chain runs once with unit weights and each
// consumer applies the weighting it needs -- IWAE_{k1 k2} (dlw, dpx) for the
// decoder's weight gradients, MIWAE(k1, k2) (dlw2) for the encoder's.  Where
// the row-chain engine runs the backward (not the ring kernels) and the image-
// row job takes the first encoder layer's backward.
static bool piwae_unit(const iwae_handle* h, const Plan& P, bool ring) {
  return P.piwae && !ring && (h->tune.engine_img_bwd || (h->tune.engine_img && !smallm_ok(h, P.Bimg))) && h->tune.piwae_one;
}
// Issue the launches tc_run / run_update recorded under defer_launch: job I'
// and the fused update as ONE tcu_kernel launch when every workgroup of it is
// resident at once (grid <= the device's CU count at one 512-thread workgroup
// per CU: the update's 147 KiB of LDS), else as the two launches they would
// have been.
static int launch_pending(iwae_handle* h) {
  const bool tc = h->pend.tc_have, up = h->pend.upd_have;
  h->pend.tc_have = h->pend.upd_have = false;
  if (tc && up) {
    const TcArgs& a = h->pend.tc;
    const UpdArgs& u = h->pend.upd;
    const int n_tc = a.block_start[kTcMaxJobs];
    const int grid = ((n_tc + 7) & ~7) + 8 * (u.per_xcd + u.per_xcd2);
    bool one_split = true;                         // (tcu_kernel's update has no split-K path)
    for (int j = 0; j < u.njobs; ++j) one_split = one_split && u.job[j].nsplit <= 1;
    const bool ok = h->pend.tc_rt == 1 && a.xcd_slots == 0 && a.bnd_block < 0 && !u.search && !u.apply &&
                    one_split && grid <= h->n_cu && n_tc > 0 && h->pend.upd_cons > 0;
    if (ok) {
      UpdWait w;
      w.ctr = h->tcu_ctr; w.err = h->err_dev; w.wait_mask = h->pend.upd_mask;
      w.n_prod = n_tc; w.n_cons = h->pend.upd_cons;
      // (fault injection: wait for a producer that does not exist, briefly)
      w.n_expect = n_tc + (h->tune.tcu_wait_test ? 1 : 0);
      w.max_spins = h->tune.tcu_wait_test ? 4096u : (1u << 24);
      // write-through hand-off where every waiting tile takes the update's
      // one-iteration path (its dZ loads are the sc1 ones): launch_tcu keeps it
      // only on the write-through instantiation
      w.wt = h->tune.tcu_wt;
      for (int j = 0; j < u.njobs; ++j)
        if ((w.wait_mask >> j) & 1u) w.wt = w.wt && u.job[j].rows > 0 && u.job[j].rows <= kUpdRowsPerIter;
      const size_t lds = std::max(h->pend.tc_lds, upd_lds_bytes());
      HIPCHK(launch_tcu(h->stream, a, u, w, lds));
      h->count.tcu++;
      if (h->prof.kind == 16 && !h->prof.have && u.do_adam) {
        // live timing (iwae_profile_replay): replays repeat this launch with the
        // update part on scratch copies of the parameters, moments and
        // fragment-major copies (job I' rewrites its own outputs): the model is untouched
        UpdArgs r = u;
        CHK(prof_state_copy(h, r));
        const TcArgs ta = a;
        h->prof.mem = [ta, r, w, lds](hipStream_t st) { return launch_tcu(st, ta, r, w, lds); };
        h->prof.flop1 = 0.0;
        h->prof.have = true;
      }
      return IWAE_OK;
    }
  }
  if (tc) HIPCHK(launch_tc(h->stream, h->pend.tc, h->pend.tc_rt, h->pend.tc_lds));
  if (up) HIPCHK(launch_update(h->stream, h->pend.upd));
  return IWAE_OK;
}

// How an engine train step ends ("How a train step ends"): where the weight
// gradients come from and what turns them into updated weights, Adam state and fragment-major
// copies (IN_FUSED: nothing follows the fused launch; APPLY_GRAD: data parallel, after the all-reduce).
struct StepRoute {
  enum Grads { FUSED_UPDATE, DW_KERNEL, UPDATE_SLAB_PASS, GROUPED_GEMMS } grads;
  enum Finish { IN_FUSED, APPLY_GRAD, APPLY_SLABS, ADAM_THEN_FX } finish;
  bool tcu;      // the fused launch is recorded for ONE launch with job I' (tcu_kernel)
};

static StepRoute step_route(const iwae_handle* h, const Plan& P, bool adam, bool img_bwd) {
  const bool fused = use_update(h, P), slab_pass = use_update_slabs(h, P), dp = h->dp_weighted;
  StepRoute r;
  r.grads = fused ? StepRoute::FUSED_UPDATE : !slab_pass ? StepRoute::GROUPED_GEMMS
            : h->tune.dw_wide ? StepRoute::DW_KERNEL : StepRoute::UPDATE_SLAB_PASS;
  const bool apply = adam && h->tune.upd && upd_tiles_ok(h);    // the update kernel's apply modes can run
  if (fused) r.finish = dp && adam ? StepRoute::APPLY_GRAD : StepRoute::IN_FUSED;
  else if (dp && apply) r.finish = StepRoute::APPLY_GRAD;
  else if (!dp && apply && h->tune.upd_apply && h->slabs) r.finish = StepRoute::APPLY_SLABS;
  else r.finish = StepRoute::ADAM_THEN_FX;
  // job I' and the fused update as one launch (tcu_kernel): recorded by tc_run
  // and run_update, issued by launch_pending.  From 256 sample rows: below, the update's
  // sample-row tiles are too short to cover job I' and the in-launch hand-off
  // costs more than the launch boundary (configs[0], 100 rows: 0.0958 vs
  // 0.0968 ms per step as two launches; profiles/r06j_tcu_rows_ab.txt)
  r.tcu = img_bwd && h->tune.tcu && fused && !dp && (h->prof.kind < 0 || h->prof.kind == 16) &&
          (long long)P.Bimg * P.kS >= 256;
  return r;
}

// After the sample-row backward: the first encoder layer's backward, the weight gradients, the update.
static int engine_step_end(iwae_handle* h, const Plan& P, const EpsSet& E, bool adam, bool img, bool unit) {
  // (a second stream for the first encoder layer's backward beside the other
  // weight gradients measured slower inside the captured graph: sequential).
  // Its image-row job also at small batches (B = 20: step 128.1 -> 126.4 us
  // against the row-block Gaussian backward + two few-row launches)
  const bool img_bwd = img || h->tune.engine_img_bwd;
  const StepRoute r = step_route(h, P, adam, img_bwd);
  h->step.defer_launch = r.tcu;
  if (img_bwd) CHK(tc_run(h, P, E, TCL_IMG_BWD, nullptr, P.piwae ? h->dlw2 : nullptr, nullptr, unit));
  else CHK(fused_encoder_bwd(h, P, P.piwae ? h->dlw2 : h->dlw, 0));
  float* const tail = h->grad + h->nparam_int;       // data parallel: the batch size behind the gradient
  const long long out0 = h->dense[h->o1].off;        // ... the output MLP's range (the last of the buffer)
  switch (r.grads) {
    case StepRoute::FUSED_UPDATE:
      if (!h->dp_weighted) {
        // weight gradients, Adam and the fragment-major copies in one launch
        CHK(run_update(h, P, UpdMode::fused(adam)));
        h->step.defer_launch = false;
        CHK(launch_pending(h));
        break;
      }
      // data parallel: the fused gradient pass (B_local * g, B_local in the
      // tail), the all-reduce, then Adam and the fragment-major copies.  (Not
      // dp_reduce_slabs: the gradients come from two update launches on two
      // streams and are reduced in two buckets, not from one sum of the slabs.)
      if (!adam) return run_update(h, P, UpdMode::dp_grads(WG_ALL, h->stream));
      if (!h->comm) return fail(h, IWAE_EINVAL, "data parallel without a library communicator");
      // two buckets whose gradient passes run side by side (each pass alone is a
      // latency chain on a fraction of the CUs): the output MLP's (the last
      // range of the buffer, with the tail) on the step's stream, then its
      // all-reduce while the other layers' pass may still run on the side
      // stream; then their all-reduce; then ONE launch of Adam and the FX / GX
      // copies from the summed buffer (the update kernel's apply mode, in place
      // of the Adam and FX-refresh launches).  Both all-reduces on one stream:
      // collectives of one communicator stay ordered.
      HIPCHK(hipEventRecord(h->ev_fork, h->stream));
      HIPCHK(hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
      CHK(run_update(h, P, UpdMode::dp_grads(WG_BUT_OUT, h->side_stream)));
      HIPCHK(hipEventRecord(h->ev_join, h->side_stream));
      CHK(run_update(h, P, UpdMode::dp_grads(WG_OUT_ONLY, h->stream)));
      CHK(allreduce_grad(h, out0, h->nparam_int - out0 + 4, " (output MLP bucket)"));
      HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
      CHK(allreduce_grad(h, 0, out0, ""));
      break;
    case StepRoute::DW_KERNEL: CHK(run_dw(h, P)); break;
    case StepRoute::UPDATE_SLAB_PASS: CHK(run_update(h, P, UpdMode::slab_pass())); break;
    case StepRoute::GROUPED_GEMMS: CHK(weight_grads(h, P, WG_ALL)); break;
  }
  switch (r.finish) {
    case StepRoute::IN_FUSED: break;
    case StepRoute::APPLY_GRAD:
      // data parallel: as finish_step, but Adam + the FX / GX copies in one
      // update launch (apply mode) in place of the Adam and FX-refresh launches
      if (r.grads != StepRoute::FUSED_UPDATE) CHK(dp_reduce_slabs(h, P, /*all_reduce=*/true));
      CHK(run_update(h, P, UpdMode::apply_grad(tail)));
      break;
    case StepRoute::APPLY_SLABS:
      // the slabs summed, Adam and the fragment-major copies in one launch (the
      // update kernel's apply mode) in place of adam_kernel + fx_refresh_kernel
      CHK(run_update(h, P, UpdMode::apply_slabs()));
      break;
    case StepRoute::ADAM_THEN_FX:
      CHK(finish_step(h, P, adam));
      // the next step's engine reads the updated weights' fragment-major copies
      if (adam) CHK(run_fx(h));
      break;
  }
  if (adam) h->fx_version = h->params_version;
  return IWAE_OK;
}

static int engine_train_body(iwae_handle* h, const Plan& P, const EpsSet& E, bool adam) {
  // The first encoder layer's l2 / head: up to 32 images the few-row N-split
  // launches (one 16-column tile per workgroup; at B = 20 the image-row jobs,
  // one image per workgroup streaming both layers' weights, took 18.2 + 18.4
  // us against 12 + 21 us and the step 142.4 vs 139.9 us), above that the
  // image-row engine jobs (B = 512: 0.954 vs 0.985 ms per step against the
  // split-K GEMM + row-block kernels)
  const bool img = h->tune.engine_img && !smallm_ok(h, P.Bimg);
  if (img) {
    // first encoder layer: input Dense (few-row / split-K), then its image-row engine job
    CHK(enc0_forward(h, P, true));
    CHK(tc_run(h, P, E, TCL_IMG_FWD));
  } else if (use_fold0(h, P)) {
    // input Dense only: its l2 and head run inside the forward launch's jobs
    CHK(enc0_forward(h, P, true));
  } else {
    CHK(enc0_forward(h, P));
  }
  bool ring = false;
  if (!nring_train_forward(h, P, E, ring)) return fail(h, IWAE_EHIP, "weight-ring train forward launch failed");
  if (!ring) CHK(tc_run(h, P, E, TCL_FWD));
  if (use_tc_bound(h, P, ring)) {
    const BoundArgs b = make_bound_args(h, P, true, -1.f, train_loss_ptr(h), adam, true);
    CHK(tc_run(h, P, E, TCL_BWD, &b, nullptr, nullptr, piwae_unit(h, P, ring)));
  } else {
    CHK(run_bound(h, P, true, -1.f, train_loss_ptr(h), adam, true));
    // the output MLP's backward on the weight ring where the forward ran on it,
    // then the engine's launch without it (encoder and prior chains).  The two
    // are independent (both read the bound's dL/dlw / dpx, the image-row job
    // after them reads both): nring_bwd 2 runs the ring kernel on the side
    // stream beside the engine's launch (each leaves CUs idle: 200 and 400
    // workgroups), joined before the image-row job
    // (nring_bwd 3, the encoder / prior backward on nre_kernel too: sequential,
    // 0.574-0.577 vs 0.582-0.583 ms with nrb_kernel on the side stream -- the
    // two ring kernels hold a CU's LDS each and cannot share one)
    const bool side = ring && h->tune.nring_bwd == 2 && h->L >= 2;
    if (side) {
      HIPCHK(hipEventRecord(h->ev_fork, h->stream));
      HIPCHK(hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
    }
    bool rb = false;
    if (!nring_train_backward(h, P, ring, rb, side ? h->side_stream : h->stream))
      return fail(h, IWAE_EHIP, "weight-ring backward launch failed");
    if (side) HIPCHK(hipEventRecord(h->ev_join, h->side_stream));
    // (the output MLP's weight-gradient slab pass following it there, beside the
    // other layers' pass on the step's stream, measured slower: 0.657-0.662 vs
    // 0.613-0.621 ms at B = 512 -- the two passes, one workgroup per CU each,
    // compete for the CUs)
    if (!rb) {
      CHK(tc_run(h, P, E, TCL_BWD, nullptr, nullptr, nullptr, piwae_unit(h, P, ring)));
    } else if (h->L >= 2) {
      // nring_bwd 3: the encoder / prior chains on the ring as well
      bool re = false;
      if (!nring_train_backward_enc(h, P, re)) return fail(h, IWAE_EHIP, "weight-ring encoder backward launch failed");
      if (!re) CHK(tc_run(h, P, E, TCL_BWD_NO_OUT));
    }
    if (side) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  // PIWAE (PDF p7): the decoder's weight gradients come from IWAE_{k1 k2} (the
  // pass above stored their dZ), the encoder's from MIWAE(k1, k2): the
  // backward chain again on dlw2 / dpx2, storing only the encoder path
  // With unit row weights (piwae_unit) the one chain above serves both
  // weightings: the weight gradients scale each layer's dZ rows by its own
  // (run_update / run_dw: dpx or dlw for the decoder, dlw2 for the encoder),
  // and the image-row job scales its dL/dh sources by dlw2 per sample.
  const bool unit = piwae_unit(h, P, ring);
  if (P.piwae && !unit) CHK(tc_run(h, P, E, TCL_BWD_ENC, nullptr, h->dlw2, h->dpx2));
  h->step.piwae_ks = unit;
  return engine_step_end(h, P, E, adam, img, unit);
}

static int fused_train_body(iwae_handle* h, const Plan& P, const EpsSet& E, bool adam) {
  CHK(fused_forward(h, P, E, true));
  CHK(run_bound(h, P, true, -1.f, train_loss_ptr(h), adam));
  if (P.piwae) {
    CHK(fused_decoder_bwd(h, P, h->dlw, h->dpx, false));      // decoder weights: IWAE_{k1 k2}
    CHK(weight_grads(h, P, WG_DECODER));
    CHK(fused_decoder_bwd(h, P, h->dlw2, h->dpx2, true));     // encoder path: MIWAE(k1, k2) (DReG: softmax^2)
    CHK(fused_encoder_bwd(h, P, h->dlw2));
    CHK(weight_grads(h, P, WG_ENCODER));
  } else {
    CHK(fused_decoder_bwd(h, P, h->dlw, h->dpx, true));
    CHK(fused_encoder_bwd(h, P, h->dlw));
    CHK(weight_grads(h, P, WG_ALL));
  }
  return finish_step(h, P, adam);
}

// forward + backward (+ Adam) after x is staged
static int train_body(iwae_handle* h, const Plan& P, const EpsSet& E, bool adam) {
  if (use_engine(h, P)) return engine_train_body(h, P, E, adam);
  // large batches: the output layer's forward (Bernoulli) and dX GEMMs on bf16x3
  // products of a split copy refreshed here, after the previous step's Adam
  h->step.out_x3 = h->x3 && h->tune.out_x3_rows > 0 && (long long)P.Bimg * P.kS >= h->tune.out_x3_rows;
  if (h->step.out_x3) CHK(run_wsplit_seg(h, h->o3));
  if (use_fused(h, P)) return fused_train_body(h, P, E, adam);
  CHK(forward_core(h, P, E, true));
  CHK(run_bound(h, P, true, -1.f, train_loss_ptr(h), adam));
  if (P.piwae) {
    CHK(decoder_bwd(h, P, h->dlw, h->dpx, true, false));      // decoder: IWAE_{k1 k2}
    CHK(decoder_bwd(h, P, h->dlw2, h->dpx2, false, true));    // encoder path: MIWAE(k1,k2) (DReG: softmax^2)
    CHK(encoder_bwd(h, P, h->dlw2));
  } else {
    CHK(decoder_bwd(h, P, h->dlw, h->dpx, true, true));
    CHK(encoder_bwd(h, P, h->dlw));
  }
  return finish_step(h, P, adam);
}

// The engine step's input Dense as the split-K GEMM (above the few-row
// launches' 32 images) reads the caller's x itself: a virtual ones column at
// x_dim (a multiple of 4 floats), and it fills x_in for the later readers.
static bool gemm_direct(const iwae_handle* h, const Plan& P) {
  return h->tune.x_direct && use_engine(h, P) && !smallm_ok(h, P.Bimg) && h->xdim % 4 == 0;
}

// re-point a captured input-layer launch at x
static hipError_t repoint_x(hipGraphExec_t exec, hipGraphNode_t node, const XLaunch& xa, const float* x) {
  hipKernelNodeParams kp;
  hipError_t e = hipGraphKernelNodeGetParams(node, &kp);
  if (e != hipSuccess) return e;
  SmArgs sa = xa.sm;
  GemmArgs ga = xa.gm;
  sa.A = x;
  ga.A = x;
  void* args[] = {xa.kind == 1 ? (void*)&ga : (void*)&sa};
  kp.kernelParams = args;
  kp.extra = nullptr;
  return hipGraphExecKernelNodeSetParams(exec, node, &kp);
}

// re-point step j's input-layer launch at the batch x + j * xstride, where it moved
static int repoint_batches(iwae_handle* h, GraphRec& g, const float* x, long long xstride) {
  for (size_t j = 0; j < g.xs_node.size(); ++j) {
    const float* xj = x + (long long)j * xstride;
    if (g.xs_cap[j] == xj) continue;
    HIPCHK(repoint_x(g.exec, g.xs_node[j], g.xs_args[j], xj));
    g.xs_cap[j] = xj;
  }
  return IWAE_OK;
}

// Graph key of a train-step graph: kind (0 forward_backward, 1 train step, 2
// multi-step), the loss config (p, alpha, beta by their bits) and the batch,
// with the kind's own entries (rest) before the float bits.
static std::vector<long long> graph_key(long long kind, const iwae_loss_config* lc, int B,
                                        std::initializer_list<long long> rest) {
  std::vector<long long> key = {kind, lc->loss, B, lc->k, lc->k1, lc->k2};
  key.insert(key.end(), rest);
  for (float f : {lc->p, lc->alpha, lc->beta}) {
    int bits;
    std::memcpy(&bits, &f, 4);
    key.push_back(bits);
  }
  return key;
}

// Capture body on the handle's stream into an executable graph stored under
// key (counted in n_captures, iwae_debug_count id 7).  body issues the work
// and fills the record's re-pointable nodes; when it or the capture fails no
// graph is left behind.
static int capture_graph(iwae_handle* h, const std::vector<long long>& key,
                         const std::function<int(GraphRec&)>& body, GraphRec** out) {
  GraphRec g;
  h->step.capturing = true;
  HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
  const int rc = body(g);
  const hipError_t ec = hipStreamEndCapture(h->stream, &g.graph);
  h->step.capturing = false;
  if (rc != IWAE_OK || ec != hipSuccess) {
    if (ec == hipSuccess) destroy_graph(g);
    if (rc != IWAE_OK) return rc;
    HIPCHK(ec);
  }
  hipError_t ei = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
  if (ei != hipSuccess) g.exec = nullptr;
  // the executable graph's device-side setup now (prepare_only included), not
  // inside the first replay of the call that is timed
  else ei = hipGraphUpload(g.exec, h->stream);
  if (ei != hipSuccess) {
    destroy_graph(g);
    HIPCHK(ei);
  }
  h->count.captures++;
  *out = &h->graphs.emplace(key, std::move(g)).first->second;
  return IWAE_OK;
}

// One train step inside a capture.  Where its first kernel reads the caller's
// x (x_user), that launch goes into the record for re-pointing.
static int capture_step(iwae_handle* h, const Plan& P, const EpsSet& E, bool adam, GraphRec& g) {
  h->step.cap_x_node = nullptr;
  CHK(train_body(h, P, E, adam));
  if (!h->step.x_user) return IWAE_OK;
  if (!h->step.cap_x_node) return fail(h, IWAE_EHIP, "train-step capture: input-layer launch not found");
  g.xs_node.push_back(h->step.cap_x_node);
  g.xs_args.push_back(h->step.cap_x_args);
  g.xs_cap.push_back(h->step.x_user);
  return IWAE_OK;
}

// What an engine step reads that must exist before it (and before a capture):
// current fragment-major copies (the step itself refreshes them after its
// Adam), the engine plans of this shape and the ring kernels' unit tables.
static int prepare_engine(iwae_handle* h, const Plan& P) {
  CHK(ensure_fx(h));
  CHK(tc_prepare(h, P));
  NrLaunch nr;
  NrbLaunch nb;
  NreLaunch ne;
  if (nring_plan(h, nr) && nrb_plan(h, nb) && h->L >= 2) {
    CHK(tc_prepare_one(h, P, TCL_BWD_NO_OUT));
    (void)nre_plan(h, ne);
  }
  return IWAE_OK;
}

// (mask: a pixel-masked step, [B][x_dim], non-zero = observed; null: none)
static int do_train(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
                    const float* const* eps, int n_eps, float* loss_dev, bool adam, const float* mask = nullptr) {
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (adam && h->dp_weighted && !h->comm)
    return fail(h, IWAE_EINVAL, "data parallel without a library communicator: call iwae_forward_backward, "
                                "all-reduce the gradient buffer, then iwae_apply_adam(h, 0)");
  Plan P;
  CHK(make_plan(h, lc, B, P));
  P.pix = mask ? 1 : 0;
  EpsSet E;
  CHK(parse_eps(h, P, eps, n_eps, E));
  CHK(ensure_capacity(h, P.Bimg, P.Bimg * P.kS, true, P.path != 0));
  const bool engine = use_engine(h, P);
  if (engine) CHK(prepare_engine(h, P));
  // the fused step's first kernel reads the caller's x itself (and fills x_in);
  // every other path stages x into x_in first.  A pixel-masked step always
  // stages (outside the captured region, like copy_x): no launch reads the
  // caller's x, so a replay needs no re-pointing for new x / mask buffers.
  const bool direct =
      !mask && P.Bimg == P.B && (((engine || use_fused(h, P)) && smallm_ok(h, P.Bimg)) || gemm_direct(h, P));
  if (mask) CHK(stage_masked(h, P, x, mask));
  else if (!direct) CHK(copy_x(h, P, x));
  StepScope scope{h};
  h->step.x_user = direct ? x : nullptr;
  const bool philox = (E.a[0] == nullptr);
  h->step.loss_out = loss_dev;
  h->step.in_train_step = true;
  if (!(h->use_graphs && philox && h->prof.kind < 0)) return train_body(h, P, E, adam);
  const auto key =
      graph_key(adam ? 1 : 0, lc, B, {(long long)(uintptr_t)loss_dev, direct ? 1 : 0, engine ? 1 : 0, P.pix});
  auto it = h->graphs.find(key);
  GraphRec* g = it == h->graphs.end() ? nullptr : &it->second;
  if (!g) CHK(capture_graph(h, key, [&](GraphRec& r) { return capture_step(h, P, E, adam, r); }, &g));
  CHK(repoint_batches(h, *g, x, 0));
  HIPCHK(hipGraphLaunch(g->exec, h->stream));
  // the replayed Adam moved the parameters: the split (bf16x3) copies the
  // evaluation paths read are stale from here (run_adam's bump only ran at capture)
  if (adam) {
    h->params_version++;
    if (engine) h->fx_version = h->params_version;   // the replayed step refreshed the fragment-major copies
  }
  return IWAE_OK;
}

static constexpr int kGraphSteps = 32;

// The graph of S consecutive steps from batch xi, captured on first use.
static int steps_graph(iwae_handle* h, const iwae_loss_config* lc, const Plan& P, const EpsSet& E, int B, int S,
                       const float* xi, GraphRec** out) {
  const auto key = graph_key(2, lc, B, {S, 1});
  auto it = h->graphs.find(key);
  if (it != h->graphs.end()) {
    *out = &it->second;
    return IWAE_OK;
  }
  return capture_graph(h, key, [&](GraphRec& g) -> int {
    for (int j = 0; j < S; ++j) {
      h->step.x_user = xi + j * (long long)B * h->xdim;
      h->step.loss_out = h->loss_slots + j;
      CHK(capture_step(h, P, E, true, g));
    }
    // the losses' copy as the graph's last node (a copy after the graph was a
    // launch of its own: +9 us gap and 4 us per call, profiles/r05q_train_step_timeline.txt);
    // captured into the no-losses sink, re-pointed per call
    g.loss_cap = h->loss_slots + kGraphSteps;
    if (hipMemcpyAsync(g.loss_cap, h->loss_slots, S * sizeof(float), hipMemcpyDeviceToDevice, h->stream) !=
            hipSuccess ||
        last_captured_node(h, &g.loss_node) != IWAE_OK)
      return fail(h, IWAE_EHIP, "multi-step capture: the losses' copy");
    if (!g.loss_node) return fail(h, IWAE_EHIP, "multi-step capture: the losses' copy node not found");
    return IWAE_OK;
  }, out);
}

// consecutive Philox train steps on the batches x + i * B * x_dim (fit's loop,
// E:82): graphs of up to kGraphSteps captured steps, so consecutive steps run
// without the per-graph launch gap; step j of a graph reads its own batch (its
// input-layer launch re-pointed when the batch moves) and writes its loss to
// loss_slots[j], copied to loss_dev + i by the graph's last node.  Data parallel with
// the library communicator: each captured step carries its all-reduces.
// Anything the multi-step graph does not cover (no graphs, staged x, data
// parallel without the library communicator, live profiling) runs as nsteps
// single steps.  prepare_only: capture every graph such a call uses (the
// lengths min(32, n) and n % 32) without launching anything, and leave the
// host's view of the parameters (versions) as it was.
static int do_train_steps(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, int nsteps,
                          float* loss_dev, bool prepare_only = false) {
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (nsteps < 0) return fail(h, IWAE_EINVAL, "nsteps must be >= 0");
  if (nsteps == 0) return IWAE_OK;
  const long long xstride = (long long)B * h->xdim;
  const bool multi = nsteps > 1 && h->use_graphs && h->prof.kind < 0 && (!h->dp_weighted || h->comm);
  // (single steps write the loss to the handle's scalar, then copy it: one
  // captured graph per shape, not one per loss address)
  auto single = [&]() -> int {
    if (prepare_only) return IWAE_OK;      // single steps capture on their first call
    for (int i = 0; i < nsteps; ++i) {
      CHK(do_train(h, lc, x + i * xstride, B, nullptr, 0, nullptr, true));
      if (loss_dev)
        HIPCHK(hipMemcpyAsync(loss_dev + i, &h->ds->scalars[0], sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    return IWAE_OK;
  };
  if (!multi) return single();
  Plan P;
  CHK(make_plan(h, lc, B, P));
  EpsSet E;
  CHK(parse_eps(h, P, nullptr, 0, E));
  CHK(ensure_capacity(h, P.Bimg, P.Bimg * P.kS, true, P.path != 0));
  const bool engine = use_engine(h, P);
  // (the engine step refreshes every copy it reads inside the step; other
  // paths decide their split-copy refreshes on the host at capture time)
  const bool direct = P.Bimg == P.B && ((engine && smallm_ok(h, P.Bimg)) || gemm_direct(h, P));
  if (!direct) return single();
  CHK(prepare_engine(h, P));
  if (!h->loss_slots) HIPCHK(hipMalloc(&h->loss_slots, 2 * kGraphSteps * sizeof(float)));
  StepScope scope{h};
  h->step.in_train_step = true;
  const long long pv = h->params_version, wv = h->wsplit_version, fv = h->fx_version;
  for (int i0 = 0, S = 0; i0 < nsteps; i0 += S) {
    S = std::min(kGraphSteps, nsteps - i0);
    const float* xi = x + i0 * xstride;
    GraphRec* gp = nullptr;
    CHK(steps_graph(h, lc, P, E, B, S, xi, &gp));
    if (prepare_only) {
      // a capture bumps the host's parameter versions as if it had run: undo
      h->params_version = pv;
      h->wsplit_version = wv;
      h->fx_version = fv;
      continue;
    }
    GraphRec& g = *gp;
    CHK(repoint_batches(h, g, xi, xstride));
    float* ldst = loss_dev ? loss_dev + i0 : h->loss_slots + kGraphSteps;
    if (g.loss_cap != ldst) {
      HIPCHK(hipGraphExecMemcpyNodeSetParams1D(g.exec, g.loss_node, ldst, h->loss_slots, S * sizeof(float),
                                               hipMemcpyDeviceToDevice));
      g.loss_cap = ldst;
    }
    HIPCHK(hipGraphLaunch(g.exec, h->stream));
    h->params_version++;
    h->fx_version = h->params_version;   // every replayed step refreshed the fragment-major copies
  }
  return IWAE_OK;
}

// Tail of the three ring planners: the unit table uploaded once (device,
// built once: FX / GX offsets are fixed per model) and the launch pointed at
// it and at the fragment-major copies.
template <class Launch>
static bool ring_plan_tail(iwae_handle* h, NrUnit*& dev, int cap, const std::vector<NrUnit>& units, Launch& R) {
  if (!dev) {
    if (hipMalloc(&dev, cap * sizeof(NrUnit)) != hipSuccess) return false;
    if (hipMemcpy(dev, units.data(), units.size() * sizeof(NrUnit), hipMemcpyHostToDevice) != hipSuccess)
      return false;
  }
  R.units = dev;
  R.fx_hi = h->fx_hi; R.fx_lo = h->fx_lo;
  R.fx_bytes = (unsigned)(h->fx_elems * (long long)sizeof(__bf16));
  return true;
}

// ------------------------------------------------ evaluation entries: shared host code
// What iwae_nll, iwae_posterior / iwae_impute, iwae_score, iwae_score_grad and
// iwae_encode share: the argument checks, the chunk rule, the walk over chunks
// and first-layer groups, the per-chunk launch fields and the layer-wise blocks.

// a[0 .. L-1], one buffer per stochastic layer, none null (optional: or n == 0)
static int ptrs_ok(iwae_handle* h, const float* const* a, int n, const char* what, bool optional) {
  if (optional && n == 0) return IWAE_OK;
  if (n != h->L || !a)
    return fail(h, IWAE_EINVAL, std::string("expected ") + std::to_string(h->L) + " " + what + " buffers (one per "
                                "stochastic layer), got " + std::to_string(n));
  for (int i = 0; i < h->L; ++i)
    if (!a[i]) return fail(h, IWAE_EINVAL, std::string("NULL ") + what + " buffer");
  return IWAE_OK;
}

// rows of x_dim floats the kernels store as float4 (ld <= 2^22: a workgroup's
// 64 rows stay within 32-bit buffer offsets); p null: nothing to check
static int ld_ok(iwae_handle* h, const float* p, int ld, const char* what) {
  if (p && (ld < h->xdim || ld > (1 << 22) || (ld & 3) || ((uintptr_t)p & 15)))
    return fail(h, IWAE_EINVAL, std::string(what) + " needs x_dim <= ld <= 2^22, a multiple of 4, 16-byte aligned");
  return IWAE_OK;
}

// N images of k samples each; whole_k: all k of an image go through one chunk, which bounds k
static int nk_ok(iwae_handle* h, int N, int k, bool whole_k = true) {
  if (N <= 0 || k <= 0) return fail(h, IWAE_EINVAL, "N and k must be positive");
  if (whole_k && k > (1 << 20)) return fail(h, IWAE_EINVAL, "k above 2^20 per image is not supported");
  return IWAE_OK;
}

// At most 256 MB of what a chunk keeps per sample row (row_bytes each), at least one image
static int cap_chunk_bytes(int imgs, int k, long long row_bytes) {
  return (int)std::min<long long>(imgs, std::max<long long>(1, (256LL << 20) / (k * row_bytes)));
}

// Images per chunk: the caller's chunk, else IWAE_KNOB_NLL_IMGS, else
// floor(nll_rows / k), at least 1 and at most N; with row_bytes (what a chunk
// keeps per sample row) at most 256 MB of those.  whole_k: a chunk holds all k
// samples of its images, which bounds k and the chunk's rows (iwae_nll splits
// the samples instead).  0 with the error set.
static int chunk_images(iwae_handle* h, int N, int k, int chunk, bool whole_k = true, long long row_bytes = 0) {
  if (nk_ok(h, N, k, whole_k) != IWAE_OK) return 0;
  if (chunk <= 0) chunk = h->tune.nll_imgs;
  // (k above nll_rows: one image; rows past what an int holds ask for no more images than N can give)
  const long long target_rows = std::max<long long>(std::min<long long>(h->tune.nll_rows, INT_MAX), k);
  int imgs = chunk > 0 ? chunk : (int)std::max<long long>(1, target_rows / k);
  if (row_bytes > 0) imgs = cap_chunk_bytes(imgs, k, row_bytes);
  imgs = std::min(imgs, N);
  if (whole_k && (long long)imgs * k > (1LL << 30)) { fail(h, IWAE_EINVAL, "chunk * k above 2^30 sample rows"); return 0; }
  return imgs;
}

// ng images from row i0 on into x_in: a copy, or with a pixel mask the two
// staged copies by select (x_in = mask ? x : 0, lik = mask ? x : -1;
// impute_stage_kernel; lik.p null: the first alone).
static int stage_x(iwae_handle* h, const float* x, const float* mask, int i0, int ng, const Mat& lik = Mat()) {
  x += (size_t)i0 * h->xdim;
  if (mask) {
    HIPCHK(launch_impute_stage(h->stream, x, mask + (size_t)i0 * h->xdim, ng, h->xdim, h->x_in.p, h->x_in.ld, lik.p,
                               lik.ld));
    return IWAE_OK;
  }
  const size_t wbytes = (size_t)h->xdim * sizeof(float);
  HIPCHK(hipMemcpy2DAsync(h->x_in.p, (size_t)h->x_in.ld * sizeof(float), x, wbytes, wbytes, ng, hipMemcpyDeviceToDevice,
                          h->stream));
  return IWAE_OK;
}

// The walk of an evaluation call over its N images: chunks of imgs images
// (one set of launches each) inside groups of sup images, staged into x_in
// together.  Fused, a group is up to IWAE_KNOB_NLL_GROUP images and (enc0) the
// first encoder layer runs once per group -- three GEMM launches and the copy
// of x per ~16 K images instead of per chunk (k = 5000: 78 chunks of 209 images;
// the per-chunk launches were ~2 % of the NLL's time) -- and the fused kernels
// read each chunk's rows of eb[0].P and x_in.  Layer-wise a group is a chunk.
//   for (ChunkWalk W(h, ...); W.i0 < N; W.i0 += W.imgs) { CHK(walk_step(h, W)); ... }
struct ChunkWalk {
  int N, k, imgs, sup;
  bool fused, enc0;
  const float *x, *mask;             // (x null: a call that needs no images; nothing is staged)
  const Mat* lik;                    // masked: where the likelihood's -1 copy is staged (read at each group)
  // the chunk, set by walk_step: images [i0, i0 + n), rows io .. of x_in / eb[0], rows r0 .. of [N][k] outputs
  int i0 = 0, n = 0, io = 0, u0 = 0;
  size_t r0 = 0;
  ChunkWalk(const iwae_handle* h, int N_, int k_, int imgs_, bool fused_, const float* x_, const float* mask_, bool enc0_,
            const Mat* lik_ = nullptr)
      : N(N_), k(k_), imgs(imgs_), sup(fused_ ? std::min(N_, imgs_ * std::max(1, h->tune.nll_group / imgs_)) : imgs_),
        fused(fused_), enc0(enc0_), x(x_), mask(mask_), lik(lik_ ? lik_ : &h->x_lik) {}
};

static int walk_step(iwae_handle* h, ChunkWalk& W) {
  W.n = std::min(W.imgs, W.N - W.i0);
  W.r0 = (size_t)W.i0 * W.k;
  if (W.x && (W.i0 == 0 || W.i0 - W.u0 >= W.sup)) {          // a new group (layer-wise: every chunk)
    W.u0 = W.i0;
    const int ng = std::min(W.sup, W.N - W.i0);
    CHK(stage_x(h, W.x, W.mask, W.i0, ng, *W.lik));
    if (W.enc0) CHK(stoch_fwd(h, h->enc[0], h->x_in, ng, h->eb[0]));
  }
  W.io = W.x ? W.i0 - W.u0 : 0;
  return IWAE_OK;
}

// The launch fields of the chunk's rows that MgLaunch, ScLaunch and SgLaunch
// share: kS samples of each image, the first encoder layer's output rows and
// the likelihood's copy xl of the images.
template <class Launch>
static void chunk_rows(const iwae_handle* h, const ChunkWalk& W, int kS, const Mat& xl, Launch& A) {
  A.rows = W.n * kS; A.kS = kS;
  A.P0 = h->eb[0].P.p + (size_t)W.io * h->eb[0].P.ld; A.ldP0 = h->eb[0].P.ld;
  A.x = xl.p + (size_t)W.io * xl.ld; A.ldx = xl.ld;
}

// mega_fwd_kernel's plan and, where its shapes apply, nring_kernel's: the
// fused k-sample forward of iwae_nll and of iwae_posterior's first pass.
struct FwdPlan {
  MgLaunch MG;
  NrLaunch NR;
  int rt = 0, waves = 8;
  size_t lds = 0;
  bool ring = false;
};

// The noise (the caller's eps [k][N][d_i], or null: Philox) and log-weight
// fields of a call's launches, after ensure_capacity.
static void fwd_call_fields(const iwae_handle* h, FwdPlan& F, const float* const* eps, int N) {
  for (int i = 0; i < 8; ++i) F.MG.eps[i] = F.NR.eps[i] = (eps && i < h->L) ? eps[i] : nullptr;
  F.MG.eps_N = F.NR.eps_N = N;
  F.MG.seed = h->seed; F.MG.rng_base = &h->ds->rng[0];
  F.MG.lw = h->lw;
}

// Samples [s0, s0 + P.kS) of the chunk's images: the weight-ring kernel where it
// is planned and P.kS >= 128 (same rows, same noise; 128 rows per workgroup span
// at most two images), else mega_fwd_kernel.
static int launch_fwd_chunk(iwae_handle* h, FwdPlan& F, const ChunkWalk& W, const Plan& P, int s0, bool injected) {
  MgLaunch& MG = F.MG;
  chunk_rows(h, W, P.kS, h->x_in, MG);
  MG.eps_i0 = W.i0; MG.eps_s0 = s0;
  if (F.ring && P.kS >= 128) {
    NrLaunch& NR = F.NR;
    NR.rows = MG.rows; NR.kS = MG.kS; NR.eps_i0 = W.i0; NR.eps_s0 = s0;
    NR.P0 = MG.P0; NR.ldP0 = MG.ldP0; NR.x = MG.x; NR.ldx = MG.ldx;
    NR.seed = MG.seed; NR.rng_base = MG.rng_base; NR.lw = MG.lw;
    HIPCHK(launch_nring(h->stream, NR));
    ++h->count.nring;
  } else {
    HIPCHK(launch_mega_fwd(h->stream, MG, F.rt, F.waves, F.lds));
  }
  ++h->count.mega;
  if (injected) ++h->count.mega_eps;
  return IWAE_OK;
}

// launch_lse's arguments for kS samples of n images (init: the first samples
// of these images) from the workspace's logp / logq and Bernoulli partials; a
// fused forward's caller points lw at its log weights instead
static LseArgs lse_args(const iwae_handle* h, int kS, int n, bool init) {
  LseArgs a{};
  a.part = h->part; a.ldpart = h->ldpart; a.npart = h->npart; a.logp = h->logp; a.logq = h->logq;
  a.kS = kS; a.Bimg = n; a.run_m = h->run_m; a.run_s = h->run_s; a.init = init;
  a.ticket = &h->ds->tickets[1]; a.rng_base = &h->ds->rng[0];
  return a;
}

// Layer-wise injected noise of the chunk: the caller's buffers [k][N][d_i], or
// (gather: a chunk of a longer call) sample s of the chunk's images, n * d
// floats at (s * N + i0) * d, copied contiguous to ws + o_eps[i] as [k][n][d_i].
static int chunk_eps(iwae_handle* h, const ChunkWalk& W, const float* const* eps, bool gather, float* ws,
                     const size_t* o_eps, EpsSet& E) {
  std::memset(&E, 0, sizeof(E));
  for (int i = 0; eps && i < h->L; ++i) {
    E.a[i] = eps[i];
    if (!gather) continue;
    const int d = h->enc[i].d;
    const size_t rb = (size_t)W.n * d * sizeof(float);
    HIPCHK(hipMemcpy2DAsync(ws + o_eps[i], rb, eps[i] + (size_t)W.i0 * d, (size_t)W.N * d * sizeof(float), rb, W.k,
                            hipMemcpyDeviceToDevice, h->stream));
    E.a[i] = ws + o_eps[i];
  }
  return IWAE_OK;
}

// The caller's latents lat[i] [k][N][d_i] of the chunk's images into the rows of h[i]
static int gather_latents(iwae_handle* h, const ChunkWalk& W, const float* const* lat) {
  ScRelayout G{};
  G.n = W.n; G.k = W.k; G.N = W.N; G.i0 = W.i0; G.gather = 1;
  for (int i = 0; i < h->L; ++i)
    G.seg[G.nseg++] = ScSeg{h->h[i].p, h->h[i].ld, 0, h->enc[i].d, const_cast<float*>(lat[i]), 0, 0};
  HIPCHK(launch_score_relayout(h->stream, G));
  return IWAE_OK;
}

// One Gaussian log-density pass: rows of H (d wide) under the (mu | zs) rows of
// P, row r's at P[r / prow_div], into out (accumulate: added to it)
static int gauss_logdens(iwae_handle* h, const Mat& P, int prow_div, int d, const Mat& H, float* out, bool accumulate,
                         int M) {
  GaussArgs g{};
  g.P = P.p; g.ldP = P.ld; g.prow_div = prow_div; g.d = d;
  g.H = H.p; g.ldH = H.ld;
  g.out = out; g.accumulate = accumulate; g.M = M;
  HIPCHK(launch_gauss_fwd(h->stream, 1, g));
  return IWAE_OK;
}

// The output MLP's hidden layers of M rows of h[0] into ob.y1, ob.y2
static int out_hidden(iwae_handle* h, int M) {
  CHK(gemm_fwd(h, EPI_TANH, h->h[0], M, h->dense[h->o1], h->ob.y1));
  return gemm_fwd(h, EPI_TANH, h->ob.y1, M, h->dense[h->o2], h->ob.y2);
}

// ... and its output Dense: the logits of those rows into p, turned into probabilities in place
static int out_probs(iwae_handle* h, int M, float* p, int ld) {
  Mat pm;
  pm.p = p; pm.ld = ld;
  CHK(gemm_fwd(h, EPI_STORE, h->ob.y2, M, h->dense[h->o3], pm));
  HIPCHK(launch_bern_probs(h->stream, p, M, h->xdim, ld));
  return IWAE_OK;
}

// The Bernoulli epilogue's arguments for log p(x | h_1) of rows that belong k
// to an image of xl, weighted wa
static GemmArgs bern_args(const iwae_handle* h, const Mat& xl, int k, float wa) {
  GemmArgs ex{};
  ex.aux = xl.p; ex.ldaux = xl.ld; ex.x_row_div = k;
  ex.part = h->part; ex.part2 = h->part2; ex.ldpart = h->ldpart;
  ex.wa = wa; ex.wb = 0.f;
  return ex;
}

// ---------------------------------------------------------------- ABI
extern "C" {

iwae_handle* iwae_create(const iwae_config* cfg, int device) {
  g_create_error.clear();
  if (!cfg) { g_create_error = "config is NULL"; return nullptr; }
  const int L = cfg->n_stochastic;
  if (L < 1 || L > IWAE_MAX_LAYERS) { g_create_error = "n_stochastic must be in [1, 8]"; return nullptr; }
  if (cfg->x_dim <= 0) { g_create_error = "x_dim must be positive"; return nullptr; }
  for (int i = 0; i < L; ++i) {
    if (cfg->n_hidden_encoder[i] <= 0 || cfg->n_latent_encoder[i] <= 0 || cfg->n_hidden_decoder[i] <= 0) {
      g_create_error = "layer sizes must be positive";
      return nullptr;
    }
  }
  for (int i = 0; i < L - 1; ++i) {
    if (cfg->n_latent_decoder[i] != cfg->n_latent_encoder[L - 2 - i]) {
      g_create_error = "n_latent_decoder[" + std::to_string(i) + "] must equal n_latent_encoder[" +
                       std::to_string(L - 2 - i) + "]";
      return nullptr;
    }
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_create_error = "hipSetDevice failed (no GPU?)";
    return nullptr;
  }
  iwae_handle* h = new iwae_handle();
  h->device = device;
  h->cfg = *cfg;
  h->L = L;
  h->xdim = cfg->x_dim;
  // encoder stochastic layers (F:48-F:49), decoder prior layers (F:86-F:87), output MLP (F:89-F:96)
  for (int i = 0; i < L; ++i) {
    const int fin = i == 0 ? cfg->x_dim : cfg->n_latent_encoder[i - 1];
    h->enc.push_back(add_stoch(h, fin, cfg->n_hidden_encoder[i], cfg->n_latent_encoder[i], i == 0 ? 0 : 1));
  }
  for (int i = 0; i < L - 1; ++i) {
    h->dec.push_back(add_stoch(h, cfg->n_latent_encoder[L - 1 - i], cfg->n_hidden_decoder[i],
                               cfg->n_latent_decoder[i], 1));
  }
  const int Hd = cfg->n_hidden_decoder[L - 1];
  h->o1 = add_dense(h, cfg->n_latent_encoder[0], Hd, 1);
  h->o2 = add_dense(h, Hd, Hd, 1);
  h->o3 = add_dense(h, Hd, cfg->x_dim, 1);
  h->keras.push_back({h->o1, 0, Hd});
  h->keras.push_back({h->o2, 0, Hd});
  h->keras.push_back({h->o3, 0, cfg->x_dim});
  for (auto& k : h->keras) h->nparam_keras += (long long)(h->dense[k.di].fin + 1) * k.width;
  for (auto& d : h->dense) {
    const int nf = d.head_d > 0 ? 8 * ((d.head_d + 3) / 4) : d.fout;
    d.fx_tiles = (nf + 15) / 16; d.fx_steps = d.ldF / 32;
    d.gx_tiles = (d.fin + 15) / 16; d.gx_steps = d.ldG / 32;
    d.fx_off = h->fx_elems;
    h->fx_elems += (long long)d.fx_tiles * d.fx_steps * 64 * 8;
    d.gx_off = h->fx_elems;
    h->fx_elems += (long long)d.gx_tiles * d.gx_steps * 64 * 8;
  }
  hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
  h->stream = h->own_stream;
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_mid, hipEventDisableTiming);
  const size_t pb = (size_t)h->nparam_int * sizeof(float);
  // the row-block kernels fetch whole padded k ranges (up to 255 rows, or 256
  // floats of a row, past a matrix's end): keep that inside a zeroed tail
  int max_ldw = 4;
  for (const auto& d : h->dense) max_ldw = std::max(max_ldw, d.ldw);
  h->params_bytes = pb + (size_t)(256 * max_ldw + 256) * sizeof(float);
  if (e == hipSuccess) e = hipMalloc(&h->params, h->params_bytes);
  if (e == hipSuccess) e = hipMalloc(&h->adam_m, pb);
  if (e == hipSuccess) e = hipMalloc(&h->adam_v, pb);
  if (e == hipSuccess) e = hipMalloc(&h->grad_own, pb + 4 * sizeof(float));   // + the DP batch-size tail
  if (e == hipSuccess) e = hipMalloc(&h->ds, sizeof(DevState));
  if (e == hipSuccess) e = hipMalloc(&h->tcu_ctr, 8 * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(h->tcu_ctr, 0, 8 * sizeof(unsigned));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->err_host, 64, hipHostMallocMapped);
  if (e == hipSuccess) { *(volatile unsigned*)h->err_host = 0u; e = hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0); }
  if (e == hipSuccess) e = hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = hipMalloc(&h->wsplit_hi, (size_t)(2 * h->wsplit_elems) * sizeof(__bf16));
  if (e == hipSuccess) e = hipMalloc(&h->fx_hi, (size_t)(2 * h->fx_elems) * sizeof(__bf16));
  if (e == hipSuccess) e = hipMemset(h->fx_hi, 0, (size_t)(2 * h->fx_elems) * sizeof(__bf16));
  if (e == hipSuccess) e = hipMemset(h->wsplit_hi, 0, (size_t)(2 * h->wsplit_elems) * sizeof(__bf16));
  if (e == hipSuccess) e = hipMemset(h->params, 0, h->params_bytes);
  if (e == hipSuccess) e = hipMemset(h->adam_m, 0, pb);
  if (e == hipSuccess) e = hipMemset(h->adam_v, 0, pb);
  if (e == hipSuccess) e = hipMemset(h->grad_own, 0, pb + 4 * sizeof(float));
  if (e == hipSuccess) {
    DevState s{};
    s.adam.lr = 1e-3f; s.adam.b1 = 0.9f; s.adam.b2 = 0.999f; s.adam.eps = 1e-7f;  // Keras defaults
    s.adam.grad_scale = 1.f; s.adam.t = 0;
    e = hipMemcpy(h->ds, &s, sizeof(s), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    g_create_error = std::string("device allocation failed: ") + hipGetErrorString(e);
    iwae_destroy(h);
    return nullptr;
  }
  h->grad = h->grad_own;
  h->wsplit_lo = h->wsplit_hi + h->wsplit_elems;
  h->fx_lo = h->fx_hi + h->fx_elems;
  e = rb_setup_attributes();
  if (e == hipSuccess) e = mega_setup_attributes();
  if (e == hipSuccess) e = score_setup_attributes();
  if (e == hipSuccess) e = sgrad_setup_attributes();
  if (e == hipSuccess) e = nring_setup_attributes();
  if (e == hipSuccess) e = smallm_setup_attributes();
  if (e == hipSuccess) e = tc_setup_attributes();
  if (e == hipSuccess) e = upd_setup_attributes();
  if (e == hipSuccess) e = dw_setup_attributes();
  if (e == hipSuccess) e = gen_setup_attributes();
  if (e == hipSuccess) e = post_setup_attributes();
  if (e != hipSuccess) {
    g_create_error = std::string("hipFuncSetAttribute failed: ") + hipGetErrorString(e);
    iwae_destroy(h);
    return nullptr;
  }
  return h;
}

const char* iwae_create_error(void) { return g_create_error.c_str(); }

void iwae_destroy(iwae_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_workspace(h);
  if (h->comm) (void)ncclCommDestroy(h->comm);
  for (auto e : h->prof.ev) (void)hipEventDestroy(e);
  if (h->params) (void)hipFree(h->params);
  if (h->adam_m) (void)hipFree(h->adam_m);
  if (h->adam_v) (void)hipFree(h->adam_v);
  if (h->grad_own) (void)hipFree(h->grad_own);
  if (h->ds) (void)hipFree(h->ds);
  if (h->tcu_ctr) (void)hipFree(h->tcu_ctr);
  if (h->err_host) (void)hipHostFree(h->err_host);
  if (h->loss_slots) (void)hipFree(h->loss_slots);
  for (GrowWs* w : {&h->post_ws, &h->sg_ws, &h->ais_ws, &h->refine_ws, &h->ws_ws, &h->agg_ws})
    if (w->p) (void)hipFree(w->p);
  if (h->nr_units) (void)hipFree(h->nr_units);
  if (h->nrb_units) (void)hipFree(h->nrb_units);
  if (h->nre_units) (void)hipFree(h->nre_units);
  if (h->wsplit_hi) (void)hipFree(h->wsplit_hi);
  if (h->fx_hi) (void)hipFree(h->fx_hi);
  if (h->prof.scratch) (void)hipFree(h->prof.scratch);
  if (h->prof.adam) (void)hipFree(h->prof.adam);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
  delete h;
}

const char* iwae_last_error(const iwae_handle* h) { return h ? h->err.c_str() : "NULL handle"; }

int iwae_set_stream(iwae_handle* h, void* s) {
  if (!h) return IWAE_EINVAL;
  h->stream = s ? (hipStream_t)s : h->own_stream;
  return IWAE_OK;
}

// A kernel-reported failure (an in-launch wait of the combined image-row
// backward + update launch that gave up: that step's gradients were computed
// from stale job-I' outputs).  Sticky until iwae_set_params.
static int kernel_status(iwae_handle* h) {
  if (h->err_host && *(volatile unsigned*)h->err_host)
    return fail(h, IWAE_EHIP, "tcu_kernel: an in-launch wait for the first encoder layer's image-row backward gave "
                              "up; the weight gradients and Adam update of that train step are invalid "
                              "(reload the parameters)");
  return IWAE_OK;
}

int iwae_synchronize(iwae_handle* h) {
  if (!h) return IWAE_EINVAL;
  HIPCHK(hipStreamSynchronize(h->stream));
  return kernel_status(h);
}

int iwae_status(iwae_handle* h) {
  if (!h) return IWAE_EINVAL;
  return kernel_status(h);
}

static uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// The Philox key of the handle's current noise stream, and the device counter
// position: each stream keeps its own position (saved / restored on a switch),
// so switching back to a stream never replays its noise, and re-selecting the
// current stream is a no-op (a data-parallel loop that evaluates with the
// sharded NLL between steps keeps drawing fresh noise).
static void derive_key(iwae_handle* h) {
  h->seed = h->noise_stream == 0 ? h->user_seed : splitmix64(h->user_seed ^ splitmix64(h->noise_stream));
  invalidate_graphs(h);                  // the key is a captured kernel argument
}

int iwae_set_noise_stream(iwae_handle* h, unsigned long long stream) {
  if (!h) return IWAE_EINVAL;
  if (stream == h->noise_stream) return IWAE_OK;
  uint64_t z[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(z, h->ds->rng, sizeof(z), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->stream_pos[h->noise_stream] = z[0];
  auto it = h->stream_pos.find(stream);
  z[0] = it == h->stream_pos.end() ? 0 : it->second;
  z[1] = 0;
  h->noise_stream = stream;
  derive_key(h);
  HIPCHK(hipMemcpyAsync(h->ds->rng, z, sizeof(z), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return IWAE_OK;
}

int iwae_set_seed(iwae_handle* h, unsigned long long seed) {
  if (!h) return IWAE_EINVAL;
  h->user_seed = seed;
  derive_key(h);
  h->stream_pos.clear();                 // every stream restarts from counter 0
  uint64_t z[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h->ds->rng, z, sizeof(z), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return IWAE_OK;
}

int iwae_set_path(iwae_handle* h, int path) {
  if (!h) return IWAE_EINVAL;
  if (path < 0 || path > 3)
    return fail(h, IWAE_EINVAL, "path must be 0 (auto), 1 (layer-wise), 2 (fused row-block) or 3 (engine)");
  h->path = path;
  h->nll_fused = path != 1;             // layer-wise everywhere when asked for
  invalidate_graphs(h);
  return IWAE_OK;
}

int iwae_set_precision(iwae_handle* h, int mode) {
  if (!h) return IWAE_EINVAL;
  if (mode != 0 && mode != 1) return fail(h, IWAE_EINVAL, "precision must be 0 (f32 MFMA) or 1 (bf16x3)");
  h->x3 = mode;
  invalidate_graphs(h);
  return IWAE_OK;
}

int iwae_set_graphs(iwae_handle* h, int enable) {
  if (!h) return IWAE_EINVAL;
  h->use_graphs = enable != 0;
  return IWAE_OK;
}

int iwae_set_tuning(iwae_handle* h, int knob, long long value) {
  if (!h) return IWAE_EINVAL;
  const bool on = value != 0;
  // kernels already queued on the handle's stream may still read the arena and
  // the plan tables that some knobs free below
  HIPCHK(hipStreamSynchronize(h->stream));
  switch (knob) {
    case IWAE_KNOB_ENGINE: h->tune.engine = on; break;
    case IWAE_KNOB_TC_IMG: h->tune.engine_img = on; break;
    case IWAE_KNOB_TC_IMGBWD: h->tune.engine_img_bwd = on; break;
    case IWAE_KNOB_TC_FOLD0: h->tune.engine_fold0 = on; break;
    case IWAE_KNOB_TC_XCD: h->tune.tc_xcd = on; break;
    case IWAE_KNOB_TC_BOUND: h->tune.tc_bound = on; break;
    case IWAE_KNOB_TC_RT:
      if (value != 1 && value != 2 && value != 4) return fail(h, IWAE_EINVAL, "TC_RT must be 1, 2 or 4");
      h->tune.tc_rt = (int)value;
      break;
    case IWAE_KNOB_UPD: h->tune.upd = on; break;
    case IWAE_KNOB_TCU_WAIT_TEST: h->tune.tcu_wait_test = on; break;
    case IWAE_KNOB_TCU_WT: h->tune.tcu_wt = on; break;
    case IWAE_KNOB_UPD_ROWS: h->tune.upd_rows = std::max(0LL, value); break;
    case IWAE_KNOB_UPD_SLABS: h->tune.upd_slabs = on; break;
    case IWAE_KNOB_UPD_SLAB_WG: h->tune.upd_slab_wg = std::max(1LL, value); break;
    case IWAE_KNOB_DW_TARGET:
      h->tune.dw_target = std::max(1LL, value);
      free_workspace(h);                 // the slab layout depends on it
      break;
    case IWAE_KNOB_SMALLM_ROWS: h->tune.smallm_rows = (int)std::max(0LL, std::min(value, 32LL)); break;
    case IWAE_KNOB_OUT_X3_ROWS: h->tune.out_x3_rows = std::max(0LL, value); break;
    case IWAE_KNOB_MG_WAVES:
      if (value != 4 && value != 8) return fail(h, IWAE_EINVAL, "MG_WAVES must be 4 or 8");
      h->tune.mg_waves = (int)value;
      break;
    case IWAE_KNOB_NLL_ROWS: h->tune.nll_rows = std::max(1LL, value); break;
    case IWAE_KNOB_NLL_IMGS: h->tune.nll_imgs = (int)std::max(0LL, std::min(value, 1LL << 20)); break;
    case IWAE_KNOB_NLL_GROUP: h->tune.nll_group = (int)std::max(1LL, std::min(value, 1LL << 20)); break;
    case IWAE_KNOB_WIDE_ROWS: h->tune.wide_rows = std::max(0LL, value); break;
    case IWAE_KNOB_DW_WIDE: h->tune.dw_wide = on; break;
    case IWAE_KNOB_DW_WG: h->tune.dw_wg = (int)std::max(8LL, std::min(value, 4096LL)); break;
    case IWAE_KNOB_PIWAE_ONE: h->tune.piwae_one = on; break;
    case IWAE_KNOB_DW_ALPHA: h->tune.dw_alpha = (int)std::max(0LL, std::min(value, 1000LL)); break;
    case IWAE_KNOB_IMG_ROWS_FWD: h->tune.img_rows_fwd = (int)std::max(0LL, std::min(value, 16LL)); break;
    case IWAE_KNOB_IMG_ROWS_BWD: h->tune.img_rows_bwd = (int)std::max(0LL, std::min(value, 16LL)); break;
    case IWAE_KNOB_X_DIRECT: h->tune.x_direct = on; break;
    case IWAE_KNOB_TCU: h->tune.tcu = on; break;
    case IWAE_KNOB_UPD_APPLY: h->tune.upd_apply = on; break;
    case IWAE_KNOB_NRING: h->tune.nring = on; break;
    case IWAE_KNOB_NRING_TRAIN: h->tune.nring_train = on; break;
    case IWAE_KNOB_NRING_TRAIN_ROWS: h->tune.nr_train_rows = std::max(0LL, value); break;
    case IWAE_KNOB_NRING_BWD: h->tune.nring_bwd = (int)std::min<long long>(std::max(0LL, value), 3); break;
    case IWAE_KNOB_UPD_WAVES: h->tune.upd_waves = value == 4 ? 4 : value >= 16 ? 16 : 8; break;
    case IWAE_KNOB_WIDE_RT: h->tune.wide_rt = value >= 4 ? 4 : value <= 1 ? 1 : 2; break;
    case IWAE_KNOB_LD_ALIGN:
      if (value != 4 && value != 8 && value != 16 && value != 32)
        return fail(h, IWAE_EINVAL, "LD_ALIGN must be 4, 8, 16 or 32");
      h->tune.ld_align = (int)value;
      free_workspace(h);
      break;
    default: return fail(h, IWAE_EINVAL, "unknown tuning knob " + std::to_string(knob));
  }
  // captured steps and engine plans were built for the previous setting
  invalidate_graphs(h);
  invalidate_tc_plans(h);
  return IWAE_OK;
}

int iwae_set_store_policy(iwae_handle* h, int mask) {
  if (!h) return IWAE_EINVAL;
  if (mask < 0 || mask > 63) return fail(h, IWAE_EINVAL, "store policy: a mask of bits 1 .. 32");
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tune.st_wt = mask;
  // captured steps and engine plans were built for the previous setting
  invalidate_graphs(h);
  invalidate_tc_plans(h);
  return IWAE_OK;
}

long long iwae_num_params(const iwae_handle* h) { return h ? h->nparam_keras : -1; }

static void keras_to_internal(const iwae_handle* h, const float* src, std::vector<float>& dst) {
  dst.assign((size_t)h->nparam_int, 0.f);
  long long o = 0;
  for (const auto& k : h->keras) {
    const DenseL& d = h->dense[k.di];
    for (int r = 0; r < d.fin; ++r)
      for (int j = 0; j < k.width; ++j) dst[d.off + (long long)r * d.ldw + k.col0 + j] = src[o++];
    for (int j = 0; j < k.width; ++j) dst[d.off + (long long)d.fin * d.ldw + k.col0 + j] = src[o++];
  }
}

static void internal_to_keras(const iwae_handle* h, const std::vector<float>& src, float* dst) {
  long long o = 0;
  for (const auto& k : h->keras) {
    const DenseL& d = h->dense[k.di];
    for (int r = 0; r < d.fin; ++r)
      for (int j = 0; j < k.width; ++j) dst[o++] = src[d.off + (long long)r * d.ldw + k.col0 + j];
    for (int j = 0; j < k.width; ++j) dst[o++] = src[d.off + (long long)d.fin * d.ldw + k.col0 + j];
  }
}

static int check_n(iwae_handle* h, long long n, const void* p) {
  if (!h) return IWAE_EINVAL;
  if (!p) return fail(h, IWAE_EINVAL, "NULL host buffer");
  if (n != h->nparam_keras)
    return fail(h, IWAE_EINVAL, "expected " + std::to_string(h->nparam_keras) + " parameters, got " +
                                   std::to_string(n));
  return IWAE_OK;
}

static int upload(iwae_handle* h, float* dev, const float* host) {
  std::vector<float> tmp;
  keras_to_internal(h, host, tmp);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dev, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice));
  return IWAE_OK;
}

static int download(iwae_handle* h, const float* dev, float* host) {
  std::vector<float> tmp((size_t)h->nparam_int);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
  internal_to_keras(h, tmp, host);
  return IWAE_OK;
}

int iwae_set_params(iwae_handle* h, const float* host, long long n) {
  CHK(check_n(h, n, host));
  CHK(upload(h, h->params, host));
  h->params_version++;
  if (h->err_host) *(volatile unsigned*)h->err_host = 0u;   // (upload synchronized: the model is reset)
  return IWAE_OK;
}

int iwae_get_params(iwae_handle* h, float* host, long long n) {
  CHK(check_n(h, n, host));
  return download(h, h->params, host);
}

int iwae_get_grads(iwae_handle* h, float* host, long long n) {
  CHK(check_n(h, n, host));
  return download(h, h->grad, host);
}

int iwae_set_adam(iwae_handle* h, float lr, float b1, float b2, float eps) {
  if (!h) return IWAE_EINVAL;
  float v[4] = {lr, b1, b2, eps};
  HIPCHK(hipMemcpyAsync(&h->ds->adam, v, sizeof(v), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return IWAE_OK;
}

int iwae_get_adam_state(iwae_handle* h, float* m, float* v, long long n, long long* step) {
  CHK(check_n(h, n, m));
  CHK(check_n(h, n, v));
  CHK(download(h, h->adam_m, m));
  CHK(download(h, h->adam_v, v));
  if (step) {
    AdamState s;
    HIPCHK(hipMemcpy(&s, &h->ds->adam, sizeof(s), hipMemcpyDeviceToHost));
    *step = s.t;
  }
  return IWAE_OK;
}

int iwae_set_adam_state(iwae_handle* h, const float* m, const float* v, long long n, long long step) {
  CHK(check_n(h, n, m));
  CHK(check_n(h, n, v));
  CHK(upload(h, h->adam_m, m));
  CHK(upload(h, h->adam_v, v));
  AdamState s;
  HIPCHK(hipMemcpy(&s, &h->ds->adam, sizeof(s), hipMemcpyDeviceToHost));
  s.t = step;
  HIPCHK(hipMemcpy(&h->ds->adam, &s, sizeof(s), hipMemcpyHostToDevice));
  return IWAE_OK;
}

int iwae_train_step(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
                    const float* const* eps, int n_eps, float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  return do_train(h, lc, x, B, eps, n_eps, loss_dev, true);
}

int iwae_train_step_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask, int B,
                           const float* const* eps, int n_eps, float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  CHK(check_masked(h, mask));
  return do_train(h, lc, x, B, eps, n_eps, loss_dev, true, mask);
}

int iwae_forward_backward_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask, int B,
                                 const float* const* eps, int n_eps, float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  CHK(check_masked(h, mask));
  return do_train(h, lc, x, B, eps, n_eps, loss_dev, false, mask);
}

int iwae_train_steps(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, int nsteps,
                     float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  if (!lc) return fail(h, IWAE_EINVAL, "loss config is NULL");
  CHK(kernel_status(h));
  CHK(do_train_steps(h, lc, x, B, nsteps, loss_dev));
  return kernel_status(h);
}

int iwae_train_steps_prepare(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, int nsteps) {
  if (!h) return IWAE_EINVAL;
  if (!lc) return fail(h, IWAE_EINVAL, "loss config is NULL");
  return do_train_steps(h, lc, x, B, nsteps, nullptr, true);
}

int iwae_forward_backward(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B,
                          const float* const* eps, int n_eps, float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  return do_train(h, lc, x, B, eps, n_eps, loss_dev, false);
}

int iwae_grad_buffer(iwae_handle* h, float** g, long long* n) {
  if (!h || !g || !n) return IWAE_EINVAL;
  *g = h->grad;
  *n = h->nparam_int;
  return IWAE_OK;
}

int iwae_grad_moments(iwae_handle* h, float* sum_dev, float* sumsq_dev) {
  if (!h) return IWAE_EINVAL;
  if (!sum_dev || !sumsq_dev) return fail(h, IWAE_EINVAL, "NULL moment buffer");
  if ((h->nparam_int & 3) != 0) return fail(h, IWAE_EINVAL, "internal gradient layout not float4-padded");
  HIPCHK(launch_grad_moments(h->stream, h->grad, sum_dev, sumsq_dev, h->nparam_int));
  return IWAE_OK;
}

int iwae_export_internal(iwae_handle* h, const float* internal_dev, float* host, long long n) {
  CHK(check_n(h, n, host));
  if (!internal_dev) return fail(h, IWAE_EINVAL, "internal_dev is NULL");
  return download(h, internal_dev, host);
}

int iwae_bind_grad_buffer(iwae_handle* h, float* g, long long n) {
  if (!h) return IWAE_EINVAL;
  const long long need = h->nparam_int + (h->dp_weighted ? 4 : 0);
  if (g && n != h->nparam_int && n != h->nparam_int + 4)
    return fail(h, IWAE_EINVAL, "grad buffer must hold " + std::to_string(h->nparam_int) + " (+4 under data "
                                "parallelism) floats");
  if (g && n < need)
    return fail(h, IWAE_EINVAL, "data parallel: the grad buffer needs " + std::to_string(need) + " floats");
  h->grad = g ? g : h->grad_own;
  invalidate_graphs(h);
  return IWAE_OK;
}

int iwae_apply_adam(iwae_handle* h, float grad_scale) {
  if (!h) return IWAE_EINVAL;
  if (!(grad_scale > 0.f)) {
    // data parallel: 1 / the all-reduced batch total in the buffer's tail
    if (!h->dp_weighted) return fail(h, IWAE_EINVAL, "grad_scale must be > 0 (0 only after iwae_dp_init)");
    return run_adam(h, AdamMode::from_grad_over(h->grad + h->nparam_int).own_tick());
  }
  return run_adam(h, AdamMode::from_grad(grad_scale).own_tick());
}

int iwae_dp_unique_id(void* out128) {
  if (!out128) return IWAE_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return IWAE_EHIP;
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(out128, &id, sizeof(id));
  return IWAE_OK;
}

int iwae_dp_init(iwae_handle* h, int rank, int world, const void* uid) {
  if (!h) return IWAE_EINVAL;
  // every argument is checked before any handle state changes: a failed call
  // leaves the handle (communicator, weighting, noise stream) as it was
  if (world < 1 || rank < 0 || rank >= world) return fail(h, IWAE_EINVAL, "need 0 <= rank < world");
  const bool weighted = world > 1 || uid != nullptr;
  if (weighted && h->grad != h->grad_own)
    return fail(h, IWAE_EINVAL, "iwae_dp_init before binding a grad buffer (then bind n + 4 floats)");
  HIPCHK(hipStreamSynchronize(h->stream));
  ncclComm_t comm = nullptr;
  if (uid) {
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    HIPCHK(hipSetDevice(h->device));
    const ncclResult_t r = ncclCommInitRank(&comm, world, id, rank);
    if (r != ncclSuccess) return fail(h, IWAE_EHIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  if (h->comm) (void)ncclCommDestroy(h->comm);
  h->comm = comm;
  h->dp_rank = rank;
  h->dp_world = world;
  h->dp_weighted = weighted;
  invalidate_graphs(h);
  return iwae_set_noise_stream(h, (unsigned long long)rank);
}

int iwae_dp_broadcast_state(iwae_handle* h) {
  if (!h) return IWAE_EINVAL;
  if (!h->comm) return fail(h, IWAE_EINVAL, "iwae_dp_broadcast_state needs iwae_dp_init with an RCCL id");
  const size_t n = (size_t)h->nparam_int;
  ncclResult_t r = ncclGroupStart();
  if (r == ncclSuccess) r = ncclBroadcast(h->params, h->params, n, ncclFloat32, 0, h->comm, h->stream);
  if (r == ncclSuccess) r = ncclBroadcast(h->adam_m, h->adam_m, n, ncclFloat32, 0, h->comm, h->stream);
  if (r == ncclSuccess) r = ncclBroadcast(h->adam_v, h->adam_v, n, ncclFloat32, 0, h->comm, h->stream);
  // the Adam step counter (an int64 at DevState::adam.t)
  if (r == ncclSuccess) r = ncclBroadcast(&h->ds->adam.t, &h->ds->adam.t, 1, ncclInt64, 0, h->comm, h->stream);
  const ncclResult_t r2 = ncclGroupEnd();
  if (r != ncclSuccess || r2 != ncclSuccess)
    return fail(h, IWAE_EHIP, std::string("ncclBroadcast: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->params_version++;
  return IWAE_OK;
}

int iwae_dp_world(const iwae_handle* h, int* world, int* comm_ranks) {
  if (!h || !world || !comm_ranks) return IWAE_EINVAL;
  *world = h->dp_world;
  int n = 0;
  if (h->comm && ncclCommCount(h->comm, &n) != ncclSuccess) n = -1;
  *comm_ranks = n;
  return IWAE_OK;
}

// (mask: a pixel-masked plan's mask, P.pix set; null otherwise)
static int eval_forward(iwae_handle* h, const Plan& P, const float* x, const float* const* eps, int n_eps,
                        EpsSet& E, const float* mask = nullptr) {
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (h->x3) CHK(ensure_wsplit(h));
  CHK(parse_eps(h, P, eps, n_eps, E));
  CHK(ensure_capacity(h, P.Bimg, P.Bimg * P.kS, false));
  if (mask) CHK(stage_masked(h, P, x, mask));
  else CHK(copy_x(h, P, x));
  return forward_core(h, P, E, false);
}

int iwae_log_weights(iwae_handle* h, const float* x, int B, int k, const float* const* eps, int n_eps,
                     float* lw) {
  if (!h) return IWAE_EINVAL;
  if (!lw) return fail(h, IWAE_EINVAL, "lw is NULL");
  iwae_loss_config lc{IWAE_LOSS_VAE, k, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, B, P));
  EpsSet E;
  CHK(eval_forward(h, P, x, eps, n_eps, E));
  CHK(run_bound(h, P, false, 1.f, &h->ds->scalars[1]));
  HIPCHK(hipMemcpyAsync(lw, h->lw, (size_t)B * k * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return IWAE_OK;
}

int iwae_bound(iwae_handle* h, const iwae_loss_config* lc, const float* x, int B, const float* const* eps,
               int n_eps, float* value_dev) {
  if (!h) return IWAE_EINVAL;
  if (!value_dev) return fail(h, IWAE_EINVAL, "value_dev is NULL");
  Plan P;
  CHK(make_plan(h, lc, B, P));
  EpsSet E;
  CHK(eval_forward(h, P, x, eps, n_eps, E));
  CHK(run_bound(h, P, false, 1.f, value_dev));
  return IWAE_OK;
}

int iwae_bound_masked(iwae_handle* h, const iwae_loss_config* lc, const float* x, const float* mask, int B,
                      const float* const* eps, int n_eps, float* value_dev) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  CHK(check_masked(h, mask));
  if (!value_dev) return fail(h, IWAE_EINVAL, "value_dev is NULL");
  Plan P;
  CHK(make_plan(h, lc, B, P));
  P.pix = 1;
  EpsSet E;
  CHK(eval_forward(h, P, x, eps, n_eps, E, mask));
  CHK(run_bound(h, P, false, 1.f, value_dev));
  return IWAE_OK;
}

int iwae_e_log_px(iwae_handle* h, const float* x, int B, int k, const float* const* eps, int n_eps,
                  float* value_dev) {
  if (!h) return IWAE_EINVAL;
  if (!value_dev) return fail(h, IWAE_EINVAL, "value_dev is NULL");
  iwae_loss_config lc{IWAE_LOSS_VAE, k, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, B, P));
  P.mode_a = BM_NONE; P.w_a = 0.f; P.need_bce = 1; P.bce_w = 1.f;
  EpsSet E;
  CHK(eval_forward(h, P, x, eps, n_eps, E));
  CHK(run_bound(h, P, false, 1.f, value_dev));
  return IWAE_OK;
}

// ------------------------------------------------ fused-chain plans
// What the plans of the kernels built on iwae_mega_dev.h (mega_fwd_kernel,
// gen_kernel, post_kernel) and sg_kernel's share: the buffer widths the stages
// need, the stage record's weight fields, and the LDS layout of the buffers.
static int r32(int x) { return (x + 31) & ~31; }

// Widths (bf16 columns) of a plan's LDS buffers.
struct ChainBufs {
  std::vector<int> width;
  explicit ChainBufs(int nb) : width(nb, 0) {}
  void widen(int b, int w) { width[b] = std::max(width[b], w); }
  // a Dense stage of padded K ldk read from `in`; out >= 0: its N outputs are
  // stored there as activations, padded to the reader's K (next_k)
  void dense(int ldk, int N, int in, int out, int next_k) {
    widen(in, ldk);
    if (out >= 0) widen(out, std::max(N, next_k));
  }
  // Each buffer = hi and lo bf16 planes [R][ld].  Row stride s dwords (ld = 2 s):
  // s = 8 mod 16 makes the fragment reads (ds_read_b128) conflict-free; s = 4
  // mod 8 (2-way) is the fallback of the plans that try one.  Fills buf_ld /
  // buf_off (bf16 units) and returns the bf16 units used.  The plans call it
  // per candidate, so a plan that returns false leaves its last candidate's
  // strides, offsets and LDS size behind and does not touch rt (the callers
  // start it at 0): a plan, rt and lds are read only on true.
  int layout(int R, bool fallback, int* buf_ld, int* buf_off) const {
    int off = 0;
    for (size_t b = 0; b < width.size(); ++b) {
      int sdw = (std::max(width[b], 32) + 1) / 2;
      while (fallback ? sdw % 8 != 4 : sdw % 16 != 8) ++sdw;
      buf_ld[b] = 2 * sdw;
      buf_off[b] = off;
      off += 2 * R * buf_ld[b];
    }
    return off;
  }
};

// Dense layer di as a stage of kind act (TANH is MG_TANH in every kernel's
// enum) reading in and writing out: the buffers widened, and, unless S is null
// (a stage the call does not run), its record filled.  Weights: the
// fragment-major split copies (FX, the train engine's): one 16-byte load per
// lane reads 1 KiB contiguous per wave.
static void chain_stage(const iwae_handle* h, ChainBufs& W, MgStage* S, int di, int in, int out, int act, int next_k) {
  const DenseL& d = h->dense[di];
  W.dense(d.ldF, d.fout, in, act == MG_TANH ? out : -1, next_k);
  if (!S) return;
  S->Whi = h->fx_hi + d.fx_off; S->Wlo = h->fx_lo + d.fx_off;
  S->W_bytes = (unsigned)((h->fx_elems - d.fx_off) * (long long)sizeof(__bf16));
  S->ldk = d.ldF; S->K = d.fin + 1; S->N = d.fout;
  S->in_buf = in; S->out_buf = out; S->act = act; S->next_k = next_k;
}
// A stochastic layer's head (rows permuted into [mu | zs] groups of 8) of
// latent width dd, sampled into / scored against buffer out (-1: post_plan's
// top latent, which has no buffer to widen; every other head has one)
static void chain_head(const iwae_handle* h, ChainBufs& W, MgStage* S, int di, int in, int out, int act, int dd,
                       int layer) {
  chain_stage(h, W, S, di, in, out, act, r32(dd + 1));
  if (out >= 0) W.widen(out, r32(dd + 1));
  if (!S) return;
  S->N = 8 * ((dd + 3) / 4);
  S->d = dd; S->layer = layer;
}

// ------------------------------------------------ fused k-sample forward
// Plan of mega_fwd_kernel for this model (iwae_mega.hip).  LDS buffers: h_0 ..
// h_{L-2} kept (ids 0 .. L-2), scratch P (id L-1, also holds h_{L-1}) and Q
// (id L).  Stages after the first encoder layer:
//   encoder i = 1..L-1:  h_{i-1} -> P (tanh) -> Q (tanh) -> head: sample h_i
//   decoder prior j:     h_{L-1-j} -> Q -> P -> head: log p(h_{L-2-j} | .)
//   output MLP:          h_0 -> Q -> P -> Dense(784) + Bernoulli
// False if it does not fit the LDS.
static bool mega_plan(iwae_handle* h, MgLaunch& M, int& rt, int& waves, size_t& lds) {
  const int L = h->L;
  std::memset(&M, 0, sizeof(M));
  const int bP = L - 1, bQ = L;
  auto hbuf = [&](int i) { return i == L - 1 ? bP : i; };
  const int nb = L + 1;
  if (nb > kMgMaxBufs) return false;
  ChainBufs W(nb);
  std::vector<MgStage> st;
  auto stage = [&](int di, int in, int out, int act, int next_k) {
    st.emplace_back();
    chain_stage(h, W, &st.back(), di, in, out, act, next_k);
  };
  auto head = [&](int di, int in, int out, int act, int dd, int layer, int stdnormal) {
    st.emplace_back();
    chain_head(h, W, &st.back(), di, in, out, act, dd, layer);
    st.back().stdnormal = stdnormal;
  };
  for (int i = 1; i < L; ++i) {
    const StochL& E = h->enc[i];
    stage(E.l1, hbuf(i - 1), bP, MG_TANH, h->dense[E.l2].ldF);
    stage(E.l2, bP, bQ, MG_TANH, h->dense[E.head].ldF);
    head(E.head, bQ, hbuf(i), MG_SAMPLE, E.d, i, i == L - 1);
  }
  for (int j = 0; j < L - 1; ++j) {
    const StochL& D = h->dec[j];
    stage(D.l1, hbuf(L - 1 - j), bQ, MG_TANH, h->dense[D.l2].ldF);
    stage(D.l2, bQ, bP, MG_TANH, h->dense[D.head].ldF);
    head(D.head, bP, hbuf(L - 2 - j), MG_PRIOR, D.d, 0, 0);
  }
  const int h0 = hbuf(0);
  stage(h->o1, h0, bQ, MG_TANH, h->dense[h->o2].ldF);
  stage(h->o2, bQ, bP, MG_TANH, h->dense[h->o3].ldF);
  stage(h->o3, bP, -1, MG_BERN, 0);
  if ((int)st.size() > kMgMaxStages) return false;
  W.widen(h0, r32(h->enc[0].d + 1));
  // LDS layout: the buffers (ChainBufs::layout, conflict-free strides first),
  // then logq, logp [R] and the [8][R] reduction scratch as floats.
  // 8-wave workgroups of 64 / 32 / 16 rows, or (h->tune.mg_waves == 4) 4-wave
  // workgroups of 32 rows, two per CU
  waves = h->tune.mg_waves == 4 ? 4 : 8;
  for (int c : {4, 2, 1}) {
    if (waves == 4 && c != 2) continue;
    const int R = 16 * c;
    for (int pass = 0; pass < 2; ++pass) {
      const int off = W.layout(R, pass == 1, M.buf_ld, M.buf_off);
      M.acc_off = (off + 3) / 2 & ~1;           // floats
      const size_t bytes = (size_t)(M.acc_off + 2 * R + 8 * R) * sizeof(float);
      if (bytes <= (waves == 4 ? 80 : 160) * 1024) {
        rt = c;
        lds = bytes;
        for (size_t i = 0; i < st.size(); ++i) M.st[i] = st[i];
        M.nst = (int)st.size();
        M.h0_buf = h0; M.d0 = h->enc[0].d; M.h0_next_k = r32(h->enc[0].d + 1); M.h0_stdnormal = L == 1;
        return true;
      }
    }
  }
  return false;
}

// Plan of nring_kernel (iwae_nring.hip): stages and the unit table in
// consumption order.  False when the model is not one of the kernel's
// instantiated shapes (mega_fwd_kernel runs instead).
static bool nring_plan(iwae_handle* h, NrLaunch& R) {
  const int L = h->L;
  std::memset(&R, 0, sizeof(R));
  if (!h->tune.nring || (L != 1 && L != 2) || h->xdim > 800) return false;
  std::vector<NrUnit> units;
  auto stage = [&](int si, int di, int N, int next_k) {
    const DenseL& d = h->dense[di];
    NrStage& S = R.st[si];
    S.N = N;
    S.ntile = (N + 15) / 16;
    S.ns = d.ldF / 32;
    S.next_ns = next_k / 32;
    for (int t = 0; t < S.ntile; ++t)
      units.push_back(NrUnit{(unsigned)((d.fx_off + (long long)t * S.ns * 512) * (long long)sizeof(__bf16)), S.ns});
    return S.ns <= 8 && d.ldF % 32 == 0;
  };
  bool ok = true;
  if (L == 2) {
    const StochL& E = h->enc[1];
    const StochL& D = h->dec[0];
    ok = ok && stage(0, E.l1, h->dense[E.l1].fout, h->dense[E.l2].ldF);
    ok = ok && stage(1, E.l2, h->dense[E.l2].fout, h->dense[E.head].ldF);
    ok = ok && stage(2, E.head, 8 * ((E.d + 3) / 4), 0);
    R.st[2].d = E.d; R.st[2].layer = 1; R.st[2].stdnormal = 1;
    ok = ok && stage(3, D.l1, h->dense[D.l1].fout, h->dense[D.l2].ldF);
    ok = ok && stage(4, D.l2, h->dense[D.l2].fout, h->dense[D.head].ldF);
    ok = ok && stage(5, D.head, 8 * ((D.d + 3) / 4), 0);
    R.st[5].d = D.d; R.st[5].layer = 0; R.st[5].stdnormal = 0;
    // the h2 pair layout holds 8 * 4 * H2 columns, h1's 8 * 4 * H1 (ones column included)
    ok = ok && r32(E.d + 1) == h->dense[D.l1].ldF && r32(h->enc[0].d + 1) == h->dense[E.l1].ldF;
  }
  ok = ok && stage(6, h->o1, h->dense[h->o1].fout, h->dense[h->o2].ldF);
  ok = ok && stage(7, h->o2, h->dense[h->o2].fout, h->dense[h->o3].ldF);
  ok = ok && stage(8, h->o3, h->dense[h->o3].fout, 0);
  ok = ok && r32(h->enc[0].d + 1) == h->dense[h->o1].ldF && (int)units.size() + NR_D <= kNrMaxUnits - 8;
  R.L = L;
  R.d0 = h->enc[0].d;
  R.xdim = h->xdim;
  R.nunits = (int)units.size();
  if (!ok || !nring_shape_ok(R)) return false;
  return ring_plan_tail(h, h->nr_units, kNrMaxUnits, units, R);
}

// The train step's forward (the engine's forward launch: job E and the output
// job) on the weight-ring kernel in train mode: large batches (the engine's
// 32 / 64-row workgroups re-stream their job's weights per tile of rows; here
// 128 rows share one stream), the model shapes nring_kernel instantiates,
// Philox or single-buffer injected noise, no Keras-BCE epilogue (L_alpha).
// Writes what tc_run(TCL_FWD) writes.  False: run the engine's launch.
static bool nring_train_forward(iwae_handle* h, const Plan& P, const EpsSet& E, bool& ran) {
  ran = false;
  const long long rows = (long long)P.Bimg * P.kS;
  if (!h->tune.nring_train || !h->x3 || rows < h->tune.nr_train_rows || P.kS < 43 || P.need_bce || use_fold0(h, P) ||
      P.Bsplit != P.Bimg || P.pix)
    return true;
  if (E.a[0] && (h->L >= 2 && !E.a[1])) return true;
  NrLaunch NR;
  if (!nring_plan(h, NR)) return true;
  if (ensure_fx(h) != IWAE_OK) return false;
  const int L = h->L;
  auto out = [](NrStage& S, const Mat& m) { S.out = m.p; S.ld_out = m.ld; };
  if (L == 2) {
    out(NR.st[0], h->eb[1].y1); out(NR.st[1], h->eb[1].y2); out(NR.st[2], h->eb[1].P);
    NR.st[2].h = h->h[1].p; NR.st[2].ld_h = h->h[1].ld; NR.st[2].eps = h->eps_st[1].p; NR.st[2].ld_eps = h->eps_st[1].ld;
    out(NR.st[3], h->db[0].y1); out(NR.st[4], h->db[0].y2); out(NR.st[5], h->db[0].P);
  }
  out(NR.st[6], h->ob.y1); out(NR.st[7], h->ob.y2); out(NR.st[8], h->ob.P);
  NR.train = 1;
  NR.h1 = h->h[0].p; NR.ld_h1 = h->h[0].ld; NR.e1 = h->eps_st[0].p; NR.ld_e1 = h->eps_st[0].ld;
  NR.logq = h->logq; NR.logp = h->logp; NR.bern = h->ebern; NR.ld_bern = 4;
  NR.wa = P.wa;
  NR.rows = (int)rows; NR.kS = P.kS;
  NR.P0 = h->eb[0].P.p; NR.ldP0 = h->eb[0].P.ld;
  NR.x = h->x_in.p; NR.ldx = h->x_in.ld;
  NR.seed = h->seed; NR.rng_base = &h->ds->rng[0];
  for (int i = 0; i < 8; ++i) NR.eps[i] = i < L ? E.a[i] : nullptr;
  NR.eps_N = P.Bimg; NR.eps_i0 = 0; NR.eps_s0 = 0;
  if (launch_nring(h->stream, NR) != hipSuccess) return false;
  ++h->count.nring_train;
  ran = true;
  return true;
}

// Plan of nrb_kernel (iwae_nring.hip): the GX units of the output MLP's
// backward in consumption order -- per k step of GX(o3) its column tiles 0..7
// and 8.. (one piece per tile, stride one tile's k steps), then GX(o2)'s and
// GX(o1)'s column tiles (one unit each, their k steps).  False when the shape
// is not instantiated (the engine's job O' runs instead).
static bool nrb_plan(iwae_handle* h, NrbLaunch& R) {
  std::memset(&R, 0, sizeof(R));
  if (!h->tune.nring_bwd || !h->x3) return false;
  const DenseL& d3 = h->dense[h->o3];
  const DenseL& d2 = h->dense[h->o2];
  const DenseL& d1 = h->dense[h->o1];
  R.gx3_tiles = d3.gx_tiles; R.gx3_steps = d3.gx_steps;
  R.gx2_tiles = d2.gx_tiles; R.gx2_steps = d2.gx_steps;
  R.gx1_tiles = d1.gx_tiles; R.gx1_steps = d1.gx_steps;
  R.N = h->xdim; R.H = d2.fout; R.d1 = d1.fin;
  if (d3.fin != R.H || d2.fin != R.H || d1.fout != R.H || d3.gx_tiles <= 8 || d3.gx_tiles > 16) return false;
  std::vector<NrUnit> units;
  auto piece = [](long long off_bf16) { return (unsigned)(off_bf16 * (long long)sizeof(__bf16)); };
  for (int s = 0; s < d3.gx_steps; ++s) {
    units.push_back(NrUnit{piece(d3.gx_off + (long long)s * 512), 8 | (d3.gx_steps << 8)});
    units.push_back(NrUnit{piece(d3.gx_off + (8LL * d3.gx_steps + s) * 512), (d3.gx_tiles - 8) | (d3.gx_steps << 8)});
  }
  for (int t = 0; t < d2.gx_tiles; ++t)
    units.push_back(NrUnit{piece(d2.gx_off + (long long)t * d2.gx_steps * 512), d2.gx_steps | (1 << 8)});
  for (int t = 0; t < d1.gx_tiles; ++t)
    units.push_back(NrUnit{piece(d1.gx_off + (long long)t * d1.gx_steps * 512), d1.gx_steps | (1 << 8)});
  R.nunits = (int)units.size();
  if (!nrb_shape_ok(R)) return false;
  return ring_plan_tail(h, h->nrb_units, kNrbMaxUnits, units, R);
}

// The output MLP's backward of a large-batch train step (the engine's job O')
// on nrb_kernel, after the bound launch (dpx in HBM), when the forward ran on
// the weight ring (its shapes; g, y1, y2 stored by it).  Writes what job O'
// writes (ob.dY2, ob.dY1, dh_out[0]).  ran = false: the engine runs job O'.
static bool nring_train_backward(iwae_handle* h, const Plan& P, bool fwd_ring, bool& ran, hipStream_t st) {
  ran = false;
  if (!fwd_ring || !h->tune.nring_bwd) return true;
  NrbLaunch NB;
  if (!nrb_plan(h, NB)) return true;
  NB.rows = P.Bimg * P.kS;
  NB.g = h->ob.P.p; NB.ld_g = h->ob.P.ld;
  NB.dpx = h->dpx;
  NB.y2 = h->ob.y2.p; NB.ld_y2 = h->ob.y2.ld; NB.y1 = h->ob.y1.p; NB.ld_y1 = h->ob.y1.ld;
  NB.dY2 = h->ob.dY2.p; NB.ld_dY2 = h->ob.dY2.ld; NB.dY1 = h->ob.dY1.p; NB.ld_dY1 = h->ob.dY1.ld;
  NB.dh = h->dh_out[0].p; NB.ld_dh = h->dh_out[0].ld;
  if (launch_nrb(st, NB) != hipSuccess) return false;
  ++h->count.nrb;
  ran = true;
  return true;
}

// Plan of nre_kernel (iwae_nring.hip): the GX units of the decoder prior's
// head, l2, l1 and the encoder's second layer's head, l2, l1 (one column tile
// each, its k steps).  2-layer paper shape only; false: the engine's job E'.
static bool nre_plan(iwae_handle* h, NreLaunch& R) {
  std::memset(&R, 0, sizeof(R));
  if (h->tune.nring_bwd != 3 || !h->x3 || h->L != 2) return false;
  const int di[6] = {h->dec[0].head, h->dec[0].l2, h->dec[0].l1, h->enc[1].head, h->enc[1].l2, h->enc[1].l1};
  std::vector<NrUnit> units;
  for (int i = 0; i < 6; ++i) {
    const DenseL& d = h->dense[di[i]];
    R.gx_tiles[i] = d.gx_tiles; R.gx_steps[i] = d.gx_steps;
    for (int t = 0; t < d.gx_tiles; ++t)
      units.push_back(NrUnit{(unsigned)((d.gx_off + (long long)t * d.gx_steps * 512) * (long long)sizeof(__bf16)),
                             d.gx_steps});
    // (after the prior chain: empty units, so nothing of the encoder chain is
    // in flight while the kernel stages the encoder's Gaussian backward in the ring's LDS)
    if (i == 2)
      for (int e = 0; e < kNreGap; ++e) units.push_back(NrUnit{0u, 0});
  }
  R.nunits = (int)units.size();
  R.dp = h->dec[0].d; R.de = h->enc[1].d;
  R.Hp = h->dense[h->dec[0].l2].fout; R.He = h->dense[h->enc[1].l2].fout;
  if (!nre_shape_ok(R)) return false;
  return ring_plan_tail(h, h->nre_units, kNrMaxUnits, units, R);
}

// The engine's job E' on nre_kernel (after nrb_kernel, which needs nothing of
// it): writes what the engine's backward launch without job O' writes.
static bool nring_train_backward_enc(iwae_handle* h, const Plan& P, bool& ran) {
  ran = false;
  NreLaunch R;
  if (!nre_plan(h, R)) return true;
  auto in = [](const Mat& m, const float*& p, int& ld) { p = m.p; ld = m.ld; };
  auto out = [](const Mat& m, float*& p, int& ld) { p = m.p; ld = m.ld; };
  R.rows = P.Bimg * P.kS;
  R.dlw = h->dlw;
  in(h->db[0].P, R.Pp, R.ld_Pp); in(h->h[0], R.h1, R.ld_h1);
  in(h->db[0].y2, R.py2, R.ld_py2); in(h->db[0].y1, R.py1, R.ld_py1);
  out(h->db[0].dP, R.pdP, R.ld_pdP); out(h->dh_prior[0], R.dh_prior, R.ld_dh_prior);
  out(h->db[0].dY2, R.pdY2, R.ld_pdY2); out(h->db[0].dY1, R.pdY1, R.ld_pdY1);
  out(h->dh_dec[1], R.dh_dec, R.ld_dh_dec);
  in(h->eb[1].P, R.Pe, R.ld_Pe); in(h->h[1], R.h2, R.ld_h2); in(h->eps_st[1], R.e2, R.ld_e2);
  in(h->eb[1].y2, R.ey2, R.ld_ey2); in(h->eb[1].y1, R.ey1, R.ld_ey1);
  out(h->eb[1].dP, R.edP, R.ld_edP); out(h->eb[1].dY2, R.edY2, R.ld_edY2); out(h->eb[1].dY1, R.edY1, R.ld_edY1);
  out(h->dh_enc[0], R.dh_enc, R.ld_dh_enc);
  if (launch_nre(h->stream, R) != hipSuccess) return false;
  ++h->count.nre;
  ran = true;
  return true;
}

// chunked k-sample NLL over N images; accumulates per-image (m, s)
// eps (optional, parity): L buffers [k][N][d_i]; only the fused kernel takes
// them chunk by chunk (the caller checks nll_mega_ok first)
static bool nll_mega_ok(iwae_handle* h) {
  MgLaunch MG;
  int rt = 0, w = 8;
  size_t lds = 0;
  return h->x3 && h->nll_fused && !h->masked && mega_plan(h, MG, rt, w, lds);
}

static int nll_core(iwae_handle* h, const float* x, int N, int k, int chunk, float* out_m, float* out_s,
                    float* out_logpx, const float* const* eps = nullptr) {
  if (!h) return IWAE_EINVAL;
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  const int imgs = chunk_images(h, N, k, chunk, false);
  if (!imgs) return IWAE_EINVAL;
  // 2^20 sample rows per chunk (measured fastest: 2^17-2^20 within 10 %, smaller slower): the samples split
  const long long target_rows = std::max<long long>(h->tune.nll_rows, k);
  const int kS = (int)std::min<long long>(k, std::max<long long>(1, target_rows / imgs));
  FwdPlan F;
  const bool mega = h->x3 && h->nll_fused && !h->masked && mega_plan(h, F.MG, F.rt, F.waves, F.lds);
  ChunkWalk W(h, N, k, imgs, mega, x, nullptr, mega);
  CHK(ensure_capacity(h, W.sup, imgs * kS, false));
  if (h->x3) CHK(ensure_wsplit(h));
  if (mega) CHK(ensure_fx(h));
  if (eps && !mega) return fail(h, IWAE_EINVAL, "injected-noise NLL chunks need the fused kernel");
  F.ring = mega && nring_plan(h, F.NR);
  fwd_call_fields(h, F, eps, N);
  for (; W.i0 < N; W.i0 += imgs) {
    CHK(walk_step(h, W));
    const int i0 = W.i0, n = W.n;
    for (int s0 = 0; s0 < k; s0 += kS) {
      Plan P;
      P.B = n; P.Bimg = n; P.Bsplit = n; P.kS = std::min(kS, k - s0);
      LseArgs a = lse_args(h, P.kS, n, s0 == 0);
      if (mega) {
        // the chunk's rows of the first encoder layer's output, then everything else fused
        CHK(launch_fwd_chunk(h, F, W, P, s0, eps != nullptr));
        a.lw = h->lw;
      } else {
        EpsSet E;
        std::memset(&E, 0, sizeof(E));
        CHK(forward_core(h, P, E, false));
      }
      HIPCHK(launch_lse(h->stream, a));
    }
    if (out_logpx) HIPCHK(launch_lse_final(h->stream, h->run_m, h->run_s, n, logf((float)k), out_logpx + i0));
    if (out_m) HIPCHK(hipMemcpyAsync(out_m + i0, h->run_m, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (out_s) HIPCHK(hipMemcpyAsync(out_s + i0, h->run_s, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  return IWAE_OK;
}

int iwae_nll(iwae_handle* h, const float* x, int N, int k, int chunk, float* out_logpx) {
  if (!h) return IWAE_EINVAL;
  if (!out_logpx) return fail(h, IWAE_EINVAL, "out_logpx is NULL");
  return nll_core(h, x, N, k, chunk, nullptr, nullptr, out_logpx);
}

int iwae_nll_partials(iwae_handle* h, const float* x, int N, int k_local, int chunk, float* out_m,
                      float* out_s) {
  if (!h) return IWAE_EINVAL;
  if (!out_m || !out_s) return fail(h, IWAE_EINVAL, "NULL output");
  return nll_core(h, x, N, k_local, chunk, out_m, out_s, nullptr);
}

int iwae_nll_eps(iwae_handle* h, const float* x, int N, int k, const float* const* eps, int n_eps,
                 float* out_logpx) {
  if (!h) return IWAE_EINVAL;
  if (!out_logpx) return fail(h, IWAE_EINVAL, "out_logpx is NULL");
  if (eps && n_eps == h->L && nll_mega_ok(h)) {
    // the kernel the NLL benchmark times (mega_fwd_kernel), fed the caller's noise
    for (int i = 0; i < h->L; ++i)
      if (!eps[i]) return fail(h, IWAE_EINVAL, "NULL eps buffer");
    return nll_core(h, x, N, k, 0, nullptr, nullptr, out_logpx, eps);
  }
  iwae_loss_config lc{IWAE_LOSS_IWAE, k, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, N, P));
  EpsSet E;
  CHK(eval_forward(h, P, x, eps, n_eps, E));
  HIPCHK(launch_lse(h->stream, lse_args(h, k, N, true)));
  HIPCHK(launch_lse_final(h->stream, h->run_m, h->run_s, N, logf((float)k), out_logpx));
  return IWAE_OK;
}

// ------------------------------------------------ evaluation statistics
// get_levels_of_units_activity (F:264-F:281): mean of every h_i over n
// samples per image.  Chunks of images keep chunk*n rows within 2^20.
int iwae_encoder_means(iwae_handle* h, const float* x, int N, int n, const float* const* eps, int n_eps,
                       float* const* out_means, int n_out) {
  if (!h) return IWAE_EINVAL;
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (N <= 0 || n <= 0) return fail(h, IWAE_EINVAL, "N and n_samples must be positive");
  if (!out_means || n_out != h->L) return fail(h, IWAE_EINVAL, "expected one output per stochastic layer");
  for (int i = 0; i < h->L; ++i)
    if (!out_means[i]) return fail(h, IWAE_EINVAL, "NULL output buffer");
  const long long max_rows = 1LL << 20;
  if (n > max_rows) return fail(h, IWAE_EINVAL, "n_samples above 2^20 per image is not supported");
  const bool injected = eps && n_eps > 0;
  int imgs = injected ? N : (int)std::max<long long>(1, max_rows / n);
  imgs = std::min(imgs, N);
  if (h->x3) CHK(ensure_wsplit(h));
  CHK(ensure_capacity(h, imgs, imgs * n, false));
  for (int i0 = 0; i0 < N; i0 += imgs) {
    const int m = std::min(imgs, N - i0);
    Plan P;
    P.B = m; P.Bimg = m; P.Bsplit = m; P.kS = n;
    EpsSet E;
    CHK(parse_eps(h, P, eps, n_eps, E));
    CHK(stage_x(h, x, nullptr, i0, m));
    CHK(encoder_fwd(h, P, E, false));
    for (int l = 0; l < h->L; ++l) {
      const int d = h->enc[l].d;
      HIPCHK(launch_group_mean(h->stream, h->h[l].p, h->h[l].ld, n, d, m, out_means[l] + (size_t)i0 * d, d,
                               1.f / (float)n, 0, l == h->L - 1 ? &h->ds->rng[0] : nullptr));
    }
  }
  return IWAE_OK;
}

// Decoder.generate_x's prior chain (F:106-F:119), layer-wise, over `rows` rows:
// h_{L-2-j} drawn from dec[j](h_{L-1-j}) for j = 0 .. L-2, h_{L-1} in place.
// eps: prior layer j's injected noise eps[j] [rows][d], or null: Philox, in a
// stream of its own (layer ids IWAE_MAX_LAYERS + j).  h_out: tight f32 copies
// h_out[i] [rows][d_i] of the drawn h_i, or null.
static int prior_chain_fwd(iwae_handle* h, int rows, const float* const* eps, float* const* h_out) {
  const int L = h->L;
  for (int j = 0; j < L - 1; ++j) {
    CHK(stoch_fwd(h, h->dec[j], h->h[L - 1 - j], rows, h->db[j]));
    GaussArgs g{};
    g.P = h->db[j].P.p; g.ldP = h->db[j].P.ld; g.prow_div = 1; g.d = h->dec[j].d;
    g.H = h->h[L - 2 - j].p; g.ldH = h->h[L - 2 - j].ld;
    g.eps_a = eps ? eps[j] : nullptr;
    if (eps && !g.eps_a) return fail(h, IWAE_EINVAL, "NULL eps buffer");
    g.kS = 1; g.Bsplit = rows; g.Bimg = rows;
    g.seed = h->seed; g.rng_base = &h->ds->rng[0]; g.layer = IWAE_MAX_LAYERS + j;
    g.out = h->logp; g.accumulate = 0; g.M = rows;
    HIPCHK(launch_gauss_fwd(h->stream, 0, g));
    if (h_out) {
      const size_t wb = (size_t)g.d * sizeof(float);
      HIPCHK(hipMemcpy2DAsync(h_out[L - 2 - j], wb, g.H, (size_t)g.ldH * sizeof(float), wb, rows,
                              hipMemcpyDeviceToDevice, h->stream));
    }
  }
  return IWAE_OK;
}

// reconstructed_x_probs / get_reconstruction_loss (F:249-F:262): one encoder
// sample, keep h_L, re-draw h_{L-1} .. h_1 from the decoder's prior layers
// (Decoder.generate_x, F:106-F:119), then the output MLP.
int iwae_reconstruct(iwae_handle* h, const float* x, int B, const float* const* eps, int n_eps, float* probs,
                     int ld_probs, float* loss_dev) {
  if (!h) return IWAE_EINVAL;
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  const int L = h->L;
  const bool injected = eps && n_eps > 0;
  if (injected && n_eps != 2 * L - 1)
    return fail(h, IWAE_EINVAL, "expected " + std::to_string(2 * L - 1) + " eps buffers (encoder, then prior)");
  if (probs && (ld_probs < h->xdim || (ld_probs & 3) || ((uintptr_t)probs & 15)))
    return fail(h, IWAE_EINVAL, "probs needs ld >= x_dim, a multiple of 4, 16-byte aligned");
  iwae_loss_config lc{IWAE_LOSS_VAE, 1, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, B, P));
  P.mode_a = BM_NONE; P.w_a = 0.f; P.need_bce = 1; P.bce_w = 1.f;
  EpsSet E;
  CHK(parse_eps(h, P, eps, injected ? L : 0, E));
  if (h->x3) CHK(ensure_wsplit(h));
  CHK(ensure_capacity(h, B, B, false));
  CHK(copy_x(h, P, x));
  CHK(encoder_fwd(h, P, E, false));
  CHK(prior_chain_fwd(h, B, injected ? eps + L : nullptr, nullptr));
  CHK(out_hidden(h, B));
  if (probs) CHK(out_probs(h, B, probs, ld_probs));
  // Keras BCE of x against those probabilities, summed over pixels, mean over
  // the batch (F:257-F:261) = -(E_q log p(x|h) with the BCE form); this pass
  // also advances the Philox base
  GemmArgs ex{};
  ex.aux = h->x_in.p; ex.ldaux = h->x_in.ld; ex.x_row_div = 1;
  ex.part = h->part; ex.part2 = h->part2; ex.ldpart = h->ldpart;
  ex.wa = P.wa; ex.wb = P.wb; ex.need_bce = 1;
  Mat gm;
  CHK(gemm_fwd(h, EPI_BERN, h->ob.y2, B, h->dense[h->o3], gm, ex));
  CHK(run_bound(h, P, false, -1.f, loss_dev ? loss_dev : &h->ds->scalars[1]));
  return IWAE_OK;
}

// ------------------------------------------------ generation from the prior
// Plan of gen_kernel for this model (iwae_generate.hip).  LDS buffers: the
// latents h_0 .. h_{L-1} kept (ids 0 .. L-1), scratch P (id L) and Q (id L+1).
//   prior layer j = 0..L-2:  h_{L-1-j} -> Q (tanh) -> P (tanh) -> head: sample h_{L-2-j}
//   output MLP:              h_0 -> Q -> P -> Dense(x_dim): probabilities / pixels
// Row strides of 8 mod 16 dwords (conflict-free fragment reads).  RT from
// {4, 2, 1}: the largest that fits 160 KB of LDS.  False if RT = 1 does not fit.
static bool gen_plan(iwae_handle* h, GnLaunch& G, int& rt, size_t& lds) {
  const int L = h->L;
  std::memset(&G, 0, sizeof(G));
  const int bP = L, bQ = L + 1, nb = L + 2;
  if (nb > kMgMaxBufs || 3 * L > kMgMaxStages) return false;
  ChainBufs W(nb);
  auto stage = [&](int di, int in, int out, int act, int next_k) {
    chain_stage(h, W, &G.st[G.nst++], di, in, out, act, next_k);
  };
  for (int j = 0; j < L - 1; ++j) {
    const StochL& D = h->dec[j];
    stage(D.l1, L - 1 - j, bQ, GN_TANH, h->dense[D.l2].ldF);
    stage(D.l2, bQ, bP, GN_TANH, h->dense[D.head].ldF);
    chain_head(h, W, &G.st[G.nst++], D.head, bP, L - 2 - j, GN_HEAD, D.d, IWAE_MAX_LAYERS + j);
  }
  stage(h->o1, 0, bQ, GN_TANH, h->dense[h->o2].ldF);
  stage(h->o2, bQ, bP, GN_TANH, h->dense[h->o3].ldF);
  stage(h->o3, bP, -1, GN_OUT, 0);
  G.d_top = h->enc[L - 1].d; G.top_buf = L - 1; G.top_next_k = r32(G.d_top + 1);
  G.top_layer = IWAE_MAX_LAYERS + L - 1; G.pix_layer = 2 * IWAE_MAX_LAYERS;
  W.widen(L - 1, G.top_next_k);
  for (int c : {4, 2, 1}) {
    lds = (size_t)W.layout(16 * c, false, G.buf_ld, G.buf_off) * sizeof(__bf16);
    if (lds <= 160 * 1024) { rt = c; return true; }
  }
  return false;
}

int iwae_generate(iwae_handle* h, int n, const float* h_top, const float* const* eps, int n_eps, const float* u,
                  float* probs, int ld_probs, float* pixels, int ld_pixels, float* const* h_out, int n_out) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (n < 0) return fail(h, IWAE_EINVAL, "n must not be negative");
  if (!probs && !pixels) return fail(h, IWAE_EINVAL, "probs and pixels are both NULL");
  CHK(ld_ok(h, probs, ld_probs, "probs"));
  CHK(ld_ok(h, pixels, ld_pixels, "pixels"));
  const bool injected = eps && n_eps > 0;
  const int need = h_top ? L - 1 : L;
  if (n_eps != 0 && n_eps != need)
    return fail(h, IWAE_EINVAL, "expected " + std::to_string(need) + " eps buffers (" +
                                   (h_top ? "the prior draws" : "h_L, then the prior draws") + "), got " +
                                   std::to_string(n_eps));
  if (n_eps != 0 && !eps) return fail(h, IWAE_EINVAL, "eps is NULL");
  for (int i = 0; injected && i < n_eps; ++i)
    if (!eps[i]) return fail(h, IWAE_EINVAL, "NULL eps buffer");
  const bool keep = h_out && n_out > 0;
  if (n_out != 0 && (!h_out || n_out != L))
    return fail(h, IWAE_EINVAL, "expected one h_out buffer per stochastic layer");
  for (int i = 0; keep && i < L; ++i)
    if (!h_out[i]) return fail(h, IWAE_EINVAL, "NULL h_out buffer");
  if (n == 0) return IWAE_OK;
  const float* eps_top = (injected && !h_top) ? eps[0] : nullptr;
  const float* const* eps_pri = injected ? eps + (h_top ? 0 : 1) : nullptr;   // prior layer j's
  GnLaunch G;
  int rt = 0;
  size_t lds = 0;
  if (h->x3 && h->path != 1 && gen_plan(h, G, rt, lds)) {
    CHK(ensure_fx(h));
    G.n = n;
    G.h_top = h_top; G.eps_top = eps_top; G.top_out = keep ? h_out[L - 1] : nullptr;
    for (int j = 0; j < L - 1; ++j) {
      GnStage& S = G.st[3 * j + 2];
      S.eps = eps_pri ? eps_pri[j] : nullptr;
      S.h_out = keep ? h_out[L - 2 - j] : nullptr;
    }
    G.probs = probs; G.ld_probs = ld_probs; G.pixels = pixels; G.ld_pixels = ld_pixels; G.u = u;
    G.seed = h->seed; G.rng_base = &h->ds->rng[0]; G.ticket = &h->ds->tickets[3];
    HIPCHK(launch_gen(h->stream, G, rt, lds));
    ++h->count.gen;
    return IWAE_OK;
  }
  // layer-wise: the GEMM and Gaussian launches of iwae_reconstruct's generate_x
  // (exact f32 products under iwae_set_precision 0), the same Philox counters
  if (h->x3) CHK(ensure_wsplit(h));
  CHK(ensure_capacity(h, 1, n, false));
  const int dL = h->enc[L - 1].d;
  HIPCHK(launch_gen_top(h->stream, h_top ? h_top : eps_top, n, dL, h->h[L - 1].p, h->h[L - 1].ld,
                        keep ? h_out[L - 1] : nullptr, h->seed, &h->ds->rng[0], IWAE_MAX_LAYERS + L - 1));
  CHK(prior_chain_fwd(h, n, eps_pri, keep ? h_out : nullptr));
  CHK(out_hidden(h, n));
  Mat pm;                                        // the logits, then the probabilities, in the caller's buffer
  pm.p = probs ? probs : pixels; pm.ld = probs ? ld_probs : ld_pixels;
  CHK(out_probs(h, n, pm.p, pm.ld));
  if (pixels)
    HIPCHK(launch_gen_pixels(h->stream, pm.p, pm.ld, u, n, h->xdim, pixels, ld_pixels, h->seed, &h->ds->rng[0],
                             2 * IWAE_MAX_LAYERS));
  HIPCHK(launch_rng_advance(h->stream, &h->ds->rng[0]));
  return IWAE_OK;
}

// Dynamic binarisation: one gather-and-draw launch on the caller's buffers (no
// workspace, no plan), then the noise position's advance.
int iwae_binarize(iwae_handle* h, const float* x, long long n_src, const long long* perm, int n, const float* u,
                  float* out, int ld_out) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (!out) return fail(h, IWAE_EINVAL, "out is NULL");
  if (n < 0 || n > (1 << 24)) return fail(h, IWAE_EINVAL, "n must be in [0, 2^24]");
  if (n_src < 0) return fail(h, IWAE_EINVAL, "n_src must not be negative");
  if (!perm && n > n_src) return fail(h, IWAE_EINVAL, "n > n_src needs perm");
  CHK(ld_ok(h, out, ld_out, "out"));
  if ((long long)n * ((h->xdim + 3) >> 2) + 255 >= (1LL << 32))
    return fail(h, IWAE_EINVAL, "n * ceil(x_dim / 4) must stay below 2^32 - 255 (one launch)");
  if (n == 0) return IWAE_OK;
  HIPCHK(launch_binarize(h->stream, x, n_src, perm, u, n, h->xdim, out, ld_out, h->seed, &h->ds->rng[0],
                         2 * IWAE_MAX_LAYERS + 3));
  ++h->count.binarize;
  HIPCHK(launch_rng_advance(h->stream, &h->ds->rng[0]));
  return IWAE_OK;
}

// ------------------------------------------------ importance-weighted posterior
// Plan of post_kernel for this model (iwae_posterior.hip).  LDS buffers: the
// latents some stage reads, h_0 .. h_{L-2} (h_0 alone when L = 1: ids 0 .. nl-1;
// the top latent of a deeper model is summed and stored by its epilogue and
// needs none), scratch P (id nl) and Q (id nl+1).
//   encoder i = 1..L-1:  h_{i-1} -> P (tanh) -> Q (tanh) -> head: sample h_i      (enc)
//   output MLP:          h_0 -> Q -> P -> Dense(x_dim): weighted probabilities    (out)
// The buffer widths are those of all these stages whatever the call wants, so
// whether the plan fits is a property of the model; only the wanted stages are
// emitted.  The partial vector is [h_1 | .. | h_L | probs].  Row strides of 8
// mod 16 dwords.  RT from {4, 2, 1}: the largest that fits 160 KB of LDS.
// False if RT = 1 does not fit.
static bool post_plan(iwae_handle* h, bool enc, bool out, PoLaunch& G, int& rt, size_t& lds) {
  const int L = h->L;
  std::memset(&G, 0, sizeof(G));
  const int nl = std::max(1, L - 1), bP = nl, bQ = nl + 1, nb = nl + 2;
  if (nb > kMgMaxBufs || 3 * L > kMgMaxStages) return false;
  ChainBufs W(nb);
  auto next = [&](bool emit) -> PoStage* { return emit ? &G.st[G.nst++] : nullptr; };
  const int d0 = h->enc[0].d;
  int off = d0;                                  // h_1's sums come first (the prologue's)
  for (int i = 1; i < L; ++i) {
    const StochL& E = h->enc[i];
    chain_stage(h, W, next(enc), E.l1, i - 1, bP, PO_TANH, h->dense[E.l2].ldF);
    chain_stage(h, W, next(enc), E.l2, bP, bQ, PO_TANH, h->dense[E.head].ldF);
    PoStage* S = next(enc);
    chain_head(h, W, S, E.head, bQ, i < nl ? i : -1, PO_SAMPLE, E.d, i);
    if (S) S->part_off = off;
    off += E.d;
  }
  chain_stage(h, W, next(out), h->o1, 0, bQ, PO_TANH, h->dense[h->o2].ldF);
  chain_stage(h, W, next(out), h->o2, bQ, bP, PO_TANH, h->dense[h->o3].ldF);
  PoStage* S3 = next(out);
  chain_stage(h, W, S3, h->o3, bP, -1, PO_OUT, 0);
  if (S3) S3->part_off = off;
  G.ld_part = r4(off + h->xdim);
  G.d0 = d0; G.h0_buf = 0; G.h0_next_k = r32(d0 + 1);
  W.widen(0, G.h0_next_k);
  // h_1 as f32 [rows][d0] in the scratch buffer the first stage does not write
  W.widen(bP, d0);
  W.widen(bQ, d0);
  G.stage_buf = (G.nst > 0 && G.st[0].out_buf == bQ) ? bP : bQ;
  for (int c : {4, 2, 1}) {
    const int R = 16 * c;
    const int o = W.layout(R, false, G.buf_ld, G.buf_off);
    lds = (size_t)o * sizeof(__bf16) + (size_t)R * sizeof(float);
    if (lds > 160 * 1024) continue;
    rt = c;
    G.w_off = o / 2;                             // the rows' weights, as floats, behind the buffers
    return true;
  }
  return false;
}

// Two passes per chunk of images (all k samples of an image in one chunk):
// pass 1 is nll_core's / iwae_nll_eps's forward and launch_lse, unchanged;
// then the weights kernel, and pass 2 on post_kernel (the rows recomputed from
// the same noise: the base launch_lse left in rng[1]) or, layer-wise, weighted
// sums over the h_i and o2 outputs pass 1 left in HBM.
//
// With a pixel mask (iwae_impute) pass 1 is the masked one -- the chunk's
// images staged by select, then the masked mega_fwd_kernel (never the weight
// ring) or impute_layerwise_fwd, whose stored logits become the second pass's
// probabilities -- pass 2 is the same, and two small epilogues follow: probs
// (the caller's x_mean) keeps x at the observed pixels, and x_draw is drawn
// from p(x | h_1 of the resampled sample) on the layer-wise GEMMs (n rows).
// mask == NULL is iwae_posterior launch for launch.
static int posterior_core(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                          const float* const* eps, int n_eps, const float* u, const float* u_pix,
                          float* const* h_mean, int n_mean, float* probs, int ld_probs, float* x_draw, int ld_draw,
                          float* const* h_sir, int n_sir, float* weights, float* ess, float* logpx) {
  const int L = h->L;
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  CHK(nk_ok(h, N, k));
  CHK(ptrs_ok(h, eps, n_eps, "eps", true));
  CHK(ptrs_ok(h, h_mean, n_mean, "h_mean", true));
  CHK(ptrs_ok(h, h_sir, n_sir, "h_sir", true));
  const bool injected = n_eps > 0, want_mean = n_mean > 0, want_sir = n_sir > 0, draw = x_draw != nullptr;
  if (!want_mean && !probs && !draw && !want_sir && !weights && !ess && !logpx)
    return fail(h, IWAE_EINVAL, "every output is NULL");
  CHK(ld_ok(h, probs, ld_probs, mask ? "x_mean" : "probs"));
  CHK(ld_ok(h, x_draw, ld_draw, "x_draw"));
  const bool need_sir = want_sir || draw;        // the SIR index, and h_1 of the resampled sample
  const bool second = want_mean || probs || need_sir;
  // ---- path and chunk
  FwdPlan F;
  MgLaunch& MG = F.MG;
  PoLaunch PO;
  int po_rt = 0;
  size_t po_lds = 0;
  const bool fused = h->x3 && h->nll_fused && h->path != 1 && !h->masked && mega_plan(h, MG, F.rt, F.waves, F.lds) &&
                     post_plan(h, want_mean || want_sir, probs != nullptr, PO, po_rt, po_lds);
  const int ldp = r4(h->xdim);                   // layer-wise: the rows' probabilities, at most 256 MB of them
  const bool rows_px = !fused && (probs || mask);          // (masked: the rows' logits, whatever the call wants)
  const int imgs = chunk_images(h, N, k, chunk, true, rows_px ? ldp * 4 : 0);
  if (!imgs) return IWAE_EINVAL;
  const int rows = imgs * k;
  Mat xm;                                        // fused masked calls: the -1 copy of the staged images
  ChunkWalk W(h, N, k, imgs, fused, x, mask, fused, &xm);
  CHK(ensure_capacity(h, W.sup, rows, false));
  if (h->x3) CHK(ensure_wsplit(h));
  if (fused) CHK(ensure_fx(h));
  F.ring = fused && !mask && k >= 128 && nring_plan(h, F.NR);
  // ---- workspace of its own (floats): w~, SIR indices, then the path's
  const int tiles = fused ? (k + 16 * po_rt - 1) / (16 * po_rt) : 0;
  const bool gather = !fused && injected && imgs < N;     // a chunk's [k][n][d] noise, contiguous
  const int d0 = h->enc[0].d, ldx = h->x_in.ld;
  WsLayout lay;
  const size_t o_wt = lay.take(weights ? 0 : rows), o_sir = lay.take(need_sir ? imgs : 0);
  const size_t o_part = lay.take(fused && second ? (size_t)imgs * tiles * PO.ld_part : 0);
  const size_t o_pw = lay.take(rows_px ? (size_t)rows * ldp : 0);
  size_t o_eps[IWAE_MAX_LAYERS] = {};
  for (int i = 0; i < L; ++i) o_eps[i] = lay.take(gather ? (size_t)rows * h->enc[i].d : 0);
  // masked calls: the -1 copy of the staged images (fused), the rows' Bernoulli sums (layer-wise),
  // h_1 of the resampled samples when the caller keeps no h_sir, and the draw's probabilities
  const size_t o_xm = lay.take(mask && fused ? (size_t)W.sup * ldx : 0);
  const size_t o_rs = lay.take(mask && !fused ? (size_t)rows * 4 : 0);
  const size_t o_h1 = lay.take(draw && !want_sir ? (size_t)imgs * d0 : 0);
  const size_t o_dp = lay.take(draw ? (size_t)imgs * ldp : 0);
  CHK(h->post_ws.reserve(h, lay.floats));
  float* ws = h->post_ws.p;
  int* sir = need_sir ? reinterpret_cast<int*>(ws + o_sir) : nullptr;
  xm.p = mask && fused ? ws + o_xm : nullptr; xm.ld = ldx;
  fwd_call_fields(h, F, injected ? eps : nullptr, N);
  for (int i = 0; i < 8; ++i) PO.eps[i] = MG.eps[i];
  PO.eps_N = N;
  for (; W.i0 < N; W.i0 += imgs) {
    CHK(walk_step(h, W));
    const int i0 = W.i0, n = W.n;
    const float* xc = x + (size_t)i0 * h->xdim;                         // the chunk's images and mask rows
    const float* mc = mask ? mask + (size_t)i0 * h->xdim : nullptr;
    // ---- pass 1: the chunk's log weights and (m, sum e), as nll_core / iwae_nll_eps
    Plan P;
    P.B = n; P.Bimg = n; P.Bsplit = n; P.kS = k;
    LseArgs a = lse_args(h, k, n, true);
    if (fused) {
      if (mask) {
        chunk_rows(h, W, k, xm, MG);
        MG.eps_i0 = i0; MG.eps_s0 = 0;
        HIPCHK(launch_mega_fwd_masked(h->stream, MG, F.rt, F.waves, F.lds));
        ++h->count.imp;
      } else {
        CHK(launch_fwd_chunk(h, F, W, P, 0, injected));
      }
      a.lw = h->lw;
    } else {
      EpsSet E;
      CHK(chunk_eps(h, W, injected ? eps : nullptr, gather, ws, o_eps, E));
      if (mask) {
        Mat Z;
        Z.p = ws + o_pw; Z.ld = ldp;
        CHK(impute_layerwise_fwd(h, P, E, mc, Z, ws + o_rs, probs != nullptr));
        ++h->count.imp_lw;
      } else {
        CHK(forward_core(h, P, E, false));
      }
    }
    if (mask && !fused) { a.part = ws + o_rs; a.ldpart = 4; a.npart = 1; }
    HIPCHK(launch_lse(h->stream, a));
    if (logpx) HIPCHK(launch_lse_final(h->stream, h->run_m, h->run_s, n, logf((float)k), logpx + i0));
    if (!second && !weights && !ess) continue;
    // ---- the weights (pass 1 drew with the base now in rng[1])
    PostWArgs w{};
    w.src = a;
    w.wt = weights ? weights + (size_t)i0 * k : ws + o_wt;
    w.ess = ess ? ess + i0 : nullptr;
    w.sir = sir;
    w.u = u ? u + i0 : nullptr;
    w.seed = h->seed; w.rng_base = &h->ds->rng[1]; w.u_layer = 2 * IWAE_MAX_LAYERS + 1;
    HIPCHK(launch_post_weights(h->stream, w));
    if (!second) continue;
    // where layer i's resampled latents go: the caller's buffer, or (h_1, for the draw alone) the workspace
    auto sel = [&](int i) -> float* {
      if (want_sir) return h_sir[i] + (size_t)i0 * h->enc[i].d;
      return draw && i == 0 ? ws + o_h1 : nullptr;
    };
    // ---- pass 2
    if (fused) {
      PO.Bimg = n; PO.kS = k; PO.tiles = tiles;
      PO.P0 = MG.P0; PO.ldP0 = MG.ldP0;
      PO.seed = h->seed; PO.rng_base = &h->ds->rng[1];
      PO.eps_i0 = i0;
      PO.wt = w.wt; PO.sir = sir;
      for (int i = 0; i < L; ++i) PO.h_sir[i] = sel(i);
      PO.want_mean = want_mean;
      PO.part = ws + o_part;
      HIPCHK(launch_post(h->stream, PO, po_rt, po_lds));
      ++h->count.post;
      PoMerge M{};
      M.part = PO.part; M.ld_part = PO.ld_part; M.tiles = tiles; M.Bimg = n;
      int po = 0;
      for (int i = 0; i < L; ++i) {
        const int d = h->enc[i].d;
        if (want_mean) {
          M.off[M.nseg] = po; M.width[M.nseg] = d; M.ldo[M.nseg] = d;
          M.out[M.nseg++] = h_mean[i] + (size_t)i0 * d;
        }
        po += d;
      }
      if (probs) {
        M.off[M.nseg] = po; M.width[M.nseg] = h->xdim; M.ldo[M.nseg] = ld_probs;
        M.out[M.nseg++] = probs + (size_t)i0 * ld_probs;
      }
      HIPCHK(launch_post_merge(h->stream, M));
    } else {
      ++h->count.post_lw;
      for (int i = 0; (want_mean || need_sir) && i < L; ++i) {
        const int d = h->enc[i].d;
        HIPCHK(launch_group_wsum(h->stream, h->h[i].p, h->h[i].ld, k, d, n, w.wt,
                                 want_mean ? h_mean[i] + (size_t)i0 * d : nullptr, d, sir, sel(i), d));
      }
      if (probs) {
        // the output MLP's o1 / o2 outputs of these rows are pass 1's (its Bernoulli GEMM read them from
        // ob.y2): the output Dense again, storing the logits (masked: pass 1 left the rows' probabilities there)
        if (!mask) CHK(out_probs(h, n * k, ws + o_pw, ldp));
        HIPCHK(launch_group_wsum(h->stream, ws + o_pw, ldp, k, h->xdim, n, w.wt, probs + (size_t)i0 * ld_probs,
                                 ld_probs, nullptr, nullptr, 0));
      }
    }
    if (!mask) continue;
    // ---- imputation epilogues
    if (probs) HIPCHK(launch_impute_fill(h->stream, xc, mc, n, h->xdim, probs + (size_t)i0 * ld_probs, ld_probs));
    if (draw) {
      // p(x | h_1) of the n resampled rows: the output MLP layer-wise (every
      // reader of this chunk's h[0] / ob rows is ahead on the stream)
      HIPCHK(hipMemcpy2DAsync(h->h[0].p, (size_t)h->h[0].ld * sizeof(float), sel(0), (size_t)d0 * sizeof(float),
                              (size_t)d0 * sizeof(float), n, hipMemcpyDeviceToDevice, h->stream));
      CHK(out_hidden(h, n));
      CHK(out_probs(h, n, ws + o_dp, ldp));
      HIPCHK(launch_impute_draw(h->stream, xc, mc, ws + o_dp, ldp, u_pix ? u_pix + (size_t)i0 * h->xdim : nullptr, n,
                                h->xdim, x_draw + (size_t)i0 * ld_draw, ld_draw, h->seed, &h->ds->rng[1],
                                2 * IWAE_MAX_LAYERS + 2));
    }
  }
  return IWAE_OK;
}

int iwae_posterior(iwae_handle* h, const float* x, int N, int k, int chunk, const float* const* eps, int n_eps,
                   const float* u, float* const* h_mean, int n_mean, float* probs, int ld_probs,
                   float* const* h_sir, int n_sir, float* weights, float* ess, float* logpx) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  return posterior_core(h, x, nullptr, N, k, chunk, eps, n_eps, u, nullptr, h_mean, n_mean, probs, ld_probs, nullptr, 0,
                        h_sir, n_sir, weights, ess, logpx);
}

// Imputation of missing pixels (Mattei & Frellsen 2019): iwae_posterior under
// the likelihood of the observed pixels alone.
int iwae_impute(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk, const float* const* eps,
                int n_eps, const float* u, const float* u_pix, float* x_mean, int ld_mean, float* x_draw, int ld_draw,
                float* const* h_mean, int n_mean, float* const* h_sir, int n_sir, float* weights, float* ess,
                float* logpx) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!mask) return fail(h, IWAE_EINVAL, "mask is NULL (an all-observed call is iwae_posterior's)");
  return posterior_core(h, x, mask, N, k, chunk, eps, n_eps, u, u_pix, h_mean, n_mean, x_mean, ld_mean, x_draw, ld_draw,
                        h_sir, n_sir, weights, ess, logpx);
}

// ------------------------------------------------ scoring given latents
// score_kernel's launch from mega_fwd_kernel's plan MG (same buffers, row
// tiles and LDS): the chains of the outputs asked for, heads as density heads.
// mega_plan's stage order: encoder layers 1 .. L-1, prior layers 0 .. L-2, the
// output MLP, three stages each.
static void score_plan(const iwae_handle* h, const MgLaunch& MG, bool q, bool ph, bool out, ScLaunch& S) {
  const int L = h->L;
  static_cast<MgLaunch&>(S) = MG;
  S.nst = 0;
  S.n_lat = L;
  for (int i = 0; i < 8; ++i) { S.lat_d[i] = i < L ? h->enc[i].d : 0; S.lat_buf[i] = -1; S.lat_next_k[i] = 0; }
  auto chain = [&](int s0, int src, int act, int target) {      // src: the latent the chain reads
    for (int u = 0; u < 3; ++u) S.st[S.nst + u] = MG.st[s0 + u];
    S.lat_buf[src] = MG.st[s0].in_buf;
    S.lat_next_k[src] = std::max(S.lat_next_k[src], MG.st[s0].ldk);
    MgStage& H = S.st[S.nst + 2];
    H.act = act; H.layer = target; H.stdnormal = 0;
    S.nst += 3;
  };
  const int e0 = 0, d0 = 3 * (L - 1), o0 = 6 * (L - 1);
  // (the first prior chain reads h_L from the scratch buffer the encoder chains write: it goes first)
  if (ph && L > 1) chain(d0, L - 1, MG_DENSP, L - 2);
  for (int i = 1; q && i < L; ++i) chain(e0 + 3 * (i - 1), i - 1, MG_DENSQ, i);
  for (int j = 1; ph && j < L - 1; ++j) chain(d0 + 3 * j, L - 1 - j, MG_DENSP, L - 2 - j);
  if (out) chain(o0, 0, MG_BERNS, 0);
  S.want_q = q ? 1 : 0;
  S.want_ph = ph ? 1 : 0;
}

// iwae_score and iwae_score_masked (mask: [N][x_dim], non-zero = observed; null: none)
static int score_core(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                      const float* const* lat, int n_lat, float* log_q, float* log_ph, float* log_px, float* probs,
                      int ld_probs) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (!log_q && !log_ph && !log_px && !probs) return fail(h, IWAE_EINVAL, "every output is NULL");
  if (!x && (log_q || log_px)) return fail(h, IWAE_EINVAL, "x is NULL (log_q and log_px need the images)");
  CHK(ptrs_ok(h, lat, n_lat, "latent", false));
  CHK(ld_ok(h, probs, ld_probs, "probs"));
  const int imgs = chunk_images(h, N, k, chunk);
  if (!imgs) return IWAE_EINVAL;
  const bool want_out = log_px || probs;
  MgLaunch MG;
  int mg_rt = 0, mg_waves = 8;
  size_t mg_lds = 0;
  const bool fused = h->x3 && h->nll_fused && h->path != 1 && !h->masked && mega_plan(h, MG, mg_rt, mg_waves, mg_lds);
  // fused: the first encoder layer runs once per group of images, as nll_core's; no row buffer is used
  ChunkWalk W(h, N, k, imgs, fused, x, mask, log_q != nullptr);
  CHK(ensure_capacity(h, W.sup, fused ? 1 : imgs * k, false));
  if (h->x3) CHK(ensure_wsplit(h));
  if (fused) CHK(ensure_fx(h));
  ScLaunch SC;
  if (fused) {
    score_plan(h, MG, log_q != nullptr, log_ph != nullptr, want_out, SC);
    for (int i = 0; i < 8; ++i) SC.eps[i] = i < L ? lat[i] : nullptr;
    SC.eps_N = N; SC.eps_s0 = 0;
    SC.rng_base = nullptr; SC.seed = 0; SC.lw = nullptr;
  }
  const Mat& xl = mask ? h->x_lik : h->x_in;      // the likelihood's copy of the images
  for (; W.i0 < N; W.i0 += imgs) {
    CHK(walk_step(h, W));
    const int i0 = W.i0, M = W.n * k;
    const size_t r0 = W.r0;
    if (fused) {
      chunk_rows(h, W, k, xl, SC);
      SC.eps_i0 = i0;
      SC.log_q = log_q ? log_q + r0 : nullptr;
      SC.log_ph = log_ph ? log_ph + r0 : nullptr;
      SC.log_px = log_px ? log_px + r0 : nullptr;
      SC.probs = probs ? probs + r0 * ld_probs : nullptr; SC.ld_probs = ld_probs;
      if (mask) {
        HIPCHK(launch_score_masked(h->stream, SC, mg_rt, mg_waves, mg_lds));
        ++h->count.score_pix;
      } else {
        HIPCHK(launch_score(h->stream, SC, mg_rt, mg_waves, mg_lds));
        ++h->count.score;
      }
      continue;
    }
    // ---- layer-wise: the latents into the workspace's rows, then forward_core's launches as density passes
    ++(mask ? h->count.score_pix_lw : h->count.score_lw);
    CHK(gather_latents(h, W, lat));
    for (int i = 0; log_q && i < L; ++i) {
      if (i > 0) CHK(stoch_fwd(h, h->enc[i], h->h[i - 1], M, h->eb[i]));
      CHK(gauss_logdens(h, h->eb[i].P, i == 0 ? k : 1, h->enc[i].d, h->h[i], log_q + r0, i > 0, M));
    }
    if (log_ph) CHK(prior_fwd(h, M, log_ph + r0));
    if (want_out) CHK(out_hidden(h, M));
    if (log_px) {
      Mat none;
      CHK(gemm_fwd(h, mask ? EPI_BERN_MASK : EPI_BERN, h->ob.y2, M, h->dense[h->o3], none, bern_args(h, xl, k, 1.f)));
      HIPCHK(launch_score_rowsum(h->stream, h->part, h->ldpart, h->npart, M, log_px + r0));
    }
    if (probs) CHK(out_probs(h, M, probs + r0 * ld_probs, ld_probs));
  }
  return IWAE_OK;
}

int iwae_score(iwae_handle* h, const float* x, int N, int k, int chunk, const float* const* lat, int n_lat,
               float* log_q, float* log_ph, float* log_px, float* probs, int ld_probs) {
  return score_core(h, x, nullptr, N, k, chunk, lat, n_lat, log_q, log_ph, log_px, probs, ld_probs);
}

// pixel-masked entries of this family: the checks they add (the siblings' own follow)
static int check_observed(iwae_handle* h, const float* x, const float* mask) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!mask) return fail(h, IWAE_EINVAL, "mask is NULL");
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL (a call that needs no images has no use for a mask)");
  return IWAE_OK;
}

int iwae_score_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                      const float* const* lat, int n_lat, float* log_q, float* log_ph, float* log_px, float* probs,
                      int ld_probs) {
  CHK(check_observed(h, x, mask));
  return score_core(h, x, mask, N, k, chunk, lat, n_lat, log_q, log_ph, log_px, probs, ld_probs);
}

// sg_kernel's plan (SgLaunch, iwae_kernels.h): the chains of the terms that are needed, each forward
// and, where its gradient is asked for, straight back.  False when it does not fit 160 KiB of LDS
// at any row tile, or its stage list or the output chain's column tiles exceed the kernel's limits.
static bool sgrad_plan(const iwae_handle* h, bool run_q, bool run_ph, bool run_px, float cq, float cph, float cpx,
                       SgLaunch& S, int& rt, size_t& lds) {
  const int L = h->L;
  std::memset(&S, 0, sizeof(S));
  const int bA = L, bB = L + 1, bP = L + 2, nb = L + 3;
  if (nb > kMgMaxBufs || L > 8) return false;
  ChainBufs W(nb);
  std::vector<SgStage> st;
  auto fwd = [&](int di, int in, int out, int kind, int next_k) {
    const DenseL& d = h->dense[di];
    SgStage T{};
    T.woff = (unsigned)d.fx_off; T.ldk = (short)d.ldF; T.N = (short)d.fout;
    T.in_buf = (signed char)in; T.out_buf = (signed char)out; T.kind = (signed char)kind; T.next_k = (short)next_k;
    W.dense(d.ldF, d.fout, in, kind == SG_TANH ? out : -1, next_k);
    st.push_back(T);
    return (int)st.size() - 1;
  };
  auto bwd = [&](int di, int in, int out, int kind, int layer) {
    const DenseL& d = h->dense[di];
    SgStage T{};
    T.woff = (unsigned)d.gx_off; T.ldk = (short)(32 * d.gx_steps); T.N = (short)d.fin;
    T.in_buf = (signed char)in; T.out_buf = (signed char)out; T.kind = (signed char)kind; T.layer = (signed char)layer;
    W.dense(32 * d.gx_steps, d.fin, in, out, 0);
    st.push_back(T);
  };
  for (int i = 0; i < 8; ++i) { S.lat_d[i] = i < L ? h->enc[i].d : 0; S.lat_buf[i] = -1; S.lat_next_k[i] = 0; }
  auto chain = [&](const StochL& C, int src, int target, int kind, float c) {
    fwd(C.l1, src, bA, SG_TANH, h->dense[C.l2].ldF);
    fwd(C.l2, bA, bB, SG_TANH, h->dense[C.head].ldF);
    const int gk = 32 * h->dense[C.head].gx_steps;
    const int s = fwd(C.head, bB, bP, kind, gk);
    st[s].N = (short)(8 * ((C.d + 3) / 4)); st[s].d = (short)C.d; st[s].layer = (signed char)target; st[s].c = c;
    S.lat_buf[src] = src;
    S.lat_next_k[src] = std::max(S.lat_next_k[src], h->dense[C.l1].ldF);
    if (c == 0.f) return;
    W.widen(bP, std::max(gk, 2 * C.d));
    bwd(C.head, bP, bB, SG_GTANH, 0);
    bwd(C.l2, bB, bA, SG_GTANH, 0);
    bwd(C.l1, bA, -1, SG_GX, src);
  };
  for (int i = 1; run_q && i < L; ++i) chain(h->enc[i], i - 1, i, SG_HEADQ, cq);
  for (int j = 0; run_ph && j < L - 1; ++j) chain(h->dec[j], L - 1 - j, L - 2 - j, SG_HEADP, cph);
  if (run_px) {
    fwd(h->o1, 0, bA, SG_TANH, h->dense[h->o2].ldF);
    fwd(h->o2, bA, bB, SG_TANH, h->dense[h->o3].ldF);
    const int s = fwd(h->o3, bB, bP, SG_OUT, 0);
    st[s].c = cpx;
    S.lat_buf[0] = 0;
    S.lat_next_k[0] = std::max(S.lat_next_k[0], h->dense[h->o1].ldF);
    const DenseL& d3 = h->dense[h->o3];
    S.out_gx_woff = (int)d3.gx_off; S.out_gx_ldk = 32 * d3.gx_steps; S.out_gx_N = d3.fin;
    if (cpx != 0.f) {
      if ((d3.fin + 15) / 16 > kSgOutTiles * kSgWaves) return false;
      W.widen(bP, 256);
      bwd(h->o2, bB, bA, SG_GTANH, 0);
      bwd(h->o1, bA, -1, SG_GX, 0);
    }
  }
  if ((int)st.size() > kSgMaxStages) return false;
  for (const SgStage& T : st)
    if (T.ldk > 32000 || T.N > 32000) return false;
  for (int i = 0; i < L; ++i)
    if (S.lat_buf[i] >= 0) W.widen(i, S.lat_next_k[i]);
  // LDS: the bf16 buffers (mega_plan's strides), the f32 gradient tiles, logq / logp
  for (int c : {4, 2, 1}) {
    const int R = 16 * c;
    for (int pass = 0; pass < 2; ++pass) {
      const int off = W.layout(R, pass == 1, S.buf_ld, S.buf_off);
      int foff = (off + 3) / 2 & ~1;            // floats
      foff = std::max(foff, 3 * kSgWaves * R);  // (the value sums' scratch reuses the buffers)
      for (int i = 0; i < L; ++i) {
        S.g_ld[i] = h->enc[i].d | 1;            // odd stride: the rows' columns spread over the banks
        S.g_off[i] = foff;
        foff += R * S.g_ld[i];
      }
      S.acc_off = foff;
      const size_t bytes = (size_t)(S.acc_off + 2 * R) * sizeof(float);
      if (bytes <= 160 * 1024) {
        rt = c;
        lds = bytes;
        for (size_t i = 0; i < st.size(); ++i) S.st[i] = st[i];
        S.nst = (int)st.size();
        S.n_lat = L;
        S.fx_hi = h->fx_hi; S.fx_lo = h->fx_lo; S.fx_elems = h->fx_elems;
        return true;
      }
    }
  }
  return false;
}

// Gradients of the scored densities with respect to the latents (include/iwae.h).
// Fused: one sg_kernel launch per chunk (sgrad_plan).  Layer-wise: iwae_score's
// gather and forward launches, then per chain the head gradients
// (sg_dens_kernel) and three backward-data GEMMs, the output MLP's Bernoulli
// epilogue writing c_px dlogit, and one scatter launch; its backward rows live
// in a workspace of the call's own (sg_ws), so the arena and what was captured
// over it stay as they are.
// (mask: iwae_score_grad_masked's, [N][x_dim], non-zero = observed; null: none)
static int sgrad_core(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                      const float* const* lat, int n_lat, const float coef[3], float* const* grad, int n_grad,
                      float* log_q, float* log_ph, float* log_px) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (n_grad == 0 && !log_q && !log_ph && !log_px) return fail(h, IWAE_EINVAL, "every output is absent");
  if (!coef) return fail(h, IWAE_EINVAL, "coef is NULL");
  for (int t = 0; t < 3; ++t)
    if (!std::isfinite(coef[t])) return fail(h, IWAE_EINVAL, "coef must be finite");
  CHK(ptrs_ok(h, lat, n_lat, "latent", false));
  if (n_grad != 0 && (n_grad != L || !grad))
    return fail(h, IWAE_EINVAL, "expected 0 or " + std::to_string(L) + " gradient buffers, got " + std::to_string(n_grad));
  for (int i = 0; n_grad && i < L; ++i)
    if (!grad[i]) return fail(h, IWAE_EINVAL, "NULL gradient buffer");
  const bool want_g = n_grad > 0;
  const float cq = coef[0], cph = coef[1], cpx = coef[2];
  const bool gq = want_g && cq != 0.f, gph = want_g && cph != 0.f, gpx = want_g && cpx != 0.f;
  const bool run_q = gq || log_q, run_ph = gph || log_ph, run_px = gpx || log_px;
  if (!x && (run_q || run_px))
    return fail(h, IWAE_EINVAL, "x is NULL (log q and log p(x|h), values or gradient terms, need the images)");
  int imgs = chunk_images(h, N, k, chunk);
  if (!imgs) return IWAE_EINVAL;
  const Mat& xl = mask ? h->x_lik : h->x_in;      // the likelihood's copy of the images
  // ---- fused: one sg_kernel launch per chunk where iwae_score's fused path applies and the plan fits
  {
    MgLaunch MG;
    SgLaunch SG;
    int mg_rt = 0, mg_waves = 8, sg_rt = 0;
    size_t mg_lds = 0, sg_lds = 0;
    const bool fused = h->x3 && h->nll_fused && h->path != 1 && !h->masked && mega_plan(h, MG, mg_rt, mg_waves, mg_lds) &&
                       sgrad_plan(h, run_q, run_ph, run_px, gq ? cq : 0.f, gph ? cph : 0.f, gpx ? cpx : 0.f, SG, sg_rt,
                                  sg_lds);
    if (fused) {
      // the first encoder layer runs once per group of images, as iwae_score's; no row buffer is used
      ChunkWalk W(h, N, k, imgs, true, x, mask, run_q);
      CHK(ensure_capacity(h, W.sup, 1, false));
      CHK(ensure_wsplit(h));
      CHK(ensure_fx(h));
      SG.fx_hi = h->fx_hi; SG.fx_lo = h->fx_lo; SG.fx_elems = h->fx_elems;
      for (int i = 0; i < 8; ++i) { SG.lat[i] = i < L ? lat[i] : nullptr; SG.grad[i] = i < L && want_g ? grad[i] : nullptr; }
      SG.lat_N = N;
      SG.cq = gq ? cq : 0.f; SG.cph = gph ? cph : 0.f;
      SG.want_q = log_q ? 1 : 0; SG.want_ph = log_ph ? 1 : 0;
      for (; W.i0 < N; W.i0 += imgs) {
        CHK(walk_step(h, W));
        const size_t r0 = W.r0;
        chunk_rows(h, W, k, xl, SG);
        SG.lat_i0 = W.i0;
        SG.log_q = log_q ? log_q + r0 : nullptr;
        SG.log_ph = log_ph ? log_ph + r0 : nullptr;
        SG.log_px = log_px ? log_px + r0 : nullptr;
        if (mask) {
          HIPCHK(launch_sgrad_masked(h->stream, SG, sg_rt, sg_lds));
          ++h->count.sgrad_pix;
        } else {
          HIPCHK(launch_sgrad(h->stream, SG, sg_rt, sg_lds));
          ++h->count.sgrad;
        }
      }
      return IWAE_OK;
    }
  }
  const int ldp = r4(h->xdim), Ho = h->dense[h->o1].fout;
  // a chunk's dlogits: at most 256 MB of them (iwae_posterior's rule for its rows of probabilities)
  if (gpx) imgs = cap_chunk_bytes(imgs, k, ldp * 4);
  const int rows = imgs * k;
  CHK(ensure_capacity(h, imgs, rows, false));
  if (h->x3) CHK(ensure_wsplit(h));
  // ---- the backward rows (floats; laid out for the largest chunk so far).  One dP per head width and
  // one dY2 / dY1 pair per hidden width: a buffer's columns past its logical width are never written
  // and stay zero, as the arena's (the GEMMs read A in quads)
  Mat dlogit, Xo, Tq[IWAE_MAX_LAYERS], Xq[IWAE_MAX_LAYERS], Tp[IWAE_MAX_LAYERS], Xp[IWAE_MAX_LAYERS];
  std::map<int, Mat> dPs, dY2s, dY1s;
  if (want_g) {
    const int R = std::max(rows, h->sg_rows);
    WsLayout lay;
    std::vector<Mat*> all;
    auto mat = [&](Mat& m, int width) {
      m.ld = r4(width);
      m.p = nullptr;
      all.push_back(&m);
      return lay.take((size_t)R * m.ld);
    };
    std::vector<size_t> offs;
    auto hid = [&](int H) {
      if (dY2s.count(H)) return;
      offs.push_back(mat(dY2s[H], H)); offs.push_back(mat(dY1s[H], H));
    };
    auto head = [&](int d) {
      if (!dPs.count(d)) offs.push_back(mat(dPs[d], 2 * d));
    };
    for (int i = 1; i < L; ++i) { hid(h->enc[i].H); head(h->enc[i].d); }
    for (int i = 0; i < L - 1; ++i) { hid(h->dec[i].H); head(h->dec[i].d); }
    hid(Ho);
    offs.push_back(mat(Xo, h->enc[0].d));
    for (int i = 0; i < L; ++i)
      for (Mat* m : {&Tq[i], &Xq[i], &Tp[i], &Xp[i]}) offs.push_back(mat(*m, h->enc[i].d));
    const size_t small = lay.floats;
    offs.push_back(mat(dlogit, h->xdim));                         // last and largest: present once a call needs it
    // (more rows are a new layout: allocated afresh and zeroed whatever the size)
    CHK(h->sg_ws.reserve(h, gpx ? lay.floats : small, true, R > h->sg_rows));
    h->sg_rows = R;
    for (size_t i = 0; i < all.size(); ++i) all[i]->p = h->sg_ws.p + offs[i];
    if (!gpx) dlogit = Mat();
  }
  // dP (one chain's head gradients) back through head -> l2 -> l1 into dx
  auto chain_bwd = [&](const StochL& s, int M, LayerBufs& b, Mat& dx) {
    Mat &dY2 = dY2s[s.H], &dY1 = dY1s[s.H];
    CHK(gemm_bwd_data(h, dPs[s.d], M, h->dense[s.head], dY2, &b.y2, nullptr));
    CHK(gemm_bwd_data(h, dY2, M, h->dense[s.l2], dY1, &b.y1, nullptr));
    CHK(gemm_bwd_data(h, dY1, M, h->dense[s.l1], dx, nullptr, nullptr));
    return IWAE_OK;
  };
  auto dens = [&](const Mat& P, int prow_div, int d, const Mat& H, Mat& tg, bool with_dP, int M) {
    SgDens a{};
    a.P = P.p; a.ldP = P.ld; a.prow_div = prow_div; a.d = d;
    a.H = H.p; a.ldH = H.ld;
    a.tg = tg.p; a.ldtg = tg.ld;
    if (with_dP) { a.dP = dPs[d].p; a.lddP = dPs[d].ld; }
    a.M = M;
    HIPCHK(launch_sg_dens(h->stream, a));
    return IWAE_OK;
  };
  for (ChunkWalk W(h, N, k, imgs, false, x, mask, run_q); W.i0 < N; W.i0 += imgs) {
    CHK(walk_step(h, W));
    const int i0 = W.i0, n = W.n, M = n * k;
    const size_t r0 = W.r0;                      // the chunk's first row of the [N][k] outputs
    ++(mask ? h->count.sgrad_pix_lw : h->count.sgrad_lw);
    CHK(gather_latents(h, W, lat));
    // ---- log q: chain i scores h_{i+1} under enc_i(h_i); its dX is h_i's
    for (int i = 0; run_q && i < L; ++i) {
      if (i > 0) CHK(stoch_fwd(h, h->enc[i], h->h[i - 1], M, h->eb[i]));
      if (log_q) CHK(gauss_logdens(h, h->eb[i].P, i == 0 ? k : 1, h->enc[i].d, h->h[i], log_q + r0, i > 0, M));
      if (!gq) continue;
      CHK(dens(h->eb[i].P, i == 0 ? k : 1, h->enc[i].d, h->h[i], Tq[i], i > 0, M));
      if (i > 0) CHK(chain_bwd(h->enc[i], M, h->eb[i], Xq[i - 1]));
    }
    // ---- log p(h): -h_L in the scatter; chain j scores h_{L-1-j} under dec_j(h_{L-j})
    if (log_ph) {
      GaussArgs g{};
      g.d = h->enc[L - 1].d; g.H = h->h[L - 1].p; g.ldH = h->h[L - 1].ld;
      g.out = log_ph + r0; g.accumulate = 0; g.M = M;
      HIPCHK(launch_gauss_fwd(h->stream, 2, g));
    }
    for (int j = 0; run_ph && j < L - 1; ++j) {
      const int src = L - 1 - j, t = L - 2 - j;
      CHK(stoch_fwd(h, h->dec[j], h->h[src], M, h->db[j]));
      if (log_ph) CHK(gauss_logdens(h, h->db[j].P, 1, h->dec[j].d, h->h[t], log_ph + r0, true, M));
      if (!gph) continue;
      CHK(dens(h->db[j].P, 1, h->dec[j].d, h->h[t], Tp[t], true, M));
      CHK(chain_bwd(h->dec[j], M, h->db[j], Xp[src]));
    }
    // ---- log p(x|h_1): the Bernoulli epilogue with the constant row weight c_px writes c_px dlogit
    if (run_px) {
      CHK(out_hidden(h, M));
      GemmArgs ex = bern_args(h, xl, k, gpx ? cpx : 1.f);
      ex.store_g = gpx ? 1 : 0;
      Mat gm;
      if (gpx) gm = dlogit;
      CHK(gemm_fwd(h, mask ? EPI_BERN_MASK : EPI_BERN, h->ob.y2, M, h->dense[h->o3], gm, ex));
      if (log_px) HIPCHK(launch_score_rowsum(h->stream, h->part, h->ldpart, h->npart, M, log_px + r0));
      if (gpx) {
        Mat &dY2 = dY2s[Ho], &dY1 = dY1s[Ho];
        CHK(gemm_bwd_data(h, dlogit, M, h->dense[h->o3], dY2, &h->ob.y2, nullptr));
        CHK(gemm_bwd_data(h, dY2, M, h->dense[h->o2], dY1, &h->ob.y1, nullptr));
        CHK(gemm_bwd_data(h, dY1, M, h->dense[h->o1], Xo, nullptr, nullptr));
      }
    }
    if (!want_g) continue;
    // ---- grad[i] = c_q (Tq_i + Xq_i) + c_ph (Tp_i + Xp_i) + Xo (i = 0) - c_ph h_L (i = L - 1), left to right
    SgScatter S{};
    S.n = n; S.k = k; S.N = N; S.i0 = i0; S.nlay = L;
    for (int i = 0; i < L; ++i) {
      SgLayer& y = S.lay[i];
      auto add = [&](const Mat& m, float c) { y.src[y.nsrc] = m.p; y.ld[y.nsrc] = m.ld; y.c[y.nsrc++] = c; };
      if (gq) add(Tq[i], cq);
      if (gq && i < L - 1) add(Xq[i], cq);
      if (gph && i < L - 1) add(Tp[i], cph);
      if (gph && i > 0) add(Xp[i], cph);
      if (gpx && i == 0) add(Xo, 1.f);
      y.c_top = gph && i == L - 1 ? cph : 0.f;
      y.lat = lat[i];
      y.out = grad[i]; y.d = h->enc[i].d;
    }
    HIPCHK(launch_sg_scatter(h->stream, S));
  }
  return IWAE_OK;
}

int iwae_score_grad(iwae_handle* h, const float* x, int N, int k, int chunk, const float* const* lat, int n_lat,
                    const float coef[3], float* const* grad, int n_grad, float* log_q, float* log_ph, float* log_px) {
  return sgrad_core(h, x, nullptr, N, k, chunk, lat, n_lat, coef, grad, n_grad, log_q, log_ph, log_px);
}

int iwae_score_grad_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk,
                           const float* const* lat, int n_lat, const float coef[3], float* const* grad, int n_grad,
                           float* log_q, float* log_ph, float* log_px) {
  CHK(check_observed(h, x, mask));
  return sgrad_core(h, x, mask, N, k, chunk, lat, n_lat, coef, grad, n_grad, log_q, log_ph, log_px);
}

// Annealed importance sampling (include/iwae.h): per transition one gradient
// pass at the state (iwae_score_grad, fused or layer-wise as it decides), the
// begin launch, then n_leapfrog passes at the proposal, each followed by the
// step launch or, the last, by the end launch (iwae_ais.hip); one finish launch
// per call.  Everything is enqueued on h->stream: coef is a host array and the
// chains' buffers (ais_ws) only grow, so the host waits only where a workspace
// grows.
// (mask: iwae_ais_masked's, handed to every gradient pass; null: none)
static int ais_core(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk, float* const* lat,
                    int n_lat, const iwae_ais_config* cfg, const float* betas, const float* const* mom, int n_mom,
                    const float* u, float* step_io, float* log_w, float* accepts, float* logpx, float* ess) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (!cfg) return fail(h, IWAE_EINVAL, "cfg is NULL");
  if (!betas) return fail(h, IWAE_EINVAL, "betas is NULL");
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  CHK(ptrs_ok(h, lat, n_lat, "latent", false));
  if (cfg->init != 0 && cfg->init != 1) return fail(h, IWAE_EINVAL, "init must be 0 (the prior) or 1 (q)");
  const int T = cfg->n_temps, nl = cfg->n_leapfrog;
  if (T < 1 || T > (1 << 24)) return fail(h, IWAE_EINVAL, "n_temps must be in [1, 2^24]");
  if (nl < 1) return fail(h, IWAE_EINVAL, "n_leapfrog must be at least 1");
  for (int t = 0; t <= T; ++t)
    if (!std::isfinite(betas[t]) || betas[t] < 0.f || betas[t] > 1.f)
      return fail(h, IWAE_EINVAL, "betas must be finite and in [0, 1]");
  if (!std::isfinite(cfg->step) || cfg->step <= 0.f)
    return fail(h, IWAE_EINVAL, "step must be positive and finite");
  if (!std::isfinite(cfg->adapt_inc) || !std::isfinite(cfg->adapt_dec) || cfg->adapt_inc <= 0.f || cfg->adapt_dec <= 0.f)
    return fail(h, IWAE_EINVAL, "adapt_inc and adapt_dec must be positive and finite");
  if (!(cfg->step_min <= cfg->step_max)) return fail(h, IWAE_EINVAL, "step_min must not exceed step_max");
  if (n_mom != 0 && ((long long)n_mom != (long long)T * L || !mom))
    return fail(h, IWAE_EINVAL, "expected 0 or n_temps * " + std::to_string(L) + " momentum buffers, got " +
                                   std::to_string(n_mom));
  for (int i = 0; i < n_mom; ++i)
    if (!mom[i]) return fail(h, IWAE_EINVAL, "NULL momentum buffer");
  if (!chunk_images(h, N, k, chunk)) return IWAE_EINVAL;
  const long long chains = (long long)N * k;
  if (chains > (1LL << 30)) return fail(h, IWAE_EINVAL, "N * k above 2^30 chains");
  // ---- the chains' buffers: per layer r, q, g [k][N][d_i]; per chain H_old, log q, log p(h), log p(x|h), and
  // the weights / steps where the caller gave none
  WsLayout lay;
  size_t o_r[IWAE_MAX_LAYERS], o_q[IWAE_MAX_LAYERS], o_g[IWAE_MAX_LAYERS];
  int dmax = 0;
  for (int i = 0; i < L; ++i) {
    const size_t n = (size_t)chains * h->enc[i].d;
    o_r[i] = lay.take(n); o_q[i] = lay.take(n); o_g[i] = lay.take(n);
    dmax = std::max(dmax, h->enc[i].d);
  }
  const size_t o_H = lay.take(chains), o_lq = lay.take(chains), o_lph = lay.take(chains), o_lpx = lay.take(chains);
  const size_t o_w = lay.take(chains), o_step = lay.take(chains);
  CHK(h->ais_ws.reserve(h, lay.floats));
  float* ws = h->ais_ws.p;
  AisArgs a{};
  a.L = L; a.N = N; a.k = k; a.chains = chains;
  a.group = dmax <= 64 ? 16 : 64;
  float* gbuf[IWAE_MAX_LAYERS];
  for (int i = 0; i < L; ++i) {
    a.d[i] = h->enc[i].d;
    a.vec[i] = (a.d[i] & 3) == 0;
    a.cur[i] = lat[i]; a.r[i] = ws + o_r[i]; a.q[i] = ws + o_q[i];
    a.g[i] = gbuf[i] = ws + o_g[i];
  }
  const int init = cfg->init;
  a.init = init;
  float* lq = init ? ws + o_lq : nullptr;          // (from the prior, log q enters neither the energy nor Delta)
  float *lph = ws + o_lph, *lpx = ws + o_lpx;
  a.lq = lq; a.lph = lph; a.lpx = lpx;
  a.H_old = ws + o_H;
  a.step = step_io ? step_io : ws + o_step;
  // logpx / ess are formed from the weights: in the workspace where the caller has no use for them
  a.log_w = log_w ? log_w : (logpx || ess) ? ws + o_w : nullptr;
  a.accepts = accepts;
  a.seed = h->seed; a.rng_base = &h->ds->rng[0];
  a.mom_layer = 2 * IWAE_MAX_LAYERS + 4; a.u_layer = 2 * IWAE_MAX_LAYERS + 12;
  a.inc = cfg->adapt_inc; a.dec = cfg->adapt_dec; a.smin = cfg->step_min; a.smax = cfg->step_max;
  if (cfg->accumulate && !log_w && a.log_w)        // no weights given, nothing to continue from: the workspace's start at 0
    HIPCHK(hipMemsetAsync(a.log_w, 0, (size_t)chains * sizeof(float), h->stream));
  for (int t = 1; t <= T; ++t) {
    const float beta = betas[t];
    const float coef[3] = {init ? 1.f - beta : 0.f, init ? beta : 1.f, beta};
    a.cq = coef[0]; a.cph = coef[1]; a.cpx = coef[2];
    a.dbeta = betas[t] - betas[t - 1];
    a.zero = t == 1 && !cfg->accumulate;
    a.step0 = t == 1 && !step_io ? cfg->step : 0.f;
    a.t_off = (unsigned)(t - 1);
    for (int i = 0; i < L; ++i) a.mom[i] = n_mom ? mom[(size_t)(t - 1) * L + i] : nullptr;
    a.u = u ? u + (size_t)(t - 1) * chains : nullptr;
    CHK(sgrad_core(h, x, mask, N, k, chunk, lat, L, coef, gbuf, L, lq, lph, lpx));
    HIPCHK(launch_ais_begin(h->stream, a));
    ++h->count.ais_launch;
    for (int l = 1; l <= nl; ++l) {
      CHK(sgrad_core(h, x, mask, N, k, chunk, a.q, L, coef, gbuf, L, lq, lph, lpx));
      if (l < nl) HIPCHK(launch_ais_step(h->stream, a));
      else HIPCHK(launch_ais_end(h->stream, a));
      ++h->count.ais_launch;
    }
    ++h->count.ais;
  }
  HIPCHK(launch_ais_finish(h->stream, a.log_w, N, k, logpx, ess, &h->ds->rng[0], (unsigned)T));
  return IWAE_OK;
}

int iwae_ais(iwae_handle* h, const float* x, int N, int k, int chunk, float* const* lat, int n_lat,
             const iwae_ais_config* cfg, const float* betas, const float* const* mom, int n_mom, const float* u,
             float* step_io, float* log_w, float* accepts, float* logpx, float* ess) {
  return ais_core(h, x, nullptr, N, k, chunk, lat, n_lat, cfg, betas, mom, n_mom, u, step_io, log_w, accepts, logpx, ess);
}

int iwae_ais_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk, float* const* lat,
                    int n_lat, const iwae_ais_config* cfg, const float* betas, const float* const* mom, int n_mom,
                    const float* u, float* step_io, float* log_w, float* accepts, float* logpx, float* ess) {
  CHK(check_observed(h, x, mask));
  return ais_core(h, x, mask, N, k, chunk, lat, n_lat, cfg, betas, mom, n_mom, u, step_io, log_w, accepts, logpx, ess);
}

// Per-image variational refinement (include/iwae.h): n_iters gradient passes
// at the samples of q* (iwae_score_grad under (0, 1, 1), fused or layer-wise as
// it decides) with one launch of iwae_refine.hip before the first, between each
// pair and after the last, then one scoring pass and the finish launch where
// the caller wants the evaluation.  Everything is enqueued on h->stream; the
// samples' buffers (refine_ws) only grow, so the host waits only where a
// workspace grows.
// (mask: iwae_refine_masked's, handed to every gradient and scoring pass; null: none)
static int refine_core(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk, float* const* mean,
                       float* const* logstd, int n_par, const iwae_refine_config* cfg, const float* const* eps,
                       int n_eps, float* const* adam, int n_adam, float* bound, float* const* lat_out, int n_lat,
                       float* log_w, float* logpx, float* ess) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (!cfg) return fail(h, IWAE_EINVAL, "cfg is NULL");
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (n_par != L || !mean || !logstd)
    return fail(h, IWAE_EINVAL, "expected " + std::to_string(L) + " mean and logstd buffers (one per stochastic layer), got " +
                                   std::to_string(n_par));
  for (int i = 0; i < L; ++i)
    if (!mean[i] || !logstd[i]) return fail(h, IWAE_EINVAL, "NULL mean or logstd buffer");
  if (cfg->objective != 0 && cfg->objective != 1) return fail(h, IWAE_EINVAL, "objective must be 0 (ELBO) or 1 (IWAE_k)");
  const int T = cfg->n_iters;
  if (T < 0 || T > (1 << 24)) return fail(h, IWAE_EINVAL, "n_iters must be in [0, 2^24]");
  if (cfg->step0 < 0 || cfg->step0 > (1 << 30)) return fail(h, IWAE_EINVAL, "step0 must be in [0, 2^30]");
  if (!std::isfinite(cfg->lr) || cfg->lr <= 0.f) return fail(h, IWAE_EINVAL, "lr must be positive and finite");
  if (!std::isfinite(cfg->epsilon) || cfg->epsilon <= 0.f)
    return fail(h, IWAE_EINVAL, "epsilon must be positive and finite");
  if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f))
    return fail(h, IWAE_EINVAL, "beta1 and beta2 must be in [0, 1)");
  if (!std::isfinite(cfg->logstd_min) || !std::isfinite(cfg->logstd_max) || cfg->logstd_min > cfg->logstd_max)
    return fail(h, IWAE_EINVAL, "logstd_min and logstd_max must be finite, logstd_min <= logstd_max");
  if (n_lat != 0 && (n_lat != L || !lat_out))
    return fail(h, IWAE_EINVAL, "expected 0 or " + std::to_string(L) + " sample buffers, got " + std::to_string(n_lat));
  for (int i = 0; i < n_lat; ++i)
    if (!lat_out[i]) return fail(h, IWAE_EINVAL, "NULL sample buffer");
  const bool eval = n_lat > 0 || log_w || logpx || ess;
  if (T == 0 && !eval) return fail(h, IWAE_EINVAL, "n_iters is 0 and no evaluation output is asked for");
  const long long P = (long long)T + (eval ? 1 : 0);
  if (n_eps != 0 && ((long long)n_eps != P * L || !eps))
    return fail(h, IWAE_EINVAL, "expected 0 or (n_iters + evaluation) * " + std::to_string(L) + " noise buffers, got " +
                                   std::to_string(n_eps));
  for (int i = 0; i < n_eps; ++i)
    if (!eps[i]) return fail(h, IWAE_EINVAL, "NULL noise buffer");
  if (n_adam != 0 && (n_adam != 4 * L || !adam))
    return fail(h, IWAE_EINVAL, "expected 0 or " + std::to_string(4 * L) + " Adam buffers, got " + std::to_string(n_adam));
  for (int i = 0; i < n_adam; ++i)
    if (!adam[i]) return fail(h, IWAE_EINVAL, "NULL Adam buffer");
  if (cfg->step0 > 0 && n_adam == 0) return fail(h, IWAE_EINVAL, "step0 > 0 continues a run: it needs the Adam buffers");
  if (!chunk_images(h, N, k, chunk)) return IWAE_EINVAL;
  const long long rows = (long long)N * k;
  if (rows > (1LL << 30)) return fail(h, IWAE_EINVAL, "N * k above 2^30 rows");
  // ---- the samples' buffers: per layer latents, noise, gradients [k][N][d_i]; per row log p(h), log p(x|h), the
  // weights; the moments [N][d_i] where the caller gave none
  WsLayout lay;
  size_t o_h[IWAE_MAX_LAYERS], o_e[IWAE_MAX_LAYERS], o_g[IWAE_MAX_LAYERS], o_m[IWAE_MAX_LAYERS][4];
  int dmax = 0, D = 0;
  for (int i = 0; i < L; ++i) {
    const int d = h->enc[i].d;
    const size_t n = (size_t)rows * d;
    o_h[i] = lay.take(n); o_e[i] = lay.take(n); o_g[i] = lay.take(n);
    for (int j = 0; j < 4; ++j) o_m[i][j] = n_adam ? 0 : lay.take((size_t)N * d);
    dmax = std::max(dmax, d);
    D += d;
  }
  const size_t o_lph = lay.take(rows), o_lpx = lay.take(rows), o_w = lay.take(rows);
  CHK(h->refine_ws.reserve(h, lay.floats));
  float* ws = h->refine_ws.p;
  RefineArgs a{};
  a.L = L; a.N = N; a.k = k; a.D = D;
  a.group = dmax <= 64 ? 16 : 64;
  float *lat[IWAE_MAX_LAYERS], *gbuf[IWAE_MAX_LAYERS];
  for (int i = 0; i < L; ++i) {
    a.d[i] = h->enc[i].d;
    a.vec[i] = (a.d[i] & 3) == 0;
    a.mean[i] = mean[i]; a.logstd[i] = logstd[i];
    a.m1m[i] = n_adam ? adam[4 * i] : ws + o_m[i][0];
    a.m2m[i] = n_adam ? adam[4 * i + 1] : ws + o_m[i][1];
    a.m1s[i] = n_adam ? adam[4 * i + 2] : ws + o_m[i][2];
    a.m2s[i] = n_adam ? adam[4 * i + 3] : ws + o_m[i][3];
    a.lat[i] = lat[i] = ws + o_h[i];
    a.epsw[i] = ws + o_e[i];
    a.g[i] = gbuf[i] = ws + o_g[i];
    a.lat_out[i] = n_lat ? lat_out[i] : nullptr;
  }
  float *lph = ws + o_lph, *lpx = ws + o_lpx;
  a.lph = lph; a.lpx = lpx; a.lw = ws + o_w;
  a.objective = cfg->objective;
  a.omb1 = 1.f - cfg->beta1; a.omb2 = 1.f - cfg->beta2; a.eps_hat = cfg->epsilon;
  a.ls_min = cfg->logstd_min; a.ls_max = cfg->logstd_max;
  a.seed = h->seed; a.rng_base = &h->ds->rng[0];
  a.noise_layer = 2 * IWAE_MAX_LAYERS + 13;
  a.eval = eval ? 1 : 0;
  // logpx / ess are formed from the weights: in the workspace where the caller has no use for them
  a.log_w = log_w ? log_w : (logpx || ess) ? ws + o_w : nullptr;
  a.logpx = logpx; a.ess = ess;
  a.rng_adv = &h->ds->rng[0]; a.n_adv = (unsigned)P;
  const float coef[3] = {0.f, 1.f, 1.f};
  auto pass_noise = [&](long long p) {             // the next draw is pass p's
    a.pass = (unsigned)p;
    for (int i = 0; i < L; ++i) a.eps_in[i] = n_eps ? eps[(size_t)p * L + i] : nullptr;
  };
  pass_noise(0);
  HIPCHK(launch_refine_begin(h->stream, a));
  ++h->count.refine_launch;
  const double b1 = cfg->beta1, b2 = cfg->beta2;
  for (int t = 0; t < T; ++t) {
    CHK(sgrad_core(h, x, mask, N, k, chunk, lat, L, coef, gbuf, L, nullptr, lph, lpx));
    const double n = (double)cfg->step0 + t + 1;
    a.lr_n = (float)((double)cfg->lr * std::sqrt(1.0 - std::pow(b2, n)) / (1.0 - std::pow(b1, n)));
    a.zero = cfg->step0 == 0 && t == 0;
    a.bound = bound ? bound + (size_t)t * N : nullptr;
    a.draw = t + 1 < T || eval;
    if (a.draw) pass_noise(t + 1);
    if (t + 1 < T) HIPCHK(launch_refine_step(h->stream, a));
    else HIPCHK(launch_refine_end(h->stream, a));
    ++h->count.refine_launch;
    ++h->count.refine;
  }
  if (eval) CHK(sgrad_core(h, x, mask, N, k, chunk, lat, L, coef, nullptr, 0, nullptr, lph, lpx));
  HIPCHK(launch_refine_finish(h->stream, a));
  return IWAE_OK;
}

int iwae_refine(iwae_handle* h, const float* x, int N, int k, int chunk, float* const* mean, float* const* logstd,
                int n_par, const iwae_refine_config* cfg, const float* const* eps, int n_eps, float* const* adam,
                int n_adam, float* bound, float* const* lat_out, int n_lat, float* log_w, float* logpx, float* ess) {
  return refine_core(h, x, nullptr, N, k, chunk, mean, logstd, n_par, cfg, eps, n_eps, adam, n_adam, bound, lat_out,
                     n_lat, log_w, logpx, ess);
}

int iwae_refine_masked(iwae_handle* h, const float* x, const float* mask, int N, int k, int chunk, float* const* mean,
                       float* const* logstd, int n_par, const iwae_refine_config* cfg, const float* const* eps,
                       int n_eps, float* const* adam, int n_adam, float* bound, float* const* lat_out, int n_lat,
                       float* log_w, float* logpx, float* ess) {
  CHK(check_observed(h, x, mask));
  return refine_core(h, x, mask, N, k, chunk, mean, logstd, n_par, cfg, eps, n_eps, adam, n_adam, bound, lat_out,
                     n_lat, log_w, logpx, ess);
}

// Encoder.call (F:56-F:75): k samples of q(h|x) per image on the layer-wise
// kernels (the rows have to reach memory), relayouted into the reference's
// sample-major buffers.
int iwae_encode(iwae_handle* h, const float* x, int N, int k, int chunk, const float* const* eps, int n_eps,
                float* const* lat_out, int n_lat, float* log_q, float* loc_top, float* scale_top) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  const int L = h->L;
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  CHK(ptrs_ok(h, eps, n_eps, "eps", true));
  CHK(ptrs_ok(h, lat_out, n_lat, "latent", true));
  if (n_lat == 0 && !log_q && !loc_top && !scale_top) return fail(h, IWAE_EINVAL, "every output is NULL");
  const int imgs = chunk_images(h, N, k, chunk);
  if (!imgs) return IWAE_EINVAL;
  const bool injected = n_eps > 0;
  const int rows = imgs * k;
  CHK(ensure_capacity(h, imgs, rows, false));
  if (h->x3) CHK(ensure_wsplit(h));
  // a chunk's [k][n][d] noise, contiguous, in iwae_posterior's workspace
  const bool gather = injected && imgs < N;
  WsLayout lay;
  size_t o_eps[IWAE_MAX_LAYERS] = {};
  for (int i = 0; i < L; ++i) o_eps[i] = lay.take(gather ? (size_t)rows * h->enc[i].d : 0);
  CHK(h->post_ws.reserve(h, lay.floats));
  for (ChunkWalk W(h, N, k, imgs, false, x, nullptr, false); W.i0 < N; W.i0 += imgs) {
    CHK(walk_step(h, W));
    const int i0 = W.i0, n = W.n;
    Plan P;
    P.B = n; P.Bimg = n; P.Bsplit = n; P.kS = k;
    EpsSet E;
    CHK(chunk_eps(h, W, injected ? eps : nullptr, gather, h->post_ws.p, o_eps, E));
    CHK(encoder_fwd(h, P, E, false));
    ScRelayout G{};
    G.n = n; G.k = k; G.N = N; G.i0 = i0; G.gather = 0;
    for (int i = 0; n_lat > 0 && i < L; ++i)
      G.seg[G.nseg++] = ScSeg{h->h[i].p, h->h[i].ld, 0, h->enc[i].d, lat_out[i], 0, 0};
    const Mat& PT = h->eb[L - 1].P;              // (mu | zs) of distributions[-1] (F:75): image rows when L = 1
    const int dT = h->enc[L - 1].d;
    if (loc_top) G.seg[G.nseg++] = ScSeg{PT.p, PT.ld, 0, dT, loc_top, 0, L == 1};
    if (scale_top) G.seg[G.nseg++] = ScSeg{PT.p, PT.ld, dT, dT, scale_top, 1, L == 1};
    HIPCHK(launch_score_relayout(h->stream, G));
    if (log_q)
      HIPCHK(hipMemcpyAsync(log_q + (size_t)i0 * k, h->logq, (size_t)n * k * sizeof(float), hipMemcpyDeviceToDevice,
                            h->stream));
    if (!injected) HIPCHK(launch_rng_advance(h->stream, &h->ds->rng[0]));
  }
  return IWAE_OK;
}

// The aggregate posterior q(h_1) = 1/M sum_m q(h_1 | x_m) at R query latents
// (DESIGN.md 3.4.12).  The reference components are the first encoder layer's
// (mu, s) of x_ref -- walk_step's layer-0 launches on image rows, k = 1, no
// sampling, no later layer -- or the caller's; one prep launch forms 1 / s and
// the log term, then the joint and per-unit kernels run over the query rows.
int iwae_aggregate(iwae_handle* h, const float* x_ref, int M, int chunk, float* loc, float* scale, const float* lat1,
                   long long R, int own_period, float* log_q_agg, float* log_q_dim, float* log_q_own,
                   float* log_q_own_dim) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!log_q_agg && !log_q_dim && !log_q_own && !log_q_own_dim) return fail(h, IWAE_EINVAL, "every output is NULL");
  if (!lat1) return fail(h, IWAE_EINVAL, "lat1 is NULL");
  if (R < 1 || R > (1LL << 30)) return fail(h, IWAE_EINVAL, "R must be in [1, 2^30]");
  if (M < 1 || M > (1 << 24)) return fail(h, IWAE_EINVAL, "M must be in [1, 2^24]");
  if (!x_ref && (!loc || !scale)) return fail(h, IWAE_EINVAL, "without x_ref both loc and scale are required");
  if (own_period < 0 || own_period > M) return fail(h, IWAE_EINVAL, "own_period must be in [0, M]");
  if (own_period == 0 && (log_q_own || log_q_own_dim))
    return fail(h, IWAE_EINVAL, "log_q_own / log_q_own_dim need own_period > 0");
  const int d = h->enc[0].d;
  int imgs = 0;
  if (x_ref) {
    imgs = chunk_images(h, M, 1, chunk);
    if (!imgs) return IWAE_EINVAL;
  }
  // the split of the references, from (R, M, d) alone
  AggArgs J{}, D{};
  J.M = D.M = M; J.d = D.d = d;
  J.log_m = D.log_m = logf((float)M);
  J.lat = D.lat = lat1; J.R = D.R = R;
  agg_split(agg_joint_wgs(R), M, kAggJointRefs, J.seg_len, J.nseg);
  D.uw = agg_dim_units(d); D.tm = agg_dim_refs(d);
  agg_split(agg_dim_wgs(R, d), M, D.tm, D.seg_len, D.nseg);
  const size_t md = (size_t)M * d;
  WsLayout lay;
  const size_t o_rs = lay.take(md), o_lc = lay.take(md);
  const size_t o_mu = lay.take(x_ref && !loc ? md : 0), o_sc = lay.take(x_ref && !scale ? md : 0);
  // split partials: a split call has fewer than kAggWgs workgroups of at most 64 rows / 1024 (row, unit)
  // pairs, so these stay below 2^18 and 2^22 floats (agg_split)
  const size_t o_pj = lay.take(log_q_agg && J.nseg > 1 ? (size_t)R * J.nseg * 2 : 0);
  const size_t o_pd = lay.take(log_q_dim && D.nseg > 1 ? (size_t)R * d * D.nseg * 2 : 0);
  if (x_ref) {
    CHK(ensure_capacity(h, imgs, imgs, false));
    if (h->x3) CHK(ensure_wsplit(h));
  }
  CHK(h->agg_ws.reserve(h, lay.floats));
  float* ws = h->agg_ws.p;
  float* mu = loc ? loc : ws + o_mu;
  float* sc = scale ? scale : ws + o_sc;
  if (x_ref) {
    for (ChunkWalk W(h, M, 1, imgs, false, x_ref, nullptr, true); W.i0 < M; W.i0 += imgs) {
      CHK(walk_step(h, W));
      const Mat& P0 = h->eb[0].P;
      ScRelayout G{};
      G.n = W.n; G.k = 1; G.N = M; G.i0 = W.i0; G.gather = 0;
      G.seg[G.nseg++] = ScSeg{P0.p, P0.ld, 0, d, mu, 0, 1};
      G.seg[G.nseg++] = ScSeg{P0.p, P0.ld, d, d, sc, 1, 1};
      HIPCHK(launch_score_relayout(h->stream, G));
    }
  }
  HIPCHK(launch_agg_prep(h->stream, sc, (long long)md, ws + o_rs, ws + o_lc));
  J.mu = D.mu = mu; J.rs = D.rs = ws + o_rs; J.lc = D.lc = ws + o_lc;
  J.vec = D.vec = (d % 4 == 0 && (((uintptr_t)lat1 | (uintptr_t)mu) & 15) == 0) ? 1 : 0;
  if (log_q_agg) {
    J.part = ws + o_pj; J.out = log_q_agg;
    HIPCHK(launch_agg_joint(h->stream, J));
    ++h->count.agg_joint;
    if (J.nseg > 1) HIPCHK(launch_agg_merge(h->stream, J.part, R, J.nseg, J.log_m, J.out));
  }
  if (log_q_dim) {
    D.part = ws + o_pd; D.out = log_q_dim;
    HIPCHK(launch_agg_dim(h->stream, D));
    ++h->count.agg_dim;
    if (D.nseg > 1) HIPCHK(launch_agg_merge(h->stream, D.part, R * d, D.nseg, D.log_m, D.out));
  }
  if (log_q_own || log_q_own_dim) HIPCHK(launch_agg_own(h->stream, J, own_period, log_q_own, log_q_own_dim));
  ++h->count.agg;
  return IWAE_OK;
}

// get_NLL_without_inactive_units (F:466-F:494): k-sample log p(x) with every
// sampled h_i multiplied by its 0/1 active-unit mask masks[i] ([dev], d_i).
int iwae_nll_masked(iwae_handle* h, const float* x, int N, int k, const float* const* eps, int n_eps,
                    const float* const* masks, int n_masks, float* out_logpx) {
  if (!h) return IWAE_EINVAL;
  if (!out_logpx) return fail(h, IWAE_EINVAL, "out_logpx is NULL");
  if (!masks || n_masks != h->L) return fail(h, IWAE_EINVAL, "expected one mask per stochastic layer");
  for (int i = 0; i < h->L; ++i)
    if (!masks[i]) return fail(h, IWAE_EINVAL, "NULL mask");
  h->masked = true;
  for (int i = 0; i < h->L; ++i) h->mask[i] = masks[i];
  const int rc = (eps && n_eps > 0) ? iwae_nll_eps(h, x, N, k, eps, n_eps, out_logpx)
                                    : nll_core(h, x, N, k, 0, nullptr, nullptr, out_logpx);
  h->masked = false;
  for (int i = 0; i < h->L; ++i) h->mask[i] = nullptr;
  return rc;
}

// ------------------------------------------------ reweighted wake-sleep step
// iwae_wake_sleep_step / _grad.  The decoder takes the IWAE
// gradient of the wake forward; every encoder layer is a weighted regression of
// log q(h_i | input) at fixed latents (GM_FIT) over two row sets laid out one
// behind the other in the train step's own activation buffers: the wake rows
// (B image rows / B k sample rows, weight c_wake softmax / B) and the n dream
// rows behind them (weight c_sleep / n), so one weight-gradient job per Dense
// sums both in a fixed order.  A phase whose coefficient is 0 is outside every
// row range: none of its rows is read.
static Mat rows_from(const Mat& m, long long r) {
  Mat o = m;
  if (o.p) o.p += r * o.ld;
  return o;
}
static LayerBufs rows_from(const LayerBufs& b, long long r) {
  LayerBufs o;
  o.y1 = rows_from(b.y1, r); o.y2 = rows_from(b.y2, r); o.P = rows_from(b.P, r);
  o.dP = rows_from(b.dP, r); o.dY2 = rows_from(b.dY2, r); o.dY1 = rows_from(b.dY1, r);
  return o;
}

// Moves workspace pointers r rows down for its lifetime, so a routine written
// for rows [0, n) of the handle's buffers runs on rows [r, r + n) instead.
struct RowShift {
  std::vector<std::pair<float**, long long>> moved;
  void mat(Mat& m, long long r) {
    if (!m.p) return;
    m.p += r * m.ld;
    moved.push_back({&m.p, r * m.ld});
  }
  void vec(float*& p, long long r) {
    p += r;
    moved.push_back({&p, r});
  }
  ~RowShift() {
    for (auto& q : moved) *q.first -= q.second;
  }
};

static bool ws_use_fused(const iwae_handle* h, long long rows) {
  if (h->path == 1 || h->L > kRbMaxJobs || h->masked || !rb_width_ok(h)) return false;
  return h->path == 2 || rows <= 65536;
}

// the encoder forward at the n dream rows' given latents: y1, y2 and P kept
// for the weight gradient, log q(h^j | x^j) into logq[M + j]
static int ws_sleep_forward(iwae_handle* h, const Plan& P, int n, bool fusedp) {
  const int L = h->L, B = P.Bimg, M = P.Bimg * P.kS;
  Plan P2 = P;
  P2.B = P2.Bimg = P2.Bsplit = n; P2.kS = 1;
  if (fusedp) {
    // the first encoder layer's own launches (few-row or split-K GEMM + row-block job) on the image rows behind B
    RowShift sh;
    sh.mat(h->x_in, B); sh.mat(h->eb[0].y1, B); sh.mat(h->eb[0].y2, B); sh.mat(h->eb[0].P, B);
    h->step.x_user = nullptr;
    CHK(enc0_forward(h, P2));
  } else {
    LayerBufs b0 = rows_from(h->eb[0], B);
    CHK(stoch_fwd(h, h->enc[0], rows_from(h->x_in, B), n, b0));
  }
  for (int i = 0; i < L; ++i) {
    const StochL& S = h->enc[i];
    LayerBufs b = rows_from(h->eb[i], i == 0 ? B : M);
    Mat tgt = rows_from(h->h[i], M);
    if (i > 0 && fusedp) {
      Mat in = rows_from(h->h[i - 1], M);
      RbFwdLaunch Lf{};
      Lf.ld_lds = rb_ld(h, false);
      RbFwdJob& J = Lf.job[0];
      J.rows = n; J.rpb = 16;
      J.in = in.p; J.ld_in = in.ld;
      J.nst = 3;
      J.st[0] = rb_fwd_stage(h, S.l1, 1, &b.y1);
      J.st[1] = rb_fwd_stage(h, S.l2, 1, &b.y2);
      J.st[2] = rb_fwd_stage(h, S.head, 0, &b.P);
      // the target-given density epilogue (the decoder prior's), accumulated into the dream rows' log q
      J.epi = 2; J.ep_d = S.d; J.ep_tgt = tgt.p; J.ep_ldtgt = tgt.ld;
      J.logp = h->logq + M; J.logp_acc = 1;
      Lf.njobs = 1;
      CHK(run_rb_fwd(h, Lf));
      continue;
    }
    if (i > 0) CHK(stoch_fwd(h, S, rows_from(h->h[i - 1], M), n, b));
    CHK(gauss_logdens(h, b.P, 1, S.d, tgt, h->logq + M, i > 0, n));
  }
  return IWAE_OK;
}

// GM_FIT backward of every encoder layer over image rows [i0, B + n) / sample
// rows [r0, M + n) and the layers' weight gradients; w: the row weights
static int ws_encoder_fit(iwae_handle* h, const Plan& P, int n, bool wake, const float* w, bool fusedp) {
  const int L = h->L, B = P.Bimg, M = P.Bimg * P.kS;
  const int i0 = wake ? 0 : B, r0 = wake ? 0 : M;
  // images that own kS rows of h_1 each (the wake images), then one row each
  // (the dream images); with kS == 1, or without the wake rows, image rows and
  // sample rows run side by side
  const bool per_image = wake && P.kS > 1;
  std::vector<Mat> keep;
  keep.reserve(6 * (size_t)L);
  std::vector<WJob> js;
  for (int i = L - 1; i >= 0; --i) {
    const StochL& S = h->enc[i];
    const int off = i == 0 ? i0 : r0, rows = (i == 0 ? B : M) + n - off;
    LayerBufs b = rows_from(h->eb[i], off);
    const Mat Hm = rows_from(h->h[i], r0);
    const Mat in = i == 0 ? rows_from(h->x_in, i0) : rows_from(h->h[i - 1], r0);
    const int kS = i == 0 && per_image ? P.kS : 1;
    const int nk = i == 0 && per_image && n > 0 ? B : 0;
    if (fusedp) {
      RbBwdLaunch Lb{};
      Lb.ld_lds = rb_ld(h, true);
      RbBwdJob& J = Lb.job[0];
      J.pro = i == 0 ? 3 : 1;
      J.rows = rows; J.rpb = i == 0 ? 1 : 16;
      J.kS = kS; J.nk_img = nk;
      J.P = b.P.p; J.ldP = b.P.ld; J.d = S.d;
      J.H = Hm.p; J.ldH = Hm.ld;
      J.dlw = w + r0;
      J.gmode = GM_FIT;
      J.dP_out = b.dP.p; J.ld_dP = b.dP.ld;
      // two stages, dY2 and dY1: no dX below (the layer's input is data)
      const bool sm0 = i == 0 && smallm_ok(h, rows);
      J.nst = sm0 ? 0 : 2;
      if (!sm0) {
        J.st[0] = rb_bwd_stage(h, S.head, &b.y2, &b.dY2);
        J.st[1] = rb_bwd_stage(h, S.l2, &b.y1, &b.dY1);
      }
      Lb.njobs = 1;
      HIPCHK(launch_rb_bwd(h->stream, Lb));
      h->count.ws_rb++;
      if (sm0) {
        CHK(smallm(h, b.dP, rows, h->dense[S.head], true, 2, &b.y2, b.dY2));
        CHK(smallm(h, b.dY2, rows, h->dense[S.l2], true, 2, &b.y1, b.dY1));
      }
      const size_t q = keep.size();
      for (const Mat& m : {in, b.dY1, b.y1, b.dY2, b.y2, b.dP}) keep.push_back(m);
      const WGroup grp = i == 0 ? WG_ENC0 : WG_ENC;
      js.push_back({S.l1, &keep[q], &keep[q + 1], rows, nullptr, grp});
      js.push_back({S.l2, &keep[q + 2], &keep[q + 3], rows, nullptr, grp});
      js.push_back({S.head, &keep[q + 4], &keep[q + 5], rows, nullptr, grp});
    } else {
      GaussBwdArgs g{};
      g.P = b.P.p; g.ldP = b.P.ld; g.prow_div = kS; g.d = S.d;
      g.H = Hm.p; g.ldH = Hm.ld;
      g.dlw = w + r0;
      g.grad_mode = GM_FIT; g.nk_img = nk;
      g.dP = b.dP.p; g.lddP = b.dP.ld;
      g.M = M + n - r0;
      HIPCHK(launch_gauss_bwd(h->stream, 0, g));
      h->count.ws_gauss++;
      CHK(stoch_bwd(h, S, in, rows, b, true, nullptr));      // (no dx: the third dX GEMM is not issued)
    }
  }
  // row-block path: the encoder's weight gradients in grouped launches
  return weight_grad_jobs(h, js);
}

static int do_wake_sleep(iwae_handle* h, const iwae_ws_config* cfg, const float* x, int B, const float* const* eps,
                         int n_eps, const float* dream_x, const float* const* dream_lat, int n_dream_lat,
                         float* values_dev, bool adam) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!cfg) return fail(h, IWAE_EINVAL, "wake-sleep config is NULL");
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (cfg->k < 1) return fail(h, IWAE_EINVAL, "k must be positive");
  if (B < 1) return fail(h, IWAE_EINVAL, "batch must be positive");
  const float cw = cfg->c_wake, cs = cfg->c_sleep;
  if (!std::isfinite(cw) || !std::isfinite(cs) || cw < 0.f || cs < 0.f)
    return fail(h, IWAE_EINVAL, "c_wake and c_sleep must be finite and not negative");
  if (cw == 0.f && cs == 0.f) return fail(h, IWAE_EINVAL, "c_wake and c_sleep are both 0");
  const int n = cfg->n_dream;
  if (cs > 0.f && n < 1) return fail(h, IWAE_EINVAL, "c_sleep > 0 needs n_dream >= 1");
  if (cs == 0.f && n != 0) return fail(h, IWAE_EINVAL, "c_sleep == 0 needs n_dream == 0");
  if ((dream_x != nullptr) != (dream_lat != nullptr))
    return fail(h, IWAE_EINVAL, "dream_x and dream_lat go together (both, or neither for the step's own dreams)");
  const int L = h->L;
  if (n_dream_lat != (dream_lat ? L : 0))
    return fail(h, IWAE_EINVAL, "n_dream_lat must be " + std::to_string(L) + " with dream_lat and 0 without");
  for (int i = 0; dream_lat && i < L; ++i)
    if (!dream_lat[i]) return fail(h, IWAE_EINVAL, "NULL dream_lat buffer");
  if ((long long)B * cfg->k + n > (1LL << 30)) return fail(h, IWAE_EINVAL, "B * k + n_dream exceeds 2^30 rows");
  if (h->dp_world > 1)
    return fail(h, IWAE_EINVAL, "wake-sleep steps are not built for data parallelism (world > 1)");
  iwae_loss_config lc{IWAE_LOSS_IWAE, cfg->k, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, B, P));
  EpsSet E;
  CHK(parse_eps(h, P, eps, n_eps, E));
  const int M = B * P.kS;
  const bool wake = cw > 0.f, sleep = cs > 0.f, own = sleep && !dream_x;
  const bool fusedp = ws_use_fused(h, (long long)M + n);
  // every workspace at its size before anything is enqueued
  CHK(ensure_capacity(h, B + n, M + n, true));
  const int ldp = r4(h->xdim);
  if (own) {
    size_t need = (size_t)n * ldp;
    for (int i = 0; i < L; ++i) need += ((size_t)n * h->enc[i].d + 3) & ~size_t(3);
    CHK(h->ws_ws.reserve(h, need));
  }
  const bool direct = fusedp && smallm_ok(h, P.Bimg);
  if (!direct) CHK(copy_x(h, P, x));
  StepScope scope{h};
  h->step.x_user = direct ? x : nullptr;
  h->step.in_train_step = true;
  h->step.out_x3 = h->x3 && h->tune.out_x3_rows > 0 && (long long)M >= h->tune.out_x3_rows;
  if (h->step.out_x3) CHK(run_wsplit_seg(h, h->o3));
  float* vals = values_dev ? values_dev : &h->ds->scalars[4];
  h->count.ws++;
  // wake forward, the IWAE loss and its row weights, the decoder's gradient
  if (fusedp) CHK(fused_forward(h, P, E, true));
  else CHK(layerwise_forward(h, P, E, true));
  CHK(run_bound(h, P, true, -1.f, vals, adam));
  if (fusedp) {
    CHK(fused_decoder_bwd(h, P, h->dlw, h->dpx, false));
    CHK(weight_grads(h, P, WG_DECODER));
  } else {
    CHK(decoder_bwd(h, P, h->dlw, h->dpx, true, false));
  }
  if (sleep) {
    const float* dx = dream_x;
    int ld_dx = h->xdim;
    const float* dl[IWAE_MAX_LAYERS] = {};
    for (int i = 0; dream_lat && i < L; ++i) dl[i] = dream_lat[i];
    if (own) {
      // one iwae_generate call as a caller would make it (outside the train
      // step's precision rules), its layer-wise launches on the rows behind the
      // wake rows: the wake latents are the encoder fit's data
      float* hl[IWAE_MAX_LAYERS] = {};
      float* p = h->ws_ws.p + (size_t)n * ldp;
      for (int i = 0; i < L; ++i) {
        hl[i] = p;
        p += ((size_t)n * h->enc[i].d + 3) & ~size_t(3);
      }
      h->step = StepState();
      {
        RowShift sh;
        for (Mat& m : h->h) sh.mat(m, M);
        for (LayerBufs& b : h->db) { sh.mat(b.y1, M); sh.mat(b.y2, M); sh.mat(b.P, M); }
        sh.mat(h->ob.y1, M); sh.mat(h->ob.y2, M);
        sh.vec(h->logp, M);
        CHK(iwae_generate(h, n, nullptr, nullptr, 0, nullptr, nullptr, 0, h->ws_ws.p, ldp, hl, L));
      }
      h->count.ws_dream++;
      h->step.in_train_step = true;
      dx = h->ws_ws.p; ld_dx = ldp;
      for (int i = 0; i < L; ++i) dl[i] = hl[i];
    }
    WsStageArgs sa{};
    sa.n = n; sa.nbuf = L + 1;
    sa.src[0] = dx; sa.ld_src[0] = ld_dx; sa.width[0] = h->xdim;
    sa.dst[0] = h->x_in.p + (size_t)B * h->x_in.ld; sa.ld_dst[0] = h->x_in.ld;
    for (int i = 0; i < L; ++i) {
      sa.src[i + 1] = dl[i]; sa.ld_src[i + 1] = sa.width[i + 1] = h->enc[i].d;
      sa.dst[i + 1] = h->h[i].p + (size_t)M * h->h[i].ld; sa.ld_dst[i + 1] = h->h[i].ld;
    }
    HIPCHK(launch_ws_stage(h->stream, sa));
    CHK(ws_sleep_forward(h, P, n, fusedp));
  }
  // row weights (dlw2's rows: no second weighting in this plan), the two encoder values, the fit
  HIPCHK(launch_ws_weights(h->stream, h->dlw, h->dlw2, M, n, cw, sleep ? cs / (float)n : 0.f));
  HIPCHK(launch_ws_values(h->stream, h->dlw, h->logq, M, n, wake ? 1 : 0, vals + 1));
  CHK(ws_encoder_fit(h, P, n, wake, h->dlw2, fusedp));
  return finish_step(h, P, adam);
}

int iwae_wake_sleep_step(iwae_handle* h, const iwae_ws_config* cfg, const float* x, int B, const float* const* eps,
                         int n_eps, const float* dream_x, const float* const* dream_lat, int n_dream_lat,
                         float* values_dev) {
  return do_wake_sleep(h, cfg, x, B, eps, n_eps, dream_x, dream_lat, n_dream_lat, values_dev, true);
}

int iwae_wake_sleep_grad(iwae_handle* h, const iwae_ws_config* cfg, const float* x, int B, const float* const* eps,
                         int n_eps, const float* dream_x, const float* const* dream_lat, int n_dream_lat,
                         float* values_dev) {
  return do_wake_sleep(h, cfg, x, B, eps, n_eps, dream_x, dream_lat, n_dream_lat, values_dev, false);
}

// ------------------------------------------ thermodynamic variational objective
// iwae_tvo_step / _grad / _weights.  A sibling of the
// wake-wake step above: the same wake forward, decoder backward without dL/dh
// and GM_FIT encoder regression over the wake rows, with tvo_kernel in place of
// the bound launch and of the ws_weights / ws_values launches: it writes the
// decoder's row weight -a_theta / B where an IWAE step has dL/dlw and dpx, and
// the regression's row weight a_phi / B (of either sign: the GM_FIT partials
// are linear in it) into dlw2's rows.
static int tvo_partition(iwae_handle* h, const float* betas, int n_part, TvoArgs& t) {
  if (!betas) return fail(h, IWAE_EINVAL, "betas is NULL");
  if (n_part < 1 || n_part > kTvoMaxPart)
    return fail(h, IWAE_EINVAL, "n_part must be in [1, " + std::to_string(kTvoMaxPart) + "]");
  for (int j = 0; j <= n_part; ++j) {
    if (!std::isfinite(betas[j])) return fail(h, IWAE_EINVAL, "betas must be finite");
    if (j > 0 && !(betas[j] > betas[j - 1])) return fail(h, IWAE_EINVAL, "betas must be strictly ascending");
    t.beta[j] = betas[j];
  }
  if (betas[0] != 0.f || betas[n_part] != 1.f) return fail(h, IWAE_EINVAL, "betas must run from 0 to 1");
  t.J = n_part;
  return IWAE_OK;
}

static int do_tvo(iwae_handle* h, const iwae_tvo_config* cfg, const float* betas, const float* x, int B,
                  const float* const* eps, int n_eps, float* values_dev, bool adam) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!cfg) return fail(h, IWAE_EINVAL, "TVO config is NULL");
  if (!x) return fail(h, IWAE_EINVAL, "x is NULL");
  if (cfg->k < 1) return fail(h, IWAE_EINVAL, "k must be positive");
  if (B < 1) return fail(h, IWAE_EINVAL, "batch must be positive");
  TvoArgs t{};
  CHK(tvo_partition(h, betas, cfg->n_part, t));
  if ((long long)B * cfg->k > (1LL << 30)) return fail(h, IWAE_EINVAL, "B * k exceeds 2^30 rows");
  if (h->dp_world > 1) return fail(h, IWAE_EINVAL, "TVO steps are not built for data parallelism (world > 1)");
  iwae_loss_config lc{IWAE_LOSS_IWAE, cfg->k, 1.f, 1.f, 0.5f, 0, 0};
  Plan P;
  CHK(make_plan(h, &lc, B, P));
  EpsSet E;
  CHK(parse_eps(h, P, eps, n_eps, E));
  const int M = B * P.kS;
  const bool fusedp = ws_use_fused(h, M);
  // the workspace at its size before anything is enqueued
  CHK(ensure_capacity(h, B, M, true));
  const bool direct = fusedp && smallm_ok(h, P.Bimg);
  if (!direct) CHK(copy_x(h, P, x));
  StepScope scope{h};
  h->step.x_user = direct ? x : nullptr;
  h->step.in_train_step = true;
  h->step.out_x3 = h->x3 && h->tune.out_x3_rows > 0 && (long long)M >= h->tune.out_x3_rows;
  if (h->step.out_x3) CHK(run_wsplit_seg(h, h->o3));
  h->count.tvo++;
  if (fusedp) CHK(fused_forward(h, P, E, true));
  else CHK(layerwise_forward(h, P, E, true));
  // the three values, both sets of row weights, the noise position and Adam's tick
  t.part = h->part; t.ldpart = h->ldpart; t.npart = h->npart;
  t.logp = h->logp; t.logq = h->logq; t.lw_out = h->lw;
  t.kS = P.kS; t.Bimg = B;
  t.a_theta = h->dlw; t.a_theta2 = h->dpx; t.s_theta = -1.f / (float)B;
  t.a_phi = h->dlw2; t.s_phi = 1.f / (float)B;
  // (per-image scratch of the train step's arena that no launch of this step reads)
  t.lower = h->contrib; t.upper = h->run_m; t.iwae = h->run_s;
  t.values = values_dev ? values_dev : &h->ds->scalars[4];
  t.ticket = &h->ds->tickets[0]; t.rng_base = &h->ds->rng[0];
  t.adam_step = adam ? &h->ds->adam.t : nullptr;
  HIPCHK(launch_tvo(h->stream, t));
  h->count.tvo_launch++;
  if (fusedp) {
    CHK(fused_decoder_bwd(h, P, h->dlw, h->dpx, false));
    CHK(weight_grads(h, P, WG_DECODER));
  } else {
    CHK(decoder_bwd(h, P, h->dlw, h->dpx, true, false));
  }
  CHK(ws_encoder_fit(h, P, 0, true, h->dlw2, fusedp));
  return finish_step(h, P, adam);
}

int iwae_tvo_step(iwae_handle* h, const iwae_tvo_config* cfg, const float* betas, const float* x, int B,
                  const float* const* eps, int n_eps, float* values_dev) {
  return do_tvo(h, cfg, betas, x, B, eps, n_eps, values_dev, true);
}

int iwae_tvo_grad(iwae_handle* h, const iwae_tvo_config* cfg, const float* betas, const float* x, int B,
                  const float* const* eps, int n_eps, float* values_dev) {
  return do_tvo(h, cfg, betas, x, B, eps, n_eps, values_dev, false);
}

int iwae_tvo_weights(iwae_handle* h, const float* lw, int N, int k, const float* betas, int n_part, float* lower,
                     float* upper, float* iwae, float* a_theta, float* a_phi) {
  if (!h) return IWAE_EINVAL;
  CHK(kernel_status(h));
  if (!lw) return fail(h, IWAE_EINVAL, "lw is NULL");
  if (N < 1) return fail(h, IWAE_EINVAL, "N must be positive");
  if (k < 1 || k > (1 << 20)) return fail(h, IWAE_EINVAL, "k must be in [1, 2^20]");
  TvoArgs t{};
  CHK(tvo_partition(h, betas, n_part, t));
  if ((long long)N * k > (1LL << 30)) return fail(h, IWAE_EINVAL, "N * k exceeds 2^30 log weights");
  if (!lower && !upper && !iwae && !a_theta && !a_phi) return fail(h, IWAE_EINVAL, "every output is NULL");
  t.lw_in = lw; t.kS = k; t.Bimg = N;
  t.a_theta = a_theta; t.s_theta = 1.f;
  t.a_phi = a_phi; t.s_phi = 1.f;
  t.lower = lower; t.upper = upper; t.iwae = iwae;
  HIPCHK(launch_tvo(h->stream, t));
  h->count.tvo_launch++;
  return IWAE_OK;
}

int iwae_debug_gemm(iwae_handle* h, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                    int M, int N, int K) {
  if (!h) return IWAE_EINVAL;
  if ((lda | ldb | ldc) & 3) return fail(h, IWAE_EINVAL, "leading dims must be multiples of 4");
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) return fail(h, IWAE_EINVAL, "pointers must be 16B aligned");
  GemmArgs a{};
  a.x3 = h->x3;
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.kchunk = K;
  HIPCHK(launch_gemm(h->stream, GEMM_FWD, EPI_STORE, choose_tile(M, N, 1), 1, false, a));
  return IWAE_OK;
}

double iwae_workspace_bytes(const iwae_handle* h) { return h ? (double)h->arena_bytes : 0.0; }

long long iwae_debug_count(const iwae_handle* h, int what) {
  if (!h) return -1;
  switch (what) {
    case 0: return h->count.mega;
    case 1: return h->count.mega_eps;
    case 2: return h->count.tc;
    case 3: return h->count.nring;
    case 4: return h->count.nring_train;
    case 5: return h->count.nrb;
    case 6: return h->count.nre;
    case 7: return h->count.captures;
    case 8: {                           // tcu_kernel spin give-ups so far (synchronous read)
      unsigned v[4] = {};
      if (hipStreamSynchronize(h->stream) != hipSuccess ||
          hipMemcpy(v, h->tcu_ctr, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
      return v[2];
    }
    case 9: return h->count.tcu;
    case 10: return h->count.gen;
    case 11: return h->count.path_rb;
    case 12: return h->count.path_gauss;
    case 13: return h->count.rb_fwd;
    case 14: return h->count.upd;
    case 15: return h->count.bound;
    case 16: return h->count.bound_multi;
    case 17: return h->count.post;
    case 18: return h->count.post_lw;
    case 19: return h->count.imp;
    case 20: return h->count.imp_lw;
    case 21: return h->count.bern_mask;
    case 22: return h->count.binarize;
    case 23: return h->count.score;
    case 24: return h->count.score_lw;
    case 25: return h->count.sgrad;
    case 26: return h->count.sgrad_lw;
    case 27: return h->count.ais;
    case 28: return h->count.ais_launch;
    case 29: return h->count.refine;
    case 30: return h->count.refine_launch;
    case 31: return h->count.score_pix;
    case 32: return h->count.score_pix_lw;
    case 33: return h->count.sgrad_pix;
    case 34: return h->count.sgrad_pix_lw;
    case 35: return h->count.ws;
    case 36: return h->count.ws_rb;
    case 37: return h->count.ws_gauss;
    case 38: return h->count.ws_dream;
    case 39: return h->count.agg;
    case 40: return h->count.agg_joint;
    case 41: return h->count.agg_dim;
    case 42: return h->count.tvo;
    case 43: return h->count.tvo_launch;
    default: return -1;
  }
}

int iwae_profile_gemm(iwae_handle* h, int kind, int epi) {
  if (!h) return IWAE_EINVAL;
  HIPCHK(hipStreamSynchronize(h->stream));
  h->prof.kind = kind;
  h->prof.epi = epi;
  h->prof.used = 0;
  h->prof.flop = 0.0;
  h->prof.have = false;
  h->prof.is_tc = false;
  h->prof.mem = nullptr;
  return IWAE_OK;
}

int iwae_profile_replay(iwae_handle* h, int n, double* total_ms, double* total_flop) {
  if (!h || !total_ms || !total_flop || n <= 0) return IWAE_EINVAL;
  if (!h->prof.have) return fail(h, IWAE_EINVAL, "no launch of the profiled GEMM class was recorded");
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventRecord(e0, h->stream));
  for (int i = 0; i < n; ++i) {
    if (h->prof.is_tc) HIPCHK(launch_tc(h->stream, h->prof.tc, h->prof.tc_rt, h->prof.tc_lds));
    else if (h->prof.kind >= 12) HIPCHK(h->prof.mem(h->stream));     // (12-16: recorded closures)
    else HIPCHK(launch_gemm(h->stream, h->prof.k, h->prof.e, h->prof.tile, h->prof.splits, h->prof.ks, h->prof.args));
  }
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *total_ms = ms;
  *total_flop = h->prof.flop1 * n;
  return IWAE_OK;
}

int iwae_profile_read(iwae_handle* h, double* total_ms, double* total_flop, long long* launches) {
  if (!h || !total_ms || !total_flop || !launches) return IWAE_EINVAL;
  HIPCHK(hipStreamSynchronize(h->stream));
  double ms = 0.0;
  for (size_t i = 0; i + 1 < h->prof.used; i += 2) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, h->prof.ev[i], h->prof.ev[i + 1]));
    ms += t;
  }
  *total_ms = ms;
  *total_flop = h->prof.flop;
  *launches = (long long)(h->prof.used / 2);
  return IWAE_OK;
}

}  // extern "C"
