/*
 * gnca.h — C ABI of the MI355X-native NCA rollout step (libgnca.so).
 *
 * This is the drop-in boundary for ONE hot path of Psylocibe23/Graph_Neural_Cellular_Automata:
 * the per-cell CA update of NeuralCAGraph.forward / NeuralCA.forward plus the mid-range graph
 * residual of GraphAugmentation.forward.  The reference has no FFI of its own: its boundary is
 * the Python nn.Module API, and the Python package graph_neural_cellular_automata_amd mirrors
 * that API on top of these entry points (ctypes).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Every tensor pointer is DEVICE memory, fp32, NCHW contiguous (the reference's layout),
 *     caller-owned.  Weight pointers use the reference's parameter layouts (Conv2d weights
 *     [out,in,1,1] / [3C,1,3,3]); no host-side repacking is needed.
 *   - All work is stream-ordered on `stream`; no entry point synchronises the device, allocates
 *     memory or copies host<->device, so calls can be captured into a hipGraph.
 *   - Return value: 0 (GNCA_OK) or a negative gnca_status; gnca_status_string() names it.
 *   - Stateless and reentrant (gnca_rollout_f32's sub-batch streams are per-device helpers whose
 *     enqueue is serialised by an internal lock).
 *   - The prior contents of `ws`, `tape` and every output buffer are ignored, and every output is
 *     written completely, unless an entry point says otherwise (a continuation piece of
 *     gnca_rollout_ex_f32 reads what the previous piece left in `ws`; `saved` and `tape` are read by
 *     the backward that they are passed to).
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   gnca_step_f32        NeuralCAGraph.forward        src/modules/ncagraph.py:106-168
 *                        NeuralCA.forward (graph off) src/modules/nca.py:64-105
 *                        GraphAugmentation.forward    src/modules/graph_augmentation.py:104-169
 *                        FixedSobelPerception.forward src/modules/perception.py:21-26
 *   gnca_message_f32     GraphAugmentation.forward    src/modules/graph_augmentation.py:104-169
 *   gnca_perceive_f32    FixedSobelPerception.forward src/modules/perception.py:21-26
 *   gnca_rollout_f32     the rollout loops that call the step once per CA step, e.g.
 *                        src/training/train_graph_augmented_nca.py:305-321,
 *                        src/testing/test_graph_augmented_regeneration.py:183-194
 *   gnca_damage_f32      the damage curriculum's batch ops, src/utils/damage.py:15-138
 *   gnca_damage_policy   apply_damage_policy_ with its draws, src/utils/damage.py:99-138
 *   gnca_step_bwd_f32    torch autograd's backward through NeuralCAGraph.forward /
 *                        NeuralCA.forward, i.e. the per-step part of the trainers'
 *                        loss.backward() (BPTT): src/training/train_graph_augmented_nca.py:369,
 *                        src/training/train_intermediate_loss.py (same loop)
 *   gnca_loss_masked_f32     masked_loss, src/training/train_intermediate_loss.py:37-51 and
 *                            src/training/train_graph_augmented_nca.py:30-49
 *   gnca_loss_stability_f32  the stability phase's loss on the close samples,
 *                            src/training/train_intermediate_loss.py:256-267
 *   gnca_optim_step          the gradient policy and optimizer.step(),
 *                            src/training/train_graph_augmented_nca.py:367-375 and
 *                            src/training/train_intermediate_loss.py:280-283
 *   gnca_pool_commit         the pool write-back with worst-k reset and random reseed,
 *                            src/training/train_graph_augmented_nca.py:377-391 and
 *                            src/training/train_intermediate_loss.py:269-296
 *   gnca_graph_diag          debug_graph_from_state, src/testing/test_graph_augmented_nca.py:77-158,
 *                            and the |M| group maps of
 *                            src/testing/test_graph_augmented_regeneration.py:196-204
 */
#ifndef GNCA_H
#define GNCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNCA_ABI_VERSION 5
#define GNCA_MAX_OFFSETS 128   /* >= (2r+1)^2-9 for r <= 5 (112) */

/* gnca_step_desc.flags */
#define GNCA_GRAPH          (1u << 0)  /* NeuralCAGraph (graph message on); clear = NeuralCA  */
#define GNCA_USE_GROUPNORM  (1u << 1)  /* nn.GroupNorm(1,C,eps) on dx (ncagraph.py:68)       */
#define GNCA_HIDDEN_ONLY    (1u << 2)  /* zero message channels 0..3 (ncagraph.py:98-100)     */
#define GNCA_ALIVE_TO_ALIVE (1u << 3)  /* mask messages by sender alive (graph_aug.py:131)   */
#define GNCA_ZERO_PAD_SHIFT (1u << 4)  /* _shift2d_pad (dx ignored) instead of torch.roll     */
#define GNCA_ATTENTION      (1u << 5)  /* also write the normalised attention map [B,H,W]    */

/* gnca_step_desc.fire_mode: the stochastic fire mask of ncagraph.py:144-146 */
#define GNCA_FIRE_NONE      0  /* fire_rate >= 1: no mask                                   */
#define GNCA_FIRE_RAND_F32  1  /* fire = (fire[b,0,i,j] <= fire_rate), fire = torch.rand(B,1,H,W) */
#define GNCA_FIRE_MASK_U8   2  /* fire = (fire[b,0,i,j] != 0), an explicit uint8 mask         */
#define GNCA_FIRE_HASH      3  /* counter RNG: u(seed, rng_step, sample_base+b, i*W+j) <= fire_rate */

typedef enum gnca_status {
  GNCA_OK = 0,
  GNCA_ERR_INVALID = -1,      /* bad shape / argument / null pointer                      */
  GNCA_ERR_UNSUPPORTED = -2,  /* shape class not compiled in: needs 4 <= C <= 32 and
                                 hidden <= 128 (<= 256 for 13 <= C <= 16)                 */
  GNCA_ERR_WORKSPACE = -3,    /* workspace too small (see gnca_workspace_bytes)            */
  GNCA_ERR_HIP = -4           /* a HIP launch failed; gnca_last_hip_error() has the code   */
} gnca_status;

typedef struct gnca_step_desc {
  int32_t B, C, H, W;         /* state shape, C >= 4 (alpha is channel 3)                    */
  int32_t hidden;             /* update_hidden (update_net.0 out channels)                   */
  int32_t d_model;            /* graph d_model (query/key channels)                          */
  int32_t num_offsets;        /* k = len(chosen offsets) this step, 0..GNCA_MAX_OFFSETS      */
  int32_t fire_mode;          /* GNCA_FIRE_*                                                 */
  uint32_t flags;             /* GNCA_* flag bits                                            */
  float update_gain;          /* NeuralCAGraph.update_gain                                    */
  float alpha_thr;            /* NeuralCAGraph.alpha_thr: pre/post-update alive masks         */
  float graph_alpha_thr;      /* GraphAugmentation.alpha_thr: sender mask (copied at ctor,
                                 ncagraph.py:79 -> graph_augmentation.py:52,117)              */
  float message_gain;         /* NeuralCAGraph.message_gain, read per call                    */
  float gn_eps;               /* GroupNorm eps (1e-3 in the reference)                        */
  float fire_rate;            /* forward(fire_rate)                                          */
  uint64_t rng_seed;          /* GNCA_FIRE_HASH only                                          */
  int64_t rng_step;           /* GNCA_FIRE_HASH only: step index in the rollout               */
  int64_t sample_base;        /* GNCA_FIRE_HASH only: global index of sample 0 of this shard  */
  int8_t offsets[2 * GNCA_MAX_OFFSETS]; /* (dy,dx) pairs in random.sample order            */
} gnca_step_desc;

typedef struct gnca_weights {
  const float* perception;    /* perception.conv.weight [3C,1,3,3]                          */
  const float* w1;            /* update_net.0.weight    [hidden,3C,1,1]                     */
  const float* b1;            /* update_net.0.bias      [hidden]                            */
  const float* w2;            /* update_net.2.weight    [C,hidden,1,1]                      */
  const float* gn_weight;     /* norm.weight [C] (NULL if !GNCA_USE_GROUPNORM)              */
  const float* gn_bias;       /* norm.bias   [C]                                            */
  const float* wq;            /* graph.query_proj.weight [d,C,1,1]  (graph only)            */
  const float* bq;            /* graph.query_proj.bias   [d]                                */
  const float* wk;            /* graph.key_proj.weight   [d,C,1,1]                          */
  const float* bk;            /* graph.key_proj.bias     [d]                                */
  const float* wm;            /* graph.msg_proj.weight   [C,C,1,1]                          */
  const float* bm;            /* graph.msg_proj.bias     [C]                                */
  const float* scaling;       /* graph.scaling           [] (device scalar)                 */
} gnca_weights;

/* ABI version (GNCA_ABI_VERSION) — lets a binding check it loaded a matching library. */
int gnca_abi_version(void);

/* Human-readable name of a gnca_status. */
const char* gnca_status_string(int status);

/* The hipError_t of the last failed launch on this thread (0 if none). */
int gnca_last_hip_error(void);

/* Bytes of device workspace gnca_step_f32 needs for `desc` (0 on invalid desc). */
size_t gnca_workspace_bytes(const gnca_step_desc* desc);

/* Measurement: the K1 kernel the plan for `desc` launches, as "name<template args>" (NUL-terminated,
 * truncated to n bytes), and its MFMA arithmetic in *arith (may be NULL): 0 = fp32 MFMA
 * (v_mfma_f32_*_f32), 1 = bf16 MFMA on exact 3-way splits of the fp32 operands (6 products per
 * fp32 product, gnca_k1_split.h), plus 2 when a rollout of this shape uses the compact update field
 * (GNCA_PHASE_COMPACT), plus 4 when a rollout of this shape runs as 2 concurrent sub-batches (one
 * stream each: one sub-batch's K2 beside the other's K1; see gnca_rollout_f32), plus 8 when a
 * rollout of this shape folds each step's finish (GroupNorm, tanh, residual, alpha gate) into the
 * next step's K1 (one K1 launch per step and one K2 at the end), plus 16 when such a fold is
 * possible for this shape (on request, GNCA_ROLLOUT_FOLD, where it is not the default).  Host-only.
 * Returns GNCA_OK or GNCA_ERR_INVALID. */
int gnca_k1_variant(const gnca_step_desc* desc, char* name, int32_t n, int32_t* arith);

/* Measurement: the K2 (finalize) kernel a step of `desc` launches, as "name<template args>":
 * "gnca_k2_finalize_flat<V,CU>" (one thread per V-cell vector, no LDS; compact update field only) or
 * the band kernel "gnca_k2_finalize<V,COMPACT,CU,ROWS>".  co = 1: a step of a rollout's sub-batch
 * pipeline, K2 beside the other sub-batch's K1 (GNCA_ERR_INVALID when a rollout of this shape runs
 * on one stream); co = 0: a rollout step with K2 alone on the chip (one-stream rollouts, the last K2
 * of a fold); co = -1: a single step (gnca_step_f32, gnca_step_masked_f32: the dense update field).
 * Host-only.  Returns GNCA_OK or GNCA_ERR_INVALID. */
int gnca_k2_variant(const gnca_step_desc* desc, int32_t co, char* name, int32_t n);

/*
 * One CA step: x_out = step(x).  Out-of-place (x_out must not alias x), like the reference.
 *   fire:  NULL, or [B,1,H,W] fp32 uniforms (GNCA_FIRE_RAND_F32) / uint8 mask (GNCA_FIRE_MASK_U8)
 *   attn:  [B,H,W] fp32, written iff GNCA_ATTENTION (min-max normalised, graph_aug.py:160-167)
 *   ws:    >= gnca_workspace_bytes(desc) bytes of device memory, 256-B aligned
 */
int gnca_step_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                  float* x_out, const void* fire, float* attn, void* ws, size_t ws_bytes,
                  void* stream);

/*
 * One step restricted to the samples with active[b] != 0 (active: uint8 [B], device memory); the
 * other samples are copied through unchanged and do not fire.  Replaces the trainers'
 * `state[mask] = model(state[mask], fire_rate)` variable-length rollout masking
 * (src/training/train_graph_augmented_nca.py:305-321) without the gather/scatter copies of the
 * sub-batch and without a host-side mask.any() sync.  `fire` (GNCA_FIRE_RAND_F32 / MASK_U8) is
 * indexed by the full batch; GNCA_ATTENTION is not supported here.
 */
int gnca_step_masked_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                         float* x_out, const void* fire, const uint8_t* active, void* ws,
                         size_t ws_bytes, void* stream);

/* Measurement hook: run only the step's kernels named in `phases` (GNCA_PHASE_* bits) with the
 * same arguments as gnca_step_f32.  gnca_step_f32 == all phases.  Skipping a phase leaves its
 * outputs stale; bench.py uses this to time K1 alone with HIP events on `stream`. */
#define GNCA_PHASE_K0 (1u << 0)  /* zero-pad offset weights                */
#define GNCA_PHASE_K1 (1u << 1)  /* perceive + gather + MLP -> dx, partials */
#define GNCA_PHASE_K2 (1u << 2)  /* GroupNorm + residual + alive gate       */
#define GNCA_PHASE_ALL (GNCA_PHASE_K0 | GNCA_PHASE_K1 | GNCA_PHASE_K2)
/* Rollout mode of the measurement hook: K2 writes the next step's alive masks into the workspace
 * and K1 reads them (what gnca_rollout_f32 does for every step after the first; needs
 * 0 <= alpha_thr <= graph_alpha_thr, and a K2 call with this bit on the same workspace first).
 * On a zero-padded-shift graph step with GNCA_PHASE_COMPACT as well, that K2 also hands over the
 * new state's per-(channel, row) sums and the next K0 reads them instead of recomputing them: both
 * calls of such a pair must carry the same flags (a pair that mixes COMPACT and non-COMPACT calls
 * would read stale sums). */
#define GNCA_PHASE_ALIVE (1u << 3)
/* Rollout mode's compact update field (what gnca_rollout_f32 does for every step when the planned
 * K1 is the 16-channel split kernel): K1 writes dx only for its live cells, packed per tile in
 * live-cell order with per-tile-row live masks, and K2 reads them back (dead cells have dx = 0).
 * Both the K1 and the K2 call of a step must carry it; ignored for other K1 variants. */
#define GNCA_PHASE_COMPACT (1u << 4)
int gnca_step_phases_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                         float* x_out, const void* fire, float* attn, void* ws, size_t ws_bytes,
                         void* stream, uint32_t phases);

/*
 * GraphAugmentation.forward alone: agg_message [B,C,H,W] (before the message policy) and, if
 * GNCA_ATTENTION, the normalised attention map.  Uses desc's graph fields only.
 */
int gnca_message_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                     float* message, float* attn, void* ws, size_t ws_bytes, void* stream);

/* FixedSobelPerception.forward: y [B,3C,H,W] in the reference's [id.., sobel_x.., sobel_y..] order. */
int gnca_perceive_f32(int32_t B, int32_t C, int32_t H, int32_t W, const float* weight,
                      const float* x, float* y, void* stream);

/*
 * A whole no-grad rollout of `steps` CA steps with GNCA_FIRE_HASH (or GNCA_FIRE_NONE) masks:
 * step t uses offsets[t*2*k .. ] (host array, k = desc->num_offsets pairs per step) and
 * rng_step = desc->rng_step + t.  x is read, x_final receives the last state; scratch holds
 * one more state ([B,C,H,W] fp32).  Equivalent to `steps` gnca_step_f32 calls.  Large batches
 * (gnca_k1_variant's arith bit 4) run as 2 sub-batches of samples, each on its own stream forked
 * from and joined back into `stream` (stream-ordered for the caller, capturable), so that one
 * sub-batch's memory-bound finalize kernel runs on the CUs beside the other's MFMA kernel; the
 * results are bitwise those of one stream.  `ws` then holds one workspace per sub-batch
 * (gnca_workspace_bytes accounts for it).
 */
int gnca_rollout_f32(const gnca_step_desc* desc, const gnca_weights* w, int32_t steps,
                     const int8_t* offsets, const float* x, float* x_final, float* scratch,
                     void* ws, size_t ws_bytes, void* stream);

/*
 * gnca_rollout_f32 in pieces: a long rollout issued as several calls (the host draws the next
 * piece's offsets while the device runs the previous piece) computes exactly the one-call result
 * when the pieces hand the alive masks over through the shared workspace:
 *   GNCA_ROLLOUT_ALIVE_OUT  the last step's K2 also writes the next state's alive masks into `ws`
 *                           (zero-padded shift on the compact field: and its fp64 row sums for K0)
 *   GNCA_ROLLOUT_ALIVE_IN   the first step's K1 reads them from `ws` (written by the previous call
 *                           with ALIVE_OUT on the same workspace; x = that call's x_final)
 * Both need 0 <= alpha_thr <= graph_alpha_thr (else GNCA_ERR_INVALID).  flags = 0 is gnca_rollout_f32.
 * A rollout that runs as concurrent sub-batches (gnca_rollout_f32) forks its helper streams in the
 * first piece and joins them into `stream` in the last one (the piece without ALIVE_OUT): between
 * pieces, x_final is complete on `stream` only for sub-batch 0, so the caller must not read it
 * before the last piece; continuation pieces reuse the first piece's weight images in `ws`.
 */
#define GNCA_ROLLOUT_ALIVE_IN  (1u << 0)
#define GNCA_ROLLOUT_ALIVE_OUT (1u << 1)
/*
 * Rollouts that fold each step's finish into the next step's K1 (gnca_k1_variant's arith bit 8: one
 * K1 launch per step, one K2 at the end) can hand the LAST step over unfinished instead, which
 * saves the K2 and the next piece's plain first K1:
 *   GNCA_ROLLOUT_PENDING_OUT  the last step is left pending: x_final receives the state BEFORE the
 *                             last step and `ws` holds that step's update field
 *   GNCA_ROLLOUT_PENDING_IN   x is such a state and `ws` the pending field of the previous call
 *                             (same desc shape, workspace and stream; desc->rng_step continues the
 *                             previous call's: the field's buffer is chosen by the step's parity)
 * A piece chain PENDING_OUT, PENDING_IN|PENDING_OUT, ..., PENDING_IN computes exactly the one-call
 * rollout.  GNCA_ERR_INVALID when the rollout does not fold, or combined with ALIVE_IN / ALIVE_OUT
 * on the same side.
 */
#define GNCA_ROLLOUT_PENDING_IN  (1u << 2)
#define GNCA_ROLLOUT_PENDING_OUT (1u << 3)
/* Fold even on the compact update field (gnca_k1_variant arith bit 16): large batches otherwise run
 * the two-stream sub-batch pipeline, which measured faster on MI355X ("The fold").
 * Where the request changes the plan (it is not the default for this shape), it is GNCA_ERR_INVALID
 * together with ALIVE_IN / ALIVE_OUT: every piece of an ALIVE chain must run one plan, and a fold
 * chain hands over with PENDING_IN / PENDING_OUT instead. */
#define GNCA_ROLLOUT_FOLD        (1u << 4)
int gnca_rollout_ex_f32(const gnca_step_desc* desc, const gnca_weights* w, int32_t steps,
                        const int8_t* offsets, const float* x, float* x_final, float* scratch,
                        void* ws, size_t ws_bytes, uint32_t flags, void* stream);

/*
 * Measurement twin of gnca_rollout_f32: the same launches, and every K1 / K2 workgroup also writes
 * two wall-clock stamps (the 100 MHz s_memrealtime counter: at its first instruction and after its
 * last barrier) into `stamps` (device memory, uint64, zero-initialised by the caller):
 *   stamps[(((t * nsub + j) * 2 + k) * stamp_cap + wg) * 2 + {0: start, 1: end}],
 *   t = step, j = sub-batch (nsub = 2 when gnca_k1_variant's arith has bit 4, else 1),
 *   k = 0 (K1) / 1 (K2)
 * so a launch's duration is max(end) - min(start) over its workgroups, with no event or marker in
 * the stream between launches.  GNCA_ERR_INVALID if a launch has more than stamp_cap workgroups.
 */
int gnca_rollout_stamped_f32(const gnca_step_desc* desc, const gnca_weights* w, int32_t steps,
                             const int8_t* offsets, const float* x, float* x_final, float* scratch,
                             void* ws, size_t ws_bytes, uint64_t* stamps, int32_t stamp_cap,
                             void* stream);

/*
 * The fire mask a GNCA_FIRE_HASH step would draw: mask[b,0,i,j] = u(rng_seed, rng_step,
 * sample_base+b, i*W+j) <= fire_rate, as uint8 [B,1,H,W] (1 = fires).  For inspection and for
 * replaying a hash-masked rollout elsewhere (e.g. as GNCA_FIRE_MASK_U8).
 */
int gnca_fire_mask_u8(const gnca_step_desc* desc, uint8_t* mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward (BPTT).  Gradients of one step, written into caller buffers (overwritten, not
 * accumulated), in the reference's parameter layouts.  A NULL pointer skips that gradient's
 * write (e.g. gn_weight/gn_bias without GNCA_USE_GROUPNORM, the graph fields for NeuralCA).
 * -------------------------------------------------------------------------------------------*/
typedef struct gnca_grads {
  float* w1;          /* d update_net.0.weight  [hidden,3C,1,1] */
  float* b1;          /* d update_net.0.bias    [hidden]        */
  float* w2;          /* d update_net.2.weight  [C,hidden,1,1]  */
  float* gn_weight;   /* d norm.weight          [C]             */
  float* gn_bias;     /* d norm.bias            [C]             */
  float* wq;          /* d graph.query_proj.weight [d,C,1,1]    */
  float* bq;          /* d graph.query_proj.bias   [d]          */
  float* wk;          /* d graph.key_proj.weight   [d,C,1,1]    */
  float* bk;          /* d graph.key_proj.bias     [d]          */
  float* wm;          /* d graph.msg_proj.weight   [C,C,1,1]    */
  float* bm;          /* d graph.msg_proj.bias     [C]          */
  float* scaling;     /* d graph.scaling           []           */
} gnca_grads;

/* Bytes of device workspace gnca_step_bwd_f32 needs for `desc` (0 on invalid desc). */
size_t gnca_bwd_workspace_bytes(const gnca_step_desc* desc);

/* Measurement: the backward MLP kernel (BB) the plan for `desc` launches without an active-sample
 * mask, as "gnca_b_mlp<CP,HB,FULL,TH,TW,RY,RX,K,LEAN>" (TH .. K 0 / -1 for the runtime-geometry
 * kernels; NUL-terminated, truncated to n bytes); a masked step never takes the LEAN (24x24) tiles.
 * Host-only.  Returns GNCA_OK or GNCA_ERR_INVALID. */
int gnca_bb_variant(const gnca_step_desc* desc, char* name, int32_t n);

/*
 * Vector-Jacobian product of one step: given the step input x (and the same desc, weights and
 * fire input as the forward call) and gy = dL/d x_out, write gx = dL/dx and the parameter
 * gradients.  The alive / fire masks are constants, the perception weight is frozen (no
 * gradient), as in the reference's autograd graph.  In torus mode the offset weights are exactly
 * uniform, so the query/key/scaling gradients are exactly zero.  gx must not alias x or gy.
 *   active: NULL, or the uint8 [B] sample mask of a gnca_step_masked_f32 forward (inactive
 *           samples: gx = gy, no parameter gradient).
 *   saved: the workspace of the gnca_step_f32 call that produced x_out (same desc, weights, x
 *          and fire), kept unmodified since: its update field and GroupNorm partials are reused.
 *          NULL: the backward recomputes them (one more forward pass).
 */
int gnca_step_bwd_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                      const void* fire, const uint8_t* active, const float* gy, float* gx,
                      const gnca_grads* grads, const void* saved, void* ws, size_t ws_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-rollout forward and BPTT: `steps` CA steps in one call each way, on a per-step schedule.
 * The forward writes every step's input state (and, unless GNCA_SCHED_RECOMPUTE, the step's
 * workspace: update field, GroupNorm partials, zero-pad offset weights and row sums) into `tape`,
 * one slot per step, each step writing straight into the next slot; the backward walks the tape in
 * reverse, keeps the weight-gradient partial rows in the workspace across steps (every row is owned
 * by one (workgroup, wave) and steps arrive in stream order: a deterministic sum, no float
 * atomics) and reduces them once.  Equivalent to `steps` gnca_step_masked_f32 / gnca_step_f32 calls
 * and the sum of their gnca_step_bwd_f32 gradients.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_SCHED_RECOMPUTE (1u << 0)  /* tape keeps states only; the backward recomputes K0/K1 */
/*
 * Segment checkpointing, k = ckpt_every >= 1 (else GNCA_ERR_INVALID / size 0).  The tape keeps only
 * the anchors S_0, S_k, S_2k, ...: A = ceil(T/k) states, each 256-byte aligned,
 *   gnca_rollout_tape_bytes = A * align256(B*C*H*W*4)                         (0 for T = 0),
 * and never a step workspace.  The forward writes the states between two anchors into the two
 * buffers of its workspace (the no-tape form's; gnca_rollout_fwd_workspace_bytes does not grow).
 * The backward takes the segments j = A-1 .. 0 in turn: it re-runs the forward of the segment's
 * steps from anchor j into a segment area of its own workspace (the same step calls, descriptors,
 * masks and fire inputs as the forward: the states are reproduced bit for bit), then walks the
 * segment backwards as the plain backward does.  The last step of a segment is not re-run (nobody
 * reads its output): its backward recomputes K0 / K1, as under GNCA_SCHED_RECOMPUTE.  With
 * m = min(k, T),
 *   gnca_rollout_bwd_workspace_bytes = (the plain schedule's) + (m-1) * state + n_ws * fwd_ws,
 *   n_ws = m-1                    each re-run step keeps its forward workspace for its backward, or
 *   n_ws = min(m-1, 1)            with GNCA_SCHED_RECOMPUTE: one workspace for the re-run steps,
 * state = align256(B*C*H*W*4), fwd_ws = the schedule's largest step workspace (256-byte aligned).
 * The accumulating rows are zeroed once, the steps' backwards arrive in the order T-1 .. 0 and each
 * reduction runs once, so every gradient is bitwise that of the plain tape.  k = 1 keeps every
 * state, k >= T only a copy of x.
 */
#define GNCA_SCHED_CHECKPOINT (1u << 1)

typedef struct gnca_rollout_sched {
  int32_t steps;              /* T, host                                                        */
  int32_t full_steps;         /* steps t < full_steps run every sample whatever nsteps says     */
  uint32_t flags;
  int32_t ckpt_every;         /* k; read only with GNCA_SCHED_CHECKPOINT (it took the place of the
                                 padding after flags: no offset and no size changed)            */
  const int8_t* offsets;     /* host  [T][2*desc->num_offsets], as gnca_rollout_f32            */
  const float* fire_rate;     /* host  [T], NULL = desc->fire_rate for every step               */
  const float* message_gain;  /* host  [T], NULL = desc->message_gain                           */
  const int32_t* nsteps;      /* DEVICE [B]: sample b takes step t iff t < nsteps[b]; NULL = all */
  const void* fire;           /* DEVICE [T][B,1,H,W] for GNCA_FIRE_RAND_F32 / MASK_U8; NULL for
                                 GNCA_FIRE_HASH (rng_step = desc->rng_step + t) / GNCA_FIRE_NONE */
} gnca_rollout_sched;

/* Bytes of `tape` a rollout of this schedule records (0 on an invalid desc or schedule; 0 steps
 * record nothing).  Host-only: reads the schedule's host arrays, never nsteps / fire. */
size_t gnca_rollout_tape_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched);

/* Bytes of device workspace gnca_rollout_fwd_f32 / gnca_rollout_bwd_f32 need (0 on an invalid
 * desc or schedule).  Host-only.  The forward's covers the no-tape form (two state buffers). */
size_t gnca_rollout_fwd_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched);
size_t gnca_rollout_bwd_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched);

/*
 * The rollout: x is read, x_final receives the state after the last step (x_final must not alias
 * x).  tape: >= gnca_rollout_tape_bytes bytes, 256-B aligned, or NULL for the no-grad form of the
 * same schedule (the states then alternate between two buffers in `ws`).  nsteps is turned into
 * the per-step active masks on the device (one launch); it is never read on the host.
 * With GNCA_SCHED_CHECKPOINT only the states S_k, S_2k, ... go to the tape (and a copy of x as
 * S_0); the others alternate between the two buffers in `ws`, and every step uses the step
 * workspace in `ws`.
 */
int gnca_rollout_fwd_f32(const gnca_step_desc* desc, const gnca_weights* w,
                         const gnca_rollout_sched* sched, const float* x, float* x_final, void* tape,
                         size_t tape_bytes, void* ws, size_t ws_bytes, void* stream);

/*
 * BPTT through the rollout that wrote `tape` (same desc, weights and schedule, the tape unmodified
 * since): gy = dL/d x_final, gx = dL/dx (must not alias gy), grads written once (overwritten, in
 * the layouts of gnca_grads; a NULL pointer skips that gradient; grads itself may be NULL).
 * With GNCA_SCHED_CHECKPOINT each segment's forward is re-run first (see the flag); x_final, gx and
 * every gradient are bitwise those of the same schedule without the flag.
 */
int gnca_rollout_bwd_f32(const gnca_step_desc* desc, const gnca_weights* w,
                         const gnca_rollout_sched* sched, const void* tape, size_t tape_bytes,
                         const float* gy, float* gx, const gnca_grads* grads, void* ws,
                         size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The attention map as a side computation, and a rollout that records frames and maps.
 * -------------------------------------------------------------------------------------------*/

/* Bytes of device workspace gnca_attention_f32 needs for `desc` (0 on an invalid desc). */
size_t gnca_attention_workspace_bytes(const gnca_step_desc* desc);

/*
 * The normalised attention map of GraphAugmentation.forward (graph_augmentation.py:160-167) for the
 * state x and desc's offsets, without the step: attn [B,H,W], min-max normalised per sample.  Reads
 * desc's B, C (<= 32), H, W, offsets, graph_alpha_thr (d_model for the zero-padded shift) and the
 * flags GNCA_GRAPH, GNCA_ALIVE_TO_ALIVE, GNCA_ZERO_PAD_SHIFT; every other field is ignored.  Weights:
 * wm, bm (and wq, bq, wk, bk, scaling for the zero-padded shift's per-sample offset weights).  Graph
 * off or num_offsets == 0: zeros.  Bitwise reproducible (no atomics).
 */
int gnca_attention_f32(const gnca_step_desc* desc, const gnca_weights* w, const float* x, float* attn,
                       void* ws, size_t ws_bytes, void* stream);

typedef struct gnca_trace_args {
  int32_t steps;              /* T                                                              */
  int32_t num_records;        /* R                                                              */
  int32_t frame_channels;     /* channels 0 .. frame_channels-1 of each frame, 1 .. C           */
  uint32_t flags;             /* reserved: 0                                                    */
  const int8_t* offsets;      /* host  [T][2*desc->num_offsets], as gnca_rollout_f32            */
  const int32_t* record;      /* host  [R], strictly increasing, values in 1 .. T               */
  float* frames;              /* DEVICE [R,B,frame_channels,H,W]: the state after step record[r] */
  float* attn;                /* DEVICE [R,B,H,W] or NULL: the map of step record[r], computed
                                 from that step's input state with that step's offsets          */
} gnca_trace_args;

/* Bytes of device workspace gnca_rollout_trace_f32 needs (0 on an invalid desc or args).  Host-only:
 * reads args->record, args->offsets (the widest step plan) and whether args->attn is set. */
size_t gnca_rollout_trace_workspace_bytes(const gnca_step_desc* desc, const gnca_trace_args* args);

/*
 * gnca_rollout_f32 that also records: the same uniform schedule (one desc, GNCA_FIRE_HASH / NONE,
 * step t uses args->offsets[t*2*k ..] and rng_step = desc->rng_step + t), issued as pieces of the
 * plain rollout that end at the record points (and, with maps, one step before them), so every
 * piece runs the plan gnca_rollout_f32 picks for the shape.  The frames, the maps and x_final are
 * bitwise those of separate gnca_rollout_f32 / gnca_attention_f32 calls.  Everything is enqueued
 * from this one call, stream-ordered on `stream`, with no host synchronisation.  x_final must not
 * alias x.
 */
int gnca_rollout_trace_f32(const gnca_step_desc* desc, const gnca_weights* w, const gnca_trace_args* args,
                           const float* x, float* x_final, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image metrics on the device, and a recording rollout that measures.
 * -------------------------------------------------------------------------------------------*/

/*
 * The trainers' per-iteration quality figures (src/training/train_graph_augmented_nca.py:405-422,
 * skimage's structural_similarity / peak_signal_noise_ratio with their defaults), for every image of
 * a batch: out[n*4 + {0,1,2,3}] = mse, pixel_perfect, psnr, ssim of image n.  Layouts as
 * gnca_loss_premult_f32: pred [N,4,H,W] with sample stride pred_bstride floats and channel stride
 * H*W, target premultiplied RGBA with sample stride target_bstride (0 = broadcast).
 * With P = (pred_rgb * pred_alpha, pred_alpha) (the product rounded to fp32), T = target,
 * X = clip(P_rgb, 0, 1), Y = clip(T_rgb, 0, 1):
 *   mse            mean over 4 channels and all cells of (P - T)^2 (gnca_loss_premult_f32's value)
 *   pixel_perfect  fraction of cells with |P_c - T_c| < 0.05 (fp32) in all 4 channels
 *   psnr           10 log10(1 / mean((X - Y)^2)) over the 3 colour channels; +inf when the mean is 0
 *   ssim           mean over the colour channels and all (H-6)(W-6) full 7x7 windows of
 *                  (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), window means m,
 *                  sample (co)variances v = 49/48 (mxy - mx my), C1 = 1e-4, C2 = 9e-4;
 *                  NaN when H < 7 or W < 7 (the other three are still computed)
 * Everything after the fp32 premultiply and clip is fp64.  Fixed-order sums, no atomics: an image's
 * four results are bitwise the same whatever N is and wherever the image stands in the batch.
 * ws: >= gnca_image_metrics_workspace_bytes(N, H, W) bytes of device memory, 8-B aligned (may be
 * NULL when that is 0).
 */
size_t gnca_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W);
int gnca_image_metrics_f32(int32_t N, int32_t H, int32_t W, const float* pred, int64_t pred_bstride,
                           const float* target, int64_t target_bstride, float* out, void* ws,
                           size_t ws_bytes, void* stream);

typedef struct gnca_trace_metrics {
  const float* target;      /* DEVICE, premultiplied RGBA [4,H,W] or [B,4,H,W]                   */
  int64_t target_bstride;   /* 0 = broadcast                                                     */
  float* out;               /* DEVICE [R,B,4]: the metrics of the state after step record[r]     */
} gnca_trace_metrics;

/*
 * gnca_rollout_trace_f32 that also measures: the same pieces, and at each record point the image
 * metrics of channels 0..3 of the piece's output state (read in place) go to out[r].  args->frames
 * may be NULL here (metrics without frames); args->attn as before.  The metrics are bitwise those of
 * gnca_image_metrics_f32 on the recorded frames.  m->target and m->out both NULL: nothing is measured.
 */
size_t gnca_rollout_trace_metrics_workspace_bytes(const gnca_step_desc* desc, const gnca_trace_args* args,
                                                  const gnca_trace_metrics* m);
int gnca_rollout_trace_metrics_f32(const gnca_step_desc* desc, const gnca_weights* w,
                                   const gnca_trace_args* args, const gnca_trace_metrics* m, const float* x,
                                   float* x_final, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph diagnostics: the decomposition of the attention map that the evaluation scripts draw
 * (src/testing/test_graph_augmented_nca.py:77-158, debug_graph_from_state, and the per-group message
 * magnitudes of src/testing/test_graph_augmented_regeneration.py:196-204), for any batch.  Neither
 * name carries the _f32 suffix.
 * -------------------------------------------------------------------------------------------*/

/*
 * With m = W_M x + b_M, src = the sender mask (3x3 max-pool of alpha > graph_alpha_thr) under
 * GNCA_ALIVE_TO_ALIVE and 1 otherwise, w_o[b] the step's offset weights (1/k on the torus, the
 * per-sample softmax of gnca_step_f32's zero-padded shift), shift_o the step's shift (torus roll;
 * zero-padded: rows only, dx ignored), the channel groups g0 = 0..2, g1 = 3, g2 = 4..C-1 (empty when
 * C = 4: zeros), G_g(p) = mean_{c in g} |m_c(p)| and S(p) = src(p) mean_c |m_c(p)|:
 * all DEVICE fp32, any pointer may be NULL and is then skipped.
 */
typedef struct gnca_graph_diag_out {
  float* magnitude;     /* [B,3,H,W]  G_g: unmasked, unweighted                                  */
  float* groups;        /* [B,3,H,W]  sum_o w_o shift_o(src G_g)                                 */
  float* per_offset;    /* [B,k,H,W]  w_o shift_o(S), in offset order                            */
  float* raw;           /* [B,H,W]    sum_o w_o shift_o(S): the un-normalised map                */
  float* attention;     /* [B,H,W]    raw min-max normalised per sample: gnca_attention_f32's map, bitwise */
  float* sender_union;  /* [B,H,W]    {0,1}: max_o shift_o(src) under GNCA_ALIVE_TO_ALIVE, else zeros */
  float* receiver;      /* [B,H,W]    {0,1}: 3x3 max-pool of alpha > graph_alpha_thr             */
  float* weights;       /* [B,k]      w_o[b]                                                     */
} gnca_graph_diag_out;

/* Bytes of device workspace gnca_graph_diag needs for `desc` (0 on an invalid desc).  Host-only. */
size_t gnca_graph_diag_workspace_bytes(const gnca_step_desc* desc);

/*
 * The diagnostics of state x for desc's offsets, without the step.  Reads the desc fields and weights
 * gnca_attention_f32 reads (C <= 32).  num_offsets == 0: every map is zero except magnitude and
 * receiver (per_offset and weights are empty); graph off: magnitude is zero too and no weight is read.
 * Every requested output is written completely.  Fixed-order sums, no atomics: bitwise reproducible,
 * and a sample's results do not depend on B or on its position in the batch.  per_offset summed over
 * o equals raw to rounding (raw accumulates with fused multiply-adds).
 */
int gnca_graph_diag(const gnca_step_desc* desc, const gnca_weights* w, const float* x,
                    const gnca_graph_diag_out* out, void* ws, size_t ws_bytes, void* stream);

/*
 * gnca_rollout_trace_metrics_f32 that also records the diagnostics of every recorded step, computed
 * from that step's input state with that step's offsets (the convention of args->attn): `diag` holds
 * [R,...]-leading versions of the outputs above ([R,B,3,H,W], [R,B,k,H,W], [R,B,H,W], [R,B,k]), any
 * of them NULL.  metrics may be NULL (gnca_rollout_trace_f32's form).  The rollout's launches and the
 * other outputs are those of the call without `diag`, bitwise.
 */
size_t gnca_rollout_trace_diag_workspace_bytes(const gnca_step_desc* desc, const gnca_trace_args* args,
                                               const gnca_trace_metrics* metrics);
int gnca_rollout_trace_diag(const gnca_step_desc* desc, const gnca_weights* w, const gnca_trace_args* args,
                            const gnca_trace_metrics* metrics, const gnca_graph_diag_out* diag, const float* x,
                            float* x_final, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * State vitals: how much of a state is alive, where its pattern lies and whether it is still
 * finite, as device numbers, and a recording rollout that takes them.  Neither name carries the
 * _f32 suffix.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_VITALS_FIELDS 13
#define GNCA_VITALS_BAND_ROWS 8    /* one workgroup reads a tile of 8 rows ...              */
#define GNCA_VITALS_TILE_COLS 256  /* ... by 256 columns of one sample, all C channels      */

/*
 * x: [B,C,H,W] fp32, C >= 4, channel stride H*W, sample stride x_bstride floats.  out[b*13 + f], fp64,
 * with a = channel 3 and every comparison in fp32 against alpha_thr as given:
 *    0  alive       cells with max_pool3x3(a) > alpha_thr (neighbours outside the image do not count):
 *                   the model's alive mask
 *    1  mature      cells with a > alpha_thr
 *    2  alpha_sum   sum of a
 *    3  mass        sum of clip(a, 0, 1)
 *  4,5  cy, cx      sum of clip(a,0,1) * i / mass, sum of clip(a,0,1) * j / mass; NaN when mass = 0
 * 6..9  y0,y1,x0,x1 inclusive bounding box of the mature cells; all -1 when there is none
 *   10  max_abs     largest |v| over all C channels and cells among finite v; 0 when there is none
 *   11  nonfinite   number of NaN / +-inf values over all C channels
 *   12  hidden_rms  sqrt(sum of v^2 / ((C-4) H W)) over the channels >= 4, finite v only; 0 when C = 4
 * Fields 0..9 are specified only for a finite alpha plane; 10 and 11 always.  One pass over the state.
 * Every sum is fp64 in a fixed order, without atomics: a sample's 13 numbers are bitwise the same
 * whatever B is and wherever the sample stands in the batch.  Two launches on `hip_stream` (a
 * hipStream_t, as the `stream` of the entry points above; DESIGN.md section 18 on the name), no allocation,
 * no host synchronisation, capturable.  ws: >= gnca_state_vitals_workspace_bytes(B, C, H, W) bytes of
 * device memory, 8-B aligned (else GNCA_ERR_WORKSPACE); the size is 0 on an invalid shape.  out: 8-B
 * aligned.  B, C, H, W <= 0, C < 4, a null x / out or a negative stride: GNCA_ERR_INVALID.
 */
size_t gnca_state_vitals_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int gnca_state_vitals(int32_t B, int32_t C, int32_t H, int32_t W, const float* x, int64_t x_bstride,
                      float alpha_thr, double* out, void* ws, size_t ws_bytes, void* hip_stream);

typedef struct gnca_trace_vitals {
  float alpha_thr;
  double* out;              /* DEVICE [R,B,13]: the vitals of the state after step record[r]       */
} gnca_trace_vitals;

/*
 * gnca_rollout_trace_diag that also takes the vitals: the same pieces and launches, and at each
 * record point gnca_state_vitals of the piece's output state (all C channels, read in place) goes to
 * vitals->out[r].  metrics and diag may each be NULL; args->frames may be NULL.  The frames, maps,
 * metrics, diagnostics and x_final are bitwise those of the call without vitals, and the vitals those
 * of gnca_state_vitals on the recorded states.  vitals NULL, or vitals->out NULL with num_records > 0:
 * GNCA_ERR_INVALID.
 */
size_t gnca_rollout_trace_vitals_workspace_bytes(const gnca_step_desc* desc, const gnca_trace_args* args,
                                                 const gnca_trace_metrics* metrics,
                                                 const gnca_graph_diag_out* diag);
int gnca_rollout_trace_vitals(const gnca_step_desc* desc, const gnca_weights* w, const gnca_trace_args* args,
                              const gnca_trace_metrics* metrics, const gnca_graph_diag_out* diag,
                              const gnca_trace_vitals* vitals, const float* x, float* x_final, void* ws,
                              size_t ws_bytes, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Step-adjacent batch op: damage (src/utils/damage.py:15-138).  ONE damage kind for the whole
 * batch, in place on the [B,C,H,W] state, with the random draws supplied by the caller (device
 * memory), so a whole batch is one launch with no host round trip per sample.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_DMG_SQUARE       0  /* cutout_square_:  zero all channels of [y,y+size) x [x,x+size)      */
#define GNCA_DMG_CIRCLE       1  /* cutout_circle_:  zero all channels where (i-cy)^2+(j-cx)^2 <= r^2  */
#define GNCA_DMG_STRIPE_H     2  /* stripe_wipe_ "h": zero rows [y0, y0+width) (pos[b] = (y0, 0))       */
#define GNCA_DMG_STRIPE_V     3  /* stripe_wipe_ "v": zero cols [x0, x0+width) (pos[b] = (0, x0))       */
#define GNCA_DMG_ALPHA_DROP   4  /* alpha_dropout_(hard): zero all channels where u<p and alpha>thr     */
#define GNCA_DMG_ALPHA_DROP_SOFT 5 /* alpha_dropout_(hard=False): alpha only                            */
#define GNCA_DMG_SALT_PEPPER  6  /* salt_pepper_alpha_: alpha *= (u >= p)                               */
#define GNCA_DMG_GAUSSIAN     7  /* gaussian_hole_: all channels *= clamp(1-exp(-r^2/(2(R*soft)^2)),0,1) */
#define GNCA_DMG_HIDDEN_NOISE 8  /* hidden_scramble_: hidden = clamp(hidden + sigma*n, 0, 1)          */

typedef struct gnca_damage_desc {
  int32_t B, C, H, W;
  int32_t kind;        /* GNCA_DMG_*                                                          */
  int32_t size;        /* square side, circle / gaussian radius, stripe width                  */
  float p;             /* alpha_drop / salt_pepper probability                                 */
  float alpha_thr;     /* alpha_drop: alive threshold                                          */
  float softness;      /* gaussian                                                             */
  float sigma;         /* hidden noise scale                                                   */
} gnca_damage_desc;

/*
 * pos:   int32 [B,2] per-sample (y, x) / centre (cy, cx) for the geometric kinds, else NULL
 * noise: fp32 uniforms [B,1,H,W] (alpha kinds) or normals [B,C-4,H,W] (hidden noise), else NULL
 */
int gnca_damage_f32(const gnca_damage_desc* desc, float* state, const int32_t* pos,
                    const float* noise, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The damage POLICY on the device (src/utils/damage.py:99-138): whether to damage, which kind, its
 * size, orientation, positions and per-cell noise are all drawn INSIDE one launch from a counter
 * RNG, so the call needs no host draw, no noise tensor and no host wait, and a kind per sample is
 * possible.  In place on the [B,C,H,W] state.  Per cell the arithmetic of every kind is that of
 * gnca_damage_f32 (same expressions, same order).
 *
 * RNG (the definition; every value is an integer, so a restatement in any language is bitwise).
 * With mix64(z) = { z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB;
 * return z ^ z>>31; } in uint64 arithmetic:
 *   k0 = mix64(seed + 0xD6E8FEB86659FD93)          (a domain constant of its own: `seed` may be the
 *   k1 = mix64(k0 + 0x9E3779B97F4A7C15 * (uint64)(event + 1))        fire hash's rng_seed)
 *   k2 = mix64(k1 ^ (sample << 8 | stream))
 *   d(seed, event, sample, stream, index) = mix64(k2 + index) >> 40            in [0, 2^24)
 * `sample` is the GLOBAL sample index sample_base + b, or GNCA_DMG_SHARED_SAMPLE for a draw the whole
 * batch (every rank of a sharded batch) shares; `stream` is a GNCA_DMG_RNG_* id; `index` is 0 for a
 * scalar draw, the cell index i * W + j for a cell uniform and (c - 4) * H * W + i * W + j for the
 * normal of hidden channel c.
 *   uniform            u = d * 2^-24 (exact in fp32)
 *   integer in [lo,hi] lo + ((d * (hi - lo + 1)) >> 24), in 64-bit integers
 *   gate               pass iff u <= prob
 *   kind               kinds[k] of the smallest k < n_kinds with u < cum[k] (k = n_kinds - 1 if none)
 *   orientation        horizontal iff d < 2^23
 *   normal             sqrtf(-2 * logf((d1 + 1) * 2^-24)) * cosf(2 pi * (d2 * 2^-24)), d1 / d2 from the
 *                      streams NORMAL_U1 / NORMAL_U2 at the same index (fp32, library logf/sqrtf/cosf)
 *
 * What is drawn.  size = integer in [size_min, size_max] (stream SIZE).  Then by kind:
 *   SQUARE        side = size; origin y in [0, max(1, H-side+1)), x in [0, max(1, W-side+1))
 *   CIRCLE        r = size > 1 ? size / 2 : 1; centre y in [r, max(r+1, H-r)), x in [r, max(r+1, W-r))
 *   GAUSSIAN      r as the circle's, centre as the circle's
 *   STRIPE_H / _V width = stripe_width > 0 ? stripe_width : size; origin y in [0, max(1, H-width+1))
 *                 (x = 0), or x in [0, max(1, W-width+1)) (y = 0)
 *   STRIPES_AUTO  the orientation is drawn (stream ORIENT), then as STRIPE_H / STRIPE_V
 *   ALPHA_DROP, ALPHA_DROP_SOFT (p = alpha_dropout_p), SALT_PEPPER (p = salt_pepper_p): a uniform per cell
 *   HIDDEN_NOISE  a normal per hidden channel and cell, scaled by hidden_sigma
 * y comes from stream Y and x from stream X.  A sample is left untouched (the reference's early
 * returns) for a side or width <= 0, p <= 0, hidden_sigma <= 0 and hidden noise at C <= 4.
 *
 * scope GNCA_DMG_SCOPE_BATCH (the reference's structure): the gate (stream GATE, u <= prob), the kind,
 * the size, the stripe orientation and the stripe origin are drawn once, with sample =
 * GNCA_DMG_SHARED_SAMPLE; the positions of square / circle / gaussian per global sample; the cell noise
 * per (global sample, cell).  per_sample_prob is not read.
 * scope GNCA_DMG_SCOPE_SAMPLE: the batch gate as above, then per global sample a gate (stream
 * SAMPLE_GATE, u <= per_sample_prob) and every other draw.
 * Either way a batch of B samples at sample_base s is bitwise rows [s, s+B) of a larger batch.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_DMG_STRIPES_AUTO 9  /* stripe_wipe_ "auto" (the policy's "stripes"): orientation drawn */
#define GNCA_DMG_MAX_KINDS   10

#define GNCA_DMG_SCOPE_BATCH  0
#define GNCA_DMG_SCOPE_SAMPLE 1

#define GNCA_DMG_SHARED_SAMPLE 0xFFFFFFFFull

#define GNCA_DMG_RNG_GATE        0
#define GNCA_DMG_RNG_SAMPLE_GATE 1
#define GNCA_DMG_RNG_KIND        2
#define GNCA_DMG_RNG_SIZE        3
#define GNCA_DMG_RNG_ORIENT      4
#define GNCA_DMG_RNG_Y           5
#define GNCA_DMG_RNG_X           6
#define GNCA_DMG_RNG_CELL        7
#define GNCA_DMG_RNG_NORMAL_U1   8
#define GNCA_DMG_RNG_NORMAL_U2   9

typedef struct gnca_damage_policy_desc {
  int32_t B, C, H, W;
  int32_t scope;               /* GNCA_DMG_SCOPE_*                                              */
  float prob;                  /* the batch gate                                                */
  float per_sample_prob;       /* the per-sample gate (GNCA_DMG_SCOPE_SAMPLE)                    */
  int32_t n_kinds;             /* 1..GNCA_DMG_MAX_KINDS                                         */
  int32_t kinds[GNCA_DMG_MAX_KINDS];   /* GNCA_DMG_* codes 0..9                                 */
  float cum[GNCA_DMG_MAX_KINDS];       /* fp32 of the running weight sums / their total (fp64 on the
                                          host); the last one 1.0                               */
  int32_t size_min, size_max;
  int32_t stripe_width;        /* <= 0: the drawn size                                          */
  float alpha_thr, alpha_dropout_p, salt_pepper_p, hidden_sigma, gaussian_softness;
  uint64_t seed;
  int64_t event;               /* the draw counter: one value per policy call                   */
  int64_t sample_base;         /* global index of sample 0 (sharded batches)                    */
  void* stream;                /* hipStream_t; NULL = the default stream                        */
} gnca_damage_policy_desc;

/*
 * One launch, stream-ordered on desc->stream; no allocation, no copy, no synchronisation (it can be
 * captured into a graph).  The stream travels in the descriptor.
 * forced_kind: int32 [B] device or NULL.  forced_kind[b] in 0..9 replaces the gates and the kind draw
 *              of sample b (the other draws stay as above); any other value leaves sample b untouched.
 * event_dev:   one int64 on the device or NULL; when given it replaces desc->event and is read by the
 *              kernel, so a captured loop that increments it draws afresh on every replay.
 * draws_out:   int32 [B,8] device or NULL: {applied, primitive kind, size argument, y, x, 0, 0, 0} per
 *              sample, where (primitive kind 0..8, size argument, (y, x)) are gnca_damage_f32's kind,
 *              size and pos[b] for the same effect; an untouched sample gets {0, -1, 0, 0, 0, 0, 0, 0}.
 * noise_out:   fp32 [B, max(1, C-4), H, W] device or NULL: the uniforms in plane 0 of a sample with an
 *              alpha kind, the normals in all C-4 planes of a hidden-noise sample (gnca_damage_f32's
 *              `noise`); every other element is NOT written.
 * GNCA_ERR_INVALID: null desc / state, B < 0, C < 4, H or W <= 0, a scope or kind code out of range,
 * n_kinds outside 1..GNCA_DMG_MAX_KINDS, size_max < size_min.  B == 0 is GNCA_OK (nothing to do).
 */
int gnca_damage_policy(const gnca_damage_policy_desc* desc, float* state, const int32_t* forced_kind,
                       const int64_t* event_dev, int32_t* draws_out, float* noise_out);

/*
 * The graph trainer's loss (src/training/train_graph_augmented_nca.py:52-61), fused:
 *   per_sample[b] = mean_{c<4,i,j} (rgba(pred)[b,c,i,j] - target[b,c,i,j])^2,
 *   rgba(pred) = (pred_rgb * pred_alpha, pred_alpha),
 * and its backward grad_pred[b,c,i,j] = g[b] * d per_sample[b] / d pred[b,c,i,j] (channels 0..3).
 * pred / grad_pred are [B,4,H,W] with sample stride `pred_bstride` floats and channel stride H*W
 * (a channel slice of a contiguous [B,C,H,W] state: pred_bstride = C*H*W); target has sample
 * stride `target_bstride` (0 = one target broadcast over the batch).  fp64 per-sample sums.
 */
int gnca_loss_premult_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pred_bstride,
                          const float* target, int64_t target_bstride, float* per_sample, void* stream);
int gnca_loss_premult_bwd_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pred_bstride,
                              const float* target, int64_t target_bstride, const float* g,
                              float* grad_pred, int64_t grad_bstride, void* stream);

/*
 * The classic trainer's objective (src/training/train_intermediate_loss.py:37-51, with the two
 * background penalties of src/training/train_graph_augmented_nca.py:30-49), fused.  Layouts are
 * those of gnca_loss_premult_f32, but pred is the RAW slice state[:, :4]: nothing is premultiplied.
 *   alive(b,i,j)  = target[b,3,i,j] > alpha_thr            (fp32, strict), dead = 1 - alive
 *   n_b           = number of alive cells of sample b      (written to alive_count[b])
 *   per_sample[b] = sum_{c<4,i,j} alive (pred - target)^2 / (n_b + 1e-8)
 *                 + lam_bg_alpha sum pred_a dead / HW
 *                 + lam_bg_rgb   sum_{c<3} |pred_c dead| / (3 HW)
 *                 + lam_area     sum pred_a / HW
 * One workgroup per sample; fixed-order fp64 sums, so a sample's value is bitwise the same alone,
 * in a batch and at any batch position.  With nsteps_out set, the stability phase's schedule is
 * written too: nsteps_out[b] = per_sample[b] < close_thresh ? close_steps : 0, compared on the stored
 * fp32 value (close_steps < 0 is GNCA_ERR_INVALID).  The backward writes all four channels of
 * grad_pred = g[b] * d per_sample[b] / d pred, with sign(0) = 0 in the |.| term.
 */
typedef struct gnca_masked_loss_desc {
  int32_t B, H, W;
  float alpha_thr;      /* alive(b,i,j) = target[b,3,i,j] > alpha_thr, compared in fp32, strict */
  float lam_area;       /* * mean_{i,j} pred_a                                                   */
  float lam_bg_alpha;   /* * mean_{i,j} pred_a * dead                 (dead = 1 - alive)         */
  float lam_bg_rgb;     /* * mean_{c<3,i,j} |pred_c * dead|                                      */
  float close_thresh;   /* read only when nsteps_out != NULL                                     */
  int32_t close_steps;  /* K                                                                     */
} gnca_masked_loss_desc;

int gnca_loss_masked_f32(const gnca_masked_loss_desc* d, const float* pred, int64_t pred_bstride,
                         const float* target, int64_t target_bstride, float* per_sample /*[B]*/,
                         int32_t* alive_count /*[B], out*/, int32_t* nsteps_out /*[B] or NULL*/,
                         void* stream);
int gnca_loss_masked_bwd_f32(const gnca_masked_loss_desc* d, const float* pred, int64_t pred_bstride,
                             const float* target, int64_t target_bstride,
                             const int32_t* alive_count, const float* g /*[B]*/,
                             float* grad_pred, int64_t grad_bstride, void* stream);

/*
 * The stability phase's loss (src/training/train_intermediate_loss.py:256-267), without the host
 * wait on close.any():
 *   loss = scale * sum_{b: close[b] != 0} sum_{c<4,i,j} (pred - target)^2,
 *   scale = 1 / (n_close 4 HW); no close sample: scale = 0 and loss = 0 (the reference skips the term).
 * Samples that are not close are not read.  ws: >= gnca_loss_stability_workspace_bytes(B) bytes of
 * device memory, 8-B aligned (else GNCA_ERR_WORKSPACE; the size is 0 on B <= 0).  Forward: per-sample
 * fp64 partials, then a one-workgroup fixed-order finish that also writes `scale` for the backward:
 *   grad_pred = g[0] * scale * 2 (pred - target) on close samples, 0 on the others.
 */
size_t gnca_loss_stability_workspace_bytes(int32_t B);
int gnca_loss_stability_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pred_bstride,
                            const float* target, int64_t target_bstride, const uint8_t* close /*[B]*/,
                            float* loss /*[1]*/, float* scale /*[1], out*/, void* ws, size_t ws_bytes,
                            void* stream);
int gnca_loss_stability_bwd_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pred_bstride,
                                const float* target, int64_t target_bstride, const uint8_t* close,
                                const float* scale, const float* g /*[1]*/, float* grad_pred,
                                int64_t grad_bstride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses at intermediate steps of one rollout ("taps"), read from the tape in place, and the BPTT
 * that adds their gradients to the running cotangent between two steps.  Neither name carries the
 * _f32 suffix and the stream travels in the descriptor, as in gnca_render_u8.
 *
 * Tap r is the state after step steps[r] (1..T): tape slot steps[r] of the rollout that wrote
 * `tape`, or x_final (contiguous [B,C,H,W]) for steps[r] == T, which is not on the tape.
 *   losses[r][b] = gnca_loss_premult_f32 / gnca_loss_masked_f32 of channels 0..3 of that state,
 *                  bitwise (one 256-thread workgroup per (tap, sample), the same fixed-order sums).
 *   alive_count  : GNCA_TAP_MASKED only, written once (it depends on the target alone).
 * The tap list is a HOST array; it reaches the device in kernel arguments, GNCA_TAP_CHUNK taps per
 * launch, so the calls work under stream capture and R has no cap.
 *
 * gnca_rollout_bwd_taps is gnca_rollout_bwd_f32 with
 *   dL/dS_t[b, c<4] += g_losses[r][b] * d losses[r][b] / d S_t        at t = steps[r],
 * each term the fp32 value of gnca_loss_premult_bwd_f32 / gnca_loss_masked_bwd_f32 and one rounded
 * add (never contracted), applied after step t's backward and before step t-1's.  gy == NULL stands
 * for a zero cotangent of x_final: the steps after the last tap are not run.  g_losses == NULL is
 * gnca_rollout_bwd_f32.  gy is never written.  ws: gnca_rollout_bwd_workspace_bytes.
 * GNCA_ERR_INVALID before any launch: a null taps / steps / target, n < 1, steps not strictly
 * increasing or outside 1..sched->steps, an unknown kind, masked.B/H/W != desc's (either kind),
 * a missing alive_count (GNCA_TAP_MASKED), gy and g_losses both NULL, gx aliasing gy.
 *
 * Under GNCA_SCHED_CHECKPOINT most tapped states are not on the tape: gnca_rollout_tap_loss then
 * returns GNCA_ERR_INVALID before any launch, and gnca_rollout_fwd_taps takes its place.  It is
 * gnca_rollout_fwd_f32 (on taps->stream) that also writes losses[r][b] right after step steps[r]
 * wrote its state, wherever that state lives: one launch of the same loss kernel per tap, given the
 * state's address.  Valid for every schedule, with or without the flag, and with tape == NULL (the
 * no-grad form); x_final and the losses are bitwise those of gnca_rollout_fwd_f32 followed by
 * gnca_rollout_tap_loss.  It rejects what gnca_rollout_tap_loss rejects (a null or malformed tap
 * list, a null losses, a missing alive_count).  gnca_rollout_bwd_taps under the flag injects a
 * tap's gradient where it does without it, reading S_t from the segment area or the anchor; with
 * gy == NULL the segments that lie wholly after the last tap are neither re-run nor walked.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_TAP_PREMULT 0
#define GNCA_TAP_MASKED 1
#define GNCA_TAP_CHUNK 32   /* taps per launch of the loss kernel */

typedef struct gnca_rollout_taps {
  int32_t n;                     /* R >= 1                                                       */
  const int32_t* steps;          /* HOST [R], strictly increasing, in 1..sched->steps            */
  int32_t kind;                  /* GNCA_TAP_*                                                   */
  gnca_masked_loss_desc masked;  /* knobs of GNCA_TAP_MASKED; B, H, W must equal the desc's      */
  const float* target;           /* DEVICE, [B or 1][4][H][W]                                    */
  int64_t target_bstride;        /* as gnca_loss_premult_f32 (0 = one target for the batch)      */
  void* stream;
} gnca_rollout_taps;

int gnca_rollout_tap_loss(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                          const gnca_rollout_taps* taps, const void* tape, size_t tape_bytes,
                          const float* x_final, float* losses /*[R][B]*/,
                          int32_t* alive_count /*[B], GNCA_TAP_MASKED only*/);
int gnca_rollout_fwd_taps(const gnca_step_desc* desc, const gnca_weights* w,
                          const gnca_rollout_sched* sched, const gnca_rollout_taps* taps,
                          const float* x, float* x_final, void* tape /*or NULL*/, size_t tape_bytes,
                          float* losses /*[R][B]*/, int32_t* alive_count /*[B], GNCA_TAP_MASKED only*/,
                          void* ws /*gnca_rollout_fwd_workspace_bytes*/, size_t ws_bytes);
int gnca_rollout_bwd_taps(const gnca_step_desc* desc, const gnca_weights* w,
                          const gnca_rollout_sched* sched, const gnca_rollout_taps* taps,
                          const void* tape, size_t tape_bytes, const float* x_final,
                          const float* gy /*or NULL = zeros*/, const float* g_losses /*[R][B] or NULL*/,
                          const int32_t* alive_count, float* gx, const gnca_grads* grads, void* ws,
                          size_t ws_bytes);

/* ---------------------------------------------------------------------------------------------
 * The iteration's tail: gradient policy + Adam in one call, and the pool write-back in one call.
 * Neither name carries the _f32 suffix of the entry points above.
 * -------------------------------------------------------------------------------------------*/

/*
 * gnca_optim_step: the trainers' gradient policy followed by torch.optim.Adam's update (no amsgrad,
 * L2 weight decay), for up to GNCA_OPTIM_MAX_TENSORS tensors per call
 * (src/training/train_graph_augmented_nca.py:367-375, src/training/train_intermediate_loss.py:280-283).
 * Per tensor, in fp32 and in torch's order of operations:
 *   NORMALIZE  g <- g / (||g||_2 + norm_eps)                       (the tensor's own norm)
 *   CLIP       g <- g * min(max_norm / (total + 1e-6), 1),  total = 2-norm over ALL tensors
 *   g <- g + weight_decay p
 *   m <- m + (1 - beta1)(g - m)          v <- beta2 v + (1 - beta2) g g
 *   p <- p - (lr / bias1) m / (sqrt(v) / sqrt(bias2) + eps)
 * with bias1 = 1 - beta1^t and bias2 = 1 - beta2^t computed by the caller from the tensor's own step
 * count t.  g is read, never written.  The sums of squares are fp64, in a fixed order that depends on
 * the element count alone (not on the pointer's alignment): bitwise reproducible, no atomics.
 *
 * sumsq == NULL: one launch.  Every workgroup recomputes the sums it needs (NORMALIZE: its tensor's,
 * CLIP: every tensor's of this call, which must then be all of them).  Allowed while the call's
 * tensors hold at most GNCA_OPTIM_ONE_LAUNCH_MAX elements together (else GNCA_ERR_WORKSPACE).
 * sumsq != NULL: device memory, fp64 [sumsq_count], 8-B aligned; tensor i of this call owns
 * sumsq[sumsq_base + i].  GNCA_OPTIM_SUMSQ writes those (one launch, one workgroup per tensor),
 * GNCA_OPTIM_UPDATE then updates from them (one launch; CLIP adds sumsq[0 .. sumsq_count) in index
 * order, so several calls' tensors can share one total).  flags = 0 means both, in that order.
 * POLICY_NONE is always one launch and ignores sumsq.  The whole descriptor travels as the kernel
 * argument: nothing is copied to the device and no table lives in device memory.
 */
#define GNCA_OPTIM_MAX_TENSORS 24
#define GNCA_OPTIM_ONE_LAUNCH_MAX 65536   /* elements; 256 KB of gradient re-read from L2 per workgroup */
#define GNCA_OPTIM_POLICY_NONE      0
#define GNCA_OPTIM_POLICY_NORMALIZE 1
#define GNCA_OPTIM_POLICY_CLIP      2
#define GNCA_OPTIM_SUMSQ  (1u << 0)
#define GNCA_OPTIM_UPDATE (1u << 1)

typedef struct gnca_optim_tensor {
  float* p;             /* DEVICE, contiguous fp32 [numel]: the parameter, updated in place          */
  const float* g;       /* its gradient (read only)                                                  */
  float* m;             /* exp_avg                                                                   */
  float* v;             /* exp_avg_sq                                                                */
  int64_t numel;
  double lr;
  double weight_decay;
  double bias1;         /* 1 - beta1^t                                                               */
  double bias2;         /* 1 - beta2^t                                                               */
} gnca_optim_tensor;

typedef struct gnca_optim_desc {
  int32_t policy;       /* GNCA_OPTIM_POLICY_*                                                       */
  int32_t num_tensors;  /* 0 .. GNCA_OPTIM_MAX_TENSORS (0: nothing is launched)                      */
  uint32_t flags;       /* GNCA_OPTIM_SUMSQ / GNCA_OPTIM_UPDATE with sumsq; 0 = both                  */
  int32_t sumsq_base;
  int32_t sumsq_count;
  int32_t reserved;     /* 0                                                                         */
  double* sumsq;        /* DEVICE fp64 [sumsq_count] or NULL                                         */
  double beta1, beta2, eps;
  double max_norm;      /* CLIP                                                                      */
  double norm_eps;      /* NORMALIZE (the trainers' 1e-8)                                            */
  gnca_optim_tensor t[GNCA_OPTIM_MAX_TENSORS];
} gnca_optim_desc;

int gnca_optim_step(const gnca_optim_desc* desc, void* stream);

/*
 * gnca_pool_commit: the trainers' pool write-back with worst-k reset and random reseed
 * (src/training/train_graph_augmented_nca.py:377-391, src/training/train_intermediate_loss.py:269-296)
 * in one launch, with no clone of the batch and no host wait.  For every b < B it writes the
 * sample_elems floats of pool slot slots[b] (slots: distinct, each in 0 .. pool_slots-1; a slot
 * outside that range is skipped) from
 *   seed1                   where rand_idx != NULL and *rand_idx == b (applied last: it wins),
 *   seeds + r sample_elems  where r < n_reset, r = sample b's rank by descending per_sample,
 *   state + b sample_elems  otherwise.
 * Rank 0 is the worst (largest) loss, as torch.topk orders; a NaN ranks above every number; equal
 * losses (and NaNs among themselves) rank by lower b first.  Only the B addressed slots are
 * written.  per_sample [B] and seeds [n_reset, sample_elems] may be NULL when n_reset == 0; seed1
 * [sample_elems] and rand_idx (one int64 on the device) may be NULL together (no reseed).
 */
typedef struct gnca_pool_commit_desc {
  int64_t pool_slots;    /* P                                                                        */
  int64_t sample_elems;  /* C*H*W                                                                    */
  int32_t B;
  int32_t n_reset;       /* 0 .. B                                                                   */
} gnca_pool_commit_desc;

int gnca_pool_commit(const gnca_pool_commit_desc* desc, float* pool, const int64_t* slots,
                     const float* state, const float* per_sample, const float* seeds, const float* seed1,
                     const int64_t* rand_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frames and maps as uint8 images: the pixel work in front of a PNG / video
 * encoder, masked_rgb and attn_to_rgb of src/testing/test_graph_augmented_regeneration.py:29-47 and
 * save_img of src/testing/test_intermediate_loss.py:18-37, without the host round trip.
 *
 * The stream of these two entry points travels in the descriptor, not as a trailing parameter: the
 * stream gate of the test suite enumerates the declarations that have that parameter against a fixed
 * case table, and these two are run on the same three legs (eager, side stream with delayed inputs,
 * capture and replay) by tests/test_gpu_render.py instead.  Everything else in the conventions above
 * holds: stream-ordered on d->stream, no allocation, no host<->device copy, no synchronisation,
 * capturable, every byte of `out` written, no workspace.
 * -------------------------------------------------------------------------------------------*/

/*
 * One frame per image, all arithmetic in fp32.  With m = (alpha > alpha_thr), strict, on fp32
 * (alpha is channel 3):
 *   GNCA_RENDER_RGB   3 bytes per pixel: v_c = clip(rgb_c * m, 0, 1) per source cell (masked_rgb)
 *   GNCA_RENDER_RGBA  4 bytes per pixel: v_c = rgb_c * m, v_a = m                     (save_img)
 * then bilinear resampling by the integer factor s = upscale with half-pixel centres
 * (F.interpolate(mode="bilinear", align_corners=False)): per axis, for output index q s + p,
 *   f = (p + 0.5) / s - 0.5,  src = max(q + f, 0),  i0 = floor(src),  i1 = min(i0 + 1, n - 1),
 *   l1 = src - i0,  l0 = 1 - l1,  value = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11),
 * then clip(., 0, 1) (always, also at s = 1, where the resampling is the identity), and
 * byte = (uint8) trunc(value * 255): truncation, as numpy's astype(np.uint8).  For s in {1,2,4,8,16}
 * the weights are exact; inputs are assumed finite (a NaN gives an unspecified byte, inside `out`).
 * One workgroup renders GNCA_RENDER_BAND_ROWS source rows of one image (fewer when the band and its
 * two halo rows would not fit the LDS; GNCA_ERR_UNSUPPORTED when three rows of the image do not).
 */
#define GNCA_RENDER_RGB  0
#define GNCA_RENDER_RGBA 1
#define GNCA_RENDER_BAND_ROWS 8
typedef struct gnca_render_desc {
  int32_t N, H, W;        /* images; source height / width                                  */
  int32_t upscale;        /* 1 .. 16                                                         */
  int32_t mode;           /* GNCA_RENDER_*                                                   */
  float   alpha_thr;
  int64_t src_nstride;    /* floats between images; channels are H*W apart, rows contiguous  */
  void*   stream;         /* hipStream_t, NULL = the null stream                             */
} gnca_render_desc;
int gnca_render_u8(const gnca_render_desc* d, const float* src, uint8_t* out);
      /* out: [N, H*s, W*s, 3|4] contiguous, 4-byte aligned */

/*
 * One colour image per map; every one of the N maps normalises on its own:
 *   GNCA_NORM_MAX     vmax = max(a); z = vmax > 0 ? clip(a / (vmax + 1e-8f), 0, 1) : 0  (attn_to_rgb)
 *   GNCA_NORM_MINMAX  z = max > min ? (a - min) / (max - min) : 0
 *   out = lut[min((int)(z * 256), 255)], three bytes.
 * The division is IEEE-correct (the index is bitwise numpy's).  lut: DEVICE uint8 [256,3].  One
 * workgroup per map: max / min by wavefront shuffles and LDS (order-independent), then the bytes.
 */
#define GNCA_NORM_MAX    0
#define GNCA_NORM_MINMAX 1
typedef struct gnca_colorize_desc { int32_t N, H, W, norm; void* stream; } gnca_colorize_desc;
int gnca_colorize_u8(const gnca_colorize_desc* d, const float* maps, const uint8_t* lut, uint8_t* out);
      /* maps [N,H,W] contiguous; out [N,H,W,3] contiguous, 4-byte aligned */

/* ---------------------------------------------------------------------------------------------
 * Forward-mode tangent (Jacobian-vector product) of the step and of a scheduled rollout (DESIGN.md
 * section 21): where a nudge v of the state is after T steps, carried forward beside the state with
 * no tape, O(1) memory in T.  Neither name carries the _f32 suffix, and the stream is named
 * hip_stream or travels in the args struct.
 *
 * The conventions are the backward's (gnca_step_bwd_f32): the pre- and post-update alive masks, the
 * sender mask and the fire mask are constants, the perception bank is frozen, and in torus mode the
 * offset weights are the constant 1/k.  With hpre, m (the message before tanh, after the hidden-only
 * zeroing), xhat, rstd and t = tanh(xn) the primal step's own intermediates at x, one step x -> x'
 * carries v -> v':
 *   y'  = perceive(v)
 *   h'  = [hpre > 0] (W1 y')                                                        (no bias)
 *   u'  = W2 h' + message_gain (1 - tanh^2(m)) hidden_only(sum_o w_o shift_o(A_send (Wm v)))
 *   u'  = u' fire A_pre
 *   xn' = gamma rstd (u' - mean(u') - xhat mean(xhat u'))    (per-sample means over C*H*W; without
 *                                                             GroupNorm xn' = u')
 *   v'  = v + update_gain (1 - t^2) xn';   v'[:, 3] *= post_alive(x')
 * A sample that a masked or nsteps step leaves alone passes v through unchanged, as it does x.
 *
 * The one gap: the zero-padded shift (GNCA_ZERO_PAD_SHIFT on a graph step with offsets), whose offset
 * weights depend on x, is GNCA_ERR_UNSUPPORTED (workspace size 0).
 * Fixed-order fp64 sums, no float atomics: bitwise reproducible, and a sample's results do not
 * depend on the other samples.  One stream, no allocation, no host synchronisation, capturable.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_TANGENT_RENORM (1u << 0)  /* renormalise v' of each sample at every recorded step */

typedef struct gnca_tangent_args {
  int32_t num_records;     /* R >= 0                                                           */
  const int32_t* record;   /* HOST [R], strictly increasing, in 1..sched->steps                */
  uint32_t flags;          /* GNCA_TANGENT_RENORM                                              */
  double* log_norm;        /* DEVICE [R][B] or NULL when R = 0                                 */
  void* stream;            /* hipStream_t, NULL = the null stream                              */
} gnca_tangent_args;

/* Bytes of device workspace gnca_step_tangent needs for `desc` (0 on an invalid or unsupported desc).
 * Host-only. */
size_t gnca_step_tangent_workspace_bytes(const gnca_step_desc* desc);

/*
 * One step and its tangent: x_out = step(x), bitwise gnca_step_f32's (gnca_step_masked_f32's with
 * `active`), and v_out = J(x) v.  fire / active as in those two entry points (active may be NULL).
 * x and v are read; x_out and v_out are written completely and must alias neither each other nor x
 * or v (GNCA_ERR_INVALID, as for a null pointer, before any launch).  ws: 256-B aligned.
 */
int gnca_step_tangent(const gnca_step_desc* desc, const gnca_weights* w, const float* x, const void* fire,
                      const uint8_t* active, const float* v, float* x_out, float* v_out, void* ws,
                      size_t ws_bytes, void* hip_stream);

/* Bytes of device workspace gnca_rollout_tangent needs (0 on an invalid or unsupported desc, schedule
 * or record list).  Host-only: reads the schedule's and the args' host arrays.  Apart from the [T][B]
 * step masks it does not grow with T. */
size_t gnca_rollout_tangent_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                            const gnca_tangent_args* args);

/*
 * The tangent of a whole rollout on the schedule gnca_rollout_fwd_f32 reads (offsets, per-step
 * fire_rate / message_gain, nsteps, full_steps, fire); GNCA_SCHED_RECOMPUTE and GNCA_SCHED_CHECKPOINT
 * are GNCA_ERR_INVALID (there is no tape).  x_final is bitwise gnca_rollout_fwd_f32's without a tape,
 * v_final the chain of gnca_step_tangent calls.  GNCA_ERR_INVALID before any launch for a null
 * pointer, aliasing between x / v and the outputs, or a malformed record list.
 *   log_norm[r][b]  the natural log of the 2-norm the tangent of sample b would have after step
 *                   record[r] had it never been renormalised: 0.5 log(sum v'^2) (fp64, fixed order)
 *                   plus the sample's carried log of earlier renormalisations; -inf for a zero tangent
 *   GNCA_TANGENT_RENORM  after the norm is recorded, v' of that sample is multiplied by
 *                   (float)(1 / sqrt(sum v'^2)) when the sum is positive and finite, and left alone
 *                   otherwise.  The host never waits.
 */
int gnca_rollout_tangent(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                         const gnca_tangent_args* args, const float* x, const float* v, float* x_final,
                         float* v_final, void* ws, size_t ws_bytes);

/* ---------------------------------------------------------------------------------------------
 * A block of K tangents, re-orthonormalised on the device (Benettin's method):
 * the thin QR of a tangent block, and the rollout that carries K directions beside one primal state.
 * The block is direction-major: v [K][B][n] fp32, n = C*H*W, so direction j is the contiguous
 * [B,C,H,W] tensor at v + j*B*n that gnca_step_tangent accepts.
 *
 * gnca_tangent_qr factors, per sample b independently, V_b = [v_1 .. v_K] (n x K) = Q_b R_b with R_b
 * upper triangular and a non-negative diagonal, by Cholesky of the fp64 Gram matrix G = V^T V (a
 * product of two fp32 values is exact in fp64; fixed-order sums, no float atomics):
 *   for j = 0..K-1:  d_j = G_jj - sum_{i<j} R_ij^2                                  (i ascending)
 *     d_j positive, finite and > 2^-44 G_jj:  R_jj = sqrt(d_j),
 *                                             R_jk = (G_jk - sum_{i<j} R_ij R_ik) / R_jj  for k > j
 *     otherwise column j is DROPPED: row j of R is zero, log R_jj = -inf, Q_j is all zeros and the
 *     column contributes nothing to later columns (its entries R_ij, i < j, stay as computed).
 *   Q_j(e) = sum_{i<=j} V_i(e) Rinv_ij   in fp64, i ascending, dropped i skipped, rounded to fp32 once,
 *   with Rinv the inverse of R on the kept rows and columns and zero elsewhere.
 * 2^-44: fp32 inputs carry a relative rounding of 2^-24, so a column in the span of the earlier ones
 * up to that rounding leaves a residual near 2^-48 G_jj; the threshold is 16 times that.  A non-finite
 * Gram entry drops its column by the same rule.  K > n is served: the surplus columns drop.
 *   v         [K][B][n], overwritten by Q
 *   r         [B][K][K] fp64 row-major, zeros below the diagonal, or NULL
 *   log_diag  [B][K] fp64, log R_jj, or NULL
 * The workspace begins with the Gram partials, fp64 [B][nchunk][K(K+1)/2], nchunk =
 * ceil(n / GNCA_TANGENT_QR_CHUNK), entry (i <= j) at j(j+1)/2 + i; their sum over the chunks, in
 * chunk order, is G.  GNCA_ERR_INVALID before any launch for K outside 1..GNCA_TANGENT_MAX_DIRS,
 * B < 1, n < 1 or a null v; bitwise reproducible, a sample's results do not depend on the others.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_TANGENT_MAX_DIRS 16
#define GNCA_TANGENT_QR_CHUNK 4096     /* elements of one sample per Gram workgroup */
#define GNCA_TBLOCK_ORTHO (1u << 0)    /* replace the block by Q at every recorded step */

typedef struct gnca_tangent_block_args {
  int32_t num_dirs;        /* K, 1..GNCA_TANGENT_MAX_DIRS                                      */
  int32_t num_records;     /* R >= 0                                                           */
  const int32_t* record;   /* HOST [R], strictly increasing, in 1..sched->steps                */
  uint32_t flags;          /* GNCA_TBLOCK_ORTHO                                                */
  double* log_r;           /* DEVICE [R][B][K] or NULL when R = 0                              */
  void* stream;            /* hipStream_t, NULL = the null stream                              */
} gnca_tangent_block_args;

/* Bytes of device workspace gnca_tangent_qr needs (0 on invalid sizes).  Host-only. */
size_t gnca_tangent_qr_workspace_bytes(int32_t num_dirs, int32_t B, int64_t n);

int gnca_tangent_qr(int32_t num_dirs, int32_t B, int64_t n, float* v, double* r, double* log_diag, void* ws,
                    size_t ws_bytes, void* hip_stream);

/* Bytes of device workspace gnca_rollout_tangent_block needs (0 on an invalid or unsupported desc,
 * schedule or args).  Host-only.  [T][B] masks, one step workspace, two states, 2K tangents, the Gram
 * partials, Rinv and the carry: apart from the masks it does not grow with T, and it is linear in K. */
size_t gnca_rollout_tangent_block_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                                  const gnca_tangent_block_args* args);

/*
 * gnca_rollout_tangent for K directions v [K][B][C][H][W] beside ONE primal state: per step the primal
 * step and the mask / GroupNorm preparation run once, the two tangent kernels once per direction.
 * Schedule, fire modes, nsteps / full_steps and support set are gnca_rollout_tangent's, and so are its
 * refusals (GNCA_SCHED_RECOMPUTE / GNCA_SCHED_CHECKPOINT: GNCA_ERR_INVALID; the zero-padded shift:
 * GNCA_ERR_UNSUPPORTED, workspace size 0), all before any launch.  x_final is bitwise
 * gnca_rollout_fwd_f32's.
 *   without GNCA_TBLOCK_ORTHO  nothing is rescaled: v_final[j] is bitwise gnca_rollout_tangent's v_final
 *       on v[j], and log_r[r][b][j] bitwise its log_norm[r][b].
 *   with GNCA_TBLOCK_ORTHO     at every recorded step the block is replaced by gnca_tangent_qr's Q
 *       (the same kernels), log_r[r][b][j] = log R_jj + carry[b][j] and then carry[b][j] += log R_jj,
 *       in fp64 and in record order.  A dropped column records -inf, leaves its carry alone and stays
 *       zero from then on.  log_r[R-1] / record[R-1] is the finite-time Lyapunov spectrum.
 * A sample that nsteps has finished passes its block through; later records re-factor an already
 * orthonormal block, so their R is I and the logs are 0 within rounding.  There is no special case.
 */
int gnca_rollout_tangent_block(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                               const gnca_tangent_block_args* args, const float* x, const float* v,
                               float* x_final, float* v_final, void* ws, size_t ws_bytes);

/* ---------------------------------------------------------------------------------------------
 * Weight-direction tangents: the three tangent entry points above with a
 * direction dtheta of the WEIGHTS carried beside the state tangent v, so that v_out / v_final is
 * J_x v + J_theta dtheta: where a nudge of the weights is after the step / the rollout, with no tape.
 * The conventions are the state tangent's (masks constant, perception bank frozen, torus offset
 * weights the constant 1/k, so that the query, key and scaling directions have exactly zero effect).
 * With y = perceive(x), h = relu(hpre), s_z = 1/k sum_o shift_o(A_send z), cnt = live senders / k:
 *   h'  = [hpre > 0] (W1 perceive(v) + dW1 y + db1)
 *   u'  = (W2 h' + dW2 h
 *          + message_gain (1 - tanh^2(m)) hidden_only(Wm s_v + dWm s_x + dbm cnt)) fire A_pre
 *   xn' = gamma rstd (u' - mean(u') - xhat mean(xhat u')) + dgamma xhat + dbeta    (at EVERY cell, dead
 *         and unfired ones included: GroupNorm runs on the masked field; without GroupNorm xn' = u')
 *   v'  = v + update_gain (1 - t^2) xn';   v'[:, 3] *= post_alive(x')
 * A sample that a masked or nsteps step leaves alone passes v through and receives no parameter
 * term; a step with message_gain == 0 or no offsets ignores dWm, dbm.  The step is dual to
 * gnca_step_bwd_f32: for (gx, g_theta) = VJP(gy), <gy, v'> = <gx, v> + sum_theta <g_theta, dtheta>.
 *
 * The direction travels as a gnca_weights `dw` whose fields w1, b1, w2, gn_weight, gn_bias, wm, bm
 * are read, each with the shape of the weight it perturbs (NULL = a zero direction for that tensor);
 * every other field is ignored.  The block entry takes dw [K]: direction j carries the pair
 * (v_j, dw[j]) beside the one primal.  The workspaces are the twins': gnca_step_tangent_workspace_bytes,
 * gnca_rollout_tangent_workspace_bytes, gnca_rollout_tangent_block_workspace_bytes.  x_out / x_final
 * stay bitwise the twins', and a zero direction gives the twins' v_out for finite inputs.
 *
 * Refused before any launch: everything the twins refuse (the zero-padded shift: GNCA_ERR_UNSUPPORTED);
 * dw == NULL or a dw tensor that is one of the outputs (GNCA_ERR_INVALID); GNCA_TANGENT_RENORM and
 * GNCA_TBLOCK_ORTHO (GNCA_ERR_INVALID): rescaling or mixing v alone breaks linearity in the pair
 * (v, dtheta).  log_norm / log_r are still recorded.  No class of the support set is refused: where
 * both weight images do not fit the LDS (hidden > 128) the kernel stages them 128 hidden rows at a time.
 * -------------------------------------------------------------------------------------------*/
int gnca_step_tangent_params(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                             const float* x, const void* fire, const uint8_t* active, const float* v, float* x_out,
                             float* v_out, void* ws, size_t ws_bytes, void* hip_stream);

int gnca_rollout_tangent_params(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                const gnca_rollout_sched* sched, const gnca_tangent_args* args, const float* x,
                                const float* v, float* x_final, float* v_final, void* ws, size_t ws_bytes);

int gnca_rollout_tangent_block_params(const gnca_step_desc* desc, const gnca_weights* w,
                                      const gnca_weights* dw /* [K] */, const gnca_rollout_sched* sched,
                                      const gnca_tangent_block_args* args, const float* x, const float* v,
                                      float* x_final, float* v_final, void* ws, size_t ws_bytes);

/* ---------------------------------------------------------------------------------------------
 * A forward-mode objective: the two tap losses and their directional
 * derivatives along K tangents, computed where the tangents are, and the kernel that assembles a
 * forward gradient from K such derivatives and K weight directions.  No new name carries the _f32
 * suffix; the stream is named hip_stream or travels in gnca_rollout_taps.
 *
 * For the state S [B,C,H,W] after a tapped step and the K tangents v_k of it (channels 0..3 only):
 *   losses[b]      bitwise gnca_loss_premult_f32 / gnca_loss_masked_f32 of S[:, :4] (the same
 *                  per-sample body, workgroup shape and order), so bitwise the reverse-mode taps'
 *   dlosses[k][b]  = sum over the cells q and the channels c < 4 of (double) grad_c(q) * (double) v_k[b,c,q]
 *                  with grad the fp32 value gnca_loss_premult_bwd_f32 / gnca_loss_masked_bwd_f32 write
 *                  for g = 1 (and the reverse-mode taps add).  Every product is exact in fp64; the sums
 *                  are fixed-order (per thread over its cells, channels ascending, then the workgroup),
 *                  no float atomics: bitwise reproducible, and a sample's numbers depend neither on the
 *                  batch around it nor on K.  The masked kind counts the target's alive cells in the
 *                  same pass.
 * One 256-thread workgroup per (sample, GNCA_LOSS_TANGENT_DIRS directions): the state's four planes
 * and the target are read once per workgroup and serve all its directions.
 *
 * gnca_loss_tangent is that kernel alone, the forward-mode counterpart of the two *_bwd_f32 entry
 * points.  d: B, H, W of either kind and the knobs of the masked one.  pred [B,4,H,W] with its sample
 * stride; v: direction k of sample b at v + k v_dstride + b v_bstride, four planes H*W apart;
 * target_bstride as gnca_loss_premult_f32 (0 = one target).  losses [B] may be NULL.
 * GNCA_ERR_INVALID before any launch: an unknown kind, a null or empty d, num_dirs < 1, a null pred,
 * v, target or dlosses, a negative stride.
 * -------------------------------------------------------------------------------------------*/
#define GNCA_LOSS_TANGENT_DIRS 4   /* directions one workgroup of the loss tangent kernel serves */

int gnca_loss_tangent(int32_t kind, const gnca_masked_loss_desc* d, int32_t num_dirs, const float* pred,
                      int64_t pred_bstride, const float* v, int64_t v_dstride, int64_t v_bstride,
                      const float* target, int64_t target_bstride, float* losses /*[B] or NULL*/,
                      double* dlosses /*[K][B]*/, void* hip_stream);

/* Bytes of device workspace the entry point below needs (0 on an invalid or unsupported desc, schedule,
 * tap list or K).  Host-only.  [T][B] masks, one step workspace, two states, 2K tangents: apart from the
 * masks it does not grow with T, and it does not grow with the number of taps. */
size_t gnca_rollout_objective_tangent_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                                      const gnca_rollout_taps* taps, int32_t num_dirs);

/*
 * The block rollout without a QR and without log norms, with the kernel above run on (x', v') right
 * after every tapped step: per step the primal runs once and the two tangent kernels once per direction.
 *   x_final   bitwise gnca_rollout_fwd_f32's
 *   v_final   [K][B][n] or NULL (not wanted); bitwise the block rollout's without GNCA_TBLOCK_ORTHO
 *             (with dw: the _params twin's)
 *   losses    f32 [R][B], bitwise gnca_rollout_fwd_taps'
 *   dlosses   f64 [R][K][B]
 *   v         [K][B][n], or NULL = a zero block (made on the device), which needs dw
 *   dw        [K] weight directions, or NULL = none, which needs v
 * Everything travels on taps->stream: no allocation, no host synchronisation, capturable.
 * Refused before any launch: what the block rollout refuses (the zero-padded shift: GNCA_ERR_UNSUPPORTED,
 * workspace size 0; GNCA_SCHED_RECOMPUTE / GNCA_SCHED_CHECKPOINT: GNCA_ERR_INVALID), what
 * gnca_rollout_fwd_taps refuses about a tap list (a missing alive_count of the masked kind included),
 * num_dirs outside 1..GNCA_TANGENT_MAX_DIRS, v and dw both NULL, a null x, x_final, losses or dlosses,
 * and aliasing between an input (x, v, a dw tensor) and an output or between two outputs.
 */
int gnca_rollout_objective_tangent(const gnca_step_desc* desc, const gnca_weights* w,
                                   const gnca_weights* dw /*[K] or NULL*/, const gnca_rollout_sched* sched,
                                   const gnca_rollout_taps* taps, int32_t num_dirs, const float* x,
                                   const float* v /*[K][B][n] or NULL = zeros*/, float* x_final,
                                   float* v_final /*[K][B][n] or NULL*/, float* losses /*[R][B]*/,
                                   double* dlosses /*[R][K][B]*/, int32_t* alive_count /*[B], masked only*/,
                                   void* ws, size_t ws_bytes);

/*
 * The forward gradient of K directional derivatives and K directions, in two launches:
 *   coef[k] = scale * sum_r tap_weight[r] * sum_b dlosses[r][k][b]       one workgroup per k, fp64, fixed
 *             order (b: per thread, then the workgroup; r ascending; products and sums rounded one by one)
 *   g[e]    = (ACCUMULATE ? g[e] : 0) + (float) sum_k coef[k] * (double) dir_k[e]
 *             k ascending, every product and sum rounded in fp64 (never contracted), rounded to fp32 once
 * for up to GNCA_OPTIM_MAX_TENSORS tensors; direction k of a tensor lives at dir + k * dir_stride.  A
 * non-finite dlosses entry makes coef[k], and with it g, non-finite: reported, not hidden.  With
 * scale = 1 / (K B) and directions drawn from N(0, I) this is the unbiased forward-gradient estimate of
 * the batch mean of the weighted tap losses.  The descriptor travels as the kernel argument (which is why
 * the directions are a base and a stride, not K pointers); coef is device memory, 8-B aligned, written
 * by the first launch and read by the second.
 * GNCA_ERR_INVALID before any launch: a null d, dlosses or coef, K, R or B < 1, num_tensors outside
 * 0..GNCA_OPTIM_MAX_TENSORS, an unknown flag, a tensor with a null g or dir or a negative numel or stride.
 */
#define GNCA_FGRAD_ACCUMULATE (1u << 0)

typedef struct gnca_forward_grad_tensor {
  float* g;             /* DEVICE, contiguous fp32 [numel]: written (or accumulated into)            */
  const float* dir;     /* direction 0 of this tensor                                                */
  int64_t dir_stride;   /* floats between two directions of this tensor                              */
  int64_t numel;
} gnca_forward_grad_tensor;

typedef struct gnca_forward_grad_desc {
  int32_t K, R, B;
  uint32_t flags;           /* GNCA_FGRAD_ACCUMULATE                                                 */
  const double* dlosses;    /* DEVICE fp64 [R][K][B]                                                 */
  const float* tap_weight;  /* DEVICE fp32 [R] or NULL = ones                                        */
  double scale;
  double* coef;             /* DEVICE fp64 [K], out                                                  */
  int32_t num_tensors;      /* 0 .. GNCA_OPTIM_MAX_TENSORS (0: the coefficients alone)               */
  int32_t reserved;         /* 0                                                                     */
  gnca_forward_grad_tensor t[GNCA_OPTIM_MAX_TENSORS];
} gnca_forward_grad_desc;

int gnca_forward_grad(const gnca_forward_grad_desc* d, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Gauss-Newton curvature-vector products of the tap objective:
 *   G dtheta = sum_r scale_r J_r^T H_r J_r dtheta,   L = sum_r scale_r sum_b loss_{r,b}
 * with J_r the Jacobian of the tapped state S_r and H_r the loss's Gauss-Newton curvature there.  Three
 * additive entry points: the loss curvature alone, a tangent forward that leaves a tape and the fields
 * H_r J_r (dtheta, v), and the BPTT that injects scale_r * field_r where gnca_rollout_bwd_taps injects
 * the loss gradients.  No new name carries the _f32 suffix; the stream is named hip_stream or travels
 * in gnca_rollout_taps.
 *
 * For a state S [B,>=4,H,W] (channels 0..3 are read), ONE tangent v of it and the target:
 *   losses[b]   bitwise gnca_loss_premult_f32 / gnca_loss_masked_f32
 *   dlosses[b]  bitwise gnca_loss_tangent's with one direction
 *   field[b][c][q], c < 4, fp32: the curvature applied to v, pulled back to S; every value is an fp64
 *               expression of the fp32 inputs, rounded to fp32 once
 *   quad[b]     fp64: the quadratic form v^T (P^T H P) v, a fixed-order sum (per thread over its cells,
 *               then the workgroup); no float atomics: bitwise reproducible, independent of the batch
 * GNCA_TAP_PREMULT (N = 4HW, a = S_3):  pd_c = a v_c + S_c v_3 (c < 3), pd_3 = v_3,
 *   field_c = (2/N) a pd_c (c < 3),  field_3 = (2/N) (sum_{c<3} S_c pd_c + pd_3),
 *   quad = (2/N) sum_q sum_c pd_c^2.  The residual term (p - target) d2p/dS2 of the bilinear rgb * a is
 *   dropped on purpose: that is what makes G positive semidefinite.
 * GNCA_TAP_MASKED (D = n_b + 1e-8, n_b the target's alive cell count, gnca_loss_masked_bwd_f32's
 *   denominator):  field_c = 2 alive v_c / D,  quad = 2 sum alive v_c^2 / D.  The area and background
 *   penalties are linear or |.| and carry no curvature (|.| at 0 as its sign(0) = 0 gradient treats it);
 *   a target with no alive cell gives an exactly zero field.
 * In exact arithmetic sum_{c,q} field v = quad.
 * One 256-thread workgroup per sample, cells q = tid, tid + 256, ...
 *
 * gnca_loss_curvature is that kernel alone.  Strides as gnca_loss_tangent: pred [B,4,H,W] with its sample
 * stride, v and field four planes H*W apart with their sample strides, target_bstride 0 = one target.
 * losses [B] and dlosses [B] may be NULL.  GNCA_ERR_INVALID before any launch: an unknown kind, a null or
 * empty d, a null pred, v, target, quad or field, a negative stride.
 * -------------------------------------------------------------------------------------------*/
int gnca_loss_curvature(int32_t kind, const gnca_masked_loss_desc* d, const float* pred, int64_t pred_bstride,
                        const float* v, int64_t v_bstride, const float* target, int64_t target_bstride,
                        float* losses /*[B] or NULL*/, double* dlosses /*[B] or NULL*/, double* quad /*[B]*/,
                        float* field /*[B][4][H][W]*/, int64_t field_bstride, void* hip_stream);

/* Bytes of device workspace gnca_rollout_gn_fwd needs (0 on an invalid or unsupported desc, schedule or
 * tap list, a schedule without GNCA_SCHED_RECOMPUTE included).  Host-only.  [T][B] masks, one step
 * workspace, two tangents and, with GNCA_SCHED_CHECKPOINT, two states for the ones between two anchors:
 * apart from the masks it does not grow with T, and it does not grow with the number of taps. */
size_t gnca_rollout_gn_fwd_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                           const gnca_rollout_taps* taps);

/*
 * gnca_rollout_objective_tangent's loop for one direction that also leaves the tape of the primal:
 *   tape      byte-identical to the one gnca_rollout_fwd_f32 writes for the same inputs and schedule:
 *             sched->flags must carry GNCA_SCHED_RECOMPUTE (states only) and may carry
 *             GNCA_SCHED_CHECKPOINT (anchors only).  Every step writes its output state straight into its
 *             slot; slot 0 is the copy of x; no other state copy is made.  gnca_rollout_tape_bytes,
 *             gnca_rollout_bwd_workspace_bytes and the backward apply unchanged.
 *   x_final   bitwise gnca_rollout_fwd_f32's
 *   fields    f32 [R][B][4][H][W], losses f32 [R][B], dlosses f64 [R][B], quad f64 [R][B]: the kernel above
 *             on (x', v') where they lie, one launch after every tapped step.  Nothing else grows with R.
 *   v         [B][n], or NULL = a zero tangent (made on the device), which needs dw
 *   dw        one weight direction, or NULL = none, which needs v
 * Everything travels on taps->stream: no allocation, no host synchronisation, capturable.
 * Refused before any launch: what gnca_rollout_objective_tangent refuses (the zero-padded shift:
 * GNCA_ERR_UNSUPPORTED, workspace size 0; a bad tap list; a missing alive_count of the masked kind; v and
 * dw both NULL), a missing GNCA_SCHED_RECOMPUTE or a null pointer (GNCA_ERR_INVALID), a short tape or
 * workspace (GNCA_ERR_WORKSPACE), and aliasing between an input (x, v, a dw tensor) and an output or between
 * two outputs.
 */
int gnca_rollout_gn_fwd(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw /*or NULL*/,
                        const gnca_rollout_sched* sched, const gnca_rollout_taps* taps, const float* x,
                        const float* v /*[B][n] or NULL = zeros*/, float* x_final, void* tape, size_t tape_bytes,
                        float* fields /*[R][B][4][H][W]*/, float* losses /*[R][B]*/, double* dlosses /*[R][B]*/,
                        double* quad /*[R][B]*/, int32_t* alive_count /*[B], masked only*/, void* ws,
                        size_t ws_bytes);

/*
 * gnca_rollout_bwd_taps without gy whose tap r injects a precomputed field instead of a loss gradient:
 *   g[b, c < 4, q] += (float)(scale[r] * fields[r][b][c][q])     one rounded product, one rounded add
 * where that entry point adds the tap's gradient (the first injection writes the whole cotangent buffer:
 * the product on channels 0..3, zeros elsewhere).  The checkpointed branch and "the steps after the last
 * tap are not run" are kept; the step's backward and its kernels are the same.  scale: HOST f32 [R].
 * With gnca_rollout_gn_fwd's tape and fields:
 *   grads = G_tt dtheta + G_tx v,   gx = G_xt dtheta + G_xx v
 * Workspace: gnca_rollout_bwd_workspace_bytes.  Everything travels on taps->stream.  GNCA_ERR_INVALID
 * before any launch: a bad tap list, a null fields, scale or gx, a schedule without GNCA_SCHED_RECOMPUTE;
 * a short tape or workspace: GNCA_ERR_WORKSPACE.
 */
int gnca_rollout_gn_bwd(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                        const gnca_rollout_taps* taps, const void* tape, size_t tape_bytes,
                        const float* fields /*[R][B][4][H][W]*/, const float* scale /*HOST [R]*/, float* gx,
                        const gnca_grads* grads, void* ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* GNCA_H */
