/* eae.h -- C ABI of libeae.so: the MI355X (gfx950) engine behind the notebook's Encoder / Decoder /
 * SupervisedAutoencoder / MLP modules and its fit / evaluate loops.
 *
 * The reference has no FFI for this path: its boundary is the Python class surface of the notebook
 * (R.md = /root/reference/Report/Hybrid_autoencoder–MLP_pipeline_for_satellite_image_classification.md):
 *   Encoder.forward  R.md:312        Decoder.forward R.md:386-389      SupervisedAutoencoder.forward R.md:429-433
 *   AE train step    R.md:646-654    AE validation step R.md:673-677   MLP.forward R.md:2565
 *   MLP train step   R.md:2641-2646  extract_features R.md:2498-2510   final evaluate R.md:3171-3187
 * Each entry point below names the reference lines it replaces.  The Python shells in
 * hybrid-autoencoder-mlp-pipeline-for-satellite-image-classification_amd/ bind these with ctypes.
 *
 * Conventions: every function returns 0 on success and a negative code on error (message: eae_last_error());
 * no C++ exception crosses the boundary.  All tensor arguments are raw DEVICE pointers owned by the caller with the
 * layout stated per argument; `stream` is a hipStream_t passed as void*; all work is enqueued on it and nothing
 * synchronises except eae_destroy / eae_mlp_destroy.  A ctx is bound to the current device and used from one thread.
 */
#ifndef EAE_H
#define EAE_H
#ifdef __cplusplus
extern "C" {
#endif

#define EAE_OK 0
#define EAE_ERR_ARG (-2)     /* bad shape / null pointer / unsupported configuration */
#define EAE_ERR_HIP (-3)     /* a HIP runtime call failed */
#define EAE_ERR_STATE (-4)   /* call order (e.g. backward without forward, ctx not bound) */

const char* eae_last_error(void);
int eae_version(void);

/* ------------------------------------------------------------------ autoencoder engine ---------------------- */
typedef struct eae_ctx eae_ctx;

typedef struct eae_config {
  int latent_dim;    /* Encoder/Decoder/SupervisedAutoencoder(latent_dim)  R.md:288, 362, 417; any width in 1..256 (padded to a
                        multiple of 64 inside the packs and workspaces; the parameter / gradient arenas keep the reference shapes) */
  int num_classes;   /* SupervisedAutoencoder(num_classes=10)             R.md:417; 1..64 */
  int image_h;       /* 64 for EuroSAT; must be a multiple of 64 */
  int image_w;
  int max_batch;     /* workspaces are sized for this many images per call */
  int quant;         /* 0: bf16 operands.  1: BASELINE config 5's stress variant -- the GEMMs of the six 3x3 layers (forward,
                        backward-data, weight gradient) take fp8 operands on v_mfma_f32_16x16x32_{fp8,bf8}_{fp8,bf8}: weights and
                        activations OCP e4m3, gradients e5m2, per-tensor power-of-two scales with delayed scaling (eae_fp8_calibrate),
                        fp32 accumulation, everything else as with 0.  Needs image_h % 128 == 0 and image_w % 256 == 0. */
  int side_streams;  /* 0: default (two engine-owned side streams for the work that only feeds the optimizer: weight gradients, head,
                        loss bookkeeping); 1 or 2: that many; -1: none, every kernel goes to the caller's stream in dependency order.
                        A process reaches the GPU through 4 hardware queues: when SEVERAL contexts are stepped concurrently (a grid of
                        small configurations, train.run_concurrent) one stream per context lets four of them run side by side, three
                        streams per context share the four queues (measured at batch 64: 4 contexts 487 K vs 352 K images/s). */
  int in_channels;   /* image bands C, 1..16 (Encoder(in_channels=C)); 0 means 3 (RGB).  Sizes conv1's weight [32,C,3,3], deconv4's
                        weight [32,C,3,3] ([Cin,Cout,kh,kw]) and bias [C], and every image-shaped tensor [B,C,H,W] of eae_step_io and
                        the calls below.  quant = 1 needs C = 3.  All members of an eae_group_* call must share it. */
} eae_config;

/* fp8 variant only.  eae_fp8_calibrate: `iters` (<= 0: 7) gradient steps WITHOUT optimizer on the given batch to settle the delayed
 * scales before the first real step (running statistics are restored, the gradient arena is overwritten).
 * eae_fp8_scales: the current scales, s_act[6], s_grad[6], s_w[6] for conv2, conv3, conv4, deconv1, deconv2, deconv3 (synchronises);
 * a scale multiplies a value before its conversion. */
struct eae_step_io;
int eae_fp8_calibrate(eae_ctx* ctx, void* stream, const struct eae_step_io* io, int iters);
int eae_fp8_scales(eae_ctx* ctx, float* out18);

#define EAE_AE_NPARAMS 38   /* model.parameters() order of SupervisedAutoencoder */
#define EAE_AE_NBN 7        /* BatchNorm2d layers: enc.encoder.{1,4,7,10}, dec.decoder.{2,5,8} */

/* Flat arena layout.  param_off[i] (i < 38) = element offset of the i-th tensor of named_parameters() in the fp32
 * parameter / gradient / Adam arenas, param_off[38] = arena length (multiple of 4; every tensor 16-byte aligned).
 * bn_off[2*l] / bn_off[2*l+1] = offsets of running_mean / running_var of BN layer l in the running-stat arena,
 * bn_off[14] = its length. */
int eae_ae_layout(const eae_config* cfg, long long* param_off, long long* bn_off);

/* Environment switches read by eae_create are listed in INTEGRATION.md.  One of them changes results: EAE_NAN_EXACT=1 -- a DIVERGED
 * train step (a non-finite BatchNorm statistic was consumed: the loss scalars read NaN) writes NaN into every parameter and both Adam
 * moments, which is what the reference's loop does to its model (loss.backward() on a non-finite loss gives every parameter a NaN
 * gradient, torch.optim.Adam propagates it: R.md:653-654; pinned by tests/golden/ae_nan_step_b8.npz).  Default: the optimizer refuses
 * the update and the last finite parameters stay (the run still reads as diverged through its NaN losses). */
int eae_create(const eae_config* cfg, eae_ctx** out);
int eae_destroy(eae_ctx* ctx);

/* Bind the caller-owned arenas (fp32 unless noted).  grads/adam_m/adam_v may be NULL for inference-only use.
 * bn_nbt: int64[7] num_batches_tracked. */
int eae_bind(eae_ctx* ctx, float* params, float* grads, float* adam_m, float* adam_v, float* bn_running,
             long long* bn_nbt);
/* The engine orders its side streams behind the caller's stream with one-wave GATE kernels that poll a device progress word
 * (no event record on the caller's stream; EAE_FORK_EVENTS=1 restores events).  Their spin is bounded by wall-clock time (30 s;
 * EAE_GATE_TIMEOUT_MS=<ms>, 0 = unbounded), so a caller's stream stalled for seconds in front of a step is simply waited for.
 * A gate that gives up sets a STICKY device word: from then on every optimizer kernel of the context leaves the parameters
 * untouched and writes NaN into the step's loss_last (the gradients of that step may come from stale activations).
 * eae_gate_timeouts synchronises the device and returns 0, or the value a gate gave up waiting for; eae_gate_timeouts_clear
 * resets the word once the caller has dealt with the failed step.  Replaces nothing in the reference (R.md:642-658 runs on one
 * in-order stream); it guards the engine's own side-stream concurrency. */
long long eae_gate_timeouts(eae_ctx* ctx);
long long eae_gate_timeouts_nosync(eae_ctx* ctx);   /* same word, no device synchronisation (the caller has synchronised its own stream) */
int eae_gate_timeouts_clear(eae_ctx* ctx);
/* Replay eae_ae_train_step from a captured hipGraph (from the third call with the same buffers, batch size and alpha) or enqueue it
 * eagerly (default; EAE_GRAPH=1 in the environment turns replay on at creation).  Replay pays when the HOST is the limit: several small
 * configurations stepped concurrently (train.py run_concurrent, R.md:599-711 at batch 64). */
int eae_set_graph(eae_ctx* ctx, int on);
/* Class-weighted cross-entropy with ignored labels in the fused steps: torch's CrossEntropyLoss(weight=w, ignore_index=i, reduction=
 * "mean") for imbalanced or partly labelled data (a scene's window labels: -1 = unlabelled, scene.py).
 * weights: device fp32 [num_classes] (finite, >= 0), caller-owned and kept until replaced, or NULL (all ones).  weights == NULL and
 * ignore_index == EAE_NO_IGNORE switch the feature off: the kernels and the contract of before (every label in [0, C)).
 * With the feature on, row r is COUNTED when labels[r] != ignore_index and 0 <= labels[r] < C -- every label out of range is ignored
 * (-1, a raster's 255), none indexes out of its row.  W = sum over the counted rows of w[y_r];
 *     CE = sum_counted w[y_r] (lse_r - logit_r[y_r]) / W,    dlogits_r = (softmax_r - onehot) w[y_r] / W, an exact zero row if not counted;
 * the number of correct predictions counts counted rows only; the logits output is unchanged.  loss_accum / loss_last keep their
 * meaning: accum[2] += CE * B, accum[3] += B (all rows of the batch), accum[4] += counted correct rows.
 * Deviation from torch: when no row is counted (or every counted row has weight 0) W = 0 and torch returns NaN, which this engine
 * reads as "diverged"; here CE = 0, the head's gradients and dz_cls are exact zeros, everything is finite and the step still trains
 * on alpha * MSE.
 * W is summed inside the head kernel by every workgroup in one fixed order (no atomics, no host synchronisation): results are
 * bitwise repeatable.  The setting reaches every call that computes CE from labels: eae_ae_forward, eae_ae_grad_step(_begin),
 * eae_ae_train_step, eae_ae_dp_train_step, eae_fp8_calibrate, eae_group_train_step, eae_group_forward; eae_ae_backward (external
 * dlogits) is unaffected.  Data parallel: each replica normalises by the W of its OWN batch and the gradients are averaged by 1/world
 * as before -- what DistributedDataParallel around a weighted criterion computes; W is not summed over the replicas.
 * A grouped call needs the feature on in every member or in none (each member its own vector and ignore_index): a mixture is
 * EAE_ERR_ARG.  Changing the setting drops the captured step graphs (eae_set_graph): the next calls capture again (synchronises
 * the device when there is one to drop). */
#define EAE_NO_IGNORE (-0x7fffffffffffffffLL - 1)
int eae_set_class_weights(eae_ctx* ctx, const float* weights, long long ignore_index);
/* Labelled-sample count: counter = a caller-owned device int64 word (kept until replaced) or NULL.  While the feature above is on,
 * every call that computes CE from labels AND accumulates its loss (io->loss_accum != NULL) adds the number of counted rows of its
 * batch to *counter -- inside the head kernel's own pass over the labels (one writer per launch): no extra launch, no host
 * synchronisation.  With the feature off nothing is written (every row counts: accum[3]).  Drops the captured step graphs like
 * eae_set_class_weights. */
int eae_set_valid_counter(eae_ctx* ctx, long long* counter);
/* Clip the global gradient norm on the device (torch.nn.utils.clip_grad_norm_ with norm_type = 2) in front of EVERY optimizer launch
 * of the context.  max_norm == 0: off (the default: the launches and the bits of before).  max_norm > 0 or +inf: on; +inf measures the
 * norm and never clips.  Negative or NaN: EAE_ERR_ARG.  norm_out: a caller-owned device float[2], kept until replaced, or NULL.
 * While on, with s = the call's grad_scale (1, or 1/world in data parallel):
 *     total = s * sqrt(sum g_i^2)   over the elements of the 38 gradient tensors -- the padding eae_ae_layout leaves between tensors
 *                                   does not contribute (the arenas are the caller's: it need not be zero)
 *     coef  = min(1, max_norm / (total + 1e-6))       in fp32
 * and Adam consumes fma(g, fl32(s * coef), weight_decay * p): weight decay is added after the clip, as in torch, and with coef == 1
 * the update is the unclipped one bit for bit.  norm_out[0] = total and norm_out[1] = coef are written by that optimizer launch, also
 * when the update is refused.  A non-finite total makes the step DIVERGED: no update, loss_last reads NaN, and with EAE_NAN_EXACT=1 the
 * NaN fill applies as for non-finite BatchNorm statistics (torch would write NaN gradients; this engine keeps the last finite state).
 * The sum is taken in fp64 by one extra launch in front of the optimizer kernel: per-workgroup partials in a fixed order, added by
 * every workgroup of the optimizer kernel in a fixed order -- no atomics, no host synchronisation, bitwise repeatable, and independent
 * of the launch geometry (a member of a grouped step computes what it computes alone).
 * Reached: eae_adam_step, eae_adam_step_scaled, eae_adam_step_dp, eae_ae_train_step (eager and graph replay, bitwise equal),
 * eae_ae_dp_train_step (the norm of the all-reduced gradient: the replicas hold the same sums and derive the same coefficient, no
 * extra collective), eae_group_train_step (each member its own max_norm and norm_out; on in every member or in none -- a mixture is
 * EAE_ERR_ARG, a member that should not clip passes +inf), fp8 contexts.  Not reached: eae_mlp_train_step (its iteration is one
 * kernel) and eae_op_adam.  Changing the setting drops the captured step graphs like eae_set_class_weights. */
int eae_set_grad_clip(eae_ctx* ctx, float max_norm, float* norm_out);
/* The host changed parameter values (load_state_dict, optimizer outside the engine): repack before next use. */
int eae_params_changed(eae_ctx* ctx);
int eae_set_adam_step(eae_ctx* ctx, long long step);
long long eae_get_adam_step(eae_ctx* ctx);

typedef struct eae_step_io {
  const float* x;            /* [B,C,H,W] fp32 NCHW (C = eae_config::in_channels), the loader contract (R.md:643) */
  const long long* labels;   /* [B] int64 (R.md:644) or NULL */
  int B;
  int train;                 /* 1: model.train() semantics (batch statistics, running-stat update); 0: model.eval() */
  int head;                  /* 1: classifier head + CrossEntropy; 0: encoder+decoder only (MSE) */
  float alpha;               /* loss = alpha * MSE(x_hat, x) + CE(logits, labels)   R.md:649-651 */
  float* x_hat;              /* optional [B,C,H,W] fp32 NCHW */
  float* logits;             /* optional [B,num_classes] fp32 */
  float* z;                  /* optional [B,latent_dim] fp32 */
  float* loss_accum;         /* optional float[8]: += loss*B, mse*B, ce*B, B, #correct  (R.md:656-657, 679-681) */
  float* loss_last;          /* optional float[4]: loss, mse, ce of this call.  With a SEPARATE optimizer call (eae_ae_grad_step /
                              * eae_ae_backward followed by eae_adam_step*) the pointer is kept until that ONE optimizer launch, which
                              * writes NaN there when it refuses the update; it is dropped afterwards: keep the buffer alive until the
                              * optimizer call of the step has been enqueued */
} eae_step_io;

/* x_hat, logits, z = model(x) (R.md:647 / 673), plus the loss terms when io->x target / labels are given. */
int eae_ae_forward(eae_ctx* ctx, void* stream, const eae_step_io* io);
/* loss.backward() for a torch-side loss (R.md:649-653): backward of the most recent eae_ae_forward -- train mode, or eval mode
 * (io->train = 0: BatchNorm with the running statistics is differentiated as the per-channel affine map it then is; the biases in
 * front of the BatchNorms then get their gradient A[c] * sum g instead of zero) -- given the gradients of its outputs (fp32; dx_hat [B,in_channels,H,W], dlogits [B,C] or NULL, dz [B,L] or NULL).  x = that forward's input batch
 * (conv1's weight gradient reads it again: the engine keeps no pointer to caller memory across calls), x_hat = its output,
 * generation = eae_forward_generation() read right after that forward: EAE_ERR_STATE if any forward ran since.
 * Gradients of all 38 tensors land in the grad arena (train mode: biases in front of a BatchNorm are exact zeros). */
long long eae_forward_generation(eae_ctx* ctx);
int eae_ae_backward(eae_ctx* ctx, void* stream, long long generation, const float* x, const float* x_hat, const float* dx_hat,
                    const float* dlogits, const float* dz);
/* zero_grad + forward + loss + backward (R.md:646-653): gradients of all 38 tensors land in the grad arena. */
int eae_ae_grad_step(eae_ctx* ctx, void* stream, const eae_step_io* io);
/* optimizer.step() of torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) over the bound arenas (R.md:624, 654). */
int eae_adam_step(eae_ctx* ctx, void* stream, float lr, float weight_decay);
/* Data-parallel training (new work, no reference counterpart): the gradient step in two halves.  After _begin the gradient
 * tensors 18..37 (dec.fc, decoder, classifier) are complete once the engine's side stream (eae_side_stream) has drained, so
 * their all-reduce can be enqueued behind that stream and overlap with _end (enc.fc + encoder).  eae_adam_step_scaled
 * multiplies the (summed) gradients by grad_scale = 1/world_size inside the optimizer kernel. */
int eae_ae_grad_step_begin(eae_ctx* ctx, void* stream, const eae_step_io* io);
int eae_ae_grad_step_end(eae_ctx* ctx, void* stream);
void* eae_side_stream(eae_ctx* ctx);
/* Test / diagnostic access to the workspace tensors of the most recent step (bf16 NHWC; the device is synchronised first):
 * kind 0 = raw conv outputs y[idx] (idx 0..3), 1 = their masked gradients gy[idx], 2 = raw transposed-conv outputs u[idx] (0..2),
 * 3 = gu[idx], 4 / 5 = the BatchNorm-backward-applied gradients dy the backward-data kernels store for the weight-gradient kernels
 * (idx 1..3 / 0..2).  Copies up to `bytes` into host memory; returns the bytes copied (negative: error).  No reference counterpart:
 * torch keeps these as autograd-internal buffers of loss.backward() (R.md:653). */
long long eae_debug_read(eae_ctx* ctx, int kind, int idx, void* host_dst, long long bytes);
/* kind EAE_DEBUG_PACK: read-only access to the pack arena, the kernel layouts of the weights (bf16 unless noted) that the pack kernel
 * derives from the parameter arena in front of the first forward after eae_bind, eae_params_changed or an optimizer step.  idx selects
 * one pack (CP = the padded band count 4 / 8 / 16, KP = 9 * CP rounded up to 32, P = image_h / 16 * image_w / 16, K = 256 * P,
 * Lp = latent_dim rounded up to 64):
 *    0       conv1 [32][KP], k = tap * CP + c
 *    1..6    p1 of conv2, conv3, conv4, deconv1, deconv2, deconv3: [A][9][B] of the weight [A][B][3][3]
 *    7..12   p2 of the same layers: [B][9][A]
 *    13      deconv4 joint pack [4 * CP][128]              14  deconv4 [32][KP] (its weight [32][C][3][3] as conv1's)
 *    15, 16  enc.fc [Lp][K'] and its transpose [K'][Lp], k' = p * 256 + c
 *    17, 18  dec.fc [K'][Lp] and its transpose [Lp][K']
 *    19, 20  classifier.0.weight [128][Lp] and enc.fc.bias [Lp], fp32: only with latent padding (Lp != latent_dim), else EAE_ERR_STATE
 *    21      dec.fc bias [K'], fp32
 *    22..27  e4m3 bytes of p1 for the six layers, 28..33 of p2: only with quant = 1, else EAE_ERR_STATE
 * Synchronises the device, copies min(bytes, length) bytes (host_dst may be NULL when bytes is 0) and returns the pack's full length,
 * so that a first call with bytes = 0 sizes the buffer.  The read never packs: it shows what the arena holds.
 * eae_debug_fill_packs: set every byte of the pack arena to `byte` and mark the packs stale (synchronises); with 0xFF every bf16, fp32
 * and e4m3 element reads as NaN until the pack kernel has written it. */
#define EAE_DEBUG_PACK 6
#define EAE_PACK_CONV1 0
#define EAE_PACK_P1 1
#define EAE_PACK_P2 7
#define EAE_PACK_DECONV4_JOINT 13
#define EAE_PACK_DECONV4_KCP 14
#define EAE_PACK_WE1 15
#define EAE_PACK_WE2 16
#define EAE_PACK_WD1 17
#define EAE_PACK_WD2 18
#define EAE_PACK_W1P 19
#define EAE_PACK_BEP 20
#define EAE_PACK_BD 21
#define EAE_PACK_FP8_P1 22
#define EAE_PACK_FP8_P2 28
int eae_debug_fill_packs(eae_ctx* ctx, int byte);
/* The same hand-off without splitting the call (no host gap between the halves): once requested, engine-owned stream `which`
 * is, after every eae_ae_grad_step, ordered after the completion of gradient tensors 18..37 (which = 0: classifier, decoder,
 * dec.fc) or 8..17 (which = 1: enc.fc, conv4, conv3); a collective enqueued behind it overlaps the rest of that step's
 * backward.  Tensors 0..7 are complete on the caller's stream when the call returns.  NULL when side-stream concurrency is
 * disabled. */
void* eae_dp_stream(eae_ctx* ctx, int which);
int eae_adam_step_scaled(eae_ctx* ctx, void* stream, float lr, float weight_decay, float grad_scale);
/* The collective owned by the engine (SURVEY.md 8b "DP eae_dp_init(ctx, rank, world, ncclUniqueId), eae_dp_allreduce_bucket"; new
 * work: the reference has no parallelism).  One process per GPU; librccl is bound at run time (the copy already in the
 * process if any).  eae_dp_unique_id: rank 0 draws the 128-byte ncclUniqueId, the caller ships it to the other ranks;
 * eae_dp_init: every rank joins (collective call).  eae_dp_allreduce_bucket: in-place sum over the ranks of gradient-arena elements
 * [elem_off, elem_off + count) on `stream`.  eae_dp_broadcast: `bytes` of a device buffer from `root` (identical replicas at start).
 * eae_ae_dp_train_step: eae_ae_train_step for a replica -- forward, loss, backward, gradient all-reduce, Adam with the 1/world scale
 * folded into the optimizer kernel -- enqueued by one call with no host code between backward and collective; overlap != 0 sends
 * the decoder-side bucket (tensors 18..37) over the engine's hand-off stream while the encoder half of the backward computes. */
int eae_dp_unique_id(void* id128);
int eae_dp_init(eae_ctx* ctx, int rank, int world, const void* id128);
int eae_dp_world(eae_ctx* ctx);
int eae_dp_destroy(eae_ctx* ctx);
int eae_dp_allreduce_bucket(eae_ctx* ctx, void* stream, long long elem_off, long long count);
int eae_dp_broadcast(eae_ctx* ctx, void* stream, void* buf, long long bytes, int root);
int eae_ae_dp_train_step(eae_ctx* ctx, void* stream, const eae_step_io* io, float lr, int overlap);
/* The decision "this step must not update the parameters" (a side-stream gate timed out: sticky; a non-finite BatchNorm statistic:
 * this step) is taken for ALL replicas together, or they would diverge silently: eae_ae_dp_train_step max-reduces one flag word over
 * the ranks next to the last gradient bucket.  For an exchange the caller runs itself (torch.distributed): eae_dp_local_bad writes this
 * rank's TWO flags (stale, diverged; 0 / 1 each) to a pair of device words on `stream`; the caller max-reduces the pair and hands it to
 * eae_adam_step_dp, which is eae_adam_step_scaled with those words as the refusal switches (NULL: the local switches).  eae_dp_init is time-bounded
 * (EAE_DP_INIT_TIMEOUT_S, default 120 s: the rendezvous runs on a helper thread the caller waits for with a deadline; the communicator
 * stays a BLOCKING one): a peer that never joins yields an error, not a hang. */
int eae_dp_local_bad(eae_ctx* ctx, void* stream, unsigned* out_dev);
int eae_adam_step_dp(eae_ctx* ctx, void* stream, float lr, float weight_decay, float grad_scale, const unsigned* peer_bad);
/* Synchronized BatchNorm across data-parallel replicas (new work; SURVEY.md 8e: R ranks x B/R with SyncBN == 1 rank x B).
 * In train mode the engine calls `fn` once per BatchNorm layer in the forward (kind 0: `count` int64 fixed-point accumulators
 * starting at element `elem_offset` of acc_i64) and once per layer in the backward (kind 1: `count` fp64 sums at element
 * `elem_offset` of sums_f64): the hook all-reduces (SUM) that range over the replicas, enqueued on `stream`, and returns 0.
 * acc_i64: caller-owned device buffer of eae_sync_bn_acc_elems() int64 (zero-initialised); sums_f64: 7*2*256 fp64.
 * world <= 1 or fn NULL switches it off (per-replica statistics, the default: DDP semantics).
 * Range of the fixed-point accumulators (csrc/eae_bn_acc.h): with N = workgroups per channel of the layer's
 * launch x world, a workgroup's sums of y and y^2 must stay below 2^38 / N in the forward (quantum 2^-24) and its sums of g and
 * g * xhat below 2^20 / N in the backward (quantum 2^-42; with world > 1 the backward sums travel as fp64 and have no limit); a larger
 * or non-finite sum flags the channel: NaN statistics, NaN losses, no update.  The world enters because the replicas' integers are
 * summed: eight replicas leave each workgroup an eighth of the range. */
typedef int (*eae_sync_fn)(void* user, int kind, long long elem_offset, long long count, void* stream);
long long eae_sync_bn_acc_elems(eae_ctx* ctx);
int eae_set_sync_bn(eae_ctx* ctx, int world, eae_sync_fn fn, void* user, void* acc_i64, void* sums_f64);
/* eae_ae_grad_step + eae_adam_step: one iteration of the reference's batch loop (R.md:642-658). */
int eae_ae_train_step(eae_ctx* ctx, void* stream, const eae_step_io* io, float lr);
/* The grid of independent configurations the reference trains one after the other at batch 64 (R.md:246, 599-711), n of them per
 * call: eae_ae_train_step's eager path (eae_group_train_step) or eae_ae_forward (eae_group_forward: the validation pass, R.md:670-682)
 * for ctxs[0..n) -- each with its own io block (inputs, labels, alpha, outputs) and lr -- enqueued as ONE sequence of grouped launches
 * on `stream` and ctxs[0]'s side streams (workgroup z of every launch works for member z with that member's own arguments).
 * geometry_mult: the launchers choose tile geometries and grids as for a batch of B * geometry_mult (0 = n; a caller whose group
 * shrinks -- early stopping -- keeps passing the original size so that a member's arithmetic does not depend on who else is still
 * training).  Each member's results are bitwise what the single-context call gives it under eae_set_geometry_mult(geometry_mult).
 * The members must have the same configuration, batch size and requested outputs, live on the current device, and have profiling,
 * fp8 and data parallel off; a mismatch is an error and leaves the members' host-side state advanced (as a failed step does).
 * n <= 64; launches carry 8 members at a time. */
int eae_group_train_step(eae_ctx* const* ctxs, int n, int geometry_mult, void* stream, const eae_step_io* ios, const float* lrs);
int eae_group_forward(eae_ctx* const* ctxs, int n, int geometry_mult, void* stream, const eae_step_io* ios);
/* Hardware queues.  ROCm multiplexes a process's streams onto 4 hardware queues and two streams on one queue run one after the other.
 * Before its first step on a caller's stream a context checks its side streams against that stream, against each other and against
 * every stream other contexts are stepping on, and replaces a side stream that collides (EAE_STREAM_PROBE=0: off, =2: verbose).
 * eae_streams_share_queue: the same check for two arbitrary streams (1 = one queue, 0 = different ones; synchronises the device);
 * eae_reserve_stream(stream, 1): a driver that steps contexts from several host threads announces its worker streams, so that the
 * contexts' side streams keep clear of them too; (stream, 0) releases. */
int eae_streams_share_queue(void* stream_a, void* stream_b);
int eae_reserve_stream(void* stream, int on);
/* Thread-local: launchers that choose a tile geometry or a grid by the size of the batch see batch * mult (1 = default).  Used by the
 * group-vs-alone parity tests; the group calls set it to their geometry_mult for their own duration. */
int eae_set_geometry_mult(int mult);
/* Encoder alone in the current mode (extract_features, R.md:2504: z = encoder(imgs)). */
int eae_encoder_forward(eae_ctx* ctx, void* stream, const float* x, int B, int train, float* z);
/* Decoder alone (Decoder.forward, R.md:386-389). */
int eae_decoder_forward(eae_ctx* ctx, void* stream, const float* z, int B, int train, float* x_hat);
/* loss.backward() through a stand-alone Encoder / Decoder (the notebook defines them as separate modules, R.md:287, 361; e.g.
 * x_hat = dec(enc(x)) with an MSE loss): backward of the most recent eae_encoder_forward / eae_decoder_forward (train or eval mode)
 * for an externally supplied gradient of its output.  generation = eae_forward_generation() right after that forward.
 * encoder: dz [B][L], x = the forward's input;  decoder: dx_hat [B,in_channels,H,W], x_hat = the forward's output, dz_out [B][L] (may be NULL). */
int eae_encoder_backward(eae_ctx* ctx, void* stream, long long generation, const float* x, const float* dz);
int eae_decoder_backward(eae_ctx* ctx, void* stream, long long generation, const float* x_hat, const float* dx_hat, float* dz_out);

/* In-situ timing of ONE launch site inside real train steps (bench.py's `roofline` object): HIP events are recorded around that
 * launch, on the stream it goes to, for up to 64 steps; eae_profile_read2 synchronises them and returns the summed bracket time,
 * the summed time of an EMPTY bracket recorded right behind each timed one (what the two event records cost by themselves) and
 * the number of launches measured.  site 0 switches the timing off.  Kernel behind each site (rocprofv3 name): */
#define EAE_PROF_OFF 0
/* site = EAE_PROF_SITE(layer, role): layer 0-3 = enc.conv1-4, 4-7 = dec.deconv1-4; role 0 forward, 1 backward-data, 2 weight gradient
 * (layer 0 has no backward-data; layer 7's forward is the fused deconv4 + sigmoid + MSE kernel) */
#define EAE_PROF_SITE(layer, role) (16 + 3 * (layer) + (role))
#define EAE_PROF_CONV2_FWD EAE_PROF_SITE(1, 0)      /* igemm_s2_kernel<0, 32, 64, 64, 16, 8, 1, 1, 0>   enc.conv2 forward */
#define EAE_PROF_CONV2_BWD EAE_PROF_SITE(1, 1)      /* igemm_s2_kernel<1, 64, 32, 32, 16, 8, 1, 2, 1>   enc.conv2 backward-data */
#define EAE_PROF_DECONV3_BWD EAE_PROF_SITE(6, 1)    /* igemm_s2_kernel<0, 32, 64, 64, 16, 8, 1, 2, 1>   dec.deconv3 backward-data */
#define EAE_PROF_CONV2_WGRAD EAE_PROF_SITE(1, 2)    /* wgrad_s2_kernel<64, 32, 16, 8, 1, 2, 1>          enc.conv2 weight gradient */
#define EAE_PROF_DECONV3_WGRAD EAE_PROF_SITE(6, 2)  /* wgrad_s2_kernel<64, 32, 16, 8, 1, 1, 2>          dec.deconv3 weight gradient */
#define EAE_PROF_DECONV4_LOSS EAE_PROF_SITE(7, 0)   /* deconv4_loss_kernel<1>                           dec.deconv4 + sigmoid + MSE + gradient */
#define EAE_PROF_CONV1_WGRAD EAE_PROF_SITE(0, 2)    /* edge_wgrad_kernel<0, 2>                          enc.conv1 weight gradient */
#define EAE_PROF_DECONV4_BWD EAE_PROF_SITE(7, 1)    /* edge_conv_kernel<1, 1>                           dec.deconv4 backward-data */
#define EAE_PROF_DECONV3_FWD EAE_PROF_SITE(6, 0)    /* igemm_s2_kernel<1, 64, 32, 32, 16, 8, 1, 1, 0>   dec.deconv3 forward */
#define EAE_PROF_NSITES 40
int eae_profile_enable(eae_ctx* ctx, int site);
/* diagnostic: copy an internal fp32 buffer (0 z, 1 dz, 2 dz_head, 3 head partials, 4 CE partials) to dst (device) */
int eae_debug_copy(eae_ctx* ctx, int which, float* dst, long long n);
int eae_profile_read(eae_ctx* ctx, double* total_ms, long long* count);
/* same, plus the summed duration of an EMPTY event bracket recorded right after each timed one (the cost of the two event
 * records themselves; subtracting it gives the kernel's own duration, which is what rocprofv3 reports) */
int eae_profile_read2(eae_ctx* ctx, double* total_ms, double* empty_ms, long long* count);

/* ------------------------------------------------------------------ per-op entry points ---------------------- */
/* Building blocks of the fused step, exported for kernel-level parity tests.  Activations are NHWC bf16. */
typedef struct eae_src {
  const void* p0;      /* mode 0: tensor; 1: raw pre-BN tensor y; 2: masked gradient g; 3: fp32 tensor */
  const void* p1;      /* mode 2: raw pre-BN tensor y */
  const float* coef;   /* mode 1: [4][C] s,t,mean,invstd; mode 2: [3][C] A,B,C */
  int mode;            /* 0 raw, 1 BN-apply+ReLU on load, 2 BN-backward-apply on load, 3 fp32 */
} eae_src;

/* kind 0: 3x3 stride-2 pad-1 conv (aten::convolution of nn.Conv2d, R.md:292-304);
 * kind 1: 3x3 stride-2 pad-1 output_padding-1 transposed conv (nn.ConvTranspose2d, R.md:370-378).
 * wpack: bf16 [cout][9][cin].  epilogue 0: +bias, raw bf16 out, statistics partials [2][cout][ntiles] (channel-major);
 * 1: ReLU mask of (yprev, prev_coef) + BN-backward partials; 2: plain store. */
int eae_op_conv_s2(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack,
                   const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef);
/* fp8 variants of the two ops above (eae_config::quant = 1 uses them; maps must be multiples of 8 x 16 positions).
 * conv: wpack_e4m3 = OCP e4m3 bytes [cout][9][cin] of w * s_w; qs (device) = {1/s_pixel, 1/(s_pixel*s_w)}; the pixel operand is
 * converted to e4m3 (activation sources) or e5m2 (source mode 2, a gradient) in registers; amax (device, may be NULL) receives the
 * largest |staged pixel operand| as float bits.  wgrad: qs (device) = {1/s_small, 1/s_big, 1/(s_small*s_big)}. */
int eae_op_conv_s2_fp8(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack_e4m3,
                       const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef,
                       const float* qs, unsigned* amax);
int eae_op_wgrad_s2_fp8(void* stream, eae_src small_src, eae_src big_src, int cs, int cb, int B, int Hs, int Ws, float* scratch,
                        long long scratch_floats, float* dw, const float* qs);
/* eae_op_conv_s2_fp8 reporting the way the engine's launches do: amax is an array of amax_slots words (a power of two) amax_stride
 * words apart, and the workgroup of tile t reports into word (t & (amax_slots - 1)) * amax_stride (atomic maximum). */
int eae_op_conv_s2_fp8_slots(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack_e4m3,
                             const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef,
                             const float* qs, unsigned* amax, int amax_slots, int amax_stride);
/* The delayed-scaling kernel of the fp8 variant, run once on a state built for the call (every pointer is HOST memory; synchronises):
 * amax_bits [3][6][64] = the 64 reporting slots of the activation, gradient and weight maxima of the six 3x3 layers (float bits),
 * scales_in [18] = s_act[6], s_grad[6], s_w[6] before the launch; scales_out [18] the scales after it, qs_out [6][8] = per layer
 * {1/s_act, 1/(s_act s_w)}, {1/s_grad, 1/(s_grad s_w)}, {1/s_small, 1/s_big, 1/(s_small s_big), 0} of the weight gradient,
 * amax_left [3][6][64] = the slots after the launch (cleared). */
int eae_op_fp8_scales(void* stream, const unsigned* amax_bits, const float* scales_in, float* scales_out, float* qs_out,
                      unsigned* amax_left);
/* number of statistics partials per channel (= workgroups) eae_op_conv_s2 writes for this shape */
int eae_op_conv_s2_ntiles(int kind, int cin, int B, int Hin, int Win);
/* first / last layer kernels: src3_kind 0 = fp32 NCHW [B,3,H,W], 1 = bf16 NHWC4 [B,H,W,4]; out [B,H/2,W/2,32] */
int eae_op_edge_conv(void* stream, int src3_kind, const void* src3, int B, int H, int W, const void* wpack32x64 /* k = tap*4 + c */,
                     const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef);
int eae_op_edge_wgrad(void* stream, int src3_kind, const void* src3, int B, int H, int W, eae_src side, float* scratch,
                      long long scratch_floats, float* dw /*[32][3][3][3]*/);
int eae_op_deconv4_loss(void* stream, eae_src a3, int B, int Hin, int Win, const void* wjoint, const float* bias,
                        const float* x, float gscale, float* x_hat, void* g4, float* loss_part /*[ntiles][4]*/);
/* The same four edge ops for C image bands (1..16), padded to CP = 4 (C = 3), 8 (C <= 8) or 16 in the kernels:
 *   eae_op_pack_edge      : the engine's packs of a [32][C][3][3] fp32 weight (conv1's, or deconv4's [Cin][Cout] one): wpack bf16
 *                           [32][KP] with k = tap*CP + c, KP = 9*CP rounded up to 32 (64 / 96 / 160; the form eae_op_edge_conv_c takes,
 *                           deconv4's for its backward-data) and, unless wjoint is NULL, the joint deconv4 pack bf16 [4*CP][128]
 *                           (n = phase*C + co, k = nb*32 + ci; the form eae_op_deconv4_loss_c takes).  Synchronous: it allocates a
 *                           small descriptor table per call and waits for the stream (a helper for tests and tools, not a hot loop).
 *   eae_op_edge_conv_c    : src_kind 0 = fp32 NCHW [B,C,H,W], 1 = bf16 NHWC-CP [B,H,W,CP]; out [B,H/2,W/2,32]
 *   eae_op_edge_wgrad_c   : dw [32][C][3][3]; scratch >= 288*C floats per workgroup (the launch uses fewer when it is short)
 *   eae_op_deconv4_loss_c : x / x_hat fp32 NCHW [B,C,2Hin,2Win], g bf16 NHWC-CP [B,2Hin,2Win,CP] (bands >= C zero),
 *                           loss_part [ntiles][4*ceil((C+1)/4)] = {sum diff^2, sum g(c) for c < C, zeros}
 *   eae_op_sigmoid_bwd_c  : as eae_op_sigmoid_bwd, x_hat / dx_hat [B,C,H,W], g NHWC-CP, db[C]; scratch >= ceil(B*H*W/256)*4*ceil((C+1)/4) */
int eae_op_pack_edge(void* stream, const float* w, int C, void* wpack, void* wjoint);
int eae_op_edge_conv_c(void* stream, int src_kind, const void* src, int C, int B, int H, int W, const void* wpack,
                       const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef);
int eae_op_edge_wgrad_c(void* stream, int src_kind, const void* src, int C, int B, int H, int W, eae_src side, float* scratch,
                        long long scratch_floats, float* dw);
int eae_op_deconv4_loss_c(void* stream, eae_src a3, int C, int B, int Hin, int Win, const void* wjoint, const float* bias,
                          const float* x, float gscale, float* x_hat, void* g, float* loss_part);
int eae_op_sigmoid_bwd_c(void* stream, const float* x_hat, const float* dx_hat, int C, int B, int H, int W, void* g, float* db,
                         float* scratch);
/* weight gradient of a 3x3 s2 layer: dw [cs][cb][3][3] fp32 (reference layout) */
int eae_op_wgrad_s2(void* stream, eae_src small_src, eae_src big_src, int cs, int cb, int B, int Hs, int Ws, float* scratch,
                    long long scratch_floats, float* dw);
int eae_op_bn_finalize(void* stream, const float* stat_part, int ntiles, int C, long long count, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, long long* nbt, float momentum,
                       float eps, float* coef);
int eae_op_bn_eval_coef(void* stream, int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* coef);
int eae_op_bn_bwd_finalize(void* stream, const float* stat_part, int ntiles, int C, long long count, const float* gamma,
                           const float* coef_fwd, float* dgamma, float* dbeta, float* coef_bwd);
/* Latent projections (nn.Linear(256*h*w, L) R.md:309 and nn.Linear(L, 256*h*w) R.md:365) on NHWC-flattened activations
 * (feature index k' = pixel*256 + channel; the permutation to the reference's c*P+p order lives in the packed weights).
 *   eae_op_fc_splitk : out[M][N] fp32 = T(a)[M][K] . w[N][K]^T (+ bias[N]) (+ addend[M][N]); split-K in slices of 128 through
 *                      `scratch` (>= K/128 * M * N floats) and a fixed-order reduction.  a.mode 0 (bf16) or 1 (BN+ReLU on load,
 *                      coef [4][256], channel = k % 256).  N % 64 == 0, K % 128 == 0.      (enc.fc forward, dec.fc backward-data)
 *   eae_op_fc_bias_bf16 : out[M][N] bf16 = a_f32[M][K] . w[N][K]^T + bias[N]; N % 256 == 0, K % 64 == 0.   (dec.fc forward)
 *   eae_op_fc_wgrad : dw = P^T . Q over the batch, written in the REFERENCE weight layout; mode 0: P = bf16 [Bt][I], Q = fp32
 *                     [Bt][J], dw [I][J] with rows permuted back to c*Pn+p (dec.fc); mode 1: P = fp32 [Bt][I], Q = BN+ReLU source
 *                     [Bt][J], dw [I][J] with columns permuted back (enc.fc); colsum = sum_b P (bias gradient) or NULL. */
int eae_op_fc_splitk(void* stream, eae_src a, const void* w_bf16, int M, int N, int K, const float* bias, const float* addend,
                     float* scratch, long long scratch_floats, float* out);
int eae_op_fc_bias_bf16(void* stream, const float* a_f32, const void* w_bf16, int M, int N, int K, const float* bias, void* out_bf16);
int eae_op_fc_wgrad(void* stream, int mode, eae_src p, eae_src q, int Bt, int I, int J, int Pn, float* dw, float* colsum);
/* Classification head Linear(L,128)-ReLU-Linear(128,C) (R.md:423-427) fused with CrossEntropyLoss(mean) (R.md:623) and its
 * whole backward, fp32.  grads = the 4 head gradients in state-dict order (W1 [128][L], b1 [128], W2 [C][128], b2 [C], each
 * padded to a multiple of 4 floats); loss2[0] = mean CE, loss2[1] = number of correct argmax.  labels NULL: forward only.
 * scratch >= eae_op_head_scratch_floats(B, L, C). */
long long eae_op_head_scratch_floats(int B, int L, int C);
int eae_op_head_ce(void* stream, const float* z, const float* w1, const float* b1, const float* w2, const float* b2,
                   const long long* labels, int B, int L, int C, float* logits, float* dz, float* grads, float* loss2,
                   float* scratch, long long scratch_floats);
/* eae_op_head_ce with the class weights and ignore_index of eae_set_class_weights (same semantics; loss2[0] = the weighted mean,
 * loss2[1] = correct among the counted rows).  class_w == NULL and ignore_index == EAE_NO_IGNORE: the kernel and the bits of eae_op_head_ce. */
int eae_op_head_ce_w(void* stream, const float* z, const float* w1, const float* b1, const float* w2, const float* b2,
                     const long long* labels, int B, int L, int C, float* logits, float* dz, float* grads, float* loss2,
                     float* scratch, long long scratch_floats, const float* class_w, long long ignore_index);
/* Sigmoid backward for an externally supplied dL/dx_hat (autograd path): g4 = bf16 NHWC4 of dx_hat*x_hat*(1-x_hat), plus the
 * deconv4 bias gradient db[3]; x_hat, dx_hat fp32 NCHW [B,3,H,W]; scratch >= ceil(B*H*W/256)*4 floats. */
int eae_op_sigmoid_bwd(void* stream, const float* x_hat, const float* dx_hat, int B, int H, int W, void* g4, float* db,
                       float* scratch);
/* pack a [A][B][3][3] fp32 weight into bf16 p1 [A][9][B] and p2 [B][9][A] */
int eae_op_pack3x3(void* stream, const float* w, int A, int B, void* p1, void* p2);
int eae_op_adam(void* stream, float* p, const float* g, float* m, float* v, long long n, double lr, double beta1,
                double beta2, double eps, double weight_decay, long long step);

/* ------------------------------------------------------------------ input staging ------ */
/* The loader-side transforms of the reference fused on the device: train = RandomHorizontalFlip -> RandomCrop(H, padding=4)
 * -> ToTensor -> AddGaussianNoise(0, noise_std) (R.md:211-230), eval = ToTensor (R.md:232-234).  in_u8: uint8 HWC [B,H,W,3];
 * out: fp32 NCHW [B,3,H,W].  Randomness: Philox4x32-10 keyed by (seed, step) unless explicit per-image params int32 [B][3] =
 * (flip, top, left) with top,left in 0..8 and/or standard-normal noise [B,3,H,W] are supplied. */
int eae_augment(void* stream, const void* in_u8, float* out, int B, int H, int W, int train, float noise_std,
                unsigned long long seed, unsigned long long step, const int* params, const float* noise);

/* Multispectral staging (in_channels 1..16): the same transform for a dataset kept in DEVICE memory, gathered by index.
 * src: uint8 (elem_bytes 1) or uint16 (elem_bytes 2) planar [N,C,H,W]; index: int64 [B] of images in 0..N-1, or NULL for images
 * 0..B-1 (an index outside 0..N-1 gives NaN for that image); divisor: fp32 [C] on the device; out: fp32 NCHW [B,C,H,W].
 * Per image: flip -> pad-4 crop (padding reads 0) -> v / divisor[c] (a true division, as ToTensor's) -> + noise_std * N(0,1)
 * (train = 0: the division only).  Randomness as eae_augment: Philox keyed by (seed, step), or explicit params int32 [B][3] /
 * noise [B,C,H,W].  With C = 3, uint8 data, divisor 255 and the same explicit draws, out is eae_augment's (on CHW data). */
int eae_stage_bands(void* stream, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index, int B,
                    const float* divisor, float* out, int train, float noise_std, unsigned long long seed, unsigned long long step,
                    const int* params, const float* noise);

/* ------------------------------------------------------------------ external MLP (R.md:2549-2566) ---------- */
typedef struct eae_mlp eae_mlp;
#define EAE_MLP_NPARAMS 10
int eae_mlp_layout(int input_dim, int num_classes, long long* param_off /*[11]*/, long long* bn_off /*[5]*/);
int eae_mlp_create(int input_dim, int num_classes, int max_batch, eae_mlp** out);
/* The classifier with a configurable architecture: n_hidden in 1..4 hidden layers of widths hidden[l] in 1..512, each
 * Linear -> BatchNorm1d -> ReLU -> Dropout(p_drop[l]) (no Dropout where p_drop[l] == 0; rates in [0, 1)), then Linear(last, C).
 * eae_mlp_layout_ex: param_off[4 * n_hidden + 3] = the offsets of W, b, gamma, beta of each hidden layer, the last W and b, then the
 * total (each tensor rounded up to 4 floats); bn_off[2 * n_hidden + 1] = running mean, running variance of each layer, then the total.
 * hidden = {128, 64} gives eae_mlp_layout's tables.  eae_mlp_create_ex yields the same opaque handle, served by the layer-table
 * kernel whatever the architecture (eae_mlp_create keeps the fixed 128 / 64 kernel); every eae_mlp_* entry point below and
 * eae_scene_classify* accept it with these differences: bn_nbt has one word per hidden layer, and drop_mask holds the keep masks
 * [B][hidden[l]] of the layers with p_drop[l] > 0, in layer order, back to back.  Hidden layer l draws its mask from Philox4x32-10 with
 * key (seed lo, seed hi) and counter (b * hidden[l] + j, step lo, step hi, 0x9E3779B9 + l).  Arguments out of range: EAE_ERR_ARG,
 * before anything is allocated. */
int eae_mlp_layout_ex(int input_dim, int num_classes, int n_hidden, const int* hidden, long long* param_off, long long* bn_off);
int eae_mlp_create_ex(int input_dim, int num_classes, int n_hidden, const int* hidden, const float* p_drop, int max_batch,
                      eae_mlp** out);
int eae_mlp_destroy(eae_mlp* m);
int eae_mlp_bind(eae_mlp* m, float* params, float* grads, float* adam_m, float* adam_v, float* bn_running,
                 long long* bn_nbt);
int eae_mlp_set_adam_step(eae_mlp* m, long long step);
/* logits = clf(xb) (R.md:2643 train mode / 2663, 3182 eval mode); dropout mask = Philox(seed, step counter) or the
 * caller-supplied keep-mask [B][128] (fp32 0/1) when drop_mask != NULL. */
int eae_mlp_forward(eae_mlp* m, void* stream, const float* x, int B, int train, unsigned long long seed,
                    const float* drop_mask, float* logits);
/* loss.backward() for a torch-side loss on the logits of the preceding train-mode eae_mlp_forward of the same batch
 * (R.md:2644-2645); gradients land in the gradient arena. */
int eae_mlp_backward(eae_mlp* m, void* stream, const float* x, int B, unsigned long long seed, const float* drop_mask,
                     const float* dlogits);
/* one iteration of R.md:2641-2649: zero_grad, forward, CE, backward, Adam(lr, weight_decay);
 * stats: float[8] += loss*B, B, #correct. */
int eae_mlp_train_step(eae_mlp* m, void* stream, const float* x, const long long* labels, int B, float lr,
                       float weight_decay, unsigned long long seed, const float* drop_mask, float* logits, float* stats);
/* forward + CE + accuracy bookkeeping without update (validation / test loops, R.md:2660-2668, 2689-2695) */
int eae_mlp_eval_step(eae_mlp* m, void* stream, const float* x, const long long* labels, int B, float* logits,
                      float* stats);
/* eae_set_class_weights for the MLP: reaches eae_mlp_train_step and eae_mlp_eval_step (eae_mlp_backward with external dlogits is
 * unaffected).  Same semantics and the same W == 0 deviation; BatchNorm statistics stay over all rows of the batch, as in torch.
 * stats[0] += CE * B, stats[1] += B (all rows), stats[2] += correct among the counted rows; in eval mode every 64-row block sums W
 * over the whole batch in the same fixed order. */
int eae_mlp_set_class_weights(eae_mlp* m, const float* weights, long long ignore_index);
/* eae_set_valid_counter for the MLP: with the feature on, eae_mlp_train_step / eae_mlp_eval_step with stats != NULL add the counted
 * rows of the batch to *counter (device int64, caller-owned, or NULL). */
int eae_mlp_set_valid_counter(eae_mlp* m, long long* counter);

/* ------------------------------------------------------------------ scene classification ---------- */
/* These entry points extend beyond the reference, which has no notebook lines for applying the pipeline to a whole scene.
 * A model of size P x P (image_h == image_w == patch) runs over windows of a planar scene [C][H][W] held on the device.  Windows
 * are placed at stride S (1 <= S <= P) on both axes; only whole windows are used: nH = (H - P) / S + 1, nW = (W - P) / S + 1.
 * Window n = i * nW + j starts at pixel (i * S, j * S).  The input value is (float)v / divisor[c], the eval-mode expression of
 * eae_stage_bands.  Offsets are 64-bit: scenes may exceed 2^31 elements. */
#define EAE_SCENE_U8 0
#define EAE_SCENE_U16 1
#define EAE_SCENE_F32 2
typedef struct eae_scene {
  const void* data;        /* [C][H][W] on the device, dtype EAE_SCENE_* */
  const float* divisor;    /* [C] on the device */
  int dtype, C, H, W;
  int patch, stride;       /* P, S */
  int border;              /* EAE_BORDER_*; every field from here on zero: the grid of whole windows described above */
  int pad_top, pad_bottom, pad_left, pad_right;
  float fill;              /* the stored value of an EAE_BORDER_CONSTANT pixel */
} eae_scene;
/* Border modes.  With border != EAE_BORDER_NONE the window grid is laid over the VIRTUAL scene of (pad_top + H + pad_bottom) x
 * (pad_left + W + pad_right) pixels: nH = (pad_top + H + pad_bottom - P) / S + 1, nW alike, and window (i, j) starts at scene pixel
 * (i * S - pad_top, j * S - pad_left).  Every call that takes an eae_scene returns bitwise what it returns for border = NONE on
 * numpy.pad(scene, ((0, 0), (pad_top, pad_bottom), (pad_left, pad_right)), mode) (and the mask padded alike, with 0 in constant mode);
 * no padded copy is made: the kernels resolve a virtual pixel when they load it.  With s = v - pad the source index of virtual
 * coordinate v on an axis of length n is s inside [0, n); EDGE clamps s to [0, n - 1]; REFLECT takes -s for s < 0 and 2 (n - 1) - s
 * for s >= n (numpy's "reflect": the edge pixel is not repeated); a CONSTANT pixel has the value (float)fill / divisor[c], and is
 * invalid for eae_scene_invalid_counts when fill matches the nodata value.  Replicated and mirrored pixels are as valid as their source.
 * Rejected (EAE_ERR_ARG): a pad outside 0..P - 1, a virtual size below P, REFLECT with pad_top or pad_bottom > H - 1 or pad_left or
 * pad_right > W - 1 (one reflection only), a fill of a uint8 / uint16 scene that is no integer of the dtype's range, an unknown mode, and
 * border = NONE with a non-zero pad.  The real scene may be smaller than P.  Window and cell maps keep their shapes, of the virtual
 * grid; eae_scene_reconstruct writes the REAL scene (see there). */
#define EAE_BORDER_NONE 0
#define EAE_BORDER_CONSTANT 1
#define EAE_BORDER_EDGE 2
#define EAE_BORDER_REFLECT 3
/* fp32 NCHW [B,C,P,P] of windows first_window .. first_window + B - 1: bitwise eae_stage_bands(train = 0) on the same windows.  No
 * model runs, so P is any positive size here (every call that runs a model wants a multiple of 64, its image size). */
int eae_scene_windows(void* stream, const eae_scene* scene, long long first_window, int B, float* out);
/* Eval-mode encoder over windows first_window .. + B - 1 (any B: split at max_batch inside), conv1 reading the scene directly
 * (zero conv padding at every window border): z [B][L].  Invalidates the resident forward (a later backward is refused). */
int eae_scene_encode(eae_ctx* ctx, void* stream, const eae_scene* scene, long long first_window, int B, float* z);
/* Encoder -> MLP (eval mode) over windows first_window .. + count - 1, in batches of at most max_batch, no host synchronisation.
 * probs [K][nH * nW] (softmax) and labels [nH * nW] (int64 argmax, first maximum) receive the windows' columns; the MLP's logits
 * are those of eae_mlp_eval_step.  Rejects quant = 1 contexts, C != in_channels, patch != image size, a scene smaller than P, S
 * outside 1..P and a NULL divisor.  Invalidates the resident forward like eae_encoder_forward. */
int eae_scene_classify(eae_ctx* ctx, eae_mlp* mlp, void* stream, const eae_scene* scene, long long first_window, long long count,
                       float* probs, long long* labels);
/* Blending (S divides P, k = P / S): cell map [K][nH + k - 1][nW + k - 1] of S x S cells, each the mean of probs [K][nH][nW] over
 * the windows that cover it; cell_labels [nH + k - 1][nW + k - 1] = argmax of the blended map (int64). */
int eae_scene_blend(void* stream, const float* probs, int K, int nH, int nW, int k, float* cell_probs, long long* cell_labels);

/* Nodata and masked windows.  Pixel (y, x) is invalid when it matches the nodata value (rule EAE_INVALID_ALL: every band equals it,
 * rasterio's dataset-mask convention; EAE_INVALID_ANY: at least one band does) or when mask[y * W + x] != 0 (mask: uint8 [H][W] on the
 * device, or NULL).  nodata_mode EAE_NODATA_NONE ignores nodata; EAE_NODATA_VALUE compares with nodata (for uint8 / uint16 scenes an
 * integer in the dtype's range, else rejected; for fp32 by ==); EAE_NODATA_NAN matches NaN (fp32 scenes only).
 * counts [nH][nW] (int32) = invalid pixels of each window.  rows is scratch of Hg * nW ints, Hg = (nH - 1) * S + P (with a border:
 * nH and nW of the virtual grid, so Hg is the virtual extent).  Every scene element and mask byte inside the grid's extent is read
 * once (with a border: once for every virtual pixel inside the extent that resolves to it); the divisor is not
 * read.  The patch size must be at most 4080. */
#define EAE_NODATA_NONE 0
#define EAE_NODATA_VALUE 1
#define EAE_NODATA_NAN 2
#define EAE_INVALID_ALL 0
#define EAE_INVALID_ANY 1
int eae_scene_invalid_counts(void* stream, const eae_scene* scene, int nodata_mode, float nodata, int rule,
                             const unsigned char* mask, int* rows, int* counts);
/* Stable compaction: windows[0 .. *count) = the ascending ids n of counts [n_windows] with counts[n] <= threshold; *count (int64) is
 * written on the device.  windows must hold n_windows ids.  One workgroup, deterministic; no host synchronisation. */
int eae_scene_select(void* stream, const int* counts, long long n_windows, int threshold, long long* windows, long long* count);
/* Index-driven forms of eae_scene_encode / eae_scene_classify: the windows are the ids windows[0 .. count) (device int64, any order,
 * duplicates allowed), count > 0 passed from the host.  encode: z [count][L] in list order.  classify: probs and labels receive the
 * listed windows' columns; every other column is left as the caller filled it.  The ids are not checked on the host (no
 * synchronisation): the kernels read an id outside [0, nH * nW) as an all-zero window and write nothing for it, a guard only; callers
 * must pass ids inside the grid. */
int eae_scene_encode_windows(eae_ctx* ctx, void* stream, const eae_scene* scene, const long long* windows, long long count, float* z);
int eae_scene_classify_windows(eae_ctx* ctx, eae_mlp* mlp, void* stream, const eae_scene* scene, const long long* windows,
                               long long count, float* probs, long long* labels);
/* eae_scene_blend over the valid windows only (labels [nH][nW] >= 0, as the index-driven classify leaves behind when labels are
 * pre-filled with -1): each cell is the mean over its valid covering windows (same summation order, divisor = their float count);
 * a cell without a valid covering window gets probabilities 0 and label -1.  With every window valid it is bitwise eae_scene_blend. */
int eae_scene_blend_valid(void* stream, const float* probs, const long long* labels, int K, int nH, int nW, int k, float* cell_probs,
                          long long* cell_labels);


/* Scene reconstruction (eval mode, bf16 contexts, both halves bound): encoder -> decoder over windows of the scene, with deconv4's
 * MSE target read from the scene itself by the expression conv1 reads it with, (float)v / divisor[c]: no [B,C,P,P] batch of windows,
 * of x_hat or of gradients is written.  x_hat is bitwise eae_decoder_forward(train = 0) on the windows' latents.  All three split at
 * max_batch inside, synchronise nothing on the host, apply the checks of eae_scene_encode / eae_scene_encode_windows and invalidate
 * the resident forward.  The sums are deterministic (fixed order, no atomics) and do not depend on how windows are batched.
 *
 * eae_set_halves: which halves of the model the bound arenas hold (default: both).  The engine of a stand-alone Encoder or Decoder
 * binds arenas whose other half is zero; the three calls below return EAE_ERR_STATE unless both halves are declared present.
 *
 * eae_scene_recon_error: err [nH * nW] receives, at the ids of windows first_window .. + count - 1, the mean of (x_hat - x)^2 over
 * the window's C * P * P elements; band_err [C][nH * nW] (or NULL) the mean over each band's P * P.
 * eae_scene_recon_error_windows: the same for the ids windows[0 .. count) (device int64, any order, duplicates allowed); every other
 * entry of err / band_err is left as the caller filled it.  An id outside [0, nH * nW) is read as zeros and nothing is written for it
 * (a guard only, as for eae_scene_encode_windows).
 *
 * eae_scene_reconstruct: the stitched reconstruction recon [C][Hg][Wg] (fp32, the units of v / divisor) of the grid's extent, Hg =
 * (nH - 1) * S + P, Wg alike, and (residual != NULL) residual [Hg][Wg], the mean over the bands of (x_hat - x)^2 of each pixel.
 * Every pixel of the extent is OWNED by exactly one window and is written by that window alone (plain stores, no accumulation): with
 * m = (P - S) / 2, window row i owns scene rows [i * S + m, i * S + m + S), extended to 0 for i = 0 and to Hg for i = nH - 1; columns
 * alike.  P - S must be even.  windows == NULL: windows 0 .. count - 1 (count = nH * nW: the whole extent); else the listed ids, and
 * the pixels owned by other windows are left as the caller filled them.  With a border the spans are those of the virtual grid and
 * recon is [C][H][W], residual [H][W], of the real scene: a window stores the pixels it owns that are real ones, and every real
 * pixel has an owner because the virtual extent covers the scene when the pads are those of a full grid. */
int eae_set_halves(eae_ctx* ctx, int encoder, int decoder);
int eae_scene_recon_error(eae_ctx* ctx, void* stream, const eae_scene* scene, long long first_window, long long count, float* err,
                          float* band_err);
int eae_scene_recon_error_windows(eae_ctx* ctx, void* stream, const eae_scene* scene, const long long* windows, long long count,
                                  float* err, float* band_err);
int eae_scene_reconstruct(eae_ctx* ctx, void* stream, const eae_scene* scene, const long long* windows, long long count, float* recon,
                          float* residual);

/* ------------------------------------------------------------------ training from a scene ---------- */
/* The loader side of training, from a scene and a label raster held on the device: no [N,C,P,P] patch dataset is cut (with
 * overlapping windows that dataset is (P/S)^2 times the scene) and no per-patch label is made on the host.  No model runs here: P is
 * any positive size, S in 1..P, C in 1..16, the grid is that of whole windows (border = EAE_BORDER_NONE; any other mode is rejected).
 *
 * eae_scene_stage_windows: out [B,C,P,P] (fp32 NCHW) = the transform of eae_stage_bands applied to windows[0 .. B) (device int64 ids of
 * the grid, any order, duplicates allowed): flip -> pad-4 crop -> (float)v / divisor[c] (a true division) -> fmaf(noise_std, n, v).
 * (flip, top, left) of batch position b and the noise come from params int32 [B][3] / noise [B,C,P,P] when given, else from the
 * Philox stream of eae_stage_bands, keyed alike (batch position b; flat pixel index over [B][P][P]; band group; seed; step): the two
 * calls draw the same values.  train = 0: the division only, bitwise eae_scene_windows.  With the window's origin (oy, ox),
 * sy = y + top - 4, sx = x + left - 4 and, after a flip, sx <- P - 1 - sx:
 *   EAE_CROP_WINDOW: a position with sy or the unflipped sx outside [0, P) reads 0, as in eae_stage_bands; out is bitwise
 *     eae_stage_bands on the materialised windows [B,C,P,P] with the same arguments.
 *   EAE_CROP_SCENE: the value is scene pixel (oy + sy, ox + sx) wherever that pixel lies inside the scene, 0 outside it: the crop
 *     jitters the window over its real neighbourhood and no black frame appears.  This is EAE_CROP_WINDOW with params (flip, 4, 4) on
 *     the window of origin (oy + top - 4, ox + (flip ? -(left - 4) : left - 4)) cut from the scene zero-padded by 4.
 * An id outside [0, nH * nW) gives NaN for that image and reads nothing (as an index outside 0..N-1 does in eae_stage_bands).  Rejected
 * (EAE_ERR_ARG): what eae_scene_windows rejects, a border mode, NULL windows / out, B <= 0, an unknown crop.  No host synchronisation. */
#define EAE_CROP_WINDOW 0
#define EAE_CROP_SCENE 1
int eae_scene_stage_windows(void* stream, const eae_scene* scene, const long long* windows, int B, float* out, int train,
                            float noise_std, unsigned long long seed, unsigned long long step, const int* params, const float* noise,
                            int crop);
/* ------------------------------------------------------------------ augmentation policy ------------ */
/* A stronger training transform for the three staging calls (eae_augment, eae_stage_bands, eae_scene_stage_windows): the eight
 * rotations and flips of the square (D4), a small rotation and scale about the centre, and a per-band gain and offset.  In the
 * image's direction:  flip -> pad-4 crop -> quarter turns -> small rotation and scale -> / divisor[c] -> gain and offset -> noise.
 *
 *   dihedral   != 0: rot in {0, 1, 2, 3} quarter turns per image, counter-clockwise as np.rot90; with the flip, all of D4.  H == W.
 *   rotate     theta_max in degrees, >= 0 (at most 180): theta uniform in [-theta_max, theta_max); positive turns as np.rot90 does.
 *   scale      s in [0, 1): sigma uniform in [1 - s, 1 + s); sigma > 1 enlarges the content.
 *   gain       in [0, 1): one g per image, uniform in [1 - gain, 1 + gain).
 *   band_gain  in [0, 1): one g_c per image and band, uniform in [1 - band_gain, 1 + band_gain).
 *   offset     >= 0: one o_c per image and band, uniform in [-offset, offset), in output units (after the divisor).
 *   draw_mode  where the per-image draws are made: 0 = chosen by the image size, 1 = by every thread, 2 = once per workgroup, through
 *              LDS (needs H * W >= 256).  The values do not depend on it.
 *
 * An output pixel (x, y) finds its value as follows, with cx = (W - 1) / 2, cy = (H - 1) / 2 and a = cos(theta) / sigma,
 * b = sin(theta) / sigma (both ranges 0: this step does not exist, X = x, Y = y):
 *   u = x - cx, v = y - cy;   X = fl(fma(a, u, -fl(b v)) + cx),   Y = fl(fma(b, u, fl(a v)) + cy)              (fp32, as written)
 *   the value is the bilinear interpolation, in fp32, of the RAW values I(floor Y + {0, 1}, floor X + {0, 1}) with the fractions of
 *   X and Y: lerp(p, q, t) = fma(t, fl(q - p), p), along x first, then along y, and ONE division by divisor[c] afterwards.  With
 *   zero fractions that is bitwise I itself, the integer path.
 *   I(yo, xo), for integers of any size, is the pixel the integer path reads for output position (xo, yo):
 *     (U, V) = (xo - cx, yo - cy) turned rot times by (U, V) <- (-V, U)                                          (exact)
 *     sx = U + cx + left - 4, sy = V + cy + top - 4;  eae_augment / eae_stage_bands / EAE_CROP_WINDOW: 0 unless 0 <= sy < H and
 *     0 <= sx < W (the unflipped sx);  then sx <- W - 1 - sx when flipped;  EAE_CROP_SCENE: scene pixel (oy + sy, ox + sx), 0 outside
 *     the scene.  The window's origin is added to these integers, never to X or Y: the result does not depend on where in a scene
 *     the window lies.  Every tap has its own inside test.
 *   v = I / divisor[c];   v <- fma(v, fl(g g_c), o_c) (when gain, band_gain or offset is set, or radio is given);
 *   v <- fma(noise_std, n, v) as in eae_stage_bands.
 * Random draws: (flip, top, left) are those of eae_stage_bands for the same (b, seed, step), whatever the policy; rot = w3 >> 30 of
 * that Philox call.  The others use calls of their own, keyed (~seed lo, seed hi), counter (b, tag + (c0 << 16), step lo, step hi):
 * tag 0xA061 (theta in degrees, sigma, g from words 0, 1, 2), 0xA062 (g_c of bands c0 .. c0 + 3), 0xA063 (o_c likewise), c0 in
 * {0, 4, 8, 12}; a uniform is fma((w >> 8) 2^-24, hi - lo, lo), and theta in radians is fl(theta * fl(pi / 180)).
 *
 * The three calls take the policy (NULL = none) and, for parity tests, explicit draws that replace the policy's (each may be NULL):
 *   geom   int32 [B][4] = (flip, top, left, rot), rot in 0..3 (H == W)        affine float [B][2] = (a, b)
 *   radio  float [B][C][2] = (gain, offset): v <- fma(v, gain, offset)         noise, as in the plain calls
 * With train = 0, or with a NULL or all-zero policy and no explicit geom / affine / radio, a call is the plain one (bitwise).  An id
 * or index outside its range still gives a NaN image and reads nothing.  Rejected (EAE_ERR_ARG): what the plain call rejects; a
 * negative or non-finite range; rotate > 180; scale, gain or band_gain >= 1; dihedral or geom with H != W; an unknown draw_mode, or
 * draw_mode 2 with H * W < 256. */
typedef struct eae_aug {
  int dihedral;
  float rotate, scale, gain, band_gain, offset;
  int draw_mode;
} eae_aug;
int eae_augment_aug(void* stream, const void* in_u8, float* out, int B, int H, int W, int train, float noise_std,
                    unsigned long long seed, unsigned long long step, const eae_aug* aug, const int* geom, const float* affine,
                    const float* radio, const float* noise);
int eae_stage_bands_aug(void* stream, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index, int B,
                        const float* divisor, float* out, int train, float noise_std, unsigned long long seed, unsigned long long step,
                        const eae_aug* aug, const int* geom, const float* affine, const float* radio, const float* noise);
int eae_scene_stage_windows_aug(void* stream, const eae_scene* scene, const long long* windows, int B, float* out, int train,
                                float noise_std, unsigned long long seed, unsigned long long step, const eae_aug* aug, const int* geom,
                                const float* affine, const float* radio, const float* noise, int crop);

/* A label for every window of the grid of whole P x P windows at stride S over a label raster [H][W] on the device, uint8
 * (elem_bytes 1) or int32 (4).  A pixel is labelled when its value is in [0, K), K in 1..64; every other value (255, negatives,
 * >= K) is unlabelled.  For window n: label[n] (int64) = the class with the most labelled pixels, the lowest class on a tie, -1 when
 * the window has none; count[n] (int32, or NULL) = that class's pixels (0 without one); labelled[n] (int32, or NULL) = the labelled
 * pixels.  Integer counts: exact, and identical from run to run.  The patch size must be at most 4080. */
int eae_scene_window_labels(void* stream, const void* raster, int elem_bytes, int H, int W, int patch, int stride, int K,
                            long long* label, int* count, int* labelled);

/* ------------------------------------------------------------------ accuracy assessment ------------ */
/* Confusion counts of a class map against a label raster, pixel by pixel, both on the device.  truth [H][W] is uint8 (elem_bytes 1)
 * or int32 (4), as in eae_scene_window_labels; pred is an int64 [cH][cW] map of cell x cell cells (the labels of
 * eae_scene_classify: cell = the patch size; the cell labels of eae_scene_blend: cell = the stride; cell = 1: a map of the raster's
 * own resolution); mask is NULL or uint8 [H][W]; counts is int64 [(K+1)][(K+1)], K in 1..64.
 *   Pixel (y, x) lies in cell ((y + oy) / cell, (x + ox) / cell): (oy, ox) = the leading pads of a border grid, 0 without one.
 *   A pixel with mask[y][x] != 0 is skipped.  Every other pixel adds 1 to counts[r][c]:
 *     r = truth[y][x] when that is in [0, K), else K (unlabelled);
 *     c = the cell's pred value when the cell lies inside the map and the value is in [0, K), else K (not classified: the -1 of an
 *         invalid or unlisted window, any value outside [0, K), a pixel the map does not cover).
 *   So the entries sum to the number of unmasked pixels.  accumulate = 0: counts is cleared first, on the stream; accumulate = 1:
 *   the call adds to what counts holds (assessment over several scenes).
 * Integer counting throughout (LDS tables per workgroup, 64-bit global adds): exact, and identical from run to run.  The raster
 * and the mask are read once; no per-pixel copy of the map is made.  Rejected (EAE_ERR_ARG): a NULL truth, pred or counts, any
 * other elem_bytes, K outside 1..64, cell < 1, a negative oy or ox, an empty raster or map, accumulate outside 0..1. */
int eae_scene_confusion(void* stream, const void* truth, int elem_bytes, int H, int W, const long long* pred, int cH, int cW, int cell,
                        int oy, int ox, const unsigned char* mask, int K, int accumulate, long long* counts);

/* ------------------------------------------------------------------ latent clustering -------------- */
/* k-means over the latents eae_scene_encode returns (no reference counterpart: the notebook classifies with a trained MLP only).  The
 * two halves of a Lloyd iteration, stateless: z [N][L] fp32 row-major, centroids [K][L] fp32, labels int64; 1 <= L <= 256,
 * 1 <= K <= 256, 1 <= N < 2^31, anything else or a NULL required pointer is EAE_ERR_ARG.  Nothing synchronises the host.
 *
 * eae_kmeans_assign: labels[n] = argmin_k ||z_n - c_k||^2, compared as score_k = ||c_k||^2 - 2 z_n . c_k in fp32 (fp32 operands and
 * accumulation, the f32-input MFMA: a k-ordered fma chain); the lowest k wins a tie, exactly (equal centroids give equal scores).
 * dist (or NULL): dist[n] = max(0, score + ||z_n||^2), the fp32 squared distance to the chosen centroid.  A row that holds a NaN or an
 * Inf gets label -1 and dist NaN.  have_prev != 0: labels is read first as the previous labelling and *changed (device, or NULL)
 * receives the exact number of rows whose label differs; have_prev == 0: labels is written only and changed is not touched.  No N x K
 * matrix is written, and a row's result does not depend on the launch geometry or on the other rows.
 *
 * eae_kmeans_update: counts[k] = the exact number of rows with label k; centroids[k] = the fp32 mean of those rows, unchanged when
 * there are none.  Labels outside [0, K) (-1 included) are skipped, values and all.  Bitwise identical from run to run: the sums are a
 * one-hot product on the same MFMA, per-workgroup partial sums go to `workspace` and a second kernel adds them in one fixed order and
 * divides; no float atomics (the counts are integer adds).  workspace: device memory of at least
 * eae_kmeans_workspace_bytes(N, L, K) bytes (host only; < 0 on bad arguments), contents irrelevant on entry; NULL or too small is
 * EAE_ERR_ARG and nothing is launched.  A row with a non-finite value must not carry a label in [0, K): 0 x Inf is NaN, and it would
 * reach every cluster of its workgroup's partial, not only its own (eae_kmeans_assign labels such rows -1). */
long long eae_kmeans_workspace_bytes(long long N, int L, int K);
int eae_kmeans_assign(void* stream, const float* z, long long N, int L, const float* centroids, int K, long long* labels, int have_prev,
                      float* dist, long long* changed);
int eae_kmeans_update(void* stream, const float* z, long long N, int L, const long long* labels, int K, float* centroids,
                      long long* counts, void* workspace, long long workspace_bytes);

/* ------------------------------------------------------------------ latent neighbours -------------- */
/* Nearest-neighbour search over latents (no reference counterpart): the k nearest rows of bank [M][L] for every row of q [Nq][L],
 * both fp32 row-major; idx int64 [Nq][k]; dist fp32 [Nq][k] or NULL.  1 <= L <= 256, 1 <= k <= 32, 1 <= Nq, M < 2^31, self_offset
 * >= -1.  Stateless; nothing synchronises the host.  Anything outside these limits, a NULL q, bank or idx, or a workspace that is
 * NULL or too small where a non-zero size is required is EAE_ERR_ARG, and nothing is launched.
 *
 * Scores: s(n, m) = ||b_m||^2 - 2 q_n . b_m in fp32, eae_kmeans_assign's expression: the dot product on the f32-input MFMA (a k-ordered
 * fma chain over L), the norm a sequential fma chain, s = fma(-2, dot, norm).  A pair's score depends on the two rows alone, not on
 * where they sit in a tile, on the grid or on the bank split.
 * Selection: row n of idx holds the k bank rows with the smallest (s, m) in lexicographic order, ascending: equal scores are ordered
 * by ascending bank index, exactly (duplicate bank rows give bitwise equal scores).  dist[n][j] = max(0, s + ||q_n||^2), the fp32
 * squared distance (||q_n||^2: the same sequential chain).
 * A bank row that holds a NaN or an Inf is never returned.  A query row that holds one gets idx -1 and dist NaN in all k slots.  When
 * fewer than k bank rows are eligible the tail slots hold -1 and NaN.  UNDEFINED: finite rows whose squared norm overflows fp32 (as
 * built they are treated like non-finite rows; do not rely on it).
 * self_offset >= 0 makes query n ineligible to match bank row n + self_offset (leave-one-out with q == bank: 0; queries that are the
 * contiguous slice bank[o : o + Nq]: o); -1 disables it.
 * Geometry: a function of (Nq, M, L, k) alone, no device query.  No Nq x M array is written anywhere.  When the query tiles alone
 * cannot fill the device the bank is cut into eae_knn_slices(...) = S > 1 slices: every (query tile, slice) workgroup writes its
 * partial top-k to `workspace` (eae_knn_workspace_bytes(...) bytes of device memory, contents irrelevant on entry) and a second
 * kernel merges the S lists of each row by the same (s, m) order.  That order is total, so the result is bitwise independent of S.
 * With S == 1 the search kernel writes idx / dist directly, eae_knn_workspace_bytes is 0 and workspace may be NULL.
 * eae_knn_workspace_bytes / eae_knn_slices are host only and return < 0 on bad arguments. */
long long eae_knn_workspace_bytes(long long Nq, long long M, int L, int k);
int eae_knn_slices(long long Nq, long long M, int L, int k);
int eae_knn_search(void* stream, const float* q, long long Nq, const float* bank, long long M, int L, int k, long long self_offset,
                   long long* idx, float* dist, void* workspace, long long workspace_bytes);

/* ------------------------------------------------------------------ latent validity ---------------- */
/* Sums of distances from query rows to the bank rows of every class (no reference counterpart): what the silhouette coefficient and a
 * table of class separation are made of.  q [Nq][L] and bank [M][L] fp32 row-major; the bank is SORTED BY CLASS: rows seg[c] ..
 * seg[c+1]-1 belong to class c, seg int64 [K+1] on the device with 0 <= seg[0] <= ... <= seg[K] <= M (values outside [0, M] are
 * clamped on the device: nothing outside the bank is read).  Rows outside [seg[0], seg[K]) belong to no class and are never read into
 * a sum, whatever they hold.  1 <= L <= 256, 1 <= K <= 256, 1 <= Nq, M < 2^31, metric 0 (Euclidean) or 1 (squared Euclidean);
 * anything else, a NULL q, bank, seg or sums, or a workspace that is NULL or too small where a non-zero size is required is
 * EAE_ERR_ARG, and nothing is launched.  Stateless; nothing synchronises the host.
 *
 * sums[n][c] = sum over the rows m of class c, m != self_pos[n], of d(q_n, b_m), fp32 [Nq][K].
 * d^2 = max(0, fma(-2, q_n . b_m, ||b_m||^2) + ||q_n||^2), eae_knn_search's expression: the dot product on the f32-input MFMA (a
 * k-ordered fma chain over L), the norms sequential fma chains; d = sqrtf(d^2) under metric 0, d = d^2 under metric 1.  Each lane of
 * the kernel adds its distances to one fp32 running sum in a fixed order, partial sums are added in one fixed order, and there are
 * no float atomics: the result is bitwise identical from run to run for the same arguments.  An empty class gives 0.
 * self_pos (device int64 [Nq], or NULL for none): the bank row, in the sorted order, that is query n itself and is left out of its
 * sums; -1 for none.
 * A query row that holds a NaN or an Inf gets a row of NaN.  Bank rows inside a segment must be finite (a precondition, as for
 * eae_kmeans_update; such a row would turn the sums of its class into NaN or Inf).  UNDEFINED: finite rows whose squared norm
 * overflows fp32.
 * Geometry: a function of (Nq, M, L, K) alone -- seg and self_pos are device data.  No Nq x M array is written anywhere.  When the
 * query tiles alone cannot fill the device a class's segment is walked by S > 1 workgroups, whose partial sums go to `workspace`
 * (eae_class_dist_workspace_bytes(...) bytes of device memory, contents irrelevant on entry) and are added by a second kernel in
 * ascending slice order; otherwise eae_class_dist_workspace_bytes is 0 and workspace may be NULL.
 * eae_class_dist_workspace_bytes is host only and returns < 0 on bad arguments. */
long long eae_class_dist_workspace_bytes(long long Nq, long long M, int L, int K);
int eae_class_dist_sums(void* stream, const float* q, long long Nq, const float* bank, long long M, int L, const long long* seg, int K,
                        const long long* self_pos, int metric, float* sums, void* workspace, long long workspace_bytes);

/* ------------------------------------------------------------------ latent Gaussian models --------- */
/* The two kernels of a Gaussian maximum-likelihood classifier over latents (no reference counterpart): per-class scatter matrices and
 * per-class quadratic forms.  z [N][L] fp32 row-major; 1 <= L <= 256, 1 <= K <= 256, 1 <= N < 2^31; anything else or a NULL required
 * pointer is EAE_ERR_ARG and nothing is launched.  Stateless; nothing synchronises the host.
 *
 * eae_class_scatter: scatter[k][i][j] = sum over the rows n of class k of (z_n[i] - means[k][i]) (z_n[j] - means[k][j]), fp32
 * [K][L][L]; means fp32 [K][L] is an input.  The rows come GROUPED BY CLASS: order int64 [N] holds row indices, and positions
 * seg[k] .. seg[k+1]-1 of it are the rows of class k (seg int64 [K+1] on the device, values clamped into [0, N]).  A row takes part
 * only if labels[row] == k as well (labels int64 [N]), and an entry of order outside [0, N) is skipped: labels outside [0, K) are
 * never summed, and nothing outside z is read.  z - m is one fp32 subtraction, the products accumulate on the f32-input MFMA, two rows
 * an instruction, in the order of `order`.  Only the tiles with i-tile <= j-tile are computed; per-chunk partial tiles go to
 * `workspace` and a second kernel adds them in ascending chunk order and writes every element and its mirror image from one register:
 * scatter[k] is bitwise symmetric, every element of the output is written (zeros for a class without rows), there are no float atomics
 * and the result is bitwise identical from run to run.  The geometry is a function of (N, L, K) alone.  workspace: device memory of at
 * least eae_class_scatter_workspace_bytes(N, L, K) bytes (host only; < 0 on bad arguments), contents irrelevant on entry; NULL or too
 * small is EAE_ERR_ARG.  Rows that take part must be finite (a precondition, as for eae_kmeans_update).
 *
 * eae_gauss_score: d_k(n) = || W_k^T (z_n - mu_k) ||^2 and score_k(n) = d_k(n) + offset[k] for every row and class.  mu fp32 [K][L],
 * offset fp32 [K], W fp32: class k's [L][L] matrix starts at element k * w_stride, w_stride = L * L, or 0 for one matrix shared by all
 * classes (anything else is EAE_ERR_ARG).  z - mu is one fp32 subtraction, u_j = sum_l W[l][j] (z - mu)[l] an l-ordered fma chain on
 * the f32-input MFMA, d the sum of the squares in one fixed order.  offset[k] == +inf marks class k as absent: its score is +inf and
 * it is never chosen.
 *   labels [N] int64: the argmin of the score, the lowest k on a tie (equal classes give equal scores); -1 for a row that holds a NaN
 *                     or an Inf, or when no class has a score below +inf.
 *   maha   [N] fp32 or NULL: max(0, d) of the chosen class; NaN for a -1 row.
 *   best   [N] fp32 or NULL: the chosen score; NaN for a non-finite row, +inf when no class was chosen.
 *   scores [N][K] fp32 or NULL: every score; a row of NaN for a non-finite row.
 * No N x K x L array exists anywhere, and a row's outputs depend on its own values and the model alone: not on N, on its position
 * or on the launch geometry. */
long long eae_class_scatter_workspace_bytes(long long N, int L, int K);
int eae_class_scatter(void* stream, const float* z, long long N, int L, const long long* labels, const long long* order,
                      const long long* seg, int K, const float* means, float* scatter, void* workspace, long long workspace_bytes);
int eae_gauss_score(void* stream, const float* z, long long N, int L, const float* mu, const float* W, long long w_stride,
                    const float* offset, int K, long long* labels, float* maha, float* best, float* scores);

/* ------------------------------------------------------------------ map post-processing ------------ */
/* Cleaning a class map on the device (no reference counterpart): majority filter, connected regions, their table, and a sieve.  A map
 * is a contiguous int64 [H][W] device array as eae_scene_classify / eae_scene_blend write it: a value in [0, K) is a class, K in 1..64,
 * every other value (the -1 of a window that was not run included) is "unclassified".  H, W >= 1 and H * W < 2^31.  Stateless; every
 * call goes to `stream` and nothing synchronises the host.  Anything outside these limits or a NULL required pointer is EAE_ERR_ARG and
 * nothing is launched.  Integers throughout (vector stores, integer atomics): every result is exact and identical from run to run.
 *
 * eae_map_majority: out[y][x] = the most frequent class among the classified cells of the (2 radius + 1)^2 window centred on (y, x),
 * clipped at the map's edge; radius in 1..7.  Ties: the centre's own class when it is among the tied ones, else the lowest class id.
 * An unclassified centre stays as stored, unless fill != 0 and the window holds a classified cell: then it takes the winner.
 * in != out (a pass reads the whole input: Jacobi).
 *
 * eae_map_regions: regions[y][x] = the region of a classified cell, -1 for an unclassified one.  A region is a maximal set of cells of
 * one class connected through edges (connectivity 4) or edges and corners (8); its id is the smallest linear index y * W + x of its
 * cells, so the result is unique.  Union-find with union-by-minimum in three launches (label 32 x 32 tiles in LDS, merge the tile
 * borders with device-scope atomics on the parent array, flatten); no workgroup waits for another.  workspace: device memory of at
 * least eae_map_workspace_bytes(H, W) bytes (host only; < 0 on bad arguments), contents irrelevant on entry; NULL or too small is
 * EAE_ERR_ARG.
 *
 * eae_map_region_stats: area int32 [H * W]: area[id] = the number of cells of region id, 0 at every index that is no region id.
 * bbox (or NULL) int32 [H * W][4]: (y0, x0, y1, x1) of region id, inclusive, at row id; rows that are no region id hold -1s.
 * regions is what eae_map_regions wrote (a value outside [0, H * W) counts nowhere).
 *
 * eae_map_sieve_pass: one sieve pass, decided entirely from its input.  With regions and area of `labels` as the two calls above give
 * them (under either connectivity): a region is small when area < min_size (min_size >= 1).  The candidates of a small region are the
 * regions that are not small and share a cell EDGE with it (for both connectivities); it takes the class of the candidate with the
 * largest area, the lowest region id on a tie, whatever the order of arrival (a 64-bit atomic max of (area << 32) | (0xFFFFFFFF - id)
 * per small root).  A small region without a candidate, and every unclassified cell, is copied as stored.  out != labels.  *changed
 * (device int64, or NULL) receives the number of cells whose value changed.  workspace: as for eae_map_regions (and may be the same:
 * the parents are dead once regions is written). */
long long eae_map_workspace_bytes(int H, int W);
int eae_map_majority(void* stream, const long long* in, int H, int W, int K, int radius, int fill, long long* out);
int eae_map_regions(void* stream, const long long* labels, int H, int W, int K, int connectivity, long long* regions, void* workspace,
                    long long workspace_bytes);
int eae_map_region_stats(void* stream, const long long* regions, int H, int W, int* area, int* bbox);
int eae_map_sieve_pass(void* stream, const long long* labels, const long long* regions, const int* area, int H, int W,
                       long long min_size, long long* out, long long* changed, void* workspace, long long workspace_bytes);

/* ------------------------------------------------------------------ zonal statistics --------------- */
/* Object-based classification (no reference counterpart): what a class map says inside every zone of a zone
 * raster, and a per-zone value painted back at pixel resolution.  zones [H][W] is a device raster of zone ids at the scene's pixel
 * resolution, int32 (zone_elem_bytes 4) or int64 (8), read natively; an id in [0, Z) is a zone, every other id (negatives: "no
 * zone") is skipped entirely.  H, W >= 1 and H * W < 2^31.  Stateless; every call goes to `stream` and nothing synchronises the host.
 *
 * eae_zonal_accumulate: labels is an int64 [cH][cW] map of cell x cell cells and probs NULL or the float [K][cH][cW] probabilities
 * of the same cells (eae_scene_classify / eae_scene_blend); mask is NULL or uint8 [H][W]; votes is int64 [Z][K + 1], prob_sums
 * int64 [Z][K], non-NULL exactly when probs is.  1 <= K <= 64, Z >= 1, Z * (K + 1) <= 2^31 - 1, cell >= 1, oy, ox >= 0.
 *   For every pixel (y, x) with mask[y][x] == 0 and z = zones[y][x] in [0, Z):
 *     its cell is ((y + oy) / cell, (x + ox) / cell), as in eae_scene_confusion;
 *     c = the cell's label when the cell lies inside the map and the label is in [0, K), else K (not classified, not covered, any
 *         other value);
 *     votes[z][c] += 1;
 *     with probs and c < K, for every class j: prob_sums[z][j] += q(probs[j][cell]),
 *       q(p) = rint(2^32 * min(max(p, 0), 1)) evaluated in double, round-half-even, q(NaN) = 0.
 *   q <= 2^32 and a zone has fewer than 2^31 pixels: every sum stays below 2^63.  So votes sums to the number of unmasked pixels
 *   whose id is in range.  accumulate = 0: both tables are cleared first, on the stream; accumulate = 1: the call adds to what they
 *   hold (several scenes).
 * Integers only (64-bit integer adds in LDS and in global memory, no float atomics): exact, identical from run to run and independent
 * of the launch geometry.  The raster and the mask are read once with 16-byte loads; no per-pixel copy of the map or of the ids is made.
 *
 * eae_zonal_paint: out[y][x] (int64 [H][W]) = values[zones[y][x]] (values: int64 [Z], Z >= 1) where the id is in [0, Z), else fill.
 * One pass; no int64 copy of the zone raster.
 *
 * Rejected (EAE_ERR_ARG, nothing launched): a NULL zones, labels, votes, values or out; probs without prob_sums or the reverse; a
 * zone_elem_bytes other than 4 or 8 or a zones pointer that is no multiple of it; K, Z, cell, oy, ox outside the limits above; an
 * empty raster or map, or H * W >= 2^31; accumulate outside 0..1. */
int eae_zonal_accumulate(void* stream, const void* zones, int zone_elem_bytes, int H, int W, const long long* labels, const float* probs,
                         int cH, int cW, int cell, int oy, int ox, const unsigned char* mask, int K, long long Z, int accumulate,
                         long long* votes, long long* prob_sums);
int eae_zonal_paint(void* stream, const void* zones, int zone_elem_bytes, int H, int W, const long long* values, long long Z,
                    long long fill, long long* out);

/* ------------------------------------------------------------------ superpixels -------------------- */
/* SLIC superpixels of a scene (no reference counterpart): the segmenter that gives eae_zonal_accumulate a zone
 * raster.  Integers only, so sums, centres and labels are unique for given inputs, whatever the launch geometry.  data is a device
 * scene [C][H][W] of dtype EAE_SCENE_U8 / U16 / F32, C in 1..16, H, W >= 1 and H * W < 2^31; divisor a device float [C]; mask NULL or
 * uint8 [H][W] (non-zero: the pixel takes no part).  The plain arguments are all there is: no window geometry.
 *   Feature: u_c(y, x) = rint(65535 * min(max(v / d_c, 0), 1)), an integer in 0..65535, evaluated in double from the stored value and
 *   the float divisor (both converted to double), round-half-even, NaN -> 0 (the comparisons in the order of the zonal q).
 *   Grid: step S in 2..256, n_h = ceil(H / S), n_w = ceil(W / S); cluster k = i * n_w + j belongs to cell (i, j), the home cell of a
 *   pixel is (y / S, x / S); n_h * n_w * (C + 3) <= 2^31 - 1.
 *   Tables: sums int64 [n_h * n_w][C + 3] = (count, sum y, sum x, sum u_0, ..); centres int32 of the same shape = (count, cy, cx,
 *   mu_0, ..), every mean (2 sum + n) / (2 n) in integers, an empty cluster (n = 0) all zeros.
 *
 * eae_slic_step: one iteration.  centres_in == NULL: every unmasked pixel belongs to its home cluster (iteration 0).  Otherwise a
 * pixel considers the clusters of the cells (i + di, j + dj), di, dj in {-1, 0, 1}, of its home cell (i, j) that lie inside the grid
 * and have count > 0, and takes the one with the smallest
 *     D = S^2 * sum_c (u_c - mu_c)^2 + spatial_weight * ((y - cy)^2 + (x - cx)^2)     (64-bit integers; 0 <= spatial_weight <= 2^40)
 * the lowest cluster id on a tie.  centres_in must come from sums of an earlier step of the same scene (then every pixel has a
 * candidate, and |y - cy|, |x - cx| < 3 S keep D below 2^63).  sums_out is cleared by the call, on the stream, and receives the sums of
 * the new assignment; labels_out (int32 [H][W], or NULL: nothing is written, intermediate iterations need no labels) receives the
 * chosen cluster, -1 for a masked pixel.  A masked pixel contributes nothing.
 *
 * eae_slic_centres: centres from sums, one thread per entry; n_clusters >= 1, n_clusters * (C + 3) <= 2^31 - 1.
 *
 * eae_map_regions_wide: eae_map_regions for maps whose labels are arbitrary int64 values: any value >= 0 is a label, compared on all
 * 64 bits, a negative value is unclassified.  The same kernels (templated on how a cell's label is read and kept), the same ids, the
 * same workspace.
 *
 * Rejected (EAE_ERR_ARG, nothing launched, the call's name in eae_last_error()): a NULL data, divisor, sums_out, sums, centres, labels,
 * regions or workspace; an unknown dtype or a data pointer that is no multiple of the element size; C, H, W, the step, the spatial
 * weight, the grid or n_clusters outside the limits above; a connectivity other than 4 or 8; a workspace that is too small. */
int eae_slic_step(void* stream, const void* data, int dtype, int C, int H, int W, const float* divisor, const unsigned char* mask,
                  int step, long long spatial_weight, const int* centres_in, long long* sums_out, int* labels_out);
int eae_slic_centres(void* stream, const long long* sums, long long n_clusters, int C, int* centres);
int eae_map_regions_wide(void* stream, const long long* labels, int H, int W, int connectivity, long long* regions, void* workspace,
                         long long workspace_bytes);

/* ------------------------------------------------------------------ change detection --------------- */
/* The two passes of an IR-MAD iteration (iteratively reweighted multivariate alteration detection, Nielsen 2007) over two scenes of
 * one place (no reference counterpart).  a and b are device scenes [C][H][W], contiguous, each of dtype
 * EAE_SCENE_U8 / U16 / F32 (the two may differ), C in 1..16, H, W >= 1, H * W < 2^31; div_a, div_b device floats [C].  The pixel
 * vector is v = [x_0 .. x_{C-1}, y_0 .. y_{C-1}], x_c = a_c / div_a[c], y_c = b_c / div_b[c], each one fp32 division.  A pixel is
 * invalid when mask[y * W + x] != 0 (mask: uint8 [H][W] or NULL), when either scene's nodata test fires (nodata_mode_*, nodata_*,
 * rule_*: EAE_NODATA_* and EAE_INVALID_* exactly as eae_scene_invalid_counts defines them, per scene), or when a float32 band holds a
 * NaN or an Inf.  Stateless; every call goes to `stream` and nothing synchronises the host.
 *
 * eae_change_moments: out_moments (device double [1 + 2C + (2C)^2]) = N = sum w, then s = sum w (v - p), then S = sum w (v - p)
 * (v - p)^T row-major, over the valid pixels; out_count (device int64) = the number of valid pixels.  weights: device float [H][W] or
 * NULL for 1; a weight that is NaN, negative or infinite makes its pixel invalid, a weight of 0 leaves it valid.  pivot: device
 * float [2C]; v - p is one fp32 subtraction.  The raster is cut into chunks of a fixed number of pixels (a multiple of 256; at most
 * 4096 chunks), a function of (C, H, W) alone.  A chunk's products w (v - p)_i * (v - p)_j accumulate in fp32 in a fixed order on the
 * f32-input MFMA (v_mfma_f32_32x32x2_f32; 2C is padded to a power of two D and the 32 x 32 tile carries 32 / D pixel streams on its
 * diagonal blocks), s and N beside it in the lane; every chunk stores its whole partial to `workspace`, and a second kernel adds the
 * partials in float64 in ascending chunk order (256 runs of consecutive chunks, then the runs) and writes S[i][j] and S[j][i] from one
 * register.  No float atomics: S is bitwise symmetric, every output word is written (zeros and a count of 0 when no pixel is valid),
 * and the result is bitwise identical from run to run.  workspace: device memory of at least
 * eae_change_moments_workspace_bytes(C, H, W) bytes (host only; < 0 on bad arguments), contents irrelevant on entry.
 *
 * eae_change_variates: per valid pixel M_i = sum_j T[j][i] (v_j - mean[j]), i < C: one fp32 fma chain in ascending j (mean: device
 * float [2C], T: device float [2C][C]); Z = sum_i M_i^2, one fma chain in ascending i; prob = Q(dof / 2, Z / 2), the chi-square
 * survival function, dof in 1..16, in closed form:
 *   dof = 2 m:     e^-h sum_{j < m} h^j / j!,                                          h = Z / 2
 *   dof = 2 m + 1: erfc(sqrt h) + e^-h sum_{j = 1..m} h^(j - 1/2) / Gamma(j + 1/2)
 * (0 above Z = 256, where every Q is below 2^-126).  out_chi2, out_prob: float [H][W]; out_variates: float [C][H][W]; each may be
 * NULL.  An invalid pixel gets chi2 = NaN, prob = 0, variates = NaN.  A pixel's results depend on its own values and the model alone:
 * not on the launch geometry, nor on which outputs are requested.
 *
 * Rejected (EAE_ERR_ARG, nothing launched, the call's name in eae_last_error()): a NULL scene, divisor, pivot, out_moments,
 * out_count, mean, T or workspace; an unknown dtype or a scene pointer that is no multiple of its element size; C, H, W or dof
 * outside the limits above; an unknown nodata mode or rule, a NaN nodata or a value outside the dtype's range for an integer scene;
 * a workspace that is too small. */
long long eae_change_moments_workspace_bytes(int C, int H, int W);
int eae_change_moments(void* stream, const void* a, const void* b, int dtype_a, int dtype_b, int C, int H, int W, const float* div_a,
                       const float* div_b, int nodata_mode_a, float nodata_a, int rule_a, int nodata_mode_b, float nodata_b,
                       int rule_b, const unsigned char* mask, const float* weights, const float* pivot, double* out_moments,
                       long long* out_count, void* workspace, long long workspace_bytes);
int eae_change_variates(void* stream, const void* a, const void* b, int dtype_a, int dtype_b, int C, int H, int W, const float* div_a,
                        const float* div_b, int nodata_mode_a, float nodata_a, int rule_a, int nodata_mode_b, float nodata_b,
                        int rule_b, const unsigned char* mask, const float* mean, const float* T, int dof, float* out_chi2,
                        float* out_prob, float* out_variates);

/* ------------------------------------------------------------------ co-registration ---------------- */
/* Tie points between two scenes of one place and the resampling of a scene through an affine map (no reference counterpart;
 * DESIGN.md section 37; tests/register_ref.py is the NumPy definition of everything below).  Scenes are device rasters [C][H][W],
 * contiguous, of dtype EAE_SCENE_U8 / U16 / F32, C in 1..16, H, W >= 1, H * W < 2^31.  Stateless; every call goes to `stream` and
 * nothing synchronises the host.
 *   Coordinates: pixel (y, x) has its centre at the integer point (x, y).  A transform is a row-major 2 x 3 double matrix M that maps
 *   a point of the DESTINATION grid to a point of the SOURCE grid: sx = (M[0] x + M[1] y) + M[2], sy = (M[3] x + M[4] y) + M[5].  For
 *   co-registration the destination is A's grid and the source is B: M says where in B a pixel of A lies.
 *   Feature: the feature of the superpixel step above, u = rint(65535 * min(max(v / d, 0), 1)), evaluated in double from the stored value
 *   and the float divisor, half to even, an integer in 0..65535; one band of each scene is matched (band_a, band_b; div_a, div_b are
 *   device floats [Ca] and [Cb], of which the matched band's entry is read).
 *   Validity: exactly as in the change moments above: a pixel is invalid when its mask byte is set (mask: uint8 [H][W] of the
 *   scene, or NULL), when the scene's nodata test fires (EAE_NODATA_*, EAE_INVALID_*, per scene, over all C bands of that scene), or
 *   when a float32 band is NaN or Inf.  A position outside the raster is invalid too.
 *
 * eae_match_tiles: the sums that define the zero-mean normalised cross-correlation of n_tiles templates of A with B at every integer
 * offset of a search window.  tile T in 4..64, radius R in 0..16, n_tiles in 1..2^20; the two scenes may differ in shape, dtype and
 * band count.  origins_a / origins_b: device int32 [n_tiles][2] = (y, x), the top-left pixel of the template in A and of the
 * zero-offset window in B; any int32, since everything outside a raster is invalid.  For tile t and offset (dy, dx) in [-R, R]^2,
 * entry o = (dy + R)(2R + 1) + (dx + R), the sums run over (i, j) in [0, T)^2 and take the pairs whose two pixels are both valid,
 * A at (ay + i, ax + j) and B at (by + dy + i, bx + dx + j):
 *     sums[t][o] = (n, sum u_a, sum u_b, sum u_a^2, sum u_b^2, sum u_a u_b)        int64 [n_tiles][(2R + 1)^2][6], all below 2^45
 * Integers only: the table is unique for given inputs, independent of the launch geometry and identical from run to run.  Every
 * output word is written (zeros where no pair is valid).
 *
 * eae_scene_resample: dst[c][y][x] for every pixel of a destination grid [Hd][Wd] (Hd, Wd >= 1, Hd * Wd < 2^31; same dtype and band
 * count as src) from the source at (sx, sy) = M (x, y).  matrix is a HOST pointer to 6 doubles, read during the call.  All arithmetic
 * is float64, one correctly rounded operation at a time and never contracted, in exactly this order:
 *   nearest (EAE_RESAMPLE_NEAREST):   one tap at floor(s + 0.5) per axis, weight 1.
 *   bilinear (EAE_RESAMPLE_BILINEAR): x0 = floor(sx), t = sx - x0; taps x0, x0 + 1 with weights (1 - t, t); likewise in y.
 *   cubic (EAE_RESAMPLE_CUBIC):       Catmull-Rom (a = -0.5, GDAL's cubic); taps x0 - 1 .. x0 + 2 with the Horner forms
 *       w0 = ((-0.5 t + 1) t - 0.5) t     w1 = ((1.5 t - 2.5) t) t + 1     w2 = ((-1.5 t + 2) t + 0.5) t     w3 = ((0.5 t - 0.5) t) t
 *   A tap (r, c) takes part when both its axis weights wy[r] and wx[c] are not exactly zero.  value = the sum over the participating
 *   taps, rows ascending and columns ascending inside a row, of (wy[r] * wx[c]) * v; the first term starts the sum (nothing is added
 *   to a zero).  An integer dtype stores rint (half to even) of the sum clamped to the dtype's range (cubic overshoots); float32
 *   one conversion from double.
 *   An output pixel is valid if and only if sx and sy are finite and every participating tap is a valid source pixel; an invalid one
 *   gets `fill` in every band (rint of it for an integer dtype) and 0 in out_valid (uint8 [Hd][Wd] or NULL), a valid one 1.  So
 *   the identity reproduces the source bit for bit, and an integer translation is a shifted copy with `fill` in the uncovered strip,
 *   for all three methods.
 *
 * Rejected (EAE_ERR_ARG, nothing launched, the call's name in eae_last_error()): a NULL scene, divisor, origin table, sums, matrix or
 * dst; an unknown dtype, method, nodata mode or rule; a scene or dst pointer that is no multiple of its element size; a band index
 * outside its scene; T, R, n_tiles, C or a shape outside the limits; a nodata value that the dtype cannot hold; a matrix entry that is
 * not finite; a fill outside an integer dtype's range (NaN included; a float32 scene takes any fill). */
#define EAE_RESAMPLE_NEAREST 0
#define EAE_RESAMPLE_BILINEAR 1
#define EAE_RESAMPLE_CUBIC 2
int eae_match_tiles(void* stream, const void* a, int dtype_a, int Ca, int Ha, int Wa, int band_a, const float* div_a,
                    int nodata_mode_a, float nodata_a, int rule_a, const unsigned char* mask_a, const void* b, int dtype_b, int Cb,
                    int Hb, int Wb, int band_b, const float* div_b, int nodata_mode_b, float nodata_b, int rule_b,
                    const unsigned char* mask_b, int tile, int radius, int n_tiles, const int* origins_a, const int* origins_b,
                    long long* sums);
int eae_scene_resample(void* stream, const void* src, int dtype, int C, int Hs, int Ws, int nodata_mode, float nodata, int rule,
                       const unsigned char* mask_src, const double* matrix, int method, double fill, void* dst, int Hd, int Wd,
                       unsigned char* out_valid);

#ifdef __cplusplus
}
#endif
#endif /* EAE_H */
