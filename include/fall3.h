/* fall3 — MI355X-native (gfx950) 3-stream fall-detection training step: C ABI.
 *
 * This is the drop-in boundary for the reference's model/step interface
 * (/root/reference/Multimodal_Fall3/model/...). Each entry point replaces one call of
 * the reference training loop (model/main.py:91-148):
 *
 *   f3_net_create      <- build_model(config)            model/build_model.py:5-19
 *   f3_net_entry       <- model.state_dict() keys/shapes  (same names, order, shapes)
 *   f3_net_forward     <- pred = model(data, sensor)      model/main.py:112, combination.py:37-46
 *   f3_net_loss        <- loss_fn(pred, label_onehot)     model/main.py:113,280 (CE, soft targets)
 *   f3_net_backward    <- loss.backward()                 model/main.py:115
 *   f3_rmsprop_step    <- optimizer.step()                model/main.py:127, optimizer.py:21
 *   f3_net_backward_rmsprop <- loss.backward(); optimizer.step()  (one GPU: the update per layer
 *                              as soon as its gradients are final)
 *   f3_optim_step      <- clip_grad_norm_(); optimizer.step() for torch.optim.SGD / Adam / AdamW /
 *                         RMSprop with weight decay   model/optimizer.py:20-29, root main.py:108-113
 *   f3_net_backward_optim <- loss.backward(); clip_grad_norm_(); optimizer.step() in one call
 *   f3_optim_hyper_set <- lr_scheduler.step(e)           model/main.py:321-322 (for a step recorded in a graph)
 *   f3_optim_step_hyper <- optimizer.step()              model/main.py:127, hyper-parameters read on the device
 *   f3_metrics_update  <- cal_top_k_accuracy(), running loss, confusion matrix   model/main.py:57-77,
 *                         134-135, 189-200 (accumulated on the device: no copy or sync per batch)
 *   f3_segment_norms   <- param.grad.norm().item() per parameter   model/main.py:84-89
 *   f3_net_loss_ex     <- CrossEntropyLoss(label_smoothing=TRAIN.LABEL_SMOOTHING)   model/main.py:280
 *   f3_net_loss_w      <- CrossEntropyLoss(weight=w, label_smoothing=eps): per-class weights
 *   f3_grad_accumulate <- .grad += g between the optimizer steps of TRAIN.ACCUM_ITER  model/main.py:115-132
 *   f3_ema_update      <- AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)).update_parameters(model)
 *                         after optimizer.step() (torch.optim.swa_utils; the loop itself has no averaging)
 *
 * Conventions: plain pointers to device memory (HIP), sizes in elements, a HIP stream
 * passed as void*. No call allocates, frees or synchronises: every buffer (flat
 * parameters, flat grads, BN buffers, workspace) is owned by the caller, so a full
 * step can be captured into a HIP graph. Every function returns 0 on success or an
 * F3_E* status (never aborts); f3_status_string() names it.
 */
#ifndef FALL3_H
#define FALL3_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F3_OK 0
#define F3_EINVAL 1001 /* bad argument / unsupported shape */
#define F3_EBATCH 1002 /* train-mode batch of 1: BatchNorm needs >1 value per channel */
#define F3_EHIP 1003   /* HIP launch error */
#define F3_ESTATE 1004 /* backward without a training forward on this workspace */
#define F3_EDEVICE 1005 /* a device-side check failed (a group barrier of the TARGCN GRU or the sensor CNN1D timed out) */

enum { F3_MODEL_TWO_STGCAN_BILSTM = 0, F3_MODEL_TWO_STGCAN = 1, F3_MODEL_STGCN = 2, F3_MODEL_BILSTM = 3 };
enum { F3_SENSOR_NONE = 0, F3_SENSOR_BILSTM = 1, F3_SENSOR_CNN_BILSTM = 2 };
enum { F3_NAMING_PACKAGE = 0, F3_NAMING_NOTEBOOK = 1 };
enum { F3_PRECISION_FP32 = 0, /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32): parity mode */
       F3_PRECISION_BF16 = 1, /* bf16 GEMM operands in HBM, fp32 accumulate (v_mfma_f32_16x16x32_bf16) */
       F3_PRECISION_BF16_FP32IN = 2, /* kernel-level entries only: bf16 arithmetic on fp32 activations */
       F3_PRECISION_BF16X3 = 4 /* split-bf16 parity mode: fp32 activations, every GEMM operand split into
                                  bf16 hi + lo, products hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16
                                  with fp32 accumulate (~2^-16 per product; gemm_x3.hip) */ };
enum { F3_ENTRY_PARAM = 0, F3_ENTRY_BUFFER = 1, F3_ENTRY_COUNTER = 2 };

typedef struct f3_config {
  int model;           /* F3_MODEL_*  (build_model.py:9-17 MODEL.NAME) */
  int num_node;        /* V: 14 coco_cut, 18 coco_mmpose (graph.py:24-49) */
  int num_partition;   /* K: 1 uniform, 2 distance, 3 spatial (graph.py:50-90) */
  int num_class;       /* DATA.NUM_CLASSES */
  int in_channels;     /* DATA.IN_CHANNELS (stgcn model) */
  int sensor;          /* F3_SENSOR_* */
  int sensor_dim;      /* DATA.SENSOR_DIM */
  int sensor_classes;  /* BiLSTM head width (package: num_class; UR notebook: 2) */
  int softmax_output;  /* notebook form returns softmax (GSTCAN_HAR_conv_10kfold.ipynb:444) */
  int naming;          /* F3_NAMING_* state_dict prefixes */
  int frames;          /* skeleton window T (30) */
  int sensor_frames;   /* IMU window Ts (30) */
  int precision;       /* F3_PRECISION_*: GEMM operand type of the skeleton streams' convs */
} f3_config;

typedef struct f3_net f3_net;

int f3_net_create(const f3_config* cfg, f3_net** out);
void f3_net_destroy(f3_net* net);

/* state_dict table: entries in reference order. kind = F3_ENTRY_*; offset indexes the
 * flat fp32 parameter array (PARAM), the flat fp32 buffer array (BUFFER: A, running
 * stats) or the flat int64 counter array (COUNTER: num_batches_tracked). */
int f3_net_num_entries(const f3_net* net);
int f3_net_entry(const f3_net* net, int i, const char** name, int* kind, int* ndim, int64_t* shape8,
                 int64_t* offset);
int64_t f3_net_param_count(const f3_net* net);
int64_t f3_net_buffer_count(const f3_net* net);
int64_t f3_net_counter_count(const f3_net* net);
int64_t f3_net_workspace_bytes(const f3_net* net, int batch);

/* Forward. skel f32[N,3,T,V] (reference layout), sensor f32[N,Ts,S] (ignored without a
 * sensor stream), out f32[N,C] (logits, or softmax for softmax_output). training=1 uses
 * batch statistics and updates running stats / num_batches_tracked in place (momentum
 * 0.1); training=0 uses running statistics. The workspace keeps what backward needs. */
int f3_net_forward(f3_net* net, int batch, int training, const float* params, float* buffers, int64_t* counters,
                   const float* skel, const float* sensor, float* out, void* workspace, void* stream);

/* loss = -(1/N) sum_i sum_c y_ic log_softmax(out_i)_c ; dout = dloss/dout. */
int f3_net_loss(f3_net* net, int batch, const float* out, const float* label, float* loss, float* dout,
                void* stream);

/* Backward of the last training forward on `workspace`: grads (flat, same layout as
 * params) are OVERWRITTEN with d(sum dout*out)/dparams. */
int f3_net_backward(f3_net* net, int batch, const float* params, const float* dout, float* grads,
                    void* workspace, void* stream);

/* Timing of the sensor CNN1D stages (GSTCAN_UR_conv.ipynb:493-514; models with the CNN1D
 * sensor branch only). enable=1 records HIP events around the Conv1D launches of every later
 * forward / backward on the sensor queue; ms (may be NULL) receives the last forward + backward's
 * 2 times in ms: both CNN1D layers forward, both backward (one cooperative launch each in
 * training; the per-layer launches in eval or under stream capture). No reference counterpart:
 * measurement only. */
int f3_net_sensor_times(f3_net* net, int enable, float* ms);

/* The same backward in two phases, for overlapping the data-parallel gradient all-reduce
 * with compute: phase 1 = zero grads, head, sensor branch and skeleton layers 4-6 (their
 * gradients, params[0 .. f3_net_grad_split) in the flat buffer); phase 2 = skeleton layers 0-3
 * and data_bn (the rest). phase 0 = both (f3_net_backward). Parameter offsets are laid out
 * phase-1-first; state_dict order is unchanged.
 * Phase 1 returns WITHOUT ordering `stream` after its private queues (the weight-gradient queues
 * keep draining while phase 2's critical path starts): make the all-reduce stream wait with
 * f3_net_wait_phase1 before reducing params[0 .. split). Phase 2 ends with `stream` ordered after
 * all work of both phases. */
int f3_net_backward_phase(f3_net* net, int batch, const float* params, const float* dout, float* grads,
                          void* workspace, int phase, void* stream);
int64_t f3_net_grad_split(const f3_net* net);
int f3_net_wait_phase1(f3_net* net, void* stream);

/* The single-GPU step's backward and optimizer in one call: f3_net_backward followed by
 * f3_rmsprop_step(params, square_avg, grads, nparam, lr, alpha, eps, 1.0) (loss.backward() +
 * optimizer.step(), model/main.py:115-127), except that each skeleton layer's RMSprop update is
 * issued on the queue that finishes that layer's gradients, as soon as they are final, instead of
 * after the whole backward; the rest (data_bn, sensor branch, head) follows the join. grads holds
 * the step's gradients afterwards as with f3_net_backward. Identical updates; not for data
 * parallelism (the all-reduce must come between the two). */
int f3_net_backward_rmsprop(f3_net* net, int batch, float* params, const float* dout, float* grads, float* square_avg,
                            void* workspace, float lr, float alpha, float eps, void* stream);
/* 1 if f3_net_backward_rmsprop issues the per-layer updates, 0 if it falls back to the backward
 * followed by one update (fixed by the parameter layout and precision; planned once per net). */
int f3_net_fused_rmsprop(f3_net* net);

/* The F3_PRECISION_* the net was created with (reads back f3_config.precision; -1 for NULL). */
int f3_net_precision(const f3_net* net);

/* Device status of the last training forward / backward (the sensor branch's cooperative CNN1D:
 * its group barriers time out instead of hanging when the workgroups cannot all be resident; the
 * launch then writes NaN into its outputs). Returns F3_EDEVICE if a copy of that error word flagged
 * a timeout (wait = 1: after every enqueued copy has completed; 0: those that have). Every
 * f3_net_forward / _backward* also returns F3_EDEVICE once when it finds a completed, flagged copy
 * from an earlier call. No reference counterpart: the reference's nn.Conv1d cannot fail this way
 * (GSTCAN_UR_conv.ipynb:493-514). */
int f3_net_status(f3_net* net, int wait);

/* torch.optim.RMSprop(lr, alpha, eps), no momentum / weight decay / centering, on
 * g = grad_scale * grads (1.0 = torch semantics; 1/world after a summed all-reduce):
 * sq = alpha*sq + (1-alpha)*g^2 ; p -= lr*g/(sqrt(sq)+eps). */
int f3_rmsprop_step(float* params, float* square_avg, const float* grads, int64_t n, float lr, float alpha,
                    float eps, float grad_scale, void* stream);

/* ---- SGD / Adam / AdamW / RMSprop with weight decay and global grad-norm clipping ----
 * f3_optim_config  <- the arguments of torch.optim.RMSprop / SGD / Adam / AdamW as build_optimizer
 *                     passes them (model/optimizer.py:8-29: lr, momentum, betas, eps, weight_decay)
 *                     plus TRAIN.MAX_NORM (root main.py:108-113 clip_grad_norm_).
 * Arithmetic is torch.optim's on g = grad_scale * clip_coef * grad:
 *   RMSPROP  g += wd p; sq = alpha sq + (1-alpha) g^2; p -= lr g / (sqrt(sq) + eps)
 *   SGD      g += wd p; buf = momentum buf + g; p -= lr (nesterov ? g + momentum buf : buf)
 *            (dampening 0; a zero buf reproduces torch's first step; momentum 0 keeps no buf)
 *   ADAM     g += wd p; m += (1-beta1)(g - m); v = beta2 v + (1-beta2) g^2;
 *            p -= lr/(1-beta1^t) m / (sqrt(v)/sqrt(1-beta2^t) + eps)
 *   ADAMW    p *= 1 - lr wd, then ADAM with wd = 0
 * state0 / state1: RMSPROP square_avg / -, SGD momentum_buffer (NULL for momentum 0) / -, ADAM(W)
 * exp_avg / exp_avg_sq. The state recurrences are evaluated in fp64 and rounded to fp32 once; the
 * one sqrt and division per element are fp32. Unsupported (F3_EINVAL): RMSprop momentum, nesterov
 * without momentum, negative / non-finite settings. The elements of skip_lo[i] .. + skip_len[i]
 * (floats, multiples of 4; the entries no backward writes, f3_net_entry_nograd) are left untouched
 * in params and states, as torch.optim skips a parameter whose .grad is None. */
enum { F3_OPT_RMSPROP = 0, F3_OPT_SGD = 1, F3_OPT_ADAM = 2, F3_OPT_ADAMW = 3 };
#define F3_OPT_MAX_SKIP 4
typedef struct f3_optim_config {
  int kind;            /* F3_OPT_*  (OPTIM.TYPE, optimizer.py:20-29) */
  int nesterov;        /* SGD(nesterov=) */
  double lr;           /* OPTIM.LR */
  double alpha;        /* RMSprop(alpha=) */
  double eps;          /* OPTIM.EPS (RMSprop / Adam / AdamW eps) */
  double momentum;     /* OPTIM.MOMENTUM (SGD) */
  double beta1, beta2; /* OPTIM.BETAS */
  double weight_decay; /* OPTIM.WEIGHT_DECAY */
  double max_norm;     /* TRAIN.MAX_NORM, clip_grad_norm_(parameters, max_norm) L2; 0 = off */
  double grad_scale;   /* 1.0 = torch semantics; 1/world after a summed all-reduce */
  int nskip;           /* <= F3_OPT_MAX_SKIP ranges that never receive a gradient */
  int64_t skip_lo[F3_OPT_MAX_SKIP], skip_len[F3_OPT_MAX_SKIP];
  int skip_nonfinite;  /* nonzero: skip the update when the gradient is not finite (below); 0 = off */
} f3_optim_config;
/* The step scalars: a device block of f3_optim_scalars_bytes() bytes (8-byte aligned, zeroed by the
 * caller before the first step) that each step's one-workgroup "begin" kernel rewrites and every
 * update launch of the step reads: int64 t (the step count, incremented per step, so a replayed HIP
 * graph advances it) at byte 0; fp32 1/(1-beta1^t), 1/sqrt(1-beta2^t) (fp64 from t, rounded once),
 * clip_coef = min(1, max_norm/(norm + 1e-6)) and grad_norm = grad_scale * ||grads||_2 at bytes 8, 12,
 * 16, 20 (clip_coef 1, grad_norm 0 with max_norm 0); then the norm's per-workgroup fp64 partial sums,
 * added in index order (no float atomics: same bits every run); then, at f3_optim_guard_offset(), the
 * guard words: int64 skipped and, 8 bytes on, int32 last_skipped. */
int64_t f3_optim_scalars_bytes(void);
/* ---- skip_nonfinite: the update is applied iff every element of the gradient it consumes is finite ----
 * What torch.cuda.amp.GradScaler.step does for an inf/NaN gradient (the reference builds one,
 * TRAIN.USE_SCALER, model/main.py:281), decided on the device with no host sync, so it holds for a
 * replayed HIP graph as well. Off (0) every launch and every bit are as without the field.
 * The test: the gradient is non-finite iff the fp64 sum of squares over grads[0..n), the one the norm
 * forms (per-workgroup partials added in index order), is not finite. That is exact: an fp32 square is
 * exact in fp64, squares are non-negative, and n * FLT_MAX^2 is far below DBL_MAX, so the sum is inf/NaN
 * exactly when some element is. The fp32 grad_norm is not the test: a finite gradient whose norm exceeds
 * FLT_MAX is applied.
 * A skipped step: params, state0 and state1 keep their bits (the update launch stores nothing: every
 * thread reads last_skipped and returns); t is not advanced, so Adam's bias corrections at the next
 * applied step are those of t + 1; clip_coef = 0.0; grad_norm = (float)(grad_scale * sqrt(sum)), inf or
 * NaN; skipped (the number of skipped updates since the block was zeroed) += 1; last_skipped = 1.
 * An applied step: last_skipped = 0, skipped unchanged; t, the bias corrections and clip_coef as without
 * the guard; grad_norm is written even with max_norm 0 (the sum is formed anyway). Parameters and states
 * are bit for bit those of the unguarded flat f3_optim_step with the same clip_coef; plain RMSprop (no
 * decay, no clipping) runs the kernel it runs with max_norm set, so its bits are those of the unguarded
 * step with a max_norm large enough that clip_coef == 1. All sums have a fixed order and there are no
 * float atomics: the same inputs give the same bits, and the same decision, on every run and every rank.
 * f3_optim_step, f3_optim_step_hyper and f3_net_backward_optim honour it (the last with one flat update
 * after the join, as with clipping); f3_optim_step_ranges returns F3_EINVAL: the decision needs every
 * gradient. scalars is then required for every kind. Unguarded steps never write the guard words. */
int64_t f3_optim_guard_offset(void); /* byte offset of `skipped` in the step scalars; last_skipped at + 8 */
/* optimizer.step() (model/main.py:127), preceded by clip_grad_norm_ when max_norm > 0 (root
 * main.py:108-113): [norm partials], begin, one flat update over n floats. grads are not modified
 * (the clip coefficient is a factor inside the update). F3_OPT_RMSPROP with weight_decay 0 and
 * max_norm 0 launches f3_rmsprop_step's kernel (same bits), unless skip_nonfinite is set: a guarded step
 * always runs norm partials, begin and the guarded update. */
int f3_optim_step(const f3_optim_config* cfg, float* params, float* state0, float* state1, const float* grads,
                  int64_t n, void* scalars, void* stream);
/* The same update over nranges <= 8 ranges (offsets / lengths in floats, multiples of 4) of the flat
 * buffers in one launch, as the per-layer updates inside f3_net_backward_optim issue it; max_norm
 * and skip_nonfinite must be 0. Elements outside the ranges are untouched. */
int f3_optim_step_ranges(const f3_optim_config* cfg, float* params, float* state0, float* state1,
                         const float* grads, int nranges, const int64_t* lo, const int64_t* len, void* scalars,
                         void* stream);
/* ---- the hyper-parameters as device values: an update recorded into a HIP graph follows a scheduler ----
 * f3_optim_step and f3_rmsprop_step take lr, betas, ... by value, so a graph that recorded them replays
 * the values it was recorded with. The hyper block is device memory of f3_optim_hyper_bytes() bytes
 * (72), 8-byte aligned, holding the fp64 values of f3_optim_config as the host passes them:
 *   byte 0 lr, 8 alpha, 16 eps, 24 momentum, 32 beta1, 40 beta2, 48 weight_decay, 56 max_norm,
 *   64 grad_scale.
 * The update launches of f3_optim_step_hyper read it when they run and derive their arguments with the
 * expressions f3_optim_step evaluates on the host, so both forms give the same bits on the same values.
 * What a recorded step cannot take from the block is its structure, which launches run and which kernel
 * variant: the kind, momentum zero or not, nesterov, max_norm zero or not, and RMSprop with weight_decay
 * 0 and max_norm 0 (f3_rmsprop_step's kernel), skip_nonfinite on or off. The configuration argument
 * supplies those. */
int64_t f3_optim_hyper_bytes(void);
/* lr_scheduler.step(e) (model/main.py:321-322), or any other change of param_groups[0] / TRAIN.MAX_NORM /
 * the world size, made visible to the recorded update: checks cfg's kind and values as f3_optim_step
 * does (finite, non-negative, alpha / betas < 1, grad_scale > 0, no RMSprop momentum), then one
 * one-thread launch on `stream` stores the nine values into the block. To be called outside stream
 * capture, ordered before the replay on the same stream. F3_EINVAL (nothing launched, the block as it
 * was): a bad value, hyper NULL or not 8-byte aligned. cfg's nesterov and skip ranges are not read. */
int f3_optim_hyper_set(const f3_optim_config* cfg, void* hyper, void* stream);
/* optimizer.step() (model/main.py:127) preceded by clip_grad_norm_ (root main.py:108-113), as
 * f3_optim_step issues them: [norm partials], begin, one flat update over n floats, each in the form that
 * reads its values from `hyper`. From cfg only the structure (above) and the skip ranges are taken; its
 * lr, alpha, eps, betas, weight_decay, grad_scale and the magnitudes of momentum and max_norm are ignored.
 * RMSprop with weight_decay 0, max_norm 0 and skip_nonfinite 0 in cfg is f3_rmsprop_step's kernel reading (float) lr,
 * alpha, eps, grad_scale from the block: as that call it touches no scalars (scalars may be NULL) and
 * keeps no step count. Same bits as f3_optim_step / f3_rmsprop_step given the block's values. */
int f3_optim_step_hyper(const f3_optim_config* cfg, float* params, float* state0, float* state1, const float* grads,
                        int64_t n, const void* hyper, void* scalars, void* stream);
/* loss.backward(); [clip_grad_norm_;] optimizer.step() (model/main.py:115-127) in one call: the
 * generalisation of f3_net_backward_rmsprop. Without clipping the begin kernel runs before the
 * private queues fork and each skeleton layer's update is issued on the queue that finishes its
 * gradients; with clipping or skip_nonfinite (both need every gradient) one flat update follows the join. The
 * net's no-gradient entries are skipped (cfg's own skip list is ignored). */
int f3_net_backward_optim(f3_net* net, int batch, float* params, const float* dout, float* grads, float* state0,
                          float* state1, void* scalars, void* workspace, const f3_optim_config* cfg, void* stream);
/* 1 if entry i is a parameter no backward ever writes (its .grad stays None in the reference: the
 * CNN1D's unused fc, GSTCAN_UR_conv.ipynb:493-514), so torch.optim keeps no state for it and applies
 * no decay; 0 otherwise; -1 for a bad index. */
int f3_net_entry_nograd(const f3_net* net, int i);

/* ---- step metrics accumulated on the device (no host sync per batch) ----
 * The accumulator block: device memory of f3_metrics_bytes(C) bytes, 8-byte aligned, zeroed by
 * f3_metrics_reset:
 *   byte 0                fp64   loss_sum          sum of per-batch mean losses
 *   byte 8                int64  batches           number of updates
 *   byte 16               int64  rows              number of rows seen
 *   byte 24               int64  correct[F3_METRICS_MAXK]   one counter per requested k (the rest stay 0)
 *   byte 24 + 8 MAXK      int64  confusion[C*C]    row = true class, column = predicted class
 * True class of a row: arg-max of its soft label (lowest index on a tie), or label_idx. Predicted
 * class: arg-max of out by the same rule. Rank of the target t: the number of classes c with
 * out[c] > out[t], or out[c] == out[t] and c < t; a NaN logit orders above every number and ties with
 * another NaN (torch.topk's order). correct[j] counts the rows with rank < top_k[j]. One 256-thread
 * workgroup per update, integer counts gathered in LDS, every word of the block written by one
 * thread with plain loads and stores (updates on one stream are serial), the loss reduced in a fixed
 * order: the same inputs give the same bits on every run. No call allocates or reads back to the
 * host, so all of them can be captured into a HIP graph. */
#define F3_METRICS_MAXK 8
/* Size of the block for C classes (1 <= C <= 64: the confusion tile is held in LDS); 0 for a bad C. */
int64_t f3_metrics_bytes(int C);
/* Zero the block (the start of an epoch, or of model/main.py:148 valid() / :199 test()). */
int f3_metrics_reset(void* acc, int C, void* stream);
/* Add one batch: replaces cal_top_k_accuracy(output, target, top_k) and the running loss of
 * model/main.py:134-135 (which begin with a copy to the host), and the concatenation of every batch's
 * logits behind the confusion matrix and macro P/R/F1 of model/main.py:189-200, 230-245. out
 * f32[N,C] is the module output. Exactly one of label (f32[N,C], soft or one-hot) and label_idx
 * (i64[N]; an index outside [0,C) counts in rows only) is given. loss != NULL: the batch mean that
 * f3_net_loss / f3_soft_ce wrote, added as (double)*loss. loss == NULL (the eval path):
 * -(1/N) sum_i sum_c y_ic log_softmax(out_i)_c is computed with ce_kernel's row arithmetic, an
 * index label taken as one-hot. top_k: nk <= F3_METRICS_MAXK host ints, passed to the kernel by
 * value. F3_EINVAL: N < 1, C < 1, C > 64, nk > F3_METRICS_MAXK, a k < 1 or k > C, both or neither
 * label forms. */
int f3_metrics_update(void* acc, const float* out, const float* label, const int64_t* label_idx, const float* loss,
                      int N, int C, const int* top_k, int nk, void* stream);
/* Per-tensor gradient L2 norms: replaces the param.grad.norm().item() per parameter of
 * visualize_weights_and_gradients (model/main.py:84-89). norms[s] = scale * ||g[seg_off[s] :
 * seg_off[s] + seg_len[s]]||_2 for s < nseg, norms[nseg] the same over all segments together.
 * seg_off / seg_len: device int64 tables in floats; offsets are multiples of 4 (g 16-byte aligned),
 * lengths arbitrary including 0; elements between segments are never read. Two launches: a
 * workgroup per 8192-float chunk of one segment stores an fp64 partial (an fp32 square is exact in
 * fp64; no float atomics); one workgroup then adds each segment's partials in index order and the
 * segment sums in a fixed order, takes sqrt and scale in fp64 and rounds to fp32 once. scratch: 8-byte
 * aligned device memory of f3_segment_norms_scratch_bytes(sum of lengths, nseg) bytes; the first
 * launch runs one workgroup per 8 bytes of it. A table needing more partials than the scratch holds
 * gives NaN norms, never a read past it. */
int64_t f3_segment_norms_scratch_bytes(int64_t total_len, int nseg);
int f3_segment_norms(const float* g, const int64_t* seg_off, const int64_t* seg_len, int nseg, float* norms,
                     void* scratch, int64_t scratch_bytes, double scale, void* stream);

/* ---- label smoothing and gradient accumulation (TRAIN.LABEL_SMOOTHING, TRAIN.ACCUM_ITER) ----
 * f3_soft_ce_ex / f3_net_loss_ex  <- torch.nn.CrossEntropyLoss(label_smoothing=eps)(pred, label)
 *                                    model/main.py:280 (the loss_fn of :113 train, :175 valid, :226 test)
 * f3_grad_accumulate              <- loss.backward() adding into .grad while optimizer.step() and
 *                                    model.zero_grad() run only every ACCUM_ITER-th batch, model/main.py:115-132
 * torch's rule for probability targets, which it also applies to class indices as one-hot rows:
 *   y' = y (1 - eps) + eps / C
 *   loss = -(1/N) sum_n sum_c y'_nc log_softmax(out_n)_c
 *   dout = (softmax(out) * sum_c y'_c - y') / N           (rows are not renormalised)
 * Exactly one of label (f32[N,C]) and label_idx (i64[N]; an index outside [0,C) is a row of zeros, as
 * f3_metrics_update counts it) is given. dout == NULL: the loss only (the eval loops), nothing else is
 * written. C <= 16 keeps the row in registers, larger C reads it from memory. N <= 4096: one 256-thread
 * workgroup stores the mean (no zeroed loss word, no atomics); at eps = 0 with a soft label this gives
 * the bits of f3_soft_ce / f3_net_loss (the same sums in the same order). Larger N: up to 1024
 * workgroups store one partial each into a block the library owns, and a second launch adds them in
 * index order; such calls must not overlap on two streams. No float atomics: the same inputs give
 * the same bits. F3_EINVAL: eps outside [0,1] or not finite, N < 1, C outside 1..64, both or neither
 * label forms. */
int f3_soft_ce_ex(const float* out, const float* label, const int64_t* label_idx, int N, int C,
                  float label_smoothing, float* loss, float* dout, void* stream);
/* f3_net_loss with smoothing: f3_soft_ce_ex(out, label, NULL, batch, num_class, ...). */
int f3_net_loss_ex(f3_net* net, int batch, const float* out, const float* label, float label_smoothing,
                   float* loss, float* dout, void* stream);
/* f3_soft_ce_w / f3_net_loss_w  <- torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps)(pred, label), the
 *                                  usual first remedy for an imbalanced label set (the fall classes are a
 *                                  small share of UP-Fall's windows); one loss_fn for train, valid and test
 * class_weight: device f32[C], w_c >= 0 and finite (checked by the caller, not here). The launch reads it
 * when it runs: a call recorded into a HIP graph follows a later in-place change of the array. With
 * lsm = log_softmax(out) torch has two normalisations, and the label form picks one:
 *   label (f32[N,C], soft or one-hot): the probability rule
 *     y'   = y (1 - eps) + eps / C
 *     a_nc = w_c y'_nc                  m_n = sum_c a_nc
 *     loss = -(1/N) sum_n sum_c a_nc lsm_nc
 *     dout = (softmax(out)_nc m_n - a_nc) / N                    (rows are not renormalised)
 *   label_idx (i64[N]): the index rule. A row is live when 0 <= t_n < C; every other index is torch's
 *   ignore_index row. Sums run over live rows only:
 *     a_nc = (1 - eps) w_c [c == t_n] + (eps / C) w_c
 *     W    = sum over live n of w_{t_n}
 *     loss = -(1/W) sum_n sum_c a_nc lsm_nc
 *     dout = (softmax(out)_nc m_n - a_nc) / W                    (an ignored row's dout is 0)
 *   W == 0 (no live row, or only rows of weight 0) gives a NaN loss and an all-NaN dout, as torch's 0/0.
 * The row is f3_soft_ce_ex's with a = y' * w (rounded on its own, after y') in the place of y' and m in
 * the place of sum_c y'_c: the same sequential fp32 sums in the same order, the register path up to
 * C = 16 and the row-in-memory path beyond. So all-ones weights give f3_soft_ce_ex's bits under either
 * rule (all indices in range), and weights that are all 2 give twice them (probability rule) or exactly
 * them (index rule, W = 2N). W is accumulated in fp64 in a fixed order and rounded to fp32 once: summed
 * in fp32 its error alone left the dout gate of the tests at N = 257. N <= 4096: one launch, for index
 * labels with a pre-pass over the labels for W. Larger N: up to 1024 workgroups store one partial each
 * into a block the library owns and a second launch adds them in index order; for index labels a
 * launch before them stores the fp64 partials of W, which every workgroup then adds in one fixed
 * order. Such calls must not overlap on two streams. dout == NULL: the loss word only. No float
 * atomics, no allocation, no sync; the same inputs give the same bits. F3_EINVAL: everything
 * f3_soft_ce_ex refuses, and a null class_weight. */
int f3_soft_ce_w(const float* out, const float* label, const int64_t* label_idx, const float* class_weight, int N,
                 int C, float label_smoothing, float* loss, float* dout, void* stream);
/* f3_net_loss_ex with class weights: f3_soft_ce_w(out, label, NULL, class_weight, batch, num_class, ...). */
int f3_net_loss_w(f3_net* net, int batch, const float* out, const float* label, const float* class_weight,
                  float label_smoothing, float* loss, float* dout, void* stream);
/* One micro-batch's gradient into the accumulator: every thread reads the device word *reset_flag;
 * non-zero (the first micro-batch after model.zero_grad(), main.py:132): acc[i] = grads[i], bit for
 * bit; zero: acc[i] = acc[i] + grads[i], one fp32 add per element, the order in which autograd's
 * in-place .grad += g sums. The word is then cleared on the same stream (a memset after the kernel),
 * so a captured graph needs one form of the micro-step; the caller sets it again after its update.
 * acc and grads 16-byte aligned, reset_flag 4-byte aligned, else F3_EINVAL; so is n < 0. n = 0 only
 * clears the word. */
int f3_grad_accumulate(float* acc, const float* grads, int64_t n, int* reset_flag, void* stream);

/* ---- parameter EMA kept on the device ----
 * f3_ema_update <- ema_model.update_parameters(model) after every optimizer.step(), with ema_model =
 *                  torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
 *                  and the default use_buffers=False (timm's ModelEma is the same recurrence), on one flat
 *                  fp32 array.
 * The EMA block: device memory of f3_ema_state_bytes() bytes (16), 8-byte aligned, zeroed by the caller:
 *   byte 0  int64  n_averaged   updates so far
 *   byte 8  fp64   decay
 * The update reads both when it runs, so an update recorded into a HIP graph advances the count and
 * follows a later f3_ema_set_decay on replay (the idea of the hyper block above). There is one form of the
 * kernel, not a by-value form and a device-reading one. */
int64_t f3_ema_state_bytes(void);
/* Checks decay on the host (finite, in [0, 1]), then one one-thread launch on `stream` stores it into the
 * block. To be called outside stream capture, ordered before the replay on the same stream, as
 * f3_optim_hyper_set. F3_EINVAL (nothing launched, the block as it was): a bad decay, state NULL or not
 * 8-byte aligned. */
int f3_ema_set_decay(void* state, double decay, void* stream);
/* n_averaged == 0: ema[i] = params[i], bit for bit (AveragedModel copies on its first update). Otherwise
 *   ema[i] = (float)((double)ema[i] + (1.0 - decay) * ((double)params[i] - (double)ema[i]))
 * evaluated in fp64 in exactly that order, without contraction, and rounded once (get_ema_multi_avg_fn's
 * lerp(ema, p, 1 - decay); the fp64 convention of f3_optim_step). params is not written. n_averaged += 1
 * happens after every element has been written: a second one-thread launch on the same stream, so no thread
 * of the update reads a count that another has advanced. float4 body plus a scalar tail, grid-stride,
 * 256-thread workgroups, at most 4096 of them. No atomics: the same inputs give the same bits on every run
 * and every rank. F3_EINVAL, checked on the host before anything touches the device: a NULL pointer, ema or
 * params not 16-byte aligned, state not 8-byte aligned, n < 0. n == 0 only advances the count. */
int f3_ema_update(float* ema, const float* params, int64_t n, void* state, void* stream);

/* Kernel-level entries used by the unit tests and bench.py: out[N,T_out,V,Cout] = conv_(KT,1)(x)
 * with x [N,T_in,V,Cin] channels-last, w in reference layout [Cout][Cin][KT], bias [Cout]
 * (stgcan.py:24-31 tcn Conv2d). wpack is scratch of Cout*KT*Cin floats for the packed
 * operand; w == NULL reuses what a previous call packed there. precision = F3_PRECISION_*:
 * FP32 -> x/dy are fp32; BF16 -> x/dy are bf16 (the network's bf16 operand tensors);
 * BF16_FP32IN -> fp32 x/dy rounded to bf16 while staging; BF16X3 -> fp32 x/dy, split-bf16 products (wpack
 * then holds the bf16 hi and lo planes of the packed weight). f3_conv_forward also takes
 * F3_CONV_BF16_OUT (bf16 x, out written as bf16 [N,T_out,V,Cout]: the step's tcn output type). */
enum { F3_CONV_BF16_OUT = 3 };
int f3_conv_forward(const void* x, const float* w, const float* bias, float* out, float* wpack, int N, int T_in,
                    int V, int Cin, int Cout, int KT, int stride, int pad, int precision, void* stream);

/* Its gradients: dx = conv^T(dy) [N,T_in,V,Cin]; dw [Cout][Cin][KT] and db [Cout] (overwritten). */
int f3_conv_backward_data(const void* dy, const float* w, float* dx, float* wpack, int N, int T_in, int V, int Cin,
                          int Cout, int KT, int stride, int pad, int precision, void* stream);
int f3_conv_backward_weight(const void* dy, const void* x, float* dw, float* db, int N, int T_in, int V, int Cin,
                            int Cout, int KT, int stride, int pad, int precision, void* stream);
/* The bf16 weight-gradient kernel alone, as the training step launches it per layer: each
 * split of the rows writes its partial dW tile to slab[split][Cout][KT*Cin] (plain stores; the
 * step then sums the splits with a separate reduce launch, not done here). bf16 dy / x;
 * requires Cout % 64 == 0, Cin % 64 == 0, slab_floats >= Cout*KT*Cin. Used to time the kernel. */
int f3_conv_wgrad_packed(const void* dy, const void* x, float* slab, long long slab_floats, int N, int T_in, int V,
                         int Cin, int Cout, int KT, int stride, int pad, void* stream);

/* F3_PRECISION_BF16X3 as the training step runs it (the native split form on the bf16 LDS-DMA kernels):
 * f3_split_x3cat writes each fp32 row x[r][0..C) as the bf16 row of 2C made of 32-channel blocks
 * [x_hi 32 | x_lo 32] (hi = RNE bf16(x), lo = RNE bf16(x - hi)); the packed weight holds, per tap, the
 * blocks [W_hi 32 | W_lo 32] (prep code 4), and a k step issues x_hi W_hi + x_lo W_hi + x_hi W_lo (the
 * split product, ~2^-16 relative) from one staged row piece.
 * f3_conv_forward_x3cat / f3_conv_backward_data_x3cat: x3 / dy3 are such rows ([N,T,V,2Cin] /
 * [N,T_out,V,2Cout]); wpack is scratch of 2 * Cout*KT*Cin bf16 (w == NULL reuses it); out / dx
 * fp32 as f3_conv_forward / f3_conv_backward_data (bias required, epilogue + bias).
 * f3_conv_backward_weight_x3cat: the bf16 weight-gradient GEMM on the same rows, dy_hi x_hi + dy_lo
 * x_hi + dy_hi x_lo (split-K partials summed into dw [Cout][Cin][KT]; db from dy_hi + dy_lo; both
 * overwritten, db may be NULL). dw == NULL: the GEMM alone at the step's split count, partials left in
 * an internal slab (timing). Requires Cin, Cout multiples of 64.
 * f3_conv_step_x3cat: two GEMMs with the epilogues the step gives them, launched alone (measurement,
 * SURVEY §8d; bench.py roofline keys), through the step's own dispatch:
 *   kind F3_STEP_GCN_FWD (stgcan.py:50-56): the gcn 1x1 conv over the graph-mixed rows in3 = [Z_hi | Z_lo]
 *     of Cin = K*C_in channels, out = conv + bias_v[(row % V)][Cout] (the graph-mixed bias), the BN1
 *     batch sums of out added into st_sum / st_sq (fp64); w [Cout][Cin] (T = the frames);
 *   kind F3_STEP_TCN_DGRAD (stgcan.py:112-121, backward): the (9,1) tcn input gradient, stride 1, from
 *     in3 = dh rows of Cout channels into out = dv [N,T,V,Cin], masked where bn1(g) <= 0 (g fp32
 *     [N,T,V,Cin]; BN from gamma / beta and the batch sums bn_sum / bn_sq over bn_count values) with
 *     the BN1-backward sums sum(dv), sum(dv * g_hat) added into st_sum / st_sq; w [Cout][Cin][9].
 *   gcn-only / dgrad-only pointers may be NULL for the other kind. */
#define F3_STEP_GCN_FWD 0
#define F3_STEP_TCN_DGRAD 1
int f3_split_x3cat(const float* x, void* out, int64_t rows, int C, void* stream);
int f3_conv_forward_x3cat(const void* x3, const float* w, const float* bias, float* out, void* wpack, int N, int T_in,
                          int V, int Cin, int Cout, int KT, int stride, int pad, void* stream);
int f3_conv_backward_data_x3cat(const void* dy3, const float* w, float* dx, void* wpack, int N, int T_in, int V,
                                int Cin, int Cout, int KT, int stride, int pad, void* stream);
int f3_conv_backward_weight_x3cat(const void* dy3, const void* x3, float* dw, float* db, int N, int T_in, int V,
                                  int Cin, int Cout, int KT, int stride, int pad, void* stream);
int f3_conv_step_x3cat(int kind, const void* in3, const float* w, void* wpack, float* out, const float* bias_v,
                       const float* g, const float* gamma, const float* beta, const double* bn_sum,
                       const double* bn_sq, float bn_count, double* st_sum, double* st_sq, int N, int T, int V,
                       int Cin, int Cout, void* stream);

/* The 1x1 conv GEMM of the bf16 step with the step's epilogues (stgcan.py:50-56 gcn conv, its
 * input gradient; stgcan.py:123-144 stride-2 residual conv and its input gradient), through the
 * step's own dispatch (the weight-stationary pw_gemm kernel where the shape allows, else igemm).
 * x bf16 [N,T_in,V,Cin] rows; wpack bf16 [Cout][Cin]; out [N,T_out,V,Cout], bf16 (out_bf16 = 1) or
 * fp32. transposed = 0: forward, T_out = (T_in - 1) / stride + 1; transposed = 1: input gradient of a
 * stride-`stride` 1x1 conv whose input had T_out frames. epi: 0 plain, 1 + bias[Cout], 5 + bias with
 * BN sums, 6 + per-joint bias[V][Cout] with BN sums, 32 out += (fp32 out). st_sum / st_sq: fp64
 * [Cout] sums of the fp32 outputs, accumulated (+=). */
int f3_pointwise_conv(const void* x, const void* wpack, const float* bias, void* out, int out_bf16, double* st_sum,
                      double* st_sq, int N, int T_in, int T_out, int V, int Cin, int Cout, int stride, int transposed,
                      int epi, void* stream);

/* RGB spatial-conv branch (BUILD-DEFINED: the reference has RGB frames only in preprocessing,
 * 3_stream/har_create3.py:36-42,101-158, so its parity is unpinned; the north star names it).
 * frames bf16 [B][T][224][224][3]; wpack bf16 [64][192] (the Conv2d(3, 64, 8, stride 8) weight
 * [64][3][8][8] with k = (dy*8 + dx)*3 + ch); feat[B][64] = mean over frames and the 28 x 28 patch
 * grid of relu(conv + bias) (overwritten). The backward gives dw [64][192] (packed order) and
 * db [64] (overwritten) from dfeat [B][64]; scratch holds f3_rgb_scratch_floats(B, T) floats. */
long long f3_rgb_scratch_floats(int B, int T);
int f3_rgb_forward(const void* frames, const void* wpack, const float* bias, float* feat, int B, int T, void* stream);
int f3_rgb_backward(const void* frames, const void* wpack, const float* bias, const float* dfeat, float* dw, float* db,
                    float* scratch, long long scratch_floats, int B, int T, void* stream);

/* Graph mix of one st_gcan block (stgcan.py:54, applied to the gcn input):
 * z[f][w][k][ci] = sum_v A_eff[k][v][w] x[f][v][ci]; backward gives dx and dA_eff (overwritten). */
int f3_graph_mix_forward(const float* A_eff, const float* x, float* z, int frames, int K, int V, int Cin,
                         void* stream);
int f3_graph_mix_backward(const float* A_eff, const float* x, const float* dz, float* dx, float* dA, int frames, int K,
                          int V, int Cin, void* stream);
/* The same with the bf16 mode's operand types: F3_MIX_X_BF16 -> x (and, backward, dz) bf16;
 * F3_MIX_Z_BF16 -> forward z written bf16 (the gcn GEMM's operand, as the step stores it);
 * F3_MIX_X3 -> fp32 operands on the bf16x3 (split-bf16) MFMA kernels of F3_PRECISION_BF16X3;
 * F3_MIX_Z3 (with F3_MIX_X3) -> forward z written as the step stores it for the gcn GEMM: per (frame,
 * node) one bf16 row [z_hi | z_lo] of 2 K Cin (z_hi = RNE bf16(z), z_lo = RNE bf16(z - z_hi)). */
enum { F3_MIX_X_BF16 = 1, F3_MIX_Z_BF16 = 2, F3_MIX_X3 = 4, F3_MIX_Z3 = 8 };
int f3_graph_mix_forward_ex(const float* A_eff, const void* x, void* z, int frames, int K, int V, int Cin, int flags,
                            void* stream);
int f3_graph_mix_backward_ex(const float* A_eff, const void* x, const void* dz, float* dx, float* dA, int frames, int K,
                             int V, int Cin, int flags, void* stream);
/* bf16x3 step: the gcn 1x1 input gradient fused into the graph-mix backward (dZ stays on chip), as
 * stream_backward launches it. dg3: rows [dg_hi | dg_lo] of 2 C bf16 per (frame, node), as f3_split_x3cat
 * writes; w [C][K Cin] is packed into wpack (2 C K Cin bf16) when non-NULL. dx [frames][V][Cin] is
 * overwritten, or added to when accumulate; dA [K][V][V] is overwritten. max_workgroups > 0 sets the
 * grid (a small test makes one workgroup walk several frames; the step passes the mix backward's
 * count); 0 = one round of resident workgroups. F3_EINVAL outside
 * Cin, C in {64, 128, 256}, C >= Cin, K <= 3, V <= 32, K V <= 64. */
int f3_gcn_dgrad_mix_x3(const void* dg3, const float* w, void* wpack, const float* A_eff, const float* x, float* dx,
                        float* dA, int frames, int K, int V, int Cin, int C, int accumulate, int max_workgroups,
                        void* stream);
/* bf16x3 step: the graph mix fused into the gcn forward 1x1 GEMM, as stream_forward launches it (one
 * kernel instead of f3_graph_mix_forward_ex(F3_MIX_X3 | F3_MIX_Z3) + f3_conv_step_x3cat(F3_STEP_GCN_FWD);
 * same bits). x fp32 [frames][V][Cin]; w [C][K Cin] is packed into wpack (2 C K Cin bf16) when non-NULL;
 * bias_v [V][C]. Outputs: z3 rows [z_hi | z_lo] of 2 K Cin bf16 per (frame, node), g fp32 [frames V][C];
 * st_sum / st_sq [C] are added to. F3_EINVAL (nothing written) outside K = 3, Cin = 64, V <= 18,
 * C in {64, 128}. (F3_GCN_FWD_FUSED=0 makes the step launch the pair; this entry always runs the kernel.) */
int f3_gcn_fwd_mix_x3(const float* A_eff, const float* x, const float* w, void* wpack, const float* bias_v, void* z3,
                      float* g, double* st_sum, double* st_sq, int frames, int K, int V, int Cin, int C,
                      void* stream);
/* The block tail as the step launches it, on caller-owned tensors: phases & 1 the forward
 * out = relu(bn2(h) att + res) (res_kind 0 none, 1 identity x, 2 bn_r(r)), phases & 2 its backward (the
 * P1 / P2 / Q2 reduction, then dh / dres). M = N TV rows of C channels; act16: h, r, x, out are bf16.
 * bn2, bnr: rows [gamma | beta | mean | var] of C floats (the running-statistics form); bn2_b, bnr_b:
 * rows [sum | sumsq] of C doubles (the backward's batch sums); att, e [N][C]; dout [M][C] fp32, or
 * dout_nc [N][C], the gradient of the pooled mean (then dout is not read).
 * signs: NULL, or sign_words >= N chunks trips 256 uint16 words, chunks = ceil(TV / 96),
 * trips = ceil(ceil(TV / chunks) / (4 RP)), RP = 256 / (C / 4): the forward sets bit 4u + e of word
 * [(n chunks + chunk) trips + trip][tid] to (stored out > 0) for row chunk_start + trip 4 RP +
 * tid / (C/4) + u RP (clamped to the chunk's last row), channel 4 (tid % (C/4)) + e, for every trip whose
 * u = 0 row lies in the chunk; the backward then reads those words and never out. With NULL it reads out.
 * Outputs: part [chunks][3][N][C] (P1 | P2 | Q2 partial rows; Q2 rows written for res_kind 2 only);
 * dh and (res_kind != 0) dres: fp32 [M][C], or with act16 bf16 (dres of res_kind 1 stays fp32), or with
 * x3 rows [hi | lo] of 2C bf16 (again not the identity dres); dbpart NULL or [chunks][N][C | C] column
 * sums of dh | dres; dgb [4][C] (dgamma2, dbeta2, dgamma_r, dbeta_r) is added to.
 * (F3_BLOCK_SIGNS=0 makes the step run without the words; this entry follows its signs argument.) */
int f3_block_signs_case(int phases, const void* h, const void* r, const void* x, const float* att, const float* e,
                        const float* bn2, const float* bnr, const double* bn2_b, const double* bnr_b,
                        const float* dout, const float* dout_nc, void* out, void* signs, long long sign_words,
                        float* part, void* dh, void* dres, float* dbpart, float* dgb, int N, int TV, int C,
                        int res_kind, int act16, int x3, void* stream);

const char* f3_status_string(int status);

/* ---- TARGCN skeleton model (BASELINE config 2; TRAGCN.py, EmbGCN.py, GRU.py, TA.py) ----
 * f3_targcn_create      <- TARGCN(adj=None, num_nodes=V)          TRAGCN.py:177-205
 *                          (the notebook's call, TARGCN_HAR_conv_10kfold.ipynb cell 3)
 * f3_targcn_entry       <- model.state_dict() keys/shapes (same names, order, shapes;
 *                          PARAM offsets 16-B aligned in the flat parameter array)
 * f3_targcn_forward     <- out = model(pts.permute(0,2,3,1))      TRAGCN.py:207-224
 * f3_targcn_backward    <- loss.backward()
 * f3_soft_ce            <- torch.nn.CrossEntropyLoss()(out, soft labels)
 * Optimizer: f3_rmsprop_step (the notebook's RMSprop). precision: F3_PRECISION_FP32 (exact fp32
 * MFMA, parity mode) or F3_PRECISION_BF16 (bf16 GEMM operands, fp32 accumulate and state). */
typedef struct f3_targcn_config {
  int num_node;   /* V (2..18) */
  int num_class;  /* fc output width */
  int precision;  /* F3_PRECISION_FP32 | F3_PRECISION_BF16 */
} f3_targcn_config;

typedef struct f3_targcn f3_targcn;

int f3_targcn_create(const f3_targcn_config* cfg, f3_targcn** out);
void f3_targcn_destroy(f3_targcn* net);
int f3_targcn_num_entries(const f3_targcn* net);
int f3_targcn_entry(const f3_targcn* net, int i, const char** name, int* kind, int* ndim, int64_t* shape8,
                    int64_t* offset);
int64_t f3_targcn_param_count(const f3_targcn* net);
int64_t f3_targcn_buffer_count(const f3_targcn* net);
int64_t f3_targcn_workspace_bytes(const f3_targcn* net, int batch);
/* source f32[B,T=30,V,3] (the notebook's pts.permute(0,2,3,1)), out f32[B,num_class] logits.
 * TARGCN has no batch statistics or dropout: train and eval forwards are the same computation;
 * the workspace keeps what backward needs. */
int f3_targcn_forward(f3_targcn* net, int batch, const float* params, const float* buffers, const float* source,
                      float* out, void* workspace, void* stream);
/* grads (flat, params layout) are OVERWRITTEN with d(sum dout*out)/dparams of the last forward. */
int f3_targcn_backward(f3_targcn* net, int batch, const float* params, const float* buffers, const float* dout,
                       float* grads, void* workspace, void* stream);
/* Stage timing (measurement aid, no reference counterpart): enable != 0 records HIP events around the
 * two GRU recurrences and the two TA layers of the following f3_targcn_forward / _backward calls on
 * their stream; ms != NULL (after such a pair) waits for them and writes 8 durations in ms:
 * gru_fwd l0, gru_fwd l1, ta_fwd l0, ta_fwd l1, ta_bwd l1, ta_bwd l0, gru_bwd l1, gru_bwd l0. */
int f3_targcn_stage_times(f3_targcn* net, int enable, float* ms);
/* Device-side status of the node-partitioned GRU recurrences (no reference counterpart: the
 * reference's GRU.py:17-27 loop has no inter-workgroup barrier). Each forward clears the barrier
 * error flag; after its recurrences the forward and the backward copy it to a host status word.
 * Returns F3_EDEVICE if a group barrier of the last forward / backward timed out (its outputs are
 * then wrong), F3_OK otherwise. wait = 1 first waits for that copy; wait = 0 reports only a copy
 * that has completed. Every f3_targcn_forward / _backward also returns F3_EDEVICE (and clears
 * the word) when it finds a completed copy flagged by an earlier call. Each call's copy has its own
 * host word (a ring), so a flag is reported once even when later calls run before the host asks. */
int f3_targcn_status(f3_targcn* net, int wait);
/* loss = -(1/N) sum_i sum_c y_ic log_softmax(out_i)_c (soft targets, not renormalised);
 * dout = dloss/dout. loss is overwritten. */
int f3_soft_ce(const float* out, const float* label, int N, int C, float* loss, float* dout, void* stream);

/* ---- musa_model.Model (the model root Multimodal_Fall3/main.py trains; model/musa_model.py) ----
 * f3_musa_create   <- Model(num_class=11, num_point=14, max_frame=300, graph=adjGraph('coco_cut',
 *                     'uniform'), bias=True, edge=True, block_size=41, embed_dim=64, n_stage=1,
 *                     act_type='tanh')                                      main.py:307-320, :492-559
 * f3_musa_entry    <- model.state_dict() keys/shapes (A included: a Parameter, requires_grad False)
 * f3_musa_forward  <- pred = model(data), x f32[N,3,T,V]                   musa_model.py:561-589
 * f3_musa_backward <- loss.backward()
 * Train mode: dropout != 0 enables the DropBlocks (keep_prob 0.9, block 41) and the head's
 * Dropout(0.2), all drawn from a counter hash of `seed` (oracle/musa_cpu.py reproduces it);
 * dropout == 0 is the reference with keep_prob 1 and p = 0. fp32 arithmetic (fp32 MFMA GEMMs). */
typedef struct f3_musa_config {
  int num_point;   /* V (13..18; 14 = coco_cut) */
  int frames;      /* T (8..64; the motion stream has T-1) */
  int num_class;   /* <= 64 */
  int precision;   /* F3_PRECISION_FP32 (0) or F3_PRECISION_BF16: the streams' 1x1 convs (graph conv,
                      residuals, point convs, Sep_TCN) on bf16 MFMA with fp32 accumulate, activations fp32
                      (the root main.py trains under bf16 autocast) */
} f3_musa_config;

typedef struct f3_musa f3_musa;

int f3_musa_create(const f3_musa_config* cfg, f3_musa** out);
void f3_musa_destroy(f3_musa* net);
int f3_musa_num_entries(const f3_musa* net);
int f3_musa_entry(const f3_musa* net, int i, const char** name, int* kind, int* ndim, int64_t* shape8,
                  int64_t* offset);
int64_t f3_musa_param_count(const f3_musa* net);
int64_t f3_musa_buffer_count(const f3_musa* net);
int64_t f3_musa_counter_count(const f3_musa* net);
int64_t f3_musa_workspace_bytes(const f3_musa* net, int batch);
int f3_musa_forward(f3_musa* net, int batch, int training, const float* params, float* buffers, int64_t* counters,
                    const float* x, float* out, void* workspace, unsigned seed, int dropout, void* stream);
/* grads (flat, params layout) are OVERWRITTEN; A and the SepTemporal blocks' edge get zeros (the
 * reference leaves their .grad None: A is frozen, those edges only shape DropBlock masks). */
int f3_musa_backward(f3_musa* net, int batch, const float* params, const float* buffers, const float* dout,
                     float* grads, void* workspace, void* stream);
/* Debug: with F3_MU_GUARD=<bytes> set before the library loads, the workspace plan puts a guard band
 * of that size after every region; this lists the guard offsets (returns the count; -1 on error). */
int f3_musa_guards(const f3_musa* net, int batch, int64_t* offsets, int max);
/* Kernel-level entry (tests, bench.py roofline): the depthwise temporal conv of SepTemporal_Block /
 * Sep_TCN, Conv2d(C, C, (K,1), (S,1), (P,0), groups=C) on channels-last x [N,T_in,V,C] -> y
 * [N,T_out,V,C], w [C][K], b [C]; sums (optional, [2C] fp64, accumulated): BatchNorm batch sums of y. */
int f3_dwconv_t_forward(const float* x, const float* w, const float* b, float* y, double* sums, int N, int T_in,
                        int V, int C, int K, int S, int P, void* stream);

/* ---- SkeletonTransformer (BASELINE config 5; skeleton_transformer.py) ----
 * f3_sktr_create     <- SkeletonTransformer(3, V, T, num_class, 32, 6, 16, 8)   :360-416
 *                       (GSTCAN_HAR_conv_kfold_trans.ipynb; V=14, T=30, 11 classes)
 * f3_sktr_entry      <- model.state_dict() keys/shapes (same names, order, shapes): PARAM
 *                       (16-B aligned offsets), BUFFER (BatchNorm3d running stats), COUNTER
 *                       (num_batches_tracked, int64)
 * f3_sktr_forward    <- out = model(x), x f32[N,3,T,V,M]                          :418-435
 * f3_sktr_backward   <- loss.backward()
 * Train mode randomness is explicit: sd = 18 stochastic-depth factors [block][spatial, temporal,
 * ffn] (torchvision StochasticDepth(p, "batch"): 0 or 1/(1-p); NULL = all 1), and the FFN
 * Dropout(dropout_p) mask comes from a counter hash of (dropout_seed, block, element) that the
 * oracle reproduces (oracle/sktr_cpu.py dropout_keep). Eval mode: running statistics, no
 * randomness. fp32 arithmetic throughout (fp32 MFMA GEMMs). */
typedef struct f3_sktr_config {
  int num_joint;   /* V: spatial attention length (14, 17, 18, 30, 32 supported) */
  int frames;      /* T: temporal attention length (same set) */
  int persons;     /* M >= 1 */
  int num_class;   /* <= 64 */
  int precision;   /* F3_PRECISION_FP32 (0) or F3_PRECISION_BF16: the 6 blocks' Linear layers (qkv, merge,
                      FFN) on bf16 MFMA with fp32 accumulate, activations fp32 in HBM (cfg 5 in bf16) */
} f3_sktr_config;

typedef struct f3_sktr f3_sktr;

int f3_sktr_create(const f3_sktr_config* cfg, f3_sktr** out);
void f3_sktr_destroy(f3_sktr* net);
int f3_sktr_num_entries(const f3_sktr* net);
int f3_sktr_entry(const f3_sktr* net, int i, const char** name, int* kind, int* ndim, int64_t* shape8,
                  int64_t* offset);
int64_t f3_sktr_param_count(const f3_sktr* net);
int64_t f3_sktr_buffer_count(const f3_sktr* net);
int64_t f3_sktr_counter_count(const f3_sktr* net);
int64_t f3_sktr_workspace_bytes(const f3_sktr* net, int batch);
int f3_sktr_forward(f3_sktr* net, int batch, int training, const float* params, float* buffers, int64_t* counters,
                    const float* x, float* out, void* workspace, const float* sd, unsigned dropout_seed,
                    float dropout_p, void* stream);
/* grads (flat, params layout) are OVERWRITTEN; needs the last forward to have been a training one. */
int f3_sktr_backward(f3_sktr* net, int batch, const float* params, const float* buffers, const float* dout,
                     float* grads, void* workspace, void* stream);

/* Debug accessor for tools/tests: device pointer of a per-layer workspace tensor
 * ("x","z","g","h","r","out","att","dh","dv","dg","dZ","dres","bn1_fsum",...) or NULL. */
void* f3_net_debug_tensor(f3_net* net, int batch, void* workspace, int stream, int layer, const char* what);

#ifdef __cplusplus
}
#endif
#endif /* FALL3_H */
