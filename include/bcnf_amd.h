/*
 * bcnf_amd — MI355X-native (gfx950 / CDNA4) CondRealNVP_v2 affine-coupling stack.
 *
 * C-ABI drop-in boundary for the reference's hot path (psaegert/bcnf, src/bcnf/models/cnf.py).
 * Plain pointers and sizes only; every tensor is fp32, row-major, contiguous, device-resident and
 * owned by the caller (the library holds no device memory across calls). Every entry point is
 * stream-ordered on the `stream` argument (a hipStream_t passed as void*), does not synchronise,
 * never throws, and returns BCNF_OK (0) or a nonzero status (see bcnf_status_string).
 *
 * The reference has no native code and hence no FFI; the functions below replace these
 * reference interfaces (file:line relative to /root/reference):
 *
 *   bcnf_stack_forward   <- CondRealNVP_v2.forward layer loop, cnf.py:476-488, with
 *                           ActNorm.forward cnf.py:348-351, ConditionalAffineCouplingLayer.forward
 *                           cnf.py:165-196 (nested MLP cnf.py:98-107) and OrthonormalTransformation.forward
 *                           cnf.py:333-335; log|det J| accumulation cnf.py:477,488; optional
 *                           log_prob = -inn_nll_loss(...,'none') - D/2 log 2pi (utils.py:49-53)
 *   bcnf_stack_backward  <- torch.autograd backward of the above (Trainer._train_batch, trainer.py:268)
 *   bcnf_stack_inverse   <- CondRealNVP_v2.inverse layer loop, cnf.py:499-506 (ActNorm.inverse
 *                           cnf.py:353-354, coupling inverse cnf.py:198-213, orthonormal inverse
 *                           cnf.py:337-339); with cond_index it also serves _sample's tiled
 *                           conditions (cnf.py:577-582) without materialising the tiled features
 *   bcnf_stack_inverse_logdet <- the same loop plus the forward's log|det J| (cnf.py:477,488) at the returned y
 *   bcnf_pack_params     <- (no reference counterpart) re-lays the nn.Module parameters into the
 *                           kernels' LDS-record layout; call after every parameter update
 *   bcnf_nll_forward     <- Trainer._train_batch forward + loss, trainer.py:260-266: the stack forward
 *                           fused with inn_nll_loss(z, log_det_J) (utils.py:40-46, reduction 'mean')
 *   bcnf_nll_backward    <- loss.backward() of that loss through the stack (trainer.py:268)
 *   bcnf_adam_step       <- optimizer.step() of torch.optim.Adam built by the Trainer (trainer.py:136,270)
 *   bcnf_clip_grad_norm  <- torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
 *                           (trainer.py:275, after the step)
 *   bcnf_validation_stats
 *                        <- Trainer._validate_batch's losses, z.mean(0), z.std(0) (trainer.py:293-303) and the
 *                           log_det_J.mean() _train logs (trainer.py:217), with the epoch's `val_loss += loss`
 *   bcnf_linear_forward / bcnf_linear_backward
 *                        <- nn.Linear of FullyConnectedFeatureNetwork (feature_network.py:114-145)
 *   bcnf_wide_*          <- the same stack interfaces for the wide-MLP shapes (FC_large / LSTM_large)
 *   bcnf_rank_count      <- the rank count of compute_y_hat_ranks (eval/calibration.py:42-46)
 *   bcnf_resimulate      <- resimulate's per-draw physics_ODE_simulation map (simulation/resimulation.py:12-18,
 *                           49-56 -> simulation/physics.py:53-160)
 *   bcnf_resim_error_median / bcnf_resim_impacts
 *                        <- notebooks/resimulation.ipynb's reductions of the re-simulated positions: the nanmedian over
 *                           the draws of the squared error, and the impacts (np.diff of z > 0) with their hist2d
 *   bcnf_render_frames   <- camera() per frame of record_trajectory, per camera of generate_data
 *                           (simulation/camera.py:30-150, simulation/sampling.py:366-368)
 *   bcnf_sample_candidates / bcnf_render_lit / bcnf_render_frames_at
 *                        <- generate_data's rejection loop (simulation/sampling.py:287-410): the prior draws, the
 *                           point of impact and the distance filter; the visibility filter's lit frames; the videos
 *                           of the accepted samples
 */
#ifndef BCNF_AMD_H
#define BCNF_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCNF_MAX_HIDDEN 8
#define BCNF_MAX_TENSORS 48
/* Version of the structs and signatures below (2: BcnfStackDesc.gemm_tiling appended; 3: bcnf_wide_fold_backward
 * takes block_lo, block_hi, its _range and _phase variants are gone). bcnf_abi_version() returns the library's; a
 * caller compares it with this macro before passing any struct. */
#define BCNF_AMD_ABI_VERSION 3

int bcnf_abi_version(void);

enum {
  BCNF_OK = 0,
  BCNF_ERR_ARG = 1,          /* invalid descriptor / null pointer / bad size */
  BCNF_ERR_UNSUPPORTED = 2,  /* shape outside this kernel family (see bcnf_stack_supported) */
  BCNF_ERR_HIP = 3           /* reserved (a HIP failure returns BCNF_ERR_HIP_BASE + its hipError_t)       */
};
/* A HIP runtime failure (launch, attribute, memset / copy) returns BCNF_ERR_HIP_BASE + the hipError_t it produced;
 * bcnf_status_string names it. The library keeps no error state between calls. */
#define BCNF_ERR_HIP_BASE 1000

/* Mirrors CondRealNVP_v2.__init__ kwargs (cnf.py:358-375) for the coupling stack. */
typedef struct BcnfStackDesc {
  int32_t size;                      /* D                                     */
  int32_t n_conditions;              /* C (features per sample, h.shape[1])   */
  int32_t n_hidden;                  /* len(nested_sizes)                      */
  int32_t hidden[BCNF_MAX_HIDDEN];   /* nested_sizes                           */
  int32_t n_blocks;                  /* n_blocks                               */
  int32_t act_norm;                  /* 0/1                                    */
  int32_t two_way;                   /* 0/1 (small family: 0 only; wide: both) */
  float dropout;                     /* p of every nn.Dropout in the nested MLP */
  int32_t gemm_tiling;               /* wide family only: 0 = each GEMM's cost-model tiling (use this); t + 1 forces
                                        tiling t (0 <= t <= 10, see bcnf_wide_gemm_test) on every GEMM of the call
                                        (tests / A-B timing). Per call: the library holds no such setting. Appended
                                        in ABI version 2 (BCNF_AMD_ABI_VERSION): C callers built against a version-1
                                        header pass a shorter struct and must be rebuilt. */
} BcnfStackDesc;

/* 1 if this descriptor runs on the fused small-width kernel family, else 0. */
int bcnf_stack_supported(const BcnfStackDesc* desc);

/* Canonical flat layouts (state_dict order of layers.*, frozen orthonormal matrices excluded /
 * separate): n_trainable = #floats of ActNorm + coupling params, n_frozen = (n_blocks-1)*D*D. */
int bcnf_param_count(const BcnfStackDesc* desc, int64_t* n_trainable, int64_t* n_frozen);

/* Bytes of the packed-parameter buffer written by bcnf_pack_params. */
int bcnf_packed_bytes(const BcnfStackDesc* desc, int64_t* bytes);

/* Bytes of the forward->backward workspace for a batch: saved block inputs, dropout masks, loss
 * partials, the hoisted condition projection HP[k][b][16] = h W1h_k^T + b1_k and the Linear-1 deltas
 * D1[k][b][16] written by the backward. Required by every forward and backward call. */
int bcnf_workspace_bytes(const BcnfStackDesc* desc, int64_t batch, int32_t training, int64_t* bytes);

/* Bytes of the gradient scratch ("slab") of a backward over `batch` samples: per-workgroup partial
 * gradients plus the split-K partials of the W1 condition columns. */
int bcnf_slab_bytes(const BcnfStackDesc* desc, int64_t batch, int64_t* bytes);

/* Bytes of the inverse's scratch (the condition projection of h_rows feature rows). */
int bcnf_inverse_scratch_bytes(const BcnfStackDesc* desc, int64_t h_rows, int64_t* bytes);

/* Re-lay params (canonical flat, n_trainable floats) and qmats ((n_blocks-1)*D*D floats) into
 * `packed` (bcnf_packed_bytes). Also writes the ActNorm log|det| constant used by the forward. */
int bcnf_pack_params(const BcnfStackDesc* desc, const float* params, const float* qmats, void* packed,
                     void* stream);

/* Forward of the whole stack given features h (B x C): z (B x D), ldj (B), optional log_prob (B).
 * training != 0 applies dropout with the counter-based RNG keyed by rng_state[0] (seed) and
 * rng_state[1] (offset), both read from DEVICE memory (graph-replay safe). `workspace`
 * (bcnf_workspace_bytes) is required; save != 0 also keeps what bcnf_stack_backward needs. */
int bcnf_stack_forward(const BcnfStackDesc* desc, const void* packed, const float* y, const float* h,
                       int64_t batch, float* z, float* ldj, float* log_prob, int32_t training,
                       const uint64_t* rng_state, void* workspace, int32_t save, void* stream);

/* Backward: given dz (B x D) and dldj (B) (either may be NULL = zeros), writes dh (B x C,
 * overwritten, nullable), dy (B x D, nullable) and the gradient scratch `slab` (bcnf_slab_bytes).
 * With dparams != NULL it then reduces into dparams (canonical flat, n_trainable floats, overwritten);
 * with dparams == NULL the caller runs bcnf_grad_reduce. `training` and `workspace` must be those of
 * the (save != 0) forward call. */
int bcnf_stack_backward(const BcnfStackDesc* desc, const void* packed, const float* h, const float* dz,
                        const float* dldj, int64_t batch, int32_t training, void* workspace, float* dy,
                        float* dh, float* dparams, void* slab, void* stream);

/* dL/dh (B x C, overwritten) = sum_k D1_k W1h_k from the deltas a backward left in `workspace` (what
 * bcnf_stack_backward does itself when its dh != NULL). */
int bcnf_stack_dh(const BcnfStackDesc* desc, const void* packed, const void* workspace, int64_t batch,
                  int32_t training, float* dh, void* stream);

/* Everything after bcnf_stack_backward(dh = dparams = NULL) in one go: dh (nullable) and dparams, as
 * bcnf_stack_dh + bcnf_grad_reduce but with the independent pieces sharing one launch. */
int bcnf_backward_tail(const BcnfStackDesc* desc, const void* packed, const void* slab, const float* h,
                       const void* workspace, int64_t batch, int32_t training, float* dh, float* dparams,
                       void* stream);

/* ---- Folded linear feature network (training fast path; no reference counterpart as a function: it
 * computes the same sums as feature_network.py:114-145's single nn.Linear [X -> C] feeding cnf.py:74-107's
 * condition input, reassociated). With Wf (C x X, row-major) and bf (C, nullable) of that Linear:
 *   Wc = W1h Wf, bc = b1 + W1h bf  (bcnf_pack_params_fold, alongside the training sections of the regular pack
 *                                   -- forward / backward records, W1hR, log-det constant; NOT the inverse records,
 *                                   so its `packed` serves the folded training pass only -- one launch)
 *   HP = x Wc^T + bc               (bcnf_fold_nll_forward: bcnf_nll_forward with x (B x X) in place of h)
 *   dW1h, dWf, dbf from Gx = D1^T [x | 1]  (bcnf_fold_backward_tail, after bcnf_nll_backward(dh = dparams
 *   = NULL) wrote `slab` sized by bcnf_fold_slab_bytes). h and dL/dh are never formed. X + 1 <= 256.
 * x rows are ldx >= X floats apart; ldx % 4 == 0 with a 16-byte aligned x selects float4 row loads (TrainStep's
 * padded pool, bcnf_amd/train.py); the padding columns are never used. */
int bcnf_fold_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t* bytes);
int bcnf_fold_slab_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t batch, int64_t* bytes);
/* A batch gather to run inside bcnf_pack_params_fold's launch (the pack does not read the batch, so the two are
 * independent): the arguments of bcnf_gather_rows2 (cursor = NULL) or bcnf_gather_batch (idx = the epoch order). */
typedef struct BcnfGather2 {
  const int64_t* idx;
  const int64_t* cursor;
  int64_t n;
  const float* src0;
  int32_t cols0;
  float* dst0;
  const float* src1;
  int32_t cols1;
  float* dst1;
} BcnfGather2;
int bcnf_pack_params_fold(const BcnfStackDesc* desc, const float* params, const float* qmats,
                          const float* feat_weight, const float* feat_bias, int32_t in_features, void* packed,
                          float* fold, const BcnfGather2* gather /* nullable */, void* stream);
int bcnf_fold_nll_forward(const BcnfStackDesc* desc, const void* packed, const float* fold, int32_t in_features,
                          const float* y, const float* x, int32_t ldx, int64_t batch, float* z, float* ldj,
                          int32_t training,
                          uint64_t* rng_state, void* workspace, int32_t finalize, float* loss_out, int32_t* guard,
                          void* stream);
/* Pack-free folded training forward: bcnf_pack_params_fold + bcnf_fold_nll_forward in ONE launch. The
 * forward builds its records from `params` / `qmats` through a per-layout table (bcnf_fold_raw_table, built once on
 * the host and copied to the device by the caller), computes h = x Wf^T + bf of its rows on the matrix cores and the
 * condition projection from h (the unfolded sums, so the loss rounds like bcnf_nll_forward on h rather than like the
 * folded Wc), and writes into `packed` exactly what bcnf_nll_backward + bcnf_fold_backward_tail read (backward
 * records, W1hR) -- `packed` serves that training pass only. gather (nullable): the rows come from the pools
 * (src0 [*][D], src1 [*][cols1]; n == batch), y / x are then unused and the forward writes the gathered rows into
 * dst0 / dst1 (ldx = cols1), as bcnf_pack_params_fold's gather did. BCNF_ERR_UNSUPPORTED where the table does not
 * apply (no ActNorm, one block, X > 128) -- use the two-launch form there. bcnf_fold_raw_table_bytes: the table's
 * size in bytes; bcnf_fold_raw_table fills `host_table` (host memory) with it. */
int bcnf_fold_raw_table_bytes(const BcnfStackDesc* desc, int32_t in_features, int64_t* bytes);
int bcnf_fold_raw_table(const BcnfStackDesc* desc, int32_t in_features, void* host_table);
int bcnf_fold_train_forward(const BcnfStackDesc* desc, const float* params, const float* qmats, const void* table,
                            const float* feat_weight, const float* feat_bias, int32_t in_features,
                            const BcnfGather2* gather /* nullable */, const float* y, const float* x, int32_t ldx,
                            int64_t batch, void* packed, float* z, float* ldj, int32_t training,
                            uint64_t* rng_state, void* workspace, int32_t finalize, float* loss_out, int32_t* guard,
                            void* stream);
/* Adam fused into bcnf_fold_backward_tail (nullable argument): every gradient the tail produces -- the flat coupling
 * parameters (slot 0), the feature Linear's weight (1) and bias (2, NULL without bias) -- also takes its
 * torch.optim.Adam update where it is produced, with the end-of-step bookkeeping of bcnf_adam_step_bookkeep
 * (step count, epoch cursor, logged values; done_counter: device int32, 0 between launches). For a training step
 * whose clip-after-step cannot be observed (trainer.py:273-275; see bcnf_adam_step_bookkeep): it replaces that
 * step's Adam launch. The gradients are still written. */
typedef struct BcnfFoldAdam {
  float* params[3];
  float* exp_avg[3];
  float* exp_avg_sq[3];
  float* step;
  double lr, beta1, beta2, eps, weight_decay;
  int64_t* advance_cursor;
  int64_t cursor_modulo;
  const float* log_values;
  float* log_history;
  int32_t* done_counter;
  const int32_t* guard;
} BcnfFoldAdam;
int bcnf_fold_backward_tail(const BcnfStackDesc* desc, const void* packed, const void* slab, const float* x,
                            int32_t ldx, int32_t in_features, const float* feat_weight, const float* feat_bias,
                            const void* workspace, int64_t batch, int32_t training, float* dparams,
                            float* dfeat_weight, float* dfeat_bias, const BcnfFoldAdam* adam /* nullable */,
                            void* stream);
/* Test hook (host arithmetic only, no launch): how one bcnf_fold_backward_tail call at `batch` rows spreads its slab
 * reduce over its three launches (k_fold_tail, k_fold_gx, k_fold_finish; the call computes its grids from the same
 * function). The reduce has n_red workgroups of 128 slab floats each over the slab stride S; each launch runs its own
 * workgroups first, then one contiguous range of the reduce workgroups (k_fold_gx's range is empty: DESIGN.md 7).
 * out[0] = n_red, out[1] = S (floats), out[2 + 2t] / out[3 + 2t] = first / count of launch t's range (t = 0, 1, 2 in
 * launch order; a count may be 0), out[8 + t] = launch t's grid size, out[11 + t] = its own workgroups (grid -
 * count). `out`: 14 int64. Checked by tests/test_fold_tail_plan.py. */
int bcnf_fold_tail_plan(const BcnfStackDesc* desc, int32_t in_features, int64_t batch, int64_t* out);

/* Deterministic (fixed-order) reduction of a backward's gradient scratch into dparams, including the
 * W1 condition columns (split-K GEMM of D1 with h). Replaces autograd's implicit batch reduction. */
int bcnf_grad_reduce(const BcnfStackDesc* desc, const void* slab, const float* h, const void* workspace,
                     int64_t batch, int32_t training, float* dparams, void* stream);

/* Inverse of the whole stack: y (N x D) from z (N x D). h has h_rows rows; row r uses feature row
 * cond_index[r] when cond_index != NULL (h_rows may then be anything), else row r (h_rows == N).
 * `scratch`: bcnf_inverse_scratch_bytes(h_rows) -- the projection is computed once per feature row.
 * Without dropout (eval, or p = 0) the stack runs on the matrix cores, 16 rows per wave;
 * training mode with dropout keeps the row-layout kernel. A row's result does not depend on its position. */
int bcnf_stack_inverse(const BcnfStackDesc* desc, const void* packed, const float* z, const float* h,
                       int64_t h_rows, const int64_t* cond_index, int64_t n_rows, float* y, int32_t training,
                       const uint64_t* rng_state, void* scratch, void* stream);

/* Inverse (eval) that also returns the density of what it returns: ldj (N) = log|det dz/dy| at the returned y, the
 * value bcnf_stack_forward(y, h) writes to its ldj (same sign), and log_prob (N, nullable) = -0.5 |z|^2 + ldj -
 * D/2 log 2pi with z the rows as passed (utils.py:49-53 at the draw). A one-way coupling's inverse passes the identity
 * half through unchanged (cnf.py:198-213), so the s = tanh(s') it forms at block k is the forward's s at y: the
 * kernel keeps their running sum (one add per coupling output) and adds the packed ActNorm constant; no second pass
 * over the n_rows rows. Eval only (no dropout: the draw is deterministic). y is bit-identical to bcnf_stack_inverse's.
 * two_way descriptors return BCNF_ERR_UNSUPPORTED (the reference's two_way inverse is not its forward's inverse, so
 * there is no density), as does a layout outside the matrix-core inverse. Arguments are validated before any HIP
 * call; NULL y / ldj is BCNF_ERR_ARG. Scratch as bcnf_stack_inverse. A row's result does not depend on its position. */
int bcnf_stack_inverse_logdet(const BcnfStackDesc* desc, const void* packed, const float* z, const float* h,
                              int64_t h_rows, const int64_t* cond_index, int64_t n_rows, float* y, float* ldj,
                              float* log_prob /* nullable */, void* scratch, void* stream);

/* ---- NLL training pass (forward + inn_nll_loss + backward without any host round trip) ---------
 * bcnf_nll_forward = bcnf_stack_forward (workspace required, save on) plus per-workgroup partials of
 *   nll = mean_b(0.5 |z_b|^2 - ldj_b)  (utils.py:40-46). With finalize != 0 a one-workgroup launch then
 *   writes loss_out[0] = loss = (nll + 0 * mse) / (1 + 0), loss_out[1] = nll, loss_out[2] = mse = 0 (the
 *   Trainer's three logged values with hybrid_weight == 0) and, when dropout is active, advances
 *   rng_state[1] by one (so graph replays draw fresh masks). With finalize == 0 that reduction is
 *   deferred to bcnf_nll_backward(loss_out, rng_state) (saves a launch in a training step). No kernel
 *   synchronises across workgroups. */
int bcnf_nll_forward(const BcnfStackDesc* desc, const void* packed, const float* y, const float* h, int64_t batch,
                     float* z, float* ldj, int32_t training, uint64_t* rng_state, void* workspace, int32_t finalize,
                     float* loss_out, int32_t* guard, void* stream);

/* Backward through loss_out w.r.t. y, h and the stack parameters: dz = z * g / B, dldj = -g / B with
 * g = dloss[0] + dloss[1], dloss being the device cotangent of loss_out[0..2] (NULL means d loss = 1,
 * i.e. loss.backward(); mse carries no gradient). z is the forward's output. With loss_out != NULL it
 * also performs the forward's deferred loss reduction (finalize == 0 there). Otherwise as
 * bcnf_stack_backward. */
int bcnf_nll_backward(const BcnfStackDesc* desc, const void* packed, const float* h, const float* z,
                      const float* dloss, int64_t batch, int32_t training, void* workspace, float* dy,
                      float* dh, float* dparams, void* slab, float* loss_out, uint64_t* rng_state, int32_t* guard,
                      void* stream);

/* ---- Optimizer ------------------------------------------------------------------------------------
 * Tensors are passed as arrays of n_tensors (<= BCNF_MAX_TENSORS) device pointers + element counts and
 * treated as one concatenated index space. bcnf_grad_partials(total) = floats of the partials buffer the kernels
 * below write / read: one sum of squared gradients per workgroup, plus one slot for their pre-reduced total.
 * Empty tensors: the pointer arrays are required, but the pointer of a tensor with numel[i] == 0 may be NULL (what
 * torch gives as an empty tensor's data pointer); such a tensor takes no part. A set whose total is 0 still runs
 * its one workgroup, which forms no address into any tensor (the kernels' clamped-index loads are skipped when
 * there is no element to clamp to): partial 0 and the total norm are 0, and the step count, cursor and log
 * bookkeeping happen as for any other set. */
int64_t bcnf_grad_partials(int64_t total_numel);

/* One torch.optim.Adam step (amsgrad = maximize = False) over every tensor; hyper-parameters are
 * doubles (derived scalars such as 1 - beta2 are formed in double and rounded once, as torch does);
 * `step` is the device-side float step count (as Adam(capturable=True) keeps it): the update uses
 * step + 1, and advance_step != 0 then stores it (a one-thread launch). With advance_step == 0 the
 * caller advances it later (bcnf_clip_grad_norm(advance_step = step)), saving that launch. With
 * grad_partials != NULL the per-workgroup sums of squared gradients for bcnf_clip_grad_norm are written. */
int bcnf_adam_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, float* step, double lr, double beta1,
                   double beta2, double eps, double weight_decay, float* grad_partials, int32_t advance_step,
                   const int32_t* guard, void* stream);

/* bcnf_adam_step (step count advanced in the same launch) whose LAST workgroup to finish also does the end-of-step
 * bookkeeping of bcnf_clip_grad_norm: epoch cursor advance and logged values -> log_history[3 * cursor]. It
 * replaces Adam + clip for a training step whose clip-after-step (trainer.py:275) cannot be observed -- one that
 * is followed, inside the same captured graph, by the next step's backward, which overwrites every gradient the
 * clip would scale (the reference discards the returned norm). done_counter: device int32, 0 between launches
 * (the last workgroup resets it). No squared-gradient partials are written. */
int bcnf_adam_step_bookkeep(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const int64_t* numel, float* step, double lr, double beta1,
                            double beta2, double eps, double weight_decay, int64_t* advance_cursor,
                            int64_t cursor_modulo, const float* log_values, float* log_history, int32_t* done_counter,
                            const int32_t* guard, void* stream);

/* Per-workgroup sums of squared gradients (when no bcnf_adam_step produced them). */
int bcnf_grad_sumsq(int32_t n_tensors, float* const* grads, const int64_t* numel, float* grad_partials, void* stream);

/* clip_grad_norm_(max_norm, norm_type=2): total = sqrt(sum partials); g *= min(max_norm/(total+1e-6), 1).
 * total_norm (device float, nullable) receives the pre-clip norm. End-of-step bookkeeping (nullable):
 * advance_step[0] += 1 (a deferred Adam step count) and advance_cursor[0] = (cursor + 1) % cursor_modulo
 * (an epoch cursor of bcnf_gather_batch). */
int bcnf_clip_grad_norm(int32_t n_tensors, float* const* grads, const int64_t* numel, const float* grad_partials,
                        float max_norm, float* total_norm, float* advance_step, int64_t* advance_cursor,
                        int64_t cursor_modulo, const float* log_values, float* log_history, const int32_t* guard,
                        void* stream);

/* Training-loop guard, int32[4] in device memory (nullable everywhere): [BCNF_GUARD_CHECK] is set by the
 * host (the Trainer checks for divergence after epoch 10, trainer.py:168); the loss finalize of
 * bcnf_nll_forward / bcnf_nll_backward raises [BCNF_GUARD_DIVERGED] when loss > 1e5 or NaN and, one step
 * later, [BCNF_GUARD_HALTED], which makes that step's RNG advance, bcnf_adam_step and bcnf_clip_grad_norm
 * no-ops. Steps can so be replayed back to back without a host sync per step: the host reads the logged
 * values afterwards and raises where the reference would, with the state it would have had.
 * bcnf_clip_grad_norm also stores log_values[0..2] (the step's loss, nll, mse) into
 * log_history[3 * cursor ...] (cursor = advance_cursor[0] before the advance, else 0); log_history may be
 * pinned host memory (system-scope stores). */
#define BCNF_GUARD_CHECK 0
#define BCNF_GUARD_DIVERGED 1
#define BCNF_GUARD_HALTED 2
#define BCNF_GUARD_CHECK_GLOBAL 3
#define BCNF_GUARD_WORDS 4

/* Data parallel form of the divergence check (trainer.py:168 on the loss every rank logs): the host leaves
 * [BCNF_GUARD_CHECK] at 0, so no rank's loss finalize judges its local shard, and sets
 * [BCNF_GUARD_CHECK_GLOBAL]; after the gradient all-reduce this one-thread launch raises [BCNF_GUARD_DIVERGED]
 * when the all-reduced loss global_values[0] > 1e5 or NaN (unless the step is already halted). Every rank sees
 * the same value, so every rank halts on the same step; the next step's loss finalize turns DIVERGED into
 * HALTED exactly as in the single-process case. */
int bcnf_guard_check_global(const float* global_values, int32_t* guard, void* stream);

/* The same bookkeeping as a one-thread launch. */
int bcnf_advance_counters(float* step, int64_t* cursor, int64_t n_batches, void* stream);

/* ---- Batch feed: dst0[r] = src0[idx[r]], dst1[r] = src1[idx[r]] (row-major rows of cols0 / cols1
 * floats) in one launch -- the shuffled-batch gather of the Trainer's DataLoader (trainer.py:164-166)
 * from device-resident data. */
int bcnf_gather_rows2(const int64_t* idx, int64_t n, const float* src0, int32_t cols0, float* dst0,
                      const float* src1, int32_t cols1, float* dst1, void* stream);
/* The same for batch number cursor[0] of an epoch order (device int64 indices, batch per batch): rows
 * order[cursor[0] * batch + r]. The cursor is advanced by a later launch (bcnf_clip_grad_norm /
 * bcnf_advance_counters), so the gather needs no cross-workgroup synchronisation (graph-replay safe). */
int bcnf_gather_batch(const int64_t* order, const int64_t* cursor, int64_t batch, const float* src0, int32_t cols0,
                      float* dst0, const float* src1, int32_t cols1, float* dst1, void* stream);

/* ---- nn.Linear (row-major, weight out_features x in_features) ------------------------------------ */
int bcnf_linear_forward(const float* x, const float* weight, const float* bias, int64_t rows, int32_t in_features,
                        int32_t out_features, float* y, void* stream);
/* Scratch bytes bcnf_linear_backward needs for its split-K weight gradient. */
int64_t bcnf_linear_work_bytes(int64_t rows, int32_t in_features, int32_t out_features);
/* dx (nullable) = dy W; dweight = dy^T x and dbias (nullable) = column sums of dy, both overwritten
 * (fixed-order split-K reduction through `work`). dweight may be NULL only when dbias is NULL too. A refused call
 * (BCNF_ERR_ARG) launches nothing; rows = 0 zero-fills dweight and dbias. */
int bcnf_linear_backward(const float* x, const float* weight, const float* dy, int64_t rows, int32_t in_features,
                         int32_t out_features, float* dx, float* dweight, float* dbias, void* work, void* stream);
/* One hidden layer of a FullyConnectedFeatureNetwork, nn.Linear -> nn.GELU() -> nn.Dropout(p) (feature_network.py:
 * 128-134, the reference runs them as three ATen ops), in ONE launch: a = mask GELU(x W^T + b) with the exact-erf
 * GELU, and g (nullable) = mask GELU'(x W^T + b) for the backward. mask = 1 / (1 - p) or 0 from an in-kernel
 * Philox4x32-10 stream when rng (device uint64 [seed, offset], read only) is given and p > 0, else 1; salt separates
 * the layers of one network. Same element-wise distribution as torch's dropout, not its bits. */
int bcnf_linear_gelu_forward(const float* x, const float* weight, const float* bias, int64_t rows, int32_t in_features,
                             int32_t out_features, float p, const uint64_t* rng, int32_t salt, float* a, float* g,
                             void* stream);
/* Backward of bcnf_linear_gelu_forward from dL/da and its g: dL/dpre = da * g is formed as the operands are loaded
 * (never stored), then as bcnf_linear_backward (same work bytes). */
int bcnf_linear_gelu_backward(const float* x, const float* weight, const float* da, const float* g, int64_t rows,
                              int32_t in_features, int32_t out_features, float* dx, float* dweight, float* dbias,
                              void* work, void* stream);

/* ---- Wide-MLP family (trajectory_FC_large / trajectory_LSTM_large class: nested_sizes = [H] * NH with H too
 * wide for the register-resident kernels above, e.g. [526] * 5, C = 1360, 26 blocks) ----------------------------
 * Same BcnfStackDesc, same canonical flat parameter layout (state_dict order) and the same reference interfaces
 * as bcnf_stack_forward / _backward / _inverse / bcnf_nll_* above (cnf.py:49-107, 165-213, 312-354, 467-508;
 * utils.py:40-53; trainer.py:260-268), built from fp32-MFMA GEMMs (v_mfma_f32_32x32x2_f32) with fused
 * bias / GELU / dropout / gradient epilogues and per-sample link kernels (coupling, log|det J|, orthonormal mix,
 * ActNorm). Requirements: equal nested sizes, size <= 32. two_way couplings (cnf.py:176-186) run as two
 * half-couplings per block (nn_a then nn_b), with the reference's inverse (cnf.py:198-213).
 * The wide family takes the canonical flat params directly plus its own packed buffer (padded weight copies,
 * bcnf_wide_pack after every parameter update). */
int bcnf_wide_supported(const BcnfStackDesc* desc);
/* Canonical flat sizes as bcnf_param_count, for the wide family (two_way: nn_a then nn_b per block). */
int bcnf_wide_param_count(const BcnfStackDesc* desc, int64_t* n_trainable, int64_t* n_frozen);
int bcnf_wide_packed_bytes(const BcnfStackDesc* desc, int64_t* bytes);
/* save != 0: the forward keeps every activation, GELU-derivative factor and block input for the backward. */
int bcnf_wide_workspace_bytes(const BcnfStackDesc* desc, int64_t batch, int32_t save, int64_t* bytes);
int bcnf_wide_inverse_scratch_bytes(const BcnfStackDesc* desc, int64_t h_rows, int64_t n_rows, int64_t* bytes);
int bcnf_wide_pack(const BcnfStackDesc* desc, const float* params, const float* qmats, void* packed, void* stream);
/* z (B x D), ldj (B); nll_part (nullable) receives 0.5 |z_b|^2 - ldj_b per sample (the per-sample inn_nll_loss,
 * utils.py:49-53 with reduction 'none'). Dropout as bcnf_stack_forward (device rng_state; the caller advances the
 * offset, or bcnf_wide_nll_finalize does). */
int bcnf_wide_forward(const BcnfStackDesc* desc, const float* params, const void* packed, const float* y,
                      const float* h, int64_t batch, float* z, float* ldj, float* nll_part, int32_t training,
                      const uint64_t* rng_state, void* workspace, int32_t save, void* stream);
/* loss_out[0..2] = [loss, nll, mse = 0] from the forward's per-sample NLL terms (workspace of that forward), plus
 * the dropout RNG advance and the divergence guard, as bcnf_nll_forward's finalize. */
int bcnf_wide_nll_finalize(const BcnfStackDesc* desc, const void* workspace, int64_t batch, int32_t save,
                           float* loss_out, uint64_t* rng_state, int32_t* guard, void* stream);
/* Backward of a save != 0 forward. nll == 0: cotangents dz (B x D) / dldj (B), either nullable. nll != 0: through
 * the NLL, dz = z g / B and dldj = -g / B with g = dloss[0] + dloss[1] (dloss nullable = 1), z = the forward's
 * output. Writes dy, dh (nullable) and dparams (canonical flat, every element overwritten; nullable). */
int bcnf_wide_backward(const BcnfStackDesc* desc, const float* params, const void* packed, const float* h,
                       const float* z, const float* dz, const float* dldj, const float* dloss, int32_t nll,
                       int64_t batch, void* workspace, float* dy, float* dh, float* dparams, void* stream);
/* Folded last feature Linear of a wide stack (trajectory_FC_large: h = x Wf^T + bf, feature_network.py:114-145 with
 * the stack's condition projection cnf.py:98-107): with x1 = [x | 1 | 0] (B x xp, xp = roundup(X + 1, 4), 16-B
 * aligned rows), wfb = [Wf | bf | 0] (C x xp) and Wcb = W0h_all wfb (nv*HP x xp):
 *   prepare:  Wcb = W0h_all wfb (after bcnf_wide_pack; wcb holds nv*HP*xp floats, nv*HP = bcnf_wide_param_count's
 *             layout: blocks x sides x 16-padded hidden width)
 *   forward:  P = x1 Wcb^T, then the unchanged stack (save is implied: a backward follows)
 *   backward: through the NLL (dloss nullable = 1): Gx = dZ0^T x1 (gx_scratch, nv*HP*xp floats), dW0h = Gx wfb^T
 *             into dparams, dwfb = W0h_all^T Gx (C x xp: [dWf | dbf]), dx = dZ0 Wcb (B x xp, columns < X).
 * h and dL/dh are never formed. */
int bcnf_wide_fold_prepare(const BcnfStackDesc* desc, const void* packed, const float* wfb, int32_t xp, float* wcb,
                           void* stream);
int bcnf_wide_fold_forward(const BcnfStackDesc* desc, const float* params, const void* packed, const float* y,
                           const float* x1, int32_t xp, const float* wcb, int64_t batch, float* z, float* ldj,
                           int32_t training, const uint64_t* rng_state, void* workspace, void* stream);
/* The backward runs over real blocks [block_lo, block_hi); the whole backward is (0, nb). Data parallelism that
 * overlaps the gradient exchange with the rest of the backward (trainer.py:244-277 is the single-process
 * step it splits) makes one call per contiguous block range, in descending order over one forward's workspace, the
 * first with block_hi = nb and the last with block_lo = 0. A call runs the backward chain until blocks
 * [block_lo, block_hi) are complete and writes their canonical parameter gradients,
 * dparams[bcnf_wide_block_offset(block_lo) .. bcnf_wide_block_offset(block_hi)); the block_lo = 0 call also writes
 * dwfb and dx. Results equal the one (0, nb) call bit for bit; calls out of that order leave the outputs undefined. */
int bcnf_wide_fold_backward(const BcnfStackDesc* desc, const float* params, const void* packed, const float* x1,
                            int32_t xp, const float* wfb, const float* wcb, const float* z, const float* dloss,
                            int64_t batch, void* workspace, float* gx_scratch, float* dparams, float* dwfb, float* dx,
                            int32_t block_lo, int32_t block_hi, void* stream);
/* Canonical flat offset of real block `block`'s first trainable parameter (its ActNorm, cnf.py:296-335 module order);
 * block = nb gives the parameter count. Host-only. */
int bcnf_wide_block_offset(const BcnfStackDesc* desc, int32_t block, int64_t* offset);
/* Rows of the padded projection (nv*HP) of a wide stack. */
int bcnf_wide_proj_rows(const BcnfStackDesc* desc, int64_t* rows);
/* Inverse: as bcnf_stack_inverse (cond_index selects feature rows; scratch = bcnf_wide_inverse_scratch_bytes). */
int bcnf_wide_inverse(const BcnfStackDesc* desc, const float* params, const void* packed, const float* z,
                      const float* h, int64_t h_rows, const int64_t* cond_index, int64_t n_rows, float* y,
                      int32_t training, const uint64_t* rng_state, void* scratch, void* stream);
/* As bcnf_stack_inverse_logdet for the wide family (one-way stacks; two_way: BCNF_ERR_UNSUPPORTED): the link kernels
 * carry ldj[row] across their launches and add each block's ActNorm constant once; the GEMM chain is unchanged. */
int bcnf_wide_inverse_logdet(const BcnfStackDesc* desc, const float* params, const void* packed, const float* z,
                             const float* h, int64_t h_rows, const int64_t* cond_index, int64_t n_rows, float* y,
                             float* ldj, float* log_prob /* nullable */, void* scratch, void* stream);
/* ---- Hybrid training loss: prediction head + MSE (cnf.py: prediction_head = nn.Linear(C, D); trainer.py:261-269
 * with hybrid_weight w > 0: loss = (nll + w * MSE(prediction_head(h), y)) / (1 + w)) ---------------------------------
 * x (B x K, rows ldx >= K floats apart; columns K .. ldx are never read into a result), W (D x K), bias (D, nullable),
 * y (B x D); 2 <= D <= 32, K >= 1, B >= 1. fp32 MFMA (v_mfma_f32_16x16x4_f32). `work` is caller-owned, 16-byte
 * aligned, bcnf_head_work_bytes(B, K, D) bytes: the residual r = x W^T + bias - y (its first B * D floats), the
 * forward's squared-error partials and the split-K partials of dW / dbias. The three launching functions are
 * stream-ordered, hold no state and reduce in a fixed order without float atomics: the same inputs give the same
 * bits on every call and replay. `weight` is the host scalar w (>= 0).
 *   forward:  r and per-workgroup sums of r^2 into `work`.
 *   backward: e = (2 g / (B D)) r with g = dloss[0] w / (1 + w) + dloss[2], dloss the device cotangent of the three
 *             logged values (NULL = [1, 0, 0]); dW (D x K) = e^T x and dbias (D) = column sums of e, split over the
 *             batch and reduced by a second small launch; dx (B x K, rows ldd >= K apart) = e W, written, or with
 *             accumulate_dx != 0 added into the existing dx (the stack's dL/dh: no separate add). Every output is
 *             nullable.
 *   finalize: after the stack's NLL finalize wrote loss_vals = [nll, nll, 0]: loss_vals[2] = mse = mean(r^2),
 *             loss_vals[0] = (nll + w mse) / (1 + w); with guard[BCNF_GUARD_CHECK_GLOBAL] set the combined loss is
 *             judged as bcnf_guard_check_global does (> 1e5 or NaN raises [BCNF_GUARD_DIVERGED]); a step already
 *             [BCNF_GUARD_HALTED] is left alone. One workgroup. */
int bcnf_head_work_bytes(int64_t batch, int32_t in_features, int32_t out_features, int64_t* bytes);
int bcnf_head_mse_forward(const float* x, int64_t ldx, int32_t in_features, const float* weight_matrix,
                          const float* bias, const float* y, int64_t batch, int32_t out_features, void* work,
                          void* stream);
int bcnf_head_mse_backward(const float* x, int64_t ldx, int32_t in_features, const float* weight_matrix, void* work,
                           const float* dloss, float weight, int64_t batch, int32_t out_features, float* dweight,
                           float* dbias, float* dx, int64_t ldd, int32_t accumulate_dx, void* stream);
int bcnf_hybrid_finalize(float* loss_vals, const void* work, int64_t batch, int32_t out_features, float weight,
                         int32_t* guard, void* stream);

/* ---- Validation statistics (Trainer._validate_batch, trainer.py:279-303, and what _train logs from its last batch,
 * trainer.py:213-217) ---------------------------------------------------------------------------------------------
 * z (B x D), ldj (B), pred and y (B x D each; both NULL when hybrid_weight == 0). One launch, one workgroup, writes
 * the 4 + 2 D floats
 *   row = [loss, nll, mse, mean(ldj), z.mean(0)[D], z.std(0)[D]]
 * with nll = mean_b(0.5 sum_d z^2 - ldj), mse = mean((pred - y)^2) (0 without pred), loss = (nll + mse w) / (1 + w)
 * evaluated in fp32 from the rounded nll and mse, and z.std the unbiased estimate (NaN at B = 1, as torch.std). Every
 * sum is fp64 in an order fixed by (B, D) -- no atomics; same inputs, same bits -- and the deviations are a second pass
 * around the fp64 mean. epoch_sum (3 doubles, nullable): after the row is written one thread adds (loss, nll, mse) as
 * doubles, so launches of one stream accumulate in batch order like the Trainer's `val_loss += loss`. cursor
 * (nullable; an epoch cursor of bcnf_gather_batch): the row is written at row + cursor[0] * (4 + 2 D) and the cursor
 * then advanced modulo n_batches, the last thing the launch does. 1 <= D <= 32 (else BCNF_ERR_UNSUPPORTED), B >= 1,
 * w >= 0 and finite; nothing is launched on a bad argument. */
int bcnf_validation_stats(const float* z, const float* ldj, const float* pred, const float* y, int64_t batch,
                          int32_t size, float weight, float* row, double* epoch_sum, int64_t* cursor,
                          int64_t n_batches, void* stream);

/* ---- Transformer feature networks (feature_network.py:183-307: MultiHeadAttention, TransformerBlock) ---------------
 * The two pieces of a block that are not a Linear layer. fp32, stream-ordered, stateless; every sum runs in a fixed
 * order (same inputs, same bits). A shape outside the stated limits returns BCNF_ERR_ARG and launches nothing.
 *
 * Attention core: out = softmax(q k^T / sqrt(head_dim)) v per (sample, head), no mask. q, k, v, out (and dout, dq, dk,
 * dv) are (B * S) rows of n_heads * head_dim floats, `ld` >= n_heads * head_dim floats apart; head h is columns
 * h * head_dim .. h * head_dim + head_dim - 1 (the head split and concatenation are index arithmetic; columns past
 * n_heads * head_dim of a row are neither read nor written). 1 <= S <= 64, 1 <= head_dim <= 64. lse is
 * (B, n_heads, S): the log-sum-exp of each score row, which the backward recomputes the probabilities from. */
int bcnf_attn_forward(const float* q, const float* k, const float* v, int64_t batch, int32_t seq_len, int32_t n_heads,
                      int32_t head_dim, int64_t ld, float* out, float* lse, void* stream);
int bcnf_attn_backward(const float* q, const float* k, const float* v, const float* out, const float* lse,
                       const float* dout, int64_t batch, int32_t seq_len, int32_t n_heads, int32_t head_dim,
                       int64_t ld, float* dq, float* dk, float* dv, void* stream);
/* Residual + LayerNorm: y = LayerNorm(x + r) over rows of d contiguous floats (biased variance, eps inside the square
 * root; gamma (d), beta (d, nullable)); mean / rstd (rows) are saved for the backward. 1 <= d <= 1024.
 * backward: dx (rows x d, nullable) is the gradient of x AND of r; dgamma / dbeta (d, nullable) are summed per
 * workgroup into `work` (caller-owned, bcnf_add_layernorm_work_bytes(rows, d) bytes; may be NULL when neither is
 * wanted) and reduced over the workgroups, in order, by a second launch. */
int bcnf_add_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta, int64_t rows,
                               int32_t d, float eps, float* y, float* mean, float* rstd, void* stream);
int bcnf_add_layernorm_work_bytes(int64_t rows, int32_t d, int64_t* bytes);
int bcnf_add_layernorm_backward(const float* x, const float* r, const float* gamma, const float* mean,
                                const float* rstd, const float* dy, int64_t rows, int32_t d, float* dx, float* dgamma,
                                float* dbeta, void* work, void* stream);

/* ---- LSTM layer (feature_network.py:310-398: VerboseLSTM's single-layer nn.LSTM modules under DualDomainLSTM) ------
 * The serial part of ONE layer, both directions in one launch; gate order and formulas are torch's (i, f, g, o):
 *   gates_t = P_t + h_{t-1} W_hh^T + b_hh,  c_t = s(f) c_{t-1} + s(i) tanh(g),  h_t = s(o) tanh(c_t),  h_0 = c_0 = 0,
 * the reverse direction walking t = S - 1 .. 0. The input projection P = x W_ih^T + b_ih is NOT part of it (one
 * bcnf_linear_forward per direction over all B * S rows), nor are the weight gradients: dW_ih, db_ih and dx come from
 * bcnf_linear_backward on the backward's dP, dW_hh (and db_hh = db_ih) from the same call with x := h_prev, the output
 * sequence shifted one step against the direction with zeros at its first step. fp32, stream-ordered, stateless, no
 * atomics; every sum runs in a fixed order (same inputs, same bits).
 *
 * Limits: hidden % 16 == 0, 16 <= hidden <= 128, seq_len >= 1, batch >= 1, dirs 1 or 2, ldp >= 4 * hidden,
 * ldo >= dirs * hidden; anything else returns BCNF_ERR_ARG and launches nothing. The *_rev pointers are read only
 * when dirs == 2; b_hh_* may be NULL (no bias).
 *
 * Layouts. p_fwd / p_rev (and dp_fwd / dp_rev): (B * S) rows, row b * S + t, `ldp` floats apart, 4 * hidden floats
 * each, gate g at columns g * hidden ... w_hh_*: (4 * hidden, hidden) row-major. out (and dout): (B * S) rows `ldo`
 * floats apart, direction d at columns d * hidden .. (d + 1) * hidden - 1 (no concatenation; columns past
 * dirs * hidden of a row are neither read nor written). gates (dirs, B * S, 4 * hidden) and cells (dirs, B * S,
 * hidden), contiguous: the activated gates and c_t the backward reads; both NULL (inference: nothing saved) or both
 * given. tanh(c_t) is recomputed. backward: dp_* receive the gradient of the pre-activation gates, step by step
 * against the forward's order (dh = dout_t + dh_rec, the gate derivatives, dP_t, dh_rec = dP_t W_hh). */
int bcnf_lstm_forward(const float* p_fwd, const float* p_rev, int64_t ldp, const float* w_hh_fwd,
                      const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev, int64_t batch,
                      int32_t seq_len, int32_t hidden, int32_t dirs, float* out, int64_t ldo, float* gates,
                      float* cells, void* stream);
int bcnf_lstm_backward(const float* dout, int64_t ldo, const float* gates, const float* cells, const float* w_hh_fwd,
                       const float* w_hh_rev, int64_t batch, int32_t seq_len, int32_t hidden, int32_t dirs,
                       float* dp_fwd, float* dp_rev, int64_t ldp, void* stream);

/* ---- CNN layer (models/cnn.py: Conv2d -> ReLU -> Dropout -> MaxPool2d(2, 2), the unit the CNN feature network
 * repeats) --------------------------------------------------------------------------------------------------------
 * ONE layer per launch and direction; nothing at the convolution's resolution is written:
 *   pre = conv2d(x, weight, bias), stride 1, zero padding (pad_h, pad_w): (n_images, c_out, Hc, Wc) with
 *         Hc = height + 2 pad_h - ksize + 1, Wc = width + 2 pad_w - ksize + 1,
 *   a   = relu(pre) * keep / (1 - p),
 *   y   = the 2 x 2 / stride-2 maximum of a, floor mode: (n_images, c_out, Hc / 2, Wc / 2); an odd last row or column
 *         of pre belongs to no window (and receives no gradient).
 * fp32, NCHW contiguous: x (n_images, c_in, height, width), weight (c_out, c_in, ksize, ksize), bias (c_out,
 * nullable). Stream-ordered, stateless, no atomics; every sum runs in a fixed order (same inputs, same bits).
 *
 * Limits: 1 <= ksize <= 8, 1 <= c_in, c_out <= 32, 0 <= pad_h, pad_w <= ksize - 1, Hc >= 2 and Wc >= 2,
 * n_images >= 1, 0 <= p < 1; anything else returns BCNF_ERR_ARG and launches nothing.
 *
 * code (uint8, the shape of y; NULL = inference, nothing saved): bits 0-1 = the winner's position in its window,
 * 0 .. 3 in row-major order (the first of equal values wins, as torch's max_pool2d), bit 2 = the winner is positive --
 * the only case in which a gradient flows (ReLU active and the unit kept).
 *
 * Dropout (p > 0 and rng_state != NULL, else none): rng_state is the device (seed, offset) pair of the library's
 * other dropout layers. Element e -- the flat index of a unit in (n_images, c_out, Hc, Wc) -- keeps iff
 * u32(e) >= thresh32(p) = round(p 2^32), where u32(e) is word e & 3 of Philox4x32-10 with
 *   counter (e >> 2 low half, e >> 2 high half, offset low half, offset high half),
 *   key     (seed low half ^ salt * 0x9E3779B9, seed high half ^ 0x40000000)
 * -- the feature Linear layers' key has 0x80000000 there, so the same (seed, offset, salt) gives both kinds of layer
 * independent draws. The backward needs no RNG: a dropped unit is a zero, which never wins with bit 2 set.
 *
 * backward: g = dy * [bit 2] / (1 - p) at each window's winner, zero elsewhere; dx (the shape of x, nullable: the
 * first layer's input is the images) = the transposed convolution of g, dweight / dbias (nullable) are summed per
 * (workgroup, row slice) into `work` (caller-owned, 16-byte aligned, bcnf_conv_block_work_bytes(...) bytes; may be NULL
 * when neither is wanted) and reduced in index order by a second launch. */
int bcnf_conv_block_forward(const float* x, const float* weight, const float* bias, int64_t n_images, int32_t c_in,
                            int32_t height, int32_t width, int32_t c_out, int32_t ksize, int32_t pad_h, int32_t pad_w,
                            float p, const uint64_t* rng_state, int32_t salt, float* y, uint8_t* code, void* stream);
int bcnf_conv_block_work_bytes(int64_t n_images, int32_t c_in, int32_t height, int32_t width, int32_t c_out,
                               int32_t ksize, int32_t pad_h, int32_t pad_w, float p, int64_t* bytes);
int bcnf_conv_block_backward(const float* x, const float* weight, const float* dy, const uint8_t* code,
                             int64_t n_images, int32_t c_in, int32_t height, int32_t width, int32_t c_out,
                             int32_t ksize, int32_t pad_h, int32_t pad_w, float p, float* dx, float* dweight,
                             float* dbias, void* work, void* stream);

/* ---- Calibration (eval/calibration.py:20-48, compute_y_hat_ranks) -----------------------------------------------
 * counts[i * dim + d] += #{ s < n_draws : y_hat[(s * n_rows + i) * dim + d] < y[i * dim + d] } for the (n_draws, n_rows,
 * dim) draws of sample(outer=True); counts is uint32 and accumulates, so draws can be fed in chunks. */
int bcnf_rank_count(const float* y_hat, const float* y, int64_t n_draws, int64_t n_rows, int32_t dim, uint32_t* counts,
                    void* stream);

/* ---- Re-simulation (simulation/resimulation.py:21-59 -> physics.py:53-160, physics_ODE_simulation per draw) -------
 * Replaces the ProcessPoolExecutor map of resimulate_trajectory (resimulation.py:12-18, 49-56) over every (draw j,
 * trajectory i). Physics parameter q (physics.py:53-72 order: x0_x x0_y x0_z v0_x v0_y v0_z g_x g_y g_z w_x w_y w_z
 * b m rho r a_x a_y a_z) is y_hat[(j * n_traj + i) * dim + param_cols[q]] (float32, or float64 with y_hat_f64) when
 * param_cols[q] >= 0 (the model predicts it: ParameterIndexMapping.dictify), else fixed[i * 19 + q] (the trajectory's
 * data_dict value, resimulation.py:53). tgrid = np.arange(0, T, dt) (steps >= 1 entries). Output
 * x[((i * n_draws + j) * steps + s) * 3 + c] (float64, = np.array(X_resimulation_list)). The velocity ODE is
 * integrated in fp64 by an adaptive Dormand-Prince 5(4) pair at (rtol, atol) between grid times; max_attempts bounds
 * the step attempts per trajectory. param_cols is a HOST array of 19; every other pointer is device memory.
 * attempts / status (int32 per (i, j)) are optional; status is BCNF_RESIM_*; a
 * trajectory that is not OK is NaN from the first grid time it could not reach. */
#define BCNF_RESIM_NPARAM 19
#define BCNF_RESIM_OK 0
#define BCNF_RESIM_NONFINITE 1   /* non-finite right-hand side at t = 0 (e.g. zero wind: 0/0 in physics.py:42) */
#define BCNF_RESIM_STEPS 2       /* step size underflow or max_attempts exhausted (divergent draw) */
int bcnf_resimulate(const void* y_hat, int32_t y_hat_f64, int64_t n_draws, int64_t n_traj, int32_t dim,
                    const int32_t* param_cols, const double* fixed, const double* tgrid, int32_t steps, double dt,
                    int32_t break_on_impact, double rtol, double atol, int32_t max_attempts, double* x,
                    int32_t* attempts, int32_t* status, void* stream);

/* ---- Re-simulation statistics (notebooks/resimulation.ipynb: what the notebook reduces bcnf_resimulate's positions
 * to). x is the (n_traj, n_draws, steps, 3) float64 output of bcnf_resimulate, device memory, steps >= 1; both entry
 * points reduce over the draw axis, check their arguments before any device call and do nothing for
 * n_traj * n_draws == 0.
 *
 * bcnf_resim_error_median: err[i * steps + s] =
 * np.nanmedian(np.nanmean((x - observed[:, None])**2, axis=3), axis=1)[i][s], bit for bit. observed is (n_traj,
 * steps, 3), float32 or (observed_f64) float64. Per draw j:
 * e_k = (x[i][j][s][k] - (double)observed[i][s][k])^2, each operation rounded on its own (no FMA), the value is
 * (the sum of the non-NaN e_k in the order k = 0, 1, 2) / their number, or NaN when all three are NaN. err is the
 * median of the c non-NaN values: the middle one for odd c, (lo + hi) / 2 for even c, NaN for c = 0. The median is
 * found by an exact sort of the values' bit patterns inside one workgroup's LDS, so the result is the same bits on
 * every run. One deviation from numpy: for odd c and n_draws < 600 numpy's small-array path returns (v + v) / 2,
 * which is inf for v > DBL_MAX / 2; this returns v.
 * n_draws <= BCNF_RESIM_ERROR_MAX_DRAWS (a column of draws, padded to a power of two, is sorted in LDS: 16384 keys of
 * 8 bytes = 128 KB of the 160 KB a gfx950 workgroup has); more returns BCNF_ERR_UNSUPPORTED and launches nothing.
 *
 * bcnf_resim_impacts: with above[s] = x[i][j][s][2] > 0 (false for NaN), a transition of draw (i, j) is a step s in
 * [0, steps - 2] with above[s] && !above[s + 1], i.e. an index of np.diff((x[i, :, :, 2] > 0).astype(int)) == -1: the
 * last step still above ground. step[i * n_draws + j] is the first transition or -1, position[(i * n_draws + j) * 3 + k]
 * = x[i][j][step][k] or NaN, transitions[i * n_draws + j] their number (thrust can lift a ball again). With edges
 * (n_edges float64 values, strictly increasing, device memory, used for both axes) and hist (n_traj, n_edges - 1,
 * n_edges - 1) int32, hist[i] counts the (x, y) = x[i][j][s][0 .. 1] of EVERY transition of trajectory i as
 * np.histogram2d(xs, ys, bins=edges) does: bin np.searchsorted(edges, v, 'right') - 1 per axis (first index: the x bin),
 * a value equal to the last edge in the last bin, values outside the edges, NaN and +-inf dropped. hist is written
 * whole (one workgroup owns hist[i], counted in LDS). edges and hist are both NULL or both given.
 * 2 <= n_edges <= BCNF_RESIM_HIST_MAX_EDGES (the (n_edges - 1)^2 int32 counters and the edge table live in one
 * workgroup's LDS: 147,460 bytes at 192 edges; 128 edges need 65,540); more returns BCNF_ERR_UNSUPPORTED and launches
 * nothing. */
#define BCNF_RESIM_ERROR_MAX_DRAWS 16384
#define BCNF_RESIM_HIST_MAX_EDGES 192
int bcnf_resim_error_median(const double* x, const void* observed, int32_t observed_f64, int64_t n_traj,
                            int64_t n_draws, int32_t steps, double* err, void* stream);
int bcnf_resim_impacts(const double* x, int64_t n_traj, int64_t n_draws, int32_t steps, const double* edges,
                       int32_t n_edges, int32_t* step, double* position, int32_t* transitions, int32_t* hist,
                       void* stream);

/* ---- Camera (simulation/camera.py:74-150 camera(), looped by record_trajectory, camera.py:30-71, and over the two
 * cameras of a sample by generate_data, sampling.py:366-368) -----------------------------------------------------------
 * Renders n_frames frames of BCNF_RENDER_HEIGHT x BCNF_RENDER_WIDTH pixels in one launch, one workgroup per frame.
 * Frame f: n_samples points ball_pos[f] + sigma[f] z_s (sigma = radius / 1.644854; z_s the three standard normals of
 * sample s, below), seen from camera c = cam_index[f] (0 <= c < n_cams; anything else gives an all-zero frame with
 * n_in[f] = -1): v = normalise(point - cam_pos[c]), ph = atan2(v . basis[c][1], v . basis[c][0]),
 * th = atan2(v . basis[c][2], v . basis[c][0]) with basis[c] = (cam_dir, cam_orthogonal, cam_orthogonal_z) as rows, all
 * in fp64. ph_edges (WIDTH + 1) and th_edges (HEIGHT + 1) are the np.linspace edge tables np.histogram2d builds; a sample
 * counts in bin (i, j) iff ph_edges[i] <= ph < ph_edges[i + 1] and th_edges[j] <= th < th_edges[j + 1], the last edge
 * of each table included, and is dropped outside the tables (or when an angle is NaN) -- the bins of
 * np.searchsorted(edges, x, 'right') - 1, decided against the tables themselves. images[f][HEIGHT - 1 - j][i] =
 * count / n_in[f] (the fp64 quotient rounded once to float, or kept as double with images_f64), n_in[f] = the samples
 * of frame f that were counted; a frame with n_in[f] == 0 is all zeros = np.flipud(vals.T) of camera.py:139-150.
 * counts (int32, the images' layout) and n_in (int32 per frame) are optional. images and counts 16-byte aligned; every
 * pointer is device memory. Stream-ordered, stateless, LDS atomics only: same inputs, same bits.
 *
 * Draw rule (the reference draws from numpy's global stream, which no kernel can follow; bcnf_amd/render.py:
 * standard_normals restates this rule in numpy and is its normative statement). Sample s of frame f draws
 *   (w0, w1, w2, w3) = Philox4x32-10 with
 *     counter (s, first_frame + f, offset low half, offset high half),
 *     key     (seed low half, seed high half ^ 0xC0000000)   -- the dropout layers' keys carry 0x80000000 / 0x40000000
 *                                                               or neither there, so one seed gives independent draws;
 *   u_i = (w_i + 0.5) 2^-32, exact in fp64 and strictly inside (0, 1);
 *   Box-Muller in fp64:  z_s = ( sqrt(-2 ln u0) cos(2 pi u1),  sqrt(-2 ln u0) sin(2 pi u1),  sqrt(-2 ln u2) cos(2 pi u3) ),
 *   with 2 pi = 6.283185307179586.
 * A frame's draws depend on (s, first_frame + f, offset, seed) only: not on n_frames, on the launch a frame is rendered
 * in, or on n_samples (the first n of a longer draw are the draw of n). first_frame + n_frames <= 2^32. */
#define BCNF_RENDER_WIDTH 160
#define BCNF_RENDER_HEIGHT 90
int bcnf_render_frames(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                       const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                       const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset, int64_t first_frame,
                       void* images, int32_t images_f64, int32_t* counts, int32_t* n_in, void* stream);
/* bcnf_render_frames with the draw rule's frame index of frame f given by frame_index[f] (device, uint32, n_frames
 * entries) instead of first_frame + f: the frames of samples that are not consecutive in the rule (the accepted
 * candidates of generate_data) in one launch. Everything else as above. */
int bcnf_render_frames_at(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                          const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                          const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset,
                          const uint32_t* frame_index, void* images, int32_t images_f64, int32_t* counts, int32_t* n_in,
                          void* stream);
/* The lit-frame pass of generate_data's visibility filter (sampling.py:370-372 needs only whether a frame is empty):
 * the same device code, draws and range test as bcnf_render_frames, writing n_in[f] only -- no histogram, no image.
 * n_in[f] equals what bcnf_render_frames writes for the same frame. frame_index as in bcnf_render_frames_at, or NULL
 * for first_frame + f. */
int bcnf_render_lit(const double* ball_pos, const int32_t* cam_index, const double* sigma, int64_t n_frames,
                    const double* cam_pos, const double* basis, int32_t n_cams, const double* ph_edges,
                    const double* th_edges, int32_t n_samples, uint64_t seed, uint64_t offset, int64_t first_frame,
                    const uint32_t* frame_index, int32_t* n_in, void* stream);

/* ---- Candidates of generate_data (simulation/sampling.py:287-410): sample_ballistic_parameters (sampling.py:156-284),
 * the runaway and underground tests, calculate_point_of_impact (physics.py:246-276) and accept_traveled_distance
 * (sampling.py:145-153) for candidates first_candidate .. first_candidate + n_candidates - 1 in one launch, fp64.
 *
 * Draw rule (bcnf_amd/generate.py:sample_candidates_host restates it in numpy and is its normative statement).
 * Slot s of candidate c, attempt t, draws
 *   (w0, w1, w2, w3) = Philox4x32-10 with
 *     counter (c low half, c high half, s, t),
 *     key     (seed low half, seed high half ^ 0x60000000)     -- BCNF_GEN_KEY_TAG: the dropout layers' keys carry
 *                                                                 0x80000000 / 0x40000000 or neither, the camera's
 *                                                                 0xC0000000;
 *   u_i = (w_i + 0.5) 2^-32;
 *   uniform(lo, hi)  = lo + (hi - lo) u0                                                     (t = 0)
 *   normal           = sqrt(-2 ln u0) cos(2 pi u1), 2 pi = 6.283185307179586                  (t = 0)
 *   gamma(k, theta)  = Marsaglia-Tsang without the squeeze: k' = k (k >= 1) or k + 1, d = k' - 1/3, c = 1 / sqrt(9 d);
 *                      attempt t = 0, 1, ...: x = the normal of (w0, w1), v = (1 + c x)^3; accepted when v > 0 and
 *                      ln u2 < x^2 / 2 + d - d v + d ln v; the value is d v theta, times u3^(1/k) first when k < 1
 *                      (u3 of the accepted attempt). t < 1000.
 * Slots follow the call order of sample_ballistic_parameters for two cameras: 0 x0_xy, 1 phi, 2 x0_z, 3 v0_xy, 4 phi_v,
 * 5 v0_z, 6 w_xy, 7 phi_w, 8 w_z, 9 a, 10 phi_a, 11 theta_a, 12 g, 13 rho, 14 r_ball, 15 Cd, 16 m, 17 cam_radian,
 * 18 cam_radius, 19-20 cam_angle, 21-22 cam_heights, 23 the uniform of accept_traveled_distance, 24 that of
 * accept_visibility. kind[s] / p0[s] / p1[s] (HOST arrays of BCNF_GEN_NSLOT) give slot s's distribution: uniform
 * (min, max), gaussian (mean, std: the draw is the standard normal, the pair feeds the transformation) or gamma
 * (shape, scale); transform[s] the reference's expression on the raw draw n: NONE n, SQRT_ABS sqrt(|n|) std + mean,
 * AFFINE n std + mean, CBRT_ABS cbrt(|n|) std + mean, SQRT sqrt(n).
 *
 * params[c][BCNF_GEN_NCOL] (device, float64), in the key order of the reference's dict: 0-2 x0, 3-5 v0, 6-8 g
 * (0, 0, -g), 9-11 w, 12 b = rho A Cd, 13 m, 14-16 a, 17-18 cam_radian_array (cam1_radian, the drawn one), 19 r,
 * 20 A = pi r^2, 21 Cd, 22 rho, 23 cam_radius, 24-25 cam_angles, 26-27 cam_heights, 28-29 the two filter uniforms.
 * code[c]: PENDING, RUNAWAY (g_z + a_z > 0), UNDERGROUND (x0_z < 0) or DISTANCE (accept_traveled_distance said no);
 * poi[c][3] / distance[c]: the point of impact and its distance to x0, NaN for RUNAWAY / UNDERGROUND. The march is
 * calculate_point_of_impact's with its default dt = 0.1: the position advances by x + v dt with the velocity at the
 * start of the interval, the velocity by the Dormand-Prince pair of bcnf_resimulate at (rtol, atol), impact is
 * x + v (-x.z / v.z) at the first z < 0, and (999, 999, 999) after 120 s or once the velocity is not finite.
 * With do_filter == 0 every candidate stays PENDING and nothing marches (poi / distance NaN). */
#define BCNF_GEN_NSLOT 25
#define BCNF_GEN_NCOL 30
#define BCNF_GEN_KEY_TAG 0x60000000u
#define BCNF_GEN_UNIFORM 0
#define BCNF_GEN_GAUSSIAN 1
#define BCNF_GEN_GAMMA 2
#define BCNF_GEN_XF_NONE 0
#define BCNF_GEN_XF_SQRT_ABS 1
#define BCNF_GEN_XF_AFFINE 2
#define BCNF_GEN_XF_CBRT_ABS 3
#define BCNF_GEN_XF_SQRT 4
#define BCNF_GEN_PENDING 0
#define BCNF_GEN_RUNAWAY 1
#define BCNF_GEN_UNDERGROUND 2
#define BCNF_GEN_DISTANCE 3
int bcnf_sample_candidates(const int32_t* kind, const int32_t* transform, const double* p0, const double* p1,
                           uint64_t seed, int64_t first_candidate, int64_t n_candidates, double cam1_radian,
                           int32_t do_filter, double rtol, double atol, int32_t max_attempts, double* params,
                           double* poi, double* distance, int32_t* code, void* stream);


const char* bcnf_status_string(int status);

/* ---------------------------------------------------------------------------------------------------------------
 * TEST-ONLY entry points. Not part of the drop-in boundary (no reference interface maps to them; INTEGRATION.md
 * binds none of them): exported so the GPU tests can poison LDS and exercise single GEMM tilings through ctypes.
 * ------------------------------------------------------------------------------------------------------------- */
/* Test hook (no reference counterpart): fill every CU's LDS with `value` (one full-LDS workgroup per CU, several
 * rounds), so a test can check that a following launch never reads LDS it did not write (the pack-free forward's
 * K padding, tests/test_gpu_fold.py). */
int bcnf_lds_fill(float value, void* stream);
/* Test hook for the GEMM tiles: C (M x N) = A B with (layout & 15) 0 = A[m][k] B[n][k], 1 = A[m][k] B[k][n],
 * 2 = A[k][m] B[k][n], 3 = A[k][m] B[n][k]; layout >> 4 forces a tiling as BcnfStackDesc.gemm_tiling (0 = the
 * dispatcher's choice, t + 1 = tiling t: 0 = 128x128 and 1 = 64x64 on v_mfma_f32_32x32x2_f32, 2 = 128x48, 3 = 128x48
 * on 8 waves, 4 = 96x48 on 6 waves (v_mfma_f32_16x16x4_f32), 5 / 6 / 7 = LDS-DMA tiling C auto / large / 48x48,
 * 8 = 176x176 on 11 waves (strided x strided layouts only), 9 / 10 = tiling W 96x48 / 48x48 (layout 0 only, the B band
 * resident in LDS, K <= 768); a forced tiling that does not apply to the layout / K runs as 64x64 (tiling 1);
 * leading dimensions and K multiples of 4, 16-byte aligned bases. Strided operands ([K][M] / [K][N] rows) are read
 * as whole float4 up to roundup4(M) / roundup4(N) columns in EVERY row, the last one included: allocate K * ld
 * floats for them (a tight (K - 1) * ld + M buffer is read out of bounds). */
int bcnf_wide_gemm_test(int32_t layout, int32_t M, int32_t N, int32_t K, const float* A, int64_t lda, const float* B,
                        int64_t ldb, float* C, int64_t ldc, void* stream);
/* Test hook (host arithmetic only, no launch): the workspace / G-region plan of one folded wide backward call
 * (bcnf_wide_fold_backward) at `batch` rows over blocks [block_lo, block_hi), dL/dx and [dWf | dbf] wanted or
 * not: out[0] = training workspace floats, out[1] = offset of the G region in it, out[2] = G region floats, out[3] =
 * the feature-side split-K partials at the region's end, out[4] / out[5] = offset (within G) / floats of the range's
 * parameter-gradient split-K scratch, out[6] / out[7] = the dL/dx / [dWf | dbf] partial needs. Checked by
 * tests/test_native_abi.py and under AddressSanitizer (tools/asan_host.sh). */
int bcnf_wide_backward_plan(const BcnfStackDesc* desc, int64_t batch, int32_t xp, int32_t want_dx, int32_t want_dwfb,
                            int32_t block_lo, int32_t block_hi, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* BCNF_AMD_H */
