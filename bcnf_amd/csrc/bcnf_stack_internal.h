// Small stack family: the seam between its translation units. bcnf_stack.hip (the C ABI) checks the arguments and
// calls one plain function per kernel family; each family's file defines its launchers and is the only file that
// launches its kernels (bcnf_rt::launch keeps a kernel's granted LDS in a static of the instantiation: one kernel,
// one translation unit). Nothing here is exported.
//
//   bcnf_stack_layout.h   constants, make_layout, LDS sizes, workspace offsets, dispatch_nh
//   bcnf_stack_rec.h      RecF / RecB / ActRec, Stage, mlp_forward*, mix, nll_finalize, sum_rows4, layout_matches
//   bcnf_stack.hip        C ABI, forward_impl / backward_impl, the pack kernels and the pack-free table builder
//   bcnf_stack_fwd.hip    k_forward, k_nll_finalize
//   bcnf_stack_inv.hip    k_hp, k_inverse (training mode), k_inverse_mfma (eval)
//   bcnf_stack_bwd.hip    k_backward
//   bcnf_stack_tail.hip   k_dh, k_bwd_tail, k_dw1h_reduce; folded: k_fold_tail, k_fold_gx, k_fold_finish
#pragma once
#include "bcnf_stack_layout.h"

#pragma GCC visibility push(hidden)
namespace bcnf_small {

// ---- bcnf_stack_fwd.hip ----
// The pack-free forward's extra operands (bcnf_fold_train_forward; k_forward's RawArgs).
struct RawForward {
  const float* P;          // canonical flat parameters
  const float* Q;          // orthonormal matrices [nb - 1][D][D]
  const uint32_t* table;   // [RAW_NS][256] (build_raw_table)
  const float* wf;         // feature Linear weight [C][X]
  const float* bf;         // its bias [C] (nullable)
  const float* ypool;      // y rows [*][D]
  float* ydst;             // gathered y rows [B][D] (nullable: no copy)
  const float* xpool;      // x rows [*][ldx]
  float* xdst;             // gathered x rows [B][ldx] (nullable: no copy)
  const int64_t* idx;      // batch row b -> pool row idx[(cursor ? cursor[0] * B : 0) + b]; NULL: row b
  const long long* cursor;
  float* pk;               // packed buffer: PB and W1hR are written here
  int X, ldx;
};
// The condition projection runs inside k_forward, on h, or on x with the folded feature Linear (`fold`: Wc / bc of
// fold_layout(L, X, ldx) instead of the packed W1h^T / b1).
int launch_forward(const BcnfLayout& L, const float* pk, const float* y, const float* h, const float* fold, int X,
                   int ldx, long long B, float* z, float* ldj, float* logp, bool drop, const uint64_t* rng,
                   float* arec, float* part, const RawForward* raw, hipStream_t st);
int launch_nll_finalize(const float* part, int nparts, long long B, float* loss_out, uint64_t* rng_w, int32_t* guard,
                        hipStream_t st);

// ---- bcnf_stack_inv.hip ----
int launch_hp(const BcnfLayout& L, const float* pk, const float* h, long long R, float* hp, hipStream_t st);
int launch_inverse(const BcnfLayout& L, const float* pk, const float* z, const float* hp, long long R,
                   const int64_t* cond_index, long long N, float* y, bool drop, const uint64_t* rng, hipStream_t st);
int launch_inverse_logdet(const BcnfLayout& L, const float* pk, const float* z, const float* hp, long long R,
                          const int64_t* cond_index, long long N, float* y, float* ldj, float* logp, hipStream_t st);

// ---- bcnf_stack_bwd.hip ----
int launch_backward(const BcnfLayout& L, const float* pk, const float* dz, const float* dldj, const float* dloss,
                    int nll, long long B, const float* arec, float* dy, float* d1, float* slab, const float* part,
                    float* loss_out, uint64_t* rng_w, int32_t* guard, hipStream_t st);

// ---- bcnf_stack_tail.hip ----
// Slab reduce + W1 condition-part split-K (+ dL/dh when dh is given) -> dparams; then the dL/dh tiles alone.
int launch_tail(const BcnfLayout& L, const float* pk, const float* slab, const float* h, const float* ws,
                long long B, float* dh, float* dparams, hipStream_t st);
int launch_dh(const BcnfLayout& L, const float* pk, const float* ws, long long B, float* dh, hipStream_t st);
// The folded tail's three launches (host arithmetic only; bcnf_fold_tail_plan reports it): each launch's own
// workgroups, and the contiguous range [first, first + count) of the n_red slab-reduce workgroups that runs behind
// them (RedShare). k_fold_finish takes a fixed quarter of n_red, rounded down, from the high end; k_fold_tail keeps
// the rest, so a stack with fewer reduce workgroups than launches is still covered. k_fold_gx takes none: a reduce
// workgroup lasts about twice that launch.
struct FoldTailPlan {
  long long S, splits;  // slab stride (floats); split-K splits
  int n_red, gx_dw;
  int own[3];           // own workgroups of k_fold_tail (split-K + the copy workgroup), k_fold_gx, k_fold_finish
  int first[3], count[3];
};
FoldTailPlan fold_tail_plan(const BcnfLayout& L, const BcnfLayout& F, int64_t batch);
// F = fold_layout(L, X, ldx); A.asc is set here (the scalars live in the slab's scratch).
int launch_fold_tail(const BcnfLayout& L, const BcnfLayout& F, const float* pk, float* slab, const float* x,
                     const float* wf, const float* bf, const float* ws, long long B, float* dparams, float* dwf,
                     float* dbf, FoldAdamArgs A, hipStream_t st);

#ifdef BCNF_PHASE_STAMPS
// Diagnostic build: each file's own 32 phase words (the forward writes slots 8-27, the backward 0-7).
int fwd_debug_phases(unsigned long long* out);
int bwd_debug_phases(unsigned long long* out);
#endif

}  // namespace bcnf_small
#pragma GCC visibility pop
