// Host/device-shared descriptors of the fused MLP kernels (see mlp_fused_impl.h) and the C API of the small-MLP
// trainers; the general launchers (GEMM, Adam, step kernels, ...) are kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "lr_table.h"

namespace dct {

constexpr int MLP_MAXL = 4;
constexpr size_t MLP_LDS_BUDGET = 160 * 1024;  // bytes of LDS one workgroup of the LDS trainer / evaluator may lay out

// Everything a launch needs about one MLP architecture, computed once on the host
// (mlp_make_shape): LDS layout, per-layer work split of the forward / dX phases and
// the ownership of weight blocks for the dW + Adam phase.
struct MlpShape {
  int L;
  int dims[MLP_MAXL + 1];
  int rows4[MLP_MAXL];  // round4(out_l)
  int cols4[MLP_MAXL];  // round4(in_l)
  int ldw[MLP_MAXL];    // LDS row stride of W_l (floats)
  int w_lds[MLP_MAXL];  // LDS offsets (floats)
  int b_lds[MLP_MAXL];
  int a_lds[MLP_MAXL + 1];  // activations A_l [BMAX][lda_l] for l >= 1; A_L = logits
  int a0_lds[2];            // double-buffered input batch (next batch is written during a step)
  int lab_lds[2];           // double-buffered labels (int)
  int lda[MLP_MAXL + 1];
  int dz_lds[MLP_MAXL];  // dZ_l [BMAX][rows4_l]
  int woff[MLP_MAXL];    // torch flat offsets of W_l / b_l
  int boff[MLP_MAXL];
  // forward split: items = (rows4/4 output groups) << f_ksl k-splits, f_kc float4s per split
  int f_ksl[MLP_MAXL], f_kc[MLP_MAXL], f_items[MLP_MAXL];
  // dX split: items = (cols4/4 column groups) << d_osl o-splits, d_oc o-groups per split
  int d_osl[MLP_MAXL], d_oc[MLP_MAXL], d_items[MLP_MAXL];
  int br;                        // rows per owned weight block: 1 (small models) or 4
  int blk_start[MLP_MAXL + 1];   // prefix count of weight blocks per layer
  int blk_cols[MLP_MAXL];        // column blocks per row (cols4/4)
  int bias_start[MLP_MAXL + 1];  // prefix count of biases
  int nblk;
  int nbias;
  int P;
  int red_lds;  // reduction scratch
  int lds_floats;
  int bmax;
  int nt;        // threads per workgroup
  int maxq;      // weight blocks per thread
  int fuse_loss; // loss computed inside the last forward layer (classes <= 4)
  int supported;
  int mlp_block;  // plan-time copy of DCT_MLP_BLOCK (MlpPlan, bindings.cpp): the launch path reads this, never
                  // the process-wide knob struct
};

// MlpStepArgs: a launch's arguments up to the optimizer's own fields - what MlpArgs was before AdamW / SGD, field for
// field.  MlpArgs (below) appends those; the batch-tiled trainer's step kernel and its Adam fold, which read none of them,
// take this prefix as their kernel argument, so an Adam step runs on the kernel-argument segment it always had.
struct MlpStepArgs {
  float* p;  // flat params (torch state_dict order): W0,b0,W1,b1,...
  float* m;  // Adam exp_avg (same layout)
  float* v;  // Adam exp_avg_sq
  float* grad_out;  // GRAD mode: [P] grads + [P] = batch loss
  const float* X;
  int ldx;
  const int* Y;
  const int* idx;
  int n_items;  // indices available to this launch
  int B;        // batch size (<= BMAX)
  int steps;
  int t0;  // Adam steps already taken (bias correction uses t0+s+1)
  float lr, b1, b2, eps, wd;
  float dropout;
  uint32_t seed;
  uint32_t step_base;
  float* loss_out;  // [steps]
  int mode;         // 0 = train (Adam fused), 1 = grad only
  int loss_kind;    // 0 = CE, 1 = MSE vs one-hot
  // eval outputs
  float* eval_acc;   // [2]: sum loss, sum correct (atomic)
  float* logits_out; // optional [n_items][C]
  // optional device step counter (Adam steps taken so far): when set it overrides t0 and
  // step_base, and the kernel advances it by `steps` -> launches are graph-replayable.
  int* step_counter;
  // optional (GRAD mode): device batch cursor into idx. The kernel uses batch *cursor, first
  // stores the previous step's (all-reduced) loss grad_out[P] into loss_out[*cursor - 1], and
  // advances the cursor -> one captured step graph replays over a whole epoch.
  int* cursor;
  // diagnostic only: per-phase cycle sums (s_memtime deltas, thread 0) + [30]/[31] realtime
  // start/end (100 MHz) when non-null; never set in production launches.
  unsigned long long* prof;
  // optional (GRAD mode, single-wave kernel): "update-then-grad". If *pending != 0 the
  // kernel first applies Adam with the (all-reduced) gradients still in grad_out, then
  // computes the new gradients; p/m/v are written back and *pending is set to 1.
  int* pending;
  // optional (single-wave kernel): tagged staging buffer for the next launch's batch,
  // [0] = batch index of the staged data, [64..) = one dword per lane per prefetch slot.
  // A launch whose cursor equals the tag reads its batch from here (one round trip, issued
  // with the parameter loads) instead of the dependent idx -> x gather.
  uint32_t* stage;
  // optional (single-wave kernel, train mode): in-kernel data-parallel gradient averaging
  // across GPUs.  Every rank pushes its step gradients as 8-byte {tag, value} granules
  // straight into each peer's receive buffer (peer-mapped over xGMI via IPC) and sums the
  // peers' granules in rank order, so all ranks apply bit-identical Adam updates with no
  // host round trip, no RCCL launch and no kernel boundary per step.  See mlp_wave_impl.h.
  unsigned long long* xg_recv;              // own receive buffer, [2][W][KX][64] granules
  unsigned long long* const* xg_peers;      // device array [W]: every rank's receive buffer
  int xg_world;                             // 0/1 = off
  int xg_rank;
  unsigned int* xg_status;                  // [0]: 0 ok, else (global step + 1) of a timeout
  long long xg_timeout;                     // spin limit in s_memrealtime ticks (100 MHz)
  int xg_poll;                              // 0 full sweeps, 1 probe-then-sweep, 2 sequential; rows kernel:
                                            // 3 | stagger << 8 = two pipelined sweeps in flight
  // optional (row-parallel kernel): wave 0 adds the s_memrealtime ticks (100 MHz) its exchange
  // took over the launch - the allreduce_ms metric of the fused DDP step
  unsigned long long* xg_ticks;
  // kernel-specific A/B knob (mlp_block3.hip: wave priority split), 0 = the kernel's default
  int tune;
  // launch constants derived on the host (bindings.cpp make_train_args): mlp_block5 reads them from
  // the kernarg segment (scalar registers) instead of deriving them in the kernel, where the compiler
  // re-materialised the divisions / logarithms inside the step loop to save vector registers
  float k_drop_scale;  // 1 / (1 - dropout), or 1 without dropout
  float k_l2b1, k_l2b2;  // log2(b1), log2(b2) (Adam bias corrections as one exp2 each)
  float k_rc1, k_rc2;  // 1 / (1 - b1), 1 / (1 - b2) (scaled-moment Adam)
  float k_sqc2;        // sqrt(1 - b2)
  // batch-tiled trainer (mlp_tile.hip): slot workspace [ceil(B / 32)][Pp] partial gradients + loss (and, weighted,
  // the sum of w[y]) of a step, the fold kernel's arrival counter in its last four floats
  float* tile_ws;
  long long tile_ws_floats;
  // optional learning-rate table (lr_table.h; last, so every other field keeps its kernel-argument offset): train
  // launches take the rate of the step that runs after `taken` = t0 + s (or *step_counter + s) steps from it instead
  // of lr.  Grad-mode launches apply no Adam and ignore it, except the single-wave kernel's update-then-grad, whose
  // pending update is the step after *step_counter - 1.
  const float* lr_tab;
  // optional class-weighted / label-smoothed cross-entropy (batch-tiled trainer only; appended, so every other field
  // keeps its offset): class_w device [C] strictly positive weights (null: all 1), label_smooth in [0, 1).  With
  // either set the loss is sum_i num_i / W, W = sum_i w[y_i] over the live rows (torch's weighted mean); both off:
  // the plain CE / MSE with the 1 / bs normaliser.  mlp_select.h refuses such a launch on every other trainer.
  const float* class_w;
  float label_smooth;
  // optional gradient accumulation (batch-tiled trainer only; appended, so every other field keeps its offset): an
  // optimizer step runs over a window of `accum` micro-batches of B rows - batches [w * accum, (w + 1) * accum) of the
  // index list - and applies (1 / accum) * sum_kb grad(loss_kb), loss_kb the micro-batch's own mean (Lightning's
  // accumulate_grad_batches; always 1 / accum, also in a short last window).  `steps`, t0, step_base, the device
  // counters, the cursor and loss_out count optimizer steps; n_items counts rows; the reported loss is the window's last
  // live micro-batch's; micro-batch kb of step t draws its dropout masks with step word t * accum + kb.  0 and 1: off.
  // mlp_select.h refuses such a launch on every other trainer.
  int accum;
};

struct MlpArgs : MlpStepArgs {
  // optimizer of a train-mode launch (batch-tiled trainer only; appended, so every other field keeps its offset):
  // MLP_OPT_ADAM (0) is the launch as it always was; MLP_OPT_ADAMW decays p by lr_t * wd before the Adam update on the
  // undecayed gradient (torch.optim.AdamW); MLP_OPT_SGD is torch.optim.SGD with `momentum`, `dampening`, `nesterov` and
  // wd coupled into the gradient - it reads and writes p and m (the momentum buffer) only, v may be null, and so may m
  // when momentum == 0; at device step count 0 the buffer is set to the gradient, whatever m held.  lr_t is the lr
  // table's rate when one is bound.  Grad-mode launches apply no optimizer and ignore these.  mlp_select.h refuses a
  // non-Adam train-mode launch on every other trainer.
  int opt_kind;
  float momentum, dampening;
  int nesterov;
};

enum MlpOptimizer { MLP_OPT_ADAM = 0, MLP_OPT_ADAMW = 1, MLP_OPT_SGD = 2 };

constexpr int XG_MAXW = 8;  // ranks of the in-kernel exchange (one node)

// One launch of the batch-tiled inference kernel (mlp_infer.hip): forward only, rows 0 .. n - 1 of the index
// list (or of X itself), per-row outputs and - with labels - order-independent statistics.
struct MlpInferArgs {
  const float* p;  // flat params (torch state_dict order), 16-byte aligned
  const float* X;
  int ldx;          // row stride of X (floats)
  const int* idx;   // optional [n] rows of X; null: rows 0 .. n - 1
  const int* Y;     // optional labels, indexed like X's rows; null: no statistics
  long long n;
  const float* norm_mean;  // optional [D0], both or neither: the gather computes (x - mean) / std in fp32
  const float* norm_std;   // (a std of 0 is replaced by 1 on the host)
  int loss_kind;           // 0 = CE, 1 = MSE vs one-hot
  float* logits_out;       // optional [n][C]
  float* probs_out;        // optional [n][C], softmax with the row maximum subtracted
  int* pred_out;           // optional [n], argmax (lowest index on ties)
  // with Y: slot workspace of dct_mlp_infer_ws_bytes(dims, L, n) bytes and the statistics, 2 + C * C words of
  // 8 bytes: [0] the loss sum (fp64), [1] the correct count (int64), [2 + y * C + pred] the confusion matrix (int64)
  void* ws;
  long long ws_bytes;
  void* stats;
  // optional class-weighted / label-smoothed cross-entropy (loss_kind 0 only): class_w device [C] (null: all 1),
  // label_smooth in [0, 1).  With either set statistic word 0 is sum_i num_i, the numerator of the weighted mean;
  // its denominator W = sum_c w[c] * (row sum c of the confusion matrix) is the host's to compute.
  const float* class_w;
  float label_smooth;
};

// fills *sh for dims[0 .. L] and plans of up to bmax rows per step (mlp_block = -1: auto, until the plan stamps
// its knob copy); -1 when L is outside 2 .. MLP_MAXL, else 0 with sh->supported set
int mlp_make_shape(MlpShape* sh, const int* dims, int L, int bmax);
hipError_t mlp_launch_train_L2(const MlpShape& sh, const MlpArgs& a, hipStream_t st);
hipError_t mlp_launch_train_L3(const MlpShape& sh, const MlpArgs& a, hipStream_t st);
hipError_t mlp_launch_train_L4(const MlpShape& sh, const MlpArgs& a, hipStream_t st);
// Which trainer runs a launch is mlp_select.h's decision; the launchers below refuse what their
// kernel does not take (hipErrorInvalidValue) and choose only among their own instantiations.
// register-resident 8-wave two-barrier trainer for D0 <= 32 -> 128 -> 128 -> C <= 4, train and
// grad mode (mlp_block3.hip): every 3x128 shape mlp_block5 does not take
hipError_t mlp_launch_block3(const MlpShape& sh, const MlpArgs& a, hipStream_t st);
// lean two-barrier trainer for the exact weather shape D0<=8 -> 128 -> 128 -> 2, train mode, the
// one-step grad mode and the in-kernel data-parallel launches (mlp_block5.hip, the default there);
// DCT_MLP_BLOCK=3 selects mlp_block3, DCT_MLP_BLOCK=0 the generic LDS trainer
hipError_t mlp_launch_block5(const MlpShape& sh, const MlpArgs& a, hipStream_t st);
// its shape (D0 <= 8 -> 128 -> 128 -> 2, batch <= 8) and the exchange buffer of its in-kernel
// data-parallel launches at `world` = 2 .. 8 ranks (0: not supported)
bool mlp_block5_shape_ok(const int* dims, int L, int B);
size_t mlp_block5_xg_bytes(int world);
hipError_t mlp_launch_eval_L2(const MlpShape& sh, const MlpArgs& a, int grid, hipStream_t st);
hipError_t mlp_launch_eval_L3(const MlpShape& sh, const MlpArgs& a, int grid, hipStream_t st);
hipError_t mlp_launch_eval_L4(const MlpShape& sh, const MlpArgs& a, int grid, hipStream_t st);

}  // namespace dct

extern "C" {
int dct_mlp_select(const dct::MlpShape* sh, int* nt, int* maxblk);
int dct_mlp_lds_train(const dct::MlpShape& sh, const dct::MlpArgs* a, void* stream);  // the generic LDS trainer
int dct_mlp_eval(const dct::MlpShape& sh, const dct::MlpArgs* a, int grid, void* stream);
int dct_mlp_wave_supported(const int* dims, int L, int B);
// rows != 0: the row-parallel kernels (mlp_select.h MLP_WAVE_ROWS), else the single-wave kernel
int dct_mlp_wave_train(const int* dims, int L, const dct::MlpArgs* a, int rows, void* stream);
size_t dct_mlp_xg_slab_granules(const int* dims, int L);
// batch-tiled trainer for per-rank batch 17..1024 (mlp_tile.hip; DCT_MLP_BLOCK=tile forces it at smaller batches)
int dct_mlp_tile_supported(const int* dims, int L);
long long dct_mlp_tile_ws_floats(const int* dims, int L, int B);
// the same for windows of `accum` micro-batches (MlpArgs::accum): accum * ceil(B / 32) slots, at most
// dct_mlp_tile_max_slots() of them (0: over the cap, or not a tile shape / batch); accum <= 1 is the value above
long long dct_mlp_tile_ws_floats_accum(const int* dims, int L, int B, int accum);
int dct_mlp_tile_max_slots(void);
int dct_mlp_tile_train(const int* dims, int L, const dct::MlpArgs* a, void* stream);
// batch-tiled forward-only inference (mlp_infer.hip); grid <= 0: default.  It and dct_mlp_tile_train share one
// forward and one host check (mlp_tile_fwd.h): the shapes of dct_mlp_tile_supported, p on a 16-byte boundary
int dct_mlp_infer(const int* dims, int L, const dct::MlpInferArgs* a, int grid, void* stream);
long long dct_mlp_infer_ws_bytes(const int* dims, int L, long long n);
}
