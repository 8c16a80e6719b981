// Which small-MLP trainer runs a training launch.  One pure host function of (shape, plan flags,
// launch key) holds the order in which the trainers are asked; the launch path (bindings.cpp
// launch_train) and the Python query (MlpPlan.trainer) both go through it.  Each trainer's own limits
// are predicates on the key, defined next to its kernel.  Nothing here allocates, builds a string or
// reads the environment: the DCT_* knobs reach it as the plan's copies (knobs.h).
#pragma once
#include "mlp_fused.h"

namespace dct {

enum MlpTrainer {
  MLP_NONE,         // no trainer runs this launch (MlpChoice::why_none)
  MLP_WAVE_SINGLE,  // mlp_wave_single*.hip
  MLP_WAVE_ROWS,    // mlp_wave_rows_x*.hip
  MLP_BLOCK5,       // mlp_block5.hip, mlp_block5_xg*.hip
  MLP_BLOCK5_B8,    // mlp_block5_b8.hip
  MLP_BLOCK3,       // mlp_block3.hip
  MLP_LDS,          // mlp_fused_l*.hip
  MLP_TILE,         // mlp_tile.hip
};
const char* mlp_trainer_name(MlpTrainer t);

// What the choice depends on in a launch's arguments: its scalars, and which pointers are bound.
struct MlpLaunchKey {
  int B, mode, steps, loss_kind, xg_world, xg_rank;
  bool cursor, stage, pending, prof, grad_out;
  bool moments;     // m and v bound
  bool xg_bufs;     // xg_recv, xg_peers and xg_status bound
  bool p_aligned;   // p on a 16-byte boundary
  bool mv_aligned;  // m and v on 16-byte boundaries (unbound counts as aligned)
  bool weighted;    // class_w bound or label_smooth != 0: only the batch-tiled trainer computes that loss
  int accum;        // MlpArgs::accum when > 1 (gradient accumulation on: only the batch-tiled trainer runs windows), else 0
  bool other_opt;   // a train-mode launch whose MlpArgs::opt_kind is not Adam (AdamW, SGD): only the batch-tiled
                    // trainer's fold applies those; grad-mode launches apply no optimizer and never set it
};
MlpLaunchKey mlp_launch_key(const MlpArgs& a);  // the only place pointers become bools

struct MlpChoice {
  MlpTrainer trainer;
  bool use_stage;        // the launch passes MlpArgs::stage on (no other trainer stages batches)
  const char* why_none;  // static text, MLP_NONE only
  bool plan_level;       // MLP_NONE only: no trainer of this plan runs such a launch at all (an invalid request),
                         // as opposed to a chosen trainer's limit on the arguments (a failed launch)
};
MlpChoice mlp_select_trainer(const MlpShape& sh, bool use_wave, bool use_tile, const MlpLaunchKey& k);

// ---- the trainers' own limits
// mlp_wave.hip: the row-parallel kernels against the single-wave kernel, and the wave kernels' exchange launches
bool mlp_wave_rows_takes(int L, const MlpLaunchKey& k);
bool mlp_wave_xg_takes(int L, const MlpLaunchKey& k);
// mlp_block5.hip: D0 <= 8 -> 128 -> 128 -> 2 at batch <= 8; train mode, the one-step grad mode and the in-kernel
// data-parallel launches at 2 .. 8 ranks (xg_shape_ok: this plan has such launches at all)
bool mlp_block5_takes(const MlpShape& sh, const MlpLaunchKey& k);
bool mlp_block5_xg_shape_ok(const MlpShape& sh, const MlpLaunchKey& k);
bool mlp_block5_two_micro(const MlpShape& sh, int B);  // mlp_block5_b8's two micro-batches per step
// mlp_block3.hip: D0 <= 32 -> 128 -> 128 -> C <= 4 at batch <= 4, train and grad mode
bool mlp_block3_takes(const MlpShape& sh, const MlpLaunchKey& k);
// mlp_tile.hip
bool mlp_tile_batch_ok(int B);
bool mlp_tile_window_ok(int B, int accum);  // accum micro-batches of B rows fit the slot cap (accum <= 1: always)
bool mlp_tile_optimizer_ok(const MlpArgs& a);  // a train-mode launch's optimizer fields are ones its fold applies

}  // namespace dct

extern "C" {
// some trainer takes this architecture at this per-rank batch (FusedMLPKernel.supported)
int dct_mlp_supported(const int* dims, int L, int batch);
}
