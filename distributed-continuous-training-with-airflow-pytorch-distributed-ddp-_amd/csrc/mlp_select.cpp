// The small-MLP trainer selector (mlp_select.h): host code only.
#include "mlp_select.h"

namespace dct {

const char* mlp_trainer_name(MlpTrainer t) {
  switch (t) {
    case MLP_WAVE_SINGLE: return "wave_single";
    case MLP_WAVE_ROWS: return "wave_rows";
    case MLP_BLOCK5: return "block5";
    case MLP_BLOCK5_B8: return "block5_b8";
    case MLP_BLOCK3: return "block3";
    case MLP_LDS: return "lds";
    case MLP_TILE: return "tile";
    default: return "none";
  }
}

MlpLaunchKey mlp_launch_key(const MlpArgs& a) {
  MlpLaunchKey k{};
  k.B = a.B;
  k.mode = a.mode;
  k.steps = a.steps;
  k.loss_kind = a.loss_kind;
  k.xg_world = a.xg_world;
  k.xg_rank = a.xg_rank;
  k.cursor = a.cursor != nullptr;
  k.stage = a.stage != nullptr;
  k.pending = a.pending != nullptr;
  k.prof = a.prof != nullptr;
  k.grad_out = a.grad_out != nullptr;
  k.moments = a.m != nullptr && a.v != nullptr;
  k.xg_bufs = a.xg_recv != nullptr && a.xg_peers != nullptr && a.xg_status != nullptr;
  k.p_aligned = ((uintptr_t)a.p & 15) == 0;
  k.mv_aligned = (((uintptr_t)a.m | (uintptr_t)a.v) & 15) == 0;
  k.weighted = a.class_w != nullptr || a.label_smooth != 0.f;
  k.accum = a.accum > 1 ? a.accum : 0;
  k.other_opt = a.mode == 0 && a.opt_kind != MLP_OPT_ADAM;
  return k;
}

static MlpChoice none(const char* why, bool plan_level) { return MlpChoice{MLP_NONE, false, why, plan_level}; }
static MlpChoice take(MlpTrainer t, bool use_stage = false) { return MlpChoice{t, use_stage, nullptr, false}; }

MlpChoice mlp_select_trainer(const MlpShape& sh, bool use_wave, bool use_tile, const MlpLaunchKey& k) {
  const bool xg = k.xg_world > 1;
  // 1. the batch-tiled trainer: the plan of batch 17..1024, or DCT_MLP_BLOCK=tile
  if (use_tile) {
    if (xg || k.pending)
      return none("the batch-tiled trainer has no in-kernel all-reduce and no update-then-grad step", true);
    if (!mlp_tile_batch_ok(k.B)) return none("batch outside the batch-tiled trainer's range", false);
    if (k.accum && !mlp_tile_window_ok(k.B, k.accum))
      return none("accumulation window over the batch-tiled trainer's slot cap (accum * ceil(B / 32) <= 256)", false);
    return take(MLP_TILE);
  }
  if (k.accum)
    return none("gradient accumulation needs the batch-tiled trainer's plan (bmax 1024)", true);
  if (k.other_opt)
    return none("AdamW / SGD need the batch-tiled trainer's plan (bmax 1024)", true);
  if (k.weighted)
    return none("class weights / label smoothing need the batch-tiled trainer's plan (bmax 1024)", true);
  if (k.pending && !use_wave) return none("update-then-grad needs the single-wave kernel", true);
  // 2. the wave kernels, where the plan is a wave plan and they take this batch
  if (use_wave && dct_mlp_wave_supported(sh.dims, sh.L, k.B)) {
    if (xg && !mlp_wave_xg_takes(sh.L, k))
      return none("the wave kernels' in-kernel all-reduce: 2-layer nets, train mode, 2 .. 8 ranks", false);
    return take(mlp_wave_rows_takes(sh.L, k) ? MLP_WAVE_ROWS : MLP_WAVE_SINGLE, k.stage);
  }
  // 3. the LDS trainer and its 3x128 block kernels
  if (!sh.supported) return none("MLP too large for the fused kernel", false);
  if (k.B < 1 || k.B > sh.bmax) return none("batch outside the plan's 1 .. bmax", false);
  MlpLaunchKey q = k;
  if (q.stage && !mlp_block5_takes(sh, q)) q.stage = false;  // only mlp_block5's grad mode stages batches here
  const MlpTrainer b5 = mlp_block5_two_micro(sh, q.B) ? MLP_BLOCK5_B8 : MLP_BLOCK5;
  if (xg) {  // in-kernel data parallelism: only the 3x128 block kernel has it here, whatever DCT_MLP_BLOCK says
    if (!mlp_block5_xg_shape_ok(sh, q))
      return none("in-kernel all-reduce needs the single-wave kernel or the 3x128 block kernel "
                  "(train mode, 2 .. 8 ranks)", true);
    if (!mlp_block5_takes(sh, q)) return none("mlp_block5 does not take this exchange launch", false);
    return take(b5, q.stage);
  }
  const int blk = sh.mlp_block;  // plan-time DCT_MLP_BLOCK: -1 auto, 8 mlp_block5_b8, 3 mlp_block3, 0 the LDS trainer
  if ((blk < 0 || blk == 8) && mlp_block5_takes(sh, q)) return take(b5, q.stage);
  if (blk != 0 && mlp_block3_takes(sh, q)) return take(MLP_BLOCK3);
  if (sh.L < 2 || sh.L > MLP_MAXL) return none("the LDS trainer is instantiated for 2 .. 4 layers", false);
  return take(MLP_LDS);
}

}  // namespace dct

extern "C" int dct_mlp_supported(const int* dims, int L, int batch) {
  if (L < 1 || batch < 1) return 0;
  if (batch > 16) return dct_mlp_tile_ws_floats(dims, L, batch) > 0 ? 1 : 0;  // the batch-tiled trainer
  dct::MlpShape sh;
  if (dct::mlp_make_shape(&sh, dims, L, batch <= 4 ? 4 : 16) != 0) return 0;
  return sh.supported;
}
