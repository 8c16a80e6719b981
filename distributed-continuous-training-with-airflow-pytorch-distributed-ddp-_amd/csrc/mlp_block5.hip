// One-rank launches (train mode, the one-step grad mode of the DDP step path, profiling) and the
// host-side checks of the 3x128 weather trainer; device code in mlp_block5_impl.h.  Compiled with
// the max-ILP machine scheduler (_build.py FILE_FLAGS): 3.90 -> 3.80 us/step at one rank
// (profiles/b5_sched_strategy_ab_r4.log).
#include "knobs.h"
#include "mlp_block5_impl.h"
#include "mlp_select.h"

namespace dct {

// in-kernel data-parallel launches of this kernel: 2 .. 8 ranks (one node), train mode; the profiling
// instantiations exist for 2 / 4 / 8
static bool b5_xg_world_ok(int w) { return w >= 2 && w <= 8; }

// per-rank batch 5..8, or every batch under DCT_MLP_BLOCK=8: two micro-batches per step (mlp_block5_b8.hip)
bool mlp_block5_two_micro(const MlpShape& sh, int B) { return B > blk5::B || sh.mlp_block == 8; }

bool mlp_block5_takes(const MlpShape& sh, const MlpLaunchKey& k) {
  const bool aligned = (sh.woff[1] % 4) == 0 && k.p_aligned && k.mv_aligned;
  const bool xg_ok = k.xg_world <= 1 ||
                     (k.mode == 0 && b5_xg_world_ok(k.xg_world) && k.xg_rank >= 0 && k.xg_rank < k.xg_world &&
                      k.xg_bufs && (!k.prof || k.xg_world == 2 || k.xg_world == 4 || k.xg_world == 8));
  const bool b8_ok = !mlp_block5_two_micro(sh, k.B) || !k.prof;  // no profiling instantiation of the b8 kernels
  return aligned && b8_ok && !k.accum && mlp_block5_shape_ok(sh.dims, sh.L, k.B) &&
         // train mode, or grad mode for ONE step (the DDP step path: grads + loss to grad_out, device cursor)
         ((k.mode == 0 && !k.cursor) || (k.mode == 1 && k.steps == 1 && k.grad_out)) &&
         (k.loss_kind == 0 || k.loss_kind == 1) && !k.pending && (!k.stage || k.mode == 1) && xg_ok;
}

bool mlp_block5_xg_shape_ok(const MlpShape& sh, const MlpLaunchKey& k) {
  return k.mode == 0 && !k.accum && mlp_block5_shape_ok(sh.dims, sh.L, k.B) && mlp_block5_xg_bytes(k.xg_world) > 0;
}

bool mlp_block5_shape_ok(const int* dims, int L, int B) {
  return L == 3 && dims[1] == blk5::H && dims[2] == blk5::H && dims[0] >= 1 && dims[0] <= blk5::DMAX &&
         dims[3] == blk5::C && B >= 1 && B <= blk5::BMAX;
}

size_t mlp_block5_xg_bytes(int world) {
  switch (world) {
    case 2: return (size_t)b5x::Lay<2>::BYTES;
    case 4: return (size_t)b5x::Lay<4>::BYTES;
    case 8: return (size_t)b5x::Lay<8>::BYTES;
    case 3: return (size_t)b5x::Lay<3>::BYTES;
    case 5: return (size_t)b5x::Lay<5>::BYTES;
    case 6: return (size_t)b5x::Lay<6>::BYTES;
    case 7: return (size_t)b5x::Lay<7>::BYTES;
    default: return 0;
  }
}

// one-rank batch <= 4 train launch: DCT_B5_SCHED=0 (knobs.h) selects the kernel without the step schedule
// (the reference of the bit-for-bit test and of same-binary A/Bs), anything else the default
template <bool WD, int LK, bool PROF = false>
static void b5_launch_sched(int sched, size_t bytes, hipStream_t st, const MlpShape& sh, const MlpArgs& a) {
  if (sched == 0) b5_launch<WD, LK, PROF>(bytes, st, sh, a);
  else b5_launch<WD, LK, PROF, true, 1, -1, 1, blk5::SCHED_DEFAULT>(bytes, st, sh, a);
}

hipError_t mlp_launch_block5(const MlpShape& sh, const MlpArgs& a, hipStream_t st) {
  const size_t bytes = (size_t)blk5::LDS_FLOATS * sizeof(float);
  const bool wd = a.wd != 0.f;
  const int sched = knobs().b5_sched;
  if (!mlp_block5_takes(sh, mlp_launch_key(a))) return hipErrorInvalidValue;
  if (mlp_block5_two_micro(sh, a.B)) {
    mlp_launch_block5_b8(bytes, st, sh, a);  // two micro-batches per step, every world size
  } else if (a.xg_world > 1) {
    mlp_launch_block5_xg(a.xg_world, bytes, st, sh, a);  // mlp_block5_xg.hip
  } else if (a.mode == 1) {  // grad mode: no Adam, no moments
    if (a.loss_kind == 0) b5_launch<false, 0, false, false>(bytes, st, sh, a);
    else b5_launch<false, 1, false, false>(bytes, st, sh, a);
  } else if (a.prof) {  // per-phase cycle stamps (tools/prof_block.py)
    if (a.loss_kind == 0) b5_launch_sched<true, 0, true>(sched, bytes, st, sh, a);
    else b5_launch_sched<true, 1, true>(sched, bytes, st, sh, a);
  } else if (a.loss_kind == 0) {
    if (wd) b5_launch_sched<true, 0>(sched, bytes, st, sh, a);
    else b5_launch_sched<false, 0>(sched, bytes, st, sh, a);
  } else {
    if (wd) b5_launch_sched<true, 1>(sched, bytes, st, sh, a);
    else b5_launch_sched<false, 1>(sched, bytes, st, sh, a);
  }
  return hipGetLastError();
}

}  // namespace dct
