// mlp_tile: batch-tiled fused fp32 trainer for the weather MLPs at per-rank batch 17..1024.
//
// The LDS / block / wave trainers keep a whole step in ONE workgroup, which stops paying at
// batch > 16.  Here one optimizer step is a grid of T = ceil(B / R) workgroups, R = 32 rows per
// workgroup (two M = 16 row blocks per MFMA column block, so every weight fragment a wave loads
// feeds two MFMAs; 4 waves per workgroup), followed by a small fold launch:
//
//   step kernel (grid T): gather rows X[idx[...]] + labels -> layer 0 on the VALU (D0 <= 32) ->
//     hidden x hidden forward on v_mfma_f32_16x16x4_f32 (exact fp32) -> head (C <= 4) + CE / MSE
//     and dlogits / bs on the VALU -> dX and dW of the hidden x hidden layer on the MFMA, the
//     narrow layers on the VALU -> the tile's partial gradients [P] and partial loss sum go to its
//     own slot of the workspace [T][Pp] with plain vector stores.  Rows >= bs contribute zeros, a
//     tile without a live row writes a zero slot.  With class weights / label smoothing (MlpArgs::class_w,
//     label_smooth; CE only) the row loss is row_loss4_weighted's numerator and un-normalised dlogits, and the
//     tile also writes the sum of w[y] over its live rows to slot word P + 1.
//   fold kernel (grid ceil((P + 1) / 256)): sums the T slots in ascending tile index (bit-identical
//     whatever order the tiles finished in), then Adam (adam_elem, train mode) or grad_out (grad
//     mode), the batch loss, and the device step counter / batch cursor.  Weighted: it first sums the tiles' w[y]
//     words in the same order into W and divides the folded gradient and loss by it (torch's weighted mean).
//     The kernel boundary is what makes the slots visible across XCDs; no workgroup ever waits on another one.  The
//     counters are advanced by the fold's last-arriving workgroup (an arrival counter that it
//     leaves at zero, so a captured launch pair replays).
//
// Gradient accumulation (MlpArgs::accum = K > 1, Lightning's accumulate_grad_batches): an optimizer step is a window of
// K micro-batches of B rows, run as ONE grid (T, K) - workgroup (tile, kb) works on batch cur * K + kb with its own bs,
// draws dropout with step word gstep * K + kb and writes slot kb * T + tile - and one fold over the K * T slots in
// ascending slot index: (1 / K) * sum_kb (micro-batch kb's mean gradient), the loss of the window's last live
// micro-batch.  K * T <= MAX_SLOTS; the counters, t0, step_base, the cursor and loss_out count optimizer steps.
//
// Weights are read straight from the flat parameter buffer (L2 resident, <= 85 KB, on a 16-byte boundary: W1
// is read as float4); activations and dZ of the tile live in LDS with the two narrow layers' weights (91.5 KB
// for the 3-layer nets, 57.7 KB for the 2-layer ones; with LayerNorm one xhat image [32][132] per hidden layer and
// 32 rstd per layer more: 125.6 KB and 74.9 KB, inside gfx950's 160 KB at one workgroup per CU, which MAX_SLOTS
// already assumes).  No LDS-DMA loads.
// The forward pieces (W1 fragment load, weight staging, layers 0 and 1, head logits), the shape rule (make_plan)
// and the launch check are mlp_tile_fwd.h's, shared with the inference kernel (mlp_infer.hip); the gather, the
// loss, the whole backward, the slots and the fold are here.
// Dropout key: mix_hash(seed + (b >> 6) * 0x9E3779B9, gstep, (LI * 64 + (b & 63)) * 65536 + o),
// b = row within the batch: rows < 64 draw the LDS kernel's mask (ops/fused_mlp.py
// dropout_keep_mask is the host mirror).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mlp_fused_impl.h"
#include "mlp_select.h"
#include "mlp_tile_fwd.h"

namespace dct {
namespace tile {

constexpr int BMAX = 1024;
// slots of one optimizer step: accum * ceil(B / R) <= MAX_SLOTS (32 at accum = 1).  256 is one workgroup per CU in a
// single round (the 3-layer carve's 91.5 KB of LDS leaves room for one per CU); it also bounds the fold's serial sum
// and the workspace (256 slots of a 3x128 net: about 18 MB)
constexpr int MAX_SLOTS = 256;
constexpr int FOLD_NT = 256;

// LDS carve (floats)
struct Lds {
  int x0, w0, wl, a1, dz1, a2, dz2, dzl, lossr, lab, xh1, xh2, rs, total;
};
__host__ __device__ inline Lds lds_layout(int L, bool norm = false) {
  Lds o;
  int off = 0;
  o.x0 = off; off += R * LDX;
  o.w0 = off; off += 128 * LDX;
  o.wl = off; off += 4 * 128 + 4;  // head weights [C][K] + bias
  o.a1 = off; off += R * LDH;
  o.dz1 = off; off += R * LDH;
  o.a2 = off; if (L == 3) off += R * LDH;
  o.dz2 = off; if (L == 3) off += R * LDH;
  o.dzl = off; off += R * 4;
  o.lossr = off; off += R;
  o.lab = off; off += R;
  // LayerNorm only, behind everything the plain carve has: xhat of the two hidden layers, rstd [2][32]
  o.xh1 = off; if (norm) off += R * LDH;
  o.xh2 = off; if (norm && L == 3) off += R * LDH;
  o.rs = off; if (norm) off += 2 * R;
  o.total = off;
  return o;
}

__device__ __forceinline__ float drop_apply(float z, uint32_t seed, uint32_t gstep, int LI, int b, int o, float p,
                                            float scale) {
  const uint32_t h = mix_hash(seed + (uint32_t)(b >> 6) * 0x9E3779B9u, gstep,
                              (uint32_t)((LI * 64 + (b & 63)) * 65536 + o));
  return (u01(h) < p) ? 0.f : z * scale;
}

// WL: the class-weighted / label-smoothed loss (class_w bound or label_smooth != 0), chosen on the host from the
// launch arguments - the plain instantiation is the kernel as it was
// ACC: gradient accumulation (MlpArgs::accum > 1), chosen on the host likewise: the grid's second dimension is the
// micro-batch kb of the window, workgroup (tile, kb) works on batch cur * accum + kb of the index list with that batch's
// own bs and dropout step word gstep * accum + kb, and writes slot kb * T + tile.  Without it the kernel is as it was.
// ACT: the hidden layers' activation (MlpAct, chosen on the host from MlpActArgs::act_kind): MLP_ACT_RELU is the kernel
// as it was.  The ReLU backward rebuilds its mask from the stored activation; a smooth activation's derivative needs the
// pre-activation z, which the tile does not keep.  Instead the forward epilogues of layers 0 and 1 - which hold z -
// store A = keep * scale * act(z) where they store it today and the local derivative D = keep * scale * act'(z) into
// the same (row, unit) of that layer's dZ image, idle until the backward; the two backward sites (head backward, dZ1
// MFMA epilogue) multiply their incoming gradient by the D they find in place and overwrite it, dZ = g * D: each
// element is written there by exactly the thread that reads it, behind the barriers that already separate forward
// and backward.  No LDS image, no recomputation, no barrier more; dW1, dW0, the bias sums and the slots are untouched.
// Rows >= bs: their D is act'(b0 ..), finite and not zero - it is their g that is an exact zero (dlogits of a dead
// row are 0, and so is every product and MFMA sum of them), so dZ = 0 * D = 0.  Units beyond H1 / H2 are never
// written and never read: the widths are multiples of 16 and every loop and column block stops at them.
// NORM: nn.LayerNorm (eps 1e-5, affine) between every hidden Linear and its activation (MlpNormArgs::norm_kind, chosen
// on the host likewise; false is the kernel as it was).  Forward, per hidden layer: the layer's epilogue stores the
// pre-norm z + b, and behind a barrier norm_rows (mlp_tile_fwd.h, 8 lanes per row) normalises the image in place -
// A = keep * scale * act(u), u = gamma * xhat + beta - and leaves xhat in the layer's own image XH, rstd in 32 floats
// and D = keep * scale * act'(u) in the idle dZ image, for ReLU too (D = keep * scale * [u > 0]), so both backward
// sites leave du = g * D in place as the smooth activations do.  Backward, behind each site's barrier (norm_backward):
// the column sums dbeta = sum_r du, dgamma = sum_r du * xhat in ascending row order into the slot's tail words, a
// barrier, then a row pass of the same 8 lanes: gw = du * gamma, s1 = sum gw / H, s2 = sum gw * xhat / H through the
// xor tree, dz = rstd * (gw - s1 - xhat * s2) in place - and the dW / db code that follows reads dz as it always did.
// Rows >= bs: the pre-norm is the bias vector, whose variance may be 0 - rstd = rsqrt(eps) and xhat = 0 are finite,
// and g is an exact zero, so du, gw, s1, s2 and dz are exact zeros.  Every sum has a fixed order.
// NORM == MLP_NORM_RMS: nn.RMSNorm (eps 1e-5) in the same places, in LayerNorm's carve: rms_rows (one pass for sum z^2,
// u = gamma * xhat, xhat = z * rstd) keeps xhat and rstd where norm_rows keeps them, and rms_backward writes the
// dgamma column sums alone and dz = rstd * (gw - xhat * s2).  gamma_2 sits H1 words behind gamma_1 (norm_off).
// RES: the skip connection h2 = h1 + Dropout(act(Norm(Linear(h1)))) of a net with two hidden layers of equal width
// (MlpResArgs::residual, chosen on the host likewise; L == 3 only).  Forward: layer 1's epilogue - layer1_block's, or
// the norm's row pass - adds A1[r][o] to what it stores into A2; A1 is only read there, also while other waves still
// read it as their MFMA operand, and A2 is an image of its own.  Backward: A2 is a sum, so its sign is no ReLU mask -
// every RES instantiation takes the D-image path of the smooth activations in both layers, ReLU with D = keep *
// scale * [. > 0].  The skip hands the head's gradient G[r][k] = sum_c dZL[r][c] * Wl[c][k] to A1 beside the branch's:
// the dZ1 MFMA epilogue recomputes G from dZL and Wl, both still in LDS (C <= 4 FMAs per element, no image and no
// barrier more), dZ1 = (dZ2 W1 + G) * D1.  Rows >= bs: dZL = 0, so G is an exact zero.  dW1 = dZ2^T A1 and the head's
// dW = dZL^T A2 are as they were.
template <int L, bool WL, bool ACC, int ACT = MLP_ACT_RELU, int NORM = MLP_NORM_OFF, bool RES = false>
__global__ __launch_bounds__(NT) void mlp_tile_step_kernel(Plan tp, MlpStepArgs a) {
  static_assert(!RES || L == 3, "the skip connection spans the second of two hidden layers");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds lo = lds_layout(L, NORM != MLP_NORM_OFF);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 15, q = lane >> 4;
  const int D0 = tp.D0, H1 = tp.H1, H2 = tp.H2, C = tp.C, K = tp.K;
  const int B = a.B;

  int cur = 0;
  if (a.cursor) cur = __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t gstep = a.step_base;
  if (a.step_counter)
    gstep = (uint32_t)__hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // (unsigned, as blockIdx.x: with a signed index the plain kernel's slot address compiled 12 bytes shorter, and the
  // shifted code measured 0.15 .. 0.3 % slower at batch 256 - profiles/accum_cost.log)
  unsigned int slot_i = blockIdx.x;
  if (ACC) {  // from here on `cur` is the micro-batch's index in the list and `gstep` its dropout step word
    const int kb = blockIdx.y;
    cur = cur * a.accum + kb;
    gstep = gstep * (uint32_t)a.accum + (uint32_t)kb;
    slot_i = blockIdx.y * gridDim.x + blockIdx.x;
  }
  const int bs = ACC ? (int)max(0ll, min((long long)B, (long long)a.n_items - (long long)cur * B))
                     : max(0, min(B, a.n_items - cur * B));
  const int row0 = blockIdx.x * R;
  const bool dropping = a.dropout > 0.f;
  const float dscale = dropping ? a.k_drop_scale : 1.0f;
  // class-weighted / label-smoothed CE: the weights in (scalar) registers
  constexpr bool wloss = WL;
  float cw[4] = {1.f, 1.f, 1.f, 1.f};
  if (WL && a.class_w) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) cw[c] = a.class_w[c];
  }

  float* X0 = lds + lo.x0;
  float* W0s = lds + lo.w0;
  float* Wl = lds + lo.wl;
  float* A1 = lds + lo.a1;
  float* dZ1 = lds + lo.dz1;
  float* A2 = lds + lo.a2;
  float* dZ2 = lds + lo.dz2;
  float* dZL = lds + lo.dzl;
  float* lossr = lds + lo.lossr;
  int* lab = reinterpret_cast<int*>(lds + lo.lab);
  float* slot = a.tile_ws + (size_t)slot_i * tp.Pp;

  // the epilogue of the hidden layers: dropout keyed by the row within the batch
  const auto drop = [&](int LI, int r, int o, float z) {
    return dropping ? drop_apply(z, a.seed, gstep, LI, row0 + r, o, a.dropout, dscale) : z;
  };
  // the same of a smooth activation, on the pre-activation: one draw of the same key scales act(z) and act'(z)
  const auto act_drop = [&](int LI, int r, int o, float z) {
    float d = 0.f, av = z;
    if constexpr (ACT != MLP_ACT_RELU) av = act_grad<ACT>(z, d);
    const float ks = dropping ? drop_apply(1.0f, a.seed, gstep, LI, row0 + r, o, a.dropout, dscale) : 1.0f;
    (LI == 0 ? dZ1 : dZ2)[r * LDH + o] = d * ks;
    return av * ks;
  };
  // norm_rows' epilogue: the same on the normalised u, with ReLU's [u > 0] as its derivative, and xhat kept
  float* XH1 = lds + lo.xh1;
  float* XH2 = lds + lo.xh2;
  float* RS = lds + lo.rs;
  const auto norm_drop = [&](int LI, int r, int o, float u, float xhat) {
    float d = u > 0.f ? 1.0f : 0.f, av = fmaxf(u, 0.f);
    if constexpr (ACT != MLP_ACT_RELU) av = act_grad<ACT>(u, d);
    const float ks = dropping ? drop_apply(1.0f, a.seed, gstep, LI, row0 + r, o, a.dropout, dscale) : 1.0f;
    (LI == 0 ? dZ1 : dZ2)[r * LDH + o] = d * ks;
    (LI == 0 ? XH1 : XH2)[r * LDH + o] = xhat;
    if constexpr (RES) {
      if (LI == 1) return A1[r * LDH + o] + av * ks;  // the skip
    }
    return av * ks;
  };
  // the plain layers' epilogue behind a skip connection (RES without a norm), on the pre-activation: act_drop with
  // ReLU's D = keep * scale * [z > 0] too, and layer 1 adds its input
  const auto res_drop = [&](int LI, int r, int o, float z) {
    float d = z > 0.f ? 1.0f : 0.f, av = fmaxf(z, 0.f);
    if constexpr (ACT != MLP_ACT_RELU) av = act_grad<ACT>(z, d);
    const float ks = dropping ? drop_apply(1.0f, a.seed, gstep, LI, row0 + r, o, a.dropout, dscale) : 1.0f;
    (LI == 0 ? dZ1 : dZ2)[r * LDH + o] = d * ks;
    return LI == 1 ? A1[r * LDH + o] + av * ks : av * ks;
  };
  // LayerNorm backward of hidden layer LI with H units, whose du = g * D stands in dZ behind a barrier: the slot's
  // dgamma / dbeta words (threads 0 .. H - 1 sum dbeta, H .. 2 H - 1 dgamma, rows ascending), then dz in place
  const auto norm_backward = [&](int LI, int H, float* dZ, const float* XH) {
    const int go = norm_off(tp, LI);
    if (tid < 2 * H) {
      const bool isg = tid >= H;
      const int o = isg ? tid - H : tid;
      float s = 0.f;
      for (int r = 0; r < R; ++r) {
        const float du = dZ[r * LDH + o];
        s = isg ? fmaf(du, XH[r * LDH + o], s) : s + du;
      }
      slot[go + (isg ? 0 : H) + o] = s;
    }
    __syncthreads();
    const int r = tid >> 3, part = tid & 7;
    const float* gamma = a.p + go;
    float* drow = dZ + r * LDH;
    const float* xrow = XH + r * LDH;
    float s1 = 0.f, s2 = 0.f;
    for (int k = part; k < H; k += 8) {
      const float gw = drow[k] * gamma[k];
      s1 += gw;
      s2 = fmaf(gw, xrow[k], s2);
    }
    s1 += __shfl_xor(s1, 1);
    s2 += __shfl_xor(s2, 1);
    s1 += __shfl_xor(s1, 2);
    s2 += __shfl_xor(s2, 2);
    s1 += __shfl_xor(s1, 4);
    s2 += __shfl_xor(s2, 4);
    const float invH = 1.0f / (float)H;
    s1 *= invH;
    s2 *= invH;
    const float rstd = RS[LI * R + r];
    for (int k = part; k < H; k += 8) drow[k] = rstd * (drow[k] * gamma[k] - s1 - xrow[k] * s2);
    __syncthreads();
  };
  // (res_drop above and rms_backward here repeat norm_drop / norm_backward rather than parametrise them: LayerNorm's
  // own lambdas stay as they were written)
  // RMSNorm backward, likewise: the slot's dgamma words alone (threads 0 .. H - 1, rows ascending), then
  // dz = rstd * (gw - xhat * s2), s2 = sum(gw * xhat) / H, in place
  const auto rms_backward = [&](int LI, int H, float* dZ, const float* XH) {
    const int go = norm_off(tp, LI, MLP_NORM_RMS);
    if (tid < H) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = fmaf(dZ[r * LDH + tid], XH[r * LDH + tid], s);
      slot[go + tid] = s;
    }
    __syncthreads();
    const int r = tid >> 3, part = tid & 7;
    const float* gamma = a.p + go;
    float* drow = dZ + r * LDH;
    const float* xrow = XH + r * LDH;
    float s2 = 0.f;
    for (int k = part; k < H; k += 8) s2 = fmaf(drow[k] * gamma[k], xrow[k], s2);
    s2 += __shfl_xor(s2, 1);
    s2 += __shfl_xor(s2, 2);
    s2 += __shfl_xor(s2, 4);
    s2 *= 1.0f / (float)H;
    const float rstd = RS[LI * R + r];
    for (int k = part; k < H; k += 8) drow[k] = rstd * (drow[k] * gamma[k] - xrow[k] * s2);
    __syncthreads();
  };

  // ---- this wave's W1 fragments of the forward MFMA: issued first, so their L2 round trips overlap the
  // gather and layer 0 instead of chaining inside the k loop
  float4 wf[2][8];
  if (L == 3) load_w1_frags(wf, a.p + tp.woff[1], H1, H2, wave, j, q);

  // ---- gather the tile's rows and labels; stage W0 and the head
  for (int e = tid; e < R * D0; e += NT) {
    const int r = e / D0, k = e - r * D0;
    const int gb = row0 + r;
    float x = 0.f;
    if (gb < bs) x = a.X[(size_t)a.idx[(size_t)cur * B + gb] * a.ldx + k];
    X0[r * LDX + k] = x;
  }
  if (tid < R) {
    const int gb = row0 + tid;
    lab[tid] = (gb < bs) ? a.Y[a.idx[(size_t)cur * B + gb]] : 0;
  }
  stage_weights(W0s, Wl, a.p, tp, L, tid);
  __syncthreads();

  // ---- layer 0: A1 = dropout(relu(X0 W0^T + b0))
  if constexpr (NORM == MLP_NORM_RMS) {  // the same through rms_rows
    layer0<1>(A1, W0s, X0, D0, H1, tid, NoEpilogue{});
    __syncthreads();
    rms_rows(A1, RS, a.p + norm_off(tp, 0, NORM), H1, 0, tid, norm_drop);
  } else if constexpr (NORM != MLP_NORM_OFF) {  // A1 = z + b0, then normalised in place: A1 = keep scale act(u), dZ1 = D, XH1 = xhat
    layer0<1>(A1, W0s, X0, D0, H1, tid, NoEpilogue{});
    __syncthreads();
    const int go = norm_off(tp, 0);
    norm_rows(A1, RS, a.p + go, a.p + go + H1, H1, 0, tid, norm_drop);
  } else if constexpr (RES) layer0<1>(A1, W0s, X0, D0, H1, tid, res_drop);  // dZ1 = D for ReLU too
  else if constexpr (ACT == MLP_ACT_RELU) layer0(A1, W0s, X0, D0, H1, tid, drop);
  else layer0<ACT>(A1, W0s, X0, D0, H1, tid, act_drop);  // A1 = keep scale act(z), dZ1 = D
  __syncthreads();

  // ---- layer 1: A2 = dropout(relu(A1 W1^T + b1)); a wave owns column blocks wave, wave + 4
  if (L == 3) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cb = wave + 4 * c;
      if (cb * 16 >= H2) break;
      if constexpr (NORM != MLP_NORM_OFF) layer1_block<1>(A2, A1, wf[c], cb, a.p[tp.boff[1] + cb * 16 + j], H1, j, q, NoEpilogue{});
      else if constexpr (RES) layer1_block<1>(A2, A1, wf[c], cb, a.p[tp.boff[1] + cb * 16 + j], H1, j, q, res_drop);  // A2 = A1 + .
      else if constexpr (ACT == MLP_ACT_RELU) layer1_block(A2, A1, wf[c], cb, a.p[tp.boff[1] + cb * 16 + j], H1, j, q, drop);
      else layer1_block<ACT>(A2, A1, wf[c], cb, a.p[tp.boff[1] + cb * 16 + j], H1, j, q, act_drop);  // dZ2 = D
    }
    __syncthreads();
    if constexpr (NORM == MLP_NORM_RMS) {
      rms_rows(A2, RS + R, a.p + norm_off(tp, 1, NORM), H2, 1, tid, norm_drop);
      __syncthreads();
    } else if constexpr (NORM != MLP_NORM_OFF) {  // A2 = z + b1 normalised in place, dZ2 = D, XH2 = xhat
      const int go = norm_off(tp, 1);
      norm_rows(A2, RS + R, a.p + go, a.p + go + H2, H2, 1, tid, norm_drop);
      __syncthreads();
    }
  }

  // ---- W1 fragments of the dZ1 MFMA (k = the H2 outputs), in flight across the head phases
  float wb[2][8][4];
  if (L == 3) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cb = wave + 4 * c;
      const float* wcol = a.p + tp.woff[1] + (size_t)(4 * q) * H1 + cb * 16 + j;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          wb[c][i][t] = (cb * 16 < H1 && i * 16 < H2) ? wcol[(size_t)(i * 16 + t) * H1] : 0.f;
    }
  }

  // ---- head (VALU, 8 lanes per row) + loss + dlogits / bs
  const float* Ah = (L == 3) ? A2 : A1;
  float* dZh = (L == 3) ? dZ2 : dZ1;
  {
    const int r = tid >> 3;
    float z[4], dz[4] = {0.f, 0.f, 0.f, 0.f};
    head_logits(z, Ah, Wl, C, K, tid);
    if ((tid & 7) == 0) {
      const bool live = (row0 + r) < bs;
      if (wloss) {
        // un-normalised: the fold divides the folded gradient and loss by W = sum of w[y] over the batch's live rows
        float wy;
        const float num = row_loss4_weighted(z, C, lab[r], cw, a.label_smooth, dz, &wy);
#pragma unroll
        for (int c = 0; c < 4; ++c) dZL[r * 4 + c] = (c < C && live) ? dz[c] : 0.f;
        lossr[r] = live ? num : 0.f;
        lab[r] = __float_as_int(live ? wy : 0.f);  // w[y] where the label was (read above, by this thread only)
      } else {
        const float inv = 1.0f / (float)(bs > 0 ? bs : 1);
        const LossAcc rl = row_loss4(z, C, lab[r], a.loss_kind, live ? inv : 0.f, dz);
#pragma unroll
        for (int c = 0; c < 4; ++c) dZL[r * 4 + c] = (c < C) ? dz[c] : 0.f;
        lossr[r] = live ? rl.loss : 0.f;
      }
    }
  }
  __syncthreads();

  // ---- head backward (VALU): dZ of the last hidden layer, dW / db of the head
  for (int e = tid; e < R * K; e += NT) {
    const int r = e / K, k = e - r * K;
    float g = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) g = fmaf(dZL[r * 4 + c], Wl[c * K + k], g);
    if constexpr (ACT == MLP_ACT_RELU && NORM == MLP_NORM_OFF && !RES) {
      const float av = Ah[r * LDH + k];
      dZh[r * LDH + k] = (av > 0.f) ? g * dscale : 0.f;
    } else {
      dZh[r * LDH + k] = g * dZh[r * LDH + k];  // the forward's D, in place
    }
  }
  for (int e = tid; e < C * K; e += NT) {
    const int c = e / K, k = e - c * K;
    float g = 0.f;
    for (int r = 0; r < R; ++r) g = fmaf(dZL[r * 4 + c], Ah[r * LDH + k], g);
    slot[tp.woff[L - 1] + e] = g;
  }
  if (tid < C) {
    float g = 0.f;
    for (int r = 0; r < R; ++r) g += dZL[r * 4 + tid];
    slot[tp.boff[L - 1] + tid] = g;
  }
  if (tid == NT - 1) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += lossr[r];
    slot[tp.P] = s;
    if (wloss) {  // the tile's share of W, rows in ascending order
      float sw = 0.f;
      for (int r = 0; r < R; ++r) sw += __int_as_float(lab[r]);
      slot[tp.P + 1] = sw;
    }
  }
  __syncthreads();
  // ---- LayerNorm backward of the last hidden layer: du -> dgamma, dbeta, dz
  if constexpr (NORM == MLP_NORM_RMS) rms_backward(L - 2, K, dZh, (L == 3) ? XH2 : XH1);
  else if constexpr (NORM != MLP_NORM_OFF) norm_backward(L - 2, K, dZh, (L == 3) ? XH2 : XH1);

  if (L == 3) {
    // ---- dZ1 = mask(A1) * (dZ2 W1) on the MFMA: k runs over the H2 outputs
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cb = wave + 4 * c;
      if (cb * 16 >= H1) break;
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const float* dr0 = dZ2 + j * LDH + 4 * q;
      const float* dr1 = dr0 + 16 * LDH;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i * 16 >= H2) break;
        const float w0 = wb[c][i][0], w1 = wb[c][i][1], w2 = wb[c][i][2], w3 = wb[c][i][3];
        const float4 d0 = *reinterpret_cast<const float4*>(dr0 + i * 16);
        const float4 d1 = *reinterpret_cast<const float4*>(dr1 + i * 16);
        acc0 = mfma4(d0.x, w0, acc0);
        acc1 = mfma4(d1.x, w0, acc1);
        acc0 = mfma4(d0.y, w1, acc0);
        acc1 = mfma4(d1.y, w1, acc1);
        acc0 = mfma4(d0.z, w2, acc0);
        acc1 = mfma4(d1.z, w2, acc1);
        acc0 = mfma4(d0.w, w3, acc0);
        acc1 = mfma4(d1.w, w3, acc1);
      }
      const int ic = cb * 16 + j;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r0 = 4 * q + i, r1 = r0 + 16;
        if constexpr (ACT == MLP_ACT_RELU && NORM == MLP_NORM_OFF && !RES) {
          dZ1[r0 * LDH + ic] = (A1[r0 * LDH + ic] > 0.f) ? acc0[i] * dscale : 0.f;
          dZ1[r1 * LDH + ic] = (A1[r1 * LDH + ic] > 0.f) ? acc1[i] * dscale : 0.f;
        } else if constexpr (RES) {  // + the skip's G = dZL Wl (K = H2 = H1, so ic < K)
          float g0 = 0.f, g1 = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < C) {
              g0 = fmaf(dZL[r0 * 4 + c], Wl[c * K + ic], g0);
              g1 = fmaf(dZL[r1 * 4 + c], Wl[c * K + ic], g1);
            }
          dZ1[r0 * LDH + ic] = (acc0[i] + g0) * dZ1[r0 * LDH + ic];
          dZ1[r1 * LDH + ic] = (acc1[i] + g1) * dZ1[r1 * LDH + ic];
        } else {
          dZ1[r0 * LDH + ic] = acc0[i] * dZ1[r0 * LDH + ic];  // layer 0's D, in place
          dZ1[r1 * LDH + ic] = acc1[i] * dZ1[r1 * LDH + ic];
        }
      }
    }
    // ---- dW1 = dZ2^T A1 on the MFMA (M = H2 outputs, N = H1 inputs, k = the tile's 32 rows)
    const int nib = H1 >> 4;
    const int ntile = (H2 >> 4) * nib;
    for (int t = wave; t < ntile; t += 4) {
      const int ob = t / nib, ib = t - ob * nib;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* dzp = dZ2 + q * LDH + ob * 16 + j;
      const float* ap = A1 + q * LDH + ib * 16 + j;
#pragma unroll
      for (int n = 0; n < R / 4; ++n) acc = mfma4(dzp[4 * n * LDH], ap[4 * n * LDH], acc);
      float* g = slot + tp.woff[1] + (size_t)(ob * 16 + 4 * q) * H1 + ib * 16 + j;
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i * H1] = acc[i];
    }
    if (tid < H2) {
      float g = 0.f;
      for (int r = 0; r < R; ++r) g += dZ2[r * LDH + tid];
      slot[tp.boff[1] + tid] = g;
    }
    __syncthreads();
    // ---- LayerNorm backward of layer 0
    if constexpr (NORM == MLP_NORM_RMS) rms_backward(0, H1, dZ1, XH1);
    else if constexpr (NORM != MLP_NORM_OFF) norm_backward(0, H1, dZ1, XH1);
  }

  // ---- dW0 = dZ1^T X0, db0 (VALU)
  for (int e = tid; e < H1 * D0; e += NT) {
    const int o = e / D0, k = e - o * D0;
    float g = 0.f;
    for (int r = 0; r < R; ++r) g = fmaf(dZ1[r * LDH + o], X0[r * LDX + k], g);
    slot[tp.woff[0] + e] = g;
  }
  if (tid < H1) {
    float g = 0.f;
    for (int r = 0; r < R; ++r) g += dZ1[r * LDH + tid];
    slot[tp.boff[0] + tid] = g;
  }
}

// The folded word e of an accumulation window (ACC): slots kb * T + t in ascending index.  Gradient words (e < P):
// (1 / accum) * sum_kb g_kb, g_kb the micro-batch's own mean gradient - its tiles already carry 1 / bs_kb, or
// (weighted) their sum over W_kb = the tiles' w[y] words in tile order, a micro-batch without a live row giving 0.
// The loss word (e == P): the mean loss of the last live micro-batch alone, n_live = min(accum, ceil(rows left / B)).
template <bool WL>
__device__ __forceinline__ float fold_window(const Plan& tp, const MlpStepArgs& a, int T, int e, int cur) {
  const float* w = a.tile_ws + e;
  const float* ww = a.tile_ws + tp.P + 1;
  if (e < tp.P) {
    float g = 0.f;
    if (WL) {
      for (int kb = 0; kb < a.accum; ++kb) {
        float gk = 0.f, W = 0.f;
#pragma unroll 8
        for (int t = 0; t < T; ++t) gk += w[(size_t)(kb * T + t) * tp.Pp];
#pragma unroll 8
        for (int t = 0; t < T; ++t) W += ww[(size_t)(kb * T + t) * tp.Pp];
        g += W > 0.f ? gk / W : 0.f;
      }
    } else {
      const int S = a.accum * T;
#pragma unroll 8
      for (int s = 0; s < S; ++s) g += w[(size_t)s * tp.Pp];
    }
    return g / (float)a.accum;
  }
  const long long left = (long long)a.n_items - (long long)cur * a.accum * a.B;  // rows from the window's first on
  if (left <= 0) return 0.f;
  const int n_live = (int)min((long long)a.accum, (left + a.B - 1) / a.B);
  const int kb = n_live - 1;
  float s = 0.f, W = 0.f;
#pragma unroll 8
  for (int t = 0; t < T; ++t) s += w[(size_t)(kb * T + t) * tp.Pp];
  if (WL) {
#pragma unroll 8
    for (int t = 0; t < T; ++t) W += ww[(size_t)(kb * T + t) * tp.Pp];
    return W > 0.f ? s / W : 0.f;
  }
  const long long bs = min((long long)a.B, left - (long long)kb * a.B);
  return s / (float)bs;
}

// The folded word e of a plain step: the T slots in ascending tile index.  Weighted: the slots hold un-normalised sums
// and W = the tiles' sums of w[y] in the same order - the same value in every thread, for every parameter and for the
// loss (0 only for a batch without a live row).  Unweighted: the plain sum - the tiles' gradients carry 1 / bs, the
// loss word does not (batch_mean).
template <bool WL>
__device__ __forceinline__ float fold_plain(const Plan& tp, const MlpStepArgs& a, int T, int e, int cur) {
  const float* w = a.tile_ws + e;
  float g = 0.f;
#pragma unroll 8
  for (int t = 0; t < T; ++t) g += w[(size_t)t * tp.Pp];
  if (WL) {
    const float* ww = a.tile_ws + tp.P + 1;
    float W = 0.f;
#pragma unroll 8
    for (int t = 0; t < T; ++t) W += ww[(size_t)t * tp.Pp];
    return W > 0.f ? g / W : 0.f;
  }
  return g;
}

// the unweighted plain step's loss word is the sum over the batch's live rows: its mean
__device__ __forceinline__ float batch_mean(const MlpStepArgs& a, int cur, float sum) {
  const int bs = max(0, min(a.B, a.n_items - cur * a.B));
  return bs > 0 ? sum / (float)bs : 0.f;
}

// The fold's train-mode branches as a function of the gradient word g, for the norm-clipped step's apply kernel: the
// optimizer (OPT: MlpArgs::opt_kind) on parameter e after tcur steps, statement for statement what the fold below does,
// so a clipped step differs from an unclipped one in g alone.  (The fold keeps its own copy: calling this from it
// reordered the Adam instantiations' bias-correction instructions, and an unclipped step's code is not to change.)
template <int OPT, class A>
__device__ __forceinline__ void opt_elem(const A& a, int e, float g, int tcur) {
  if constexpr (OPT == MLP_OPT_SGD) {
    const float lr_t = lr_for(a.lr_tab, a.lr, tcur);
    const bool mom = a.momentum != 0.f;  // (uniform: a kernel argument)
    float pv = a.p[e], mv = mom ? a.m[e] : 0.f;
    sgd_elem(pv, g, mv, lr_t, a.momentum, a.dampening, a.wd, a.nesterov != 0, tcur == 0);
    a.p[e] = pv;
    if (mom) a.m[e] = mv;
  } else {
    const int t = tcur + 1;
    const float bc1 = 1.f - pow_t(log2f(a.b1), (float)t);
    const float bc2 = 1.f - pow_t(log2f(a.b2), (float)t);
    const float lr_t = lr_for(a.lr_tab, a.lr, tcur);  // (next to the counter read above)
    const float step_size = lr_t / bc1;
    const float rbc2 = __builtin_amdgcn_rsqf(bc2);
    float pv = a.p[e], mv = a.m[e], vv = a.v[e];
    if (OPT == MLP_OPT_ADAMW) pv *= 1.f - lr_t * a.wd;
    adam_elem<OPT != MLP_OPT_ADAMW>(pv, g, mv, vv, a.b1, a.b2, a.wd, step_size, rbc2, a.eps);
    a.p[e] = pv;
    a.m[e] = mv;
    a.v[e] = vv;
  }
}

// the last workgroup of a launch to arrive advances the counters (every workgroup has read them by then) and leaves
// the arrival counter at zero, so a captured launch sequence replays
template <class A>
__device__ __forceinline__ void advance_counters(const A& a, unsigned int* done, int cur, int tcur) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned int old = atomicAdd(done, 1u);
    if (old == gridDim.x - 1) {
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.cursor) __hip_atomic_store(a.cursor, cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.step_counter) __hip_atomic_store(a.step_counter, tcur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// One word per thread through fold_plain, or (ACC: MlpArgs::accum > 1) the accum * T slots of a window through
// fold_window; then the optimizer (train mode) or grad_out (grad mode), the loss and the counters, which count
// optimizer steps.  OPT (MlpArgs::opt_kind, chosen on the host like WL and ACC): MLP_OPT_ADAM is the kernel as it was;
// MLP_OPT_ADAMW decays p by the step's rate times wd and runs adam_elem on the undecayed gradient; MLP_OPT_SGD
// (sgd_elem) touches p and the momentum buffer m only - first step (the buffer becomes the gradient) is device step
// count 0, the word Adam's bias correction reads.  Grad mode never reads OPT's fields: its launches use OPT = Adam.
// CLIP (MlpClipArgs::clip_kind, train mode only, chosen on the host likewise): MLP_CLIP_VALUE clamps the gradient word
// to [-clip_val, clip_val] before the optimizer sees it (a NaN stays one); clipping by norm needs the whole gradient
// first and is the kernel pair below, not an instantiation of this one.
// The Adam instantiations take MlpStepArgs, the arguments without the optimizer's fields (mlp_fused.h), the other
// unclipped ones MlpArgs, the arguments without the clip fields: their kernel-argument segment, and with it their
// code, is what it was before those fields existed.
template <int OPT, int CLIP = MLP_CLIP_OFF>
using FoldArgs = std::conditional_t<CLIP != MLP_CLIP_OFF, MlpClipArgs,
                                    std::conditional_t<OPT == MLP_OPT_ADAM, MlpStepArgs, MlpArgs>>;
static_assert(sizeof(MlpStepArgs) == 312 && sizeof(MlpArgs) == 328,
              "the unclipped tile kernels' kernel-argument types keep their size (README: 16 more bytes cost 1 %)");

template <bool WL, bool ACC, int OPT = MLP_OPT_ADAM, int CLIP = MLP_CLIP_OFF>
__global__ __launch_bounds__(FOLD_NT) void mlp_tile_fold_kernel(Plan tp, FoldArgs<OPT, CLIP> a, int T,
                                                                unsigned int* done) {
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_cnt[0] = a.cursor ? __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    s_cnt[1] = a.step_counter ? __hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.t0;
  }
  __syncthreads();
  const int cur = s_cnt[0], tcur = s_cnt[1];
  const bool adam = (a.mode == 0);
  const int e = blockIdx.x * FOLD_NT + tid;
  if (e <= tp.P) {
    // the step's gradient word (e < P) or loss word (e == P)
    float g = ACC ? fold_window<WL>(tp, a, T, e, cur) : fold_plain<WL>(tp, a, T, e, cur);
    if (e < tp.P) {
      if constexpr (CLIP == MLP_CLIP_VALUE)
        if (adam) g = g > a.clip_val ? a.clip_val : (g < -a.clip_val ? -a.clip_val : g);
      if constexpr (OPT == MLP_OPT_SGD) {
        if (adam) {
          const float lr_t = lr_for(a.lr_tab, a.lr, tcur);
          const bool mom = a.momentum != 0.f;  // (uniform: a kernel argument)
          float pv = a.p[e], mv = mom ? a.m[e] : 0.f;
          sgd_elem(pv, g, mv, lr_t, a.momentum, a.dampening, a.wd, a.nesterov != 0, tcur == 0);
          a.p[e] = pv;
          if (mom) a.m[e] = mv;
        } else {
          a.grad_out[e] = g;
        }
      } else if (adam) {
        const int t = tcur + 1;
        const float bc1 = 1.f - pow_t(log2f(a.b1), (float)t);
        const float bc2 = 1.f - pow_t(log2f(a.b2), (float)t);
        const float lr_t = lr_for(a.lr_tab, a.lr, tcur);  // (next to the counter read above)
        const float step_size = lr_t / bc1;
        const float rbc2 = __builtin_amdgcn_rsqf(bc2);
        float pv = a.p[e], mv = a.m[e], vv = a.v[e];
        if (OPT == MLP_OPT_ADAMW) pv *= 1.f - lr_t * a.wd;
        adam_elem<OPT != MLP_OPT_ADAMW>(pv, g, mv, vv, a.b1, a.b2, a.wd, step_size, rbc2, a.eps);
        a.p[e] = pv;
        a.m[e] = mv;
        a.v[e] = vv;
      } else {
        a.grad_out[e] = g;
      }
    } else {
      const float bl = (WL || ACC) ? g : batch_mean(a, cur, g);
      if (a.cursor && cur > 0 && a.loss_out) a.loss_out[cur - 1] = a.grad_out[tp.P];
      if (a.loss_out && !a.cursor) a.loss_out[0] = bl;
      if (!adam) a.grad_out[tp.P] = bl;
    }
  }
  advance_counters(a, done, cur, tcur);
}

// ---- clipping by norm: the fold and the optimizer as two kernels, with the global norm between them.
// fold_norm (grid ceil((P + 1) / 256), as the fold): thread e computes its word through fold_plain / fold_window - the
// bits a grad-mode launch writes - and stores it to gf[e] (the batch loss to gf[P]); the workgroup sums g^2 over its
// e < P in a fixed order - wave butterfly, then the four wave sums through LDS in wave order - into part[blockIdx.x],
// a plain vector store.  It reads the cursor (the window / live-row count of the fold) and advances nothing.
template <bool WL, bool ACC>
__global__ __launch_bounds__(FOLD_NT) void mlp_tile_fold_norm_kernel(Plan tp, MlpStepArgs a, int T, float* gf,
                                                                     float* part) {
  __shared__ int s_cur;
  __shared__ float wsums[FOLD_NT / 64];
  const int tid = threadIdx.x;
  if (tid == 0) s_cur = a.cursor ? __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
  __syncthreads();
  const int cur = s_cur;
  const int e = blockIdx.x * FOLD_NT + tid;
  float sq = 0.f;
  if (e <= tp.P) {
    const float g = ACC ? fold_window<WL>(tp, a, T, e, cur) : fold_plain<WL>(tp, a, T, e, cur);
    if (e < tp.P) {
      gf[e] = g;
      sq = g * g;
    } else {
      gf[e] = (WL || ACC) ? g : batch_mean(a, cur, g);
    }
  }
  sq = wave_sum(sq);
  if ((tid & 63) == 0) wsums[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) {
    float v = wsums[0];
#pragma unroll
    for (int w = 1; w < FOLD_NT / 64; ++w) v += wsums[w];
    part[blockIdx.x] = v;
  }
}

// apply (same grid, the launch behind fold_norm: the kernel boundary is what makes part[] visible across XCDs): every
// wave sums all gridDim.x <= 84 partials itself in one fixed order - lane l adds partials l, l + 64, .., then the
// butterfly - so every thread of the grid holds the same bits of norm and coef = min(clip_val / (norm + 1e-6), 1) with
// no broadcast through memory or LDS; then opt_elem on gf[e] * coef (the product also at coef == 1: exact), the loss
// word's bookkeeping and the counters as the fold.  Workgroup 0 leaves {norm, coef} in stats.
template <int OPT>
__global__ __launch_bounds__(FOLD_NT) void mlp_tile_apply_kernel(Plan tp, MlpClipArgs a, const float* gf,
                                                                 const float* part, float* stats,
                                                                 unsigned int* done) {
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_cnt[0] = a.cursor ? __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    s_cnt[1] = a.step_counter ? __hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.t0;
  }
  float t = 0.f;
  for (unsigned int i = tid & 63; i < gridDim.x; i += 64) t += part[i];
  t = wave_sum(t);
  const float norm = sqrtf(t);
  const float c = a.clip_val / (norm + 1e-6f);
  const float coef = c > 1.0f ? 1.0f : c;  // (a NaN stays a NaN, as torch.clamp(max=1))
  __syncthreads();
  const int cur = s_cnt[0], tcur = s_cnt[1];
  const int e = blockIdx.x * FOLD_NT + tid;
  if (e < tp.P) {
    float g;
    {
      // the clipped word is rounded on its own: contracted into SGD's g + wd p (fma(gf, coef, wd p)) it would not be
      // the unclipped step's fma(wd, p, g) at coef == 1
#pragma clang fp contract(off)
      g = gf[e] * coef;
    }
    opt_elem<OPT>(a, e, g, tcur);
  } else if (e == tp.P) {  // the fold's loss bookkeeping of a train-mode launch; gf[P] is the batch loss
    if (a.cursor && cur > 0 && a.loss_out) a.loss_out[cur - 1] = a.grad_out[tp.P];
    if (a.loss_out && !a.cursor) a.loss_out[0] = gf[e];
  }
  if (blockIdx.x == 0 && tid == 0) {
    stats[0] = norm;
    stats[1] = coef;
  }
  advance_counters(a, done, cur, tcur);
}

// clip_ws carve (floats, every part on a 16-byte boundary): gf[P + 1] | part[G] | {norm, coef}
struct ClipWs {
  int part, stats, total;
};
__host__ inline ClipWs clip_ws_layout(const Plan& tp) {
  ClipWs o;
  const int G = (tp.P + 1 + FOLD_NT - 1) / FOLD_NT;
  o.part = (tp.P + 1 + 3) & ~3;
  o.stats = o.part + ((G + 3) & ~3);
  o.total = o.stats + 4;
  return o;
}

// the fold of a launch: the Adam instantiation (the kernel as it was, on the kernel arguments it always had) for Adam
// and for every grad-mode launch
template <bool WL, bool ACC>
static void launch_fold(int grid, const Plan& tp, const MlpArgs& a, int T, unsigned int* done, hipStream_t st) {
  const int opt = a.mode == 0 ? a.opt_kind : (int)MLP_OPT_ADAM;
  const dim3 g(grid), b(FOLD_NT);
  if (opt == MLP_OPT_ADAM) {
    const MlpStepArgs& base = a;
    hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_ADAM>), g, b, 0, st, tp, base, T, done);
  } else if (opt == MLP_OPT_ADAMW) {
    hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_ADAMW>), g, b, 0, st, tp, a, T, done);
  } else {
    hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_SGD>), g, b, 0, st, tp, a, T, done);
  }
}

// what follows the step kernel of a clipped train-mode launch: by value the fold's clamping instantiation, by norm
// fold_norm + apply over the launch's clip_ws
template <bool WL, bool ACC>
static void launch_fold_clipped(int grid, const Plan& tp, const MlpClipArgs& a, int T, unsigned int* done,
                                hipStream_t st) {
  const dim3 g(grid), b(FOLD_NT);
  if (a.clip_kind == MLP_CLIP_VALUE) {
    if (a.opt_kind == MLP_OPT_ADAM)
      hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_ADAM, MLP_CLIP_VALUE>), g, b, 0, st, tp, a, T, done);
    else if (a.opt_kind == MLP_OPT_ADAMW)
      hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_ADAMW, MLP_CLIP_VALUE>), g, b, 0, st, tp, a, T, done);
    else
      hipLaunchKernelGGL((mlp_tile_fold_kernel<WL, ACC, MLP_OPT_SGD, MLP_CLIP_VALUE>), g, b, 0, st, tp, a, T, done);
    return;
  }
  const ClipWs cw = clip_ws_layout(tp);
  float* gf = a.clip_ws;
  float* part = a.clip_ws + cw.part;
  float* stats = a.clip_ws + cw.stats;
  const MlpStepArgs& base = a;
  hipLaunchKernelGGL((mlp_tile_fold_norm_kernel<WL, ACC>), g, b, 0, st, tp, base, T, gf, part);
  if (a.opt_kind == MLP_OPT_ADAM)
    hipLaunchKernelGGL((mlp_tile_apply_kernel<MLP_OPT_ADAM>), g, b, 0, st, tp, a, gf, part, stats, done);
  else if (a.opt_kind == MLP_OPT_ADAMW)
    hipLaunchKernelGGL((mlp_tile_apply_kernel<MLP_OPT_ADAMW>), g, b, 0, st, tp, a, gf, part, stats, done);
  else
    hipLaunchKernelGGL((mlp_tile_apply_kernel<MLP_OPT_SGD>), g, b, 0, st, tp, a, gf, part, stats, done);
}

// CLIPPED: a train-mode launch with a clip kind set - the same step kernel, launch_fold_clipped behind it
// ACT, NORM, RES: the step kernel's activation, norm kind and skip connection; the folds behind it know none of them
// (tp.P counts the norm's words)
template <int L, bool WL, bool ACC, bool CLIPPED = false, int ACT = MLP_ACT_RELU, int NORM = MLP_NORM_OFF,
          bool RES = false>
static hipError_t launch_steps(const Plan& tp, const std::conditional_t<CLIPPED, MlpClipArgs, MlpArgs>& a0,
                               unsigned int* done, hipStream_t st) {
  const int T = (a0.B + R - 1) / R;
  const size_t bytes = (size_t)lds_layout(L, NORM != MLP_NORM_OFF).total * sizeof(float);
  auto fn = mlp_tile_step_kernel<L, WL, ACC, ACT, NORM, RES>;
  const int AK = ACC ? a0.accum : 1;  // micro-batches per optimizer step: the index list advances by AK * B rows
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  const int fold_grid = (tp.P + 1 + FOLD_NT - 1) / FOLD_NT;
  for (int s = 0; s < a0.steps; ++s) {
    auto a = a0;
    a.steps = 1;
    a.idx = a0.idx + (size_t)s * AK * a0.B;
    a.n_items = a0.n_items - s * AK * a0.B;
    a.t0 = a0.t0 + s;
    a.step_base = a0.step_base + (uint32_t)s;
    if (a0.loss_out && !a0.cursor) a.loss_out = a0.loss_out + s;
    hipLaunchKernelGGL(fn, dim3(T, AK), dim3(NT), bytes, st, tp, a);
    if constexpr (CLIPPED) launch_fold_clipped<WL, ACC>(fold_grid, tp, a, T, done, st);
    else launch_fold<WL, ACC>(fold_grid, tp, a, T, done, st);
  }
  return hipGetLastError();
}

// the clipped launches' dispatch (defined behind dct_mlp_tile_train: their instantiations follow the unclipped ones)
static hipError_t train_clipped(const Plan& tp, const MlpClipArgs& a, int L, bool wl, bool acc, unsigned int* done,
                                hipStream_t st);
// the smooth activations' dispatch (likewise behind it, and behind the clipped ones)
static hipError_t train_act(const Plan& tp, const MlpActArgs& a, int L, bool wl, bool acc, unsigned int* done,
                            hipStream_t st);
// the normed models' dispatch (behind all of them), LayerNorm first
static hipError_t train_norm(const Plan& tp, const MlpNormArgs& a, int L, bool wl, bool acc, unsigned int* done,
                             hipStream_t st);
// the dispatch of the models with a skip connection (behind those): every norm kind, L == 3
static hipError_t train_res(const Plan& tp, const MlpNormArgs& a, bool wl, bool acc, unsigned int* done,
                            hipStream_t st);

}  // namespace tile

bool mlp_tile_batch_ok(int B) { return B >= 1 && B <= tile::BMAX; }
bool mlp_tile_window_ok(int B, int accum) {
  return mlp_tile_batch_ok(B) && (accum <= 1 || (long long)accum * ((B + tile::R - 1) / tile::R) <= tile::MAX_SLOTS);
}

// a train-mode launch's optimizer fields (grad mode ignores them): a known kind, wd >= 0, and for SGD torch's rules -
// momentum >= 0, Nesterov only with momentum > 0 and no dampening; p, and the moments the optimizer reads, bound
bool mlp_tile_optimizer_ok(const MlpArgs& a) {
  if (a.mode != 0) return true;
  if (a.opt_kind != MLP_OPT_ADAM && a.opt_kind != MLP_OPT_ADAMW && a.opt_kind != MLP_OPT_SGD) return false;
  if (a.opt_kind == MLP_OPT_ADAM) return true;  // (the launch as it always was: nothing new refused)
  if (!(a.wd >= 0.f) || !a.p) return false;
  if (a.opt_kind == MLP_OPT_ADAMW) return a.m && a.v;
  if (!(a.momentum >= 0.f)) return false;
  if (a.nesterov && (a.momentum <= 0.f || a.dampening != 0.f)) return false;
  return a.momentum == 0.f || a.m;
}

bool mlp_tile_clip_ok(const MlpClipArgs& a) {
  if (a.mode != 0 || a.clip_kind == MLP_CLIP_OFF) return true;
  if (a.clip_kind != MLP_CLIP_NORM && a.clip_kind != MLP_CLIP_VALUE) return false;
  return a.clip_val > 0.f && a.clip_val <= 3.402823466e38f;  // finite and > 0 (a NaN fails the first comparison)
}

}  // namespace dct

extern "C" {

int dct_mlp_tile_supported(const int* dims, int L) {
  dct::tile::Plan tp;
  return dct::tile::make_plan(&tp, dims, L) ? 1 : 0;
}

// floats of the slot workspace for batches up to B: [ceil(B / R)][Pp] slots + the fold's arrival counter
long long dct_mlp_tile_ws_floats(const int* dims, int L, int B) {
  dct::tile::Plan tp;
  if (!dct::tile::make_plan(&tp, dims, L) || B < 1 || B > dct::tile::BMAX) return 0;
  const long long T = (B + dct::tile::R - 1) / dct::tile::R;
  return T * tp.Pp + 4;
}

long long dct_mlp_tile_ws_floats_accum(const int* dims, int L, int B, int accum) {
  if (accum <= 1) return dct_mlp_tile_ws_floats(dims, L, B);
  dct::tile::Plan tp;
  if (!dct::tile::make_plan(&tp, dims, L) || !dct::mlp_tile_window_ok(B, accum)) return 0;
  const long long T = (B + dct::tile::R - 1) / dct::tile::R;
  return accum * T * tp.Pp + 4;
}

int dct_mlp_tile_max_slots(void) { return dct::tile::MAX_SLOTS; }

long long dct_mlp_tile_clip_ws_floats(const int* dims, int L) {
  dct::tile::Plan tp;
  return dct::tile::make_plan(&tp, dims, L) ? dct::tile::clip_ws_layout(tp).total : 0;
}

long long dct_mlp_tile_ws_floats_norm(const int* dims, int L, int B, int accum, int norm) {
  if (!norm) return dct_mlp_tile_ws_floats_accum(dims, L, B, accum);
  dct::tile::Plan tp;
  if (!dct::mlp_norm_ok(norm) || !dct::tile::make_plan(&tp, dims, L, norm) || !dct::mlp_tile_window_ok(B, accum)) return 0;
  const long long T = (B + dct::tile::R - 1) / dct::tile::R;
  return (accum > 1 ? accum : 1) * T * tp.Pp + 4;
}

long long dct_mlp_tile_clip_ws_floats_norm(const int* dims, int L, int norm) {
  dct::tile::Plan tp;
  return dct::mlp_norm_ok(norm) && dct::tile::make_plan(&tp, dims, L, norm) ? dct::tile::clip_ws_layout(tp).total : 0;
}

long long dct_mlp_tile_num_params(const int* dims, int L, int norm) {
  dct::tile::Plan tp;
  return dct::mlp_norm_ok(norm) && dct::tile::make_plan(&tp, dims, L, norm) ? tp.P : 0;
}

int dct_mlp_tile_train(const int* dims, int L, const dct::MlpResArgs* a, void* stream) {
  dct::tile::Plan tp;
  if (!dct::mlp_norm_ok(a->norm_kind)) return (int)hipErrorInvalidValue;
  const int norm = a->norm_kind;
  if (!dct::tile::plan_launch(&tp, dims, L, a->p, norm)) return (int)hipErrorInvalidValue;
  if (!dct::mlp_residual_ok(dims, L, a->residual)) return (int)hipErrorInvalidValue;
  if (!dct::mlp_act_ok(a->act_kind)) return (int)hipErrorInvalidValue;
  if (a->B < 1 || a->B > dct::tile::BMAX || a->steps < 1 || a->n_items < 1) return (int)hipErrorInvalidValue;
  if (a->mode == 1 && a->steps != 1) return (int)hipErrorInvalidValue;
  const int accum = a->accum > 1 ? a->accum : 1;
  if (a->accum < 0 || !dct::mlp_tile_window_ok(a->B, accum)) return (int)hipErrorInvalidValue;
  if (!a->cursor && (long long)(a->steps - 1) * accum * a->B >= a->n_items) return (int)hipErrorInvalidValue;
  if (a->xg_world > 1 || a->pending) return (int)hipErrorInvalidValue;
  if (!dct::mlp_tile_optimizer_ok(*a)) return (int)hipErrorInvalidValue;
  if (!(a->label_smooth >= 0.f && a->label_smooth < 1.f)) return (int)hipErrorInvalidValue;
  if ((a->class_w || a->label_smooth != 0.f) && a->loss_kind != 0) return (int)hipErrorInvalidValue;  // CE only
  if (!a->tile_ws || a->tile_ws_floats < dct_mlp_tile_ws_floats_norm(dims, L, a->B, accum, norm))
    return (int)hipErrorInvalidValue;
  unsigned int* done = reinterpret_cast<unsigned int*>(a->tile_ws + (a->tile_ws_floats - 4));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool wl = a->class_w || a->label_smooth != 0.f;
  if (!dct::mlp_tile_clip_ok(*a)) return (int)hipErrorInvalidValue;
  const bool clipped = a->mode == 0 && a->clip_kind != dct::MLP_CLIP_OFF;
  if (clipped && a->clip_kind == dct::MLP_CLIP_NORM &&
      (!a->clip_ws || ((uintptr_t)a->clip_ws & 15) || a->clip_ws_floats < dct_mlp_tile_clip_ws_floats_norm(dims, L, norm)))
    return (int)hipErrorInvalidValue;
  // a skip connection: its own step-kernel instantiations for every norm kind and activation
  if (a->residual) return (int)dct::tile::train_res(tp, *a, wl, accum > 1, done, st);
  // LayerNorm / RMSNorm: their own step-kernel instantiations for every activation, in train and grad mode alike
  if (norm) return (int)dct::tile::train_norm(tp, *a, L, wl, accum > 1, done, st);
  // a smooth activation: its own step-kernel instantiations in train and grad mode alike, every fold as it is
  if (a->act_kind != dct::MLP_ACT_RELU) return (int)dct::tile::train_act(tp, *a, L, wl, accum > 1, done, st);
  if (clipped) {
    return (int)dct::tile::train_clipped(tp, *a, L, wl, accum > 1, done, st);
  }
  // (the plain instantiations first: they keep their place at the head of the code object)
  if (accum <= 1) {
    if (wl)
      return (int)(L == 2 ? dct::tile::launch_steps<2, true, false>(tp, *a, done, st)
                          : dct::tile::launch_steps<3, true, false>(tp, *a, done, st));
    return (int)(L == 2 ? dct::tile::launch_steps<2, false, false>(tp, *a, done, st)
                        : dct::tile::launch_steps<3, false, false>(tp, *a, done, st));
  }
  if (wl)
    return (int)(L == 2 ? dct::tile::launch_steps<2, true, true>(tp, *a, done, st)
                        : dct::tile::launch_steps<3, true, true>(tp, *a, done, st));
  return (int)(L == 2 ? dct::tile::launch_steps<2, false, true>(tp, *a, done, st)
                      : dct::tile::launch_steps<3, false, true>(tp, *a, done, st));
}

}  // extern "C"

namespace dct {
namespace tile {

static hipError_t train_clipped(const Plan& tp, const MlpClipArgs& a, int L, bool wl, bool acc, unsigned int* done,
                                hipStream_t st) {
  if (!acc) {
    if (wl)
      return L == 2 ? launch_steps<2, true, false, true>(tp, a, done, st)
                    : launch_steps<3, true, false, true>(tp, a, done, st);
    return L == 2 ? launch_steps<2, false, false, true>(tp, a, done, st)
                  : launch_steps<3, false, false, true>(tp, a, done, st);
  }
  if (wl)
    return L == 2 ? launch_steps<2, true, true, true>(tp, a, done, st)
                  : launch_steps<3, true, true, true>(tp, a, done, st);
  return L == 2 ? launch_steps<2, false, true, true>(tp, a, done, st)
                : launch_steps<3, false, true, true>(tp, a, done, st);
}

template <int ACT, bool CLIPPED, int NORM = MLP_NORM_OFF, bool RES = false>
static hipError_t train_act_steps(const Plan& tp, const MlpClipArgs& a, int L, bool wl, bool acc, unsigned int* done,
                                  hipStream_t st) {
  if constexpr (RES) {  // two hidden layers: no 2-layer instantiation exists
    if (L != 3) return hipErrorInvalidValue;
    if (!acc)
      return wl ? launch_steps<3, true, false, CLIPPED, ACT, NORM, true>(tp, a, done, st)
                : launch_steps<3, false, false, CLIPPED, ACT, NORM, true>(tp, a, done, st);
    return wl ? launch_steps<3, true, true, CLIPPED, ACT, NORM, true>(tp, a, done, st)
              : launch_steps<3, false, true, CLIPPED, ACT, NORM, true>(tp, a, done, st);
  } else {
  if (!acc) {
    if (wl)
      return L == 2 ? launch_steps<2, true, false, CLIPPED, ACT, NORM>(tp, a, done, st)
                    : launch_steps<3, true, false, CLIPPED, ACT, NORM>(tp, a, done, st);
    return L == 2 ? launch_steps<2, false, false, CLIPPED, ACT, NORM>(tp, a, done, st)
                  : launch_steps<3, false, false, CLIPPED, ACT, NORM>(tp, a, done, st);
  }
  if (wl)
    return L == 2 ? launch_steps<2, true, true, CLIPPED, ACT, NORM>(tp, a, done, st)
                  : launch_steps<3, true, true, CLIPPED, ACT, NORM>(tp, a, done, st);
  return L == 2 ? launch_steps<2, false, true, CLIPPED, ACT, NORM>(tp, a, done, st)
                : launch_steps<3, false, true, CLIPPED, ACT, NORM>(tp, a, done, st);
  }
}

template <int ACT, int NORM = MLP_NORM_OFF, bool RES = false>
static hipError_t train_act_kind(const Plan& tp, const MlpActArgs& a, int L, bool wl, bool acc, unsigned int* done,
                                 hipStream_t st) {
  if (a.mode == 0 && a.clip_kind != MLP_CLIP_OFF)
    return train_act_steps<ACT, true, NORM, RES>(tp, a, L, wl, acc, done, st);
  return train_act_steps<ACT, false, NORM, RES>(tp, a, L, wl, acc, done, st);
}

static hipError_t train_act(const Plan& tp, const MlpActArgs& a, int L, bool wl, bool acc, unsigned int* done,
                            hipStream_t st) {
  switch (a.act_kind) {
    case MLP_ACT_GELU: return train_act_kind<MLP_ACT_GELU>(tp, a, L, wl, acc, done, st);
    case MLP_ACT_GELU_TANH: return train_act_kind<MLP_ACT_GELU_TANH>(tp, a, L, wl, acc, done, st);
    case MLP_ACT_SILU: return train_act_kind<MLP_ACT_SILU>(tp, a, L, wl, acc, done, st);
    default: return hipErrorInvalidValue;
  }
}

// every activation of one (norm kind, skip) pair
template <int NORM, bool RES>
static hipError_t train_model(const Plan& tp, const MlpActArgs& a, int L, bool wl, bool acc, unsigned int* done,
                              hipStream_t st) {
  switch (a.act_kind) {
    case MLP_ACT_RELU: return train_act_kind<MLP_ACT_RELU, NORM, RES>(tp, a, L, wl, acc, done, st);
    case MLP_ACT_GELU: return train_act_kind<MLP_ACT_GELU, NORM, RES>(tp, a, L, wl, acc, done, st);
    case MLP_ACT_GELU_TANH: return train_act_kind<MLP_ACT_GELU_TANH, NORM, RES>(tp, a, L, wl, acc, done, st);
    case MLP_ACT_SILU: return train_act_kind<MLP_ACT_SILU, NORM, RES>(tp, a, L, wl, acc, done, st);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t train_norm(const Plan& tp, const MlpNormArgs& a, int L, bool wl, bool acc, unsigned int* done,
                             hipStream_t st) {
  if (a.norm_kind == MLP_NORM_LAYER) return train_model<MLP_NORM_LAYER, false>(tp, a, L, wl, acc, done, st);
  return train_model<MLP_NORM_RMS, false>(tp, a, L, wl, acc, done, st);
}

static hipError_t train_res(const Plan& tp, const MlpNormArgs& a, bool wl, bool acc, unsigned int* done,
                            hipStream_t st) {
  switch (a.norm_kind) {
    case MLP_NORM_OFF: return train_model<MLP_NORM_OFF, true>(tp, a, 3, wl, acc, done, st);
    case MLP_NORM_LAYER: return train_model<MLP_NORM_LAYER, true>(tp, a, 3, wl, acc, done, st);
    default: return train_model<MLP_NORM_RMS, true>(tp, a, 3, wl, acc, done, st);
  }
}

}  // namespace tile
}  // namespace dct
