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
// for the 3-layer nets, 57.7 KB for the 2-layer ones).  No LDS-DMA loads.
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
  int x0, w0, wl, a1, dz1, a2, dz2, dzl, lossr, lab, total;
};
__host__ __device__ inline Lds lds_layout(int L) {
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
template <int L, bool WL, bool ACC>
__global__ __launch_bounds__(NT) void mlp_tile_step_kernel(Plan tp, MlpStepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds lo = lds_layout(L);
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
  layer0(A1, W0s, X0, D0, H1, tid, drop);
  __syncthreads();

  // ---- layer 1: A2 = dropout(relu(A1 W1^T + b1)); a wave owns column blocks wave, wave + 4
  if (L == 3) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int cb = wave + 4 * c;
      if (cb * 16 >= H2) break;
      layer1_block(A2, A1, wf[c], cb, a.p[tp.boff[1] + cb * 16 + j], H1, j, q, drop);
    }
    __syncthreads();
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
    const float av = Ah[r * LDH + k];
    dZh[r * LDH + k] = (av > 0.f) ? g * dscale : 0.f;
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
        dZ1[r0 * LDH + ic] = (A1[r0 * LDH + ic] > 0.f) ? acc0[i] * dscale : 0.f;
        dZ1[r1 * LDH + ic] = (A1[r1 * LDH + ic] > 0.f) ? acc1[i] * dscale : 0.f;
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

// One word per thread through fold_plain, or (ACC: MlpArgs::accum > 1) the accum * T slots of a window through
// fold_window; then the optimizer (train mode) or grad_out (grad mode), the loss and the counters, which count
// optimizer steps.  OPT (MlpArgs::opt_kind, chosen on the host like WL and ACC): MLP_OPT_ADAM is the kernel as it was;
// MLP_OPT_ADAMW decays p by the step's rate times wd and runs adam_elem on the undecayed gradient; MLP_OPT_SGD
// (sgd_elem) touches p and the momentum buffer m only - first step (the buffer becomes the gradient) is device step
// count 0, the word Adam's bias correction reads.  Grad mode never reads OPT's fields: its launches use OPT = Adam.
// The Adam instantiations take MlpStepArgs, the arguments without the optimizer's fields (mlp_fused.h): their
// kernel-argument segment, and with it their code, is what it was before those fields existed.
template <int OPT>
using FoldArgs = std::conditional_t<OPT == MLP_OPT_ADAM, MlpStepArgs, MlpArgs>;

template <bool WL, bool ACC, int OPT = MLP_OPT_ADAM>
__global__ __launch_bounds__(FOLD_NT) void mlp_tile_fold_kernel(Plan tp, FoldArgs<OPT> a, int T, unsigned int* done) {
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
    const float g = ACC ? fold_window<WL>(tp, a, T, e, cur) : fold_plain<WL>(tp, a, T, e, cur);
    if (e < tp.P) {
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
  // the last workgroup to arrive advances the counters: every workgroup has read them by then
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const unsigned int old = atomicAdd(done, 1u);
    if (old == gridDim.x - 1) {
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.cursor) __hip_atomic_store(a.cursor, cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.step_counter) __hip_atomic_store(a.step_counter, tcur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
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

template <int L, bool WL, bool ACC>
static hipError_t launch_steps(const Plan& tp, const MlpArgs& a0, unsigned int* done, hipStream_t st) {
  const int T = (a0.B + R - 1) / R;
  const size_t bytes = (size_t)lds_layout(L).total * sizeof(float);
  auto fn = mlp_tile_step_kernel<L, WL, ACC>;
  const int AK = ACC ? a0.accum : 1;  // micro-batches per optimizer step: the index list advances by AK * B rows
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  const int fold_grid = (tp.P + 1 + FOLD_NT - 1) / FOLD_NT;
  for (int s = 0; s < a0.steps; ++s) {
    MlpArgs a = a0;
    a.steps = 1;
    a.idx = a0.idx + (size_t)s * AK * a0.B;
    a.n_items = a0.n_items - s * AK * a0.B;
    a.t0 = a0.t0 + s;
    a.step_base = a0.step_base + (uint32_t)s;
    if (a0.loss_out && !a0.cursor) a.loss_out = a0.loss_out + s;
    hipLaunchKernelGGL(fn, dim3(T, AK), dim3(NT), bytes, st, tp, a);
    launch_fold<WL, ACC>(fold_grid, tp, a, T, done, st);
  }
  return hipGetLastError();
}

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

int dct_mlp_tile_train(const int* dims, int L, const dct::MlpArgs* a, void* stream) {
  dct::tile::Plan tp;
  if (!dct::tile::plan_launch(&tp, dims, L, a->p)) return (int)hipErrorInvalidValue;
  if (a->B < 1 || a->B > dct::tile::BMAX || a->steps < 1 || a->n_items < 1) return (int)hipErrorInvalidValue;
  if (a->mode == 1 && a->steps != 1) return (int)hipErrorInvalidValue;
  const int accum = a->accum > 1 ? a->accum : 1;
  if (a->accum < 0 || !dct::mlp_tile_window_ok(a->B, accum)) return (int)hipErrorInvalidValue;
  if (!a->cursor && (long long)(a->steps - 1) * accum * a->B >= a->n_items) return (int)hipErrorInvalidValue;
  if (a->xg_world > 1 || a->pending) return (int)hipErrorInvalidValue;
  if (!dct::mlp_tile_optimizer_ok(*a)) return (int)hipErrorInvalidValue;
  if (!(a->label_smooth >= 0.f && a->label_smooth < 1.f)) return (int)hipErrorInvalidValue;
  if ((a->class_w || a->label_smooth != 0.f) && a->loss_kind != 0) return (int)hipErrorInvalidValue;  // CE only
  if (!a->tile_ws || a->tile_ws_floats < dct_mlp_tile_ws_floats_accum(dims, L, a->B, accum))
    return (int)hipErrorInvalidValue;
  unsigned int* done = reinterpret_cast<unsigned int*>(a->tile_ws + (a->tile_ws_floats - 4));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool wl = a->class_w || a->label_smooth != 0.f;
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
