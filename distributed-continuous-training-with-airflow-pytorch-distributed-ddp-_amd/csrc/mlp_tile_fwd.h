// mlp_tile_fwd: the forward pass of a 32-row tile, shared by the batch-tiled trainer (mlp_tile.hip) and the
// batch-tiled inference kernel (mlp_infer.hip): the shape rule and flat offsets, the host check of a launch, and
// the device pieces each kernel calls in its own order - W1 fragment load, weight staging, layer 0 on the VALU,
// layer 1 on v_mfma_f32_16x16x4_f32 (exact fp32), head logits.  The gather, the loss and the LDS carve stay with
// each kernel.  Layers 0 and 1 hand every post-ReLU value to an epilogue epi(layer, row in the tile, unit, z):
// the trainer's dropout, the inference kernel's identity.  With a smooth activation (GELU, tanh-GELU, SiLU) they hand
// over the pre-activation instead and the epilogue applies act_grad / ActEpilogue below.  With LayerNorm (make_plan's
// norm) the layers store the pre-norm z + b through NoEpilogue and norm_rows normalises the image in place, handing
// u = gamma * xhat + beta and xhat to its own epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_fused.h"

namespace dct {
namespace tile {

constexpr int R = 32;     // rows per tile
constexpr int NT = 256;   // 4 waves
constexpr int LDH = 132;  // LDS row stride of the hidden activations / dZ (128 + 4)
constexpr int LDX = 33;   // LDS row stride of the input tile and of W0

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Plan {
  int L;        // 2 or 3 linear layers
  int D0, H1, H2, C;  // H2 = 0 when L == 2
  int K;        // width feeding the head (H2, or H1 when L == 2)
  int woff[3], boff[3];  // torch flat offsets (layer 2 unused when L == 2; the head is layer L - 1)
  int P, Pp;    // parameters, slot stride of the trainer's workspace (floats)
};
// With LayerNorm the flat buffer carries gamma_1 [H1], beta_1 [H1] (, gamma_2 [H2], beta_2 [H2]) behind the head's bias:
// P and Pp count them, woff / boff do not move, and the tail needs no field of its own.  With RMSNorm (norm = 2,
// MLP_NORM_RMS) there is no beta: gamma_1 [H1] (, gamma_2 [H2]).
__host__ __device__ inline int norm_words(int norm) {  // vectors per hidden layer of an MlpNorm kind
  return norm == MLP_NORM_OFF ? 0 : (norm == MLP_NORM_RMS ? 1 : 2);
}
__host__ __device__ inline int norm_off(const Plan& tp, int layer, int norm = MLP_NORM_LAYER) {  // gamma of hidden layer 0 / 1
  return tp.boff[tp.L - 1] + tp.C + (layer == 0 ? 0 : norm_words(norm) * tp.H1);  // (LayerNorm: beta = + H)
}

// Shapes: 2 or 3 linear layers, D0 1..32, hidden widths multiples of 16 in 16..128, C 2..4.  norm: the MlpNorm kind.
static inline bool make_plan(Plan* tp, const int* dims, int L, int norm = 0) {
  if (L != 2 && L != 3) return false;
  const int D0 = dims[0], C = dims[L];
  if (D0 < 1 || D0 > 32 || C < 2 || C > 4) return false;
  for (int l = 1; l < L; ++l)
    if (dims[l] < 16 || dims[l] > 128 || dims[l] % 16 != 0) return false;
  *tp = Plan{};
  tp->L = L;
  tp->D0 = D0;
  tp->H1 = dims[1];
  tp->H2 = (L == 3) ? dims[2] : 0;
  tp->C = C;
  tp->K = dims[L - 1];
  int flat = 0;
  for (int l = 0; l < L; ++l) {
    tp->woff[l] = flat;
    flat += dims[l] * dims[l + 1];
    tp->boff[l] = flat;
    flat += dims[l + 1];
  }
  flat += norm_words(norm) * (tp->H1 + tp->H2);
  tp->P = flat;
  tp->Pp = (flat + 2 + 3) & ~3;  // [P] gradients, the loss sum, the weighted loss's sum of w[y]
  return true;
}

// What both launchers ask before anything else: a shape make_plan takes, and parameters on a 16-byte boundary -
// load_w1_frags reads W1 as float4 (woff[1] = (D0 + 1) * H1 floats keeps the alignment of p).
static inline bool plan_launch(Plan* tp, const int* dims, int L, const float* p, int norm = 0) {
  return make_plan(tp, dims, L, norm) && p && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

struct NoEpilogue {
  __device__ __forceinline__ float operator()(int, int, int, float z) const { return z; }
};

// ---- the smooth activations (MlpAct 1 .. 3; ACT = 0, ReLU, is the fmaxf in layer0 / layer1_block themselves).
// act_grad returns act(z) and leaves act'(z) in d; both come from ONE transcendental's worth of shared terms, in fp32
// with the full-precision library functions:
//   gelu       Phi = 0.5 (1 + erff(z / sqrt 2)), phi = exp(-z^2 / 2) / sqrt(2 pi):  z Phi,  Phi + z phi
//   gelu_tanh  t = tanhf(c (z + 0.044715 z^3)), c = sqrt(2 / pi):  0.5 z (1 + t),
//              0.5 (1 + t) + 0.5 z (1 - t^2) c (1 + 3 * 0.044715 z^2)     (torch's approximate="tanh" and its backward)
//   silu       s = 1 / (1 + expf(-z)):  z s,  s (1 + z (1 - s))
// Every value is finite for a finite z of any size the forward can produce (exp underflows to 0, s to 0 or 1), so
// 0 * act' is an exact zero - what the trainer's backward relies on for the rows beyond the batch.
template <int ACT>
__device__ __forceinline__ float act_grad(float z, float& d) {
  static_assert(ACT >= 1 && ACT <= 3, "a smooth MlpAct");
  if constexpr (ACT == 1) {
    const float Phi = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    const float phi = 0.39894228040143267794f * expf(-0.5f * z * z);
    d = fmaf(z, phi, Phi);
    return z * Phi;
  } else if constexpr (ACT == 2) {
    const float c = 0.79788456080286535588f, k = 0.044715f;
    const float z2 = z * z;
    const float t = tanhf(c * fmaf(k * z2, z, z));
    const float h = 0.5f * (1.0f + t);
    d = fmaf(0.5f * z * (1.0f - t * t), c * fmaf(3.0f * k, z2, 1.0f), h);
    return z * h;
  } else {
    const float s = 1.0f / (1.0f + expf(-z));
    d = s * fmaf(z, 1.0f - s, 1.0f);
    return z * s;
  }
}

// the forward alone (the inference kernel's epilogue): act_grad's value, its unused derivative left to the compiler
template <int ACT>
struct ActEpilogue {
  __device__ __forceinline__ float operator()(int, int, int, float z) const {
    float d;
    return act_grad<ACT>(z, d);
  }
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// This wave's W1 fragments of the layer-1 MFMA: column blocks wave, wave + 4, zero beyond H2 / H1.
__device__ __forceinline__ void load_w1_frags(float4 (&wf)[2][8], const float* w1, int H1, int H2, int wave, int j,
                                              int q) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int cb = wave + 4 * c;
    const float* wrow = w1 + (size_t)(cb * 16 + j) * H1 + 4 * q;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      wf[c][i] = (cb * 16 < H2 && i * 16 < H1) ? *reinterpret_cast<const float4*>(wrow + i * 16)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// W0 [H1][D0] with b0 in the pad column 32; the head weights [C][K] with the head bias at Wl[4 * 128 + c].
__device__ __forceinline__ void stage_weights(float* W0s, float* Wl, const float* p, const Plan& tp, int L, int tid) {
  for (int e = tid; e < tp.H1 * tp.D0; e += NT) {
    const int o = e / tp.D0, k = e - o * tp.D0;
    W0s[o * LDX + k] = p[tp.woff[0] + e];
  }
  for (int e = tid; e < tp.C * tp.K; e += NT) Wl[e] = p[tp.woff[L - 1] + e];
  if (tid < tp.C) Wl[4 * 128 + tid] = p[tp.boff[L - 1] + tid];
  if (tid < tp.H1) W0s[tid * LDX + 32] = p[tp.boff[0] + tid];
}

// Layer 0 (VALU): A1 = epi(relu(X0 W0^T + b0)).  ACT != 0 (a smooth MlpAct): epi gets the pre-activation z itself
// and applies the activation (ActEpilogue, or the trainer's, which also leaves act'(z) in the dZ image).
template <int ACT = 0, class Epi>
__device__ __forceinline__ void layer0(float* A1, const float* W0s, const float* X0, int D0, int H1, int tid,
                                       Epi epi) {
  for (int e = tid; e < R * H1; e += NT) {
    const int r = e / H1, o = e - r * H1;
    float z = W0s[o * LDX + 32];  // b0, staged in the pad column
    for (int k = 0; k < D0; ++k) z = fmaf(W0s[o * LDX + k], X0[r * LDX + k], z);
    A1[r * LDH + o] = epi(0, r, o, ACT == 0 ? fmaxf(z, 0.f) : z);
  }
}

// Column block cb of layer 1 (MFMA): A2[:, 16 cb ..] = epi(relu(A1 W1^T + b1)), two M = 16 row blocks per weight
// fragment; wf: the block's fragments from load_w1_frags, bv: b1 of this lane's unit 16 cb + j.  ACT as in layer0.
template <int ACT = 0, class Epi>
__device__ __forceinline__ void layer1_block(float* A2, const float* A1, const float4 (&wf)[8], int cb, float bv,
                                             int H1, int j, int q, Epi epi) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const float* ar0 = A1 + j * LDH + 4 * q;
  const float* ar1 = ar0 + 16 * LDH;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i * 16 >= H1) break;
    // k of MFMA t, lane group q: 16 i + 4 q + t (the same permutation on both operands)
    const float4 wv = wf[i];
    const float4 a0 = *reinterpret_cast<const float4*>(ar0 + i * 16);
    const float4 a1 = *reinterpret_cast<const float4*>(ar1 + i * 16);
    acc0 = mfma4(a0.x, wv.x, acc0);
    acc1 = mfma4(a1.x, wv.x, acc1);
    acc0 = mfma4(a0.y, wv.y, acc0);
    acc1 = mfma4(a1.y, wv.y, acc1);
    acc0 = mfma4(a0.z, wv.z, acc0);
    acc1 = mfma4(a1.z, wv.z, acc1);
    acc0 = mfma4(a0.w, wv.w, acc0);
    acc1 = mfma4(a1.w, wv.w, acc1);
  }
  const int o = cb * 16 + j;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r0 = 4 * q + i, r1 = r0 + 16;
    A2[r0 * LDH + o] = epi(1, r0, o, ACT == 0 ? fmaxf(acc0[i] + bv, 0.f) : acc0[i] + bv);
    A2[r1 * LDH + o] = epi(1, r1, o, ACT == 0 ? fmaxf(acc1[i] + bv, 0.f) : acc1[i] + bv);
  }
}

// LayerNorm of one hidden layer's image (VALU, 8 lanes per row in head_logits' thread-to-row mapping; the caller's
// barriers stand before and behind it): A [32][LDH] holds the pre-norm z + b of the layer's H units.  Lane `part` of
// row r strides units part, part + 8, ..: the mean first, then the centred sum of squares (two passes, as torch), each
// closed by the 3-step xor tree, so all 8 lanes hold the same bits of mean and rstd = rsqrt(biased var + eps).  The
// same lanes then sweep the row once more, xhat = (z - mean) rstd, u = gamma xhat + beta, and store
// A = epi(LI, r, unit, u, xhat): the activation (and what the trainer keeps for its backward).  gamma / beta: the flat
// buffer (L2 resident).  rs (may be null): rstd of the 32 rows.  A row of equal values has var = 0 and rstd =
// rsqrt(eps), finite.  Every element is read and written by one thread only.
template <class Epi>
__device__ __forceinline__ void norm_rows(float* A, float* rs, const float* gamma, const float* beta, int H, int LI,
                                          int tid, Epi epi) {
  const int r = tid >> 3, part = tid & 7;
  float* row = A + r * LDH;
  const float invH = 1.0f / (float)H;
  float s = 0.f;
  for (int k = part; k < H; k += 8) s += row[k];
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 4);
  const float mean = s * invH;
  float v = 0.f;
  for (int k = part; k < H; k += 8) {
    const float d = row[k] - mean;
    v = fmaf(d, d, v);
  }
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  const float rstd = rsqrtf(fmaf(v, invH, 1e-5f));
  if (rs && part == 0) rs[r] = rstd;
  for (int k = part; k < H; k += 8) {
    const float xhat = (row[k] - mean) * rstd;
    row[k] = epi(LI, r, k, fmaf(gamma[k], xhat, beta[k]), xhat);
  }
}

// RMSNorm of one hidden layer's image: norm_rows without the mean - the same 8 lanes per row make ONE pass for
// sum z^2, close it by the same xor tree, rstd = rsqrt(sum / H + eps), and sweep the row once more: xhat = z rstd,
// u = gamma xhat, A = epi(LI, r, unit, u, xhat).  An all-zero row has rstd = rsqrt(eps), finite, and xhat = u = 0.
template <class Epi>
__device__ __forceinline__ void rms_rows(float* A, float* rs, const float* gamma, int H, int LI, int tid, Epi epi) {
  const int r = tid >> 3, part = tid & 7;
  float* row = A + r * LDH;
  float v = 0.f;
  for (int k = part; k < H; k += 8) {
    const float z = row[k];
    v = fmaf(z, z, v);
  }
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  const float rstd = rsqrtf(fmaf(v, 1.0f / (float)H, 1e-5f));
  if (rs && part == 0) rs[r] = rstd;
  for (int k = part; k < H; k += 8) {
    const float xhat = row[k] * rstd;
    row[k] = epi(LI, r, k, gamma[k] * xhat, xhat);
  }
}

// the inference kernel's epilogue of norm_rows / rms_rows: act(u) alone (ACT = 0: ReLU)
template <int ACT>
struct NormActEpilogue {
  __device__ __forceinline__ float operator()(int, int, int, float u, float) const {
    if constexpr (ACT == 0) {
      return fmaxf(u, 0.f);
    } else {
      float d;
      return act_grad<ACT>(u, d);
    }
  }
};

// the same behind a skip connection (layer 1 only): skip[r][unit] + act(u), skip = the layer's input image A1
template <int ACT>
struct ResEpilogue {
  const float* skip;
  __device__ __forceinline__ float operator()(int, int r, int o, float u, float = 0.f) const {
    return skip[r * LDH + o] + NormActEpilogue<ACT>{}(0, r, o, u, 0.f);
  }
};

// Head (VALU, 8 lanes per row): z = the logits of row tid >> 3 (0 beyond C), in all 8 lanes after the xor tree.
__device__ __forceinline__ void head_logits(float (&z)[4], const float* Ah, const float* Wl, int C, int K, int tid) {
  const int r = tid >> 3, part = tid & 7;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = part; k < K; k += 8) {
    const float av = Ah[r * LDH + k];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < C) acc[c] = fmaf(Wl[c * K + k], av, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    acc[c] += __shfl_xor(acc[c], 1);
    acc[c] += __shfl_xor(acc[c], 2);
    acc[c] += __shfl_xor(acc[c], 4);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) z[c] = (c < C) ? acc[c] + Wl[4 * 128 + c] : 0.f;
}

}  // namespace tile
}  // namespace dct
