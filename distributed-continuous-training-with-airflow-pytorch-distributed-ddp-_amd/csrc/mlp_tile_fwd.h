// mlp_tile_fwd: the forward pass of a 32-row tile, shared by the batch-tiled trainer (mlp_tile.hip) and the
// batch-tiled inference kernel (mlp_infer.hip): the shape rule and flat offsets, the host check of a launch, and
// the device pieces each kernel calls in its own order - W1 fragment load, weight staging, layer 0 on the VALU,
// layer 1 on v_mfma_f32_16x16x4_f32 (exact fp32), head logits.  The gather, the loss and the LDS carve stay with
// each kernel.  Layers 0 and 1 hand every post-ReLU value to an epilogue epi(layer, row in the tile, unit, z):
// the trainer's dropout, the inference kernel's identity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// Shapes: 2 or 3 linear layers, D0 1..32, hidden widths multiples of 16 in 16..128, C 2..4.
static inline bool make_plan(Plan* tp, const int* dims, int L) {
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
  tp->P = flat;
  tp->Pp = (flat + 2 + 3) & ~3;  // [P] gradients, the loss sum, the weighted loss's sum of w[y]
  return true;
}

// What both launchers ask before anything else: a shape make_plan takes, and parameters on a 16-byte boundary -
// load_w1_frags reads W1 as float4 (woff[1] = (D0 + 1) * H1 floats keeps the alignment of p).
static inline bool plan_launch(Plan* tp, const int* dims, int L, const float* p) {
  return make_plan(tp, dims, L) && p && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

struct NoEpilogue {
  __device__ __forceinline__ float operator()(int, int, int, float z) const { return z; }
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

// Layer 0 (VALU): A1 = epi(relu(X0 W0^T + b0))
template <class Epi>
__device__ __forceinline__ void layer0(float* A1, const float* W0s, const float* X0, int D0, int H1, int tid,
                                       Epi epi) {
  for (int e = tid; e < R * H1; e += NT) {
    const int r = e / H1, o = e - r * H1;
    float z = W0s[o * LDX + 32];  // b0, staged in the pad column
    for (int k = 0; k < D0; ++k) z = fmaf(W0s[o * LDX + k], X0[r * LDX + k], z);
    A1[r * LDH + o] = epi(0, r, o, fmaxf(z, 0.f));
  }
}

// Column block cb of layer 1 (MFMA): A2[:, 16 cb ..] = epi(relu(A1 W1^T + b1)), two M = 16 row blocks per weight
// fragment; wf: the block's fragments from load_w1_frags, bv: b1 of this lane's unit 16 cb + j.
template <class Epi>
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
    A2[r0 * LDH + o] = epi(1, r0, o, fmaxf(acc0[i] + bv, 0.f));
    A2[r1 * LDH + o] = epi(1, r1, o, fmaxf(acc1[i] + bv, 0.f));
  }
}

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
