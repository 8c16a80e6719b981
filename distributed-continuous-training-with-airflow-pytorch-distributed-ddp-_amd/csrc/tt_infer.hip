// tt_infer: whole-model forward-only TabTransformer inference (BASELINE.json config 5: 64 feature tokens, d_model 64,
// 4 heads of 16, FFN 256; 1..8 blocks, 2..8 classes) - Trainer.validate / test / predict in ONE launch.
//
//   infer kernel (grid G, 256 threads, persistent over samples): a workgroup carries one sample from its table row to
//     its logits without leaving the CU.  The sample's 64 features are staged in LDS (optionally (x - mean) / std, the
//     scoring script's "raw" contract); the first block's LN1 forms the token rows x E + c with the embedding kernel's
//     fmaf; the fp32 residual tile (64 x HS_LD) then stays in LDS through all L blocks.  A block is
//     tt_block_fwd_kernel's (tt_block.hip) phase by phase - LN1 | QKV on v_mfma_f32_16x16x32_bf16, one head per wave |
//     attention on 16x16x16, exp2-domain softmax | projection + residual | LN2 | FC1 + erf-GELU with swapped operands
//     | FC2 + residual - with the same wave-to-column split, the same bf16 rounding points (LN outputs, q / k / v, P,
//     o, F) and fp32 accumulation, so a trained model scores with the arithmetic it was trained with.  Weights stream
//     from L2 as MFMA B fragments out of ONE bf16 image per block (Wqkv | Wo | W1 | W2, W_STRIDE elements) and one fp32
//     vector image (ln1_w, ln1_b, bqkv, bo, ln2_w, ln2_b, b1, b2, V_STRIDE floats): two base pointers and L.
//     The last block's FC2 epilogue leaves the token mean (64 floats) in LDS instead of the tile, and wave 0 runs the
//     training head's chain (tt_io.hip head_chain) in fp32 on fp32 parameters it holds in registers, lane = dimension:
//     LayerNorm, Linear(64, C), max, exp, log -> logits / softmax probabilities / argmax, each written only when its
//     pointer is given.  Meanwhile wave 1 stages the next sample's features, which it loaded a sample ahead.
//     Nothing per-sample reaches HBM except the requested outputs: 256 B in, 4 C bytes out.
//   statistics (labels given): mlp_infer.hip's contract and scheme.  The n samples are cut into at most 4096 slots of
//     S = ceil(n / 4096) consecutive samples; a workgroup owns whole slots (s, s + G, ...), sums a slot in ascending
//     sample order - the loss in fp64, the counts as 64-bit integers, confusion cell k in lane k of wave 0 - and writes
//     it with plain vector stores.  A fold launch (grid 2 + C * C, one wave each) adds word e of the slots in a fixed
//     order.  No atomics, no tickets: the statistics words and every output are bit-identical whatever the grid.
//
// LDS: 68.5 KB (residual 17 KB, LN / attention outputs 9 KB each, QKV then FFN hidden 33 KB, features and token mean
// 256 B each) - two workgroups per CU, as in training.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dct_common.h"
#include "kernels.h"

namespace dct {
namespace tti {

constexpr int T = 64, DM = 64, NH = 4, DH = 16, FF = 256;
constexpr int HS_LD = DM + 4;       // fp32 residual rows (272 B)
constexpr int AS_LD = DM + 8;       // bf16 LN output / attention output rows (144 B)
constexpr int QKV_LD = 3 * DM + 8;  // bf16 (400 B)
constexpr int F_LD = FF + 8;        // bf16 (528 B)
constexpr int HS_BYTES = T * HS_LD * 4;
constexpr int AS_BYTES = T * AS_LD * 2;
constexpr int R_BYTES = T * F_LD * 2;  // QKV (25.6 KB) then FFN hidden (33.8 KB)
constexpr int LDS_BYTES = HS_BYTES + 2 * AS_BYTES + R_BYTES + 2 * DM * 4;
static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");

// element offsets in a block's bf16 weight image and fp32 vector image
constexpr int W_QKV = 0, W_O = 3 * DM * DM, W_1 = W_O + DM * DM, W_2 = W_1 + FF * DM, W_STRIDE = W_2 + DM * FF;
constexpr int V_LN1W = 0, V_LN1B = DM, V_BQKV = 2 * DM, V_BO = 5 * DM, V_LN2W = 6 * DM, V_LN2B = 7 * DM, V_B1 = 8 * DM,
              V_B2 = 8 * DM + FF, V_STRIDE = 9 * DM + FF;
static_assert(W_STRIDE == 49152 && V_STRIDE == 832, "the host packs these strides (ops/nn.py tt_infer)");

constexpr int LMAX = 8, CMIN = 2, CMAX = 8;
constexpr int MAX_SLOTS = 4096;
constexpr int SLOT_WORDS = 2 + CMAX * CMAX;  // 8-byte words per slot: loss (fp64), correct, confusion cells
constexpr int FOLD_NT = 64;
constexpr int MAX_GRID = 65536;

// samples per slot and slots of n samples
struct Slots {
  long long S;
  int nslots;
};
static Slots slots_of(long long n) {
  Slots o;
  o.S = (n + MAX_SLOTS - 1) / MAX_SLOTS;
  o.nslots = (int)((n + o.S - 1) / o.S);
  return o;
}

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(bf16x4 a, bf16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float sum4g(float v) {  // over lanes l, l^16, l^32, l^48
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ float max4g(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}
__device__ __forceinline__ bf16x4 pack4(f32x4 v) {
  bf16x4 r;
  r[0] = (short)f32_to_bf16(v[0]); r[1] = (short)f32_to_bf16(v[1]);
  r[2] = (short)f32_to_bf16(v[2]); r[3] = (short)f32_to_bf16(v[3]);
  return r;
}

// LayerNorm of the wave's 16 rows: lane -> row 16 wv + (lane & 15), columns 16 g .. 16 g + 15 (tt_block.hip
// layer_norm_rows).  EMBED: the fp32 row is the feature token XS[row] * E[row] + c[row] and is written to HS;
// otherwise it is read from HS.  The bf16 normalised row goes to AS.
template <bool EMBED>
__device__ __forceinline__ void layer_norm_rows(float* HS, uint16_t* AS, const float* XS, const float* E,
                                                const float* cb, const float* w, const float* b, float eps) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = 16 * wv + (lane & 15), g = lane >> 4;
  float v[16];
  float4* hp = reinterpret_cast<float4*>(HS + r * HS_LD + 16 * g);
  if (EMBED) {
    const float xv = XS[r];
    const float4* ep = reinterpret_cast<const float4*>(E + r * DM + 16 * g);
    const float4* cp = reinterpret_cast<const float4*>(cb + r * DM + 16 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 e = ep[q], cc = cp[q];
      v[4 * q] = fmaf(xv, e.x, cc.x); v[4 * q + 1] = fmaf(xv, e.y, cc.y);
      v[4 * q + 2] = fmaf(xv, e.z, cc.z); v[4 * q + 3] = fmaf(xv, e.w, cc.w);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = hp[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) s += v[e];
  const float mean = sum4g(s) * (1.f / DM);
  float qv = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) { const float d = v[e] - mean; qv += d * d; }
  const float rstd = rsqrtf(sum4g(qv) * (1.f / DM) + eps);
  if (EMBED) {
#pragma unroll
    for (int q = 0; q < 4; ++q) hp[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
  float wv4[16], bv4[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 tw = reinterpret_cast<const float4*>(w + 16 * g)[q];
    const float4 tb = reinterpret_cast<const float4*>(b + 16 * g)[q];
    wv4[4 * q] = tw.x; wv4[4 * q + 1] = tw.y; wv4[4 * q + 2] = tw.z; wv4[4 * q + 3] = tw.w;
    bv4[4 * q] = tb.x; bv4[4 * q + 1] = tb.y; bv4[4 * q + 2] = tb.z; bv4[4 * q + 3] = tb.w;
  }
  bf16x8 o0, o1;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o0[e] = (short)f32_to_bf16((v[e] - mean) * rstd * wv4[e] + bv4[e]);
    o1[e] = (short)f32_to_bf16((v[e + 8] - mean) * rstd * wv4[e + 8] + bv4[e + 8]);
  }
  *reinterpret_cast<bf16x8*>(AS + r * AS_LD + 16 * g) = o0;
  *reinterpret_cast<bf16x8*>(AS + r * AS_LD + 16 * g + 8) = o1;
}

// QKV = a1 Wqkv^T + bqkv for head wv (Q, K, V column tiles wv, 4 + wv, 8 + wv), bf16 into RS
__device__ __forceinline__ void qkv_head(uint16_t* RS, const uint16_t* AS, const uint16_t* wqkv, const float* bqkv,
                                         int wv, int c, int g) {
  f32x4 acc[3][4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < DM / 32; ++ks) {
    bf16x8 bw[3], af[4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      bw[t] = *reinterpret_cast<const bf16x8*>(wqkv + (size_t)(t * DM + DH * wv + c) * DM + 32 * ks + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(AS + (16 * i + c) * AS_LD + 32 * ks + 8 * g);
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] = mfma32(af[i], bw[t], acc[t][i]);
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int col = t * DM + DH * wv + c;
    const float bv = bqkv[col];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) RS[(16 * i + 4 * g + r) * QKV_LD + col] = f32_to_bf16(acc[t][i][r] + bv);
  }
}

// attention of head wv over the 64 tokens (S^T = K Q^T; P V), bf16 output columns 16 wv .. into OS.  sl: the score
// scale times log2(e) - softmax in the exp2 domain, each score one fma + v_exp_f32
__device__ __forceinline__ void attention_head(uint16_t* OS, const uint16_t* RS, float sl, int wv, int c, int g) {
  const uint16_t* Qs = RS + DH * wv;
  const uint16_t* Ks = RS + DM + DH * wv;
  const uint16_t* Vs = RS + 2 * DM + DH * wv;
  f32x4 st[4][4];
  bf16x4 kf[4], qf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kf[i] = *reinterpret_cast<const bf16x4*>(Ks + (16 * i + c) * QKV_LD + 4 * g);
    qf[i] = *reinterpret_cast<const bf16x4*>(Qs + (16 * i + c) * QKV_LD + 4 * g);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) st[i][j] = mfma16(kf[i], qf[j], (f32x4){0.f, 0.f, 0.f, 0.f});
  bf16x4 pf[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float m = -3.402823466e+38f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, st[i][j][r]);
    m = max4g(m) * sl;
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(st[i][j][r], sl, -m));
        st[i][j][r] = e;
        l += e;
      }
    l = sum4g(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int i = 0; i < 4; ++i) pf[j][i] = pack4(st[i][j] * inv);
  }
  bf16x4 vf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint16_t* vp = Vs + (16 * i + 4 * g) * QKV_LD + c;
    vf[i][0] = (short)vp[0]; vf[i][1] = (short)vp[QKV_LD];
    vf[i][2] = (short)vp[2 * QKV_LD]; vf[i][3] = (short)vp[3 * QKV_LD];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = mfma16(pf[j][i], vf[i], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) OS[(16 * j + 4 * g + r) * AS_LD + DH * wv + c] = f32_to_bf16(acc[r]);
  }
}

// h1 = h + o Wo^T + bo, column tile wv of all 64 rows (each wave streams its quarter of the weight)
__device__ __forceinline__ void proj_residual(float* HS, const uint16_t* OS, const uint16_t* wo, const float* bo, int wv,
                                              int c, int g) {
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < DM / 32; ++ks) {
    const bf16x8 bw = *reinterpret_cast<const bf16x8*>(wo + (size_t)(16 * wv + c) * DM + 32 * ks + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i] = mfma32(*reinterpret_cast<const bf16x8*>(OS + (16 * i + c) * AS_LD + 32 * ks + 8 * g), bw, acc[i]);
  }
  const int col = 16 * wv + c;
  const float bv = bo[col];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) HS[(16 * i + 4 * g + r) * HS_LD + col] += acc[i][r] + bv;
}

// F = gelu(a2 W1^T + b1) for columns 64 wv .. 64 wv + 63, bf16 into RS.  Operands swapped (A = W1 rows, B = a2 rows):
// the C tile is [column][token], so a lane holds 4 consecutive columns of one token and stores them as 8 bytes
__device__ __forceinline__ void fc1_gelu(uint16_t* RS, const uint16_t* AS, const uint16_t* w1, const float* b1, int wv,
                                         int c, int g) {
  f32x4 acc[4][4];  // [token tile][column tile of this wave]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < DM / 32; ++ks) {
    bf16x8 af[4], bw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      bw[t] = *reinterpret_cast<const bf16x8*>(w1 + (size_t)(64 * wv + 16 * t + c) * DM + 32 * ks + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(AS + (16 * i + c) * AS_LD + 32 * ks + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][t] = mfma32(bw[t], af[i], acc[i][t]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col0 = 64 * wv + 16 * t + 4 * g;
    const float4 bv = *reinterpret_cast<const float4*>(b1 + col0);
    const float bvs[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t fp[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) fp[r] = f32_to_bf16(gelu_f(acc[i][t][r] + bvs[r]));
      *reinterpret_cast<uint2*>(RS + (16 * i + c) * F_LD + col0) =
          make_uint2(fp[0] | ((uint32_t)fp[1] << 16), fp[2] | ((uint32_t)fp[3] << 16));
    }
  }
}

// out = h1 + F W2^T + b2 for column tile wv.  LAST: the model's last block leaves the column's token mean in PS
// instead of the tile (the training kernel's pool: 16 rows in-lane, then the column's four row groups by shuffles)
template <bool LAST>
__device__ __forceinline__ void fc2_residual(float* HS, float* PS, const uint16_t* RS, const uint16_t* w2,
                                             const float* b2, int wv, int c, int g) {
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < FF / 32; ++ks) {
    const bf16x8 bw = *reinterpret_cast<const bf16x8*>(w2 + (size_t)(16 * wv + c) * FF + 32 * ks + 8 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i] = mfma32(*reinterpret_cast<const bf16x8*>(RS + (16 * i + c) * F_LD + 32 * ks + 8 * g), bw, acc[i]);
  }
  const int col = 16 * wv + c;
  const float bv = b2[col];
  float cs = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* hp = HS + (16 * i + 4 * g + r) * HS_LD + col;
      const float v = *hp + (acc[i][r] + bv);
      if (LAST) cs += v;
      else *hp = v;
    }
  if (LAST) {
    cs += __shfl_xor(cs, 16);
    cs += __shfl_xor(cs, 32);
    if (g == 0) PS[col] = cs * (1.f / T);
  }
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256, 2) void tt_infer_kernel(TtInferArgs a, long long S, int nslots, float sl) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* HS = reinterpret_cast<float*>(smem);
  uint16_t* AS = reinterpret_cast<uint16_t*>(smem + HS_BYTES);
  uint16_t* OS = reinterpret_cast<uint16_t*>(smem + HS_BYTES + AS_BYTES);
  uint16_t* RS = reinterpret_cast<uint16_t*>(smem + HS_BYTES + 2 * AS_BYTES);
  float* XS = reinterpret_cast<float*>(smem + HS_BYTES + 2 * AS_BYTES + R_BYTES);  // the sample's features
  float* PS = XS + DM;                                                              // its token mean
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int C = a.C, L = a.L;
  const bool stats = a.Y != nullptr;

  // ---- once per workgroup.  Wave 0: the head's fp32 parameters, lane = dimension (class slots past C re-read class
  // C - 1 and are masked, as head_chain's).  Wave 1: feature `lane`'s normalisation constants
  float h_lnw = 0.f, h_lnb = 0.f, h_w[CMAX], h_b[CMAX];
#pragma unroll
  for (int k = 0; k < CMAX; ++k) h_w[k] = h_b[k] = 0.f;
  if (wv == 0) {
    h_lnw = a.ln_w[lane];
    h_lnb = a.ln_b[lane];
#pragma unroll
    for (int k = 0; k < CMAX; ++k) {
      const int kc = k < C ? k : C - 1;
      h_w[k] = a.head_w[kc * DM + lane];
      h_b[k] = a.head_b[kc];
    }
  }
  const bool norm = a.norm_mean != nullptr;
  float nm = 0.f, ns = 1.f;
  if (wv == 1 && norm) {
    nm = a.norm_mean[lane];
    ns = a.norm_std[lane];
  }
  // wave 1 loads a sample's feature `lane` one sample ahead of its use
  float xnext = 0.f;
  if (wv == 1 && (int)blockIdx.x < nslots) {
    const long long i = (long long)blockIdx.x * S;
    xnext = a.X[(size_t)(a.idx ? (long long)a.idx[i] : i) * a.ldx + lane];
  }

  for (int s = blockIdx.x; s < nslots; s += gridDim.x) {
    // the slot's accumulators, wave 0: the loss in lane 0, the correct count in every lane, cell k in lane k
    double sl_loss = 0.0;
    long long sl_corr = 0, sl_conf = 0;
    const long long i0 = (long long)s * S;
    const long long i1 = (i0 + S < a.n) ? i0 + S : a.n;
    for (long long i = i0; i < i1; ++i) {
      if (wv == 1) {
        XS[lane] = norm ? (xnext - nm) / ns : xnext;
        long long nx = i + 1;
        if (nx >= i1) nx = ((long long)s + gridDim.x < nslots) ? ((long long)s + gridDim.x) * S : -1;
        if (nx >= 0) xnext = a.X[(size_t)(a.idx ? (long long)a.idx[nx] : nx) * a.ldx + lane];
      }
      int y = -1;  // (used by wave 0 behind the blocks: the load's latency hides under them)
      if (wv == 0 && stats) y = a.Y[a.idx ? (long long)a.idx[i] : i];
      __syncthreads();

      for (int l = 0; l < L; ++l) {
        const uint16_t* wb = a.wimg + (size_t)l * W_STRIDE;
        const float* vb = a.vimg + (size_t)l * V_STRIDE;
        // LN1 (rows of this wave); the first block embeds the features where it reads its input
        if (l == 0) layer_norm_rows<true>(HS, AS, XS, a.E, a.c, vb + V_LN1W, vb + V_LN1B, a.eps);
        else layer_norm_rows<false>(HS, AS, nullptr, nullptr, nullptr, vb + V_LN1W, vb + V_LN1B, a.eps);
        __syncthreads();
        qkv_head(RS, AS, wb + W_QKV, vb + V_BQKV, wv, c, g);
        __syncthreads();
        attention_head(OS, RS, sl, wv, c, g);
        __syncthreads();
        proj_residual(HS, OS, wb + W_O, vb + V_BO, wv, c, g);
        __syncthreads();  // LN2 rows need every wave's columns
        layer_norm_rows<false>(HS, AS, nullptr, nullptr, nullptr, vb + V_LN2W, vb + V_LN2B, a.eps);
        __syncthreads();
        fc1_gelu(RS, AS, wb + W_1, vb + V_B1, wv, c, g);
        __syncthreads();
        if (l == L - 1) fc2_residual<true>(HS, PS, RS, wb + W_2, vb + V_B2, wv, c, g);
        else fc2_residual<false>(HS, PS, RS, wb + W_2, vb + V_B2, wv, c, g);
        __syncthreads();
      }

      // ---- head, wave 0 (the others go on to the next sample's barrier): tt_io.hip head_chain's arithmetic on the
      // token mean, then the outputs and the sample's statistics
      if (wv == 0) {
        const float p = PS[lane];
        const float mean = wsum(p) * (1.f / DM);
        const float dv = p - mean;
        const float rstd = rsqrtf(wsum(dv * dv) * (1.f / DM) + a.eps);
        const float xhat = dv * rstd;
        const float z = xhat * h_lnw + h_lnb;
        float logit[CMAX], ex[CMAX];
#pragma unroll
        for (int k = 0; k < CMAX; ++k) logit[k] = (k < C) ? wsum(z * h_w[k]) + h_b[k] : -3.402823466e+38f;
        float mx = logit[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < CMAX; ++k)
          if (k < C && logit[k] > mx) { mx = logit[k]; am = k; }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < CMAX; ++k) {
          ex[k] = (k < C) ? expf(logit[k] - mx) : 0.f;
          se += ex[k];
        }
        float myz = 0.f, mye = 0.f, zy = 0.f;
#pragma unroll
        for (int k = 0; k < CMAX; ++k) {
          if (k == lane) { myz = logit[k]; mye = ex[k]; }
          if (k == y) zy = logit[k];
        }
        if (lane < C) {
          if (a.logits_out) a.logits_out[(size_t)i * C + lane] = myz;
          if (a.probs_out) a.probs_out[(size_t)i * C + lane] = mye / se;
        }
        if (lane == 0 && a.pred_out) a.pred_out[i] = am;
        if (stats) {
          const bool ok = y >= 0 && y < C;
          const int cell = ok ? y * C + am : -1;
          sl_loss += (double)(mx + logf(se) - zy);
          sl_corr += (ok && y == am) ? 1 : 0;
          sl_conf += (lane == cell) ? 1 : 0;
        }
      }
    }
    if (stats && wv == 0) {
      long long* slot = reinterpret_cast<long long*>(a.ws) + (size_t)s * SLOT_WORDS;
      if (lane == 0) {
        slot[0] = __double_as_longlong(sl_loss);
        slot[1] = sl_corr;
      }
      if (lane < C * C) slot[2 + lane] = sl_conf;
    }
  }
}

// word e of the statistics = sum of word e of the slots: lane l adds slots l, l + 64, ... in ascending order, then the
// 64 lane sums go through one xor tree - a fixed order (mlp_infer.hip's fold)
__global__ __launch_bounds__(FOLD_NT) void tt_infer_fold_kernel(const long long* ws, int nslots, long long* out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e == 0) {
    double v = 0.0;
    for (int s = lane; s < nslots; s += FOLD_NT) v += __longlong_as_double(ws[(size_t)s * SLOT_WORDS]);
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) out[0] = __double_as_longlong(v);
  } else {
    long long v = 0;
    for (int s = lane; s < nslots; s += FOLD_NT) v += ws[(size_t)s * SLOT_WORDS + e];
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) out[e] = v;
  }
}

}  // namespace tti
}  // namespace dct

extern "C" {

int dct_tt_infer_supported(int T, int DM, int H, int FF, int L, int C) {
  using namespace dct::tti;
  return T == dct::tti::T && DM == dct::tti::DM && H == NH && FF == dct::tti::FF && L >= 1 && L <= LMAX && C >= CMIN &&
         C <= CMAX;
}

// bytes of the slot workspace of a launch over n samples with labels: at most 4096 slots, whatever n is
long long dct_tt_infer_ws_bytes(int L, int C, long long n) {
  using namespace dct::tti;
  if (!dct_tt_infer_supported(dct::tti::T, dct::tti::DM, NH, dct::tti::FF, L, C) || n < 1) return 0;
  return (long long)slots_of(n).nslots * SLOT_WORDS * 8;
}

int dct_tt_infer(const dct::TtInferArgs* a, int T, int DM, int H, int FF, int grid, void* stream) {
  using namespace dct::tti;
  if (!dct_tt_infer_supported(T, DM, H, FF, a->L, a->C)) return (int)hipErrorInvalidValue;
  if (a->n < 1 || !a->X || a->ldx < T || grid > MAX_GRID) return (int)hipErrorInvalidValue;
  if (!a->E || !a->c || !a->wimg || !a->vimg || !a->ln_w || !a->ln_b || !a->head_w || !a->head_b)
    return (int)hipErrorInvalidValue;
  // 16-byte vector loads of the embedding and of both images
  if ((reinterpret_cast<uintptr_t>(a->E) | reinterpret_cast<uintptr_t>(a->c) | reinterpret_cast<uintptr_t>(a->wimg) |
       reinterpret_cast<uintptr_t>(a->vimg)) & 15)
    return (int)hipErrorInvalidValue;
  if ((a->norm_mean == nullptr) != (a->norm_std == nullptr)) return (int)hipErrorInvalidValue;
  const Slots sl = slots_of(a->n);
  if (a->Y) {
    if (!a->ws || !a->stats || reinterpret_cast<uintptr_t>(a->ws) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(a->stats) % 8 != 0 || a->ws_bytes < dct_tt_infer_ws_bytes(a->L, a->C, a->n))
      return (int)hipErrorInvalidValue;
  }
  // two workgroups per CU fill the machine; more would only re-read the head's parameters
  static int resident = 0;
  if (!resident) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)tt_infer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    resident = 2 * (cus > 0 ? cus : 1);
  }
  if (grid <= 0) grid = sl.nslots < resident ? sl.nslots : resident;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float scale_log2e = 1.f / sqrtf((float)DH) * 1.4426950408889634f;
  hipLaunchKernelGGL(tt_infer_kernel, dim3(grid), dim3(256), LDS_BYTES, st, *a, sl.S, sl.nslots, scale_log2e);
  if (a->Y)
    hipLaunchKernelGGL(tt_infer_fold_kernel, dim3(2 + a->C * a->C), dim3(FOLD_NT), 0, st,
                       reinterpret_cast<const long long*>(a->ws), sl.nslots, reinterpret_cast<long long*>(a->stats));
  return (int)hipGetLastError();
}

}  // extern "C"
