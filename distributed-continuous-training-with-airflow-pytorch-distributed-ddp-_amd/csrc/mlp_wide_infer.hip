// mlp_wide_infer: fused forward-only bf16 inference for the wide MLPs the graph engine trains (256-1024-1024-1024-2 and
// its kin) - the counterpart of mlp_infer.hip beyond the batch-tiled shapes.  bf16 operands, fp32 accumulation, bf16
// activations between layers: the rounding points of the graph engine's training step.  One launch covers a rank's
// shard and no activation leaves the CU.
//
//   Shapes: 2..4 linear layers, D0 a multiple of 32 in 32..1024, hidden widths multiples of 128 in 128..1024,
//     2..8 classes, ReLU or erf-GELU (dct_common.h gelu_f, the GEMM epilogues' form), no norm, no skip connection.
//   Work split: a workgroup of 8 waves carries a tile of BM = 64 rows through every layer.  The tile's activation
//     image is [64][KM + 8] bf16 in LDS (KM the widest layer input: 129 KB at 1024 - one image is all that fits), so
//     a layer runs IN PLACE: wave w owns output columns w N / 8 .. (w + 1) N / 8 of all 64 rows and keeps that whole
//     slab as fp32 accumulators of v_mfma_f32_16x16x32_bf16 in registers (4 row blocks x N / 128 column blocks x 4 =
//     128 at N = 1024), runs the full K loop against the image, waits at a barrier until every wave has finished
//     reading, then adds the bias, applies the activation, rounds to bf16 and stores its own columns over the image.
//   Operands: the weights are a bf16 copy of the flat parameters in torch's [N][K] order, read straight from
//     global memory (L2) one k-step ahead of their use - a lane's fragment is one 16-byte load of 8 k-contiguous
//     values; the weight fragment is the MFMA's A operand and the image fragment (one ds_read_b128) its B operand,
//     so a lane's 4 results are 4 consecutive columns of one row: one 8-byte LDS store per fragment in the epilogue.
//   Gather: X rows (through idx when bound), optionally (x - mean) / std in fp32, rounded to bf16 once.
//   Head (C <= 8): on the VALU in fp32 from the last image with the bf16-rounded head weights, 8 lanes per row;
//     logits, softmax probabilities, argmax (lowest index on ties), with labels the CE / MSE row loss.
//   Statistics: mlp_infer.hip's contract and scheme - the T = ceil(n / 64) tiles are cut into at most 4096 slots of
//     S consecutive tiles, a workgroup owns whole slots (s, s + G, ...), sums a slot's tiles in ascending order (loss
//     in fp64, counts as int64) and writes it with plain vector stores; a fold launch adds the slots in a fixed order.
//     No atomics: the same bits whatever the grid.  Rows >= n of the last tile are gathered as zeros and write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dct_common.h"
#include "mlp_fused.h"

namespace dct {
namespace wide {

constexpr int BM = 64;    // rows of a tile
constexpr int NT = 512;   // 8 waves
constexpr int PAD = 8;    // bf16 elements behind an image row: the 16-byte reads of 16 rows spread over all banks
constexpr int MAXC = 8;
constexpr int MAX_SLOTS = 4096;
constexpr int SLOT_WORDS = 2 + MAXC * MAXC;  // 8-byte words per slot: loss (fp64), correct, confusion cells
constexpr int FOLD_NT = 64;
constexpr int MAX_GRID = 65536;

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Plan {
  int L, C, lda;
  int dims[MLP_MAXL + 1];
  int woff[MLP_MAXL], boff[MLP_MAXL];  // flat offsets (elements), the same in the fp32 vector and its bf16 copy
};

// the shape rule (head of the file); every woff is a multiple of 8, so every bf16 weight row starts on 16 bytes
static bool make_plan(Plan* tp, const int* dims, int L) {
  if (!dims || L < 2 || L > MLP_MAXL) return false;
  if (dims[0] < 32 || dims[0] > 1024 || dims[0] % 32) return false;
  for (int l = 1; l < L; ++l)
    if (dims[l] < 128 || dims[l] > 1024 || dims[l] % 128) return false;
  if (dims[L] < 2 || dims[L] > MAXC) return false;
  tp->L = L;
  tp->C = dims[L];
  int off = 0, km = 0;
  for (int l = 0; l < L; ++l) {
    tp->dims[l] = dims[l];
    tp->woff[l] = off;
    off += dims[l] * dims[l + 1];
    tp->boff[l] = off;
    off += dims[l + 1];
    if (dims[l] > km) km = dims[l];
  }
  tp->dims[L] = dims[L];
  tp->lda = km + PAD;
  return true;
}

static size_t lds_bytes(const Plan& tp) { return (size_t)BM * tp.lda * 2 + 3 * BM * 4; }  // image, row loss, cell, label

struct Slots {
  long long T, S;
  int nslots;
};
static Slots slots_of(long long n) {
  Slots o;
  o.T = (n + BM - 1) / BM;
  o.S = (o.T + MAX_SLOTS - 1) / MAX_SLOTS;
  o.nslots = (int)((o.T + o.S - 1) / o.S);
  return o;
}

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 ld8(const uint16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

__device__ __forceinline__ float pick8(const float (&v)[MAXC], int i) {
  float o = v[0];
#pragma unroll
  for (int c = 1; c < MAXC; ++c) o = (i == c) ? v[c] : o;
  return o;
}

// One hidden layer in place: img[0..64)[0..K) -> img[0..64)[0..N), N = 128 NB.  A operand: W rows (output columns)
// col0 + 16 cb + (lane & 15), k = k0 + 8 (lane >> 4) + e; B operand: image rows 16 rb + (lane & 15), the same k;
// result: row 16 rb + (lane & 15), columns col0 + 16 cb + 4 (lane >> 4) + r.
template <int NB, int ACT>
__device__ __forceinline__ void layer(uint16_t* img, int lda, const uint16_t* W, const float* bias, int K, int wave,
                                      int lane) {
  const int j = lane & 15, q = lane >> 4;
  const int col0 = wave * (NB * 16);
  f32x4 acc[NB][4];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) acc[cb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* wp = W + (size_t)(col0 + j) * K + 8 * q;
  const uint16_t* ap = img + j * lda + 8 * q;
  bf16x8 wc[NB], wn[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) wc[cb] = ld8(wp + (size_t)cb * 16 * K);
  for (int k0 = 0; k0 < K; k0 += 32) {
    // the next k-step's weights are on their way while this one's MFMAs run (the last step re-reads its own)
    const int kn = (k0 + 32 < K) ? k0 + 32 : k0;
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) wn[cb] = ld8(wp + (size_t)cb * 16 * K + kn);
    bf16x8 af[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) af[rb] = ld8(ap + rb * 16 * lda + k0);
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[cb][rb] = mfma32(wc[cb], af[rb], acc[cb][rb]);
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) wc[cb] = wn[cb];
  }
  __syncthreads();  // every wave has read the image: its columns may be overwritten
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) {
    const int c = col0 + cb * 16 + 4 * q;
    float b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bias[c + r];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      uint32_t h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = acc[cb][rb][r] + b[r];
        h[r] = f32_to_bf16(ACT == MLP_ACT_GELU ? gelu_f(z) : fmaxf(z, 0.f));
      }
      *reinterpret_cast<uint2*>(img + (rb * 16 + j) * lda + c) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
  }
  __syncthreads();
}

// F.cross_entropy(weight = w, label_smoothing = eps) of one row before its normaliser (row_loss4_weighted's formula
// for C <= 8): t[c] = (1 - eps) w[y] [c == y] + (eps / C) w[c], num = sum_c t[c] (lse - z[c])
// (class_w null: all weights 1; read here, by one lane per row, not held in registers across the layers)
__device__ __forceinline__ float weighted_ce(const float (&z)[MAXC], int C, int y, const float* class_w, float eps,
                                             float lse) {
  float w[MAXC], wy = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    w[c] = (class_w && c < C) ? class_w[c] : 1.f;
    if (c == y) wy = w[c];
  }
  const float on = (1.f - eps) * wy, sm = eps / (float)C;
  float num = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) num = fmaf(fmaf(sm, w[c], (c == y) ? on : 0.f), lse - z[c], num);
  return num;
}

template <int ACT>
__global__ __launch_bounds__(NT) void mlp_wide_infer_kernel(Plan tp, MlpWideInferArgs a, long long T, long long S,
                                                             int nslots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int L = tp.L, C = tp.C, lda = tp.lda, D0 = tp.dims[0];
  const bool stats = a.Y != nullptr;
  const bool norm = a.norm_mean != nullptr;
  const bool wloss = a.class_w != nullptr || a.label_smooth != 0.f;
  uint16_t* img = reinterpret_cast<uint16_t*>(smem);
  float* lossr = reinterpret_cast<float*>(smem + (size_t)BM * lda * 2);
  int* cell = reinterpret_cast<int*>(lossr + BM);
  int* lab = cell + BM;

  for (int s = blockIdx.x; s < nslots; s += gridDim.x) {
    // the slot's accumulators, wave 0: the loss in lane 0, the correct count in every lane, cell k in lane k
    double sl_loss = 0.0;
    long long sl_corr = 0, sl_conf = 0;
    const long long t0 = (long long)s * S;
    const long long t1 = (t0 + S < T) ? t0 + S : T;
    for (long long t = t0; t < t1; ++t) {
      const long long row0 = t * BM;
      const int live = (a.n - row0 < BM) ? (int)(a.n - row0) : BM;

      // ---- gather the tile's rows (normalised when asked), rounded to bf16 once, and its labels
      for (int e = tid; e < BM * D0; e += NT) {
        const int r = e / D0, k = e - r * D0;
        float x = 0.f;
        if (r < live) {
          const long long src = a.idx ? (long long)a.idx[row0 + r] : row0 + r;
          x = a.X[(size_t)src * a.ldx + k];
          if (norm) x = (x - a.norm_mean[k]) / a.norm_std[k];
        }
        img[r * lda + k] = f32_to_bf16(x);
      }
      if (stats && tid < BM) {
        int y = -1;
        if (tid < live) y = a.Y[a.idx ? (long long)a.idx[row0 + tid] : row0 + tid];
        lab[tid] = y;
      }
      __syncthreads();

      // ---- the hidden layers, in place (each ends behind a barrier)
      for (int l = 0; l + 1 < L; ++l) {
        const uint16_t* W = a.wb + tp.woff[l];
        const float* b = a.p + tp.boff[l];
        const int K = tp.dims[l];
        switch (tp.dims[l + 1] >> 7) {
          case 1: layer<1, ACT>(img, lda, W, b, K, wave, lane); break;
          case 2: layer<2, ACT>(img, lda, W, b, K, wave, lane); break;
          case 3: layer<3, ACT>(img, lda, W, b, K, wave, lane); break;
          case 4: layer<4, ACT>(img, lda, W, b, K, wave, lane); break;
          case 5: layer<5, ACT>(img, lda, W, b, K, wave, lane); break;
          case 6: layer<6, ACT>(img, lda, W, b, K, wave, lane); break;
          case 7: layer<7, ACT>(img, lda, W, b, K, wave, lane); break;
          default: layer<8, ACT>(img, lda, W, b, K, wave, lane); break;
        }
      }

      // ---- head: 8 lanes of a row split its K / 8 chunks of 8, then all 8 hold the row's logits
      {
        const int r = tid >> 3, part = tid & 7;
        const int K = tp.dims[L - 1];
        const uint16_t* Wl = a.wb + tp.woff[L - 1];
        const float* bl = a.p + tp.boff[L - 1];
        float z[MAXC], ex[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) z[c] = 0.f;
        for (int k = part * 8; k < K; k += 64) {
          const bf16x8 av = ld8(img + r * lda + k);
          float af[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) af[e] = bf16_to_f32((uint16_t)av[e]);
#pragma unroll
          for (int c = 0; c < MAXC; ++c) {
            if (c < C) {
              const bf16x8 wv = ld8(Wl + c * K + k);
#pragma unroll
              for (int e = 0; e < 8; ++e) z[c] = fmaf(af[e], bf16_to_f32((uint16_t)wv[e]), z[c]);
            }
          }
        }
        float mx = -3.402823466e+38f;
        int am = 0;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          z[c] += __shfl_xor(z[c], 1);
          z[c] += __shfl_xor(z[c], 2);
          z[c] += __shfl_xor(z[c], 4);
          if (c < C) {
            z[c] += bl[c];
            if (z[c] > mx) { mx = z[c]; am = c; }
          }
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          ex[c] = (c < C) ? expf(z[c] - mx) : 0.f;
          se += ex[c];
        }
        if (r < live) {
          const size_t g = (size_t)(row0 + r);
          if (part < C) {
            if (a.logits_out) a.logits_out[g * C + part] = pick8(z, part);
            if (a.probs_out) a.probs_out[g * C + part] = pick8(ex, part) / se;
          }
          if (part == 0 && a.pred_out) a.pred_out[g] = am;
        }
        if (stats && part == 0) {
          const int y = lab[r];
          const float lse = mx + logf(se);
          float loss = 0.f;
          if (wloss) {
            // labels outside 0 .. C - 1 carry no weight and add nothing
            loss = (y >= 0 && y < C) ? weighted_ce(z, C, y, a.class_w, a.label_smooth, lse) : 0.f;
          } else if (a.loss_kind == 0) {
            loss = lse - pick8(z, y < 0 ? 0 : y);
            if (y < 0 || y >= C) loss = lse;
          } else {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
              if (c < C) {
                const float d = z[c] - (c == y ? 1.f : 0.f);
                loss += d * d;
              }
            }
            loss /= (float)C;
          }
          const bool ok = r < live && y >= 0 && y < C;
          lossr[r] = (r < live) ? loss : 0.f;
          cell[r] = ok ? y * C + am : -1;
        }
      }
      __syncthreads();  // the image is free for the next gather; the rows' losses and cells are in LDS

      // ---- the tile's statistics, wave 0 (lane = row): the loss in a fixed tree, counts by ballot
      if (stats && wave == 0) {
        const int cl = cell[lane];
        double lv = (double)lossr[lane];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) lv += __shfl_xor(lv, off);
        sl_loss += lv;
        const bool hit = cl >= 0 && (cl / C) == (cl % C);
        sl_corr += __popcll(__ballot(hit));
        for (int k = 0; k < C * C; ++k) {
          const unsigned long long m = __ballot(cl == k);
          if (lane == k) sl_conf += __popcll(m);
        }
      }
    }
    if (stats && wave == 0) {
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
// 64 lane sums go through one xor tree - a fixed order whatever the grid was
__global__ __launch_bounds__(FOLD_NT) void mlp_wide_infer_fold_kernel(const long long* ws, int nslots, long long* out) {
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

template <int ACT>
static hipError_t launch(const Plan& tp, const MlpWideInferArgs& a, const Slots& sl, int grid, hipStream_t st) {
  const size_t bytes = lds_bytes(tp);
  auto fn = mlp_wide_infer_kernel<ACT>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), bytes, st, tp, a, sl.T, sl.S, sl.nslots);
  if (a.Y)
    hipLaunchKernelGGL(mlp_wide_infer_fold_kernel, dim3(2 + tp.C * tp.C), dim3(FOLD_NT), 0, st,
                       reinterpret_cast<const long long*>(a.ws), sl.nslots, reinterpret_cast<long long*>(a.stats));
  return hipGetLastError();
}

}  // namespace wide
}  // namespace dct

extern "C" {

int dct_mlp_wide_infer_supported(const int* dims, int L, int act_kind) {
  dct::wide::Plan tp;
  return dct::wide::make_plan(&tp, dims, L) && (act_kind == dct::MLP_ACT_RELU || act_kind == dct::MLP_ACT_GELU);
}

long long dct_mlp_wide_infer_ws_bytes(const int* dims, int L, long long n) {
  dct::wide::Plan tp;
  if (!dct::wide::make_plan(&tp, dims, L) || n < 1) return 0;
  return (long long)dct::wide::slots_of(n).nslots * dct::wide::SLOT_WORDS * 8;
}

int dct_mlp_wide_infer(const int* dims, int L, const dct::MlpWideInferArgs* a, int grid, void* stream) {
  dct::wide::Plan tp;
  if (!dct_mlp_wide_infer_supported(dims, L, a->act_kind) || !dct::wide::make_plan(&tp, dims, L))
    return (int)hipErrorInvalidValue;
  if (!a->p || !a->wb || reinterpret_cast<uintptr_t>(a->wb) % 16 != 0) return (int)hipErrorInvalidValue;
  if (a->n < 1 || !a->X || a->ldx < tp.dims[0]) return (int)hipErrorInvalidValue;
  if ((a->norm_mean == nullptr) != (a->norm_std == nullptr)) return (int)hipErrorInvalidValue;
  if (a->loss_kind != 0 && a->loss_kind != 1) return (int)hipErrorInvalidValue;
  if (!(a->label_smooth >= 0.f && a->label_smooth < 1.f)) return (int)hipErrorInvalidValue;
  if ((a->class_w || a->label_smooth != 0.f) && a->loss_kind != 0) return (int)hipErrorInvalidValue;  // CE only
  if (grid > dct::wide::MAX_GRID) return (int)hipErrorInvalidValue;
  const dct::wide::Slots sl = dct::wide::slots_of(a->n);
  if (a->Y) {
    if (!a->ws || !a->stats || reinterpret_cast<uintptr_t>(a->ws) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(a->stats) % 8 != 0 || a->ws_bytes < dct_mlp_wide_infer_ws_bytes(dims, L, a->n))
      return (int)hipErrorInvalidValue;
  }
  if (grid <= 0) grid = sl.nslots;  // nothing is staged per workgroup: one per slot balances best
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a->act_kind == dct::MLP_ACT_GELU) return (int)dct::wide::launch<dct::MLP_ACT_GELU>(tp, *a, sl, grid, st);
  return (int)dct::wide::launch<dct::MLP_ACT_RELU>(tp, *a, sl, grid, st);
}

}  // extern "C"
