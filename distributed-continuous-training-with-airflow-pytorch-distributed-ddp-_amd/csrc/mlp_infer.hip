// mlp_infer: batch-tiled forward-only fp32 inference for the weather MLPs - the tile forward of mlp_tile_fwd.h
// (the one mlp_tile.hip's step kernel trains through: same shape rule, staging, layers and head), without dropout,
// with per-row outputs and order-independent statistics.  Here: the once-per-workgroup staging, the normalising
// gather, the tile walk, the outputs, the loss and the statistics.
//
//   infer kernel (grid G): every workgroup stages W0, the head weights and the biases in LDS ONCE and keeps
//     its W1 fragments of the MFMA in registers, then walks tiles of R = 32 rows: gather rows X[idx[..]]
//     (optionally (x - mean) / std, the scoring script's "raw" contract) -> layer 0 on the VALU (D0 <= 32) ->
//     hidden x hidden forward on v_mfma_f32_16x16x4_f32 (exact fp32) -> head (C <= 4) on the VALU ->
//     logits / softmax probabilities / argmax, each written only when its pointer is given.
//   statistics (labels given): loss sum (CE or MSE; with MlpInferArgs::class_w / label_smooth the sum of the
//     weighted, smoothed CE numerators of row_loss4_weighted, whose normaliser W the host takes from the confusion
//     matrix's row sums), correct count, C x C confusion matrix (rows = label,
//     columns = prediction).  The T = ceil(n / 32) tiles are cut into at most 4096 slots of S = ceil(T / 4096)
//     consecutive tiles.  A workgroup owns whole slots (slot s, s + G, ...), accumulates a slot's tiles in
//     ascending order - the loss in fp64, the counts as 64-bit integers - and writes the slot with plain vector
//     stores.  What a slot holds is a function of the inputs and n alone, not of G or of who finished first.
//   fold kernel (grid 2 + C * C, one wave each): word e of the statistics is the sum of word e of the slots:
//     lane l adds slots l, l + 64, ... in ascending order, then the 64 lane sums go through one xor tree - a fixed
//     order, so the fp64 loss sum is bit-identical from run to run and from grid to grid.
//   The kernel boundary is the only synchronisation: no atomics, no workgroup waits on another one.
//
// Shapes: those of dct_mlp_tile_supported (tile::make_plan), parameters on a 16-byte boundary.  LDS: 57.5 KB for
// the 3-layer nets, 40.6 KB for the 2-layer ones.  Rows >= n of the last tile are gathered as zeros and write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_fused_impl.h"
#include "mlp_tile_fwd.h"

namespace dct {
namespace infer {

using namespace tile;  // R, NT, LDH, LDX, Plan and the forward pieces

constexpr int MAX_SLOTS = 4096;
constexpr int SLOT_WORDS = 18;  // 8-byte words per slot: loss (fp64), correct, 16 confusion cells
constexpr int FOLD_NT = 64;
constexpr int MAX_GRID = 65536;

// tiles, tiles per slot and slots of n rows
struct Slots {
  long long T, S;
  int nslots;
};
static Slots slots_of(long long n) {
  Slots o;
  o.T = (n + R - 1) / R;
  o.S = (o.T + MAX_SLOTS - 1) / MAX_SLOTS;
  o.nslots = (int)((o.T + o.S - 1) / o.S);
  return o;
}

// LDS carve (floats)
struct Lds {
  int x0, w0, wl, nrm, a1, a2, lossr, cell, total;
};
__host__ __device__ inline Lds lds_layout(int L) {
  Lds o;
  int off = 0;
  o.x0 = off; off += R * LDX;
  o.w0 = off; off += 128 * LDX;    // W0 [H1][D0], b0 in the pad column 32
  o.wl = off; off += 4 * 128 + 4;  // head weights [C][K] + bias
  o.nrm = off; off += 64;          // mean [32], std [32]
  o.a1 = off; off += R * LDH;
  o.a2 = off; if (L == 3) off += R * LDH;
  o.lossr = off; off += R;
  o.cell = off; off += R;
  o.total = off;
  return o;
}

__device__ __forceinline__ float pick4(const float (&v)[4], int i) {
  return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

// WL: the class-weighted / label-smoothed loss, chosen on the host from the launch arguments - the plain
// instantiation is the kernel as it was
template <int L, bool WL>
__global__ __launch_bounds__(NT) void mlp_infer_kernel(Plan tp, MlpInferArgs a, long long T, long long S, int nslots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Lds lo = lds_layout(L);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 15, q = lane >> 4;
  const int D0 = tp.D0, H1 = tp.H1, H2 = tp.H2, C = tp.C, K = tp.K;
  const bool stats = a.Y != nullptr;
  const bool norm = a.norm_mean != nullptr;
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
  float* nm = lds + lo.nrm;
  float* ns = nm + 32;
  float* A1 = lds + lo.a1;
  float* A2 = lds + lo.a2;
  float* lossr = lds + lo.lossr;
  int* cell = reinterpret_cast<int*>(lds + lo.cell);
  int* lab = cell;  // the gather leaves the label here, the head turns it into the confusion cell

  // ---- once per workgroup: this wave's W1 fragments (column blocks wave, wave + 4) and b1 stay in registers,
  // W0, the head and the normalisation constants in LDS
  float4 wf[2][8];
  float b1v[2] = {0.f, 0.f};
  if (L == 3) {
    load_w1_frags(wf, a.p + tp.woff[1], H1, H2, wave, j, q);
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if ((wave + 4 * c) * 16 < H2) b1v[c] = a.p[tp.boff[1] + (wave + 4 * c) * 16 + j];
  }
  stage_weights(W0s, Wl, a.p, tp, L, tid);
  if (tid < D0) {
    nm[tid] = norm ? a.norm_mean[tid] : 0.f;
    ns[tid] = norm ? a.norm_std[tid] : 1.f;
  }
  __syncthreads();  // the gather below already reads the normalisation constants

  for (int s = blockIdx.x; s < nslots; s += gridDim.x) {
    // the slot's accumulators, wave 0: the loss in lane 0, the correct count in every lane, cell k in lane k
    double sl_loss = 0.0;
    long long sl_corr = 0, sl_conf = 0;
    const long long t0 = (long long)s * S;
    const long long t1 = (t0 + S < T) ? t0 + S : T;
    for (long long t = t0; t < t1; ++t) {
      const long long row0 = t * R;
      const int live = (a.n - row0 < R) ? (int)(a.n - row0) : R;

      // ---- gather the tile's rows (normalised when asked) and labels
      for (int e = tid; e < R * D0; e += NT) {
        const int r = e / D0, k = e - r * D0;
        float x = 0.f;
        if (r < live) {
          const long long src = a.idx ? (long long)a.idx[row0 + r] : row0 + r;
          x = a.X[(size_t)src * a.ldx + k];
          if (norm) x = (x - nm[k]) / ns[k];
        }
        X0[r * LDX + k] = x;
      }
      if (stats && tid < R) {
        int y = -1;
        if (tid < live) y = a.Y[a.idx ? (long long)a.idx[row0 + tid] : row0 + tid];
        lab[tid] = y;
      }
      __syncthreads();

      // ---- layer 0: A1 = relu(X0 W0^T + b0)
      layer0(A1, W0s, X0, D0, H1, tid, NoEpilogue{});
      __syncthreads();

      // ---- layer 1: A2 = relu(A1 W1^T + b1); a wave owns column blocks wave, wave + 4
      if (L == 3) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int cb = wave + 4 * c;
          if (cb * 16 >= H2) break;
          layer1_block(A2, A1, wf[c], cb, b1v[c], H1, j, q, NoEpilogue{});
        }
        __syncthreads();
      }

      // ---- head (all 8 lanes of a row hold its logits) + outputs + row loss
      {
        const int r = tid >> 3, part = tid & 7;
        float z[4], ex[4];
        head_logits(z, (L == 3) ? A2 : A1, Wl, C, K, tid);
        float mx = -3.402823466e+38f;
        int am = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C && z[c] > mx) { mx = z[c]; am = c; }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          ex[c] = (c < C) ? expf(z[c] - mx) : 0.f;
          se += ex[c];
        }
        if (r < live) {
          const size_t g = (size_t)(row0 + r);
          if (part < C) {
            if (a.logits_out) a.logits_out[g * C + part] = pick4(z, part);
            if (a.probs_out) a.probs_out[g * C + part] = pick4(ex, part) / se;
          }
          if (part == 0 && a.pred_out) a.pred_out[g] = am;
        }
        if (stats && part == 0) {
          const int y = lab[r];
          float loss = 0.f;
          if (wloss) {
            // the trainer's row loss (mlp_fused_impl.h): the numerator of the weighted mean; labels outside 0 .. C - 1
            // carry no weight and add nothing
            float dz[4], wy;
            loss = row_loss4_weighted(z, C, y, cw, a.label_smooth, dz, &wy);
            if (y < 0 || y >= C) loss = 0.f;
          } else if (a.loss_kind == 0) {
            float zy = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c == y) zy = z[c];
            loss = mx + logf(se) - zy;
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if (c < C) {
                const float d = z[c] - (c == y ? 1.f : 0.f);
                loss += d * d;
              }
            }
            loss /= (float)C;
          }
          const bool ok = r < live && y >= 0 && y < C;
          lossr[r] = (r < live) ? loss : 0.f;
          cell[r] = ok ? y * C + am : -1;  // (lab[r] is read above, by this thread only)
        }
      }

      // ---- the tile's statistics, wave 0: rows in a fixed tree, counts by ballot
      if (stats) {
        __syncthreads();
        if (wave == 0) {
          const int cl = (lane < R) ? cell[lane] : -1;
          double lv = (lane < R) ? (double)lossr[lane] : 0.0;
          lv += __shfl_xor(lv, 16);
          lv += __shfl_xor(lv, 8);
          lv += __shfl_xor(lv, 4);
          lv += __shfl_xor(lv, 2);
          lv += __shfl_xor(lv, 1);
          sl_loss += lv;  // lane 0's is the sum of rows 0..31
          const bool hit = cl >= 0 && (cl / C) == (cl % C);
          sl_corr += __popcll(__ballot(hit));
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const unsigned long long m = __ballot(cl == k);
            if (lane == k) sl_conf += __popcll(m);
          }
        }
      }
    }
    if (stats && wave == 0) {
      long long* slot = reinterpret_cast<long long*>(a.ws) + (size_t)s * SLOT_WORDS;
      if (lane == 0) {
        slot[0] = __double_as_longlong(sl_loss);
        slot[1] = sl_corr;
      }
      if (lane < 16) slot[2 + lane] = sl_conf;
    }
  }
}

// word e of the statistics = sum of word e of the slots, in a fixed order (see the head of the file)
__global__ __launch_bounds__(FOLD_NT) void mlp_infer_fold_kernel(const long long* ws, int nslots, long long* out) {
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

template <int L, bool WL>
static hipError_t launch(const Plan& tp, const MlpInferArgs& a, const Slots& sl, int grid, hipStream_t st) {
  const size_t bytes = (size_t)lds_layout(L).total * sizeof(float);
  auto fn = mlp_infer_kernel<L, WL>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), bytes, st, tp, a, sl.T, sl.S, sl.nslots);
  if (a.Y)
    hipLaunchKernelGGL(mlp_infer_fold_kernel, dim3(2 + tp.C * tp.C), dim3(FOLD_NT), 0, st,
                       reinterpret_cast<const long long*>(a.ws), sl.nslots, reinterpret_cast<long long*>(a.stats));
  return hipGetLastError();
}

}  // namespace infer
}  // namespace dct

extern "C" {

// bytes of the slot workspace of a launch over n rows with labels: at most 4096 slots, whatever n is
long long dct_mlp_infer_ws_bytes(const int* dims, int L, long long n) {
  dct::tile::Plan tp;
  if (!dct::tile::make_plan(&tp, dims, L) || n < 1) return 0;
  return (long long)dct::infer::slots_of(n).nslots * dct::infer::SLOT_WORDS * 8;
}

int dct_mlp_infer(const int* dims, int L, const dct::MlpInferArgs* a, int grid, void* stream) {
  dct::tile::Plan tp;
  if (!dct::tile::plan_launch(&tp, dims, L, a->p)) return (int)hipErrorInvalidValue;
  if (a->n < 1 || !a->X || a->ldx < tp.D0) return (int)hipErrorInvalidValue;
  if ((a->norm_mean == nullptr) != (a->norm_std == nullptr)) return (int)hipErrorInvalidValue;
  if (a->loss_kind != 0 && a->loss_kind != 1) return (int)hipErrorInvalidValue;
  if (!(a->label_smooth >= 0.f && a->label_smooth < 1.f)) return (int)hipErrorInvalidValue;
  if ((a->class_w || a->label_smooth != 0.f) && a->loss_kind != 0) return (int)hipErrorInvalidValue;  // CE only
  if (grid > dct::infer::MAX_GRID) return (int)hipErrorInvalidValue;
  const dct::infer::Slots sl = dct::infer::slots_of(a->n);
  if (a->Y) {
    if (!a->ws || !a->stats || reinterpret_cast<uintptr_t>(a->ws) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(a->stats) % 8 != 0 || a->ws_bytes < dct_mlp_infer_ws_bytes(dims, L, a->n))
      return (int)hipErrorInvalidValue;
  }
  if (grid <= 0) grid = sl.nslots < 1024 ? sl.nslots : 1024;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a->class_w || a->label_smooth != 0.f)
    return (int)(L == 2 ? dct::infer::launch<2, true>(tp, *a, sl, grid, st)
                        : dct::infer::launch<3, true>(tp, *a, sl, grid, st));
  return (int)(L == 2 ? dct::infer::launch<2, false>(tp, *a, sl, grid, st)
                      : dct::infer::launch<3, false>(tp, *a, sl, grid, st));
}

}  // extern "C"
