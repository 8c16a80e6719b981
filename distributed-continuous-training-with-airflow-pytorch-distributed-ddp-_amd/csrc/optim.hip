// Fused flat-buffer Adam for MI355X.
//
// Replaces torch.optim.Adam's per-parameter loop (reference train_lightning_ddp.py:88,
// torch 2.1 single-tensor implementation on CPU). All parameters of a model live in ONE
// flat fp32 buffer (the DDP gradient buckets are views of the matching flat grad buffer),
// so one launch updates every parameter: float4 loads, grid sized to the chip
// (<= 2048 workgroups, grid-stride), bias correction folded into two scalars.
// Optional outputs: a bf16 shadow copy of the updated weights for the MFMA GEMM path, and
// gradient pre-scaling (e.g. 1/world_size when the all-reduce summed).
// Gradient clipping: a norm kernel leaves {norm, coef} on the device and the Adam launch behind it
// reads the coefficient (or clamps by value); the gradient buffer is not rewritten.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "adam_impl.h"
#include "dct_common.h"
#include "kernels.h"

namespace dct {

// out = in * scale (+ optional bf16 cast) - used to average summed gradients and to refresh
// bf16 weight shadows after a checkpoint load.
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* in, uint16_t* out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = f32_to_bf16(in[i]);
}

// Global L2 norm of the flat gradient and the clip coefficient, on the device (gradient clipping by norm,
// torch.nn.utils.clip_grad_norm_): stats = {|grad_scale| sqrt(sum g_i^2), min(max_norm / (norm + 1e-6), 1)}.
// The Adam launch that follows reads stats[1] (AdamArgs::clip_coef), so a captured step replays with no host round trip.
// One launch, <= CLIP_MAX_GRID workgroups (a function of n alone), every sum in a fixed order - no float atomics into
// an accumulator, the same bits on every launch and on every rank that holds the same gradient:
//   thread   four accumulators (one per float4 component) over its grid-stride float4s, (x + y) + (z + w), then
//            the n % 4 tail (workgroup 0, threads 0 .. 2, one element each)
//   wave     xor butterfly 32 .. 1 (wave_sum)
//   group    the four wave sums through LDS, in wave order
//   grid     one partial per workgroup; the last workgroup to arrive (agent-scope ticket, reset to 0 for the next
//            launch or replay; nothing waits) sums them: lane l takes partials l, l + 64, .., then the butterfly.
//            Partial and ticket are memory-side atomics ordered by s_waitcnt, and the partials are read by atomics
//            too (as the head loss of tt_io.hip): no agent-scope fences.
constexpr int CLIP_BLOCK = 256;     // threads of a workgroup (tests/clip_cases.py counts the additions from these)
constexpr int CLIP_MAX_GRID = 256;  // workgroups: one per compute unit pulling on HBM; 3.4 M gradients are 13 passes

struct ClipArgs {
  const float* g;
  int64_t n;
  float grad_scale, max_norm;
  float* partial;    // [CLIP_MAX_GRID]
  unsigned* ticket;  // 0 between launches
  float* stats;      // {norm, coef}
};

__global__ __launch_bounds__(CLIP_BLOCK) void grad_clip_coef_kernel(ClipArgs a) {
  __shared__ float wsums[CLIP_BLOCK / 64];
  __shared__ unsigned last;
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * CLIP_BLOCK;
  const float4* g4 = reinterpret_cast<const float4*>(a.g);
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x; i < n4; i += stride) {
    const float4 g = g4[i];
    sx += g.x * g.x;
    sy += g.y * g.y;
    sz += g.z * g.z;
    sw += g.w * g.w;
  }
  float s = (sx + sy) + (sz + sw);
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < a.n - (n4 << 2)) {
    const float t = a.g[(n4 << 2) + threadIdx.x];
    s += t * t;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsums[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = wsums[0];
#pragma unroll
    for (int w = 1; w < CLIP_BLOCK / 64; ++w) v += wsums[w];
    atomicExch(a.partial + blockIdx.x, v);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (last && threadIdx.x < 64) {
    float t = 0.f;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 64) t += atomicAdd(a.partial + i, 0.f);
    t = wave_sum(t);
    if (threadIdx.x == 0) {
      const float norm = fabsf(a.grad_scale) * sqrtf(t);
      const float c = a.max_norm / (norm + 1e-6f);
      a.stats[0] = norm;
      a.stats[1] = c > 1.0f ? 1.0f : c;  // (a NaN stays a NaN, as torch.clamp(max=1))
      __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Flat SGD (torch.optim.SGD, maximize=False: sgd_elem) for the DDP step path of a model whose optimizer is SGD:
// adam_flat_range's float4 grid-stride body, tail, step epilogue and late read of the device scalars, over p, g and the
// momentum buffer m only (m unread and may be null when mu == 0).  The device counter already includes the step being
// applied (as flat Adam's): counter - 1 steps were taken before it, which indexes the rate table, and the first step
// (the buffer becomes the gradient, whatever m held) is counter == 1.
struct SgdArgs {
  float* p;
  const float* g;
  float* m;
  int64_t n;
  float lr, mu, damp, wd, grad_scale;
  int nesterov;
  int first;                // host step count t == 1; replaced by the device counter's when one is set
  const int* step_counter;  // optional: t read on device (graph-replayable launches)
  int* cursor;              // optional step epilogue, as AdamArgs
  const float* loss_slot;
  float* loss_out;
  int loss_cap;
  const float* lr_tab;  // optional rate table (lr_table.h), with step_counter
};

__device__ __forceinline__ void sgd_device_scalars(SgdArgs& a) {
  const int ti = __hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.lr = lr_for(a.lr_tab, a.lr, ti - 1);
  a.first = ti == 1;
}

__device__ __forceinline__ void sgd_one(float& p, float g, float& m, const SgdArgs& a) {
  sgd_elem(p, g * a.grad_scale, m, a.lr, a.mu, a.damp, a.wd, a.nesterov != 0, a.first != 0);
}

__global__ __launch_bounds__(256) void sgd_flat_kernel(SgdArgs a) {
  if (a.cursor && blockIdx.x == 0 && threadIdx.x == 0) {
    const int c = a.cursor[0];
    if (a.loss_out && c >= 0 && c < a.loss_cap) a.loss_out[c] = a.loss_slot[0];
    a.cursor[0] = c + 1;
  }
  bool pending = a.step_counter != nullptr;  // read after the first element's loads are issued (adam_flat_range)
  const bool mom = a.mu != 0.f;              // (uniform: a kernel argument)
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(a.p);
  const float4* g4 = reinterpret_cast<const float4*>(a.g);
  float4* m4 = reinterpret_cast<float4*>(a.m);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 p = p4[i];
    const float4 g = g4[i];
    float4 m = mom ? m4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (pending) {
      sgd_device_scalars(a);
      pending = false;
    }
    sgd_one(p.x, g.x, m.x, a);
    sgd_one(p.y, g.y, m.y, a);
    sgd_one(p.z, g.z, m.z, a);
    sgd_one(p.w, g.w, m.w, a);
    p4[i] = p;
    if (mom) m4[i] = m;
  }
  // tail (n % 4)
  const int64_t tail0 = n4 << 2;
  const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gt < a.n - tail0) {
    if (pending) sgd_device_scalars(a);
    const int64_t i = tail0 + gt;
    float p = a.p[i], m = mom ? a.m[i] : 0.f;
    sgd_one(p, a.g[i], m, a);
    a.p[i] = p;
    if (mom) a.m[i] = m;
  }
}

}  // namespace dct

static inline int grid_for(int64_t work, int block) {
  int64_t g = (work + block - 1) / block;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// AdamArgs of a flat step at host step count t (dct_adam_flat_step and its clipped form)
static dct::AdamArgs flat_step_args(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                                    float b1, float b2, float eps, float wd, int64_t t, float grad_scale,
                                    int decoupled, const int* step_counter, int* cursor, const float* loss_slot,
                                    float* loss_out, int loss_cap) {
  dct::AdamArgs a{};
  a.p = p; a.g = g; a.m = m; a.v = v; a.p_bf16 = p_bf16; a.n = n;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
  const double bc1 = 1.0 - __builtin_pow((double)b1, (double)t);
  const double bc2 = 1.0 - __builtin_pow((double)b2, (double)t);
  a.step_size = (float)(lr / bc1);
  a.rbc2 = (float)(1.0 / __builtin_sqrt(bc2));
  a.grad_scale = grad_scale;
  a.decoupled = decoupled;
  a.step_counter = step_counter;
  a.cursor = cursor;
  a.loss_slot = loss_slot;
  a.loss_out = loss_out;
  a.loss_cap = loss_cap;
  return a;
}

extern "C" {

int dct_adam_flat_step(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                       float b1, float b2, float eps, float wd, int64_t t, float grad_scale, int decoupled,
                       const int* step_counter, int* cursor, const float* loss_slot, float* loss_out, int loss_cap,
                       void* stream) {
  return dct_adam_flat_step_lr(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, t, grad_scale, decoupled, step_counter,
                               cursor, loss_slot, loss_out, loss_cap, nullptr, 0.f, nullptr, stream);
}

int dct_grad_clip_workspace_floats(void) { return dct::CLIP_MAX_GRID; }

int dct_grad_clip_coef(const float* g, int64_t n, float grad_scale, float max_norm, float* partial, unsigned* ticket,
                       float* stats, void* stream) {
  if (n <= 0 || !g || !partial || !ticket || !stats || !(max_norm >= 0.f) || ((uintptr_t)g & 15))
    return (int)hipErrorInvalidValue;
  dct::ClipArgs a{};
  a.g = g; a.n = n; a.grad_scale = grad_scale; a.max_norm = max_norm;
  a.partial = partial; a.ticket = ticket; a.stats = stats;
  int64_t grid = ((n >> 2) + dct::CLIP_BLOCK - 1) / dct::CLIP_BLOCK;
  grid = std::min<int64_t>(std::max<int64_t>(grid, 1), dct::CLIP_MAX_GRID);
  hipLaunchKernelGGL(dct::grad_clip_coef_kernel, dim3((unsigned)grid), dim3(dct::CLIP_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

int dct_adam_flat_step_clipped(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                               float b1, float b2, float eps, float wd, int64_t t, float grad_scale, int decoupled,
                               const int* step_counter, int* cursor, const float* loss_slot, float* loss_out,
                               int loss_cap, const float* clip_coef, float clip_value, void* stream) {
  return dct_adam_flat_step_lr(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, t, grad_scale, decoupled, step_counter,
                               cursor, loss_slot, loss_out, loss_cap, clip_coef, clip_value, nullptr, stream);
}

// a rate table is read at the device step count, and its header as one aligned 8-byte word
static bool lr_tab_ok(const float* lr_tab, const int* step_counter) {
  return !lr_tab || (step_counter && !((uintptr_t)lr_tab & 15));
}

int dct_adam_flat_step_lr(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr, float b1,
                          float b2, float eps, float wd, int64_t t, float grad_scale, int decoupled,
                          const int* step_counter, int* cursor, const float* loss_slot, float* loss_out, int loss_cap,
                          const float* clip_coef, float clip_value, const float* lr_tab, void* stream) {
  if (!(clip_value >= 0.f) || !lr_tab_ok(lr_tab, step_counter)) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (cursor && !loss_slot) return (int)hipErrorInvalidValue;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return (int)hipErrorInvalidValue;
  dct::AdamArgs a = flat_step_args(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, t, grad_scale, decoupled, step_counter,
                                   cursor, loss_slot, loss_out, loss_cap);
  a.clip_coef = clip_coef;
  a.clip_value = clip_value;
  a.lr_tab = lr_tab;
  const dim3 grid(grid_for((n + 3) / 4, 256));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!clip_coef && clip_value == 0.f)  // no clipping: the unclipped kernel
    hipLaunchKernelGGL(dct::adam_flat_kernel<false>, grid, dim3(256), 0, st, a);
  else if (clip_value > 0.f) hipLaunchKernelGGL(dct::adam_flat_clip_kernel<2>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(dct::adam_flat_clip_kernel<1>, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int dct_sgd_flat_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float dampening,
                      int nesterov, float wd, int64_t t, float grad_scale, const int* step_counter, int* cursor,
                      const float* loss_slot, float* loss_out, int loss_cap, const float* lr_tab, void* stream) {
  if (!(momentum >= 0.f) || !(wd >= 0.f) || (nesterov && (momentum <= 0.f || dampening != 0.f)) ||
      !lr_tab_ok(lr_tab, step_counter))
    return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (cursor && !loss_slot) return (int)hipErrorInvalidValue;
  if (!p || !g || (momentum != 0.f && !m)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) return (int)hipErrorInvalidValue;
  dct::SgdArgs a{};
  a.p = p; a.g = g; a.m = m; a.n = n;
  a.lr = lr; a.mu = momentum; a.damp = dampening; a.wd = wd; a.grad_scale = grad_scale;
  a.nesterov = nesterov ? 1 : 0;
  a.first = t <= 1;
  a.step_counter = step_counter;
  a.cursor = cursor;
  a.loss_slot = loss_slot;
  a.loss_out = loss_out;
  a.loss_cap = loss_cap;
  a.lr_tab = lr_tab;
  hipLaunchKernelGGL(dct::sgd_flat_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

int dct_adam_flat_step_parts(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                             float b1, float b2, float eps, float wd, float grad_scale, int decoupled,
                             const int* step_counter, int* cursor, const float* loss_slot, float* loss_out,
                             int loss_cap, int nparts, const int64_t* part_off, const int64_t* part_n,
                             const float* const* part, const int* part_splits, void* stream) {
  return dct_adam_flat_step_parts_lr(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, grad_scale, decoupled, step_counter,
                                     cursor, loss_slot, loss_out, loss_cap, nparts, part_off, part_n, part, part_splits,
                                     nullptr, stream);
}

int dct_adam_flat_step_parts_lr(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                                float b1, float b2, float eps, float wd, float grad_scale, int decoupled,
                                const int* step_counter, int* cursor, const float* loss_slot, float* loss_out,
                                int loss_cap, int nparts, const int64_t* part_off, const int64_t* part_n,
                                const float* const* part, const int* part_splits, const float* lr_tab, void* stream) {
  if (n <= 0) return 0;
  if (!step_counter || (cursor && !loss_slot) || nparts < 0 || nparts > 3 || !lr_tab_ok(lr_tab, step_counter))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return (int)hipErrorInvalidValue;
  dct::AdamArgs a{};
  a.p = p; a.g = g; a.m = m; a.v = v; a.p_bf16 = p_bf16; a.n = n;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
  a.grad_scale = grad_scale;
  a.decoupled = decoupled;
  a.step_counter = step_counter;
  a.lr_tab = lr_tab;
  a.cursor = cursor;
  a.loss_slot = loss_slot;
  a.loss_out = loss_out;
  a.loss_cap = loss_cap;
  a.nparts = nparts;
  int max_sp = 1;
  for (int r = 0; r < nparts; ++r) {
    if ((part_off[r] | part_n[r]) & 3 || part_off[r] + part_n[r] > (n & ~3LL) || ((uintptr_t)part[r] & 15) ||
        part_splits[r] < 1 || part_splits[r] > 8)
      return (int)hipErrorInvalidValue;
    a.part_off[r] = part_off[r]; a.part_n[r] = part_n[r]; a.part[r] = part[r]; a.part_splits[r] = part_splits[r];
    max_sp = std::max(max_sp, part_splits[r]);
  }
  const dim3 grid(grid_for((n + 3) / 4, 256));
  if (max_sp > 4)
    hipLaunchKernelGGL((dct::adam_flat_kernel<true, 8>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL((dct::adam_flat_kernel<true, 4>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

int dct_adam_range(const dct::AdamRange* r, int* cursor, const float* loss_slot, float* loss_out, int loss_cap,
                   void* stream) {
  dct::AdamArgs a{};
  int max_sp = 1;
  const int e = dct::adam_args_from_range(*r, a, &max_sp);
  if (e) return e;
  if (cursor && !loss_slot) return (int)hipErrorInvalidValue;
  a.cursor = cursor;
  a.loss_slot = loss_slot;
  a.loss_out = loss_out;
  a.loss_cap = loss_cap;
  const dim3 grid(grid_for((r->hi - r->lo + 3) / 4, 256));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (max_sp > 4) hipLaunchKernelGGL((dct::adam_range_kernel<8>), grid, dim3(256), 0, st, a, r->lo, r->hi);
  else hipLaunchKernelGGL((dct::adam_range_kernel<4>), grid, dim3(256), 0, st, a, r->lo, r->hi);
  return (int)hipGetLastError();
}

int dct_adam_flat(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, float lr,
                  float b1, float b2, float eps, float wd, int64_t t, float grad_scale, int decoupled,
                  const int* step_counter, void* stream) {
  return dct_adam_flat_step(p, g, m, v, p_bf16, n, lr, b1, b2, eps, wd, t, grad_scale, decoupled, step_counter,
                            nullptr, nullptr, nullptr, 0, stream);
}

int dct_f32_to_bf16(const float* in, uint16_t* out, int64_t n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(dct::f32_to_bf16_kernel, dim3(grid_for(n, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), in, out, n);
  return (int)hipGetLastError();
}

}  // extern "C"
