// Exponential moving average of the parameters, kept on the device: what
// torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)).update_parameters(model)
// does after every optimizer.step() (use_buffers=False), on the one flat fp32 parameter array.
// Contract: include/fall3.h (f3_ema_update).
//
// The count and the decay live in a 16-byte device block that the kernels read when they run, so an
// update recorded into a HIP graph advances the count and follows a later f3_ema_set_decay on replay
// (the idea of optim.hip's hyper block). The lerp is evaluated in fp64 and rounded to fp32 once, the
// convention of optim.hip: e + (1-d)(p - e) cancels, and the kernel is memory bound (2 loads, 1 store
// per element), so the fp64 VALU work is free.
#include <cmath>

#include "common.h"
#include "fall3.h"

namespace f3 {

struct EmaState {
  long long n_averaged;  // byte 0: updates so far
  double decay;          // byte 8
};
static_assert(sizeof(EmaState) == 16, "the EMA block is 16 bytes (include/fall3.h)");

// One element. contract(off): the vector body and the scalar tail round identically, and the three fp64
// operations are the ones a numpy fp64 evaluation of the same expression performs.
F3_DEV float ema_lerp(float e, float p, double omd) {
#pragma clang fp contract(off)
  const double ed = (double)e;
  return (float)(ed + omd * ((double)p - ed));
}

// float4 body + scalar tail over n floats, grid-stride (as optim_kernel). Every thread reads the block;
// no thread writes it: the count is advanced by ema_count_kernel, after this kernel on the stream.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p,
                                                         long long n, const EmaState* __restrict__ st) {
#pragma clang fp contract(off)
  const bool first = st->n_averaged == 0;
  const double omd = 1.0 - st->decay;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    if (!first) {
      const f32x4 ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) pv[e] = ema_lerp(ev[e], pv[e], omd);
    }
    reinterpret_cast<f32x4*>(ema)[i] = pv;
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) {
    float v = p[i];
    if (!first) v = ema_lerp(ema[i], v, omd);
    ema[i] = v;
  }
}

// one thread, after every element has been written: n_averaged += 1
__global__ void ema_count_kernel(EmaState* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->n_averaged = st->n_averaged + 1;
}

// one thread: the decay into the block (f3_ema_set_decay), launched eagerly on the caller's stream
__global__ void ema_decay_write_kernel(EmaState* __restrict__ st, double decay) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->decay = decay;
}

}  // namespace f3

using namespace f3;

extern "C" {

int64_t f3_ema_state_bytes(void) { return (int64_t)sizeof(EmaState); }

int f3_ema_set_decay(void* state, double decay, void* stream) {
  if (!state || (uintptr_t)state % 8) return F3_EINVAL;
  if (!std::isfinite(decay) || decay < 0.0 || decay > 1.0) return F3_EINVAL;
  hipLaunchKernelGGL(ema_decay_write_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     static_cast<EmaState*>(state), decay);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int f3_ema_update(float* ema, const float* params, int64_t n, void* state, void* stream) {
  if (!ema || !params || !state || n < 0) return F3_EINVAL;
  if (((uintptr_t)ema | (uintptr_t)params) % 16 || (uintptr_t)state % 8) return F3_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  EmaState* st = static_cast<EmaState*>(state);
  if (n > 0) {
    const long long blocks = (n / 4 + 255) / 256;
    const int grid = (int)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096);  // optim_kernel's cap
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, s, ema, params, (long long)n,
                       static_cast<const EmaState*>(st));
    F3_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ema_count_kernel, dim3(1), dim3(64), 0, s, st);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

}  // extern "C"
