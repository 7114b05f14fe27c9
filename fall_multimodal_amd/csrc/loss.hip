// The two settings of the reference's driver that the fused step lacked:
//   TRAIN.LABEL_SMOOTHING  torch.nn.CrossEntropyLoss(label_smoothing=eps)   Multimodal_Fall3/model/main.py:280,
//                          the one loss_fn of train() / valid() / test()    main.py:113, 175, 226
//   TRAIN.ACCUM_ITER       loss.backward() into .grad that optimizer.step() / model.zero_grad() consume
//                          only every ACCUM_ITER-th batch                   main.py:115-132
// and the one CrossEntropyLoss argument a user sets beside them for an imbalanced label set:
//   weight=w               per-class weights, f3_soft_ce_w
// Formulas and contracts: include/fall3.h (f3_soft_ce_ex, f3_soft_ce_w, f3_grad_accumulate). Nothing here allocates,
// syncs or uses a float atomic: every word has one writer per launch and every sum a fixed order, so
// the same inputs give the same bits and every call can be captured into a HIP graph.
#include <cmath>

#include "common.h"
#include "fall3.h"

namespace f3 {

constexpr int kSceOneBlock = 4096;  // batches up to this size: the single-workgroup form (ce_kernel's bound)
constexpr int kSceRegs = 16;        // class counts up to this: the row is loaded into registers up front
constexpr int kSceMaxC = 64;
constexpr int kSceMaxBlocks = 1024; // workgroups of the large-batch form (grid-stride over the rows beyond)

// The per-workgroup partial sums of the large-batch form. Library-owned so that the entry needs no
// scratch argument; launches on one stream are serial, callers on two streams must not overlap there.
__device__ float g_sce_partials[kSceMaxBlocks];

struct SoftCeArgs {
  const float* out;
  const float* label;          // soft targets [N,C], or
  const long long* label_idx;  // class indices [N] (one-hot rows; an index outside [0,C) is a row of zeros)
  float* loss;
  float* dout;                 // may be null: loss only
  int N, C;
  float keep, share;           // 1 - eps, eps / C:  y' = y * keep + share
};

// One row: returns -(sum_c y'_c log_softmax(o)_c) and stores dout's row. With y' in the place of y this is
// ce_kernel's row (head.hip) statement for statement, the same sequential sums in the same order, so at
// eps = 0 (y * 1 + 0 is exact) it gives ce_kernel's bits. That needs the same roundings too, so they are
// written out here and fp contraction is off for the whole row: y' is one fmaf, each loss product is fused
// into the row sum (l = fmaf(-y', o - lse, l)) and dout's product into its difference, which is what
// ce_kernel compiles to; left to the compiler, the register path packed the loss products in pairs and
// added them rounded, and the loss then differed from ce_kernel's in its last bit on some batches.
// CN > 0: the register path, compiled for exactly CN = a.C classes (a run-time bound keeps sixteen lane
// masks alive across the row loop and spills scalar registers); CN = 0: the row is read from memory, any a.C.
// WT (f3_soft_ce_w): a = y' * w, rounded on its own after y', stands in the place of y', m = sum_c a_c in
// the place of sum_c y'_c and D (N, or W rounded to fp32) in the place of N; a row whose index lies outside
// [0, C) is torch's ignore_index row: it adds nothing to the loss and stores 0 / D (zeros, or torch's NaN
// when W == 0), selected at the end, not branched round. Without WT such a row is a row of zeros and D is N.
template <int CN, bool WT>
F3_DEV float soft_ce_row(const SoftCeArgs& a, const float* w, float D, int n) {
#pragma clang fp contract(off)
  const int C = CN ? CN : a.C;
  const float* o = a.out + (size_t)n * C;
  const float* y = a.label ? a.label + (size_t)n * C : nullptr;
  float* d = a.dout ? a.dout + (size_t)n * C : nullptr;
  int t = -1;  // the index label's class; -1: a soft label, or an index outside [0, C)
  if (!y) {
    const long long ti = a.label_idx[n];
    t = ti >= 0 && ti < C ? (int)ti : -1;
  }
  const bool dead = WT && !y && t < 0;
  float l = 0.f;
  if constexpr (CN > 0) {
    // every load issued before the first use
    float ov[CN], yv[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      ov[c] = o[c];
      yv[c] = y ? y[c] : (c == t ? 1.f : 0.f);
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) yv[c] = fmaf(yv[c], a.keep, a.share);
    if constexpr (WT) {
#pragma unroll
      for (int c = 0; c < CN; ++c) yv[c] = yv[c] * w[c];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < CN; ++c) mx = fmaxf(mx, ov[c]);
    float s = 0.f, ys = 0.f;
#pragma unroll
    for (int c = 0; c < CN; ++c) { s += expf(ov[c] - mx); ys += yv[c]; }
    const float lse = mx + logf(s);
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      l = fmaf(-yv[c], ov[c] - lse, l);
      if (d) d[c] = (dead ? 0.f : fmaf(expf(ov[c] - lse), ys, -yv[c])) / D;
    }
  } else {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, o[c]);
    float s = 0.f, ys = 0.f;
    for (int c = 0; c < C; ++c) {
      float yc = fmaf(y ? y[c] : (c == t ? 1.f : 0.f), a.keep, a.share);
      if constexpr (WT) yc = yc * w[c];
      s += expf(o[c] - mx);
      ys += yc;
    }
    const float lse = mx + logf(s);
    for (int c = 0; c < C; ++c) {
      float yc = fmaf(y ? y[c] : (c == t ? 1.f : 0.f), a.keep, a.share);
      if constexpr (WT) yc = yc * w[c];
      l = fmaf(-yc, o[c] - lse, l);
      if (d) d[c] = (dead ? 0.f : fmaf(expf(o[c] - lse), ys, -yc)) / D;
    }
  }
  return dead ? 0.f : l;
}

// the workgroup's sum of its threads' values in ce_kernel<true>'s order: xor-shuffles inside each
// wave, then the four wave sums left to right (valid in thread 0)
F3_DEV float sce_block_sum(float v, float* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ONE: a single 256-thread workgroup walks every row (thread t takes rows t, t + 256, ...) and stores the
// mean: no zeroed loss word beforehand. Otherwise gridDim.x <= kSceMaxBlocks workgroups stride over the
// rows and each stores one partial; soft_ce_finish_kernel adds them.
template <int CN, bool ONE>
__global__ __launch_bounds__(256) void soft_ce_kernel(SoftCeArgs a) {
  __shared__ float red[4];
  float lsum = 0.f;
  const int stride = ONE ? 256 : (int)gridDim.x * 256;
  for (long long n = (ONE ? 0 : (long long)blockIdx.x * 256) + threadIdx.x; n < a.N; n += stride)
    lsum += soft_ce_row<CN, false>(a, nullptr, (float)a.N, (int)n);
  const float sum = sce_block_sum(lsum, red);
  if (threadIdx.x == 0) {
    if (ONE) *a.loss = sum / (float)a.N;
    else g_sce_partials[blockIdx.x] = sum;
  }
}

// one workgroup: the partials through LDS (coalesced loads), added by thread 0 in index order
__global__ __launch_bounds__(256) void soft_ce_finish_kernel(float* __restrict__ loss, int nblk, int N) {
  __shared__ float part[kSceMaxBlocks];
  for (int i = threadIdx.x; i < nblk; i += 256) part[i] = g_sce_partials[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int i = 0; i < nblk; ++i) sum += part[i];
    *loss = sum / (float)N;
  }
}

// ---- class weights: torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps) -------------------------
// Both of torch's rules (include/fall3.h, f3_soft_ce_w): soft labels divide by N, index labels by
// W = sum of w[t_n] over the rows whose index lies in [0, C); every other row is torch's ignore_index row.

// fp64 partial sums of W in the large-batch form (library-owned, as g_sce_partials)
__device__ double g_sce_wpartials[kSceMaxBlocks];

struct SoftCeWArgs {
  SoftCeArgs b;
  const float* w;  // class weights [C], read when the launch runs
  int nwblk;       // large-batch index rule: the number of g_sce_wpartials the launch before stored
};

// w[t_n] of a live row, 0 of an ignored one
F3_DEV double sce_live_weight(const SoftCeWArgs& a, long long n) {
  const long long t = a.b.label_idx[n];
  return t >= 0 && t < a.b.C ? (double)a.w[t] : 0.0;
}

// the workgroup's fp64 sum in sce_block_sum's order, valid in every thread
F3_DEV double sce_block_sum_d(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// W of the large-batch form from the stored partials: thread t adds partials t, t + 256, ... and the
// workgroup sums those: the same order, so the same bits, in every workgroup and in the finish launch
F3_DEV double sce_w_from_partials(int nwblk, double* red) {
  double w = 0.0;
  for (int i = threadIdx.x; i < nwblk; i += 256) w += g_sce_wpartials[i];
  return sce_block_sum_d(w, red);
}

// the large-batch index rule's first launch: workgroup b stores the fp64 sum of the live weights of
// its rows (the rows soft_ce_w_kernel<CN, false> gives it) into g_sce_wpartials[b]
__global__ __launch_bounds__(256) void soft_ce_w_sum_kernel(SoftCeWArgs a) {
  __shared__ double dred[4];
  double w = 0.0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < a.b.N; n += stride) w += sce_live_weight(a, n);
  const double sum = sce_block_sum_d(w, dred);
  if (threadIdx.x == 0) g_sce_wpartials[blockIdx.x] = sum;
}

// soft_ce_kernel with the divisor found first: N for soft labels; for index labels W, summed in fp64 in
// a fixed order (ONE: a pre-pass over the labels; otherwise from the partials of the launch before) and
// rounded to fp32 once
template <int CN, bool ONE>
__global__ __launch_bounds__(256) void soft_ce_w_kernel(SoftCeWArgs a) {
  __shared__ float red[4];
  __shared__ double dred[4];
  float D = (float)a.b.N;
  if (a.b.label_idx) {
    if (ONE) {
      double w = 0.0;
      for (int n = threadIdx.x; n < a.b.N; n += 256) w += sce_live_weight(a, n);
      D = (float)sce_block_sum_d(w, dred);
    } else {
      D = (float)sce_w_from_partials(a.nwblk, dred);
    }
  }
  float lsum = 0.f;
  const int stride = ONE ? 256 : (int)gridDim.x * 256;
  for (long long n = (ONE ? 0 : (long long)blockIdx.x * 256) + threadIdx.x; n < a.b.N; n += stride)
    lsum += soft_ce_row<CN, true>(a.b, a.w, D, (int)n);
  const float sum = sce_block_sum(lsum, red);
  if (threadIdx.x == 0) {
    if (ONE) *a.b.loss = sum / D;
    else g_sce_partials[blockIdx.x] = sum;
  }
}

// soft_ce_finish_kernel dividing by N (nwblk == 0) or by W from the same partials in the same order
__global__ __launch_bounds__(256) void soft_ce_w_finish_kernel(float* __restrict__ loss, int nblk, int N, int nwblk) {
  __shared__ float part[kSceMaxBlocks];
  __shared__ double dred[4];
  float D = (float)N;
  if (nwblk > 0) D = (float)sce_w_from_partials(nwblk, dred);
  for (int i = threadIdx.x; i < nblk; i += 256) part[i] = g_sce_partials[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int i = 0; i < nblk; ++i) sum += part[i];
    *loss = sum / D;
  }
}

// acc = reset ? g : acc + g, one fp32 add per element (the order of autograd's in-place .grad += g);
// float4 body + scalar tail over n floats, grid-stride (as optim_kernel). Every thread reads the
// device word *reset_flag: one captured form of the micro-step serves both cases.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                              long long n, const int* __restrict__ reset_flag) {
  const bool reset = *reset_flag != 0;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    if (!reset) v = reinterpret_cast<const f32x4*>(acc)[i] + v;
    reinterpret_cast<f32x4*>(acc)[i] = v;
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) {
    float v = g[i];
    if (!reset) v = acc[i] + v;
    acc[i] = v;
  }
}

}  // namespace f3

using namespace f3;

extern "C" {

int f3_soft_ce_ex(const float* out, const float* label, const int64_t* label_idx, int N, int C,
                  float label_smoothing, float* loss, float* dout, void* stream) {
  if (!out || !loss || N < 1 || C < 1 || C > kSceMaxC) return F3_EINVAL;
  if ((label != nullptr) == (label_idx != nullptr)) return F3_EINVAL;  // exactly one label form
  if (!std::isfinite(label_smoothing) || label_smoothing < 0.f || label_smoothing > 1.f) return F3_EINVAL;
  SoftCeArgs a;
  a.out = out; a.label = label; a.label_idx = reinterpret_cast<const long long*>(label_idx);
  a.loss = loss; a.dout = dout; a.N = N; a.C = C;
  a.keep = 1.f - label_smoothing;
  a.share = label_smoothing / (float)C;
  hipStream_t s = (hipStream_t)stream;
  const long long blocks = ((long long)N + 255) / 256;
  const bool one = N <= kSceOneBlock;
  const int grid = one ? 1 : (int)(blocks < kSceMaxBlocks ? blocks : kSceMaxBlocks);
#define F3_SCE_CASE(CN)                                                                            \
  case CN:                                                                                         \
    if (one) hipLaunchKernelGGL((soft_ce_kernel<CN, true>), dim3(1), dim3(256), 0, s, a);          \
    else hipLaunchKernelGGL((soft_ce_kernel<CN, false>), dim3(grid), dim3(256), 0, s, a);          \
    break;
  switch (C <= kSceRegs ? C : 0) {
    F3_SCE_CASE(1) F3_SCE_CASE(2) F3_SCE_CASE(3) F3_SCE_CASE(4) F3_SCE_CASE(5) F3_SCE_CASE(6)
    F3_SCE_CASE(7) F3_SCE_CASE(8) F3_SCE_CASE(9) F3_SCE_CASE(10) F3_SCE_CASE(11) F3_SCE_CASE(12)
    F3_SCE_CASE(13) F3_SCE_CASE(14) F3_SCE_CASE(15) F3_SCE_CASE(16)
    F3_SCE_CASE(0)
  }
#undef F3_SCE_CASE
  F3_LAUNCH_CHECK();
  if (!one) {
    hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(256), 0, s, loss, grid, N);
    F3_LAUNCH_CHECK();
  }
  return F3_OK;
}

int f3_soft_ce_w(const float* out, const float* label, const int64_t* label_idx, const float* class_weight, int N,
                 int C, float label_smoothing, float* loss, float* dout, void* stream) {
  if (!out || !loss || !class_weight || N < 1 || C < 1 || C > kSceMaxC) return F3_EINVAL;
  if ((label != nullptr) == (label_idx != nullptr)) return F3_EINVAL;  // exactly one label form
  if (!std::isfinite(label_smoothing) || label_smoothing < 0.f || label_smoothing > 1.f) return F3_EINVAL;
  SoftCeWArgs a;
  a.b.out = out; a.b.label = label; a.b.label_idx = reinterpret_cast<const long long*>(label_idx);
  a.b.loss = loss; a.b.dout = dout; a.b.N = N; a.b.C = C;
  a.b.keep = 1.f - label_smoothing;
  a.b.share = label_smoothing / (float)C;
  a.w = class_weight;
  hipStream_t s = (hipStream_t)stream;
  const long long blocks = ((long long)N + 255) / 256;
  const bool one = N <= kSceOneBlock;
  const int grid = one ? 1 : (int)(blocks < kSceMaxBlocks ? blocks : kSceMaxBlocks);
  a.nwblk = (!one && label_idx) ? grid : 0;
  if (a.nwblk) {
    hipLaunchKernelGGL(soft_ce_w_sum_kernel, dim3(grid), dim3(256), 0, s, a);
    F3_LAUNCH_CHECK();
  }
#define F3_SCE_CASE(CN)                                                                            \
  case CN:                                                                                         \
    if (one) hipLaunchKernelGGL((soft_ce_w_kernel<CN, true>), dim3(1), dim3(256), 0, s, a);        \
    else hipLaunchKernelGGL((soft_ce_w_kernel<CN, false>), dim3(grid), dim3(256), 0, s, a);        \
    break;
  switch (C <= kSceRegs ? C : 0) {
    F3_SCE_CASE(1) F3_SCE_CASE(2) F3_SCE_CASE(3) F3_SCE_CASE(4) F3_SCE_CASE(5) F3_SCE_CASE(6)
    F3_SCE_CASE(7) F3_SCE_CASE(8) F3_SCE_CASE(9) F3_SCE_CASE(10) F3_SCE_CASE(11) F3_SCE_CASE(12)
    F3_SCE_CASE(13) F3_SCE_CASE(14) F3_SCE_CASE(15) F3_SCE_CASE(16)
    F3_SCE_CASE(0)
  }
#undef F3_SCE_CASE
  F3_LAUNCH_CHECK();
  if (!one) {
    hipLaunchKernelGGL(soft_ce_w_finish_kernel, dim3(1), dim3(256), 0, s, loss, grid, N, a.nwblk);
    F3_LAUNCH_CHECK();
  }
  return F3_OK;
}

int f3_grad_accumulate(float* acc, const float* grads, int64_t n, int* reset_flag, void* stream) {
  if (n < 0 || !reset_flag || (uintptr_t)reset_flag % 4 || (n && (!acc || !grads))) return F3_EINVAL;
  if (((uintptr_t)acc | (uintptr_t)grads) % 16) return F3_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    const long long blocks = (n / 4 + 255) / 256;
    const int grid = (int)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(grid), dim3(256), 0, s, acc, grads, (long long)n, reset_flag);
    F3_LAUNCH_CHECK();
  }
  // the next call adds: the caller sets the word again where its model.zero_grad() stands
  if (hipMemsetAsync(reset_flag, 0, sizeof(int), s) != hipSuccess) return F3_EHIP;
  return F3_OK;
}

}  // extern "C"
