// Step metrics kept on the device (layout and semantics: include/fall3.h):
//   running loss and top-k accuracy per batch   Multimodal_Fall3/model/main.py:57-77, 134-135
//   confusion matrix behind valid() / test()    model/main.py:148-248, main_cross_validation.py:247
//   per-parameter gradient L2 norms             model/main.py:84-89 (visualize_weights_and_gradients)
// Nothing here allocates or reads back to the host, so every call can be captured into a HIP graph.
// There are no global atomics: launches on one stream are serial and every word of an accumulator
// block has exactly one writer per launch, so the same inputs give the same bits on every run.
#include <cmath>

#include "common.h"
#include "fall3.h"

namespace f3 {

constexpr int kMetMaxC = 64;   // the confusion tile lives in LDS (64 x 64 int32 = 16 KiB)
constexpr int kMetRegs = 16;   // class counts up to this: the row is loaded into registers up front (ce_kernel)
constexpr int kMetHead = 2 + F3_METRICS_MAXK;  // int64 words between loss_sum and the confusion matrix

struct MetricsArgs {
  void* acc;
  const float* out;
  const float* label;
  const long long* label_idx;
  const float* loss;
  int N, C, nk;
  int k[F3_METRICS_MAXK];  // by value: no device table to keep alive behind a captured launch
};

// a NaN logit orders above every number (and ties with another NaN), as torch.topk / argmax order it
F3_DEV bool met_gt(float a, float b) { return a > b || (a != a && b == b); }
F3_DEV bool met_eq(float a, float b) { return a == b || (a != a && b != b); }

// One 256-thread workgroup walks the rows (thread t takes rows t, t + 256, ...). Counts are gathered
// in LDS with integer atomics (exact, order-free); the loss is reduced as ce_kernel<true> reduces it.
template <bool REGS>
__global__ __launch_bounds__(256) void metrics_update_kernel(MetricsArgs a) {
  __shared__ int conf[kMetMaxC * kMetMaxC];
  __shared__ int corr[F3_METRICS_MAXK];
  __shared__ float red[4];
  const int C = a.C, tid = threadIdx.x;
  for (int i = tid; i < C * C; i += 256) conf[i] = 0;
  if (tid < F3_METRICS_MAXK) corr[tid] = 0;
  __syncthreads();
  const int lim = REGS ? kMetRegs : C;
  constexpr int kU = REGS ? kMetRegs : 1;  // full unroll over the register row; the global-row loops stay rolled
  float lsum = 0.f;
  for (int n = tid; n < a.N; n += 256) {
    const float* o = a.out + (size_t)n * C;
    const float* y = a.label ? a.label + (size_t)n * C : nullptr;
    float ov[kMetRegs], yv[kMetRegs];
    long long ti = 0;
    if (!y) ti = a.label_idx[n];
    if (REGS) {
      // every load issued before the first use (clamped indices: no branches between them)
#pragma unroll
      for (int c = 0; c < kMetRegs; ++c) {
        const int cc = c < C ? c : C - 1;
        ov[c] = o[cc];
        yv[c] = y ? y[cc] : 0.f;
      }
    }
    auto O = [&](int c) { return REGS ? ov[c] : o[c]; };
    auto Y = [&](int c) { return REGS ? yv[c] : y[c]; };
    // the true class: arg-max of the soft label, lowest index on a tie; or the given index (a row
    // whose index lies outside [0, C) counts in `rows` only)
    int t = 0;
    bool valid = true;
    if (y) {
      float best = Y(0);
#pragma unroll kU
      for (int c = 1; c < lim; ++c)
        if (c < C && Y(c) > best) { best = Y(c); t = c; }
    } else {
      valid = ti >= 0 && ti < C;
      t = valid ? (int)ti : 0;
    }
    // the prediction (first class that nothing precedes) and the target's rank
    float ot = 0.f;
    if (REGS) {
#pragma unroll
      for (int c = 0; c < kMetRegs; ++c) ot = c == t ? ov[c] : ot;
    } else {
      ot = o[t];
    }
    int p = 0, rank = 0;
    float pbest = O(0);
#pragma unroll kU
    for (int c = 0; c < lim; ++c)
      if (c < C) {
        const float x = O(c);
        if (met_gt(x, pbest)) { pbest = x; p = c; }
        rank += (met_gt(x, ot) || (met_eq(x, ot) && c < t)) ? 1 : 0;
      }
    if (valid) {
      atomicAdd(&conf[t * C + p], 1);
      for (int j = 0; j < a.nk; ++j)
        if (rank < a.k[j]) atomicAdd(&corr[j], 1);
    }
    if (!a.loss) {
      // -(sum_c y_c log_softmax(out)_c): the row arithmetic of ce_kernel (head.hip); an index label is one-hot
      float mx = -INFINITY;
#pragma unroll kU
      for (int c = 0; c < lim; ++c)
        if (c < C) mx = fmaxf(mx, O(c));
      float s = 0.f;
#pragma unroll kU
      for (int c = 0; c < lim; ++c)
        if (c < C) s += expf(O(c) - mx);
      const float lse = mx + logf(s);
      float l = 0.f;
#pragma unroll kU
      for (int c = 0; c < lim; ++c)
        if (c < C) {
          const float yc = y ? Y(c) : ((valid && c == t) ? 1.f : 0.f);
          l -= yc * (O(c) - lse);
        }
      lsum += l;
    }
  }
  if (!a.loss) {
    for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
  }
  __syncthreads();
  double* loss_sum = static_cast<double*>(a.acc);
  long long* cnt = static_cast<long long*>(a.acc) + 1;  // batches, rows, correct[MAXK], confusion[C*C]
  if (tid == 0) {
    // the block's scalars have one writer: plain loads and stores
    const float batch_loss = a.loss ? *a.loss : (red[0] + red[1] + red[2] + red[3]) / (float)a.N;
    *loss_sum += (double)batch_loss;
    cnt[0] += 1;
    cnt[1] += a.N;
    for (int j = 0; j < a.nk; ++j) cnt[2 + j] += corr[j];
  }
  // each confusion word is owned by one thread (a single thread walking C*C words would serialise
  // up to 4096 round trips); untouched cells are neither read nor written
  for (int i = tid; i < C * C; i += 256)
    if (conf[i]) cnt[kMetHead + i] += conf[i];
}

// ---- per-segment gradient norms --------------------------------------------------------------
constexpr long long kSegChunk = 8192;  // floats per workgroup of the first launch (8 float4 per thread)

F3_DEV long long seg_chunks(long long len) { return len > 0 ? (len + kSegChunk - 1) / kSegChunk : 0; }

// Thread t owns the contiguous slice [t * per, (t + 1) * per) of the segment table. Returns the number
// of chunks in the slice and, through `before`, the number in all earlier slices (an LDS scan over
// the 256 slice counts). Both launches number the partials through this, so they agree.
F3_DEV long long seg_slice_scan(const long long* __restrict__ seg_len, int nseg, int per, long long* sh,
                                long long& before) {
  const int tid = threadIdx.x;
  const int lo = tid * per < nseg ? tid * per : nseg;
  const int hi = lo + per < nseg ? lo + per : nseg;
  long long mine = 0;
  for (int i = lo; i < hi; ++i) mine += seg_chunks(seg_len[i]);
  sh[tid] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const long long v = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  before = sh[tid] - mine;
  return mine;
}

// first launch: workgroup b squares one chunk of one segment in fp64 (the square of an fp32 value is
// exact there) and stores partial[b]. float4 loads on the 16-byte-aligned body, a scalar tail,
// wave-64 shuffles, then LDS across the four waves: a fixed order.
__global__ __launch_bounds__(256) void segment_partials_kernel(const float* __restrict__ g,
                                                               const long long* __restrict__ seg_off,
                                                               const long long* __restrict__ seg_len, int nseg,
                                                               double* __restrict__ partials) {
  __shared__ long long sh[256];
  __shared__ long long where[2];
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  const int per = (nseg + 255) / 256;
  const long long b = blockIdx.x;
  if (tid == 0) where[0] = -1;
  long long before;
  const long long mine = seg_slice_scan(seg_len, nseg, per, sh, before);  // (its barriers publish where[0])
  if (b >= before && b < before + mine) {  // exactly one thread: the chunk lies in its slice
    long long k = b - before;
    int s = tid * per;
    for (;; ++s) {
      const long long c = seg_chunks(seg_len[s]);
      if (k < c) break;
      k -= c;
    }
    where[0] = s;
    where[1] = k;
  }
  __syncthreads();
  if (where[0] < 0) return;  // a workgroup past the last chunk (the grid is an upper bound)
  const long long off = seg_off[where[0]], len = seg_len[where[0]];
  const long long lo = where[1] * kSegChunk;
  const long long n = len - lo < kSegChunk ? len - lo : kSegChunk;
  const float* x = g + off + lo;
  // (offsets are multiples of 4 floats by contract; one that is not takes the scalar path whole)
  const long long n4 = ((uintptr_t)x % 16 == 0) ? n / 4 : 0;
  double acc = 0.0;
  for (long long i = tid; i < n4; i += 256) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
  }
  for (long long i = n4 * 4 + tid; i < n; i += 256) acc += (double)x[i] * (double)x[i];
  acc = warp_sum_d(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// second launch, one workgroup: each thread adds the partials of its slice's segments in index order
// and stores norms[s]; thread 0 then adds the 256 slice sums in index order for norms[nseg].
// sqrt and scale in fp64, rounded to fp32 once. A table that needs more partials than the scratch
// holds yields NaN for the segments concerned instead of a read past the scratch.
__global__ __launch_bounds__(256) void segment_norms_kernel(const double* __restrict__ partials, long long npart,
                                                            const long long* __restrict__ seg_len, int nseg,
                                                            float* __restrict__ norms, double scale) {
  __shared__ long long sh[256];
  __shared__ double tot[256];
  const int tid = threadIdx.x;
  const int per = (nseg + 255) / 256;
  long long at;
  seg_slice_scan(seg_len, nseg, per, sh, at);
  const int lo = tid * per < nseg ? tid * per : nseg;
  const int hi = lo + per < nseg ? lo + per : nseg;
  double slice = 0.0;
  for (int s = lo; s < hi; ++s) {
    const long long c = seg_chunks(seg_len[s]);
    double sum = 0.0;
    if (at + c > npart) {
      sum = NAN;
    } else {
      for (long long i = 0; i < c; ++i) sum += partials[at + i];
    }
    at += c;
    norms[s] = (float)(scale * sqrt(sum));
    slice += sum;
  }
  tot[tid] = slice;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < 256; ++i) sum += tot[i];
    norms[nseg] = (float)(scale * sqrt(sum));
  }
}

}  // namespace f3

using namespace f3;

extern "C" {

int64_t f3_metrics_bytes(int C) {
  if (C < 1 || C > kMetMaxC) return 0;
  return (int64_t)sizeof(double) + (int64_t)sizeof(int64_t) * (kMetHead + (int64_t)C * C);
}

int f3_metrics_reset(void* acc, int C, void* stream) {
  if (!acc || (uintptr_t)acc % 8 || C < 1 || C > kMetMaxC) return F3_EINVAL;
  if (hipMemsetAsync(acc, 0, (size_t)f3_metrics_bytes(C), (hipStream_t)stream) != hipSuccess) return F3_EHIP;
  return F3_OK;
}

int f3_metrics_update(void* acc, const float* out, const float* label, const int64_t* label_idx, const float* loss,
                      int N, int C, const int* top_k, int nk, void* stream) {
  if (!acc || (uintptr_t)acc % 8 || !out || N < 1) return F3_EINVAL;
  if (C < 1 || C > kMetMaxC || nk < 0 || nk > F3_METRICS_MAXK || (nk && !top_k)) return F3_EINVAL;
  if ((label != nullptr) == (label_idx != nullptr)) return F3_EINVAL;  // exactly one label form
  MetricsArgs a;
  a.acc = acc; a.out = out; a.label = label; a.label_idx = reinterpret_cast<const long long*>(label_idx);
  a.loss = loss; a.N = N; a.C = C; a.nk = nk;
  for (int j = 0; j < F3_METRICS_MAXK; ++j) a.k[j] = 0;
  for (int j = 0; j < nk; ++j) {
    if (top_k[j] < 1 || top_k[j] > C) return F3_EINVAL;
    a.k[j] = top_k[j];
  }
  hipStream_t s = (hipStream_t)stream;
  if (C <= kMetRegs) hipLaunchKernelGGL(metrics_update_kernel<true>, dim3(1), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(metrics_update_kernel<false>, dim3(1), dim3(256), 0, s, a);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int64_t f3_segment_norms_scratch_bytes(int64_t total_len, int nseg) {
  if (total_len < 0 || nseg < 0) return 0;
  // every segment rounds its chunk count up at most once; never 0, so a caller can always allocate it
  return (int64_t)sizeof(double) * (total_len / kSegChunk + nseg + 1);
}

int f3_segment_norms(const float* g, const int64_t* seg_off, const int64_t* seg_len, int nseg, float* norms,
                     void* scratch, int64_t scratch_bytes, double scale, void* stream) {
  if (!norms || nseg < 0 || !std::isfinite(scale)) return F3_EINVAL;
  if (nseg && (!g || !seg_off || !seg_len || !scratch || (uintptr_t)scratch % 8 || (uintptr_t)g % 16)) return F3_EINVAL;
  const long long npart = scratch_bytes / (long long)sizeof(double);
  if (nseg && (npart < 1 || npart > 0x7fffffffLL)) return F3_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long* off = reinterpret_cast<const long long*>(seg_off);
  const long long* len = reinterpret_cast<const long long*>(seg_len);
  double* partials = static_cast<double*>(scratch);
  if (nseg) {
    hipLaunchKernelGGL(segment_partials_kernel, dim3((unsigned)npart), dim3(256), 0, s, g, off, len, nseg, partials);
    F3_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(segment_norms_kernel, dim3(1), dim3(256), 0, s, partials, npart, len, nseg, norms, scale);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

}  // extern "C"
