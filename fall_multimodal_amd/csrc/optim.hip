// The optimizers of build_optimizer besides plain RMSprop (Multimodal_Fall3/model/optimizer.py:20-29:
// torch.optim.SGD / Adam / AdamW; RMSprop with weight decay) and the root driver's global gradient-norm
// clipping (Multimodal_Fall3/main.py:108-113 clip_grad_norm_), as flat updates over the one parameter
// buffer. Formulas: include/fall3.h (f3_optim_config).
//
// Every launch of one step reads the step scalars (OptScalars) that the step's begin kernel wrote, so
// the Adam step count lives on the device and a replayed graph advances it. The state recurrences
// (momentum buffer, exp_avg, exp_avg_sq, square_avg) and the effective gradient are evaluated in fp64
// and rounded to fp32 once: m + (1-b1)(g - m) cancels, and an fp32 evaluation loses relative accuracy
// of the result exactly there. The kernels are memory bound (3-4 loads, 2-3 stores per element), so
// the fp64 VALU work is free. The one sqrt and the one division per element are fp32.
//
// The hyper-parameters reach the kernels by value (f3_optim_step), or, for a step recorded into a HIP
// graph, from the OptHyper device block when the kernel runs (f3_optim_step_hyper, optim_hyper_kernel):
// lr_scheduler.step(e) (model/main.py:321-322) then takes effect on a replay. Both forms give the same bits.
#include <cmath>
#include <cstddef>

#include "common.h"
#include "sensor.h"
#include "fall3.h"

namespace f3 {

// kernel variants: the F3_OPT_* kinds, and SGD without a momentum buffer
enum { OK_RMS = 0, OK_SGD = 1, OK_ADAM = 2, OK_ADAMW = 3, OK_SGD0 = 4 };

struct OptArgs {
  double lr, a, oma, mu, b1, omb1, b2, omb2, wd, gscale;
  float lr_f, eps_f;
  int nesterov;
};

// The kernel arguments from the hyper-parameters as f3_optim_config carries them: evaluated on the host
// for the by-value kernels and per thread in the device-reading ones (each is one IEEE operation or one
// conversion, so both places give the same bits).
__host__ __device__ inline OptArgs opt_args_of(double lr, double alpha, double eps, double mu, double b1, double b2,
                                               double wd, double gscale, int nesterov) {
#pragma clang fp contract(off)
  OptArgs a;
  a.lr = lr; a.a = alpha; a.oma = 1.0 - alpha; a.mu = mu;
  a.b1 = b1; a.omb1 = 1.0 - b1; a.b2 = b2; a.omb2 = 1.0 - b2; a.wd = wd; a.gscale = gscale;
  a.lr_f = (float)lr; a.eps_f = (float)eps; a.nesterov = nesterov;
  return a;
}

// One element. contract(off): the flat and the ranges kernel, and the vector body and the scalar tail,
// must round identically (the per-layer updates are compared bit for bit with the flat one).
template <int KIND>
F3_DEV void opt_update(float& p, float& s0, float& s1, float grad, const OptArgs& a, double sg, float bc1,
                       float bc2s) {
#pragma clang fp contract(off)
  double g = sg * (double)grad;
  double pd = (double)p;
  if (KIND == OK_ADAMW) pd = pd * (1.0 - a.lr * a.wd);
  else g = g + a.wd * pd;
  if (KIND == OK_RMS) {
    const float sq = (float)(a.a * (double)s0 + a.oma * g * g);
    s0 = sq;
    p = p - a.lr_f * (float)g / (sqrtf(sq) + a.eps_f);
  } else if (KIND == OK_SGD) {
    const float buf = (float)(a.mu * (double)s0 + g);
    s0 = buf;
    const double d = a.nesterov ? g + a.mu * (double)buf : (double)buf;
    p = (float)(pd - a.lr * d);
  } else if (KIND == OK_SGD0) {
    p = (float)(pd - a.lr * g);
  } else {
    const float m = (float)((double)s0 + a.omb1 * (g - (double)s0));
    const float v = (float)(a.b2 * (double)s1 + a.omb2 * g * g);
    s0 = m;
    s1 = v;
    const float q = m / (sqrtf(v) * bc2s + a.eps_f);
    p = (float)(pd - (a.lr * (double)bc1) * (double)q);
  }
}

template <int KIND>
F3_DEV void opt_update4(float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1,
                        const float* __restrict__ g, long long i4, const OptArgs& a, double sg, float bc1,
                        float bc2s) {
  constexpr bool has0 = KIND != OK_SGD0, has1 = KIND == OK_ADAM || KIND == OK_ADAMW;
  const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i4];
  f32x4 pv = reinterpret_cast<f32x4*>(p)[i4];
  f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
  if (has0) av = reinterpret_cast<f32x4*>(s0)[i4];
  if (has1) bv = reinterpret_cast<f32x4*>(s1)[i4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = pv[e], ae = av[e], be = bv[e];
    opt_update<KIND>(pe, ae, be, gv[e], a, sg, bc1, bc2s);
    pv[e] = pe; av[e] = ae; bv[e] = be;
  }
  reinterpret_cast<f32x4*>(p)[i4] = pv;
  if (has0) reinterpret_cast<f32x4*>(s0)[i4] = av;
  if (has1) reinterpret_cast<f32x4*>(s1)[i4] = bv;
}

F3_DEV bool opt_skipped(const OptSkip& k, long long i) {
  bool in = false;
  for (int j = 0; j < k.n; ++j) in = in || (i >= k.lo[j] && i < k.lo[j] + k.len[j]);
  return in;
}

// flat shape: float4 body + scalar tail over n floats, grid-stride (as rmsprop_kernel). GUARD (the step's
// skip_nonfinite): every thread reads the begin kernel's verdict and returns before its first load when
// the step is skipped, so nothing is stored; without GUARD the test is not compiled in.
template <int KIND, bool GUARD = false>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, float* __restrict__ s0,
                                                    float* __restrict__ s1, const float* __restrict__ g,
                                                    long long n, OptArgs a, OptSkip skip,
                                                    const OptScalars* __restrict__ sc) {
  if (GUARD && sc->last_skipped != 0) return;
  const double sg = a.gscale * (double)sc->clip_coef;
  const float bc1 = sc->bc1, bc2s = sc->bc2s;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    if (skip.n && opt_skipped(skip, i * 4)) continue;  // skip ranges are whole float4s
    opt_update4<KIND>(p, s0, s1, g, i, a, sg, bc1, bc2s);
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) {
    if (skip.n && opt_skipped(skip, i)) continue;
    float pe = p[i], ae = KIND != OK_SGD0 ? s0[i] : 0.f, be = (KIND == OK_ADAM || KIND == OK_ADAMW) ? s1[i] : 0.f;
    opt_update<KIND>(pe, ae, be, g[i], a, sg, bc1, bc2s);
    p[i] = pe;
    if (KIND != OK_SGD0) s0[i] = ae;
    if (KIND == OK_ADAM || KIND == OK_ADAMW) s1[i] = be;
  }
}

// optim_kernel in the form a HIP graph records: every thread builds its OptArgs from the hyper-parameter
// block once, before its loop, with opt_args_of's expressions (the ones the host evaluates for
// optim_kernel), and the elements go through the same opt_update4 / opt_update, so the two forms give the
// same bits on the same values and a replay follows the block. Which variant runs (KIND, nesterov) is the
// step's structure and stays an argument. A kernel of its own with the loop written again: moving the
// loop into a function shared with optim_kernel changes that kernel's instruction schedule, and the
// by-value kernels are to stay the code they were.
template <int KIND, bool GUARD = false>
__global__ __launch_bounds__(256) void optim_hyper_kernel(float* __restrict__ p, float* __restrict__ s0,
                                                          float* __restrict__ s1, const float* __restrict__ g,
                                                          long long n, const OptHyper* __restrict__ h, int nesterov,
                                                          OptSkip skip, const OptScalars* __restrict__ sc) {
  if (GUARD && sc->last_skipped != 0) return;
  const OptArgs a = opt_args_of(h->lr, h->alpha, h->eps, h->momentum, h->beta1, h->beta2, h->weight_decay,
                                h->grad_scale, nesterov);
  const double sg = a.gscale * (double)sc->clip_coef;
  const float bc1 = sc->bc1, bc2s = sc->bc2s;
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    if (skip.n && opt_skipped(skip, i * 4)) continue;
    opt_update4<KIND>(p, s0, s1, g, i, a, sg, bc1, bc2s);
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) {
    if (skip.n && opt_skipped(skip, i)) continue;
    float pe = p[i], ae = KIND != OK_SGD0 ? s0[i] : 0.f, be = (KIND == OK_ADAM || KIND == OK_ADAMW) ? s1[i] : 0.f;
    opt_update<KIND>(pe, ae, be, g[i], a, sg, bc1, bc2s);
    p[i] = pe;
    if (KIND != OK_SGD0) s0[i] = ae;
    if (KIND == OK_ADAM || KIND == OK_ADAMW) s1[i] = be;
  }
}

// ranges shape (as rmsprop_ranges_kernel): n4 float4s spread over r.n 16-byte-aligned ranges
template <int KIND>
__global__ __launch_bounds__(256) void optim_ranges_kernel(float* __restrict__ p, float* __restrict__ s0,
                                                           float* __restrict__ s1, const float* __restrict__ g,
                                                           RmsRanges r, long long n4, OptArgs a,
                                                           const OptScalars* __restrict__ sc) {
  const double sg = a.gscale * (double)sc->clip_coef;
  const float bc1 = sc->bc1, bc2s = sc->bc2s;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
    long long k = i;
    int j = 0;
    for (; j < r.n - 1 && k >= r.len[j] / 4; ++j) k -= r.len[j] / 4;
    opt_update4<KIND>(p, s0, s1, g, r.lo[j] / 4 + k, a, sg, bc1, bc2s);
  }
}

// sum g^2 in fp64 (an fp32 square is exact in fp64): workgroup b owns the fixed slice of float4s
// [b * chunk4, (b+1) * chunk4), its threads stride through it, an LDS tree adds the 256 thread sums in a
// fixed order, and the workgroup stores one partial. Block 0 also takes the n % 4 tail. No atomics.
__global__ __launch_bounds__(256) void gradnorm_partials_kernel(const float* __restrict__ g, long long n,
                                                                double* __restrict__ partials) {
  __shared__ double sh[256];
  const long long n4 = n / 4;
  const long long chunk4 = (n4 + gridDim.x - 1) / gridDim.x;
  const long long lo = blockIdx.x * chunk4;
  const long long hi = lo + chunk4 < n4 ? lo + chunk4 : n4;
  double acc = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long i = n4 * 4; i < n; ++i) acc += (double)g[i] * (double)g[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// once per optimizer step, one workgroup: t += 1, the bias corrections in fp64 from the integer t, the
// norm from the partials in index order, the clip coefficient (clip_grad_norm_: max_norm / (norm + 1e-6),
// clamped to 1; a non-finite norm propagates as in torch).
// guard (skip_nonfinite): the partials are always summed, and the step is skipped iff the fp64 sum of
// squares is not finite, which is exactly when some element is (an fp32 square is exact in fp64, the
// squares are non-negative and n * FLT_MAX^2 is far below DBL_MAX). The fp32 grad_norm is not the test: a
// finite gradient may have a norm above FLT_MAX. A skip leaves t and the bias corrections as they were,
// writes clip_coef 0 and the non-finite norm, counts itself and sets last_skipped for the update launch.
F3_DEV void optim_begin(OptScalars* __restrict__ sc, int adam, double b1, double b2, double max_norm,
                        double gscale, int guard) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0;
  if (max_norm > 0.0 || guard)
    for (int i = 0; i < kNormBlocks; ++i) sum += sc->partials[i];
  const double nd = gscale * sqrt(sum);
  if (guard) {
    if (!isfinite(sum)) {
      sc->clip_coef = 0.f;
      sc->grad_norm = (float)nd;
      sc->skipped = sc->skipped + 1;
      sc->last_skipped = 1;
      return;
    }
    sc->last_skipped = 0;
  }
  const long long t = sc->t + 1;
  sc->t = t;
  float bc1 = 1.f, bc2s = 1.f;
  if (adam) {
    bc1 = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    bc2s = (float)(1.0 / sqrt(1.0 - pow(b2, (double)t)));
  }
  sc->bc1 = bc1;
  sc->bc2s = bc2s;
  float coef = 1.f, norm = 0.f;
  if (max_norm > 0.0) {
    const double c = max_norm / (nd + 1e-6);
    norm = (float)nd;
    coef = (float)(c > 1.0 ? 1.0 : c);
  } else if (guard) {
    norm = (float)nd;  // a by-product: the sum was formed anyway
  }
  sc->clip_coef = coef;
  sc->grad_norm = norm;
}

__global__ void optim_begin_kernel(OptScalars* __restrict__ sc, int adam, double b1, double b2, double max_norm,
                                   double gscale, int guard) {
  optim_begin(sc, adam, b1, b2, max_norm, gscale, guard);
}

// The recorded form: the betas, max_norm and grad_scale from the block. Whether the step clips or guards
// (the norm partials were launched before this kernel) is structure: without clip max_norm counts as 0.
__global__ void optim_begin_hyper_kernel(OptScalars* __restrict__ sc, int adam, int clip, int guard,
                                         const OptHyper* __restrict__ h) {
  optim_begin(sc, adam, h->beta1, h->beta2, clip ? h->max_norm : 0.0, h->grad_scale, guard);
}

// one thread: the nine values into the block (f3_optim_hyper_set), launched eagerly on the caller's stream
__global__ void optim_hyper_write_kernel(OptHyper* __restrict__ h, OptHyper v) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  h->lr = v.lr; h->alpha = v.alpha; h->eps = v.eps; h->momentum = v.momentum;
  h->beta1 = v.beta1; h->beta2 = v.beta2; h->weight_decay = v.weight_decay;
  h->max_norm = v.max_norm; h->grad_scale = v.grad_scale;
}

}  // namespace f3

using namespace f3;

namespace {
OptArgs opt_args(const OptLaunch& o) {
  return opt_args_of(o.lr, o.alpha, o.eps, o.mu, o.b1, o.b2, o.wd, o.gscale, o.nesterov);
}
int opt_variant(const OptLaunch& o) { return o.kind == F3_OPT_SGD && o.mu == 0.0 ? (int)OK_SGD0 : o.kind; }
int opt_grid(long long n4) {
  const long long blocks = (n4 + 255) / 256;
  return (int)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096);
}
bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }
// the configuration's skip ranges for a flat update over n floats
int opt_skip_of(const f3_optim_config* cfg, int64_t n, OptSkip* skip) {
  if (n < 0 || cfg->nskip < 0 || cfg->nskip > F3_OPT_MAX_SKIP) return F3_EINVAL;
  skip->n = cfg->nskip;
  for (int j = 0; j < skip->n; ++j) {
    skip->lo[j] = cfg->skip_lo[j];
    skip->len[j] = cfg->skip_len[j];
    if (skip->lo[j] < 0 || skip->len[j] < 0 || skip->lo[j] % 4 || skip->len[j] % 4 ||
        skip->lo[j] + skip->len[j] > ((n + 3) / 4) * 4)
      return F3_EINVAL;
  }
  return F3_OK;
}
}  // namespace

// the kind and the values of a configuration, as every entry that takes one checks them
static int opt_check_values(const f3_optim_config* c) {
  if (!c || c->kind < F3_OPT_RMSPROP || c->kind > F3_OPT_ADAMW) return F3_EINVAL;
  if (!finite_nonneg(c->lr) || !finite_nonneg(c->weight_decay) || !finite_nonneg(c->max_norm) ||
      !std::isfinite(c->grad_scale) || c->grad_scale <= 0.0)
    return F3_EINVAL;
  if (c->kind == F3_OPT_RMSPROP) {
    if (c->momentum != 0.0) return F3_EINVAL;  // RMSprop momentum: not built
    if (!finite_nonneg(c->alpha) || c->alpha >= 1.0 || !finite_nonneg(c->eps)) return F3_EINVAL;
  } else if (c->kind == F3_OPT_SGD) {
    if (!finite_nonneg(c->momentum)) return F3_EINVAL;
  } else {
    if (!finite_nonneg(c->beta1) || c->beta1 >= 1.0 || !finite_nonneg(c->beta2) || c->beta2 >= 1.0 ||
        !finite_nonneg(c->eps))
      return F3_EINVAL;
  }
  return F3_OK;
}

// what the structure of a step (kind, momentum zero or not, nesterov) asks of the state pointers
static int opt_check_states(const f3_optim_config* c, const float* s0, const float* s1) {
  if (c->kind == F3_OPT_RMSPROP) return s0 ? F3_OK : F3_EINVAL;
  if (c->kind == F3_OPT_SGD) {
    if (c->nesterov && c->momentum == 0.0) return F3_EINVAL;  // torch: nesterov needs a momentum
    return c->momentum != 0.0 && !s0 ? F3_EINVAL : F3_OK;
  }
  return s0 && s1 ? F3_OK : F3_EINVAL;
}

int f3_optim_resolve(const f3_optim_config* c, float* p, float* s0, float* s1, const float* g, void* scalars,
                     OptLaunch* o) {
  if (!c || !p || !g || !scalars || (uintptr_t)scalars % 8) return F3_EINVAL;
  F3_TRY(opt_check_values(c));
  F3_TRY(opt_check_states(c, s0, s1));
  const bool adam = c->kind == F3_OPT_ADAM || c->kind == F3_OPT_ADAMW;
  o->kind = c->kind; o->nesterov = c->nesterov != 0;
  o->lr = c->lr; o->alpha = c->alpha; o->eps = c->eps; o->mu = c->momentum;
  o->b1 = adam ? c->beta1 : 0.0; o->b2 = adam ? c->beta2 : 0.0;
  o->wd = c->weight_decay; o->max_norm = c->max_norm; o->gscale = c->grad_scale;
  o->p = p; o->s0 = s0; o->s1 = s1; o->g = g; o->sc = static_cast<OptScalars*>(scalars);
  o->guard = c->skip_nonfinite != 0;
  return F3_OK;
}

int f3_optim_begin(const OptLaunch& o, long long n, hipStream_t s) {
  if (n < 0 || (uintptr_t)o.g % 16) return F3_EINVAL;
  if (o.max_norm > 0.0 || o.guard) {
    hipLaunchKernelGGL(gradnorm_partials_kernel, dim3(kNormBlocks), dim3(256), 0, s, o.g, n, o.sc->partials);
    F3_LAUNCH_CHECK();
  }
  const int adam = o.kind == F3_OPT_ADAM || o.kind == F3_OPT_ADAMW;
  hipLaunchKernelGGL(optim_begin_kernel, dim3(1), dim3(64), 0, s, o.sc, adam, o.b1, o.b2, o.max_norm, o.gscale,
                     (int)o.guard);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

#define F3_OPT_DISPATCH(VARIANT, KERNEL, ...)                                               \
  switch (VARIANT) {                                                                        \
    case OK_RMS: hipLaunchKernelGGL(KERNEL<OK_RMS>, __VA_ARGS__); break;                    \
    case OK_SGD: hipLaunchKernelGGL(KERNEL<OK_SGD>, __VA_ARGS__); break;                    \
    case OK_SGD0: hipLaunchKernelGGL(KERNEL<OK_SGD0>, __VA_ARGS__); break;                  \
    case OK_ADAM: hipLaunchKernelGGL(KERNEL<OK_ADAM>, __VA_ARGS__); break;                  \
    default: hipLaunchKernelGGL(KERNEL<OK_ADAMW>, __VA_ARGS__); break;                      \
  }
// the guarded instantiations (flat shapes only: the decision needs every gradient)
#define F3_OPT_DISPATCH_GUARDED(VARIANT, KERNEL, ...)                                                     \
  switch (VARIANT) {                                                                                      \
    case OK_RMS: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<OK_RMS, true>), __VA_ARGS__); break;           \
    case OK_SGD: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<OK_SGD, true>), __VA_ARGS__); break;           \
    case OK_SGD0: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<OK_SGD0, true>), __VA_ARGS__); break;         \
    case OK_ADAM: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<OK_ADAM, true>), __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<OK_ADAMW, true>), __VA_ARGS__); break;             \
  }

int f3_optim_flat(const OptLaunch& o, long long n, const OptSkip& skip, hipStream_t s) {
  if (n < 0 || skip.n < 0 || skip.n > kOptSkip) return F3_EINVAL;
  for (int j = 0; j < skip.n; ++j)
    if (skip.lo[j] % 4 || skip.len[j] % 4 || skip.lo[j] < 0 || skip.len[j] < 0) return F3_EINVAL;
  if (((uintptr_t)o.p | (uintptr_t)o.s0 | (uintptr_t)o.s1 | (uintptr_t)o.g) % 16) return F3_EINVAL;
  if (n == 0) return F3_OK;
  if (o.legacy_rms())  // skipped entries carry a zero gradient: RMSprop without decay leaves them as they are
    return f3_rmsprop(o.p, o.s0, o.g, n, (float)o.lr, (float)o.alpha, (float)o.eps, (float)o.gscale, s);
  const OptArgs a = opt_args(o);
  const OptScalars* sc = o.sc;
  if (o.guard) {
    F3_OPT_DISPATCH_GUARDED(opt_variant(o), optim_kernel, dim3(opt_grid(n / 4)), dim3(256), 0, s, o.p, o.s0, o.s1,
                            o.g, n, a, skip, sc);
  } else {
    F3_OPT_DISPATCH(opt_variant(o), optim_kernel, dim3(opt_grid(n / 4)), dim3(256), 0, s, o.p, o.s0, o.s1, o.g, n, a,
                    skip, sc);
  }
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int f3_optim_ranges(const OptLaunch& o, const RmsRanges& r, hipStream_t s) {
  // the norm and the guard's decision need every gradient: flat update after the backward
  if (o.max_norm > 0.0 || o.guard) return F3_EINVAL;
  if (o.legacy_rms())
    return f3_rmsprop_ranges(o.p, o.s0, o.g, r, (float)o.lr, (float)o.alpha, (float)o.eps, (float)o.gscale, s);
  if (r.n < 0 || r.n > kRmsRanges) return F3_EINVAL;
  if (((uintptr_t)o.p | (uintptr_t)o.s0 | (uintptr_t)o.s1 | (uintptr_t)o.g) % 16) return F3_EINVAL;
  long long n4 = 0;
  for (int j = 0; j < r.n; ++j) {
    if (r.lo[j] % 4 || r.len[j] % 4 || r.len[j] < 0 || r.lo[j] < 0) return F3_EINVAL;
    n4 += r.len[j] / 4;
  }
  if (n4 == 0) return F3_OK;
  const OptArgs a = opt_args(o);
  const OptScalars* sc = o.sc;
  F3_OPT_DISPATCH(opt_variant(o), optim_ranges_kernel, dim3(opt_grid(n4)), dim3(256), 0, s, o.p, o.s0, o.s1, o.g, r,
                  n4, a, sc);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

extern "C" {

int64_t f3_optim_scalars_bytes(void) { return (int64_t)sizeof(OptScalars); }

int64_t f3_optim_guard_offset(void) { return (int64_t)offsetof(OptScalars, skipped); }

int f3_optim_step(const f3_optim_config* cfg, float* params, float* state0, float* state1, const float* grads,
                  int64_t n, void* scalars, void* stream) {
  OptLaunch o;
  F3_TRY(f3_optim_resolve(cfg, params, state0, state1, grads, scalars, &o));
  OptSkip skip;
  F3_TRY(opt_skip_of(cfg, n, &skip));
  hipStream_t s = (hipStream_t)stream;
  F3_TRY(f3_optim_begin(o, n, s));
  return f3_optim_flat(o, n, skip, s);
}

int64_t f3_optim_hyper_bytes(void) { return (int64_t)sizeof(OptHyper); }

int f3_optim_hyper_set(const f3_optim_config* cfg, void* hyper, void* stream) {
  if (!hyper || (uintptr_t)hyper % 8) return F3_EINVAL;
  F3_TRY(opt_check_values(cfg));
  const OptHyper v = {cfg->lr, cfg->alpha, cfg->eps, cfg->momentum, cfg->beta1, cfg->beta2, cfg->weight_decay,
                      cfg->max_norm, cfg->grad_scale};
  hipLaunchKernelGGL(optim_hyper_write_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     static_cast<OptHyper*>(hyper), v);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int f3_optim_step_hyper(const f3_optim_config* cfg, float* params, float* state0, float* state1, const float* grads,
                        int64_t n, const void* hyper, void* scalars, void* stream) {
  if (!cfg || !params || !grads || !hyper || (uintptr_t)hyper % 8) return F3_EINVAL;
  if (cfg->kind < F3_OPT_RMSPROP || cfg->kind > F3_OPT_ADAMW) return F3_EINVAL;
  if (cfg->kind == F3_OPT_RMSPROP && cfg->momentum != 0.0) return F3_EINVAL;  // RMSprop momentum: not built
  F3_TRY(opt_check_states(cfg, state0, state1));
  OptSkip skip;
  F3_TRY(opt_skip_of(cfg, n, &skip));
  if (((uintptr_t)params | (uintptr_t)state0 | (uintptr_t)state1 | (uintptr_t)grads) % 16) return F3_EINVAL;
  const OptHyper* h = static_cast<const OptHyper*>(hyper);
  hipStream_t s = (hipStream_t)stream;
  // the structure, from cfg: the plain-RMSprop route, clipping and the guard on or off, the kernel variant
  const bool clip = cfg->max_norm > 0.0;
  const bool guard = cfg->skip_nonfinite != 0;
  if (cfg->kind == F3_OPT_RMSPROP && cfg->weight_decay == 0.0 && !clip && !guard)
    return f3_rmsprop_hyper(params, state0, grads, n, h, s);  // skipped entries: as in f3_optim_flat
  if (!scalars || (uintptr_t)scalars % 8) return F3_EINVAL;
  OptScalars* sc = static_cast<OptScalars*>(scalars);
  if (clip || guard) {
    hipLaunchKernelGGL(gradnorm_partials_kernel, dim3(kNormBlocks), dim3(256), 0, s, grads, n, sc->partials);
    F3_LAUNCH_CHECK();
  }
  const int adam = cfg->kind == F3_OPT_ADAM || cfg->kind == F3_OPT_ADAMW;
  hipLaunchKernelGGL(optim_begin_hyper_kernel, dim3(1), dim3(64), 0, s, sc, adam, (int)clip, (int)guard, h);
  F3_LAUNCH_CHECK();
  if (n == 0) return F3_OK;
  const int variant = cfg->kind == F3_OPT_SGD && cfg->momentum == 0.0 ? (int)OK_SGD0 : cfg->kind;
  const int nesterov = cfg->nesterov != 0;
  const OptScalars* csc = sc;
  if (guard) {
    F3_OPT_DISPATCH_GUARDED(variant, optim_hyper_kernel, dim3(opt_grid(n / 4)), dim3(256), 0, s, params, state0,
                            state1, grads, (long long)n, h, nesterov, skip, csc);
  } else {
    F3_OPT_DISPATCH(variant, optim_hyper_kernel, dim3(opt_grid(n / 4)), dim3(256), 0, s, params, state0, state1,
                    grads, (long long)n, h, nesterov, skip, csc);
  }
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int f3_optim_step_ranges(const f3_optim_config* cfg, float* params, float* state0, float* state1,
                         const float* grads, int nranges, const int64_t* lo, const int64_t* len, void* scalars,
                         void* stream) {
  OptLaunch o;
  F3_TRY(f3_optim_resolve(cfg, params, state0, state1, grads, scalars, &o));
  if (nranges < 0 || nranges > kRmsRanges || (nranges && (!lo || !len)) || o.max_norm > 0.0 || o.guard)
    return F3_EINVAL;
  RmsRanges r;
  r.n = nranges;
  for (int j = 0; j < nranges; ++j) {
    r.lo[j] = lo[j];
    r.len[j] = len[j];
  }
  hipStream_t s = (hipStream_t)stream;
  F3_TRY(f3_optim_begin(o, 0, s));
  return f3_optim_ranges(o, r, s);
}

}  // extern "C"
