// Kernel-level entries of the C ABI (include/fall3.h): single convolutions, weight gradients and graph
// mixes as the step launches them, for the parity tests and the roofline tools. They share no state
// with the network (net.cpp); their scratch is kept for the process lifetime.
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "kernels.h"
#include "layers.h"
#include "host_args.h"
#include "fall3.h"

using namespace f3;

extern "C" {

// test-entry scratch (kept for the process lifetime; the network uses its workspace)
static const unsigned short* test_zero_page() {
  static void* z = nullptr;
  if (!z && hipMalloc(&z, 4096) == hipSuccess) (void)hipMemset(z, 0, 4096);
  return (const unsigned short*)z;
}
static float* test_scratch(size_t n) {
  static float* p = nullptr;
  static size_t cap = 0;
  if (n > cap) {
    if (p) (void)hipFree(p);
    p = nullptr;
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return nullptr;
    cap = n;
  }
  return p;
}

int f3_conv_forward(const void* x, const float* w, const float* bias, float* out, float* wpack, int N, int T_in,
                    int V, int Cin, int Cout, int KT, int stride, int pad, int precision, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (precision < 0 || precision > F3_PRECISION_BF16X3) return F3_EINVAL;
  const bool bf_out = precision == F3_CONV_BF16_OUT;
  if (bf_out) precision = F3_PRECISION_BF16;
  const int x3 = precision == F3_PRECISION_BF16X3;
  const int hb = precision != F3_PRECISION_FP32;
  if (w) {  // w == NULL: wpack already holds the packed operand (timing the GEMM alone)
    PrepTable t;
    t.n = 0;
    add_job(t, PREP_PACK_CONV, Cout * KT * Cin, wpack, w, nullptr, nullptr, Cout, Cin, KT, x3 ? 2 : hb);
    F3_TRY(f3_prep(t, s));
  }
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_out * V, Cout, Cin, KT, stride, pad, 0, T_out, T_in, V, Cin, Cout);
  if (precision == F3_PRECISION_BF16) {
    a.inb = (const unsigned short*)x;
    a.zero = test_zero_page();
  } else {
    a.in = (const float*)x;
  }
  a.w = wpack; a.wb = bf(wpack, hb); a.out = out; a.bias = bias; a.x3 = x3;
  if (bf_out) a.outb = reinterpret_cast<unsigned short*>(out);
  return f3_conv_gemm(&a, 0, EPI_BIAS, s);
}

int f3_conv_backward_data(const void* dy, const float* w, float* dx, float* wpack, int N, int T_in, int V, int Cin,
                          int Cout, int KT, int stride, int pad, int precision, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (precision < 0 || (precision > 2 && precision != F3_PRECISION_BF16X3)) return F3_EINVAL;
  const int x3 = precision == F3_PRECISION_BF16X3;
  const int hb = precision != F3_PRECISION_FP32;
  PrepTable t;
  t.n = 0;
  add_job(t, PREP_PACK_CONV_T, Cout * KT * Cin, wpack, w, nullptr, nullptr, Cout, Cin, KT, x3 ? 2 : hb);
  F3_TRY(f3_prep(t, s));
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_in * V, Cin, Cout, KT, stride, pad, 1, T_in, T_out, V, Cout, Cin);
  if (precision == F3_PRECISION_BF16) {
    a.inb = (const unsigned short*)dy;
    a.zero = test_zero_page();
  } else {
    a.in = (const float*)dy;
  }
  a.w = wpack; a.wb = bf(wpack, hb); a.out = dx; a.x3 = x3;
  return f3_conv_gemm(&a, 0, 0, s);
}

int f3_pointwise_conv(const void* x, const void* wpack, const float* bias, void* out, int out_bf16, double* st_sum,
                      double* st_sq, int N, int T_in, int T_out, int V, int Cin, int Cout, int stride, int transposed,
                      int epi, void* stream) {
  if (!x || !wpack || !out || N <= 0 || T_in <= 0 || T_out <= 0 || V <= 0 || (stride != 1 && stride != 2)) return F3_EINVAL;
  if (epi != 0 && epi != EPI_BIAS && epi != (EPI_BIAS | EPI_STATS) && epi != (EPI_BIASV | EPI_STATS) && epi != EPI_ADD)
    return F3_EINVAL;
  if (transposed ? (T_in != (T_out - 1) / stride + 1) : (T_out != (T_in - 1) / stride + 1)) return F3_EINVAL;
  if ((epi & EPI_ADD) && out_bf16) return F3_EINVAL;
  if ((epi & EPI_STATS) && (!st_sum || !st_sq)) return F3_EINVAL;
  if ((epi & (EPI_BIAS | EPI_BIASV)) && !bias) return F3_EINVAL;
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_out * V, Cout, Cin, 1, stride, 0, transposed, T_out, T_in, V, Cin, Cout);
  a.inb = (const unsigned short*)x;
  a.wb = (const unsigned short*)wpack;
  a.zero = test_zero_page();
  if (out_bf16) a.outb = (unsigned short*)out;
  else a.out = (float*)out;
  a.bias = bias; a.st_sum = st_sum; a.st_sq = st_sq;
  if (!f3_igemm_ok(a)) return F3_EINVAL;
  return f3_igemm_bf16(&a, epi, (hipStream_t)stream);
}

// ---- bf16x3 on the bf16 kernels, as the step launches them ([hi | lo] operand rows, native form) ----
int f3_split_x3cat(const float* x, void* out, int64_t rows, int C, void* stream) {
  if (!x || !out || rows < 0 || C <= 0 || C % 4) return F3_EINVAL;
  return f3_split_x3(x, static_cast<unsigned short*>(out), rows, C, (hipStream_t)stream);
}

static bool x3cat_shape_ok(int N, int T_in, int V, int Cin, int Cout, int KT, int stride, int pad) {
  return N > 0 && T_in > 0 && V > 0 && Cin > 0 && Cout > 0 && KT > 0 && (stride == 1 || stride == 2) && pad >= 0 &&
         (T_in + 2 * pad - KT) / stride + 1 > 0 && Cin % 8 == 0 && Cout % 8 == 0;
}

int f3_conv_forward_x3cat(const void* x3, const float* w, const float* bias, float* out, void* wpack, int N, int T_in,
                          int V, int Cin, int Cout, int KT, int stride, int pad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!x3 || !bias || !out || !wpack || !x3cat_shape_ok(N, T_in, V, Cin, Cout, KT, stride, pad)) return F3_EINVAL;
  if (w) {  // the step's packing (native [W_hi 32 | W_lo 32] blocks; w == NULL: wpack already packed)
    PrepTable t;
    t.n = 0;
    add_job(t, PREP_PACK_CONV, Cout * KT * Cin * x3mul(x3code()), static_cast<float*>(wpack), w, nullptr, nullptr,
            Cout, Cin, KT, x3code());
    F3_TRY(f3_prep(t, s));
  }
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_out * V, Cout, Cin, KT, stride, pad, 0, T_out, T_in, V, 2 * Cin, Cout);
  x3_gemm(a, Cin);
  a.inb = static_cast<const unsigned short*>(x3); a.zero = test_zero_page();
  a.wb = static_cast<const unsigned short*>(wpack); a.out = out; a.bias = bias;
  if (!f3_igemm_ok(a)) return F3_EINVAL;
  return f3_conv_gemm(&a, 0, EPI_BIAS, s);
}

int f3_conv_backward_data_x3cat(const void* dy3, const float* w, float* dx, void* wpack, int N, int T_in, int V,
                                int Cin, int Cout, int KT, int stride, int pad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!dy3 || !dx || !wpack || !x3cat_shape_ok(N, T_in, V, Cin, Cout, KT, stride, pad)) return F3_EINVAL;
  if (w) {  // the transposed packing, as the step's
    PrepTable t;
    t.n = 0;
    add_job(t, PREP_PACK_CONV_T, Cout * KT * Cin * x3mul(x3code()), static_cast<float*>(wpack), w, nullptr, nullptr,
            Cout, Cin, KT, x3code());
    F3_TRY(f3_prep(t, s));
  }
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_in * V, Cin, Cout, KT, stride, pad, 1, T_in, T_out, V, 2 * Cout, Cin);
  x3_gemm(a, Cout);
  a.inb = static_cast<const unsigned short*>(dy3); a.zero = test_zero_page();
  a.wb = static_cast<const unsigned short*>(wpack); a.out = dx;
  if (!f3_igemm_ok(a)) return F3_EINVAL;
  return f3_conv_gemm(&a, 0, 0, s);
}

int f3_conv_step_x3cat(int kind, const void* in3, const float* w, void* wpack, float* out, const float* bias_v,
                       const float* g, const float* gamma, const float* beta, const double* bn_sum,
                       const double* bn_sq, float bn_count, double* st_sum, double* st_sq, int N, int T, int V,
                       int Cin, int Cout, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool gcn = kind == F3_STEP_GCN_FWD, dgrad = kind == F3_STEP_TCN_DGRAD;
  if ((!gcn && !dgrad) || !in3 || !wpack || !out || !st_sum || !st_sq) return F3_EINVAL;
  if (gcn && !bias_v) return F3_EINVAL;
  if (dgrad && (!g || !gamma || !beta || !bn_sum || !bn_sq || bn_count <= 0.f)) return F3_EINVAL;
  const int KT = gcn ? 1 : 9, pad = gcn ? 0 : 4;
  if (!x3cat_shape_ok(N, T, V, Cin, Cout, KT, 1, pad)) return F3_EINVAL;
  if (w) {  // the step's packing (w == NULL: wpack already packed)
    PrepTable t;
    t.n = 0;
    add_job(t, gcn ? PREP_PACK_CONV : PREP_PACK_CONV_T, Cout * KT * Cin * x3mul(x3code()), static_cast<float*>(wpack),
            w, nullptr, nullptr, Cout, Cin, KT, x3code());
    F3_TRY(f3_prep(t, s));
  }
  ConvGemmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.inb = static_cast<const unsigned short*>(in3); a.zero = test_zero_page();
  a.wb = static_cast<const unsigned short*>(wpack); a.out = out; a.st_sum = st_sum; a.st_sq = st_sq;
  if (gcn) {  // layer_forward's gcn GEMM: [Z_hi | Z_lo] rows of K Ci channels, graph-mixed bias, BN1 sums
    a.g = geom(N * T * V, Cout, Cin, 1, 1, 0, 0, T, T, V, Cin, Cout);
    x3_gemm(a, Cin);
    a.bias = bias_v;
    if (!f3_igemm_ok(a)) return F3_EINVAL;
    return f3_conv_gemm(&a, 0, EPI_BIASV | EPI_STATS, s);
  }
  // layer_backward_main's tcn input gradient: dh rows [hi | lo] of Cout channels (the tcn's output) into
  // dv[M][Cin]; ReLU mask of bn1(g) and the BN1-backward sums in the epilogue (RELUMASK)
  a.g = geom(N * T * V, Cin, Cout, KT, 1, pad, 1, T, T, V, Cout, Cin);
  x3_gemm(a, Cout);
  a.aux = g; a.ldaux = Cin;
  a.epi_bn.sum = bn_sum; a.epi_bn.sumsq = bn_sq; a.epi_bn.gamma = gamma; a.epi_bn.beta = beta;
  a.epi_bn.count = bn_count; a.epi_bn.eval = 0;
  if (!f3_igemm_ok(a)) return F3_EINVAL;
  return f3_conv_gemm(&a, 0, EPI_RELUMASK, s);
}

int f3_conv_backward_weight_x3cat(const void* dy3, const void* x3, float* dw, float* db, int N, int T_in, int V,
                                  int Cin, int Cout, int KT, int stride, int pad, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!dy3 || !x3 || !x3cat_shape_ok(N, T_in, V, Cin, Cout, KT, stride, pad)) return F3_EINVAL;
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  const long long cap = kWgradSlabFloats * 4;  // the step's x3 slab (plan: W.slab)
  float* slab = test_scratch((size_t)cap + 2 * Cout);
  if (!slab) return F3_EHIP;
  WgradArgs a;
  std::memset(&a, 0, sizeof(a));
  a.ldy = 2 * Cout; a.outmap = WG_OUT_CONV; a.bf16 = 1;
  a.dyb = static_cast<const unsigned short*>(dy3); a.inb = static_cast<const unsigned short*>(x3);
  a.zero = test_zero_page(); a.slab = slab; a.slab_cap = cap;
  a.g = geom(N * T_out * V, Cout, Cin, KT, stride, pad, 0, T_out, T_in, V, 2 * Cin, Cout);
  a.x3seg = 1;
  if (dw) {  // dw == NULL: the GEMM alone (partials left in the slab)
    if (hipMemsetAsync(dw, 0, sizeof(float) * Cout * Cin * KT, s) != hipSuccess) return F3_EHIP;
    a.dw_ref = dw;
    if (db) {
      if (hipMemsetAsync(db, 0, sizeof(float) * Cout, s) != hipSuccess) return F3_EHIP;
      a.db = db;
    }
  }
  if (!f3_wgrad_glds_ok(a)) return F3_EINVAL;
  return f3_conv_wgrad(&a, 0, s);
}

int f3_conv_backward_weight(const void* dy, const void* x, float* dw, float* db, int N, int T_in, int V, int Cin,
                            int Cout, int KT, int stride, int pad, int precision, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (precision < 0 || (precision > 2 && precision != F3_PRECISION_BF16X3)) return F3_EINVAL;
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  if (hipMemsetAsync(dw, 0, sizeof(float) * Cout * Cin * KT, s) != hipSuccess) return F3_EHIP;
  if (db && hipMemsetAsync(db, 0, sizeof(float) * Cout, s) != hipSuccess) return F3_EHIP;
  WgradArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_out * V, Cout, Cin, KT, stride, pad, 0, T_out, T_in, V, Cin, Cout);
  a.ldy = Cout; a.dw = dw; a.db = db; a.outmap = WG_OUT_CONV;
  a.x3 = precision == F3_PRECISION_BF16X3;
  a.bf16 = precision != F3_PRECISION_FP32 && !a.x3;
  if (precision == F3_PRECISION_BF16) {
    a.dyb = (const unsigned short*)dy;
    a.inb = (const unsigned short*)x;
    a.zero = test_zero_page();
    if (f3_wgrad_glds_ok(a)) {  // split partials in a scratch slab, summed into dw (the step's path)
      const long long cap = kWgradSlabFloats;
      float* slab = test_scratch((size_t)cap);
      if (!slab) return F3_EHIP;
      a.slab = slab; a.slab_cap = cap; a.dw_ref = dw;
      return f3_conv_wgrad(&a, 0, s);
    }
  } else {
    a.dy = (const float*)dy;
    a.in = (const float*)x;
  }
  return f3_conv_wgrad(&a, 0, s);
}

int f3_conv_wgrad_packed(const void* dy, const void* x, float* slab, long long slab_floats, int N, int T_in, int V,
                         int Cin, int Cout, int KT, int stride, int pad, void* stream) {
  if (!dy || !x || !slab || N < 1) return F3_EINVAL;
  const int T_out = (T_in + 2 * pad - KT) / stride + 1;
  WgradArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = geom(N * T_out * V, Cout, Cin, KT, stride, pad, 0, T_out, T_in, V, Cin, Cout);
  a.ldy = Cout; a.dw = nullptr; a.db = nullptr; a.outmap = WG_OUT_CONV; a.bf16 = 1;
  a.slab = slab; a.slab_cap = slab_floats; a.dw_ref = nullptr;  // the kernel alone: partials stay in the slab
  a.dyb = (const unsigned short*)dy; a.inb = (const unsigned short*)x; a.zero = test_zero_page();
  if (!f3_wgrad_glds_ok(a)) return F3_EINVAL;
  return f3_conv_wgrad(&a, 0, (hipStream_t)stream);
}

int f3_graph_mix_forward(const float* A_eff, const float* x, float* z, int frames, int K, int V, int Cin,
                         void* stream) {
  MixArgs m;
  std::memset(&m, 0, sizeof(m));
  m.K = K; m.V = V; m.Cin = Cin; m.frames = frames; m.A = A_eff; m.x = x; m.z = z;
  return f3_mix_fwd(&m, (hipStream_t)stream);
}

int f3_graph_mix_backward(const float* A_eff, const float* x, const float* dz, float* dx, float* dA, int frames, int K,
                          int V, int Cin, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(dA, 0, sizeof(float) * K * V * V, s) != hipSuccess) return F3_EHIP;
  MixArgs m;
  std::memset(&m, 0, sizeof(m));
  m.K = K; m.V = V; m.Cin = Cin; m.frames = frames; m.A = A_eff; m.x = x; m.z = const_cast<float*>(dz);
  m.dx = dx; m.dA = dA; m.accumulate = 0;
  static float* part = nullptr;  // test entry only: scratch kept for the process lifetime
  if (!part && hipMalloc(&part, sizeof(float) * kMixParts * 1024) != hipSuccess) return F3_EHIP;
  m.part = part;
  return f3_mix_bwd(&m, s);
}

int f3_graph_mix_forward_ex(const float* A_eff, const void* x, void* z, int frames, int K, int V, int Cin, int flags,
                            void* stream) {
  if (!A_eff || !x || !z || frames < 0 || (flags & ~15) || ((flags & F3_MIX_X3) && (flags & 3))) return F3_EINVAL;
  if ((flags & F3_MIX_Z3) && !(flags & F3_MIX_X3)) return F3_EINVAL;
  MixArgs m;
  std::memset(&m, 0, sizeof(m));
  m.K = K; m.V = V; m.Cin = Cin; m.frames = frames; m.A = A_eff;
  m.x = static_cast<const float*>(x); m.x16 = flags & F3_MIX_X_BF16; m.x3 = (flags & F3_MIX_X3) != 0;
  m.z = static_cast<float*>(z);
  if (flags & F3_MIX_Z_BF16) m.zb = static_cast<unsigned short*>(z);
  if (flags & F3_MIX_Z3) m.z3 = static_cast<unsigned short*>(z);
  return f3_mix_fwd(&m, (hipStream_t)stream);
}

int f3_graph_mix_backward_ex(const float* A_eff, const void* x, const void* dz, float* dx, float* dA, int frames, int K,
                             int V, int Cin, int flags, void* stream) {
  if (!A_eff || !x || !dz || !dx || !dA || frames < 0 || (flags & ~5) || ((flags & F3_MIX_X3) && (flags & 1)))
    return F3_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(dA, 0, sizeof(float) * K * V * V, s) != hipSuccess) return F3_EHIP;
  MixArgs m;
  std::memset(&m, 0, sizeof(m));
  m.K = K; m.V = V; m.Cin = Cin; m.frames = frames; m.A = A_eff; m.x = static_cast<const float*>(x);
  m.dx = dx; m.dA = dA; m.accumulate = 0; m.x3 = (flags & F3_MIX_X3) != 0;
  if (flags & F3_MIX_X_BF16) {
    m.x16 = 1;
    m.dzb = static_cast<const unsigned short*>(dz);
  } else {
    m.z = const_cast<float*>(static_cast<const float*>(dz));
  }
  static float* part = nullptr;  // test entry only: scratch kept for the process lifetime
  if (!part && hipMalloc(&part, sizeof(float) * kMixParts * 1024) != hipSuccess) return F3_EHIP;
  m.part = part;
  return f3_mix_bwd(&m, s);
}

int f3_gcn_dgrad_mix_x3(const void* dg3, const float* w, void* wpack, const float* A_eff, const float* x, float* dx,
                        float* dA, int frames, int K, int V, int Cin, int C, int accumulate, int max_workgroups,
                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!dg3 || !wpack || !A_eff || !x || !dx || !dA || frames < 0 || max_workgroups < 0) return F3_EINVAL;
  if (!f3_gcn_dgrad_mix_ok(K, V, Cin, C) || K * V * V > 1024) return F3_EINVAL;  // (the scratch rows below)
  if (w) {  // the step's transposed packing of w [C][K Cin] (w == NULL: wpack already packed)
    PrepTable t;
    t.n = 0;
    add_job(t, PREP_PACK_CONV_T, C * K * Cin * x3mul(x3code()), static_cast<float*>(wpack), w, nullptr, nullptr, C,
            K * Cin, 1, x3code());
    F3_TRY(f3_prep(t, s));
  }
  if (hipMemsetAsync(dA, 0, sizeof(float) * K * V * V, s) != hipSuccess) return F3_EHIP;
  static float* part = nullptr;  // test entry only: scratch kept for the process lifetime
  if (!part && hipMalloc(&part, sizeof(float) * kMixParts * 1024) != hipSuccess) return F3_EHIP;
  GcnDgradMixArgs a;
  std::memset(&a, 0, sizeof(a));
  a.frames = frames; a.K = K; a.V = V; a.Cin = Cin; a.C = C; a.dg = static_cast<const unsigned short*>(dg3);
  a.w = static_cast<const unsigned short*>(wpack); a.A = A_eff; a.x = x; a.dx = dx; a.dA = dA;
  a.accumulate = accumulate != 0; a.part = part; a.max_workgroups = max_workgroups;
  return f3_gcn_dgrad_mix(&a, s);
}

int f3_gcn_fwd_mix_x3(const float* A_eff, const float* x, const float* w, void* wpack, const float* bias_v, void* z3,
                      float* g, double* st_sum, double* st_sq, int frames, int K, int V, int Cin, int C,
                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!A_eff || !x || !wpack || !bias_v || !z3 || !g || !st_sum || !st_sq || frames < 0) return F3_EINVAL;
  if (!f3_gcn_fwd_mix_ok(K, V, Cin, C)) return F3_EINVAL;
  if (w) {  // the step's packing of w [C][K Cin] (w == NULL: wpack already packed)
    PrepTable t;
    t.n = 0;
    add_job(t, PREP_PACK_CONV, C * K * Cin * x3mul(x3code()), static_cast<float*>(wpack), w, nullptr, nullptr, C,
            K * Cin, 1, x3code());
    F3_TRY(f3_prep(t, s));
  }
  GcnFwdMixArgs a;
  std::memset(&a, 0, sizeof(a));
  a.frames = frames; a.K = K; a.V = V; a.Cin = Cin; a.C = C; a.A = A_eff; a.x = x;
  a.z3 = static_cast<unsigned short*>(z3); a.w = static_cast<const unsigned short*>(wpack); a.bias = bias_v; a.g = g;
  a.st_sum = st_sum; a.st_sq = st_sq; a.zero = test_zero_page();
  return f3_gcn_fwd_mix(&a, s);
}

int f3_block_signs_case(int phases, const void* h, const void* r, const void* x, const float* att, const float* e,
                        const float* bn2, const float* bnr, const double* bn2_b, const double* bnr_b,
                        const float* dout, const float* dout_nc, void* out, void* signs, long long sign_words,
                        float* part, void* dh, void* dres, float* dbpart, float* dgb, int N, int TV, int C,
                        int res_kind, int act16, int x3, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (N <= 0 || TV <= 0 || C < 4 || C % 4 || C > 256 || 256 % (C / 4)) return F3_EINVAL;
  if (res_kind < RES_NONE || res_kind > RES_CONV || (act16 && x3)) return F3_EINVAL;
  if (!h || !att || !bn2 || !out || (res_kind == RES_CONV && (!r || !bnr)) || (res_kind == RES_ID && !x)) return F3_EINVAL;
  if (signs && sign_words < f3_block_sign_words(N, TV, C)) return F3_EINVAL;
  BlockArgs a;
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.TV = TV; a.C = C; a.res_kind = res_kind; a.inv_tv = 1.f / (float)TV; a.act16 = act16;
  // BN rows [gamma | beta | mean | var] of C: the running-statistics form, so the caller owns every input
  a.bn2.gamma = bn2; a.bn2.beta = bn2 + C; a.bn2.rmean = bn2 + 2 * C; a.bn2.rvar = bn2 + 3 * C;
  a.bn2.count = (float)N * (float)TV; a.bn2.eval = 1;
  if (res_kind == RES_CONV) {
    a.bnr = a.bn2;
    a.bnr.gamma = bnr; a.bnr.beta = bnr + C; a.bnr.rmean = bnr + 2 * C; a.bnr.rvar = bnr + 3 * C;
  }
  a.h = static_cast<const float*>(h); a.r = static_cast<const float*>(r); a.x = static_cast<const float*>(x);
  a.att = att; a.out = static_cast<float*>(out); a.signs = static_cast<unsigned short*>(signs);
  if (phases & 1) F3_TRY(f3_block_out(a, s));
  if (!(phases & 2)) return F3_OK;
  if (!e || !bn2_b || !part || !dh || !dgb || (!dout && !dout_nc) || (res_kind == RES_CONV && !bnr_b) ||
      (res_kind != RES_NONE && !dres))
    return F3_EINVAL;
  a.dout = dout_nc ? nullptr : dout; a.dout_nc = dout_nc; a.e = e;
  a.bn2_bsum = bn2_b; a.bn2_bsq = bn2_b + C;
  if (res_kind == RES_CONV) {
    a.bnr_bsum = const_cast<double*>(bnr_b); a.bnr_bsq = const_cast<double*>(bnr_b) + C;  // (read only here)
  }
  a.dgamma2 = dgb; a.dbeta2 = dgb + C; a.dgammar = dgb + 2 * C; a.dbetar = dgb + 3 * C;
  a.part = part; a.no_colsum = 1;  // the P1 / P2 / Q2 partial rows stay in part [chunks][3][N][C]
  a.dh = static_cast<float*>(dh);
  a.dres = static_cast<float*>(dres);
  const bool gemm_rows = act16 || x3;  // dh / dres as the step's GEMM operands: bf16, or [hi | lo] rows
  a.dhb = gemm_rows ? static_cast<unsigned short*>(dh) : nullptr;
  a.dresb = gemm_rows && res_kind == RES_CONV ? static_cast<unsigned short*>(dres) : nullptr;
  a.x3 = x3;
  F3_TRY(f3_block_bwd_reduce(a, s));
  a.no_colsum = 0;
  a.dbpart = dbpart;
  return f3_block_bwd_apply(a, s);
}

}  // extern "C"
