// Host-side helpers shared by the step (net.cpp) and the kernel-level entries (kernel_entries.cpp):
// argument-block builders and the packed-operand conventions. Included by .cpp files only.
#pragma once
#include <algorithm>

#include "kernels.h"
#include "layers.h"

namespace f3 {

inline ConvGeom geom(int M, int Nc, int Kc, int KT, int S, int P, int tr, int T_out, int T_in, int V, int lda,
                     int ldo) {
  ConvGeom g;
  g.M = M; g.Nc = Nc; g.Kc = Kc; g.KT = KT; g.S = S; g.P = P; g.transposed = tr;
  g.T_out = T_out; g.T_in = T_in; g.V = V; g.lda = lda; g.ldo = ldo;
  return g;
}

inline void add_job(PrepTable& t, int type, int n, float* dst, const float* s0, const float* s1, const float* s2,
                    int d0, int d1, int d2, int bf16 = 0) {
  PrepJob& j = t.jobs[t.n++];
  j.type = type; j.n = n; j.dst = dst; j.s0 = s0; j.s1 = s1; j.s2 = s2; j.d0 = d0; j.d1 = d1; j.d2 = d2;
  j.bf16 = bf16;
}

// slab capacity: one round of resident 128x128 weight-gradient tiles (2 per CU x 256 CUs), or 16
// splits of the 256 x 256 x 9 tcn weight (wgrad_taps: 16 tiles x 16 splits = one workgroup per
// CU); the launchers cap the split count to it
// capacity of a stream's weight-gradient split-K slab (floats; the bf16x3 launches use 4x this)
constexpr long long kWgradSlabFloats = std::max(512LL * 128 * 128, 16LL * 256 * 256 * 9);

// bf16 view of a packed operand (the fp32-sized slot holds the bf16 copy in bf16 mode)
inline const unsigned short* bf(const float* p, int on) { return on ? reinterpret_cast<const unsigned short*>(p) : nullptr; }
// bf16 view of an activation slot (bf16 mode stores GEMM operand tensors as bf16)
inline unsigned short* bfa(float* p, int on) { return on ? reinterpret_cast<unsigned short*>(p) : nullptr; }

// bf16x3 mode (F3_PRECISION_BF16X3, the default): fp32 activations as in the fp32 mode; GEMM operands
// as bf16 rows [x_hi | x_lo] written by their producers and weights packed per tap in 32-channel
// blocks [W_hi | W_lo] (prep code 4), three bf16 MFMA products per block (x3_gemm below).
// bf16x3 GEMMs on the bf16 kernels in the native form (ConvGemmArgs::x3n, prep code 4: [x_hi | x_lo]
// rows staged once, three MFMAs per 32-channel block). The round-4 K-concatenated form (Kc = 3C,
// [W_hi | W_hi | W_lo], the third K segment re-staging x_hi) measured 8 % slower per step (9.97-10.02
// vs 9.11-9.12 ms, profiles/r05_x3n_ab.txt) and is gone.
constexpr int x3code() { return 4; }
// packed size (bf16 elements) of n weights in a prep code
inline int x3mul(int code) { return code == 4 ? 2 : 1; }
// set a bf16x3 GEMM on [hi | lo] rows of C channels (lda 2C)
inline void x3_gemm(ConvGemmArgs& a, int C) {
  a.x3n = 1;
  a.g.lda = 2 * C;
}

}  // namespace f3
