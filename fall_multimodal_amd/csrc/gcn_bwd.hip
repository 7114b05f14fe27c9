// gcn input gradient fused into the graph-mix backward of the bf16x3 mode: dZ never reaches HBM.
//
// Per frame f (V joints), for one 64-channel chunk j of Cin and all K taps:
//   dZ_f[w][k][ci] = sum_c dg_f[w][c] W[c][k Cin + ci]        (bf16x3: W_lo dg_hi + W_hi dg_lo + W_hi dg_hi)
//   dx_f[v][ci] (+)= sum_{w,k} A~[k][v][w] dZ_f[w][k][ci]      (both operands split, as mix_bwd_x3)
//   dA[k][v][w]  += sum_{f,ci} x_f[v][ci] dZ_f[w][k][ci]       (per-workgroup partial row, summed by f3_colsum)
// which is what pw_gemm<EPI 0> + mix_bwd_x3_kernel computed through an fp32 dZ [frames][V][K][Cin] in
// HBM (written once, read once: 2 x frames V K Cin 4 bytes per layer).
//
// Workgroup = one channel chunk j, frames slot, slot + slots, ... (the Cin / 64 workgroups of a slot
// have adjacent XCD-remapped ids, so a frame's dg rows come from HBM once and from that XCD's L2
// afterwards). The chunk's weight slice W[0..C)[k Cin + 64 j + 0..64) stays in registers for the whole
// launch as MFMA A fragments, read from the step's packed transposed weight (prep code 4: row
// k Cin + ci, 32-channel blocks [hi 32 | lo 32]). The GEMM is issued transposed (A = W^T, B = dg^T), so
// a lane ends up with 4 consecutive channels of one dZ row: one split4_store into the hi / lo bf16
// planes that mix_bwd_x3_kernel's dX (transposed LDS reads) and dA (16-B reads) stages read, unchanged.
//
// Same bits as the pair where the step uses it (Cin = 64): dZ by pw_gemm's MFMA chain
// per element (C <= 128), dx by mix_bwd_x3's schedule, dA with the mix backward's frame-to-row map
// (GcnDgradMixArgs::max_workgroups) and a single channel chunk.
//
// C = 64 / 128: 4 waves; wave q holds columns 16 q .. 16 q + 15 of every tap over all of C (48 / 96
// VGPRs) and computes both 16-row tiles of the frame. C = 256: 8 waves in two groups g that each hold
// one half of C (96 VGPRs instead of 192, two waves per SIMD instead of one); a wave gives the tile
// row it does not own to its partner through LDS (fp32) and adds the partner's half to its own tile
// row mt = g before the split, then computes dX / dA of v tile g.
//
// LDS (bytes), RB = 144 (64 channels + 16), GB = 4 C + 16:
//   xh, xl  [32][RB]   x_f chunk, hi / lo            2 x 4608
//   zh, zl  [64][RB]   dZ_f rows wk = w K + k        2 x 9216  (rows K V .. 63 stay zero)
//   gs      [32][GB]   dg_f rows [hi | lo]           8704 / 16896 / 33280   (C = 64 / 128 / 256)
//   dxs     [32][68] fp32, aliased on gs: the frame's dX tile, so dx leaves (and its old rows arrive,
//           identity residual) as 16-B pieces in x's own piece order.
//   red     [8][3][64] x 16 B (C = 256): the exchanged half sums    24576
//   afr     [2][2][2][64] x 16 B (C = 64): A~ hi / lo MFMA fragments  8192
// The next frame's x and dg pieces and this frame's old dx rows are in registers while the frame's
// MFMAs run. One workgroup writes each dx element; two runs are bit-identical.
#include "igemm.h"
#include "layers.h"

#include <algorithm>
#include <cstring>

namespace f3 {

typedef __bf16 gb_bf16x4 __attribute__((ext_vector_type(4)));
typedef short gb_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const char gb_lds_t;

F3_DEV void gb_a_split(float t, __bf16& hi, __bf16& lo) {  // hi = top 16 bits, lo = the rest rounded
  const float h = __uint_as_float(__float_as_uint(t) & 0xffff0000u);
  hi = __builtin_bit_cast(__bf16, (unsigned short)(__float_as_uint(h) >> 16));
  lo = (__bf16)(t - h);
}

F3_DEV void gb_split4_store(const f32x4 v, char* hi, char* lo) {  // hi = RNE bf16, lo = RNE bf16 of the rest
  gb_bf16x4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (__bf16)v[e];
    l[e] = (__bf16)(v[e] - (float)h[e]);
  }
  *reinterpret_cast<gb_bf16x4*>(hi) = h;
  *reinterpret_cast<gb_bf16x4*>(lo) = l;
}

F3_DEV f32x4 gb_mfma_x3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = mfma_bf16x(al, bh, c);
  c = mfma_bf16x(ah, bl, c);
  return mfma_bf16x(ah, bh, c);
}

// the gcn GEMM's three products in pw_gemm's order (hi hi, then dg_lo W_hi, then dg_hi W_lo, per
// 32-channel block ascending): the same MFMA chain per element, so dZ is the pair's bit for bit
F3_DEV f32x4 gb_mfma_dz(bf16x8 wh, bf16x8 wl, bf16x8 gh, bf16x8 gl, f32x4 c) {
  c = mfma_bf16x(wh, gh, c);
  c = mfma_bf16x(wh, gl, c);
  return mfma_bf16x(wl, gh, c);
}

// Workgroup barrier of the frame loop: LDS traffic only. (__syncthreads() also waits vmcnt(0), i.e. for
// the next frame's prefetch issued just before: every frame then cost a global round trip.)
F3_DEV void gb_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

constexpr int kGbRB = 144, kGbXR = 32, kGbZR = 64, kGbKmax = 3, kGbDxLd = 68;
constexpr int gb_groups(int C) { return C == 256 ? 2 : 1; }  // wave groups sharing the C reduction
constexpr int gb_threads(int C) { return 256 * gb_groups(C); }

template <int C, bool ACC>
__global__ __launch_bounds__(gb_threads(C)) __attribute__((amdgpu_waves_per_eu(C == 64 ? 3 : 1)))
void gcn_dgrad_mix_x3_kernel(GcnDgradMixArgs a) {
  constexpr int RB = kGbRB, GB = 4 * C + 16, G16 = C / 4;  // G16: 16-B pieces of a dg row
  constexpr int NG = gb_groups(C), NT = gb_threads(C);
  constexpr bool ALDS = C == 64;  // A~ fragments in LDS instead of registers
  constexpr int KSL = C / 32 / NG;  // 32-channel blocks of C per wave
  constexpr int MTL = 2 / NG;       // 16-row tiles a wave finishes (dZ split, dX, dA)
  constexpr int PX = 512 / NT, PG = 8 * C / NT;  // pieces per thread: 32 rows x 16 (x, dx), 32 rows x G16 (dg)
  extern __shared__ __attribute__((aligned(16))) char smb[];
  char* xh = smb;
  char* xl = xh + kGbXR * RB;
  char* zh = xl + kGbXR * RB;
  char* zl = zh + kGbZR * RB;
  char* gs = zl + kGbZR * RB;
  float* dxs = reinterpret_cast<float*>(gs);
  f32x4* red = reinterpret_cast<f32x4*>(gs + kGbXR * GB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int wq = wave & 3, g = NG == 2 ? wave >> 2 : 0;
  const int fr = lane & 15, fg = lane >> 4;
  const int K = a.K, V = a.V, KV = K * V, Cin = a.Cin;
  const int nch = Cin >> 6;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int slot = lin / nch, j = lin - slot * nch, slots = gridDim.x / nch;
  const int nx = V * 16, ng = V * G16;
  const bool two = V > 16;

  // this wave's weight columns n = k Cin + 64 j + 16 wq + fr as MFMA A fragments (rows n, k-dim: its
  // group's blocks of c)
  bf16x8 wh[kGbKmax][KSL], wl[kGbKmax][KSL];
#pragma unroll
  for (int k = 0; k < kGbKmax; ++k)
#pragma unroll
    for (int ks = 0; ks < KSL; ++ks) {
      // (taps k >= K repeat tap K - 1 and are never used: no branch around the loads)
      const __bf16* row =
          reinterpret_cast<const __bf16*>(a.w) + ((size_t)min(k, K - 1) * Cin + 64 * j + 16 * wq + fr) * 2 * C;
      wh[k][ks] = *reinterpret_cast<const bf16x8*>(row + 64 * (g * KSL + ks) + 8 * fg);
      wl[k][ks] = *reinterpret_cast<const bf16x8*>(row + 64 * (g * KSL + ks) + 32 + 8 * fg);
    }
  // A_eff through LDS: one coalesced pass instead of 32 per-lane loads behind their bounds checks
  {
    float* At = reinterpret_cast<float*>(zh);  // K V V <= 64 x 32 floats, inside the z planes
    for (int e = tid; e < KV * V; e += NT) At[e] = a.A[e];
    gb_barrier();
  }
  // A~ as the dX A operand: rows v = 16 mt + fr, k = wk = 32 ks + 8 fg + e (mt = g with two groups)
  bf16x8 ahi[MTL][2], alo[MTL][2];
#pragma unroll
  for (int ml = 0; ml < MTL; ++ml)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 h, l;
        const int wk = 32 * ks + 8 * fg + e, v = 16 * (NG == 2 ? g : ml) + fr;
        const int w = wk / K, k = wk - w * K;
        const bool in = wk < KV && v < V;
        const float t = reinterpret_cast<const float*>(zh)[in ? (k * V + v) * V + w : 0];
        gb_a_split(in ? t : 0.f, h, l);
        ahi[ml][ks][e] = h;
        alo[ml][ks][e] = l;
      }
  // C = 64: the fragments wait in LDS (every wave's are the same) and are re-read per frame, which
  // takes the kernel to 168 VGPRs: three workgroups per CU, so mix_bwd_x3's 768 rows are one round
  bf16x8* afr = reinterpret_cast<bf16x8*>(gs + kGbXR * GB);  // [hi, lo][MTL][2][64 lanes]
  if constexpr (ALDS) {
    if (wave == 0) {
#pragma unroll
      for (int ml = 0; ml < MTL; ++ml)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          afr[(ml * 2 + ks) * 64 + lane] = ahi[ml][ks];
          afr[(MTL * 2 + ml * 2 + ks) * 64 + lane] = alo[ml][ks];
        }
    }
  }
  gb_barrier();  // A_eff's image is read; the z planes are zeroed and filled next
  // zero once: dZ rows K V .. 63 (they meet A~'s zero columns), x rows V .. 31 (dA rows never stored),
  // dg rows V .. 31 (dZ rows never stored): no uninitialised LDS reaches an MFMA
  for (int o = KV * RB + tid * 16; o < kGbZR * RB; o += NT * 16) {
    *reinterpret_cast<f32x4*>(zh + o) = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(zl + o) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int o = V * RB + tid * 16; o < kGbXR * RB; o += NT * 16) {
    *reinterpret_cast<f32x4*>(xh + o) = f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(xl + o) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // (later frames find dxs' rows there: dX rows >= V are exact zeros, and a column w >= V of the
  // transposed GEMM only feeds dZ rows that are not stored)
  for (int o = V * GB + tid * 16; o < kGbXR * GB; o += NT * 16)
    *reinterpret_cast<f32x4*>(gs + o) = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 dacc[MTL];
#pragma unroll
  for (int ml = 0; ml < MTL; ++ml) dacc[ml] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (a second prefetched frame in registers measured the same: 47.6 vs 48.1 us at C = 64, 98 vs 97 at 256)
  f32x4 rx[PX], rg[PG], ro[PX];
  auto prefetch = [&](int f) {  // unconditional, clamped loads
    const float* xg = a.x + (size_t)f * V * Cin + 64 * j;
    const f32x4* gg = reinterpret_cast<const f32x4*>(reinterpret_cast<const __bf16*>(a.dg) + (size_t)f * V * 2 * C);
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int i = min(tid + q * NT, nx - 1);
      rx[q] = *reinterpret_cast<const f32x4*>(xg + (size_t)(i >> 4) * Cin + (i & 15) * 4);
    }
#pragma unroll
    for (int q = 0; q < PG; ++q) rg[q] = gg[min(tid + q * NT, ng - 1)];
  };
  prefetch(slot);  // (slot < frames: the grid has at most frames slots)
  for (int f = slot; f < a.frames; f += slots) {
    gb_barrier();  // the previous frame's reads of the planes and of dxs are done
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int i = tid + q * NT;
      if (i < nx) {
        const int o = (i >> 4) * RB + (i & 15) * 8;
        gb_split4_store(rx[q], xh + o, xl + o);
      }
    }
#pragma unroll
    for (int q = 0; q < PG; ++q) {
      const int i = tid + q * NT;
      if (i < ng) *reinterpret_cast<f32x4*>(gs + (i / G16) * GB + (i % G16) * 16) = rg[q];
    }
    gb_barrier();
    float* dxf = a.dx + (size_t)f * V * Cin + 64 * j;
    if (ACC) {
#pragma unroll
      for (int q = 0; q < PX; ++q) {
        const int i = min(tid + q * NT, nx - 1);
        ro[q] = *reinterpret_cast<const f32x4*>(dxf + (size_t)(i >> 4) * Cin + (i & 15) * 4);
      }
    }
    // (no branch around a global load or store in the loop: behind one, hipcc waits vmcnt(0) at the next
    // use of any load, which made every prefetch a round trip; past the last frame it re-reads it)
    prefetch(min(f + slots, a.frames - 1));
    // dZ^T tiles: rows ci = 16 wq + 4 fg + r, column w = 16 mt + fr, per tap (over this group's part of C)
    f32x4 acc[2][kGbKmax];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int k = 0; k < kGbKmax; ++k) acc[mt][k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (mt == 0 || two) {
#pragma unroll
        for (int ks = 0; ks < KSL; ++ks) {
          const char* p = gs + (16 * mt + fr) * GB + (32 * (g * KSL + ks) + 8 * fg) * 2;
          const bf16x8 gh = *reinterpret_cast<const bf16x8*>(p);
          const bf16x8 gl = *reinterpret_cast<const bf16x8*>(p + 2 * C);
#pragma unroll
          for (int k = 0; k < kGbKmax; ++k)
            if (k < K) acc[mt][k] = gb_mfma_dz(wh[k][ks], wl[k][ks], gh, gl, acc[mt][k]);
        }
      }
    }
    f32x4 fin[MTL][kGbKmax];  // the finished tiles: both (one group) or tile row g with the partner's half added
    if constexpr (NG == 2) {
#pragma unroll
      for (int k = 0; k < kGbKmax; ++k) red[(wave * kGbKmax + k) * 64 + lane] = g ? acc[0][k] : acc[1][k];
      gb_barrier();
#pragma unroll
      for (int k = 0; k < kGbKmax; ++k)
        fin[0][k] = (g ? acc[1][k] : acc[0][k]) + red[((wave ^ 4) * kGbKmax + k) * 64 + lane];
    } else {
#pragma unroll
      for (int ml = 0; ml < MTL; ++ml)
#pragma unroll
        for (int k = 0; k < kGbKmax; ++k) fin[ml][k] = acc[ml][k];
    }
#pragma unroll
    for (int ml = 0; ml < MTL; ++ml)
#pragma unroll
      for (int k = 0; k < kGbKmax; ++k) {
        const int w = 16 * (NG == 2 ? g : ml) + fr;
        if (k < K && w < V) {
          const int o = (w * K + k) * RB + (16 * wq + 4 * fg) * 2;
          gb_split4_store(fin[ml][k], zh + o, zl + o);
        }
      }
    gb_barrier();  // dZ planes complete; gs is free for dxs
    // dX_f[v][c] = sum_wk A~[v][wk] dZ_f[wk][c]: this wave's channel tile 16 wq .. 16 wq + 15
    {
      bf16x8 bh[2], bl[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int o = (32 * ks + 8 * fg + (fr >> 2)) * RB + 32 * wq + 8 * (fr & 3);
        const unsigned ph = (unsigned)(size_t)(gb_lds_t*)(zh + o), pl = (unsigned)(size_t)(gb_lds_t*)(zl + o);
        gb_s16x4 h0, h1, l0, l1;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(h0) : "v"(ph));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(h1) : "v"(ph), "n"(4 * RB));
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(l0) : "v"(pl));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(l1) : "v"(pl), "n"(4 * RB));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(h0), "+v"(h1), "+v"(l0), "+v"(l1)::"memory");
        bh[ks] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7));
        bl[ks] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int ml = 0; ml < MTL; ++ml) {
        f32x4 xa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 ah = ALDS ? afr[(ml * 2 + ks) * 64 + lane] : ahi[ml][ks];
          const bf16x8 al = ALDS ? afr[(MTL * 2 + ml * 2 + ks) * 64 + lane] : alo[ml][ks];
          xa = gb_mfma_x3(ah, al, bh[ks], bl[ks], xa);
        }
        // lane holds v = 16 mt + 4 fg + r, c = 16 wq + fr
        const int mt = NG == 2 ? g : ml;
#pragma unroll
        for (int r = 0; r < 4; ++r) dxs[(16 * mt + 4 * fg + r) * kGbDxLd + 16 * wq + fr] = xa[r];
      }
    }
    // dA[v][wk] += sum_c X_f[v][c] dZ_f[wk][c]: wk tile 16 wq .. 16 wq + 15, this wave's v tiles
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cb = (32 * ks + 8 * fg) * 2;
      const bf16x8 z_h = *reinterpret_cast<const bf16x8*>(zh + (16 * wq + fr) * RB + cb);
      const bf16x8 z_l = *reinterpret_cast<const bf16x8*>(zl + (16 * wq + fr) * RB + cb);
#pragma unroll
      for (int ml = 0; ml < MTL; ++ml) {
        const int mt = NG == 2 ? g : ml;
        const bf16x8 x_h = *reinterpret_cast<const bf16x8*>(xh + (16 * mt + fr) * RB + cb);
        const bf16x8 x_l = *reinterpret_cast<const bf16x8*>(xl + (16 * mt + fr) * RB + cb);
        dacc[ml] = gb_mfma_x3(x_h, x_l, z_h, z_l, dacc[ml]);
      }
    }
    gb_barrier();  // the dX tile is in dxs
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      // pieces past the frame repeat its last piece (the same value to the same address)
      const int i = min(tid + q * NT, nx - 1);
      f32x4 v = *reinterpret_cast<const f32x4*>(dxs + (i >> 4) * kGbDxLd + (i & 15) * 4);
      if (ACC) v += ro[q];
      *reinterpret_cast<f32x4*>(dxf + (size_t)(i >> 4) * Cin + (i & 15) * 4) = v;
    }
  }
  // partial row of dA in the reference layout [k][v][w]: every (v < V, wk < KV) has one owner
  float* row = a.part + (size_t)lin * K * V * V;
#pragma unroll
  for (int ml = 0; ml < MTL; ++ml)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = 16 * (NG == 2 ? g : ml) + 4 * fg + r, wk = 16 * wq + fr;
      if (v < V && wk < KV) {
        const int w = wk / K, k = wk - w * K;
        row[(k * V + v) * V + w] = dacc[ml][r];
      }
    }
}

template <int C>
static size_t gb_lds() {
  return (size_t)2 * (kGbXR + kGbZR) * kGbRB + (size_t)kGbXR * (4 * C + 16) +
         (gb_groups(C) == 2 ? (size_t)8 * kGbKmax * 64 * 16 : 0) + (C == 64 ? (size_t)8 * 64 * 16 : 0);
}

// one round of resident workgroups (occupancy at the kernel's LDS and registers), per C
template <int C>
static int gb_slots() {
  static const int slots = [] {
    int per_cu[2] = {0, 0}, dev = 0, cus = 256;
    const void* fn[2] = {(const void*)gcn_dgrad_mix_x3_kernel<C, false>, (const void*)gcn_dgrad_mix_x3_kernel<C, true>};
    for (int i = 0; i < 2; ++i) {
      (void)hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)gb_lds<C>());
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu[i], fn[i], gb_threads(C), gb_lds<C>()) != hipSuccess ||
          per_cu[i] < 1)
        per_cu[i] = 1;
    }
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipGetLastError();
    return std::min(per_cu[0], per_cu[1]) * cus;
  }();
  return slots;
}

static int gb_grid(const GcnDgradMixArgs* a) {
  const int nch = a->Cin / 64;
  int wgs = a->C == 64 ? gb_slots<64>() : a->C == 128 ? gb_slots<128>() : gb_slots<256>();
  // a caller's count holds whether it is resident or not: it fixes the frame-to-row map, and with it
  // the order in which dA is summed
  wgs = std::min(a->max_workgroups > 0 ? a->max_workgroups : wgs, kMixParts);
  const int slots = std::max(1, std::min(a->frames, wgs / nch));
  return slots * nch;
}

template <int C>
static int gb_launch(const GcnDgradMixArgs* a, int grid, hipStream_t s) {
  if (a->accumulate)
    hipLaunchKernelGGL((gcn_dgrad_mix_x3_kernel<C, true>), dim3(grid), dim3(gb_threads(C)), gb_lds<C>(), s, *a);
  else
    hipLaunchKernelGGL((gcn_dgrad_mix_x3_kernel<C, false>), dim3(grid), dim3(gb_threads(C)), gb_lds<C>(), s, *a);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

}  // namespace f3

using namespace f3;

bool f3_gcn_dgrad_mix_ok(int K, int V, int Cin, int C) {
  const auto ch = [](int c) { return c == 64 || c == 128 || c == 256; };
  return K >= 1 && K <= kGbKmax && V >= 1 && V <= 32 && K * V <= 64 && ch(Cin) && ch(C) && C >= Cin;
}

int f3_gcn_dgrad_mix_parts(const GcnDgradMixArgs* a) {
  if (!f3_gcn_dgrad_mix_ok(a->K, a->V, a->Cin, a->C) || a->frames <= 0) return 0;
  return gb_grid(a);
}

int f3_gcn_dgrad_mix(const GcnDgradMixArgs* a, hipStream_t s) {
  if (!f3_gcn_dgrad_mix_ok(a->K, a->V, a->Cin, a->C)) return F3_EINVAL;
  if (!a->dg || !a->w || !a->A || !a->x || !a->dx || !a->part) return F3_EINVAL;
  if (a->frames <= 0) return F3_OK;
  const int grid = gb_grid(a);
  F3_TRY(a->C == 64 ? gb_launch<64>(a, grid, s) : a->C == 128 ? gb_launch<128>(a, grid, s) : gb_launch<256>(a, grid, s));
  if (a->no_colsum) return F3_OK;
  return f3_colsum(a->part, grid, a->K * a->V * a->V, a->dA, s);
}
