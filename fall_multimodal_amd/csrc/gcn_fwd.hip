// gcn forward of the bf16x3 mode with the graph mix fused into the 1x1 GEMM (Cin = 64, K = 3, C = 64 / 128):
// Z is written once for the weight gradient and never read back.
//
//   Z_f[w][k][ci] = sum_v A~[k][v][w] x_f[v][ci]            (both operands split, as mix_fwd_x3_kernel)
//   g[m][c]       = sum_n Z[m][n] W[c][n] + bias_v[m % V][c]  (m = f V + w, n = k Cin + ci; pw_gemm's X3N chain)
// which is what mix_fwd_x3_kernel<64, true> + pw_gemm_kernel<EPI_BIASV | EPI_STATS, 12, WN, 32, true, true>
// computed through the [Z_hi | Z_lo] rows in HBM (written once, read once).
//
// Same bits as the pair: this is pw_gemm's kernel (weight slices in registers, the same contiguous range of
// 32-row tiles per workgroup, the same MFMA chain per tile, bias table, output image and statistics path)
// with one change: a tile's A block ([6 blocks][32 rows][hi 32 | lo 32], swizzled) is not LDS-DMA'd from the
// Z rows, it is computed into the LDS buffer by the mix kernel's MFMA triple per element (channels as M, wk
// as N, v as k, A~ fragments from atil / a_split in registers, accumulator from zero), split into
// z_hi = RNE bf16(acc), z_lo = RNE bf16(acc - z_hi). The Z rows leave from that buffer as 16-B pieces in the
// layout mix_fwd_x3_kernel<64, true> writes.
//
// The workgroup walks its tiles; before tile t's GEMM it computes the frames not yet done up to the one
// holding the tile's last row. A frame that straddles tiles t and t + 1 is computed once and scattered
// into both buffers (two buffers suffice: V <= 18 < 32 rows); a frame cut by the range boundary is computed
// by both workgroups, each keeping its own rows. x arrives by LDS-DMA as raw fp32 in 32-row blocks aligned
// with the tiles (8 KB: one 1-KB instruction per wave and tile; past the problem, or past the block after the
// range, from the zero page) into a ring of 8 blocks, 7 ahead; a lane reads its fragment elements
// x_f[v = 8 fg + e][c] from the ring and splits them in registers (the values split4_store put into the
// planes). At the end of tile t block t + 2 must have landed (tile t + 1's frames reach into it); the wait
// counts the younger operations exactly: every tile issues its g pieces (but the first), one DMA and three
// Z pieces per thread, unconditionally. The staged pieces (g, Z) are read from LDS with inline asm and their
// own lgkmcnt wait, as in pw_gemm: hipcc would wait vmcnt(0) before a plain read of them.
//
// LDS (bytes), NT = 64 WN:
//   A ring  2 x [6][32][128]          49152
//   x ring  8 x [32][256]             65536
//   image   [32][NT + 4] fp32          8704 / 16896
//   bias    [18][NT] fp32              4608 / 9216
//   red     [2][2][NT] fp32            1024 / 2048      total 129024 / 142848
#include "igemm.h"
#include "layers.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace f3 {

constexpr int GF_THREADS = 512;  // 8 waves: GEMM wm = wave & 1, wj = wave >> 1; mix mt = wave & 3, nh = wave >> 2
constexpr int GF_VMAX = 18, GF_K = 3, GF_CIN = 64, GF_KC = GF_K * GF_CIN;
constexpr int GF_BM = 32, GF_KS = 2 * GF_KC / 32;  // 12 weight slices (hi / lo of 6 blocks)
constexpr int GF_XD = 7, GF_NXB = GF_XD + 1;        // x blocks ahead, ring size
constexpr int GF_RING = GF_BM * GF_NXB;             // ring rows (a power of two)
constexpr int GF_ZP = GF_BM * 4 * GF_KC / 16 / GF_THREADS;  // 16-B Z pieces per thread and tile (3)

template <int WN>
struct GfLds {
  static constexpr int NT = 64 * WN;
  static constexpr int ABUF = GF_BM * GF_KC * 2 * 2;  // [6][32][128]
  static constexpr int OTS = NT + 4;
  static constexpr int X_OFF = 2 * ABUF;
  static constexpr int OT_OFF = X_OFF + GF_RING * GF_CIN * 4;
  static constexpr int BV_OFF = OT_OFF + GF_BM * OTS * 4;
  static constexpr int RED_OFF = BV_OFF + GF_VMAX * NT * 4;
  static constexpr int BYTES = RED_OFF + 2 * 2 * NT * 4;
  static constexpr int PIECES = GF_BM * NT * 4 / 16 / GF_THREADS;  // g pieces per thread and tile
};

typedef __bf16 gf_bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned gf_u32x4 __attribute__((ext_vector_type(4)));

F3_DEV void gf_a_split(float t, __bf16& hi, __bf16& lo) {  // hi = top 16 bits, lo = the rest rounded
  const float h = __uint_as_float(__float_as_uint(t) & 0xffff0000u);
  hi = __builtin_bit_cast(__bf16, (unsigned short)(__float_as_uint(h) >> 16));
  lo = (__bf16)(t - h);
}

F3_DEV float gf_atil(const float* A, int K, int V, int wk, int v) {
  if (wk >= K * V || v >= V) return 0.f;
  const int w = wk / K, k = wk - w * K;
  return A[(k * V + v) * V + w];
}

F3_DEV f32x4 gf_mfma_x3m(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 c) {  // mix_fwd_x3_kernel's order
  c = mfma_bf16x(al, bh, c);
  c = mfma_bf16x(ah, bl, c);
  return mfma_bf16x(ah, bh, c);
}

template <int WN>
__global__ __launch_bounds__(GF_THREADS) void gcn_fwd_mix_x3_kernel(GcnFwdMixArgs a, int per_wg) {
  using L = GfLds<WN>;
  constexpr int NT = L::NT, OTS = L::OTS, KS = GF_KS, K = GF_K, CIN = GF_CIN, PIECES = L::PIECES;
  constexpr int OPS = 1 + GF_ZP + PIECES;                  // vector-memory operations per thread and tile
  constexpr int NSTEADY = GF_ZP + OPS * (GF_XD - 2);       // younger than block t + 2's DMA at the end of tile t
  static_assert(L::BYTES <= 160 * 1024 && NSTEADY < 64 && GF_ZP * GF_THREADS * 16 == L::ABUF, "gcn_fwd LDS / vmcnt");
  static_assert((GF_RING & (GF_RING - 1)) == 0 && PIECES >= 1, "ring");
  extern __shared__ __attribute__((aligned(16))) char gf_smem[];
  char* img = gf_smem + L::OT_OFF;
  float* bv = reinterpret_cast<float*>(gf_smem + L::BV_OFF);
  float* red = reinterpret_cast<float*>(gf_smem + L::RED_OFF);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wj = wave >> 1;   // GEMM: 16-row half, 16 WN columns
  const int mt = wave & 3, nh = wave >> 2;   // mix: channel tile, wk tiles 2 nh, 2 nh + 1
  const int fr = lane & 15, fg = lane >> 4;
  const int V = a.V, KV = K * V, M = a.frames * V;
  const int ntiles = (M + GF_BM - 1) / GF_BM;
  const int range = xcd_remap(blockIdx.x, gridDim.x);
  const int tile0 = range * per_wg, tile1 = min(ntiles, tile0 + per_wg);
  if (tile0 >= tile1) return;

  // x block b (rows 32 b .. 32 b + 31 of x, fp32) -> ring slot (b - (tile0 - 1)) % NXB: wave w rows
  // 4 w .. 4 w + 3, lane = (row, 16-B piece). Always issued; rows outside [0, M) and past the block after
  // the range (the last frame's reach; the ring runs XD blocks ahead) from the zero page.
  const int rbase = (tile0 - 1) * GF_BM;  // x row of ring row 0 (may be -32)
  const int mend = min(M, (tile1 + 1) * GF_BM);
  char* xring = gf_smem + L::X_OFF;
  auto load_block = [&](int b) {
    const int m = b * GF_BM + wave * 4 + (lane >> 4);
    const void* src = (m >= 0 && m < mend) ? (const void*)(a.x + (size_t)m * CIN + (lane & 15) * 4) : (const void*)a.zero;
    char* dst = xring + (((b * GF_BM - rbase) & (GF_RING - 1)) + wave * 4) * (CIN * 4);
    __builtin_amdgcn_global_load_lds(src, (lds_void_t*)dst, 16, 0, 0);
  };
  // Prologue, one round trip: the bias table [V][NT] (contiguous: one column group) and x blocks
  // tile0 - 1 .. tile0 + XD - 1 by LDS-DMA, then the register operands by plain loads; hipcc waits for
  // everything at their first use (it does not count loads and LDS-DMA in order), which is what the first
  // tile needs anyway. The table's last 1-KB piece may run past V NT floats into `red` (written later).
#pragma unroll
  for (int i = 0; i < (GF_VMAX * NT * 4 + 8191) / 8192; ++i) {
    const int o = (wave + 8 * i) * 1024;  // wave-uniform
    if (o < V * NT * 4) {
      const void* src = o + lane * 16 < V * NT * 4 ? (const void*)(reinterpret_cast<const char*>(a.bias) + o + lane * 16)
                                                   : (const void*)a.zero;
      __builtin_amdgcn_global_load_lds(src, (lds_void_t*)(gf_smem + L::BV_OFF + o), 16, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < GF_NXB; ++i) load_block(tile0 - 1 + i);

  // this wave's weight slice (pw_gemm X3N: slice 2b is block b's W_hi, 2b + 1 its W_lo; packed row 2 Kc)
  bf16x8 wf[WN][KS];
#pragma unroll
  for (int y = 0; y < WN; ++y) {
    const unsigned short* wr = a.w + (size_t)(wj * 16 * WN + y * 16 + fr) * (2 * GF_KC) + fg * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) wf[y][s] = *reinterpret_cast<const bf16x8*>(wr + s * 32);
  }
  // A~ as the mix MFMA's B operand: lane holds k = v = 8 fg + e, n = wk = 16 (2 nh + q) + fr
  bf16x8 bhi[2], blo[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      __bf16 h, l;
      gf_a_split(gf_atil(a.A, K, V, 16 * (2 * nh + q) + fr, 8 * fg + e), h, l);
      bhi[q][e] = h;
      blo[q][e] = l;
    }
  float ssum[WN], ssq[WN];
#pragma unroll
  for (int y = 0; y < WN; ++y) ssum[y] = ssq[y] = 0.f;
  // everything issued above has landed; use the loaded registers here, before the loop's DMA
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int y = 0; y < WN; ++y)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(wf[y][s]));
#pragma unroll
  for (int q = 0; q < 2; ++q) asm volatile("" ::"v"(bhi[q]), "v"(blo[q]));
  __builtin_amdgcn_s_barrier();
  const unsigned x_lds = (unsigned)(size_t)(lds_void_t*)xring;
  const unsigned a_lds = (unsigned)(size_t)(lds_void_t*)gf_smem;
  const unsigned img_lds = (unsigned)(size_t)(lds_void_t*)img;

  // frame f: Z_f into the A buffers of the tiles that own its rows (this workgroup's tiles only)
  auto mix_frame = [&](int f) {
    const int rel0 = f * V - rbase;
    float xv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int v = min(8 * fg + e, V - 1);
      const unsigned ad = x_lds + (unsigned)(((rel0 + v) & (GF_RING - 1)) * (CIN * 4) + (16 * mt + fr) * 4);
      asm volatile("ds_read_b32 %0, %1" : "=v"(xv[e]) : "v"(ad));
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]), "+v"(xv[4]), "+v"(xv[5]), "+v"(xv[6]), "+v"(xv[7])
                 :
                 : "memory");
    bf16x8 xah, xal;  // lane holds x[v = 8 fg + e][c = 16 mt + fr], rows v >= V zero
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = 8 * fg + e < V ? xv[e] : 0.f;
      const __bf16 h = (__bf16)x;
      xah[e] = h;
      xal[e] = (__bf16)(x - (float)h);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int wk = 16 * (2 * nh + q) + fr;
      const f32x4 acc = gf_mfma_x3m(xah, xal, bhi[q], blo[q], f32x4{0.f, 0.f, 0.f, 0.f});
      // lane holds Z[wk][c = 16 mt + 4 fg + r], r = 0..3: GEMM row m = f V + w, 32-channel block 2 k + mt / 2,
      // 8 bytes of 16-B piece 2 (mt & 1) + fg / 2 (hi) and 4 + that (lo)
      const int w = wk / K, k = wk - w * K;
      const int m = f * V + w, tt = m >> 5, r = m & 31;
      gf_bf16x4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = (__bf16)acc[e];
        l[e] = (__bf16)(acc[e] - (float)h[e]);
      }
      if (wk < KV && tt >= tile0 && tt < tile1) {
        char* row = gf_smem + ((tt - tile0) & 1) * L::ABUF + ((2 * k + (mt >> 1)) * GF_BM + r) * 128 + (fg & 1) * 8;
        const int p = 2 * (mt & 1) + (fg >> 1);
        *reinterpret_cast<gf_bf16x4*>(row + swz(r, p) * 16) = h;
        *reinterpret_cast<gf_bf16x4*>(row + swz(r, 4 + p) * 16) = l;
      }
    }
  };

  // a tile's staged g rows -> HBM (16-B pieces; FULL: every row valid, all tiles but the problem's last)
  constexpr int CPR = NT * 4 / 16;
  auto store_g = [&](int tile, auto full) {
    gf_u32x4 v[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int q = tid + i * GF_THREADS, rl = q / CPR, c = q - rl * CPR;
      asm volatile("ds_read_b128 %0, %1" : "=v"(v[i]) : "v"(img_lds + (unsigned)(rl * OTS * 4 + c * 16)));
    }
    if constexpr (PIECES == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0])::"memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[PIECES - 1])::"memory");
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int q = tid + i * GF_THREADS, rl = q / CPR, c = q - rl * CPR;
      const int m = tile * GF_BM + rl;
      if (!decltype(full)::value && m >= M) continue;
      *reinterpret_cast<gf_u32x4*>(reinterpret_cast<char*>(a.g + (size_t)m * NT) + c * 16) = v[i];
    }
  };
  // a tile's Z rows [hi 192 | lo 192] from its A buffer -> HBM: piece j of a 768-B row is 16-B piece
  // j % 4 (+ 4 for lo) of block (j % 24) / 4
  static_assert(GF_ZP == 3, "store_z waits for three reads");
  auto store_z = [&](int tile, int buf, auto full) {
    gf_u32x4 v[GF_ZP];
#pragma unroll
    for (int i = 0; i < GF_ZP; ++i) {
      const int q = tid + i * GF_THREADS, rl = q / 48, j = q - rl * 48;
      const int lo = j >= 24, jj = j - 24 * lo, b = jj >> 2, p = (jj & 3) + 4 * lo;
      asm volatile("ds_read_b128 %0, %1"
                   : "=v"(v[i])
                   : "v"(a_lds + (unsigned)(buf * L::ABUF + (b * GF_BM + rl) * 128 + swz(rl, p) * 16)));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2])::"memory");
#pragma unroll
    for (int i = 0; i < GF_ZP; ++i) {
      const int q = tid + i * GF_THREADS, rl = q / 48, j = q - rl * 48;
      const int m = tile * GF_BM + rl;
      if (!decltype(full)::value && m >= M) continue;
      *reinterpret_cast<gf_u32x4*>(reinterpret_cast<char*>(a.z3) + (size_t)m * (4 * GF_KC) + j * 16) = v[i];
    }
  };

  int fnext = (tile0 * GF_BM) / V;  // first frame not yet placed
  auto body = [&](int tile, auto first, auto full) {
    const int it = tile - tile0, buf = it & 1;
    if constexpr (!decltype(first)::value) store_g(tile - 1, std::true_type{});
    const int flast = (min(tile * GF_BM + GF_BM, M) - 1) / V;
    for (; fnext <= flast; ++fnext) mix_frame(fnext);
    // the tile's block is placed; block tile - 1 of the x ring is dead (its frames are done)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    load_block(tile + GF_XD);
    store_z(tile, buf, full);
    const char* A = gf_smem + buf * L::ABUF;
    f32x4 acc[WN];
#pragma unroll
    for (int y = 0; y < WN; ++y) acc[y] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < KS / 2; ++b) {
      const int r = wm * 16 + fr;
      const bf16x8 fah = *reinterpret_cast<const bf16x8*>(A + (b * GF_BM + r) * 128 + swz(r, fg) * 16);
      const bf16x8 fal = *reinterpret_cast<const bf16x8*>(A + (b * GF_BM + r) * 128 + swz(r, 4 + fg) * 16);
#pragma unroll
      for (int y = 0; y < WN; ++y) {
        acc[y] = mfma_bf16x(fah, wf[y][2 * b], acc[y]);
        acc[y] = mfma_bf16x(fal, wf[y][2 * b], acc[y]);
        acc[y] = mfma_bf16x(fah, wf[y][2 * b + 1], acc[y]);
      }
    }
    // every thread's reads of the image (store_g above) and of the A buffer are done
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rl = wm * 16 + fg * 4 + r, m = tile * GF_BM + rl;
      const bool ok = m < M;
      const int vj = (ok ? m : 0) % V;  // (no branch: the four rows' table reads are issued together)
#pragma unroll
      for (int y = 0; y < WN; ++y) {
        const int jl = wj * 16 * WN + y * 16 + fr;
        float v = acc[y][r];
        v += bv[vj * NT + jl];
        if (!ok) v = 0.f;
        ssum[y] += v;
        ssq[y] += v * v;
        reinterpret_cast<float*>(img)[rl * OTS + jl] = v;
      }
    }
    // x block tile + 2 has landed: it was issued in tile it + 2 - XD, after which that tile issued its Z
    // pieces and each later tile OPS operations, which stay in flight (the first XD - 2 tiles' blocks
    // landed in the prologue and fewer operations are outstanding: no wait)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NSTEADY) : "memory");
    __builtin_amdgcn_s_barrier();
  };
  const bool ragged = tile1 == ntiles && M % GF_BM != 0;  // the problem's last tile is ours and partial
  const int tfull = ragged ? tile1 - 1 : tile1;
  if (tile0 < tfull) {
    body(tile0, std::true_type{}, std::true_type{});
    for (int tile = tile0 + 1; tile < tfull; ++tile) body(tile, std::false_type{}, std::true_type{});
    if (ragged) body(tile1 - 1, std::false_type{}, std::false_type{});
  } else {
    body(tile0, std::true_type{}, std::false_type{});
  }
  store_g(tile1 - 1, std::false_type{});
  // ---- BN sums of the workgroup's tiles: lanes -> waves -> one fp64 add per column (pw_gemm's) ----
#pragma unroll
  for (int y = 0; y < WN; ++y) {
    ssum[y] += __shfl_xor(ssum[y], 16, 64);
    ssum[y] += __shfl_xor(ssum[y], 32, 64);
    ssq[y] += __shfl_xor(ssq[y], 16, 64);
    ssq[y] += __shfl_xor(ssq[y], 32, 64);
  }
  if (fg == 0) {
#pragma unroll
    for (int y = 0; y < WN; ++y) {
      red[(wm * 2 + 0) * NT + wj * 16 * WN + y * 16 + fr] = ssum[y];
      red[(wm * 2 + 1) * NT + wj * 16 * WN + y * 16 + fr] = ssq[y];
    }
  }
  __syncthreads();
  for (int t = tid; t < 2 * NT; t += GF_THREADS) {
    const int q = t / NT, j = t - q * NT;
    const float s = red[(0 * 2 + q) * NT + j] + red[(1 * 2 + q) * NT + j];
    atomic_add_d((q == 0 ? a.st_sum : a.st_sq) + j, (double)s);
  }
  // drain the DMA of the blocks past the range before the workgroup ends
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace f3

using namespace f3;

bool f3_gcn_fwd_mix_ok(int K, int V, int Cin, int C) {
  return K == GF_K && Cin == GF_CIN && V >= 1 && V <= GF_VMAX && (C == 64 || C == 128);
}

template <int WN>
static int gf_launch(const GcnFwdMixArgs& a, int grid, int per_wg, hipStream_t s) {
  constexpr int lds = GfLds<WN>::BYTES;
  F3_LDS_LIMIT((gcn_fwd_mix_x3_kernel<WN>), lds);
  hipLaunchKernelGGL((gcn_fwd_mix_x3_kernel<WN>), dim3(grid), dim3(GF_THREADS), lds, s, a, per_wg);
  F3_LAUNCH_CHECK();
  return F3_OK;
}

int f3_gcn_fwd_mix(const GcnFwdMixArgs* args, hipStream_t s) {
  const GcnFwdMixArgs& a = *args;
  if (!f3_gcn_fwd_mix_ok(a.K, a.V, a.Cin, a.C) || a.frames < 0) return F3_EINVAL;
  if (!a.A || !a.x || !a.z3 || !a.w || !a.bias || !a.g || !a.st_sum || !a.st_sq || !a.zero) return F3_EINVAL;
  if ((long long)a.frames * a.V >= (1ll << 31) - 64 * GF_BM) return F3_EINVAL;
  // 16-B pieces: x rows and the bias table by LDS-DMA, Z and g rows by 16-B stores
  if ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.z3) |
       reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.w)) & 15)
    return F3_EINVAL;
  if (a.frames == 0) return F3_OK;
  static int cus = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipGetLastError();
    return n;
  }();
  // pw_gemm's ranges (one column group): the statistics partials are summed per workgroup
  const int ntiles = (a.frames * a.V + GF_BM - 1) / GF_BM;
  const int nr0 = std::max(1, cus);
  const int per_wg = (ntiles + nr0 - 1) / nr0;
  const int grid = (ntiles + per_wg - 1) / per_wg;
  return a.C == 64 ? gf_launch<1>(a, grid, per_wg, s) : gf_launch<2>(a, grid, per_wg, s);
}
