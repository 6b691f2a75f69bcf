// gemm_glds_kernel: the LDS-DMA GEMM / implicit-GEMM conv kernel for gfx950, its helpers and its picker.  A header, because its 105
// instantiations are compiled in two units: gemm_glds_gemm.hip (CONV = false) and gemm_glds_conv.hip (CONV = true) each include it and
// export pick_glds_unit<CONV>; everything here has internal linkage, one copy per unit.
//
// bf16 fast path: same tile / MFMA / epilogue, but BOTH operands are staged global -> LDS with
// global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip, no ds_write): on gfx950 a ds_write_b128 costs ~13 LDS
// cycles per wave-instruction (MI355X_MICROARCH.md §LDS), which made the register-staged kernel LDS-bound.
// One wave-instruction writes 1 KiB = 8 rows x 128 B, lane-linear; the XOR swizzle of the 16-byte chunk is
// applied on the per-lane SOURCE address (guide rule 21).  Out-of-image taps / tile tails read a 16-byte zero
// page instead, which gives the zero padding for free.
// Pipeline: a ring of STAGES LDS buffers, k-tiles t+1 .. t+STAGES-1 in flight while tile t is multiplied.  Each wave
// waits for ITS OWN loads of tile t with a counted s_waitcnt vmcnt (loads retire in order, so "all but the newest
// (STAGES-2) tiles' worth"), then one s_barrier makes every wave's part of tile t visible and proves that everybody is
// done reading the buffer of tile t-1, which is the one the next DMA batch overwrites.  STAGES = 2 keeps two blocks per
// CU (2 x 74 KB); grids that cannot put two blocks on a CU anyway run STAGES = 4 (147 KB) so that a lone block still
// covers the ~1.5 us global -> LDS latency.
#pragma once
#include "gemm_shared.h"

namespace {
using namespace crg_mm;
using crg_plan::Launch;

// s_waitcnt vmcnt(n * LOADS) for a wave-uniform number of k-tile batches n = 0..4 that may stay in flight
template <int LOADS>
__device__ __forceinline__ void wait_batches(int n) {
  if (n <= 0) wait_vmcnt<0>();
  else if (n == 1) wait_vmcnt<(1 * LOADS < 64 ? 1 * LOADS : 0)>();
  else if (n == 2) wait_vmcnt<(2 * LOADS < 64 ? 2 * LOADS : 0)>();
  else if (n == 3) wait_vmcnt<(3 * LOADS < 64 ? 3 * LOADS : 0)>();
  else wait_vmcnt<(4 * LOADS < 64 ? 4 * LOADS : 0)>();
}

// (launch bounds: configuration A - 128-row tiles, 4 waves, 2 stages - is built for TWO blocks per CU: its register budget is 256.  The
// plain instantiations fit it on their own (156 VGPRs + 80 accumulators); the one that emits GroupNorm statistics needs the cap.)
// XT: the extra side channel this instantiation carries (each keeps ~10-40 more values live, hence template arms rather than runtime branches):
//   0 none; 1 = GST, emits GroupNorm statistics (p.gstat); 2 = RST, emits LayerNorm row statistics (p.rstat); 3 = LNE, LayerNorm as an
//   epilogue correction from the producer's row statistics (p.ln_stat, see GemmP) - no residual in that form (none of its callers has one)
template <int WNT, typename YT, bool CONV, int STAGES, int WMT, int KG, int NS = 1, bool PAIR = false, int XT = 0>
#ifndef CRG_LB_A  // dev knob (tools/build_variant.sh): 1 (default) = every configuration-A instantiation is capped at 256 registers (unified file: 191-204
           // VGPRs, no accumulator registers; bench A/B in one call: 246.6 -> 245.6 ms), 0 = only the statistics one
#define CRG_LB_A 1
#endif
__global__ __launch_bounds__(256 * KG, ((XT != 0 || CRG_LB_A) && KG == 1 && WMT == 4 && STAGES == 2 && NS == 1) ? 2 : 1) void gemm_glds_kernel(GemmP p) {
  constexpr bool GST = XT == 1, RST = XT == 2, LNE = XT == 3;
  static_assert(!PAIR || (sizeof(YT) == 2 && NS == 1), "paired columns: bf16 output, single-plane operands");
  static_assert(!(GST || RST) || PAIR, "GroupNorm / LayerNorm statistics come from the paired epilogue");  // GST / RST: the instantiations that emit them
  static_assert(!LNE || (!CONV && NS == 1 && sizeof(YT) == 2), "LayerNorm epilogue: bf16 GEMM");
  // NS = 2: split-bf16 (fp32-class) operands - the activations arrive pre-split as two bf16 planes (hi = bf16(x),
  // lo = bf16(x - hi), written by the producing GroupNorm / split pass), the weights as their two packed planes; all four
  // are staged by LDS-DMA and every fragment pair costs three MFMAs (hi*hi + hi*lo + lo*hi).
  // Block tile (32*WMT) x (32*WNT) x 64; 4*KG waves.  The 4 waves of a k-group tile the block 2 x 2 (each 16*WMT rows x
  // 16*WNT columns); with KG == 2 the second group multiplies the second 32-wide k-step of every k-tile (in-block
  // split-K: twice the waves per SIMD on the same LDS traffic - for grids that cannot put two blocks on a CU) and its
  // accumulators are folded into group 0 through LDS before the epilogue.
  constexpr int BMT = 32 * WMT;
  constexpr int BN = 32 * WNT;
  constexpr int NW = 4 * KG;
  constexpr int XS_BYTES = BMT * 128;
  constexpr int WS_BYTES = BN * 128;
  constexpr int STAGE_BYTES = NS * (XS_BYTES + WS_BYTES);  // [X hi][X lo][W hi][W lo]
  constexpr int XRG = BMT / 8, WRG = BN / 8;      // 8-row groups (one 1 KiB wave-instruction each)
  constexpr int XL = (XRG + NW - 1) / NW;         // DMA instructions per wave per k-tile (uniform: waves without a row
  constexpr int WL = (WRG + NW - 1) / NW;         // group left issue a dummy load so that vmcnt counts stay uniform)
  constexpr int DUMMY = STAGES * STAGE_BYTES;     // 1 KiB scratch target of the dummy loads
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int kg = wave >> 2;  // k-group of this wave
  const int wm = (wave & 3) >> 1, wn = wave & 1;

  int tile_m, tile_n, sid;
  block_to_tile(p, tile_m, tile_n, sid);
  const int m0 = tile_m * BMT, n0 = tile_n * BN;
  const int bz = blockIdx.y;

  const bf16* A = reinterpret_cast<const bf16*>(p.a) + (long)bz * p.a_bs;
  const bf16* Wp = p.w + (long)bz * p.w_bs;
  // lo planes live at a fixed element distance from the hi planes (same layout): one offset each
  const long a_lo_off = NS == 2 ? reinterpret_cast<const bf16*>(p.a_lo) - reinterpret_cast<const bf16*>(p.a) : 0;
  const long w_lo_off = NS == 2 ? p.w_lo - p.w : 0;
  const bf16* zpage = p.zero_page;

  // this lane always stages LDS row (8*g + lane/8), physical chunk lane%8 of row group g = wave + NW*q;
  // the data it carries is logical chunk clog = (lane%8) ^ (row%8)
  const int rsub = lane >> 3;
  const int clog = (lane & 7) ^ rsub;

  long xrow_off[XL];
  int xh[XL], xw[XL];
  bool xok[XL];
#pragma unroll
  for (int q = 0; q < XL; ++q) {
    const int m = m0 + (wave + NW * q) * 8 + rsub;
    xok[q] = m < p.M && (wave + NW * q) < XRG;
    if (CONV) {
      const int hw = p.Ho * p.Wo;
      const int img = m / hw;
      const int rem = m - img * hw;
      const int ho = rem / p.Wo;
      const int wo = rem - ho * p.Wo;
      xrow_off[q] = (long)img * p.H * p.W;
      xh[q] = ho * p.stride - p.pad_t;
      xw[q] = wo * p.stride - p.pad_l;
    } else {
      xrow_off[q] = (long)m * p.lda;
      xh[q] = xw[q] = 0;
    }
  }
  bool wok[WL];
  long wrow_off[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q) {
    const int pos = (wave + NW * q) * 8 + rsub;                     // LDS row of the weight tile this lane stages
    const int n = n0 + (PAIR ? unpair_col<WNT>(pos) : pos);       // the output column (= weight row) that lives there
    wok[q] = n < p.N && (wave + NW * q) < WRG;
    wrow_off[q] = (long)n * p.ldw;
  }

  // k-tile range of this K-slice: the first ks_r slices take ks_q + 1 tiles, the others ks_q (ks_q, ks_r from the host - a
  // 64-bit division by the runtime split count here cost ~1 us of scalar work on every block's latency chain)
  const int kt_begin = sid * p.ks_q + (sid < p.ks_r ? sid : p.ks_r);
  const int nk = kt_begin + p.ks_q + (sid < p.ks_r ? 1 : 0);

  // running (tap, channel) of this lane's logical chunk; advanced by 64 channels per k-tile
  int kc = kt_begin * BK + clog * 8;
  int tap = 0, cch = kc;
  const int taps = p.ks * p.ks;
  if (CONV) {
    if (p.cm) {
      tap = kt_begin % taps;
      cch = (kt_begin / taps) * BK + clog * 8;
    } else {
      tap = kc / p.Ctot;
      cch = kc - tap * p.Ctot;
    }
  }
  const int Hv = p.up ? 2 * p.H : p.H, Wv = p.up ? 2 * p.W : p.W;

  auto stage = [&](int buf) {
    char* xs = smem + buf * STAGE_BYTES;
    char* ws = xs + NS * XS_BYTES;
    const bool kok = kc < p.K;
    if (CONV) {
      const int kh = (p.ks == 3) ? (tap * 11) >> 5 : 0;
      const int kw = (p.ks == 3) ? tap - kh * 3 : 0;
      const bool second = cch >= p.C1;
      const bf16* base = reinterpret_cast<const bf16*>(second ? p.x2 : p.a);
      const int Cs = second ? p.C2 : p.C1;
      const int cs = second ? cch - p.C1 : cch;
#pragma unroll
      for (int q = 0; q < XL; ++q) {
        const int hv = xh[q] + kh, wv = xw[q] + kw;
        const bool ok = kok && xok[q] && (unsigned)hv < (unsigned)Hv && (unsigned)wv < (unsigned)Wv;
        const int hs = p.up ? hv >> 1 : hv, wsrc = p.up ? wv >> 1 : wv;
        const bf16* src = ok ? base + (xrow_off[q] + (long)hs * p.W + wsrc) * Cs + cs : zpage;
        char* dst = (wave + NW * q) < XRG ? xs + (wave + NW * q) * 1024 : smem + DUMMY;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        if constexpr (NS == 2) {
          const bf16* src2 = ok ? src + a_lo_off : zpage;
          char* dst2 = (wave + NW * q) < XRG ? dst + XS_BYTES : smem + DUMMY;
          __builtin_amdgcn_global_load_lds((gptr_t)src2, (lptr_t)dst2, 16, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < XL; ++q) {
        const bool ok = kok && xok[q];
        const bf16* src = ok ? A + xrow_off[q] + kc : zpage;
        char* dst = (wave + NW * q) < XRG ? xs + (wave + NW * q) * 1024 : smem + DUMMY;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        if constexpr (NS == 2) {
          const bf16* src2 = ok ? src + a_lo_off : zpage;
          char* dst2 = (wave + NW * q) < XRG ? dst + XS_BYTES : smem + DUMMY;
          __builtin_amdgcn_global_load_lds((gptr_t)src2, (lptr_t)dst2, 16, 0, 0);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < WL; ++q) {
      const bool ok = kok && wok[q];
      const bf16* src = ok ? Wp + wrow_off[q] + kc : zpage;
      char* dst = (wave + NW * q) < WRG ? ws + (wave + NW * q) * 1024 : smem + DUMMY;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
      if constexpr (NS == 2) {
        const bf16* src2 = ok ? src + w_lo_off : zpage;
        char* dst2 = (wave + NW * q) < WRG ? dst + WS_BYTES : smem + DUMMY;
        __builtin_amdgcn_global_load_lds((gptr_t)src2, (lptr_t)dst2, 16, 0, 0);
      }
    }
    // advance to the next k-tile
    kc += BK;
    if (CONV) {
      if (p.cm) {
        if (++tap == taps) {
          tap = 0;
          cch += BK;
        }
      } else {
        cch += BK;
        while (cch >= p.Ctot) {
          cch -= p.Ctot;
          ++tap;
        }
      }
    }
  };

  f32x4 acc[WNT][WMT];
#pragma unroll
  for (int i = 0; i < WNT; ++i)
#pragma unroll
    for (int j = 0; j < WMT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fq = lane >> 4;
  // residual tile of this lane, fetched first so that its latency hides under the whole K loop (bf16 outputs); being the
  // oldest loads in flight they are retired by the first counted wait
  // The loads below are UNCONDITIONAL on clamped, always-valid addresses (rows >= M / columns >= N are never used by the
  // epilogue): a `cond ? load : 0` select made the compiler zero-fill, branch and - worse - wait (s_waitcnt vmcnt(0)) right
  // behind every load, which serialised the residual latency in front of the first DMA of every block.
  // PAIR: one 16-byte load per tile pair (r2) plus an 8-byte one for an odd last tile (r1).
  bf16x4 rres[PAIR ? 1 : WNT][PAIR ? 1 : WMT];
  bf16x8 r2[PAIR ? (WNT / 2 > 0 ? WNT / 2 : 1) : 1][PAIR ? WMT : 1];
  bf16x4 r1[PAIR ? WMT : 1];
  f32x4 bpre[WNT];
  const bool pre_res = !LNE && sizeof(YT) == 2 && p.res && p.splits == 1 && (p.ldr & 3) == 0 && (p.N & 3) == 0 && p.epi != CRG_EPI_GEGLU;
  const bool pre_bias = p.bias_mode == CRG_BIAS_COL && p.splits == 1 && (p.N & 3) == 0 && p.epi != CRG_EPI_GEGLU;
  if (kg == 0) {
    const int nb = n0 + wn * (16 * WNT);
    if (pre_res) {
      const bf16* R = reinterpret_cast<const bf16*>(p.res) + (long)bz * p.r_bs;
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int m = m0 + wm * (16 * WMT) + j * 16 + frow;
        const bf16* Rm = R + (long)(m < p.M ? m : p.M - 1) * p.ldr;
        if constexpr (PAIR) {
#pragma unroll
          for (int u = 0; u < WNT / 2; ++u) {
            const int n = nb + 32 * u + 8 * fq;
            r2[u][j] = *reinterpret_cast<const bf16x8*>(Rm + (n + 8 <= p.N ? n : p.N - 8));
          }
          if constexpr (WNT & 1) {
            const int n = nb + 16 * (WNT - 1) + 4 * fq;
            r1[j] = *reinterpret_cast<const bf16x4*>(Rm + (n + 4 <= p.N ? n : p.N - 4));
          }
        } else {
#pragma unroll
          for (int i = 0; i < WNT; ++i) {
            const int n = nb + i * 16 + fq * 4;
            rres[i][j] = *reinterpret_cast<const bf16x4*>(Rm + (n + 4 <= p.N ? n : p.N - 4));
          }
        }
      }
    }
    // column bias of this lane's 4-wide output groups: also fetched ahead of the K loop (a lone block per CU would otherwise
    // pay a full global-load latency between its last MFMA and its first store)
    if (pre_bias) {
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int n = (PAIR && i < 2 * (WNT / 2)) ? nb + 32 * (i >> 1) + 8 * fq + 4 * (i & 1) : nb + 16 * i + 4 * fq;
        bpre[i] = *reinterpret_cast<const f32x4*>(p.bias + (n + 4 <= p.N ? n : p.N - 4));
      }
    }
  }

  constexpr int LOADS = NS * (XL + WL);  // LDS-DMA instructions per wave per k-tile
  constexpr int D = STAGES - 1;   // prefetch distance
#pragma unroll
  for (int s = 0; s < D; ++s)
    if (kt_begin + s < nk) stage(s);
  // LNE: (rstd, mean * rstd) of this lane's rows and the column sums ln_s of its columns.  Lane l of the wave folds the partials of the
  // wave's row l (coalesced: consecutive lanes, consecutive rows of a plane); the values of rows 16 j + frow come over by ds_bpermute.
  // Placed BEHIND the first DMA batches: the fold needs the partials, so the wait it implies covers the DMA latency it runs beside
  // (ahead of them it would put a load round trip in front of every block's first DMA).
  float ln_r = 0.f, ln_mr = 0.f;
  f32x4 spre[LNE ? WNT : 1];
  if constexpr (LNE) {
    if (kg == 0) {
      const int rl = lane < 16 * WMT ? lane : 16 * WMT - 1;
      const int mr = m0 + wm * (16 * WMT) + rl;
      const f32x2 rm = ln_row_coeffs(p.ln_stat, mr < p.M ? mr : p.M - 1, p.ln_parts, p.K, p.ln_eps);
      ln_r = rm[0];
      ln_mr = rm[1];
      const int nb = n0 + wn * (16 * WNT);
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int n = (PAIR && i < 2 * (WNT / 2)) ? nb + 32 * (i >> 1) + 8 * fq + 4 * (i & 1) : nb + 16 * i + 4 * fq;
        spre[i] = *reinterpret_cast<const f32x4*>(p.ln_s + (n + 4 <= p.N ? n : p.N - 4));
      }
    }
  }

  int buf = 0, nbuf = D;  // ring positions of tile kt and of tile kt + D
  // PF (the one-block-per-CU in-block split-K configuration: 64-row tiles, 8 waves, 4 stages): the fragments of k-tile kt + 1 are
  // requested at the top of k-tile kt and consumed one barrier later, so that no MFMA block waits out an LDS round trip (a k-tile
  // is 10 MFMAs per wave here: barrier + read latency + MFMAs in series was ~1100 cycles per k-tile for 160 cycles of matrix work).
  // Needs k-tile kt + 1 in LDS at the top of k-tile kt: the counted wait leaves one batch fewer in flight (two k-tiles of lead).
#ifdef CRG_GEMM_NOPF
  constexpr bool PF = false;
#else
  constexpr bool PF = KG == 2 && STAGES >= 4 && NS == 1;
#endif
  if constexpr (PF) {
    bf16x8 xf[2][WMT], wf[2][WNT];
    auto reads = [&](int set, int b) {
      const char* xs = smem + b * STAGE_BYTES;
      const char* ws = xs + XS_BYTES;
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(xs + lds_off(wm * (16 * WMT) + j * 16 + frow, kg * 4 + fq));
        if (set == 0) xf[0][j] = v; else xf[1][j] = v;
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(ws + lds_off(wn * (16 * WNT) + i * 16 + frow, kg * 4 + fq));
        if (set == 0) wf[0][i] = v; else wf[1][i] = v;
      }
    };
    auto mm = [&](const bf16x8 (&x)[WMT], const bf16x8 (&w)[WNT]) {
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) acc[i][j] = CRG_MFMA_16x16x32(w[i], x[j], acc[i][j]);
    };
    // top of k-tile kt (PARITY = which fragment set holds it): k-tile kt + 1 landed, barrier, issue kt + D, request kt + 1, multiply kt
    auto ktile = [&](int kt, auto PARc) {
      constexpr int par = decltype(PARc)::value;
      const int after = nk - 2 - kt;  // k-tiles issued after kt + 1 (they may stay in flight: at most D - 2)
      wait_batches<LOADS>(after < D - 2 ? after : D - 2);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_setprio(2);
      if (kt + D < nk) stage(nbuf);
      __builtin_amdgcn_s_setprio(0);
      const int b1 = (buf + 1 == STAGES) ? 0 : buf + 1;
      if (kt + 1 < nk) reads(par ^ 1, b1);
      __builtin_amdgcn_sched_barrier(0);
      mm(xf[par], wf[par]);
      __builtin_amdgcn_sched_barrier(0);
      buf = b1;
      nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
    };
    if (kt_begin < nk) {
      // first k-tile: wait for it alone, publish, request its fragments (the only exposed read)
      const int newer = nk - 1 - kt_begin;
      wait_batches<LOADS>(newer < D - 1 ? newer : D - 1);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      reads(0, 0);
    }
    int kt = kt_begin;
    for (; kt + 1 < nk; kt += 2) {
      ktile(kt, std::integral_constant<int, 0>{});
      ktile(kt + 1, std::integral_constant<int, 1>{});
    }
    if (kt < nk) ktile(kt, std::integral_constant<int, 0>{});
  } else {
  for (int kt = kt_begin; kt < nk; ++kt) {
    const int newer = nk - 1 - kt;  // tiles issued after tile kt that may stay in flight (at most D - 1)
    if constexpr (D >= 4) wait_batches<LOADS>(newer < D - 1 ? newer : D - 1);
    else if (D >= 3 && newer >= 2) wait_vmcnt<(D >= 3 ? 2 : 0) * LOADS>();
    else if (D >= 2 && newer >= 1) wait_vmcnt<(D >= 2 ? 1 : 0) * LOADS>();
    else wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // the DMA issue (address VALU + 1 KiB pieces) runs at raised wave priority: next to a wave of the CU's other block that
    // streams MFMAs it was issued late and its data landed late (conv -2..3 % per shape, GEMM neutral; raising the priority
    // of the MFMA phase instead was 4 % slower)
    __builtin_amdgcn_s_setprio(2);
    if (kt + D < nk) stage(nbuf);
    __builtin_amdgcn_s_setprio(0);
    const char* xs = smem + buf * STAGE_BYTES;
    const char* ws = xs + NS * XS_BYTES;
#pragma unroll
    for (int k2 = 0; k2 < 2 / KG; ++k2) {
      const int ks = KG == 2 ? kg : k2;
      bf16x8 xf[WMT], wf[WNT], xl[NS == 2 ? WMT : 1], wl[NS == 2 ? WNT : 1];
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int off = lds_off(wm * (16 * WMT) + j * 16 + frow, ks * 4 + fq);
        xf[j] = *reinterpret_cast<const bf16x8*>(xs + off);
        if constexpr (NS == 2) xl[j] = *reinterpret_cast<const bf16x8*>(xs + XS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int off = lds_off(wn * (16 * WNT) + i * 16 + frow, ks * 4 + fq);
        wf[i] = *reinterpret_cast<const bf16x8*>(ws + off);
        if constexpr (NS == 2) wl[i] = *reinterpret_cast<const bf16x8*>(ws + WS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) {
          if constexpr (NS == 2) {
            acc[i][j] = CRG_MFMA_16x16x32(wl[i], xf[j], acc[i][j]);
            acc[i][j] = CRG_MFMA_16x16x32(wf[i], xl[j], acc[i][j]);
          }
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
        }
    }
    buf = (buf + 1 == STAGES) ? 0 : buf + 1;
    nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
  }
  }
  if constexpr (KG == 2) {
    // fold the second k-group's partial tile into the first: [wave&3][i][j][lane] f32x4 in the (now idle) ring
    static_assert(4 * WNT * WMT * 64 * 16 <= STAGES * STAGE_BYTES, "reduction buffer must fit in the DMA ring");
    __syncthreads();  // every wave is done reading the ring (all DMA batches were retired by the last counted wait)
    f32x4* red = reinterpret_cast<f32x4*>(smem) + ((wave & 3) * WNT * WMT) * 64 + lane;
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) red[(i * WMT + j) * 64] = acc[i][j];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int i = 0; i < WNT; ++i)
#pragma unroll
      for (int j = 0; j < WMT; ++j) acc[i][j] += red[(i * WMT + j) * 64];
  }
  if constexpr (LNE) {
    // y = rstd * (acc - mean * s[n]) (+ bias' in the epilogue): LayerNorm(x) W^T from the GEMM on the raw rows
#pragma unroll
    for (int j = 0; j < WMT; ++j) {
      const float rj = __shfl(ln_r, j * 16 + frow), mj = __shfl(ln_mr, j * 16 + frow);
#pragma unroll
      for (int i = 0; i < WNT; ++i) acc[i][j] = rj * acc[i][j] - mj * spre[i];
    }
  }
  if constexpr (PAIR && !CONV && !GST && !RST) {
    if (p.vt && n0 >= p.vt_n0) {
      // transposed n-tile (the V third of a fused Q | K | V projection -> V^T [sample][channel][token], what the LDS-DMA / pipelined
      // attention kernels stage): lane = one token x 8 (4) consecutive channels -> one 2-byte store per channel; the 16 lanes of a
      // DPP row hold 16 consecutive tokens, i.e. 32 contiguous bytes of a V^T row per store instruction and row
      const int Cv = p.N - p.vt_n0;
      const int nb = n0 + wn * (16 * WNT);
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int m = m0 + wm * (16 * WMT) + j * 16 + frow;
        if (m >= p.M) continue;
        const int bs = m / p.vt_T, tk = m - bs * p.vt_T;
        bf16* V = p.vt + ((long)bs * Cv - p.vt_n0) * p.vt_ld + tk;
#pragma unroll
        for (int u = 0; u < WNT / 2; ++u) {
          const int n = nb + 32 * u + 8 * fq;
          if (n >= p.N) continue;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = e < 4 ? acc[2 * u][j][e] : acc[2 * u + 1][j][e - 4];
            if (pre_bias) v += e < 4 ? bpre[2 * u][e] : bpre[2 * u + 1][e - 4];
            V[(long)(n + e) * p.vt_ld] = (bf16)v;
          }
        }
        if constexpr (WNT & 1) {
          const int n = nb + 16 * (WNT - 1) + 4 * fq;
          if (n < p.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[WNT - 1][j][e];
              if (pre_bias) v += bpre[WNT - 1][e];
              V[(long)(n + e) * p.vt_ld] = (bf16)v;
            }
          }
        }
      }
      return;
    }
  }
  if constexpr (PAIR) {
    gemm_epilogue_pairs<WNT, WMT, GST ? 1 : 0, RST>(p, acc, m0, n0, wm, wn, frow, fq, bz, r2, r1, pre_res, bpre, pre_bias);
  } else {
    gemm_epilogue<WNT, YT, WMT>(p, acc, m0, n0, wm, wn, frow, fq, bz, sid, rres, pre_res, bpre, pre_bias);
  }
}

// gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, PAIR, XT>: the epilogues that exist for (YT, CONV)
template <int WNT, typename YT, bool CONV, int STAGES, int WMT, int KG>
KernFn pick_glds_epilogue(const Launch& L) {
  if constexpr (sizeof(YT) == 2) {
    if constexpr (!CONV) {
      if (L.xt == 3) return L.pair ? gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, true, 3> : gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, false, 3>;
      if (L.xt == 2) return gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, true, 2>;
    }
    if (L.xt == 1) return gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, true, 1>;
    if (L.pair) return gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG, 1, true>;
  }
  return gemm_glds_kernel<WNT, YT, CONV, STAGES, WMT, KG>;
}

template <int WNT, typename YT, bool CONV>
KernFn pick_glds(const Launch& L) {
  if (L.ns == 2) {  // pre-split planes: 8 waves in two k-groups
    if constexpr (sizeof(YT) == 4) return gemm_glds_kernel<WNT, float, CONV, 2, 4, 2, 2>;
    return nullptr;
  }
  switch (L.cfg) {
    case 3: return pick_glds_epilogue<WNT, YT, CONV, CRG_C_STAGES, 2, 2>(L);
    case 4: return pick_glds_epilogue<WNT, YT, CONV, 2, 2, 1>(L);
    default: return pick_glds_epilogue<WNT, YT, CONV, 2, 4, 1>(L);
  }
}

// the kernel of this unit's CONV for the planned launch: tile width and output type
template <bool CONV>
KernFn pick_glds_unit(const Launch& L) {
  switch (L.wnt) {
    case 1: return L.y_f32 ? pick_glds<1, float, CONV>(L) : pick_glds<1, bf16, CONV>(L);
    case 4: return L.y_f32 ? pick_glds<4, float, CONV>(L) : pick_glds<4, bf16, CONV>(L);
    case 5: return L.y_f32 ? pick_glds<5, float, CONV>(L) : pick_glds<5, bf16, CONV>(L);
    default: return nullptr;
  }
}

}  // namespace
