// MFMA GEMM / implicit-GEMM conv2d for gfx950: the register-staged kernel (gemm_kernel).
//
//   Y[m][n] = epilogue( sum_k X[m][k] * W[n][k] )      (both operands K-contiguous)
//
// Block tile 128(m) x 32*WNT(n) x 64(k), 256 threads = 4 waves as 2(m) x 2(n); each wave owns
// 64(m) x 16*WNT(n) as 4 x WNT accumulators of v_mfma_f32_16x16x32_bf16.  The MFMA is issued with
// the WEIGHT tile as the A operand and the ACTIVATION tile as the B operand, so that D rows = n:
// a lane then holds 4 CONSECUTIVE output channels of one output row, and the epilogue (bias,
// timestep-embedding vector, residual, SiLU/GEGLU) runs on 4-wide vectors with 8/16-byte stores.
//
// Staging: global -> registers -> LDS (ds_write_b128), double-buffered LDS, one barrier per k-tile;
// the loads of k-tile t+1 are issued before the MFMAs of tile t and written after them (guide
// §6 G15 "async-STAGE split").  LDS rows are 128 B with the 16-B chunk index XOR-swizzled by
// (row & 7) so that the ds_read_b128 fragment reads (16 rows x same chunk) are conflict-free.
//
// The conv variant only changes the activation loader: row m -> (image, ho, wo), k -> (tap, channel)
// with zero fill outside the (optionally nearest-2x-upsampled) image and a second input pointer
// for the UNet skip concat.  BF16X3 (NSPLIT=2) stages hi and lo bf16 planes of both operands and
// issues hi*hi + hi*lo + lo*hi.
//
// A header: compiled in conv_rowhalo.hip, the other family whose unpaired epilogue is gemm_epilogue<WNT, YT, 4, false> (see there).
#pragma once
#include "gemm_shared.h"

namespace {
using namespace crg_mm;
using crg_plan::Launch;

__device__ __forceinline__ bf16x8 split_hi(const crg_vec8<float>& v, bf16x8& lo) {
  bf16x8 hi;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float f = v.get(i);
    bf16 h = (bf16)f;
    hi[i] = h;
    lo[i] = (bf16)(f - (float)h);
  }
  return hi;
}

// KG = 2 (the split-bf16 path): 8 waves; the second group of four multiplies the second 32-wide k-step of every k-tile and
// every thread stages half as many rows.  That path fills the LDS with one block per CU, and with one wave per SIMD the
// staging VALU work (fp32 -> hi/lo split, conv addressing: as many issue cycles as the MFMAs) ran strictly after the MFMAs;
// two waves per SIMD overlap one wave's staging with the other's MFMAs.
template <int WNT, int NSPLIT, typename AT, typename YT, bool CONV, int KG>
__global__ __launch_bounds__(256 * KG) void gemm_kernel(GemmP p) {
  constexpr int BN = 32 * WNT;
  constexpr int RS = 32 * KG;              // rows staged per pass by the block
  constexpr int XL = BM / RS;              // A rows per thread
  constexpr int WL = (BN + RS - 1) / RS;   // W rows per thread (last one guarded when RS does not divide BN)
  constexpr int XS_BYTES = BM * 128;
  constexpr int WS_BYTES = BN * 128;
  constexpr int STAGE_BYTES = NSPLIT * (XS_BYTES + WS_BYTES);
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int kg = wave >> 2;
  const int wm = (wave & 3) >> 1, wn = wave & 1;

  int tile_m, tile_n, sid;
  block_to_tile(p, tile_m, tile_n, sid);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int bz = blockIdx.y;

  const AT* A = reinterpret_cast<const AT*>(p.a) + (long)bz * p.a_bs;
  const bf16* A_lo = p.a_lo ? reinterpret_cast<const bf16*>(p.a_lo) + (long)bz * p.a_bs : nullptr;
  const bf16* Wp = p.w + (long)bz * p.w_bs;
  const bf16* Wlo = (NSPLIT == 2) ? p.w_lo + (long)bz * p.w_bs : nullptr;

  const int cc = t & 7;   // 16-byte chunk column inside the 64-wide k-tile
  const int r0 = t >> 3;  // 0..RS-1

  // ---- per-thread row descriptors (fixed for the whole K loop) ----
  long xrow_off[XL];   // linear: element offset of row start; conv: image index
  int xh[XL], xw[XL];  // conv: top-left input coordinate (virtual = after upsample)
  bool xok[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int m = m0 + r0 + RS * i;
    xok[i] = m < p.M;
    if (CONV) {
      const int hw = p.Ho * p.Wo;
      const int img = m / hw;
      const int rem = m - img * hw;
      const int ho = rem / p.Wo;
      const int wo = rem - ho * p.Wo;
      xrow_off[i] = img;
      xh[i] = ho * p.stride - p.pad_t;
      xw[i] = wo * p.stride - p.pad_l;
    } else {
      xrow_off[i] = (long)m * p.lda;
      xh[i] = xw[i] = 0;
    }
  }
  bool wok[WL];
  long wrow_off[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int n = n0 + r0 + RS * i;
    wok[i] = n < p.N && r0 + RS * i < BN;
    wrow_off[i] = (long)n * p.ldw;
  }

  crg_vec8<AT> xr[XL];
  bf16x8 xr_lo[XL];  // only when A is a pre-split weight (a_is_weight)
  bf16x8 wr[WL], wr_lo[WL];
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  auto load_tile = [&](int kt) {
    const int kc = kt * BK + cc * 8;
    const bool kok = kc < p.K;
    if (CONV) {
      int tap, c;
      if (p.cm) {
        const int taps = p.ks * p.ks;
        tap = kt % taps;
        c = (kt / taps) * BK + cc * 8;
      } else {
        tap = kc / p.Ctot;
        c = kc - tap * p.Ctot;
      }
      const int kh = tap / p.ks;
      const int kw = tap - kh * p.ks;
      const int Hv = p.up ? 2 * p.H : p.H, Wv = p.up ? 2 * p.W : p.W;
      const bool second = c >= p.C1;
      const AT* base = reinterpret_cast<const AT*>(second ? p.x2 : p.a);
      const int Cs = second ? p.C2 : p.C1;
      const int cs = second ? c - p.C1 : c;
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int hv = xh[i] + kh, wv = xw[i] + kw;
        const bool ok = kok && xok[i] && (unsigned)hv < (unsigned)Hv && (unsigned)wv < (unsigned)Wv;
        if (ok) {
          const int hs = p.up ? hv >> 1 : hv, ws = p.up ? wv >> 1 : wv;
          xr[i].load(base + ((xrow_off[i] * p.H + hs) * p.W + ws) * Cs + cs);
        } else {
          xr[i].zero();
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        if (kok && xok[i]) {
          xr[i].load(A + xrow_off[i] + kc);
          if (NSPLIT == 2 && sizeof(AT) == 2) xr_lo[i] = *reinterpret_cast<const bf16x8*>(A_lo + xrow_off[i] + kc);
        } else {
          xr[i].zero();
          if (NSPLIT == 2 && sizeof(AT) == 2) xr_lo[i] = zero8;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      if (kok && wok[i]) {
        wr[i] = *reinterpret_cast<const bf16x8*>(Wp + wrow_off[i] + kc);
        if (NSPLIT == 2) wr_lo[i] = *reinterpret_cast<const bf16x8*>(Wlo + wrow_off[i] + kc);
      } else {
        wr[i] = zero8;
        if (NSPLIT == 2) wr_lo[i] = zero8;
      }
    }
  };

  auto store_tile = [&](int stage) {
    char* xs = smem + stage * STAGE_BYTES;
    char* ws = xs + NSPLIT * XS_BYTES;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int row = r0 + RS * i;
      const int off = lds_off(row, cc);
      if constexpr (sizeof(AT) == 4) {
        bf16x8 lo;
        const crg_vec8<float>& xv = reinterpret_cast<const crg_vec8<float>&>(xr[i]);
        bf16x8 hi = split_hi(xv, lo);
        *reinterpret_cast<bf16x8*>(xs + off) = hi;
        if (NSPLIT == 2) *reinterpret_cast<bf16x8*>(xs + XS_BYTES + off) = lo;
      } else {
        *reinterpret_cast<bf16x8*>(xs + off) = reinterpret_cast<const crg_vec8<bf16>&>(xr[i]).v;
        if (NSPLIT == 2) *reinterpret_cast<bf16x8*>(xs + XS_BYTES + off) = xr_lo[i];
      }
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int row = r0 + RS * i;
      if (RS * (WL - 1) + RS > BN && row >= BN) continue;  // guarded last pass
      const int off = lds_off(row, cc);
      *reinterpret_cast<bf16x8*>(ws + off) = wr[i];
      if (NSPLIT == 2) *reinterpret_cast<bf16x8*>(ws + WS_BYTES + off) = wr_lo[i];
    }
  };

  f32x4 acc[WNT][4];
#pragma unroll
  for (int i = 0; i < WNT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // k-tile range of this K-slice: the first ks_r slices take ks_q + 1 tiles, the others ks_q (ks_q, ks_r from the host - a
  // 64-bit division by the runtime split count here cost ~1 us of scalar work on every block's latency chain)
  const int kt_begin = sid * p.ks_q + (sid < p.ks_r ? sid : p.ks_r);
  const int nk = kt_begin + p.ks_q + (sid < p.ks_r ? 1 : 0);
  load_tile(kt_begin);
  store_tile(kt_begin & 1);
  __syncthreads();

  const int frow = lane & 15;
  const int fq = lane >> 4;
  for (int kt = kt_begin; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load_tile(kt + 1);
    const char* xs = smem + (kt & 1) * STAGE_BYTES;
    const char* ws = xs + NSPLIT * XS_BYTES;
#pragma unroll
    for (int k2 = 0; k2 < 2 / KG; ++k2) {
      const int ks = KG == 2 ? kg : k2;
      bf16x8 xf[4], xl[4], wf[WNT], wl[WNT];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int off = lds_off(wm * 64 + j * 16 + frow, ks * 4 + fq);
        xf[j] = *reinterpret_cast<const bf16x8*>(xs + off);
        if (NSPLIT == 2) xl[j] = *reinterpret_cast<const bf16x8*>(xs + XS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int off = lds_off(wn * (16 * WNT) + i * 16 + frow, ks * 4 + fq);
        wf[i] = *reinterpret_cast<const bf16x8*>(ws + off);
        if (NSPLIT == 2) wl[i] = *reinterpret_cast<const bf16x8*>(ws + WS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (NSPLIT == 2) {
            acc[i][j] = CRG_MFMA_16x16x32(wl[i], xf[j], acc[i][j]);
            acc[i][j] = CRG_MFMA_16x16x32(wf[i], xl[j], acc[i][j]);
          }
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
        }
    }
    if (more) store_tile((kt + 1) & 1);
    __syncthreads();
  }

  if constexpr (KG == 2) {
    // fold the second k-group's partial tile into the first through the (now idle) staging buffers
    static_assert(4 * WNT * 4 * 64 * 16 <= 2 * STAGE_BYTES, "reduction buffer must fit in the staging LDS");
    f32x4* red = reinterpret_cast<f32x4*>(smem) + ((wave & 3) * WNT * 4) * 64 + lane;
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[(i * 4 + j) * 64] = acc[i][j];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int i = 0; i < WNT; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += red[(i * 4 + j) * 64];
  }
  const bf16x4 no_pre[WNT][4] = {};
  const f32x4 no_bias[WNT] = {};
  gemm_epilogue<WNT, YT>(p, acc, m0, n0, wm, wn, frow, fq, bz, sid, no_pre, false, no_bias, false);
}

// gemm_kernel<WNT, NSPLIT, AT, YT, CONV, NSPLIT>: fp32 A with the half-type product, or split-bf16 on 8 waves (two k-groups)
template <int WNT, bool CONV>
KernFn reg_kernel(const Launch& L) {
  if (L.ns == 1) return L.y_f32 ? gemm_kernel<WNT, 1, float, float, CONV, 1> : gemm_kernel<WNT, 1, float, bf16, CONV, 1>;
  if (L.a_f32) return gemm_kernel<WNT, 2, float, float, CONV, 2>;
  if constexpr (!CONV) return gemm_kernel<WNT, 2, bf16, float, false, 2>;
  return nullptr;
}

template <bool CONV>
KernFn reg_width(const Launch& L) {
  switch (L.wnt) {
    case 1: return reg_kernel<1, CONV>(L);
    case 4: return reg_kernel<4, CONV>(L);
    case 5: return reg_kernel<5, CONV>(L);
    default: return nullptr;
  }
}

}  // namespace
