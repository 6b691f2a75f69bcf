// conv3_rowhalo_kernel (gfx950): 3x3 / stride 1 / pad 1 implicit-GEMM conv whose three taps of a kernel row share one halo'd row buffer.
//
// 3x3 / stride 1 / pad 1 convs whose image width divides 128 (16, 32, 64, 128: every UNet level above 8x8), chunk-major K.
// The plain implicit GEMM stages the activation tile once per TAP (9 x 16 KB per 64-channel chunk) although the three taps
// of one kernel row read the same image rows shifted by one pixel.  Here a 128-pixel tile = R = 128 / W whole image rows;
// per (chunk, kernel row kh) ONE buffer of R x (W + 2) pixels (the rows with a one-pixel halo left and right, zero outside
// the image) is staged and the three taps kw = 0..2 read their A fragments from it at a pixel offset of kw.  Activation
// bytes staged per chunk 144 -> 51 KB, all staged bytes per k-tile 36 -> 26 KB: the K loop of these kernels is bound by the
// LDS-DMA fill (in-kernel laps: DMA issue 46 % of the conv K loop), not by MFMA issue.
// LDS: weight ring 2 x BN x 128 B as before + 2 row buffers of <= 20 KB = 74-78 KB, still two blocks per CU.  The row buffer of
// group g + 1 is filled during the three k-tiles of group g (its pieces are spread over them); every k-tile starts with
// s_waitcnt vmcnt(0) + s_barrier, so each piece has landed and is visible before its first reader and the buffer it
// overwrites (group g - 1's) has no reader left.
// NS = 2 (with KG = 2: eight waves, the second k-group multiplies the second 32-wide k-step, folded through LDS at the end): the
// split-bf16 fp32-class form on pre-split planes (VAE) - activation hi / lo row buffers and weight hi / lo ring, three MFMAs per
// fragment pair; 132 KB, one block per CU like the 4-plane kernel it replaces, but 43 instead of 64 KB staged per k-tile.
// Widths that are multiples of 128 (VAE levels 128..512) use one row SEGMENT of 128 pixels per tile (R = 1, halo = the
// neighbouring pixels of the same row).
// MT = 2: 256-row tiles on eight waves (4 x 2), one block per CU: the weight k-tile is staged once per 256 rows (31 KB per
// k-tile and 256 x BN outputs instead of 2 x 26 KB).
// MX (round 4, NS = 2 / KG = 2 only): the fp32-class product on ONE fp16 pass plus two cross terms at fp8 precision on the block-scaled MX
// matrix instruction.  Plane 0 of both operands is fp16 (x16 = half(x), w16 = half(w)); plane 1 holds, per 64-deep k-tile and row, 64 e4m3
// bytes of the fp16 value ("hi8", scaled by a power of two) followed by 64 e4m3 bytes of the remainder x - x16 ("lo8") - the same 128 bytes
// per row and k-tile as a second bf16 plane, so the staging code does not change.  acc += w16 x16 (v_mfma_f32_16x16x32_f16, the group's
// 32-deep k-step) + BOTH cross terms of the k-tile in ONE v_mfma_scale_f32_16x16x128_f8f6f4 per output tile: its 128-deep contraction is
// the concatenation [w_lo8 | w_hi8] . [x_hi8 | x_lo8] - lane block l >> 4 = 0, 1 reads the lo8 half of the weight row and the hi8 half of the
// pixel row, block 2, 3 the other halves (32 bytes per lane and fragment) - which needs the two terms' scale products to be equal (they are:
// lo8 is stored at 2^11 x the hi8 scale on both sides).  The k-groups share the cross work by weight row tiles.  Per 16 x 16 x 64: 2 x 18
// cycles per k-group + 33.5 in one of them instead of 3 x 2 x 18 (tools/probes/mx_layout.hip); the cross terms only need ~4 bits: emulated
// pixel L-inf of the full VAE decode 8e-5 against 2e-5 for bf16 x 3, bound 1e-3 (tools/vae_precision_emul.py); measured 1.9e-5.
// STATUS (round 4): correct (per-op rel-L2 7.5e-6 against 3.2e-6 for bf16 x 3; full VAE decode pixel L-inf 1.9e-5 against 2.0e-5) but 3-13 %
// SLOWER than bf16 x 3 on the VAE's shapes (decoder 3x3 convs of a batch of four, tools/mx_probe.py: 23.1 ms against 21.5), so the VAE does
// not use it by default (ops.VAE_MX).  What was measured on the way: a first form that paired two k-tiles per cross
// instruction (exec-masked half-wave gathers, operands held across the barrier) 23.6 ms; that form without its cross MFMAs 15.5 ms and with
// neither gathers nor cross MFMAs 15.4 ms - the main fp16 pass alone, a third of today's matrix work, is 28 % faster; the eight scaled
// instructions per k-tile and wave then cost 7.7 ms where their bare issue time (33.5 cycles each beside 16 x 18 for the main pass) predicts
// about 3: in this loop the block-scaled instruction is about twice as expensive as in a bare loop.  Next: e2m3 cross operands (19.5
// cycles per instruction) and 32 x 32 x 64 tiles.
// TAPS = 2 (p.up == 2): the conv behind a nearest-2x upsample as four 2x2 convs ON THE SOURCE GRID, one per output parity (a, b):
//   y[2i + a][2j + b] = sum_{u, v in {0, 1}} W'_ab[u][v] x[i + a - 1 + u][j + b - 1 + v]
// with W'_ab the sums of the 3x3 taps that read the same source pixel (crg_pack_weight CRG_PACK_CONV_UP2: [parity][Cout][Cin / 64][u][v][64],
// ldw = 4 Cin) - 4 / 9 of the multiplies of the gather form above.  The GEMM rows are VIRTUAL: mv = ((img * 4 + parity) * H + i) * W + j, i.e.
// a batch of 4 N source-sized images, so the row buffers are exactly those of a plain conv on H x W; a tile never straddles a parity
// (H W % TP == 0, host-checked), which makes the parity block-uniform.  A group is (chunk, kernel row kh = a + u): its TWO k-tiles read the
// row buffer at pixel offsets b and b + 1, and the next group's pieces are spread over two k-tiles instead of three (every k-tile still
// starts with vmcnt(0) + barrier: same hazard argument).  Only the output address differs in the epilogue (up2_out_row); split-K slabs and
// the GroupNorm statistics stay in mv order, which is per-sample contiguous.  rows / seg geometries only.
//
// This unit also compiles gemm_kernel (gemm_reg_kernel.h, 21 small instantiations) and exports its picker.  Reason: compiled in a unit of its
// own, conv3_rowhalo_kernel's eight unpaired TAPS = 3 instantiations come out with two scalar instructions of the epilogue in the other order
// (same size, registers and LDS; measured when gemm_conv.hip was split) - they share gemm_epilogue<WNT, YT, 4, false> with gemm_kernel and
// gemm_glds_kernel, and with either of those in the unit all 22 are byte-identical to what the single file gave.
#include "gemm_reg_kernel.h"

namespace {
using namespace crg_mm;
using crg_plan::Launch;

template <int WNT, typename YT, bool PAIR, int NS = 1, int KG = 1, int MT = 1, bool MX = false, int TAPS = 3>
__global__ __launch_bounds__(256 * KG * MT, (KG == 1 && MT == 1) ? 2 : 1) void conv3_rowhalo_kernel(GemmP p) {
  static_assert(TAPS == 3 || (TAPS == 2 && !MX), "TAPS: 3, or 2 for the sub-pixel form of the upsample conv (not on the MX arm)");
  static_assert(!PAIR || (sizeof(YT) == 2 && NS == 1), "paired columns: bf16 output, single-plane operands");
  static_assert(MT == 1 || (KG == 1 && NS == 1), "256-row tiles: single-plane operands, no in-block split-K");
  static_assert(!MX || (NS == 2 && KG == 2 && MT == 1), "MX: the split-plane form on two k-groups");
  constexpr int WMT = 4, NW = 4 * KG * MT;
  constexpr int TP = 128 * MT;  // tile pixels
  constexpr int BN = 32 * WNT;
  constexpr int WS_BYTES = BN * 128;
  constexpr int WRG = BN / 8;
  constexpr int WL = (WRG + NW - 1) / NW;
  constexpr int XI = ((MT == 2 ? 36 : 20) + NW - 1) / NW;  // row-buffer pieces (8 pixels = 1 KiB) per wave, group and plane: TP + 2 R pixels, W >= 16
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int kg = MT == 2 ? 0 : wave >> 2;
  const int wm = MT == 2 ? wave >> 1 : (wave & 3) >> 1, wn = wave & 1;
  // geometry lives on the OUTPUT grid (Ho x Wo; the nearest-2x upsampled image when p.up), sources are read at (h >> up, w >> up)
  // (TAPS == 2: the geometry is the SOURCE grid, images = (sample, parity) pairs)
  const int Wd = TAPS == 2 ? p.W : p.Wo, Hd = TAPS == 2 ? p.H : p.Ho, sh = (TAPS == 3 && p.up) ? 1 : 0;
  // three buffer geometries: rows (W divides the tile: R whole image rows, each with a zero / neighbour pixel left and right),
  // seg (W a multiple of the tile: one row segment) and lin (any other width: the TP + 2 pixels m0 - 1 .. m0 + TP in linear
  // pixel order; a tap that would wrap around an image row is zeroed in the A fragment instead of in the buffer)
  const bool lin = TAPS == 3 && p.halo_lin != 0;
  const bool seg = lin || Wd > TP;       // lin shares seg's addressing: buffer pixel b <-> linear pixel m0 - 1 + b
  const int WP = seg ? TP + 2 : Wd + 2;
  const int R = seg ? 1 : TP / Wd;
  const int xpix = R * WP;
  const int XP = (xpix + 7) >> 3;
  const int xbuf_bytes = XP * 1024;      // one plane of one row buffer
  char* const wring = smem;              // [stage][plane][BN x 128 B]
  char* const xbuf = smem + 2 * NS * WS_BYTES;  // [parity][plane][xbuf_bytes]

  int tile_m, tile_n, sid;
  block_to_tile(p, tile_m, tile_n, sid);
  const int m0 = tile_m * TP, n0 = tile_n * BN;
  const int bz = 0;
  const int par = TAPS == 2 ? (m0 / (Hd * Wd)) & 3 : 0;  // output parity (a, b) = (par >> 1, par & 1) of this tile
  const int par_a = par >> 1, par_b = par & 1;
  const bf16* Wp = p.w + (long)par * p.N * p.ldw;         // its slab of the parity weight image
  const long a_lo_off = NS == 2 ? reinterpret_cast<const bf16*>(p.a_lo) - reinterpret_cast<const bf16*>(p.a) : 0;
  const long w_lo_off = NS == 2 ? p.w_lo - p.w : 0;
  const bf16* zpage = p.zero_page;
  const int rsub = lane >> 3;
  const int clog = (lane & 7) ^ rsub;

  // row-buffer pieces of this lane: piece jp = wave + NW i covers buffer pixels 8 jp .. 8 jp + 7, this lane pixel 8 jp + rsub
  int xsrc[XI];        // source pixel index of (image, row 0, column w >> up), valid when a mask bit is set
  int xh[XI];          // output-grid row h of the buffer pixel: kernel row kh reads source row (h + kh - 1) >> up
  unsigned xmask[XI];  // bit kh: row h + kh - 1 inside the image (and pixel inside the tile / image / problem)
  {
    const int rows_total = p.M / Wd;  // N * H image rows
    const int row0 = m0 / Wd;
    const int w0 = m0 - row0 * Wd;    // first pixel of the segment (0 unless seg)
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int b = 8 * (wave + NW * i) + rsub;
      int grow, w;
      bool ok;
      if (lin) {
        const int pb = m0 - 1 + b;  // the pixel whose (kh - 1)-th row neighbour this buffer pixel holds
        ok = b < xpix && pb >= 0 && pb < p.M;
        grow = (pb < 0 ? 0 : pb) / Wd;
        w = pb - grow * Wd;
      } else {
        const int r = b / WP, col = b - r * WP;
        grow = row0 + r;
        w = w0 + col - 1;
        ok = b < xpix && grow < rows_total && w >= 0 && w < Wd;
      }
      const int img = grow / Hd, h = grow - img * Hd;
      unsigned msk = 0;
      if (ok) msk = (h >= 1 ? 1u : 0u) | 2u | (h + 1 < Hd ? 4u : 0u);
      xmask[i] = msk;
      xh[i] = h;
      xsrc[i] = (TAPS == 2 ? img >> 2 : img) * p.H * p.W + (w >> sh);
    }
  }
  bool wok[WL];
  long wrow_off[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q) {
    const int pos = (wave + NW * q) * 8 + rsub;
    const int n = n0 + (PAIR ? unpair_col<WNT>(pos) : pos);
    wok[q] = n < p.N && (wave + NW * q) < WRG;
    wrow_off[q] = (long)n * p.ldw;
  }
  // K slice of this block in (chunk, kernel row) groups of TAPS k-tiles (ks_q / ks_r are in groups for this kernel)
  const int g_begin = sid * p.ks_q + (sid < p.ks_r ? sid : p.ks_r);
  const int g_end = g_begin + p.ks_q + (sid < p.ks_r ? 1 : 0);

  auto stage_x = [&](int g, int slot) {  // this wave's pieces i with i % TAPS == slot of group g's row buffer(s)
    const int c = g / TAPS, kh = g - TAPS * c + par_a;
    const int cch = c * 64 + clog * 8;
    const bool second = cch >= p.C1;
    const bf16* base = reinterpret_cast<const bf16*>(second ? p.x2 : p.a);
    const int Cs = second ? p.C2 : p.C1;
    const int cs = second ? cch - p.C1 : cch;
    char* xb = xbuf + ((g - g_begin) & 1) * (NS * xbuf_bytes);
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      if (i % TAPS != slot) continue;
      const int jp = wave + NW * i;
      if (jp < XP) {  // wave-uniform
        const bool ok = (xmask[i] >> kh) & 1u;
        const bf16* src = ok ? base + (long)(xsrc[i] + ((xh[i] + kh - 1) >> sh) * p.W) * Cs + cs : zpage;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(xb + jp * 1024), 16, 0, 0);
        if constexpr (NS == 2) {
          const bf16* src2 = ok ? src + a_lo_off : zpage;
          __builtin_amdgcn_global_load_lds((gptr_t)src2, (lptr_t)(xb + xbuf_bytes + jp * 1024), 16, 0, 0);
        }
      }
    }
  };
  auto stage_w = [&](int kt, int buf) {  // weight k-tile kt (64 K-elements) of this block's BN rows
    char* ws = wring + buf * (NS * WS_BYTES);
    const long kc = (long)kt * BK + clog * 8;
#pragma unroll
    for (int q = 0; q < WL; ++q) {
      if ((wave + NW * q) < WRG) {  // wave-uniform
        const bf16* src = wok[q] ? Wp + wrow_off[q] + kc : zpage;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(ws + (wave + NW * q) * 1024), 16, 0, 0);
        if constexpr (NS == 2) {
          const bf16* src2 = wok[q] ? src + w_lo_off : zpage;
          __builtin_amdgcn_global_load_lds((gptr_t)src2, (lptr_t)(ws + WS_BYTES + (wave + NW * q) * 1024), 16, 0, 0);
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
  // buffer pixel of this lane's output pixels for tap kw = 0 (tap kw adds kw): output pixel (r, w) of the tile sits at r * WP + w
  int xb0[WMT];
#pragma unroll
  for (int j = 0; j < WMT; ++j) {
    const int ml = wm * 64 + j * 16 + frow;
    const int r = seg ? 0 : ml / Wd;
    xb0[j] = r * WP + (ml - r * Wd);
  }
  // lin: output pixels in the first / last image column must not see the wrapped neighbour (taps kw = 0 / kw = 2)
  unsigned edge = 0;  // bit j: first column, bit 8 + j: last column
  if (lin) {
#pragma unroll
    for (int j = 0; j < WMT; ++j) {
      const int m = m0 + wm * 64 + j * 16 + frow;
      const int wcol = m % Wd;
      edge |= (wcol == 0 ? 1u : 0u) << j;
      edge |= (wcol == Wd - 1 ? 1u : 0u) << (8 + j);
    }
  }

  // residual / bias prefetch: as in gemm_glds_kernel (unconditional loads on clamped addresses)
  bf16x4 rres[PAIR ? 1 : WNT][PAIR ? 1 : WMT];
  bf16x8 r2[PAIR ? (WNT / 2 > 0 ? WNT / 2 : 1) : 1][PAIR ? WMT : 1];
  bf16x4 r1[PAIR ? WMT : 1];
  f32x4 bpre[WNT];
  const bool pre_res = sizeof(YT) == 2 && p.res && p.splits == 1 && (p.ldr & 3) == 0 && (p.N & 3) == 0;
  const bool pre_bias = !MX && p.bias_mode == CRG_BIAS_COL && p.splits == 1 && (p.N & 3) == 0;  // (MX: no registers to spare: the epilogue loads it)
  if (kg == 0) {
    const int nb = n0 + wn * (16 * WNT);
    if (pre_res) {
      const bf16* Rp = reinterpret_cast<const bf16*>(p.res);
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int m = m0 + wm * 64 + j * 16 + frow;
        const bf16* Rm = Rp + (long)(m < p.M ? m : p.M - 1) * p.ldr;
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
    if (pre_bias) {
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int n = (PAIR && i < 2 * (WNT / 2)) ? nb + 32 * (i >> 1) + 8 * fq + 4 * (i & 1) : nb + 16 * i + 4 * fq;
        bpre[i] = *reinterpret_cast<const f32x4*>(p.bias + (n + 4 <= p.N ? n : p.N - 4));
      }
    }
  }

  if (g_begin < g_end) {
    stage_x(g_begin, 0);
    stage_x(g_begin, 1);
    if constexpr (TAPS == 3) stage_x(g_begin, 2);
    stage_w(TAPS * g_begin, 0);
  }
  // KG == 2: the two k-groups are the two waves of every SIMD (wave w and w + 4).  Run in lockstep they read their fragments together
  // and multiply together, and the matrix pipe idles during the reads.  The second group therefore runs its MFMAs ONE K-TILE LATE, from
  // fragments it keeps in registers across the barrier: per k-tile it first multiplies the previous k-tile's fragments (while its partner
  // reads) and then reads this k-tile's (while its partner multiplies) - MI355X_MICROARCH.md "Two waves per SIMD" item 9.  No extra LDS:
  // a slot is refilled one barrier after the group's reads of it have returned, as before.
#ifdef CRG_X3_NOSTAGGER
  constexpr bool STAG = false;
#else
  // (the 160-wide split-plane tile has no registers left for a loop-carried fragment set; neither has the MX form: with its cross operands
  //  loop-carried as well it spills 92 bytes per lane and measured 16 % slower than its lockstep loop)
  constexpr bool STAG = KG == 2 && WNT == 4 && !MX;
#endif
  constexpr bool LO = NS == 2 && !MX;  // a second bf16 plane multiplied on the same instruction (bf16 x 3)
  bf16x8 sxf[STAG ? WMT : 1], swf[STAG ? WNT : 1], sxl[STAG && LO ? WMT : 1], swl[STAG && LO ? WNT : 1];
  if constexpr (STAG) {
#pragma unroll
    for (int j = 0; j < WMT; ++j) { sxf[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; if constexpr (LO) sxl[j] = sxf[j]; }
#pragma unroll
    for (int i = 0; i < WNT; ++i) { swf[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; if constexpr (LO) swl[i] = swf[i]; }
  }
  // MX: cross-term operand registers (32 e4m3 bytes per lane and fragment): this k-group's weight row tiles [ci0, ci0 + CW) and all pixel tiles
  typedef int v8i __attribute__((ext_vector_type(8)));
  typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
  constexpr int CW = MX ? (WNT + 1) / 2 : 1;
  const int ci0 = kg * CW;
  v8i wc[CW], xc[MX ? WMT : 1];
  if constexpr (MX) {  // (the staggered group multiplies once before its first reads)
#pragma unroll
    for (int q = 0; q < CW; ++q) wc[q] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < WMT; ++j) xc[j] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const int mx_sa = MX ? p.mx_scale[0][0] : 0, mx_sb = MX ? p.mx_scale[0][1] : 0;  // E8M0 scales: W lo8 and X hi8 (= the hi8 x lo8 product)
  auto mx_reads = [&](const char* ws, const char* xs, int kw) {
    if constexpr (MX) {
      const int cwq = ((fq + 2) & 3) * 2, cxq = fq * 2;  // 16-byte chunks of the 128-byte record: W [lo8 | hi8] order, X [hi8 | lo8]
#pragma unroll
      for (int q = 0; q < CW; ++q) {
        const int i = ci0 + q < WNT ? ci0 + q : WNT - 1;
        const int row = wn * (16 * WNT) + i * 16 + frow;
        const u32x4 c0 = *reinterpret_cast<const u32x4*>(ws + WS_BYTES + lds_off(row, cwq));
        const u32x4 c1 = *reinterpret_cast<const u32x4*>(ws + WS_BYTES + lds_off(row, cwq + 1));
        wc[q] = v8i{(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
      }
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const u32x4 c0 = *reinterpret_cast<const u32x4*>(xs + xbuf_bytes + lds_off(xb0[j] + kw, cxq));
        const u32x4 c1 = *reinterpret_cast<const u32x4*>(xs + xbuf_bytes + lds_off(xb0[j] + kw, cxq + 1));
        xc[j] = v8i{(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
      }
      if (kw != 1 && lin) {  // block-uniform: a tap that would wrap around an image row contributes zeros
#pragma unroll
        for (int j = 0; j < WMT; ++j)
          if ((edge >> (kw == 0 ? j : 8 + j)) & 1u) xc[j] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };
  auto mx_cross = [&]() {
    if constexpr (MX) {
#pragma unroll
      for (int q = 0; q < CW; ++q) {
        if (ci0 + q < WNT) {  // wave-uniform (odd WNT: the second group has one row tile fewer)
#pragma unroll
          for (int j = 0; j < WMT; ++j) {
            // (acc[kg * CW + q] with a compile-time index in each arm: no dynamic register indexing)
            if (kg == 0) acc[q][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wc[q], xc[j], acc[q][j], 0, 0, 0, mx_sa, 0, mx_sb);
            else acc[(CW + q) < WNT ? CW + q : 0][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wc[q], xc[j], acc[(CW + q) < WNT ? CW + q : 0][j], 0, 0, 0, mx_sa, 0, mx_sb);
          }
        }
      }
    }
  };
  auto stag_mma = [&]() {
    if constexpr (STAG) {
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) {
          if constexpr (LO) {
            acc[i][j] = CRG_MFMA_16x16x32(swl[i], sxf[j], acc[i][j]);
            acc[i][j] = CRG_MFMA_16x16x32(swf[i], sxl[j], acc[i][j]);
          }
          if constexpr (MX) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, swf[i]), __builtin_bit_cast(h16x8, sxf[j]), acc[i][j], 0, 0, 0);
          else acc[i][j] = CRG_MFMA_16x16x32(swf[i], sxf[j], acc[i][j]);
        }
      mx_cross();
    }
  };
  int wbuf = 0;
  auto k_loop = [&](auto GBc) {
  constexpr bool GB = decltype(GBc)::value;
  for (int g = g_begin; g < g_end; ++g) {
    const char* xs = xbuf + ((g - g_begin) & 1) * (NS * xbuf_bytes);
#pragma unroll
    for (int kt = 0; kt < TAPS; ++kt) {
      const int kw = TAPS == 2 ? kt + par_b : kt;  // buffer pixel offset of this k-tile's tap
      wait_vmcnt<0>();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_setprio(2);
      if (kt < TAPS - 1 || g + 1 < g_end) stage_w(TAPS * g + kt + 1, wbuf ^ 1);
      if (g + 1 < g_end) stage_x(g + 1, kt);
      __builtin_amdgcn_s_setprio(0);
      const char* ws = wring + wbuf * (NS * WS_BYTES);
      if constexpr (STAG) {
        // one fragment set for both groups; only the ORDER differs: group 0 reads, then multiplies; group 1 multiplies (the
        // previous k-tile's fragments, zeros the first time), then reads
        auto stag_reads = [&]() {
#pragma unroll
          for (int j = 0; j < WMT; ++j) {
            const int off = lds_off(xb0[j] + kw, kg * 4 + fq);
            sxf[j] = *reinterpret_cast<const bf16x8*>(xs + off);
            if constexpr (LO) sxl[j] = *reinterpret_cast<const bf16x8*>(xs + xbuf_bytes + off);
          }
          if (kw != 1 && lin) {
#pragma unroll
            for (int j = 0; j < WMT; ++j) {
              if ((edge >> (kw == 0 ? j : 8 + j)) & 1u) {
                sxf[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if constexpr (LO) sxl[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
              }
            }
          }
#pragma unroll
          for (int i = 0; i < WNT; ++i) {
            const int off = lds_off(wn * (16 * WNT) + i * 16 + frow, kg * 4 + fq);
            swf[i] = *reinterpret_cast<const bf16x8*>(ws + off);
            if constexpr (LO) swl[i] = *reinterpret_cast<const bf16x8*>(ws + WS_BYTES + off);
          }
          mx_reads(ws, xs, kw);
        };
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (GB) {
          stag_mma();
          __builtin_amdgcn_sched_barrier(0);
          stag_reads();
          wait_lgkmcnt0();  // the reads have RETURNED before the next barrier lets the slot be refilled
        } else {
          stag_reads();
          __builtin_amdgcn_sched_barrier(0);
          stag_mma();
        }
      } else {
#pragma unroll
      for (int k2 = 0; k2 < 2 / KG; ++k2) {
        const int ks = KG == 2 ? kg : k2;
        bf16x8 xf[WMT], wf[WNT], xl[NS == 2 ? WMT : 1], wl[NS == 2 ? WNT : 1];
#pragma unroll
        for (int j = 0; j < WMT; ++j) {
          const int off = lds_off(xb0[j] + kw, ks * 4 + fq);
          xf[j] = *reinterpret_cast<const bf16x8*>(xs + off);
          if constexpr (NS == 2 && !MX) xl[j] = *reinterpret_cast<const bf16x8*>(xs + xbuf_bytes + off);
        }
        if (kw != 1 && lin) {  // block-uniform branch: nothing on the hot path of the other geometries
#pragma unroll
          for (int j = 0; j < WMT; ++j) {
            if ((edge >> (kw == 0 ? j : 8 + j)) & 1u) {
              xf[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
              if constexpr (NS == 2) xl[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
          }
        }
#pragma unroll
        for (int i = 0; i < WNT; ++i) {
          const int off = lds_off(wn * (16 * WNT) + i * 16 + frow, ks * 4 + fq);
          wf[i] = *reinterpret_cast<const bf16x8*>(ws + off);
          if constexpr (NS == 2 && !MX) wl[i] = *reinterpret_cast<const bf16x8*>(ws + WS_BYTES + off);
        }
        if constexpr (MX) {
          mx_reads(ws, xs, kw);
#pragma unroll
          for (int i = 0; i < WNT; ++i)
#pragma unroll
            for (int j = 0; j < WMT; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, wf[i]), __builtin_bit_cast(h16x8, xf[j]), acc[i][j], 0, 0, 0);
          mx_cross();
        } else {
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
      }
      }
      wbuf ^= 1;
    }
  }
  if constexpr (STAG && GB) stag_mma();  // the last k-tile's fragments
  };
  if (STAG && kg == 1) k_loop(std::integral_constant<bool, true>{});
  else k_loop(std::integral_constant<bool, false>{});
  if constexpr (KG == 2) {
    // fold the second k-group's partial tile into the first: [wave & 3][i][j][lane] f32x4 in the (now idle) weight ring / row buffers
    static_assert(KG == 1 || 4 * WNT * WMT * 64 * 16 <= 2 * NS * WS_BYTES + 2 * NS * 17 * 1024, "reduction buffer must fit in the block's LDS");
    __syncthreads();  // every wave is done reading (all DMA was retired by the last vmcnt(0))
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
  if constexpr (PAIR) {
    gemm_epilogue_pairs<WNT, WMT, 2, false, TAPS == 2>(p, acc, m0, n0, wm, wn, frow, fq, bz, r2, r1, pre_res, bpre, pre_bias);
  } else {
    gemm_epilogue<WNT, YT, WMT, TAPS == 2>(p, acc, m0, n0, wm, wn, frow, fq, bz, sid, rres, pre_res, bpre, pre_bias);
  }
}

// conv3_rowhalo_kernel<WNT, YT, PAIR, NS, KG, MT, MX, TAPS>
template <int WNT>
KernFn rowhalo_kernel(const Launch& L) {
  if (L.y_f32)  // pre-split planes
    return L.mx ? conv3_rowhalo_kernel<WNT, float, false, 2, 2, 1, true>
                : L.taps == 2 ? conv3_rowhalo_kernel<WNT, float, false, 2, 2, 1, false, 2> : conv3_rowhalo_kernel<WNT, float, false, 2, 2>;
  if (L.mt == 2) {
    if (L.taps == 2) return L.pair ? conv3_rowhalo_kernel<WNT, bf16, true, 1, 1, 2, false, 2> : conv3_rowhalo_kernel<WNT, bf16, false, 1, 1, 2, false, 2>;
    return L.pair ? conv3_rowhalo_kernel<WNT, bf16, true, 1, 1, 2> : conv3_rowhalo_kernel<WNT, bf16, false, 1, 1, 2>;
  }
  if (L.taps == 2) return L.pair ? conv3_rowhalo_kernel<WNT, bf16, true, 1, 1, 1, false, 2> : conv3_rowhalo_kernel<WNT, bf16, false, 1, 1, 1, false, 2>;
  return L.pair ? conv3_rowhalo_kernel<WNT, bf16, true> : conv3_rowhalo_kernel<WNT, bf16, false>;
}

}  // namespace

namespace crg_mm {
KernFn pick_reg(const Launch& L, bool conv) { return conv ? reg_width<true>(L) : reg_width<false>(L); }
KernFn pick_rowhalo(const Launch& L) {  // 128- / 160-wide tiles only
  switch (L.wnt) {
    case 4: return rowhalo_kernel<4>(L);
    case 5: return rowhalo_kernel<5>(L);
    default: return nullptr;
  }
}
}  // namespace crg_mm
