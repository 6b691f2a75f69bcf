"""Shapes of the video-VAE kernel tests (tests/test_svd_vae_ops_gpu.py) and a numpy twin of the address arithmetic of
cremage_amd/csrc/video_x3.hip.

The twin restates, index for index, which element offsets `conv_frames_x3_kernel` and `conv_frames_thin_kernel` generate - the LDS-DMA
sources in both activation planes and both weight planes, the LDS positions of the four planes of a stage, the fp32 epilogue accesses,
and the thin kernel's per-pixel reads - so that tests/test_svd_vae_cpu.py can hold every one of them inside its operand and inside the
row's own video without a GPU, for every shape the GPU tests launch.

The twin is a restatement: whoever changes the kernel's tiling, staging or epilogue mapping edits this file in the same change.
tests/test_svd_vae_cpu.py::test_twin_constants_are_the_kernels reads the constants below back from the kernel's source, so a changed tile
height, k-tile depth, stage layout or block residency fails there until the twin follows."""
import numpy as np

# (b, T, S, Cin, Cout)
X3_CASES = [(2, 3, 129, 128, 128), (1, 1, 64, 128, 256), (2, 5, 200, 256, 128), (1, 4, 128, 512, 512), (1, 2, 1, 96, 32)]
# further launches of the GPU tests: isolation (the compared video between two NaN ones) and batch position
X3_EXTRA = [(3, 3, 129, 128, 128), (1, 3, 129, 128, 128), (3, 2, 1, 96, 32), (1, 5, 200, 256, 128), (3, 5, 200, 256, 128)]
X3_TAILS = [(1, 1, 1, 32, 32), (1, 1, 129, 96, 64), (3, 1, 1, 96, 96), (1, 7, 129, 96, 160), (2, 2, 1, 32, 64)]
# (b, T, S, C)
THIN_CASES = [(b, T, S, C) for C in (3, 4) for T in (1, 2, 5) for S in (1, 129) for b in (2,)]
THIN_EXTRA = [(3, T, S, 3) for T in (1, 2, 5) for S in (1, 129)] + [(1, T, S, 3) for T in (1, 2, 5) for S in (1, 129)]
THIN_TAILS = [(1, 1, 1, 1), (1, 1, 1, 8), (2, 3, 257, 8), (1, 4, 300, 5)]

BM, BK = 128, 64     # CF_BM of video_x3.hip, crg_mm::BK of gemm_shared.h
BLOCKS_PER_CU = 2     # __launch_bounds__(256, 2): one stage of four planes per block, two blocks share the CU's LDS


def x3_wnt(cout):
    """tile width / 32 as crg_conv_frames_x3 picks it: from Cout alone"""
    return 4 if cout % 128 == 0 else 2 if cout % 64 == 0 else 1


def conv_frames_x3_offsets(b, T, S, Cin, Cout):
    """Every LDS-DMA source the kernel selects (the SAME element offset is added to the hi and to the lo plane), the byte extents of the
    four planes of a stage in LDS, and the epilogue's fp32 offsets."""
    M, N, K = b * T * S, Cout, 3 * Cin
    wnt = x3_wnt(Cout)
    BN = 32 * wnt
    tiles_m, tiles_n, nk = -(-M // BM), -(-N // BN), -(-K // BK)
    xs_bytes, ws_bytes = BM * 128, BN * 128
    stage_bytes = 2 * (xs_bytes + ws_bytes)
    # per lane: logical chunk clog, running (tap, cch) exactly as the kernel advances them (no division)
    tap_of = np.zeros(nk * 8, dtype=np.int64)
    cch_of = np.zeros(nk * 8, dtype=np.int64)
    for clog in range(8):
        kc, tap, cch = clog * 8, 0, clog * 8
        while cch >= Cin:
            cch -= Cin
            tap += 1
        for kt in range(nk):
            tap_of[kt * 8 + clog], cch_of[kt * 8 + clog] = tap, cch
            kc += BK
            cch += BK
            while cch >= Cin:
                cch -= Cin
                tap += 1
    kc = np.arange(nk * 8, dtype=np.int64) * 8
    kok = kc < K
    m = np.arange(tiles_m * BM, dtype=np.int64)
    fr = (m // S) % T
    xok, xprev, xnext = m < M, fr > 0, fr + 1 < T
    tap2, cch2 = tap_of[None, :], cch_of[None, :]
    x_sel = kok[None, :] & xok[:, None] & ((tap2 == 1) | np.where(tap2 == 0, xprev[:, None], xnext[:, None]))
    x_off = m[:, None] * Cin + (tap2 - 1) * (S * Cin) + cch2
    n = np.arange(tiles_n * BN, dtype=np.int64)
    w_sel = kok[None, :] & (n < N)[:, None]
    w_off = n[:, None] * K + kc[None, :]
    # LDS-DMA destinations inside a stage: row group g of 8 rows -> 1 KiB at g * 1024 (+ lane * 16) of its plane
    x_groups, w_groups = np.arange(BM // 8), np.arange(BN // 8)
    dma = dict(x_hi=x_groups * 1024, x_lo=xs_bytes + x_groups * 1024, w_hi=2 * xs_bytes + w_groups * 1024,
               w_lo=2 * xs_bytes + ws_bytes + w_groups * 1024)
    planes = dict(x_hi=(0, xs_bytes), x_lo=(xs_bytes, 2 * xs_bytes), w_hi=(2 * xs_bytes, 2 * xs_bytes + ws_bytes),
                  w_lo=(2 * xs_bytes + ws_bytes, stage_bytes))
    # fragment reads: row r of a plane, logical chunk c -> r * 128 + ((c ^ (r & 7)) << 4)
    chunks = np.arange(8)
    x_rows = np.arange(BM)
    w_rows = np.arange(BN)
    x_read = x_rows[:, None] * 128 + ((chunks[None, :] ^ (x_rows[:, None] & 7)) << 4)
    w_read = w_rows[:, None] * 128 + ((chunks[None, :] ^ (w_rows[:, None] & 7)) << 4)
    # epilogue: lane (frow, fq) of wave (wm, wn): rows m0 + wm * 64 + j * 16 + frow, columns n0 + wn * 16 wnt + i * 16 + fq * 4 .. + 3
    em = (np.arange(tiles_m)[:, None, None, None] * BM + np.arange(2)[None, :, None, None] * 64 + np.arange(4)[None, None, :, None] * 16
          + np.arange(16)[None, None, None, :]).reshape(-1)
    en = (np.arange(tiles_n)[:, None, None, None] * BN + np.arange(2)[None, :, None, None] * (16 * wnt) + np.arange(wnt)[None, None, :, None] * 16
          + np.arange(4)[None, None, None, :] * 4).reshape(-1)
    em, en = em[em < M], en[en < N]
    y_off = em[:, None] * N + en[None, :]
    return dict(M=M, N=N, K=K, x_sel=x_sel, x_off=x_off, tap=np.broadcast_to(tap2, x_sel.shape), kok=kok, m=m, w_sel=w_sel, w_off=w_off,
                lds_bytes=stage_bytes, stage_bytes=stage_bytes, dma=dma, planes=planes, x_read=x_read, w_read=w_read,
                xs_bytes=xs_bytes, ws_bytes=ws_bytes, y_off=y_off, y_frame=em // S)


def conv_frames_thin_offsets(b, T, S, C):
    """Per pixel row m and tap d: whether the kernel reads row m + (d - 1) S, and that row; the write row; the launch's thread count."""
    M = b * T * S
    threads = -(-M // 256) * 256
    m = np.arange(threads, dtype=np.int64)
    live = m < M
    fr = (m // S) % T
    d = np.arange(3)
    sel = live[:, None] & ((d[None, :] == 1) | np.where(d[None, :] == 0, (fr > 0)[:, None], (fr + 1 < T)[:, None]))
    row = m[:, None] + (d[None, :] - 1) * S
    CP = 4 if C <= 4 else 8
    w_src = np.array([(co * C + ci) * 3 + dd for dd in range(3) for co in range(CP) for ci in range(CP) if co < C and ci < C], dtype=np.int64)
    return dict(M=M, m=m, live=live, sel=sel, row=row, w_src=w_src, w_lds=3 * CP * CP, CP=CP)
