"""Shapes of the temporal-kernel tests (tests/test_svd_ops_gpu.py) and a numpy twin of the address arithmetic of cremage_amd/csrc/video.hip.

The twin restates, index for index, which element offsets `conv_frames_kernel` and `attn_frames_kernel` generate - global reads and
writes and the LDS positions - so that tests/test_svd_cpu.py can assert, without a GPU, that every one of them lies inside its operand
for every shape the GPU tests launch (frame offsets r +- S, the per-pixel frame stride, T = 1, b = 1 and the S tails included)."""
import numpy as np

# (b, T, S, Cin, Cout)
CONV_CASES = [(1, 1, 16, 32, 32), (2, 2, 40, 32, 64), (2, 3, 9, 64, 32), (1, 14, 72, 320, 320), (2, 25, 24, 1280, 640)]
# (b, T, S, heads, d)
ATTN_CASES = [(1, 1, 8, 1, 16), (2, 3, 128, 2, 16), (1, 14, 40, 5, 64), (2, 25, 72, 5, 64), (1, 32, 9, 1, 64)]

BM, BK = 128, 64


def conv_wnt(cout):
    """tile width / 32 as crg_conv_frames picks it: from Cout alone"""
    return 4 if cout % 128 == 0 else 2 if cout % 64 == 0 else 1


def conv_frames_offsets(b, T, S, Cin, Cout):
    """Every LDS-DMA source the kernel selects.  Returns dict of arrays over (tile row m, 8-channel chunk kc8):
    x_sel (bool: read from x, else the zero page), x_off (element offset into x), tap, plus the weight side and the LDS extents."""
    M, N, K = b * T * S, Cout, 3 * Cin
    wnt = conv_wnt(Cout)
    BN = 32 * wnt
    tiles_m, tiles_n, nk = -(-M // BM), -(-N // BN), -(-K // BK)
    stage_bytes = BM * 128 + BN * 128
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
    # LDS: destination of the DMA pieces (row group g of 8 rows -> 1 KiB at g * 1024, lane * 16 inside) and the fragment reads
    rows = np.arange(BM)
    chunks = np.arange(8)
    lds_read = rows[:, None] * 128 + ((chunks[None, :] ^ (rows[:, None] & 7)) << 4)
    return dict(M=M, N=N, K=K, x_sel=x_sel, x_off=x_off, tap=np.broadcast_to(tap2, x_sel.shape), kok=kok, m=m, w_sel=w_sel, w_off=w_off,
                lds_bytes=2 * stage_bytes, x_dma_end=(BM // 8 - 1) * 1024 + 63 * 16 + 16, w_dma_end=BM * 128 + (BN // 8 - 1) * 1024 + 63 * 16 + 16,
                stage_bytes=stage_bytes, x_read_end=int(lds_read.max()) + 16, xs_bytes=BM * 128,
                y_end=(M - 1) * N + (N - 4) + 4)


def attn_frames_offsets(b, T, S, H, d, esize, ld):
    """Per block of the launch: the element offsets of the q / k / v / o accesses (rows of `ld` elements, head h at column h * d) and
    the LDS byte extents.  Yields dicts; DP and the block geometry as launch_attn_frames sets them."""
    DP = 16 if d <= 16 else 32 if d <= 32 else 64
    G = 256 // T
    rowb = DP * esize + 16
    rows = G * T
    SH = S * H
    lds = 2 * rows * rowb
    ppr = d * esize // 16
    epp = 16 // esize
    for vb in range(b):
        for bx in range(-(-SH // G)):
            g0 = bx * G
            tid = np.arange(256, dtype=np.int64)
            g, t = tid // T, tid % T
            gg = g0 + g
            active = (g < G) & (gg < SH)
            px, hd = gg // H, gg % H
            qrow = (vb * T + t) * S + px
            c = np.arange(DP // 8, dtype=np.int64)
            cm = (c * 8 < d)
            q_off = (qrow[:, None] * ld + hd[:, None] * d + c[None, :] * 8)[active][:, cm]
            i = np.arange(rows * ppr, dtype=np.int64)
            row, pc = i // ppr, i % ppr
            rg, rt = row // T, row % T
            rgg = g0 + rg
            st = rgg < SH
            rpx, rhd = rgg // H, rgg % H
            r = (vb * T + rt) * S + rpx
            kv_off = (r * ld + rhd * d + pc * epp)[st]
            lds_st = (row * rowb + pc * 16)[st] + rows * rowb  # the V half is the upper one
            lds_rd = ((g * T)[active][:, None] + np.arange(T)[None, :]) * rowb + rows * rowb + (int(cm.sum()) - 1) * 8 * esize + 8 * esize
            yield dict(q_off=q_off, q_rows=qrow[active], kv_off=kv_off, kv_rows=r[st], lds=lds, lds_st_end=lds_st + 16, lds_rd_end=lds_rd,
                       video=vb, epp=epp, staged_rows=np.unique(row[st]), read_rows=np.unique((g * T)[active][:, None] + np.arange(T)[None, :]))
