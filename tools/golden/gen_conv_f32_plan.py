"""Generator of tests/golden/conv_f32_plan.npz: the launch plan of the fp32 convolution family (csrc/conv_f32_plan.h) over a sweep that puts
a row on either side of every comparison of the selection.  Run from the repository root, for the day a routing change is INTENDED:

    python -m tools.golden.gen_conv_f32_plan [path of a library that exports fmi_conv2d_f32_plan]

The library defaults to the built libfmi_hip.so; a g++ -DFMI_HOST_EMU build of csrc/conv.hip + csrc/gemm.hip serves as well (no GPU is
used).  The committed table was NOT made by this program but from the selection text as it was before the plan header existed: see
profiles/conv_f32_dispatch.txt.  `sweep()` is the list of inputs, shared with whatever evaluates them.

Table (numpy .npz): in_cols / out_cols, the names of a row's inputs and outputs; rows, int32 [rows][inputs..., outputs...].
  inputs   pass (0 forward, 1 adjoint, 2 weight gradient, 3 the ResBlock pair), flags (FMI_F32_PLAN_* of include/fmi_hip.h, always with
           FMI_F32_PLAN_MODES: reproducible mode and FMI_DMA_OFF are the row's, not the process's; THIN_OUT / THIN_IN hold what the thin
           kernels' predicates answer for the descriptor), C2 (pair), then the descriptor
  outputs  out[0..43] of fmi_conv2d_f32_plan
"""
from __future__ import annotations

import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
OUT = os.path.join(ROOT, "tests", "golden", "conv_f32_plan.npz")
IN_COLS = ["pass", "flags", "C2", "N", "H", "W", "C", "K", "kh", "kw", "stride", "pad", "dil", "pad_mode", "x_cstride", "y_cstride"]
LAUNCH_COLS = ["route", "tile", "dma", "fl", "init", "ksplit", "chunk", "grid_x", "grid_y", "code"]
OUT_COLS = ["status", "launches", "early", "bits"] + [f"{c}{p}" for p in range(4) for c in LAUNCH_COLS]
X_AL16, W_AL16, OUT_AL16, RES, RES_AL16, X3, X3_AL16, W3, W3_AL16, Y3, Y3_AL16 = 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
BIAS, MASK, ACT, BATCH_W, DET, MODES, DMA_SHIFT, THIN_OUT, THIN_IN = 0x800, 0x1000, 0x2000, 0x4000, 0x8000, 0x10000, 17, 0x100000, 0x200000
AL = X_AL16 | W_AL16 | OUT_AL16 | MODES  # every fp32 operand aligned
P3X, P3W, P3Y = X3 | X3_AL16, W3 | W3_AL16, Y3 | Y3_AL16
(GEMM, GEMM_W3, GEMM_P3, C3, C3_W3, C3_P3, CONVT3X3, WGRAD_GEMM, WGRAD_P3, WGRAD_P3_3X3, THIN_OUT_ROUTE, THIN_IN_ROUTE) = range(1, 13)
# shapes of the pair that tests/test_host_resblock_pair.py asserts: (N, H = W, C = C2, K)
PAIR_ASSERTED = [(8, 32, 128, 128), (8, 32, 128, 256), (8, 16, 128, 128), (8, 8, 128, 128), (8, 128, 32, 64), (8, 64, 64, 128), (8, 64, 128, 128),
                 (8, 128, 64, 128), (2, 8, 64, 64), (1, 1, 64, 64), (2, 8, 16, 16), (8, 128, 16, 32)]


def row(pass_, flags, n, h, w, c, k, ksz=1, stride=1, pad=0, dil=1, pad_mode=0, xcs=None, ycs=None, c2=0):
    return [pass_, flags, c2, n, h, w, c, k, ksz, ksz, stride, pad, dil, pad_mode, c if xcs is None else xcs, k if ycs is None else ycs]


def line(pass_, m, c, k, flags, ksz=1, **kw):
    """a 1 x m map: m pixels; 3x3 with pad 1 keeps the size"""
    return row(pass_, flags, 1, 1, m, c, k, ksz, 1, ksz // 2, **kw)


def around(bm, bn, thr, ncols, factor=1):
    """row counts that put ceil(M / bm) * ceil(ncols / bn) * factor just below, and twice at, thr"""
    tn = -(-ncols // bn)
    tm = -(-thr // (tn * factor))
    return [m for m in ((tm - 1) * bm, (tm - 1) * bm + 1, tm * bm) if m > 0]


def sweep():
    rows = []
    # ---- the tile tables: N <= 32 / <= 64 / > 64, the 384 / 800 / 256 workgroup thresholds, the M > 64 / M > 32 terms (ACT: never split) ----
    for ncols in (32, 36, 64, 68, 128, 132, 256):
        ms = {1, 32, 33, 64, 65, 128, 129}
        for bm, bn, thr in ((128, 64, 384), (128, 128, 800), (64, 128, 384), (32, 128, 256), (256, 128, 256), (256, 64, 256)):
            ms.update(around(bm, bn, thr, ncols))
        for m in sorted(ms):
            for p in (0, 1):
                cin, cout = (64, ncols) if p == 0 else (ncols, 64)
                rows.append(line(p, m, cin, cout, AL | ACT))                        # GEMM, LDS-DMA
                rows.append(line(p, m, cin, cout, AL | ACT | P3W))                  # GEMM_W3
                rows.append(line(p, m, cin, cout, AL | ACT | P3W | P3X))            # GEMM_P3
                rows.append(line(p, m, cin, cout, AL | ACT, ksz=3))                 # C3
                rows.append(line(p, m, cin, cout, AL | ACT | P3W, ksz=3))           # C3_W3 / C3
                rows.append(line(p, m, cin, cout, AL | ACT | P3W | P3X, ksz=3))     # C3_P3
                # the same tables in reproducible mode with a long reduction (blocked accumulation), on the register-staged kernels
                # (a misaligned image; FMI_DMA_OFF bit 1 under weight pieces)
                cin, cout = (656, ncols) if p == 0 else (ncols, 656)
                for bits in (AL | DET, AL | DET | P3W, AL | DET | P3W | P3X, (AL | DET) & ~X_AL16, AL | P3W | (2 << DMA_SHIFT)):
                    rows.append(line(p, m, cin, cout, bits))
                cin, cout = (80, ncols) if p == 0 else (ncols, 80)
                rows.append(line(p, m, cin, cout, AL | DET, ksz=3))
    # ---- conv_ksplit: K 512 / 2304 / 4608, tiles 192 / 320 / 520 / 800, the weight-streaming case; the init launch; reproducible mode ----
    for c in (496, 512, 2288, 2304, 4592, 4608, 8192):
        for tiles in (1, 2, 16, 17, 24, 100, 191, 192, 319, 320, 520, 521, 799, 800):
            for bits in (AL, AL | DET, AL | ACT, AL | P3W, AL | P3W | P3X):
                rows.append(line(0, 128 * tiles, c, 128, bits))
                rows.append(line(1, 128 * tiles, 128, c, bits))
        for m, ncols in ((128, 2048), (128, 2176), (129, 128), (64, 512), (16, 512), (1, 512)):
            rows.append(line(0, m, c, ncols, AL))
    for c in (64, 128, 256, 512):  # 3x3: K = 9 C; the it_chunk normalisation
        for tiles in (1, 4, 16, 17, 100, 192, 320, 521, 800):
            for bits in (AL, AL | DET, AL | P3W, AL | P3W | P3X, AL | P3W | P3X | DET):
                rows.append(line(0, 128 * tiles, c, 128, bits, ksz=3))
                rows.append(line(1, 128 * tiles, 128, c, bits, ksz=3))
    # ---- blocked accumulation: kchunk 640 / 656, it_chunk 12 / 15 (C 64 / 80), both modes; the eight-wave piece tiles take it in either ----
    for c in (640, 656):
        for bits in (AL | DET, AL, AL | DET | P3W, AL | DET | P3W | P3X, AL | DET | (2 << DMA_SHIFT)):
            rows.append(line(0, 4096, c, 128, bits))
    for c in (64, 80):
        for m in (4096, 70000):
            for bits in (AL | DET, AL, AL | DET | P3W, AL | P3W | P3X, AL | DET | P3W | P3X):
                for k in (64, 128):
                    rows.append(line(0, m, c, k, bits, ksz=3))
    # ---- operand facts: alignment, pitch, padding, dilation, per-sample weights, channel multiples ----
    for ksz in (1, 3):
        for c, k in ((3, 8), (16, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 62), (24, 16), (48, 128)):
            for bits in (AL, AL & ~X_AL16, AL & ~W_AL16, AL | P3W, AL | W3, AL | P3W | P3X, AL | P3W | X3, AL | P3X, AL | P3W | P3X | P3Y, AL | Y3, AL | ACT):
                rows.append(row(0, bits, 2, 8, 8, c, k, ksz, 1, ksz // 2))
                rows.append(row(1, bits, 2, 8, 8, c, k, ksz, 1, ksz // 2))
            rows.append(row(0, AL | P3W | P3X, 2, 8, 8, c, k, ksz, 1, ksz // 2, xcs=c + 4))
            rows.append(row(0, AL | P3W, 2, 8, 8, c, k, ksz, 1, ksz // 2, xcs=c + 1))
            rows.append(row(1, AL | P3W | P3X, 2, 8, 8, c, k, ksz, 1, ksz // 2, ycs=k + 4))
            rows.append(row(0, AL | BATCH_W | P3W | P3X, 4, 8, 8, c, k, ksz, 1, ksz // 2))
            rows.append(row(1, AL | BATCH_W, 4, 8, 8, c, k, ksz, 1, ksz // 2))
            rows.append(row(0, AL | RES | RES_AL16 | BIAS, 2, 8, 8, c, k, ksz, 1, ksz // 2))
            rows.append(row(1, AL | MASK, 2, 8, 8, c, k, ksz, 1, ksz // 2))
            rows.append(row(1, AL | MASK | BIAS, 2, 8, 8, c, k, ksz, 1, ksz // 2))
        for bits in (AL, AL | P3W | P3X):
            rows.append(row(0, bits, 2, 8, 8, 64, 64, 3, 1, 1, pad_mode=1))   # reflect padding
            rows.append(row(1, bits, 2, 8, 8, 64, 64, 3, 1, 1, pad_mode=1))   # refused
            rows.append(row(0, bits, 2, 8, 8, 64, 64, 3, 1, 2, dil=2))        # dilation 2
            rows.append(row(1, bits, 2, 8, 8, 64, 64, 3, 1, 2, dil=2))
            rows.append(row(1, bits, 2, 9, 9, 64, 64, 3, 2, 2, dil=2))        # dilated and strided: refused
    # ---- FMI_DMA_OFF bits 1, 2, 4 ----
    for off in (1, 2, 4):
        for bits in (AL, AL | P3W):
            rows.append(line(0, 4096, 64, 128, bits | (off << DMA_SHIFT)))
            rows.append(line(1, 4096, 64, 128, bits | (off << DMA_SHIFT)))
        rows.append(line(2, 4096, 64, 128, AL | (off << DMA_SHIFT)))
        rows.append(row(3, AL | (off << DMA_SHIFT), 8, 32, 32, 32, 64, 3, 1, 1, c2=32))
    # ---- strided adjoints: with and without the shared init; the one-launch ConvTranspose at its bounds (32768 pixels, C <= 64) ----
    for h in (2, 4, 8, 32, 64):
        for c, k in ((512, 512), (64, 128), (128, 64)):
            for bits in (AL, AL | DET, AL | P3W, AL | P3W | P3X, AL | BATCH_W):
                rows.append(row(1, bits, 2, h, h, c, k, 3, 2, 1))
    rows.append(row(1, AL, 1, 1, 7, 64, 64, 3, 2, 1))    # phases without pixels
    rows.append(row(1, AL, 1, 8, 8, 64, 512, 1, 2, 0))   # phases without taps
    rows.append(row(1, AL, 1, 9, 9, 64, 64, 3, 3, 0))    # stride 3: nine phases
    for w in (126, 128):
        for c in (60, 64, 68, 128):
            for k in (64, 72):
                for bits in (AL | P3W, AL, AL | W3, AL | P3W | P3X, AL | P3W | X3, (AL | P3W) & ~X_AL16, AL | P3W | MASK, AL | P3W | BIAS | RES | RES_AL16, AL | P3W | BATCH_W):
                    rows.append(row(1, bits, 8, 128, w, c, k, 3, 2, 1))
    rows.append(row(1, AL | P3W, 8, 128, 128, 64, 64, 3, 2, 1, ycs=66))
    # ---- the thin kernels' early exits ----
    for p in (0, 1, 2):
        for n, h, w in ((1, 8, 32), (2, 130, 70), (1, 3, 3), (1, 2, 8)):
            for bits in (AL, AL & ~X_AL16, AL & ~OUT_AL16, AL | BIAS, AL | BATCH_W):
                rows.append(row(p, bits, n, h, w, 32, 3, 3, 1, 1))
        for n, h, w, c, k, ks in ((1, 256, 512, 3, 32, 3), (2, 260, 253, 3, 64, 3), (1, 512, 256, 3, 32, 1), (1, 256, 511, 3, 32, 3), (2, 40, 36, 3, 64, 3)):
            for bits in (AL, AL | RES, AL | RES | RES_AL16, AL & ~OUT_AL16, AL | THIN_IN, AL | THIN_IN | BIAS):
                if p == 1 or not bits & THIN_IN:  # only the adjoint's THIN_IN is an input
                    rows.append(row(p, bits, n, h, w, c, k, ks, 1, ks // 2))
    # ---- weight gradient: four routes, P / 512, the XCD rounding (6 -> 8), 8 splits in x, the bias row, per-sample weights, reproducible mode ----
    for c, k, ksz in ((64, 64, 3), (64, 128, 3), (128, 256, 3), (32, 64, 3), (64, 64, 1), (64, 128, 1), (256, 32, 1), (3, 64, 3), (3, 64, 1), (30, 20, 1), (512, 512, 3)):
        for px in (256, 511, 512, 1024, 2559, 2560, 3071, 3072, 3584, 4096, 16384, 65536, 1 << 20):
            for bits in (AL, AL | BIAS, AL | P3X | P3Y, AL | P3X | P3Y | BIAS, AL | DET, AL | DET | P3X | P3Y, AL | P3X | Y3, AL & ~X_AL16, AL & ~W_AL16):
                rows.append(row(2, bits, 1, px // 16 if px % 16 == 0 else 1, 16 if px % 16 == 0 else px, c, k, ksz, 1, ksz // 2))
        for bits in (AL | BATCH_W, AL | BATCH_W | BIAS):
            rows.append(row(2, bits, 4, 64, 64, c, k, ksz, 1, ksz // 2))
        rows.append(row(2, AL | P3X | P3Y, 1, 64, 8, c, k, ksz, 1, ksz // 2))      # W < 16
        rows.append(row(2, AL | P3X | P3Y, 2, 64, 64, c, k, ksz, 2, ksz // 2))     # stride 2
    for c, k in ((49152, 64), (49024, 64), (102400, 128), (102272, 128)):          # the weight gradient's 128 x 64 / 128 x 128 tiles: 384 / 800 tiles
        for bits in (AL, AL | DET, AL & ~X_AL16):
            rows.append(row(2, bits, 1, 1, 1024, c, k))
    rows.append(row(2, AL | BATCH_W, 70000, 1, 1, 16, 16, 1, 1, 0))              # per-sample weights beyond the grid's y
    # ---- the ResBlock pair: the asserted shapes, both sides of its 2048 / 16384 / 32768 pixel bounds, the split ----
    for n, h, c, k in PAIR_ASSERTED:
        for bits in (AL, AL | P3W, AL | ACT, AL | DET, AL | BIAS):
            rows.append(row(3, bits, n, h, h, c, k, 3, 1, 1, c2=c))
    for px in (2048, 2049, 16383, 16384, 32768, 32769):
        for c, k in ((128, 128), (64, 128), (32, 64), (16, 64), (128, 256)):
            rows.append(row(3, AL, 1, 1, px, c, k, 3, 1, 1, c2=c))
    for h in (4, 8, 16):
        for c, k, c2 in ((128, 128, 128), (256, 128, 64), (512, 512, 256), (32, 64, 32), (64, 32, 16)):
            for bits in (AL, AL | P3W, AL | DET | P3W, AL | ACT):
                rows.append(row(3, bits, 2, h, h, c, k, 3, 1, 1, c2=c2))
    rows.append(row(3, AL, 2, 8, 8, 64, 64, 3, 2, 1, c2=64))  # refused
    rows.append(row(3, AL, 2, 8, 8, 64, 64, 3, 1, 1, c2=24))
    rows += gpu_rows()
    seen, uniq = set(), []
    for r in rows:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            uniq.append(r)
    return uniq


# what the GPU tests prove or assert, as rows: CASES of tests/test_gpu_p3.py (forward and adjoint from piece images; the weight gradient's
# list there), the routed shapes of tests/test_gpu_thin_in.py and SHAPES of tests/test_gpu_thin_paths.py (32 -> 3).  The host test takes the
# shapes from those files, not from here.
P3_CASES = [(2, 64, 64, 40, 36, 3, 1, 1), (1, 128, 192, 33, 31, 3, 1, 1), (2, 256, 128, 16, 16, 3, 1, 1), (2, 64, 128, 24, 24, 1, 1, 0),
            (2, 64, 64, 32, 32, 3, 2, 1), (1, 32, 64, 20, 20, 3, 1, 1), (1, 64, 32, 64, 64, 3, 1, 1), (8, 128, 128, 64, 64, 3, 1, 1)]
THIN_IN_ROUTES = [(1, 3, 32, 256, 512, 3), (2, 3, 64, 260, 253, 3), (1, 3, 32, 512, 256, 1)]
THIN_OUT_SHAPES = [(1, 8, 32), (1, 70, 33), (2, 130, 70), (2, 3, 40), (2, 37, 3), (3, 20, 24), (1, 3, 3), (2, 16, 64), (1, 9, 34), (1, 26, 98), (2, 41, 200)]


def gpu_rows():
    rows = []
    for n, c, k, h, w, ksz, stride, pad in P3_CASES:
        for p in (0, 1):
            for bits in (AL | P3W | P3X, AL | P3W):
                rows.append(row(p, bits, n, h, w, c, k, ksz, stride, pad))
        rows.append(row(2, AL | P3X | P3Y, n, h, w, c, k, ksz, stride, pad))
    for n, c, k, h, w, ks in THIN_IN_ROUTES:
        rows.append(row(0, AL, n, h, w, c, k, ks, 1, ks // 2))
        rows.append(row(1, AL | THIN_IN, n, h, w, c, k, ks, 1, ks // 2))
    for n, h, w in THIN_OUT_SHAPES:
        for p in (0, 1, 2):
            rows.append(row(p, AL, n, h, w, 32, 3, 3, 1, 1))
    return rows


def desc_of(r):
    from face_mask_inpaint_amd import _lib

    n, h, w, c, k, kh, kw, stride, pad, dil, pad_mode, xcs, ycs = r[3:16]
    dl = max(dil, 1)
    return _lib.ConvDesc(n, h, w, c, (h + 2 * pad - dl * (kh - 1) - 1) // stride + 1, (w + 2 * pad - dl * (kw - 1) - 1) // stride + 1, k, xcs, ycs, kh, kw,
                         stride, pad, pad_mode, dil)


def evaluate(lib, rows):
    """the query's answer for every input row"""
    from face_mask_inpaint_amd import _lib

    fn = lib.fmi_conv2d_f32_plan
    fn.argtypes, fn.restype = _lib.PREDICATES["fmi_conv2d_f32_plan"], C.c_int
    out = (C.c_int * len(OUT_COLS))()
    res = []
    thin = [getattr(lib, name, None) for name in ("fmi_conv2d_thin_supported", "fmi_conv2d_thin_in_routed")]
    for r in rows:
        d = desc_of(r)
        if all(thin):  # a device build: the predicates' answers go into the row; a g++ build keeps what the row says
            r = list(r)
            r[1] = (r[1] & ~THIN_OUT) | (THIN_OUT if r[0] != 3 and thin[0](C.byref(d)) else 0)
            if r[0] != 1:  # the adjoint's THIN_IN is an input in every build
                r[1] = (r[1] & ~THIN_IN) | (THIN_IN if r[0] == 0 and thin[1](C.byref(d)) else 0)
        rc = fn(C.byref(d), r[0] | (r[2] << 8), r[1], C.cast(out, C.c_void_p))
        assert rc == out[0], (r, rc, list(out))
        res.append(list(r) + list(out))
    return res


def write(rows, path=OUT):
    import numpy as np

    np.savez_compressed(path, rows=np.array(rows, dtype=np.int32), in_cols=np.array(IN_COLS), out_cols=np.array(OUT_COLS))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from face_mask_inpaint_amd import _lib

    table = evaluate(C.CDLL(sys.argv[1] if len(sys.argv) > 1 else _lib.LIB_PATH), sweep())
    write(table)
    print(f"{OUT}: {len(table)} rows")
