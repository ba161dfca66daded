"""CPU: the launch plan of the fp32 convolution family (csrc/conv_f32_plan.h) through fmi_conv2d_f32_plan on the g++ -DFMI_HOST_EMU build of
csrc/conv.hip + csrc/gemm.hip -- the code the GPU entries decide with, without a GPU.

* tests/golden/conv_f32_plan.npz pins the decisions of the dispatch as it was before the plan header existed (how the table was made:
  profiles/conv_f32_dispatch.txt): every row must be reproduced exactly;
* properties that hold whatever the table says, over the same inputs;
* the table reaches every (route, tile, kernel form) the launchers' switches name;
* the shapes whose route the GPU tests prove (tests/test_gpu_p3.py, test_gpu_thin_in.py, test_gpu_thin_paths.py) are in the table with it.

Two limits, stated rather than hidden.  instantiations() below is written by hand from the launchers' switches (gemm_core.h with_gemm_tile and
launch_gemm_plan, conv3x3.h, conv_p3.h, convt3x3.h), not extracted from them: a tile added to a switch must be added here.  It counts
(route, tile, kernel form) and so leaves out what multiplies a kernel without another decision: the pair's X2 instantiations of
conv3x3_dma_kernel and its GEMM loader types (ConvK2 / ConvWX2 / ConvWX32 / WgradAX2) take the same plan functions as the single convolution, and
the table's pair rows pin them.  The generator keeps literal copies of the GPU tests' shape lists (P3_CASES, THIN_IN_ROUTES, THIN_OUT_SHAPES) so
that sweep() needs no test module; this file imports the ORIGINALS and find() fails if one of their shapes is not in the table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from face_mask_inpaint_amd import _lib
from tools.golden import gen_conv_f32_plan as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face_mask_inpaint_amd", "csrc")
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
NIN, NOUT = len(G.IN_COLS), len(G.OUT_COLS)
GEMM_TILES = [128032, 128064, 64064, 128128, 64128, 32128]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libfmi_emu_conv_f32_plan.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-DFMI_HOST_EMU", "-x", "c++", os.path.join(CSRC, "conv.hip"), os.path.join(CSRC, "gemm.hip"), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def table():
    t = np.load(os.path.join(ROOT, "tests", "golden", "conv_f32_plan.npz"))
    assert [str(c) for c in t["in_cols"]] == G.IN_COLS and [str(c) for c in t["out_cols"]] == G.OUT_COLS
    rows = t["rows"].tolist()
    assert len(rows) > 5000
    return rows


@pytest.fixture(scope="module")
def answers(lib, table):
    """the query's answer for every row of the table, computed once"""
    return [r[NIN:] for r in G.evaluate(lib, [r[:NIN] for r in table])]


def launches(r):
    """the listed launches of a row (or of an answer prefixed with its inputs) as dicts"""
    out = r[NIN:]
    return [dict(zip(G.LAUNCH_COLS, out[4 + 10 * p:14 + 10 * p])) for p in range(min(out[1], 4))]


def test_every_row_of_the_table_is_reproduced(table, answers):
    wrong = [(r[:NIN], r[NIN:], got) for r, got in zip(table, answers) if got != r[NIN:]]
    assert not wrong, f"{len(wrong)} of {len(table)} rows differ; first (inputs, table, query): {wrong[:3]}"


def test_the_sweep_is_the_tables_input(table):
    """sweep() of the generator still lists the table's inputs (the thin kernels' predicate bits aside, which the table carries)"""
    strip = lambda r: (r[0], r[1] & ~(G.THIN_OUT | (0 if r[0] == 1 else G.THIN_IN)), *r[2:NIN])
    assert [strip(r) for r in table] == [strip(r) for r in G.sweep()]


def phases_of(r):
    """(rows, reduction) of every live phase, from the geometry"""
    d = G.desc_of(r)
    n = 1 if r[1] & G.BATCH_W else d.N
    if r[0] == 0:
        return [(n * d.OH * d.OW, d.kh * d.kw * d.C)]
    res, s = [], d.stride
    for py in range(s):
        for px in range(s):
            gh, gw = (d.H - py + s - 1) // s, (d.W - px + s - 1) // s
            if gh > 0 and gw > 0:
                taps = len(range((py + d.pad) % s, d.kh, s)) * len(range((px + d.pad) % s, d.kw, s))
                res.append((n * gh * gw, taps * d.K))
    return res


def test_properties_of_every_plan(table, answers):
    for r, o in zip(table, answers):
        status, nl, early, bits = o[:4]
        if status != OK:
            assert status in (BAD_ARG, UNSUPPORTED) and not any(o[1:]), (r[:NIN], o)
            continue
        if early:
            assert nl == 0 and not any(o[3:]) and early in (G.THIN_OUT_ROUTE, G.THIN_IN_ROUTE), (r[:NIN], o)
            continue
        d, flags, ls = G.desc_of(r), r[1], launches(r[:NIN] + o)
        x3 = flags & G.X3 and flags & G.X3_AL16
        w3 = flags & G.W3 and flags & G.W3_AL16
        y3 = flags & G.Y3 and flags & G.Y3_AL16
        for l in ls:
            bm, bn = divmod(l["tile"], 1000)
            assert l["grid_x"] > 0 and l["grid_y"] > 0 and l["ksplit"] >= 1, (r[:NIN], o)
            assert l["code"] == l["route"] << 24 | l["dma"] << 23 | l["fl"] << 22 | l["tile"]
            if flags & G.DET:
                assert l["ksplit"] == 1 and not l["init"], (r[:NIN], o)
            if l["route"] in (G.GEMM_P3, G.C3_P3):  # a p3 route only with both piece images present and aligned
                assert x3 and w3, (r[:NIN], o)
            if l["route"] in (G.GEMM_W3, G.C3_W3):
                assert w3, (r[:NIN], o)
            if l["route"] in (G.WGRAD_P3, G.WGRAD_P3_3X3):
                assert x3 and y3 and not flags & G.BIAS, (r[:NIN], o)
            if l["dma"]:
                assert l["route"] in (G.GEMM, G.GEMM_W3, G.WGRAD_GEMM), (r[:NIN], o)
        if r[0] in (0, 1):
            ncols = d.K if r[0] == 0 else d.C
            red_c = d.C if r[0] == 0 else d.K
            if ls[0]["route"] == G.CONVT3X3:
                assert nl == 1 and d.stride == 2 and ls[0]["grid_x"] == -(-d.N * d.OH * d.OW // 128) * -(-d.C // 32) and not bits
                continue
            ph = phases_of(r)
            assert nl == len(ph), (r[:NIN], o)
            for l, (m, red) in zip(ls, ph):
                bm, bn = divmod(l["tile"], 1000)
                assert l["grid_x"] == -(-m // bm) * -(-ncols // bn), (r[:NIN], o)  # grid x = tile count
                if l["route"] in (G.C3, G.C3_W3, G.C3_P3):
                    red = 3 * (red_c // 16)  # whole (ky, 16 channels) steps
                else:
                    assert l["chunk"] % 16 == 0
                if red:
                    assert l["ksplit"] * l["chunk"] >= red > (l["ksplit"] - 1) * l["chunk"], (r[:NIN], o)
                assert l["grid_y"] == l["ksplit"] * (d.N if flags & G.BATCH_W and l["route"] == G.GEMM else 1), (r[:NIN], o)
                # the init kernel runs exactly when the reduction is split or the phases share one
                shared = bits & 1
                assert l["init"] == (0 if shared else int(l["ksplit"] > 1)), (r[:NIN], o)
                if (flags & G.ACT and r[0] == 0) or flags & G.BATCH_W or (d.stride > 1 and r[0] == 1 and not shared):
                    assert l["ksplit"] == 1 and not l["init"], (r[:NIN], o)
        elif r[0] == 2:
            (l,) = ls
            p = d.N * d.OH * d.OW
            bm, bn = divmod(l["tile"], 1000)
            if l["route"] == G.WGRAD_GEMM:
                n = 1 if flags & G.BATCH_W else d.N
                p = n * d.OH * d.OW
                rows_ = d.kh * d.kw * d.C + (1 if bits & 2 else 0)
                assert bool(bits & 2) == bool(flags & G.BIAS) and l["grid_x"] == -(-rows_ // bm) * -(-d.K // bn), (r[:NIN], o)
                assert l["grid_y"] == l["ksplit"] * (d.N if flags & G.BATCH_W else 1)
            else:
                splits_x = -(-l["ksplit"] // 8) * 8 if bits & 4 else 1
                assert bool(bits & 4) == (l["ksplit"] >= 8) and l["grid_x"] == -(-d.kh * d.kw * d.C // bm) * -(-d.K // bn) * splits_x, (r[:NIN], o)
                assert l["grid_y"] == (1 if bits & 4 else l["ksplit"])
            assert l["chunk"] % 16 == 0 and l["ksplit"] * l["chunk"] >= p > (l["ksplit"] - 1) * l["chunk"], (r[:NIN], o)
            assert l["ksplit"] == 1 or p // l["ksplit"] >= 256, (r[:NIN], o)  # at least 512 pixels per asked split, 8-rounding aside


def instantiations():
    """(route, tile, LDS-DMA kernel, blocked accumulation) of every kernel the launchers' switches name"""
    ks = {(rt, t, dma, fl) for rt in (G.GEMM, G.GEMM_W3, G.WGRAD_GEMM) for t in GEMM_TILES for dma, fl in ((1, 0), (1, 1), (0, 0))}  # launch_gemm_plan
    ks |= {(G.GEMM_P3, t, 0, fl) for t in GEMM_TILES for fl in (0, 1)}                                                              # launch_gemm_p3
    ks |= {(G.C3, t, 0, fl) for t in GEMM_TILES[:5] for fl in (0, 1)} | {(G.C3_W3, 128064, 0, fl) for fl in (0, 1)}                # launch_conv3x3
    ks |= {(G.C3_P3, t, 0, fl) for t in (256128, 256064, 128128, 128064) for fl in (0, 1)}                                          # launch_conv3x3_p3
    ks |= {(G.WGRAD_P3, t, 0, fl) for t in (128032, 128064, 128128) for fl in (0, 1)}                                               # launch_wgrad_p3
    ks |= {(G.WGRAD_P3_3X3, t, 0, fl) for t in (192064, 192128) for fl in (0, 1)} | {(G.CONVT3X3, 128032, 0, 0)}
    return ks


def test_table_reaches_every_kernel(table):
    want = instantiations()
    assert len(want) == 54 + 12 + 12 + 8 + 6 + 5
    got = {(l["route"], l["tile"], l["dma"], l["fl"]) for r in table if r[NIN] == OK for l in launches(r)}
    assert not got - want, f"the table names kernels that do not exist: {got - want}"
    assert not want - got, f"instantiations no row reaches: {sorted(want - got)}"
    assert {r[NIN + 2] for r in table} >= {0, G.THIN_OUT_ROUTE, G.THIN_IN_ROUTE}


def find(table, pass_, bits, n, h, w, c, k, ksz, stride, pad):
    key = tuple(G.row(pass_, bits, n, h, w, c, k, ksz, stride, pad))
    strip = lambda r: (r[0], r[1] & ~(G.THIN_OUT | (0 if r[0] == 1 else G.THIN_IN)), *r[2:NIN])
    hits = [r for r in table if strip(r) == key]
    assert len(hits) == 1, key
    return hits[0]


def test_routes_the_gpu_tests_prove_are_in_the_table(table):
    import test_gpu_p3 as P3
    import test_gpu_thin_in as TI
    import test_gpu_thin_paths as TP

    for n, c, k, h, w, ksz, stride, pad in P3.CASES:  # the forward and the adjoint from piece images, and without the activation's
        for p in (0, 1):
            r = find(table, p, G.AL | G.P3W | G.P3X, n, h, w, c, k, ksz, stride, pad)
            tap3 = ksz == 3 and stride == 1
            assert r[NIN] == OK and all(l["route"] == (G.C3_P3 if tap3 else G.GEMM_P3) for l in launches(r)), r
            r = find(table, p, G.AL | G.P3W, n, h, w, c, k, ksz, stride, pad)
            assert r[NIN] == OK and all(l["route"] in (G.C3, G.C3_W3, G.GEMM_W3) for l in launches(r)), r
    # (the last case's comment there, "the 256 x 128 eight-wave tile", is not what the selection does: 128 workgroups of that tile are below
    # its 256-workgroup threshold and the table holds 128 x 128 -- profiles/conv_f32_dispatch.txt)
    r = find(table, 0, G.AL | G.P3W | G.P3X, *[P3.CASES[2][i] for i in (0, 3, 4, 1, 2, 5, 6, 7)])
    assert launches(r)[0]["ksplit"] > 1 and launches(r)[0]["init"]  # "small map: split reduction (atomic epilogue)"
    wg = [m for m in P3.test_weight_gradient_with_pieces_of_both_operands.pytestmark if m.name == "parametrize"][0].args[1]
    for n, c, k, h, w, ksz, stride, pad in wg:
        if (n, c, k, h, w, ksz, stride, pad) in P3.CASES:
            r = find(table, 2, G.AL | G.P3X | G.P3Y, n, h, w, c, k, ksz, stride, pad)
            want = G.WGRAD_P3_3X3 if ksz == 3 and stride == 1 and c % 64 == 0 and w >= 16 else G.WGRAD_P3
            assert r[NIN] == OK and launches(r)[0]["route"] == want, r
    routes = [m for m in TI.test_thin_in_routes.pytestmark if m.name == "parametrize"][0].args[1]
    for n, c, k, h, w, ks, _act in routes:
        r = find(table, 0, G.AL, n, h, w, c, k, ks, 1, ks // 2)
        assert r[NIN] == OK and r[NIN + 2] == (G.THIN_IN_ROUTE if ks == 3 else 0), r  # of the 1x1 form only the weight gradient is routed there
        r = find(table, 1, G.AL | G.THIN_IN, n, h, w, c, k, ks, 1, ks // 2)
        assert r[NIN] == OK and r[NIN + 2] == (G.THIN_IN_ROUTE if ks == 3 else 0), r
    for n, h, w in TP.SHAPES:
        for p in (0, 1, 2):
            r = find(table, p, G.AL, n, h, w, 32, 3, 3, 1, 1)
            assert r[NIN] == OK and r[NIN + 2] == G.THIN_OUT_ROUTE and r[NIN + 1] == 0, r


def test_pair_rows_agree_with_the_pair_queries(lib, table):
    """the rows of pass 3 hold what fmi_conv2d_pair_routed answers; tests/test_host_resblock_pair.py asserts the same shapes"""
    fn = lib.fmi_conv2d_pair_routed
    fn.argtypes, fn.restype = _lib.PREDICATES["fmi_conv2d_pair_routed"], C.c_int
    seen = set()
    for r in table:
        if r[0] == 3 and r[NIN] == OK:
            d = G.desc_of(r)
            assert fn(C.byref(d), r[2]) == r[NIN + 3] >> 4, r
            seen.add((d.N, d.H, d.C, d.K))
    assert seen >= set(G.PAIR_ASSERTED)


def test_query_refuses_what_the_entries_refuse(lib):
    fn = lib.fmi_conv2d_f32_plan
    fn.argtypes, fn.restype = _lib.PREDICATES["fmi_conv2d_f32_plan"], C.c_int
    out = (C.c_int * NOUT)(*([-7] * NOUT))
    d = _lib.ConvDesc(1, 8, 8, 64, 8, 8, 64, 64, 64, 3, 3, 1, 1, 0, 1)
    assert fn(C.byref(d), 0, G.AL, C.cast(out, C.c_void_p)) == OK and out[4] == G.C3 and out[1] == 1
    assert fn(None, 0, G.AL, C.cast(out, C.c_void_p)) == BAD_ARG and fn(C.byref(d), 0, G.AL, None) == BAD_ARG
    assert fn(C.byref(d), 4, G.AL, C.cast(out, C.c_void_p)) == BAD_ARG and not any(out[1:])
    for bad, code in ((dict(OH=7), BAD_ARG), (dict(C=0), BAD_ARG), (dict(x_cstride=32), BAD_ARG), (dict(pad_mode=2), UNSUPPORTED)):
        e = _lib.ConvDesc(1, 8, 8, 64, 8, 8, 64, 64, 64, 3, 3, 1, 1, 0, 1)
        for k, v in bad.items():
            setattr(e, k, v)
        for p in (0, 1, 2, 3 | 64 << 8):
            assert fn(C.byref(e), p, G.AL, C.cast(out, C.c_void_p)) == code and out[0] == code and not any(out[1:]), (bad, p, list(out))


def test_last_plan_is_exported(lib):
    assert lib.fmi_debug_f32_last_plan() == 0  # the emulation launches nothing
