"""CPU: the launch plan of the bf16 convolution family (csrc/conv_bf16_plan.h) through fmi_conv2d_bf16_plan on the g++ -DFMI_HOST_EMU build
of csrc/conv_bf16.hip -- the code the GPU entries decide with, without a GPU.

* tests/golden/conv_bf16_plan.npz pins the decisions of the dispatch as it was before the plan existed (how the table was made:
  profiles/conv_bf16_dispatch.txt): every row must be reproduced exactly;
* the tiles the GPU tests prove on hardware (ADJ_CASES of tests/test_gpu_vgg_bf16.py) are in the table with those values;
* the table reaches every kernel instantiation the library has.  One exception, stated rather than hidden: conv_bf16_kernel<TB256x256, BK 32>
  with the plain store is instantiated (it always was) but the selection takes the 256 x 256 tile at BK 64 only, so no table of its decisions
  can hold it; the test asserts that it stays absent, i.e. 30 of the 31 instantiations are reached;
* properties that hold whatever the table says, over the same inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from face_mask_inpaint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face_mask_inpaint_amd", "csrc")
OK, BAD_ARG, UNSUPPORTED = 0, 1, 2
SPLIT_WS, COLSCALE, COLSCALE_AL16, OUT_AL8, DET, MODES = 1, 2, 4, 8, 16, 32
PLAIN, ACT, CHAN, GROUP, MASK = range(5)
NOUT = 14
TILES_B = [(128, 32), (128, 64), (64, 64), (64, 128), (128, 128), (256, 256)]  # TileB of conv_bf16_kernel
TILES_8P = [(512, 128), (256, 256)]                                            # Tile8P of the eight-phase kernel


@pytest.fixture(scope="module")
def plan():
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libfmi_emu_conv_bf16.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-DFMI_HOST_EMU", "-x", "c++", os.path.join(CSRC, "conv_bf16.hip"), "-o", so])
    fn = C.CDLL(so).fmi_conv2d_bf16_plan
    fn.argtypes, fn.restype = _lib.PREDICATES["fmi_conv2d_bf16_plan"], C.c_int
    return fn


@pytest.fixture(scope="module")
def table():
    t = np.load(os.path.join(ROOT, "tests", "golden", "conv_bf16_plan.npz"))
    cols, rows = [str(c) for c in t["in_cols"]] + [str(c) for c in t["out_cols"]], t["rows"].tolist()
    assert len(t["in_cols"]) == 15 and len(t["out_cols"]) == NOUT and len(rows) > 2000
    return [dict(zip(cols, r), raw=r) for r in rows]


def desc_of(r):
    oh = (r["H"] + 2 * r["pad"] - r["kh"]) // r["stride"] + 1
    ow = (r["W"] + 2 * r["pad"] - r["kw"]) // r["stride"] + 1
    return _lib.ConvDesc(r["N"], r["H"], r["W"], r["C"], oh, ow, r["K"], r["x_cstride"], r["y_cstride"], r["kh"], r["kw"], r["stride"], r["pad"], 0, 1)


def query(plan, d, pass_, stage, groups, flags):
    out = (C.c_int * NOUT)(*([-7] * NOUT))
    rc = plan(C.byref(d) if d is not None else None, pass_, stage, groups, flags, C.cast(out, C.c_void_p))
    return rc, list(out)


@pytest.fixture(scope="module")
def answers(plan, table):
    """the query's answer for every row of the table, computed once"""
    res = []
    for r in table:
        rc, out = query(plan, desc_of(r), r["pass"], r["stage"], r["groups"], r["flags"])
        assert rc == out[0]
        res.append(out)
    return res


def test_every_row_of_the_table_is_reproduced(table, answers):
    wrong = [(r["raw"][:15], r["raw"][15:], got) for r, got in zip(table, answers) if got != r["raw"][15:]]
    assert not wrong, f"{len(wrong)} of {len(table)} rows differ; first (inputs, table, query): {wrong[:3]}"


def kernel_of(r):
    """the kernel instantiation a row's decision names: (kernel, BM, BN, BK, output stage)"""
    bm, bn, eight = r["tile"] % 1000000 // 1000, r["tile"] % 1000, r["tile"] >= 1000000
    if r["pass"] == 2:
        return ("wgrad_8ph" if eight else "wgrad", bm, bn, 64, "-")
    bk = 64 if (r["C"] if r["pass"] == 0 else r["K"]) % 64 == 0 else 32
    stage = {PLAIN: "act" if eight else "none", ACT: "act", CHAN: "chan", GROUP: "group", MASK: "mask"}[r["stage"]]
    return ("conv_8ph" if eight else "conv", bm, bn, bk, stage)


def instantiations():
    """what conv_kernel_exists_b of csrc/conv_bf16.hip admits, and the weight gradient's four kernels"""
    ks = {("conv", bm, bn, bk, "none") for bm, bn in TILES_B for bk in (32, 64)}
    ks |= {("conv", bm, bn, 64, "mask") for bm, bn in TILES_B if bn >= 64}
    ks |= {("conv", bm, bn, 64, "chan") for bm, bn in TILES_B if bm == 128 and bn >= 64}
    ks |= {("conv", bm, bn, 64, "group") for bm, bn in TILES_B if bm <= bn}
    ks |= {("conv_8ph", bm, bn, 64, st) for bm, bn in TILES_8P for st in ("act", "mask")}
    ks |= {("wgrad", 128, bn, 64, "-") for bn in (32, 64, 128)} | {("wgrad_8ph", 256, 256, 64, "-")}
    return ks


def test_table_reaches_every_kernel(table):
    want = instantiations()
    assert len(want) == 12 + 5 + 2 + 4 + 4 + 3 + 1
    got = {kernel_of(r) for r in table if r["status"] == OK}
    assert not got - want, f"the table names kernels that do not exist: {got - want}"
    # `BK == 64 && ... && N > 128 && wgs(256, 256) >= 200`: the selection has never taken the 256 x 256 tile at BK 32 (module docstring)
    assert want - got == {("conv", 256, 256, 32, "none")}, want - got


def test_tiles_the_gpu_tests_prove_are_in_the_table(table):
    import test_gpu_vgg_bf16 as VG

    rows = {tuple(r["raw"][:15]): r for r in table}
    for (n, h, w, c, k), mode, tile in VG.ADJ_CASES:
        for stage in (PLAIN, MASK):  # test_masked_adjoint asserts the tile of the masked and of the plain launch
            key = (1, stage, 1, OUT_AL8 | MODES | (mode << 8), n, h, w, c, k, 3, 3, 1, 1, c, k)
            assert key in rows, key
            assert (rows[key]["status"], rows[key]["tile"]) == (OK, tile), (key, rows[key]["tile"], tile)


def test_properties_of_every_plan(table, answers):
    for r, o in zip(table, answers):
        status, tile, ksplit, grid, tiles, tiles_n, phases, kchunk = o[0], o[1], o[2], o[3:6], o[6:10], o[10], o[11], o[12]
        if status != OK:
            assert status == UNSUPPORTED and not any(o[1:]), (r["raw"], o)
            continue
        bm, bn, eight = tile % 1000000 // 1000, tile % 1000, tile >= 1000000
        assert all(0 < g < 2 ** 31 for g in grid) and ksplit >= 1, (r["raw"], o)
        d = desc_of(r)
        flags = r["flags"]
        if r["pass"] == 2:
            p = d.N * d.OH * d.OW
            assert kchunk % 64 == 0 and ksplit * kchunk >= p, (r["raw"], o)
            assert tiles[0] == -(-(d.kh * d.kw * d.C) // bm) * -(-d.K // bn) and tiles_n == -(-d.K // bn)
            if flags & DET:
                assert ksplit == 1 and not eight
            continue
        ncols, red = (d.K, d.C) if r["pass"] == 0 else (d.C, d.K)
        # rows and reduction of every phase, from the geometry (forward: one phase; adjoint: the sub-pixel phases of the stride)
        if r["pass"] == 0:
            ms, ks, taps = [d.N * d.OH * d.OW], [d.kh * d.kw * d.C], [d.kh * d.kw]
        else:
            ms, ks, taps = [], [], []
            s = d.stride
            for py in range(s):
                for px in range(s):
                    gh, gw = (d.H - py + s - 1) // s, (d.W - px + s - 1) // s
                    if gh <= 0 or gw <= 0:
                        continue
                    t = len(range((py + d.pad) % s, d.kh, s)) * len(range((px + d.pad) % s, d.kw, s))
                    ms.append(d.N * gh * gw), ks.append(t * d.K), taps.append(t)
        assert phases == len(ms) and tiles_n == -(-ncols // bn)
        assert tiles[:phases] == [-(-m // bm) * tiles_n for m in ms] and not any(tiles[phases:]), (r["raw"], o)
        assert grid == [max(tiles), r["groups"] if r["stage"] == GROUP else phases, ksplit]
        if (flags & DET) or (flags & COLSCALE) or r["stage"] != PLAIN or not (flags & SPLIT_WS):
            assert ksplit == 1, (r["raw"], o)
        if eight:
            assert red % 64 == 0 and ncols % 4 == 0 and max(taps) <= 32 and all(k % 64 == 0 for k in ks) and ksplit == 1, (r["raw"], o)


def test_query_refuses_what_the_entries_refuse(plan):
    d = _lib.ConvDesc(1, 8, 8, 64, 8, 8, 64, 64, 64, 3, 3, 1, 1, 0, 1)
    rc, out = query(plan, d, 0, PLAIN, 1, OUT_AL8 | MODES)
    assert rc == OK and out[1] == 64064
    assert query(plan, None, 0, PLAIN, 1, 0)[0] == BAD_ARG                     # null descriptor
    assert plan(C.byref(d), 0, PLAIN, 1, 0, None) == BAD_ARG                   # null out
    assert query(plan, d, 3, PLAIN, 1, 0)[0] == BAD_ARG and query(plan, d, 0, 5, 1, 0)[0] == BAD_ARG
    for bad, code in ((dict(OH=7), BAD_ARG), (dict(C=0), BAD_ARG), (dict(x_cstride=32), BAD_ARG), (dict(dil=2), UNSUPPORTED),
                      (dict(pad_mode=1), UNSUPPORTED)):  # check_desc_b, the first thing every entry does
        e = _lib.ConvDesc(1, 8, 8, 64, 8, 8, 64, 64, 64, 3, 3, 1, 1, 0, 1)
        for k, v in bad.items():
            setattr(e, k, v)
        for pass_ in (0, 1, 2):
            rc, out = query(plan, e, pass_, PLAIN, 1, 0)
            assert rc == code and out[0] == code and not any(out[1:]), (bad, pass_, rc, out)
    s3 = _lib.ConvDesc(1, 9, 9, 64, 3, 3, 64, 64, 64, 3, 3, 3, 0, 0, 1)
    assert query(plan, s3, 1, PLAIN, 1, 0)[0] == UNSUPPORTED and query(plan, s3, 0, PLAIN, 1, 0)[0] == OK  # adjoint: stride <= 2


def test_query_defaults_to_the_library_modes(plan):
    """without FMI_PLAN_MODES the tile mode is the one fmi_debug_bf16_tile set"""
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_build", "libfmi_emu_conv_bf16.so"))
    d = _lib.ConvDesc(2, 16, 16, 512, 16, 16, 256, 512, 256, 3, 3, 1, 1, 0, 1)
    assert query(plan, d, 1, PLAIN, 1, OUT_AL8)[1][1] == 64064
    prev = lib.fmi_debug_bf16_tile(8)
    try:
        assert query(plan, d, 1, PLAIN, 1, OUT_AL8)[1][1] == 1256256
        assert query(plan, d, 1, PLAIN, 1, OUT_AL8 | MODES)[1][1] == 64064
    finally:
        lib.fmi_debug_bf16_tile(prev)
