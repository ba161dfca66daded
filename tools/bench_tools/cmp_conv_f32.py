"""cmp_conv_f32.py <cand.so> <ref.so>: the entries of the fp32 convolution family (csrc/conv.hip: forward, adjoint, weight gradient) under
two builds of the library on identical inputs; every output must be torch.equal on the raw bits.  The cases are those of
tests/test_gpu_conv_f32_plan.py (one per route and tile family, at the shapes its host search finds with the CANDIDATE's query) and the
training step's own layers (STEP_LAYERS).  A split reduction and the weight gradients accumulate with atomics outside the reproducible
mode: those cases run in that mode only, every other case in both.  Exit status 1 on any difference.  Either build may lack entries the
other has (an older library next to a newer one): only the entries the cases call are needed, and the plan query only of the candidate."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from face_mask_inpaint_amd import functional as FF, _lib  # noqa: E402
import test_gpu_conv_f32_plan as T  # noqa: E402

dev = torch.device("cuda:0")
libs = [_lib.Library(sys.argv[1], strict=False), _lib.Library(sys.argv[2], strict=False)]
#              n    h   ci   co  k  stride   (the layers of the benchmark step that tools/bench_tools/p3_time.py times, and two strided ones)
STEP_LAYERS = [(8, 128, 256, 256, 3, 1), (24, 56, 256, 256, 3, 1), (24, 28, 512, 512, 3, 1), (24, 224, 64, 64, 3, 1), (24, 112, 128, 128, 3, 1),
               (8, 32, 128, 128, 3, 1), (8, 64, 128, 128, 3, 1), (8, 256, 32, 32, 3, 1), (8, 128, 256, 64, 1, 1), (8, 64, 128, 256, 3, 2), (16, 8, 512, 512, 3, 2)]
cand = libs[0]  # the plan query is asked of the candidate only, whatever library the last case left current
bad = ran = 0


def run(lib, pass_, n, h, w, c, k, ksz, stride, w3, x3, y3, bias, seed):
    """one entry on fixed inputs -> its output tensors"""
    g = torch.Generator().manual_seed(seed)
    pad = ksz // 2
    wt_ = torch.randn(k, c, ksz, ksz, generator=g) / (c * ksz * ksz) ** 0.5
    (pw,) = FF.prepare_weights([(wt_.to(dev), None, None)])
    xd = torch.randn(n, h, w, c, generator=g).to(dev)
    b = torch.randn(k, generator=g).to(dev) if bias else None
    d, oh, ow = FF.conv_desc(n, h, w, c, k, ksz, ksz, stride, pad)
    gyd = torch.randn(n, oh, ow, k, generator=g).to(dev)
    keep = []
    if w3 and pw.w3 is not None and pw.w3[0 if pass_ == 0 else 1] is not None:
        d.w3 = pw.w3[0 if pass_ == 0 else 1].data_ptr()
    if x3:
        keep.append(T._split(FF, xd if pass_ != 1 else gyd))
        d.x3 = keep[-1].data_ptr()
    if y3:
        keep.append(T._split(FF, gyd))
        d.y3 = keep[-1].data_ptr()
    if pass_ == 0:
        y = torch.full((n, oh, ow, k), float("nan"), device=dev)
        lib.conv2d_fwd_f32(C.byref(d), FF._p(xd), FF._p(pw.wf.detach()), FF._p(b), None, FF._p(y), 0, 1, 0, FF._st())
        out = [y]
    elif pass_ == 1:
        dx = torch.full((n, h, w, c), float("nan"), device=dev)
        lib.conv2d_dgrad_f32(C.byref(d), FF._p(gyd), FF._p(pw.wt), None, None, FF._p(dx), 1, 0, FF._st())
        out = [dx]
    else:
        dw, db = torch.zeros(ksz * ksz, c, k, device=dev), (torch.zeros(k, device=dev) if bias else None)
        lib.conv2d_wgrad_f32(C.byref(d), FF._p(xd), FF._p(gyd), FF._p(dw), FF._p(db), 1, 0, FF._st())
        out = [dw] + ([db] if bias else [])
    torch.cuda.synchronize()
    return out


def case(name, det, *args):
    global bad, ran
    res = []
    for lib in libs:
        _lib._LIB = lib
        with FF.deterministic(det), torch.no_grad():
            res.append(run(lib, *args))
    ok = all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))
    ran += 1
    bad += not ok
    print(f"{'ok  ' if ok else 'DIFF'} {name}{' det' if det else ''}: {len(res[0])} tensors, {sum(o.numel() for o in res[0])} elements")


for pass_, cases in ((0, T.FWD), (1, T.ADJ), (2, T.WGRAD)):
    for name, cs in cases:
        cs = dict(cs)
        want, hw, det_case = cs.pop("want"), cs.pop("hw", None), cs.pop("det", False)
        w3, x3, y3 = cs.get("w3", False), cs.get("x3", False), cs.get("y3", False)
        bias = cs.get("bias", pass_ == 0)
        flags = T.BASE | (T.G.P3W if w3 else 0) | (T.G.P3X if x3 else 0) | (T.G.P3Y if y3 else 0) | (T.G.BIAS if bias else 0)
        _lib._LIB = cand
        with FF.deterministic(det_case):
            n, h, w = T.smallest(FF, pass_, flags, cs["c"], cs["k"], cs["ksz"], cs.get("stride", 1), want, hw, cand)
            d, _, _ = FF.conv_desc(n, h, w, cs["c"], cs["k"], cs["ksz"], cs["ksz"], cs.get("stride", 1), cs["ksz"] // 2)
            _, o, ls = T.query(d, pass_, flags, cand)
        atomics = pass_ == 2 or o[3] & 1 or any(l["init"] for l in ls) or bool(o[2])  # the thin kernels' weight gradients and splits are not this file's
        for det in ((True,) if atomics else (False, True)):
            case(f"{('fwd', 'dgrad', 'wgrad')[pass_]} {name} {n}x{h}x{w} {cs['c']}->{cs['k']} k{cs['ksz']}", det, pass_, n, h, w, cs["c"], cs["k"], cs["ksz"],
                 cs.get("stride", 1), w3, x3, y3, bias, 7)
for i, (n, h, ci, co, ks, stride) in enumerate(STEP_LAYERS):
    for pieces in (False, True):
        for pass_ in (0, 1, 2):
            for det in ((True,) if pass_ == 2 else (False, True)):
                if not det and pass_ != 2:  # a split reduction outside the reproducible mode meets through atomics: skip where the plan splits
                    d, _, _ = FF.conv_desc(n, h, h, ci, co, ks, ks, stride, ks // 2)
                    _, o, ls = T.query(d, pass_, T.BASE | T.G.P3W | (T.G.P3X if pieces else 0) | (T.G.BIAS if pass_ == 0 else 0), cand)
                    if o[3] & 1 or any(l["init"] for l in ls):
                        continue
                case(f"{('fwd', 'dgrad', 'wgrad')[pass_]} layer {n}x{h}^2 {ci}->{co} k{ks} s{stride}{' pieces' if pieces else ''}", det, pass_, n, h, h, ci, co, ks,
                     stride, True, pieces, pieces and pass_ == 2, pass_ == 0, 100 + i)
print(f"{'OK' if not bad else 'FAILED'}: {ran} cases, {bad} differ")
sys.exit(1 if bad else 0)
