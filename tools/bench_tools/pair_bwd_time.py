"""Stand-alone timer of the backward of the decoder's ConvTranspose2d pairs (last block 8 x 512^2 32+64 -> 32, second last 8 x 256^2
64+128 -> 64) for two builds of the library in one call:  python tools/bench_tools/pair_bwd_time.py LIB_A.so LIB_B.so
Per library, alternating: the separate launches (two adjoints + two weight gradients + the bias pass + the two fills, exactly what
_ConvTransposePair.backward runs without the one-pass entry) and, where the library has it and takes the shape, the one-pass backward
(fmi_conv_transpose2d_pair_bwd_f32, fused launch + finishing launch).  TFLOP/s = 2 x 2 * pixels * (cs1 + cs2) * cb * 9 / time."""
import ctypes as C, os, sys, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib
dev = torch.device("cuda:0")
def timeit(fn, nrep=10):
    for _ in range(3): fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); s.record()
    for _ in range(nrep): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / nrep
libs = [(_p, _lib.Library(_p, strict=False)) for _p in sys.argv[1:]]
for n, h, cs1, cs2, cb in ((8, 512, 32, 64, 32), (8, 256, 64, 128, 64)):
    _lib._LIB = libs[0][1]
    x1 = torch.randn(n, h, h, cs1, device=dev); x2 = torch.randn(n, h, h, cs2, device=dev); gy = torch.randn(n, 2 * h, 2 * h, cb, device=dev)
    pw1, pw2 = FF.prepare_weights([(torch.randn(cs1, cb, 3, 3, device=dev) * 0.05, None, None), (torch.randn(cs2, cb, 3, 3, device=dev) * 0.05, None, None)])
    d, _, _ = FF.conv_desc(n, 2 * h, 2 * h, cb, cs1, 3, 3, 2, 1)
    flop = 2 * 2.0 * (x1.numel() + x2.numel()) * cb * 9
    gbytes = (gy.numel() + 2 * x1.numel() + 2 * x2.numel()) * 4 / 1e9
    def separate():
        for x, pw in ((x1, pw1), (x2, pw2)):
            ns = types.SimpleNamespace(saved_tensors=(x, pw.wf), cfg=(3, 3, 2, 1), has=(False, False), HW=(2 * h, 2 * h), wf3=pw.w3[0], x3=None, needs_input_grad=(True, True) + (False,) * 9)
            FF._ConvTranspose2d.backward(ns, gy)
        gb = torch.zeros(cb, device=dev)
        FF._L().bias_grad_f32(FF._p(gy), gy.numel() // cb, cb, cb, FF._p(gb), FF._st())
    for rnd in range(2):  # every library twice, alternating
        for path, lib in libs:
            _lib._LIB = lib
            ts = timeit(separate)
            print("%dx%dx%d %d+%d->%d  %-40s separate launches %.3f ms (%.1f TFLOP/s)" % (n, h, h, cs1, cs2, cb, path[-40:], ts, flop / ts / 1e9), flush=True)
            if hasattr(lib, "conv_transpose2d_pair_bwd_f32") and lib.conv_transpose2d_pair_bwd_supported(C.byref(d), cs1, cs2):
                nb = lib.conv_transpose2d_pair_bwd_ws_bytes(C.byref(d), cs1, cs2); ws = torch.empty(nb // 4, device=dev)
                gx1, gx2, gw1, gw2, gb = torch.empty_like(x1), torch.empty_like(x2), torch.empty_like(pw1.wf), torch.empty_like(pw2.wf), torch.empty(cb, device=dev)
                tb = timeit(lambda: lib.conv_transpose2d_pair_bwd_f32(C.byref(d), FF._p(x1), FF._p(x2), cs2, FF._p(gy), C.c_void_p(pw1.w3[0].data_ptr()), C.c_void_p(pw2.w3[0].data_ptr()),
                                                                      FF._p(gx1), FF._p(gx2), FF._p(gw1), FF._p(gw2), FF._p(gb), FF._p(ws), nb, FF._st()))
                print("%-60s one-pass backward %.3f ms (%.1f TFLOP/s; %.2f TB/s of %.2f GB)" % ("", tb, flop / tb / 1e9, gbytes / tb, gbytes), flush=True)
                del ws, gx1, gx2
            else:
                print("%-60s one-pass backward: not in this library for this shape" % "", flush=True)
    del x1, x2, gy
