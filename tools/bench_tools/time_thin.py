"""Stand-alone timer of the Output block's thin-output kernels (32 -> 3, reflect padding, 8 x 1024 x 1024) for one or more builds of
the library in one call:  python tools/bench_tools/time_thin.py LIB_A.so [LIB_B.so ...]
Per library: forward, the separate backward entries (tanh backward + adjoint + weight gradient) and, where the library has it, the
one-pass backward (fmi_conv2d_thin_lrelu_bwd_f32, fused launch + finishing launch).  TB/s = algorithmic bytes / time."""
import ctypes as C, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib
dev = torch.device("cuda:0"); st = torch.cuda.current_stream().cuda_stream
n, h, c, k, slope = 8, 1024, 32, 3, 0.1
x = torch.randn(n, h, h, c, device=dev); wf = torch.randn(9, c, k, device=dev) * 0.05; wt = wf.permute(0, 2, 1).contiguous()
d, oh, ow = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1, 1)
y = torch.empty(n, h, h, k, device=dev); gy = torch.randn(n, h, h, k, device=dev); gt = torch.empty_like(gy); gx = torch.empty_like(x)
gw = torch.zeros_like(wf); gb = torch.zeros(k, device=dev)
def timeit(fn, nrep=10):
    for _ in range(3): fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); s.record()
    for _ in range(nrep): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / nrep
xb, yb = x.numel() * 4 / 1e9, y.numel() * 4 / 1e9
for rnd in range(2):  # every library twice, alternating
    for path in sys.argv[1:]:
        lib = _lib.Library(path, strict=False)
        tf = timeit(lambda: lib.conv2d_thin_lrelu_fwd_f32(C.byref(d), FF._p(x), slope, FF._p(wf), FF._p(gb), FF._p(y), 1, st))
        tf0 = timeit(lambda: lib.conv2d_thin_lrelu_fwd_f32(C.byref(d), FF._p(x), slope, FF._p(wf), FF._p(gb), FF._p(y), 0, st))
        tt = timeit(lambda: lib.eltwise_f32(FF.EW_TANH_BWD, FF._p(gy), FF._p(y), FF._p(gt), gy.numel(), 0.0, st)) if hasattr(lib, "eltwise_f32") else float("nan")
        td = timeit(lambda: lib.conv2d_thin_lrelu_dgrad_f32(C.byref(d), FF._p(gt), FF._p(wt), FF._p(x), slope, FF._p(gx), st))
        tw = timeit(lambda: lib.conv2d_thin_lrelu_wgrad_f32(C.byref(d), FF._p(x), slope, FF._p(gt), FF._p(gw), FF._p(gb), st))
        print("%-28s fwd %.3f ms (%.2f TB/s; %.3f without tanh)  tanh_bwd %.3f  dgrad %.3f ms (%.2f TB/s)  wgrad %.3f ms (%.2f TB/s)  separate backward %.3f ms" % (
            os.path.basename(path), tf, (xb + yb) / tf, tf0, tt, td, (2 * xb + yb) / td, tw, (xb + yb) / tw, tt + td + tw), flush=True)
        if hasattr(lib, "conv2d_thin_lrelu_bwd_f32"):
            nb = lib.conv2d_thin_lrelu_bwd_ws_bytes(C.byref(d)); ws = torch.empty(nb // 4, device=dev)
            tb = timeit(lambda: lib.conv2d_thin_lrelu_bwd_f32(C.byref(d), FF._p(x), slope, FF._p(gy), FF._p(y), FF._p(wt), FF._p(gx), FF._p(gw), FF._p(gb), FF._p(ws), nb, st))
            print("%-28s one-pass backward %.3f ms (%.2f TB/s of %.2f GB)" % ("", tb, (2 * xb + 2 * yb) / tb, 2 * xb + 2 * yb), flush=True)
