"""Stand-alone timer of the thin-input convolutions (C = 3: the image-facing first layers of the encoders, the discriminator and VGG16)
for two builds of the library in one call:  python tools/bench_tools/thin_in_time.py PARENT.so NEW.so
Per shape of the PICNet step and per library, alternating, every repetition timed by its own event pair (3 warm-ups, 10 repetitions):
  fwd   : fmi_conv2d_fwd_f32 (routes to thinin.hip where the library has it),
  wgrad : fmi_conv2d_wgrad_f32 + fmi_bias_grad_f32 into zeroed buffers (the fills themselves are NOT timed), and, where the library has it,
          fmi_conv2d_thin_in_wgrad_f32 (dW and dbias, nothing to zero),
  dgrad : fmi_conv2d_dgrad_f32.
Prints median / min / max in microseconds and the algorithmic bytes (the large tensor once + the image) over the median as a share of the
6.29 TB/s copy rate.  A shape goes to the new kernel only if its median is below the parent's by more than the parent's max - min."""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib
dev = torch.device("cuda:0")
COPY = 6.29e12
def times(fn, nrep=10):
    for _ in range(3): fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(nrep)]
    torch.cuda.synchronize()
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1e3 for s, e in ev]
def report(tag, path, ts, nbytes):
    med = statistics.median(ts)
    print("%-34s %-28s median %8.1f us  min %8.1f  max %8.1f  spread %6.1f   %5.1f %% of the copy rate" % (
        tag, path[-28:], med, min(ts), max(ts), max(ts) - min(ts), 100.0 * nbytes / (med * 1e-6) / COPY), flush=True)
libs = [(p, _lib.Library(p, strict=False)) for p in sys.argv[1:]]
SHAPES = (("fwd", 24, 224, 64, 3), ("fwd", 8, 256, 32, 3), ("fwd", 8, 128, 32, 1), ("wgrad", 8, 256, 32, 3), ("wgrad", 8, 128, 32, 1),
          ("dgrad", 24, 224, 64, 3), ("dgrad", 8, 256, 32, 3), ("dgrad", 8, 128, 32, 1))
for part, n, h, k, ks in SHAPES:
    c, taps = 3, ks * ks
    x = torch.randn(n, h, h, c, device=dev); big = torch.randn(n, h, h, k, device=dev); bias = torch.randn(k, device=dev)
    w = torch.randn(k, c, ks, ks, device=dev) * 0.1
    wf = w.permute(2, 3, 1, 0).reshape(taps, c, k).contiguous(); wt = w.permute(2, 3, 0, 1).reshape(taps, k, c).contiguous()
    d, _, _ = FF.conv_desc(n, h, h, c, k, ks, ks, 1, ks // 2, 0)
    nbytes = 4 * (big.numel() + x.numel())
    tag = "%s %dx%dx%d %d->%d k%d" % (part, n, h, h, c, k, ks)
    st = FF._st()
    for rnd in range(2):  # every library twice, alternating
        for path, lib in libs:
            if part == "fwd":
                report(tag, path, times(lambda: lib.conv2d_fwd_f32(C.byref(d), FF._p(x), FF._p(wf), FF._p(bias), None, FF._p(big), 0, 1, 0, st)), nbytes)
            elif part == "dgrad":
                dx = torch.empty_like(x)
                report(tag, path, times(lambda: lib.conv2d_dgrad_f32(C.byref(d), FF._p(big), FF._p(wt), None, None, FF._p(dx), 1, 0, st)), nbytes)
            else:
                gw, gb = torch.zeros(taps, c, k, device=dev), torch.zeros(k, device=dev)
                def generic():
                    lib.conv2d_wgrad_f32(C.byref(d), FF._p(x), FF._p(big), FF._p(gw), None, 1, 0, st)
                    lib.bias_grad_f32(FF._p(big), big.numel() // k, k, k, FF._p(gb), st)
                report(tag + " generic+bias", path, times(generic), nbytes)
                if hasattr(lib, "conv2d_thin_in_wgrad_f32") and lib.conv2d_thin_in_supported(C.byref(d)):
                    nb = lib.conv2d_thin_in_wgrad_ws_bytes(C.byref(d)); ws = torch.empty(nb // 4, device=dev)
                    report(tag + " thin-in", path, times(lambda: lib.conv2d_thin_in_wgrad_f32(C.byref(d), FF._p(x), FF._p(big), FF._p(gw), FF._p(gb), FF._p(ws), nb, st)), nbytes)
    del x, big
