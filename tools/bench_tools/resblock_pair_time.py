"""Stand-alone timer of the ResBlock pair  conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2  for two builds of the library in one process:
    python tools/bench_tools/resblock_pair_time.py PARENT.so NEW.so
Per ResBlock shape of the PICNet step (256^2, batch 8), alternating the two in ROUNDS rounds:
  fwd   : PARENT's fmi_conv2d_fwd_f32 twice (the 1x1 bypass, then conv2 with its result as residual)  against  NEW's fmi_conv2d_pair_fwd_f32;
  wgrad : PARENT's weight gradients as functional._Conv2d issues them (two fmi_conv2d_wgrad_f32 with the bias gradient riding along; for a
          shape on the piece-image path fmi_conv2d_wgrad_f32 from pieces twice + fmi_bias_grad_f32)  against  NEW's
          fmi_conv2d_pair_wgrad_f32.
A measurement is one event pair around CALLS back-to-back invocations (so the gap between the two launches counts, as it does in the step);
a round's figure is the median of REPS measurements, in microseconds per invocation.  Piece images of activations are cut before the
clock starts (they come from passes both routes need), and the accumulated destinations are not re-zeroed between invocations.
A shape is routed to the fused entry (fmi_conv2d_pair_routed in csrc/conv.hip) only if the fused figure is lower in EVERY round."""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF, _lib
dev = torch.device("cuda:0")
ROUNDS, REPS, CALLS = 5, 7, 20
SHAPES = ((8, 32, 128, 128), (8, 32, 128, 256), (8, 16, 128, 128), (8, 8, 128, 128), (8, 128, 32, 64), (8, 64, 64, 128))  # N, H = W, C1 = C2, K
def figure(fn):
    for _ in range(3): fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        for _ in range(CALLS): fn()
        e.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) * 1e3 / CALLS for s, e in ev)
parent, new = (_lib.Library(p, strict=False) for p in sys.argv[1:3])
print("parent %s\nnew    %s\nrounds %d, median of %d measurements of %d invocations each, microseconds per invocation" % (sys.argv[1], sys.argv[2], ROUNDS, REPS, CALLS))
for n, h, c, k in SHAPES:
    x1, x2, gy = (torch.randn(n, h, h, ch, device=dev) for ch in (c, c, k))
    b1, b2 = torch.randn(k, device=dev), torch.randn(k, device=dev)
    pw1, pw2 = FF.prepare_weights([(torch.randn(k, c, 3, 3, device=dev) * 0.05, None, None), (torch.randn(k, c, 1, 1, device=dev) * 0.1, None, None)])
    p3 = FF.p3_wanted(n * h * h, c, k, 9)  # conv2 runs from piece images of x1 today: such a shape keeps the two launches unless measured here
    x3 = FF.p3_of(x1) if p3 else None
    d3, _, _ = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1, w3=pw1.w3[0], x3=x3)
    d1, _, _ = FF.conv_desc(n, h, h, c, k, 1, 1, 1, 0, w3=pw2.w3[0])
    dp, _, _ = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1, w3=pw1.w3[0])
    st, P = FF._st(), FF._p
    s, y = torch.empty(n, h, h, k, device=dev), torch.empty(n, h, h, k, device=dev)
    w3b = C.c_void_p(pw2.w3[0].data_ptr())
    def fwd_two():
        parent.conv2d_fwd_f32(C.byref(d1), P(x2), P(pw2.wf), P(b2), None, P(s), 0, 1, 0, st)
        parent.conv2d_fwd_f32(C.byref(d3), P(x1), P(pw1.wf), P(b1), P(s), P(y), 0, 1, 0, st)
    def fwd_pair():
        new.conv2d_pair_fwd_f32(C.byref(dp), P(x1), P(x2), c, P(pw1.wf), P(pw2.wf), w3b, P(b1), P(b2), P(y), 0, st)
    g1, g2, gb, gb2 = torch.zeros(9, c, k, device=dev), torch.zeros(1, c, k, device=dev), torch.zeros(k, device=dev), torch.zeros(k, device=dev)
    w3d, _, _ = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1)
    w1d, _, _ = FF.conv_desc(n, h, h, c, k, 1, 1, 1, 0)
    pieces_wgrad = p3 and c % 32 == 0 and k % 16 == 0
    if pieces_wgrad:  # functional._Conv2d.backward: both operands as pieces, the bias gradient in its own pass (3x3 only; the 1x1 is below the piece threshold)
        gy3 = FF.p3_of(gy)
        w3d.x3, w3d.y3 = x3.data_ptr(), gy3.data_ptr()
    def wgrad_two():
        if pieces_wgrad:
            parent.conv2d_wgrad_f32(C.byref(w3d), P(x1), P(gy), P(g1), None, 1, 0, st)
            parent.bias_grad_f32(P(gy), gy.numel() // k, k, k, P(gb), st)
        else:
            parent.conv2d_wgrad_f32(C.byref(w3d), P(x1), P(gy), P(g1), P(gb), 1, 0, st)
        parent.conv2d_wgrad_f32(C.byref(w1d), P(x2), P(gy), P(g2), P(gb2), 1, 0, st)
    wpd, _, _ = FF.conv_desc(n, h, h, c, k, 3, 3, 1, 1)
    def wgrad_pair():
        new.conv2d_pair_wgrad_f32(C.byref(wpd), P(x1), P(x2), c, P(gy), P(g1), P(g2), P(gb), st)
    tag = "%dx%dx%d %d->%d +1x1 %d%s" % (n, h, h, c, k, c, " (conv2 from pieces today)" if p3 else "")
    if not new.conv2d_pair_supported(C.byref(dp), c):
        print("%-46s not supported by the fused entries" % tag, flush=True)
        continue
    for part, two, pair, flops in (("fwd", fwd_two, fwd_pair, 2.0 * n * h * h * k * 10 * c), ("wgrad", wgrad_two, wgrad_pair, 2.0 * n * h * h * k * 10 * c)):
        rows = []
        for _ in range(ROUNDS):
            rows.append((figure(two), figure(pair)))
        wins = all(b < a for a, b in rows)
        ma, mb = statistics.median(a for a, _ in rows), statistics.median(b for _, b in rows)
        print("%-5s %-46s two launches %s | fused %s | medians %7.1f -> %7.1f us (%5.1f TFLOP/s) | fused lower in %d / %d rounds -> %s" % (
            part, tag, " ".join("%7.1f" % a for a, _ in rows), " ".join("%7.1f" % b for _, b in rows), ma, mb, flops / (mb * 1e-6) / 1e12,
            sum(b < a for a, b in rows), ROUNDS, "ROUTE" if wins else "keep two launches"), flush=True)
    del x1, x2, gy, s, y
