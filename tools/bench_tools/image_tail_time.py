"""The image tail of pSp inference at N = 8, S = 1024 and S = 256: median of 20 timed calls after 5 warm-ups (device events) of
(a) the composition the fused kernel replaces -- FF.to_nchw -> FF.to_nhwc -> FF.adaptive_avg_pool -> FF.to_nchw -> (x + 1) / 2 -> clamp -> * 255
    -> .to(uint8) -> permute to HWC -- and
(b) FF.image_tail with all three outputs (and with 'pooled' alone),
plus the bytes/s of (b) (input + the outputs asked for) against the 6.29 TB/s measured-copy figure.  One JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from face_mask_inpaint_amd import functional as FF  # noqa: E402

COPY_TBS = 6.29


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def parent_path(x):
    img = FF.to_nchw(x)                                               # what Generator.forward returns
    pooled = FF.to_nchw(FF.adaptive_avg_pool(FF.to_nhwc(img), 256, 256)).contiguous()
    unit = (pooled + 1) / 2
    u8 = (unit.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return pooled, unit, u8


def main():
    dev = torch.device("cuda:0")
    res = {}
    with torch.no_grad():
        for s in (1024, 256):
            x = torch.rand(8, s, s, 3, device=dev) * 3 - 1.5
            p, u, b = parent_path(x)
            o = FF.image_tail(x)
            assert float((o["pooled"] - p).abs().max()) <= 1e-5 and int((o["u8"].int() - b.int()).abs().max()) <= 1
            in_b, out_all = x.numel() * 4, 2 * 8 * 3 * 65536 * 4 + 8 * 3 * 65536
            t_a = timed(lambda: parent_path(x))
            t_b = timed(lambda: FF.image_tail(x))
            t_p = timed(lambda: FF.image_tail(x, want=("pooled",)))
            res[f"S{s}"] = dict(parent_ms=round(t_a, 4), image_tail_ms=round(t_b, 4), image_tail_pooled_only_ms=round(t_p, 4),
                                image_tail_TBs=round((in_b + out_all) / t_b / 1e9, 3), pooled_only_TBs=round((in_b + 8 * 3 * 65536 * 4) / t_p / 1e9, 3),
                                share_of_copy_rate=round((in_b + out_all) / t_b / 1e9 / COPY_TBS, 3))
    print(json.dumps(dict(image_tail_time=res, n=8, copy_TBs=COPY_TBS)))


if __name__ == "__main__":
    main()
