"""GPU: the pSp trainer (face_mask_inpaint_amd/train_psp.py) and the one-pass pixel head of pSpLoss (csrc/psploss.hip,
FF.psp_pixel_head) against tests/golden/psp_train.pt (the reference's own pSpLoss.__call__ in fp32 and float64,
tools/golden/gen_psp_train.py) and tests/golden/psp_criteria.pt."""
import os
import time
import types

import numpy as np
import pytest
import torch

from test_host_psp_train import CASES, U, head_inputs, restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _dev(ts, dev):
    return [None if t is None else t.to(dev) for t in ts]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _laid_out(t, layout):
    """the same [N, 3, H, W] values, contiguous ("planar") or in channels-last memory ("nhwc": what pSp.forward's pool hands over)"""
    return t if layout == "planar" else t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("layout", ["planar", "nhwc"])
@pytest.mark.parametrize("name", CASES)
def test_pixel_head_forward(dev, golden, name, layout):
    """pairs bit-equal to torch's single rounded products; l2 / l2_ref within max(4 |ref32 - ref64|, 4 * 2^-24 |ref64|) of the reference's
    float64 values (the fp32 difference carries u, its square 2 u, the final fp32 rounding u); two runs bit-identical"""
    from face_mask_inpaint_amd import functional as FF

    fx = golden("psp_train.pt")
    c = fx["head"][name]
    y_hat, y, ref, mask = _dev(head_inputs(fx, name), dev)
    y_hat = _laid_out(y_hat, layout)
    assert y_hat.is_contiguous() == (layout == "planar")
    n = y_hat.shape[0]
    pair_out, pair_in, l2, l2_ref = FF.psp_pixel_head(y_hat, y, ref, mask)
    im = (1 - mask).unsqueeze(1) if mask is not None else None
    want_out = torch.cat([_nhwc(y_hat * im), _nhwc(y * im)]) if mask is not None else torch.cat([_nhwc(y_hat), _nhwc(y)])
    assert pair_out.shape == (2 * n,) + tuple(y_hat.shape[2:]) + (3,) and pair_out.is_contiguous()
    assert torch.equal(pair_out, want_out)
    if ref is None:
        assert pair_in is None and l2_ref is None
    else:
        m = mask.unsqueeze(1)
        assert torch.equal(pair_in, torch.cat([_nhwc(y_hat * m), _nhwc(ref * m)]))
    for got, k in ((l2, "loss_l2"), (l2_ref, "loss_l2_ref")):
        if got is None:
            continue
        r64, r32 = float(c[k + "64"]), float(c[k])
        bound = max(4 * abs(r32 - r64), 4 * U * abs(r64))
        print(f"{name} {k}: got {float(got):.10f} float64 {r64:.12f} error {abs(float(got) - r64):.2e} bound {bound:.2e}")
        assert got.dim() == 0 and abs(float(got) - r64) <= bound, (k, float(got), r64)
    again = FF.psp_pixel_head(y_hat, y, ref, mask)
    with FF.deterministic():
        third = FF.psp_pixel_head(y_hat, y, ref, mask)
    for other in (again, third):
        for a, b in zip((pair_out, pair_in, l2, l2_ref), other):
            assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("layout", ["planar", "nhwc"])
@pytest.mark.parametrize("name", CASES)
def test_pixel_head_backward(dev, golden, name, layout):
    """every entry of d / d y_hat within 8 * 2^-24 x the sum of the absolute values of its four terms (at most eight rounded operations per
    entry), against float64 on the same fp32 inputs: with seeded upstream gradients for both pairs and both scalars, and with the pair
    gradients absent and g2 = (1, 1) against the fixture's float64 gradient; an absent pair gradient equals a zero one"""
    from face_mask_inpaint_amd import functional as FF

    fx = golden("psp_train.pt")
    c = fx["head"][name]
    y_hat, y, ref, mask = head_inputs(fx, name)
    n, _, h, w = y_hat.shape
    inner = ref is not None
    g = torch.Generator().manual_seed(11)
    g_out = torch.randn(2 * n, h, w, 3, generator=g)
    g_in = torch.randn(2 * n, h, w, 3, generator=g) if inner else None
    g2 = (0.7, -1.3)
    yd, rd, md = _dev((y, ref, mask), dev)

    def run(use_out, use_in, g2):
        yh = _laid_out(y_hat.to(dev), layout).detach().requires_grad_(True)
        po, pi, l2, l2r = FF.psp_pixel_head(yh, yd, rd, md)
        total = l2 * g2[0]
        if inner:
            total = total + l2r * g2[1]
        if use_out is not None:
            total = total + (po * use_out.to(dev)).sum()
        if use_in is not None:
            total = total + (pi * use_in.to(dev)).sum()
        total.backward()
        return yh.grad.cpu()

    def check(got, want, mag, what):
        err = (got.double() - want).abs()
        worst = float((err / mag.clamp_min(1e-300)).max()) / U
        print(f"{name} {what}: worst error {worst:.2f} x 2^-24 x sum|terms| (bound 8)")
        assert bool(torch.isfinite(got).all()) and bool((err <= 8 * U * mag).all()), what

    got = run(g_out, g_in, g2)
    _, _, want, mag = restated(y_hat, y, ref, mask, g_out[:n], g_in[:n] if inner else None, g2)
    check(got, want, mag, "all four upstream gradients")
    got1 = run(None, None, (1.0, 1.0))
    _, _, want, mag = restated(y_hat, y, ref, mask)
    check(got1, want, mag, "g2 = (1, 1) against the restatement")
    check(got1, c["grad64"], mag, "g2 = (1, 1) against the fixture's float64 gradient")
    # an absent pair gradient equals a zero one (autograd hands the kernel a null pointer for an unused output)
    assert torch.equal(run(None, g_in, g2), run(torch.zeros_like(g_out), g_in, g2))
    if inner:
        assert torch.equal(run(g_out, None, g2), run(g_out, torch.zeros_like(g_in), g2))


def test_pixel_head_refuses_what_it_cannot_do(dev):
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd._lib import FmiError

    a = torch.zeros(2, 3, 8, 8, device=dev)
    m = torch.zeros(2, 8, 8, device=dev)
    for bad in (lambda: FF.psp_pixel_head(a.double(), a), lambda: FF.psp_pixel_head(a, a[:1]), lambda: FF.psp_pixel_head(a[:, :2], a[:, :2]),
                lambda: FF.psp_pixel_head(a, a, a, m[:, :4]), lambda: FF.psp_pixel_head(a, a.clone().requires_grad_(True)),
                lambda: FF.psp_pixel_head(a, a, a.clone().requires_grad_(True), m), lambda: FF.psp_pixel_head(a, a, a, m.clone().requires_grad_(True)),
                lambda: FF.psp_pixel_head(a.cpu(), a.cpu())):
        with pytest.raises(FmiError):
            bad()


def test_psp_loss_with_the_fused_head_against_reference(dev, golden):
    """the full-loss part of test_gpu_psp.py::test_lpips_id_and_full_psp_loss_against_reference with fused_head = True, at its bounds;
    then the same call without ref and mask against a float64 restatement of criteria/__init__.py:58-73"""
    from oracle import psp_cpu as PS  # checker
    from oracle.seeded import check_digest, criteria_inputs  # checker
    from test_oracle_criteria import criterion

    fx = golden("psp_criteria.pt")
    crit = criterion(fx).to(dev)
    assert crit.fused_head is False
    crit.fused_head = True
    x, y, rf, yh, mask = (t.to(dev) for t in criteria_inputs(fx["seeds"]["inputs"]))
    yh.requires_grad_(True)
    f = fx["psp_loss_full"]
    lat = f["latent"].to(dev).requires_grad_(True)
    loss, ld, id_logs = crit(x, y, yh, lat, latent_avg=f["latent_avg"].to(dev), ref=rf, mask=mask)
    assert abs(float(loss) / float(f["loss"]) - 1) <= 1e-3
    assert set(ld) == set(f["loss_dict"])
    for k, want in f["loss_dict"].items():
        assert abs(ld[k] - float(want)) <= 1e-3 * abs(float(want)) + 1e-6, (k, ld[k], float(want))
    loss.backward()
    check_digest(yh.grad, f["gy_hat"], 5e-3, "d loss / d y_hat")
    torch.testing.assert_close(lat.grad.cpu(), f["glatent"], rtol=1e-3, atol=1e-8)
    # ---- no ref, no mask: l2 and LPIPS on the plain images (the ID term, which has its own test, switched off)
    yh.grad = None
    crit.defer_logs, crit.id_lambda = True, 0.0
    loss, ld, _ = crit(x, y, yh, lat.detach(), latent_avg=None, ref=None, mask=None)
    assert list(ld) == ["loss_l2", "loss_lpips", "loss"] and all(torch.is_tensor(v) and v.is_cuda for v in ld.values())
    P = {k: v.detach().cpu().double() for k, v in crit.state_dict().items()}
    yh64 = yh.detach().cpu().double().requires_grad_(True)
    l2_64 = ((yh64 - y.cpu().double()) ** 2).mean()
    lp_64 = PS.lpips_alex(P, "lpips_loss.", yh64, y.cpu().double())
    loss64 = l2_64 * crit.l2_lambda + lp_64 * crit.lpips_lambda
    assert abs(float(ld["loss_l2"]) - float(l2_64)) <= 1e-3 * float(l2_64)
    assert abs(float(ld["loss_lpips"]) - float(lp_64)) <= 1e-3 * float(lp_64)
    assert abs(float(loss) - float(loss64)) <= 1e-3 * float(loss64) and float(ld["loss"]) == float(loss)
    loss.backward()
    loss64.backward()
    err = float((yh.grad.cpu().double() - yh64.grad).abs().max()) / float(yh64.grad.abs().max())
    print(f"no ref / no mask: d loss / d y_hat error {err:.2e} of the largest entry (bound 5e-3)")
    assert err <= 5e-3


# ---------------------------------------------------------------------------------------------------------------------------------
class _StandInGenerator(torch.nn.Module):
    """y = x * w per channel: an encoder with one parameter tensor, a decoder without parameters"""

    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Module()
        self.encoder.w = torch.nn.Parameter(torch.tensor([0.9, 1.1, 1.3]))
        self.decoder = torch.nn.Module()
        self.latent_avg = None
        self.calls = []

    def forward(self, x, ref=None, src_mask=None, return_latents=False, randomize_noise=True):
        self.calls.append((self.training, ref is not None, src_mask is not None, randomize_noise))
        return x * self.encoder.w.view(1, 3, 1, 1), self.encoder.w.view(1, 1, 3)


class _StandInLoss:
    """mean(y_hat^2), NaN on the chosen TRAINING calls; records the parameter it sees at every training call"""

    def __init__(self, gen, nan_calls):
        self.gen, self.nan_calls, self.train_calls, self.seen = gen, set(nan_calls), 0, []
        self.defer_logs = False

    def __call__(self, x, y, y_hat, latent, latent_avg=None, ref=None, mask=None):
        loss = (y_hat ** 2).mean()
        if self.gen.training:
            self.seen.append(self.gen.encoder.w.detach().clone())
            if self.train_calls in self.nan_calls:
                loss = loss * float("nan")
            self.train_calls += 1
        assert self.defer_logs is True
        return loss, {"loss": loss.detach()}, None


def _plateau(values, lr, patience=2, factor=0.8, threshold=1e-4):
    """ReduceLROnPlateau('max', patience, factor) restated: relative threshold, no cooldown; the learning rate after each value"""
    best, bad, out = -float("inf"), 0, []
    for v in values:
        if v > best * (1 + threshold) if best != -float("inf") else True:
            best, bad = v, 0
        else:
            bad += 1
        if bad > patience:
            lr, bad = lr * factor, 0
        out.append(lr)
    return out


@pytest.mark.parametrize("optimizer", ["adam", "ranger"])
def test_train_net_control_flow_with_stand_ins(dev, tmp_path, optimizer):
    from face_mask_inpaint_amd import train_psp as TP

    n_items, nan_calls, epochs = 20, (0, 5, 6, 27), 2
    g = torch.Generator().manual_seed(3)
    batch = lambda: dict(src_img=torch.rand(1, 3, 16, 16, generator=g).to(dev) * 2 - 1, gt_img=torch.rand(1, 3, 16, 16, generator=g).to(dev),
                         raw_gt_img=torch.rand(1, 3, 16, 16, generator=g).to(dev), ref_img=torch.rand(1, 3, 16, 16, generator=g).to(dev),
                         mask=torch.randint(0, 2, (1, 16, 16), generator=g).to(dev))
    train_loader, val_loader = [batch() for _ in range(n_items)], [batch() for _ in range(2)]
    gen = _StandInGenerator().to(dev)
    crit = _StandInLoss(gen, nan_calls)
    args = TP.get_args(["--optimizer", optimizer, "--use_ref"])
    events, history = [], {}
    out = TP.train_net(gen, dev, train_loader, val_loader, args, epochs=epochs, batch_size=1, learning_rate=1e-2, save_checkpoint=True,
                       dir_checkpoint=str(tmp_path / "ck"), run_name="run7", eval_options={"ssim"}, debug=False, callback=events.append,
                       history=history, psp_loss=crit)
    assert out is history and history["n_train"] == n_items and history["n_val"] == 2
    # the reference's loop, restated: global_step advances on finite losses only; the round test runs after EVERY batch
    division, gs, want_steps, want_skipped = n_items // (10 * 1), 0, [], []
    for i in range(epochs * n_items):
        if i in nan_calls:
            want_skipped.append(i)
        else:
            gs += 1
        if gs % division == 0:
            want_steps.append(gs)
    assert division == 2 and history["skipped"] == want_skipped and history["val_steps"] == want_steps
    assert want_steps[0] == 0 and want_steps.count(4) == 3  # a round before any step (batch 0 skipped) and the repeats after batches 5 and 6
    assert len(history["losses"]) == epochs * n_items - len(nan_calls) and all(np.isfinite(history["losses"]))
    for i in range(epochs * n_items - 1):  # a skipped step leaves the parameters as they were; a taken one moves them
        assert torch.equal(crit.seen[i], crit.seen[i + 1]) == (i in nan_calls), i
    steps = [e["step"] for e in events if "learning rate" not in e]
    assert steps == list(range(1, gs + 1))
    assert len(history["val"]) == len(want_steps) and all(set(v) == {"val loss", "ssim"} for v in history["val"])
    assert all(np.isfinite(v["val loss"]) and -1 <= v["ssim"] <= 1 for v in history["val"])
    want_lrs = _plateau([v["val loss"] for v in history["val"]], 1e-2)
    assert history["lrs"] == pytest.approx(want_lrs, rel=1e-12) and want_lrs[-1] < 1e-2  # the 'max' on a falling loss: it does reduce
    ck = [str(tmp_path / "ck" / "run7" / f"G_checkpoint_epoch{e}.pth") for e in (1, 2)]
    assert history["checkpoints"] == ck and all(os.path.isfile(p) for p in ck)
    sd = torch.load(ck[1], map_location="cpu", weights_only=True)
    assert list(sd) == ["encoder.w"] and torch.equal(sd["encoder.w"], gen.encoder.w.detach().cpu())
    assert gen.training
    # the forward calls: training ones with args.randomize_noise (False), evaluation ones with the default (True); ref and mask passed
    assert all(c[1] and c[2] for c in gen.calls)
    assert all(c[3] is False for c in gen.calls if c[0]) and all(c[3] is True for c in gen.calls if not c[0])
    assert sum(c[0] for c in gen.calls) == epochs * n_items and sum(not c[0] for c in gen.calls) == 2 * len(want_steps)


def _write_dataset(root, n=24, size=256):
    """n synthetic items in the trainers' layout: <id>.jpg, <id>_surgical.jpg, <id>.npy, and an identity file of n / 2 pairs"""
    from PIL import Image

    rng = np.random.RandomState(5)
    for d in ("src", "ref", "mask"):
        os.makedirs(os.path.join(root, d))
    lines = []
    for i in range(n):
        key = "%06d" % i
        base = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
        img = np.asarray(Image.fromarray(base).resize((size, size), Image.BICUBIC)).copy()
        y0, x0 = 60 + 3 * i, 40 + 2 * i
        m = np.zeros((size, size), np.uint8)
        m[y0:y0 + 100, x0:x0 + 120] = 255
        src = img.copy()
        src[m > 0] = 255
        Image.fromarray(img).save(os.path.join(root, "ref", key + ".jpg"), quality=92)
        Image.fromarray(src).save(os.path.join(root, "src", key + "_surgical.jpg"), quality=92)
        np.save(os.path.join(root, "mask", key + ".npy"), m)
        lines.append(f"{key}.jpg {i // 2}")
    with open(os.path.join(root, "identity.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def test_train_psp_end_to_end(dev, golden, tmp_path):
    """24 synthetic 256 x 256 items -> 21 training / 3 validation items at batch 2 (21 // 20 = 1: the smallest set on which the reference's
    rule validates at all); pSp(output_size=256) with attention, decoder trained, default lambdas, one epoch: 11 steps, 11 validation
    rounds, one checkpoint with the reference's keys that loads back every way it is used; the BatchNorm counters read 22 = 11 forwards x
    (src, ref).  Wall time on the MI355X: see DESIGN.md section 4."""
    from oracle.seeded import seeded_fill_, seeded_tensor  # checker
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd import train_psp as TP
    from face_mask_inpaint_amd.dataloader import get_reference_dataloader, to_device_batch
    from face_mask_inpaint_amd.modules.psp.criteria import pSpLoss
    from face_mask_inpaint_amd.modules.psp.psp import pSp
    from face_mask_inpaint_amd.optim import FusedAdam

    t0 = time.perf_counter()
    root = str(tmp_path / "data")
    _write_dataset(root)
    args = TP.get_args(["--data_root", root, "--src_img_path", "src", "--ref_img_path", "ref", "--mask_path", "mask", "--identity_file_path",
                        "identity.txt", "--batch_size", "2", "--output_size", "256", "--train_decoder", "1", "--use_ref", "--use_attention",
                        "--start_from_latent_avg", "--epochs", "1", "--checkpoint_path", str(tmp_path / "ck"), "--run_name", "e2e"])
    torch.manual_seed(0)
    train_loader, val_loader = get_reference_dataloader(args.src_img_path, args.ref_img_path, args.mask_path, args.identity_file_path, args.batch_size,
                                                        apply_transform=True, val_amount=0.1, img_scale=args.img_scale, use_ssim=True, device=dev)
    assert len(train_loader.indices) == 21 and len(val_loader.indices) == 3 and len(train_loader) == 11 and len(val_loader) == 1
    gen = pSp(args)
    seeded_fill_(gen, 777)
    gen = gen.to(dev)
    gen.latent_avg = seeded_tensor((args.n_styles, 512), 778, 0.5).to(dev)
    t1 = time.perf_counter()
    history = TP.train_net(gen, dev, train_loader, val_loader, args, epochs=1, batch_size=2, learning_rate=args.learning_rate, save_checkpoint=True,
                           dir_checkpoint=args.checkpoint_path, run_name=args.run_name, eval_options={"ssim", "ms_ssim"}, debug=False)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert len(history["losses"]) == 11 and all(np.isfinite(history["losses"])) and not history["skipped"]
    assert len(history["val"]) == 11 and history["val_steps"] == list(range(1, 12))
    for v in history["val"]:
        assert set(v) == {"val loss", "ssim", "ms_ssim"}
        assert np.isfinite(v["val loss"]) and 0 <= v["ssim"] <= 1 and 0 <= v["ms_ssim"] <= 1, v
    assert history["checkpoints"] == [str(tmp_path / "ck" / "e2e" / "G_checkpoint_epoch1.pth")]
    sd = torch.load(history["checkpoints"][0], map_location="cpu", weights_only=True)
    assert list(sd.keys()) == golden("psp_train.pt")["keys"]
    live = gen.state_dict()
    assert all(torch.equal(sd[k], live[k].cpu()) for k in sd)
    # every BatchNorm is in the encoder's input layer / body, which the reference runs on src AND on ref (psp_encoders.py:101-119): two
    # updates per training forward with --use_ref, as the reference's own run records (tests/golden/psp_whole.pt: 2 after one forward)
    per_forward = int(golden("psp_whole.pt")["stats_after"]["encoder.input_layer.1.num_batches_tracked"])
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert per_forward == 2 and len(tracked) == 52 and all(int(sd[k]) == 11 * per_forward for k in tracked)
    assert gen.training
    fresh = pSp(args).to(dev)
    fresh.load_state_dict(sd, strict=True)
    opts = types.SimpleNamespace(**{**vars(args), "pt_ckpt_path": history["checkpoints"][0]})
    via = pSp(opts)
    assert via.latent_avg is None
    for k, v in via.state_dict().items():
        assert torch.equal(v, sd[k]), k
    del via
    # ---- reproducible mode: the first three steps on one batch, twice, bit-identical
    batch = to_device_batch(next(iter(val_loader)), dev)
    crit = pSpLoss(args).to(dev)
    crit.fused_head = True
    crit_state = {k: v.clone() for k, v in crit.state_dict().items()}

    def three_steps():
        torch.manual_seed(123)
        fresh.load_state_dict(sd, strict=True)
        fresh.latent_avg = gen.latent_avg
        fresh.train()
        crit.load_state_dict(crit_state)
        params = [p for p in list(fresh.encoder.parameters()) + list(fresh.decoder.parameters()) if p.requires_grad]
        opt = FusedAdam(params, lr=1e-4)
        out = []
        with FF.deterministic():
            for _ in range(3):
                loss, _, stepped = TP.train_step(fresh, crit, opt, batch, args)
                assert stepped
                out.append(loss)
        return torch.stack(out).cpu()

    a, b = three_steps(), three_steps()
    t3 = time.perf_counter()
    print(f"end to end: data + model {t1 - t0:.1f} s, train_net (11 steps + 11 validation rounds) {t2 - t1:.1f} s, checks {t3 - t2:.1f} s; "
          f"losses {history['losses'][0]:.4f} -> {history['losses'][-1]:.4f}, ssim {history['val'][-1]['ssim']:.4f}")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (a, b)
