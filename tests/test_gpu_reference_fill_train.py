"""GPU: the PICNet trainer (face_mask_inpaint_amd/train_reference_fill.py) and the one-pass image head of GANOptimizer (csrc/ganhead.hip,
FF.gan_image_head, GANOptimizer.fused_head) against tests/golden/ref_train.pt (the reference's own scale_img / mask expressions / VGGLoss
operands in fp32 and float64, tools/golden/gen_reference_fill_train.py) and tests/golden/picnet_train_tiny.pt."""
import pytest
import torch

from test_host_reference_fill_train import CASES, U, backward_k, check_backward, check_forward, head_inputs, out_size, restated, upstream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _laid_out(t, layout):
    """the same [N, 3, H, W] values, contiguous ("planar") or in channels-last memory ("nhwc": what ReferenceFill.forward hands over)"""
    return t if layout == "planar" else t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _case(fx, name, dev):
    cfg = fx["head_inputs"][name]
    cpu = head_inputs(fx, name)
    c = fx["head"][name]
    pick = (lambda t: t[:, c["rows"]][:, :, c["cols"]]) if name == "e" else (lambda t: t)
    return cfg, c, cpu, [t.to(dev) for t in cpu], pick


@pytest.mark.parametrize("layout", ["planar", "nhwc"])
@pytest.mark.parametrize("name", CASES)
def test_image_head_forward_and_backward(dev, golden, name, layout):
    """cases a-e in both layouts of gen at the bounds of test_host_reference_fill_train.py (check_forward, check_backward with
    K = backward_k(contributors)); the backward of every case against the in-test float64 restatement with lerp_of's weights.  Repeated
    runs, one of them under FF.deterministic(), give the same bits, and an absent upstream gradient equals a zero one"""
    from face_mask_inpaint_amd import functional as FF

    fx = golden("ref_train.pt")
    cfg, c, cpu, (gen, gt, src, ref, mask), pick = _case(fx, name, dev)
    mean, std = fx["mean"].to(dev), fx["std"].to(dev)
    n, h, w = cfg["shape"]
    oh, ow = out_size(h, w, cfg["vgg_size"])
    gx, g_l1 = upstream(fx, name)
    g1 = torch.tensor(g_l1, dtype=torch.float32)
    want = restated(*cpu, fx["mean"], fx["std"], cfg["vgg_size"], gx, float(g1))

    def run(gx_dev, g1_dev):
        g = _laid_out(gen, layout).detach().requires_grad_(True)
        assert g.is_contiguous() == (layout == "planar")
        x_in, y_in, l1 = FF.gan_image_head(g, gt, src, ref, mask, mean, std, vgg_size=cfg["vgg_size"])
        assert x_in.shape == (3 * n, oh, ow, 3) and x_in.is_contiguous() and y_in.shape == x_in.shape and l1.dim() == 0
        assert x_in.requires_grad and not y_in.requires_grad
        obj = 0
        if gx_dev is not None:
            obj = obj + (x_in * gx_dev).sum()
        if g1_dev is not None:
            obj = obj + l1 * g1_dev
        (d,) = torch.autograd.grad(obj, g)
        assert d.stride() == g.stride()  # gen's own layout
        return x_in.detach(), y_in.detach(), l1.detach(), d

    x_in, y_in, l1, d = run(gx.to(dev), g1.to(dev))
    worst = check_forward(x_in.cpu(), y_in.cpu(), l1.cpu(), want, c, pick)
    k = backward_k(want["contributors"])
    worst["grad"] = check_backward(d.cpu(), want, k)
    print(name, layout, "K", k, worst)
    with FF.deterministic():
        again = run(gx.to(dev), g1.to(dev))
    for a, b in zip((x_in, y_in, l1, d), again):
        assert torch.equal(a, b)
    for a, b in zip((x_in, y_in, l1, d), run(gx.to(dev), g1.to(dev))):
        assert torch.equal(a, b)
    assert torch.equal(run(None, g1.to(dev))[3], run(torch.zeros_like(gx).to(dev), g1.to(dev))[3])
    assert torch.equal(run(gx.to(dev), None)[3], run(gx.to(dev), torch.zeros((), device=dev))[3])


@pytest.mark.parametrize("name", CASES)
def test_composed_path_meets_the_same_forward_bounds(dev, golden, name):
    """resize_bilinear of mask_mul and FF.l1_loss -- the operands GANOptimizer builds without the fused head -- on the same inputs at the
    same bounds: the bound is about the arithmetic, not about the restatement.  At 224 the composed operands are VGGLoss._input's"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd.modules.loss import GANOptimizer, VGGLoss

    fx = golden("ref_train.pt")
    cfg, c, cpu, (gen, gt, src, ref, mask), pick = _case(fx, name, dev)
    mean, std = fx["mean"].to(dev), fx["std"].to(dev)
    n, h, w = cfg["shape"]
    oh, ow = out_size(h, w, cfg["vgg_size"])
    inp = lambda img: FF.resize_bilinear(FF.to_nhwc(img), oh, ow, mean, std)
    xs = [gen, GANOptimizer._masked(gen, mask, True), GANOptimizer._masked(gen, mask, False)]
    ys = [gt, src, GANOptimizer._masked(ref, mask, False)]
    x_in, y_in = torch.cat([inp(v) for v in xs]), torch.cat([inp(v) for v in ys])
    l1 = FF.l1_loss(FF.to_nhwc(gen), FF.to_nhwc(gt))
    want = restated(*cpu, fx["mean"], fx["std"], cfg["vgg_size"])
    print(name, "composed", check_forward(x_in.cpu(), y_in.cpu(), l1.cpu(), want, c, pick))
    if name == "e":
        vgg = VGGLoss(8).to(dev)
        assert torch.equal(vgg.mean.view(3), mean) and torch.equal(vgg.std.view(3), std)
        assert torch.equal(torch.cat([vgg._input(v) for v in xs]), x_in)


def test_image_head_refuses_what_it_cannot_do(dev):
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd._lib import FmiError

    a, m, v = torch.zeros(1, 3, 4, 4, device=dev), torch.zeros(1, 4, 4, device=dev), torch.ones(3, device=dev)
    for i in range(1, 7):
        args = [a, a, a, a, m, v, v]
        args[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(FmiError, match="with respect to gen only"):
            FF.gan_image_head(*args)
    with pytest.raises(FmiError, match="fp32"):
        FF.gan_image_head(a, a, a.half(), a, m, v, v)
    with pytest.raises(FmiError, match="device tensors"):
        FF.gan_image_head(a, a, a, a, m.cpu(), v, v)
    x_in, y_in, l1 = FF.gan_image_head(a, a, a, a, m, v, v)  # no gradient wanted: fine
    assert x_in.shape == (3, 4, 4, 3) and float(l1) == 0.0


def test_forward_multi_prepared_equals_forward_multi(dev):
    """forward_multi is its operand construction followed by forward_multi_prepared: the same bits from the operands it builds"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd.modules.loss import GANOptimizer, VGGLoss

    torch.manual_seed(3)
    vgg = VGGLoss(8).to(dev)
    gen, gt, src, ref = (torch.rand(2, 3, 32, 32, device=dev) for _ in range(4))
    mask = (torch.rand(2, 32, 32, device=dev) < 0.4).float()
    triples = [(gen, gt, "perceptual"), (GANOptimizer._masked(gen, mask, True), src, "style"),
               (GANOptimizer._masked(gen, mask, False), GANOptimizer._masked(ref, mask, False), "contextual")]
    with FF.deterministic():
        a = vgg.forward_multi(triples)
        x = torch.cat([vgg._input(t[0]) for t in triples])
        y = torch.cat([vgg._input(t[1]) for t in triples])
        b = vgg.forward_multi_prepared(x, y, [t[2] for t in triples])
    assert len(a) == len(b) == 3
    for u, v in zip(a, b):
        assert torch.equal(u, v) and bool(torch.isfinite(u)) and float(u) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the helpers of tests/test_gpu_model.py::test_two_training_steps_against_reference_golden
def _load(mod, sd, dev):
    missing, unexpected = mod.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(".shortcut." in "." + k or ".module." in k for k in missing), missing
    return mod.to(dev)


def _tiny_models(fx, dev, fused=True):
    from face_mask_inpaint_amd.modules.loss import GANOptimizer
    from face_mask_inpaint_amd.modules.model import ReferenceFill
    from face_mask_inpaint_amd.modules.pluralistic_model import network
    from face_mask_inpaint_amd.optim import FusedAdam

    cfg = fx["config"]
    enc = dict(type="pluralistic", ngf=8, z_nc=cfg["enc_z_nc"], img_f=16, layers=5, norm="none", activation="LeakyReLU", L=cfg["enc_L"])
    dec = dict(ngf=8, z_nc=16, img_f=32, layers=5, norm="instance", activation="LeakyReLU", L=0)
    G = _load(ReferenceFill(None, dict(enc), dict(dec), use_att=True, out_size=(cfg["out_size"],) * 2), fx["G_sd0"], dev)
    D = _load(network.define_d(ndf=8, img_f=32, layers=cfg["disc_layers"], norm="none", activation="LeakyReLU", model_type="ResDis"), fx["D_sd0"], dev)
    optG = FusedAdam([p for p in G.parameters() if p.requires_grad], lr=cfg["lr"])
    optD = FusedAdam([p for p in D.parameters() if p.requires_grad], lr=cfg["lr"])
    gopt = GANOptimizer(optD, optG, vgg_width_div=cfg["vgg_div"])
    gopt.vgg_loss.load_state_dict(fx["V_sd"])
    gopt.fused_head = fused
    return G, D, gopt.to(dev), optG, optD


def _spy(opt, names_params, sink):
    orig = opt.step

    def step(closure=None):
        sink.append({n: p.grad.detach().cpu().clone() for n, p in names_params if p.grad is not None})
        return orig(closure)

    opt.step = step


def _reference_fp32_error(fx, key):
    worst = 0.0
    for step in (0, 1):
        st = fx[f"step{step}"]
        for n, g64 in st[f"{key}_grads64"].items():
            mx = float(g64.abs().max())
            if mx > 1e-12:
                worst = max(worst, float((st[f"{key}_grads"][n] - g64).abs().max()) / mx)
    return worst


def _check_grads_fp64(got, st, key, step, net_bound):
    for n, g64 in st[f"{key}_grads64"].items():
        assert n in got, f"missing grad {key}.{n}"
        mx = float(g64.abs().max())
        if mx <= 1e-12:
            assert float(got[n].abs().max()) <= 1e-6, f"{key} grad {n} step {step} should vanish"
            continue
        err = float((got[n] - g64).abs().max()) / mx
        ref = float((st[f"{key}_grads"][n] - g64).abs().max()) / mx
        assert err <= net_bound, f"{key} grad {n} step {step}: {err:.3e} of max|g| > {net_bound:.3e} (reference fp32: {ref:.3e})"
        if err > 2 * ref + 4e-6:
            assert key != "D", f"D grad {n} step {step}: {err:.3e} > 2 x reference's own {ref:.3e}"


def test_two_training_steps_with_the_fused_head_against_reference_golden(dev, golden):
    """the step-0 and restarted step-1 checks of test_gpu_model.py::test_two_training_steps_against_reference_golden at that test's own
    bounds, with ``gopt.fused_head = True``: generated image and the five losses against the imported reference (1e-3) and its float64
    values, every parameter gradient against the reference's float64 evaluation, SpectralNorm u / v after the step"""
    from face_mask_inpaint_amd import functional as FF

    fx = golden("picnet_train_tiny.pt")
    bound_g = 2 * _reference_fp32_error(fx, "G")
    bound_d = max(2 * _reference_fp32_error(fx, "D"), 1e-5)
    assert bound_g < 5e-3 and bound_d < 1e-4, (bound_g, bound_d)

    def run_step(G, D, gopt, s):
        m = FF.binarise_mask(s["mask"].to(dev))
        gen = G(s["src"].to(dev), s["ref"].to(dev), src_mask=m, eps=(s["eps_p"].to(dev), s["eps_q"].to(dev)))
        return gen, gopt(D, s["src"].to(dev), s["gt"].to(dev), s["ref"].to(dev), gen, m)

    def check_outputs(gen, losses, s, step):
        torch.testing.assert_close(gen.detach().cpu(), s["gen"], rtol=1e-3, atol=1e-5)
        d_loss, g_loss, perc, sty, cx = losses
        for got, key in ((g_loss, "g_loss"), (d_loss, "d_loss"), (perc, "perc"), (sty, "style"), (cx, "cx")):
            torch.testing.assert_close(got.detach().cpu(), s[key], rtol=1e-3, atol=1e-9, msg=lambda mm, key=key: f"{key} step {step}: {mm}")
        for got, want in zip(losses, s["losses64"]):
            assert abs(float(got) / float(want) - 1) <= 1e-3

    for step, sds in ((0, ("G_sd0", "D_sd0", "G_sd1", "D_sd1")), (1, ("G_sd1", "D_sd1", "G_sd2", "D_sd2"))):
        f = dict(fx)
        f["G_sd0"], f["D_sd0"] = fx[sds[0]], fx[sds[1]]
        G, D, gopt, optG, optD = _tiny_models(f, dev)
        assert gopt.fused_head
        grads = {"G": [], "D": []}
        _spy(optG, list(G.named_parameters()), grads["G"])
        _spy(optD, list(D.named_parameters()), grads["D"])
        s = fx[f"step{step}"]
        gen, losses = run_step(G, D, gopt, s)
        check_outputs(gen, losses, s, step)
        _check_grads_fp64(grads["G"][0], s, "G", step, bound_g)
        _check_grads_fp64(grads["D"][0], s, "D", step, bound_d)
        for mod, key in ((G, sds[2]), (D, sds[3])):
            sd = mod.state_dict()
            for k, v in fx[key].items():
                if k.endswith("weight_u") or k.endswith("weight_v"):
                    torch.testing.assert_close(sd[k].cpu(), v, rtol=1e-4, atol=1e-6, msg=lambda mm, k=k: f"{k}: {mm}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
N_TRAIN, N_VAL, LR = 10, 2, 1e-3


def _batches(count, seed, size):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        mask = torch.zeros(1, size, size, dtype=torch.int64)
        y0, x0 = (int(v) for v in torch.randint(4, size // 2, (2,), generator=g))
        mask[0, y0:y0 + size // 3, x0:x0 + size // 3] = 255  # a binary map as the dataset delivers it (int64): non-zero = masked
        out.append(dict(src_img=torch.rand(1, 3, size, size, generator=g), ref_img=torch.rand(1, 3, size, size, generator=g),
                        gt_img=torch.rand(1, 3, size, size, generator=g), mask=mask))
    return out


def _plateau(values, lr, patience=2, factor=0.8, threshold=1e-4):
    """host replay of torch's ReduceLROnPlateau('max', rel threshold): the learning rate after each value"""
    best, bad, out = -float("inf"), 0, []
    for v in values:
        if v > best * (1 + threshold):
            best, bad = v, 0
        else:
            bad += 1
        if bad > patience:
            lr, bad = lr * factor, 0
        out.append(lr)
    return out


def _fresh(fx, dev):
    G, D, gopt, _, _ = _tiny_models(fx, dev)
    return G, D, gopt


def _train(fx, dev, path, callback=None, built=None):
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd import train_reference_fill as TR

    size = fx["config"]["out_size"]
    G, D, gopt = _fresh(fx, dev)
    if built is not None:
        built(G, D)
    torch.manual_seed(11)
    with FF.deterministic():
        hist = TR.train_net(G, D, dev, _batches(N_TRAIN, 5, size), _batches(N_VAL, 6, size), epochs=1, batch_size=1, learning_rate=LR, save_checkpoint=True,
                            dir_checkpoint=str(path), run_name="run", eval_options={"ssim"}, callback=callback, gan_optimizer=gopt)
    return G, D, gopt, hist


@pytest.fixture(scope="module")
def trained(dev, golden, tmp_path_factory):
    """one epoch of train_net on the tiny models of picnet_train_tiny.pt (64 x 64, width-divided VGG handed over through gan_optimizer=):
    10 in-memory training batches of 1, 2 validation batches, under FF.deterministic() from torch.manual_seed"""
    fx = golden("picnet_train_tiny.pt")
    snaps, modes = [], []

    def callback(event):
        if "G train loss" in event:
            snaps.append([p.detach().clone() for p in D_ref[0].parameters()])
        else:
            modes.append((G_ref[0].training, D_ref[0].training))

    G_ref, D_ref = [None], [None]
    path = tmp_path_factory.mktemp("ref_train")
    G, D, gopt, hist = _train(fx, dev, path, callback, lambda g, d: (G_ref.__setitem__(0, g), D_ref.__setitem__(0, d)))
    return dict(G=G, D=D, gopt=gopt, hist=hist, snaps=snaps, modes=modes, path=path)


def test_train_net_history_cadence_schedulers_and_checkpoints(dev, golden, trained):
    import math
    import os
    import re

    fx, ref = golden("picnet_train_tiny.pt"), golden("ref_train.pt")
    h = trained["hist"]
    assert h["n_train"] == N_TRAIN and h["n_val"] == N_VAL
    assert len(h["losses_G"]) == len(h["losses_D"]) == N_TRAIN and all(math.isfinite(v) for v in h["losses_G"] + h["losses_D"])
    assert N_TRAIN // (10 * 1) == 1 and h["val_steps"] == list(range(1, N_TRAIN + 1))  # division_step == 1: a round after every step
    assert all(set(m) == {"D validation loss", "G validation loss", "ssim"} and all(math.isfinite(v) for v in m.values()) for m in h["val"])
    assert h["lrs_G"] == _plateau([m["G validation loss"] for m in h["val"]], LR)
    assert h["lrs_D"] == _plateau([m["D validation loss"] for m in h["val"]], LR)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR), "max", patience=2, factor=0.8)
    lrs = []
    for m in h["val"]:
        sch.step(m["G validation loss"])
        lrs.append(sch.optimizer.param_groups[0]["lr"])
    assert lrs == h["lrs_G"]
    assert trained["gopt"].fused_head and trained["gopt"].optimizer_G.param_groups[0]["lr"] == h["lrs_G"][-1]
    # nets back in train() after every evaluate
    assert trained["modes"] == [(True, True)] * N_TRAIN and trained["G"].training and trained["D"].training
    # checkpoints: names, strict loads into fresh models, the fixture's key structure
    run = os.path.join(str(trained["path"]), "run")
    assert [os.path.basename(p) for p in h["checkpoints"]] == ["G_checkpoint_epoch1.pth", "D_checkpoint_epoch1.pth"]
    assert sorted(os.listdir(run)) == ["D_checkpoint_epoch1.pth", "G_checkpoint_epoch1.pth"]
    G, D, _ = _fresh(fx, dev)
    for net, tag, trained_net, keys in ((G, "G", trained["G"], ref["keys_G"]), (D, "D", trained["D"], ref["keys_D"])):
        sd = torch.load(os.path.join(run, f"{tag}_checkpoint_epoch1.pth"), map_location="cpu", weights_only=True)
        net.load_state_dict(sd, strict=True)
        for k, v in trained_net.state_dict().items():
            assert torch.equal(v.cpu(), sd[k]), k
        # the architecture's prefix structure: the tiny nets are the default ones with fewer / narrower blocks and no mask detector, so
        # every key, block numbers aside, is one the reference's checkpoint has, under the same top-level modules
        pat = lambda ks: {re.sub(r"\d+", "#", k) for k in ks if not k.startswith("mask_detector.")}
        assert pat(sd) <= pat(keys), sorted(pat(sd) - pat(keys))[:5]
        assert {k.split(".")[0] for k in pat(sd)} == {k.split(".")[0] for k in pat(keys)}


def test_train_net_is_reproducible_and_equals_a_hand_written_loop(dev, golden, trained, tmp_path):
    """a second run from the same seeds gives the same bits; so does a loop written here over the same batches with the same optimisers,
    schedulers and fused GANOptimizer"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd import train_reference_fill as TR
    from face_mask_inpaint_amd.dataloader import to_device_batch
    from face_mask_inpaint_amd.optim import FusedAdam

    fx = golden("picnet_train_tiny.pt")
    h = trained["hist"]
    _, _, _, again = _train(fx, dev, tmp_path)
    assert again["losses_G"] == h["losses_G"] and again["losses_D"] == h["losses_D"] and again["val"] == h["val"]

    size = fx["config"]["out_size"]
    G, D, gopt = _fresh(fx, dev)
    optG = FusedAdam([p for p in G.parameters() if p.requires_grad], lr=LR)
    optD = FusedAdam([p for p in D.parameters() if p.requires_grad], lr=LR)
    schG = torch.optim.lr_scheduler.ReduceLROnPlateau(optG, "max", patience=2, factor=0.8)
    schD = torch.optim.lr_scheduler.ReduceLROnPlateau(optD, "max", patience=2, factor=0.8)
    gopt.optimizer_D, gopt.optimizer_G = optD, optG
    val = _batches(N_VAL, 6, size)
    lg, ld = [], []
    torch.manual_seed(11)
    with FF.deterministic():
        G.train(), D.train()
        for batch in _batches(N_TRAIN, 5, size):
            b = to_device_batch(batch, dev)
            gen = G(b["src_img"], b["ref_img"], src_mask=b["true_masks"])
            d_loss, g_loss, _, _, _ = gopt(D, b["src_img"], b["gt_img"], b["ref_img"], gen, b["true_masks"])
            lg.append(float(g_loss)), ld.append(float(d_loss))
            m = TR.evaluate(G, D, val, gopt.calc_loss, dev, 1, {"ssim"})
            schD.step(float(m["D validation loss"]))
            schG.step(float(m["G validation loss"]))
    assert lg == h["losses_G"] and ld == h["losses_D"]


def test_generator_pass_sees_the_updated_discriminator(dev, golden, trained):
    """G pass with D frozen, then the D step, then the next G pass with D frozen: the frozen pass must see the UPDATED D weights (a stale
    weight pack would not).  The D weights change between consecutive steps, and the second step's G loss differs from a run whose D was
    never updated while the first step's does not"""
    from face_mask_inpaint_amd import functional as FF
    from face_mask_inpaint_amd.dataloader import to_device_batch
    from face_mask_inpaint_amd.optim import FusedAdam

    snaps = trained["snaps"]
    assert len(snaps) == N_TRAIN
    for a, b in zip(snaps, snaps[1:]):
        assert any(not torch.equal(p, q) for p, q in zip(a, b))
    fx = golden("picnet_train_tiny.pt")
    size = fx["config"]["out_size"]
    G, D, gopt = _fresh(fx, dev)
    optG = FusedAdam([p for p in G.parameters() if p.requires_grad], lr=LR)
    optD = FusedAdam([p for p in D.parameters() if p.requires_grad], lr=LR)
    optD.step = lambda closure=None: None  # D is never updated
    gopt.optimizer_D, gopt.optimizer_G = optD, optG
    val = _batches(N_VAL, 6, size)
    from face_mask_inpaint_amd import train_reference_fill as TR

    lg = []
    torch.manual_seed(11)
    with FF.deterministic():
        for batch in _batches(2, 5, size):
            b = to_device_batch(batch, dev)
            gen = G(b["src_img"], b["ref_img"], src_mask=b["true_masks"])
            lg.append(float(gopt(D, b["src_img"], b["gt_img"], b["ref_img"], gen, b["true_masks"])[1]))
            TR.evaluate(G, D, val, gopt.calc_loss, dev, 1, {"ssim"})  # keeps the random stream of the trained run
    h = trained["hist"]
    assert lg[0] == h["losses_G"][0] and lg[1] != h["losses_G"][1]
