"""GPU: the mask-detector trainer -- the fused CrossEntropy + Dice loss, its backward, the Dice score and the dice_* helpers against
the imported reference's fp32 and float64 runs (tests/golden/md_train.pt, tools/golden/gen_mask_detector_train.py), one training step
and four Adam steps of the training-mode UNet, and train_net end to end on an enlarged copy of the golden dataset.

Bounds.  Op level, nothing chaotic: ce within 16 * 2^-24 * max(1, max|logit|) of float64 (a few ulps per exp / log, double sums), dice and
the Dice score within 16 * 2^-24, every dlogits entry within 1e-3 of the tensor's largest (the project's fp32 bound).  Step level:
logits 1e-3 of the largest float64 entry, scalars max(4 x the reference fp32 run's own error, the op-level bound), gradients through
oracle.seeded.check_adjudicated (the error distribution of the reference's own fp32 run).  Every measured figure is printed."""
import os
import shutil

import pytest
import torch

from face_mask_inpaint_amd import train_mask_detector as TM  # every test here fails at import without the feature

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 16 * 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden):
    f = dict(golden("md_train.pt"))
    f["parts"] = {n: golden(os.path.join("md_train_parts", n + ".pt")) for n in f["parts"]}
    return f


def _case(fx, name):
    """(logits NHWC fp32, target uint8, the recorded values); the 1 x 1024^2 case is rebuilt from its seed"""
    from oracle.seeded import seeded_tensor  # checker

    c = fx["ops"][name]
    if name != "c2_big":
        return c["logits"], c["target"], c
    cfg = fx["config"]
    t = torch.zeros(1, 1024, 1024, dtype=torch.uint8)
    a, b, c0, d = cfg["big_rect"]
    t[0, a:b, c0:d] = 1
    return seeded_tensor((1, 1024, 1024, 2), cfg["big_seed"], cfg["big_scale"]), t, c


def _loss_and_grad(FF, x, t):
    x = x.clone().requires_grad_(True)
    loss, ce, dice = FF.seg_ce_dice_loss(x, t)
    assert loss.dim() == ce.dim() == dice.dim() == 0 and loss.is_cuda and not ce.requires_grad and not dice.requires_grad
    loss.backward()
    return loss.detach(), ce, dice, x.grad


@pytest.mark.parametrize("name", ["c2_odd", "c2_empty", "c3", "c3_odd", "c2_big"])
@pytest.mark.parametrize("kind", ["int64", "fp32"])
def test_loss_backward_and_score_against_float64(dev, fx, name, kind):
    from face_mask_inpaint_amd import functional as FF
    from oracle.seeded import check_digest, digest_error  # checker

    x, t8, c = _case(fx, name)
    t = t8.to(dev).to(torch.int64) if kind == "int64" else (t8 > 0).float().to(dev)  # the dataset's map (> 0 in the kernel), or a {0, 1} map
    loss, ce, dice, gx = _loss_and_grad(FF, x.to(dev), t)
    score = FF.seg_dice_score(x.to(dev), t)
    assert score.dim() == 0 and score.is_cuda
    mx = max(1.0, float(x.abs().max()))
    e_ce, e_dice, e_score = abs(float(ce) - float(c["ce64"])), abs(float(dice) - float(c["dice64"])), abs(float(score) - float(c["score64"]))
    g_nchw = gx.permute(0, 3, 1, 2).contiguous().cpu()
    if name == "c2_big":
        e_g = digest_error(g_nchw, c["dlogits64"])
    else:
        e_g = float((g_nchw.double() - c["dlogits64"]).abs().max()) / float(c["dlogits64"].abs().max())
    print("\n%s/%s: ce %.3e (bound %.3e; reference fp32 %.1e)  dice %.3e (bound %.3e; reference fp32 %.1e)  score %.3e  dlogits / max %.3e (bound 1e-3)" % (
        name, kind, e_ce, U * mx, abs(float(c["ce"] - c["ce64"])), e_dice, U, abs(float(c["dice"] - c["dice64"])), e_score, e_g))
    assert e_ce <= U * mx
    assert e_dice <= U
    assert abs(float(loss) - float(c["ce64"]) - float(c["dice64"])) <= U * mx + U
    assert e_score <= U and abs(float(score) - float(c["score"])) <= U
    assert e_g <= 1e-3
    if name == "c2_big":
        check_digest(g_nchw, c["dlogits64"], 1e-3, name)
    # two calls: bit-identical in default mode (fixed-order partial sums, no atomics)
    loss2, ce2, dice2, gx2 = _loss_and_grad(FF, x.to(dev), t)
    assert torch.equal(loss, loss2) and torch.equal(ce, ce2) and torch.equal(dice, dice2) and torch.equal(gx, gx2)
    assert torch.equal(score, FF.seg_dice_score(x.to(dev), t))


def test_upstream_gradient_is_a_device_scalar(dev, fx):
    """d(3 loss) = 3 d(loss): the factor reaches the kernel through autograd's device scalar"""
    from face_mask_inpaint_amd import functional as FF

    x, t8, _ = _case(fx, "c3")
    t = t8.to(dev).to(torch.int64)
    g1 = _loss_and_grad(FF, x.to(dev), t)[3]
    xx = x.to(dev).requires_grad_(True)
    (FF.seg_ce_dice_loss(xx, t)[0] * 3.0).backward()
    assert float((xx.grad - 3.0 * g1).abs().max()) <= 4 * 2.0 ** -24 * float(g1.abs().max()) * 3


def test_dice_score_special_samples(dev, fx):
    """empty target and empty prediction -> exactly 1; empty target, non-empty prediction -> eps / (n + eps); ties go to the first class"""
    from face_mask_inpaint_amd import functional as FF

    x, t8, _ = _case(fx, "c2_empty")
    x, t = x.to(dev), t8.to(dev).to(torch.int64)
    assert float(FF.seg_dice_score(x[1:2].contiguous(), t[1:2].contiguous())) == 1.0
    n_pred = int(x[2].argmax(-1).sum())
    got = float(FF.seg_dice_score(x[2:3].contiguous(), t[2:3].contiguous()))
    assert n_pred > 0 and abs(got - 1e-6 / (n_pred + 1e-6)) <= 1e-12
    tie = torch.zeros(1, 4, 4, 2, device=dev)  # every pixel tied: class 0 everywhere, whatever the target
    assert float(FF.seg_dice_score(tie, torch.zeros(1, 4, 4, dtype=torch.int64, device=dev))) == 1.0
    ones = torch.ones(1, 4, 4, dtype=torch.int64, device=dev)
    assert abs(float(FF.seg_dice_score(tie, ones)) - 1e-6 / (16 + 1e-6)) <= 1e-12
    tie[..., 1] = 1.0
    assert float(FF.seg_dice_score(tie, ones)) == 1.0


@pytest.mark.parametrize("name", ["c2_empty", "c3"])
def test_dice_helpers_against_the_reference(dev, fx, name):
    """dice_coeff / multiclass_dice_coeff / dice_loss on fp32 probabilities and one-hot targets.  The inputs are the float64 probabilities
    rounded to fp32 (2^-24 relative each), the sums are double: 16 * 2^-24 against the float64 values"""
    from face_mask_inpaint_amd.modules import loss as L

    x, t8, c = _case(fx, name)
    n_classes = x.shape[-1]
    probs = torch.softmax(x.double().permute(0, 3, 1, 2), 1).float().to(dev)
    onehot = torch.nn.functional.one_hot((t8 > 0).long(), n_classes).permute(0, 3, 1, 2).float().to(dev)
    got = {}
    for rbf in (False, True):
        got[f"dice_coeff_{int(rbf)}"] = L.dice_coeff(probs[:, 1], onehot[:, 1], reduce_batch_first=rbf)
        got[f"multiclass_{int(rbf)}"] = L.multiclass_dice_coeff(probs, onehot, reduce_batch_first=rbf)
    got["dice_coeff_2d"] = L.dice_coeff(probs[0, 1], onehot[0, 1])
    got["dice_loss"] = L.dice_loss(probs[:, 1], onehot[:, 1], multiclass=False)
    got["dice_loss_multiclass"] = L.dice_loss(probs, onehot, multiclass=True)
    for k, v in got.items():
        assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32, k
        e, e_ref = abs(float(v) - float(c["helpers64"][k])), abs(float(c["helpers"][k]) - float(c["helpers64"][k]))
        print("\n%s %-22s %.9f  error %.2e (reference fp32 %.2e)" % (name, k, float(v), e, e_ref))
        assert e <= U, k
    # ranks the reference's recursion takes besides [N, C, H, W]: [N, C, W] (each class ONE mask, loss.py:156) and [N, C, D, H, W]
    def coeff(a, b, eps=1e-6):
        a, b = a.double().cpu(), b.double().cpu()
        tot = float(a.sum() + b.sum())
        inter = float((a * b).sum())
        return (2 * inter + eps) / ((2 * inter if tot == 0 else tot) + eps)

    p3, o3 = probs[:, :, 0].contiguous(), onehot[:, :, 0].contiguous()
    want = sum(coeff(p3[:, k], o3[:, k]) for k in range(n_classes)) / n_classes
    assert abs(float(L.multiclass_dice_coeff(p3, o3)) - want) <= U
    with pytest.raises(ValueError):
        L.multiclass_dice_coeff(p3, o3, reduce_batch_first=True)
    p5, o5 = probs.unsqueeze(2).repeat(1, 1, 2, 1, 1), onehot.unsqueeze(2).repeat(1, 1, 2, 1, 1)
    want = sum(coeff(p5[i, k, d], o5[i, k, d]) for i in range(p5.shape[0]) for k in range(n_classes) for d in range(2)) / (p5.shape[0] * n_classes * 2)
    assert abs(float(L.multiclass_dice_coeff(p5, o5)) - want) <= U
    want = sum(coeff(p5[:, k], o5[:, k]) for k in range(n_classes)) / n_classes
    assert abs(float(L.multiclass_dice_coeff(p5, o5, reduce_batch_first=True)) - want) <= U
    # the evaluate() composition through the general helpers equals the fused metric
    from face_mask_inpaint_amd import functional as FF

    pred = torch.nn.functional.one_hot(x.argmax(-1), n_classes).permute(0, 3, 1, 2).float().to(dev)
    general = L.multiclass_dice_coeff(pred[:, 1:, ...], onehot[:, 1:, ...], reduce_batch_first=False)
    assert abs(float(general) - float(FF.seg_dice_score(x.to(dev), t8.to(dev).to(torch.int64)))) <= 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------------------
def _step_setup(fx, dev):
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from oracle.seeded import seeded_fill_  # checker

    cfg = fx["config"]
    net = MaskDetector(n_channels=3, bilinear=True)
    seeded_fill_(net, cfg["md_seed"])
    net = net.to(dev).train()
    x = torch.rand(tuple(cfg["step_shape"]), generator=torch.Generator().manual_seed(cfg["x_seed"])).to(dev)
    t = fx["step"]["target"].to(dev).to(torch.int64)  # 0 / 255 / 1: the dataset's map, binarised in the kernel
    return net, x, t


BN_BIAS = ("double_conv.0.bias", "double_conv.3.bias")  # convolution biases in front of a BatchNorm: their true gradient is zero


def test_one_training_step_against_the_reference(dev, fx):
    """forward, fused loss and backward of the train-mode UNet on the fixture batch: logits, ce / dice / loss, the 56 gradients through
    check_adjudicated with its default factors, the 18 zero-gradient biases, the BatchNorm running statistics.
    The step runs under FF.deterministic(): an fp32 gradient's worst entry is decided by single ReLU mask elements whose pre-activation
    lies inside the forward rounding error, and in default mode fp32 atomics move that rounding from run to run, so
    the same tree would meet or miss the worst-case limit by chance; in reproducible mode the outcome belongs to the build."""
    from face_mask_inpaint_amd import functional as FF
    from oracle.seeded import check_adjudicated  # checker

    st, P = fx["step"], fx["parts"]
    net, x, t = _step_setup(fx, dev)
    with FF.deterministic():
        logits = net.model.nhwc(FF.to_nhwc(x))
        loss, ce, dice = FF.seg_ce_dice_loss(logits, t)
        loss.backward()
    loss, ce, dice = loss.detach(), ce.detach(), dice.detach()
    l64 = P["step_logits64"]
    got = logits.detach().permute(0, 3, 1, 2).cpu()
    e = float((got.double() - l64.double()).abs().max()) / float(l64.abs().max())
    e_ref = float((P["step_logits"].double() - l64.double()).abs().max()) / float(l64.abs().max())
    print("\nstep: logits / max|logit| %.2e (the reference's fp32 run %.2e; bound 1e-3)" % (e, e_ref))
    assert e <= 1e-3
    mx = max(1.0, float(l64.abs().max()))
    for k, v, op_bound in (("ce", ce, U * mx), ("dice", dice, U), ("loss", loss, U * mx + U)):
        err, ref_err = abs(float(v) - float(st[k + "64"])), abs(float(st[k]) - float(st[k + "64"]))
        print("step: %-4s %.9f  error %.2e (reference fp32 %.2e; bound %.2e)" % (k, float(v), err, ref_err, max(4 * ref_err, op_bound)))
        assert err <= max(4 * ref_err, op_bound), k
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert len(grads) == 74 and all(g is not None for g in grads.values())
    zero = [n for n in grads if n.endswith(BN_BIAS)]
    assert len(zero) == 18
    d32 = {n: d for n, d in P["step_gparams"].items() if n not in zero}
    d64 = {n: d for n, d in P["step_gparams64"].items() if n not in zero}
    assert len(d64) == 56
    check_adjudicated(grads, d32, d64, what="mask-detector step")
    for n in zero:
        g, gw = grads[n], grads[n[:-len("bias")] + "weight"]
        assert bool(torch.isfinite(g).all()), n
        assert float(g.abs().max()) < 1e-3 * float(gw.abs().max()), (n, float(g.abs().max()), float(gw.abs().max()))
    sd = net.state_dict()
    worst = 0.0
    for k, want in st["bn64"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(want) == 1, k
            continue
        err = float((sd[k].cpu().double() - want.double()).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-3, (k, err)
    assert len(st["bn64"]) == 54
    print("step: BatchNorm running statistics, worst error / max %.2e (bound 1e-3)" % worst)


def _four_steps(fx, dev):
    from face_mask_inpaint_amd.optim import FusedAdam

    net, x, t = _step_setup(fx, dev)
    opt = FusedAdam(net.parameters(), lr=fx["config"]["lr"])
    losses = [TM.train_step(net, opt, x, t) for _ in range(fx["config"]["steps"])]
    assert all(l.is_cuda and l.dim() == 0 and not l.requires_grad for l in losses)
    return net, torch.stack(losses).cpu()


def test_trajectory_of_four_adam_steps(dev, fx):
    """the losses of 4 x train_step at lr 1e-5 against the reference's float64 trajectory.  Parameters after an Adam step are NOT compared
    with the reference: the first step moves every entry by +-lr whatever its gradient's size, and entries whose gradient is rounding
    noise go either way -- the reference's own fp32 and float64 parameters are ~4 lr apart after two steps.  Reproducibility of the
    parameters is asserted instead."""
    from face_mask_inpaint_amd import functional as FF

    tr = fx["trajectory"]
    _, losses = _four_steps(fx, dev)
    ref_dev = float((tr["losses"] - tr["losses64"]).abs().max())
    bound = max(4 * ref_dev, 1e-5)
    err = (losses.double() - tr["losses64"]).abs()
    print("\ntrajectory: losses %s; error vs float64 %s (reference fp32 deviates by %.2e; bound %.2e)" % (
        ["%.7f" % v for v in losses.tolist()], ["%.2e" % v for v in err.tolist()], ref_dev, bound))
    assert bool(torch.isfinite(losses).all()) and float(err.max()) <= bound
    assert float(losses[-1]) < float(losses[0])  # as in the reference's run
    assert float(tr["losses64"][-1]) < float(tr["losses64"][0])
    with FF.deterministic():
        net_a, la = _four_steps(fx, dev)
        net_b, lb = _four_steps(fx, dev)
    assert torch.equal(la, lb)
    sa, sb = net_a.state_dict(), net_b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _lr_rule(scores, lr, patience=2, factor=0.1, threshold=1e-4, eps=1e-8):
    """ReduceLROnPlateau(optimizer, 'max', patience=2) with torch's defaults (rel threshold, no cooldown, min_lr 0), restated"""
    best, bad, out = float("-inf"), 0, []
    for s in scores:
        if s > best * (1 + threshold):
            best, bad = s, 0
        else:
            bad += 1
        if bad > patience:
            if lr - lr * factor > eps:
                lr = lr * factor
            bad = 0
        out.append(lr)
    return out


def test_train_net_end_to_end(dev, fx, tmp_path):
    """2 epochs on 24 items (the 8 golden 40 x 48 pairs under new ids; with 8 the reference's rule n_train // (10 * batch_size) is 0 and no
    validation would run): 20 training items, 4 validation items, batch 2 -> a validation round after every step.  A score of exactly 0
    is legitimate (with seeded running statistics the eval-mode network predicts one class everywhere; so did the reference)."""
    from face_mask_inpaint_amd.modules.mask_detector import MaskDetector
    from oracle.seeded import seeded_fill_  # checker

    src = os.path.join(ROOT, "tests", "golden", "dataset")
    img, msk, ckpt = tmp_path / "images_masked", tmp_path / "binary_map", tmp_path / "ckpt"
    img.mkdir(), msk.mkdir()
    ids = sorted(f.split("_")[0] for f in os.listdir(os.path.join(src, "images_masked")))
    assert len(ids) == 8
    for r in range(3):
        for i in ids:
            shutil.copy(os.path.join(src, "images_masked", i + "_surgical.jpg"), img / f"{r + 2}{i}_surgical.jpg")
            shutil.copy(os.path.join(src, "binary_map", i + ".npy"), msk / f"{r + 2}{i}.npy")
    net = MaskDetector(n_channels=3, bilinear=True)
    seeded_fill_(net, fx["config"]["md_seed"])
    net.to(dev)
    events = []
    lr0 = 1e-5
    hist = TM.train_net(net, dev, epochs=2, batch_size=2, learning_rate=lr0, val_percent=1 / 6, save_checkpoint=True, img_scale=1.0, amp=False,
                        dir_img=img, dir_mask=msk, dir_checkpoint=ckpt, seed=7, callback=events.append)
    assert hist["n_train"] == 20 and hist["n_val"] == 4
    assert len(hist["losses"]) == 20 and all(isinstance(v, float) and v == v and abs(v) != float("inf") for v in hist["losses"])
    assert len(hist["val_scores"]) == 20 and hist["val_steps"] == list(range(1, 21))
    assert all(0.0 <= s <= 1.0 for s in hist["val_scores"])
    want = _lr_rule(hist["val_scores"], lr0)
    print("\ntrain_net: losses %.5f .. %.5f; validation scores %s; learning rates %s" % (hist["losses"][0], hist["losses"][-1],
                                                                                      sorted(set(hist["val_scores"])), sorted(set(hist["lrs"]))))
    assert len(hist["lrs"]) == 20 and all(abs(a - b) <= 1e-12 * lr0 + 1e-20 for a, b in zip(hist["lrs"], want)), (hist["lrs"], want)
    assert sum("validation Dice" in e for e in events) == 20 and sum("train loss" in e for e in events) == 20
    assert [os.path.basename(p) for p in hist["checkpoints"]] == ["checkpoint_epoch1.pth", "checkpoint_epoch2.pth"]
    assert net.training
    for p in hist["checkpoints"]:
        sd = torch.load(p, weights_only=True)
        assert list(sd.keys()) == fx["keys"]
        fresh = MaskDetector(n_channels=3, bilinear=True)
        fresh.load_state_dict(sd, strict=True)
    last = torch.load(hist["checkpoints"][-1], weights_only=True)
    assert all(torch.equal(v.cpu(), last[k].cpu()) for k, v in net.state_dict().items())
    assert int(last["model.inc.double_conv.1.num_batches_tracked"]) == 20
