"""Bodies of the baseline-model tests (model/baseline_models.py: Linear_NIR, MLP_NIR), shared by the CPU suite (C ABI served by the
numpy emulator, tests/test_baselines_emulated.py) and the MI355X suite (tests/test_gpu_baselines.py).

Expected values: stock ``torch.nn`` in float64 on the CPU -- ``nn.Linear`` / ``nn.Sequential(Linear, ReLU, Linear, ReLU, Linear)`` on
the permuted input, ``F.mse_loss``, ``torch.optim.Adam`` -- which is literally the arithmetic of the reference's
model/baseline_models.py:17-23, 80-93, 28, 98, 70, 139.  Tolerances: prediction 1e-5 max-norm relative, loss 1e-3
relative, gradients 1e-3 relative L2 per tensor (3e-4 at full size); the two training routes agree to 1e-6 relative.
Parameters after 5 Adam steps: Adam divides every element by its own magnitude, so a per-tensor gradient bound does not carry over
element by element; the first steps move every element by ~lr whatever its size, so the check is on the MOVEMENT: per tensor
||dp - dp_ref||_2 <= 1e-2 ||dp_ref||_2 (ten times the gradient bound: an element at a tenth of its tensor's rms gradient may carry ten
times the tensor's relative error), and no single parameter further from the reference than the same 1e-2 of the largest possible
movement 5 lr, plus 1e-6 of the tensor's max for the fp32 storage of the parameter itself.
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

SHAPES = [(1, 5, 5), (3, 67, 93), (2, 64, 64)]
LR = 1e-3


def cfg(lr=LR):
    ns = types.SimpleNamespace
    return ns(base_configs=ns(learning_rate=lr, model_name="MLP_NIR"), custom_configs=ns(Logging=ns(num_val_images=0)))


def stock(kind):
    """the reference's module body (baseline_models.py:17, :80-86)"""
    if kind == "linear":
        return nn.Linear(3, 1)
    return nn.Sequential(nn.Linear(3, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 1))


PREFIX = {"linear": "linear.", "mlp": "mlp."}


def make(kind, seed, dev):
    from model.baseline_models import Linear_NIR, MLP_NIR
    torch.manual_seed(seed)
    m = (Linear_NIR if kind == "linear" else MLP_NIR)(cfg())
    return m.to(dev)


def ref64(kind, model):
    r = stock(kind).double()
    r.load_state_dict({k[len(PREFIX[kind]):]: v.detach().cpu().double() for k, v in model.state_dict().items()})
    return r


def ref_forward(r, rgb):
    B, _, H, W = rgb.shape
    return r(rgb.double().permute(0, 2, 3, 1).reshape(-1, 3)).reshape(B, 1, H, W)


def batch(shape, seed, dev=None):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    b = {"rgb": 0.02 + 0.58 * torch.rand(B, 3, H, W, generator=g), "nir": 0.05 + 0.75 * torch.rand(B, 1, H, W, generator=g)}
    return b if dev is None else {k: v.to(dev) for k, v in b.items()}


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def check(what, err, tol):
    print(f"{what}: {err:.3e} (bound {tol:g})")
    assert err == err and err <= tol, f"{what}: {err:.3e} > {tol:g}"


def ref_grads(kind, model, b):
    r = ref64(kind, model)
    pred = ref_forward(r, b["rgb"].cpu())
    loss = F.mse_loss(pred, b["nir"].cpu().double())
    loss.backward()
    return r, pred.detach(), loss.item(), {PREFIX[kind] + k: p.grad for k, p in r.named_parameters()}


def forward_loss_gradients(kind, shape, dev, grad_tol=1e-3, seed=3):
    """prediction, loss and every gradient of both routes (autograd bridge, fused train entry) against float64"""
    tag = f"{kind} {shape}"
    m = make(kind, seed, dev).train()
    b = batch(shape, seed + 100, dev)
    r, pred64, loss64, g64 = ref_grads(kind, m, b)
    pred = m(b["rgb"])
    assert pred.shape == b["nir"].shape and pred.requires_grad
    check(f"{tag} forward", relerr(pred, pred64), 1e-5)
    loss = m.training_step(b, 0)
    check(f"{tag} training_step loss", abs(loss.item() - loss64) / loss64, 1e-3)
    loss.backward()
    for k, p in m.named_parameters():
        check(f"{tag} autograd grad {k}", rel_l2(p.grad, g64[k]), grad_tol)
    # the fused entry, without its Adam step: gradients in the flat range, loss accumulated
    from nirgan_hip import pixmlp as PX
    flat = m._flat()
    lossbuf = torch.full((1,), 0.25, dtype=torch.float32, device=dev)
    flat.grad.fill_(7.0)                                       # overwritten, not accumulated
    PX.train(flat, m.hidden, b["rgb"].contiguous(), flat.grad, PX.workspace(b["rgb"], m.hidden), nir=b["nir"].contiguous(), loss=lossbuf)
    check(f"{tag} fused loss (accumulated onto 0.25)", abs(lossbuf.item() - 0.25 - loss64) / loss64, 1e-3)
    for k, gv in flat.grad_views().items():
        check(f"{tag} fused grad {k}", rel_l2(gv, g64[k]), grad_tol)
    used = torch.zeros(flat.total, dtype=torch.bool)
    for o, n, _ in flat.slices.values():
        used[o:o + n] = True
    assert (flat.grad.cpu()[~used] == 0).all(), "padding elements of the gradient range must be zero"
    return m, b


def five_adam_steps(kind, shape, dev, seed=5):
    """Lightning-style training_step + backward + optimizer.step() and train_batch, 5 steps each on one batch, against float64 Adam"""
    tag = f"{kind} {shape}"
    b = batch(shape, seed + 100, dev)
    m1, m2 = make(kind, seed, dev).train(), make(kind, seed, dev).train()
    r = ref64(kind, m1)
    p0 = {k: v.detach().cpu().double().clone() for k, v in m1.named_parameters()}
    ropt = torch.optim.Adam(r.parameters(), lr=LR)
    opt = m1.configure_optimizers()
    for i in range(5):
        ropt.zero_grad()
        F.mse_loss(ref_forward(r, b["rgb"].cpu()), b["nir"].cpu().double()).backward()
        ropt.step()
        opt.zero_grad()
        m1.training_step(b, i).backward()
        opt.step()
        view = m2.train_batch(b)
    assert set(view.as_dict()) == {"train/loss"} and m2.steps == 5 and m2._flat().step_count == 5 and m1._flat().step_count == 5
    ref = {PREFIX[kind] + k: v.detach() for k, v in r.named_parameters()}
    for (k, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
        check(f"{tag} routes agree {k}", relerr(a, c), 1e-6)
        for name, q in (("lightning", a), ("fused", c)):
            dq, dref = q.detach().cpu().double() - p0[k], ref[k] - p0[k]
            check(f"{tag} {name} movement after 5 Adam steps {k}", rel_l2(dq, dref), 1e-2)
            worst = (q.detach().cpu().double() - ref[k]).abs().max().item()
            check(f"{tag} {name} parameters after 5 Adam steps {k} (abs)", worst, 1e-2 * 5 * LR + 1e-6 * ref[k].abs().max().item())


def state_dict_and_seed(kind):
    from model.baseline_models import Linear_NIR, MLP_NIR
    for s in (0, 7):
        torch.manual_seed(s)
        m = (Linear_NIR if kind == "linear" else MLP_NIR)(cfg())
        torch.manual_seed(s)
        r = stock(kind)
        want = {PREFIX[kind] + k: v for k, v in r.state_dict().items()}
        got = m.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    m.load_state_dict({PREFIX[kind] + k: v + 1 for k, v in r.state_dict().items()}, strict=True)
    r2 = stock(kind)
    r2.load_state_dict({k[len(PREFIX[kind]):]: v for k, v in m.state_dict().items()}, strict=True)
    for k, v in r.state_dict().items():
        assert torch.equal(r2.state_dict()[k], v + 1)


def fit_checkpoint_resume(kind, dev, tmp_path):
    from nirgan_hip.fit import fit
    train = [batch((2, 16, 16), 20 + i) for i in range(3)]
    val = [batch((2, 16, 16), 30)]
    m = make(kind, 1, dev)
    ck = tmp_path / "b.ckpt"
    hist = fit(m, train, val, max_epochs=2, log_every=1, ckpt_path=str(ck), device=dev)
    assert len(hist["train"]) == 6 and all("train/loss" in r and r["train/loss"] > 0 for r in hist["train"])
    assert len(hist["val"]) == 2 and {"val/L1", "val/L2", "val/PSNR", "val/SSIM"} <= set(hist["val"][0])
    assert m.steps == 6 and m._flat().step_count == 6
    c = torch.load(str(ck), weights_only=False)
    assert c["global_step"] == 6 and len(c["optimizer_states"]) == 1 and c["lr_schedulers"] == []
    assert float(c["optimizer_states"][0]["state"][0]["step"]) == 6.0
    stock(kind).load_state_dict({k[len(PREFIX[kind]):]: v for k, v in c["state_dict"].items()}, strict=True)
    ropt = torch.optim.Adam(stock(kind).parameters(), lr=LR)
    ropt.load_state_dict(c["optimizer_states"][0])              # a stock Adam accepts the optimizer state
    # an uninterrupted third epoch == resume for one more epoch
    fit(m, train, val, max_epochs=1, log_every=0, device=dev)
    m2 = make(kind, 99, dev)
    h2 = fit(m2, train, val, max_epochs=3, log_every=0, resume_from=str(ck), device=dev)
    assert len(h2["val"]) == 1 and m2._flat().step_count == 9 and m._flat().step_count == 9
    for (k, a), (_, c2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a.detach().cpu(), c2.detach().cpu()), "resumed " + k
