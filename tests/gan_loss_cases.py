"""Bodies of the tests of the vanilla and wgangp GAN objectives (nirgan_gan_loss, functional.GanLossFn, networks.GANLoss, the fused
trainer's ``gan_mode``), shared by the CPU suite (the numpy statement tests/emu_gan_loss.py: tests/test_gan_loss_emulated.py) and the
MI355X suite (the HIP library: tests/test_gpu_gan_loss.py).  Every body takes ``dev``.

Reference: stock torch in float64 on the CPU -- ``BCEWithLogitsLoss()(x64, full_like(x64, t))`` for vanilla, ``-x64.mean()`` (real) /
``+x64.mean()`` (fake) for wgangp, gradients from autograd on these.  The oracle is not involved.

Bounds (u = 2^-24)
  gradient, vanilla   |got - ref| <= 8 u |weight| / n per element, absolute: sigmoid - t is at most 1 in magnitude and comes from one
                      expf, one division and one subtraction, then two products; cancellation near sigmoid = t rules a relative bound out
  gradient, wgangp    bitwise fp32((s * weight) * (1.f / (float)n)), the header's statement
  loss                measured: e32 is the relative error against float64 of the same loss evaluated by stock torch in fp32 on the CPU
                      on the same input; the entry has to lie within 8 max(e32, u) of float64 (the summation orders differ and neither
                      is privileged; eight leaves room for a tree against a sequential order at these n).  Every case prints e32 and the
                      entry's error before it asserts.
"""
import functools

import numpy as np
import torch

from nirgan_hip import lib as L

U = 2.0 ** -24
MODES = ("vanilla", "wgangp")
SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 1800)      # one short of / past the wave, workgroup and vector widths; 2*30*30
TARGETS = (1.0, 0.0, 0.9)
WEIGHTS = (1.0, 0.37)
# value -> position: where n allows; spread over the first wave, the wave and workgroup edges and the second trip's first element
PLANTED = ((0.0, 0), (1e-4, 2), (-1e-4, 5), (20.0, 17), (-20.0, 40), (88.0, 62), (-88.0, 64), (100.0, 130), (-100.0, 255),
           (1e4, 256), (-1e4, 1024))
SENT = -7.25e11                                                    # guard value around grad and loss_out
GUARD = 64
FUSED_TOL = 1e-4        # fused step against the autograd route: the bound of the lsgan pair, tests/test_host_logic_emulated.py:296
PARITY = 1e-3           # README: 1e-3 relative against the float64 reference (losses; rel L2 of every gradient)


def stream(dev):
    return torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else None


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rel(got, ref):
    got, ref = float(got), float(ref)
    if ref == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - ref) / abs(ref)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """randn * 3 with the planted values; computed once, nobody writes to it"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(1000 + n)) * 3
    for v, at in PLANTED:
        if at < n:
            x[at] = v
    return x


def objective(mode, x, t):
    """the reference's GANLoss on stock torch, in the dtype of x"""
    if mode == "vanilla":
        return torch.nn.BCEWithLogitsLoss()(x, torch.full_like(x, t))
    return -x.mean() if t > 0.5 else x.mean()


@functools.lru_cache(maxsize=None)
def reference(mode, n, t, w):
    """(float64 loss, float64 gradient, e32) of weight * objective"""
    x64 = inputs(n).double().requires_grad_(True)
    loss = w * objective(mode, x64, t)
    loss.backward()
    l32 = (w * objective(mode, inputs(n).clone(), t)).item()
    return loss.item(), x64.grad.clone(), rel(l32, loss.item())


def launch(dev, mode, x, t, w, with_grad=True, calls=1):
    """the entry on guarded buffers: (loss_out[0], grad or None); the guards are checked here"""
    n = x.numel()
    lbuf = torch.full((2 * GUARD + 1,), SENT, device=dev)
    lbuf[GUARD] = 0.0
    gbuf = torch.full((2 * GUARD + n,), SENT, device=dev)
    for _ in range(calls):
        L.call("nirgan_gan_loss", x.data_ptr(), n, L.GAN_MODES[mode], t, w, lbuf.data_ptr() + 4 * GUARD,
               gbuf.data_ptr() + 4 * GUARD if with_grad else None, stream(dev))
    sync(dev)
    lb, gb = lbuf.cpu(), gbuf.cpu()
    assert (lb[:GUARD] == SENT).all() and (lb[GUARD + 1:] == SENT).all(), "a write next to loss_out"
    assert (gb[:GUARD] == SENT).all() and (gb[GUARD + n:] == SENT).all(), "a write next to grad"
    if not with_grad:
        assert (gb == SENT).all(), "grad = NULL wrote a gradient"
    return lb[GUARD].clone(), (gb[GUARD:GUARD + n].clone() if with_grad else None)


def check_loss(tag, got, ref, e32):
    err = rel(got, ref)
    print(f"GANLOSS {tag} | e32 {e32:.3e} | entry {err:.3e} | bound {8 * max(e32, U):.3e}")
    assert np.isfinite(float(got)), tag
    assert err <= 8 * max(e32, U), f"{tag}: loss {float(got)!r} against {ref!r}: {err:.3e} > 8 max({e32:.3e}, 2^-24)"


def check_grad(tag, mode, got, ref, n, t, w):
    assert torch.isfinite(got).all(), tag + ": non-finite gradient"
    if mode == "wgangp":
        want = (np.float32(-w if t > 0.5 else w)) * (np.float32(1) / np.float32(n))
        assert isinstance(want, np.float32)
        assert torch.equal(bits(got), bits(torch.full((n,), float(want)))), f"{tag}: gradient bits"
        assert abs(float(want) - ref[0].item()) <= 4 * U * abs(ref[0].item())     # and that statement is the float64 gradient
        return
    err = (got.double() - ref).abs().max().item()
    bound = 8 * U * abs(w) / n
    print(f"GANLOSS {tag} | grad err / bound {err / bound:.3e}")
    assert err <= bound, f"{tag}: gradient off by {err:.3e} > {bound:.3e}"


def kernel_case(dev, mode, n):
    """every target and weight at one size: loss, gradient, guards, accumulation, forward only, two runs"""
    x = inputs(n).to(dev)
    for t in TARGETS:
        for w in WEIGHTS:
            tag = f"{mode} n {n} t {t} w {w}"
            ref_l, ref_g, e32 = reference(mode, n, t, w)
            loss, grad = launch(dev, mode, x, t, w)
            check_loss(tag, loss, ref_l, e32)
            check_grad(tag, mode, grad, ref_g, n, t, w)
            twice, grad2 = launch(dev, mode, x, t, w, calls=2)
            check_loss(tag + " two calls", twice, 2 * ref_l, e32)
            assert torch.equal(bits(grad2), bits(grad)), tag + ": the gradient is overwritten, not accumulated"
            fwd, _ = launch(dev, mode, x, t, w, with_grad=False)
            assert torch.equal(bits(fwd), bits(loss)), tag + ": grad = NULL changes the loss bits"
            again_l, again_g = launch(dev, mode, x, t, w)
            assert torch.equal(bits(again_l), bits(loss)) and torch.equal(bits(again_g), bits(grad)), tag + ": two runs differ"


def odd_offset_case(dev, mode, n=1800):
    """pred one float into a larger buffer (4-byte aligned only): the same bits as the aligned run"""
    x = inputs(n).to(dev)
    big = torch.zeros(n + 7, device=dev)
    big[1:1 + n] = x
    view = big[1:1 + n]
    assert view.data_ptr() % 8 == 4
    for t, w in ((1.0, 1.0), (0.9, 0.37)):
        ref_l, ref_g, e32 = reference(mode, n, t, w)
        loss, grad = launch(dev, mode, view, t, w)
        check_loss(f"{mode} n {n} t {t} w {w} odd offset", loss, ref_l, e32)
        check_grad(f"{mode} n {n} t {t} w {w} odd offset", mode, grad, ref_g, n, t, w)
        l0, g0 = launch(dev, mode, x, t, w)
        assert torch.equal(bits(l0), bits(loss)) and torch.equal(bits(g0), bits(grad))


def argument_errors(be):
    """on the library itself: every refusal comes before any launch, so no GPU is needed"""
    x = torch.zeros(8)
    out = torch.zeros(1)
    for args in ((x.data_ptr(), 8, 0, 1.0, 1.0, out.data_ptr(), None, None),          # mode 0: lsgan has its own entry
                 (x.data_ptr(), 8, 3, 1.0, 1.0, out.data_ptr(), None, None),
                 (x.data_ptr(), 0, 1, 1.0, 1.0, out.data_ptr(), None, None),
                 (None, 8, 1, 1.0, 1.0, out.data_ptr(), None, None),
                 (x.data_ptr(), 8, 2, 1.0, 1.0, None, None, None)):
        assert be.nirgan_gan_loss(*args) == -1, args
        msg = be.nirgan_last_error()
        assert "gan_loss" in (msg.decode() if isinstance(msg, bytes) else msg), msg
    assert out[0] == 0


# ------------------------------------------------------------------------------------------------ module
def construction():
    from model import networks
    for mode in MODES:
        crit = networks.GANLoss(mode)
        assert list(crit.state_dict().keys()) == ["real_label", "fake_label"]
        assert crit.real_label.item() == 1.0 and crit.fake_label.item() == 0.0 and crit.gan_mode == mode
        smoothed = networks.GANLoss(mode, 0.9, 0.1)
        assert abs(smoothed.real_label.item() - 0.9) < 1e-7 and abs(smoothed.fake_label.item() - 0.1) < 1e-7
    import pytest
    with pytest.raises(NotImplementedError):
        networks.GANLoss("hinge")


def autograd_route(dev, mode):
    """crit(pred, real / fake).backward() against float64 within the kernel bounds; an in-place edit of real_label reaches the kernel"""
    from model import networks
    n = 1800
    crit = networks.GANLoss(mode).to(dev)
    for real, t in ((True, 1.0), (False, 0.0), (True, 0.9)):
        if t == 0.9:
            crit.real_label.fill_(0.9)
        ref_l, ref_g, e32 = reference(mode, n, t, 1.0)
        pred = inputs(n).reshape(2, 1, 30, 30).to(dev).requires_grad_(True)
        loss = crit(pred, real)
        assert loss.dim() == 0 and loss.requires_grad
        (3.0 * loss).backward()                                   # the upstream scalar multiplies the stored gradient
        check_loss(f"GANLoss({mode}) real {real} t {t}", loss.detach().cpu(), ref_l, e32)
        g3 = pred.grad.detach().cpu().reshape(-1)
        if mode == "wgangp":
            check_grad(f"GANLoss({mode}) real {real} t {t}", mode, g3 / 3.0, ref_g, n, t, 1.0)
        else:
            err = (g3.double() - 3.0 * ref_g).abs().max().item()
            assert err <= 3.0 * (8 + 1) * U / n, f"GANLoss({mode}) t {t}: gradient off by {err:.3e}"      # + the product with 3


# ------------------------------------------------------------------------------------------------ fused trainer
def make_model(dev, mode, ngf=8, golden_dir=None, seed=0):
    """Px2Px_PL of tests/api_cases.py's config with ``gan_mode``; the small golden nets' weights when ngf == 8"""
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, ngf)
    cfg.base_configs.gan_mode = mode
    torch.manual_seed(seed)
    m = Px2Px_PL(cfg)
    if golden_dir is not None:
        A._load_golden_weights(m, A.load(golden_dir, "f1_g6_d.npz"), False)
    return m.to(dev).train()


def batch64(dev, B=2, size=64):
    g = torch.Generator().manual_seed(3)
    return {"rgb": (0.02 + 0.58 * torch.rand(B, 3, size, size, generator=g)).to(dev),
            "nir": (0.05 + 0.75 * torch.rand(B, 1, size, size, generator=g)).to(dev)}


def fused_step(m, batch):
    """one train_batch: (losses, gradients of D, gradients of G)"""
    out = m.train_batch(batch).as_dict()
    tr = m.fused_trainer()
    gD = {k: v.detach().cpu().clone() for k, v in tr.flatD.grad_views().items()}
    gG = {k: v.detach().cpu().clone() for k, v in tr.flatG.grad_views().items()}
    return out, gD, gG


def dead_bias_keys(net):
    """biases of the convolutions that feed an InstanceNorm directly: their gradient is zero in exact arithmetic, rounding noise in
    any float format -- compared on the scale of their layer's weight gradient instead of their own"""
    names = [k for k, _ in net.named_modules()]
    mods = dict(net.named_modules())
    dead = set()
    for a, b in zip(names, names[1:]):
        if isinstance(mods[a], (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and isinstance(mods[b], torch.nn.InstanceNorm2d):
            dead.add(a + ".bias")
    return dead


def grads_close(what, got, ref, dead, tol, l2):
    assert set(got) >= set(ref), set(ref) - set(got)
    for k, r in ref.items():
        g, r = got[k].double().reshape(-1), r.double().reshape(-1)
        assert torch.isfinite(g).all(), f"{what} {k}"
        scale = ref[k[:-4] + "weight"].double().reshape(-1) if k in dead else r
        if l2:
            err, den = (g - r).norm().item(), scale.norm().item()
        else:
            err, den = (g - r).abs().max().item(), scale.abs().max().item()
        assert err <= tol * max(den, 1e-30), f"{what} {k}: {err / max(den, 1e-30):.3e} > {tol:.0e}"


class _Block(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        nn = torch.nn
        self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c), nn.ReLU(True),
                                        nn.ReflectionPad2d(1), nn.Conv2d(c, c, 3), nn.InstanceNorm2d(c))

    def forward(self, x):
        return x + self.conv_block(x)


class _Seq(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.model = torch.nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def stock_patchgan(ndf=8):
    """the 70 x 70 PatchGAN with instance norm as stock torch.nn (fp32 as built; the reference's state_dict keys)"""
    nn = torch.nn
    d = [nn.Conv2d(4, ndf, 4, stride=2, padding=1), nn.LeakyReLU(0.2, True)]
    for cin, cout, s in ((ndf, 2 * ndf, 2), (2 * ndf, 4 * ndf, 2), (4 * ndf, 8 * ndf, 1)):
        d += [nn.Conv2d(cin, cout, 4, stride=s, padding=1), nn.InstanceNorm2d(cout), nn.LeakyReLU(0.2, True)]
    d += [nn.Conv2d(8 * ndf, 1, 4, stride=1, padding=1)]
    return _Seq(d)


def stock_nets(m, ngf=8, n_blocks=6):
    """float64 torch.nn restatement of the two networks (the published pix2pix ResNet generator and 70 x 70 PatchGAN with instance
    norm), built here and filled from the model's state dict"""
    nn = torch.nn
    g = [nn.ReflectionPad2d(3), nn.Conv2d(3, ngf, 7), nn.InstanceNorm2d(ngf), nn.ReLU(True)]
    for i in range(2):
        c = ngf * 2 ** i
        g += [nn.Conv2d(c, 2 * c, 3, stride=2, padding=1), nn.InstanceNorm2d(2 * c), nn.ReLU(True)]
    g += [_Block(4 * ngf) for _ in range(n_blocks)]
    for i in range(2):
        c = ngf * 2 ** (2 - i)
        g += [nn.ConvTranspose2d(c, c // 2, 3, stride=2, padding=1, output_padding=1), nn.InstanceNorm2d(c // 2), nn.ReLU(True)]
    g += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, 1, 7), nn.Tanh()]
    G, D = _Seq(g).double(), stock_patchgan(ngf).double()
    G.load_state_dict({k: v.detach().cpu().double() for k, v in m.netG.state_dict().items()})
    D.load_state_dict({k: v.detach().cpu().double() for k, v in m.netD.state_dict().items()})
    return G, D


def stock_step(G, D, mode, batch, lambda_gan=1.0, lambda_l1=100.0, lr=2e-4, beta1=0.5):
    """the two optimizer passes of one batch in float64: (losses, gradients of D, gradients of G against the stepped D)"""
    rgb, nir = batch["rgb"].cpu().double(), batch["nir"].cpu().double()
    pred = G(rgb)
    loss_d = objective(mode, D(torch.cat((rgb, pred.detach()), 1)), 0.0) + objective(mode, D(torch.cat((rgb, nir), 1)), 1.0)
    opt = torch.optim.Adam(D.parameters(), lr=lr, betas=(beta1, 0.999))
    opt.zero_grad()
    loss_d.backward()
    gD = {k: p.grad.clone() for k, p in D.named_parameters()}
    opt.step()
    gan = objective(mode, D(torch.cat((rgb, pred), 1)), 1.0)
    loss_g = lambda_gan * gan + lambda_l1 * (pred - nir).abs().mean()
    G.zero_grad()
    loss_g.backward()
    gG = {k: p.grad.clone() for k, p in G.named_parameters()}
    return {"loss_D": loss_d.item(), "loss_G": loss_g.item(), "loss_G_gan": gan.item()}, gD, gG


def fused_against_autograd(dev, golden_dir, mode):
    """train_batch against training_step(.., 0) -> backward -> Adam(D) -> training_step(.., 1) -> backward of the same build"""
    batch = batch64(dev)
    out, gD, gG = fused_step(make_model(dev, mode, golden_dir=golden_dir), batch)
    m = make_model(dev, mode, golden_dir=golden_dir)
    (opt_d, opt_g), _ = m.configure_optimizers()
    loss_d = m.training_step(batch, 0, 0)
    opt_d.zero_grad()
    loss_d.backward()
    refD = {k: p.grad.detach().cpu().clone() for k, p in m.netD.named_parameters()}
    opt_d.step()
    for p in m.netD.parameters():
        p.requires_grad_(False)
    loss_g = m.training_step(batch, 0, 1)
    opt_g.zero_grad()
    loss_g.backward()
    refG = {k: p.grad.detach().cpu().clone() for k, p in m.netG.named_parameters()}
    want = {"loss_D": float(loss_d.detach()), "loss_G": float(loss_g.detach()), "loss_G_gan": float(m.logged["model_loss/generator_GAN_loss"])}
    for k, v in want.items():
        print(f"GANLOSS fused {mode} {k} {out[k]!r} autograd {v!r}")
        assert abs(out[k] - v) <= FUSED_TOL * abs(v), f"{mode} {k}: {out[k]} against {v}"
    G64, D64 = stock_nets(m)
    grads_close(f"{mode} gD", gD, refD, dead_bias_keys(D64), FUSED_TOL, l2=False)
    grads_close(f"{mode} gG", gG, refG, dead_bias_keys(G64), FUSED_TOL, l2=False)


def fused_against_float64(dev, golden_dir, mode):
    """train_batch against the same step on the stock-torch float64 restatement"""
    batch = batch64(dev)
    m = make_model(dev, mode, golden_dir=golden_dir)
    G64, D64 = stock_nets(m)
    out, gD, gG = fused_step(m, batch)
    want, refD, refG = stock_step(G64, D64, mode, batch)
    for k, v in want.items():
        print(f"GANLOSS fused {mode} {k} {out[k]!r} float64 {v!r}")
        assert abs(out[k] - v) <= PARITY * abs(v), f"{mode} {k}: {out[k]} against {v}"
    grads_close(f"{mode} gD", gD, refD, dead_bias_keys(D64), PARITY, l2=True)
    grads_close(f"{mode} gG", gG, refG, dead_bias_keys(G64), PARITY, l2=True)


def fused_step_runs_and_repeats(dev, mode, ngf=64):
    """full-width nets: finite losses, both networks stepped, and the same step from the same weights gives the same bits"""
    batch = batch64(dev)
    runs = []
    for _ in range(2):
        m = make_model(dev, mode, ngf=ngf, seed=7)
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        out = m.train_batch(batch).as_dict()
        assert all(np.isfinite(v) for v in out.values()), out
        after = {k: v.detach().clone() for k, v in m.state_dict().items()}
        for net in ("netG.", "netD."):
            assert any(not torch.equal(before[k], after[k]) for k in after if k.startswith(net)), net + " did not step"
        runs.append((out, after))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(torch.equal(bits(runs[0][1][k]), bits(runs[1][1][k])) for k in runs[0][1])
    print(f"GANLOSS fused {mode} full width {runs[0][0]}")
