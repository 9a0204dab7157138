"""Bodies of the tests of the pixel discriminator (netD 'pixel': csrc/pixdisc.hip, nets.PixelDiscriminatorEngine,
networks.PixelDiscriminator, the fused trainer), shared by the CPU suite (the numpy statement tests/emu_pixel_disc.py:
tests/test_pixel_disc_emulated.py) and the MI355X suite (the HIP library: tests/test_gpu_pixel_disc.py).  Every body takes ``dev``.

Reference: stock torch.nn in float64 on the CPU,
    Sequential(Conv2d(4,64,1), LeakyReLU(0.2), Conv2d(64,128,1), InstanceNorm2d(128), LeakyReLU(0.2), Conv2d(128,1,1))
under the attribute ``net`` (the reference's state_dict keys), filled with ``load_state_dict(strict=True)``.  The same module in fp32 on
the CPU gives the stock-fp32 error e32 of every quantity on the same inputs.

Bounds: min(1e-3, max(floor, 10 e32)); floor 2e-6 for ``out`` (max-norm relative), 1e-5 for gradients (relative L2 per tensor;
net.5.bias |got - ref| / |ref|).  Ten covers another summation order (MFMA K order, record merges) on a maximum over few samples; 1e-3
is the project's parity bound.  Every case asserts e32 <= 1e-4 (otherwise the seed is wrong) and prints every figure before it asserts.

Inputs are built in float64 with the LeakyReLU kinks controlled (delta = 1e-5), else one decision on a |z1| ~ 1e-8 element puts stock
fp32 itself at 1e-3:  (1) the four input values of every pixel with a z1 element within delta max|z1| of zero are drawn again until none
is left;  (2) dout is zero at every pixel with an xh element within delta max|xh| of zero.  Each set is at most 2 % of the pixels.
"""
import functools

import numpy as np
import torch

from nirgan_hip import lib as L

SHAPES = [(1, 1, 2), (1, 5, 5), (2, 7, 9), (40, 3, 3), (3, 67, 93), (2, 64, 64), (1, 128, 160)]
SMALL = SHAPES[:4]
LARGE_MEAN_SHAPES = [(1, 5, 5), (3, 67, 93), (2, 64, 64)]
GUARD_SHAPES = [(1, 1, 2), (1, 1, 33), (3, 11, 31), (5, 5, 41), (40, 3, 3)]
BIG = (8, 256, 256)
DELTA, SEED = 1e-5, 4          # seeds 3 and 5 put stock fp32 itself past 1e-4 on (1, 1, 2) or leave a kink set above 2 %
FLOOR_OUT, FLOOR_GRAD, PARITY, STOCK_MAX = 2e-6, 1e-5, 1e-3, 1e-4
KEYS = ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.5.weight", "net.5.bias"]
SENT = -7.25e11


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Stock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.net = nn.Sequential(nn.Conv2d(4, 64, 1), nn.LeakyReLU(0.2), nn.Conv2d(64, 128, 1), nn.InstanceNorm2d(128), nn.LeakyReLU(0.2),
                                 nn.Conv2d(128, 1, 1))

    def forward(self, x):
        return self.net(x)


def define_pixel():
    from model import networks
    return networks.define_D(4, 64, "pixel", norm="instance", init_type="normal", init_gain=0.02)


@functools.lru_cache(maxsize=None)
def weights(wset):
    """state dict (fp32) of weight set 1 (init_net as it comes), 2 (trained-like) or 3 (2 with net.0.bias = 4: large means)"""
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in define_pixel().state_dict().items()}
    assert list(sd) == KEYS
    if wset >= 2:
        g = torch.Generator().manual_seed(11)
        for k in KEYS:
            sd[k] = (0.3 if k.endswith("weight") else 0.1) * torch.randn(sd[k].shape, generator=g)
    if wset == 3:
        sd["net.0.bias"] = torch.full((64,), 4.0)
    return sd


def stock(wset, dtype):
    m = Stock().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in weights(wset).items()}, strict=True)
    return m


def ours(wset, dev):
    m = define_pixel()
    m.load_state_dict(weights(wset), strict=True)
    return m.to(dev)


def rel_max(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def rel_l2(got, ref):
    return (got.double().cpu() - ref).norm().item() / max(ref.norm().item(), 1e-300)


def bound(e32, floor):
    return min(PARITY, max(floor, 10.0 * e32))


def run_stock(m, x, dout):
    """(out, parameter gradients, gx) of sum(dout * m(x)) on stock torch, in the dtype of m"""
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    out = m(x)
    (out * dout).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, x.grad.detach().clone()


@functools.lru_cache(maxsize=None)
def case(shape, wset, gradients=True):
    """Inputs (float64, kinks controlled), the float64 results and the stock-fp32 errors of one (shape, weight set); computed once and
    shared, nobody writes to it."""
    B, H, W = shape
    g = torch.Generator().manual_seed(SEED * 1000 + B * 7 + H * 3 + W)
    m64 = stock(wset, torch.float64)
    x = torch.rand(B, 4, H, W, generator=g, dtype=torch.float64) * 2 - 1
    npix = B * H * W
    redrawn = torch.zeros(B, H, W, dtype=torch.bool)
    if gradients:
        for _ in range(50):
            with torch.no_grad():
                z1 = m64.net[0](x)
            near = (z1.abs() < DELTA * z1.abs().max()).any(1)
            if not near.any():
                break
            redrawn |= near
            fresh = torch.rand(B, 4, H, W, generator=g, dtype=torch.float64) * 2 - 1
            x = torch.where(near.unsqueeze(1), fresh, x)
        else:
            raise AssertionError("kink control of z1 did not converge")
    else:
        # the large-mean forward case: a narrow input range under net.0.bias = 4 puts |mean| / std of z2 near 1e2 in the median channel
        # and past 1e3 in the widest (narrower inputs put stock fp32 itself past 1e-4 on the larger shapes)
        x = 0.1 * x
        with torch.no_grad():
            z2 = m64.net[2](m64.net[1](m64.net[0](x)))
        ratio = z2.mean((2, 3)).abs() / z2.std((2, 3), unbiased=False)
        print(f"PIXD case {shape} w{wset} | |mean| / std of z2: median {ratio.median().item():.3e} max {ratio.max().item():.3e}")
        assert ratio.max().item() >= 2e2
    dout = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
    zeroed = torch.zeros(B, H, W, dtype=torch.bool)
    if gradients:
        with torch.no_grad():
            xh = m64.net[3](m64.net[2](m64.net[1](m64.net[0](x))))
        zeroed = (xh.abs() < DELTA * xh.abs().max()).any(1)
        dout = torch.where(zeroed.unsqueeze(1), torch.zeros_like(dout), dout)
    f1, f2 = redrawn.sum().item() / npix, zeroed.sum().item() / npix
    print(f"PIXD case {shape} w{wset} | pixels redrawn {f1:.4f} | dout zeroed {f2:.4f}")
    assert f1 <= 0.02 and f2 <= 0.02, (shape, wset, f1, f2)
    m32 = stock(wset, torch.float32)
    if gradients:
        out, gp, gx = run_stock(m64, x, dout)
        o32, gp32, gx32 = run_stock(m32, x.float(), dout.float())
    else:
        with torch.no_grad():
            out, o32 = m64(x), m32(x.float())
        gp, gx, gp32, gx32 = {}, None, {}, None
    e32 = {"out": rel_max(o32, out)}
    if gradients:
        e32["gx"] = rel_l2(gx32, gx)
        e32["gpred"] = rel_l2(gx32[:, 3], gx[:, 3])
        for k in KEYS:
            if k == "net.2.bias":
                continue
            e32[k] = rel_l2(gp32[k], gp[k])
    for k, v in e32.items():
        print(f"PIXD case {shape} w{wset} | stock fp32 {k} {v:.3e}")
        assert v <= STOCK_MAX, f"stock fp32 itself is off on {k}: {v:.3e} (choose another seed)"
    return {"x": x, "dout": dout, "out": out, "gp": gp, "gx": gx, "e32": e32}


def make_engine(wset, shape, dev):
    """(module, flat storage, engine) on the flat ranges of a fresh module with the weight set loaded"""
    from nirgan_hip.nets import PixelDiscriminatorEngine
    m = ours(wset, dev)
    flat = m._flat()
    eng = PixelDiscriminatorEngine(flat.param_views(), flat.grad_views(), *shape)
    return m, flat, eng


def check(tag, what, err, e32, floor):
    b = bound(e32, floor)
    print(f"PIXD {tag} | {what} err {err:.3e} | stock fp32 {e32:.3e} | bound {b:.3e}")
    assert np.isfinite(err) and err <= b, f"{tag} {what}: {err:.3e} > {b:.3e} (stock fp32 {e32:.3e})"


def compare(tag, c, out=None, grads=None, gx=None, gpred=None):
    e = c["e32"]
    if out is not None:
        assert out.shape == c["out"].shape
        check(tag, "out", rel_max(out, c["out"]), e["out"], FLOOR_OUT)
    if grads is not None:
        for k in KEYS:
            if k == "net.2.bias":
                assert (grads[k] == 0).all(), f"{tag}: net.2.bias feeds the InstanceNorm, its gradient is written as exact zeros"
            else:
                check(tag, k, rel_l2(grads[k], c["gp"][k]), e[k], FLOOR_GRAD)
    if gx is not None:
        check(tag, "gx", rel_l2(gx, c["gx"].permute(0, 2, 3, 1)), e["gx"], FLOOR_GRAD)
    if gpred is not None:
        check(tag, "gpred", rel_l2(gpred, c["gx"][:, 3]), e["gpred"], FLOOR_GRAD)


def engine_level(shape, wset, dev):
    """forward, PARAMS, INPUT and PRED of the engine against float64; flat padding zero; PRED is channel 3 of INPUT bitwise"""
    c = case(shape, wset)
    tag = f"{shape} w{wset}"
    m, flat, eng = make_engine(wset, shape, dev)
    flat.grad.fill_(SENT)
    out = eng.forward(c["x"].float().to(dev)).clone()
    eng.backward(c["dout"].float().to(dev), frozen=False)
    grads = {k: v.detach().cpu().clone() for k, v in flat.grad_views().items()}
    gx = eng.backward(None, frozen=True).detach().cpu().clone()
    gpred = eng.backward(None, frozen=True, pred_only=True).detach().cpu().clone()
    sync(dev)
    compare(tag, c, out=out, grads=grads, gx=gx, gpred=gpred)
    full = flat.grad.detach().cpu()
    assert full.numel() == 8772 and (full[8769:] == 0).all(), "padding elements of the flat gradient are zero"
    assert torch.equal(bits(gpred), bits(gx[..., 3])), "PRED is channel 3 of INPUT, bitwise"
    return m, flat, eng


def large_mean_forward(shape, dev):
    """weight set 3: |mean| / std of z2 is 2e2 .. 1e4; a plain fp32 sum / sum of squares is 1.4e-4 .. 0.14 off here"""
    c = case(shape, 3, gradients=False)
    m, flat, eng = make_engine(3, shape, dev)
    out = eng.forward(c["x"].float().to(dev)).clone()
    sync(dev)
    compare(f"{shape} w3 large mean", c, out=out)


def autograd_route(shape, wset, dev):
    """the module itself: D(x) with autograd through DiscriminatorFn, parameters and input"""
    c = case(shape, wset)
    m = ours(wset, dev)
    x = c["x"].float().to(dev).requires_grad_(True)
    out = m(x)
    (out * c["dout"].float().to(dev)).sum().backward()
    sync(dev)
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    compare(f"{shape} w{wset} autograd", c, out=out.detach(), grads=grads, gx=x.grad.detach().permute(0, 2, 3, 1))


def state_dict_and_seed(golden):
    """keys, shapes and seeded weights: the fixture's (the reference's define_D under manual_seed(0)) and stock torch.nn's"""
    torch.manual_seed(0)
    m = define_pixel()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert list(sd) == KEYS
    for k in KEYS:
        want = torch.from_numpy(golden["sd/" + k])
        assert sd[k].shape == want.shape and torch.equal(sd[k], want), k
    torch.manual_seed(0)
    r = Stock()
    for mod in r.net:
        if isinstance(mod, torch.nn.Conv2d):
            torch.nn.init.normal_(mod.weight.data, 0.0, 0.02)
            torch.nn.init.constant_(mod.bias.data, 0.0)
    for k, v in r.state_dict().items():
        assert torch.equal(sd[k], v), k
    r.load_state_dict(sd, strict=True)
    m.load_state_dict({k: v + 1 for k, v in r.state_dict().items()}, strict=True)
    assert all(torch.equal(m.state_dict()[k], sd[k] + 1) for k in KEYS)


def golden_forward(golden, dev):
    """the fixture's fp32 output on its 2 x 4 x 8 x 8 input"""
    m = define_pixel()
    m.load_state_dict({k: torch.from_numpy(golden["sd/" + k]) for k in KEYS}, strict=True)
    m = m.to(dev)
    with torch.no_grad():
        out = m(torch.from_numpy(golden["x"]).to(dev))
    want = torch.from_numpy(golden["out"]).double()
    err = rel_max(out, want)
    print(f"PIXD golden forward err {err:.3e}")
    assert out.shape == want.shape and err <= 1e-5        # two fp32 evaluations of one function: ten times FLOOR_OUT apart at most


# ------------------------------------------------------------------------------------------------ Px2Px_PL
def make_model(dev, mode="lsgan", ngf=8, seed=0):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, ngf)
    cfg.base_configs.netD, cfg.base_configs.ndf, cfg.base_configs.gan_mode = "pixel", 64, mode
    torch.manual_seed(seed)
    m = Px2Px_PL(cfg)
    assert type(m.netD).__name__ == "PixelDiscriminator"
    return m.to(dev).train()


def batch(dev, B=2, size=32, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"rgb": (0.02 + 0.58 * torch.rand(B, 3, size, size, generator=g)).to(dev),
            "nir": (0.05 + 0.75 * torch.rand(B, 1, size, size, generator=g)).to(dev)}


def lightning_step(m, opts, b, i):
    opt_d, opt_g = opts
    loss_d = m.training_step(b, i, 0)
    opt_d.zero_grad()
    loss_d.backward()
    opt_d.step()
    for p in m.netD.parameters():
        p.requires_grad_(False)
    loss_g = m.training_step(b, i, 1)
    opt_g.zero_grad()
    loss_g.backward()
    opt_g.step()
    for p in m.netD.parameters():
        p.requires_grad_(True)
    return float(loss_d.detach()), float(loss_g.detach())


def routes_agree(dev, steps=5):
    """five steps of the Lightning sequence and of train_batch from the same weights: every parameter within 1e-6 relative"""
    b = batch(dev)
    m1, m2 = make_model(dev), make_model(dev)
    (opt_d, opt_g), _ = m1.configure_optimizers()
    for i in range(steps):
        ld, lg = lightning_step(m1, (opt_d, opt_g), b, i)
        out = m2.train_batch(b).as_dict()
        assert all(np.isfinite(v) for v in out.values()), out
    print(f"PIXD routes: lightning loss_D {ld!r} loss_G {lg!r} | fused {out['loss_D']!r} {out['loss_G']!r}")
    tr = m2.fused_trainer()
    assert tr.steps == steps and tr.flatD.step_count == steps and type(tr.D2).__name__ == "PixelDiscriminatorEngine"
    worst = 0.0
    for (k, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
        a, c = a.detach().cpu().double(), c.detach().cpu().double()
        err = (a - c).abs().max().item() / max(a.abs().max().item(), 1e-30)
        worst = max(worst, err)
        assert err <= 1e-6, f"routes differ on {k}: {err:.3e}"
    print(f"PIXD routes agree after {steps} steps: worst {worst:.3e}")


def objective(mode, x, t):
    if mode == "lsgan":
        return ((x - t) ** 2).mean()
    if mode == "vanilla":
        return torch.nn.BCEWithLogitsLoss()(x, torch.full_like(x, t))
    return -x.mean() if t > 0.5 else x.mean()


def fused_losses_against_float64(dev, mode):
    """loss_D_fake / loss_D_real of one fused step against float64 D(cat(rgb, pred)) with D's parameters from before the step,
    loss_G_gan with those after it"""
    b = batch(dev)
    m = make_model(dev, mode)
    before = {k: v.detach().cpu().double().clone() for k, v in m.netD.state_dict().items()}
    out = m.train_batch(b).as_dict()
    tr = m.fused_trainer()
    pred = tr.pred.detach().cpu().double()
    after = {k: v.detach().cpu().double().clone() for k, v in m.netD.state_dict().items()}
    rgb, nir = b["rgb"].cpu().double(), b["nir"].cpu().double()
    D = Stock().double()
    with torch.no_grad():
        D.load_state_dict(before, strict=True)
        want = {"loss_D_fake": objective(mode, D(torch.cat((rgb, pred), 1)), 0.0).item(),
                "loss_D_real": objective(mode, D(torch.cat((rgb, nir), 1)), 1.0).item()}
        D.load_state_dict(after, strict=True)
        want["loss_G_gan"] = objective(mode, D(torch.cat((rgb, pred), 1)), 1.0).item()
    assert any(not torch.equal(before[k], after[k]) for k in before), "D did not step"
    for k, v in want.items():
        err = abs(out[k] - v) / abs(v)
        print(f"PIXD fused {mode} {k} {out[k]!r} float64 {v!r} err {err:.3e}")
        assert err <= PARITY, f"{mode} {k}: {out[k]} against {v}"


def fit_checkpoint_resume(dev, tmp_path):
    from nirgan_hip.fit import fit
    import api_cases as A
    train, val = A._loaders(dev)
    m = make_model(dev)
    ck = tmp_path / "p.ckpt"
    hist = fit(m, train, val, max_epochs=1, log_every=1, ckpt_path=str(ck), device=dev)
    assert len(hist["train"]) == 2 and len(hist["val"]) == 1 and "val/L1" in hist["val"][0]
    assert all(np.isfinite(r["loss_D"]) and np.isfinite(r["loss_G"]) for r in hist["train"]), hist["train"]
    c = torch.load(str(ck), weights_only=False)
    assert "netD.net.0.weight" in c["state_dict"] and "netD.net.5.bias" in c["state_dict"] and c["global_step"] == 2
    Stock().load_state_dict({k[5:]: v for k, v in c["state_dict"].items() if k.startswith("netD.")}, strict=True)
    # an uninterrupted second epoch == resume for one more epoch
    fit(m, train, val, max_epochs=1, log_every=0, device=dev)
    m2 = make_model(dev, seed=9)
    h2 = fit(m2, train, val, max_epochs=2, log_every=0, resume_from=str(ck), device=dev)
    assert len(h2["val"]) == 1 and m2.fused_trainer().flatD.step_count == 4
    for (k, a), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a.detach().cpu(), q.detach().cpu()), "resumed " + k


# ------------------------------------------------------------------------------------------------ the entries on raw buffers
def raw_run(shape, wset, dev, c, guard=0, nan_ws=False):
    """fwd and the three bwd modes through the C ABI on buffers of the caller's making: every output is carved out of a larger buffer
    filled with SENT (``guard`` floats on each side, a multiple of 4 so that gx stays 16-byte aligned), the workspace is NaN on entry.
    Returns the outputs (clones) after checking the guards."""
    import ctypes as C
    B, H, W = shape
    n = B * H * W
    m = ours(wset, dev)
    flat = m._flat()
    x = c["x"].float().permute(0, 2, 3, 1).contiguous().to(dev)
    dout = c["dout"].float().reshape(-1).contiguous().to(dev)
    nws = int(L.backend().nirgan_pixdisc_ws_elems(B, H, W, 64))
    assert nws > 0
    ws = torch.full((nws,), float("nan") if nan_ws else 0.0, device=dev)
    sizes = {"out": n, "stats": B * 256, "grads": 8772, "gx": 4 * n, "gpred": n}
    bufs = {k: torch.full((v + 2 * guard,), SENT, device=dev) for k, v in sizes.items()}

    def ptr(k):
        return bufs[k].data_ptr() + 4 * guard
    d = L.PixDiscDesc()
    d.x, d.B, d.H, d.W, d.ndf, d.params = x.data_ptr(), B, H, W, 64, flat.flat.data_ptr()
    d.stats, d.out, d.dout, d.ws, d.ws_elems = ptr("stats"), ptr("out"), dout.data_ptr(), ws.data_ptr(), nws
    st = torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else None
    L.call("nirgan_pixdisc_fwd", C.byref(d), st)
    for mode, key in ((L.PIXDISC_PARAMS, "grads"), (L.PIXDISC_INPUT, "gx"), (L.PIXDISC_PRED, "gpred")):
        if nan_ws:
            ws.fill_(float("nan"))
        d.mode = mode
        d.grads = ptr("grads") if mode == L.PIXDISC_PARAMS else None
        d.gx = None if mode == L.PIXDISC_PARAMS else ptr(key)
        L.call("nirgan_pixdisc_bwd", C.byref(d), st)
    sync(dev)
    res = {}
    for k, v in sizes.items():
        b = bufs[k].cpu()
        if guard:
            assert (b[:guard] == SENT).all() and (b[guard + v:] == SENT).all(), f"{shape}: a write next to {k}"
        body = b[guard:guard + v].clone()
        assert torch.isfinite(body).all() and (body != SENT).all(), f"{shape}: {k} not fully written"
        res[k] = body
    return res, flat


def raw_compare(tag, shape, c, res, flat):
    B, H, W = shape
    grads = {k: res["grads"][o:o + cnt].view(shp) for k, (o, cnt, shp) in flat.slices.items()}
    compare(tag, c, out=res["out"].view(B, 1, H, W), grads=grads, gx=res["gx"].view(B, H, W, 4), gpred=res["gpred"].view(B, H, W))
    assert (res["grads"][8769:] == 0).all()
    assert torch.equal(bits(res["gpred"]), bits(res["gx"].view(-1, 4)[:, 3])), "PRED is channel 3 of INPUT, bitwise"


def guarded(shape, dev):
    c = case(shape, 2)
    res, flat = raw_run(shape, 2, dev, c, guard=64, nan_ws=True)
    raw_compare(f"{shape} w2 guarded", shape, c, res, flat)


def two_runs_bitwise(shape, dev, c=None):
    c = c if c is not None else case(shape, 2)
    a, _ = raw_run(shape, 2, dev, c)
    b, _ = raw_run(shape, 2, dev, c, nan_ws=True)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{shape}: two runs differ in {k}"
    return a


def zero_dout(shape, dev):
    c = dict(case(shape, 2))
    c["dout"] = torch.zeros_like(c["dout"])
    res, _ = raw_run(shape, 2, dev, c, nan_ws=True)
    for k in ("grads", "gx", "gpred"):
        assert (res[k] == 0).all(), f"{shape}: dout = 0 leaves nonzero {k}"


def doubled_batch(shape, dev):
    """[fake ; real] as one batch of 2B against two forwards of B: the same out per sample, bitwise"""
    B, H, W = shape
    ca, cb = case(shape, 2), case(shape, 1)                    # two different inputs of the same shape
    m, flat, e2 = make_engine(2, (2 * B, H, W), dev)
    from nirgan_hip.nets import PixelDiscriminatorEngine
    e1 = PixelDiscriminatorEngine(flat.param_views(), flat.grad_views(), B, H, W)
    xa, xb = ca["x"].float().to(dev), cb["x"].float().to(dev)
    both = e2.forward(torch.cat((xa, xb), 0)).clone()
    oa = e1.forward(xa).clone()
    ob = e1.forward(xb).clone()
    sync(dev)
    assert torch.equal(bits(both[:B]), bits(oa)) and torch.equal(bits(both[B:]), bits(ob))


def thirty_steps_twice(dev):
    b = batch(dev, B=2, size=64)
    runs = []
    for _ in range(2):
        m = make_model(dev, ngf=16, seed=7)
        hist = [m.train_batch(b).as_dict() for _ in range(30)]
        assert all(np.isfinite(h["loss_D"]) and np.isfinite(h["loss_G"]) for h in hist), hist
        runs.append((hist, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    print(f"PIXD thirty steps: first {runs[0][0][0]} last {runs[0][0][-1]}")
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(torch.equal(bits(runs[0][1][k]), bits(runs[1][1][k])) for k in runs[0][1])
