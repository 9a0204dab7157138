"""The fused train step (``Px2Px_PL.train_batch`` -> ``Pix2PixTrainer.step``) replayed over a pairwise matrix of its options, shared by
the CPU suite (C ABI served by the numpy emulators: tests/test_step_matrix_emulated.py) and the MI355X suite (the HIP library:
tests/test_gpu_step_matrix.py).  Every body takes ``dev`` and a ``Bounds``.

The kernels underneath are pinned launch by launch elsewhere; what these rows pin is the wiring between them when two or more options
are selected together: descriptor fields, buffer sharing, gradient accumulation into ``dpred``, loss slots, per-part scaling, mask
indexing, packed-weight versions and the shape-state cache.

Reference: ONE float64 step on the CPU composed of the pieces the other suites already use -- ``dropout_cases.forward64`` (generator:
plain, injection, post correction, dropout masks) between ``F.pad(mode="reflect")`` and the crop, ``gan_loss_cases.stock_patchgan`` /
``pixel_disc_cases.Stock`` (discriminators), ``gan_loss_cases.objective`` and ``O.lsgan_loss`` (objectives), ``O.l1_loss``,
``O.rs_weighted_loss``, ``O.ssim_map`` (``O.ssim_loss`` is ``1 - ssim_map(.., 11).mean()`` behind a cast to fp32: the body without the
cast) and ``O.adam_step``.  The reference always sees the whole batch, with the dropout masks of ``nirgan_hip.dropout.mask`` at the
``(seed, call)`` the step used and the extent of the padded trunk, ``(H + 2 pad) / 4``.

Bounds are the project's own: see ``GPU8``, ``GPU32`` and ``EMU`` below.  The same step evaluated by stock torch in fp32 on the CPU has
to lie within HALF of the MI355X bounds on every asserted quantity (``reference_alone``); a row that does not gets another data seed.
A seed in the table differs from 1 for that reason, or with the evidence written next to the table that one ReLU decision within
rounding of zero explains a miss.
"""
import collections
import itertools

AXES = collections.OrderedDict([
    ("disc", ("basic", "pixel")),                               # basic: ndf = ngf; pixel: ndf 64
    ("gan", ("lsgan", "vanilla", "wgangp")),
    ("gen", ("g6", "g9", "inject", "inject_pc")),               # inject: 9 blocks, 'multiply', scale parameter; _pc: + post_correction
    ("drop", (0, 1)),
    ("pad", (0, 10)),
    ("rs", ("off", "l1", "l2")),                                # lambda_rs = 1 with the criterion; NDVI / NDWI / EVI weights
    ("ssim", (0.0, 0.5)),
    ("micro", (1, 2)),
    ("shape", ((2, 32, 32), (4, 32, 32), (3, 36, 40), (1, 40, 40))),
])
Row = collections.namedtuple("Row", "id disc gan gen drop pad rs ssim micro shape ngf seed lr")

# Generated greedily over the allowed pairs, then frozen: a row's id is stable.  seed = the data seed, lr = the learning rate at which a
# stale second step is distinguishable (stale_is_distinguishable); 2e-4 is the configs' own and reaches that on every row.
# Seeds other than 1, each the first that passes after the ones named:
#   m00 3   reference_alone: seeds 1, 2 put stock fp32 at 0.87 / 2.2 of the 2e-3 on gD net.5.bias (vanilla at sigmoid ~ 0.5: the fake and
#           the real half of the last bias's gradient cancel)
#   m03 3, m06 4, m10 3, w01 7   reference_alone: stock fp32 itself misses the gradient bound on the earlier seeds, every generator
#           tensor upstream of one layer by the same 2e-3 .. 1.5e-2 and the tensors behind it at 1e-6: one ReLU within rounding of zero
#   m07 3   seed 1 as above (stock fp32, step one).  Seed 2 passed reference_alone and the emulator and missed on the MI355X in (c), the
#           step back at the first shape: gG model.14.conv_block.1.weight 2.8e-2, everything upstream 1.2e-2, everything behind and pred
#           within 3e-6.  Of the 190 080 generator ReLU decisions of that step's float64 reference six lie within 3e-5 of zero; with ONE of
#           them taken the other way (the ReLU behind model.14.conv_block.1's norm, element (0, 17, 5, 8), |z| = 1.3e-6) the device's worst
#           generator tensor is 2.5e-6 from the reference.
#   w00 2   seed 1 passed reference_alone and missed EMU's 1e-4 in (a) on the emulator, every generator tensor upstream of model.19 at
#           5.5e-4 (the MI355X gives the same 5.467e-4, inside its 1e-2).  Of 2 145 024 decisions 51 lie within 3e-5 of zero; with the one
#           behind model.19's norm, element (0, 28, 39, 71), |z| = 1.35e-6, taken the other way the worst tensor is 2.9e-6 (emulator) and
#           1.0e-5 (MI355X) from the reference.
ROWS = [
    Row("m00", "pixel", "vanilla", "g9", 1, 10, "l1", 0.5, 2, (4, 32, 32), 8, 3, 2e-4),
    Row("m01", "basic", "lsgan", "inject_pc", 0, 0, "l1", 0.0, 1, (1, 40, 40), 8, 1, 2e-4),
    Row("m02", "basic", "wgangp", "g6", 1, 0, "off", 0.5, 2, (2, 32, 32), 8, 1, 2e-4),
    Row("m03", "pixel", "wgangp", "g9", 0, 10, "l2", 0.0, 1, (3, 36, 40), 8, 3, 2e-4),
    Row("m04", "basic", "vanilla", "inject", 1, 0, "l2", 0.0, 1, (4, 32, 32), 8, 1, 2e-4),
    Row("m05", "pixel", "lsgan", "inject", 0, 10, "off", 0.5, 2, (1, 40, 40), 8, 1, 2e-4),
    Row("m06", "pixel", "vanilla", "inject_pc", 0, 10, "l2", 0.5, 2, (2, 32, 32), 8, 4, 2e-4),
    Row("m07", "basic", "lsgan", "g9", 1, 0, "off", 0.0, 2, (3, 36, 40), 8, 3, 2e-4),
    Row("m08", "basic", "lsgan", "g6", 0, 10, "off", 0.5, 1, (4, 32, 32), 8, 1, 2e-4),
    Row("m09", "pixel", "vanilla", "g6", 0, 0, "l1", 0.5, 2, (3, 36, 40), 8, 1, 2e-4),
    Row("m10", "basic", "wgangp", "inject", 1, 10, "l1", 0.0, 1, (2, 32, 32), 8, 3, 2e-4),
    Row("m11", "pixel", "wgangp", "g6", 1, 0, "l2", 0.0, 1, (1, 40, 40), 8, 1, 2e-4),
    Row("m12", "pixel", "wgangp", "inject_pc", 1, 0, "off", 0.5, 1, (4, 32, 32), 8, 1, 2e-4),
    Row("m13", "pixel", "vanilla", "g9", 0, 0, "off", 0.5, 1, (1, 40, 40), 8, 1, 2e-4),
    Row("m14", "basic", "lsgan", "g9", 0, 10, "l2", 0.5, 2, (2, 32, 32), 8, 1, 2e-4),
]
# ngf = ndf = 32 (the pixel discriminator keeps its 64) at 2 x 64 x 64: the trunk on the Winograd and split-tile routes
WIDE = [
    Row("w00", "pixel", "vanilla", "g6", 1, 10, "off", 0.0, 1, (2, 64, 64), 32, 2, 2e-4),
    Row("w01", "basic", "wgangp", "g6", 0, 0, "off", 0.5, 2, (2, 64, 64), 32, 7, 2e-4),
]
# (c): the shape switch -- row id -> the other batch shape of the table; both discriminators, the dropout key bit on and off
SWITCH = {"m00": (1, 40, 40), "m07": (2, 32, 32), "m08": (3, 36, 40)}
BY_ID = {r.id: r for r in ROWS + WIDE}
CONSTRAINTS = ("injection needs square tiles (shape (3, 36, 40) with inject / inject_pc)",
               "(H + 2 pad) % 4 == 0 and (W + 2 pad) % 4 == 0")


def allowed(cfg):
    """the product's constraints on a combination of levels (injection's 9 blocks and dropout's fp32 are levels / fixed here)"""
    _, H, W = cfg["shape"]
    if cfg["gen"].startswith("inject") and H != W:
        return False
    return (H + 2 * cfg["pad"]) % 4 == 0 and (W + 2 * cfg["pad"]) % 4 == 0


def _pairs(cfg):
    return {((a, cfg[a]), (b, cfg[b])) for a, b in itertools.combinations(AXES, 2)}


def missing_pairs(rows=None):
    """(pairs of levels of two axes that some allowed combination contains and no row of the table does, pairs no combination allows)"""
    rows = ROWS if rows is None else rows
    need, every = set(), set()
    for levels in itertools.product(*AXES.values()):
        cfg = dict(zip(AXES, levels))
        every |= _pairs(cfg)
        if allowed(cfg):
            need |= _pairs(cfg)
    have = set()
    for r in rows:
        cfg = {a: getattr(r, a) for a in AXES}
        assert all(cfg[a] in AXES[a] for a in AXES) and allowed(cfg), r
        have |= _pairs(cfg)
    return sorted(need - have, key=repr), sorted(every - need, key=repr)


# ------------------------------------------------------------------------------------------------ bounds
class Bounds:
    """out: pred (max error over the reference's max) and every loss (relative); l2 / mx: per gradient tensor, relative L2 and, where
    given, relative max; scalar: one-element tensors (scale_param, post_correction_param, a last bias), relative."""

    def __init__(self, name, out, l2, mx, scalar, definite=1e-4):
        self.name, self.out, self.l2, self.mx, self.scalar, self.definite = name, out, l2, mx, scalar, definite


GPU8 = Bounds("gpu ngf 8", 1e-3, 1e-3, None, 2e-3)       # gan_loss_cases.PARITY; 2e-3: test_gpu_nets._fused_step_against_oracle
# test_gpu_nets.test_medium_width_nets_take_the_winograd_paths (its comment: at this width a few activations within rounding of zero
# take the other branch in any fp32 evaluation).  definite: api_cases.adam_close holds an element to the reference's side of the Adam step
# when its reference gradient exceeds 1e-4 of the tensor's maximum -- which takes gradient errors far below that; where the gradient
# bound itself allows an element to be off by mx of the maximum, only an element beyond mx has a sign the bound guarantees.
GPU32 = Bounds("gpu ngf 32", 1e-3, 1e-2, 1e-1, 1e-2, definite=1e-1)
EMU = Bounds("emulator", 2e-5, 1e-4, 2e-4, 1e-4)         # api_cases.CPU_TOL
DROP_SEED = 0x1234ABCD5678


def gpu_bounds(row):
    return GPU8 if row.ngf == 8 else GPU32


# ------------------------------------------------------------------------------------------------ model, batch, masks
def n_blocks(row):
    return 6 if row.gen == "g6" else 9


def dead_keys(row):
    """(generator, discriminator) biases that feed an InstanceNorm directly: zero gradient in exact arithmetic"""
    import nirgan_oracle as O
    g = O.shadowed_bias_keys("G", n_blocks(row))
    if row.drop:
        g = {k.replace("conv_block.5", "conv_block.6") for k in g}
    return g, ({"net.2.bias"} if row.disc == "pixel" else O.shadowed_bias_keys("D"))


def config(row, **base):
    import api_cases as A
    inject = row.gen.startswith("inject")
    cfg = A.px_config(n_blocks(row), row.ngf, row.pad, 0.0 if row.rs == "off" else 1.0, inject, lambda_ssim=row.ssim)
    b = cfg.base_configs
    if row.disc == "pixel":
        b.netD, b.ndf = "pixel", 64
    b.gan_mode, b.no_dropout, b.lr = row.gan, not row.drop, row.lr
    if row.rs != "off":
        b.rs_losses_criterium = row.rs
    cfg.satclip.post_correction = row.gen == "inject_pc"
    for k, v in base.items():
        setattr(b, k, v)
    return cfg


def make_model(row, dev):
    """Px2Px_PL of the row from seeded weights (the same every time), in training mode on ``dev``, with the row's ``micro_batches``"""
    import torch
    from model.pix2pix import Px2Px_PL
    torch.manual_seed(5)
    m = Px2Px_PL(config(row))
    with torch.no_grad():
        if row.gen.startswith("inject"):       # (init_net's N(0, 0.02) on the projection keeps the modulation tiny: make it count)
            m.netG.fc.weight.mul_(4.0)
            m.netG.scale_param.fill_(0.5)
        if row.gen == "inject_pc":
            m.netG.post_correction_param.fill_(0.9)
        if row.rs != "off":                    # the indices are singular where pred + band ~ 0: pred in (0.5, 1), as fixture f1_g9_rs_pad
            dict(m.netG.named_parameters())[f"model.{17 + n_blocks(row)}.bias"].fill_(1.5)
    m = m.to(dev).train()
    m.fused_trainer().micro_batches = row.micro
    if row.drop:
        m.netG.set_dropout_state(seed=DROP_SEED, call=10)
    return m


def make_batch(row, dev, shape=None):
    import torch
    import dropout_cases as Dc
    B, H, W = shape or row.shape
    rgb, nir = Dc.synth(B, H, W, 100 * row.seed + B)
    batch = {"rgb": rgb.to(dev), "nir": nir.to(dev)}
    if row.gen.startswith("inject"):
        batch["coords"] = torch.randn(B, 256, generator=torch.Generator().manual_seed(row.seed + 50)).to(dev)
    return batch


def masks(row, call, dev, shape=None):
    """the blocks' {0, 2} masks of one call for the WHOLE batch (sample0 = 0), on the padded trunk's extent; None without dropout"""
    from nirgan_hip import dropout as HD
    if not row.drop:
        return None
    B, H, W = shape or row.shape
    return [HD.mask(DROP_SEED, call, j, B, (H + 2 * row.pad) // 4, (W + 2 * row.pad) // 4, 4 * row.ngf, device=dev).cpu()
            for j in range(n_blocks(row))]


def params_of(m):
    """({name: fp32 clone} of netG, of netD) on the CPU"""
    return ({k: v.detach().cpu().clone() for k, v in m.netG.named_parameters()},
            {k: v.detach().cpu().clone() for k, v in m.netD.named_parameters()})


def moments_of(flat):
    mm, vv = flat.moments()
    return {k: (mm[o:o + n].view(s).detach().cpu().clone(), vv[o:o + n].view(s).detach().cpu().clone()) for k, (o, n, s) in flat.slices.items()}


# ------------------------------------------------------------------------------------------------ the reference step
def stock_discriminator(row, params_D, dtype):
    import gan_loss_cases as Gc
    import pixel_disc_cases as Pc
    D = (Pc.Stock() if row.disc == "pixel" else Gc.stock_patchgan(row.ngf)).to(dtype)
    D.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in params_D.items()}, strict=True)
    return D


def gan_objective(mode, x, real):
    import gan_loss_cases as Gc
    import nirgan_oracle as O
    return O.lsgan_loss(x, real) if mode == "lsgan" else Gc.objective(mode, x, 1.0 if real else 0.0)


def reference_step(row, params_G, params_D, batch, masks_d, masks_g, dtype=None, moments=None, step=1, lr=None):
    """One batch in the reference's order -- D pass on pred.detach(), Adam(D), G pass against the stepped, frozen D, Adam(G) -- on stock
    torch on the CPU in ``dtype`` (float64).  masks_d / masks_g: the dropout masks of the two generator forwards (the same for
    train_batch, which runs one).  moments: ({name: (m, v)} of G, of D) and ``step`` for a step that is not the first.
    Returns pred, the loss keys of LossView.as_dict, gD, gG and both parameter sets after the step."""
    import torch
    import torch.nn.functional as F
    import api_cases as A
    import dropout_cases as Dc
    import nirgan_oracle as O
    dtype = dtype or torch.float64
    lr = row.lr if lr is None else lr
    nb, pad = n_blocks(row), row.pad
    pG = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params_G.items()}
    D = stock_discriminator(row, params_D, dtype)
    rgb, nir = batch["rgb"].detach().cpu().to(dtype), batch["nir"].detach().cpu().to(dtype)
    emb = batch["coords"].detach().cpu().to(dtype) if "coords" in batch else None
    mom = moments or ({}, {})

    def generator(mk):
        mk = [1.0] * nb if mk is None else [t.to(dtype) for t in mk]
        x = F.pad(rgb, (pad,) * 4, mode="reflect") if pad else rgb
        y = Dc.forward64(pG, x, nb, mk, emb, post_correction=row.gen == "inject_pc")
        return y[..., pad:-pad, pad:-pad] if pad else y

    def adam(named, grads, state):
        out = {}
        for k, p in named:
            mv = state.get(k)
            m_, v_ = (mv[0].to(dtype).clone(), mv[1].to(dtype).clone()) if mv is not None else (torch.zeros_like(p), torch.zeros_like(p))
            q = p.detach().clone()
            O.adam_step(q, grads[k], m_, v_, step, lr=lr, b1=0.5)
            out[k] = q
        return out
    # ---- optimizer 0
    pred_d = generator(masks_d)
    l_fake = gan_objective(row.gan, D(torch.cat((rgb, pred_d.detach()), 1)), False)
    l_real = gan_objective(row.gan, D(torch.cat((rgb, nir), 1)), True)
    namedD = list(D.named_parameters())
    gD = dict(zip([k for k, _ in namedD], torch.autograd.grad(l_fake + l_real, [p for _, p in namedD])))
    pD1 = adam(namedD, gD, mom[1])
    with torch.no_grad():
        for k, p in namedD:
            p.copy_(pD1[k])
    # ---- optimizer 1
    pred = pred_d if masks_g is masks_d else generator(masks_g)
    for p in D.parameters():
        p.requires_grad_(False)
    gan = gan_objective(row.gan, D(torch.cat((rgb, pred), 1)), True)
    l1 = O.l1_loss(pred, nir)
    losses = {"loss_D_fake": l_fake, "loss_D_real": l_real, "loss_D": l_fake + l_real, "loss_G_gan": gan, "loss_G_l1": l1}
    loss_g = gan * 1.0 + l1 * 100.0
    if row.rs != "off":
        losses["loss_G_rs"] = O.rs_weighted_loss(rgb, nir, pred, dict(A.RS_W), row.rs)
        loss_g = loss_g + losses["loss_G_rs"] * 1.0
    if row.ssim > 0.0:
        losses["loss_G_ssim"] = 1.0 - O.ssim_map(pred, nir, 11).mean()
        loss_g = loss_g + losses["loss_G_ssim"] * row.ssim
    losses["loss_G"] = loss_g
    gG = dict(zip(pG, torch.autograd.grad(loss_g, list(pG.values()))))
    pG1 = adam(list(pG.items()), gG, mom[0])
    return {"pred": pred.detach(), "losses": {k: float(v.detach()) for k, v in losses.items()}, "gD": gD, "gG": gG, "pG": pG1, "pD": pD1}


# ------------------------------------------------------------------------------------------------ one comparison
class Worst:
    """the largest error / bound seen per kind of quantity, printed per row and part"""

    def __init__(self):
        self.r = {}

    def see(self, kind, err, bound, what):
        ratio = err / bound
        if ratio >= self.r.get(kind, (-1.0, ""))[0]:
            self.r[kind] = (ratio, what)
        return ratio

    def line(self):
        return " | ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in self.r.items())

    def top(self):
        return max(v[0] for v in self.r.values())


def compare(tag, row, got, ref, bounds, worst, lr=None, params=True, pred=True, before=None):
    """every asserted quantity of one step: got / ref as reference_step returns them.  Collects everything, prints, then asserts.
    before: ((pG, pD) in front of the step, (moments of G, of D) or None for zeros, the step's number) for the replay of Adam."""
    import torch
    import api_cases as A
    fails = []

    def see(kind, err, bound, what):
        if not err <= bound:                                    # (a NaN fails)
            fails.append(f"{what}: {err:.3e} > {bound:.1e}")
        worst.see(kind, err, bound, what)
    if pred:
        p, r = got["pred"].double().cpu(), ref["pred"].double()
        assert p.shape == r.shape, (tag, p.shape, r.shape)
        see("pred", (p - r).abs().max().item() / r.abs().max().item(), bounds.out, "pred")
    assert set(got["losses"]) == set(ref["losses"]), (tag, sorted(got["losses"]), sorted(ref["losses"]))
    for k, v in ref["losses"].items():
        see("loss", abs(float(got["losses"][k]) - v) / abs(v), bounds.out, k)
    deadG, deadD = dead_keys(row)
    for name, dead in (("gG", deadG), ("gD", deadD)):
        assert set(got[name]) == set(ref[name]), (tag, name)
        for k, r in ref[name].items():
            g, r = got[name][k].double().cpu().reshape(-1), r.double().reshape(-1)
            # (a dead bias, or a bias whose gradient is exactly zero -- the last one under wgangp, +1/n and -1/n over as many patches --
            # has no scale of its own: its layer's weight gradient gives it)
            scale = ref[name][k[:-4] + "weight"].double().reshape(-1) if k in dead or not r.any() else r
            e2, em = (g - r).norm().item() / max(scale.norm().item(), 1e-300), (g - r).abs().max().item() / max(scale.abs().max().item(), 1e-300)
            if r.numel() == 1:
                see("scalar", e2, bounds.scalar, f"{name} {k}")
            else:
                see("grad", e2, bounds.l2, f"{name} {k}")
                if bounds.mx is not None:
                    see("gmax", em, bounds.mx, f"{name} {k} (max)")
    print(f"STEPMATRIX {row.id} {tag} [{bounds.name}] err/bound: {worst.line()}")
    assert not fails, f"{row.id} {tag}: " + "; ".join(fails[:8])
    if not params:
        return
    import nirgan_oracle as O
    lr = row.lr if lr is None else lr
    for name, pname, dead, net in (("gG", "pG", deadG, 0), ("gD", "pD", deadD, 1)):
        if pname not in got:
            continue
        for k, r in ref[pname].items():
            what = f"{row.id} {tag} {pname} {k}"
            p = got[pname][k].detach().cpu().float().reshape(-1)
            assert torch.isfinite(p).all(), what
            if before is not None:
                # the Adam step itself, exactly: O.adam_step in float64 on the device's OWN gradient and moments from the parameters in front
                # of the step.  fp32 against float64 of one p - lr' m / (sqrt(v) / c + eps): 1e-6 of max|p| (as test_gpu_nets does) for the
                # rounding of p, 1e-5 of a step for the step's own half a dozen operations.  Every tensor, the dead biases included.
                q = before[0][net][k].detach().cpu().double().clone()
                mv = before[1][net].get(k) if before[1] is not None else None
                m_, v_ = (mv[0].double().clone(), mv[1].double().clone()) if mv is not None else (torch.zeros_like(q), torch.zeros_like(q))
                O.adam_step(q, got[name][k].detach().cpu().double(), m_, v_, before[2], lr=lr, b1=0.5)
                e, tol = (p.double() - q.reshape(-1)).abs().max().item(), 1e-6 * q.abs().max().item() + 1e-5 * lr
                assert e <= tol, f"{what}: {e:.3e} from Adam on its own gradient (allowed {tol:.3e})"
            if k in dead:
                continue
            # api_cases.adam_close on the elements whose reference gradient has a definite sign (its own rule), one step at the most
            # on the others.  (Its guard against a gradient that is mostly noise does not fit every tensor here: an element of the
            # pixel discriminator's first bias whose channel keeps one sign over the batch sums a zero-mean InstanceNorm gradient.)
            g, r = ref[name][k].detach().float().reshape(-1), r.detach().float().reshape(-1)
            live = g.abs() > bounds.definite * g.abs().max().clamp_min(1e-30)
            assert live.any() or not g.any(), what
            # (behind the first step the update is lr' m / sqrt(v), continuous in the gradient: where the gradient bound allows an
            # element to be off by mx of the maximum it bounds no element's update below a step, and the replay above stands alone)
            if live.any() and (bounds.definite <= 1e-4 or before is None or before[2] == 1):
                A.adam_close(p[live], r[live], g[live], what, lr=lr)
            d = (p - r).abs()
            # (an element nothing reads -- an fc row no resized pixel samples -- and the last bias under wgangp, whose gradient is +w/n over
            # the fake and -w/n over the real patches: exactly zero in the reference, the parameter stays where it was)
            assert (d * (g == 0)).max().item() <= 1e-7, f"{what}: a parameter with zero gradient moved"
            assert d.max().item() <= 2.0 * lr * 1.001 + 1e-7, f"{what}: moved by more than a step: {d.max().item():.3e}"


# ------------------------------------------------------------------------------------------------ the device's side
def snapshot(m, out):
    """what one train_batch left, as reference_step returns it, plus the host-side state the row asserts"""
    tr = m.fused_trainer()
    pG, pD = params_of(m)
    rec = {"pred": tr.pred.detach().cpu().clone(), "losses": dict(out), "pG": pG, "pD": pD,
           "gG": {k: v.detach().cpu().clone() for k, v in tr.flatG.grad_views().items()},
           "gD": {k: v.detach().cpu().clone() for k, v in tr.flatD.grad_views().items()},
           "moments": (moments_of(tr.flatG), moments_of(tr.flatD)),
           "parts": [(mm.lo, mm.hi, mm.G.sample0) for mm in tr._state.micros], "n": tr._state.n, "states": len(tr._states),
           "drop": m.netG.dropout_state() if hasattr(m.netG, "dropout_state") else None}
    return rec


def expected_parts(row, shape=None):
    B = (shape or row.shape)[0]
    n = row.micro if B % row.micro == 0 else 1          # trainer._micro_count: the fallback to one part
    per = B // n
    return [(i * per, (i + 1) * per, i * per if row.drop else 0) for i in range(n)]


def host_state(tag, row, rec, call, shape=None):
    want = expected_parts(row, shape)
    assert rec["n"] == len(want), f"{row.id} {tag}: {rec['n']} parts, expected {len(want)}"
    assert rec["parts"] == want, f"{row.id} {tag}: parts (lo, hi, sample0) {rec['parts']}, expected {want}"
    if row.drop:
        assert rec["drop"] == (DROP_SEED, call), f"{row.id} {tag}: dropout state {rec['drop']}, expected call {call}"


def device_run(dev, row, switch=None):
    """two train_batch steps from the seeded model (and, with ``switch``, one at that shape and one at the first again): the snapshots"""
    m = make_model(row, dev)
    p0 = params_of(m)
    batch = make_batch(row, dev)
    recs = [snapshot(m, m.train_batch(batch).as_dict()) for _ in range(2)]
    if switch is not None:
        other = make_batch(row, dev, switch)
        recs.append(snapshot(m, m.train_batch(other).as_dict()))
        recs.append(snapshot(m, m.train_batch(batch).as_dict()))
    return p0, batch, recs


def bits_equal(tag, a, b):
    import torch
    for k in ("pred", "gG", "gD", "pG", "pD"):
        for name, x, y in ([(k, a[k], b[k])] if k == "pred" else [(f"{k} {n}", a[k][n], b[k][n]) for n in a[k]]):
            assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), f"{tag}: two runs differ in {name}"
    assert a["losses"] == b["losses"], f"{tag}: two runs differ in the losses: {a['losses']} {b['losses']}"


def stale_is_distinguishable(row, fresh, stale, applied):
    """(b) can notice a stale packed weight only if the reference at the stepped parameters and the one at the step-zero parameters
    differ by at least ten times the bound applied, in pred and in loss_G"""
    dp = (fresh["pred"] - stale["pred"]).abs().max().item() / fresh["pred"].abs().max().item()
    dl = abs(fresh["losses"]["loss_G"] - stale["losses"]["loss_G"]) / abs(fresh["losses"]["loss_G"])
    print(f"STEPMATRIX {row.id} stale against fresh at lr {row.lr:g}: pred {dp:.3e} loss_G {dl:.3e} (needed {10 * applied:.1e})")
    assert dp >= 10 * applied and dl >= 10 * applied, f"{row.id}: a stale second step is not distinguishable at lr {row.lr:g}: pred {dp:.3e} loss_G {dl:.3e}"


def lightning_sequence(dev, row):
    """training_step(b, 0, 0) -> backward -> HipAdam.step -> D frozen -> training_step(b, 0, 1) -> backward, from the seeded model"""
    m = make_model(row, dev)
    batch = make_batch(row, dev)
    (opt_d, opt_g), _ = m.configure_optimizers()
    loss_d = m.training_step(batch, 0, 0)
    opt_d.zero_grad()
    loss_d.backward()
    rec = {"gD": {k: q.grad.detach().cpu().clone() for k, q in m.netD.named_parameters()}}
    opt_d.step()
    for q in m.netD.parameters():
        q.requires_grad_(False)
    loss_g = m.training_step(batch, 0, 1)
    opt_g.zero_grad()
    loss_g.backward()
    rec["gG"] = {k: q.grad.detach().cpu().clone() for k, q in m.netG.named_parameters()}
    lg = {k: float(v) for k, v in m.logged.items() if k.startswith("model_loss/")}
    rec["losses"] = {"loss_D": float(loss_d.detach()), "loss_D_fake": lg["model_loss/discriminator_fake"],
                     "loss_D_real": lg["model_loss/discriminator_real"], "loss_G": float(loss_g.detach()),
                     "loss_G_gan": lg["model_loss/generator_GAN_loss"], "loss_G_l1": lg["model_loss/generator_L1"]}
    if row.rs != "off":
        rec["losses"]["loss_G_rs"] = lg["model_loss/indices_loss_weighted"]
    if row.ssim > 0.0:
        rec["losses"]["loss_G_ssim"] = lg["model_loss/generator_ssim"]
    rec["pD"] = params_of(m)[1]                     # (the sequence stops in front of Adam(G))
    rec["drop"] = m.netG.dropout_state() if row.drop else None
    return rec


def fused_against_lightning(row, fused, light):
    """without dropout both routes evaluate the same function: gan_loss_cases.FUSED_TOL"""
    import gan_loss_cases as Gc
    for k, v in light["losses"].items():
        assert abs(fused["losses"][k] - v) <= Gc.FUSED_TOL * abs(v), f"{row.id} fused against lightning {k}: {fused['losses'][k]} against {v}"
    deadG, deadD = dead_keys(row)
    Gc.grads_close(f"{row.id} fused against lightning gD", fused["gD"], light["gD"], deadD, Gc.FUSED_TOL, l2=False)
    Gc.grads_close(f"{row.id} fused against lightning gG", fused["gG"], light["gG"], deadG, Gc.FUSED_TOL, l2=False)


# ------------------------------------------------------------------------------------------------ the row
def run_row(dev, row, bounds, lightning=True, switch=True):
    """(a) first step, (b) second step, (c) shape switch on the rows of SWITCH, (d) the Lightning sequence, (e) bitwise repeat"""
    sw = SWITCH.get(row.id) if switch else None
    p0, batch, recs = device_run(dev, row, sw)
    cpu = {k: v.cpu() for k, v in batch.items()}
    # ---- (a)
    mk = masks(row, 11, dev)
    ref1 = reference_step(row, p0[0], p0[1], cpu, mk, mk)
    compare("a first step", row, recs[0], ref1, bounds, Worst(), before=(p0, None, 1))
    host_state("a", row, recs[0], 11)
    # ---- (b): the reference re-seeded from the device's parameters and moments after step one (Adam's division does not compound)
    mk = masks(row, 12, dev)
    ref2 = reference_step(row, recs[0]["pG"], recs[0]["pD"], cpu, mk, mk, moments=recs[0]["moments"], step=2)
    stale = reference_step(row, p0[0], p0[1], cpu, mk, mk)
    stale_is_distinguishable(row, ref2, stale, gpu_bounds(row).out)
    compare("b second step", row, recs[1], ref2, bounds, Worst(), before=((recs[0]["pG"], recs[0]["pD"]), recs[0]["moments"], 2))
    host_state("b", row, recs[1], 12)
    assert recs[1]["states"] == 1
    # ---- (c)
    if sw is not None:
        assert recs[2]["pred"].shape == (sw[0], 1, sw[1], sw[2]) and all(v == v for v in recs[2]["losses"].values())
        host_state("c other shape", row, recs[2], 13, sw)
        mk = masks(row, 14, dev)
        ref4 = reference_step(row, recs[2]["pG"], recs[2]["pD"], cpu, mk, mk, moments=recs[2]["moments"], step=4)
        compare("c back at the first shape", row, recs[3], ref4, bounds, Worst(), before=((recs[2]["pG"], recs[2]["pD"]), recs[2]["moments"], 4))
        host_state("c", row, recs[3], 14)
        assert recs[2]["states"] == 2 and recs[3]["states"] == 2, "one _ShapeState per (B, H, W[, dropout])"
    # ---- (d): with dropout the two forwards draw calls 11 and 12
    if lightning:
        light = lightning_sequence(dev, row)
        refl = ref1 if not row.drop else reference_step(row, p0[0], p0[1], cpu, masks(row, 11, dev), masks(row, 12, dev))
        compare("d lightning", row, light, refl, bounds, Worst(), pred=False, before=(p0, None, 1))
        if row.drop:
            assert light["drop"] == (DROP_SEED, 12)
        else:
            fused_against_lightning(row, recs[0], light)
    # ---- (e)
    _, _, again = device_run(dev, row, sw)
    for i, (a, b) in enumerate(zip(recs, again)):
        bits_equal(f"{row.id} e step {i + 1}", a, b)


def reference_alone(row):
    """the same restatement in fp32 on stock torch against float64, steps one and two: within half of the MI355X bounds everywhere"""
    import torch
    from nirgan_hip import lib as L
    assert L.is_emulated(), "the masks come from the emulator here"
    m = make_model(row, "cpu")
    p0 = params_of(m)
    batch = make_batch(row, "cpu")
    worst = Worst()
    mk = masks(row, 11, "cpu")
    r64, r32 = reference_step(row, p0[0], p0[1], batch, mk, mk), reference_step(row, p0[0], p0[1], batch, mk, mk, dtype=torch.float32)
    compare("fp32 restatement step 1", row, r32, r64, gpu_bounds(row), worst)
    mk = masks(row, 12, "cpu")
    zero = lambda p: {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in p.items()}      # noqa: E731
    mom = (zero(r32["pG"]), zero(r32["pD"]))
    s64 = reference_step(row, r32["pG"], r32["pD"], batch, mk, mk, moments=mom, step=2)
    s32 = reference_step(row, r32["pG"], r32["pD"], batch, mk, mk, moments=mom, step=2, dtype=torch.float32)
    compare("fp32 restatement step 2", row, s32, s64, gpu_bounds(row), worst, params=False)
    if row.drop:             # (d) with dropout: the Lightning sequence's two forwards draw the masks of calls 11 and 12
        mk = (masks(row, 11, "cpu"), masks(row, 12, "cpu"))
        l64, l32 = reference_step(row, p0[0], p0[1], batch, *mk), reference_step(row, p0[0], p0[1], batch, *mk, dtype=torch.float32)
        compare("fp32 restatement lightning", row, l32, l64, gpu_bounds(row), worst, params=False)
    assert worst.top() <= 0.5, f"{row.id}: stock fp32 uses {worst.top():.2f} of a bound ({worst.line()}): the row needs another data seed"
    return worst
