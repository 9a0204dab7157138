"""Bodies of the dropout tests, shared by the CPU suite (C ABI served by the numpy statement of tests/emu_dropout.py:
tests/test_dropout_emulated.py) and the MI355X suite (the HIP library: tests/test_gpu_dropout.py).

The mask is a function of (seed, call, stream_id, position) alone (include/nirgan_hip.h: nirgan_dropout_desc), so every check is
exact where the arithmetic is (bitwise masks, selects, folds) and uses the no-dropout bounds where it is the network's fp32
arithmetic that is compared (dropout is a select and a multiplication by 2: it earns no extra margin).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nirgan_oracle as O
from api_cases import Tol, close, grad_close
from emu_dropout import keep_mask, mask_nchw, philox4x32_10
from nirgan_hip import dropout as HD
from nirgan_hip import lib as L

KNOWN_ANSWERS = [       # Philox4x32-10: (counter, key) -> output words
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
MASK_SHAPES = [(1, 2, 2, 4), (3, 5, 7, 64), (2, 9, 11, 32), (2, 16, 16, 256)]
SEEDS = [(1234, 0), (0x9ABCDEF0, 0x12345678)]           # (lo, hi): the second with a non-zero high word
ns = types.SimpleNamespace


def seed64(seed):
    return seed[0] | (seed[1] << 32)


# ------------------------------------------------------------------------------------------------ kernel level
def philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = tuple(int(w[0]) for w in philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(g) for g in got])


def mask_bitwise(dev, shape, seed):
    B, H, W, Cc = shape
    for call in (1, 2):
        for sid in (0, 5):
            for s0 in (0, 3):
                got = HD.mask(seed64(seed), call, sid, B, H, W, Cc, sample0=s0, device=dev).cpu().numpy()
                want = mask_nchw(seed, call, sid, B, H, W, Cc, s0)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, seed, call, sid, s0)


def _reflect_pad_nhwc(x, pad):
    if pad == 0:
        return x.clone()
    return F.pad(x.permute(0, 3, 1, 2), (pad,) * 4, mode="reflect").permute(0, 2, 3, 1).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def in_place_semantics(dev, pad):
    B, H, W, Cc, seed, call, sid, guard = 2, 5, 7, 8, SEEDS[1], 3, 2, 64
    g = torch.Generator().manual_seed(5 + pad)
    x = torch.randn(B, H, W, Cc, generator=g)
    keep = torch.from_numpy(keep_mask(seed, call, sid, B, H, W, Cc))
    drop = (~keep).nonzero()
    x[tuple(drop[0])] = float("nan")                    # a NaN and an Inf at dropped positions come out as +0
    x[tuple(drop[1])] = float("inf")
    kept = keep.nonzero()
    x[tuple(kept[0])] = float("inf")                    # a kept Inf stays Inf
    padded = _reflect_pad_nhwc(x, pad)
    n = padded.numel()
    buf = torch.full((n + 2 * guard,), 7.25)
    buf[guard:guard + n] = padded.reshape(-1)
    buf = buf.to(dev)
    state = HD.state_words(seed, call).to(dev)
    HD.apply_halo(buf[guard:guard + n], state, B, H, W, Cc, pad, sid)
    out = buf.cpu()
    assert torch.equal(out[:guard], torch.full((guard,), 7.25)) and torch.equal(out[guard + n:], torch.full((guard,), 7.25)), "guard floats written"
    got = out[guard:guard + n].reshape(B, H + 2 * pad, W + 2 * pad, Cc)
    want = torch.where(keep, 2.0 * x, torch.zeros(()))
    inner = got[:, pad:pad + H, pad:pad + W]
    assert np.array_equal(_bits(inner), _bits(want)), "interior is not select(mask, 2x, 0)"
    assert np.array_equal(_bits(got), _bits(_reflect_pad_nhwc(inner, pad))), "halo is not the reflection of the new interior"
    assert inner[tuple(drop[0])].item() == 0.0 and inner[tuple(drop[1])].item() == 0.0 and not np.signbit(inner[tuple(drop[0])].item())
    assert torch.isinf(inner[tuple(kept[0])])


def _fold(gp, pad):
    """Adjoint of ReflectionPad2d on [B][H + 2 pad][W + 2 pad][C]: every halo element added onto the interior pixel it reflects."""
    B, hp, wp, Cc = gp.shape
    H, W = hp - 2 * pad, wp - 2 * pad
    out = torch.zeros(B, H, W, Cc, dtype=gp.dtype)

    def src(i, n):
        i = abs(i - pad)
        return 2 * (n - 1) - i if i >= n else i
    for y in range(hp):
        for x in range(wp):
            out[:, src(y, H), src(x, W)] += gp[:, y, x]
    return out


def fold_identity(dev):
    B, H, W, Cc, pad, seed, call, sid = 2, 5, 7, 8, 1, SEEDS[0], 1, 4
    g = torch.Generator().manual_seed(11)
    gp = torch.randn(B, H + 2, W + 2, Cc, generator=g)
    buf = gp.clone().to(dev)
    HD.apply_halo(buf, HD.state_words(seed, call).to(dev), B, H, W, Cc, pad, sid)
    m = torch.from_numpy(mask_nchw(seed, call, sid, B, H, W, Cc)).permute(0, 2, 3, 1)
    # x2 is exact and commutes with the sums, a dropped element adds +0: bitwise.  "Times the mask" is the entry's select (a product
    # with 0 would leave -0 where the folded gradient is negative; the select and the sum of +0 terms both leave +0)
    want = torch.where(m > 0, 2.0 * _fold(gp, pad), torch.zeros(()))
    assert np.array_equal(_bits(_fold(buf.cpu(), pad)), _bits(want))


def statistics(dev):
    B, H, W, Cc = 2, 9, 11, 64
    ms = {}
    for sid in (0, 1):
        for call in (1, 2):
            m = HD.mask(1234, call, sid, B, H, W, Cc, device=dev).cpu() > 0
            ms[(sid, call)] = m
            frac = m.float().mean().item()
            print(f"keep fraction stream {sid} call {call}: {frac:.4f}")
            assert abs(frac - 0.5) <= 0.022, (sid, call, frac)          # 5 sigma of 12 672 fair bits
    for a, b in (((0, 1), (1, 1)), ((0, 2), (1, 2)), ((0, 1), (0, 2)), ((1, 1), (1, 2))):
        diff = (ms[a] != ms[b]).float().mean().item()
        assert 0.4 <= diff <= 0.6, (a, b, diff)


def advance(dev):
    state = HD.state_words((7, 9), 41).to(dev)
    st = torch.cuda.current_stream(state.device).cuda_stream if state.device.type == "cuda" else None
    for k in range(3):
        L.call("nirgan_dropout_advance", state.data_ptr(), st)
        assert state.cpu().tolist() == [7, 9, 42 + k, 0]
    a = HD.mask((7, 9), 44, 0, 1, 3, 3, 4, device=dev)
    ones = torch.ones(1, 3, 3, 4, device=dev)
    HD.apply_halo(ones, state, 1, 3, 3, 4, 0, 0)                        # the kernels read the call the advance left
    assert torch.equal(ones.permute(0, 3, 1, 2), a)


def argument_errors(be):
    """Every listed error returns -1 with a message before any launch (host tensors: a launch would fault)."""
    buf, state = torch.zeros(2 * 6 * 7 * 8 + 4), HD.state_words(1, 1)

    def desc(**kw):
        d = L.DropoutDesc()
        d.buf, d.buf_elems, d.B, d.H, d.W, d.C, d.pad = buf.data_ptr(), 2 * 6 * 7 * 8, 2, 4, 5, 8, 1
        d.state, d.stream_id, d.sample0 = state.data_ptr(), 0, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = {"null buf": dict(buf=None), "null state": dict(state=None), "C % 4": dict(C=6), "pad < 0": dict(pad=-1),
             "pad >= min(H, W)": dict(pad=4, buf_elems=1 << 30), "buf_elems": dict(buf_elems=2 * 6 * 7 * 8 - 1),
             "2^40": dict(B=1 << 20, H=1 << 10, W=1 << 10, C=4, pad=0, buf_elems=1 << 62)}
    for what, kw in cases.items():
        assert be.nirgan_dropout_halo(C.byref(desc(**kw)), None) == -1, what
        assert b"dropout_halo" in be.nirgan_last_error(), what
    if not getattr(be, "is_emulator", False):
        assert be.nirgan_dropout_halo(None, None) == -1
    assert be.nirgan_dropout_advance(None, None) == -1 and b"dropout_advance" in be.nirgan_last_error()


# ------------------------------------------------------------------------------------------------ whole net
def stock_generator(input_nc, output_nc, ngf, n_blocks):
    """The module list of the reference's ResnetGenerator with use_dropout=True as stock torch.nn (InstanceNorm, reflect padding):
    written down here for the key list, the initialisation order and the float64 comparison."""
    IN = lambda c: nn.InstanceNorm2d(c, affine=False, track_running_stats=False)     # noqa: E731

    class Block(nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.conv_block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, 3), IN(dim), nn.ReLU(True), nn.Dropout(0.5),
                                            nn.ReflectionPad2d(1), nn.Conv2d(dim, dim, 3), IN(dim))

    class Gen(nn.Module):
        def __init__(self):
            super().__init__()
            m = [nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, 7), IN(ngf), nn.ReLU(True)]
            for i in range(2):
                m += [nn.Conv2d(ngf * 2 ** i, ngf * 2 ** (i + 1), 3, stride=2, padding=1), IN(ngf * 2 ** (i + 1)), nn.ReLU(True)]
            m += [Block(ngf * 4) for _ in range(n_blocks)]
            for i in range(2):
                c = ngf * 2 ** (2 - i)
                m += [nn.ConvTranspose2d(c, c // 2, 3, stride=2, padding=1, output_padding=1), IN(c // 2), nn.ReLU(True)]
            m += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, output_nc, 7), nn.Tanh()]
            self.model = nn.Sequential(*m)
    return Gen()


def _stock_init(net, gain=0.02):
    for mod in net.modules():            # module order = the reference's init_weights walk
        if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
            nn.init.normal_(mod.weight.data, 0.0, gain)
            nn.init.constant_(mod.bias.data, 0.0)


def state_dict_is_the_references():
    from model import networks
    rng = torch.get_rng_state()
    torch.manual_seed(3)
    ours = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", True, "normal", 0.02)
    after = torch.rand(1)
    torch.manual_seed(3)
    stock = stock_generator(3, 1, 8, 6)
    _stock_init(stock)
    assert torch.equal(after, torch.rand(1)), "construction consumed other random numbers than the reference's layers do"
    torch.set_rng_state(rng)
    sd, ref = ours.state_dict(), stock.state_dict()
    assert list(sd) == list(ref)
    assert "model.10.conv_block.6.weight" in sd and not [k for k in sd if "conv_block.5" in k]
    for k in ref:
        assert torch.equal(sd[k], ref[k]), k
    stock.load_state_dict(sd, strict=True)
    other = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", True, "normal", 0.02)
    other.load_state_dict(ref, strict=True)
    assert isinstance(ours.model[10].conv_block[4], nn.Dropout) and ours.model[10].conv_block[4].p == 0.5
    assert ours.use_dropout and ours.dropout_state() == (None, 0)


def synth(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.02 + 0.58 * torch.rand(B, 3, H, W, generator=g), 0.05 + 0.75 * torch.rand(B, 1, H, W, generator=g)


def eval_mode_is_the_identity(dev, ngf=8, size=32):
    from model import networks
    torch.manual_seed(4)
    drop = networks.define_G(3, 1, ngf, "resnet_6blocks", "instance", True, "normal", 0.02)
    plain = networks.define_G(3, 1, ngf, "resnet_6blocks", "instance", False, "normal", 0.02)
    plain.load_state_dict({k.replace("conv_block.6", "conv_block.5"): v for k, v in drop.state_dict().items()}, strict=True)
    rgb = synth(2, size, size, 1)[0].to(dev)
    drop, plain = drop.to(dev).eval(), plain.to(dev).eval()
    with torch.no_grad():
        a, b = drop(rgb), plain(rgb)
    assert np.array_equal(_bits(a), _bits(b))
    assert drop.dropout_state() == (None, 0), "an eval-mode forward drew a seed or counted a call"


def forward64(p, x, n_blocks, masks, embeds=None, post_correction=False):
    """float64 restatement of the generator with the blocks' dropout as a multiplication by the given {0, 2} masks (a net built without
    dropout carries the blocks' second convolution as conv_block.5: read off the keys).  It runs in the dtype of its arguments."""
    c2 = "conv_block.6" if "model.10.conv_block.6.weight" in p else "conv_block.5"
    IN = lambda t: F.instance_norm(t, eps=1e-5)                  # noqa: E731
    rp = lambda t, n: F.pad(t, (n,) * 4, mode="reflect")         # noqa: E731
    h = F.relu(IN(F.conv2d(rp(x, 3), p["model.1.weight"], p["model.1.bias"])))
    z = IN(F.conv2d(h, p["model.4.weight"], p["model.4.bias"], stride=2, padding=1))
    if embeds is not None:
        z = O.inject_modulation(p, z, embeds, "multiply", True)
    h = F.relu(IN(F.conv2d(F.relu(z), p["model.7.weight"], p["model.7.bias"], stride=2, padding=1)))
    for j in range(n_blocks):
        i = 10 + j
        t = F.relu(IN(F.conv2d(rp(h, 1), p[f"model.{i}.conv_block.1.weight"], p[f"model.{i}.conv_block.1.bias"])))
        t = t * masks[j]
        h = h + IN(F.conv2d(rp(t, 1), p[f"model.{i}.{c2}.weight"], p[f"model.{i}.{c2}.bias"]))
    for i in (10 + n_blocks, 13 + n_blocks):
        h = F.relu(IN(F.conv_transpose2d(h, p[f"model.{i}.weight"], p[f"model.{i}.bias"], stride=2, padding=1, output_padding=1)))
    i = 17 + n_blocks
    out = torch.tanh(F.conv2d(rp(h, 3), p[f"model.{i}.weight"], p[f"model.{i}.bias"]))
    return out * p["post_correction_param"] if post_correction else out          # generator_inject.py:133-134


def inject_config(ngf, no_dropout=False):
    return ns(base_configs=ns(input_nc=3, output_nc=1, ngf=ngf, netG="resnet_9blocks", norm="instance", no_dropout=no_dropout,
                              init_type="normal", init_gain=0.02),
              satclip=ns(satclip_inject_style="multiply", post_correction=False, post_correction_init=1.0, scaling_param=True,
                         scaling_param_init=0.01))


def shadowed(n_blocks):
    return {k.replace("conv_block.5", "conv_block.6") for k in O.shadowed_bias_keys("G", n_blocks)}


def make_generator(ngf, n_blocks, inject, seed=6):
    from model import networks
    torch.manual_seed(seed)
    if inject:
        from model.generator_inject import define_G_inject
        net = define_G_inject(inject_config(ngf))
        with torch.no_grad():            # (init_net's N(0, 0.02) on the 16384 x 256 projection keeps the modulation tiny: make it count)
            net.fc.weight.mul_(4.0)
            net.scale_param.fill_(0.5)
        return net
    return networks.define_G(3, 1, ngf, f"resnet_{n_blocks}blocks", "instance", True, "normal", 0.02)


def train_mode_against_float64(dev, ngf, n_blocks, B, H, W, tol: Tol, inject=False, seed=(0xC0FFEE, 0x51)):
    net = make_generator(ngf, n_blocks, inject)
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    net = net.to(dev).train()
    rgb = synth(B, H, W, 2)[0]
    g = torch.Generator().manual_seed(8)
    emb = torch.randn(B, 256, generator=g) if inject else None
    w = torch.randn(B, 1, H, W, generator=g)
    net.set_dropout_state(seed=seed64(seed), call=4)
    args = (rgb.to(dev),) + ((emb.to(dev),) if inject else ())
    pred = net(*args)
    assert net.dropout_state() == (seed64(seed), 5)
    (pred * w.to(dev)).sum().backward()
    masks = [HD.mask(seed64(seed), 5, j, B, H // 4, W // 4, 4 * ngf, device=dev).cpu().double() for j in range(n_blocks)]
    for j, m in enumerate(masks):        # the masks the engine used are the exported ones, which are the restatement's
        assert np.array_equal(m.float().numpy(), mask_nchw(seed, 5, j, B, H // 4, W // 4, 4 * ngf)), j
    ref = forward64(p64, rgb.double(), n_blocks, masks, None if emb is None else emb.double())
    (ref * w.double()).sum().backward()
    e = (pred.detach().cpu().double() - ref.detach()).abs().max().item() / ref.detach().abs().max().item()
    print(f"pred: max err {e:.3e} of the range")
    close(pred, ref, tol.out, "pred")
    skip = shadowed(n_blocks)
    for k, q in net.named_parameters():
        if k in skip:
            continue
        r = p64[k].grad
        e2 = ((q.grad.detach().cpu().double() - r).norm() / r.norm().clamp_min(1e-30)).item()
        print(f"grad {k}: rel L2 {e2:.3e}")
    for k, q in net.named_parameters():
        if k not in skip:
            grad_close(q.grad, p64[k].grad, tol, "grad " + k)
    return net


def mask_sequence(dev, ngf=8, size=32):
    net = make_generator(ngf, 6, False).to(dev).train()
    rgb = synth(2, size, size, 3)[0].to(dev)
    w = torch.linspace(-1.0, 1.0, 2 * size * size).reshape(2, 1, size, size).to(dev)

    def run():
        for q in net.parameters():
            q.grad = None
        pred = net(rgb)
        (pred * w).sum().backward()
        return pred.detach().clone(), [q.grad.clone() for q in net.parameters()]
    torch.manual_seed(77)
    p1, g1 = run()
    seed, call = net.dropout_state()
    assert call == 1 and seed is not None
    torch.manual_seed(77)
    assert seed == int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()), "the default seed is not torch's default generator's"
    p2, _ = run()
    assert net.dropout_state() == (seed, 2)
    assert not torch.equal(p1, p2), "two training forwards drew the same mask"
    net.set_dropout_state(seed=seed, call=0)
    p3, g3 = run()
    assert np.array_equal(_bits(p1), _bits(p3))
    for a, b in zip(g1, g3):
        assert np.array_equal(_bits(a), _bits(b))
    with torch.no_grad():                # training mode without autograd still drops (nn.Dropout's rule) and counts
        p4 = net(rgb)
    assert net.dropout_state() == (seed, 2) and not torch.equal(p4, p3)


def px_config(ngf, lr, no_dropout=False):
    from api_cases import px_config as base
    cfg = base(6, ngf)
    cfg.base_configs.no_dropout = no_dropout
    cfg.base_configs.lr = lr
    return cfg


def fused_trainer(dev, ngf=8, size=32):
    from model.pix2pix import Px2Px_PL
    torch.manual_seed(9)
    m = Px2Px_PL(px_config(ngf, 0.0)).to(dev).train()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    rgb, nir = synth(4, size, size, 4)
    batch = {"rgb": rgb.to(dev), "nir": nir.to(dev)}
    seed = 0x1234ABCD5678
    m.netG.set_dropout_state(seed=seed, call=10)
    out = m.train_batch(batch).as_dict()
    assert all(np.isfinite(v) for v in out.values()), out
    assert m.netG.dropout_state() == (seed, 11)
    tr = m.fused_trainer()
    assert tr.G.dropout and tr.G.drop_state.cpu().tolist()[2] == 11
    gG = {k: v.clone() for k, v in tr.flatG.grad_views().items()}
    flatG, flatD = tr.flatG.grad.clone(), tr.flatD.grad.clone()        # (the autograd route below writes the same flat ranges)
    pred = tr.pred.clone()
    # the autograd route at the same (seed, call), lr = 0: the generator pass of the Lightning sequence
    m.netG.set_dropout_state(call=10)
    for q in m.netD.parameters():
        q.requires_grad_(False)
    loss_g = m.training_step(batch, 1, 1)
    loss_g.backward()
    assert m.netG.dropout_state() == (seed, 11)
    close(loss_g, out["loss_G"], 1e-5, "loss_G")
    skip = shadowed(6)
    for k, q in m.netG.named_parameters():
        if k not in skip:
            close(q.grad, gG[k], 1e-6, "autograd vs fused " + k)
    # micro_batches = 2: the two halves draw the masks of samples 0..1 and 2..3 of the same call
    m2 = Px2Px_PL(px_config(ngf, 0.0))
    m2.load_state_dict(sd)
    m2 = m2.to(dev).train()
    m2.fused_trainer().micro_batches = 2
    m2.netG.set_dropout_state(seed=seed, call=10)
    m2.train_batch(batch)
    tr2 = m2.fused_trainer()
    assert tr2._state.n == 2 and [mm.G.sample0 for mm in tr2._state.micros] == [0, 2] and m2.netG.dropout_state() == (seed, 11)
    close(tr2.pred, pred, 1e-5, "pred, two micro-batches")
    assert ((tr2.flatG.grad - flatG).norm() / flatG.norm()).item() < 1e-3
    assert ((tr2.flatD.grad - flatD).norm() / flatD.norm()).item() < 1e-4


def bf16_refusal(dev):
    net = make_generator(8, 6, False).to(dev).train()
    net.precision = "bf16"
    with pytest.raises(NotImplementedError, match="fp32"):
        net(synth(1, 32, 32, 1)[0].to(dev))
    net.eval()                           # the identity needs no mask: every operand mode runs it
    with torch.no_grad():
        assert torch.isfinite(net(synth(1, 32, 32, 1)[0].to(dev))).all()


def legacy_model_accepts_dropout(dev, size=32):
    """Pix2PixModel (model/pix2pix_model.py:65 passes ``not opt.no_dropout``): one optimize_parameters with dropout -- finite losses, ONE
    training forward counted, generator gradients everywhere but on the biases an InstanceNorm shadows."""
    from model.pix2pix_model import Pix2PixModel
    torch.manual_seed(12)
    model = Pix2PixModel(px_config(8, 0.0002))
    assert model.netG.use_dropout and "model.10.conv_block.6.weight" in model.netG.state_dict()
    model.to(dev)
    rgb, nir = synth(2, size, size, 6)
    model.set_input({"A": rgb.to(dev), "B": nir.to(dev)})
    model.netG.set_dropout_state(seed=99, call=0)
    model.optimize_parameters()
    assert model.netG.dropout_state() == (99, 1)
    for v in (model.loss_D, model.loss_G_GAN, model.loss_G_L1):
        assert torch.isfinite(torch.as_tensor(v)).all()
    m = HD.mask(99, 1, 0, 2, size // 4, size // 4, 32, device=dev)
    assert set(m.unique().tolist()) == {0.0, 2.0}
