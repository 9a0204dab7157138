"""Every weight-gradient launch the shipped nets emit, replayed at its exact geometry against the float64 restatement of its descriptor
(tests/wgrad_replay.py).

Census: one training step of the trainer in each configuration of CONFIGS; the backward plans (G.bwd, D2.bwd, D1.bwd_pred, as
bench.py::mfma_probes walks them) are searched for nirgan_wgrad_igemm, nirgan_conv_wgrad_pair and nirgan_wino6_gemm_wgrad_pair ops, and
each descriptor is copied.  Replay: the copy is pointed at buffers of its own (the sizes it declares) and launched through the entry point
the plan uses:
  * integer pass -- every element of P and Q (halos and the channels beyond N included) from {-2, -1, 1, 2}: every product and partial sum
    is exact in fp32, in bf16 and in the split forms, so every slab of every split and plane must be BITWISE the float64 restatement, and
    the slab memory past the launch's slabs (plus a guard) must still hold the sentinel;
  * random pass -- N(0, 1) operands (bf16 values where the launch reads bf16): (a) every slab element within the rigorous bound of its
    inner product, gamma_n |P|^T |Q| with n = the products summed in fp32 (rows_per_split times the bf16 products per fp32 product), plus
    slack for the products the split forms drop; (b) on the three-term split tile, max and rms error against float64 at most 2.0 x and
    2.5 x those of the same descriptor on the exact-fp32 tile (test_gpu_x3.py's bounds); (c) a second launch gives the same bits.
The fused pairs run as pairs: the data-gradient half reads the replay's P buffer (the same dY) and writes scratch; only the weight-gradient
half is checked here.  nirgan_wino6_gemm_wgrad_pair (exact-fp32 mode only) is replayed through nirgan_wgrad_igemm with its weight-gradient
descriptor: the fused pair kernel itself stays covered only by the equality tests of test_gpu_kernels.py."""
import ctypes as C
import gc
import time

import pytest
import torch

import wgrad_replay as R
from nirgan_hip import geometry as G
from nirgan_hip import lib as L
from nirgan_hip.engine import Ctx, Halo, Plan, emit_conv, emit_wgrad
from nirgan_hip.options import OPT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# csrc/igemm_wgrad.hip: WGRAD_KERNEL_NAMES and PAIR_KERNEL_NAMES
WGRAD_ROUTES = ("wgrad_x3_kernel<256>", "wgrad_x3_kernel<128>", "wgrad_igemm256_kernel", "wgrad_persist_kernel", "wgrad_igemm16_kernel",
                "wgrad_igemm_kernel<128>", "wgrad_igemm_kernel<64>")
PAIR_ROUTES = ("(two launches)", "conv_wgrad_pair256_kernel", "conv_wgrad_pair_kernel")
X3_ROUTES = WGRAD_ROUTES[:2]

CONFIGS = {   # name -> trainer setup
    "configs[1]": dict(blocks=6, B=16, size=256),
    "padding=10": dict(blocks=6, B=16, size=256, padding=10),
    "configs[3] per GPU": dict(blocks=9, B=8, size=512, padding=10, inject=True),
    "configs[2] geometry": dict(blocks=9, B=32, size=256),
    "exact fp32": dict(blocks=6, B=16, size=256, split3=False),
    "bf16": dict(blocks=6, B=16, size=256, precision="bf16"),
    "bf16x3": dict(blocks=6, B=16, size=256, precision="bf16x3"),
}

_CENSUS = {}     # config -> [Op]


class Op:
    """one weight-gradient launch of a plan: `w` a copy of its descriptor, `c` the copy of the data-gradient half of a fused pair"""

    def __init__(self, kind, plan, w, c=None):
        self.kind, self.plan, self.w, self.c = kind, plan, R.copy_desc(w), (R.copy_desc(c) if c is not None else None)
        be = L.backend()
        self.pair = be.nirgan_conv_wgrad_pair_kernel_name(C.byref(c), C.byref(w)).decode() if kind == "pair" else None
        self.route = be.nirgan_wgrad_kernel_name(C.byref(w)).decode()     # what a stand-alone launch of the weight gradient runs on

    def geometry(self):
        """the descriptors without their pointers: ops of equal geometry run the same launch"""
        key = []
        for d in (self.w, self.c):
            if d is None:
                continue
            key.append(tuple((n, tuple(getattr(d, n)) if n.startswith("tap_") else getattr(d, n)) for n, t in type(d)._fields_
                             if t is not C.c_void_p))
        return self.kind, tuple(key)

    def line(self):
        w = self.w
        route = self.route if self.pair in (None, "(two launches)") else self.pair
        return (f"  {self.plan:9s} {self.kind:5s} B {w.B:3d} OH {w.OH:4d} OW {w.OW:4d} N {w.N:5d} K {w.ntaps * w.run:5d} planes {max(w.nplanes, 1):2d} "
                f"nsplit {w.nsplit:4d} rows {w.rows_per_split:6d} prec {w.precision} {'twins ' if w.pq_bf16 else ''}-> {route}")


def _trainer(blocks, B, size, padding=0, inject=False, precision="fp32"):
    import types
    from model import networks
    from nirgan_hip.trainer import Pix2PixTrainer
    torch.manual_seed(0)
    embeds = None
    if inject:
        from model.generator_inject import define_G_inject
        ns = types.SimpleNamespace
        cfg = ns(base_configs=ns(input_nc=3, output_nc=1, ngf=64, netG=f"resnet_{blocks}blocks", norm="instance", no_dropout=True,
                                 init_type="normal", init_gain=0.02),
                 satclip=ns(satclip_inject_style="multiply", post_correction=False, post_correction_init=1.0,
                            scaling_param=True, scaling_param_init=0.01))
        netG = define_G_inject(cfg)
        embeds = torch.randn(B, 256, generator=torch.Generator().manual_seed(99)).to(DEV)
    else:
        netG = networks.define_G(3, 1, 64, f"resnet_{blocks}blocks", "instance", False, "normal", 0.02)
    netD = networks.define_D(4, 64, "basic", 3, "instance", "normal", 0.02)
    tr = Pix2PixTrainer(netG.to(DEV), netD.to(DEV), n_blocks=blocks, padding=padding, precision=precision,
                        inject={"style": "multiply", "use_scale": True} if inject else None)
    g = torch.Generator().manual_seed(1234)
    rgb = (0.02 + 0.58 * torch.rand(B, 3, size, size, generator=g)).to(DEV)
    nir = (0.05 + 0.75 * torch.rand(B, 1, size, size, generator=g)).to(DEV)
    return tr, rgb, nir, embeds


def census(name):
    """the weight-gradient ops of one training step in configuration `name` (built once per session; the trainer is freed)"""
    if name in _CENSUS:
        return _CENSUS[name]
    setup = dict(CONFIGS[name])
    split3 = setup.pop("split3", True)
    old = OPT.split3
    OPT.split3 = split3
    try:
        tr, rgb, nir, embeds = _trainer(**setup)
        tr.step(rgb, nir, embeds)
        torch.cuda.synchronize()
        ops = []
        for plan_name, plan in (("G.bwd", tr.G.bwd), ("D2.bwd", tr.D2.bwd), ("D1.pred", tr.D1.bwd_pred)):
            for op, args in plan.ops:
                if op == "nirgan_wgrad_igemm":
                    ops.append(Op("wgrad", plan_name, args[0]._obj))
                elif op == "nirgan_conv_wgrad_pair":
                    ops.append(Op("pair", plan_name, args[1]._obj, args[0]._obj))
                elif op == "nirgan_wino6_gemm_wgrad_pair":
                    ops.append(Op("wino6", plan_name, args[1]._obj))
    finally:
        OPT.split3 = old
    del tr, rgb, nir, embeds
    gc.collect()
    torch.cuda.empty_cache()
    assert ops, f"{name}: no weight-gradient launch in the backward plans"
    _CENSUS[name] = ops
    return ops


def _integers(t: torch.Tensor, g: torch.Generator):
    v = torch.tensor([-2.0, -1.0, 1.0, 2.0], device=DEV)[torch.randint(0, 4, (t.numel(),), generator=g, device=DEV)]
    t.copy_(v.to(t.dtype))


def _randn(t: torch.Tensor, bf16_values: bool, g: torch.Generator):
    v = torch.randn(t.numel(), generator=g, device=DEV)
    t.copy_((v.to(torch.bfloat16) if bf16_values else v).to(t.dtype))


def _err(got, ref):
    e = (got.double() - ref).abs()
    s = ref.abs().max().item()
    return e.max().item() / s, e.pow(2).mean().sqrt().item() / s


class Replay:
    """one op over fresh buffers, launched the way the plan launches it"""

    def __init__(self, op: Op):
        self.op = op
        c = op.c
        same = c is not None and bool(c.in_bf16) == bool(op.w.pq_bf16)
        self.f = R.FreshWgrad(op.w, DEV, p_elems_min=c.in_elems if same else 0)
        self.keep = []
        if c is not None:
            inp = self.f.p if same else torch.zeros(c.in_elems, dtype=torch.bfloat16 if c.in_bf16 else torch.float32, device=DEV)
            self.c, self.keep = R.fresh_conv(c, inp, DEV)
        be = L.backend()
        assert be.nirgan_wgrad_kernel_name(C.byref(self.f.d)).decode() == op.route, "the replay's copy routes elsewhere"
        if c is not None:
            assert be.nirgan_conv_wgrad_pair_kernel_name(C.byref(self.c), C.byref(self.f.d)).decode() == op.pair

    def launch(self, standalone=False):
        self.f.arm()
        if self.op.kind == "pair" and not standalone:
            L.call("nirgan_conv_wgrad_pair", C.byref(self.c), C.byref(self.f.d), None)
        else:
            L.call("nirgan_wgrad_igemm", C.byref(self.f.d), None)
        torch.cuda.synchronize()
        return self.f.written()

    def where(self, got, ref):
        bad = (got.double() != ref).nonzero()
        nan = int(torch.isnan(got).sum())
        return f"{len(bad)} elements differ, {nan} never written (sentinel), first at [plane, split, n, J] = {bad[0].tolist() if len(bad) else None}"


# fp32 products each route sums per pixel: gamma_n with n = rows_per_split * this (products of bf16 terms are exact in fp32)
PRODUCTS_PER_PIXEL = {0: 1, 1: 1, 2: 3, 3: 6}


def replay(op: Op, g: torch.Generator, report: dict):
    """the integer and the random pass of one op; report[route] collects the worst (b) ratios of the split tile"""
    r = Replay(op)
    d, f = r.f.d, r.f
    tag = f"{op.line().strip()}"
    # -- integer pass: bitwise
    assert 4 * d.rows_per_split < 2 ** 24
    _integers(f.p, g)
    _integers(f.q, g)
    got = r.launch()
    ref = R.restate(d, f.p, f.q)
    assert torch.equal(got.double(), ref), f"integer pass: {r.where(got, ref)}; {tag}"
    assert f.untouched_tail(), f"integer pass: a store past the launch's slabs; {tag}"
    # -- random pass
    bf16_values = bool(d.pq_bf16) or d.precision == 1
    _randn(f.p, bf16_values, g)
    _randn(f.q, bf16_values, g)
    got = r.launch().clone()
    again = r.launch()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), f"(c) a second launch differs; {tag}"
    assert f.untouched_tail(), f"random pass: a store past the launch's slabs; {tag}"
    ref, scale = R.restate_with_scale(d, f.p, f.q, precision=d.precision)
    n = PRODUCTS_PER_PIXEL[d.precision] * d.rows_per_split
    bound = (n + d.nsplit + 8) * 2.0 ** -24 * scale
    err = (got.double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    assert (err <= bound).all(), f"(a) rounding bound exceeded by {worst:.3g} x; {tag}"
    runs_on = op.route if op.pair in (None, "(two launches)") else op.pair
    if runs_on in X3_ROUTES:
        # (b) against the exact-fp32 tile on the same descriptor and operands
        exact = R.restate(d, f.p, f.q)
        e3 = _err(got, exact)
        d.precision = 0
        assert L.backend().nirgan_wgrad_kernel_name(C.byref(d)).decode().startswith("wgrad_igemm_kernel<")
        e0 = _err(r.launch(standalone=True), exact)
        d.precision = 3
        assert e3[0] <= 2.0 * e0[0] + 2e-7 and e3[1] <= 2.5 * e0[1] + 5e-8, (f"(b) split tile vs exact tile (max, rms): {e3} vs {e0}; {tag}")
        rb = report.setdefault(runs_on, [0.0, 0.0])
        rb[0], rb[1] = max(rb[0], e3[0] / max(e0[0], 1e-300)), max(rb[1], e3[1] / max(e0[1], 1e-300))
    report.setdefault("(a) worst fraction of the bound", [0.0])[0] = max(report.get("(a) worst fraction of the bound", [0.0])[0], worst)
    del r


def _unique(ops):
    seen, out = set(), []
    for op in ops:
        k = op.geometry()
        if k not in seen:
            seen.add(k)
            out.append(op)
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_weight_gradient_launch_replays_against_float64(config):
    t0 = time.time()
    ops = census(config)
    g = torch.Generator(device=DEV).manual_seed(17)
    report = {}
    uniq = _unique(ops)
    for op in uniq:
        assert op.route in WGRAD_ROUTES, op.line()
        assert op.pair is None or op.pair in PAIR_ROUTES, op.line()
        replay(op, g, report)
    torch.cuda.empty_cache()
    print(f"\n{config}: {len(ops)} weight-gradient ops, {len(uniq)} geometries replayed in {time.time() - t0:.1f} s; "
          + "; ".join(f"{k}: " + ", ".join(f"{v:.3g}" for v in vs) for k, vs in report.items()))


# ----------------------------------------------------------------------------------------------------- coverage
def _synthetic(route):
    """an emit_wgrad descriptor for a route no census configuration reaches (None: no recipe)"""
    ctx = Ctx(DEV, precision="bf16" if route in ("wgrad_igemm256_kernel", "wgrad_igemm16_kernel") else "fp32")
    cin, cout, k, s, B, H = {"wgrad_igemm256_kernel": (256, 256, 3, 1, 2, 32), "wgrad_igemm16_kernel": (128, 128, 3, 2, 2, 32)}.get(
        route, (64, 128, 3, 2, 2, 32))
    OH = G.conv_out(H, k, s, 1)
    x = Halo(ctx, B, H, H, cin, 1, twin=True)
    zpad = k - 1 if s == 1 else 1
    dy = Halo(ctx, B, OH, OH, cout, zpad, twin=True)
    plan = Plan(ctx)
    d = emit_wgrad(plan, ctx, dy, x, G.conv_fwd_taps(k, cin), G.conv_fwd_pack(cout, cin, k), ctx.zeros(cout, cin, k, k),
                   N=cout, OH=OH, OW=OH, p_oh=zpad, p_ow=zpad, q_stride=s)
    op = Op("wgrad", "synthetic", d)
    return op if op.route == route else None


def _synthetic_pair():
    """a fused data-gradient + weight-gradient launch that the library runs as two launches: the weight gradient of a stride-1 Conv2d(128,
    128, 3) on the three-term split tile (pair_route sends precision 3 to two launches), built as the engine's ConvLayer builds it"""
    ctx = Ctx(DEV)
    B, H, cin, cout, k = 2, 32, 128, 128, 3
    x = Halo(ctx, B, H, H, cin, 1)
    dy = Halo(ctx, B, H, H, cout, k - 1)
    gx = Halo(ctx, B, H, H, cin, 1)
    hw = [(kh, kw) for kh in range(k) for kw in range(k)]
    dspec = G.conv_dgrad_pack(cout, cin, k, hw)
    wd = ctx.zeros(dspec.N, dspec.K)
    cdesc = emit_conv(None, ctx, dy, G.conv_dgrad_s1_taps(k, cout), wd, None, gx, N=cin, OH=gx.hp, OW=gx.wp)
    plan = Plan(ctx)
    d = emit_wgrad(plan, ctx, dy, x, G.conv_fwd_taps(k, cin), G.conv_fwd_pack(cout, cin, k), ctx.zeros(cout, cin, k, k),
                   N=cout, OH=H, OW=H, p_oh=k - 1, p_ow=k - 1, q_stride=1, q_oh=0, q_ow=0, pair_with=cdesc)
    op = Op("pair", "synthetic", d, cdesc)
    return op if op.pair == "(two launches)" else None


def test_census_covers_every_weight_gradient_route():
    """the union of the census (built here if the replay tests have not built it) and of synthetic descriptors for the routes it misses
    covers all seven kernels of WGRAD_KERNEL_NAMES and the three pair routes; the synthetic ones are replayed like the census"""
    routes, pairs = set(), set()
    for name in CONFIGS:
        ops = census(name)
        print(f"\n{name}: {len(ops)} weight-gradient ops")
        for op in ops:
            print(op.line())
            if op.pair is not None:
                pairs.add(op.pair)
            if op.pair in (None, "(two launches)"):
                routes.add(op.route)
    # the YAML default's ragged widths (276 x 276 tiles: OW = 138 and 69, down layers and transposed layers) run on the exact-fp32 tile
    # today: a rewrite that routes them onto the split tile changes this expectation
    ragged = [op for op in census("padding=10") if op.w.OW in (138, 69)]
    assert {op.w.OW for op in ragged} == {138, 69} and all(op.route == "wgrad_igemm_kernel<128>" for op in ragged), [op.line() for op in ragged]
    missing = [r for r in WGRAD_ROUTES if r not in routes]
    g = torch.Generator(device=DEV).manual_seed(18)
    for route in missing:
        op = _synthetic(route)
        assert op is not None, f"no census configuration and no synthetic descriptor reaches {route}"
        print("synthetic" + op.line())
        replay(op, g, {})
        routes.add(op.route)
    if "(two launches)" not in pairs:
        op = _synthetic_pair()
        assert op is not None, "no census configuration and no synthetic descriptor reaches the pair route (two launches)"
        print("synthetic" + op.line())
        replay(op, g, {})
        pairs.add(op.pair)
    assert set(WGRAD_ROUTES) <= routes, set(WGRAD_ROUTES) - routes
    assert set(PAIR_ROUTES) <= pairs, set(PAIR_ROUTES) - pairs
