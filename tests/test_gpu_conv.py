"""Every convolution launch the shipped nets emit at small shapes -- nirgan_conv_igemm, nirgan_conv_igemm_group and the convolution half of
nirgan_conv_wgrad_pair -- replayed at its exact geometry against the float64 restatement of its descriptor (tests/conv_replay.py).

Census: the engines of a configuration of scripts/plan_signature.py, built on the device by Pix2PixTrainer._prepare (no step runs); every
plan of PLAN_NAMES of G, D2 and D1 is searched and each descriptor is copied.  Replay: the copy is pointed at buffers of its own (the
sizes it declares; the members of a group share what the originals share), must route as the original does, and is launched through the
entry point the plan uses.  A pair's weight-gradient half writes scratch and is not checked here (tests/test_gpu_wgrad.py does).
  * integer pass -- every element of in, w and bias (halos and the channels beyond `run` included) from {-2, -1, 1, 2}; 4 K + 2 < 2^24, so
    every product and partial sum is exact in every precision and split-K order: `out` must be BITWISE the restatement (its nearest-even
    bf16 for a bf16 output), everything outside the written set must still hold the sentinel, and the statistics' and fused sums'
    records are bitwise where every intermediate is an integer below 2^24 (conv_replay.Replay.verify), within the bounds below elsewhere;
  * random pass -- N(0, 1) operands (bf16 values where the buffer holds bf16): (a) every output element within (n + ksplit + 8) 2^-24 scale,
    n = K x the bf16 products per fp32 product of the modelled precision (1, 1, 3, 6), scale = |in| . |w| + |bias| of the modelled terms,
    plus one bf16 ulp of |ref| for a bf16 output; the records within conv_replay.stats_bound / fuse_bound of the same per-element bound;
    (b) on the three split-tile routes max and rms error against float64 at most 2.0 x those of the same problem on the exact-fp32 tile
    (+ 2e-7 / 5e-8: test_gpu_x3.py's bound); (c) a second launch gives the same bits, and the sentinel still holds.
Routes the small shapes cannot reach are replayed on synthetic descriptors (test_census_covers_every_convolution_route)."""
import ctypes as C
import gc
import importlib.util
import os
import time

import pytest
import torch

import conv_replay as R
from nirgan_hip import geometry as G
from nirgan_hip import lib as L
from nirgan_hip.engine import Ctx, Halo, emit_conv
from nirgan_hip.options import OPT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(ROOT, "scripts", "plan_signature.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

CONFIGS = (
    "g6_fp32_2x128_pad0", "g6_fp32_1x256_pad0",            # the default mode; the second reaches the epilogue-sized maps
    "g9_fp32_2x128_pad10", "g9_fp32_1x256_pad10",          # the ragged 148- and 276-wide maps
    "g6_bf16_2x128_pad0", "g6_bf16_1x256_pad0", "g6_bf16x3_2x128_pad0",
    "no_split3_fp32_1x256",                                # exact fp32 everywhere
    "winograd_off_1x256",                                  # the residual 3 x 3 layers as implicit GEMM
    "inject",                                              # the nn.Linear launches
    "rect_fp32_2x128x192",
    "no_epilogue_stats_fp32_1x256", "no_fuse_inbwd_fp32_1x256",
)
PAIR_ROUTES = ("(two launches)", "conv_wgrad_pair256_kernel", "conv_wgrad_pair_kernel")

_CENSUS = {}        # config -> [Launch]
_DONE = set()       # geometries already replayed (by an earlier configuration)
_WORST = {}         # route -> worst fraction of bound (a)


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def routes_of(la):
    """names the launch: la.names (each problem alone, nirgan_conv_kernel_name), la.pair (nirgan_conv_wgrad_pair_kernel_name) and la.route =
    (kernel the convolution runs on, epilogue form, single | group | pair)"""
    be = L.backend()
    la.names = [(be.nirgan_conv_kernel_name(C.byref(d)) or b"(refused)").decode() for d in la.ds]
    la.pair = be.nirgan_conv_wgrad_pair_kernel_name(C.byref(la.ds[0]), C.byref(la.w)).decode() if la.kind == "pair" else None
    if la.kind == "group":
        kernel = R.group_route(la.ds, la.names, cus())
    elif la.kind == "pair" and la.pair != "(two launches)":
        kernel = la.pair
    else:
        kernel = la.names[0]
        # (the restatement of the group's routing, checked where the library answers: a launch of one problem)
        assert kernel == "conv_igemm256_kernel" or R.group_route(la.ds, la.names, cus()) == kernel, (kernel, la.line())
    la.route = (kernel, R.launch_form(la.ds), la.kind)
    return la


def census(name):
    """the convolution launches of configuration `name`, routed while the engines' buffers are alive (built once per session)"""
    if name not in _CENSUS:
        engines = keep = None
        try:
            engines, keep = R.build_engines(P, P.CONFIGS[name], DEV)
            _CENSUS[name] = [routes_of(la) for la in R.launches_of(engines, P.PLAN_NAMES)]
        finally:
            OPT.reset()
        del engines, keep
        gc.collect()
        torch.cuda.empty_cache()
        assert _CENSUS[name], f"{name}: no convolution launch in the plans"
    return _CENSUS[name]


def gpu_bound(d, ref, scale):
    """(a): gamma_n |in| . |w| with n = the bf16 products summed in fp32 per output element, the split-K partial sums and slack for the
    products the split forms drop (test_gpu_wgrad.py's form)"""
    n = d.ntaps * d.run * R.PRODUCTS_PER_FP32[R.modelled_precision(d)]
    return (n + max(d.ksplit, 1) + 8) * 2.0 ** -24 * scale


def launch(r: R.Replay):
    la = r.launch
    ds = [f.d for f in r.members]
    r.arm()
    if la.kind == "single":
        L.call("nirgan_conv_igemm", C.byref(ds[0]), None)
    elif la.kind == "group":
        arr = (C.POINTER(L.ConvDesc) * len(ds))(*[C.pointer(d) for d in ds])
        L.call("nirgan_conv_igemm_group", arr, len(ds), None)
    else:
        L.call("nirgan_conv_wgrad_pair", C.byref(ds[0]), C.byref(r.fw.d), None)
    torch.cuda.synchronize()


def _err(got, ref):
    e = (got.double() - ref).abs()
    s = ref.abs().max().item()
    return e.max().item() / s, e.pow(2).mean().sqrt().item() / s


def exact_tile_problems(f: R.FreshConv):
    """the problem of member f as descriptors of precision 0 without the epilogue's sums (what the split tile is compared with): itself; with
    out_span = 2 over pixel pairs (out_cs == N) one pixel of N channels; with out_span = 2 over dense pixels one problem per pixel of the
    row -- its half of the weight rows and of the bias, the output window one pixel to the right"""
    d = f.d
    span, ch, K = R.span_of(d), R.channels_of(d), d.ntaps * d.run
    out = []
    for q in range(span if d.out_cs != d.N else 1):
        e = R.copy_desc(d)
        e.precision, e.out_span, e.w_x3, e.w_x3_plane, e.algo = 0, 0, None, 0, 0
        e.stats_ws, e.fuse_y, e.fuse_mean, e.fuse_rstd, e.fuse_part = None, None, None, None, None
        if span == 2 and d.out_cs != d.N:
            e.N, e.out_ow = ch, d.out_ow + q
            e.w, e.w_elems = f.w.data_ptr() + 4 * q * ch * K, ch * K
            e.bias = f.bias.data_ptr() + 4 * q * ch if f.bias is not None else None
        out.append(e)
    return out


def replay(la, g: torch.Generator, report: dict):
    """the integer and the random pass of one launch; report collects the worst fractions per route"""
    r = R.Replay(la, DEV)
    be = L.backend()
    tag = f"{la.line()} -> {la.route}"
    # the copy routes as the original does
    assert [(be.nirgan_conv_kernel_name(C.byref(f.d)) or b"(refused)").decode() for f in r.members] == la.names, tag
    if la.kind == "pair":
        assert be.nirgan_conv_wgrad_pair_kernel_name(C.byref(r.members[0].d), C.byref(r.fw.d)).decode() == la.pair, tag
    assert all(4 * d.ntaps * d.run + 2 < 2 ** 24 for d in la.ds)
    # -- integer pass: bitwise
    r.fill(True, g)
    launch(r)
    r.verify(True, gpu_bound, "integer pass; " + tag)
    # -- random pass: (c) two launches, the second one checked
    r.fill(False, g)
    launch(r)
    first = r.snapshot()
    launch(r)
    assert all(torch.equal(a, b) for a, b in zip(first, r.snapshot())), f"(c) a second launch differs; {tag}"
    worst = r.verify(False, gpu_bound, "random pass; " + tag)
    rep = report.setdefault(la.route[0], {"out": 0.0, "stats": 0.0, "fused": 0.0})
    for k, v in worst.items():
        rep[k] = max(rep[k], v)
    _WORST[la.route[0]] = max(_WORST.get(la.route[0], 0.0), worst["out"])
    if la.route[0] in R.X3_ROUTES:
        # (b) against the exact-fp32 tile on the same problem and operands
        exacts = [R.restate_conv(f.d, f.inp, f.w, f.bias, 0, kinds=("value",))[1][0] for f in r.members]
        e3s = [_err(f.out[ref["off"]], exact) for f, ref, exact in zip(r.members, r.reference(), exacts)]
        r.arm()
        for f, ref, exact, e3 in zip(r.members, r.reference(), exacts, e3s):
            assert ref["prec"] == 3, tag
            for e in exact_tile_problems(f):
                assert be.nirgan_conv_kernel_name(C.byref(e)).decode().startswith("conv_igemm_kernel<"), tag
                L.call("nirgan_conv_igemm", C.byref(e), None)
            torch.cuda.synchronize()
            e0 = _err(f.out[ref["off"]], exact)
            assert e3[0] <= 2.0 * e0[0] + 2e-7 and e3[1] <= 2.0 * e0[1] + 5e-8, f"(b) split tile vs exact tile (max, rms): {e3} vs {e0}; {tag}"
            rb = report.setdefault("(b) " + la.route[0], {"max": 0.0, "rms": 0.0})
            rb["max"], rb["rms"] = max(rb["max"], e3[0] / max(e0[0], 1e-300)), max(rb["rms"], e3[1] / max(e0[1], 1e-300))
    del r


def _unique(launches, done):
    out = []
    for la in launches:
        k = la.geometry()
        if k not in done:
            done.add(k)
            out.append(la)
    return out


def _report(report):
    return "; ".join(f"{k}: " + ", ".join(f"{n} {v:.3g}" for n, v in vs.items() if v) for k, vs in report.items())


@pytest.mark.parametrize("config", CONFIGS)
def test_every_convolution_launch_replays_against_float64(config):
    t0 = time.time()
    las = census(config)
    todo = _unique(las, _DONE)
    g = torch.Generator(device=DEV).manual_seed(23)
    report = {}
    for la in todo:
        assert la.route[0] in R.CONV_KERNEL_NAMES + PAIR_ROUTES[1:], la.line()
        replay(la, g, report)
    torch.cuda.empty_cache()
    print(f"\n{config}: {len(las)} convolution launches, {len(_unique(las, set()))} distinct geometries, {len(todo)} not replayed before, "
          f"routes {sorted({la.route for la in las})}, {time.time() - t0:.1f} s; worst fractions of the bounds: {_report(report)}")


# ----------------------------------------------------------------------------------------------------- coverage
def _first_OH(d, want) -> int:
    """the smallest OH (the buffers are those of a larger one) at which the library routes d to `want`"""
    e = R.copy_desc(d)
    for oh in range(1, d.OH + 1):
        e.OH = oh
        if d.stats_ws or d.fuse_y:
            if (oh * d.OW) % 128:
                continue
            e.stats_chunks, e.fuse_chunks = oh * d.OW // 64, oh * d.OW // 128
        name = L.backend().nirgan_conv_kernel_name(C.byref(e))
        if name and name.decode() == want:
            return oh
    return 0


def _synthetic(kernel, form, OH=None):
    """A 3 x 3 stride-1 Conv2d built with emit_conv on the smallest map (B = 1, 128 pixels wide, as many rows as it takes) that the library
    routes to `kernel` on this device's CUs (None: no recipe): the register-fed tile wants 128-column tiles on three quarters of the
    CUs, three K-tiles and 24 with the fused pass (cin = 32 / 96); the eight-wave split tile of 128 columns is what a fused pass with
    fewer K-tiles takes at that size; the 256-wide tile wants bf16 operands, N = 256, 64-channel slices and rounds 62 % full."""
    recipes = {(R.X3R, "plain"): (32, 128, "fp32"), (R.X3R, "stats"): (32, 128, "fp32"), (R.X3R, "fused"): (96, 128, "fp32"),
               ("conv_x3_kernel<128>", "fused"): (32, 128, "fp32"), ("conv_igemm256_kernel", "plain"): (64, 256, "bf16")}
    if (kernel, form) not in recipes:
        return None
    cin, cout, prec = recipes[(kernel, form)]
    B, W, k = 1, 128, 3
    H = OH or max(8 * cus(), 512)          # (rows enough for either threshold: 3/4 of the CUs in 256 x 128 tiles, 159 tiles of 256 x 256)
    ctx = Ctx(DEV, precision=prec)
    x = Halo(ctx, B, H, W, cin, 1, twin=(prec == "bf16"))
    y = Halo(ctx, B, H, W, cout, 0)
    K = k * k * cin
    if prec == "bf16":
        w = torch.zeros(cout, K, dtype=torch.bfloat16, device=DEV)
    else:
        w = ctx.zeros(cout, K)
        w.x3 = (torch.zeros(3 * cout * K, dtype=torch.bfloat16, device=DEV), cout * K)
    bias = ctx.zeros(cout) if form != "fused" else None
    d = emit_conv(None, ctx, x, G.conv_fwd_taps(k, cin), w, bias, y, N=cout, OH=H, OW=W, allow_split=False)
    keep = [ctx, x, y, w, bias]
    if form == "stats":
        ws = torch.zeros(B * (H * W // 64) * 4 * cout, device=DEV)
        d.stats_ws, d.stats_ws_elems, d.stats_chunk0, d.stats_chunks = ws.data_ptr(), ws.numel(), 0, H * W // 64
        keep.append(ws)
    if form == "fused":
        fy, fm, fr = torch.zeros(B * H * W * cout, device=DEV), torch.zeros(B * cout, device=DEV), torch.zeros(B * cout, device=DEV)
        part = torch.zeros(B * (H * W // 128) * 2 * cout, device=DEV)
        d.fuse_y, d.fuse_mean, d.fuse_rstd, d.fuse_h, d.fuse_w = fy.data_ptr(), fm.data_ptr(), fr.data_ptr(), H, W
        d.fuse_act, d.fuse_slope = (1, 0.0) if kernel == R.X3R else (2, 0.2)        # ReLU (its integer pass is bitwise) / LeakyReLU
        d.fuse_part, d.fuse_part_elems, d.fuse_chunk0, d.fuse_chunks = part.data_ptr(), part.numel(), 0, H * W // 128
        keep += [fy, fm, fr, part]
    if OH is None:
        oh = _first_OH(d, kernel)
        del keep
        return _synthetic(kernel, form, oh) if oh else None
    la = routes_of(R.Launch("single", "synthetic", [d]))
    del keep
    return la if la.route[:2] == (kernel, form) else None


def test_census_covers_every_convolution_route():
    """the union over the configurations of (kernel, epilogue form, single | group | pair), completed by synthetic descriptors for what the
    small shapes cannot reach: all six kernels of CONV_KERNEL_NAMES, and the register-fed tile in its three forms (the kernel-level
    assertion that its stats and fused forms are the ones measured); the synthetic ones are replayed like the census"""
    routes = {}
    for name in CONFIGS:
        for la in census(name):
            routes.setdefault(la.route, f"census ({name})")
    want = [(k, None) for k in R.CONV_KERNEL_NAMES] + [(R.X3R, form) for form in R.X3R_FORMS]
    g = torch.Generator(device=DEV).manual_seed(24)
    report = {}
    for kernel, form in want:
        if any(r[0] == kernel and form in (None, r[1]) for r in routes):
            continue
        t0 = time.time()
        la = _synthetic(kernel, form or ("fused" if kernel == "conv_x3_kernel<128>" else "plain"))
        assert la is not None, f"no census configuration and no synthetic descriptor reaches {kernel} {form or ''}"
        replay(la, g, report)
        routes[la.route] = f"synthetic ({la.line()}; {time.time() - t0:.1f} s)"
        torch.cuda.empty_cache()
    print(f"\n{cus()} CUs; convolution routes (kernel, epilogue form, launcher):")
    for r in sorted(routes):
        print(f"  {r[0]:28s} {R.X3R_FORMS[r[1]] if r[0] == R.X3R else r[1]:12s} {r[2]:7s} {routes[r]}")
    print("worst fractions of the bounds on the synthetic descriptors: " + _report(report))
    print("worst fraction of bound (a) per route so far: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_WORST.items())))
    kernels = {r[0] for r in routes}
    assert set(R.CONV_KERNEL_NAMES) <= kernels, set(R.CONV_KERNEL_NAMES) - kernels
    forms = {r[1] for r in routes if r[0] == R.X3R}
    assert forms == set(R.X3R_FORMS), set(R.X3R_FORMS) - forms
