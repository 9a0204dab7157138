"""The float64 restatement of the weight-gradient descriptor (tests/wgrad_replay.py) against the numpy emulator's nirgan_wgrad_igemm on
descriptors the engine emits (emit_wgrad, emit_wgrad_pixel_pairs) and on a plane batch of the Winograd form, and a negative control: a
window off by one pixel changes the restatement, so the bitwise replay of tests/test_gpu_wgrad.py would notice it.  No GPU."""
import pytest
import torch

import wgrad_replay as R
from emu_backend import EmuBackend
from nirgan_hip import geometry as G
from nirgan_hip import lib as L
from nirgan_hip.engine import Ctx, Halo, Plan, emit_wgrad, emit_wgrad_pixel_pairs
from nirgan_hip.options import OPT


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


def _descs(plan):
    return [a[0]._obj for n, a in plan.ops if n == "nirgan_wgrad_igemm"]


def conv_case(ctx, B, H, W, cin, cout, k, s, pad, extra=0):
    """Conv2d(cin, cout, k, s, pad) as the engine's ConvLayer emits it: p = dY in a halo of k - 1 (or 1), q = X in a halo of pad + extra"""
    OH, OW = G.conv_out(H, k, s, pad), G.conv_out(W, k, s, pad)
    x = Halo(ctx, B, H, W, cin, pad + extra, twin=True)
    zpad = k - 1 if s == 1 else 1
    dy = Halo(ctx, B, OH, OW, cout, zpad, twin=True)
    plan = Plan(ctx)
    emit_wgrad(plan, ctx, dy, x, G.conv_fwd_taps(k, cin), G.conv_fwd_pack(cout, cin, k), ctx.zeros(cout, cin, k, k),
               N=cout, OH=OH, OW=OW, p_oh=zpad, p_ow=zpad, q_stride=s, q_oh=extra, q_ow=extra)
    return _descs(plan)[0]


def convT_case(ctx, B, H, W, cin, cout, k, p):
    """ConvTranspose2d(cin, cout, k, 2, p, output_padding 1): p = X (rows = input channels), q = dY gathered with stride 2"""
    x = Halo(ctx, B, H, W, cin, 1, twin=True)
    dy = Halo(ctx, B, 2 * H, 2 * W, cout, 1, twin=True)
    plan = Plan(ctx)
    emit_wgrad(plan, ctx, x, dy, G.convT_dgrad_taps(k, cout), G.convT_dgrad_pack(cin, cout, k), ctx.zeros(cin, cout, k, k),
               N=cin, OH=H, OW=W, p_oh=x.pad, p_ow=x.pad, q_stride=2, q_oh=dy.pad - p, q_ow=dy.pad - p)
    return _descs(plan)[0]


def rowpacked_case(ctx, B, H, W, cin, cout, k, pad, cs=4):
    """the first 7 x 7 layer: one tap per kernel row, a run of k * cs floats crossing k pixels"""
    x = Halo(ctx, B, H, W, cs, pad + 1)
    dy = Halo(ctx, B, H, W, cout, 0)
    plan = Plan(ctx)
    emit_wgrad(plan, ctx, dy, x, G.conv_rowpacked_taps(k, cs), G.conv_rowpacked_pack(cout, cin, k, cs), ctx.zeros(cout, cin, k, k),
               N=cout, OH=H, OW=W, p_oh=0, p_ow=0, q_stride=1, q_oh=1, q_ow=1)
    return _descs(plan)[0]


def pixel_pair_case(ctx, B, H, W):
    """the same layer on the split tile, two adjacent output pixels per GEMM row (engine.emit_wgrad_pixel_pairs)"""
    x = Halo(ctx, B, H, W, 4, 5)          # (halo 5 for a kernel of 7: q_oh 2, q_ow 1 pixel pair)
    dy = Halo(ctx, B, H, W, 64, 0)
    plan = Plan(ctx)
    assert emit_wgrad_pixel_pairs(plan, ctx, dy, x, ctx.zeros(64, 3, 7, 7), k=7, p=3, cin=3, cout=64, OH=H, OW=W)
    return _descs(plan)[0]


def planes_case(ctx, NP, T, K, Cc, nsplit):
    """the transform-domain weight gradient of a Winograd layer: NP planes of dU[f] = Yt[f]^T V[f] (engine.emit_wino6_backward)"""
    d = L.WgradDesc()
    d.p_elems, d.p_hp, d.p_wp, d.p_cs, d.p_oh, d.p_ow = NP * T * K, 1, T, K, 0, 0
    d.q_elems, d.q_hp, d.q_wp, d.q_cs = NP * T * Cc, 1, T, Cc
    d.q_stride, d.q_oh, d.q_ow, d.run, d.ntaps = 1, 0, 0, Cc, 1
    d.B, d.OH, d.OW, d.N = 1, 1, T, K
    d.nsplit, d.rows_per_split = nsplit, -(-(-(-T // nsplit)) // 32) * 32
    d.slab_elems = NP * nsplit * K * Cc
    d.nplanes, d.p_plane, d.q_plane = NP, T * K, T * Cc
    return d


def cases(monkeypatch):
    """(name, descriptor) over the emulator; each builds its own context"""
    monkeypatch.setattr(OPT, "split3", True)
    fp = Ctx("cpu")
    out = [
        ("conv s1, p_oh 2", conv_case(fp, 2, 9, 11, 16, 32, 3, 1, 1)),
        ("conv s2, q_oh 1", conv_case(fp, 3, 13, 10, 8, 24, 3, 2, 1, extra=1)),
        ("conv 4x4 s2, N 128 (split tile)", conv_case(fp, 2, 64, 64, 8, 128, 4, 2, 1)),
        ("convT s2", convT_case(fp, 2, 7, 6, 24, 16, 3, 1)),
        ("row-packed 7x7", rowpacked_case(fp, 1, 10, 12, 3, 16, 7, 3)),
        ("pixel pairs", pixel_pair_case(fp, 1, 8, 64)),
        ("planes", planes_case(fp, 3, 50, 16, 8, 2)),
    ]
    for prec in ("bf16", "bf16x3"):
        ctx = Ctx("cpu", precision=prec)
        out.append((f"conv s1 {prec}", conv_case(ctx, 2, 10, 9, 72, 80, 3, 1, 1)))
    out.append(("convT s2 bf16", convT_case(Ctx("cpu", precision="bf16"), 1, 9, 8, 80, 72, 3, 1)))
    return out


def _fill(t: torch.Tensor, integers: bool, g: torch.Generator):
    if integers:
        v = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (t.numel(),), generator=g)]
    else:
        v = torch.randn(t.numel(), generator=g)
    t.copy_(v.to(t.dtype))


def test_restatement_equals_the_emulator(emu, monkeypatch):
    g = torch.Generator().manual_seed(5)
    seen = set()
    for name, d in cases(monkeypatch):
        M = d.B * d.OH * d.OW
        seen.update({"q_stride 2"} if d.q_stride == 2 else set())
        seen.update({"p_oh"} if d.p_oh else set())
        seen.update({"q_oh"} if d.q_oh else set())
        seen.update({"run > q_cs"} if d.run > d.q_cs else set())
        seen.update({"pixel pairs"} if d.N == 2 * 64 and d.run == 32 and d.precision == 3 else set())
        seen.update({"planes"} if d.nplanes > 1 else set())
        seen.update({"bf16 twins"} if d.pq_bf16 else set())
        seen.update({"ragged split"} if M % d.rows_per_split else set())
        seen.update({f"precision {d.precision}"})
        for integers in (True, False):
            f = R.FreshWgrad(d, "cpu")
            _fill(f.p, integers, g)
            _fill(f.q, integers, g)
            f.arm()
            assert emu.nirgan_wgrad_igemm(f.d) == 0, (name, emu.nirgan_last_error())
            got = f.written().double()
            ref = R.restate(f.d, f.p, f.q, precision=d.precision)
            assert f.untouched_tail(), name
            if integers:
                assert torch.equal(got, ref), name
            else:
                # (the emulator contracts in float64 too, in another order, then rounds to fp32)
                scale = R.restate(f.d, f.p, f.q, precision=d.precision, absolute=True)
                assert ((got - ref).abs() <= 2.0 ** -24 * ref.abs() + 2.0 ** -40 * scale).all(), name
    want = {"q_stride 2", "p_oh", "q_oh", "run > q_cs", "pixel pairs", "planes", "bf16 twins", "ragged split",
            "precision 0", "precision 1", "precision 2", "precision 3"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("field,delta", [("p_oh", 1), ("p_ow", -1), ("q_oh", -1), ("q_ow", 1)])
def test_a_window_off_by_one_changes_the_restatement(emu, field, delta):
    """negative control of the bitwise replay: on integer data (halos included) the restatement of a descriptor whose P or Q window moved
    by one pixel differs from the unshifted one in most slab elements"""
    ctx = Ctx("cpu")
    d = conv_case(ctx, 2, 12, 12, 8, 16, 3, 1, 1, extra=1)
    assert d.p_oh == d.p_ow == 2 and d.q_oh == d.q_ow == 1
    g = torch.Generator().manual_seed(6)
    f = R.FreshWgrad(d, "cpu")
    _fill(f.p, True, g)
    _fill(f.q, True, g)
    ref = R.restate(f.d, f.p, f.q)
    moved = R.copy_desc(f.d)
    setattr(moved, field, getattr(moved, field) + delta)
    # (the moved window stays inside the buffers: the library would accept the descriptor)
    assert moved.p_oh + moved.OH <= moved.p_hp and moved.p_ow + moved.OW <= moved.p_wp and min(moved.p_oh, moved.p_ow, moved.q_oh, moved.q_ow) >= 0
    assert (moved.OH - 1) * moved.q_stride + moved.q_oh + 2 < moved.q_hp and (moved.OW - 1) * moved.q_stride + moved.q_ow + 2 < moved.q_wp
    other = R.restate(moved, f.p, f.q)
    assert (other != ref).double().mean() > 0.5
