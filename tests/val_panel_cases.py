"""Bodies shared by tests/test_val_panel_emulated.py (numpy emulator, CPU) and tests/test_gpu_val_panel.py (MI355X): the
validation-panel entry (nirgan_val_panel, utils.logging_helpers.panel_device) and the figures built on it.

Expected values are stock numpy / torch on the CPU, stating the reference's lines (utils/logging_helpers.py) literally:
``np.histogram(v, bins=100, range=(0, 1))`` of torch's fp32 ``clamp(1.5 * x, 0, 1)``, ``torch.quantile`` in float64 on the float32
values, ``torch.min / max / mean`` in float64 and the numpy NDVI expression in float32.

Bounds:
  histograms            EQUAL, integer for integer; the counts add up to the window size minus its NaNs
  nir_disp / pred_disp  BITWISE equal to torch's fp32 clamp (NaN where torch has NaN)
  min / max             EQUAL as values
  mean                  1e-6 relative to the float64 mean
  rgb_lo / rgb_hi       4 * 2^-24 * max(|a|, |b|) of the float64 torch.quantile, a and b the two neighbouring order statistics: the
                        fp32 rounding of one multiply-add on them.  Where torch.quantile is not finite (an infinite order statistic
                        gives inf - inf = NaN in its lerp) the value has to be the same, NaN included
  NDVI planes           1e-6 absolute against the float32 numpy expression
  rgb_disp              1e-6 absolute against clamp((c - lo) / (hi - lo), 0, 1) in float64 with the ENTRY's own lo / hi; 0 where hi == lo
"""
import math

import numpy as np
import torch

from utils.logging_helpers import PANEL_OUTPUTS, panel_device

EPS24 = 2.0 ** -24
f32 = np.float32

# (B, H, W) -> windows (y0, x0, ch, cw): odd offsets and the full tile.  5 x 5 is smaller than one workgroup's share; 67 x 93 has an
# odd pixel count (the guarded scalar loads) and several blocks per tile; 256^2 with the figure's crop 240 and 532^2 with crop 500
# spread one tile's selection over many workgroups
SHAPES = {(1, 5, 5): [(0, 0, 5, 5), (1, 1, 3, 3)],
          (3, 67, 93): [(0, 0, 67, 93), (3, 5, 41, 57)],
          (2, 64, 64): [(0, 0, 64, 64), (1, 3, 33, 21)],
          (5, 256, 256): [(8, 8, 240, 240), (7, 9, 241, 239)],
          (1, 532, 532): [(16, 16, 500, 500), (0, 0, 532, 532), (15, 17, 501, 499)]}
CASES = [(shape, win) for shape, wins in SHAPES.items() for win in wins]


def inputs(shape, seed=0):
    """rgb in [-0.25, 1.25] (clamping matters, the raw mode sees both signs), nir / pred in [-0.1, 0.9] (x 1.5 leaves [0, 1] on both sides)"""
    B, H, W = shape
    g = torch.Generator().manual_seed(100 + seed)
    rgb = torch.rand(B, 3, H, W, generator=g) * 1.5 - 0.25
    nir = torch.rand(B, 1, H, W, generator=g) - 0.1
    pred = torch.rand(B, 1, H, W, generator=g) - 0.1
    return rgb, nir, pred


def quantile_ref(x, perc):
    """x: 1-D fp32 CPU tensor -> [(float64 torch.quantile, bound)] for q = perc / 100 and (100 - perc) / 100"""
    x64 = x.double()
    s = torch.sort(x64).values
    out = []
    for q in (perc / 100.0, (100.0 - perc) / 100.0):
        ref = torch.quantile(x64, q).item()
        pos = q * (x.numel() - 1)
        a, b = s[math.floor(pos)].item(), s[math.ceil(pos)].item()
        out.append((ref, 4 * EPS24 * max(abs(a), abs(b))))
    return out


def reference(rgb, nir, pred, win, gain=1.5, perc=2.0, clamp_rgb=True):
    y0, x0, ch, cw = win
    B = nir.shape[0]
    sl = (slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
    ref = {}
    for name, t in (("nir_disp", nir), ("pred_disp", pred)):
        ref[name] = (t[:, 0] * gain).clamp(0, 1)[sl]
    ref["hist"] = np.stack([np.stack([np.histogram(ref[k][b].numpy().ravel(), bins=100, range=(0, 1))[0] for k in ("nir_disp", "pred_disp")])
                            for b in range(B)])
    ref["nan_in_window"] = np.stack([[int(torch.isnan(ref[k][b]).sum()) for k in ("nir_disp", "pred_disp")] for b in range(B)])
    st = []
    for t in (nir, pred):
        v = t.double().reshape(B, -1)
        st += [torch.stack([torch.min(v[b]) for b in range(B)]), torch.stack([torch.max(v[b]) for b in range(B)]),
               torch.stack([torch.mean(v[b]) for b in range(B)])]
    ref["stats"] = torch.stack(st, dim=1)
    if rgb is not None:
        c = rgb.clamp(0, 1) if clamp_rgb else rgb
        ref["c"] = c
        ref["quant"] = [quantile_ref(c[b].flatten(), perc) for b in range(B)]
        R = rgb[:, 0].numpy()[sl]
        with np.errstate(all="ignore"):
            for name, t in (("ndvi_nir_disp", nir), ("ndvi_pred_disp", pred)):
                v = t[:, 0].numpy()[sl]
                ndvi = (v - R) / (v + R + 1e-6)
                ndvi = np.clip(ndvi, -1, 1)
                ref[name] = (ndvi + 1) / 2
                assert ref[name].dtype == np.float32
    return ref


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    nan = torch.isnan(b)
    return a.shape == b.shape and torch.equal(torch.isnan(a), nan) and torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


def check_quantile(got, ref, bound, what):
    if not math.isfinite(ref):
        assert got == ref or (got != got and ref != ref), f"{what}: {got!r} against torch.quantile {ref!r}"
        return
    print(f"{what}: {got!r} torch.quantile {ref!r} err {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound, f"{what}: {got!r} against torch.quantile {ref!r}: err {abs(got - ref):.3e} > {bound:.3e}"


def check_panel(got, rgb, nir, pred, win, gain=1.5, perc=2.0, clamp_rgb=True, what=""):
    """every output of ``got`` against ``reference`` under the bounds of the module docstring; prints each figure first"""
    y0, x0, ch, cw = win
    B = nir.shape[0]
    ref = reference(rgb, nir, pred, win, gain, perc, clamp_rgb)
    got = {k: v.detach().cpu() for k, v in got.items()}
    hist = got["hist"].numpy()
    assert hist.dtype == np.int32 and hist.shape == (B, 2, 100)
    assert np.array_equal(hist, ref["hist"]), f"{what}: histogram differs from np.histogram in {int((hist != ref['hist']).sum())} bins"
    assert np.array_equal(hist.sum(axis=2), ch * cw - ref["nan_in_window"]), what
    for k in ("nir_disp", "pred_disp"):
        assert same_bits(got[k], ref[k]), f"{what}: {k} is not bitwise torch's clamp"
    stats = got["stats"].double()
    for j in (0, 1, 3, 4):
        r = ref["stats"][:, j]
        assert (((stats[:, j] == r) | (torch.isnan(stats[:, j]) & torch.isnan(r)))).all(), (what, j, stats[:, j], r)
    for j in (2, 5):
        r = ref["stats"][:, j]
        nan = torch.isnan(r)
        assert torch.equal(torch.isnan(stats[:, j]), nan), (what, j)
        err = ((stats[:, j] - r).abs() / r.abs().clamp(min=1e-30))[~nan]
        if err.numel():
            print(f"{what} mean column {j}: relative err {err.max().item():.3e} bound 1e-6")
            assert (err <= 1e-6).all(), f"{what} mean column {j}: relative err {err.max().item():.3e}"
    if rgb is None:
        assert torch.isnan(stats[:, 6:]).all() and set(got) == {"hist", "stats", "nir_disp", "pred_disp"}
        return
    for b in range(B):
        for j in range(2):
            check_quantile(stats[b, 6 + j].item(), *ref["quant"][b][j], f"{what} tile {b} {'rgb_lo' if j == 0 else 'rgb_hi'}")
    for k in ("ndvi_nir_disp", "ndvi_pred_disp"):
        a, r = got[k].numpy(), ref[k]
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(a), nan), (what, k)
        err = np.abs(a.astype(np.float64) - r.astype(np.float64))[~nan]
        print(f"{what} {k}: err {err.max() if err.size else 0:.3e} bound 1e-6")
        assert (err <= 1e-6).all(), f"{what} {k}: err {err.max():.3e}"
    c = ref["c"][:, :, y0:y0 + ch, x0:x0 + cw].permute(0, 2, 3, 1).double()
    for b in range(B):
        lo, hi = stats[b, 6].item(), stats[b, 7].item()
        a = got["rgb_disp"][b].double()
        if hi == lo:
            assert (a == 0).all(), (what, b)
        elif math.isfinite(lo) and math.isfinite(hi):
            err = (a - ((c[b] - lo) / (hi - lo)).clamp(0, 1)).abs().max().item()
            print(f"{what} tile {b} rgb_disp: err {err:.3e} bound 1e-6")
            assert err <= 1e-6, f"{what} tile {b} rgb_disp: err {err:.3e}"
        elif lo != lo or hi != hi:
            assert torch.isnan(a).all(), (what, b)


def panel_case(dev, case, perc=2.0, clamp_rgb=True):
    shape, win = case
    rgb, nir, pred = inputs(shape, seed=shape[1] + win[0])
    got = panel_device(rgb.to(dev), nir.to(dev), pred.to(dev), crop=win, gain=1.5, perc=perc, clamp_rgb=clamp_rgb)
    assert tuple(got) == PANEL_OUTPUTS and all(v.device.type == torch.device(dev).type for v in got.values())
    check_panel(got, rgb, nir, pred, win, 1.5, perc, clamp_rgb, f"{shape} {win} perc {perc} clamp {clamp_rgb}")
    return got


# ---------------------------------------------------------------------------------------------------------------- histogram edges
def edge_targets():
    """every float32 edge k / 100 of np.histogram's table and its two float32 neighbours"""
    e = np.linspace(0, 1, 101, dtype=f32)
    return np.array([v for k in range(101) for v in (np.nextafter(e[k], f32(-1)), e[k], np.nextafter(e[k], f32(2)))], dtype=f32)


def preimage(t, gain=f32(1.5)):
    """a float32 x with fp32(gain * x) == t, or None where no float32 has that product"""
    x = f32(np.float64(t) / np.float64(gain))
    cands, a, b = [x], x, x
    for _ in range(3):
        a, b = np.nextafter(a, f32(-9)), np.nextafter(b, f32(9))
        cands += [a, b]
    for c in cands:
        if f32(gain * c) == t:
            return c
    lo = max(c for c in cands if f32(gain * c) < t)
    hi = min(c for c in cands if f32(gain * c) > t)
    assert np.nextafter(lo, f32(9)) == hi                    # two CONSECUTIVE floats whose products straddle t: no float32 maps onto it
    return None


def histogram_edges(dev):
    """Planted nir / pred whose stretch lands on the bin edges.

    gain 1.5 (the figure's): for 260 of the 303 targets {edge k / 100 and its two float32 neighbours} a float32 x with
    fp32(1.5 x) == target exists and is planted; for the other 43 (among them the edges 0.05, 0.1 and 0.2 themselves) NO float32 has
    that product -- 1.5 x steps by 1.5 ulp where x and 1.5 x share a binade -- which ``preimage`` proves by exhibiting the two
    consecutive floats whose products straddle the target.  gain 1.0 (second call): x = target, so all 303 are hit.  Both calls also
    carry 0, -0, 1, values above 1 and below 0 and a NaN, and the planted values are checked to hit what they should."""
    tg = edge_targets()
    extra = np.array([0.0, -0.0, 1.0, 1.0000001, 1.5, 7.0, -1e-9, -0.3, np.nan], dtype=f32)
    H, W = 23, 47
    win = (1, 3, 21, 41)
    for gain in (1.5, 1.0):
        xs = [preimage(t, f32(gain)) for t in tg]
        hit = [x is not None for x in xs]
        assert sum(hit) == (260 if gain == 1.5 else 303), sum(hit)
        if gain == 1.5:
            assert all(hit[3 * k] or hit[3 * k + 1] or hit[3 * k + 2] for k in range(101))
        planted = np.concatenate([np.array([x for x in xs if x is not None], dtype=f32), (extra / f32(gain)).astype(f32)])
        rgb, nir, pred = inputs((2, H, W), seed=3)
        g = torch.Generator().manual_seed(8)
        for t, tile in ((nir, 0), (pred, 1)):
            spots = torch.randperm(win[2] * win[3], generator=g)[:planted.size]
            yy, xx = win[0] + spots // win[3], win[1] + spots % win[3]
            t[tile, 0, yy, xx] = torch.from_numpy(planted)
            v = (t[tile, 0, yy, xx] * gain).clamp(0, 1).numpy()                  # the planted values hit their targets
            want = np.clip(np.concatenate([tg[np.array(hit)], extra]), 0, 1)
            assert np.array_equal(v[:-1], want[:-1]) and np.isnan(v[-1]) and np.signbit(v[sum(hit) + 1])
        got = panel_device(rgb.to(dev), nir.to(dev), pred.to(dev), crop=win, gain=gain)
        check_panel(got, rgb, nir, pred, win, gain, what=f"edges gain {gain}")
        hist = got["hist"].cpu().numpy()
        assert hist[0, 0].sum() == win[2] * win[3] - 1 and hist[1, 1].sum() == win[2] * win[3] - 1 and hist[0, 1].sum() == win[2] * win[3]


# ---------------------------------------------------------------------------------------------------------------- order statistics
def adversarial_rgb(H=6, W=7):
    """name -> (rgb tile [3][H][W], perc, clamp_rgb); n = 126 values, so 0.25 (n - 1) = 31.25 and 0.02 (n - 1) = 2.5 are no integers"""
    g = torch.Generator().manual_seed(31)
    n = 3 * H * W
    out = {}
    for perc in (0.0, 2.0, 25.0):
        for clamp in (False, True):
            out[f"random perc {perc} clamp {clamp}"] = (torch.randn(n, generator=g), perc, clamp)
            out[f"sixteenths perc {perc} clamp {clamp}"] = (torch.round(torch.rand(n, generator=g) * 24 - 4) / 16, perc, clamp)
    z = torch.rand(n, generator=g) - 0.5
    z[::5], z[1::5] = 0.0, -0.0
    out["both zeros"] = (z, 25.0, False)
    out["zeros only"] = (torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0)), 25.0, True)
    den = torch.rand(n, generator=g) * 1e-3
    den[::3], den[1::3] = 1e-41, -3e-42
    out["denormals"] = (den, 25.0, False)
    inf = torch.randn(n, generator=g)
    inf[:3], inf[3:6] = float("inf"), float("-inf")
    out["infinities inside the ranks"] = (inf[torch.randperm(n, generator=g)], 25.0, False)
    out["infinities at the ranks"] = (inf[torch.randperm(n, generator=g)], 2.0, False)
    out["infinities clamped"] = (inf[torch.randperm(n, generator=g)], 2.0, True)
    split = torch.cat([-torch.rand(32, generator=g) - 0.1, torch.rand(n - 32, generator=g) + 0.1])
    s = torch.sort(split).values
    assert s[31] < 0 < s[32] and math.floor(0.25 * (n - 1)) == 31 and math.ceil(0.25 * (n - 1)) == 32    # the two ranks differ in the top digit
    out["neighbouring ranks of opposite sign"] = (split[torch.randperm(n, generator=g)], 25.0, False)
    out["all equal"] = (torch.full((n,), 0.375), 2.0, True)
    return {k: (v.reshape(3, H, W).contiguous(), p, c) for k, (v, p, c) in out.items()}


def adversarial_quantiles(dev):
    """every plane as a tile of ONE batch per (perc, clamp_rgb) group, so that neighbours of very different content share a call"""
    planes = adversarial_rgb()
    groups = {}
    for name, (t, perc, clamp) in planes.items():
        groups.setdefault((perc, clamp), []).append((name, t))
    for (perc, clamp), items in groups.items():
        rgb = torch.stack([t for _, t in items])
        _, nir, pred = inputs((len(items), 6, 7), seed=1)
        got = panel_device(rgb.to(dev), nir.to(dev), pred.to(dev), perc=perc, clamp_rgb=clamp, want=("stats", "rgb_disp"))
        stats = got["stats"].cpu().double()
        for b, (name, t) in enumerate(items):
            c = t.clamp(0, 1) if clamp else t
            for j, (ref, bound) in enumerate(quantile_ref(c.flatten(), perc)):
                check_quantile(stats[b, 6 + j].item(), ref, bound, f"{name} [{j}]")
        alone = panel_device(rgb[1:2].to(dev), nir[1:2].to(dev), pred[1:2].to(dev), perc=perc, clamp_rgb=clamp, want=("stats", "rgb_disp"))
        assert same_bits(alone["stats"][0], got["stats"][1]) and same_bits(alone["rgb_disp"][0], got["rgb_disp"][1])


def nan_isolation(dev):
    """a NaN in one tile's rgb, or nir, changes that tile's affected outputs only: every other tile's outputs keep their bits"""
    shape, win = (3, 40, 52), (3, 5, 31, 41)
    rgb, nir, pred = inputs(shape, seed=6)
    clean = panel_device(rgb.to(dev), nir.to(dev), pred.to(dev), crop=win)
    for which in ("rgb", "nir"):
        r, n = rgb.clone(), nir.clone()
        (r if which == "rgb" else n)[1, 0, 20, 30] = float("nan")
        got = panel_device(r.to(dev), n.to(dev), pred.to(dev), crop=win)
        for k in PANEL_OUTPUTS:
            for b in (0, 2):
                assert same_bits(got[k][b].float() if k != "hist" else got[k][b].view(torch.float32),
                                 clean[k][b].float() if k != "hist" else clean[k][b].view(torch.float32)), (which, k, b)
        st = got["stats"][1].cpu()
        if which == "rgb":
            assert torch.isnan(st[6:]).all() and same_bits(st[:6], clean["stats"][1][:6]) and torch.isnan(got["rgb_disp"][1]).all()
            assert torch.equal(got["hist"][1].cpu(), clean["hist"][1].cpu())
        else:
            assert torch.isnan(st[:3]).all() and same_bits(st[3:], clean["stats"][1][3:])
            assert got["hist"][1, 0].sum().item() == win[2] * win[3] - 1 and torch.equal(got["hist"][1, 1].cpu(), clean["hist"][1, 1].cpu())
            assert same_bits(got["rgb_disp"][1], clean["rgb_disp"][1])
        check_panel(got, r, n, pred, win, what=f"NaN in {which}")


def val_stats_case(dev, shape=(3, 40, 52)):
    from utils.logging_helpers import VAL_STATS_KEYS, val_stats_device
    _, nir, pred = inputs(shape, seed=2)
    got = val_stats_device(nir.to(dev), pred.to(dev))
    assert got.shape == (6,) and got.dtype == torch.float32 and len(VAL_STATS_KEYS) == 6
    ref = [torch.min(pred), torch.max(pred), torch.mean(pred.double()), torch.min(nir), torch.max(nir), torch.mean(nir.double())]
    for k, a, r in zip(VAL_STATS_KEYS, got.cpu().tolist(), ref):
        r = float(r)
        print(f"{k}: {a!r} torch {r!r}")
        assert (a == r) if "mean" not in k else abs(a - r) <= 1e-6 * abs(r), (k, a, r)


class NirModel(torch.nn.Module):
    """a stand-in model with the reference's predict_step and a config: what validation_figures needs"""

    def __init__(self, log_ndvi=True):
        super().__init__()
        from types import SimpleNamespace as NS
        self.w = torch.nn.Parameter(torch.tensor([0.5, 0.3, 0.4]))
        self.config = NS(custom_configs=NS(Logging=NS(log_ndvi=log_ndvi, num_val_images=2)))


def image_ok(im, min_h, min_w):
    a = np.asarray(im)
    assert a.ndim == 3 and a.shape[2] == 4 and a.dtype == np.uint8 and a.shape[0] >= min_h and a.shape[1] >= min_w, a.shape
    assert a[..., :3].std() > 0                                                       # something was drawn


def figures_case(dev, size=72, B=6):
    """the three plot functions on device tensors: images of the expected extent (dpi 100 and 50, at most 5 rows)"""
    from utils.logging_helpers import plot_index, plot_tensors, plot_tensors_hist
    rgb, nir, pred = (t.to(dev) for t in inputs((B, size, size), seed=4))
    image_ok(plot_tensors(rgb[:2], nir[:2], pred[:2]), 900, 1400)
    image_ok(plot_tensors_hist(rgb, nir, pred), 480 * min(B, 5), 1900)
    image_ok(plot_index(rgb[:1], nir[:1], pred[:1], index_name="NDVI"), 240, 700)
