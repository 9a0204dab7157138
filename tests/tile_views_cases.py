"""Case bodies of the dihedral test-time augmentation (nirgan_tile_views_expand / nirgan_tile_views_merge, predict_tiled(tta=...),
predict_tta), shared by tests/test_tile_views_emulated.py (numpy emulator, CPU) and tests/test_gpu_tile_views.py (MI355X).

The numpy restatement below is written from the header's definition of view g (bit 0 mirrors columns, bit 1 mirrors rows, bit 2
transposes):  view_g(x)[i][j] = x[i'][j'],  (a, b) = (j, i) if bit 2 else (i, j),  i' = H-1-a if bit 1 else a,  j' = W-1-b if bit 0
else b.  Without bit 2 that is np.flip along the mirrored axes; with it, y = those flips of x and view[i][j] = y[j][i], a swapaxes of
y.  The flips are involutions, so the inverse is the swapaxes first and then the same flips.

Bounds.  Expand is a permutation and merge is float32 adds in a stated tree plus one multiply by a power of two: every comparison
with the restatement is BITWISE, there is no tolerance.  The one derived bound is the mirror case's: both sides hold the same eight
terms in two tree orders, a tree of 8 has three levels of additions whose roundings sum to at most 3 * 2^-24 * max|v| after the
division by 8, so the two sides differ by at most 6 * 2^-24 * max|v|.  Where predict_tiled(blend="blend") follows the merge, the blend
keeps its own float64 restatement and bound (tests/tile_blend_cases.py) and is compared bitwise with the blend entry run on the
restated merge.
"""
import ctypes as C

import numpy as np
import torch

import tile_blend_cases as Bc
from nirgan_hip import lib as L
from nirgan_hip.inference import predict_tiled, predict_tta

f32 = np.float32
BLOCK = 64                                                                      # side of the staged block (csrc/tileviews.hip: TV_B)
GUARD = 64
SQUARES = [1, 4, 12, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 4]
RECTS = [(5, 7), (64, 23), (37, 130)]                                           # k <= 4 only
VIEWS = (1, 2, 4, 8)
SHAPE_VIEWS = [((t, t), k) for t in SQUARES for k in VIEWS] + [(hw, k) for hw in RECTS for k in (1, 2, 4)]
CHANNELS, COUNTS = (1, 3), (1, 3)
TTA = {"none": 1, "flip": 2, "flips": 4, "d4": 8}
SCENES = [(1, 3, 13, 29), (2, 3, 37, 50)]
TILINGS = [(16, 2, 4), (12, 3, 3)]                                              # (tile, margin, overlap)
BLENDS = ("none", "blend")
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------------ numpy restatement
def view(x, g):
    """view g of the trailing two axes of x"""
    y = x
    if g & 1:
        y = np.flip(y, -1)
    if g & 2:
        y = np.flip(y, -2)
    if g & 4:
        y = np.swapaxes(y, -1, -2)
    return np.ascontiguousarray(y)


def unview(v, g):
    y = np.swapaxes(v, -1, -2) if g & 4 else v
    if g & 1:
        y = np.flip(y, -1)
    if g & 2:
        y = np.flip(y, -2)
    return np.ascontiguousarray(y)


def expand_np(x, k):
    """[n][C][H][W] -> [n][k][C][H][W], any dtype (bit patterns are moved)"""
    return np.stack([view(x, g) for g in range(k)], axis=1)


def merge_np(v, dtype=f32):
    """[n][k][C][H][W] -> [n][C][H][W]: the pairwise tree ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)) in ``dtype``, then one multiply by 1/k"""
    k = v.shape[1]
    terms = [unview(v[:, g], g).astype(dtype) for g in range(k)]
    while len(terms) > 1:
        terms = [(terms[i] + terms[i + 1]).astype(dtype) for i in range(0, len(terms), 2)]
    return (terms[0] * dtype(1.0 / k)).astype(dtype)


def bits(a):
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ raw entries
def guarded(n, fill, dev, shift):
    """n floats filled with ``fill`` between two NaN guard bands of GUARD floats; shift = 1: a base that is not 16-byte aligned"""
    buf = torch.full((GUARD + shift + n + GUARD,), float("nan"), device=dev)
    assert buf.data_ptr() % 16 == 0
    inner = buf[GUARD + shift:GUARD + shift + n]
    inner.fill_(float(fill))
    return buf, inner


def guards_intact(buf, n, shift):
    lo, hi = buf[:GUARD + shift], buf[GUARD + shift + n:]
    return hi.numel() == GUARD and bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())


def placed(values, dev, shift):
    """a float32 numpy array on the device at an aligned (shift = 0) or shifted address; returns (keep-alive, flat view)"""
    flat = torch.from_numpy(np.ascontiguousarray(values).reshape(-1).view(np.int32).copy())
    buf = torch.zeros(GUARD + shift + flat.numel(), dtype=torch.int32, device=dev)
    buf[GUARD + shift:] = flat.to(dev)                                           # integer copies: NaN payloads stay as they are
    return buf, buf[GUARD + shift:].view(torch.float32)


def views_desc(n, Cc, H, W, k, src, dst):
    d = L.TileViewsDesc()
    d.n, d.C, d.H, d.W, d.views, d.src, d.dst = n, Cc, H, W, k, src.data_ptr(), dst.data_ptr()
    return d


def run_entry(name, dev, values, out_elems, n, Cc, H, W, k, shift, fill):
    """one call of an entry on guarded buffers -> the destination as a numpy array (guards checked)"""
    keep, src = placed(values, dev, shift)
    buf, dst = guarded(out_elems, fill, dev, shift)
    L.check(getattr(L.backend(), name)(C.byref(views_desc(n, Cc, H, W, k, src, dst)), Bc.stream_of(dev)), name)
    out = dst.cpu().numpy().copy()
    assert guards_intact(buf, out_elems, shift), (name, n, Cc, H, W, k, shift)
    assert same_bits(src, np.ascontiguousarray(values).reshape(-1)), "the source was written"
    return out


def rand_values(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(f32)


def nan_values(shape, seed):
    """quiet and signalling NaNs of both signs with random payloads"""
    rng = np.random.default_rng(seed)
    payload = rng.integers(1, 1 << 23, size=shape, dtype=np.uint32)
    sign = rng.integers(0, 2, size=shape, dtype=np.uint32) << np.uint32(31)
    return (np.uint32(0x7F800000) | payload | sign).view(f32)


def shapes_of(hw):
    return [(n, Cc) + tuple(hw) for n in COUNTS for Cc in CHANNELS]


def expand_is_bitwise(dev, hw, k, shift):
    """case 1: dst [n][k][C][H][W] is the restated views bit for bit, NaN payloads included; every element written, guards kept"""
    for n, Cc, H, W in shapes_of(hw):
        for x in (rand_values((n, Cc, H, W), H + W + k), nan_values((n, Cc, H, W), n + Cc)):
            got = run_entry("nirgan_tile_views_expand", dev, x, n * k * Cc * H * W, n, Cc, H, W, k, shift, SENTINEL)
            assert same_bits(got.reshape(n, k, Cc, H, W), expand_np(x, k)), (n, Cc, H, W, k, shift)


def merge_is_bitwise(dev, hw, k, shift):
    """case 2: dst [n][C][H][W] is the float32 tree of the restated inverse views bit for bit; dst starts as NaN and comes out finite"""
    for n, Cc, H, W in shapes_of(hw):
        v = rand_values((n, k, Cc, H, W), 7 * H + W + k)
        got = run_entry("nirgan_tile_views_merge", dev, v, n * Cc * H * W, n, Cc, H, W, k, shift, float("nan"))
        assert np.isfinite(got).all() and same_bits(got.reshape(n, Cc, H, W), merge_np(v)), (n, Cc, H, W, k, shift)


def round_trip_is_bitwise(dev, hw, k, shift):
    """case 3: merge(expand(x)) == x"""
    for n, Cc, H, W in shapes_of(hw):
        x = rand_values((n, Cc, H, W), 3 * H + W + k)
        mid = run_entry("nirgan_tile_views_expand", dev, x, n * k * Cc * H * W, n, Cc, H, W, k, shift, SENTINEL)
        got = run_entry("nirgan_tile_views_merge", dev, mid, n * Cc * H * W, n, Cc, H, W, k, shift, float("nan"))
        assert same_bits(got.reshape(n, Cc, H, W), x), (n, Cc, H, W, k, shift)


# ------------------------------------------------------------------------------------------------ predict_tiled
def run_tiled(model, scene, tiling, blend, tta, batch=20, **kw):
    tile, margin, overlap = tiling
    return predict_tiled(model, scene, tile=tile, margin=margin, batch=batch, blend=blend, overlap=overlap, tta=tta, **kw)


def refused_today(shape, tiling, blend):
    """nirgan_tile_gather reflects once, like F.pad(mode='reflect'): a scene narrower than its reflected border (margin + the round-up
    of the extent to whole cores) is refused, with every ``tta`` as without one.  Only nirgan_tile_gather_ov continues the reflection
    periodically.  Of the cases here that is scene 13 x 29 with tile 16, margin 2 and blend="none" (bottom border 24 - 13 + 2 = 13)."""
    _, _, H, W = shape
    tile, margin, _ = tiling
    core = tile - 2 * margin
    border = [-(-e // core) * core - e + margin for e in (H, W)]
    return blend == "none" and not (margin < H and margin < W and border[0] < H and border[1] < W)


def refusal_is_todays(scene, tiling, blend):
    """such a case stays a case: every ``tta`` is refused by the gather exactly as the plain call is, before the model is called"""
    import pytest
    for tta in TTA:
        rec = Bc.Recorder(Bc.tile_ramp)
        with pytest.raises(RuntimeError, match="reflected border is wider than the scene"):
            run_tiled(rec, scene, tiling, blend, tta)
        assert rec.inputs == []


def todays_placement(dev, merged, shape, tiling, blend):
    """the existing scatter or blend ENTRY on per-tile predictions [count][1][tile][tile] -> scene [B][1][H][W]"""
    B, _, H, W = shape
    tile, margin, overlap = tiling
    be, st = L.backend(), Bc.stream_of(dev)
    tiles = torch.from_numpy(merged).to(dev).contiguous()
    out = torch.full((B, 1, H, W), float("nan"), device=dev)
    if blend == "none":
        L.check(be.nirgan_tile_scatter(tiles.data_ptr(), B, 1, H, W, tile, margin, 0, len(merged), out.data_ptr(), st), "tile_scatter")
    else:
        L.check(be.nirgan_tile_blend(C.byref(Bc.desc(out, tiles, shape, tiling, "linear", 0, len(merged), channels=1)), st), "tile_blend")
    return out.cpu().numpy()


def check_against_recorded(dev, got, rec, seen_plain, shape, tiling, blend, k):
    """the recorded model inputs are the views of the plain run's tiles; ``got`` is merge (float32 restatement) + today's placement of
    the recorded outputs"""
    B, _, H, W = shape
    tile, margin, overlap = tiling
    seen, preds = rec.tiles()
    total = len(seen_plain)
    assert seen.shape == (total * k,) + seen_plain.shape[1:] and preds.shape == (total * k, 1, tile, tile)
    assert same_bits(seen.reshape((total, k) + seen_plain.shape[1:]), expand_np(seen_plain, k))
    merged = merge_np(preds.reshape(total, k, 1, tile, tile))
    ref = Bc.blend64(merged, B, H, W, tile, margin, overlap if blend == "blend" else 0, "linear")
    out = got.cpu().numpy()
    if blend == "none":
        assert same_bits(out, ref.astype(f32))                                    # weights 1: the float64 restatement copies
    else:
        err = np.abs(out.astype(np.float64) - ref).max() / np.abs(merged).max()
        assert err <= Bc.TOL, err
    assert same_bits(out, todays_placement(dev, merged, shape, tiling, blend))


def model_sees_the_right_views(dev, shape, tiling, blend):
    """case 4"""
    scene = Bc.scene_of(shape).to(dev)
    if refused_today(shape, tiling, blend):
        return refusal_is_todays(scene, tiling, blend)
    plain = Bc.Recorder(Bc.tile_ramp)
    run_tiled(plain, scene, tiling, blend, "none")
    seen_plain, _ = plain.tiles()
    assert len(seen_plain) == Bc.count(shape[0], shape[2], shape[3], tiling[0], tiling[1], tiling[2] if blend == "blend" else 0)
    for tta, k in TTA.items():
        if k == 1:
            continue
        rec = Bc.Recorder(Bc.tile_ramp)
        got = run_tiled(rec, scene, tiling, blend, tta)
        assert got.shape == (shape[0], 1, shape[2], shape[3]) and got.dtype == scene.dtype
        assert max(len(x) for x in rec.inputs) <= 20, "batch bounds the model's batch"
        check_against_recorded(dev, got, rec, seen_plain, shape, tiling, blend, k)


def equivariant_model_is_unchanged(dev, shape, tiling, blend):
    """case 5: take0 does not look at the orientation, the k terms of every pixel are equal and their mean is that value exactly"""
    scene = Bc.scene_of(shape).to(dev)
    if refused_today(shape, tiling, blend):
        return refusal_is_todays(scene, tiling, blend)
    plain = run_tiled(Bc.take0, scene, tiling, blend, "none")
    for tta in ("flip", "flips", "d4"):
        assert torch.equal(run_tiled(Bc.take0, scene, tiling, blend, tta), plain), tta


def split_does_not_matter(dev, shape, tiling, blend):
    """case 6"""
    scene = Bc.scene_of(shape).to(dev)
    if refused_today(shape, tiling, blend):
        return refusal_is_todays(scene, tiling, blend)
    runs = [run_tiled(Bc.tile_ramp, scene, tiling, blend, "d4", batch=b) for b in (1, 7, 64)]
    assert torch.equal(runs[1], runs[0]) and torch.equal(runs[2], runs[0])
    assert bool(torch.isfinite(runs[0]).all())


def output_commutes_with_a_mirror(dev):
    """case 7: one square tile that is all core.  tile_ramp is elementwise and depends on the position inside the tile, so its plain
    prediction does not commute with a column mirror; averaged over D4 it does, up to the two tree orders of the same eight terms"""
    t = 16
    scene = Bc.scene_of((1, 3, t, t)).to(dev)
    mirrored = torch.flip(scene, dims=[-1]).contiguous()
    worst = {}
    for tta in ("d4", "none"):
        ra, rb = Bc.Recorder(Bc.tile_ramp), Bc.Recorder(Bc.tile_ramp)
        a = predict_tiled(ra, mirrored, tile=t, margin=0, tta=tta)
        b = torch.flip(predict_tiled(rb, scene, tile=t, margin=0, tta=tta), dims=[-1])
        vmax = max(np.abs(ra.tiles()[1]).max(), np.abs(rb.tiles()[1]).max())
        worst[tta] = float((a - b).abs().max().item()), 6.0 * 2.0 ** -24 * float(vmax)
        print(f"mirror {tta}: |P(mirror x) - mirror P(x)| = {worst[tta][0]:.3e}, bound {worst[tta][1]:.3e}")
    assert worst["d4"][0] <= worst["d4"][1]
    assert worst["none"][0] > worst["none"][1], "the plain prediction has to violate the bound, or the case shows nothing"


def embeds_follow_the_scene(dev):
    """case 8: B = 2, every one of a tile's k views gets the embedding of the scene the tile was cut from"""
    shape, tiling = (2, 3, 37, 50), (16, 2, 4)
    scene = Bc.scene_of(shape)
    embeds = torch.tensor([[0.25, 9.0], [-0.5, 9.0]])
    rows = []

    def model(x, e):
        assert e.shape == (x.shape[0], 2)
        rows.append(e[:, 0].detach().cpu())
        return x[:, :1] + e[:, :1, None, None]
    ref = (scene[:, :1] + embeds[:, 0][:, None, None, None])
    for blend in BLENDS:
        per_image = Bc.count(1, 37, 50, 16, 2, 4 if blend == "blend" else 0)
        for tta, k in TTA.items():
            rows.clear()
            got = run_tiled(model, scene.to(dev), tiling, blend, tta, batch=24, embeds=embeds.to(dev))
            want = embeds[:, 0].repeat_interleave(per_image * k)                  # tile-major, a tile's k views side by side
            assert torch.equal(torch.cat(rows), want), (blend, tta)
            if blend == "none":
                assert torch.equal(got.cpu(), ref), (blend, tta)                  # k equal terms: exactly x + e
            else:
                assert (got.cpu().double() - ref.double()).abs().max().item() <= Bc.TOL * ref.abs().max().item()


def tta_none_is_todays_path(dev, shape, tiling, blend):
    """the default and tta="none" agree bitwise with a call that does not name tta"""
    tile, margin, overlap = tiling
    scene = Bc.scene_of(shape).to(dev)
    if refused_today(shape, tiling, blend):
        return refusal_is_todays(scene, tiling, blend)
    old = predict_tiled(Bc.tile_ramp, scene, tile=tile, margin=margin, batch=3, blend=blend, overlap=overlap)
    assert torch.equal(run_tiled(Bc.tile_ramp, scene, tiling, blend, "none", batch=3), old)


# ------------------------------------------------------------------------------------------------ predict_tta
def whole_tiles(dev, shape, tta):
    """predict_tta: one model call on the B * k views, bitwise the restated merge of what the model answered"""
    k = TTA[tta]
    x = Bc.scene_of(shape)

    def ramp(v):                                                                 # elementwise, position dependent, any extent
        h, w = v.shape[-2:]
        r = torch.arange(h * w, dtype=torch.float32, device=v.device).reshape(1, 1, h, w) / float(h * w)
        return v[:, :1] * (0.5 + r)
    rec = Bc.Recorder(ramp)
    got = predict_tta(rec, x.to(dev), tta=tta)
    assert len(rec.inputs) == 1 and got.shape == (shape[0], 1) + tuple(shape[2:])
    seen, preds = rec.tiles()
    if k == 1:
        assert same_bits(seen, x.numpy()) and same_bits(got, preds)
        return
    assert same_bits(seen.reshape((shape[0], k) + tuple(shape[1:])), expand_np(x.numpy(), k))
    hv, wv = preds.shape[-2:]
    assert same_bits(got, merge_np(preds.reshape(shape[0], k, 1, hv, wv)))


def whole_tiles_with_embeds(dev):
    x = Bc.scene_of((3, 3, 12, 12))
    embeds = torch.tensor([[0.25], [-0.5], [0.125]])
    got = predict_tta(lambda v, e: v[:, :1] + e[:, :1, None, None], x.to(dev), tta="d4", embeds=embeds.to(dev))
    assert torch.equal(got.cpu(), x[:, :1] + embeds[:, 0][:, None, None, None])


# ------------------------------------------------------------------------------------------------ argument errors
def bad_fields():
    """(field, value, word of the message) on a valid 2 x 3 x 12 x 12 descriptor with 8 views"""
    return [("src", None, b"null"), ("dst", None, b"null"), ("views", 0, b"views"), ("views", 3, b"views"), ("views", 16, b"views"),
            ("views", -8, b"views"), ("H", 13, b"square"), ("W", 5, b"square"), ("n", 0, b"shape"), ("n", -1, b"shape"), ("C", 0, b"shape"),
            ("H", 0, b"shape"), ("W", -3, b"shape"), ("n", 1 << 29, b"2^31"), ("C", 1 << 28, b"2^31")]


def valid_desc(buf, k=8):
    d = L.TileViewsDesc()
    d.n, d.C, d.H, d.W, d.views = 2, 3, 12, 12, k
    d.src = d.dst = buf.data_ptr()
    return d


def entries_reject_bad_arguments(be):
    """case 9 through the raw entries of ``be`` (the emulator or the real library: nothing is launched, so no GPU is needed)"""
    buf = torch.zeros(64)
    for entry in ("nirgan_tile_views_expand", "nirgan_tile_views_merge"):
        fn, who = getattr(be, entry), entry[7:].encode()
        d = valid_desc(buf)
        for field, value, word in bad_fields():
            keep = getattr(d, field)
            setattr(d, field, value)
            assert fn(C.byref(d), None) == -1, (entry, field, value)
            msg = be.nirgan_last_error()
            assert who in msg and word in msg, (entry, field, msg)
            setattr(d, field, keep)
        d = valid_desc(buf, k=4)                                                   # a plane of 2^31 elements (flips: no square needed)
        d.H, d.W = 1 << 16, 1 << 15
        assert fn(C.byref(d), None) == -1 and b"2^31" in be.nirgan_last_error() and who in be.nirgan_last_error()
    assert (buf == 0).all()
