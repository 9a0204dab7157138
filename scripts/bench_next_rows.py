#!/usr/bin/env python3
"""Timings of the widened rows on one MI355X: forward-only generator throughput (inference path),
image metrics, SatCLIP location encoder, histogram matching.  Event-timed, inputs resident in HBM."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch
from model import networks
from model.satclip.location_encoder import LocationEncoder, get_neural_network, get_positional_encoding
from nirgan_hip.inference import histogram_match, predict_tiled
from utils.calculate_metrics import image_metrics_device

dev = "cuda:0"


def timeit(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


torch.manual_seed(0)
net = networks.define_G(3, 1, 64, "resnet_9blocks", "instance", False, "normal", 0.02).to(dev).eval()
net.data_pad = 10
x = torch.rand(16, 3, 256, 256, device=dev)
for prec in ("fp32", "bf16x3", "bf16"):
    net.precision = prec
    with torch.no_grad():
        ms = timeit(lambda: net(x))
    gf = 98.28 * (276 / 256) ** 2 * 16
    print(f"N1 inference  9-block, pad 10, bs 16 @256^2, {prec:6s}: {ms:7.3f} ms/batch  {16 / ms * 1e3:8.1f} tiles/s  {gf / ms:6.1f} TFLOP/s algorithmic")
# tiled inference of one 4096 x 4096 scene: 512-pixel tiles with 16 pixels of context per side (core 480: 9 x 9 = 81 tiles, 8 per launch)
from nirgan_hip import lib as L
net.precision = "fp32"
net.data_pad = 0
scene = torch.rand(1, 3, 4096, 4096, device=dev)
with torch.no_grad():
    ms = timeit(lambda: predict_tiled(net, scene, tile=512, margin=16, batch=8), reps=3, warm=1)
tiles = torch.empty(8, 3, 512, 512, device=dev)
pred8 = torch.rand(8, 1, 512, 512, device=dev)
outs = torch.empty(1, 1, 4096, 4096, device=dev)
st = torch.cuda.current_stream().cuda_stream
mg = timeit(lambda: L.call("nirgan_tile_gather", scene.data_ptr(), 1, 3, 4096, 4096, 512, 16, 0, 8, tiles.data_ptr(), st), reps=50)
msc = timeit(lambda: L.call("nirgan_tile_scatter", pred8.data_ptr(), 1, 1, 4096, 4096, 512, 16, 0, 8, outs.data_ptr(), st), reps=50)
print(f"N1 tiled scene 4096^2 (81 tiles of 512, margin 16, 8 per launch), 9-block fp32: {ms:8.2f} ms/scene = {4096 * 4096 / ms / 1e3:7.1f} Mpixel/s; "
      f"gather of 8 tiles {mg * 1e3:6.1f} us ({2 * tiles.numel() * 4 / mg / 1e6:6.0f} GB/s), scatter {msc * 1e3:6.1f} us")
# the same scene and model with cross-faded tile overlaps: overlap = core // 4 = 120, stride 360: 12 x 12 = 144 tiles
import ctypes as C
ov = (512 - 2 * 16) // 4
total = int(L.backend().nirgan_tile_count_ov(1, 4096, 4096, 512, 16, ov))
with torch.no_grad():
    msb = timeit(lambda: predict_tiled(net, scene, tile=512, margin=16, batch=8, blend="blend", overlap=ov), reps=3, warm=1)


def blend_pass(entry, channels, scene_buf, tile_buf, window=0):
    """every launch of one scene (8 tiles each, ascending) of one of the two entries, without the model"""
    d = L.TileBlendDesc()
    d.B, d.C, d.H, d.W, d.tile, d.margin, d.overlap, d.window = 1, channels, 4096, 4096, 512, 16, ov, window
    d.scene, d.tiles = scene_buf.data_ptr(), tile_buf.data_ptr()
    for first in range(0, total, 8):
        d.first, d.n = first, min(8, total - first)
        L.call(entry, C.byref(d), st)


mgo = timeit(lambda: blend_pass("nirgan_tile_gather_ov", 3, scene, tiles), reps=20)
mbl = timeit(lambda: blend_pass("nirgan_tile_blend", 1, outs, pred8), reps=20)
mbc = timeit(lambda: blend_pass("nirgan_tile_blend", 1, outs, pred8, window=1), reps=20)
print(f"N1 tiled scene 4096^2 blended ({total} tiles of 512, margin 16, overlap {ov}, 8 per launch), 9-block fp32: {msb:8.2f} ms/scene = "
      f"{4096 * 4096 / msb / 1e3:7.1f} Mpixel/s ({msb / ms:5.3f} x the unblended time, tiles x {total / 81:5.3f}); all {-(-total // 8)} launches of a scene: "
      f"gather_ov {mgo * 1e3:7.1f} us ({2 * total * 3 * 512 * 512 * 4 / mgo / 1e6:6.0f} GB/s), blend linear {mbl * 1e3:7.1f} us, cosine {mbc * 1e3:7.1f} us "
      f"({(total * 480 * 480 + 2 * 4096 * 4096) * 4 / mbl / 1e6:6.0f} GB/s); share of the scene time {(mgo + mbl) / msb * 100:5.2f} %")
a, b = torch.rand(16, 1, 256, 256, device=dev), torch.rand(16, 1, 256, 256, device=dev)
ms = timeit(lambda: image_metrics_device(a, b), reps=50)
print(f"N2 metrics    16 x 256^2 (L1, L2, SSIM-5): {ms * 1e3:7.1f} us  ({2 * a.numel() * 4 / ms / 1e6:6.1f} GB/s of input)")
enc = LocationEncoder(get_positional_encoding("sphericalharmonics", 10, "analytic"), get_neural_network("siren", 100, 256, 512, 2)).double().eval().to(dev)
ll = torch.stack((torch.rand(32, dtype=torch.float64) * 360 - 180, torch.rand(32, dtype=torch.float64) * 180 - 90), -1).to(dev)
ms = timeit(lambda: enc(ll), reps=50)
print(f"N3 location encoder  32 coordinates, L=10 -> 512 -> 512 -> 256, fp64: {ms * 1e3:7.1f} us")
for shape in ((16, 1, 256, 256), (2, 1, 512, 512)):
    img, ref = torch.randn(*shape, device=dev), torch.rand(*shape, device=dev)
    ms = timeit(lambda: histogram_match(img, ref), reps=10)
    print(f"N4 histogram matching {shape}: {ms:7.3f} ms  ({shape[0] / ms * 1e3:7.1f} tiles/s)")
