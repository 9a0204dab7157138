"""The pixel discriminator (netD 'pixel') without a GPU: the host logic on the numpy statement of the nirgan_pixdisc_* entries
(tests/emu_pixel_disc.py) against stock torch.nn in float64, the argument checks of the real library, a two-rank gloo run and the
metadata of the cross-compiled kernels.  Bodies shared with tests/test_gpu_pixel_disc.py (tests/pixel_disc_cases.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pixel_disc_cases as Pc
from emu_pixel_disc import EmuPixelDisc
from nirgan_hip import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def emu():
    be = EmuPixelDisc()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "f11_pixel_d.npz"))


def test_state_dict_keys_and_seeded_weights_are_the_references(golden):
    Pc.state_dict_and_seed(golden)


def test_golden_forward(emu, golden):
    Pc.golden_forward(golden, "cpu")


@pytest.mark.parametrize("wset", [1, 2])
@pytest.mark.parametrize("shape", Pc.SMALL, ids=str)
def test_engine_forward_params_input_pred_against_float64(emu, shape, wset):
    Pc.engine_level(shape, wset, "cpu")
    assert emu.calls.count("pixdisc_fwd") == 1 and [c for c in emu.calls if isinstance(c, tuple)] == [("pixdisc_bwd", 0), ("pixdisc_bwd", 1), ("pixdisc_bwd", 2)]


@pytest.mark.parametrize("shape", [(1, 5, 5), (2, 7, 9)], ids=str)
def test_module_autograd_route_against_float64(emu, shape):
    Pc.autograd_route(shape, 2, "cpu")


def test_large_mean_forward(emu):
    Pc.large_mean_forward((1, 5, 5), "cpu")


def test_lightning_sequence_and_train_batch_agree_over_five_steps(emu):
    Pc.routes_agree("cpu")
    assert "pixdisc_fwd" in emu.calls and ("pixdisc_bwd", 0) in emu.calls and ("pixdisc_bwd", 2) in emu.calls


@pytest.mark.parametrize("mode", ["lsgan", "vanilla", "wgangp"])
def test_fused_step_losses_against_float64(emu, mode):
    Pc.fused_losses_against_float64("cpu", mode)


def test_fit_history_checkpoint_resume(emu, tmp_path):
    Pc.fit_checkpoint_resume("cpu", tmp_path)


def test_emulator_enforces_the_contract(emu):
    m, flat, eng = Pc.make_engine(2, (2, 7, 9), "cpu")
    n = int(emu.nirgan_pixdisc_ws_elems(2, 7, 9, 64))
    x, stats, out, ws = torch.zeros(2, 7, 9, 4), torch.zeros(2, 128, 2), torch.zeros(2, 7, 9), torch.zeros(n)
    d = L.PixDiscDesc()
    d.x, d.B, d.H, d.W, d.ndf, d.params, d.stats, d.out = x.data_ptr(), 2, 7, 9, 64, flat.flat.data_ptr(), stats.data_ptr(), out.data_ptr()
    d.ws, d.ws_elems = ws.data_ptr(), n - 1
    assert emu.nirgan_pixdisc_fwd(C.byref(d)) == -1 and b"workspace" in emu.nirgan_last_error()
    d.ws_elems = n
    assert emu.nirgan_pixdisc_fwd(C.byref(d)) == 0
    d.dout, d.grads, d.mode = out.data_ptr(), flat.grad.data_ptr(), 3
    assert emu.nirgan_pixdisc_bwd(C.byref(d)) == -1 and b"mode" in emu.nirgan_last_error()
    flat.grad.fill_(Pc.SENT)
    d.mode = L.PIXDISC_PARAMS
    assert emu.nirgan_pixdisc_bwd(C.byref(d)) == 0
    g = flat.grad_views()
    assert (g["net.2.bias"] == 0).all() and (flat.grad[8769:] == 0).all() and (flat.grad != Pc.SENT).all()
    d.H, d.W = 1, 1
    assert emu.nirgan_pixdisc_fwd(C.byref(d)) == -1 and b"shape" in emu.nirgan_last_error()


def test_real_library_rejects_bad_descriptors_before_any_launch():
    be = L.backend()
    assert not L.is_emulated()
    d = L.PixDiscDesc()
    assert be.nirgan_pixdisc_fwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"null" in be.nirgan_last_error()
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"null" in be.nirgan_last_error()
    buf = torch.zeros(1 << 16)
    d.x = d.params = d.stats = d.out = d.dout = d.grads = d.gx = d.ws = buf.data_ptr()
    d.B, d.H, d.W, d.ndf, d.ws_elems = 1, 5, 5, 32, 1 << 30
    assert be.nirgan_pixdisc_fwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"ndf" in be.nirgan_last_error()
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"ndf" in be.nirgan_last_error()
    d.ndf = 64
    for shape in ((1, 1, 1), (1, 5, 0), (0, 5, 5), (1 << 12, 1 << 10, 1 << 9)):
        d.B, d.H, d.W = shape
        assert be.nirgan_pixdisc_fwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"shape" in be.nirgan_last_error(), shape
        assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"shape" in be.nirgan_last_error(), shape
        assert be.nirgan_pixdisc_ws_elems(*shape, 64) == 0
    d.B, d.H, d.W, d.ws_elems = 1, 5, 5, 10
    assert be.nirgan_pixdisc_fwd(d, None) == -1 and b"workspace" in be.nirgan_last_error()
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"workspace" in be.nirgan_last_error()
    d.ws_elems, d.mode = 1 << 30, 3
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"pixdisc" in be.nirgan_last_error() and b"mode" in be.nirgan_last_error()
    d.mode, d.grads = L.PIXDISC_PARAMS, None
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"null" in be.nirgan_last_error()
    d.mode, d.grads, d.gx = L.PIXDISC_PRED, buf.data_ptr(), None
    assert be.nirgan_pixdisc_bwd(d, None) == -1 and b"null" in be.nirgan_last_error()
    assert be.nirgan_pixdisc_ws_elems(1, 5, 5, 32) == 0 and (buf == 0).all()
    # the workspace is a function of the shape only and stays small: records, nothing per pixel
    n = be.nirgan_pixdisc_ws_elems(32, 256, 256, 64)
    assert 0 < n and n * 4 < 16e6
    emu = EmuPixelDisc()
    for args in [(32, 256, 256, 64), (1, 1, 2, 64), (1, 5, 5, 64), (3, 67, 93, 64), (40, 3, 3, 64), (8, 256, 256, 64)]:
        assert emu.nirgan_pixdisc_ws_elems(*args) == be.nirgan_pixdisc_ws_elems(*args) > 0, args


def test_descriptor_layout_matches_the_header(tmp_path):
    """the ctypes mirror has exactly the C layout: sizeof and the offset of the last field, computed by gcc"""
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
                 'printf("%zu %zu %d %d %d %d\\n", sizeof(nirgan_pixdisc_desc), offsetof(nirgan_pixdisc_desc, ws_elems), NIRGAN_PIXDISC_PARAMS,'
                 ' NIRGAN_PIXDISC_INPUT, NIRGAN_PIXDISC_PRED, NIRGAN_PIXDISC_TILE);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    size, off, m0, m1, m2, tile = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(L.PixDiscDesc) == size and L.PixDiscDesc.ws_elems.offset == off
    assert (m0, m1, m2, tile) == (L.PIXDISC_PARAMS, L.PIXDISC_INPUT, L.PIXDISC_PRED, L.PIXDISC_TILE)


def test_one_spatial_element_and_other_widths_raise(emu):
    from model import networks
    from nirgan_hip.nets import PixelDiscriminatorEngine
    with pytest.raises(NotImplementedError):
        networks.define_D(4, 32, "pixel", norm="instance")
    with pytest.raises(NotImplementedError):
        networks.define_D(4, 64, "pixel", norm="batch")
    m = Pc.ours(1, "cpu")
    flat = m._flat()
    with pytest.raises(ValueError, match="Expected more than 1 spatial element"):
        PixelDiscriminatorEngine(flat.param_views(), flat.grad_views(), 3, 1, 1)
    with pytest.raises(ValueError, match="Expected more than 1 spatial element"):
        m(torch.zeros(2, 4, 1, 1))
    with pytest.raises(ValueError, match="Expected more than 1 spatial element"):       # what stock torch answers
        Pc.Stock()(torch.zeros(2, 4, 1, 1))
    for prec in ("bf16", "bf16x3"):                                                     # accepted; the network runs fp32 in every mode
        PixelDiscriminatorEngine(flat.param_views(), flat.grad_views(), 1, 5, 5, precision=prec)
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 4, 5, 5))


# ------------------------------------------------------------------------------------------------ data parallel (gloo, two ranks)
def _setup_path():
    for p in (os.path.join(ROOT, "nir-gan_amd"), os.path.join(ROOT, "oracle"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _nets():
    from model import networks
    torch.manual_seed(5)
    netG = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", False, "normal", 0.02)
    netD = networks.define_D(4, 64, "pixel", 3, "instance", "normal", 0.02)
    return netG, netD


def _dp_batch():
    g = torch.Generator().manual_seed(77)
    return 0.02 + 0.58 * torch.rand(4, 3, 32, 32, generator=g), 0.05 + 0.75 * torch.rand(4, 1, 32, 32, generator=g)


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    _setup_path()
    torch.set_num_threads(2)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from emu_pixel_disc import EmuPixelDisc as Emu
    from nirgan_hip import lib as Lw
    from nirgan_hip.parallel import GradReducer, shard_batch
    from nirgan_hip.trainer import Pix2PixTrainer
    Lw.set_backend(Emu())
    netG, netD = _nets()
    red = GradReducer()
    tr = Pix2PixTrainer(netG, netD, n_blocks=6, reducer=red)
    rgb, nir = _dp_batch()
    out = tr.step(shard_batch(rgb, rank, world), shard_batch(nir, rank, world)).as_dict()
    st = tr._state
    # the generator keeps its buckets; the discriminator's 35 KB go as one blocking all-reduce
    assert st.bucketed and not st.bucketedD and st.headD is None and st.headG is not None and not red._pending
    assert any(n == "__hook__" for n, _ in tr.G.bwd.ops) and not any(n == "__hook__" for n, _ in tr.D2.bwd.ops)
    torch.save({"gD": tr.flatD.grad.clone(), "gG": tr.flatG.grad.clone(), "pD": tr.flatD.flat.clone(), "loss": out},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gradients_equal_single_process(tmp_path):
    import torch.multiprocessing as mp
    _setup_path()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in (0, 1))
    for k in ("gD", "gG", "pD"):
        assert torch.equal(r0[k], r1[k]), k
    from nirgan_hip.trainer import Pix2PixTrainer
    L.set_backend(EmuPixelDisc())
    try:
        netG, netD = _nets()
        tr = Pix2PixTrainer(netG, netD, n_blocks=6)
        out = tr.step(*_dp_batch()).as_dict()
    finally:
        L.set_backend(None)
    for k, ref in (("gD", tr.flatD.grad), ("gG", tr.flatG.grad)):
        err = (r0[k] - ref).norm().item() / ref.norm().item()
        print(f"PIXD two ranks {k} err {err:.3e}")
        assert err < 1e-4, (k, err)
    assert torch.equal(r0["pD"] != 0, tr.flatD.flat != 0)
    assert abs(0.5 * (r0["loss"]["loss_D"] + r1["loss"]["loss_D"]) - out["loss_D"]) < 1e-5 * abs(out["loss_D"])


# ------------------------------------------------------------------------------------------------ the shipped kernels
def test_pass_kernels_run_on_the_matrix_pipe_without_scratch(tmp_path):
    """csrc/pixdisc.hip compiled to gfx950 assembly: every pass kernel (statistics, output, backward sums, and the three gradient modes)
    issues fp32 MFMAs only, spills nothing, uses no scratch, and its LDS fits a CU (160 KB)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "pixdisc.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "pixdisc.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    names = [n for n in re.findall(r"^(_Z\w+):", text, re.M) if "pixdisc_kernelILi" in n]
    assert len(names) == 6, names
    for name in names:
        mode = int(re.search(r"pixdisc_kernelILi(\d)E", name).group(1))
        body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        mfma = re.findall(r"^\s*(v_mfma_f32_\w+)", body, re.M)
        least = {0: 128, 1: 128, 2: 128, 3: 128 + 128 + 128, 4: 128 + 128, 5: 128 + 128}[mode]
        assert len(mfma) >= least and set(mfma) == {"v_mfma_f32_32x32x2_f32"}, (mode, len(mfma), set(mfma))
        assert not re.search(r"^\s*scratch_", body, re.M), mode
        desc = text[text.index(".amdhsa_kernel " + name):text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + name))]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
        print(f"pixdisc pass kernel mode {mode}: {len(mfma)} MFMA, LDS {lds} B, scratch {scratch} B, spilled VGPRs {md and md.group(1)}")
        assert scratch == 0 and 0 < lds < 160 * 1024, (mode, scratch, lds)
        assert md and int(md.group(1)) == 0, mode
