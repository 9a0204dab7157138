"""The baseline models (model/baseline_models.py: Linear_NIR, MLP_NIR; train.py --baseline) without a GPU: the host logic on the numpy
statement of the nirgan_pixmlp_* entries (tests/emu_baselines.py) against stock torch.nn in float64, the argument checks of the real
library, and the disassembly of the shipped kernels (hipcc cross-compiles).  Bodies shared with tests/test_gpu_baselines.py."""
import os
import re
import subprocess

import pytest
import torch

import baseline_cases as Bc
from emu_baselines import EmuBaselines
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["linear", "mlp"]


@pytest.fixture()
def emu():
    be = EmuBaselines()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_seeded_weights_are_the_references(kind, capsys):
    Bc.state_dict_and_seed(kind)


@pytest.mark.parametrize("shape", Bc.SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_loss_gradients_against_float64(emu, kind, shape):
    Bc.forward_loss_gradients(kind, shape, "cpu")
    assert "pixmlp_fwd" in emu.calls and "pixmlp_train" in emu.calls


@pytest.mark.parametrize("shape", Bc.SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_five_adam_steps_both_routes_against_float64(emu, kind, shape):
    Bc.five_adam_steps(kind, shape, "cpu")
    assert emu.calls.count("adam") == 10


@pytest.mark.parametrize("kind", KINDS)
def test_fit_history_checkpoint_resume(emu, kind, tmp_path):
    Bc.fit_checkpoint_resume(kind, "cpu", tmp_path)


def test_cnn_nir_and_cpu_tensors_raise():
    from model.baseline_models import CNN_NIR, MLP_NIR
    with pytest.raises(NotImplementedError, match="CNN_NIR"):
        CNN_NIR(Bc.cfg())
    m = MLP_NIR(Bc.cfg())
    b = Bc.batch((1, 5, 5), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(b["rgb"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train().train_batch(b)


def test_emulator_enforces_the_workspace_and_accumulates_the_loss(emu):
    import ctypes as C
    m = Bc.make("mlp", 0, "cpu").train()
    b = Bc.batch((1, 5, 5), 0)
    flat = m._flat()
    pred, loss, ws = torch.empty(1, 1, 5, 5), torch.zeros(1), torch.empty(int(emu.nirgan_pixmlp_ws_elems(1, 5, 5, 64)))
    d = L.PixMlpDesc()
    d.rgb, d.nir, d.B, d.H, d.W, d.hidden = b["rgb"].data_ptr(), b["nir"].data_ptr(), 1, 5, 5, 64
    d.params, d.grads, d.loss_out, d.ws, d.ws_elems = flat.flat.data_ptr(), flat.grad.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel() - 1
    assert emu.nirgan_pixmlp_train(C.byref(d)) == -1 and b"workspace" in emu.nirgan_last_error()
    d.ws_elems = ws.numel()
    assert emu.nirgan_pixmlp_train(C.byref(d)) == 0 and emu.nirgan_pixmlp_train(C.byref(d)) == 0
    one = torch.nn.functional.mse_loss(m(b["rgb"]), b["nir"]).item()
    assert abs(loss.item() - 2 * one) <= 1e-5 * one


def test_real_library_rejects_bad_arguments_before_any_launch():
    be = L.backend()
    assert not L.is_emulated()
    d = L.PixMlpDesc()
    assert be.nirgan_pixmlp_fwd(d, None) == -1 and b"pixmlp" in be.nirgan_last_error()
    assert be.nirgan_pixmlp_train(d, None) == -1 and b"pixmlp" in be.nirgan_last_error()
    buf = torch.zeros(4484 + 3 * 25 + 64)
    d.rgb = d.nir = d.params = d.grads = d.pred = d.loss_out = d.ws = buf.data_ptr()
    d.B, d.H, d.W, d.hidden, d.ws_elems = 1, 5, 5, 32, 1 << 20
    assert be.nirgan_pixmlp_fwd(d, None) == -1 and b"hidden" in be.nirgan_last_error()
    assert be.nirgan_pixmlp_train(d, None) == -1 and b"hidden" in be.nirgan_last_error()
    d.hidden, d.W = 64, 0
    assert be.nirgan_pixmlp_train(d, None) == -1 and b"shape" in be.nirgan_last_error()
    d.W, d.ws_elems = 5, 10
    assert be.nirgan_pixmlp_train(d, None) == -1 and b"workspace" in be.nirgan_last_error()
    n = be.nirgan_pixmlp_ws_elems(32, 256, 256, 64)
    assert 0 < n and n * 4 < 8e6
    assert n == be.nirgan_pixmlp_ws_elems(64, 256, 256, 64)            # grid x record, nothing per pixel
    nl = be.nirgan_pixmlp_ws_elems(32, 256, 256, 0)
    assert 0 < nl and nl * 4 < 8e6 and nl == be.nirgan_pixmlp_ws_elems(64, 256, 256, 0)
    assert be.nirgan_pixmlp_ws_elems(1, 1, 1, 64) == 4488 and be.nirgan_pixmlp_ws_elems(1, 1, 1, 32) == 0
    # the emulator restates the same sizes
    emu = EmuBaselines()
    for args in [(32, 256, 256, 64), (1, 5, 5, 64), (3, 67, 93, 64), (3, 67, 93, 0), (64, 256, 256, 0), (1, 1, 1, 0)]:
        assert emu.nirgan_pixmlp_ws_elems(*args) == be.nirgan_pixmlp_ws_elems(*args), args


def test_shipped_train_kernel_runs_on_the_matrix_pipe_without_scratch(tmp_path):
    """csrc/pixmlp.hip compiled to gfx950 assembly the way scripts/check_x3_asm.py does: the hidden = 64 train kernel issues fp32 MFMAs,
    spills nothing, uses no scratch, and its LDS fits a CU (160 KB)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "pixmlp.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "pixmlp.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    name = next(n for n in re.findall(r"^(_Z\w+):", text, re.M) if "pixmlp64_kernelILb1E" in n)
    body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
    mfma = re.findall(r"^\s*(v_mfma_f32_\w+)", body, re.M)
    assert len(mfma) >= 192 and set(mfma) == {"v_mfma_f32_32x32x2_f32"}, (len(mfma), set(mfma))
    assert not re.search(r"^\s*scratch_", body, re.M)
    desc = text[text.index(".amdhsa_kernel " + name):text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + name))]
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
    print(f"pixmlp64 train kernel: {len(mfma)} MFMA, LDS {lds} B, scratch {scratch} B")
    assert scratch == 0 and 0 < lds < 160 * 1024
    md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
    assert md and int(md.group(1)) == 0
