"""Dropout of the generator's residual blocks without a GPU: the Philox restatement against its known answers, the host logic
(module layout, state, plans, trainer) on the numpy statement of the nirgan_dropout_* entries (tests/emu_dropout.py), the argument
checks of the real library and the descriptor's layout.  Bodies shared with tests/test_gpu_dropout.py (tests/dropout_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import dropout_cases as Dc
from api_cases import CPU_TOL
from emu_dropout import EmuDropout
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuDropout()
    L.set_backend(be)
    yield be
    L.set_backend(None)


def test_philox_known_answers():
    Dc.philox_known_answers()


@pytest.mark.parametrize("seed", Dc.SEEDS, ids=str)
@pytest.mark.parametrize("shape", Dc.MASK_SHAPES[:3], ids=str)
def test_mask_export_equals_the_restatement(emu, shape, seed):
    Dc.mask_bitwise("cpu", shape, seed)


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_in_place_semantics(emu, pad):
    Dc.in_place_semantics("cpu", pad)


def test_fold_identity(emu):
    Dc.fold_identity("cpu")


def test_statistics(emu):
    Dc.statistics("cpu")


def test_advance(emu):
    Dc.advance("cpu")


def test_argument_errors_emulator(emu):
    Dc.argument_errors(emu)


def test_argument_errors_real_library():
    """The library itself, on host pointers: every case returns before a launch (no GPU here)."""
    assert not L.is_emulated()
    Dc.argument_errors(L.backend())


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof and the last field's offset of nirgan_dropout_desc as gcc lays it out (as test_capi_exports does for the others)."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %zu\\n", sizeof(nirgan_dropout_desc), offsetof(nirgan_dropout_desc, sample0));\nreturn 0;}\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    size, off = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(L.DropoutDesc) == size and L.DropoutDesc.sample0.offset == off
    assert L.DropoutDesc._fields_[-1][0] == "sample0"


def test_state_dict_is_the_references():
    Dc.state_dict_is_the_references()


def test_eval_mode_is_the_no_dropout_generator(emu):
    Dc.eval_mode_is_the_identity("cpu")
    assert not [c for c in emu.calls if c == "dropout_advance" or (isinstance(c, tuple) and c[0] == "dropout_halo")]


def test_train_mode_against_float64(emu):
    Dc.train_mode_against_float64("cpu", 8, 6, 2, 32, 32, CPU_TOL)
    halos = [c for c in emu.calls if isinstance(c, tuple) and c[0] == "dropout_halo"]
    plan = [c for c in halos if c[2] == 1]         # (the case's own mask exports run on dense tensors: pad 0)
    # forward: blocks 0..5 on c1's halo'd output; backward: blocks 5..0 on the padded gradient
    assert plan == [("dropout_halo", j, 1) for j in range(6)] + [("dropout_halo", j, 1) for j in range(5, -1, -1)]
    assert emu.calls.count("dropout_advance") == 1 and emu.calls.index("dropout_advance") < emu.calls.index("nchw_to_halo")


def test_train_mode_inject_against_float64(emu):
    Dc.train_mode_against_float64("cpu", 8, 9, 1, 32, 32, CPU_TOL, inject=True)


def test_winograd_width_plans_give_up_the_three_fusions(emu):
    """ngf = 32 (128-channel trunk, the Winograd route): with dropout no block folds c1's apply into c2's input transform, no data
    gradient's output transform takes c1's first backward pass, no dY is evaluated inside the transform; without, all three happen."""
    from nirgan_hip.flat import FlatParams
    from nirgan_hip.nets import GeneratorEngine
    seen = {}
    for drop in (False, True):
        net = Dc.make_generator(32, 6, False)
        flat = FlatParams(net)
        eng = GeneratorEngine(flat.param_views(), flat.grad_views(), 6, 1, 48, 48, dropout=drop)
        seen[drop] = ([n for n, _ in eng.fwd.ops], [n for n, _ in eng.bwd.ops], eng)
    f0, b0, e0 = seen[False]
    f1, b1, e1 = seen[True]
    assert f0.count("nirgan_wino6_input_norm") == 6 and f1.count("nirgan_wino6_input_norm") == 0
    assert f1[0] == "nirgan_dropout_advance" and f1.count("nirgan_dropout_halo") == 6 and b1.count("nirgan_dropout_halo") == 6
    assert "nirgan_dropout_halo" not in f0 + b0 and "nirgan_dropout_advance" not in f0
    assert b0.count("nirgan_wino6_input_dy_norm") == 12 and b1.count("nirgan_wino6_input_dy_norm") == 6      # c2 keeps its own
    for _, c1, c2 in e1.blocks:
        assert c1.two_pass_in_bwd and not c2.two_pass_in_bwd and not c1.defer_apply
    # every c1 backward of the dropout engine reads the padded gradient itself: the op in front of it is the mask
    idx = [i for i, n in enumerate(b1) if n == "nirgan_dropout_halo"]
    assert all(b1[i + 1] == "nirgan_instnorm_bwd" for i in idx)
    for i in idx:
        d = e1.bwd.ops[i + 1][1][0]._obj
        assert d.g_fold == 1 and d.sums_chunks == 0 and d.dy
    e1.set_dropout_state(5, 0)
    e1.forward(Dc.synth(1, 48, 48, 5)[0])
    e1.backward(torch.ones_like(e1.pred))
    assert all(torch.isfinite(g).all() for g in e1.grads.values()) and e1.drop_words == (5, 0, 1)


def test_mask_sequence(emu):
    Dc.mask_sequence("cpu")


def test_fused_trainer(emu):
    Dc.fused_trainer("cpu")


def test_bf16_modes_refuse_dropout(emu):
    Dc.bf16_refusal("cpu")


def test_legacy_model_accepts_dropout(emu):
    Dc.legacy_model_accepts_dropout("cpu")
