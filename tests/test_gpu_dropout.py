"""Dropout of the generator's residual blocks on the MI355X: csrc/dropout.hip against the numpy Philox restatement bit for bit, and
the networks with dropout against a float64 stock-torch restatement that multiplies by the exported masks.  Bodies shared with
tests/test_dropout_emulated.py (tests/dropout_cases.py).

Bounds of the whole-net comparisons: those of the same widths without dropout -- api_cases.GPU_TOL for the narrow nets, and for the
256-channel trunk on the Winograd route the engine-level bounds of tests/test_gpu_nets.py against float64 (1e-3 of the output, 6e-3
relative L2 and 5e-2 of the maximum per gradient tensor).  Dropout is a select and an exact doubling: no extra margin."""
import pytest
import torch

import dropout_cases as Dc
from api_cases import GPU_TOL, Tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE_TOL = Tol(1e-3, 6e-3, 5e-2)


@pytest.mark.parametrize("seed", Dc.SEEDS, ids=str)
@pytest.mark.parametrize("shape", Dc.MASK_SHAPES, ids=str)
def test_mask_export_equals_the_restatement(shape, seed):
    Dc.mask_bitwise(DEV, shape, seed)


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_in_place_semantics(pad):
    Dc.in_place_semantics(DEV, pad)


def test_fold_identity():
    Dc.fold_identity(DEV)


def test_statistics():
    Dc.statistics(DEV)


def test_advance():
    Dc.advance(DEV)


def test_argument_errors():
    from nirgan_hip import lib as L
    Dc.argument_errors(L.backend())


def test_eval_mode_is_the_no_dropout_generator():
    Dc.eval_mode_is_the_identity(DEV, ngf=16, size=36)


def test_train_mode_against_float64_odd_maps():
    """ngf 16, B = 2, 36 x 44: block maps 9 x 11 (odd, not square), the direct tiles."""
    Dc.train_mode_against_float64(DEV, 16, 6, 2, 36, 44, GPU_TOL)


def test_train_mode_against_float64_winograd_width():
    """ngf 64, 32 x 32: C = 256 on the Winograd route, the layers that give up their three fusions."""
    net = Dc.train_mode_against_float64(DEV, 64, 6, 1, 32, 32, WIDE_TOL)
    assert net.__dict__.get("_pool_obj") is not None


def test_train_mode_inject_against_float64():
    Dc.train_mode_against_float64(DEV, 8, 9, 1, 32, 32, GPU_TOL, inject=True)


def test_mask_sequence():
    Dc.mask_sequence(DEV)


def test_fused_trainer():
    Dc.fused_trainer(DEV)


def test_bf16_modes_refuse_dropout():
    Dc.bf16_refusal(DEV)


def test_legacy_model_accepts_dropout():
    Dc.legacy_model_accepts_dropout(DEV)
