"""The fused train step over the pairwise option matrix of tests/step_matrix_cases.py without a GPU: the table's coverage, the
reference-alone condition (stock fp32 against float64), the refusals behind the table's constraints, and every row's bodies with the C ABI
served by the numpy emulators (pixel discriminator + objectives + dropout on the common emulator).  The same bodies run against the HIP
library in tests/test_gpu_step_matrix.py.

The two ngf-32 rows run (a), (b) and (e) here: an emulated step at that width takes several seconds, and (c) / (d) exercise host logic
that does not depend on the width (they run on the MI355X for these rows too)."""
import pytest
import torch

import step_matrix_cases as M

torch.set_num_threads(4)
DEV = "cpu"
IDS = [r.id for r in M.ROWS]


@pytest.fixture()
def emu():
    from emu_dropout import EmuDropout
    from emu_pixel_disc import EmuPixelDisc
    from nirgan_hip import lib as L

    class Emu(EmuPixelDisc, EmuDropout):
        pass
    be = Emu()
    L.set_backend(be)
    yield be
    L.set_backend(None)


def test_table_covers_every_allowed_pair():
    missing, excluded = M.missing_pairs()
    print("excluded by the constraints", M.CONSTRAINTS, ":", excluded)
    assert not missing, f"pairs of levels no row holds: {missing}"
    # what the constraints take away is exactly injection on the non-square shape
    assert excluded == sorted(((("gen", g), ("shape", (3, 36, 40))) for g in ("inject", "inject_pc")), key=repr)
    assert len({r.id for r in M.ROWS + M.WIDE}) == len(M.ROWS) + len(M.WIDE) and 14 <= len(M.ROWS) <= 18
    assert set(M.SWITCH) <= set(IDS) and {M.BY_ID[i].disc for i in M.SWITCH} == {"basic", "pixel"} and {M.BY_ID[i].drop for i in M.SWITCH} == {0, 1}
    w0, w1 = M.WIDE
    assert (w0.disc, w0.gan, w0.drop, w0.pad, w0.ngf, w0.shape) == ("pixel", "vanilla", 1, 10, 32, (2, 64, 64))
    assert (w1.disc, w1.gan, w1.ssim, w1.micro, w1.ngf, w1.shape) == ("basic", "wgangp", 0.5, 2, 32, (2, 64, 64))


@pytest.mark.parametrize("rid", IDS + [r.id for r in M.WIDE])
def test_stock_fp32_lies_within_half_of_the_device_bounds(emu, rid):
    M.reference_alone(M.BY_ID[rid])


@pytest.mark.parametrize("rid", IDS)
def test_row(emu, rid):
    M.run_row(DEV, M.BY_ID[rid], M.EMU)


@pytest.mark.parametrize("rid", [r.id for r in M.WIDE])
def test_wide_row(emu, rid):
    M.run_row(DEV, M.BY_ID[rid], M.EMU, lightning=False, switch=False)


# ------------------------------------------------------------------------------------------------ what the table leaves out: refusals
def _model(row, **base):
    from model.pix2pix import Px2Px_PL
    torch.manual_seed(5)
    return Px2Px_PL(M.config(row, **base))


def test_injection_refuses_six_blocks_and_non_square_tiles(emu):
    row = M.BY_ID["m04"]
    with pytest.raises(NotImplementedError, match="resnet_9blocks"):
        _model(row, netG="resnet_6blocks")
    m = _model(row).train()
    with pytest.raises(ValueError, match="square"):
        m.train_batch(M.make_batch(row, DEV, (3, 36, 40)))


def test_dropout_refuses_the_bf16_operand_modes(emu):
    row = M.BY_ID["m02"]
    m = _model(row).train()
    m.fused_trainer().precision = "bf16"
    with pytest.raises(NotImplementedError, match="fp32"):
        m.train_batch(M.make_batch(row, DEV))


def test_padded_extent_must_be_a_multiple_of_four(emu):
    row = M.BY_ID["m08"]
    m = _model(row).train()
    with pytest.raises(ValueError, match="multiple of 4"):
        m.train_batch(M.make_batch(row, DEV, (1, 34, 34)))


def test_lambda_hist_and_concat_style_are_refused():
    row = M.BY_ID["m01"]
    with pytest.raises(NotImplementedError, match="lambda_hist"):
        _model(row, lambda_hist=1.0)
    from model.pix2pix import Px2Px_PL
    cfg = M.config(row)
    cfg.satclip.satclip_style = "concat"
    with pytest.raises(NotImplementedError, match="concat"):
        Px2Px_PL(cfg)
