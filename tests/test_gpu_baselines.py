"""The baseline models (model/baseline_models.py: Linear_NIR, MLP_NIR) ON THE MI355X through csrc/pixmlp.hip: against stock torch.nn in
float64 (bodies and tolerances in tests/baseline_cases.py), at full size (bs 32, 256 x 256: gradients 3e-4 relative L2, ReLU masks not
forced), bitwise reproducibility, the train entry's stored prediction, tiled inference, partial tiles with guard values."""
import pytest
import torch

import baseline_cases as Bc
from nirgan_hip import lib as L
from nirgan_hip import pixmlp as PX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["linear", "mlp"]


@pytest.mark.parametrize("shape", Bc.SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_loss_gradients_against_float64(kind, shape):
    Bc.forward_loss_gradients(kind, shape, DEV)


@pytest.mark.parametrize("shape", Bc.SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_five_adam_steps_both_routes_against_float64(kind, shape):
    Bc.five_adam_steps(kind, shape, DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_full_size_batch_against_float64(kind):
    """ReLU masks not forced: of the 2.7e8 pre-activations of this batch some hundred lie within fp32 rounding of zero whatever the seed
    (a seed with none does not exist at this size), and each moves one pixel's share, 1 / 2.1e6, of a gradient -- far inside 3e-4."""
    Bc.forward_loss_gradients(kind, (32, 256, 256), DEV, grad_tol=3e-4, seed=3)


def _train_once(m, b, keep_pred=True):
    flat = m._flat()
    ws = PX.workspace(b["rgb"], m.hidden)
    ws.fill_(float("nan"))
    g = torch.full((flat.total,), float("nan"), device=DEV)
    loss = torch.zeros(1, device=DEV)
    pred = torch.empty_like(b["nir"]) if keep_pred else None
    PX.train(flat, m.hidden, b["rgb"], g, ws, nir=b["nir"], loss=loss, pred=pred)
    torch.cuda.synchronize()
    return ws, g, loss, pred


@pytest.mark.parametrize("kind", KINDS)
def test_zero_residual_gives_exact_zeros(kind):
    m = Bc.make(kind, 2, DEV).train()
    b = Bc.batch((3, 67, 93), 11, DEV)
    b["nir"] = PX.forward(m._flat(), m.hidden, b["rgb"])
    _, g, loss, _ = _train_once(m, b)
    assert loss.item() == 0.0 and (g == 0).all()


@pytest.mark.parametrize("shape", [(3, 67, 93), (8, 256, 256)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_train_entry_is_bitwise_reproducible_and_its_pred_is_the_forward_entrys(kind, shape):
    m = Bc.make(kind, 2, DEV).train()
    b = Bc.batch(shape, 12, DEV)
    ws1, g1, l1, p1 = _train_once(m, b)
    ws2, g2, l2, p2 = _train_once(m, b)
    assert torch.equal(ws1, ws2) and torch.isfinite(ws1).all(), "records"
    assert torch.equal(g1, g2) and torch.equal(l1, l2) and torch.isfinite(g1).all()
    fwd = PX.forward(m._flat(), m.hidden, b["rgb"])
    assert torch.equal(p1, fwd) and torch.equal(p2, fwd)
    _, g3, l3, _ = _train_once(m, b, keep_pred=False)          # storing pred changes nothing else
    assert torch.equal(g3, g1) and torch.equal(l3, l1)


@pytest.mark.parametrize("kind", KINDS)
def test_fifty_fused_steps_twice_are_bitwise_equal(kind):
    b = Bc.batch((4, 128, 128), 13, DEV)
    runs = []
    for _ in range(2):
        m = Bc.make(kind, 4, DEV).train()
        for _ in range(50):
            view = m.train_batch(b)
        runs.append(([p.detach().clone() for p in m.parameters()], view.as_dict()["train/loss"]))
    assert all(torch.equal(a, c) for a, c in zip(runs[0][0], runs[1][0])) and runs[0][1] == runs[1][1]
    first = Bc.make(kind, 4, DEV).train().train_batch(b).as_dict()["train/loss"]
    assert runs[0][1] < first, "50 Adam steps on one batch lower its loss"


@pytest.mark.parametrize("kind", KINDS)
def test_predict_tiled_equals_the_whole_scene(kind):
    from nirgan_hip.inference import predict_tiled
    m = Bc.make(kind, 6, DEV).eval()
    g = torch.Generator().manual_seed(1)
    scene = (0.02 + 0.58 * torch.rand(1, 3, 300, 517, generator=g)).to(DEV)
    with torch.no_grad():
        whole = m(scene)
    tiled = predict_tiled(m, scene, tile=128, margin=8)
    assert tiled.shape == whole.shape
    Bc.check(f"{kind} predict_tiled vs whole scene", Bc.relerr(tiled, whole), 1e-6)
    Bc.check(f"{kind} whole scene vs float64", Bc.relerr(whole, Bc.ref_forward(Bc.ref64(kind, m), scene.cpu())), 1e-5)


@pytest.mark.parametrize("shape", [(1, 1, 1023), (1, 1, 1025), (3, 11, 31), (5, 5, 41), (1, 1, 1), (1, 1, 33)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_partial_tiles_leave_the_guards_alone(kind, shape):
    """pixel counts one less / one more than a multiple of the kernels' pixel tiles (32 per wave for hidden = 64, 256 per workgroup for
    hidden = 0: 1023 = 3 * 11 * 31 and 1025 = 5 * 5 * 41, the latter two with images that end inside a tile)"""
    B, H, W = shape
    n = B * H * W
    assert L.PIXMLP_TILE == 32
    m = Bc.make(kind, 8, DEV).train()
    flat = m._flat()
    b = Bc.batch(shape, 14, DEV)
    G = 64
    pbuf = torch.full((n + 2 * G,), 123.0, device=DEV)
    gbuf = torch.full((flat.total + 2 * G,), 321.0, device=DEV)
    lbuf = torch.full((1 + 2 * G,), 55.0, device=DEV)
    lbuf[G] = 0
    ws = PX.workspace(b["rgb"], m.hidden)
    PX.train(flat, m.hidden, b["rgb"], gbuf[G:G + flat.total], ws, nir=b["nir"], loss=lbuf[G:G + 1], pred=pbuf[G:G + n])
    torch.cuda.synchronize()
    for name, buf, k, v in (("pred", pbuf, n, 123.0), ("grads", gbuf, flat.total, 321.0), ("loss", lbuf, 1, 55.0)):
        assert (buf[:G] == v).all() and (buf[G + k:] == v).all(), name + " guard"
    r, pred64, loss64, g64 = Bc.ref_grads(kind, m, b)
    Bc.check(f"{kind} {shape} pred", Bc.relerr(pbuf[G:G + n].view(B, 1, H, W), pred64), 1e-5)
    Bc.check(f"{kind} {shape} loss", abs(lbuf[G].item() - loss64) / loss64, 1e-3)
    got = gbuf[G:G + flat.total]
    for k, (o, cnt, shp) in flat.slices.items():
        Bc.check(f"{kind} {shape} grad {k}", Bc.rel_l2(got[o:o + cnt].view(shp), g64[k]), 1e-3)
    assert torch.equal(PX.forward(flat, m.hidden, b["rgb"]).view(-1), pbuf[G:G + n])


@pytest.mark.parametrize("kind", KINDS)
def test_fit_history_checkpoint_resume(kind, tmp_path):
    Bc.fit_checkpoint_resume(kind, DEV, tmp_path)
