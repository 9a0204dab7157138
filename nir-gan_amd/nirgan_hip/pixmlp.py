"""Host side of the fused per-pixel baseline kernels (csrc/pixmlp.hip; reference model/baseline_models.py).

``forward`` / ``train`` fill a ``nirgan_pixmlp_desc`` from boundary tensors (rgb B x 3 x H x W, nir B x 1 x H x W, fp32 NCHW)
and a network's ``FlatParams``; ``PixMlpFn`` is the autograd bridge behind ``Linear_NIR`` / ``MLP_NIR``'s ``forward``: its
backward is the train entry's gradient path with the upstream gradient in place of 2 (pred - nir) / n (descriptor field
``dpred``), so ``mse_loss(model(rgb), nir).backward()`` and the fused ``train_batch`` run the same kernel.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import lib as L
from .flat import FlatParams

FLAT_ELEMS = {0: 8, 64: 4484}       # flat range per `hidden`: Linear(3,1); Linear(3,64), Linear(64,64), Linear(64,1), tensors padded to 4


def _require_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError(f"{what}: tensors must live on the MI355X (cuda); the HIP path has no CPU fallback")


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream if t.device.type == "cuda" else None


def _boundary(t: torch.Tensor, channels: int, what: str) -> torch.Tensor:
    if t.dim() != 4 or t.shape[1] != channels:
        raise ValueError(f"{what} must be B x {channels} x H x W, got {tuple(t.shape)}")
    return t.detach().contiguous().float()


def _desc(flat: FlatParams, hidden: int, rgb: torch.Tensor) -> L.PixMlpDesc:
    if flat.total != FLAT_ELEMS[hidden]:
        raise ValueError(f"pixmlp: a flat range of {FLAT_ELEMS[hidden]} floats expected for hidden = {hidden}, the module has {flat.total}")
    d = L.PixMlpDesc()
    d.rgb, (d.B, _, d.H, d.W), d.hidden, d.params = rgb.data_ptr(), rgb.shape, hidden, flat.flat.data_ptr()
    return d


def workspace(rgb: torch.Tensor, hidden: int) -> torch.Tensor:
    B, _, H, W = rgb.shape
    return torch.empty(int(L.backend().nirgan_pixmlp_ws_elems(B, H, W, hidden)), dtype=torch.float32, device=rgb.device)


def forward(flat: FlatParams, hidden: int, rgb: torch.Tensor) -> torch.Tensor:
    """pred = model(rgb); rgb already contiguous fp32 on the parameters' device."""
    B, _, H, W = rgb.shape
    pred = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    d = _desc(flat, hidden, rgb)
    d.pred = pred.data_ptr()
    L.call("nirgan_pixmlp_fwd", C.byref(d), _stream(rgb))
    return pred


def train(flat: FlatParams, hidden: int, rgb: torch.Tensor, grads: torch.Tensor, ws: torch.Tensor, nir: torch.Tensor = None,
          loss: torch.Tensor = None, dpred: torch.Tensor = None, pred: torch.Tensor = None) -> None:
    """One nirgan_pixmlp_train: ``grads`` (flat layout) overwritten; with ``nir`` the mean squared error is ADDED to ``loss[0]``, with
    ``dpred`` the gradients are those of sum(pred * dpred)."""
    d = _desc(flat, hidden, rgb)
    d.nir = None if nir is None else nir.data_ptr()
    d.dpred = None if dpred is None else dpred.data_ptr()
    d.grads, d.ws, d.ws_elems = grads.data_ptr(), ws.data_ptr(), ws.numel()
    d.loss_out = None if loss is None else loss.data_ptr()
    d.pred = None if pred is None else pred.data_ptr()
    L.call("nirgan_pixmlp_train", C.byref(d), _stream(rgb))


class PixMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, rgb, *params):
        _require_device(rgb, type(net).__name__)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError(f"{type(net).__name__}: the gradient with respect to the input image is not on the MI355X path")
        flat = net._flat()
        x = _boundary(rgb, 3, "rgb").to(flat.device)
        pred = forward(flat, net.hidden, x)
        if any(ctx.needs_input_grad[2:]):
            ctx.net, ctx.x, ctx.ver = net, x, flat.values_version()
        return pred

    @staticmethod
    def backward(ctx, dpred):
        net, x = ctx.net, ctx.x
        flat = net._flat()
        if flat.values_version() != ctx.ver:
            raise RuntimeError(f"{type(net).__name__} backward: the parameters were modified after the forward of this graph")
        # the hidden activations were never stored: the train kernel computes them again next to the gradients.  ONE buffer in the flat
        # layout, the per-parameter gradients are views of it (HipAdam.step then reads it in place, optim.py)
        g = torch.empty(flat.total, dtype=torch.float32, device=flat.device)
        ws = net.__dict__.get("_bwd_ws")                        # the records' workspace stays with the module, as in train_batch
        if ws is None or ws[0] != (x.shape, flat.device):
            ws = net.__dict__["_bwd_ws"] = ((x.shape, flat.device), workspace(x, net.hidden))
        train(flat, net.hidden, x, g, ws[1], dpred=dpred.detach().contiguous().float())
        return (None, None) + tuple(g[o:o + k].view(s) for (o, k, s) in (flat.slices[n] for n in flat.names))
