"""MI355X-native counterpart of the reference's ``model/baseline_models.py`` (``train.py --baseline y``, :47-54).

``Linear_NIR(config)`` and ``MLP_NIR(config)``: the reference's constructor argument, ``state_dict`` keys (``linear.*``;
``mlp.0.*``, ``mlp.2.*``, ``mlp.4.*``) and parameter initialisation (the same ``torch.nn`` constructors in the same order, so
the same ``torch.manual_seed`` gives the same initial weights and the reference's checkpoints load with ``strict=True``).
The models are applied per pixel (baseline_models.py:19-23, :88-93); here the whole chain -- and in training the MSE, its
backward and every parameter gradient -- is ONE pass over the pixels (csrc/pixmlp.hip): the 64-wide hidden activations
never reach HBM.

``forward`` is differentiable with respect to the parameters (nirgan_hip/pixmlp.py::PixMlpFn), so the reference's
``training_step`` + ``loss.backward()`` + ``configure_optimizers()`` work as they are; ``train_batch(batch)`` is the fused
form: one nirgan_pixmlp_train (prediction, loss, gradients) and one nirgan_adam, no host synchronisation.
Device tensors only (a CPU tensor raises unless the test emulator is installed).  Out of scope: ``CNN_NIR``, image plots,
wandb, data-parallel training.
"""
from __future__ import annotations

import torch
import torch.nn as nn

try:  # Lightning is optional: the reference pins 1.9 (requirements.txt:18)
    import pytorch_lightning as pl
    _Base = pl.LightningModule
    _HAVE_PL = True
except Exception:  # pragma: no cover - depends on the environment
    _Base = torch.nn.Module
    _HAVE_PL = False

from nirgan_hip import pixmlp as PX
from nirgan_hip.flat import FlatParams
from nirgan_hip.optim import HipAdam
from utils.calculate_metrics import calculate_metrics


class BaselineLossView:
    """Lazy view of the last fused step's loss (reading synchronises; the hot loop never does)."""

    def __init__(self, loss: torch.Tensor):
        self.loss = loss

    def as_dict(self):
        return {"train/loss": float(self.loss.detach().cpu()[0])}


class _PixelBaseline(_Base):
    """Shared plumbing of the per-pixel baselines: flat parameter storage, the autograd bridge, the fused step."""

    hidden = None                   # nirgan_pixmlp_desc.hidden
    is_pixel_baseline = True        # nirgan_hip.fit.fit: one optimizer, no scheduler
    masked_validation = False       # True: validation_step's scalars are over batch["valid"] (fit sets it for a run)

    def _setup(self, config):
        self.config = config
        self.lr = float(config.base_configs.learning_rate)      # a YAML 1.1 reader hands '1e-3' over as a string
        self.steps = 0
        self.logged = {}

    def _flat(self) -> FlatParams:
        f = self.__dict__.get("_flat_obj")
        if f is None:
            f = FlatParams(self)
            self.__dict__["_flat_obj"] = f
        else:
            f.ensure()
        return f

    def _log(self, name, value):
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:
            self.log(name, value)
        else:
            self.logged[name] = value.detach() if torch.is_tensor(value) else value

    # ------------------------------------------------------------------ the reference's methods
    def forward(self, x):
        return PX.PixMlpFn.apply(self, x, *self.parameters())

    @torch.no_grad()
    def predict_step(self, rgb):
        assert self.training == False, "Model is in training mode, set to eval mode before predicting"
        return self.forward(rgb)

    def training_step(self, batch, batch_idx):
        rgb, nir = batch["rgb"], batch["nir"]
        pred = self(rgb)
        loss = nn.functional.mse_loss(pred, nir)
        self._log("train/loss", loss)
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """Scalar part of the reference's validation (baseline_models.py:32-40, :102-110): val/L1, val/L2, val/PSNR, val/SSIM on
        the device; the image / wandb logging is out of scope."""
        rgb, nir = batch["rgb"], batch["nir"]
        nir_pred = self(rgb)
        if getattr(self, "masked_validation", False):          # fit(masked_validation=True): the scalars over the batch's valid pixels
            metrics = calculate_metrics(pred=nir_pred, target=nir, phase="val", valid=batch.get("valid"))
        else:
            metrics = calculate_metrics(pred=nir_pred, target=nir, phase="val")
        for k, v in metrics.items():
            self._log(k, v)
        return metrics["val/L1"]

    @torch.no_grad()
    def validation_figures(self, batch) -> dict:
        """The figures the reference logs from validation_step (baseline_models.py:43-55): ``Images/Val NIR`` and, with
        ``custom_configs.Logging.log_ndvi``, ``Images/Val NDVI``, as images (utils.logging_helpers); wandb stays out."""
        assert self.training == False, "Model is in training mode, set to eval mode before plotting validation figures"
        from utils.logging_helpers import validation_figures
        rgb, nir = batch["rgb"], batch["nir"]
        return validation_figures(self, rgb[:, :3], nir, self(rgb))

    def configure_optimizers(self):
        return HipAdam(self.parameters(), lr=self.lr, net=self)

    # ------------------------------------------------------------------ fused fast path
    def train_batch(self, batch):
        """training_step + backward + Adam of one batch: one nirgan_pixmlp_train, one nirgan_adam; returns a lazy loss view."""
        assert self.training == True, "Model is in eval mode, set to training mode before training"
        PX._require_device(batch["rgb"], type(self).__name__)
        flat = self._flat()
        rgb = PX._boundary(batch["rgb"], 3, "rgb").to(flat.device)
        nir = PX._boundary(batch["nir"], 1, "nir").to(flat.device)
        if nir.shape[0] != rgb.shape[0] or nir.shape[2:] != rgb.shape[2:]:
            raise ValueError(f"rgb {tuple(rgb.shape)} and nir {tuple(nir.shape)} do not belong to the same tiles")
        st = self.__dict__.get("_fused_state")
        if st is None or st[0] != (rgb.shape, flat.device):
            st = (rgb.shape, flat.device), PX.workspace(rgb, self.hidden), torch.zeros(1, dtype=torch.float32, device=flat.device)
            self.__dict__["_fused_state"] = st
        _, ws, loss = st
        loss.zero_()                                            # the entry accumulates into loss_out
        PX.train(flat, self.hidden, rgb, flat.grad, ws, nir=nir, loss=loss)
        flat.adam_step(self.lr, 0.9, 0.999, 1e-8, stream=PX._stream(rgb))        # torch.optim.Adam(lr=...) defaults, baseline_models.py:70, :139
        self.steps += 1
        return BaselineLossView(loss)


class Linear_NIR(_PixelBaseline):
    hidden = 0

    def __init__(self, config):
        super().__init__()
        print("Creating Baseline Linear NIR Model")
        self._setup(config)
        self.linear = nn.Linear(3, 1)


class MLP_NIR(_PixelBaseline):
    hidden = 64

    def __init__(self, config):
        super().__init__()
        print("Creating Baseline MLP NIR Model")
        self._setup(config)
        self.mlp = nn.Sequential(
            nn.Linear(3, 64),
            nn.ReLU(),
            nn.Linear(64, 64),
            nn.ReLU(),
            nn.Linear(64, 1)
        )


class CNN_NIR(_Base):
    def __init__(self, config):
        raise NotImplementedError('Baseline model name [CNN_NIR] is not on the MI355X path yet (Linear_NIR and MLP_NIR are)')
