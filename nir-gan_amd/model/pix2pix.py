"""MI355X-native counterpart of the reference's ``model/pix2pix.py`` (class ``Px2Px_PL``).

Same constructor argument (the YAML config tree), attributes (``netG, netD, criterionGAN,
criterionL1, rs_losses, satclip, config, opt``) and methods (``forward, predict_step,
training_step, extract_batch, configure_optimizers``; reference model/pix2pix.py:17-492).
It subclasses ``pytorch_lightning.LightningModule`` when Lightning is importable (so the
reference's train.py drives it unchanged) and ``torch.nn.Module`` otherwise; in both cases
``train_batch(batch)`` runs the whole two-optimizer batch on the fused HIP trainer.

The train / validation image metrics (calculate_metrics: L1, L2, PSNR, SSIM) are one fused device pass
(utils/calculate_metrics.py -> nirgan_image_metrics) instead of the reference's ``.cpu()`` round trip.
Out of scope here (plot/wandb branches): validation_step's image logging, the SatCLIP location
encoder itself -- ``coords`` may carry the precomputed B x 256 embeddings (as the reference's own smoke test
does, pix2pix.py:509-526).
"""
from __future__ import annotations

import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau

try:  # Lightning is optional: the reference pins 1.9 (requirements.txt:18)
    import pytorch_lightning as pl
    _Base = pl.LightningModule
    _HAVE_PL = True
except Exception:  # pragma: no cover - depends on the environment
    _Base = torch.nn.Module
    _HAVE_PL = False

from model import networks
from nirgan_hip import functional as HF
from nirgan_hip.optim import HipAdam
from nirgan_hip.trainer import Pix2PixTrainer
from utils.calculate_metrics import calculate_metrics


def _cfg(node, name, default=None):
    """Optional config entry: OmegaConf nodes, namespaces and attribute-dicts signal absence differently."""
    try:
        v = getattr(node, name)
    except (AttributeError, KeyError):
        return default
    return default if v is None else v


class HipL1Loss(torch.nn.Module):
    """torch.nn.L1Loss() for (prediction, target) NIR tiles on the fused HIP pixel-loss pass."""

    def forward(self, pred, target, valid=None):
        """``valid``: a [B,1,H,W] mask (``valid != 0``, shared by the channels): the mean runs over its pixels only, 0 if there is none"""
        if pred.dim() != 4 or pred.shape != target.shape:
            raise ValueError(f"HipL1Loss: prediction {tuple(pred.shape)} and target {tuple(target.shape)} must be equal 4-d shapes")
        B, C, H, W = pred.shape
        if valid is not None:
            if tuple(valid.shape) != (B, 1, H, W):
                raise ValueError(f"HipL1Loss: valid {tuple(valid.shape)} must be {(B, 1, H, W)}")
            valid = valid.expand(B, C, H, W).reshape(B * C, 1, H, W)
        # the mean over all elements does not care how they are split over (B, C): any channel count runs as B*C planes
        return HF.pix_loss(None, target.reshape(B * C, 1, H, W), pred.reshape(B * C, 1, H, W), (1.0, 0, 0, 0, 0, 0, 0), 0, valid)


class Px2Px_PL(_Base):
    masked_validation = False       # True: validation_step's scalars are over batch["valid"] (nirgan_hip.fit.fit sets it for a run)

    def __init__(self, opt):
        super(Px2Px_PL, self).__init__()
        self.opt = opt.base_configs
        self.config = opt
        self.isTrain = self.opt.isTrain
        sat = self.config.satclip
        use_sat = bool(sat.use_satclip)
        if use_sat and sat.satclip_style == "concat":
            raise NotImplementedError("SatCLIP 'concat' style is not on the MI355X path; use 'inject'")
        elif use_sat and sat.satclip_style == "inject":
            print(f"Creating SatCLIP Injection Generator with injection style: '{sat.satclip_inject_style}'.")
            from model.generator_inject import define_G_inject
            self.netG = define_G_inject(self.config)
        else:
            print("Creating Standard Pix2Pix Generator.")
            self.netG = networks.define_G(self.opt.input_nc, self.opt.output_nc, self.opt.ngf, self.opt.netG, self.opt.norm,
                                          not self.opt.no_dropout, self.opt.init_type, self.opt.init_gain)
        self.netD = networks.define_D(self.opt.input_nc + self.opt.output_nc, self.opt.ndf, self.opt.netD,
                                      self.opt.n_layers_D, self.opt.norm, self.opt.init_type, self.opt.init_gain)
        self.criterionGAN = networks.GANLoss(self.opt.gan_mode)
        self.criterionL1 = HipL1Loss()
        if self.opt.lambda_rs_losses > 0.0:
            from utils.remote_sensing_indices import RemoteSensingIndices
            self.rs_losses = RemoteSensingIndices(mode="loss", criterion=self.opt.rs_losses_criterium)
        self.lambda_ssim = float(_cfg(self.opt, "lambda_ssim", 0.0) or 0.0)
        if (_cfg(self.opt, "lambda_hist", 0.0) or 0.0) > 0.0:
            # the reference's own branch calls an undefined hist_loss (pix2pix.py:239-243): it cannot run there either
            raise NotImplementedError("lambda_hist > 0 is not on the MI355X path (the reference's training_step calls an undefined hist_loss)")
        self.satclip = use_sat
        # frozen SatCLIP location encoder (pix2pix.py:69-80): built from the checkpoint when it is there (no network
        # here: the file must be local); without it ``coords`` must already carry the B x 256 embeddings
        self.satclip_model = None
        self._satclip_path = _cfg(sat, "satclip_path") or "model/satclip/satclip-resnet50-l10.ckpt"
        self._fused = None
        self.logged = {}

    # ------------------------------------------------------------------ pad -> netG -> crop
    def forward(self, input, embeds=None, use_padding=True):
        pad = int(self.config.Data.padding_amount) if self.config.Data.padding else 0
        self.netG.data_pad = pad           # reflect pad + crop are folded into the first / last kernel
        if not self.satclip:
            return self.netG(input)
        if self.config.satclip.satclip_style == "inject":
            return self.netG(input, embeds)
        raise NotImplementedError("SatClip Style not recognized")

    @torch.no_grad()
    def predict_step(self, rgb, coords=None):
        assert self.training == False, "Model is in training mode, set to eval mode before predicting"
        if self.satclip == False:
            batch = {"rgb": rgb, "nir": torch.Tensor([0])}
            rgb, _ = self.extract_batch(batch)
            return self.forward(rgb)
        if self.config.satclip.satclip_style == "inject":
            batch = {"rgb": rgb, "nir": torch.Tensor([0]), "coords": coords}
            rgb, _, embeds = self.extract_batch(batch)
            return self.forward(rgb, embeds)
        raise NotImplementedError("SatClip Style not recognized, choose 'concat' or 'inject'")

    def _log(self, name, value):
        if _HAVE_PL and getattr(self, "_trainer", None) is not None:
            self.log(name, value)
        else:
            self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def training_step(self, batch, batch_idx, optimizer_idx):
        assert self.training == True, "Model is in eval mode, set to training mode before training"
        embeds = None
        if self.satclip == False:
            rgb, nir = self.extract_batch(batch)
        else:
            rgb, nir, embeds = self.extract_batch(batch)
        pred = self.forward(rgb, embeds) if embeds is not None else self.forward(rgb)
        # train metrics every 10th batch on the first optimizer pass (pix2pix.py:181-191), computed on the device
        if optimizer_idx == 0 and batch_idx % 10 == 0 and self._wants_metrics():
            for k, v in calculate_metrics(pred=pred, target=nir, phase="train").items():
                self._log(k, v)
            if hasattr(self.netG, "scale_param"):
                self._log("scale_param", self.netG.scale_param.item())
            if hasattr(self.netG, "post_correction_param"):
                self._log("post_correction_param", self.netG.post_correction_param.item())
        if optimizer_idx == 0:
            fake_AB = torch.cat((rgb, pred), 1)
            real_AB = torch.cat((rgb, nir), 1)
            # the reference calls netD twice (pix2pix.py:197-204); InstanceNorm is per sample, so ONE pass over [fake ; real] gives
            # the same two patch maps (and one backward instead of two)
            nb = fake_AB.shape[0]
            both = self.netD(torch.cat((fake_AB.detach(), real_AB), 0))
            pred_fake, pred_real = both[:nb], both[nb:]
            loss_D_fake = self.criterionGAN(pred_fake, False)
            loss_D_real = self.criterionGAN(pred_real, True)
            loss_D = (loss_D_fake + loss_D_real)
            self._log("model_loss/discriminator_real", loss_D_real)
            self._log("model_loss/discriminator_fake", loss_D_fake)
            self._log("model_loss/discriminator_loss", loss_D)
            return loss_D
        if optimizer_idx == 1:
            fake_AB = torch.cat((rgb, pred), 1)
            pred_fake = self.netD(fake_AB)
            loss_G_GAN = self.criterionGAN(pred_fake, True)
            self._log("model_loss/generator_GAN_loss", loss_G_GAN)
            valid = batch.get("valid")                                   # the loader's mask (return_valid=True): the reconstruction terms skip nodata
            loss_G_L1 = self.criterionL1(pred, nir, valid)
            self._log("model_loss/generator_L1", loss_G_L1)
            loss_G = loss_G_GAN * self.opt.lambda_GAN + loss_G_L1 * self.opt.lambda_L1
            if self.lambda_ssim > 0.0:                                   # pix2pix.py:233-237
                if valid is not None:
                    raise NotImplementedError("valid with lambda_ssim > 0: the SSIM windows would straddle the mask")
                from utils.losses import ssim_loss
                loss_G_ssim = ssim_loss(pred, nir)
                self._log("model_loss/generator_ssim", loss_G_ssim)
                loss_G = loss_G + loss_G_ssim * self.lambda_ssim
            if self.opt.lambda_rs_losses > 0.0:
                losses_rs_indices = self.rs_losses.get_and_weight_losses(rgb, nir, pred,
                                                                         loss_config=dict(self.opt.internal_rs_loss_weights), valid=valid)
                self._log("model_loss/indices_loss_weighted", losses_rs_indices)
                loss_G = loss_G + losses_rs_indices * self.opt.lambda_rs_losses
            self._log("model_loss/generator_total_loss", loss_G)
            return loss_G

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """Scalar part of the reference's validation (pix2pix.py:259-315): val/L1, val/L2, val/PSNR, val/SSIM (the
        ReduceLROnPlateau monitor is val/L1, :488-492), prediction/input statistics and the six index errors; the
        image/plot/wandb logging is out of scope."""
        embeds = None
        if self.satclip == False:
            rgb, nir = self.extract_batch(batch)
        else:
            rgb, nir, embeds = self.extract_batch(batch)
        nir_pred = self.predict_step(rgb, embeds) if embeds is not None else self.predict_step(rgb)
        rgb = rgb[:, :3, :, :]
        if getattr(self, "masked_validation", False):          # fit(masked_validation=True): the scalars over the batch's valid pixels
            metrics = calculate_metrics(pred=nir_pred, target=nir, phase="val", valid=batch.get("valid"))
        else:
            metrics = calculate_metrics(pred=nir_pred, target=nir, phase="val")
        for k, v in metrics.items():
            self._log(k, v)
        if self._wants_metrics() and batch_idx < self._num_val_images():
            if _cfg(_cfg(_cfg(self.config, "custom_configs"), "Logging"), "log_input_stats", False):
                self._log("val_stats/min_pred", torch.min(nir_pred).item())
                self._log("val_stats/max_pred", torch.max(nir_pred).item())
                self._log("val_stats/mean_pred", torch.mean(nir_pred).item())
                self._log("val_stats/min_input", torch.min(nir).item())
                self._log("val_stats/max_input", torch.max(nir).item())
                self._log("val_stats/mean_input", torch.mean(nir).item())
            if self.opt.lambda_rs_losses > 0.0:
                for k, v in self.rs_losses.get_and_weight_losses(rgb, nir, nir_pred, mode="logging_dict").items():
                    self._log(k, v)
        return metrics["val/L1"]

    @torch.no_grad()
    def validation_figures(self, batch) -> dict:
        """The figures the reference logs from validation_step (pix2pix.py:286-298): ``Images/Val NIR`` (plot_tensors_hist) and, with
        ``custom_configs.Logging.log_ndvi``, ``Images/Val NDVI`` (plot_index), as images; the prediction is validation_step's.  The
        numbers behind each figure come from one nirgan_val_panel call (utils.logging_helpers).  wandb stays out."""
        assert self.training == False, "Model is in training mode, set to eval mode before plotting validation figures"
        from utils.logging_helpers import validation_figures
        embeds = None
        if self.satclip == False:
            rgb, nir = self.extract_batch(batch)
        else:
            rgb, nir, embeds = self.extract_batch(batch)
        nir_pred = self.predict_step(rgb, embeds) if embeds is not None else self.predict_step(rgb)
        return validation_figures(self, rgb[:, :3, :, :], nir, nir_pred)

    def _wants_metrics(self) -> bool:
        """The reference logs only when a logger with an experiment is attached (pix2pix.py:182, :280); without
        Lightning the values go to ``self.logged``."""
        if _HAVE_PL:
            lg = getattr(self, "logger", None)
            return bool(lg) and hasattr(lg, "experiment")
        return True

    def _num_val_images(self) -> int:
        return int(_cfg(_cfg(_cfg(self.config, "custom_configs"), "Logging"), "num_val_images", 0))

    def extract_batch(self, batch):
        rgb = batch["rgb"]
        nir = batch["nir"]
        if not self.satclip:
            return rgb, nir
        coords = batch["coords"]
        if self.config.satclip.satclip_style == "inject":
            return rgb, nir, self.satclip_get_inject(coords)
        raise NotImplementedError("SatClip Style not recognized, choose 'concat' or 'inject'")

    def satclip_get_inject(self, coords):
        """pix2pix.py:481-484: lon/lat -> embeddings with the frozen location encoder (one fused fp64 HIP launch).
        B x 256 inputs are taken as precomputed embeddings (the reference's own smoke test feeds those, :509-526)."""
        if coords is not None and coords.dim() == 2 and coords.shape[-1] == 256:
            return coords.float()
        # the same coords tensor in both optimizer passes of a batch gives the same embeddings OBJECT (the generator then
        # recognises the repeated forward, functional._ForwardRecord)
        hit = self.__dict__.get("_emb_record")
        if hit is not None and hit[0] is coords and hit[1] == coords._version:
            return hit[2]
        if coords is None or coords.dim() != 2 or coords.shape[-1] != 2:
            raise ValueError("coords must be B x 2 (lon, lat) or B x 256 precomputed SatCLIP embeddings")
        if self.satclip_model is None:
            import os
            if not os.path.exists(self._satclip_path):
                raise FileNotFoundError(f"SatCLIP checkpoint '{self._satclip_path}' not found (config.satclip.satclip_path); "
                                        "pass B x 256 embeddings as 'coords' or provide the checkpoint")
            from model.satclip.satclip_wrapper import SatClIP_wrapper
            self.satclip_model = SatClIP_wrapper(self._satclip_path, device=coords.device).eval()
        with torch.no_grad():
            emb = self.satclip_model.predict(coords.double()).float()
        self.__dict__["_emb_record"] = (coords, coords._version, emb)
        return emb

    def configure_optimizers(self):
        optim_g = HipAdam(self.netG.parameters(), lr=self.opt.lr, betas=(self.opt.beta1, 0.999), net=self.netG)
        optim_d = HipAdam(self.netD.parameters(), lr=self.opt.lr, betas=(self.opt.beta1, 0.999), net=self.netD)
        sched_g = ReduceLROnPlateau(optim_g, mode='min', patience=self.config.Schedulers.patience_g)
        sched_d = ReduceLROnPlateau(optim_d, mode='min', patience=self.config.Schedulers.patience_d)
        return ([optim_d, optim_g],
                [{'scheduler': sched_d, 'monitor': self.config.Schedulers.metric, 'interval': 'epoch'},
                 {'scheduler': sched_g, 'monitor': self.config.Schedulers.metric, 'interval': 'epoch'}])

    # ------------------------------------------------------------------ fused fast path
    def fused_trainer(self, reducer=None) -> Pix2PixTrainer:
        if self._fused is None:
            sat = self.config.satclip
            inject = None
            if self.satclip:
                inject = {"style": sat.satclip_inject_style, "use_scale": bool(sat.scaling_param),
                          "post_correction": bool(sat.post_correction)}
            pad = int(self.config.Data.padding_amount) if self.config.Data.padding else 0
            self._fused = Pix2PixTrainer(
                self.netG, self.netD, n_blocks=self.netG.n_blocks, lr=self.opt.lr, beta1=self.opt.beta1,
                lambda_gan=self.opt.lambda_GAN, lambda_l1=self.opt.lambda_L1, lambda_rs=self.opt.lambda_rs_losses,
                rs_weights=dict(self.opt.internal_rs_loss_weights), rs_criterion=self.opt.rs_losses_criterium,
                padding=pad, inject=inject, reducer=reducer, lambda_ssim=self.lambda_ssim, gan_mode=self.opt.gan_mode)
        return self._fused

    def train_batch(self, batch):
        """Both optimizer passes of one batch (D then G) on the fused HIP trainer; returns a lazy loss view."""
        assert self.training == True, "Model is in eval mode, set to training mode before training"
        if self.satclip:
            rgb, nir, embeds = self.extract_batch(batch)
        else:
            (rgb, nir), embeds = self.extract_batch(batch), None
        tr = self.fused_trainer()
        tr.real_label, tr.fake_label = self.criterionGAN._label_value(True), self.criterionGAN._label_value(False)   # networks.py:229-230
        return tr.step(rgb, nir, embeds, valid=batch.get("valid"))
