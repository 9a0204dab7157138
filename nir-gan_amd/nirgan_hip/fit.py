"""A Lightning-free training loop for ``Px2Px_PL`` ("train.py drops in without Lightning").

What the reference delegates to ``pytorch_lightning.Trainer.fit`` (train.py:118-136) and what of it touches the hot
path: per batch the two optimizer passes (here ONE fused call, ``model.train_batch``), per epoch the validation scalars
(``validation_step``: val/L1, val/L2, val/PSNR, val/SSIM) and ``ReduceLROnPlateau`` on ``config.Schedulers.metric``
for both optimizers (model/pix2pix.py:485-492), plus a checkpoint in Lightning's layout: ``state_dict`` with the
reference's keys (train.py:61-65 / create_synthetic_dataset.py:24-26 load it with ``strict=False``), ``optimizer_states``
(both Adams: moments and step counts, torch.optim.Adam's format) and ``lr_schedulers`` (both ReduceLROnPlateau), so that
``resume_from`` continues a run the way ``Trainer(resume_from_checkpoint=...)`` does (train.py:66-70,126).  Loggers, wandb and
callbacks are out of scope.  Data parallel: pass a ``parallel.GradReducer`` (one process per GPU, RCCL); validation
metrics are averaged over ranks when a process group is initialised.  ``tile_table_path``: every validation epoch also
writes the per-tile metrics table of its validation batches (validation_utils.tile_metrics.evaluate_tiles, the reference's
spider_validation_callback) to ``<stem>_e<epoch><ext>``; rank 0 writes it under data parallel.  ``time_series``: every
``time_series_every`` validation epochs the NDVI time series of a date stack (validation_utils.time_series_validation.ndvi_timeline,
what the reference plots from on_validation_epoch_end, model/pix2pix.py:347-412) is appended to ``history["time_series"]``.  ``figures_dir``: every ``figures_every`` validation epochs the reference's two validation figures
(utils.logging_helpers, model/pix2pix.py:286-298) of the first ``Logging.num_val_images`` validation batches are written as PNG files.
``land_cover_table_path``: every validation epoch also writes the land-cover-stratified table (validation_utils.land_cover.
evaluate_land_cover) of its validation batches to ``<stem>_e<epoch><ext>``, rank 0 under data parallel.
``masked_validation``: the validation batches carry ``valid`` and the ``val/*`` scalars and the tile table are taken over the valid
pixels (utils.calculate_metrics.calculate_metrics(valid=), evaluate_tiles(masked=True)).
wandb and Lightning loggers stay out of scope.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, Dict, Iterable, Optional

import torch


def _to_device(batch: dict, device) -> dict:
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _rank_mean(value: float, device) -> float:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([value], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t)
        return float(t.item()) / dist.get_world_size()
    return value


def _write_table(evaluate, model, val_loader, device, path, crop, epoch):
    import os
    stem, ext = os.path.splitext(path)
    evaluate(model, val_loader, crop=crop, device=device, csv_path=f"{stem}_e{epoch}{ext}")


def _time_series(model, time_series, device, epoch):
    """ndvi_timeline of the stack under the model as it is now: ``time_series`` is a glob of rasters or a (rgbs, nirs) pair"""
    from validation_utils.time_series_validation import get_pred_nirs_and_info, ndvi_timeline, predict_stack
    if isinstance(time_series, str):
        rgbs, nirs, preds, _ = get_pred_nirs_and_info(model, device, time_series)
    else:
        rgbs, nirs = (torch.as_tensor(t).to(device) for t in time_series)
        preds = predict_stack(model, rgbs)
    return {"epoch": epoch, **ndvi_timeline(rgbs, nirs, preds)}


def _write_figures(model, val_loader, device, figures_dir, epoch, history):
    """val_nir_e<epoch>_b<i>.png (and val_ndvi_.. with Logging.log_ndvi) of the first Logging.num_val_images validation batches"""
    import os
    from model.pix2pix import _cfg
    count = int(_cfg(_cfg(_cfg(model.config, "custom_configs"), "Logging"), "num_val_images", 0) or 0)
    os.makedirs(figures_dir, exist_ok=True)
    names = {"Images/Val NIR": "val_nir", "Images/Val NDVI": "val_ndvi"}
    for i, batch in enumerate(val_loader):
        if i >= count:
            break
        for key, im in model.validation_figures(_to_device(batch, device)).items():
            path = os.path.join(figures_dir, f"{names[key]}_e{epoch}_b{i}.png")
            if hasattr(im, "save"):
                im.save(path)
            else:                                            # without Pillow the helper returns an H x W x 4 array
                import matplotlib.image
                matplotlib.image.imsave(path, im)
            history["figures"].append(path)


def _run_extras(model, val_loader, device, epoch, val_epochs, history, rank0, opts):
    """What a validation epoch adds beside its scalars, in this order: tile table, land-cover table, time series, figures.  The
    files are rank 0's to write under data parallel; every rank keeps the time series in its history."""
    def due(every):
        return val_epochs % max(int(every), 1) == 0
    if opts["tile_table_path"] is not None and rank0:
        from validation_utils.tile_metrics import evaluate_tiles
        if opts.get("masked"):
            from functools import partial
            evaluate_tiles = partial(evaluate_tiles, masked=True)
        _write_table(evaluate_tiles, model, val_loader, device, opts["tile_table_path"], opts["tile_table_crop"], epoch)
    if opts["land_cover_table_path"] is not None and rank0:
        from validation_utils.land_cover import evaluate_land_cover
        _write_table(evaluate_land_cover, model, val_loader, device, opts["land_cover_table_path"], opts["land_cover_crop"], epoch)
    if opts["time_series"] is not None and due(opts["time_series_every"]):
        history["time_series"].append(_time_series(model, opts["time_series"], device, epoch))
    if opts["figures_dir"] is not None and due(opts["figures_every"]) and rank0:
        _write_figures(model, val_loader, device, opts["figures_dir"], epoch, history)


def _baseline_kind(model, reducer):
    """model.baseline_models.Linear_NIR / MLP_NIR (train.py:47-54 with --baseline): ONE optimizer, no scheduler
    (baseline_models.py:69-70, :138-139); the checkpoint keeps Lightning's layout with one entry in ``optimizer_states``."""
    if reducer is not None:
        raise NotImplementedError("data-parallel training of the baseline models is not on the MI355X path")
    optim = model.configure_optimizers()

    def restore(ck):
        model.load_state_dict(ck["state_dict"], strict=True)
        model._flat().touch()
        if "optimizer_states" in ck:
            optim.load_state_dict(ck["optimizer_states"][0])
            model.lr = optim.param_groups[0]["lr"]
    return SimpleNamespace(restore=restore, after_val=lambda val: None, lr=lambda: {"lr": model.lr},
                           states=lambda: {"optimizer_states": [optim.state_dict()], "lr_schedulers": []})


def _px2px_kind(model, reducer):
    """model.pix2pix.Px2Px_PL: two optimizers (order of configure_optimizers: [D, G], pix2pix.py:490) and ReduceLROnPlateau on
    ``Schedulers.metric`` for both, interval 'epoch' (pix2pix.py:488-492); the fused trainer takes the learning rates over."""
    trainer = model.fused_trainer(reducer=reducer)
    (optim_d, optim_g), scheds = model.configure_optimizers()
    sched_d, sched_g = scheds[0]["scheduler"], scheds[1]["scheduler"]
    monitor = scheds[0]["monitor"]

    def hand_over():
        trainer.lr_d, trainer.lr_g = optim_d.param_groups[0]["lr"], optim_g.param_groups[0]["lr"]

    def restore(ck):
        model.load_state_dict(ck["state_dict"], strict=False)
        trainer.flatG.touch()
        trainer.flatD.touch()
        if "optimizer_states" in ck:
            optim_d.load_state_dict(ck["optimizer_states"][0])
            optim_g.load_state_dict(ck["optimizer_states"][1])
            hand_over()
        for sch, sd in zip((sched_d, sched_g), ck.get("lr_schedulers", [])):
            sch.load_state_dict(sd)

    def after_val(val):
        if monitor in val:
            sched_d.step(val[monitor])
            sched_g.step(val[monitor])
            hand_over()
    return SimpleNamespace(restore=restore, after_val=after_val,
                           lr=lambda: {"lr_d": trainer.lr if trainer.lr_d is None else trainer.lr_d,
                                       "lr_g": trainer.lr if trainer.lr_g is None else trainer.lr_g},
                           states=lambda: {"optimizer_states": [optim_d.state_dict(), optim_g.state_dict()],
                                           "lr_schedulers": [sched_d.state_dict(), sched_g.state_dict()]})


def fit(model, train_loader: Iterable[dict], val_loader: Optional[Iterable[dict]] = None, *, max_epochs: int = 1,
        device=None, reducer=None, log_every: int = 10, on_log: Optional[Callable[[Dict[str, float]], None]] = None,
        ckpt_path: Optional[str] = None, resume_from: Optional[str] = None, tile_table_path: Optional[str] = None,
        tile_table_crop: Optional[int] = 240, time_series=None, time_series_every: int = 1,
        figures_dir: Optional[str] = None, figures_every: int = 1, land_cover_table_path: Optional[str] = None,
        land_cover_crop: Optional[int] = 240, masked_validation: bool = False) -> Dict[str, list]:
    """Train ``model`` (model.pix2pix.Px2Px_PL, or a model.baseline_models baseline: _baseline_kind).  Returns the history
    {'train': [...], 'val': [...], 'lr': [...]}.  ``tile_table_path`` (default None: nothing changes): per validation epoch, the
    per-tile table of the validation batches as CSV, evaluated on the centred ``tile_table_crop`` window (None: whole tiles).
    ``time_series`` (default None: nothing changes): a glob of date rasters (validation_utils.get_pred_nirs_and_info) or a
    ``(rgbs [T,3,H,W], nirs [T,1,H,W])`` pair; every ``time_series_every`` validation epochs ``ndvi_timeline``'s dict of the stack
    under the current model (plus ``epoch``) is appended to ``history["time_series"]``.  ``figures_dir`` (default None: nothing
    changes): every ``figures_every`` validation epochs the validation figures (``model.validation_figures``) of the first
    ``Logging.num_val_images`` validation batches are written there as ``val_nir_e<epoch>_b<i>.png`` / ``val_ndvi_e<epoch>_b<i>.png``
    (rank 0 under data parallel) and the paths appended to ``history["figures"]``.  ``land_cover_table_path`` (default None: nothing
    changes): per validation epoch, the land-cover-stratified table (validation_utils.evaluate_land_cover) of the validation batches,
    which must then carry a ``mask`` of class ids, on the centred ``land_cover_crop`` window as ``<stem>_e<epoch><ext>`` (rank 0 under
    data parallel).  ``masked_validation`` (default False: nothing changes): the validation batches carry ``valid``
    (``grid_loader(.., return_valid=True)``) and the ``val/*`` scalars are those over the valid pixels of each batch
    (``calculate_metrics(.., valid=)``; the model's ``masked_validation`` attribute is set for the run and restored), the tile table
    of ``tile_table_path`` is the masked one, and the epoch value of each key is its mean over the batches where it is finite.  A key
    without a finite batch is NaN, is not handed to the scheduler, and is listed in ``history["val_not_finite"]``."""
    device = device or next(model.parameters()).device
    extras = dict(tile_table_path=tile_table_path, tile_table_crop=tile_table_crop, time_series=time_series,
                  time_series_every=time_series_every, figures_dir=figures_dir, figures_every=figures_every,
                  land_cover_table_path=land_cover_table_path, land_cover_crop=land_cover_crop, masked=bool(masked_validation))
    run = (model, train_loader, val_loader, max_epochs, device, reducer, log_every, on_log, ckpt_path, resume_from, extras)
    if not masked_validation:
        return _fit(*run)
    was = getattr(model, "masked_validation", False)
    model.masked_validation = True
    try:
        return _fit(*run)
    finally:
        model.masked_validation = was


def _val_scalars(model, val_loader, device):
    """the epoch's ``val/*`` scalars: per key the mean over the validation batches"""
    sums, n = {}, 0
    for i, batch in enumerate(val_loader):
        model.logged.clear() if hasattr(model, "logged") else None
        model.validation_step(_to_device(batch, device), i)
        for k, v in getattr(model, "logged", {}).items():
            if k.startswith("val/"):
                sums[k] = sums.get(k, 0.0) + float(v)
        n += 1
    return {k: _rank_mean(v / max(n, 1), device) for k, v in sums.items()}


def _masked_val_scalars(model, val_loader, device):
    """the epoch's ``val/*`` scalars under masked validation: per key the mean over the batches where its value is finite (a batch
    without a valid pixel gives NaN), NaN for a key with no such batch"""
    sums, counts = {}, {}
    for i, batch in enumerate(val_loader):
        model.logged.clear() if hasattr(model, "logged") else None
        model.validation_step(_to_device(batch, device), i)
        for k, v in getattr(model, "logged", {}).items():
            if k.startswith("val/"):
                sums.setdefault(k, 0.0)
                counts.setdefault(k, 0)
                if math.isfinite(float(v)):
                    sums[k] += float(v)
                    counts[k] += 1
    return {k: _rank_mean(sums[k] / counts[k] if counts[k] else float("nan"), device) for k in sums}


def _fit(model, train_loader, val_loader, max_epochs, device, reducer, log_every, on_log, ckpt_path, resume_from, extras):
    time_series, figures_dir = extras["time_series"], extras["figures_dir"]
    kind = (_baseline_kind if getattr(model, "is_pixel_baseline", False) else _px2px_kind)(model, reducer)
    rank0 = reducer is None or getattr(reducer, "rank", 0) == 0
    history = {"train": [], "val": [], "lr": []}
    if time_series is not None:
        history["time_series"] = []
    if figures_dir is not None:
        history["figures"] = []
    step, first_epoch, val_epochs = 0, 0, 0
    if resume_from is not None:
        ck = torch.load(resume_from, map_location=device, weights_only=False)
        kind.restore(ck)
        step, first_epoch = int(ck.get("global_step", 0)), int(ck.get("epoch", -1)) + 1
    for epoch in range(first_epoch, max_epochs):
        if hasattr(train_loader, "set_epoch"):               # nirgan_hip.data.SceneLoader: a resumed run draws this epoch's batches
            train_loader.set_epoch(epoch)
        model.train()
        for batch in train_loader:
            view = model.train_batch(_to_device(batch, device))
            if log_every and step % log_every == 0:          # reading the losses synchronises: not every step
                rec = {"epoch": epoch, "step": step, **view.as_dict()}
                history["train"].append(rec)
                if on_log:
                    on_log(rec)
            step += 1
        if val_loader is not None:
            model.eval()
            val = (_masked_val_scalars if extras["masked"] else _val_scalars)(model, val_loader, device)
            val["epoch"] = epoch
            history["val"].append(val)
            if on_log:
                on_log(val)
            if extras["masked"]:                             # a NaN key is not the scheduler's to see
                lost = sorted(k for k, v in val.items() if not math.isfinite(v))
                if lost:
                    history.setdefault("val_not_finite", []).append({"epoch": epoch, "keys": lost})
                kind.after_val({k: v for k, v in val.items() if k not in lost})
            else:
                kind.after_val(val)
            _run_extras(model, val_loader, device, epoch, val_epochs, history, rank0, extras)
            val_epochs += 1
        history["lr"].append({"epoch": epoch, **kind.lr()})
        if ckpt_path is not None and rank0:
            torch.save({"epoch": epoch, "global_step": step, "state_dict": model.state_dict(), **kind.states()}, ckpt_path)
    return history
