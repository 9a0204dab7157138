"""``fit`` with all four per-epoch extras switched on at once (tile table, land-cover table, NDVI time series, figures), for a
``Px2Px_PL`` and for a pixel baseline, on the numpy emulators (tests/emu_class_metrics.py, the end of the chain): the extras change
nothing the loop computes, come in their order, and write their files under their names."""
import csv
import os

import pytest
import torch

import api_cases as A
import baseline_cases as Bc
import class_metric_cases as Cc
import time_series_cases as Sc
from emu_class_metrics import EmuClassMetrics
from nirgan_hip import lib as L


@pytest.fixture()
def emu():
    be = EmuClassMetrics()
    L.set_backend(be)
    yield be
    L.set_backend(None)


def _px():
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, 8)
    cfg.custom_configs.Logging.num_val_images = 1
    torch.manual_seed(0)
    return Px2Px_PL(cfg).to("cpu")


def _linear():
    m = Bc.make("linear", 0, "cpu")
    m.config.custom_configs.Logging.num_val_images = 1
    return m


@pytest.mark.parametrize("fresh", [_px, _linear], ids=["px2px", "linear"])
def test_all_four_extras_at_once_change_nothing_and_write_their_files(emu, fresh, tmp_path):
    from nirgan_hip.fit import fit
    from validation_utils.land_cover import LAND_COVER_KEYS
    from validation_utils.tile_metrics import TABLE_KEYS
    train, val = A._loaders("cpu", n_train=1, n_val=2)
    val = [dict(b, mask=Cc.masks((2, 32, 32), 24, seed=40 + i)) for i, b in enumerate(val)]
    ref = fresh()
    plain = fit(ref, train, val, max_epochs=2, log_every=1, device="cpu")
    assert list(plain) == ["train", "val", "lr"]
    assert not {"tile_metrics", "class_metrics", "window_stats", "val_panel"} & set(emu.calls)
    m = fresh()
    hist = fit(m, train, val, max_epochs=2, log_every=1, device="cpu",
               tile_table_path=str(tmp_path / "tables" / "tiles.csv"), tile_table_crop=24,
               land_cover_table_path=str(tmp_path / "tables" / "land.csv"), land_cover_crop=24,
               time_series=Sc.date_stack(T=5, size=40), figures_dir=str(tmp_path / "figs"))
    assert list(hist) == ["train", "val", "lr", "time_series", "figures"]
    for key in ("train", "val", "lr"):
        assert hist[key] == plain[key], key
    assert m.training == ref.training and not m.training
    # per epoch: tile table, land-cover table, time series (two window calls), one figure
    extras = [c for c in emu.calls if c in ("tile_metrics", "class_metrics", "window_stats", "val_panel")]
    assert extras == ["tile_metrics", "class_metrics", "window_stats", "window_stats", "val_panel"] * 2
    assert sorted(os.listdir(tmp_path / "tables")) == ["land_e0.csv", "land_e1.csv", "tiles_e0.csv", "tiles_e1.csv"]
    for epoch in (0, 1):
        rows = list(csv.reader(open(tmp_path / "tables" / f"tiles_e{epoch}.csv")))
        assert rows[0] == [""] + list(TABLE_KEYS) and [int(r[1]) for r in rows[1:]] == [0, 1, 2, 3]
        rows = list(csv.reader(open(tmp_path / "tables" / f"land_e{epoch}.csv")))
        assert rows[0] == [""] + list(LAND_COVER_KEYS)
        # tiles 0..3 in order, classes in id order; class 3 is absent from the last tile of each batch of masks
        assert [(int(r[1]), int(r[4])) for r in rows[1:]] == [(t, c) for t in range(4) for c in range(5) if not (c == 3 and t in (1, 3))]
    assert [e["epoch"] for e in hist["time_series"]] == [0, 1] and all(len(e["ndvi_true"]) == 5 for e in hist["time_series"])
    assert [os.path.basename(p) for p in hist["figures"]] == ["val_nir_e0_b0.png", "val_nir_e1_b0.png"]
    assert all(os.path.getsize(p) > 1000 for p in hist["figures"])
