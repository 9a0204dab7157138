"""MI355X-native counterpart of the reference's ``validation_utils`` package: the per-tile metrics table
(get_results_table.py:59-94, spider_validation_callback.py:28-64) built on one fused device pass per batch.
The geo-context join (geopandas), the PNG plots and the time-series plots are out of scope."""
from .tile_metrics import TABLE_KEYS, evaluate_tiles, spider_validation_callback  # noqa: F401
from .val_utils import crop_center  # noqa: F401
