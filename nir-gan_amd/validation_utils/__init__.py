"""MI355X-native counterpart of the reference's ``validation_utils`` package: the per-tile metrics table
(get_results_table.py:59-94, spider_validation_callback.py:28-64) built on one fused device pass per batch, and the NDVI time
series (time_series_validation.py) on batched predictions and one device call per window; the land-cover-stratified table
(land_cover.py) behind the reference's CLC figures (utils/plot_clc_utils.py, utils/plot_clc_pred.py); the geo-context join of the
table to a country layer and a Koeppen raster on two device entries (geo_ablation.py) and the radar charts drawn from it
(plot_val_spiders.py)."""
from .geo_ablation import (PolygonLayer, RasterLayer, append_info_to_df, clean_economy, final_touch, get_climate_zones,  # noqa: F401
                           get_countries, points_in_regions, raster_lookup, read_geojson_table, write_geojson)
from .land_cover import CLC_CLASSES, CLC_COLORS, evaluate_land_cover, summarize_land_cover  # noqa: F401
from .plot_val_spiders import plot_radar_comparison, summarize_by  # noqa: F401
from .tile_metrics import MASKED_TABLE_KEYS, TABLE_KEYS, evaluate_tiles, spider_validation_callback  # noqa: F401
from .time_series_validation import (calculate_and_plot_timeline, get_pred_nirs_and_info, ndvi_timeline,  # noqa: F401
                                     plot_ndvi_timeline, plot_timeline)
from .val_utils import crop_center  # noqa: F401
