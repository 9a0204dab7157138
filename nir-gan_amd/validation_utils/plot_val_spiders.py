"""MI355X-native counterpart of the reference's ``validation_utils/plot_val_spiders.py``: the SatCLIP / no-SatCLIP radar charts of
the joined validation table (validation_utils/geo_ablation.py), per continent, Koeppen class or economy.

``plot_radar_comparison`` keeps the reference's signature, Koeppen label map, removal of the undetermined class, titles, legend
labels and output file name; tables are the project's dicts of lists.  It draws on the Agg backend, writes the PNG and also returns
the image through the helper of validation_utils/time_series_validation.py.  The categories are those present in BOTH tables,
sorted (the reference silently assumes both tables have the same ones).  Not pixel-exact.  The reference's module runs a script body
over hard-coded paths on import; this one has none.
"""
import math
import os

from .time_series_validation import _image, _plt

KOPPEN_LABELS = {"A": "Tropical", "B": "Arid", "C": "Temperate", "D": "Continental", "E": "Polar", "U": "Undetermined"}


def _missing(v):
    return v is None or (isinstance(v, float) and math.isnan(v))


def summarize_by(table, key, metrics=("psnr", "ssim")):
    """Per-category float64 means of ``metrics``: what ``DataFrame.groupby(key).agg("mean")`` gives -- categories sorted, rows
    without a category dropped, NaN values skipped (a category with none left gets NaN).  Returns ``{key: [categories],
    metric: [means], ..}``."""
    groups = {}
    for i, cat in enumerate(table[key]):
        if not _missing(cat):
            groups.setdefault(cat, []).append(i)
    cats = sorted(groups)
    out = {key: cats}
    for m in metrics:
        col, means = table[m], []
        for cat in cats:
            vals = [float(col[i]) for i in groups[cat] if not _missing(col[i])]
            means.append(math.fsum(vals) / len(vals) if vals else float("nan"))
        out[m] = means
    return out


def plot_radar_comparison(sc, no_sc, data_type, out_name="", folder="validation_utils/metrics_folder/"):
    """Two radar charts (PSNR, SSIM) of the per-category means of table ``sc`` (solid, "SatCLIP") against ``no_sc`` (dashed,
    "No SatCLIP"), written to ``<folder>/metrics_radar_satclip[_<out_name>]_<data_type>.png`` (blanks as underscores) and returned."""
    t1, t2 = sc, no_sc
    if data_type == "Koppen_Class":

        def relabel(t):
            keep = [i for i, v in enumerate(t["Koppen_Class"]) if v != "U"]
            out = {k: [col[i] for i in keep] for k, col in t.items()}
            out["Koppen_Class"] = [KOPPEN_LABELS.get(v, v) for v in out["Koppen_Class"]]
            return out
        t1, t2 = relabel(t1), relabel(t2)
    s1, s2 = summarize_by(t1, data_type), summarize_by(t2, data_type)
    categories = sorted(set(s1[data_type]) & set(s2[data_type]))
    if not categories:
        raise ValueError(f"plot_radar_comparison: the two tables share no '{data_type}' category")
    N = len(categories)
    angles = [n / float(N) * 2 * math.pi for n in range(N)]
    angles += angles[:1]
    plt = _plt()
    fig, (ax1, ax2) = plt.subplots(nrows=1, ncols=2, figsize=(12, 6), subplot_kw=dict(polar=True))

    def values(s, metric):
        at = {c: v for c, v in zip(s[data_type], s[metric])}
        v = [at[c] for c in categories]
        return v + v[:1]

    def plot_radar(ax, metric, title):
        ax.set_xticks(angles[:-1])
        ax.set_xticklabels([str(c) for c in categories], color="grey", size=13)
        ax.set_title(title, size=15, position=(0.5, 1.1))
        ax.plot(angles, values(s1, metric), linewidth=2, linestyle="solid", label="SatCLIP")
        ax.plot(angles, values(s2, metric), linewidth=2, linestyle="dashed", label="No SatCLIP")
        ax.legend(loc="upper right", bbox_to_anchor=(0.1, 0.1))

    plot_radar(ax1, "psnr", "PSNR")
    plot_radar(ax2, "ssim", "SSIM")
    if out_name != "":
        out_name = "_" + out_name
    name = f"metrics_radar_satclip{out_name}_{data_type}.png".replace(" ", "_")
    os.makedirs(folder, exist_ok=True)
    plt.tight_layout()
    plt.savefig(os.path.join(folder, name))
    return _image(plt)
