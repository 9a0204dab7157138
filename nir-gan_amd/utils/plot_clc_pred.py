"""MI355X-native counterpart of the reference's ``utils/plot_clc_pred.py``: rgb, actual and predicted NIR and the CLC land-cover
mask of one tile side by side.

The reference's signature, panel titles, rgb x 5 clip, viridis 0..1 NIR panels and five-class legend are kept; its hard-coded
output path is dropped (see utils/plot_clc_utils.py): ONE host copy, drawn on Agg, the image is returned.  Not pixel-exact.
"""
from utils.plot_clc_utils import _clc_cmap, _host_planes


def plot_rgb_nir_and_mask(rgb_tensor, nir, pred_nir, mask_tensor, it=0, title=None):
    """rgb_tensor [3, H, W], nir / pred_nir [1, H, W] or [H, W], mask_tensor [H, W] class ids; returns the image.  ``it`` numbered
    the reference's output file and is unused."""
    from utils.logging_helpers import _draw
    plt, image = _draw()
    rgb, mask, n, p = _host_planes(rgb_tensor, mask_tensor, nir, pred_nir)
    _, axes = plt.subplots(1, 4, figsize=(20, 6))
    axes[0].imshow(rgb)
    axes[1].imshow(n, cmap="viridis", vmin=0, vmax=1)
    axes[2].imshow(p, cmap="viridis", vmin=0, vmax=1)
    axes[3].imshow(mask, cmap=_clc_cmap(), vmin=0, vmax=4, interpolation="nearest")
    for ax, name in zip(axes, ("RGB", "Ground Truth NIR", "Predicted NIR", "CLC Mask")):
        ax.set_title(name)
        ax.axis("off")
    if title:
        plt.suptitle(title)
    return image(plt)
