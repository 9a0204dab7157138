"""MI355X-native counterpart of the reference's ``utils/plot_clc_utils.py``: an rgb tile beside its CLC land-cover mask.

The reference's signature, panel titles, rgb x 5 clip and five-class legend (validation_utils.land_cover.CLC_COLORS, ``vmin=0,
vmax=4``) are kept; its hard-coded output path is dropped: the figure is drawn on the Agg backend from ONE host copy and returned
through the image helper of utils/logging_helpers.py, nothing is written.  Not pixel-exact.  The numbers behind the figure are
``validation_utils.evaluate_land_cover``.
"""
import torch


def _clc_cmap():
    from matplotlib.colors import ListedColormap
    from validation_utils.land_cover import CLC_COLORS
    return ListedColormap(list(CLC_COLORS))


def _host_planes(rgb_tensor, mask_tensor, *planes):
    """ONE host copy of a single image's tensors: rgb [3, H, W] (x 5, clipped to [0, 1]) as [H, W, 3], the mask and every further
    plane ([1, H, W] or [H, W]) as [H, W]"""
    rgb = torch.as_tensor(rgb_tensor).detach()
    if rgb.dim() != 3 or rgb.shape[0] < 3:
        raise ValueError(f"rgb_tensor must be one image [3, H, W], got {tuple(rgb.shape)}")
    H, W = rgb.shape[-2:]
    dev = rgb.device
    rest = []
    for t in (mask_tensor,) + planes:
        t = torch.as_tensor(t).detach()
        if t.numel() != H * W or t.dim() not in (2, 3):
            raise ValueError(f"mask and nir planes must be [H, W] or [1, H, W] matching rgb, got {tuple(t.shape)}")
        rest.append(t.to(dev).to(torch.float32).reshape(1, H, W))
    flat = torch.cat([(rgb[:3].to(torch.float32) * 5).clamp(0, 1)] + rest).cpu().numpy()
    return (flat[:3].transpose(1, 2, 0),) + tuple(flat[3 + i] for i in range(len(rest)))


def plot_rgb_and_mask(rgb_tensor, mask_tensor, it=0, title=None):
    """rgb_tensor [3, H, W] in [0, 1], mask_tensor [H, W] (or [1, H, W]) class ids; returns the image.  ``it`` numbered the
    reference's output file and is unused; ``title`` becomes the figure's title."""
    from utils.logging_helpers import _draw
    plt, image = _draw()
    rgb, mask = _host_planes(rgb_tensor, mask_tensor)
    _, axes = plt.subplots(1, 2, figsize=(10, 5))
    axes[0].imshow(rgb)
    axes[0].set_title("RGB Image")
    axes[1].imshow(mask, cmap=_clc_cmap(), vmin=0, vmax=4, interpolation="nearest")
    axes[1].set_title("CLC Mask")
    for ax in axes:
        ax.axis("off")
    if title:
        plt.suptitle(title)
    return image(plt)
