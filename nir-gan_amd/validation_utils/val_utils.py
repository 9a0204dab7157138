"""``crop_center`` with the reference's signature (validation_utils/val_utils.py:20-42), on numpy arrays and torch tensors."""


def crop_center(im, target_height):
    """Centre ``target_height x target_height`` crop of a ``C x H x W`` or ``H x W`` image (a view, nothing is copied).
    The crop starts at ``(H - target_height) // 2`` and ``(W - target_height) // 2``."""
    target_width = target_height
    if len(im.shape) not in (2, 3):
        raise AssertionError(f"Expected 2D or 3D array, got shape {tuple(im.shape)}")
    h, w = im.shape[-2], im.shape[-1]
    assert target_height <= h and target_width <= w, "Target size must be <= image size"
    start_h = (h - target_height) // 2
    start_w = (w - target_width) // 2
    return im[..., start_h:start_h + target_height, start_w:start_w + target_width]
