"""Training batches from device-resident scenes: the entries of csrc/scenesample.hip seen from Python.

The reference reads a tile per item through rasterio, ``.astype(np.float32) / 10000``, bands 0..2 = RGB, band 3 = NIR, ``coords`` =
lon / lat of the centre pixel (data/SR_dataset_RGB.py:24-56).  Here the scenes are uploaded ONCE as they are stored (uint16 or
float32, planar) and every batch is cut, normalised, mirrored / rotated and georeferenced on the device by ``nirgan_scene_sample``:
two launches, no host synchronisation.  Which windows a batch holds is a pure function of ``(seed, draw, sample index)`` (Philox4x32-10,
as the dropout mask): a step can be drawn again, a resumed run draws what the uninterrupted run would have drawn, and ranks need no
shared state -- rank r takes samples ``r * batch_size ..`` of the same logical batch.

    pool = ScenePool(scenes, nodata=0, geotransforms=geo)          # or ScenePool.from_npz(paths)
    fit(model, pool.loader(16, 256, steps_per_epoch=1000, seed=1), max_epochs=10)

With ``scales`` every sample also draws a resolution factor f, cuts an f*T window and is delivered as the T x T tile of its f x f block
means (``nirgan_scene_sample_scaled``): a 10 m pool then trains on 10, 20, 30 and 40 m tiles, mixed by integer weights:

    pool.loader(16, 256, steps_per_epoch=1000, seed=1, scales=(1, 2, 3, 4), scale_weights=(4, 2, 1, 1))

Validation wants the SAME windows at every epoch: ``grid`` lists a fixed, non-overlapping grid of windows over the scenes (filtered by
the sampler's nodata rule, at any of the factors), ``gather`` cuts an explicit list of windows through ``nirgan_scene_gather`` -- also
the ``"window"`` rows of a sampled batch, bitwise as sampled -- and ``grid_loader`` is the re-iterable over a grid that ``fit`` and
``evaluate_tiles`` take as their validation data.  The training sampler draws ANYWHERE in its pool, so a grid is held
out only if it comes from a separate pool of held-out scenes, or from the two halves of ``pool.split(...)``:

    val_loader = val_pool.grid_loader(16, 256, factors=(1, 2), max_invalid=0)
    fit(model, pool.loader(16, 256, steps_per_epoch=1000, seed=1, scales=(1, 2)), val_loader, max_epochs=10)

``split`` holds rectangles of a pool's scenes out (``split_blocks`` picks them on a block lattice): ``split.train`` samples through
``nirgan_scene_sample_origins``, whose draw runs over a table of the admissible window ORIGINS -- no window it can name touches a
held-out rectangle (widened by ``guard`` pixels), whatever the nodata attempts do, and every admissible window is equally likely;
``split.val`` lists the grid windows lying fully inside one held-out rectangle.  Both halves share the pool's buffers:

    split = pool.split_blocks(512, 0.2, seed=3, guard=16)
    fit(model, split.train.loader(16, 256, steps_per_epoch=1000, seed=1, scales=(1, 2)),
        split.val.grid_loader(16, 256, factors=(1, 2)), max_epochs=10)

``pool.predict(model, s, ...)`` is the inference side: the NIR band of scene ``s`` through ``nirgan_hip.inference.predict_scene``,
read in place from the pool's buffer.

With ``max_invalid > 0`` a window is delivered with its nodata pixels as ordinary values.  ``return_valid=True`` (``sample``,
``loader``, ``gather``, ``grid_loader``, on the pool and on both halves of a split) adds ``"valid"`` [B,1,T,T] to the batch: 1 where the
pixel's source block is clean, from the prefix tables in one ``nirgan_scene_valid`` launch.  ``train_batch`` /
``Pix2PixTrainer.step(..., valid=)`` then keep the other pixels out of L1 and the index losses:

    fit(model, pool.loader(16, 256, steps_per_epoch=1000, seed=1, max_invalid=256 * 256 // 2, return_valid=True), max_epochs=10)

Reading ``.tif`` is out of scope (no rasterio here): convert once to ``.npz``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as L
from .dropout import split_seed

_DTYPES = {np.dtype(np.uint16): L.SCENE_U16, np.dtype(np.float32): L.SCENE_F32}


def _as_array(scene) -> np.ndarray:
    if torch.is_tensor(scene):
        scene = scene.detach().cpu().numpy()
    a = np.ascontiguousarray(scene)
    if a.ndim != 3:
        raise ValueError(f"a scene is [C, H, W], got shape {a.shape}")
    return a


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def _is_integer(x, lo) -> bool:
    """whether ``x`` is an integer -- no bool, no fraction -- of at least ``lo``"""
    return not isinstance(x, bool) and x == int(x) and int(x) >= lo


def _side(what, f, tile) -> int:
    """the side ``f * tile`` of the source window of ``what`` (scale / factor) f; the entries take windows below 2^31 pixels"""
    if (f * tile) ** 2 >= 2 ** 31:
        raise ValueError(f"{what} {f}: the window ({f} * {tile})^2 has 2^31 pixels or more")
    return f * tile


def _fill(d, pool, table, out, tile, draw=None):
    """The descriptor fields every scene entry shares: pool, table (device, host), geo, band, tile, divisor and the outputs; with
    ``draw`` = (B, augment, seed, draw, sample0, max_invalid) also what the three samplers share beyond that."""
    d.pool, d.pool_elems, d.dtype, d.S, d.C = pool.pool.data_ptr(), pool.pool_elems, pool.dtype, len(pool.shapes), pool.C
    d.table, d.table_host = table[0].data_ptr(), table[1].ctypes.data
    d.geo = pool.geo.data_ptr() if pool.geo is not None else None
    d.band = (C.c_int * 4)(*pool.bands)
    d.tile, d.divisor = tile, pool.divisor
    d.rgb, d.nir = out["rgb"].data_ptr(), out["nir"].data_ptr()
    d.coords = out["coords"].data_ptr() if pool.geo is not None else None
    if draw is not None:
        d.B, augment, seed, number, sample0, max_invalid = draw
        d.prefix, d.prefix_elems = (pool.prefix.data_ptr() if pool.prefix is not None else None), pool.prefix_elems
        d.views = L.SCENE_VIEWS[augment]
        d.seed_lo, d.seed_hi = split_seed(seed)
        d.draw, d.sample0, d.max_invalid = int(number) & ((1 << 64) - 1), int(sample0) & 0xFFFFFFFF, int(max_invalid)
        d.window = out["window"].data_ptr()


def _valid_out(pool, out, n, tile):
    """``out["valid"]``, a contiguous float32 [n, 1, T, T] tensor on the pool's device, made if ``out`` holds none"""
    t = out.get("valid")
    if t is None:
        t = out["valid"] = torch.empty((n, 1, tile, tile), dtype=torch.float32, device=pool.device)
    if tuple(t.shape) != (n, 1, tile, tile) or t.dtype != torch.float32 or t.device != pool.pool.device or not t.is_contiguous():
        raise ValueError(f"out['valid'] must be a contiguous float32 {(n, 1, tile, tile)} tensor on {pool.pool.device}")
    return t


def _scene_valid(pool, tile, window, window_host, n_windows, first, n, valid):
    """One ``nirgan_scene_valid`` launch: the mask of rows ``first .. first + n - 1`` of the device rows ``window`` into
    ``valid``.  ``window_host``: the same rows as a numpy array, or None -- the rows of a draw, which the kernel bounds itself."""
    d = L.SceneValidDesc()
    table = pool._table(tile)                                                    # columns 1, 2, 4 are read: the table of any side will do
    d.S, d.table, d.table_host = len(pool.shapes), table[0].data_ptr(), table[1].ctypes.data
    d.prefix, d.prefix_elems = (pool.prefix.data_ptr() if pool.prefix is not None else None), pool.prefix_elems
    d.tile, d.window, d.window_host = tile, window.data_ptr(), (window_host.ctypes.data if window_host is not None else None)
    d.n_windows, d.first, d.n, d.valid = n_windows, first, n, valid.data_ptr()
    L.call("nirgan_scene_valid", C.byref(d), _stream(pool.device))


def _fill_scales(d, factors, weights):
    d.K = len(factors)
    d.factor, d.weight = (C.c_int * 8)(*factors), (C.c_uint32 * 8)(*weights)


class _Sampler:
    """``sample`` and ``loader`` of ``ScenePool`` and ``SplitTrain``.  A subclass has a ``device``, makes the output tensors in
    ``_outputs`` and names its entry and descriptor in ``_describe``."""

    def sample(self, batch_size, tile, *, seed, draw, sample0=0, augment="d4", max_invalid=0, return_windows=False, out=None,
               scales=None, scale_weights=None, return_valid=False):
        """One batch ``{"rgb" [B,3,T,T], "nir" [B,1,T,T][, "coords" [B,2]]}``, plus ``"window"`` [B,4] int32 = (scene, y0, x0,
        view | attempt << 8 | (factor - 1) << 16 | exhausted << 31) with ``return_windows``.  Sample b is a function of ``(seed, draw,
        sample0 + b)`` alone.  ``augment``: "d4" (8 views), "flips" (4) or "none".  ``max_invalid``: the most invalid pixels a window
        may hold (only with ``nodata``); after 8 rejected attempts the last window is returned and bit 31 of its window word is set.
        ``out``: the tensors to write into (the dict of an earlier call with ``return_windows`` and the same shapes) instead of new ones.
        ``scales``: distinct resolution factors in 1 .. 8 (sorted before use), one drawn per sample with the positive integer
        ``scale_weights`` (default: all 1); the sample is then an f*T window of the source (y0, x0 in source pixels, ``max_invalid``
        per f x f block, coords of the window's centre) delivered as the T x T tile of its f x f block means.  None: factor 1 -- a
        ``ScenePool`` through ``nirgan_scene_sample``, as ever; a ``SplitTrain`` through its one entry.
        ``return_valid``: the batch also carries ``"valid"`` [B,1,T,T] float32, 1 where the pixel's f x f source block holds no invalid
        pixel and 0 elsewhere, in the orientation of the delivered pixels (all ones without ``nodata``): one ``nirgan_scene_valid``
        launch on the rows the draw just wrote, no copy to the host.  ``Pix2PixTrainer.step(..., valid=)`` and the
        losses' ``valid=`` take it."""
        if augment not in L.SCENE_VIEWS:
            raise ValueError(f"augment must be one of {sorted(L.SCENE_VIEWS)}, got {augment!r}")
        B, tile = int(batch_size), int(tile)
        if B <= 0 or tile <= 0:
            raise ValueError("batch_size and tile must be positive")
        out = out if out is not None else self._outputs(B, tile)
        entry, d = self._describe(out, B, tile, seed, draw, sample0, augment, max_invalid, scales, scale_weights)
        pool = self if isinstance(self, ScenePool) else self.pool               # the ScenePool itself, or a SplitTrain's
        if return_valid:
            valid = _valid_out(pool, out, B, tile)
        L.call(entry, C.byref(d), _stream(self.device))
        if return_valid:
            _scene_valid(pool, tile, out["window"], None, B, 0, B, valid)
        drop = [k for k, keep in (("window", return_windows), ("valid", return_valid)) if not keep and k in out]
        return {k: v for k, v in out.items() if k not in drop} if drop else out

    def loader(self, batch_size, tile, steps_per_epoch, *, seed, augment="d4", max_invalid=0, rank=0, world=1, scales=None,
               scale_weights=None, return_valid=False):
        """``SceneLoader`` over this source: it only asks for ``_outputs`` and ``sample``"""
        return SceneLoader(self, batch_size, tile, steps_per_epoch, seed=seed, augment=augment, max_invalid=max_invalid, rank=rank,
                           world=world, scales=scales, scale_weights=scale_weights, return_valid=return_valid)


def _grid(pool, regions, tile, factors, stride, max_invalid, cover, nothing_left):
    """The grid of ``ScenePool.grid`` over regions ``(scene, y0, x0, h, w)``: whole scenes there, held-out rectangles in
    ``SplitVal.grid``.  ``regions``: a callable, asked once the other arguments have passed; ``nothing_left``: how the ValueError of an
    empty grid ends."""
    tile = int(tile)
    if tile <= 0:
        raise ValueError("tile must be positive")
    factors, _ = check_scales(factors)
    if stride is not None and not _is_integer(stride, 1):
        raise ValueError(f"stride must be an integer of at least 1 (source pixels), got {stride!r}")
    if not _is_integer(max_invalid, 0):
        raise ValueError(f"max_invalid must be a non-negative integer, got {max_invalid!r}")
    regions = regions()
    parts, keeps = [], []
    for f in factors:
        side = _side("factor", f, tile)
        step = side if stride is None else int(stride)
        for s, y0, x0, h, w in regions:
            if h < side or w < side:
                continue
            yy, xx = np.meshgrid(y0 + _grid_starts(h, side, step, cover), x0 + _grid_starts(w, side, step, cover), indexing="ij")
            part = np.empty((yy.size, 4), dtype=np.int32)
            part[:, 0], part[:, 1], part[:, 2], part[:, 3] = s, yy.reshape(-1), xx.reshape(-1), (f - 1) << 16
            parts.append(part)
            if pool.prefix is not None:
                P = pool.invalid_prefix(s)
                y, x = (torch.from_numpy(part[:, c].astype(np.int64)).to(pool.device) for c in (1, 2))
                count = P[y + side, x + side].long() - P[y, x + side].long() - P[y + side, x].long() + P[y, x].long()
                keeps.append(count <= int(max_invalid) * f * f)
    rows = np.concatenate(parts) if parts else np.empty((0, 4), dtype=np.int32)
    if keeps:
        rows = rows[torch.cat(keeps).cpu().numpy()]                              # the one copy to the host
    if not len(rows):
        raise ValueError(f"the grid is empty: no window of tile {tile} at factors {factors} {nothing_left}")
    return WindowList(rows, pool.device)


def _grid_loader(pool, grid, batch_size, tile, rank, world, return_valid=False, **kw):
    """``GridLoader`` over this rank's rows of ``grid(tile, **kw)``: the rows i with ``i % world == rank``, in order"""
    if not 0 <= int(rank) < int(world):
        raise ValueError(f"rank {rank} outside 0 .. world-1 = {int(world) - 1}")
    full = grid(tile, **kw)
    mine = full if int(world) == 1 else WindowList(full.host[int(rank)::int(world)], pool.device)
    return GridLoader(pool, mine, batch_size, tile, return_valid=return_valid)


class ScenePool(_Sampler):
    """``scenes``: a list of [C, H, W] arrays or tensors, all uint16 or all float32, with one C >= 4; uploaded once into one exactly
    sized device buffer.  ``bands``: the source planes of R, G, B, NIR.  ``divisor``: what every value is divided by (float32).
    ``nodata``: if given, a pixel is invalid where any selected band equals it (uint16) or is NaN (float32; the value itself is not
    used), and a 2-D prefix count of invalid pixels is built per scene (4 bytes per pixel) so that ``sample`` can reject windows.
    ``geotransforms``: per scene ``(lon0, dlon, lat0, dlat)``, the outer corner of pixel [0][0] and the per-pixel steps of an
    axis-aligned EPSG:4326 grid; batches then carry ``coords``."""

    def __init__(self, scenes, *, bands=(0, 1, 2, 3), divisor=10000.0, nodata=None, geotransforms=None, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda" and not L.is_emulated():
            raise RuntimeError("ScenePool: the pool must live on the MI355X (cuda); the HIP path has no CPU fallback")
        arrays = [_as_array(s) for s in scenes]
        if not arrays:
            raise ValueError("ScenePool needs at least one scene")
        dt = arrays[0].dtype
        if dt not in _DTYPES or any(a.dtype != dt for a in arrays):
            raise ValueError("scenes must be all uint16 or all float32")
        self.C = int(arrays[0].shape[0])
        if self.C < 4 or any(a.shape[0] != self.C for a in arrays):
            raise ValueError("every scene needs the same number of bands, at least 4")
        self.bands = tuple(int(b) for b in bands)
        if len(self.bands) != 4 or any(not 0 <= b < self.C for b in self.bands):
            raise ValueError(f"bands must name four planes in 0 .. {self.C - 1}")
        self.divisor = float(divisor)
        if not self.divisor or self.divisor != self.divisor:
            raise ValueError("divisor must be a non-zero number")
        self.dtype = _DTYPES[dt]
        self.shapes = [(int(a.shape[1]), int(a.shape[2])) for a in arrays]
        sizes = [a.size for a in arrays]
        self.offsets = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        self.pool_elems = int(sum(sizes))
        as_int16 = dt == np.uint16                                               # bit patterns: the kernels read uint16
        self.pool = torch.empty(self.pool_elems, dtype=torch.int16 if as_int16 else torch.float32, device=self.device)
        for a, off in zip(arrays, self.offsets):                                 # scene by scene: no second host copy of the whole set
            flat = a.reshape(-1)
            self.pool[off:off + a.size].copy_(torch.from_numpy(flat.view(np.int16) if as_int16 else flat))
        self.geo = None
        if geotransforms is not None:
            g = np.ascontiguousarray(np.asarray(geotransforms, dtype=np.float64)).reshape(-1, 4)
            if g.shape[0] != len(arrays):
                raise ValueError(f"{g.shape[0]} geotransforms for {len(arrays)} scenes")
            self.geo = torch.from_numpy(g.copy()).to(self.device)
        self.nodata = nodata
        self.prefix, self.prefix_offsets, self.prefix_elems = None, [-1] * len(arrays), 0
        if nodata is not None:
            self._build_prefix()
        self._tables = {}                                                        # tile -> (device table, host table)

    @classmethod
    def from_npz(cls, paths, key="data", geo_key="geotransform", **kw):
        """One scene per ``.npz`` file: ``key`` holds [C, H, W]; ``geo_key`` (if every file has it) the four geotransform numbers."""
        scenes, geo = [], []
        for path in ([paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else paths):
            with np.load(path) as z:
                scenes.append(np.ascontiguousarray(z[key]))
                if geo_key is not None and geo_key in z.files:
                    geo.append(np.asarray(z[geo_key], dtype=np.float64).reshape(4))
        if geo and len(geo) != len(scenes):
            raise ValueError(f"only {len(geo)} of {len(scenes)} files hold '{geo_key}'")
        kw.setdefault("geotransforms", geo or None)
        return cls(scenes, **kw)

    def __len__(self):
        return len(self.shapes)

    def _build_prefix(self):
        sizes = [(h + 1) * (w + 1) for h, w in self.shapes]
        self.prefix_offsets = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        self.prefix_elems = int(sum(sizes))
        self.prefix = torch.empty(self.prefix_elems, dtype=torch.int32, device=self.device)
        for (h, w), off, poff in zip(self.shapes, self.offsets, self.prefix_offsets):
            d = L.ScenePrefixDesc()
            d.pool, d.pool_elems, d.dtype, d.offset = self.pool.data_ptr(), self.pool_elems, self.dtype, off
            d.C, d.H, d.W = self.C, h, w
            d.band = (C.c_int * 4)(*self.bands)
            d.nodata = int(self.nodata) if self.dtype == L.SCENE_U16 else 0
            d.prefix = self.prefix.data_ptr() + 4 * poff
            L.call("nirgan_scene_invalid_prefix", C.byref(d), _stream(self.device))

    def invalid_prefix(self, scene: int) -> torch.Tensor:
        """The [(H+1), (W+1)] int32 prefix counts of invalid pixels of one scene (a view; None without ``nodata``)."""
        if self.prefix is None:
            return None
        h, w = self.shapes[scene]
        off = self.prefix_offsets[scene]
        return self.prefix[off:off + (h + 1) * (w + 1)].view(h + 1, w + 1)

    def windows(self, tile: int, factor: int = 1) -> int:
        """How many windows the pool holds for tiles of side ``tile`` at resolution factor ``factor`` (source side ``factor * tile``)."""
        return int(self._table(int(factor) * int(tile))[1][-1, 3])

    @staticmethod
    def window_factor(window):
        """The resolution factor of each row of a ``"window"`` tensor or array [..., 4]: bits 16 .. 18 of the last word, plus 1."""
        return ((window[..., 3] >> 16) & 7) + 1

    def _table(self, tile: int):
        tile = int(tile)
        if tile not in self._tables:
            t = np.empty((len(self.shapes), L.SCENE_TABLE_COLS), dtype=np.int64)
            total = 0
            for s, ((h, w), off, poff) in enumerate(zip(self.shapes, self.offsets, self.prefix_offsets)):
                if h >= tile and w >= tile:
                    total += (h - tile + 1) * (w - tile + 1)
                t[s] = (off, h, w, total, poff)
            self._tables[tile] = (torch.from_numpy(t.copy()).to(self.device), t)
        return self._tables[tile]

    def _scaled_tables(self, tile: int, factors):
        """the tables of the sides ``f * tile`` stacked to [K][S][cols], on the device and on the host"""
        key = (int(tile), tuple(factors))
        if key not in self._tables:
            t = np.stack([self._table(f * int(tile))[1] for f in factors])
            self._tables[key] = (torch.from_numpy(t.copy()).to(self.device), t)
        return self._tables[key]

    def _outputs(self, B, tile):
        out = {"rgb": torch.empty((B, 3, tile, tile), dtype=torch.float32, device=self.device),
               "nir": torch.empty((B, 1, tile, tile), dtype=torch.float32, device=self.device),
               "window": torch.empty((B, 4), dtype=torch.int32, device=self.device)}
        if self.geo is not None:
            out["coords"] = torch.empty((B, 2), dtype=torch.float32, device=self.device)
        return out

    def _describe(self, out, B, tile, seed, draw, sample0, augment, max_invalid, scales, scale_weights):
        """(name of the entry, its descriptor) of one checked ``sample`` call writing into ``out``"""
        if scales is None:
            if scale_weights is not None:
                raise ValueError("scale_weights without scales")
            entry, d, table = "nirgan_scene_sample", L.SceneSampleDesc(), self._table(tile)
            if int(table[1][-1, 3]) == 0:
                raise ValueError(f"no scene of the pool holds a {tile} x {tile} window")
        else:
            entry, d = "nirgan_scene_sample_scaled", L.SceneScaledDesc()
            factors, weights = check_scales(scales, scale_weights)
            for f in factors:
                _side("scale", f, tile)
            table = self._scaled_tables(tile, factors)
            for f, t in zip(factors, table[1]):
                if int(t[-1, 3]) == 0:
                    raise ValueError(f"scale {f}: no scene of the pool holds a {f * tile} x {f * tile} window")
            _fill_scales(d, factors, weights)
        _fill(d, self, table, out, tile, (B, augment, seed, draw, sample0, max_invalid))
        return entry, d

    def grid(self, tile, *, factors=(1,), stride=None, max_invalid=0, cover=True, scenes=None) -> "WindowList":
        """A fixed, deterministic list of windows over the scenes, for ``gather`` and ``grid_loader``.  ``factors``:
        distinct resolution factors in 1 .. 8, used in ascending order; a factor f cuts windows of side L = f * tile.  ``stride``: the
        step between windows in SOURCE pixels (default L: no overlap; at least 1).  A scene with H >= L and W >= L gives the rows
        0, stride, 2 * stride, ... <= H - L, with ``cover`` also H - L if that is not the last one already (the far edge is then
        covered by one overlapping row), and the columns by the same rule; a smaller scene gives nothing.  ``scenes``: the scene
        indices to use, in this order (default: all).  Order of the list: factor, then scene, then row, then column.  With ``nodata`` a
        window is kept iff it holds at most ``max_invalid * f * f`` invalid pixels, the scaled sampler's rule; without, all are kept.
        Every word is ``(f - 1) << 16``: view 0.  The filter runs on the device on the scenes' prefix tables (four gathers per scene
        and factor) and its verdicts come back in ONE copy, the only synchronisation; a pool without ``nodata`` needs none.
        ValueError if no window is left."""
        def regions():
            ids = list(range(len(self.shapes))) if scenes is None else [int(s) for s in scenes]
            if any(not 0 <= s < len(self.shapes) for s in ids):
                raise ValueError(f"scenes must name scenes in 0 .. {len(self.shapes) - 1}, got {list(scenes)}")
            return [(s, 0, 0) + self.shapes[s] for s in ids]
        return _grid(self, regions, tile, factors, stride, max_invalid, cover, "is left on these scenes")

    def gather(self, windows, tile, *, first=0, count=None, out=None, return_valid=False):
        """``{"rgb" [n,3,T,T], "nir" [n,1,T,T][, "coords" [n,2]]}`` of the rows ``first .. first + count - 1`` (default: to the end) of
        an explicit list of windows, through ``nirgan_scene_gather``: bitwise what ``sample`` delivered for the same window rows.
        ``windows``: a ``WindowList`` (of ``grid``), or any int32 tensor or array [n, 4] of (scene, y0, x0, word) rows such as the
        ``"window"`` of ``sample(..., return_windows=True)``; an array or tensor is wrapped in a ``WindowList`` on every call, which
        costs a tensor on the device one copy to the host (a synchronisation) -- wrap it once yourself to cut it repeatedly.
        ``tile``: the side T of the delivered tiles; a row of factor f cuts f*T source pixels.  ``out``: the dict of tensors to write
        into (same shapes) instead of new ones.  ``return_valid``: also ``"valid"`` [n,1,T,T], the mask of ``sample(...,
        return_valid=True)`` for the same rows, bitwise; the rows' host copy is checked as the gather checks it."""
        if self.device.type != "cuda" and not L.is_emulated():
            raise RuntimeError("ScenePool.gather: the pool must live on the MI355X (cuda); the HIP path has no CPU fallback")
        wl = windows if isinstance(windows, WindowList) else WindowList(windows, self.device)
        if wl.device.device != self.pool.device:
            raise ValueError(f"the windows live on {wl.device.device}, the pool on {self.pool.device}")
        tile, first = int(tile), int(first)
        n = len(wl) - first if count is None else int(count)
        if tile <= 0 or first < 0 or n <= 0 or first + n > len(wl):
            raise ValueError(f"tile must be positive and rows [{first}, {first + n}) a non-empty part of the {len(wl)} windows")
        if out is None:
            out = {k: v for k, v in self._outputs(n, tile).items() if k != "window"}
        for k, shape in (("rgb", (n, 3, tile, tile)), ("nir", (n, 1, tile, tile))) + ((("coords", (n, 2)),) if self.geo is not None else ()):
            t = out[k]
            if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.pool.device or not t.is_contiguous():
                raise ValueError(f"out[{k!r}] must be a contiguous float32 {shape} tensor on {self.pool.device}")
        d = L.SceneGatherDesc()
        _fill(d, self, self._table(tile), out, tile)                             # columns 0 .. 2 are read: the table of any side will do
        d.window, d.window_host, d.n_windows, d.first, d.n = wl.device.data_ptr(), wl.host.ctypes.data, len(wl), first, n
        if return_valid:
            valid = _valid_out(self, out, n, tile)
        L.call("nirgan_scene_gather", C.byref(d), _stream(self.device))
        if return_valid:
            _scene_valid(self, tile, wl.device, wl.host, len(wl), first, n, valid)
        keys = ("rgb", "nir", "coords") + (("valid",) if return_valid else ())
        return {k: out[k] for k in keys if k in out and (k != "coords" or self.geo is not None)}

    def grid_loader(self, batch_size, tile, *, factors=(1,), stride=None, max_invalid=0, cover=True, scenes=None, rank=0, world=1,
                    return_valid=False):
        """``GridLoader`` over ``grid(tile, ...)``: a fixed validation set.  Rank ``rank`` of ``world`` takes the rows i of the grid
        with ``i % world == rank``, in order."""
        return _grid_loader(self, self.grid, batch_size, tile, rank, world, return_valid, factors=factors, stride=stride,
                            max_invalid=max_invalid, cover=cover, scenes=scenes)

    def scene(self, s: int) -> torch.Tensor:
        """Scene ``s`` as a [C, H, W] VIEW of the pool's buffer (int16 bit patterns of a uint16 pool); nothing is copied."""
        if not 0 <= int(s) < len(self.shapes):
            raise ValueError(f"scene {s} outside 0 .. {len(self.shapes) - 1}")
        (h, w), off = self.shapes[int(s)], self.offsets[int(s)]
        return self.pool[off:off + self.C * h * w].view(self.C, h, w)

    def predict(self, model, s: int, **kw) -> torch.Tensor:
        """The predicted NIR band [H, W] of scene ``s``: ``nirgan_hip.inference.predict_scene`` on a view of the pool's buffer with
        the pool's first three ``bands``, its ``divisor``, ``nodata`` and the scene's geotransform row.  ``kw``: the
        other keywords of ``predict_scene`` (tile, margin, overlap, window, batch, tta, embeds, out, scale, nodata_out, match,
        match_nodata)."""
        from .inference import predict_scene
        fixed = {"bands", "divisor", "nodata", "geotransform"} & set(kw)
        if fixed:
            raise TypeError(f"ScenePool.predict: {sorted(fixed)} come from the pool")
        view = self.scene(s)
        return predict_scene(model, view, bands=self.bands[:3], divisor=self.divisor, nodata=self.nodata,
                             geotransform=None if self.geo is None else self.geo[int(s)], **kw)

    def band_histogram(self, band: int, scenes=None) -> torch.Tensor:
        """int64 [65536]: the pooled histogram of stored band ``band`` over the named scenes (default: all) of a uint16 pool, codes
        equal to the pool's ``nodata`` left out -- one count per scene into one table.  As ``match`` of ``predict`` it
        matches a predicted band to the statistics of a whole set of real ones."""
        from .inference import scene_histogram
        if self.dtype != L.SCENE_U16:
            raise ValueError("ScenePool.band_histogram: the pool must hold uint16 scenes")
        if not 0 <= int(band) < self.C:
            raise ValueError(f"band {band} outside 0 .. {self.C - 1}")
        ids = list(range(len(self.shapes))) if scenes is None else [int(s) for s in scenes]
        hist = torch.zeros(65536, dtype=torch.int64, device=self.device)
        for s in ids:
            scene_histogram(self.scene(s)[int(band)], self.nodata, hist)
        return hist

    def split(self, val, guard=0) -> "PoolSplit":
        """Hold rectangles of the scenes out of training.  ``val``: ``(scene, y0, x0, h, w)`` rectangles in source pixels,
        each inside its scene, pairwise disjoint (ValueError otherwise); an empty list holds nothing out.  ``guard`` >= 0: no training
        window comes closer than ``guard`` pixels to a rectangle.  The ``PoolSplit``'s ``.train`` and ``.val`` share this pool's
        buffers, nothing is copied."""
        return PoolSplit(self, val, guard)

    def split_blocks(self, block, val_fraction, seed, guard=0) -> "PoolSplit":
        """``split`` on a lattice of ``block`` x ``block`` cells.  The candidates are the FULL cells (s, i, j), i < H_s // block, j < W_s
        // block (partial cells at the far edges always train); ``n = max(1, int(val_fraction * cells + 0.5))`` of them are held out:
        those with the smallest ``block_key(seed, s, i, j)``, ties broken by (s, i, j) -- pure Python integers, the same cells on every
        platform.  Adjacent cells of a block row are merged into one rectangle, and runs over the same columns in consecutive block
        rows are stacked."""
        if not _is_integer(block, 1):
            raise ValueError(f"block must be a positive integer, got {block!r}")
        if not 0.0 < float(val_fraction) < 1.0:
            raise ValueError(f"val_fraction must lie strictly between 0 and 1, got {val_fraction!r}")
        return PoolSplit(self, block_rectangles(self.shapes, int(block), float(val_fraction), int(seed)), guard)


_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """one step of SplitMix64 from state ``x``: the standard constants and shifts, Python integers mod 2^64"""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def block_key(seed: int, s: int, i: int, j: int) -> int:
    """the key of cell (i, j) of scene s in ``split_blocks``: splitmix64(splitmix64(splitmix64((seed mod 2^64) ^ s) ^ i) ^ j)"""
    return splitmix64(splitmix64(splitmix64((int(seed) & _M64) ^ s) ^ i) ^ j)


def block_rectangles(shapes, block, val_fraction, seed):
    """the held-out rectangles ``(scene, y0, x0, h, w)`` of ``ScenePool.split_blocks``, sorted by (scene, y0, x0)"""
    cells = [(s, i, j) for s, (h, w) in enumerate(shapes) for i in range(h // block) for j in range(w // block)]
    if not cells:
        raise ValueError(f"no scene holds a full {block} x {block} block")
    n = max(1, int(val_fraction * len(cells) + 0.5))
    held = set(sorted(cells, key=lambda c: (block_key(seed, *c), c))[:n])
    out = []
    for s, (h, w) in enumerate(shapes):
        open_runs = {}                                                           # (j0, j1) -> the block row the stack began at
        for i in range(h // block + 1):                                          # one row past the last closes what is open
            runs, j = [], 0
            while j < w // block:
                if (s, i, j) in held:
                    j0 = j
                    while (s, i, j + 1) in held:
                        j += 1
                    runs.append((j0, j + 1))
                j += 1
            for run in [r for r in open_runs if r not in runs]:
                i0 = open_runs.pop(run)
                out.append((s, i0 * block, run[0] * block, (i - i0) * block, (run[1] - run[0]) * block))
            for run in runs:
                open_runs.setdefault(run, i)
    return sorted(out)


def origin_rectangles(shape, side, held, guard=0):
    """The admissible window origins of ONE scene as disjoint rectangles ``(oy, ox, oh, ow)``: ``[0, H - side] x [0, W - side]`` minus
    the origins whose ``side`` x ``side`` window touches one of the rectangles ``held`` = ``(y0, x0, h, w)`` widened by ``guard``.  A
    sweep over y-slabs: the breakpoints of the forbidden origin rectangles cut the origin rows into slabs, each slab keeps the
    complement of its forbidden x-intervals, and consecutive slabs with the same intervals are merged.  Order: by oy, then ox."""
    H, W = shape
    ny, nx = H - side + 1, W - side + 1
    if ny < 1 or nx < 1:
        return []
    forbidden = []                                                               # half-open origin rectangles (ya, yb, xa, xb)
    for ry, rx, rh, rw in held:
        ya, yb = max(0, ry - guard - side + 1), min(ny, ry + rh + guard)
        xa, xb = max(0, rx - guard - side + 1), min(nx, rx + rw + guard)
        if ya < yb and xa < xb:
            forbidden.append((ya, yb, xa, xb))
    cuts = sorted({0, ny} | {y for f in forbidden for y in f[:2]})
    slabs = []                                                                   # [y start, y end, free x-intervals]
    for ya, yb in zip(cuts, cuts[1:]):
        free, x = [], 0
        for xa, xb in sorted((f[2], f[3]) for f in forbidden if f[0] <= ya < f[1]):
            if xa > x:
                free.append((x, xa))
            x = max(x, xb)
        if x < nx:
            free.append((x, nx))
        if slabs and slabs[-1][1] == ya and slabs[-1][2] == free:
            slabs[-1][1] = yb
        else:
            slabs.append([ya, yb, free])
    return [(ya, xa, yb - ya, xb - xa) for ya, yb, free in slabs for xa, xb in free]


class PoolSplit:
    """A pool with rectangles held out (``ScenePool.split`` / ``split_blocks``).  ``rectangles``: the held-out ``(scene,
    y0, x0, h, w)`` as given; ``guard``; ``train``: the sampler of everything else (``SplitTrain``); ``val``: the grid inside the
    rectangles (``SplitVal``).  Both read the pool's own device buffers."""

    def __init__(self, pool, val, guard=0):
        if not _is_integer(guard, 0):
            raise ValueError(f"guard must be a non-negative integer (source pixels), got {guard!r}")
        rects = []
        for r in val:
            try:
                s, y0, x0, h, w = (int(v) for v in r)
                exact = all(v == int(v) for v in r)
            except (TypeError, ValueError):
                raise ValueError(f"a held-out rectangle is (scene, y0, x0, h, w) in integers, got {r!r}") from None
            if not exact:
                raise ValueError(f"a held-out rectangle is (scene, y0, x0, h, w) in integers, got {r!r}")
            if not 0 <= s < len(pool.shapes):
                raise ValueError(f"rectangle {r!r}: scene {s} outside 0 .. {len(pool.shapes) - 1}")
            H, W = pool.shapes[s]
            if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
                raise ValueError(f"rectangle {r!r} is empty or not inside scene {s} ({H} x {W})")
            for o in rects:
                if o[0] == s and y0 < o[1] + o[3] and o[1] < y0 + h and x0 < o[2] + o[4] and o[2] < x0 + w:
                    raise ValueError(f"rectangles {o!r} and {(s, y0, x0, h, w)!r} overlap")
            rects.append((s, y0, x0, h, w))
        self.pool, self.rectangles, self.guard = pool, rects, int(guard)
        self.train, self.val = SplitTrain(self), SplitVal(self)

    def overlap(self, windows, tile, guard=0) -> np.ndarray:
        """The audit, on the host: int64 [n], for each row ``(scene, y0, x0, word)`` of ``windows`` (a ``WindowList``, tensor or array
        [n, 4]) the number of pixels of its ``f * tile`` window that lie inside a held-out rectangle, each widened by ``guard`` pixels
        on every side -- 0 for every row ``train`` draws (also with this split's own guard), ``(f * tile)^2`` for every row of
        ``val.grid``."""
        rows = windows.host if isinstance(windows, WindowList) else windows
        rows = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows).astype(np.int64).reshape(-1, 4)
        side = (((rows[:, 3] >> 16) & 7) + 1) * int(tile)
        guard = int(guard)
        out = np.zeros(len(rows), dtype=np.int64)
        for s, y0, x0, h, w in self.rectangles:
            dy = np.minimum(rows[:, 1] + side, y0 + h + guard) - np.maximum(rows[:, 1], y0 - guard)
            dx = np.minimum(rows[:, 2] + side, x0 + w + guard) - np.maximum(rows[:, 2], x0 - guard)
            out += np.where(rows[:, 0] == s, np.clip(dy, 0, None) * np.clip(dx, 0, None), 0)
        return out


class SplitTrain(_Sampler):
    """The training half of a ``PoolSplit``: ``sample`` / ``loader`` with ``ScenePool``'s signatures, through
    ``nirgan_scene_sample_origins``.  The draw runs over a table of rectangles of admissible window origins, built on the host by
    ``origin_rectangles`` once per ``(tile, factors)``: it is exactly uniform over the admissible windows and cannot name a window
    that touches a held-out rectangle widened by the guard."""

    def __init__(self, split):
        self.split, self.pool, self.device = split, split.pool, split.pool.device
        self._origins = {}                                                       # (tile, factors) -> (device rows, host rows, first, count)

    def _outputs(self, B, tile):
        return self.pool._outputs(B, tile)

    def _table(self, tile, factors):
        key = (int(tile), tuple(factors))
        if key not in self._origins:
            rows, first, count = [], [], []
            held = {s: [r[1:] for r in self.split.rectangles if r[0] == s] for s in range(len(self.pool.shapes))}
            for f in key[1]:
                side, cum = _side("scale", f, key[0]), 0
                first.append(len(rows))
                for s, shape in enumerate(self.pool.shapes):
                    for oy, ox, oh, ow in origin_rectangles(shape, side, held[s], self.split.guard):
                        cum += oh * ow
                        rows.append((s, oy, ox, oh, ow, cum))
                count.append(len(rows) - first[-1])
                if not count[-1]:
                    raise ValueError(f"scale {f}: no {side} x {side} window of the pool lies outside the held-out rectangles (guard {self.split.guard})")
            host = np.asarray(rows, dtype=np.int64).reshape(-1, L.SCENE_ORIGIN_COLS)
            self._origins[key] = (torch.from_numpy(host.copy()).to(self.device), host, tuple(first), tuple(count))
        return self._origins[key]

    def origins(self, tile, factor=1) -> np.ndarray:
        """the host rows ``(scene, oy, ox, oh, ow, cum)`` of the origin table for windows of side ``factor * tile`` (a copy)"""
        return self._table(tile, (int(factor),))[1].copy()

    def windows(self, tile, factor=1) -> int:
        """how many windows of side ``factor * tile`` are admissible"""
        return int(self._table(tile, (int(factor),))[1][-1, 5])

    def _describe(self, out, B, tile, seed, draw, sample0, augment, max_invalid, scales, scale_weights):
        """(name of the entry, its descriptor) of one checked ``sample`` call writing into ``out``: ``ScenePool.sample`` on the
        admissible windows.  After 8 rejected nodata attempts the last window is returned with bit 31 set, as there -- it is an
        admissible window all the same."""
        if scales is None and scale_weights is not None:
            raise ValueError("scale_weights without scales")
        factors, weights = check_scales(scales, scale_weights) if scales is not None else ((1,), (1,))
        origins, origins_host, first, count = self._table(tile, factors)
        d = L.SceneOriginsDesc()
        _fill(d, self.pool, self.pool._table(tile), out, tile, (B, augment, seed, draw, sample0, max_invalid))   # columns 0, 1, 2, 4 are read
        _fill_scales(d, factors, weights)
        d.origins, d.origins_host, d.R = origins.data_ptr(), origins_host.ctypes.data, len(origins_host)
        d.first, d.count = (C.c_int * 8)(*first), (C.c_int * 8)(*count)
        return "nirgan_scene_sample_origins", d


class SplitVal:
    """The validation half of a ``PoolSplit``: ``grid`` lists the windows lying FULLY inside one held-out rectangle, ``gather`` and
    ``grid_loader`` cut them from the pool's buffers (``nirgan_scene_gather``, ``GridLoader``)."""

    def __init__(self, split):
        self.split, self.pool, self.device = split, split.pool, split.pool.device

    def grid(self, tile, *, factors=(1,), stride=None, max_invalid=0, cover=True) -> "WindowList":
        """``ScenePool.grid`` with every held-out rectangle in the place of a scene: a rectangle of h x w pixels at (y0, x0) with h >= L
        and w >= L gives the rows y0 + 0, stride, 2 * stride, ... <= y0 + h - L (with ``cover`` also y0 + h - L) and the columns by the
        same rule.  Order: factor, then rectangle as given to ``split``, then row, then column.  The nodata filter is the grid's own.
        ValueError if no window is left."""
        return _grid(self.pool, lambda: self.split.rectangles, tile, factors, stride, max_invalid, cover, "lies inside a held-out rectangle")

    def gather(self, windows, tile, *, first=0, count=None, out=None, return_valid=False):
        """``ScenePool.gather``: the rows are cut as they are named, whichever half they came from"""
        return self.pool.gather(windows, tile, first=first, count=count, out=out, return_valid=return_valid)

    def grid_loader(self, batch_size, tile, *, factors=(1,), stride=None, max_invalid=0, cover=True, rank=0, world=1, return_valid=False):
        """``GridLoader`` over ``grid(tile, ...)``; rank ``rank`` of ``world`` takes the rows i with ``i % world == rank``, in order"""
        return _grid_loader(self.pool, self.grid, batch_size, tile, rank, world, return_valid, factors=factors, stride=stride,
                            max_invalid=max_invalid, cover=cover)


def _grid_starts(extent, side, step, cover):
    """0, step, 2 * step, ... <= extent - side, and with ``cover`` extent - side itself if it is not the last"""
    last = extent - side
    starts = list(range(0, last + 1, step))
    if cover and starts[-1] != last:
        starts.append(last)
    return np.asarray(starts, dtype=np.int64)


class WindowList:
    """An int32 [n, 4] list of window rows (scene, y0, x0, word) on the device (``.device``, a tensor) with its copy on the host
    (``.host``, a numpy array): ``nirgan_scene_gather`` checks every row on the host copy and cuts from the device copy.  Built from a
    host array it uploads (no synchronisation); built from a device tensor it copies to the host ONCE, here.  Both copies are the
    list's own and are not to be written afterwards."""

    def __init__(self, windows, device):
        device = torch.device(device)
        if torch.is_tensor(windows):
            if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 4:
                raise ValueError(f"windows must be int32 [n, 4], got {windows.dtype} {tuple(windows.shape)}")
            self.host = np.ascontiguousarray(windows.detach().cpu().numpy()).copy()
            self.device = windows.detach().to(device).contiguous().clone()
        else:
            a = np.asarray(windows)
            if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != 4:
                raise ValueError(f"windows must be int32 [n, 4], got {a.dtype} {a.shape}")
            self.host = np.ascontiguousarray(a).copy()
            self.device = torch.from_numpy(self.host.copy()).to(device)

    def __len__(self):
        return int(self.host.shape[0])


class GridLoader:
    """A re-iterable over a fixed ``WindowList``: ``ceil(rows / batch_size)`` batches ``{"rgb", "nir"[, "coords"]}`` of
    ``pool.gather``, the last one possibly smaller, and EVERY ``iter()`` yields bitwise the same batches -- there is no epoch and no
    ``set_epoch``, so ``fit`` may walk it as often as it likes and epoch 3 is scored on the windows of epoch 30.  The batches are views
    of one set of tensors made at the first ``iter()``: a batch is valid until the next one is drawn.  A consumer that keeps batches
    across draws has to clone them; ``evaluate_tiles`` regroups what it is given into its own ``batch_size`` and holds a batch smaller
    than that back, so give it a ``batch_size`` no larger than the loader's.  ``windows``: this rank's rows; ``factor_of_row``:
    their resolution factors (numpy).  It has no ``__getitem__``: it is an iterable of batches, not a dataset of samples."""

    def __init__(self, pool, windows, batch_size, tile, return_valid=False):
        if int(batch_size) <= 0 or int(tile) <= 0:
            raise ValueError("batch_size and tile must be positive")
        if not len(windows):
            raise ValueError("a GridLoader needs at least one window (this rank's share of the grid is empty)")
        self.pool, self.windows, self.batch_size, self.tile = pool, windows, int(batch_size), int(tile)
        self.factor_of_row = ScenePool.window_factor(windows.host)
        self.return_valid = bool(return_valid)                                  # the batches carry "valid" (``ScenePool.gather``)
        self._buffers = None

    def __len__(self):
        return -(-len(self.windows) // self.batch_size)

    def __iter__(self):
        if self._buffers is None:
            self._buffers = {k: v for k, v in self.pool._outputs(self.batch_size, self.tile).items() if k != "window"}
            if self.return_valid:
                _valid_out(self.pool, self._buffers, self.batch_size, self.tile)
        for first in range(0, len(self.windows), self.batch_size):
            n = min(self.batch_size, len(self.windows) - first)
            yield self.pool.gather(self.windows, self.tile, first=first, count=n, out={k: v[:n] for k, v in self._buffers.items()},
                                   return_valid=self.return_valid)

    def by_factor(self):
        """``(f, GridLoader)`` for every factor of the list in ascending order, each over the rows of that factor alone"""
        for f in sorted(set(self.factor_of_row.tolist())):
            yield f, GridLoader(self.pool, WindowList(self.windows.host[self.factor_of_row == f], self.windows.device.device),
                                self.batch_size, self.tile, return_valid=self.return_valid)


def check_scales(scales, scale_weights=None):
    """``scales`` / ``scale_weights`` as the entry wants them: (factors rising, their weights); ValueError for what it would refuse"""
    try:
        pairs = list(zip(scales, scale_weights if scale_weights is not None else [1] * len(scales), strict=True))
    except (TypeError, ValueError):
        raise ValueError("scales must be a sequence of integers and scale_weights, if given, as long as scales") from None
    if not 1 <= len(pairs) <= L.SCENE_MAX_SCALES:
        raise ValueError(f"scales must name 1 .. {L.SCENE_MAX_SCALES} factors, got {len(pairs)}")
    for f, w in pairs:
        if not _is_integer(f, 1) or int(f) > L.SCENE_MAX_FACTOR:
            raise ValueError(f"scale {f!r} is not an integer in 1 .. {L.SCENE_MAX_FACTOR}")
        if not _is_integer(w, 1):
            raise ValueError(f"scale {f}: the weight {w!r} is not a positive integer")
    pairs = sorted((int(f), int(w)) for f, w in pairs)
    factors, weights = tuple(f for f, _ in pairs), tuple(w for _, w in pairs)
    for a, b in zip(factors, factors[1:]):
        if a == b:
            raise ValueError(f"scale {a} is named twice")
    if sum(weights) >= 2 ** 32:
        raise ValueError(f"scales {factors}: the weights sum to 2^32 or more")
    return factors, weights


class SceneLoader:
    """A re-iterable of ``steps_per_epoch`` batches per epoch.  Step i of epoch e is ``pool.sample(..., draw=e * steps_per_epoch + i,
    sample0=rank * batch_size, scales=..., scale_weights=...)``.  ``set_epoch(e)`` names the epoch of the next ``iter()`` (``fit`` calls it, so a resumed run
    continues where the checkpoint stopped); without it every ``iter()`` moves on by one epoch.  The batches of one loader share their
    tensors: a batch is valid until the next one is drawn, nothing is allocated per step.  With ``return_valid`` every batch also carries
    the mask ``"valid"`` of ``sample`` -- one more tensor of the loader's own, one more launch per batch."""

    def __init__(self, pool, batch_size, tile, steps_per_epoch, *, seed, augment="d4", max_invalid=0, rank=0, world=1, scales=None,
                 scale_weights=None, return_valid=False):
        if not 0 <= int(rank) < int(world):
            raise ValueError(f"rank {rank} outside 0 .. world-1 = {int(world) - 1}")
        if int(steps_per_epoch) <= 0:
            raise ValueError("steps_per_epoch must be positive")
        if augment not in L.SCENE_VIEWS:
            raise ValueError(f"augment must be one of {sorted(L.SCENE_VIEWS)}, got {augment!r}")
        self.pool, self.batch_size, self.tile, self.steps_per_epoch = pool, int(batch_size), int(tile), int(steps_per_epoch)
        self.seed, self.augment, self.max_invalid, self.rank, self.world = seed, augment, int(max_invalid), int(rank), int(world)
        if scales is None and scale_weights is not None:
            raise ValueError("scale_weights without scales")
        self.scales, self.scale_weights = (None, None) if scales is None else check_scales(scales, scale_weights)
        self.return_valid = bool(return_valid)                                  # the batches carry "valid" (``sample``)
        self.epoch = 0
        self._buffers = None                                                     # one set of output tensors, made at the first iter()

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        if self._buffers is None:
            self._buffers = self.pool._outputs(self.batch_size, self.tile)
        for i in range(self.steps_per_epoch):
            yield self.pool.sample(self.batch_size, self.tile, seed=self.seed, draw=epoch * self.steps_per_epoch + i,
                                   sample0=self.rank * self.batch_size, augment=self.augment, max_invalid=self.max_invalid,
                                   out=self._buffers, scales=self.scales, scale_weights=self.scale_weights,
                                   return_valid=self.return_valid)
