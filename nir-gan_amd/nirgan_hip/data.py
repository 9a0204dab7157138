"""Training batches from device-resident scenes: the sampler of csrc/scenepool.hip seen from Python.

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


class ScenePool:
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

    def sample(self, batch_size, tile, *, seed, draw, sample0=0, augment="d4", max_invalid=0, return_windows=False, out=None,
               scales=None, scale_weights=None):
        """One batch ``{"rgb" [B,3,T,T], "nir" [B,1,T,T][, "coords" [B,2]]}``, plus ``"window"`` [B,4] int32 = (scene, y0, x0,
        view | attempt << 8 | (factor - 1) << 16 | exhausted << 31) with ``return_windows``.  Sample b is a function of ``(seed, draw,
        sample0 + b)`` alone.  ``augment``: "d4" (8 views), "flips" (4) or "none".  ``max_invalid``: the most invalid pixels a window
        may hold (only with ``nodata``); after 8 rejected attempts the last window is returned and bit 31 of its window word is set.
        ``out``: the tensors to write into (the dict of an earlier call with ``return_windows`` and the same shapes) instead of new ones.
        ``scales``: distinct resolution factors in 1 .. 8 (sorted before use), one drawn per sample with the positive integer
        ``scale_weights`` (default: all 1); the sample is then an f*T window of the source (y0, x0 in source pixels, ``max_invalid``
        per f x f block, coords of the window's centre) delivered as the T x T tile of its f x f block means.  None: factor 1
        through ``nirgan_scene_sample``, as ever."""
        if augment not in L.SCENE_VIEWS:
            raise ValueError(f"augment must be one of {sorted(L.SCENE_VIEWS)}, got {augment!r}")
        B, tile = int(batch_size), int(tile)
        if B <= 0 or tile <= 0:
            raise ValueError("batch_size and tile must be positive")
        out = out if out is not None else self._outputs(B, tile)
        entry, d = self._describe(out, B, tile, seed, draw, sample0, augment, max_invalid, scales, scale_weights)
        L.call(entry, C.byref(d), _stream(self.device))
        return out if return_windows else {k: v for k, v in out.items() if k != "window"}

    def _describe(self, out, B, tile, seed, draw, sample0, augment, max_invalid, scales, scale_weights):
        """(name of the entry, its descriptor) of one checked ``sample`` call writing into ``out``"""
        if scales is None:
            if scale_weights is not None:
                raise ValueError("scale_weights without scales")
            d = L.SceneSampleDesc()
            table, table_host = self._table(tile)
            if int(table_host[-1, 3]) == 0:
                raise ValueError(f"no scene of the pool holds a {tile} x {tile} window")
            entry = "nirgan_scene_sample"
        else:
            d = L.SceneScaledDesc()
            factors, weights = check_scales(scales, scale_weights)
            for f in factors:
                if (f * tile) ** 2 >= 2 ** 31:
                    raise ValueError(f"scale {f}: the window ({f} * {tile})^2 has 2^31 pixels or more")
            table, table_host = self._scaled_tables(tile, factors)
            for f, t in zip(factors, table_host):
                if int(t[-1, 3]) == 0:
                    raise ValueError(f"scale {f}: no scene of the pool holds a {f * tile} x {f * tile} window")
            d.K = len(factors)
            d.factor, d.weight = (C.c_int * 8)(*factors), (C.c_uint32 * 8)(*weights)
            entry = "nirgan_scene_sample_scaled"
        d.pool, d.pool_elems, d.dtype, d.S, d.C = self.pool.data_ptr(), self.pool_elems, self.dtype, len(self.shapes), self.C
        d.table, d.table_host = table.data_ptr(), table_host.ctypes.data
        d.prefix, d.prefix_elems = (self.prefix.data_ptr() if self.prefix is not None else None), self.prefix_elems
        d.geo = self.geo.data_ptr() if self.geo is not None else None
        d.band = (C.c_int * 4)(*self.bands)
        d.tile, d.B, d.views, d.divisor = tile, B, L.SCENE_VIEWS[augment], self.divisor
        d.seed_lo, d.seed_hi = split_seed(seed)
        d.draw, d.sample0, d.max_invalid = int(draw) & ((1 << 64) - 1), int(sample0) & 0xFFFFFFFF, int(max_invalid)
        d.rgb, d.nir, d.window = out["rgb"].data_ptr(), out["nir"].data_ptr(), out["window"].data_ptr()
        d.coords = out["coords"].data_ptr() if self.geo is not None else None
        return entry, d

    def loader(self, batch_size, tile, steps_per_epoch, *, seed, augment="d4", max_invalid=0, rank=0, world=1, scales=None,
               scale_weights=None):
        return SceneLoader(self, batch_size, tile, steps_per_epoch, seed=seed, augment=augment, max_invalid=max_invalid, rank=rank,
                           world=world, scales=scales, scale_weights=scale_weights)


def check_scales(scales, scale_weights=None):
    """``scales`` / ``scale_weights`` as the entry wants them: (factors rising, their weights); ValueError for what it would refuse"""
    try:
        pairs = list(zip(scales, scale_weights if scale_weights is not None else [1] * len(scales), strict=True))
    except (TypeError, ValueError):
        raise ValueError("scales must be a sequence of integers and scale_weights, if given, as long as scales") from None
    if not 1 <= len(pairs) <= L.SCENE_MAX_SCALES:
        raise ValueError(f"scales must name 1 .. {L.SCENE_MAX_SCALES} factors, got {len(pairs)}")
    for f, w in pairs:
        if isinstance(f, bool) or f != int(f) or not 1 <= int(f) <= L.SCENE_MAX_FACTOR:
            raise ValueError(f"scale {f!r} is not an integer in 1 .. {L.SCENE_MAX_FACTOR}")
        if isinstance(w, bool) or w != int(w) or int(w) <= 0:
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
    tensors: a batch is valid until the next one is drawn, nothing is allocated per step."""

    def __init__(self, pool, batch_size, tile, steps_per_epoch, *, seed, augment="d4", max_invalid=0, rank=0, world=1, scales=None,
                 scale_weights=None):
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
                                   out=self._buffers, scales=self.scales, scale_weights=self.scale_weights)
