"""The Winograd data, plane-GEMM and output stages without a GPU: the bodies of tests/wino_stage_cases.py on the numpy emulator
(tests/emu_backend.py), and the checks that keep their expectations honest -- the case tables' own conditions (every route named, every
shape reason present), eager fp32 torch of every bounded formula inside its bound and of every integer-pass formula bitwise on the float64
reference, a census of the engines' nirgan_wino6_* ops whose features the raw cases must all produce, and emulators with one planted,
subtle error each that must fail a named body.  Bodies shared with tests/test_gpu_wino_stages.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import conv_replay as R
import wino_stage_cases as S
from emu_backend import EmuBackend, arr, obj
from emu_pixel_disc import EmuPixelDisc
from nirgan_hip import lib as L
from nirgan_hip.options import OPT
from weight_path_cases import w6_geo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(ROOT, "scripts", "plan_signature.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

ident = lambda c: "-".join(map(str, c)).replace(" ", "")


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)
    OPT.reset()


# ------------------------------------------------------------------------------------------------ bodies on the emulator
def test_the_case_tables_name_every_route_and_shape_reason():
    S.in_table_conditions_hold()
    S.gemm_table_conditions_hold()
    S.out_table_conditions_hold()
    S.fuse_table_conditions_hold()
    assert {c.kernel for c in S.PAIR_CASES} == {"wino6_pair_kernel", "wino6_pair16_kernel", "wino6_pair16p_kernel", ""}
    assert {c.kind for c in S.DYNORM_CASES} == {"fold", "skip", "pre"} and all(c.shape[3] % 32 == 0 for c in S.DYNORM_CASES)


def test_the_library_routes_every_transform_case_to_the_kernel_its_table_names():
    """the compiled library's own routing, asked without a launch (the query reads r, C / K, algo and fuse_gz alone, so it needs no GPU);
    the bodies ask again on the device with the descriptor they launch"""
    name = L.backend().nirgan_wino6_transform_kernel_name

    def named(v, ch, algo, stage, fused=False):
        d = L.Wino6Desc()
        d.r, d.C, d.K, d.algo, d.fuse_gz = v, ch, ch, algo, (16 if fused else None)
        return name(C.byref(d), stage).decode()

    for c in S.IN_CASES:
        if c.entry != "dy":
            assert named(c.v, c.C, c.algo, S.IN_STAGE[c.entry]) == c.kernel, c
    for c in S.DYNORM_CASES:
        assert named(6, c.shape[3], 0, L.W6_STAGE_INPUT_DY_NORM) == S.DYNORM_KERNEL, c
    for c in S.OUT_CASES:
        assert named(c.v, c.K, 0, L.W6_STAGE_OUTPUT) == c.kernel, c
    for c in S.FUSE_CASES:
        assert named(6, c.K, c.algo, L.W6_STAGE_OUTPUT, fused=True) == c.kernel, c


@pytest.mark.parametrize("case", S.IN_CASES, ids=ident)
def test_input_transform(emu, case):
    S.input_against_float64("cpu", case)
    assert emu.calls.count({"input": "wino6_in", "input_norm": "wino6_in_norm", "input_dy": "wino6_in", "dy": "wino6_dy"}[case.entry]) == 4


@pytest.mark.parametrize("case", S.DYNORM_CASES, ids=ident)
def test_input_transform_of_the_instance_norm_backward(emu, case):
    S.dynorm_against_float64("cpu", case)
    assert emu.calls.count("wino6_dy_norm") == 2


@pytest.mark.parametrize("case", S.GEMM_CASES, ids=ident)
def test_plane_gemm(emu, case):
    S.gemm_against_float64("cpu", case)


@pytest.mark.parametrize("case", S.PAIR_CASES, ids=ident)
def test_plane_gemm_with_the_weight_gradient(emu, case):
    S.pair_against_float64("cpu", case)


@pytest.mark.parametrize("case", S.OUT_CASES, ids=ident)
def test_output_transform(emu, case):
    S.output_against_float64("cpu", case)


@pytest.mark.parametrize("case", S.FUSE_CASES, ids=ident)
def test_fused_output_transform(emu, case):
    S.fused_output_against_float64("cpu", case)
    assert "wino6_out_inbwd" in emu.calls


def test_input_guards(emu):
    S.input_guards("cpu")


def test_gemm_guards(emu):
    S.gemm_guards("cpu")


def test_output_guards(emu):
    S.output_guards("cpu")


# ------------------------------------------------------------------------------------------------ the reference alone
def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def eager_two_stage(Mx, P32):
    """the two 1-D stages as two fp32 einsums with fp32 matrices: [p p][T][c]"""
    m = f32(Mx)
    t = torch.einsum("ai,btsijc->btsajc", m, P32)
    return torch.einsum("lj,btsajc->albtsc", m, t).reshape(Mx.shape[0] ** 2, -1, P32.shape[-1]).numpy()


@pytest.mark.parametrize("case", S.IN_CASES, ids=ident)
def test_eager_fp32_input_transforms_lie_inside_the_bound(case):
    c = case
    r, mo, n = w6_geo(c.v)
    for integer in (True, False):
        o = S.in_data(c, integer)
        H, W = o["H"], o["W"]
        what = f"{tuple(c)} {'integer' if integer else 'random'}"
        if c.entry == "input_norm":
            z = (o["y"] - o["mean"][:, None, None]) * o["rstd"][:, None, None]
            assert z.dtype == np.float32
            neg = np.float32(1.0 if c.opt == S.NONE else 0.0 if c.opt == S.RELU else o["slope"])
            a = np.where(z > 0, z, z * neg)
            x = a[:, S.reflect_idx(H)][:, :, S.reflect_idx(W)]
        elif c.entry != "dy":
            x = o["x"]
        if c.entry != "dy":
            P32 = f32(S.patches(x.astype(np.float64), c.v, *S.tiles_of(H, W, c.v)))
            S.held("eager wino6_input V", what, eager_two_stage(S.mats(c.v)[0], P32), o["V"], o["bV"], integer)
        if c.entry in ("input_dy", "dy"):
            p = r - 1 if c.entry == "input_dy" else c.opt
            dy = (o["x"] if c.entry == "input_dy" else o["dy"])[:, p:p + c.hw[0], p:p + c.hw[1]]
            S.held("eager wino6_dy Yt", what, eager_two_stage(S.mats(c.v)[2], f32(S.dy_blocks(dy.astype(np.float64), c.v))), o["Yt"], o["bYt"], integer)


def eager_R(M, B, H, W, v):
    r, mo, n = w6_geo(v)
    TH, TW = S.tiles_of(H, W, v)
    at = f32(S.mats(v)[1])
    t = torch.einsum("pa,albtsk->plbtsk", at, f32(M).reshape(n, n, B, TH, TW, -1))
    return torch.einsum("ql,plbtsk->btpsqk", at, t).reshape(B, mo * TH, mo * TW, -1).numpy()


@pytest.mark.parametrize("case", S.OUT_CASES, ids=ident)
def test_eager_fp32_output_transform_lies_inside_the_bound(case):
    c = case
    mo = w6_geo(c.v)[1]
    H, W = c.hw
    for integer in (True, False):
        o = S.out_data(c, integer)
        Rr = eager_R(o["M"], c.B, H, W, c.v)
        y = Rr[:, :H, :W] + (o["bias"] if c.bias else np.float32(0))
        rec = None
        if c.stats:
            valid = np.zeros((Rr.shape[1], Rr.shape[2], 1), dtype=np.float32)
            valid[:H, :W] = 1
            k = Rr[:, ::mo, ::mo]
            dl = (S.tile_view(Rr, mo) - k[:, :, :, None, :]) * S.tile_view(np.broadcast_to(valid, Rr.shape[:3] + (1,)), mo)
            cnt = np.broadcast_to(S.tile_view(np.broadcast_to(valid, Rr.shape[:3] + (1,)), mo).sum(3), k.shape)
            rec = np.stack([k, f32(dl).sum(3).numpy(), f32(dl * dl).sum(3).numpy(), cnt], 3).astype(np.float32)
        assert y.dtype == np.float32
        S.output_checks(c, integer, y, rec)


@pytest.mark.parametrize("case", S.FUSE_CASES, ids=ident)
def test_eager_fp32_fused_output_lies_inside_the_bound(case):
    c = case
    H, W = c.hw
    TH, TW = S.tiles_of(H, W, 6)
    for integer in (True, False):
        o = S.fuse_data(c, integer)
        ga = S.fold(eager_R(o["M"], c.B, H, W, 6), H, W)
        if c.g2:
            ga = ga + o["g2"]
        z = (o["y"] - o["mean"][:, None, None]) * o["rstd"][:, None, None]
        neg = np.float32(1.0 if c.act == S.NONE else 0.0 if c.act == S.RELU else o["slope"])
        gz = np.where(z > 0, ga, ga * neg)
        assert ga.dtype == np.float32 and z.dtype == np.float32 and gz.dtype == np.float32
        grid = np.zeros((2, c.B, 6 * TH, 6 * TW, c.K), dtype=np.float32)
        grid[0, :, 1:H - 1, 1:W - 1], grid[1, :, 1:H - 1, 1:W - 1] = gz, gz * z
        part = np.stack([f32(S.tile_view(grid[i], 6)).sum(3).numpy() for i in (0, 1)], 3)
        S.fused_checks(c, integer, ga, part)


@pytest.mark.parametrize("case", [g for g in S.GEMM_CASES if not g.x3], ids=ident)
def test_eager_fp32_plane_gemm_lies_inside_the_bound(case):
    g = case
    n = w6_geo(g.v)[2]
    for integer in (True, False):
        seed = 11 * S.GEMM_CASES.index(g) + integer
        V, Uh = S.draw((n * n, g.T, g.C), integer, seed), S.draw((n * n, g.K, g.C), integer, seed + 3)
        got = torch.bmm(f32(V), f32(Uh).transpose(1, 2)).numpy()
        ref = V.astype(np.float64) @ Uh.astype(np.float64).transpose(0, 2, 1)
        A = np.abs(V).astype(np.float64) @ np.abs(Uh).astype(np.float64).transpose(0, 2, 1)
        S.held("eager wino6_gemm", f"{tuple(g)}", got, ref, (g.C + 8) * S.U * A, integer)


@pytest.mark.parametrize("v", S.VARIANTS)
def test_the_integer_pass_is_exact_at_the_stated_magnitudes(v):
    """the worst case over inputs of magnitude 2, in float64: |V| <= 5000; |y|, |Yt| 2^(2 GRAN) < 2^23.2; the fused mode's g_a with both
    folds and fuse_g2 < 2^23.9 (the data drawn is held to 2^24 element by element: exact_or_die)"""
    BT, AT, A = S.mats(v)
    rows = lambda m: np.abs(m).sum(1)
    g2 = 4.0 ** S.GRAN[v]
    assert 2 * rows(BT).max() ** 2 <= 5000
    assert 2 * rows(AT).max() ** 2 * g2 < 2 ** 23.2 and 2 * rows(A).max() ** 2 * g2 < 2 ** 23.2
    if v == 6:
        pair = max(rows(AT)[a] + rows(AT)[a + 2] for a in range(4))            # a halo line and its fold partner share a tile, two lines apart
        assert (2 * pair ** 2 + 2) * g2 < 2 ** 23.9


# ------------------------------------------------------------------------------------------------ census of the engines' ops
ENTRY = {"input": "nirgan_wino6_input", "input_norm": "nirgan_wino6_input_norm", "input_dy": "nirgan_wino6_input_dy", "dy": "nirgan_wino6_dy"}
TRANSFORM_ALGOS = (L.W6_PATCH_PER_THREAD, L.W6_PATCH_PER_LANES)


def _axes(head, H, W, v):
    """a feature per dimension: the extent modulo the tile size"""
    mo = w6_geo(v)[1]
    return {head + ("H", H % mo), head + ("W", W % mo)}


def op_features(op, args) -> set:
    """the feature tuples of one emitted op.  Fields a launch does not read are left out of its tuple: the transforms ignore U3 and the
    plane-GEMM values of `algo`, the plane GEMMs ignore the extent (it only sets T), the bias and the fused-mode fields."""
    d = obj(args[0])
    v = 3 if d.r == 0 else d.r
    if op == "nirgan_wino6_dy":
        return _axes((op, v, d.K % 32 == 0, 0, None), d.H, d.W, v)
    algo = d.algo if d.algo in TRANSFORM_ALGOS else 0
    if op in ("nirgan_wino6_input", "nirgan_wino6_input_dy", "nirgan_wino6_input_dy_norm", "nirgan_wino6_input_norm"):
        return _axes((op, v, d.C % 32 == 0, algo, args[4] if op == "nirgan_wino6_input_norm" else None), d.H, d.W, v)
    if op in ("nirgan_wino6_gemm", "nirgan_wino6_gemm_wgrad_pair"):
        return {(op, v, d.C % 32 == 0, bool(d.U3), bool(d.U), d.algo)}
    assert op == "nirgan_wino6_output", op
    return _axes((op, v, d.K % 32 == 0, bool(d.bias), bool(d.stats_ws), bool(d.fuse_gz), bool(d.fuse_g2), d.fuse_act if d.fuse_gz else 0, algo), d.H, d.W, v)


def case_features() -> set:
    """the same tuples of the raw cases of tests/wino_stage_cases.py"""
    out = set()
    for c in S.IN_CASES:
        H, W = S.in_extent(c)
        out |= _axes((ENTRY[c.entry], c.v, c.C % 32 == 0, c.algo if c.algo in TRANSFORM_ALGOS else 0, c.opt if c.entry == "input_norm" else None), H, W, c.v)
    for c in S.DYNORM_CASES:
        out |= _axes(("nirgan_wino6_input_dy_norm", 6, True, 0, None), c.shape[1] + 2, c.shape[2] + 2, 6)
    for g in S.GEMM_CASES:
        out.add(("nirgan_wino6_gemm", g.v, g.C % 32 == 0, bool(g.x3), g.x3 != 2, g.algo))
    for c in S.PAIR_CASES:
        out.add(("nirgan_wino6_gemm_wgrad_pair", c.v, c.cout % 32 == 0, False, True, 0))
    for c in S.OUT_CASES:
        out |= _axes(("nirgan_wino6_output", c.v, c.K % 32 == 0, c.bias, c.stats, False, False, 0, 0), *c.hw, c.v)
    for c in S.FUSE_CASES:
        out |= _axes(("nirgan_wino6_output", 6, c.K % 32 == 0, False, False, True, c.g2, c.act, c.algo if c.algo in TRANSFORM_ALGOS else 0), *c.hw, 6)
    return out


def census() -> dict:
    """{feature: a configuration that emits it} over every configuration of scripts/plan_signature.py: the engines built on the CPU under
    the emulator, plans built, nothing launched"""
    seen = {}
    L.set_backend(EmuPixelDisc())
    zeros = torch.zeros
    try:
        for name, cfg in P.CONFIGS.items():
            torch.zeros = lambda *a, **kw: torch.empty(*a, **kw)       # building a plan reads no buffer (scripts/plan_signature.py)
            try:
                engines, keep = R.build_engines(P, cfg)
                for eng in engines.values():
                    for pname in P.PLAN_NAMES:
                        for op, args in getattr(getattr(eng, pname, None), "ops", ()):
                            if isinstance(op, str) and op.startswith("nirgan_wino6_") and "weights" not in op and "finish" not in op:
                                for f in op_features(op, args):
                                    seen.setdefault(f, name)
                del engines, keep
            finally:
                torch.zeros = zeros
                OPT.reset()
    finally:
        L.set_backend(None)
    return seen


def test_every_feature_the_engines_emit_has_a_raw_case():
    seen = census()
    entries = {f[0] for f in seen}
    assert entries == {"nirgan_wino6_input", "nirgan_wino6_input_norm", "nirgan_wino6_input_dy", "nirgan_wino6_input_dy_norm", "nirgan_wino6_gemm",
                       "nirgan_wino6_gemm_wgrad_pair", "nirgan_wino6_output"}, entries
    missing = {f: cfg for f, cfg in seen.items() if f not in case_features()}
    assert not missing, "emitted by the engines, produced by no raw case:\n" + "\n".join(f"  {f}  ({cfg})" for f, cfg in sorted(missing.items(), key=str))


# ------------------------------------------------------------------------------------------------ planted errors
def _copy(d):
    c = type(d)()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(d))
    return c


class OneBTCoefficientOff(EmuBackend):
    """F(6x6,3x3): B^T[1][3] = 16 instead of 17 -- the planes of row 1 and of column 1 differ in the fourth digit"""
    _W6 = dict(EmuBackend._W6)
    _bt = EmuBackend._W6[6][1].copy()
    _bt[1, 3] = 16
    _W6[6] = (EmuBackend._W6[6][0], _bt, EmuBackend._W6[6][2])


class LastTileColumnStartsOnePixelLate(EmuBackend):
    def _wino6_V(self, x, B, H, W, Cc, v=3):
        V = super()._wino6_V(x, B, H, W, Cc, v)
        late = np.zeros_like(x)
        late[:, :, :-1] = x[:, :, 1:]
        V[:, :, :, :, -1] = super()._wino6_V(late, B, H, W, Cc, v)[:, :, :, :, -1]
        return V


class LinesPastTheBufferRepeatTheLastLine(EmuBackend):
    def _wino6_V(self, x, B, H, W, Cc, v=3):
        r, mo, n = self._geo6(v)
        TH, TW = -(-H // mo), -(-W // mo)
        xe = np.pad(x, ((0, 0), (0, mo * TH - H), (0, mo * TW - W), (0, 0)), mode="edge")
        return super()._wino6_V(xe, B, mo * TH, mo * TW, Cc, v)


class YtAlsoForTheTileColumnBehindTheLast(EmuBackend):
    """tx == yTW passes the test: the store lands on the next tile row's first tile, behind the plane for the last one"""

    def nirgan_wino6_input_dy(self, cref, yref, stream=None):
        rc = super().nirgan_wino6_input_dy(cref, yref)
        c, y = obj(cref), obj(yref)
        if rc == 0:
            v = self._r6(c.r)
            r, mo, n = self._geo6(v)
            yTH, yTW, TW = -(-y.H // mo), -(-y.W // mo), -(-c.W // mo)
            if TW > yTW:
                yT = y.B * yTH * yTW
                Yt = arr(y.Yt, n * n * yT * y.K + y.K)
                for f in range(n * n):
                    for t in range(yTW, yT + 1, yTW):
                        Yt[f * yT * y.K + t * y.K:f * yT * y.K + (t + 1) * y.K] = 1.0
        return rc


class _FusedRedo(EmuBackend):
    """the fused mode's g_a recomputed with another fold"""

    def _fold(self, R, H, W):
        raise NotImplementedError

    def nirgan_wino6_output(self, ref, stream=None):
        rc = super().nirgan_wino6_output(ref)
        d = obj(ref)
        if rc == 0 and d.fuse_gz:
            B, H, W, K = d.B, d.H, d.W, d.K
            TH, TW = -(-H // 6), -(-W // 6)
            M = arr(d.M, 64 * B * TH * TW * K).reshape(8, 8, B, TH, TW, K).astype(np.float64)
            AT = self._W6[6][2]
            Y = np.einsum("pa,albyxk,ql->bypxqk", AT, M, AT).reshape(B, 6 * TH, 6 * TW, K)[:, :H, :W]
            ga = self._fold(Y.copy(), H, W)[:, 1:H - 1, 1:W - 1]
            if d.fuse_g2:
                ga = ga + arr(d.fuse_g2, ga.size).reshape(ga.shape)
            arr(d.fuse_gz, ga.size)[:] = ga.reshape(-1).astype(np.float32)
        return rc


class FarFoldOntoTheLineBefore(_FusedRedo):
    def _fold(self, R, H, W):
        R[:, 2] += R[:, 0]
        R[:, H - 4] += R[:, H - 1]
        R[:, :, 2] += R[:, :, 0]
        R[:, :, W - 3] += R[:, :, W - 1]
        return R


class ColumnFoldFirstCornerCountedOnce(_FusedRedo):
    """columns first, and the row fold adds the halo rows as they were before it: a corner reaches its partner through one fold only"""

    def _fold(self, R, H, W):
        R0 = R.copy()
        R[:, :, 2] += R0[:, :, 0]
        R[:, :, W - 3] += R0[:, :, W - 1]
        R[:, 2] += R0[:, 0]
        R[:, H - 3] += R0[:, H - 1]
        return R


class EdgeTilesCountAWholeTile(EmuBackend):
    def nirgan_wino6_output(self, ref, stream=None):
        rc = super().nirgan_wino6_output(ref)
        d = obj(ref)
        if rc == 0 and d.stats_ws:
            mo = self._geo6(self._r6(d.r))[1]
            T = d.B * -(-d.H // mo) * -(-d.W // mo)
            arr(d.stats_ws, T * 4 * d.K).reshape(T, 4, d.K)[:, 3] = mo * mo
        return rc


class FusedSumsIncludeTheHalo(EmuBackend):
    """sum g_z also over the halo pixels of the padded extent (their unfolded values)"""

    def nirgan_wino6_output(self, ref, stream=None):
        rc = super().nirgan_wino6_output(ref)
        d = obj(ref)
        if rc == 0 and d.fuse_gz:
            B, H, W, K = d.B, d.H, d.W, d.K
            TH, TW = -(-H // 6), -(-W // 6)
            M = arr(d.M, 64 * B * TH * TW * K).reshape(8, 8, B, TH, TW, K).astype(np.float64)
            AT = self._W6[6][2]
            Y = np.einsum("pa,albyxk,ql->bypxqk", AT, M, AT).reshape(B, 6 * TH, 6 * TW, K)
            Y[:, 1:H - 1, 1:W - 1] = 0
            Y[:, H:] = 0
            Y[:, :, W:] = 0
            arr(d.fuse_part, B * TH * TW * 2 * K).reshape(B, TH, TW, 2, K)[:, :, :, 0] += Y.reshape(B, TH, 6, TW, 6, K).sum((2, 4)).astype(np.float32)
        return rc


class OnePlaneReadsItsNeighboursU(EmuBackend):
    def nirgan_wino6_gemm(self, ref, stream=None):
        d = obj(ref)
        if d.U3 or not d.U or d.K <= 64 or self._r6(d.r) not in self._W6:
            return super().nirgan_wino6_gemm(ref)
        npl = self._geo6(self._r6(d.r))[2] ** 2
        Uc = arr(d.U, npl * d.K * d.C).reshape(npl, d.K * d.C).copy()
        Uc[5] = Uc[6]
        d2 = _copy(d)
        d2.U = Uc.ctypes.data
        return super().nirgan_wino6_gemm(d2)


class VScaled(EmuBackend):
    """a relative error of 2^-18 on V"""

    def nirgan_wino6_input(self, ref, stream=None):
        rc = super().nirgan_wino6_input(ref)
        d = obj(ref)
        if rc == 0:
            v = self._r6(d.r)
            n = self._geo6(v)[2] ** 2 * self.nirgan_wino6_tiles_r(d.B, d.H, d.W, v) * d.C
            arr(d.V, n)[:] *= np.float32(1 + 2.0 ** -18)
        return rc


class OneStoreBehindTheLastPlane(EmuBackend):
    def nirgan_wino6_input(self, ref, stream=None):
        rc = super().nirgan_wino6_input(ref)
        d = obj(ref)
        if rc == 0:
            v = self._r6(d.r)
            n = self._geo6(v)[2] ** 2 * self.nirgan_wino6_tiles_r(d.B, d.H, d.W, v) * d.C
            arr(d.V, n + 1)[n] = 1.0
        return rc


class FusedDyPassWritesTheDescribedBuffer(EmuBackend):
    """dY materialised where c->x points (what the emulator did before it was held to the header)"""

    def nirgan_wino6_input_dy_norm(self, cref, yref, nref, stream=None):
        rc = super().nirgan_wino6_input_dy_norm(cref, yref, nref)
        c = obj(cref)
        if rc == 0:
            arr(c.x, 1)[0] = 0.0
        return rc


def _in(entry, v, Cc, hw, algo=0):
    return next(c for c in S.IN_CASES if (c.entry, c.v, c.C, c.hw, c.algo) == (entry, v, Cc, hw, algo))


def _out(v, K, hw):
    return next(c for c in S.OUT_CASES if (c.v, c.K, c.hw) == (v, K, hw) and c.stats)


def _fuse(K, hw):
    return next(c for c in S.FUSE_CASES if (c.K, c.hw) == (K, hw))


MUTANTS = [
    (OneBTCoefficientOff, "input r6 (7, 13)", lambda: S.input_against_float64("cpu", _in("input", 6, 36, (7, 13)))),
    (OneBTCoefficientOff, "input_norm r6 (2, 3)", lambda: S.input_against_float64("cpu", _in("input_norm", 6, 8, (2, 3)))),
    (OneBTCoefficientOff, "input_dy_norm fold", lambda: S.dynorm_against_float64("cpu", S.DYNORM_CASES[0])),
    (LastTileColumnStartsOnePixelLate, "input r6 (7, 13)", lambda: S.input_against_float64("cpu", _in("input", 6, 36, (7, 13)))),
    (LastTileColumnStartsOnePixelLate, "input r3 (5, 9)", lambda: S.input_against_float64("cpu", _in("input", 3, 36, (5, 9)))),
    (LastTileColumnStartsOnePixelLate, "input_dy r4 (11, 7)", lambda: S.input_against_float64("cpu", _in("input_dy", 4, 32, (11, 7)))),
    (LinesPastTheBufferRepeatTheLastLine, "input r6 (7, 13)", lambda: S.input_against_float64("cpu", _in("input", 6, 36, (7, 13)))),
    (LinesPastTheBufferRepeatTheLastLine, "input r4 (5, 9)", lambda: S.input_against_float64("cpu", _in("input", 4, 32, (5, 9)))),
    (LinesPastTheBufferRepeatTheLastLine, "input_norm r6 (17, 11)", lambda: S.input_against_float64("cpu", _in("input_norm", 6, 32, (17, 11)))),
    (YtAlsoForTheTileColumnBehindTheLast, "input_dy r6 (6, 6)", lambda: S.input_against_float64("cpu", _in("input_dy", 6, 32, (6, 6)))),
    (YtAlsoForTheTileColumnBehindTheLast, "input_dy r3 (2, 3)", lambda: S.input_against_float64("cpu", _in("input_dy", 3, 4, (2, 3)))),
    (FarFoldOntoTheLineBefore, "fused (9, 6)", lambda: S.fused_output_against_float64("cpu", _fuse(4, (9, 6)))),
    (FarFoldOntoTheLineBefore, "fused (12, 12)", lambda: S.fused_output_against_float64("cpu", _fuse(32, (12, 12)))),
    (ColumnFoldFirstCornerCountedOnce, "fused (6, 6)", lambda: S.fused_output_against_float64("cpu", _fuse(4, (6, 6)))),
    (ColumnFoldFirstCornerCountedOnce, "fused (11, 15)", lambda: S.fused_output_against_float64("cpu", _fuse(36, (11, 15)))),
    (EdgeTilesCountAWholeTile, "output r6 (7, 13)", lambda: S.output_against_float64("cpu", _out(6, 128, (7, 13)))),
    (EdgeTilesCountAWholeTile, "output r3 (2, 3)", lambda: S.output_against_float64("cpu", _out(3, 4, (2, 3)))),
    (FusedSumsIncludeTheHalo, "fused (6, 9)", lambda: S.fused_output_against_float64("cpu", _fuse(36, (6, 9)))),
    (FusedSumsIncludeTheHalo, "fused (10, 11)", lambda: S.fused_output_against_float64("cpu", _fuse(96, (10, 11)))),
    (OnePlaneReadsItsNeighboursU, "gemm C 4", lambda: S.gemm_against_float64("cpu", S.GEMM_CASES[0])),
    (OnePlaneReadsItsNeighboursU, "gemm32p", lambda: S.gemm_against_float64("cpu", S.GEMM_CASES[10])),
    (OnePlaneReadsItsNeighboursU, "pair", lambda: S.pair_against_float64("cpu", S.PAIR_CASES[1])),
    (VScaled, "input r3 (2, 3)", lambda: S.input_against_float64("cpu", _in("input", 3, 4, (2, 3)))),
    (VScaled, "input_dy r6 (7, 13)", lambda: S.input_against_float64("cpu", _in("input_dy", 6, 96, (7, 13)))),
    (OneStoreBehindTheLastPlane, "input r4 (4, 4)", lambda: S.input_against_float64("cpu", _in("input", 4, 4, (4, 4)))),
    (OneStoreBehindTheLastPlane, "input r6 (12, 18)", lambda: S.input_against_float64("cpu", _in("input", 6, 96, (12, 18)))),
    (FusedDyPassWritesTheDescribedBuffer, "input_dy_norm skip", lambda: S.dynorm_against_float64("cpu", S.DYNORM_CASES[1])),
]


@pytest.mark.parametrize("at", range(len(MUTANTS)), ids=lambda i: f"{MUTANTS[i][0].__name__}-{MUTANTS[i][1].replace(' ', '_')}")
def test_an_emulator_with_one_planted_error_fails_the_body(at):
    mutant, _, body = MUTANTS[at]
    try:
        L.set_backend(EmuBackend())
        body()                                      # the plain emulator passes ...
        L.set_backend(mutant())
        with pytest.raises(AssertionError):         # ... and the mutant does not
            body()
    finally:
        L.set_backend(None)
        OPT.reset()
