"""nirgan_instnorm_fwd / nirgan_instnorm_bwd without a GPU: the bodies of tests/instnorm_cases.py on the numpy emulator
(tests/emu_backend.py), and the checks that keep their derived bounds honest -- a float32 numpy restatement of the algorithm the header
of csrc/instnorm.hip documents (sums about pixel 0, in_nchunk chunks, row groups and the finalize added in the kernels' order, fp32 z)
inside every bound on every case, and emulators with one planted error each that must fail a body.  Bodies shared with
tests/test_gpu_instnorm.py."""
import numpy as np
import pytest

import instnorm_cases as Ic
from emu_backend import EmuBackend, arr, arr16, bf16_round, load_y, obj, reflect
from nirgan_hip import lib as L

f32 = np.float32


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("name", list(Ic.FWD))
def test_forward(emu, name):
    Ic.fwd_against_float64("cpu", name)
    assert set(emu.calls) <= {"in_fwd", "in_fwd_pre"}


@pytest.mark.parametrize("name", list(Ic.BWD))
def test_backward(emu, name):
    Ic.bwd_against_float64("cpu", name)


def test_argument_guards(emu):
    Ic.guards("cpu")


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def seq_sum(x, axis):
    """the elements along ``axis`` added one after the other in fp32"""
    x = np.moveaxis(x, axis, 0)
    acc = x[0].copy()
    for i in range(1, x.shape[0]):
        acc = (acc + x[i]).astype(f32)
    return acc


def grouped_sum(x, groups):
    """x [B][n][C]: group r adds elements r, r + groups, ... in order, then the groups are added in order (zeros fill the ragged end)"""
    B, n, Cc = x.shape
    steps = -(-n // groups)
    full = np.zeros((B, steps * groups, Cc), f32)
    full[:, :n] = x
    return seq_sum(seq_sum(full.reshape(B, steps, groups, Cc), 1), 1)


def chunk_partials(t, shape):
    """t [B][HW][C] fp32 -> [B][nchunk][C]: the per-chunk sums as a block forms them"""
    B, H, W, Cc = shape
    g = Ic.geometry(shape)
    full = np.zeros((B, g["nchunk"] * g["ppc"], Cc), f32)
    full[:, :H * W] = t
    per = full.reshape(B * g["nchunk"], g["ppc"], Cc)
    return grouped_sum(per, g["nrg"]).reshape(B, g["nchunk"], Cc)


def finalize(part, Cc):
    return grouped_sum(part, Ic.in_nrg(Ic.fin_cw(Cc)))


def twin_bits(x, truncate=False):
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    return ((u if truncate else bf16_round(x).view(np.uint32)) >> 16).astype(np.uint16)


class Restated(EmuBackend):
    """both entries in fp32 numpy, operation by operation in the kernels' order; ``mutate`` plants one error"""
    mutate = None

    def nirgan_instnorm_fwd(self, ref, stream=None):
        d, mu = obj(ref), self.mutate
        msg = self._in_fwd_guard(d)
        B, H, W, Cc = d.B, d.H, d.W, d.C
        shape, HW = (B, H, W, Cc), H * W
        if not msg and d.norm and d.ws_elems < B * (d.stats_chunks * 4 if d.stats_chunks > 0 else Ic.in_nchunk(B, HW, Cc) * 2) * Cc:
            msg = "in_fwd: ws too small"
        if msg:
            return self._fail(msg)
        y = load_y(d.y, B * HW * Cc, d.y_bf16).reshape(B, HW, Cc).astype(f32)
        inv = f32(1.0) / f32(HW)
        if d.norm:
            if d.stats_chunks > 0:
                p = arr(d.ws, B * d.stats_chunks * 4 * Cc).reshape(B, d.stats_chunks, 4, Cc)
                k = p[:, 0, 0].copy()
                dk = p[:, :, 0] - k[:, None]
                a1, a2, n = p[:, :, 1], p[:, :, 2], p[:, :, 3]
                s1 = finalize((a1 + n * dk).astype(f32), Cc)
                cross = f32(0.0) if mu == "re-basing without 2 dk s1" else f32(2.0) * dk * a1
                s2 = finalize(((a2 + cross).astype(f32) + (n * dk).astype(f32) * dk).astype(f32), Cc)
                if d.stats_shift and mu != "stats_shift ignored":
                    k = (k + arr(d.stats_shift, Cc)).astype(f32)
            else:
                k = y[:, 0].copy()
                v = (y - k[:, None]).astype(f32)
                part = arr(d.ws, B * Ic.in_nchunk(B, HW, Cc) * 2 * Cc).reshape(B, -1, 2, Cc)
                part[:, :, 0], part[:, :, 1] = chunk_partials(v, shape), chunk_partials((v * v).astype(f32), shape)
                s1, s2 = finalize(part[:, :, 0], Cc), finalize(part[:, :, 1], Cc)
            m = (s1 * inv).astype(f32)
            var = np.maximum((s2 * inv).astype(f32) - (m * m).astype(f32), f32(0)).astype(f32)
            if mu == "unbiased variance":
                var = (var * f32(HW / (HW - 1))).astype(f32)
            if mu == "eps outside the root":
                rstd = (f32(1) / (np.sqrt(var) + f32(d.eps))).astype(f32)
            else:
                rstd = (f32(1) / np.sqrt((var + f32(d.eps)).astype(f32))).astype(f32)
            mean = m if mu == "mean without k" else (k + m).astype(f32)
            arr(d.mean, B * Cc).reshape(B, Cc)[:] = mean
            arr(d.rstd, B * Cc).reshape(B, Cc)[:] = rstd
            z = ((y - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32)
        else:
            z = y
        if not d.out and not d.out_bf16:
            return 0
        if d.act == 1:
            z = np.where(z > 0, z, f32(0))
        elif d.act == 2:
            z = np.where(z > 0, z, (z * f32(d.slope)).astype(f32)) if mu != "slope on the positive side" else \
                np.where(z > 0, (z * f32(d.slope)).astype(f32), z)
        a = z.reshape(B, H, W, Cc)
        if d.residual:
            rp = 0 if mu == "residual read at r_pad = 0" else d.r_pad
            a = (a + arr(d.residual, B * d.r_hp * d.r_wp * Cc).reshape(B, d.r_hp, d.r_wp, Cc)[:, rp:rp + H, rp:rp + W]).astype(f32)
        P = d.o_pad
        if d.border == 1 and P > 0:
            if mu == "symmetric halo":
                hh, ww = (np.clip(np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i)), 0, n - 1)
                          for i, n in ((np.arange(d.o_hp) - P, H), (np.arange(d.o_wp) - P, W)))
            else:
                hh, ww = reflect(np.arange(d.o_hp) - P, H), reflect(np.arange(d.o_wp) - P, W)
            full, region = a[:, hh][:, :, ww], (slice(None), slice(None), slice(None))
        else:
            full, region = a, (slice(None), slice(P, P + H), slice(P, P + W))
        if d.out:
            arr(d.out, B * d.o_hp * d.o_wp * Cc).reshape(B, d.o_hp, d.o_wp, Cc)[region] = full
        if d.out_bf16:
            arr16(d.out_bf16, B * d.o_hp * d.o_wp * Cc).reshape(B, d.o_hp, d.o_wp, Cc)[region] = twin_bits(full, mu == "twin truncated")
        return 0

    def nirgan_instnorm_bwd(self, ref, stream=None):
        d, mu = obj(ref), self.mutate
        msg = self._in_bwd_guard(d)
        if msg:
            return self._fail(msg)
        B, H, W, Cc = d.B, d.H, d.W, d.C
        shape, HW = (B, H, W, Cc), H * W
        pre = d.norm and d.sums_chunks > 0
        ga = np.zeros((B, H, W, Cc), f32)
        if pre and d.gsum_out:
            ga = arr(d.gsum_out, B * HW * Cc).reshape(B, H, W, Cc).copy()
        else:
            if d.g:
                g = load_y(d.g, B * d.g_hp * d.g_wp * Cc, d.g_bf16).reshape(B, d.g_hp, d.g_wp, Cc).astype(f32)
                P = d.g_pad
                if d.g_fold:
                    if mu == "fold counts the edge row twice":
                        hh, ww = (np.clip(np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i)), 0, n - 1)
                                  for i, n in ((np.arange(d.g_hp) - P, H), (np.arange(d.g_wp) - P, W)))
                    else:
                        hh, ww = reflect(np.arange(d.g_hp) - P, H), reflect(np.arange(d.g_wp) - P, W)
                    inner_h, inner_w = (np.arange(d.g_hp) >= P) & (np.arange(d.g_hp) < P + H), (np.arange(d.g_wp) >= P) & (np.arange(d.g_wp) < P + W)
                    for i in range(d.g_hp):
                        for j in range(d.g_wp):
                            if mu == "fold without the corner image" and not inner_h[i] and not inner_w[j]:
                                continue
                            ga[:, hh[i], ww[j]] = (ga[:, hh[i], ww[j]] + g[:, i, j]).astype(f32)
                else:
                    ga = g[:, P:P + H, P:P + W].copy()
            if d.g2:
                ga = (ga + arr(d.g2, B * HW * Cc).reshape(B, H, W, Cc)).astype(f32)
            if d.gsum_out:
                arr(d.gsum_out, B * HW * Cc).reshape(B, H, W, Cc)[:] = ga
        ga = ga.reshape(B, HW, Cc)
        z = None
        if d.norm or d.act in (1, 2):
            y = load_y(d.y, B * HW * Cc, d.y_bf16).reshape(B, HW, Cc).astype(f32)
            if d.norm:
                mean, rstd = arr(d.mean, B * Cc).reshape(B, 1, Cc), arr(d.rstd, B * Cc).reshape(B, 1, Cc)
                z = ((y - mean).astype(f32) * rstd).astype(f32)
            else:
                z = y
        gz = ga
        if d.act in (1, 2):
            gz = np.where(z > 0, ga, (ga * f32(0.0 if d.act == 1 else d.slope)).astype(f32))
        nchunk = Ic.in_nchunk(B, HW, Cc)
        if not d.norm:
            o = arr(d.dy, B * d.d_hp * d.d_wp * Cc).reshape(B, d.d_hp, d.d_wp, Cc)
            o[:, d.d_pad:d.d_pad + H, d.d_pad:d.d_pad + W] = gz.reshape(B, H, W, Cc)
            if d.dy_bf16:
                t = arr16(d.dy_bf16, o.size).reshape(o.shape)
                t[:, d.d_pad:d.d_pad + H, d.d_pad:d.d_pad + W] = twin_bits(gz.reshape(B, H, W, Cc))
            if d.dbias:
                rows = arr(d.ws, B * nchunk * Cc).reshape(B * nchunk, Cc)
                rows[:] = chunk_partials(gz, shape).reshape(B * nchunk, Cc)
                db = arr(d.dbias, Cc)
                if mu == "dbias overwritten":
                    db[:] = 0
                db[:] = (db + seq_sum(rows, 0)).astype(f32)
            return 0
        pch = d.sums_chunks if pre else nchunk
        part = arr(d.ws, B * pch * 2 * Cc).reshape(B, pch, 2, Cc)
        if not pre:
            part[:, :, 0], part[:, :, 1] = chunk_partials(gz, shape), chunk_partials((gz * z).astype(f32), shape)
        inv = f32(1.0) / f32(HW)
        m1, m2 = (finalize(part[:, :, 0], Cc) * inv).astype(f32), (finalize(part[:, :, 1], Cc) * inv).astype(f32)
        mm = arr(d.ws, B * pch * 2 * Cc + B * 2 * Cc)[B * pch * 2 * Cc:].reshape(B, 2, Cc)
        mm[:, 0], mm[:, 1] = m1, m2
        if not d.dy and not d.dy_bf16:
            return 0
        t = f32(0.0) if mu == "dy without the z m2 term" else (z * m2[:, None]).astype(f32)
        inner = ((gz - m1[:, None]).astype(f32) - t).astype(f32)
        dy = (inner if mu == "dy without rstd" else (rstd * inner).astype(f32)).reshape(B, H, W, Cc)
        if d.dy:
            arr(d.dy, B * d.d_hp * d.d_wp * Cc).reshape(B, d.d_hp, d.d_wp, Cc)[:, d.d_pad:d.d_pad + H, d.d_pad:d.d_pad + W] = dy
        if d.dy_bf16:
            arr16(d.dy_bf16, B * d.d_hp * d.d_wp * Cc).reshape(B, d.d_hp, d.d_wp, Cc)[:, d.d_pad:d.d_pad + H, d.d_pad:d.d_pad + W] = twin_bits(dy)
        return 0


@pytest.fixture()
def restated():
    L.set_backend(Restated())
    yield
    L.set_backend(None)


@pytest.mark.parametrize("name", list(Ic.FWD))
def test_fp32_restatement_of_the_forward_lies_inside_the_bounds(restated, name):
    Ic.fwd_against_float64("cpu", name, family="fp32 in_fwd")


@pytest.mark.parametrize("name", list(Ic.BWD))
def test_fp32_restatement_of_the_backward_lies_inside_the_bounds(restated, name):
    Ic.bwd_against_float64("cpu", name, family="fp32 in_bwd")


def test_fp32_restatement_refuses_what_the_library_refuses(restated):
    Ic.guards("cpu")


# ------------------------------------------------------------------------------------------------ planted errors
MUTANTS = [("unbiased variance", "fwd", "9"), ("unbiased variance", "fwd", "5"), ("eps outside the root", "fwd", "1"),
           ("mean without k", "fwd", "3"), ("re-basing without 2 dk s1", "fwd", "11-shift"), ("re-basing without 2 dk s1", "fwd", "11-noshift"),
           ("stats_shift ignored", "fwd", "11-shift"), ("slope on the positive side", "fwd", "2"), ("symmetric halo", "fwd", "1"),
           ("symmetric halo", "fwd", "2"), ("residual read at r_pad = 0", "fwd", "3"), ("residual read at r_pad = 0", "fwd", "10"),
           ("twin truncated", "fwd", "5"), ("twin truncated", "fwd", "8"),
           ("fold without the corner image", "bwd", "1"), ("fold without the corner image", "bwd", "2"),
           ("fold counts the edge row twice", "bwd", "1"), ("fold counts the edge row twice", "bwd", "5"),
           ("dy without the z m2 term", "bwd", "3"), ("dy without the z m2 term", "bwd", "11-gsum"), ("dy without rstd", "bwd", "6"),
           ("dy without rstd", "bwd", "chained"), ("dbias overwritten", "bwd", "10")]


class DbiasUnderNorm(EmuBackend):
    """what the emulator did before: sum dy added to dbias with norm = 1, which the library never does"""

    def nirgan_instnorm_bwd(self, ref, stream=None):
        rc, d = super().nirgan_instnorm_bwd(ref), obj(ref)
        if rc == 0 and d.norm and d.dbias and d.dy:
            arr(d.dbias, d.C)[:] += arr(d.dy, d.B * d.d_hp * d.d_wp * d.C).reshape(-1, d.C).sum(0)
        return rc


@pytest.mark.parametrize("at", range(len(MUTANTS)), ids=lambda i: "-".join(MUTANTS[i]).replace(" ", "_"))
def test_an_emulator_with_one_planted_error_fails_the_body(at):
    mutate, kind, name = MUTANTS[at]
    body = (lambda: Ic.fwd_against_float64("cpu", name)) if kind == "fwd" else (lambda: Ic.bwd_against_float64("cpu", name))
    try:
        L.set_backend(Restated())
        body()                                      # the restatement passes ...
        bad = Restated()
        bad.mutate = mutate
        L.set_backend(bad)
        with pytest.raises(AssertionError):         # ... and with the planted error it does not
            body()
    finally:
        L.set_backend(None)


def test_an_emulator_that_adds_to_dbias_under_norm_fails_the_body():
    try:
        L.set_backend(DbiasUnderNorm())
        with pytest.raises(AssertionError, match="dbias"):
            Ic.bwd_against_float64("cpu", "3")
    finally:
        L.set_backend(None)

