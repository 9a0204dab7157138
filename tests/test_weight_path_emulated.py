"""The weight pack, split, slab-sum and Winograd weight-transform launches without a GPU: the bodies of tests/weight_path_cases.py on the
numpy emulator (tests/emu_backend.py), and the checks that keep their expectations honest -- the stated input conditions, the host's
round-to-nearest-even against torch's own conversion, eager fp32 torch of every bounded formula inside its bound, the Winograd matrices
against a direct correlation, and emulators with one planted, subtle error each that must fail a named body.  Bodies shared with
tests/test_gpu_weight_path.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import weight_path_cases as Wc
from emu_backend import EmuBackend, arr, arr16, bf16_round
from nirgan_hip import lib as L
from streaming_cases import U, within


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("case", Wc.PACK_CASES, ids=str)
def test_pack_rows(emu, case):
    Wc.pack_conditions_hold(case)
    Wc.pack_against_host("cpu", case)
    assert emu.calls == ["pack"] * (2 if case[3] else 1)


@pytest.mark.parametrize("njobs", sorted(Wc.PACK_TABLES))
def test_pack_rows_batch(emu, njobs):
    Wc.pack_table_conditions_hold(njobs)
    Wc.pack_batch_against_host("cpu", njobs)


def test_pack_rows_batch_planes_of_special_values(emu):
    Wc.pack_batch_specials("cpu")


@pytest.mark.parametrize("nsplit", Wc.NSPLITS)
def test_reduce_rows(emu, nsplit):
    Wc.reduce_against_float64("cpu", nsplit)
    assert {"reduce", "reduce_part"} <= set(emu.calls)


@pytest.mark.parametrize("njobs", sorted(Wc.REDUCE_TABLES))
def test_reduce_rows_batch(emu, njobs):
    Wc.reduce_table_conditions_hold(njobs)
    Wc.reduce_batch_against_float64("cpu", njobs)


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_weights(emu, v, flip):
    Wc.wino_weights_against_float64("cpu", v, flip)


@pytest.mark.parametrize("njobs", sorted(Wc.WINO_TABLES))
def test_wino6_weights_batch(emu, njobs):
    Wc.wino_batch_against_single("cpu", njobs)


@pytest.mark.parametrize("nsplit", Wc.FIN_NSPLITS)
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_wgrad_finish(emu, v, nsplit):
    Wc.finish_against_float64("cpu", v, nsplit)


@pytest.mark.parametrize("layers", Wc.FIN_BATCH_LAYERS)
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_wgrad_finish_batch(emu, v, layers):
    Wc.finish_batch_against_single("cpu", v, layers)
    assert "wino6_fin_batch" in emu.calls


def test_table_builders(emu):
    Wc.table_builders("cpu")


def test_guards(emu):
    Wc.guards("cpu")


def test_the_emulator_refuses_what_the_kernels_clamp(emu):
    Wc.clamps_refused_by_the_emulator("cpu")


# ------------------------------------------------------------------------------------------------ the reference alone
def test_host_rounding_is_torchs_round_to_nearest_even():
    bits = np.concatenate([Wc.pack_values(4096, 3), Wc.HEAD])
    ours = Wc.rne_bf16_bits(bits)
    theirs = torch.from_numpy(bits.view(np.int32)).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ours, theirs)
    # the ties go to the even upper half, their neighbours to the nearer one
    assert list(Wc.rne_bf16_bits(Wc.HEAD[:4])) == [0x3F80, 0x3F82, 0x4001, 0xC002]
    x = Wc.as_f32(bits)
    planes = Wc.split3_host(x)
    assert Wc.planes_sum_exactly(planes, x)
    rest = x.copy()
    for p in planes:            # each term is torch's rounding of what the previous ones left
        t = torch.from_numpy(rest).to(torch.bfloat16)
        assert np.array_equal(t.view(torch.int16).numpy().view(np.uint16), p)
        rest = rest - t.float().numpy()
    assert (rest == 0).all()


def test_the_integer_slabs_sum_exactly():
    """every partial sum of the integer pass is an integer far below 2^24, in any association"""
    s = Wc.slab_values((35, 3, 516), True, 1)
    assert set(s.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0} and (35 + 1) * 2 < 2 ** 24


@pytest.mark.parametrize("nsplit", Wc.NSPLITS)
def test_eager_fp32_slab_sums_lie_inside_the_bound(nsplit):
    for K, N, acc, kind in Wc.reduce_combos():
        imap, stride, dst_elems = Wc.reduce_map(kind, N, K)
        slabs = Wc.slab_values((nsplit, N, K), False, 31 * nsplit + K + N)
        old = Wc.slab_values((dst_elems,), False, 17 * nsplit + K)
        ref, A, owned = Wc.reduce_expect(slabs, old, imap, stride, dst_elems, acc, 0, N)
        idx, ok = Wc.scatter_index(imap, stride, N)
        got = old.clone()
        s = slabs.sum(0)[:, torch.from_numpy(ok)]
        got[torch.from_numpy(idx)] = got[torch.from_numpy(idx)] + s if acc else s
        within("eager reduce_rows", f"{nsplit} {K} {N} {acc} {kind}", got[torch.from_numpy(owned)], torch.from_numpy(ref[owned]),
               torch.from_numpy((nsplit + 1) * U * A[owned]))
        assert (imap < 0).any() == (kind == "syn")


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_eager_fp32_weight_transform_lies_inside_the_bound(v, flip):
    for K, Cc in Wc.WINO_KC:
        w, ref, bound = Wc.wino_w_case(v, K, Cc, flip)
        within("eager wino6_weights", f"r{v} {K} {Cc} {flip}", Wc.wino_w_eager32(v, K, Cc, flip), ref, bound)


@pytest.mark.parametrize("nsplit", Wc.FIN_NSPLITS)
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_eager_fp32_finish_lies_inside_the_bound(v, nsplit):
    for K, Cc in Wc.FIN_KC:
        for acc in (0, 1):
            ref, bound = Wc.finish_ref(v, nsplit, K, Cc, acc)
            within("eager wino6_wgrad_finish", f"r{v} {nsplit} {K} {Cc} {acc}", Wc.finish_eager32(v, nsplit, K, Cc, acc), ref, bound)


@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_the_winograd_matrices_reproduce_a_direct_correlation(v):
    """the G, B^T, A^T the references use, against the operation itself in float64: 36, 49 and 64 planes"""
    r, mo, n = Wc.w6_geo(v)
    assert n * n == {3: 36, 4: 49, 6: 64}[v]
    for seed in range(4):
        assert Wc.winograd_identity_error(v, seed) < 1e-12


# ------------------------------------------------------------------------------------------------ planted errors
def _u16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


class BatchPackTakesThePlaneMFromTheValue(EmuBackend):
    """m = the rounding of what the value's own upper half leaves (x - trunc(x)), not of the remainder x - h: wrong wherever h was
    rounded up"""

    def nirgan_pack_rows_batch(self, jobs, njobs, total_blocks, stream=None):
        rc = super().nirgan_pack_rows_batch(jobs, njobs, total_blocks)
        if rc or not jobs:
            return rc
        J = np.ctypeslib.as_array((C.c_int64 * (njobs * 10)).from_address(int(jobs))).reshape(njobs, 10)
        for src, dst, imap, src_elems, N, K, stride, first, w3, plane in J:
            if w3:
                n = int(N) * int(K)
                x = arr(int(dst), n)
                h = bf16_round(x)
                m = bf16_round(x - (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32))
                arr16(int(w3) + 2 * int(plane), n)[:] = _u16(m)
                arr16(int(w3) + 4 * int(plane), n)[:] = _u16(bf16_round(x - h - m))
        return rc


class Bf16ByTruncation(EmuBackend):
    def nirgan_pack_rows(self, src, src_elems, stride, imap, dst, N, K, stream=None, bf16=False):
        if not bf16:
            return super().nirgan_pack_rows(src, src_elems, stride, imap, dst, N, K)
        tmp = np.zeros((N, K), dtype=np.float32)
        rc = super().nirgan_pack_rows(src, src_elems, stride, imap, tmp.ctypes.data, N, K)
        if rc == 0:
            arr16(int(dst), N * K)[:] = _u16(tmp).reshape(-1)
        return rc


class ReduceBatchReadsAccumulateFromJob0(EmuBackend):
    def nirgan_reduce_rows_batch(self, jobs, njobs, total_blocks, stream=None):
        J = np.ctypeslib.as_array((C.c_int64 * (njobs * 10)).from_address(int(jobs))).reshape(njobs, 10).copy()
        J[:, 7] = (J[:, 7] & 0xffffffff) | (J[0, 7] >> 32 << 32)
        return super().nirgan_reduce_rows_batch(J.ctypes.data, njobs, total_blocks)


class SkipsTheLastFloat4OfARowOf256kPlus4(EmuBackend):
    """K % 256 == 4: the row's last float4 is the only one of its 256-column block"""

    def nirgan_pack_rows(self, src, src_elems, stride, imap, dst, N, K, stream=None, bf16=False):
        if bf16 or K % 256 != 4 or not dst:
            return super().nirgan_pack_rows(src, src_elems, stride, imap, dst, N, K, bf16=bf16)
        o = arr(dst, N * K).reshape(N, K)
        keep = o[:, K - 4:].copy()
        rc = super().nirgan_pack_rows(src, src_elems, stride, imap, dst, N, K)
        o[:, K - 4:] = keep
        return rc

    def nirgan_reduce_rows(self, slabs, nsplit, N, K, imap, dst, dst_elems, stride, accumulate, stream=None):
        if K % 256 != 4 or K < 8:
            return super().nirgan_reduce_rows(slabs, nsplit, N, K, imap, dst, dst_elems, stride, accumulate)
        m = arr(imap, K, np.int32).copy()
        m[K - 4:] = -1
        return super().nirgan_reduce_rows(slabs, nsplit, N, K, m.ctypes.data, dst, dst_elems, stride, accumulate)


class FlipTransposesButDoesNotReverseTheTaps(EmuBackend):
    def nirgan_wino6_weights_r(self, w, K, Cc, r, flip, U, stream=None, U3=None):
        v = self._r6(r)
        if not flip or v not in self._W6:
            return super().nirgan_wino6_weights_r(w, K, Cc, r, flip, U, U3=U3)
        f = self._geo6(v)[0]
        turned = np.ascontiguousarray(arr(w, K * Cc * f * f).reshape(Cc, K, f, f)[:, :, ::-1, ::-1])      # reversed twice: not at all
        return super().nirgan_wino6_weights_r(turned.ctypes.data, K, Cc, r, flip, U, U3=U3)


class FinishOmitsTheLastSplitOf4kPlus1(EmuBackend):
    def nirgan_wino6_wgrad_finish_r(self, slabs, nsplit, K, Cc, r, grad, accumulate, stream=None):
        v = self._r6(r)
        if nsplit % 4 != 1 or v not in self._W6 or not slabs:
            return super().nirgan_wino6_wgrad_finish_r(slabs, nsplit, K, Cc, r, grad, accumulate)
        n = self._geo6(v)[2]
        short = arr(slabs, n * n * nsplit * K * Cc).reshape(n * n, nsplit, K * Cc).copy()
        short[:, nsplit - 1] = 0
        return super().nirgan_wino6_wgrad_finish_r(short.ctypes.data, nsplit, K, Cc, r, grad, accumulate)


class ReduceScaled(EmuBackend):
    """a relative error of 2^-18 in a two-term sum"""

    def nirgan_reduce_rows(self, slabs, nsplit, N, K, imap, dst, dst_elems, stride, accumulate, stream=None):
        s = arr(slabs, nsplit * N * K).copy() * np.float32(1 + 2.0 ** -18) if slabs and N > 0 and K > 0 else None
        return super().nirgan_reduce_rows(s.ctypes.data if s is not None else slabs, nsplit, N, K, imap, dst, dst_elems, stride, accumulate)


class WinoBatchTakesTheFlipOfJob0(EmuBackend):
    def nirgan_wino6_weights_batch(self, jobs, njobs, total_blocks, stream=None):
        J = np.ctypeslib.as_array((C.c_int64 * (njobs * 8)).from_address(int(jobs))).reshape(njobs, 8).copy()
        J[:, 4] = J[0, 4]                                  # every job takes job 0's transpose_flip
        return super().nirgan_wino6_weights_batch(J.ctypes.data, njobs, total_blocks)


MUTANTS = [
    (BatchPackTakesThePlaneMFromTheValue, "pack_rows_batch of 1", lambda: Wc.pack_batch_against_host("cpu", 1)),
    (BatchPackTakesThePlaneMFromTheValue, "pack_rows_batch of 7", lambda: Wc.pack_batch_against_host("cpu", 7)),
    (Bf16ByTruncation, "pack_rows_bf16 (1, 8)", lambda: Wc.pack_against_host("cpu", ("cf", 1, 8, True))),
    (Bf16ByTruncation, "pack_rows_bf16 (3, 1032)", lambda: Wc.pack_against_host("cpu", ("tf", 3, 1032, True))),
    (Bf16ByTruncation, "pack_rows_batch of 7", lambda: Wc.pack_batch_against_host("cpu", 7)),
    (ReduceBatchReadsAccumulateFromJob0, "reduce_rows_batch of 2", lambda: Wc.reduce_batch_against_float64("cpu", 2)),
    (ReduceBatchReadsAccumulateFromJob0, "reduce_rows_batch of 5", lambda: Wc.reduce_batch_against_float64("cpu", 5)),
    (SkipsTheLastFloat4OfARowOf256kPlus4, "pack_rows (2, 1028)", lambda: Wc.pack_against_host("cpu", ("cd1", 2, 1028, False))),
    (SkipsTheLastFloat4OfARowOf256kPlus4, "reduce_rows nsplit 5", lambda: Wc.reduce_against_float64("cpu", 5)),
    (SkipsTheLastFloat4OfARowOf256kPlus4, "emit_deferred_reduce_rows", lambda: Wc.deferred_reduce_equals_single("cpu")),
    (FlipTransposesButDoesNotReverseTheTaps, "wino6_weights r3 flip", lambda: Wc.wino_weights_against_float64("cpu", 3, 1)),
    (FlipTransposesButDoesNotReverseTheTaps, "wino6_weights r4 flip", lambda: Wc.wino_weights_against_float64("cpu", 4, 1)),
    (FlipTransposesButDoesNotReverseTheTaps, "wino6_weights r6 flip", lambda: Wc.wino_weights_against_float64("cpu", 6, 1)),
    (FinishOmitsTheLastSplitOf4kPlus1, "wino6_wgrad_finish r3 nsplit 5", lambda: Wc.finish_against_float64("cpu", 3, 5)),
    (FinishOmitsTheLastSplitOf4kPlus1, "wino6_wgrad_finish r6 nsplit 1", lambda: Wc.finish_against_float64("cpu", 6, 1)),
    (FinishOmitsTheLastSplitOf4kPlus1, "wino6_wgrad_finish_batch r4 of 3", lambda: Wc.finish_batch_against_single("cpu", 4, 3)),
    (ReduceScaled, "reduce_rows nsplit 2", lambda: Wc.reduce_against_float64("cpu", 2)),
    (WinoBatchTakesTheFlipOfJob0, "wino6_weights_batch of 2", lambda: Wc.wino_batch_against_single("cpu", 2)),
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
