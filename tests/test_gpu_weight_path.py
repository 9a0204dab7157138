"""The weight pack, split, slab-sum and Winograd weight-transform launches on the MI355X (nirgan_pack_rows / _bf16 / _batch,
nirgan_reduce_rows / _part / _batch, nirgan_wino6_weights / _r / _x3 / _batch, nirgan_wino6_wgrad_finish / _r / _batch, and the engine's
job-table builders), each raw entry against bit-exact host expectations and float64 under the derived bounds of
tests/weight_path_cases.py (cases, inputs, references, bounds and bodies are there)."""
import pytest

import weight_path_cases as Wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", Wc.PACK_CASES, ids=str)
def test_pack_rows(case):
    Wc.pack_against_host(DEV, case)


@pytest.mark.parametrize("njobs", sorted(Wc.PACK_TABLES))
def test_pack_rows_batch(njobs):
    Wc.pack_batch_against_host(DEV, njobs)


def test_pack_rows_batch_planes_of_special_values():
    Wc.pack_batch_specials(DEV)


@pytest.mark.parametrize("nsplit", Wc.NSPLITS)
def test_reduce_rows(nsplit):
    Wc.reduce_against_float64(DEV, nsplit)


@pytest.mark.parametrize("njobs", sorted(Wc.REDUCE_TABLES))
def test_reduce_rows_batch(njobs):
    Wc.reduce_batch_against_float64(DEV, njobs)


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_weights(v, flip):
    Wc.wino_weights_against_float64(DEV, v, flip)


@pytest.mark.parametrize("njobs", sorted(Wc.WINO_TABLES))
def test_wino6_weights_batch(njobs):
    Wc.wino_batch_against_single(DEV, njobs)


@pytest.mark.parametrize("nsplit", Wc.FIN_NSPLITS)
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_wgrad_finish(v, nsplit):
    Wc.finish_against_float64(DEV, v, nsplit)


@pytest.mark.parametrize("layers", Wc.FIN_BATCH_LAYERS)
@pytest.mark.parametrize("v", Wc.VARIANTS)
def test_wino6_wgrad_finish_batch(v, layers):
    Wc.finish_batch_against_single(DEV, v, layers)


def test_table_builders():
    Wc.table_builders(DEV)


def test_guards():
    Wc.guards(DEV)


def test_pack_rows_reads_zero_past_src_elems():
    Wc.pack_clamps_past_src_elems(DEV)


def test_reduce_rows_drops_stores_past_dst_elems():
    Wc.reduce_clamps_past_dst_elems(DEV)
