"""The fused train step over the pairwise option matrix of tests/step_matrix_cases.py on the MI355X: every row, from seeded weights, held
to one float64 reference step -- first step, second step (re-seeded from the device's parameters), shape switch on three rows, the
Lightning sequence on the same row, and a bitwise repeat.  Bounds: 1e-3 on pred, the losses and every gradient tensor's relative L2 at
ngf 8 (2e-3 on one-element tensors); the two ngf-32 rows take the bounds of test_gpu_nets.test_medium_width_nets_take_the_winograd_paths
(1e-2 L2, 1e-1 max) for the reason its comment gives.  The same bodies run on the emulators in tests/test_step_matrix_emulated.py,
where the table's coverage and the stock-fp32 condition on every row's data seed are checked.  profiles/step_matrix_gpu.txt holds the
printed error / bound ratios of a run."""
import pytest

import step_matrix_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("rid", [r.id for r in M.ROWS + M.WIDE])
def test_row(rid):
    row = M.BY_ID[rid]
    M.run_row(DEV, row, M.gpu_bounds(row))
