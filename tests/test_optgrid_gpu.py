"""Whole-model gradients of aggr="max", propagate=K and drop_edge=P against float64 -- on the device: the groups of
tests/test_optgrid.py on the real provider (asserted: HipKernels, max / DropEdge structures that are not the composed ones, and the
composed propagation steps raise), against tests/_optgrid_workers.model64x through conftest.held_to_fixture (fixture: the float32 twin;
every pair goes to the parity log).  One rank and P = 2 run every configuration with tuning.wgrad_lane 0 and 1 in the same process:
every gradient, logit, loss and buffer bit-identical; P = 3 runs lane 0.  Every rank of a group is one process -- three at the most --
that runs its configurations in sequence; the shapes are the grid's own (n = 1 100, hidden 32 / 44 / 30 / 132, K <= 3).  No test here
may take longer than the slowest of tests/test_gradgrid_gpu.py: the list on one rank and the width axis at 132 are therefore two worker
groups each (DESIGN.md section 2 has the measured durations)."""
import pytest

import _optgrid_workers as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.GG.make_datasets(str(tmp_path_factory.mktemp("optgrid_gpu")))


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("task", W.TASKS)
def test_option_grid_on_one_rank_with_and_without_the_side_lane(datasets, task, half):
    """The list and the dense pair, in two worker groups of eight (_optgrid_workers.one_rank_groups)."""
    assert W.run_group_x(datasets, task, W.one_rank_groups()[half], 1, True, lanes=(0, 1)) > 2 * 8 * 2 * 6


@pytest.mark.parametrize("group", W.width_groups(), ids=lambda g: g[0])
def test_width_axis(datasets, group):
    """44: float4 paths and a partly filled mask word; 30: no multiple of 4; 132: above the dense kernels' 128 (two groups)."""
    W.run_group_x(datasets, "single", group[1], 1, True)


@pytest.mark.parametrize("P,lanes", [(2, (0, 1)), (3, (0,))])
@pytest.mark.parametrize("task", W.TASKS)
def test_ranks_hold_the_reduced_gradient(datasets, task, P, lanes):
    W.run_group_x(datasets, task, W.rank_subset_x(), P, True, lanes=lanes)
