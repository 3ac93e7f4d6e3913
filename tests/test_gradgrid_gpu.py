"""Whole-model gradients of every layer option against float64 -- on the device: PGCN.run on the real kernels over the option grid of
tests/test_gradgrid.py (norm x root_weight x bias x residual x dropout, both tasks, hidden widths 32 / 44 / 30 / 132, 1 - 3 ranks on one
GPU), two steps at lr = 0, against tests/_gradgrid_workers.model64: the loss, the logits, every parameter's gradient after the
all-reduce, the batch-norm buffers and the eval-mode logits through conftest.held_to_fixture (fixture: the float32 twin; every pair goes
to the parity log), and with tuning.wgrad_lane 0 and 1 in the same process: every gradient, logit, loss and buffer bit-identical.
Every rank of a group is one process that runs its configurations in sequence.  The eleven configurations without a weight seed
(_gradgrid_workers.NO_SEED) run on their least doubtful seed and are held like the rest, with no element excused."""
import pytest

import _gradgrid_workers as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gradgrid_gpu")))


@pytest.mark.parametrize("norm", W.NORMS)
@pytest.mark.parametrize("task", W.TASKS)
def test_main_grid_on_one_rank_with_and_without_the_side_lane(datasets, task, norm):
    assert W.run_group(datasets, task, W.main_grid(norm), 1, True, lanes=(0, 1)) > 2 * 16 * 2 * 6


@pytest.mark.parametrize("hidden", W.WIDTHS_AXIS)
@pytest.mark.parametrize("task", W.TASKS)
def test_width_axis(datasets, task, hidden):
    """44: float4 paths and a partly filled mask word; 30: the dense kernels refuse, the library route and the keep-words kernel run, the
    norms take their scalar paths; 132: above the dense kernels' 128."""
    W.run_group(datasets, task, W.width_axis(hidden), 1, True)


@pytest.mark.parametrize("P,lanes", [(2, (0, 1)), (3, (0,))])
@pytest.mark.parametrize("task", W.TASKS)
def test_ranks_hold_the_reduced_gradient(datasets, task, P, lanes):
    W.run_group(datasets, task, W.rank_subset(), P, True, lanes=lanes)
