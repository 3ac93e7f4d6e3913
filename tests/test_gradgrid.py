"""Whole-model gradients of every layer option against float64 -- the CPU side: PGCN.run on the checker-backed kernels over the option
grid (norm x root_weight x bias x residual x dropout, both tasks, three further hidden widths, 1 - 3 ranks over gloo), two steps at
lr = 0, against tests/_gradgrid_workers.model64: the loss, the logits, EVERY parameter's gradient after the all-reduce, the batch-norm
buffers and the eval-mode logits, each through conftest.held_to_fixture with the float32 twin as the fixture.  Here the reference and
the wiring of the autograd nodes are held (saved tensors, needs_input_grad branches, the order of returned gradients, the loss scale,
the all-reduce that must add and not average); tests/test_gradgrid_gpu.py holds the kernels in the same way.

The seed rule (_gradgrid_workers.pick_seed) as the issue states it -- no doubtful ReLU input at either step for some weight seed in
0 .. 15, doubtful = within 8 times the twin's largest error on that layer's ReLU input -- cannot be met by every configuration:
measured here on the CPU, from the reference alone, the smallest doubtful count over the 16 seeds is
    hidden 132 (435 600 ReLU inputs a step), single:     none 8, batch+root+drop 5, node+res+drop 7, none+root+bias+res+drop 1
    hidden 132,                              multilabel: none 2, batch+root+drop 5, node+res+drop 5, none+root+bias+res+drop 3
    hidden 44, multilabel: batch+root+drop 1;   hidden 32, multilabel: batch+res+drop 1, batch+bias+res+drop 1
and 0 for the other 109 (seed 0 for 48 of them, a seed below 5 for 99).  Those eleven are _gradgrid_workers.NO_SEED, with the
arithmetic that shows why the rule's premise fails for them.  They run on their least doubtful seed and are held to the same bound
with no element excused -- which asks more of the kernels than inputs without doubtful elements would; any OTHER configuration
without a seed fails its group."""
import pytest

import _gradgrid_workers as W


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gradgrid")))


def test_the_grid_is_the_grid():
    for norm in W.NORMS:
        assert len({W.tag(c) for c in W.main_grid(norm)}) == 16
    sub = W.rank_subset()
    assert len({W.tag(c) for c in sub}) == len(sub) >= 12 and W.covers_all_pairs(sub)
    assert not W.covers_all_pairs(sub[:4])
    full = {W.tag(c) for n in W.NORMS for c in W.main_grid(n)}
    assert {W.tag(c) for c in sub} <= full
    assert all(len(W.width_axis(h)) == 4 for h in W.WIDTHS_AXIS)
    # what may lack a weight seed is part of the grid, no more than the measured eleven, and none of it runs on 2 or 3 ranks
    grid = {t for h in W.WIDTHS_AXIS for t in map(W.tag, W.width_axis(h))} | full
    assert len(W.NO_SEED) == 11 and all(task in W.TASKS and t in grid for task, t in W.NO_SEED)
    assert not {t for _, t in W.NO_SEED} & {W.tag(c) for c in sub}


def test_parameter_names_under_a_norm(datasets):
    """bias=True under a norm: a bias on the OUTPUT layer only -- in the reference's statement, which the grid tests hold the model to."""
    c = W.config("batch", bias=True)
    names = W.parameter_names(W.widths_of("single", c), c)
    assert [n for n in names if n.endswith(".bias")] == ["3.bias"] and "0.bn_bias" in names and "3.bn_bias" not in names
    c = W.config("node", root=True, bias=True)
    names = W.parameter_names(W.widths_of("single", c), c)
    assert [n for n in names if n.endswith(".bias")] == ["3.bias"] and "2.ln_weight" in names and "3.root.weight" in names
    assert W.buffer_names([24, 32, 32, 32, 7], c) == [] and len(W.buffer_names([24, 32, 32, 32, 7], W.config("batch"))) == 6


def test_model64_is_the_existing_float64_loops_where_their_options_meet(datasets):
    """The new statement against the suite's older one-feature loops: the first training step's loss over the train rows (their record
    of epoch 0 without dropout is that step's own logits) to 1e-10 relative -- unit scales, zero shifts and biases, as those loops start.
    The multi-label loop pins the loss's divisor: the mean over the train rows' elements."""
    import _layernorm_workers as LW
    import _rootweight_workers as RW
    import torch
    for task, c, loop in (("single", W.config("node", residual=True), lambda d, w: LW.float64_reference(d, w, epochs=1, weight_seed=5, residual=True)),
                          ("single", W.config("batch"), lambda d, w: W.BW.float64_reference(d, w, epochs=1, weight_seed=5)),
                          ("single", W.config(root=True, bias=True), lambda d, w: RW.float64_reference(d, w, epochs=1, weight_seed=5)),
                          ("single", W.config(), lambda d, w: W.NW.float64_reference(d, w, epochs=1, weight_seed=5)),
                          ("multilabel", W.config(), lambda d, w: W.MW.float64_reference(d, w, epochs=1, weight_seed=5))):
        _, data = datasets[task]
        widths = W.widths_of(task, c)
        params = W.initial_params(widths, c, 5)
        for k, v in params.items():
            if v.dim() == 1:
                v.copy_(torch.ones_like(v) if k.endswith("weight") else torch.zeros_like(v))
        loss = float(W.model64(data, widths, params, dict(c, task=task), 0)[0])
        want = loop(data, widths)[0][0]["loss"]["train"]
        print("%s %s: model64 %.15g, the older loop %.15g" % (task, W.tag(c), loss, want))
        assert abs(loss - want) <= 1e-10 * abs(want), (task, W.tag(c))
        dropped = float(W.model64(data, widths, params, dict(c, task=task, dropout=W.DROPOUT), 0)[0])
        assert abs(dropped - loss) > 1e-6 * abs(loss)                      # (and dropout changes it)


@pytest.mark.parametrize("norm", W.NORMS)
@pytest.mark.parametrize("task", W.TASKS)
def test_main_grid_on_one_rank(datasets, task, norm):
    assert W.run_group(datasets, task, W.main_grid(norm), 1, False) > 16 * 2 * 6


@pytest.mark.parametrize("hidden", W.WIDTHS_AXIS)
@pytest.mark.parametrize("task", W.TASKS)
def test_width_axis(datasets, task, hidden):
    W.run_group(datasets, task, W.width_axis(hidden), 1, False)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("task", W.TASKS)
def test_ranks_hold_the_reduced_gradient(datasets, task, P):
    """The pairwise-covering subset on 2 and 3 ranks under the seeded random part vectors: the gradient after the all-reduce is held to
    the same bound on every rank."""
    W.run_group(datasets, task, W.rank_subset(), P, False)
