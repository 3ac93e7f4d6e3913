"""Whole-model gradients of the three layer options merged after the gradient grid -- aggr="max", propagate=K (APPNP) and drop_edge=P
-- against float64, the CPU side: PGCN.run on the checker-backed kernels over gloo (the composed routes of the three), over a
pairwise-covering list of norm x root_weight x bias x residual x dropout x aggr x propagate (14 configurations at hidden 32, two more on
dense_layers), both tasks, three further hidden widths, 1 - 3 ranks, two steps at lr = 0, against tests/_optgrid_workers.model64x: the
loss, the logits, EVERY parameter's gradient after the all-reduce, the batch-norm buffers and the eval-mode logits through
conftest.held_to_fixture with the float32 twin as fixture, as tests/test_gradgrid.py holds the older options.  What is new on the
grid: a skip connection into backward_max / backward_drop, propagate over max and over DropEdge layers (the undropped matrix; the
shared send / halo slabs at two widths), propagate under a norm, a root weight and a residual link, the multi-label task (41
propagated labels), three ranks, widths other than 32, and the eval mode of max and of DropEdge + propagate models.
tests/test_optgrid_gpu.py holds the kernels in the same way.

The seed rule is GG's, unchanged, applied from the reference alone (for max: model64x selecting by the definition on its own layer
input).  Measured here on the CPU, from the reference alone, the smallest doubtful count over the 16 seeds is
    hidden 132 (435 600 ReLU inputs a step), single: node+res+drop+max 1, batch+root+dropedge+K3 10, none+root+bias+res+K1 0 | 2
and 0 for the other 38: all 32 of the list and the dense pair in both tasks (seed 0 for 13 of them, a seed below 5 for 28, the
largest 10) and the width axis at 44 and 30 (seeds 5, 4, 0 and 2, 14, 0).  The third count depends on the host's fp32 products (the
twin): 4 - 12 doubtful inputs per seed and none at seed 14 here, 2 - 14 and 2 at seed 14 on the host of the device runs, where the
rule therefore finds no seed.  Those three are _optgrid_workers.NO_SEED_X: they run on their least doubtful seed (14 for the third,
on both hosts) and are held to the same bound with no element excused; any OTHER configuration without a seed fails its group, and
nothing that runs on 2 or 3 ranks is listed."""
import numpy as np
import pytest
import torch

import _optgrid_workers as W

GG, AW, PW, DW = W.GG, W.AW, W.PW, W.DW


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return GG.make_datasets(str(tmp_path_factory.mktemp("optgrid")))


def test_the_list_covers_every_pair():
    from conftest import pkg
    M = pkg("PGCN")
    grid = W.option_grid()
    assert len({W.tag(c) for c in grid}) == len(grid) <= 16 and W.covers_all_pairs(grid)
    assert not W.covers_all_pairs(grid[:9]) and not W.covers_all_pairs([c for c in grid if c["aggr"] != "max"])
    assert all(c["hidden"] == W.HIDDEN and not c["dense"] for c in grid)
    dense = W.dense_configs()
    assert [W.tag(c) for c in dense] == ["batch+res+drop-h32+dense+K3", "node+bias-h32+dense+K1"]
    everything = grid + dense + [c for h in W.WIDTHS_AXIS for c in W.width_axis_x(h)]
    for c in everything:                              # every configuration is one run() accepts
        kw = W.run_options(c)
        M._check_propagate(kw.get("propagate"), kw.get("ppr_alpha"), kw.get("dense_layers"), kw.get("aggr"), c["root"] or None)
        M._check_drop_edge(kw.get("drop_edge"), "sym", kw.get("aggr"), kw.get("dense_layers"))
        assert (kw.get("drop_edge") == DW.P_DROP) == (c["aggr"] == "drop") and (kw.get("aggr") == "max") == (c["aggr"] == "max")
    with pytest.raises(ValueError):                   # (and the checks do refuse: DropEdge with max, dense layers with a root weight)
        M._check_drop_edge(DW.P_DROP, "sym", "max", None)
    with pytest.raises(ValueError):
        M._check_propagate(3, 0.1, True, None, True)
    # a configuration with sum / None keeps GG's tag; every other tag is new
    assert W.tag(W.config("batch", 1, 0, 1, W.DROPOUT)) == GG.tag(GG.config("batch", 1, 0, 1, W.DROPOUT))
    assert sum(W.tag(c) == GG.tag(c) for c in everything) == 1
    sub = W.rank_subset_x()
    assert len(sub) <= 8 and {W.tag(c) for c in sub} <= {W.tag(c) for c in grid}
    assert any(c["aggr"] == "max" and c["residual"] for c in sub)
    assert any(c["aggr"] == "drop" and c["residual"] and c["dropout"] > 0 for c in sub)
    assert any(c["aggr"] == "max" and c["prop"] for c in sub) and any(c["aggr"] == "drop" and c["prop"] for c in sub)
    assert any(c["norm"] == "batch" and c["aggr"] != "sum" and (c["prop"] or c["residual"]) for c in sub)
    for h in W.WIDTHS_AXIS:
        assert [W.tag(c) for c in W.width_axis_x(h)] == ["node+res+drop-h%d+max" % h, "batch+root-h%d+dropedge+K3" % h,
                                                         "none+root+bias+res-h%d+K1" % h]
    # the device's worker groups are these lists, cut
    halves = W.one_rank_groups()
    assert sorted(map(W.tag, halves[0] + halves[1])) == sorted(map(W.tag, grid + dense)) and len(halves[0]) == len(halves[1]) == 8
    assert [W.tag(c) for _, g in W.width_groups() for c in g] == [W.tag(c) for h in W.WIDTHS_AXIS for c in W.width_axis_x(h)]
    # what may lack a weight seed is part of these lists, and none of it runs on 2 or 3 ranks
    tags = {W.tag(c) for c in everything}
    assert all(task in W.TASKS and t in tags for task, t in W.NO_SEED_X)
    assert not {t for _, t in W.NO_SEED_X} & {W.tag(c) for c in sub}


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (what, float(np.abs(a - b).max()))


def test_model64x_is_the_older_statements_where_they_meet(datasets):
    """One seed, one step.  sum / None: GG.model64 in double at the grid's four layers, loss, logits and every gradient bit for bit.
    The three options at three layers and the single task, where the older statements live, to 1e-12 relative: max under a given
    selection against AW.model_sel; propagate on plain GCN layers and on dense layers against PW.model64; DropEdge against
    DW.model64_drop in training and against GG.model64 in eval mode."""
    seed, step = 5, 1
    for task in W.TASKS:
        _, data = datasets[task]
        for c in (W.config(), W.config("batch", 1, 0, 1, W.DROPOUT), W.config("node", 0, 1, 1, W.DROPOUT), W.config("none", 1, 1, 1, 0.0)):
            widths = GG.widths_of(task, c)
            params = GG.initial_params(widths, c, seed)
            for training in (True, False):
                old = GG.model64(data, widths, params, dict(c, task=task), step, training)
                new = W.model64x(data, widths, params, dict(c, task=task), step, training)
                assert GG._same_bits(old[0].numpy(), new[0].numpy()) and GG._same_bits(old[1].numpy(), new[1].numpy()), (task, W.tag(c))
                assert sorted(old[2]) == sorted(new[2]) and all(GG._same_bits(old[2][k].numpy(), new[2][k].numpy()) for k in old[2])
                assert all(GG._same_bits(old[3][k].numpy(), new[3][k].numpy()) for k in old[3])
    _, data = datasets["single"]
    rng = np.random.default_rng(3)
    rowptr, col = AW.sym_pattern(data["A"])
    # max: a selection that is nobody's own (the winners of random features): the linearisation, not the definition, is compared
    for c in (AW.config("none", 1, 1, W.DROPOUT), AW.config("node"), AW.config("batch", 1, 0, W.DROPOUT)):
        widths = AW.widths_of(c)
        params = GG.initial_params(widths, c, seed)
        args = [AW.oracle_max(rowptr, col, np.arange(W.N), rng.random((W.N, f)))[1] for f in widths[:-1]]
        assert all((a >= 0).all() for a in args)
        l0, z0, g0 = AW.model_sel(data, widths, params, dict(c, task="single"), step, args)
        l1, z1, g1, _ = W.model64x(data, widths, params, dict(c, task="single", aggr="max", prop=None, dense=False), step, args=args)
        _close(l1, l0, "max loss"), _close(z1, z0, "max logits")
        for k in g0:
            _close(g1[k], g0[k], "max grad " + k)
    # max with args=None (what the seed rule runs): the definition's own selection on the first layer's input, the features, is
    # AW.oracle_max's -- a one-layer model under that explicit selection is the same model bit for bit
    c = W.config("none", 1, 1, aggr="max")
    params = GG.initial_params([GG.FIN, GG.CLASSES], c, seed)
    first = [AW.oracle_max(rowptr, col, np.arange(W.N), data["X"].astype(np.float64))[1]]
    own = W.model64x(data, [GG.FIN, GG.CLASSES], params, dict(c, task="single"), step)
    sel = W.model64x(data, [GG.FIN, GG.CLASSES], params, dict(c, task="single"), step, args=first)
    assert GG._same_bits(own[1].numpy(), sel[1].numpy()) and all(GG._same_bits(own[2][k].numpy(), sel[2][k].numpy()) for k in own[2])
    assert float((own[1] - W.model64x(data, [GG.FIN, GG.CLASSES], params, dict(c, task="single", aggr="sum"), step)[1]).abs().max()) > 1e-3
    # propagate
    for c in PW.model_configs() + [PW.config(False, K=1, alpha=0.1)]:
        widths = PW.widths_of(c)
        params = GG.initial_params(widths, c, seed)
        l0, z0, g0 = PW.model64(data, widths, params, c, step)
        mine = dict(c, task="single", aggr="sum", prop=(c["K"], c["alpha"]))
        l1, z1, g1, _ = W.model64x(data, widths, params, mine, step)
        _close(l1, l0, "prop loss"), _close(z1, z0, "prop logits")
        for k in g0:
            _close(g1[k], g0[k], "prop grad " + k)
        assert float((z1 - W.model64x(data, widths, params, dict(mine, prop=None), step)[1]).abs().max()) > 1e-3
    # DropEdge
    for c in (DW.config(), DW.config("node", 1, 1, W.DROPOUT), DW.config("batch", 1, 0, 0.0)):
        widths = DW.widths_of(c)
        params = GG.initial_params(widths, c, seed)
        opts = dict(c, task="single")
        mine = dict(opts, aggr="drop", prop=None, dense=False)
        l0, z0, g0, b0 = DW.model64_drop(data, widths, params, opts, step, torch.float64)
        l1, z1, g1, b1 = W.model64x(data, widths, params, mine, step)
        _close(l1, l0, "drop loss"), _close(z1, z0, "drop logits")
        for k in g0:
            _close(g1[k], g0[k], "drop grad " + k)
        for k in b0:
            _close(b1[k], b0[k], "drop buffer " + k)
        e0 = GG.model64(data, widths, params, opts, step, False, torch.float64, b0)
        e1 = W.model64x(data, widths, params, mine, step, False, torch.float64, b0)
        _close(e1[0], e0[0], "drop eval loss"), _close(e1[1], e0[1], "drop eval logits")
        assert float((z1 - e1[1]).abs().max()) > 1e-3                              # (the mask changes the training logits)


@pytest.mark.parametrize("task", W.TASKS)
def test_option_grid_on_one_rank(datasets, task):
    assert W.run_group_x(datasets, task, W.option_grid() + W.dense_configs(), 1, False) > 16 * 2 * 6


@pytest.mark.parametrize("hidden", W.WIDTHS_AXIS)
def test_width_axis(datasets, hidden):
    W.run_group_x(datasets, "single", W.width_axis_x(hidden), 1, False)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("task", W.TASKS)
def test_ranks_hold_the_reduced_gradient(datasets, task, P):
    """The rank subset on 2 and 3 ranks under the seeded random part vectors: the gradient after the all-reduce is held to the same
    bound on every rank; with three ranks a row receives candidates (max) and partial sums from two peers."""
    W.run_group_x(datasets, task, W.rank_subset_x(), P, False)
