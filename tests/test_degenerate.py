"""Every layer option on a rank that owns nothing, a rank whose rows are in no set and a rank of one row -- the CPU side: PGCN.run and
the GAT classifier on the checker-backed kernels over gloo under the four part vectors of tests/_degenerate_workers.py (E2, E3: an
empty rank, on three ranks the reporting one; S2: 37 rows, none labelled; O2: one train row), against the float64 models of the
balanced tests through their own runners: the loss summed over the ranks, both steps' training logits, every parameter's gradient
after the all-reduce on EVERY rank, the batch-norm buffers and the eval logits, each through conftest.held_to_fixture with the float32
twin as the fixture -- no new tolerance, no element excused.  Here the wiring is held: zero-row tensors through the autograd nodes,
the masked losses' global divisor, batch norm's column sums from a rank without rows, empty exchange rounds;
tests/test_degenerate_gpu.py runs the same groups on the kernels (14, two of them as two worker groups each:
_degenerate_workers.newer_cases)."""
import pytest
import torch

import _degenerate_workers as W
from conftest import pkg


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.GG.make_datasets(str(tmp_path_factory.mktemp("degenerate")))


@pytest.fixture(scope="module")
def gat_datasets(tmp_path_factory):
    return W.GT.make_datasets(str(tmp_path_factory.mktemp("degenerate_gat")))


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    return str(tmp_path_factory.mktemp("degenerate_vectors"))


def test_the_lists_and_the_vectors(datasets):
    assert len(W.cases("pgcn")) + len(W.cases("newer")) + len(W.cases("gat")) == 14
    assert len(W.newer_cases()) == len(W.cases("newer")) + 2 and {v for v, _, _ in W.newer_cases()} == set(W.VECTORS)
    assert W.newer_configs(0) + W.newer_configs(1) == W.newer_configs()
    assert [W.GG.tag(c) for c in W.pgcn_configs()] == ["none+res+drop-h32", "none+drop-h30", "batch+root+drop-h30", "node+res+drop-h30"]
    assert len(W.newer_configs()) == 6 and {c["aggr"] for c in W.newer_configs()} == {"max", "drop"}
    assert {c["prop"] for c in W.newer_configs()} == set(W.OX.PROPS)
    assert len({W.GT.tag(o) for o in W.gat_configs("single")}) == 8
    for task in W.GG.TASKS:
        data = datasets[task][1]
        for name, (P, who) in W.VECTORS.items():
            pv = W.part_vector(name, data)
            W.check_vector(name, [(pv == r).nonzero()[0] for r in range(P)], data)


def test_unpack_sign_mask_of_no_rows():
    M = pkg("PGCN")
    out = M.unpack_sign_mask(torch.zeros((0, 2), dtype=torch.int32), 44)
    assert out.dtype is torch.bool and out.shape == (0, 44)
    words = torch.tensor([[5, -1], [-2 ** 31, 1 << 11]], dtype=torch.int32)
    want = torch.zeros((2, 44), dtype=torch.bool)
    want[0, [0, 2]] = True
    want[0, 32:] = True
    want[1, [31, 43]] = True
    assert torch.equal(M.unpack_sign_mask(words, 44), want)
    assert torch.equal(M.unpack_sign_mask(words, 64)[:, :44], want) and M.unpack_sign_mask(words, 64).shape == (2, 64)


def test_the_dropout_fallback_on_an_empty_rank(datasets, vectors):
    """The plain layer with dropout on two ranks of which one owns nothing: its backward unpacks a sign mask of no rows."""
    W.pgcn_group(datasets, vectors, "E2", "single", False, configs=W.pgcn_configs()[:1])


@pytest.mark.parametrize("vector,task", W.cases("pgcn"))
def test_pgcn_options(datasets, vectors, vector, task):
    assert W.pgcn_group(datasets, vectors, vector, task, False) > 4 * 2 * 2


@pytest.mark.parametrize("vector,task,half", W.newer_cases())
def test_newer_options(datasets, vectors, vector, task, half):
    assert W.newer_group(datasets, vectors, vector, task, False, half) > 3 * 2 * 2


@pytest.mark.parametrize("vector,task", W.cases("gat"))
def test_gat_options(gat_datasets, vectors, vector, task):
    assert W.gat_group(gat_datasets, vectors, vector, task, False) > 8 * 2 * 2
