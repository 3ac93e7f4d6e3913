"""Every layer option on a rank that owns nothing, a rank whose rows are in no set and a rank of one row -- on the device: the
groups of tests/test_degenerate.py on the real kernels, the ranks sharing one GPU over gloo as in tests/test_gradgrid_gpu.py.  What is
held, and to what, is that file's docstring; on two ranks the PGCN groups run with tuning.wgrad_lane 0 and 1 and ask for the same
bits (the newer-option groups run lane 0: _degenerate_workers.newer_group has the measured reason).  Here the kernels' wrappers are
held: zero-row tensors whose data_ptr() is 0 and whose strides are arbitrary, work-spaces sized for no rows, the one-row leading
dimension, max and DropEdge structures without a stored entry."""
import pytest

import _degenerate_workers as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.GG.make_datasets(str(tmp_path_factory.mktemp("degenerate_gpu")))


@pytest.fixture(scope="module")
def gat_datasets(tmp_path_factory):
    return W.GT.make_datasets(str(tmp_path_factory.mktemp("degenerate_gat_gpu")))


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    return str(tmp_path_factory.mktemp("degenerate_vectors_gpu"))


@pytest.mark.parametrize("vector,task", W.cases("pgcn"))
def test_pgcn_options(datasets, vectors, vector, task):
    assert W.pgcn_group(datasets, vectors, vector, task, True) > 4 * 2 * 2


@pytest.mark.parametrize("vector,task,half", W.newer_cases())
def test_newer_options(datasets, vectors, vector, task, half):
    assert W.newer_group(datasets, vectors, vector, task, True, half) > 3 * 2 * 2


@pytest.mark.parametrize("vector,task", W.cases("gat"))
def test_gat_options(gat_datasets, vectors, vector, task):
    assert W.gat_group(gat_datasets, vectors, vector, task, True) > 8 * 2 * 2
