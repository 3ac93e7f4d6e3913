"""Every layer option on a rank that owns nothing, a rank whose rows are in no set and a rank of one row -- on the device: the
groups of tests/test_degenerate.py on the real kernels, the ranks sharing one GPU over gloo as in tests/test_gradgrid_gpu.py.  What is
held, and to what, is that file's docstring; on two ranks the PGCN groups run with tuning.wgrad_lane 0 and 1 and ask for the same
bits (the newer-option groups run lane 0: _degenerate_workers.newer_group has the measured reason).  Here the kernels' wrappers are
held: zero-row tensors whose data_ptr() is 0 and whose strides are arbitrary, work-spaces sized for no rows, the one-row leading
dimension, max and DropEdge structures without a stored entry.

The options merged since run under every vector as well (_degenerate_workers.OPTION_GROUPS, 20 groups): every answer comes from
HipKernels, and every rank -- the one without rows too -- reports the kernels' route: gpr_workspace(0, f, K) and the finishing launch
over no records, score planes and the da work-space of a structure without entries, a permutation of length 0.

No group may take longer than the balanced test_gradgrid_gpu.test_ranks_hold_the_reduced_gradient[single-2-lanes0] of the same
session; HISTORY.md section 39 has the measured lines."""
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
def softmax_dataset(tmp_path_factory):
    return W.SM.make_dataset(str(tmp_path_factory.mktemp("degenerate_softmax_gpu")))


@pytest.fixture(scope="module")
def gpr_dataset(tmp_path_factory):
    return W.GP.make_dataset(str(tmp_path_factory.mktemp("degenerate_gpr_gpu")))


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


@pytest.mark.parametrize("vector,task", W.option_cases("softmax"))
def test_softmax_aggregation(softmax_dataset, vectors, vector, task):
    assert W.softmax_group(softmax_dataset, vectors, vector, True) > 4 * 2 * 2


@pytest.mark.parametrize("vector,task", W.option_cases("gpr"))
def test_gpr(gpr_dataset, vectors, vector, task):
    assert W.gpr_group(gpr_dataset, vectors, vector, True) > 2 * 2 * 2


@pytest.mark.parametrize("vector,task", W.option_cases("attndrop"))
def test_attention_dropout(gat_datasets, vectors, vector, task):
    assert W.attention_group("attndrop", gat_datasets, vectors, vector, task, True) > 2 * 2 * 2


@pytest.mark.parametrize("vector,task", W.option_cases("gatv2"))
def test_gatv2(gat_datasets, vectors, vector, task):
    assert W.attention_group("gatv2", gat_datasets, vectors, vector, task, True) > 2 * 2 * 2


@pytest.mark.parametrize("vector,task", W.option_cases("gatdot"))
def test_dot_product_attention(gat_datasets, vectors, vector, task):
    assert W.attention_group("gatdot", gat_datasets, vectors, vector, task, True) > 2 * 2
