"""Gated aggregation on the MI355X: the four kernels of csrc/pgcn_agggated.hip against the float64 definition of
tests/_agggated_workers.py (its docstring derives the bound), the engine at 2 and 3 ranks, and the whole model on cora, real kernels.

f = 4: one vector; 7: the scalar body (leading dimension 21, unaligned slices); 64: one full pass; 72: a ragged second pass; 128: two
passes.  Every operand is a column slice of a 3 f wide product or gradient.  Plans: unsliced, XCD-sliced, sliced with 64-feature passes."""
import numpy as np
import pytest
import torch

from conftest import pkg

import _agggated_workers as W

pytestmark = pytest.mark.gpu

WIDTHS = (4, 7, 64, 72, 128)
PLANS = ("unsliced", "sliced", "sliced+fpass64")


@pytest.fixture(scope="module")
def case():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    c = W.make_case(max(WIDTHS))
    K, K64 = pkg("kernels").HipKernels(dev), pkg("kernels").HipKernels(dev)
    K64.base_flags |= pkg("_lib").SPMM_FPASS64
    gid = torch.from_numpy(c["gid"])
    c["plans"] = {}
    for name, Kv, S in zip(PLANS, (K, K, K64), (1, 8, 8)):
        p = dict(K=Kv, A=Kv.prepare_max(W.host_csr(c["M"]), gid, chunk=W.CHUNK, nslices=S),
                 halves=[Kv.prepare_max(W.host_csr(h), gid, chunk=W.CHUNK, nslices=S) for h in c["halves"]],
                 AT=Kv.prepare_max(W.host_csr(c["MT"]), None, chunk=W.CHUNK, nslices=S))
        assert p["A"].nslots > 3 and p["AT"].nslots > 1 and p["A"].nslices == S            # cut rows, both ways
        c["plans"][name] = p
    return c


def _run(p, case, f, structures=None, shifted=False):
    """(Z1, DEN, dK, dQV) through the four kernels.  ``shifted``: every operand starts 4 bytes into its allocation: the scalar body."""
    def place(a):
        t = torch.from_numpy(a).cuda()
        if shifted:
            t = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)[1:1 + t.numel()].view(t.shape).copy_(t)
            assert t.data_ptr() % 16 == 4
        return t
    Kv, fill = p["K"], lambda w: place(np.full((W.N, w), 77, np.float32))       # (a launch that does not accumulate ignores what the outputs hold)
    Y, G = (place(a) for a in W.operands(case, f))
    K, QV, Z, DEN, dY = Y[:, :f], Y[:, f:], fill(f), fill(f), fill(3 * f)
    structures = structures or [p["A"]]
    for k, A in enumerate(structures):
        Kv.agggated(A, K, QV, Z, DEN, accumulate=k > 0)
    panel = Kv.agggated_finish(Kv.agggated_finish(Z, DEN), DEN, G, K)
    for k, A in enumerate(structures):
        Kv.agggated_grad_rows(A, panel, QV, dY[:, :f], accumulate=k > 0)
    Kv.agggated_grad_cols(p["AT"], QV, panel, dY[:, f:])
    return [t.cpu().numpy() for t in (Z, DEN, dY[:, :f], dY[:, f:])]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("f", WIDTHS)
def test_kernels_are_the_definition(case, f, plan):
    """All four within the bound (error / bound is printed); a second call gives the same bits, at f = 64 from the scalar body; at f = 7 and
    72 also the column-disjoint halves joined by PGCN_SPMM_ACCUMULATE against the definition over their union."""
    p = case["plans"][plan]
    first = _run(p, case, f)
    W.check_all(case, f, *first, (plan, f))
    assert all(np.array_equal(W.AW.bits(a), W.AW.bits(b)) for a, b in zip(first, _run(p, case, f, shifted=f == 64)))
    if f in (7, 72):
        W.check_all(case, f, *_run(p, case, f, structures=p["halves"]), (plan, f, "halves"))


@pytest.mark.parametrize("name,P", [("karate", 3), ("gemat11", 2)])
def test_engine_on_ranks_that_share_the_device(name, P):
    """The halo structures, the strided gather of the boundary rows and the unpack into the [dQ | dV] slice on the real kernels."""
    res = W.AW._spawn(W.engine_worker, P, W.graph_paths(name, P), True)
    assert all(not r["composed"] and r["hip"] == "HipKernels" for r in res)
    W.check_engine(res, name, P)


def test_model_on_cora_against_float64_autograd(tmp_path):
    """run(aggr="gated", root_weight, bias, norm="node", residual), lr = 0, one rank, --hidden 64: loss, logits, gradients against float64."""
    import _propagate_workers as PP
    from scipy.io import mmread
    paths = PP.make_cora(str(tmp_path))
    data = dict(A=mmread(paths["A"]).tocsr(), X=np.load(paths["features"]), labels=np.load(paths["labels"]), split=np.load(paths["split"]))
    assert W.check_model(data, W.AW._spawn(W.model_worker, 1, paths, True, hidden=64), "agggated/model/gpu") == (False, {"HipKernels"})
