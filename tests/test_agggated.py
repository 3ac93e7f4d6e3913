"""Gated aggregation without a GPU: the composed routes of engine.py against the float64 definition of tests/_agggated_workers.py
within its bound, the engine at 1, 2 and 3 ranks on karate and gemat11 under their committed part vectors, the whole model against
float64 autograd of the plain formulation with the checkpoint round trip, the refusals and the command line."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import pkg

import _agggated_workers as W
from _agggated_workers import ENGINE_F as F


@pytest.mark.parametrize("split", [False, True])
def test_composed_routes_are_the_definition(split, monkeypatch):
    """All four on column slices of one 3 f wide product, row blocks of 64; ``split``: two column-disjoint structures joined by accumulation."""
    E, case = pkg("engine"), W.make_case(F)
    monkeypatch.setattr(E, "GATED_BLOCK_ROWS", 64)
    cpu, gid = torch.device("cpu"), torch.from_numpy(case["gid"])
    fwd = [E.composed_max_csr(W.host_csr(m), gid, cpu) for m in (case["halves"] if split else [case["M"]])]
    AT = E.composed_max_csr(W.host_csr(case["MT"]), None, cpu)
    Y, G = (torch.from_numpy(a) for a in W.operands(case, F))
    K, QV = Y[:, :F], Y[:, F:]
    Z, DEN, dY = torch.full((W.N, F), 77.0), torch.full((W.N, F), 77.0), torch.full((W.N, 3 * F), 77.0)
    for k, A in enumerate(fwd):
        E.agggated_composed(A, K, QV, Z, DEN, accumulate=k > 0)
    panel = E.agggated_finish_composed(E.agggated_finish_composed(Z, DEN), DEN, G, K)
    for k, A in enumerate(fwd):
        E.agggated_grad_rows_composed(A, panel, QV, dY[:, :F], accumulate=k > 0)
    E.agggated_grad_cols_composed(AT, QV, panel, dY[:, F:])
    W.check_all(case, F, Z.numpy(), DEN.numpy(), dY[:, :F].numpy(), dY[:, F:].numpy(), ("composed", split))


def test_refusals_the_checkpoint_record_and_the_command_line():
    P, C, drop = pkg("PGCN"), pkg("checkpoint"), pkg("dropout")
    assert P.ALL_AGGRS == ("sum", "max", "pna", "gated")
    for kw, word in ((dict(aggregate=False), "aggregate=False"), (dict(softmax_beta=1.0), "softmax_beta"),
                     (dict(drop_edge=drop.EdgeDrop(0.5, drop.DropoutState(1, torch.device("cpu")))), "drop_edge")):
        with pytest.raises(ValueError, match='aggr="gated" does not go with %s' % word):
            P.PGCN(None, 4, 4, aggr="gated", **kw)
    with pytest.raises(ValueError, match='operand="bf16" does not go with aggr="gated"'):
        P.PGCN(None, 4, 4, aggr="gated", operand="bf16")
    layer = P.PGCN(None, 4, 6, aggr="gated", root_weight=True, bias=True)
    assert tuple(layer.linear.weight.shape) == (18, 4) and tuple(layer.root.weight.shape) == (6, 4) and layer.linear.bias is None
    for check, kw in ((P._check_softmax_beta, dict(softmax_beta=1.0)), (P._check_drop_edge, dict(drop_edge=0.5, normalize="sym")),
                      (P._check_propagate, dict(propagate=None, ppr_alpha=None, dense_layers=True))):
        with pytest.raises(ValueError, match='aggr="gated"'):
            check(aggr="gated", **kw)
    arch = C.architecture([8, 16, 4], "single", aggr="gated")
    assert arch["aggr"] == "gated" and P._architecture(8, 4, 2, 16, None, False, 0.0, 0, None, False, False, False, aggr="gated") == arch
    g = lambda name: os.path.join(W.GOLDEN, name)
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(W.HERE), "PGCN.py"), "-a", g("karate.mtx"), "-p", g("karate.mtx.1.rp"),
                          "-b", "gloo", "-s", "1", "-l", "2", "-f", "16", "--aggr", "gated"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "need them" in out.stdout, (out.returncode, out.stdout[-500:], out.stderr[-500:])


@pytest.mark.parametrize("name", ["karate", "gemat11"])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_engine_under_the_committed_part_vectors(name, P):
    res = W.AW._spawn(W.engine_worker, P, W.graph_paths(name, P), False)
    assert all(r["composed"] for r in res)
    W.check_engine(res, name, P)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.AW.make_dataset(str(tmp_path_factory.mktemp("agggated")))


@pytest.mark.parametrize("P", [1, 2, "E2", "O2"])
def test_model_against_float64_autograd(dataset, tmp_path, P):
    """run(aggr="gated", root_weight, bias, norm="node", residual), lr = 0: 1, 2 ranks with the round trip; a rank of no rows (E2), one row (O2)."""
    import _degenerate_workers as DG
    paths, data = dataset
    if isinstance(P, str):
        res = W.AW._spawn(W.model_worker, DG.VECTORS[P][0], DG.with_vector(paths, P, data, str(tmp_path), "gated"), False)
        DG.check_vector(P, [r["results"][0]["own"] for r in res], data)
    else:
        res = W.AW._spawn(W.model_worker, P, paths, False, scratch=str(tmp_path))
        assert all("reloaded" in r["results"][0] for r in res)
    assert W.check_model(data, res, "agggated/model/%s" % P)[0]
