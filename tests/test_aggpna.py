"""PNA layers without a GPU: the composed route (engine.aggpna_composed / aggpna_finish_composed / aggpna_backward_composed) against
the float64 definition of tests/_aggpna_workers.py within its derived bounds, the order-free outputs under a split, delta and the
scalers under 1, 2 and 3 ranks, the layer's refusals, the checkpoint record, and the whole model against the double model."""
import numpy as np
import pytest
import torch

from conftest import pkg

import _aggpna_workers as W

F = 12
FAMILIES = ("uniform", "relu", "equal", "offset")


@pytest.fixture(scope="module")
def case():
    E = pkg("engine")
    c = W.make_pattern(F)
    cpu = torch.device("cpu")
    gid = torch.from_numpy(c["gid"])
    c["A"] = E.composed_max_csr(W.host_csr(c["M"]), gid, cpu)
    c["A_halves"] = [E.composed_max_csr(W.host_csr(h), gid, cpu) for h in c["halves"]]
    c["AT"] = E.composed_max_csr(W.host_csr(c["MT"]), None, cpu)
    return c


def _forward(E, structures, B, deg, priors=()):
    n, f = structures[0].nrows, B.shape[1]
    S, AMAX, AMIN = torch.full((n, 4 * f), 77.0), torch.full((n, f), 77, dtype=torch.int32), torch.full((n, f), 77, dtype=torch.int32)
    E.aggpna_composed(structures[0], B, S, AMAX, AMIN)
    for A, prior in zip(structures[1:], priors):
        E.aggpna_composed(A, B, S, AMAX, AMIN, prior, accumulate=True)
    E.aggpna_finish_composed(S, deg)
    return S.numpy(), AMAX.numpy(), AMIN.numpy()


@pytest.mark.parametrize("fam", FAMILIES)
def test_composed_route_is_the_definition(case, fam):
    """Forward and backward in fp32 inside every bound on every family: what the GPU tests then ask of the kernels.  ``equal`` gives
    STD = sqrt(1e-5f) exactly; ``offset`` is the family a difference of squares fails."""
    E = pkg("engine")
    o = case["want"][fam]
    deg = torch.from_numpy(o["d"].astype(np.int32))
    B = torch.from_numpy(case["H"][fam])
    S, AMAX, AMIN = _forward(E, [case["A"]], B, deg)
    W.assert_forward(S, AMAX, AMIN, o, ("composed", fam))
    if fam == "equal":
        assert (S[o["d"] > 0, 3 * F:] == np.sqrt(np.float32(1e-5) + np.float32(0))).all()
    dS = np.ascontiguousarray(case["dS"].reshape(W.NROWS, 4 * F))
    panel = E.aggpna_finish_composed(torch.from_numpy(S), deg, torch.from_numpy(dS), torch.from_numpy(AMAX), torch.from_numpy(AMIN))
    D = torch.full((W.NCOLS, F), 77.0)
    E.aggpna_backward_composed(case["AT"], torch.from_numpy(case["gid"].astype(np.int32)), B, panel, D)
    cnt = W.assert_backward(D.numpy(), case["rowptr"], case["col"], case["gid"], case["H"][fam], dS, S, AMAX, AMIN, ("composed", fam))
    assert cnt.max() >= 1000


@pytest.mark.parametrize("fam", ("relu", "offset"))
def test_halves_accumulated_give_the_order_free_bits(case, fam):
    E = pkg("engine")
    o = case["want"][fam]
    deg = torch.from_numpy(o["d"].astype(np.int32))
    B = torch.from_numpy(case["H"][fam])
    whole = _forward(E, [case["A"]], B, deg)
    for order in ((0, 1), (1, 0)):
        structures = [case["A_halves"][k] for k in order]
        prior = torch.from_numpy(np.diff(case["halves"][order[0]].indptr).astype(np.int32))
        S, AMAX, AMIN = _forward(E, structures, B, deg, [prior])
        assert np.array_equal(AMAX, whole[1]) and np.array_equal(AMIN, whole[2])
        assert np.array_equal(W.bits(S[:, F:3 * F]), W.bits(whole[0][:, F:3 * F]))
        W.assert_forward(S, AMAX, AMIN, o, ("halves", fam))


def test_refusals_and_the_checkpoint_record():
    P, C = pkg("PGCN"), pkg("checkpoint")
    drop = pkg("dropout")
    for kw, word in ((dict(aggregate=False), "aggregate=False"), (dict(softmax_beta=1.0), "softmax_beta"),
                     (dict(drop_edge=drop.EdgeDrop(0.5, drop.DropoutState(1, torch.device("cpu")))), "drop_edge")):
        with pytest.raises(ValueError, match='aggr="pna" does not go with %s' % word):
            P.PGCN(None, 4, 4, aggr="pna", **kw)
    layer = P.PGCN(None, 4, 6, aggr="pna", root_weight=True)
    assert tuple(layer.linear.weight.shape) == (6, 48) and tuple(layer.root.weight.shape) == (6, 4)
    for check, kw in ((P._check_softmax_beta, dict(softmax_beta=1.0, aggr="pna")), (P._check_drop_edge, dict(drop_edge=0.5, normalize="sym", aggr="pna")),
                      (P._check_propagate, dict(propagate=None, ppr_alpha=None, dense_layers=True, aggr="pna"))):
        with pytest.raises(ValueError, match='aggr="pna"'):
            check(**kw)
    arch = C.architecture([8, 16, 4], "single", aggr="pna")
    assert arch["aggr"] == "pna" and arch != C.architecture([8, 16, 4], "single", aggr="max")
    assert "aggr" not in C.architecture([8, 16, 4], "single", aggr="sum") and C.architecture([8, 16, 4], "single", aggr="max")["aggr"] == "max"
    assert P._architecture(8, 4, 2, 16, None, False, 0.0, 0, None, False, False, False, aggr="pna") == arch
    assert pkg("engine").pna_delta([0, 3]) == np.log(2.0) and pkg("engine").pna_delta([5]) == 0.0


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggpna")))


def test_engine_delta_and_scalers_under_any_partition(dataset):
    """forward_pna / backward_pna on the composed route against the oracle; delta and the scalers are the same BITS under 1, 2 and 3
    ranks and both part vectors."""
    paths, data = dataset
    seen = []
    for P, pv in ((1, "pv"), (2, "pv"), (2, "cpv"), (3, "pv")):
        res = W.AW._spawn(W.engine_worker, P, paths, False, partvec=pv)
        assert all(r["composed"] for r in res)
        seen.append(W.check_engine(res, data, P))
    assert all(s[0] == seen[0][0] and np.array_equal(W.bits(s[1]), W.bits(seen[0][1])) and np.array_equal(W.bits(s[2]), W.bits(seen[0][2]))
               for s in seen)


def test_model_against_the_double_model_and_the_checkpoint_round_trip(dataset, tmp_path):
    """Every configuration at 1 and 2 ranks against the float64 model; the last one is saved, loaded with epochs=0 and predicted from;
    the loss lines the two rank counts print are the same text."""
    paths, data = dataset
    printed = []
    for P in (1, 2):
        res = W.AW._spawn(W.model_worker, P, paths, False, scratch=str(tmp_path))
        assert all(r["composed"] for rank in res for r in rank["results"])
        assert W.check_models(data, res) > 0
        printed.append([r["losses"] for r in res[0]["results"]])
    assert printed[0] == printed[1] and all(len(lines) > 0 for lines in printed[0]), printed


@pytest.mark.parametrize("name", ["E2", "E3", "O2"])
def test_ranks_without_rows_and_of_one_row(dataset, tmp_path, name):
    """A rank that owns nothing (E2: of two, E3: of three) or one row (O2) goes through pna_degrees, forward_pna, backward_pna, the
    scalers and the model: the same oracle, the same delta."""
    W.degenerate_group(dataset, str(tmp_path), name, False)
