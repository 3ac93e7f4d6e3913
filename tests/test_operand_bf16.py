"""bf16 operands of the aggregation without a GPU: the composed route against the definition AH = A . bf16(H), dH = A^T . bf16(G), the
option on PGCN / run / the command line (values, refusals, fp32 = the model of before call for call), checkpoints across operand
types and a 2-rank gloo run.  The kernels of csrc/pgcn_bf16.hip: tests/test_operand_bf16_gpu.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _nodeclass_workers as NW
import _operand_bf16_workers as W
from conftest import gpath, pkg, read_partvec
from oracle_kernels import OracleKernels


class RecordingKernels(OracleKernels):
    def __init__(self):
        self.calls = []

    def spmm(self, A, B, C, accumulate=False):
        self.calls.append(("spmm", tuple(B.shape), bool(accumulate)))
        return super().spmm(A, B, C, accumulate)


def _engine(K=None):
    Pm, I, E = pkg("partition"), pkg("ingest"), pkg("engine")
    A = I.mmread(gpath("karate.mtx")).tocoo()
    n = A.shape[0]
    part = Pm.build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                              torch.from_numpy(A.data.astype(np.float32)), n, torch.zeros(n, dtype=torch.int64), 0, 1)
    return E.AggregationEngine(part, K or OracleKernels(), torch.device("cpu")), sp.csr_matrix(A), n


def test_composed_route_is_the_definition_bit_for_bit():
    M = pkg("PGCN")
    eng, A, n = _engine()
    rng = np.random.default_rng(3)
    H = torch.from_numpy(rng.standard_normal((n, 7)).astype(np.float32)).requires_grad_(True)
    G = torch.from_numpy(rng.standard_normal((n, 7)).astype(np.float32))
    assert not torch.equal(H.detach().to(torch.bfloat16).float(), H.detach())
    out = M.PSpMMBf16.apply(eng, H)
    out.backward(G)
    assert eng._bf16.composed
    rounded = lambda x: x.detach().to(torch.bfloat16).to(torch.float32)
    assert torch.equal(out.detach().view(torch.int32), eng.forward(rounded(H)).view(torch.int32))
    assert torch.equal(H.grad.view(torch.int32), eng.backward(rounded(G)).view(torch.int32))
    own = eng.part.owned.numpy()                   # local row i is global row own[i]
    for got, mat, x in ((out.detach(), A, H.detach()), (H.grad, A.T, G)):
        full = np.zeros((n, 7), np.float32)
        full[own] = x.numpy()
        want, bound = W.definition64(mat, full)
        assert (np.abs(got.numpy().astype(np.float64) - want[own]) <= bound[own]).all()


CONFLICTS = [(dict(aggr="max"), "aggr"), (dict(aggr="pna"), "aggr"), (dict(softmax_beta=1.0), "softmax_beta"),
             (dict(drop_edge=0.5), "drop_edge"), (dict(propagate=2), "propagate"), (dict(gpr=2), "gpr")]


@pytest.mark.parametrize("kw,name", CONFLICTS)
def test_conflicts_are_refused_naming_both_options(kw, name, tmp_path, monkeypatch, capsys):
    M, D = pkg("PGCN"), pkg("dropout")
    files = dict(features="f.npy", labels="l.npy", split="s.npy")
    with pytest.raises(ValueError, match="operand.*%s" % name):
        M.run(0, 1, 2, 4, "A.mtx", "A.pv", "gloo", normalize="sym", operand="bf16", **files, **kw)
    if name not in ("propagate", "gpr"):           # (a layer option)
        eng, _, _ = _engine()
        if name == "drop_edge":
            kw = dict(drop_edge=D.EdgeDrop(0.5, D.DropoutState(0, torch.device("cpu"))))
        with pytest.raises(ValueError, match="operand.*%s" % name):
            M.PGCN(eng, 4, 4, operand="bf16", **kw)
    argv = ["-a", "A.mtx", "-p", "A.pv", "--normalize", "sym", "--operand", "bf16"]
    for k in files:
        (tmp_path / files[k]).write_bytes(b"")
        argv += ["--" + k, str(tmp_path / files[k])]
    flag = {"softmax_beta": "softmax-aggr"}.get(name, name.replace("_", "-"))
    with pytest.raises(SystemExit) as e:
        M.main(argv + ["--" + flag, str(next(iter(kw.values()))) if name != "drop_edge" else "0.5"])
    assert e.value.code == 2
    msg = capsys.readouterr().out
    assert "--operand bf16" in msg and "--" + flag in msg


def test_values(monkeypatch, capsys):
    M = pkg("PGCN")
    assert M.OPERANDS == ("fp32", "bf16")
    eng, _, _ = _engine()
    for bad in ("int8", "bfloat16", 16):
        with pytest.raises(ValueError, match="operand takes fp32 \\| bf16"):
            M.PGCN(eng, 4, 4, operand=bad)
        with pytest.raises(ValueError, match="operand takes fp32 \\| bf16"):
            M.run(0, 1, 2, 4, "A.mtx", "A.pv", "gloo", operand=bad)
    with pytest.raises(SystemExit) as e:
        M.main(["-a", "A.mtx", "-p", "A.pv", "--operand", "int8"])
    assert e.value.code == 2 and "--operand takes fp32|bf16" in capsys.readouterr().out
    assert M.PGCN(eng, 4, 4, operand="bf16")._aggregate == M.PSpMMBf16.apply
    assert M.PGCN(eng, 4, 4, operand="fp32")._aggregate == M.PGCN(eng, 4, 4)._aggregate == M.PSpMM.apply
    started = []

    class Process:                                 # the command line hands the option on by name, only when it is bf16
        exitcode = 0

        def __init__(self, target, args, kwargs=None):
            started.append(kwargs)

        def start(self):
            pass

        def join(self):
            pass

    monkeypatch.setattr(M.mp, "Process", Process)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.setenv(k, "0")
    for value in ("bf16", "fp32"):
        M.main(["-a", "A.mtx", "-p", "A.pv", "--operand", value])
    assert started == [{"operand": "bf16"}, None]


def test_fp32_makes_the_calls_of_a_model_without_the_option():
    M = pkg("PGCN")
    logs = []
    for kw in ({}, {"operand": "fp32"}, {"operand": "bf16"}):
        K = RecordingKernels()
        eng, _, n = _engine(K)
        torch.manual_seed(0)
        model = torch.nn.Sequential(M.PGCN(eng, 5, 6, bias=True, **kw), M.PGCN(eng, 6, 3, relu=False, **kw))
        H = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 5)).astype(np.float32))
        for _ in range(2):
            model(H).sum().backward()
        logs.append((K.calls, [p.grad.clone() for p in model.parameters()], eng._bf16))
    assert logs[0][0] == logs[1][0] and all(torch.equal(a, b) for a, b in zip(logs[0][1], logs[1][1])) and logs[1][2] is None
    assert logs[2][2] is not None and not all(torch.equal(a, b) for a, b in zip(logs[0][1], logs[2][1]))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return NW.make_dataset(str(tmp_path_factory.mktemp("operand_bf16")))


def test_ranks_over_gloo_and_checkpoints_across_operand_types(dataset, tmp_path):
    paths, _ = dataset
    one, two = (W.spawn(W.run_worker, P, False, paths, operand="bf16")[0] for P in (1, 2))
    assert one["aggregate"] == ["PSpMMBf16"] * NW.NLAYERS
    assert len(one["history"]) == len(two["history"]) == NW.EPOCHS
    for a, b in zip(one["history"], two["history"]):
        assert abs(a["loss"] - b["loss"]) <= 1e-5 * abs(a["loss"])          # the bound of tests/test_nodeclass.py
    plain = W.spawn(W.run_worker, 1, False, paths)[0]
    assert plain["aggregate"] == ["PSpMM"] * NW.NLAYERS and plain["history"][0]["loss"] != one["history"][0]["loss"]
    # a checkpoint written under one operand type resumes under the other: the option is no architecture field
    M = pkg("PGCN")
    for first, then in (("bf16", None), (None, "bf16")):
        ck = str(tmp_path / ("%s.ckpt" % first))
        W.spawn(W.run_worker, 1, False, paths, operand=first, epochs=1, save=ck)
        res = W.spawn(W.run_worker, 1, False, paths, operand=then, epochs=1, load=ck)[0]
        assert [h["epoch"] for h in res["history"]] == [0, 1]          # the checkpoint's epoch, then one more
    assert "operand" not in pkg("checkpoint").ARCH_FIELDS and not hasattr(pkg("PGAT"), "OPERANDS") and M.OPERANDS
