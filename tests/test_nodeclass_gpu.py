"""The masked loss / accuracy kernels on the GPU (csrc/pgcn_loss.hip: pgcn_masked_nll_f32, pgcn_masked_nll_backward_f32) against
float64 and numpy, their repeatability, graph capture, and the node-classification loop end to end: P real-kernel ranks on one GPU
against one rank and the float64 reference of tests/_nodeclass_workers.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _nodeclass_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

# test_hip_gpu.test_row_nll_kernels_vs_torch's shapes + the class counts of real data sets + padded leading dimensions
SHAPES = [(1, 1, 1), (513, 16, 16), (4000, 128, 128), (777, 100, 104), (300, 1024, 1024), (50, 65, 65), (1001, 256, 260), (35, 64, 64),
          (18, 4, 4), (5000, 7, 7), (3001, 41, 41), (2000, 47, 48), (999, 172, 172), (640, 7, 12), (100003, 41, 64), (70001, 172, 176),
          (232965, 128, 128), (0, 41, 41)]


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _case(dev, n, C, ld, seed=None):
    g = torch.Generator(device=dev)
    g.manual_seed(n + C if seed is None else seed)
    buf = torch.randn((n, ld), device=dev, generator=g) * 8
    y = torch.randint(0, C, (n,), device=dev, generator=g)
    s = torch.randint(0, 4, (n,), device=dev, generator=g).to(torch.uint8)
    if n > 6 and C > 2:
        buf[1, 0] = float("-inf")
        buf[2, :C] = 300.0                                           # equal maxima everywhere: arg-max 0
        buf[3, 1] = -300.0
        buf[4, :C] = float("-inf")
        buf[4, C - 1] = 1.0
        buf[5, C // 2:C] = buf[5, :C].max() + 1.0                    # equal maxima from the middle on
        y[1], y[4] = 1, C - 1                                        # (finite entries: the row losses stay finite)
        s[1], s[2], s[4], s[5] = 1, 2, 1, 3
    y[s == 0] = -1                                                   # unlabelled rows are in no set
    return buf[:, :C], y, s


def _check_forward(x, y, s, lse, st):
    n, C = x.shape
    xd = x.double()
    ref_lse = torch.logsumexp(xd, 1)
    if n:
        assert float((lse.double() - ref_lse).abs().max()) <= 1e-5 * max(1.0, float(ref_lse.abs().max()))
    pred = np.argmax(x.cpu().numpy(), 1) if n else np.zeros(0, np.int64)
    yh, sh = y.cpu().numpy(), s.cpu().numpy()
    for k in (1, 2, 3):
        m = sh == k
        assert int(st.rows[k]) == int(m.sum())
        assert int(st.correct[k]) == int((pred[m] == yh[m]).sum())
        mt = torch.from_numpy(m).to(x.device)
        want = float(F.cross_entropy(xd[mt], y[mt], reduction="sum")) if m.any() else 0.0
        got = float(st.loss_sum[k])
        print("set %d: %d rows, loss_sum %.9g (float64 %.9g)" % (k, int(m.sum()), got, want))
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert int(st.rows[0]) == int((sh == 0).sum()) and float(st.loss_sum[0]) == 0.0 and int(st.correct[0]) == 0


@pytest.mark.parametrize("n,C,ld", SHAPES)
def test_masked_kernels_against_float64(K, dev, n, C, ld, monkeypatch):
    P = pkg("PGCN")
    monkeypatch.setattr(P, "_kernel_provider", K)                    # masked_loss asks this provider for the kernels
    x, y, s = _case(dev, n, C, ld)
    out = K.masked_nll(x, y, s)
    assert out is not None
    lse, st = out
    _check_forward(x, y, s, lse, st)
    again = K.masked_nll(x, y, s)                                    # two calls: the same bits
    assert torch.equal(again[0], lse) and all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(again[1], st))
    # through the autograd node, against float64 cross entropy over the train rows
    n_train = int((s == 1).sum()) + 3
    xg = x.detach().clone().requires_grad_(True) if ld == C else x.detach().requires_grad_(True)
    loss, st2 = P.masked_loss(xg, y, s, n_train)
    (loss * 1.5).backward()
    train = s == 1
    xr = x.detach().double().requires_grad_(True)
    ref = F.cross_entropy(xr[train], y[train], reduction="sum") / n_train
    (ref * 1.5).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
    assert torch.equal(st2.correct, st.correct) and torch.equal(st2.rows, st.rows)
    assert torch.equal(st2.loss_sum.view(torch.int64), st.loss_sum.view(torch.int64))       # the kernel's record, not the composition's
    if n:
        assert float((xg.grad.double() - xr.grad)[train].abs().max() if bool(train.any()) else 0.0) <= 2e-6
        assert torch.equal(xg.grad[~train], torch.zeros_like(xg.grad[~train]))
    dx = K.masked_nll_backward(x, y, s, lse, torch.ones((), device=dev), 1.0 / n_train)
    assert torch.equal(dx, K.masked_nll_backward(x, y, s, lse, torch.ones((), device=dev), 1.0 / n_train))
    torch.cuda.synchronize()


def test_backward_overwrites_padded_blocks(K, dev):
    """Padded leading dimensions on both paths (44 of 48 columns: float4; 41 of 48: a wave per row), a device-side factor and a scale."""
    for C, ld in ((44, 48), (41, 48), (44, 44), (41, 41)):
        x, y, s = _case(dev, 3001, C, ld)               # (each width gets rows of its own: a sliced row could be all -inf)
        lse, _ = K.masked_nll(x, y, s)
        dx = K.masked_nll_backward(x, y, s, lse, torch.full((), 2.0, device=dev), 0.25)
        train = s == 1
        xr = x.double().requires_grad_(True)
        (F.cross_entropy(xr[train], y[train], reduction="sum") * 0.5).backward()
        assert dx.shape == (3001, C) and bool(torch.isfinite(dx).all())
        assert float((dx.double() - xr.grad).abs().max()) <= 2e-6 and torch.equal(dx[~train], torch.zeros_like(dx[~train]))


@pytest.mark.parametrize("C", [7, 128])
def test_equal_maxima_take_the_lowest_index(K, dev, C):
    n = 4096
    g = torch.Generator(device=dev)
    g.manual_seed(C)
    x = torch.randint(0, 3, (n, C), device=dev, generator=g).float()       # many ties in every row
    y = torch.randint(0, C, (n,), device=dev, generator=g)
    pred = torch.from_numpy(np.argmax(x.cpu().numpy(), 1)).to(dev)
    y[::2] = pred[::2]                                                       # half the rows are right by the lowest-index rule
    s = (torch.arange(n, device=dev) % 3 + 1).to(torch.uint8)
    lse, st = K.masked_nll(x, y, s)
    for k in (1, 2, 3):
        assert int(st.correct[k]) == int(((pred == y) & (s == k)).sum()) and int(st.rows[k]) == int((s == k).sum())
    assert int(st.correct[1:].sum()) >= n // 2


def test_all_zero_split_and_unlabelled_rows(K, dev):
    x, y, _ = _case(dev, 1000, 41, 41)
    s = torch.zeros(1000, dtype=torch.uint8, device=dev)
    y[:] = -1
    lse, st = K.masked_nll(x, y, s)
    assert st.rows.tolist() == [1000, 0, 0, 0] and st.correct.tolist() == [0, 0, 0, 0] and st.loss_sum.tolist() == [0.0] * 4
    assert float((lse.double() - torch.logsumexp(x.double(), 1)).abs().max()) <= 1e-5 * float(lse.abs().max())
    dx = K.masked_nll_backward(x, y, s, lse, torch.ones((), device=dev), 1.0)
    assert torch.equal(dx, torch.zeros_like(dx))
    # a label far outside [0, C) on a row in no set is never used as an index
    y[:] = 2 ** 40
    lse2, st2 = K.masked_nll(x, y, s)
    assert torch.equal(lse2, lse) and st2.rows.tolist() == [1000, 0, 0, 0]
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [41, 128])
def test_out_of_range_label_poisons_its_set_only(K, dev, C):
    x, y, s = _case(dev, 2000, C, C)
    i = int(torch.nonzero(s == 1)[10])
    good = K.masked_nll(x, y, s)[1]
    for bad in (C, -1, 2 ** 40):
        y2 = y.clone()
        y2[i] = bad
        lse, st = K.masked_nll(x, y2, s)
        assert bool(torch.isnan(st.loss_sum[1]))
        assert torch.equal(st.loss_sum[2:].view(torch.int64), good.loss_sum[2:].view(torch.int64))
        hit = bool(x[i].argmax() == y[i])
        assert int(st.correct[1]) == int(good.correct[1]) - (1 if hit else 0) and torch.equal(st.rows, good.rows)
        dx = K.masked_nll_backward(x, y2, s, lse, torch.ones((), device=dev), 1.0)
        assert float((dx[i].double() - torch.exp(x[i].double() - lse[i].double())).abs().max()) <= 2e-6   # no column matches
    torch.cuda.synchronize()


def test_more_than_1024_columns_is_refused(K, dev):
    _lib = pkg("_lib")
    x = torch.zeros((4, 1025), device=dev)
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    s = torch.ones(4, dtype=torch.uint8, device=dev)
    assert K.masked_nll(x, y, s) is None and K.masked_nll_backward(x, y, s, torch.zeros(4, device=dev), torch.ones((), device=dev), 1.0) is None
    rec = torch.zeros(12, dtype=torch.int64, device=dev)
    ws = torch.zeros(64, dtype=torch.int64, device=dev)
    rc = K.lib.pgcn_masked_nll_f32(x.data_ptr(), 1025, y.data_ptr(), s.data_ptr(), 4, 1025, torch.zeros(4, device=dev).data_ptr(),
                                   rec.data_ptr(), ws.data_ptr(), 512, None)
    assert rc == _lib.PGCN_EUNSUPPORTED
    assert K.lib.pgcn_masked_nll_ws_bytes(0) == 96 and K.lib.pgcn_masked_nll_ws_bytes(65) == 192
    # and the composition takes over in masked_loss
    P = pkg("PGCN")
    loss, st = P.masked_loss(x.requires_grad_(True), y, s, 4)
    assert abs(float(loss.detach()) - float(np.log(1025))) <= 1e-5 * np.log(1025) and st.rows.tolist() == [0, 4, 0, 0]


def test_forward_and_backward_replay_in_one_graph(K, dev):
    """Captured on a single stream: a host synchronisation or an allocation outside the pool would fail the capture."""
    n, C = 20000, 41
    x, y, s = _case(dev, n, C, C, seed=1)
    x = x.contiguous()
    gs = torch.ones((), device=dev)
    K.masked_nll(x, y, s)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            lse, st = K.masked_nll(x, y, s)
            dx = K.masked_nll_backward(x, y, s, lse, gs, 0.5)
    torch.cuda.synchronize()
    x2, _, _ = _case(dev, n, C, C, seed=2)
    x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    _check_forward(x, y, s, lse, st)
    train = s == 1
    xr = x.double().requires_grad_(True)
    (F.cross_entropy(xr[train], y[train], reduction="sum") * 0.5).backward()
    assert float((dx.double() - xr.grad).abs().max()) <= 2e-6 and torch.equal(dx[~train], torch.zeros_like(dx[~train]))
    eager = K.masked_nll(x, y, s)
    assert torch.equal(eager[0], lse) and torch.equal(eager[1].loss_sum.view(torch.int64), st.loss_sum.view(torch.int64))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("nodeclass_gpu")))


@pytest.mark.parametrize("dropout", [0.0, W.DROPOUT])
def test_ranks_on_one_gpu_against_one_rank_and_float64(dataset, dropout):
    paths, data = dataset
    ref, final = W.float64_reference(data, [W.FIN, W.HIDDEN, W.CLASSES], dropout=dropout)
    one = None
    for P in (1, 2, 3):
        res = W.spawn_run(P, paths, True, dropout=dropout)
        assert all(r["hip"] == "HipKernels" for r in res)
        worst = W.check_against_reference(res, ref, final, data)
        print("P = %d, dropout %.1f: largest relative loss error against float64 %.3g" % (P, dropout, worst))
        if one is None:
            one = res
        else:
            for a, b in zip(one[0]["history"], res[0]["history"]):
                assert a["rows"] == b["rows"]
                for name in W.SETS:                                 # against one rank: both within the criterion of the same reference
                    assert abs(a["losses"][name] - b["losses"][name]) <= 2e-5 * abs(a["losses"][name])
    last = one[0]["stdout"].strip().splitlines()[-1].split()
    assert last[:2] == ["Best", "Val"] and last[3:5] == ["at", "epoch"] and last[6:8] == ["|", "Test"]
    best = one[0]["best"]
    assert abs(float(last[2]) - best["val"]) < 1e-4 and int(last[5]) == best["epoch"] and abs(float(last[8]) - best["test"]) < 1e-4
