"""pgcn_predict_f32 (csrc/pgcn_predict.hip) on the device against numpy on the same fp32 logits (tests/_predict_workers.py: the bounds
are derived there): classes and label bits exactly, confidences and probabilities within the derived bounds, over the shape grid with
planted ties; a planted NaN; layout (leading dimensions, poisoned padding, canary rows, a misaligned base, NULL outputs, refusals);
repeatability and graph capture; agreement with the loss kernels' counts; then save / resume / predict end to end through both
launchers.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import _predict_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.25e33)


@pytest.fixture(scope="module")
def env():
    kernels, _lib = pkg("kernels"), pkg("_lib")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, _lib


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _unpack(bits, C):
    return pkg("nodedata").unpack_label_words(bits.cpu().numpy(), C).astype(bool)


def _worst(err, bound):
    return float((err / bound).max()) if err.size else 0.0


def _check_single(where, X, out, Xt=None):
    n, C = X.shape
    cls = out.cls.cpu().numpy()
    assert cls.dtype == np.int64 and np.array_equal(cls, W.argmax_first(X)), where            # integers get no tolerance
    if n == 0:
        return
    P64, _ = W.softmax64(X)
    bp, bc, brow = W.softmax_bounds(X)
    prob, conf = out.prob.cpu().numpy().astype(np.float64), out.conf.cpu().numpy().astype(np.float64)
    ep, ec = _worst(np.abs(prob - P64), bp), _worst(np.abs(conf - P64.max(axis=1)), bc)
    er = _worst(np.abs(prob.sum(axis=1) - 1.0), brow)
    line = "%s: error / bound  prob %.3g  conf %.3g  row sums %.3g" % (where, ep, ec, er)
    if Xt is not None:               # for the record, not asserted: torch's own fp32 softmax on the same device and input
        line += "   (torch.softmax fp32: %.3g)" % _worst(np.abs(torch.softmax(Xt, 1).cpu().numpy().astype(np.float64) - P64), bp)
    print(line, flush=True)
    assert ep <= 1.0 and ec <= 1.0 and er <= 1.0, line
    assert np.array_equal(out.conf.cpu().numpy(), out.prob.cpu().numpy()[np.arange(n), cls])      # conf IS the probability of cls


def _check_multi(where, X, out):
    n, C = X.shape
    bits = out.bits.cpu().numpy()
    assert bits.dtype == np.int32 and bits.shape == (n, (C + 31) // 32), where
    assert np.array_equal(bits.view(np.uint32), pkg("nodedata").pack_label_words(X > 0)), where   # exactly, bits at and above C zero
    if n == 0:
        return
    e = _worst(np.abs(out.prob.cpu().numpy().astype(np.float64) - W.sigmoid64(X)), W.sigmoid_bound(X))
    print("%s: error / bound  sigmoid %.3g" % (where, e), flush=True)
    assert e <= 1.0, where


@pytest.mark.parametrize("C", W.GRID_C)
def test_classes_bits_and_probabilities_over_the_shape_grid(env, C):
    """256 / 260 columns: the last row of one wave and the first of two; 32 / 33: the word boundary of the bits; 128 / 129 rows: a band
    and one row more.  Planted: equal maxima at columns (3, 4), (0, C - 1), (255, 256), an all-equal row, -inf everywhere but one
    column, a row of +0.0 / -0.0 (nothing there is > 0)."""
    k, dev, _ = env
    for n in W.GRID_N:
        X, planted = W.make_logits(n, C)
        Xt = _t(X, dev)
        single = k.predict(Xt, "single", want_prob=True)
        multi = k.predict(Xt, "multilabel", want_prob=True)
        assert single.bits is None and multi.cls is None and multi.conf is None
        _check_single("single n = %d C = %d" % (n, C), X, single, Xt)
        _check_multi("multilabel n = %d C = %d" % (n, C), X, multi)
        cls = single.cls.cpu().numpy()
        for name, want in (("tie3_4", 3), ("tie0_%d" % (C - 1), 0), ("tie255_256", 255), ("equal", 0), ("neginf", C // 2), ("zeros", 0)):
            if name in planted:
                assert cls[planted[name]] == want, (name, n, C)
        if "zeros" in planted:
            assert not multi.bits[planted["zeros"]].any()
        if "neginf" in planted:
            assert float(single.conf[planted["neginf"]]) == 1.0


@pytest.mark.parametrize("C", [5, 41, 128, 260])
def test_a_nan_stays_in_its_row_and_cls_is_what_the_loss_kernel_counts(env, C):
    """A NaN planted in one row leaves every other row's outputs bit-identical; that row's cls is the arg-max pgcn_masked_nll_f32 counts:
    a label equal to it is a hit, any other is not (one pass of the loss kernel per candidate label)."""
    k, dev, _ = env
    n, row = 131, 77
    X, _ = W.make_logits(n, C, seed=1)
    Xn = X.copy()
    Xn[row, C // 3] = np.nan
    a, b = k.predict(_t(X, dev), "single", want_prob=True), k.predict(_t(Xn, dev), "single", want_prob=True)
    ma, mb = k.predict(_t(X, dev), "multilabel", want_prob=True), k.predict(_t(Xn, dev), "multilabel", want_prob=True)
    others = torch.arange(n, device=dev) != row
    for x, y in ((a.cls, b.cls), (a.conf, b.conf), (a.prob, b.prob), (ma.bits, mb.bits), (ma.prob, mb.prob)):
        assert torch.equal(x[others].view(torch.int32 if x.dtype is torch.float32 else x.dtype),
                           y[others].view(torch.int32 if y.dtype is torch.float32 else y.dtype))
    cls = int(b.cls[row])
    assert cls == int(W.argmax_first(Xn)[row]) and 0 <= cls < C
    assert bool(torch.isnan(b.conf[row])) and not _unpack(mb.bits, C)[row, C // 3]
    split = torch.zeros(n, dtype=torch.uint8, device=dev)
    split[row] = 2
    hits = []
    for label in range(C):
        labels = torch.full((n,), label, dtype=torch.int64, device=dev)
        hits.append(int(k.masked_nll(_t(Xn, dev), labels, split)[1].correct[2]))
    assert hits == [1 if label == cls else 0 for label in range(C)], (cls, hits)
    # a row of NaN only: no class, no label is a hit
    Xn[row] = np.nan
    c = k.predict(_t(Xn, dev), "single")
    assert int(c.cls[row]) == -1
    assert int(k.masked_nll(_t(Xn, dev), torch.zeros(n, dtype=torch.int64, device=dev), split)[1].correct[2]) == 0


def _raw(lib, X, ldx, n, C, task, cls=None, conf=None, bits=None, prob=None, ldp=0, stream=0):
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    return lib.pgcn_predict_f32(p(X), ldx, n, C, task, p(cls), p(conf), p(bits), p(prob), ldp, stream)


@pytest.mark.parametrize("C", [3, 8, 33, 128, 260])
def test_layout_padding_canaries_misaligned_base_and_null_outputs(env, C):
    k, dev, _lib = env
    lib, n, pad, canary = _lib.lib(), 129, 5, 3
    X, _ = W.make_logits(n, C, seed=2)
    want = k.predict(_t(X, dev), "single", want_prob=True)
    wantm = k.predict(_t(X, dev), "multilabel", want_prob=True)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    # leading dimensions larger than C, poisoned padding; canary rows behind the last row; a base misaligned by 4 bytes
    for ld, off in ((C + pad, 0), (C + 4, 1), (C, 1)):
        Xbuf = torch.full(((n + canary) * ld + off,), float(POISON), dtype=torch.float32, device=dev)
        Xv = Xbuf[off:].view(n + canary, ld)
        Xv[:n, :C] = _t(X, dev)
        Pbuf = torch.full_like(Xbuf, float(POISON))
        Pv = Pbuf[off:].view(n + canary, ld)
        cls = torch.full((n + canary,), -99, dtype=torch.int64, device=dev)
        conf = torch.full((n + canary,), float(POISON), dtype=torch.float32, device=dev)
        mw = (C + 31) // 32
        bits = torch.full((n + canary, mw), -99, dtype=torch.int32, device=dev)
        _lib.check(_raw(lib, Xv, ld, n, C, 0, cls, conf, None, Pv, ld, stream), "pgcn_predict_f32")
        torch.cuda.synchronize()
        assert torch.equal(cls[:n], want.cls) and bool((cls[n:] == -99).all())
        assert torch.equal(conf[:n].view(torch.int32), want.conf.view(torch.int32)) and bool((conf[n:] == float(POISON)).all())
        assert torch.equal(Pv[:n, :C].contiguous().view(torch.int32), want.prob.view(torch.int32))        # the bits of the float4 path
        assert bool((Pv[:n, C:] == float(POISON)).all()) and bool((Pv[n:] == float(POISON)).all()) and bool((Pbuf[:off] == float(POISON)).all())
        assert bool((bits == -99).all())                                                                  # task 0 leaves bits alone
        Pbuf.fill_(float(POISON))
        _lib.check(_raw(lib, Xv, ld, n, C, 1, cls, conf, bits, Pv, ld, stream), "pgcn_predict_f32")
        torch.cuda.synchronize()
        assert torch.equal(bits[:n], wantm.bits) and bool((bits[n:] == -99).all())
        assert torch.equal(Pv[:n, :C].contiguous().view(torch.int32), wantm.prob.view(torch.int32))
        assert bool((Pv[:n, C:] == float(POISON)).all()) and bool((Pv[n:] == float(POISON)).all())
        assert torch.equal(cls[:n], want.cls) and torch.equal(conf[:n].view(torch.int32), want.conf.view(torch.int32))   # task 1 leaves them
    # NULL outputs are not formed, the others are the same
    Xt = _t(X, dev)
    only = k.predict(Xt, "single", want_conf=False, want_prob=False)
    assert only.conf is None and only.prob is None and torch.equal(only.cls, want.cls)
    conf = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_raw(lib, Xt, C, n, C, 0, None, conf, None, None, 0, stream), "pgcn_predict_f32")
    assert torch.equal(conf.view(torch.int32), want.conf.view(torch.int32))
    assert _raw(lib, Xt, C, n, C, 0, None, None, None, None, 0, stream) == 0 and _raw(lib, Xt, C, n, C, 1, None, None, None, None, 0, stream) == 0
    assert _raw(lib, None, C, 0, C, 0, None, None, None, None, 0, stream) == 0                            # nrows == 0 launches nothing


def test_bad_sizes_are_refused_with_nothing_launched(env):
    k, dev, _lib = env
    lib = _lib.lib()
    X = torch.zeros((4, 1025), dtype=torch.float32, device=dev)
    cls = torch.full((4,), -99, dtype=torch.int64, device=dev)
    prob = torch.full((4, 1025), 5.0, dtype=torch.float32, device=dev)
    for args in ((X, 1025, 4, 1025, 0, cls, None, None, None, 0), (X, 7, 4, 8, 0, cls, None, None, None, 0),
                 (X, 8, 4, 8, 0, cls, None, None, prob, 7), (X, 8, 4, 0, 0, cls, None, None, None, 0),
                 (X, 8, -1, 8, 0, cls, None, None, None, 0), (X, 8, 4, 8, 2, cls, None, None, None, 0)):
        assert _raw(lib, *args) == -1
        assert b"pgcn_predict_f32" in lib.pgcn_last_error()
    torch.cuda.synchronize()
    assert bool((cls == -99).all()) and bool((prob == 5.0).all())
    assert k.predict(X, "single") is None and k.predict(X.double()[:, :8], "single") is None       # the gate: operands it does not take


@pytest.mark.parametrize("task", ["single", "multilabel"])
def test_two_calls_and_a_captured_replay_give_the_same_bits(env, task):
    k, dev, _ = env
    X, _ = W.make_logits(513, 100, seed=3)
    Xt = _t(X, dev)
    a, b = k.predict(Xt, task, want_prob=True), k.predict(Xt, task, want_prob=True)
    same = lambda x, y: all(u is None and v is None or torch.equal(u.view(torch.int32) if u.dtype is torch.float32 else u,    # noqa: E731
                                                                   v.view(torch.int32) if v.dtype is torch.float32 else v) for u, v in zip(x, y))
    assert same(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        k.predict(Xt, task, want_prob=True)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = k.predict(Xt, task, want_prob=True)
    for t in c:
        if t is not None:
            t.zero_()
    graph.replay()                                          # one replay, single stream
    torch.cuda.synchronize()
    assert same(a, c)


def test_counts_from_predictions_equal_the_loss_kernels_counts(env):
    """Hit counts recomputed from cls / bits and the labels equal masked_nll(...).correct and the tp / fp / fn planes of masked_bce
    exactly: random logits (with exact ties: quantised to 1 / 4), every set present."""
    k, dev, _ = env
    ND = pkg("nodedata")
    rng = np.random.default_rng(9)
    for n, C in ((1000, 7), (777, 41), (300, 128), (130, 260)):
        X = (np.round(4 * rng.standard_normal((n, C))) / 4).astype(np.float32)
        split = rng.integers(0, 4, n).astype(np.uint8)
        labels = rng.integers(0, C, n).astype(np.int64)
        Xt, st, lt = _t(X, dev), _t(split, dev), _t(labels, dev)
        cls = k.predict(Xt, "single").cls
        correct = k.masked_nll(Xt, lt, st)[1].correct.cpu().numpy()
        mine = [int(((cls == lt) & (st == s)).sum()) for s in (1, 2, 3)]
        assert (X == X.max(axis=1, keepdims=True)).sum(axis=1).max() > 1                       # there ARE equal maxima
        assert mine == correct[1:].tolist(), (n, C, mine, correct)
        Y = rng.integers(0, 2, (n, C)).astype(np.uint8)
        words = _t(ND.pack_label_words(Y).view(np.int32), dev)
        rec = k.masked_bce(Xt, words, st)
        p, y = _unpack(k.predict(Xt, "multilabel").bits, C), Y.astype(bool)
        for s in (1, 2, 3):
            m = (split == s)[:, None]
            assert (int((p & y & m).sum()), int((p & ~y & m).sum()), int((~p & y & m).sum())) == \
                (int(rec.tp[s]), int(rec.fp[s]), int(rec.fn[s])), (n, C, s)


# ---- end to end: ranks on one GPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.NW.make_dataset(str(tmp_path_factory.mktemp("predict_gpu")))


@pytest.mark.parametrize("P", [1, 2])
def test_train_save_predict_reproduces_the_best_record(dataset, tmp_path, P):
    """Dropout configuration: the counts recomputed from pred.npy equal the best record's exactly -- both come from the same eval-mode
    forward over the same weights through kernels without atomics.  Then --load --epochs 0 --predict writes the same files."""
    paths, data = dataset
    d = str(tmp_path)
    kw = W.data_kw(paths, hidden=W.HIDDEN, epochs=W.EPOCHS, lr=W.LR_OVERSHOOT_DROPOUT, dropout=W.DROPOUT, dropout_seed=W.DROPOUT_SEED)
    jobs = [dict(kw=dict(kw, save=d + "/m.pt", predict=d + "/out", proba=True)),
            dict(kw=dict(kw, epochs=0, load=d + "/m.pt", predict=d + "/again", proba=True))]
    res = W.spawn_jobs(P, paths, True, "PGCN", jobs)[0]
    assert all("error" not in r for r in res), res
    assert res[0]["hip"] == "HipKernels"
    best = res[0]["best"]
    got = W.counts_from_files(d + "/out", data["labels"], data["split"])
    print("P = %d: best epoch %d of %d, correct %r, from pred.npy %r" % (P, best["epoch"], W.EPOCHS, best["correct"], got["correct"]))
    assert 0 <= best["epoch"] < W.EPOCHS - 1, "the best epoch must not be the last one"
    assert got["correct"] == best["correct"]
    assert "Predicting with the weights of the best epoch %05d" % best["epoch"] in res[0]["stdout"]
    for ext in (".pred.npy", ".conf.npy", ".prob.npy"):
        assert np.array_equal(np.load(d + "/out" + ext), np.load(d + "/again" + ext)), ext
    assert W.same_entry(res[1]["best"], best) and not [f for f in os.listdir(d) if f.endswith(".tmp")]


def _resume_jobs(d, kw):
    return [dict(kw=dict(kw, epochs=W.EPOCHS, save=d + "/straight.pt")), dict(kw=dict(kw, epochs=W.EPOCHS, save=d + "/repeat.pt")),
            dict(kw=dict(kw, epochs=W.FIRST_LEG, save=d + "/leg.pt")),
            dict(kw=dict(kw, epochs=W.EPOCHS - W.FIRST_LEG, load=d + "/leg.pt", save=d + "/resumed.pt"))]


def _check_resume(where, d, res):
    """The resumed run is as close to the straight run as the straight run's repeat is: bit-identical where the repeat is, else its
    largest weight difference may not exceed the repeat's.  The yardstick is the parent behaviour -- a repeat run."""
    assert all("error" not in r for r in res), res
    straight, repeat, resumed = (torch.load(d + "/%s.pt" % name, weights_only=True) for name in ("straight", "repeat", "resumed"))
    gap = lambda a, b: max(float((a["model"][k].double() - b["model"][k].double()).abs().max()) for k in a["model"])      # noqa: E731
    g_repeat, g_resumed = gap(straight, repeat), gap(straight, resumed)
    print("%s: largest weight difference to the straight run: its repeat %.3g, the resumed run %.3g" % (where, g_repeat, g_resumed))
    assert resumed["epochs"] == straight["epochs"] == W.EPOCHS and resumed["dropout_step"] == straight["dropout_step"]
    assert [h["epoch"] for h in resumed["history"]] == list(range(W.EPOCHS))
    if g_repeat == 0.0:
        keys = ("model", "optimizer", "best")
        assert not W.same_state({k: straight[k] for k in keys}, {k: repeat[k] for k in keys})
        assert not W.same_state({k: straight[k] for k in keys}, {k: resumed[k] for k in keys})
        assert all(W.same_entry(a, b) for a, b in zip(straight["history"], resumed["history"]))
    else:
        assert g_resumed <= g_repeat


def test_resume_is_as_close_to_the_straight_run_as_its_repeat(dataset, tmp_path):
    paths, _ = dataset
    d = str(tmp_path)
    kw = W.config_kw("buffers", paths)
    _check_resume("PGCN, dropout + batch norm + fused Adam", d, W.spawn_jobs(1, paths, True, "PGCN", _resume_jobs(d, kw))[0])


def test_pgat_train_save_resume_predict(tmp_path):
    """One PGAT run of the same shape, dropout configuration, one rank: the counts of the best record from pred.npy; resume against a
    repeat."""
    d = str(tmp_path)
    paths, data = W.TW.make_datasets(d)
    kw = W.config_kw("gat", paths)
    jobs = _resume_jobs(d, kw) + [dict(kw=dict(kw, epochs=W.EPOCHS, predict=d + "/out"))]
    res = W.spawn_jobs(1, paths, True, "PGAT", jobs)[0]
    _check_resume("PGAT, dropout + fused Adam", d, res[:4])
    best = res[4]["best"]
    got = W.counts_from_files(d + "/out", data["single"]["labels"], data["single"]["split"])
    print("PGAT: best epoch %d of %d, correct %r, from pred.npy %r" % (best["epoch"], W.EPOCHS, best["correct"], got["correct"]))
    assert got["correct"] == best["correct"]
