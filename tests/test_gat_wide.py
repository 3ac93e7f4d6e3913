"""Layers of 257 to 1024 columns without a GPU: the switch, the shape predicates, and two training steps of `PGAT.run` at 8 x 64 on the
checker-backed provider (which has no wide kernels, so the engine keeps the route of before)."""
import math

import _workers
from conftest import gpath, pkg
from test_engine_gloo import _spawn
from test_gat_gloo import _losses


def test_switch_and_shapes():
    T, gat, kernels = pkg("tuning"), pkg("gat"), pkg("kernels")
    assert T.load({}).gat_wide is True and T.load({"PGCN_TUNING": "gat_wide=0"}).gat_wide is False
    wide = kernels.HipKernels._heads_wide
    assert all(wide(h, d) for h, d in [(8, 64), (5, 64), (3, 128), (4, 128), (8, 128), (2, 256), (3, 256), (4, 256)])
    assert not any(wide(h, d) for h, d in [(4, 64), (2, 128), (1, 256), (5, 256), (9, 64), (16, 32), (5, 96), (0, 64)])
    eng = object.__new__(gat.GatEngine)
    eng.wide, eng.k = True, kernels.HipKernels
    assert eng._wide(8, 64) and not eng.covers(8, 64) and eng.covers(4, 64) and not eng._wide(4, 64)
    eng.wide = False
    assert not eng._wide(8, 64)
    eng.wide, eng.k = True, object()                     # a provider without the kernels
    assert not eng._wide(8, 64)


def test_run_trains_two_steps_at_8x64():
    """`PGAT.run` (the command line's body) with 8 heads x 64 on two gloo ranks: two optimizer steps over the reused layer states."""
    res = _spawn(_workers.gat_run_worker, 2, gpath("karate.A.mtx"), gpath("karate.mtx.2.rp"), "standard", 8, 2, 512, 3, 2)
    losses = _losses(res[0]["stdout"])                    # (rank 0 prints the global loss)
    assert all(r["provider"] == "OracleKernels" for r in res)
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses) and losses[1] < losses[0]
