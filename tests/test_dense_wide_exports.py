"""include/pgcn_dense_wide.h: every entry point it declares is exported by libpgcn_gemm.so and bound by PGCN.bind_dense_library with
the declared argument counts; the wide_*_fused functions leave CPU tensors to the library route; the tunable parses.
(A header of its own for the reason of include/pgcn_wgrad_masked.h: tests/test_zz_dense_fused.py pins the names in pgcn_gemm.h.)"""
import ctypes
import os
import re

import torch

from conftest import ROOT, pkg

ARGS = {"pgcn_dense_wide_abi_version": 0, "pgcn_dense_wide_last_error": 0, "pgcn_wide_image_ws_bytes": 2, "pgcn_wide_linear_relu_f32": 19,
        "pgcn_wide_grad_input_f32": 16, "pgcn_wide_weight_grad_ws_elems": 3, "pgcn_wide_weight_grad_f32": 14}


def test_library_exports_the_wide_entry_points():
    P = pkg("PGCN")
    src = open(os.path.join(ROOT, "include", "pgcn_dense_wide.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(pgcn_[a-z0-9_]+)\s*\(", src))) == sorted(ARGS)
    L = ctypes.CDLL(P.GEMM_LIB_PATH)
    for name in ARGS:
        assert hasattr(L, name), "libpgcn_gemm.so does not export %s" % name
    B = P.bind_dense_library(P.GEMM_LIB_PATH)
    assert B.pgcn_has_dense_wide and B.pgcn_dense_wide_abi_version() == 1
    for name, count in ARGS.items():
        assert len(getattr(B, name).argtypes) == count, name
    # host-side answers: 48 KB per chunk of 64 x 128; partial matrices of at most 32 MB
    assert B.pgcn_wide_image_ws_bytes(256, 256) == 8 * 49152 and B.pgcn_wide_image_ws_bytes(132, 8) == 3 * 49152
    assert B.pgcn_wide_weight_grad_ws_elems(232965, 256, 256) == 128 * 256 * 256
    assert 0 < B.pgcn_wide_weight_grad_ws_elems(1, 1024, 1024) <= 8 << 20


def test_cpu_tensors_and_the_tunable():
    P, T = pkg("PGCN"), pkg("tuning")
    x, w = torch.randn(5, 256), torch.randn(256, 256)
    assert P.wide_linear_relu_fused(x, w, True, True) is None
    assert P.wide_grad_input_fused(x, None, 1.0, w, False) is None
    assert P.wide_weight_grad_masked_fused(x, None, 1.0, x) is None
    assert T.load({"PGCN_TUNING": "dense_wide=0"}).dense_wide == 0 and T.load({}).dense_wide in (0, 1)
