"""include/pgcn_wgrad_masked.h: every entry point it declares is exported by libpgcn_gemm.so and bound by PGCN.bind_dense_library.
(The declarations have a header of their own because tests/test_zz_dense_fused.py pins the list of names in include/pgcn_gemm.h.)"""
import ctypes
import os
import re

from conftest import ROOT, pkg


def test_library_exports_the_masked_weight_gradient():
    P = pkg("PGCN")
    src = open(os.path.join(ROOT, "include", "pgcn_wgrad_masked.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(pgcn_[a-z0-9_]+)\s*\(", src)))
    assert names == ["pgcn_linear_weight_grad_masked_f32", "pgcn_wgrad_masked_abi_version"]
    L = ctypes.CDLL(P.GEMM_LIB_PATH)
    for n in names:
        assert hasattr(L, n), "libpgcn_gemm.so does not export %s" % n
    B = P.bind_dense_library(P.GEMM_LIB_PATH)
    assert B.pgcn_has_wgrad_masked and B.pgcn_wgrad_masked_abi_version() == 1
    assert len(B.pgcn_linear_weight_grad_masked_f32.argtypes) == 14
