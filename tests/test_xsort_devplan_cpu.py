"""The xsort plan accessors exist: exported by libsblas.so, declared in
include/sblas.h, bound on sblas.DeviceCSR (no GPU needed)."""
import inspect
import os
import re
import subprocess

from conftest import ROOT

LIB = os.path.join(ROOT, "s-blas_amd", "libsblas.so")
NAMES = ("sblas_csr_xsort_export", "sblas_csr_xsort_build_info")


def test_library_exports_the_accessors(sb):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True,
                         text=True).stdout
    syms = {line.split(" ", 2)[2] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "sblas.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert n in syms
        assert re.search(r"\b%s\s*\(" % n, header)
        getattr(sb.lib, n)  # resolvable through the loader too


def test_devicecsr_binds_the_accessors(sb):
    assert list(inspect.signature(sb.DeviceCSR.xsort_export).parameters) == ["self", "what"]
    assert list(inspect.signature(sb.DeviceCSR.xsort_build_info).parameters) == ["self"]
    assert sb.lib.sblas_csr_xsort_export.argtypes is not None
    assert len(sb.lib.sblas_csr_xsort_export.argtypes) == 5
    assert len(sb.lib.sblas_csr_xsort_build_info.argtypes) == 2


def test_null_handle_is_refused(sb):
    assert sb.lib.sblas_csr_xsort_export(None, 0, None, 0, None) == 1
    assert sb.lib.sblas_csr_xsort_build_info(None, None) == 1


def test_hook_lists_name_the_host_plan_options():
    for path in ("include/sblas.h", "s-blas_amd/csrc/sblas_internal.hpp"):
        text = open(os.path.join(ROOT, path)).read()
        for hook in ("xs_hostplan", "csr5_hostplan"):
            assert '"%s"' % hook in text, (path, hook)
