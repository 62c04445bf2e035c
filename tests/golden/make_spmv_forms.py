"""Regenerate tests/golden/spmv_forms/<case>-<form>.npz: y of every GPU case of
tests/spmv_cases.py through the deterministic SpMV forms (row split, CSR5
plain / 3 panels / host-built descriptors, XCD panels), for beta = 0 (y0
seeded with NaN) and beta != 0.

The committed files were written by the library as it stood BEFORE the CSR5
tile forms and the vec4 row-split order were removed; test_spmv_args_gpu.py
asserts bit equality against them.  Needs a GPU:
    python tests/golden/make_spmv_forms.py        (SBLAS_LIB selects the build)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "s-blas_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sblas  # noqa: E402
import spmv_cases as sc  # noqa: E402


def main():
    out = os.path.join(HERE, "spmv_forms")
    os.makedirs(out, exist_ok=True)
    for name in sc.GPU_CASES:
        case = sc.gpu_case(name)
        for form, algo, opts in sc.GOLDEN_FORMS:
            y_beta0, _ = sc.run_case(torch, sblas, case, algo, opts, 0.0)
            y_beta, _ = sc.run_case(torch, sblas, case, algo, opts, sc.BETA)
            np.savez_compressed(os.path.join(out, f"{name}-{form}.npz"), y_beta0=y_beta0, y_beta=y_beta)
    print("wrote", len(sc.GPU_CASES) * len(sc.GOLDEN_FORMS), "files to", out, "with", sblas.LIB_PATH)


if __name__ == "__main__":
    main()
