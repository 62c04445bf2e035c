#!/usr/bin/env python3
"""Build time of the xsort SpMV layout: the device inspector against the
host inspector, in one process on one GPU.

The matrix is bench.py's (--matrix synth|rmat|stencil27 with --nrows / --scale
/ --grid).  The plan is built on fresh handles, first under the test option
"xs_hostplan" (the host build: entries copied back, sorted under OpenMP,
copied up), then by default (the device build); all four plan buffers
(sblas_csr_xsort_export) are compared byte for byte.  Prints one JSON line:
both build times (wall seconds, analysis entry to ready: the best of --reps
builds and every single one), the device build's scratch and device->host
bytes, their ratio and `layout_identical`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["synth", "rmat", "stencil27"], default="synth")
    ap.add_argument("--nrows", type=int, default=2_000_000)
    ap.add_argument("--heavy", type=int, default=96)
    ap.add_argument("--light", type=int, default=9)
    ap.add_argument("--scale", type=int, default=21, help="R-MAT scale (n = 2^scale)")
    ap.add_argument("--grid", type=int, default=160, help="stencil mesh edge (n = grid^3)")
    ap.add_argument("--reps", type=int, default=3, help="builds per inspector (fresh handle each)")
    args = ap.parse_args()

    import torch
    import sblas

    assert torch.cuda.is_available(), "needs a GPU"
    if args.matrix == "synth":
        n = args.nrows
        rp = sblas.gen_synth_rowptr(n, args.heavy, args.light)
        col, val = sblas.gen_synth_rows(n, rp, 0, n, args.heavy, args.light, seed=42)
        what = f"synth n={n} heavy={args.heavy} light={args.light}"
    elif args.matrix == "rmat":
        rp, col, val = sblas.gen_rmat(args.scale, 16, seed=50)
        n = len(rp) - 1
        what = f"rmat scale={args.scale}"
    else:
        g = args.grid
        rp, col, val = sblas.gen_stencil3d(g, g, g, 27, seed=49)
        n = len(rp) - 1
        what = f"stencil27 grid={g}"
    nnz = int(rp[-1])

    def build(host: bool):
        """-> (build infos of every rep, the last handle's exports, shape, plan bytes)"""
        infos, keep = [], None
        for _ in range(args.reps):
            A = sblas.DeviceCSR.upload(0, n, rp, col, val)
            with sblas.test_options(**({"xs_hostplan": 1} if host else {})):
                A.analyse(sblas.XSORT)
            infos.append(A.xsort_build_info())
            if keep is not None:
                keep.close()
            keep = A
        out = ([keep.xsort_export(w) for w in range(4)], keep.xsort_info(), keep.plan_bytes(sblas.XSORT))
        keep.close()
        return (infos,) + out

    hi, he, hshape, hbytes = build(True)
    di, de, dshape, dbytes = build(False)
    same = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(he, de))
    same = same and hshape == dshape and hbytes == dbytes
    hs = min(i.build_s for i in hi)
    ds = min(i.build_s for i in di)
    print(json.dumps({
        "tool": "bench_xsort_plan", "matrix": what, "n": n, "nnz": nnz,
        "host_build_s": round(hs, 6), "device_build_s": round(ds, 6),
        "host_over_device": round(hs / ds, 2) if ds > 0 else None,
        "host_build_s_all": [round(i.build_s, 6) for i in hi],
        "device_build_s_all": [round(i.build_s, 6) for i in di],
        "host_built": [not i.device_built for i in hi] == [True] * args.reps,
        "device_built": all(i.device_built for i in di),
        "scratch_bytes": di[-1].scratch_bytes, "scratch_bytes_per_entry": round(di[-1].scratch_bytes / max(nnz, 1), 2),
        "d2h_bytes": di[-1].d2h_bytes, "host_d2h_bytes": hi[-1].d2h_bytes,
        "plan_bytes": dbytes, "chunks": dshape["chunks"], "ranges": dshape["ranges"],
        "layout_identical": bool(same)}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
