#!/usr/bin/env python3
"""Cost of new values on an analysed handle: sblas_csr_set_values against the
route callers had before it (destroy, sblas_csr_from_device, analyse again),
in one process on one GPU.

The matrix is bench.py's (--matrix synth|rmat|stencil27 with --nrows / --scale
/ --grid; the defaults are config 2).  Per algorithm in XSORT, CSR5, PANEL,
ROWSPLIT, on a handle made from device arrays and analysed:
  first_call_s      wall seconds of the first set_values (it builds the maps)
  map_bytes         what the maps hold afterwards
  steady_ms         device span of a later set_values: stream events around
                    the call, the best of --reps, and every single one
  route_s           wall seconds of close + from_device + analyse with the new
                    values (best of --reps, and every one)
  bytes_moved       what the refresh must read and write (d_val and the CSR
                    values once each; per mapped layout the map, the gathered
                    values and the stored slots; CSR5's plain tiles without a map)
  copy_probe_ms     sblas_hbm_probe_timed mode 2 moving the same number of bytes
  identical         the refreshed handle against a fresh one: XSORT's exports
                    0-3 byte for byte (and y in deterministic mode), the other
                    algorithms' y bit for bit
Prints one JSON line; `layout_identical` is the XSORT comparison.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--reps", type=int, default=5, help="steady-state calls and route round trips per algorithm")
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
    m, nnz = len(rp) - 1, int(rp[-1])
    rng = np.random.default_rng(11)
    drp = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).cuda()
    dcol = torch.from_numpy(np.ascontiguousarray(col, np.int32)).cuda()
    dval = [torch.from_numpy(np.ascontiguousarray(val, np.float64)).cuda()]
    dval += [torch.from_numpy(rng.standard_normal(nnz)).cuda() for _ in range(2)]
    xd = torch.from_numpy(rng.standard_normal(n)).cuda()
    y0 = torch.from_numpy(rng.standard_normal(m)).cuda()
    # the copy probe's src | dst: room for the most any algorithm moves (~37 B per entry)
    scratch = torch.zeros(5 * nnz + 4096, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def handle(algo, v):
        A = sblas.DeviceCSR.from_device(0, m, n, nnz, drp.data_ptr(), dcol.data_ptr(), v.data_ptr())
        A.analyse(algo)
        torch.cuda.synchronize()
        return A

    def y_of(A, algo):
        y = y0.clone()
        A.spmv(algo, 1.25, xd.data_ptr(), 0.75, y.data_ptr())
        torch.cuda.synchronize()
        return y.cpu().numpy()

    out = {"tool": "bench_set_values", "matrix": what, "n": n, "nnz": nnz, "reps": args.reps}
    for name, algo in (("xsort", sblas.XSORT), ("csr5", sblas.CSR5), ("panel", sblas.PANEL),
                       ("rowsplit", sblas.ROWSPLIT)):
        A = handle(algo, dval[0])
        t0 = time.perf_counter()
        A.set_values(dval[1].data_ptr())
        torch.cuda.synchronize()
        first_s = time.perf_counter() - t0
        vi = A.values_info()
        steady = []
        for r in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            A.set_values(dval[1 + (r + 1) % 2].data_ptr())
            e1.record()
            e1.synchronize()
            steady.append(e0.elapsed_time(e1))
        last = dval[1 + args.reps % 2]  # the values A holds now
        F = handle(algo, last)
        if algo == sblas.XSORT:
            same = all(a.shape == b.shape and np.array_equal(a, b)
                       for a, b in zip((A.xsort_export(w) for w in range(4)), (F.xsort_export(w) for w in range(4))))
            same = same and A.xsort_info() == F.xsort_info()
            A.deterministic = F.deterministic = True
        else:
            same = True
        same = bool(same and np.array_equal(y_of(A, algo), y_of(F, algo)))
        panels = A.panels(algo)
        F.close()
        route = []
        for r in range(args.reps):
            t0 = time.perf_counter()
            A.close()
            A = sblas.DeviceCSR.from_device(0, m, n, nnz, drp.data_ptr(), dcol.data_ptr(), dval[r % 3].data_ptr())
            A.analyse(algo)
            torch.cuda.synchronize()
            route.append(time.perf_counter() - t0)
        A.close()
        # d_val read + CSR values written; per mapped slot 4 B of map and 8 B stored, 8 B gathered per entry
        slots = vi["map_bytes"] // 4
        moved = 16 * nnz
        if slots:
            moved += 4 * slots + 8 * nnz + 8 * slots
        elif algo == sblas.CSR5:  # plain tiles: the values read again, the tiles written
            moved += 8 * nnz + 8 * ((nnz + 1023) // 1024 * 1024)
        half = (moved // 2 + 15) // 16 * 16  # a copy of `half` bytes moves 2 * half
        assert 2 * half <= scratch.numel() * 8
        probe = min(sblas.hbm_probe_timed(2, scratch.data_ptr(), scratch.data_ptr() + half, half)
                    for _ in range(args.reps))
        best = min(steady)
        out[name] = {
            "panels": panels, "first_call_s": round(first_s, 6), "map_build_s": round(vi["map_build_s"], 6),
            "map_bytes": vi["map_bytes"], "map_algos": vi["map_algos"], "rebuilt": vi["rebuilt"],
            "steady_ms": round(best, 4), "steady_ms_all": [round(t, 4) for t in steady],
            "route_s": round(min(route), 6), "route_s_all": [round(t, 6) for t in route],
            "route_over_steady": round(min(route) * 1e3 / best, 1) if best > 0 else None,
            "bytes_moved": moved, "bytes_per_entry": round(moved / max(nnz, 1), 2),
            "copy_probe_ms": None if probe is None else round(probe, 4),
            "fraction_of_copy_rate": None if probe is None or best <= 0 else round(probe / best, 3),
            "identical": same}
    out["layout_identical"] = out["xsort"]["identical"]
    out["all_identical"] = all(out[k]["identical"] for k in ("xsort", "csr5", "panel", "rowsplit"))
    print(json.dumps(out))
    return 0 if out["all_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
