#!/usr/bin/env python3
"""Per-CU request model of the xsort SpMV on config 2's row structure, used to
read the layout experiments of DESIGN.md §6.

The plan is the real planner's: sblas.xsort_plan_host (csrc/xsort_plan.cpp)
returns the ranges and the items of every XCD queue, and this tool counts for
every item (what one workgroup = one CU runs) its L1->L2 line requests: the x
lines its gathers touch (uniform columns: L (1 - exp(-c / L)) per block) plus
the 128-B lines of its entry stream (12 B per entry).  Items are dealt to the
CUs in queue order (greedy, as the persistent grid claims them); the model
time is the busiest CU's requests x CYCLES_PER_REQUEST / clock.

Until the planner became callable from the CPU this tool carried its own copy
of it, with what-if modes the real planner cannot express (unpaired items,
pairing "always", light ranges split by columns, other row caps and lambdas).
Their results are recorded in profiles/r03 .. r05; that version of the tool is
in the repository's history.

No GPU needed.  Usage: python3 xs_plan_model.py [--n 2000000] [--world 1]
"""
import argparse
import heapq
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sblas  # noqa: E402

CUS = 256
CLOCK = 2.4e9
CYCLES_PER_REQUEST = 4.0  # calibrated on the default layout at N = 1 (131 us)


def config2_rowptr(n, heavy=96, light=9, world=1):
    """Row lengths of rank 0's cyclic share (sblas_dist.make_cyclic_plan:
    8*world equal chunks, chunk j to rank j % world)."""
    lens = np.where(np.arange(n) < n // 8, heavy, light).astype(np.int64)
    if world > 1:
        nch = 8 * world
        cr = (n + nch - 1) // nch
        keep = np.zeros(n, bool)
        for j in range(0, nch, world):
            keep[j * cr:min(n, (j + 1) * cr)] = True
        lens = lens[keep]
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp


def plan(rp, n, mode=None, wstar=None, k=1, allwide=None):
    """mode: "paired" / "solo" force the planner's solo choice, None leaves it
    to the planner; wstar fixes the sub-item cost; k workgroups per CU."""
    p = sblas.xsort_plan_host(rp, n, CUS * k, cap=wstar, allwide=allwide,
                              solo=None if mode is None else mode == "solo")
    q, G = p["q"], p["G"]
    Lg = max(1.0, p["Wg"] / 16.0)
    R = p["ranges"]
    cnt = (rp[R[:, 0] + R[:, 1]] - rp[R[:, 0]]).tolist()  # entries per range

    def req(sub):
        """requests of sub-item range << 8 | k (-1: none)"""
        if sub < 0:
            return 0.0
        wide = (sub & 255) != 0
        L = q * Lg if wide else G * Lg
        c = cnt[sub >> 8] / 8.0 if wide else cnt[sub >> 8]
        return L * (1 - math.exp(-c / L)) + c * 12 / 128

    queues = [[req(int(a)) + req(int(b)) for a, b in items] for items in p["queues"]]
    if os.environ.get("XS_MODEL_DEBUG"):
        print("queue totals (k req):", [round(sum(qq) / 1e3) for qq in queues],
              "items:", [len(qq) for qq in queues], "largest items (k):",
              sorted((round(v / 1e3, 1) for qq in queues for v in qq), reverse=True)[:6],
              "wide ranges:", p["nwide"], "narrow:", p["nranges"] - p["nwide"])
    # 32 CUs per XCD claim from their own queue first (greedy list schedule)
    busiest = 0.0
    for qq in queues:
        heap = [0.0] * (CUS // 8)
        for v in qq:
            heapq.heappush(heap, heapq.heappop(heap) + v)
        busiest = max(busiest, max(heap))
    total_req = sum(map(sum, queues))
    return {"mode": "solo" if p["solo"] else "paired", "max_range_rows": int(R[:, 1].max()) if len(R) else 0,
            "narrow": p["nranges"] - p["nwide"], "wide_ranges": p["nwide"],
            "items": p["nitems"], "requests_M": round(total_req / 1e6, 2),
            "busiest_cu_k": round(busiest / 1e3, 1),
            # perfect balance: the chip's requests spread evenly over the CUs
            "balanced_k": round(total_req / CUS / 1e3, 1),
            "model_us": round(busiest * CYCLES_PER_REQUEST / CLOCK * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--rmat", type=int, default=0, help="model an R-MAT graph of this scale instead")
    args = ap.parse_args()
    if args.rmat:
        rp, _, _ = sblas.gen_rmat(args.rmat, 16, seed=50)
        print(plan(rp, len(rp) - 1))
        return
    rp = config2_rowptr(args.n, world=args.world)
    for mode in ("paired", "solo"):
        print(plan(rp, args.n, mode))


if __name__ == "__main__":
    main()
