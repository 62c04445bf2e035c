"""The xsort planner on the CPU (sblas.xsort_plan_host: no GPU, no handle).

Three kinds of check: the structural invariants every plan must satisfy, the
decisions that follow from the planner's code (group sizing, solo, all-wide),
and a lock to recorded plans: tests/golden/xsort_plan/ holds what the planner
decided on an MI355X (256 CUs) before it became a pure function -- for every
matrix and option set of tests/test_xsort_devplan_gpu.py plus two synthetic
shapes: sblas_csr_xsort_info, the exported wide-range records, the claim
heads and the four leading words of every exported item record (stored as
`sub` per record plus one (rows, pbase, widx) row per range, which is what
those words hold).  The plan's chunk counts ("chunks", "max_item_chunks")
belong to the layout, not the planner, and are not compared.
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_xsort_devplan_gpu import MATRICES, OPT_IDS, OPTS

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "xsort_plan", "*.npz")))
WRANGE = np.dtype([("row0", "<i4"), ("nrows", "<i4"), ("wide", "<i4"), ("widx", "<i4"), ("pbase", "<i8")])
_RP = {}


def rowptr(sb, name):
    """(n, rowptr) of a named shape, generated once."""
    if name not in _RP:
        if name in MATRICES:
            n, rp = MATRICES[name](np.random.default_rng(2024))[:2]
        elif name == "synth2m":
            n, rp = 2_000_000, sb.gen_synth_rowptr(2_000_000)
        elif name == "synth320k":
            n, rp = 320_000, sb.gen_synth_rowptr(320_000)
        elif name == "empty_matrix":
            n, rp = 10, np.zeros(1, np.int64)
        elif name == "wide_n":
            n, rp = 2_200_000, np.arange(2001, dtype=np.int64) * 40
        else:
            raise KeyError(name)
        rp = np.ascontiguousarray(rp, np.int64)
        rp.setflags(write=False)
        _RP[name] = (n, rp)
    return _RP[name]


def check_structure(p, rp, resident):
    m = len(rp) - 1
    R = p["ranges"]
    row0, nrows, wide, widx, pbase = R.T if len(R) else np.zeros((5, 0), np.int64)
    assert p["nranges"] == len(R) and p["nwide"] == int(wide.sum())
    # the ranges tile [0, m) in order
    assert np.all(nrows >= 1)
    assert np.array_equal(row0, np.concatenate([[0], np.cumsum(nrows)[:-1]])) if len(R) else m == 0
    assert int(nrows.sum()) == m
    w = wide == 1
    assert np.all((wide == 0) | w)
    entries = rp[row0 + nrows] - rp[row0]
    assert np.all(nrows[w] <= 8192) and np.all(entries[w] >= 1)
    assert np.all(nrows[~w] <= (16384 if p["solo"] else 8192))
    assert np.array_equal(widx[w], np.arange(w.sum())) and np.all(widx[~w] == -1)
    assert np.array_equal(pbase[w], np.concatenate([[0], np.cumsum(8 * nrows[w])[:-1]])[:w.sum()])
    assert p["partial_len"] == int(8 * nrows[w].sum())
    # the queues hold every sub-item exactly once
    queues = p["queues"]
    assert len(queues) == 8
    want = set()
    for i in np.flatnonzero(w):
        want.update((int(i) << 8) | k for k in range(1, 9))
    want.update(int(i) << 8 for i in np.flatnonzero(~w))
    seen = []
    for k, q in enumerate(queues):
        assert q.shape == (p["qlen"][k], 2)
        assert not np.any((q[:, 0] < 0) & (q[:, 1] < 0))
        subs = q[q >= 0]
        kk = subs & 255
        assert np.all((kk == 0) | (kk == k + 1)), "a wide sub-item sits in its XCD's queue"
        seen.extend(subs.tolist())
        if p["solo"]:
            narrow_first = (q[:, 0] >= 0) & ((q[:, 0] & 255) == 0)
            assert np.all(q[narrow_first, 1] == -1)
    assert len(seen) == len(want) and set(seen) == want
    # queue statistics
    qlen, qstat = p["qlen"], p["qstat"]
    assert p["qstride"] == max(1, int(qlen.max()))
    assert p["nitems"] == int(qlen.sum())
    assert p["grid"] == min(p["nitems"], resident)
    for k in range(8):
        assert qstat[k] == min(qlen[k], sum(1 for b in range(p["grid"]) if b % 8 == k))
    assert p["dynamic"] == int(qstat.sum() < p["nitems"])


def same_plan(a, b):
    for k in a:
        if k == "queues":
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
        else:
            assert np.array_equal(a[k], b[k]), k


CASES = {
    "synth2m": ("synth2m", 256, {}),
    "synth320k": ("synth320k", 256, {}),
    "mostly_empty": ("mostly_empty", 256, {}),
    "unit_rows": ("unit_rows", 256, {}),
    "one_dense_row": ("one_dense_row", 256, {}),
    "empty_matrix": ("empty_matrix", 256, {}),
    "no_entries": ("no_entries", 256, {}),
    "wide_n": ("wide_n", 256, {}),
    "unit_rows_resident4": ("unit_rows", 4, {}),
    "unit_rows_cap50": ("unit_rows", 256, {"cap": 50}),
    "unit_rows_allwide0": ("unit_rows", 256, {"allwide": 0}),
    "unit_rows_solo1": ("unit_rows", 256, {"solo": 1}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_structure(sb, case):
    name, resident, over = CASES[case]
    n, rp = rowptr(sb, name)
    p = sb.xsort_plan_host(rp, n, resident, **over)
    check_structure(p, rp, resident)
    same_plan(p, sb.xsort_plan_host(rp, n, resident, **over))
    m = len(rp) - 1
    if not over:
        empty = int(np.sum(np.diff(rp) == 0))
        assert p["solo"] == int(m > 0 and 5 * empty >= 2 * m)
    if case == "unit_rows_resident4":
        assert p["nitems"] > 4 and p["dynamic"] == 1
    if case == "unit_rows_solo1":
        assert p["solo"] == 1
    if case == "unit_rows_allwide0":
        assert p["nwide"] == 0  # a row holds one entry, a wide range needs 16 a row
    if case == "unit_rows_cap50":
        assert p["nranges"] != sb.xsort_plan_host(rp, n, resident)["nranges"]
    if case == "mostly_empty":
        assert p["solo"] == 1


def test_group_sizing(sb):
    p = sb.xsort_plan_host(rowptr(sb, "synth2m")[1], 2_000_000, 256)
    assert (p["q"], p["G"], p["Wg"]) == (2, 16, 125000)
    n, rp = rowptr(sb, "wide_n")
    p = sb.xsort_plan_host(rp, n, 256)
    assert (p["q"], p["G"]) == (3, 24)
    with pytest.raises(sb.SblasError, match=r"unsupported.*160 column groups"):
        sb.xsort_plan_host(np.zeros(3, np.int64), 20_000_000, 256)


@pytest.mark.parametrize("m,empty,solo", [(10, 4, 1), (10, 3, 0), (5, 2, 1), (5, 1, 0)])
def test_solo_threshold(sb, m, empty, solo):
    lens = np.array([0] * empty + [3] * (m - empty))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert sb.xsort_plan_host(rp, 100, 256)["solo"] == solo


def test_all_wide_limit(sb):
    """Every non-empty range is wide up to 6,000,000 entries; beyond, rows of
    10 entries (< 16) are never wide, nor are the 320,000 shape's light rows."""
    def all_wide(p, rp):
        R = p["ranges"]
        entries = rp[R[:, 0] + R[:, 1]] - rp[R[:, 0]]
        return bool(np.all(R[entries > 0, 2] == 1))

    rp = np.arange(600_001, dtype=np.int64) * 10
    assert rp[-1] == 6_000_000
    assert all_wide(sb.xsort_plan_host(rp, 600_000, 256), rp)
    rp = rp.copy()
    rp[-1] += 1
    p = sb.xsort_plan_host(rp, 600_000, 256)
    assert not all_wide(p, rp) and p["nwide"] == 0
    n, rp = rowptr(sb, "synth320k")
    assert rp[-1] > 6_000_000
    p = sb.xsort_plan_host(rp, n, 256)
    assert not all_wide(p, rp) and 0 < p["nwide"] < p["nranges"]


def test_invalid_arguments(sb):
    info = np.zeros(27, np.int64)
    rp = np.zeros(2, np.int64)
    f = sb.lib.sblas_xsort_plan_host
    assert f(1, 10, None, 256, None, -1, -1, sb.ptr(info), None, 0, None, 0) == 1
    assert f(1, 10, sb.ptr(rp), 256, None, -1, -1, None, None, 0, None, 0) == 1
    assert f(-1, 10, sb.ptr(rp), 256, None, -1, -1, sb.ptr(info), None, 0, None, 0) == 1
    assert f(1, 10, sb.ptr(rp), 256, None, -1, -1, sb.ptr(info), None, 0, None, 0) == 0
    ranges = np.zeros(5, np.int64)
    assert info[4] == 1 and f(1, 10, sb.ptr(rp), 256, None, -1, -1, sb.ptr(info), sb.ptr(ranges), 0, None, 0) == 1


def test_fixtures_cover_every_case():
    want = {f"{m}-{o}" for m in MATRICES for o in OPT_IDS} | {"synth320k-default", "synth2m-default"}
    assert {os.path.basename(p)[:-4] for p in FIXTURES} == want


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_plan_is_the_recorded_plan(sb, path):
    name, oid = os.path.basename(path)[:-4].rsplit("-", 1)
    over = {k[3:]: v for k, v in OPTS[OPT_IDS.index(oid)].items()}  # xs_cap -> cap, ...
    z = np.load(path)
    n, rp = rowptr(sb, name)
    assert n == int(z["n"])
    p = sb.xsort_plan_host(rp, n, int(z["cus"]), **over)
    ready, ranges, wide, items, grid, solo = (int(v) for v in z["info"][:6])
    assert (1, p["nranges"], p["nwide"], p["nitems"], p["grid"], p["solo"]) == (ready, ranges, wide, items, grid,
                                                                               solo)
    R = p["ranges"]
    # the wide ranges' records, byte for byte
    wr = np.zeros(p["nwide"], WRANGE)
    for j, f in enumerate(WRANGE.names):
        wr[f] = R[R[:, 2] == 1, j]
    assert np.array_equal(wr.view(np.uint8), z["wranges"])
    # the item records: word 0 of slot (queue * qstride + index, team), then
    # each range's rows word, pbase and widx
    sub = np.full((8, p["qstride"], 2), -1, np.int32)
    for k, q in enumerate(p["queues"]):
        sub[k, :len(q)] = q
    assert np.array_equal(sub.ravel(), z["sub"])
    assert np.array_equal((R[:, 0] & 0xffffffff) | (R[:, 1] << 32), z["range_rows"])
    assert np.array_equal(R[:, 4], z["range_pbase"])
    assert np.array_equal(R[:, 3], z["range_widx"])
    heads = np.zeros(32, np.int32)
    heads[0:8] = heads[16:24] = p["qstat"]
    assert np.array_equal(heads, z["heads"])
