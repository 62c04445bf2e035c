"""The matrices of the transpose tests, by name, so that the GPU tests and the
CPU test of the pass shape (sblas.transpose_shape_host) see the same ones.

transpose_case(sb, name, seed) -> (m, n, rowptr int64, col int32, val f64)
transpose_edge(name)           -> the same, the edge shapes (n = 5000)
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = ["qh768", "ash85", "random", "longcols", "wide", "big", "shortrows", "sparserows", "hugecols",
         "narrow2tiles", "manyrows"]
MGPU_CASES = ["qh768", "ash85", "random", "longcols", "wide"]
EDGES = ["one_entry", "one_row", "one_col_tall", "last_col", "tile_edge", "dup_free_dense_row", "empty_tail_rows"]


def rand_csr(rng, m, n, maxlen, empty_frac=0.1, long_rows=()):
    lens = rng.integers(0, maxlen, m)
    lens[rng.random(m) < empty_frac] = 0
    for r, L in long_rows:
        lens[r] = L
    lens = np.minimum(lens, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = (np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
           if rp[-1] else np.zeros(0, np.int32))
    return rp, col, rng.standard_normal(int(rp[-1]))


def _from_lens(rng, lens, n):
    """rows of lens[r] distinct sorted columns each (rows beyond lens are empty)"""
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
    return rp, col, rng.standard_normal(int(rp[-1]))


def transpose_case(sb, name, seed=5):
    rng = np.random.default_rng(seed)
    if name in ("qh768", "ash85"):
        return sb.mm_read(os.path.join(GOLDEN, f"{name}.mtx"), 0)
    if name == "random":
        m, n = 3000, 2500
        rp, col, val = rand_csr(rng, m, n, 30)
    elif name == "big":  # 2.2M nonzeros over 3M columns: 2 tiles per workgroup
        m, n = 110000, 3_000_000
        rp, col, val = _from_lens(rng, rng.integers(0, 40, m), n)
    elif name == "shortrows":  # 0-3 entries per row, half the rows empty: a 4096-entry tile
        # holds thousands of row starts (pass A's row derivation takes several windows)
        m, n = 200000, 5000
        rp, col, val = _from_lens(rng, rng.integers(0, 4, m) * (rng.random(m) < 0.5), n)
    elif name == "sparserows":  # 2^24 columns (16 key bits past pass A) and one row in 100
        # non-empty: a segment spans > 2^16 rows, so pass A cannot pack the row offset
        m, n = 300000, 1 << 24
        rp, col, val = _from_lens(rng, np.where(rng.random(m) < 0.01, 5, 0), n)
    elif name == "wide":  # more columns than rows, many empty columns
        m, n = 50, 100000
        rp, col, val = rand_csr(rng, m, n, 400, empty_frac=0.3)
    elif name == "longcols":  # 40 columns of ~3,500 entries: few, long final buckets
        m, n = 9000, 40
        rp, col, val = rand_csr(rng, m, n, 40, empty_frac=0.2)
    elif name == "hugecols":  # n > 2^24: pass A would need 9 bits, so 4 LSD passes over 5 tiles
        m, n = 4000, (1 << 24) + 1
        rp, col, val = _from_lens(rng, np.full(m, 5), n)
    elif name == "narrow2tiles":  # n <= 512 and more than one tile: 2 LSD passes over 2 tiles
        m, n = 2000, 300
        rp, col, val = _from_lens(rng, np.full(m, 3), n)
    elif name == "manyrows":  # 24 row bits + 8 column bits exceed a word: pass B hands the
        # last pass keys and rows apart
        m, n, filled = (1 << 23) + 5, 5000, 20000
        rp, col, val = _from_lens(rng, np.full(filled, 3), n)
        rp = np.concatenate([rp, np.full(m - filled, rp[-1], np.int64)])
    else:
        raise KeyError(name)
    return m, n, rp, col, val


def transpose_edge(name):
    rng = np.random.default_rng(7)
    n = 5000
    if name == "one_entry":
        m = 3
        rp = np.array([0, 0, 1, 1], np.int64)
        col = np.array([4321], np.int32)
    elif name == "one_row":
        m = 1
        col = np.sort(rng.choice(n, 3000, replace=False)).astype(np.int32)
        rp = np.array([0, len(col)], np.int64)
    elif name == "one_col_tall":
        m = 20000
        rp = np.arange(m + 1, dtype=np.int64)
        col = np.full(m, 777, np.int32)
    elif name == "last_col":
        m = 4096
        rp = np.arange(m + 1, dtype=np.int64)
        col = np.full(m, n - 1, np.int32)
    elif name == "tile_edge":  # 4097 nonzeros: one full tile and one entry
        m = 4097
        rp = np.arange(m + 1, dtype=np.int64)
        col = rng.integers(0, n, m).astype(np.int32)
    elif name == "dup_free_dense_row":  # every column of one row, then sparse rows
        m = 700
        lens = np.concatenate([[n], rng.integers(0, 5, m - 1)])
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = np.concatenate([np.arange(n)] + [np.sort(rng.choice(n, L, replace=False)) for L in lens[1:]]).astype(np.int32)
    elif name == "empty_tail_rows":
        m = 50000
        lens = np.concatenate([rng.integers(1, 6, 1000), np.zeros(m - 1000, np.int64)])
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens[:1000]]).astype(np.int32)
    else:
        raise KeyError(name)
    return m, n, rp, col, rng.standard_normal(len(col))
