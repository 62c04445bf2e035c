"""The systems of the triangular-solve tests, by name, so that the GPU tests
and the CPU test of the solve shape (sblas.trsv_shape_host,
sblas.trsv_levels_host) see the same ones.  Every system here is a CSC
triangle with the diagonal first (lower, substitution 0) / last (upper,
substitution 1) in each column.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NCU = 256  # CUs of an MI355X: the ncu of the expected shapes


def kat(name, sub):
    """the reference's known-answer systems: (colptr, rowidx, val, b, x_ref)"""
    g = np.load(os.path.join(GOLDEN, f"trsv_{name}_{sub}.npz"))
    return g["colptr"], g["rowidx"], g["val"], g["b"], g["x_ref"]


def _banded_system(sb, n, seed=11):
    cp, ri, v = sb.gen_lower_banded(n, 4, 5000, seed)
    xref = np.floor(sb.gen_vector(n, seed + 1) * 10.0) + 1.0
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    b = np.bincount(ri, weights=v * xref[cols], minlength=n)
    return cp, ri, v, b, xref


def csc_matmat(cp, ri, cv, X):
    """B = L X for CSC L (exact for the integer KAT systems)."""
    B = np.zeros_like(X)
    for c in range(len(cp) - 1):
        s, e = cp[c], cp[c + 1]
        B[ri[s:e]] += cv[s:e, None] * X[c][None, :]
    return B


def schedule_system(shape, sub):
    """"chain" = a bidiagonal system (n levels of one row), "wide" = a
    diagonal-heavy system with a few long dependency columns (levels of more
    than 2,048 rows); integer values and solution: (cp, ri, cv, b, xref)"""
    rng = np.random.default_rng(17 + sub)
    n = 5000 if shape == "chain" else 60000
    cols, rows = [], []
    for c in range(n):
        deps = []
        if shape == "chain":
            if (sub == 0 and c + 1 < n) or (sub == 1 and c > 0):
                deps = [c + 1 if sub == 0 else c - 1]
        else:
            lo, hi = (c + 1, min(n, c + 4000)) if sub == 0 else (max(0, c - 4000), c)
            if hi > lo and rng.random() < 0.3:
                deps = sorted(set(rng.integers(lo, hi, 2).tolist()))
        rr = [c] + deps if sub == 0 else deps + [c]
        rows.append(rr)
    cp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ri = np.concatenate(rows).astype(np.int32)
    cv = rng.integers(1, 4, len(ri)).astype(np.float64)
    diag_pos = cp[:-1] if sub == 0 else cp[1:] - 1
    cv[diag_pos] = 1.0
    xref = rng.integers(-3, 4, n).astype(np.float64)
    colidx = np.repeat(np.arange(n), np.diff(cp))
    b = np.bincount(ri, weights=cv * xref[colidx], minlength=n)
    return cp, ri, cv, b, xref


def from_deps(n, deps, sub=0, seed=3):
    """Integer system from dependencies: deps[i] = the rows that row i waits
    for (smaller than i forward, larger backward).  Unit diagonal,
    off-diagonals in 1..3, integer x: (cp, ri, cv, b, xref), all exact."""
    rng = np.random.default_rng(seed)
    cols = [[] for _ in range(n)]  # column c: the rows that depend on row c
    for i, ds in enumerate(deps):
        for c in ds:
            assert (c < i) if sub == 0 else (c > i)
            cols[c].append(i)
    rows = [[c] + sorted(r) if sub == 0 else sorted(r) + [c] for c, r in enumerate(cols)]
    cp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ri = np.concatenate(rows).astype(np.int32)
    cv = rng.integers(1, 4, len(ri)).astype(np.float64)
    cv[cp[:-1] if sub == 0 else cp[1:] - 1] = 1.0
    xref = rng.integers(-3, 4, n).astype(np.float64)
    colidx = np.repeat(np.arange(n), np.diff(cp))
    b = np.bincount(ri, weights=cv * xref[colidx], minlength=n)
    return cp, ri, cv, b, xref


def chain_system(n, sub):
    """bidiagonal: every row depends on the previous one of the solve order"""
    if sub == 0:
        return from_deps(n, [[i - 1] if i else [] for i in range(n)], 0)
    return from_deps(n, [[i + 1] if i + 1 < n else [] for i in range(n)], 1)


def one_level_then_row(width):
    """`width` diagonal-only rows, then one row depending on row 0: a level of
    `width` rows and a level of one"""
    return from_deps(width + 1, [[] for _ in range(width)] + [[0]])


def three_run_system():
    """2,049 diagonal-only rows, one row depending on row 0, 2,049 rows
    depending on that row: n = 4,099, levels of 2,049 / 1 / 2,049 rows, so the
    level-set executor runs wide, narrow, wide"""
    w = 2049
    return from_deps(2 * w + 1, [[] for _ in range(w)] + [[0]] + [[w] for _ in range(w)])
