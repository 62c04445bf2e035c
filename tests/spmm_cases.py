"""The matrices of the SpMM tests, by name, so that the GPU tests and the CPU
test of the SpMM shape (sblas.spmm_shape_host) see the same ones, and the
per-entry bound every SpMM test uses.

spmm_matrix(form, rng)  -> (m, k, rowptr int64, col int32, val f64) of test_spmm
spmm_case(name)         -> dict(m, k, rp, col, val, opts): the named cases
case_shape(name, c, n)  -> the plan a named case must take when built at width n
"""
import numpy as np

from transpose_cases import rand_csr

# test options under which a form's plan is built
FORM_OPTS = {"rowwave": {}, "splitk": {"spmm_mfma_fill": 2}, "ct": {"spmm_ctile": 1}, "ctrows": {"spmm_ctile": 1}}
# form -> (rowform, ctile, nmfma)
FORM_KERNELS = {"rowwave": (1, 0, 0), "splitk": (2, 0, 0), "ct": (0, 1, 0), "ctrows": (0, 1, 0)}


def spmm_bound(rp, col, val, B, alpha, beta, C0):
    u = 2.0 ** -53
    m = len(rp) - 1
    k = np.diff(rp).astype(np.float64)
    gam = (k * u / (1 - k * u))[:, None]
    rows = np.repeat(np.arange(m), np.diff(rp))
    S = np.zeros((m, B.shape[1]))
    np.add.at(S, rows, np.abs(alpha * val[:, None] * B[col, :]))
    return 4 * gam * S + 4 * u * np.abs(beta * C0) + 1e-300


def spmm_matrix(form, rng):
    """test_spmm's matrix of a form (draws from rng; B and C0 follow from the same rng)"""
    m, k = {"ctrows": 2500, "splitk": 60}.get(form, 700), 5000
    rp, col, val = rand_csr(rng, m, k, 2000 if form == "splitk" else 50, long_rows=[(3, 3000)])
    return m, k, rp, col, val


def _csr(rows, rng):
    lens = np.array([len(r) for r in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = (np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(0, np.int32))
    return rp, col, rng.standard_normal(int(rp[-1]))


def block_dense_csr(rng, nblk, width, k, sparse_tail=0):
    """16-row blocks, each dense over `width` random columns (MFMA path), plus
    `sparse_tail` random sparse rows (row-wave path)."""
    rows = []
    for _ in range(nblk):
        cols = np.sort(rng.choice(k, width, replace=False))
        for _ in range(16):
            keep = cols[rng.random(width) < 0.9]  # ~90% fill
            rows.append(keep)
    for _ in range(sparse_tail):
        rows.append(np.sort(rng.choice(k, 20, replace=False)))
    lens = np.array([len(r) for r in rows])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    return rp, col, rng.standard_normal(int(rp[-1]))


def unsorted_dups(rng, m, k, lo, hi, dup=0.2):
    """rows of lo..hi entries in random order, about `dup` of them repeats of a
    column the row already has"""
    rows = []
    for _ in range(m):
        L = int(rng.integers(lo, hi))
        nd = int(round(L * dup)) if L > 1 else 0
        c = rng.choice(k, L - nd, replace=False)
        c = np.concatenate([c, rng.choice(c, nd)]) if nd else c
        rows.append(rng.permutation(c))
    return rows


K_NONDIRECT = (1 << 21) + 4096 + 37   # 1026 whole slabs of 2048 columns and one of 37
K_UNSUPPORTED = (1 << 24) + (1 << 14) + 1

# the five forms of the argument tests -> the named case that gives the matrix
FORMS = ["rowwave", "splitk", "mfma", "ctfast", "ctslow"]
FORM_CASE = {"rowwave": "rowwave", "splitk": "splitk", "mfma": "mfma", "ctfast": "ct", "ctslow": "ctrows"}
DUP_CASE = {"rowwave": "dup_rowwave", "splitk": "dup_splitk", "mfma": "dup_mfma", "ctfast": "dup_ct",
            "ctslow": "dup_ct"}

CASES = ["rowwave", "splitk", "mfma", "ct", "ctrows", "splitk_mfma", "nondirect", "unsupported", "dup_rowwave",
         "dup_splitk", "dup_mfma", "dup_ct", "empty_tail"]


def spmm_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    k, opts = 5000, {}
    if name == "rowwave":
        rp, col, val = rand_csr(rng, 300, k, 50, long_rows=[(3, 3000)])
    elif name == "splitk":  # 60 rows of ~1,000: long rows on average; the fill rule is switched off
        rp, col, val = rand_csr(rng, 60, k, 2000, long_rows=[(3, 3000)])
        opts = {"spmm_mfma_fill": 2}
    elif name == "mfma":  # 4 MFMA blocks and 21 sparse rows (m = 85: a partial last block)
        rp, col, val = block_dense_csr(rng, 4, 37, k, sparse_tail=21)
    elif name == "ct":  # one row block, 3 slabs
        rp, col, val = rand_csr(rng, 700, k, 50, long_rows=[(3, 3000)])
        opts = {"spmm_ctile": 1}
    elif name == "ctrows":  # 3 row blocks of 834
        rp, col, val = rand_csr(rng, 2500, k, 50, long_rows=[(3, 3000)])
        opts = {"spmm_ctile": 1}
    elif name == "splitk_mfma":  # 3 MFMA blocks, then 20 rows of 300 distinct columns: split-k through rows[]
        k = 200_000
        rp, col, val = block_dense_csr(rng, 3, 37, k)
        rows = [col[rp[r]:rp[r + 1]] for r in range(48)]
        rows += [np.sort(rng.choice(k, 300, replace=False)) for _ in range(20)]
        rp, col, val = _csr(rows, rng)
    elif name == "nondirect":
        # m = 1,100 (one row block, rbits 11) over k > 2^21 columns: keys hold XCD-local columns.
        # 200 columns in each of 19 slabs: every residue s % 8 twice (slabs 0-7, 512-519), the last
        # whole slabs (1024, 1025) and the partial one (1026, all its 37); 27 entries per row out of
        # those 3,637 columns, so every column is shared by ~8 rows of the tile while a 16-row
        # block still has ~407 distinct columns for its 432 entries (not dense: 432 < 1.28 * 407)
        k = K_NONDIRECT
        pool = []
        for s in list(range(8)) + list(range(512, 520)) + [1024, 1025, 1026]:
            w = min(2048, k - s * 2048)
            pool.append(s * 2048 + np.sort(rng.choice(w, min(200, w), replace=False)))
        pool = np.concatenate(pool)
        pool[0], pool[-1] = 0, k - 1  # the first and the last column of B
        rp, col, val = _csr([np.sort(rng.choice(pool, 27, replace=False)) for _ in range(1100)], rng)
        opts = {"spmm_ctile": 1}
    elif name == "unsupported":  # XCD-local columns beyond 2^21 at rbits 11: the row kernels serve it
        k = K_UNSUPPORTED
        pool = np.concatenate([[0, k - 1], rng.choice(k, 500, replace=False)])
        rp, col, val = _csr([np.sort(rng.choice(pool, 12, replace=False)) for _ in range(1100)], rng)
        opts = {"spmm_ctile": 1}
    elif name == "dup_rowwave":
        rp, col, val = _csr(unsorted_dups(rng, 150, k, 0, 80, dup=0.1), rng)
    elif name == "dup_splitk":
        rp, col, val = _csr(unsorted_dups(rng, 40, k, 200, 600, dup=0.3), rng)
        opts = {"spmm_mfma_fill": 2}
    elif name == "dup_mfma":
        # block 0: 16 rows of 4 entries, each one column 4 times: 64 entries over 16 distinct columns
        # (dense, 64 >= 1.28 * 16) where the 16 distinct entries alone are not (16 < 20.48);
        # blocks 1-2: block-dense with shuffled rows and repeats; then 20 sparse rows
        rows = [np.full(4, c) for c in rng.choice(k, 16, replace=False)]
        for _ in range(2):
            cols = rng.choice(k, 37, replace=False)
            for _ in range(16):
                keep = cols[rng.random(37) < 0.8]
                rows.append(rng.permutation(np.concatenate([keep, rng.choice(keep, 6)])))
        rows += unsorted_dups(rng, 20, k, 5, 30, dup=0.1)
        rp, col, val = _csr(rows, rng)
    elif name == "dup_ct":
        rp, col, val = _csr(unsorted_dups(rng, 700, k, 0, 60, dup=0.1), rng)
        opts = {"spmm_ctile": 1}
    elif name == "empty_tail":  # the last 40 rows are empty
        rp, col, val = rand_csr(rng, 100, k, 50)
        rp, col, val = np.concatenate([rp, np.full(40, rp[-1])]), col, val
    else:
        raise KeyError(name)
    return dict(m=len(rp) - 1, k=k, rp=rp, col=col, val=val, opts=opts)


def _plan(nmfma, nsparse, sparse_nnz, rowform, ct=None, ct_supported=1):
    """ct = (ns, nrb, R, rbits, wlog, direct) of a C-tile plan"""
    d = dict(nmfma=nmfma, nsparse=nsparse, sparse_nnz=sparse_nnz, rowform=rowform, ctile=int(ct is not None),
             ct_supported=ct_supported, ns=0, nrb=0, R=0, rbits=0, wlog=0, direct=0)
    if ct:
        d.update(zip(("ns", "nrb", "R", "rbits", "wlog", "direct"), ct))
    return d


PLAN_KEYS = tuple(_plan(0, 0, 0, 0))


def case_shape(name, c, n_plan=16):
    """The plan a case must take when built at width n_plan, from the rules of
    include/sblas.h (sblas_spmm_shape_host) and the case's construction."""
    m, nnz = c["m"], int(c["rp"][-1])
    ncg = -(-n_plan // 16)
    if name in ("rowwave", "dup_rowwave", "empty_tail"):
        return _plan(0, m, nnz, 1)
    if name in ("splitk", "dup_splitk"):
        return _plan(0, m, nnz, 2)
    if name == "mfma":  # 4 blocks of 16 rows on MFMA, 21 rows of 20 entries beside them
        return _plan(4, 21, 21 * 20, 1)
    if name == "splitk_mfma":  # 6,000 >= 256 * 20
        return _plan(3, 20, 20 * 300, 2)
    if name == "dup_mfma":
        return _plan(3, 20, int(c["rp"][-1] - c["rp"][48]), 1)
    if name in ("ct", "dup_ct"):  # R = 700 < 2^10; direct: 5000 <= 2^22
        return _plan(0, m, nnz, 0, (max(1, 32 // ncg), 1, 700, 10, 11, 1))
    if name == "ctrows":  # ceil(2500 / 1204) = 3 blocks of ceil(2500 / 3) = 834 rows
        return _plan(0, m, nnz, 0, (max(1, 32 // (3 * ncg)), 3, 834, 10, 11, 1))
    if name == "nondirect":  # R = 1100 <= 2^11; k > 2^21: not direct; 129 slabs per XCD x 2048 <= 2^21
        return _plan(0, m, nnz, 0, (max(1, 32 // ncg), 1, 1100, 11, 11, 0))
    if name == "unsupported":  # 8,201 slabs: 1,026 per XCD x 2048 > 2^21; 12 entries per row: wave per row
        return _plan(0, m, nnz, 1, None, ct_supported=0)
    raise KeyError(name)
