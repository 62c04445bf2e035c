"""Shared CSR SpMV cases: the small matrices of test_spmv_args_gpu.py (and of
the parent-golden vectors under golden/spmv_forms/), the generators
test_spmv_gpu.py compares CSR5's two descriptor builders on, and the numpy
restatements test_spmv_shape_cpu.py checks the host functions against.

Constants restated from the library (csrc/spmv_shape.hpp): a stream block
holds <= 2048 entries and <= 1024 rows, a long row is cut into 8192-entry
chunks, a CSR5 tile is 64 lanes x 16 entries."""
import numpy as np

BLOCK_NNZ, BLOCK_ROWS, LONG_CHUNK = 2048, 1024, 8192
TILE, SIGMA = 1024, 16

# ---------------------------------------------------------------------------
# generators moved from test_spmv_gpu.py (same draws from the caller's rng)
# ---------------------------------------------------------------------------


def random_csr(rng, m, n, density_rows, long_rows=(), empty_frac=0.1):
    lens = rng.integers(0, density_rows, size=m)
    lens[rng.random(m) < empty_frac] = 0
    for r, L in long_rows:
        lens[r] = L
    lens = np.minimum(lens, n)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lens]
                         ).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    val = rng.standard_normal(int(rp[-1]))
    return rp, col, val


def _from_lens(rng, lens, n):
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens]).astype(np.int32)
    val = rng.standard_normal(int(rp[-1]))
    return rp, col, val


def ragged(rng):
    m, n = 3000, 40000
    return (m, n) + random_csr(rng, m, n, 60, long_rows=[(5, 2049), (17, 8192), (900, 30000)])


def empty_runs(rng):
    """long runs of empty rows inside and across tiles"""
    m, n = 20000, 5000
    lens = np.zeros(m, np.int64)
    live = rng.choice(m, 900, replace=False)
    lens[live] = rng.integers(1, 40, 900)
    lens[-1] = 3000
    return (m, n) + _from_lens(rng, lens, n)


def tile_rows(rng):
    """rows of exactly one tile, and of 1 / 16 entries"""
    m, n = 600, 3000
    lens = rng.choice([1, 16, 1024, 0], m)
    return (m, n) + _from_lens(rng, lens, n)


# ---------------------------------------------------------------------------
# GPU cases: row lengths per case; columns leave the middle third of x (and
# column 0) unused, so a split into 3 column panels has an empty panel, or
# ("first") stay in the first third, so only one panel is live.
# ---------------------------------------------------------------------------
N_COLS = 30000
ALPHA, BETA = 1.25, 0.75


def _rows_one_block(k):
    base = min(BLOCK_NNZ // k, 40)
    lens = [1 + (7 * i + 36) % base for i in range(k)]
    if k >= 4:
        lens[1] = 0
    return lens


STREAM_ROWS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 1024)

GPU_LENS = {f"rows{k}": _rows_one_block(k) for k in STREAM_ROWS}
GPU_LENS.update({
    "block2048": [300] * 6 + [248, 5],          # a stream block of exactly 2048 entries
    "unaligned": [2047, 3, 5, 7, 2, 0, 9],      # second block's first entry is 2047
    "long2049": [2049],                         # single chunk, writes y itself
    "long2049_off": [3, 2049, 2],               # the same from entry 3 (backwards over-read)
    "long8192": [1, 8192],
    "long8193": [8193],                         # second chunk holds one entry
    "two_long": [4, 9000, 6, 0, 16385, 3],      # slots 0-1 and 2-4
    "empty_block": [0] * 1024 + [3, 0, 5, 2],   # a stream block of only empty rows
    # CSR5: tile 0 with 301 row ends (ends on the tile edge), tile 1 with 1024
    "c5_ends": [3] * 300 + [124] + [1] * 1024 + [10, 20],
    # a gap tile with 200 row ends
    "c5_gap": [3, 0] * 200 + [0, 0, 500, 0, 7],
    # a row over tiles 0-2 (tile 1 has no row start), a padded last tile; x[0] = inf
    "c5_pad_inf": [10, 3000, 5, 0, 12, 485],
    # every column in the first third: one live panel
    "first_third": [5, 0, 2049, 7, 9000],
})
GPU_CASES = tuple(GPU_LENS)

# (id, algo, test options) of the parent-golden vectors
GOLDEN_FORMS = (("rowsplit", 1, {}), ("csr5", 2, {}), ("csr5_panel3", 2, {"csr5_panel": 1, "panels": 3}),
                ("csr5_hostplan", 2, {"csr5_hostplan": 1}), ("panel3", 4, {"panels": 3}))

_CACHE = {}


def gpu_case(name):
    """dict(m, n, rp, col, val, x, y0) of a GPU case; built once, do not modify"""
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng(1000 + GPU_CASES.index(name))
    lens = np.asarray(GPU_LENS[name], np.int64)
    n = N_COLS
    third = n // 3
    avail = np.arange(1, third) if name == "first_third" else np.concatenate(
        [np.arange(1, third), np.arange(2 * third, n)])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(avail, L, replace=False)) for L in lens]).astype(np.int32)
    val = rng.standard_normal(int(rp[-1]))
    x = rng.standard_normal(n)
    if name == "c5_pad_inf":
        x[0] = np.inf  # the padded tail's column is 0: its products must not reach y
    y0 = rng.standard_normal(len(lens))
    for a in (rp, col, val, x, y0):
        a.setflags(write=False)
    _CACHE[name] = dict(m=len(lens), n=n, rp=rp, col=col, val=val, x=x, y0=y0)
    return _CACHE[name]


def panel_rowptrs(case, psplit):
    """the rowptr of every non-empty column panel of a split into psplit panels"""
    n, rp, col = case["n"], case["rp"], case["col"]
    W = (n + psplit - 1) // psplit
    row = np.repeat(np.arange(case["m"]), np.diff(rp))
    out = []
    for p in range(psplit):
        cnt = np.bincount(row[col // W == p], minlength=case["m"])
        if cnt.sum():
            out.append(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64))
    return out


def run_case(torch, sb, case, algo, opts, beta):
    """y of one launch (beta == 0: y0 seeded with NaN), and the handle's spmv_info if the library has it"""
    y0 = np.full(case["m"], np.nan) if beta == 0.0 else case["y0"].copy()
    with sb.test_options(**opts):
        A = sb.DeviceCSR.upload(0, case["n"], case["rp"], case["col"], case["val"])
        A.analyse(algo)
    xd = torch.from_numpy(case["x"].copy()).cuda()
    yd = torch.from_numpy(y0).cuda()
    A.spmv(algo, ALPHA, xd.data_ptr(), beta, yd.data_ptr())
    torch.cuda.synchronize()
    info = A.spmv_info(algo) if hasattr(A, "spmv_info") else None
    out = yd.cpu().numpy()
    A.close()
    return out, info


# ---------------------------------------------------------------------------
# CPU cases (test_spmv_shape_cpu.py)
# ---------------------------------------------------------------------------
MiB = 1 << 20
N_120MIB = 120 * MiB // 8     # x of 120 MiB: the widest matrix AUTO gives to xsort
N_GATE = 8 * MiB // 8 + 1     # the narrowest x (8 MiB + 8 B) past the panels' size gate

# (arguments of sblas.spmv_shape_host for algo 0, expected algorithm)
PICK_CASES = [
    (dict(n=1000, nnz=1_999_999, share=0.125), 4),
    (dict(n=1000, nnz=2_000_000, share=0.125), 5),
    (dict(n=N_120MIB, nnz=3_000_000, share=0.125), 5),
    (dict(n=N_120MIB + 1, nnz=3_000_000, share=0.125), 4),
    (dict(n=1000, nnz=3_000_000, share=0.25), 5),
    (dict(n=1000, nnz=3_000_000, share=0.2500001), 1),
    (dict(n=1000, nnz=1000, share=0.2500001), 1),
    (dict(n=1000, nnz=1000, share=0.25, adjacency=0.5), 1),
    (dict(n=1000, nnz=1000, share=0.25, adjacency=0.4999999), 4),
    (dict(n=1000, nnz=3_000_000, share=0.125, adjacency=0.9), 5),   # xsort first, whatever the adjacency
] + [(dict(n=1000, nnz=1000, share=0.125, auto_env=v), v) for v in (1, 2, 3, 4, 5)] + [
    (dict(n=1000, nnz=1000, share=0.125, auto_env=0), 4),
    (dict(n=1000, nnz=1000, share=0.125, auto_env=6), 4),
    (dict(n=1000, nnz=3_000_000, share=0.125, auto_env=-1), 5),
]

_PAY = dict(n=N_GATE, nnz=2_000_000, scattered=0.5, share=0.25)   # every condition of the panel rule just met

# (algo, arguments, expected fields)
PANEL_CASES = [
    (1, _PAY, dict(algo=1, panels=1, npanels=3, W=349526, wants_probe=1)),
    (1, dict(_PAY, n=N_GATE - 1), dict(panels=0, wants_probe=0)),
    (1, dict(_PAY, nnz=1_999_999), dict(panels=0, wants_probe=0)),
    (1, dict(_PAY, scattered=0.4999999), dict(panels=0, wants_probe=1)),
    (1, dict(_PAY, share=0.2500001), dict(panels=0, wants_probe=1)),
    (2, _PAY, dict(algo=2, panels=1, npanels=3, c5_host=0, wants_probe=1)),
    (3, _PAY, dict(algo=3, panels=1, npanels=3)),
    (2, dict(_PAY, n=N_GATE - 1), dict(panels=0, wants_probe=0)),
    (2, dict(_PAY, nnz=1_999_999), dict(panels=0, wants_probe=0)),
    (2, dict(_PAY, scattered=0.4999999), dict(panels=0)),
    (2, dict(_PAY, share=0.2500001), dict(panels=0)),
    # default_panels: ~4 MiB of x per panel, at most 8, at most n
    (4, dict(n=4 * MiB // 8, nnz=10), dict(algo=4, panels=1, npanels=1, W=4 * MiB // 8, wants_probe=0)),
    (4, dict(n=4 * MiB // 8 + 1, nnz=10), dict(npanels=2, W=262145)),
    (4, dict(n=32 * MiB // 8, nnz=10), dict(npanels=8, W=524288)),
    (4, dict(n=64 * MiB // 8, nnz=10), dict(npanels=8, W=1048576)),
    (4, dict(n=3, nnz=10, panels=8), dict(npanels=3, W=1)),
    (4, dict(n=0, nnz=0, panels=4), dict(npanels=1, W=0)),
    (4, dict(n=1000, nnz=10, panels=3), dict(npanels=3, W=334)),
    (4, dict(n=1000, nnz=10, panels=0), dict(npanels=1)),
    (4, dict(n=1000, nnz=10, panels=100), dict(npanels=64)),
    # CSR5 doubles the count (at most 8) from 32M entries, unless "panels" says how many
    (2, dict(_PAY, nnz=31_999_999), dict(panels=1, npanels=3)),
    (2, dict(_PAY, nnz=32_000_000), dict(panels=1, npanels=6, W=174763)),
    (2, dict(_PAY, n=32 * MiB // 8, nnz=32_000_000), dict(npanels=8)),
    (2, dict(_PAY, nnz=32_000_000, panels=4), dict(panels=1, npanels=4)),
    (1, dict(_PAY, nnz=32_000_000), dict(panels=1, npanels=3)),      # the row split never doubles
    # the hooks override the size gate (and then no probe is needed)
    (1, dict(n=1000, nnz=10, rs_panel=1), dict(panels=1, npanels=1, wants_probe=0)),
    (1, dict(_PAY, rs_panel=0), dict(panels=0, wants_probe=0)),
    (1, dict(_PAY, csr5_panel=0), dict(panels=1)),                   # CSR5's hook is not the row split's
    (2, dict(n=1000, nnz=10, csr5_panel=1, panels=3), dict(panels=1, npanels=3, wants_probe=0)),
    (2, dict(n=1000, nnz=10, csr5_panel=1), dict(panels=0, npanels=1)),   # one panel is no panel form
    (2, dict(_PAY, csr5_panel=0), dict(panels=0, wants_probe=0)),
    (2, dict(_PAY, rs_panel=0), dict(panels=1)),
    # host-built descriptors have no panel form
    (2, dict(_PAY, csr5_hostplan=1), dict(panels=0, c5_host=1)),
    (2, dict(_PAY, csr5_hostplan=0), dict(panels=1, c5_host=0)),
    (2, dict(n=1000, nnz=10, csr5_panel=1, panels=3, csr5_hostplan=1), dict(panels=0, c5_host=1)),
    (5, _PAY, dict(algo=5, panels=0, npanels=0, W=0, wants_probe=0)),
    # AUTO's pick carries the picked algorithm's shape
    (0, dict(n=1000, nnz=1000, share=0.125), dict(algo=4, panels=1, npanels=1, wants_probe=1)),
    (0, dict(_PAY, nnz=1_999_999, adjacency=0.9), dict(algo=1, panels=0)),
]

# (row lengths, expected [row, a, b] per block, expected counts:
#  blocks, stream, long1, longn, slots, max_rows)
ROWBLOCK_CASES = {
    "sum2048": ([1000, 1000, 48], [[0, 3, 0]], (1, 1, 0, 0, 0, 3)),
    "sum2049": ([1000, 1000, 49], [[0, 2, 0], [2, 3, 0]], (2, 2, 0, 0, 0, 2)),
    "row2048": ([2048], [[0, 1, 0]], (1, 1, 0, 0, 0, 1)),
    "row2049": ([2049], [[0, -1, -1]], (1, 0, 1, 0, 0, 1)),
    "row8192": ([8192], [[0, -1, -1]], (1, 0, 1, 0, 0, 1)),
    "row8193": ([8193], [[0, -1, 0], [0, -2, 1]], (2, 0, 0, 1, 2, 1)),
    "row16385": ([16385], [[0, -1, 0], [0, -2, 1], [0, -3, 2]], (3, 0, 0, 1, 3, 1)),
    "rows1025": ([1] * 1025, [[0, 1024, 0], [1024, 1025, 0]], (2, 2, 0, 0, 0, 1024)),
    "all_empty": ([0] * 5, [[0, 5, 0]], (1, 1, 0, 0, 0, 5)),
    "all_empty1025": ([0] * 1025, [[0, 1024, 0], [1024, 1025, 0]], (2, 2, 0, 0, 0, 1024)),
    "m0": ([], [], (0, 0, 0, 0, 0, 0)),
    "long_between": ([3, 3000, 4], [[0, 1, 0], [1, -1, -1], [2, 3, 0]], (3, 2, 1, 0, 0, 1)),
    "two_slots": ([9000, 2, 20000], [[0, -1, 0], [0, -2, 1], [1, 2, 0], [2, -1, 2], [2, -2, 3], [2, -3, 4]],
                  (6, 1, 0, 2, 5, 1)),
    "full_then_more": ([2048, 1], [[0, 1, 0], [1, 2, 0]], (2, 2, 0, 0, 0, 1)),
}

# row lengths of the CSR5 descriptor cases (beside GPU_LENS and the three generators)
CSR5_LENS = {
    "nnz1": [1], "nnz1023": [1023], "nnz1024": [1024], "nnz1025": [1025],
    "sevens1023": [7] * 146 + [1], "sevens1024": [7] * 146 + [2], "sevens1025": [7] * 146 + [3],
    "ones1024": [1] * 1024,                       # every bit of every lane set
    "row3000": [5, 3000, 9],                      # a head run of 2 after the row's first tile
    "tile_edge": [1000, 24, 8],                   # a row ending exactly on the tile edge
    "empty_start": [0, 0, 0, 5, 6],
    "empty_end": [5, 6, 0, 0],
    "empty_across_edge": [1020, 4, 0, 0, 7, 0, 3],   # empty rows on the tile edge itself
    "empty_inside": [3, 0, 4, 0, 0, 5] * 200,
    "all_empty": [0] * 9,
    "m0": [],
    "long_run": [7, 5000, 0, 2],
}


def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def csr5_brute(rp):
    """CSR5's tile descriptors of a rowptr, restated with numpy (entry by entry)"""
    rp = np.asarray(rp, np.int64)
    m, nnz = len(rp) - 1, int(rp[-1])
    nt = -(-nnz // TILE)
    lens = np.diff(rp)
    live = np.flatnonzero(lens > 0)
    start = np.zeros(nt * TILE, bool)
    start[rp[live]] = True
    flags = (start.reshape(nt * 64, SIGMA).astype(np.uint32) << np.arange(SIGMA, dtype=np.uint32)).sum(1)
    row_of = np.repeat(np.arange(m), lens)  # the row of every entry
    tile_row, seg_off, seg_row = np.full(nt + 1, m, np.uint32), np.zeros(nt + 1, np.int64), []
    for t in range(nt):
        e, last = t * TILE, min(nnz, (t + 1) * TILE) - 1
        rf, rl = row_of[e], row_of[last]
        gap = bool(np.any(lens[rf:rl + 1] == 0))
        tile_row[t] = rf | (0x80000000 if gap else 0)
        seg_off[t] = len(seg_row)
        if gap:
            seg_row += [r for r in live if e <= rp[r] <= last]
    seg_off[nt] = len(seg_row)
    head_run = np.zeros(nt, np.int64)  # maximal runs of tiles whose first entry continues one row
    t = 0
    while t < nt:
        u = t
        while u < nt and not start[u * TILE] and row_of[u * TILE] == row_of[t * TILE]:
            u += 1
        head_run[t] = u - t
        t = max(u, t + 1)
    return dict(flags=flags.astype(np.uint32), tile_row=tile_row, seg_off=seg_off, seg_row=np.asarray(seg_row, np.int64),
                empty_rows=np.flatnonzero(lens == 0), head_run=head_run)
