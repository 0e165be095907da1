"""Inputs for the tests of merge_points (dsa_encode_merged_sequential_batch, merge_points = 1; synth.merge_points): point clouds
whose cells are exact by construction, and the contract restated in numpy.

Exact cells: integer-valued positions on the grid ([0, 0, 0], 2^bits - 1) quantise to themselves, whatever the float arithmetic.
The cells lie along z -- cell j is (0, 0, j) -- so that the Morton key is monotone in j (bit b of z is bit 3 b of the key), a
multiplicity per cell says how many rows fall into it, and the rows are shuffled, so that "the smallest row of the cell" is not the
first row seen and sorted entry e belongs to the cell the multiplicities put there.

    pin(pos, bits, grid)            (kept, row_entries, cells): numpy quantisation (meshutil), np.unique over the integer triples,
                                    the smallest row per cell, the cells in Morton order (ordercases.morton_key)
    along_z(mults, bits, seed)      Case of sum(mults) rows, cell j with mults[j] rows
    cases()                         [Case(name, pos, bits, grid)]  grid: (origin[3], range) or None; every case of the host check"""
import collections

import numpy as np

import meshutil
import ordercases as oc

TILE = oc.TILE
Case = collections.namedtuple("Case", "name pos bits grid")


def quantised(pos, bits, grid=None):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    if grid is None:
        return meshutil.source_quantization(pos, bits)[2]
    return meshutil.quantize(pos, np.asarray(grid[0], np.float32), np.float32(grid[1]), bits)


def pin(pos, bits, grid=None):
    """The contract from the integers alone: the cells are the distinct integer triples (the positions here quantise into 0 ..
    2^bits - 1, so the low bits are the integers), kept[j] the smallest row of the j-th cell in Morton order, row_entries[r] the
    j of r's cell."""
    q = quantised(pos, bits, grid)
    assert q.min() >= 0 and q.max() <= (1 << bits) - 1
    cells, first, inverse = np.unique(q, axis=0, return_index=True, return_inverse=True)      # first: the smallest row of each
    inverse = np.asarray(inverse).ravel()
    order = np.argsort(oc.morton_key(cells, bits), kind="stable")                             # (keys of distinct cells are distinct)
    rank = np.zeros(len(cells), np.int64)
    rank[order] = np.arange(len(cells))
    return first[order].astype(np.uint32), rank[inverse].astype(np.uint32), cells[order]


def z_grid(bits):
    return (np.float32([0, 0, 0]), np.float32((1 << bits) - 1))


def along_z(name, mults, bits, seed):
    mults = np.asarray(mults, np.int64)
    assert len(mults) <= 1 << bits and mults.min() >= 1
    z = np.repeat(np.arange(len(mults)), mults)
    z = z[np.random.default_rng(seed).permutation(len(z))]
    pos = np.zeros((len(z), 3), np.float32)
    pos[:, 2] = z
    return Case(name, pos, bits, z_grid(bits))


def runs_of(case):
    """the multiplicities of a case of along_z, cell by cell: the runs of equal keys in sorted order"""
    return np.bincount(case.pos[:, 2].astype(np.int64))


SIZES = [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def sized(bits=14):
    """every size around the tile in three patterns: all distinct (m = n), all identical (m = 1), every cell twice"""
    out = []
    for k, n in enumerate(SIZES):
        out.append(along_z("distinct-%d" % n, np.ones(n, np.int64), bits, 200 + k))
        out.append(along_z("identical-%d" % n, [n], bits, 300 + k))
        twice = [2] * (n // 2) + [1] * (n % 2)
        out.append(along_z("twice-%d" % n, twice, bits, 400 + k))
    return out


def boundary_runs(bits=14):
    """runs of equal keys across the kernels' boundaries, as multiplicities over the sorted entries"""
    T = TILE
    return [
        along_z("run-over-63|64", [60, 8, 100], bits, 501),                     # entries 60 .. 67: one cell over the step boundary
        along_z("run-over-1023|1024", [1000, 48, 500], bits, 502),             # entries 1000 .. 1047: one cell over the tile boundary
        along_z("run-of-1500", [10, 1500, 10], bits, 503),
        along_z("two-whole-tiles", [T, 2 * T, 5], bits, 504),                   # a run that is exactly tiles 1 and 2
        along_z("head-at-a-tile-start", [T - 1, 1, 7, 30], bits, 505),         # the head of cell 2 is entry T
        along_z("tile-with-no-head", [T - 5, 2 * T + 10, 3], bits, 506),       # tile 1 lies inside the run of cell 1
        along_z("heads-at-every-64", [64] * 40, bits, 507),
        # entries 60 .. 67 | 1000 .. 1047 | a head at 2 T, of a run of 1 500 | 3 548 .. 6 243: tiles 4 and 5 whole, without a head
        along_z("all-of-it", [60, 8, 932, 48, 1000, 1500, 2696, 1, 1, 3], bits, 508),
    ]


def spans(case):
    """what the runs of a case of along_z cross, by name"""
    T = TILE
    start = np.concatenate([[0], np.cumsum(runs_of(case))])
    pairs = list(zip(start[:-1], start[1:]))
    over = lambda e: any(a < e < b for a, b in pairs)          # noqa: E731  (entries e - 1 and e lie in one run)
    return {"63|64": over(64), "1023|1024": over(T), "run of 1500": 1500 in runs_of(case), "head at a tile start": any(a > 0 and a % T == 0 for a in start[:-1]),
            "two whole tiles": any(b - (a + T - 1) // T * T >= 2 * T for a, b in pairs), "tile with no head": any(b - (a // T + 1) * T >= T for a, b in pairs)}


def half_duplicated(n, seed, bits=11):
    """n rows of a random cloud of which about half repeat the position of another row (shuffled): cells by the coder's arithmetic
    on own bounds"""
    rng = np.random.default_rng(seed)
    base = oc.random_cloud(max(1, (n + 1) // 2), seed + 1)
    pos = np.concatenate([base, base[rng.integers(0, len(base), n - len(base))]]) if n > len(base) else base
    return Case("half-%d" % n, np.ascontiguousarray(pos[rng.permutation(len(pos))]), bits, None)


def dropped_extremes(seed=61, bits=11):
    """own bounds whose minimum and maximum of every component are held by rows the merge drops: rows 4 and 5 are copies of
    rows 2 and 3 moved by less than half a cell, outwards"""
    rng = np.random.default_rng(seed)
    pos = (rng.random((600, 3)).astype(np.float32) * np.float32(0.8) + np.float32(0.1))
    pos[2], pos[3] = np.float32([0.0, 0.0, 0.0]), np.float32([1.0, 1.0, 1.0])
    step = np.float32(1.0 / ((1 << bits) - 1))
    pos[4], pos[5] = pos[2] - np.float32(0.25) * step, pos[3] + np.float32(0.25) * step     # the extremes; they share the cells of rows 2 and 3
    # rows 2 and 3 come first in row order: they stay, rows 4 and 5 go
    return Case("dropped-extremes", pos, bits, None)


def explicit(seed=62, bits=5):
    pos = oc.random_cloud(3000, seed) * np.float32(3.0) - np.float32(1.0)
    return Case("explicit-grid", pos, bits, (np.float32([-1.5, -1.25, -1.0]), np.float32(4.5)))


def large(seed=63, bits=12):
    """about 70 000 points in 2 049 cells of 1 to 67 rows each"""
    rng = np.random.default_rng(seed)
    return along_z("large", rng.integers(1, 68, 2048).tolist() + [1], bits, seed)


def cases():
    return sized() + boundary_runs() + [half_duplicated(n, 70 + n) for n in (1, 777, TILE + 5)] + [dropped_extremes(), explicit()]
