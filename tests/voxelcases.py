"""Inputs for the tests of voxels coarser than the position grid (dsa_encode_voxel_sequential_batch, voxel_bits = C, voxel_point;
synth.merge_voxels), and the three rules restated in Python integers -- nothing here is shared with the C++ twin or the kernels.

Exact integers: integer-valued positions on the grid ([0, 0, 0], 2^B - 1) quantise to themselves (mergecases), so a case is written
down as the integers q (n, 3) its rows are coded as; the voxel of a row is q >> s per axis, s = B - C, the offset inside it q & (2^s -
1).  A case names its voxels in Morton order with a multiplicity each, so that sorted entry e belongs to the voxel the multiplicities
put there; the rows are shuffled unless the case is about their order.

    pin(case, point)        (kept, row_entries, coded): the contract in Python integers -- key by bit interleave, the rows sorted by
                            (key, row), heads where key >> 3 s changes; FIRST the head's row, CENTROID floor((2 S + cnt) / (2 cnt))
                            per component at that row, NEAREST the row with the smallest (dist, row); coded (m, 3) the integers
                            the position stream codes at the kept rows
    cases()                 [Case(name, pos, bits, C, grid)], each at most about 12 000 points, B in {6, 11, 14, 20}, C in {1, 2, B - 1, B}"""
import collections
import functools

import numpy as np

import mergecases as mc

TILE = mc.TILE
FIRST, CENTROID, NEAREST = 0, 1, 2
POINTS = (FIRST, CENTROID, NEAREST)
Case = collections.namedtuple("Case", "name pos bits C grid")


def _key(q, bits):
    k = 0
    for b in range(bits):
        for c in range(3):
            k |= ((q[c] >> b) & 1) << (3 * b + 2 - c)
    return k


def integers(case):
    """the integers the position stream codes for the rows of a case, as Python lists"""
    return [[int(x) for x in r] for r in mc.quantised(case.pos, case.bits, case.grid)]


def rule(q, bits, C, point):
    """The contract on integer rows q (a list of 3-lists) at B = bits, voxel_bits = C (0: the position cells): (kept, row_entries,
    coded) in Python integers."""
    n, s = len(q), (bits - C if C else 0)
    keys = [_key(r, bits) for r in q]
    perm = sorted(range(n), key=lambda r: (keys[r], r))
    first, rows_of, entry = [], [], [0] * n
    for e, r in enumerate(perm):
        if e == 0 or keys[r] >> (3 * s) != keys[perm[e - 1]] >> (3 * s):
            first.append(r)
            rows_of.append([])
        rows_of[-1].append(r)
        entry[r] = len(first) - 1
    kept, coded = list(first), [list(q[r]) for r in first]
    span = (1 << s) - 1
    for j, rows in enumerate(rows_of):
        if point == CENTROID:
            cnt = len(rows)
            coded[j] = [(2 * sum(q[r][c] for r in rows) + cnt) // (2 * cnt) for c in range(3)]
        elif point == NEAREST:
            dist = lambda r: sum((2 * (q[r][c] & span) - span) ** 2 for c in range(3))          # noqa: E731
            kept[j] = min(rows, key=lambda r: (dist(r), r))
            coded[j] = list(q[kept[j]])
    return kept, entry, coded


@functools.lru_cache(maxsize=None)
def _pin(name, point):
    case = named(name)
    kept, entry, coded = rule(integers(case), case.bits, case.C, point)
    return np.asarray(kept, np.uint32), np.asarray(entry, np.uint32), np.asarray(coded, np.int64).reshape(-1, 3)


def pin(case, point):
    return _pin(case.name, point)


def _morton(v, bits):
    return [_key([int(x) for x in r], bits) for r in v]


def from_integers(name, q, bits, C):
    q = np.asarray(q, np.int64).reshape(-1, 3)
    assert q.min() >= 0 and q.max() < 1 << bits and 1 <= C <= bits
    return Case(name, q.astype(np.float32), bits, C, mc.z_grid(bits))


def voxel_runs(name, bits, C, mults, seed, shuffle=True):
    """len(mults) distinct voxels of the C-bit grid, in Morton order voxel i with mults[i] rows at random offsets inside it"""
    rng = np.random.default_rng(seed)
    s, k = bits - C, len(mults)
    assert k <= 8 ** C
    if k == 8 ** C or 8 ** C <= 4096:
        ids = rng.permutation(8 ** C)[:k]
        vox = np.stack([(ids >> (2 * C)) & ((1 << C) - 1), (ids >> C) & ((1 << C) - 1), ids & ((1 << C) - 1)], axis=1)
    else:
        vox = np.unique(rng.integers(0, 1 << C, (4 * k + 64, 3)), axis=0)
        vox = vox[rng.permutation(len(vox))[:k]]
        assert len(vox) == k
    vox = vox[np.argsort(np.asarray(_morton(vox, C), np.uint64), kind="stable")]
    q = np.repeat(vox, np.asarray(mults, np.int64), axis=0) << s
    q = q + rng.integers(0, 1 << s, q.shape)
    if shuffle:
        q = q[rng.permutation(len(q))]
    return from_integers(name, q, bits, C)


def runs_of(case):
    """the rows of every voxel of a case in Morton order of the voxels"""
    q = np.asarray(integers(case), np.int64) >> (case.bits - case.C)
    _, inverse, counts = np.unique(np.asarray(_morton(q, case.C), np.uint64), return_inverse=True, return_counts=True)
    return counts


# runs that end at entries 63, 64 and 65 of a wave step and at 1023, 1024 and 1025 of a tile: eight voxels, which the 1-bit grid has
STEP_AND_TILE_ENDS = [64, 1, 1, TILE - 66, 1, 1, 70, 3]
BC = [(6, 1), (6, 2), (6, 5), (6, 6), (11, 1), (11, 2), (11, 10), (11, 11), (14, 1), (14, 2), (14, 13), (14, 14), (20, 1), (20, 2), (20, 19), (20, 20)]


def centroid_ties():
    """sums of exactly .5 above an integer in every component, over 2, 4 and 6 rows: they round up.  s = 4, three voxels."""
    a = [[0, 0, 0], [1, 1, 1]]
    b = [[16, 0, 0], [16, 0, 0], [17, 1, 1], [17, 1, 1]]
    c = [[3, 18, 5]] * 3 + [[4, 19, 6]] * 3
    # (Morton order of the voxels: (0, 0, 0), (0, 1, 0), (1, 0, 0))
    return from_integers("centroid-ties-6-2", a + b + c, 6, 2), np.array([[1, 1, 1], [4, 19, 6], [17, 1, 1]], np.int64)


def centroid_in_an_empty_cell():
    """the mean of (0, 0, 0) and (4, 4, 4) is (2, 2, 2), a cell no row occupies; of three corners of a voxel a cell inside it"""
    q = [[0, 0, 0], [4, 4, 4], [1024, 1024, 0], [2047, 1024, 0], [1024, 2047, 0]]
    return from_integers("centroid-empty-cell-11-1", q, 11, 1), np.array([[2, 2, 2], [1365, 1365, 0]], np.int64)


def nearest_ties():
    """two and four rows at equal distance, mirrored about the centre of the voxel, the smaller row later in Morton order, and a
    row farther out in front of them all: the first arrival, the first in sorted order and the smallest row are all wrong.  s = 2."""
    two = [[0, 0, 0], [2, 2, 2], [1, 1, 1]]                                      # rows 0 .. 2 of voxel (0, 0, 0): row 1 wins
    four = [[7, 4, 4], [6, 6, 6], [5, 6, 5], [6, 5, 6], [5, 5, 5]]               # rows 3 .. 7 of voxel (1, 1, 1): row 4 wins
    return from_integers("nearest-ties-11-9", two + four, 11, 9), np.array([1, 4], np.uint32)


def nearest_far_corners():
    """s = 19: rows at opposite corners of a voxel, dist = 3 (2^19 - 1)^2 each, the smaller row wins; and a voxel whose corner rows
    lose to a row one step nearer"""
    top = (1 << 19) - 1
    q = [[top, top, top], [0, 0, 0], [1 << 19, 0, 0], [(1 << 19) + top, top, top], [(1 << 19) + 1, 0, 0]]
    return from_integers("nearest-corners-20-1", q, 20, 1), np.array([0, 4], np.uint32)


DESIGNED = {"centroid-ties-6-2": (CENTROID, centroid_ties), "centroid-empty-cell-11-1": (CENTROID, centroid_in_an_empty_cell),
            "nearest-ties-11-9": (NEAREST, nearest_ties), "nearest-corners-20-1": (NEAREST, nearest_far_corners)}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for B, C in BC:
        out.append(voxel_runs("ends-%d-%d" % (B, C), B, C, STEP_AND_TILE_ENDS, 100 * B + C))
    out.append(voxel_runs("one-voxel-2100-14-2", 14, 2, [2100], 1))              # tiles with no head
    out.append(voxel_runs("one-voxel-2100-20-1", 20, 1, [2100], 2))
    out.append(voxel_runs("single-rows-11-10", 11, 10, [1] * 3000, 3))           # every voxel has one row
    out.append(voxel_runs("single-rows-6-2", 6, 2, [1] * 64, 4))
    out.append(voxel_runs("mixed-14-13", 14, 13, list(np.random.default_rng(5).integers(1, 9, 1500)), 5))
    out.append(voxel_runs("mixed-20-19", 20, 19, list(np.random.default_rng(6).integers(1, 5, 2500)), 6))
    out.extend(make()[0] for _, make in DESIGNED.values())
    d = voxel_runs("x", 11, 2, [5, 1, 9, 2, 30], 7)                               # every row four times
    out.append(Case("duplicated-11-2", np.ascontiguousarray(np.tile(d.pos, (4, 1))[np.random.default_rng(8).permutation(4 * len(d.pos))]), 11, 2, d.grid))
    rng = np.random.default_rng(9)                                                # floats on an explicit grid that is not their bounds
    out.append(Case("explicit-grid-11-2", (rng.random((3000, 3)) * [1.0, 0.7, 0.2] + 0.1).astype(np.float32), 11, 2, (np.float32([0, 0, 0]), np.float32(1.5))))
    out.append(Case("own-bounds-14-13", (rng.random((2500, 3)) * [0.01, 0.01, 0.002]).astype(np.float32), 14, 13, None))
    assert len({c.name for c in out}) == len(out) and max(len(c.pos) for c in out) <= 12000
    return out


def named(name):
    return next(c for c in cases() if c.name == name)


def groups():
    """the cases of one (B, C) are a batch: [((B, C), [Case])]"""
    keys = sorted({(c.bits, c.C) for c in cases()})
    return [(k, [c for c in cases() if (c.bits, c.C) == k]) for k in keys]


def cpu_args(case, **more):
    """the arguments of synth.encode_merged / encode_cell_parts / encode_lod_parts for the case"""
    import draco_sharp_amd.synth as synth
    out = dict(pos=case.pos, opt=synth.options(pos_bits=case.bits), pos_grid=None if case.grid is None else synth.grid(case.grid[0], case.grid[1]))
    out.update(more)
    return out


def cloud(case, **more):
    """the PointCloudData of the device call"""
    import draco_sharp_amd as dsa
    return dsa.PointCloudData(case.pos, position_grid=None if case.grid is None else dsa.Grid(case.grid[0], float(case.grid[1])), **more)
