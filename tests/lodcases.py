"""Inputs for the tests of lod_base_bits (dsa_encode_lod_sequential_batch, lod_base_bits >= 1; synth.lod_parts /
synth.encode_lod_parts): point clouds built from chosen integer cells on the explicit grid of origin 0 and range 2^B - 1, so that
the population of every level is exact by construction, and the contract restated in numpy.  Seeds are fixed.

A cloud is a set of Morton keys of B bit-triples.  Every point has zeros below the triple that gives it its level: a point of
level 0 is the smallest key of its coarse cell (D triples, then zeros); a point of level l >= 1 takes the key of a point of a lower
level -- whose triples from D + l - 1 on are zero -- and puts a digit 1 .. 7 into triple D + l - 1.  Its cell at D + l triples is
new, its cell at D + l - 1 triples is its parent's, and whatever lies in front of it in Morton order shares exactly D + l - 1
triples with it: level l.  So level l can hold up to 7 (m_0 + ... + m_(l-1)) points, level 0 up to 8^D.

    built(name, B, D, pops, N, seed, dup)   the cloud of populations pops, every cell dup times (a list: per kept entry), shuffled
    pin(c)                                  (lod, row_entries, ranges, level, qmin, qmax, levels of kept, kept) from numpy alone
    populations() / sizes() / boundaries() / special()      the lists below
    large()                                 70 001 points at 11 bits, D = 7, N = 300
    cases()                                 every case but large()"""
import collections

import numpy as np

import mergecases as mc
import ordercases as oc
import splitcases as sc

TILE = oc.TILE
INT32_MAX = sc.INT32_MAX
Case = collections.namedtuple("Case", "name pos bits grid part_cells lod_base_bits")
EDGES = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1]


def cells_of_keys(keys, bits):
    """the integer triples of Morton keys: x the top bit of every bit-triple"""
    keys = np.asarray(keys, np.uint64)
    q = np.zeros((len(keys), 3), np.int64)
    for b in range(bits):
        for c in range(3):
            q[:, c] |= (((keys >> np.uint64(3 * b + 2 - c)) & np.uint64(1)).astype(np.int64)) << b
    return q


def keys_of(bits, base_bits, pops, rng):
    """Morton keys with pops[l] points of level l, ascending"""
    L = bits - base_bits + 1
    assert len(pops) == L and 1 <= pops[0] <= 8 ** base_bits
    coarse = np.sort(rng.choice(8 ** base_bits, pops[0], replace=False)).astype(np.uint64)
    keys = [coarse << np.uint64(3 * (bits - base_bits))]
    for l in range(1, L):
        parents = np.concatenate(keys)
        assert pops[l] <= 7 * len(parents), (l, pops[l], len(parents))
        slot = rng.choice(7 * len(parents), pops[l], replace=False)
        digit = (slot % 7 + 1).astype(np.uint64)
        keys.append(parents[slot // 7] | (digit << np.uint64(3 * (bits - base_bits - l))))
    return np.sort(np.concatenate(keys))


def built(name, bits, base_bits, pops, part_cells, seed, dup=1, own=False):
    rng = np.random.default_rng(seed)
    keys = keys_of(bits, base_bits, list(pops), rng)
    dup = np.broadcast_to(np.asarray(dup, np.int64), keys.shape)
    pos = cells_of_keys(np.repeat(keys, dup), bits).astype(np.float32)
    pos = pos[rng.permutation(len(pos))]
    if own:                # the cloud's own bounds: the cells are whatever the coder's arithmetic makes of them
        return Case(name, pos * np.float32(0.25) - np.float32(7.0), bits, None, part_cells, base_bits)
    return Case(name, pos, bits, mc.z_grid(bits), part_cells, base_bits)


def populations():
    """every edge as the population of a level -- first, middle and last -- at a part size that cuts it"""
    out = []
    for k, m in enumerate(EDGES):
        if m:
            out.append(built("pop-first-%d" % m, 6, 4, [m, min(7 * m, 70), 9], 64, 900 + k))
        big = max(m, 1)
        out.append(built("pop-middle-%d" % m, 6, 4, [-(-big // 7) + 3, m, 11], 63, 920 + k))
        out.append(built("pop-last-%d" % m, 5, 3, [-(-big // 40) + 2, 5 * (-(-big // 40) + 2), m], 65, 940 + k))
    return out


def sizes():
    """every edge as part_cells over levels of 150, 1025 and 2049 points, over a small cloud for N = 1 and 2, and over levels of N and 2 N points"""
    out = [built("sizes-N%d" % N, 6, 4, [150, TILE + 1, 2 * TILE + 1], N, 960 + k) for k, N in enumerate(EDGES[3:] + [INT32_MAX])]
    out += [built("small-N%d" % N, 4, 3, [9, 21], N, 970 + N) for N in (1, 2)]
    out += [built("full-parts-N%d" % N, 6, 4, [150, N, 2 * N], N, 975 + k) for k, N in enumerate(EDGES[3:])]      # a level that is one full part, and one that is two
    return out


def boundaries():
    """where level 1 begins in lod order: inside a 64-entry step, on a step edge, on a tile edge"""
    T = TILE
    return [built("boundary-inside-a-step", 5, 4, [100, 300], 128, 981), built("boundary-on-a-step-edge", 5, 4, [128, 300], 128, 982),
            built("boundary-on-a-tile-edge", 5, 4, [T, 300], 500, 983), built("boundary-on-two-tile-edges", 6, 4, [T, T, 77], T, 984)]


def special():
    T = TILE
    twice = np.full(700 + 300 + 150, 2, np.int64)
    twice[0] = 3               # an odd number of rows in front of every other cell: the two rows of a cell lie on both sides of sorted entry T
    return [
        built("empty-level-in-the-middle", 6, 3, [40, 0, 90, 200], 64, 991),
        built("two-empty-levels", 6, 3, [5, 0, 0, 30], 7, 992),
        built("all-in-level-0", 5, 5, [3000], 700, 993),                   # D = B: one level
        built("all-in-level-0-N-max", 4, 4, [777], INT32_MAX, 994),
        built("one-cell", 6, 3, [1, 0, 0, 0], 64, 995, dup=5),
        built("one-point", 6, 3, [1, 0, 0, 0], 1, 996),
        built("own-bounds", 6, 3, [60, 170, 400, 900], 100, 997, dup=2, own=True),
        built("every-cell-twice", 6, 4, [700, 300, 150], 256, 998, dup=twice),
        built("one-stream-a-level", 6, 3, [64, 65, 63, 2], INT32_MAX, 999),
        built("many-empty-slots", 5, 3, [20, 50, 100], 16, 1000, dup=4),     # 680 rows in 170 cells: 45 slots, 13 parts
    ]


def large(seed=1001):
    """70 001 rows of a height field on an 11-bit grid, about a fifth of them in a cell another row has: D = 7, five levels"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 2048, (56000, 2))
    z = (1023 + 900 * np.sin(xy[:, 0] / 300.0) * np.cos(xy[:, 1] / 410.0)).astype(np.int64)
    cells = np.concatenate([xy, z[:, None]], axis=1)
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), 70001 - len(cells))]])
    cells[0], cells[1] = (0, 0, 0), (2047, 2047, 2047)
    return Case("large", cells[rng.permutation(len(cells))].astype(np.float32), 11, mc.z_grid(11), 300, 7)


def cases():
    return populations() + sizes() + boundaries() + special()


def quantised(c):
    return mc.quantised(c.pos, c.bits, c.grid)


Pin = collections.namedtuple("Pin", "lod row_entries ranges level qmin qmax kept_level kept")


def pin(c):
    """The contract from numpy alone: keys of the integers, the distinct ones ascending with the smallest row of each, the level
    rule, the stable partition by level, the parts of every level and the boxes of their integers."""
    q = quantised(c)
    key = oc.morton_key(q, c.bits)
    ukey, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    kept = first.astype(np.uint32)                 # (np.unique: the first occurrence, the smallest row of the cell)
    B, D = c.bits, c.lod_base_bits
    common = np.zeros(len(ukey), np.int64)         # leading bit-triples a key shares with the key in front of it
    still = np.ones(max(len(ukey) - 1, 0), bool)
    for t in range(B):
        shift = np.uint64(3 * (B - 1 - t))
        still = still & ((ukey[1:] >> shift) == (ukey[:-1] >> shift))
        common[1:] += still
    kept_level = np.maximum(0, common + 1 - D)
    kept_level[0] = 0
    L = B - D + 1
    assert kept_level.max() < L
    order = np.argsort(kept_level, kind="stable")
    lod = kept[order]
    place = np.zeros(len(kept), np.int64)
    place[order] = np.arange(len(kept))
    row_entries = place[inverse.reshape(-1)].astype(np.uint32)
    counts = np.bincount(kept_level, minlength=L)
    base = np.concatenate([[0], np.cumsum(counts)])
    ranges, level = [], []
    for l in range(L):
        if counts[l]:
            for lo, hi in sc.parts(int(counts[l]), c.part_cells):
                ranges.append([base[l] + lo, base[l] + hi])
                level.append(l)
    ranges = np.array(ranges, np.int64).reshape(-1, 2)
    qmin = np.array([q[lod[lo:hi]].min(axis=0) for lo, hi in ranges], np.int32)
    qmax = np.array([q[lod[lo:hi]].max(axis=0) for lo, hi in ranges], np.int32)
    return Pin(lod, row_entries, ranges, np.array(level, np.uint32), qmin, qmax, kept_level, kept)


def slots(c):
    """the part slots the layout gives the cloud: ceil(n / N) + L - 1"""
    return -(-len(c.pos) // c.part_cells) + c.bits - c.lod_base_bits
