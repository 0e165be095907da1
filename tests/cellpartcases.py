"""Inputs for the tests of part_cells (dsa_encode_cell_parts_sequential_batch, part_cells >= 1; synth.cell_parts /
synth.encode_cell_parts): point clouds whose cells are exact by construction (mergecases.along_z: cell j is (0, 0, j), a
multiplicity per cell, the rows shuffled), with numbers of kept points m and part sizes N on the edges of the kernels -- the 64
entries of a wave step, the 1024-entry tile of the sort and of k_enc_part_bounds -- and the contract restated in numpy.  Seeds are
fixed.  N = 1 and 2 are cut only from clouds of up to 130 rows: a cloud has ceil(n / N) part slots, each with regions of its own.

    pin(c)                  (kept, row_entries, ranges, qmin, qmax): mergecases.pin, splitcases.parts over m, numpy's boxes
    part_sizes(m, n)        every part_cells a cloud of n rows in m cells is cut at
    sized()                 m over M in three patterns: all distinct (m = n: no empty slot), every cell twice (n = 2 m), all
                            identical (m = 1: every slot behind the first is empty)
    cuts()                  cuts inside a tile of the sorted order and on its edge, runs of equal keys just in front of a cut,
                            own bounds, an explicit grid that is not the cells'
    large()                 70 001 rows in 2 049 cells at part_cells 120: 18 parts
    cases()                 every case but large()"""
import collections

import numpy as np

import mergecases as mc
import ordercases as oc
import splitcases as sc

TILE = oc.TILE
INT32_MAX = sc.INT32_MAX
BITS = 12                  # 2 T + 1 cells along z need 12 bits
Case = collections.namedtuple("Case", "name pos bits grid part_cells")
M = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
N_EDGES = [63, 64, 65, TILE - 1, TILE, TILE + 1, INT32_MAX]


def part_sizes(m, n):
    """the edges, and around m: m = N (one full part) and m = N + 1 (two parts); full_slots() has m = P_max N"""
    out = ([1, 2] if n <= 130 else []) + N_EDGES + ([m, m - 1] if n <= 130 * m else [])
    return sorted({N for N in out if N >= 1})


def with_parts(c, N, name=None):
    return Case(name or "%s-N%d" % (c.name, N), c.pos, c.bits, c.grid, N)


def sized(bits=BITS):
    out = []
    for k, m in enumerate(M):
        clouds = [mc.along_z("distinct-m%d" % m, np.ones(m, np.int64), bits, 700 + k), mc.along_z("twice-m%d" % m, [2] * m, bits, 720 + k),
                  mc.along_z("identical-n%d" % m, [m], bits, 740 + k)]
        for c in clouds:
            cells = len(mc.runs_of(c))
            out += [with_parts(c, N) for N in part_sizes(cells, len(c.pos))]
    return out


def full_slots(bits=BITS):
    """m = P_max N with P_max > 1: n = m, every slot of the layout is a full part (126 = 2 * 63, 2 T = 2 * T)"""
    return [with_parts(mc.along_z("distinct-m126", np.ones(126, np.int64), bits, 761), 63), with_parts(mc.along_z("distinct-m2T", np.ones(2 * TILE, np.int64), bits, 762), TILE)]


def cuts(bits=BITS):
    T = TILE
    own = mc.along_z("own-bounds", [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5] * 40, bits, 771)
    own = mc.Case(own.name, own.pos * np.float32(0.25) - np.float32(7.0), bits, None)          # 440 cells on the cloud's own bounds
    grid = mc.along_z("explicit-grid", [2, 7, 1] * 300, bits, 772)
    grid = mc.Case(grid.name, grid.pos, bits, (np.float32([-3.0, -2.0, -5.0]), np.float32(4100.0)))       # a grid that is not the cells': steps of a little over 1, where two neighbours may share a cell
    return [
        with_parts(mc.along_z("cut-inside-a-tile", [3] * 100, bits, 763), 50),               # kept entry 50 is sorted entry 150
        with_parts(mc.along_z("cut-on-a-tile-edge", [T // 2, T // 2, 5, 1, 1, 7], bits, 764), 2),      # kept entry 2 is sorted entry T
        with_parts(mc.along_z("run-over-63|64-at-a-cut", [60, 8] + [1] * 10, bits, 765), 2),    # the run of cell 1 is sorted 60 .. 67, the cut right behind it
        with_parts(mc.along_z("run-over-1023|1024-at-a-cut", [1000, 48] + [3] * 10, bits, 766), 2),
        with_parts(mc.along_z("run-of-1500-at-a-cut", [10, 1500, 10, 1, 2, 3], bits, 767), 2),
        with_parts(mc.along_z("all-of-it", [60, 8, 932, 48, 1000, 1500, 2696, 1, 1, 3], bits, 768), 3),
        with_parts(own, 100), with_parts(own, 440), with_parts(grid, 128), with_parts(grid, 450),
    ]


def large(seed=781, bits=BITS):
    rng = np.random.default_rng(seed)
    mults = rng.integers(1, 67, 2048).tolist()                 # (about 68 600 rows; the last cell takes the rest)
    mults.append(70001 - sum(mults))
    return with_parts(mc.along_z("large", mults, bits, seed), 120, "large")


def cases():
    return sized() + full_slots() + cuts()


def quantised(c):
    return mc.quantised(c.pos, c.bits, c.grid)


def pin(c):
    """(kept, row_entries, ranges, qmin, qmax) from numpy alone: the cells of mergecases.pin, splitcases.parts over the m kept
    entries, and the boxes of the integers of every slice of kept"""
    kept, cells, _ = mc.pin(c.pos, c.bits, c.grid)
    q = quantised(c)
    r = sc.parts(len(kept), c.part_cells)
    return kept, cells, r, np.array([q[kept[lo:hi]].min(axis=0) for lo, hi in r], np.int32), np.array([q[kept[lo:hi]].max(axis=0) for lo, hi in r], np.int32)


def slots(c):
    """the part slots the layout gives the cloud: ceil(n / N)"""
    return -(-len(c.pos) // c.part_cells)
