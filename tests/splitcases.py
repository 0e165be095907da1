"""Inputs for the tests of part_points (dsa_encode_split_sequential_batch, part_points >= 1; synth.split_parts / synth.encode_split):
point clouds whose sizes and part sizes sit on the edges of the kernels -- the 64 entries of a wave step, the 1024-entry tile of the
sort and of k_enc_part_bounds -- and the contract restated in numpy.  Seeds are fixed.

    parts(n, N)             the pin: P = ceil(n / N), part p = [p n // P, (p + 1) n // P) in Python's integers; (P, 2) int64
    part_sizes(n)           every part_points a cloud of n points is cut at
    sized()                 [Case(name, pos, bits, grid, part_points)] over SIZES x part_sizes
    cuts()                  cuts at a wave step, at a tile edge, and inside a run of equal keys
    large()                 70 001 points at part_points 4096: 18 parts (host check and CPU test only)
    cases()                 every case of the host check but large()"""
import collections

import numpy as np

import mergecases as mc
import ordercases as oc

TILE = oc.TILE
Case = collections.namedtuple("Case", "name pos bits grid part_points")
SIZES = [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
INT32_MAX = 2**31 - 1


def parts(n, N):
    P = -(-n // N) if N else 1
    return np.array([[p * n // P, (p + 1) * n // P] for p in range(P)], np.int64).reshape(P, 2)


def part_sizes(n):
    out = ([1] if n <= 65 else []) + [2, 63, 64, 65, TILE - 1, TILE, TILE + 1, n - 1, n, n + 1, INT32_MAX]
    return sorted({N for N in out if N >= 1})


def sized(bits=11):
    out = []
    for k, n in enumerate(SIZES):
        pos = oc.random_cloud(n, 600 + k)
        out += [Case("n%d-N%d" % (n, N), pos, bits, None, N) for N in part_sizes(n)]
    return out


def run_over_a_cut(bits=14):
    """cells along z with multiplicities (mergecases.along_z): 300 rows, the run of cell 2 is sorted entries 140 .. 159, and at
    part_points 150 the cut at entry 150 lies inside it -- the points of one cell land in two parts, and nothing is merged"""
    c = mc.along_z("run-over-a-cut", [100, 40, 20, 140], bits, 611)
    return Case(c.name, c.pos, c.bits, c.grid, 150)


def cuts():
    T = TILE
    return [Case("n2T-NT", oc.random_cloud(2 * T, 621), 11, None, T),                      # a cut at a tile edge of the sort
            Case("n2T+1-NT+1", oc.random_cloud(2 * T + 1, 622), 11, None, T + 1),          # parts of T + 1 and T: the cut one entry behind it
            Case("n130-N65", oc.random_cloud(130, 623), 11, None, 65),                     # a cut one entry behind a wave step
            run_over_a_cut(),
            Case("explicit-grid", oc.random_cloud(2500, 624) * np.float32(3.0) - np.float32(1.0), 12, (np.float32([-1.5, -1.25, -1.0]), np.float32(4.5)), 700)]


def large():
    return Case("large", oc.random_cloud(70001, 631), 11, None, 4096)


def cases():
    return sized() + cuts()


def quantised(c):
    return mc.quantised(c.pos, c.bits, c.grid)


def pin(c):
    """(perm, ranges, qmin, qmax) from numpy alone: the order of ordercases over numpy's quantisation, the ranges of parts(), and
    the boxes of the integers of every slice"""
    q = quantised(c)
    perm = oc.morton_order(q, c.bits)
    r = parts(len(c.pos), c.part_points)
    return perm, r, np.array([q[perm[lo:hi]].min(axis=0) for lo, hi in r], np.int32), np.array([q[perm[lo:hi]].max(axis=0) for lo, hi in r], np.int32)
