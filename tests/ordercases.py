"""Inputs for the tests of the Morton point order (dsa_encode_ordered_sequential_batch, point_order = 1; synth.point_order): point
sets whose sizes sit on the edges of the sort's tile, position bits that give every pass count, keys that tie, keys that differ in
one lane of the interleave only, a grid of the caller's, and the shuffled height field of the size guard.  Seeds are fixed.

    morton_key(q, bits)     the definition, restated in numpy: the bits of x, y, z interleaved, x the top bit of every triple
    morton_order(q, bits)   np.lexsort((rows, key)): ascending (key, row)
    cases()                 [Case(name, pos, bits, grid, faces)]  grid: (origin[3], range) or None; faces (F, 3) uint32 or None"""
import collections

import numpy as np

TILE = 1024                 # DSA_ENCODE_ORDER_TILE (tests/test_encode_order_abi.py holds it against the header)
Case = collections.namedtuple("Case", "name pos bits grid faces")


def morton_key(q, bits):
    q = (np.asarray(q).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)          # uint32(q)
    key = np.zeros(len(q), np.uint64)
    for b in range(bits):
        for c in range(3):
            key |= ((q[:, c] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - c)
    return key


def morton_order(q, bits):
    key = morton_key(q, bits)
    return np.lexsort((np.arange(len(key)), key)).astype(np.uint32)


def height_field(nx, ny, seed):
    """nx * ny points of a smooth height field over the unit square, rows shuffled."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0, 1, nx, dtype=np.float32), np.linspace(0, 1, ny, dtype=np.float32))
    z = 0.15 * np.sin(7 * x) * np.cos(5 * y) + 0.05 * np.sin(23 * x * y)
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    return np.ascontiguousarray(pos[rng.permutation(len(pos))])


def random_cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def size_guard():
    """The shuffled 200 x 250 height field of the size bound (11 bits)."""
    return height_field(200, 250, 7)


SIZES = [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 70001]
PASS_BITS = [1, 2, 8, 11, 14, 16, 20]          # 1, 1, 3, 5, 6, 6 and 8 passes


def sized():
    return [Case("size-%d" % n, random_cloud(n, 100 + k), 11, None, None) for k, n in enumerate(SIZES)]


def passes():
    pos = random_cloud(3000, 5)
    return [Case("bits-%d" % b, pos, b, None, None) for b in PASS_BITS]


def degenerate():
    rng = np.random.default_rng(11)
    n = 1500
    same = np.tile(np.float32([0.25, -3.0, 7.5]), (n, 1))
    two = np.where((np.arange(n) % 2)[:, None] == 0, np.float32([0, 0, 0]), np.float32([1, 1, 1])).astype(np.float32)
    out = [Case("identical", same, 11, None, None), Case("alternating", two, 11, None, None)]
    for c, axis in enumerate("xyz"):
        p = np.zeros((n, 3), np.float32)
        p[:, c] = rng.random(n).astype(np.float32)
        # (own bounds: the range is this axis's extent, the other two quantise to 0)
        out.append(Case("along-" + axis, p, 14, None, None))
    half = random_cloud(n // 2, 12)
    out.append(Case("half-duplicates", np.concatenate([half, half[rng.permutation(len(half))]]), 11, None, None))
    return out


def gridded():
    pos = random_cloud(2500, 21) * np.float32(3.0) - np.float32(1.0)
    return [Case("explicit-grid", pos, 12, (np.float32([-1.5, -1.25, -1.0]), np.float32(4.5)), None)]


def meshed():
    """A small triangulated field with shuffled ids: the faces go through the inverse of the order."""
    nx, ny = 40, 33
    pos = height_field(nx, ny, 31)
    rng = np.random.default_rng(32)
    faces = rng.integers(0, len(pos), (900, 3)).astype(np.uint32)
    return [Case("mesh-%d" % len(pos), pos, 11, None, faces)]


def cases():
    return sized() + passes() + degenerate() + gridded() + meshed() + [Case("height-field", size_guard(), 11, None, None)]
