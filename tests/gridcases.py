"""Inputs for the quantisation grids of the encoder (dsa_encode_grid_batch, synth.encode_grid) and a numpy pin of what a grid
means, written from the contract and from neither coder:

    q = floor((v - origin[c]) * (max_q / range) + 0.5), every step rounded to float32, max_q = 2^bits - 1
    v' = origin[c] + q * (range / max_q)                                      (what a decoder gives back)
    a shared grid: minimum per component over all rows of every array of the group, range the largest extent, 1 if that is 0

numpy only; everything is deterministic (seeded)."""
import collections

import numpy as np

from meshutil import quantize

POS_BITS, UV_BITS = 11, 10
Case = collections.namedtuple("Case", "name pos faces uvs")


def grid_faces(nx, ny):
    """faces of an nx x ny vertex grid, row major, oriented"""
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            f += [[a, a + 1, a + nx + 1], [a, a + nx + 1, a + nx]]
    return np.array(f, np.uint32)


def heightfield(n=17, seed=11):
    """(n, n, 3) float32: a jittered heightfield over the unit square"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, n, dtype=np.float32), np.linspace(0, 1, n, dtype=np.float32), indexing="ij")
    z = (0.2 * np.sin(5 * x) * np.cos(3 * y) + 0.05 * rng.standard_normal((n, n))).astype(np.float32)
    return np.stack([x, y, z], axis=-1).astype(np.float32)


def tiles(n=17, seed=11):
    """A 2 x 2 set of tiles cut from one heightfield of n x n vertices (n odd): tile (r, c) holds rows r*h .. r*h + h and columns
    likewise, h = (n - 1) / 2, so that the border rows and columns are the same floats, bit for bit, in the tiles that share
    them.  Returns [(Case, index), ...]: index (h + 1, h + 1, 2) the (row, column) of every tile vertex in the whole field.  The
    jitter makes the tiles' own bounds differ."""
    field = heightfield(n, seed)
    h = (n - 1) // 2
    out = []
    for r in range(2):
        for c in range(2):
            rows, cols = np.arange(r * h, r * h + h + 1), np.arange(c * h, c * h + h + 1)
            pos = np.ascontiguousarray(field[np.ix_(rows, cols)].reshape(-1, 3))
            index = np.stack(np.meshgrid(rows, cols, indexing="ij"), axis=-1)
            uv = np.ascontiguousarray(pos[:, :2])
            out.append((Case("tile-%d-%d" % (r, c), pos, grid_faces(h + 1, h + 1), uv), index.reshape(-1, 2)))
    return out


def voxel(n=9, seed=3):
    """A voxel-corner mesh: every coordinate an integer 0 .. 15 (a stepped heightfield over an n x n lattice)."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    z = rng.integers(0, 16, (n, n))
    z[0, 0], z[-1, -1] = 0, 15
    pos = np.stack([i, j, z], axis=-1).reshape(-1, 3).astype(np.float32)
    return Case("voxel", pos, grid_faces(n, n), None)


def texel(n=9, seed=5):
    """A grid whose texture coordinates are whole texels of a 1024-texel atlas, k / 1024."""
    rng = np.random.default_rng(seed)
    pos = np.ascontiguousarray(heightfield(n, seed).reshape(-1, 3))
    uv = (rng.integers(0, 1024, (n * n, 2)).astype(np.float32) / np.float32(1024.0)).astype(np.float32)
    return Case("texel", pos, grid_faces(n, n), uv)


def own_bounds(vals):
    """(origin, range) of an array's own bounds, the grid every encoder call takes by default"""
    vals = np.asarray(vals, np.float32).reshape(len(vals), -1)
    mn = vals.min(axis=0).astype(np.float32)
    rng = np.float32((vals.max(axis=0).astype(np.float32) - mn).max())
    return mn, (np.float32(1.0) if rng == 0 else rng)


def shared_bounds(arrays):
    """(origin, range) of the union of the arrays: numpy's minimum and maximum over their concatenation"""
    return own_bounds(np.concatenate([np.asarray(a, np.float32).reshape(len(a), -1) for a in arrays]))


def pin(vals, origin, rng, bits):
    """the integers of `vals` on the grid (int64, not clipped: a value outside 0 .. max_q is off the grid)"""
    vals = np.asarray(vals, np.float32)
    return quantize(vals.reshape(len(vals), -1), np.asarray(origin, np.float32)[:vals.reshape(len(vals), -1).shape[1]], rng, bits)


def dequantize(q, origin, rng, bits):
    """what a decoder returns for the integers q: origin + q * (range / max_q) in float32"""
    delta = np.float32(np.float32(rng) / np.float32((1 << bits) - 1))
    return (np.asarray(origin, np.float32) + (np.asarray(q).astype(np.float32) * delta).astype(np.float32)).astype(np.float32)


def first_bad_row(vals, origin, rng, bits):
    """(row, finite) of the refusal a grid gives an array, or None: the smallest row with a value that is not finite, else the
    smallest row whose integer leaves 0 .. max_q"""
    vals = np.asarray(vals, np.float32).reshape(len(vals), -1)
    bad = np.flatnonzero(~np.isfinite(vals).all(axis=1))
    if len(bad):
        return int(bad[0]), False
    with np.errstate(all="ignore"):
        q = pin(vals, origin, rng, bits)
    off = np.flatnonzero(((q < 0) | (q > (1 << bits) - 1)).any(axis=1))
    return (int(off[0]), True) if len(off) else None


def refusal(name, row, finite):
    """the message of such a mesh (include/draco_mi355x.h, dsa_quantization_grid)"""
    return "%s: row %d %s" % (name, row, "lies off the quantisation grid" if finite else "is not finite")


def damaged(what, n=9, seed=7):
    """The heightfield of `texel` with one position changed, and the grid of the undamaged field (origin, range): "off": a value
    just off the grid (one cell below the origin); "edge": a value that rounds onto the last cell (inside); "nan" / "inf": a
    value that is not finite."""
    c = texel(n, seed)
    origin, rng = own_bounds(c.pos)
    pos = c.pos.copy()
    cell = np.float32(rng / np.float32((1 << POS_BITS) - 1))
    row = 3 * n + 4
    if what == "off":
        pos[row, 2] = origin[2] - cell
    elif what == "edge":
        pos[row, 0] = origin[0] + rng + np.float32(0.49) * cell
    elif what == "nan":
        pos[row, 1] = np.nan
    elif what == "inf":
        pos[row, 1] = -np.inf
    else:
        raise ValueError(what)
    return Case(what, pos, c.faces, c.uvs), (origin, rng), row


def cloud_chunks(points=200, seed=9):
    """A point cloud in four chunks: a helix cut into four pieces of unequal extent."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 6 * np.pi, 4 * points).astype(np.float32)
    pos = np.stack([np.cos(t) * (1 + 0.1 * t), np.sin(t) * (1 + 0.1 * t), 0.3 * t], axis=-1).astype(np.float32)
    pos += (0.01 * rng.standard_normal(pos.shape)).astype(np.float32)
    return [np.ascontiguousarray(pos[k * points:(k + 1) * points]) for k in range(4)]
