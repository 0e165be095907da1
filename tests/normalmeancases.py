"""Inputs for the tests of mean_normals (dsa_encode_normal_mean_sequential_batch; synth.merge_mean_normals, synth.encode_merged(
mean_normals=)): point clouds of mergecases -- integer positions on z_grid(bits) with a multiplicity per cell and shuffled rows, or
random clouds on their own bounds -- with normals designed per cell, and the rule restated in Python integers from its contract
(include/draco_mi355x.h), not from the C++.

    rdiv / vector / unit / tail / mean_code    the rule, step by step, on Python integers (math.isqrt, // floor division)
    floats_of(codes, nbits)         float32 normals that the quantiser codes as the given canonical codes: the integer vector of step 1
    canonical_codes(nbits)          every code the quantiser can give at nbits
    cases()                         [Case]: idempotence on every canonical code at 2 - 6 bits, axes and corners, zero normals, opposite
                                    pairs, sums that nearly cancel, cells across the fold and across the diamond edge, ties of rdiv,
                                    cells of 1, 2, 5 and 3 000 rows, clouds of 1 .. 2 100 points at 6 position bits, normal bits 2, 3,
                                    8, 11 and 20
    pin(case)                       (kept, row_entries, (m, 2) codes entry j must carry): q from the oracle's decode of the plain ordered
                                    stream of all n rows (the CPU coder's, no merge), held to the numpy quantiser of meshutil, the
                                    rule per cell
    dequantised(case)               the float32 normals a decoder makes of the pin's codes (the oracle's, on a stream that carries them)
    cpu_args(case) / cloud(case)    the arguments of the synth twins / the PointCloudData of the device call
The cases of one (position bits, normal bits) are one batch."""
import collections
import functools
import math

import numpy as np

import meancases as mn
import mergecases as mc
import meshutil
import oracle
import draco_sharp_amd.synth as synth

TILE = mc.TILE
BITS = mn.BITS
# normals: (n, 3) float32; nbits: normal_bits; expect: {cell: (s, t)} codes known by construction
Case = collections.namedtuple("Case", "name pos bits grid normals nbits expect")


# ---------------------------------------------------------------------------------------------------------------- the rule
def center(nbits):
    return ((1 << nbits) - 2) // 2


def rdiv(num, den):
    assert den > 0
    return (2 * num + den) // (2 * den)


def vector(s, t, nbits):
    """step 1: the integer vector of L1 norm c a code stands for"""
    c = center(nbits)
    a, b = s - c, t - c
    sg = lambda x: -1 if x < 0 else 1          # noqa: E731
    if abs(a) + abs(b) <= c:
        return (c - abs(a) - abs(b), a, b)
    return (-(abs(a) + abs(b) - c), sg(a) * (c - abs(b)), sg(b) * (c - abs(a)))


def unit(v):
    """step 2: the unit vector in Q30"""
    n2 = sum(x * x for x in v)
    length = math.isqrt(n2 << 24)
    return tuple(rdiv(x << 42, length) for x in v)


def canonical(s, t, nbits):
    mv, c = (1 << nbits) - 2, center(nbits)
    if (s, t) in ((0, 0), (0, mv), (mv, 0)):
        return mv, mv
    if s == 0 and t > c:
        return s, c - (t - c)
    if s == mv and t < c:
        return s, c + (c - t)
    if t == mv and s < c:
        return c + (c - s), t
    if t == 0 and s > c:
        return c - (s - c), t
    return s, t


def tail(i0, i1, z_negative, nbits):
    """the quantiser from i2 = center - |i0| - |i1| on"""
    mv, c = (1 << nbits) - 2, center(nbits)
    i2 = c - abs(i0) - abs(i1)
    if i2 < 0:
        i1 = i1 + i2 if i1 > 0 else i1 - i2
        i2 = 0
    if z_negative:
        i2 = -i2
    if i0 >= 0:
        s, t = i1 + c, i2 + c
    else:
        s = abs(i2) if i1 < 0 else mv - abs(i2)
        t = abs(i1) if i2 < 0 else mv - abs(i1)
    return canonical(s, t, nbits)


def mean_vector(codes, nbits):
    """steps 1 - 4: M"""
    U = [0, 0, 0]
    for s, t in codes:
        for k, x in enumerate(unit(vector(int(s), int(t), nbits))):
            U[k] += x
    return tuple(rdiv(x, len(codes)) for x in U)


def mean_code(codes, nbits):
    """the code of a cell with these rows"""
    if len(codes) == 1:
        return int(codes[0][0]), int(codes[0][1])
    c = center(nbits)
    M = mean_vector(codes, nbits)
    A = sum(abs(x) for x in M)
    if A == 0:
        return tail(c, 0, False, nbits)
    return tail(rdiv(M[0] * c, A), rdiv(M[1] * c, A), M[2] < 0, nbits)


def direction(code, nbits):
    """the float64 unit vector of a code"""
    v = np.array(vector(int(code[0]), int(code[1]), nbits), np.float64)
    return v / np.linalg.norm(v)


def canonical_codes(nbits):
    mv = (1 << nbits) - 2
    return [(s, t) for s in range(mv + 1) for t in range(mv + 1) if canonical(s, t, nbits) == (s, t)]


def floats_of(codes, nbits):
    """float32 normals the quantiser codes as `codes` (canonical ones): the integer vectors themselves, exact in float32"""
    out = np.array([vector(int(s), int(t), nbits) for s, t in codes], np.float32)
    assert np.array_equal(meshutil.oct_quantize(out, nbits), np.asarray(codes, np.int64).reshape(-1, 2))
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
def of_cells(name, sets, nbits, seed, expect=None, bits=BITS):
    """a cloud whose cell j holds the rows sets[j], each a float normal (3,) -- shuffled"""
    base = mc.along_z(name, [len(s) for s in sets], bits, seed)
    normals = mn.by_cell(base, lambda j, k: np.asarray(sets[j], np.float32).reshape(k, 3), np.float32, nc=3)
    return Case(name, base.pos, base.bits, base.grid, normals, nbits, expect or {})


def idempotence():
    """every canonical code at 2 - 6 bits as a cell of 2 - 4 identical rows: the cell keeps the code"""
    out = []
    for nbits in (2, 3, 4, 5, 6):
        codes = canonical_codes(nbits)
        f = floats_of(codes, nbits)
        sets = [np.repeat(f[j:j + 1], 2 + j % 3, axis=0) for j in range(len(codes))]
        out.append(of_cells("idempotent-%d" % nbits, sets, nbits, 1100 + nbits, {j: codes[j] for j in range(len(codes))}))
    return out


AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])


def axes_and_corners(nbits):
    """the six axis normals alone, in identical pairs and mixed; the canonicalised corner and edge codes; zero input normals, which
    the quantiser codes as (1, 0, 0); opposite pairs, whose sum cancels to the code of (1, 0, 0)"""
    mv, c = (1 << nbits) - 2, center(nbits)
    x_code = (c, c)
    corners = [(mv, mv), (0, c), (c, 0), (mv, c), (c, mv)] + ([(0, 1), (mv, mv - 1), (1, mv), (mv - 1, 0)] if nbits > 2 else [])
    corners = sorted({canonical(s, t, nbits) for s, t in corners})
    cf = floats_of(corners, nbits)
    sets = [[a] for a in AXES] + [[a, a] for a in AXES] + [[a, a, a] for a in cf] + [[AXES[0], AXES[2]], [AXES[0], AXES[2], AXES[4]], [AXES[1], AXES[3], AXES[5]], [AXES[1], AXES[2]]]
    expect = {6 + k: tuple(int(x) for x in meshutil.oct_quantize(AXES[k:k + 1], nbits)[0]) for k in range(6)}
    expect.update({12 + k: corners[k] for k in range(len(corners))})
    at = len(sets)
    zero = np.float32([0, 0, 0])
    sets += [[zero, zero], [zero], [zero, AXES[0]], [zero, zero, AXES[4], AXES[4]]]
    expect.update({at: x_code, at + 1: x_code, at + 2: x_code})
    at = len(sets)
    tilted = np.float32([0.3, -0.5, 0.2])
    sets += [[AXES[0], AXES[1]], [AXES[2], AXES[3]], [AXES[4], AXES[5]], [AXES[2], AXES[3], AXES[2], AXES[3]], [tilted, -tilted]]
    expect.update({at + k: x_code for k in range(4)})
    return of_cells("axes-corners-zero-opposite-%d" % nbits, sets, nbits, 1200 + nbits, expect)


def nearly_cancelling(nbits):
    """sums that nearly cancel: a normal against its opposite moved by one code step, three normals 120 degrees apart in a plane
    with one of them a step off, two against one"""
    mv, c = (1 << nbits) - 2, center(nbits)
    step = lambda s, t: floats_of([canonical(s, t, nbits)], nbits)[0]          # noqa: E731
    w = np.float32([np.cos(2 * np.pi / 3), np.sin(2 * np.pi / 3), 0])
    # (mv - 1, mv) is one step from -x = (mv, mv), (c - 1, 0) one step from -z = (c, 0)
    sets = [[AXES[0], step(mv - 1, mv)], [AXES[4], step(c - 1, 0)], [AXES[0], w, w * np.float32([1, -1, 1])],
            [AXES[2], AXES[2], AXES[3]], [np.float32([0.6, 0.5, 0.4]), np.float32([-0.6, -0.5, -0.41])]]
    return of_cells("nearly-cancelling-%d" % nbits, sets, nbits, 1300 + nbits)


def across_the_fold(nbits):
    """x < 0 on both sides of y = 0 and of z = 0: the two codes lie in different corners of the (s, t) square, and the mean of the
    INTEGERS (s, t) points elsewhere -- toward +x.  And cells across the diamond edge x ~ 0, where the two codes lie on the two
    sides of |a| + |b| = c."""
    sets = [[np.float32([-0.8, 0.1, 0.3]), np.float32([-0.8, -0.1, 0.3])], [np.float32([-0.8, 0.3, 0.1]), np.float32([-0.8, 0.3, -0.1])],
            [np.float32([-0.9, 0.05, 0.05]), np.float32([-0.9, -0.05, -0.05]), np.float32([-0.9, 0.05, -0.05]), np.float32([-0.9, -0.05, 0.05])],
            [np.float32([0.02, 0.6, 0.4]), np.float32([-0.02, 0.6, 0.4])], [np.float32([0.03, -0.7, 0.2]), np.float32([-0.03, -0.7, 0.2]), np.float32([-0.03, -0.7, 0.25])],
            [np.float32([0.0, 0.5, 0.5]), np.float32([-0.05, 0.5, 0.5])]]
    return of_cells("fold-and-diamond-edge-%d" % nbits, sets, nbits, 1400 + nbits)


def searched(nbits, seed, wanted, tries=5000):
    """the first pair of random canonical codes (of a seeded sequence) for which wanted(codes) holds"""
    rng = np.random.default_rng(seed)
    mv = (1 << nbits) - 2
    for _ in range(tries):
        pair = [canonical(int(s), int(t), nbits) for s, t in rng.integers(0, mv + 1, (2, 2))]
        if wanted(pair):
            return pair
    raise AssertionError("no such pair")


def tie_in_step_4(pair, nbits):
    U = [sum(u) for u in zip(*[unit(vector(s, t, nbits)) for s, t in pair])]
    return any(x % 2 for x in U)                 # cnt = 2: U_k odd is U_k / 2 at a half


def tie_in_step_5(pair, nbits):
    M, c = mean_vector(pair, nbits), center(nbits)
    A = sum(abs(x) for x in M)
    return A != 0 and any((2 * M[k] * c + A) % (2 * A) == 0 and (2 * M[k] * c) % (2 * A) != 0 for k in (0, 1))


def ties(nbits):
    """cells of two rows whose sum has an odd component (step 4 rounds a half), and whose mean vector scaled to the centre lies at a
    half (step 5 rounds a half): +x and +y at every bit count are of the second kind; searched pairs of both kinds where the
    bits have some"""
    # (at 2 bits every unit vector is an axis, +-2^30 exactly, and at 3 bits no sum of two is odd either)
    pairs = [searched(nbits, 1500 + k, lambda p: tie_in_step_4(p, nbits)) for k in range(3)] if nbits >= 8 else []
    sets = [floats_of(p, nbits) for p in pairs] + [[AXES[0], AXES[2]], [AXES[0], AXES[4]], [AXES[1], AXES[5]]]
    assert tie_in_step_5([tuple(int(x) for x in r) for r in meshutil.oct_quantize(np.float32([AXES[0], AXES[2]]), nbits)], nbits)
    if nbits == 3:                               # (searched pairs beside the axes; from 8 bits on random pairs rarely hold one)
        sets += [floats_of(searched(nbits, 1600 + k, lambda p: tie_in_step_5(p, nbits)), nbits) for k in range(3)]
    return of_cells("ties-%d" % nbits, sets, nbits, 1500 + nbits)


def cone(rng, k, axis, spread):
    v = np.asarray(axis, np.float64) + rng.normal(size=(k, 3)) * spread
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def run_lengths(nbits):
    """cells of 1, 2, 5 and 3 000 rows (the long run spans three tiles), normals in a cone around an axis of the cell and, in the
    last cells, all over the sphere"""
    rng = np.random.default_rng(1700 + nbits)
    mults = [1, 2, 5, 3000, 1, 5, 2, 64, 65]
    sets = [cone(rng, k, rng.normal(size=3), 0.3 if j < 6 else 5.0) for j, k in enumerate(mults)]
    return of_cells("runs-1-2-5-3000-%d" % nbits, sets, nbits, 1700 + nbits)


def tile_with_no_head(nbits):
    """mergecases' run whose middle tile has no head, with normals"""
    base = next(c for c in mc.boundary_runs(BITS) if c.name == "tile-with-no-head")
    rng = np.random.default_rng(1800 + nbits)
    normals = mn.by_cell(base, lambda j, k: cone(rng, k, [(-1) ** j, 0.4, 0.2 * j], 0.5), np.float32, nc=3)
    return Case("tile-with-no-head-%d" % nbits, base.pos, base.bits, base.grid, normals, nbits, {})


SIZES = (1, 2, 63, 64, 65, 1025, 2100)


def small_clouds(nbits=8):
    """clouds of 1 .. 2 100 points at 6 position bits on their own bounds, about half of the rows repeating a position, normals that
    follow the position with noise"""
    out = []
    for n in SIZES:
        base = mc.half_duplicated(n, 1900 + n, bits=6)
        rng = np.random.default_rng(1950 + n)
        v = base.pos.astype(np.float64) - 0.5 + rng.normal(size=(n, 3)) * 0.4
        v[np.linalg.norm(v, axis=1) < 1e-3] = [0.0, 0.0, 1.0]
        out.append(Case("cloud-%d" % n, base.pos, base.bits, base.grid, (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32), nbits, {}))
    return out


NORMAL_BITS = (2, 3, 8, 11, 20)


@functools.lru_cache(maxsize=None)
def cases():
    out = idempotence()
    for nbits in NORMAL_BITS:
        out += [axes_and_corners(nbits), nearly_cancelling(nbits), across_the_fold(nbits), ties(nbits), run_lengths(nbits)]
    out += [tile_with_no_head(8), tile_with_no_head(20)] + small_clouds()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def named(name):
    return next(c for c in cases() if c.name == name)


def groups():
    """the cases of one (position bits, normal bits) are a batch: [((bits, nbits), [Case])]"""
    keys = sorted({(c.bits, c.nbits) for c in cases()})
    return [(k, [c for c in cases() if (c.bits, c.nbits) == k]) for k in keys]


def cpu_args(case, rows=None, **more):
    """the arguments of synth.encode_merged / encode_cell_parts / encode_lod_parts / encode_ordered for the case (rows: a shuffle;
    more: further attributes)"""
    take = (lambda a: a) if rows is None else (lambda a: None if a is None else np.ascontiguousarray(a[rows]))
    opt = synth.options(pos_bits=case.bits, normal_bits=case.nbits)
    out = dict(pos=take(case.pos), normals=take(case.normals), opt=opt, pos_grid=None if case.grid is None else synth.grid(case.grid[0], case.grid[1]))
    out.update({k: take(v) for k, v in more.items()})
    return out


def cloud(case, rows=None, **more):
    """the PointCloudData of the device call (rows: a shuffle of the input rows; more: further arguments)"""
    import draco_sharp_amd as dsa
    take = (lambda a: a) if rows is None else (lambda a: None if a is None else np.ascontiguousarray(a[rows]))
    return dsa.PointCloudData(take(case.pos), normals=take(case.normals), position_grid=None if case.grid is None else dsa.Grid(case.grid[0], float(case.grid[1])), **more)


@functools.lru_cache(maxsize=None)
def _pin(name):
    case = named(name)
    kept, cells, _ = mc.pin(case.pos, case.bits, case.grid)
    data, perm = synth.encode_ordered(geometry=0, **cpu_args(case))
    dec = oracle.decode(data)
    assert dec.num_points == len(case.pos) and len(dec.attributes) == 2
    q = np.zeros((len(case.pos), 2), np.int64)
    q[perm] = dec.attributes[1].portable
    assert np.array_equal(q, meshutil.oct_quantize(case.normals, case.nbits)), name          # the integers the plain call codes
    order = np.argsort(cells, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=len(kept)))])
    want = np.array([mean_code(q[order[bounds[j]:bounds[j + 1]]], case.nbits) for j in range(len(kept))], np.int64).reshape(-1, 2)
    for j, code in case.expect.items():
        assert tuple(want[j]) == tuple(code), (name, j, tuple(want[j]), code)          # the pin agrees with what the case was built to give
    return kept, cells, want, q


def pin(case):
    """(kept, row_entries, (m, 2) codes entry j carries)"""
    return _pin(case.name)[:3]


def codes_of_rows(case):
    """(n, 2) the codes the plain call codes for the rows"""
    return _pin(case.name)[3]


@functools.lru_cache(maxsize=None)
def _dequantised(name):
    case = named(name)
    kept, cells, want = pin(case)
    stream = synth.encode_grid(case.pos[kept], None, normals=case.normals[kept], opt=synth.options(pos_bits=case.bits, normal_bits=case.nbits), form=0, geometry=0,
                               pos_grid=synth.bounds_grid(case.pos) if case.grid is None else synth.grid(case.grid[0], case.grid[1]), normal_portable=want.astype(np.int32))
    dec = oracle.decode(stream)
    assert np.array_equal(dec.attributes[1].portable, want)
    return np.ascontiguousarray(dec.attributes[1].values, np.float32).reshape(-1, 3)


def dequantised(case):
    """(m, 3) float32: what a decoder makes of the pin's codes, entry by entry"""
    return _dequantised(case.name)


def decoded(streams):
    """the normals' codes of the streams' entries joined, through the oracle"""
    return np.concatenate([oracle.decode(s).attributes[1].portable for s in streams]).astype(np.int64)
