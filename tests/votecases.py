"""Inputs for the tests of vote_attributes (dsa_encode_vote_sequential_batch; synth.merge_votes, synth.encode_merged(vote_attributes=)):
point clouds of mergecases.along_z -- integer positions on z_grid(bits), a multiplicity per cell, shuffled rows -- with label values
designed per cell, and the contract restated in Python: collections.Counter per cell, the highest count, then min of the tuples.

    cases()                         [Case]: ties, pairs, a late winner, a spread majority, every run shape of
                                    mergecases.boundary_runs, crowded tables, a mask mixed with mean_attributes
    refusals()                      [(Case, whole call, words of the device's message, words of the twin's)]: three components,
                                    normals, positions, a missing attribute, the same bit in both masks
    pin(case)                       per attribute of the stream the (m, nc) signed integers entry j must carry: q from the oracle's
                                    decode of the plain ordered stream of all n rows (the CPU coder's, no merge); for a voted
                                    attribute the most frequent tuple of the cell, the smallest of those with equally many rows;
                                    for an averaged one meancases.mean; q[kept[j]] otherwise
    cpu_args(case) / cloud(case)    the arguments of the synth twins / the PointCloudData of the device call (meancases')
Every case is on one position grid, so that the cases of a mask are one batch."""
import collections
import functools

import numpy as np

import meancases as mn
import mergecases as mc
import oracle
import draco_sharp_amd.synth as synth

TILE = mc.TILE
BITS = mn.BITS
# as meancases.Case, with `vote` and `mean` the two masks over the attributes of the stream
Case = collections.namedtuple("Case", "name pos bits grid normals uvs generic extras vote mean expect")

by_cell, attributes, cpu_args, cloud = mn.by_cell, mn.attributes, mn.cpu_args, mn.cloud


def make(base, normals=None, uvs=None, generic=None, extras=(), vote=0, mean=0, expect=None, name=None):
    return Case(name or base.name, base.pos, base.bits, base.grid, normals, uvs, generic, list(extras), vote, mean, expect or {})


def signed(q):
    """integers as the coder holds them: 32 bits, signed (a uint32 at or above 2^31 is negative)"""
    return ((np.asarray(q).astype(np.int64) + 2**31) % 2**32) - 2**31


def ties():
    """{3,5} -> 3, {5,3,5,3} -> 3, {-1,0} -> -1, {-128,127} -> -128, {2,2,1} -> 2, {7} -> 7: among equally many rows the smallest
    SIGNED value"""
    sets = [[3, 5], [5, 3, 5, 3], [-1, 0], [-128, 127], [2, 2, 1], [7]]
    base = mc.along_z("ties", [len(s) for s in sets], BITS, 1001)
    want = np.array([[3], [3], [-1], [-128], [2], [7]], np.int64)
    vals = lambda dt: by_cell(base, lambda j, k: sets[j], dt)          # noqa: E731
    return make(base, extras=[(vals(np.int8), 0, None), (vals(np.int16), 0, None), (vals(np.int32), 0, None)], vote=0b1110, expect={1: want, 2: want, 3: want})


def pairs():
    """two components: equal counts that differ only in component 1; that differ in component 0 with the opposite order in component
    1; two tuples twice each; a majority that is not the smallest.  And uint32 values above 2^31, negative as coded -- all of them,
    and 2^20 away from 2^31 itself: the wrap transform of the format works in 32 bits, it holds no range of 2^31 and more (such
    values cannot stand beside small ones) and its corrections overflow at the very end of the range."""
    sets = [[(4, 9), (4, -2)], [(1, 100), (2, -100)], [(-5, 0), (3, -7), (-5, 0), (3, -7)], [(0, 0), (0, 1), (0, 1)], [(-3, 3)]]
    top = 2**31 + 2**20
    wide = [[top + 1, top + 5], [top + 70000, top], [top + 9, top + 7, top + 9, top + 7], [top + 3, top + 2, top + 3], [top]]
    base = mc.along_z("pairs", [len(s) for s in sets], BITS, 1002)
    want = np.array([[4, -2], [1, 100], [-5, 0], [0, 1], [-3, 3]], np.int64)
    want_wide = signed(np.array([[top + 1], [top], [top + 7], [top + 3], [top]]))
    two = lambda dt: by_cell(base, lambda j, k: sets[j], dt, nc=2)          # noqa: E731
    return make(base, extras=[(two(np.int16), 0, None), (two(np.int32), 0, None), (by_cell(base, lambda j, k: wide[j], np.uint32), 0, None)], vote=0b1110,
                expect={1: want, 2: want, 3: want_wide})


def late_winner():
    """cell 0, sorted entries 0 .. 129: 64 distinct values fill the first step, then 66 rows of one value -- the winner is absent
    from the first step of its run, and in the third step it is the first lane's"""
    base = mc.along_z("late-winner", [130, 3, 70], BITS, 1003)
    vals = by_cell(base, lambda j, k: list(range(1, 65)) + [200] * 66 if j == 0 else ([9, 8, 9] if j == 1 else [j] * k), np.uint16)
    return make(base, extras=[(vals, 0, None)], vote=0b10, expect={1: np.array([[200], [9], [2]], np.int64)})


def spread_majority():
    """a winner whose rows lie one in every step of a run of five steps, never in its first lane: five single inserts against values
    that come twice"""
    base = mc.along_z("spread-majority", [320, 2], BITS, 1004)
    run = [1000 + i % 160 for i in range(320)]
    for s in range(5):
        run[64 * s + 7 + s] = 7
    vals = by_cell(base, lambda j, k: run if j == 0 else [4, 4], np.uint16)
    return make(base, extras=[(vals, 0, None)], vote=0b10, expect={1: np.array([[7], [4]], np.int64)})


def run_shapes():
    """a uint8 label out of four and an int16 pair out of six, both voted, over every run shape: multiplicity 1 throughout, the runs
    of mergecases.boundary_runs (ending at / beginning at / straddling a 64-entry step and a 1024-entry tile), one run of 2 TILE + 1
    identical rows, one point"""
    out = []
    bases = [mc.along_z("distinct-65", np.ones(65, np.int64), BITS, 1006), mc.along_z("distinct-%d" % (TILE + 1), np.ones(TILE + 1, np.int64), BITS, 1007)]
    bases += mc.boundary_runs(BITS) + [mc.along_z("one-point", [1], BITS, 1009)]
    for k, base in enumerate(bases):
        rng = np.random.default_rng(1010 + k)
        n = len(base.pos)
        pair = np.stack([rng.integers(-1, 2, n), rng.integers(-300, -298, n)], axis=1).astype(np.int16)
        out.append(make(base, extras=[(rng.integers(0, 4, (n, 1)).astype(np.uint8), 0, None), (pair, 0, None)], vote=0b110))
    base = mc.along_z("identical-%d" % (2 * TILE + 1), [2 * TILE + 1], BITS, 1008)
    n = len(base.pos)
    out.append(make(base, extras=[(np.full((n, 1), 33, np.uint8), 0, None), (np.tile(np.int16([[-2, 5]]), (n, 1)), 0, None)], vote=0b110,
                    expect={1: np.array([[33]], np.int64), 2: np.array([[-2, 5]], np.int64)}))
    return out


def crowded_tables():
    """one cell of 3 000 rows with 3 000 distinct values: the table at its highest load, probes that wrap; one cell of 3 000 rows
    over three values, 1 000 each: a tie across tiles; a cloud whose every cell holds the same two values"""
    rng = np.random.default_rng(1020)
    one = mc.along_z("all-distinct-3000", [3000], BITS, 1021)
    distinct = (rng.permutation(3000) + 100).astype(np.uint16).reshape(-1, 1)
    three = mc.along_z("three-way-tie-3000", [3000], BITS, 1022)
    thirds = rng.permutation(np.repeat(np.uint16([40000, 17, 900]), 1000)).reshape(-1, 1)
    same = mc.along_z("same-two-values", [2] * 600, BITS, 1023)
    two = by_cell(same, lambda j, k: [9, 4] if j % 2 else [4, 9], np.uint16)
    return [make(one, extras=[(distinct, 0, None)], vote=0b10, expect={1: np.array([[100]], np.int64)}),
            make(three, extras=[(thirds, 0, None)], vote=0b10, expect={1: np.array([[17]], np.int64)}),
            make(same, extras=[(two, 0, None)], vote=0b10, expect={1: np.full((600, 1), 4, np.int64)})]


def mixed_mask():
    """the stream: 0 positions, 1 texture coordinates (voted), 2 a uint8 x 4 colour (mean), 3 a uint8 label (voted), 4 an int16 (neither:
    row kept[j]), 5 a float at 12 bits on an explicit grid (voted)"""
    rng = np.random.default_rng(1030)
    base = mc.along_z("mixed-mask", rng.integers(1, 9, 200), BITS, 1030)
    n = len(base.pos)
    uvs = np.float32([[0.0, 1.0], [0.25, 0.5], [1.0, 0.0], [0.25, 0.75]])[rng.integers(0, 4, n)]
    floats = np.float32([-1.0, -0.5, 0.125, 1.75])[rng.integers(0, 4, n)].reshape(-1, 1)
    return make(base, uvs=uvs, generic=rng.integers(0, 256, (n, 4)).astype(np.uint8),
                extras=[(rng.integers(0, 5, (n, 1)).astype(np.uint8), 0, None), (rng.integers(-32768, 32768, (n, 1)).astype(np.int16), 0, None), (floats, 12, ([-1.5], 4.0))],
                vote=0b101010, mean=0b100)


@functools.lru_cache(maxsize=None)
def cases():
    return tuple([ties(), pairs(), late_winner(), spread_majority()] + run_shapes() + crowded_tables() + [mixed_mask()])


@functools.lru_cache(maxsize=None)
def refusals():
    """clouds whose masks are refused: by the device per cloud, in one slot, the message naming vote_attributes and the attribute --
    or, for a bit in both masks, the whole call before any cloud is looked at; by the twin with an exception"""
    rng = np.random.default_rng(1040)
    base = mc.along_z("refused", [2, 1, 3], BITS, 1040)
    n = len(base.pos)
    label, colour = (rng.integers(0, 4, (n, 1)).astype(np.uint8), 0, None), (rng.integers(0, 256, (n, 3)).astype(np.uint8), 0, None)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    return ((make(base, extras=[colour], vote=0b10, name="three-components"), False, ("vote_attributes 0x2", "attribute 1", "3 components", "64 bits"), "1 - 2 integers"),
            (make(base, normals=normals, extras=[label], vote=0b10, name="normals"), False, ("vote_attributes 0x2", "attribute 1", "normals", "not built"), "positions and normals"),
            (make(base, extras=[label], vote=0b11, name="positions"), False, ("vote_attributes 0x3", "attribute 0", "positions"), "positions and normals"),
            (make(base, extras=[label], vote=0b100, name="missing-attribute"), False, ("vote_attributes 0x4", "attribute 2", "has 2 attributes"), "does not have"),
            (make(base, extras=[label], vote=0b10, mean=0b10, name="both-masks"), True, ("vote_attributes 0x2 and mean_attributes 0x2 share a bit",), "share a bit"))


def named(name):
    return next(c for c in cases() if c.name == name)


def groups():
    """the cases of one pair of masks are a batch: [((vote, mean), [Case])]"""
    keys = sorted({(c.vote, c.mean) for c in cases()})
    return [(k, [c for c in cases() if (c.vote, c.mean) == k]) for k in keys]


def vote(rows):
    """the rule: the tuple the most rows have, the smallest of those with equally many"""
    count = collections.Counter(tuple(int(x) for x in r) for r in rows)
    most = max(count.values())
    return min(t for t, k in count.items() if k == most)


@functools.lru_cache(maxsize=None)
def _pin(name):
    case = named(name)
    kept, cells, _ = mc.pin(case.pos, case.bits, case.grid)
    data, perm = synth.encode_ordered(geometry=0, **cpu_args(case))
    dec = oracle.decode(data)
    assert dec.num_points == len(case.pos) and len(dec.attributes) == 1 + len(attributes(case))
    order = np.argsort(cells, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=len(kept)))])
    out = {}
    for a, _, _ in attributes(case):
        q = np.zeros(dec.attributes[a].portable.shape, np.int64)
        q[perm] = signed(dec.attributes[a].portable)
        rows = lambda j: q[order[bounds[j]:bounds[j + 1]]]          # noqa: E731
        if (case.vote >> a) & 1:
            out[a] = np.array([vote(rows(j)) for j in range(len(kept))], np.int64)
        elif (case.mean >> a) & 1:
            out[a] = np.array([[mn.mean(rows(j)[:, c]) for c in range(q.shape[1])] for j in range(len(kept))], np.int64)
        else:
            out[a] = q[kept]
    for a, want in case.expect.items():
        assert np.array_equal(out[a], want), (name, a)          # the pin agrees with what the case was built to give
    return kept, cells, out


def pin(case):
    """(kept, row_entries, {attribute of the stream: (m, nc) signed integers entry j carries})"""
    return _pin(case.name)


def decoded(streams):
    """per attribute beyond the positions the signed integers of the streams' entries joined, through the oracle"""
    return {a: signed(v) for a, v in mn.decoded(streams).items()}
