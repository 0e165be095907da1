"""lod_base_bits on the CPU: synth.lod_parts against the contract restated in numpy (lodcases.pin: keys, unique, the level rule, the
stable partition, the parts of every level), what the levels mean -- levels 0 .. l are exactly one point per occupied cell of the
grid with D + l bits per axis, the cell's first point in Morton order -- the slot bound, D = B against synth.encode_cell_parts, and
every stream of synth.encode_lod_parts against synth.encode_grid of the gathered rows on the grid of ALL rows, which is what the
contract says the streams are."""
import numpy as np
import pytest

import lodcases as lc
import ordercases as oc
import draco_sharp_amd.synth as synth


def grid_of(c):
    return None if c.grid is None else synth.grid(c.grid[0], c.grid[1])


CASES = lc.cases() + [lc.large()]
PINS = {c.name: lc.pin(c) for c in CASES}          # computed once, read by every test


def counts_of(c):
    return np.bincount(PINS[c.name].kept_level, minlength=c.bits - c.lod_base_bits + 1).tolist()


def test_the_cases_are_what_they_say():
    T = lc.TILE
    assert len({c.name for c in CASES}) == len(CASES)
    by = {c.name: c for c in CASES}
    edges = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1]
    assert lc.EDGES == edges
    for m in edges:            # every edge as the population of a first, a middle and a last level
        assert m == 0 or counts_of(by["pop-first-%d" % m])[0] == m
        assert counts_of(by["pop-middle-%d" % m])[1] == m and counts_of(by["pop-last-%d" % m])[-1] == m
    assert {c.part_cells for c in CASES} >= {1, 2, 63, 64, 65, T - 1, T, T + 1, lc.INT32_MAX}
    sizes = {int(hi - lo) for c in CASES for lo, hi in PINS[c.name].ranges}
    assert sizes >= {1, 2, 63, 64, 65, T - 1, T, T + 1}                    # ... and as the size of a part
    assert all(counts_of(by["sizes-N%d" % N]) == [150, T + 1, 2 * T + 1] for N in (63, 64, 65, T - 1, T, T + 1, lc.INT32_MAX))
    # where level 1 begins in lod order
    assert counts_of(by["boundary-inside-a-step"])[0] % 64 not in (0,) and counts_of(by["boundary-on-a-step-edge"])[0] == 128
    assert counts_of(by["boundary-on-a-tile-edge"])[0] == T and counts_of(by["boundary-on-two-tile-edges"])[:2] == [T, T]
    # ... and in kept order the levels lie mixed: a 64-entry step and a tile hold several
    for name in ("boundary-on-a-tile-edge", "sizes-N64", "large"):
        lv = PINS[name].kept_level
        assert len(set(lv[:64].tolist())) >= 2 and len(set(lv[T - 32:T + 32].tolist())) >= 2, name
    assert counts_of(by["empty-level-in-the-middle"]) == [40, 0, 90, 200] and counts_of(by["two-empty-levels"]) == [5, 0, 0, 30]
    for name in ("all-in-level-0", "all-in-level-0-N-max"):
        assert by[name].lod_base_bits == by[name].bits and len(counts_of(by[name])) == 1
    assert counts_of(by["one-cell"]) == [1, 0, 0, 0] and len(by["one-cell"].pos) == 5 and len(by["one-point"].pos) == 1
    assert by["own-bounds"].grid is None and all(c.grid is not None and c.grid[1] == (1 << c.bits) - 1 for c in CASES if c.name != "own-bounds")
    # every cell twice (the first three times): the two rows of a cell lie on both sides of the tile edge of the SORTED order
    c = by["every-cell-twice"]
    key = np.sort(oc.morton_key(lc.quantised(c), c.bits))
    assert len(key) == 2 * 1150 + 1 and key[T - 1] == key[T] and key[2 * T - 1] == key[2 * T] and len(np.unique(key)) == 1150
    c = by["many-empty-slots"]
    assert lc.slots(c) == 45 and len(PINS[c.name].ranges) == 13
    c = by["large"]
    assert len(c.pos) == 70001 and (c.bits, c.lod_base_bits, c.part_cells) == (11, 7, 300) and min(counts_of(c)) > 300 and len(PINS["large"].kept) < 60000
    assert all(len(c.pos) <= 70001 for c in CASES)


def test_the_twin_is_the_pin():
    for c in CASES:
        got = synth.lod_parts(c.pos, c.bits, c.part_cells, c.lod_base_bits, grid_of(c))
        want = PINS[c.name]
        assert all(g.dtype == np.uint32 for g in got[:4]) and got[4].dtype == got[5].dtype == np.int32, c.name
        for g, w in zip(got, want[:6]):
            assert g.shape == w.shape and np.array_equal(g, w), c.name
        lod, cells, ranges, level = got[:4]
        # a permutation of kept, stable within a level; every row finds the lod entry of its cell
        assert np.array_equal(np.sort(lod), np.sort(want.kept)) and np.array_equal(lod[cells], want.kept[np.searchsorted(oc.morton_key(lc.quantised(c)[want.kept], c.bits),
                                                                                                                       oc.morton_key(lc.quantised(c), c.bits))]), c.name
        size = ranges[:, 1].astype(np.int64) - ranges[:, 0]
        assert size.min() >= 1 and size.max() <= c.part_cells and np.all(np.diff(level.astype(np.int64)) >= 0), c.name
        assert ranges[0, 0] == 0 and ranges[-1, 1] == len(lod) and np.array_equal(ranges[1:, 0], ranges[:-1, 1]), c.name
        for l in set(level.tolist()):          # the rule of part_cells applied to the level's points
            s = size[level == l]
            assert len(s) == -(-int(s.sum()) // c.part_cells) and s.max() - s.min() <= 1, (c.name, l)


def test_levels_0_to_l_are_one_point_per_cell_and_the_first_of_it():
    for c in CASES:
        p = PINS[c.name]
        key = oc.morton_key(lc.quantised(c), c.bits)
        B, D = c.bits, c.lod_base_bits
        counts = np.bincount(p.kept_level, minlength=B - D + 1)
        for l in range(B - D + 1):
            shift = np.uint64(3 * (B - D - l))
            chosen = key[p.lod[:counts[:l + 1].sum()]]
            cells, first = np.unique(key >> shift, return_index=True)          # (every occupied cell; np.unique: ascending)
            smallest = np.array([key[(key >> shift) == cell].min() for cell in cells]) if len(cells) < 300 else None
            assert len(chosen) == len(cells) and np.array_equal(np.sort(chosen >> shift), cells), (c.name, l)
            # the chosen point is the smallest key of its cell: the cell's first point in Morton order
            order = np.argsort(key, kind="stable")
            low = key[order][np.searchsorted(key[order] >> shift, cells)]
            assert np.array_equal(np.sort(chosen), low) and (smallest is None or np.array_equal(smallest, low)), (c.name, l)
        assert counts.sum() == len(p.kept) == len(np.unique(key))


def test_the_slot_bound():
    for c in CASES:
        p = PINS[c.name]
        L = c.bits - c.lod_base_bits + 1
        live = len(set(p.level.tolist()))
        assert len(p.ranges) <= -(-len(p.kept) // c.part_cells) + live - 1 <= -(-len(c.pos) // c.part_cells) + L - 1 == lc.slots(c), c.name


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), uvs=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                extra=[synth.Extra(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)), synth.Extra(rng.random((n, 2)).astype(np.float32), quantization_bits=12)])


def test_all_points_in_level_0_are_the_streams_of_cell_parts():
    for c in [c for c in CASES if c.lod_base_bits == c.bits] + [lc.Case("large-D-is-B", lc.large().pos, 11, lc.large().grid, 4096, 11)]:
        a = attributes_of(len(c.pos), 5) if len(c.pos) < 5000 else {}
        opt = synth.options(pos_bits=c.bits)
        got = synth.encode_lod_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=c.part_cells, lod_base_bits=c.lod_base_bits, **a)
        want = synth.encode_cell_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=c.part_cells, **a)
        assert got.streams == want.streams and got.levels == 1 and not got.level.any(), c.name
        for g, w in zip(got[1:6], want[1:]):
            assert np.array_equal(g, w), c.name
    none = synth.encode_lod_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=c.part_cells, lod_base_bits=0)
    assert none.streams == want.streams and none.levels == 1


STREAMS = [c for c in CASES if c.name in ("pop-middle-65", "pop-last-1", "small-N1", "sizes-N1023", "boundary-on-a-tile-edge", "empty-level-in-the-middle", "one-cell",
                                           "own-bounds", "every-cell-twice", "many-empty-slots", "large")]


@pytest.mark.parametrize("c", STREAMS, ids=[c.name for c in STREAMS])
def test_every_stream_is_the_plain_coder_on_the_grid_of_all_rows(c):
    n = len(c.pos)
    a = attributes_of(n, 9) if c.name != "large" else {}
    opt = synth.options(pos_bits=c.bits)
    got = synth.encode_lod_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=c.part_cells, lod_base_bits=c.lod_base_bits, **a)
    p = PINS[c.name]
    assert len(got.streams) == len(p.ranges) and got.levels == c.bits - c.lod_base_bits + 1
    for g, w in zip((got.kept, got.row_entries, got.ranges, got.level, got.qmin, got.qmax), p[:6]):
        assert np.array_equal(g, w)
    pg = grid_of(c) or synth.bounds_grid(c.pos)
    for s, (stream, (lo, hi)) in enumerate(zip(got.streams, p.ranges)):
        rows = p.lod[lo:hi]
        kw = {}
        if a:
            ex = [synth.Extra(e.values[rows], attribute_type=e.attribute_type, quantization_bits=e.quantization_bits,
                              grid=synth.bounds_grid(e.values) if e.values.dtype == np.float32 else None) for e in a["extra"]]
            kw = dict(normals=a["normals"][rows], uvs=a["uvs"][rows], generic=a["generic"][rows], extra=ex, uv_grid=synth.bounds_grid(a["uvs"]))
        assert stream == synth.encode_grid(c.pos[rows], None, opt=opt, form=0, geometry=0, pos_grid=pg, **kw), (c.name, s)
