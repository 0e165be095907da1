"""part_cells on the CPU: synth.cell_parts against the contract restated in numpy (cellpartcases.pin: mergecases.pin, then
splitcases.parts over the m kept entries), synth.encode_cell_parts read back through the oracle -- every part codes the integers of
its slice of kept, and its box is the box of what it decodes to -- and against synth.encode_split of rows[kept] on the explicit
grids of ALL rows, which is what the contract says the streams are."""
import numpy as np
import pytest

import cellpartcases as cc
import mergecases as mc
import oracle
import draco_sharp_amd.synth as synth


def grid_of(c):
    return None if c.grid is None else synth.grid(c.grid[0], c.grid[1])


def test_the_cases_are_what_they_say():
    cases = cc.cases()
    m = lambda c: len(np.unique(cc.quantised(c), axis=0))      # noqa: E731
    sized = cc.sized()
    assert sorted({m(c) for c in sized if c.name.startswith("distinct")}) == cc.M == [1, 2, 63, 64, 65, cc.TILE - 1, cc.TILE, cc.TILE + 1, 2 * cc.TILE + 1]
    assert {c.part_cells for c in cases} >= {1, 2, 63, 64, 65, cc.TILE - 1, cc.TILE, cc.TILE + 1, cc.INT32_MAX}
    assert all(m(c) == 1 for c in sized if c.name.startswith("identical")) and all(2 * m(c) == len(c.pos) for c in sized if c.name.startswith("twice"))
    # an all-identical cloud in many slots, a full part, one point over a full part, every slot full
    assert any(c.name.startswith("identical") and cc.slots(c) > 30 for c in cases)
    assert any(m(c) == c.part_cells > 1 for c in cases) and any(m(c) == c.part_cells + 1 for c in cases)
    assert all(m(c) == cc.slots(c) * c.part_cells and cc.slots(c) == 2 for c in cc.full_slots())
    by = {c.name.rsplit("-N", 1)[0]: c for c in cc.cuts()}
    starts = lambda c: np.concatenate([[0], np.cumsum(mc.runs_of(c))])      # noqa: E731  (the sorted entry of every kept entry)
    assert starts(by["cut-inside-a-tile"])[50] == 150 and starts(by["cut-on-a-tile-edge"])[2] == cc.TILE
    assert mc.spans(by["run-over-63|64-at-a-cut"])["63|64"] and mc.spans(by["run-over-1023|1024-at-a-cut"])["1023|1024"]
    assert any(c.grid is None for c in cases) and any(c.grid is not None and c.grid[1] != (1 << c.bits) - 1 for c in cases)
    c = cc.large()
    assert len(c.pos) == 70001 and m(c) == 2049 and len(cc.pin(c)[2]) == 18


CASES = cc.cases() + [cc.large()]


def test_the_twin_is_the_pin():
    for c in CASES:
        kept, cells, ranges, qmin, qmax = synth.cell_parts(c.pos, c.bits, c.part_cells, grid_of(c))
        want = cc.pin(c)
        assert kept.dtype == cells.dtype == ranges.dtype == np.uint32 and qmin.dtype == qmax.dtype == np.int32, c.name
        for got, w in zip((kept, cells, ranges, qmin, qmax), want):
            assert got.shape == w.shape and np.array_equal(got, w), c.name
        size = ranges[:, 1].astype(np.int64) - ranges[:, 0]
        assert len(ranges) == -(-len(kept) // c.part_cells) <= cc.slots(c) and size.min() >= 1 and size.max() <= c.part_cells and size.max() - size.min() <= 1, c.name
        assert ranges[0, 0] == 0 and ranges[-1, 1] == len(kept) and np.array_equal(ranges[1:, 0], ranges[:-1, 1]), c.name


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), uvs=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                extra=[synth.Extra(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)), synth.Extra(rng.random((n, 2)).astype(np.float32), quantization_bits=12)])


STREAMS = cc.cuts() + cc.full_slots() + [c for c in cc.sized() if c.part_cells in (2, 64, cc.TILE) and len(c.pos) in (65, 130, cc.TILE + 1, 2 * cc.TILE + 1)] + [cc.large()]


def dequantized(q, origin, rng, bits):
    """the decoder's float of integer q: every step rounded to float32"""
    delta = np.float32(rng) / np.float32((1 << bits) - 1)
    return (np.asarray(q, np.float32) * delta).astype(np.float32) + np.asarray(origin, np.float32)


@pytest.mark.parametrize("c", STREAMS, ids=[c.name for c in STREAMS])
def test_every_part_through_the_oracle_and_against_the_split_coder(c):
    n = len(c.pos)
    a = attributes_of(n, 9) if c.name != "large" else {}
    opt = synth.options(pos_bits=c.bits)
    got = synth.encode_cell_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=c.part_cells, **a)
    kept, cells, ranges, want_min, want_max = cc.pin(c)
    assert len(got.streams) == len(ranges) and np.array_equal(got.kept, kept) and np.array_equal(got.row_entries, cells) and np.array_equal(got.ranges, ranges)
    assert np.array_equal(got.qmin, want_min) and np.array_equal(got.qmax, want_max)
    q = cc.quantised(c)
    # the split coder of rows[kept] on the explicit grids of ALL rows: the same cuts (the kept rows are distinct cells in Morton
    # order, so their order is the identity), the same bytes
    pg = grid_of(c) or synth.bounds_grid(c.pos)
    kw = {}
    if a:
        ex = [synth.Extra(e.values[kept], attribute_type=e.attribute_type, quantization_bits=e.quantization_bits,
                          grid=synth.bounds_grid(e.values) if e.values.dtype == np.float32 else None) for e in a["extra"]]
        kw = dict(normals=a["normals"][kept], uvs=a["uvs"][kept], generic=a["generic"][kept], extra=ex, uv_grid=synth.bounds_grid(a["uvs"]))
    split = synth.encode_split(c.pos[kept], opt=opt, pos_grid=pg, part_points=c.part_cells, **kw)
    assert len(split) == len(ranges)
    seen = set()
    for p, (stream, (lo, hi)) in enumerate(zip(got.streams, ranges)):
        assert stream == split[p][0] and np.array_equal(split[p][1], np.arange(lo, hi)), p
        assert np.array_equal(split[p][2], want_min[p]) and np.array_equal(split[p][3], want_max[p]), p
        d = oracle.decode(stream)
        pos = [x for x in d.attributes if x.att_type == 0][0]
        assert d.num_points == hi - lo and np.array_equal(pos.portable, q[kept[lo:hi]]), p
        # the box the handle reports -- the decoder's floats of qmin / qmax -- is the box of the decoded positions, bit for bit
        v = np.ascontiguousarray(pos.values, np.float32).reshape(-1, 3)
        for ext, box in ((v.min(axis=0), got.qmin[p]), (v.max(axis=0), got.qmax[p])):
            assert np.array_equal(ext.view(np.uint32), dequantized(box, pg.origin[:3], pg.range, c.bits).view(np.uint32)), p
        cell = {tuple(t) for t in pos.portable.tolist()}
        assert len(cell) == hi - lo and not (cell & seen), p           # no position integer twice, in a part or across parts
        seen |= cell
    assert len(seen) == len(kept)


def test_no_parts_is_the_merged_stream():
    c = cc.cuts()[0]
    opt = synth.options(pos_bits=c.bits)
    merged, kept, cells = synth.encode_merged(c.pos, opt=opt, pos_grid=grid_of(c))
    for N in (len(kept), len(kept) + 1, cc.INT32_MAX, 0):
        got = synth.encode_cell_parts(c.pos, opt=opt, pos_grid=grid_of(c), part_cells=N)
        assert got.streams == [merged] and np.array_equal(got.kept, kept) and np.array_equal(got.row_entries, cells) and got.ranges.tolist() == [[0, len(kept)]]
