"""merge_points on the CPU: synth.merge_points (what the device's merge kernels are held to) against the contract restated in numpy
(mergecases.pin: numpy quantisation, np.unique over the integer triples, the smallest row per cell, the cells in Morton order),
synth.encode_merged against the plain coder of the kept rows on explicit grids and read back through the oracle, and a cloud
without two points in one cell against synth.encode_ordered."""
import numpy as np
import pytest

import mergecases as mc
import oracle
import ordercases as oc
import draco_sharp_amd.synth as synth


def grid_of(c):
    return None if c.grid is None else synth.grid(c.grid[0], c.grid[1])


def positions(stream):
    return [a for a in oracle.decode(stream).attributes if a.att_type == 0][0]


CASES = mc.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_merge_points_is_the_contract(c):
    kept, cells = synth.merge_points(c.pos, c.bits, grid_of(c))
    want_kept, want_cells, _ = mc.pin(c.pos, c.bits, c.grid)
    assert kept.dtype == np.uint32 and cells.dtype == np.uint32 and len(cells) == len(c.pos)
    assert np.array_equal(kept, want_kept) and np.array_equal(cells, want_cells)
    # ... and as the rule over the sorted order states it
    perm = synth.point_order(c.pos, c.bits, grid_of(c))
    key = oc.morton_key(mc.quantised(c.pos, c.bits, c.grid), c.bits)[perm]
    head = np.concatenate([[True], key[1:] != key[:-1]])
    assert np.array_equal(kept, perm[head])
    assert np.array_equal(cells[perm], np.cumsum(head) - 1)


def test_cells_by_construction():
    """the multiplicities put sorted entry e into its cell: kept[j] is the smallest row with z = j"""
    runs = mc.boundary_runs()
    assert all(mc.spans(runs[-1]).values()), mc.spans(runs[-1])
    for c, what in zip(runs, ("63|64", "1023|1024", "run of 1500", "two whole tiles", "head at a tile start", "tile with no head")):
        assert mc.spans(c)[what], (c.name, mc.spans(c))
    for c in runs + mc.sized():
        kept, cells = synth.merge_points(c.pos, c.bits, grid_of(c))
        z = c.pos[:, 2].astype(np.int64)
        assert len(kept) == len(mc.runs_of(c)) and np.array_equal(cells, z)
        assert np.array_equal(kept, [np.flatnonzero(z == j)[0] for j in range(len(kept))])
    c = mc.dropped_extremes()
    kept, cells = synth.merge_points(c.pos, c.bits)
    assert cells[4] == cells[2] and cells[5] == cells[3] and 2 in kept and 3 in kept and 4 not in kept and 5 not in kept
    assert all(c.pos[:, k].argmin() == 4 and c.pos[:, k].argmax() == 5 for k in range(3))


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), uvs=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                extra=[synth.Extra(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)), synth.Extra(rng.integers(0, 100000, (n, 1)).astype(np.uint32)),
                       synth.Extra(rng.random((n, 2)).astype(np.float32), quantization_bits=12)])


def test_own_bounds_and_the_equal_explicit_grid_write_one_stream():
    """what lets the contract name a plain call: an explicit grid goes into the header as it is, and the integers are the same"""
    pos = oc.random_cloud(900, 5) * np.float32(2.5) - np.float32(0.75)
    a = attributes_of(900, 6)
    opt = synth.options(pos_bits=11)
    own = synth.encode_grid(pos, None, opt=opt, form=0, geometry=0, **a)
    ex = [synth.Extra(e.values, attribute_type=e.attribute_type, quantization_bits=e.quantization_bits,
                      grid=synth.bounds_grid(e.values) if e.values.dtype == np.float32 else None) for e in a["extra"]]
    on_grid = synth.encode_grid(pos, None, a["normals"], a["uvs"], a["generic"], ex, opt, form=0, geometry=0, pos_grid=synth.bounds_grid(pos),
                                uv_grid=synth.bounds_grid(a["uvs"]))
    assert own == on_grid


@pytest.mark.parametrize("c", [mc.half_duplicated(777, 9), mc.dropped_extremes(), mc.explicit(), mc.boundary_runs()[-1]], ids=lambda c: c.name)
def test_encode_merged_is_the_plain_stream_of_the_kept_rows(c):
    n = len(c.pos)
    a = attributes_of(n, 3)
    opt = synth.options(pos_bits=c.bits)
    stream, kept, cells = synth.encode_merged(c.pos, opt=opt, pos_grid=grid_of(c), **a)
    want_kept, want_cells, want_q = mc.pin(c.pos, c.bits, c.grid)
    assert np.array_equal(kept, want_kept) and np.array_equal(cells, want_cells)
    m = len(kept)
    # the plain coder of the kept rows, every quantised attribute on the bounds of ALL rows, written out here from the contract
    ex = [synth.Extra(e.values[kept], attribute_type=e.attribute_type, quantization_bits=e.quantization_bits,
                      grid=synth.bounds_grid(e.values) if e.values.dtype == np.float32 else None) for e in a["extra"]]
    plain = synth.encode_grid(c.pos[kept], None, a["normals"][kept], a["uvs"][kept], a["generic"][kept], ex, opt, form=0, geometry=0,
                              pos_grid=grid_of(c) or synth.bounds_grid(c.pos), uv_grid=synth.bounds_grid(a["uvs"]))
    assert stream == plain
    got = oracle.decode(stream)
    assert got.num_points == m and len(got.attributes) == 7
    assert np.array_equal(positions(stream).portable, want_q)          # the unique cells, in Morton order
    # every attribute: the values the plain stream of ALL rows decodes to, at the kept rows (the bounds are those of all rows)
    full = oracle.decode(synth.encode_grid(c.pos, None, opt=opt, form=0, geometry=0, pos_grid=grid_of(c), **a))
    for x, y in zip(got.attributes, full.attributes):
        assert x.att_type == y.att_type and np.array_equal(x.values.view(np.uint8), y.values[kept].view(np.uint8))
        if x.portable is not None:
            assert np.array_equal(x.portable, y.portable[kept])


def test_without_two_points_in_a_cell_the_stream_is_the_ordered_one():
    c = [c for c in mc.sized() if c.name == "distinct-%d" % (2 * mc.TILE + 1)][0]
    a = attributes_of(len(c.pos), 4)
    opt = synth.options(pos_bits=c.bits)
    merged, kept, cells = synth.encode_merged(c.pos, opt=opt, pos_grid=grid_of(c), **a)
    ordered, perm = synth.encode_ordered(c.pos, None, opt=opt, geometry=0, pos_grid=grid_of(c), **a)
    assert merged == ordered and np.array_equal(kept, perm) and np.array_equal(cells[perm], np.arange(len(perm)))


def test_refusals_of_the_host_twin():
    p = oc.random_cloud(10, 1)
    with pytest.raises(RuntimeError, match="bits out of range"):
        synth.merge_points(p, 21)
    bad = p.copy()
    bad[4, 1] = np.nan
    with pytest.raises(RuntimeError, match="row 4"):
        synth.merge_points(bad, 11, synth.grid([0, 0, 0], 2.0))
