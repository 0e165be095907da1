"""Voxels coarser than the position grid, the CPU coder's twin (synth.merge_voxels, encode_merged / encode_cell_parts /
encode_lod_parts with voxel_bits / voxel_point; draco-sharp_amd/csrc/dsa_encode_host.h merge_points) held to the contract restated in
Python integers (voxelcases.pin) on every designed case, for the three rules.  No GPU."""
import numpy as np
import pytest

import mergecases as mc
import voxelcases as vc
import draco_sharp_amd.synth as synth


def twin(case, point, C=None):
    return synth.merge_voxels(case.pos, case.bits, None if case.grid is None else synth.grid(case.grid[0], case.grid[1]), case.C if C is None else C, point)


@pytest.mark.parametrize("point", vc.POINTS)
def test_every_case_is_the_pin(point):
    """kept, row_entries and the integers the position stream codes at the kept rows: the twin's are the pin's"""
    assert {(c.bits, c.C) for c in vc.cases()} >= set(vc.BC)
    for c in vc.cases():
        kept, entry, coded = twin(c, point)
        pk, pe, pc = vc.pin(c, point)
        assert np.array_equal(kept, pk) and np.array_equal(entry, pe), (c.name, point)
        assert np.array_equal(coded[kept], pc), (c.name, point)
        q = np.asarray(vc.integers(c), np.int64)
        rest = np.ones(len(q), bool)
        rest[kept] = False
        assert np.array_equal(coded[rest], q[rest]), (c.name, point)            # (only the kept rows carry anything but the quantiser's output)
        s = c.bits - c.C
        assert np.array_equal(coded[kept] >> s, q[kept] >> s), (c.name, point)  # (the coded point lies in its voxel)


def test_the_designed_values():
    """the centroids that tie and that land in an empty cell, the nearest rows that tie: the values written down with the cases"""
    for name, (point, make) in vc.DESIGNED.items():
        case, want = make()
        kept, entry, coded = twin(case, point)
        if point == vc.CENTROID:
            assert np.array_equal(coded[kept], want), name
        else:
            assert np.array_equal(kept, want), name
    case, want = vc.centroid_in_an_empty_cell()
    q = np.asarray(vc.integers(case), np.int64)
    assert not (q == want[0]).all(axis=1).any()
    # the nearest rows are neither the first of their voxels in sorted order nor their smallest rows
    case, want = vc.nearest_ties()
    first = twin(case, vc.FIRST)[0]
    assert not np.array_equal(first, want) and list(first) == [0, 7] and list(want) == [1, 4]


def test_the_shapes_the_cases_promise():
    """runs that end at entries 63, 64, 65, 1023, 1024, 1025; a cloud in one voxel; voxels of one row"""
    for B, C in vc.BC:
        ends = np.cumsum(vc.runs_of(vc.named("ends-%d-%d" % (B, C)))) - 1
        assert {63, 64, 65, vc.TILE - 1, vc.TILE, vc.TILE + 1} <= set(ends.tolist()), (B, C)
    assert list(vc.runs_of(vc.named("one-voxel-2100-14-2"))) == [2100] and 2100 > 2 * vc.TILE
    assert set(vc.runs_of(vc.named("single-rows-11-10")).tolist()) == {1}
    assert all(n % 4 == 0 for n in vc.runs_of(vc.named("duplicated-11-2")))


@pytest.mark.parametrize("point", vc.POINTS)
def test_voxel_bits_B_is_voxel_bits_0(point):
    """C = B keeps what merge_points keeps, whatever the rule; and voxel_bits = 0 is merge_points"""
    for c in vc.cases():
        kept, entry, coded = twin(c, point, C=c.bits)
        k0, e0, c0 = twin(c, 0, C=0)
        km, em = synth.merge_points(c.pos, c.bits, None if c.grid is None else synth.grid(c.grid[0], c.grid[1]))
        assert np.array_equal(kept, k0) and np.array_equal(entry, e0) and np.array_equal(coded, c0), (c.name, point)
        assert np.array_equal(k0, km) and np.array_equal(e0, em), c.name
        assert np.array_equal(km, mc.pin(c.pos, c.bits, c.grid)[0]), c.name


def test_streams_and_levels_of_the_twin():
    """encode_merged with voxels is encode_grid of the kept rows with the coded integers; parts and levels cut the same kept rows, L = C - D + 1"""
    c = vc.named("ends-11-10")
    for point in vc.POINTS:
        kept, entry, coded = twin(c, point)
        stream, k, e = synth.encode_merged(voxel_bits=c.C, voxel_point=point, **vc.cpu_args(c))
        assert np.array_equal(k, kept) and np.array_equal(e, entry)
        want = synth.encode_grid(c.pos[kept], None, form=0, geometry=0, opt=synth.options(pos_bits=c.bits), pos_grid=synth.grid(c.grid[0], c.grid[1]),
                                 pos_portable=coded[kept])
        assert stream == want, point
        off = synth.encode_merged(voxel_bits=c.bits, voxel_point=point, **vc.cpu_args(c))[0]
        assert off == synth.encode_merged(**vc.cpu_args(c))[0] and off != stream
        parts = synth.encode_cell_parts(part_cells=7, voxel_bits=c.C, voxel_point=point, **vc.cpu_args(c))
        assert np.array_equal(parts.kept, kept) and np.array_equal(parts.row_entries, entry)
        for (lo, hi), mn, mx in zip(parts.ranges, parts.qmin, parts.qmax):
            assert np.array_equal(mn, coded[kept[lo:hi]].min(axis=0)) and np.array_equal(mx, coded[kept[lo:hi]].max(axis=0))
        D = 4
        lod = synth.encode_lod_parts(part_cells=7, lod_base_bits=D, voxel_bits=c.C, voxel_point=point, **vc.cpu_args(c))
        assert lod.levels == c.C - D + 1 and sorted(lod.kept.tolist()) == sorted(kept.tolist())
        for l in range(lod.levels):         # levels 0 .. l: one point per occupied cell of the grid with D + l bits
            rows = np.concatenate([lod.kept[lo:hi] for (lo, hi), lv in zip(lod.ranges, lod.level) if lv <= l])
            cells = coded[rows] >> (c.bits - D - l)
            every = np.unique(np.asarray(vc.integers(c), np.int64) >> (c.bits - D - l), axis=0)
            assert len(np.unique(cells, axis=0)) == len(rows) == len(every), (point, l)
    with pytest.raises(RuntimeError, match="lod_base_bits out of range"):
        synth.encode_lod_parts(part_cells=7, lod_base_bits=c.C + 1, voxel_bits=c.C, **vc.cpu_args(c))
    with pytest.raises(RuntimeError, match="voxel_point"):
        synth.merge_voxels(c.pos, c.bits, None, 0, 1)
