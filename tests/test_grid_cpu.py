"""Quantisation grids given by the caller, the CPU coder (synth.encode_grid, synth.shared_grid) read back through the oracle: the
header carries the grid's floats bit for bit, the integers are those of the numpy pin of tests/gridcases.py (written from the
formula, independent of both coders), a grid equal to the mesh's own bounds and no grid at all give the bytes of before, values
off the grid or not finite are refused in the stated words, and regular data on its own grid decodes exactly.  No GPU needed."""
import numpy as np
import pytest

import gridcases as gc
import oracle
import draco_sharp_amd.synth as synth


def bits_of(x):
    return np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).tolist()


def sorted_rows(a):
    a = np.asarray(a)
    a = a.reshape(len(a), -1)
    return a[np.lexsort(a.T[::-1])]


def attribute(stream, att_type):
    return [a for a in oracle.decode(stream).attributes if a.att_type == att_type][0]


@pytest.fixture(scope="module")
def tiles():
    return gc.tiles()


def test_shared_grid_is_numpys_minimum_and_extent(tiles):
    arrays = [c.pos for c, _ in tiles]
    g = synth.shared_grid(arrays)
    origin, rng = gc.shared_bounds(arrays)
    assert g.mode == 1 and bits_of(list(g.origin)[:3]) == bits_of(origin) and bits_of(g.range) == bits_of(rng)
    own = [gc.own_bounds(a) for a in arrays]
    assert len({tuple(bits_of(o)) + tuple(bits_of(r)) for o, r in own}) == 4      # the tiles' own grids all differ
    # an array with a value that is not finite takes no part; a flat group has range 1; -0.0 lies below +0.0
    bad = arrays[1].copy()
    bad[3, 0] = np.inf
    g2 = synth.shared_grid([arrays[0], bad])
    o0, r0 = gc.own_bounds(arrays[0])
    assert bits_of(list(g2.origin)[:3]) == bits_of(o0) and bits_of(g2.range) == bits_of(r0)
    flat = synth.shared_grid([np.full((4, 2), 0.25, np.float32)])
    assert list(flat.origin)[:2] == [0.25, 0.25] and flat.range == 1.0
    zero = synth.shared_grid([np.array([[0.0], [-0.0]], np.float32), np.array([[-0.0], [0.0]], np.float32)])
    assert bits_of(zero.origin[0]) == bits_of(np.float32(-0.0))
    with pytest.raises(RuntimeError, match="not finite"):
        synth.shared_grid([bad])


@pytest.mark.parametrize("form", ["edgebreaker", "sequential", "cloud", "points"])
def test_header_and_integers_are_the_pins(tiles, form):
    origin, rng = gc.shared_bounds([c.pos for c, _ in tiles])
    uo, ur = gc.shared_bounds([c.uvs for c, _ in tiles])
    for c, _ in tiles:
        kw = dict(pos_grid=synth.grid(origin, rng), uv_grid=synth.grid(uo, ur))
        if form == "edgebreaker":
            s = synth.encode_grid(c.pos, c.faces, uvs=c.uvs, **kw)
        elif form == "sequential":
            s = synth.encode_grid(c.pos, c.faces, uvs=c.uvs, form=0, geometry=1, **kw)
        elif form == "cloud":
            s = synth.encode_grid(c.pos, None, uvs=c.uvs, form=0, geometry=0, **kw)
        else:
            s = synth.encode_grid(c.pos, c.faces, uvs=c.uvs, form=2, **kw)
        for att_type, vals, o, r, bits in ((0, c.pos, origin, rng, gc.POS_BITS), (3, c.uvs, uo, ur, gc.UV_BITS)):
            a = attribute(s, att_type)
            nc = vals.shape[1]
            assert bits_of(a.q_min[:nc]) == bits_of(o) and bits_of(a.q_range) == bits_of(r) and a.q_bits == bits
            want = gc.pin(vals, o, r, bits)
            assert want.min() >= 0 and want.max() <= (1 << bits) - 1
            if form in ("sequential", "cloud"):
                assert np.array_equal(a.portable, want)              # point i of the stream is row i
            else:
                assert np.array_equal(sorted_rows(a.portable), sorted_rows(want))
            assert np.array_equal(sorted_rows(a.values).view(np.uint32), sorted_rows(gc.dequantize(want, o, r, bits)).view(np.uint32))


def test_own_bounds_as_a_grid_and_no_grid_give_the_bytes_of_before(tiles):
    c = tiles[2][0]
    o, r = gc.own_bounds(c.pos)
    uo, ur = gc.own_bounds(c.uvs)
    before = synth.encode_mesh(c.pos, c.faces, uvs=c.uvs)
    assert synth.encode_grid(c.pos, c.faces, uvs=c.uvs) == before
    assert synth.encode_grid(c.pos, c.faces, uvs=c.uvs, pos_grid=synth.grid(o, r), uv_grid=synth.grid(uo, ur)) == before
    assert synth.encode_grid(c.pos, c.faces, uvs=c.uvs, pos_grid=synth.grid([0, 0, 0], 1.0, mode=0)) == before
    assert synth.encode_grid(c.pos, c.faces, uvs=c.uvs, form=0, pos_grid=synth.grid(o, r)) == synth.encode_sequential(c.pos, c.faces, uvs=c.uvs)
    assert synth.encode_grid(c.pos, None, form=0, geometry=0, pos_grid=synth.grid(o, r)) == synth.encode_point_cloud(c.pos)
    assert synth.encode_grid(c.pos, c.faces, uvs=c.uvs, form=2, pos_grid=synth.grid(o, r)) == synth.encode_mesh_points(c.pos, c.faces, uvs=c.uvs)
    w = np.random.default_rng(1).random((len(c.pos), 4)).astype(np.float32)
    wo, wr = gc.own_bounds(w)
    ids = np.arange(len(c.pos), dtype=np.uint16)
    with_grid = [synth.Extra(w, quantization_bits=9, grid=synth.grid(wo, wr)), synth.Extra(ids)]
    assert synth.encode_grid(c.pos, c.faces, extra=with_grid) == synth.encode_mesh(c.pos, c.faces, extra=[synth.Extra(w, quantization_bits=9), synth.Extra(ids)])


@pytest.mark.parametrize("what", ["off", "nan", "inf"])
def test_values_off_the_grid_or_not_finite_are_refused(what):
    c, (origin, rng), row = gc.damaged(what)
    assert gc.first_bad_row(c.pos, origin, rng, gc.POS_BITS) == (row, what == "off")
    want = gc.refusal("positions", row, what == "off")
    for kw in (dict(), dict(form=0, geometry=1), dict(form=2)):
        with pytest.raises(RuntimeError) as e:
            synth.encode_grid(c.pos, c.faces, uvs=c.uvs, pos_grid=synth.grid(origin, rng), **kw)
        assert str(e.value) == want


def test_a_value_that_is_not_finite_is_named_before_one_off_the_grid():
    c, (origin, rng), row = gc.damaged("nan")
    pos = c.pos.copy()
    pos[1, 0] = origin[0] - rng            # row 1 is off the grid, row `row` holds the NaN
    with pytest.raises(RuntimeError) as e:
        synth.encode_grid(pos, c.faces, pos_grid=synth.grid(origin, rng))
    assert str(e.value) == gc.refusal("positions", row, False)


def test_a_value_that_rounds_onto_the_last_cell_is_inside():
    c, (origin, rng), row = gc.damaged("edge")
    assert gc.first_bad_row(c.pos, origin, rng, gc.POS_BITS) is None
    a = attribute(synth.encode_grid(c.pos, c.faces, form=0, pos_grid=synth.grid(origin, rng)), 0)
    assert a.portable[row, 0] == (1 << gc.POS_BITS) - 1
    assert np.array_equal(a.portable, gc.pin(c.pos, origin, rng, gc.POS_BITS))


def test_other_attributes_are_named_and_checked():
    c = gc.texel()
    uo, ur = gc.own_bounds(c.uvs)
    uv = c.uvs.copy()
    uv[17, 1] = np.float32(2.0)
    with pytest.raises(RuntimeError) as e:
        synth.encode_grid(c.pos, c.faces, uvs=uv, uv_grid=synth.grid(uo, ur))
    assert str(e.value) == gc.refusal("texcoords", 17, True)
    w = np.random.default_rng(2).random((len(c.pos), 2)).astype(np.float32)
    w[40, 0] = np.nan
    with pytest.raises(RuntimeError) as e:
        synth.encode_grid(c.pos, c.faces, extra=[synth.Extra(np.arange(len(c.pos), dtype=np.uint8)), synth.Extra(w, grid=synth.grid([0, 0], 1.0))])
    assert str(e.value) == gc.refusal("attribute 1", 40, False)


@pytest.mark.parametrize("grid, message", [
    (lambda: synth.grid([0, 0, 0], 0.0), "positions: grid.range 0: finite and above 0"),
    (lambda: synth.grid([0, 0, 0], -1.0), "positions: grid.range -1: finite and above 0"),
    (lambda: synth.grid([0, 0, 0], np.inf), "positions: grid.range inf: finite and above 0"),
    (lambda: synth.grid([0, np.nan, 0], 1.0), "positions: grid.origin[1] is not finite"),
    (lambda: synth.grid([0, 0, 0], 1.0, mode=3), "positions: grid.mode 3: 0 (own bounds), 1 (explicit) or 2 (shared within the group)"),
    (lambda: synth.grid([0, 0, 0], 1.0, mode=-1), "positions: grid.mode -1: 0 (own bounds), 1 (explicit) or 2 (shared within the group)"),
])
def test_a_grid_that_is_none_is_refused_by_its_field(grid, message):
    c = gc.voxel()
    with pytest.raises(RuntimeError) as e:
        synth.encode_grid(c.pos, c.faces, pos_grid=grid())
    assert str(e.value) == message


def test_reserved_words_integer_attributes_and_absent_attributes():
    c = gc.voxel()
    g = synth.grid([0, 0, 0], 1.0)
    g.reserved[1] = 5
    with pytest.raises(RuntimeError, match="positions: grid.reserved is not zero"):
        synth.encode_grid(c.pos, c.faces, pos_grid=g)
    with pytest.raises(RuntimeError, match=r"attribute 0: grid.mode 1 on an attribute that is not quantised"):
        synth.encode_grid(c.pos, c.faces, extra=[synth.Extra(np.arange(len(c.pos), dtype=np.int16), grid=synth.grid([0], 1.0))])
    with pytest.raises(RuntimeError, match="texcoords: grid.mode 1 for an attribute the mesh does not have"):
        synth.encode_grid(c.pos, c.faces, uv_grid=synth.grid([0, 0], 1.0))


def test_voxels_and_texels_on_their_own_grid_decode_exactly():
    v = gc.voxel()
    s = synth.encode_grid(v.pos, v.faces, form=0, pos_grid=synth.grid([0, 0, 0], float((1 << gc.POS_BITS) - 1)))
    a = attribute(s, 0)
    assert np.array_equal(a.values.view(np.uint32), v.pos.view(np.uint32))
    assert np.array_equal(a.portable, v.pos.astype(np.int32))
    own = attribute(synth.encode_sequential(v.pos, v.faces), 0)
    assert not np.array_equal(own.values, v.pos)                       # the bounding box does not keep the integers
    t = gc.texel()
    s = synth.encode_grid(t.pos, t.faces, uvs=t.uvs, form=0, uv_grid=synth.grid([0, 0], 1023.0 / 1024.0))
    a = attribute(s, 3)
    assert np.array_equal(a.values.view(np.uint32), t.uvs.view(np.uint32))
    assert not np.array_equal(attribute(synth.encode_sequential(t.pos, t.faces, uvs=t.uvs), 3).values, t.uvs)


def test_tiles_on_a_shared_grid_meet_at_their_borders(tiles):
    """The crack, stated on the pin and held against the CPU coder: on their own grids the tiles disagree about a border vertex,
    on the group's grid every vertex of the field has one decoded position."""
    own, shared = {}, {}
    g = synth.shared_grid([c.pos for c, _ in tiles])
    origin, rng = np.array(list(g.origin)[:3], np.float32), np.float32(g.range)
    for c, index in tiles:
        o, r = gc.own_bounds(c.pos)
        deq_own = gc.dequantize(gc.pin(c.pos, o, r, gc.POS_BITS), o, r, gc.POS_BITS)
        a = attribute(synth.encode_grid(c.pos, c.faces, form=0, pos_grid=g), 0)
        assert np.array_equal(a.values.view(np.uint32), gc.dequantize(gc.pin(c.pos, origin, rng, gc.POS_BITS), origin, rng, gc.POS_BITS).view(np.uint32))
        for row, (r_, c_) in enumerate(index):
            own.setdefault((int(r_), int(c_)), set()).add(tuple(bits_of(deq_own[row])))
            shared.setdefault((int(r_), int(c_)), set()).add(tuple(bits_of(a.values[row])))
    assert any(len(v) > 1 for v in own.values())
    assert sum(1 for v in shared.values() if len(v) > 1) == 0 and any(len(v) == 1 for v in shared.values())
