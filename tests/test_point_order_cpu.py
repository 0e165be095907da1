"""The Morton point order of sequential streams on the CPU: synth.point_order (what the device's sort is held to) against the
definition restated in numpy over the integers the oracle decodes, synth.encode_ordered read back through the oracle, and the
size guard on the shuffled height field."""
import numpy as np
import pytest

import oracle
import ordercases as oc
import draco_sharp_amd.synth as synth


def grid_of(c):
    return None if c.grid is None else synth.grid(c.grid[0], c.grid[1])


def positions(stream):
    return [a for a in oracle.decode(stream).attributes if a.att_type == 0][0]


CASES = [c for c in oc.cases() if len(c.pos) <= 5000] + [oc.cases()[-1]]


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_point_order_is_the_definition(c):
    """key from the integers the oracle decodes out of the stream in the caller's order, rows by np.lexsort((rows, key))"""
    plain = synth.encode_grid(c.pos, None, opt=synth.options(pos_bits=c.bits), form=0, geometry=0, pos_grid=grid_of(c))
    q = positions(plain).portable
    assert q.shape == (len(c.pos), 3) and q.min() >= 0 and q.max() <= (1 << c.bits) - 1
    perm = synth.point_order(c.pos, c.bits, grid_of(c))
    assert perm.dtype == np.uint32 and np.array_equal(perm, oc.morton_order(q, c.bits))
    assert np.array_equal(np.sort(perm), np.arange(len(c.pos)))


def test_the_key_reads_the_low_bits_only_and_ties_go_to_the_smaller_row():
    q = np.array([[5, 0, 0], [1, 0, 0], [-1, -1, -1], [1, 0, 0], [0, 0, 1], [0, 1, 0]], np.int32)
    assert oc.morton_key(q, 2).tolist() == [4, 4, 63, 4, 1, 2]          # 5 & 3 = 1; -1 & 3 = 3 in every lane
    assert oc.morton_order(q, 2).tolist() == [4, 5, 0, 1, 3, 2]
    assert int(oc.morton_key(np.array([[(1 << 20) - 1, 0, 0]]), 20)[0]) == sum(1 << (3 * b + 2) for b in range(20))
    # identical points: the identity
    same = np.tile(np.float32([1, 2, 3]), (300, 1))
    assert np.array_equal(synth.point_order(same, 11), np.arange(300))


def test_refusals_of_the_host_twin():
    p = oc.random_cloud(10, 1)
    with pytest.raises(RuntimeError, match="bits out of range"):
        synth.point_order(p, 21)
    bad = p.copy()
    bad[4, 1] = np.nan
    with pytest.raises(RuntimeError, match="row 4"):
        synth.point_order(bad, 11, synth.grid([0, 0, 0], 2.0))


@pytest.mark.parametrize("geometry,compressed", [(0, False), (1, False), (1, True)])
def test_encode_ordered_round_trips_to_the_permuted_input(geometry, compressed):
    rng = np.random.default_rng(3)
    c = oc.meshed()[0]
    n = len(c.pos)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    uv = rng.random((n, 2)).astype(np.float32)
    gen = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    extra = [synth.Extra(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)), synth.Extra(rng.integers(0, 100000, (n, 1)).astype(np.uint32)),
             synth.Extra(rng.random((n, 2)).astype(np.float32), quantization_bits=12)]
    faces = c.faces if geometry else None
    opt = synth.options(pos_bits=c.bits)
    stream, perm = synth.encode_ordered(c.pos, faces, nrm, uv, gen, extra, opt, geometry=geometry, compressed=compressed)
    assert np.array_equal(perm, synth.point_order(c.pos, c.bits))
    plain = oracle.decode(synth.encode_grid(c.pos, faces, nrm, uv, gen, extra, opt, form=0, geometry=geometry, compressed=compressed))
    got = oracle.decode(stream)
    assert got.num_points == n and len(got.attributes) == len(plain.attributes) == 7
    for a, b in zip(got.attributes, plain.attributes):
        assert a.att_type == b.att_type and len(a.point_map) == 0
        assert np.array_equal(a.values.view(np.uint8), b.values[perm].view(np.uint8))
        if a.portable is not None:
            assert np.array_equal(a.portable, b.portable[perm])
    if geometry:
        rank = np.zeros(n, np.int64)
        rank[perm] = np.arange(n)
        assert np.array_equal(got.faces, rank[c.faces.astype(np.int64)])
        assert np.array_equal(perm[got.faces], plain.faces)             # the same triangles over the caller's rows, in the caller's order


def test_the_order_halves_a_shuffled_height_field():
    """200 x 250 shuffled rows at 11 bits (ordercases.size_guard): the host coder gives 87 836 bytes ordered against 194 403 as
    given, ratio 0.45.  The bound of 0.5 guards against an order that stops ordering; it is no target."""
    pos = oc.size_guard()
    opt = synth.options(pos_bits=11)
    plain = synth.encode_point_cloud(pos, opt)
    ordered, perm = synth.encode_ordered(pos, opt=opt, geometry=0)
    print("bytes as given %d, Morton-ordered %d, ratio %.3f" % (len(plain), len(ordered), len(ordered) / len(plain)))
    assert len(ordered) <= 0.5 * len(plain)
    assert np.array_equal(positions(ordered).portable, positions(plain).portable[perm])
