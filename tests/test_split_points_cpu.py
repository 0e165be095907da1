"""part_points on the CPU: synth.split_parts against the ranges restated in numpy (splitcases.parts), synth.part_boxes against
numpy's order and boxes (splitcases.pin), synth.encode_split against the plain coder of every slice on the bounds of all rows --
written out here from the contract -- and read back through the oracle, and one part against synth.encode_ordered."""
import numpy as np
import pytest

import oracle
import ordercases as oc
import splitcases as sc
import draco_sharp_amd.synth as synth


def grid_of(c):
    return None if c.grid is None else synth.grid(c.grid[0], c.grid[1])


def positions(stream):
    return [a for a in oracle.decode(stream).attributes if a.att_type == 0][0]


def test_ranges_are_the_pin():
    seen = 0
    for n in sc.SIZES + [70001, 2**28 - 1]:           # (the last: p n beyond 32 bits)
        for N in (sc.part_sizes(n) if n < 2**20 else [2**16 + 1, 2**27]) + [4096]:
            r = synth.split_parts(n, N)
            want = sc.parts(n, N)
            assert r.dtype == np.uint32 and r.shape == want.shape and np.array_equal(r, want), (n, N)
            size = r[:, 1].astype(np.int64) - r[:, 0]
            assert len(r) == -(-n // N) and size.min() >= 1 and size.max() <= N and size.max() - size.min() <= 1, (n, N)
            assert r[0, 0] == 0 and r[-1, 1] == n and np.array_equal(r[1:, 0], r[:-1, 1]), (n, N)          # the ranges tile [0, n)
            seen += 1
    assert seen > 120
    assert np.array_equal(synth.split_parts(777, 0), [[0, 777]])                                          # part_points 0: one part
    assert len(sc.parts(70001, 4096)) == 18 and len(synth.split_parts(65537, 1)) == 65537
    with pytest.raises(RuntimeError, match="positions are missing"):
        synth.split_parts(0, 5)


CASES = sc.cuts() + [c for c in sc.sized() if c.name.split("-")[0] in ("n65", "n%d" % (sc.TILE + 1), "n%d" % (2 * sc.TILE + 1))]


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_boxes_and_rows_are_numpys(c):
    perm, ranges, qmin, qmax = synth.part_boxes(c.pos, c.bits, c.part_points, grid_of(c))
    want_perm, want_ranges, want_min, want_max = sc.pin(c)
    assert np.array_equal(perm, want_perm) and np.array_equal(ranges, want_ranges)
    assert qmin.dtype == np.int32 and np.array_equal(qmin, want_min) and np.array_equal(qmax, want_max)


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), uvs=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                extra=[synth.Extra(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)), synth.Extra(rng.random((n, 2)).astype(np.float32), quantization_bits=12)])


STREAMS = sc.cuts() + [sc.Case("n%d-N700" % (2 * sc.TILE + 77), oc.random_cloud(2 * sc.TILE + 77, 641), 11, None, 700), sc.large()]


@pytest.mark.parametrize("c", STREAMS, ids=[c.name for c in STREAMS])
def test_every_part_is_the_plain_stream_of_its_slice(c):
    n = len(c.pos)
    a = attributes_of(n, 7) if c.name != "large" else {}
    opt = synth.options(pos_bits=c.bits)
    got = synth.encode_split(c.pos, opt=opt, pos_grid=grid_of(c), part_points=c.part_points, **a)
    perm, ranges, want_min, want_max = sc.pin(c)
    assert len(got) == len(ranges) and (c.name != "large" or len(got) == 18)
    q = sc.quantised(c)
    # the single ordered stream: the parts' integers, one behind the other, are its integers
    ordered, operm = synth.encode_ordered(c.pos, None, opt=opt, geometry=0, pos_grid=grid_of(c), **a)
    assert np.array_equal(operm, perm)
    whole = oracle.decode(ordered)
    joined = [[] for _ in whole.attributes]
    for (stream, rows, qmin, qmax), (lo, hi), mn, mx in zip(got, ranges, want_min, want_max):
        assert np.array_equal(rows, perm[lo:hi]) and np.array_equal(qmin, mn) and np.array_equal(qmax, mx)
        # the plain coder of the slice, every quantised attribute on the bounds of ALL the cloud's rows
        kw = {}
        if a:
            ex = [synth.Extra(e.values[rows], attribute_type=e.attribute_type, quantization_bits=e.quantization_bits,
                              grid=synth.bounds_grid(e.values) if e.values.dtype == np.float32 else None) for e in a["extra"]]
            kw = dict(normals=a["normals"][rows], uvs=a["uvs"][rows], generic=a["generic"][rows], extra=ex, uv_grid=synth.bounds_grid(a["uvs"]))
        plain = synth.encode_grid(c.pos[rows], None, opt=opt, form=0, geometry=0, pos_grid=grid_of(c) or synth.bounds_grid(c.pos), **kw)
        assert stream == plain, (lo, hi)
        d = oracle.decode(stream)
        assert d.num_points == hi - lo and len(d.attributes) == len(whole.attributes)
        assert np.array_equal(positions(stream).portable, q[rows])                    # the quantised integers of positions[perm[lo:hi]]
        for k, x in enumerate(d.attributes):
            joined[k].append(x.portable if x.portable is not None else x.values)
    for k, y in enumerate(whole.attributes):
        assert np.array_equal(np.concatenate(joined[k]), y.portable if y.portable is not None else y.values), k


def test_one_part_is_the_ordered_stream():
    pos = oc.random_cloud(sc.TILE + 5, 651)
    a = attributes_of(len(pos), 8)
    opt = synth.options(pos_bits=11)
    ordered, perm = synth.encode_ordered(pos, None, opt=opt, geometry=0, **a)
    for N in (len(pos), len(pos) + 1, sc.INT32_MAX, 0):
        (stream, rows, qmin, qmax), = synth.encode_split(pos, opt=opt, part_points=N, **a)
        assert stream == ordered and np.array_equal(rows, perm)
