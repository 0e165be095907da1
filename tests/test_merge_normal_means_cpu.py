"""The host coder's twin of mean_normals (synth.merge_mean_normals, synth.encode_merged / encode_cell_parts / encode_lod_parts with
mean_normals=; dsa_encode_host.h merge_mean_normals): its streams decode, through the oracle, to the rule restated in Python integers
(normalmeancases.pin: q from the oracle's decode of the plain ordered stream of all rows, the rule per cell), on every case of
normalmeancases; the result does not depend on the order of the rows; against the float64 normalised sum it stays within the
quantiser's own largest angle; mean_normals=False is the vote twin byte for byte.  No GPU needed: what the device must write is held
to these twins by tests/test_gpu_encode_normal_means.py."""
import numpy as np
import pytest

import meshutil
import normalmeancases as nc
import oracle
import draco_sharp_amd.synth as synth


def test_the_rule_on_designed_cells():
    """the pin itself and synth.merge_mean_normals on cells whose answer is known: identical rows, opposite pairs, +x with +y"""
    for nbits in (2, 3, 8, 11, 20):
        c, mv = nc.center(nbits), (1 << nbits) - 2
        x, y, z, nx = (c, c), tuple(int(v) for v in meshutil.oct_quantize(np.float32([[0, 1, 0]]), nbits)[0]), (c, mv), (mv, mv)
        assert nc.vector(*x, nbits) == (c, 0, 0) and nc.vector(*y, nbits) == (0, c, 0) and nc.vector(*z, nbits) == (0, 0, c) and nc.vector(*nx, nbits) == (-c, 0, 0)
        assert nc.unit((c, 0, 0)) == (1 << 30, 0, 0)
        sets = [[x, x], [y, y, y], [x, nx], [z, nx, x], [x], [nx, nx, nx, nx], [x, y]]
        want = [x, y, x, z, x, nx, nc.mean_code([x, y], nbits)]
        assert [nc.mean_code(s, nbits) for s in sets] == want
        q = np.array([code for s in sets for code in s], np.int32)
        cells = np.repeat(np.arange(len(sets)), [len(s) for s in sets]).astype(np.uint32)
        for order in (np.arange(len(q)), np.random.default_rng(nbits).permutation(len(q))):
            got = synth.merge_mean_normals(q[order], nbits, cells[order], len(sets))
            assert got.dtype == np.int32 and [tuple(r) for r in got.tolist()] == want, nbits
    with pytest.raises(RuntimeError, match="row entry at or above m"):
        synth.merge_mean_normals(np.zeros((4, 2), np.int32) + 3, 3, np.arange(4, dtype=np.uint32), 3)
    with pytest.raises(RuntimeError, match="a code outside"):
        synth.merge_mean_normals(np.full((2, 2), 7, np.int32), 3, np.zeros(2, np.uint32), 1)
    with pytest.raises(RuntimeError, match="2 - 20 bits"):
        synth.merge_mean_normals(np.zeros((2, 2), np.int32), 21, np.zeros(2, np.uint32), 1)


@pytest.mark.parametrize("nbits", [2, 3, 4, 5, 6, 8])
def test_idempotence_on_every_canonical_code(nbits):
    """a cell whose rows all carry the same code keeps it: every canonical code, 2 - 4 rows"""
    codes = np.array(nc.canonical_codes(nbits), np.int32)
    assert len(codes) > ((1 << nbits) - 3) ** 2
    for rows in (2, 3, 4):
        q = np.repeat(codes, rows, axis=0)
        cells = np.repeat(np.arange(len(codes)), rows).astype(np.uint32)
        assert np.array_equal(synth.merge_mean_normals(q, nbits, cells, len(codes)), codes), (nbits, rows)


@pytest.mark.parametrize("nbits", [11, 16, 20])
def test_idempotence_on_random_codes(nbits):
    rng = np.random.default_rng(nbits)
    codes = meshutil.oct_quantize(rng.normal(size=(20000, 3)), nbits).astype(np.int32)
    q = np.repeat(codes, 3, axis=0)
    cells = np.repeat(np.arange(len(codes)), 3).astype(np.uint32)
    assert np.array_equal(synth.merge_mean_normals(q, nbits, cells, len(codes)), codes)
    assert all(nc.mean_code([tuple(c)] * 3, nbits) == tuple(c) for c in codes[:300].tolist())


def random_cells(nbits, count, seed):
    """`count` cells of 2 - 6 rows, quantised by the numpy quantiser: (codes (N, 2), row_entries (N,), sizes).  The rows of a cell are
    what the points of a voxel carry: directions scattered widely (a normal deviate of 0.7 per component) around an axis of the
    cell's own, drawn uniformly from the sphere -- rows drawn from the whole sphere independently cancel in 7 % of the cells at 2
    bits, where six codes are all there is, and say nothing about a mean"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, count)
    axis = rng.normal(size=(count, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    rows = np.repeat(axis, sizes, axis=0) + 0.7 * rng.normal(size=(int(sizes.sum()), 3))
    codes = meshutil.oct_quantize(rows, nbits).astype(np.int32)
    return codes, np.repeat(np.arange(count), sizes).astype(np.uint32), sizes


def directions(codes, nbits):
    """the float64 unit vectors of codes (N, 2), step 1 of the rule in numpy"""
    c = nc.center(nbits)
    a, b = codes[:, 0].astype(np.int64) - c, codes[:, 1].astype(np.int64) - c
    inside = np.abs(a) + np.abs(b) <= c
    sg = lambda x: np.where(x < 0, -1, 1)          # noqa: E731
    v = np.stack([c - np.abs(a) - np.abs(b), np.where(inside, a, sg(a) * (c - np.abs(b))), np.where(inside, b, sg(b) * (c - np.abs(a)))], axis=1).astype(np.float64)
    return v / np.linalg.norm(v, axis=1)[:, None]


def angles(u, v):
    return np.degrees(np.arccos(np.clip((u * v).sum(axis=1), -1.0, 1.0)))


@pytest.mark.parametrize("nbits", [2, 3, 5, 8, 11, 16, 20])
def test_against_the_float64_normalised_sum(nbits):
    """20 000 random cells: the rule's code against the float64 sum of the rows' unit vectors, normalised.  Cells whose sum is
    shorter than 1e-3 have no direction to compare with (at most 5 % of the cells).  The angle between the rule's code and the
    float64 direction must not exceed the largest angle the numpy quantiser itself makes on these directions at these bits: the bound
    is computed here, from the quantiser's own error, not a constant"""
    count = 20000
    codes, cells, sizes = random_cells(nbits, count, 4000 + nbits)
    got = synth.merge_mean_normals(codes, nbits, cells, count)
    assert np.array_equal(directions(codes[:50], nbits), np.array([nc.direction(c, nbits) for c in codes[:50]]))
    total = np.zeros((count, 3))
    np.add.at(total, cells, directions(codes, nbits))
    length = np.linalg.norm(total, axis=1)
    keep = length > 1e-3
    assert keep.mean() >= 0.95, (nbits, 1.0 - keep.mean())
    d = total[keep] / length[keep][:, None]
    quantiser = angles(directions(meshutil.oct_quantize(d, nbits), nbits), d)
    rule = angles(directions(got[keep], nbits), d)
    print("normal bits %d: %d of %d cells compared, the rule's largest angle %.6f degrees, the quantiser's %.6f, codes that differ %d"
          % (nbits, int(keep.sum()), count, rule.max(), quantiser.max(), int((got[keep] != meshutil.oct_quantize(d, nbits)).any(axis=1).sum())))
    assert rule.max() <= quantiser.max(), (nbits, rule.max(), quantiser.max())
    # and the twin is the pin on a part of them
    first = np.concatenate([[0], np.cumsum(sizes)])
    for j in range(0, count, 40):
        assert tuple(got[j]) == nc.mean_code(codes[first[j]:first[j + 1]], nbits), (nbits, j)


@pytest.mark.parametrize("case", nc.cases(), ids=lambda c: c.name)
def test_the_twin_decodes_to_the_pin(case):
    kept, cells, want = nc.pin(case)
    stream, k, c = synth.encode_merged(mean_normals=True, **nc.cpu_args(case))
    assert np.array_equal(k, kept) and np.array_equal(c, cells)
    assert np.array_equal(nc.decoded([stream]), want), case.name
    # positions are never touched, and the decoded floats are the dequantised codes of the pin
    plain = oracle.decode(synth.encode_merged(**nc.cpu_args(case))[0])
    dec = oracle.decode(stream)
    assert np.array_equal(dec.attributes[0].portable, plain.attributes[0].portable) and dec.num_points == len(kept)
    assert np.array_equal(plain.attributes[1].portable, nc.codes_of_rows(case)[kept])
    assert np.ascontiguousarray(dec.attributes[1].values, np.float32).tobytes() == nc.dequantised(case).tobytes()


def test_the_designed_cases_are_what_they_say():
    names = {c.name for c in nc.cases()}
    assert names >= {"idempotent-%d" % b for b in (2, 3, 4, 5, 6)} | {"tile-with-no-head-8", "cloud-1", "cloud-2", "cloud-63", "cloud-64", "cloud-65", "cloud-1025", "cloud-2100"}
    assert {c.nbits for c in nc.cases()} >= {2, 3, 8, 11, 20} and max(len(c.pos) for c in nc.cases()) < 12000
    assert all(c.bits == 6 for c in nc.cases() if c.name.startswith("cloud-"))
    for nbits in nc.NORMAL_BITS:
        # the fold: the mean of the integers (s, t) points elsewhere -- more than 45 degrees off -- where the rule is within a degree or the bits' step
        case = nc.named("fold-and-diamond-edge-%d" % nbits)
        kept, cells, want = nc.pin(case)
        q = nc.codes_of_rows(case)
        for j in (0, 1, 2):
            rows = q[cells == j]
            true = sum(nc.direction(r, nbits) for r in rows)
            true /= np.linalg.norm(true)
            assert true[0] < -0.5 and (nbits < 8 or len({tuple(np.sign(r - nc.center(nbits))) for r in rows}) >= 2)        # x < 0, codes in different corners of the square
            naive = nc.direction(nc.canonical(*[int(v) for v in np.floor(rows.mean(axis=0) + 0.5)], nbits), nbits)
            rule = nc.direction(want[j], nbits)
            if nbits >= 8:
                assert np.degrees(np.arccos(naive @ true)) > 45.0 and np.degrees(np.arccos(rule @ true)) < 1.5, (nbits, j)
            assert rule @ true >= naive @ true - 1e-12
        # the diamond edge: the rows of cells 3 and 4 lie on both sides of |a| + |b| = c
        for j in (3, 4):
            inside = {bool(abs(int(s) - nc.center(nbits)) + abs(int(t) - nc.center(nbits)) <= nc.center(nbits)) for s, t in q[cells == j]}
            assert nbits < 8 or inside == {True, False}, (nbits, j)
        # the long run spans three tiles
        case = nc.named("runs-1-2-5-3000-%d" % nbits)
        assert sorted(np.bincount(nc.pin(case)[1]).tolist())[-1] == 3000 and 3000 > 2 * nc.TILE
        # the ties are ties
        case = nc.named("ties-%d" % nbits)
        kept, cells, want = nc.pin(case)
        q = nc.codes_of_rows(case)
        pairs = [[tuple(int(v) for v in r) for r in q[cells == j]] for j in range(len(kept))]
        assert any(nc.tie_in_step_5(p, nbits) for p in pairs) and (nbits < 8 or sum(nc.tie_in_step_4(p, nbits) for p in pairs) >= 3)
    # opposite normals give the code of (1, 0, 0), at every bit count
    for nbits in nc.NORMAL_BITS:
        c = nc.center(nbits)
        assert nc.mean_code([(c, c), ((1 << nbits) - 2, (1 << nbits) - 2)], nbits) == (c, c)


@pytest.mark.parametrize("name", ["runs-1-2-5-3000-8", "fold-and-diamond-edge-11", "ties-20", "cloud-2100", "axes-corners-zero-opposite-3"])
def test_the_order_of_the_rows_does_not_matter(name):
    """two shuffles of the same cloud: byte-equal streams, normals included, which without the option differ"""
    case = nc.named(name)
    n = len(case.pos)
    orders = [np.random.default_rng(seed).permutation(n) for seed in (31, 32)]
    streams = [synth.encode_merged(mean_normals=True, **nc.cpu_args(case, rows))[0] for rows in orders]
    assert streams[0] == streams[1] == synth.encode_merged(mean_normals=True, **nc.cpu_args(case))[0]
    plain = [synth.encode_merged(**nc.cpu_args(case, rows))[0] for rows in orders]
    assert plain[0] != plain[1]


def beside(case, seed=77):
    """a colour to average (attribute 2) and a label to vote on (attribute 3) beside the normals of a case"""
    rng = np.random.default_rng(seed)
    n = len(case.pos)
    return rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 4, (n, 1)).astype(np.uint8)


def test_mean_normals_false_is_the_vote_twin():
    case = nc.named("runs-1-2-5-3000-8")
    colour, label = beside(case)
    args = nc.cpu_args(case, extra=None)
    args["extra"] = [synth.Extra(colour), synth.Extra(label)]
    masks = dict(mean_attributes=0b100, vote_attributes=0b1000)
    assert synth.encode_merged(mean_normals=False, **masks, **args)[0] == synth.encode_merged(**masks, **args)[0]
    a = synth.encode_lod_parts(part_cells=64, lod_base_bits=10, mean_normals=False, **masks, **args)
    b = synth.encode_lod_parts(part_cells=64, lod_base_bits=10, **masks, **args)
    assert a.streams == b.streams and len(a.streams) >= 2
    with_normals = synth.encode_merged(mean_normals=True, **masks, **args)[0]
    assert with_normals != synth.encode_merged(**masks, **args)[0]
    # the other attributes are what the masks alone make them
    da, db = oracle.decode(with_normals), oracle.decode(synth.encode_merged(**masks, **args)[0])
    assert all(np.array_equal(da.attributes[k].portable, db.attributes[k].portable) for k in (0, 2, 3)) and not np.array_equal(da.attributes[1].portable, db.attributes[1].portable)
    # a cloud without normals: the option changes nothing
    bare = dict(args, normals=None)
    assert synth.encode_merged(mean_normals=True, mean_attributes=0b10, vote_attributes=0b100, **bare)[0] == synth.encode_merged(mean_attributes=0b10, vote_attributes=0b100, **bare)[0]
    # a mask on the normals stays refused
    for kw in (dict(mean_attributes=0b10), dict(vote_attributes=0b10)):
        with pytest.raises(ValueError, match="normals"):
            synth.encode_merged(mean_normals=True, **kw, **args)


def test_parts_and_levels_carry_the_mean_normals():
    """the cell-parts and lod twins: the joined entries of the parts are the pin's, in kept and in lod order"""
    case = nc.named("cloud-2100")
    kept, cells, want = nc.pin(case)
    parts = synth.encode_cell_parts(part_cells=64, mean_normals=True, **nc.cpu_args(case))
    assert len(parts.streams) >= 2 and np.array_equal(parts.kept, kept)
    assert np.array_equal(nc.decoded(parts.streams), want)
    lod = synth.encode_lod_parts(part_cells=64, lod_base_bits=2, mean_normals=True, **nc.cpu_args(case))
    at = np.zeros(len(cells), np.int64)
    at[kept] = np.arange(len(kept))
    assert len(lod.streams) >= 3 and not np.array_equal(lod.kept, kept)
    assert np.array_equal(nc.decoded(lod.streams), want[at[lod.kept]])
