"""The rows a coded stream carries, on the CPU: the host coder's entry rows (synth.entry_rows, the twin the device's
dsa_encoded_entry_rows is held to in tests/test_gpu_source_rows.py) put through the oracle's point maps and held to the pins of
tests/rowcases.py, which are written from the values passed and the decoded stream, not from the coder's bookkeeping: (a) counters
that decode to the rows, (b) the bytes of the row named, (c) normals of 14 directions, (d) the identity of linear streams -- over
indexed, seamed, listed-id, repaired and welded input, in depth-first and prediction-degree order.  No GPU needed."""
import numpy as np
import pytest

import oracle
import rowcases as R

GROUPS = R.cases()


def decoded_rows(c):
    ref = oracle.decode(R.encode(c))
    decoded, num_points = R.from_oracle(ref)
    entry = R.twin(c)
    assert [len(e) for e in entry] == [len(d.values) for d in decoded], c.name          # an array per attribute, an element per entry
    return decoded, num_points, R.rows_by_point(entry, decoded, num_points)


def test_the_cases_hold_what_the_issue_asks_for():
    names = [c.name for c in R.all_cases()]
    assert len(set(names)) == len(names)
    points = [len(c.pos) for c in GROUPS["grids"]]
    assert min(points) == 20 and max(points) >= 17 * 13                  # 5 x 4 to 17 x 13 points
    assert {c.name.split("/")[0] for c in GROUPS["grids"]} >= {"holes16x12", "torus9x7", "two-parts10x7"}
    assert any(c.opt.get("traversal_method") == 1 for c in R.all_cases()) and any(c.opt.get("traversal_method") == 2 for c in R.all_cases())
    assert any(c.opt.get("predictive_connectivity") == 2 for c in R.all_cases())
    assert any(c.weld_attributes for c in GROUPS["welded"]) and any(not c.weld_attributes for c in GROUPS["welded"])
    assert {c.opt.get("repair_topology") for c in GROUPS["repaired"]} == {1, 2}
    assert len(R.DIRECTIONS) == 14 and np.sort((R.DIRECTIONS @ R.DIRECTIONS.T).ravel())[-15] < np.cos(np.radians(54))


@pytest.mark.parametrize("c", GROUPS["grids"] + GROUPS["seamed"] + GROUPS["listed"] + GROUPS["repaired"], ids=lambda c: c.name)
def test_counters_decode_to_the_rows(c):
    """(a), and (b) on the same stream."""
    cc, counter, mirrors = R.with_counters(c)
    decoded, num_points, rows = decoded_rows(cc)
    R.check_counters(cc, counter, mirrors, decoded, num_points, rows)
    R.check_bytes(cc, decoded, num_points, rows)
    if cc.nid is not None or cc.uid is not None:
        assert mirrors, c.name


SPLIT = {}


def representatives(arrays, used, count):
    """Per point the smallest used point whose rows in every array are byte-equal (unused points: themselves)."""
    key = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(count, -1) for a in arrays], axis=1)
    rep, first = np.arange(count), {}
    for p in used.tolist():
        rep[p] = first.setdefault(key[p].tobytes(), p)
    return rep


@pytest.mark.parametrize("c", GROUPS["welded"], ids=lambda c: c.name)
def test_welded_rows_name_points_with_the_bytes_that_were_coded(c):
    """(b), and which point: a row is the representative -- the smallest used point -- of a class of the key set the attribute is
    welded by: its own where some vertex has two of its rows, else the vertex's (positions, the generic attribute, the attributes
    of the list that stay in the vertex key, and every set no vertex has two of).  The classes are restated here from the bytes."""
    decoded, num_points, rows = decoded_rows(c)
    R.check_bytes(c, decoded, num_points, rows)
    vals, used, P = R.values(c), np.unique(c.faces), len(c.pos)
    base = len(vals) - len(c.extras)
    alone = [c.weld_attributes and base + k <= 7 for k in range(len(c.extras))]          # (a corner attribute's index in the stream is at most 7)
    own = [False] + [True] * ((c.nrm is not None) + (c.uv is not None)) + [False] * (c.generic is not None) + alone
    assert len(own) == len(vals)
    vertex = representatives([v for v, o in zip(vals, own) if not o], used, P)
    split = 0
    for a, (v, r) in enumerate(zip(vals, rows)):
        assert np.isin(r, used).all(), (c.name, a)
        rep = vertex
        if own[a]:
            mine = representatives([v], used, P)
            if (mine[used] != mine[vertex[used]]).any():          # some vertex has two of its rows: it went on per corner
                rep, split = mine, split + 1
        assert np.array_equal(rep[r.astype(np.int64)], r), (c.name, a)
        assert set(np.unique(r).tolist()) == set(np.unique(rep[used]).tolist()), (c.name, a)          # every class is in the stream, by its representative
    SPLIT[c.name] = split


def test_both_kinds_of_key_set_were_among_them():
    """(behind the test above) attributes that went on per corner, by their own classes, and ones that stayed per vertex."""
    assert len(SPLIT) == len(GROUPS["welded"]) and sum(1 for v in SPLIT.values() if v) >= 10 and sum(1 for v in SPLIT.values() if not v) >= 3, SPLIT


@pytest.mark.parametrize("c", [g for g in GROUPS["grids"][::3] + GROUPS["seamed"][::3] + GROUPS["repaired"][::4] + GROUPS["welded"][::3] if g.nrm is not None], ids=lambda c: c.name)
def test_normals_of_fourteen_directions(c):
    """(c)"""
    cd = R.with_directions(c)
    decoded, num_points, rows = decoded_rows(cd)
    R.check_normals(cd, decoded, num_points, rows)


@pytest.mark.parametrize("c", GROUPS["linear"], ids=lambda c: c.name)
def test_linear_streams_are_the_identity(c):
    """(d)"""
    entry = R.twin(c)
    assert len(entry) == len(R.values(c))
    for e in entry:
        assert np.array_equal(e, np.arange(len(c.pos), dtype=np.uint32))
    decoded, num_points, rows = decoded_rows(c)
    R.check_bytes(c, decoded, num_points, rows)


def test_prediction_degree_order_moves_the_entries():
    """What the traversal cases are taken for: the positions' entries change their order, and the rows follow."""
    c = next(c for c in GROUPS["grids"] if c.opt.get("traversal_method") == 1)
    plain = R.twin(c._replace(opt={}))
    assert not np.array_equal(R.twin(c)[0], plain[0]) and np.array_equal(np.sort(R.twin(c)[0]), np.sort(plain[0]))

