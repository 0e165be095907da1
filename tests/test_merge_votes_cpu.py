"""The host coder's twin of vote_attributes (synth.merge_votes, synth.encode_merged / encode_cell_parts / encode_lod_parts with
vote_attributes=; dsa_encode_host.h merge_votes): its streams decode, through the oracle, to the contract restated in Python
(votecases.pin: q from the oracle's decode of the plain ordered stream of all rows, collections.Counter per cell, the highest count,
then min of the tuples), on every case of votecases; vote_attributes=0 is the mean twin byte for byte; the result does not depend on
the order of the rows.  No GPU needed: what the device must write is held to these twins by tests/test_gpu_encode_votes.py."""
import numpy as np
import pytest

import oracle
import votecases as vc
import draco_sharp_amd.synth as synth


def test_the_rule_on_designed_sets():
    """the most rows, then the smallest signed tuple, in synth.merge_votes itself, with one and with two components"""
    sets = [[3, 5], [5, 3, 5, 3], [-1, 0], [-128, 127], [2, 2, 1], [7], [-2**31, 2**31 - 1], [9] * 70 + list(range(64)), [4, 4, -6, -6, -6]]
    want = [3, 3, -1, -128, 2, 7, -2**31, 9, -6]
    assert [vc.vote([[x] for x in s])[0] for s in sets] == want
    q = np.concatenate([np.asarray(s, np.int64) for s in sets]).astype(np.int32)
    cells = np.repeat(np.arange(len(sets)), [len(s) for s in sets]).astype(np.uint32)
    for order in (np.arange(len(q)), np.random.default_rng(1).permutation(len(q))):
        got = synth.merge_votes(q[order].reshape(-1, 1), cells[order], len(sets))
        assert got.dtype == np.int32 and got[:, 0].tolist() == want
    pairs = [[(4, 9), (4, -2)], [(1, 100), (2, -100)], [(-5, 0), (3, -7), (-5, 0), (3, -7)], [(0, 0), (0, 1), (0, 1)], [(-2**31, 5), (-2**31, -2**31)]]
    q2 = np.concatenate([np.asarray(s, np.int64) for s in pairs]).astype(np.int32)
    cells2 = np.repeat(np.arange(len(pairs)), [len(s) for s in pairs]).astype(np.uint32)
    assert synth.merge_votes(q2, cells2, len(pairs)).tolist() == [[4, -2], [1, 100], [-5, 0], [0, 1], [-2**31, -2**31]]
    with pytest.raises(RuntimeError, match="row entry at or above m"):
        synth.merge_votes(q.reshape(-1, 1), cells, len(sets) - 1)
    with pytest.raises(RuntimeError, match="1 - 2 integers"):
        synth.merge_votes(np.zeros((4, 3), np.int32), np.zeros(4, np.uint32), 1)


@pytest.mark.parametrize("case", vc.cases(), ids=lambda c: c.name)
def test_the_twin_decodes_to_the_pin(case):
    kept, cells, want = vc.pin(case)
    stream, k, c = synth.encode_merged(vote_attributes=case.vote, mean_attributes=case.mean, **vc.cpu_args(case))
    assert np.array_equal(k, kept) and np.array_equal(c, cells)
    got = vc.decoded([stream])
    assert sorted(got) == sorted(want) and case.vote != 0 and case.vote >> (1 + len(got)) == 0
    for a in want:
        assert np.array_equal(got[a], want[a]), (case.name, a)
    # positions are never touched, without the masks every attribute carries row kept[j], and the header of a voted quantised
    # attribute is the one of the plain merged stream: bounds and grid untouched
    plain = oracle.decode(synth.encode_merged(**vc.cpu_args(case))[0])
    dec = oracle.decode(stream)
    assert np.array_equal(dec.attributes[0].portable, plain.attributes[0].portable) and dec.num_points == len(kept)
    for a in want:
        if not ((case.vote | case.mean) >> a) & 1:
            assert np.array_equal(vc.signed(plain.attributes[a].portable), want[a])
        assert (dec.attributes[a].q_min, dec.attributes[a].q_range, dec.attributes[a].q_bits) == (plain.attributes[a].q_min, plain.attributes[a].q_range, plain.attributes[a].q_bits)


def test_the_designed_cases_are_what_they_say():
    late, spread = vc.named("late-winner"), vc.named("spread-majority")
    kept, cells, _ = vc.pin(late)
    rows = np.flatnonzero(cells == 0)                       # ascending rows: the sorted order of the cell
    assert len(rows) == 130 and len(set(late.extras[0][0][rows[:64], 0].tolist())) == 64 and set(late.extras[0][0][rows[64:], 0].tolist()) == {200}
    kept, cells, _ = vc.pin(spread)
    rows = np.flatnonzero(cells == 0)
    at = np.flatnonzero(spread.extras[0][0][rows, 0] == 7)
    assert sorted(at // 64) == [0, 1, 2, 3, 4] and all(at % 64 != 0)
    assert {c.name for c in vc.cases()} >= {"run-over-63|64", "run-over-1023|1024", "tile-with-no-head", "identical-%d" % (2 * vc.TILE + 1), "one-point"}
    assert max(len(c.pos) for c in vc.cases()) < 8000


def test_mask_0_is_the_mean_twin():
    case = vc.named("mixed-mask")
    args = vc.cpu_args(case)
    assert synth.encode_merged(mean_attributes=case.mean, vote_attributes=0, **args)[0] == synth.encode_merged(mean_attributes=case.mean, **args)[0]
    a = synth.encode_lod_parts(part_cells=64, lod_base_bits=10, mean_attributes=case.mean, vote_attributes=0, **args)
    b = synth.encode_lod_parts(part_cells=64, lod_base_bits=10, mean_attributes=case.mean, **args)
    assert a.streams == b.streams and len(a.streams) >= 2
    assert synth.encode_merged(mean_attributes=case.mean, vote_attributes=case.vote, **args)[0] != synth.encode_merged(mean_attributes=case.mean, **args)[0]


@pytest.mark.parametrize("name", ["ties", "pairs", "all-distinct-3000", "three-way-tie-3000", "same-two-values"])
def test_the_order_of_the_rows_does_not_matter(name):
    """two shuffles of the same cloud: byte-equal streams, which without the mask differ"""
    case = vc.named(name)
    n = len(case.pos)
    orders = [np.random.default_rng(seed).permutation(n) for seed in (21, 22)]      # (whose first rows carry different values, also in the clouds of one cell)
    streams = [synth.encode_merged(vote_attributes=case.vote, **vc.cpu_args(case, rows))[0] for rows in orders]
    assert streams[0] == streams[1] == synth.encode_merged(vote_attributes=case.vote, **vc.cpu_args(case))[0]
    plain = [synth.encode_merged(**vc.cpu_args(case, rows))[0] for rows in orders]
    assert plain[0] != plain[1]


def test_parts_and_levels_carry_the_votes():
    """the cell-parts and lod twins: the joined entries of the parts are the pin's, in kept and in lod order"""
    case = vc.named("mixed-mask")
    kept, cells, want = vc.pin(case)
    parts = synth.encode_cell_parts(part_cells=64, vote_attributes=case.vote, mean_attributes=case.mean, **vc.cpu_args(case))
    assert len(parts.streams) >= 2 and np.array_equal(parts.kept, kept)
    got = vc.decoded(parts.streams)
    for a in want:
        assert np.array_equal(got[a], want[a]), a
    lod = synth.encode_lod_parts(part_cells=64, lod_base_bits=2, vote_attributes=case.vote, mean_attributes=case.mean, **vc.cpu_args(case))
    at = np.zeros(len(cells), np.int64)
    at[kept] = np.arange(len(kept))
    got = vc.decoded(lod.streams)
    assert len(lod.streams) >= 3 and not np.array_equal(lod.kept, kept)
    for a in want:
        assert np.array_equal(got[a], want[a][at[lod.kept]]), a


def test_refusals_of_the_twin():
    assert [c.name for c, _, _, _ in vc.refusals()] == ["three-components", "normals", "positions", "missing-attribute", "both-masks"]
    for case, _, _, text in vc.refusals():
        with pytest.raises((ValueError, RuntimeError), match=text):
            synth.encode_merged(vote_attributes=case.vote, mean_attributes=case.mean, **vc.cpu_args(case))
    case = vc.named("ties")
    for vote, mean, text in ((1, 0, "positions and normals"), (1 << 9, 0, "does not have"), (2, 2, "share a bit")):
        with pytest.raises(ValueError, match=text):
            synth.encode_merged(vote_attributes=vote, mean_attributes=mean, **vc.cpu_args(case))
