"""The host coder's twin of mean_attributes (synth.merge_means, synth.encode_merged / encode_cell_parts / encode_lod_parts with
mean_attributes=; dsa_encode_host.h merge_means and the portable integers of MeshIn): its streams decode, through the oracle, to the
contract restated in Python integers (meancases.pin: q from the oracle's decode of the plain ordered stream of all rows, the mean
per cell by floor((2 S + cnt) / (2 cnt))), on every case of meancases; the result does not depend on the order of the rows.  No GPU
needed: what the device must write is held to these twins by tests/test_gpu_encode_means.py."""
import numpy as np
import pytest

import meancases as mn
import oracle
import draco_sharp_amd.synth as synth


def test_the_rule_on_designed_sets():
    """ties toward +infinity, negative sums, sums beyond 32 bits, in synth.merge_means itself"""
    sets = [[0, 1], [-1, 0], [-2, -1], [1, 2, 2], [1, 1, 2], [-7], [2**27] * 2049, [-2**27] * 2049, [2**31 - 1] * 3, [-2**31] * 5, [-3, -4], [3, 4]]
    want = [1, 0, -1, 2, 1, -7, 2**27, -2**27, 2**31 - 1, -2**31, -3, 4]
    assert [mn.mean(s) for s in sets] == want
    q = np.concatenate([np.asarray(s, np.int64) for s in sets]).astype(np.int32)
    cells = np.repeat(np.arange(len(sets)), [len(s) for s in sets]).astype(np.uint32)
    rows = np.random.default_rng(1).permutation(len(q))
    for order in (np.arange(len(q)), rows):
        got = synth.merge_means(q[order].reshape(-1, 1), cells[order], len(sets))
        assert got.dtype == np.int32 and got[:, 0].tolist() == want
    two = synth.merge_means(np.stack([q, -q.astype(np.int64)], axis=1).clip(-2**31, 2**31 - 1).astype(np.int32), cells, len(sets))
    assert two[:, 0].tolist() == want and two[:4, 1].tolist() == [0, 1, 2, -2]        # {0,-1} -> 0, {1,0} -> 1, {2,1} -> 2, {-1,-2,-2} -> -2 (-5 / 3 rounds to -2)
    with pytest.raises(RuntimeError, match="row entry at or above m"):
        synth.merge_means(q.reshape(-1, 1), cells, len(sets) - 1)


@pytest.mark.parametrize("case", mn.cases(), ids=lambda c: c.name)
def test_the_twin_decodes_to_the_pin(case):
    kept, cells, want = mn.pin(case)
    stream, k, c = synth.encode_merged(mean_attributes=case.mask, **mn.cpu_args(case))
    assert np.array_equal(k, kept) and np.array_equal(c, cells)
    got = mn.decoded([stream])
    assert sorted(got) == sorted(want) and case.mask != 0 and case.mask >> (1 + len(got)) == 0
    for a in want:
        assert np.array_equal(got[a], want[a]), (case.name, a)
    for a, means in case.expect.items():
        assert (case.mask >> a) & 1 and np.array_equal(want[a], means), (case.name, a)
    # positions are never touched, and without the mask every attribute carries row kept[j]
    plain = oracle.decode(synth.encode_merged(**mn.cpu_args(case))[0])
    dec = oracle.decode(stream)
    assert np.array_equal(dec.attributes[0].portable, plain.attributes[0].portable) and dec.num_points == len(kept)
    for a in want:
        if not (case.mask >> a) & 1:
            assert np.array_equal(plain.attributes[a].portable, want[a])
    # the header of a masked quantised attribute is the one of the plain merged stream: bounds and grid untouched
    for a in want:
        assert (dec.attributes[a].q_min, dec.attributes[a].q_range, dec.attributes[a].q_bits) == (plain.attributes[a].q_min, plain.attributes[a].q_range, plain.attributes[a].q_bits)


def test_wide_sums_leave_32_bits():
    case = next(c for c in mn.cases() if c.name == "wide-sums")
    kept, cells, want = mn.pin(case)
    count = np.bincount(cells)
    assert count.tolist() == [2049, 3, 2049, 4097, 2] and 2049 * 2**27 > 2**32
    assert int(want[2][3, 0]) * 4097 > 2**32 and want[2][3, 0] > 2**20 - 1 - 300           # the float attribute's long run, near the top of its 20 bits


@pytest.mark.parametrize("name", ["signed", "components", "all-of-it", "wide-sums"])
def test_the_order_of_the_rows_does_not_matter(name):
    """two shuffles of the same cloud with every attribute but positions (and normals) masked: byte-equal streams"""
    case = next(c for c in mn.cases() if c.name == name)
    mask = 0
    for a, kind, _ in mn.attributes(case):
        if kind != "normals":
            mask |= 1 << a
    if case.normals is not None:            # the normals of the kept row depend on the order: leave them out of the comparison's input
        case = case._replace(normals=None)
        mask = sum(1 << (a - 1) for a in range(2, 17) if (mask >> a) & 1)
    n = len(case.pos)
    streams = []
    for seed in (11, 12):
        rows = np.random.default_rng(seed).permutation(n)
        streams.append(synth.encode_merged(mean_attributes=mask, **mn.cpu_args(case, rows))[0])
    assert streams[0] == streams[1]
    assert synth.encode_merged(**mn.cpu_args(case, np.random.default_rng(11).permutation(n)))[0] != synth.encode_merged(**mn.cpu_args(case, np.random.default_rng(12).permutation(n)))[0]


def test_parts_and_levels_carry_the_means():
    """the cell-parts and lod twins: the joined entries of the parts are the pin's, in kept and in lod order"""
    case = next(c for c in mn.cases() if c.name == "signed")
    kept, cells, want = mn.pin(case)
    parts = synth.encode_cell_parts(part_cells=64, mean_attributes=case.mask, **mn.cpu_args(case))
    assert len(parts.streams) >= 2 and np.array_equal(parts.kept, kept)
    got = mn.decoded(parts.streams)
    for a in want:
        assert np.array_equal(got[a], want[a]), a
    lod = synth.encode_lod_parts(part_cells=64, lod_base_bits=2, mean_attributes=case.mask, **mn.cpu_args(case))
    at = np.zeros(len(cells), np.int64)
    at[kept] = np.arange(len(kept))
    got = mn.decoded(lod.streams)
    assert len(lod.streams) >= 3 and not np.array_equal(lod.kept, kept)
    for a in want:
        assert np.array_equal(got[a], want[a][at[lod.kept]]), a


def test_refusals_of_the_twin():
    case = mn.cases()[0]
    for mask, text in ((1, "positions and normals"), (1 << 9, "does not have")):
        with pytest.raises(ValueError, match=text):
            synth.encode_merged(mean_attributes=mask, **mn.cpu_args(case))
