"""The designed symbol streams of tests/encsymbolcases.py, held to their conditions on the CPU.  Every case is an int32 attribute of
a point cloud, written by the CPU coder (synth.encode_point_cloud_attributes): the oracle must return the designed symbols and the
input array; tests/ransref.py -- a plain reference of the entropy layer -- must read the designed symbols from the attribute's
section and write the coder's rANS bytes from the table it parsed; and every entry of the case's `expect` must hold, read from
ransref's trace of the section and from encsymbolcases.write_trace, a trace of RAnsEncoder.Write made of ransref.rans_encode.  An
entry of `expect` that nothing here checks fails the test."""
import collections

import numpy as np
import pytest

import encsymbolcases as E
import oracle
import ransref
import symbolcases as S
import test_symbol_designs_cpu as D

NAMES = [c.name for c in E.CASES]
Report = collections.namedtuple("Report", "syms trace write normalised")
_reports = {}


def report(c):
    """(ransref's symbols, its Trace, the WriteTrace, normalise() of the coded histogram) of the attribute's section, made once."""
    if c.name not in _reports:
        b = E.built(c)
        at = E.attribute_section(b.stream, c.n)
        syms, end, tr = ransref.parse_section(b.stream, at, c.n * c.nc, c.nc)
        assert end == len(b.stream) - 25, (c.name, end, len(b.stream))
        coded = tr.tags if tr.scheme == 0 else syms
        counts = np.bincount(coded, minlength=33 if tr.scheme == 0 else 0).tolist()
        _reports[c.name] = Report(syms, tr, E.write_trace(coded, tr.freq, tr.cum, tr.precision), E.normalise(counts, tr.precision))
    return _reports[c.name]


# ------------------------------------------------------------------------------------------------------- the carrier
def test_the_transform_restated_wraps_at_both_parities():
    """max_dif 5: corrections -2 .. 2; max_dif 4: -2 .. 1 (the rule carry() leans on: m residues, symbols 0 .. m - 1)"""
    assert E.transform(np.array([[0], [4], [0], [2], [4], [1]]), 1).tolist() == [0, 1, 2, 4, 4, 4]
    assert E.transform(np.array([[0], [3], [0], [2], [3], [1]]), 1).tolist() == [0, 1, 2, 3, 2, 3]
    for m in (4, 5):
        every = E.carry([0, 1] + list(range(m)), 1, m)
        assert every is not None and every[1] == m


def test_at_least_75_designs_are_carried_unchanged_and_at_most_4_are_not():
    assert len(E.NOT_CARRIED) <= 4 and len(E.CARRIED) >= 75 and len(E.CARRIED) + len(E.NOT_CARRIED) == len(S.CASES)
    by = {c.name: c for c in S.CASES}
    for name in E.CARRIED:
        c, mine = by[name], E.BY_NAME[name]
        assert E.built(mine).seq == list(c.make(c)) and (mine.scheme, mine.level, mine.family, mine.nc) == (c.scheme, c.level, c.family, c.nc)
    for name, reason in E.NOT_CARRIED:
        c = by[name]
        assert reason and E.carry(c.make(c), c.nc) is None, name                  # no m of the searched range reaches both ends
        stand_in = E.BY_NAME[name + "-ballast"]
        seq = E.built(stand_in).seq
        assert seq[len(seq) - len(c.make(c)):] == list(c.make(c))                  # the whole sequence, behind the ballast


def test_sizes_are_what_the_conditions_need():
    big = {c.name for c in E.CASES if c.n * c.nc > 45000}
    assert big == set(E.FREQ1_NAMES) | {"histogram-cap-4097", "histogram-cap-4098", "histogram-cap-4099"}
    assert all(E.BY_NAME[n].n * E.BY_NAME[n].nc == 176400 for n in big)
    assert len(E.WIDE_ALPHABETS) <= 3
    assert {c.family for c in E.CASES} == set(E.FAMILIES) and all(E.family(f) for f in E.ENCODE_FAMILIES)


# ------------------------------------------------------------------------------------------------------ every case
def check_encode_expectations(c, b, r):
    """The conditions of a case of the encode direction, each from the traces."""
    e = dict(c.expect)
    tr, w, nz = r.trace, r.write, r.normalised
    coded = tr.tags if tr.scheme == 0 else r.syms
    assert tr.precision == e.pop("precision", 12)
    if "freq" in e:
        assert tr.freq == e.pop("freq")
    if "num_distinct" in e:
        assert tr.num_distinct == e.pop("num_distinct")
    if "size_rans" in e:
        assert tr.size_rans == e.pop("size_rans")
    if "size_mod" in e:
        assert w.size % 64 == e.pop("size_mod")                        # bytes held at the last store of the 64-lane register
    if "count_mod" in e:
        assert len(coded) % 64 == e.pop("count_mod")                   # symbols of the last stretch
    if "flush_straddles" in e:
        assert E.flush_straddles(w) == e.pop("flush_straddles") and w.flush_bytes > 1
    if "flush_bytes" in e:
        assert w.flush_bytes == e.pop("flush_bytes") == tr.init_form + 1
    if "divide_classes" in e:
        assert e.pop("divide_classes") <= w.classes
        assert w.over >= 1 and w.exact >= 1, (w.over, w.exact)
        assert "power-of-two" not in w.over_classes and "one" not in w.over_classes          # 2^32 / p is exact there
    if "normalise" in e:
        assert nz.branch == e.pop("normalise")
    if "long_by" in e:
        assert nz.excess == e.pop("long_by")
    if "long_by_at_least" in e:
        assert nz.excess >= e.pop("long_by_at_least")
    if "sweep_stops_at_one" in e:
        assert nz.stops_at_one == e.pop("sweep_stops_at_one") and nz.sweeps >= 2
    if "choice" in e:
        tagged, raw = E.scheme_totals(b.seq, c.nc)
        assert tagged - raw == e.pop("choice") and c.scheme == -1
        assert tr.scheme == (0 if tagged < raw else 1)                 # the scheme byte the coder wrote: tagged only when strictly cheaper
    if e.pop("choice_raw_cheaper", False):
        tagged, raw = E.scheme_totals(b.seq, c.nc)
        assert raw < tagged and max(b.seq).bit_length() == 19 and c.scheme == -1
    if "scheme_written" in e:
        assert tr.scheme == e.pop("scheme_written")
    if "hist_cap" in e:
        span = int(b.values.max()) - int(b.values.min())
        assert span + 3 == b.m + 2 == e.pop("hist_cap") and tr.scheme == 1       # enc_integer_hist_cap(lo, hi)
    if "count_above" in e:
        assert max(np.bincount(b.seq)) > e.pop("count_above")
    if "top_symbol" in e:
        assert max(b.seq) == e.pop("top_symbol") == b.m - 1
    if "tags" in e:
        assert set(tr.tags) == e.pop("tags") and tr.scheme == 0
    if "max_symbol" in e:
        assert max(b.seq) == e.pop("max_symbol") >= 1 << 18
    assert not e, e


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_its_conditions(name):
    c = E.BY_NAME[name]
    b = E.built(c)
    r = report(c)
    tr, w = r.trace, r.write
    print(name, "m", b.m, "precision", tr.precision, "rANS bytes", tr.size_rans, "flush", w.flush_bytes, "at", w.flush_at, "estimate one too large", w.over, "exact",
          w.exact, sorted(w.classes), "normalise", r.normalised.branch, r.normalised.excess)
    # the oracle: the designed symbols, the input array
    ref = oracle.decode(b.stream)
    g = ref.attributes[-1]
    assert g.values.dtype == np.int32 and np.array_equal(g.values, b.values)
    assert [int(s) for s in g.symbols.ravel()] == b.seq
    # ransref: reads the designed symbols, writes the coder's bytes from the table it parsed
    assert r.syms == b.seq
    coded = tr.tags if tr.scheme == 0 else r.syms
    section = b.stream[tr.off_rans:tr.off_rans + tr.size_rans]
    assert ransref.rans_encode(coded, tr.freq, tr.cum, tr.precision) == section
    assert w.size == tr.size_rans and w.flush_bytes == tr.init_form + 1 and w.over + w.exact == len(coded)
    # the table is rans_tables' of the coded histogram
    assert r.normalised.prob == tr.freq
    if c.source is not None:
        D.check_expectations(c, b.seq, tr)
    else:
        check_encode_expectations(c, b, r)


def test_an_unknown_expectation_fails():
    c = E.BY_NAME["length-flush-straddles"]
    with pytest.raises(AssertionError):
        check_encode_expectations(c._replace(expect=dict(c.expect, nobody_checks_this=1)), E.built(c), report(c))


# -------------------------------------------------------------------------------------------- what the list covers
def test_every_branch_form_outcome_and_residue_is_named_by_a_case():
    new = [c for c in E.CASES if c.source is None]
    assert {c.expect["normalise"] for c in new if "normalise" in c.expect} == {"exact", "short", "long"}
    assert {report(c).normalised.branch for c in E.family("enc-normalise")} == {"exact", "short", "long"}
    assert any(c.expect.get("long_by") == 1 for c in new) and any(c.expect.get("sweep_stops_at_one") for c in new)
    assert {c.expect["flush_bytes"] for c in E.family("enc-flush")} | {report(c).write.flush_bytes for c in E.family("flush")} == {1, 2, 3, 4}
    assert {c.expect["flush_bytes"] for c in E.family("enc-flush") if c.expect.get("precision") == 16} == {2, 3, 4}
    assert {c.expect["size_mod"] for c in E.family("enc-length") if "count_mod" in c.expect} == {0, 1, 63}
    assert {c.expect["count_mod"] for c in E.family("enc-length") if "count_mod" in c.expect} == {0, 1, 63}
    assert any(c.expect.get("flush_straddles") for c in E.family("enc-length"))
    divide = E.family("enc-divide")
    assert {c.expect["precision"] for c in divide} == {12, 16, 20}
    assert set().union(*[c.expect["divide_classes"] for c in divide]) == {"one", "power-of-two", "other", "near-full"}
    assert all(report(c).write.over and report(c).write.exact for c in divide)
    assert sorted(c.expect["choice"] for c in E.family("enc-choice") if "choice" in c.expect) == [-1, 0, 1]
    assert sorted(c.expect["hist_cap"] for c in E.family("enc-histogram") if c.n * c.nc == 176400) == [4097, 4098, 4099]
    assert sorted(c.nc for c in E.family("enc-tagged-bits")) == [1, 2, 3, 4]
    assert {report(c).trace.precision for c in E.CASES} == {12, 13, 15, 16, 18, 19, 20}


def test_the_estimate_is_exact_for_powers_of_two_and_one_too_large_elsewhere():
    """what the correction step of k_enc_rans is for, in int: ceil(2^32 / p) is 2^32 / p for a power of two, and above it by less
    than 1 / p otherwise, so the estimate exceeds the quotient by less than state / 2^32 < 1"""
    seen = set()
    for p in (1, 3, 1 << 7, 4095, 4096, (1 << 20) - 5, 1 << 20):
        for x in list(range(4 * p, 4 * p + 300)) + list(range(1024 * p - 300, 1024 * p)) + [k * p - 1 for k in range(5, 1024, 7)]:
            est, q = (x * (0xFFFFFFFF // p + 1)) >> 32, x // p
            assert est - q in ((0,) if p & (p - 1) == 0 else (0, 1)), (p, x)
            seen.add((p, est - q))
    assert {(4095, 1), ((1 << 20) - 5, 1)} <= seen and (3, 1) not in seen        # (a small p never: x p < 2^32)


# ------------------------------------------------------------------------------------------------------- refusals
def test_the_refused_cases_hold_symbols_of_2_18_and_above():
    """the raw scheme forced on them is refused by the device encoder (test_gpu_encode_symbol_designs.py); left to itself the coder
    writes them tagged"""
    assert len(E.REFUSED) >= 2
    for c, scheme, words in E.REFUSED:
        assert scheme == 1 and c.scheme != 1 and words == E.RAW_BEYOND
        assert max(E.built(c).seq) >= 1 << 18 and report(c).trace.scheme == 0


def test_one_changed_value_is_noticed():
    for name in ("length-size-63-count-63", "divide-16", "choice-difference--1", "tagged-bits-x3"):
        c = E.BY_NAME[name]
        b = E.built(c)
        v = b.values.copy()
        v[c.n // 2, 0] += 1 if v[c.n // 2, 0] < v.max() else -1
        other = E.cpu_stream(c, v)
        assert other != b.stream and not np.array_equal(oracle.decode(other).attributes[-1].values, b.values)
