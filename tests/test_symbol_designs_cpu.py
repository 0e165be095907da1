"""The designed symbol streams of tests/symbolcases.py, held to their conditions on the CPU.  Every condition is read from the trace
of tests/ransref.py -- a plain reference of the entropy layer written from the reference's files -- not from the coder: the
ReadInit form, the bytes each Read took, the table, the tokens.  Then: ransref's symbols are the designed sequence; the oracle
returns the input array and the same symbols; ransref's encoder reproduces the coder's rANS bytes from the parsed table; the host
parse (tests/hostcheck/needs_host.cpp) names the decoder the case names; the general path's source and the lane kernels, as
stand-alone host programs (tests/hostcheck/general_host.cpp, lanes_host.cpp, built as test_hostcheck.py and test_hostcheck_lanes.py
build them), decode every stream to the input array; and a changed value or a changed byte is noticed."""
import numpy as np
import pytest

import oracle
import prunecases as pc
import ransref
import symbolcases as S
import draco_sharp_amd.synth as synth
import test_hostcheck
import test_hostcheck_lanes

NAMES = [c.name for c in S.CASES]
BY_NAME = {c.name: c for c in S.CASES}

general_exe = test_hostcheck.exe
lanes_exe = test_hostcheck_lanes.exe


@pytest.fixture(scope="module")
def reports():
    """{name: (symbols, Trace, end offset, host mask)} of every case: one run of the host walk for the whole list."""
    rep = S.host_report([S.built(c).stream for c in S.CASES])
    out = {}
    for c, r in zip(S.CASES, rep):
        b = S.built(c)
        out[c.name] = S.trace_of_stream(b.stream, len(b.seq), c.nc, r) + (r[0],)
    return out


# ------------------------------------------------------------------------------------------------ the reference itself
def test_precisions_14_and_17_do_not_exist():
    assert sorted({ransref.precision_of(m) for m in range(1, 19)}) == [12, 13, 15, 16, 18, 19, 20]


@pytest.mark.parametrize("nc,scheme,level,spread", [(1, 1, 5, 40), (3, 1, 10, 300), (2, 1, 3, 5000), (1, 1, 10, 70000), (1, 0, 5, 1 << 17), (4, 0, 5, 900)])
def test_the_reference_and_the_coder_agree_in_both_directions(nc, scheme, level, spread):
    """ransref reads what synth.encode_symbols wrote, and writes the same rANS bytes from the table it parsed."""
    rng = np.random.default_rng([nc, scheme, level, spread])
    values = np.minimum(rng.geometric(4.0 / spread, 4200 * nc) - 1, S.TOP).astype(np.uint32)
    blk = synth.encode_symbols(values, nc, scheme, level)
    syms, end, tr = ransref.parse_section(blk, 0, len(values), nc)
    assert end == len(blk) and syms == [int(v) for v in values] and tr.scheme == scheme
    coded = tr.tags if scheme == 0 else syms
    assert ransref.rans_encode(coded, tr.freq, tr.cum, tr.precision) == blk[tr.off_rans:tr.off_rans + tr.size_rans]


def test_what_the_coder_cannot_write():
    """The arithmetic behind the substitutions symbolcases.py lists."""
    with pytest.raises(ValueError):
        S.level_for(65, 11)                              # 16 bits need 256 distinct symbols: no {65 472, 1 x 64} table
    assert S.level_for(256, 11) == 10 and S.level_for(65, 9) == 10 and S.level_for(128, 10) == 10
    for bits in (12, 13, 15, 16):                        # 2^P distinct symbols put the precision above P ...
        assert all(ransref.precision_of(min(18, (1 << bits).bit_length() + adj)) > bits for adj in (-2, -1, 0, 1, 2))
    assert (1 << 18).bit_length() > 18                   # ... and from 18 bits on they are more than the raw scheme takes
    assert ((4 << 12) * 256 - 1) - (4 << 12) < 1 << 22   # 12 bits: state - l_base never needs ReadInit's 4-byte form
    assert ransref.rans_encode([0] * 7, [4096], [0], 12) == b"\x00"
    assert np.array_equal(np.frombuffer(synth.encode_symbols(np.zeros(4, np.uint32), 1, 0, 5), np.uint8)[:3], [0, 2, 3])     # value 0 has tag 1: {scheme 0, 2 symbols, a zero run of 1}


# ------------------------------------------------------------------------------------------------------ every case
def longest_run(seq, wanted):
    best = run = 0
    for s in seq:
        run = run + 1 if s in wanted else 0
        best = max(best, run)
    return best


def check_expectations(c, seq, tr):
    e = dict(c.expect)
    taken = tr.bytes_per_symbol
    coded = tr.tags if c.scheme == 0 else seq
    low = min(f for f in tr.freq if f)
    rare = {s for s, f in enumerate(tr.freq) if 0 < f <= low + 1}          # (the normalisation takes 1 off some of a group of equals)
    top = tr.freq.index(max(tr.freq))
    assert tr.scheme == c.scheme and tr.precision == e.pop("precision", 12)
    if "freq" in e:
        assert tr.freq == e.pop("freq")
    if "top_freq" in e:
        assert max(tr.freq) == e.pop("top_freq")
    if "num_symbols" in e:
        assert tr.num_symbols == e.pop("num_symbols")
    if "num_distinct" in e:
        assert tr.num_distinct == e.pop("num_distinct")
    if "init_form" in e:
        assert tr.init_form == e.pop("init_form")
    if "size_rans" in e:
        assert tr.size_rans == e.pop("size_rans")
    if "rare_at" in e:
        assert [i for i, s in enumerate(coded) if s in rare] == e.pop("rare_at") and low == 1
    if "last_block" in e:
        assert len(coded) % 64 == e.pop("last_block")
    if "silent_span" in e:
        assert max(k for _, k in ransref.zero_spans(taken)) >= e.pop("silent_span") > 256          # longer than 4 blocks
    if e.pop("window_edge", False):
        assert S.spans_on_a_window_edge(tr)
    if "max_bytes" in e:
        # a symbol leaves a state of 4 at least (quotient 4, frequency 1): 2 bytes lift it to 2^18 = l_base at 16 bits, 3 to 2^26 > l_base at 20
        assert max(taken) == e.pop("max_bytes")
    if "full_block" in e:
        assert ransref.full_blocks(taken, e.pop("full_block"))
    if e.pop("heavy_block", False):
        blocks = [b for b in range(1, len(coded) // 64) if all(s in rare for s in coded[64 * b - 1:64 * b + 64])]     # (a Read takes what the symbol before it cost)
        assert blocks
        if low == 1:
            assert all(8 * tr.precision - 1 <= sum(taken[64 * b:64 * b + 64]) <= 8 * tr.precision + 1 for b in blocks)
    if "top_run" in e:
        run, burst = e.pop("top_run"), e.pop("burst", 0)
        assert any(all(s == top for s in coded[i - run:i]) and all(s in rare for s in coded[i:i + burst])
                   for i in range(run, len(coded) - burst + 1) if coded[i - 1] == top and (burst == 0 or coded[i] in rare))
    if "burst" in e:
        assert longest_run(coded, rare) >= e.pop("burst")
    if "zero_runs" in e:
        runs = ransref.zero_runs(tr.freq)
        assert all(r in runs for r in e.pop("zero_runs"))
    if "run_tokens" in e:
        assert longest_run([t[0] for t in tr.tokens], {"run"}) >= e.pop("run_tokens")
    if "tags" in e:
        assert set(tr.tags) == e.pop("tags")
    assert not e, e


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_its_conditions(reports, name):
    c = BY_NAME[name]
    b = S.built(c)
    syms, tr, end, mask = reports[name]
    assert syms == b.seq and end == len(b.stream)                         # the reference reads the designed sequence, to the stream's end
    print(name, "precision", tr.precision, "bytes per Read: max", max(tr.bytes_per_symbol), "rANS bytes", tr.size_rans, "form", tr.init_form)
    check_expectations(c, b.seq, tr)
    # the oracle: the input array, the same symbols
    ref = oracle.decode(b.stream)
    g = ref.attributes[-1]
    assert g.pred_method == -2 and g.values.dtype == np.int32 and np.array_equal(g.values, S.expected_entries(c))
    assert [int(s) for s in g.symbols.ravel()] == b.seq
    # the reference's encoder writes the coder's bytes
    coded = tr.tags if c.scheme == 0 else syms
    assert ransref.rans_encode(coded, tr.freq, tr.cum, tr.precision) == b.stream[tr.off_rans:tr.off_rans + tr.size_rans]
    # the decoder the case names, by the host parse
    bits = pc.need_bits()
    if c.scheme == 0:
        assert mask == bits["ALL"]                                        # (the host sees no further than a tag stream)
        room = S.rows(c.grid) * c.nc * 4 >= (4 * S.vertices(c.grid) + 15) // 16 * 16 + 40960
        assert (c.decoder == "tags") == (room and tr.num_distinct > 1)    # dsa_kernels.h reg_decode_stream<REG_TAGS>
    elif c.pooled:
        assert mask == bits["ALL"] and (tr.num_symbols + 2) * 4 > S.rows(c.grid) * c.nc * 4
    else:
        assert mask != bits["ALL"] and S.early_field(mask) == S.EARLY[c.decoder], hex(mask)
    assert c.decoder == "tags" or c.scheme == 0 or c.decoder == S.decoder_of(tr.num_symbols, tr.num_distinct, tr.precision, S.rows(c.grid) * c.nc * 4)


def test_both_sides_of_every_switch(reports):
    """Each constant of dsa_needs.h has a named case on either side, the same data where the rule allows it."""
    tr = {n: reports[n][1] for n in NAMES}
    dec = {n: BY_NAME[n].decoder for n in NAMES}
    for edge in (64, 960, 2048, 4032, 4096):
        for used in ("few", "all"):
            a, b = ("switch-%d-symbols-%s" % (ns, used) for ns in (edge, edge + 1))
            assert (tr[a].num_symbols, tr[b].num_symbols) == (edge, edge + 1) and tr[a].precision == tr[b].precision
    assert (dec["switch-64-symbols-all"], dec["switch-65-symbols-all"]) == ("tier0", "wide")
    assert (dec["switch-960-symbols-all"], dec["switch-961-symbols-all"]) == ("tier1", "tier2")
    assert (dec["switch-2048-symbols-all"], dec["switch-2049-symbols-all"]) == ("wide", "tier2")
    assert (dec["switch-4032-symbols-few"], dec["switch-4033-symbols-few"]) == ("tier2", "tier0")          # the compact alphabet begins
    assert (dec["switch-4096-symbols-few-room"], dec["switch-4097-symbols-few-room"]) == ("reg", "tier0")
    assert (dec["switch-4096-symbols-100-room"], dec["switch-4097-symbols-100-room"]) == ("reg", "wide")
    assert (dec["switch-distinct-1"], dec["switch-distinct-2"]) == ("tier0", "reg")
    for a, b, pa, pb, da, db in (("switch-precision-12", "switch-precision-13", 12, 13, "reg", "wide"), ("switch-precision-16", "switch-precision-18", 16, 18, "wide", "tier2")):
        assert S.built(BY_NAME[a]).seq == S.built(BY_NAME[b]).seq and (tr[a].precision, tr[b].precision, dec[a], dec[b]) == (pa, pb, da, db)
    a, b = tr["switch-compact-met"], tr["switch-compact-missed"]
    assert 2 * a.num_distinct + 1 == a.num_symbols + 2 and 2 * b.num_distinct + 1 == b.num_symbols + 3
    assert (dec["switch-compact-met"], dec["switch-compact-missed"]) == ("wide", "tier2")
    a, b = BY_NAME["switch-region-40960"], BY_NAME["switch-region-40928"]
    assert S.built(a).seq == S.built(b).seq and (S.rows(a.grid) * 16, S.rows(b.grid) * 16, a.decoder, b.decoder) == (40960, 40928, "reg", "wide")
    # ... and to within one row: 12-byte rows, 3 414 | 3 413 of them, the smaller mesh's symbols the first of the larger one's
    a, b = BY_NAME["switch-region-40968-x3"], BY_NAME["switch-region-40956-x3"]
    assert (S.rows(a.grid), S.rows(b.grid), a.nc, b.nc, a.decoder, b.decoder) == (3414, 3413, 3, 3, "reg", "wide")
    assert S.rows(b.grid) * 12 < 40960 <= S.rows(a.grid) * 12 and S.built(b).seq[:len(S.built(a).seq)] == S.built(a).seq
    forms = {(reports[n][1].precision, reports[n][1].init_form) for n in NAMES if BY_NAME[n].family == "flush"}
    assert forms == {(12, 0), (12, 1), (12, 2), (18, 0), (18, 1), (18, 2), (18, 3)}


# ------------------------------------------------------------------------------------- the product's source on the host
@pytest.mark.parametrize("family", S.FAMILIES)
def test_general_path_source_decodes_the_input_array(general_exe, tmp_path, family):
    for c in S.family(family):
        for half_lut in (False, True):
            status, detail, got = test_hostcheck.host_decode(general_exe, S.built(c).stream, tmp_path, force=True, half_lut=half_lut)
            assert status == 0, (c.name, detail)
            assert np.array_equal(got[2][-1][2], S.expected_entries(c)), c.name


@pytest.mark.parametrize("family", S.FAMILIES)
def test_lane_kernels_decode_the_input_array(lanes_exe, tmp_path, family):
    taken = 0
    for c in S.family(family):
        status, detail, atts = test_hostcheck_lanes.lanes_decode(lanes_exe, S.built(c).stream, tmp_path)
        if c.pooled and 4 * (S.TOP + 3) > 1 << 20 and max(S.built(c).seq) == S.TOP:
            # the cumulative table of 2^18 symbols is 16 bytes more than the 1 MiB pool of the host program: the walk hands the mesh
            # to the general path (site 170), as the library's does when its 64 MiB are spent
            assert (status, detail) == (2, 170), (c.name, status, detail)
            continue
        assert status == 0, (c.name, detail)
        if atts[-1] is not None:                       # (None: an alphabet beyond the lane tiers)
            taken += 1
            assert np.array_equal(atts[-1], S.expected_entries(c)), c.name
    print(family, "streams the lane kernels took:", taken)


# ------------------------------------------------------------------------------------------------- what the checks catch
@pytest.mark.parametrize("name", ["skew-4095-1-at-64", "thirst-16", "switch-compact-missed", "gaps-4096", "tags-all-x3"])
def test_one_changed_value_or_byte_is_noticed(reports, name):
    c = BY_NAME[name]
    b = S.built(c)
    syms, tr, end, _ = reports[name]
    # one value of the input: the stream no longer carries the designed sequence
    v = b.values.copy()
    v[S.entry_order(c.grid)[70], 0] += 1
    other = S.encode(c, v)
    assert not np.array_equal(oracle.decode(other).attributes[-1].values, S.expected_entries(c))
    got = S.trace_of_stream(other, len(b.seq), c.nc)[0]
    assert got != b.seq and sum(x != y for x, y in zip(got, b.seq)) == 1
    # one byte of the rANS section: other symbols, or a stream nobody reads.  (Not its first byte, which is read last: its low bits
    # can end in the final state, which no decoder looks at.)
    for at in sorted({tr.size_rans // 3 + 1, tr.size_rans // 2, tr.size_rans - 1}):
        d = bytearray(b.stream)
        d[tr.off_rans + at] ^= 0x10
        try:
            changed = S.trace_of_stream(bytes(d), len(b.seq), c.nc)[0] != b.seq
        except (ValueError, IndexError, AssertionError):
            changed = True
        assert changed, at
        try:
            same = np.array_equal(oracle.decode(bytes(d)).attributes[-1].values, S.expected_entries(c))
        except oracle.OracleError:
            same = False
        assert not same, at
