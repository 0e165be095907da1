"""Symbol streams with designed statistics for the entropy decoders (k_symbols_reg, k_symbols_wide, k_tags, the k_symbols<TIER>
tiers with their compact-alphabet variant, the pooled tables behind them), shared by test_symbol_designs_cpu.py and
test_gpu_symbol_designs.py.

A case is a sequence of symbols.  It reaches a decoder as a generic int32 attribute of 1 - 4 components on a GRID mesh with
positions only, written by the project's CPU coder with prediction method -2 (no_prediction=8: the symbols are zigzag(value)),
the scheme forced, and the compression_level that gives the wanted max_bit_length (plan::choose_scheme: bit length of the distinct
count, -2 / -1 / 0 / +1 / +2 by level).  No stream is patched: every one is what the coder writes from data, and the expected
result is the input array.  The position of a symbol in the stream is the position of its vertex in the traversal, taken from a
first encode of the same mesh (entry_order).

What the coder's rules put out of reach, and what stands in for it (each asserted where it is used):
  * a uniform alphabet of frequency-1 symbols needs 2^P distinct symbols, whose bit length alone puts the precision above P: the
    thirst cases use alphabets in which every symbol but one has frequency 1, the rare ones laid in bursts over whole blocks;
  * a symbol of count c has frequency round(c * 2^P / n), so frequency 1 needs n > 2^P / 1.5 symbols: the 15 / 16-bit cases have
    44 100 symbols, the 18 - 20-bit ones 176 400 (a frequency of at most 3 / 3 / 7 is what a 3-byte refill needs there);
  * at 16 bits the raw scheme needs at least 256 distinct symbols (bit length 9, +2), so the largest frequency the coder can write
    is 65 536 - 255 = 65 281, not the 65 472 of a 65-symbol alphabet; at 15 bits 32 768 - 127; at 13 bits 8 192 - 64 is reached;
  * a block of 64 reads that take 2 bytes each exists at 16 bits only (a frequency-1 symbol leaves a state of 4 .. 1023, two bytes
    below 2^18); at 12 bits such symbols take 2, 1, 2, 1 ..., at 20 bits 3, 2, 3, 2 ...: there the block is one of 64 frequency-1
    (smallest-frequency) symbols, 8 P - 1 .. 8 P + 1 bytes in all when they have frequency 1;
  * ReadInit's 1-byte form needs state - l_base < 64.  A last Write that does not renormalise leaves that only under a largest
    frequency above 2^P - 16 ({4095, 1} at 12 bits, or a one-symbol alphabet, whose section is the single byte 0); one that does
    renormalise has only to land in [4 p, 4 p + 64) for the frequency p of the first symbol, which any p allows: at 18 bits the
    1- and the 2-byte form are searched on a 525-entry mesh (flush_18_renormalised).  The 4-byte form needs a state of 2^22 + l_base, which 12 bits
    cannot have (l_base * 256 = 2^22);
  * the coder (like the reference's) writes bit length 1 for the value 0, so tag 0 does not occur: tag 1 stands in for it and
    "all tags" are 1 .. 18."""
import atexit
import collections
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle
import prunecases as pc
import ransref
import draco_sharp_amd.synth as synth

Case = collections.namedtuple("Case", "name family prop decoder pooled grid nc scheme level make expect")

TOP = (1 << 18) - 1
# (cells in x, cells in y): vertices
REG = (39, 63)            # 2 560: x 4 components x 4 bytes = 40 960, the output region k_symbols_reg asks for
# the output region holds a row per encoded vertex and split symbol (rows()), a few more than the entries.  At 4 components no GRID
# of 2 540 to 2 561 vertices has 2 559 rows: the pair with the same 2 556 entries on both sides is two rows apart.  At 3 components
# (12 bytes a row) 40 960 lies between 3 413 and 3 414 rows, and both exist: that pair holds the switch to within one row.
ROOM = (3, 638)           # 2 556 entries, 2 560 rows x 16 bytes = 40 960
BELOW = (2, 851)          # 2 556 entries, 2 558 rows: 40 928
ROOM3 = (5, 567)          # 3 408 entries, 3 414 rows x 12 bytes = 40 968
BELOW3 = (2, 1136)        # 3 411 entries, 3 413 rows: 40 956 -- more entries in the smaller region
S525 = (20, 24)
ONE_OVER = (14, 228)      # 3 435 x 3 = 10 305 symbols: 1 in the last block
ONE_SHORT = (56, 60)      # 3 477 x 3 = 10 431 symbols: 63 in the last block
FORM0 = (39, 70)          # 2 840 x 4 = 11 360
BIG = (104, 104)          # 11 025 x 4 = 44 100 symbols: frequency 1 at 15 and 16 bits
HUGE = (209, 209)         # 44 100 x 4 = 176 400 symbols: frequency 1 / 3 / 6 at 18 / 19 / 20 bits
SMALL = (19, 15)          # 320
S625 = (24, 24)
S992 = (30, 31)
S2070 = (44, 45)
S4200 = (59, 69)          # x 1 x 4 bytes = 16 800: holds the cumulative table of 4 097 symbols (16 396 bytes)
S17K = (130, 130)         # 17 161 x 1 x 4 bytes: holds the cumulative table of 16 400 symbols
T0, T1, T63 = (53, 63), (6, 502), (4, 690)        # 3 456, 3 521, 3 455 entries: 0 / 1 / 63 in the last block of a tag stream
T3, T2 = (63, 79), (79, 127)                      # 5 120, 10 240: k_tags has room at 3 and at 2 components


def vertices(grid):
    return (grid[0] + 1) * (grid[1] + 1)


def level_for(distinct, mbl):
    """The compression_level at which choose_scheme writes max_bit_length `mbl` for `distinct` distinct symbols."""
    base = distinct.bit_length()
    for level, adj in ((5, -1), (7, 0), (3, -2), (8, 1), (10, 2)):
        if min(18, max(1, base + adj)) == mbl:
            return level
    raise ValueError("%d distinct symbols cannot have max_bit_length %d" % (distinct, mbl))


def shuffled(items, seed):
    """Fisher-Yates with a 64-bit LCG: the same order everywhere."""
    items = list(items)
    x = seed * 6364136223846793005 + 1442695040888963407 & (1 << 64) - 1
    for i in range(len(items) - 1, 0, -1):
        x = x * 6364136223846793005 + 1442695040888963407 & (1 << 64) - 1
        j = (x >> 33) % (i + 1)
        items[i], items[j] = items[j], items[i]
    return items


def dealt(counts, seed):
    out = []
    for s, c in counts:
        out += [s] * c
    return shuffled(out, seed)


# ------------------------------------------------------------------------------------------------------- the carrier
@functools.lru_cache(None)
def mesh(grid):
    pos, _, _, faces = synth.make_mesh(synth.GRID, grid[0], grid[1], 5)
    return pos, faces


_rows = {}


@functools.lru_cache(None)
def entry_order(grid):
    """The input vertex of every entry of the attribute's stream, from a first encode of the mesh with the vertex index as value."""
    pos, faces = mesh(grid)
    probe = np.arange(len(pos), dtype=np.int32).reshape(-1, 1)
    data = synth.encode_mesh(pos, faces, None, None, generic=probe, opt=synth.options(no_prediction=8, generic_components=1))
    ref = oracle.decode(data)
    _rows[grid] = ref.num_vertices
    order = ref.attributes[-1].values[:, 0].astype(np.int64)
    assert len(order) == len(pos) and np.array_equal(np.sort(order), np.arange(len(pos)))
    return order


def rows(grid):
    """Rows of an attribute's output region (dsa_host_parse.h layout_mesh): encoded vertices + split symbols of the mesh."""
    entry_order(grid)
    return _rows[grid]


def values_of(case, seq):
    """The input array (vertices, components) int32 whose stream carries `seq`."""
    v = vertices(case.grid)
    assert len(seq) == v * case.nc and 0 <= min(seq) and max(seq) <= TOP, case.name
    sym = np.asarray(seq, np.int64).reshape(v, case.nc)
    signed = np.where(sym & 1, -(sym >> 1) - 1, sym >> 1).astype(np.int32)
    out = np.zeros((v, case.nc), np.int32)
    out[entry_order(case.grid)] = signed
    out.setflags(write=False)
    return out


def encode(case, values):
    pos, faces = mesh(case.grid)
    return synth.encode_mesh(pos, faces, None, None, generic=values,
                             opt=synth.options(no_prediction=8, force_scheme=case.scheme, compression_level=case.level, generic_components=case.nc))


_built = {}
Built = collections.namedtuple("Built", "seq values stream")


def built(case):
    """(designed symbols, input array, stream) of a case, made once."""
    if case.name not in _built:
        seq = case.make(case)
        values = values_of(case, seq)
        _built[case.name] = Built(seq, values, encode(case, values))
    return _built[case.name]


def expected_entries(case):
    """The decoded attribute in entry order: the input rows in the order of the traversal."""
    return built(case).values[entry_order(case.grid)]


@functools.lru_cache(None)
def _needs_host():
    d = tempfile.mkdtemp(prefix="needs_host")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "needs_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, pc.NEEDS_HOST_SRC], check=True)
    return exe


def host_report(streams):
    """[(mask, off_attributes, [(off_table, off_rans, size_rans)] per attribute)] from the host walk (tests/hostcheck/needs_host.cpp
    mask).  The walk ends at a tagged section (the host sees no further): the mask is then every bit and the attribute's offsets
    are 0."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        names = []
        for k, s in enumerate(streams):
            names.append(os.path.join(d, "%d.drc" % k))
            open(names[-1], "wb").write(s)
        lines = subprocess.run([_needs_host(), "mask"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    for line in lines:
        w = line.split()
        assert w[0] == "0", line
        out.append((int(w[2], 16), int(w[4]), [tuple(int(x) for x in a.split(":")) for a in w[5:]]))
    return out


def section_start(data, off_attributes, num_vertices, sections):
    """The offset of the scheme byte of the generic attribute's section, the last of the stream, by a walk from the start of the
    attribute data (the host walk's off_attributes): the number of attribute decoders and {data id, decoder type, traversal} of
    each; per decoder the attribute count, {type, data type, components, normalized, unique id} of each attribute and a decoder
    type each; then the positions' {method, transform, compressed 1} and their section (raw: table and rANS bytes are stepped over;
    tagged: read, since only the tags say how many value bits follow), the two bounds of their wrap transform, their quantisation
    (3 minima, range, bits: 17 bytes) and the attribute's own {method -2, compressed 1}.  Where the host walk saw the sections
    (raw streams) its offsets confirm the walk."""
    at = off_attributes
    decoders = data[at]
    at += 1 + 3 * decoders
    for _ in range(decoders):
        count, at = ransref.varint(data, at)
        for _ in range(count):
            _, at = ransref.varint(data, at + 4)
        at += count
    assert decoders == 2 and data[at + 2] == 1, (decoders, data[at:at + 3])
    at += 3
    if data[at] == 1:
        _, _, at = ransref.read_table(data, at + 2)
        size, at = ransref.varint(data, at)
        assert sections[0][1:] == (at, size), sections
        at += size
    else:
        _, at, _ = ransref.parse_section(data, at, 3 * num_vertices, 3)
    at += 8 + 17 + 2
    assert data[at - 2] == 0xFE and data[at - 1] == 1 and data[at] in (0, 1), data[at - 2:at + 1]
    if sections[1][0]:
        assert data[at] == 1 and ransref.varint(data, at + 2)[1] == sections[1][0], sections
    return at


EARLY = {"reg": 0, "tier0": 1, "tier1": 2, "tier2": 4, "wide": 8, "tags": 1, "walk": 1}        # NEED_TIER0 .. NEED_WIDE of the early launch


def early_field(mask):
    b = pc.need_bits()
    return (mask >> b["SHIFT_EARLY"]) & 0xF


# ------------------------------------------------------------------------------------------------------------ cases
CASES = []


def case(name, family, prop, decoder, grid, nc, make, expect, scheme=1, level=5, pooled=False):
    assert name not in [c.name for c in CASES]
    CASES.append(Case(name, family, prop, decoder, pooled, grid, nc, scheme, level, make, expect))


def n_of(c):
    return vertices(c.grid) * c.nc


# ---- skew
def two_symbols(at):
    def make(c):
        n = n_of(c)
        seq = [0] * n
        seq[at % n] = 1
        return seq
    return make


for label, grid, nc, at in (("first", REG, 4, 0), ("last", REG, 4, -1), ("at-63", REG, 4, 63), ("at-64", REG, 4, 64), ("at-65", REG, 4, 65),
                            ("last-block-of-1", ONE_OVER, 3, -1), ("last-block-of-63", ONE_SHORT, 3, -1)):
    n = vertices(grid) * nc
    case("skew-4095-1-" + label, "skew", "table {4095, 1}, the rare symbol " + label, "reg", grid, nc, two_symbols(at),
         dict(precision=12, freq=[4095, 1], rare_at=[at % n], last_block=n % 64, silent_span=n // 2))


def one_top(distinct, top=0, burst=0, burst_at=0):
    """`distinct` symbols, all of count 1 but `top`; the rare ones spread evenly, or `burst` of them in a row from burst_at on and
    the others spread evenly behind them."""
    def make(c):
        n = n_of(c)
        rare = shuffled([s for s in range(distinct) if s != top], distinct)
        seq = [top] * n
        if burst:
            rest = len(rare) - burst
            first = burst_at + burst + 64
            at = list(range(burst_at, burst_at + burst)) + [first + (k * (n - first)) // max(rest, 1) for k in range(rest)]
        else:
            at = [(k + 1) * n // distinct - 1 for k in range(len(rare))]
        assert len(at) == len(rare) and len(set(at)) == len(at) and max(at) < n
        for p, s in zip(at, rare):
            seq[p] = s
        return seq
    return make


for bits, mbl, distinct, grid, top in ((13, 9, 65, REG, 0), (15, 10, 128, BIG, 64), (16, 11, 256, BIG, 0)):
    case("skew-wide-%d" % bits, "skew", "%d symbols, all of frequency 1 but one: the largest frequency the coder writes at %d bits" % (distinct, bits), "wide",
         grid, 4, one_top(distinct, top), dict(precision=bits, top_freq=(1 << bits) - distinct + 1, num_symbols=distinct, num_distinct=distinct),
         level=level_for(distinct, mbl))


# ---- silence
SILENCE_TRAIL = 40000


def silence_12_layout(n, t):
    """Rare symbols 1 .. 40 of count 16 and the top symbol 0: a lead of 512 - t rare ones, the top run (1 100 at least), a burst of
    128 rare ones, t more between top ones, 40 000 top ones."""
    rare = shuffled([1 + k % 40 for k in range(640)], 12)
    lead = 512 - t
    after = rare[lead:lead + 128] + [x for pair in zip(rare[lead + 128:], [0] * t) for x in pair] + [0] * SILENCE_TRAIL
    run = n - lead - len(after)
    assert run >= 1100 and len(rare[lead + 128:]) == t
    return rare[:lead] + [0] * run + after, lead, run


def silence_12(c):
    """Frequency 1 of 4096 for a symbol of count 16 among 44 100, 4056 for the top one.  t is searched so that, in one of the silent
    spans of the top run, the next byte is the last of a 256-byte window of the decoder (offset + (off_rans & 3) a multiple of 256):
    first on the reference coder alone (the bytes written for what follows the run), then on the stream itself."""
    n = n_of(c)
    freq = [4056] + [1] * 40
    cum = ransref.cumulative(freq, 12)
    seq, lead, run = silence_12_layout(n, 0)
    mis = trace_of_stream(encode(c, values_of(c, seq)), n, c.nc)[1].off_rans & 3
    trail, state = ransref.rans_encode([0] * SILENCE_TRAIL, freq, cum, 12, tail=False)
    for t in range(0, 300):
        seq, lead, run = silence_12_layout(n, t)
        more, _ = ransref.rans_encode(seq[lead + run:n - SILENCE_TRAIL], freq, cum, 12, tail=False, state=state)
        if -(len(trail) + len(more) + mis) % 256 <= 8 and straddles(c, seq, lead, run):      # (the run itself takes a few bytes)
            return seq
    raise AssertionError("no layout puts a silent span on a window's edge")


def straddles(c, seq, first, length):
    """A span of more than 256 reads without a byte inside seq[first : first + length] whose next byte is the last of a window."""
    data = encode(c, values_of(c, seq))
    tr = trace_of_stream(data, len(seq), c.nc)[1]
    return bool(spans_on_a_window_edge(tr, first, length))


def spans_on_a_window_edge(tr, first=0, length=None):
    """[(first Read, length)] of the spans of more than 256 Reads without a byte (inside [first, first + length)) during which the
    next byte to read is the last of a 256-byte window as k_symbols_reg cuts them: from the rANS section's start rounded down to
    a multiple of 4 (reg_decode_stream; a mesh's stream starts on a multiple of 16 in the arena)."""
    offs = ransref.offsets_before(tr)
    mis = tr.off_rans & 3
    last = len(tr.bytes_per_symbol) if length is None else first + length
    return [(a, k) for a, k in ransref.zero_spans(tr.bytes_per_symbol)
            if k > 256 and first <= a and a + k <= last and offs[a] > 0 and (offs[a] + mis) % 256 == 0]


def trace_of_stream(data, num_values, nc, report=None):
    """(symbols, Trace, end offset) of the generic attribute's section by ransref; report: the stream's entry of host_report."""
    _, off_attributes, sections = report or host_report([data])[0]
    at = section_start(data, off_attributes, num_values // nc, sections)
    syms, end, tr = ransref.parse_section(data, at, num_values, nc)
    return syms, tr, end


case("silence-12-window-edge", "silence", "1 100 top symbols (4056 of 4096) in front of 128 rarest ones; a silent span on the edge of a 256-byte window",
     "reg", BIG, 4, silence_12, dict(precision=12, top_freq=4056, silent_span=257, window_edge=True, top_run=1024, burst=128))
case("silence-12-p-minus-1", "silence", "table {4095, 1}, the rare symbol in the middle: 80 blocks without a byte on either side", "reg", REG, 4,
     two_symbols(5120), dict(precision=12, freq=[4095, 1], silent_span=5000, top_run=5000))
case("silence-13-wide", "silence", "1 152 top symbols (8064 of 8192) in front of 128 frequency-1 symbols", "wide", REG, 4,
     one_top(129, 0, burst=128, burst_at=1152), dict(precision=13, top_freq=8064, silent_span=257, top_run=1024, burst=128), level=level_for(129, 9))


# ---- thirst
def thirst_12(c):
    n = n_of(c)
    rare = shuffled([1 + k % 43 for k in range(129)], 3)
    return [0] * 640 + rare[:128] + [0] * (n - 769) + rare[128:]


case("thirst-12", "thirst", "128 frequency-1 symbols in a row at 12 bits (43 symbols of count 3 among 10 240)", "reg", REG, 4, thirst_12,
     dict(precision=12, top_freq=4053, max_bytes=2, heavy_block=True, burst=128))
for bits, mbl, distinct, grid, dec in ((13, 9, 129, REG, "wide"), (15, 10, 200, BIG, "wide"), (16, 11, 300, BIG, "wide"),
                                       (18, 12, 600, HUGE, "tier1"), (19, 13, 1100, HUGE, "tier2"), (20, 14, 2100, HUGE, "tier2")):
    exp = dict(precision=bits, max_bytes=2 if bits <= 16 else 3, heavy_block=True, burst=128, num_symbols=distinct)
    if bits == 16:
        exp["full_block"] = 2
    case("thirst-%d" % bits, "thirst", "128 smallest-frequency symbols in a row at %d bits, %d distinct" % (bits, distinct), dec, grid, 4,
         one_top(distinct, 0, burst=128, burst_at=6400), exp, level=level_for(distinct, mbl))


case("thirst-20-dense", "thirst", "16 400 distinct symbols among 17 161 at 20 bits (frequency 61: a Read takes 2 bytes at most, 244 <= state), "
     "the cumulative table in the attribute's own region", "tier2", S17K, 1, lambda c: dealt([(0, n_of(c) - 16399)] + [(s, 1) for s in range(1, 16400)], 20),
     dict(precision=20, max_bytes=2, num_symbols=16400, num_distinct=16400, heavy_block=True), level=level_for(16400, 14))


# ---- flush
def searched_form(base, options, form):
    """base with its first three symbols replaced by the first triple of `options` (in order) for which the coder's block ends in
    ReadInit's form `form`."""
    def make(c):
        seq = list(base(c))
        for a in options:
            for b in options:
                for d in options:
                    seq[0], seq[1], seq[2] = a, b, d
                    blk = synth.encode_symbols(np.asarray(seq, np.uint32), c.nc, 1, c.level)
                    if blk[-1] >> 6 == form:
                        return seq
        raise AssertionError("form %d not found" % form)
    return make


def geometric_8(c):
    return [0, 0, 0] + dealt([(0, 157), (1, 80), (2, 40), (3, 20), (4, 10), (5, 5), (6, 3), (7, 2)], 8)


def many_520(c):
    return [0, 0, 0] + dealt([(0, 103)] + [(s, 1) for s in range(1, 520)], 18)


for form in (1, 2):
    case("flush-12-form-%d" % form, "flush", "ReadInit's %d-byte form at 12 bits" % (form + 1), "tier0", SMALL, 1,
         searched_form(geometric_8, range(8), form), dict(precision=12, init_form=form))
case("flush-12-form-0", "flush", "ReadInit's 1-byte form at 12 bits: {4095, 1}, 11 337 top symbols in front of the rare one", "reg", FORM0, 4,
     two_symbols(11337), dict(precision=12, freq=[4095, 1], init_form=0))
case("flush-one-byte", "flush", "a one-symbol alphabet: the rANS section is the single byte 0", "tier0", SMALL, 1,
     lambda c: [5] * n_of(c), dict(precision=12, init_form=0, size_rans=1, num_distinct=1, num_symbols=6), level=7)
for form in (2, 3):
    case("flush-18-form-%d" % form, "flush", "ReadInit's %d-byte form at 18 bits" % (form + 1), "tier1", S625, 1,
         searched_form(many_520, range(16), form), dict(precision=18, init_form=form), level=level_for(520, 12))


def flush_18_renormalised(form):
    """state - l_base < 64 (form 0) or < 2^14 (form 1) behind a last Write that renormalises.  The stream begins {0, d}: the coder
    writes d, then 0 (frequency p, cum 0) last.  In front of that Write the state is q 2^18 + r + cum[d] with r < freq[d]; it is
    1024 p at least (p >= 1024: one shift by 8), and the Write leaves 2^20 + (state >> 8) - 4 p.  So q = 4 p >> 10, and with
    low = (4 p & 1023) << 8 form 0 needs low <= r + cum[d] < low + 2^14, form 1 low + 2^14 <= r + cum[d] (2^18 is less than 2^22 on):
    the first d whose whole interval lies there is taken, from the coder's own table.  What is left is q, the state in front of
    d's Write over freq[d], one value of 4 .. 1023 with probability log(1 + 1 / q) / log 256 -- 1 in 50 with a symbol 0 of 5 in 525
    (q = 9), so the order of the other 523 symbols is shuffled with seed 0, 1, 2 ... until the coder's tail says the form."""
    def make(c):
        n = n_of(c)
        rest = [0] * (n - 521) + list(range(1, 520))
        for d in range(1, 520):
            blk = synth.encode_symbols(np.asarray([0, d] + rest, np.uint32), c.nc, 1, c.level)
            freq, _, _ = ransref.read_table(blk, 2)
            cum = ransref.cumulative(freq, 18)
            low = ((4 * freq[0] & 1023) << 8) + (form << 14)
            if freq[0] >= 1024 and low <= cum[d] and cum[d] + freq[d] <= (low + (1 << 14) if form == 0 else 1 << 18):
                break
        else:
            raise AssertionError("no symbol in the window")
        for seed in range(2000):
            seq = [0, d] + shuffled(rest, seed)
            if synth.encode_symbols(np.asarray(seq, np.uint32), c.nc, 1, c.level)[-1] >> 6 == form:
                return seq
        raise AssertionError("form %d not found" % form)
    return make


for form in (0, 1):
    case("flush-18-form-%d" % form, "flush", "ReadInit's %d-byte form at 18 bits, behind a last Write that renormalises" % (form + 1), "tier1", S525, 1,
         flush_18_renormalised(form), dict(precision=18, init_form=form, num_distinct=520), level=level_for(520, 12))


# ---- switches
def alphabet(largest, used, seed):
    """Symbols 0 .. largest of which `used` occur (0 and largest among them, the others evenly between), dealt evenly."""
    def make(c):
        n = n_of(c)
        ids = sorted({(k * largest) // (used - 1) for k in range(used)}) if used > 1 else [largest]
        assert len(ids) == used and n >= used
        return shuffled([ids[k % used] for k in range(n)], seed)
    return make


def decoder_of(num_symbols, distinct, precision, out_cap):
    """dsa_needs.h by hand, for the names of the switch cases (the test holds them against the host parse's own answer)."""
    if precision == 12 and num_symbols <= 4096 and distinct > 1 and out_cap >= 40960:
        return "reg"
    compact = num_symbols > 4032
    nse = distinct if compact else num_symbols
    if distinct > 1 and 64 < nse <= 2048 and precision <= 16 and (2 * nse + 1 <= num_symbols + 2 if compact else out_cap >= 4 * (nse + 1)):
        return "wide"
    nse = distinct if compact and distinct <= 4032 else num_symbols
    return "tier0" if nse <= 64 else ("tier1" if nse <= 960 else "tier2")


def switch(name, prop, decoder, grid, nc, num_symbols, used, mbl=None, level=None, make=None):
    """The decoder is named here by hand; test_case_holds_its_conditions holds it against decoder_of() on the parsed table and the
    mesh's rows, and against the host parse's own answer."""
    lv = level if level is not None else (level_for(used, mbl) if mbl else 5)
    base = used.bit_length() + {3: -2, 5: -1, 7: 0, 8: 1, 10: 2}[lv]
    precision = ransref.precision_of(min(18, max(1, base)))
    case("switch-" + name, "switches", prop, decoder, grid, nc, make or alphabet(num_symbols - 1, used, num_symbols),
         dict(precision=precision, num_symbols=num_symbols, num_distinct=used), level=lv)


for edge, grid, few, every in ((64, SMALL, ("tier0", "wide"), ("tier0", "wide")), (960, S992, ("wide", "wide"), ("tier1", "tier2")),
                               (2048, S2070, ("wide", "tier2"), ("wide", "tier2")), (4032, S4200, ("tier2", "tier0"), ("tier2", "tier2")),
                               (4096, S4200, ("tier0", "tier0"), ("tier2", "tier2"))):
    for k, ns in enumerate((edge, edge + 1)):
        switch("%d-symbols-few" % ns, "largest symbol + 1 = %d, 3 used" % ns, few[k], grid, 1, ns, 3)
        switch("%d-symbols-all" % ns, "largest symbol + 1 = %d, all used" % ns, every[k], grid, 1, ns, ns, level=10 if edge == 960 else 3)
for ns, few, hundred in ((4096, "reg", "reg"), (4097, "tier0", "wide")):
    switch("%d-symbols-few-room" % ns, "largest symbol + 1 = %d, 3 used, room for k_symbols_reg" % ns, few, REG, 4, ns, 3)
    switch("%d-symbols-100-room" % ns, "largest symbol + 1 = %d, 100 used, room for k_symbols_reg" % ns, hundred, REG, 4, ns, 100, level=3)
switch("distinct-1", "one symbol occurs (frequency 4096)", "tier0", REG, 4, 8, 1)
switch("distinct-2", "two symbols occur", "reg", REG, 4, 8, 2)
switch("precision-12", "200 distinct symbols at max_bit_length 8", "reg", REG, 4, 200, 200, mbl=8)
switch("precision-13", "the same data at max_bit_length 9", "wide", REG, 4, 200, 200, mbl=9)
switch("precision-16", "1 100 distinct symbols at max_bit_length 11", "wide", REG, 4, 1100, 1100, mbl=11)
switch("precision-18", "the same data at max_bit_length 12", "tier2", REG, 4, 1100, 1100, mbl=12)
switch("compact-met", "2048 of 4095 symbols used: 2 nse + 1 = num_symbols + 2", "wide", S4200, 1, 4095, 2048, level=3)
switch("compact-missed", "2048 of 4094 symbols used: 2 nse + 1 = num_symbols + 3", "tier2", S4200, 1, 4094, 2048, level=3)
switch("region-40960", "100 distinct symbols, 2 556 entries x 4, an output region of 40 960 bytes", "reg", ROOM, 4, 100, 100)
switch("region-40928", "the same symbols in a region of 40 928 bytes (no GRID has one of 40 944 at 4 components)", "wide", BELOW, 4, 100, 100)


def region_x3(c):
    """One sequence for both meshes: each carries its first vertices x 3 symbols."""
    return shuffled([k % 100 for k in range(3 * vertices(BELOW3))], 40960)[:n_of(c)]


switch("region-40968-x3", "100 distinct symbols x 3, 3 414 rows: the first region of 12-byte rows that holds 40 960 bytes", "reg", ROOM3, 3, 100, 100, make=region_x3)
switch("region-40956-x3", "the same symbols, 3 413 rows: one row fewer, 4 bytes short", "wide", BELOW3, 3, 100, 100, make=region_x3)


# ---- gaps
def used_symbols(ids, seed):
    def make(c):
        n = n_of(c)
        return shuffled([ids[k % len(ids)] for k in range(n)], seed)
    return make


case("gaps-63-64-65", "gaps", "zero runs of 63, 64 and 65 symbols between used ones", "reg", REG, 4, used_symbols([0, 64, 129, 195, 196], 1),
     dict(precision=12, zero_runs=[63, 64, 65], num_symbols=197, num_distinct=5))
case("gaps-63-64-65-small", "gaps", "the same alphabet without room for k_symbols_reg", "wide", SMALL, 1, used_symbols([0, 64, 129, 195, 196], 2),
     dict(precision=12, zero_runs=[63, 64, 65], num_symbols=197))
case("gaps-4096", "gaps", "a zero run of 4 096 symbols (64 run tokens in a row)", "tier0", REG, 4, used_symbols([0, 4097, 4200], 3),
     dict(precision=12, zero_runs=[4096, 102], num_symbols=4201, run_tokens=64))
case("gaps-100000", "gaps", "zero runs of 100 499 and 161 642 symbols, largest symbol 2^18 - 1", "tier0", REG, 4, used_symbols([0, 100500, TOP], 4),
     dict(precision=12, zero_runs=[100499, TOP - 100501], num_symbols=TOP + 1, run_tokens=1571), pooled=True)
case("gaps-two-ends", "gaps", "two used symbols, 0 and 2^18 - 1", "tier0", SMALL, 2, used_symbols([0, TOP], 5),
     dict(precision=12, zero_runs=[TOP - 1], num_symbols=TOP + 1, num_distinct=2, run_tokens=4096), pooled=True)
case("gaps-wide-compact", "gaps", "100 used symbols among 2^13, runs of 81 and 82", "wide", REG, 4,
     used_symbols([(k * 8191) // 99 for k in range(100)], 6), dict(precision=12, num_symbols=8192, num_distinct=100), level=3)


# ---- tags
def tagged(tags_of_entries):
    """A value of `tag` bits in the first component of every entry (tag 1: 0 or 1), values of up to `tag` bits in the others."""
    def make(c):
        tags = tags_of_entries(vertices(c.grid))
        seq = []
        for e, t in enumerate(tags):
            seq.append((e >> 1) & 1 if t == 1 else (1 << (t - 1)) | (e * 2654435761 & ((1 << (t - 1)) - 1)))
            seq += [(e * 40503 + k) & ((1 << t) - 1) for k in range(1, c.nc)]
        return seq
    return make


def all_tags(v):
    """A skewed table: tag t on about v / 2^t of the entries, at least one (7919 is prime: no entry is named twice), tag 1 on the rest."""
    tags = [1] * v
    at = 0
    for t in range(18, 1, -1):
        for _ in range(max(1, v >> t)):
            tags[(at * 7919 + 3) % v] = t
            at += 1
    return tags


def mostly_one(wide_at):
    return lambda v: [18 if e == wide_at % v else 1 for e in range(v)]


ALL_TAGS = set(range(1, 19))
case("tags-one-tag-x1", "tags", "every entry has tag 7: a one-symbol tag table", "walk", SMALL, 1, tagged(lambda v: [7] * v), dict(tags={7}, num_distinct=1), scheme=0)
case("tags-one-tag-x4", "tags", "every entry has tag 7, room for k_tags (which leaves one-symbol tables to the walk)", "walk", T0, 4, tagged(lambda v: [7] * v),
     dict(tags={7}, num_distinct=1), scheme=0)
case("tags-smallest-beside-18-x4", "tags", "tag 1 beside one 18-bit entry at position 64: table {4095, 1} over two tags", "tags", T0, 4, tagged(mostly_one(64)),
     dict(tags={1, 18}, top_freq=4095, last_block=0), scheme=0)
case("tags-4095-1-last-block-of-1-x4", "tags", "table {4095, 1}, the 18-bit entry alone in the last block", "tags", T1, 4, tagged(mostly_one(-1)),
     dict(tags={1, 18}, top_freq=4095, last_block=1), scheme=0)
case("tags-all-x4-last-block-of-63", "tags", "tags 1 .. 18, skewed table, 63 entries in the last block", "tags", T63, 4, tagged(all_tags), dict(tags=ALL_TAGS, last_block=63), scheme=0)
case("tags-all-x3", "tags", "tags 1 .. 18, 3 components", "tags", T3, 3, tagged(all_tags), dict(tags=ALL_TAGS, last_block=0), scheme=0)
case("tags-all-x2", "tags", "tags 1 .. 18, 2 components", "tags", T2, 2, tagged(all_tags), dict(tags=ALL_TAGS, last_block=0), scheme=0)
case("tags-all-x1", "tags", "tags 1 .. 18, 1 component: the walk decodes the tags", "walk", SMALL, 1, tagged(all_tags), dict(tags=ALL_TAGS), scheme=0)

FAMILIES = ["skew", "silence", "thirst", "flush", "switches", "gaps", "tags"]
assert {c.family for c in CASES} == set(FAMILIES)


def family(name):
    return [c for c in CASES if c.family == name]
