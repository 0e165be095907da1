"""Symbol streams with designed statistics for the ENCODER's entropy layer (draco-sharp_amd/csrc/dsa_encode.h: the symbol and
histogram part of k_enc_corr, k_enc_plan over dsa_symbol_plan.h, k_enc_rans), shared by test_encode_symbol_designs_cpu.py and
test_gpu_encode_symbol_designs.py.

A case is a sequence of symbols `seq` of `n` entries x `nc` components.  It reaches the encoder as an int32 attribute of a point
cloud: a sequential stream predicts by Difference in row order and entry i is row i, so with c = unzigzag(symbol) the walk
    v[i] = lo + (v[i - 1] - lo + c[i]) mod m,    v[-1] = 0,    lo <= 0 <= lo + m - 1    (per component)
gives values whose corrections are the sequence again, PROVIDED the values reach both lo and lo + m - 1: the bounds of the wrap
transform are then lo and lo + m - 1, max_dif is m, and a correction is brought into min_corr .. max_corr, the m residues.
carry() walks, restates the transform (clamp, min_corr / max_corr for even and odd max_dif, zigzag) in numpy and asserts that it
turns the values back into the sequence.  m is searched from max(seq) + 1 upwards over M_SEARCH values; a case may name its m
(the histogram family: hist_cap of k_enc_corr is m + 2, enc_integer_hist_cap).

The case list:
  * every sequence of symbolcases.CASES that carries, with its scheme and level, its family and its expectations (but for
    `window_edge`, a property of where the decoder's 256-byte windows fall in a mesh's stream);
  * NOT_CARRIED: the sequences whose walk reaches m - 1 for no searched m, each with the reason, replaced by a stand-in that
    keeps the property and spends ballast entries in front to reach the ends (a first entry {1, 0 ...}: component 0 steps to
    m - 1, the others stay at 0);
  * the families of the encode direction, every condition named in `expect` and asserted on the CPU from write_trace(), a plain
    trace of RAnsEncoder.Write made of ransref.rans_encode one symbol at a time (not of k_enc_rans):
      enc-length     rANS section sizes and symbol counts congruent to 0, 1 and 63 modulo 64 (the 64-lane byte register of
                     k_enc_rans: its last store with 0, 1 and 63 bytes held, its last stretch of symbols), and a flush of more
                     than one byte that crosses a multiple of 64; found by searching the number of rare symbols
      enc-divide     frequencies p that are no power of two, a power of two, 1, and 2^precision - 16 at least, at 12, 16 and 20
                     bits: the estimate (state * (0xFFFFFFFF // p + 1)) >> 32 of state / p is one too large at least once and
                     exact at least once in every stream
      enc-flush      the four forms of AnsEncoder.WriteEnd at 16 bits (the 4-byte form needs 15 bits at least: 2^22 is the
                     whole state range at 12), and the one-symbol alphabet, whose section is the single byte 0
      enc-normalise  the three branches of plan::rans_tables, named by normalise(), a restatement of the rounding
                     int(f / total * 2^P + 0.5) with the zero lifted to 1 and of the fix-up loop: the sum exact, short (the
                     top symbol topped up), long by 1, long by many with a sweep that stops at a probability of 1
      enc-choice     symbol_scheme -1 on dyadic statistics (every f / n a power of two: both Shannon sums are integers, and
                     det_log2 of a power of two is exact), tagged_total - raw_total of -1, 0 and +1 found by a search over entry
                     count, components and bit lengths (scheme_totals: Python int), and a largest symbol of bit length 19
      enc-histogram  m of 4095, 4096, 4097 (hist_cap 4097, 4098, 4099: the LDS / global switch of k_enc_corr at 4098), 176 400
                     symbols each, so that many blocks merge into one histogram, one symbol with a count above 65 535; and the
                     same switch at 3 components and 6 000 symbols, which also rides on a position stream of 12 bits
      enc-tagged-bits  entries of bit length 1 .. 29 at 1, 2, 3, 4 components (values within +-2^27: m = 2^28 + 1, lo = -2^27),
                     symbols of 2^18 and above, which are tagged-only: forcing the raw scheme is refused (REFUSED)

PLAN_EMPTY_TOP (dsa_symbol_plan.h) cannot be reached through an attribute.  It needs the symbol sorted last at a probability of
1 or less with an excess left.  A sweep maps p to min(floor(rel p), p - 1), at least 1, which keeps the order of the
probabilities (only the step that ends the loop is cut short), so the symbol sorted last stays the largest: all probabilities are
then 1 and their sum, the number d of distinct symbols, exceeds 2^P.  But choose_scheme gives d symbols a bit length of
bit_length(d) - 2 at least and P = clamp(3 / 2 of it, 12, 20): d > 2^12 has P >= 16, d > 2^16 has P = 20, and d <= 2^18."""
import collections
import itertools

import numpy as np

import ransref
import symbolcases as S
import draco_sharp_amd.synth as synth

Case = collections.namedtuple("Case", "name family n nc scheme level make expect m lo source")

M_SEARCH = 200
POS_BITS = 11           # of the cloud's positions
FREQ1_NAMES = ("thirst-18", "thirst-19", "thirst-20")       # the only cases that need 176 400 symbols, beside enc-histogram's three
RAW_BEYOND = "symbol_scheme 1 (raw) forced on an integer attribute with symbols of 2^18 and above: the device coder writes those tagged only"


# ------------------------------------------------------------------------------------------------------- the carrier
def unzigzag(sym):
    sym = np.asarray(sym, np.int64)
    return np.where(sym & 1, -(sym >> 1) - 1, sym >> 1)


def transform(values, nc):
    """The rule of k_enc_corr for a sequential integer stream, restated: Difference prediction from the row before (0 in front of
    the first), clamped to the bounds of all values; the correction wrapped into min_corr .. max_corr; zigzag."""
    v = np.asarray(values, np.int64).reshape(-1, nc)
    mn, mx = int(v.min()), int(v.max())
    max_dif = 1 + mx - mn
    max_corr = max_dif // 2
    min_corr = -max_corr
    if max_dif % 2 == 0:
        max_corr -= 1
    pred = np.clip(np.vstack([np.zeros((1, nc), np.int64), v[:-1]]), mn, mx)
    cr = v - pred
    cr = np.where(cr < min_corr, cr + max_dif, np.where(cr > max_corr, cr - max_dif, cr))
    return np.where(cr >= 0, cr << 1, ((-(cr + 1)) << 1) | 1).ravel()


def carry(seq, nc, m=None, lo=0):
    """(values int32 (n, nc), m): the walk of `seq` under the first m of max(seq) + 1 ... that reaches both ends (or under the m
    given); None when no searched m does."""
    seq = np.asarray(seq, np.int64)
    steps = np.cumsum(unzigzag(seq).reshape(-1, nc), axis=0)
    first = int(seq.max()) + 1
    for cand in ([m] if m is not None else range(first, first + M_SEARCH)):
        assert cand >= first and lo <= 0 <= lo + cand - 1
        v = lo + (steps - lo) % cand
        if v.min() == lo and v.max() == lo + cand - 1:
            assert np.array_equal(transform(v, nc), seq)
            assert -(1 << 31) <= lo and lo + cand - 1 < 1 << 31
            values = v.astype(np.int32)
            values.setflags(write=False)
            return values, cand
    return None


def positions(n):
    """Any fixed-seed float rows: the cloud's positions."""
    return np.random.default_rng(n).random((n, 3), dtype=np.float32)


Built = collections.namedtuple("Built", "seq values m stream")
_built = {}


def cpu_stream(case, values, scheme=None):
    opt = synth.options(pos_bits=POS_BITS, force_scheme=case.scheme if scheme is None else scheme, compression_level=case.level)
    return synth.encode_point_cloud_attributes(positions(case.n), opt=opt, extra=[synth.Extra(values)])


def built(case):
    """(designed symbols, input array, m, the CPU coder's stream) of a case, made once."""
    if case.name not in _built:
        seq = [int(s) for s in case.make(case)]
        assert len(seq) == case.n * case.nc, (case.name, len(seq))
        got = carry(seq, case.nc, case.m, case.lo)
        assert got is not None, case.name
        _built[case.name] = Built(seq, got[0], got[1], cpu_stream(case, got[0]))
    return _built[case.name]


def attribute_section(data, n):
    """The offset of the scheme byte of the attribute's section by a forward walk of the point-cloud stream: "DRACO", version 2.2,
    type 0, method 0, flags; int32 points; one attributes decoder; its attribute count and {type, data type, components,
    normalized, unique id} of each, a decoder type each; the positions' {method, transform, compressed 1}, their section and the
    two bounds of their wrap transform; the attribute's {method, transform, compressed 1}.  Its section ends 25 bytes before the
    end of the stream: its own wrap bounds (8), then the positions' quantisation (3 minima, range, bits: 17)."""
    assert data[:5] == b"DRACO" and tuple(data[5:9]) == (2, 2, 0, 0)
    assert int.from_bytes(data[11:15], "little") == n and data[15] == 1
    count, at = ransref.varint(data, 16)
    assert count == 2
    for _ in range(count):
        _, at = ransref.varint(data, at + 4)
    at += count
    assert data[at + 2] == 1
    _, at, _ = ransref.parse_section(data, at + 3, 3 * n, 3)
    at += 8
    assert data[at] == 0 and data[at + 1] == 1 and data[at + 2] == 1, data[at:at + 3]       # Difference, wrap, compressed
    return at + 3


# ------------------------------------------------------------------------------------- the trace of RAnsEncoder.Write
WriteTrace = collections.namedtuple("WriteTrace", "size flush_bytes flush_at over exact classes over_classes count")


def divide_class(p, precision):
    out = {"one"} if p == 1 else ({"power-of-two"} if p & (p - 1) == 0 else {"other"})
    if p >= (1 << precision) - 16:
        out.add("near-full")
    return out


def write_trace(coded, freq, cum, precision):
    """RAnsEncoder.Write symbol by symbol (ransref.rans_encode on one symbol, from the state the one before left), then WriteEnd.
    In front of every division the state x (behind the renormalisation bytes) and the frequency p give the multiply-high estimate
    (x * (0xFFFFFFFF // p + 1)) >> 32: `over` counts the Writes where it is the quotient + 1, `exact` where it is the quotient
    (it is never anything else), `classes` / `over_classes` the kinds of p met at all / with an estimate one too large.
    size: bytes of the section; flush_at: bytes written in front of the flush; flush_bytes: 1 .. 4."""
    state = 4 << precision
    size = over = exact = 0
    classes, over_classes = set(), set()
    kinds = {}
    for s in reversed(coded):
        p = freq[s]
        written, after = ransref.rans_encode([s], freq, cum, precision, tail=False, state=state)
        x = state >> (8 * len(written))
        assert x < p << 10 and (len(written) == 0 or x >= p << 2)
        q, est = x // p, (x * (0xFFFFFFFF // p + 1)) >> 32
        assert est in (q, q + 1) and after == (q << precision) + x % p + cum[s]
        if p not in kinds:
            kinds[p] = divide_class(p, precision)
        classes |= kinds[p]
        if est == q:
            exact += 1
        else:
            over += 1
            over_classes |= kinds[p]
        size += len(written)
        state = after
    flush = ransref.rans_encode([], freq, cum, precision, state=state)
    return WriteTrace(size + len(flush), len(flush), size, over, exact, classes, over_classes, len(coded))


def flush_straddles(tr):
    """The flush's bytes lie on both sides of a multiple of 64."""
    return tr.flush_bytes > 1 and tr.flush_at // 64 != (tr.flush_at + tr.flush_bytes - 1) // 64


def block_trace(seq, nc, scheme, level):
    """(ransref Trace, WriteTrace) of the section the CPU coder's symbol coder writes for seq (the searches; the tests trace the
    section of the stream)."""
    blk = synth.encode_symbols(np.asarray(seq, np.uint32), nc, scheme, level)
    syms, end, tr = ransref.parse_section(blk, 0, len(seq), nc)
    assert end == len(blk) and syms == list(seq)
    return tr, write_trace(tr.tags if tr.scheme == 0 else syms, tr.freq, tr.cum, tr.precision)


# ------------------------------------------------------------------------------------------ rans_tables, restated
Normalised = collections.namedtuple("Normalised", "branch excess stops_at_one sweeps prob")


def normalise(counts, precision):
    """plan::rans_tables in Python: probabilities int(f / total * 2^P + 0.5), a zero of a symbol that occurs lifted to 1; the sum
    exact, or short (the symbol sorted last, by probability and stably, gets the rest), or long (sweeps from the largest
    probability down, each scaled by 2^P / sum, until the excess is gone; a sweep stops at a probability of 1)."""
    counts = list(counts)
    while counts and counts[-1] == 0:
        counts.pop()
    total, full = sum(counts), 1 << precision
    prob = []
    for f in counts:
        rp = int(f / total * float(full) + 0.5)
        prob.append(1 if rp == 0 and f > 0 else rp)
    total_prob = sum(prob)
    excess = total_prob - full
    if excess == 0:
        return Normalised("exact", 0, False, 0, prob)
    order = sorted(range(len(prob)), key=lambda i: prob[i])
    if excess < 0:
        prob[order[-1]] -= excess
        return Normalised("short", excess, False, 0, prob)
    error, stops, sweeps = excess, False, 0
    while error > 0:
        sweeps += 1
        rel = float(full) / float(total_prob)
        for j in range(len(order) - 1, -1, -1):
            sid = order[j]
            if prob[sid] <= 1:
                assert j != len(order) - 1                      # PLAN_EMPTY_TOP: out of reach (the module's docstring)
                stops = True
                break
            fix = prob[sid] - int(rel * prob[sid])
            fix = max(fix, 1)
            fix = min(fix, prob[sid] - 1, error)
            prob[sid] -= fix
            total_prob -= fix
            error -= fix
            if total_prob == full:
                break
    return Normalised("long", excess, stops, sweeps, prob)


# ---------------------------------------------------------------------------------------------- choose_scheme, in int
def exact_log2(x):
    assert x > 0 and x & (x - 1) == 0, "%d is no power of two" % x
    return x.bit_length() - 1


def scheme_totals(seq, nc):
    """(tagged_total, raw_total) of plan::choose_scheme for dyadic statistics, in Python int: -sum f log2(f / n) over the tags of
    the entries / over the symbols, approx_table_bits, and the value bits of the tagged scheme."""
    entries = [seq[i:i + nc] for i in range(0, len(seq), nc)]
    tags = [max(1, max(e).bit_length()) for e in entries]

    def shannon(items, n):
        return sum(f * (exact_log2(n) - exact_log2(f)) for f in collections.Counter(items).values())

    def table_bits(max_value, unique):
        d = max_value - unique
        return 8 * unique + 8 * (unique + (d // 64 if d >= 0 else -(-d // 64)))       # C's division truncates

    nu_tag, nu_raw = len(set(tags)), len(set(seq))
    tagged = shannon(tags, len(entries)) + table_bits(nu_tag, nu_tag) + sum(tags) * nc
    raw = shannon(seq, len(seq)) + table_bits(max(seq), nu_raw)
    return tagged, raw


# ------------------------------------------------------------------------------------------------------------ cases
CASES = []
NOT_CARRIED = (
    ("gaps-two-ends", "two used symbols 0 and 2^18 - 1: the steps are 0 and -2^17, the walk visits 0 and the multiples of 2^17 alone"),
    ("tags-all-x2", "symbols of up to 18 bits on 10 240 entries: uniform steps in 2^18 residues do not meet m - 1"),
)
REFUSED = []            # (case, forced scheme, the device encoder's words: the CPU coder would count a histogram of up to 2^28 values)


def case(name, family, n, nc, make, expect, scheme=1, level=5, m=None, lo=0, source=None):
    assert name not in [c.name for c in CASES]
    CASES.append(Case(name, family, n, nc, scheme, level, make, expect, m, lo, source))
    return CASES[-1]


def with_ballast(c, entries):
    """The sequence of symbolcases case c behind `entries` ballast entries: {1, 0 ...} (component 0 steps from 0 to m - 1, the
    others reach 0), then entries of zeros."""
    def make(_):
        seq = list(c.make(c))
        return ([1] + [0] * (c.nc - 1)) + [0] * (c.nc * (entries - 1)) + seq
    return make


for _c in S.CASES:
    _expect = {k: v for k, v in _c.expect.items() if k != "window_edge"}
    _n = S.vertices(_c.grid)
    if _c.name == "gaps-two-ends":
        # one ballast entry {1, 0}: a third symbol, the zero run between 1 and 2^18 - 1 one shorter (still 4 096 run tokens)
        _expect.update(zero_runs=[S.TOP - 2], num_distinct=3)
        case(_c.name + "-ballast", _c.family, _n + 1, _c.nc, with_ballast(_c, 1), _expect, _c.scheme, _c.level, source=_c)
    elif _c.name == "tags-all-x2":
        # 64 ballast entries of tag 1, which the table holds already: the last block stays a whole one
        case(_c.name + "-ballast", _c.family, _n + 64, _c.nc, with_ballast(_c, 64), _expect, _c.scheme, _c.level, source=_c)
    else:
        case(_c.name, _c.family, _n, _c.nc, (lambda c: lambda _: c.make(c))(_c), _expect, _c.scheme, _c.level, source=_c)
CARRIED = [c.name for c in CASES if c.source is not None and c.name == c.source.name]


def anchored(rest, nc=1):
    """[0 ...], [1, 0 ...] in front of `rest`: the first entry stays at 0, the second steps to m - 1, for every m."""
    return [0] * nc + [1] + [0] * (nc - 1) + list(rest)


# ---- enc-length
GEOMETRIC = [(0, 160), (1, 80), (2, 40), (3, 20), (4, 10), (5, 5), (6, 3), (7, 2)]


def with_rare(count, rare, seed):
    """`count` symbols behind the anchor: the geometric mix, `rare` of its symbols 0 replaced by 7."""
    body = [s for s, c in GEOMETRIC for _ in range(c)]
    body = [body[k % len(body)] for k in range(count - 2)]
    zeros = [i for i, s in enumerate(body) if s == 0]
    for i in zeros[:rare]:
        body[i] = 7
    return anchored(S.shuffled(body, seed))


def searched_length(count, wanted):
    """The first number of rare symbols (0 .. 150) for which the trace of the coder's section meets wanted(WriteTrace)."""
    def make(c):
        for rare in range(150):
            seq = with_rare(count, rare, count)
            if wanted(block_trace(seq, c.nc, c.scheme, c.level)[1]) and carry(seq, c.nc) is not None:
                return seq
        raise AssertionError("no length found")
    return make


for _r, _count in ((0, 1024), (1, 1025), (63, 1087)):
    case("length-size-%d-count-%d" % (_r, _r), "enc-length", _count, 1, searched_length(_count, (lambda r: lambda w: w.size % 64 == r)(_r)),
         dict(precision=12, size_mod=_r, count_mod=_r))
case("length-flush-straddles", "enc-length", 1000, 1, searched_length(1000, flush_straddles), dict(precision=12, flush_straddles=True))
case("length-flush-fills-the-register", "enc-length", 1001, 1,
     searched_length(1001, lambda w: w.flush_bytes > 1 and (w.flush_at + w.flush_bytes) % 64 == 0 and not flush_straddles(w)),
     dict(precision=12, size_mod=0, flush_straddles=False))


# ---- enc-divide
def counted(counts, seed):
    return lambda c: anchored(S.dealt(counts, seed))


def one_top_dyadic(n, distinct, each):
    """n = 2^k symbols at a precision of 4 n or 32 n: `each` of every symbol but 0, the rest on 0.  The sum of the rounded
    probabilities is exact, so every frequency is its count times 2^P / n: a power of two for the `each`, none for symbol 0."""
    top = n - each * (distinct - 1)
    assert top > each and each & (each - 1) == 0 and top & (top - 1)
    return counted([(0, top - 1), (1, each - 1)] + [(s, each) for s in range(2, distinct)], distinct)


# At 12 bits the state stays below 2^22 and the estimate is one too large only for x p (ceil(2^32 / p) - 2^32 / p) >= 2^32 with
# x mod p = p - 1: p near 2^12 and a state in the upper part of its range, a few times in tens of thousands of symbols.
case("divide-12-near-full", "enc-divide", 30000, 1, lambda c: anchored([0] * 29998),
     dict(precision=12, freq=[4095, 1], divide_classes={"one", "other", "near-full"}))
case("divide-12-power-of-two", "enc-divide", 40960, 1, counted([(0, 40939), (1, 19)], 1),
     dict(precision=12, freq=[4094, 2], divide_classes={"power-of-two", "other", "near-full"}))
case("divide-16", "enc-divide", 16384, 1, one_top_dyadic(16384, 300, 32), dict(precision=16, divide_classes={"other", "power-of-two"}), level=S.level_for(300, 11))
case("divide-20", "enc-divide", 32768, 1, one_top_dyadic(32768, 2100, 8), dict(precision=20, divide_classes={"other", "power-of-two"}), level=S.level_for(2100, 14))


# ---- enc-flush
def many_300(c):
    return anchored([0, 0, 0] + S.dealt([(0, 95)] + [(s, 1) for s in range(1, 300)], 16))


def searched_flush(base, options, flush_bytes):
    """base with the three symbols behind the anchor replaced by the first triple of `options` for which the coder's section ends
    in a flush of flush_bytes bytes."""
    def make(c):
        seq = list(base(c))
        for a in options:
            for b in options:
                for d in options:
                    seq[2], seq[3], seq[4] = a, b, d
                    if synth.encode_symbols(np.asarray(seq, np.uint32), c.nc, c.scheme, c.level)[-1] >> 6 == flush_bytes - 1:
                        return seq
        raise AssertionError("no flush of %d bytes found" % flush_bytes)
    return make


for _nb in (2, 3, 4):
    case("flush-16-%d-bytes" % _nb, "enc-flush", 399, 1, searched_flush(many_300, range(24), _nb), dict(precision=16, flush_bytes=_nb), level=S.level_for(300, 11))
case("flush-one-symbol", "enc-flush", 300, 2, lambda c: [4, 4] * 300, dict(precision=12, flush_bytes=1, size_rans=1, num_distinct=1), level=7)


# ---- enc-normalise
def searched_normalise(n, distinct, wanted):
    """Counts {n - 2 - rest on symbol 0, a geometric tail} with the first `rest` shape for which normalise() names the wanted
    branch (the precision is 12: fewer than 256 distinct symbols at level 5)."""
    def make(c):
        for k in range(2, 400):
            tail = [(s, 1 + (k * (distinct - s)) // distinct) for s in range(1, distinct)]
            top = n - 2 - sum(f for _, f in tail)
            if top <= 0:
                break
            counts = [top + 1] + [f for _, f in tail]
            counts[1] += 1                                       # (the anchor's 0 and 1)
            if wanted(normalise(counts, 12)):
                return anchored(S.dealt([(0, top)] + tail, k))
        raise AssertionError("no counts found")
    return make


case("normalise-exact", "enc-normalise", 2048, 1, counted([(0, 1022), (1, 511), (2, 256), (3, 128), (4, 64), (5, 32), (6, 16), (7, 8), (8, 4), (9, 2), (10, 1), (11, 2)], 1),
     dict(precision=12, normalise="exact"))
case("normalise-short", "enc-normalise", 3000, 1, searched_normalise(3000, 40, lambda r: r.branch == "short" and r.excess <= -2),
     dict(precision=12, normalise="short"))
case("normalise-long-by-1", "enc-normalise", 3000, 1, searched_normalise(3000, 40, lambda r: r.branch == "long" and r.excess == 1),
     dict(precision=12, normalise="long", long_by=1))
case("normalise-long-by-many", "enc-normalise", 40000, 1, lambda c: anchored(S.dealt([(0, 40000 - 2 - 200)] + [(s, 1) for s in range(1, 201)], 3)),
     dict(precision=12, normalise="long", long_by_at_least=100, sweep_stops_at_one=True), level=7)


# ---- enc-choice
def dyadic(k, nc, classes, top):
    """2^k entries of nc equal components: class (t, a, b) is 2^a entries over 2^b symbols of bit length t (tag t), 2^(a - b)
    entries each; class (1, a, 1) holds the anchor's 0 and 1.  `top`: the largest symbol, of the class with the largest t."""
    def make(c):
        first, body = [], []
        tmax = max(t for t, _, _ in classes)
        for t, a, b in classes:
            lowest = 0 if t == 1 else 1 << (t - 1)
            syms = [lowest + i for i in range(1 << b)]
            if t == tmax:
                syms[-1] = top
            assert len(set(syms)) == len(syms) and all(max(1, s.bit_length()) == t for s in syms), (t, syms)
            mine = [s for s in syms for _ in range(1 << (a - b))]
            if t == 1:
                assert syms == [0, 1]
                mine.remove(0)
                mine.remove(1)
                first = [0, 1]
            body += mine
        assert first and len(first) + len(body) == 1 << k
        return [s for e in first + S.shuffled(body, k) for s in [e] * nc]
    return make


def dyadic_difference(k, nc, classes, top):
    """tagged_total - raw_total of dyadic(...), from the classes alone (the search; scheme_totals recounts it from the sequence)."""
    tag_bits = sum((1 << a) * (k - a) for _, a, _ in classes)
    raw_bits = nc * sum((1 << a) * (k - a + b) for _, a, b in classes)
    total_bl = sum((1 << a) * t for t, a, _ in classes)
    unique = sum(1 << b for _, _, b in classes)
    d = top - unique
    table = 16 * unique + 8 * (d // 64 if d >= 0 else 0)
    return tag_bits + 16 * len(classes) + total_bl * nc - raw_bits - table


def dyadic_splits(k, parts):
    """The ways to write 2^k as `parts` powers of two: exponents in descending order."""
    found = {(k,)}
    for _ in range(parts - 1):
        found = {tuple(sorted(p[:i] + (p[i] - 1, p[i] - 1) + p[i + 1:], reverse=True)) for p in found for i in range(len(p)) if p[i] > 0}
    return sorted(found, reverse=True)


def searched_choice(wanted):
    """The first design (k, nc, classes, top) with tagged_total - raw_total == wanted, in a fixed order: 2^k entries (k 3 .. 8) of
    nc = 1, 2, 4 components, 2 .. 4 classes whose entry counts split 2^k (the anchor's class of bit length 1 the largest), the
    others' bit lengths ascending in 2 .. 18, every number of symbols a class can hold; the largest symbol is solved for (every
    64 symbols between the largest and the number of distinct ones cost the raw table 8 bits)."""
    for k in range(3, 9):
        for nc in (1, 2, 4):
            for j in (2, 3, 4):
                for parts in dyadic_splits(k, j):
                    if parts[0] < 1:
                        continue
                    for ts in itertools.combinations(range(2, 19), j - 1):
                        for bs in itertools.product(*[range(min(a, t - 1) + 1) for t, a in zip(ts, parts[1:])]):
                            classes = [(1, parts[0], 1)] + list(zip(ts, parts[1:], bs))
                            t, b = ts[-1], bs[-1]
                            least = (1 << (t - 1)) + (1 << b) - 1
                            unique = sum(1 << b for _, _, b in classes)
                            rest = dyadic_difference(k, nc, classes, unique) - wanted           # 8 q must make up for it
                            if rest < 0 or rest % 8:
                                continue
                            top = max(least, unique + 64 * (rest // 8))
                            if top < 1 << t and dyadic_difference(k, nc, classes, top) == wanted:
                                return k, nc, classes, top
    raise AssertionError("no design with a difference of %d" % wanted)


CHOICE = {}
for _d in (-1, 0, 1):
    _k, _nc, _classes, _top = searched_choice(_d)
    CHOICE[_d] = (_k, _nc, _classes, _top)
    case("choice-difference-%+d" % _d, "enc-choice", 1 << _k, _nc, dyadic(_k, _nc, _classes, _top), dict(choice=_d, scheme_written=0 if _d < 0 else 1), scheme=-1)
# raw would be cheaper (three symbols, a bit an entry and 4 096 run tokens in the table against 19 value bits for half the entries), but 2^18 is beyond it
case("choice-bit-length-19", "enc-choice", 4096, 1, dyadic(12, 1, [(1, 11, 1), (19, 11, 0)], 1 << 18), dict(choice_raw_cheaper=True, scheme_written=0, max_symbol=1 << 18),
     scheme=-1)


# ---- enc-histogram
def wide_alphabet(m, total, top, nc):
    """Symbol 0 `top` times, the others over 1 .. m - 1 (m - 1 and m - 2, the two ends of the corrections, among them), dealt."""
    def make(c):
        rest = total - 2 * nc - top
        body = [0] * top + [1 + (k * 2654435761) % (m - 1) for k in range(rest - 2)] + [m - 1, m - 2]
        return anchored(S.shuffled(body, m), nc)
    return make


for _m in (4095, 4096, 4097):
    case("histogram-cap-%d" % (_m + 2), "enc-histogram", 44100, 4, wide_alphabet(_m, 176400, 70000, 4),
         dict(precision=16 if _m == 4095 else 18, hist_cap=_m + 2, count_above=65535, top_symbol=_m - 1), m=_m)
for _m in (4096, 4097):
    case("histogram-cap-%d-x3" % (_m + 2), "enc-histogram", 2000, 3, wide_alphabet(_m, 6000, 1500, 3), dict(precision=18, hist_cap=_m + 2, top_symbol=_m - 1), m=_m)


# ---- enc-tagged-bits
TAG_LO, TAG_M = -(1 << 27), (1 << 28) + 1


def all_bit_lengths(nc):
    """Entries of bit length 1 .. 29, 8 rounds of them in a shuffled order, behind an anchor of their own: the first symbol
    2^28 - 1 (a step of -2^27: the walk is at lo), then 1 (a step of -1: at lo + m - 1).  Bit length 29 is the symbol 2^28 alone
    (the correction +2^27 = max_corr of the odd m); the other components hold anything of at most the entry's length."""
    def make(c):
        seq = [(1 << 28) - 1] + [0] * (nc - 1) + [1] + [0] * (nc - 1)
        tags = S.shuffled([1 + k % 29 for k in range(c.n - 2)], nc)
        for e, t in enumerate(tags):
            lead = (e >> 1) & 1 if t == 1 else (1 << 28 if t == 29 else (1 << (t - 1)) | (e * 2654435761 & ((1 << (t - 1)) - 1)))
            seq.append(lead)
            seq += [min(1 << 28, (e * 40503 + k * 977) & ((1 << t) - 1)) for k in range(1, nc)]
        return seq
    return make


for _nc in (1, 2, 3, 4):
    _case = case("tagged-bits-x%d" % _nc, "enc-tagged-bits", 234, _nc, all_bit_lengths(_nc),
                 dict(tags=set(range(1, 30)), max_symbol=1 << 28), scheme=-1 if _nc % 2 else 0, m=TAG_M, lo=TAG_LO)
    if _nc in (1, 4):
        REFUSED.append((_case, 1, RAW_BEYOND))
REFUSED.append(([c for c in CASES if c.name == "choice-bit-length-19"][0], 1, RAW_BEYOND))

ENCODE_FAMILIES = ["enc-length", "enc-divide", "enc-flush", "enc-normalise", "enc-choice", "enc-histogram", "enc-tagged-bits"]
FAMILIES = S.FAMILIES + ENCODE_FAMILIES
assert {c.family for c in CASES} == set(FAMILIES)
BY_NAME = {c.name: c for c in CASES}
WIDE_ALPHABETS = [c.name for c in CASES if c.expect.get("num_symbols", 0) >= 1 << 18]      # k_enc_plan walks them on one lane


def family(name):
    return [c for c in CASES if c.family == name]
