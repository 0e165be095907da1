"""A plain reference of the entropy layer of a symbol section (TEST INFRASTRUCTURE ONLY): pure Python over int, written from the
reference's RAnsSymbolDecoder.cs (table tokens), RAnsDecoder.cs (ReadInit, Read, BuildLookupTable), SymbolDecoding.cs (raw and
tagged sections), RAnsEncoder.cs / AnsEncoder.cs (Write, WriteEnd) and SURVEY Appendix D -- not from oracle/ and not from the
project's coder, so that the two can be held against it from both sides.

A section is: scheme byte (0 tagged, 1 raw); raw only: max_bit_length; varint symbol count; the frequency tokens (low two bits 3:
a run of zero frequencies of (byte >> 2) + 1 symbols; else that many extra bytes follow, frequency = byte >> 2 | extras << 6, 14);
varint byte count; the rANS bytes, read from their tail; tagged only: the value bits, least significant first.

The rANS precision follows the section's max_bit_length: clamp(3 * mbl / 2, 12, 20) -- mbl 1 .. 8 give 12, 9 gives 13, 10 gives 15,
11 gives 16, 12 gives 18, 13 gives 19, 14 .. 18 give 20.  Precisions 14 and 17 do not exist.  A tag stream has 12 (mbl 5)."""
import collections

IO_BASE = 256

Trace = collections.namedtuple("Trace", "scheme mbl precision num_symbols num_distinct freq cum tokens off_table off_rans size_rans "
                               "init_form bytes_per_symbol tags")


def precision_of(mbl):
    return min(20, max(12, (3 * mbl) // 2))


assert [precision_of(m) for m in range(1, 19)] == [12] * 8 + [13, 15, 16, 18, 19] + [20] * 5


def varint(data, at):
    value, shift = 0, 0
    while True:
        b = data[at]
        at += 1
        value |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return value, at


def read_table(data, at):
    """RAnsSymbolDecoder.Create from the symbol count on: (freq, tokens, end).  tokens: ("run", symbols) / ("freq", extra bytes)."""
    num_symbols, at = varint(data, at)
    freq, tokens = [0] * num_symbols, []
    i = 0
    while i < num_symbols:
        b = data[at]
        at += 1
        token = b & 3
        if token == 3:
            offset = b >> 2
            if i + offset >= num_symbols:
                raise ValueError("zero run past the alphabet")
            tokens.append(("run", offset + 1))
            i += offset
        else:
            prob = b >> 2
            for k in range(token):
                prob |= data[at] << (8 * (k + 1) - 2)
                at += 1
            freq[i] = prob
            tokens.append(("freq", token))
        i += 1
    return freq, tokens, at


def cumulative(freq, precision_bits):
    cum, c = [], 0
    for f in freq:
        cum.append(c)
        c += f
    if c != 1 << precision_bits:
        raise ValueError("frequencies sum to %d, not 2^%d" % (c, precision_bits))
    return cum


def read_init(buf, precision_bits):
    """RAnsDecoder.ReadInit: (state, buffer offset, form 0 .. 3 = bytes of the tail - 1)."""
    size = len(buf)
    if size < 1:
        raise ValueError("empty rANS section")
    form = buf[size - 1] >> 6
    if size < form + 1:
        raise ValueError("rANS section shorter than its tail")
    x = 0
    for k in range(form + 1):
        x |= buf[size - 1 - form + k] << (8 * k)
    x &= (1 << (8 * (form + 1) - 2)) - 1
    l_base = 4 << precision_bits
    state = x + l_base
    if state >= l_base * IO_BASE:
        raise ValueError("invalid state")
    return state, size - 1 - form, form


def rans_decode(buf, freq, cum, precision_bits, count):
    """RAnsDecoder.Read count times: (symbols, init form, bytes taken by each Read)."""
    precision = 1 << precision_bits
    l_base = 4 * precision
    lut = [0] * precision
    for i, f in enumerate(freq):
        if f:
            lut[cum[i]:cum[i] + f] = [i] * f
    state, off, form = read_init(buf, precision_bits)
    out, taken = [], []
    for _ in range(count):
        n = 0
        while state < l_base and off > 0:
            off -= 1
            state = state * IO_BASE + buf[off]
            n += 1
        quo, rem = state // precision, state % precision
        s = lut[rem]
        state = quo * freq[s] + rem - cum[s]
        out.append(s)
        taken.append(n)
    return out, form, taken


def rans_encode(symbols, freq, cum, precision_bits, tail=True, state=None):
    """RAnsEncoder.Write from the last symbol to the first, then AnsEncoder.WriteEnd: the bytes of the section.  tail False: (bytes
    written so far, state) without the end.  state: go on from there."""
    precision = 1 << precision_bits
    l_base = 4 * precision
    state = l_base if state is None else state
    out = bytearray()
    for s in reversed(symbols):
        p = freq[s]
        if p == 0:
            raise ValueError("symbol %d has no frequency" % s)
        limit = l_base // precision * IO_BASE * p
        while state >= limit:
            out.append(state % IO_BASE)
            state //= IO_BASE
        state = (state // p) * precision + state % p + cum[s]
    if not tail:
        return bytes(out), state
    x = state - l_base
    if x < 1 << 6:
        out.append(x)
    elif x < 1 << 14:
        out += (0x4000 + x).to_bytes(2, "little")
    elif x < 1 << 22:
        out += (0x800000 + x).to_bytes(3, "little")
    elif x < 1 << 30:
        out += (0xC0000000 + x).to_bytes(4, "little")
    else:
        raise ValueError("state too large")
    return bytes(out)


def parse_section(data, at, num_values, num_components=1):
    """SymbolDecoding.DecodeSymbols at offset `at`: (symbols, end offset, Trace)."""
    scheme = data[at]
    at += 1
    if scheme == 1:
        mbl = data[at]
        at += 1
        if not 1 <= mbl <= 18:
            raise ValueError("max_bit_length %d" % mbl)
    elif scheme == 0:
        mbl = 5
    else:
        raise ValueError("scheme %d" % scheme)
    precision_bits = precision_of(mbl)
    _, off_table = varint(data, at)
    freq, tokens, at = read_table(data, at)
    if not freq:
        raise ValueError("no symbols")
    cum = cumulative(freq, precision_bits)
    size, at = varint(data, at)
    off_rans = at
    buf = data[at:at + size]
    if len(buf) != size:
        raise ValueError("rANS section past the end")
    at += size
    count = num_values if scheme == 1 else (num_values + num_components - 1) // num_components
    syms, form, taken = rans_decode(buf, freq, cum, precision_bits, count)
    tags = None
    if scheme == 0:
        tags, syms, bit = syms, [], 0
        for t in tags:
            for _ in range(num_components):
                v = 0
                for k in range(t):
                    v |= ((data[at + (bit >> 3)] >> (bit & 7)) & 1) << k
                    bit += 1
                syms.append(v)
        at += (bit + 7) >> 3
    tr = Trace(scheme, mbl, precision_bits, len(freq), sum(1 for f in freq if f), freq, cum, tokens, off_table, off_rans, size, form, taken, tags)
    return syms, at, tr


# ------------------------------------------------------------------------------------------------ what a trace shows
def zero_spans(taken):
    """[(first, length)] of the maximal runs of Reads that took no byte."""
    out, start = [], None
    for i, n in enumerate(taken + [1]):
        if n == 0 and start is None:
            start = i
        elif n != 0 and start is not None:
            out.append((start, i - start))
            start = None
    return out


def offsets_before(trace):
    """The buffer offset (bytes of the rANS section still unread) in front of every Read, and behind the last."""
    off = trace.size_rans - 1 - trace.init_form
    out = [off]
    for n in trace.bytes_per_symbol:
        off -= n
        out.append(off)
    return out


def full_blocks(taken, per_symbol):
    """The 64-symbol blocks (aligned to the stream's start) in which every Read took per_symbol bytes."""
    return [b for b in range(len(taken) // 64) if all(n == per_symbol for n in taken[64 * b:64 * b + 64])]


def zero_runs(freq):
    """Lengths of the interior runs of zero frequencies."""
    out, run = [], 0
    for f in freq:
        if f == 0:
            run += 1
        else:
            if run:
                out.append(run)
            run = 0
    return out
