"""The designed symbol streams of tests/symbolcases.py through the entropy decoders on the device: k_symbols_reg, k_symbols_wide,
k_tags, the three k_symbols<TIER> with their compact alphabets, the pooled tables -- one batch per family, the whole list on the
general path, and the whole list repeated to 2 049 meshes beside k_chain.  The expected generic attribute is the INPUT array, bit
for bit (integer attributes are lossless, and with prediction method -2 the stream's symbols are zigzag(value)); everything else
of a mesh is held against the oracle.  Batch.schedule_needs and debug array 5 show that the stream was decoded where the case
says.  tests/test_symbol_designs_cpu.py holds every case to the condition it was designed for.

The carriers are early attributes (no prediction).  The late and the corner launch run the same device functions with other
filter flags; parallelogram-predicted carriers, whose symbols cannot be laid out by hand, are not part of this file.  No case is
set aside: there is no allow-list here."""
import numpy as np
import pytest

import oracle
import prunecases as pc
import symbolcases as S
import draco_sharp_amd as dsa
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SRC_TAGGED, SRC_RAW = 0, 1          # csrc/dsa_types.h


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


_refs = {}


def ref_of(c):
    if c.name not in _refs:
        _refs[c.name] = oracle.decode(S.built(c).stream)
    return _refs[c.name]


def check_values(b, i, c, debug=True):
    """Mesh i of batch b is case c: decoded, the generic attribute the input array, the rest the oracle's."""
    info = b.mesh_info(i)
    assert info.status == 0, (c.name, i, info.status, info.detail)
    got = b.result(i)
    g = got.ConnectedData.Attributes[-1]
    want = S.expected_entries(c)
    assert g.Values.dtype == np.int32 and g.Values.shape == want.shape and g.Values.tobytes() == want.tobytes(), (c.name, i)
    assert_same(got, ref_of(c), b if debug else None, i)
    return info


def check_decoder(b, i, c):
    """The kernel that decoded the generic attribute's stream, from the need bits of the finished descriptor and debug array 5."""
    nd = b.schedule_needs(i)
    assert S.early_field(nd["device"]) == S.EARLY[c.decoder], (c.name, hex(nd["device"]))
    assert nd["device"] & ~nd["launched"] == 0
    source, num_symbols, third, size_rans = (int(x) for x in b.debug_array(i, 5, np.uint32, 64).reshape(16, 4)[1])
    seq = S.built(c).seq
    tagged = nd["device"] & pc.need_bits()["TAGS"]
    if c.scheme == 0:
        assert source == SRC_TAGGED and tagged and third == (1 if c.decoder == "tags" else 0), (c.name, third)      # k_tags / the walk
    else:
        assert source == SRC_RAW and num_symbols == max(seq) + 1 and third == c.expect.get("precision", 12) and size_rans >= 1, c.name
        if "size_rans" in c.expect:
            assert size_rans == c.expect["size_rans"]


@pytest.mark.parametrize("family", S.FAMILIES)
def test_family_on_the_fast_kernels(ctx, family):
    cases = S.family(family)
    b = dsa.Batch(ctx, [S.built(c).stream for c in cases])
    b.decode()
    for i, c in enumerate(cases):
        info = check_values(b, i, c)
        assert info.decode_path == 0, (c.name, info.decode_path)
        check_decoder(b, i, c)
    b.close()


def test_every_decoder_is_named_by_some_case():
    assert {c.decoder for c in S.CASES} == {"reg", "wide", "tier0", "tier1", "tier2", "tags", "walk"}
    assert any(c.pooled for c in S.CASES)


def test_whole_list_on_the_general_path(ctx, monkeypatch):
    monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
    b = dsa.Batch(ctx, [S.built(c).stream for c in S.CASES])
    b.decode()
    for i, c in enumerate(S.CASES):
        info = check_values(b, i, c)
        assert info.decode_path != 0, c.name
    b.close()


def test_whole_list_in_a_crowded_batch(ctx):
    """2 049 meshes: the decoders run beside k_chain, and the 2^18-symbol tables of the gaps cases share the batch's pool (a mesh
    that finds it spent is decoded again by the general path: equal values either way)."""
    n = 2049
    cases = [S.CASES[i % len(S.CASES)] for i in range(n)]
    ctx.set_profiling(True)
    try:
        b = dsa.Batch(ctx, [S.built(c).stream for c in cases])
        b.decode()
        kernels = b.kernel_times()
    finally:
        ctx.set_profiling(False)
    assert kernels.get("k_chain", 0) > 0, kernels
    bad = [(cases[i].name, i, b.status(i), b.mesh_info(i).detail) for i in range(n) if b.status(i) != 0]
    assert not bad, bad[:8]
    paths = [b.mesh_info(i).decode_path for i in range(n)]
    print("decode paths:", {p: paths.count(p) for p in sorted(set(paths))})
    fell_back = [(cases[i].name, i, paths[i]) for i in range(n) if paths[i] != 0 and not cases[i].pooled]
    assert not fell_back, fell_back[:8]               # only a mesh whose table comes from the pool may find it spent
    picked = list(range(0, n, 61)) + [n - 2, n - 1]
    assert len({cases[i].name for i in picked}) >= 30
    for i in picked:
        check_values(b, i, cases[i], debug=False)
        if paths[i] == 0:
            check_decoder(b, i, cases[i])
    b.close()
    ctx.trim()
