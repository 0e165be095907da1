"""dsa_batch_decode launches only the kernel groups the host parse found work for (csrc/dsa_needs.h); k_seal has the last word.
Small batches that straddle what the pruning depends on -- the capacity rule of k_symbols_reg, tagged streams, the wide kernel,
GeometricNormal / TexCoordsPortable, corner attributes, linear sequencing, corrupt streams -- decoded with the pruned schedule
and with DSA_PRUNE=0 (everything launched): equal to the oracle bit for bit both ways, the groups a mesh needs launched, the
device's need bits a subset of the host's mask."""
import functools
import subprocess

import numpy as np
import pytest

import oracle
import draco_sharp_amd as dsa
import prunecases as pc
from test_gpu_parity import assert_same, assert_same_attributes

pytestmark = pytest.mark.gpu

B = pc.need_bits()
ALL = B["ALL"]
BATCHES = pc.batches()


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


@functools.lru_cache(None)
def reference(stream):
    return oracle.decode(stream)


def decode(ctx, streams, prune, monkeypatch):
    if prune:
        monkeypatch.delenv("DSA_PRUNE", raising=False)
    else:
        monkeypatch.setenv("DSA_PRUNE", "0")
    b = dsa.Batch(ctx, streams)
    b.decode()
    return b


def same_as_oracle(got, ref):
    """Faces, portable values, point maps, floats bit for bit; a point cloud has no faces (entry i is point i)."""
    if ref.encoder_type == 0:
        assert type(got.ConnectedData) is dsa.PointCloud and got.ConnectedData.PointsCount == ref.num_points
        assert_same_attributes(got.ConnectedData, ref)
    else:
        assert_same(got, ref)


def check_against_oracle_and_masks(b, streams):
    for i, s in enumerate(streams):
        assert b.status(i) == 0, (i, b.mesh_info(i).detail)
        same_as_oracle(b.result(i), reference(s))
        nd = b.schedule_needs(i)
        assert nd["device"] & ~nd["host"] == 0, (i, hex(nd["device"]), hex(nd["host"]))          # the host walk is conservative
        assert nd["device"] & ~nd["launched"] == 0, (i, hex(nd["device"]), hex(nd["launched"]))  # and what a mesh needed was launched
        assert nd["host"] & ~nd["batch"] == 0


# what the pruned decode of each batch must have launched (bits that must be set / must be clear); 2 - 8 meshes: no OS_FLAG
EXPECT = {
    "bench_only": (B["PREDICT_EARLY"], ALL & ~B["PREDICT_EARLY"]),
    "small_last": (ALL, 0),                                                    # the 8 x 8 mesh is tagged: everything
    "small_raw_last": (0, B["TAGS"] | B["GEOMETRIC"] | B["TEXCOORDS"] | pc.tiers("corner")),
    "tagged_last": (ALL, 0),
    "wide_among": (pc.group("WIDE", "late") | B["PREDICT_EARLY"], B["TAGS"] | pc.tiers("early") | pc.group("TIER0", "late") | pc.group("TIER1", "late") | pc.group("TIER2", "late")),
    "stock_last": (B["GEOMETRIC"] | B["TEXCOORDS"] | B["FINALIZE_LATE"] | B["PREDICT_EARLY"], B["TAGS"] | pc.tiers("early") | pc.tiers("late")),
    "seamed_among": (ALL, 0),
    "linear_among": (ALL, 0),
}


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "DSA_PRUNE=0"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batches_equal_the_oracle_with_and_without_pruning(ctx, monkeypatch, name, prune):
    streams = BATCHES[name]
    b = decode(ctx, streams, prune, monkeypatch)
    check_against_oracle_and_masks(b, streams)
    launched = b.schedule_needs(0)["launched"]
    note = b.schedule_note()
    if not prune:
        assert launched == ALL and "every kernel group launched" in note, note
    else:
        must, must_not = EXPECT[name]
        assert launched & must == must and launched & must_not == 0, (name, hex(launched))
        assert launched == b.schedule_needs(0)["batch"]
    if name == "small_raw_last" and prune:
        # the tiers the small mesh needs are launched, and only those launches' groups that have such a stream
        small = b.schedule_needs(len(streams) - 1)
        assert small["device"] & (pc.tiers("early") | pc.tiers("late")) and small["device"] & ~launched == 0
        assert all(b.schedule_needs(i)["device"] & (pc.tiers("early") | pc.tiers("late")) == 0 for i in range(len(streams) - 1))
    b.close()


def test_the_note_names_what_a_bench_batch_leaves_out(ctx, monkeypatch):
    b = decode(ctx, BATCHES["bench_only"], True, monkeypatch)
    note, cnote = b.schedule_note(), ctx.schedule_note()
    for word in ("tags", "early symbols: tier 0 tier 1 tier 2 wide", "late symbols: tier 0 tier 1 tier 2 wide", "GeometricNormal", "TexCoordsPortable",
                 "late k_predict", "late k_finalize"):
        assert word in note, (word, note)
    assert cnote.startswith("k_register_gate") and cnote.endswith(note), cnote
    b.close()


def test_kernel_times_of_a_pruned_decode(ctx, monkeypatch):
    """The event pairs of kernels that were left out are not recorded: kernel_times() reports the others, and a left-out kernel
    reads as absent (0 through .get)."""
    ctx.set_profiling(True)
    try:
        b = decode(ctx, BATCHES["bench_only"], True, monkeypatch)
        times = b.kernel_times()
        stages = b.stage_times()
    finally:
        ctx.set_profiling(False)
    assert times.get("k_tags", 0) == 0 and times.get("k_texcoords", 0) == 0
    assert any(v > 0 for v in times.values()) and all(np.isfinite(v) and v >= 0 for v in stages.values())
    b.close()


def test_golden_streams_under_the_pruned_schedule(ctx, monkeypatch):
    names, streams = zip(*pc.golden_streams())
    for prune in (True, False):
        b = decode(ctx, list(streams), prune, monkeypatch)
        check_against_oracle_and_masks(b, streams)
        b.close()


@functools.lru_cache(None)
def corrupt_copies():
    """Cuts and single flipped bits of an 80 x 80 bench stream inside the attribute header, inside a symbol table and inside a
    symbol stream (offsets from the host walk's own report), between two sound meshes."""
    import os
    import tempfile
    s = pc.bench(1)
    with tempfile.TemporaryDirectory() as d:
        exe, f = os.path.join(d, "needs_host"), os.path.join(d, "s.drc")
        subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe, pc.NEEDS_HOST_SRC], check=True)
        open(f, "wb").write(s)
        w = subprocess.run([exe, "mask", f], capture_output=True, text=True, check=True).stdout.split()
    off_att = int(w[4])
    atts = [tuple(int(x) for x in a.split(":")) for a in w[5:]]
    places = [off_att + 2, off_att + 9]
    for table, rans, size in atts:
        places += [table + 3, (table + rans) // 2, rans + 1, rans + size // 2, rans + size - 1]
    cuts = [s[:p] for p in places]
    flips = [s[:p] + bytes([s[p] ^ (1 << bit)]) + s[p + 1:] for p in places for bit in (0, 7)]
    # two batches: a cut the host sees makes it launch everything, and the flips it cannot see would then never meet the pruned schedule
    return [pc.bench(2)] + cuts + [pc.bench(3)], [pc.bench(2)] + flips + [pc.bench(3)]


@pytest.mark.parametrize("kind", [0, 1], ids=["cuts", "flips"])
def test_corrupt_streams_get_the_verdict_of_the_unpruned_schedule(ctx, monkeypatch, kind):
    streams = corrupt_copies()[kind]
    got = {}
    for prune in (True, False):
        b = decode(ctx, streams, prune, monkeypatch)
        rows = []
        for i in range(len(streams)):
            info = b.mesh_info(i)
            row = [info.status, info.detail if info.status else 0]
            if info.status == 0:
                m = b.result(i).ConnectedData
                row += [m.Faces.tobytes()] + [a.Values.tobytes() for a in m.Attributes] + [a.PointMap.tobytes() for a in m.Attributes]
                nd = b.schedule_needs(i)
                assert nd["device"] & ~nd["host"] == 0 and nd["device"] & ~nd["launched"] == 0
            rows.append(row)
        got[prune] = rows
        b.close()
    assert got[True][0][0] == 0 and got[True][-1][0] == 0
    assert any(r[0] != 0 for r in got[True])
    print(kind, [tuple(r[:2]) for r in got[True]])
    for i, (a, c) in enumerate(zip(got[True], got[False])):
        assert a == c, (i, a[:2], c[:2])
