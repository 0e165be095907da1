"""Encode direction, the entropy layer (draco-sharp_amd/csrc/dsa_encode.h: the symbol statistics of k_enc_corr, k_enc_plan over
dsa_symbol_plan.h, k_enc_rans) on the designed symbol streams of tests/encsymbolcases.py.  Every case is an int32 attribute of a
point cloud whose corrections are the designed symbols (test_encode_symbol_designs_cpu.py holds each to its conditions on the
CPU); the device must write the CPU coder's bytes, whoever plans -- the host (DSA_ENC_HOST_PLAN=1), k_enc_plan (0), or the
library's own rule in a call of 300 clouds and more.  The 3-component cases also ride on the position stream (integral floats on
the grid {0, 2^bits - 1}: they quantise to themselves) and on a sequential mesh; the device's streams decode to the input array
on the device; and the raw scheme forced on symbols of 2^18 and above fails alone, beside clouds that succeed."""
import time

import numpy as np
import pytest

import encsymbolcases as E
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def config_of(c, scheme=None, **kw):
    return dsa.Config(position_bits=E.POS_BITS, symbol_scheme=c.scheme if scheme is None else scheme, speed=10 - c.level, **kw)


def cloud_of(c):
    return dsa.PointCloudData(E.positions(c.n), attributes=[dsa.Attribute(E.built(c).values)])


def by_config(cases):
    """{(scheme, level): cases}: a call has one configuration"""
    out = {}
    for c in cases:
        out.setdefault((c.scheme, c.level), []).append(c)
    return out


def set_plan(monkeypatch, host_plan):
    if host_plan is None:
        monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    else:
        monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)


# ------------------------------------------------------------------------------------------ a family at a time
@pytest.mark.parametrize("host_plan", ["0", "1"])
@pytest.mark.parametrize("family", E.FAMILIES)
def test_clouds_match_the_cpu_coder(ctx, monkeypatch, family, host_plan):
    set_plan(monkeypatch, host_plan)
    for _, cases in sorted(by_config(E.family(family)).items()):
        clouds = [cloud_of(c) for c in cases]
        t0 = time.perf_counter()
        got = list(dsa.DracoEncoder(ctx).EncodeBatch(clouds, config_of(cases[0])))
        print("%s host_plan=%s scheme %d level %d: %d clouds, %.1f ms" % (family, host_plan, cases[0].scheme, cases[0].level, len(cases), (time.perf_counter() - t0) * 1e3))
        for c, g in zip(cases, got):
            exp = E.built(c).stream
            assert g == exp, (c.name, len(g), len(exp), first_difference(g, exp))


def first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


# ------------------------------------------------------------------------------------------- one crowded call
CROWD = 300


@pytest.mark.parametrize("config", sorted(by_config(E.CASES)))
def test_a_crowded_call_plans_by_the_librarys_own_rule(ctx, monkeypatch, config):
    """300 clouds and more with no override: the device plans by its own rule (k_enc_plan from 256 meshes on).  The cases of one
    configuration, cycled; the alphabets of 2^18 symbols, which k_enc_plan walks on one lane each, stay out."""
    set_plan(monkeypatch, None)
    cases = [c for c in by_config(E.CASES)[config] if c.name not in E.WIDE_ALPHABETS]
    crowd = [cases[k % len(cases)] for k in range(max(CROWD, len(cases)))]
    shared = {c.name: cloud_of(c) for c in cases}
    t0 = time.perf_counter()
    got = dsa.DracoEncoder(ctx).TryEncodeBatch([shared[c.name] for c in crowd], config_of(cases[0]))
    print("scheme %d level %d: %d clouds of %d cases, %.1f ms" % (config + (len(crowd), len(cases), (time.perf_counter() - t0) * 1e3)))
    assert len(got) == len(crowd)
    for k, (c, g) in enumerate(zip(crowd, got)):
        assert isinstance(g, bytes), (k, c.name, g)                     # every status
    for k in sorted(set(range(0, len(crowd), 7)) | {len(crowd) - 2, len(crowd) - 1}):
        assert got[k] == E.built(crowd[k]).stream, (k, crowd[k].name)


# ---------------------------------------------------------------------------------------------- other carriers
def three_component_cases():
    """the cases of 3 components whose values are integers a float holds: they also are positions"""
    return [c for c in E.CASES if c.nc == 3 and c.lo == 0]


def position_bits_of(m):
    return max(1, (m - 1).bit_length())


def test_three_component_cases_on_the_position_stream(ctx, monkeypatch):
    """kind 0: the values as integral floats on the grid {origin 0, range 2^bits - 1}, bits the smallest with m <= 2^bits, quantise
    to themselves; their corrections are the designed symbols, counted in a histogram of 2^bits + 2 entries (4098 at 12 bits)."""
    cases = three_component_cases()
    bits = {c.name: position_bits_of(E.built(c).m) for c in cases}
    assert 12 in bits.values() and len(cases) >= 5
    for host_plan in ("0", "1"):
        set_plan(monkeypatch, host_plan)
        for c in cases:
            b, nb = E.built(c), bits[c.name]
            assert b.m <= 1 << nb and (nb == 1 or b.m > 1 << (nb - 1))
            pos = b.values.astype(np.float32)
            assert np.array_equal(pos.astype(np.int64), b.values)
            full = float((1 << nb) - 1)
            exp = synth.encode_grid(pos, opt=synth.options(pos_bits=nb, force_scheme=c.scheme, compression_level=c.level), form=0, geometry=0,
                                    pos_grid=synth.grid([0, 0, 0], full))
            got = dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(pos, position_grid=dsa.Grid([0, 0, 0], full))],
                                                    dsa.Config(position_bits=nb, symbol_scheme=c.scheme, speed=10 - c.level))
            assert got[0] == exp, (c.name, nb, host_plan)
            if host_plan == "0":
                assert [int(x) for x in oracle.decode(exp).attributes[0].symbols.ravel()] == b.seq, c.name      # the case's symbols


def test_three_component_cases_on_a_sequential_mesh(ctx, monkeypatch):
    cases = three_component_cases() + E.family("enc-tagged-bits")
    for host_plan in ("0", "1"):
        set_plan(monkeypatch, host_plan)
        for _, group in sorted(by_config(cases).items()):
            meshes, want = [], []
            for c in group:
                pos = E.positions(c.n)
                faces = np.arange(3 * (c.n // 3), dtype=np.uint32).reshape(-1, 3)
                meshes.append(dsa.MeshData(pos, faces, attributes=[dsa.Attribute(E.built(c).values)]))
                want.append(synth.encode_sequential(pos, faces, opt=synth.options(pos_bits=E.POS_BITS, force_scheme=c.scheme, compression_level=c.level),
                                                    extra=[synth.Extra(E.built(c).values)]))
            got = dsa.DracoEncoder(ctx).EncodeBatch(meshes, config_of(group[0], encoding_method=0))
            for c, g, w in zip(group, got, want):
                assert g == w, (c.name, host_plan)


# ------------------------------------------------------------------------------------------------- round trip
def test_device_streams_decode_to_the_input_on_the_device(ctx):
    cases = [E.family(f)[-1] for f in E.FAMILIES]
    streams = []
    for _, group in sorted(by_config(cases).items()):
        streams += list(zip(group, dsa.DracoEncoder(ctx).EncodeBatch([cloud_of(c) for c in group], config_of(group[0]))))
    b = dsa.Batch(ctx, [s for _, s in streams])
    b.decode()
    for i, (c, _) in enumerate(streams):
        assert b.status(i) == 0, (c.name, b.mesh_info(i).detail)
        a = b.result(i).ConnectedData.Attributes[-1]
        values, pmap = np.asarray(a.Values), a.PointMap
        rows = values[np.asarray(pmap, np.int64)] if pmap is not None and len(pmap) else values
        assert rows.dtype == np.int32 and np.array_equal(rows.reshape(c.n, c.nc), E.built(c).values), c.name
    b.close()


# --------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_the_raw_scheme_forced_beyond_2_18_fails_alone(ctx, monkeypatch, host_plan):
    set_plan(monkeypatch, host_plan)
    good = [E.BY_NAME["length-size-1-count-1"], E.BY_NAME["normalise-short"]]
    for bad, scheme, words in E.REFUSED:
        assert (bad.level, scheme) == (good[0].level, good[0].scheme) == (good[1].level, good[1].scheme)
        got = dsa.DracoEncoder(ctx).TryEncodeBatch([cloud_of(good[0]), cloud_of(bad), cloud_of(good[1])], config_of(bad, scheme=scheme))
        assert isinstance(got[1], Exception) and str(got[1]).endswith(words), (bad.name, got[1])
        assert got[0] == E.built(good[0]).stream and got[2] == E.built(good[1]).stream, bad.name
