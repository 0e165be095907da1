"""The device encoder's prediction arithmetic (enc_tex_portable and enc_geo_normal inside k_enc_corr, the parallelogram and
multi-parallelogram corrections) on the designed geometry of tests/predictcases.py, at the designs' own bit depths of up to 20.

Reference: the CPU coder's stream, byte for byte -- the stream whose symbols tests/test_predict_designs_cpu.py holds against a
Python-integer restatement of the arithmetic, so the packed orientation and flip bits are checked through the bytes as well -- and
the numpy pin of the quantised input after a round trip through the device decoder."""
import collections

import pytest

import encodecall
import predictcases as P
import draco_sharp_amd as dsa
import test_gpu_encode_level as LV
import test_gpu_encode_stock as S
from test_gpu_irregular import pin_equal

pytestmark = pytest.mark.gpu

# (entry point, Config keywords, the option set of predictcases whose stream the bytes must equal)
PER_VERTEX = [("ex", dict(texcoord_prediction=5, normal_prediction=6), "stock"),
              ("ex", dict(texcoord_prediction=5, normal_prediction=6, edgebreaker_method=2), "stock-valence"),
              ("level", dict(multi_parallelogram=4), "multi")]
SEAMED = [("corners", dict(texcoord_prediction=5), None),
          ("ex", dict(texcoord_prediction=5, normal_prediction=6), "stock"),
          ("ex", dict(texcoord_prediction=5, normal_prediction=6, edgebreaker_method=2), "stock-valence")]


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def mesh_data(d):
    if d.seams is None:
        return dsa.MeshData(d.pos, d.faces, d.normals, d.uv)
    return S.corner_data(P.corner_arguments(d))


def by_bits(designs):
    """{bits: [designs]}: one encode call per quantisation, which is an option of the call."""
    groups = collections.OrderedDict()
    for d in designs:
        groups.setdefault(d.bits, []).append(d)
    return groups


def encode(ctx, entry, meshes, cfg):
    if entry == "level":
        return LV.encode(ctx, meshes, cfg)
    if entry == "ex":
        return S.encode(ctx, meshes, cfg)
    st, out = encodecall.call(ctx, "dsa_encode_batch_corners", meshes, cfg._native(), messages=False)
    assert st == 0, ctx.error()
    return out


def check(ctx, designs, configs):
    """Every design through every configuration: the CPU coder's bytes; then all streams through the device decoder: the input."""
    streams, pins = [], []
    for bits, group in by_bits(designs).items():
        meshes = [mesh_data(d) for d in group]
        for entry, kw, option_set in configs:
            cfg = dsa.Config(position_bits=bits[0], texcoord_bits=bits[1], normal_bits=bits[2], **kw)
            got = encode(ctx, entry, meshes, cfg)
            for d, m, (st, g) in zip(group, meshes, got):
                assert st == 0, (d.name, entry, kw, st)
                want = (LV.cpu if entry == "level" else S.cpu)(m, cfg)
                if option_set is not None:
                    assert want == P.stream(d, option_set), (d.name, entry, kw)      # the stream the CPU test pinned to the reference
                assert g == want, (d.name, entry, kw, len(g), len(want))
                streams.append(g)
                pins.append(d)
    b = dsa.Batch(ctx, streams)
    try:
        b.decode()
        for i, d in enumerate(pins):
            assert b.status(i) == 0, (i, d.name, b.mesh_info(i).detail)
            pin_equal(b.result(i).ConnectedData, P.pin(d))
    finally:
        b.close()


@S.BOTH_PATHS
def test_per_vertex_designs_match_the_cpu_coder(ctx, monkeypatch, host):
    S.force_path(monkeypatch, host)
    check(ctx, P.PLAIN, PER_VERTEX)


@S.BOTH_PATHS
def test_seamed_designs_match_the_cpu_coder(ctx, monkeypatch, host):
    S.force_path(monkeypatch, host)
    check(ctx, P.SEAMED, SEAMED)
