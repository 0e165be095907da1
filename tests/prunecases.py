"""Streams, batches and need-bit names shared by the tests of the pruned decode schedule (test_needs_cpu.py,
test_gpu_pruned_schedule.py).  The smallest shapes at which pruning can go wrong straddle the capacity rule of sym_reg_eligible
(draco-sharp_amd/csrc/dsa_needs.h: the tables of k_symbols_reg need 40 960 bytes of the attribute's output region): a GRID 80 x 80
mesh has 6 561 vertices, so each of its streams is k_symbols_reg's; a GRID 8 x 8 mesh has every stream in a tier."""
import functools
import json
import os
import re
import struct

import draco_sharp_amd.synth as synth
from meshutil import seamed_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "draco-sharp_amd", "csrc", "dsa_needs.h")
NEEDS_HOST_SRC = os.path.join(HERE, "hostcheck", "needs_host.cpp")       # the host walk as a stand-alone program


@functools.lru_cache(None)
def need_bits():
    """{name: value} of the NEED_* macros of dsa_needs.h (the tier bits as the header has them: unshifted)."""
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define NEED_(\w+) (0x[0-9A-Fa-f]+|\d+)u", text)}


def group(name, which):
    """A tier / wide bit (TIER0, TIER1, TIER2, WIDE) in the field of the early, late or corner symbol launch."""
    b = need_bits()
    return b[name] << b["SHIFT_" + which.upper()]


def tiers(which):
    return sum(group(n, which) for n in ("TIER0", "TIER1", "TIER2", "WIDE"))


@functools.lru_cache(None)
def grid(nx, ny, seed, opts=()):
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, seed)
    return synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**dict(opts)))


def bench(seed):
    """The dialect bench.py decodes (default options: parallelogram positions and texture coordinates, octahedral-delta normals,
    raw 12-bit symbol streams), 80 x 80 cells."""
    return grid(80, 80, seed)


@functools.lru_cache(None)
def seamed():
    return synth.encode_mesh_corners(*seamed_mesh(synth, synth.GRID, 40, 33, 3, None, "stripes"))


@functools.lru_cache(None)
def sequential():
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 40, 33, 2)
    return synth.encode_mesh_sequential(pos, faces, nrm, uv)


@functools.lru_cache(None)
def point_cloud():
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 40, 33, 2)
    return synth.encode_point_cloud(pos)


def golden_streams():
    """The committed streams under tests/golden: the reference's house_04 sample and the dialect vectors."""
    out = [("house_04", open(os.path.join(HERE, "golden", "house_04.obj.drc"), "rb").read())]
    rows = json.load(open(os.path.join(HERE, "golden", "dialect_vectors.json")))
    raw = open(os.path.join(HERE, "golden", "dialect_vectors.bin"), "rb").read()
    at = 0
    for r in rows:
        n, = struct.unpack_from("<I", raw, at)
        out.append((r["name"], raw[at + 4:at + 4 + n]))
        at += 4 + n
    return out


STOCK = (("normal_prediction", 6), ("uv_prediction", 5))


def batches():
    """{name: [stream, ...]}: the batches of the issue's cases 1 - 7 (2 - 8 meshes each), the odd mesh last or in the middle."""
    three = [bench(1), bench(2), bench(3)]
    return {
        "bench_only": three + [bench(4)],
        "small_last": three + [grid(8, 8, 5)],                                       # its streams fall out of k_symbols_reg (and are tagged)
        "small_raw_last": three + [grid(8, 8, 5, (("force_scheme", 1),))],          # the same with raw streams: tiers, no tags
        "tagged_last": three + [grid(80, 80, 6, (("force_scheme", 0),))],
        "wide_among": [bench(1), grid(80, 80, 7, (("pos_bits", 14),)), bench(2)],
        "stock_last": three + [grid(80, 80, 8, STOCK)],
        "seamed_among": [bench(1), seamed(), bench(2)],
        "linear_among": [bench(1), sequential(), point_cloud(), bench(2)],
    }
