"""k_symbols_reg maps a 64-position block to its symbols and stores it while the next block decodes, and takes the next 256-byte
window of the stream from a register requested a window earlier (csrc/dsa_kernels.h, reg_decode_stream<REG_ATTR>).  What can go
wrong there sits at the ends: the last block of a stream (full, one position, 63 positions), the drain behind the loop, the first
window of the lowest stream of the arena (nothing may be requested below it), the windows crossed in between at every alignment,
and a stream that runs out of bytes.  A stream reaches the kernel only if its attribute's output region holds the kernel's 40 960
bytes of tables (sym_reg_eligible), so the meshes are GRIDs of 5 - 6 k vertices, positions 11 b, octahedral normals 8 b (positive
corrections: no zig-zag), texture coordinates 10 b, raw symbol streams forced; every mesh is compared with the oracle as
test_gpu_parity does, and through Batch.schedule_needs no mesh may have needed a tier or the wide kernel."""
import functools
import os
import subprocess
import tempfile

import pytest

import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import prunecases as pc
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

OPTS = dict(pos_bits=11, normal_bits=8, uv_bits=10, force_scheme=1)
# (cells in x, cells in y) -> vertices, and what the position stream's length (3 per vertex) leaves in its last block
SHAPES = {"multiple_of_64": (63, 95, 64 * 96, 0), "one_over": (142, 36, 143 * 37, 1), "one_short": (52, 96, 53 * 97, 63)}
OTHER_KERNELS = pc.tiers("early") | pc.tiers("late") | pc.tiers("corner")


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


@functools.lru_cache(None)
def stream(shape, seed):
    nx, ny, _, _ = SHAPES[shape]
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, seed)
    return synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**OPTS))


@functools.lru_cache(None)
def reference(data):
    return oracle.decode(data)


@functools.lru_cache(None)
def seeds32():
    names = sorted(SHAPES)
    return [stream(names[s % 3], 100 + s) for s in range(32)]


def check(b, i, data):
    assert b.status(i) == 0, (i, b.mesh_info(i).detail)
    assert_same(b.result(i), reference(data))
    nd = b.schedule_needs(i)
    assert nd["device"] & OTHER_KERNELS == 0, (i, hex(nd["device"]))      # every stream was k_symbols_reg's


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_mesh_alone_in_its_batch(ctx, shape):
    """The lowest stream of the arena, and the three remainders of the last block."""
    _, _, vertices, rest = SHAPES[shape]
    data = stream(shape, 7)
    ref = reference(data)
    pos, nrm, uv = ref.attributes
    assert pos.num_entries == vertices and (3 * pos.num_entries) % 64 == rest
    assert nrm.num_entries >= 5120 and uv.num_entries >= 5120             # the capacity rule, 2-component floats
    if shape == "multiple_of_64":
        assert (3 * pos.num_entries, 2 * uv.num_entries) == (18432, 12288)
    b = dsa.Batch(ctx, [data])
    b.decode()
    check(b, 0, data)
    b.close()


def test_thirty_two_seeds(ctx):
    """Section sizes and alignments of the rANS sections vary with the seed; every stream crosses dozens of windows."""
    streams = seeds32()
    assert len({len(s) % 4 for s in streams}) > 1
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, s in enumerate(streams):
        check(b, i, s)
    b.close()


def test_crowded_batch(ctx):
    """2 049 meshes: the decoders run beside k_chain, as an early and a late launch."""
    base = seeds32()
    streams = [base[i % 32] for i in range(2049)]
    b = dsa.Batch(ctx, streams)
    b.decode()
    bad = [(i, b.status(i), b.mesh_info(i).detail) for i in range(len(streams)) if b.status(i) != 0]
    assert not bad, bad[:5]
    for i in list(range(0, 2049, 61)) + [2047, 2048]:
        check(b, i, streams[i])
    b.close()


@functools.lru_cache(None)
def rans_sections(data):
    """[(offset, size)] of the rANS section of every attribute, from the host walk's own report."""
    with tempfile.TemporaryDirectory() as d:
        exe, f = os.path.join(d, "needs_host"), os.path.join(d, "s.drc")
        subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe, pc.NEEDS_HOST_SRC], check=True)
        open(f, "wb").write(data)
        w = subprocess.run([exe, "mask", f], capture_output=True, text=True, check=True).stdout.split()
    return [tuple(int(x) for x in a.split(":"))[1:] for a in w[5:]]


def test_streams_cut_inside_a_rans_section(ctx):
    """Four cuts inside each rANS section, between two sound meshes: equal to the oracle or refused, never other values."""
    data = stream("one_over", 7)
    sections = rans_sections(data)
    assert len(sections) == 3 and all(size > 1024 for _, size in sections)
    cuts = [data[:off + at] for off, size in sections for at in (1, size // 3, size - 257, size - 1)]
    streams = [stream("one_short", 8)] + cuts + [stream("multiple_of_64", 9)]
    b = dsa.Batch(ctx, streams)
    b.decode()
    check(b, 0, streams[0])
    check(b, len(streams) - 1, streams[-1])
    verdicts = []
    for i in range(1, len(streams) - 1):
        try:
            ref = oracle.decode(streams[i])
        except oracle.OracleError:
            ref = None
        st = b.status(i)
        verdicts.append((st, b.mesh_info(i).detail if st else 0, ref is not None))
        if ref is None:
            assert st != 0, i
        elif st == 0:
            assert_same(b.result(i), ref)
    print(verdicts)
    b.close()
