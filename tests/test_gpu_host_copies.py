"""Where a batch's host copies live and where their memory goes: the output block (dsa_batch_download) and the vertex arrays
(dsa_batch_vertex_arrays) of ONE batch pass from the library's pinned mirror to a caller's buffer and back, decode after decode,
with a mesh that answers from the second-chance batch (block 1) read after every step; the context's caches are emptied between
two batches, and a batch is built from the blocks another one just gave back.  Every array is compared with the oracle's."""
import ctypes as C

import pytest

import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native
from test_gpu_download import check_views, streams_mixed
from test_gpu_vertex_arrays import check_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def mixed(seed):
    """test_gpu_download's mixed set and a MultiParallelogram stream, which the fast kernels hand back whatever else they keep."""
    pos, nrm, uv, faces = synth.make_mesh(synth.TWO_PARTS, 12, 9, seed)
    return streams_mixed(seed) + [synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(pos_prediction=2))]


@pytest.fixture(scope="module")
def streams():
    return mixed(5)


def check_blocks(b):
    """The second-chance mesh answers from block 1, every other mesh from block 0."""
    lay = native.MeshOutput()
    retried = [i for i in range(b.n) if b.status(i) == 0 and b.mesh_info(i).decode_path == 2]
    assert retried
    for i in range(b.n):
        assert native.lib().dsa_batch_output_layout(b._h, i, C.byref(lay)) == 0
        assert lay.block == (1 if i in retried else 0), i


def request(fmt, device_only=False):
    return native.VertexRequest({"values": native.DSA_VA_VALUES, "quantized": native.DSA_VA_QUANTIZED}[fmt], native.DSA_VA_DEVICE_ONLY if device_only else 0, 0)


def test_output_copy_changes_owner_on_one_batch(ctx, streams):
    L = native.lib()
    b = dsa.Batch(ctx, streams)
    full, compact = b.output_bytes, b.compact_bytes
    assert 0 < compact < full
    p, q = L.dsa_host_alloc(full), L.dsa_host_alloc(compact)
    assert p and q
    try:
        b.decode(wait=False)                                   # 1. the library's mirror
        b.download()
        mine = L.dsa_batch_host_output(b._h, 0)
        assert mine and mine not in (p, q) and L.dsa_batch_host_output(b._h, 1)
        check_views(b, streams); check_blocks(b)
        b.decode(wait=False)                                   # 2. a caller's buffer of exactly output_bytes
        assert L.dsa_batch_download(b._h, p, full) == 0
        b.wait()
        assert L.dsa_batch_host_output(b._h, 0) == p and L.dsa_batch_host_output(b._h, 1) not in (None, p)
        check_views(b, streams); check_blocks(b)
        b.decode(wait=False)                                   # 3. no buffer: the library's again
        b.download()
        assert L.dsa_batch_host_output(b._h, 0) not in (None, p, q)
        check_views(b, streams); check_blocks(b)
        b.decode(wait=False)                                   # 4. compact, into a caller's buffer of exactly compact_bytes
        assert L.dsa_batch_download_compact(b._h, q, compact) == 0
        b.wait()
        assert L.dsa_batch_host_output(b._h, 0) == q
        check_views(b, streams, compact=True); check_blocks(b)
    finally:
        b.close()
        L.dsa_host_free(p); L.dsa_host_free(q)


def test_vertex_arrays_change_owner_on_one_batch(ctx, streams):
    L = native.lib()
    b = dsa.Batch(ctx, streams)
    nv, nq = b.vertex_arrays_bytes("values"), b.vertex_arrays_bytes("quantized")
    assert 0 < nq < nv
    p, q = L.dsa_host_alloc(nq), L.dsa_host_alloc(nv)
    assert p and q
    try:
        b.decode(wait=False)                                   # 1. values in the library's mirror, beside a download of the same decode
        b.download(wait=False)
        b.vertex_arrays("values", wait=False)
        b.wait()
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) not in (None, p, q) and L.dsa_batch_host_vertex_arrays(b._h, 1)
        check_batch(b, streams, "values"); check_views(b, streams); check_blocks(b)
        b.decode(wait=False)                                   # 2. quantized in a caller's buffer of exactly its size
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(request("quantized")), p, nq) == 0
        b.wait()
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) == p
        check_batch(b, streams, "quantized"); check_blocks(b)
        b.vertex_arrays("values", device_only=True)            # nothing on the host, the device block still right
        assert not L.dsa_batch_host_vertex_arrays(b._h, 0) and not L.dsa_batch_host_vertex_arrays(b._h, 1)
        check_batch(b, streams, "values", device=True)
        b.decode(wait=False)                                   # 3. no buffer: the library's mirror again
        b.vertex_arrays("values")
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) not in (None, p, q)
        check_batch(b, streams, "values"); check_blocks(b)
        b.decode(wait=False)                                   # 4. the other caller's buffer, then the library's on the same decode
        b.download(wait=False, compact=True)
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(request("values")), q, nv) == 0
        b.wait()
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) == q
        check_batch(b, streams, "values"); check_views(b, streams, compact=True); check_blocks(b)
        b.vertex_arrays("quantized")
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) not in (None, p, q)
        check_batch(b, streams, "quantized"); check_views(b, streams, compact=True)
    finally:
        b.close()
        L.dsa_host_free(p); L.dsa_host_free(q)


def test_trim_between_two_batches(ctx, streams):
    L = native.lib()

    def both(b):
        b.decode(wait=False)
        b.download(wait=False)
        b.vertex_arrays("values", wait=False)
        b.wait()
        check_views(b, streams); check_batch(b, streams, "values"); check_blocks(b)

    b = dsa.Batch(ctx, streams)
    both(b)
    b.close()
    ctx.trim()                                                 # the second batch finds every cache empty
    b = dsa.Batch(ctx, streams)
    full, nv = b.output_bytes, b.vertex_arrays_bytes("values")
    p = L.dsa_host_alloc(max(full, nv))
    assert p
    try:
        b.decode(wait=False)
        assert L.dsa_batch_download(b._h, p, full - 1) == native.DSA_ERR_INVALID_ARGUMENT
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(request("values")), p, nv - 1) == native.DSA_ERR_INVALID_ARGUMENT
        assert L.dsa_batch_download(b._h, None, 0) == 0
        assert L.dsa_batch_download(b._h, None, 0) == native.DSA_ERR_INVALID_ARGUMENT      # one is queued already
        assert L.dsa_batch_download_compact(b._h, p, full) == native.DSA_ERR_INVALID_ARGUMENT
        b.vertex_arrays("values", wait=False)
        b.wait()
        assert L.dsa_batch_host_output(b._h, 0) not in (None, p) and L.dsa_batch_host_vertex_arrays(b._h, 0) not in (None, p)
        check_views(b, streams); check_batch(b, streams, "values"); check_blocks(b)
        ctx.trim()                                             # with a batch alive: only what lies idle goes
        both(b)
    finally:
        b.close()
        L.dsa_host_free(p)


def test_a_batch_built_from_blocks_just_given_back(streams):
    """A batch is closed while another is in flight; the next one is made of its arena, mirrors and descriptor zones."""
    L = native.lib()
    c = dsa.Context(0)                                         # a context of its own: its caches hold what this test put there
    other = mixed(18)

    def queue(s):
        b = dsa.Batch(c, s)
        b.decode(wait=False)
        b.download(wait=False)
        b.vertex_arrays("values", wait=False)
        return b

    try:
        b1, b2 = queue(streams), queue(other)
        b1.wait()
        check_views(b1, streams); check_batch(b1, streams, "values")
        assert b1.vertex_arrays_bytes("values") < b1.output_bytes
        mirror = L.dsa_batch_host_output(b1._h, 0)
        b1.close()                                             # b2 is still queued or running
        b3 = queue(streams)
        b2.wait()
        check_views(b2, other); check_batch(b2, other, "values")
        b3.wait()
        # the best fit for b3's output block among the mirrors b1 gave back is the mirror of b1's output block
        assert L.dsa_batch_host_output(b3._h, 0) == mirror
        check_views(b3, streams); check_batch(b3, streams, "values"); check_blocks(b3)
        b2.close(); b3.close()
    finally:
        c.close()
