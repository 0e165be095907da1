"""The host-compilable part of the vertex arrays (draco-sharp_amd/csrc/dsa_vertex_arrays.h: the sizing of the block and the body of
k_vertex_arrays' gather) compiled under AddressSanitizer + UBSan (tests/hostcheck/varrays_host.cpp) and run on meshes decoded by
the oracle, in both formats: every array aligned, inside the reported size and apart from every other; the rows equal to
values[point_map] / portable[point_map]; an attribute quantised with 18 bits absent from the quantized format; a map entry that
points behind the value array gives a row of zeros and no sanitizer report.  A check of the product source on CPU, not a CPU
decode path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import meshutil
import oracle
import vacases
from typedcases import values as typed_values

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "varrays_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("varrays") / "varrays_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def fnv(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.fixture(scope="module")
def decoded():
    """(name, oracle mesh) of every input, decoded once."""
    out = []
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 6, 5, 1)
    out.append(("grid", synth.encode_mesh(pos, faces, nrm, uv)))
    out.append(("holes-seamed", synth.encode_mesh_corners(*meshutil.seamed_mesh(synth, synth.HOLES, 12, 9, 4, "checker", "stripes"))))
    rng = np.random.default_rng(7)
    out.append(("cloud-1", synth.encode_point_cloud(rng.random((1, 3), np.float32))))
    out.append(("cloud-500", synth.encode_point_cloud(rng.random((500, 3), np.float32))))
    for dtype, nc in ((np.uint8, 3), (np.int16, 3)):
        gen = typed_values(dtype, "random", len(pos), nc, seed=3)
        out.append(("%s-x%d" % (np.dtype(dtype).name, nc), synth.encode_mesh(pos, faces, nrm, uv, generic=gen, opt=synth.options(generic_components=nc))))
    out.append(("pos-18-bits", synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(pos_bits=18))))
    out.append(("bad-map", synth.encode_mesh(pos, faces, nrm, uv)))
    meshes = [(name, oracle.decode(s)) for name, s in out]
    bad = meshes[-1][1]                    # the last entry of the shared map points one behind the value arrays
    for a in bad.attributes:
        a.point_map = a.point_map.copy()
        a.point_map[-1] = a.num_entries
    return meshes


def write(path, meshes):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for k, (name, ref) in enumerate(meshes):
            reps = vacases.map_representatives(ref)
            cap_points = ref.num_points + (5 if k % 2 else 0)          # a capacity above the count, as a seamed mesh has
            f.write(struct.pack("<IIIII", ref.num_points, cap_points, ref.num_faces, 1 if ref.encoder_type == 1 else 0, len(ref.attributes)))
            f.write(np.ascontiguousarray(ref.faces, np.int32).tobytes())
            for a, (att, rep) in enumerate(zip(ref.attributes, reps)):
                f.write(bytes([att.att_type, att.data_type, att.num_components, att.seq_type, rep, vacases.quantisation_bits(att), 0, 0]))
                f.write(struct.pack("<I", att.num_entries))
                f.write(att.values.tobytes())
                if att.seq_type != 0:
                    f.write(np.ascontiguousarray(att.portable, np.int32).tobytes())
                if rep == a:
                    f.write(np.ascontiguousarray(att.point_map, np.uint32).tobytes())


def test_layout_and_gather_of_both_formats(exe, tmp_path, decoded):
    path = tmp_path / "meshes.bin"
    write(path, decoded)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "varrays: %d meshes, both formats laid out and gathered" % len(decoded) in r.stdout, r.stdout
    lines = r.stdout.splitlines()
    sizes = {tuple(int(x) for x in ln.replace(":", "").split()[2:5:2]): int(ln.split()[-1]) for ln in lines if ln.startswith("bytes ")}
    assert sizes[(1, 0)] < sizes[(0, 0)] and sizes[(0, 9)] < sizes[(0, 0)] and sizes[(1, 9)] < sizes[(1, 0)]
    for fi, fmt in enumerate(("values", "quantized")):
        for i, (name, ref) in enumerate(decoded):
            head = "mesh %d format %d " % (i, fi)
            got = [ln[len(head):] for ln in lines if ln.startswith(head)]
            assert len(got) == 1 + len(ref.attributes), (name, got)
            if ref.encoder_type == 0:
                assert got[0] == "indices none", (name, got[0])
            else:
                assert got[0] == "indices u16 1 digest %s" % fnv(ref.faces.astype(np.uint16).tobytes()), (name, got[0])
            for a, att in enumerate(ref.attributes):
                rows = vacases.expected_rows(ref, a, fmt)
                if rows is None:
                    assert name == "pos-18-bits" and a == 0 and fmt == "quantized"
                    assert got[1 + a] == "attribute %d absent" % a, (name, got[1 + a])
                    continue
                stride = (rows.shape[1] * rows.itemsize + 3) & ~3 if rows.dtype == np.uint16 and att.seq_type in (2, 3) and fmt == "quantized" else rows.shape[1] * rows.itemsize
                padded = np.zeros((len(rows), stride), np.uint8)
                padded[:, :rows.shape[1] * rows.itemsize] = rows.view(np.uint8).reshape(len(rows), -1)
                data_type = 4 if rows.dtype == np.uint16 and fmt == "quantized" and att.seq_type in (2, 3) else att.data_type
                want = "attribute %d stride %d type %d components %d digest %s" % (a, stride, data_type, rows.shape[1], fnv(padded.tobytes()))
                assert got[1 + a] == want, (name, fmt, got[1 + a], want)
    # the bad map did make a row of zeros
    name, bad = decoded[-1]
    assert name == "bad-map" and not vacases.expected_rows(bad, 0, "values")[-1].any() and vacases.expected_rows(bad, 0, "values")[0].any()
