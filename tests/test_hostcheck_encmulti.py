"""The encoder's level kernels (draco-sharp_amd/csrc/dsa_encode_multi.h: the prediction-degree walk one lane per mesh and its entry
maps, MultiParallelogram / ConstrainedMultiParallelogram one thread per entry, the crease lists) compiled for the host under
AddressSanitizer + UBSan (tests/hostcheck/encmulti_host.cpp) and held against the host coder (prediction_degree_sequence,
write_attribute_values with prediction 2 / 4) on the same faces, values and corner ids -- the same order, symbols and crease
lists or the same refusal, and no access outside a mesh's arrays.  A check of the product source on CPU, not a CPU encode path."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import irregular
import meshutil

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encmulti_host.cpp")
KINDS = (synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS)
LINE = re.compile(r"encmulti: (\d+) meshes, (\d+) orders alike \((\d+) with topology splits\), (\d+) without, (\d+) refused alike, "
                  r"(\d+) streams alike \((\d+) seamed\), crease flags (\d+) (\d+) (\d+) (\d+)")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encmulti") / "encmulti_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes):
    """meshes: (nv, faces, (rows, ids) or None); returns the numbers of the program's summary line"""
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for nv, faces, att in meshes:
            faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", nv, len(faces)))
            f.write(faces.tobytes())
            f.write(struct.pack("<I", att[0] if att is not None else 0))
            if att is not None:
                f.write(np.ascontiguousarray(att[1], np.uint32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = LINE.search(r.stdout)
    assert m, r.stdout
    return [int(x) for x in m.groups()]


def fan(n, closed):
    r = n if closed else n + 1
    return (1 + r, np.array([[0, 1 + i, 1 + (i + 1) % r] for i in range(n)]), None)


def test_topologies_at_thirty_sizes(exe, tmp_path):
    meshes = []
    for k, kind in enumerate(KINDS):
        for s in range(30):
            nx, ny = (12 + s % 6, 12 + s // 6) if kind == synth.HOLES else (3 + s % 7 + k, 3 + s // 4)
            pos, _, _, faces = synth.make_mesh(kind, nx, ny, 100 * k + s)
            meshes.append((len(pos), faces, None))
    n, ordered, _, plain, refused, streams, _, c1, c2, c3, c4 = run(exe, tmp_path, meshes)
    assert n == 150 and refused == 0 and ordered + plain == n and plain == n // 4
    assert streams == 4 * n
    assert min(c1, c2, c3, c4) > 0                      # entries with one, two, three and four parallelograms all occur


def test_tiny_meshes_fans_and_irregular_connectivity(exe, tmp_path):
    meshes = [(3, np.array([[0, 1, 2]]), None), (4, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]), None), fan(200, True), fan(200, False)]
    for c in irregular.SMALL:
        pos, _, _, faces = irregular.mesh(c)
        meshes.append((len(pos), faces, None))
    n, ordered, splits, plain, refused, streams, _, *_ = run(exe, tmp_path, meshes)
    assert n == 4 + len(irregular.SMALL) and refused == 0 and ordered + plain == n
    assert splits >= 4                                  # the handles of tests/irregular.py: topology splits in the connectivity
    assert streams == 4 * n
    # one triangle alone: no entry finds a parallelogram, all four crease lists empty
    assert run(exe, tmp_path, meshes[:1])[-4:] == [0, 0, 0, 0]
    # the tetrahedron: its last vertex closes three faces whose other vertices all precede it -- one entry with three parallelograms,
    # three flags in the third list (in each of the two orders), the other lists empty
    assert run(exe, tmp_path, meshes[1:2])[-4:] == [0, 0, 6, 0]


def test_seamed_attribute_tables(exe, tmp_path):
    meshes = []
    for k, kind in enumerate(KINDS):
        nx, ny = (14, 12) if kind == synth.HOLES else (9 + k, 7 + k)
        for j, pat in enumerate(("stripes", "island", "checker", "single")):
            pos, faces, _, _, uv, uid = meshutil.seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=None, uv_charts=pat)
            meshes.append((len(pos), faces, (len(uv), uid)))
    for k, c in enumerate(irregular.SMALL):
        pos, nrm, uv, faces = irregular.mesh(c)
        _, _, _, _, rows_u, uid = irregular.with_seams(pos, nrm, uv, faces, "none", ("stripes", "checker", "island")[k % 3], seed=k)
        meshes.append((len(pos), faces, (len(rows_u), uid)))
    n, _, _, _, refused, streams, seamed, *_ = run(exe, tmp_path, meshes)
    assert n == len(meshes) and refused == 0
    assert seamed >= n                                   # at least half of the tables have interior seams (two streams each)
    assert streams == 4 * n + seamed


def test_refusals_are_the_host_coders(exe, tmp_path):
    pos, _, _, faces = synth.make_mesh(synth.GRID, 10, 8, 1)
    dup = np.concatenate([faces, faces[:1]])                                       # non-manifold edges
    flip = np.array(synth.make_mesh(synth.TORUS, 8, 6, 2)[3])
    flip[2] = flip[2][::-1]
    meshes = [(len(pos), faces, None), (len(pos), dup, None), (48, flip, None), (len(pos), faces, None)]
    n, ordered, _, plain, refused, *_ = run(exe, tmp_path, meshes)
    assert n == 4 and refused == 2 and ordered + plain == 2
