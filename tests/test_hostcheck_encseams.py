"""The encoder's seam kernels (draco-sharp_amd/csrc/dsa_encode_seams.h: seam edges, attribute vertices, the attribute walk one
lane per (mesh, attribute), operand entries, seam bits) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/encseams_host.cpp) and held against the host coder (AttrConn, dfs_sequence, write_stream's seam loop) on the
same faces and corner ids: the synthetic topologies x the chart patterns x UV only / normals only / both -- the same results or
the same refusal, and no access outside a mesh's arrays.  A check of the product source on CPU, not a CPU encode path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import irregular
import meshutil

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encseams_host.cpp")
PATTERNS = ("stripes", "island", "checker", "random", "single", "none")
KINDS = (synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encseams") / "encseams_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes):
    """meshes: (nv, faces, normal (rows, ids) or None, uv (rows, ids) or None)"""
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for nv, faces, nid, uid in meshes:
            faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", nv, len(faces)))
            f.write(faces.tobytes())
            f.write(struct.pack("<I", (1 if nid is not None else 0) | (2 if uid is not None else 0)))
            for a in (nid, uid):
                if a is not None:
                    rows, ids = a
                    f.write(struct.pack("<I", rows))
                    f.write(np.ascontiguousarray(ids, np.uint32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def seamed(kind, nx, ny, seed, normal_charts, uv_charts):
    pos, faces, nrm, nid, uv, uid = meshutil.seamed_mesh(synth, kind, nx, ny, seed, normal_charts=normal_charts, uv_charts=uv_charts)
    return (len(pos), faces, None if nid is None else (len(nrm), nid), None if uid is None else (len(uv), uid))


def irregular_seamed():
    """The small cases of tests/irregular.py (fans of 1 .. 300 corners, ids and faces in no order, handles), two chart patterns each."""
    meshes = []
    for k, c in enumerate(irregular.SMALL):
        pos, nrm, uv, faces = irregular.mesh(c)
        for j in (k, k + 3):
            _, _, rows_n, nid, rows_u, uid = irregular.with_seams(pos, nrm, uv, faces, PATTERNS[(j + 1) % len(PATTERNS)], PATTERNS[j % len(PATTERNS)], seed=j)
            meshes.append((len(pos), faces, (len(rows_n), nid), (len(rows_u), uid)))
    return meshes


def test_irregular_meshes_are_all_coded(exe, tmp_path):
    meshes = irregular_seamed()
    out = run(exe, tmp_path, meshes)
    assert "%d meshes, %d coded alike, 0 refused alike, " % (len(meshes), len(meshes)) in out, out


def test_topologies_by_chart_patterns(exe, tmp_path):
    meshes = []
    for k, kind in enumerate(KINDS):
        nx, ny = (14, 12) if kind == synth.HOLES else (9 + k, 7 + k)
        for j, pat in enumerate(PATTERNS):
            meshes.append(seamed(kind, nx, ny, 10 * k + j, None, pat))          # UV only
            meshes.append(seamed(kind, nx, ny, 10 * k + j, pat, None))          # normals only
            meshes.append(seamed(kind, nx, ny, 10 * k + j, pat, PATTERNS[(j + 2) % len(PATTERNS)]))      # both
    meshes += irregular_seamed()
    assert len(meshes) == 90 + 2 * len(irregular.SMALL)
    out = run(exe, tmp_path, meshes)
    n = len(meshes)
    assert "%d meshes, " % n in out, out
    coded = int(out.split("meshes, ")[1].split(" coded")[0])
    refused = int(out.split("alike, ")[1].split(" refused")[0])
    assert coded + refused == n
    assert coded >= n // 2, out                   # (random charts refuse some meshes: non-manifold attribute fans are the host coder's call too)
    assert int(out.split("refused alike, ")[1].split(" seamed")[0]) > n // 2, out


def test_odd_inputs(exe, tmp_path):
    rng = np.random.default_rng(5)
    meshes = []
    pos, _, _, faces = synth.make_mesh(synth.GRID, 10, 8, 1)
    nv, F = len(pos), len(faces)
    meshes.append((nv, faces, None, (3 * F, np.arange(3 * F).reshape(-1, 3))))           # every corner its own row: all edges cut
    meshes.append((nv, faces, (1, np.zeros((F, 3))), None))                               # one row for all: no seam
    bad = np.array(faces, np.int64)
    bad[3, 1] = nv + 4
    meshes.append((nv, bad, None, (nv, bad % nv)))                                         # face index out of range
    meshes.append((nv, faces, None, (5, rng.integers(0, 9, (F, 3)))))                     # id out of range
    meshes.append((3, np.array([[0, 1, 2]]), (3, np.array([[0, 1, 2]])), (1, np.array([[0, 0, 0]]))))
    fan = np.array([[0, i, i + 1] for i in range(1, 60)] + [[0, 60, 1]])
    meshes.append((61, fan, None, (120, np.array([[i % 7, i, i + 1] for i in range(60)]))))      # a vertex of valence 60 with cuts
    pos, _, _, faces = synth.make_mesh(synth.TORUS, 8, 6, 2)
    flip = np.array(faces)
    flip[2] = flip[2][::-1]
    meshes.append((len(pos), flip, None, (len(pos), flip)))                               # damaged: the connectivity's refusal
    out = run(exe, tmp_path, meshes)
    assert "%d meshes, " % len(meshes) in out, out
