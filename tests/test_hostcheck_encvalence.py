"""The encoder's valence pass (draco-sharp_amd/csrc/dsa_encode_schemes.h: k_enc_val_init, k_enc_valence one lane per mesh,
k_enc_val_split, behind the connectivity walk recording its start faces' times) compiled for the host under AddressSanitizer +
UBSan (tests/hostcheck/encvalence_host.cpp) and held against the host coder's valence_context_symbols on the same faces: the six
context lists of meshes of every shape the generator makes, meshes with topology splits among them, and no access outside a mesh's
arrays.  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import irregular

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encvalence_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encvalence") / "encvalence_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes):
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for nv, faces in meshes:
            faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", nv, len(faces)))
            f.write(faces.tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_context_lists_of_every_shape(exe, tmp_path):
    meshes = []
    for k, kind in enumerate((synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS) * 6):
        nx, ny = 4 + (7 * k) % 29, 4 + (5 * k) % 31
        if kind == synth.HOLES: nx, ny = max(nx, 12), max(ny, 12)
        pos, _, _, faces = synth.make_mesh(kind, nx, ny, 60 + k)
        meshes.append((len(pos), faces))
    meshes.append((3, np.array([[0, 1, 2]])))                                   # one triangle
    meshes.append((4, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])))     # a tetrahedron: closed, interior start face
    fan = np.array([[0, i, i + 1] for i in range(1, 200)] + [[0, 200, 1]])      # a vertex of valence 200
    meshes.append((201, fan))
    meshes.append((152, fan[:150]))                                             # an open fan
    splitting = 0
    for c in irregular.SMALL:                    # flipped, subdivided, thickened, shuffled: every context list, both clamps
        pos, _, _, faces = irregular.mesh(c)
        splitting += c.splits and len(meshes) % 4 != 3          # (the driver codes every fourth mesh with standard symbols)
        meshes.append((len(pos), faces))
    assert splitting >= 4
    out = run(exe, tmp_path, meshes)
    m = re.search(r"(\d+) meshes, (\d+) valence lists alike \((\d+) with topology splits\), (\d+) standard, (\d+) refused alike", out)
    assert m, out
    total, alike, splits, standard, refused = map(int, m.groups())
    assert total == len(meshes) and refused == 0 and alike + standard == total and alike >= 3 * total // 4 - 1
    # tori, holes and two-part meshes split the traversal (the S-symbol fan walks ran): at least the five the grids gave before,
    # and every irregular case with a handle, a hole or a second component
    assert splits >= 5 + splitting


def test_damaged_meshes_fail_alike(exe, tmp_path):
    rng = np.random.default_rng(5)
    meshes = []
    for it in range(80):
        pos, _, _, faces = synth.make_mesh((synth.GRID, synth.TORUS, synth.HOLES)[it % 3], 8 + it % 7, 8 + it % 5, it)
        faces = faces.copy()
        if it % 2:
            faces = np.concatenate([faces, faces[rng.integers(0, len(faces), 2)]])      # duplicated faces
        else:
            faces[rng.integers(0, len(faces))] = faces[rng.integers(0, len(faces))][::-1]   # a flipped copy
        meshes.append((len(pos), faces))
    out = run(exe, tmp_path, meshes)
    assert "%d meshes" % len(meshes) in out
