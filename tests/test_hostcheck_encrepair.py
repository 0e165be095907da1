"""The encoder's topology-repair kernels (draco-sharp_amd/csrc/dsa_encode_repair.h: marks, corners by vertex, per-edge matching, the
break pass and the fan pass one lane per mesh) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/encrepair_host.cpp) and held against the host coder's repair (CornerTable::repair, the literal transcription
of the reference's three passes) on the same faces: every case of tests/defects.py, clean meshes, and 2 000 face soups -- the
same c2v', opposites, parents and counts; then every repaired table through the connectivity kernels of dsa_encode_conn.h as the
library lays it out (opposites given, value rows through k_enc_repair_rows) against the host coder's plan in repair mode -- symbols,
start-face bits, split events, traversal order, value rows, operand entries -- and no access outside a mesh's arrays.  A check of the product source on CPU, not a
CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import defects
import irregular

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encrepair_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encrepair") / "encrepair_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes, counts=False):
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for nv, faces in meshes:
            faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", nv, len(faces)))
            f.write(faces.tobytes())
    r = subprocess.run([exe, str(path)] + (["counts"] if counts else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_named_cases_and_their_counts(exe, tmp_path):
    """The header counts of tests/defects.py::named (points = V' - isolated, faces = F - degenerate) and the number of edges the
    break pass cuts, from the host coder's repair; the kernels give the same tables."""
    cases = defects.named() + defects.placed() + [defects.ALL_DEGENERATE]
    out = run(exe, tmp_path, [(c.nv, c.faces) for c in cases], counts=True)
    assert "%d meshes, %d repaired alike, 0 given up at the step bound, %d walked alike" % (len(cases), len(cases), len(cases) - 1) in out      # (all but the one without a face left)
    lines = [ln for ln in out.splitlines() if ":" in ln and ln.split(":")[0].isdigit()]
    assert len(lines) == len(cases)
    named = {d.name for d in defects.named()}
    for c, ln in zip(cases, lines):
        v2, isolated, degenerate, breaks = [int(x) for x in ln.split(":")[1].split()]
        if c is defects.ALL_DEGENERATE:
            assert degenerate == len(c.faces) and isolated == c.nv and v2 == c.nv
            continue
        assert (v2 - isolated, len(c.faces) - degenerate) == (c.points, c.num_faces), c.name
        if c.name in named:
            assert breaks == defects.BREAKS.get(c.name, 0), (c.name, breaks)


def test_clean_and_damaged_meshes(exe, tmp_path):
    meshes = []
    for k, kind in enumerate((synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS) * 2):
        nx, ny = 4 + (7 * k) % 29, 4 + (5 * k) % 31
        if kind == synth.HOLES: nx, ny = max(nx, 12), max(ny, 12)
        pos, _, _, faces = synth.make_mesh(kind, nx, ny, 40 + k)
        meshes.append((len(pos), faces))
    for c in irregular.SMALL:
        pos, _, _, faces = irregular.mesh(c)
        meshes.append((len(pos), faces))
    for c in defects.injected_small():
        meshes.append((c.nv, c.faces))
    rng = np.random.default_rng(3)
    pos, _, _, faces = synth.make_mesh(synth.GRID, 32, 32, 8)       # 50 defects of every kind in one mesh
    nv, f = len(pos), faces
    for k in range(50):
        nv, f = defects.inject(nv, f, defects.KINDS[k % len(defects.KINDS)], 1, rng)
    meshes.append((nv, f))
    out = run(exe, tmp_path, meshes)
    assert "%d meshes, %d repaired alike, 0 given up at the step bound, %d walked alike" % (len(meshes), len(meshes), len(meshes)) in out


def test_2000_soups(exe, tmp_path):
    soups = defects.soups(2000)
    out = run(exe, tmp_path, [(c.nv, c.faces) for c in soups])
    coded = sum(1 for c in soups if not defects.is_degenerate(c.faces).all())
    assert "2000 meshes, 2000 repaired alike, 0 given up at the step bound, %d walked alike" % coded in out


def test_a_face_listed_thousands_of_times_ends_at_the_bound(exe, tmp_path):
    """One edge faced by 3 000 corners: the replay of that edge is quadratic and the kernel gives the mesh up (ENC_REPAIR_BOUND), it
    does not spin; a copy count the bound allows is repaired like the host coder does."""
    many = np.tile(np.array([[0, 1, 2]], np.uint32), (3000, 1))
    some = np.tile(np.array([[0, 1, 2]], np.uint32), (40, 1))
    out = run(exe, tmp_path, [(3, many), (3, some)])
    assert "2 meshes, 1 repaired alike, 1 given up at the step bound, 1 walked alike" in out
