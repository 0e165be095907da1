"""The encoder's weld kernels (draco-sharp_amd/csrc/dsa_encode_weld.h: marks, the open-addressing insert with its minimum, the
scan, the maps, the per-vertex test, the gather) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/encweld_host.cpp) and held against the host coder's weld (synth::weld_points) on every case of
tests/weldcases.py: the same counts, maps, faces, corner ids and welded rows with the threads run forwards and backwards -- which
thread wins a slot or a minimum changes no number that leaves the kernels -- and no access outside a mesh's arrays (the arena's
gaps are poisoned).  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import weldcases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encweld_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encweld") / "encweld_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            P = len(c.pos)
            segs = [np.ascontiguousarray(c.pos, np.float32)]
            if c.generic is not None:
                segs.append(np.ascontiguousarray(c.generic).reshape(P, -1))
            segs += [np.ascontiguousarray(e).reshape(P, -1) for e in c.extra]
            faces = np.ascontiguousarray(c.faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<IIIII", P, len(faces), int(c.normals is not None), int(c.uvs is not None), len(segs)))
            f.write(struct.pack("<%dI" % len(segs), *[s.shape[1] * s.dtype.itemsize for s in segs]))
            f.write(faces.tobytes())
            for s in segs:
                f.write(s.tobytes())
            if c.normals is not None:
                f.write(np.ascontiguousarray(c.normals, np.float32).tobytes())
            if c.uvs is not None:
                f.write(np.ascontiguousarray(c.uvs, np.float32).tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "meshes.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encweld: %d meshes welded alike, forwards and backwards" % len(cases) in r.stdout


def in_range(c):
    return len(c.faces) == 0 or int(np.asarray(c.faces).max()) < len(c.pos)      # (the host refuses the others before any launch)


def test_every_case(exe, tmp_path):
    cases = [c for c in weldcases.cases() if in_range(c)]
    assert len(cases) == len(weldcases.cases()) - 1
    run(exe, tmp_path, cases)


def test_nothing_to_weld(exe, tmp_path):
    """P = 0 with and without attributes, F = 0, every point unused but three, one point named by every corner."""
    z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    none = np.zeros((0, 3), np.uint32)
    p = np.arange(30, dtype=np.float32).reshape(10, 3)
    cases = [weldcases.Case("P=0", z3, none), weldcases.Case("P=0 with attributes", z3, none, z3, z2),
             weldcases.Case("F=0", p, none, p, p[:, :2].copy()),
             weldcases.Case("three used", p, np.array([[9, 0, 4]], np.uint32), p, p[:, :2].copy()),
             weldcases.Case("one point", p, np.full((5, 3), 7, np.uint32), p, p[:, :2].copy())]
    run(exe, tmp_path, cases)
