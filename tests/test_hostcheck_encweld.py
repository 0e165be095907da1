"""The encoder's weld kernels (draco-sharp_amd/csrc/dsa_encode_weld.h: marks, the open-addressing insert with its minimum, the
scan, the maps, the per-vertex test, the gather, under the product's launch sequence enc_weld_launch) compiled for the host under
AddressSanitizer + UBSan (tests/hostcheck/encweld_host.cpp) and held against the host coder's weld (synth::weld_points) on every
case of tests/weldcases.py with 0, 1, 3 and 7 listed attributes welded alone (0: the three key sets of dsa_encode_points_batch and
dsa_weld_batch): the same counts, maps, faces, corner ids and welded rows with the threads run forwards and backwards -- which
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
# the rows of the listed attributes: every width the copy and the comparison branch on (a multiple of 4 bytes or not)
LISTED_DTYPES = [(np.uint8, 4), (np.uint16, 1), (np.uint8, 3), (np.float32, 2), (np.uint8, 1), (np.int32, 4), (np.float32, 3)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encweld") / "encweld_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def listed_of(pos, count, seed=0):
    """`count` per-point arrays over the points `pos`: attribute j is a function of the position alone when j is even (no vertex
    has two of its rows) and also of the point's index when j is odd (every third point of a vertex has a row of its own)."""
    P = len(pos)
    key = np.ascontiguousarray(pos, np.float32).view(np.uint32).reshape(P, -1).astype(np.uint64).sum(axis=1) if P else np.zeros(0, np.uint64)
    out = []
    for j in range(count):
        dtype, nc = LISTED_DTYPES[j % len(LISTED_DTYPES)]
        k = key * np.uint64(2654435761 + 2 * j + seed) >> np.uint64(7)
        if j % 2:
            k = k + (np.arange(P, dtype=np.uint64) % np.uint64(3) == 0) * np.uint64(1 + j)
        cols = np.stack([(k >> np.uint64(3 * c)) & np.uint64(0xFFFF) for c in range(nc)], axis=1) if P else np.zeros((0, nc), np.uint64)
        out.append(np.ascontiguousarray(cols.astype(np.float32) / np.float32(64) if dtype is np.float32 else cols.astype(dtype)))
    return out


def write(path, cases):
    """cases: [(weldcases.Case, [listed arrays])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c, listed in cases:
            P = len(c.pos)
            segs = [np.ascontiguousarray(c.pos, np.float32)]
            if c.generic is not None:
                segs.append(np.ascontiguousarray(c.generic).reshape(P, -1))
            segs += [np.ascontiguousarray(e).reshape(P, -1) for e in c.extra]
            faces = np.ascontiguousarray(c.faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<IIIIII", P, len(faces), int(c.normals is not None), int(c.uvs is not None), len(segs), len(listed)))
            f.write(struct.pack("<%dI" % len(segs), *[s.shape[1] * s.dtype.itemsize for s in segs]))
            f.write(struct.pack("<%dI" % len(listed), *[a.shape[1] * a.dtype.itemsize for a in listed]))
            f.write(faces.tobytes())
            for s in segs:
                f.write(s.tobytes())
            if c.normals is not None:
                f.write(np.ascontiguousarray(c.normals, np.float32).tobytes())
            if c.uvs is not None:
                f.write(np.ascontiguousarray(c.uvs, np.float32).tobytes())
            for a in listed:
                f.write(a.tobytes())


def run(exe, tmp_path, cases, max_grid_y=None):
    path = tmp_path / "meshes.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)] + ([str(max_grid_y)] if max_grid_y else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encweld: %d meshes welded alike, forwards and backwards" % len(cases) in r.stdout


def in_range(c):
    return len(c.faces) == 0 or int(np.asarray(c.faces).max()) < len(c.pos)      # (the host refuses the others before any launch)


def batch(count):
    """One batch: meshes with `count` listed attributes beside meshes with fewer (the grid is sized by the most)."""
    cases = [c for c in weldcases.cases() if in_range(c)]
    assert len(cases) == len(weldcases.cases()) - 1
    return [(c, listed_of(c.pos, count if k % 5 else count // 2, seed=k)) for k, c in enumerate(cases)]


def test_every_case(exe, tmp_path):
    """No listed attribute: the three key sets of dsa_encode_points_batch and dsa_weld_batch."""
    run(exe, tmp_path, batch(0))


@pytest.mark.parametrize("count", [1, 3, 7])
def test_every_case_with_listed_attributes(exe, tmp_path, count):
    run(exe, tmp_path, batch(count))


@pytest.mark.parametrize("per", [2, 1])
def test_every_case_in_slices(exe, tmp_path, per):
    """The batch of count = 3 (6 key sets) with grid y so small that a launch takes `per` meshes: many slices, the last one short
    (the executable holds every mesh against the host coder's weld, as it does unsliced)."""
    cases = batch(3)
    assert len(cases) % 2 == 1 and len(cases) > 4
    run(exe, tmp_path, cases, max_grid_y=6 * per + (5 if per == 2 else 0))


def test_the_listed_attributes_split_and_do_not(exe):
    """What the cases are taken for: an odd attribute gives some vertex two rows, an even one none."""
    import draco_sharp_amd.synth as synth
    c = next(c for c in weldcases.cases() if c.name == "grid/None-stripes")
    arrays = listed_of(c.pos, 4)
    w = synth.weld_points(c.pos, c.faces, c.normals, c.uvs, extra=[synth.Extra(a) for a in arrays], weld_attributes=True)
    assert [x is None for x in w.extra_corners] == [True, False, True, False]
    assert w.num_vertices == len(np.unique(np.ascontiguousarray(c.pos).view(np.uint32).reshape(len(c.pos), -1), axis=0))


def nothing_to_weld():
    """P = 0 with and without attributes, F = 0, every point unused but three, one point named by every corner."""
    z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    none = np.zeros((0, 3), np.uint32)
    p = np.arange(30, dtype=np.float32).reshape(10, 3)
    return [weldcases.Case("P=0", z3, none), weldcases.Case("P=0 with attributes", z3, none, z3, z2),
            weldcases.Case("F=0", p, none, p, p[:, :2].copy()),
            weldcases.Case("three used", p, np.array([[9, 0, 4]], np.uint32), p, p[:, :2].copy()),
            weldcases.Case("one point", p, np.full((5, 3), 7, np.uint32), p, p[:, :2].copy())]


def test_nothing_to_weld(exe, tmp_path):
    """... over the three key sets of dsa_encode_points_batch and dsa_weld_batch."""
    run(exe, tmp_path, [(c, []) for c in nothing_to_weld()])


def test_nothing_to_weld_with_listed_attributes(exe, tmp_path):
    """... with 1, 3 and 7 listed attributes welded alone (none: test_nothing_to_weld)."""
    for count in (1, 3, 7):
        run(exe, tmp_path, [(c, listed_of(c.pos, count)) for c in nothing_to_weld()])
