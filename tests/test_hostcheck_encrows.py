"""The two kernels of draco-sharp_amd/csrc/dsa_encode_rows.h (k_enc_entry_rows behind the encoder's attribute stage, k_source_rows
behind a decode) compiled for the host under AddressSanitizer + UBSan (tests/hostcheck/encrows_host.cpp) and run on every case of
tests/rowcases.py over the arena the product's own layout makes with track_rows set: the rows are the host coder's, with the
threads run forwards and backwards, and there is no access outside a region (the gaps are poisoned) -- an entry index at and beyond
the tracked count, a mesh that failed and an empty one included.  A check of the product source on CPU, not a CPU encode path of
the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rowcases as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encrows_host.cpp")
DATA_TYPES = {np.dtype(np.int8): 1, np.dtype(np.uint8): 2, np.dtype(np.int16): 3, np.dtype(np.uint16): 4, np.dtype(np.int32): 5, np.dtype(np.uint32): 6,
              np.dtype(np.float32): 9}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encrows") / "encrows_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            nv, nf = len(c.pos), len(c.faces)
            gen = None if c.generic is None else np.ascontiguousarray(c.generic, np.uint8).reshape(nv, -1)
            f.write(struct.pack("<12I", c.form, nv, nf, int(c.nrm is not None), int(c.uv is not None), 0 if c.nid is None else len(c.nrm), 0 if c.uid is None else len(c.uv),
                                0 if gen is None else gen.shape[1], c.opt.get("repair_topology", 0), c.opt.get("traversal_method", 0), int(c.weld_attributes), len(c.extras)))
            f.write(np.ascontiguousarray(c.faces, np.uint32).tobytes())
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            for values, ids in ((c.nrm, c.nid), (c.uv, c.uid)):
                if values is not None:
                    f.write(np.ascontiguousarray(values, np.float32).tobytes())
                    if ids is not None:
                        f.write(np.ascontiguousarray(ids, np.uint32).tobytes())
            if gen is not None:
                f.write(gen.tobytes())
            for e in c.extras:
                f.write(struct.pack("<3I", DATA_TYPES[e.values.dtype], e.values.shape[1], 0 if e.corners is None else len(e.values)))
                f.write(np.ascontiguousarray(e.values).tobytes())
                if e.corners is not None:
                    f.write(np.ascontiguousarray(e.corners, np.uint32).tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "meshes.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encrows: %d meshes, entry rows and source rows as the host coder has them, forwards and backwards" % len(cases) in r.stdout


@pytest.mark.parametrize("group", [g for g in R.cases() if g != "linear"])
def test_every_case(exe, tmp_path, group):
    cases = R.cases()[group]
    assert len(cases) >= 10
    run(exe, tmp_path, cases)


def test_the_smallest_mesh(exe, tmp_path):
    """One triangle, per vertex and per point."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.uint32)
    run(exe, tmp_path, [R.case("triangle", 1, tri, f), R.case("triangle-points", 2, tri, f, tri, None, tri[:, :2].copy())])
