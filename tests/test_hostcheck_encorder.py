"""The encoder's point-order kernels (draco-sharp_amd/csrc/dsa_encode_order.h: keys, the segmented radix sort, rank, the faces
through rank, under the product's launch sequence enc_order_stage and in the arena of the product's layout) compiled for the host
under AddressSanitizer + UBSan (tests/hostcheck/encorder_host.cpp) and held against the host coder's order (synth::point_order) on
every case of tests/ordercases.py, with the threads run forwards and backwards and the arena's gaps poisoned.  A check of the
product source on CPU, not a CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ordercases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encorder_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encorder") / "encorder_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            faces = np.zeros((0, 3), np.uint32) if c.faces is None else np.ascontiguousarray(c.faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<IIII", len(c.pos), c.bits, int(c.grid is not None), len(faces)))
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            if c.grid is not None:
                f.write(np.float32(list(c.grid[0]) + [c.grid[1]]).tobytes())
            f.write(faces.tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encorder: %d cases in " % len(cases) in r.stdout and "ordered as the host coder orders them" in r.stdout


def test_every_case(exe, tmp_path):
    cases = ordercases.cases()
    assert {c.bits for c in cases} >= set(ordercases.PASS_BITS) and any(c.faces is not None for c in cases) and any(c.grid is not None for c in cases)
    run(exe, tmp_path, cases)


def test_wide_faces(exe, tmp_path):
    """A mesh over more than 65 536 points: its compressed indices are remapped at 32 bits."""
    pos = ordercases.random_cloud(66000, 41)
    faces = np.random.default_rng(42).integers(0, len(pos), (500, 3)).astype(np.uint32)
    run(exe, tmp_path, [ordercases.Case("wide", pos, 9, None, faces)])
