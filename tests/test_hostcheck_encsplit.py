"""The encoder's part kernel (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_part_bounds, behind the product's sort and under the
product's launch sequences, in the arena of the product's layout for a split chunk -- a set of stream records per part on one set
of values) compiled for the host under AddressSanitizer + UBSan (tests/hostcheck/encsplit_host.cpp) and held against the host coder
(synth::split_parts, synth::part_boxes) on every case of tests/splitcases.py, with the threads run forwards and backwards and the
arena's gaps poisoned.  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import splitcases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encsplit_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encsplit") / "encsplit_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<IIII", len(c.pos), c.bits, int(c.grid is not None), c.part_points))
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            if c.grid is not None:
                f.write(np.float32(list(c.grid[0]) + [c.grid[1]]).tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    points = sum(len(c.pos) for c in cases)
    parts = sum(len(sc.parts(len(c.pos), c.part_points)) for c in cases)
    assert "encsplit: %d cases in " % len(cases) in r.stdout and "(%d points, %d parts)" % (2 * points, 2 * parts) in r.stdout, r.stdout


def test_every_case(exe, tmp_path):
    cases = sc.cases()
    assert len(cases) > 100 and any(c.grid is not None for c in cases) and any(c.name == "run-over-a-cut" for c in cases)
    assert {c.part_points for c in cases} >= {1, 2, 63, 64, 65, sc.TILE - 1, sc.TILE, sc.TILE + 1, sc.INT32_MAX}
    run(exe, tmp_path, cases)


def test_the_18_part_cloud(exe, tmp_path):
    c = sc.large()
    assert len(c.pos) == 70001 and len(sc.parts(70001, c.part_points)) == 18
    run(exe, tmp_path, [c])
