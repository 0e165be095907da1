"""The encoder's cell-parts step (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_part_cells, between the product's merge and its
part boxes, under the product's launch sequences, in the arena of the product's layout for a cell-parts chunk -- part slots sized on
the device, a set of stream records per slot on one set of values) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/enccellparts_host.cpp) and held against the host coder (synth::cell_parts) on every case of tests/cellpartcases.py,
with the threads run forwards and backwards, the arena's gaps poisoned, and the regions of every slot that stays empty poisoned too:
no kernel touches them.  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cellpartcases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "enccellparts_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("enccellparts") / "enccellparts_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<IIII", len(c.pos), c.bits, int(c.grid is not None), c.part_cells))
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            if c.grid is not None:
                f.write(np.float32(list(c.grid[0]) + [c.grid[1]]).tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    points = sum(len(c.pos) for c in cases)
    parts = sum(len(cc.pin(c)[2]) for c in cases)
    empty = sum(cc.slots(c) for c in cases) - parts
    assert "enccellparts: %d cases in " % len(cases) in r.stdout, r.stdout
    assert "(%d points, %d parts, %d empty slots untouched)" % (2 * points, 2 * parts, 2 * empty) in r.stdout, r.stdout
    return empty


def test_every_case(exe, tmp_path):
    cases = cc.cases()
    assert len(cases) > 150 and any(c.grid is None for c in cases) and any(c.name.startswith("identical") for c in cases)
    assert {c.part_cells for c in cases} >= {1, 2, 63, 64, 65, cc.TILE - 1, cc.TILE, cc.TILE + 1, cc.INT32_MAX}
    assert run(exe, tmp_path, cases) > 500


def test_the_18_part_cloud(exe, tmp_path):
    c = cc.large()
    assert len(c.pos) == 70001 and len(cc.pin(c)[2]) == 18 and cc.slots(c) == 584
    assert run(exe, tmp_path, [c]) == 584 - 18
