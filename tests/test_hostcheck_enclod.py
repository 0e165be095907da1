"""The encoder's level-of-detail steps (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_lod_levels, k_enc_lod_scan,
k_enc_lod_scatter, k_enc_lod_cells, k_enc_part_cells, between the product's merge and its part boxes, under the product's launch
sequence, in the arena of the product's layout for a chunk with lod_base_bits >= 1 -- ceil(n / N) + L - 1 part slots sized on the
device, a set of stream records per slot on one set of values, lod and pos in the sort's dead key buffer) compiled for the host
under AddressSanitizer + UBSan (tests/hostcheck/enclod_host.cpp, a program of its own) and held against the host coder
(synth::lod_parts) on every case of tests/lodcases.py, with the threads run forwards and backwards, the arena's gaps poisoned, and
the regions of every slot that stays empty poisoned too: no kernel touches them.  A check of the product source on CPU, not a CPU
encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import lodcases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "enclod_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("enclod") / "enclod_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<IIIII", len(c.pos), c.bits, int(c.grid is not None), c.part_cells, c.lod_base_bits))
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            if c.grid is not None:
                f.write(np.float32(list(c.grid[0]) + [c.grid[1]]).tobytes())


def run(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    write(path, cases)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    points = sum(len(c.pos) for c in cases)
    parts = sum(len(lc.pin(c).ranges) for c in cases)
    empty = sum(lc.slots(c) for c in cases) - parts
    assert "enclod: %d cases in " % len(cases) in r.stdout, r.stdout
    assert "(%d points, %d parts, %d empty slots untouched)" % (2 * points, 2 * parts, 2 * empty) in r.stdout, r.stdout
    return empty


def test_every_case(exe, tmp_path):
    cases = lc.cases()
    assert len(cases) > 45 and any(c.grid is None for c in cases) and any(c.lod_base_bits == c.bits for c in cases)
    assert {c.part_cells for c in cases} >= {1, 2, 63, 64, 65, lc.TILE - 1, lc.TILE, lc.TILE + 1, lc.INT32_MAX}
    assert run(exe, tmp_path, cases) > 80


def test_the_large_cloud(exe, tmp_path):
    c = lc.large()
    assert len(c.pos) == 70001 and lc.slots(c) == 238
    assert run(exe, tmp_path, [c]) == 238 - len(lc.pin(c).ranges)
