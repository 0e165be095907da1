"""The encoder's mean-normal kernels (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_normal_sum, k_enc_normal_store, behind the product's
sort and merge and under the product's launch sequence, in the arena of the product's layout) compiled for the host under
AddressSanitizer + UBSan (tests/hostcheck/encnormalmeans_host.cpp) and held against the host coder (synth::merge_points,
synth::merge_mean_normals, which shares nothing with the kernels but the quantiser's tail) on every case of tests/mergecases.py: alone
and with an averaged and a voted stream beside the normals -- the means and the normals each count the rows of every cell, in regions of
their own, and neither count may be doubled -- the threads run forwards and backwards, the arena's gaps poisoned and the sums and counts
filled with a pattern until the product's memset; with part_cells and lod_base_bits through the levels and the part slots the product
runs behind the pass; and a chunk without normals, whose layout must be the one of the request without the option.  A check of the
product source on CPU, not a CPU encode path of the product."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mergecases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encnormalmeans_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encnormalmeans") / "encnormalmeans_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def write(path, cases, part_cells=0, lod_base_bits=0):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<IIIII", len(c.pos), c.bits, int(c.grid is not None), part_cells, lod_base_bits))
            f.write(np.ascontiguousarray(c.pos, np.float32).tobytes())
            if c.grid is not None:
                f.write(np.float32(list(c.grid[0]) + [c.grid[1]]).tobytes())


def run(exe, tmp_path, cases, **slots):
    path = tmp_path / "cases.bin"
    write(path, cases, **slots)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    points = sum(len(c.pos) for c in cases)
    cells = sum(len(mergecases.pin(c.pos, c.bits, c.grid)[0]) for c in cases)
    # alone and beside a mean and a vote, forwards and backwards
    assert "encnormalmeans: %d cases in " % len(cases) in r.stdout and "(%d points, %d cells, " % (4 * points, 4 * cells) in r.stdout, r.stdout
    return int(re.search(r"(\d+) code components moved", r.stdout).group(1))


def test_every_case(exe, tmp_path):
    cases = mergecases.cases()
    assert len({c.bits for c in cases}) >= 3 and any(c.grid is None for c in cases) and any(c.name == "tile-with-no-head" for c in cases)
    assert run(exe, tmp_path, cases) > 1000             # kept rows whose code the mean changed: there is something to average


def test_a_large_cloud(exe, tmp_path):
    """about 70 000 points in 2 049 cells: 69 tiles, most of them without a head"""
    c = mergecases.large()
    assert 60000 < len(c.pos) < 80000
    run(exe, tmp_path, [c])


def test_normals_through_levels_and_slots(exe, tmp_path):
    """three clouds of 1, 1 025 and 2 100 points with duplicates at 6 bits, part_cells = 7, lod_base_bits = 4: the steps the product
    runs behind the pass -- k_enc_lod_cells rewrites the cells[] the sum read -- leave the mean codes where they were"""
    cases = [mergecases.half_duplicated(n, 90 + n, bits=6) for n in (1, mergecases.TILE + 1, 2100)]
    run(exe, tmp_path, cases, part_cells=7, lod_base_bits=4)
