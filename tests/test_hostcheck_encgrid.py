"""The encoder's grid kernels (draco-sharp_amd/csrc/dsa_encode_grid.h: the bounds of an array with its finite flag, the fold of a
group, the quantiser on a given grid with its smallest offending rows) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/encgrid_host.cpp) and held against the host coder (synth::shared_grid, synth::quantize_on_grid) on every case of
tests/gridcases.py: the same keys, flags, grids, integers and refusals with the threads run forwards and backwards and with one
block per array and with three -- which thread wins a minimum changes no number that leaves the kernels -- and no access outside
an array (the arena's gaps are poisoned).  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gridcases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encgrid_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encgrid") / "encgrid_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def arrays():
    """(group, bits, explicit (origin, range) or None, values): every case of gridcases.py, arrays of one group side by side"""
    out = []
    tiles = [c for c, _ in gc.tiles()]
    out += [(1, gc.POS_BITS, None, c.pos) for c in tiles]
    out += [(2, gc.UV_BITS, None, c.uvs) for c in tiles]
    v = gc.voxel()
    out.append((3, gc.POS_BITS, (np.zeros(3, np.float32), np.float32(2047.0)), v.pos))
    t = gc.texel()
    out.append((4, gc.UV_BITS, (np.zeros(2, np.float32), np.float32(1023.0 / 1024.0)), t.uvs))
    for what in ("off", "edge", "nan", "inf"):
        c, grid, _ = gc.damaged(what)
        out.append((5, gc.POS_BITS, grid, c.pos))
    # a group with a member that holds a NaN (it takes no part), one whose members all do, a flat one, one value, no rows
    nan = gc.damaged("nan")[0].pos
    out += [(6, gc.POS_BITS, None, tiles[0].pos), (6, gc.POS_BITS, None, nan + np.float32(50)), (6, gc.POS_BITS, None, tiles[3].pos)]
    out += [(7, 8, None, nan), (7, 8, None, gc.damaged("inf")[0].pos)]
    out += [(8, 14, None, np.full((300, 4), -0.25, np.float32)), (9, 1, None, np.array([[3.5]], np.float32)), (10, 11, None, np.zeros((0, 3), np.float32))]
    out += [(11, 20, None, np.array([[0.0], [-0.0], [1e30], [-1e30]], np.float32)), (11, 20, None, np.array([[-0.0], [0.0]], np.float32))]
    out += [(12, gc.POS_BITS, None, p) for p in gc.cloud_chunks(points=700)]
    return out


def test_grid_kernels_match_the_host_coder_under_asan(exe, tmp_path):
    items = arrays()
    path = tmp_path / "arrays.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for group, bits, grid, values in items:
            v = np.ascontiguousarray(values, np.float32)
            origin = np.zeros(4, np.float32)
            rng = np.float32(0.0)
            if grid is not None:
                origin[:v.shape[1]] = grid[0]
                rng = np.float32(grid[1])
            f.write(struct.pack("<IIII", group, v.shape[1], len(v), bits) + origin.tobytes() + rng.tobytes() + v.tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encgrid: %d arrays bounded, folded and quantised alike, forwards and backwards" % len(items) in r.stdout
