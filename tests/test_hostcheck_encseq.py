"""The index kernel of the sequential encoder (draco-sharp_amd/csrc/dsa_encode_seqidx.h: the phases of k_enc_seq_indices) compiled
for the host under AddressSanitizer + UBSan (tests/hostcheck/encseq_host.cpp) and held against the host coder's
sequential_index_symbols + symbol_stats on the same faces: symbols, bit lengths, maximum, both histograms and total_bl, on 16- and
32-bit face uploads, alphabets on both sides of the LDS histogram's 4096 bins, face counts that are no multiple of the block, and
no access outside a mesh's arrays.  A check of the product source on CPU, not a CPU encode path of the product."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import irregular
import seqcases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encseq_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encseq") / "encseq_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes, blocks):
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for nv, faces in meshes:
            faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", nv, len(faces)))
            f.write(faces.tobytes())
    r = subprocess.run([exe, str(path), str(blocks)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) runs of (\d+) meshes alike \((\d+) as 16-bit uploads, (\d+) within the LDS histogram, (\d+) with symbols beyond it, (\d+) not a multiple", r.stdout)
    assert m, r.stdout
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_statistics_of_every_shape(exe, tmp_path, blocks):
    meshes = []
    for k, kind in enumerate((synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS) * 2):
        nx, ny = 12 + (7 * k) % 29, 12 + (5 * k) % 31
        pos, _, _, faces = synth.make_mesh(kind, nx, ny, 80 + k)
        meshes.append((len(pos), faces))
    for points in sorted(seqcases.WIDTH_GRIDS)[:2]:               # alphabets of 510 and 512 symbols
        pos, _, _, faces = seqcases.grid(points)
        meshes.append((points, faces))
    for c in irregular.SMALL:                                      # flipped, subdivided, thickened, shuffled
        pos, _, _, faces = irregular.mesh(c)
        meshes.append((len(pos), faces))
    for _, pos, _, _, faces in seqcases.refused_by_edgebreaker():  # legal here
        meshes.append((len(pos), faces))
    meshes.append((3, np.array([[0, 1, 2]])))
    meshes.append((1, np.array([[0, 0, 0]])))                      # an alphabet of two symbols
    rng = np.random.default_rng(4)
    meshes.append((2047, rng.integers(0, 2047, (999, 3))))         # random jumps below the LDS limit (2 * 2047 < 4096)
    meshes.append((2049, np.concatenate([rng.integers(0, 2049, (1001, 3)), [[0, 2048, 0]]])))      # ... and just above it: symbols 4096 and 4097, the first two outside the LDS bins
    meshes.append((70000, rng.integers(0, 70000, (5000, 3))))      # 32-bit uploads only, most symbols beyond the LDS bins
    runs, total, narrow, lds_only, beyond, ragged = run(exe, tmp_path, meshes, blocks)
    assert total == len(meshes) and runs == 2 * len(meshes) - 1 and narrow == len(meshes) - 1
    # both upload widths of the 2049-point mesh and the 70 000-point mesh reach past the LDS bins
    assert lds_only >= 8 and beyond >= 3 and ragged >= 10


def test_bench_size_and_wide_meshes(exe, tmp_path):
    meshes = []
    for points in (65535, 65536):
        pos, _, _, faces = seqcases.grid(points)
        faces = faces.copy()
        faces[-1, 2] = points - 1
        meshes.append((points, faces))
    pos, _, _, faces = synth.make_mesh(synth.GRID, 300, 250, 3)      # 75 551 points: 32-bit uploads, an alphabet of 151 102
    meshes.append((len(pos), faces))
    pos, _, _, faces = irregular.mesh("torus-128x256-flipped")
    meshes.append((len(pos), faces))
    runs, total, narrow, lds_only, beyond, ragged = run(exe, tmp_path, meshes, 48)
    assert (runs, total, narrow, lds_only) == (7, 4, 3, 0)
