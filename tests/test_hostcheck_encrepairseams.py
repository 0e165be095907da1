"""Attributes given per corner over a mesh whose topology needs the repair, the device's side compiled for the host under
AddressSanitizer + UBSan (tests/hostcheck/encrepairseams_host.cpp): the repair kernels with k_enc_repair_face_scan and
k_enc_repair_ids (draco-sharp_amd/csrc/dsa_encode_repair.h), CornerTable::from_repaired, then the table, walk and seam kernels
(dsa_encode_seams.h) over the repaired chunk with the ids the kernels compacted -- held against the host coder with
repair_topology = 2 on the same faces and ids, and not one access outside a mesh's arrays.  A check of the product source on CPU,
not a CPU encode path."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import defects
import seamdefects as sd
import draco_sharp_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "encrepairseams_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encrepairseams") / "encrepairseams_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def run(exe, tmp_path, meshes):
    """meshes: Seamed (rows of an attribute: those of its value array), or (Seamed, normal rows, uv rows)"""
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(meshes)))
        for m in meshes:
            m, rows_n, rows_u = (m, len(m.nrm), len(m.uv)) if isinstance(m, sd.Seamed) else m
            faces = np.ascontiguousarray(m.faces, np.uint32).reshape(-1, 3)
            f.write(struct.pack("<II", len(m.pos), len(faces)))
            f.write(faces.tobytes())
            f.write(struct.pack("<I", (1 if m.nid is not None else 0) | (2 if m.uid is not None else 0)))
            for ids, rows in ((m.nid, rows_n), (m.uid, rows_u)):
                if ids is not None:
                    f.write(struct.pack("<I", rows))
                    f.write(np.ascontiguousarray(ids, np.uint32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def counts(out):
    return dict(zip(("meshes", "coded", "repaired", "seamed", "wide", "refused", "bad", "bound"), (int(x) for x in re.findall(r"\d+", out))))


def test_named_and_placed_cases_with_ids_of_three_kinds(exe, tmp_path):
    meshes = [sd.with_ids(c, kind, j) for c in defects.named() + defects.placed() for j, kind in enumerate(sd.ID_KINDS)]
    got = counts(run(exe, tmp_path, meshes))
    assert got["coded"] == got["repaired"] == len(meshes) and got["seamed"] > len(meshes) // 2 and got["bound"] == 0, got


def test_the_whole_array_shifts_behind_a_degenerate_face(exe, tmp_path):
    """degenerate-first / degenerate-last with every corner its own row: the compacted array is the source's moved by two faces /
    cut short by one, narrow and wide."""
    cases = [c for c in defects.placed() if c.name in ("degenerate-first", "degenerate-last")]
    meshes = []
    for c in cases:
        m = sd.with_ids(c, "corner")
        meshes += [m, (m, 70000, 65537), (m, 65536, 65536)]
    got = counts(run(exe, tmp_path, meshes))
    assert got["coded"] == got["repaired"] == 6 and got["wide"] == 4, got


def test_injected_small_meshes_and_seamed_sources(exe, tmp_path):
    meshes = []
    for k, c in enumerate(defects.injected_small()):
        meshes.append(sd.with_ids(c, sd.ID_KINDS[k % 3], k))
    for j, charts in enumerate(sd.CHARTS):
        for name, kind, nx, ny in (("grid", synth.GRID, 6, 5), ("torus", synth.TORUS, 9, 8), ("holes", synth.HOLES, 14, 12)):
            clean = sd.seamed_source(synth, name, kind, nx, ny, charts, 4 + j)
            meshes.append(clean)                     # (needs no repair: the kernels leave the ids as they are)
            for k, defect in enumerate(defects.KINDS):
                meshes.append(sd.inject(clean, defect, 1 + 4 * ((j + k) % 2), np.random.default_rng(100 * j + 10 * k)))
    got = counts(run(exe, tmp_path, meshes))
    assert got["coded"] == len(meshes) and got["repaired"] >= len(meshes) - 15 - 20 and got["seamed"] > 0 and got["bound"] == 0, got


def test_soups_with_ids(exe, tmp_path):
    soups = defects.soups(2000)
    meshes = [sd.soup_with_ids(c, k) for k, c in enumerate(soups)]
    got = counts(run(exe, tmp_path, meshes))
    all_degenerate = sum(1 for c in soups if defects.is_degenerate(c.faces).all())
    assert got["refused"] == all_degenerate and got["coded"] + got["refused"] + got["bound"] == 2000 and got["bound"] == 0, got
    assert got["repaired"] > 500 and got["seamed"] > 500, got


def test_an_id_out_of_range_fails_its_mesh_alone(exe, tmp_path):
    c = next(c for c in defects.named() if c.name == "grid-face-doubled")
    good = sd.with_ids(c, "stripes")
    bad_n = good._replace(nid=np.where(np.arange(good.nid.size).reshape(-1, 3) == 7, len(good.nrm), good.nid).astype(np.uint32))
    bad_u = good._replace(uid=np.where(np.arange(good.uid.size).reshape(-1, 3) == 50, len(good.uv) + 9, good.uid).astype(np.uint32))
    d = next(c for c in defects.placed() if c.name == "degenerate-first")
    deg = sd.with_ids(d, "corner")
    bad_deg = deg._replace(uid=np.where(np.arange(deg.uid.size).reshape(-1, 3) == 1, 1 << 20, deg.uid).astype(np.uint32))      # (in a degenerate face: checked all the same)
    got = counts(run(exe, tmp_path, [good, bad_n, good, bad_u, bad_deg, good]))
    assert got["coded"] == 3 and got["bad"] == 3, got
