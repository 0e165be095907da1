"""The host-compilable part of the joined vertex arrays (draco-sharp_amd/csrc/dsa_joined_arrays.h: the layout of a group and the
body of k_joined_arrays' gather) compiled under AddressSanitizer + UBSan (tests/hostcheck/joined_host.cpp) and run on clouds cut
into parts by the CPU coder (synth.encode_split) and decoded by the oracle: every array aligned, inside the reported size and apart
from every other; in both formats and both orders the rows equal to the numpy concatenation / permutation of the per-part
expectation (vacases.expected_rows); the members run forwards and backwards over a poisoned block; a target row beyond num_rows
writes nothing; a group whose members differ in their attribute tables is refused.  A check of the product source on CPU, not a CPU
decode path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import oracle
import vacases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "joined_host.cpp")
POISON = 0xEE


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("joined") / "joined_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def fnv(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def cut(n, part_points, seed, extras=True, bits=11):
    """[(oracle mesh, rows)] of a cloud of n points cut at part_points: colour uint8 x 3 and an int16 x 3 behind the positions"""
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 3), np.float32)
    extra = None
    if extras:
        extra = [synth.Extra(rng.integers(0, 256, (n, 3)).astype(np.uint8), attribute_type=2), synth.Extra(rng.integers(-30000, 30000, (n, 3)).astype(np.int16), attribute_type=4)]
    parts = synth.encode_split(pos, extra=extra, opt=synth.options(pos_bits=bits), part_points=part_points)
    return [(oracle.decode(stream), np.asarray(rows, np.uint32)) for stream, rows, _, _ in parts]


@pytest.fixture(scope="module")
def groups():
    """(name, [(oracle mesh, rows)], refused) per group"""
    a = cut(777, 200, 11)                       # 4 parts of 194 / 195 points: byte rows at odd first rows
    b = cut(130, 65, 12, extras=False, bits=18)  # positions of 18 bits: absent from the quantised format
    c = cut(5, 0, 13)
    c[0][1][3] = 5 + 5                           # a target row beyond the group's rows: that point is left out
    assert len(a) == 4 and len(b) == 2 and len(c) == 1
    return [("parts", a, False), ("18-bits", b, False), ("bad-target", c, False), ("two-tables", [a[0], b[0]], True)]


def write(path, groups):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(groups)))
        for name, members, refused in groups:
            f.write(struct.pack("<I", len(members)))
            for ref, rows in members:
                assert ref.num_faces == 0 and all(len(a.point_map) == 0 for a in ref.attributes)
                f.write(struct.pack("<III", ref.num_points, 0, len(ref.attributes)))
                for att in ref.attributes:
                    f.write(bytes([att.att_type, att.data_type, att.num_components, att.seq_type, vacases.quantisation_bits(att), 0, 0, 0]))
                    f.write(struct.pack("<I", att.num_entries))
                    f.write(att.values.tobytes())
                    if att.seq_type != 0:
                        f.write(np.ascontiguousarray(att.portable, np.int32).tobytes())
                assert len(rows) == ref.num_points
                f.write(np.ascontiguousarray(rows, np.uint32).tobytes())


def padded(ref, a, fmt):
    """(rows as bytes [points, stride], data type, components) of attribute a of a part, None where the format leaves it out"""
    att = ref.attributes[a]
    rows = vacases.expected_rows(ref, a, fmt)
    if rows is None:
        return None
    quantised = fmt == "quantized" and att.seq_type in (2, 3)
    width = rows.shape[1] * rows.itemsize
    stride = (width + 3) & ~3 if quantised else width
    out = np.zeros((len(rows), stride), np.uint8)
    out[:, :width] = np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), -1)
    return out, 4 if quantised else att.data_type, rows.shape[1]


def test_layout_and_gather_of_both_formats_and_orders(exe, tmp_path, groups):
    path = tmp_path / "groups.bin"
    write(path, groups)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "joined: %d groups, both formats and both orders laid out and gathered" % len(groups) in r.stdout, r.stdout
    lines = r.stdout.splitlines()
    sizes = {tuple(int(x) for x in ln.replace(":", "").split()[2:5:2]): int(ln.split()[-1]) for ln in lines if ln.startswith("bytes ")}
    assert sizes[(1, 0)] < sizes[(0, 0)] and sizes[(0, 5)] < sizes[(0, 0)] and sizes[(1, 5)] < sizes[(1, 0)]
    for g, (name, members, refused) in enumerate(groups):
        if refused:
            assert "group %d refused why 2 member 1" % g in lines, (name, lines[:8])       # JA_TABLE, shown by the second member
            assert not [ln for ln in lines if ln.startswith("group %d format" % g)], name
            continue
        sums = np.cumsum([0] + [ref.num_points for ref, _ in members])
        assert "group %d rows %d first %s" % (g, sums[-1], " ".join(str(x) for x in sums[:-1])) in lines, (name, lines[:8])
        n = int(sums[-1])
        for fi, fmt in enumerate(("values", "quantized")):
            for order in (0, 1):
                head = "group %d format %d order %d " % (g, fi, order)
                got = [ln[len(head):] for ln in lines if ln.startswith(head)]
                assert len(got) == len(members[0][0].attributes), (name, got)
                for a in range(len(members[0][0].attributes)):
                    per_part = [padded(ref, a, fmt) for ref, _ in members]
                    if per_part[0] is None:
                        assert name == "18-bits" and a == 0 and fmt == "quantized"
                        assert got[a] == "attribute %d absent" % a, (name, got[a])
                        continue
                    joined = np.concatenate([p[0] for p in per_part])
                    if order == 1:
                        rows = np.concatenate([rows for _, rows in members]).astype(np.int64)
                        ok = rows < n
                        assert ok.all() == (name != "bad-target")
                        out = np.full_like(joined, POISON)
                        out[rows[ok]] = joined[ok]
                        if name != "bad-target":
                            assert np.array_equal(np.sort(rows), np.arange(n))         # a bijection: every row written once
                        joined = out
                    want = "attribute %d stride %d type %d components %d digest %s" % (a, joined.shape[1], per_part[0][1], per_part[0][2], fnv(joined.tobytes()))
                    assert got[a] == want, (name, fmt, order, got[a], want)
