"""dsa_encode_voxel_sequential_batch (voxels coarser than the position grid: the first point, the centroid or the nearest point of
every voxel, on the device): the ctypes mirror and the C# declaration of its struct against the header as a C compiler lays it out, the
defaults, the exports in every layer, every option the call refuses before anything is touched and the field its message names,
voxel_bits = 0 reaching the normal-mean path, the errors of Config and how it routes, the words of the header.  No GPU needed: the
options are checked before the context is looked at, and a context that was never opened still carries the message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("normal_mean", "voxel_bits", "voxel_point", "reserved")
SYMBOLS = ("dsa_encode_default_voxel_options", "dsa_encode_voxel_sequential_batch")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_voxel_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_voxel_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu %zu %d %d %d", sizeof(dsa_encode_normal_mean_options), sizeof(dsa_encode_vote_options), DSA_VOXEL_POINT_FIRST, DSA_VOXEL_POINT_CENTROID, DSA_VOXEL_POINT_NEAREST);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt = native.EncodeVoxelOptions
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS)
    assert got == [C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [320, 288, 0, 1, 2]       # (the existing structs stay)
    assert C.sizeof(opt) == C.sizeof(native.EncodeNormalMeanOptions) + 32 == 352 and opt.voxel_bits.offset == 320 and opt.voxel_point.offset == 324 and opt.reserved.offset == 328
    assert dict(opt._fields_)["voxel_bits"] is C.c_int32 and dict(opt._fields_)["voxel_point"] is C.c_int32 and dict(opt._fields_)["normal_mean"] is native.EncodeNormalMeanOptions
    assert (native.VOXEL_POINT_FIRST, native.VOXEL_POINT_CENTROID, native.VOXEL_POINT_NEAREST) == (0, 1, 2) == (dsa.VOXEL_POINT_FIRST, dsa.VOXEL_POINT_CENTROID, dsa.VOXEL_POINT_NEAREST)


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4                       # the feature is detected by the symbol


def options(point_order=1, geometry=0, merge_points=1, part_cells=0, lod_base_bits=0, position_bits=None, mean_normals=0, **kw):
    o = native.EncodeVoxelOptions()
    native.lib().dsa_encode_default_voxel_options(C.byref(o))
    m = o.normal_mean.vote.mean.lod.cell_parts.split.merge
    m.order.point_order, m.merge_points = point_order, merge_points
    o.normal_mean.vote.mean.lod.cell_parts.part_cells, o.normal_mean.vote.mean.lod.lod_base_bits, o.normal_mean.mean_normals = part_cells, lod_base_bits, mean_normals
    if geometry is not None:
        m.order.sequential.geometry = geometry
    if position_bits is not None:
        m.order.sequential.base.position_bits = position_bits
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_normal_mean_call():
    L = native.lib()
    xo, no = native.EncodeVoxelOptions(), native.EncodeNormalMeanOptions()
    C.memset(C.byref(xo), 0xFF, C.sizeof(xo))
    L.dsa_encode_default_voxel_options(C.byref(xo))
    L.dsa_encode_default_normal_mean_options(C.byref(no))
    assert bytes(xo.normal_mean) == bytes(no) and xo.voxel_bits == 0 and xo.voxel_point == 0 and list(xo.reserved) == [0] * 6
    L.dsa_encode_default_voxel_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_voxel_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    refused(options(voxel_bits=-1), "voxel_bits below 0")
    refused(options(voxel_bits=12), "voxel_bits above the default position_bits 11")
    refused(options(voxel_bits=15, position_bits=14), "voxel_bits above position_bits")
    refused(options(voxel_bits=5, merge_points=0), "voxel_bits without merge_points")
    refused(options(voxel_bits=5, merge_points=0, point_order=0), "voxel_bits without merge_points and point_order")
    refused(options(voxel_bits=5, geometry=1), "voxel_bits with geometry 1")
    for value in (-1, 3, 1 << 16):
        refused(options(voxel_bits=5, voxel_point=value), "voxel_point outside 0 .. 2")
    for value in (1, 2):
        refused(options(voxel_point=value), "voxel_point without voxel_bits")
    refused(options(voxel_bits=5, lod_base_bits=6, part_cells=7), "lod_base_bits above voxel_bits")
    for k in range(6):
        o = options(voxel_bits=5, voxel_point=1)
        o.reserved[k] = 1
        refused(o, "reserved")
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved, voxel_bits 0")
    # what the nested calls refuse, through this one
    refused(options(voxel_bits=5, mean_normals=2), "mean_normals")
    refused(options(voxel_bits=5, lod_base_bits=3), "lod_base_bits without part_cells")
    refused(options(voxel_bits=5, part_cells=-1), "part_cells")
    o = options(voxel_bits=5)
    o.normal_mean.reserved[3] = 1
    refused(o, "normal_mean.reserved")
    o = options(voxel_bits=5)
    o.normal_mean.vote.mean.mean_attributes = 1 << 20
    refused(o, "mean_attributes")
    # valid options get as far as the missing context
    for point in (0, 1, 2):
        refused(options(voxel_bits=5, voxel_point=point, lod_base_bits=5, part_cells=7, mean_normals=1), "no context")
        refused(options(voxel_bits=11, voxel_point=point), "no context, voxel_bits = position_bits")
    refused(options(), "no context, nothing asked")
    assert L.dsa_encode_voxel_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_the_words_of_every_refusal():
    """the check itself, in the source: every refusal of the new struct names its field, in the order the header lists them, in front
    of the nested checks where it needs nothing of them"""
    src = open(os.path.join(ROOT, "draco-sharp_amd", "csrc", "dsa_encode.h")).read()
    body = src[src.index("static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_voxel_options &o"):]
    body = body[:body.index("\n}\n")]
    words = ['ENC_REFUSE("voxel_bits %d: 0', 'ENC_REFUSE("voxel_bits %d needs merge_points 1', 'ENC_REFUSE("voxel_point %d: 0 (DSA_VOXEL_POINT_FIRST)',
             'ENC_REFUSE("voxel_point %d needs voxel_bits >= 1', 'ENC_RESERVED(o, 6, "dsa_encode_voxel_options")', "enc_check_options(ctx, o.normal_mean, null_argument)",
             'ENC_REFUSE("voxel_bits %d is above position_bits %d', 'ENC_REFUSE("lod_base_bits %d is above voxel_bits %d']
    at = [body.index(w) for w in words]
    assert at == sorted(at)


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeVoxelOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeNormalMeanOptions NormalMean", "public int VoxelBits", "public int VoxelPoint", "public fixed int Reserved[6]"]
    h = re.search(r"typedef struct dsa_encode_voxel_options \{(.*?)\} dsa_encode_voxel_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_normal_mean_options normal_mean", "int32_t voxel_bits", "int32_t voxel_point", "int32_t reserved[6]"]
    for name in ("dsa_encode_default_voxel_options(out DsaEncodeVoxelOptions options)",
                 "dsa_encode_voxel_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeVoxelOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int VoxelBits", "public int VoxelPoint", "dsa_encode_voxel_sequential_batch", "xo.VoxelBits = VoxelBits", "xo.VoxelPoint = VoxelPoint",
                 "xo.NormalMean.MeanNormals = MeanNormals ? 1u : 0u", "xo.NormalMean.Vote.Mean.Lod.LodBaseBits = LodBaseBits", "VoxelBits needs MergePoints 1", "VoxelPoint needs VoxelBits >= 1"):
        assert word in enc
    assert enc.count("if (VoxelBits != 0)") == 2 and enc.index("if (VoxelBits != 0)") < enc.index("else if (MeanNormals)")      # the widest call first, in both places


def test_the_words_of_the_header():
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    comment = header[header.index("dsa_encode_normal_mean_sequential_batch with voxels coarser than the position grid"):header.index("typedef struct dsa_encode_voxel_options")]
    for word in ("voxel(r) = key(r) >> 3 s", "s = B - C", "first[j]", "smallest (key, row)", "NOT in", "P[j][c] = floor((2 S + cnt) / (2 cnt))", "ties upwards",
                 "2 (q[r][c] & (2^s - 1)) - (2^s - 1)", "smallest (dist, row)", "L = C - D + 1", "ceil(n / N) + L - 1", "voxel_bits = 0 with voxel_point = 0", "voxel_bits = B with any voxel_point",
                 "DSA_ERR_INVALID_ARGUMENT", "k_enc_voxel_near", "k_enc_voxel_pick", "dsa_encode_grid_sequential_batch"):
        assert word in comment, word
    for word in ("weighted centroids", "the row nearest the centroid", "not a power of two of the grid step", "voxels of", "reductions per coarser lod cell"):
        assert word in comment[comment.index("Not built:"):], word
    # "the smallest input row of its cell" holds with voxel_bits = 0 alone, and the header says so where it says it
    for m in re.finditer(r"smallest input row\s+\*?\s*of (its|the) cell", header):
        assert "with voxel_bits = 0" in header[m.start():m.start() + 160] or "NOT in" in header[m.start() - 120:m.start()], header[m.start():m.start() + 80]


def test_config_switch():
    base = dict(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    assert dsa.Config().voxel_bits == 0 and dsa.Config().voxel_point == 0
    cfg = dsa.Config(voxel_bits=5, voxel_point=dsa.VOXEL_POINT_CENTROID, **base)
    assert cfg.voxel_bits == 5 and cfg.voxel_point == 1
    for bad in (-1, 12, 1.5, "5", None, True):
        with pytest.raises(ValueError, match="voxel_bits"):
            dsa.Config(voxel_bits=bad, **base)
    assert dsa.Config(voxel_bits=14, position_bits=14, **base).voxel_bits == 14
    for bad in (-1, 3, "centroid", None):
        with pytest.raises(ValueError, match="voxel_point"):
            dsa.Config(voxel_bits=5, voxel_point=bad, **base)
    with pytest.raises(ValueError, match="voxel_point.*needs voxel_bits >= 1"):
        dsa.Config(voxel_point=dsa.VOXEL_POINT_NEAREST, **base)
    for kw in (dict(point_order=dsa.POINT_ORDER_MORTON, encoding_method=0), dict(encoding_method=0), dict()):
        with pytest.raises(ValueError, match="voxel_bits.*merge_points=MERGE_CELLS"):
            dsa.Config(voxel_bits=5, **kw)
    with pytest.raises(ValueError, match="lod_base_bits 6 is above voxel_bits 5"):
        dsa.Config(voxel_bits=5, part_cells=7, lod_base_bits=6, **base)
    cfg = dsa.Config(voxel_bits=9, voxel_point=dsa.VOXEL_POINT_NEAREST, mean_normals=True, vote_attributes=[3], mean_attributes=[2], part_cells=4096, lod_base_bits=9, position_bits=13, **base)
    pos = np.zeros((4, 3), np.float32)
    colour, label = dsa.Attribute(np.zeros((4, 3), np.uint8)), dsa.Attribute(np.zeros((4, 1), np.uint8))
    cloud = dsa.PointCloudData(pos, normals=np.ones((4, 3), np.float32), attributes=[colour, label])
    o = cfg._native_voxel(0, [cloud])
    assert (o.voxel_bits, o.voxel_point, list(o.reserved)) == (9, 2, [0] * 6)
    n = o.normal_mean
    assert n.mean_normals == 1 and n.vote.vote_attributes == 0b1000 and n.vote.mean.mean_attributes == 0b100 and n.vote.mean.lod.lod_base_bits == 9 and n.vote.mean.lod.cell_parts.part_cells == 4096
    m = n.vote.mean.lod.cell_parts.split.merge
    assert m.merge_points == 1 and m.order.point_order == 1 and m.order.sequential.geometry == 0 and m.order.sequential.base.position_bits == 13


class _Recorder:
    """native.lib() with every encode entry point replaced by a recorder: which call EncodeBatch chooses, and with what."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.startswith("dsa_encode_") or "default" in name:
            return real

        def record(*args):
            self.calls.append((name, args))
            return 0
        return record


def test_encode_batch_takes_the_new_entry_point_only_when_asked(monkeypatch):
    r = _Recorder(native.lib())
    monkeypatch.setattr(native, "lib", lambda: r)

    class Ctx:
        _h = None
    enc = dsa.DracoEncoder(Ctx())
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    label, colour = dsa.Attribute(np.zeros((4, 1), np.uint8)), dsa.Attribute(np.zeros((4, 3), np.uint8))
    cloud, bare = dsa.PointCloudData(pos, normals=np.ones((4, 3), np.float32), attributes=[label, colour]), dsa.PointCloudData(pos)
    base = dict(point_order=1, merge_points=1, encoding_method=0)
    # voxel_bits = 0: the calls keep arriving where they always did
    enc.EncodeBatch([cloud], dsa.Config(**base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(part_cells=2, lod_base_bits=3, **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(mean_attributes=[3], **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(mean_normals=True, voxel_bits=0, **base), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_merged_sequential_batch", "dsa_encode_lod_sequential_batch", "dsa_encode_mean_sequential_batch", "dsa_encode_normal_mean_sequential_batch"]
    del r.calls[:]
    for cfg, clouds, want in ((dsa.Config(voxel_bits=4, **base), [cloud, bare], (4, 0, 0, 0, 0, 0, 0)),
                              (dsa.Config(voxel_bits=4, voxel_point=1, mean_normals=True, vote_attributes=[2], mean_attributes=[3], part_cells=2, **base), [cloud, cloud], (4, 1, 1, 4, 8, 2, 0)),
                              (dsa.Config(voxel_bits=11, voxel_point=2, part_cells=2, lod_base_bits=3, **base), [bare, cloud], (11, 2, 0, 0, 0, 2, 3))):
        enc.EncodeBatch(clouds, cfg, handle=True)
        assert [c[0] for c in r.calls] == ["dsa_encode_voxel_sequential_batch"]
        _, n, _, grids, opt, _ = r.calls[0][1]
        o = opt._obj
        nm = o.normal_mean
        assert n == 2 and grids is None
        assert (o.voxel_bits, o.voxel_point, nm.mean_normals, nm.vote.vote_attributes, nm.vote.mean.mean_attributes, nm.vote.mean.lod.cell_parts.part_cells, nm.vote.mean.lod.lod_base_bits) == want
        del r.calls[:]
    with pytest.raises(ValueError, match="takes point clouds"):
        enc.EncodeBatch([dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32))], dsa.Config(voxel_bits=4, **base), handle=True)
