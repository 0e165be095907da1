"""dsa_encode_vote_sequential_batch (the most frequent value of every cell in chosen attributes of merged point clouds, on the
device): the ctypes mirror and the C# declaration of its struct against the header as a C compiler lays it out, the defaults, the
exports in every layer, every option the call refuses before anything is touched, mask 0 reaching the mean path, the errors of Config
and how it routes.  No GPU needed (the texts of the refusals need a context to be read from: tests/test_gpu_encode_votes.py asserts
them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("mean", "vote_attributes", "reserved")
SYMBOLS = ("dsa_encode_default_vote_options", "dsa_encode_vote_sequential_batch")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_vote_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_vote_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu %zu %zu %zu %zu %d", sizeof(dsa_encode_mean_options), sizeof(dsa_encode_lod_options), sizeof(dsa_encode_cell_parts_options), sizeof(dsa_part_info), sizeof(dsa_lod_info), DSA_MAX_ATTRIBUTES);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt = native.EncodeVoteOptions
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS)
    assert got == [C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [256, 224, 192, 80, 48, native.MAX_ATTRIBUTES]       # (the existing structs stay)
    assert C.sizeof(opt) == C.sizeof(native.EncodeMeanOptions) + 32 == 288 and opt.vote_attributes.offset == 256 and opt.reserved.offset == 260
    assert dict(opt._fields_)["vote_attributes"] is C.c_uint32


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4                       # the feature is detected by the symbol


def options(point_order=1, geometry=0, merge_points=1, part_cells=0, lod_base_bits=0, mean_attributes=0, **kw):
    o = native.EncodeVoteOptions()
    native.lib().dsa_encode_default_vote_options(C.byref(o))
    m = o.mean.lod.cell_parts.split.merge
    m.order.point_order, m.merge_points, o.mean.lod.cell_parts.part_cells, o.mean.lod.lod_base_bits, o.mean.mean_attributes = point_order, merge_points, part_cells, lod_base_bits, mean_attributes
    if geometry is not None:
        m.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_mean_call():
    L = native.lib()
    vo, mo = native.EncodeVoteOptions(), native.EncodeMeanOptions()
    C.memset(C.byref(vo), 0xFF, C.sizeof(vo))
    L.dsa_encode_default_vote_options(C.byref(vo))
    L.dsa_encode_default_mean_options(C.byref(mo))
    assert bytes(vo.mean) == bytes(mo) and vo.vote_attributes == 0 and list(vo.reserved) == [0] * 7
    L.dsa_encode_default_vote_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_vote_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    refused(options(merge_points=0, vote_attributes=2), "vote_attributes without merge_points")
    refused(options(merge_points=0, point_order=0, vote_attributes=2), "vote_attributes without merge_points and point_order")
    refused(options(point_order=0, vote_attributes=2), "vote_attributes with merge_points, without point_order")
    refused(options(geometry=1, vote_attributes=2), "vote_attributes with geometry 1")
    refused(options(geometry=None, vote_attributes=2), "vote_attributes with the default geometry (meshes)")
    for bit in range(native.MAX_ATTRIBUTES, 32):
        refused(options(vote_attributes=1 << bit), "a bit at or above DSA_MAX_ATTRIBUTES")
    refused(options(vote_attributes=0xFFFFFFFF), "every bit")
    refused(options(vote_attributes=0b110, mean_attributes=0b100), "a bit in both masks")
    for k in range(7):
        o = options(vote_attributes=2)
        o.reserved[k] = 1
        refused(o, "reserved")
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved, no mask")
    # what the nested calls refuse, through this one
    refused(options(lod_base_bits=-1, part_cells=5, vote_attributes=2), "lod_base_bits")
    refused(options(lod_base_bits=3, vote_attributes=2), "lod_base_bits without part_cells")
    refused(options(part_cells=-1, vote_attributes=2), "part_cells")
    refused(options(merge_points=2, vote_attributes=2), "merge_points")
    refused(options(mean_attributes=1 << 20, vote_attributes=2), "mean_attributes")
    o = options(vote_attributes=2)
    o.mean.reserved[2] = 1
    refused(o, "mean.reserved")
    o = options(vote_attributes=2)
    o.mean.lod.cell_parts.split.part_points = 7
    refused(o, "part_points")
    # valid options get as far as the missing context: with a mask, with both masks, and with mask 0 on the mean path
    refused(options(vote_attributes=2), "no context")
    refused(options(vote_attributes=0xFF00, mean_attributes=0x00FE, part_cells=5, lod_base_bits=3), "no context, every legal bit between the two masks, parts and levels")
    refused(options(mean_attributes=2), "no context, no vote")
    refused(options(), "no context, no mask")
    assert L.dsa_encode_vote_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeVoteOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeMeanOptions Mean", "public uint VoteAttributes", "public fixed int Reserved[7]"]
    h = re.search(r"typedef struct dsa_encode_vote_options \{(.*?)\} dsa_encode_vote_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_mean_options mean", "uint32_t vote_attributes", "int32_t reserved[7]"]
    for name in ("dsa_encode_default_vote_options(out DsaEncodeVoteOptions options)",
                 "dsa_encode_vote_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeVoteOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public uint VoteAttributes", "dsa_encode_vote_sequential_batch", "vo.VoteAttributes = VoteAttributes", "vo.Mean.MeanAttributes = MeanAttributes",
                 "vo.Mean.Lod.LodBaseBits = LodBaseBits", "vo.Mean.Lod.CellParts.PartCells = PartCells", "vo.Mean.Lod.CellParts.Split.Merge = mo", "VoteAttributes needs MergePoints 1"):
        assert word in enc
    # what the header says is not built, in the comment of the vote call; the mean call no longer lists the vote there
    comment = header[header.index("dsa_encode_mean_sequential_batch with the most frequent value"):header.index("typedef struct dsa_encode_vote_options")]
    for word in ("tuples of 3 or 4 components", "a vote over normals", "weighted votes", "votes per coarser lod cell", "the winning count or", "votes without the merge"):
        assert word in comment[comment.index("Not built:"):], word
    mean = header[header.index("dsa_encode_lod_sequential_batch with the mean of every cell"):header.index("typedef struct dsa_encode_mean_options")]
    not_built = mean[mean.index("Not built:"):mean.index("Built since")]
    assert "vote" not in not_built and "weighted means" in not_built


def test_config_switch():
    assert dsa.Config().vote_attributes == 0
    base = dict(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    assert dsa.Config(vote_attributes=0b110, **base).vote_attributes == 6
    assert dsa.Config(vote_attributes=[1, 2], **base).vote_attributes == 6 and dsa.Config(vote_attributes=(15,), **base).vote_attributes == 1 << 15
    assert dsa.Config(vote_attributes=[], **base).vote_attributes == 0
    for bad, text in ((1 << 16, "a bit at or above 16"), ([16], "a bit at or above 16"), (-1, "a bit at or above 16"), (1, "positions"), ([0, 3], "positions"),
                      ("all", "a mask or a list"), ([-1], "indices of the stream"), ([1.5], "indices of the stream")):
        with pytest.raises(ValueError, match=text):
            dsa.Config(vote_attributes=bad, **base)
    for kw in (dict(point_order=dsa.POINT_ORDER_MORTON, encoding_method=0), dict(encoding_method=0), dict()):
        with pytest.raises(ValueError, match="vote_attributes.*merge_points=MERGE_CELLS"):
            dsa.Config(vote_attributes=2, **kw)
    for mean in (0b110, [2], "all"):
        with pytest.raises(ValueError, match="vote_attributes.*mean_attributes.*not both"):
            dsa.Config(vote_attributes=0b100, mean_attributes=mean, **base)
    cfg = dsa.Config(vote_attributes=[2, 4], mean_attributes=[1], part_cells=4096, lod_base_bits=9, position_bits=13, **base)
    pos = np.zeros((4, 3), np.float32)
    o = cfg._native_vote(0, [dsa.PointCloudData(pos)])
    assert o.vote_attributes == 0b10100 and o.mean.mean_attributes == 0b10 and list(o.reserved) == [0] * 7 and o.mean.lod.lod_base_bits == 9 and o.mean.lod.cell_parts.part_cells == 4096
    m = o.mean.lod.cell_parts.split.merge
    assert m.merge_points == 1 and m.order.point_order == 1 and m.order.sequential.geometry == 0 and m.order.sequential.base.position_bits == 13
    # one mask for the call: its clouds have the same attributes
    colour = dsa.Attribute(np.zeros((4, 3), np.uint8))
    plain = dsa.PointCloudData(pos, texcoords=np.zeros((4, 2), np.float32), attributes=[colour])
    with_normals = dsa.PointCloudData(pos, normals=np.ones((4, 3), np.float32), attributes=[colour])
    assert cfg._native_vote(0, [plain, plain]).vote_attributes == 0b10100
    with pytest.raises(ValueError, match="same attributes"):
        cfg._native_vote(0, [plain, with_normals])


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
    mesh, cloud = dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32)), dsa.PointCloudData(pos, attributes=[label, colour])
    base = dict(point_order=1, merge_points=1, encoding_method=0)
    # the calls without the option keep arriving where they always did
    enc.EncodeBatch([cloud], dsa.Config(), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(**base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(part_cells=2, **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(part_cells=2, lod_base_bits=3, **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(mean_attributes=[2], **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(mean_attributes=[2], vote_attributes=0, **base), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_merged_sequential_batch", "dsa_encode_cell_parts_sequential_batch",
                                       "dsa_encode_lod_sequential_batch", "dsa_encode_mean_sequential_batch", "dsa_encode_mean_sequential_batch"]
    del r.calls[:]
    for cfg, want in ((dsa.Config(vote_attributes=2, **base), (2, 0, 0, 0)), (dsa.Config(vote_attributes=[1], mean_attributes=[2], part_cells=2, **base), (2, 4, 2, 0)),
                      (dsa.Config(vote_attributes=[1], part_cells=2, lod_base_bits=3, **base), (2, 0, 2, 3))):
        enc.EncodeBatch([cloud, cloud], cfg, handle=True)
        assert [c[0] for c in r.calls] == ["dsa_encode_vote_sequential_batch"]
        _, n, _, grids, opt, _ = r.calls[0][1]
        o = opt._obj
        assert n == 2 and grids is None and (o.vote_attributes, o.mean.mean_attributes, o.mean.lod.cell_parts.part_cells, o.mean.lod.lod_base_bits) == want
        m = o.mean.lod.cell_parts.split.merge
        assert m.merge_points == 1 and m.order.point_order == 1 and m.order.sequential.geometry == 0
        del r.calls[:]
    with pytest.raises(ValueError, match="takes point clouds"):
        enc.EncodeBatch([mesh], dsa.Config(vote_attributes=2, **base), handle=True)
    with pytest.raises(ValueError, match="same attributes"):
        enc.EncodeBatch([cloud, dsa.PointCloudData(pos, attributes=[label])], dsa.Config(vote_attributes=2, **base), handle=True)
    assert not r.calls
