"""dsa_encode_normal_mean_sequential_batch (the mean normal of every cell of merged point clouds, on the device): the ctypes mirror
and the C# declaration of its struct against the header as a C compiler lays it out, the defaults, the exports in every layer, every
option the call refuses before anything is touched, mean_normals = 0 reaching the vote path, the errors of Config and how it routes,
the words of the header.  No GPU needed (the texts of the refusals need a context to be read from:
tests/test_gpu_encode_normal_means.py asserts them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("vote", "mean_normals", "reserved")
SYMBOLS = ("dsa_encode_default_normal_mean_options", "dsa_encode_normal_mean_sequential_batch")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_normal_mean_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_normal_mean_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu %zu %zu %zu %zu %zu %d", sizeof(dsa_encode_vote_options), sizeof(dsa_encode_mean_options), sizeof(dsa_encode_lod_options), sizeof(dsa_encode_cell_parts_options), sizeof(dsa_part_info), sizeof(dsa_lod_info), DSA_MAX_ATTRIBUTES);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt = native.EncodeNormalMeanOptions
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS)
    assert got == [C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [288, 256, 224, 192, 80, 48, native.MAX_ATTRIBUTES]       # (the existing structs stay)
    assert C.sizeof(opt) == C.sizeof(native.EncodeVoteOptions) + 32 == 320 and opt.mean_normals.offset == 288 and opt.reserved.offset == 292
    assert dict(opt._fields_)["mean_normals"] is C.c_uint32 and dict(opt._fields_)["vote"] is native.EncodeVoteOptions


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4                       # the feature is detected by the symbol


def options(point_order=1, geometry=0, merge_points=1, part_cells=0, lod_base_bits=0, mean_attributes=0, vote_attributes=0, **kw):
    o = native.EncodeNormalMeanOptions()
    native.lib().dsa_encode_default_normal_mean_options(C.byref(o))
    m = o.vote.mean.lod.cell_parts.split.merge
    m.order.point_order, m.merge_points = point_order, merge_points
    o.vote.mean.lod.cell_parts.part_cells, o.vote.mean.lod.lod_base_bits, o.vote.mean.mean_attributes, o.vote.vote_attributes = part_cells, lod_base_bits, mean_attributes, vote_attributes
    if geometry is not None:
        m.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_vote_call():
    L = native.lib()
    no, vo = native.EncodeNormalMeanOptions(), native.EncodeVoteOptions()
    C.memset(C.byref(no), 0xFF, C.sizeof(no))
    L.dsa_encode_default_normal_mean_options(C.byref(no))
    L.dsa_encode_default_vote_options(C.byref(vo))
    assert bytes(no.vote) == bytes(vo) and no.mean_normals == 0 and list(no.reserved) == [0] * 7
    L.dsa_encode_default_normal_mean_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_normal_mean_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    refused(options(merge_points=0, mean_normals=1), "mean_normals without merge_points")
    refused(options(merge_points=0, point_order=0, mean_normals=1), "mean_normals without merge_points and point_order")
    refused(options(point_order=0, mean_normals=1), "mean_normals with merge_points, without point_order")
    refused(options(geometry=1, mean_normals=1), "mean_normals with geometry 1")
    refused(options(geometry=None, mean_normals=1), "mean_normals with the default geometry (meshes)")
    for value in (2, 3, 1 << 16, 0xFFFFFFFF):
        refused(options(mean_normals=value), "mean_normals above 1")
    for k in range(7):
        o = options(mean_normals=1)
        o.reserved[k] = 1
        refused(o, "reserved")
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved, mean_normals 0")
    # what the nested calls refuse, through this one
    refused(options(lod_base_bits=-1, part_cells=5, mean_normals=1), "lod_base_bits")
    refused(options(lod_base_bits=3, mean_normals=1), "lod_base_bits without part_cells")
    refused(options(part_cells=-1, mean_normals=1), "part_cells")
    refused(options(merge_points=2, mean_normals=1), "merge_points")
    refused(options(mean_attributes=1 << 20, mean_normals=1), "mean_attributes")
    refused(options(vote_attributes=1 << 20, mean_normals=1), "vote_attributes")
    refused(options(vote_attributes=0b110, mean_attributes=0b100, mean_normals=1), "a bit in both masks")
    o = options(mean_normals=1)
    o.vote.reserved[2] = 1
    refused(o, "vote.reserved")
    o = options(mean_normals=1)
    o.vote.mean.reserved[0] = 1
    refused(o, "vote.mean.reserved")
    o = options(mean_normals=1)
    o.vote.mean.lod.cell_parts.split.part_points = 7
    refused(o, "part_points")
    # valid options get as far as the missing context: with the option, with it beside both masks, parts and levels, and without it
    refused(options(mean_normals=1), "no context")
    refused(options(mean_normals=1, vote_attributes=0xFF00, mean_attributes=0x00FC, part_cells=5, lod_base_bits=3), "no context, both masks, parts and levels")
    refused(options(vote_attributes=4), "no context, no mean normals")
    refused(options(), "no context, nothing asked")
    assert L.dsa_encode_normal_mean_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeNormalMeanOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeVoteOptions Vote", "public uint MeanNormals", "public fixed int Reserved[7]"]
    h = re.search(r"typedef struct dsa_encode_normal_mean_options \{(.*?)\} dsa_encode_normal_mean_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_vote_options vote", "uint32_t mean_normals", "int32_t reserved[7]"]
    for name in ("dsa_encode_default_normal_mean_options(out DsaEncodeNormalMeanOptions options)",
                 "dsa_encode_normal_mean_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeNormalMeanOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public bool MeanNormals", "dsa_encode_normal_mean_sequential_batch", "no.MeanNormals = 1", "no.Vote.VoteAttributes = VoteAttributes", "no.Vote.Mean.MeanAttributes = MeanAttributes",
                 "no.Vote.Mean.Lod.LodBaseBits = LodBaseBits", "no.Vote.Mean.Lod.CellParts.PartCells = PartCells", "no.Vote.Mean.Lod.CellParts.Split.Merge = mo", "MeanNormals needs MergePoints 1"):
        assert word in enc
    assert enc.count("if (MeanNormals)") == 2 and enc.index("if (MeanNormals)") < enc.index("else if (VoteAttributes != 0)")      # the widest call first, in both places


def test_the_words_of_the_header():
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    # the mean call: mean normals moved from "Not built" to "Built since"
    mean = header[header.index("dsa_encode_lod_sequential_batch with the mean of every cell"):header.index("typedef struct dsa_encode_mean_options")]
    not_built, since = mean[mean.index("Not built:"):mean.index("Built since")], mean[mean.index("Built since"):]
    assert "mean normals" not in not_built and "weighted means" in not_built and "means per coarser lod cell" in not_built
    assert "mean normals" in since and "dsa_encode_normal_mean_sequential_batch" in since and "a vote for label attributes" in since
    # the new call: the rule and what is still not built
    comment = header[header.index("dsa_encode_vote_sequential_batch with the mean normal of every cell"):header.index("typedef struct dsa_encode_normal_mean_options")]
    for word in ("rdiv(num, den) = floor((2 num + den) / (2 den))", "isqrt", "<< 42", "<< 24", "sg(0) = +1", "A = 0", "a cell of one row keeps its code", "mean_normals = 0",
                 "merge_points = 1", "DSA_ERR_INVALID_ARGUMENT", "k_enc_normal_sum", "k_enc_normal_store"):
        assert word in comment, word
    for word in ("a vote over normals", "weighted means", "means per coarser lod cell", "mean normals of meshes"):
        assert word in comment[comment.index("Not built:"):], word


def test_config_switch():
    assert dsa.Config().mean_normals is False
    base = dict(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    assert dsa.Config(mean_normals=True, **base).mean_normals is True and dsa.Config(mean_normals=1, **base).mean_normals is True
    assert dsa.Config(mean_normals=False, **base).mean_normals is False and dsa.Config(mean_normals=0, **base).mean_normals is False
    for bad in (2, -1, "yes", None, [1]):
        with pytest.raises(ValueError, match="mean_normals.*False or True"):
            dsa.Config(mean_normals=bad, **base)
    for kw in (dict(point_order=dsa.POINT_ORDER_MORTON, encoding_method=0), dict(encoding_method=0), dict()):
        with pytest.raises(ValueError, match="mean_normals.*merge_points=MERGE_CELLS"):
            dsa.Config(mean_normals=True, **kw)
    # a mask on the normals is none of this option's business: the masks keep their own rules
    cfg = dsa.Config(mean_normals=True, vote_attributes=[3], mean_attributes=[2], part_cells=4096, lod_base_bits=9, position_bits=13, normal_bits=11, **base)
    pos = np.zeros((4, 3), np.float32)
    nrm = np.ones((4, 3), np.float32)
    colour, label = dsa.Attribute(np.zeros((4, 3), np.uint8)), dsa.Attribute(np.zeros((4, 1), np.uint8))
    cloud = dsa.PointCloudData(pos, normals=nrm, attributes=[colour, label])
    o = cfg._native_normal_mean(0, [cloud])
    assert o.mean_normals == 1 and list(o.reserved) == [0] * 7 and o.vote.vote_attributes == 0b1000 and o.vote.mean.mean_attributes == 0b100
    assert o.vote.mean.lod.lod_base_bits == 9 and o.vote.mean.lod.cell_parts.part_cells == 4096
    m = o.vote.mean.lod.cell_parts.split.merge
    assert m.merge_points == 1 and m.order.point_order == 1 and m.order.sequential.geometry == 0 and m.order.sequential.base.position_bits == 13 and m.order.sequential.base.normal_bits == 11
    # without a mask the clouds of a call need not have the same attributes: one has normals, one has none
    plain = dsa.Config(mean_normals=True, **base)
    o = plain._native_normal_mean(0, [cloud, dsa.PointCloudData(pos)])
    assert o.mean_normals == 1 and o.vote.vote_attributes == 0 and o.vote.mean.mean_attributes == 0
    with pytest.raises(ValueError, match="same attributes"):
        cfg._native_normal_mean(0, [cloud, dsa.PointCloudData(pos, attributes=[colour, label])])


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
    mesh = dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32))
    cloud, bare = dsa.PointCloudData(pos, normals=np.ones((4, 3), np.float32), attributes=[label, colour]), dsa.PointCloudData(pos)
    base = dict(point_order=1, merge_points=1, encoding_method=0)
    # the calls without the option keep arriving where they always did
    enc.EncodeBatch([cloud], dsa.Config(), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(**base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(part_cells=2, **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(part_cells=2, lod_base_bits=3, **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(mean_attributes=[3], **base), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(vote_attributes=[2], mean_normals=False, **base), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_merged_sequential_batch", "dsa_encode_cell_parts_sequential_batch",
                                       "dsa_encode_lod_sequential_batch", "dsa_encode_mean_sequential_batch", "dsa_encode_vote_sequential_batch"]
    del r.calls[:]
    for cfg, clouds, want in ((dsa.Config(mean_normals=True, **base), [cloud, bare], (0, 0, 0, 0)), (dsa.Config(mean_normals=True, vote_attributes=[2], mean_attributes=[3], part_cells=2, **base), [cloud, cloud], (4, 8, 2, 0)),
                              (dsa.Config(mean_normals=True, part_cells=2, lod_base_bits=3, **base), [bare, cloud], (0, 0, 2, 3))):
        enc.EncodeBatch(clouds, cfg, handle=True)
        assert [c[0] for c in r.calls] == ["dsa_encode_normal_mean_sequential_batch"]
        _, n, _, grids, opt, _ = r.calls[0][1]
        o = opt._obj
        assert n == 2 and grids is None and o.mean_normals == 1
        assert (o.vote.vote_attributes, o.vote.mean.mean_attributes, o.vote.mean.lod.cell_parts.part_cells, o.vote.mean.lod.lod_base_bits) == want
        m = o.vote.mean.lod.cell_parts.split.merge
        assert m.merge_points == 1 and m.order.point_order == 1 and m.order.sequential.geometry == 0
        del r.calls[:]
    with pytest.raises(ValueError, match="takes point clouds"):
        enc.EncodeBatch([mesh], dsa.Config(mean_normals=True, **base), handle=True)
    with pytest.raises(ValueError, match="same attributes"):
        enc.EncodeBatch([cloud, bare], dsa.Config(mean_normals=True, vote_attributes=[2], **base), handle=True)
