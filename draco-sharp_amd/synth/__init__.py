"""Synthetic inputs: procedural meshes and a CPU writer of Draco v2.2 streams
(ctypes binding of libdsa_synth.so).  Used by tests and bench.py to make .drc
inputs; not part of the decode path."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_DIR, "libdsa_synth.so")

GRID, TORUS, SPHERE, HOLES, TWO_PARTS = 0, 1, 2, 3, 4


class Options(C.Structure):
    _fields_ = [("pos_bits", C.c_int32), ("uv_bits", C.c_int32), ("normal_bits", C.c_int32),
                ("single_connectivity", C.c_int32), ("force_scheme", C.c_int32),
                ("compression_level", C.c_int32), ("pos_prediction", C.c_int32), ("uv_prediction", C.c_int32),
                ("normal_prediction", C.c_int32), ("traversal_method", C.c_int32), ("predictive_connectivity", C.c_int32),
                ("normal_transform", C.c_int32), ("raw_integers", C.c_int32), ("no_prediction", C.c_int32),
                ("generic_components", C.c_int32), ("generic_data_type", C.c_int32), ("repair_topology", C.c_int32)]


# element types of the generic attribute (CPU coder only): numpy dtype -> Draco's data type id
GENERIC_DATA_TYPES = {np.dtype(np.int8): 1, np.dtype(np.uint8): 2, np.dtype(np.int16): 3, np.dtype(np.uint16): 4,
                      np.dtype(np.int32): 5, np.dtype(np.uint32): 6}


FLOAT32_DATA_TYPE = 9
UNIQUE_ID_DEFAULT = 0xFFFFFFFF


class ExtraInput(C.Structure):
    """synth_extra: one more per-vertex attribute behind the built-in ones."""
    _fields_ = [("attribute_type", C.c_int32), ("data_type", C.c_int32), ("num_components", C.c_uint32), ("normalized", C.c_int32),
                ("unique_id", C.c_uint32), ("quantization_bits", C.c_int32), ("values", C.c_void_p)]


class ExtraCornersInput(C.Structure):
    """synth_extra_corners: row ids per corner for one attribute of an ExtraInput list (corners NULL: one row per vertex)."""
    _fields_ = [("corners", C.c_void_p), ("num_rows", C.c_uint32), ("reserved", C.c_uint32)]


class Grid(C.Structure):
    """A quantisation grid given by the caller (dsa_quantization_grid): mode 0 the attribute's own bounds, 1 explicit."""
    _fields_ = [("origin", C.c_float * 4), ("range", C.c_float), ("mode", C.c_int32), ("reserved", C.c_uint32 * 2)]


class GridsInput(C.Structure):
    """synth_grids: the grids of the positions, the first UV set and the extras of one mesh."""
    _fields_ = [("position", Grid), ("texcoord", Grid), ("attributes", C.POINTER(Grid))]


def grid(origin, range, mode=1):
    """An explicit grid: origin per component (1 - 4 floats) and one range."""
    g = Grid()
    o = np.asarray(origin, np.float32).ravel()
    if not 1 <= len(o) <= 4:
        raise ValueError("a grid has 1 to 4 origin components")
    for c, x in enumerate(o):
        g.origin[c] = x
    g.range, g.mode = np.float32(range), mode
    return g


def shared_grid(arrays):
    """The grid a group of meshes shares for one attribute slot (mode 2 of the device encoder), as an explicit grid: minimum per
    component over all rows of every array (N, nc) whose values are all finite, range the largest extent, 1 if that is 0."""
    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    arrays = [a.reshape(len(a), -1) for a in arrays]
    if not arrays or any(a.shape[1] != arrays[0].shape[1] for a in arrays):
        raise ValueError("shared_grid: arrays of one component count")
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    rows = (C.c_uint32 * len(arrays))(*[len(a) for a in arrays])
    g = Grid()
    L = lib()
    if L.synth_shared_grid(ptrs, rows, len(arrays), arrays[0].shape[1], C.byref(g)):
        raise RuntimeError(_err())
    return g


class Extra:
    """One more per-vertex attribute for the `extra=[...]` of the encode calls: values (V,) or (V, 1..4) of int8 / uint8 / int16 /
    uint16 / int32 / uint32 (coded as they are) or float32 (quantised to quantization_bits; 0: uv_bits for attribute_type 3, else
    8).  attribute_type 2 colour, 3 texture coordinate, 4 generic; unique_id None: the attribute's index in the stream.
    data_type / num_components override what the array says (the refusal tests).
    corners: (F, 3) row ids into `values`, which then holds any number of rows -- the attribute is given per corner, and an interior
    edge across which the ids differ is a seam of this attribute alone (Edgebreaker streams; the attribute's index in the stream must
    be at most 7).  rows overrides the row count the ids are held against (the refusal tests).
    portable: float32 values, encode_grid(form=0): int32 (V, nc) coded in place of the quantiser's output, bounds and grid untouched."""

    def __init__(self, values, attribute_type=4, normalized=False, unique_id=None, quantization_bits=0, data_type=None, num_components=None, grid=None,
                 corners=None, rows=None, portable=None):
        self.grid = grid                      # float32: a Grid (encode_grid), None: its own bounds
        self.portable = None if portable is None else np.ascontiguousarray(portable, np.int32).reshape(len(portable), -1)
        self.corners = None if corners is None else np.ascontiguousarray(corners, np.uint32)
        v = np.asarray(values)
        if v.dtype not in GENERIC_DATA_TYPES and v.dtype != np.dtype(np.float32):
            raise ValueError("extra attribute: dtype %s is none of int8 ... uint32, float32" % v.dtype)
        v = np.ascontiguousarray(v)
        self.values = v.reshape(len(v), -1)
        self.attribute_type = attribute_type
        self.data_type = (GENERIC_DATA_TYPES.get(v.dtype, FLOAT32_DATA_TYPE)) if data_type is None else data_type
        self.num_components = self.values.shape[1] if num_components is None else num_components
        self.normalized = int(normalized)
        self.unique_id = UNIQUE_ID_DEFAULT if unique_id is None else unique_id
        self.quantization_bits = quantization_bits
        self.rows = len(self.values) if rows is None else rows


def _extra_corners(extra, nf):
    """The synth_extra_corners array of a list of Extra, None when none of them has ids."""
    if not any(e.corners is not None for e in extra):
        return None
    arr = (ExtraCornersInput * max(1, len(extra)))()
    for k, e in enumerate(extra):
        if e.corners is None:
            continue
        if e.corners.size != 3 * nf:
            raise ValueError("extra attribute %d: one id per corner of `faces`" % k)
        arr[k].corners, arr[k].num_rows = e.corners.ctypes.data, e.rows
    return arr


def _extras(extra, nv):
    """The synth_extra array of a list of Extra; the Extras own the value arrays, keep them beside it."""
    arr = (ExtraInput * max(1, len(extra)))()
    for k, e in enumerate(extra):
        if e.corners is None and len(e.values) != nv:
            raise ValueError("extra attribute %d: one row per vertex" % k)
        arr[k].attribute_type, arr[k].data_type, arr[k].num_components = e.attribute_type, e.data_type, e.num_components
        arr[k].normalized, arr[k].unique_id, arr[k].quantization_bits = e.normalized, e.unique_id, e.quantization_bits
        arr[k].values = e.values.ctypes.data
    return arr


def _encode_attributes(edgebreaker, pos, faces, nrm, nci, uv, uci, generic, geometry, compressed, extra, opt):
    """Any stream with `extra` behind the built-in attributes (synth_encode_attributes)."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    faces = None if faces is None else np.ascontiguousarray(faces, np.uint32)
    nrm = None if nrm is None else np.ascontiguousarray(nrm, np.float32)
    uv = None if uv is None else np.ascontiguousarray(uv, np.float32)
    nci = None if nci is None else np.ascontiguousarray(nci, np.uint32)
    uci = None if uci is None else np.ascontiguousarray(uci, np.uint32)
    opt = opt or options()
    gen = None
    if generic is not None:
        gen, opt = _generic(generic, opt)
        if not edgebreaker:
            gen = gen.reshape(len(gen), -1)
            if opt.generic_components != gen.shape[1]:
                o2 = Options()
                C.memmove(C.byref(o2), C.byref(opt), C.sizeof(Options))
                o2.generic_components = gen.shape[1]
                opt = o2
    extra = [e if isinstance(e, Extra) else Extra(e) for e in extra]
    arr = _extras(extra, len(pos))
    ec = _extra_corners(extra, 0 if faces is None else len(faces))
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    out, n = C.c_void_p(), C.c_size_t()
    if ec is None:
        rc = L.synth_encode_attributes(1 if edgebreaker else 0, ptr(pos), len(pos), ptr(faces), 0 if faces is None else len(faces),
                                       ptr(nrm), 0 if nrm is None else len(nrm), ptr(nci), ptr(uv), 0 if uv is None else len(uv), ptr(uci),
                                       ptr(gen), geometry, 1 if compressed else 0, arr, len(extra), C.byref(opt), C.byref(out), C.byref(n))
    else:
        rc = L.synth_encode_corner_attributes(1 if edgebreaker else 0, ptr(pos), len(pos), ptr(faces), 0 if faces is None else len(faces),
                                              ptr(nrm), 0 if nrm is None else len(nrm), ptr(nci), ptr(uv), 0 if uv is None else len(uv), ptr(uci),
                                              ptr(gen), geometry, 1 if compressed else 0, arr, ec, len(extra), C.byref(opt), C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def build(force=False):
    src = os.path.join(_DIR, "synth_encoder.cpp")
    deps = [src, os.path.join(_DIR, "..", "csrc", "dsa_encode_host.h")]
    if force or not os.path.exists(_LIB_PATH) or any(os.path.getmtime(_LIB_PATH) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["make", "-C", _DIR, "-s"])
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB_PATH)
        L.synth_last_error.restype = C.c_char_p
        L.synth_default_options.argtypes = [C.POINTER(Options)]
        L.synth_encode_mesh.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_mesh_corners.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Options), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_size_t)]
        L.synth_encode_point_cloud.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Options), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_size_t)]
        L.synth_encode_mesh_sequential.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_sequential.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_attributes.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ExtraInput), C.c_uint32,
                                              C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_corner_attributes.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ExtraInput), C.POINTER(ExtraCornersInput),
                                                     C.c_uint32, C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_weld_points_attributes.restype = C.c_void_p
        L.synth_weld_points_attributes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.POINTER(ExtraInput), C.c_uint32, C.POINTER(Options), C.c_int]
        L.synth_welded_listed.restype = C.c_uint32
        L.synth_welded_listed.argtypes = [C.c_void_p]
        L.synth_welded_listed_counts.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.synth_encode_points_attributes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(ExtraInput), C.c_uint32, C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_corner_attributes_grid.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ExtraInput), C.POINTER(ExtraCornersInput),
                                                          C.c_uint32, C.POINTER(GridsInput), C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_entry_rows.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ExtraInput), C.POINTER(ExtraCornersInput),
                                       C.c_uint32, C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.synth_weld_points.restype = C.c_void_p
        L.synth_weld_points.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(ExtraInput), C.c_uint32, C.POINTER(Options)]
        L.synth_welded_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.synth_welded_array.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_welded_free.argtypes = [C.c_void_p]
        L.synth_encode_points.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(ExtraInput), C.c_uint32, C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_grid.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(ExtraInput), C.c_uint32,
                                        C.POINTER(GridsInput), C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.synth_encode_grid_portable.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ExtraInput), C.c_uint32, C.POINTER(GridsInput),
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(Options), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        L.synth_quantized.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(Grid), C.c_void_p]
        L.synth_merge_means.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.synth_merge_votes.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.synth_merge_mean_normals.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.synth_quantized_normals.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.synth_point_order.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_void_p]
        L.synth_merge_points.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        L.synth_merge_voxels.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
        L.synth_split_parts.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.synth_part_boxes.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.synth_cell_parts.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int, C.c_int]
        L.synth_lod_parts.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Grid), C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int, C.c_int]
        L.synth_shared_grid.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.POINTER(Grid)]
        L.synth_free.argtypes = [C.c_void_p]
        L.synth_make_mesh.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.synth_make_batch.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int,
                                       C.POINTER(Options), C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
        L.synth_encode_symbols.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_size_t)]
        L.synth_encode_rabs.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def options(**kw):
    """synth_options with the given fields set.  repair_topology: 0 strict, 1 the reference's repaired corner table, 2 as 1 and
    attributes given per corner (encode_mesh_corners, encode_mesh_points, encode_grid) are coded over it (1 refuses them)."""
    o = Options()
    lib().synth_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown synth option %r" % k)
        setattr(o, k, v)
    return o


def _err():
    return lib().synth_last_error().decode()


def _generic(generic, opt):
    """The generic attribute as a contiguous array of its own integer dtype (anything else: uint8, as before) and options
    whose generic_data_type says so (a copy: the caller's options stay)."""
    gen = np.asarray(generic)
    if gen.dtype not in GENERIC_DATA_TYPES:
        gen = gen.astype(np.uint8)
    gen = np.ascontiguousarray(gen)
    dt = GENERIC_DATA_TYPES[gen.dtype]
    if opt.generic_data_type != dt:
        o2 = Options()
        C.memmove(C.byref(o2), C.byref(opt), C.sizeof(Options))
        o2.generic_data_type = dt
        opt = o2
    return gen, opt


def make_mesh(kind, nx, ny, seed):
    """Returns (pos[V,3] f32, normals[V,3] f32, uv[V,2] f32, faces[F,3] u32)."""
    L = lib()
    nv, nf = C.c_uint32(), C.c_uint32()
    if L.synth_make_mesh(kind, nx, ny, seed, C.byref(nv), C.byref(nf), None, None, None, None):
        raise RuntimeError(_err())
    pos = np.zeros((nv.value, 3), np.float32)
    nrm = np.zeros((nv.value, 3), np.float32)
    uv = np.zeros((nv.value, 2), np.float32)
    faces = np.zeros((nf.value, 3), np.uint32)
    L.synth_make_mesh(kind, nx, ny, seed, C.byref(nv), C.byref(nf), pos.ctypes.data, nrm.ctypes.data,
                      uv.ctypes.data, faces.ctypes.data)
    return pos, nrm, uv, faces


def encode_mesh(pos, faces, normals=None, uvs=None, generic=None, opt=None, extra=None):
    """extra: list of Extra (or arrays): more per-vertex attributes behind the built-in ones."""
    if extra:
        return _encode_attributes(True, pos, faces, normals, None, uvs, None, generic, 1, False, extra, opt)
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    faces = np.ascontiguousarray(faces, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32)
    out, n = C.c_void_p(), C.c_size_t()
    opt = opt or options()
    gen = None
    if generic is not None:
        gen, opt = _generic(generic, opt)
    rc = L.synth_encode_mesh(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces),
                             None if nrm is None else nrm.ctypes.data, None if uv is None else uv.ctypes.data,
                             None if gen is None else gen.ctypes.data, C.byref(opt), C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def encode_mesh_corners(pos, faces, normals=None, normal_corners=None, uvs=None, uv_corners=None, opt=None, generic=None, extra=None):
    """Mesh whose normals / texture coordinates are given per corner: `faces` [F,3] index `pos`, `normal_corners` /
    `uv_corners` [F,3] index the rows of `normals` / `uvs` (None: that attribute has one row per vertex).  Edges across
    which the ids differ become attribute seams in the stream (seam bits, attribute corner table, corner attribute).
    `generic`: the per-vertex integer attribute of encode_mesh (its components per opt.generic_components)."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    faces = np.ascontiguousarray(faces, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32)
    nci = None if normal_corners is None else np.ascontiguousarray(normal_corners, np.uint32)
    uci = None if uv_corners is None else np.ascontiguousarray(uv_corners, np.uint32)
    for ids, vals, name in ((nci, nrm, "normal"), (uci, uv, "uv")):
        if ids is not None and (vals is None or ids.shape != faces.shape):
            raise ValueError("%s_corners needs %ss and one id per corner of `faces`" % (name, name))
        if ids is None and vals is not None and len(vals) != len(pos):
            raise ValueError("per-vertex %ss need one row per vertex" % name)
    if extra:
        return _encode_attributes(True, pos, faces, nrm, nci, uv, uci, generic, 1, False, extra, opt)
    out, n = C.c_void_p(), C.c_size_t()
    opt = opt or options()
    gen = None
    if generic is not None:
        gen, opt = _generic(generic, opt)
    rc = L.synth_encode_mesh_corners(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces),
                                     None if nrm is None else nrm.ctypes.data, 0 if nrm is None else len(nrm),
                                     None if nci is None else nci.ctypes.data,
                                     None if uv is None else uv.ctypes.data, 0 if uv is None else len(uv),
                                     None if uci is None else uci.ctypes.data, None if gen is None else gen.ctypes.data,
                                     C.byref(opt), C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


class Welded:
    """What weld_points returns.  Maps (uint32; 0xFFFFFFFF for a point no face names): vertex_of_point / normal_of_point /
    texcoord_of_point [P], vertex_point [V] / normal_point [N] / texcoord_point [T] (the representative point of every class; the
    normal / texcoord maps are None when the mesh has no such attribute).  The welded mesh: pos [V,3], faces [F,3], generic and
    extra (rows of vertex_point), normals with normal_corners [F,3] (None and V rows when normals_per_vertex), uvs with
    uv_corners likewise.  weld_attributes: extra_corners[k] [F,3] / extra_of_point[k] [P] / extra_point[k] of a listed attribute
    welded alone that some vertex has two rows of (extra[k] then holds the attribute's own rows), else None."""


def _points_args(pos, faces, normals, uvs, generic, extra, opt):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
    opt = opt or options()
    gen = None
    if generic is not None:
        gen, opt = _generic(generic, opt)
        gen = gen.reshape(len(gen), -1)
        if opt.generic_components != gen.shape[1]:          # the components are the array's own (a copy: the caller's options stay)
            o2 = Options()
            C.memmove(C.byref(o2), C.byref(opt), C.sizeof(Options))
            o2.generic_components = gen.shape[1]
            opt = o2
    for a, name in ((nrm, "normals"), (uv, "uvs"), (gen, "generic")):
        if a is not None and len(a) != len(pos):
            raise ValueError("%s: one row per point" % name)
    extra = [e if isinstance(e, Extra) else Extra(e) for e in (extra or [])]
    return pos, faces, nrm, uv, gen, extra, _extras(extra, len(pos)), opt


def _no_point_ids(extra):
    if any(e.corners is not None for e in extra):
        raise ValueError("per-point input takes no corner ids")


def weld_points(pos, faces, normals=None, uvs=None, generic=None, extra=None, opt=None, weld_attributes=False):
    """The weld of a mesh given as one row per point (dsa_encode_host.h weld_points): used points with byte-equal position,
    generic and extra rows are one vertex; normals and uvs are welded each alone and handed on per corner, or per vertex where
    no vertex has two of them.  weld_attributes: every extra whose index in the stream is at most 7 leaves the vertex key and is
    welded alone like normals and uvs.  Returns a Welded."""
    L = lib()
    pos, faces, nrm, uv, gen, extra, arr, opt = _points_args(pos, faces, normals, uvs, generic, extra, opt)
    _no_point_ids(extra)
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    h = L.synth_weld_points_attributes(ptr(pos), len(pos), ptr(faces), len(faces), ptr(nrm), ptr(uv), ptr(gen), arr, len(extra), C.byref(opt),
                                       1 if weld_attributes else 0)
    if not h:
        raise RuntimeError(_err())
    try:
        counts = (C.c_uint32 * 8)()
        L.synth_welded_counts(h, counts)

        def array(which, dtype):
            data, nbytes = C.c_void_p(), C.c_size_t()
            if L.synth_welded_array(h, which, C.byref(data), C.byref(nbytes)):
                raise RuntimeError("synth_welded_array(%d)" % which)
            return np.frombuffer(C.string_at(data, nbytes.value), dtype).copy() if nbytes.value else np.zeros(0, dtype)
        w = Welded()
        w.num_points, w.num_faces, w.num_vertices, w.num_normals, w.num_texcoords = [int(c) for c in counts[:5]]
        w.normals_per_vertex, w.texcoords_per_vertex = bool(counts[5]), bool(counts[6])
        w.vertex_of_point, w.vertex_point = array(0, np.uint32), array(1, np.uint32)
        w.normal_of_point, w.normal_point = (array(2, np.uint32), array(3, np.uint32)) if nrm is not None else (None, None)
        w.texcoord_of_point, w.texcoord_point = (array(4, np.uint32), array(5, np.uint32)) if uv is not None else (None, None)
        w.faces = array(6, np.uint32).reshape(-1, 3)
        w.normal_corners = None if w.normals_per_vertex else array(7, np.uint32).reshape(-1, 3)
        w.uv_corners = None if w.texcoords_per_vertex else array(8, np.uint32).reshape(-1, 3)
        w.normals = None if nrm is None else array(9, np.float32).reshape(-1, 3)
        w.uvs = None if uv is None else array(10, np.float32).reshape(-1, 2)
        g = 16
        w.pos = array(g, np.float32).reshape(-1, 3)
        g += 1
        w.generic = None
        if gen is not None:
            w.generic = array(g, gen.dtype).reshape(-1, gen.shape[1])
            g += 1
        w.extra, w.extra_corners, w.extra_of_point, w.extra_point = [], [], [], []
        alone = int(L.synth_welded_listed(h))
        for k, e in enumerate(extra):
            if k < alone:
                lc = (C.c_uint32 * 2)()
                L.synth_welded_listed_counts(h, k, lc)
                w.extra.append(array(64 + 4 * k + 3, e.values.dtype).reshape(-1, e.values.shape[1]))
                w.extra_corners.append(None if lc[1] else array(64 + 4 * k + 2, np.uint32).reshape(-1, 3))
                w.extra_of_point.append(array(64 + 4 * k, np.uint32))
                w.extra_point.append(array(64 + 4 * k + 1, np.uint32))
                continue
            w.extra.append(array(g, e.values.dtype).reshape(-1, e.values.shape[1]))
            w.extra_corners.append(None)
            w.extra_of_point.append(None)
            w.extra_point.append(None)
            g += 1
        return w
    finally:
        L.synth_welded_free(h)


def encode_mesh_points(pos, faces, normals=None, uvs=None, generic=None, extra=None, opt=None, weld_attributes=False):
    """weld_points followed by the coder of encode_mesh_corners on the welded mesh (extra: Extras with one row per point).  What
    dsa_encode_points_batch must write; with weld_attributes what dsa_encode_corner_attributes_batch must."""
    L = lib()
    pos, faces, nrm, uv, gen, extra, arr, opt = _points_args(pos, faces, normals, uvs, generic, extra, opt)
    _no_point_ids(extra)
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.synth_encode_points_attributes(ptr(pos), len(pos), ptr(faces), len(faces), ptr(nrm), ptr(uv), ptr(gen), arr, len(extra), C.byref(opt),
                                          1 if weld_attributes else 0, C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def encode_grid(pos, faces=None, normals=None, uvs=None, generic=None, extra=None, opt=None, form=1, normal_corners=None, uv_corners=None,
                geometry=1, compressed=False, pos_grid=None, uv_grid=None, weld_attributes=False, uv_portable=None, normal_portable=None, pos_portable=None):
    """Any stream of this module with quantisation grids given by the caller: pos_grid / uv_grid / Extra.grid are Grids (grid(),
    shared_grid()) or None for the attribute's own bounds.  form 1: the arguments of encode_mesh_corners (Edgebreaker); form 0:
    of encode_sequential (geometry 1) / encode_point_cloud_attributes (geometry 0, faces None); form 2: of encode_mesh_points
    (one row per point).  Without a grid the bytes are those calls'.  What dsa_encode_grid_batch /
    dsa_encode_grid_sequential_batch must write.  uv_portable (N, 2) int32 / Extra.portable (form 0, point clouds): the integers
    coded for that quantised attribute in place of the quantiser's output, the header's bounds or grid as the floats give them;
    normal_portable (N, 2) int32 likewise: the octahedral codes (s, t) coded for the normals; pos_portable (N, 3) int32 likewise: the
    integers coded for the positions (the voxel centroids of dsa_encode_voxel_sequential_batch)."""
    L = lib()
    pos, fc, nrm, uv, gen, extra, arr, opt = _points_args(pos, np.zeros((0, 3), np.uint32) if faces is None else faces, normals if normal_corners is None else None,
                                                          uvs if uv_corners is None else None, generic, extra, opt)
    if normal_corners is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if uv_corners is not None:
        uv = np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
    nci = None if normal_corners is None else np.ascontiguousarray(normal_corners, np.uint32)
    uci = None if uv_corners is None else np.ascontiguousarray(uv_corners, np.uint32)
    gi = GridsInput()
    if pos_grid is not None:
        gi.position = pos_grid
    if uv_grid is not None:
        gi.texcoord = uv_grid
    ga = (Grid * max(1, len(extra)))()
    for k, e in enumerate(extra):
        if e.grid is not None:
            ga[k] = e.grid
    gi.attributes = ga
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    out, n = C.c_void_p(), C.c_size_t()
    ec = _extra_corners(extra, len(fc))
    if normal_portable is not None and nrm is None:
        raise ValueError("normal_portable goes with normals")
    if uv_portable is not None or normal_portable is not None or pos_portable is not None or any(e.portable is not None for e in extra):
        if form != 0 or geometry != 0 or len(fc) or ec is not None:
            raise ValueError("portable integers go with a point cloud (form 0, geometry 0)")
        up = None if uv_portable is None else np.ascontiguousarray(uv_portable, np.int32).reshape(len(pos), 2)
        for k, e in enumerate(extra):
            if e.portable is not None and e.portable.shape != (len(pos), e.num_components):
                raise ValueError("extra attribute %d: portable holds one row of num_components integers per point" % k)
        ep = (C.c_void_p * max(1, len(extra)))(*[None if e.portable is None else e.portable.ctypes.data for e in extra])
        npt = None if normal_portable is None else np.ascontiguousarray(normal_portable, np.int32).reshape(len(pos), 2)
        ppt = None if pos_portable is None else np.ascontiguousarray(pos_portable, np.int32).reshape(len(pos), 3)
        rc = L.synth_encode_grid_portable(ptr(pos), len(pos), ptr(nrm), ptr(uv), ptr(gen), arr, len(extra), C.byref(gi), ptr(npt), ptr(up), ep, C.byref(opt),
                                          C.byref(out), C.byref(n), ptr(ppt))
    elif ec is None and not weld_attributes:
        rc = L.synth_encode_grid(form, ptr(pos), len(pos), ptr(fc) if len(fc) else None, len(fc), ptr(nrm), 0 if nrm is None else len(nrm), ptr(nci),
                                 ptr(uv), 0 if uv is None else len(uv), ptr(uci), ptr(gen), geometry, 1 if compressed else 0, arr, len(extra),
                                 C.byref(gi), C.byref(opt), C.byref(out), C.byref(n))
    else:
        rc = L.synth_encode_corner_attributes_grid(form, ptr(pos), len(pos), ptr(fc) if len(fc) else None, len(fc), ptr(nrm), 0 if nrm is None else len(nrm),
                                                   ptr(nci), ptr(uv), 0 if uv is None else len(uv), ptr(uci), ptr(gen), geometry, 1 if compressed else 0,
                                                   arr, ec, len(extra), C.byref(gi), C.byref(opt), 1 if weld_attributes else 0, C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def point_order(pos, bits, grid=None):
    """The Morton order of the points `pos` (N, 3) at `bits` position bits: uint32 perm, the rows in ascending (key, row) with
    key = the bits of the quantised x, y, z interleaved, x the top bit of every triple.  Quantised as the coder does it: on the
    positions' own bounds, or on `grid` (grid(), shared_grid()).  The order of dsa_encode_ordered_sequential_batch, point_order = 1."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    perm = np.zeros(len(pos), np.uint32)
    if L.synth_point_order(pos.ctypes.data, len(pos), int(bits), None if grid is None else C.byref(grid), perm.ctypes.data):
        raise RuntimeError(_err())
    return perm


def encode_ordered(pos, faces=None, normals=None, uvs=None, generic=None, extra=None, opt=None, geometry=1, compressed=False,
                   pos_grid=None, uv_grid=None):
    """encode_grid with form=0 for the input in Morton order: (stream, perm) with perm = point_order(pos, opt.pos_bits, pos_grid),
    every per-point array taken at [perm] and the faces through the inverse of perm.  What
    dsa_encode_ordered_sequential_batch with point_order = 1 must write, and the rows its handle must report.  (One difference, by
    design: an attribute on its own bounds whose minimum is attained by a -0.0 and a +0.0 gets the sign of the first of them in
    the order coded here, the device that of the first in the caller's order -- its bounds are the caller's rows', as in every
    split or merged call; bounds_grid of the caller's array as an explicit grid gives the device's header.)"""
    opt = opt or options()
    perm = point_order(pos, opt.pos_bits, pos_grid)
    take = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a).reshape(len(perm), -1)[perm])      # noqa: E731
    ex = []
    for e in (extra or []):
        e = e if isinstance(e, Extra) else Extra(e)
        ex.append(Extra(e.values[perm], attribute_type=e.attribute_type, normalized=bool(e.normalized), unique_id=e.unique_id,
                        quantization_bits=e.quantization_bits, data_type=e.data_type, num_components=e.num_components, grid=e.grid))
    fc = None
    if faces is not None:
        rank = np.zeros(len(perm), np.uint32)
        rank[perm] = np.arange(len(perm), dtype=np.uint32)
        fc = rank[np.ascontiguousarray(faces, np.uint32)]
    gen = None if generic is None else (np.asarray(generic)[perm])
    data = encode_grid(take(pos), fc, take(normals), take(uvs), gen, ex, opt, form=0, geometry=geometry, compressed=compressed,
                       pos_grid=pos_grid, uv_grid=uv_grid)
    return data, perm


VOXEL_POINT_FIRST, VOXEL_POINT_CENTROID, VOXEL_POINT_NEAREST = 0, 1, 2


def merge_voxels(pos, bits, grid=None, voxel_bits=0, voxel_point=0):
    """merge_points over the cells of the grid with voxel_bits = C bits per axis (0: the position cells): (kept, row_entries, coded).
    The voxel of a row is its key without the low 3 (bits - C) bits; entry e of the sorted order is a head iff e == 0 or its voxel
    differs from that of entry e - 1.  voxel_point 0: kept[j] the voxel's first row in (key, row) order; 1 (centroid): that row,
    its position integers floor((2 S + cnt) / (2 cnt)) per component over the voxel's rows; 2 (nearest): the row with the smallest
    (dist, row), dist the squared distance from the voxel's centre in doubled coordinates.  coded (N, 3) int32: the integers the
    position stream codes for every row -- the quantiser's output, the centroids at the kept rows.  What
    dsa_encode_voxel_sequential_batch keeps."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    kept = np.zeros(len(pos), np.uint32)
    cells = np.zeros(len(pos), np.uint32)
    coded = np.zeros((len(pos), 3), np.int32)
    m = C.c_uint32()
    if L.synth_merge_voxels(pos.ctypes.data, len(pos), int(bits), None if grid is None else C.byref(grid), int(voxel_bits), int(voxel_point), kept.ctypes.data,
                            C.byref(m), cells.ctypes.data, coded.ctypes.data):
        raise RuntimeError(_err())
    return kept[:m.value].copy(), cells, coded


def merge_points(pos, bits, grid=None):
    """One point per occupied cell of the position grid: (kept, row_entries) for the points `pos` (N, 3) at `bits` position bits,
    quantised as point_order quantises them.  With perm = point_order(pos, bits, grid) and key the interleaved bits, entry e is a
    head iff e == 0 or key[perm[e]] != key[perm[e - 1]]; kept (uint32, m) lists perm[e] over the heads in sorted order -- the
    smallest row of every cell, with voxel_bits = 0 -- and row_entries (uint32, N) holds for every row the index in kept of its cell.  What
    dsa_encode_merged_sequential_batch with merge_points = 1 keeps."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    kept = np.zeros(len(pos), np.uint32)
    cells = np.zeros(len(pos), np.uint32)
    m = C.c_uint32()
    if L.synth_merge_points(pos.ctypes.data, len(pos), int(bits), None if grid is None else C.byref(grid), kept.ctypes.data, C.byref(m), cells.ctypes.data):
        raise RuntimeError(_err())
    return kept[:m.value].copy(), cells


def bounds_grid(values):
    """The explicit grid equal to the own bounds of `values` (N, nc) float32: origin the minimum per component, range the largest
    extent in float32 arithmetic, 1 where that is 0 -- what the coder finds for an attribute without a grid."""
    v = np.ascontiguousarray(values, np.float32)
    v = v.reshape(len(v), -1)
    # (the minimum of a component is the value of the first row that attains it, as the coder's serial compare leaves it: that
    # decides the sign of a zero minimum, which np.min does not define)
    mn = np.array([col[np.flatnonzero(col == col.min())[0]] for col in v.T], np.float32)
    rng = np.float32(np.max((v.max(axis=0) - mn).astype(np.float32)))
    return grid(mn, rng if rng != 0 else np.float32(1.0))


def quantized(values, bits, grid=None):
    """The integers (N, nc) int32 the coder quantises `values` (N, nc) float32 to at `bits` bits: on their own bounds, or on `grid`."""
    L = lib()
    v = np.ascontiguousarray(values, np.float32)
    v = v.reshape(len(v), -1)
    out = np.zeros(v.shape, np.int32)
    if L.synth_quantized(v.ctypes.data, len(v), v.shape[1], int(bits), None if grid is None else C.byref(grid), out.ctypes.data):
        raise RuntimeError(_err())
    return out


def merge_means(q, row_entries, m):
    """The mean of every cell: q (N, nc) int32 the integers the plain call codes for the rows, row_entries (N,) below m as
    merge_points has them; (m, nc) int32, entry j component c = floor((2 S + cnt) / (2 cnt)) over the cnt rows of cell j with sum S,
    in 64 bits -- the exact mean, ties toward +infinity.  What dsa_encode_mean_sequential_batch codes for a masked attribute."""
    L = lib()
    q = np.ascontiguousarray(q, np.int32)
    q = q.reshape(len(q), -1)
    cells = np.ascontiguousarray(row_entries, np.uint32)
    out = np.zeros((int(m), q.shape[1]), np.int32)
    if L.synth_merge_means(q.ctypes.data, len(q), q.shape[1], cells.ctypes.data, int(m), out.ctypes.data):
        raise RuntimeError(_err())
    return out


def merge_votes(q, row_entries, m):
    """The most frequent value of every cell: q (N, nc) int32 with nc 1 or 2, row_entries (N,) below m as merge_points has them;
    (m, nc) int32, entry j the tuple q[r] that the most rows r of cell j have, among tuples with equally many rows the
    lexicographically smallest (signed components, component 0 first).  What dsa_encode_vote_sequential_batch codes for a voted
    attribute."""
    L = lib()
    q = np.ascontiguousarray(q, np.int32)
    q = q.reshape(len(q), -1)
    cells = np.ascontiguousarray(row_entries, np.uint32)
    out = np.zeros((int(m), q.shape[1]), np.int32)
    if L.synth_merge_votes(q.ctypes.data, len(q), q.shape[1], cells.ctypes.data, int(m), out.ctypes.data):
        raise RuntimeError(_err())
    return out


def quantized_normals(normals, bits):
    """The octahedral codes (s, t) the coder quantises the normals (N, 3) to at `bits` normal bits: (N, 2) int32."""
    L = lib()
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    out = np.zeros((len(nrm), 2), np.int32)
    if L.synth_quantized_normals(nrm.ctypes.data, len(nrm), int(bits), out.ctypes.data):
        raise RuntimeError(_err())
    return out


def merge_mean_normals(q, bits, row_entries, m):
    """The mean normal of every cell: q (N, 2) int32 octahedral codes at `bits` normal bits, row_entries (N,) below m as merge_points
    has them; (m, 2) int32, entry j the code of the normalised sum of the unit normals of the rows of cell j by the integer rule of
    dsa_encode_normal_mean_sequential_batch (a cell of one row keeps its code).  What that call codes for the normals."""
    L = lib()
    q = np.ascontiguousarray(q, np.int32).reshape(-1, 2)
    cells = np.ascontiguousarray(row_entries, np.uint32)
    out = np.zeros((int(m), 2), np.int32)
    if L.synth_merge_mean_normals(q.ctypes.data, len(q), int(bits), cells.ctypes.data, int(m), out.ctypes.data):
        raise RuntimeError(_err())
    return out


def _extra_rows(e, rows, grid=None):
    """Extra e with its rows (and its portable integers) taken at `rows` (an index array or a slice); grid: in place of e.grid."""
    return Extra(e.values[rows], attribute_type=e.attribute_type, normalized=bool(e.normalized), unique_id=e.unique_id,
                 quantization_bits=e.quantization_bits, data_type=e.data_type, num_components=e.num_components, grid=e.grid if grid is None else grid,
                 portable=None if e.portable is None else e.portable[rows])


def merged_arguments(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, mean_attributes=0, vote_attributes=0,
                     mean_normals=False, voxel_bits=0, voxel_point=0):
    """The arguments of the plain call that writes a merged stream: (kept, row_entries, kwargs for encode_grid(form=0, geometry=0))
    -- every per-point array at [kept], every quantised attribute on an explicit grid equal to the bounds of ALL its rows (the
    grid given, where one was).  mean_attributes: bit a: attribute a of the stream (0 positions, then normals, uvs, generic and the
    extras, those given) carries merge_means of its cell in place of row kept[j] -- an integer attribute as the mean array, a
    quantised one as portable integers (uv_portable / Extra.portable) on the unchanged grid.  vote_attributes: likewise, bit a:
    attribute a (of 1 or 2 components) carries merge_votes of its cell; the two masks share no bit.  mean_normals: the normals, where
    given, carry merge_mean_normals of their cell as portable codes (normal_portable).  voxel_bits / voxel_point: the cells are
    merge_voxels' and kept its rows; the centroids go as portable integers (pos_portable) on the unchanged grid."""
    opt = opt or options()
    kept, cells, coded = merge_voxels(pos, opt.pos_bits, pos_grid, voxel_bits, voxel_point)
    m = len(kept)
    index = 1 + (normals is not None)                       # the stream's attribute index of the next attribute
    if mean_attributes & 1 or (normals is not None and mean_attributes & 2):
        raise ValueError("mean_attributes: positions and normals carry no mean")
    if vote_attributes & 1 or (normals is not None and vote_attributes & 2):
        raise ValueError("vote_attributes: positions and normals are not voted on")
    if mean_attributes & vote_attributes:
        raise ValueError("vote_attributes and mean_attributes share a bit")
    replaced = mean_attributes | vote_attributes

    def of_cells(q):        # what entry j carries in place of row kept[j], for the attribute `index` stands at
        return (merge_votes if (vote_attributes >> index) & 1 else merge_means)(q, cells, m)

    take = lambda a, nc: None if a is None else np.ascontiguousarray(np.asarray(a).reshape(-1, nc)[kept])      # noqa: E731
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    ug = uv_grid if uv_grid is not None or uvs is None else bounds_grid(np.asarray(uvs, np.float32).reshape(-1, 2))
    uv_portable = None
    if uvs is not None:
        if (replaced >> index) & 1:
            uv_portable = of_cells(quantized(np.asarray(uvs, np.float32).reshape(-1, 2), opt.uv_bits, ug))
        index += 1
    gen = None if generic is None else np.asarray(generic)[kept]
    if generic is not None:
        if (replaced >> index) & 1:
            g = np.asarray(generic)
            gen = of_cells(g.reshape(len(g), -1).astype(np.int32)).astype(g.dtype).reshape((m,) + g.shape[1:])
        index += 1
    ex = []
    for e in (extra or []):
        e = e if isinstance(e, Extra) else Extra(e)
        g = e.grid
        is_float = e.values.dtype == np.dtype(np.float32)
        if g is None and is_float:
            g = bounds_grid(e.values)
        x = _extra_rows(e, kept, g)
        if (replaced >> index) & 1:
            if is_float:
                bits = e.quantization_bits or (opt.uv_bits if e.attribute_type == 3 else 8)
                x.portable = of_cells(quantized(e.values, bits, g))
            else:
                x.values = np.ascontiguousarray(of_cells(e.values.astype(np.int64).astype(np.int32)).astype(e.values.dtype))
        ex.append(x)
        index += 1
    if mean_attributes >> index:
        raise ValueError("mean_attributes: a bit names an attribute the stream does not have")
    if vote_attributes >> index:
        raise ValueError("vote_attributes: a bit names an attribute the stream does not have")
    kw = dict(pos=pos[kept], normals=take(normals, 3), uvs=take(uvs, 2), generic=gen,
              extra=ex, opt=opt, pos_grid=pos_grid if pos_grid is not None else bounds_grid(pos), uv_grid=ug)
    if uv_portable is not None:
        kw["uv_portable"] = uv_portable
    if mean_normals and normals is not None:
        kw["normal_portable"] = merge_mean_normals(quantized_normals(np.asarray(normals, np.float32).reshape(-1, 3), opt.normal_bits), opt.normal_bits, cells, m)
    if voxel_point == VOXEL_POINT_CENTROID:
        kw["pos_portable"] = np.ascontiguousarray(coded[kept])
    return kept, cells, kw


def encode_merged(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, mean_attributes=0, vote_attributes=0,
                  mean_normals=False, voxel_bits=0, voxel_point=0):
    """encode_grid(form=0, geometry=0) of one point per occupied cell: (stream, kept, row_entries), merged_arguments coded.  What
    dsa_encode_merged_sequential_batch with merge_points = 1 must write, and the rows its handle must report; with mean_attributes
    what dsa_encode_mean_sequential_batch must, with vote_attributes what dsa_encode_vote_sequential_batch must, with mean_normals
    what dsa_encode_normal_mean_sequential_batch must, with voxel_bits / voxel_point what dsa_encode_voxel_sequential_batch must."""
    kept, cells, kw = merged_arguments(pos, normals, uvs, generic, extra, opt, pos_grid, uv_grid, mean_attributes, vote_attributes, mean_normals,
                                       voxel_bits, voxel_point)
    p = kw.pop("pos")
    return encode_grid(p, None, form=0, geometry=0, **kw), kept, cells


def split_parts(n, part_points):
    """The sorted order of a cloud of n points in parts of at most part_points points: an (P, 2) uint32 array of [lo, hi) with P =
    ceil(n / part_points) and part p = [floor(p n / P), floor((p + 1) n / P)) -- every part 1 .. part_points points, sizes that
    differ by at most one.  part_points 0: one part.  The ranges of dsa_encode_split_sequential_batch."""
    L = lib()
    parts = C.c_uint64()
    if L.synth_split_parts(int(n), int(part_points), None, 0, C.byref(parts)):
        raise RuntimeError(_err())
    ranges = np.zeros((parts.value, 2), np.uint32)
    if L.synth_split_parts(int(n), int(part_points), ranges.ctypes.data, len(ranges), C.byref(parts)):
        raise RuntimeError(_err())
    return ranges


def part_boxes(pos, bits, part_points, grid=None):
    """(perm, ranges, qmin, qmax) of the parts of the points `pos` (N, 3): perm = point_order(pos, bits, grid), ranges =
    split_parts(N, part_points), and qmin / qmax (P, 3) int32 the minimum and maximum per component of the integers the position
    stream codes for rows perm[lo:hi]."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    ranges = split_parts(len(pos), part_points)
    perm = np.zeros(len(pos), np.uint32)
    qmin, qmax = np.zeros((len(ranges), 3), np.int32), np.zeros((len(ranges), 3), np.int32)
    if L.synth_part_boxes(pos.ctypes.data, len(pos), int(bits), None if grid is None else C.byref(grid), int(part_points), perm.ctypes.data,
                          qmin.ctypes.data, qmax.ctypes.data):
        raise RuntimeError(_err())
    return perm, ranges, qmin, qmax


def split_arguments(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, part_points=0):
    """Per part of a split cloud the arguments of the plain call that writes its stream: [(rows, qmin, qmax, kwargs for
    encode_grid(form=0, geometry=0))] -- every per-point array at [rows] = perm[lo:hi], every quantised attribute on an explicit
    grid equal to the bounds of ALL the cloud's rows (the grid given, where one was)."""
    opt = opt or options()
    perm, ranges, qmin, qmax = part_boxes(pos, opt.pos_bits, part_points, pos_grid)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    pg = pos_grid if pos_grid is not None else bounds_grid(pos)
    ug = uv_grid if uv_grid is not None or uvs is None else bounds_grid(np.asarray(uvs, np.float32).reshape(-1, 2))
    extras = []
    for e in (extra or []):
        e = e if isinstance(e, Extra) else Extra(e)
        g = e.grid
        if g is None and e.values.dtype == np.dtype(np.float32):
            g = bounds_grid(e.values)
        extras.append((e, g))
    out = []
    for p, (lo, hi) in enumerate(ranges):
        rows = perm[lo:hi]
        take = lambda a, nc: None if a is None else np.ascontiguousarray(np.asarray(a).reshape(-1, nc)[rows])      # noqa: E731
        ex = [Extra(e.values[rows], attribute_type=e.attribute_type, normalized=bool(e.normalized), unique_id=e.unique_id,
                    quantization_bits=e.quantization_bits, data_type=e.data_type, num_components=e.num_components, grid=g) for e, g in extras]
        kw = dict(pos=pos[rows], normals=take(normals, 3), uvs=take(uvs, 2), generic=None if generic is None else np.asarray(generic)[rows],
                  extra=ex, opt=opt, pos_grid=pg, uv_grid=ug)
        out.append((rows, qmin[p], qmax[p], kw))
    return out


def encode_split(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, part_points=0):
    """The Morton order of a point cloud in parts of at most part_points points, each coded as a point cloud of its own on the
    cloud's grid: [(stream, rows, qmin, qmax)], split_arguments coded.  What dsa_encode_split_sequential_batch with part_points >= 1
    must write, and what its handle must report for every part."""
    out = []
    for rows, qmin, qmax, kw in split_arguments(pos, normals, uvs, generic, extra, opt, pos_grid, uv_grid, part_points):
        p = kw.pop("pos")
        out.append((encode_grid(p, None, form=0, geometry=0, **kw), rows, qmin, qmax))
    return out


def cell_parts(pos, bits, part_cells, grid=None, voxel_bits=0, voxel_point=0):
    """(kept, row_entries, ranges, qmin, qmax) of the points `pos` (N, 3): kept / row_entries = merge_points(pos, bits, grid), ranges =
    split_parts(len(kept), part_cells) -- parts of the KEPT order -- and qmin / qmax (P, 3) int32 the minimum and maximum per
    component of the integers the position stream codes for rows kept[lo:hi]."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    kept, cells = np.zeros(len(pos), np.uint32), np.zeros(len(pos), np.uint32)
    m, parts = C.c_uint32(), C.c_uint64()
    grid = None if grid is None else C.byref(grid)
    if L.synth_cell_parts(pos.ctypes.data, len(pos), int(bits), grid, int(part_cells), kept.ctypes.data, C.byref(m), cells.ctypes.data, None, None, None, 0, C.byref(parts),
                          int(voxel_bits), int(voxel_point)):
        raise RuntimeError(_err())
    ranges = np.zeros((parts.value, 2), np.uint32)
    qmin, qmax = np.zeros((parts.value, 3), np.int32), np.zeros((parts.value, 3), np.int32)
    if L.synth_cell_parts(pos.ctypes.data, len(pos), int(bits), grid, int(part_cells), kept.ctypes.data, C.byref(m), cells.ctypes.data, ranges.ctypes.data,
                          qmin.ctypes.data, qmax.ctypes.data, len(ranges), C.byref(parts), int(voxel_bits), int(voxel_point)):
        raise RuntimeError(_err())
    return kept[:m.value].copy(), cells, ranges, qmin, qmax


CellParts = collections.namedtuple("CellParts", "streams kept row_entries ranges qmin qmax")


def encode_cell_parts(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, part_cells=0, mean_attributes=0, vote_attributes=0,
                      mean_normals=False, voxel_bits=0, voxel_point=0):
    """One point per occupied cell, and the kept order in parts of at most part_cells points, each coded as a point cloud of its own
    on the cloud's grid: CellParts(streams, kept, row_entries, ranges, qmin, qmax) with merged_arguments' rows and grids -- every
    per-point array at [kept[lo:hi]], every quantised attribute on an explicit grid equal to the bounds of ALL input rows (the grid
    given, where one was).  What dsa_encode_cell_parts_sequential_batch with part_cells >= 1 must write, and what its handle must
    report."""
    opt = opt or options()
    kept, cells, ranges, qmin, qmax = cell_parts(pos, opt.pos_bits, part_cells, pos_grid, voxel_bits, voxel_point)
    _, _, kw = merged_arguments(pos, normals, uvs, generic, extra, opt, pos_grid, uv_grid, mean_attributes, vote_attributes, mean_normals, voxel_bits, voxel_point)
    p = kw.pop("pos")
    streams = []
    for lo, hi in ranges:
        take = lambda a: None if a is None else np.ascontiguousarray(a[lo:hi])          # noqa: E731
        ex = [_extra_rows(e, slice(lo, hi)) for e in kw["extra"]]
        streams.append(encode_grid(take(p), None, normals=take(kw["normals"]), uvs=take(kw["uvs"]), generic=take(kw["generic"]), extra=ex, opt=opt,
                                   form=0, geometry=0, pos_grid=kw["pos_grid"], uv_grid=kw["uv_grid"], uv_portable=take(kw.get("uv_portable")),
                                   normal_portable=take(kw.get("normal_portable")), pos_portable=take(kw.get("pos_portable"))))
    return CellParts(streams, kept, cells, ranges, qmin, qmax)


def lod_parts(pos, bits, part_cells, lod_base_bits, grid=None, voxel_bits=0, voxel_point=0):
    """(lod, row_entries, ranges, levels, qmin, qmax) of the points `pos` (N, 3): lod the kept rows of merge_points in ascending
    (level, position in kept) -- level(0) = 0, level(j) = max(0, c + 1 - lod_base_bits) with c the leading bit-triples the keys of
    kept[j] and kept[j - 1] share -- row_entries the lod entry of the cell of every row, ranges (P, 2) the parts of every level in
    turn (split_parts of the level's points, an empty level has none), levels (P,) the level of every part, qmin / qmax (P, 3) int32
    the box of the position integers of rows lod[lo:hi]."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    lod, cells = np.zeros(len(pos), np.uint32), np.zeros(len(pos), np.uint32)
    m, parts = C.c_uint32(), C.c_uint64()
    grid = None if grid is None else C.byref(grid)
    if L.synth_lod_parts(pos.ctypes.data, len(pos), int(bits), grid, int(part_cells), int(lod_base_bits), lod.ctypes.data, C.byref(m), cells.ctypes.data,
                         None, None, None, None, 0, C.byref(parts), int(voxel_bits), int(voxel_point)):
        raise RuntimeError(_err())
    ranges, levels = np.zeros((parts.value, 2), np.uint32), np.zeros(parts.value, np.uint32)
    qmin, qmax = np.zeros((parts.value, 3), np.int32), np.zeros((parts.value, 3), np.int32)
    if L.synth_lod_parts(pos.ctypes.data, len(pos), int(bits), grid, int(part_cells), int(lod_base_bits), lod.ctypes.data, C.byref(m), cells.ctypes.data,
                         ranges.ctypes.data, levels.ctypes.data, qmin.ctypes.data, qmax.ctypes.data, len(ranges), C.byref(parts), int(voxel_bits), int(voxel_point)):
        raise RuntimeError(_err())
    return lod[:m.value].copy(), cells, ranges, levels, qmin, qmax


LodParts = collections.namedtuple("LodParts", "streams kept row_entries ranges qmin qmax level levels")


def encode_lod_parts(pos, normals=None, uvs=None, generic=None, extra=None, opt=None, pos_grid=None, uv_grid=None, part_cells=0, lod_base_bits=0,
                     mean_attributes=0, vote_attributes=0, mean_normals=False, voxel_bits=0, voxel_point=0):
    """Additive levels of detail of the kept points, every level in parts of at most part_cells points, each part coded as a point
    cloud of its own on the cloud's grid: what encode_cell_parts returns with `kept` the rows in LOD order (ranges and row_entries
    count in it), plus `level` per stream and `levels` = L = position bits (voxel_bits, where given) - lod_base_bits + 1.  Every per-point array at
    [lod[lo:hi]], every quantised attribute on an explicit grid equal to the bounds of ALL input rows (the grid given, where one
    was).  What dsa_encode_lod_sequential_batch with lod_base_bits >= 1 must write, and what its handle must report.
    lod_base_bits 0: encode_cell_parts, every stream of level 0 of 1."""
    opt = opt or options()
    if lod_base_bits == 0:
        cp = encode_cell_parts(pos, normals, uvs, generic, extra, opt, pos_grid, uv_grid, part_cells, mean_attributes, vote_attributes, mean_normals, voxel_bits, voxel_point)
        return LodParts(*cp, level=np.zeros(len(cp.streams), np.uint32), levels=1)
    lod, cells, ranges, level, qmin, qmax = lod_parts(pos, opt.pos_bits, part_cells, lod_base_bits, pos_grid, voxel_bits, voxel_point)
    kept, _, kw = merged_arguments(pos, normals, uvs, generic, extra, opt, pos_grid, uv_grid, mean_attributes, vote_attributes, mean_normals, voxel_bits, voxel_point)
    at = np.zeros(int(kept.max()) + 1, np.int64)
    at[kept] = np.arange(len(kept))
    idx = at[lod]                                # where in kept (the order of merged_arguments' arrays) every lod entry lies
    p = kw.pop("pos")
    streams = []
    for lo, hi in ranges:
        take = lambda a: None if a is None else np.ascontiguousarray(a[idx[lo:hi]])          # noqa: E731
        ex = [_extra_rows(e, idx[lo:hi]) for e in kw["extra"]]
        streams.append(encode_grid(take(p), None, normals=take(kw["normals"]), uvs=take(kw["uvs"]), generic=take(kw["generic"]), extra=ex, opt=opt,
                                   form=0, geometry=0, pos_grid=kw["pos_grid"], uv_grid=kw["uv_grid"], uv_portable=take(kw.get("uv_portable")),
                                   normal_portable=take(kw.get("normal_portable")), pos_portable=take(kw.get("pos_portable"))))
    return LodParts(streams, lod, cells, ranges, qmin, qmax, level, (voxel_bits or opt.pos_bits) - lod_base_bits + 1)


def entry_rows(pos, faces=None, normals=None, uvs=None, generic=None, extra=None, opt=None, form=1, normal_corners=None, uv_corners=None,
               geometry=1, weld_attributes=False):
    """The entry rows of the stream encode_grid writes for the same arguments: a list with one uint32 array per attribute of the
    stream (positions, then normals, texture coordinates, generic where present, then `extra`), element e the row of the value array
    passed for that attribute whose bytes entry e of the stream carries.  form 1: the vertex, or the row id of an attribute given
    per corner; with opt.repair_topology a vertex the repair made reads its root parent's row.  form 2 (one row per point): the
    point whose row was read -- the representative of the attribute's key set, of the vertex where the attribute went on per vertex.
    form 0: the identity.  What dsa_encoded_entry_rows must report."""
    L = lib()
    pos, fc, nrm, uv, gen, extra, arr, opt = _points_args(pos, np.zeros((0, 3), np.uint32) if faces is None else faces, normals if normal_corners is None else None,
                                                          uvs if uv_corners is None else None, generic, extra, opt)
    if normal_corners is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if uv_corners is not None:
        uv = np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
    nci = None if normal_corners is None else np.ascontiguousarray(normal_corners, np.uint32)
    uci = None if uv_corners is None else np.ascontiguousarray(uv_corners, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    out, counts, na = C.c_void_p(), (C.c_uint32 * 32)(), C.c_uint32()
    rc = L.synth_entry_rows(form, ptr(pos), len(pos), ptr(fc) if len(fc) else None, len(fc), ptr(nrm), 0 if nrm is None else len(nrm), ptr(nci),
                            ptr(uv), 0 if uv is None else len(uv), ptr(uci), ptr(gen), geometry, arr, _extra_corners(extra, len(fc)), len(extra),
                            C.byref(opt), 1 if weld_attributes else 0, C.byref(out), counts, C.byref(na))
    if rc:
        raise RuntimeError(_err())
    total = sum(counts[a] for a in range(na.value))
    flat = np.frombuffer(C.string_at(out, 4 * total), np.uint32).copy() if total else np.zeros(0, np.uint32)
    L.synth_free(out)
    ends = np.cumsum([counts[a] for a in range(na.value)]).tolist()
    return [flat[e - counts[a]:e] for a, e in enumerate(ends)]


def encode_mesh_sequential(pos, faces, normals=None, uvs=None, compressed=True, opt=None):
    """Sequential mesh stream (MeshSequentialEncoder): faces as point indices, attributes in point order."""
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    faces = np.ascontiguousarray(faces, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32)
    out, n = C.c_void_p(), C.c_size_t()
    opt = opt or options()
    rc = L.synth_encode_mesh_sequential(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces),
                                        None if nrm is None else nrm.ctypes.data, None if uv is None else uv.ctypes.data,
                                        1 if compressed else 0, C.byref(opt), C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def encode_point_cloud(pos, opt=None):
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    out, n = C.c_void_p(), C.c_size_t()
    opt = opt or options()
    if L.synth_encode_point_cloud(pos.ctypes.data, len(pos), C.byref(opt), C.byref(out), C.byref(n)):
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def _sequential(pos, faces, normals, uvs, generic, geometry, compressed, opt, extra=None):
    L = lib()
    pos = np.ascontiguousarray(pos, np.float32)
    faces = None if faces is None else np.ascontiguousarray(faces, np.uint32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32)
    opt = opt or options()
    gen = None
    if generic is not None:
        gen, opt = _generic(generic, opt)
        gen = gen.reshape(len(gen), -1)
        if len(gen) != len(pos) or not 1 <= gen.shape[1] <= 4:
            raise ValueError("generic attribute: one row of 1 - 4 integer components per point")
        if opt.generic_components != gen.shape[1]:          # the components are the array's own (a copy: the caller's options stay)
            o2 = Options()
            C.memmove(C.byref(o2), C.byref(opt), C.sizeof(Options))
            o2.generic_components = gen.shape[1]
            opt = o2
    for a, name in ((nrm, "normals"), (uv, "uvs")):
        if a is not None and len(a) != len(pos):
            raise ValueError("%s: one row per point" % name)
    if extra:
        return _encode_attributes(False, pos, faces, nrm, None, uv, None, gen, geometry, compressed, extra, opt)
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.synth_encode_sequential(pos.ctypes.data, len(pos), None if faces is None else faces.ctypes.data,
                                   0 if faces is None else len(faces), None if nrm is None else nrm.ctypes.data,
                                   None if uv is None else uv.ctypes.data, None if gen is None else gen.ctypes.data,
                                   geometry, 1 if compressed else 0, C.byref(opt), C.byref(out), C.byref(n))
    if rc:
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def encode_sequential(pos, faces, normals=None, uvs=None, generic=None, compressed=False, opt=None, extra=None):
    """Sequential mesh stream with every per-vertex attribute (generic: (V,) or (V, 1..4) of int8 / uint8 / int16 / uint16 / int32 / uint32): faces and points keep the
    caller's order; any list of triangles over the points is legal.  compressed: indices through the symbol coder, else raw
    at the bitstream's widths.  What dsa_encode_sequential_batch must write for geometry 1."""
    return _sequential(pos, faces, normals, uvs, generic, 1, compressed, opt, extra)


def encode_point_cloud_attributes(pos, normals=None, uvs=None, generic=None, opt=None, extra=None):
    """Sequential point cloud with per-point normals / texture coordinates / generic integer attribute; positions only:
    the bytes of encode_point_cloud.  What dsa_encode_sequential_batch must write for geometry 0."""
    return _sequential(pos, None, normals, uvs, generic, 0, False, opt, extra)


def make_batch(kind, nx, ny, seed0, count, normals=True, uvs=True, opt=None, threads=None):
    """Encodes `count` meshes (seeds seed0..) and returns (blob uint8[...], offsets uint64[count+1])."""
    L = lib()
    opt = opt or options()
    threads = threads or min(os.cpu_count() or 1, 32)
    blob = C.c_void_p()
    offsets = np.zeros(count + 1, np.uint64)
    mask = (1 if normals else 0) | (2 if uvs else 0)
    if L.synth_make_batch(kind, nx, ny, seed0, count, mask, C.byref(opt), threads, C.byref(blob), offsets.ctypes.data):
        raise RuntimeError(_err())
    total = int(offsets[-1])
    arr = np.frombuffer(C.string_at(blob, total), np.uint8).copy() if total else np.zeros(0, np.uint8)
    L.synth_free(blob)
    return arr, offsets


def encode_symbols(values, nc=1, force_scheme=-1, compression_level=5):
    """DecodeSymbols()-compatible block (scheme byte first) for uint32 `values`."""
    L = lib()
    v = np.ascontiguousarray(values, np.uint32).ravel()
    out, n = C.c_void_p(), C.c_size_t()
    if L.synth_encode_symbols(v.ctypes.data, v.size, nc, force_scheme, compression_level, C.byref(out), C.byref(n)):
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data


def encode_rabs(bits):
    """rABS bit block {prob_zero, size varint, bytes} for a 0/1 array."""
    L = lib()
    b = np.ascontiguousarray(bits, np.uint8).ravel()
    out, n = C.c_void_p(), C.c_size_t()
    if L.synth_encode_rabs(b.ctypes.data, b.size, C.byref(out), C.byref(n)):
        raise RuntimeError(_err())
    data = C.string_at(out, n.value)
    L.synth_free(out)
    return data
