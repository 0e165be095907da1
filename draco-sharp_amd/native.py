"""ctypes binding of libdraco_mi355x.so (include/draco_mi355x.h).  There is no CPU
fallback: if the HIP library is missing or no GPU is present the calls raise."""
import ctypes as C
import os
import subprocess

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("DSA_LIB") or os.path.join(_DIR, "libdraco_mi355x.so")   # DSA_LIB: kernel-ablation builds

DSA_OK, DSA_ERR_INVALID_DATA, DSA_ERR_NOT_IMPLEMENTED, DSA_ERR_INVALID_ARGUMENT, DSA_ERR_DEVICE, DSA_ERR_OUT_OF_MEMORY = range(6)
DSA_NUM_STAGES = 8
DSA_OUTPUT_FACES_U16 = 1
NO_MAP = 0xFFFFFFFFFFFFFFFF   # dsa_mesh_output.point_map: the identity map, not stored (compact download)
DSA_VA_VALUES, DSA_VA_QUANTIZED = 0, 1      # dsa_vertex_request.format
DSA_VA_DEVICE_ONLY = 1                      # dsa_vertex_request.flags
DSA_VA_ABSENT = 1                           # dsa_vertex_attribute.flags
DSA_VA_INDICES_U16 = 1                      # dsa_mesh_vertex_arrays.flags
VA_NONE = 0xFFFFFFFFFFFFFFFF                # an array that is not in the block
DSA_SOURCE_ROWS_DEVICE_ONLY = C.c_size_t(-1).value      # dsa_batch_source_rows: dst NULL with this dst_bytes: no host copy
DSA_JOIN_STREAM_ORDER, DSA_JOIN_INPUT_ORDER = 0, 1      # dsa_join_request.order

# every symbol include/draco_mi355x.h declares
EXPORTS = [
    "dsa_abi_version", "dsa_device_count", "dsa_context_create", "dsa_context_destroy", "dsa_last_error",
    "dsa_batch_create", "dsa_batch_create_packed", "dsa_batch_decode", "dsa_batch_wait", "dsa_batch_free",
    "dsa_batch_size", "dsa_batch_algorithmic_bytes", "dsa_batch_arena_bytes", "dsa_batch_mesh_info",
    "dsa_batch_attribute_info", "dsa_batch_copy_faces", "dsa_batch_copy_attribute_values", "dsa_batch_copy_point_map",
    "dsa_batch_copy_portable_values", "dsa_batch_device_faces", "dsa_batch_device_attribute_values",
    "dsa_batch_device_point_map", "dsa_batch_output_bytes", "dsa_batch_download", "dsa_batch_compact_bytes", "dsa_batch_download_compact", "dsa_batch_host_output", "dsa_batch_output_layout",
    "dsa_batch_vertex_arrays_bytes", "dsa_batch_vertex_arrays", "dsa_batch_vertex_arrays_layout", "dsa_batch_host_vertex_arrays", "dsa_batch_device_vertex_arrays",
    "dsa_batch_source_rows_bytes", "dsa_batch_source_rows", "dsa_batch_source_rows_layout", "dsa_batch_host_source_rows", "dsa_batch_device_source_rows",
    "dsa_batch_joined_arrays_bytes", "dsa_batch_joined_arrays", "dsa_batch_joined_arrays_layout", "dsa_batch_joined_member", "dsa_batch_host_joined_arrays", "dsa_batch_device_joined_arrays",
    "dsa_host_alloc", "dsa_host_free", "dsa_host_register", "dsa_host_unregister", "dsa_batch_copy_metadata", "dsa_batch_copy_debug", "dsa_context_set_profiling", "dsa_batch_stage_times",
    "dsa_batch_kernel_times", "dsa_context_trim", "dsa_context_schedule_note",
    "dsa_encode_default_options", "dsa_encode_batch", "dsa_encode_batch_corners",
    "dsa_encode_default_options_ex", "dsa_encode_batch_ex", "dsa_encode_sequential_default_options", "dsa_encode_sequential_batch",
    "dsa_encode_attributes_batch", "dsa_encode_attributes_sequential_batch",
    "dsa_encode_default_level_options", "dsa_encode_level_batch",
    "dsa_encode_default_repair_options", "dsa_encode_repair_batch",
    "dsa_encode_points_batch", "dsa_weld_batch", "dsa_welded_size", "dsa_welded_mesh", "dsa_welded_free",
    "dsa_encode_default_grid_options", "dsa_encode_grid_batch", "dsa_encode_grid_sequential_batch",
    "dsa_encode_default_seam_repair_options", "dsa_encode_seam_repair_batch",
    "dsa_encode_default_corner_attributes_options", "dsa_encode_corner_attributes_batch",
    "dsa_encode_default_rows_options", "dsa_encode_rows_batch", "dsa_encoded_entry_rows", "dsa_encoded_attributes",
    "dsa_encode_default_order_options", "dsa_encode_ordered_sequential_batch",
    "dsa_encode_default_merge_options", "dsa_encode_merged_sequential_batch", "dsa_encoded_row_entries",
    "dsa_encode_default_split_options", "dsa_encode_split_sequential_batch", "dsa_encoded_parts", "dsa_encoded_part_info",
    "dsa_encode_default_cell_parts_options", "dsa_encode_cell_parts_sequential_batch",
    "dsa_encode_default_lod_options", "dsa_encode_lod_sequential_batch", "dsa_encoded_lod_info",
    "dsa_encode_default_mean_options", "dsa_encode_mean_sequential_batch",
    "dsa_encode_default_vote_options", "dsa_encode_vote_sequential_batch",
    "dsa_encode_default_normal_mean_options", "dsa_encode_normal_mean_sequential_batch",
    "dsa_encode_default_voxel_options", "dsa_encode_voxel_sequential_batch",
    "dsa_encoded_size", "dsa_encoded_stream", "dsa_encoded_free",
    "dsa_pool_create", "dsa_pool_destroy", "dsa_pool_size", "dsa_pool_last_error", "dsa_pool_decode", "dsa_pool_job_locate",
    "dsa_pool_job_chunks", "dsa_pool_job_free", "dsa_pool_plan",
]


class EncodeOptions(C.Structure):
    _fields_ = [("position_bits", C.c_int32), ("texcoord_bits", C.c_int32), ("normal_bits", C.c_int32),
                ("single_connectivity", C.c_int32), ("symbol_scheme", C.c_int32), ("compression_level", C.c_int32),
                ("position_prediction", C.c_int32), ("texcoord_prediction", C.c_int32)]


class EncodeOptionsEx(C.Structure):
    """dsa_encode_options_ex: valence Edgebreaker (edgebreaker_method 2, or -1 by speed and face count) and GeometricNormal
    (normal_prediction 6) beside the options of dsa_encode_batch."""
    _fields_ = [("base", EncodeOptions), ("edgebreaker_method", C.c_int32), ("normal_prediction", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class EncodeLevelOptions(C.Structure):
    """dsa_encode_level_options: multi_parallelogram (0 off, 4 ConstrainedMultiParallelogram, 2 MultiParallelogram, -1 the
    reference's rule per mesh) and traversal_method (0 depth first, 1 / 2 prediction degree) beside the options of
    dsa_encode_attributes_batch."""
    _fields_ = [("ex", EncodeOptionsEx), ("multi_parallelogram", C.c_int32), ("traversal_method", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class EncodeRepairOptions(C.Structure):
    """dsa_encode_repair_options: topology (0 strict, 1 the reference's corner table: degenerate faces, non-manifold edges and
    vertices and isolated vertices are repaired, not refused) beside the options of dsa_encode_level_batch."""
    _fields_ = [("level", EncodeLevelOptions), ("topology", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeSequentialOptions(C.Structure):
    """dsa_encode_sequential_options: sequential meshes (geometry 1; compress_connectivity 0 raw indices, 1 compressed) and point
    clouds (geometry 0) beside the quantisation bits, symbol_scheme and compression_level of dsa_encode_batch."""
    _fields_ = [("base", EncodeOptions), ("geometry", C.c_int32), ("compress_connectivity", C.c_int32),
                ("reserved", C.c_int32 * 6)]


POINT_ORDER_CALLER, POINT_ORDER_MORTON = 0, 1      # dsa_encode_order_options.point_order
ENCODE_ORDER_TILE = 1024                            # DSA_ENCODE_ORDER_TILE: entries of a tile of the sort behind POINT_ORDER_MORTON


class EncodeOrderOptions(C.Structure):
    """dsa_encode_order_options: the options of dsa_encode_grid_sequential_batch, and point_order (1: the points of every stream in
    Morton order of their quantised positions; the handle keeps the permutation: dsa_encoded_entry_rows)."""
    _fields_ = [("sequential", EncodeSequentialOptions), ("point_order", C.c_int32), ("reserved", C.c_int32 * 7)]


MERGE_NONE, MERGE_CELLS = 0, 1                      # dsa_encode_merge_options.merge_points


class EncodeMergeOptions(C.Structure):
    """dsa_encode_merge_options: the options of dsa_encode_ordered_sequential_batch, and merge_points (1: one point per occupied
    cell of the position grid of a point cloud; the handle keeps the kept rows and the entry of every input row:
    dsa_encoded_entry_rows, dsa_encoded_row_entries)."""
    _fields_ = [("order", EncodeOrderOptions), ("merge_points", C.c_int32), ("reserved", C.c_int32 * 7)]


ENCODE_MAX_PARTS = 65536                            # DSA_ENCODE_MAX_PARTS: parts of one cloud
MAX_ATTRIBUTES = 16                                 # DSA_MAX_ATTRIBUTES: attributes of a stream


class EncodeSplitOptions(C.Structure):
    """dsa_encode_split_options: the options of dsa_encode_merged_sequential_batch, and part_points (N >= 1: the Morton order of
    every point cloud in parts of at most N points, a stream each; the handle has a slot per stream: dsa_encoded_parts,
    dsa_encoded_part_info)."""
    _fields_ = [("merge", EncodeMergeOptions), ("part_points", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeCellPartsOptions(C.Structure):
    """dsa_encode_cell_parts_options: the options of dsa_encode_split_sequential_batch, and part_cells (N >= 1, with merge_points = 1:
    the KEPT order of every point cloud in parts of at most N points, sized on the device; the handle is shaped like a split one)."""
    _fields_ = [("split", EncodeSplitOptions), ("part_cells", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeLodOptions(C.Structure):
    """dsa_encode_lod_options: the options of dsa_encode_cell_parts_sequential_batch, and lod_base_bits (D >= 1, with part_cells >= 1:
    the kept points of every cloud in additive levels of detail, level 0 one point per cell of the grid with D bits per axis, every
    level in parts of at most part_cells points; the handle is shaped like a cell-parts one)."""
    _fields_ = [("cell_parts", EncodeCellPartsOptions), ("lod_base_bits", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeMeanOptions(C.Structure):
    """dsa_encode_mean_options: the options of dsa_encode_lod_sequential_batch, and mean_attributes (with merge_points = 1: bit a set:
    attribute a of the stream carries, per component, the exact mean of the integers of the rows of the cell, ties upwards; positions
    and normals carry none)."""
    _fields_ = [("lod", EncodeLodOptions), ("mean_attributes", C.c_uint32), ("reserved", C.c_int32 * 7)]


class EncodeVoteOptions(C.Structure):
    """dsa_encode_vote_options: the options of dsa_encode_mean_sequential_batch, and vote_attributes (with merge_points = 1: bit a set:
    attribute a of the stream, of 1 or 2 components, carries the tuple of coded integers that the most rows of the cell have, among
    tuples of equally many rows the lexicographically smallest; positions and normals are not voted on, the two masks share no bit)."""
    _fields_ = [("mean", EncodeMeanOptions), ("vote_attributes", C.c_uint32), ("reserved", C.c_int32 * 7)]


class EncodeNormalMeanOptions(C.Structure):
    """dsa_encode_normal_mean_options: the options of dsa_encode_vote_sequential_batch, and mean_normals (with merge_points = 1: 1: the
    normals of every cloud that has them carry, per kept point, the mean normal of its cell by the integer rule of the header)."""
    _fields_ = [("vote", EncodeVoteOptions), ("mean_normals", C.c_uint32), ("reserved", C.c_int32 * 7)]


# dsa_encode_voxel_options.voxel_point (DSA_VOXEL_POINT_*)
VOXEL_POINT_FIRST, VOXEL_POINT_CENTROID, VOXEL_POINT_NEAREST = 0, 1, 2


class EncodeVoxelOptions(C.Structure):
    """dsa_encode_voxel_options: the options of dsa_encode_normal_mean_sequential_batch, voxel_bits (with merge_points = 1: C >= 1: one
    point per occupied cell of the grid with C bits per axis, whatever position_bits the positions are stored at) and voxel_point
    (VOXEL_POINT_*: the voxel's first row, that row at the voxel's mean position, or the row nearest the voxel's centre)."""
    _fields_ = [("normal_mean", EncodeNormalMeanOptions), ("voxel_bits", C.c_int32), ("voxel_point", C.c_int32), ("reserved", C.c_int32 * 6)]


class LodInfo(C.Structure):
    """dsa_lod_info: which level of which input a stream of an encode with lod_base_bits >= 1 belongs to."""
    _fields_ = [("input", C.c_uint32), ("level", C.c_uint32), ("levels", C.c_uint32), ("cell_bits", C.c_uint32),
                ("level_first_stream", C.c_uint32), ("level_streams", C.c_uint32), ("level_points", C.c_uint32), ("part_in_level", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class PartInfo(C.Structure):
    """dsa_part_info: which part of which input a stream of a split encode is, and the box of its points."""
    _fields_ = [("input", C.c_uint32), ("part", C.c_uint32), ("parts", C.c_uint32), ("first_entry", C.c_uint32), ("num_points", C.c_uint32),
                ("position_bits", C.c_uint32), ("qmin", C.c_int32 * 3), ("qmax", C.c_int32 * 3), ("box_min", C.c_float * 3),
                ("box_max", C.c_float * 3), ("reserved", C.c_uint32 * 2)]


class MeshInput(C.Structure):
    _fields_ = [("num_vertices", C.c_uint32), ("num_faces", C.c_uint32), ("positions", C.c_void_p), ("faces", C.c_void_p),
                ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("generic", C.c_void_p), ("generic_components", C.c_uint32),
                ("reserved", C.c_uint32)]


class MeshCornerInput(C.Structure):
    """dsa_mesh_corner_input: a mesh whose normals / texture coordinates may be given per corner (row ids per face corner)."""
    _fields_ = [("mesh", MeshInput), ("normal_corners", C.c_void_p), ("texcoord_corners", C.c_void_p),
                ("num_normals", C.c_uint32), ("num_texcoords", C.c_uint32)]


UNIQUE_ID_DEFAULT = 0xFFFFFFFF   # dsa_attribute_input.unique_id: the attribute's index in the stream


class AttributeInput(C.Structure):
    """dsa_attribute_input: one more per-vertex attribute behind the built-in ones (attribute_type 2 colour, 3 texture coordinate,
    4 generic; data_type 1 int8 ... 6 uint32, 9 float32)."""
    _fields_ = [("attribute_type", C.c_int32), ("data_type", C.c_int32), ("num_components", C.c_uint32), ("normalized", C.c_int32),
                ("unique_id", C.c_uint32), ("quantization_bits", C.c_int32), ("values", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class MeshAttrInput(C.Structure):
    """dsa_mesh_attr_input: a mesh (or point cloud) with an attribute list."""
    _fields_ = [("mesh", MeshCornerInput), ("attributes", C.POINTER(AttributeInput)), ("num_attributes", C.c_uint32),
                ("reserved", C.c_uint32)]


class QuantizationGrid(C.Structure):
    """dsa_quantization_grid: mode 0 the attribute's own bounds, 1 explicit (origin per component, one range), 2 shared by the
    meshes of a group."""
    _fields_ = [("origin", C.c_float * 4), ("range", C.c_float), ("mode", C.c_int32), ("reserved", C.c_uint32 * 2)]


class MeshGrids(C.Structure):
    """dsa_mesh_grids: the grids of one mesh (positions, the first UV set, the attribute list) and its group."""
    _fields_ = [("position", QuantizationGrid), ("texcoord", QuantizationGrid), ("attributes", C.POINTER(QuantizationGrid)),
                ("group", C.c_uint32), ("reserved", C.c_uint32)]


class EncodeGridOptions(C.Structure):
    """dsa_encode_grid_options: the options of dsa_encode_repair_batch, and weld_points (1: the input of dsa_encode_points_batch)."""
    _fields_ = [("repair", EncodeRepairOptions), ("weld_points", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeSeamRepairOptions(C.Structure):
    """dsa_encode_seam_repair_options: the options of dsa_encode_grid_batch, and corner_repair (1: attributes given per corner are
    coded over a mesh whose topology needs the repair; needs topology 1)."""
    _fields_ = [("grid", EncodeGridOptions), ("corner_repair", C.c_int32), ("reserved", C.c_int32 * 7)]


class AttributeCorners(C.Structure):
    """dsa_attribute_corners: row ids per corner for one attribute of the list (corners NULL: per vertex)."""
    _fields_ = [("corners", C.c_void_p), ("num_rows", C.c_uint32), ("reserved", C.c_uint32)]


class MeshAttributeCorners(C.Structure):
    """dsa_mesh_attribute_corners: the ids of the listed attributes of one mesh (attributes NULL: all per vertex)."""
    _fields_ = [("attributes", C.POINTER(AttributeCorners)), ("reserved", C.c_uint32 * 2)]


class EncodeCornerAttributesOptions(C.Structure):
    """dsa_encode_corner_attributes_options: the options of dsa_encode_seam_repair_batch, and weld_attributes (1: with weld_points
    every listed attribute is welded alone, like normals and texture coordinates)."""
    _fields_ = [("seam_repair", EncodeSeamRepairOptions), ("weld_attributes", C.c_int32), ("reserved", C.c_int32 * 7)]


class EncodeRowsOptions(C.Structure):
    """dsa_encode_rows_options: the options of dsa_encode_corner_attributes_batch, and track_rows (1: the handle keeps, per stream
    and attribute, the row of the caller's arrays every entry carries: dsa_encoded_entry_rows)."""
    _fields_ = [("corner_attributes", EncodeCornerAttributesOptions), ("track_rows", C.c_int32), ("reserved", C.c_int32 * 7)]


class WeldedInfo(C.Structure):
    """dsa_welded_info: the weld of one mesh given as one row per point -- counts, whether normals / texture coordinates collapse
    to one row per vertex, and the six maps (host memory owned by the dsa_welded handle)."""
    _fields_ = [("status", C.c_int32), ("num_points", C.c_uint32), ("num_vertices", C.c_uint32), ("num_normals", C.c_uint32),
                ("num_texcoords", C.c_uint32), ("normals_per_vertex", C.c_uint32), ("texcoords_per_vertex", C.c_uint32),
                ("reserved", C.c_uint32),
                ("vertex_of_point", C.c_void_p), ("vertex_point", C.c_void_p), ("normal_of_point", C.c_void_p),
                ("normal_point", C.c_void_p), ("texcoord_of_point", C.c_void_p), ("texcoord_point", C.c_void_p)]


class MeshInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("detail", C.c_int32), ("major_version", C.c_uint8), ("minor_version", C.c_uint8),
                ("encoder_type", C.c_uint8), ("encoder_method", C.c_uint8), ("flags", C.c_uint16), ("decode_path", C.c_uint16),
                ("num_faces", C.c_uint32), ("num_points", C.c_uint32), ("num_attributes", C.c_uint32),
                ("drc_bytes", C.c_uint64)]


class MeshOutput(C.Structure):
    _fields_ = [("block", C.c_uint32), ("flags", C.c_uint32), ("faces", C.c_uint64), ("values", C.c_uint64 * 16), ("point_map", C.c_uint64 * 16)]


class VertexRequest(C.Structure):
    """dsa_vertex_request: format (DSA_VA_VALUES / DSA_VA_QUANTIZED), flags (DSA_VA_DEVICE_ONLY), attribute_types (bit t: attributes of
    GeometryAttributeType t; 0 = all)."""
    _fields_ = [("format", C.c_int32), ("flags", C.c_uint32), ("attribute_types", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class VertexAttribute(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("stride", C.c_uint32), ("data_type", C.c_int32), ("num_components", C.c_uint32), ("flags", C.c_uint32)]


class MeshVertexArrays(C.Structure):
    _fields_ = [("block", C.c_uint32), ("flags", C.c_uint32), ("indices", C.c_uint64), ("num_points", C.c_uint32), ("num_indices", C.c_uint32),
                ("attributes", VertexAttribute * 16)]


class MeshSourceRows(C.Structure):
    """dsa_mesh_source_rows: where the arrays of one mesh lie in the block of dsa_batch_source_rows."""
    _fields_ = [("block", C.c_uint32), ("num_points", C.c_uint32), ("num_attributes", C.c_uint32), ("reserved", C.c_uint32), ("rows", C.c_uint64 * 16)]


class JoinGroup(C.Structure):
    """dsa_join_group: meshes first_mesh .. first_mesh + num_meshes of the batch."""
    _fields_ = [("first_mesh", C.c_uint32), ("num_meshes", C.c_uint32)]


class JoinRequest(C.Structure):
    """dsa_join_request: arrays (as for dsa_batch_vertex_arrays), order (DSA_JOIN_STREAM_ORDER / DSA_JOIN_INPUT_ORDER)."""
    _fields_ = [("arrays", VertexRequest), ("order", C.c_int32), ("reserved", C.c_uint32 * 7)]


class JoinedArrays(C.Structure):
    """dsa_joined_arrays: where the arrays of one group lie in the block of dsa_batch_joined_arrays."""
    _fields_ = [("first_mesh", C.c_uint32), ("num_meshes", C.c_uint32), ("num_rows", C.c_uint32), ("order", C.c_int32), ("attributes", VertexAttribute * 16)]


class AttributeInfo(C.Structure):
    _fields_ = [("attribute_type", C.c_int32), ("data_type", C.c_int32), ("num_components", C.c_int32),
                ("normalized", C.c_int32), ("unique_id", C.c_uint32), ("num_entries", C.c_uint32),
                ("byte_stride", C.c_uint32), ("decoder_type", C.c_int32), ("prediction_method", C.c_int32),
                ("prediction_transform", C.c_int32), ("quantization_bits", C.c_int32), ("range", C.c_float),
                ("min_values", C.c_float * 4)]


def build(force=False):
    """Compiles the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    # make knows the prerequisites (compiler-written depfile)
    subprocess.check_call(["make", "-C", _DIR, "-s"] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libdraco_mi355x.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, u32 = C.c_void_p, C.c_uint32
        L.dsa_abi_version.restype = C.c_int
        L.dsa_device_count.restype = C.c_int
        L.dsa_context_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.dsa_context_destroy.argtypes = [vp]
        L.dsa_last_error.restype = C.c_char_p
        L.dsa_last_error.argtypes = [vp]
        L.dsa_batch_create.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
        L.dsa_batch_create_packed.argtypes = [vp, u32, vp, vp, C.POINTER(vp)]
        L.dsa_batch_decode.argtypes = [vp]
        L.dsa_batch_wait.argtypes = [vp]
        L.dsa_batch_free.argtypes = [vp]
        L.dsa_batch_size.restype = u32
        L.dsa_batch_size.argtypes = [vp]
        L.dsa_batch_algorithmic_bytes.restype = C.c_uint64
        L.dsa_batch_algorithmic_bytes.argtypes = [vp]
        L.dsa_batch_arena_bytes.restype = C.c_uint64
        L.dsa_batch_arena_bytes.argtypes = [vp]
        L.dsa_batch_mesh_info.argtypes = [vp, u32, C.POINTER(MeshInfo)]
        L.dsa_batch_attribute_info.argtypes = [vp, u32, u32, C.POINTER(AttributeInfo)]
        L.dsa_batch_copy_faces.argtypes = [vp, u32, vp]
        L.dsa_batch_copy_attribute_values.argtypes = [vp, u32, u32, vp]
        L.dsa_batch_copy_point_map.argtypes = [vp, u32, u32, vp]
        L.dsa_batch_copy_portable_values.argtypes = [vp, u32, u32, vp]
        for f in ("dsa_batch_device_faces",):
            getattr(L, f).restype = vp
            getattr(L, f).argtypes = [vp, u32]
        for f in ("dsa_batch_device_attribute_values", "dsa_batch_device_point_map"):
            getattr(L, f).restype = vp
            getattr(L, f).argtypes = [vp, u32, u32]
        L.dsa_batch_output_bytes.restype = C.c_uint64
        L.dsa_batch_output_bytes.argtypes = [vp]
        L.dsa_batch_download.argtypes = [vp, vp, C.c_size_t]
        L.dsa_batch_download_compact.argtypes = [vp, vp, C.c_size_t]
        L.dsa_batch_compact_bytes.restype = C.c_uint64
        L.dsa_batch_compact_bytes.argtypes = [vp]
        L.dsa_batch_host_output.restype = vp
        L.dsa_batch_host_output.argtypes = [vp, u32]
        L.dsa_batch_output_layout.argtypes = [vp, u32, C.POINTER(MeshOutput)]
        L.dsa_batch_vertex_arrays_bytes.restype = C.c_uint64
        L.dsa_batch_vertex_arrays_bytes.argtypes = [vp, C.POINTER(VertexRequest)]
        L.dsa_batch_vertex_arrays.argtypes = [vp, C.POINTER(VertexRequest), vp, C.c_size_t]
        L.dsa_batch_vertex_arrays_layout.argtypes = [vp, u32, C.POINTER(MeshVertexArrays)]
        for f in ("dsa_batch_host_vertex_arrays", "dsa_batch_device_vertex_arrays"):
            getattr(L, f).restype = vp
            getattr(L, f).argtypes = [vp, u32]
        if hasattr(L, "dsa_batch_source_rows"):
            L.dsa_batch_source_rows_bytes.restype = C.c_uint64
            L.dsa_batch_source_rows_bytes.argtypes = [vp, vp, vp]
            L.dsa_batch_source_rows.argtypes = [vp, vp, vp, vp, C.c_size_t]
            L.dsa_batch_source_rows_layout.argtypes = [vp, u32, C.POINTER(MeshSourceRows)]
            for f in ("dsa_batch_host_source_rows", "dsa_batch_device_source_rows"):
                getattr(L, f).restype = vp
                getattr(L, f).argtypes = [vp, u32]
        if hasattr(L, "dsa_batch_joined_arrays"):
            L.dsa_batch_joined_arrays_bytes.restype = C.c_uint64
            L.dsa_batch_joined_arrays_bytes.argtypes = [vp, C.POINTER(JoinRequest), u32, C.POINTER(JoinGroup)]
            L.dsa_batch_joined_arrays.argtypes = [vp, C.POINTER(JoinRequest), u32, C.POINTER(JoinGroup), vp, vp, vp, C.c_size_t]
            L.dsa_batch_joined_arrays_layout.argtypes = [vp, u32, C.POINTER(JoinedArrays)]
            L.dsa_batch_joined_member.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
            for f in ("dsa_batch_host_joined_arrays", "dsa_batch_device_joined_arrays"):
                getattr(L, f).restype = vp
                getattr(L, f).argtypes = [vp]
        L.dsa_host_alloc.restype = vp
        L.dsa_host_alloc.argtypes = [C.c_size_t]
        L.dsa_host_free.restype = None
        L.dsa_host_free.argtypes = [vp]
        L.dsa_host_register.argtypes = [vp, C.c_size_t]
        L.dsa_host_unregister.argtypes = [vp]
        L.dsa_batch_copy_metadata.argtypes = [vp, u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.dsa_batch_copy_debug.argtypes = [vp, u32, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.dsa_context_set_profiling.argtypes = [vp, C.c_int]
        L.dsa_batch_stage_times.argtypes = [vp, C.POINTER(C.c_float * DSA_NUM_STAGES), C.POINTER(C.c_char_p * DSA_NUM_STAGES)]
        L.dsa_batch_kernel_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_uint32)]
        L.dsa_context_trim.argtypes = [vp]
        L.dsa_context_schedule_note.restype = C.c_char_p
        L.dsa_context_schedule_note.argtypes = [vp]
        L.dsa_encode_default_options.argtypes = [C.POINTER(EncodeOptions)]
        L.dsa_encode_default_options.restype = None
        L.dsa_encode_batch.argtypes = [vp, u32, C.POINTER(MeshInput), C.POINTER(EncodeOptions), C.POINTER(vp)]
        L.dsa_encode_batch_corners.argtypes = [vp, u32, C.POINTER(MeshCornerInput), C.POINTER(EncodeOptions), C.POINTER(vp)]
        L.dsa_encode_default_options_ex.argtypes = [C.POINTER(EncodeOptionsEx)]
        L.dsa_encode_default_options_ex.restype = None
        L.dsa_encode_batch_ex.argtypes = [vp, u32, C.POINTER(MeshCornerInput), C.POINTER(EncodeOptionsEx), C.POINTER(vp)]
        L.dsa_encode_sequential_default_options.argtypes = [C.POINTER(EncodeSequentialOptions)]
        L.dsa_encode_sequential_default_options.restype = None
        L.dsa_encode_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshInput), C.POINTER(EncodeSequentialOptions), C.POINTER(vp)]
        L.dsa_encode_attributes_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(EncodeOptionsEx), C.POINTER(vp)]
        L.dsa_encode_attributes_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(EncodeSequentialOptions), C.POINTER(vp)]
        L.dsa_encode_default_level_options.argtypes = [C.POINTER(EncodeLevelOptions)]
        L.dsa_encode_default_level_options.restype = None
        L.dsa_encode_level_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(EncodeLevelOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_repair_batch"):      # (DSA_LIB may name an older build for a same-box A/B; build() checks EXPORTS on the tree's own)
            L.dsa_encode_default_repair_options.argtypes = [C.POINTER(EncodeRepairOptions)]
            L.dsa_encode_default_repair_options.restype = None
            L.dsa_encode_repair_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(EncodeRepairOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_points_batch"):
            L.dsa_encode_points_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(EncodeRepairOptions), C.POINTER(vp)]
            L.dsa_weld_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(vp)]
            L.dsa_welded_size.restype = u32
            L.dsa_welded_size.argtypes = [vp]
            L.dsa_welded_mesh.argtypes = [vp, u32, C.POINTER(WeldedInfo)]
            L.dsa_welded_free.argtypes = [vp]
            L.dsa_welded_free.restype = None
        if hasattr(L, "dsa_encode_grid_batch"):
            L.dsa_encode_default_grid_options.argtypes = [C.POINTER(EncodeGridOptions)]
            L.dsa_encode_default_grid_options.restype = None
            L.dsa_encode_grid_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeGridOptions), C.POINTER(vp)]
            L.dsa_encode_grid_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeSequentialOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_seam_repair_batch"):
            L.dsa_encode_default_seam_repair_options.argtypes = [C.POINTER(EncodeSeamRepairOptions)]
            L.dsa_encode_default_seam_repair_options.restype = None
            L.dsa_encode_seam_repair_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeSeamRepairOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_corner_attributes_batch"):
            L.dsa_encode_default_corner_attributes_options.argtypes = [C.POINTER(EncodeCornerAttributesOptions)]
            L.dsa_encode_default_corner_attributes_options.restype = None
            L.dsa_encode_corner_attributes_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(MeshAttributeCorners),
                                                             C.POINTER(EncodeCornerAttributesOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_rows_batch"):
            L.dsa_encode_default_rows_options.argtypes = [C.POINTER(EncodeRowsOptions)]
            L.dsa_encode_default_rows_options.restype = None
            L.dsa_encode_rows_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(MeshAttributeCorners),
                                                C.POINTER(EncodeRowsOptions), C.POINTER(vp)]
            L.dsa_encoded_entry_rows.argtypes = [vp, u32, u32, vp, C.c_size_t, C.POINTER(u32)]
            L.dsa_encoded_attributes.argtypes = [vp, u32, C.POINTER(u32)]
        if hasattr(L, "dsa_encode_ordered_sequential_batch"):
            L.dsa_encode_default_order_options.argtypes = [C.POINTER(EncodeOrderOptions)]
            L.dsa_encode_default_order_options.restype = None
            L.dsa_encode_ordered_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeOrderOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_merged_sequential_batch"):
            L.dsa_encode_default_merge_options.argtypes = [C.POINTER(EncodeMergeOptions)]
            L.dsa_encode_default_merge_options.restype = None
            L.dsa_encode_merged_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeMergeOptions), C.POINTER(vp)]
            L.dsa_encoded_row_entries.argtypes = [vp, u32, vp, C.c_size_t, C.POINTER(u32)]
        if hasattr(L, "dsa_encode_split_sequential_batch"):
            L.dsa_encode_default_split_options.argtypes = [C.POINTER(EncodeSplitOptions)]
            L.dsa_encode_default_split_options.restype = None
            L.dsa_encode_split_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeSplitOptions), C.POINTER(vp)]
            L.dsa_encoded_parts.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
            L.dsa_encoded_part_info.argtypes = [vp, u32, C.POINTER(PartInfo)]
        if hasattr(L, "dsa_encode_cell_parts_sequential_batch"):
            L.dsa_encode_default_cell_parts_options.argtypes = [C.POINTER(EncodeCellPartsOptions)]
            L.dsa_encode_default_cell_parts_options.restype = None
            L.dsa_encode_cell_parts_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeCellPartsOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_lod_sequential_batch"):
            L.dsa_encode_default_lod_options.argtypes = [C.POINTER(EncodeLodOptions)]
            L.dsa_encode_default_lod_options.restype = None
            L.dsa_encode_lod_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeLodOptions), C.POINTER(vp)]
            L.dsa_encoded_lod_info.argtypes = [vp, u32, C.POINTER(LodInfo)]
        if hasattr(L, "dsa_encode_mean_sequential_batch"):
            L.dsa_encode_default_mean_options.argtypes = [C.POINTER(EncodeMeanOptions)]
            L.dsa_encode_default_mean_options.restype = None
            L.dsa_encode_mean_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeMeanOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_vote_sequential_batch"):
            L.dsa_encode_default_vote_options.argtypes = [C.POINTER(EncodeVoteOptions)]
            L.dsa_encode_default_vote_options.restype = None
            L.dsa_encode_vote_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeVoteOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_normal_mean_sequential_batch"):
            L.dsa_encode_default_normal_mean_options.argtypes = [C.POINTER(EncodeNormalMeanOptions)]
            L.dsa_encode_default_normal_mean_options.restype = None
            L.dsa_encode_normal_mean_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeNormalMeanOptions), C.POINTER(vp)]
        if hasattr(L, "dsa_encode_voxel_sequential_batch"):
            L.dsa_encode_default_voxel_options.argtypes = [C.POINTER(EncodeVoxelOptions)]
            L.dsa_encode_default_voxel_options.restype = None
            L.dsa_encode_voxel_sequential_batch.argtypes = [vp, u32, C.POINTER(MeshAttrInput), C.POINTER(MeshGrids), C.POINTER(EncodeVoxelOptions), C.POINTER(vp)]
        L.dsa_encoded_size.restype = u32
        L.dsa_encoded_size.argtypes = [vp]
        L.dsa_encoded_stream.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.dsa_encoded_free.argtypes = [vp]
        L.dsa_encoded_free.restype = None
        L.dsa_pool_create.argtypes = [C.POINTER(C.c_int), u32, u32, C.POINTER(vp)]
        L.dsa_pool_destroy.argtypes = [vp]
        L.dsa_pool_destroy.restype = None
        L.dsa_pool_size.argtypes = [vp]
        L.dsa_pool_size.restype = u32
        L.dsa_pool_last_error.argtypes = [vp]
        L.dsa_pool_last_error.restype = C.c_char_p
        L.dsa_pool_decode.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
        L.dsa_pool_job_locate.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
        L.dsa_pool_job_chunks.argtypes = [vp]
        L.dsa_pool_job_chunks.restype = u32
        L.dsa_pool_job_free.argtypes = [vp]
        L.dsa_pool_job_free.restype = None
        L.dsa_pool_plan.argtypes = [u32, C.POINTER(C.c_size_t), u32, C.POINTER(u32), C.POINTER(u32)]
        L.dsa_pool_plan.restype = u32
        _lib = L
    return _lib
