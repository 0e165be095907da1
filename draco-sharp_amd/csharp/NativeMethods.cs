// P/Invoke declarations for libdraco_mi355x.so (include/draco_mi355x.h).
// This file is what a draco-sharp maintainer adds next to src/Draco/IO/DracoDecoder.cs; it cannot be
// compiled in the build image (no .NET SDK), the ctypes binding in draco-sharp_amd/native.py is the
// executable twin used by the tests.  Blittable structs only, no callbacks, library-owned memory.
using System;
using System.Runtime.InteropServices;

namespace Draco.IO.Gpu;

internal enum DsaStatus : int
{
    Ok = 0,
    InvalidData = 1,      // -> InvalidDataException
    NotImplemented = 2,   // -> NotImplementedException
    InvalidArgument = 3,  // -> ArgumentException
    Device = 4,           // -> InvalidOperationException(dsa_last_error)
    OutOfMemory = 5       // -> OutOfMemoryException
}

[StructLayout(LayoutKind.Sequential)]
internal struct DsaMeshInfo
{
    public int Status;
    public int Detail;
    public byte MajorVersion, MinorVersion, EncoderType, EncoderMethod;
    public ushort Flags;
    public ushort DecodePath;   // 0 wave-per-mesh kernels, 1 general path, 2 general path at the second attempt
    public uint NumFaces;
    public uint NumPoints;
    public uint NumAttributes;
    public ulong DrcBytes;
}

[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaAttributeInfo
{
    public int AttributeType;
    public int DataType;
    public int NumComponents;
    public int Normalized;
    public uint UniqueId;
    public uint NumEntries;
    public uint ByteStride;
    public int DecoderType;
    public int PredictionMethod;
    public int PredictionTransform;
    public int QuantizationBits;
    public float Range;
    public fixed float MinValues[4];
}

[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshOutput       // byte offsets of a mesh's arrays inside the batch's output block (dsa_batch_download)
{
    public uint Block;        // 0: the batch's block, 1: the block of the meshes decoded a second time (general path)
    public uint Flags;            // DSA_OUTPUT_FACES_U16 = 1 (compact download)
    public ulong Faces;
    public fixed ulong Values[16];
    public fixed ulong PointMap[16];
}

// dsa_vertex_request (dsa_batch_vertex_arrays): one index array and one row per point and attribute, gathered on the device (32 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaVertexRequest
{
    public int Format;              // 0 DSA_VA_VALUES: decoded values, 1 DSA_VA_QUANTIZED: quantised attributes as uint16 rows of portable integers
    public uint Flags;              // 1 DSA_VA_DEVICE_ONLY: gather, no device -> host transfer
    public uint AttributeTypes;     // bit t: attributes of GeometryAttributeType t; 0 = all
    public fixed uint Reserved[5];  // zero
}

[StructLayout(LayoutKind.Sequential)]
internal struct DsaVertexAttribute  // 24 bytes
{
    public ulong Offset;            // byte offset in the block; ulong.MaxValue when absent
    public uint Stride;             // bytes per point
    public int DataType;            // Draco.IO.Enums.DataType of the stored elements (UInt16 = 4 for quantised rows)
    public uint NumComponents;      // stored per row (2 for octahedral normals in the quantised format)
    public uint Flags;              // 1 DSA_VA_ABSENT: left out by the mask, or quantised with more than 16 bits
}

[StructLayout(LayoutKind.Sequential)]
internal struct DsaMeshVertexArrays // 408 bytes
{
    public uint Block;              // 0, or 1 for a mesh decoded a second time
    public uint Flags;              // 1 DSA_VA_INDICES_U16
    public ulong Indices;           // ushort / uint [3 * faces]; ulong.MaxValue for a point cloud
    public uint NumPoints, NumIndices;
    public DsaVertexAttribute A0, A1, A2, A3, A4, A5, A6, A7, A8, A9, A10, A11, A12, A13, A14, A15;   // attributes[DSA_MAX_ATTRIBUTES]

    internal unsafe DsaVertexAttribute Attribute(uint a)
    {
        if (a >= 16) throw new ArgumentOutOfRangeException(nameof(a));
        fixed (DsaVertexAttribute* p = &A0) return p[a];
    }
}

// dsa_join_group / dsa_join_request / dsa_joined_arrays (dsa_batch_joined_arrays): the part streams of a cloud as one array per attribute
[StructLayout(LayoutKind.Sequential)]
internal struct DsaJoinGroup        // 8 bytes
{
    public uint FirstMesh, NumMeshes;   // meshes FirstMesh .. FirstMesh + NumMeshes of the batch
}

[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaJoinRequest   // 64 bytes
{
    public DsaVertexRequest Arrays; // exactly as for dsa_batch_vertex_arrays
    public int Order;               // 0 DSA_JOIN_STREAM_ORDER, 1 DSA_JOIN_INPUT_ORDER
    public fixed uint Reserved[7];  // zero
}

[StructLayout(LayoutKind.Sequential)]
internal struct DsaJoinedArrays     // 400 bytes
{
    public uint FirstMesh, NumMeshes, NumRows;
    public int Order;
    public DsaVertexAttribute A0, A1, A2, A3, A4, A5, A6, A7, A8, A9, A10, A11, A12, A13, A14, A15;   // attributes[DSA_MAX_ATTRIBUTES]

    internal unsafe DsaVertexAttribute Attribute(uint a)
    {
        if (a >= 16) throw new ArgumentOutOfRangeException(nameof(a));
        fixed (DsaVertexAttribute* p = &A0) return p[a];
    }
}

[StructLayout(LayoutKind.Sequential)]
internal struct DsaEncodeOptions
{
    public int PositionBits, TexcoordBits, NormalBits;
    public int SingleConnectivity;
    public int SymbolScheme;        // -1 auto, 0 tagged, 1 raw
    public int CompressionLevel;    // 10 - Config.Speed
    public int PositionPrediction, TexcoordPrediction;
}

// dsa_encode_options_ex (dsa_encode_batch_ex): valence Edgebreaker, TexCoordsPortable, GeometricNormal
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeOptionsEx
{
    public DsaEncodeOptions Base;
    public int EdgebreakerMethod;   // 0 standard, 2 valence, -1 by speed and face count (DracoEncoder.cs:86-97)
    public int NormalPrediction;    // 0 difference, 6 GeometricNormal
    public fixed int Reserved[6];   // zero
}

// dsa_encode_level_options (dsa_encode_level_batch): MultiParallelogram / ConstrainedMultiParallelogram, prediction-degree order (96 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeLevelOptions
{
    public DsaEncodeOptionsEx Ex;
    public int MultiParallelogram;  // 0 off, 4 constrained, 2 plain, -1 by speed and point count (PredictionSchemeEncoderFactory.cs:63-71)
    public int TraversalMethod;     // 0 depth first, 1 prediction degree for the positions' decoder, 2 for every decoder without seams
    public fixed int Reserved[6];   // zero
}

// dsa_welded_info (dsa_weld_batch): the weld of one mesh given as one row per point; the maps live in the handle (80 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaWeldedInfo
{
    public int Status;
    public uint NumPoints, NumVertices, NumNormals, NumTexcoords;
    public uint NormalsPerVertex, TexcoordsPerVertex;
    public uint Reserved;           // zero
    public uint* VertexOfPoint, VertexPoint;
    public uint* NormalOfPoint, NormalPoint;
    public uint* TexcoordOfPoint, TexcoordPoint;
}

// dsa_encode_repair_options (dsa_encode_repair_batch): the reference's corner table for meshes that are not clean (128 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeRepairOptions
{
    public DsaEncodeLevelOptions Level;
    public int Topology;            // 0 strict, 1 repair as CornerTable(faces) does (CornerTable.cs:28-43)
    public fixed int Reserved[7];   // zero
}

// dsa_quantization_grid: the grid of one quantised attribute (32 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaQuantizationGrid
{
    public fixed float Origin[4];
    public float Range;
    public int Mode;                // 0 own bounds, 1 explicit (quantization_origin / quantization_range), 2 shared within Group
    public fixed uint Reserved[2];  // zero
}

// dsa_mesh_grids: the grids of one mesh, parallel to DsaMeshAttrInput (80 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshGrids
{
    public DsaQuantizationGrid Position, Texcoord;
    public DsaQuantizationGrid* Attributes;     // NumAttributes entries or null
    public uint Group;
    public uint Reserved;           // zero
}

// dsa_encode_grid_options (dsa_encode_grid_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeGridOptions
{
    public DsaEncodeRepairOptions Repair;
    public int WeldPoints;          // 1: one row per point, as dsa_encode_points_batch
    public fixed int Reserved[7];   // zero
}

// dsa_encode_seam_repair_options (dsa_encode_seam_repair_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeSeamRepairOptions
{
    public DsaEncodeGridOptions Grid;
    public int CornerRepair;        // 1: attributes given per corner are coded over a mesh whose topology needs the repair (needs Topology 1)
    public fixed int Reserved[7];   // zero
}

// dsa_attribute_corners: row ids per corner for one attribute of the list (16 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaAttributeCorners
{
    public uint* Corners;           // 3 * NumFaces row ids into the attribute's Values, or null: per vertex
    public uint NumRows;            // rows of Values when Corners is set
    public uint Reserved;           // zero
}

// dsa_mesh_attribute_corners: the ids of the listed attributes of one mesh, parallel to DsaMeshAttrInput (16 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshAttributeCorners
{
    public DsaAttributeCorners* Attributes;     // NumAttributes entries or null
    public fixed uint Reserved[2];  // zero
}

// dsa_encode_corner_attributes_options (dsa_encode_corner_attributes_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeCornerAttributesOptions
{
    public DsaEncodeSeamRepairOptions SeamRepair;
    public int WeldAttributes;      // 1: with WeldPoints every listed attribute is welded alone, like normals and texture coordinates
    public fixed int Reserved[7];   // zero
}

// dsa_encode_rows_options (dsa_encode_rows_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeRowsOptions
{
    public DsaEncodeCornerAttributesOptions CornerAttributes;
    public int TrackRows;           // 1: the handle keeps, per stream and attribute, the row of the caller's arrays every entry carries
    public fixed int Reserved[7];   // zero
}

// dsa_encode_sequential_options (dsa_encode_sequential_batch): sequential meshes and point clouds
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeSequentialOptions
{
    public DsaEncodeOptions Base;       // quantisation bits, SymbolScheme, CompressionLevel are used
    public int Geometry;                // 1 triangular mesh, 0 point cloud (Constants.EncodingType)
    public int CompressConnectivity;    // 0 raw indices, 1 compressed (ConfigOptionName.CompressConnectivity)
    public fixed int Reserved[6];       // zero
}

// dsa_encode_order_options (dsa_encode_ordered_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeOrderOptions
{
    public DsaEncodeSequentialOptions Sequential;
    public int PointOrder;          // 0: the caller's order; 1: Morton order of the quantised positions, the handle keeps the permutation
    public fixed int Reserved[7];   // zero
}

// dsa_encode_merge_options (dsa_encode_merged_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeMergeOptions
{
    public DsaEncodeOrderOptions Order;
    public int MergePoints;         // 0: every point is coded; 1: one point per occupied cell of the position grid (point clouds, PointOrder 1)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_split_options (dsa_encode_split_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeSplitOptions
{
    public DsaEncodeMergeOptions Merge;
    public int PartPoints;          // 0: one stream per cloud; N >= 1: the Morton order in parts of at most N points (point clouds, PointOrder 1, MergePoints 0)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_cell_parts_options (dsa_encode_cell_parts_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeCellPartsOptions
{
    public DsaEncodeSplitOptions Split;
    public int PartCells;           // 0: the request of the split call; N >= 1: the KEPT order of MergePoints in parts of at most N points (point clouds, PointOrder 1, MergePoints 1, PartPoints 0)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_lod_options (dsa_encode_lod_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeLodOptions
{
    public DsaEncodeCellPartsOptions CellParts;
    public int LodBaseBits;         // 0: the request of the cell-parts call; D >= 1: additive levels of detail of the kept points, level 0 on the grid of D bits per axis (needs PartCells >= 1)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_mean_options (dsa_encode_mean_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeMeanOptions
{
    public DsaEncodeLodOptions Lod;
    public uint MeanAttributes;     // 0: the request of the lod call; bit a: attribute a of the stream carries the exact mean of its cell's rows (needs MergePoints 1)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_vote_options (dsa_encode_vote_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeVoteOptions
{
    public DsaEncodeMeanOptions Mean;
    public uint VoteAttributes;     // 0: the request of the mean call; bit a: attribute a of the stream (1 or 2 components) carries the most frequent value of its cell's rows (needs MergePoints 1)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_normal_mean_options (dsa_encode_normal_mean_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeNormalMeanOptions
{
    public DsaEncodeVoteOptions Vote;
    public uint MeanNormals;        // 0: the request of the vote call; 1: the normals of every kept point are the mean normal of its cell (needs MergePoints 1)
    public fixed int Reserved[7];   // zero
}

// dsa_encode_voxel_options (dsa_encode_voxel_sequential_batch)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaEncodeVoxelOptions
{
    public DsaEncodeNormalMeanOptions NormalMean;
    public int VoxelBits;           // 0: the request of the normal-mean call; C >= 1: one point per cell of the grid with C bits per axis (needs MergePoints 1)
    public int VoxelPoint;          // 0 the voxel's first row, 1 that row at the voxel's mean position, 2 the row nearest the voxel's centre
    public fixed int Reserved[6];   // zero
}

// dsa_lod_info (dsa_encoded_lod_info)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaLodInfo
{
    public uint Input;
    public uint Level, Levels;
    public uint CellBits;
    public uint LevelFirstStream, LevelStreams;
    public uint LevelPoints;
    public uint PartInLevel;
    public fixed uint Reserved[4];  // zero
}

// dsa_part_info (dsa_encoded_part_info)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaPartInfo
{
    public uint Input, Part, Parts; // which cloud of the call, which of its parts, how many it has
    public uint FirstEntry, NumPoints;
    public uint PositionBits;
    public fixed int QMin[3];
    public fixed int QMax[3];
    public fixed float BoxMin[3];
    public fixed float BoxMax[3];
    public fixed uint Reserved[2];  // zero
}

[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshInput
{
    public uint NumVertices, NumFaces;
    public float* Positions;
    public uint* Faces;
    public float* Normals;
    public float* Texcoords;
    public byte* Generic;           // ABI 4: num_vertices * GenericComponents bytes or null
    public uint GenericComponents;
    public uint Reserved;
}

// dsa_mesh_corner_input (dsa_encode_batch_corners): normals / texture coordinates given per corner
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshCornerInput
{
    public DsaMeshInput Mesh;       // Normals / Texcoords hold NumNormals / NumTexcoords rows where the ids below are set
    public uint* NormalCorners;     // 3 * NumFaces row ids into Mesh.Normals, or null: per vertex
    public uint* TexcoordCorners;   // 3 * NumFaces row ids into Mesh.Texcoords, or null: per vertex
    public uint NumNormals, NumTexcoords;
}

// dsa_attribute_input: one more per-vertex attribute behind the built-in ones (40 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaAttributeInput
{
    public int AttributeType;       // GeometryAttributeType: 2 colour, 3 texture coordinate, 4 generic
    public int DataType;            // Draco.IO.Enums.DataType: 1 Int8 .. 6 UInt32, 9 Float32
    public uint NumComponents;      // 1..4
    public int Normalized;          // 0 / 1 (integer types)
    public uint UniqueId;           // 0xFFFFFFFF: the attribute's index in the stream
    public int QuantizationBits;    // Float32 only: 1..20; 0: the texture coordinates' bits for type 3, else 8
    public void* Values;            // NumVertices rows, packed
    public fixed uint Reserved[2];  // zero
}

// dsa_mesh_attr_input (dsa_encode_attributes_batch / dsa_encode_attributes_sequential_batch): a mesh with an attribute list (96 bytes)
[StructLayout(LayoutKind.Sequential)]
internal unsafe struct DsaMeshAttrInput
{
    public DsaMeshCornerInput Mesh;
    public DsaAttributeInput* Attributes;   // written behind the built-in attributes in list order
    public uint NumAttributes, Reserved;
}

internal static unsafe partial class NativeMethods
{
    private const string Lib = "draco_mi355x";

    [DllImport(Lib)] internal static extern int dsa_abi_version();
    [DllImport(Lib)] internal static extern int dsa_device_count();
    [DllImport(Lib)] internal static extern DsaStatus dsa_context_create(int device, IntPtr stream, out IntPtr ctx);
    [DllImport(Lib)] internal static extern void dsa_context_destroy(IntPtr ctx);
    [DllImport(Lib)] internal static extern IntPtr dsa_last_error(IntPtr ctx);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_create(IntPtr ctx, uint n, byte** streams, nuint* lengths, out IntPtr batch);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_create_packed(IntPtr ctx, uint n, byte* blob, ulong* offsets, out IntPtr batch);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_decode(IntPtr batch);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_wait(IntPtr batch);
    [DllImport(Lib)] internal static extern void dsa_batch_free(IntPtr batch);
    [DllImport(Lib)] internal static extern uint dsa_batch_size(IntPtr batch);
    [DllImport(Lib)] internal static extern ulong dsa_batch_algorithmic_bytes(IntPtr batch);
    [DllImport(Lib)] internal static extern ulong dsa_batch_arena_bytes(IntPtr batch);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_mesh_info(IntPtr batch, uint mesh, out DsaMeshInfo info);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_attribute_info(IntPtr batch, uint mesh, uint attribute, out DsaAttributeInfo info);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_faces(IntPtr batch, uint mesh, int* dst);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_attribute_values(IntPtr batch, uint mesh, uint attribute, void* dst);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_point_map(IntPtr batch, uint mesh, uint attribute, uint* dst);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_portable_values(IntPtr batch, uint mesh, uint attribute, int* dst);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_device_faces(IntPtr batch, uint mesh);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_device_attribute_values(IntPtr batch, uint mesh, uint attribute);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_device_point_map(IntPtr batch, uint mesh, uint attribute);
    // whole-batch copy-out: one transfer of every output array into a pinned mirror (or caller memory), beside the next batch's kernels
    [DllImport(Lib)] internal static extern ulong dsa_batch_output_bytes(IntPtr batch);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_download(IntPtr batch, void* dst, nuint dstBytes);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_download_compact(IntPtr batch, void* dst, nuint dstBytes);
    [DllImport(Lib)] internal static extern ulong dsa_batch_compact_bytes(IntPtr batch);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_host_output(IntPtr batch, uint block);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_output_layout(IntPtr batch, uint mesh, out DsaMeshOutput layout);
    // vertex arrays: per-point rows gathered on the device behind the decode, one transfer; added after ABI 4 (detect by the symbol)
    [DllImport(Lib)] internal static extern ulong dsa_batch_vertex_arrays_bytes(IntPtr batch, in DsaVertexRequest request);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_vertex_arrays(IntPtr batch, in DsaVertexRequest request, void* dst, nuint dstBytes);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_vertex_arrays_layout(IntPtr batch, uint mesh, out DsaMeshVertexArrays layout);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_host_vertex_arrays(IntPtr batch, uint block);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_device_vertex_arrays(IntPtr batch, uint block);
    [DllImport(Lib)] internal static extern ulong dsa_batch_joined_arrays_bytes(IntPtr batch, in DsaJoinRequest request, uint numGroups, DsaJoinGroup* groups);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_joined_arrays(IntPtr batch, in DsaJoinRequest request, uint numGroups, DsaJoinGroup* groups, IntPtr encoded, uint* encodedMesh, void* dst, nuint dstBytes);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_joined_arrays_layout(IntPtr batch, uint group, out DsaJoinedArrays layout);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_joined_member(IntPtr batch, uint mesh, out uint group, out uint firstRow, out uint numRows);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_host_joined_arrays(IntPtr batch);
    [DllImport(Lib)] internal static extern IntPtr dsa_batch_device_joined_arrays(IntPtr batch);
    [DllImport(Lib)] internal static extern IntPtr dsa_host_alloc(nuint bytes);
    [DllImport(Lib)] internal static extern void dsa_host_free(IntPtr p);
    [DllImport(Lib)] internal static extern DsaStatus dsa_host_register(void* p, nuint bytes);
    [DllImport(Lib)] internal static extern DsaStatus dsa_host_unregister(void* p);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_metadata(IntPtr batch, uint mesh, byte* dst, nuint dstBytes, out nuint length);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_copy_debug(IntPtr batch, uint mesh, int what, void* dst, nuint dstBytes, out nuint written);
    [DllImport(Lib)] internal static extern DsaStatus dsa_context_set_profiling(IntPtr ctx, int enabled);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_stage_times(IntPtr batch, float* ms, IntPtr* names);
    [DllImport(Lib)] internal static extern DsaStatus dsa_batch_kernel_times(IntPtr batch, float* ms, IntPtr* names, uint capacity, out uint count);
    [DllImport(Lib)] internal static extern DsaStatus dsa_context_trim(IntPtr ctx);
    [DllImport(Lib)] internal static extern IntPtr dsa_context_schedule_note(IntPtr ctx);

    // encode direction (DracoEncoder.Encode, src/Draco/IO/DracoEncoder.cs:22-41)
    [DllImport(Lib)] internal static extern void dsa_encode_default_options(out DsaEncodeOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_batch(IntPtr ctx, uint n, DsaMeshInput* meshes, in DsaEncodeOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_batch_corners(IntPtr ctx, uint n, DsaMeshCornerInput* meshes, in DsaEncodeOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_options_ex(out DsaEncodeOptionsEx options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_batch_ex(IntPtr ctx, uint n, DsaMeshCornerInput* meshes, in DsaEncodeOptionsEx options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_sequential_default_options(out DsaEncodeSequentialOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_sequential_batch(IntPtr ctx, uint n, DsaMeshInput* meshes, in DsaEncodeSequentialOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_level_options(out DsaEncodeLevelOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_level_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeLevelOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_repair_options(out DsaEncodeRepairOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_repair_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeRepairOptions options, out IntPtr encoded);
    // meshes given as one row per point: the weld in front of dsa_encode_repair_batch, and the weld alone (detect by symbol)
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_points_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeRepairOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_grid_options(out DsaEncodeGridOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_grid_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeGridOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_seam_repair_options(out DsaEncodeSeamRepairOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_seam_repair_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSeamRepairOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_corner_attributes_options(out DsaEncodeCornerAttributesOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_corner_attributes_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, DsaMeshAttributeCorners* corners, in DsaEncodeCornerAttributesOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_grid_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSequentialOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_weld_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, out IntPtr welded);
    [DllImport(Lib)] internal static extern uint dsa_welded_size(IntPtr welded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_welded_mesh(IntPtr welded, uint mesh, out DsaWeldedInfo info);
    [DllImport(Lib)] internal static extern void dsa_welded_free(IntPtr welded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_attributes_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeOptionsEx options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_attributes_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeSequentialOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern uint dsa_encoded_size(IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_rows_options(out DsaEncodeRowsOptions options);
    [DllImport(Lib)] internal static extern void dsa_encode_default_order_options(out DsaEncodeOrderOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_ordered_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeOrderOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_merge_options(out DsaEncodeMergeOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_merged_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeMergeOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_row_entries(IntPtr encoded, uint mesh, uint* dst, nuint capacity, out uint count);
    [DllImport(Lib)] internal static extern void dsa_encode_default_split_options(out DsaEncodeSplitOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_split_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSplitOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_cell_parts_options(out DsaEncodeCellPartsOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_cell_parts_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeCellPartsOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_lod_options(out DsaEncodeLodOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_lod_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeLodOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_lod_info(IntPtr encoded, uint stream, out DsaLodInfo info);
    [DllImport(Lib)] internal static extern void dsa_encode_default_mean_options(out DsaEncodeMeanOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_mean_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeMeanOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_vote_options(out DsaEncodeVoteOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_vote_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeVoteOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_normal_mean_options(out DsaEncodeNormalMeanOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_normal_mean_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeNormalMeanOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern void dsa_encode_default_voxel_options(out DsaEncodeVoxelOptions options);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_voxel_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeVoxelOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_parts(IntPtr encoded, uint input, out uint firstStream, out uint count);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_part_info(IntPtr encoded, uint stream, out DsaPartInfo info);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encode_rows_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, DsaMeshAttributeCorners* corners, in DsaEncodeRowsOptions options, out IntPtr encoded);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_entry_rows(IntPtr encoded, uint mesh, uint attribute, uint* dst, nuint capacity, out uint count);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_attributes(IntPtr encoded, uint mesh, out uint count);
    [DllImport(Lib)] internal static extern DsaStatus dsa_encoded_stream(IntPtr encoded, uint mesh, out byte* bytes, out nuint length);
    [DllImport(Lib)] internal static extern void dsa_encoded_free(IntPtr encoded);

    // multi-GPU submit for a single-process host: one context + worker thread per listed device inside the library
    [DllImport(Lib)] internal static extern DsaStatus dsa_pool_create(int* devices, uint numDevices, uint chunkMeshes, out IntPtr pool);
    [DllImport(Lib)] internal static extern void dsa_pool_destroy(IntPtr pool);
    [DllImport(Lib)] internal static extern uint dsa_pool_size(IntPtr pool);
    [DllImport(Lib)] internal static extern IntPtr dsa_pool_last_error(IntPtr pool);
    [DllImport(Lib)] internal static extern DsaStatus dsa_pool_decode(IntPtr pool, uint n, byte** streams, nuint* lengths, out IntPtr job);
    [DllImport(Lib)] internal static extern DsaStatus dsa_pool_job_locate(IntPtr job, uint stream, out IntPtr batch, out uint mesh, out uint worker);
    [DllImport(Lib)] internal static extern uint dsa_pool_job_chunks(IntPtr job);
    [DllImport(Lib)] internal static extern void dsa_pool_job_free(IntPtr job);
    [DllImport(Lib)] internal static extern uint dsa_pool_plan(uint n, nuint* lengths, uint chunkMeshes, uint* order, uint* chunkBegin);

    internal static void Check(DsaStatus status, IntPtr ctx, string what)
    {
        if (status == DsaStatus.Ok) return;
        var msg = ctx == IntPtr.Zero ? what : $"{what}: {Marshal.PtrToStringAnsi(dsa_last_error(ctx))}";
        throw status switch
        {
            DsaStatus.InvalidData => new System.IO.InvalidDataException(msg),
            DsaStatus.NotImplemented => new NotImplementedException(msg),
            DsaStatus.InvalidArgument => new ArgumentException(msg),
            DsaStatus.OutOfMemory => new OutOfMemoryException(msg),
            _ => new InvalidOperationException(msg),
        };
    }
}
