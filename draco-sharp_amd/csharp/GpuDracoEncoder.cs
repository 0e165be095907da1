// GPU-backed twin of Draco.IO.DracoEncoder (src/Draco/IO/DracoEncoder.cs:8-41) for triangle meshes with positions, normals and
// texture coordinates.  Like the reference (CornerTable.cs:571-596 CreateFromAttribute), a mesh whose points do not map one to one
// onto position values, or whose normal / texture coordinate mapping differs from the position mapping, is coded in corner form:
// vertices are position values, normals / texture coordinates keep their own values with an id per corner, and the edges where
// those ids change become attribute seams (dsa_encode_batch_corners).  Not compiled in the build image (no .NET SDK); the executable twin
// is draco-sharp_amd/encoder.py.  Config options honoured: quantisation bits per attribute type and Speed
// (src/Draco/IO/Config.cs); everything else keeps the reference's defaults (standard Edgebreaker, DFS traversal).
// An explicitly set ConfigOptionName.EncodingMethod of SequentialEncoding (with ConfigOptionName.CompressConnectivity) and a
// PointCloud that is not a Mesh go through dsa_encode_sequential_batch: points and faces in the caller's order, one value per point.
// Every PointAttribute beyond positions, normals, the first texture coordinates and a uint8 generic attribute -- colours, joints and
// weights, further UV sets, feature ids -- is passed as an extra with its AttributeType, DataType, NumComponents, Normalized and
// UniqueId (dsa_encode_attributes_batch / dsa_encode_attributes_sequential_batch); without such attributes the calls are what they were.
// The levels above the default (dsa_encode_level_batch): an explicitly set position PredictionScheme of MultiParallelogram (2) or
// ConstrainedMultiParallelogram (4) replaces Parallelogram by it; with SpeedLadder set, Config.Speed chooses as the reference does --
// ConstrainedMultiParallelogram at Speed < 2 for meshes of 40 points or more, prediction-degree order at Speed 0.  Neither set: the
// calls and their bytes are what they were.
// RepairTopology (dsa_encode_repair_batch, topology 1): meshes with degenerate faces, the same face twice, fins, faces turned over,
// fans that meet at a vertex or unused vertices are coded on the corner table CornerTable(faces) builds (CornerTable.cs:28-43), as
// DracoEncoder.Encode codes them, instead of failing; clean meshes give the same bytes.  A mesh in corner form that needs the
// repair still fails (NotImplementedException) unless RepairSeams is set (dsa_encode_seam_repair_batch, corner_repair 1): then its
// normals and texture coordinates are coded over the repaired table, as DracoEncoder.Encode codes them.
// CornerAttributes / WeldAttributes (dsa_encode_corner_attributes_batch): the attributes beyond the built-in slots -- a second UV set,
// colours, feature ids -- may have seams of their own.  CornerAttributes: in corner form, such an attribute whose point-to-value map
// differs from the positions' keeps its own values with an id per corner taken from that map.  WeldAttributes (with WeldPoints): the
// library welds every such attribute alone instead of making it part of the vertex key.  Neither set: the calls and their bytes are
// what they were.  (Like the rest of this file, written against the header and not compiled in the build image.)
using System;
using System.Collections.Generic;
using System.IO;
using System.Runtime.InteropServices;
using Draco.IO.Attributes;
using Draco.IO.Enums;

namespace Draco.IO.Gpu;

public sealed unsafe class GpuDracoEncoder : IDisposable
{
    private IntPtr _ctx;

    /// <summary>Follow the reference's speed ladder above its default level (PredictionSchemeEncoderFactory.cs:63-71,
    /// MeshEdgeBreakerEncoder.cs:528-546) instead of writing the default level's schemes at every Speed.</summary>
    public bool SpeedLadder { get; set; }

    /// <summary>Repair non-manifold, degenerate and isolated input as the reference's CornerTable does (CornerTable.cs:28-43)
    /// instead of refusing it.</summary>
    public bool RepairTopology { get; set; }

    /// <summary>With RepairTopology: also code meshes in corner form (UV charts, hard edges; with WeldPoints, what the weld makes of
    /// them) whose topology needs the repair, instead of failing them with NotImplementedException
    /// (dsa_encode_seam_repair_batch).  Unset: nothing changes.</summary>
    public bool RepairSeams { get; set; }

    /// <summary>Hand every mesh over as one row per point (the value of each attribute at the point, faces over points) and let the
    /// library weld the points into vertices (dsa_encode_points_batch): points with byte-equal positions, generic and extra rows
    /// are one vertex, normals and texture coordinates become corner attributes where a vertex has two of them.  For meshes whose
    /// point-to-value maps were never deduplicated (a glTF primitive or an OBJ loaded row by row).  Unset: nothing changes.</summary>
    public bool WeldPoints { get; set; }

    /// <summary>With WeldPoints: weld every attribute beyond the built-in slots alone, like normals and texture coordinates, instead
    /// of making its rows part of the vertex key (dsa_encode_corner_attributes_batch, weld_attributes 1): a lightmap UV set or a
    /// colour with a hard edge then cuts its own connectivity only.  An attribute past index 7 of the stream stays in the key.
    /// Unset: nothing changes.</summary>
    public bool WeldAttributes { get; set; }
    // TrackRows (dsa_encode_rows_batch, track_rows = 1): the encoder keeps, per stream and attribute, which row of the input every
    // entry of the stream carries -- the value index in the form the encoder is given (an attribute's own MappedIndex where it goes
    // per corner, the positions' where it goes per vertex), with WeldPoints the point of the per-point input; sequential streams and point clouds: the identity.  EntryRows(i) returns them
    // after Encode.  The streams are the bytes they are without it.  What carries morph targets across the weld and Edgebreaker's
    // renumbering.
    public bool TrackRows { get; set; }
    // PointOrder (dsa_encode_ordered_sequential_batch): 0 the points of a sequential stream or point cloud in the caller's order; 1 in
    // Morton order of their quantised positions, found on the device -- entry e of every attribute carries row perm[e] of the input,
    // faces are written through the inverse; EntryRows(i) returns perm for every attribute.  The format gives the order of a
    // sequential stream no meaning, and a scan or a shuffled sample codes to half its size or less this way.  Edgebreaker streams
    // order their own entries: with 1 an Edgebreaker encode throws.
    public int PointOrder { get; set; }
    // MergePoints (dsa_encode_merged_sequential_batch): 0 every point is coded; 1 one point per occupied cell of the position grid of a
    // point cloud -- of the points whose quantised positions are equal the one with the smallest row stays, entry j of every attribute
    // carries row kept[j], every quantised attribute keeps the bounds of all input rows.  EntryRows(i) returns kept for every
    // attribute, RowEntries(i) the entry of the cell of every input row.  Needs PointOrder 1; point clouds only: merging the points of
    // a mesh would collapse its faces, and an encode of meshes throws.
    public int MergePoints { get; set; }
    private uint[][] _rowEntries;
    // Of stream i of the most recent Encode with MergePoints: for every input row the entry of the stream whose cell the row lies in.
    public uint[] RowEntries(int i) => _rowEntries != null && i >= 0 && i < _rowEntries.Length ? _rowEntries[i] : throw new InvalidOperationException("no row entries: set MergePoints before Encode");
    // PartPoints (dsa_encode_split_sequential_batch): 0 one stream per cloud; N >= 1 the Morton order of every point cloud cut into
    // ceil(n / N) parts of at most N points, each an ordinary point-cloud stream on the cloud's one quantisation grid.  Encode then
    // returns one array per STREAM (the inputs in order, the parts of an input in order); Parts(i) names the streams of input i,
    // PartInfo(s) says which part stream s is and gives the box of its points, EntryRows(s) its slice of the order.  Needs
    // PointOrder 1 and MergePoints 0; point clouds only: a part of a mesh would need its faces cut, and an encode of meshes throws.
    public int PartPoints { get; set; }
    // PartCells (dsa_encode_cell_parts_sequential_batch): parts WITH MergePoints.  0 no parts; N >= 1 the kept order of every point
    // cloud -- one point per quantisation cell, m of them, a number only the device knows -- cut into ceil(m / N) parts of at most N
    // kept points, sized on the device.  Encode returns one array per STREAM as with PartPoints; Parts(i), PartInfo(s) (FirstEntry /
    // NumPoints in kept order) and EntryRows(s) serve the parts, RowEntries(Parts(i).First) the cloud's row entries in the global
    // kept order.  Needs PointOrder 1 and MergePoints 1, and PartPoints 0; point clouds only.
    public int PartCells { get; set; }
    // LodBaseBits (dsa_encode_lod_sequential_batch): additive levels of detail WITH PartCells.  0 no levels; D in 1 .. position bits
    // puts the kept points of every cloud into L = position bits - D + 1 levels -- levels 0 .. l together are exactly one point per
    // occupied cell of the grid with D + l bits per axis, the cell's first point in Morton order -- and cuts every level into parts
    // of at most PartCells points.  The streams of an input are the parts of level 0, then of level 1, ...; Parts(i), PartInfo(s),
    // EntryRows(s) and RowEntries(Parts(i).First) count in LOD order (kept by level, then by position in kept); LodInfo(s) says
    // which level stream s belongs to.  Needs PartCells >= 1 (and so PointOrder 1 and MergePoints 1); point clouds only.
    public int LodBaseBits { get; set; }
    public struct LodLevel
    {
        public uint Input, Level, Levels, CellBits, LevelFirstStream, LevelStreams, LevelPoints, PartInLevel;
    }
    private LodLevel[] _lodInfo;
    // Of stream s of the most recent Encode with LodBaseBits: which level it belongs to, and the streams and points of that level.
    public LodLevel LodInfo(int s) => _lodInfo != null && s >= 0 && s < _lodInfo.Length ? _lodInfo[s] : throw new InvalidOperationException("no levels: set LodBaseBits before Encode");
    // MeanAttributes (dsa_encode_mean_sequential_batch): the mean of the cell WITH MergePoints.  0 every attribute of a kept point
    // carries its own row; bit a set: attribute a of the stream (0 positions, then normals, texture coordinates, the generic attribute
    // and the listed attributes, those the cloud has) carries, per component, floor((2 S + cnt) / (2 cnt)) over the cnt input rows of
    // the cell, S the sum of the integers the plain call codes for them -- the exact mean, ties upwards, whatever the order of the
    // rows.  Positions and normals carry no mean: a cloud whose mask names them, or an attribute it does not have, fails alone.
    // PartCells and LodBaseBits compose with it; EntryRows, RowEntries, PartInfo and LodInfo are unchanged.  Needs MergePoints 1.
    public uint MeanAttributes { get; set; }
    // VoteAttributes (dsa_encode_vote_sequential_batch): the most frequent value of the cell WITH MergePoints, for labels -- a
    // classification, an instance id, a return number -- whose mean is a class nobody assigned.  Bit a set: attribute a of the stream
    // (counted as for MeanAttributes; 1 or 2 components) carries the tuple of coded integers that the most input rows of the cell
    // have, among tuples of equally many rows the lexicographically smallest (signed components, component 0 first), whatever the
    // order of the rows.  Positions, normals and attributes of 3 or 4 components are not voted on: a cloud whose mask names them, or
    // an attribute it does not have, fails alone.  An attribute takes the vote or the mean, not both.  Needs MergePoints 1.
    public uint VoteAttributes { get; set; }
    // MeanNormals (dsa_encode_normal_mean_sequential_batch): true: WITH MergePoints the normals of every cloud that has them carry, per
    // kept point, the code of the normalised sum of the unit normals of the cell's rows, by the rule in 64-bit integers on the
    // octahedral codes that the header states, whatever the order of the rows; a cell of one row keeps its code.  A cloud without
    // normals is coded as before.  PartCells, LodBaseBits, MeanAttributes and VoteAttributes compose with it.  Needs MergePoints 1.
    public bool MeanNormals { get; set; }
    // VoxelBits, VoxelPoint (dsa_encode_voxel_sequential_batch): VoxelBits = C >= 1: WITH MergePoints one point per occupied cell of the
    // grid with C bits per axis is kept, whatever PositionBits >= C the positions are stored at.  VoxelPoint: 0 the voxel's first row
    // in (key, row) order; 1 that row, its position coded as the exact integer mean of the voxel's quantised positions (ties
    // upwards); 2 the input row nearest the voxel's centre (ties to the smaller row).  MeanAttributes, VoteAttributes and MeanNormals
    // reduce over the voxel, PartCells cuts the kept voxels, LodBaseBits = D needs D <= C and gives C - D + 1 levels.
    public int VoxelBits { get; set; }
    public int VoxelPoint { get; set; }
    public struct PartBox
    {
        public uint Input, Part, Parts, FirstEntry, NumPoints, PositionBits;
        public int[] QMin, QMax;         // per component, over the position integers the stream codes
        public float[] BoxMin, BoxMax;   // what the decoder returns for them: the box of the part's decoded positions
    }
    private (uint First, uint Count)[] _parts;
    private PartBox[] _partInfo;
    // Of input i of the most recent Encode with PartPoints: its streams, first and count.
    public (uint First, uint Count) Parts(int i) => _parts != null && i >= 0 && i < _parts.Length ? _parts[i] : throw new InvalidOperationException("no parts: set PartPoints before Encode");
    // Of stream s of the most recent Encode with PartPoints: which part it is, and its box.
    public PartBox PartInfo(int s) => _partInfo != null && s >= 0 && s < _partInfo.Length ? _partInfo[s] : throw new InvalidOperationException("no parts: set PartPoints before Encode");
    private uint[][][] _entryRows;
    // Of stream i of the most recent Encode with TrackRows: per attribute of the stream (positions, then normals, texture coordinates,
    // generic where present, then the others) the row of the input every entry carries.
    public uint[][] EntryRows(int i) => _entryRows != null && i >= 0 && i < _entryRows.Length ? _entryRows[i] : throw new InvalidOperationException("no entry rows: set TrackRows before Encode");

    /// <summary>In corner form: an attribute beyond the built-in slots whose point-to-value map differs from the positions' keeps its
    /// own values, with an id per corner taken from that map (dsa_encode_corner_attributes_batch), instead of one value per position
    /// value.  The attribute must lie at index 1 to 7 of the stream.  Unset: nothing changes.</summary>
    public bool CornerAttributes { get; set; }

    // Quantisation grids (dsa_encode_grid_batch).  The reference's own options quantization_origin / quantization_range, set per
    // attribute type for positions or texture coordinates, are honoured as explicit grids (SequentialQuantizationAttributeEncoder.cs:
    // 19-23).  Groups, when set (one number per mesh of the batch), lets the meshes of one group share the grid of their positions:
    // the tiles of a surface, the primitives of one glTF mesh.  Edgebreaker meshes; unset, the calls and their bytes are what they were.
    public IReadOnlyList<uint> Groups { get; set; }

    private static bool ExplicitGrid(Config config, GeometryAttributeType type, int components, ref DsaQuantizationGrid grid)
    {
        if (!config.IsAttributeOptionSet((int)type, ConfigOptionName.Attribute.QuantizationOrigin) || !config.IsAttributeOptionSet((int)type, ConfigOptionName.Attribute.QuantizationRange)) return false;
        var origin = new List<float>(config.GetAttributeOptionValues<float>((int)type, ConfigOptionName.Attribute.QuantizationOrigin, components));
        for (int c = 0; c < components && c < origin.Count; ++c) grid.Origin[c] = origin[c];
        grid.Range = config.GetAttributeOption((int)type, ConfigOptionName.Attribute.QuantizationRange, 1.0f);
        grid.Mode = 1;
        return true;
    }

    // the grids of a batch, or null when no mesh has one
    private DsaMeshGrids[] Grids(Config config, int count)
    {
        var probe = new DsaQuantizationGrid();
        bool pos = ExplicitGrid(config, GeometryAttributeType.Position, 3, ref probe), uv = ExplicitGrid(config, GeometryAttributeType.TexCoord, 2, ref probe);
        if (!pos && !uv && Groups == null) return null;
        if (Groups != null && Groups.Count != count) throw new ArgumentException("Groups: one number per mesh of the batch");
        var grids = new DsaMeshGrids[count];
        for (int i = 0; i < count; ++i)
        {
            if (pos) ExplicitGrid(config, GeometryAttributeType.Position, 3, ref grids[i].Position);
            else if (Groups != null) grids[i].Position.Mode = 2;
            if (uv) ExplicitGrid(config, GeometryAttributeType.TexCoord, 2, ref grids[i].Texcoord);
            grids[i].Group = Groups != null ? Groups[i] : 0;
        }
        return grids;
    }

    public GpuDracoEncoder(int device = 0)
    {
        NativeMethods.Check(NativeMethods.dsa_context_create(device, IntPtr.Zero, out _ctx), IntPtr.Zero, "dsa_context_create");
    }

    /// <summary>Same contract as DracoEncoder.Encode(BinaryWriter, Config, PointCloud, attributes): writes one .drc stream.</summary>
    public void Encode(BinaryWriter writer, Config config, Mesh.Mesh mesh)
    {
        writer.Write(EncodeBatch(new[] { mesh }, config)[0]);
    }

    /// <summary>Point clouds (not meshes): sequential point-cloud streams, point i of the stream is point i of the cloud.</summary>
    public void Encode(BinaryWriter writer, Config config, PointCloud.PointCloud cloud)
    {
        if (cloud is Mesh.Mesh mesh) { Encode(writer, config, mesh); return; }
        writer.Write(EncodeSequential(new[] { cloud }, config, 0)[0]);
    }

    public byte[][] EncodeBatch(IReadOnlyList<PointCloud.PointCloud> clouds, Config config)
    {
        foreach (var c in clouds) if (c is Mesh.Mesh) throw new ArgumentException("a batch holds meshes or point clouds, not both");
        return EncodeSequential(clouds, config, 0);
    }

    // dsa_encode_sequential_batch: geometry 1 meshes, 0 point clouds; one value per point, in point order
    private byte[][] EncodeSequential(IReadOnlyList<PointCloud.PointCloud> items, Config config, int geometry)
    {
        NativeMethods.dsa_encode_sequential_default_options(out var so);
        so.Base.PositionBits = config.GetAttributeOption((int)GeometryAttributeType.Position, ConfigOptionName.Attribute.QuantizationBits, so.Base.PositionBits);
        so.Base.TexcoordBits = config.GetAttributeOption((int)GeometryAttributeType.TexCoord, ConfigOptionName.Attribute.QuantizationBits, so.Base.TexcoordBits);
        so.Base.NormalBits = config.GetAttributeOption((int)GeometryAttributeType.Normal, ConfigOptionName.Attribute.QuantizationBits, so.Base.NormalBits);
        so.Base.SymbolScheme = config.GetOption(ConfigOptionName.SymbolEncodingMethod, so.Base.SymbolScheme);
        so.Base.CompressionLevel = 10 - config.Speed;
        so.Geometry = geometry;
        so.CompressConnectivity = geometry == 1 && config.GetOption(ConfigOptionName.CompressConnectivity, false) ? 1 : 0;
        var inputs = new DsaMeshInput[items.Count];
        var pins = new List<GCHandle>();
        IntPtr encoded = IntPtr.Zero;
        try
        {
            bool anyExtras = false;
            foreach (var m in items) anyExtras = anyExtras || ExtraAttributes(m).Count > 0;
            for (int i = 0; i < items.Count; ++i)
            {
                var m = items[i];
                inputs[i].NumVertices = (uint)m.PointsCount;
                inputs[i].Positions = (float*)Pin(Floats(m, GeometryAttributeType.Position, 3), pins);
                inputs[i].Normals = (float*)Pin(Floats(m, GeometryAttributeType.Normal, 3), pins);
                inputs[i].Texcoords = (float*)Pin(Floats(m, GeometryAttributeType.TexCoord, 2), pins);
                var generic = Bytes(m, GeometryAttributeType.Generic, out uint genericComponents);
                inputs[i].Generic = (byte*)Pin(generic, pins);
                inputs[i].GenericComponents = generic == null ? 0 : genericComponents;
                if (geometry == 1 && m is Mesh.Mesh mesh)
                {
                    inputs[i].NumFaces = (uint)mesh.FacesCount;
                    var faces = new uint[mesh.FacesCount * 3];
                    for (int f = 0; f < mesh.FacesCount; ++f) { var face = mesh.GetFace((uint)f); faces[3 * f] = (uint)face[0]; faces[3 * f + 1] = (uint)face[1]; faces[3 * f + 2] = (uint)face[2]; }
                    inputs[i].Faces = (uint*)Pin(faces, pins);
                }
            }
            if (MeanAttributes != 0 && MergePoints != 1) throw new ArgumentException("MeanAttributes needs MergePoints 1: the mean is the mean over the points of a cell");
            if (VoteAttributes != 0 && MergePoints != 1) throw new ArgumentException("VoteAttributes needs MergePoints 1: the vote is a vote of the points of a cell");
            if (MeanNormals && MergePoints != 1) throw new ArgumentException("MeanNormals needs MergePoints 1: the mean normal is the mean over the points of a cell");
            if (VoxelBits != 0 && MergePoints != 1) throw new ArgumentException("VoxelBits needs MergePoints 1: a voxel keeps one of the points of a cell");
            if (VoxelPoint != 0 && VoxelBits == 0) throw new ArgumentException("VoxelPoint needs VoxelBits >= 1: the centroid and the nearest point are those of a voxel");
            if ((VoteAttributes & MeanAttributes) != 0) throw new ArgumentException("VoteAttributes and MeanAttributes share a bit: an attribute carries the most frequent value of its cell or the mean, not both");
            if (LodBaseBits != 0 && PartCells == 0) throw new ArgumentException("LodBaseBits needs PartCells >= 1: every level is cut into parts of at most PartCells points");
            if (PartPoints != 0 || PartCells != 0)
            {
                if (geometry != 0) throw new ArgumentException((PartCells != 0 ? "PartCells" : "PartPoints") + " takes point clouds: a part of a mesh would need its faces cut");
                NativeMethods.dsa_encode_default_split_options(out var po);
                po.Merge.Order.Sequential = so;
                po.Merge.Order.PointOrder = PointOrder;
                po.Merge.MergePoints = MergePoints;
                po.PartPoints = PartPoints;
                var ain = new DsaMeshAttrInput[items.Count];
                for (int i = 0; i < items.Count; ++i) { ain[i].Mesh.Mesh = inputs[i]; Extras(items[i], null, (uint)items[i].PointsCount, ref ain[i], pins); }
                if (VoxelBits != 0)             // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_voxel_options(out var xo);
                    xo.NormalMean.Vote.Mean.Lod.CellParts.Split = po;
                    xo.NormalMean.Vote.Mean.Lod.CellParts.PartCells = PartCells;
                    xo.NormalMean.Vote.Mean.Lod.LodBaseBits = LodBaseBits;
                    xo.NormalMean.Vote.Mean.MeanAttributes = MeanAttributes;
                    xo.NormalMean.Vote.VoteAttributes = VoteAttributes;
                    xo.NormalMean.MeanNormals = MeanNormals ? 1u : 0u;
                    xo.VoxelBits = VoxelBits;
                    xo.VoxelPoint = VoxelPoint;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_voxel_sequential_batch(_ctx, (uint)items.Count, p, null, in xo, out encoded), _ctx, "dsa_encode_voxel_sequential_batch");
                }
                else if (MeanNormals)           // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_normal_mean_options(out var no);
                    no.Vote.Mean.Lod.CellParts.Split = po;
                    no.Vote.Mean.Lod.CellParts.PartCells = PartCells;
                    no.Vote.Mean.Lod.LodBaseBits = LodBaseBits;
                    no.Vote.Mean.MeanAttributes = MeanAttributes;
                    no.Vote.VoteAttributes = VoteAttributes;
                    no.MeanNormals = 1;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_normal_mean_sequential_batch(_ctx, (uint)items.Count, p, null, in no, out encoded), _ctx, "dsa_encode_normal_mean_sequential_batch");
                }
                else if (VoteAttributes != 0)   // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_vote_options(out var vo);
                    vo.Mean.Lod.CellParts.Split = po;
                    vo.Mean.Lod.CellParts.PartCells = PartCells;
                    vo.Mean.Lod.LodBaseBits = LodBaseBits;
                    vo.Mean.MeanAttributes = MeanAttributes;
                    vo.VoteAttributes = VoteAttributes;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_vote_sequential_batch(_ctx, (uint)items.Count, p, null, in vo, out encoded), _ctx, "dsa_encode_vote_sequential_batch");
                }
                else if (MeanAttributes != 0)   // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_mean_options(out var eo);
                    eo.Lod.CellParts.Split = po;
                    eo.Lod.CellParts.PartCells = PartCells;
                    eo.Lod.LodBaseBits = LodBaseBits;
                    eo.MeanAttributes = MeanAttributes;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_mean_sequential_batch(_ctx, (uint)items.Count, p, null, in eo, out encoded), _ctx, "dsa_encode_mean_sequential_batch");
                }
                else if (LodBaseBits != 0)      // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_lod_options(out var lo);
                    lo.CellParts.Split = po;
                    lo.CellParts.PartCells = PartCells;
                    lo.LodBaseBits = LodBaseBits;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_lod_sequential_batch(_ctx, (uint)items.Count, p, null, in lo, out encoded), _ctx, "dsa_encode_lod_sequential_batch");
                }
                else if (PartCells != 0)        // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_cell_parts_options(out var co);
                    co.Split = po;
                    co.PartCells = PartCells;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_cell_parts_sequential_batch(_ctx, (uint)items.Count, p, null, in co, out encoded), _ctx, "dsa_encode_cell_parts_sequential_batch");
                }
                else
                fixed (DsaMeshAttrInput* p = ain)
                    NativeMethods.Check(NativeMethods.dsa_encode_split_sequential_batch(_ctx, (uint)items.Count, p, null, in po, out encoded), _ctx, "dsa_encode_split_sequential_batch");
                int streams = (int)NativeMethods.dsa_encoded_size(encoded);
                var split = Streams(encoded, streams);
                var parts = new (uint First, uint Count)[items.Count];
                for (uint i = 0; i < items.Count; ++i)
                    NativeMethods.Check(NativeMethods.dsa_encoded_parts(encoded, i, out parts[i].First, out parts[i].Count), _ctx, $"input {i}");
                var info = new PartBox[streams];
                for (uint s = 0; s < streams; ++s)
                {
                    NativeMethods.Check(NativeMethods.dsa_encoded_part_info(encoded, s, out var pi), _ctx, $"stream {s}");
                    info[s] = new PartBox { Input = pi.Input, Part = pi.Part, Parts = pi.Parts, FirstEntry = pi.FirstEntry, NumPoints = pi.NumPoints, PositionBits = pi.PositionBits,
                                            QMin = new[] { pi.QMin[0], pi.QMin[1], pi.QMin[2] }, QMax = new[] { pi.QMax[0], pi.QMax[1], pi.QMax[2] },
                                            BoxMin = new[] { pi.BoxMin[0], pi.BoxMin[1], pi.BoxMin[2] }, BoxMax = new[] { pi.BoxMax[0], pi.BoxMax[1], pi.BoxMax[2] } };
                }
                _parts = parts; _partInfo = info;
                if (LodBaseBits != 0)
                {
                    _lodInfo = new LodLevel[streams];
                    for (uint s = 0; s < streams; ++s)
                    {
                        NativeMethods.Check(NativeMethods.dsa_encoded_lod_info(encoded, s, out var li), _ctx, $"stream {s}");
                        _lodInfo[s] = new LodLevel { Input = li.Input, Level = li.Level, Levels = li.Levels, CellBits = li.CellBits, LevelFirstStream = li.LevelFirstStream,
                                                     LevelStreams = li.LevelStreams, LevelPoints = li.LevelPoints, PartInLevel = li.PartInLevel };
                    }
                }
                if (PartCells != 0)             // the row entries of every cloud, in the global kept order: kept with its first stream
                {
                    _rowEntries = new uint[streams][];
                    for (int i = 0; i < items.Count; ++i)
                    {
                        uint s = parts[i].First;
                        NativeMethods.Check(NativeMethods.dsa_encoded_row_entries(encoded, s, null, 0, out uint rows), _ctx, $"stream {s}");
                        _rowEntries[s] = new uint[rows];
                        fixed (uint* r = _rowEntries[s])
                            NativeMethods.Check(NativeMethods.dsa_encoded_row_entries(encoded, s, r, (nuint)rows, out rows), _ctx, $"stream {s}");
                    }
                }
                return split;
            }
            if (MergePoints != 0)
            {
                if (geometry != 0) throw new ArgumentException("MergePoints takes point clouds: merging the points of a mesh would collapse its faces and lose its seams");
                NativeMethods.dsa_encode_default_merge_options(out var mo);
                mo.Order.Sequential = so;
                mo.Order.PointOrder = PointOrder;
                mo.MergePoints = MergePoints;
                var ain = new DsaMeshAttrInput[items.Count];
                for (int i = 0; i < items.Count; ++i) { ain[i].Mesh.Mesh = inputs[i]; Extras(items[i], null, (uint)items[i].PointsCount, ref ain[i], pins); }
                if (VoxelBits != 0)             // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_voxel_options(out var xo);
                    xo.NormalMean.Vote.Mean.Lod.CellParts.Split.Merge = mo;
                    xo.NormalMean.Vote.Mean.MeanAttributes = MeanAttributes;
                    xo.NormalMean.Vote.VoteAttributes = VoteAttributes;
                    xo.NormalMean.MeanNormals = MeanNormals ? 1u : 0u;
                    xo.VoxelBits = VoxelBits;
                    xo.VoxelPoint = VoxelPoint;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_voxel_sequential_batch(_ctx, (uint)items.Count, p, null, in xo, out encoded), _ctx, "dsa_encode_voxel_sequential_batch");
                }
                else if (MeanNormals)           // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_normal_mean_options(out var no);
                    no.Vote.Mean.Lod.CellParts.Split.Merge = mo;
                    no.Vote.Mean.MeanAttributes = MeanAttributes;
                    no.Vote.VoteAttributes = VoteAttributes;
                    no.MeanNormals = 1;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_normal_mean_sequential_batch(_ctx, (uint)items.Count, p, null, in no, out encoded), _ctx, "dsa_encode_normal_mean_sequential_batch");
                }
                else if (VoteAttributes != 0)   // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_vote_options(out var vo);
                    vo.Mean.Lod.CellParts.Split.Merge = mo;
                    vo.Mean.MeanAttributes = MeanAttributes;
                    vo.VoteAttributes = VoteAttributes;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_vote_sequential_batch(_ctx, (uint)items.Count, p, null, in vo, out encoded), _ctx, "dsa_encode_vote_sequential_batch");
                }
                else if (MeanAttributes != 0)   // (the widest call only when its option is set)
                {
                    NativeMethods.dsa_encode_default_mean_options(out var eo);
                    eo.Lod.CellParts.Split.Merge = mo;
                    eo.MeanAttributes = MeanAttributes;
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_mean_sequential_batch(_ctx, (uint)items.Count, p, null, in eo, out encoded), _ctx, "dsa_encode_mean_sequential_batch");
                }
                else
                fixed (DsaMeshAttrInput* p = ain)
                    NativeMethods.Check(NativeMethods.dsa_encode_merged_sequential_batch(_ctx, (uint)items.Count, p, null, in mo, out encoded), _ctx, "dsa_encode_merged_sequential_batch");
                var merged = Streams(encoded, items.Count);
                _rowEntries = new uint[items.Count][];
                for (uint i = 0; i < items.Count; ++i)
                {
                    NativeMethods.Check(NativeMethods.dsa_encoded_row_entries(encoded, i, null, 0, out uint rows), _ctx, $"mesh {i}");
                    _rowEntries[i] = new uint[rows];
                    fixed (uint* r = _rowEntries[i])
                        NativeMethods.Check(NativeMethods.dsa_encoded_row_entries(encoded, i, r, (nuint)rows, out rows), _ctx, $"mesh {i}");
                }
                return merged;
            }
            if (PointOrder != 0)
            {
                NativeMethods.dsa_encode_default_order_options(out var oo);
                oo.Sequential = so;
                oo.PointOrder = PointOrder;
                var ain = new DsaMeshAttrInput[items.Count];
                for (int i = 0; i < items.Count; ++i) { ain[i].Mesh.Mesh = inputs[i]; Extras(items[i], null, (uint)items[i].PointsCount, ref ain[i], pins); }
                fixed (DsaMeshAttrInput* p = ain)
                    NativeMethods.Check(NativeMethods.dsa_encode_ordered_sequential_batch(_ctx, (uint)items.Count, p, null, in oo, out encoded), _ctx, "dsa_encode_ordered_sequential_batch");
                return Streams(encoded, items.Count);
            }
            if (anyExtras)
            {
                var ain = new DsaMeshAttrInput[items.Count];
                for (int i = 0; i < items.Count; ++i) { ain[i].Mesh.Mesh = inputs[i]; Extras(items[i], null, (uint)items[i].PointsCount, ref ain[i], pins); }
                fixed (DsaMeshAttrInput* p = ain)
                    NativeMethods.Check(NativeMethods.dsa_encode_attributes_sequential_batch(_ctx, (uint)items.Count, p, in so, out encoded), _ctx, "dsa_encode_attributes_sequential_batch");
                return Streams(encoded, items.Count);
            }
            fixed (DsaMeshInput* p = inputs)
                NativeMethods.Check(NativeMethods.dsa_encode_sequential_batch(_ctx, (uint)items.Count, p, in so, out encoded), _ctx, "dsa_encode_sequential_batch");
            return Streams(encoded, items.Count);
        }
        finally
        {
            if (encoded != IntPtr.Zero) NativeMethods.dsa_encoded_free(encoded);
            foreach (var h in pins) if (h.IsAllocated) h.Free();
        }
    }

    public byte[][] EncodeBatch(IReadOnlyList<Mesh.Mesh> meshes, Config config)
    {
        // an explicitly set EncodingMethod of SequentialEncoding: the sequential call (unset, or Edgebreaker: the call and its bytes
        // are what they were; the reference's speed-10 rule applies only where the option is unset, and stays Edgebreaker here)
        if (config.IsOptionSet(ConfigOptionName.EncodingMethod) && config.GetOption(ConfigOptionName.EncodingMethod, -1) == Constants.EncodingMethod.SequentialEncoding)
        {
            var items = new PointCloud.PointCloud[meshes.Count];
            for (int i = 0; i < meshes.Count; ++i) items[i] = meshes[i];
            return EncodeSequential(items, config, 1);
        }
        if (LodBaseBits != 0) throw new ArgumentException("LodBaseBits takes point clouds: levels of meshes are not built");
        if (PartCells != 0) throw new ArgumentException("PartCells takes point clouds: a part of a mesh would need its faces cut");
        if (PartPoints != 0) throw new ArgumentException("PartPoints takes point clouds: a part of a mesh would need its faces cut");
        if (MergePoints != 0) throw new ArgumentException("MergePoints takes point clouds: merging the points of a mesh would collapse its faces and lose its seams");
        if (PointOrder != 0) throw new ArgumentException("PointOrder needs a sequential stream (EncodingMethod SequentialEncoding, or point clouds): Edgebreaker orders its own entries");
        NativeMethods.dsa_encode_default_options(out var opt);
        // per-attribute-type options are keyed by (int)GeometryAttributeType (Config.cs:55-62)
        opt.PositionBits = config.GetAttributeOption((int)GeometryAttributeType.Position, ConfigOptionName.Attribute.QuantizationBits, opt.PositionBits);
        opt.TexcoordBits = config.GetAttributeOption((int)GeometryAttributeType.TexCoord, ConfigOptionName.Attribute.QuantizationBits, opt.TexcoordBits);
        opt.NormalBits = config.GetAttributeOption((int)GeometryAttributeType.Normal, ConfigOptionName.Attribute.QuantizationBits, opt.NormalBits);
        opt.SymbolScheme = config.GetOption(ConfigOptionName.SymbolEncodingMethod, opt.SymbolScheme);
        opt.CompressionLevel = 10 - config.Speed;
        // explicitly set schemes (ConfigOptionName.EdgeBreakerMethod, ConfigOptionName.Attribute.PredictionScheme) go through
        // dsa_encode_batch_ex; unset, the call and its bytes are what they were
        const int unset = int.MinValue;
        int ebMethod = config.GetOption(ConfigOptionName.EdgeBreakerMethod, unset);
        int uvScheme = config.GetAttributeOption((int)GeometryAttributeType.TexCoord, ConfigOptionName.Attribute.PredictionScheme, unset);
        int posScheme = config.GetAttributeOption((int)GeometryAttributeType.Position, ConfigOptionName.Attribute.PredictionScheme, unset);
        int normalScheme = config.GetAttributeOption((int)GeometryAttributeType.Normal, ConfigOptionName.Attribute.PredictionScheme, unset);
        if (uvScheme != unset) opt.TexcoordPrediction = uvScheme;
        if (posScheme != unset) opt.PositionPrediction = posScheme;
        bool extended = ebMethod != unset || normalScheme != unset;
        int multi = 0, traversal = 0;
        if (posScheme == 2 || posScheme == 4) { multi = posScheme; opt.PositionPrediction = 1; }      // (the options underneath keep the ids they take)
        else if (SpeedLadder && posScheme == unset) multi = -1;
        if (multi != 0 && uvScheme == multi) opt.TexcoordPrediction = 1;
        if (SpeedLadder && config.Speed == 0) traversal = 1;
        if (RepairSeams && !RepairTopology) throw new ArgumentException("RepairSeams codes attributes over the repaired corner table: it needs RepairTopology");
        if (WeldAttributes && !WeldPoints) throw new ArgumentException("WeldAttributes welds the attributes of per-point input each alone: it needs WeldPoints");
        _entryRows = null;
        var inputs = new DsaMeshInput[meshes.Count];
        var pins = new List<GCHandle>();
        IntPtr encoded = IntPtr.Zero;
        try
        {
            if (WeldPoints)
            {
                var pin = new DsaMeshAttrInput[meshes.Count];
                for (int i = 0; i < meshes.Count; ++i)
                {
                    var m = meshes[i];
                    ref DsaMeshInput mi = ref pin[i].Mesh.Mesh;
                    mi.NumVertices = (uint)m.PointsCount;
                    mi.NumFaces = (uint)m.FacesCount;
                    mi.Positions = (float*)Pin(Floats(m, GeometryAttributeType.Position, 3), pins);
                    mi.Normals = (float*)Pin(Floats(m, GeometryAttributeType.Normal, 3), pins);
                    mi.Texcoords = (float*)Pin(Floats(m, GeometryAttributeType.TexCoord, 2), pins);
                    var generic = Bytes(m, GeometryAttributeType.Generic, out uint genericComponents);
                    mi.Generic = (byte*)Pin(generic, pins);
                    mi.GenericComponents = generic == null ? 0 : genericComponents;
                    var faces = new uint[m.FacesCount * 3];
                    for (int f = 0; f < m.FacesCount; ++f) { var face = m.GetFace((uint)f); faces[3 * f] = (uint)face[0]; faces[3 * f + 1] = (uint)face[1]; faces[3 * f + 2] = (uint)face[2]; }
                    mi.Faces = (uint*)Pin(faces, pins);
                    Extras(m, null, (uint)m.PointsCount, ref pin[i], pins);      // (one row per point, as for a sequential stream)
                }
                NativeMethods.dsa_encode_default_repair_options(out var wp);
                wp.Level.Ex.Base = opt;
                wp.Level.Ex.EdgebreakerMethod = ebMethod != unset ? ebMethod : 0;
                wp.Level.Ex.NormalPrediction = normalScheme != unset ? normalScheme : 0;
                wp.Level.MultiParallelogram = multi;
                wp.Level.TraversalMethod = traversal;
                wp.Topology = RepairTopology ? 1 : 0;
                var wg = Grids(config, meshes.Count);
                if (wg != null) for (int i = 0; i < meshes.Count; ++i) if (pin[i].Mesh.Mesh.Texcoords == null) wg[i].Texcoord = default;
                if (WeldAttributes || TrackRows)
                {
                    NativeMethods.dsa_encode_default_corner_attributes_options(out var co);
                    co.SeamRepair.Grid.Repair = wp;
                    co.SeamRepair.Grid.WeldPoints = 1;
                    co.SeamRepair.CornerRepair = RepairSeams ? 1 : 0;
                    if (WeldAttributes) co.WeldAttributes = 1;
                    if (TrackRows)
                    {
                        NativeMethods.dsa_encode_default_rows_options(out var ro);
                        ro.CornerAttributes = co;
                        ro.TrackRows = 1;
                        fixed (DsaMeshAttrInput* p = pin) fixed (DsaMeshGrids* g = wg)
                            NativeMethods.Check(NativeMethods.dsa_encode_rows_batch(_ctx, (uint)meshes.Count, p, g, null, in ro, out encoded), _ctx, "dsa_encode_rows_batch");
                        return Streams(encoded, meshes.Count);
                    }
                    fixed (DsaMeshAttrInput* p = pin) fixed (DsaMeshGrids* g = wg)
                        NativeMethods.Check(NativeMethods.dsa_encode_corner_attributes_batch(_ctx, (uint)meshes.Count, p, g, null, in co, out encoded), _ctx, "dsa_encode_corner_attributes_batch");
                    return Streams(encoded, meshes.Count);
                }
                if (RepairSeams)
                {
                    NativeMethods.dsa_encode_default_seam_repair_options(out var so);
                    so.Grid.Repair = wp;
                    so.Grid.WeldPoints = 1;
                    so.CornerRepair = 1;
                    fixed (DsaMeshAttrInput* p = pin) fixed (DsaMeshGrids* g = wg)
                        NativeMethods.Check(NativeMethods.dsa_encode_seam_repair_batch(_ctx, (uint)meshes.Count, p, g, in so, out encoded), _ctx, "dsa_encode_seam_repair_batch");
                    return Streams(encoded, meshes.Count);
                }
                if (wg != null)
                {
                    NativeMethods.dsa_encode_default_grid_options(out var go);
                    go.Repair = wp;
                    go.WeldPoints = 1;
                    fixed (DsaMeshAttrInput* p = pin) fixed (DsaMeshGrids* g = wg)
                        NativeMethods.Check(NativeMethods.dsa_encode_grid_batch(_ctx, (uint)meshes.Count, p, g, in go, out encoded), _ctx, "dsa_encode_grid_batch");
                    return Streams(encoded, meshes.Count);
                }
                fixed (DsaMeshAttrInput* p = pin)
                    NativeMethods.Check(NativeMethods.dsa_encode_points_batch(_ctx, (uint)meshes.Count, p, in wp, out encoded), _ctx, "dsa_encode_points_batch");
                return Streams(encoded, meshes.Count);
            }
            bool anyCorners = false, anyExtras = false;
            foreach (var m in meshes) { anyCorners = anyCorners || NeedsCornerForm(m); anyExtras = anyExtras || ExtraAttributes(m).Count > 0; }
            var grids = Grids(config, meshes.Count);
            if (anyExtras || multi != 0 || traversal != 0 || RepairTopology || grids != null || TrackRows)
            {
                // the attribute list rides on the corner form (extras per vertex: the value of the last point of each position value)
                var ain = new DsaMeshAttrInput[meshes.Count];
                var acorners = CornerAttributes && anyExtras ? new DsaMeshAttributeCorners[meshes.Count] : null;
                bool anyAttributeIds = false;
                for (int i = 0; i < meshes.Count; ++i)
                {
                    CornerForm(meshes[i], ref ain[i].Mesh, pins);
                    if (acorners == null) Extras(meshes[i], meshes[i].GetNamedAttribute(GeometryAttributeType.Position), ain[i].Mesh.Mesh.NumVertices, ref ain[i], pins);
                    else anyAttributeIds = CornerExtras(meshes[i], ain[i].Mesh.Mesh.NumVertices, ref ain[i], ref acorners[i], pins) || anyAttributeIds;
                }
                NativeMethods.dsa_encode_default_options_ex(out var ax);
                ax.Base = opt;
                ax.EdgebreakerMethod = ebMethod != unset ? ebMethod : 0;
                ax.NormalPrediction = normalScheme != unset ? normalScheme : 0;
                if (grids != null) for (int i = 0; i < meshes.Count; ++i) if (ain[i].Mesh.Mesh.Texcoords == null) grids[i].Texcoord = default;
                if (anyAttributeIds || TrackRows)
                {
                    NativeMethods.dsa_encode_default_corner_attributes_options(out var co);
                    co.SeamRepair.Grid.Repair.Level.Ex = ax;
                    co.SeamRepair.Grid.Repair.Level.MultiParallelogram = multi;
                    co.SeamRepair.Grid.Repair.Level.TraversalMethod = traversal;
                    co.SeamRepair.Grid.Repair.Topology = RepairTopology ? 1 : 0;
                    co.SeamRepair.CornerRepair = RepairSeams ? 1 : 0;
                    if (TrackRows)
                    {
                        NativeMethods.dsa_encode_default_rows_options(out var ro);
                        ro.CornerAttributes = co;
                        ro.TrackRows = 1;
                        fixed (DsaMeshAttrInput* p = ain) fixed (DsaMeshGrids* g = grids) fixed (DsaMeshAttributeCorners* c = acorners)
                            NativeMethods.Check(NativeMethods.dsa_encode_rows_batch(_ctx, (uint)meshes.Count, p, g, c, in ro, out encoded), _ctx, "dsa_encode_rows_batch");
                        return Streams(encoded, meshes.Count);
                    }
                    fixed (DsaMeshAttrInput* p = ain) fixed (DsaMeshGrids* g = grids) fixed (DsaMeshAttributeCorners* c = acorners)
                        NativeMethods.Check(NativeMethods.dsa_encode_corner_attributes_batch(_ctx, (uint)meshes.Count, p, g, c, in co, out encoded), _ctx, "dsa_encode_corner_attributes_batch");
                    return Streams(encoded, meshes.Count);
                }
                if (RepairSeams)
                {
                    NativeMethods.dsa_encode_default_seam_repair_options(out var so);
                    so.Grid.Repair.Level.Ex = ax;
                    so.Grid.Repair.Level.MultiParallelogram = multi;
                    so.Grid.Repair.Level.TraversalMethod = traversal;
                    so.Grid.Repair.Topology = 1;
                    so.CornerRepair = 1;
                    fixed (DsaMeshAttrInput* p = ain) fixed (DsaMeshGrids* g = grids)
                        NativeMethods.Check(NativeMethods.dsa_encode_seam_repair_batch(_ctx, (uint)meshes.Count, p, g, in so, out encoded), _ctx, "dsa_encode_seam_repair_batch");
                    return Streams(encoded, meshes.Count);
                }
                if (grids != null)
                {
                    NativeMethods.dsa_encode_default_grid_options(out var go);
                    go.Repair.Level.Ex = ax;
                    go.Repair.Level.MultiParallelogram = multi;
                    go.Repair.Level.TraversalMethod = traversal;
                    go.Repair.Topology = RepairTopology ? 1 : 0;
                    fixed (DsaMeshAttrInput* p = ain) fixed (DsaMeshGrids* g = grids)
                        NativeMethods.Check(NativeMethods.dsa_encode_grid_batch(_ctx, (uint)meshes.Count, p, g, in go, out encoded), _ctx, "dsa_encode_grid_batch");
                    return Streams(encoded, meshes.Count);
                }
                if (multi != 0 || traversal != 0 || RepairTopology)
                {
                    NativeMethods.dsa_encode_default_level_options(out var lv);
                    lv.Ex = ax;
                    lv.MultiParallelogram = multi;
                    lv.TraversalMethod = traversal;
                    if (RepairTopology)
                    {
                        NativeMethods.dsa_encode_default_repair_options(out var rp);
                        rp.Level = lv;
                        rp.Topology = 1;
                        fixed (DsaMeshAttrInput* p = ain)
                            NativeMethods.Check(NativeMethods.dsa_encode_repair_batch(_ctx, (uint)meshes.Count, p, in rp, out encoded), _ctx, "dsa_encode_repair_batch");
                        return Streams(encoded, meshes.Count);
                    }
                    fixed (DsaMeshAttrInput* p = ain)
                        NativeMethods.Check(NativeMethods.dsa_encode_level_batch(_ctx, (uint)meshes.Count, p, in lv, out encoded), _ctx, "dsa_encode_level_batch");
                    return Streams(encoded, meshes.Count);
                }
                fixed (DsaMeshAttrInput* p = ain)
                    NativeMethods.Check(NativeMethods.dsa_encode_attributes_batch(_ctx, (uint)meshes.Count, p, in ax, out encoded), _ctx, "dsa_encode_attributes_batch");
                return Streams(encoded, meshes.Count);
            }
            if (anyCorners || extended)
            {
                var cin = new DsaMeshCornerInput[meshes.Count];
                for (int i = 0; i < meshes.Count; ++i) CornerForm(meshes[i], ref cin[i], pins);
                fixed (DsaMeshCornerInput* p = cin)
                {
                    if (extended)
                    {
                        NativeMethods.dsa_encode_default_options_ex(out var ex);
                        ex.Base = opt;
                        ex.EdgebreakerMethod = ebMethod != unset ? ebMethod : 0;
                        ex.NormalPrediction = normalScheme != unset ? normalScheme : 0;
                        NativeMethods.Check(NativeMethods.dsa_encode_batch_ex(_ctx, (uint)meshes.Count, p, in ex, out encoded), _ctx, "dsa_encode_batch_ex");
                    }
                    else
                        NativeMethods.Check(NativeMethods.dsa_encode_batch_corners(_ctx, (uint)meshes.Count, p, in opt, out encoded), _ctx, "dsa_encode_batch_corners");
                }
                return Streams(encoded, meshes.Count);
            }
            for (int i = 0; i < meshes.Count; ++i)
            {
                var m = meshes[i];
                inputs[i].NumVertices = (uint)m.PointsCount;
                inputs[i].NumFaces = (uint)m.FacesCount;
                inputs[i].Positions = (float*)Pin(Floats(m, GeometryAttributeType.Position, 3), pins);
                inputs[i].Normals = (float*)Pin(Floats(m, GeometryAttributeType.Normal, 3), pins);
                inputs[i].Texcoords = (float*)Pin(Floats(m, GeometryAttributeType.TexCoord, 2), pins);
                var generic = Bytes(m, GeometryAttributeType.Generic, out uint genericComponents);      // uint8 attributes of 1 - 4 components
                inputs[i].Generic = (byte*)Pin(generic, pins);
                inputs[i].GenericComponents = generic == null ? 0 : genericComponents;
                var faces = new uint[m.FacesCount * 3];
                for (int f = 0; f < m.FacesCount; ++f) { var face = m.GetFace((uint)f); faces[3 * f] = (uint)face[0]; faces[3 * f + 1] = (uint)face[1]; faces[3 * f + 2] = (uint)face[2]; }
                inputs[i].Faces = (uint*)Pin(faces, pins);
            }
            fixed (DsaMeshInput* p = inputs)
                NativeMethods.Check(NativeMethods.dsa_encode_batch(_ctx, (uint)meshes.Count, p, in opt, out encoded), _ctx, "dsa_encode_batch");
            return Streams(encoded, meshes.Count);
        }
        finally
        {
            if (encoded != IntPtr.Zero) NativeMethods.dsa_encoded_free(encoded);
            foreach (var h in pins) if (h.IsAllocated) h.Free();
        }
    }

    private byte[][] Streams(IntPtr encoded, int count)
    {
        var result = new byte[count][];
        for (uint i = 0; i < count; ++i)
        {
            NativeMethods.Check(NativeMethods.dsa_encoded_stream(encoded, i, out var bytes, out var length), _ctx, $"mesh {i}");
            result[i] = new ReadOnlySpan<byte>(bytes, (int)length).ToArray();
        }
        _rowEntries = null; _parts = null; _partInfo = null; _lodInfo = null;
        if (TrackRows || PointOrder != 0) _entryRows = Rows(encoded, count);      // (a sequential handle answers with the identity, or with the point order)
        return result;
    }

    // dsa_encoded_entry_rows of every stream, for the attributes dsa_encoded_attributes counts
    private uint[][][] Rows(IntPtr encoded, int count)
    {
        var result = new uint[count][][];
        for (uint i = 0; i < count; ++i)
        {
            NativeMethods.Check(NativeMethods.dsa_encoded_attributes(encoded, i, out uint attributes), _ctx, $"mesh {i}");
            result[i] = new uint[attributes][];
            for (uint a = 0; a < attributes; ++a)
            {
                NativeMethods.Check(NativeMethods.dsa_encoded_entry_rows(encoded, i, a, null, 0, out uint entries), _ctx, $"mesh {i}");
                result[i][a] = new uint[entries];
                fixed (uint* r = result[i][a])
                    NativeMethods.Check(NativeMethods.dsa_encoded_entry_rows(encoded, i, a, r, (nuint)entries, out entries), _ctx, $"mesh {i}");
            }
        }
        return result;
    }

    // corner form when the points do not map one to one onto position values, or a normal / texture coordinate mapping differs
    // from the position mapping
    private static bool NeedsCornerForm(Mesh.Mesh m)
    {
        var pa = m.GetNamedAttribute(GeometryAttributeType.Position);
        if (pa == null) return false;
        var seen = new bool[Math.Max(pa.UniqueEntriesCount, (uint)m.PointsCount)];
        for (uint p = 0; p < m.PointsCount; ++p)
        {
            uint v = pa.MappedIndex(p);
            if (v >= seen.Length || seen[v]) return true;
            seen[v] = true;
        }
        return SeparateIds(m, pa, GeometryAttributeType.Normal) || SeparateIds(m, pa, GeometryAttributeType.TexCoord);
    }

    private static bool SeparateIds(Mesh.Mesh m, PointAttribute pa, GeometryAttributeType type)
    {
        var a = m.GetNamedAttribute(type);
        if (a == null) return false;
        for (uint p = 0; p < m.PointsCount; ++p) if (a.MappedIndex(p) != pa.MappedIndex(p)) return true;
        return false;
    }

    // Vertices = position values, faces = the position value of every corner; a normal / texture coordinate attribute whose mapping
    // differs from the positions' keeps its own values with an id per corner, otherwise it is per vertex.  The generic attribute is
    // per vertex (the value of the last point of each position value).
    private static void CornerForm(Mesh.Mesh m, ref DsaMeshCornerInput c, List<GCHandle> pins)
    {
        var pa = m.GetNamedAttribute(GeometryAttributeType.Position)!;
        uint nv = 0;
        for (uint p = 0; p < m.PointsCount; ++p) nv = Math.Max(nv, pa.MappedIndex(p) + 1);
        var faces = new uint[m.FacesCount * 3];
        var pointOf = new uint[m.FacesCount * 3];
        for (int f = 0; f < m.FacesCount; ++f)
        {
            var face = m.GetFace((uint)f);
            for (int k = 0; k < 3; ++k) { pointOf[3 * f + k] = (uint)face[k]; faces[3 * f + k] = pa.MappedIndex((uint)face[k]); }
        }
        c.Mesh.NumVertices = nv;
        c.Mesh.NumFaces = (uint)m.FacesCount;
        c.Mesh.Faces = (uint*)Pin(faces, pins);
        c.Mesh.Positions = (float*)Pin(Values(pa, nv, 3), pins);
        c.Mesh.Normals = (float*)Pin(PerCornerOrVertex(m, pa, GeometryAttributeType.Normal, 3, nv, pointOf, out var nid, out c.NumNormals), pins);
        c.NormalCorners = (uint*)Pin(nid, pins);
        c.Mesh.Texcoords = (float*)Pin(PerCornerOrVertex(m, pa, GeometryAttributeType.TexCoord, 2, nv, pointOf, out var tid, out c.NumTexcoords), pins);
        c.TexcoordCorners = (uint*)Pin(tid, pins);
        var generic = Bytes(m, GeometryAttributeType.Generic, out uint gc);
        if (generic != null)
        {
            var g = new byte[nv * gc];
            for (uint p = 0; p < m.PointsCount; ++p) Array.Copy(generic, p * gc, g, pa.MappedIndex(p) * gc, gc);
            c.Mesh.Generic = (byte*)Pin(g, pins);
            c.Mesh.GenericComponents = gc;
        }
    }

    private static float[]? PerCornerOrVertex(Mesh.Mesh m, PointAttribute pa, GeometryAttributeType type, int nc, uint nv, uint[] pointOf, out uint[]? ids, out uint rows)
    {
        ids = null;
        rows = 0;
        var a = m.GetNamedAttribute(type);
        if (a == null) return null;
        if (!SeparateIds(m, pa, type))
        {
            var v = new float[nv * nc];
            for (uint p = 0; p < m.PointsCount; ++p)
                for (int c = 0; c < nc; ++c) v[pa.MappedIndex(p) * nc + c] = a.Buffer!.Read<float>((int)(a.ByteOffset + a.MappedIndex(p) * a.ByteStride + 4 * c));
            return v;
        }
        ids = new uint[pointOf.Length];
        for (int k = 0; k < pointOf.Length; ++k) { ids[k] = a.MappedIndex(pointOf[k]); rows = Math.Max(rows, ids[k] + 1); }
        return Values(a, rows, nc);
    }

    // the first `count` values of a float attribute, by value index
    private static float[] Values(PointAttribute a, uint count, int nc)
    {
        var v = new float[count * nc];
        for (uint i = 0; i < count; ++i)
            for (int c = 0; c < nc; ++c) v[i * nc + c] = a.Buffer!.Read<float>((int)(a.ByteOffset + i * a.ByteStride + 4 * c));
        return v;
    }

    // values of a per-vertex float attribute in point order (null when the mesh has no such attribute)
    private static float[]? Floats(PointCloud.PointCloud m, GeometryAttributeType type, int nc)
    {
        var a = m.GetNamedAttribute(type);
        if (a == null) return null;
        var v = new float[m.PointsCount * nc];
        for (uint p = 0; p < m.PointsCount; ++p)
            for (int c = 0; c < nc; ++c) v[p * nc + c] = a.Buffer!.Read<float>((int)(a.ByteOffset + a.MappedIndex(p) * a.ByteStride + 4 * c));
        return v;
    }

    // a uint8 attribute of 1 - 4 components per point (the first of its type), or null
    private static byte[]? Bytes(PointCloud.PointCloud m, GeometryAttributeType type, out uint nc)
    {
        nc = 0;
        var a = m.GetNamedAttribute(type);
        if (a == null || a.DataType != DataType.UInt8 || a.NumComponents < 1 || a.NumComponents > 4) return null;
        nc = (uint)a.NumComponents;
        var v = new byte[m.PointsCount * nc];
        for (uint p = 0; p < m.PointsCount; ++p)
            for (int c = 0; c < nc; ++c) v[p * nc + c] = a.Buffer!.Read<byte>((int)(a.ByteOffset + a.MappedIndex(p) * a.ByteStride + c));
        return v;
    }

    // The attributes the built-in slots do not take, in the cloud's order: everything but the first position, normal and texture
    // coordinate attribute and the generic attribute Bytes() passes as DsaMeshInput.Generic.
    private static List<PointAttribute> ExtraAttributes(PointCloud.PointCloud m)
    {
        var builtin = new HashSet<PointAttribute>();
        foreach (var t in new[] { GeometryAttributeType.Position, GeometryAttributeType.Normal, GeometryAttributeType.TexCoord })
        {
            var a = m.GetNamedAttribute(t);
            if (a != null) builtin.Add(a);
        }
        var g = m.GetNamedAttribute(GeometryAttributeType.Generic);
        if (g != null && g.DataType == DataType.UInt8 && g.NumComponents >= 1 && g.NumComponents <= 4) builtin.Add(g);
        var extras = new List<PointAttribute>();
        foreach (var a in m.Attributes) if (!builtin.Contains(a)) extras.Add(a);
        return extras;
    }

    private static int ElementSize(DataType t) => t switch
    {
        DataType.Int8 or DataType.UInt8 => 1,
        DataType.Int16 or DataType.UInt16 => 2,
        DataType.Int32 or DataType.UInt32 or DataType.Float32 => 4,
        _ => throw new NotSupportedException($"attribute data type {t}: the encoder takes Int8 .. UInt32 and Float32"),
    };

    // dsa_mesh_attr_input.attributes of a cloud: one packed row per vertex (pa null: per point; else per position value, the value of
    // the last point of each), read at ByteOffset + ByteStride * id like GeometryAttribute does
    private static void Extras(PointCloud.PointCloud m, PointAttribute? pa, uint nv, ref DsaMeshAttrInput dst, List<GCHandle> pins)
    {
        var extras = ExtraAttributes(m);
        if (extras.Count == 0) return;
        var list = new DsaAttributeInput[extras.Count];
        for (int k = 0; k < extras.Count; ++k)
        {
            var a = extras[k];
            if (a.AttributeType != GeometryAttributeType.Color && a.AttributeType != GeometryAttributeType.TexCoord && a.AttributeType != GeometryAttributeType.Generic)
                throw new NotSupportedException($"a second attribute of type {a.AttributeType}: extras are colours, texture coordinates and generic attributes");
            if (a.NumComponents < 1 || a.NumComponents > 4) throw new NotSupportedException("attributes of more than four components");
            int row = ElementSize(a.DataType) * a.NumComponents;
            var bytes = new byte[nv * row];
            for (uint p = 0; p < m.PointsCount; ++p)
            {
                long src = a.ByteOffset + (long)a.MappedIndex(p) * a.ByteStride;
                long at = (long)(pa == null ? p : pa.MappedIndex(p)) * row;
                for (int b = 0; b < row; ++b) bytes[at + b] = a.Buffer!.Read<byte>((int)(src + b));
            }
            list[k].AttributeType = (int)a.AttributeType;
            list[k].DataType = (int)a.DataType;
            list[k].NumComponents = (uint)a.NumComponents;
            list[k].Normalized = a.Normalized && a.DataType != DataType.Float32 ? 1 : 0;
            list[k].UniqueId = a.UniqueId;
            list[k].QuantizationBits = 0;
            list[k].Values = (void*)Pin(bytes, pins);
        }
        dst.Attributes = (DsaAttributeInput*)Pin(list, pins);
        dst.NumAttributes = (uint)extras.Count;
    }

    // Extras() for the corner form with CornerAttributes: an attribute whose point-to-value map differs from the positions' keeps its
    // own values (one packed row per value index) and gets an id per corner from that map; every other attribute is per vertex as in
    // Extras().  Returns whether any attribute got ids.
    private static bool CornerExtras(Mesh.Mesh m, uint nv, ref DsaMeshAttrInput dst, ref DsaMeshAttributeCorners corners, List<GCHandle> pins)
    {
        var pa = m.GetNamedAttribute(GeometryAttributeType.Position)!;
        Extras(m, pa, nv, ref dst, pins);
        var extras = ExtraAttributes(m);
        if (extras.Count == 0) return false;
        var list = new DsaAttributeCorners[extras.Count];
        bool any = false;
        for (int k = 0; k < extras.Count; ++k)
        {
            var a = extras[k];
            bool separate = false;
            for (uint p = 0; p < m.PointsCount && !separate; ++p) separate = a.MappedIndex(p) != pa.MappedIndex(p);
            if (!separate) continue;
            var ids = new uint[m.FacesCount * 3];
            uint rows = 0;
            for (int f = 0; f < m.FacesCount; ++f)
            {
                var face = m.GetFace((uint)f);
                for (int c = 0; c < 3; ++c) { ids[3 * f + c] = a.MappedIndex((uint)face[c]); rows = Math.Max(rows, ids[3 * f + c] + 1); }
            }
            int row = ElementSize(a.DataType) * a.NumComponents;
            var bytes = new byte[rows * row];
            for (uint v = 0; v < rows; ++v)
            {
                long src = a.ByteOffset + (long)v * a.ByteStride;
                for (int b = 0; b < row; ++b) bytes[(long)v * row + b] = a.Buffer!.Read<byte>((int)(src + b));
            }
            dst.Attributes[k].Values = (void*)Pin(bytes, pins);
            list[k].Corners = (uint*)Pin(ids, pins);
            list[k].NumRows = rows;
            any = true;
        }
        if (any) corners.Attributes = (DsaAttributeCorners*)Pin(list, pins);
        return any;
    }

    private static IntPtr Pin(Array? a, List<GCHandle> pins)
    {
        if (a == null) return IntPtr.Zero;
        var h = GCHandle.Alloc(a, GCHandleType.Pinned);
        pins.Add(h);
        return h.AddrOfPinnedObject();
    }

    public void Dispose()
    {
        if (_ctx != IntPtr.Zero) { NativeMethods.dsa_context_destroy(_ctx); _ctx = IntPtr.Zero; }
    }
}
