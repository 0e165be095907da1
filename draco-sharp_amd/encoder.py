"""Host-side mirror of the reference's encode surface for the GPU path:

  DracoEncoder.Encode(BinaryWriter, Config, PointCloud, attributes)     src/Draco/IO/DracoEncoder.cs:22-41
  Config (quantisation bits, speed, prediction overrides)              src/Draco/IO/Config.cs

bound to the dsa_encode_* entry points of libdraco_mi355x.so.  Connectivity (corner table, Edgebreaker symbols, attribute
order), attribute quantisation / prediction / rANS coding are HIP kernels; the library's host side chooses the symbol schemes
and lays the bytes out; there is no CPU fallback."""
import ctypes as C
import os
import time

import numpy as np

from . import native
from .decoder import DeviceException, _raise, default_context


def _shared(meshes, table, what):
    """table(m) of the clouds of a call, which a mask over the attributes of the stream (`what`) needs to be one; None without clouds"""
    tables = {table(m) for m in meshes}
    if len(tables) > 1:
        raise ValueError("%s is one mask for the call: its clouds must have the same attributes (give a mask per call otherwise)" % what)
    return tables.pop() if tables else None


class Config:
    """Subset of src/Draco/IO/Config.cs that the device path honours.

    The method ids are the format's own: edgebreaker_method 0 standard, 2 valence, -1 the reference's rule per mesh (valence at
    speed < 5 for meshes of 1000 faces or more); position_prediction 0 difference, 1 parallelogram; texcoord_prediction also 5
    TexCoordsPortable; normal_prediction 0 difference, 6 GeometricNormal.  Defaults write what the speed-5 default writes.

    encoding_method (Constants.cs EncodingMethod): 1 Edgebreaker (default), 0 sequential -- faces as point indices, points and
    faces in the caller's order, any list of triangles legal -- or -1 the reference's rule (DracoEncoder.cs:43-57: sequential
    exactly when speed == 10).  compress_connectivity (ConfigOptionName.CompressConnectivity) chooses compressed over raw indices
    of a sequential mesh.  A sequential stream predicts by Difference: the prediction and connectivity options above do not shape it.

    The levels above the default (dsa_encode_level_batch): multi_parallelogram 4 writes ConstrainedMultiParallelogram, 2
    MultiParallelogram, in place of Parallelogram (positions and the first UV set; with 4 and parallelogram positions also the
    generic attribute and the attribute list), -1 the reference's rule per mesh (4 at speed < 2 for meshes of 40 points or more);
    traversal_method 1 sequences the positions' decoder (every decoder under single_connectivity) in prediction-degree order, 2
    every decoder without interior seams.  Sequential configs and point clouds refuse both: they predict by Difference in point order.

    repair_topology (dsa_encode_repair_batch, topology 1): meshes with degenerate faces, the same face twice, fins, faces turned
    over, fans that meet at a vertex or vertices no face uses are coded on the reference's repaired corner table (CornerTable.cs:
    28-43) instead of being refused; clean meshes give the same bytes.  Edgebreaker streams only; attributes given per corner over
    a mesh that needs the repair are refused as not implemented, unless repair_seams is set.

    repair_seams (dsa_encode_seam_repair_batch, corner_repair 1; needs repair_topology): a mesh that needs the repair and carries
    normal_corners / texcoord_corners -- or, with weld_points, UV charts and hard edges -- is coded: the ids of the faces that are
    not degenerate over the repaired table, its cut edges boundaries of every attribute.  Every other mesh gives the bytes it gave.

    weld_points (dsa_encode_points_batch): the rows of a MeshData are per point, not per vertex -- a glTF primitive, an OBJ after
    triangulation, Batch.vertex_arrays: points are duplicated wherever a UV chart or a hard edge passes.  Points with byte-equal
    positions, generic and attribute rows are welded into one vertex, normals and texture coordinates go on per corner (or per
    vertex where no vertex has two), and the welded mesh is coded with the other options as they are.  Edgebreaker streams of
    meshes without corner ids only.

    weld_attributes (dsa_encode_corner_attributes_batch; needs weld_points): the attributes of the list leave the vertex key and
    are welded each alone, like normals and texture coordinates -- a lightmap UV set with its own charts or a colour with a hard
    edge then cuts its own connectivity only, and positions are not duplicated along its seams.  An attribute whose index in the
    stream is above 7 stays in the vertex key (the decoder takes corner attributes for attribute data 0 to 6).

    track_rows (dsa_encode_rows_batch): the result keeps, per stream and attribute, which row of the arrays passed every entry of
    the stream carries (EncodedStreams.entry_rows) -- what carries morph targets or simulation state across Edgebreaker's
    renumbering, the repair's new vertices and the weld.  The streams are the bytes they are without it; 4 bytes per entry and
    attribute are kept.  Sequential streams need no tracking: their entry i is row i.

    point_order (dsa_encode_ordered_sequential_batch): 0 the points of a sequential stream in the caller's order; 1
    (POINT_ORDER_MORTON) in Morton order of their quantised positions, found on the device -- entry e of every attribute carries
    row perm[e] of the caller's arrays, faces are written through the inverse.  The format gives the order of a sequential stream
    no meaning, and a scan or a shuffled sample codes to half its size or less this way.  EncodedStreams.entry_rows(i) returns
    perm (the same for every attribute) and Batch.source_rows carries side data across.  Sequential streams and point clouds
    only: Edgebreaker orders its own entries.

    merge_points (dsa_encode_merged_sequential_batch): 0 every point is coded; 1 (MERGE_CELLS) one point per occupied cell of the
    position grid -- of the points whose quantised positions are equal the one with the smallest row stays, entry j of every
    attribute carries row kept[j], and every quantised attribute keeps the bounds of all input rows.  With Grid(origin, range) on
    the positions the voxel is range / (2^position_bits - 1).  EncodedStreams.entry_rows(i) returns kept (for every attribute),
    EncodedStreams.row_entries(i) the entry of the cell of every input row (what averages colours or counts points per cell).
    Point clouds only, under a sequential config with point_order=POINT_ORDER_MORTON: the points of a cell lie side by side in
    that order, and merging the points of a mesh would collapse its faces.

    part_points (dsa_encode_split_sequential_batch): 0 one stream per cloud; N >= 1 the Morton order of every point cloud cut into
    P = ceil(n / N) parts of at most N points, part p sorted entries [floor(p n / P), floor((p + 1) n / P)), each an ordinary
    point-cloud stream of its own on the cloud's one quantisation grid -- streams that encode and decode side by side, fit
    together without cracks, and come with a box each.  The EncodedStreams then runs over STREAMS (inputs in order, the parts of
    an input in order): parts(i) is the range of input i's streams, part_info(s) says which part stream s is and gives its box,
    entry_rows(s) its slice of the order.  Point clouds only, under a sequential config with point_order=POINT_ORDER_MORTON and
    without merge_points.

    part_cells (dsa_encode_cell_parts_sequential_batch): parts WITH merge_points=MERGE_CELLS.  0 no parts; N >= 1 the kept order of
    every point cloud -- kept[0 .. m) as merge_points defines it, m a number only the device knows -- cut into P = ceil(m / N) parts
    of at most N kept points, part p kept entries [floor(p m / P), floor((p + 1) m / P)), each an ordinary point-cloud stream on the
    cloud's one quantisation grid (the bounds of all n input rows).  The EncodedStreams runs over STREAMS as with part_points:
    parts(i), part_info(s) (first_entry / num_points in kept order) and entry_rows(s) = kept[lo:hi]; row_entries(parts(i)[0]) is the
    cloud's row_entries in the global kept order, row_parts(i) turns it into (part, entry) per input row.  Needs a sequential config
    with point_order=POINT_ORDER_MORTON and merge_points=MERGE_CELLS, and no part_points.

    lod_base_bits (dsa_encode_lod_sequential_batch): additive levels of detail WITH part_cells.  0 no levels; D in 1 .. position_bits
    puts the kept points of every cloud into L = position_bits - D + 1 levels -- levels 0 .. l together are exactly one point per
    occupied cell of the grid with D + l bits per axis, the cell's first point in Morton order -- and cuts every level into parts of
    at most part_cells points (part_cells >= n: one stream per level).  The streams of an input are the parts of level 0, then of
    level 1, ...; parts(i), part_info(s), entry_rows(s), row_entries(parts(i)[0]) and row_parts(i) count in LOD order (kept by
    ascending (level, position in kept)); lod_info(s) says which level stream s belongs to, levels(i) gives the streams of every
    level.  Needs part_cells >= 1 (and so point_order=POINT_ORDER_MORTON and merge_points=MERGE_CELLS).

    mean_attributes (dsa_encode_mean_sequential_batch): the mean of the cell WITH merge_points=MERGE_CELLS.  0 every attribute of a
    kept point carries its own row; a mask (bit a: attribute a of the stream -- 0 positions, then normals, texture coordinates, the
    generic attribute and the attribute list, those the cloud has), a list of such indices, or "all" (every attribute of the cloud
    but positions and normals; the clouds of a call must then have the same attributes): those attributes carry, per component,
    floor((2 S + cnt) / (2 cnt)) over the cnt input rows of the cell, S the sum of the integers the plain call codes for them -- the
    exact mean, ties upwards, whatever the order of the rows.  Positions and normals carry no mean.  part_cells and lod_base_bits
    compose with it; entry_rows, row_entries, part_info and lod_info are unchanged, cell_counts(i) counts the rows of every cell.

    vote_attributes (dsa_encode_vote_sequential_batch): the most frequent value of the cell WITH merge_points=MERGE_CELLS, for labels
    -- a classification, an instance id, a return number -- whose mean is a class nobody assigned.  A mask or a list of attribute
    indices of the stream, counted as for mean_attributes: those attributes (of 1 or 2 components) carry the tuple of coded integers
    that the most input rows of the cell have, among tuples of equally many rows the lexicographically smallest (signed components,
    component 0 first), whatever the order of the rows.  Positions and normals are not voted on, an attribute takes the vote or the
    mean, not both, and the clouds of a call must have the same attributes.  Everything else is as with mean_attributes.

    mean_normals (dsa_encode_normal_mean_sequential_batch): True: WITH merge_points=MERGE_CELLS the normals of every cloud that has
    them carry, per kept point, the code of the normalised sum of the unit normals of the cell's rows -- by a rule in 64-bit integers
    on the octahedral codes (include/draco_mi355x.h), whatever the order of the rows; a cell of one row keeps its code.  A cloud
    without normals is coded as before; a bit of mean_attributes or vote_attributes on the normals stays refused.  part_cells,
    lod_base_bits and the two masks compose with it; the handle is unchanged.

    voxel_bits, voxel_point (dsa_encode_voxel_sequential_batch): voxel_bits = C >= 1: WITH merge_points=MERGE_CELLS one point per
    occupied cell of the grid with C bits per axis is kept, whatever position_bits >= C the positions are stored at -- the voxel of a
    point is the top 3 C bits of its Morton key.  voxel_point says which: VOXEL_POINT_FIRST the voxel's first row in (key, row)
    order, VOXEL_POINT_CENTROID that row with its position coded as the exact integer mean of the voxel's quantised positions (ties
    upwards), VOXEL_POINT_NEAREST the input row nearest the voxel's centre (ties to the smaller row), as it is.  mean_attributes,
    vote_attributes and mean_normals reduce over the voxel; part_cells cuts the kept voxels; lod_base_bits = D needs D <= C and gives
    C - D + 1 levels.  voxel_bits=0 (default) is the request without it; voxel_bits=position_bits keeps what merge_points keeps."""

    EDGEBREAKER_METHODS = (0, 2, -1)
    POSITION_PREDICTIONS = (0, 1)
    TEXCOORD_PREDICTIONS = (0, 1, 5)
    NORMAL_PREDICTIONS = (0, 6)
    ENCODING_METHODS = (1, 0, -1)
    MULTI_PARALLELOGRAMS = (0, 2, 4, -1)
    TRAVERSAL_METHODS = (0, 1, 2)
    POINT_ORDERS = (native.POINT_ORDER_CALLER, native.POINT_ORDER_MORTON)
    MERGE_POINTS = (native.MERGE_NONE, native.MERGE_CELLS)
    VOXEL_POINTS = (native.VOXEL_POINT_FIRST, native.VOXEL_POINT_CENTROID, native.VOXEL_POINT_NEAREST)

    def __init__(self, position_bits=11, texcoord_bits=10, normal_bits=8, speed=5, single_connectivity=False,
                 symbol_scheme=-1, position_prediction=1, texcoord_prediction=1, edgebreaker_method=0, normal_prediction=0,
                 encoding_method=1, compress_connectivity=False, multi_parallelogram=0, traversal_method=0, repair_topology=False, weld_points=False,
                 repair_seams=False, weld_attributes=False, track_rows=False, point_order=0, merge_points=0, part_points=0, part_cells=0,
                 lod_base_bits=0, mean_attributes=0, vote_attributes=0, mean_normals=False, voxel_bits=0, voxel_point=0):
        for name, value, legal in (("encoding_method", encoding_method, self.ENCODING_METHODS),
                                   ("edgebreaker_method", edgebreaker_method, self.EDGEBREAKER_METHODS),
                                   ("position_prediction", position_prediction, self.POSITION_PREDICTIONS),
                                   ("texcoord_prediction", texcoord_prediction, self.TEXCOORD_PREDICTIONS),
                                   ("normal_prediction", normal_prediction, self.NORMAL_PREDICTIONS),
                                   ("multi_parallelogram", multi_parallelogram, self.MULTI_PARALLELOGRAMS),
                                   ("traversal_method", traversal_method, self.TRAVERSAL_METHODS),
                                   ("point_order", point_order, self.POINT_ORDERS),
                                   ("merge_points", merge_points, self.MERGE_POINTS)):
            if value not in legal:
                raise ValueError("%s %r: the encoder writes one of %s" % (name, value, legal))
        self.position_bits, self.texcoord_bits, self.normal_bits = position_bits, texcoord_bits, normal_bits
        self.speed = speed                      # compression level = 10 - speed (DracoEncoder.cs:50-56)
        self.single_connectivity = single_connectivity
        self.symbol_scheme = symbol_scheme
        self.position_prediction, self.texcoord_prediction = position_prediction, texcoord_prediction
        self.edgebreaker_method, self.normal_prediction = edgebreaker_method, normal_prediction
        self.encoding_method, self.compress_connectivity = encoding_method, bool(compress_connectivity)
        self.multi_parallelogram, self.traversal_method = multi_parallelogram, traversal_method
        self.repair_topology = bool(repair_topology)
        if self.repair_topology and self.sequential:
            raise ValueError("repair_topology shapes Edgebreaker streams: a sequential stream takes any list of triangles as it is")
        if self.leveled and self.sequential:
            raise ValueError("multi_parallelogram / traversal_method shape Edgebreaker streams: a sequential stream predicts by Difference in point order")
        self.repair_seams = bool(repair_seams)
        if self.repair_seams and not self.repair_topology:
            raise ValueError("repair_seams codes attributes given per corner over the repaired corner table: it needs repair_topology=True")
        self.weld_points = bool(weld_points)
        if self.weld_points and self.sequential:
            raise ValueError("weld_points shapes Edgebreaker streams: a sequential stream keeps the caller's points as they are")
        self.weld_attributes = bool(weld_attributes)
        if self.weld_attributes and not self.weld_points:
            raise ValueError("weld_attributes welds the listed attributes of per-point input each alone: it needs weld_points=True")
        self.track_rows = bool(track_rows)
        self.point_order = point_order
        self.merge_points = merge_points
        if self.merge_points != 0 and not (self.sequential and self.point_order == native.POINT_ORDER_MORTON):
            raise ValueError("merge_points keeps one point per cell of the position grid: it needs a sequential config (encoding_method 0) with point_order=POINT_ORDER_MORTON")
        self.part_points = int(part_points)
        if self.part_points < 0 or self.part_points > 2**31 - 1:
            raise ValueError("part_points %r: 0 (one stream per cloud) or the largest number of points of a part" % (part_points,))
        if self.part_points != 0 and (not (self.sequential and self.point_order == native.POINT_ORDER_MORTON) or self.merge_points != 0):
            raise ValueError("part_points cuts the Morton order of a point cloud into parts: it needs a sequential config (encoding_method 0) with point_order=POINT_ORDER_MORTON and no merge_points")

        self.part_cells = int(part_cells)
        if self.part_cells < 0 or self.part_cells > 2**31 - 1:
            raise ValueError("part_cells %r: 0 (no parts) or the largest number of kept points of a part" % (part_cells,))
        if self.part_cells != 0 and not (self.sequential and self.point_order == native.POINT_ORDER_MORTON and self.merge_points == native.MERGE_CELLS):
            raise ValueError("part_cells cuts the kept order of merge_points into parts: it needs a sequential config (encoding_method 0) with point_order=POINT_ORDER_MORTON and merge_points=MERGE_CELLS")
        # (part_cells together with part_points never gets here: part_points has refused the merge_points that part_cells needs)

        self.lod_base_bits = int(lod_base_bits)
        if self.lod_base_bits < 0:
            raise ValueError("lod_base_bits %r: 0 (no levels) or the bits per axis of the grid of level 0, 1 .. position_bits" % (lod_base_bits,))
        if self.lod_base_bits > self.position_bits:
            raise ValueError("lod_base_bits %r is above position_bits %r: level 0 cannot be finer than the quantisation grid" % (lod_base_bits, self.position_bits))
        if self.lod_base_bits != 0 and self.part_cells == 0:
            raise ValueError("lod_base_bits puts the kept points of merge_points into levels and cuts every level into parts: it needs part_cells >= 1 "
                             "(a sequential config with point_order=POINT_ORDER_MORTON and merge_points=MERGE_CELLS)")

        if isinstance(mean_attributes, str):
            if mean_attributes != "all":
                raise ValueError("mean_attributes %r: a mask, a list of attribute indices of the stream, or \"all\"" % (mean_attributes,))
            self.mean_attributes = "all"
        else:
            if isinstance(mean_attributes, (list, tuple, set, frozenset)):
                if any(int(a) != a or a < 0 for a in mean_attributes):
                    raise ValueError("mean_attributes %r: attribute indices of the stream, 0 and above" % (mean_attributes,))
                mask = 0
                for a in mean_attributes:
                    mask |= 1 << int(a)
            else:
                mask = int(mean_attributes)
            if mask < 0 or mask >> native.MAX_ATTRIBUTES:
                raise ValueError("mean_attributes %r: a bit at or above %d names no attribute of a stream" % (mean_attributes, native.MAX_ATTRIBUTES))
            if mask & 1:
                raise ValueError("mean_attributes %r: attribute 0 holds the positions, which are equal inside a cell and are never averaged" % (mean_attributes,))
            self.mean_attributes = mask
        if self.mean_attributes != 0 and self.merge_points != native.MERGE_CELLS:
            raise ValueError("mean_attributes takes the mean over the points of a cell: it needs merge_points=MERGE_CELLS "
                             "(a sequential config with point_order=POINT_ORDER_MORTON)")

        if isinstance(vote_attributes, (list, tuple, set, frozenset)):
            if any(int(a) != a or a < 0 for a in vote_attributes):
                raise ValueError("vote_attributes %r: attribute indices of the stream, 0 and above" % (vote_attributes,))
            mask = 0
            for a in vote_attributes:
                mask |= 1 << int(a)
        elif isinstance(vote_attributes, str):
            raise ValueError("vote_attributes %r: a mask or a list of attribute indices of the stream" % (vote_attributes,))
        else:
            mask = int(vote_attributes)
        if mask < 0 or mask >> native.MAX_ATTRIBUTES:
            raise ValueError("vote_attributes %r: a bit at or above %d names no attribute of a stream" % (vote_attributes, native.MAX_ATTRIBUTES))
        if mask & 1:
            raise ValueError("vote_attributes %r: attribute 0 holds the positions, which are equal inside a cell and are never voted on" % (vote_attributes,))
        self.vote_attributes = mask
        if self.vote_attributes != 0 and self.merge_points != native.MERGE_CELLS:
            raise ValueError("vote_attributes takes the most frequent value over the points of a cell: it needs merge_points=MERGE_CELLS "
                             "(a sequential config with point_order=POINT_ORDER_MORTON)")
        if self.vote_attributes != 0 and (self.mean_attributes == "all" or self.mean_attributes & self.vote_attributes):
            raise ValueError("vote_attributes %r and mean_attributes %r name the same attribute: it carries the most frequent value of its cell or the mean, not both"
                             % (vote_attributes, mean_attributes))

        if mean_normals not in (False, True, 0, 1):
            raise ValueError("mean_normals %r: False or True" % (mean_normals,))
        self.mean_normals = bool(mean_normals)
        if self.mean_normals and self.merge_points != native.MERGE_CELLS:
            raise ValueError("mean_normals takes the mean normal over the points of a cell: it needs merge_points=MERGE_CELLS "
                             "(a sequential config with point_order=POINT_ORDER_MORTON)")

        if isinstance(voxel_bits, bool) or not isinstance(voxel_bits, int) or not 0 <= voxel_bits <= self.position_bits:
            raise ValueError("voxel_bits %r: 0 (no voxels) or the bits per axis of the voxel grid, 1 .. position_bits (%d)" % (voxel_bits, self.position_bits))
        self.voxel_bits = voxel_bits
        if voxel_point not in self.VOXEL_POINTS:
            raise ValueError("voxel_point %r: one of VOXEL_POINT_FIRST, VOXEL_POINT_CENTROID, VOXEL_POINT_NEAREST %r" % (voxel_point, self.VOXEL_POINTS))
        self.voxel_point = int(voxel_point)
        if self.voxel_bits != 0 and self.merge_points != native.MERGE_CELLS:
            raise ValueError("voxel_bits keeps one of the points of a voxel: it needs merge_points=MERGE_CELLS "
                             "(a sequential config with point_order=POINT_ORDER_MORTON)")
        if self.voxel_point != 0 and self.voxel_bits == 0:
            raise ValueError("voxel_point %r needs voxel_bits >= 1: the centroid and the nearest point are those of a voxel" % (voxel_point,))
        if self.voxel_bits != 0 and self.lod_base_bits > self.voxel_bits:
            raise ValueError("lod_base_bits %d is above voxel_bits %d: level 0 cannot be finer than the voxel grid" % (self.lod_base_bits, self.voxel_bits))

    def _mean_mask(self, meshes):
        """mean_attributes as the mask of a call over `meshes`: "all" is every attribute but positions and normals, and needs clouds
        with the same attributes."""
        if self.mean_attributes != "all":
            return self.mean_attributes

        def every(m):
            count = 1 + (m.normals is not None) + (m.texcoords is not None) + (m.generic is not None) + len(m.attributes)
            return ((1 << count) - 1) & ~1 & ~(2 if m.normals is not None else 0)
        return _shared(meshes, every, "mean_attributes=\"all\"") or 0

    def _native_mean(self, geometry, meshes):
        o = native.EncodeMeanOptions()
        native.lib().dsa_encode_default_mean_options(C.byref(o))
        o.lod = self._native_lod(geometry)
        o.mean_attributes = self._mean_mask(meshes)
        return o

    def _native_vote(self, geometry, meshes):
        """the options of dsa_encode_vote_sequential_batch for a call over `meshes`, which must have the same attributes: the mask
        counts the attributes of the stream"""
        _shared(meshes, lambda m: (m.normals is not None, m.texcoords is not None, m.generic is not None, len(m.attributes)), "vote_attributes")
        o = native.EncodeVoteOptions()
        native.lib().dsa_encode_default_vote_options(C.byref(o))
        o.mean = self._native_mean(geometry, meshes)
        o.vote_attributes = self.vote_attributes
        return o

    def _native_normal_mean(self, geometry, meshes):
        """the options of dsa_encode_normal_mean_sequential_batch for a call over `meshes` (which must have the same attributes only
        where a mask says so)"""
        o = native.EncodeNormalMeanOptions()
        native.lib().dsa_encode_default_normal_mean_options(C.byref(o))
        if self.vote_attributes != 0:
            o.vote = self._native_vote(geometry, meshes)
        else:
            o.vote.mean = self._native_mean(geometry, meshes)
        o.mean_normals = 1 if self.mean_normals else 0
        return o

    def _native_voxel(self, geometry, meshes):
        """the options of dsa_encode_voxel_sequential_batch for a call over `meshes`"""
        o = native.EncodeVoxelOptions()
        native.lib().dsa_encode_default_voxel_options(C.byref(o))
        o.normal_mean = self._native_normal_mean(geometry, meshes)
        o.voxel_bits = self.voxel_bits
        o.voxel_point = self.voxel_point
        return o

    @property
    def sequential(self):
        """True when meshes are written as sequential streams: asked for, or by the reference's rule at speed 10."""
        return self.encoding_method == 0 or (self.encoding_method == -1 and self.speed == 10)

    def _native_sequential(self, geometry):
        o = native.EncodeSequentialOptions()
        native.lib().dsa_encode_sequential_default_options(C.byref(o))
        o.base = self._native()
        o.geometry = geometry
        o.compress_connectivity = 1 if (self.compress_connectivity and geometry == 1) else 0
        return o

    def _native_order(self, geometry):
        o = native.EncodeOrderOptions()
        native.lib().dsa_encode_default_order_options(C.byref(o))
        o.sequential = self._native_sequential(geometry)
        o.point_order = self.point_order
        return o

    def _native_merge(self, geometry):
        o = native.EncodeMergeOptions()
        native.lib().dsa_encode_default_merge_options(C.byref(o))
        o.order = self._native_order(geometry)
        o.merge_points = self.merge_points
        return o

    def _native_split(self, geometry):
        o = native.EncodeSplitOptions()
        native.lib().dsa_encode_default_split_options(C.byref(o))
        o.merge = self._native_merge(geometry)
        o.part_points = self.part_points
        return o

    def _native_cell_parts(self, geometry):
        o = native.EncodeCellPartsOptions()
        native.lib().dsa_encode_default_cell_parts_options(C.byref(o))
        o.split = self._native_split(geometry)
        o.part_cells = self.part_cells
        return o

    def _native_lod(self, geometry):
        o = native.EncodeLodOptions()
        native.lib().dsa_encode_default_lod_options(C.byref(o))
        o.cell_parts = self._native_cell_parts(geometry)
        o.lod_base_bits = self.lod_base_bits
        return o

    @property
    def extended(self):
        """True when an option only dsa_encode_batch_ex takes is set."""
        return self.edgebreaker_method != 0 or self.normal_prediction != 0

    @property
    def leveled(self):
        """True when an option only dsa_encode_level_batch takes is set."""
        return self.multi_parallelogram != 0 or self.traversal_method != 0

    def _native_repair(self):
        o = native.EncodeRepairOptions()
        native.lib().dsa_encode_default_repair_options(C.byref(o))
        o.level = self._native_level()
        o.topology = 1 if self.repair_topology else 0
        return o

    def _native_level(self):
        o = native.EncodeLevelOptions()
        native.lib().dsa_encode_default_level_options(C.byref(o))
        o.ex = self._native_ex()
        o.multi_parallelogram, o.traversal_method = self.multi_parallelogram, self.traversal_method
        return o

    def _native_ex(self):
        o = native.EncodeOptionsEx()
        native.lib().dsa_encode_default_options_ex(C.byref(o))
        o.base = self._native()
        o.edgebreaker_method, o.normal_prediction = self.edgebreaker_method, self.normal_prediction
        return o

    def _native(self):
        o = native.EncodeOptions()
        native.lib().dsa_encode_default_options(C.byref(o))
        o.position_bits, o.texcoord_bits, o.normal_bits = self.position_bits, self.texcoord_bits, self.normal_bits
        o.single_connectivity = 1 if self.single_connectivity else 0
        o.symbol_scheme = self.symbol_scheme
        o.compression_level = 10 - self.speed
        o.position_prediction, o.texcoord_prediction = self.position_prediction, self.texcoord_prediction
        return o


class Grid:
    """The quantisation grid of one float attribute (positions, the first UV set, a float32 Attribute) when it is not the
    attribute's own bounding box -- the reference's quantization_origin / quantization_range.  Grid(origin, range): origin per
    component and one range, written into the stream's header as they are; every value must be finite and quantise into
    0 .. 2^bits - 1, else its mesh is refused.  Grid.shared(): the grid is taken over every mesh of the batch with the same
    `group` that has the attribute, asks for a shared grid there and has the same component count (tiles of one surface, the
    primitives of one glTF mesh): border vertices then decode to the same floats on both sides."""

    def __init__(self, origin, range, mode=1):
        o = np.atleast_1d(np.asarray(origin, np.float32)).ravel()
        if not 1 <= len(o) <= 4:
            raise ValueError("Grid: 1 - 4 origin components")
        if mode == 1 and not (np.all(np.isfinite(o)) and np.isfinite(np.float32(range)) and np.float32(range) > 0):
            raise ValueError("Grid: a finite origin and a finite range above 0")
        self.origin, self.range, self.mode = o, np.float32(range), mode

    @classmethod
    def shared(cls):
        return cls([0.0], 1.0, mode=2)

    def _native(self, components):
        g = native.QuantizationGrid()
        if self.mode == 1 and len(self.origin) != components:
            raise ValueError("Grid: %d origin components for an attribute of %d" % (len(self.origin), components))
        for c, x in enumerate(self.origin):
            g.origin[c] = x
        g.range, g.mode = self.range, self.mode
        return g


def _check_grid(grid, name):
    if grid is not None and not isinstance(grid, Grid):
        raise ValueError("%s: a Grid or None" % name)
    return grid


ATTRIBUTE_DATA_TYPES = {np.dtype(np.int8): 1, np.dtype(np.uint8): 2, np.dtype(np.int16): 3, np.dtype(np.uint16): 4,
                        np.dtype(np.int32): 5, np.dtype(np.uint32): 6, np.dtype(np.float32): 9}      # Draco's DataType ids


class Attribute:
    """One more per-vertex (per-point) attribute behind positions / normals / the first UV set / `generic`: COLOR_0, JOINTS_0,
    WEIGHTS_0, a second UV set, feature ids.  values (V,) or (V, 1..4); the element type is the array's: int8, uint8, int16,
    uint16, int32, uint32 (coded as they are; 32-bit values within +-2^27 as int32) or float32 (quantised to quantization_bits,
    1..20; 0: the texture coordinates' bits for attribute_type 3, else 8).  attribute_type 2 colour, 3 texture coordinate,
    4 generic; normalized goes into the descriptor of an integer attribute; unique_id None: the attribute's index in the stream.
    corners (F, 3): the attribute given per corner -- row ids into `values`, which then hold as many rows as the ids need (a
    lightmap set with its own charts, a colour with a hard edge); edges across which the ids differ are seams of this attribute
    alone (dsa_encode_corner_attributes_batch).  The attribute's index in the stream must be at most 7."""

    def __init__(self, values, attribute_type=4, normalized=False, unique_id=None, quantization_bits=0, grid=None, corners=None):
        v = np.asarray(values)
        self.corners = corners                                    # (checked against the faces by MeshData)
        self.grid = _check_grid(grid, "Attribute grid")           # float32 only: a Grid in place of the values' own bounds
        if grid is not None and v.dtype != np.dtype(np.float32):
            raise ValueError("Attribute grid: only float32 values are quantised; integer attributes have no grid")
        if v.dtype not in ATTRIBUTE_DATA_TYPES:
            raise ValueError("attribute values of dtype %s: one of int8, uint8, int16, uint16, int32, uint32, float32" % v.dtype)
        if v.ndim not in (1, 2) or len(v) == 0:
            raise ValueError("attribute values: (V,) or (V, 1..4)")
        v = np.ascontiguousarray(v).reshape(len(v), -1)
        if not 1 <= v.shape[1] <= 4:
            raise ValueError("attribute values: 1 - 4 components per vertex")
        self.values = v
        self.attribute_type, self.normalized, self.unique_id, self.quantization_bits = attribute_type, bool(normalized), unique_id, quantization_bits

    @property
    def data_type(self):
        return ATTRIBUTE_DATA_TYPES[self.values.dtype]


def _attributes(attributes, rows):
    out = []
    for k, a in enumerate(attributes or []):
        if not isinstance(a, Attribute):
            a = Attribute(a)
        if getattr(a, "corners", None) is None and len(a.values) != rows:
            raise ValueError("attribute %d: one row per vertex (%d rows for %d vertices)" % (k, len(a.values), rows))
        out.append(a)
    return out


def _attribute_ids(attributes, faces):
    """Attribute.corners of a mesh's list checked like MeshData._ids and made (F, 3) uint32."""
    for k, a in enumerate(attributes):
        if getattr(a, "corners", None) is None:
            continue
        name = "attribute %d corners" % k
        ids = np.asarray(a.corners)
        if ids.shape != (len(faces), 3) and ids.size != 3 * len(faces):
            raise ValueError("%s: one id per face corner, shape (F, 3)" % name)
        if ids.size and (np.issubdtype(ids.dtype, np.signedinteger) and ids.min() < 0):
            raise ValueError("%s: ids are row numbers, not negative" % name)
        ids = np.ascontiguousarray(ids.reshape(len(faces), 3), np.uint32)
        if ids.size and int(ids.max()) >= len(a.values):
            raise ValueError("%s: id %d out of range (%d rows)" % (name, int(ids.max()), len(a.values)))
        a.corners = ids


def _has_attribute_ids(m):
    return any(getattr(a, "corners", None) is not None for a in (getattr(m, "attributes", None) or []))


def _fill_attribute_corners(dst, m, keep):
    """dsa_mesh_attribute_corners of mesh `m`; `keep` holds the ctypes array alive."""
    atts = getattr(m, "attributes", None) or []
    if not _has_attribute_ids(m):
        return
    arr = (native.AttributeCorners * len(atts))()
    for k, a in enumerate(atts):
        if getattr(a, "corners", None) is not None:
            arr[k].corners, arr[k].num_rows = a.corners.ctypes.data, len(a.values)
    keep.append(arr)
    dst.attributes = arr


def _fill_attr_input(dst, m, keep):
    """dsa_mesh_attr_input.attributes / num_attributes of mesh `m`; `keep` holds the ctypes array alive."""
    atts = getattr(m, "attributes", None) or []
    dst.num_attributes = len(atts)
    if not atts:
        return
    arr = (native.AttributeInput * len(atts))()
    for k, a in enumerate(atts):
        arr[k].attribute_type, arr[k].data_type, arr[k].num_components = a.attribute_type, a.data_type, a.values.shape[1]
        arr[k].normalized = 1 if a.normalized else 0
        arr[k].unique_id = native.UNIQUE_ID_DEFAULT if a.unique_id is None else a.unique_id
        arr[k].quantization_bits = a.quantization_bits
        arr[k].values = a.values.ctypes.data
    keep.append(arr)
    dst.attributes = arr


def _set_grids(m, position_grid, texcoord_grid, group, texcoords):
    """position_grid / texcoord_grid (a Grid or None: the attribute's own bounds) and the group number of shared grids."""
    m.position_grid = _check_grid(position_grid, "position_grid")
    m.texcoord_grid = _check_grid(texcoord_grid, "texcoord_grid")
    if texcoord_grid is not None and texcoords is None:
        raise ValueError("texcoord_grid without texcoords")
    if int(group) != group or not 0 <= group <= 0xFFFFFFFF:
        raise ValueError("group: a number 0 .. 2^32 - 1")
    m.group = int(group)


def _has_grid(m):
    return (getattr(m, "position_grid", None) is not None or getattr(m, "texcoord_grid", None) is not None
            or any(getattr(a, "grid", None) is not None for a in (getattr(m, "attributes", None) or [])))


def _fill_grids(dst, m, keep):
    """dsa_mesh_grids of mesh `m`; `keep` holds the ctypes array alive."""
    if getattr(m, "position_grid", None) is not None:
        dst.position = m.position_grid._native(3)
    if getattr(m, "texcoord_grid", None) is not None:
        dst.texcoord = m.texcoord_grid._native(2)
    dst.group = getattr(m, "group", 0)
    atts = getattr(m, "attributes", None) or []
    if any(getattr(a, "grid", None) is not None for a in atts):
        arr = (native.QuantizationGrid * len(atts))()
        for k, a in enumerate(atts):
            if getattr(a, "grid", None) is not None:
                arr[k] = a.grid._native(a.values.shape[1])
        keep.append(arr)
        dst.attributes = arr


def _native_meshes(meshes, form=None):
    """The native arrays of a list of MeshData / PointCloudData: (array of `form`, dsa_mesh_grids array or None, keep).  `form`
    is native.MeshAttrInput -- what every call of this module passes: corner ids and the attribute list where a mesh has them --
    or, for a caller of the narrower entry points, native.MeshCornerInput / native.MeshInput, which leave out what they cannot
    say.  The grids are there when some mesh sets one.  `keep` holds the ctypes arrays alive; the numpy arrays are the meshes'."""
    form = form or native.MeshAttrInput
    n = len(meshes)
    arr = (form * max(1, n))()
    keep = []
    for i, m in enumerate(meshes):
        ci = arr[i].mesh if form is native.MeshAttrInput else arr[i]
        mi = arr[i] if form is native.MeshInput else ci.mesh
        mi.num_vertices, mi.num_faces = len(m.positions), len(m.faces)
        mi.positions = m.positions.ctypes.data
        mi.faces = m.faces.ctypes.data if len(m.faces) else None
        mi.normals = m.normals.ctypes.data if m.normals is not None else None
        mi.texcoords = m.texcoords.ctypes.data if m.texcoords is not None else None
        g = getattr(m, "generic", None)
        mi.generic = g.ctypes.data if g is not None else None
        mi.generic_components = g.shape[1] if g is not None else 0
        if form is not native.MeshInput:
            nci, uci = getattr(m, "normal_corners", None), getattr(m, "texcoord_corners", None)
            ci.normal_corners = nci.ctypes.data if nci is not None else None
            ci.texcoord_corners = uci.ctypes.data if uci is not None else None
            ci.num_normals = len(m.normals) if m.normals is not None else 0
            ci.num_texcoords = len(m.texcoords) if m.texcoords is not None else 0
        if form is native.MeshAttrInput:
            _fill_attr_input(arr[i], m, keep)
    grids = None
    if any(_has_grid(m) for m in meshes):
        grids = (native.MeshGrids * max(1, n))()
        for i, m in enumerate(meshes):
            _fill_grids(grids[i], m, keep)
    return arr, grids, keep


class MeshData:
    """Triangle mesh with per-vertex attributes: positions (V,3) f32, faces (F,3) u32, optional normals (V,3), uvs (V,2) and one
    generic uint8 attribute of 1 - 4 components (V,) or (V,C): vertex colours, ids (ABI 4).  attributes: a list of Attribute
    (or arrays) written behind those, of any integer element type or float32 (dsa_encode_attributes_batch).

    normal_corners / texcoord_corners (F,3) u32: the normals / texture coordinates given per corner -- row ids into `normals` /
    `texcoords`, which then hold as many rows as the ids need (UV charts, hard edges).  Edges whose end points carry different ids
    on their two faces become attribute seams (dsa_encode_batch_corners).  Attribute(..., corners=) gives an attribute of the list
    per corner in the same way (dsa_encode_corner_attributes_batch).

    position_grid / texcoord_grid: a Grid in place of the attribute's own bounds (Attribute(..., grid=) for a float32 attribute
    of the list); group: the meshes of a batch whose Grid.shared() attributes share one grid (dsa_encode_grid_batch)."""

    def __init__(self, positions, faces, normals=None, texcoords=None, generic=None, normal_corners=None, texcoord_corners=None, attributes=None,
                 position_grid=None, texcoord_grid=None, group=0):
        _set_grids(self, position_grid, texcoord_grid, group, texcoords)
        self.positions = np.ascontiguousarray(positions, np.float32)
        self.attributes = _attributes(attributes, len(self.positions))
        self.faces = np.ascontiguousarray(faces, np.uint32)
        _attribute_ids(self.attributes, self.faces)
        self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32)
        self.texcoords = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32)
        self.normal_corners = self._ids(normal_corners, self.normals, 3, "normal")
        self.texcoord_corners = self._ids(texcoord_corners, self.texcoords, 2, "texcoord")
        self.generic = None
        if generic is not None:
            g = np.ascontiguousarray(generic, np.uint8)
            g = g.reshape(len(g), -1)
            if len(g) != len(self.positions) or not 1 <= g.shape[1] <= 4:
                raise ValueError("generic attribute: one row of 1 - 4 uint8 components per vertex")
            self.generic = g

    def _ids(self, ids, rows, nc, name):
        if ids is None:
            return None
        if rows is None:
            raise ValueError("%s_corners needs %ss" % (name, name))
        if rows.ndim != 2 or rows.shape[1] != nc:
            raise ValueError("%ss given per corner: one row of %d components per value" % (name, nc))
        a = np.asarray(ids)
        if a.shape != (len(self.faces), 3) and a.size != 3 * len(self.faces):
            raise ValueError("%s_corners: one id per face corner, shape (F, 3)" % name)
        if a.size and (np.issubdtype(a.dtype, np.signedinteger) and a.min() < 0):
            raise ValueError("%s_corners: ids are row numbers, not negative" % name)
        a = np.ascontiguousarray(a.reshape(len(self.faces), 3), np.uint32)
        if a.size and int(a.max()) >= len(rows):
            raise ValueError("%s_corners: id %d out of range (%d rows)" % (name, int(a.max()), len(rows)))
        return a

    @property
    def per_corner(self):
        return getattr(self, "normal_corners", None) is not None or getattr(self, "texcoord_corners", None) is not None or _has_attribute_ids(self)


class PointCloudData:
    """Point cloud with per-point attributes: positions (N,3) f32, optional normals (N,3), texcoords (N,2) and one generic uint8
    attribute of 1 - 4 components (N,) or (N,C).  Written as a sequential point-cloud stream (dsa_encode_sequential_batch,
    geometry 0): point i of the stream is row i.  attributes: as for MeshData, one row per point."""

    def __init__(self, positions, normals=None, texcoords=None, generic=None, attributes=None, position_grid=None, texcoord_grid=None, group=0):
        _set_grids(self, position_grid, texcoord_grid, group, texcoords)
        self.positions = np.ascontiguousarray(positions, np.float32)
        self.attributes = _attributes(attributes, len(self.positions))
        if _has_attribute_ids(self):
            raise ValueError("attribute corners need the faces of a mesh: a point cloud has one value per point")
        self.faces = np.zeros((0, 3), np.uint32)
        self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32)
        self.texcoords = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32)
        for a, nc, name in ((self.positions, 3, "positions"), (self.normals, 3, "normals"), (self.texcoords, 2, "texcoords")):
            if a is not None and (a.ndim != 2 or a.shape[1] != nc or len(a) != len(self.positions)):
                raise ValueError("%s: one row of %d components per point" % (name, nc))
        self.generic = None
        if generic is not None:
            g = np.ascontiguousarray(generic, np.uint8)
            g = g.reshape(len(g), -1)
            if len(g) != len(self.positions) or not 1 <= g.shape[1] <= 4:
                raise ValueError("generic attribute: one row of 1 - 4 uint8 components per point")
            self.generic = g


class EncodedStreams:
    """The .drc streams of a batch, a sequence of `bytes`.  The bytes stay in the library's buffers until a stream is asked
    for (indexing, iteration), so that a caller who hands the batch on -- to a file, a socket, dsa.Batch -- pays for one copy of
    what it touches instead of for 4096 fresh allocations up front; `sizes` needs none.  A mesh that could not be encoded raises
    when the batch is made, like the reference's encoder does for its one mesh."""

    def __init__(self, ctx, handle, n):
        L = native.lib()
        self._ctx = ctx
        self._h, self._free = handle, L.dsa_encoded_free
        self._ptr, self._len, self._cache = [0] * n, [0] * n, [None] * n
        p, ln = C.c_void_p(), C.c_size_t()
        try:
            for i in range(n):
                st = L.dsa_encoded_stream(handle, i, C.byref(p), C.byref(ln))
                if st != 0:
                    _raise(st, ctx.error())
                self._ptr[i], self._len[i] = p.value, ln.value
        except Exception:
            self.close()
            raise

    @property
    def sizes(self):
        return list(self._len)

    def __len__(self):
        return len(self._len)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        b = self._cache[i]
        if b is None:
            if self._h is None:
                raise ValueError("the encoded batch was closed")
            b = self._cache[i] = C.string_at(self._ptr[i], self._len[i])
        return b

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return len(self) == len(other) and all(a == b for a, b in zip(self, other))

    def entry_rows(self, i):
        """Of stream i a list with one uint32 array per attribute of the stream (positions, then normals, texture coordinates,
        generic where present, then the attribute list): element e is the row of the array passed for that attribute whose bytes
        entry e of the stream carries -- with weld_points a point of the per-point arrays.  Needs Config(track_rows=True), or a
        sequential stream (the identity; with Config(point_order=1) the permutation, for every attribute); dsa_encoded_entry_rows."""
        if self._h is None:
            raise ValueError("the encoded batch was closed")
        return _entry_rows(self._ctx, self._h, i + len(self) if i < 0 else i)

    def row_entries(self, i):
        """Of stream i of an encode with Config(merge_points=MERGE_CELLS) a uint32 array with one element per input row: the entry
        of the stream whose cell the row lies in (entry_rows(i)[a][row_entries(i)[r]] is the kept row of r's cell);
        dsa_encoded_row_entries."""
        if self._h is None:
            raise ValueError("the encoded batch was closed")
        return _row_entries(self._ctx, self._h, i + len(self) if i < 0 else i)

    def cell_counts(self, i):
        """Of stream i of an encode with Config(merge_points=MERGE_CELLS) (with parts: of an input's first stream) a uint32 array with
        one element per kept point of the cloud: the input rows of its cell, np.bincount of row_entries(i) -- what a mean of
        Config(mean_attributes=...) was taken over."""
        cells = self.row_entries(i)
        m = int(cells.max()) + 1 if len(cells) else 0       # (every kept point has a row: its own)
        return np.bincount(cells, minlength=m).astype(np.uint32)

    def row_parts(self, i):
        """Of input i of an encode with Config(merge_points=MERGE_CELLS, part_cells=N): (part, entry), two uint32 arrays with one
        element per input row -- the part of the input whose stream codes the row's cell (stream parts(i)[part]) and the entry of
        that stream; searchsorted of the parts' first_entry in the cloud's row_entries, and the difference."""
        r = self.parts(i)
        cells = self.row_entries(r[0])
        first = np.array([self.part_info(s).first_entry for s in r], np.uint32)
        part = (np.searchsorted(first, cells, side="right") - 1).astype(np.uint32)
        return part, (cells - first[part]).astype(np.uint32)

    def parts(self, i):
        """The streams of input i of the encode as a range: with Config(part_points=N) or Config(part_cells=N) its parts in order,
        else range(i, i + 1); dsa_encoded_parts."""
        if self._h is None:
            raise ValueError("the encoded batch was closed")
        first, count = C.c_uint32(), C.c_uint32()
        st = native.lib().dsa_encoded_parts(self._h, i, C.byref(first), C.byref(count))
        if st != 0:
            _raise(st, "no input %r" % (i,))
        return range(first.value, first.value + count.value)

    def part_info(self, s):
        """Of stream s of an encode with Config(part_points=N) a native.PartInfo: input, part, parts, first_entry, num_points,
        position_bits, qmin / qmax (the position integers the stream codes, per component) and box_min / box_max (the floats the
        decoder returns for them: bit for bit the box of the part's decoded positions); dsa_encoded_part_info."""
        if self._h is None:
            raise ValueError("the encoded batch was closed")
        return _part_info(self._ctx, self._h, s + len(self) if s < 0 else s)

    def lod_info(self, s):
        """Of stream s of an encode with Config(lod_base_bits=D) a native.LodInfo: input, level, levels (L), cell_bits (D + level),
        level_first_stream / level_streams (the streams of its level), level_points and part_in_level; dsa_encoded_lod_info."""
        if self._h is None:
            raise ValueError("the encoded batch was closed")
        return _lod_info(self._ctx, self._h, s + len(self) if s < 0 else s)

    def levels(self, i):
        """The streams of input i of an encode with Config(lod_base_bits=D) per level: a list of L ranges of streams, level 0 first,
        an empty range for a level without points."""
        r = self.parts(i)
        out, s = [], r.start
        for level in range(self.lod_info(s).levels):
            info = self.lod_info(s) if s < r.stop else None
            count = info.level_streams if info is not None and info.level == level else 0
            out.append(range(s, s + count))
            s += count
        return out

    def close(self):
        """Releases the library's buffers (streams already taken stay valid)."""
        if self._h is not None:
            self._free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class TriedStreams(list):
    """What TryEncodeBatch returns: per mesh the stream or the exception; `encoded`: with keep=True the open handle, else None."""
    encoded = None


class _EncodedHandle:
    """An encoded batch some of whose meshes may have failed (TryEncodeBatch(keep=True)): what Batch.source_rows and entry_rows need."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle

    def entry_rows(self, i):
        return _entry_rows(self._ctx, self._h, i)

    def row_entries(self, i):
        return _row_entries(self._ctx, self._h, i)

    def part_info(self, s):
        return _part_info(self._ctx, self._h, s)

    def close(self):
        if self._h is not None:
            native.lib().dsa_encoded_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def join_plan(encoded, inputs=None):
    """What dsa.Batch and Batch.joined_arrays take to put the parts of the inputs of an encode back together: (streams, groups,
    encoded_mesh) -- the streams of the inputs (None: all of the call) one after the other, per input a group (first_mesh,
    num_meshes) of the batch made from `streams`, and per mesh of that batch the stream of `encoded` it came from.  `encoded`: an
    open EncodedStreams, or the handle of TryEncodeBatch(keep=True); an input that was refused is left out."""
    h = getattr(encoded, "_h", None)
    if h is None:
        raise ValueError("join_plan takes an open encoded batch")
    L = native.lib()
    first, count = C.c_uint32(), C.c_uint32()
    if inputs is None:
        inputs = []
        while L.dsa_encoded_parts(h, len(inputs), C.byref(first), C.byref(count)) == 0:
            inputs.append(len(inputs))
    streams, groups, encoded_mesh = [], [], []
    p, ln = C.c_void_p(), C.c_size_t()
    for i in inputs:
        if L.dsa_encoded_parts(h, int(i), C.byref(first), C.byref(count)) != 0:
            raise ValueError("no input %r" % (i,))
        taken = []
        for s in range(first.value, first.value + count.value):
            if L.dsa_encoded_stream(h, s, C.byref(p), C.byref(ln)) != 0:
                taken = None                     # a refused input keeps one slot, which returns its status
                break
            taken.append(C.string_at(p, ln.value))
        if not taken:
            continue
        groups.append((len(streams), len(taken)))
        encoded_mesh += range(first.value, first.value + count.value)
        streams += taken
    return streams, groups, np.asarray(encoded_mesh, np.uint32)


def _entry_rows(ctx, handle, i):
    """dsa_encoded_entry_rows of mesh i for every attribute dsa_encoded_attributes counts."""
    L = native.lib()
    count = C.c_uint32()
    st = L.dsa_encoded_attributes(handle, i, C.byref(count))
    if st != 0:
        _raise(st, ctx.error())
    out = []
    for a in range(count.value):
        st = L.dsa_encoded_entry_rows(handle, i, a, None, 0, C.byref(count))
        if st != 0:
            _raise(st, ctx.error())
        rows = np.empty(count.value, np.uint32)
        st = L.dsa_encoded_entry_rows(handle, i, a, rows.ctypes.data, len(rows), C.byref(count))
        if st != 0:
            _raise(st, ctx.error())
        out.append(rows)
    return out


def _row_entries(ctx, handle, i):
    """dsa_encoded_row_entries of mesh i."""
    L = native.lib()
    count = C.c_uint32()
    st = L.dsa_encoded_row_entries(handle, i, None, 0, C.byref(count))
    if st != 0:
        _raise(st, ctx.error())
    cells = np.empty(count.value, np.uint32)
    st = L.dsa_encoded_row_entries(handle, i, cells.ctypes.data, len(cells), C.byref(count))
    if st != 0:
        _raise(st, ctx.error())
    return cells


def _part_info(ctx, handle, s):
    """dsa_encoded_part_info of stream s."""
    info = native.PartInfo()
    st = native.lib().dsa_encoded_part_info(handle, s, C.byref(info))
    if st != 0:
        _raise(st, ctx.error())
    return info


def _lod_info(ctx, handle, s):
    """dsa_encoded_lod_info of stream s."""
    info = native.LodInfo()
    st = native.lib().dsa_encoded_lod_info(handle, s, C.byref(info))
    if st != 0:
        _raise(st, ctx.error())
    return info


class WeldedMaps:
    """dsa_welded_info of one mesh as numpy arrays (copies): num_points / num_vertices / num_normals / num_texcoords,
    normals_per_vertex / texcoords_per_vertex, and vertex_of_point [P] (0xFFFFFFFF: a point no face names), vertex_point [V],
    normal_of_point / normal_point, texcoord_of_point / texcoord_point (None when the mesh has no such attribute)."""

    def __init__(self, info):
        self.num_points, self.num_vertices = info.num_points, info.num_vertices
        self.num_normals, self.num_texcoords = info.num_normals, info.num_texcoords
        self.normals_per_vertex, self.texcoords_per_vertex = bool(info.normals_per_vertex), bool(info.texcoords_per_vertex)

        def array(ptr, count):
            return np.frombuffer(C.string_at(ptr, 4 * count), np.uint32).copy() if ptr and count else np.zeros(0, np.uint32)
        self.vertex_of_point, self.vertex_point = array(info.vertex_of_point, info.num_points), array(info.vertex_point, info.num_vertices)
        has_n, has_t = bool(info.normal_of_point) or info.num_normals > 0, bool(info.texcoord_of_point) or info.num_texcoords > 0
        self.normal_of_point = array(info.normal_of_point, info.num_points) if has_n else None
        self.normal_point = array(info.normal_point, info.num_normals) if has_n else None
        self.texcoord_of_point = array(info.texcoord_of_point, info.num_points) if has_t else None
        self.texcoord_point = array(info.texcoord_point, info.num_texcoords) if has_t else None


class DracoEncoder:
    def __init__(self, context=None):
        self._ctx = context

    def EncodeBatch(self, meshes, config=None, handle=False):
        """meshes: list of MeshData (or of PointCloudData) -> sequence of bytes (.drc streams, EncodedStreams).  A sequential
        config (Config.sequential) and point clouds go through dsa_encode_grid_sequential_batch, every other batch through
        dsa_encode_seam_repair_batch -- or, when an Attribute carries corners or config.weld_attributes is set, through
        dsa_encode_corner_attributes_batch, which takes both.  A mesh that cannot be encoded raises
        (TryEncodeBatch: the batch with its failures, mesh by mesh)."""
        n = len(meshes)
        config = config or Config()
        # what the batch is, before anything touches the device: meshes or point clouds, not both; a sequential stream has one
        # value per point
        clouds = sum(1 for m in meshes if isinstance(m, PointCloudData))
        if clouds and clouds != n:
            raise ValueError("a batch holds meshes or point clouds, not both")
        if config.leveled and (clouds or config.sequential):
            raise ValueError("multi_parallelogram / traversal_method shape Edgebreaker streams: point clouds and sequential streams predict by Difference in point order")
        if (clouds or config.sequential) and any(getattr(m, "per_corner", False) for m in meshes):
            raise ValueError("attributes given per corner need Edgebreaker connectivity (encoding_method 1): a sequential stream has one value per point")
        if getattr(config, "point_order", 0) != 0 and not (clouds or config.sequential):
            raise ValueError("point_order needs a sequential stream (encoding_method 0, or point clouds): Edgebreaker orders its own entries")
        if getattr(config, "part_cells", 0) != 0 and not clouds:
            raise ValueError("part_cells takes point clouds (PointCloudData): a part of a mesh would need its faces cut")
        if getattr(config, "part_points", 0) != 0 and not clouds:
            raise ValueError("part_points takes point clouds (PointCloudData): a part of a mesh would need its faces cut")
        if getattr(config, "merge_points", 0) != 0 and not clouds:
            raise ValueError("merge_points takes point clouds (PointCloudData): merging the points of a mesh would collapse its faces and lose its seams")
        weld = getattr(config, "weld_points", False)
        if weld and (clouds or config.sequential):
            raise ValueError("weld_points shapes Edgebreaker streams of meshes: point clouds and sequential streams keep the caller's points")
        if weld and any(getattr(m, "per_corner", False) for m in meshes):
            raise ValueError("weld_points takes one row per point: normal_corners / texcoord_corners describe a mesh that is welded already")
        if getattr(config, "weld_attributes", False) and not weld:
            raise ValueError("weld_attributes welds the listed attributes of per-point input each alone: it needs weld_points=True")
        ctx = self._ctx or default_context()
        L = native.lib()
        if clouds or config.sequential:
            return self._encode_sequential(ctx, meshes, config, 0 if clouds else 1, handle=handle)
        # every Edgebreaker batch through the widest entry point: with the fields a Config leaves alone at their defaults, empty
        # attribute lists and no grids it is the very request of the narrower calls (include/draco_mi355x.h)
        arr, grids, keep = _native_meshes(meshes)
        opt = native.EncodeSeamRepairOptions()
        L.dsa_encode_default_seam_repair_options(C.byref(opt))
        opt.grid.repair = config._native_repair()
        opt.grid.weld_points = 1 if weld else 0
        opt.corner_repair = 1 if getattr(config, "repair_seams", False) else 0
        h = C.c_void_p()
        weld_attributes = getattr(config, "weld_attributes", False)
        t0 = time.perf_counter()
        track_rows = getattr(config, "track_rows", False)
        if track_rows or weld_attributes or any(_has_attribute_ids(m) for m in meshes):
            # ids on attributes of the list, or the list welded attribute by attribute: the one call that takes them -- and, with
            # track_rows, the one beyond it whose handle keeps the entry rows
            wide = native.EncodeCornerAttributesOptions()
            L.dsa_encode_default_corner_attributes_options(C.byref(wide))
            wide.seam_repair = opt
            wide.weld_attributes = 1 if weld_attributes else 0
            corners = (native.MeshAttributeCorners * max(1, n))()
            for i, m in enumerate(meshes):
                _fill_attribute_corners(corners[i], m, keep)
            if track_rows:
                widest = native.EncodeRowsOptions()
                L.dsa_encode_default_rows_options(C.byref(widest))
                widest.corner_attributes = wide
                widest.track_rows = 1
                st = L.dsa_encode_rows_batch(ctx._h, n, arr, grids, corners, C.byref(widest), C.byref(h))
            else:
                st = L.dsa_encode_corner_attributes_batch(ctx._h, n, arr, grids, corners, C.byref(wide), C.byref(h))
        else:
            st = L.dsa_encode_seam_repair_batch(ctx._h, n, arr, grids, C.byref(opt), C.byref(h))
        t1 = time.perf_counter()
        if st != 0:
            _raise(st, ctx.error())
        if handle:
            return ctx, h, n
        r = EncodedStreams(ctx, h, n)
        if os.environ.get("DSA_ENC_TIMING"):            # diagnostics, like the library's own phase clocks
            print("[EncodeBatch] native call %.1f ms, result handles %.1f ms" % ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3), flush=True)
        return r

    # The sequential entry points from the widest to the narrowest: (the option that asks for it, the builder of its options, the entry
    # point, whether its handle has a slot per stream, so that n is read back from it).  A Config reaches the first whose option it
    # sets -- the widest call only when its option is set, and the plain case keeps arriving through the call it always took.
    _SEQUENTIAL_CALLS = (
        ("voxel_bits", "_native_voxel", "dsa_encode_voxel_sequential_batch", True),
        ("mean_normals", "_native_normal_mean", "dsa_encode_normal_mean_sequential_batch", True),
        ("vote_attributes", "_native_vote", "dsa_encode_vote_sequential_batch", True),
        ("mean_attributes", "_native_mean", "dsa_encode_mean_sequential_batch", True),
        ("lod_base_bits", "_native_lod", "dsa_encode_lod_sequential_batch", True),
        ("part_cells", "_native_cell_parts", "dsa_encode_cell_parts_sequential_batch", True),
        ("part_points", "_native_split", "dsa_encode_split_sequential_batch", True),
        ("merge_points", "_native_merge", "dsa_encode_merged_sequential_batch", False),
        ("point_order", "_native_order", "dsa_encode_ordered_sequential_batch", False),
        (None, "_native_sequential", "dsa_encode_grid_sequential_batch", False),
    )

    def _encode_sequential(self, ctx, meshes, config, geometry, handle=False):
        n = len(meshes)
        arr, grids, keep = _native_meshes(meshes)
        h = C.c_void_p()
        for option, build, entry, slots in self._SEQUENTIAL_CALLS:
            if option is not None and getattr(config, option, 0) == 0:
                continue
            if option == "mean_attributes":             # (a mask that names no attribute the meshes have asks for nothing)
                if config._mean_mask(meshes) == 0:
                    continue
                opt = config._native_mean(geometry, meshes)
            elif option in ("vote_attributes", "mean_normals", "voxel_bits"):
                opt = getattr(config, build)(geometry, meshes)
            else:
                opt = getattr(config, build)(geometry)
            break
        st = getattr(native.lib(), entry)(ctx._h, n, arr, grids, C.byref(opt), C.byref(h))
        if st != 0:
            _raise(st, ctx.error())
        if slots:
            n = native.lib().dsa_encoded_size(h)
        return (ctx, h, n) if handle else EncodedStreams(ctx, h, n)

    def TryEncodeBatch(self, meshes, config=None, keep=False):
        """EncodeBatch that keeps the meshes the encoder refuses: a list with, per mesh, the stream as bytes or the exception (its text says why)
        that EncodeBatch would have raised for it.  A failure of the call itself still raises.  keep=True: the list is a TriedStreams
        whose `encoded` is the open handle (entry_rows(i), close(); what Batch.source_rows takes), which the caller closes."""
        ctx, h, n = self.EncodeBatch(meshes, config, handle=True)
        L = native.lib()
        out = TriedStreams()
        p, ln = C.c_void_p(), C.c_size_t()
        try:
            for i in range(n):
                st = L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln))
                if st == 0:
                    out.append(C.string_at(p, ln.value))
                    continue
                try:
                    _raise(st, ctx.error())
                except Exception as e:          # noqa: BLE001  (the exception is the result)
                    out.append(e)
            if keep:
                out.encoded, h = _EncodedHandle(ctx, h), None
        finally:
            if h is not None:
                L.dsa_encoded_free(h)
        return out

    def WeldBatch(self, meshes):
        """The weld of dsa_encode_points_batch alone (dsa_weld_batch): per MeshData given as one row per point a WeldedMaps with
        the maps between points and vertices / normal rows / texture coordinate rows as numpy arrays -- what carries further
        per-point data (morph targets) across the weld: row v of a welded array is row vertex_point[v] of the per-point one.  A
        mesh that cannot be welded (a face index out of range) raises."""
        if any(isinstance(m, PointCloudData) for m in meshes):
            raise ValueError("the weld takes meshes: a point cloud has no faces that name its points")
        if any(getattr(m, "per_corner", False) for m in meshes):
            raise ValueError("the weld takes one row per point: normal_corners / texcoord_corners describe a mesh that is welded already")
        ctx = self._ctx or default_context()
        L = native.lib()
        n = len(meshes)
        arr, _, keep = _native_meshes(meshes)
        h = C.c_void_p()
        st = L.dsa_weld_batch(ctx._h, n, arr, C.byref(h))
        if st != 0:
            _raise(st, ctx.error())
        try:
            out = []
            info = native.WeldedInfo()
            for i in range(n):
                st = L.dsa_welded_mesh(h, i, C.byref(info))
                if st != 0:
                    _raise(st, ctx.error())
                out.append(WeldedMaps(info))
            return out
        finally:
            L.dsa_welded_free(h)

    def Encode(self, mesh, config=None):
        return self.EncodeBatch([mesh], config)[0]
