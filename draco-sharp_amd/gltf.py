"""glTF 2.0 containers in front of the batch decode path: every primitive that carries KHR_draco_mesh_compression in
any number of .gltf / .glb assets becomes one stream of one `Batch` (the caller on the input
side of the path).  Only the container is handled here -- JSON, GLB chunks, buffers and buffer views; what is inside
the buffer view goes to the GPU untouched.  GltfDracoWriter is the counterpart on the encode side: it compresses the TRIANGLES
primitives of any number of assets in one EncodeBatch (Config(weld_points=True): a primitive is one row per point) and rewrites
the documents with the extension.

The extension object is `{"bufferView": i, "attributes": {"POSITION": id, ...}}`: the ids are Draco unique ids
(PointCloud.GetAttributeByUniqueId), decoded values are per *point* and the faces are point indices, which is exactly
glTF's vertex / index model.
"""
import base64
import json
import os
import struct

import numpy as np

from .decoder import Batch, Draco, DracoHeader, InvalidDataException, Mesh, PointAttribute, default_context

EXTENSION = "KHR_draco_mesh_compression"
_GLB_MAGIC, _CHUNK_JSON, _CHUNK_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_TYPE_COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT2": 4, "MAT3": 9, "MAT4": 16}


class GltfAsset:
    """Parsed container: the JSON document and the bytes of every buffer."""

    def __init__(self, doc, buffers, name=""):
        self.doc = doc
        self.buffers = buffers
        self.name = name

    def buffer_view(self, index):
        views = self.doc.get("bufferViews", [])
        if not 0 <= index < len(views):
            raise InvalidDataException("%s: bufferView %d does not exist" % (self.name, index))
        v = views[index]
        b = v.get("buffer", -1)
        if not 0 <= b < len(self.buffers):
            raise InvalidDataException("%s: bufferView %d names buffer %d" % (self.name, index, b))
        off, length = int(v.get("byteOffset", 0)), int(v["byteLength"])
        data = self.buffers[b]
        if off < 0 or length < 0 or off + length > len(data):
            raise InvalidDataException("%s: bufferView %d leaves its buffer" % (self.name, index))
        return bytes(data[off:off + length])


def read_asset(source, base_dir=None, name=None):
    """source: path of a .gltf / .glb file, or the bytes of either.  base_dir resolves relative buffer URIs."""
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        with open(path, "rb") as f:
            data = f.read()
        return read_asset(data, base_dir=os.path.dirname(os.path.abspath(path)), name=name or os.path.basename(path))
    data = bytes(source)
    name = name or "<bytes>"
    glb_bin = None
    if len(data) >= 12 and struct.unpack_from("<I", data, 0)[0] == _GLB_MAGIC:
        _, version, total = struct.unpack_from("<III", data, 0)
        if version != 2 or total > len(data) or total < 20:
            raise InvalidDataException("%s: not a GLB 2 container" % name)
        pos, doc = 12, None
        while pos + 8 <= total:
            clen, ctype = struct.unpack_from("<II", data, pos)
            pos += 8
            if clen > total - pos:
                raise InvalidDataException("%s: GLB chunk leaves the file" % name)
            if ctype == _CHUNK_JSON and doc is None:
                doc = json.loads(data[pos:pos + clen].decode("utf-8"))
            elif ctype == _CHUNK_BIN and glb_bin is None:
                glb_bin = data[pos:pos + clen]
            pos += (clen + 3) & ~3
        if doc is None:
            raise InvalidDataException("%s: GLB without a JSON chunk" % name)
    else:
        try:
            doc = json.loads(data.decode("utf-8"))
        except (UnicodeDecodeError, ValueError) as e:
            raise InvalidDataException("%s: neither GLB nor glTF JSON (%s)" % (name, e))
    buffers = []
    for i, b in enumerate(doc.get("buffers", [])):
        uri = b.get("uri")
        if uri is None:
            if i != 0 or glb_bin is None:
                raise InvalidDataException("%s: buffer %d has no uri and there is no GLB binary chunk" % (name, i))
            raw = glb_bin
        elif uri.startswith("data:"):
            head, _, payload = uri.partition(",")
            if not head.endswith(";base64"):
                raise InvalidDataException("%s: buffer %d: only base64 data URIs are supported" % (name, i))
            raw = base64.b64decode(payload)
        else:
            if base_dir is None:
                raise InvalidDataException("%s: buffer %d is external (%s) and no base directory was given" % (name, i, uri))
            raw = _read_external_buffer(name, i, base_dir, uri)
        if len(raw) < int(b.get("byteLength", 0)):
            raise InvalidDataException("%s: buffer %d is shorter than its byteLength" % (name, i))
        buffers.append(raw)
    return GltfAsset(doc, buffers, name)


def _read_external_buffer(name, i, base_dir, uri):
    """An external buffer is a file below the asset's own directory, nothing else: an asset is untrusted input, so
    URIs with a scheme (file:, http:, ...), absolute paths and paths that climb out of base_dir (also percent-encoded
    or through symbolic links) are rejected instead of opened."""
    import re
    from urllib.parse import unquote
    if re.match(r"^[A-Za-z][A-Za-z0-9+.-]*:", uri):
        raise InvalidDataException("%s: buffer %d: URI scheme not supported (%s)" % (name, i, uri.split(":", 1)[0]))
    rel = unquote(uri)
    if os.path.isabs(rel) or rel.startswith(("/", "\\")) or "\x00" in rel:
        raise InvalidDataException("%s: buffer %d: absolute buffer path" % (name, i))
    root = os.path.realpath(base_dir)
    path = os.path.realpath(os.path.join(root, rel))
    if os.path.commonpath([root, path]) != root or path == root:
        raise InvalidDataException("%s: buffer %d: buffer path leaves the asset directory" % (name, i))
    try:
        with open(path, "rb") as f:
            return f.read()
    except OSError as e:
        raise InvalidDataException("%s: buffer %d: cannot read external buffer (%s)" % (name, i, e.strerror))


class DracoPrimitive:
    """One compressed primitive: where it sits in the asset, its stream and the extension's attribute ids."""

    def __init__(self, asset, mesh, primitive, stream, attribute_ids, accessors, indices_accessor, mode):
        self.asset, self.mesh, self.primitive = asset, mesh, primitive
        self.stream = stream
        self.attribute_ids = attribute_ids          # semantic -> Draco unique id
        self.accessors = accessors                  # semantic -> accessor index of the primitive
        self.indices_accessor = indices_accessor
        self.mode = mode


def draco_primitives(asset):
    """Every primitive of the asset that carries the extension, in document order."""
    out = []
    for mi, mesh in enumerate(asset.doc.get("meshes", [])):
        for pi, prim in enumerate(mesh.get("primitives", [])):
            ext = prim.get("extensions", {}).get(EXTENSION)
            if ext is None:
                continue
            mode = prim.get("mode", 4)
            if mode not in (4, 5):                  # the extension allows TRIANGLES and TRIANGLE_STRIP only
                raise InvalidDataException("%s: mesh %d primitive %d: Draco compression with mode %d" % (asset.name, mi, pi, mode))
            stream = asset.buffer_view(int(ext["bufferView"]))
            ids = {k: int(v) for k, v in ext.get("attributes", {}).items()}
            out.append(DracoPrimitive(asset, mi, pi, stream, ids, dict(prim.get("attributes", {})), prim.get("indices"), mode))
    return out


class DecodedPrimitive:
    """indices: uint32[3 * faces] (point ids); attributes: semantic -> array[points, components]; quantization: semantic ->
    (min, range, bits) for the attributes load(quantized=True) returned as integers (dsa_batch_vertex_arrays in
    include/draco_mi355x.h states the dequantisation).  draco: the stream as a Draco object whose attributes carry one value per
    point (identity point maps)."""

    def __init__(self, source, draco, indices, attributes, quantization=None):
        self.source, self.draco, self.indices, self.attributes = source, draco, indices, attributes
        self.quantization = quantization or {}


class GltfDracoLoader:
    """Decodes the compressed primitives of many assets in one batch on one GPU."""

    def __init__(self, context=None):
        self.ctx = context or default_context()

    def load(self, sources, quantized=False):
        """One batch, one decode, ONE download: the vertex arrays of the batch (Batch.vertex_arrays) are already what glTF wants,
        a row per point.  quantized=True: positions, normals and texture coordinates stay the integers the stream carries (uint16;
        normals as two octahedral coordinates) and DecodedPrimitive.quantization[semantic] is (min, range, bits) -- the form
        KHR_mesh_quantization lets a renderer consume; an attribute quantised with more than 16 bits comes back as floats."""
        assets = [s if isinstance(s, GltfAsset) else read_asset(s) for s in sources]
        prims = [p for a in assets for p in draco_primitives(a)]
        results = [[] for _ in assets]
        if not prims:
            return results
        batch = Batch(self.ctx, [p.stream for p in prims])
        try:
            batch.decode(wait=False)
            batch.vertex_arrays("quantized" if quantized else "values")
            index_of = {id(a): i for i, a in enumerate(assets)}
            for i, p in enumerate(prims):
                views = batch.vertex_views(i)
                if any(a["values"] is None for a in views["attributes"]):          # more than 16 bits: those rows as floats, the old way
                    for a, att in zip(views["attributes"], batch.result(i).ConnectedData.Attributes):
                        if a["values"] is None:
                            a["values"] = att.Values[att.PointMap]
                results[index_of[id(p.asset)]].append(self._expand(p, batch.mesh_info(i), views))
        finally:
            batch.close()
        return results

    @staticmethod
    def _expand(p, info, views):
        where = "%s: mesh %d primitive %d" % (p.asset.name, p.mesh, p.primitive)
        if views["indices"] is None:
            raise InvalidDataException("%s: the stream is a point cloud" % where)
        accessors = p.asset.doc.get("accessors", [])

        def accessor(index, what):
            if index is None:
                return None
            if not 0 <= index < len(accessors):
                raise InvalidDataException("%s: %s accessor %d does not exist" % (where, what, index))
            return accessors[index]

        indices = views["indices"].astype(np.uint32).reshape(-1)          # copies: the views die with the batch
        acc = accessor(p.indices_accessor, "indices")
        if acc is not None and int(acc.get("count", -1)) != indices.size:
            raise InvalidDataException("%s: indices accessor counts %s, the stream has %d" % (where, acc.get("count"), indices.size))
        ident = np.arange(info.num_points, dtype=np.uint32)
        atts = []
        for a in views["attributes"]:
            att = PointAttribute(a["info"], np.array(a["values"]), ident, None)
            att.UniqueEntriesCount, att.IsMappingIdentity = info.num_points, True
            atts.append(att)
        draco = Draco(DracoHeader(info), Mesh(atts, info.num_points, indices.reshape(-1, 3).astype(np.int32)))
        attributes, quantization = {}, {}
        for semantic, uid in p.attribute_ids.items():
            k = next((k for k, a in enumerate(atts) if a.UniqueId == uid), None)
            if k is None:
                raise InvalidDataException("%s: no Draco attribute with unique id %d (%s)" % (where, uid, semantic))
            values = atts[k].Values                                       # one value per point = per glTF vertex
            acc = accessor(p.accessors.get(semantic), semantic)
            if acc is not None:
                if int(acc.get("count", -1)) != info.num_points:
                    raise InvalidDataException("%s: %s accessor counts %s, the stream has %d points" % (where, semantic, acc.get("count"), info.num_points))
                nc = _TYPE_COMPONENTS.get(acc.get("type"))
                if nc is not None and nc != views["attributes"][k]["info"].num_components:
                    raise InvalidDataException("%s: %s accessor is %s, the stream has %d components" % (where, semantic, acc.get("type"), views["attributes"][k]["info"].num_components))
            attributes[semantic] = values
            if views["attributes"][k]["quantization"] is not None:
                quantization[semantic] = views["attributes"][k]["quantization"]
        return DecodedPrimitive(p, draco, indices, attributes, quantization)


# ------------------------------------------------------------------------------------------------------------ the writer
_COMPONENT_DTYPES = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}


def read_accessor(asset, index):
    """The elements of accessor `index` as an array [count, components] of its component type (byteStride honoured)."""
    accessors = asset.doc.get("accessors", [])
    if not isinstance(index, int) or not 0 <= index < len(accessors):
        raise InvalidDataException("%s: accessor %r does not exist" % (asset.name, index))
    acc = accessors[index]
    dtype, nc = _COMPONENT_DTYPES.get(acc.get("componentType")), _TYPE_COMPONENTS.get(acc.get("type"))
    if dtype is None or nc is None:
        raise InvalidDataException("%s: accessor %d: unknown componentType / type" % (asset.name, index))
    if "sparse" in acc or "bufferView" not in acc:
        raise InvalidDataException("%s: accessor %d: sparse accessors and accessors without a buffer view are not read" % (asset.name, index))
    count = int(acc.get("count", 0))
    view = asset.doc.get("bufferViews", [])[acc["bufferView"]] if 0 <= acc["bufferView"] < len(asset.doc.get("bufferViews", [])) else None
    data = asset.buffer_view(acc["bufferView"])
    row = np.dtype(dtype).itemsize * nc
    stride = int(view.get("byteStride", 0)) or row
    off = int(acc.get("byteOffset", 0))
    if count < 0 or stride < row or off < 0 or (count and off + (count - 1) * stride + row > len(data)):
        raise InvalidDataException("%s: accessor %d leaves its buffer view" % (asset.name, index))
    if count == 0:
        return np.zeros((0, nc), dtype)
    raw = np.frombuffer(data, np.uint8, (count - 1) * stride + row, off)
    rows = np.lib.stride_tricks.as_strided(raw, (count, row), (stride, 1))
    return np.ascontiguousarray(rows).view(dtype).reshape(count, nc)


class PlannedPrimitive:
    """A primitive the writer compresses: where it sits, its MeshData (one row per point, as the accessors give them) and the
    Draco unique id of every semantic (the attribute's index in the stream)."""

    def __init__(self, asset, mesh, primitive, data, attribute_ids, targets=None):
        self.asset, self.mesh, self.primitive, self.data, self.attribute_ids = asset, mesh, primitive, data, attribute_ids
        self.targets = targets or []        # morph targets: per target {semantic: deltas, one row per point of the primitive}


class SkippedPrimitive:
    """A primitive that stays as it is, and why."""

    def __init__(self, asset, mesh, primitive, reason):
        self.asset, self.mesh, self.primitive, self.reason = asset, mesh, primitive, reason


def _listed_semantic(semantic):
    """attribute_type of a semantic that goes through the attribute list (2 colour, 3 texture coordinate, 4 generic), or None."""
    head, _, n = semantic.rpartition("_")
    if not n.isdigit():
        return None
    if head == "COLOR":
        return 2
    if head == "TEXCOORD":
        return 3
    return 4 if head in ("JOINTS", "WEIGHTS") else None


def _weld_conflict(key_rows, deltas, used):
    """Do two used points whose rows in every array of `key_rows` are byte-equal have different rows in `deltas`?  (The weld joins
    such points, and the stream carries the row of one of them: the other's delta would be lost.)"""
    key = np.concatenate([np.ascontiguousarray(k).view(np.uint8).reshape(len(k), -1) for k in key_rows], axis=1)[used]
    d = np.ascontiguousarray(deltas).view(np.uint8).reshape(len(deltas), -1)[used]
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return bool((d != d[first[inverse.reshape(-1)]]).any())


def plan_compression(assets, shared_grid=None, weld_attributes=False):
    """Needs no device.  (planned, skipped): every TRIANGLES primitive with float32 VEC3 POSITION and indices becomes a MeshData
    -- NORMAL (float32 VEC3) and TEXCOORD_0 (float32 VEC2) as built-ins, COLOR_n, JOINTS_n, WEIGHTS_n, TEXCOORD_n in other forms
    through the attribute list in their component types -- every other primitive is skipped with the reason.
    shared_grid="mesh": the planned primitives of one glTF mesh, and only those, are one group whose positions share a quantisation
    grid (Grid.shared(): a vertex on the cut between two primitives decodes to the same floats in both); None: every primitive
    on its own bounds.
    Morph targets (`targets`) ride beside the stream: the writer carries their deltas across the encode by the rows the encoder
    tracks (GltfDracoWriter.compress).  A primitive is skipped when a target names a semantic that has no base attribute of that
    name in the stream, or with "morph target k of S differs between points the weld joins" when two points whose rows in the key
    set S is welded by are byte-equal have different deltas (weld_attributes: as the Config of the encode will have it -- the
    attributes of the list are then key sets of their own, else part of the positions' key)."""
    from .encoder import Attribute, Grid, MeshData
    if shared_grid not in (None, "mesh"):
        raise ValueError("shared_grid %r: None or \"mesh\"" % (shared_grid,))
    planned, skipped = [], []
    groups = 0
    for asset in assets:
        accessors = asset.doc.get("accessors", [])
        for mi, mesh in enumerate(asset.doc.get("meshes", [])):
            groups += 1                                      # (group 0 is what a mesh without one has)
            for pi, prim in enumerate(mesh.get("primitives", [])):
                def skip(reason):
                    skipped.append(SkippedPrimitive(asset, mi, pi, reason))
                atts = prim.get("attributes", {})
                if EXTENSION in prim.get("extensions", {}):
                    skip("already compressed"); continue
                if prim.get("mode", 4) != 4:
                    skip("mode %d: only TRIANGLES (4) are compressed" % prim.get("mode")); continue
                if prim.get("indices") is None:
                    skip("no indices"); continue
                if "POSITION" not in atts:
                    skip("no POSITION"); continue

                def form(semantic):
                    a = accessors[atts[semantic]] if isinstance(atts[semantic], int) and 0 <= atts[semantic] < len(accessors) else {}
                    return a.get("componentType"), a.get("type")
                if form("POSITION") != (5126, "VEC3"):
                    skip("POSITION is not float32 VEC3"); continue
                try:
                    pos = read_accessor(asset, atts["POSITION"])
                    idx = read_accessor(asset, prim["indices"])
                    if idx.shape[1] != 1 or idx.dtype not in (np.uint8, np.uint16, np.uint32) or len(idx) % 3 or len(idx) == 0:
                        skip("indices are not a list of triangles"); continue
                    normals = texcoords = None
                    ids, listed, why = {"POSITION": 0}, [], None
                    if "NORMAL" in atts and form("NORMAL") == (5126, "VEC3"):
                        normals = read_accessor(asset, atts["NORMAL"])
                        ids["NORMAL"] = len(ids)
                    if "TEXCOORD_0" in atts and form("TEXCOORD_0") == (5126, "VEC2"):
                        texcoords = read_accessor(asset, atts["TEXCOORD_0"])
                        ids["TEXCOORD_0"] = len(ids)
                    for semantic in atts:
                        if semantic in ids:
                            continue
                        kind = _listed_semantic(semantic)
                        if kind is None:
                            why = "attribute %s is not compressed" % semantic
                            break
                        values = read_accessor(asset, atts[semantic])
                        if values.shape[1] > 4:
                            why = "attribute %s has more than 4 components" % semantic
                            break
                        ids[semantic] = len(ids)
                        listed.append(Attribute(values, attribute_type=kind, normalized=bool(accessors[atts[semantic]].get("normalized", False))))
                    if why is None and len(ids) > 16:
                        why = "more than 16 attributes"
                    rows = [normals, texcoords] + [a.values for a in listed]
                    if why is None and any(r is not None and len(r) != len(pos) for r in rows):
                        why = "attribute accessors of different counts"
                    targets, used = [], None
                    if why is None and prim.get("targets"):      # (the points the faces name: what the weld looks at)
                        used = np.unique(idx.astype(np.int64))
                        if int(used.max()) >= len(pos):
                            why = "morph targets over indices out of range"
                    for k, target in enumerate(prim.get("targets") or []):
                        if why is not None:
                            break
                        deltas = {}
                        for semantic, accessor in target.items():
                            if semantic not in ids:
                                why = "morph target %d of %s: no base attribute of that name in the stream" % (k, semantic)
                                break
                            d = read_accessor(asset, accessor)
                            if len(d) != len(pos):
                                why = "attribute accessors of different counts"
                                break
                            # the key set the semantic is welded by: its own rows, or for what stays in the vertex key that key
                            in_key = [pos] + [a.values for j, a in enumerate(listed) if not weld_attributes or 1 + (normals is not None) + (texcoords is not None) + j > 7]
                            own = {"NORMAL": normals, "TEXCOORD_0": texcoords}.get(semantic)
                            if own is None and semantic != "POSITION":
                                j = ids[semantic] - 1 - (normals is not None) - (texcoords is not None)
                                own = listed[j].values if weld_attributes and ids[semantic] <= 7 else None
                            if _weld_conflict(in_key if own is None else [own], d, used):
                                why = "morph target %d of %s differs between points the weld joins" % (k, semantic)
                                break
                            deltas[semantic] = d
                        targets.append(deltas)
                    if why is not None:
                        skip(why); continue
                except InvalidDataException as e:
                    skip(str(e)); continue
                if shared_grid == "mesh":
                    data = MeshData(pos, idx.astype(np.uint32).reshape(-1, 3), normals, texcoords, attributes=listed, position_grid=Grid.shared(), group=groups)
                else:
                    data = MeshData(pos, idx.astype(np.uint32).reshape(-1, 3), normals, texcoords, attributes=listed)
                planned.append(PlannedPrimitive(asset, mi, pi, data, ids, targets))
    return planned, skipped


def _references(doc, key, out):
    if isinstance(doc, dict):
        for k, v in doc.items():
            if k == key and isinstance(v, int) and not isinstance(v, bool):
                out.append((doc, k))
            else:
                _references(v, key, out)
    elif isinstance(doc, list):
        for v in doc:
            _references(v, key, out)


def _used_accessors(doc):
    used = set()
    for mesh in doc.get("meshes", []):
        for prim in mesh.get("primitives", []):
            used.update(v for v in prim.get("attributes", {}).values() if isinstance(v, int))
            if isinstance(prim.get("indices"), int):
                used.add(prim["indices"])
            for t in prim.get("targets", []) or []:
                used.update(v for v in t.values() if isinstance(v, int))
    for anim in doc.get("animations", []):
        for smp in anim.get("samplers", []):
            used.update(v for v in (smp.get("input"), smp.get("output")) if isinstance(v, int))
    for skin in doc.get("skins", []):
        if isinstance(skin.get("inverseBindMatrices"), int):
            used.add(skin["inverseBindMatrices"])
    for node in doc.get("nodes", []):
        for ext in (node.get("extensions") or {}).values():
            if isinstance(ext, dict):
                used.update(v for v in (ext.get("attributes") or {}).values() if isinstance(v, int))
    return used


def rewrite_asset(asset, coded):
    """Needs no device.  The asset as GLB bytes with the primitives of `coded` -- {(mesh, primitive): (stream, num_points, num_faces,
    {semantic: unique id})}, with morph targets a fifth element [{semantic: deltas, one row per point of the stream}] that is
    written as uncompressed accessors of num_points rows (min / max recomputed) -- carrying KHR_draco_mesh_compression: the stream in a buffer view of its own, accessors of the
    decoded counts without buffer views (copies: an accessor may serve other primitives), extensionsUsed / extensionsRequired.
    Accessors no primitive, animation or skin names any more lose their buffer views, buffer views nothing names are dropped, and
    what is left is packed into the one binary chunk."""
    doc = json.loads(json.dumps(asset.doc))
    accessors = doc.setdefault("accessors", [])
    views = doc.setdefault("bufferViews", [])
    before = _used_accessors(doc)
    streams = []
    for (mi, pi), entry in sorted(coded.items()):
        stream, num_points, num_faces, ids = entry[:4]
        prim = doc["meshes"][mi]["primitives"][pi]

        def fresh(index, count):
            acc = {k: v for k, v in accessors[index].items() if k not in ("bufferView", "byteOffset", "sparse")}
            acc["count"] = int(count)
            accessors.append(acc)
            return len(accessors) - 1
        prim["attributes"] = {s: fresh(a, num_points) for s, a in prim["attributes"].items()}
        prim["indices"] = fresh(prim["indices"], 3 * num_faces)
        streams.append(bytes(stream))
        views.append({"buffer": -1 - (len(streams) - 1), "byteLength": len(stream)})        # (negative: stream k, placed below)
        prim.setdefault("extensions", {})[EXTENSION] = {"bufferView": len(views) - 1, "attributes": {s: int(i) for s, i in ids.items()}}
        for k, deltas in enumerate(entry[4] if len(entry) > 4 else []):
            for semantic, rows in deltas.items():
                rows = np.ascontiguousarray(rows)
                acc = {key: v for key, v in accessors[prim["targets"][k][semantic]].items() if key not in ("bufferView", "byteOffset", "sparse", "min", "max")}
                acc["count"] = int(num_points)
                if len(rows) and (semantic == "POSITION" or "min" in accessors[prim["targets"][k][semantic]]):
                    acc["min"], acc["max"] = rows.min(axis=0).tolist(), rows.max(axis=0).tolist()
                streams.append(rows.tobytes())
                views.append({"buffer": -1 - (len(streams) - 1), "byteLength": rows.nbytes})
                acc["bufferView"] = len(views) - 1
                accessors.append(acc)
                prim["targets"][k][semantic] = len(accessors) - 1
    if coded:
        for key in ("extensionsUsed", "extensionsRequired"):
            if EXTENSION not in doc.setdefault(key, []):
                doc[key].append(EXTENSION)
    for index in before - _used_accessors(doc):
        for k in ("bufferView", "byteOffset"):
            accessors[index].pop(k, None)
    refs = []
    _references(doc, "bufferView", refs)
    keep = sorted({d[k] for d, k in refs if 0 <= d[k] < len(views)})
    renumber = {old: new for new, old in enumerate(keep)}
    blob = bytearray()
    packed = []
    for old in keep:
        v = dict(views[old])
        data = streams[-1 - v["buffer"]] if v["buffer"] < 0 else asset.buffer_view(old)
        while len(blob) % 4:
            blob.append(0)
        v["buffer"], v["byteOffset"], v["byteLength"] = 0, len(blob), len(data)
        blob += data
        packed.append(v)
    for d, k in refs:
        if d[k] in renumber:
            d[k] = renumber[d[k]]
    doc["bufferViews"] = packed
    if not packed:
        doc.pop("bufferViews")
    doc["buffers"] = [{"byteLength": len(blob)}] if blob else []
    if not doc["buffers"]:
        doc.pop("buffers")
    if not accessors:
        doc.pop("accessors")
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    blob += b"\0" * (-len(blob) % 4)
    chunks = struct.pack("<II", len(text), _CHUNK_JSON) + text
    if blob:
        chunks += struct.pack("<II", len(blob), _CHUNK_BIN) + bytes(blob)
    return struct.pack("<III", _GLB_MAGIC, 2, 12 + len(chunks)) + chunks


class CompressedAsset:
    """glb: the rewritten asset; compressed: [(mesh, primitive, stream bytes, points in the stream)]; skipped: [SkippedPrimitive],
    the primitives that stayed as they were (outside what the writer compresses, or refused by the encoder) with the reason."""

    def __init__(self, glb, compressed, skipped):
        self.glb, self.compressed, self.skipped = glb, compressed, skipped


class GltfDracoWriter:
    """Compresses the TRIANGLES primitives of many assets in one batch on one GPU."""

    def __init__(self, context=None):
        self.ctx = context or default_context()

    def compress(self, sources, config=None, shared_grid=None):
        """sources: paths, bytes or GltfAssets.  shared_grid="mesh": the primitives of one glTF mesh share the quantisation grid of
        their positions (plan_compression), so that the mesh does not crack along the cuts between them; None: today's bytes.  One EncodeBatch with weld_points=True codes every planned primitive (the other
        options of `config` as given); one decode batch of the result gives the accessor counts -- a stream can hold more points
        than its primitive had where seams cross.  Config(weld_points=True, weld_attributes=True): the attributes of the list
        (TEXCOORD_1 with lightmap charts of its own, COLOR_0 with a hard edge) are welded each alone instead of being part of the
        vertex key, so their seams do not duplicate positions, normals and TEXCOORD_0; the extension's attribute ids and the accessor
        counts follow the stream as ever.  A primitive with morph targets is coded with track_rows: Batch.source_rows on the decode
        batch says which point of the primitive every point of the stream carries, and every target accessor is rewritten,
        uncompressed, with num_points rows delta[rows[S][p]] (plan_compression skips what cannot be carried).  Returns a
        CompressedAsset per source."""
        import copy
        from .encoder import Config, DracoEncoder
        assets = [s if isinstance(s, GltfAsset) else read_asset(s) for s in sources]
        cfg = copy.copy(config) if config is not None else Config()
        cfg.weld_points = True
        planned, skipped = plan_compression(assets, shared_grid, getattr(cfg, "weld_attributes", False))
        cfg.track_rows = any(p.targets for p in planned)
        if cfg.sequential:
            raise ValueError("the writer codes Edgebreaker streams (weld_points): a sequential config keeps the caller's points")
        coded = {id(a): {} for a in assets}
        if planned:
            streams = DracoEncoder(self.ctx).TryEncodeBatch([p.data for p in planned], cfg, keep=cfg.track_rows)
            encoded, batch = streams.encoded, None
            try:
                good = [k for k, s in enumerate(streams) if isinstance(s, bytes)]
                for k, s in enumerate(streams):
                    if not isinstance(s, bytes):
                        skipped.append(SkippedPrimitive(planned[k].asset, planned[k].mesh, planned[k].primitive, "the encoder refused it: %s" % s))
                if good:
                    batch = Batch(self.ctx, [streams[k] for k in good])
                    batch.decode()
                    rows = batch.source_rows(encoded, encoded_mesh=good) if encoded is not None else None
                    for j, k in enumerate(good):
                        info = batch.mesh_info(j)
                        p = planned[k]
                        moved = []
                        if p.targets:
                            if isinstance(rows[j], Exception):
                                raise rows[j]
                            moved = [{s: d[rows[j][p.attribute_ids[s]].astype(np.int64)] for s, d in t.items()} for t in p.targets]
                        coded[id(p.asset)][(p.mesh, p.primitive)] = (streams[k], info.num_points, info.num_faces, p.attribute_ids, moved)
            finally:
                if batch is not None:
                    batch.close()
                if encoded is not None:
                    encoded.close()
        out = []
        for a in assets:
            mine = coded[id(a)]
            out.append(CompressedAsset(rewrite_asset(a, mine), [(m, p, v[0], v[1]) for (m, p), v in sorted(mine.items())],
                                       [s for s in skipped if s.asset is a]))
        return out
