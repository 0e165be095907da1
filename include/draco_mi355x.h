/* include/draco_mi355x.h
 *
 * C-ABI of libdraco_mi355x.so: batched Draco (bitstream 2.2) mesh decode on one
 * MI355X per context.  This is the drop-in boundary under draco-sharp's
 *     DracoDecoder.Decode(BinaryReader)            src/Draco/IO/DracoDecoder.cs:19-42
 * The reference has no FFI layer (everything is managed code), so these entry
 * points are what a P/Invoke binding for that method binds instead of running
 *     ConnectivityDecoder.DecodeConnectivity       src/Draco/IO/Mesh/MeshEdgeBreakerDecoder.cs:25-134
 *     ConnectivityDecoder.DecodeAttributes         src/Draco/IO/ConnectivityDecoder.cs:16-44
 * in-process.  The C# binding is in draco-sharp_amd/csharp/ and INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, blittable structs, no callbacks into
 * the caller, library-owned result memory with explicit release.  Every call
 * returns a dsa_status; the per-mesh status of a batch mirrors the exception
 * the C# would raise for that stream (InvalidDataException /
 * NotImplementedException, src/Draco/IO/Extensions/Assertions.cs:5-24,
 * src/Draco/IO/DracoDecoder.cs:49,70,87-97).  One bad stream never poisons the
 * rest of the batch.
 *
 * Threading: a context is bound to one GPU; its calls that queue work (dsa_batch_create, _decode, _download,
 * dsa_encode_batch) come from one host thread at a time; different contexts (one per GPU) are independent.
 * dsa_batch_wait and dsa_batch_free of a batch may run on another thread than the one that is creating or decoding
 * the context's NEXT batch (the pool does this: a consumer frees job k while the workers decode job k+1): the
 * context's caches of arenas, pinned mirrors and descriptor zones, its count of live batches and the turn of its
 * staging buffers and stream sets are behind a lock.  One batch is still used by one thread at a time.
 */
#ifndef DRACO_MI355X_H_
#define DRACO_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSA_ABI_VERSION 4
#define DSA_MAX_ATTRIBUTES 16  /* attributes per mesh handled by the device path; more: DSA_ERR_NOT_IMPLEMENTED */
#define DSA_NUM_STAGES 8

typedef enum dsa_status {
  DSA_OK = 0,
  DSA_ERR_INVALID_DATA = 1,     /* -> System.IO.InvalidDataException */
  DSA_ERR_NOT_IMPLEMENTED = 2,  /* -> System.NotImplementedException (stream feature outside the device path: see INTEGRATION.md section 5) */
  DSA_ERR_INVALID_ARGUMENT = 3, /* -> System.ArgumentException */
  DSA_ERR_DEVICE = 4,           /* HIP runtime failure; see dsa_last_error */
  DSA_ERR_OUT_OF_MEMORY = 5
} dsa_status;

typedef struct dsa_context dsa_context;
typedef struct dsa_batch dsa_batch;

/* DracoHeader (src/Draco/DracoHeader.cs:5-23) + Mesh/PointCloud counts
 * (src/Draco/IO/Mesh/Mesh.cs:15-69, src/Draco/IO/PointCloud/PointCloud.cs:11-133). */
typedef struct dsa_mesh_info {
  int32_t status;            /* dsa_status of this stream */
  int32_t detail;            /* internal site code of the first failing check (diagnostics): 1xx header / section walk
                              * (k_locate), 2xx Edgebreaker connectivity, 3xx traversal, 4xx entropy decode, 5xx prediction,
                              * 6xx general path (valence, seams, corner attributes, sequential meshes) */
  uint8_t major_version, minor_version, encoder_type, encoder_method;
  uint16_t flags;
  uint16_t decode_path;      /* which kernels decoded the stream: 0 the wave-per-mesh kernels, 1 the general path (predictive traversal,
                              * attribute seams, corner attributes, sequential meshes, the schemes of INTEGRATION.md section 5),
                              * 2 the general path at the second attempt (what the fast kernels found behind the symbol streams) */
  uint32_t num_faces;
  uint32_t num_points;
  uint32_t num_attributes;
  uint64_t drc_bytes;        /* length of the compressed stream */
} dsa_mesh_info;

/* PointAttribute / GeometryAttribute (src/Draco/IO/Attributes/PointAttribute.cs:5-63,
 * GeometryAttribute.cs:8-67) + AttributeTransformData. */
typedef struct dsa_attribute_info {
  int32_t attribute_type;    /* GeometryAttributeType: 0 position, 1 normal, 2 color, 3 texcoord, 4 generic */
  int32_t data_type;         /* DataType enum (src/Draco/IO/Enums/DataType.cs) */
  int32_t num_components;
  int32_t normalized;
  uint32_t unique_id;
  uint32_t num_entries;      /* UniqueEntriesCount: values in traversal order */
  uint32_t byte_stride;      /* packed AoS: size(data_type) * num_components */
  int32_t decoder_type;      /* SequentialAttributeEncoderType: 0 generic, 1 integer, 2 quantization, 3 normals */
  int32_t prediction_method; /* PredictionSchemeMethod */
  int32_t prediction_transform;
  int32_t quantization_bits; /* quantization / octahedron transform parameter */
  float range;               /* quantization transform */
  float min_values[4];
} dsa_attribute_info;

int dsa_abi_version(void);
int dsa_device_count(void);

/* Creates a context on `device`.  `stream` is a hipStream_t to run on (NULL =
 * the context creates its own non-blocking stream). */
dsa_status dsa_context_create(int device, void *stream, dsa_context **out);
void dsa_context_destroy(dsa_context *ctx);
/* Message of the last failing call on this context (valid until the next call). */
const char *dsa_last_error(const dsa_context *ctx);

/* Builds a batch from n host-resident .drc streams: parses the fixed headers to
 * size the device arena, takes it from the context's cache (or allocates it) and
 * queues the upload of the compressed bytes.  The streams are copied into pinned
 * staging memory before the call returns -- the caller's buffers are not
 * referenced afterwards -- and travel in one DMA on the context's upload stream,
 * beside the kernels of a batch decoded meanwhile; dsa_batch_decode orders its
 * kernels behind that transfer. */
dsa_status dsa_batch_create(dsa_context *ctx, uint32_t n, const uint8_t *const *streams, const size_t *lengths,
                            dsa_batch **out);
/* Same, for streams stored back to back in one blob: stream i is
 * blob[offsets[i] .. offsets[i+1]). */
dsa_status dsa_batch_create_packed(dsa_context *ctx, uint32_t n, const uint8_t *blob, const uint64_t *offsets,
                                   dsa_batch **out);
/* Enqueues the device-resident decode of the whole batch (compressed bytes in
 * HBM -> faces, attribute values and point maps in HBM).  Asynchronous.  A context
 * created without a stream of the caller's owns two sets of streams and uses them in
 * turn, so that a decode queued while the previous batch is still running starts beside
 * that batch's tail instead of behind it (two device-resident batches in flight); a
 * context created on a caller's stream runs every decode in that stream's order.
 * Decoding the same batch again waits for its previous decode. */
dsa_status dsa_batch_decode(dsa_batch *batch);
/* Waits for the decode (and for a download / vertex arrays queued with dsa_batch_download / dsa_batch_vertex_arrays) and collects
 * the per-mesh results.  Waits for this batch only: another batch of the same context may
 * be queued behind it (upload of batch k+1 beside the kernels of batch k beside the
 * download of batch k-1 is the intended use; a context keeps up to three arenas and
 * pinned mirrors of freed batches for that). */
dsa_status dsa_batch_wait(dsa_batch *batch);
void dsa_batch_free(dsa_batch *batch);

uint32_t dsa_batch_size(const dsa_batch *batch);
/* Algorithmic bytes of the decoded batch: compressed
 * bytes read + faces + attribute values + explicit point maps written. */
uint64_t dsa_batch_algorithmic_bytes(const dsa_batch *batch);
/* Device bytes of the batch arena (inputs + outputs + scratch). */
uint64_t dsa_batch_arena_bytes(const dsa_batch *batch);

dsa_status dsa_batch_mesh_info(const dsa_batch *batch, uint32_t mesh, dsa_mesh_info *out);
dsa_status dsa_batch_attribute_info(const dsa_batch *batch, uint32_t mesh, uint32_t attribute, dsa_attribute_info *out);

/* Copy-out (device -> caller memory). */
dsa_status dsa_batch_copy_faces(const dsa_batch *batch, uint32_t mesh, int32_t *dst /* num_faces*3, point ids */);
dsa_status dsa_batch_copy_attribute_values(const dsa_batch *batch, uint32_t mesh, uint32_t attribute, void *dst);
dsa_status dsa_batch_copy_point_map(const dsa_batch *batch, uint32_t mesh, uint32_t attribute, uint32_t *dst /* num_points */);
/* Portable (pre-transform) int32 values, for integer-exactness checks. */
dsa_status dsa_batch_copy_portable_values(const dsa_batch *batch, uint32_t mesh, uint32_t attribute, int32_t *dst);

/* Whole-batch copy-out, what DracoDecoder.Decode's caller needs (src/Draco/IO/DracoDecoder.cs:19-42 returns host
 * objects: Mesh.Faces, PointAttribute buffers, src/Draco/IO/Attributes/PointAttribute.cs:38-63).  The arrays a caller
 * receives -- faces, attribute values and point maps of every mesh -- lie in one block of the batch's arena
 * (dsa_batch_output_bytes long).  dsa_batch_download queues ONE device -> host transfer of that block on the context's
 * download stream, ordered behind the batch's kernels, into `dst` (at least dsa_batch_output_bytes; pinned memory --
 * dsa_host_alloc or dsa_host_register -- for the link's full rate) or, with dst == NULL, into a pinned mirror the library
 * owns (valid until dsa_batch_free or the next dsa_batch_decode of the batch).  Asynchronous: dsa_batch_wait waits for it.
 * dsa_batch_output_layout gives the byte offsets of a mesh's arrays inside the block (array lengths: dsa_batch_mesh_info /
 * dsa_batch_attribute_info).  Meshes that were decoded a second time through the general path
 * live in a second block (block == 1), always mirrored by the library.  After a download the dsa_batch_copy_* calls above
 * are served from the host copy. */
#define DSA_OUTPUT_FACES_U16 1u                 /* dsa_mesh_output.flags: the faces of this mesh are uint16 (compact download, <= 65 536 points) */
typedef struct dsa_mesh_output {
  uint32_t block;                               /* 0: the batch's block (dst / mirror), 1: the block of the re-decoded meshes */
  uint32_t flags;                               /* DSA_OUTPUT_* (0 after a full download) */
  uint64_t faces;                               /* int32[num_faces * 3], or uint16[num_faces * 3] with DSA_OUTPUT_FACES_U16 */
  uint64_t values[DSA_MAX_ATTRIBUTES];          /* attribute a: num_entries * byte_stride bytes */
  uint64_t point_map[DSA_MAX_ATTRIBUTES];       /* attribute a: uint32[num_points]; compact download: attributes decoded in one order
                                                 * share one map (equal offsets), UINT64_MAX: the identity (point i = entry i), not stored */
} dsa_mesh_output;
uint64_t dsa_batch_output_bytes(const dsa_batch *batch);
dsa_status dsa_batch_download(dsa_batch *batch, void *dst, size_t dst_bytes);
/* The same with less on the link (ABI 3): the attribute values as they are, the faces as uint16 wherever a mesh has at most 65 536
 * points, and one point map per DISTINCT map -- the attributes of a mesh that were decoded in one traversal order (all per-vertex
 * attributes; the attributes of one corner-attribute decoder) share theirs, the identity map of a point cloud is not stored.  The
 * packing runs on the device behind the decode; dsa_batch_output_layout then describes the compact host copy (flags, shared /
 * absent maps) and the dsa_batch_copy_* calls widen from it.  Meshes decoded a second time (block 1) keep the full layout.
 * 2.25 -> 1.59 MB for a 64k-triangle mesh with three per-vertex attributes. */
uint64_t dsa_batch_compact_bytes(const dsa_batch *batch);
dsa_status dsa_batch_download_compact(dsa_batch *batch, void *dst, size_t dst_bytes);
const void *dsa_batch_host_output(const dsa_batch *batch, uint32_t block);   /* NULL until dsa_batch_wait has seen the download finish */
dsa_status dsa_batch_output_layout(const dsa_batch *batch, uint32_t mesh, dsa_mesh_output *out);
/* Vertex arrays: the results in the form a renderer draws -- per mesh ONE index array and per attribute ONE array with a row per
 * point (= per glTF vertex), each in a block of its own beside the output block.  A HIP kernel behind the decode gathers the rows
 * through the point maps (k_vertex_arrays), so that no map crosses the link and no caller gathers on the host; one transfer
 * downloads the block.  Optional and for the whole batch; dsa_batch_download, _download_compact and every accessor above keep
 * working on a batch that also made vertex arrays (a download and vertex arrays may be outstanding together).  Added after ABI 4
 * without changing it: callers detect the feature by the symbol dsa_batch_vertex_arrays.
 *   When: wherever dsa_batch_download may be called, also before dsa_batch_wait -- queued behind the batch's kernels on the
 *     context's download stream; dsa_batch_wait waits for it too (upload k+1 beside kernels k beside download k-1 keeps one wait per
 *     batch).  A second call while the first is in flight is refused (DSA_ERR_INVALID_ARGUMENT); a new dsa_batch_decode of the batch
 *     invalidates the arrays.
 *   Size: fixed when the request arrives, from the stream headers (attribute types and component counts, the counts of points
 *     and faces): dsa_batch_vertex_arrays_bytes.  Every array is 64-byte aligned.  `dst` (pinned memory for the link's full rate)
 *     must hold that many bytes; with dst == NULL the library uses a pinned mirror of its own (valid until dsa_batch_free, the next
 *     dsa_batch_decode or the next request).
 *   Indices: uint16 where the stream's header bounds the mesh to at most 65 536 points -- encoded vertices + split symbols, known
 *     before the decode: the rule of the compact download -- (DSA_VA_INDICES_U16), else uint32.
 *   DSA_VA_VALUES rows: exactly byte_stride bytes, the bytes of Values[PointMap[p]].
 *   DSA_VA_QUANTIZED rows: an attribute whose decoder_type is 2 (quantisation) or 3 (octahedral normals) is stored as its portable
 *     integers in uint16 rows -- num_components of them, 2 for normals -- with the stride rounded up to a multiple of 4 and zero
 *     filled (what KHR_mesh_quantization lets a renderer consume).  Every other attribute is stored as under DSA_VA_VALUES.
 *     Dequantisation, with the parameters dsa_batch_attribute_info returns, in float32 with two separate roundings:
 *       decoder_type 2:  value[c] = min_values[c] + (float)q[c] * (range / (float)((1 << quantization_bits) - 1))
 *       decoder_type 3:  (s, t) = q on the octahedron of quantization_bits bits (OctahedronToolBox.cs), in float32:
 *                        k = 2 / (float)((1 << quantization_bits) - 2);  y = (float)s * k - 1;  z = (float)t * k - 1;
 *                        x = 1 - |y| - |z|;  o = max(-x, 0);  y += y < 0 ? o : -o;  z += z < 0 ? o : -o;  n = x * x + y * y + z * z;
 *                        value = (x, y, z) * (1 / sqrt((double)n)), each product in double and rounded to float32; (0, 0, 0) where n < 1e-6.
 *     An attribute the decode finds quantised with MORE than 16 bits has no such rows: its array stays unwritten, the layout
 *     reports it DSA_VA_ABSENT with offset UINT64_MAX (the space stays reserved: the layout is a function of the headers) and the
 *     caller takes that attribute through DSA_VA_VALUES or the accessors above.
 *   attribute_types: a mask that leaves an attribute out reserves nothing for it; the layout reports it absent.
 *   An entry index of a point map that is not below the attribute's num_entries gives a row of zeros.
 *   Meshes decoded a second time (decode_path 2) get their arrays from the retry batch as block 1, with the same request;
 *     dsa_batch_wait queues that when it builds the retry batch.  Meshes the general path decodes in the first batch are gathered
 *     like any other.  A failed mesh has no arrays: dsa_batch_vertex_arrays_layout returns its status.
 *   A format or flag outside the values below or a non-zero reserved word fails the call with DSA_ERR_INVALID_ARGUMENT and
 *     dsa_last_error names the field.
 *   The pool (dsa_pool_*, below) exposes its batches as const dsa_batch *: its jobs cannot request vertex arrays. */
#define DSA_VA_VALUES 0          /* rows = the attribute's decoded values */
#define DSA_VA_QUANTIZED 1       /* attributes with decoder_type 2 / 3: the portable integers as uint16 rows; others as VALUES */
#define DSA_VA_DEVICE_ONLY 1u    /* dsa_vertex_request.flags: gather, but queue no device -> host transfer */
typedef struct dsa_vertex_request {
  int32_t format;                /* DSA_VA_VALUES / DSA_VA_QUANTIZED */
  uint32_t flags;                /* DSA_VA_DEVICE_ONLY or 0 */
  uint32_t attribute_types;      /* bit t: include attributes of GeometryAttributeType t; 0 = all */
  uint32_t reserved[5];          /* must be zero */
} dsa_vertex_request;            /* 32 bytes */
#define DSA_VA_ABSENT 1u         /* dsa_vertex_attribute.flags: not in the block (left out by the mask, or not representable) */
typedef struct dsa_vertex_attribute {
  uint64_t offset;               /* byte offset in the block; UINT64_MAX when absent */
  uint32_t stride;               /* bytes per point */
  int32_t data_type;             /* Draco DataType of the stored elements (uint16 = 4 for quantised rows) */
  uint32_t num_components;       /* stored per row (2 for octahedral normals in the quantised format) */
  uint32_t flags;                /* DSA_VA_ABSENT */
} dsa_vertex_attribute;          /* 24 bytes */
#define DSA_VA_INDICES_U16 1u
typedef struct dsa_mesh_vertex_arrays {
  uint32_t block;                /* 0, or 1 for a mesh decoded a second time, as in dsa_mesh_output */
  uint32_t flags;                /* DSA_VA_INDICES_U16 */
  uint64_t indices;              /* uint16 / uint32 [3 * num_faces]; UINT64_MAX for a point cloud */
  uint32_t num_points, num_indices;
  dsa_vertex_attribute attributes[DSA_MAX_ATTRIBUTES];
} dsa_mesh_vertex_arrays;        /* 408 bytes */
/* Bytes of block 0 for this request (0: no batch, or a request the call would refuse). */
uint64_t dsa_batch_vertex_arrays_bytes(const dsa_batch *batch, const dsa_vertex_request *request);
dsa_status dsa_batch_vertex_arrays(dsa_batch *batch, const dsa_vertex_request *request, void *dst, size_t dst_bytes);
/* Where mesh `mesh`'s arrays lie in its block (after dsa_batch_wait; for the most recent request). */
dsa_status dsa_batch_vertex_arrays_layout(const dsa_batch *batch, uint32_t mesh, dsa_mesh_vertex_arrays *out);
const void *dsa_batch_host_vertex_arrays(const dsa_batch *batch, uint32_t block);     /* NULL until dsa_batch_wait has seen the transfer finish (always with DSA_VA_DEVICE_ONLY) */
const void *dsa_batch_device_vertex_arrays(const dsa_batch *batch, uint32_t block);   /* valid until dsa_batch_free, the next dsa_batch_decode or the next request */
/* Pinned host memory for download destinations (and for inputs a caller reuses). */
void *dsa_host_alloc(size_t bytes);
void dsa_host_free(void *p);
dsa_status dsa_host_register(void *p, size_t bytes);
dsa_status dsa_host_unregister(void *p);

/* Device pointers of the results, for consumers that stay on the GPU.  Valid
 * until dsa_batch_free. */
const int32_t *dsa_batch_device_faces(const dsa_batch *batch, uint32_t mesh);
const void *dsa_batch_device_attribute_values(const dsa_batch *batch, uint32_t mesh, uint32_t attribute);
const uint32_t *dsa_batch_device_point_map(const dsa_batch *batch, uint32_t mesh, uint32_t attribute);

/* The metadata block of a stream (header flag 0x8000; what Metadata/MetadataDecoder.cs:5-49 reads: per-attribute
 * elements, then the file element), byte for byte.  The decode path skips it structurally; the managed side parses
 * these bytes into DracoMetadata when the caller asks.  dst may be NULL to query *length (0: no metadata). */
dsa_status dsa_batch_copy_metadata(const dsa_batch *batch, uint32_t mesh, uint8_t *dst, size_t dst_bytes, size_t *length);

/* Diagnostics for the parity tests: intermediate products of the path.
 * what: 0 opposite[3F], 1 corner_to_vertex[3F], 2 data_to_corner[entries], 3 vertex_to_data[vertices],
 *       4 uint32[20] clocks recorded by the per-mesh kernels (s_memtime deltas between phases; [13..17] ticks, start and
 *         duration of the connectivity and the traversal wave in s_memrealtime ticks: readable for failed meshes too),
 *       5 uint32[DSA_MAX_ATTRIBUTES][4] per attribute {symbol source, alphabet size, rANS precision bits (tagged symbols: 1 where
 *         k_tags decoded the tag stream, 0 where the stream walk did), rANS payload bytes},
 *       6 the traversal trace of a -DDSA_TRAV_TRACE build,
 *       7 uint32[4] the pruned schedule of the batch's most recent decode as this mesh saw it, in the NEED_* bits of
 *         csrc/dsa_needs.h: {kernel groups the host parse asked for on the mesh's behalf, groups the mesh's finished descriptor
 *         needed (k_seal; 0 for a failed mesh), groups the decode launched, the host's mask for the whole batch} -- the second is
 *         a subset of the first, and a mesh with a need outside the third does not end with status 0,
 *       8 char[] the same in words: the kernel groups that decode left out (not terminated; `mesh` is ignored).
 *       (7 and 8 describe this batch's decode also for a mesh that was handed to the general path.) */
dsa_status dsa_batch_copy_debug(const dsa_batch *batch, uint32_t mesh, int what, void *dst, size_t dst_bytes, size_t *written);

/* Per-stage device time of the last dsa_batch_decode, in ms (HIP events on the
 * context's stream; enabled with dsa_context_set_profiling).  names[] receives
 * static strings. */
dsa_status dsa_context_set_profiling(dsa_context *ctx, int enabled);
dsa_status dsa_batch_stage_times(const dsa_batch *batch, float ms[DSA_NUM_STAGES], const char *names[DSA_NUM_STAGES]);
/* Durations of the step's main kernels, each from an event pair of its own on the stream it was launched on (profiling
 * enabled): what a row of `rocprofv3 --kernel-trace --stats` shows for that kernel.  *count receives how many kernels
 * were timed in the last decode; at most `capacity` entries of ms[] / names[] (static strings) are written. */
dsa_status dsa_batch_kernel_times(const dsa_batch *batch, float *ms, const char **names, uint32_t capacity, uint32_t *count);
/* Releases what the context keeps between calls: arenas, pinned mirrors and descriptor zones of freed batches, the
 * encoder's lanes (device buffers + pinned staging).  The library does this itself when an allocation fails. */
dsa_status dsa_context_trim(dsa_context *ctx);
/* What the context found when it checked the assumptions its kernel schedule rests on (static string owned by the context): the
 * register counts of the kernels whose occupancy the late symbol launch of a crowded batch is timed by, and whether that
 * mechanism (k_register_gate) is in use or was left out because the counts of this build no longer add up.  Behind it, after a
 * "; ", the kernel groups the context's most recent decode left out because the host parse found no mesh of the batch that needs
 * them (DSA_PRUNE=0 in the environment: nothing is left out); that part changes with every dsa_batch_decode on the context. */
const char *dsa_context_schedule_note(const dsa_context *ctx);

/* ------------------------------------------------------------------ encode direction
 * Drop-in for DracoEncoder.Encode(BinaryWriter, Config, PointCloud, attributes)   src/Draco/IO/DracoEncoder.cs:22-41
 * on a batch of triangle meshes with per-vertex attributes (sequential meshes and point clouds: dsa_encode_sequential_batch
 * below): Edgebreaker (standard traversal) connectivity, quantisation,
 * prediction, symbol statistics, scheme selection and rANS coding as HIP kernels (BASELINE.json configs[4]); the host
 * checks index ranges before and lays the bytes of each stream out after (batches below 256 meshes let the host
 * threads do connectivity and symbol plans as well: the device's fixed latency exceeds their work).
 * Options mirror the reference's Config (src/Draco/IO/Config.cs): quantisation bits per attribute type, speed
 * (compression_level = 10 - speed), prediction scheme overrides. */
typedef struct dsa_encode_options {
  int32_t position_bits;       /* 1..20, default 11 */
  int32_t texcoord_bits;       /* 1..20, default 10 */
  int32_t normal_bits;         /* 2..20, default 8  */
  int32_t single_connectivity; /* 0: one attributes decoder per attribute (Draco default at speed 5), 1: one for all */
  int32_t symbol_scheme;       /* -1 choose per stream (SymbolEncoding.cs:8-40), 0 tagged, 1 raw */
  int32_t compression_level;   /* 0..10, default 5 */
  int32_t position_prediction; /* PredictionSchemeMethod: 1 parallelogram (default), 0 difference; other values fail the call */
  int32_t texcoord_prediction; /* 1 parallelogram (default), 0 difference, 5 TexCoordsPortable; other values fail the call */
} dsa_encode_options;

typedef struct dsa_mesh_input {
  uint32_t num_vertices, num_faces;
  const float *positions;      /* num_vertices * 3 */
  const uint32_t *faces;       /* num_faces * 3 vertex indices; manifold, no isolated vertices (dsa_encode_sequential_batch: any) */
  const float *normals;        /* num_vertices * 3 or NULL */
  const float *texcoords;      /* num_vertices * 2 or NULL */
  /* ABI 4: one generic attribute of 1 - 4 uint8 components per vertex (vertex colours, material ids ...), coded as an integer
   * attribute (SequentialAttributeEncoderType.Integer, GeometryAttributeType.Generic) with the prediction of the positions'
   * family (difference / parallelogram); NULL / 0: none */
  const uint8_t *generic;      /* num_vertices * generic_components or NULL */
  uint32_t generic_components;
  uint32_t reserved;
} dsa_mesh_input;

typedef struct dsa_encoded dsa_encoded;

void dsa_encode_default_options(dsa_encode_options *options);
/* Encodes n meshes (host-resident inputs, copied) into n .drc streams.  Synchronous.  A mesh that cannot be
 * encoded (non-manifold, isolated vertex, index out of range) fails alone: see dsa_encoded_stream. */
dsa_status dsa_encode_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes, const dsa_encode_options *options,
                            dsa_encoded **out);
/* Meshes whose normals and / or texture coordinates are given per corner (UV charts, hard edges): what the reference encoder
 * takes from a point cloud whose attributes map points to values (CornerTable.cs:571-596 CreateFromAttribute).  An edge whose end
 * points carry different ids on its two faces becomes an attribute seam (MeshAttributeCornerTable.cs:32-155): seam bits, the
 * attribute's own corner table and order, a corner attribute in the stream (MeshEdgeBreakerEncoder.cs:403-440).  Standard
 * Edgebreaker, difference / parallelogram prediction, single_connectivity = 0.  Positions and the generic attribute stay per
 * vertex.  Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_batch_corners. */
typedef struct dsa_mesh_corner_input {
  dsa_mesh_input mesh;                 /* as for dsa_encode_batch; when an id array below is set, the matching value array
                                          (mesh.normals / mesh.texcoords) holds num_* rows instead of num_vertices */
  const uint32_t *normal_corners;      /* 3 * num_faces row ids into mesh.normals, or NULL: per vertex */
  const uint32_t *texcoord_corners;    /* 3 * num_faces row ids into mesh.texcoords, or NULL: per vertex */
  uint32_t num_normals, num_texcoords;
} dsa_mesh_corner_input;
/* dsa_encode_batch for dsa_mesh_corner_input; the result is read with the dsa_encoded_* accessors.  A mesh fails alone
 * (dsa_encoded_stream): a row id >= its row count (DSA_ERR_INVALID_DATA), ids with single_connectivity = 1 (DSA_ERR_INVALID_DATA),
 * generic != NULL with generic_components outside 1..4 or ids without their values (DSA_ERR_INVALID_ARGUMENT). */
dsa_status dsa_encode_batch_corners(dsa_context *ctx, uint32_t n, const dsa_mesh_corner_input *meshes,
                                    const dsa_encode_options *options, dsa_encoded **out);
/* The schemes stock encoders write at their default level: valence Edgebreaker symbols, TexCoordsPortable texture coordinates,
 * GeometricNormal normals (Constants.EdgeBreakerTraversalDecoderType, PredictionSchemeMethod).  Added after ABI 4 without
 * changing it: callers detect the feature by the symbol dsa_encode_batch_ex.  A value outside the ones listed fails the call with
 * DSA_ERR_INVALID_ARGUMENT (dsa_last_error says which). */
typedef struct dsa_encode_options_ex {
  dsa_encode_options base;      /* as for dsa_encode_batch; base.texcoord_prediction may also be 5 (TexCoordsPortable),
                                   base.position_prediction is 0 or 1 */
  int32_t edgebreaker_method;   /* 0 standard (default), 2 valence, -1 the reference's rule (DracoEncoder.cs:86-97), decided per
                                   mesh: valence when compression_level > 5 (speed < 5) and the mesh has >= 1000 faces */
  int32_t normal_prediction;    /* 0 difference (default), 6 GeometricNormal */
  int32_t reserved[6];          /* must be zero */
} dsa_encode_options_ex;
void dsa_encode_default_options_ex(dsa_encode_options_ex *options);
/* dsa_encode_batch_corners with the options above: meshes with per-vertex attributes, attributes given per corner, or both.  A
 * mesh fails alone as there; the streams of legal dsa_encode_batch / _corners options are the same bytes through either call. */
dsa_status dsa_encode_batch_ex(dsa_context *ctx, uint32_t n, const dsa_mesh_corner_input *meshes, const dsa_encode_options_ex *options,
                               dsa_encoded **out);
/* Sequential streams: what the reference's encoder writes at speed 10 (DracoEncoder.cs:43-57, :79-82 EncodingMethod ->
 * Mesh/MeshSequentialEncoder.cs) and for a point cloud (PointCloud/PointCloudSequentialEncoder.cs).  No corner table and no
 * traversal: any list of triangles over any set of points is legal -- non-manifold edges and vertices, isolated vertices,
 * degenerate and duplicated faces -- and the stream returns the caller's points and faces in the caller's order (point i is
 * vertex i, face k is faces[3k .. 3k + 2]).  One attributes encoder with a linear sequencer; positions, texture coordinates and
 * the generic attribute by Difference + wrap, normals by the canonicalised octahedral delta.  Attribute quantisation, prediction,
 * the index symbols of compressed connectivity, scheme selection and rANS coding are HIP kernels; raw indices are laid out by
 * the host from the caller's array at the bitstream's widths (u8 below 256 points, u16 below 65 536, varint below 2^21, u32 from
 * there).  Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_sequential_batch. */
typedef struct dsa_encode_sequential_options {
  dsa_encode_options base;       /* position_bits, texcoord_bits, normal_bits, symbol_scheme, compression_level are used;
                                    single_connectivity, position_prediction and texcoord_prediction do not influence the bytes
                                    (values dsa_encode_batch refuses still fail the call) */
  int32_t geometry;              /* 1 triangular mesh (default), 0 point cloud (Constants.EncodingType) */
  int32_t compress_connectivity; /* 0 raw indices (default, = ConfigOptionName.CompressConnectivity false), 1 compressed:
                                    differences of consecutive indices, sign in the low bit, through the symbol coder */
  int32_t reserved[6];           /* must be zero */
} dsa_encode_sequential_options;   /* 64 bytes */
void dsa_encode_sequential_default_options(dsa_encode_sequential_options *options);
/* Encodes n meshes (geometry 1) or n point clouds (geometry 0: positions and the per-point attributes of dsa_mesh_input,
 * num_faces = 0) into n sequential .drc streams, read with the dsa_encoded_* accessors.  An option outside its values or a
 * non-zero reserved entry fails the call with DSA_ERR_INVALID_ARGUMENT (dsa_last_error names the field).  A mesh fails alone
 * (dsa_encoded_stream) and the rest of the batch encodes: positions missing or num_vertices = 0, geometry 1 without faces, a
 * face index >= num_vertices (DSA_ERR_INVALID_DATA); geometry 0 with num_faces != 0 -- faces are not dropped silently -- or
 * generic != NULL with generic_components outside 1..4 (DSA_ERR_INVALID_ARGUMENT).  Nothing else about a mesh is checked. */
dsa_status dsa_encode_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes,
                                       const dsa_encode_sequential_options *options, dsa_encoded **out);
/* The attribute list: any number of further per-vertex attributes behind the built-in ones (positions, normals, the first UV
 * set, mesh.generic), what DracoEncoder.Encode(writer, config, pointCloud, attributes) takes -- COLOR_0, JOINTS_0 / WEIGHTS_0, a
 * second UV set, feature ids.  Integer element types (int8 ... uint32) are coded as they are (SequentialAttributeEncoderType.
 * Integer), float32 is quantised (Quantization); the prediction is the one mesh.generic gets: the positions' family for
 * Edgebreaker streams, Difference for sequential ones -- never TexCoordsPortable, which stays the first UV set's.  Each extra
 * goes into an attributes decoder by the rule that places mesh.generic (single_connectivity).  Values are read on the device in
 * their own element type (k_enc_quantize); 32-bit values are promised within +-2^27 as int32 (the wrap transform's arithmetic is
 * int32).  Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_attributes_batch. */
#define DSA_UNIQUE_ID_DEFAULT 0xFFFFFFFFu
typedef struct dsa_attribute_input {
  int32_t attribute_type;     /* GeometryAttributeType: 2 colour, 3 texture coordinate, 4 generic */
  int32_t data_type;          /* Draco DataType: 1 int8, 2 uint8, 3 int16, 4 uint16, 5 int32, 6 uint32, 9 float32 */
  uint32_t num_components;    /* 1..4 */
  int32_t normalized;         /* 0 / 1, written into the descriptor (integer types; a float32 attribute writes 0) */
  uint32_t unique_id;         /* DSA_UNIQUE_ID_DEFAULT: the attribute's index in the stream */
  int32_t quantization_bits;  /* float32 only: 1..20; 0 = texcoord_bits for attribute_type 3, else 8 */
  const void *values;         /* num_vertices rows, packed (num_components elements of data_type each), one row per vertex / point */
  uint32_t reserved[2];       /* must be zero */
} dsa_attribute_input;          /* 40 bytes */
typedef struct dsa_mesh_attr_input {
  dsa_mesh_corner_input mesh;                 /* as for dsa_encode_batch_ex, its own `generic` included */
  const dsa_attribute_input *attributes;      /* extras, written behind the built-in attributes in list order */
  uint32_t num_attributes, reserved;          /* reserved: must be zero */
} dsa_mesh_attr_input;          /* 96 bytes */
/* dsa_encode_batch_ex (Edgebreaker) and dsa_encode_sequential_batch (sequential meshes, point clouds) for meshes with an
 * attribute list.  With no extras the streams are the bytes of those calls; one extra {4, uint8, nc, 0, default} and no
 * mesh.generic gives the bytes of the same data passed as mesh.generic.  Beside the failures of those calls a mesh fails alone
 * with DSA_ERR_INVALID_ARGUMENT (the message names the attribute's index in the list and the field): built-in attributes plus
 * extras exceed DSA_MAX_ATTRIBUTES; attribute_type, data_type, num_components, normalized or quantization_bits outside the
 * values above; values NULL; a reserved word not zero; two attributes of the mesh with one unique id (built-in attributes have
 * their index); the sequential call with corner ids (it has one value per point and does not drop them silently).  Integer
 * symbols of 2^18 and above (32-bit types with spread values) are written by the tagged scheme, as the CPU coder does; with
 * symbol_scheme = 1 forced such a mesh fails alone with DSA_ERR_INVALID_DATA -- the one place the device refuses what the CPU
 * coder may attempt. */
dsa_status dsa_encode_attributes_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes,
                                       const dsa_encode_options_ex *options, dsa_encoded **out);
dsa_status dsa_encode_attributes_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes,
                                                  const dsa_encode_sequential_options *options, dsa_encoded **out);
/* The levels above the default of the reference's speed ladder, for the widest mesh input.
 *   multi_parallelogram   replaces Parallelogram (method 1) where the stream would carry it.  4 ConstrainedMultiParallelogram
 *       (PredictionSchemeEncoderFactory.cs:63-71): the positions (position_prediction == 1), the first UV set
 *       (texcoord_prediction == 1), and -- where the positions take it -- mesh.generic and every extra.  2 MultiParallelogram:
 *       positions and the first UV set only.  -1: the reference's rule per mesh, 4 when compression_level >= 9 (speed < 2) and
 *       num_vertices >= 40, else off.  Difference, TexCoordsPortable, normals and GeometricNormal are untouched.  The crease flags
 *       of method 4 are chosen per entry: the subset of its (up to four) parallelograms with the smallest wrapped correction --
 *       the CPU coder's choice, not the reference's running-entropy heuristic; any choice decodes.
 *   traversal_method      MeshTraversalMethod per attributes decoder: 0 depth first; 1 prediction degree
 *       (MaxPredictionDegreeTraverser) for the positions' decoder (every decoder's under single_connectivity); 2 for every
 *       decoder without interior seams.  A seamed attribute is always sequenced depth first.
 * With both at 0 the streams are those of dsa_encode_attributes_batch; per-mesh failures are that call's.  A value outside the
 * lists or a non-zero reserved word fails the call with DSA_ERR_INVALID_ARGUMENT and dsa_last_error names the field.  The streams
 * are byte-identical to the CPU coder's.  Added after ABI 4 without changing it: callers detect the feature by the symbol
 * dsa_encode_level_batch. */
typedef struct dsa_encode_level_options {
  dsa_encode_options_ex ex;      /* as for dsa_encode_attributes_batch, same legal values */
  int32_t multi_parallelogram;   /* 0 off (default), 4, 2 or -1 */
  int32_t traversal_method;      /* 0 depth first (default), 1 or 2 */
  int32_t reserved[6];           /* must be zero */
} dsa_encode_level_options;
void dsa_encode_default_level_options(dsa_encode_level_options *options);
dsa_status dsa_encode_level_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes,
                                  const dsa_encode_level_options *options, dsa_encoded **out);
/* dsa_encode_level_batch for meshes that are not clean: the same face twice, fins, fans that meet at a vertex, faces turned
 * over, faces with a repeated index, vertices no face uses -- what every other Edgebreaker call refuses mesh by mesh ("degenerate
 * face", "non-manifold edge (duplicate half-edge)", "non-manifold vertex", "isolated vertex").
 *   topology   0 strict: the bytes and the failures of dsa_encode_level_batch.
 *              1 the reference's corner table, CornerTable(faces) (IO/Mesh/CornerTable.cs:28-43), over the position indices:
 *       degenerate faces (two equal indices) take no part; corners are matched in index order, corner c facing a -> b with the
 *       earliest still-pending b -> a of a face with another tip (the scan over the whole pending list: :346-371 as written
 *       only looks at its first entry); BreakNonManifoldEdges (:396-469) cuts the edges of a fan that reach one vertex twice;
 *       ComputeVertexCorners (:471-547) gives every fan of a vertex behind the first -- faces in index order -- a new vertex with
 *       that vertex as its parent.  The stream codes V' - isolated points and F - degenerate faces
 *       (MeshEdgeBreakerEncoder.cs:41-47); every attribute writes, for a vertex with a parent, the parent's row; quantisation
 *       bounds are taken over all num_vertices rows passed, isolated ones included (AttributeQuantizationTransform.cs:66-100).
 *       Everything else -- holes, start faces, symbols, split events, attribute orders, valence contexts, every prediction
 *       scheme -- runs on the repaired table unchanged.
 * A clean mesh gives the bytes of dsa_encode_level_batch with options.level, whatever `topology` is: the call codes the batch
 * as that call does, and codes again, on the repaired table, only the meshes refused for one of the reasons above (repair
 * kernels of their own, dsa_encode_repair.h; with host connectivity -- DSA_ENC_HOST_CONN, batches below 256 meshes -- the host
 * coder's table).  Per mesh with topology = 1: every face degenerate or num_faces = 0 fails with DSA_ERR_INVALID_DATA ("all
 * triangles are degenerate"); an index out of range, missing positions and the attribute-list checks fail as they do today; a
 * mesh with normal_corners / texcoord_corners whose position table needs repair fails alone with DSA_ERR_NOT_IMPLEMENTED (this
 * call writes no seam tables over a repaired table, dsa_encode_seam_repair_batch does; with clean topology it is coded as by
 * dsa_encode_level_batch).  topology
 * outside {0, 1} or a non-zero reserved word fails the call with DSA_ERR_INVALID_ARGUMENT and dsa_last_error names the field.
 * The streams are byte-identical to the CPU coder's with repair_topology = 1.  Added after ABI 4 without changing it: callers
 * detect the feature by the symbol dsa_encode_repair_batch. */
typedef struct dsa_encode_repair_options {
  dsa_encode_level_options level;   /* as for dsa_encode_level_batch, same legal values */
  int32_t topology;                 /* 0 strict (default), 1 the reference's corner table */
  int32_t reserved[7];              /* must be zero */
} dsa_encode_repair_options;
void dsa_encode_default_repair_options(dsa_encode_repair_options *options);
dsa_status dsa_encode_repair_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes,
                                   const dsa_encode_repair_options *options, dsa_encoded **out);
/* Meshes given as one row per point -- a glTF primitive, an OBJ after triangulation, the output of dsa_batch_vertex_arrays: a
 * point is duplicated wherever a UV chart or a hard edge passes.  `meshes` is read as: mesh.mesh.num_vertices points, every value
 * array (positions, normals, texcoords, generic, every attribute of the list) with one row per point, faces over points;
 * normal_corners / texcoord_corners NULL.  The weld in front of the coder (dsa_encode_weld.h on the device; DSA_ENC_HOST_WELD,
 * batches below 256 meshes: the host threads):
 *   - a point is used when a face names it; a face index >= num_vertices fails the mesh (DSA_ERR_INVALID_DATA, "face index out
 *     of range") before anything is read through the faces;
 *   - two used points are one vertex when their position rows, their mesh.generic rows and their rows in every attribute of the
 *     list are equal byte for byte (floats as bit patterns: -0.0 is not +0.0, a NaN equals the NaN of the same payload) -- so an
 *     attribute of the list that jumps across an edge cuts the positions there; dsa_encode_corner_attributes_batch with
 *     weld_attributes = 1 welds the listed attributes alone instead;
 *   - the representative of a vertex is its used point of smallest index; vertices are numbered by ascending representative;
 *   - normals and texture coordinates are welded the same way, each alone, and go to the coder as rows with ids per corner --
 *     unless no vertex has two of them: then as one row per vertex (the row of the vertex's representative), without ids.
 * The welded mesh is coded as dsa_encode_repair_batch codes it, with the same options, and every per-mesh failure of that call
 * stays (a face degenerate after the weld, a non-manifold edge or vertex under topology = 0, ids with single_connectivity = 1,
 * seams over a table that needs repair: DSA_ERR_NOT_IMPLEMENTED -- see dsa_encode_seam_repair_batch).  A mesh with corner ids set fails alone with
 * DSA_ERR_INVALID_ARGUMENT.  The streams are byte-identical to the CPU coder's on the welded mesh.  Added after ABI 4 without
 * changing it: callers detect the feature by the symbol dsa_encode_points_batch. */
dsa_status dsa_encode_points_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes,
                                   const dsa_encode_repair_options *options, dsa_encoded **out);
/* The weld alone: per mesh the maps between points and vertices / normal rows / texture coordinate rows, in host memory owned by
 * the handle (valid until dsa_welded_free).  *_of_point[num_points]: the class of every point, 0xFFFFFFFF for a point no face
 * names; *_point[count]: the representative point of every class -- what a caller carries further per-point data across the weld
 * with (morph targets: row v of the welded array is row vertex_point[v] of the per-point one).  The normal / texcoord maps are
 * NULL and their counts 0 when the mesh has no such attribute.  *_per_vertex: no vertex has two rows of the attribute (the
 * coder then takes it per vertex). */
typedef struct dsa_welded dsa_welded;
typedef struct dsa_welded_info {
  int32_t status;                        /* DSA_OK, or why the mesh could not be welded */
  uint32_t num_points, num_vertices, num_normals, num_texcoords;
  uint32_t normals_per_vertex, texcoords_per_vertex;
  uint32_t reserved;                     /* zero */
  const uint32_t *vertex_of_point, *vertex_point;
  const uint32_t *normal_of_point, *normal_point;
  const uint32_t *texcoord_of_point, *texcoord_point;
} dsa_welded_info;                       /* 80 bytes */
dsa_status dsa_weld_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, dsa_welded **out);
uint32_t dsa_welded_size(const dsa_welded *welded);
/* Fills `info` for mesh `mesh`; returns the mesh's status (a failed mesh: its status, dsa_last_error says why, the maps NULL). */
dsa_status dsa_welded_mesh(const dsa_welded *welded, uint32_t mesh, dsa_welded_info *info);
void dsa_welded_free(dsa_welded *welded);
/* Quantisation grids given by the caller (the reference's quantization_origin / quantization_range per attribute:
 * SequentialQuantizationAttributeEncoder.cs:19-23, AttributeQuantizationTransform.SetParameters) or shared by the meshes of a
 * batch, for the attributes that are quantised: positions, the first UV set, float32 attributes of the list.  Normals
 * (octahedral) and integer attributes have no grid.
 *   mode 0   the attribute's own bounds (minimum per component, range the largest extent, 1 if that is 0): what every other call
 *       does.  The minimum of a component carries the bits of the first of the caller's rows that attains it (rows [5, -0.0, +0.0]
 *       put 0x80000000 into the header), in the caller's order also where point_order sorts the entries.  A mesh fails alone
 *       with DSA_ERR_INVALID_ARGUMENT when a value of the attribute is not finite ("positions: row 417 is not finite": the
 *       smallest such row, the words of mode 1), else when the range cannot carry the bit depth -- the extent overflowed to
 *       infinity, or (2^bits - 1) / range did (a range below about 2^bits * 2.9e-39): "positions: the range 9.97e-40 of its
 *       values cannot carry 11 quantisation bits (...)".  The first such attribute of the mesh answers.
 *   mode 1   explicit: origin[c] per component and one range; the stream's header carries exactly those floats.  The values are
 *       quantised as always, q = floor((v - origin[c]) * (max_q / range) + 0.5) with every step rounded to float32 and
 *       max_q = 2^bits - 1.  A mesh fails alone with DSA_ERR_INVALID_ARGUMENT when a value of the attribute is not finite or
 *       its q lies outside [0, max_q] (the check is on the integer: a value that rounds onto the last cell is inside).  The
 *       message names the attribute and a row: the smallest row with a value that is not finite, else the smallest row with a
 *       value off the grid ("positions: row 7 is not finite", "attribute 2: row 40 lies off the quantisation grid").
 *   mode 2   shared: for one attribute slot (positions, the first UV set, attribute k of the list) the grid is taken over every
 *       mesh of the batch with the same `group`, that attribute present, mode 2 there and the same component count: minimum per
 *       component over all rows passed (num_vertices rows; num_texcoords rows of texcoords given per corner; every point of
 *       dsa_encode_points input, used or not), range the largest extent, 1 if that is 0.  -0.0 is below +0.0.  A mesh with a
 *       value there that is not finite takes no part in the grid (and fails alone as under mode 1); every other mesh takes
 *       part, also one that fails a later check, so the grid depends on the inputs alone, never on chunks or passes.  With the
 *       grid known the attribute is coded exactly as under mode 1 with that grid.
 * Per mesh, DSA_ERR_INVALID_ARGUMENT with the field in the message: a mode outside 0 - 2, a range that is not finite or <= 0
 * or an origin that is not finite (mode 1), a mode other than 0 for normals or an integer attribute or an attribute the mesh
 * does not have, a reserved word that is not zero.  Origin components beyond the attribute's are not read.
 * With grids == NULL or every mode 0 the streams are byte for byte those of dsa_encode_repair_batch / dsa_encode_points_batch
 * (weld_points = 1) / dsa_encode_attributes_sequential_batch with the same options.  Added after ABI 4 without changing it:
 * callers detect the feature by the symbol dsa_encode_grid_batch. */
typedef struct dsa_quantization_grid {
  float origin[4];
  float range;
  int32_t mode;                            /* 0 own bounds, 1 explicit, 2 shared within `group` */
  uint32_t reserved[2];                    /* must be zero */
} dsa_quantization_grid;                   /* 32 bytes */
typedef struct dsa_mesh_grids {
  dsa_quantization_grid position, texcoord;
  const dsa_quantization_grid *attributes; /* num_attributes entries parallel to dsa_mesh_attr_input.attributes, or NULL: all mode 0 */
  uint32_t group;                          /* mode 2: the meshes that share a grid */
  uint32_t reserved;                       /* must be zero */
} dsa_mesh_grids;                          /* 80 bytes */
typedef struct dsa_encode_grid_options {
  dsa_encode_repair_options repair;        /* as for dsa_encode_repair_batch, same legal values */
  int32_t weld_points;                     /* 0 (default); 1: `meshes` are one row per point, as for dsa_encode_points_batch */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_grid_options;
void dsa_encode_default_grid_options(dsa_encode_grid_options *options);
/* `grids` is parallel to `meshes` (or NULL). */
dsa_status dsa_encode_grid_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                 const dsa_encode_grid_options *options, dsa_encoded **out);
/* dsa_encode_grid_batch that also codes attributes given per corner over a mesh whose topology needs the repair -- the asset from
 * the wild: UV charts and hard edges, and a doubled face, a fin, a sliver with a repeated index, a bow-tie, a two-sided sheet.
 * corner_repair = 1 (needs grid.repair.topology = 1, else the call fails with DSA_ERR_INVALID_ARGUMENT): such a mesh, which the
 * calls above refuse with DSA_ERR_NOT_IMPLEMENTED, is coded on the repaired table: the ids of the faces that are not degenerate,
 * in source order, the attribute seams over the repaired table's edges (an edge the repair cut is a boundary), positions read
 * through the row of every vertex.  Row counts and quantisation bounds stay those of all rows passed.  An id not below its row
 * count fails the mesh alone ("normal id out of range" / "texture coordinate id out of range"), degenerate faces included.  With
 * weld_points = 1 the input is one row per point, else normal_corners / texcoord_corners are the caller's.  Meshes that need no
 * repair, and every mesh under corner_repair = 0, give the bytes and the messages of dsa_encode_grid_batch.  corner_repair
 * outside {0, 1} or a non-zero reserved word fails the call.  The streams are byte-identical to the CPU coder's with
 * repair_topology = 2.  single_connectivity with ids stays refused.  Added after ABI 4 without changing it: callers detect the
 * feature by the symbol dsa_encode_seam_repair_batch. */
typedef struct dsa_encode_seam_repair_options {
  dsa_encode_grid_options grid;            /* as for dsa_encode_grid_batch, same legal values */
  int32_t corner_repair;                   /* 0 (default): per-corner attributes over a mesh that needs repair are refused as ever; 1: coded */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_seam_repair_options;
void dsa_encode_default_seam_repair_options(dsa_encode_seam_repair_options *options);
dsa_status dsa_encode_seam_repair_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                        const dsa_encode_seam_repair_options *options, dsa_encoded **out);
/* dsa_encode_seam_repair_batch that takes row ids per corner for the attributes of the list too (TEXCOORD_1 with its own chart
 * layout, COLOR_0 with a hard edge, feature ids): seams beyond normals and the first UV set.
 *   corners[i].attributes[k] (parallel to meshes[i].attributes; `corners`, or a mesh's `attributes`, NULL: none) gives attribute k
 *   3 * num_faces row ids into its `values`, which then hold num_rows rows.  An interior edge across which the ids differ is a seam
 *   of that attribute alone; the attribute is written as a corner attribute with a connectivity of its own when it has such an
 *   edge, else per vertex.  Its prediction stays the one mesh.generic gets (the positions' family), over its own corner table when
 *   it has interior seams.  Quantisation bounds, integer bounds and shared grids (mode 2) are taken over its num_rows rows.
 *   mesh.generic stays per vertex.  Everything corner_repair = 1 does for normals and texture coordinates holds for these ids too.
 *   weld_attributes = 1 (needs grid.weld_points = 1): every listed attribute leaves the vertex key of the weld (see
 *   dsa_encode_points_batch) and is a key set of its own, welded like normals and texture coordinates: the vertex key is then
 *   positions + mesh.generic, and a listed attribute goes on per corner when some vertex has two of its rows, else per vertex with
 *   the representative's row and no ids.  A lightmap set then cuts its own connectivity only and the surface stays watertight.
 *   This library's decoder takes corner attributes for attribute data 0 to 6, so: a listed attribute whose index in the stream
 *   (positions 0, then normals, texcoords, generic where present, then the list) is above 7 stays in the vertex key under
 *   weld_attributes = 1, and explicit ids on such an attribute fail the mesh alone with DSA_ERR_INVALID_ARGUMENT ("attribute k:
 *   corner ids on attribute j of the stream ...").
 * Per mesh: an id at or above num_rows: DSA_ERR_INVALID_DATA "attribute k id out of range" (degenerate faces included); explicit
 * ids together with weld_points: DSA_ERR_INVALID_ARGUMENT as for the built-in ids; a non-zero reserved word of either struct:
 * DSA_ERR_INVALID_ARGUMENT; ids with single_connectivity stay refused.  The call fails with DSA_ERR_INVALID_ARGUMENT for
 * weld_attributes outside {0, 1}, weld_attributes = 1 without weld_points, or a non-zero reserved word of the options.  With
 * corners == NULL and weld_attributes = 0 streams and messages are byte for byte those of dsa_encode_seam_repair_batch.  The
 * streams are byte-identical to the CPU coder's.  dsa_weld_batch has no such mode: callers of weld_attributes get the streams.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_corner_attributes_batch. */
typedef struct dsa_attribute_corners {
  const uint32_t *corners;                 /* 3 * num_faces row ids into the attribute's values, or NULL: per vertex */
  uint32_t num_rows;                       /* rows of `values` when corners != NULL */
  uint32_t reserved;                       /* must be zero */
} dsa_attribute_corners;                   /* 16 bytes */
typedef struct dsa_mesh_attribute_corners {
  const dsa_attribute_corners *attributes; /* num_attributes entries parallel to dsa_mesh_attr_input.attributes, or NULL */
  uint32_t reserved[2];                    /* must be zero */
} dsa_mesh_attribute_corners;              /* 16 bytes */
typedef struct dsa_encode_corner_attributes_options {
  dsa_encode_seam_repair_options seam_repair; /* as for dsa_encode_seam_repair_batch, same legal values */
  int32_t weld_attributes;                 /* 0 (default): today's vertex key; 1: listed attributes welded alone; needs weld_points */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_corner_attributes_options;
void dsa_encode_default_corner_attributes_options(dsa_encode_corner_attributes_options *options);
/* `grids` and `corners` are parallel to `meshes` (or NULL). */
dsa_status dsa_encode_corner_attributes_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                              const dsa_mesh_attribute_corners *corners, const dsa_encode_corner_attributes_options *options,
                                              dsa_encoded **out);
/* dsa_encode_corner_attributes_batch whose handle can tell which row of the caller's arrays every entry of a stream carries, so
 * that data which does not travel in the stream (morph targets, simulation state, another LOD's skinning) can be carried across an
 * encode: Edgebreaker renumbers vertices, the weld merges points, the repair adds vertices with parents.
 *   track_rows = 1: the handle keeps, per coded mesh and attribute of the stream (positions 0, then normals, texcoords, generic
 *   where present, then the list), entry_rows[a], uint32[entries of a]: the index of the row of the caller's value array for `a`
 *   whose bytes the encoder read for entry e -- the vertex index of an attribute given per vertex; the row id of an attribute given
 *   per corner (normal_corners / texcoord_corners / dsa_attribute_corners), seamed or not; over a repaired table (topology = 1,
 *   corner_repair = 1) for a vertex the repair made the row read, its root parent's, and nothing for isolated vertices and
 *   degenerate faces, which have no entries; with weld_points = 1 a POINT of the caller's per-point arrays, the one whose row was
 *   read: the representative (smallest index) of the row's class in the key set of the attribute, or of its vertex where the
 *   attribute went to the coder per vertex -- with weld_attributes = 1 the listed attributes by their own sets.  Entries are in the
 *   order the decoder of the attribute produces them (depth first, prediction degree, or a seamed attribute's own walk), which is
 *   what the point maps of a decoded mesh index: rows of point p = entry_rows[a][map[a][p]] (dsa_batch_device_point_map).
 *   Costs 4 bytes per entry and attribute in the handle, and one kernel per chunk (k_enc_entry_rows) whose output leaves the device
 *   with the coded bytes.  track_rows = 0: the bytes, the messages and the work of dsa_encode_corner_attributes_batch.
 * track_rows outside {0, 1} or a non-zero reserved word fails the call with DSA_ERR_INVALID_ARGUMENT and dsa_last_error names
 * the field.  Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_rows_batch. */
typedef struct dsa_encode_rows_options {
  dsa_encode_corner_attributes_options corner_attributes; /* as for dsa_encode_corner_attributes_batch, same legal values */
  int32_t track_rows;                      /* 0 (default): nothing kept; 1: the handle keeps the entry rows */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_rows_options;
void dsa_encode_default_rows_options(dsa_encode_rows_options *options);
dsa_status dsa_encode_rows_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                 const dsa_mesh_attribute_corners *corners, const dsa_encode_rows_options *options, dsa_encoded **out);
/* The same for sequential meshes and point clouds (dsa_encode_attributes_sequential_batch). */
dsa_status dsa_encode_grid_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                            const dsa_encode_sequential_options *options, dsa_encoded **out);
/* dsa_encode_grid_sequential_batch with the points of every stream in an order of the encoder's choosing.  A sequential stream
 * codes its points in the order they come in, Difference + wrap from one to the next, and the format gives that order no meaning:
 * a scan, a particle set or a shuffled sample codes little better than noise as given, and to half its size or less in an order
 * that keeps neighbours together.
 *   point_order = 1: Morton order of the quantised positions.  With q[r][c] the integer the stream codes for component c of
 *   position row r (on the attribute's own bounds, the caller's grid or its group's, whichever applies) and B = position_bits,
 *       key(r) = sum over b < B, c < 3 of ((uint32(q[r][c]) >> b) & 1) << (3 b + 2 - c)      (x the top bit of every triple)
 *   and perm lists the rows in ascending (key(r), r): ties go to the smaller row, so the order is a function of the input alone.
 *   Entry e of EVERY attribute of the stream carries row perm[e] of the caller's array for that attribute; with geometry 1 every
 *   face index f is written rank[f], rank the inverse of perm, faces and the corners within a face in the caller's order.  The
 *   stream is byte for byte that of dsa_encode_grid_sequential_batch for positions[perm], normals[perm], ... every listed
 *   attribute[perm] and rank[faces] with the same options and grids: an ordinary sequential Draco 2.2 stream.  The order is found
 *   on the device (a key per point and a segmented radix sort over all clouds of a chunk, ceil(3 B / 8) passes).  The handle keeps
 *   perm per coded stream, 4 bytes per point: dsa_encoded_entry_rows returns it for every attribute of the stream, and
 *   dsa_batch_source_rows works with such a handle as with one of dsa_encode_rows_batch.  Every refusal of a mesh keeps its
 *   status and text, and a refused mesh fails alone.
 *   point_order = 0: the bytes, the messages, the work and the identity rows of dsa_encode_grid_sequential_batch.
 * point_order outside {0, 1} or a non-zero reserved word fails the call with DSA_ERR_INVALID_ARGUMENT and dsa_last_error names
 * the field.  Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_ordered_sequential_batch. */
#define DSA_ENCODE_ORDER_TILE 1024u       /* entries of a tile of the sort (what a test of its edges is sized by) */
typedef struct dsa_encode_order_options {
  dsa_encode_sequential_options sequential; /* as for dsa_encode_grid_sequential_batch, same legal values */
  int32_t point_order;                     /* 0 (default): the caller's order; 1: Morton order of the quantised positions */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_order_options;
void dsa_encode_default_order_options(dsa_encode_order_options *options);
dsa_status dsa_encode_ordered_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                               const dsa_encode_order_options *options, dsa_encoded **out);
/* dsa_encode_ordered_sequential_batch that codes one point per occupied quantisation cell of a point cloud.  A scan, a merged set
 * of sweeps or a particle set at 11 - 14 position bits puts many points into one cell of the position grid; the stream would code
 * every one of them (a zero correction per component and a full set of attribute values) and the decoder would hand back points
 * whose positions are bit-identical.  With an explicit dsa_quantization_grid (origin, range) the caller chooses the voxel:
 * range / (2^position_bits - 1).
 *   merge_points = 1 (taken only with point_order = 1 and geometry 0): with key(r) and perm (the rows in ascending (key, row)) as
 *   documented for point_order = 1, entry e of the sorted order is a head iff e == 0 or key[perm[e]] != key[perm[e - 1]]; kept is
 *   the list of perm[e] over the heads in sorted order, m = its length.  The sort is stable, so kept[j] is the smallest input row
 *   of its cell (with voxel_bits = 0: dsa_encode_voxel_sequential_batch below), and the result is a function of the input alone.  The cell IS the key (with voxel_bits = 0), built from the low position_bits bits of
 *   the quantised integers: two rows merge exactly when the plain ordered call would give them equal keys, and no other notion of
 *   equality is introduced.  A value on a grid that the call refuses today is still refused, with its own text.
 *   The stream codes m points; entry j of EVERY attribute carries row kept[j] of the caller's array for that attribute.  Bounds
 *   and quantisers run in front of the merge, so every quantised attribute (positions, the UV set, float attributes of the list)
 *   keeps the bounds of ALL input rows, not of the kept ones: the stream is byte for byte that of
 *   dsa_encode_grid_sequential_batch (geometry 0) for positions[kept], normals[kept], ... every listed attribute[kept] with every
 *   quantised attribute on an explicit grid equal to the bounds of all its rows (origin = the per-component minima, range = the
 *   largest extent, 1 where that is 0) -- where a grid was given or shared, on that grid.  Integer attributes and octahedral
 *   normals carry no bounds.  (A stream on its own bounds and one on the equal explicit grid have identical headers.)
 *   The handle: dsa_encoded_entry_rows returns kept for every attribute, count m; dsa_encoded_row_entries returns for every input
 *   row r the entry j whose cell r lies in (key(kept[j]) == key(r)), count n -- what averages colours, votes labels or counts the
 *   points per cell without redoing the quantisation; 4 bytes per input row in the handle, with merge_points = 1 only, on any
 *   other handle DSA_ERR_INVALID_ARGUMENT and dsa_last_error names merge_points.  dsa_batch_source_rows works with a merged handle
 *   as with an ordered one; the entry count is m.  Found on the device behind the sort (head flags by ballot, a scan of the tiles'
 *   counts, a compaction without atomics; dsa_encode_order.h).  A refused cloud fails alone, with the status and text it has today.
 *   merge_points = 0: the bytes, the messages, the work and the rows of dsa_encode_ordered_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: merge_points outside
 * {0, 1}; merge_points = 1 with point_order != 1; merge_points = 1 with geometry != 0 (merging the points of a sequential mesh
 * would collapse faces and lose seams: meshes are not taken); a non-zero reserved word.  Refusals of the nested option structs
 * keep their own words.  Added after ABI 4 without changing it: callers detect the feature by the symbol
 * dsa_encode_merged_sequential_batch. */
typedef struct dsa_encode_merge_options {
  dsa_encode_order_options order;          /* as for dsa_encode_ordered_sequential_batch, same legal values */
  int32_t merge_points;                    /* 0 (default): every point is coded; 1: one point per occupied cell of the position grid */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_merge_options;
void dsa_encode_default_merge_options(dsa_encode_merge_options *options);
dsa_status dsa_encode_merged_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                              const dsa_encode_merge_options *options, dsa_encoded **out);
/* Of stream `mesh` of a handle of dsa_encode_merged_sequential_batch with merge_points = 1: row_entries, uint32[n], one per input
 * row (above).  dst NULL: the count alone; capacity in elements. */
dsa_status dsa_encoded_row_entries(const dsa_encoded *encoded, uint32_t mesh, uint32_t *dst, size_t capacity, uint32_t *count);
/* dsa_encode_merged_sequential_batch that cuts the Morton order of a point cloud into parts of bounded size, each a stream of its
 * own.  Both directions of the library code a stream on one wave, which suits a batch of many small streams and is the wrong shape
 * for one cloud of millions of points; a run of consecutive entries of the Morton order is a spatially compact set of points, and a
 * sequential stream of it is an ordinary Draco 2.2 point cloud.  The parts of a cloud share its one quantisation grid, so they
 * encode and decode side by side, fit together without cracks, and each comes with a box to cull or stream by.
 *   part_points = N >= 1 (taken only with point_order = 1, geometry 0 and merge_points = 0): with perm the rows in ascending
 *   (key, row) as documented for point_order = 1 and n the cloud's points, P = ceil(n / N) and part p is sorted entries
 *   [floor(p n / P), floor((p + 1) n / P)), computed in 64 bits: every part has 1 .. N points, sizes differ by at most one, and the
 *   result is a function of the input alone.  Part p is coded as a point cloud of its own; entry j of EVERY attribute carries row
 *   perm[lo_p + j].  Bounds and quantisers run once per cloud, in front of the sort, so every quantised attribute of every part
 *   (positions, the UV set, float attributes of the list) keeps the bounds of ALL the cloud's rows, or the grid that was given or
 *   shared: the stream of part p is byte for byte that of dsa_encode_grid_sequential_batch (geometry 0) for positions[perm[lo:hi]],
 *   normals[...], every listed attribute[...] with every quantised attribute on an explicit grid equal to the bounds of all its rows
 *   (origin = the per-component minima, range = the largest extent, 1 where that is 0).  With P = 1 that is the stream of the
 *   ordered call.  Integer attributes and octahedral normals carry no bounds; wrap bounds, symbol statistics, scheme choice and
 *   tables are each part's own.
 *   The handle: dsa_encoded_size is the number of STREAMS -- the inputs in call order, the parts of one input in order p.  An input
 *   that is refused fails alone with the status and text it has today and occupies one stream slot, which returns that status.
 *   dsa_encoded_parts names the slots of an input (on a handle of any other call: first_stream = input, count = 1).
 *   dsa_encoded_entry_rows(stream, a) returns perm[lo_p:hi_p] for every attribute (perm is kept once per cloud),
 *   dsa_batch_source_rows works with the handle as with an ordered one (encoded_mesh[i] names a stream), dsa_encoded_row_entries
 *   stays refused.  dsa_encoded_part_info fills dsa_part_info: qmin / qmax are, per component, the minimum and maximum of the
 *   position integers the part's stream codes (found on the device behind the sort: k_enc_part_bounds, dsa_encode_order.h), box_min /
 *   box_max the floats this library's decoder returns for them on the part's grid -- float(q) * (range / float(2^position_bits - 1))
 *   + origin, every step rounded to float32 -- and since that is monotone in the integer, bit for bit the minimum and maximum of the
 *   part's decoded positions.  On a handle made without part_points >= 1 it returns DSA_ERR_INVALID_ARGUMENT and dsa_last_error
 *   names part_points.
 *   A cloud with ceil(n / N) > DSA_ENCODE_MAX_PARTS fails alone with DSA_ERR_INVALID_ARGUMENT; the message names part_points, n and
 *   the limit.
 *   part_points = 0: the bytes, the messages, the work, the rows and the handle shape of dsa_encode_merged_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: part_points < 0;
 * part_points >= 1 with point_order != 1 (parts are runs of the Morton order); with geometry != 0 (a part of a mesh would need its
 * faces cut); with merge_points = 1; a non-zero reserved word.  Refusals of the nested option structs keep their own words.
 * Not built: parts with merge_points = 1 (the number of kept points, and so of parts, is known only on the device; the merged call
 * already lowers nv there and the same step could size parts -- a follow-up), parts of sequential meshes, parts of the caller's
 * order (point_order = 0).  (The parts as one array per attribute on the decode side: dsa_batch_joined_arrays.)
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_split_sequential_batch. */
#define DSA_ENCODE_MAX_PARTS 65536u        /* parts of one cloud */
typedef struct dsa_encode_split_options {
  dsa_encode_merge_options merge;          /* as for dsa_encode_merged_sequential_batch, same legal values */
  int32_t part_points;                     /* 0 (default): one stream per cloud; N >= 1: parts of at most N points */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_split_options;
void dsa_encode_default_split_options(dsa_encode_split_options *options);
dsa_status dsa_encode_split_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                             const dsa_encode_split_options *options, dsa_encoded **out);
/* The stream slots of input `input` of the call that made the handle: first_stream .. first_stream + count. */
dsa_status dsa_encoded_parts(const dsa_encoded *encoded, uint32_t input, uint32_t *first_stream, uint32_t *count);
typedef struct dsa_part_info {
  uint32_t input, part, parts;             /* which cloud of the call, which of its parts, how many it has */
  uint32_t first_entry, num_points;        /* the part is sorted entries first_entry .. first_entry + num_points of the cloud */
  uint32_t position_bits;
  int32_t qmin[3], qmax[3];                /* per component, over the position integers the part's stream codes */
  float box_min[3], box_max[3];            /* what the decoder returns for qmin / qmax */
  uint32_t reserved[2];                    /* zero */
} dsa_part_info;
dsa_status dsa_encoded_part_info(const dsa_encoded *encoded, uint32_t stream, dsa_part_info *out);
/* dsa_encode_split_sequential_batch for the combination it refuses: one point per quantisation cell (merge_points = 1) AND parts of
 * bounded size -- what a large scan needs, which without the merge codes many bit-identical points per cell and without the parts
 * runs its one merged stream on one wave in both directions.  The number of kept points, and so of parts, is known only on the
 * device; here the parts are sized there (k_enc_part_cells, dsa_encode_order.h, behind the step that already lowers nv), and
 * nothing goes through the host in between: built here.
 *   part_cells = N >= 1 (taken only with point_order = 1, geometry 0, merge_points = 1 and split.part_points = 0): with kept[0 .. m)
 *   and row_entries exactly what merge_points = 1 defines for the cloud, P = ceil(m / N) and part p is kept entries
 *   [floor(p m / P), floor((p + 1) m / P)), computed in 64 bits -- the rule of part_points applied to m in place of n: every part has
 *   1 .. N points, sizes differ by at most one.  Part p is an ordinary Draco 2.2 point-cloud stream; entry j of every attribute
 *   carries row kept[lo_p + j].  Bounds and quantisers run once per cloud, in front of the sort, so every quantised attribute of
 *   every part is on the bounds of ALL n input rows (or the grid given or shared), and the parts fit together without cracks: the
 *   stream of part p is byte for byte what dsa_encode_split_sequential_batch writes for part p of the input rows[kept] on explicit
 *   grids equal to those bounds.  Wrap bounds, symbol statistics, scheme choice and tables are each part's own.
 *   The handle is shaped like a split handle: a slot per STREAM, inputs in call order, the parts of an input in order p; a refused
 *   input keeps one slot and fails alone.  dsa_encoded_parts names the slots of an input; dsa_encoded_part_info(s) gives first_entry
 *   / num_points in KEPT order, qmin / qmax and box_min / box_max as for split parts (the box is bit for bit the box of the part's
 *   decoded positions); dsa_encoded_entry_rows(s, a) returns kept[lo_p:hi_p]; dsa_encoded_row_entries on the FIRST slot of an input
 *   returns the cloud's row_entries in the global kept order (uint32[n]), on a later slot of the input it is refused and the message
 *   names the first slot.  The part and local entry of input row r are searchsorted(first_entry, row_entries[r]) and the difference.
 *   dsa_batch_source_rows works per slot, as with a split handle.
 *   A cloud with ceil(n / N) > DSA_ENCODE_MAX_PARTS fails alone with DSA_ERR_INVALID_ARGUMENT (the host can only bound P by n); the
 *   message names part_cells, n and the limit.
 *   part_cells = 0: the bytes, the messages, the work, the rows and the handle shape of dsa_encode_split_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: part_cells < 0;
 * part_cells >= 1 with merge_points != 1, with point_order != 1, with geometry != 0, with part_points != 0; a non-zero reserved
 * word.  Refusals of the nested option structs keep their own words.
 * Not built: parts of sequential meshes, parts of the caller's order.  (The parts as one array per attribute on the decode side:
 * dsa_batch_joined_arrays, in stream order.)
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_cell_parts_sequential_batch. */
typedef struct dsa_encode_cell_parts_options {
  dsa_encode_split_options split;          /* as for dsa_encode_split_sequential_batch, same legal values */
  int32_t part_cells;                      /* 0 (default): the very request of the split call; N >= 1: parts of at most N kept points */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_cell_parts_options;
void dsa_encode_default_cell_parts_options(dsa_encode_cell_parts_options *options);
dsa_status dsa_encode_cell_parts_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                                  const dsa_encode_cell_parts_options *options, dsa_encoded **out);
/* dsa_encode_cell_parts_sequential_batch with a coarse-to-fine order: additive levels of detail of every merged point cloud, on the
 * device.  A consumer of tiled scans (3D Tiles "ADD" refinement, progressive download) takes a few thousand points that cover the
 * whole cloud first, then the points that refine it, each piece an ordinary stream with a box.
 *   lod_base_bits = D, 1 <= D <= B = position_bits (taken only with point_order = 1, geometry 0, merge_points = 1 and part_cells =
 *   N >= 1; one stream per level is part_cells >= n).  With kept[0 .. m) and key() exactly what merge_points = 1 defines for the
 *   cloud (keys distinct and ascending): for j >= 1, c(j) is the number of leading bit-triples, out of the B triples of a key, that
 *   key(kept[j]) and key(kept[j - 1]) have in common, c = B - ceil(bitlength(key[j] ^ key[j - 1]) / 3) in 0 .. B - 1; level(0) = 0 and
 *   level(j) = max(0, c(j) + 1 - D).  The cloud has L = B - D + 1 levels, 0 .. L - 1.  The points of levels 0 .. l together are
 *   exactly one point per occupied cell of the grid with D + l bits per axis (the cell of a point: the top 3 (D + l) bits of its
 *   key), the cell's first point in Morton order -- so the representative of a coarse cell is also the representative of the finer
 *   cells that contain it -- and all levels together are the kept points.  D = B puts every point in level 0: the streams are byte
 *   for byte those of part_cells.
 *   lod[0 .. m) is kept in ascending (level, position in kept), a stable partition; m_l the points of level l, level l is
 *   lod[base_l .. base_l + m_l).  Level l is cut by the rule of part_cells applied to m_l: P_l = ceil(m_l / N), part p of level l is
 *   entries [base_l + floor(p m_l / P_l), base_l + floor((p + 1) m_l / P_l)), computed in 64 bits; an empty level has no part.  The
 *   stream slots of an input are the parts of level 0, then those of level 1, and so on.  Every slot is an ordinary Draco 2.2
 *   point-cloud stream; entry j of every attribute carries row lod[lo + j].  Bounds and quantisers run once per cloud, in front of
 *   the sort: every stream is byte for byte what dsa_encode_grid_sequential_batch (geometry 0) writes for rows[lod[lo:hi]] with
 *   every quantised attribute on an explicit grid equal to the bounds of ALL n input rows (or the grid given or shared).  Wrap
 *   bounds, symbol statistics, scheme choice and tables are each stream's own.
 *   The handle is shaped like a cell-parts handle, with "kept order" read as "lod order": dsa_encoded_parts and
 *   dsa_encoded_part_info (first_entry / num_points in lod order, part / parts over all slots of the input, the boxes bit for bit the
 *   box of the slot's decoded positions), dsa_encoded_entry_rows(s, a) = lod[lo:hi], dsa_encoded_row_entries on an input's first
 *   slot (for every input row the lod-order entry of its cell), dsa_batch_source_rows per slot.  dsa_part_info is unchanged, its
 *   reserved words stay zero; dsa_encoded_lod_info(encoded, stream, out) says which level a slot belongs to.  On a handle made
 *   without lod_base_bits >= 1 it returns DSA_ERR_INVALID_ARGUMENT and the message names lod_base_bits.
 *   The host can bound the slots only by S_max = ceil(n / N) + L - 1 (sum ceil(m_l / N) <= ceil(m / N) + non-empty levels - 1): the
 *   layout reserves S_max slots and the device sizes them (k_enc_part_cells, dsa_encode_order.h).  A cloud with S_max >
 *   DSA_ENCODE_MAX_PARTS fails alone with DSA_ERR_INVALID_ARGUMENT; the message names lod_base_bits, part_cells, n and the limit.  A
 *   refused cloud keeps one slot.
 *   lod_base_bits = 0: the bytes, the messages, the work, the rows and the handle shape of dsa_encode_cell_parts_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: lod_base_bits < 0;
 * lod_base_bits > position_bits; lod_base_bits >= 1 with part_cells = 0, or without merge_points = 1 / point_order = 1 / geometry 0;
 * a non-zero reserved word.  Refusals of the nested option structs keep their own words.
 * Not built: a representative nearest the cell centre instead of first in Morton order; levels of sequential meshes; levels
 * without the merge.  The joined decode-side layout of the levels, every level a prefix of one array per attribute, is
 * dsa_batch_joined_arrays in stream order (below).
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_lod_sequential_batch. */
typedef struct dsa_encode_lod_options {
  dsa_encode_cell_parts_options cell_parts; /* as for dsa_encode_cell_parts_sequential_batch, same legal values */
  int32_t lod_base_bits;                   /* 0 (default): the very request of the cell-parts call; D >= 1: levels, level 0 on the grid of D bits per axis */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_lod_options;
void dsa_encode_default_lod_options(dsa_encode_lod_options *options);
dsa_status dsa_encode_lod_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                           const dsa_encode_lod_options *options, dsa_encoded **out);
typedef struct dsa_lod_info {
  uint32_t input;                          /* the input the stream belongs to */
  uint32_t level, levels;                  /* its level, and L = position_bits - lod_base_bits + 1 */
  uint32_t cell_bits;                      /* lod_base_bits + level: levels 0 .. level are one point per cell of the grid with so many bits per axis */
  uint32_t level_first_stream, level_streams;      /* the stream slots of this level */
  uint32_t level_points;                   /* m_l */
  uint32_t part_in_level;                  /* stream - level_first_stream */
  uint32_t reserved[4];                    /* zero */
} dsa_lod_info;
dsa_status dsa_encoded_lod_info(const dsa_encoded *encoded, uint32_t stream, dsa_lod_info *out);
/* dsa_encode_lod_sequential_batch with the mean of every cell in chosen attributes of its kept point: what a voxel-grid downsample
 * does to colour, intensity or a UV, on the device.  With merge_points = 1 alone entry j of every attribute carries row kept[j], the
 * smallest input row of the cell (with voxel_bits = 0): for anything but the position that is the value of whichever point came first in the caller's
 * rows.  Here the masked attributes carry the mean over all rows of the cell instead.
 *   mean_attributes: bit a set: attribute a of the STREAM (0 the positions, then normals, texture coordinates, the generic
 *   attribute and the listed attributes, those the cloud has) carries the cell's mean.  Taken only with merge_points = 1 (and so
 *   point_order = 1, geometry 0); part_cells and lod_base_bits compose with it unchanged.
 *   key, perm, kept[0 .. m) and row_entries are exactly what merge_points = 1 defines.  R(j) = { r : row_entries[r] == j }, cnt =
 *   |R(j)|.  For every masked attribute a and component c, q_a[r][c] is the integer the plain call codes for row r: the quantiser's
 *   output on the cloud's bounds or grid for a quantised float attribute, the element widened to int32 for an integer attribute.
 *   Entry j carries
 *       mean = floor((2 S + cnt) / (2 cnt)),   S = sum over r in R(j) of q_a[r][c],
 *   in 64-bit signed arithmetic with floor division: the exact mean, ties toward +infinity; a cell of one point keeps its value.
 *   Pure integer arithmetic: a function of the SET of rows of the cell, not of their order, bit-identical on host and device.  The
 *   mean lies between the minimum and the maximum of its addends, so bounds, grids, histogram sizes, the range of the wrap bounds
 *   and every refusal are those of the call without the mask.  An attribute without its bit carries row kept[j]; positions are
 *   never touched (they are equal inside a cell).
 *   Every stream is byte for byte what the same call with mean_attributes = 0 writes for an input whose masked attributes hold, at
 *   row kept[j], values whose coded integers are the means: for an integer attribute the mean array itself, for a quantised one the
 *   mean integers on the unchanged bounds or grid.  The handle is unchanged in shape: dsa_encoded_entry_rows is kept / lod slices
 *   (the row the entry's unmasked attributes carry), dsa_encoded_row_entries, dsa_encoded_part_info, dsa_encoded_lod_info and
 *   dsa_batch_source_rows work as before; the number of rows of cell j is the count of j in row_entries.
 *   mean_attributes = 0: the bytes, the messages, the work, the rows and the handle shape of dsa_encode_lod_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: mean_attributes != 0
 * without merge_points = 1; a bit at or above DSA_MAX_ATTRIBUTES; a non-zero reserved word.  Refusals of the nested option structs
 * keep their own words.  A cloud fails alone with DSA_ERR_INVALID_ARGUMENT (it keeps one slot; the message names mean_attributes
 * and the attribute) when a set bit names the positions, the normals, or an attribute its stream does not have.
 * On the device two kernels behind the merge (k_enc_mean_sum 24 VGPR / 45 SGPR, k_enc_mean_store 23 / 29; no LDS, no scratch;
 * dsa_encode_order.h) take 0.6 ms of a 64 ms call for a 4 Mi-point scan with a colour and a float attribute in 256 parts, against 264 ms
 * for download, host means and a second encode.
 * Not built: weighted means; means per coarser lod cell (a level's point carries the mean of its finest cell).  Built since, for
 * categories whose mean is a class nobody assigned: a vote for label attributes, dsa_encode_vote_sequential_batch below; and
 * mean normals (octahedral integers do not average across the fold: a vector sum by a fixed-point rule of its own, not a bit of
 * this mask, which stays refused), dsa_encode_normal_mean_sequential_batch below.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_mean_sequential_batch. */
typedef struct dsa_encode_mean_options {
  dsa_encode_lod_options lod;              /* as for dsa_encode_lod_sequential_batch, same legal values */
  uint32_t mean_attributes;                /* 0 (default): the very request of the lod call; bit a: attribute a of the stream carries the cell's mean */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_mean_options;
void dsa_encode_default_mean_options(dsa_encode_mean_options *options);
dsa_status dsa_encode_mean_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                            const dsa_encode_mean_options *options, dsa_encoded **out);
/* dsa_encode_mean_sequential_batch with the most frequent value of every cell in chosen attributes of its kept point: what a
 * voxel-grid downsample does to a classification, an instance id, a return number or a feature id -- categories, whose mean is a
 * class nobody assigned, and of which the kept point otherwise carries whichever row came first in the caller's order.
 *   vote_attributes: bit a set: attribute a of the STREAM (counted as mean_attributes counts them) carries the cell's most frequent
 *   value.  Taken only with merge_points = 1; part_cells, lod_base_bits and mean_attributes (on other attributes) compose with it
 *   as they are.
 *   key, perm, kept, row_entries, R(j) and q_a[r][c] are exactly what the mean call defines.  For a voted attribute a with nc
 *   components the value of row r is the tuple (q_a[r][0], .., q_a[r][nc - 1]) as a whole.  Entry j carries the tuple that the most
 *   rows of R(j) have; among tuples with equally many rows the lexicographically smallest one, components compared as signed 32-bit
 *   integers, component 0 first.  The winner is a function of the SET of rows of the cell, not of their order (ties are the common
 *   case in cells of two to four rows), bit-identical on host and device; a cell of one row keeps its value.  The voted tuple is
 *   the tuple of some row of the cell, so bounds, grids, histogram sizes, wrap ranges and every refusal are those of the call
 *   without the mask.  Integer attributes of every element type, the built-in texture coordinates and quantised float attributes
 *   of 1 or 2 components are voted on their coded integers.
 *   Every stream is byte for byte what the same call with vote_attributes = 0 writes for an input that holds the winners at row
 *   kept[j].  The handle is unchanged: its shape, dsa_encoded_entry_rows, dsa_encoded_row_entries, the cell counts, part_info,
 *   lod_info, dsa_batch_source_rows and the join plan.
 *   vote_attributes = 0: the bytes, the messages, the work and the handle of dsa_encode_mean_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: vote_attributes != 0
 * without merge_points = 1; a bit at or above DSA_MAX_ATTRIBUTES; a bit set in both vote_attributes and mean_attributes; a
 * non-zero reserved word.  Refusals of the nested option structs keep their own words.  A cloud fails alone with
 * DSA_ERR_INVALID_ARGUMENT (it keeps one slot; the message names vote_attributes and the attribute) when a set bit names the
 * positions, the normals (a vote over octahedral integers is not built), an attribute its stream does not have, or an attribute
 * of 3 or 4 components (only tuples that pack into 64 bits are built).
 * On the device four launches behind the merge, beside the mean kernels (k_enc_vote_count, k_enc_vote_best twice, k_enc_vote_store;
 * dsa_encode_order.h): an open-addressing table of two slots a point per voted attribute counts the rows of every (cell, tuple),
 * no sort; DESIGN.md 7.3 has what it costs.
 * Not built: tuples of 3 or 4 components; a vote over normals; weighted votes; votes per coarser lod cell; the winning count or
 * share per cell in the handle; votes without the merge.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_vote_sequential_batch. */
typedef struct dsa_encode_vote_options {
  dsa_encode_mean_options mean;            /* as for dsa_encode_mean_sequential_batch, same legal values */
  uint32_t vote_attributes;                /* 0 (default): the very request of the mean call; bit a: attribute a of the stream carries the cell's most frequent value */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_vote_options;
void dsa_encode_default_vote_options(dsa_encode_vote_options *options);
dsa_status dsa_encode_vote_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                            const dsa_encode_vote_options *options, dsa_encoded **out);
/* dsa_encode_vote_sequential_batch with the mean normal of every cell in the normals of its kept point: what a voxel-grid downsample
 * does to normals.  With merge_points = 1 alone a kept point carries the normal of whichever row came first in the caller's order.
 *   mean_normals = 1: in every cloud that has normals, entry j of the normal attribute carries the code of the normalised sum of the
 *   unit normals of the rows of cell j.  Taken only with merge_points = 1; part_cells, lod_base_bits, mean_attributes and
 *   vote_attributes (on the other attributes) compose with it as they are.  A cloud without normals is coded as before.
 *   The rule works on the octahedral codes (s, t) the plain call codes for the rows at normal_bits = b, in 64-bit integers.  With
 *   max_value = 2^b - 2, c = max_value / 2 and rdiv(num, den) = floor((2 num + den) / (2 den)), floor division, den > 0:
 *     1. a = s - c, b' = t - c; v = (c - |a| - |b'|, a, b') where |a| + |b'| <= c, else
 *        v = (c - |a| - |b'|, sg(a) (c - |b'|), sg(b') (c - |a|)), sg(0) = +1: the integer vector of L1 norm c the code stands for;
 *     2. len = isqrt((v . v) << 24), the exact floor square root, and u_k = rdiv(v_k << 42, len): the unit vector in Q30;
 *     3. U = the sum of u over the cnt rows of the cell;
 *     4. M_k = rdiv(U_k, cnt);
 *     5. A = |M_0| + |M_1| + |M_2|.  A = 0 (the normals cancel): i0 = c, i1 = 0, z positive -- the code the quantiser gives a zero
 *        vector, that of (1, 0, 0).  Else i0 = rdiv(M_0 c, A), i1 = rdiv(M_1 c, A), z negative iff M_2 < 0.  From there the
 *        quantiser's own tail: i2 = c - |i0| - |i1|, its correction where that is negative, the fold and the canonicalisation;
 *     6. a cell of one row keeps its code.
 *   Pure integer arithmetic: a function of the SET of rows of the cell, bit-identical on host and device.  The angle to the
 *   float64 mean direction stays within the quantiser's own largest angle at those bits.  Bounds, grids, histogram sizes and every
 *   refusal are those of the call without it.
 *   Every stream is byte for byte what the same call with mean_normals = 0 writes for an input whose normals are coded, at row
 *   kept[j], as the mean codes.  The handle is unchanged, the cell counts included.
 *   mean_normals = 0: the bytes, the messages, the work and the handle of dsa_encode_vote_sequential_batch.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: mean_normals above 1;
 * mean_normals = 1 without merge_points = 1; a non-zero reserved word.  Refusals of the nested option structs keep their own
 * words, and a mean_attributes or vote_attributes bit on the normals stays refused per cloud.
 * On the device two kernels behind the merge, beside the means and the votes (k_enc_normal_sum, k_enc_normal_store;
 * dsa_encode_order.h); DESIGN.md 7.3 has what they cost.
 * Not built: a vote over normals; weighted means; means per coarser lod cell; mean normals of meshes.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_normal_mean_sequential_batch. */
typedef struct dsa_encode_normal_mean_options {
  dsa_encode_vote_options vote;            /* as for dsa_encode_vote_sequential_batch, same legal values */
  uint32_t mean_normals;                   /* 0 (default): the very request of the vote call; 1: the normals of every kept point are the mean normal of its cell */
  int32_t reserved[7];                     /* must be zero */
} dsa_encode_normal_mean_options;
void dsa_encode_default_normal_mean_options(dsa_encode_normal_mean_options *options);
dsa_status dsa_encode_normal_mean_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                                   const dsa_encode_normal_mean_options *options, dsa_encoded **out);
/* dsa_encode_normal_mean_sequential_batch with voxels coarser than the position grid: with voxel_bits = C >= 1 the merge keeps one
 * point per occupied cell of the grid with C bits per axis, whatever position_bits = B >= C the positions are stored at, and
 * voxel_point says which point.  What PCL VoxelGrid / Open3D voxel_down_sample (centroid) and PCL UniformSampling (nearest) do, with
 * a voxel edge of 2^(B - C) steps of the position grid.
 *   Voxel.  s = B - C; key(r), perm and q[r][c] exactly what point_order = 1 defines; voxel(r) = key(r) >> 3 s, the top 3 C bits of
 *   the key.  Entry e of the sorted order is a head iff e == 0 or voxel(perm[e]) != voxel(perm[e - 1]); m is the number of heads,
 *   first[j] = perm[e] of head j, row_entries[r] the j whose voxel row r lies in, R(j) the rows with row_entries[r] == j, cnt =
 *   |R(j)|.  With s = 0 this is the merge as it stands.  first[j] is the voxel's smallest (key, row): with s > 0 it is NOT in
 *   general the smallest input row of the voxel (a later row may lie in a finer cell that sorts first).
 *   DSA_VOXEL_POINT_FIRST.  kept[j] = first[j]; every attribute carries that row, positions included.
 *   DSA_VOXEL_POINT_CENTROID.  kept[j] = first[j]; component c of the position at entry j is coded as
 *       P[j][c] = floor((2 S + cnt) / (2 cnt)),   S = the sum of q[r][c] over R(j),
 *   the rule of mean_attributes: 64-bit arithmetic, ties upwards, a voxel of one row keeps its value.  Each component's mean lies
 *   between its minimum and maximum over the voxel, so P[j] lies in voxel j: the kept keys stay distinct and ascending, and the
 *   bounds, the grid and every refusal stay those of the call without the option.  P[j] may be a fine cell that no input row
 *   occupies.
 *   DSA_VOXEL_POINT_NEAREST.  In doubled coordinates d_c(r) = 2 (q[r][c] & (2^s - 1)) - (2^s - 1), dist(r) = d_0^2 + d_1^2 + d_2^2
 *   (below 2^42, unsigned 64 bits); kept[j] is the row of R(j) with the smallest (dist, row).  Every attribute carries row kept[j],
 *   positions included, and no value is changed.  A function of the SET of rows.
 *   Composition.  mean_attributes, vote_attributes and mean_normals reduce over R(j) of the VOXEL and write at kept[j]; part_cells
 *   cuts the m entries; part boxes are those of the integers the stream codes (CENTROID: of the centroids); row_entries,
 *   cell_counts, entry_rows, part_info, source_rows and the join plan keep their meaning with "cell" read as "voxel".
 *   Levels.  With lod_base_bits = D the levels are those of the lod rule on the kept keys, 1 <= D <= C and L = C - D + 1: two kept
 *   points differ within their top C triples, so levels 0 .. l are one point per occupied cell of the grid with D + l bits.
 *   dsa_lod_info.levels and cell_bits report L and D + level; the slot bound is ceil(n / N) + L - 1.
 *   Equal streams.  Every stream is byte for byte what dsa_encode_grid_sequential_batch (geometry 0) writes for the m rows kept with
 *   these settings: every quantised attribute on the grid equal to the bounds of all n rows, or on the grid given or shared; for
 *   CENTROID the position integers P in place of the quantiser's output; the masked, voted and normal attributes as their calls
 *   define them over the voxels.
 *   voxel_bits = 0 with voxel_point = 0: the bytes, the messages, the work, the rows and the handle of
 *   dsa_encode_normal_mean_sequential_batch.  voxel_bits = B with any voxel_point: the same streams and rows as well.
 * Fails the call with DSA_ERR_INVALID_ARGUMENT before any mesh is looked at, dsa_last_error naming the field: voxel_bits below 0 or
 * above position_bits; voxel_bits >= 1 without merge_points = 1; voxel_point outside {0, 1, 2}; voxel_point != 0 with voxel_bits =
 * 0; lod_base_bits above voxel_bits when voxel_bits >= 1; a non-zero reserved word.  Refusals of the nested option structs keep
 * their own words, and a mean_attributes or vote_attributes bit on the positions stays refused per cloud.
 * On the device: a shift in the head predicate of the merge and of the cell passes; CENTROID makes the positions a stream of the
 * means pass; NEAREST is a pass of its own in front of them (k_enc_voxel_near, k_enc_voxel_pick; dsa_encode_order.h).
 * Not built: weighted centroids; the row nearest the centroid; a voxel edge that is not a power of two of the grid step; voxels of
 * meshes; reductions per coarser lod cell.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_encode_voxel_sequential_batch. */
#define DSA_VOXEL_POINT_FIRST    0         /* the voxel's first row in (key, row) order, its position as it is */
#define DSA_VOXEL_POINT_CENTROID 1         /* that row, its position replaced by the voxel's mean position */
#define DSA_VOXEL_POINT_NEAREST  2         /* the input row nearest the voxel's centre, as it is */
typedef struct dsa_encode_voxel_options {
  dsa_encode_normal_mean_options normal_mean; /* as for dsa_encode_normal_mean_sequential_batch, same legal values */
  int32_t voxel_bits;                      /* 0 (default): the very request of the normal-mean call; C >= 1: one point per cell of the grid with C bits per axis */
  int32_t voxel_point;                     /* DSA_VOXEL_POINT_* */
  int32_t reserved[6];                     /* must be zero */
} dsa_encode_voxel_options;
void dsa_encode_default_voxel_options(dsa_encode_voxel_options *options);
dsa_status dsa_encode_voxel_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                             const dsa_encode_voxel_options *options, dsa_encoded **out);
/* The rows of a decoded batch per POINT: for every mesh of `batch` and every attribute a of its stream,
 *     rows[a][p] = entry_rows[a][map[a][p]]          (map: the decoder's point -> entry map, dsa_batch_device_point_map)
 * -- which row of the arrays given to the encoder point p carries, gathered on the device (k_source_rows) so that neither the maps
 * nor an array per mesh cross the link.  `encoded` is the handle the streams came from: of dsa_encode_rows_batch with track_rows =
 * 1, or of a sequential call (entry i is row i); a handle without rows fails the call with DSA_ERR_INVALID_ARGUMENT (the message
 * names track_rows).  encoded_mesh[i] names the stream of `encoded` that mesh i of the batch was created from; NULL: stream i.
 * Shaped like dsa_batch_vertex_arrays: the work is queued on the download stream behind the batch's kernels, dsa_batch_wait waits
 * for it, the result is one block of 64-byte aligned uint32 arrays (dsa_batch_source_rows_bytes; dst NULL: a pinned mirror of the
 * library's, dsa_batch_host_source_rows; dst NULL with dst_bytes = DSA_SOURCE_ROWS_DEVICE_ONLY: no host copy, the block stays on the
 * device, dsa_batch_device_source_rows), and dsa_batch_source_rows_layout says where the arrays of a mesh lie.  `encoded` must stay
 * alive until dsa_batch_wait has returned.  A point whose entry lies at or beyond the tracked ones reads 0xFFFFFFFF; a point cloud's
 * identity map is honoured without a stored map.  A mesh fails alone -- nothing is written for it, and the layout call returns
 * its status -- when it failed to decode, when its stream failed to encode, or with DSA_ERR_INVALID_ARGUMENT when its compressed
 * length, its attribute count or an attribute's entry count is not that of the stream named (length and attribute count are
 * known at the call: such a mesh has no room in the block; the entry counts are known behind the decode: the kernel then leaves the
 * mesh's room unwritten).  Meshes on decode_path 2 have theirs in block 1,
 * from the retry batch, as the vertex arrays do.  A new decode of the batch invalidates the arrays.  Batches a pool owns
 * (dsa_pool_*) are const and take no request.  Added after ABI 4 without changing it: callers detect the feature by the symbol. */
#define DSA_SOURCE_ROWS_DEVICE_ONLY (~(size_t)0)
typedef struct dsa_mesh_source_rows {
  uint32_t block;                          /* 0: the batch's block; 1: the block of the meshes decoded a second time */
  uint32_t num_points, num_attributes;
  uint32_t reserved;                       /* zero */
  uint64_t rows[DSA_MAX_ATTRIBUTES];       /* offset inside the block of uint32[num_points]; UINT64_MAX: no such attribute */
} dsa_mesh_source_rows;                    /* 144 bytes */
uint64_t dsa_batch_source_rows_bytes(const dsa_batch *batch, const dsa_encoded *encoded, const uint32_t *encoded_mesh);
dsa_status dsa_batch_source_rows(dsa_batch *batch, const dsa_encoded *encoded, const uint32_t *encoded_mesh, void *dst, size_t dst_bytes);
dsa_status dsa_batch_source_rows_layout(const dsa_batch *batch, uint32_t mesh, dsa_mesh_source_rows *out);
const void *dsa_batch_host_source_rows(const dsa_batch *batch, uint32_t block);
const void *dsa_batch_device_source_rows(const dsa_batch *batch, uint32_t block);
/* Joined vertex arrays: the part streams of a cloud (part_points, merge_points + part_cells, lod_base_bits, mean_attributes cut one
 * cloud into many ordinary streams) as ONE array per attribute and cloud.  A group names meshes first_mesh .. first_mesh + num_meshes
 * of a decoded batch; a HIP kernel behind the decode (k_joined_arrays, dsa_joined_arrays.h) gathers the rows of all its members
 * into the group's arrays, and one transfer downloads the block -- no concatenation per attribute and no inverse permutation on the
 * host.  Shaped like dsa_batch_vertex_arrays and dsa_batch_source_rows.
 *   Block: a function of the stream headers only.  Per group, in group order, each attribute of the members' common attribute table
 *     gets one 64-byte aligned array of num_rows rows, num_rows = the sum of the members' header point counts.  Stride, data type,
 *     components and the DSA_VA_ABSENT rules (the type mask; more than 16 bits in the quantised format) are those of
 *     dsa_batch_vertex_arrays, and a row holds bit for bit what that call with the same `arrays` request puts in the member's own
 *     array.  Meshes of the batch that are in no group get nothing.
 *   order = DSA_JOIN_STREAM_ORDER: the rows of member 0, then member 1, ...; dsa_batch_joined_member says where a mesh's rows start.
 *     Levels: given the members of a lod handle in slot order, level l is a prefix of every array -- rows [0, first_row of the first
 *     member of level l + 1), the whole array for the last level: a caller slices by dsa_batch_joined_member and dsa_encoded_lod_info.
 *   order = DSA_JOIN_INPUT_ORDER: row r is the point that carries row r of the arrays the encoder was given.  Needs `encoded`
 *     (encoded_mesh as for dsa_batch_source_rows; NULL: stream i), a handle of a sequential call whose streams carry every input row
 *     exactly once (point_order 0 or 1, part_points; not merge_points = 1).  The members of a group must be ALL parts of one input, in
 *     part order (a handle without parts: one member per group).  The member's slice of the permutation is uploaded and the kernel
 *     writes point p of member k to row perm[lo_k + p], a bijection onto 0 .. n - 1; a target at or beyond num_rows is skipped.
 *     `encoded` must stay alive until dsa_batch_wait has returned.
 *   When: wherever dsa_batch_vertex_arrays may be called, before dsa_batch_wait included; queued on the download stream behind the
 *     batch's kernels with an event of its own that dsa_batch_wait waits for.  A download, vertex arrays and source rows may be
 *     outstanding beside it; a second join request while one is in flight is refused; a new dsa_batch_decode invalidates the block.
 *     dst == NULL: a pinned mirror of the library's, filled in one transfer (dsa_batch_host_joined_arrays); a dst of the caller's
 *     (dsa_batch_joined_arrays_bytes; pinned for the link's full rate) receives the arrays alone, one transfer per array: bytes of
 *     dst outside the reported arrays are left as they were; DSA_VA_DEVICE_ONLY transfers nothing
 *     (dsa_batch_device_joined_arrays).  Batches a pool owns are const and take no request.
 *   Fails the call with DSA_ERR_INVALID_ARGUMENT, dsa_last_error naming the field: a fault of `arrays`; order outside its values; a
 *     non-zero reserved word; num_groups > 0 with groups == NULL; a group of 0 meshes or one reaching beyond the batch; a mesh in two
 *     groups; DSA_JOIN_INPUT_ORDER without `encoded`, with a handle without rows, or with an Edgebreaker handle; a dst that is too
 *     small.
 *   A group fails alone -- its arrays stay reserved, what they hold is unspecified, dsa_batch_joined_arrays_layout returns the status
 *     and a message that names the group and the member.  Known at the call, DSA_ERR_INVALID_ARGUMENT: a member has faces; members
 *     differ in attribute count, or per attribute in type, data type, components or decoder type; the row sum is above 2^32 - 1; for
 *     input order the members are not the parts of one input in order, the handle is merged, or a member's compressed length or
 *     attribute count is not the named stream's.  Known behind the decode: a member failed to decode (the group gets its status); a
 *     member is on decode_path 2 (DSA_ERR_INVALID_ARGUMENT: the join does not read the retry batch; no point-cloud stream this
 *     library writes goes there); with DSA_VA_QUANTIZED a quantised attribute's (quantization_bits, min_values, range) differs
 *     between members, compared as bit patterns -- one grid is what makes joined integers meaningful (DSA_VA_VALUES needs no such
 *     check).
 * Not in this call: joined index arrays of meshes; input order for merged handles (many rows share an entry: the caller gathers
 * joined[row_entries]); members decoded a second time; a join across batches or pool jobs; glTF.
 * Added after ABI 4 without changing it: callers detect the feature by the symbol dsa_batch_joined_arrays. */
#define DSA_JOIN_STREAM_ORDER 0   /* rows of member 0, then member 1, ...: point p of member k is row first_row[k] + p */
#define DSA_JOIN_INPUT_ORDER  1   /* row r is the point that carries row r of the arrays the encoder was given */
typedef struct dsa_join_group { uint32_t first_mesh, num_meshes; } dsa_join_group;      /* meshes first_mesh .. + num_meshes of the batch */
typedef struct dsa_join_request {
  dsa_vertex_request arrays;      /* format, flags (DSA_VA_DEVICE_ONLY), attribute_types: exactly as for dsa_batch_vertex_arrays */
  int32_t order;                  /* DSA_JOIN_* */
  uint32_t reserved[7];           /* must be zero */
} dsa_join_request;               /* 64 bytes */
typedef struct dsa_joined_arrays {
  uint32_t first_mesh, num_meshes, num_rows; int32_t order;
  dsa_vertex_attribute attributes[DSA_MAX_ATTRIBUTES];
} dsa_joined_arrays;              /* 400 bytes */
/* Bytes of the block for this request (0: no batch, or a request the call would refuse). */
uint64_t dsa_batch_joined_arrays_bytes(const dsa_batch *batch, const dsa_join_request *request, uint32_t num_groups, const dsa_join_group *groups);
dsa_status dsa_batch_joined_arrays(dsa_batch *batch, const dsa_join_request *request, uint32_t num_groups, const dsa_join_group *groups,
                                   const dsa_encoded *encoded, const uint32_t *encoded_mesh, void *dst, size_t dst_bytes);
/* Where group `group`'s arrays lie in the block (after dsa_batch_wait; for the most recent request), or why it has none. */
dsa_status dsa_batch_joined_arrays_layout(const dsa_batch *batch, uint32_t group, dsa_joined_arrays *out);
/* The group of the most recent request mesh `mesh` is a member of, and its rows there in stream order. */
dsa_status dsa_batch_joined_member(const dsa_batch *batch, uint32_t mesh, uint32_t *group, uint32_t *first_row, uint32_t *num_rows);
const void *dsa_batch_host_joined_arrays(const dsa_batch *batch);       /* NULL until dsa_batch_wait has seen the transfer finish (always with DSA_VA_DEVICE_ONLY) */
const void *dsa_batch_device_joined_arrays(const dsa_batch *batch);     /* valid until dsa_batch_free, the next dsa_batch_decode or the next request */
uint32_t dsa_encoded_size(const dsa_encoded *encoded);
/* Bytes of stream `mesh` (owned by `encoded`, valid until dsa_encoded_free) or that mesh's failure status. */
dsa_status dsa_encoded_stream(const dsa_encoded *encoded, uint32_t mesh, const uint8_t **bytes, size_t *length);
/* The entry rows of attribute `attribute` (its index in the stream) of stream `mesh`: *count receives the number of entries, and
 * dst, when not NULL, `*count` rows (capacity: the room in dst, in rows; too little: DSA_ERR_INVALID_ARGUMENT, *count set).  A
 * failed mesh returns its own status.  A handle of a sequential call answers with the identity (entry i is row i).  A handle of
 * an Edgebreaker call made without track_rows = 1 returns DSA_ERR_INVALID_ARGUMENT and dsa_last_error names track_rows. */
dsa_status dsa_encoded_entry_rows(const dsa_encoded *encoded, uint32_t mesh, uint32_t attribute, uint32_t *dst, size_t capacity, uint32_t *count);
/* The number of attributes stream `mesh` has entry rows for (`attribute` above runs below it); the same statuses. */
dsa_status dsa_encoded_attributes(const dsa_encoded *encoded, uint32_t mesh, uint32_t *count);
void dsa_encoded_free(dsa_encoded *encoded);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-GPU submit for a host that is one process (the C# host cannot use torch.distributed): a pool owns one
 * context per listed device and decodes a list of independent streams with one worker thread per context.
 * The reference creates everything per call (src/Draco/IO/DracoDecoder.cs:19-42): streams share nothing, so the
 * partition is free -- streams are sorted by compressed length (longest first, the proxy for decode work), cut into
 * chunks of `chunk_meshes`, and the workers pull chunk after chunk from one atomic queue; a chunk is one batch on the
 * worker's context (no collective, no peer traffic).  A device may be listed more than once
 * (several contexts on one GPU).  dsa_pool_decode blocks until every chunk is decoded; results stay on the device
 * that decoded them and are read through the dsa_batch_* accessors of the batch dsa_pool_job_locate names. */
typedef struct dsa_pool dsa_pool;
typedef struct dsa_pool_job dsa_pool_job;

/* chunk_meshes == 0: chosen per job (one chunk per device up to 4096 meshes each, 4096-mesh chunks beyond).  A worker keeps two
 * chunks in flight on its context (upload of the next beside the kernels of the current).  Jobs may outlive the pool object:
 * dsa_pool_destroy with jobs alive takes effect when the last of them is freed.  One dsa_pool_decode at a time per pool. */
dsa_status dsa_pool_create(const int *devices, uint32_t num_devices, uint32_t chunk_meshes, dsa_pool **out);
void dsa_pool_destroy(dsa_pool *pool);
uint32_t dsa_pool_size(const dsa_pool *pool);                 /* number of contexts / worker threads */
const char *dsa_pool_last_error(const dsa_pool *pool);
dsa_status dsa_pool_decode(dsa_pool *pool, uint32_t n, const uint8_t *const *streams, const size_t *lengths, dsa_pool_job **out);
/* Where stream `stream` of the job was decoded: the batch, its index inside it, and the worker (index into the
 * pool's device list) that took its chunk. */
dsa_status dsa_pool_job_locate(const dsa_pool_job *job, uint32_t stream, const dsa_batch **batch, uint32_t *mesh, uint32_t *worker);
uint32_t dsa_pool_job_chunks(const dsa_pool_job *job);
void dsa_pool_job_free(dsa_pool_job *job);
/* The queue order of a job (no GPU needed): order[0..n) = stream indices longest first (ties by index),
 * chunk_begin[0..chunks] = chunk boundaries in `order` (chunk_begin needs n + 1 entries).  Returns the chunk count. */
uint32_t dsa_pool_plan(uint32_t n, const size_t *lengths, uint32_t chunk_meshes, uint32_t *order, uint32_t *chunk_begin);

#ifdef __cplusplus
}
#endif
#endif /* DRACO_MI355X_H_ */
