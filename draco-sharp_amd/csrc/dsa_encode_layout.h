// draco-sharp_amd/csrc/dsa_encode_layout.h  (included by dsa_encode.h)
//
// Encode direction, the part of a chunk's host work that needs no device and nothing of HIP (it compiles with plain g++ like
// dsa_encode_host.h; tests/hostcheck/enclayout_host.cpp runs it under AddressSanitizer):
//   EncRequest   a call of any encode entry point: the mesh array in its widest form (enc_widen), the options in their widest struct
//   EncChunk     the state of one chunk of a request on its way through the stages of encode_chunk / encode_sequential_chunk
//   enc_plan_mesh / enc_check_sequential_mesh   the host's checks of a mesh and its plan (what the threads over meshes run)
//   enc_layout / enc_layout_sequential          the arena: EncStream / EncConn / EncSeam / EncSeqIdx records, upload lists, sizes
// The arena is laid out by one allocator in two passes over the meshes: the first places what the host provides (faces, corner
// ids, entry maps, topology views, source values, context lists) and lists it for upload, input_bytes is where it ends; the
// second hands out everything the kernels write from there on.  No size is computed anywhere else.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/draco_mi355x.h"
#include "dsa_common.h"
#include "dsa_encode_host.h"
#include "dsa_encode_conn.h"
#include "dsa_encode_repair.h"
#include "dsa_encode_weld.h"
#include "dsa_encode_grid.h"
#include "dsa_encode_seams.h"
#include "dsa_encode_seqidx.h"
#include "dsa_encode_schemes.h"
#include "dsa_encode_multi.h"
#include "dsa_encode_rows.h"
#include "dsa_encode_order.h"

namespace dsa {

struct EncStream {                 // one per (mesh, attribute); lives in device memory, mirrored on the host
  uint64_t src;                    // f32 source values, vertex order, nc_out per vertex
  uint64_t e2v, ops;               // per mesh: entry -> vertex; i32[3*entries] parallelogram operand entries (next, prev, opposite) or -1
  uint64_t vals, d, syms, bl;      // i32[nv*nc] vertex order, i32[nv*nc] traversal order, u32[nv*nc] symbols, u8[nv] bit length per entry
  uint64_t hist_raw;               // u32[hist_cap]
  uint64_t out_rans, out_bits;     // coded bytes
  uint64_t prob, cum;              // u32[num_symbols] (filled by the host between the two device phases)
  uint32_t nv, nc_out, nc, kind;   // nv: entries; kind 0: quantised + wrap, 1: normals (octahedral, canonicalised delta), 2: integers + wrap (src: elements of
                                   //   type `elem`), 3: a valence context list of the connectivity (syms given, nc 1; no values, no prediction)
  uint32_t rows, rows_pad;         // value rows of `src` / `vals` (= nv, but for an attribute given per corner: its row count; k_enc_seam_operands sets nv)
  uint32_t bits, prediction, hist_cap, out_cap;
  float qmin[4], qrange;
  int32_t wrap_mn, wrap_mx;
  uint32_t max_value, overflow;
  unsigned long long total_bl;
  uint32_t hist_tag[33];
  uint32_t method, precision_bits, num_symbols;
  uint32_t rans_len, bits_len;
  uint64_t plan_order, plan_tmp;   // u32[table_cap] each: scratch of k_enc_plan
  uint32_t usbl, plan_status;      // raw scheme: unique-symbols bit length; dsa::plan::PLAN_* of k_enc_plan
  // prediction 5 (TexCoordsPortable, kind 0) and 6 (GeometricNormal, kind 1): the topology view of dsa_encode_schemes.h (EncTopo)
  // -- set by the host, for a seamed attribute on the device path by k_enc_seam_topo -> k_enc_corr
  uint64_t pos_vals, t_c2p, t_c2a, t_opp, t_d2c, t_v2d;
  uint64_t ori;                    // u8[cap] per entry 0 / 2 / 3 (TexCoordsPortable's branch and orientation) -- k_enc_corr -> k_enc_orient
  uint64_t flags;                  // u32[(cap + 31) / 32] side bits, bit k of the list: orientations (delta-coded against true, last
                                   //   entry first; k_enc_orient) or flips (entry order; k_enc_corr) -- -> download (write_rabs)
  uint32_t t_nc3, num_flags;       // 3F; OUTPUT: bits in `flags`
  // prediction 2 / 4 (MultiParallelogram, ConstrainedMultiParallelogram; kind 0 and 2; dsa_encode_multi.h): the topology view above;
  // prediction 4: `ori` holds per entry the parallelograms found and their crease flags (k_enc_multi -> k_enc_crease), `flags` the
  // four crease lists, list j packed from word cr_at[j] on, cr_n[j] bits (OUTPUT) -- k_enc_crease -> download (write_rabs)
  uint32_t cr_at[4], cr_n[4];
  uint32_t pd_want, pad_level;     // pd_want: an attribute given per corner whose decoder takes the prediction-degree order unless it is seamed
  uint32_t linear, elem;           // linear: entry i is value row i (sequential streams, dsa_encode_sequential.h): `d` is `vals`, no e2v, no gather
                                   // elem (kind 2): Draco's data type of `src`, 1 int8, 2 uint8, 3 int16, 4 uint16, 5 int32, 6 uint32
  uint32_t grid_mode;              // kind 0: not 0: qmin / qrange are a grid given by the host (the caller's, or its group's), k_enc_grid_quantize in place
                                   //   of k_enc_bounds and k_enc_quantize
  uint32_t grid_nonfinite, grid_off;      // kind 0: its smallest row with a value that is not finite (on a grid or under own bounds: k_enc_bounds) / on a grid: whose
                                   //   integer leaves 0 .. max_q (the host sets ENC_GRID_NO_ROW)
  uint32_t part;                   // not 0: the stream of a part behind the first of a split cloud (dsa_encode_order.h): src, vals and the quantiser's
                                   //   floats are the first part's: k_enc_bounds / k_enc_quantize leave it alone, and so does k_enc_grid_quantize (its grid_mode is 0)
                                   //   ENC_PART_SIZED set: a part slot whose nv the device decides (k_enc_part_cells), 0 where the cloud has fewer parts
};
// EncStream::part of a part behind the first: ENC_PART_BEHIND, and with sizes of the device's ENC_PART_SIZED as well -- the one
// layout in which a value stream can be empty (a zero-point cloud is refused at the door).  Such a slot must be passed by: no
// kernel and no host step may touch its regions, and it has no piece among the downloads.  k_enc_part_cells therefore turns the
// records of an empty slot into what every step passes by already, an empty list (kind 3, nv 0: k_enc_gather and k_enc_corr return
// on the kind, k_enc_plan, k_enc_rans and the host's plans on the empty list), so that not one instruction of those kernels
// changes: a test of this flag in the prologue of k_enc_rans moved its serial loop and cost the merged call of a 1 Mi-point stream
// 8 %.  The flag itself tells the piece packer, on the host, to emit nothing for the record.
static const uint32_t ENC_PART_BEHIND = 1u, ENC_PART_SIZED = 2u;

// The raw symbol scheme takes symbols below 2^18 (dsa_symbol_plan.h choose_scheme; symbol_stats of the host coder builds no
// histogram of values beyond): no stream's histogram is larger than this, and a stream whose histogram has this size may hold
// symbols beyond it (32-bit integer attributes with spread values) -- those are not counted, and k_enc_plan goes the tagged way.
static const uint32_t ENC_RAW_SYMBOL_LIMIT = 1u << 18, ENC_HIST_CAP_LIMIT = ENC_RAW_SYMBOL_LIMIT + 2u;
static_assert(ENC_HIST_CAP_LIMIT == EM_HIST_CAP_LIMIT, "k_enc_multi counts symbols like k_enc_corr");
// hist_cap of an integer attribute whose values (as int32) span lo .. hi: zig-zagged wrapped corrections lie in 0 .. hi - lo + 1
static inline uint32_t enc_integer_hist_cap(int32_t lo, int32_t hi) {
  const uint64_t span = (uint64_t)((int64_t)hi - (int64_t)lo) + 3ull;
  return (uint32_t)(span < ENC_HIST_CAP_LIMIT ? span : ENC_HIST_CAP_LIMIT);
}

// Value rows and entries of an attribute in traversal order (entry p: the value of the corner the walk reached it by; ids null:
// the corner's vertex) and its parallelogram operand entries on table `ct` (MeshPredictionSchemeParallelogramEncoder.cs:35-56).
template <class CT>
static void entry_maps(const CT &ct, const synth::Sequence &seq, const uint32_t *ids, std::vector<uint32_t> &e2v, std::vector<int32_t> *ops) {
  const uint32_t entries = (uint32_t)seq.data_to_corner.size();
  e2v.resize(entries);
  if (ops) ops->assign((size_t)3 * entries, -1);
  for (uint32_t p = 0; p < entries; ++p) {
    const uint32_t ci = seq.data_to_corner[p];
    e2v[p] = ids ? ids[ci] : ct.vertex(ci);
    if (p == 0 || !ops) continue;
    const uint32_t oci = ct.opposite(ci);
    if (oci == synth::kInvalid) continue;
    const int32_t vo = seq.vertex_to_data[ct.vertex(oci)];
    const int32_t vn = seq.vertex_to_data[ct.vertex(synth::CornerTable::next(oci))];
    const int32_t vp = seq.vertex_to_data[ct.vertex(synth::CornerTable::prev(oci))];
    if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { (*ops)[3 * p] = vn; (*ops)[3 * p + 1] = vp; (*ops)[3 * p + 2] = vo; }
  }
}
}  // namespace dsa

struct dsa_encoded {
  dsa_context *ctx = nullptr;
  std::vector<std::vector<uint8_t>> streams;
  std::vector<int32_t> status;
  std::vector<std::string> messages;
  // entry rows (dsa_encoded_entry_rows).  ROWS_TRACKED: rows[mesh][attribute of the stream], kept by a call with track_rows = 1
  // (dsa_encode_rows.h); ROWS_LINEAR: a sequential call, entry i is row i, and linear[mesh] = (attributes, points) is all it takes;
  // ROWS_ORDERED: a sequential call with point_order = 1 (dsa_encode_order.h): linear[mesh] as before, and order[mesh] the
  // permutation every attribute of the stream went through, kept once -- with merge_points = 1 the kept rows, linear[mesh].second
  // of them, and cells[mesh] the entry of the cell of every input row (dsa_encoded_row_entries); `merged` says which
  enum { ROWS_NONE = 0, ROWS_TRACKED = 1, ROWS_LINEAR = 2, ROWS_ORDERED = 3 };
  int rows_kind = ROWS_NONE;
  std::vector<std::vector<std::vector<uint32_t>>> rows;
  std::vector<std::pair<uint32_t, uint32_t>> linear;
  std::vector<std::vector<uint32_t>> order, cells;
  bool merged = false;
  // dsa_encode_split_sequential_batch with part_points >= 1 (`split`).  While the chunks run the handle has one entry per input, and
  // parts[input] holds the streams of its parts; flatten_parts then makes it one entry per STREAM: part_first[input] names an input's
  // slots (one for a refused input), part_info[stream] says which part it is, and order[] keeps perm once per cloud, in the slot
  // of its first part -- row_data serves every part its slice.
  // (lod_base_bits >= 1: `lod` of a part says which level it is, level_first_stream counted from the input's first slot until
  // flatten_parts; lod_info[stream] then answers dsa_encoded_lod_info, and lod_bits says the handle has levels)
  struct Part { std::vector<uint8_t> stream; dsa_part_info info; dsa_lod_info lod; };
  uint32_t lod_bits = 0;
  std::vector<dsa_lod_info> lod_info;
  bool split = false;
  std::vector<std::vector<Part>> parts;
  std::vector<uint32_t> part_first;
  std::vector<dsa_part_info> part_info;
  void keep_parts(size_t n) { split = true; parts.resize(n); }
  void keep_rows(int kind, size_t n) { rows_kind = kind; if (kind == ROWS_TRACKED) rows.resize(n); if (kind == ROWS_LINEAR || kind == ROWS_ORDERED) linear.resize(n); if (kind == ROWS_ORDERED) order.resize(n); }
  void keep_cells(size_t n) { merged = true; cells.resize(n); }
  // attributes of stream `mesh` with entry rows; entries of attribute a; their rows (null: entry e is row e)
  uint32_t row_attributes(size_t mesh) const { return rows_kind == ROWS_TRACKED ? (uint32_t)rows[mesh].size() : linear[mesh].first; }
  uint32_t row_entries(size_t mesh, uint32_t a) const { return rows_kind == ROWS_TRACKED ? (uint32_t)rows[mesh][a].size() : linear[mesh].second; }
  const uint32_t *row_data(size_t mesh, uint32_t a) const {
    if (rows_kind == ROWS_ORDERED && !part_info.empty()) return order[part_first[part_info[mesh].input]].data() + part_info[mesh].first_entry;
    return rows_kind == ROWS_TRACKED ? rows[mesh][a].data() : (rows_kind == ROWS_ORDERED ? order[mesh].data() : nullptr);
  }
  // mesh `from` of `part` into place `to`: stream, status, message and what it has of rows
  void take(size_t to, dsa_encoded &part, size_t from) {
    streams[to].swap(part.streams[from]); status[to] = part.status[from]; messages[to].swap(part.messages[from]);
    if (rows_kind == ROWS_TRACKED && from < part.rows.size()) rows[to].swap(part.rows[from]);
    if ((rows_kind == ROWS_LINEAR || rows_kind == ROWS_ORDERED) && from < part.linear.size()) linear[to] = part.linear[from];
    if (rows_kind == ROWS_ORDERED && from < part.order.size()) order[to].swap(part.order[from]);
    if (merged && from < part.cells.size()) cells[to].swap(part.cells[from]);
    if (split && from < part.parts.size()) parts[to].swap(part.parts[from]);
  }
  void flatten_parts() {
    const size_t n = streams.size();
    part_first.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
      if (status[i] == DSA_OK && parts[i].empty()) { status[i] = DSA_ERR_DEVICE; messages[i] = "the parts did not come back"; }
      part_first[i + 1] = part_first[i] + (status[i] == DSA_OK ? (uint32_t)parts[i].size() : 1u);
    }
    const size_t total = part_first[n];
    std::vector<std::vector<uint8_t>> s2(total);
    std::vector<int32_t> st2(total, DSA_OK);
    std::vector<std::string> m2(total);
    std::vector<std::pair<uint32_t, uint32_t>> l2(total);
    std::vector<std::vector<uint32_t>> o2(total), c2(merged ? total : 0);      // (part_cells: row_entries once per cloud, in the slot of its first part)
    dsa_part_info none;
    memset(&none, 0, sizeof(none));
    part_info.assign(total, none);
    dsa_lod_info no_level;
    memset(&no_level, 0, sizeof(no_level));
    lod_info.assign(total, no_level);
    for (size_t i = 0; i < n; ++i) {
      const size_t f = part_first[i];
      if (status[i] != DSA_OK) { st2[f] = status[i]; m2[f].swap(messages[i]); part_info[f].input = (uint32_t)i; part_info[f].parts = 1; continue; }
      o2[f].swap(order[i]);
      if (merged) c2[f].swap(cells[i]);
      for (size_t p = 0; p < parts[i].size(); ++p) {
        s2[f + p].swap(parts[i][p].stream); part_info[f + p] = parts[i][p].info; l2[f + p] = {linear[i].first, parts[i][p].info.num_points};
        lod_info[f + p] = parts[i][p].lod; lod_info[f + p].level_first_stream += (uint32_t)f;
      }
    }
    streams.swap(s2); status.swap(st2); messages.swap(m2); linear.swap(l2); order.swap(o2);
    if (merged) cells.swap(c2);
    parts.clear();
  }
};

// A call of an encode entry point.  The meshes in the widest form (a narrower array is widened once, enc_widen), the options in
// the widest struct of their kind: what a narrower entry point does not have stays empty / at its default, which every check passes.
// The grids of one mesh as a request carries them (dsa_mesh_grids copied, the attribute list's up to what a stream may hold):
// slot 0 the positions, 1 the first UV set, 2 + k attribute k of the list.  enc_stage_grids turns mode 2 into mode 1 with the
// group's grid before any chunk looks.
static_assert(sizeof(synth::Grid) == sizeof(dsa_quantization_grid) && sizeof(dsa_quantization_grid) == 32 && sizeof(dsa_mesh_grids) == 80, "dsa_quantization_grid is the host coder's Grid");
struct EncMeshGrids {
  synth::Grid slot[2 + synth::kMaxAttributes];
  uint32_t group = 0;
  const char *error = nullptr;             // what the struct alone says against itself
  EncMeshGrids() { memset(slot, 0, sizeof(slot)); }
};
static EncMeshGrids enc_take_grids(const dsa_mesh_grids &g, uint32_t num_attributes) {
  EncMeshGrids out;
  memcpy(&out.slot[0], &g.position, sizeof(synth::Grid));
  memcpy(&out.slot[1], &g.texcoord, sizeof(synth::Grid));
  for (uint32_t k = 0; k < num_attributes && k < synth::kMaxAttributes && g.attributes; ++k) memcpy(&out.slot[2 + k], &g.attributes[k], sizeof(synth::Grid));
  out.group = g.group;
  if (g.reserved != 0) out.error = "dsa_mesh_grids.reserved is not zero";
  return out;
}
struct EncRequest {
  uint32_t n = 0;
  const dsa_mesh_attr_input *meshes = nullptr;
  bool sequential = false;
  // dsa_encode_batch alone, kept from the time it had a mesh form of its own: a `generic` pointer whose generic_components lies
  // outside 1 .. 4 is dropped and the mesh coded without the attribute.  Every other Edgebreaker entry refuses such a mesh
  // ("generic attribute needs 1 - 4 components"), and so does every sequential one, dsa_encode_sequential_batch included.
  bool drop_generic_outside_1_4 = false;
  bool repair_scan = false;                // dsa_encode_repair_batch, topology = 1, the first pass: two faces turned against each other over the same vertices are refused too
  bool repair = false;                     // dsa_encode_repair_batch, topology = 1, the second pass: the meshes the first pass refused for their topology, on the repaired corner table
  bool corner_repair = false;              // dsa_encode_seam_repair_batch, corner_repair = 1: the second pass codes attributes given per corner over the repaired table (else it refuses them)
  bool weld = false;                       // dsa_encode_points_batch / dsa_weld_batch: `meshes` holds one row per point, every chunk welds its meshes first (enc_stage_weld)
  std::vector<synth::Welded> *weld_sink = nullptr;      // dsa_weld_batch: receives the weld of every mesh, nothing is coded
  const EncMeshGrids *grids = nullptr;     // dsa_encode_grid_batch / _sequential_batch: parallel to `meshes` (null: every attribute on its own bounds)
  const dsa_mesh_attribute_corners *att_corners = nullptr;      // dsa_encode_corner_attributes_batch: parallel to `meshes` (null: the listed attributes are per vertex)
  bool weld_attributes = false;            // ... weld_attributes = 1: the listed attributes are key sets of their own in the weld (dsa_encode_weld.h: 3 + L key sets)
  bool track_rows = false;                 // dsa_encode_rows_batch, track_rows = 1: the handle keeps the entry rows of every stream (dsa_encode_rows.h)
  bool point_order = false;                // dsa_encode_ordered_sequential_batch, point_order = 1: the points of every stream in Morton order (dsa_encode_order.h)
  bool merge_points = false;               // dsa_encode_merged_sequential_batch, merge_points = 1 (with point_order, point clouds): one point per cell of the position grid
  bool merged() const { return sequential && point_order && merge_points && !weld_sink; }
  uint32_t part_points = 0;                // dsa_encode_split_sequential_batch, part_points >= 1 (with point_order, point clouds, no merge): the sorted order in parts of at most so many points
  uint32_t part_cells = 0;                 // dsa_encode_cell_parts_sequential_batch, part_cells >= 1 (with point_order and merge_points, point clouds): the KEPT order in parts of at most so many points
  bool cell_parts() const { return sequential && point_order && merge_points && part_cells >= 1 && part_points == 0 && seq.geometry == 0 && !weld_sink; }
  bool split() const { return (sequential && point_order && !merge_points && part_points >= 1 && seq.geometry == 0 && !weld_sink) || cell_parts(); }
  uint32_t part_size() const { return cell_parts() ? part_cells : part_points; }      // N of either
  uint32_t lod_base_bits = 0;              // dsa_encode_lod_sequential_batch, lod_base_bits D >= 1 (with part_cells): the kept order by (level, kept), every level in parts
  bool lod() const { return cell_parts() && lod_base_bits >= 1; }
  uint32_t voxel_bits = 0, voxel_point = 0; // dsa_encode_voxel_sequential_batch (with merge_points): C >= 1: one point per cell of the grid with C bits per axis; DSA_VOXEL_POINT_*
  uint32_t voxel_shift() const { return merged() && seq.geometry == 0 && voxel_bits >= 1 && voxel_bits < (uint32_t)seq.base.position_bits ? (uint32_t)seq.base.position_bits - voxel_bits : 0u; }      // s = B - C
  bool centroids() const { return voxel_shift() != 0 && voxel_point == DSA_VOXEL_POINT_CENTROID; }      // (C = B: every rule keeps what the merge keeps, nothing more runs)
  bool nearest() const { return voxel_shift() != 0 && voxel_point == DSA_VOXEL_POINT_NEAREST; }
  uint32_t lod_levels() const { return lod() ? (uint32_t)seq.base.position_bits - voxel_shift() - lod_base_bits + 1u : 1u; }      // L = C - D + 1 (D <= C <= position_bits: enc_check_options)
  uint32_t mean_attributes = 0;            // dsa_encode_mean_sequential_batch (with merge_points): bit a: attribute a of the stream carries the mean of its cell (k_enc_mean_*)
  bool means() const { return merged() && seq.geometry == 0 && (mean_attributes != 0 || centroids()); }      // (centroids: the positions are a stream of the means pass)
  uint32_t vote_attributes = 0;            // dsa_encode_vote_sequential_batch (with merge_points): bit a: attribute a of the stream carries the most frequent value of its cell (k_enc_vote_*)
  bool votes() const { return merged() && seq.geometry == 0 && vote_attributes != 0; }
  bool mean_normals = false;               // dsa_encode_normal_mean_sequential_batch (with merge_points): the normals of a cloud that has them carry the mean normal of the cell (k_enc_normal_*)
  bool normal_means() const { return merged() && seq.geometry == 0 && mean_normals; }
  int rows_kind() const { return weld_sink ? dsa_encoded::ROWS_NONE : (sequential ? (point_order ? dsa_encoded::ROWS_ORDERED : dsa_encoded::ROWS_LINEAR) : (track_rows ? dsa_encoded::ROWS_TRACKED : dsa_encoded::ROWS_NONE)); }
  dsa_encode_level_options level{};        // Edgebreaker streams
  dsa_encode_sequential_options seq{};     // sequential streams
  const dsa_encode_options &base() const { return sequential ? seq.base : level.ex.base; }
  const dsa_mesh_attr_input &attr(size_t i) const { return meshes[i]; }
  const dsa_mesh_corner_input &corner(size_t i) const { return meshes[i].mesh; }
  const dsa_mesh_input &mesh(size_t i) const { return meshes[i].mesh.mesh; }
};
// The array of an entry point that takes dsa_mesh_input or dsa_mesh_corner_input in the request's form: no ids, no list (null: empty).
static inline void enc_wide(dsa_mesh_attr_input &w, const dsa_mesh_corner_input &m) { w.mesh = m; }
static inline void enc_wide(dsa_mesh_attr_input &w, const dsa_mesh_input &m) { w.mesh.mesh = m; }
template <class Mesh>
static std::vector<dsa_mesh_attr_input> enc_widen(const Mesh *meshes, uint32_t n) {
  std::vector<dsa_mesh_attr_input> wide(meshes ? n : 0);
  if (!wide.empty()) memset(wide.data(), 0, sizeof(dsa_mesh_attr_input) * wide.size());
  for (uint32_t i = 0; i < wide.size(); ++i) enc_wide(wide[i], meshes[i]);
  return wide;
}
// the options as the host coder takes them (a sequential stream has no connectivity, prediction or traversal options)
static synth::Options enc_synth_options(const EncRequest &rq) {
  const dsa_encode_options &od = rq.base();
  synth::Options opt;
  opt.pos_bits = od.position_bits; opt.uv_bits = od.texcoord_bits; opt.normal_bits = od.normal_bits;
  opt.force_scheme = od.symbol_scheme; opt.compression_level = od.compression_level;
  if (rq.sequential) return opt;
  opt.single_connectivity = od.single_connectivity; opt.pos_prediction = od.position_prediction; opt.uv_prediction = od.texcoord_prediction;
  opt.normal_prediction = rq.level.ex.normal_prediction; opt.traversal_method = rq.level.traversal_method;
  opt.repair_topology = rq.repair ? (rq.corner_repair ? 2 : 1) : 0;
  return opt;
}

static_assert(ORD_TILE == DSA_ENCODE_ORDER_TILE, "the header tells the sort's tile size");
struct EncCopy { uint64_t off, src_off; uint32_t bytes, pad; };      // a region filled from the lane's repair arena (enc_stage_uploads), not from host memory; the layout of dsa::PackItem
struct EncUpload { uint64_t off; const void *src; size_t bytes; bool narrow; };       // narrow: src is u32[bytes / 2], the staging copy keeps the low halves
// The arena, handed out in 256-byte aligned regions one behind the other.
struct EncArena {
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> *log = nullptr;      // (offset, bytes) of every region, for the host check of the layout
  uint64_t take(uint64_t bytes) { const uint64_t at = cur; cur = (cur + bytes + 255) & ~255ull; if (log) log->push_back({at, bytes}); return at; }
  uint64_t put(std::vector<EncUpload> &ups, const void *src, uint64_t bytes, bool narrow) { const uint64_t at = take(bytes); ups.push_back({at, src, (size_t)bytes, narrow}); return at; }
};
// A cell pass of the point-order stage (dsa_encode_order.h: the means, the votes, the mean normals) beside its typed records, one per chosen stream.
struct EncCellPass {
  std::vector<dsa::EncCellStreams> clouds;  // one per cloud, parallel to EncLayout::ord
  std::vector<uint32_t> stream;             // stream[k]: the stream of the pass's record k
  uint64_t clouds_at = 0, records_at = 0;   // both among the uploads
  uint32_t most = 0;                        // the most chosen streams a cloud of the chunk has: the y of the kernels' grid
  // the streams of a cloud of `na` attributes from stream s0 on that `mask` names (the positions only for the voxel rules, which
  // pass lowest = 0): record(stream) appends the typed record of each; then the cloud's own record
  template <class Append>
  void list(uint32_t mask, uint32_t s0, size_t na, Append &&record, uint32_t lowest = 1u) {
    dsa::EncCellStreams C{(uint32_t)stream.size(), 0u};
    for (uint32_t k = lowest; k < na && k < 32u; ++k) {
      if (!((mask >> k) & 1u)) continue;
      record(s0 + k); stream.push_back(s0 + k);
      ++C.count;
    }
    most = std::max(most, C.count);
    clouds.push_back(C);
  }
  template <class Record>
  void upload(const std::vector<Record> &records, EncArena &A, std::vector<EncUpload> &uploads) {
    if (records.empty()) return;
    clouds_at = A.put(uploads, clouds.data(), sizeof(dsa::EncCellStreams) * clouds.size(), false);
    records_at = A.put(uploads, records.data(), sizeof(Record) * records.size(), false);
  }
};
struct EncLayout {
  std::vector<dsa::EncStream> streams;
  std::vector<dsa::EncConn> conns;          // device connectivity: one per mesh (a mesh that failed the host's checks: F = 0, no arrays)
  std::vector<dsa::EncSeam> seams;          // device connectivity: one per (mesh, attribute given per corner)
  std::vector<dsa::EncSeqIdx> idx;          // sequential, compressed indices: one per mesh
  std::vector<dsa::EncRows> rows;           // EncRequest::track_rows: one per (mesh, attribute), in stream order
  std::vector<uint32_t> rows_of_stream;     // ... per stream its record in `rows` (DSA_INVALID: a context list); empty without track_rows
  std::vector<EncCopy> copies_a;            // phase A, a repaired table with corner ids: the ids of the coded faces, which k_enc_repair_ids left on the device
  std::vector<EncUpload> uploads_a, uploads;      // phase A: what the walks need (the faces, the corner ids; device connectivity only); the rest
  std::vector<uint32_t> first_stream;       // streams of mesh i: first_stream[i] .. first_stream[i + 1]
  uint64_t input_bytes = 0, total_bytes = 0;      // the uploads fill [0, input_bytes); the kernels' regions lie behind
  uint32_t max_rows = 0, maxf = 0, max_count = 0; // grid sizes: value rows / entries of a stream, faces of a mesh, index symbols of a mesh
  bool any_multi = false, any_crease = false, any_valence = false;      // streams predicted by method 2 / 4; by method 4; meshes coded with valence symbols
  bool any_grid = false;                    // streams on a grid that is not their own bounds (k_enc_grid_quantize)
  // EncRequest::point_order (dsa_encode_order.h): one record per mesh that passed its checks and the (cloud, tile) pairs of all of
  // them, both among the uploads at ord_at / ord_tiles_at
  std::vector<dsa::EncOrder> ord;
  std::vector<dsa::EncOrderTile> ord_tiles;
  uint64_t ord_at = 0, ord_tiles_at = 0;
  uint32_t ord_passes = 0;
  bool merge = false;                       // EncRequest::merge_points: the records say so, the streams read kept in place of perm
  std::vector<uint32_t> ord_of_mesh;        // merge or split: the record of mesh i of the chunk (DSA_INVALID: it has none)
  // EncRequest::split: a record per part of every cloud (the parts of a cloud side by side, part_of_mesh[i] its first) and the
  // (part, tile) pairs of all of them, both among the uploads
  bool split = false;
  bool cell_parts = false;                  // EncRequest::cell_parts: split and merge, a cloud's records are part SLOTS the device sizes (k_enc_part_cells)
  bool lod = false;                         // EncRequest::lod: cell_parts whose slots are the parts of the cloud's levels (k_enc_lod_*, then k_enc_part_cells)
  std::vector<dsa::EncPart> parts;
  std::vector<dsa::EncPartTile> part_tiles;
  std::vector<uint32_t> part_of_mesh;
  uint64_t parts_at = 0, part_tiles_at = 0;
  // EncRequest::means, EncRequest::votes: a cell pass each (EncCellPass above) with its typed records, one per masked / voted stream,
  // and what it accumulates in, one range of the arena that is zeroed on the stream in front of its kernels: the means' holds the
  // sums and counts, the votes' behind it tables, counts and values.  The vote records come back behind the stage: EncVote::full
  // (enc_vote_refusals).  EncRequest::normal_means: a third pass, a record per cloud that has normals, its range -- vector sums and
  // counts -- behind the votes'; a chunk without normals has no record, no range and no launch of it
  // EncRequest::nearest: a fourth pass, in front of the three (they write at the rows it picks), a record per cloud, its range -- the
  // best distance and row of every voxel -- behind the normals'.  EncRequest::centroids: the positions are the first record of the
  // means pass of every cloud, which then runs with mean_attributes = 0 too
  EncCellPass mean_pass, vote_pass, normal_pass, near_pass;
  uint64_t mean_zero_at = 0, mean_zero_bytes = 0, vote_zero_at = 0, vote_zero_bytes = 0, normal_zero_at = 0, normal_zero_bytes = 0, near_zero_at = 0, near_zero_bytes = 0;
  std::vector<dsa::EncVoxel> voxels;
  std::vector<dsa::EncMean> means;
  std::vector<dsa::EncVote> votes;
  std::vector<dsa::EncNormal> normals;
};

// ---- the point-order stage of a chunk whose layout has order records (dsa_encode_order.h has the kernels and their contracts): the
// one launch sequence, which enc_stage_attributes runs on the device and every host check of these kernels thread by thread.
//   launch(kernel, grid x, grid y, block, arguments...)   hipLaunchKernelGGL on the lane's stream; the thread-by-thread loop
//   zero(offset, bytes)                                   hipMemsetAsync on that stream; memset
//   after(name)                                           behind every group of kernels: the product asks for a launch error and, under
//                                                         DSA_ENC_TIMING, drains the stream and prints the lap `name` (nullptr: a group
//                                                         without a lap of its own, its time is part of the next lap).  False ends
//                                                         the stage, which then returns false.
// meshes: the chunk codes meshes (rank); gx_faces: blocks over the corners of its largest mesh with compressed indices (0: no mesh
// has any).  `streams`: the chunk's ns EncStream records where the kernels read and write them.
template <class Launch, class Zero, class After>
static inline bool enc_order_stage(Launch &&launch, Zero &&zero, After &&after, const EncLayout &L, bool meshes, uint32_t gx_faces,
                                   uint8_t *arena, dsa::EncStream *streams, uint32_t ns) {
  const uint32_t nc = (uint32_t)L.ord.size(), nt = (uint32_t)L.ord_tiles.size(), np = (uint32_t)L.parts.size(), npt = (uint32_t)L.part_tiles.size();
  const uint32_t nm = (uint32_t)L.means.size(), nv = (uint32_t)L.votes.size(), nn = (uint32_t)L.normals.size(), wave = (uint32_t)WAVE;
  if (nc == 0 || nt == 0) return true;
  dsa::EncOrder *clouds = (dsa::EncOrder *)(arena + L.ord_at);
  const dsa::EncOrderTile *tiles = (const dsa::EncOrderTile *)(arena + L.ord_tiles_at);
  dsa::EncPart *parts = (dsa::EncPart *)(arena + L.parts_at);
  const dsa::EncPartTile *part_tiles = (const dsa::EncPartTile *)(arena + L.part_tiles_at);
  const dsa::EncMean *means = (const dsa::EncMean *)(arena + L.mean_pass.records_at);
  dsa::EncVote *votes = (dsa::EncVote *)(arena + L.vote_pass.records_at);
  const dsa::EncNormal *normals = (const dsa::EncNormal *)(arena + L.normal_pass.records_at);
  const dsa::EncVoxel *voxels = (const dsa::EncVoxel *)(arena + L.near_pass.records_at);
  const uint32_t nx = (uint32_t)L.voxels.size();
  // a cell pass: its range zeroed, kernels(the clouds' records, grid y), its lap
  auto cell_pass = [&](const EncCellPass &P, uint64_t zero_at, uint64_t zero_bytes, const char *lap, auto &&kernels) -> bool {
    if (P.stream.empty()) return true;
    zero(zero_at, zero_bytes);
    if (P.most) kernels((const dsa::EncCellStreams *)(arena + P.clouds_at), P.most);
    return after(lap);
  };
  // the permutation of every cloud, behind the quantisers and in front of the gather
  launch(dsa::k_enc_order_keys, nt, 1u, 256u, arena, clouds, tiles, nt);
  for (uint32_t p = 0; p < L.ord_passes; ++p) {
    launch(dsa::k_enc_order_hist, nt, 1u, wave, arena, clouds, tiles, nt, p);
    launch(dsa::k_enc_order_scan, nc, 1u, wave, arena, clouds, nc);
    launch(dsa::k_enc_order_scatter, nt, 1u, wave, arena, clouds, tiles, nt, p);
  }
  if (meshes) launch(dsa::k_enc_order_rank, nt, 1u, 256u, arena, clouds, tiles, nt);
  if (meshes && gx_faces) launch(dsa::k_enc_order_faces, gx_faces, nc, 256u, arena, clouds, nc);
  if (!after("point order")) return false;
  if (L.merge) {               // merge_points: one point per cell, behind the sort; nv of the cloud's streams falls to the cells it has
    launch(dsa::k_enc_merge_heads, nt, 1u, wave, arena, clouds, tiles, nt);
    launch(dsa::k_enc_merge_scan<dsa::EncStream>, nc, 1u, wave, arena, clouds, nc, streams, ns);
    launch(dsa::k_enc_merge_compact, nt, 1u, wave, arena, clouds, tiles, nt);
    if (!after("point merge")) return false;
  }
  // voxel_point = nearest: kept[j] becomes the row of voxel j nearest its centre, in front of the three passes below, which write at kept[j]
  if (!cell_pass(L.near_pass, L.near_zero_at, L.near_zero_bytes, "voxel nearest", [&](const dsa::EncCellStreams *xclouds, uint32_t most) {
        launch(dsa::k_enc_voxel_near, nt, most, wave, arena, clouds, tiles, nt, xclouds, voxels, nx, 0u);
        launch(dsa::k_enc_voxel_near, nt, most, wave, arena, clouds, tiles, nt, xclouds, voxels, nx, 1u);
        launch(dsa::k_enc_voxel_pick, nt, most, 256u, arena, clouds, tiles, nt, xclouds, voxels, nx);
      })) return false;
  // mean_attributes: the mean of the cell into vals at every kept row, in front of everything that reads vals or turns row_entries into lod order
  // (voxel_point = centroid: the positions among them -- behind everything that reads the positions of other rows, the nearest pass, and
  // in front of the levels and the boxes, which read keys and boxes from vals at the kept rows)
  if (!cell_pass(L.mean_pass, L.mean_zero_at, L.mean_zero_bytes, "cell means", [&](const dsa::EncCellStreams *mclouds, uint32_t most) {
        launch(dsa::k_enc_mean_sum, nt, most, wave, arena, clouds, tiles, nt, mclouds, means, nm);
        launch(dsa::k_enc_mean_store, nt, most, 256u, arena, clouds, tiles, nt, mclouds, means, nm);
      })) return false;
  // vote_attributes: the most frequent tuple of the cell into vals at every kept row, beside the means (other streams), in front of the same readers
  if (!cell_pass(L.vote_pass, L.vote_zero_at, L.vote_zero_bytes, "cell votes", [&](const dsa::EncCellStreams *vclouds, uint32_t most) {
        launch(dsa::k_enc_vote_count, nt, most, wave, arena, clouds, tiles, nt, vclouds, votes, nv);
        launch(dsa::k_enc_vote_best, nt, most, 256u, arena, clouds, tiles, nt, vclouds, (const dsa::EncVote *)votes, nv, 0u);
        launch(dsa::k_enc_vote_best, nt, most, 256u, arena, clouds, tiles, nt, vclouds, (const dsa::EncVote *)votes, nv, 1u);
        launch(dsa::k_enc_vote_store, nt, most, 256u, arena, clouds, tiles, nt, vclouds, (const dsa::EncVote *)votes, nv);
      })) return false;
  // mean_normals: the mean normal of the cell into the normals' codes at every kept row, beside the two above (another stream), in front of the same readers
  if (!cell_pass(L.normal_pass, L.normal_zero_at, L.normal_zero_bytes, "cell normals", [&](const dsa::EncCellStreams *nclouds, uint32_t most) {
        launch(dsa::k_enc_normal_sum, nt, most, wave, arena, clouds, tiles, nt, nclouds, normals, nn);
        launch(dsa::k_enc_normal_store, nt, most, 256u, arena, clouds, tiles, nt, nclouds, normals, nn);
      })) return false;
  if (L.lod && np) {           // lod_base_bits: the kept order by (level, kept); the slot sizer below cuts every level into its parts
    launch(dsa::k_enc_lod_levels, nt, 1u, wave, arena, clouds, tiles, nt);
    launch(dsa::k_enc_lod_scan, nc, 1u, wave, arena, clouds, nc);
    launch(dsa::k_enc_lod_scatter, nt, 1u, wave, arena, clouds, tiles, nt);
    launch(dsa::k_enc_lod_cells, nt, 1u, 256u, arena, clouds, tiles, nt);
  }
  if (L.cell_parts) {          // part_cells: k_enc_merge_scan has left m (k_enc_lod_scan the points of every level), the sizes of the part slots follow from it on the device
    if (np) launch(dsa::k_enc_part_cells<dsa::EncStream>, (np + wave - 1u) / wave, 1u, wave, arena, clouds, nc, parts, np, streams, ns);
    if (!after(L.lod ? "levels" : nullptr)) return false;
  }
  if (L.split) {               // part_points: the box of every part's position integers, behind the sort (the parts' streams read their slices of it as they are)
    if (np && npt) launch(dsa::k_enc_part_bounds, npt, 1u, wave, arena, clouds, nc, parts, np, part_tiles, npt);
    if (!after("part boxes")) return false;
  }
  return true;
}

static inline bool enc_multi_scheme(const synth::PortableAttr &a) { return a.seq_type != 3 && (a.prediction == 2 || a.prediction == 4); }
// the attribute reads the mesh's topology (TexCoordsPortable, GeometricNormal, the multi-parallelogram schemes)
static inline bool enc_topo_scheme(const synth::PortableAttr &a) { return (a.seq_type == 2 && a.prediction == 5) || (a.seq_type == 3 && a.prediction == 6) || enc_multi_scheme(a); }

struct EncChunk {
  const EncRequest &rq;
  uint32_t base, n, batch_n;               // meshes base .. base + n of the request's batch_n
  synth::Options opt;
  bool host_conn = false, host_plan = false, want_pd = false;     // connectivity / symbol plans by the host; the prediction-degree order beside the depth-first one
  std::unique_ptr<dsa_encoded> E;           // per mesh: status, message and in the end the stream
  std::vector<synth::MeshIn> ins;
  std::vector<synth::MeshPlan> plans;       // (a sequential stream's: the attributes alone)
  std::vector<std::vector<synth::ExtraAttr>> extras;
  std::vector<std::vector<uint32_t>> extra_cap;                   // per mesh and attribute of the plan: hist_cap of an integer extra, else 0
  // host connectivity: entry -> vertex and operand entries in depth-first and in prediction-degree order; per attribute given per
  // corner its own entry -> value row, when it is seamed its own operands, with prediction 5 / 6 its table's opposites
  std::vector<std::vector<uint32_t>> e2v, e2v_pd;
  std::vector<std::vector<int32_t>> ops, ops_pd;
  std::vector<std::vector<std::vector<uint32_t>>> att_e2v, att_opp;
  std::vector<std::vector<std::vector<int32_t>>> att_ops;
  // a repaired table (EncRequest::repair), per mesh: the value row of every corner (both paths: what the schemes that read the
  // positions index them by); device connectivity: the table the repair kernels left, degenerate faces and isolated vertices
  // counted out (ct.c2v, ct.opp, ct.row), which the layout uploads in place of the caller's faces
  std::vector<std::vector<uint32_t>> c2row;
  std::vector<synth::CornerTable> rep;
  // ... and with corner ids (EncRequest::corner_repair), per mesh and attribute of the plan: where in the lane's repair arena the ids
  // of the coded faces lie, in the width ids_narrow says (kNoIds: the attribute has no ids)
  static constexpr uint64_t kNoIds = ~0ull;
  std::vector<std::vector<uint64_t>> rep_ids;
  std::vector<dsa::EncRepairRows> rep_rows;
  // a weld request (EncRequest::weld): the weld of every mesh, in buffers of the chunk's own, and the welded meshes in the form
  // every stage behind enc_stage_weld reads (mesh(i) / corner(i) / attr(i) point here instead of at the caller's arrays)
  std::vector<synth::Welded> weld;
  std::vector<std::vector<dsa_attribute_input>> weld_attrs;
  std::vector<std::vector<dsa_attribute_corners>> weld_corners;      // weld_attributes: the ids of the listed attributes welded alone (empty: none has two rows at a vertex)
  std::vector<dsa_mesh_attr_input> welded;
  EncLayout L;
  std::vector<std::pair<uint64_t, uint64_t>> *region_log = nullptr;
  // the device's side and what comes back from it
  uint8_t *arena = nullptr;
  dsa::EncStream *d_streams = nullptr;
  dsa::EncConn *d_conns = nullptr;
  dsa::EncSeam *d_seams = nullptr;
  std::vector<int> stream_mesh;
  std::vector<synth::SymbolPlan> splans;
  std::vector<std::vector<uint8_t>> rans, bits, flag_bits, crease;      // per stream; crease[4 s + j]: list j of stream s
  std::vector<std::vector<uint32_t>> entry_rows;                        // per stream (EncRequest::track_rows)
  std::vector<std::vector<uint32_t>> row_cells;                         // per stream, a cloud's first alone (EncRequest::merge_points): row_entries
  std::vector<uint32_t> parts;                                          // EncRequest::split, per mesh: how many parts it is coded in (enc_check_sequential_mesh)
  std::vector<std::vector<dsa::EncPart>> part_boxes;                    // ... per stream, a cloud's first alone: the records of its parts as k_enc_part_bounds left them
  uint32_t num_parts(uint32_t i) const { return parts.empty() ? 1u : parts[i]; }        // (part_cells: the slots laid out, ceil(n / part_cells))
  // part_cells: the parts the device made of cloud i -- the slots in front whose records came back with points -- and their points, m
  uint32_t live_parts(uint32_t i, uint32_t *points = nullptr) const {
    const uint32_t s0 = L.first_stream[i], na = (uint32_t)plans[i].atts.size();
    uint32_t live = 0, m = 0;
    for (uint32_t p = 0, np = num_parts(i); p < np && L.streams[s0 + p * na].nv != 0u; ++p) { ++live; m += L.streams[s0 + p * na].nv; }
    if (points) *points = m;
    return live;
  }

  EncChunk(const EncRequest &r, uint32_t b, uint32_t cnt, uint32_t bn) : rq(r), base(b), n(cnt), batch_n(bn), opt(enc_synth_options(r)), E(new (std::nothrow) dsa_encoded()), ins(cnt), plans(cnt), extras(cnt), extra_cap(cnt) {
    if (!E) return;                        // (the chunk function answers)
    E->streams.resize(n); E->status.assign(n, DSA_OK); E->messages.resize(n);
    E->keep_rows(r.rows_kind(), n);
    if (r.merged()) E->keep_cells(n);
    if (r.split()) { E->keep_parts(n); parts.assign(n, 1u); }
  }
  const dsa_mesh_attr_input &attr(uint32_t i) const { return welded.empty() ? rq.attr(base + i) : welded[i]; }
  const dsa_mesh_corner_input &corner(uint32_t i) const { return attr(i).mesh; }
  const dsa_mesh_input &mesh(uint32_t i) const { return attr(i).mesh.mesh; }
  // the row ids of the listed attributes of mesh i (null: all per vertex): the caller's, or after a weld the weld's
  const dsa_attribute_corners *att_corners(uint32_t i) const {
    if (!welded.empty()) return i < weld_corners.size() && !weld_corners[i].empty() ? weld_corners[i].data() : nullptr;
    return rq.att_corners ? rq.att_corners[base + i].attributes : nullptr;
  }
  // vertices and faces of mesh i as the connectivity kernels and the streams see them
  uint32_t coded_vertices(uint32_t i) const { return !rep.empty() ? rep[i].nv() : (plans[i].coded_vertices >= 0 ? (uint32_t)plans[i].coded_vertices : mesh(i).num_vertices); }
  uint32_t coded_faces(uint32_t i) const { return !rep.empty() ? rep[i].nf() : (plans[i].coded_faces >= 0 ? (uint32_t)plans[i].coded_faces : mesh(i).num_faces); }
  bool good(uint32_t i) const { return E->status[i] == DSA_OK; }
  void refuse(uint32_t i, dsa_status st, const std::string &why) { E->status[i] = st; E->messages[i] = why; }
  // valence symbols per mesh: asked for, or by the reference's rule (speed < 5 and not a tiny mesh)
  bool valence_of(uint32_t i) const { const int32_t m = rq.level.ex.edgebreaker_method; return !rq.sequential && (m == 2 || (m == -1 && opt.compression_level > 5 && mesh(i).num_faces >= 1000)); }
  // MultiParallelogram per mesh: the method asked for, or by the reference's rule (speed < 2 and at least 40 points)
  int32_t multi_of(uint32_t i) const { const int32_t m = rq.level.multi_parallelogram; return m == -1 ? ((opt.compression_level >= 9 && mesh(i).num_vertices >= 40) ? 4 : 0) : m; }
  // value rows of an attribute of mesh i: its ids' row count when it is given per corner
  uint32_t rows_of(uint32_t i, const synth::PortableAttr &a) const {
    if (!a.corner_value) return mesh(i).num_vertices;
    return a.extra_values ? a.extra_rows : (a.att_type == 1 ? corner(i).num_normals : corner(i).num_texcoords);
  }
  bool ids_narrow(uint32_t i, const synth::PortableAttr &a) const { return rows_of(i, a) <= 65536; }
  // the decoder of attribute k takes the prediction-degree order (MeshPlan::uses_pd; for an attribute given per corner on the
  // device path: unless it turns out seamed -- k_enc_pd_corner_streams, k_enc_seam_topo)
  bool uses_pd(uint32_t i, size_t k) const { return want_pd && (host_conn ? plans[i].uses_pd(k) : (opt.traversal_method == 2 || opt.single_connectivity != 0 || k == 0)); }
  uint32_t hist_cap_of(uint32_t i, size_t k) const { return extra_cap[i][k]; }      // (0: by the attribute's bits)
};

// The attribute list of a mesh as the host coder takes it (`ex` keeps them alive beside `in`); what the C structs
// alone can say against them -- a reserved word -- is answered here, the rest by synth::extras_error.  "" when they can be written.
static std::string enc_take_extras(const dsa_mesh_attr_input &am, std::vector<synth::ExtraAttr> &ex, synth::MeshIn &in, const dsa_attribute_corners *corners = nullptr) {
  char buf[96];
  if (am.reserved != 0) return "dsa_mesh_attr_input.reserved is not zero";
  if (am.num_attributes && !am.attributes) return "attributes: the list is missing";
  ex.resize(am.num_attributes);
  for (uint32_t k = 0; k < am.num_attributes; ++k) {
    const dsa_attribute_input &x = am.attributes[k];
    for (int r = 0; r < 2; ++r)
      if (x.reserved[r] != 0) { snprintf(buf, sizeof(buf), "attribute %u: reserved[%d] is not zero", k, r); return buf; }
    ex[k].att_type = x.attribute_type; ex[k].data_type = x.data_type; ex[k].nc = x.num_components; ex[k].normalized = x.normalized;
    ex[k].unique_id = x.unique_id; ex[k].bits = x.quantization_bits; ex[k].values = x.values;
    if (!corners) continue;
    if (corners[k].reserved != 0) { snprintf(buf, sizeof(buf), "attribute %u: dsa_attribute_corners.reserved is not zero", k); return buf; }
    if (corners[k].corners) { ex[k].corners = corners[k].corners; ex[k].rows = corners[k].num_rows; }
  }
  in.extras = ex.data(); in.num_extras = am.num_attributes;
  return synth::extras_error(in);
}
// The grids of mesh i (null: none) against its attributes, and into `in` / `ex` for the plan; "" when they can be used.  Mode 2
// has become mode 1 by now (enc_stage_grids).
static std::string enc_take_mesh_grids(const EncMeshGrids *g, std::vector<synth::ExtraAttr> &ex, synth::MeshIn &in) {
  if (!g) return "";
  if (g->error) return g->error;
  std::string why = synth::grid_error(g->slot[0], 3, true, "positions");
  if (why.empty()) why = in.uvs ? synth::grid_error(g->slot[1], 2, true, "texcoords") : synth::grid_error_absent(g->slot[1], "texcoords");
  for (uint32_t k = 0; k < in.num_extras && k < synth::kMaxAttributes && why.empty(); ++k)
    why = synth::grid_error(g->slot[2 + k], (int)ex[k].nc, ex[k].data_type == 9, synth::grid_slot_name(ex[k].att_type, (int)k));
  if (!why.empty()) return why;
  in.pos_grid = &g->slot[0];
  if (in.uvs) in.uv_grid = &g->slot[1];
  for (uint32_t k = 0; k < in.num_extras && k < synth::kMaxAttributes; ++k) ex[k].grid = &g->slot[2 + k];
  return "";
}
// hist_cap of an integer extra: one-byte types by their range, wider ones by the values present (a pass over the values by the
// host thread that checks the mesh's indices anyway): zig-zagged wrapped corrections lie in 0 .. max - min + 1
static uint32_t enc_extra_hist_cap(const synth::PortableAttr &a, uint32_t rows) {
  if (synth::data_type_size(a.data_type) == 1) return (1u << 8) + 2u;
  const size_t total = (size_t)rows * (size_t)a.nc;
  int32_t lo = 0, hi = 0;
  if (a.data_type == 3) { const int16_t *p = (const int16_t *)a.extra_values; int16_t l = p[0], h = p[0]; for (size_t k = 1; k < total; ++k) { l = p[k] < l ? p[k] : l; h = p[k] > h ? p[k] : h; } lo = l; hi = h; }
  else if (a.data_type == 4) { const uint16_t *p = (const uint16_t *)a.extra_values; uint16_t l = p[0], h = p[0]; for (size_t k = 1; k < total; ++k) { l = p[k] < l ? p[k] : l; h = p[k] > h ? p[k] : h; } lo = l; hi = h; }
  else { const int32_t *p = (const int32_t *)a.extra_values; lo = hi = p[0]; for (size_t k = 1; k < total; ++k) { lo = p[k] < lo ? p[k] : lo; hi = p[k] > hi ? p[k] : hi; } }     // (uint32 by reinterpretation)
  return dsa::enc_integer_hist_cap(lo, hi);
}
// the bounds of the integer extras' values of mesh i, once its plan has said which attributes there are
static void enc_extra_caps(EncChunk &ck, uint32_t i) {
  const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
  ck.extra_cap[i].assign(atts.size(), 0);
  for (size_t k = 0; k < atts.size(); ++k)
    if (atts[k].extra_values && atts[k].seq_type == 1) ck.extra_cap[i][k] = enc_extra_hist_cap(atts[k], ck.rows_of(i, atts[k]));
}

// ---- a weld request, mesh i: what the weld itself indexes by is checked here, before anything reads through the faces (the
// rest of the mesh is the coder's to judge, on the welded form).  The segments of the vertex key into `key`; false: refused.
static bool enc_weld_check(EncChunk &ck, uint32_t i, std::vector<synth::WeldSeg> &key, std::vector<synth::WeldSeg> *listed = nullptr) {
  const dsa_mesh_attr_input &am = ck.rq.attr(ck.base + i);
  const dsa_mesh_input &m = am.mesh.mesh;
  if (am.mesh.normal_corners || am.mesh.texcoord_corners) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "per-point input takes no corner ids (normal_corners / texcoord_corners must be NULL)"); return false; }
  if (ck.rq.att_corners) {
    const dsa_mesh_attribute_corners &mc = ck.rq.att_corners[ck.base + i];
    if (mc.reserved[0] != 0 || mc.reserved[1] != 0) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "dsa_mesh_attribute_corners.reserved is not zero"); return false; }
    for (uint32_t k = 0; mc.attributes && k < am.num_attributes; ++k)
      if (mc.attributes[k].corners) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "per-point input takes no corner ids (the corners of attribute " + std::to_string(k) + " must be NULL)"); return false; }
  }
  if (m.generic && (m.generic_components < 1 || m.generic_components > 4)) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "generic attribute needs 1 - 4 components"); return false; }
  synth::MeshIn in{m.positions, m.num_vertices, m.faces, m.num_faces, m.normals, m.texcoords, m.generic};
  std::vector<synth::ExtraAttr> ex;
  const std::string why = enc_take_extras(am, ex, in);
  if (!why.empty()) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, why); return false; }
  if ((m.num_vertices && !m.positions) || (m.num_faces && !m.faces)) { ck.refuse(i, DSA_ERR_INVALID_DATA, "mesh needs positions and faces"); return false; }
  for (size_t k = 0, nk = (size_t)m.num_faces * 3; k < nk; ++k)
    if (m.faces[k] >= m.num_vertices) { ck.refuse(i, DSA_ERR_INVALID_DATA, "face index out of range"); return false; }
  key = synth::weld_vertex_key(in, m.generic ? m.generic_components : 0, ck.rq.weld_attributes, listed);
  return true;
}
// the welded mesh i in the C structs, pointed at ck.weld[i] (a refused mesh: an empty one, which nothing reads)
static void enc_weld_view(EncChunk &ck, uint32_t i) {
  dsa_mesh_attr_input &out = ck.welded[i];
  memset(&out, 0, sizeof(out));
  if (!ck.good(i)) return;
  const dsa_mesh_attr_input &am = ck.rq.attr(ck.base + i);
  const synth::Welded &w = ck.weld[i];
  dsa_mesh_input &m = out.mesh.mesh;
  size_t g = 0;
  m.num_vertices = w.vertex.count; m.num_faces = w.F;
  m.positions = (const float *)w.vertex_rows[g++].data();
  m.faces = w.faces.data();
  if (am.mesh.mesh.generic) { m.generic = w.vertex_rows[g++].data(); m.generic_components = am.mesh.mesh.generic_components; }
  ck.weld_attrs[i].assign(am.attributes, am.attributes + am.num_attributes);
  // (the listed attributes welded alone are the first w.listed.size() of the list; the rest stayed in the vertex key)
  bool any_ids = false;
  for (const synth::Welded::Listed &l : w.listed) any_ids = any_ids || !l.per_vertex;
  if (any_ids) { dsa_attribute_corners none; memset(&none, 0, sizeof(none)); ck.weld_corners[i].assign(am.num_attributes, none); }
  for (uint32_t k = 0; k < am.num_attributes; ++k) {
    if (k >= w.listed.size()) { ck.weld_attrs[i][k].values = w.vertex_rows[g++].data(); continue; }
    const synth::Welded::Listed &l = w.listed[k];
    ck.weld_attrs[i][k].values = l.rows.data();
    if (!l.per_vertex) { ck.weld_corners[i][k].corners = l.corners.data(); ck.weld_corners[i][k].num_rows = l.keys.count; }
  }
  out.attributes = ck.weld_attrs[i].data(); out.num_attributes = am.num_attributes;
  if (am.mesh.mesh.normals) {
    m.normals = (const float *)w.normal_rows.data();
    if (!w.normals_per_vertex) { out.mesh.normal_corners = w.normal_corners.data(); out.mesh.num_normals = w.normal.count; }
  }
  if (am.mesh.mesh.texcoords) {
    m.texcoords = (const float *)w.texcoord_rows.data();
    if (!w.texcoords_per_vertex) { out.mesh.texcoord_corners = w.texcoord_corners.data(); out.mesh.num_texcoords = w.texcoord.count; }
  }
}

// ---- Edgebreaker streams, host phase 1 for mesh i: the checks of everything the kernels index by, the attribute descriptors, and
// with host connectivity the connectivity, traversal orders and entry maps
static void enc_plan_mesh(EncChunk &ck, uint32_t i) {
  const dsa_mesh_input &m = ck.mesh(i);
  const synth::Options &opt = ck.opt;
  synth::MeshIn &in = ck.ins[i];
  in.pos = m.positions; in.nv = m.num_vertices; in.faces = m.faces; in.nf = m.num_faces; in.normals = m.normals; in.uvs = m.texcoords;
  in.generic = m.generic;
  if (m.generic && (m.generic_components < 1 || m.generic_components > 4)) {
    if (!ck.rq.drop_generic_outside_1_4) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "generic attribute needs 1 - 4 components");
    in.generic = nullptr;
  }
  const dsa_mesh_corner_input &cm = ck.corner(i);
  if ((cm.normal_corners && !m.normals) || (cm.texcoord_corners && !m.texcoords)) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "corner ids without their values");
  in.normal_corners = cm.normal_corners; in.nn = cm.num_normals;
  in.uv_corners = cm.texcoord_corners; in.nu = cm.num_texcoords;
  std::string why;
  if (ck.welded.empty() && ck.rq.att_corners && (ck.rq.att_corners[ck.base + i].reserved[0] != 0 || ck.rq.att_corners[ck.base + i].reserved[1] != 0)) why = "dsa_mesh_attribute_corners.reserved is not zero";
  if (why.empty()) why = enc_take_extras(ck.attr(i), ck.extras[i], in, ck.att_corners(i));
  if (why.empty()) why = enc_take_mesh_grids(ck.rq.grids ? &ck.rq.grids[ck.base + i] : nullptr, ck.extras[i], in);
  if (!why.empty()) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, why);
  const bool listed_ids = synth::extras_have_corners(in);
  // (every mesh of a repair request is one whose topology the first pass refused)
  if (ck.rq.repair && !ck.rq.corner_repair && (in.normal_corners || in.uv_corners || listed_ids))
    return ck.refuse(i, DSA_ERR_NOT_IMPLEMENTED, "attributes given per corner (normal_corners / texcoord_corners) over a mesh whose topology needs repair are not implemented");
  try {
    synth::check(m.positions && m.faces && m.num_vertices >= 3 && m.num_faces >= 1, "mesh needs positions and faces");
    for (size_t k = 0; k < (size_t)m.num_faces * 3; ++k) synth::check(m.faces[k] < m.num_vertices, "face index out of range");
    if (in.normal_corners) for (size_t k = 0; k < (size_t)m.num_faces * 3; ++k) synth::check(in.normal_corners[k] < in.nn, "normal id out of range");
    if (in.uv_corners) for (size_t k = 0; k < (size_t)m.num_faces * 3; ++k) synth::check(in.uv_corners[k] < in.nu, "texture coordinate id out of range");
    if (listed_ids) { const std::string bad = synth::extras_id_error(in); synth::check(bad.empty(), bad.c_str()); }
    synth::check(ck.host_conn || (uint64_t)m.num_faces * 3 <= (uint64_t)dsa::EC_CORNER_MASK, "mesh too large for the device connectivity coder");
    synth::Options mo = opt;                                   // (the components of the generic attribute are the mesh's own)
    mo.generic_components = in.generic ? (int32_t)m.generic_components : 1;
    mo.predictive_connectivity = ck.valence_of(i) ? 2 : 0;
    if (const int32_t mp = ck.multi_of(i)) {                   // in place of Parallelogram (plan_attributes: the generic attribute and the extras follow the positions to method 4)
      if (opt.pos_prediction == 1) mo.pos_prediction = mp;
      if (opt.uv_prediction == 1) mo.uv_prediction = mp;
    }
    synth::MeshPlan &pl = ck.plans[i];
    if (!ck.host_conn) {                                       // the rest of the plan comes from the device
      synth::check(!((in.normal_corners || in.uv_corners || listed_ids) && opt.single_connectivity), "attributes given per corner need a connectivity of their own (single_connectivity = 0)");
      synth::check(!(in.normal_corners || in.uv_corners || listed_ids) || 24ull * m.num_faces + 16u < (1ull << 32), "mesh too large for the device connectivity coder");
      synth::plan_attributes(in, mo, pl);
      enc_extra_caps(ck, i);
      return;
    }
    synth::plan_mesh(in, mo, pl);
    if (ck.rq.repair_scan)                                     // (k_enc_repair_scan on the device path)
      for (uint32_t c = 0; c < pl.ct.nc(); ++c) synth::check(pl.ct.opp[c] == synth::kInvalid || pl.ct.c2v[pl.ct.opp[c]] != pl.ct.c2v[c], dsa::enc_conn_message(dsa::ENC_NONMANIFOLD_EDGE));
    enc_extra_caps(ck, i);
    dsa::entry_maps(pl.ct, pl.seq, nullptr, ck.e2v[i], &ck.ops[i]);
    if (ck.want_pd) dsa::entry_maps(pl.ct, pl.seq_pd, nullptr, ck.e2v_pd[i], &ck.ops_pd[i]);
    if (!pl.ct.row.empty()) {                                  // a repaired table: an entry reads the row of its vertex, the position of a corner is its row's
      for (uint32_t &v : ck.e2v[i]) v = pl.ct.row[v];
      if (ck.want_pd) for (uint32_t &v : ck.e2v_pd[i]) v = pl.ct.row[v];
      ck.c2row[i].resize(pl.ct.nc());
      for (uint32_t c = 0; c < pl.ct.nc(); ++c) ck.c2row[i][c] = pl.ct.row[pl.ct.c2v[c]];
    }
    ck.att_e2v[i].assign(pl.atts.size(), {}); ck.att_ops[i].assign(pl.atts.size(), {}); ck.att_opp[i].assign(pl.atts.size(), {});
    for (size_t k = 1; k < pl.atts.size(); ++k) {
      const uint32_t *ids = pl.atts[k].corner_value;
      if (!ids) continue;
      if (pl.seamed(k)) dsa::entry_maps(pl.conns[k], pl.seq_att[k], ids, ck.att_e2v[i][k], &ck.att_ops[i][k]);
      else dsa::entry_maps(pl.ct, pl.uses_pd(k) ? pl.seq_pd : pl.seq, ids, ck.att_e2v[i][k], nullptr);      // (the positions' operands)
      if (!pl.seamed(k) || !enc_topo_scheme(pl.atts[k])) continue;
      std::vector<uint32_t> &o = ck.att_opp[i][k];
      o.resize(pl.ct.nc());
      for (uint32_t c = 0; c < pl.ct.nc(); ++c) o[c] = pl.conns[k].opposite(c);
    }
  } catch (const std::exception &e) { ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
}
// the chunk's switches and the vectors enc_plan_mesh fills (DSA_ENC_HOST_CONN / DSA_ENC_HOST_PLAN as the caller read them)
static void enc_begin_plans(EncChunk &ck, bool host_conn, bool host_plan) {
  ck.host_conn = host_conn; ck.host_plan = host_plan; ck.want_pd = ck.opt.traversal_method != 0;
  if (ck.rq.repair) ck.c2row.resize(ck.n);
  if (!host_conn) return;
  ck.e2v.resize(ck.n); ck.ops.resize(ck.n); ck.att_e2v.resize(ck.n); ck.att_ops.resize(ck.n); ck.att_opp.resize(ck.n);
  if (ck.want_pd) { ck.e2v_pd.resize(ck.n); ck.ops_pd.resize(ck.n); }
}

// ---- sequential streams, the host's checks of mesh i (everything the kernels index by) and its attribute descriptors
static void enc_check_sequential_mesh(EncChunk &ck, uint32_t i) {
  const dsa_mesh_input &m = ck.mesh(i);
  const bool is_mesh = ck.rq.seq.geometry == 1, compressed = is_mesh && ck.rq.seq.compress_connectivity == 1;
  if (!m.positions || m.num_vertices == 0) return ck.refuse(i, DSA_ERR_INVALID_DATA, "positions are missing");
  if (!is_mesh && m.num_faces != 0) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "a point cloud has no faces (geometry = 0, num_faces != 0)");
  if (is_mesh && (m.num_faces == 0 || !m.faces)) return ck.refuse(i, DSA_ERR_INVALID_DATA, "a mesh needs faces");
  if (m.generic && (m.generic_components < 1 || m.generic_components > 4)) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "generic attribute needs 1 - 4 components");
  if (ck.corner(i).normal_corners || ck.corner(i).texcoord_corners)
    return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "corner ids with a sequential stream: it has one value per point (normal_corners / texcoord_corners must be NULL)");
  // (what the 32-bit sizes of a stream's regions hold: 4 bytes per component and symbol, and a margin)
  if (m.num_vertices > (1u << 28) || (compressed && m.num_faces > (1u << 28))) return ck.refuse(i, DSA_ERR_INVALID_DATA, "mesh too large for the device coder");
  if (is_mesh) {
    uint32_t top = 0;
    for (size_t k = 0, nk = (size_t)m.num_faces * 3; k < nk; ++k) top = m.faces[k] > top ? m.faces[k] : top;
    if (top >= m.num_vertices) return ck.refuse(i, DSA_ERR_INVALID_DATA, "face index out of range");
  }
  synth::MeshIn &in = ck.ins[i];
  in.pos = m.positions; in.nv = m.num_vertices; in.faces = is_mesh ? m.faces : nullptr; in.nf = is_mesh ? m.num_faces : 0;
  in.normals = m.normals; in.uvs = m.texcoords; in.generic = m.generic;
  synth::Options mo = ck.opt;
  mo.generic_components = m.generic ? (int32_t)m.generic_components : 1;
  std::string why = enc_take_extras(ck.attr(i), ck.extras[i], in);
  if (why.empty()) why = enc_take_mesh_grids(ck.rq.grids ? &ck.rq.grids[ck.base + i] : nullptr, ck.extras[i], in);
  if (!why.empty()) return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, why);
  synth::plan_sequential_attributes(in, mo, ck.plans[i].atts);
  enc_extra_caps(ck, i);
  if (ck.rq.means()) {       // mean_attributes: every set bit names an attribute of this cloud's stream that can carry a mean
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    char buf[240];
    for (uint32_t a = 0; a < 32u; ++a) {
      if (!((ck.rq.mean_attributes >> a) & 1u)) continue;
      if (a >= atts.size()) snprintf(buf, sizeof(buf), "mean_attributes 0x%x: bit %u names attribute %u of the stream, which has %zu attributes", ck.rq.mean_attributes, a, a, atts.size());
      else if (a == 0) snprintf(buf, sizeof(buf), "mean_attributes 0x%x: bit 0 names attribute 0, the positions: they are equal inside a cell and are never averaged", ck.rq.mean_attributes);
      else if (atts[a].seq_type == 3) snprintf(buf, sizeof(buf), "mean_attributes 0x%x: bit %u names attribute %u, the normals: mean normals are not built (octahedral integers do not average across the fold)", ck.rq.mean_attributes, a, a);
      else continue;
      return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, buf);
    }
  }
  if (ck.rq.votes()) {       // vote_attributes: every set bit names an attribute of this cloud's stream whose tuples can be voted on
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    char buf[240];
    for (uint32_t a = 0; a < 32u; ++a) {
      if (!((ck.rq.vote_attributes >> a) & 1u)) continue;
      if (a >= atts.size()) snprintf(buf, sizeof(buf), "vote_attributes 0x%x: bit %u names attribute %u of the stream, which has %zu attributes", ck.rq.vote_attributes, a, a, atts.size());
      else if (a == 0) snprintf(buf, sizeof(buf), "vote_attributes 0x%x: bit 0 names attribute 0, the positions: they are equal inside a cell and are never voted on", ck.rq.vote_attributes);
      else if (atts[a].seq_type == 3) snprintf(buf, sizeof(buf), "vote_attributes 0x%x: bit %u names attribute %u, the normals: a vote over octahedral integers is not built", ck.rq.vote_attributes, a, a);
      else if (atts[a].nc > 2) snprintf(buf, sizeof(buf), "vote_attributes 0x%x: bit %u names attribute %u of %d components: only tuples of 1 or 2 components, which pack into 64 bits, are built", ck.rq.vote_attributes, a, a, (int)atts[a].nc);
      else continue;
      return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, buf);
    }
  }
  if (!ck.rq.split()) return;
  // (lod_base_bits: a level more can cost a slot more -- sum ceil(m_l / N) <= ceil(m / N) + non-empty levels - 1)
  const uint64_t parts = synth::split_count(m.num_vertices, ck.rq.part_size()) + (ck.rq.lod_levels() - 1u);
  if (parts > DSA_ENCODE_MAX_PARTS && ck.rq.lod()) {
    char buf[240];
    snprintf(buf, sizeof(buf), "lod_base_bits %u with part_cells %u may cut the cloud's n = %u points into %llu parts (ceil(n / part_cells) + %u levels - 1): at most %u (DSA_ENCODE_MAX_PARTS)",
             ck.rq.lod_base_bits, ck.rq.part_cells, m.num_vertices, (unsigned long long)parts, ck.rq.lod_levels(), DSA_ENCODE_MAX_PARTS);
    return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, buf);
  }
  if (parts > DSA_ENCODE_MAX_PARTS && ck.rq.cell_parts()) {       // (the host bounds the parts by the points that came in: the kept ones are the device's to count)
    char buf[200];
    snprintf(buf, sizeof(buf), "part_cells %u may cut the cloud's n = %u points into %llu parts: at most %u (DSA_ENCODE_MAX_PARTS)", ck.rq.part_cells, m.num_vertices, (unsigned long long)parts, DSA_ENCODE_MAX_PARTS);
    return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, buf);
  }
  if (parts > DSA_ENCODE_MAX_PARTS) {
    char buf[160];
    snprintf(buf, sizeof(buf), "part_points %u cuts the cloud's n = %u points into %llu parts: at most %u (DSA_ENCODE_MAX_PARTS)", ck.rq.part_points, m.num_vertices, (unsigned long long)parts, DSA_ENCODE_MAX_PARTS);
    return ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, buf);
  }
  ck.parts[i] = (uint32_t)parts;
}

// ---- the regions of a stream, shared by both layouts
// A value stream's description and its source values among the inputs (`rows` of them; S.nv, S.prediction, S.linear: the caller's).
static void enc_value_stream_input(dsa::EncStream &S, const synth::PortableAttr &a, const dsa_mesh_input &m, uint32_t rows, EncArena &A, std::vector<EncUpload> &ups) {
  const bool integer = a.seq_type == 1;                  // the generic uint8 attribute, an integer extra
  const void *src = a.extra_values ? a.extra_values
                    : (a.att_type == 0 ? (const void *)m.positions : (a.att_type == 1 ? (const void *)m.normals : (integer ? (const void *)m.generic : (const void *)m.texcoords)));
  S.rows = rows; S.nc_out = (uint32_t)a.nc_out; S.nc = (uint32_t)a.nc; S.kind = a.seq_type == 3 ? 1u : (integer ? 2u : 0u);
  S.bits = integer ? 9u : (uint32_t)a.bits;              // (9: the zig-zagged corrections of bytes are below 512)
  S.elem = integer ? (uint32_t)a.data_type : 0u;
  S.grid_nonfinite = S.grid_off = dsa::ENC_GRID_NO_ROW;  // (own bounds: k_enc_bounds writes grid_nonfinite; a grid: k_enc_grid_quantize both)
  if (S.kind == 0 && a.grid && a.grid->mode != 0) {      // the header's floats are the grid's
    S.grid_mode = 1;
    for (uint32_t c = 0; c < S.nc_out && c < 4; ++c) S.qmin[c] = a.grid->origin[c];
    S.qrange = a.grid->range;
  }
  S.src = A.put(ups, src, (integer ? (uint64_t)synth::data_type_size(a.data_type) : 4ull) * rows * S.nc_out, false);
}
static void enc_table_regions(dsa::EncStream &S, EncArena &A) {
  const uint64_t table_cap = std::max<uint64_t>(S.hist_cap, 64);   // the tagged scheme's alphabet is 33 bit lengths
  S.prob = A.take(4ull * table_cap); S.cum = A.take(4ull * table_cap);
  S.plan_order = A.take(4ull * table_cap); S.plan_tmp = A.take(4ull * table_cap);
}
// What the kernels write of a value stream of up to `cap` entries; hist_cap: of an integer extra by the values present, 0: by the bits.
// vals: not 0: where the values lie already (a part behind the first of a split cloud).
static void enc_value_stream_regions(dsa::EncStream &S, uint32_t cap, uint32_t hist_cap, EncArena &A, uint64_t vals = 0) {
  S.vals = vals ? vals : A.take(4ull * S.rows * S.nc);
  S.d = S.linear ? S.vals : A.take(4ull * cap * S.nc);   // linear order: the values are the entries
  S.syms = A.take(4ull * cap * S.nc); S.bl = A.take(cap);
  S.hist_cap = hist_cap ? hist_cap : (1u << S.bits) + 2u;        // zig-zag of a wrapped correction / a positive octahedral correction fits
  S.hist_raw = A.take(4ull * S.hist_cap);
  S.out_cap = 4u * cap * S.nc + 16u;                     // (tagged bit fields are at most 32 bits a symbol, a coded symbol at most 20 bits and the flush)
  S.out_rans = A.take(S.out_cap); S.out_bits = A.take(S.out_cap);
  enc_table_regions(S, A);
}
// A list stream (kind 3: one component, its symbols given) of `count` symbols below hist_cap, and its regions.  own: symbols, bit
// lengths and coded bytes lie in regions of the stream's own (else a kernel points it at regions of its mesh and sets the count);
// syms_given: the symbols are among the inputs.
static void enc_list_stream(dsa::EncStream &S, uint32_t hist_cap, uint32_t count) { S.kind = 3; S.nc = S.nc_out = 1; S.hist_cap = hist_cap; S.nv = count; }
static void enc_list_stream_regions(dsa::EncStream &S, EncArena &A, bool own, bool syms_given) {
  S.hist_raw = A.take(4ull * S.hist_cap);
  enc_table_regions(S, A);
  if (!own) return;
  if (!syms_given) S.syms = A.take(4ull * S.nv);
  S.bl = A.take(S.nv); S.out_cap = 4u * S.nv + 16u; S.out_rans = A.take(S.out_cap); S.out_bits = A.take(S.out_cap);
}
// records of the chunk's streams, all zero, and first_stream from the streams each mesh that passed its checks has beside its attributes'
static void enc_layout_begin(EncChunk &ck, uint32_t more_streams_of_valence, uint32_t more_streams) {
  EncLayout &L = ck.L;
  L.first_stream.assign(ck.n + 1, 0);
  for (uint32_t i = 0; i < ck.n; ++i) {
    L.any_valence = L.any_valence || ck.valence_of(i);
    for (size_t k = 0; ck.good(i) && k < ck.plans[i].atts.size(); ++k) { const synth::PortableAttr &a = ck.plans[i].atts[k]; L.any_grid = L.any_grid || (a.seq_type == 2 && a.grid && a.grid->mode != 0); }
    L.first_stream[i + 1] = L.first_stream[i] + (ck.good(i) ? ((uint32_t)ck.plans[i].atts.size() + more_streams + (ck.valence_of(i) ? more_streams_of_valence : 0u)) * ck.num_parts(i) : 0u);
  }
  dsa::EncStream zero;
  memset(&zero, 0, sizeof(zero));
  L.streams.assign(L.first_stream[ck.n], zero);
  if (ck.rq.track_rows && !ck.rq.sequential) L.rows_of_stream.assign(L.streams.size(), DSA_INVALID);
}

// ---- the arena of a chunk of Edgebreaker streams
static void enc_layout(EncChunk &ck) {
  EncLayout &L = ck.L;
  const uint32_t n = ck.n;
  const bool host_conn = ck.host_conn, want_pd = ck.want_pd;
  EncArena A;
  A.log = ck.region_log;
  enc_layout_begin(ck, 6, 0);
  // inputs, phase A (device connectivity): the faces, and right behind them the corner ids (the seam kernels read them as they
  // were uploaded).  Half of what the walks wait for is the upload of the faces: indices below 65 536 are narrowed to 16 bits by
  // the copy into pinned staging (which reads them anyway) and widened by the first kernel of the chunk; the ids likewise.
  if (!host_conn) {
    dsa::EncConn none;
    memset(&none, 0, sizeof(none));
    none.status = dsa::ENC_ISOLATED;
    L.conns.assign(n, none);
  }
  for (uint32_t i = 0; i < n && !host_conn; ++i) {
    if (!ck.good(i)) continue;
    const dsa_mesh_input &m = ck.mesh(i);
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    dsa::EncConn &C = L.conns[i];
    C.status = dsa::ENC_OK;
    C.F = ck.coded_faces(i); C.V = ck.coded_vertices(i); C.split_cap = C.F; C.fail_key = 0xFFFFFFFFu;
    C.vstream = ck.valence_of(i) ? L.first_stream[i] + (uint32_t)atts.size() : DSA_INVALID;
    C.faces_narrow = C.V <= 65536 ? 1u : 0u;
    (C.faces_narrow ? C.faces16 : C.faces) = A.put(L.uploads_a, ck.rep.empty() ? m.faces : ck.rep[i].c2v.data(), (C.faces_narrow ? 6ull : 12ull) * C.F, C.faces_narrow != 0);
    if (!ck.rep.empty()) {                                     // a repaired table: its opposites are given, and the row of every vertex
      C.opp = A.put(L.uploads_a, ck.rep[i].opp.data(), 12ull * C.F, false);
      dsa::EncRepairRows R;
      memset(&R, 0, sizeof(R));
      R.row = A.put(L.uploads_a, ck.rep[i].row.data(), 4ull * C.V, false); R.count = C.V; R.pad = i;
      ck.rep_rows.push_back(R);
    }
    L.maxf = std::max(L.maxf, C.F);
    for (size_t k = 0; k < atts.size(); ++k) {
      if (!atts[k].corner_value) continue;
      dsa::EncSeam Z;
      memset(&Z, 0, sizeof(Z));
      Z.mesh = i; Z.stream = L.first_stream[i] + (uint32_t)k; Z.ids_narrow = ck.ids_narrow(i, atts[k]) ? 1u : 0u; Z.rows = ck.rows_of(i, atts[k]);
      const uint64_t id_bytes = (Z.ids_narrow ? 6ull : 12ull) * C.F;
      if (!ck.rep_ids.empty() && k < ck.rep_ids[i].size() && ck.rep_ids[i][k] != EncChunk::kNoIds) {      // (atts[k].corner_value is the caller's array, over the source's faces)
        Z.ids = A.take(id_bytes);
        L.copies_a.push_back({Z.ids, ck.rep_ids[i][k], (uint32_t)id_bytes, 0});
      } else Z.ids = A.put(L.uploads_a, atts[k].corner_value, id_bytes, Z.ids_narrow != 0);
      L.seams.push_back(Z);
    }
  }
  // inputs, the rest: the source values of every stream; with host connectivity also the entry maps of the mesh (and of attributes
  // given per corner), the topology views of the schemes that read them, and the valence context lists
  for (uint32_t i = 0; i < n; ++i) {
    if (!ck.good(i)) continue;
    const dsa_mesh_input &m = ck.mesh(i);
    const synth::MeshPlan &pl = ck.plans[i];
    const uint32_t V = ck.coded_vertices(i), s0 = L.first_stream[i];
    auto put = [&](const void *src, uint64_t bytes) { return A.put(L.uploads, src, bytes, false); };
    const bool repaired = ck.rq.repair && !ck.c2row[i].empty();
    const uint64_t t_c2row = repaired ? put(ck.c2row[i].data(), 4ull * ck.c2row[i].size()) : 0;
    uint64_t o_e2v[2] = {0, 0}, o_ops[2] = {0, 0}, t_c2v = 0, t_opp = 0, t_d2c[2] = {0, 0}, t_v2d[2] = {0, 0};       // [1]: in prediction-degree order
    bool needs_topo = false;
    for (const synth::PortableAttr &a : pl.atts) needs_topo = needs_topo || enc_topo_scheme(a);
    if (host_conn) {
      o_e2v[0] = put(ck.e2v[i].data(), 4ull * V); o_ops[0] = put(ck.ops[i].data(), 12ull * V);
      if (want_pd) { o_e2v[1] = put(ck.e2v_pd[i].data(), 4ull * V); o_ops[1] = put(ck.ops_pd[i].data(), 12ull * V); }
      if (needs_topo) {                                       // the position table and orders, once per mesh
        t_c2v = put(pl.ct.c2v.data(), 4ull * pl.ct.c2v.size()); t_opp = put(pl.ct.opp.data(), 4ull * pl.ct.opp.size());
        t_d2c[0] = put(pl.seq.data_to_corner.data(), 4ull * pl.seq.data_to_corner.size()); t_v2d[0] = put(pl.seq.vertex_to_data.data(), 4ull * pl.seq.vertex_to_data.size());
        if (want_pd) { t_d2c[1] = put(pl.seq_pd.data_to_corner.data(), 4ull * pl.seq_pd.data_to_corner.size()); t_v2d[1] = put(pl.seq_pd.vertex_to_data.data(), 4ull * pl.seq_pd.vertex_to_data.size()); }
      }
    }
    // track_rows: a record per attribute; over a welded mesh the representative points of its rows go up, every key set's once
    const std::vector<uint32_t> *row_points[2 + synth::kMaxAttributes * 2] = {};
    uint64_t row_points_at[2 + synth::kMaxAttributes * 2] = {};
    size_t num_row_points = 0;
    for (size_t k = 0; ck.rq.track_rows && k < pl.atts.size(); ++k) {
      dsa::EncRows R;
      memset(&R, 0, sizeof(R));
      R.stream = s0 + (uint32_t)k;
      if (!ck.welded.empty()) {
        const std::vector<uint32_t> *point = &synth::weld_row_points(ck.weld[i], pl.atts[k]);
        size_t q = 0;
        while (q < num_row_points && row_points[q] != point) ++q;
        if (q == num_row_points) { row_points[q] = point; row_points_at[q] = put(point->data(), 4ull * point->size()); ++num_row_points; }
        R.point = row_points_at[q]; R.num_points = (uint32_t)point->size();
      }
      L.rows_of_stream[R.stream] = (uint32_t)L.rows.size();
      L.rows.push_back(R);
    }
    for (size_t k = 0; k < pl.atts.size(); ++k) {
      const synth::PortableAttr &a = pl.atts[k];
      dsa::EncStream &S = L.streams[s0 + k];
      const bool pd = ck.uses_pd(i, k);
      S.nv = V; S.prediction = (uint32_t)a.prediction;
      if (host_conn) {
        S.e2v = o_e2v[pd]; S.ops = o_ops[pd];
        if (a.corner_value) {                                 // as many entries as its walk has, its own value rows, seamed: its own operands
          S.nv = (uint32_t)ck.att_e2v[i][k].size();
          S.e2v = put(ck.att_e2v[i][k].data(), 4ull * S.nv);
          if (!ck.att_ops[i][k].empty()) S.ops = put(ck.att_ops[i][k].data(), 12ull * S.nv);
        }
      } else if (a.corner_value) S.pd_want = pd ? 1u : 0u;
      enc_value_stream_input(S, a, m, ck.rows_of(i, a), A, L.uploads);
      if (repaired && !host_conn) S.t_c2p = t_c2row;          // (kept below, where the connectivity's own regions become the stream's view)
      if (!host_conn || !enc_topo_scheme(a)) continue;
      S.t_c2p = S.t_c2a = t_c2v; S.t_opp = t_opp; S.t_d2c = t_d2c[pd]; S.t_v2d = t_v2d[pd];
      if (repaired) S.t_c2p = t_c2row;
      if (a.corner_value && pl.seamed(k)) {                   // a seamed attribute's own table and order
        const std::vector<uint32_t> &c2a = pl.conns[k].c2v, &o2 = ck.att_opp[i][k], &d2c = pl.seq_att[k].data_to_corner;
        const std::vector<int32_t> &v2d = pl.seq_att[k].vertex_to_data;
        S.t_c2a = put(c2a.data(), 4ull * c2a.size()); S.t_opp = put(o2.data(), 4ull * o2.size());
        S.t_d2c = put(d2c.data(), 4ull * d2c.size()); S.t_v2d = put(v2d.data(), 4ull * v2d.size());
      }
    }
    // valence symbols: six more streams, the context lists (alphabet C S L R E).  Host connectivity: the host coder's lists.
    for (uint32_t k = 0; k < 6 && ck.valence_of(i); ++k) {
      dsa::EncStream &S = L.streams[s0 + pl.atts.size() + k];
      const std::vector<uint32_t> &list = pl.ctx_symbols[k];
      enc_list_stream(S, 8, host_conn ? (uint32_t)list.size() : 0u);
      S.bits = 3;
      if (host_conn && S.nv) S.syms = put(list.data(), 4ull * S.nv);
    }
  }
  L.input_bytes = A.cur;
  // everything the kernels write
  size_t z = 0, rr = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!ck.good(i)) continue;
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    const uint64_t V = ck.coded_vertices(i), F = ck.coded_faces(i);
    const uint32_t s0 = L.first_stream[i];
    dsa::EncConn *C = host_conn ? nullptr : &L.conns[i];
    if (C) {
      if (C->faces_narrow) C->faces = A.take(12 * F);
      if (ck.rep.empty()) C->opp = A.take(12 * F);
      C->voff = A.take(4 * (V + 1)); C->vcur = A.take(4 * V); C->vlist = A.take(12 * F); C->vcorner = A.take(4 * V);
      C->vvis = A.take(V); C->frec = A.take(32 * F);
      C->stack = A.take(4 * F); C->processed = A.take(4 * F); C->init_corners = A.take(4 * F);
      C->symbols = A.take(F); C->start_bits = A.take(F); C->splits = A.take(12ull * C->split_cap);
      C->d2c = A.take(4 * V); C->v2d = A.take(4 * V); C->e2v = A.take(4 * V); C->ops = A.take(12 * V);
      if (want_pd) {
        C->pd_d2c = A.take(4 * V); C->pd_v2d = A.take(4 * V); C->pd_e2v = A.take(4 * V); C->pd_ops = A.take(12 * V);
        C->pd_next = A.take(12 * F); C->pd_degree = A.take(4 * V); C->pd_fvis = A.take(F);
      }
      if (!ck.rep.empty()) { dsa::EncRepairRows &R = ck.rep_rows[rr++]; R.e2v = C->e2v; R.pd_e2v = want_pd ? C->pd_e2v : 0; }      // (pushed above in this order)
      if (ck.valence_of(i)) {
        C->init_time = A.take(4 * F); C->vtime = A.take(4 * F); C->vval = A.take(4 * (V + F)); C->vc2v = A.take(12 * F);
        C->vctx = A.take(F); C->vsyms = A.take(4 * F); C->vbl = A.take(F); C->vrans = A.take(4 * F + 96); C->vbits = A.take(4 * F + 96);
      }
    }
    for (size_t k = 0; k < atts.size(); ++k) {
      const synth::PortableAttr &a = atts[k];
      dsa::EncStream &S = L.streams[s0 + k];
      const bool pd = ck.uses_pd(i, k);
      // entries: as the inputs said, or for an attribute given per corner on the device path as many as its walk may have (3F at
      // most, k_enc_seam_operands sets the count)
      uint32_t cap = S.nv;
      if (C) { S.e2v = pd ? C->pd_e2v : C->e2v; S.ops = pd ? C->pd_ops : C->ops; }
      if (C && a.corner_value) {
        cap = 3u * (uint32_t)F;
        dsa::EncSeam &Z = L.seams[z++];
        Z.edge_seam = A.take(3 * F); Z.vert_seam = A.take(V); Z.afirst = A.take(4 * V); Z.aoff = A.take(4 * (V + 1));
        Z.c2av = A.take(12 * F); Z.opp2 = A.take(12 * F); Z.v2lm = A.take(12 * F); Z.avis = A.take(3 * F); Z.frec = A.take(32 * F);
        Z.stack = A.take(4 * F); Z.d2c = A.take(12 * F); Z.v2d = A.take(12 * F); Z.e2v = A.take(12 * F); Z.ops = A.take(36 * F);
        Z.rank = A.take(4 * F); Z.rcorner = A.take(4 * F); Z.eoff = A.take(4 * (F + 1)); Z.bits = A.take(4 * ((3 * F + 31) / 32));
        S.e2v = Z.e2v; S.ops = Z.ops;
      }
      enc_value_stream_regions(S, cap, ck.hist_cap_of(i, k), A);
      if (ck.rq.track_rows) { dsa::EncRows &R = L.rows[L.rows_of_stream[s0 + k]]; R.cap = cap; R.out = A.take(4ull * cap); }
      L.max_rows = std::max(L.max_rows, std::max(S.rows, cap));
      if (!enc_topo_scheme(a)) continue;
      if (C) { const uint64_t c2row = S.t_c2p; S.t_c2p = S.t_c2a = C->faces; S.t_opp = C->opp; S.t_d2c = pd ? C->pd_d2c : C->d2c; S.t_v2d = pd ? C->pd_v2d : C->v2d; if (!ck.rep.empty()) S.t_c2p = c2row; }      // the connectivity's own (a repaired table: positions by row)
      S.t_nc3 = 3u * (uint32_t)F;
      if (!enc_multi_scheme(a)) {
        S.pos_vals = L.streams[s0].vals;                      // (the positions are attribute 0: their stream is the mesh's first)
        if (a.seq_type == 2) S.ori = A.take(cap);
        S.flags = A.take(4ull * ((cap + 31) / 32));
        continue;
      }
      L.any_multi = true;
      if (a.prediction != 4) continue;
      L.any_crease = true;                                    // found + crease flags per entry; the four crease lists
      S.ori = A.take(cap);
      S.flags = A.take(4ull * dsa::em_crease_words(cap, S.cr_at));
    }
    // the context lists.  Device connectivity: their sizes and places are set by k_enc_val_split in the mesh's regions.
    for (uint32_t k = 0; k < 6 && ck.valence_of(i); ++k) enc_list_stream_regions(L.streams[s0 + atts.size() + k], A, host_conn, host_conn);
  }
  L.total_bytes = A.cur;
}

// ---- the arena of a chunk of sequential streams: the attributes in point order, and with compressed indices the index stream
// behind them, a list of 3F symbols below 2V given by k_enc_seq_indices from the faces (16-bit where every index fits)
// EncRequest::point_order: no stream is linear -- every value stream of a cloud reads its entries through one shared entry -> row
// map, the permutation the sort kernels of dsa_encode_order.h leave (their records and tile list among the uploads, their
// regions among what the kernels write).  Without it nothing here moves.
// EncRequest::merge_points: the map is the other row buffer, where k_enc_merge_compact leaves the kept rows, and a region of 4
// bytes per point takes row_entries; every region stays sized for the points that came in, k_enc_merge_scan lowers nv below them.
// EncRequest::split: a cloud of P parts has P sets of stream records (stream s0 + p * attributes + k: attribute k of part p) on one
// set of source values and integers; the EncPart records and their (part, tile) pairs go up beside the sort's.
// EncRequest::cell_parts (split and merge): P is the device's to know, so a cloud has P_max = ceil(n / part_cells) part SLOTS, each
// with records, regions and tiles for min(part_cells, n) points -- under n + part_cells points per attribute in all; the streams' map
// is the kept buffer, as with the merge, and k_enc_part_cells writes every slot's lo, n, nv and e2v.
// EncRequest::lod (cell_parts with levels): ceil(n / part_cells) + L - 1 slots, the streams' map is the lod buffer, which with pos takes
// the sort's dead key buffer; a level table per cloud among the kernels' regions; k_enc_part_cells writes the slots from it.
// EncRequest::means (merge with mean_attributes): an EncCellStreams per cloud and an EncMean per masked stream among the uploads; behind
// every other region a u32[n] count region per cloud and an i64[n nc] sum region per masked stream, one range that is zeroed on the
// stream in front of k_enc_mean_sum.  No region is reused and nothing else grows.
// EncRequest::votes (merge with vote_attributes): likewise an EncCellStreams per cloud and an EncVote per voted stream among the uploads;
// behind the means' range per voted stream a table of 2 n slots of 8 bytes (a crowded chunk of small clouds pays for its points, not
// for tiles), u32[n] counts and u64[n] values, one range that is zeroed on the stream in front of k_enc_vote_count.
// EncRequest::normal_means (merge with mean_normals): an EncCellStreams per cloud and an EncNormal per cloud that has normals among the
// uploads; behind the votes' range per such cloud a u32[n] count region and an i64[3 n] sum region, one range that is zeroed on the
// stream in front of k_enc_normal_sum.  A chunk without normals has none of it.
static void enc_layout_sequential(EncChunk &ck) {
  EncLayout &L = ck.L;
  const bool is_mesh = ck.rq.seq.geometry == 1, compressed = is_mesh && ck.rq.seq.compress_connectivity == 1, ordered = ck.rq.point_order;
  const bool merge = ordered && !is_mesh && ck.rq.merge_points, split = ck.rq.split();
  const bool cell_parts = ck.rq.cell_parts();
  L.merge = merge; L.split = split; L.cell_parts = cell_parts; L.lod = ck.rq.lod();
  if (merge || split) L.ord_of_mesh.assign(ck.n, DSA_INVALID);
  if (split) L.part_of_mesh.assign(ck.n, DSA_INVALID);
  EncArena A;
  A.log = ck.region_log;
  enc_layout_begin(ck, 0, compressed ? 1 : 0);
  for (uint32_t i = 0; i < ck.n; ++i) {
    if (!ck.good(i)) continue;
    const dsa_mesh_input &m = ck.mesh(i);
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    const uint32_t V = m.num_vertices, s0 = L.first_stream[i];
    for (size_t k = 0; k < atts.size(); ++k) {
      dsa::EncStream &S = L.streams[s0 + k];
      S.nv = V; S.prediction = 0; S.linear = ordered ? 0u : 1u;
      enc_value_stream_input(S, atts[k], m, V, A, L.uploads);
    }
    if (ordered) {
      dsa::EncOrder O;
      memset(&O, 0, sizeof(O));
      O.n = V; O.tiles = (V + ORD_TILE - 1u) / ORD_TILE; O.bits = (uint32_t)ck.opt.pos_bits; O.last = dsa::enc_order_passes(O.bits) & 1u;
      if (merge) { O.merge = 1; O.stream0 = s0; O.streams = (uint32_t)atts.size(); O.voxel_shift = ck.rq.voxel_shift(); O.voxel_point = O.voxel_shift ? ck.rq.voxel_point : 0u; }
      if (merge || split) L.ord_of_mesh[i] = (uint32_t)L.ord.size();
      // the masked and the voted streams of the cloud (the first part's: the parts share its vals)
      // (centroids: the positions too, the cloud's first record -- the one that counts the rows of every voxel)
      if (ck.rq.means()) L.mean_pass.list(ck.rq.mean_attributes | (ck.rq.centroids() ? 1u : 0u), s0, atts.size(), [&](uint32_t s) {
        dsa::EncMean M;
        memset(&M, 0, sizeof(M));
        M.nc = L.streams[s].nc;
        L.means.push_back(M);
      }, ck.rq.centroids() ? 0u : 1u);
      if (ck.rq.nearest()) L.near_pass.list(1u, s0, atts.size(), [&](uint32_t) {
        dsa::EncVoxel X;
        memset(&X, 0, sizeof(X));
        L.voxels.push_back(X);
      }, 0u);
      if (ck.rq.votes()) L.vote_pass.list(ck.rq.vote_attributes, s0, atts.size(), [&](uint32_t s) {
        dsa::EncVote X;
        memset(&X, 0, sizeof(X));
        X.nc = L.streams[s].nc; X.cap = 2u * V;                // (V <= 2^28: enc_check_sequential_mesh)
        L.votes.push_back(X);
      });
      // the normals of the cloud, attribute 1 where it has them (plan_sequential_attributes)
      if (ck.rq.normal_means()) L.normal_pass.list(atts.size() > 1 && atts[1].att_type == 1 && !atts[1].extra_values ? 2u : 0u, s0, atts.size(), [&](uint32_t s) {
        dsa::EncNormal X;
        memset(&X, 0, sizeof(X));
        X.bits = L.streams[s].bits;
        L.normals.push_back(X);
      });
      for (uint32_t t = 0; t < O.tiles; ++t) L.ord_tiles.push_back({(uint32_t)L.ord.size(), t});
      if (split) {                                             // the parts of the cloud: their sizes need nothing of the device
        L.part_of_mesh[i] = (uint32_t)L.parts.size();
        // (part_cells: the slots of the cloud, lo and n the device's to write -- k_enc_part_cells -- and tiles for the most a slot can hold)
        if (cell_parts) { O.part_cells = ck.rq.part_cells; O.part0 = (uint32_t)L.parts.size(); O.part_slots = ck.num_parts(i); O.lod_bits = L.lod ? ck.rq.lod_base_bits : 0u; }
        for (uint32_t p = 0, np = ck.num_parts(i); p < np; ++p) {
          dsa::EncPart P;
          memset(&P, 0, sizeof(P));
          P.cloud = (uint32_t)L.ord.size();
          if (!cell_parts) { P.lo = synth::split_bound(V, np, p); P.n = synth::split_bound(V, np, p + 1u) - P.lo; }
          for (int c = 0; c < 3; ++c) { P.qmin[c] = INT32_MAX; P.qmax[c] = INT32_MIN; }
          for (uint32_t t = 0, nt = ((cell_parts ? std::min(ck.rq.part_cells, V) : P.n) + ORD_TILE - 1u) / ORD_TILE; t < nt; ++t) L.part_tiles.push_back({(uint32_t)L.parts.size(), t});
          L.parts.push_back(P);
        }
      }
      L.ord.push_back(O);
    }
    if (!compressed) continue;
    dsa::EncSeqIdx X;
    memset(&X, 0, sizeof(X));
    X.count = 3u * m.num_faces; X.narrow = V <= 65536 ? 1u : 0u; X.stream = s0 + (uint32_t)atts.size();
    X.faces = A.put(L.uploads, m.faces, (X.narrow ? 2ull : 4ull) * X.count, X.narrow != 0);
    L.idx.push_back(X);
    L.max_count = std::max(L.max_count, X.count);
    enc_list_stream(L.streams[X.stream], 2u * V, X.count);
    if (ordered) { dsa::EncOrder &O = L.ord.back(); O.faces = X.faces; O.count = X.count; O.narrow = X.narrow; }
  }
  if (!L.ord.empty()) {                                        // (the vectors are complete: their storage stays where it is until the upload)
    L.ord_passes = dsa::enc_order_passes((uint32_t)ck.opt.pos_bits);
    L.ord_at = A.put(L.uploads, L.ord.data(), sizeof(dsa::EncOrder) * L.ord.size(), false);
    L.ord_tiles_at = A.put(L.uploads, L.ord_tiles.data(), sizeof(dsa::EncOrderTile) * L.ord_tiles.size(), false);
  }
  L.mean_pass.upload(L.means, A, L.uploads);
  L.vote_pass.upload(L.votes, A, L.uploads);
  L.normal_pass.upload(L.normals, A, L.uploads);
  L.near_pass.upload(L.voxels, A, L.uploads);
  if (!L.parts.empty()) {
    L.parts_at = A.put(L.uploads, L.parts.data(), sizeof(dsa::EncPart) * L.parts.size(), false);
    L.part_tiles_at = A.put(L.uploads, L.part_tiles.data(), sizeof(dsa::EncPartTile) * L.part_tiles.size(), false);
  }
  L.input_bytes = A.cur;
  for (uint32_t i = 0, o = 0; i < ck.n; ++i) {
    if (!ck.good(i)) continue;
    const uint32_t V = ck.mesh(i).num_vertices, s0 = L.first_stream[i], na = (uint32_t)ck.plans[i].atts.size();
    if (ordered) {                                             // the sort's regions; the buffer its last pass writes is the streams' map
      dsa::EncOrder &O = L.ord[o++];
      for (int b = 0; b < 2; ++b) { O.key[b] = A.take(8ull * V); O.row[b] = A.take(4ull * V); }
      O.hist = A.take(4ull * ORD_RADIX * O.tiles);
      if (is_mesh) O.rank = A.take(4ull * V);
      if (merge) O.cells = A.take(4ull * V);
      // (lod_base_bits: lod and pos in the key buffer the last pass read -- dead behind the merge, two u32[n] -- and the level table)
      if (L.lod) { O.lod_rows = O.key[O.last ^ 1u]; O.lod_table = A.take(sizeof(dsa::EncLodTable)); }
      for (uint32_t k = 0; k < na; ++k) L.streams[s0 + k].e2v = merge ? dsa::ord_kept(O) : dsa::ord_sorted(O).row;
    }
    if (split) {
      // a set of records per part: the first part's with the part's entries -- a slice of the sorted rows -- and regions of the
      // part's size; the values are the cloud's, quantised once
      const dsa::EncOrder &O = L.ord[o - 1];
      for (uint32_t p = 0, np = ck.num_parts(i); p < np; ++p) {
        const dsa::EncPart &P = L.parts[L.part_of_mesh[i] + p];
        for (uint32_t k = 0; k < na; ++k) {
          dsa::EncStream &S = L.streams[s0 + p * na + k];
          if (p) { S = L.streams[s0 + k]; S.part = dsa::ENC_PART_BEHIND; S.grid_mode = 0; }      // (grid_mode 0: k_enc_grid_quantize passes it by too; the header's floats are the first part's)
          if (cell_parts) {                                    // a slot: nv and e2v are the device's to write; regions for the most it can hold
            if (p) { S.part |= dsa::ENC_PART_SIZED; S.nv = 0; }
            enc_value_stream_regions(S, std::min(ck.rq.part_cells, V), ck.hist_cap_of(i, k), A, p ? L.streams[s0 + k].vals : 0);
            continue;
          }
          S.nv = P.n; S.e2v = dsa::ord_sorted(O).row + 4ull * P.lo;
          enc_value_stream_regions(S, P.n, ck.hist_cap_of(i, k), A, p ? L.streams[s0 + k].vals : 0);
        }
      }
    } else
    for (uint32_t k = 0; k < na; ++k) enc_value_stream_regions(L.streams[s0 + k], V, ck.hist_cap_of(i, k), A);
    if (ordered) L.ord[o - 1].vals = L.streams[s0].vals;      // (the positions are attribute 0: their stream is the mesh's first)
    L.max_rows = std::max(L.max_rows, V);
    if (compressed) enc_list_stream_regions(L.streams[s0 + na], A, true, false);
  }
  // what a cell pass accumulates in: one range behind everything else, zeroed as one
  auto range = [&](const EncCellPass &P, uint64_t &at, uint64_t &bytes, auto &&regions) { if (P.stream.empty()) return; at = A.cur; regions(); bytes = A.cur - at; };
  range(L.mean_pass, L.mean_zero_at, L.mean_zero_bytes, [&] {      // the counts of every cloud and the sums of every masked stream
    for (size_t o = 0; o < L.mean_pass.clouds.size(); ++o) {
      const dsa::EncCellStreams &C = L.mean_pass.clouds[o];
      if (C.count == 0) continue;
      const uint64_t V = L.ord[o].n, cnt = A.take(4ull * V);
      for (uint32_t k = C.first; k < C.first + C.count; ++k) { dsa::EncMean &M = L.means[k]; M.vals = L.streams[L.mean_pass.stream[k]].vals; M.cnt = cnt; M.acc = A.take(8ull * V * M.nc); }
    }
  });
  range(L.vote_pass, L.vote_zero_at, L.vote_zero_bytes, [&] {      // behind the means': the table, the counts and the values of every voted stream
    for (size_t k = 0; k < L.votes.size(); ++k) {
      dsa::EncVote &X = L.votes[k];
      const uint64_t V = X.cap / 2u;
      X.vals = L.streams[L.vote_pass.stream[k]].vals;
      X.table = A.take(8ull * X.cap); X.best_cnt = A.take(4ull * V); X.best_val = A.take(8ull * V);
    }
  });
  range(L.normal_pass, L.normal_zero_at, L.normal_zero_bytes, [&] {  // behind the votes': the counts and the vector sums of every cloud with normals
    for (size_t o = 0; o < L.normal_pass.clouds.size(); ++o) {
      const dsa::EncCellStreams &C = L.normal_pass.clouds[o];
      if (C.count == 0) continue;
      const uint64_t V = L.ord[o].n;
      dsa::EncNormal &X = L.normals[C.first];
      X.vals = L.streams[L.normal_pass.stream[C.first]].vals; X.cnt = A.take(4ull * V); X.acc = A.take(24ull * V);
    }
  });
  range(L.near_pass, L.near_zero_at, L.near_zero_bytes, [&] {      // behind the normals': the best distance and row of every voxel of every cloud
    for (size_t o = 0; o < L.near_pass.clouds.size(); ++o) {
      const dsa::EncCellStreams &C = L.near_pass.clouds[o];
      if (C.count == 0) continue;
      const uint64_t V = L.ord[o].n;
      dsa::EncVoxel &X = L.voxels[C.first];
      X.best_dist = A.take(8ull * V); X.best_row = A.take(4ull * V);
    }
  });
  L.total_bytes = A.cur;
}
