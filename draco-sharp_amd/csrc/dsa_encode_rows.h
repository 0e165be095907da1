// draco-sharp_amd/csrc/dsa_encode_rows.h  (included by dsa_encode_layout.h)
//
// Entry rows (dsa_encode_rows_batch, track_rows = 1; dsa_encoded_entry_rows): which row of the caller's value array every entry of
// every attribute of a coded stream carries, so that data which does not travel in the stream -- morph targets, simulation state --
// can be carried across an encode.  Edgebreaker renumbers, the repair gives new vertices their parents' rows, the weld merges
// points: all of it is in device memory when the attribute stage has run, and is composed here before the chunk's arena goes.
//   entry -> value row   EncStream::e2v, as k_enc_gather reads it: the connectivity's order (depth first or prediction degree), the
//                        seam walk's row ids for an attribute given per corner, and over a repaired table the row of the entry's
//                        vertex -- its root parent's for a vertex the repair made (k_enc_repair_rows has rewritten e2v in place;
//                        with host connectivity enc_plan_mesh has)
//   value row -> point   a weld request: the representative point of the row's class in the attribute's key set, or of the vertex
//                        where the attribute went to the coder per vertex (synth::weld_row_points)
// k_enc_entry_rows: a thread per entry, a record per (mesh, attribute), once per chunk behind the attribute kernels; the rows leave
// the device among the pieces of the chunk's coded bytes (enc_code_streams), not in a transfer of their own.  The host coder's twin
// is synth::plan_entry_rows / welded_entry_rows (dsa_encode_host.h); tests/hostcheck/encrows_host.cpp holds the two against each
// other under the sanitizers.  k_source_rows, at the end, is the other half: the rows of a decoded batch per point.  Nothing here
// needs HIP beyond the kernels' index variables.
#pragma once
#include <stdint.h>

namespace dsa {

static const uint32_t ENC_ROWS_NONE = 0xFFFFFFFFu;      // a value row outside the weld's classes (no stream the coder writes has one)

struct EncRows {
  uint64_t point;                  // u32[num_points]: value row -> point of the caller's (a weld request); num_points 0: the row itself
  uint64_t out;                    // u32[cap] OUTPUT: the row of every entry
  uint32_t stream;                 // the EncStream whose e2v and entry count are read where they lie (a seam walk sets them on the device)
  uint32_t num_points, cap, pad;
};

template <class Stream>
__global__ __launch_bounds__(256) void k_enc_entry_rows(uint8_t *arena, const EncRows *recs, uint32_t n, const Stream *streams) {
  const uint32_t r = blockIdx.y;
  if (r >= n) return;
  const EncRows R = recs[r];
  const Stream &S = streams[R.stream];
  const uint32_t entries = S.nv < R.cap ? S.nv : R.cap;
  const uint32_t *e2v = S.linear ? nullptr : (const uint32_t *)(arena + S.e2v);
  const uint32_t *point = R.num_points ? (const uint32_t *)(arena + R.point) : nullptr;
  uint32_t *out = (uint32_t *)(arena + R.out);
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += gridDim.x * blockDim.x) {
    uint32_t row = e2v ? e2v[e] : e;
    if (point) row = row < R.num_points ? point[row] : ENC_ROWS_NONE;
    out[e] = row;
  }
}

// ---- behind a decode (dsa_batch_source_rows; dsa_source_rows.h): the rows of a decoded batch per POINT.  The decoder keeps a map
// point -> entry per attribute, and entries are the same sequence on both sides by construction of the bitstream:
//     rows[a][p] = entry_rows[a][map[a][p]]
// One table record per mesh; the tracked entry rows of every stream lie in front of the arrays in the block the kernel writes.
static const uint64_t SRC_ROWS_IDENTITY = ~0ull;      // SrcRowsAttr::map: point p is entry p (a point cloud stores no map); ::rows: entry e is row e (a sequential stream)
#define SRC_ROWS_MAX_ATT 16                           // == DSA_MAX_ATT
struct SrcRowsAttr {
  uint64_t map;                    // in the decode arena: u32[cap_points] point -> entry
  uint64_t rows;                   // in the block: u32[num_rows] the tracked entry rows
  uint64_t out;                    // in the block: u32[cap_points] OUTPUT, 64-byte aligned
  uint32_t num_rows, pad;
};
struct SrcRowsMesh {
  uint32_t num_attributes;         // 0: the mesh has no arrays (its stream is not the tracked one)
  uint32_t cap_points, pad[2];
  SrcRowsAttr att[SRC_ROWS_MAX_ATT];
};
// grid (blocks per mesh, meshes), a thread per (attribute, point): consecutive lanes consecutive points of one attribute.  Desc:
// the decoder's record of a mesh (status 0: decoded; num_points, num_attributes and att[a].num_entries as decoded), read where the
// decode left it.  A mesh one of whose attributes decoded to another number of entries than were tracked is not the stream the rows
// were kept for: nothing of it is written (dsa_batch_source_rows_layout answers for it).
template <class Desc>
__global__ __launch_bounds__(256) void k_source_rows(const uint8_t *arena, const Desc *descs, uint32_t n, const SrcRowsMesh *table, uint8_t *block) {
  const uint32_t mesh = blockIdx.y;
  if (mesh >= n) return;
  const Desc &D = descs[mesh];
  if (D.status != 0) return;
  const SrcRowsMesh &T = table[mesh];
  const uint32_t points = D.num_points < T.cap_points ? D.num_points : T.cap_points;
  if (D.num_attributes != T.num_attributes || T.num_attributes > SRC_ROWS_MAX_ATT) return;
  const uint32_t attributes = T.num_attributes;
  for (uint32_t a = 0; a < attributes; ++a) if (D.att[a].num_entries != T.att[a].num_rows) return;
  for (uint32_t a = 0; a < attributes; ++a) {
    const SrcRowsAttr A = T.att[a];
    const uint32_t *map = A.map == SRC_ROWS_IDENTITY ? nullptr : (const uint32_t *)(arena + A.map);
    const uint32_t *rows = A.rows == SRC_ROWS_IDENTITY ? nullptr : (const uint32_t *)(block + A.rows);
    uint32_t *out = (uint32_t *)(block + A.out);
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < points; p += gridDim.x * blockDim.x) {
      const uint32_t e = map ? map[p] : p;
      out[p] = e < A.num_rows ? (rows ? rows[e] : e) : ENC_ROWS_NONE;
    }
  }
}

}  // namespace dsa
