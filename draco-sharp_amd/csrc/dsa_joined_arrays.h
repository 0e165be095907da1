// draco-sharp_amd/csrc/dsa_joined_arrays.h
// Joined vertex arrays (dsa_batch_joined_arrays): the part streams of a point cloud (part_points, part_cells, lod_base_bits cut one
// cloud into many ordinary streams) as ONE array per attribute and cloud.  A group names meshes of a decoded batch; its arrays have a
// row per point of all members, in stream order (member 0, then member 1 ...) or in the order of the rows the encoder was given
// (the member's slice of the handle's permutation says where each point goes).  Three parts, as in dsa_vertex_arrays.h, whose rules
// for stride, data type and absent attributes are used unchanged: the layout of a group, the body of the gather as plain functions
// over raw pointers, and k_joined_arrays, which calls them per element.  The first two compile without HIP:
// tests/hostcheck/joined_host.cpp runs them under the sanitizers.
#pragma once
#include <stdint.h>

#include "dsa_vertex_arrays.h"

#define JA_NO_ROWS (~0ull)      // JaMember::rows: stream order, point p goes to row first_row + p
#define JA_ORDER_STREAM 0       // == DSA_JOIN_STREAM_ORDER
#define JA_ORDER_INPUT 1        // == DSA_JOIN_INPUT_ORDER
// why ja_layout_group refuses a group (the arrays stay laid out, by the first member's table)
#define JA_OK 0
#define JA_FACES 1              // a member has faces
#define JA_TABLE 2              // members differ in attribute count, or per attribute in type, data type, components or decoder type
#define JA_ROWS 3               // the row sum is above 2^32 - 1

// One entry of the member list the host hands k_joined_arrays.
struct JaMember {
  uint32_t mesh;        // of the batch
  uint32_t group;       // whose arrays it writes
  uint32_t first_row;   // of its points in stream order: the running sum of the header point counts
  uint32_t num_points;  // the header's count: rows reserved for it, and uploaded rows it has
  uint64_t rows;        // offset of its uint32[num_points] target rows inside the uploaded rows; JA_NO_ROWS
};
// A group's record is a VaMesh: no indices, cap_points = the rows of the group, every map the identity.
typedef VaMesh JaGroup;

// What the layout needs to know about a member: the fixed part of its header.
struct JaMemberIn { const VaAttrIn *atts; uint32_t natt; uint32_t points; uint32_t has_faces; };

DSA_VA_HD inline bool ja_same_attr(const VaAttrIn &x, const VaAttrIn &y) {
  return x.att_type == y.att_type && x.data_type == y.data_type && x.nc == y.nc && x.seq_type == y.seq_type;
}
// Places the arrays of one group behind `cur` and returns the new end: num_rows = the sum of the members' header point counts, the
// arrays by va_layout_mesh over the first member's attribute table.  first_row[k] receives member k's first row.  *why / *member:
// JA_OK, or the first fault and the member that shows it; a group whose rows do not fit 32 bits reserves nothing.
DSA_VA_HD inline uint64_t ja_layout_group(const JaMemberIn *mem, uint32_t count, int format, uint32_t type_mask, uint64_t cur, JaGroup &g,
                                          uint32_t *first_row, int *why, uint32_t *member) {
  *why = JA_OK; *member = 0;
  uint64_t rows = 0;
  for (uint32_t k = 0; k < count; ++k) {
    if (first_row) first_row[k] = (uint32_t)(rows < 0xFFFFFFFFull ? rows : 0xFFFFFFFFull);
    rows += mem[k].points;
    if (*why != JA_OK) continue;
    if (mem[k].has_faces) { *why = JA_FACES; *member = k; continue; }
    if (rows > 0xFFFFFFFFull) { *why = JA_ROWS; *member = k; continue; }
    bool same = mem[k].natt == mem[0].natt;
    for (uint32_t a = 0; same && a < mem[k].natt && a < DSA_MAX_ATT; ++a) same = ja_same_attr(mem[k].atts[a], mem[0].atts[a]);
    if (!same) { *why = JA_TABLE; *member = k; }
  }
  const uint32_t num_rows = rows > 0xFFFFFFFFull ? 0u : (uint32_t)rows;
  const uint64_t end = va_layout_mesh(count ? mem[0].atts : nullptr, count ? mem[0].natt : 0u, num_rows, 0, false, format, type_mask, cur, g);
  for (uint32_t a = 0; a < DSA_MAX_ATT; ++a) g.att[a].map_rep = VA_IDENTITY;      // point clouds: point p is entry p
  return end;
}

// ---- the gather, per element
// The row of the joined array point p of a member goes to.
DSA_VA_HD inline uint32_t ja_target_row(const JaMember &M, const uint32_t *rows, uint32_t p) { return rows ? rows[p] : M.first_row + p; }
// Element k of point p's row (k: the dword of a whole-dword row, 0 for a byte row) into row `target` of the group's array; a target
// at or beyond the group's rows writes nothing.
DSA_VA_HD inline void ja_store_element(uint8_t *array, const VaAttr &t, const void *src, uint32_t num_entries, uint32_t num_rows, uint32_t target,
                                       uint32_t k, uint32_t p) {
  if (target >= num_rows) return;
  va_store_element(array, t, src, num_entries, target, k, p);
}

#if defined(__HIPCC__)
namespace dsa {
// k_joined_arrays: grid (chunks of VA_CHUNK points, entry of the member list from `first`), 256 threads, grid-stride inside a member,
// behind the decode on the download stream.  Members are point clouds: point p is entry p, no map is read, so there is no LDS and no
// barrier.  Whole-dword rows take a lane per output dword (in stream order consecutive lanes, consecutive addresses; in input order
// the lanes of one row read the same rows[p]), other rows -- uint8 x 3, int16 x 3: a member's first row in such an array is in
// general not dword aligned -- a lane per row, byte by byte.
__global__ __launch_bounds__(256) void k_joined_arrays(const uint8_t *arena, const MeshLayout *layouts, const MeshDesc *descs, uint32_t n, const JaMember *members,
                                                       uint32_t first, uint32_t num_members, const JaGroup *groups, const uint8_t *rows_base, uint8_t *block) {
  const uint32_t e = first + blockIdx.y;
  if (e >= num_members) return;
  const JaMember M = members[e];
  if (M.mesh >= n) return;
  const MeshDesc *D = &descs[M.mesh];
  if (D->status != ST_OK) return;
  const MeshLayout &L = layouts[M.mesh];
  const JaGroup &T = groups[M.group];
  const uint32_t npts = D->num_points < M.num_points ? D->num_points : M.num_points;
  const uint32_t natt = D->num_attributes < T.cap_attributes ? D->num_attributes : T.cap_attributes;
  const uint32_t *rows = M.rows == JA_NO_ROWS ? nullptr : (const uint32_t *)(rows_base + M.rows);
  for (uint32_t a = 0; a < natt; ++a) {
    const VaAttr &t = T.att[a];
    uint32_t ne = 0;
    if (!va_attr_written(t, D->att[a], L.out_cap[a], L.work_cap[a], &ne)) continue;
    const void *src = t.kind == VA_KIND_QUANTIZED ? (const void *)(arena + L.work[a]) : (const void *)(arena + L.out[a]);
    uint8_t *array = block + t.offset;
    const uint32_t words = va_words(t);
    for (uint32_t p0 = blockIdx.x * VA_CHUNK; p0 < npts; p0 += gridDim.x * VA_CHUNK) {
      const uint32_t count = npts - p0 < VA_CHUNK ? npts - p0 : VA_CHUNK;
      if (words) {
        for (uint32_t i = threadIdx.x; i < count * words; i += blockDim.x) {
          const uint32_t r = i / words, p = p0 + r;
          ja_store_element(array, t, src, ne, T.cap_points, ja_target_row(M, rows, p), i - r * words, p);
        }
      } else if (threadIdx.x < count) {
        const uint32_t p = p0 + threadIdx.x;
        ja_store_element(array, t, src, ne, T.cap_points, ja_target_row(M, rows, p), 0, p);
      }
    }
  }
}
}  // namespace dsa
#endif
