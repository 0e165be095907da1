// draco-sharp_amd/csrc/dsa_vertex_arrays.h
// Vertex arrays (dsa_batch_vertex_arrays): the results of a decoded batch as a consumer draws them -- per mesh one index array and
// per attribute one array with a row per POINT, gathered on the device through the point maps, so that no map crosses the link.
// Three parts: the layout of the block (sized from what the host parse knows, like the packed block of a compact download), the
// body of the gather as plain functions over raw pointers, and k_vertex_arrays, which calls them per element.  The first two
// compile without HIP: tests/hostcheck/varrays_host.cpp runs them under the sanitizers.
#pragma once
#include <stdint.h>

#include "dsa_types.h"

#if defined(__HIPCC__)
#define DSA_VA_HD __host__ __device__
#else
#define DSA_VA_HD
#endif

#define VA_FORMAT_VALUES 0      // == DSA_VA_VALUES: rows are the decoded values, byte_stride bytes
#define VA_FORMAT_QUANTIZED 1   // == DSA_VA_QUANTIZED: quantised attributes (seq_type 2 / 3) as uint16 rows of portable integers
#define VA_NONE (~0ull)         // an array that is not in the block
#define VA_IDENTITY 0xFFu       // VaAttr::map_rep: point i = entry i, no map is read
#define VA_KIND_VALUES 0u
#define VA_KIND_QUANTIZED 1u
#define VA_CHUNK 256u           // points a block of k_vertex_arrays gathers per turn (= its threads)

// Where one attribute's rows go, and how they are made.
struct VaAttr {
  uint64_t offset;      // inside the block, 64-byte aligned; VA_NONE: left out (attribute mask)
  uint32_t stride;      // bytes per point
  uint8_t kind;         // VA_KIND_*
  uint8_t map_rep;      // the first attribute of the mesh that is decoded in this attribute's order: its map serves both; VA_IDENTITY
  uint8_t nc;           // components stored per row
  uint8_t data_type;    // Draco DataType of the stored elements
};
// One mesh of the block: the table the host hands k_vertex_arrays.
struct VaMesh {
  uint64_t indices;     // VA_NONE: a point cloud
  uint32_t u16;         // indices stored as uint16 (the CompactMesh::u16 rule)
  uint32_t cap_points, cap_faces, cap_attributes;
  VaAttr att[DSA_MAX_ATT];
};

// What the sizing needs to know about an attribute: the fixed part of its header.
struct VaAttrIn { uint8_t att_type, data_type, nc, seq_type; uint8_t map_rep; };

DSA_VA_HD inline uint32_t va_dt_len(uint32_t dt) {
  switch (dt) { case 1: case 2: case 11: return 1; case 3: case 4: return 2; case 5: case 6: case 9: return 4; case 7: case 8: case 10: return 8; default: return 0; }
}
DSA_VA_HD inline uint64_t va_align(uint64_t v) { return (v + 63) & ~63ull; }
// Indices are uint16 while every point id of the mesh fits: decided from the header's counts, for the compact download too.
DSA_VA_HD inline uint32_t va_indices_u16(uint32_t cap_points) { return cap_points <= 65536u ? 1u : 0u; }
DSA_VA_HD inline bool va_quantised(uint32_t seq_type) { return seq_type == 2 || seq_type == 3; }
// portable components of a quantised attribute: octahedral normals carry two
DSA_VA_HD inline uint32_t va_portable_nc(uint32_t seq_type, uint32_t nc) { return seq_type == 3 ? 2u : nc; }

// Places the arrays of one mesh behind `cur` (offset inside the block) and returns the new end.  A function of the headers only:
// nothing here waits for the decode.  type_mask: bit t = attributes of GeometryAttributeType t are wanted, 0 = all.
DSA_VA_HD inline uint64_t va_layout_mesh(const VaAttrIn *atts, uint32_t natt, uint32_t cap_points, uint32_t cap_faces, bool has_faces, int format,
                                         uint32_t type_mask, uint64_t cur, VaMesh &m) {
  m.u16 = va_indices_u16(cap_points);
  m.cap_points = cap_points; m.cap_faces = cap_faces; m.cap_attributes = natt < DSA_MAX_ATT ? natt : DSA_MAX_ATT;
  m.indices = VA_NONE;
  if (has_faces) { m.indices = cur; cur = va_align(cur + (uint64_t)cap_faces * (m.u16 ? 6u : 12u)); }
  for (uint32_t a = 0; a < DSA_MAX_ATT; ++a) {
    VaAttr &t = m.att[a];
    t.offset = VA_NONE; t.stride = 0; t.kind = VA_KIND_VALUES; t.map_rep = VA_IDENTITY; t.nc = 0; t.data_type = 0;
    if (a >= m.cap_attributes) continue;
    const VaAttrIn &A = atts[a];
    t.map_rep = A.map_rep;
    if (format == VA_FORMAT_QUANTIZED && va_quantised(A.seq_type)) {
      t.kind = VA_KIND_QUANTIZED; t.nc = (uint8_t)va_portable_nc(A.seq_type, A.nc); t.data_type = 4;
      t.stride = (2u * t.nc + 3u) & ~3u;                                  // whole dwords, zero filled
    } else {
      t.nc = A.nc; t.data_type = A.data_type; t.stride = va_dt_len(A.data_type) * A.nc;
    }
    if (type_mask != 0 && !(A.att_type < 32 && ((type_mask >> A.att_type) & 1u))) continue;      // reserves nothing
    if (t.stride == 0) continue;
    t.offset = cur;
    cur = va_align(cur + (uint64_t)t.stride * cap_points);
  }
  return cur;
}

// ---- the gather, per element
// Word w of the index array of a mesh with nc corners stored as uint16: two corners to a word (k_pack_output and k_vertex_arrays).
DSA_VA_HD inline uint32_t va_index_pair(const int32_t *faces, uint32_t w, uint32_t nc) {
  const uint32_t lo = (uint32_t)faces[2 * w], hi = 2 * w + 1 < nc ? (uint32_t)faces[2 * w + 1] : 0u;
  return (lo & 0xFFFFu) | (hi << 16);
}
// Dword k of the row of `entry` in an array of num_entries rows of `words` dwords.  An entry that is not in the array gives zero
// and reads nothing.
DSA_VA_HD inline uint32_t va_value_word(const uint32_t *src, uint32_t entry, uint32_t num_entries, uint32_t words, uint32_t k) {
  return entry < num_entries ? src[(uint64_t)entry * words + k] : 0u;
}
// The same for rows that are no whole dwords (uint8 x 1 / 3, int16 x 3 ...): the whole row, byte by byte.
DSA_VA_HD inline void va_value_row(uint8_t *dst, const uint8_t *src, uint32_t entry, uint32_t num_entries, uint32_t stride) {
  if (entry < num_entries) { const uint8_t *row = src + (uint64_t)entry * stride; for (uint32_t i = 0; i < stride; ++i) dst[i] = row[i]; }
  else for (uint32_t i = 0; i < stride; ++i) dst[i] = 0;
}
// Dword k of a quantised row: portable components 2k and 2k + 1 of `entry` narrowed to uint16, zero behind the last component.
DSA_VA_HD inline uint32_t va_quantised_word(const int32_t *portable, uint32_t entry, uint32_t num_entries, uint32_t ncp, uint32_t k) {
  if (entry >= num_entries) return 0u;
  const int32_t *row = portable + (uint64_t)entry * ncp;
  const uint32_t lo = 2 * k < ncp ? (uint32_t)row[2 * k] & 0xFFFFu : 0u, hi = 2 * k + 1 < ncp ? (uint32_t)row[2 * k + 1] & 0xFFFFu : 0u;
  return lo | (hi << 16);
}
// Elements an attribute's array has for `points` points: one per dword where rows are whole dwords, else one per row.
DSA_VA_HD inline uint32_t va_words(const VaAttr &t) { return (t.stride & 3u) == 0 ? t.stride / 4u : 0u; }
// Element e of `count` points starting at point p0: its row is p0 + e / words (word rows) or p0 + e (byte rows); `entry` is that
// row's entry.  src: the attribute's decoded values (VA_KIND_VALUES) or its int32 portable values (VA_KIND_QUANTIZED).
DSA_VA_HD inline void va_store_element(uint8_t *array, const VaAttr &t, const void *src, uint32_t num_entries, uint32_t point, uint32_t k, uint32_t entry) {
  const uint32_t words = va_words(t);
  if (words == 0) { va_value_row(array + (uint64_t)point * t.stride, (const uint8_t *)src, entry, num_entries, t.stride); return; }
  uint32_t *dst = (uint32_t *)(array + (uint64_t)point * t.stride) + k;
  *dst = t.kind == VA_KIND_QUANTIZED ? va_quantised_word((const int32_t *)src, entry, num_entries, t.nc, k)
                                     : va_value_word((const uint32_t *)src, entry, num_entries, words, k);
}
// Whether the decoded attribute is what the table laid out (the layout is made from the host's parse of the same header; an
// attribute quantised with more than 16 bits has no uint16 rows: its array stays unwritten and the layout reports it absent), and
// how many of its entries may be read: never more than the capacity of the region they were decoded into.
DSA_VA_HD inline bool va_attr_written(const VaAttr &t, const AttrDesc &A, uint32_t out_cap_bytes, uint32_t work_cap_elems, uint32_t *num_entries) {
  if (t.offset == VA_NONE || t.stride == 0) return false;
  if (t.kind == VA_KIND_QUANTIZED) {
    if (!va_quantised(A.seq_type) || A.nc_portable != t.nc || A.q_bits > 16 || A.source == SRC_BYTES) return false;
    const uint32_t cap = work_cap_elems / t.nc;
    *num_entries = A.num_entries < cap ? A.num_entries : cap;
    return true;
  }
  if (va_dt_len(A.data_type) * A.nc != t.stride) return false;
  const uint32_t cap = out_cap_bytes / t.stride;
  *num_entries = A.num_entries < cap ? A.num_entries : cap;
  return true;
}

#if defined(__HIPCC__)
namespace dsa {
// k_vertex_arrays: grid (chunks of points, mesh), 256 threads, grid-stride inside a mesh -- the shape of k_pack_output, behind the
// decode on the download stream.  Per turn a block takes VA_CHUNK points: every distinct map of the mesh is read once per point
// (a lane per point, the entries parked in LDS), then every attribute decoded in that order stores its rows of the chunk with a
// lane per output dword -- consecutive lanes, consecutive addresses -- or, for rows that are no whole dwords, a lane per row.  The
// gathered loads stay in L2: the value array of a mesh is a few hundred kilobytes and the maps are nearly sorted.
__global__ __launch_bounds__(256) void k_vertex_arrays(const uint8_t *arena, const MeshLayout *layouts, const MeshDesc *descs, uint32_t n, const VaMesh *table,
                                                       uint8_t *block) {
  __shared__ uint32_t s_entry[VA_CHUNK];
  const uint32_t mesh = blockIdx.y;
  if (mesh >= n) return;
  const MeshDesc *D = &descs[mesh];
  if (D->status != ST_OK) return;
  const MeshLayout &L = layouts[mesh];
  const VaMesh &T = table[mesh];
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const uint32_t nf = D->num_faces < T.cap_faces ? D->num_faces : T.cap_faces, nc = 3u * nf;
  const uint32_t npts = D->num_points < T.cap_points ? D->num_points : T.cap_points;
  if (T.indices != VA_NONE) {
    const int32_t *faces = (const int32_t *)(arena + L.faces);
    if (T.u16) {
      uint32_t *dst = (uint32_t *)(block + T.indices);
      for (uint32_t w = tid; w < (nc + 1) / 2; w += stride) dst[w] = va_index_pair(faces, w, nc);
    } else {
      int32_t *dst = (int32_t *)(block + T.indices);
      for (uint32_t i = tid; i < nc; i += stride) dst[i] = faces[i];
    }
  }
  const uint32_t natt = D->num_attributes < T.cap_attributes ? D->num_attributes : T.cap_attributes;
  for (uint32_t g = 0; g < natt; ++g) {
    const uint32_t rep = T.att[g].map_rep;
    if (rep != g && rep != VA_IDENTITY) continue;                    // served by the turn of its representative
    const uint32_t *map = rep == VA_IDENTITY ? nullptr : (const uint32_t *)(arena + L.map[g]);
    for (uint32_t p0 = blockIdx.x * VA_CHUNK; p0 < npts; p0 += gridDim.x * VA_CHUNK) {      // (uniform per block: the barriers are safe)
      const uint32_t count = npts - p0 < VA_CHUNK ? npts - p0 : VA_CHUNK;
      if (threadIdx.x < count) s_entry[threadIdx.x] = map ? map[p0 + threadIdx.x] : p0 + threadIdx.x;
      __syncthreads();
      for (uint32_t a = g; a < natt; ++a) {
        const VaAttr &t = T.att[a];
        if (a != g && (rep == VA_IDENTITY || t.map_rep != g)) continue;
        uint32_t ne = 0;
        if (!va_attr_written(t, D->att[a], L.out_cap[a], L.work_cap[a], &ne)) continue;
        const void *src = t.kind == VA_KIND_QUANTIZED ? (const void *)(arena + L.work[a]) : (const void *)(arena + L.out[a]);
        uint8_t *array = block + t.offset;
        const uint32_t words = va_words(t);
        if (words) {
          for (uint32_t e = threadIdx.x; e < count * words; e += blockDim.x) {
            const uint32_t row = e / words;
            va_store_element(array, t, src, ne, p0 + row, e - row * words, s_entry[row]);
          }
        } else if (threadIdx.x < count) va_store_element(array, t, src, ne, p0 + threadIdx.x, 0, s_entry[threadIdx.x]);
      }
      __syncthreads();
    }
  }
}
}  // namespace dsa
#endif
