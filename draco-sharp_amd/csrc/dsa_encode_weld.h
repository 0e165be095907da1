// draco-sharp_amd/csrc/dsa_encode_weld.h  (included by dsa_encode_layout.h, behind dsa_encode_repair.h)
//
// Encode direction: the weld of meshes given as one row per point -- a glTF primitive, an OBJ after triangulation,
// Batch.vertex_arrays.  It is synth::weld_points of dsa_encode_host.h on arrays in device memory; tests/hostcheck/encweld_host.cpp
// holds the two against each other.  3 + L key sets per mesh, L = 0 for dsa_encode_points_batch and dsa_weld_batch, L <= 7 for
// dsa_encode_corner_attributes_batch with weld_attributes = 1 (a stream carries corner attributes at its indices 1 to 7) -- the
// vertex (positions, the generic attribute, every listed attribute that stays in the key: what stays per vertex in the stream), the
// normal, the texture coordinate, and L listed attributes each alone -- each the same five steps over the points a face names:
//   k_enc_weld_mark      used[p] = 1 for every point of a face (plain byte stores of one value)
//   k_enc_weld_insert    open addressing over point indices: a table of a power of two >= 2 P slots, 0 = empty, else point + 1;
//                        the hash mixes every word of the key, atomicCAS claims an empty slot, a full comparison of the rows
//                        settles an occupied one, probing is linear.  Slots only ever fill and equal keys probe the same
//                        sequence: a class ends in exactly one slot whatever the arrival order.  The slot keeps the smallest
//                        point of its class (atomicMin; a point that sees a smaller one there already sends none: the value only
//                        falls) -- any point of the class compares alike, so the slot's value may change under a reader.
//   k_enc_weld_scan      a point is its class's representative when its slot holds it; exclusive scan of those flags over the
//                        points in index order, one wave per (mesh, key set): classes numbered by ascending representative
//   k_enc_weld_assign    *_of_point: the number of the representative in the point's slot
//   k_enc_weld_differs   per (mesh, key set behind the vertex's): does any point's row id differ from that of its vertex's
//                        representative
//   k_enc_weld_gather    per (mesh, key set): the welded rows (an attribute no vertex has two rows of: the row of each vertex's
//                        representative) and the faces / corner ids through the maps
// Which thread wins a slot or a minimum decides where a class lies in the table, never a number that leaves the kernels: ranks,
// maps, flags and rows are functions of the class representatives.  Grid: (blocks over points, meshes x `sets`) with `sets` the
// most key sets a mesh of the launch has; a (mesh, set) pair the mesh does not have returns at once (enc_weld_launch).  Indices out
// of range never come here: the host refuses such a mesh before the launch.  P = 0, F = 0, all points equal and all points unused
// run every loop zero or P times and write inside their regions.
#pragma once

namespace dsa {

static const uint32_t EW_MAX_LISTED = 7, EW_MAX_SETS = 3 + EW_MAX_LISTED;
static const uint32_t EW_MAX_SEGS = 20;     // positions, mesh.generic, the attribute list (DSA_MAX_ATTRIBUTES in all), normals, texture coordinates
struct EncWeldSeg { uint64_t src, dst; uint32_t row_bytes, pad; };      // P rows of the caller's; the welded rows
struct EncWeldSet {                // one key set of a mesh
  uint64_t table;                  // u32[cap] slot -> 0, or 1 + the smallest point of the class that claimed it
  uint64_t slot;                   // u32[P] the slot of every used point's class
  uint64_t rank;                   // u32[P] at a representative: the number of its class
  uint64_t of;                     // u32[P] OUTPUT class of every point, DSA_INVALID for an unused one
  uint64_t point;                  // u32[P] OUTPUT representative of every class (`count` of them)
  uint32_t first_seg, num_segs;    // its segments in EncWeld::seg; num_segs 0: the mesh has no such attribute
  uint32_t cap, count;             // count: OUTPUT
};
struct EncWeld {                   // one per mesh; device memory, mirrored on the host
  uint64_t faces, used;            // u32[3F] point of every corner; u8[P]
  uint64_t faces_out;              // u32[3F] OUTPUT vertex of every corner
  uint64_t corners_out[EW_MAX_SETS];       // [k >= 1] u32[3F] OUTPUT row of key set k of every corner (written when differs[k])
  uint32_t differs[EW_MAX_SETS];   // [k >= 1] OUTPUT: some vertex has two rows of key set k
  uint32_t P, F;
  uint32_t num_sets, pad;          // 3 + L
  uint32_t status, detail;
  EncWeldSet set[EW_MAX_SETS];     // vertex, normal, texture coordinate, listed attribute 0 .. L - 1 (num_segs 0: the mesh has no such attribute)
  EncWeldSeg seg[EW_MAX_SEGS];
};
enum { ENC_WELD_OK = 0, ENC_WELD_TABLE_FULL = 1 };
static inline const char *enc_weld_message(uint32_t) { return "weld failed: the point table is full"; }

// The record of a mesh of P points and F faces, its regions from `take(bytes)` (enc_stage_weld; the host check with poisoned gaps),
// in two steps like the arena of a chunk: enc_weld_inputs places what the host uploads -- the faces and the caller's rows, for
// every mesh of the chunk one behind the other, so that the uploads fill one stretch of the arena and nothing else lies in it --
// and enc_weld_regions everything the kernels write, which must start at zero.  vertex_row_bytes[0 .. num_vertex_segs): the rows
// of the vertex key (positions first); listed_row_bytes[0 .. num_listed): the rows of the listed attributes welded alone (none for
// the three-set calls).  Device memory per mesh, before the 256-byte rounding of every region:
//   (24 + 12 a) F + P + (1 + a) (16 P + 4 cap) + 2 R P     a: how many of normals / texture coordinates / listed attributes welded
//   alone the mesh has (0 - 9), R: the bytes of a point's rows in all its arrays, cap: the power of two >= max(2 P, 16), below 4 P.
template <class Take>
static inline EncWeld enc_weld_inputs(Take &&take, uint32_t P, uint32_t F, const uint32_t *vertex_row_bytes, uint32_t num_vertex_segs, bool normals, bool texcoords,
                                      const uint32_t *listed_row_bytes, uint32_t num_listed) {
  EncWeld W;
  memset(&W, 0, sizeof(W));
  W.P = P; W.F = F; W.num_sets = 3u + num_listed;
  W.faces = take(12ull * F);
  uint32_t at = 0;
  for (uint32_t k = 0; k < W.num_sets; ++k) {
    EncWeldSet &S = W.set[k];
    S.first_seg = at;
    S.num_segs = k == 0 ? num_vertex_segs : (k == 1 ? (normals ? 1u : 0u) : (k == 2 ? (texcoords ? 1u : 0u) : 1u));
    for (uint32_t g = 0; g < S.num_segs; ++g, ++at) {
      W.seg[at].row_bytes = k == 0 ? vertex_row_bytes[g] : (k == 1 ? 12u : (k == 2 ? 8u : listed_row_bytes[k - 3u]));
      W.seg[at].src = take((uint64_t)P * W.seg[at].row_bytes);
    }
  }
  return W;
}
template <class Take>
static inline void enc_weld_regions(Take &&take, EncWeld &W) {
  const uint64_t P = W.P, F = W.F;
  W.used = take(P); W.faces_out = take(12ull * F);
  uint32_t cap = 16;
  while (cap < 2ull * P) cap <<= 1;
  for (uint32_t k = 0; k < W.num_sets; ++k) {
    EncWeldSet &S = W.set[k];
    if (S.num_segs == 0) continue;
    for (uint32_t g = 0; g < S.num_segs; ++g) W.seg[S.first_seg + g].dst = take(P * W.seg[S.first_seg + g].row_bytes);
    S.cap = cap;
    S.table = take(4ull * cap); S.slot = take(4ull * P); S.rank = take(4ull * P); S.of = take(4ull * P); S.point = take(4ull * P);
    if (k > 0) W.corners_out[k] = take(12ull * F);
  }
}

// (a relaxed atomic load: the slot may be claimed or lowered by another thread between two looks)
__device__ __forceinline__ uint32_t ew_peek(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ uint32_t ew_hash(const uint8_t *arena, const EncWeldSeg *segs, uint32_t num_segs, uint32_t p) {
  uint32_t h = 0x9E3779B9u;
  for (uint32_t g = 0; g < num_segs; ++g) {
    const uint32_t rb = segs[g].row_bytes;
    const uint8_t *row = arena + segs[g].src + (uint64_t)p * rb;
    if ((rb & 3u) == 0) { const uint32_t *w = (const uint32_t *)row; for (uint32_t k = 0; k < rb / 4u; ++k) { h ^= w[k]; h *= 0x85EBCA6Bu; h ^= h >> 13; } }
    else for (uint32_t k = 0; k < rb; ++k) { h ^= row[k]; h *= 0x01000193u; }
  }
  h ^= h >> 16; h *= 0xC2B2AE35u; h ^= h >> 15;
  return h;
}
__device__ __forceinline__ bool ew_equal(const uint8_t *arena, const EncWeldSeg *segs, uint32_t num_segs, uint32_t p, uint32_t q) {
  for (uint32_t g = 0; g < num_segs; ++g) {
    const uint32_t rb = segs[g].row_bytes;
    const uint8_t *a = arena + segs[g].src + (uint64_t)p * rb, *b = arena + segs[g].src + (uint64_t)q * rb;
    if ((rb & 3u) == 0) { for (uint32_t k = 0; k < rb / 4u; ++k) if (((const uint32_t *)a)[k] != ((const uint32_t *)b)[k]) return false; }
    else for (uint32_t k = 0; k < rb; ++k) if (a[k] != b[k]) return false;
  }
  return true;
}

// blockIdx.y = mesh * sets + key set (k_enc_weld_mark: the mesh alone)
#define ENC_WELD_PROLOGUE(mesh_expr)                                                                \
  const uint32_t mesh = (mesh_expr);                                                                \
  if (mesh >= n) return;                                                                            \
  EncWeld *E = &welds[mesh];                                                                        \
  if (E->status != ENC_WELD_OK) return;                                                             \
  const uint32_t P = E->P, F = E->F, NC = 3u * F;                                                   \
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;       \
  const uint32_t *faces = (const uint32_t *)(arena + E->faces);                                     \
  (void)P; (void)F; (void)NC; (void)t0; (void)stride; (void)faces;

__global__ __launch_bounds__(256) void k_enc_weld_mark(uint8_t *arena, EncWeld *welds, uint32_t n) {
  ENC_WELD_PROLOGUE(blockIdx.y)
  uint8_t *used = arena + E->used;
  for (uint32_t c = t0; c < NC; c += stride) { const uint32_t p = faces[c]; if (p < P) used[p] = 1; }
}

__global__ __launch_bounds__(256) void k_enc_weld_insert(uint8_t *arena, EncWeld *welds, uint32_t n, uint32_t sets) {
  ENC_WELD_PROLOGUE(blockIdx.y / sets)
  const uint32_t k = blockIdx.y % sets;
  if (k >= E->num_sets) return;
  const EncWeldSet &S = E->set[k];
  if (S.num_segs == 0) return;
  const EncWeldSeg *segs = E->seg + S.first_seg;
  const uint8_t *used = arena + E->used;
  uint32_t *table = (uint32_t *)(arena + S.table), *slot = (uint32_t *)(arena + S.slot);
  const uint32_t mask = S.cap - 1u;
  for (uint32_t p = t0; p < P; p += stride) {
    if (!used[p]) continue;
    uint32_t s = ew_hash(arena, segs, S.num_segs, p) & mask, steps = 0;
    for (; steps < S.cap; ++steps, s = (s + 1u) & mask) {
      uint32_t cur = ew_peek(&table[s]);
      if (cur == 0) { cur = atomicCAS(&table[s], 0u, p + 1u); if (cur == 0) break; }
      if (cur - 1u < P && ew_equal(arena, segs, S.num_segs, cur - 1u, p)) { if (p + 1u < cur) atomicMin(&table[s], p + 1u); break; }
    }
    if (steps >= S.cap) { if (atomicCAS(&E->status, 0u, (uint32_t)ENC_WELD_TABLE_FULL) == 0u) E->detail = p; s = 0; }      // (cap >= 2 P: never)
    slot[p] = s;
  }
}

// one wave per (mesh, key set): blockIdx.x = mesh * sets + key set
__global__ __launch_bounds__(WAVE) void k_enc_weld_scan(uint8_t *arena, EncWeld *welds, uint32_t n, uint32_t sets) {
  const uint32_t mesh = blockIdx.x / sets, k = blockIdx.x % sets, lane = threadIdx.x;
  if (mesh >= n) return;
  EncWeld *E = &welds[mesh];
  if (E->status != ENC_WELD_OK || k >= E->num_sets) return;
  EncWeldSet &S = E->set[k];
  if (S.num_segs == 0) return;
  const uint32_t P = E->P;
  const uint8_t *used = arena + E->used;
  const uint32_t *table = (const uint32_t *)(arena + S.table), *slot = (const uint32_t *)(arena + S.slot);
  uint32_t *rank = (uint32_t *)(arena + S.rank), *point = (uint32_t *)(arena + S.point);
  uint32_t base = 0;
#if defined(__HIPCC__)
  for (uint32_t p0 = 0; p0 < P; p0 += WAVE) {
    const uint32_t p = p0 + lane;
    const uint32_t x = (p < P && used[p] && table[slot[p]] == p + 1u) ? 1u : 0u;
    uint32_t incl = x;
    for (int d = 1; d < WAVE; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, WAVE); if ((int)lane >= d) incl += y; }
    if (x) { rank[p] = base + incl - 1u; point[base + incl - 1u] = p; }
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
  if (lane == 0) S.count = base;
#else       // the sanitizer build of tests/hostcheck/encweld_host.cpp runs the lanes of a wave one after the other: lane 0 sums
  if (lane == 0) {
    for (uint32_t p = 0; p < P; ++p) if (used[p] && table[slot[p]] == p + 1u) { rank[p] = base; point[base] = p; ++base; }
    S.count = base;
  }
#endif
}

__global__ __launch_bounds__(256) void k_enc_weld_assign(uint8_t *arena, EncWeld *welds, uint32_t n, uint32_t sets) {
  ENC_WELD_PROLOGUE(blockIdx.y / sets)
  const uint32_t k = blockIdx.y % sets;
  if (k >= E->num_sets) return;
  const EncWeldSet &S = E->set[k];
  if (S.num_segs == 0) return;
  const uint8_t *used = arena + E->used;
  const uint32_t *table = (const uint32_t *)(arena + S.table), *slot = (const uint32_t *)(arena + S.slot), *rank = (const uint32_t *)(arena + S.rank);
  uint32_t *of = (uint32_t *)(arena + S.of);
  for (uint32_t p = t0; p < P; p += stride) of[p] = used[p] ? rank[table[slot[p]] - 1u] : DSA_INVALID;
}

__global__ __launch_bounds__(256) void k_enc_weld_differs(uint8_t *arena, EncWeld *welds, uint32_t n, uint32_t sets) {
  ENC_WELD_PROLOGUE(blockIdx.y / sets)
  const uint32_t k = blockIdx.y % sets;
  if (k == 0 || k >= E->num_sets) return;
  const EncWeldSet &SV = E->set[0], &S = E->set[k];
  if (S.num_segs == 0) return;
  const uint8_t *used = arena + E->used;
  const uint32_t *vtable = (const uint32_t *)(arena + SV.table), *vslot = (const uint32_t *)(arena + SV.slot), *of = (const uint32_t *)(arena + S.of);
  bool differs = false;
  for (uint32_t p = t0; p < P; p += stride) if (used[p] && of[p] != of[vtable[vslot[p]] - 1u]) differs = true;
  if (differs) E->differs[k] = 1u;             // (every writer stores the same value)
}

__device__ __forceinline__ void ew_copy_row(uint8_t *arena, const EncWeldSeg &g, uint32_t to, uint32_t from) {
  const uint32_t rb = g.row_bytes;
  const uint8_t *a = arena + g.src + (uint64_t)from * rb;
  uint8_t *b = arena + g.dst + (uint64_t)to * rb;
  if ((rb & 3u) == 0) for (uint32_t k = 0; k < rb / 4u; ++k) ((uint32_t *)b)[k] = ((const uint32_t *)a)[k];
  else for (uint32_t k = 0; k < rb; ++k) b[k] = a[k];
}
// key set 0: the faces and the rows of the vertex key; key set k >= 1: its rows (no vertex has two: the row of each vertex's
// representative) and, where some vertex has two, the ids of every corner
__global__ __launch_bounds__(256) void k_enc_weld_gather(uint8_t *arena, EncWeld *welds, uint32_t n, uint32_t sets) {
  ENC_WELD_PROLOGUE(blockIdx.y / sets)
  const uint32_t k = blockIdx.y % sets;
  if (k >= E->num_sets) return;
  const EncWeldSet &SV = E->set[0];
  const uint32_t V = SV.count;
  const uint32_t *vof = (const uint32_t *)(arena + SV.of), *vpoint = (const uint32_t *)(arena + SV.point);
  if (k == 0) {
    uint32_t *faces_out = (uint32_t *)(arena + E->faces_out);
    for (uint32_t c = t0; c < NC; c += stride) faces_out[c] = vof[faces[c]];
    for (uint32_t g = 0; g < SV.num_segs; ++g)
      for (uint32_t v = t0; v < V; v += stride) ew_copy_row(arena, E->seg[SV.first_seg + g], v, vpoint[v]);
    return;
  }
  const EncWeldSet &S = E->set[k];
  if (S.num_segs == 0) return;
  const bool seamed = E->differs[k] != 0;
  const uint32_t *of = (const uint32_t *)(arena + S.of), *point = seamed ? (const uint32_t *)(arena + S.point) : vpoint;
  const uint32_t rows = seamed ? S.count : V;
  for (uint32_t r = t0; r < rows; r += stride) ew_copy_row(arena, E->seg[S.first_seg], r, point[r]);
  if (!seamed) return;
  uint32_t *corners = (uint32_t *)(arena + E->corners_out[k]);
  for (uint32_t c = t0; c < NC; c += stride) corners[c] = of[faces[c]];
}

// The six steps over `nr` records whose meshes have at most `sets` key sets: launch(kernel, grid x, grid y, block, arguments...) is
// hipLaunchKernelGGL on the lane's stream in enc_stage_weld and the thread-by-thread loop in the host check.  Grid y is meshes x
// key sets, in slices of at most max_grid_y rows (a mesh's steps read its own record and regions only, so slices are independent).
template <class Launch>
static inline void enc_weld_launch(Launch &&launch, uint8_t *arena, EncWeld *recs, uint32_t nr, uint32_t sets, uint32_t gx, uint32_t max_grid_y = 65535u) {
  const uint32_t per = max_grid_y / sets > 1u ? max_grid_y / sets : 1u;
  for (uint32_t r0 = 0; r0 < nr; r0 += per) {
    EncWeld *welds = recs + r0;
    const uint32_t cnt = nr - r0 < per ? nr - r0 : per;
    launch(k_enc_weld_mark, gx, cnt, 256u, arena, welds, cnt);
    launch(k_enc_weld_insert, gx, sets * cnt, 256u, arena, welds, cnt, sets);
    launch(k_enc_weld_scan, sets * cnt, 1u, (uint32_t)WAVE, arena, welds, cnt, sets);
    launch(k_enc_weld_assign, gx, sets * cnt, 256u, arena, welds, cnt, sets);
    launch(k_enc_weld_differs, gx, sets * cnt, 256u, arena, welds, cnt, sets);
    launch(k_enc_weld_gather, gx, sets * cnt, 256u, arena, welds, cnt, sets);
  }
}

}  // namespace dsa
