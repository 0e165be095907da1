// draco-sharp_amd/csrc/dsa_encode_weld_list.h  (included by dsa_encode_layout.h, behind dsa_encode_weld.h)
//
// Encode direction: the weld of meshes given as one row per point with every listed attribute a key set of its own
// (dsa_encode_corner_attributes_batch, weld_attributes = 1).  It is synth::weld_points of dsa_encode_host.h with `listed` segments on
// arrays in device memory; tests/hostcheck/encweldlist_host.cpp holds the two against each other.  3 + L key sets per mesh -- the
// vertex (positions, the generic attribute, the listed attributes that stay in the key), the normal, the texture coordinate, and
// L <= 7 listed attributes each alone (a stream carries corner attributes at its indices 1 to 7) -- each the five steps of
// dsa_encode_weld.h, whose hash, comparison, row copy and records of a set (EncWeldSet, EncWeldSeg) are used as they are:
//   k_enc_wlist_mark      used[p] = 1 for every point of a face
//   k_enc_wlist_insert    open addressing over point indices, per (mesh, key set): atomicCAS claims an empty slot, a full comparison
//                         of the rows settles an occupied one, atomicMin keeps the smallest point of the class in the slot
//   k_enc_wlist_scan      classes numbered by ascending representative, one wave per (mesh, key set)
//   k_enc_wlist_assign    *_of_point
//   k_enc_wlist_differs   per (mesh, key set behind the vertex's): does any point's row id differ from that of its vertex's representative
//   k_enc_wlist_gather    the welded rows, the faces and the corner ids through the maps, per (mesh, key set)
// Which thread wins a slot or a minimum decides where a class lies in the table, never a number that leaves the kernels: slots only
// ever fill, equal keys probe the same sequence, so a class ends in exactly one slot whatever the arrival order; its slot ends at
// the smallest point of the class; ranks, maps, flags and rows are functions of those.  Grid: (blocks over points, meshes x `sets`)
// with `sets` the most key sets a mesh of the launch has; a (mesh, set) pair the mesh does not have returns at once.  Indices out
// of range never come here: the host refuses such a mesh before the launch.  P = 0, F = 0, all points equal and all points unused
// run every loop zero or P times and write inside their regions.
#pragma once

namespace dsa {

static const uint32_t EWL_MAX_LISTED = 7, EWL_MAX_SETS = 3 + EWL_MAX_LISTED;
struct EncWeldList {               // one per mesh; device memory, mirrored on the host
  uint64_t faces, used;            // u32[3F] point of every corner; u8[P]
  uint64_t faces_out;              // u32[3F] OUTPUT vertex of every corner
  uint64_t corners_out[EWL_MAX_SETS];      // [k >= 1] u32[3F] OUTPUT row of key set k of every corner (written when differs[k])
  uint32_t differs[EWL_MAX_SETS];  // [k >= 1] OUTPUT: some vertex has two rows of key set k
  uint32_t P, F;
  uint32_t num_sets, pad;          // 3 + L
  uint32_t status, detail;
  EncWeldSet set[EWL_MAX_SETS];    // vertex, normal, texture coordinate, listed attribute 0 .. L - 1 (num_segs 0: the mesh has no such attribute)
  EncWeldSeg seg[EW_MAX_SEGS];
};

// The record of a mesh, in the two steps of enc_weld_inputs / enc_weld_regions.  vertex_row_bytes[0 .. num_vertex_segs): the rows of
// the vertex key (positions first); listed_row_bytes[0 .. num_listed): the rows of the listed attributes welded alone.  Device
// memory per mesh, before the 256-byte rounding of every region:
//   (24 + 12 a) F + P + (1 + a) (16 P + 4 cap) + 2 R P     a: how many of normals / texture coordinates / listed attributes welded
//   alone the mesh has (0 - 9), R: the bytes of a point's rows in all its arrays, cap: the power of two >= max(2 P, 16), below 4 P.
template <class Take>
static inline EncWeldList enc_wlist_inputs(Take &&take, uint32_t P, uint32_t F, const uint32_t *vertex_row_bytes, uint32_t num_vertex_segs, bool normals, bool texcoords,
                                           const uint32_t *listed_row_bytes, uint32_t num_listed) {
  EncWeldList W;
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
static inline void enc_wlist_regions(Take &&take, EncWeldList &W) {
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

// blockIdx.y = mesh * sets + key set (k_enc_wlist_mark: the mesh alone)
#define ENC_WLIST_PROLOGUE(mesh_expr)                                                               \
  const uint32_t mesh = (mesh_expr);                                                                \
  if (mesh >= n) return;                                                                            \
  EncWeldList *E = &welds[mesh];                                                                    \
  if (E->status != ENC_WELD_OK) return;                                                             \
  const uint32_t P = E->P, F = E->F, NC = 3u * F;                                                   \
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;       \
  const uint32_t *faces = (const uint32_t *)(arena + E->faces);                                     \
  (void)P; (void)F; (void)NC; (void)t0; (void)stride; (void)faces;

__global__ __launch_bounds__(256) void k_enc_wlist_mark(uint8_t *arena, EncWeldList *welds, uint32_t n) {
  ENC_WLIST_PROLOGUE(blockIdx.y)
  uint8_t *used = arena + E->used;
  for (uint32_t c = t0; c < NC; c += stride) { const uint32_t p = faces[c]; if (p < P) used[p] = 1; }
}

__global__ __launch_bounds__(256) void k_enc_wlist_insert(uint8_t *arena, EncWeldList *welds, uint32_t n, uint32_t sets) {
  ENC_WLIST_PROLOGUE(blockIdx.y / sets)
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
__global__ __launch_bounds__(WAVE) void k_enc_wlist_scan(uint8_t *arena, EncWeldList *welds, uint32_t n, uint32_t sets) {
  const uint32_t mesh = blockIdx.x / sets, k = blockIdx.x % sets, lane = threadIdx.x;
  if (mesh >= n) return;
  EncWeldList *E = &welds[mesh];
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
#else       // the sanitizer build of tests/hostcheck/encweldlist_host.cpp runs the lanes of a wave one after the other: lane 0 sums
  if (lane == 0) {
    for (uint32_t p = 0; p < P; ++p) if (used[p] && table[slot[p]] == p + 1u) { rank[p] = base; point[base] = p; ++base; }
    S.count = base;
  }
#endif
}

__global__ __launch_bounds__(256) void k_enc_wlist_assign(uint8_t *arena, EncWeldList *welds, uint32_t n, uint32_t sets) {
  ENC_WLIST_PROLOGUE(blockIdx.y / sets)
  const uint32_t k = blockIdx.y % sets;
  if (k >= E->num_sets) return;
  const EncWeldSet &S = E->set[k];
  if (S.num_segs == 0) return;
  const uint8_t *used = arena + E->used;
  const uint32_t *table = (const uint32_t *)(arena + S.table), *slot = (const uint32_t *)(arena + S.slot), *rank = (const uint32_t *)(arena + S.rank);
  uint32_t *of = (uint32_t *)(arena + S.of);
  for (uint32_t p = t0; p < P; p += stride) of[p] = used[p] ? rank[table[slot[p]] - 1u] : DSA_INVALID;
}

__global__ __launch_bounds__(256) void k_enc_wlist_differs(uint8_t *arena, EncWeldList *welds, uint32_t n, uint32_t sets) {
  ENC_WLIST_PROLOGUE(blockIdx.y / sets)
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

// key set 0: the faces and the rows of the vertex key; key set k >= 1: its rows (no vertex has two: the row of each vertex's
// representative) and, where some vertex has two, the ids of every corner
__global__ __launch_bounds__(256) void k_enc_wlist_gather(uint8_t *arena, EncWeldList *welds, uint32_t n, uint32_t sets) {
  ENC_WLIST_PROLOGUE(blockIdx.y / sets)
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

}  // namespace dsa
