// draco-sharp_amd/csrc/dsa_encode_repair.h  (included by dsa_encode.h, behind dsa_encode_conn.h)
//
// Encode direction: the reference's corner table for meshes the connectivity kernels refuse -- degenerate faces, the same face
// twice, fins, faces turned over, fans that meet at a vertex, vertices no face uses (dsa_encode_repair_batch, topology = 1).
//   CornerTable.cs:28-43   ComputeOppositeCorners (:298-394, with the scan over the whole pending list that the loop header of
//                          :346 lost), BreakNonManifoldEdges (:396-469), ComputeVertexCorners (:471-547)
// It is synth::CornerTable::repair of dsa_encode_host.h on arrays in device memory; tests/hostcheck/encrepair_host.cpp holds the
// two against each other.  What comes out per mesh: c2v' (a fan behind the first of its vertex carries a new vertex V, V + 1, ...),
// the opposites, the parent of every new vertex and the counts (V', isolated, degenerate, edges cut).  The host counts the
// degenerate faces and the isolated vertices out and lays the mesh out at its real size; from there it takes the kernels of
// dsa_encode_conn.h like any other mesh, its opposites given (k_enc_table_opposites would join edges the repair cut) and its value
// rows read through the row of every vertex (k_enc_repair_rows).  Clean meshes never come here.
// Attributes given per corner (dsa_encode_seam_repair_batch, corner_repair = 1) come along: their ids go up with the faces,
// k_enc_repair_face_scan / k_enc_repair_ids leave the ids of the coded faces on the device, in the width the layout takes them, and
// enc_stage_uploads copies them into the chunk's arena; the seam kernels (dsa_encode_seams.h) then run over the repaired chunk.
//
// Grid-parallel (blocks per mesh x meshes): the marks of degenerate faces, corners by vertex, the matching, the isolated count.
//   The half-edges of one undirected edge interact with no others: the thread of the edge's first corner replays the edge's queue
//   in corner order -- the pending entries the sequential pass would keep at the two end points, earliest first.
// One lane per mesh, several meshes to a wave, like the walks of k_enc_connectivity: the break pass and the fan pass, which decide
//   every step from what the steps before left.  The break pass asks "did an edge of this fan reach that vertex already" of a
//   stamp per vertex (the fan, and the first two edge corners that reached it: the reference's list scan cuts at the first entry
//   that is not the opposite, which is the first or the second), not of a list: a fan of valence 60 000 is 60 000 steps, not 1.8e9.
// Every loop is bounded by a count derived from F; a mesh that exhausts it fails alone (ENC_REPAIR_BOUND: the same face listed
// thousands of times makes the replay of one edge quadratic).  No array lives in a lane's private memory: everything the passes
// keep is in the mesh's regions, every step is loads and stores the lanes of a wave issue together.
#pragma once

namespace dsa {

struct EncRepair {                 // one per mesh; device memory, mirrored on the host
  uint64_t faces;                  // u32[3F] input: vertex of every corner
  uint64_t c2v;                    // u32[3F] OUTPUT c2v'
  uint64_t opp;                    // u32[3F] OUTPUT opposite corner or INVALID
  uint64_t parent;                 // u32[3F] OUTPUT parent of vertex V + k (V' - V of them)
  uint64_t voff, vcur, vlist;      // u32[V+1], u32[V], u32[3F]: corners of the faces that are not degenerate, by vertex
  uint64_t pend;                   // u8[3F] matching: 1 the corner waits for its opposite
  uint64_t bvis, cvis;             // u8[3F] each: visited marks of the break pass (kept from sweep to sweep) and of the fan pass; 1 from the start for a degenerate face
  uint64_t vvis;                   // u8[V] fan pass: the vertex has its first fan
  uint64_t stamp;                  // u32[3V] break pass, per vertex: the fan that reached it last, the first and the second edge corner that did
  uint32_t F, V;
  uint32_t num_vertices, isolated, degenerate, breaks;     // OUTPUT
  uint32_t status, detail;
  // attributes given per corner over the repaired table (dsa_encode_seam_repair_batch, corner_repair = 1; 0 / unset otherwise)
  uint64_t fmap;                   // u32[F] OUTPUT of k_enc_repair_face_scan: the coded index of a source face, INVALID for a degenerate one
  uint32_t coded_faces, pad;       // OUTPUT: F - degenerate, as the scan counted them
};
enum { ENC_REPAIR_OK = 0, ENC_REPAIR_BOUND = 1 };
static inline const char *enc_repair_message(uint32_t status) {
  return status == ENC_REPAIR_BOUND ? "topology repair: step bound exhausted (a face listed thousands of times?)" : "topology repair failed";
}
__device__ __forceinline__ void er_fail(EncRepair *E, uint32_t status, uint32_t detail) { if (atomicCAS(&E->status, 0u, status) == 0u) E->detail = detail; }

#define ENC_REPAIR_PROLOGUE                                                                         \
  const uint32_t mesh = blockIdx.y;                                                                 \
  if (mesh >= n) return;                                                                            \
  EncRepair *E = &reps[mesh];                                                                       \
  if (E->status != ENC_REPAIR_OK) return;                                                           \
  const uint32_t F = E->F, V = E->V, NC = 3u * F;                                                   \
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;       \
  const uint32_t *faces = (const uint32_t *)(arena + E->faces);                                     \
  (void)F; (void)V; (void)NC; (void)t0; (void)stride; (void)faces;

// c2v' starts as the faces, no corner has an opposite; degenerate faces are marked (their corners count as visited in both
// serial passes and take no part in anything) and counted; corners per vertex (voff[v + 1], the faces that are not degenerate)
__global__ __launch_bounds__(256) void k_enc_repair_mark(uint8_t *arena, EncRepair *reps, uint32_t n) {
  ENC_REPAIR_PROLOGUE
  uint32_t *c2v = (uint32_t *)(arena + E->c2v), *opp = (uint32_t *)(arena + E->opp), *voff = (uint32_t *)(arena + E->voff);
  uint8_t *bvis = arena + E->bvis, *cvis = arena + E->cvis;
  uint32_t degenerate = 0;
  for (uint32_t f = t0; f < F; f += stride) {
    const uint32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool deg = a == b || a == c || b == c;
    for (uint32_t k = 0; k < 3; ++k) { c2v[3 * f + k] = faces[3 * f + k]; opp[3 * f + k] = DSA_INVALID; bvis[3 * f + k] = cvis[3 * f + k] = deg ? 1 : 0; }
    if (deg) { ++degenerate; continue; }
    atomicAdd(&voff[a + 1], 1u); atomicAdd(&voff[b + 1], 1u); atomicAdd(&voff[c + 1], 1u);
  }
  if (degenerate) atomicAdd(&E->degenerate, degenerate);
}

// ---- attributes given per corner over a repaired table: the ids of the coded faces.  The table the layout takes has the
// degenerate faces counted out (CornerTable::from_repaired: the source's other faces in source order), so the id of source corner
// 3f + k belongs at 3f' + k.  The scan: one wave per mesh over the marks k_enc_repair_mark left (bvis of a face's first corner;
// launched before the break pass, which marks what it visits), 64 faces a round by ballot.  Then one thread per source corner of
// every (mesh, attribute with ids) record: the id checked against the attribute's row count (the host coder's "id out of range",
// degenerate faces included) and stored narrow or wide by the layout's rule (EncChunk::ids_narrow: rows <= 65 536 -> u16).
struct EncRepairIds {              // one per (mesh, attribute with ids); device memory, mirrored on the host
  uint64_t src;                    // u32[3F] input: the caller's id per source corner
  uint64_t dst;                    // u16[3F'] / u32[3F'] OUTPUT (room for 3F)
  uint32_t rep;                    // the mesh's EncRepair
  uint32_t rows, narrow;           // value rows of the attribute; 1: u16 output
  uint32_t att_type;               // 1 normals, 3 texture coordinates, 0x100 + k attribute k of the list (which message a bad id earns)
  uint32_t bad, pad;               // OUTPUT: 1 an id is not below `rows`
};
__global__ __launch_bounds__(WAVE) void k_enc_repair_face_scan(uint8_t *arena, EncRepair *reps, uint32_t n) {
  const uint32_t mesh = blockIdx.x, lane = threadIdx.x;
  if (mesh >= n) return;
  EncRepair *E = &reps[mesh];
  if (E->status != ENC_REPAIR_OK || !E->fmap) return;
  const uint32_t F = E->F;
  const uint8_t *bvis = arena + E->bvis;
  uint32_t *fmap = (uint32_t *)(arena + E->fmap);
  uint32_t base = 0;
#if defined(__HIPCC__)
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t f0 = 0; f0 < F; f0 += WAVE) {
    const uint32_t f = f0 + lane;
    const bool kept = f < F && bvis[3u * f] == 0;
    const uint64_t km = __ballot(kept);
    if (f < F) fmap[f] = kept ? base + (uint32_t)__popcll(km & below) : DSA_INVALID;
    base += (uint32_t)__popcll(km);
  }
#else       // the sanitizer build of tests/hostcheck runs the lanes of a wave one after the other: lane 0 counts
  if (lane == 0) for (uint32_t f = 0; f < F; ++f) fmap[f] = bvis[3u * f] == 0 ? base++ : DSA_INVALID;
#endif
  if (lane == 0) E->coded_faces = base;
}
__global__ __launch_bounds__(256) void k_enc_repair_ids(uint8_t *arena, const EncRepair *reps, EncRepairIds *ids, uint32_t n) {
  const uint32_t r = blockIdx.y;
  if (r >= n) return;
  EncRepairIds *I = &ids[r];
  const EncRepair *E = &reps[I->rep];
  if (E->status != ENC_REPAIR_OK || !E->fmap) return;
  const uint32_t NC = 3u * E->F, rows = I->rows;
  const uint32_t *fmap = (const uint32_t *)(arena + E->fmap), *src = (const uint32_t *)(arena + I->src);
  uint16_t *dst16 = (uint16_t *)(arena + I->dst);
  uint32_t *dst32 = (uint32_t *)(arena + I->dst);
  const bool narrow = I->narrow != 0;
  bool bad = false;
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < NC; c += gridDim.x * blockDim.x) {
    const uint32_t id = src[c], f = c / 3u, to = fmap[f];
    if (id >= rows) { bad = true; continue; }
    if (to == DSA_INVALID) continue;
    const uint32_t at = 3u * to + (c - 3u * f);                // (to < F' <= F: inside the room for 3F)
    if (narrow) dst16[at] = (uint16_t)id; else dst32[at] = id;
  }
  if (bad) I->bad = 1;                                         // (every writer stores the same word)
}

// exclusive prefix sum, one wave per mesh (k_enc_table_offsets on these records); a vertex without a corner is isolated
__global__ __launch_bounds__(WAVE) void k_enc_repair_offsets(uint8_t *arena, EncRepair *reps, uint32_t n) {
  const uint32_t mesh = blockIdx.x, lane = threadIdx.x;
  if (mesh >= n) return;
  EncRepair *E = &reps[mesh];
  if (E->status != ENC_REPAIR_OK) return;
  const uint32_t V = E->V;
  uint32_t *voff = (uint32_t *)(arena + E->voff), *vcur = (uint32_t *)(arena + E->vcur);
  uint32_t base = 0, isolated = 0;
#if defined(__HIPCC__)
  for (uint32_t v0 = 0; v0 < V; v0 += WAVE) {
    const uint32_t v = v0 + lane;
    uint32_t x = v < V ? voff[v + 1] : 0u, incl = x;
    if (v < V && x == 0) ++isolated;
    for (int d = 1; d < WAVE; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, WAVE); if ((int)lane >= d) incl += y; }
    if (v < V) { voff[v + 1] = base + incl; vcur[v] = base + incl - x; }
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
  if (isolated) atomicAdd(&E->isolated, isolated);
#else       // the sanitizer build of tests/hostcheck/encrepair_host.cpp runs the lanes of a wave one after the other: lane 0 sums
  if (lane == 0) {
    for (uint32_t v = 0; v < V; ++v) { const uint32_t x = voff[v + 1]; if (x == 0) ++isolated; vcur[v] = base; base += x; voff[v + 1] = base; }
    E->isolated = isolated;
  }
#endif
}

__global__ __launch_bounds__(256) void k_enc_repair_lists(uint8_t *arena, EncRepair *reps, uint32_t n) {
  ENC_REPAIR_PROLOGUE
  uint32_t *vcur = (uint32_t *)(arena + E->vcur), *vlist = (uint32_t *)(arena + E->vlist);
  const uint8_t *bvis = arena + E->bvis;
  for (uint32_t c = t0; c < NC; c += stride) if (!bvis[c]) vlist[atomicAdd(&vcur[faces[c]], 1u)] = c;
}

// ---- opposites.  Corner c faces the directed edge a -> b (a at next(c), b at prev(c)); in corner order it takes the earliest
// corner still waiting that faces b -> a and whose face has another tip, else it waits itself.  The corners that face one
// undirected edge are found through the shorter corner list of its end points: a corner k at x with next(k) at y belongs to a face
// whose corner prev(k) faces x -> y, one with prev(k) at y to a face whose corner next(k) faces y -> x.  The thread of the edge's
// first corner replays the edge: the next corner in index order by a scan of the list (its order is the atomic counter's), its
// partner by another.
__global__ __launch_bounds__(256) void k_enc_repair_opposites(uint8_t *arena, EncRepair *reps, uint32_t n) {
  ENC_REPAIR_PROLOGUE
  uint32_t *opp = (uint32_t *)(arena + E->opp);
  const uint32_t *voff = (const uint32_t *)(arena + E->voff), *vlist = (const uint32_t *)(arena + E->vlist);
  const uint8_t *bvis = arena + E->bvis;
  uint8_t *pend = arena + E->pend;
  const uint32_t step_limit = 64u * NC + 4096u;
  for (uint32_t c = t0; c < NC; c += stride) {
    if (bvis[c]) continue;
    const uint32_t a = faces[ec_next(c)], b = faces[ec_prev(c)];
    // x: the end point whose list is read; forward: the corners that face x -> y
    const bool at_b = voff[b + 1] - voff[b] <= voff[a + 1] - voff[a];
    const uint32_t x = at_b ? b : a, y = at_b ? a : b, lo = voff[x], hi = voff[x + 1];
    uint32_t steps = 0;
    // the least corner of the edge above `above` (-1: the least of all); dir: 1 when it faces x -> y
    auto next_corner = [&](int64_t above, uint32_t &dir) {
      uint32_t best = DSA_INVALID;
      for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t k = vlist[i];
        ++steps;
        if (faces[ec_next(k)] == y) { const uint32_t e = ec_prev(k); if ((int64_t)e > above && e < best) { best = e; dir = 1; } }
        else if (faces[ec_prev(k)] == y) { const uint32_t e = ec_next(k); if ((int64_t)e > above && e < best) { best = e; dir = 0; } }
      }
      return best;
    };
    uint32_t dir = 0;
    if (next_corner(-1, dir) != c) continue;                  // (another thread's edge)
    int64_t last = -1;
    for (;;) {
      const uint32_t cur = next_corner(last, dir);
      if (cur == DSA_INVALID) break;
      if (steps > step_limit) { er_fail(E, ENC_REPAIR_BOUND, cur); break; }
      const uint32_t tip = faces[cur];
      uint32_t partner = DSA_INVALID;                         // the earliest waiting corner that faces the other way, with another tip
      for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t k = vlist[i];
        ++steps;
        uint32_t e = DSA_INVALID;
        if (faces[ec_next(k)] == y) { if (dir == 0) e = ec_prev(k); }
        else if (faces[ec_prev(k)] == y) { if (dir == 1) e = ec_next(k); }
        if (e != DSA_INVALID && e < partner && pend[e] && faces[e] != tip) partner = e;
      }
      if (partner == DSA_INVALID) pend[cur] = 1;
      else { pend[partner] = 0; opp[cur] = partner; opp[partner] = cur; }
      last = (int64_t)cur;
    }
  }
}

// ---- the two serial passes: lane l of block b takes mesh b * lanes_per_wave + l
__global__ __launch_bounds__(WAVE) void k_enc_repair_fans(uint8_t *arena, EncRepair *reps, uint32_t n, uint32_t lanes_per_wave) {
  if (threadIdx.x >= lanes_per_wave) return;
  const uint32_t mesh = blockIdx.x * lanes_per_wave + threadIdx.x;
  if (mesh >= n) return;
  EncRepair *E = &reps[mesh];
  if (E->status != ENC_REPAIR_OK) return;
  const uint32_t F = E->F, V = E->V, NC = 3u * F;
  uint32_t *c2v = (uint32_t *)(arena + E->c2v), *opp = (uint32_t *)(arena + E->opp), *parent = (uint32_t *)(arena + E->parent);
  uint32_t *stamp = (uint32_t *)(arena + E->stamp);
  uint8_t *bvis = arena + E->bvis, *cvis = arena + E->cvis, *vvis = arena + E->vvis;
  auto swing_left = [&](uint32_t c) { const uint32_t o = opp[ec_next(c)]; return o == DSA_INVALID ? o : ec_next(o); };
  auto swing_right = [&](uint32_t c) { const uint32_t o = opp[ec_prev(c)]; return o == DSA_INVALID ? o : ec_prev(o); };
  uint32_t steps = 0;
  bool failed = false;
  const uint32_t step_limit = 64u * NC + 4096u;
  auto runaway = [&]() { if (++steps > step_limit) failed = true; return failed; };

  // BreakNonManifoldEdges, :396-469.  A sweep that cut a fan leaves corners of it unvisited behind the place it cut at; every
  // corner in front of the first such place is visited, so the next sweep starts there.
  uint32_t breaks = 0, fan = 0, restart = 0;
  while (restart < NC && !failed) {
    uint32_t again = NC;
    for (uint32_t c = restart; c < NC && !runaway(); ++c) {
      if (bvis[c]) continue;
      ++fan;
      uint32_t first = c, cur = c, nx = swing_left(cur);
      while (nx != first && nx != DSA_INVALID && !bvis[nx] && !runaway()) { cur = nx; nx = swing_left(cur); }
      first = cur;
      do {
        if (runaway()) break;
        bvis[cur] = 1;
        const uint32_t sink_c = ec_next(cur), edge_c = ec_prev(cur), sink_v = c2v[sink_c], from_v = c2v[edge_c];
        uint32_t other = DSA_INVALID;
        if (stamp[3 * sink_v] == fan) {                       // an edge of this fan reached the sink before: cut unless it is this edge seen from the other side
          const uint32_t e1 = stamp[3 * sink_v + 1], e2 = stamp[3 * sink_v + 2];
          other = e1 != opp[edge_c] ? e1 : e2;
        }
        if (other != DSA_INVALID) {
          const uint32_t o_edge = opp[edge_c], o_other = opp[other];
          if (o_edge != DSA_INVALID) opp[o_edge] = DSA_INVALID;
          if (o_other != DSA_INVALID) opp[o_other] = DSA_INVALID;
          opp[edge_c] = DSA_INVALID; opp[other] = DSA_INVALID;
          ++breaks;
          again = c < again ? c : again;
          break;
        }
        if (stamp[3 * from_v] != fan) { stamp[3 * from_v] = fan; stamp[3 * from_v + 1] = sink_c; stamp[3 * from_v + 2] = DSA_INVALID; }
        else if (stamp[3 * from_v + 2] == DSA_INVALID) stamp[3 * from_v + 2] = sink_c;
        cur = swing_right(cur);
      } while (cur != first && cur != DSA_INVALID);
    }
    restart = again;
  }

  // ComputeVertexCorners, :471-547: corners in index order; the first fan of a vertex keeps it, every later one is a new vertex
  uint32_t nv = V;
  for (uint32_t c = 0; c < NC && !runaway(); ++c) {
    if (cvis[c]) continue;
    uint32_t v = c2v[c];
    bool fresh = false;
    if (vvis[v]) { parent[nv - V] = v; v = nv++; fresh = true; }
    else vvis[v] = 1;
    uint32_t act = c;
    while (act != DSA_INVALID && !runaway()) {
      cvis[act] = 1;
      if (fresh) c2v[act] = v;
      act = swing_left(act);
      if (act == c) break;
    }
    if (act == DSA_INVALID) {
      act = swing_right(c);
      while (act != DSA_INVALID && !runaway()) { cvis[act] = 1; if (fresh) c2v[act] = v; act = swing_right(act); }
    }
  }
  E->num_vertices = nv; E->breaks = breaks;
  if (failed) er_fail(E, ENC_REPAIR_BOUND, steps);
}

// ---- the one kind of mesh the strict table takes and the reference's table does not leave as it is: two faces over the same three
// vertices, turned against each other (every half-edge once, every vertex one closed fan of two).  The reference's matching does
// not pair a corner with one of the same tip vertex, so it codes two separate triangles.  Behind k_enc_table_corners in the first
// pass of a repair call: such a mesh is refused there like any other that needs the repair, and comes back on the repaired table.
__global__ __launch_bounds__(256) void k_enc_repair_scan(uint8_t *arena, EncConn *conns, uint32_t n) {
  const uint32_t mesh = blockIdx.y;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK) return;
  const uint32_t NC = 3u * E->F;
  const uint32_t *c2v = (const uint32_t *)(arena + E->faces), *opp = (const uint32_t *)(arena + E->opp);
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < NC; c += gridDim.x * blockDim.x) {
    const uint32_t o = opp[c];
    if (o < NC && c2v[o] == c2v[c]) atomicMin(&E->fail_key, (uint32_t)ENC_NONMANIFOLD_EDGE);
  }
}

// ---- behind k_enc_operands / k_enc_pd_operands, for a mesh laid out from a repaired table: an entry's vertex becomes the value
// row it reads (the vertex itself, or the parent of a vertex the repair made)
struct EncRepairRows { uint64_t e2v, pd_e2v, row; uint32_t count, pad; };      // pd_e2v: 0 without a prediction-degree order
__global__ __launch_bounds__(256) void k_enc_repair_rows(uint8_t *arena, const EncRepairRows *rows, uint32_t n) {
  const uint32_t mesh = blockIdx.y;
  if (mesh >= n) return;
  const EncRepairRows R = rows[mesh];
  const uint32_t *row = (const uint32_t *)(arena + R.row);
  uint32_t *e2v = (uint32_t *)(arena + R.e2v), *pd = R.pd_e2v ? (uint32_t *)(arena + R.pd_e2v) : nullptr;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < R.count; p += gridDim.x * blockDim.x) {
    const uint32_t v = e2v[p];
    if (v < R.count) e2v[p] = row[v];
    if (pd) { const uint32_t w = pd[p]; if (w < R.count) pd[p] = row[w]; }
  }
}

}  // namespace dsa
