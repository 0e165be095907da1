// draco-sharp_amd/csrc/dsa_encode_seams.h  (included by dsa_encode.h after dsa_encode_conn.h)
//
// Encode direction, attributes given per corner (dsa_encode_batch_corners): the attribute seams on the device.  Each step is the
// device form of the host coder's (dsa_encode_host.h), down to the order of ids:
//   seam edges           AttrConn::build, first loop          MeshAttributeCornerTable.cs:32-78   k_enc_seam_edges
//   attribute vertices   AttrConn::build, second loop         MeshAttributeCornerTable.cs:95-155  k_enc_seam_fans, _offsets, _assign
//   attribute walk       dfs_sequence on the attribute table  MeshEdgeBreakerEncoder.cs:545-566   k_enc_seam_records, k_enc_seam_walk
//   operand entries      write_attribute_values' parallelogram on the attribute table             k_enc_seam_operands
//   seam bits            write_stream's seam loop             MeshEdgeBreakerEncoder.cs:418-440   k_enc_seam_rank, _count, _scan, _bits
// One EncSeam per (mesh, attribute with ids).  An attribute with ids but without an interior seam is coded as a per-vertex
// attribute whose values come through its ids (entry p: row ids[d2c[p]] of the position walk, the positions' operands).  The
// table kernels are grid-parallel (blocks per record x records), the walk is one lane per record, several to a wave, like the
// second walk of k_enc_connectivity (the same code: ec_dfs_walk over the attribute's face records).  The seam bits leave the
// device packed one bit per edge; the host's stream layout rABS-codes them (write_rabs).
#pragma once

namespace dsa {

struct EncSeam {                   // one per (mesh, attribute given per corner); device memory, mirrored on the host
  // arena regions: what they hold -- written by -> last read by (the arena is cleared at the start of a chunk)
  uint64_t ids;                    // u32[3F] (u16[3F] when ids_narrow) value row per corner -- upload phase A -> k_enc_seam_operands
  uint64_t edge_seam, vert_seam;   // u8[3F] edge across corner cut (seam or boundary), u8[V] vertex on a cut -- k_enc_seam_edges -> k_enc_seam_bits / k_enc_seam_fans
  uint64_t afirst, aoff;           // u32[V] first corner of a vertex's fans, u32[V+1] attribute vertex ids per position vertex (scan)
                                   //   -- k_enc_seam_fans, k_enc_seam_offsets -> k_enc_seam_assign
  uint64_t c2av, opp2, v2lm;       // u32[3F] attribute vertex per corner -- k_enc_seam_assign -> k_enc_seam_operands, k_enc_corr (prediction 5
                                   //   / 6); u32[3F] opposite cut at seams -- k_enc_seam_records -> k_enc_seam_operands, k_enc_corr (the
                                   //   ring of GeometricNormal, the neighbours of TexCoordsPortable); u32[3F] left-most corner per attribute vertex
                                   //   -- k_enc_seam_assign -> (the host check; AttrConn::v2lm)
  uint64_t avis, frec;             // u8[3F] attribute vertex marks (2 boundary, 4 visited), EcFace[F] the attribute's face records
                                   //   -- k_enc_seam_records -> k_enc_seam_walk
  uint64_t stack, d2c, v2d;        // u32[F] walk stack -- k_enc_seam_walk only; u32[3F], i32[3F] entries -- k_enc_seam_walk (v2d: -1 by
                                   //   k_enc_seam_assign) -> k_enc_seam_operands, k_enc_corr (prediction 5 / 6)
  uint64_t e2v, ops;               // u32[3F] value row per entry, i32[9F] operand entries (the stream's own) -- k_enc_seam_operands -> k_enc_gather / k_enc_corr
  uint64_t rank, rcorner, eoff;    // u32[F] decoder rank of a face, u32[F] corner at a rank -- k_enc_seam_rank -> k_enc_seam_bits;
                                   //   u32[F+1] seam-bit offset per rank -- k_enc_seam_count, k_enc_seam_scan -> k_enc_seam_bits
  uint64_t bits;                   // u32[(3F + 31) / 32] bit k: interior edge k in decoder order is cut -- k_enc_seam_bits -> download (stream layout)
  uint32_t mesh, stream, ids_narrow, rows;
  uint32_t interior_seams;         // OUTPUT: an interior edge is cut (else the attribute is coded per vertex through its ids)
  uint32_t num_av, num_entries;    // OUTPUT: attribute vertices, entries the walk visited
  uint32_t status;                 // 0 ok; ENC_SEAM_LOOP / ENC_SEAM_UNREACHED / ENC_SEAM_BITS (see enc_seam_message)
};

enum { ENC_SEAM_OK = 0, ENC_SEAM_LOOP = 1, ENC_SEAM_UNREACHED = 2, ENC_SEAM_BITS = 3 };
static inline const char *enc_seam_message(uint32_t status) {
  switch (status) {
    case ENC_SEAM_LOOP: return "attribute seam loop";
    case ENC_SEAM_UNREACHED: return "attribute traversal did not reach every attribute vertex";
    default: return "attribute seam coding failed";
  }
}

__device__ __forceinline__ uint32_t es_id(const uint8_t *arena, const EncSeam &S, uint32_t c) {
  return S.ids_narrow ? (uint32_t)((const uint16_t *)(arena + S.ids))[c] : ((const uint32_t *)(arena + S.ids))[c];
}

// Exclusive scan in place, one wave: off[i + 1] holds count(i) on entry, off[i] the sum of count(0 .. i-1) on exit; returns the total.
__device__ __forceinline__ uint32_t es_wave_scan(uint32_t *off, uint32_t n, uint32_t lane) {
  uint32_t base = 0;
#if defined(__HIPCC__)
  if (lane == 0) off[0] = 0;
  for (uint32_t v0 = 0; v0 < n; v0 += WAVE) {
    const uint32_t v = v0 + lane;
    const uint32_t x = v < n ? off[v + 1] : 0u;
    uint32_t incl = x;
    for (int d = 1; d < WAVE; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, WAVE); if ((int)lane >= d) incl += y; }
    if (v < n) off[v + 1] = base + incl;
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
#else       // the sanitizer build of tests/hostcheck runs the lanes of a wave one after the other: lane 0 sums
  if (lane == 0) { off[0] = 0; for (uint32_t v = 0; v < n; ++v) { base += off[v + 1]; off[v + 1] = base; } }
  else base = off[n];
#endif
  return base;
}

#define ENC_SEAM_PROLOGUE                                                                           \
  const uint32_t si = blockIdx.y;                                                                   \
  if (si >= ns) return;                                                                             \
  EncSeam *S = &seams[si];                                                                          \
  const EncConn *E = &conns[S->mesh];                                                               \
  if (E->status != ENC_OK || E->fail_key != 0xFFFFFFFFu || S->status != ENC_SEAM_OK) return;        \
  const uint32_t F = E->F, V = E->V, NC = 3u * F;                                                   \
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;       \
  const uint32_t *c2v = (const uint32_t *)(arena + E->faces);                                       \
  const uint32_t *opp = (const uint32_t *)(arena + E->opp);                                         \
  uint8_t *edge_seam = arena + S->edge_seam;                                                        \
  (void)F; (void)V; (void)NC; (void)t0; (void)stride; (void)c2v; (void)opp; (void)edge_seam;

// ---- seam edges (AttrConn::build): a boundary edge is cut; an interior edge is cut when either of its end points carries
// different ids on its two faces.  Both end points of a cut are seam vertices.  (The marks start at zero: the arena is cleared.)
__global__ __launch_bounds__(256) void k_enc_seam_edges(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  uint8_t *vert_seam = arena + S->vert_seam;
  bool interior = false;
  for (uint32_t c = t0; c < NC; c += stride) {
    const uint32_t o = opp[c];
    bool cut = o == DSA_INVALID;
    if (!cut && o > c) {
      // the edge's end points: next(c) lies on prev(o), prev(c) on next(o)
      cut = es_id(arena, *S, ec_next(c)) != es_id(arena, *S, ec_prev(o)) || es_id(arena, *S, ec_prev(c)) != es_id(arena, *S, ec_next(o));
      if (cut) {
        interior = true;
        edge_seam[o] = 1;                                   // (every writer of a mark stores the same byte)
        vert_seam[c2v[ec_next(o)]] = 1; vert_seam[c2v[ec_prev(o)]] = 1;
      }
    }
    if (cut) { edge_seam[c] = 1; vert_seam[c2v[ec_next(c)]] = 1; vert_seam[c2v[ec_prev(c)]] = 1; }
  }
  if (interior) S->interior_seams = 1;
}

// ---- attribute vertices, per position vertex: start at its left-most corner (moved left to the cut on a seam vertex), swing
// right and open a new attribute vertex behind every cut.  Counted first, numbered after the scan, in position-vertex order:
// the ids of AttrConn::build.  A swing never takes more steps than the vertex has corners (the manifold check saw to that).
__device__ __forceinline__ uint32_t es_opposite(const uint32_t *opp, const uint8_t *edge_seam, uint32_t c) {
  return (c == DSA_INVALID || edge_seam[c]) ? DSA_INVALID : opp[c];
}
__global__ __launch_bounds__(256) void k_enc_seam_fans(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  const uint32_t *vcorner = (const uint32_t *)(arena + E->vcorner), *voff = (const uint32_t *)(arena + E->voff);
  const uint8_t *vert_seam = arena + S->vert_seam;
  uint32_t *afirst = (uint32_t *)(arena + S->afirst), *aoff = (uint32_t *)(arena + S->aoff);
  for (uint32_t v = t0; v < V; v += stride) {
    const uint32_t cnt = voff[v + 1] - voff[v];
    uint32_t first = vcorner[v], guard = 0, fans = 1;
    if (vert_seam[v]) {
      uint32_t act = ec_next(es_opposite(opp, edge_seam, ec_next(first)));
      while (act != DSA_INVALID) { first = act; act = ec_next(es_opposite(opp, edge_seam, ec_next(act))); if (++guard > cnt) { S->status = ENC_SEAM_LOOP; break; } }
    }
    afirst[v] = first;
    guard = 0;
    uint32_t act = ec_prev(opp[ec_prev(first)]);
    while (act != DSA_INVALID && act != first && ++guard <= cnt) {
      if (edge_seam[ec_next(act)]) ++fans;
      act = ec_prev(opp[ec_prev(act)]);
    }
    aoff[v + 1] = fans < cnt ? fans : cnt;
  }
}
__global__ __launch_bounds__(WAVE) void k_enc_seam_offsets(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  const uint32_t si = blockIdx.x;
  if (si >= ns) return;
  EncSeam *S = &seams[si];
  const EncConn *E = &conns[S->mesh];
  if (E->status != ENC_OK || E->fail_key != 0xFFFFFFFFu || S->status != ENC_SEAM_OK) return;
  const uint32_t total = es_wave_scan((uint32_t *)(arena + S->aoff), E->V, threadIdx.x);
  if (threadIdx.x == 0) S->num_av = total;
}
__global__ __launch_bounds__(256) void k_enc_seam_assign(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  const uint32_t *afirst = (const uint32_t *)(arena + S->afirst), *aoff = (const uint32_t *)(arena + S->aoff);
  uint32_t *c2av = (uint32_t *)(arena + S->c2av), *v2lm = (uint32_t *)(arena + S->v2lm);
  int32_t *v2d = (int32_t *)(arena + S->v2d);
  for (uint32_t v = t0; v < V; v += stride) {
    const uint32_t first = afirst[v], hi = aoff[v + 1];
    uint32_t id = aoff[v];
    for (uint32_t a = id; a < hi; ++a) v2d[a] = -1;
    c2av[first] = id; v2lm[id] = first;
    uint32_t act = ec_prev(opp[ec_prev(first)]);
    while (act != DSA_INVALID && act != first) {
      if (edge_seam[ec_next(act)]) { if (id + 1 >= hi) break; ++id; v2lm[id] = act; }        // (the same swing as the count)
      c2av[act] = id;
      act = ec_prev(opp[ec_prev(act)]);
    }
  }
}

// ---- the attribute's face records for the walk: attribute vertices at the corners, opposites cut at seams; an attribute vertex
// on a cut is on the attribute's boundary (the swing left of its left-most corner ends there)
__global__ __launch_bounds__(256) void k_enc_seam_records(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  if (!S->interior_seams) return;
  const uint32_t *c2av = (const uint32_t *)(arena + S->c2av);
  uint32_t *opp2 = (uint32_t *)(arena + S->opp2);
  uint8_t *avis = arena + S->avis;
  uint4 *frec = (uint4 *)(arena + S->frec);
  for (uint32_t f = t0; f < F; f += stride) {
    const uint32_t c = 3u * f;
    const uint32_t o0 = es_opposite(opp, edge_seam, c), o1 = es_opposite(opp, edge_seam, c + 1), o2 = es_opposite(opp, edge_seam, c + 2);
    const uint32_t a0 = c2av[c], a1 = c2av[c + 1], a2 = c2av[c + 2];
    opp2[c] = o0; opp2[c + 1] = o1; opp2[c + 2] = o2;
    frec[2 * f] = make_uint4(a0, a1, a2, o0);
    frec[2 * f + 1] = make_uint4(o1, o2, 0u, 0u);
    if (o0 == DSA_INVALID) { avis[a1] = 2; avis[a2] = 2; }
    if (o1 == DSA_INVALID) { avis[a2] = 2; avis[a0] = 2; }
    if (o2 == DSA_INVALID) { avis[a0] = 2; avis[a1] = 2; }
  }
}

// ---- the attribute walk, one lane per record: ec_dfs_walk from the connectivity's processed corners (decoder order), on the
// attribute's records; the step bound of the connectivity walks
__global__ __launch_bounds__(WAVE) void k_enc_seam_walk(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns, uint32_t lanes_per_wave) {
  if (threadIdx.x >= lanes_per_wave) return;
  const uint32_t si = blockIdx.x * lanes_per_wave + threadIdx.x;
  if (si >= ns) return;
  EncSeam *S = &seams[si];
  const EncConn *E = &conns[S->mesh];
  if (E->status != ENC_OK || S->status != ENC_SEAM_OK || !S->interior_seams) return;
  const uint32_t F = E->F, NC = 3u * F, A = S->num_av;
  bool stuck = false;
  const uint32_t count = ec_dfs_walk((const uint4 *)(arena + S->frec), (uint32_t *)(arena + S->frec), arena + S->avis, (uint32_t *)(arena + S->stack),
                                     (uint32_t *)(arena + S->d2c), (int32_t *)(arena + S->v2d), (const uint32_t *)(arena + E->processed),
                                     (const uint32_t *)(arena + E->init_corners), E->num_processed, E->num_init, F, A, 64u * NC + 4096u, stuck);
  S->num_entries = count;
  if (stuck) S->status = ENC_SEAM_LOOP;
  else if (count != A) S->status = ENC_SEAM_UNREACHED;
}

// ---- entries -> value rows and the parallelogram operand entries (k_enc_operands on the attribute table: an opposite across a
// seam is none).  Without an interior seam: the position walk's entries through the ids, the positions' operands.  The stream's
// entry count and operand array are set here, before k_enc_gather reads them.
// (Stream: dsa_encode.h's EncStream, which is defined behind this file; its fields nv and ops are the ones set here)
template <class Stream>
__global__ __launch_bounds__(256) void k_enc_seam_operands(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns, Stream *streams) {
  ENC_SEAM_PROLOGUE
  Stream &T = streams[S->stream];
  uint32_t *e2v = (uint32_t *)(arena + S->e2v);
  const bool seamed = S->interior_seams != 0;
  const uint32_t entries = seamed ? S->num_av : V;
  if (t0 == 0) { T.nv = entries; T.ops = seamed ? S->ops : E->ops; }
  if (!seamed) {
    const uint32_t *d2c = (const uint32_t *)(arena + E->d2c);
    for (uint32_t p = t0; p < V; p += stride) e2v[p] = es_id(arena, *S, d2c[p]);
    return;
  }
  const uint32_t *d2c = (const uint32_t *)(arena + S->d2c), *c2av = (const uint32_t *)(arena + S->c2av), *opp2 = (const uint32_t *)(arena + S->opp2);
  const int32_t *v2d = (const int32_t *)(arena + S->v2d);
  int32_t *ops = (int32_t *)(arena + S->ops);
  for (uint32_t p = t0; p < entries; p += stride) {
    const uint32_t ci = d2c[p];
    e2v[p] = es_id(arena, *S, ci);
    int32_t on = -1, op = -1, oo = -1;
    if (p > 0) {
      const uint32_t oci = opp2[ci];
      if (oci != DSA_INVALID) {
        const int32_t vo = v2d[c2av[oci]], vn = v2d[c2av[ec_next(oci)]], vp = v2d[c2av[ec_prev(oci)]];
        if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { on = vn; op = vp; oo = vo; }
      }
    }
    ops[3 * p] = on; ops[3 * p + 1] = op; ops[3 * p + 2] = oo;
  }
}

// ---- seam bits (write_stream's seam loop): faces in decoder order (processed corners last to first, then the init corners); per
// face the edges whose other face comes later, corner, next, previous; one bit per such edge: is it cut
__global__ __launch_bounds__(256) void k_enc_seam_rank(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  if (!S->interior_seams) return;
  const uint32_t *processed = (const uint32_t *)(arena + E->processed), *init = (const uint32_t *)(arena + E->init_corners);
  uint32_t *rank = (uint32_t *)(arena + S->rank), *rcorner = (uint32_t *)(arena + S->rcorner);
  const uint32_t np = E->num_processed, ni = E->num_init;
  for (uint32_t r = t0; r < np + ni && r < F; r += stride) {
    const uint32_t c = r < np ? processed[np - 1 - r] & (uint32_t)EC_CORNER_MASK : init[r - np];
    rank[c / 3u] = r; rcorner[r] = c;
  }
}
__global__ __launch_bounds__(256) void k_enc_seam_count(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  if (!S->interior_seams) return;
  const uint32_t *rank = (const uint32_t *)(arena + S->rank), *rcorner = (const uint32_t *)(arena + S->rcorner);
  uint32_t *eoff = (uint32_t *)(arena + S->eoff);
  for (uint32_t r = t0; r < F; r += stride) {
    const uint32_t c = rcorner[r], ks[3] = {c, ec_next(c), ec_prev(c)};
    uint32_t k = 0;
    for (int j = 0; j < 3; ++j) { const uint32_t o = opp[ks[j]]; if (o != DSA_INVALID && rank[o / 3u] > r) ++k; }
    eoff[r + 1] = k;
  }
}
__global__ __launch_bounds__(WAVE) void k_enc_seam_scan(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  const uint32_t si = blockIdx.x;
  if (si >= ns) return;
  EncSeam *S = &seams[si];
  const EncConn *E = &conns[S->mesh];
  if (E->status != ENC_OK || S->status != ENC_SEAM_OK || !S->interior_seams) return;
  const uint32_t total = es_wave_scan((uint32_t *)(arena + S->eoff), E->F, threadIdx.x);
  if (threadIdx.x == 0 && total != E->interior_edges) S->status = ENC_SEAM_BITS;
}
__global__ __launch_bounds__(256) void k_enc_seam_bits(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns) {
  ENC_SEAM_PROLOGUE
  if (!S->interior_seams) return;
  const uint32_t *rank = (const uint32_t *)(arena + S->rank), *rcorner = (const uint32_t *)(arena + S->rcorner), *eoff = (const uint32_t *)(arena + S->eoff);
  uint32_t *bits = (uint32_t *)(arena + S->bits);
  for (uint32_t r = t0; r < F; r += stride) {
    const uint32_t c = rcorner[r], ks[3] = {c, ec_next(c), ec_prev(c)};
    uint32_t at = eoff[r];
    for (int j = 0; j < 3; ++j) {
      const uint32_t o = opp[ks[j]];
      if (o == DSA_INVALID || rank[o / 3u] <= r) continue;
      if (edge_seam[ks[j]]) atomicOr(&bits[at >> 5], 1u << (at & 31u));
      ++at;
    }
  }
}

}  // namespace dsa
