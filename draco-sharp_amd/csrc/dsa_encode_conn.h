// draco-sharp_amd/csrc/dsa_encode_conn.h  (included by dsa_encode.h)
//
// Encode direction, connectivity on the device: corner table, Edgebreaker symbols,
// depth-first attribute order and parallelogram operand entries of a batch of triangle meshes, one wave per mesh.
//   corner table            CornerTable.cs:15-172 (opposites from shared edges, left-most corners, manifold checks)
//   Edgebreaker traversal   MeshEdgeBreakerEncoder.cs:38-124 (start faces), :158-183 (init face), :185-274 (symbols),
//                           :276-303 (holes), :331-361 (hole ids), :373-390 (topology splits)
//   attribute order         Traverser/DepthFirstTraverser.cs:9-99, MeshTraversalSequencer.cs:13-31
// It is the host coder of dsa_encode_host.h (CornerTable::build, EbEncoder, dfs_sequence) on arrays in device memory.  The table
// construction and the operand entries are grid-parallel kernels (blocks per mesh x meshes).  The two traversals are sequential
// by nature -- every step decides the next from what is visited -- and bound by the latency of one memory round trip per step:
// they run ONE LANE PER MESH, several meshes to a wave (k_enc_connectivity), so that a memory instruction carries the step of
// every mesh of the wave and thousands of walks are in flight on a handful of waves per CU.
// The byte stream that results is the CPU coder's (tests/test_gpu_encode.py compares them).
#pragma once

namespace dsa {

struct EncConn {                   // one per mesh; device memory, mirrored on the host
  uint64_t faces;                  // u32[3F] input: vertex of every corner
  uint64_t faces16;                // u16[3F], when faces_narrow: the same as it was uploaded (every index fits; k_enc_table_clear widens it into `faces`)
  uint64_t opp;                    // u32[3F] opposite corner or INVALID
  uint64_t voff, vcur, vlist;      // u32[V+1], u32[V], u32[3F]: corners by vertex
  uint64_t vcorner;                // u32[V] left-most corner
  uint64_t vvis;                   // u8[V] marks of a vertex: 1 visited by the Edgebreaker walk, 2 on a boundary, 4 visited by the attribute walk, 8 its hole is coded
  uint64_t frec;                   // EcFace[F]: what a step of either walk needs of a face, in one 32-byte record
  uint64_t stack;                  // u32[F]
  uint64_t processed, init_corners;// u32[F] each; processed: corner | symbol << 29
  uint64_t symbols;                // u8[F] OUTPUT encoder order, bit patterns 0 1 3 5 7 (k_enc_operands takes them out of `processed`)
  uint64_t start_bits;             // u8[F] OUTPUT
  uint64_t splits;                 // u32[3 * split_cap] OUTPUT (source, split, edge)
  uint64_t d2c, v2d;               // u32[V], i32[V]
  uint64_t e2v, ops;               // u32[V], i32[3V] OUTPUT for the attribute kernels
  uint32_t F, V, split_cap, faces_narrow;
  uint32_t fail_key;               // k_enc_table_corners: the least status code that any vertex earned (the host coder's order of checks), or ~0
  uint32_t num_symbols, num_start_bits, num_splits, num_split_symbols, num_processed, num_init, num_entries, interior_edges;   // OUTPUT
  uint32_t status, detail;         // 0 ok; else the host coder's complaint (see enc_conn_message)
  // valence context lists (dsa_encode_schemes.h, which lists the regions with their writers and readers); vstream: the first of
  // the mesh's six list streams, DSA_INVALID for a mesh coded with standard symbols (all regions then 0)
  uint64_t init_time, vtime, vval, vc2v, vctx, vsyms, vbl, vrans, vbits;
  uint32_t vstream;
  uint32_t vcount[6];              // OUTPUT of k_enc_valence: symbols per context
  // prediction-degree order (dsa_encode_multi.h), all 0 for a mesh whose decoders take the depth-first order alone:
  //   pd_d2c, pd_v2d  u32[V], i32[V]  the second order                       k_enc_pd_walk -> k_enc_pd_operands, k_enc_multi / k_enc_corr (topology view)
  //   pd_e2v, pd_ops  u32[V], i32[3V] entry -> vertex, operand entries       k_enc_pd_operands -> k_enc_gather / k_enc_corr
  //   pd_next, pd_degree, pd_fvis  u32[3F], u32[V], u8[F]  stack links, degree counters, face marks   k_enc_pd_walk only
  uint64_t pd_d2c, pd_v2d, pd_e2v, pd_ops, pd_next, pd_degree, pd_fvis;
};
// A face as the walks see it: the vertices at its corners, the corners across its edges (o[k] = opposite of corner 3f + k), and two
// marks -- mark: 0 not visited by the Edgebreaker walk; 1 visited; s + 2 visited, and the S with symbol id s was coded at it (what
// MeshEdgeBreakerEncoder.cs keeps in a face -> split symbol map); mark2: visited by the attribute walk.  From a corner of the face,
// the vertex at it and the corners across its right and left edge are fields of this record; the faces across are one load each.
struct EcFace { uint32_t v0, v1, v2, o0, o1, o2, mark, mark2; };
static_assert(sizeof(EcFace) == 32, "face record");

enum { ENC_OK = 0, ENC_DEGENERATE = 1, ENC_NONMANIFOLD_EDGE = 2, ENC_RING = 3, ENC_NONMANIFOLD_VERTEX = 4, ENC_ISOLATED = 5, ENC_UNREACHED = 6, ENC_SPLITS = 7 };
static inline const char *enc_conn_message(uint32_t status) {
  switch (status) {
    case ENC_DEGENERATE: return "degenerate face in input mesh";
    case ENC_NONMANIFOLD_EDGE: return "non-manifold edge (duplicate half-edge)";
    case ENC_RING: return "vertex ring does not close";
    case ENC_NONMANIFOLD_VERTEX: return "non-manifold vertex in input mesh";
    case ENC_ISOLATED: return "isolated vertex in input mesh";
    case ENC_UNREACHED: return "traversal did not reach every vertex";
    case ENC_SPLITS: return "too many topology splits";
    default: return "connectivity coding failed";
  }
}

__device__ __forceinline__ uint32_t ec_next(uint32_t c) { return c == DSA_INVALID ? c : ((c + 1) % 3 ? c + 1 : c - 2); }
__device__ __forceinline__ uint32_t ec_prev(uint32_t c) { return c == DSA_INVALID ? c : (c % 3 ? c - 1 : c + 2); }

struct EcTable {                   // the corner table as the traversals see it
  const uint32_t *c2v, *opp, *vcorner;
  __device__ __forceinline__ uint32_t opposite(uint32_t c) const { return c == DSA_INVALID ? c : opp[c]; }
  __device__ __forceinline__ uint32_t vertex(uint32_t c) const { return c == DSA_INVALID ? DSA_INVALID : c2v[c]; }
  __device__ __forceinline__ uint32_t swing_right(uint32_t c) const { return ec_prev(opposite(ec_prev(c))); }
  __device__ __forceinline__ uint32_t swing_left(uint32_t c) const { return ec_next(opposite(ec_next(c))); }
  __device__ __forceinline__ uint32_t right_corner(uint32_t c) const { return opposite(ec_next(c)); }
  __device__ __forceinline__ uint32_t left_corner(uint32_t c) const { return opposite(ec_prev(c)); }
};

__device__ __forceinline__ void ec_fail(EncConn *E, uint32_t status, uint32_t detail) { if (atomicCAS(&E->status, 0u, status) == 0u) E->detail = detail; }


// The corner table is built by kernels of their own, every mesh of the chunk on as many blocks as its corners ask for (grid: blocks
// per mesh x meshes): nothing in it is sequential, and on one wave per mesh -- where the walks below have to live -- it took a
// quarter of the connectivity time.  A step that needs the previous one complete for the whole mesh is a launch.
#define ENC_TABLE_PROLOGUE                                                                          \
  const uint32_t mesh = blockIdx.y;                                                                 \
  if (mesh >= n) return;                                                                            \
  EncConn *E = &conns[mesh];                                                                        \
  if (E->status != ENC_OK) return;                                                                  \
  const uint32_t F = E->F, V = E->V, NC = 3u * F;                                                   \
  const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;       \
  const uint32_t *c2v = (const uint32_t *)(arena + E->faces);                                       \
  (void)F; (void)V; (void)NC; (void)t0; (void)stride; (void)c2v;

// counts start at zero; the marks of the walks too
__global__ __launch_bounds__(256) void k_enc_table_clear(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  uint32_t *voff = (uint32_t *)(arena + E->voff);
  uint8_t *vvis = arena + E->vvis;
  int32_t *v2d = (int32_t *)(arena + E->v2d);
  for (uint32_t v = t0; v <= V; v += stride) voff[v] = 0;
  for (uint32_t v = t0; v < V; v += stride) { vvis[v] = 0; v2d[v] = -1; }
  if (E->faces_narrow) {
    const uint16_t *narrow = (const uint16_t *)(arena + E->faces16);
    uint32_t *wide = (uint32_t *)(arena + E->faces);
    for (uint32_t c = t0; c < NC; c += stride) wide[c] = narrow[c];
  }
}

// ---- corners by vertex (counting sort: counts -> offsets -> lists), CornerTable.cs:41-67 needs them implicitly
__global__ __launch_bounds__(256) void k_enc_table_count(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  uint32_t *voff = (uint32_t *)(arena + E->voff);
  for (uint32_t c = t0; c < NC; c += stride) {
    const uint32_t a = c2v[ec_next(c)], b = c2v[ec_prev(c)];
    if (a == b || a == c2v[c] || b == c2v[c]) ec_fail(E, ENC_DEGENERATE, c / 3);
    atomicAdd(&voff[c2v[c] + 1], 1u);
  }
}

// exclusive prefix sum, one wave per mesh: voff[v + 1] held count(v)
__global__ __launch_bounds__(WAVE) void k_enc_table_offsets(uint8_t *arena, EncConn *conns, uint32_t n) {
  const uint32_t mesh = blockIdx.x, lane = threadIdx.x;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK) return;
  const uint32_t V = E->V;
  uint32_t *voff = (uint32_t *)(arena + E->voff), *vcur = (uint32_t *)(arena + E->vcur);
  uint32_t base = 0;
#if defined(__HIPCC__)
  for (uint32_t v0 = 0; v0 < V; v0 += WAVE) {
    const uint32_t v = v0 + lane;
    uint32_t x = v < V ? voff[v + 1] : 0u, incl = x;
    for (int d = 1; d < WAVE; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, WAVE); if ((int)lane >= d) incl += y; }
    if (v < V) { voff[v + 1] = base + incl; vcur[v] = base + incl - x; }
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
#else       // the sanitizer build of tests/hostcheck/encconn_host.cpp runs the lanes of a wave one after the other: lane 0 sums
  if (lane == 0) for (uint32_t v = 0; v < V; ++v) { const uint32_t x = voff[v + 1]; vcur[v] = base; base += x; voff[v + 1] = base; }
#endif
}

__global__ __launch_bounds__(256) void k_enc_table_lists(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  uint32_t *vcur = (uint32_t *)(arena + E->vcur), *vlist = (uint32_t *)(arena + E->vlist);
  for (uint32_t c = t0; c < NC; c += stride) vlist[atomicAdd(&vcur[c2v[c]], 1u)] = c;
}

// ---- opposites: corner c faces the edge next(c) -> prev(c) = a -> b; its opposite is the corner facing b -> a.  That face has a
// corner k at b whose next is a (opposite: prev(k)) and a corner k' at a whose previous is b (opposite: next(k')): the shorter of
// the two vertex lists is searched, so that a vertex of huge valence (the apex of a cone) costs its neighbours nothing.  The same
// directed edge twice is a non-manifold edge.  (The lists of a vertex come out of the atomic counter in any order; nothing below
// depends on it.)
__global__ __launch_bounds__(256) void k_enc_table_opposites(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  uint32_t *opp = (uint32_t *)(arena + E->opp);
  const uint32_t *voff = (const uint32_t *)(arena + E->voff), *vlist = (const uint32_t *)(arena + E->vlist);
  for (uint32_t c = t0; c < NC; c += stride) {
    const uint32_t a = c2v[ec_next(c)], b = c2v[ec_prev(c)];
    const uint32_t na = voff[a + 1] - voff[a], nb = voff[b + 1] - voff[b];
    uint32_t found = DSA_INVALID, same = 0;
    if (nb <= na) {
      for (uint32_t i = voff[b]; i < voff[b + 1]; ++i) {
        const uint32_t k = vlist[i];
        if (c2v[ec_next(k)] == a) found = ec_prev(k);          // face (b, a, .): reverse edge
        if (c2v[ec_prev(k)] == a) ++same;                      // face (a, b, .) seen from its corner at b: the edge itself
      }
    } else {
      for (uint32_t i = voff[a]; i < voff[a + 1]; ++i) {
        const uint32_t k = vlist[i];
        if (c2v[ec_prev(k)] == b) found = ec_next(k);          // face (b, a, .) seen from its corner at a
        if (c2v[ec_next(k)] == b) ++same;                      // face (a, b, .): the edge itself
      }
    }
    if (same != 1) ec_fail(E, ENC_NONMANIFOLD_EDGE, c);
    opp[c] = found;
  }
}

// ---- left-most corner per vertex (first corner in index order, moved left to the boundary if there is one) and the manifold
// check: every corner of the vertex is reached by swinging right from there; the count of interior half-edges; the face records
// of the walks; and the boundary mark of a vertex: the end of an edge without an opposite.  (MeshEdgeBreakerEncoder.cs:331-361
// numbers the boundary loops and keeps "loop coded" per number; the walks below only ever ask "is this vertex on a boundary" and
// "is the loop through this vertex coded", which a mark on every vertex of a loop answers -- a vertex that passed the manifold
// check lies on one loop at most.)
__global__ __launch_bounds__(256) void k_enc_table_corners(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  const uint32_t *opp = (const uint32_t *)(arena + E->opp), *voff = (const uint32_t *)(arena + E->voff), *vlist = (const uint32_t *)(arena + E->vlist);
  uint32_t *vcorner = (uint32_t *)(arena + E->vcorner);
  uint8_t *vvis = arena + E->vvis;
  uint4 *frec = (uint4 *)(arena + E->frec);
  EcTable ct;
  ct.c2v = c2v; ct.opp = opp; ct.vcorner = vcorner;
  uint32_t interior = 0;
  for (uint32_t f = t0; f < F; f += stride) {
    const uint32_t c = 3u * f;
    const uint32_t o0 = opp[c], o1 = opp[c + 1], o2 = opp[c + 2], v0 = c2v[c], v1 = c2v[c + 1], v2 = c2v[c + 2];
    interior += (o0 != DSA_INVALID ? 1u : 0u) + (o1 != DSA_INVALID ? 1u : 0u) + (o2 != DSA_INVALID ? 1u : 0u);
    frec[2 * f] = make_uint4(v0, v1, v2, o0);
    frec[2 * f + 1] = make_uint4(o1, o2, 0u, 0u);
    if (o0 == DSA_INVALID) { vvis[v1] = 2; vvis[v2] = 2; }      // (every writer stores the same byte)
    if (o1 == DSA_INVALID) { vvis[v2] = 2; vvis[v0] = 2; }
    if (o2 == DSA_INVALID) { vvis[v0] = 2; vvis[v1] = 2; }
  }
  if (interior) atomicAdd(&E->interior_edges, interior);      // half-edges here; the walk kernel halves it
  for (uint32_t v = t0; v < V; v += stride) {
    const uint32_t cnt = voff[v + 1] - voff[v];
    if (cnt == 0) { atomicMin(&E->fail_key, (uint32_t)ENC_ISOLATED); vcorner[v] = DSA_INVALID; continue; }
    uint32_t first = DSA_INVALID;
    for (uint32_t i = voff[v]; i < voff[v + 1]; ++i) first = vlist[i] < first ? vlist[i] : first;
    uint32_t act = ct.swing_left(first), c = first, guard = 0, lm = first;
    while (act != DSA_INVALID && act != first) { c = act; act = ct.swing_left(act); if (++guard >= NC) { atomicMin(&E->fail_key, (uint32_t)ENC_RING); break; } }
    if (act != first) lm = c;
    vcorner[v] = lm;
    uint32_t reach = 0, k = lm;
    do { ++reach; k = ct.swing_right(k); } while (k != DSA_INVALID && k != lm && reach <= cnt);
    if (reach != cnt) atomicMin(&E->fail_key, (uint32_t)ENC_NONMANIFOLD_VERTEX);
  }
}

// ---- the two walks, one lane per mesh
__device__ __forceinline__ EcFace ec_face(const uint4 *frec, uint32_t f) {
  const uint4 a = frec[2 * f], b = frec[2 * f + 1];
  EcFace r;
  r.v0 = a.x; r.v1 = a.y; r.v2 = a.z; r.o0 = a.w; r.o1 = b.x; r.o2 = b.y; r.mark = b.z; r.mark2 = b.w;
  return r;
}
struct EcHop { uint32_t v, rc, lc; };                  // from corner 3f + k: the vertex at it, the corners across its right and left edge
__device__ __forceinline__ EcHop ec_hop(const EcFace &r, uint32_t k) {
  uint32_t v0 = r.v0, v1 = r.v1, v2 = r.v2, o0 = r.o0, o1 = r.o1, o2 = r.o2;
#if defined(__HIPCC__)
  // The six words are values in registers from here on.  Without this the optimiser turns "one of three fields by k" into a table
  // in scratch memory -- the record stored and read back through the memory pipeline in front of every step's loads, a dependent
  // round trip more per step.
  asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(o0), "+v"(o1), "+v"(o2));
#endif
  EcHop h;
  h.v = k == 0 ? v0 : (k == 1 ? v1 : v2);
  h.rc = k == 0 ? o1 : (k == 1 ? o2 : o0);             // opposite of the next corner
  h.lc = k == 0 ? o2 : (k == 1 ? o0 : o1);             // opposite of the previous corner
  return h;
}
enum { EC_MARK = 6, EC_MARK2 = 7, EC_CORNER_MASK = 0x1FFFFFFF, EC_SYMBOL_SHIFT = 29 };    // words of a face record; fields of a `processed` entry

// Depth-first attribute order over the decoder's face order (DepthFirstTraverser.cs:9-99), one lane: the second walk of
// k_enc_connectivity over the position table, and the walk of a seamed attribute over that attribute's face records
// (dsa_encode_seams.h).  Vertex marks: 2 on a boundary, 4 visited; face mark: word EC_MARK2 of the record.  Entries go to
// d2c / v2d (nv of them at most); returns how many vertices were visited, `stuck` when the step bound or a full stack stopped it.
__device__ __forceinline__ uint32_t ec_dfs_walk(const uint4 *frec, uint32_t *fw, uint8_t *vvis, uint32_t *stack, uint32_t *d2c, int32_t *v2d,
                                                const uint32_t *processed, const uint32_t *init_corners, uint32_t nproc, uint32_t ninit,
                                                uint32_t F, uint32_t V, uint32_t step_limit, bool &stuck) {
  const uint32_t nstarts = nproc + ninit;
  uint32_t count = 0, dfs_steps = 0, nfaces = 0;
  auto visit = [&](uint32_t v, uint32_t vm, uint32_t c) { vvis[v] = (uint8_t)(vm | 4u); v2d[v] = (int32_t)count; if (count < V) d2c[count] = c; ++count; };
  for (uint32_t i = 0; i < nstarts && !stuck && nfaces < F;) {
    // the next start whose face is still to do: eight candidates a round trip
    uint32_t cand[8], m2[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t k = i + j;
      cand[j] = k < nstarts ? (k < nproc ? processed[nproc - 1 - k] & (uint32_t)EC_CORNER_MASK : init_corners[k - nproc]) : DSA_INVALID;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) m2[j] = cand[j] != DSA_INVALID ? fw[8 * (cand[j] / 3u) + EC_MARK2] : 1u;
    uint32_t start = DSA_INVALID, hit = 8;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) if (hit == 8 && m2[j] == 0) { hit = j; start = cand[j]; }
    if (hit == 8) { i += 8; continue; }
    i += hit + 1;
    uint32_t sp = 0;
    stack[sp++] = start;
    {
      const EcFace sf = ec_face(frec, start / 3u);
      const uint32_t k = start - 3u * (start / 3u);
      const uint32_t nvx = k == 0 ? sf.v1 : (k == 1 ? sf.v2 : sf.v0), pvx = k == 0 ? sf.v2 : (k == 1 ? sf.v0 : sf.v1);
      { const uint32_t m = vvis[nvx]; if (!(m & 4u)) visit(nvx, m, ec_next(start)); }
      { const uint32_t m = vvis[pvx]; if (!(m & 4u)) visit(pvx, m, ec_prev(start)); }
    }
    while (sp && !stuck) {
      uint32_t corner = stack[sp - 1];
      if (corner == DSA_INVALID) { --sp; continue; }
      uint32_t f = corner / 3u;
      EcFace cur = ec_face(frec, f);
      if (cur.mark2 != 0) { --sp; continue; }
      for (;;) {
        if (++dfs_steps > step_limit || count > V) { stuck = true; break; }
        const EcHop h = ec_hop(cur, corner - 3u * f);
        const uint32_t fr = h.rc == DSA_INVALID ? 0u : h.rc / 3u, fl = h.lc == DSA_INVALID ? 0u : h.lc / 3u;
        const uint32_t vm = vvis[h.v];
        const EcFace R = ec_face(frec, fr), L = ec_face(frec, fl);
        const bool r_done = h.rc == DSA_INVALID || fr == f || R.mark2 != 0, l_done = h.lc == DSA_INVALID || fl == f || L.mark2 != 0;
        fw[8 * f + EC_MARK2] = 1u;
        ++nfaces;
        if (!(vm & 4u)) {
          visit(h.v, vm, corner);
          if (!(vm & 2u)) { corner = h.rc; f = fr; cur = R; continue; }
        }
        if (r_done) {
          if (l_done) { --sp; break; }
          corner = h.lc; f = fl; cur = L;
        } else {
          if (l_done) { corner = h.rc; f = fr; cur = R; }
          else {
            if (sp >= F) { stuck = true; break; }
            stack[sp - 1] = h.lc; stack[sp++] = h.rc;
            break;
          }
        }
      }
    }
  }
  return count;
}

// Lane l of block b walks mesh b * lanes_per_wave + l.  A step of either walk is one memory round trip -- the marks of the vertex
// at the corner and the records of the two faces across, which all hang off what the previous step loaded, are issued together --
// and two stores (the mark of the face; the corner and its symbol).  Lanes whose meshes differ in shape diverge and rejoin by
// the compiler's rules; meshes of one shape (a batch of scans of one kind) step in lockstep.
// Every walk below ends by itself on a mesh that passed the checks above (the host coder, which has no such counter, was fuzzed
// with 20 000 damaged meshes); the counter only makes sure that a kernel can never spin: a GPU does not take Ctrl-C.
// record_time (k_enc_connectivity_timed): the walk also records, per interior start face, how many symbols were coded before it
// (init_time; what the valence pass needs of the host coder's face_time beside the order of `processed`).
template <bool record_time>
__device__ __forceinline__ void ec_connectivity(uint8_t *arena, EncConn *conns, uint32_t n, uint32_t lanes_per_wave) {
  if (threadIdx.x >= lanes_per_wave) return;
  const uint32_t mesh = blockIdx.x * lanes_per_wave + threadIdx.x;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK) return;
  if (E->fail_key != 0xFFFFFFFFu) { ec_fail(E, E->fail_key, 0); return; }
  const uint32_t F = E->F, V = E->V, NC = 3u * F;
  const uint32_t *c2v = (const uint32_t *)(arena + E->faces);
  const uint32_t *opp = (const uint32_t *)(arena + E->opp);
  EcTable ct;
  ct.c2v = c2v; ct.opp = opp; ct.vcorner = (const uint32_t *)(arena + E->vcorner);
  uint8_t *vvis = arena + E->vvis;
  uint32_t *stack = (uint32_t *)(arena + E->stack), *processed = (uint32_t *)(arena + E->processed), *init_corners = (uint32_t *)(arena + E->init_corners);
  uint8_t *start_bits = arena + E->start_bits;
  uint32_t *splits = (uint32_t *)(arena + E->splits);
  uint32_t *d2c = (uint32_t *)(arena + E->d2c);
  int32_t *v2d = (int32_t *)(arena + E->v2d);
  const uint4 *frec = (const uint4 *)(arena + E->frec);
  uint32_t *fw = (uint32_t *)(arena + E->frec);                                   // the records as words: marks at 8 f + EC_MARK, 8 f + EC_MARK2

  uint32_t steps = 0;
  bool failed = false;
  const uint32_t step_limit = 64u * NC + 4096u;
  auto runaway = [&]() { if (++steps > step_limit) failed = true; return failed; };
  // the first face at or behind `from` whose mark (word w of its record) is still zero, or F: eight records a round trip
  auto next_fresh = [&](uint32_t from, uint32_t w) {
    while (from < F) {
      uint32_t m[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) { const uint32_t f = from + j < F ? from + j : F - 1; m[j] = fw[8 * f + w]; }
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) if (from + j < F && m[j] == 0) return from + j;
      from += 8;
    }
    return F;
  };

  // ---- Edgebreaker symbols
  uint32_t nproc = 0, ninit = 0, nstart = 0, nsplit = 0, nsplit_sym = 0;
  int32_t last_symbol_id = -1;
  auto encode_hole = [&](uint32_t start_corner, bool encode_first) {            // MeshEdgeBreakerEncoder.cs:276-303
    uint32_t c = ec_prev(start_corner);
    while (opp[c] != DSA_INVALID && !runaway()) c = ec_next(opp[c]);
    const uint32_t start_v = c2v[start_corner];
    { const uint32_t m = vvis[start_v]; vvis[start_v] = (uint8_t)(m | (encode_first ? 1u : 0u) | ((m & 2u) ? 8u : 0u)); }
    uint32_t act = c2v[ec_prev(c)];
    while (act != start_v && !runaway()) {
      vvis[act] |= 9;                                                             // visited; its loop is coded
      c = ec_next(c);
      while (opp[c] != DSA_INVALID && !runaway()) c = ec_next(opp[c]);
      act = c2v[ec_prev(c)];
    }
  };
  auto check_split = [&](int32_t src_symbol, uint32_t edge, uint32_t neighbor_mark) {     // :373-390
    if (neighbor_mark < 2u) return;
    if (nsplit >= E->split_cap) { failed = true; return; }
    splits[3 * nsplit] = (uint32_t)src_symbol; splits[3 * nsplit + 1] = neighbor_mark - 2u; splits[3 * nsplit + 2] = edge;
    ++nsplit;
  };
  auto encode_from_corner = [&](uint32_t corner0) {                             // :185-274
    uint32_t sp = 0;
    stack[sp++] = corner0;
    while (sp && !failed) {
      uint32_t corner = stack[sp - 1];
      if (corner == DSA_INVALID) { --sp; continue; }
      uint32_t f = corner / 3u;
      EcFace cur = ec_face(frec, f);
      if (cur.mark != 0) { --sp; continue; }
      for (;;) {
        if (runaway() || nproc >= F) { failed = true; break; }
        ++last_symbol_id;
        const EcHop h = ec_hop(cur, corner - 3u * f);
        const uint32_t fr = h.rc == DSA_INVALID ? 0u : h.rc / 3u, fl = h.lc == DSA_INVALID ? 0u : h.lc / 3u;
        const uint32_t vm = vvis[h.v];
        const EcFace R = ec_face(frec, fr), L = ec_face(frec, fl);
        // (a face across an edge is never the face itself on a manifold mesh; the test stays, the mark of the face itself being
        // what this step sets)
        const bool r_self = h.rc != DSA_INVALID && fr == f, l_self = h.lc != DSA_INVALID && fl == f;
        const bool r_done = h.rc == DSA_INVALID || r_self || R.mark != 0, l_done = h.lc == DSA_INVALID || l_self || L.mark != 0;
        const bool seen = (vm & 1u) != 0, on_boundary = (vm & 2u) != 0;
        uint32_t sym, mark = 1u, move;                                             // move: 0 end of the strip, 1 right, 2 left, 3 split
        if (!seen) vvis[h.v] = (uint8_t)(vm | 1u);
        if (!seen && !on_boundary) { sym = 0; move = 1; }
        else if (r_done) {
          if (h.rc != DSA_INVALID && !r_self) check_split(last_symbol_id, 1, R.mark);
          if (l_done) {
            if (h.lc != DSA_INVALID && !l_self) check_split(last_symbol_id, 0, L.mark);
            sym = 7; move = 0;
          } else { sym = 5; move = 2; }
        } else if (l_done) {
          if (h.lc != DSA_INVALID && !l_self) check_split(last_symbol_id, 0, L.mark);
          sym = 3; move = 1;
        } else {
          sym = 1; move = 3;
          ++nsplit_sym;
          if (on_boundary && !(vm & 8u)) encode_hole(corner, false);
          mark = (uint32_t)last_symbol_id + 2u;
        }
        fw[8 * f + EC_MARK] = mark;
        processed[nproc++] = corner | (sym << EC_SYMBOL_SHIFT);
        if (move == 1) { corner = h.rc; f = fr; cur = R; continue; }
        if (move == 2) { corner = h.lc; f = fl; cur = L; continue; }
        if (move == 3) {                                                          // (sp <= F by itself: every push marks a face first)
          if (sp >= F) { failed = true; break; }
          stack[sp - 1] = h.lc; stack[sp++] = h.rc;
        } else --sp;
        break;
      }
    }
  };
  for (uint32_t face = 0; !failed && nproc + ninit < F; ++face) {                 // :38-124 (every face is coded once: the scan is over when all are)
    face = next_fresh(face, EC_MARK);
    if (face >= F) break;
    // (the reference asks at each of the three corners of a face whether the face is still to do)
    for (int rep = 0; rep < 3 && !failed && fw[8 * face + EC_MARK] == 0; ++rep) {
      // find_init_face, :158-183
      uint32_t corner = 3 * face, start = DSA_INVALID;
      bool interior_face = true;
      for (int i = 0; i < 3; ++i) {
        if (opp[corner] == DSA_INVALID) { start = corner; interior_face = false; break; }
        if (vvis[c2v[corner]] & 2u) {
          uint32_t rc = corner;
          while (rc != DSA_INVALID && !runaway()) { corner = rc; rc = ct.swing_right(rc); }
          start = ec_prev(corner);
          interior_face = false;
          break;
        }
        corner = ec_next(corner);
      }
      if (interior_face) start = corner;
      start_bits[nstart++] = interior_face ? 1 : 0;
      if (interior_face) {
        vvis[c2v[start]] |= 1; vvis[c2v[ec_next(start)]] |= 1; vvis[c2v[ec_prev(start)]] |= 1;
        fw[8 * face + EC_MARK] = 1u;
        if (record_time && E->init_time) ((uint32_t *)(arena + E->init_time))[ninit] = nproc;
        init_corners[ninit++] = ec_next(start);
        const uint32_t o = opp[ec_next(start)];
        if (o != DSA_INVALID && fw[8 * (o / 3u) + EC_MARK] == 0) encode_from_corner(o);
      } else {
        encode_hole(ec_next(start), true);
        encode_from_corner(start);
      }
    }
  }
  if (failed) ec_fail(E, steps > step_limit ? ENC_RING : ENC_SPLITS, nsplit);
  E->num_symbols = nproc; E->num_start_bits = nstart; E->num_splits = nsplit; E->num_split_symbols = nsplit_sym;
  E->num_processed = nproc; E->num_init = ninit; E->interior_edges /= 2;
  if (failed) return;

  // ---- depth-first attribute order over the decoder's face order (processed corners last to first, then the init
  // corners), DepthFirstTraverser.cs:9-99.  A vertex is on a boundary -- SwingLeft of its left-most corner is invalid -- exactly
  // when it is the end of an edge without an opposite.  The marks of this walk are its own (mark2, bit 4 of a vertex).
  bool stuck = false;
  const uint32_t count = ec_dfs_walk(frec, fw, vvis, stack, d2c, v2d, processed, init_corners, nproc, ninit, F, V, step_limit, stuck);
  E->num_entries = count;
  if (stuck) ec_fail(E, ENC_RING, count);
  else if (count != V) ec_fail(E, ENC_UNREACHED, count);
}
__global__ __launch_bounds__(WAVE) void k_enc_connectivity(uint8_t *arena, EncConn *conns, uint32_t n, uint32_t lanes_per_wave) {
  ec_connectivity<false>(arena, conns, n, lanes_per_wave);
}
// the same for a chunk with meshes coded with valence symbols (dsa_encode_schemes.h)
__global__ __launch_bounds__(WAVE) void k_enc_connectivity_timed(uint8_t *arena, EncConn *conns, uint32_t n, uint32_t lanes_per_wave) {
  ec_connectivity<true>(arena, conns, n, lanes_per_wave);
}

// ---- the symbols as bytes; entry -> vertex and the parallelogram operand entries of every entry (MeshPredictionSchemeParallelogramEncoder.cs:35-56)
__global__ __launch_bounds__(256) void k_enc_operands(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  const uint32_t *opp = (const uint32_t *)(arena + E->opp), *d2c = (const uint32_t *)(arena + E->d2c);
  const int32_t *v2d = (const int32_t *)(arena + E->v2d);
  uint32_t *e2v = (uint32_t *)(arena + E->e2v);
  int32_t *ops = (int32_t *)(arena + E->ops);
  {
    const uint32_t *processed = (const uint32_t *)(arena + E->processed);
    uint8_t *symbols = arena + E->symbols;
    const uint32_t ns = E->num_symbols;
    for (uint32_t i = t0; i < ns; i += stride) symbols[i] = (uint8_t)(processed[i] >> EC_SYMBOL_SHIFT);
  }
  for (uint32_t p = t0; p < V; p += stride) {
    const uint32_t ci = d2c[p];
    e2v[p] = c2v[ci];
    int32_t on = -1, op = -1, oo = -1;
    if (p > 0) {
      const uint32_t oci = opp[ci];
      if (oci != DSA_INVALID) {
        const int32_t vo = v2d[c2v[oci]], vn = v2d[c2v[ec_next(oci)]], vp = v2d[c2v[ec_prev(oci)]];
        if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { on = vn; op = vp; oo = vo; }
      }
    }
    ops[3 * p] = on; ops[3 * p + 1] = op; ops[3 * p + 2] = oo;
  }
}

}  // namespace dsa
