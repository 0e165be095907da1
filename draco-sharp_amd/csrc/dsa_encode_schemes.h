// draco-sharp_amd/csrc/dsa_encode_schemes.h  (included by dsa_encode.h after dsa_encode_seams.h)
//
// Encode direction, the schemes stock encoders write at their default level (dsa_encode_batch_ex), each the device form of the
// CPU coder's function in dsa_encode_host.h, down to its integer arithmetic:
//   TexCoordsPortable       write_attribute_values, prediction 5   MeshPredictionSchemeTexCoordsPortableEncoder.cs +
//                                                                  ...PortablePredictor.cs                 enc_tex_portable, k_enc_orient
//   GeometricNormal         write_attribute_values, prediction 6   MeshPredictionSchemeGeometricNormalEncoder.cs +
//                                                                  ...PredictorArea.cs                     enc_geo_normal
//   valence context lists   valence_context_symbols                MeshEdgeBreakerTraversalValenceEncoder.cs
//                                                                  k_enc_val_init, k_enc_valence, k_enc_val_split, k_enc_list_stats
// The two predictions are one lane per entry inside k_enc_corr (dsa_encode.h).  Their inputs: the attribute's traversal-order
// values, the quantised positions in vertex order (the mesh's position stream), and a topology view -- corner -> position vertex,
// corner -> vertex of the attribute's table and that table's opposites, entry -> corner, vertex -> entry: the position table for a
// per-vertex attribute, the attribute's own (EncSeam c2av / opp2 / d2c / v2d) for a seamed one.  Their side bits (orientations,
// flips) leave the device packed, one bit per flag; the host's stream layout rABS-codes them (write_rabs).
// The valence pass is serial per mesh, one lane per mesh like the walks of k_enc_connectivity; its six context lists become six
// symbol streams of the mesh (EncStream kind 3) and go through k_enc_plan / k_enc_rans like every attribute stream.
#pragma once

namespace dsa {

struct EncTopo {                   // what the two predictions read of a mesh; pointers into the arena
  const int32_t *d;                // i32[entries * nc] traversal-order values
  const int32_t *pos;              // i32[V * 3] quantised positions, vertex order
  const uint32_t *c2p, *c2a, *opp; // u32[3F]: position vertex, attribute-table vertex, attribute-table opposite per corner
  const uint32_t *d2c;             // u32[entries] entry -> corner
  const int32_t *v2d;              // i32[attribute vertices] vertex -> entry
  uint32_t nc3;                    // 3F: bound of every corner index (a ring walk never takes more steps)
};

// Core/MathUtilities.cs:5-25
__device__ __forceinline__ uint64_t enc_isqrt(uint64_t number) {
  if (number == 0) return 0;
  uint64_t act = number, root = 1;
  while (act >= 2) { root *= 2; act /= 4; }
  do { root = (root + number / root) / 2; } while (root * root > number);
  return root;
}

// TexCoordsPortable prediction of entry p (MeshPredictionSchemeTexCoordsPortablePredictor.cs:46-150, encoder side: both
// candidates, the closer one wins).  ori: 0 the entry took no full branch, 2 / 3 it did with orientation false / true.
__device__ __forceinline__ void enc_tex_portable(const EncTopo &T, uint32_t p, int32_t pred[2], uint32_t &ori) {
  const int32_t data_id = (int32_t)p;
  const uint32_t ci = T.d2c[p];
  const int32_t next_id = T.v2d[T.c2a[ec_next(ci)]], prev_id = T.v2d[T.c2a[ec_prev(ci)]];
  auto P = [&](int32_t entry, int k) { return (int64_t)T.pos[(size_t)T.c2p[T.d2c[entry]] * 3 + k]; };
  pred[0] = 0; pred[1] = 0; ori = 0;
  if (prev_id >= 0 && next_id >= 0 && prev_id < data_id && next_id < data_id) {
    const int64_t n_uv[2] = {T.d[next_id * 2], T.d[next_id * 2 + 1]}, p_uv[2] = {T.d[prev_id * 2], T.d[prev_id * 2 + 1]};
    if (p_uv[0] == n_uv[0] && p_uv[1] == n_uv[1]) { pred[0] = (int32_t)p_uv[0]; pred[1] = (int32_t)p_uv[1]; return; }
    int64_t pn[3], cn[3], pd[3], pnx[3];
    for (int k = 0; k < 3; ++k) { pd[k] = P(data_id, k); pnx[k] = P(next_id, k); pn[k] = P(prev_id, k) - pnx[k]; cn[k] = pd[k] - pnx[k]; }
    const int64_t pn_norm2 = pn[0] * pn[0] + pn[1] * pn[1] + pn[2] * pn[2];
    if (pn_norm2 != 0) {
      const int64_t cn_dot_pn = pn[0] * cn[0] + pn[1] * cn[1] + pn[2] * cn[2];
      const int64_t pn_uv[2] = {p_uv[0] - n_uv[0], p_uv[1] - n_uv[1]};
      const int64_t x_uv[2] = {n_uv[0] * pn_norm2 + cn_dot_pn * pn_uv[0], n_uv[1] * pn_norm2 + cn_dot_pn * pn_uv[1]};
      int64_t cx[3];
      for (int k = 0; k < 3; ++k) cx[k] = pd[k] - (pnx[k] + (cn_dot_pn * pn[k]) / pn_norm2);
      const uint64_t cx_norm2 = (uint64_t)(cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2]);
      const int64_t norm = (int64_t)enc_isqrt(cx_norm2 * (uint64_t)pn_norm2);
      const int64_t cx_uv[2] = {pn_uv[1] * norm, -pn_uv[0] * norm};
      const int64_t c0[2] = {(x_uv[0] + cx_uv[0]) / pn_norm2, (x_uv[1] + cx_uv[1]) / pn_norm2};
      const int64_t c1[2] = {(x_uv[0] - cx_uv[0]) / pn_norm2, (x_uv[1] - cx_uv[1]) / pn_norm2};
      const int64_t u = T.d[p * 2], v = T.d[p * 2 + 1];
      const uint64_t e0 = (uint64_t)((u - c0[0]) * (u - c0[0]) + (v - c0[1]) * (v - c0[1]));
      const uint64_t e1 = (uint64_t)((u - c1[0]) * (u - c1[0]) + (v - c1[1]) * (v - c1[1]));
      if (e0 < e1) { pred[0] = (int32_t)c0[0]; pred[1] = (int32_t)c0[1]; ori = 3; }
      else { pred[0] = (int32_t)c1[0]; pred[1] = (int32_t)c1[1]; ori = 2; }
      return;
    }
  }
  int32_t data_offset = 0;
  bool zero = false;
  if (prev_id >= 0 && prev_id < data_id) data_offset = prev_id * 2;
  if (next_id >= 0 && next_id < data_id) data_offset = next_id * 2;
  else { if (data_id > 0) data_offset = (data_id - 1) * 2; else zero = true; }
  if (!zero) { pred[0] = T.d[data_offset]; pred[1] = T.d[data_offset + 1]; }
}

// PredictionSchemeNormalOctahedronCanonicalizedEncodingTransform.cs:47-83 (oct_canon_corr of the host coder)
__device__ __forceinline__ void enc_oct_canon_corr(int32_t center, int32_t max_q, int32_t os, int32_t ot, int32_t ps, int32_t pt, int32_t out[2]) {
  os -= center; ot -= center; ps -= center; pt -= center;
  const int32_t aps = ps < 0 ? -ps : ps, apt = pt < 0 ? -pt : pt;
  if (!((uint32_t)aps + (uint32_t)apt <= (uint32_t)center)) { oct_invert_diamond(center, os, ot); oct_invert_diamond(center, ps, pt); }
  const bool bottom_left = (ps == 0 && pt == 0) || (ps < 0 && pt <= 0);
  if (!bottom_left) {
    int rot;
    if (ps == 0) rot = pt == 0 ? 0 : (pt > 0 ? 3 : 1);
    else if (ps > 0) rot = pt >= 0 ? 2 : 1;
    else rot = pt <= 0 ? 0 : 3;
    oct_rotate(os, ot, rot); oct_rotate(ps, pt, rot);
  }
  out[0] = os - ps; out[1] = ot - pt;
  if (out[0] < 0) out[0] += max_q;
  if (out[1] < 0) out[1] += max_q;
}
// Octa::from_int_vector of the host coder
__device__ __forceinline__ void enc_oct_from_int(int32_t center, int32_t max_value, const int32_t v[3], int32_t &s, int32_t &t) {
  if (v[0] >= 0) { s = v[1] + center; t = v[2] + center; }
  else {
    s = v[1] < 0 ? abs(v[2]) : max_value - abs(v[2]);
    t = v[2] < 0 ? abs(v[1]) : max_value - abs(v[1]);
  }
  if ((s == 0 && t == 0) || (s == 0 && t == max_value) || (s == max_value && t == 0)) { s = max_value; t = max_value; }
  else if (s == 0 && t > center) t = center - (t - center);
  else if (s == max_value && t < center) t = center + (center - t);
  else if (t == max_value && s < center) s = center + (center - s);
  else if (t == 0 && s > center) s = center - (s - center);
}
// The tail of the octahedral quantiser (Octa::from_float_vector of the host coder from iv[2] on), shared by enc_oct_from_float and
// the mean normals (k_enc_normal_store): the code of the vector scaled to L1 norm `center` whose first two components rounded to
// i0 and i1 and whose third is negative or not.
__device__ __forceinline__ void enc_oct_from_scaled(int32_t center, int32_t max_value, int32_t i0, int32_t i1, bool z_negative, int32_t &s, int32_t &t) {
  int32_t i2 = center - abs(i0) - abs(i1);
  if (i2 < 0) { if (i1 > 0) i1 += i2; else i1 -= i2; i2 = 0; }
  if (z_negative) i2 = -i2;
  const int32_t v[3] = {i0, i1, i2};
  enc_oct_from_int(center, max_value, v, s, t);
}

// GeometricNormal correction of entry p (geometric_normal_prediction + the flip choice of write_attribute_values): the area-weighted
// ring of the entry's corner on the attribute's table, positions of the position table, 64-bit sums; the prediction or its
// negation, whichever leaves the smaller correction.  Returns false when the ring does not close within the mesh's corners.
__device__ __forceinline__ bool enc_geo_normal(const EncTopo &T, uint32_t p, int32_t bits, uint32_t sym[2], bool &flip) {
  const int32_t max_q = (1 << bits) - 1, max_value = max_q - 1, center = max_value / 2;
  const uint32_t ci = T.d2c[p];
  auto P = [&](uint32_t c, int k) { return (int64_t)T.pos[(size_t)T.c2p[c] * 3 + k]; };
  auto opposite = [&](uint32_t c) { return c == DSA_INVALID ? c : T.opp[c]; };
  auto swing_left = [&](uint32_t c) { return ec_next(opposite(ec_next(c))); };
  auto swing_right = [&](uint32_t c) { return ec_prev(opposite(ec_prev(c))); };
  const int64_t pc[3] = {P(ci, 0), P(ci, 1), P(ci, 2)};
  uint64_t n[3] = {0, 0, 0};
  uint32_t c = ci, steps = 0;
  bool left = true;
  while (c != DSA_INVALID) {
    if (++steps > T.nc3 + 1) return false;
    const uint32_t cn = ec_next(c), cp = ec_prev(c);
    uint64_t a[3], b[3];
    for (int k = 0; k < 3; ++k) { a[k] = (uint64_t)(P(cn, k) - pc[k]); b[k] = (uint64_t)(P(cp, k) - pc[k]); }
    n[0] += a[1] * b[2] - a[2] * b[1];
    n[1] += a[2] * b[0] - a[0] * b[2];
    n[2] += a[0] * b[1] - a[1] * b[0];
    if (left) {
      c = swing_left(c);
      if (c == DSA_INVALID) { c = swing_right(ci); left = false; }
      else if (c == ci) break;
    } else c = swing_right(c);
  }
  int64_t nv[3] = {(int64_t)n[0], (int64_t)n[1], (int64_t)n[2]};
  uint64_t as = 0;
  bool sat = false;
  for (int k = 0; k < 3; ++k) {
    const uint64_t x = nv[k] < 0 ? (uint64_t)0 - (uint64_t)nv[k] : (uint64_t)nv[k];
    if (x > (uint64_t)INT64_MAX || as > (uint64_t)INT64_MAX - x) sat = true; else as += x;
  }
  const int64_t abs_sum = sat ? INT64_MAX : (int64_t)as;
  const int64_t upper = (int64_t)1 << 29;
  if (abs_sum > upper) { const int64_t q = abs_sum / upper; for (int k = 0; k < 3; ++k) nv[k] /= q; }
  int32_t v3[3] = {(int32_t)nv[0], (int32_t)nv[1], (int32_t)nv[2]};
  const int64_t s3 = (v3[0] < 0 ? -(int64_t)v3[0] : (int64_t)v3[0]) + (v3[1] < 0 ? -(int64_t)v3[1] : (int64_t)v3[1]) + (v3[2] < 0 ? -(int64_t)v3[2] : (int64_t)v3[2]);
  if (s3 == 0) v3[0] = center;
  else {
    v3[0] = (int32_t)(((int64_t)v3[0] * center) / s3);
    v3[1] = (int32_t)(((int64_t)v3[1] * center) / s3);
    const int32_t rest = center - abs(v3[0]) - abs(v3[1]);
    v3[2] = v3[2] >= 0 ? rest : -rest;
  }
  int32_t pps, ppt, pns, pnt;
  enc_oct_from_int(center, max_value, v3, pps, ppt);
  const int32_t neg[3] = {-v3[0], -v3[1], -v3[2]};
  enc_oct_from_int(center, max_value, neg, pns, pnt);
  const int32_t os = T.d[2 * p], ot = T.d[2 * p + 1];
  int32_t cp[2], cn[2];
  enc_oct_canon_corr(center, max_q, os, ot, pps, ppt, cp);
  enc_oct_canon_corr(center, max_q, os, ot, pns, pnt, cn);
  auto mod_max = [&](int32_t x) { return x > center ? x - max_q : (x < -center ? x + max_q : x); };
  const int32_t wp = abs(mod_max(cp[0])) + abs(mod_max(cp[1])), wn = abs(mod_max(cn[0])) + abs(mod_max(cn[1]));
  flip = !(wp < wn);
  sym[0] = (uint32_t)(flip ? cn[0] : cp[0]); sym[1] = (uint32_t)(flip ? cn[1] : cp[1]);
  return true;
}

// TexCoordsPortable / GeometricNormal of a seamed attribute read the attribute's own table and order (else the positions', which
// the host set): one thread per (mesh, attribute given per corner), behind k_enc_seam_operands.
template <class Stream>
__global__ __launch_bounds__(256) void k_enc_seam_topo(const EncConn *conns, const EncSeam *seams, uint32_t ns, Stream *streams) {
  const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
  if (si >= ns) return;
  const EncSeam &S = seams[si];
  if (conns[S.mesh].status != ENC_OK || S.status != ENC_SEAM_OK || !S.interior_seams) return;
  Stream &T = streams[S.stream];
  T.t_c2a = S.c2av; T.t_opp = S.opp2; T.t_d2c = S.d2c; T.t_v2d = S.v2d;
}

// ---- valence context lists (valence_context_symbols), device path.  Regions of EncConn, written by -> last read by:
//   init_time  u32[F]    encoder time of every interior start face                 k_enc_connectivity (record_time) -> k_enc_val_init
//   vtime      u32[F]    face -> index of the first symbol coded with it visited  k_enc_val_init -> k_enc_valence
//   vval       i32[V+F]  valence per vertex (+ one per S: the split tip's right half) k_enc_val_init -> k_enc_valence
//   vc2v       u32[3F]   vertex per corner, split tips renumbered                   k_enc_val_init -> k_enc_valence
//   vctx       u8[F]     context (0 - 5) of the symbol before each one             k_enc_valence -> k_enc_val_split
//   vsyms, vbl u32[F], u8[F]  the six lists back to back (streams' syms / bl)     k_enc_val_split, k_enc_list_stats -> k_enc_rans
//   vrans, vbits u8[4F + 96] each: the six lists' coded bytes                     k_enc_rans -> download (stream layout)
__global__ __launch_bounds__(256) void k_enc_val_init(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  if (E->vstream == DSA_INVALID) return;
  const uint32_t *opp = (const uint32_t *)(arena + E->opp), *processed = (const uint32_t *)(arena + E->processed);
  const uint32_t *init = (const uint32_t *)(arena + E->init_corners), *init_time = (const uint32_t *)(arena + E->init_time);
  uint32_t *vtime = (uint32_t *)(arena + E->vtime), *vc2v = (uint32_t *)(arena + E->vc2v);
  int32_t *vval = (int32_t *)(arena + E->vval);
  const uint32_t np = E->num_processed < F ? E->num_processed : F, ni = E->num_init < F ? E->num_init : F;
  for (uint32_t c = t0; c < NC; c += stride) {
    const uint32_t v = c2v[c];
    vc2v[c] = v;
    atomicAdd((uint32_t *)&vval[v], opp[ec_prev(c)] == DSA_INVALID ? 2u : 1u);     // edges around a vertex: faces, +1 on a boundary
  }
  for (uint32_t i = t0; i < np; i += stride) vtime[(processed[i] & (uint32_t)EC_CORNER_MASK) / 3u] = i;
  for (uint32_t k = t0; k < ni; k += stride) vtime[init[k] / 3u] = init_time[k];
}

// One lane per mesh.  Symbol i (encoder order) stands at corner processed[i]; the context of the symbol before it is the valence
// of the vertex at next(corner) before the symbol's update.  At an S the fans left and right of the tip are walked to the first
// coded face: the left part keeps the vertex, the right part gets a new one.
__global__ __launch_bounds__(WAVE) void k_enc_valence(uint8_t *arena, EncConn *conns, uint32_t n, uint32_t lanes_per_wave) {
  if (threadIdx.x >= lanes_per_wave) return;
  const uint32_t mesh = blockIdx.x * lanes_per_wave + threadIdx.x;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK || E->vstream == DSA_INVALID) return;
  const uint32_t F = E->F, V = E->V, NC = 3u * F;
  const uint32_t *opp = (const uint32_t *)(arena + E->opp), *processed = (const uint32_t *)(arena + E->processed);
  const uint32_t *vtime = (const uint32_t *)(arena + E->vtime);
  uint32_t *vc2v = (uint32_t *)(arena + E->vc2v);
  int32_t *vval = (int32_t *)(arena + E->vval);
  uint8_t *vctx = arena + E->vctx;
  const uint32_t ns = E->num_symbols < F ? E->num_symbols : F;
  const uint32_t vcap = V + F;
  uint32_t count[6] = {0, 0, 0, 0, 0, 0};
  uint32_t nv = V, steps = 0;
  const uint32_t step_limit = 4u * NC + 4096u;
  int32_t prev_symbol = -1;
  bool failed = false;
  for (uint32_t i = 0; i < ns && !failed; ++i) {
    const uint32_t w = processed[i], corner = w & (uint32_t)EC_CORNER_MASK, symbol = w >> EC_SYMBOL_SHIFT;
    const uint32_t nx = ec_next(corner), pv = ec_prev(corner);
    const uint32_t a_nx = vc2v[nx], a_pv = vc2v[pv], a_c = vc2v[corner];
    const int32_t active_valence = vval[a_nx];
    if (symbol == 0) { vval[a_nx] -= 1; vval[a_pv] -= 1; }
    else if (symbol == 1) {
      vval[a_nx] -= 1; vval[a_pv] -= 1;
      int32_t left = 0, right = 0;
      uint32_t a = opp[pv];
      while (a != DSA_INVALID && vtime[a / 3u] > i) { ++left; a = opp[ec_next(a)]; if (++steps > step_limit) { failed = true; break; } }
      vval[a_c] = left + 1;
      if (nv >= vcap) { failed = true; break; }
      a = opp[nx];
      while (a != DSA_INVALID && vtime[a / 3u] > i) { ++right; vc2v[ec_next(a)] = nv; a = opp[ec_prev(a)]; if (++steps > step_limit) { failed = true; break; } }
      vval[nv] = right + 1;
      ++nv;
    } else if (symbol == 5) { vval[a_c] -= 1; vval[a_nx] -= 1; vval[a_pv] -= 2; }
    else if (symbol == 3) { vval[a_c] -= 1; vval[a_nx] -= 2; vval[a_pv] -= 1; }
    else { vval[a_c] -= 2; vval[a_nx] -= 2; vval[a_pv] -= 2; }
    if (prev_symbol != -1) {
      const int32_t clamped = active_valence < 2 ? 2 : (active_valence > 7 ? 7 : active_valence);
      vctx[i - 1] = (uint8_t)(clamped - 2);
      ++count[clamped - 2];
    }
    prev_symbol = (int32_t)symbol;
  }
  if (failed) { ec_fail(E, ENC_RING, 0); return; }
  for (int k = 0; k < 6; ++k) E->vcount[k] = count[k];
}

// One wave per mesh: the symbols (ids C 0, S 1, L 2, R 3, E 4) into their six lists, stably, and the six streams' regions: the lists
// lie back to back in vsyms / vbl, their coded bytes in vrans / vbits at 4 bytes per symbol + 16 each.
template <class Stream>
__global__ __launch_bounds__(WAVE) void k_enc_val_split(uint8_t *arena, EncConn *conns, uint32_t n, Stream *streams) {
  const uint32_t mesh = blockIdx.x, lane = threadIdx.x;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK || E->vstream == DSA_INVALID) return;
  const uint32_t *processed = (const uint32_t *)(arena + E->processed);
  const uint8_t *vctx = arena + E->vctx;
  uint32_t *vsyms = (uint32_t *)(arena + E->vsyms);
  uint32_t base[6], off = 0;
  for (int k = 0; k < 6; ++k) {
    base[k] = off;
    if (lane == 0) {
      Stream &S = streams[E->vstream + k];
      S.nv = E->vcount[k];
      S.syms = E->vsyms + 4ull * off; S.bl = E->vbl + off;
      S.out_cap = 4u * E->vcount[k] + 16u;
      S.out_rans = E->vrans + 4ull * off + 16ull * k; S.out_bits = E->vbits + 4ull * off + 16ull * k;
    }
    off += E->vcount[k];
  }
  const uint32_t total = E->num_symbols ? E->num_symbols - 1u : 0u;
  if (off != total) { if (lane == 0) ec_fail(E, ENC_RING, off); return; }
  static constexpr uint32_t id_of[8] = {0, 1, 0, 2, 0, 3, 0, 4};
#if defined(__HIPCC__)
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t i0 = 0; i0 < total; i0 += WAVE) {
    const uint32_t i = i0 + lane;
    const bool in = i < total;
    const uint32_t k = in ? vctx[i] : 6u, v = in ? id_of[(processed[i] >> EC_SYMBOL_SHIFT) & 7u] : 0u;
    for (uint32_t j = 0; j < 6; ++j) {
      const uint64_t m = __ballot(k == j);
      if (k == j) vsyms[base[j] + (uint32_t)__popcll(m & below)] = v;
      base[j] += (uint32_t)__popcll(m);
    }
  }
#else       // the sanitizer build of tests/hostcheck runs the lanes of a wave one after the other: lane 0 scatters
  if (lane == 0)
    for (uint32_t i = 0; i < total; ++i) { const uint32_t k = vctx[i]; if (k < 6) vsyms[base[k]++] = id_of[(processed[i] >> EC_SYMBOL_SHIFT) & 7u]; }
#endif
}

}  // namespace dsa
