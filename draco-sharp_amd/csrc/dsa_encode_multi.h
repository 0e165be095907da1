// draco-sharp_amd/csrc/dsa_encode_multi.h  (included by dsa_encode.h after dsa_encode_schemes.h)
//
// Encode direction, the two rungs of the reference's speed ladder above its default level (dsa_encode_level_batch), each the
// device form of the CPU coder's function in dsa_encode_host.h, down to its integer arithmetic:
//   MultiParallelogram (2), ConstrainedMultiParallelogram (4)
//                           write_attribute_values, prediction 2 / 4   MeshPredictionSchemeMultiParallelogramEncoder.cs,
//                                                                      ...ConstrainedMultiParallelogramEncoder.cs      k_enc_multi, k_enc_crease
//   prediction-degree order prediction_degree_sequence                  Traverser/MaxPredictionDegreeTraverser.cs:22-152  k_enc_pd_walk, k_enc_pd_operands,
//                                                                                                                      k_enc_pd_corner_streams
// k_enc_multi is one thread per entry over the topology view of dsa_encode_schemes.h (EncTopo): the position table for a per-vertex
// attribute (and one given per corner without interior seams), the attribute's own for a seamed one.  The constrained scheme's
// choice of crease flags is the CPU coder's -- per entry the subset of its (up to four) parallelograms with the smallest wrapped
// correction, the first such mask in ascending order -- which is independent per entry.  Symbols, bit lengths and statistics
// come out as k_enc_corr leaves them, so k_enc_plan / k_enc_rans run unchanged behind it.  The crease flags of an entry with
// `found` parallelograms go to list found - 1 in entry order: k_enc_multi leaves found and the flags per entry, k_enc_crease (one
// wave per stream) compacts them stably into four packed bit lists, which the host's stream layout rABS-codes (write_rabs).
// The prediction-degree walk is serial per mesh, one lane per mesh like the walks of k_enc_connectivity, behind them on their stream.
// The kernels are templates over the stream record (EncStream of dsa_encode.h; tests/hostcheck/encmulti_host.cpp has its own).
#pragma once

namespace dsa {

static const uint32_t EM_HIST_CAP_LIMIT = (1u << 18) + 2u;      // ENC_HIST_CAP_LIMIT of dsa_encode.h (which asserts that they agree)

__device__ __forceinline__ uint32_t em_zigzag(int32_t v) { return v >= 0 ? (uint32_t)v << 1 : (((uint32_t)(-(v + 1))) << 1) | 1u; }

// ---- symbol statistics of an attribute stream as k_enc_corr (dsa_encode.h) gathers them: the block counts its symbols in LDS and
// adds what it counted to the stream's histogram once; bit-length tags, the largest symbol and the total bit length likewise.
// k_enc_corr keeps its own text of the same steps: routed through these helpers it compiled to 102 scalar registers instead of
// 100, one wave per SIMD less by the compiler's count (7 against 8), in three arrangements of the helpers; the kernel of the
// default path is not given up for that.  Whoever changes one changes the other: tests/test_gpu_encode_level.py and the host
// check compare k_enc_multi's statistics with symbol_stats of the host coder, tests/test_gpu_encode.py those of k_enc_corr.
static const uint32_t ENC_LDS_HIST = 4098u;
struct EncStats { uint32_t *hist, *tag, *max; unsigned long long *bl; };      // the block's counters in LDS: u32[ENC_LDS_HIST], u32[33], one each
#define ENC_STATS_LDS(name)                                                                              \
  __shared__ uint32_t name##_tag[33];                                                                    \
  __shared__ uint32_t name##_max;                                                                        \
  __shared__ unsigned long long name##_bl;                                                               \
  __shared__ uint32_t name##_hist[dsa::ENC_LDS_HIST];                                                    \
  const dsa::EncStats name{name##_hist, name##_tag, &name##_max, &name##_bl};
// clears the block's counters; returns whether the stream's alphabet is counted in LDS
template <class Stream>
__device__ __forceinline__ bool enc_stats_begin(const EncStats &sh, const Stream &S) {
  const bool lds_hist = S.hist_cap <= ENC_LDS_HIST;
  if (lds_hist) for (uint32_t i = threadIdx.x; i < S.hist_cap; i += blockDim.x) sh.hist[i] = 0;
  if (threadIdx.x < 33) sh.tag[threadIdx.x] = 0;
  if (threadIdx.x == 0) { *sh.max = 0; *sh.bl = 0; }
#if defined(__HIPCC__)
  __syncthreads();
#endif
  return lds_hist;
}
// one symbol; beyond_ok: a symbol outside a histogram of the largest size is no overflow (max_value tells k_enc_plan)
template <class Stream>
__device__ __forceinline__ void enc_stats_symbol(const EncStats &sh, Stream &S, uint32_t *hist, bool lds_hist, bool beyond_ok, uint32_t sy) {
  if (sy < S.hist_cap) atomicAdd(lds_hist ? &sh.hist[sy] : &hist[sy], 1u); else if (!beyond_ok) S.overflow = 1;
}
// one entry whose largest symbol is mc: its bit length
__device__ __forceinline__ void enc_stats_entry(const EncStats &sh, uint8_t *bl, uint32_t p, uint32_t mc) {
  const uint32_t b = (mc > 0 ? 31u - (uint32_t)__builtin_clz(mc) : 0u) + 1u;
  bl[p] = (uint8_t)b;
  atomicAdd(&sh.tag[b], 1u);
  atomicMax(sh.max, mc);
  atomicAdd(sh.bl, (unsigned long long)b);
}
// what the block counted -> the stream
template <class Stream>
__device__ __forceinline__ void enc_stats_end(const EncStats &sh, Stream &S, uint32_t *hist, bool lds_hist) {
#if defined(__HIPCC__)
  __syncthreads();
  if (lds_hist) for (uint32_t i = threadIdx.x; i < S.hist_cap; i += blockDim.x) { const uint32_t c = sh.hist[i]; if (c) atomicAdd(&hist[i], c); }
  if (threadIdx.x < 33 && sh.tag[threadIdx.x]) atomicAdd(&S.hist_tag[threadIdx.x], sh.tag[threadIdx.x]);
  if (threadIdx.x == 0) { atomicMax(&S.max_value, *sh.max); atomicAdd(&S.total_bl, *sh.bl); }
#else       // the sanitizer build of tests/hostcheck runs the threads of a block one after the other: every thread adds what it
            // counted and leaves the block's counters at zero for the next
  if (lds_hist) for (uint32_t i = 0; i < S.hist_cap; ++i) { const uint32_t c = sh.hist[i]; if (c) atomicAdd(&hist[i], c); sh.hist[i] = 0; }
  for (uint32_t i = 0; i < 33; ++i) { if (sh.tag[i]) atomicAdd(&S.hist_tag[i], sh.tag[i]); sh.tag[i] = 0; }
  atomicMax(&S.max_value, *sh.max); S.total_bl += *sh.bl;
  *sh.max = 0; *sh.bl = 0;
#endif
}

struct EmWrap {                    // WrapEnc of the host coder
  int32_t mn, mx, max_dif, max_corr, min_corr;
  __device__ __forceinline__ void init(int32_t lo, int32_t hi) {
    mn = lo; mx = hi; max_dif = 1 + mx - mn; max_corr = max_dif / 2; min_corr = -max_corr;
    if ((max_dif & 1) == 0) max_corr -= 1;
  }
  __device__ __forceinline__ int32_t corr(int32_t orig, int32_t pred) const {
    const int32_t p = pred > mx ? mx : (pred < mn ? mn : pred);
    int32_t c = orig - p;
    if (c < min_corr) c += max_dif; else if (c > max_corr) c -= max_dif;
    return c;
  }
};

// The parallelogram across corner c for entry p: next + prev - opposite of the face behind the edge, in uint32 arithmetic, when all
// three entries precede p.
__device__ __forceinline__ bool em_para(const EncTopo &T, uint32_t p, uint32_t c, uint32_t nc, int32_t *out) {
  const uint32_t oci = T.opp[c];
  if (oci == DSA_INVALID) return false;
  const int32_t vo = T.v2d[T.c2a[oci]], vn = T.v2d[T.c2a[ec_next(oci)]], vp = T.v2d[T.c2a[ec_prev(oci)]];
  if (!(vo >= 0 && vn >= 0 && vp >= 0 && vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p)) return false;
  for (uint32_t k = 0; k < nc; ++k)
    out[k] = (int32_t)((uint32_t)T.d[(size_t)vn * nc + k] + (uint32_t)T.d[(size_t)vp * nc + k] - (uint32_t)T.d[(size_t)vo * nc + k]);
  return true;
}

// Prediction of entry p >= 1 by method 2 / 4 (write_attribute_values lines "a.prediction == 2 || a.prediction == 4").  crease: found
// in bits 0-2, flag i (1 = parallelogram i dropped) in bit 4 + i.  Returns false when a ring walk took more steps than the mesh has
// corners (a table that is no manifold's; the mesh then fails alone).
__device__ __forceinline__ bool em_predict(const EncTopo &T, const EmWrap &wr, uint32_t p, uint32_t nc, uint32_t method, int32_t *pred, uint32_t &crease) {
  auto swing_left = [&](uint32_t c) { const uint32_t o = T.opp[ec_next(c)]; return ec_next(o); };
  auto swing_right = [&](uint32_t c) { const uint32_t o = T.opp[ec_prev(c)]; return ec_prev(o); };
  const uint32_t start = T.d2c[p];
  const int32_t *dp = T.d + (size_t)p * nc, *dq = T.d + (size_t)(p - 1) * nc;
  uint32_t c = start, steps = 0;
  int32_t found = 0;
  crease = 0;
  for (uint32_t k = 0; k < nc; ++k) pred[k] = dq[k];
  if (method == 2) {
    int32_t cand[4], sum[4] = {0, 0, 0, 0};
    while (c != DSA_INVALID) {
      if (++steps > T.nc3 + 1u) return false;
      if (em_para(T, p, c, nc, cand)) { for (uint32_t k = 0; k < nc; ++k) sum[k] = (int32_t)((uint32_t)sum[k] + (uint32_t)cand[k]); ++found; }
      c = swing_right(c);
      if (c == start) c = DSA_INVALID;
    }
    if (found) for (uint32_t k = 0; k < nc; ++k) pred[k] = sum[k] / found;
    return true;
  }
  int32_t cand[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  bool first_pass = true;
  while (c != DSA_INVALID) {
    if (++steps > T.nc3 + 1u) return false;
    int32_t one[4];
    if (em_para(T, p, c, nc, one)) {                           // (kept by compare-and-select: an index by `found` would put the candidates in scratch memory)
#pragma unroll
      for (int32_t i = 0; i < 4; ++i)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (i == found && k < nc) cand[i][k] = one[k];
      if (++found == 4) break;
    }
    c = first_pass ? swing_left(c) : swing_right(c);
    if (c == start) break;
    if (c == DSA_INVALID && first_pass) { first_pass = false; c = swing_right(start); }
  }
  if (!found) return true;
  long long best_cost = -1;
  uint32_t best_mask = 0;
  for (uint32_t mask = 0; mask < (1u << found); ++mask) {      // bit i set: parallelogram i is used
    const int32_t used = (int32_t)__builtin_popcount(mask);
    long long cost = 0;
    for (uint32_t k = 0; k < nc; ++k) {
      uint32_t s = 0;
#pragma unroll
      for (int32_t i = 0; i < 4; ++i) if (i < found && ((mask >> i) & 1u)) s += (uint32_t)cand[i][k];
      const int32_t cr = wr.corr(dp[k], used ? (int32_t)s / used : dq[k]);
      cost += cr < 0 ? -(long long)cr : (long long)cr;
    }
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_mask = mask; }
  }
  const int32_t used = (int32_t)__builtin_popcount(best_mask);
  if (used)
    for (uint32_t k = 0; k < nc; ++k) {
      uint32_t s = 0;
#pragma unroll
      for (int32_t i = 0; i < 4; ++i) if (i < found && ((best_mask >> i) & 1u)) s += (uint32_t)cand[i][k];
      pred[k] = (int32_t)s / used;
    }
  crease = (uint32_t)found | ((~best_mask & ((1u << found) - 1u)) << 4);
  return true;
}

// corrections -> symbols, per-entry bit lengths, statistics of the streams predicted by method 2 / 4 (kind 0 quantised values, kind 2
// integers); the statistics through enc_stats_* above.
template <class Stream>
__global__ __launch_bounds__(256) void k_enc_multi(uint8_t *arena, Stream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.y;
  if (si >= ns) return;
  Stream &S = streams[si];
  if (S.kind == 1 || S.kind == 3 || (S.prediction != 2 && S.prediction != 4)) return;
  ENC_STATS_LDS(sh)
  const bool lds_hist = enc_stats_begin(sh, S);
  const bool beyond_ok = S.kind == 2 && S.hist_cap == EM_HIST_CAP_LIMIT;
  uint32_t *syms = (uint32_t *)(arena + S.syms);
  uint8_t *bl = arena + S.bl;
  uint32_t *hist = (uint32_t *)(arena + S.hist_raw);
  const uint32_t nc = S.nc < 4u ? S.nc : 4u, method = S.prediction;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  EmWrap wr;
  wr.init(S.wrap_mn, S.wrap_mx);
  EncTopo T;
  T.d = (const int32_t *)(arena + S.d); T.pos = nullptr; T.c2p = nullptr;
  T.c2a = (const uint32_t *)(arena + S.t_c2a); T.opp = (const uint32_t *)(arena + S.t_opp);
  T.d2c = (const uint32_t *)(arena + S.t_d2c); T.v2d = (const int32_t *)(arena + S.t_v2d); T.nc3 = S.t_nc3;
  uint8_t *crease = arena + S.ori;
  for (uint32_t p = tid; p < S.nv; p += stride) {
    int32_t pred[4] = {0, 0, 0, 0};
    uint32_t cr = 0, mc = 0;
    if (p > 0 && !em_predict(T, wr, p, nc, method, pred, cr)) { S.overflow = 1; cr = 0; }
    if (method == 4) crease[p] = (uint8_t)cr;
    for (uint32_t c = 0; c < nc; ++c) {
      const uint32_t sy = em_zigzag(wr.corr(T.d[(size_t)p * nc + c], pred[c]));
      syms[(size_t)p * nc + c] = sy;
      enc_stats_symbol(sh, S, hist, lds_hist, beyond_ok, sy);
      mc = sy > mc ? sy : mc;
    }
    enc_stats_entry(sh, bl, p, mc);
  }
  enc_stats_end(sh, S, hist, lds_hist);
}

// The crease flags of ConstrainedMultiParallelogram, four bit lists per stream in entry order: list j holds the j + 1 flags of every
// entry that found j + 1 parallelograms.  One wave per stream, 64 entries a round: the lanes of a list find their place by a ballot
// (k_enc_val_split's pattern) and set their flags with atomics into the packed words at flags + 4 * cr_at[j]; cr_n[j]: bits of list j.
template <class Stream>
__global__ __launch_bounds__(WAVE) void k_enc_crease(uint8_t *arena, Stream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x, lane = threadIdx.x;
  if (si >= ns) return;
  Stream &S = streams[si];
  if (S.kind == 1 || S.kind == 3 || S.prediction != 4 || S.overflow) return;
  const uint8_t *crease = arena + S.ori;
  uint32_t *flags = (uint32_t *)(arena + S.flags);
  const uint32_t nv = S.nv;
  uint32_t base[4] = {0, 0, 0, 0};
  const uint32_t at0 = S.cr_at[0], at1 = S.cr_at[1], at2 = S.cr_at[2], at3 = S.cr_at[3];
#if defined(__HIPCC__)
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t r0 = 0; r0 < nv; r0 += WAVE) {
    const uint32_t e = r0 + lane;
    const uint32_t b = e < nv ? crease[e] : 0u, found = b & 7u, drop = b >> 4;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint64_t m = __ballot(found == j + 1u);
      if (found == j + 1u) {
        const uint32_t at = base[j] + (uint32_t)__popcll(m & below) * (j + 1u), w0 = j == 0 ? at0 : (j == 1 ? at1 : (j == 2 ? at2 : at3));
        for (uint32_t i = 0; i <= j; ++i) if ((drop >> i) & 1u) atomicOr(&flags[w0 + ((at + i) >> 5)], 1u << ((at + i) & 31u));
      }
      base[j] += (uint32_t)__popcll(m) * (j + 1u);
    }
  }
#else
  if (lane == 0)
    for (uint32_t e = 0; e < nv; ++e) {
      const uint32_t b = crease[e], found = b & 7u, drop = b >> 4;
      if (found < 1u || found > 4u) continue;
      const uint32_t j = found - 1u, w0 = j == 0 ? at0 : (j == 1 ? at1 : (j == 2 ? at2 : at3));
      for (uint32_t i = 0; i <= j; ++i) { const uint32_t at = base[j] + i; if ((drop >> i) & 1u) flags[w0 + (at >> 5)] |= 1u << (at & 31u); }
      base[j] += found;
    }
#endif
  if (lane == 0) for (uint32_t j = 0; j < 4; ++j) S.cr_n[j] = base[j];
}

// word offsets of the four crease lists inside a stream's `flags` region for `cap` entries at most; returns the words in all
static inline uint32_t em_crease_words(uint32_t cap, uint32_t at[4]) {
  uint64_t w = 0;
  for (uint32_t j = 0; j < 4; ++j) { at[j] = (uint32_t)w; w += ((uint64_t)(j + 1u) * cap + 31u) / 32u; }
  return (uint32_t)w;
}

// ---- prediction-degree order (prediction_degree_sequence of the host coder) on the face records of the connectivity walk, one lane.
// Three priority stacks threaded through one word per corner (traverse_prediction_degree of dsa_general.h): a corner is pushed by
// the face across its edge, once, and as a start corner only while all three stacks are empty, so it is in one list at a time.
// Marks of its own: fvis u8[F], mark 16 (bit 4) of a vertex's mark byte; degree u32[V] (both zero on entry).  Returns the vertices visited.
__device__ __forceinline__ uint32_t ec_pd_walk(const uint4 *frec, uint8_t *fvis, uint8_t *vvis, uint32_t *next, uint32_t *degree, uint32_t *d2c, int32_t *v2d,
                                               const uint32_t *processed, const uint32_t *init_corners, uint32_t nproc, uint32_t ninit,
                                               uint32_t F, uint32_t V, uint32_t step_limit, bool &stuck) {
  const uint32_t END = 0xFFFFFFFDu, nstarts = nproc + ninit;
  uint32_t h0 = END, h1 = END, h2 = END, best = 0, count = 0, steps = 0;
  auto visit = [&](uint32_t v, uint32_t vm, uint32_t c) { vvis[v] = (uint8_t)(vm | 16u); v2d[v] = (int32_t)count; if (count < V) d2c[count] = c; ++count; };
  auto push = [&](uint32_t c, uint32_t pr) {
    if (pr == 0) { next[c] = h0; h0 = c; } else if (pr == 1) { next[c] = h1; h1 = c; } else { next[c] = h2; h2 = c; }
    if (pr < best) best = pr;
  };
  auto pop = [&]() -> uint32_t {
    if (best == 0 && h0 != END) { const uint32_t c = h0; h0 = next[c]; return c; }
    if (best <= 1 && h1 != END) { const uint32_t c = h1; h1 = next[c]; best = 1; return c; }
    if (h2 != END) { const uint32_t c = h2; h2 = next[c]; best = 2; return c; }
    return DSA_INVALID;
  };
  auto tip_of = [](const EcFace &r, uint32_t k) { return k == 0 ? r.v0 : (k == 1 ? r.v1 : r.v2); };
  for (uint32_t i = 0; i < nstarts && !stuck && count <= V; ++i) {
    const uint32_t start = i < nproc ? processed[nproc - 1 - i] & (uint32_t)EC_CORNER_MASK : init_corners[i - nproc];
    if (start >= 3u * F || fvis[start / 3u]) continue;                  // (a start whose face is done would be pushed, popped and dropped)
    push(start, 0);
    best = 0;
    {
      const EcFace sf = ec_face(frec, start / 3u);
      const uint32_t k = start - 3u * (start / 3u);
      const uint32_t nvx = k == 0 ? sf.v1 : (k == 1 ? sf.v2 : sf.v0), pvx = k == 0 ? sf.v2 : (k == 1 ? sf.v0 : sf.v1), tvx = tip_of(sf, k);
      { const uint32_t m = vvis[nvx]; if (!(m & 16u)) visit(nvx, m, ec_next(start)); }
      { const uint32_t m = vvis[pvx]; if (!(m & 16u)) visit(pvx, m, ec_prev(start)); }
      { const uint32_t m = vvis[tvx]; if (!(m & 16u)) visit(tvx, m, start); }
    }
    for (;;) {
      if (++steps > step_limit) { stuck = true; break; }
      uint32_t corner = pop();
      if (corner == DSA_INVALID) break;
      uint32_t f = corner / 3u;
      if (fvis[f]) continue;
      EcFace cur = ec_face(frec, f);
      for (;;) {
        if (++steps > step_limit || count > V) { stuck = true; break; }
        fvis[f] = 1;
        const EcHop h = ec_hop(cur, corner - 3u * f);
        const uint32_t fr = h.rc == DSA_INVALID ? 0u : h.rc / 3u, fl = h.lc == DSA_INVALID ? 0u : h.lc / 3u;
        const uint32_t vm = vvis[h.v];
        const EcFace R = ec_face(frec, fr), L = ec_face(frec, fl);
        const bool rdone = h.rc == DSA_INVALID || fr == f || fvis[fr] != 0, ldone = h.lc == DSA_INVALID || fl == f || fvis[fl] != 0;
        if (!(vm & 16u)) visit(h.v, vm, corner);
        if (!ldone) {
          const uint32_t tip = tip_of(L, h.lc - 3u * fl);
          const uint32_t pr = (vvis[tip] & 16u) ? 0u : (++degree[tip] > 1u ? 1u : 2u);
          if (rdone && pr <= best) { corner = h.lc; f = fl; cur = L; continue; }
          push(h.lc, pr);
        }
        if (!rdone) {
          const uint32_t tip = tip_of(R, h.rc - 3u * fr);
          const uint32_t pr = (vvis[tip] & 16u) ? 0u : (++degree[tip] > 1u ? 1u : 2u);
          if (pr <= best) { corner = h.rc; f = fr; cur = R; continue; }
          push(h.rc, pr);
        }
        break;
      }
      if (stuck) break;
    }
  }
  return count;
}

// Lane l of block b walks mesh b * lanes_per_wave + l, behind k_enc_connectivity on its stream; only the meshes of the chunk that ask
// for the order (pd_d2c set).  A walk that does not end within the step limit of the depth-first walk fails its mesh with ENC_RING.
__global__ __launch_bounds__(WAVE) void k_enc_pd_walk(uint8_t *arena, EncConn *conns, uint32_t n, uint32_t lanes_per_wave) {
  if (threadIdx.x >= lanes_per_wave) return;
  const uint32_t mesh = blockIdx.x * lanes_per_wave + threadIdx.x;
  if (mesh >= n) return;
  EncConn *E = &conns[mesh];
  if (E->status != ENC_OK || !E->pd_d2c) return;
  const uint32_t F = E->F, V = E->V;
  bool stuck = false;
  const uint32_t count = ec_pd_walk((const uint4 *)(arena + E->frec), arena + E->pd_fvis, arena + E->vvis, (uint32_t *)(arena + E->pd_next), (uint32_t *)(arena + E->pd_degree),
                                    (uint32_t *)(arena + E->pd_d2c), (int32_t *)(arena + E->pd_v2d), (const uint32_t *)(arena + E->processed),
                                    (const uint32_t *)(arena + E->init_corners), E->num_processed < F ? E->num_processed : F, E->num_init < F ? E->num_init : F,
                                    F, V, 64u * 3u * F + 4096u, stuck);
  if (stuck) ec_fail(E, ENC_RING, count);
  else if (count != V) ec_fail(E, ENC_UNREACHED, count);
}

// entry -> vertex and the parallelogram operand entries of the second order (k_enc_operands for d2c / v2d of the prediction-degree walk)
__global__ __launch_bounds__(256) void k_enc_pd_operands(uint8_t *arena, EncConn *conns, uint32_t n) {
  ENC_TABLE_PROLOGUE
  if (!E->pd_d2c) return;
  const uint32_t *opp = (const uint32_t *)(arena + E->opp), *d2c = (const uint32_t *)(arena + E->pd_d2c);
  const int32_t *v2d = (const int32_t *)(arena + E->pd_v2d);
  uint32_t *e2v = (uint32_t *)(arena + E->pd_e2v);
  int32_t *ops = (int32_t *)(arena + E->pd_ops);
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

// An attribute given per corner that turned out to have no interior seam is coded per vertex through its ids (k_enc_seam_operands:
// the positions' depth-first order); where its decoder takes the prediction-degree order (stream.pd_want), its value rows and
// operands follow the second order instead.  Behind k_enc_seam_operands and k_enc_pd_operands.
template <class Stream>
__global__ __launch_bounds__(256) void k_enc_pd_corner_streams(uint8_t *arena, const EncConn *conns, EncSeam *seams, uint32_t ns, Stream *streams) {
  ENC_SEAM_PROLOGUE
  Stream &T = streams[S->stream];
  if (S->interior_seams || !T.pd_want || !E->pd_d2c) return;
  if (t0 == 0) T.ops = E->pd_ops;
  uint32_t *e2v = (uint32_t *)(arena + S->e2v);
  const uint32_t *d2c = (const uint32_t *)(arena + E->pd_d2c);
  for (uint32_t p = t0; p < V; p += stride) e2v[p] = es_id(arena, *S, d2c[p]);
}

}  // namespace dsa
