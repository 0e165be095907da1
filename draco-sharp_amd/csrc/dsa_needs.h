// draco-sharp_amd/csrc/dsa_needs.h
// Which kernel takes which attribute, written once for the kernels (dsa_kernels.h, dsa_seams.h), for k_seal and for the host parse
// (dsa_host_parse.h): the predicates the symbol, prediction and dequantisation kernels select their work by, and the per-mesh
// "need" bits derived from them.  dsa_batch_decode launches a kernel of the groups below only when the host parse found a mesh of
// the batch that needs it; k_seal derives the same bits from the descriptors the device parse filled and refuses a mesh whose needs
// the launched set does not cover, so the two parses cannot disagree silently.  Plain C++ over AttrDesc / MeshLayout: no HIP.
#pragma once
#include "dsa_common.h"

#if defined(__HIPCC__)
#define DSA_HD __host__ __device__ __forceinline__
#else
#define DSA_HD inline
#endif

namespace dsa {

#define SYM_MAX_LDS 4032      // 63 blocks of 64 cumulative entries searched in LDS by k_symbols
#define REG_MAX_SYMS 4096     // a 12-bit-precision table has 4096 slots: no more symbols than that can have a frequency
#define WIDE_MAX_SYMS 2048    // k_symbols_wide: 32 registers of 64 {cumulative, frequency} words

// The symbol kernels are launched twice when the batch is decoded on four streams: once for the attributes whose prediction
// waits for the traversal (parallelogram: "late") and once, on a stream of higher priority that goes on to predict and
// dequantise them, for those whose prediction does not ("early": difference, octahedral delta, none).
#define SYM_WIDE 0x800u        // k_symbols_wide is part of the launch set (DSA_SYM_WIDE=0: its streams stay with the LDS tiers)
#define SYM_EARLY_ONLY 0x100u
#define SYM_LATE_ONLY 0x200u
#define SYM_CORNER 0x1000u     // the launch for corner attributes (behind k_seam_tables, which counts their entries); every other launch skips them
// late prediction of a batch with corner attributes, in two launches: what only waits for the position traversal / what waits for
// the seam tables and the attribute traversals as well
#define PRED_FRONT 0x10000u
#define PRED_BEHIND 0x20000u
#define PW_FLAG 4u             // DSA_LANES bit 2: wrap schemes by k_predict_wrap (default on)
#define OS_FLAG 16u            // the canonicalised octahedral delta is k_predict_oct_streams' (crowded batches)

DSA_HD bool att_behind_tables(const AttrDesc &a) { return a.corner_data != 0 || a.late_located != 0; }
DSA_HD bool att_is_late(const AttrDesc &a) { return (a.have_scheme && a.pred_kind != 0) || att_behind_tables(a); }
DSA_HD bool pred_filtered(const AttrDesc &a, uint32_t flags) {
  return ((flags & PRED_FRONT) && att_behind_tables(a)) || ((flags & PRED_BEHIND) && !att_behind_tables(a));
}
// the symbol launch an attribute's stream belongs to: 0 early, 1 late, 2 corner
DSA_HD uint32_t sym_group_of(const AttrDesc &a) {
  if (att_behind_tables(a)) return 2u;
  return (a.have_scheme && a.pred_kind != 0) ? 1u : 0u;     // parallelogram, geometric normal, texture coordinates: after the traversal
}
DSA_HD bool sym_filtered(const AttrDesc &a, uint32_t flags) {
  const uint32_t g = sym_group_of(a);
  if (g == 2u) return !(flags & SYM_CORNER);
  if (flags & SYM_CORNER) return true;
  return ((flags & SYM_EARLY_ONLY) && g == 1u) || ((flags & SYM_LATE_ONLY) && g == 0u);
}

// Which raw streams k_symbols_reg takes (12-bit precision, at most 4096 symbols more than one of which occurs -- one non-zero symbol
// is a frequency of 4096, which the packed {freq, rem - cum} word cannot hold --, table scratch in the attribute's output region).
DSA_HD bool sym_reg_eligible(const AttrDesc &a, const MeshLayout &L, uint32_t ai) {
  return a.source == SRC_RAW && a.precision_bits == 12 && a.num_symbols <= REG_MAX_SYMS && a.num_distinct > 1 &&
         L.out_cap[ai] >= 4096 * 6 + REG_MAX_SYMS * 4;
}
// Which raw streams k_symbols_wide takes: any precision, at most 2048 symbols to search -- those of the alphabet, or, for a sparse
// large alphabet (14-bit positions: 16 384 ids, about 2 000 used), its non-zero ones -- and room for the tables in global memory.
DSA_HD bool sym_wide_eligible(const AttrDesc &a, const MeshLayout &L, uint32_t ai) {
  if (a.source != SRC_RAW || a.num_distinct <= 1 || sym_reg_eligible(a, L, ai)) return false;
  const bool compact = a.num_symbols > SYM_MAX_LDS;
  const uint32_t nse = compact ? a.num_distinct : a.num_symbols;
  if (nse <= 64 || nse > WIDE_MAX_SYMS || a.precision_bits > 16) return false;     // {cum, freq} packed in 16 + 16 bits
  return compact ? (a.table != 0 && 2ull * nse + 1 <= (unsigned long long)a.num_symbols + 2) : (L.out_cap[ai] >= 4ull * (nse + 1));
}
// a sparse large alphabet (14-bit positions: 16 384 ids, a few thousand of them used) is searched through its non-zero
// symbols; the table k_locate reserved for the serial fallback holds the compact -> symbol map instead
DSA_HD bool sym_tier_compact(const AttrDesc &a) {
  return a.source == SRC_RAW && a.num_symbols > SYM_MAX_LDS && a.num_distinct <= SYM_MAX_LDS && a.num_distinct >= 1 && a.table != 0;
}
// The k_symbols<TIER> that takes an attribute's stream (the attribute is not SRC_BYTES and belongs to the launch): 0 alphabets <= 64
// and the tagged / fixed-width sources, 1 alphabets <= 960, 2 alphabets <= SYM_MAX_LDS and the large-alphabet fallback; -1 where
// k_symbols_reg or k_symbols_wide takes it.
DSA_HD int sym_tier_of(const AttrDesc &a, const MeshLayout &L, uint32_t ai, uint32_t flags) {
  if (sym_reg_eligible(a, L, ai)) return -1;
  if ((flags & SYM_WIDE) && sym_wide_eligible(a, L, ai)) return -1;
  const uint32_t ns = a.source == SRC_RAW ? a.num_symbols : 0u;
  const uint32_t nse = sym_tier_compact(a) ? a.num_distinct : ns;
  return nse <= 64 ? 0 : (nse <= 960 ? 1 : 2);
}

DSA_HD bool wrap_fast_ok(const AttrDesc &a, uint32_t flags) {
  return (flags & PW_FLAG) && a.have_scheme && a.source != SRC_BYTES && a.pred_transform == 1 && a.pred_kind != 3 && a.pred_kind != 4 && a.nc_portable >= 1 && a.nc_portable <= 4 &&
         1u + (uint32_t)a.wrap_max - (uint32_t)a.wrap_min < (1u << 25) && a.num_entries != 0;       // (max_dif of the transform, in unsigned arithmetic)
}
DSA_HD bool pw_dequant_fused(const AttrDesc &a, uint32_t flags) {
  return wrap_fast_ok(a, flags) && a.seq_type == 2 && a.nc == a.nc_portable && a.q_bits >= 1 && a.q_bits <= 30;
}
DSA_HD bool oct_stream_eligible(const AttrDesc &a) {
  return a.have_scheme && a.source != SRC_BYTES && a.pred_transform == 3 && a.pred_kind == 0 && a.corner_data == 0 && a.num_entries != 0 && !a.early_done &&
         a.oct_max_q >= 3 && a.oct_max_q < (1 << OCT_PK_MAX_BITS);      // the packed step's range; finer octahedra stay with k_predict
}
// The phase of k_predict that takes an attribute (0 early, 1 late); -1 where another kernel predicts it or nothing does.
DSA_HD int predict_phase_of(const AttrDesc &a, uint32_t flags) {
  if (!a.have_scheme || a.source == SRC_BYTES) return -1;
  if (wrap_fast_ok(a, flags)) return -1;                    // k_predict_wrap
  if ((flags & OS_FLAG) && oct_stream_eligible(a)) return -1;   // k_predict_oct_streams
  if (a.pred_kind == 2 || a.pred_kind == 3 || a.pred_kind == 4) return -1;            // k_predict_geometric, k_texcoords, k_multipara
  return att_is_late(a) ? 1 : 0;
}

// ---- need bits of a mesh: the kernel groups of dsa_batch_decode that have work for it.  Kernels outside these groups (k_symbols_reg,
// the late k_predict_wrap, the early k_finalize, everything of the connectivity) are launched for every batch.
#define NEED_TAGS 0x1u            // k_tags + k_locate_resume rounds: a tagged symbol stream, or a walk that stopped for another reason
#define NEED_TIER0 0x1u           // the four kernels of a symbol launch beside k_symbols_reg, shifted by the launch's group:
#define NEED_TIER1 0x2u
#define NEED_TIER2 0x4u
#define NEED_WIDE 0x8u
#define NEED_SHIFT_EARLY 1u
#define NEED_SHIFT_LATE 5u
#define NEED_SHIFT_CORNER 9u
#define NEED_GEOMETRIC 0x2000u    // GeometricNormal: k_flip_bits, k_vertex_positions, k_predict_geometric
#define NEED_TEXCOORDS 0x4000u    // TexCoordsPortable: k_orient_bits, k_texcoords_prepare, k_texcoords
#define NEED_PREDICT_EARLY 0x8000u    // something only k_predict takes, in front of / behind the traversal
#define NEED_PREDICT_LATE 0x10000u
#define NEED_WRAP_EARLY 0x20000u      // something the early k_predict_wrap takes
#define NEED_FINALIZE_LATE 0x40000u   // something the phase-1 k_finalize still has to do
#define NEED_ALL 0x7FFFFu
#define DSA_SITE_NEEDS 171        // detail site of a mesh that needs a kernel the decode left out and that the general path cannot take over

DSA_HD uint32_t attr_needs(const AttrDesc &a, const MeshLayout &L, uint32_t ai, uint32_t flags) {
  uint32_t nd = 0;
  if (a.source == SRC_TAGGED) nd |= NEED_TAGS;
  if (a.source != SRC_BYTES) {
    const uint32_t g = sym_group_of(a), shift = g == 2u ? NEED_SHIFT_CORNER : (g == 1u ? NEED_SHIFT_LATE : NEED_SHIFT_EARLY);
    if (!sym_reg_eligible(a, L, ai)) {
      const int tier = sym_tier_of(a, L, ai, flags);
      nd |= (tier < 0 ? NEED_WIDE : (NEED_TIER0 << (uint32_t)tier)) << shift;
    }
    if (a.have_scheme && a.pred_kind == 2) nd |= NEED_GEOMETRIC;
    if (a.have_scheme && a.pred_kind == 3) nd |= NEED_TEXCOORDS;
  }
  const int phase = predict_phase_of(a, flags);
  if (phase == 0) nd |= NEED_PREDICT_EARLY;
  if (phase == 1) nd |= NEED_PREDICT_LATE;
  if (wrap_fast_ok(a, flags) && !att_is_late(a)) nd |= NEED_WRAP_EARLY;
  if (att_is_late(a) && !pw_dequant_fused(a, flags)) nd |= NEED_FINALIZE_LATE;
  return nd;
}
// The need bits of a mesh from its finished descriptor (k_seal).  A general-path mesh has k_general's kernels, which are launched
// whenever the host routed a mesh there, and the phase-1 k_finalize; a walk that did not reach its end wanted the resume rounds.
DSA_HD uint32_t mesh_needs(const MeshDesc &D, const MeshLayout &L, uint32_t flags) {
  if (D.general) return NEED_FINALIZE_LATE;
  uint32_t nd = D.values_pending ? NEED_TAGS : 0u;
  for (uint32_t ai = 0; ai < D.num_attributes && ai < DSA_MAX_ATT; ++ai) nd |= attr_needs(D.att[ai], L, ai, flags);
  return nd;
}
// "needs covered by launched": every group a mesh needs was part of the decode.
DSA_HD bool needs_covered(uint32_t needs, uint32_t launched) { return (needs & ~launched) == 0u; }

}  // namespace dsa
