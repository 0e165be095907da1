// draco-sharp_amd/csrc/dsa_encode.h  (included by dsa_api.hip)
//
// Encode direction of the C-ABI (include/draco_mi355x.h, dsa_encode_*): the drop-in for
//     DracoEncoder.Encode(BinaryWriter, Config, PointCloud, ...)        src/Draco/IO/DracoEncoder.cs:22-41
// for a batch of triangle meshes with per-vertex positions / normals / texture coordinates, a generic uint8 attribute and an
// attribute list of further typed integer / float attributes (dsa_encode_attributes_batch)
// (BASELINE.json configs[4]: "batch quantize + parallelogram predict + rANS encode as HIP kernels").
//
// Split of the work:
//   GPU   (dsa_encode_conn.h)  k_enc_connectivity corner table, Edgebreaker symbols, depth-first attribute order, parallelogram
//                                                 operand entries, one wave per mesh (DSA_ENC_HOST_CONN=1: by the host coder)
//   GPU   (dsa_encode_repair.h) k_enc_repair_*   dsa_encode_repair_batch: the reference's corner table for the meshes the kernels above refuse
//   GPU   (dsa_encode_grid.h)  k_enc_grid_*      dsa_encode_grid_batch: grids shared by a group reduced in front of the chunks; attributes on a given grid quantised and checked
//   GPU   (this file)          k_enc_bounds      quantisation range per attribute   AttributeQuantizationTransform.cs:66-108
//                              k_enc_quantize    floats -> portable ints, normals -> octahedral (s,t), typed integers -> int32   :136-177, OctahedronToolBox.cs:28-119
//                              k_enc_gather      vertex order -> traversal order, wrap bounds           PredictionSchemeWrapTransform.cs:88-100
//                              k_enc_corr        prediction, correction, zig-zag, symbol statistics     MeshPredictionSchemeParallelogramEncoder.cs:35-56,
//                                                                                                       PredictionSchemeWrapEncodingTransform.cs:45-90,
//                                                                                                       ...NormalOctahedronCanonicalizedEncodingTransform.cs:47-83
//                              k_enc_rans        rANS coding of every stream, one wave per stream        RAnsEncoder.cs:22-30, AnsEncoder.cs:34-64, SymbolEncoding.cs:92-193
//                              k_enc_plan        symbol-scheme choice + frequency-table normalisation from the histograms, one lane per
//                                                stream (dsa_symbol_plan.h, the code the host coder runs)   SymbolEncoding.cs:8-40, RAnsSymbolEncoder.cs:15-123
//   host  (dsa_encode_host.h)  input checks; at the end the stream layout: bit-packing of the Edgebreaker symbols, table bytes, section order
//                              (threads over meshes).  DSA_ENC_HOST_PLAN=1: the symbol plans by the host between the two device phases.
//   GPU   (dsa_encode_rows.h)  k_enc_entry_rows  dsa_encode_rows_batch, track_rows = 1: the row of the caller's arrays every entry carries
//   GPU   (dsa_encode_order.h) k_enc_order_*     dsa_encode_ordered_sequential_batch, point_order = 1: Morton keys and a segmented radix sort
//                                                over all clouds of a chunk, between k_enc_quantize and k_enc_gather
//                              k_enc_merge_*     dsa_encode_merged_sequential_batch, merge_points = 1: one point per cell of the position grid,
//                                                the heads of the runs of equal keys behind the sort; nv of the cloud's streams falls on the device
//                              k_enc_part_bounds dsa_encode_split_sequential_batch, part_points >= 1: the sorted order in parts, a set of stream
//                                                records each; the box of every part's position integers behind the sort
//                              k_enc_part_cells  dsa_encode_cell_parts_sequential_batch, part_cells >= 1: both -- the KEPT order in parts, whose
//                                                number and sizes follow from m on the device: part slots, sized behind k_enc_merge_scan
//                              k_enc_lod_*       dsa_encode_lod_sequential_batch, lod_base_bits >= 1: the kept order by (level, kept), every
//                                                level in parts: levels, scan, scatter, row entries and the slots, in place of k_enc_part_cells
//                              k_enc_mean_*      dsa_encode_mean_sequential_batch, mean_attributes != 0: the mean of the cell into the masked
//                                                attributes' integers at every kept row, behind the merge
//                              k_enc_vote_*      dsa_encode_vote_sequential_batch, vote_attributes != 0: the most frequent tuple of the cell
//                                                into the voted attributes' integers at every kept row, beside the means
//                              k_enc_normal_*    dsa_encode_normal_mean_sequential_batch, mean_normals = 1: the mean normal of the cell into
//                                                the normals' octahedral codes at every kept row, beside the two above
//                              k_enc_voxel_*     dsa_encode_voxel_sequential_batch, voxel_bits >= 1: the cell is the key without its low
//                                                3 (position_bits - voxel_bits) bits; the nearest point of every voxel into kept
//         (dsa_encode_layout.h) the request of an entry point, the state of a chunk, the per-mesh checks and plans, the arena layout
// Every entry point fills an EncRequest and calls encode_request; a chunk of it goes through the stages of encode_chunk (or of
// encode_sequential_chunk, dsa_encode_sequential.h) on a lane.
// The result is byte-identical to the CPU coder of dsa_encode_host.h (tests/test_gpu_encode.py), hence decodes
// bit-exactly to the quantised input.
#pragma once
#include <chrono>
#include <memory>
#include <thread>

#include "dsa_encode_layout.h"

namespace dsa {

static const int ENC_PLAN_RAW_BEYOND_LIMIT = 1000;      // plan_status beside dsa::plan::PLAN_*: see enc_plan_message
static const char *const ENC_RAW_BEYOND_MESSAGE = "symbol_scheme 1 (raw) forced on an integer attribute with symbols of 2^18 and above: the device coder writes those tagged only";

__device__ __forceinline__ uint32_t enc_msb(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
__device__ __forceinline__ uint32_t enc_zigzag(int32_t v) { return v >= 0 ? (uint32_t)v << 1 : (((uint32_t)(-(v + 1))) << 1) | 1u; }

// Quantisation range: per-component min / max, range = largest extent (1 if degenerate).  GRID: the chunk has streams on a grid
// that is not their own bounds (EncStream::grid_mode; dsa_encode_grid.h) -- their records hold it already, and
// k_enc_grid_quantize quantises them; a chunk without such streams launches <false>, the kernel it always ran.
// The minimum of a component carries the bits of the FIRST row that attains it, as the serial strict compare of the reference
// and of the host coder leaves it (synth::quantize): the header holds those four bytes, and -0.0 == +0.0 attains the same
// minimum with another sign.  So a minimum travels with its row, and of two equal minima the one of the smaller row stays --
// whatever the block shape and the order of the folds.  The maximum needs no such rule: only max - min is used.
// The smallest row with a value that is not finite lands in grid_nonfinite (ENC_GRID_NO_ROW: none), and the host refuses the mesh
// (enc_quantiser_refusals); the bounds of such a stream mean nothing.
// Cost of the rows and the finite check against the kernel without them: 27 VGPRs in place of 22 (4 rows, 1 bad row) and 13 KiB
// of LDS a block in place of 8 (u32[4][256] rows and u32[256] bad rows beside the two f32[4][256]); no scratch, 8 waves / SIMD
// and one block per stream as before (profiles/README.md: the encode legs stay within their run-to-run spread).
template <bool GRID>
__global__ __launch_bounds__(256) void k_enc_bounds(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.kind != 0 || S.part != 0) return;         // (a part behind the first of a split cloud: the first part's bounds are the cloud's)
  if (GRID && S.grid_mode != 0) return;
  __shared__ float s_mn[4][256], s_mx[4][256];
  __shared__ uint32_t s_row[4][256], s_bad[256];
  const float *src = (const float *)(arena + S.src);
  const uint32_t nc = S.nc_out, tid = threadIdx.x;
  float mn[4], mx[4];
  uint32_t row[4], bad = ENC_GRID_NO_ROW;
  for (uint32_t c = 0; c < 4; ++c) { mn[c] = src[c < nc ? c : 0]; mx[c] = mn[c]; row[c] = 0; }
  for (uint32_t v = tid; v < S.rows; v += 256)      // (rows ascend: the strict compare keeps the thread's first)
    for (uint32_t c = 0; c < nc; ++c) {
      const float x = src[(size_t)v * nc + c];
      if (x < mn[c]) { mn[c] = x; row[c] = v; }
      if (x > mx[c]) mx[c] = x;
      if ((__float_as_uint(x) & 0x7F800000u) == 0x7F800000u && bad == ENC_GRID_NO_ROW) bad = v;
    }
  for (uint32_t c = 0; c < 4; ++c) { s_mn[c][tid] = mn[c]; s_mx[c][tid] = mx[c]; s_row[c][tid] = row[c]; }
  s_bad[tid] = bad;
  __syncthreads();
  for (uint32_t h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
      for (uint32_t c = 0; c < 4; ++c) {
        const float o = s_mn[c][tid + h], m = s_mn[c][tid];
        const uint32_t orow = s_row[c][tid + h];
        if (o < m || (o == m && orow < s_row[c][tid])) { s_mn[c][tid] = o; s_row[c][tid] = orow; }
        if (s_mx[c][tid + h] > s_mx[c][tid]) s_mx[c][tid] = s_mx[c][tid + h];
      }
      if (s_bad[tid + h] < s_bad[tid]) s_bad[tid] = s_bad[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float range = 0.0f;
    for (uint32_t c = 0; c < nc; ++c) { S.qmin[c] = s_mn[c][0]; const float dlt = __fsub_rn(s_mx[c][0], s_mn[c][0]); if (dlt > range) range = dlt; }
    if (range == 0.0f) range = 1.0f;
    S.qrange = range;
    S.grid_nonfinite = s_bad[0];
  }
}

// OctahedronToolBox.cs:28-119 (float vector -> canonical octahedral coordinates), in double as the host coder
__device__ void enc_oct_from_float(const float *in, int32_t bits, int32_t &s, int32_t &t) {
  const int32_t max_q = (1 << bits) - 1, max_value = max_q - 1, center = max_value / 2;
  const double v0 = in[0], v1 = in[1], v2 = in[2];
  const double abs_sum = __dadd_rn(__dadd_rn(fabs(v0), fabs(v1)), fabs(v2));
  double s0, s1, s2;
  if (abs_sum > 1e-6) { const double sc = __ddiv_rn(1.0, abs_sum); s0 = __dmul_rn(v0, sc); s1 = __dmul_rn(v1, sc); s2 = __dmul_rn(v2, sc); }
  else { s0 = 1; s1 = 0; s2 = 0; }
  int32_t i0 = (int32_t)floor(__dadd_rn(__dmul_rn(s0, (double)center), 0.5));
  int32_t i1 = (int32_t)floor(__dadd_rn(__dmul_rn(s1, (double)center), 0.5));
  enc_oct_from_scaled(center, max_value, i0, i1, s2 < 0, s, t);      // (the tail and the canonicalisation: dsa_encode_schemes.h, with the mean normals)
}

template <bool GRID>      // (as for k_enc_bounds)
__global__ __launch_bounds__(256) void k_enc_quantize(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.y;
  if (si >= ns) return;
  const EncStream &S = streams[si];
  if (S.part != 0) return;                        // (a part behind the first of a split cloud: `vals` are the first part's)
  if (GRID && S.kind == 0 && S.grid_mode != 0) return;
  const float *src = (const float *)(arena + S.src);
  int32_t *vals = (int32_t *)(arena + S.vals);
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  if (S.kind == 0) {                // Quantizer: floor((v - min) * (max_q / range) + 0.5), every step rounded to f32
    const float inv_delta = __fdiv_rn((float)(int32_t)((1u << S.bits) - 1u), S.qrange);
    const uint32_t nc = S.nc_out, total = S.rows * nc;
    // What the host refuses the mesh for behind this stage (enc_quantiser_refusals: a value that is not finite, a range that is
    // not or that max_q does not divide finitely) shows here as a sum that is not finite: it is written as 0, as
    // k_enc_grid_quantize writes an offending value, so that the kernels behind stay among integers of 0 .. max_q.
    for (uint32_t i = tid; i < total; i += stride) {
      const float v = __fsub_rn(src[i], S.qmin[i % nc]);
      const float t = __fadd_rn(__fmul_rn(v, inv_delta), 0.5f);
      vals[i] = (__float_as_uint(t) & 0x7F800000u) == 0x7F800000u ? 0 : (int32_t)floorf(t);
    }
  } else if (S.kind == 2) {         // an integer attribute: its values as they are (SequentialIntegerAttributeEncoder.cs: no transform)
    // rows are packed at itemsize * nc (a 2-byte type of 3 components is not 4-byte aligned per row): one element per lane and
    // load, each aligned to its own size (src is 256-byte aligned), consecutive lanes consecutive elements; widened to int32,
    // uint32 by reinterpretation (generic_value of the host coder).  The type is the stream's: the switch is uniform per block.
    const uint8_t *srcb = arena + S.src;
    const uint32_t total = S.rows * S.nc;
    switch (S.elem) {
      case 1: for (uint32_t i = tid; i < total; i += stride) vals[i] = (int32_t)((const int8_t *)srcb)[i]; break;
      case 3: for (uint32_t i = tid; i < total; i += stride) vals[i] = (int32_t)((const int16_t *)srcb)[i]; break;
      case 4: for (uint32_t i = tid; i < total; i += stride) vals[i] = (int32_t)((const uint16_t *)srcb)[i]; break;
      case 5: case 6: for (uint32_t i = tid; i < total; i += stride) vals[i] = ((const int32_t *)srcb)[i]; break;
      default: for (uint32_t i = tid; i < total; i += stride) vals[i] = (int32_t)srcb[i]; break;      // 2: uint8
    }
  } else if (S.kind == 1) {
    for (uint32_t v = tid; v < S.rows; v += stride) {
      int32_t s, t;
      enc_oct_from_float(src + (size_t)v * 3, (int32_t)S.bits, s, t);
      vals[2 * v] = s; vals[2 * v + 1] = t;
    }
  }
}

// traversal order + bounds of the wrap transform over all values of the attribute
__global__ __launch_bounds__(256) void k_enc_gather(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.kind == 3) return;
  __shared__ int32_t s_mn[256], s_mx[256];
  const int32_t *vals = (const int32_t *)(arena + S.vals);
  int32_t *d = (int32_t *)(arena + S.d);
  const uint32_t *e2v = (const uint32_t *)(arena + S.e2v);
  const uint32_t nc = S.nc, tid = threadIdx.x;
  int32_t mn = 0x7FFFFFFF, mx = (int32_t)0x80000000;
  if (S.linear) {                  // the values are in entry order where they lie: the bounds alone
    for (uint32_t i = tid, total = S.nv * nc; i < total; i += 256) { const int32_t x = vals[i]; if (x < mn) mn = x; if (x > mx) mx = x; }
  } else
  for (uint32_t e = tid; e < S.nv; e += 256) {
    const uint32_t v = e2v[e];
    for (uint32_t c = 0; c < nc; ++c) { const int32_t x = vals[(size_t)v * nc + c]; d[(size_t)e * nc + c] = x; if (x < mn) mn = x; if (x > mx) mx = x; }
  }
  s_mn[tid] = mn; s_mx[tid] = mx;
  __syncthreads();
  for (uint32_t h = 128; h >= 1; h >>= 1) {
    if (tid < h) { if (s_mn[tid + h] < s_mn[tid]) s_mn[tid] = s_mn[tid + h]; if (s_mx[tid + h] > s_mx[tid]) s_mx[tid] = s_mx[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) { S.wrap_mn = s_mn[0]; S.wrap_mx = s_mx[0]; }
}

// corrections -> symbols, per-entry bit lengths, statistics
__global__ __launch_bounds__(256) void k_enc_corr(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.y;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.kind == 3) return;                      // (a valence context list: k_enc_list_stats)
  if (S.kind != 1 && (S.prediction == 2 || S.prediction == 4)) return;      // (MultiParallelogram: k_enc_multi)
  __shared__ uint32_t s_tag[33];
  __shared__ uint32_t s_max;
  __shared__ unsigned long long s_bl;
  // the block counts its symbols in LDS and adds what it counted to the stream's histogram once (alphabets of up to 12 bits; a
  // global atomic per symbol was a third of the attribute kernels' time)
  __shared__ uint32_t s_hist[4098];
  const bool lds_hist = S.hist_cap <= 4098u;
  // a symbol outside a histogram of the largest size is no overflow: the raw scheme is out of the question then (max_value tells k_enc_plan)
  const bool beyond_ok = S.kind == 2 && S.hist_cap == ENC_HIST_CAP_LIMIT;
  if (lds_hist) for (uint32_t i = threadIdx.x; i < S.hist_cap; i += blockDim.x) s_hist[i] = 0;
  if (threadIdx.x < 33) s_tag[threadIdx.x] = 0;
  if (threadIdx.x == 0) { s_max = 0; s_bl = 0; }
  __syncthreads();
  const int32_t *d = (const int32_t *)(arena + S.d);
  const int32_t *ops = (const int32_t *)(arena + S.ops);
  uint32_t *syms = (uint32_t *)(arena + S.syms);
  uint8_t *bl = arena + S.bl;
  uint32_t *hist = (uint32_t *)(arena + S.hist_raw);
  const uint32_t nc = S.nc;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  // wrap transform, PredictionSchemeWrapEncodingTransform.cs:45-90 (E-5) + WrapTransform.cs:88-100
  const int32_t mn = S.wrap_mn, mx = S.wrap_mx, max_dif = 1 + mx - mn;
  int32_t max_corr = max_dif / 2;
  const int32_t min_corr = -max_corr;
  if ((max_dif & 1) == 0) max_corr -= 1;
  // octahedron
  const int32_t o_max_q = (1 << S.bits) - 1, o_center = (o_max_q - 1) / 2;
  // TexCoordsPortable / GeometricNormal: positions and topology (dsa_encode_schemes.h)
  const bool portable = S.kind == 0 && S.prediction == 5, geometric = S.kind == 1 && S.prediction == 6;
  EncTopo T;
  T.d = d; T.pos = (const int32_t *)(arena + S.pos_vals);
  T.c2p = (const uint32_t *)(arena + S.t_c2p); T.c2a = (const uint32_t *)(arena + S.t_c2a); T.opp = (const uint32_t *)(arena + S.t_opp);
  T.d2c = (const uint32_t *)(arena + S.t_d2c); T.v2d = (const int32_t *)(arena + S.t_v2d); T.nc3 = S.t_nc3;
  uint8_t *ori = arena + S.ori;
  uint32_t *flags = (uint32_t *)(arena + S.flags);
  for (uint32_t p = tid; p < S.nv; p += stride) {
    uint32_t mc = 0;
    if (geometric) {
      uint32_t sy[2];
      bool flip = false;
      if (!enc_geo_normal(T, p, (int32_t)S.bits, sy, flip)) { S.overflow = 1; sy[0] = sy[1] = 0; }
      if (flip) atomicOr(&flags[p >> 5], 1u << (p & 31u));
      for (uint32_t c = 0; c < 2; ++c) {
        syms[2 * p + c] = sy[c];
        if (sy[c] < S.hist_cap) atomicAdd(lds_hist ? &s_hist[sy[c]] : &hist[sy[c]], 1u); else S.overflow = 1;
        mc = sy[c] > mc ? sy[c] : mc;
      }
    } else if (S.kind != 1) {
      int32_t vn = -1, vp = -1, vo = -1;
      if (S.prediction == 1 && p > 0) { vn = ops[3 * p]; vp = ops[3 * p + 1]; vo = ops[3 * p + 2]; }
      int32_t tp[2] = {0, 0};
      if (portable) { uint32_t o = 0; enc_tex_portable(T, p, tp, o); ori[p] = (uint8_t)o; }
      for (uint32_t c = 0; c < nc; ++c) {
        int32_t pred;
        if (portable) pred = tp[c & 1u];
        else if (vn >= 0) pred = d[(size_t)vn * nc + c] + d[(size_t)vp * nc + c] - d[(size_t)vo * nc + c];
        else pred = p > 0 ? d[(size_t)(p - 1) * nc + c] : 0;
        const int32_t pc = pred > mx ? mx : (pred < mn ? mn : pred);
        int32_t cr = d[(size_t)p * nc + c] - pc;
        if (cr < min_corr) cr += max_dif; else if (cr > max_corr) cr -= max_dif;
        const uint32_t sy = enc_zigzag(cr);
        syms[(size_t)p * nc + c] = sy;
        if (sy < S.hist_cap) atomicAdd(lds_hist ? &s_hist[sy] : &hist[sy], 1u); else if (!beyond_ok) S.overflow = 1;
        mc = sy > mc ? sy : mc;
      }
    } else {                        // PredictionSchemeNormalOctahedronCanonicalizedEncodingTransform.cs:47-83
      int32_t os = d[2 * p] - o_center, ot = d[2 * p + 1] - o_center;
      int32_t ps = (p > 0 ? d[2 * (p - 1)] : 0) - o_center, pt = (p > 0 ? d[2 * (p - 1) + 1] : 0) - o_center;
      const int32_t aps = ps < 0 ? -ps : ps, apt = pt < 0 ? -pt : pt;
      if (!((uint32_t)aps + (uint32_t)apt <= (uint32_t)o_center)) { oct_invert_diamond(o_center, os, ot); oct_invert_diamond(o_center, ps, pt); }
      const bool bottom_left = (ps == 0 && pt == 0) || (ps < 0 && pt <= 0);
      if (!bottom_left) {
        int rot;
        if (ps == 0) rot = pt == 0 ? 0 : (pt > 0 ? 3 : 1);
        else if (ps > 0) rot = pt >= 0 ? 2 : 1;
        else rot = pt <= 0 ? 0 : 3;
        oct_rotate(os, ot, rot); oct_rotate(ps, pt, rot);
      }
      int32_t c0 = os - ps, c1 = ot - pt;
      if (c0 < 0) c0 += o_max_q;
      if (c1 < 0) c1 += o_max_q;
      const uint32_t sy[2] = {(uint32_t)c0, (uint32_t)c1};     // positive: no zig-zag
      for (uint32_t c = 0; c < 2; ++c) {
        syms[2 * p + c] = sy[c];
        if (sy[c] < S.hist_cap) atomicAdd(lds_hist ? &s_hist[sy[c]] : &hist[sy[c]], 1u); else S.overflow = 1;
        mc = sy[c] > mc ? sy[c] : mc;
      }
    }
    const uint32_t b = (mc > 0 ? enc_msb(mc) : 0u) + 1u;
    bl[p] = (uint8_t)b;
    atomicAdd(&s_tag[b], 1u);
    atomicMax(&s_max, mc);
    atomicAdd(&s_bl, (unsigned long long)b);
  }
  __syncthreads();
  if (lds_hist) for (uint32_t i = threadIdx.x; i < S.hist_cap; i += blockDim.x) { const uint32_t c = s_hist[i]; if (c) atomicAdd(&hist[i], c); }
  if (threadIdx.x < 33 && s_tag[threadIdx.x]) atomicAdd(&S.hist_tag[threadIdx.x], s_tag[threadIdx.x]);
  if (threadIdx.x == 0) { atomicMax(&S.max_value, s_max); atomicAdd(&S.total_bl, s_bl); }
}

// Symbol-scheme choice and frequency-table normalisation, one lane per stream: dsa_symbol_plan.h, the code the host coder
// runs, on the histograms k_enc_corr left in device memory.  Sequential per stream (a stable sort and a fix-up loop over the
// alphabet), thousands of streams side by side; its tables go straight to k_enc_rans, no host in between.
__global__ __launch_bounds__(WAVE) void k_enc_plan(uint8_t *arena, EncStream *streams, uint32_t ns, int force_scheme, int compression_level) {
  const uint32_t si = blockIdx.x * WAVE + threadIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.overflow || (S.kind == 3 && S.nv == 0)) return;      // (an empty context list is not coded: its size 0 is all of it)
  // symbols of 2^18 and above (an integer attribute): the tagged scheme whatever the histogram of values would say, which is not
  // read -- plan_symbols of the host coder with no raw histogram.  The raw scheme forced on such a stream: refused here.
  const bool tagged_only = S.kind == 2 && S.max_value >= ENC_RAW_SYMBOL_LIMIT;
  if (tagged_only && force_scheme == 1) { S.plan_status = (uint32_t)ENC_PLAN_RAW_BEYOND_LIMIT; S.overflow = 1; return; }
  if (!tagged_only && S.max_value >= S.hist_cap) { S.overflow = 1; return; }
  const uint32_t *raw = (const uint32_t *)(arena + S.hist_raw);
  uint32_t *prob = (uint32_t *)(arena + S.prob), *cum = (uint32_t *)(arena + S.cum);
  uint32_t *order = (uint32_t *)(arena + S.plan_order), *tmp = (uint32_t *)(arena + S.plan_tmp);
  int method = tagged_only ? 0 : 1, usbl = 0;
  int rc = tagged_only ? (int)plan::PLAN_OK
                       : plan::choose_scheme((const uint32_t *)S.hist_tag, raw, S.max_value, (uint64_t)S.nv * S.nc, S.nc, (uint64_t)S.total_bl, force_scheme, compression_level, &method, &usbl);
  int pb = 12;
  uint32_t nsym = 0;
  if (rc == plan::PLAN_OK)
    rc = method == 0 ? plan::rans_tables(5, (const uint32_t *)S.hist_tag, (size_t)33, prob, cum, order, tmp, &pb, &nsym)
                     : plan::rans_tables(usbl, raw, (size_t)S.max_value + 1, prob, cum, order, tmp, &pb, &nsym);
  S.plan_status = (uint32_t)rc;
  if (rc != plan::PLAN_OK) { S.overflow = 1; return; }
  S.method = (uint32_t)method; S.usbl = (uint32_t)usbl; S.precision_bits = (uint32_t)pb; S.num_symbols = nsym;
}

// rANS coding, one WAVE per stream.  The coder state is a serial chain (x' = (x / p) << bits + x % p + cum after the renormalisation
// bytes), so it lives in scalar registers; what the wave does in parallel is everything off the chain: 64 symbols at a time are
// looked up (frequency, cumulative count, and the reciprocal that turns the division into a multiply-high with one correction),
// and the bytes collect in a register, a lane each, and leave 64 at a time.
// Symbols are fed last -> first (SymbolEncoding.cs:177-183); bytes are written in coding order, the decoder reads
// them from the end (RAnsEncoder.cs:22-30, AnsEncoder.cs:34-64).
__global__ __launch_bounds__(WAVE) void k_enc_rans(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x, lane = threadIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.overflow || (S.kind == 3 && S.nv == 0)) return;
  const uint32_t *prob = (const uint32_t *)(arena + S.prob), *cum = (const uint32_t *)(arena + S.cum);
  const uint32_t *syms = (const uint32_t *)(arena + S.syms);
  const uint8_t *bl = arena + S.bl;
  uint8_t *out = arena + S.out_rans;
  const uint32_t pb = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.precision_bits), precision = 1u << pb, l_base = precision * 4u;
  const bool tagged = S.method == 0;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tagged ? S.nv : S.nv * S.nc));
  const uint32_t cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.out_cap);
  uint32_t state = l_base, len = 0;                 // wave-uniform
  uint32_t held = 0, bytes = 0;                     // bytes of lane j of `bytes`: out[len - held + j], j < held
  auto emit = [&](uint32_t byte) {
    bytes = lane == held ? byte : bytes;
    ++held; ++len;
    if (held == WAVE) {
      const uint32_t at = len - WAVE + lane;
      if (at < cap) out[at] = (uint8_t)bytes;
      held = 0;
    }
  };
  for (uint32_t hi = n; hi > 0;) {
    const uint32_t cnt = hi < WAVE ? hi : WAVE;
    // lane j holds the j-th symbol of this stretch in coding order
    uint32_t p = 1, c = 0, magic = 0;
    if (lane < cnt) {
      const uint32_t k = hi - 1 - lane;
      const uint32_t sym = tagged ? (uint32_t)bl[k] : syms[k];
      p = prob[sym]; c = cum[sym];
      if (p == 0) p = 1;                              // (a symbol that occurs has a frequency; a zero here must not spin the loop below)
      magic = p > 1 ? 0xFFFFFFFFu / p + 1u : 0u;      // ceil(2^32 / p)
    }
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)p, (int)j), cj = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)j);
      const uint32_t mj = (uint32_t)__builtin_amdgcn_readlane((int)magic, (int)j);
      const uint32_t lim = pj << 10;                // (l_base / precision) * 256 * p; p <= precision <= 2^20
      while (state >= lim) { emit(state & 0xFFu); state >>= 8; }
      // state / p: the multiply-high by ceil(2^32 / p) is the quotient or one more (state < 2^32, error < state / 2^32 < 1)
      uint32_t q = pj > 1 ? __umulhi(state, mj) : state;
      uint32_t r = state - q * pj;
      if ((int32_t)r < 0) { --q; r += pj; }
      state = (q << pb) + r + cj;
    }
    hi -= cnt;
  }
  const uint32_t fs = state - l_base;
  uint32_t v, nb;
  if (fs < (1u << 6)) { v = fs; nb = 1; }
  else if (fs < (1u << 14)) { v = 0x4000u + fs; nb = 2; }
  else if (fs < (1u << 22)) { v = 0x800000u + fs; nb = 3; }
  else { v = 0xC0000000u + fs; nb = 4; }
  for (uint32_t i = 0; i < nb; ++i) emit((v >> (8 * i)) & 0xFFu);
  if (lane < held) { const uint32_t at = len - held + lane; if (at < cap) out[at] = (uint8_t)bytes; }
  if (lane != 0) return;
  S.rans_len = len;
  if (len > cap || fs >= (1u << 30)) S.overflow = 1;
  // tagged scheme: the values follow as raw LSB-first bit fields of their entry's length (SymbolEncoding.cs:117-137)
  uint32_t blen = 0;
  if (tagged) {
    uint8_t *bits = arena + S.out_bits;
    uint64_t acc = 0;
    uint32_t nacc = 0;
    for (uint32_t e = 0; e < S.nv; ++e) {
      const uint32_t b = bl[e];
      for (uint32_t c = 0; c < S.nc; ++c) {
        const uint64_t val = (uint64_t)syms[(size_t)e * S.nc + c] & (b >= 32 ? 0xFFFFFFFFull : ((1ull << b) - 1ull));
        acc |= val << nacc;
        nacc += b;
        while (nacc >= 8) { if (blen < cap) bits[blen] = (uint8_t)(acc & 0xFF); ++blen; acc >>= 8; nacc -= 8; }
      }
    }
    if (nacc > 0) { if (blen < cap) bits[blen] = (uint8_t)(acc & 0xFF); ++blen; }
    if (blen > cap) S.overflow = 1;
  }
  S.bits_len = blen;
}

// Statistics of a valence context list (kind 3; its symbols are given): bit lengths, histograms, maximum -- what k_enc_corr
// gathers for an attribute (symbol_stats of the host coder, nc = 1).  One block per stream.
__global__ __launch_bounds__(256) void k_enc_list_stats(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.kind != 3 || S.overflow) return;
  __shared__ uint32_t s_hist[8];
  if (threadIdx.x < 8) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t *syms = (const uint32_t *)(arena + S.syms);
  uint8_t *bl = arena + S.bl;
  for (uint32_t p = threadIdx.x; p < S.nv; p += 256) {
    const uint32_t v = syms[p] < 8u ? syms[p] : 7u;
    bl[p] = (uint8_t)((v > 0 ? enc_msb(v) : 0u) + 1u);
    atomicAdd(&s_hist[v], 1u);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t *hist = (uint32_t *)(arena + S.hist_raw);
  unsigned long long total = 0;
  for (uint32_t v = 0; v < 8; ++v) {
    const uint32_t c = s_hist[v];
    if (!c) continue;
    if (v >= S.hist_cap) { S.overflow = 1; continue; }
    hist[v] = c;
    const uint32_t b = (v > 0 ? enc_msb(v) : 0u) + 1u;
    S.hist_tag[b] += c;
    total += (unsigned long long)c * b;
    S.max_value = v;
  }
  S.total_bl = total;
}

// TexCoordsPortable's orientation bits (write_attribute_values, prediction 5): only the entries that took the full branch, last
// entry first, each coded as "equal to the one before" (the first against true).  One wave per stream, 64 entries a round: the
// kept lanes find their predecessor among the lower lanes of the round (or the round before) and set their bit at their place.
__global__ __launch_bounds__(WAVE) void k_enc_orient(uint8_t *arena, EncStream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.x, lane = threadIdx.x;
  if (si >= ns) return;
  EncStream &S = streams[si];
  if (S.kind != 0 || S.prediction != 5 || S.overflow) return;
  const uint8_t *ori = arena + S.ori;
  uint32_t *flags = (uint32_t *)(arena + S.flags);
  const uint32_t nv = S.nv;
  uint32_t base = 0;
  bool carry = true;
#if defined(__HIPCC__)
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t r0 = 0; r0 < nv; r0 += WAVE) {
    const uint32_t r = r0 + lane;                     // the r-th entry from the end
    const uint32_t o = r < nv ? ori[nv - 1u - r] : 0u;
    const bool kept = o != 0u, val = o == 3u;
    const uint64_t km = __ballot(kept), om = __ballot(kept && val);
    const uint64_t lower = km & below;
    const bool before = lower ? ((om >> (63 - __clzll(lower))) & 1ull) != 0 : carry;
    if (kept && val == before) { const uint32_t at = base + (uint32_t)__popcll(lower); atomicOr(&flags[at >> 5], 1u << (at & 31u)); }
    if (km) carry = ((om >> (63 - __clzll(km))) & 1ull) != 0;
    base += (uint32_t)__popcll(km);
  }
#else
  if (lane == 0)
    for (uint32_t r = 0; r < nv; ++r) {
      const uint32_t o = ori[nv - 1u - r];
      if (!o) continue;
      const bool val = o == 3u;
      if (val == carry) flags[base >> 5] |= 1u << (base & 31u);
      carry = val; ++base;
    }
#endif
  if (lane == 0) S.num_flags = base;
}

}  // namespace dsa

namespace dsa {
// Many small pieces in one transfer: k_enc_pack gathers pieces of the arena into one buffer (then one copy to the host),
// k_enc_unpack scatters one uploaded buffer into the arena.  A batch has thousands of such pieces (symbols and split events per
// mesh, histograms, tables and coded bytes per stream); as copies of their own they cost more than the kernels between them.
struct PackItem { uint64_t arena_off, packed_off; uint32_t len, pad; };
__global__ __launch_bounds__(256) void k_enc_pack(const uint8_t *arena, uint8_t *packed, const PackItem *items, uint32_t n) {
  if (blockIdx.x >= n) return;
  const PackItem it = items[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < it.len; i += 256) packed[it.packed_off + i] = arena[it.arena_off + i];
}
__global__ __launch_bounds__(256) void k_enc_unpack(uint8_t *arena, const uint8_t *packed, const PackItem *items, uint32_t n) {
  if (blockIdx.x >= n) return;
  const PackItem it = items[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < it.len; i += 256) arena[it.arena_off + i] = packed[it.packed_off + i];
}

}  // namespace dsa

// ------------------------------------------------------------------------------------------------ host side
// ---- transfers of a chunk, shared by the chunk functions (encode_chunk below, encode_sequential_chunk of dsa_encode_sequential.h)
// uploads in pieces through the lane's two pinned staging buffers: host threads fill one while the DMA engine drains the
// other (a pageable source would be staged by the runtime, one thread, a few GB/s)
static hipError_t enc_upload(EncLane &lane, uint8_t *arena, hipStream_t st, const std::vector<EncUpload> &ups) {
  const uint64_t piece_cap = 192ull << 20;
  size_t i0 = 0;
  while (i0 < ups.size()) {
    const uint64_t lo = ups[i0].off;
    size_t i1 = i0 + 1;
    while (i1 < ups.size() && ups[i1].off + ups[i1].bytes - lo <= piece_cap) ++i1;
    const uint64_t hi = ups[i1 - 1].off + ups[i1 - 1].bytes;
    hostutil::Staging &stg = lane.stage[lane.next];
    lane.next ^= 1;
    hipError_t e = stg.acquire((size_t)(hi - lo));
    if (e != hipSuccess) return e;
    uint8_t *h = stg.buf.p;
    hostutil::parallel_for((uint32_t)(i1 - i0), [&](uint32_t k) {
      const EncUpload &u = ups[i0 + k];
      if (!u.narrow) { memcpy(h + (u.off - lo), u.src, u.bytes); return; }
      const uint32_t *src = (const uint32_t *)u.src;
      uint16_t *dst = (uint16_t *)(h + (u.off - lo));               // (offsets are multiples of 256)
      for (size_t e = 0, ne = u.bytes / 2; e < ne; ++e) dst[e] = (uint16_t)src[e];
    }, 2);
    e = hipMemcpyAsync(arena + lo, h, (size_t)(hi - lo), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = stg.submitted(st);
    if (e != hipSuccess) return e;
    i0 = i1;
  }
  return hipSuccess;
}
// pieces of the arena -> one host buffer (items[k].packed_off filled in); host buffer -> pieces of the arena
// (into *host, or with `view` and no `host` without that copy: *view points at the pieces in the lane's pinned staging buffer, valid
// until the gather after next)
static dsa_status enc_gather(EncLane &lane, const uint8_t *arena, std::vector<dsa::PackItem> &items, std::vector<uint8_t> *host, const uint8_t **view) {
  uint64_t total = 0;
  for (auto &it : items) { it.packed_off = total; total += ((uint64_t)it.len + 15) & ~15ull; }
  if (view) *view = nullptr; else host->resize(total);
  if (items.empty() || total == 0) return DSA_OK;
  uint8_t *d_packed = nullptr; dsa::PackItem *d_items = nullptr;
  hipError_t e = lane.packed.ensure(total);
  if (e == hipSuccess) e = lane.items.ensure(sizeof(dsa::PackItem) * items.size());
  d_packed = (uint8_t *)lane.packed.p; d_items = (dsa::PackItem *)lane.items.p;
  if (e == hipSuccess) e = hipMemcpyAsync(d_items, items.data(), sizeof(dsa::PackItem) * items.size(), hipMemcpyHostToDevice, lane.st);
  if (e == hipSuccess) { hipLaunchKernelGGL(dsa::k_enc_pack, dim3((uint32_t)items.size()), dim3(256), 0, lane.st, arena, d_packed, d_items, (uint32_t)items.size()); e = hipGetLastError(); }
  // through pinned staging (a pageable destination is staged by the runtime at a fraction of the link's rate)
  hostutil::Staging &stg = lane.stage[lane.next];
  lane.next ^= 1;
  if (e == hipSuccess) e = stg.acquire((size_t)total);
  if (e == hipSuccess) e = hipMemcpyAsync(stg.buf.p, d_packed, total, hipMemcpyDeviceToHost, lane.st);
  if (e == hipSuccess) e = hipStreamSynchronize(lane.st);
  if (e == hipSuccess) { if (view) *view = stg.buf.p; else hostutil::parallel_memcpy(host->data(), stg.buf.p, (size_t)total); }
  return e == hipSuccess ? DSA_OK : (e == hipErrorOutOfMemory ? DSA_ERR_OUT_OF_MEMORY : DSA_ERR_DEVICE);
}
static dsa_status enc_scatter(EncLane &lane, uint8_t *arena, std::vector<dsa::PackItem> &items, const std::vector<uint8_t> &host) {
  if (items.empty() || host.empty()) return DSA_OK;
  uint8_t *d_packed = nullptr; dsa::PackItem *d_items = nullptr;
  hipError_t e = lane.packed.ensure(host.size());
  if (e == hipSuccess) e = lane.items.ensure(sizeof(dsa::PackItem) * items.size());
  d_packed = (uint8_t *)lane.packed.p; d_items = (dsa::PackItem *)lane.items.p;
  if (e == hipSuccess) e = hipMemcpyAsync(d_items, items.data(), sizeof(dsa::PackItem) * items.size(), hipMemcpyHostToDevice, lane.st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_packed, host.data(), host.size(), hipMemcpyHostToDevice, lane.st);
  if (e == hipSuccess) { hipLaunchKernelGGL(dsa::k_enc_unpack, dim3((uint32_t)items.size()), dim3(256), 0, lane.st, arena, d_packed, d_items, (uint32_t)items.size()); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(lane.st);
  return e == hipSuccess ? DSA_OK : (e == hipErrorOutOfMemory ? DSA_ERR_OUT_OF_MEMORY : DSA_ERR_DEVICE);
}

#define ENC_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { return set_err(ctx, e_ == hipErrorOutOfMemory ? DSA_ERR_OUT_OF_MEMORY : DSA_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); } } while (0)
#define ENC_ST(call) do { dsa_status s_ = (call); if (s_ != DSA_OK) { return set_err(ctx, s_, "%s failed", #call); } } while (0)
#define ENC_STAGE(call) do { const dsa_status s_ = (call); if (s_ != DSA_OK) return s_; } while (0)      // (the stage has said why)
// ---- scheme choice and rANS tables by the host from the device statistics (DSA_ENC_HOST_PLAN), between the two device phases:
// histograms down, plans by threads over streams, tables up.  A stream whose plan fails fails its mesh.
static dsa_status enc_host_plans(dsa_context *ctx, EncLane &lane, EncChunk &ck) {
  std::vector<dsa::EncStream> &hs = ck.L.streams;
  std::vector<synth::SymbolPlan> &splans = ck.splans;
  const std::vector<int> &stream_mesh = ck.stream_mesh;
  const synth::Options &opt = ck.opt;
  dsa_encoded *E = ck.E.get();
  const uint32_t ns = (uint32_t)hs.size();
  std::vector<std::vector<uint32_t>> hists(ns);
  {
    std::vector<dsa::PackItem> items;
    for (uint32_t s = 0; s < ns; ++s) {
      if (hs[s].kind == 3 && hs[s].nv == 0) continue;
      if (hs[s].kind == 2 && hs[s].max_value >= dsa::ENC_RAW_SYMBOL_LIMIT && !hs[s].overflow) continue;      // tagged only: no histogram of values (plan_stream)
      if (hs[s].overflow || hs[s].max_value >= hs[s].hist_cap) { hs[s].overflow = 1; continue; }
      items.push_back({hs[s].hist_raw, 0, 4u * (hs[s].max_value + 1u), s});
    }
    std::vector<uint8_t> host;
    ENC_ST(enc_gather(lane, ck.arena, items, &host, nullptr));
    for (auto &it : items) {
      hists[it.pad].resize(it.len / 4);
      memcpy(hists[it.pad].data(), host.data() + it.packed_off, it.len);
    }
  }
  std::vector<std::string> plan_error(ns);
  auto plan_stream = [&](uint32_t s) {
    const uint32_t i = (uint32_t)stream_mesh[s];
    if (E->status[i] != DSA_OK || (hs[s].kind == 3 && hs[s].nv == 0)) return;
    try {
      synth::check(!hs[s].overflow, "symbol outside the histogram range");
      const bool tagged_only = hs[s].kind == 2 && hs[s].max_value >= dsa::ENC_RAW_SYMBOL_LIMIT;
      synth::check(!(tagged_only && opt.force_scheme == 1), dsa::ENC_RAW_BEYOND_MESSAGE);
      synth::SymbolStats stt;
      stt.n = (size_t)hs[s].nv * hs[s].nc; stt.nc = (int)hs[s].nc; stt.max_value = hs[s].max_value; stt.total_bl = hs[s].total_bl;
      stt.tag_freq.assign(hs[s].hist_tag, hs[s].hist_tag + 33);
      stt.raw_freq.assign(hists[s].begin(), hists[s].end());
      synth::plan_symbols(stt, opt.force_scheme, opt.compression_level, splans[s]);
      hs[s].method = (uint32_t)splans[s].method;
      hs[s].precision_bits = (uint32_t)splans[s].coder.precision_bits;
      hs[s].num_symbols = splans[s].coder.num_symbols;
      synth::check(splans[s].coder.num_symbols <= std::max<uint32_t>(hs[s].hist_cap, 64), "alphabet larger than the table region");
    } catch (const std::exception &e) { plan_error[s] = e.what(); if (plan_error[s].empty()) plan_error[s] = "symbol plan failed"; hs[s].overflow = 1; }
  };
  hostutil::parallel_for(ns, plan_stream);
  {
    std::vector<dsa::PackItem> items;
    std::vector<uint8_t> host;
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t i = (uint32_t)stream_mesh[s];
      if (E->status[i] != DSA_OK) continue;
      if (!plan_error[s].empty()) { E->status[i] = DSA_ERR_INVALID_DATA; E->messages[i] = plan_error[s]; continue; }
      const uint32_t bytes = 4u * splans[s].coder.num_symbols;
      for (int t = 0; t < 2; ++t) {
        const std::vector<uint32_t> &src = t == 0 ? splans[s].coder.prob : splans[s].coder.cum;
        items.push_back({t == 0 ? hs[s].prob : hs[s].cum, (uint64_t)host.size(), bytes, s});
        host.insert(host.end(), (const uint8_t *)src.data(), (const uint8_t *)src.data() + bytes);
        host.resize((host.size() + 15) & ~(size_t)15);
      }
    }
    ENC_ST(enc_scatter(lane, ck.arena, items, host));
  }
  return DSA_OK;
}
// the plans of k_enc_plan: what it refused, said per mesh
static void enc_device_plan_errors(EncChunk &ck) {
  const std::vector<dsa::EncStream> &hs = ck.L.streams;
  const std::vector<int> &stream_mesh = ck.stream_mesh;
  dsa_encoded *E = ck.E.get();
  const uint32_t ns = (uint32_t)hs.size();
  for (uint32_t s = 0; s < ns; ++s) {
    const uint32_t i = (uint32_t)stream_mesh[s];
    if (E->status[i] != DSA_OK || !hs[s].overflow) continue;
    E->status[i] = DSA_ERR_INVALID_DATA;
    E->messages[i] = hs[s].plan_status == (uint32_t)dsa::ENC_PLAN_RAW_BEYOND_LIMIT ? dsa::ENC_RAW_BEYOND_MESSAGE
                     : (hs[s].plan_status ? dsa::plan::plan_message((int)hs[s].plan_status) : "symbol outside the histogram range");
  }
}
// ---- device phase 2: entropy coding (behind the host's plans: k_enc_rans here; k_enc_plan's: it has run), then the coded bytes of
// every stream, the probability tables k_enc_plan made and the side bits down in one transfer; splans[s].head receives the bytes in
// front of the payload.
static dsa_status enc_code_streams(dsa_context *ctx, EncLane &lane, EncChunk &ck) {
  uint8_t *arena = ck.arena;
  dsa::EncStream *d_streams = ck.d_streams;
  std::vector<dsa::EncStream> &hs = ck.L.streams;
  std::vector<synth::SymbolPlan> &splans = ck.splans;
  std::vector<std::vector<uint8_t>> &rans = ck.rans, &bits = ck.bits, &flag_bits = ck.flag_bits;
  const std::vector<int> &stream_mesh = ck.stream_mesh;
  const dsa_encoded *E = ck.E.get();
  const bool host_plan = ck.host_plan;
  const uint32_t ns = (uint32_t)hs.size();
  hipStream_t st = lane.st;
  if (host_plan) {
    ENC_TRY(hipMemcpyAsync(d_streams, hs.data(), sizeof(dsa::EncStream) * ns, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dsa::k_enc_rans, dim3(ns), dim3(WAVE), 0, st, arena, d_streams, ns);
    ENC_TRY(hipMemcpyAsync(hs.data(), d_streams, sizeof(dsa::EncStream) * ns, hipMemcpyDeviceToHost, st));
    ENC_TRY(hipStreamSynchronize(st));
  }
  // coded bytes of every stream (and, when k_enc_plan made them, the probability tables: the stream carries them)
  // and the side bits of TexCoordsPortable / GeometricNormal, packed
  // (track_rows: a fifth piece per stream, its entry rows -- k_enc_entry_rows has run behind the attribute kernels)
  // (point_order: the fifth piece of a mesh's first stream is the permutation its streams share -- dsa_encode_order.h; with
  // merge_points the kept rows, nv of them as the records say, and a sixth piece, row_entries of all its input rows)
  // (part_points: the fifth piece of a cloud's first stream is the whole permutation, whose slices its parts' streams read, the
  // sixth the records of its parts with their boxes)
  // (part_cells: both -- the fifth piece the kept rows of the whole cloud, m of them as the sizes of its slots add up, the sixth the
  // records of its live parts, a seventh row_entries; an empty slot -- an empty list by then, ENC_PART_SIZED in its record -- has no
  // piece at all)
  const bool track = !ck.L.rows_of_stream.empty(), ordered = !ck.L.ord.empty(), merge = ck.L.merge, split = ck.L.split, cell_parts = ck.L.cell_parts;
  const size_t per = merge && split ? 7 : (merge || split ? 6 : (track || ordered ? 5 : 4)), cells_piece = split ? 6 : 5;
  std::vector<dsa::PackItem> items;
  for (uint32_t s = 0; s < ns; ++s) {
    if (hs[s].overflow || E->status[stream_mesh[s]] != DSA_OK) continue;
    if ((hs[s].part & dsa::ENC_PART_SIZED) != 0u && hs[s].nv == 0u) continue;
    if (hs[s].kind == 1 && hs[s].prediction == 6) hs[s].num_flags = hs[s].nv;
    items.push_back({hs[s].out_rans, 0, hs[s].rans_len, s});
    items.push_back({hs[s].out_bits, 0, hs[s].bits_len, s});
    items.push_back({hs[s].prob, 0, host_plan ? 0u : 4u * hs[s].num_symbols, s});
    const bool creased = hs[s].kind != 1 && hs[s].prediction == 4;      // (its `flags` hold the four crease lists: below)
    items.push_back({hs[s].flags, 0, hs[s].flags && !creased ? 4u * ((hs[s].num_flags + 31u) / 32u) : 0u, s});
    if (track) {
      const dsa::EncRows *R = ck.L.rows_of_stream[s] != DSA_INVALID ? &ck.L.rows[ck.L.rows_of_stream[s]] : nullptr;
      items.push_back({R ? R->out : 0, 0, R ? 4u * std::min(hs[s].nv, R->cap) : 0u, s});
    } else if (ordered) {
      const bool first = s == ck.L.first_stream[stream_mesh[s]];
      uint32_t order_rows = split ? ck.L.ord[ck.L.ord_of_mesh[stream_mesh[s]]].n : hs[s].nv, part_records = ck.num_parts((uint32_t)stream_mesh[s]);
      if (cell_parts && first) part_records = ck.live_parts((uint32_t)stream_mesh[s], &order_rows);
      items.push_back({hs[s].e2v, 0, first ? 4u * order_rows : 0u, s});
      if (split) items.push_back({ck.L.parts_at + sizeof(dsa::EncPart) * ck.L.part_of_mesh[stream_mesh[s]], 0, first ? (uint32_t)sizeof(dsa::EncPart) * part_records : 0u, s});
      if (merge) { const dsa::EncOrder &O = ck.L.ord[ck.L.ord_of_mesh[stream_mesh[s]]]; items.push_back({O.cells, 0, first ? 4u * O.n : 0u, s}); }
    }
  }
  const uint8_t *host = nullptr;
  ENC_ST(enc_gather(lane, arena, items, nullptr, &host));
  hostutil::parallel_for((uint32_t)(items.size() / per), [&](uint32_t m) {
    const size_t k = per * (size_t)m;
    const uint32_t s = items[k].pad;
    if (split && items[k + 5].len) { const dsa::EncPart *r = (const dsa::EncPart *)(host + items[k + 5].packed_off); ck.part_boxes[s].assign(r, r + items[k + 5].len / sizeof(dsa::EncPart)); }
    if (merge && items[k + cells_piece].len) { const uint32_t *r = (const uint32_t *)(host + items[k + cells_piece].packed_off); ck.row_cells[s].assign(r, r + items[k + cells_piece].len / 4u); }
    if (per >= 5 && items[k + 4].len) { const uint32_t *r = (const uint32_t *)(host + items[k + 4].packed_off); ck.entry_rows[s].assign(r, r + items[k + 4].len / 4u); }
    if (items[k].len) rans[s].assign(host + items[k].packed_off, host + items[k].packed_off + items[k].len);
    if (items[k + 1].len) bits[s].assign(host + items[k + 1].packed_off, host + items[k + 1].packed_off + items[k + 1].len);
    if (hs[s].flags && !(hs[s].kind != 1 && hs[s].prediction == 4)) {
      const uint32_t *words = (const uint32_t *)(host + items[k + 3].packed_off);
      flag_bits[s].resize(hs[s].num_flags);
      for (uint32_t e = 0; e < hs[s].num_flags; ++e) flag_bits[s][e] = (uint8_t)((words[e >> 5] >> (e & 31u)) & 1u);
    }
    if (hs[s].kind == 3 && hs[s].nv == 0) return;
    if (!host_plan) {                      // the bytes in front of the payload: scheme, (raw: unique-symbols bit length), table
      synth::SymbolPlan &pl = splans[s];
      pl.method = (int)hs[s].method;
      pl.coder.num_symbols = hs[s].num_symbols;
      const uint32_t *pr = (const uint32_t *)(host + items[k + 2].packed_off);
      pl.coder.prob.assign(pr, pr + hs[s].num_symbols);
      pl.head.u8((uint8_t)pl.method);
      if (pl.method != 0) pl.head.u8((uint8_t)hs[s].usbl);
      pl.coder.write_table(pl.head);
    }
  }, 8);
  // the crease lists of ConstrainedMultiParallelogram streams (ck.crease[4 s + j]: list j of stream s, a byte per flag): a
  // transfer of their own, made only when the chunk has such streams
  if (ck.L.any_crease) {
    std::vector<dsa::PackItem> citems;
    for (uint32_t s = 0; s < ns; ++s) {
      if (hs[s].overflow || E->status[stream_mesh[s]] != DSA_OK || hs[s].kind == 1 || hs[s].prediction != 4 || !hs[s].flags) continue;
      for (uint32_t j = 0; j < 4; ++j) citems.push_back({hs[s].flags + 4ull * hs[s].cr_at[j], 0, 4u * ((hs[s].cr_n[j] + 31u) / 32u), 4u * s + j});
    }
    const uint8_t *chost = nullptr;
    ENC_ST(enc_gather(lane, arena, citems, nullptr, &chost));
    hostutil::parallel_for((uint32_t)citems.size(), [&](uint32_t m) {
      const dsa::PackItem &it = citems[m];
      const uint32_t cnt = hs[it.pad / 4u].cr_n[it.pad & 3u];
      std::vector<uint8_t> &b = ck.crease[it.pad];
      b.resize(cnt);
      const uint32_t *words = (const uint32_t *)(chost + it.packed_off);
      for (uint32_t e = 0; e < cnt; ++e) b[e] = (uint8_t)((words[e >> 5] >> (e & 31u)) & 1u);
    }, 8);
  }
  return DSA_OK;
}
// a symbol stream as encode_symbols writes it: scheme and table, coded bytes, (tagged) the raw bit fields
static void enc_put_coded(synth::ByteWriter &bw, const synth::SymbolPlan &pl, const std::vector<uint8_t> &rans, const std::vector<uint8_t> &bits, uint32_t method) {
  bw.bytes(pl.head.d);
  bw.varint(rans.size());
  bw.bytes(rans);
  if (method == 0) bw.bytes(bits);
}

// an attribute's coded values as both stream writers carry them (SequentialIntegerAttributeEncoder.cs:55-128): prediction method
// `method` and its transform, the symbols of stream s, the side bits of the method, the transform's data
static void enc_write_attribute_values(synth::ByteWriter &bw, const EncChunk &ck, uint32_t s, int8_t method) {
  const dsa::EncStream &S = ck.L.streams[s];
  bw.i8(method); bw.i8(S.kind == 1 ? 3 : 1);
  bw.u8(1);
  enc_put_coded(bw, ck.splans[s], ck.rans[s], ck.bits[s], S.method);
  if (S.kind == 0 && S.prediction == 5) { bw.i32((int32_t)ck.flag_bits[s].size()); synth::write_rabs(bw, ck.flag_bits[s]); }      // TexCoordsPortable's orientations
  if (S.kind != 1 && S.prediction == 4)                    // ...ConstrainedMultiParallelogramEncoder.cs: the four crease lists
    for (size_t j = 0; j < 4; ++j) { const std::vector<uint8_t> &cl = ck.crease[4 * (size_t)s + j]; bw.varint(cl.size()); if (!cl.empty()) synth::write_rabs(bw, cl); }
  if (S.kind == 1) { const int32_t max_q = (1 << S.bits) - 1; bw.i32(max_q); bw.i32((max_q - 1) / 2); }
  else { bw.i32(S.wrap_mn); bw.i32(S.wrap_mx); }
  if (S.kind == 1 && S.prediction == 6) synth::write_rabs(bw, ck.flag_bits[s]);      // GeometricNormal's flips
}
// AttributeQuantizationTransform.cs:123-134 / AttributeOctahedronTransform.cs:44-47 (an integer attribute has no transform to describe)
static void enc_write_transform(synth::ByteWriter &bw, const dsa::EncStream &S) {
  if (S.kind == 0) { for (uint32_t c = 0; c < S.nc_out; ++c) bw.f32(S.qmin[c]); bw.f32(S.qrange); bw.u8((uint8_t)S.bits); }
  else if (S.kind == 1) bw.u8((uint8_t)S.bits);
}

// DSA_ENC_TIMING=1 (diagnostics): wall time of every stage of a chunk on stderr
struct EncLap {
  const void *lane;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void operator()(const char *what) {
    static const bool timing = getenv("DSA_ENC_TIMING") != nullptr;
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    static const auto t_zero = now;
    fprintf(stderr, "[dsa_encode_batch] lane %p at %9.2f ms: %-28s %8.2f ms\n", lane, std::chrono::duration<double, std::milli>(now - t_zero).count(), what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};
static dsa_status enc_check_bits(dsa_context *ctx, const dsa_encode_options &o) {
  if (o.position_bits < 1 || o.position_bits > 20 || o.texcoord_bits < 1 || o.texcoord_bits > 20 || o.normal_bits < 2 || o.normal_bits > 20)
    return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "quantisation bits out of range (positions/texcoords 1..20, normals 2..20)");
  return DSA_OK;
}
// Both symbol-plan stages and the connectivity are the serial algorithms on one lane per mesh / per stream: a batch takes 150 - 250 ms
// (connectivity) and about 40 ms (plans) whatever its size, which the host threads beat on a small batch (measured: 64 meshes 84 ms
// on the host, 128 meshes 252 ms on the device).  Below 256 meshes the host does both (DSA_ENC_HOST_CONN / DSA_ENC_HOST_PLAN = 1
// or 0 force one or the other; read per call: the tests compare the paths).
static bool enc_host_choice(const char *name, uint32_t batch_n) { const char *e = getenv(name); return e ? atoi(e) != 0 : batch_n < 256; }

// ---- the stages of encode_chunk, in their order
// a weld request (dsa_encode_points_batch, dsa_weld_batch, dsa_encode_corner_attributes_batch over per-point input): the meshes
// arrive as one row per point; the weld of every mesh
// (dsa_encode_weld.h; DSA_ENC_HOST_WELD, batches below 256 meshes: synth::weld_points on the host threads) into buffers the chunk
// owns, and the chunk's mesh view pointed at them -- everything behind runs on the welded meshes as if the caller had passed them.
// Device path: memory of its own per lane, the point arrays up on a turn of the link, the kernels, then counts, maps and welded
// rows back (the welded rows cross the link again with the ordinary uploads: the layout reads host memory).
// false: the mesh is too large for the device weld and is refused
static bool enc_weld_sizes_fit(EncChunk &ck, uint32_t i, const dsa_mesh_input &m, size_t segments, size_t listed) {
  if (m.num_vertices > (1u << 28) || m.num_faces > (1u << 28)) { ck.refuse(i, DSA_ERR_INVALID_DATA, "mesh too large for the device weld"); return false; }
  if (segments + listed + 2 > dsa::EW_MAX_SEGS || listed > dsa::EW_MAX_LISTED) { ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, "too many attributes for the device weld"); return false; }
  return true;
}
// the per-point arrays of mesh `m` into the upload list, in the order of enc_weld_inputs: faces, the vertex key's segments, normals,
// texture coordinates, the listed attributes welded alone (W.seg[g] / W.set[1] / W.set[2] / W.set[3 + j])
static void enc_weld_uploads(std::vector<EncUpload> &ups, const dsa::EncWeld &W, const dsa_mesh_input &m, const std::vector<synth::WeldSeg> &key, const std::vector<synth::WeldSeg> &listed) {
  if (m.num_faces) ups.push_back({W.faces, m.faces, 12ull * m.num_faces, false});
  for (size_t g = 0; g < key.size() && m.num_vertices; ++g) ups.push_back({W.seg[g].src, key[g].rows, (size_t)m.num_vertices * key[g].row_bytes, false});
  if (m.normals && m.num_vertices) ups.push_back({W.seg[W.set[1].first_seg].src, m.normals, 12ull * m.num_vertices, false});
  if (m.texcoords && m.num_vertices) ups.push_back({W.seg[W.set[2].first_seg].src, m.texcoords, 8ull * m.num_vertices, false});
  for (size_t j = 0; j < listed.size() && m.num_vertices; ++j) ups.push_back({W.seg[W.set[3 + j].first_seg].src, listed[j].rows, (size_t)m.num_vertices * listed[j].row_bytes, false});
}
// the lane's weld memory of `total` bytes, cleared behind the inputs; the uploads on a turn of the link; the records up
// (ups is in arena order; a piece of enc_upload copies a whole stretch of the arena from pinned staging, gaps included: that is
// why no region a kernel expects at zero may lie among the inputs)
static dsa_status enc_weld_begin(dsa_context *ctx, EncLane &lane, hostutil::TurnGuard &turn, uint64_t total, uint64_t input_bytes, const std::vector<EncUpload> &ups,
                                 const std::vector<dsa::EncWeld> &recs, uint8_t **arena, dsa::EncWeld **d_recs) {
  ENC_TRY(lane.weld.ensure(total ? total : 256));
  ENC_TRY(lane.weld_recs.ensure(sizeof(dsa::EncWeld) * recs.size()));
  *arena = (uint8_t *)lane.weld.p;
  *d_recs = (dsa::EncWeld *)lane.weld_recs.p;
  if (total > input_bytes) ENC_TRY(hipMemsetAsync(*arena + input_bytes, 0, total - input_bytes, lane.st));
  turn.acquire_free();
  ENC_TRY(enc_upload(lane, *arena, lane.st, ups));
  turn.release();
  ENC_TRY(hipMemcpyAsync(*d_recs, recs.data(), sizeof(dsa::EncWeld) * recs.size(), hipMemcpyHostToDevice, lane.st));
  return DSA_OK;
}
// ... the launches checked, the records down
static dsa_status enc_weld_records(dsa_context *ctx, EncLane &lane, std::vector<dsa::EncWeld> &recs, const dsa::EncWeld *d_recs) {
  ENC_TRY(hipGetLastError());
  ENC_TRY(hipMemcpyAsync(recs.data(), d_recs, sizeof(dsa::EncWeld) * recs.size(), hipMemcpyDeviceToHost, lane.st));
  ENC_TRY(hipStreamSynchronize(lane.st));
  return DSA_OK;
}
// counts known: the maps, the faces and ids, the welded rows in one transfer
struct EncWeldFetch {
  std::vector<dsa::PackItem> items;
  std::vector<void *> dest;
  void want32(std::vector<uint32_t> &v, uint64_t at, uint64_t count) { v.resize(count); if (count) { items.push_back({at, 0, (uint32_t)(4 * count), 0}); dest.push_back(v.data()); } }
  void want8(std::vector<uint8_t> &v, uint64_t at, uint64_t bytes) { v.resize(bytes); if (bytes) { items.push_back({at, 0, (uint32_t)bytes, 0}); dest.push_back(v.data()); } }
  // a key set's maps; one behind the vertex's: its rows (row_bytes each: the set's own classes when some vertex has two, else V) and then its ids
  void want_keys(synth::WeldKeys &keys, const dsa::EncWeldSet &S, uint32_t P) { keys.count = S.count; want32(keys.of_point, S.of, P); want32(keys.point, S.point, S.count); }
  void want_attribute(const dsa::EncWeldSet &S, const dsa::EncWeldSeg &seg, bool seamed, uint32_t V, uint32_t F, uint64_t corners_at, std::vector<uint8_t> &rows, std::vector<uint32_t> &corners) {
    want8(rows, seg.dst, (uint64_t)seg.row_bytes * (seamed ? S.count : V));
    if (seamed) want32(corners, corners_at, 3ull * F);
  }
  dsa_status run(dsa_context *ctx, EncLane &lane, const uint8_t *arena) {
    const uint8_t *host = nullptr;
    ENC_ST(enc_gather(lane, arena, items, nullptr, &host));
    hostutil::parallel_for((uint32_t)items.size(), [&](uint32_t k) { memcpy(dest[k], host + items[k].packed_off, items[k].len); }, 8);
    return DSA_OK;
  }
};
// 3 + L key sets per mesh: listed[i] holds the L attributes of the list welded alone (dsa_encode_corner_attributes_batch with
// weld_attributes = 1), none for dsa_encode_points_batch and dsa_weld_batch
static dsa_status enc_stage_weld(dsa_context *ctx, EncLane &lane, hostutil::TurnGuard &turn, EncChunk &ck) {
  if (!ck.rq.weld) return DSA_OK;
  const uint32_t n = ck.n;
  ck.weld.assign(n, synth::Welded());
  ck.weld_attrs.assign(n, {});
  ck.weld_corners.assign(n, {});
  std::vector<std::vector<synth::WeldSeg>> keys(n), listed(n);
  hostutil::parallel_for(n, [&](uint32_t i) { enc_weld_check(ck, i, keys[i], &listed[i]); });
  const bool on_host = enc_host_choice("DSA_ENC_HOST_WELD", ck.batch_n);
  std::vector<dsa::EncWeld> recs;
  std::vector<uint32_t> mesh_of;
  std::vector<EncUpload> ups;
  EncArena A;
  uint32_t most = 1, sets = 3;
  for (uint32_t i = 0; i < n && !on_host; ++i) {
    if (!ck.good(i)) continue;
    const dsa_mesh_input &m = ck.rq.mesh(ck.base + i);
    if (!enc_weld_sizes_fit(ck, i, m, keys[i].size(), listed[i].size())) continue;
    uint32_t row_bytes[dsa::EW_MAX_SEGS], listed_bytes[dsa::EW_MAX_LISTED];
    for (size_t g = 0; g < keys[i].size(); ++g) row_bytes[g] = keys[i][g].row_bytes;
    for (size_t j = 0; j < listed[i].size(); ++j) listed_bytes[j] = listed[i][j].row_bytes;
    dsa::EncWeld W = dsa::enc_weld_inputs([&](uint64_t bytes) { return A.take(bytes); }, m.num_vertices, m.num_faces, row_bytes, (uint32_t)keys[i].size(), m.normals != nullptr,
                                          m.texcoords != nullptr, listed_bytes, (uint32_t)listed[i].size());
    enc_weld_uploads(ups, W, m, keys[i], listed[i]);
    recs.push_back(W); mesh_of.push_back(i);
    most = std::max(most, std::max(m.num_vertices, 3u * m.num_faces));
    sets = std::max(sets, W.num_sets);
  }
  const uint64_t input_bytes = A.cur;                      // the uploads fill [0, input_bytes); the kernels' regions lie behind
  for (dsa::EncWeld &W : recs) dsa::enc_weld_regions([&](uint64_t bytes) { return A.take(bytes); }, W);
  if (on_host) {
    hostutil::parallel_for(n, [&](uint32_t i) {
      if (!ck.good(i)) return;
      const dsa_mesh_input &m = ck.rq.mesh(ck.base + i);
      try { synth::weld_points(m.num_vertices, m.faces, m.num_faces, keys[i], m.normals, m.texcoords, ck.weld[i], listed[i]); }
      catch (const std::exception &e) { ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
    });
  } else if (!recs.empty()) {
    const uint32_t nr = (uint32_t)recs.size();
    hipStream_t st = lane.st;
    uint8_t *arena = nullptr;
    dsa::EncWeld *d_recs = nullptr;
    ENC_STAGE(enc_weld_begin(ctx, lane, turn, A.cur, input_bytes, ups, recs, &arena, &d_recs));
    const uint32_t gx = std::max(1u, std::min(128u, (most + 1023u) / 1024u));
    dsa::enc_weld_launch([st](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { hipLaunchKernelGGL(kernel, dim3(grid_x, grid_y), dim3(block), 0, st, args...); },
                         arena, d_recs, nr, sets, gx);
    ENC_STAGE(enc_weld_records(ctx, lane, recs, d_recs));
    EncWeldFetch fetch;
    for (uint32_t r = 0; r < nr; ++r) {
      const uint32_t i = mesh_of[r];
      const dsa::EncWeld &W = recs[r];
      bool sane = W.status == dsa::ENC_WELD_OK;
      for (uint32_t k = 0; k < W.num_sets; ++k) sane = sane && W.set[k].count <= W.P;
      if (!sane) { ck.refuse(i, DSA_ERR_INVALID_DATA, dsa::enc_weld_message(W.status)); continue; }
      synth::Welded &w = ck.weld[i];
      w.P = W.P; w.F = W.F;
      w.listed.assign(W.num_sets - 3u, synth::Welded::Listed());
      const uint32_t V = W.set[0].count;
      fetch.want32(w.faces, W.faces_out, 3ull * W.F);
      w.vertex_rows.resize(W.set[0].num_segs);
      for (uint32_t g = 0; g < W.set[0].num_segs; ++g) fetch.want8(w.vertex_rows[g], W.seg[g].dst, (uint64_t)V * W.seg[g].row_bytes);
      for (uint32_t k = 0; k < W.num_sets; ++k) {
        const dsa::EncWeldSet &S = W.set[k];
        if (S.num_segs == 0) continue;
        if (k == 0) { fetch.want_keys(w.vertex, S, W.P); continue; }
        const synth::Welded::KeySet a = w.key_set(k);
        const bool seamed = W.differs[k] != 0;
        fetch.want_keys(a.keys, S, W.P);
        a.per_vertex = !seamed;
        fetch.want_attribute(S, W.seg[S.first_seg], seamed, V, W.F, W.corners_out[k], a.rows, a.corners);
      }
    }
    ENC_STAGE(fetch.run(ctx, lane, arena));
  }
  ck.welded.resize(n);
  for (uint32_t i = 0; i < n; ++i) enc_weld_view(ck, i);
  return DSA_OK;
}
// host phase 1: checks, connectivity, traversal order, operand entries (threads over meshes)
static dsa_status enc_stage_plans(dsa_context *ctx, EncChunk &ck) {
  // (the quantisation bits of an Edgebreaker call are checked here, per chunk: a call with n = 0 has no chunk and returns DSA_OK
  // whatever they are, while a sequential call checks them up front -- enc_check_options)
  if (enc_check_bits(ctx, ck.rq.base()) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  enc_begin_plans(ck, enc_host_choice("DSA_ENC_HOST_CONN", ck.batch_n), enc_host_choice("DSA_ENC_HOST_PLAN", ck.batch_n));
  hostutil::parallel_for(ck.n, [&](uint32_t i) { if (ck.good(i)) enc_plan_mesh(ck, i); });          // (a mesh the weld refused stays refused) capped thread count, every thread joined on every path (dsa_host_util.h)
  return DSA_OK;
}
// a repair request on the device path (dsa_encode_repair.h): the repaired corner table of every mesh by the repair kernels, in
// device memory of its own; the tables come back, the host counts degenerate faces and isolated vertices out
// (CornerTable::from_repaired) and the layout that follows is that of the meshes at their real sizes.  Host connectivity: the
// host coder repaired the table in enc_plan_mesh.
static dsa_status enc_stage_repair(dsa_context *ctx, EncLane &lane, EncChunk &ck) {
  if (!ck.rq.repair || ck.host_conn) return DSA_OK;
  const uint32_t n = ck.n;
  ck.rep.assign(n, synth::CornerTable());
  std::vector<dsa::EncRepair> recs;
  std::vector<dsa::EncRepairIds> id_recs;      // attributes given per corner (EncRequest::corner_repair): their ids go up with the faces, the ids of the coded faces stay on the device for the layout
  std::vector<const uint32_t *> id_src;
  std::vector<uint32_t> mesh_of;
  EncArena A;
  uint32_t maxf = 1;
  if (ck.rq.corner_repair) ck.rep_ids.assign(n, {});
  for (uint32_t i = 0; i < n; ++i) {
    if (!ck.good(i)) continue;
    const dsa_mesh_input &m = ck.mesh(i);
    const uint64_t F = m.num_faces, V = m.num_vertices;
    dsa::EncRepair R;
    memset(&R, 0, sizeof(R));
    R.F = m.num_faces; R.V = m.num_vertices;
    R.faces = A.take(12 * F); R.c2v = A.take(12 * F); R.opp = A.take(12 * F); R.parent = A.take(12 * F);
    R.voff = A.take(4 * (V + 1)); R.vcur = A.take(4 * V); R.vlist = A.take(12 * F);
    R.pend = A.take(3 * F); R.bvis = A.take(3 * F); R.cvis = A.take(3 * F); R.vvis = A.take(V); R.stamp = A.take(12 * V);
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    for (size_t k = 0; ck.rq.corner_repair && k < atts.size(); ++k) {
      if (!atts[k].corner_value) continue;
      if (!R.fmap) { R.fmap = A.take(4 * F); ck.rep_ids[i].assign(atts.size(), EncChunk::kNoIds); }
      dsa::EncRepairIds I;
      memset(&I, 0, sizeof(I));
      I.rep = (uint32_t)recs.size(); I.rows = ck.rows_of(i, atts[k]); I.narrow = ck.ids_narrow(i, atts[k]) ? 1u : 0u; I.att_type = atts[k].extra_index >= 0 ? 0x100u + (uint32_t)atts[k].extra_index : (uint32_t)atts[k].att_type;
      I.src = A.take(12 * F); I.dst = A.take((I.narrow ? 6 : 12) * F);
      ck.rep_ids[i][k] = I.dst;
      id_recs.push_back(I); id_src.push_back(atts[k].corner_value);
    }
    recs.push_back(R); mesh_of.push_back(i);
    maxf = std::max(maxf, m.num_faces);
  }
  const uint32_t nr = (uint32_t)recs.size(), ni = (uint32_t)id_recs.size();
  if (!nr) return DSA_OK;
  hipStream_t st = lane.st;
  ENC_TRY(lane.repair.ensure(A.cur));
  ENC_TRY(lane.repair_recs.ensure(std::max(sizeof(dsa::EncRepair), sizeof(dsa::EncRepairRows)) * n));
  if (ni) ENC_TRY(lane.repair_ids.ensure(sizeof(dsa::EncRepairIds) * ni));
  uint8_t *arena = (uint8_t *)lane.repair.p;
  dsa::EncRepair *d_recs = (dsa::EncRepair *)lane.repair_recs.p;
  dsa::EncRepairIds *d_ids = (dsa::EncRepairIds *)lane.repair_ids.p;
  ENC_TRY(hipMemsetAsync(arena, 0, A.cur, st));
  for (uint32_t r = 0; r < nr; ++r) ENC_TRY(hipMemcpyAsync(arena + recs[r].faces, ck.mesh(mesh_of[r]).faces, 12ull * recs[r].F, hipMemcpyHostToDevice, st));
  for (uint32_t q = 0; q < ni; ++q) ENC_TRY(hipMemcpyAsync(arena + id_recs[q].src, id_src[q], 12ull * recs[id_recs[q].rep].F, hipMemcpyHostToDevice, st));
  ENC_TRY(hipMemcpyAsync(d_recs, recs.data(), sizeof(dsa::EncRepair) * nr, hipMemcpyHostToDevice, st));
  if (ni) ENC_TRY(hipMemcpyAsync(d_ids, id_recs.data(), sizeof(dsa::EncRepairIds) * ni, hipMemcpyHostToDevice, st));
  const uint32_t walk_lanes = 16;
  const dim3 gt(std::max(1u, std::min(128u, (3u * maxf + 1023u) / 1024u)), nr);
  hipLaunchKernelGGL(dsa::k_enc_repair_mark, gt, dim3(256), 0, st, arena, d_recs, nr);
  if (ni) {                  // (in front of the break pass: it marks the corners it visits in the array the scan reads)
    hipLaunchKernelGGL(dsa::k_enc_repair_face_scan, dim3(nr), dim3(WAVE), 0, st, arena, d_recs, nr);
    hipLaunchKernelGGL(dsa::k_enc_repair_ids, dim3(gt.x, ni), dim3(256), 0, st, arena, d_recs, d_ids, ni);
  }
  hipLaunchKernelGGL(dsa::k_enc_repair_offsets, dim3(nr), dim3(WAVE), 0, st, arena, d_recs, nr);
  hipLaunchKernelGGL(dsa::k_enc_repair_lists, gt, dim3(256), 0, st, arena, d_recs, nr);
  hipLaunchKernelGGL(dsa::k_enc_repair_opposites, gt, dim3(256), 0, st, arena, d_recs, nr);
  hipLaunchKernelGGL(dsa::k_enc_repair_fans, dim3((nr + walk_lanes - 1) / walk_lanes), dim3(WAVE), 0, st, arena, d_recs, nr, walk_lanes);
  ENC_TRY(hipGetLastError());
  ENC_TRY(hipMemcpyAsync(recs.data(), d_recs, sizeof(dsa::EncRepair) * nr, hipMemcpyDeviceToHost, st));
  if (ni) ENC_TRY(hipMemcpyAsync(id_recs.data(), d_ids, sizeof(dsa::EncRepairIds) * ni, hipMemcpyDeviceToHost, st));
  ENC_TRY(hipStreamSynchronize(st));
  for (const dsa::EncRepairIds &I : id_recs)      // (the host's checks saw every id before; the kernel's answer is the same one)
    if (I.bad && ck.good(mesh_of[I.rep]))
      ck.refuse(mesh_of[I.rep], DSA_ERR_INVALID_DATA, I.att_type >= 0x100u ? "attribute " + std::to_string(I.att_type - 0x100u) + " id out of range" : std::string(I.att_type == 1 ? "normal id out of range" : "texture coordinate id out of range"));
  std::vector<synth::CornerTable::Repaired> out(nr);
  for (uint32_t r = 0; r < nr; ++r) {
    const dsa::EncRepair &R = recs[r];
    if (R.status != dsa::ENC_REPAIR_OK || R.num_vertices < R.V || R.num_vertices - R.V > 3ull * R.F) continue;
    synth::CornerTable::Repaired &o = out[r];
    o.c2v.resize(3ull * R.F); o.opp.resize(3ull * R.F); o.parent.resize(R.num_vertices - R.V);
    ENC_TRY(hipMemcpyAsync(o.c2v.data(), arena + R.c2v, 12ull * R.F, hipMemcpyDeviceToHost, st));
    ENC_TRY(hipMemcpyAsync(o.opp.data(), arena + R.opp, 12ull * R.F, hipMemcpyDeviceToHost, st));
    if (!o.parent.empty()) ENC_TRY(hipMemcpyAsync(o.parent.data(), arena + R.parent, 4ull * o.parent.size(), hipMemcpyDeviceToHost, st));
    o.num_vertices = R.num_vertices; o.isolated = R.isolated; o.degenerate = R.degenerate; o.breaks = R.breaks;
  }
  ENC_TRY(hipStreamSynchronize(st));
  hostutil::parallel_for(nr, [&](uint32_t r) {
    const uint32_t i = mesh_of[r];
    const dsa::EncRepair &R = recs[r];
    if (!ck.good(i)) return;
    if (R.status != dsa::ENC_REPAIR_OK) return ck.refuse(i, DSA_ERR_INVALID_DATA, dsa::enc_repair_message(R.status));
    if (out[r].c2v.empty()) return ck.refuse(i, DSA_ERR_INVALID_DATA, dsa::enc_repair_message(~0u));
    try {
      const dsa_mesh_input &m = ck.mesh(i);
      synth::CornerTable &t = ck.rep[i];
      t.from_repaired(out[r], m.faces, m.num_faces, m.num_vertices);
      synth::check(!R.fmap || R.coded_faces == t.nf(), dsa::enc_repair_message(~0u));      // (the ids were compacted over the faces the scan kept)
      ck.c2row[i].resize(t.nc());
      for (uint32_t c = 0; c < t.nc(); ++c) ck.c2row[i][c] = t.row[t.c2v[c]];
    } catch (const std::exception &e) { ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
  });
  return DSA_OK;
}
// the lane's device memory for the layout, cleared (histograms start at zero); the first uploads (host connectivity: all of them;
// else phase A, what the walks need) on the chunk's turn on the link; the stream records.  Shared with encode_sequential_chunk.
static dsa_status enc_stage_uploads(dsa_context *ctx, EncLane &lane, hostutil::TurnGuard &turn, EncChunk &ck) {
  const EncLayout &L = ck.L;
  const bool all = ck.host_conn || ck.rq.sequential;
  ENC_TRY(lane.arena.ensure(L.total_bytes ? L.total_bytes : 256));
  ENC_TRY(lane.streams.ensure(sizeof(dsa::EncStream) * L.streams.size()));
  ck.arena = (uint8_t *)lane.arena.p; ck.d_streams = (dsa::EncStream *)lane.streams.p;
  if (lane.walk_st) ENC_TRY(hipStreamSynchronize(lane.walk_st));     // (idle unless a previous chunk on this lane ended in an error)
  ENC_TRY(hipMemsetAsync(ck.arena, 0, L.total_bytes, lane.st));
  turn.acquire_a();
  ENC_TRY(enc_upload(lane, ck.arena, lane.st, all ? L.uploads : L.uploads_a));
  if (all) turn.release();
  if (!L.copies_a.empty()) {      // the ids of the coded faces, device to device from the repair arena (behind the upload: a piece of it covers the gaps between its regions)
    static_assert(sizeof(EncCopy) == sizeof(dsa::PackItem) && offsetof(EncCopy, src_off) == offsetof(dsa::PackItem, packed_off) && offsetof(EncCopy, bytes) == offsetof(dsa::PackItem, len), "EncCopy is a PackItem");
    const uint32_t nc = (uint32_t)L.copies_a.size();        // (the layout's: alive until the chunk ends)
    ENC_TRY(lane.items.ensure(sizeof(dsa::PackItem) * nc));
    ENC_TRY(hipMemcpyAsync(lane.items.p, L.copies_a.data(), sizeof(dsa::PackItem) * nc, hipMemcpyHostToDevice, lane.st));
    hipLaunchKernelGGL(dsa::k_enc_unpack, dim3(nc), dim3(256), 0, lane.st, ck.arena, (const uint8_t *)lane.repair.p, (const dsa::PackItem *)lane.items.p, nc);
    ENC_TRY(hipGetLastError());
  }
  ENC_TRY(hipMemcpyAsync(ck.d_streams, L.streams.data(), sizeof(dsa::EncStream) * L.streams.size(), hipMemcpyHostToDevice, lane.st));
  return DSA_OK;
}
// device phase 0 (device connectivity): corner table, Edgebreaker symbols, attribute order (one wave per mesh); meshes that failed
// the host's checks have F = 0 and no arrays.  The walks on their stream; behind them the rest of the uploads.
static dsa_status enc_stage_connectivity(dsa_context *ctx, EncLane &lane, hostutil::TurnGuard &turn, EncChunk &ck) {
  if (ck.host_conn) return DSA_OK;
  EncLayout &L = ck.L;
  const uint32_t n = ck.n, nz = (uint32_t)L.seams.size();
  // meshes to a wave of the walks (k_enc_connectivity: one lane per mesh); DSA_ENC_WALK_LANES = 1 .. 64 for measurements
  const uint32_t walk_lanes = [&]() { const char *e = getenv("DSA_ENC_WALK_LANES"); const int v = e ? atoi(e) : 0; return (uint32_t)(v >= 1 && v <= 64 ? v : 16); }();
  hipStream_t st = lane.st;
  uint8_t *arena = ck.arena;
  ENC_TRY(lane.conns.ensure(sizeof(dsa::EncConn) * n));
  dsa::EncConn *d_conns = ck.d_conns = (dsa::EncConn *)lane.conns.p;
  ENC_TRY(hipMemcpyAsync(d_conns, L.conns.data(), sizeof(dsa::EncConn) * n, hipMemcpyHostToDevice, st));
  const dim3 gt(std::max(1u, std::min(128u, (3u * L.maxf + 1023u) / 1024u)), n);        // table kernels: blocks per mesh x meshes
  hipLaunchKernelGGL(dsa::k_enc_table_clear, gt, dim3(256), 0, st, arena, d_conns, n);
  hipLaunchKernelGGL(dsa::k_enc_table_count, gt, dim3(256), 0, st, arena, d_conns, n);
  hipLaunchKernelGGL(dsa::k_enc_table_offsets, dim3(n), dim3(WAVE), 0, st, arena, d_conns, n);
  hipLaunchKernelGGL(dsa::k_enc_table_lists, gt, dim3(256), 0, st, arena, d_conns, n);
  if (ck.rep.empty()) hipLaunchKernelGGL(dsa::k_enc_table_opposites, gt, dim3(256), 0, st, arena, d_conns, n);      // (a repaired table's opposites came with its faces)
  hipLaunchKernelGGL(dsa::k_enc_table_corners, gt, dim3(256), 0, st, arena, d_conns, n);
  if (ck.rq.repair_scan) hipLaunchKernelGGL(dsa::k_enc_repair_scan, gt, dim3(256), 0, st, arena, d_conns, n);
  // the walks on their stream; the attribute values travel and are quantised meanwhile
  ENC_TRY(hipEventRecord(lane.tables_done, st));
  ENC_TRY(hipStreamWaitEvent(lane.walk_st, lane.tables_done, 0));
  hipLaunchKernelGGL(L.any_valence ? dsa::k_enc_connectivity_timed : dsa::k_enc_connectivity, dim3((n + walk_lanes - 1) / walk_lanes), dim3(WAVE), 0, lane.walk_st, arena, d_conns, n, walk_lanes);
  if (ck.want_pd) hipLaunchKernelGGL(dsa::k_enc_pd_walk, dim3((n + walk_lanes - 1) / walk_lanes), dim3(WAVE), 0, lane.walk_st, arena, d_conns, n, walk_lanes);
  if (nz) {
    // attributes given per corner: seams and attribute vertices beside the connectivity walk, the attribute walks behind it
    ENC_TRY(lane.seams.ensure(sizeof(dsa::EncSeam) * nz));
    dsa::EncSeam *d_seams = ck.d_seams = (dsa::EncSeam *)lane.seams.p;
    ENC_TRY(hipMemcpyAsync(d_seams, L.seams.data(), sizeof(dsa::EncSeam) * nz, hipMemcpyHostToDevice, st));
    const dim3 gz(gt.x, nz);
    hipLaunchKernelGGL(dsa::k_enc_seam_edges, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
    hipLaunchKernelGGL(dsa::k_enc_seam_fans, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
    hipLaunchKernelGGL(dsa::k_enc_seam_offsets, dim3(nz), dim3(WAVE), 0, st, arena, d_conns, d_seams, nz);
    hipLaunchKernelGGL(dsa::k_enc_seam_assign, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
    hipLaunchKernelGGL(dsa::k_enc_seam_records, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
    ENC_TRY(hipEventRecord(lane.seams_done, st));
    ENC_TRY(hipStreamWaitEvent(lane.walk_st, lane.seams_done, 0));
    hipLaunchKernelGGL(dsa::k_enc_seam_walk, dim3((nz + walk_lanes - 1) / walk_lanes), dim3(WAVE), 0, lane.walk_st, arena, d_conns, d_seams, nz, walk_lanes);
  }
  if (L.any_valence) {
    // valence context lists behind the walks, on their stream: one more serial pass per mesh, then the lists into six streams
    hipLaunchKernelGGL(dsa::k_enc_val_init, gt, dim3(256), 0, lane.walk_st, arena, d_conns, n);
    hipLaunchKernelGGL(dsa::k_enc_valence, dim3((n + walk_lanes - 1) / walk_lanes), dim3(WAVE), 0, lane.walk_st, arena, d_conns, n, walk_lanes);
    hipLaunchKernelGGL(dsa::k_enc_val_split<dsa::EncStream>, dim3(n), dim3(WAVE), 0, lane.walk_st, arena, d_conns, n, ck.d_streams);
  }
  ENC_TRY(hipEventRecord(lane.walk_done, lane.walk_st));
  turn.release();
  turn.acquire_b();
  ENC_TRY(enc_upload(lane, arena, st, L.uploads));
  turn.release();
  return DSA_OK;
}
// device phase 1: quantise, (device connectivity, behind the walks: operand entries, seam results) order, correct, count; a
// sequential chunk: the same kernels in point order, and the index symbols; without a host round trip for the plans device phase
// 2 follows at once; then the records come back.  Shared with encode_sequential_chunk.
static dsa_status enc_stage_attributes(dsa_context *ctx, EncLane &lane, EncChunk &ck) {
  EncLayout &L = ck.L;
  const uint32_t n = ck.n, ns = (uint32_t)L.streams.size(), nz = (uint32_t)L.seams.size(), nx = (uint32_t)L.idx.size();
  const bool sequential = ck.rq.sequential, device_conn = !ck.host_conn && !sequential;
  hipStream_t st = lane.st;
  uint8_t *arena = ck.arena;
  dsa::EncStream *d_streams = ck.d_streams;
  dsa::EncConn *d_conns = ck.d_conns;
  dsa::EncSeam *d_seams = ck.d_seams;
  const uint32_t gx = std::max(1u, std::min(64u, (L.max_rows + 2047) / 2048));
  bool order_timing = false;
  EncLap order_lap{&lane};
  // a grid of (gx, streams) blocks, in slices of what the y of a grid holds: a split cloud of many parts has more streams than that
  // (every other chunk: one launch, as ever)
  auto over_streams = [&](auto kernel) {
    for (uint32_t s = 0; s < ns; s += 65535u) { const uint32_t cnt = std::min(65535u, ns - s); hipLaunchKernelGGL(kernel, dim3(gx, cnt), dim3(256), 0, st, arena, d_streams + s, cnt); }
  };
  if (!L.any_grid) {
    hipLaunchKernelGGL(dsa::k_enc_bounds<false>, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
    over_streams(dsa::k_enc_quantize<false>);
  } else {                   // streams on a grid of the caller's or of their group: their bounds are given, their values are checked
    hipLaunchKernelGGL(dsa::k_enc_bounds<true>, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
    over_streams(dsa::k_enc_quantize<true>);
    over_streams(dsa::k_enc_grid_quantize<dsa::EncStream>);
  }
  if (device_conn) {
    const dim3 gt(std::max(1u, std::min(128u, (3u * L.maxf + 1023u) / 1024u)), n), gz(gt.x, nz);
    ENC_TRY(hipStreamWaitEvent(st, lane.walk_done, 0));
    hipLaunchKernelGGL(dsa::k_enc_operands, gt, dim3(256), 0, st, arena, d_conns, n);
    if (ck.want_pd) hipLaunchKernelGGL(dsa::k_enc_pd_operands, gt, dim3(256), 0, st, arena, d_conns, n);
    if (!ck.rep_rows.empty()) {                                // repaired tables: an entry reads the row of its vertex
      const uint32_t nr = (uint32_t)ck.rep_rows.size();
      ENC_TRY(lane.repair_recs.ensure(sizeof(dsa::EncRepairRows) * nr));
      ENC_TRY(hipMemcpyAsync(lane.repair_recs.p, ck.rep_rows.data(), sizeof(dsa::EncRepairRows) * nr, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(dsa::k_enc_repair_rows, dim3(gx, nr), dim3(256), 0, st, arena, (const dsa::EncRepairRows *)lane.repair_recs.p, nr);
    }
    if (nz) {
      hipLaunchKernelGGL(dsa::k_enc_seam_operands<dsa::EncStream>, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz, d_streams);
      if (ck.want_pd) hipLaunchKernelGGL(dsa::k_enc_pd_corner_streams<dsa::EncStream>, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz, d_streams);
      hipLaunchKernelGGL(dsa::k_enc_seam_topo<dsa::EncStream>, dim3((nz + 255) / 256), dim3(256), 0, st, d_conns, d_seams, nz, d_streams);
      hipLaunchKernelGGL(dsa::k_enc_seam_rank, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
      hipLaunchKernelGGL(dsa::k_enc_seam_count, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
      hipLaunchKernelGGL(dsa::k_enc_seam_scan, dim3(nz), dim3(WAVE), 0, st, arena, d_conns, d_seams, nz);
      hipLaunchKernelGGL(dsa::k_enc_seam_bits, gz, dim3(256), 0, st, arena, d_conns, d_seams, nz);
    }
  }
  if (!L.ord.empty()) {      // point_order: the permutation of every cloud behind the quantisers, in front of the gather (dsa_encode_order.h)
    // DSA_ENC_TIMING (read per chunk: tools/encode_order_timing.py times one leg of a process): the stream is drained around the
    // order kernels and behind the stage, and the three laps say what share of the chunk's device time the order takes (with
    // merge_points a fourth around the merge kernels: tools/encode_merge_timing.py)
    order_timing = getenv("DSA_ENC_TIMING") != nullptr;
    if (order_timing) { ENC_TRY(hipStreamSynchronize(st)); order_lap("uploads + quantisers"); }
    const uint32_t gf = L.max_count ? std::max(1u, std::min(64u, (L.max_count + 1023u) / 1024u)) : 0u;
    // the stage's one launch sequence (enc_order_stage, dsa_encode_layout.h); `said`: what the first call of it that failed left
    dsa_status said = DSA_OK;
    auto zero = [&](uint64_t off, uint64_t bytes) -> dsa_status { ENC_TRY(hipMemsetAsync(arena + off, 0, bytes, st)); return DSA_OK; };
    auto behind = [&](const char *lap) -> dsa_status { ENC_TRY(hipGetLastError()); if (order_timing && lap) { ENC_TRY(hipStreamSynchronize(st)); order_lap(lap); } return DSA_OK; };
    if (!enc_order_stage([st](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { hipLaunchKernelGGL(kernel, dim3(grid_x, grid_y), dim3(block), 0, st, args...); },
                         [&](uint64_t off, uint64_t bytes) { if (said == DSA_OK) said = zero(off, bytes); },
                         [&](const char *lap) { if (said == DSA_OK) said = behind(lap); return said == DSA_OK; },
                         L, ck.rq.seq.geometry == 1, gf, arena, d_streams, ns))
      return said;
  }
  hipLaunchKernelGGL(dsa::k_enc_gather, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
  over_streams(dsa::k_enc_corr);
  if (L.any_multi) hipLaunchKernelGGL(dsa::k_enc_multi<dsa::EncStream>, dim3(gx, ns), dim3(256), 0, st, arena, d_streams, ns);
  if (L.any_crease) hipLaunchKernelGGL(dsa::k_enc_crease<dsa::EncStream>, dim3(ns), dim3(WAVE), 0, st, arena, d_streams, ns);
  if (!sequential) {
    hipLaunchKernelGGL(dsa::k_enc_orient, dim3(ns), dim3(WAVE), 0, st, arena, d_streams, ns);
    hipLaunchKernelGGL(dsa::k_enc_list_stats, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
  }
  if (nx) {                  // compressed indices of sequential meshes: their symbols and statistics
    ENC_TRY(lane.conns.ensure(sizeof(dsa::EncSeqIdx) * nx));
    dsa::EncSeqIdx *d_idx = (dsa::EncSeqIdx *)lane.conns.p;
    ENC_TRY(hipMemcpyAsync(d_idx, L.idx.data(), sizeof(dsa::EncSeqIdx) * nx, hipMemcpyHostToDevice, st));
    const uint32_t gi = std::max(1u, std::min(64u, (L.max_count + SEQ_SYMBOLS_PER_BLOCK - 1) / SEQ_SYMBOLS_PER_BLOCK));
    hipLaunchKernelGGL(dsa::k_enc_seq_indices<dsa::EncStream>, dim3(gi, nx), dim3(SEQ_BLOCK), 0, st, arena, d_idx, nx, d_streams);
  }
  if (!ck.host_plan) {       // tables by k_enc_plan
    hipLaunchKernelGGL(dsa::k_enc_plan, dim3((ns + WAVE - 1) / WAVE), dim3(WAVE), 0, st, arena, d_streams, ns, (int)ck.opt.force_scheme, (int)ck.opt.compression_level);
    hipLaunchKernelGGL(dsa::k_enc_rans, dim3(ns), dim3(WAVE), 0, st, arena, d_streams, ns);
  }
  if (!L.rows.empty()) {     // track_rows: entry -> value row (-> point of a weld request), where the orders still lie (dsa_encode_rows.h)
    const uint32_t nr = (uint32_t)L.rows.size();
    ENC_TRY(lane.rows.ensure(sizeof(dsa::EncRows) * nr));
    ENC_TRY(hipMemcpyAsync(lane.rows.p, L.rows.data(), sizeof(dsa::EncRows) * nr, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dsa::k_enc_entry_rows<dsa::EncStream>, dim3(gx, nr), dim3(256), 0, st, arena, (const dsa::EncRows *)lane.rows.p, nr, (const dsa::EncStream *)d_streams);
  }
  if (sequential) ENC_TRY(hipGetLastError());
  ENC_TRY(hipMemcpyAsync(L.streams.data(), d_streams, sizeof(dsa::EncStream) * ns, hipMemcpyDeviceToHost, st));
  if (device_conn) ENC_TRY(hipMemcpyAsync(L.conns.data(), d_conns, sizeof(dsa::EncConn) * n, hipMemcpyDeviceToHost, st));
  if (nz) ENC_TRY(hipMemcpyAsync(L.seams.data(), d_seams, sizeof(dsa::EncSeam) * nz, hipMemcpyDeviceToHost, st));
  // vote_attributes: the records of the voted streams, for EncVote::full (enc_vote_refusals)
  if (!L.votes.empty()) ENC_TRY(hipMemcpyAsync(L.votes.data(), arena + L.vote_pass.records_at, sizeof(dsa::EncVote) * L.votes.size(), hipMemcpyDeviceToHost, st));
  ENC_TRY(hipStreamSynchronize(st));
  if (order_timing) order_lap("gather to entropy coding");
  return DSA_OK;
}
// a mesh the device refused: its status, and its attribute streams are not coded
static void enc_refuse_mesh(EncChunk &ck, uint32_t i, const char *why) {
  ck.refuse(i, DSA_ERR_INVALID_DATA, why);
  for (uint32_t s = ck.L.first_stream[i]; s < ck.L.first_stream[i + 1]; ++s) ck.L.streams[s].overflow = 1;
}
// device connectivity: what the stream layout needs of it (symbols, start-face bits, split events, two counts) and of the
// attributes given per corner (which are seamed, and their seam bits) comes down packed; a failed step fails its mesh
static dsa_status enc_stage_conn_results(dsa_context *ctx, EncLane &lane, EncChunk &ck) {
  if (ck.host_conn) return DSA_OK;
  const EncLayout &L = ck.L;
  std::vector<dsa::PackItem> conn_items;
  for (uint32_t i = 0; i < ck.n; ++i) {
    if (!ck.good(i)) continue;
    const dsa::EncConn &C = L.conns[i];
    if (C.status != dsa::ENC_OK) { enc_refuse_mesh(ck, i, dsa::enc_conn_message(C.status)); continue; }
    conn_items.push_back({C.symbols, 0, C.num_symbols, i});
    conn_items.push_back({C.start_bits, 0, C.num_start_bits, i});
    conn_items.push_back({C.splits, 0, 12u * C.num_splits, i});
    ck.plans[i].interior_edges = (int64_t)C.interior_edges;
    if (!ck.rep.empty()) { ck.plans[i].coded_vertices = C.V; ck.plans[i].coded_faces = C.F; }
  }
  const uint8_t *conn_host = nullptr;
  ENC_ST(enc_gather(lane, ck.arena, conn_items, nullptr, &conn_host));
  hostutil::parallel_for((uint32_t)(conn_items.size() / 3), [&](uint32_t m) {
    const size_t k = 3 * (size_t)m;
    const uint32_t i = conn_items[k].pad;
    const dsa::EncConn &C = L.conns[i];
    synth::EbResult &eb = ck.plans[i].eb;
    eb.num_split_symbols = C.num_split_symbols;
    if (conn_items[k].len) eb.symbols.assign(conn_host + conn_items[k].packed_off, conn_host + conn_items[k].packed_off + conn_items[k].len);
    if (conn_items[k + 1].len) eb.start_face_bits.assign(conn_host + conn_items[k + 1].packed_off, conn_host + conn_items[k + 1].packed_off + conn_items[k + 1].len);
    eb.splits.resize(C.num_splits);
    const uint32_t *sp = C.num_splits ? (const uint32_t *)(conn_host + conn_items[k + 2].packed_off) : nullptr;
    for (size_t q = 0; q < eb.splits.size(); ++q) eb.splits[q] = {sp[3 * q], sp[3 * q + 1], sp[3 * q + 2]};
  }, 8);
  std::vector<dsa::PackItem> seam_items;
  for (uint32_t z = 0; z < L.seams.size(); ++z) {
    const dsa::EncSeam &Z = L.seams[z];
    const uint32_t i = Z.mesh;
    if (!ck.good(i)) continue;
    if (Z.status != dsa::ENC_SEAM_OK) { enc_refuse_mesh(ck, i, dsa::enc_seam_message(Z.status)); continue; }
    synth::MeshPlan &pl = ck.plans[i];
    if (pl.seamed_given.empty()) pl.seamed_given.assign(pl.atts.size(), 0);
    pl.seamed_given[Z.stream - L.first_stream[i]] = Z.interior_seams ? 1 : 0;
    if (Z.interior_seams) seam_items.push_back({Z.bits, 0, 4u * ((L.conns[i].interior_edges + 31u) / 32u), z});
  }
  std::vector<uint8_t> seam_host;
  ENC_ST(enc_gather(lane, ck.arena, seam_items, &seam_host, nullptr));
  for (auto &it : seam_items) {
    const dsa::EncSeam &Z = L.seams[it.pad];
    synth::MeshPlan &pl = ck.plans[Z.mesh];
    if (!ck.good(Z.mesh)) continue;
    const uint32_t ne = L.conns[Z.mesh].interior_edges;
    if (pl.seam_bits_given.empty()) pl.seam_bits_given.assign(pl.atts.size(), std::vector<uint8_t>(ne, 0));
    std::vector<uint8_t> &b = pl.seam_bits_given[Z.stream - L.first_stream[Z.mesh]];
    const uint32_t *words = (const uint32_t *)(seam_host.data() + it.packed_off);
    for (uint32_t e = 0; e < ne; ++e) b[e] = (uint8_t)((words[e >> 5] >> (e & 31u)) & 1u);
  }
  return DSA_OK;
}
// a quantised stream the quantiser cannot take: its mesh is refused, in the host coder's words (synth::quantize,
// synth::quantize_on_grid), before anything is coded from it -- the first such attribute of the mesh answers.  On a grid a value
// that is not finite or off the grid (k_enc_grid_quantize); under own bounds a value that is not finite (k_enc_bounds), else a
// range that is not finite or so small that max_q / range is not (the bounds as they came back)
static void enc_quantiser_refusals(EncChunk &ck) {
  for (uint32_t i = 0; i < ck.n; ++i) {
    if (!ck.good(i)) continue;
    const uint32_t s0 = ck.L.first_stream[i];
    for (size_t k = 0; k < ck.plans[i].atts.size(); ++k) {
      const dsa::EncStream &S = ck.L.streams[s0 + k];
      if (S.kind != 0) continue;
      const synth::PortableAttr &a = ck.plans[i].atts[k];
      const std::string name = synth::grid_slot_name(a.att_type, a.extra_index);
      const bool finite = S.grid_nonfinite == dsa::ENC_GRID_NO_ROW;
      std::string why;
      if (!finite || (S.grid_mode != 0 && S.grid_off != dsa::ENC_GRID_NO_ROW)) why = synth::grid_row_message(name, finite ? S.grid_off : S.grid_nonfinite, finite);
      else if (S.grid_mode == 0 && !synth::quant_range_ok(S.qrange, (int)S.bits)) why = synth::quant_range_message(name, S.qrange, (int)S.bits);
      if (why.empty()) continue;
      ck.refuse(i, DSA_ERR_INVALID_ARGUMENT, why);
      for (uint32_t s = s0; s < ck.L.first_stream[i + 1]; ++s) ck.L.streams[s].overflow = 1;
      break;
    }
  }
}
// vote_attributes: a voted stream whose table k_enc_vote_count found full (EncVote::full; it cannot be at two slots a point): its
// cloud fails alone, nothing is coded from it
static void enc_vote_refusals(EncChunk &ck) {
  for (size_t k = 0; k < ck.L.votes.size(); ++k) {
    if (!ck.L.votes[k].full) continue;
    const uint32_t s = ck.L.vote_pass.stream[k], i = (uint32_t)ck.stream_mesh[s];
    if (!ck.good(i)) continue;
    char buf[160];
    snprintf(buf, sizeof(buf), "internal error: the vote table of attribute %u (vote_attributes 0x%x, %u slots) was found full", s - ck.L.first_stream[i], ck.rq.vote_attributes, ck.L.votes[k].cap);
    ck.refuse(i, DSA_ERR_DEVICE, buf);
    for (uint32_t t = ck.L.first_stream[i]; t < ck.L.first_stream[i + 1]; ++t) ck.L.streams[t].overflow = 1;
  }
}
// host phase 2 and device phase 2, shared with encode_sequential_chunk: scheme choice and rANS tables from the device statistics
// (by the host, or what k_enc_plan said), then the entropy coding and its downloads; `lap`, when given, between the two
static dsa_status enc_stage_code(dsa_context *ctx, EncLane &lane, EncChunk &ck, EncLap *lap) {
  const uint32_t ns = (uint32_t)ck.L.streams.size();
  ck.splans.resize(ns); ck.stream_mesh.assign(ns, 0);
  for (uint32_t i = 0; i < ck.n; ++i) for (uint32_t s = ck.L.first_stream[i]; s < ck.L.first_stream[i + 1]; ++s) ck.stream_mesh[s] = (int)i;
  enc_quantiser_refusals(ck);
  enc_vote_refusals(ck);
  if (ck.host_plan) ENC_STAGE(enc_host_plans(ctx, lane, ck));
  else enc_device_plan_errors(ck);
  if (lap) (*lap)("histograms + symbol plans");
  ck.rans.resize(ns); ck.bits.resize(ns); ck.flag_bits.resize(ns); ck.crease.resize(ck.L.any_crease ? 4 * (size_t)ns : 0);
  if (!ck.L.rows_of_stream.empty() || !ck.L.ord.empty()) ck.entry_rows.resize(ns);
  if (ck.L.merge) ck.row_cells.resize(ns);
  if (ck.L.split) ck.part_boxes.resize(ns);
  return ns ? enc_code_streams(ctx, lane, ck) : DSA_OK;
}
// host phase 3: the stream layout (threads over meshes; write_stream may throw like any part of the host coder)
static void enc_stage_streams(EncChunk &ck) {
  const EncLayout &L = ck.L;
  hostutil::parallel_for(ck.n, [&](uint32_t i) {
    if (!ck.good(i)) return;
    for (uint32_t s = L.first_stream[i]; s < L.first_stream[i + 1]; ++s)       // (the context lists included)
      if (L.streams[s].overflow) return ck.refuse(i, DSA_ERR_INVALID_DATA, "entropy coding failed");
    synth::ByteWriter w;
    const uint32_t s0 = L.first_stream[i];
    try {
      synth::MeshPlan &pl = ck.plans[i];
      if (pl.valence) {                                        // the six context lists: their streams follow the attributes'
        const uint32_t v0 = s0 + (uint32_t)pl.atts.size();
        pl.ctx_given = true;
        for (uint32_t k = 0; k < 6; ++k) {
          pl.ctx_count[k] = L.streams[v0 + k].nv;
          synth::ByteWriter bw;
          if (L.streams[v0 + k].nv) enc_put_coded(bw, ck.splans[v0 + k], ck.rans[v0 + k], ck.bits[v0 + k], L.streams[v0 + k].method);
          pl.ctx_coded[k].swap(bw.d);
        }
      }
      synth::write_stream(w, ck.ins[i], pl,
        [&](synth::ByteWriter &bw, size_t k) {
          const dsa::EncStream &S = L.streams[s0 + k];
          enc_write_attribute_values(bw, ck, s0 + (uint32_t)k, S.kind == 1 ? (int8_t)(S.prediction == 6 ? 6 : 0) : (int8_t)pl.atts[k].prediction);
        },
        [&](synth::ByteWriter &bw, size_t k) { enc_write_transform(bw, L.streams[s0 + k]); });
    } catch (const std::exception &e) { return ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
    ck.E->streams[i].swap(w.d);
    if (!ck.entry_rows.empty()) {                             // (a mesh that failed has none: its status answers)
      ck.E->rows[i].resize(ck.plans[i].atts.size());
      for (size_t k = 0; k < ck.E->rows[i].size(); ++k) ck.E->rows[i][k].swap(ck.entry_rows[s0 + k]);
    }
  });
}

// Meshes base .. base + count of an Edgebreaker request, a chunk of a batch of batch_n, on a lane: the stages above in their order.
static dsa_status encode_chunk(dsa_context *ctx, EncLane &lane, const EncRequest &rq, uint32_t base, uint32_t count, uint32_t batch_n, dsa_encoded **out) {
  hostutil::TurnGuard turn(lane.upload_turn, lane.upload_chunk);      // (whatever happens below, the other chunks' uploads do not wait for this one's)
  HIP_TRY(ctx, hipSetDevice(lane.device));
  EncChunk ck(rq, base, count, batch_n);
  if (!ck.E) return set_err(ctx, DSA_ERR_OUT_OF_MEMORY, "host allocation failed");
  ck.E->ctx = ctx;
  EncLap lap{&lane};
  ENC_STAGE(enc_stage_weld(ctx, lane, turn, ck));
  if (ck.rq.weld) lap("weld");
  ENC_STAGE(enc_stage_plans(ctx, ck));
  lap("host checks / plan");
  ENC_STAGE(enc_stage_repair(ctx, lane, ck));
  if (ck.rq.repair) lap("topology repair");
  enc_layout(ck);
  if (!ck.L.streams.empty()) {
    ENC_STAGE(enc_stage_uploads(ctx, lane, turn, ck));
    lap("layout + uploads queued");
    ENC_STAGE(enc_stage_connectivity(ctx, lane, turn, ck));
    ENC_STAGE(enc_stage_attributes(ctx, lane, ck));
    lap("device phases 0 + 1");
    ENC_STAGE(enc_stage_conn_results(ctx, lane, ck));
  }
  lap("connectivity results");
  ENC_STAGE(enc_stage_code(ctx, lane, ck, &lap));
  lap("device phase 2 + downloads");
  enc_stage_streams(ck);
  lap("stream layout");
  *out = ck.E.release();
  return DSA_OK;
}

// dsa_weld_batch: the weld stage alone; the weld of every mesh into the request's sink, the statuses into the chunk's result
static dsa_status weld_chunk(dsa_context *ctx, EncLane &lane, const EncRequest &rq, uint32_t base, uint32_t count, uint32_t batch_n, dsa_encoded **out) {
  hostutil::TurnGuard turn(lane.upload_turn, lane.upload_chunk);
  HIP_TRY(ctx, hipSetDevice(lane.device));
  EncChunk ck(rq, base, count, batch_n);
  if (!ck.E) return set_err(ctx, DSA_ERR_OUT_OF_MEMORY, "host allocation failed");
  ck.E->ctx = ctx;
  ENC_STAGE(enc_stage_weld(ctx, lane, turn, ck));
  for (uint32_t i = 0; i < count; ++i) if (ck.good(i)) std::swap((*rq.weld_sink)[base + i], ck.weld[i]);
  *out = ck.E.release();
  return DSA_OK;
}

#include "dsa_encode_sequential.h"

// ---- the option check of every entry point, each layer once and the outermost first.  ENC_REFUSE: the call fails with this text.
#define ENC_REFUSE(...) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, __VA_ARGS__)
#define ENC_RESERVED(o, count, name) for (int k = 0; k < (count); ++k) if ((o).reserved[k] != 0) ENC_REFUSE(name ".reserved[%d] is not zero", k)
// The prediction methods of `base` the device coder writes; any other value would put a method byte in front of data it does not
// describe.  (They do not shape a sequential stream; values dsa_encode_batch refuses are refused all the same.)
static dsa_status enc_check_base(dsa_context *ctx, const dsa_encode_options &o) {
  if (o.position_prediction != 0 && o.position_prediction != 1)
    ENC_REFUSE("position_prediction %d: the encoder writes 0 (difference) or 1 (parallelogram)", (int)o.position_prediction);
  if (o.texcoord_prediction != 0 && o.texcoord_prediction != 1 && o.texcoord_prediction != 5)
    ENC_REFUSE("texcoord_prediction %d: the encoder writes 0 (difference), 1 (parallelogram) or 5 (TexCoordsPortable)", (int)o.texcoord_prediction);
  return DSA_OK;
}
// Edgebreaker streams: the widest options, in which every narrower entry point has left what it does not have at its default.
// (The quantisation bits are checked per chunk: enc_stage_plans.)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_rows_options &w, bool null_argument) {
  const dsa_encode_corner_attributes_options &c = w.corner_attributes;
  const dsa_encode_seam_repair_options &s = c.seam_repair;
  const dsa_encode_grid_options &g = s.grid;
  const dsa_encode_repair_options &r = g.repair;
  const dsa_encode_level_options &d = r.level;
  const dsa_encode_options_ex &ex = d.ex;
  if (w.track_rows != 0 && w.track_rows != 1) ENC_REFUSE("track_rows %d: 0 (nothing kept) or 1 (the handle keeps the entry rows of every stream)", (int)w.track_rows);
  ENC_RESERVED(w, 7, "dsa_encode_rows_options");
  if (c.weld_attributes != 0 && c.weld_attributes != 1) ENC_REFUSE("weld_attributes %d: 0 (listed attributes in the vertex key) or 1 (listed attributes welded alone)", (int)c.weld_attributes);
  ENC_RESERVED(c, 7, "dsa_encode_corner_attributes_options");
  if (c.weld_attributes == 1 && g.weld_points != 1) ENC_REFUSE("weld_attributes 1 needs weld_points 1 (rows per point), weld_points is %d", (int)g.weld_points);
  if (s.corner_repair != 0 && s.corner_repair != 1) ENC_REFUSE("corner_repair %d: 0 (refused as ever) or 1 (coded over the repaired table)", (int)s.corner_repair);
  ENC_RESERVED(s, 7, "dsa_encode_seam_repair_options");
  if (s.corner_repair == 1 && r.topology != 1) ENC_REFUSE("corner_repair 1 needs topology 1 (the reference's corner table), topology is %d", (int)r.topology);
  if (g.weld_points != 0 && g.weld_points != 1) ENC_REFUSE("weld_points %d: 0 (rows per vertex) or 1 (rows per point)", (int)g.weld_points);
  ENC_RESERVED(g, 7, "dsa_encode_grid_options");
  if (r.topology != 0 && r.topology != 1) ENC_REFUSE("topology %d: 0 (strict) or 1 (the reference's corner table)", (int)r.topology);
  ENC_RESERVED(r, 7, "dsa_encode_repair_options");
  if (null_argument) ENC_REFUSE("null argument");
  if (enc_check_base(ctx, ex.base) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (ex.edgebreaker_method != 0 && ex.edgebreaker_method != 2 && ex.edgebreaker_method != -1)
    ENC_REFUSE("edgebreaker_method %d: 0 (standard), 2 (valence) or -1 (by speed and face count)", (int)ex.edgebreaker_method);
  if (ex.normal_prediction != 0 && ex.normal_prediction != 6) ENC_REFUSE("normal_prediction %d: 0 (difference) or 6 (GeometricNormal)", (int)ex.normal_prediction);
  ENC_RESERVED(ex, 6, "dsa_encode_options_ex");
  if (d.multi_parallelogram != 0 && d.multi_parallelogram != 2 && d.multi_parallelogram != 4 && d.multi_parallelogram != -1)
    ENC_REFUSE("multi_parallelogram %d: 0 (off), 2 (MultiParallelogram), 4 (ConstrainedMultiParallelogram) or -1 (by speed and vertex count)", (int)d.multi_parallelogram);
  if (d.traversal_method != 0 && d.traversal_method != 1 && d.traversal_method != 2)
    ENC_REFUSE("traversal_method %d: 0 (depth first), 1 (prediction degree for the positions' decoder) or 2 (for every decoder without interior seams)", (int)d.traversal_method);
  ENC_RESERVED(d, 6, "dsa_encode_level_options");
  return DSA_OK;
}
// sequential streams (their quantisation bits are checked here, up front)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_sequential_options &d, bool null_argument) {
  if (null_argument) ENC_REFUSE("null argument");
  if (enc_check_base(ctx, d.base) != DSA_OK || enc_check_bits(ctx, d.base) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (d.geometry != 0 && d.geometry != 1) ENC_REFUSE("geometry %d: 1 (triangular mesh) or 0 (point cloud)", (int)d.geometry);
  if (d.compress_connectivity != 0 && d.compress_connectivity != 1) ENC_REFUSE("compress_connectivity %d: 0 (raw indices) or 1 (compressed)", (int)d.compress_connectivity);
  ENC_RESERVED(d, 6, "dsa_encode_sequential_options");
  return DSA_OK;
}
// ... in an order of the encoder's choosing (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_order_options &o, bool null_argument) {
  if (o.point_order != 0 && o.point_order != 1) ENC_REFUSE("point_order %d: 0 (the caller's order) or 1 (Morton order of the quantised positions)", (int)o.point_order);
  ENC_RESERVED(o, 7, "dsa_encode_order_options");
  return enc_check_options(ctx, o.sequential, null_argument);
}
// ... with one point per cell of the position grid (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_merge_options &o, bool null_argument) {
  if (o.merge_points != 0 && o.merge_points != 1) ENC_REFUSE("merge_points %d: 0 (every point is coded) or 1 (one point per occupied cell of the position grid)", (int)o.merge_points);
  if (o.merge_points == 1 && o.order.point_order != 1) ENC_REFUSE("merge_points 1 needs point_order 1 (it was %d): the points of a cell are found side by side in the Morton order", (int)o.order.point_order);
  if (o.merge_points == 1 && o.order.sequential.geometry != 0) ENC_REFUSE("merge_points 1 needs geometry 0 (it was %d): merging the points of a mesh would collapse its faces and lose its seams", (int)o.order.sequential.geometry);
  ENC_RESERVED(o, 7, "dsa_encode_merge_options");
  return enc_check_options(ctx, o.order, null_argument);
}
// ... or the sorted order in parts of bounded size (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_split_options &o, bool null_argument) {
  if (o.part_points < 0) ENC_REFUSE("part_points %d: 0 (one stream per cloud) or the largest number of points of a part, 1 and above", (int)o.part_points);
  if (o.part_points >= 1 && o.merge.order.point_order != 1) ENC_REFUSE("part_points %d needs point_order 1 (it was %d): parts are runs of the Morton order", (int)o.part_points, (int)o.merge.order.point_order);
  if (o.part_points >= 1 && o.merge.order.sequential.geometry != 0) ENC_REFUSE("part_points %d needs geometry 0 (it was %d): a part of a mesh would need its faces cut", (int)o.part_points, (int)o.merge.order.sequential.geometry);
  if (o.part_points >= 1 && o.merge.merge_points == 1) ENC_REFUSE("part_points %d with merge_points 1: the number of kept points, and so of parts, is known only on the device (not built)", (int)o.part_points);
  ENC_RESERVED(o, 7, "dsa_encode_split_options");
  return enc_check_options(ctx, o.merge, null_argument);
}
// ... or the kept order of merge_points in parts of bounded size, sized on the device (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_cell_parts_options &o, bool null_argument) {
  const dsa_encode_merge_options &m = o.split.merge;
  if (o.part_cells < 0) ENC_REFUSE("part_cells %d: 0 (the request of dsa_encode_split_sequential_batch) or the largest number of kept points of a part, 1 and above", (int)o.part_cells);
  if (o.part_cells >= 1 && m.merge_points != 1) ENC_REFUSE("part_cells %d needs merge_points 1 (it was %d): parts of the points as they came in are part_points", (int)o.part_cells, (int)m.merge_points);
  if (o.part_cells >= 1 && m.order.point_order != 1) ENC_REFUSE("part_cells %d needs point_order 1 (it was %d): parts are runs of the Morton order", (int)o.part_cells, (int)m.order.point_order);
  if (o.part_cells >= 1 && m.order.sequential.geometry != 0) ENC_REFUSE("part_cells %d needs geometry 0 (it was %d): a part of a mesh would need its faces cut", (int)o.part_cells, (int)m.order.sequential.geometry);
  if (o.part_cells >= 1 && o.split.part_points != 0) ENC_REFUSE("part_cells %d with part_points %d: one of the two sizes the parts", (int)o.part_cells, (int)o.split.part_points);
  ENC_RESERVED(o, 7, "dsa_encode_cell_parts_options");
  return enc_check_options(ctx, o.split, null_argument);
}
// ... or that order by (level, kept), every level in parts (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_lod_options &o, bool null_argument) {
  const dsa_encode_cell_parts_options &c = o.cell_parts;
  const dsa_encode_merge_options &m = c.split.merge;
  const int bits = (int)m.order.sequential.base.position_bits;
  if (o.lod_base_bits < 0) ENC_REFUSE("lod_base_bits %d: 0 (the request of dsa_encode_cell_parts_sequential_batch) or the bits per axis of the grid of level 0, 1 .. position_bits", (int)o.lod_base_bits);
  if (o.lod_base_bits >= 1 && c.part_cells == 0) ENC_REFUSE("lod_base_bits %d needs part_cells >= 1 (it was 0): every level is cut into parts of at most part_cells points", (int)o.lod_base_bits);
  if (o.lod_base_bits >= 1 && m.merge_points != 1) ENC_REFUSE("lod_base_bits %d needs merge_points 1 (it was %d): the levels are levels of the kept points", (int)o.lod_base_bits, (int)m.merge_points);
  if (o.lod_base_bits >= 1 && m.order.point_order != 1) ENC_REFUSE("lod_base_bits %d needs point_order 1 (it was %d): the level of a point follows from its neighbour in the Morton order", (int)o.lod_base_bits, (int)m.order.point_order);
  if (o.lod_base_bits >= 1 && m.order.sequential.geometry != 0) ENC_REFUSE("lod_base_bits %d needs geometry 0 (it was %d): levels of meshes are not built", (int)o.lod_base_bits, (int)m.order.sequential.geometry);
  ENC_RESERVED(o, 7, "dsa_encode_lod_options");
  if (enc_check_options(ctx, c, null_argument) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (o.lod_base_bits > bits) ENC_REFUSE("lod_base_bits %d is above position_bits %d: level 0 cannot be finer than the quantisation grid", (int)o.lod_base_bits, bits);
  return DSA_OK;
}
// a mask over the attributes of a merged cloud's stream (`name`: mean_attributes, vote_attributes; `is`: what it asks of the points of a cell)
static dsa_status enc_check_cell_mask(dsa_context *ctx, const char *name, uint32_t mask, const dsa_encode_merge_options &m, const char *is) {
  if (mask != 0 && m.merge_points != 1) ENC_REFUSE("%s 0x%x needs merge_points 1 (it was %d): %s of a cell", name, (unsigned)mask, (int)m.merge_points, is);
  if (mask >> DSA_MAX_ATTRIBUTES) ENC_REFUSE("%s 0x%x: a bit at or above %d (DSA_MAX_ATTRIBUTES) names no attribute of a stream", name, (unsigned)mask, (int)DSA_MAX_ATTRIBUTES);
  return DSA_OK;
}
// ... with the mean of the cell in the masked attributes of the kept points (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_mean_options &o, bool null_argument) {
  if (enc_check_cell_mask(ctx, "mean_attributes", o.mean_attributes, o.lod.cell_parts.split.merge, "the mean is the mean over the points") != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  ENC_RESERVED(o, 7, "dsa_encode_mean_options");
  return enc_check_options(ctx, o.lod, null_argument);
}
// ... or with the most frequent value of the cell in the voted attributes of the kept points (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_vote_options &o, bool null_argument) {
  if (enc_check_cell_mask(ctx, "vote_attributes", o.vote_attributes, o.mean.lod.cell_parts.split.merge, "the vote is a vote of the points") != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (o.vote_attributes & o.mean.mean_attributes) ENC_REFUSE("vote_attributes 0x%x and mean_attributes 0x%x share a bit: an attribute carries the most frequent value of its cell or the mean, not both", (unsigned)o.vote_attributes, (unsigned)o.mean.mean_attributes);
  ENC_RESERVED(o, 7, "dsa_encode_vote_options");
  return enc_check_options(ctx, o.mean, null_argument);
}
// ... or with the mean normal of the cell in the normals of the kept points (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_normal_mean_options &o, bool null_argument) {
  const dsa_encode_merge_options &m = o.vote.mean.lod.cell_parts.split.merge;
  if (o.mean_normals > 1) ENC_REFUSE("mean_normals %u: 0 (the request of dsa_encode_vote_sequential_batch) or 1 (the normals of every kept point are the mean normal of its cell)", (unsigned)o.mean_normals);
  if (o.mean_normals != 0 && m.merge_points != 1) ENC_REFUSE("mean_normals %u needs merge_points 1 (it was %d): the mean normal is the mean over the points of a cell", (unsigned)o.mean_normals, (int)m.merge_points);
  ENC_RESERVED(o, 7, "dsa_encode_normal_mean_options");
  return enc_check_options(ctx, o.vote, null_argument);
}
// ... or with voxels coarser than the position grid and a choice of the point each keeps (dsa_encode_order.h)
static dsa_status enc_check_options(dsa_context *ctx, const dsa_encode_voxel_options &o, bool null_argument) {
  const dsa_encode_lod_options &l = o.normal_mean.vote.mean.lod;
  const dsa_encode_merge_options &m = l.cell_parts.split.merge;
  const int bits = (int)m.order.sequential.base.position_bits;
  if (o.voxel_bits < 0) ENC_REFUSE("voxel_bits %d: 0 (the request of dsa_encode_normal_mean_sequential_batch) or the bits per axis of the voxel grid, 1 .. position_bits", (int)o.voxel_bits);
  if (o.voxel_bits >= 1 && m.merge_points != 1) ENC_REFUSE("voxel_bits %d needs merge_points 1 (it was %d): a voxel keeps one of the points of a cell", (int)o.voxel_bits, (int)m.merge_points);
  if (o.voxel_point < 0 || o.voxel_point > 2) ENC_REFUSE("voxel_point %d: 0 (DSA_VOXEL_POINT_FIRST), 1 (DSA_VOXEL_POINT_CENTROID) or 2 (DSA_VOXEL_POINT_NEAREST)", (int)o.voxel_point);
  if (o.voxel_point != 0 && o.voxel_bits == 0) ENC_REFUSE("voxel_point %d needs voxel_bits >= 1 (it was 0): the centroid and the nearest point are those of a voxel", (int)o.voxel_point);
  ENC_RESERVED(o, 6, "dsa_encode_voxel_options");
  if (enc_check_options(ctx, o.normal_mean, null_argument) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (o.voxel_bits > bits) ENC_REFUSE("voxel_bits %d is above position_bits %d: a voxel cannot be finer than the quantisation grid", (int)o.voxel_bits, bits);
  if (o.voxel_bits >= 1 && l.lod_base_bits > o.voxel_bits) ENC_REFUSE("lod_base_bits %d is above voxel_bits %d: level 0 cannot be finer than the voxel grid", (int)l.lod_base_bits, (int)o.voxel_bits);
  return DSA_OK;
}
#undef ENC_RESERVED
#undef ENC_REFUSE

// the context's lanes, `lanes` of them at least (kept between calls)
static dsa_status enc_ensure_lanes(dsa_context *ctx, uint32_t lanes) {
  while (ctx->enc_lanes.size() < lanes) {
    std::unique_ptr<EncLane> l(new EncLane());
    l->device = ctx->device;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    HIP_TRY(ctx, hipStreamCreateWithFlags(&l->st, hipStreamNonBlocking));
    // (a priority has its own few hardware queues: the walk streams are dealt over two, so that four walks run side by side)
    HIP_TRY(ctx, hipStreamCreateWithPriority(&l->walk_st, hipStreamNonBlocking, (ctx->enc_lanes.size() & 1) ? greatest : least));
    HIP_TRY(ctx, hipEventCreateWithFlags(&l->tables_done, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&l->walk_done, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&l->seams_done, hipEventDisableTiming));
    ctx->enc_lanes.push_back(std::move(l));
  }
  return DSA_OK;
}

// A batch is coded in chunks, several of them in flight (each on a lane of its own: stream + pinned staging + device memory).  The
// device stages of a chunk are bound by latency -- the walks of k_enc_connectivity take a memory round trip per step, 0.1 - 0.2 s
// whatever the number of meshes -- so the more chunks are under way the better: the uploads of the chunks go over the link one
// after the other (a turn each: the first chunk's kernels start after its own upload, not after everybody's), the kernels of one
// run beside the walks of the others and beside the host's stream layout of those that are done.  The walks need the faces only:
// those go first (phase A of every chunk in front of any phase B, hostutil::UploadTurns), the attribute values follow while the
// walks run, on a stream of their own.  Streams of one priority share four hardware queues, on which the kernels of different
// streams wait for each other: four lanes, their walk streams at another priority.  Small batches are one chunk.
// `code_chunk(sink, lane, base, count, &part)`: codes meshes base .. base + count of the batch on the lane.
template <class ChunkFn>
static dsa_status encode_batch_chunks(dsa_context *ctx, uint32_t n, ChunkFn &&code_chunk, dsa_encoded **out, int rows_kind = dsa_encoded::ROWS_NONE, bool merged = false, bool split = false) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t max_lanes = [&]() { const char *e = getenv("DSA_ENC_LANES"); const int v = e ? atoi(e) : 0; return (uint32_t)(v >= 1 && v <= 16 ? v : 4); }();
  const uint32_t chunk_max = [&]() { const char *e = getenv("DSA_ENC_CHUNK"); const int v = e ? atoi(e) : 0; return (uint32_t)(v >= 1 ? v : 0); }();
  // as many chunks as lanes, of 512 to 1024 meshes (a chunk's device memory: about 9 MB per 64k-triangle mesh)
  const uint32_t chunk = chunk_max ? std::min(std::max(n, 1u), chunk_max) : (n <= 512 ? std::max(n, 1u) : std::min(1024u, std::max(512u, (n + max_lanes - 1) / max_lanes)));
  const uint32_t chunks = (n + chunk - 1) / chunk, lanes = std::max(1u, std::min(chunks, max_lanes));
  // (Tapering the last chunks -- the batch is over when its last chunk is, and what shrinks with a chunk is everything around its
  // walks -- was measured twice and did not beat equal chunks for 4096 meshes (470 - 490 against 410 ms while the stream layout was
  // slow, 376 - 426 against 370 - 383 since); it helps 8192 meshes (605 against 680 ms) and costs 2048 (296 against 235).)
  std::vector<uint32_t> bounds(chunks + 1, 0);
  for (uint32_t c = 0; c <= chunks; ++c) bounds[c] = (uint32_t)std::min<uint64_t>(n, (uint64_t)c * chunk);
  ENC_STAGE(enc_ensure_lanes(ctx, lanes));
  hostutil::UploadTurns upload_turn(chunks);
  for (uint32_t l = 0; l < lanes; ++l) ctx->enc_lanes[l]->upload_turn = &upload_turn;
  struct Unhook { dsa_context *c; ~Unhook() { for (auto &l : c->enc_lanes) l->upload_turn = nullptr; } } unhook{ctx};
  std::unique_ptr<dsa_encoded> E(new dsa_encoded());
  E->ctx = ctx;
  E->streams.resize(n); E->status.assign(n, DSA_OK); E->messages.resize(n);
  E->keep_rows(rows_kind, n);
  if (merged) E->keep_cells(n);
  if (split) E->keep_parts(n);
  std::atomic<uint32_t> next{0};
  std::atomic<int> failed{DSA_OK};
  std::vector<std::string> errs(lanes);
  auto work = [&](uint32_t l) noexcept {
    try {
      dsa_context sink;                              // receives this lane's error text (set_err writes ctx->err: not from several threads)
      sink.device = ctx->device;
      if (hipSetDevice(ctx->device) != hipSuccess) { int ok = DSA_OK; failed.compare_exchange_strong(ok, DSA_ERR_DEVICE); return; }
      for (;;) {
        const uint32_t c = next.fetch_add(1, std::memory_order_relaxed);
        if (c >= chunks) break;
        if (failed.load(std::memory_order_relaxed) != DSA_OK) { upload_turn.finish_a(c, false); break; }     // (a chunk given up is not one the others' uploads wait for)
        const uint32_t base = bounds[c], cnt = bounds[c + 1] - base;
        if (cnt == 0) { upload_turn.finish_a(c, false); continue; }
        ctx->enc_lanes[l]->upload_chunk = c;
        dsa_encoded *part = nullptr;
        const auto t_chunk = std::chrono::steady_clock::now();
        const dsa_status st = code_chunk(&sink, *ctx->enc_lanes[l], base, cnt, &part);
        if (getenv("DSA_ENC_TIMING")) fprintf(stderr, "[dsa_encode_batch] chunk %u (%u meshes) returned after %8.2f ms\n", c, cnt, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_chunk).count());
        if (st != DSA_OK) { errs[l] = sink.err; int ok = DSA_OK; failed.compare_exchange_strong(ok, st); break; }
        std::unique_ptr<dsa_encoded> owner(part);
        for (uint32_t i = 0; i < cnt; ++i) E->take(base + i, *part, i);
      }
    } catch (const std::bad_alloc &) { int ok = DSA_OK; failed.compare_exchange_strong(ok, DSA_ERR_OUT_OF_MEMORY); }
    catch (...) { int ok = DSA_OK; failed.compare_exchange_strong(ok, DSA_ERR_DEVICE); }
  };
  {
    struct Joiner { std::vector<std::thread> t; ~Joiner() { for (auto &x : t) if (x.joinable()) x.join(); } } joiner;
    try { joiner.t.reserve(lanes); for (uint32_t l = 1; l < lanes; ++l) joiner.t.emplace_back(work, l); } catch (...) {}
    work(0);
  }
  if (failed.load() != DSA_OK) {
    for (const std::string &e : errs) if (!e.empty()) return set_err(ctx, (dsa_status)failed.load(), "%s", e.c_str());
    return set_err(ctx, (dsa_status)failed.load(), "encoding failed");
  }
  if (getenv("DSA_ENC_TIMING")) fprintf(stderr, "[dsa_encode_batch] batch of %u done\n", n);
  if (split) E->flatten_parts();                   // from an entry per input to an entry per stream
  *out = E.release();
  return DSA_OK;
}


// ---- shared grids (mode 2 of dsa_quantization_grid; dsa_encode_grid.h), once per request and in front of its chunks: a group may
// span chunks and both passes of a repair request, and its grid must depend on the inputs alone.  Every (mesh, slot) of mode 2
// whose attribute is there and quantised is an item; the items of one group number, slot and component count lie side by side
// and are one group.  Their values go up through the staged upload of lane 0 in pieces of at most 256 MiB (they travel again
// with the chunk that codes them: nothing of a chunk's arena exists yet), k_enc_grid_bounds takes every piece, k_enc_grid_fold
// all groups at the end; the grids come back and every member's slot becomes mode 1 with its group's grid.
static dsa_status enc_stage_grids(dsa_context *ctx, const EncRequest &rq, std::vector<EncMeshGrids> &grids) {
  struct Member { uint32_t mesh, slot, nc, rows; const void *src; };
  std::vector<Member> members;
  for (uint32_t i = 0; i < rq.n; ++i) {
    EncMeshGrids &g = grids[i];
    if (g.error) continue;
    const dsa_mesh_attr_input &am = rq.attr(i);
    const dsa_mesh_input &m = am.mesh.mesh;
    auto shared = [](const synth::Grid &x) { return x.mode == 2 && x.reserved[0] == 0 && x.reserved[1] == 0; };
    auto take = [&](uint32_t slot, uint32_t nc, uint32_t rows, const void *src) {
      if (!src || rows == 0) return;                          // (the mesh is refused for what is missing)
      if (rows > (1u << 28)) { g.error = "mesh too large for a shared grid"; return; }
      members.push_back({i, slot, nc, rows, src});
    };
    if (shared(g.slot[0])) take(0, 3, m.num_vertices, m.positions);
    if (shared(g.slot[1]) && m.texcoords) take(1, 2, (am.mesh.texcoord_corners && !rq.weld && !rq.sequential) ? am.mesh.num_texcoords : m.num_vertices, m.texcoords);
    for (uint32_t k = 0; k < am.num_attributes && k < synth::kMaxAttributes && am.attributes; ++k) {
      const dsa_attribute_input &x = am.attributes[k];
      // (an attribute given per corner: over the rows its ids index, like the texture coordinates above)
      const dsa_attribute_corners *ac = (rq.att_corners && !rq.weld && !rq.sequential && rq.att_corners[i].attributes) ? &rq.att_corners[i].attributes[k] : nullptr;
      if (shared(g.slot[2 + k]) && x.data_type == 9 && x.num_components >= 1 && x.num_components <= 4) take(2 + k, x.num_components, (ac && ac->corners) ? ac->num_rows : m.num_vertices, x.values);
    }
  }
  if (members.empty()) return DSA_OK;
  std::stable_sort(members.begin(), members.end(), [&](const Member &a, const Member &b) {
    const uint32_t ga = grids[a.mesh].group, gb = grids[b.mesh].group;
    return ga != gb ? ga < gb : (a.slot != b.slot ? a.slot < b.slot : a.nc < b.nc);
  });
  const uint32_t ni = (uint32_t)members.size();
  std::vector<dsa::EncGridItem> items(ni);
  std::vector<dsa::EncGridGroup> groups;
  for (uint32_t k = 0; k < ni; ++k) {
    const Member &b = members[k];
    dsa::EncGridItem &I = items[k];
    memset(&I, 0, sizeof(I));
    I.rows = b.rows; I.nc = b.nc;
    for (int c = 0; c < 4; ++c) I.mn[c] = 0xFFFFFFFFu;
    const bool opens = k == 0 || grids[members[k - 1].mesh].group != grids[b.mesh].group || members[k - 1].slot != b.slot || members[k - 1].nc != b.nc;
    if (opens) { dsa::EncGridGroup G; memset(&G, 0, sizeof(G)); G.first = k; G.nc = b.nc; groups.push_back(G); }
    ++groups.back().count;
  }
  const uint32_t ng = (uint32_t)groups.size();
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ENC_STAGE(enc_ensure_lanes(ctx, 1));
  EncLane &lane = *ctx->enc_lanes[0];
  hipStream_t st = lane.st;
  ENC_TRY(lane.items.ensure(sizeof(dsa::EncGridItem) * ni));
  ENC_TRY(lane.packed.ensure(sizeof(dsa::EncGridGroup) * ng));
  dsa::EncGridItem *d_items = (dsa::EncGridItem *)lane.items.p;
  dsa::EncGridGroup *d_groups = (dsa::EncGridGroup *)lane.packed.p;
  const uint64_t piece_cap = 256ull << 20;
  const uint32_t piece_items = 32768;
  for (uint32_t k0 = 0; k0 < ni;) {
    EncArena A;
    std::vector<EncUpload> ups;
    uint32_t k1 = k0, most = 1;
    while (k1 < ni && k1 - k0 < piece_items && (k1 == k0 || A.cur < piece_cap)) {
      const Member &b = members[k1];
      items[k1].src = A.put(ups, b.src, 4ull * b.rows * b.nc, false);
      most = std::max(most, b.rows);
      ++k1;
    }
    ENC_TRY(lane.arena.ensure(A.cur ? A.cur : 256));
    ENC_TRY(enc_upload(lane, (uint8_t *)lane.arena.p, st, ups));
    ENC_TRY(hipMemcpyAsync(d_items + k0, items.data() + k0, sizeof(dsa::EncGridItem) * (k1 - k0), hipMemcpyHostToDevice, st));
    const uint32_t gx = std::max(1u, std::min(64u, (most + 2047u) / 2048u));
    hipLaunchKernelGGL(dsa::k_enc_grid_bounds, dim3(gx, k1 - k0), dim3(256), 0, st, (const uint8_t *)lane.arena.p, d_items + k0, k1 - k0);
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipStreamSynchronize(st));                       // (items and the arena are the next piece's)
    k0 = k1;
  }
  ENC_TRY(hipMemcpyAsync(d_groups, groups.data(), sizeof(dsa::EncGridGroup) * ng, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dsa::k_enc_grid_fold, dim3((ng + WAVE - 1) / WAVE), dim3(WAVE), 0, st, (const dsa::EncGridItem *)d_items, d_groups, ng);
  ENC_TRY(hipGetLastError());
  ENC_TRY(hipMemcpyAsync(groups.data(), d_groups, sizeof(dsa::EncGridGroup) * ng, hipMemcpyDeviceToHost, st));
  ENC_TRY(hipStreamSynchronize(st));
  for (const dsa::EncGridGroup &G : groups)
    for (uint32_t k = G.first; k < G.first + G.count; ++k) {
      synth::Grid &x = grids[members[k].mesh].slot[members[k].slot];
      memcpy(x.origin, G.origin, sizeof(x.origin));
      x.range = G.range; x.mode = 1;
    }
  return DSA_OK;
}

// A checked request through its chunks.  batch_n: the size of the batch the request belongs to (what chooses between host and
// device connectivity); 0: the request's own
static dsa_status encode_request(dsa_context *ctx, const EncRequest &rq, dsa_encoded **out, uint32_t batch_n = 0) {
  if (batch_n == 0) batch_n = rq.n;
  return encode_batch_chunks(ctx, rq.n, [&](dsa_context *sink, EncLane &lane, uint32_t base, uint32_t cnt, dsa_encoded **part) {
    if (rq.weld_sink) return weld_chunk(sink, lane, rq, base, cnt, batch_n, part);
    return rq.sequential ? encode_sequential_chunk(sink, lane, rq, base, cnt, rq.n, part) : encode_chunk(sink, lane, rq, base, cnt, batch_n, part);
  }, out, rq.rows_kind(), rq.merged(), rq.split());
}
// dsa_encode_repair_batch, topology = 1: the batch as dsa_encode_level_batch codes it; then the meshes refused for their topology
// once more as a request of their own, on the repaired corner table (EncRequest::repair), their results into the first's places.
// Clean meshes take the kernels they always took and nothing else.
static bool enc_topology_refusal(const std::string &why) {
  for (uint32_t s : {(uint32_t)dsa::ENC_DEGENERATE, (uint32_t)dsa::ENC_NONMANIFOLD_EDGE, (uint32_t)dsa::ENC_RING, (uint32_t)dsa::ENC_NONMANIFOLD_VERTEX, (uint32_t)dsa::ENC_ISOLATED})
    if (why == dsa::enc_conn_message(s)) return true;
  return false;
}
static dsa_status encode_repair_request(dsa_context *ctx, const EncRequest &request, dsa_encoded **out) {
  EncRequest rq = request;
  rq.repair_scan = true;
  const dsa_status st = encode_request(ctx, rq, out);
  if (st != DSA_OK || rq.n == 0) return st;
  std::unique_ptr<dsa_encoded> E(*out);
  *out = nullptr;
  std::vector<uint32_t> again;
  std::vector<dsa_mesh_attr_input> sub;
  std::vector<EncMeshGrids> sub_grids;
  std::vector<dsa_mesh_attribute_corners> sub_corners;
  for (uint32_t i = 0; i < rq.n; ++i) {
    if (E->status[i] != DSA_ERR_INVALID_DATA) continue;
    const dsa_mesh_input &m = rq.mesh(i);
    if (m.positions && m.num_vertices >= 3 && m.num_faces == 0 && E->messages[i] == "mesh needs positions and faces") { E->messages[i] = "all triangles are degenerate"; continue; }
    if (enc_topology_refusal(E->messages[i])) { again.push_back(i); sub.push_back(rq.attr(i)); if (rq.grids) sub_grids.push_back(rq.grids[i]); if (rq.att_corners) sub_corners.push_back(rq.att_corners[i]); }
  }
  if (!again.empty()) {
    EncRequest r2 = rq;
    r2.repair_scan = false; r2.repair = true; r2.n = (uint32_t)again.size(); r2.meshes = sub.data(); r2.grids = rq.grids ? sub_grids.data() : nullptr; r2.att_corners = rq.att_corners ? sub_corners.data() : nullptr;
    dsa_encoded *second = nullptr;
    const dsa_status s2 = encode_request(ctx, r2, &second, rq.n);
    if (s2 != DSA_OK) return s2;
    std::unique_ptr<dsa_encoded> E2(second);
    for (uint32_t k = 0; k < r2.n; ++k) E->take(again[k], *E2, k);
  }
  *out = E.release();
  return DSA_OK;
}

// ---- Every entry point: the widest options of its kind at their defaults, the layer the caller passed copied in, the meshes in
// the widest form, and one way on under DSA_GUARD (host vectors and threads inside: nothing may unwind into the caller): the
// option check, the caller's grids copied and the shared ones resolved once for the whole request (enc_stage_grids;
// dsa_encode_grid.h), then the request through its chunks -- with topology 1 through both passes of encode_repair_request.
// Each wider call with its added fields at their defaults is the very request of the narrower one.
static dsa_status encode_checked(dsa_context *ctx, EncRequest &rq, const dsa_mesh_grids *grids, bool repair, dsa_encoded **out) {
  std::vector<EncMeshGrids> taken;
  if (grids && rq.n) {
    taken.resize(rq.n);
    bool any = false;
    for (uint32_t i = 0; i < rq.n; ++i) {
      taken[i] = enc_take_grids(grids[i], rq.attr(i).num_attributes);
      any = any || taken[i].error != nullptr;
      for (const synth::Grid &g : taken[i].slot) any = any || g.mode != 0 || g.reserved[0] != 0 || g.reserved[1] != 0;
    }
    if (any) {                                               // (else it is the very request of the call without grids)
      ENC_STAGE(enc_stage_grids(ctx, rq, taken));
      rq.grids = taken.data();
    }
  }
  return repair ? encode_repair_request(ctx, rq, out) : encode_request(ctx, rq, out);
}
static dsa_status encode_edgebreaker(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_rows_options &w,
                                     dsa_encoded **out, bool drop_generic_outside_1_4 = false, const dsa_mesh_attribute_corners *corners = nullptr) {
  if (enc_check_options(ctx, w, !ctx || !out || (n && !meshes)) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  const dsa_encode_corner_attributes_options &c = w.corner_attributes;
  const dsa_encode_seam_repair_options &o = c.seam_repair;
  EncRequest rq;
  rq.n = n; rq.meshes = meshes; rq.drop_generic_outside_1_4 = drop_generic_outside_1_4;
  rq.level = o.grid.repair.level;
  rq.weld = o.grid.weld_points == 1; rq.corner_repair = o.corner_repair == 1;
  rq.att_corners = n ? corners : nullptr; rq.weld_attributes = c.weld_attributes == 1;
  rq.track_rows = w.track_rows == 1;
  return encode_checked(ctx, rq, grids, o.grid.repair.topology == 1, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_voxel_options &vx, dsa_encoded **out) {
  if (enc_check_options(ctx, vx, !ctx || !out || (n && !meshes)) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  const dsa_encode_normal_mean_options &nm = vx.normal_mean;
  const dsa_encode_vote_options &v = nm.vote;
  const dsa_encode_mean_options &a = v.mean;
  const dsa_encode_lod_options &l = a.lod;
  const dsa_encode_cell_parts_options &c = l.cell_parts;
  const dsa_encode_split_options &s = c.split;
  const dsa_encode_merge_options &m = s.merge;
  const dsa_encode_order_options &o = m.order;
  EncRequest rq;
  rq.n = n; rq.meshes = meshes; rq.sequential = true;
  rq.seq = o.sequential; rq.point_order = o.point_order == 1; rq.merge_points = m.merge_points == 1; rq.part_points = (uint32_t)s.part_points; rq.part_cells = (uint32_t)c.part_cells; rq.lod_base_bits = (uint32_t)l.lod_base_bits;
  rq.mean_attributes = a.mean_attributes; rq.vote_attributes = v.vote_attributes; rq.mean_normals = nm.mean_normals == 1;
  rq.voxel_bits = (uint32_t)vx.voxel_bits; rq.voxel_point = (uint32_t)vx.voxel_point;
  const dsa_status st = encode_checked(ctx, rq, grids, false, out);
  if (st == DSA_OK && rq.lod()) (*out)->lod_bits = rq.lod_base_bits;
  return st;
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_normal_mean_options &nm, dsa_encoded **out) {
  dsa_encode_voxel_options vx;
  dsa_encode_default_voxel_options(&vx);
  vx.normal_mean = nm;
  return encode_sequential(ctx, n, meshes, grids, vx, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_vote_options &v, dsa_encoded **out) {
  dsa_encode_normal_mean_options nm;
  dsa_encode_default_normal_mean_options(&nm);
  nm.vote = v;
  return encode_sequential(ctx, n, meshes, grids, nm, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_mean_options &a, dsa_encoded **out) {
  dsa_encode_vote_options v;
  dsa_encode_default_vote_options(&v);
  v.mean = a;
  return encode_sequential(ctx, n, meshes, grids, v, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_lod_options &l, dsa_encoded **out) {
  dsa_encode_mean_options a;
  dsa_encode_default_mean_options(&a);
  a.lod = l;
  return encode_sequential(ctx, n, meshes, grids, a, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_cell_parts_options &c, dsa_encoded **out) {
  dsa_encode_lod_options l;
  dsa_encode_default_lod_options(&l);
  l.cell_parts = c;
  return encode_sequential(ctx, n, meshes, grids, l, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_split_options &s, dsa_encoded **out) {
  dsa_encode_cell_parts_options c;
  dsa_encode_default_cell_parts_options(&c);
  c.split = s;
  return encode_sequential(ctx, n, meshes, grids, c, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_merge_options &m, dsa_encoded **out) {
  dsa_encode_split_options s;
  dsa_encode_default_split_options(&s);
  s.merge = m;
  return encode_sequential(ctx, n, meshes, grids, s, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_order_options &o, dsa_encoded **out) {
  dsa_encode_merge_options m;
  dsa_encode_default_merge_options(&m);
  m.order = o;
  return encode_sequential(ctx, n, meshes, grids, m, out);
}
static dsa_status encode_sequential(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  dsa_encode_order_options o;
  dsa_encode_default_order_options(&o);
  if (options) o.sequential = *options;
  return encode_sequential(ctx, n, meshes, grids, o, out);
}
// the array of a narrower entry point widened, owned by the call
template <class Mesh>
static dsa_status encode_edgebreaker_narrow(dsa_context *ctx, uint32_t n, const Mesh *meshes, const dsa_encode_rows_options &o, dsa_encoded **out, bool drop_generic_outside_1_4 = false) {
  const std::vector<dsa_mesh_attr_input> wide = enc_widen(meshes, n);
  return encode_edgebreaker(ctx, n, wide.empty() ? nullptr : wide.data(), nullptr, o, out, drop_generic_outside_1_4);
}
static dsa_encode_rows_options enc_default_options() { dsa_encode_rows_options o; dsa_encode_default_rows_options(&o); return o; }

extern "C" {

void dsa_encode_default_options(dsa_encode_options *o) {
  if (!o) return;
  synth::Options d;
  o->position_bits = d.pos_bits; o->texcoord_bits = d.uv_bits; o->normal_bits = d.normal_bits;
  o->single_connectivity = d.single_connectivity; o->symbol_scheme = d.force_scheme; o->compression_level = d.compression_level;
  o->position_prediction = d.pos_prediction; o->texcoord_prediction = d.uv_prediction;
}
void dsa_encode_default_options_ex(dsa_encode_options_ex *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_options(&o->base);
}
void dsa_encode_default_level_options(dsa_encode_level_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_options_ex(&o->ex);
}
void dsa_encode_sequential_default_options(dsa_encode_sequential_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_options(&o->base);
  o->geometry = 1;
  o->compress_connectivity = 0;
}
void dsa_encode_default_order_options(dsa_encode_order_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_sequential_default_options(&o->sequential);
}
void dsa_encode_default_merge_options(dsa_encode_merge_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_order_options(&o->order);
}
void dsa_encode_default_split_options(dsa_encode_split_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_merge_options(&o->merge);
}
void dsa_encode_default_cell_parts_options(dsa_encode_cell_parts_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_split_options(&o->split);
}
void dsa_encode_default_lod_options(dsa_encode_lod_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_cell_parts_options(&o->cell_parts);
}
void dsa_encode_default_mean_options(dsa_encode_mean_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_lod_options(&o->lod);
}
void dsa_encode_default_vote_options(dsa_encode_vote_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_mean_options(&o->mean);
}
void dsa_encode_default_normal_mean_options(dsa_encode_normal_mean_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_vote_options(&o->vote);
}
void dsa_encode_default_voxel_options(dsa_encode_voxel_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_normal_mean_options(&o->normal_mean);
}
void dsa_encode_default_repair_options(dsa_encode_repair_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_level_options(&o->level);
}
void dsa_encode_default_grid_options(dsa_encode_grid_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_repair_options(&o->repair);
}
void dsa_encode_default_seam_repair_options(dsa_encode_seam_repair_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_grid_options(&o->grid);
}
void dsa_encode_default_corner_attributes_options(dsa_encode_corner_attributes_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_seam_repair_options(&o->seam_repair);
}
void dsa_encode_default_rows_options(dsa_encode_rows_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_corner_attributes_options(&o->corner_attributes);
}

dsa_status dsa_encode_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes, const dsa_encode_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair.level.ex.base = *options;
  DSA_GUARD(ctx, encode_edgebreaker_narrow(ctx, n, meshes, o, out, true));      // (EncRequest::drop_generic_outside_1_4: this entry alone)
}
dsa_status dsa_encode_batch_corners(dsa_context *ctx, uint32_t n, const dsa_mesh_corner_input *meshes, const dsa_encode_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair.level.ex.base = *options;
  DSA_GUARD(ctx, encode_edgebreaker_narrow(ctx, n, meshes, o, out));
}
dsa_status dsa_encode_batch_ex(dsa_context *ctx, uint32_t n, const dsa_mesh_corner_input *meshes, const dsa_encode_options_ex *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair.level.ex = *options;
  DSA_GUARD(ctx, encode_edgebreaker_narrow(ctx, n, meshes, o, out));
}
dsa_status dsa_encode_attributes_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_options_ex *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair.level.ex = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, nullptr, o, out));
}
// The levels above the default: MultiParallelogram / ConstrainedMultiParallelogram in place of Parallelogram, prediction-degree
// attribute order (dsa_encode_multi.h).
dsa_status dsa_encode_level_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_level_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair.level = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, nullptr, o, out));
}
// ... that also takes meshes with degenerate faces, non-manifold edges and vertices and isolated vertices (topology = 1: the
// reference's corner table, dsa_encode_repair.h).
dsa_status dsa_encode_repair_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_repair_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, nullptr, o, out));
}
// dsa_encode_repair_batch for meshes given as one row per point: every chunk welds its meshes first (enc_stage_weld), the welded
// meshes are coded as that call codes them.  With topology = 1 the meshes refused for their topology are welded again in the
// second pass: they are the few, and the weld is cheap beside keeping every chunk's buffers alive.
dsa_status dsa_encode_points_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_repair_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid.repair = *options;
  o.corner_attributes.seam_repair.grid.weld_points = 1;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, nullptr, o, out));
}
// ... with a quantisation grid per float attribute, given by the caller or shared within a group (dsa_encode_grid.h).
dsa_status dsa_encode_grid_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_grid_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair.grid = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, grids, o, out));
}
// ... with attributes given per corner coded over a repaired table (EncRequest::corner_repair; the second pass of
// encode_repair_request, dsa_encode_repair.h: k_enc_repair_face_scan, k_enc_repair_ids).
dsa_status dsa_encode_seam_repair_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_seam_repair_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes.seam_repair = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, grids, o, out));
}
// ... with row ids per corner for the attributes of the list, given by the caller (EncRequest::att_corners) or found by the weld
// with every listed attribute a key set of its own (EncRequest::weld_attributes; dsa_encode_weld.h with L > 0).
dsa_status dsa_encode_corner_attributes_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                              const dsa_mesh_attribute_corners *corners, const dsa_encode_corner_attributes_options *options, dsa_encoded **out) {
  dsa_encode_rows_options o = enc_default_options();
  if (options) o.corner_attributes = *options;
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, grids, o, out, false, corners));
}
// ... whose handle also keeps, with track_rows = 1, the row of the caller's value arrays every entry of every stream carries
// (EncRequest::track_rows; dsa_encode_rows.h: k_enc_entry_rows behind the attribute kernels of every chunk).
dsa_status dsa_encode_rows_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids,
                                 const dsa_mesh_attribute_corners *corners, const dsa_encode_rows_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, encode_edgebreaker(ctx, n, meshes, grids, options ? *options : enc_default_options(), out, false, corners));
}
dsa_status dsa_encode_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { const std::vector<dsa_mesh_attr_input> wide = enc_widen(meshes, n); return encode_sequential(ctx, n, wide.empty() ? nullptr : wide.data(), nullptr, options, out); }());
}
dsa_status dsa_encode_attributes_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, encode_sequential(ctx, n, meshes, nullptr, options, out));
}
dsa_status dsa_encode_grid_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, encode_sequential(ctx, n, meshes, grids, options, out));
}
// ... with the points of every stream in an order of the encoder's choosing (point_order = 1: Morton order of the quantised
// positions, found on the device -- dsa_encode_order.h); point_order = 0 is the very request of the call above.
dsa_status dsa_encode_ordered_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_order_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_order_options o; dsa_encode_default_order_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... and of point clouds one point per occupied cell of the position grid (merge_points = 1: the heads of the runs of equal keys
// behind the sort, compacted on the device -- dsa_encode_order.h); merge_points = 0 is the very request of the call above.
dsa_status dsa_encode_merged_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_merge_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_merge_options o; dsa_encode_default_merge_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or the sorted order of every point cloud in parts of at most part_points points, a stream and a box each (part_points >= 1:
// dsa_encode_order.h); part_points = 0 is the very request of the call above.
dsa_status dsa_encode_split_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_split_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_split_options o; dsa_encode_default_split_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with merge_points = 1, the KEPT order in parts of at most part_cells points, sized on the device (part_cells >= 1:
// k_enc_part_cells, dsa_encode_order.h); part_cells = 0 is the very request of the call above.
dsa_status dsa_encode_cell_parts_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_cell_parts_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_cell_parts_options o; dsa_encode_default_cell_parts_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with lod_base_bits >= 1, that order by (level, kept) and every level in parts (k_enc_lod_*, dsa_encode_order.h);
// lod_base_bits = 0 is the very request of the call above.
dsa_status dsa_encode_lod_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_lod_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_lod_options o; dsa_encode_default_lod_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with mean_attributes != 0, the mean of the cell in the masked attributes of every kept point (k_enc_mean_*, dsa_encode_order.h);
// mean_attributes = 0 is the very request of the call above.
dsa_status dsa_encode_mean_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_mean_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_mean_options o; dsa_encode_default_mean_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with vote_attributes != 0, the most frequent value of the cell in the voted attributes of every kept point (k_enc_vote_*,
// dsa_encode_order.h); vote_attributes = 0 is the very request of the call above, which arrives here.
dsa_status dsa_encode_vote_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_vote_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_vote_options o; dsa_encode_default_vote_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with mean_normals = 1, the mean normal of the cell in the normals of every kept point (k_enc_normal_*, dsa_encode_order.h);
// mean_normals = 0 is the very request of the call above, which arrives here.
dsa_status dsa_encode_normal_mean_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_normal_mean_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_normal_mean_options o; dsa_encode_default_normal_mean_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}
// ... or, with voxel_bits >= 1, one point per cell of a grid coarser than the position grid: its first point, its centroid or the point
// nearest its centre (a shift in the head predicate, the means pass, k_enc_voxel_*; dsa_encode_order.h); voxel_bits = 0 is the very
// request of the call above, which arrives here.
dsa_status dsa_encode_voxel_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_mesh_grids *grids, const dsa_encode_voxel_options *options, dsa_encoded **out) {
  DSA_GUARD(ctx, [&] { dsa_encode_voxel_options o; dsa_encode_default_voxel_options(&o); if (options) o = *options; return encode_sequential(ctx, n, meshes, grids, o, out); }());
}

struct dsa_welded {
  dsa_context *ctx = nullptr;
  std::vector<synth::Welded> meshes;
  std::vector<int32_t> status;
  std::vector<std::string> messages;
};
static dsa_status weld_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, dsa_welded **out) {
  if (!ctx || !out || (n && !meshes)) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  std::unique_ptr<dsa_welded> W(new dsa_welded());
  W->meshes.resize(n);
  EncRequest rq;
  rq.n = n; rq.meshes = meshes;
  dsa_encode_default_level_options(&rq.level);
  rq.weld = true;
  rq.weld_sink = &W->meshes;
  dsa_encoded *E = nullptr;
  const dsa_status st = encode_request(ctx, rq, &E);
  if (st != DSA_OK) return st;
  std::unique_ptr<dsa_encoded> owner(E);
  W->ctx = ctx;
  W->status.swap(E->status); W->messages.swap(E->messages);
  *out = W.release();
  return DSA_OK;
}
dsa_status dsa_weld_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, dsa_welded **out) {
  DSA_GUARD(ctx, weld_batch(ctx, n, meshes, out));
}
uint32_t dsa_welded_size(const dsa_welded *w) { return w ? (uint32_t)w->meshes.size() : 0; }
dsa_status dsa_welded_mesh(const dsa_welded *w, uint32_t mesh, dsa_welded_info *info) {
  if (!w || !info || mesh >= w->meshes.size()) return DSA_ERR_INVALID_ARGUMENT;
  memset(info, 0, sizeof(*info));
  info->status = w->status[mesh];
  if (w->status[mesh] != DSA_OK) return set_err(w->ctx, (dsa_status)w->status[mesh], "mesh %u: %s", mesh, w->messages[mesh].c_str());
  const synth::Welded &m = w->meshes[mesh];
  info->num_points = m.P; info->num_vertices = m.vertex.count; info->num_normals = m.normal.count; info->num_texcoords = m.texcoord.count;
  info->normals_per_vertex = m.normals_per_vertex ? 1 : 0; info->texcoords_per_vertex = m.texcoords_per_vertex ? 1 : 0;
  auto data = [](const std::vector<uint32_t> &v) { return v.empty() ? nullptr : v.data(); };
  info->vertex_of_point = data(m.vertex.of_point); info->vertex_point = data(m.vertex.point);
  info->normal_of_point = data(m.normal.of_point); info->normal_point = data(m.normal.point);
  info->texcoord_of_point = data(m.texcoord.of_point); info->texcoord_point = data(m.texcoord.point);
  return DSA_OK;
}
void dsa_welded_free(dsa_welded *w) { delete w; }


uint32_t dsa_encoded_size(const dsa_encoded *e) { return e ? (uint32_t)e->streams.size() : 0; }

dsa_status dsa_encoded_stream(const dsa_encoded *e, uint32_t mesh, const uint8_t **bytes, size_t *length) {
  if (!e || mesh >= e->streams.size() || !bytes || !length) return DSA_ERR_INVALID_ARGUMENT;
  if (e->status[mesh] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[mesh], "mesh %u: %s", mesh, e->messages[mesh].c_str());
  *bytes = e->streams[mesh].data();
  *length = e->streams[mesh].size();
  return DSA_OK;
}

// How many attributes stream `mesh` has entry rows for (what bounds `attribute` below).
dsa_status dsa_encoded_attributes(const dsa_encoded *e, uint32_t mesh, uint32_t *count) {
  if (!e || mesh >= e->streams.size() || !count) return DSA_ERR_INVALID_ARGUMENT;
  *count = 0;
  if (e->status[mesh] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[mesh], "mesh %u: %s", mesh, e->messages[mesh].c_str());
  if (e->rows_kind == dsa_encoded::ROWS_NONE) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "the entry rows of this handle were not kept: encode with dsa_encode_rows_batch and track_rows = 1");
  *count = e->row_attributes(mesh);
  return DSA_OK;
}
// The entry of the cell of every input row of stream `mesh` (merge_points = 1): row_entries[r] = j with key(kept[j]) = key(r).
dsa_status dsa_encoded_row_entries(const dsa_encoded *e, uint32_t mesh, uint32_t *dst, size_t capacity, uint32_t *count) {
  if (!e || mesh >= e->streams.size() || !count) return DSA_ERR_INVALID_ARGUMENT;
  *count = 0;
  if (e->status[mesh] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[mesh], "mesh %u: %s", mesh, e->messages[mesh].c_str());
  if (!e->merged) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "the row entries of this handle were not kept: encode with dsa_encode_merged_sequential_batch and merge_points = 1");
  if (!e->part_info.empty() && e->part_first[e->part_info[mesh].input] != mesh)      // (part_cells: row_entries are the cloud's, kept with its first part)
    return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "stream %u is part %u of input %u: the row entries of a cloud in parts are kept once, ask its first stream, %u", mesh, e->part_info[mesh].part,
                   e->part_info[mesh].input, e->part_first[e->part_info[mesh].input]);
  const std::vector<uint32_t> &cells = e->cells[mesh];
  *count = (uint32_t)cells.size();
  if (!dst) return DSA_OK;
  if (capacity < cells.size()) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u: %u row entries, room for %llu", mesh, (uint32_t)cells.size(), (unsigned long long)capacity);
  if (!cells.empty()) memcpy(dst, cells.data(), 4ull * cells.size());
  return DSA_OK;
}
// The stream slots of input `input`: of a split handle what flatten_parts laid out, of any other the input's own.
dsa_status dsa_encoded_parts(const dsa_encoded *e, uint32_t input, uint32_t *first_stream, uint32_t *count) {
  if (!e || !first_stream || !count) return DSA_ERR_INVALID_ARGUMENT;
  *first_stream = 0; *count = 0;
  const size_t inputs = e->part_first.empty() ? e->streams.size() : e->part_first.size() - 1;
  if (input >= inputs) return DSA_ERR_INVALID_ARGUMENT;
  if (e->part_first.empty()) { *first_stream = input; *count = 1; return DSA_OK; }
  *first_stream = e->part_first[input]; *count = e->part_first[input + 1] - e->part_first[input];
  return DSA_OK;
}
// Which part stream `stream` is, and the box of its points (part_points >= 1).
dsa_status dsa_encoded_part_info(const dsa_encoded *e, uint32_t stream, dsa_part_info *out) {
  if (!e || stream >= e->streams.size() || !out) return DSA_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  if (!e->split) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "this handle has no parts: encode with dsa_encode_split_sequential_batch and part_points >= 1");
  if (e->status[stream] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[stream], "mesh %u: %s", stream, e->messages[stream].c_str());
  *out = e->part_info[stream];
  return DSA_OK;
}
// Which level stream `stream` belongs to (lod_base_bits >= 1).
dsa_status dsa_encoded_lod_info(const dsa_encoded *e, uint32_t stream, dsa_lod_info *out) {
  if (!e || stream >= e->streams.size() || !out) return DSA_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  if (e->lod_bits == 0 || e->lod_info.size() != e->streams.size()) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "this handle has no levels: encode with dsa_encode_lod_sequential_batch and lod_base_bits >= 1");
  if (e->status[stream] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[stream], "mesh %u: %s", stream, e->messages[stream].c_str());
  *out = e->lod_info[stream];
  return DSA_OK;
}
// The entry rows of attribute `attribute` of stream `mesh`: a sequential handle answers with the identity (with point_order = 1:
// with the permutation, the same for every attribute), an Edgebreaker handle with what track_rows kept.
dsa_status dsa_encoded_entry_rows(const dsa_encoded *e, uint32_t mesh, uint32_t attribute, uint32_t *dst, size_t capacity, uint32_t *count) {
  if (!e || mesh >= e->streams.size() || !count) return DSA_ERR_INVALID_ARGUMENT;
  *count = 0;
  if (e->status[mesh] != DSA_OK) return set_err(e->ctx, (dsa_status)e->status[mesh], "mesh %u: %s", mesh, e->messages[mesh].c_str());
  if (e->rows_kind == dsa_encoded::ROWS_NONE) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "the entry rows of this handle were not kept: encode with dsa_encode_rows_batch and track_rows = 1");
  const uint32_t attributes = e->row_attributes(mesh);
  if (attribute >= attributes) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u: attribute %u of %u", mesh, attribute, attributes);
  const uint32_t entries = e->row_entries(mesh, attribute);
  const uint32_t *rows = e->row_data(mesh, attribute);
  *count = entries;
  if (!dst) return DSA_OK;
  if (capacity < entries) return set_err(e->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u, attribute %u: %u entry rows, room for %llu", mesh, attribute, entries, (unsigned long long)capacity);
  if (!rows) for (uint32_t i = 0; i < entries; ++i) dst[i] = i;
  else if (entries) memcpy(dst, rows, 4ull * entries);
  return DSA_OK;
}

void dsa_encoded_free(dsa_encoded *e) { delete e; }

}  // extern "C"

#undef ENC_TRY
#undef ENC_ST
#undef ENC_STAGE
