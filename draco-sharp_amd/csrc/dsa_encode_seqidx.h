// draco-sharp_amd/csrc/dsa_encode_seqidx.h  (included by dsa_encode_sequential.h)
//
// Encode direction, compressed indices of a sequential mesh on the device (MeshSequentialEncoder.cs:84-121, the bitstream's
// form): symbol k = |f[k] - f[k-1]| << 1 | sign with f[-1] = 0 over the faces as they were uploaded, and what symbol_stats of the
// host coder (dsa_encode_host.h, nc = 1) gathers of them -- bit length per symbol, maximum, raw histogram over an alphabet of up
// to 2 * num_vertices, the 33-bin histogram of bit lengths and their sum.  The stream then is a list whose symbols are given
// (EncStream kind 3): k_enc_plan and k_enc_rans code it like any other.
//
// Nothing here is sequential: a grid-parallel kernel, blocks per mesh x meshes.  Where the counts go is what costs.  Index
// deltas of a real mesh pile onto a handful of values (a triangle strip of a grid repeats five of them), and one global atomic
// per symbol on those is what cost k_enc_corr a third of its time.  So a block counts in LDS and touches
// global memory once per bin it used:
//   * symbols below SEQ_LDS_BINS (the small deltas, where the pile is) in an LDS histogram, flushed at the end of the block;
//   * larger symbols (jumps across the vertex range: spread over the alphabet, little contention) straight to global memory;
//   * bit lengths in one 33-bin LDS histogram per wave of the block; their sum is taken from the bins at the flush, the
//     maximum is kept per thread and joins once.
// LDS over a within-wave aggregation (match-any by ballots): the hot set is a few values, but not one, and a ballot round per
// distinct value of a wave costs more than the LDS atomics it saves; the LDS histogram also bounds the global atomics of a
// block by the bins it used whatever the data.
//
// The three phases of the kernel are functions of (block, thread) with no wave intrinsics, so that tests/hostcheck/encseq_host.cpp
// runs them thread by thread under AddressSanitizer against the host coder.
#pragma once

namespace dsa {

#define SEQ_LDS_BINS 4096u
#define SEQ_BLOCK 256u
#define SEQ_SYMBOLS_PER_BLOCK 4096u      // what a block of the grid is sized for (16 symbols a thread)

struct EncSeqIdx {                 // one per mesh with compressed indices; device memory
  uint64_t faces;                  // u16[count] (narrow) or u32[count]: the point of every corner, as uploaded
  uint32_t count;                  // 3F symbols
  uint32_t narrow;
  uint32_t stream;                 // the mesh's index stream (kind 3: syms, bl, hist_raw, hist_cap, hist_tag, max_value, total_bl, overflow)
  uint32_t pad;
};
struct SeqIdxShared {
  uint32_t hist[SEQ_LDS_BINS];
  uint32_t tag[SEQ_BLOCK / WAVE][33];
  uint32_t max_value;
};

__device__ __forceinline__ void seq_idx_clear(SeqIdxShared &sh, uint32_t tid) {
  for (uint32_t i = tid; i < SEQ_LDS_BINS; i += SEQ_BLOCK) sh.hist[i] = 0;
  for (uint32_t i = tid; i < (SEQ_BLOCK / WAVE) * 33u; i += SEQ_BLOCK) sh.tag[i / 33u][i % 33u] = 0;
  if (tid == 0) sh.max_value = 0;
}
template <class ST>
__device__ __forceinline__ void seq_idx_count(SeqIdxShared &sh, uint8_t *arena, const EncSeqIdx &X, ST &S, uint32_t block, uint32_t blocks, uint32_t tid) {
  const uint16_t *f16 = (const uint16_t *)(arena + X.faces);
  const uint32_t *f32 = (const uint32_t *)(arena + X.faces);
  uint32_t *syms = (uint32_t *)(arena + S.syms);
  uint8_t *bl = arena + S.bl;
  uint32_t *hist = (uint32_t *)(arena + S.hist_raw);
  const uint32_t cap = S.hist_cap, wave = tid / WAVE;
  const bool narrow = X.narrow != 0;
  uint32_t mx = 0;
  for (uint32_t k = block * SEQ_BLOCK + tid; k < X.count; k += blocks * SEQ_BLOCK) {
    const uint32_t cur = narrow ? (uint32_t)f16[k] : f32[k];
    const uint32_t last = k ? (narrow ? (uint32_t)f16[k - 1] : f32[k - 1]) : 0u;
    const uint32_t sy = cur >= last ? (cur - last) << 1 : ((last - cur) << 1) | 1u;
    const uint32_t b = (sy > 0 ? 31u - (uint32_t)__builtin_clz(sy) : 0u) + 1u;
    syms[k] = sy;
    bl[k] = (uint8_t)b;
    atomicAdd(&sh.tag[wave][b], 1u);
    if (sy >= cap) S.overflow = 1;
    else if (sy < SEQ_LDS_BINS) atomicAdd(&sh.hist[sy], 1u);
    else atomicAdd(&hist[sy], 1u);
    mx = sy > mx ? sy : mx;
  }
  if (mx) atomicMax(&sh.max_value, mx);
}
template <class ST>
__device__ __forceinline__ void seq_idx_flush(const SeqIdxShared &sh, uint8_t *arena, ST &S, uint32_t tid) {
  uint32_t *hist = (uint32_t *)(arena + S.hist_raw);
  const uint32_t bins = S.hist_cap < SEQ_LDS_BINS ? S.hist_cap : SEQ_LDS_BINS;
  for (uint32_t i = tid; i < bins; i += SEQ_BLOCK) { const uint32_t c = sh.hist[i]; if (c) atomicAdd(&hist[i], c); }
  if (tid < 33u) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < SEQ_BLOCK / WAVE; ++w) c += sh.tag[w][tid];
    if (c) { atomicAdd(&S.hist_tag[tid], c); atomicAdd(&S.total_bl, (unsigned long long)c * tid); }
  }
  if (tid == 0 && sh.max_value) atomicMax(&S.max_value, sh.max_value);
}

#if defined(__HIPCC__)
template <class ST>
__global__ __launch_bounds__(SEQ_BLOCK) void k_enc_seq_indices(uint8_t *arena, const EncSeqIdx *idx, uint32_t n, ST *streams) {
  const uint32_t mesh = blockIdx.y;
  if (mesh >= n) return;
  const EncSeqIdx X = idx[mesh];
  if (blockIdx.x * SEQ_BLOCK >= X.count) return;            // (the grid is sized for the chunk's largest mesh)
  ST &S = streams[X.stream];
  __shared__ SeqIdxShared sh;
  seq_idx_clear(sh, threadIdx.x);
  __syncthreads();
  seq_idx_count(sh, arena, X, S, blockIdx.x, gridDim.x, threadIdx.x);
  __syncthreads();
  seq_idx_flush(sh, arena, S, threadIdx.x);
}
#endif

}  // namespace dsa
