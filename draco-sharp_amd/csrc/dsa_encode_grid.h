// draco-sharp_amd/csrc/dsa_encode_grid.h  (included by dsa_encode_layout.h, behind dsa_encode_weld.h)
//
// Encode direction: quantisation grids that are not the attribute's own bounds (dsa_encode_grid_batch,
// dsa_encode_grid_sequential_batch; include/draco_mi355x.h dsa_quantization_grid) -- given by the caller (mode 1) or shared by the
// meshes of a group (mode 2).  It is synth::quantize_on_grid and synth::shared_grid of dsa_encode_host.h on arrays in device
// memory; tests/hostcheck/encgrid_host.cpp holds the two against each other.
//   once per request, in front of its chunks (enc_stage_grids: a group may span chunks and both passes of a repair request):
//     k_enc_grid_bounds    per (mesh, attribute slot) of mode 2: minimum and maximum per component over all rows, and whether a
//                          value is not finite.  Blocks over rows x items; a thread folds its rows, (on the device) a wave its
//                          threads, and the item takes the result by atomicMin / atomicMax on order keys of the floats (-0.0
//                          below +0.0): minima and maxima of integers, the same bits whatever the grid of blocks.
//     k_enc_grid_fold      per group (a run of items with one group number, slot and component count): the fold of its items
//                          without such a value into origin and range (ComputeParameters over the union: the largest extent, 1 if 0)
//   in the chunk that codes the attribute, in place of k_enc_bounds / k_enc_quantize for the streams with a grid (whose records
//   carry origin and range from the host: EncStream::grid_mode, qmin, qrange):
//     k_enc_grid_quantize  the quantiser's arithmetic, and the smallest row with a value that is not finite / whose integer
//                          leaves 0 .. max_q (atomicMin into the stream's record; such a value is written as 0, so that whatever
//                          runs behind it on the device stays inside its histograms)
// Streams without a grid never come here.  Vector stores and vector atomics only.
#pragma once

namespace dsa {

static const uint32_t ENC_GRID_NO_ROW = 0xFFFFFFFFu;
struct EncGridItem {               // one (mesh, attribute slot) that shares a grid; device memory, mirrored on the host
  uint64_t src;                    // f32[rows * nc] among the inputs of the stage's arena
  uint32_t rows, nc;
  uint32_t mn[4], mx[4];           // OUTPUT order keys (enc_grid_key) of the minima / maxima; the host sets 0xFFFFFFFF / 0
  uint32_t nonfinite, pad;         // OUTPUT 1: some value is not finite (the item takes no part in its group's grid)
};
struct EncGridGroup {              // one grid: items first .. first + count (of one group number, slot and component count)
  uint32_t first, count, nc;
  uint32_t clean;                  // OUTPUT items that took part
  float origin[4], range;          // OUTPUT (no clean item: 0 and 1, which nothing is coded on -- every member is refused)
  uint32_t pad[3];
};

// floats as integers of the same order, -0.0 below +0.0 (NaNs sort outside the infinities and never get here)
__device__ __forceinline__ uint32_t enc_grid_key(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float enc_grid_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
__device__ __forceinline__ bool enc_grid_finite(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0x7F800000u) != 0x7F800000u;
}
// one rounding per step, as the host coder's volatile floats
#if defined(__HIPCC__)
__device__ __forceinline__ float enc_grid_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float enc_grid_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float enc_grid_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float enc_grid_div(float a, float b) { return __fdiv_rn(a, b); }
#else
static inline float enc_grid_sub(float a, float b) { volatile float r = a - b; return r; }
static inline float enc_grid_mul(float a, float b) { volatile float r = a * b; return r; }
static inline float enc_grid_add(float a, float b) { volatile float r = a + b; return r; }
static inline float enc_grid_div(float a, float b) { volatile float r = a / b; return r; }
#endif

// grid: (blocks over rows, items)
__global__ __launch_bounds__(256) void k_enc_grid_bounds(const uint8_t *arena, EncGridItem *items, uint32_t n) {
  const uint32_t it = blockIdx.y;
  if (it >= n) return;
  EncGridItem &I = items[it];
  const float *src = (const float *)(arena + I.src);
  const uint32_t nc = I.nc < 4u ? I.nc : 4u;
  uint32_t mn[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[4] = {0u, 0u, 0u, 0u}, bad = 0u;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x; v < I.rows; v += stride)
    for (uint32_t c = 0; c < nc; ++c) {
      const float x = src[(size_t)v * nc + c];
      if (!enc_grid_finite(x)) { bad = 1u; continue; }
      const uint32_t k = enc_grid_key(x);
      mn[c] = k < mn[c] ? k : mn[c];
      mx[c] = k > mx[c] ? k : mx[c];
    }
#if defined(__HIPCC__)
  // the wave's fold: one set of atomics per wave (inactive rows hold the identities)
  for (uint32_t o = WAVE / 2; o >= 1; o >>= 1) {
    for (uint32_t c = 0; c < 4; ++c) {
      const uint32_t a = (uint32_t)__shfl_xor((int)mn[c], (int)o, WAVE), b = (uint32_t)__shfl_xor((int)mx[c], (int)o, WAVE);
      mn[c] = a < mn[c] ? a : mn[c];
      mx[c] = b > mx[c] ? b : mx[c];
    }
    bad |= (uint32_t)__shfl_xor((int)bad, (int)o, WAVE);
  }
  if ((threadIdx.x & (WAVE - 1u)) != 0u) return;
#endif
  for (uint32_t c = 0; c < nc; ++c) {
    if (mn[c] != 0xFFFFFFFFu) atomicMin(&I.mn[c], mn[c]);
    if (mx[c] != 0u) atomicMax(&I.mx[c], mx[c]);
  }
  if (bad) atomicMax(&I.nonfinite, 1u);
}

// one thread per group
__global__ __launch_bounds__(WAVE) void k_enc_grid_fold(const EncGridItem *items, EncGridGroup *groups, uint32_t ng) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng) return;
  EncGridGroup &G = groups[g];
  const uint32_t nc = G.nc < 4u ? G.nc : 4u;
  uint32_t mn[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[4] = {0u, 0u, 0u, 0u}, clean = 0u;
  for (uint32_t k = G.first; k < G.first + G.count; ++k) {
    const EncGridItem &I = items[k];
    if (I.nonfinite || I.rows == 0u) continue;
    ++clean;
    for (uint32_t c = 0; c < nc; ++c) { mn[c] = I.mn[c] < mn[c] ? I.mn[c] : mn[c]; mx[c] = I.mx[c] > mx[c] ? I.mx[c] : mx[c]; }
  }
  float range = 0.0f;
  for (uint32_t c = 0; c < 4; ++c) G.origin[c] = 0.0f;
  for (uint32_t c = 0; c < nc && clean; ++c) {
    const float lo = enc_grid_float(mn[c]), d = enc_grid_sub(enc_grid_float(mx[c]), lo);
    G.origin[c] = lo;
    if (d > range) range = d;
  }
  G.range = range == 0.0f ? 1.0f : range;
  G.clean = clean;
}

// The streams of a chunk with a grid (kind 0, grid_mode != 0; qmin / qrange hold it): Quantizer, floor((v - origin) * (max_q /
// range) + 0.5) with every step rounded to f32 -- k_enc_quantize's arithmetic -- and the check of every value.  grid: (blocks
// over values, streams)
template <class Stream>
__global__ __launch_bounds__(256) void k_enc_grid_quantize(uint8_t *arena, Stream *streams, uint32_t ns) {
  const uint32_t si = blockIdx.y;
  if (si >= ns) return;
  Stream &S = streams[si];
  if (S.kind != 0 || S.grid_mode == 0) return;
  const float *src = (const float *)(arena + S.src);
  int32_t *vals = (int32_t *)(arena + S.vals);
  const float max_q = (float)(int32_t)((1u << S.bits) - 1u), inv_delta = enc_grid_div(max_q, S.qrange);
  const uint32_t nc = S.nc_out, total = S.rows * nc;
  uint32_t bad_finite = ENC_GRID_NO_ROW, bad_off = ENC_GRID_NO_ROW;      // ascending rows per thread: the first is its smallest
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x; i < total; i += stride) {
    const float x = src[i];
    const float f = floorf(enc_grid_add(enc_grid_mul(enc_grid_sub(x, S.qmin[i % nc]), inv_delta), 0.5f));
    const bool finite = enc_grid_finite(x), on = f >= 0.0f && f <= max_q;
    vals[i] = finite && on ? (int32_t)f : 0;
    if (!finite) { if (bad_finite == ENC_GRID_NO_ROW) bad_finite = i / nc; }
    else if (!on && bad_off == ENC_GRID_NO_ROW) bad_off = i / nc;
  }
  if (bad_finite != ENC_GRID_NO_ROW) atomicMin(&S.grid_nonfinite, bad_finite);
  if (bad_off != ENC_GRID_NO_ROW) atomicMin(&S.grid_off, bad_off);
}

}  // namespace dsa
