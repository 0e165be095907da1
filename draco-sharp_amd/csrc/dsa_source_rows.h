// draco-sharp_amd/csrc/dsa_source_rows.h  (included by dsa_api.hip, behind dsa_encode.h)
//
// dsa_batch_source_rows: for a batch decoded from the streams of an encode that kept its entry rows (dsa_encode_rows_batch,
// track_rows = 1; a sequential handle: the identity, or with point_order = 1 the stored permutation, with merge_points = 1 the kept rows), per mesh and attribute one uint32 array with a row per POINT -- which row of
// the arrays the encoder was given the point carries.  Shaped like the vertex arrays (dsa_batch_vertex_arrays): a device block of
// the batch's own [table of SrcRowsMesh | the tracked entry rows | the arrays], filled from pinned staging in one transfer on the
// download stream, k_source_rows (dsa_encode_rows.h) behind the decode's kernels, the arrays down in one transfer, an event of their
// own that dsa_batch_wait waits for; a layout call, a host mirror, a device pointer.  No launch and no transfer is per mesh.
// Meshes the fast kernels handed back (decode_path 2) get theirs as block 1 from the retry batch, as the vertex arrays do.
#pragma once

static_assert(SRC_ROWS_MAX_ATT == DSA_MAX_ATT, "a table record holds every attribute of a mesh");

// What mesh i of the batch is held against: stream em of `encoded`.  Its arrays are refused (the mesh alone) when that stream
// failed, or is not the one the mesh was created from as far as the host can tell before the decode has run: another compressed
// length, another number of attributes.  (The entry counts are known behind the decode: k_source_rows writes nothing for a mesh whose counts are not the tracked ones,
// and dsa_batch_source_rows_layout answers for it.)
static int32_t sr_mesh_status(const dsa_batch *b, uint32_t i, const dsa_encoded *e, uint32_t em) {
  if (em >= e->streams.size()) return DSA_ERR_INVALID_ARGUMENT;
  if (e->status[em] != DSA_OK) return e->status[em];
  const MeshLayout &L = b->layouts[i];
  if (e->streams[em].size() != L.stream_len) return DSA_ERR_INVALID_ARGUMENT;
  const uint32_t attributes = e->row_attributes(em);
  if (attributes != L.cap_attributes || attributes > DSA_MAX_ATT) return DSA_ERR_INVALID_ARGUMENT;
  return DSA_OK;
}
static uint32_t sr_entries(const dsa_encoded *e, uint32_t em, uint32_t a) {
  return e->row_entries(em, a);
}
// The table and the sizes of the block's parts: head = table + tracked entry rows (what goes up), then the arrays (what comes down).
struct SrcRowsPlan { std::vector<dsa::SrcRowsMesh> table; std::vector<int32_t> status; uint64_t table_bytes = 0, head_bytes = 0, bytes = 0; };
static void sr_plan(const dsa_batch *b, const dsa_encoded *e, const uint32_t *encoded_mesh, SrcRowsPlan &P) {
  dsa::SrcRowsMesh none;
  memset(&none, 0, sizeof(none));
  P.table.assign(b->n, none);
  P.status.assign(b->n, DSA_OK);
  P.table_bytes = align_up(sizeof(dsa::SrcRowsMesh) * (uint64_t)(b->n ? b->n : 1), 256);
  uint64_t up = P.table_bytes, down = 0;
  for (uint32_t i = 0; i < b->n; ++i) {
    const uint32_t em = encoded_mesh ? encoded_mesh[i] : i;
    P.status[i] = sr_mesh_status(b, i, e, em);
    if (P.status[i] != DSA_OK) continue;
    const MeshLayout &L = b->layouts[i];
    uint8_t rep[DSA_MAX_ATT];
    map_representatives(b->host[i], L.cap_attributes, rep);
    dsa::SrcRowsMesh &T = P.table[i];
    T.num_attributes = L.cap_attributes; T.cap_points = L.cap_points;
    for (uint32_t a = 0; a < T.num_attributes; ++a) {
      dsa::SrcRowsAttr &A = T.att[a];
      A.map = rep[a] == MAP_REP_IDENTITY ? dsa::SRC_ROWS_IDENTITY : L.map[rep[a]];
      A.num_rows = sr_entries(e, em, a);
      A.rows = dsa::SRC_ROWS_IDENTITY;
      if (e->rows_kind != dsa_encoded::ROWS_LINEAR) { A.rows = up; up = align_up(up + 4ull * A.num_rows, 64); }
      A.out = down; down = align_up(down + 4ull * L.cap_points, 64);      // (relative to the arrays: the head's size is added when it is known)
    }
  }
  P.head_bytes = align_up(up, 256);
  P.bytes = down;
  for (dsa::SrcRowsMesh &T : P.table) for (uint32_t a = 0; a < T.num_attributes; ++a) T.att[a].out += P.head_bytes;
}
static dsa_status sr_check_handle(dsa_context *ctx, const dsa_encoded *e) {
  if (!e) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "null argument");
  if (e->rows_kind == dsa_encoded::ROWS_NONE) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "the entry rows of this handle were not kept: encode with dsa_encode_rows_batch and track_rows = 1");
  return DSA_OK;
}

static dsa_status batch_source_rows(dsa_batch *b, const dsa_encoded *e, const uint32_t *encoded_mesh, void *dst, size_t dst_bytes) {
  dsa_context *ctx = b->ctx;
  if (const dsa_status st = sr_check_handle(ctx, e)) return st;
  if (!b->decoded) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_decode was not called");
  if (b->sr_valid && !b->sr_done) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "the batch's source rows are still in flight");
  const bool to_host = !(dst == nullptr && dst_bytes == DSA_SOURCE_ROWS_DEVICE_ONLY);
  SrcRowsPlan P;
  sr_plan(b, e, encoded_mesh, P);
  if (to_host && dst && dst_bytes < P.bytes) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "destination smaller than the source rows (dsa_batch_source_rows_bytes)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!b->ev_sr) HIP_TRY(ctx, hipEventCreateWithFlags(&b->ev_sr, hipEventDisableTiming));
  if (b->sr_queued && !b->sr_done) { HIP_TRY(ctx, hipEventSynchronize(b->ev_sr)); b->sr_done = true; }      // a request from before the batch was decoded again: its buffers are reused
  const uint64_t need = P.head_bytes + (P.bytes ? P.bytes : 256);
  if (!b->d_sr || b->d_sr_cap < need) {                      // the device block: from the cache the vertex arrays' blocks come from
    ctx->spare_vertex.give(b->d_sr, b->d_sr_cap);
    b->d_sr = nullptr; b->d_sr_cap = 0;
    if (dsa_status st = get_block(ctx, ctx->spare_vertex, need, spares::grow_exact, {&ctx->spare_vertex, &ctx->spare_packed, &ctx->spare_arenas}, "source-rows block of %llu bytes: %s", &b->d_sr, &b->d_sr_cap)) return st;
  }
  if (!b->sr_pin || b->sr_pin_bytes < P.head_bytes) {        // pinned staging of the head
    ctx->spare_mirrors.give(b->sr_pin, b->sr_pin_bytes);
    b->sr_pin = nullptr; b->sr_pin_bytes = 0;
    if (dsa_status st = get_block(ctx, ctx->spare_mirrors, P.head_bytes, spares::grow_floor256, {&ctx->spare_mirrors}, "pinned staging of %llu bytes for the entry rows: %s", &b->sr_pin, &b->sr_pin_bytes)) return st;
  }
  if (to_host) { if (dsa_status st = place(ctx, b->sr_mirror, dst, dst_bytes, P.bytes ? P.bytes : 256)) return st; }
  b->sr.swap(P.table); b->sr_status.swap(P.status);
  b->sr_bytes = P.bytes; b->sr_head_bytes = P.head_bytes; b->sr_to_host = to_host;
  b->sr_encoded = e;
  b->sr_map.clear();
  if (encoded_mesh) b->sr_map.assign(encoded_mesh, encoded_mesh + b->n); else for (uint32_t i = 0; i < b->n; ++i) b->sr_map.push_back(i);
  // the head: the table, and behind it the entry rows of every mesh that has arrays
  if (b->n) memcpy(b->sr_pin, b->sr.data(), sizeof(dsa::SrcRowsMesh) * (size_t)b->n);
  hostutil::parallel_for(b->n, [&](uint32_t i) {
    const dsa::SrcRowsMesh &T = b->sr[i];
    for (uint32_t a = 0; a < T.num_attributes; ++a)
      if (T.att[a].rows != dsa::SRC_ROWS_IDENTITY && T.att[a].num_rows) memcpy(b->sr_pin + T.att[a].rows, e->row_data(b->sr_map[i], a), 4ull * T.att[a].num_rows);
  }, 64);
  HIP_TRY(ctx, hipMemcpyAsync(b->d_sr, b->sr_pin, P.head_bytes, hipMemcpyHostToDevice, ctx->down));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->down, b->ev_done, 0));
  if (b->n && P.bytes) {
    uint32_t max_points = 0;
    for (uint32_t i = 0; i < b->n; ++i) max_points = std::max(max_points, b->layouts[i].cap_points);
    const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((max_points + 8 * 256 - 1) / (8 * 256), 16));
    hipLaunchKernelGGL(dsa::k_source_rows<MeshDesc>, dim3(gx, b->n), dim3(256), 0, ctx->down, (const uint8_t *)b->arena, (const MeshDesc *)b->d_descs, b->n, (const dsa::SrcRowsMesh *)b->d_sr, b->d_sr);
    HIP_TRY(ctx, hipGetLastError());
    if (to_host) HIP_TRY(ctx, copy_down(ctx, b->sr_mirror.p, b->d_sr + P.head_bytes, P.bytes));
  }
  HIP_TRY(ctx, hipEventRecord(b->ev_sr, ctx->down));
  b->sr_valid = true; b->sr_queued = true; b->sr_done = false;
  if (b->retry) {                                            // block 1: the meshes decoded a second time
    std::vector<uint32_t> again(b->retry->n, 0);
    for (uint32_t i = 0; i < b->n; ++i) if (b->retry_index[i] >= 0 && (uint32_t)b->retry_index[i] < b->retry->n) again[b->retry_index[i]] = i;
    return batch_source_rows_retry(b, b->retry, again);
  }
  return DSA_OK;
}
// block 1 of the request the batch holds, on its retry batch: mesh k there is mesh again[k] here
static dsa_status batch_source_rows_retry(dsa_batch *b, dsa_batch *rb, const std::vector<uint32_t> &again) {
  std::vector<uint32_t> em(rb->n, 0);
  for (uint32_t k = 0; k < rb->n && k < again.size(); ++k) em[k] = b->sr_map[again[k]];
  return batch_source_rows(rb, b->sr_encoded, em.data(), nullptr, b->sr_to_host ? 0 : DSA_SOURCE_ROWS_DEVICE_ONLY);
}

extern "C" {

uint64_t dsa_batch_source_rows_bytes(const dsa_batch *b, const dsa_encoded *e, const uint32_t *encoded_mesh) {
  if (!b || !e || e->rows_kind == dsa_encoded::ROWS_NONE) return 0;
  try { SrcRowsPlan P; sr_plan(b, e, encoded_mesh, P); return P.bytes; } catch (...) { return 0; }
}
dsa_status dsa_batch_source_rows(dsa_batch *b, const dsa_encoded *e, const uint32_t *encoded_mesh, void *dst, size_t dst_bytes) {
  if (!b) return DSA_ERR_INVALID_ARGUMENT;
  DSA_GUARD(b->ctx, batch_source_rows(b, e, encoded_mesh, dst, dst_bytes));
}
const void *dsa_batch_host_source_rows(const dsa_batch *b, uint32_t block) {
  if (!b || !b->sr_valid || !b->sr_done) return nullptr;
  if (block == 1) return b->retry ? dsa_batch_host_source_rows(b->retry, 0) : nullptr;
  return block == 0 && b->sr_to_host ? b->sr_mirror.p : nullptr;
}
const void *dsa_batch_device_source_rows(const dsa_batch *b, uint32_t block) {
  if (!b || !b->sr_valid) return nullptr;
  if (block == 1) return b->retry ? dsa_batch_device_source_rows(b->retry, 0) : nullptr;
  return block == 0 && b->d_sr ? b->d_sr + b->sr_head_bytes : nullptr;
}
dsa_status dsa_batch_source_rows_layout(const dsa_batch *b, uint32_t mesh, dsa_mesh_source_rows *out) {
  const Located at = locate(b, mesh);
  const dsa_batch *src = at.b; const uint32_t m = at.mesh;
  CHECK_MESH(src, m);
  if (!out) return DSA_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  out->block = at.block;
  for (uint32_t a = 0; a < DSA_MAX_ATTRIBUTES; ++a) out->rows[a] = UINT64_MAX;
  if (!src->sr_valid || m >= src->sr.size()) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "no source rows were requested since the batch was decoded");
  const MeshDesc &D = src->descs[m];
  if (D.status != ST_OK) return set_err(b->ctx, (dsa_status)D.status, "mesh %u failed to decode", (unsigned)mesh);
  if (src->sr_status[m] != DSA_OK)
    return set_err(b->ctx, (dsa_status)src->sr_status[m], src->sr_status[m] == DSA_ERR_INVALID_ARGUMENT ? "mesh %u: the stream it was decoded from is not stream %u of the encoded handle (compressed length or attribute count differ)" : "mesh %u: stream %u of the encoded handle failed to encode", (unsigned)mesh, (unsigned)src->sr_map[m]);
  const dsa::SrcRowsMesh &T = src->sr[m];
  if (D.num_attributes != T.num_attributes) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u: %u attributes decoded, %u tracked", (unsigned)mesh, (unsigned)D.num_attributes, (unsigned)T.num_attributes);
  for (uint32_t a = 0; a < T.num_attributes; ++a)
    if (D.att[a].num_entries != T.att[a].num_rows)
      return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u, attribute %u: %u entries decoded, %u tracked: not the stream the rows were kept for", (unsigned)mesh, a, (unsigned)D.att[a].num_entries, (unsigned)T.att[a].num_rows);
  out->num_points = std::min(D.num_points, T.cap_points);
  out->num_attributes = T.num_attributes;
  for (uint32_t a = 0; a < T.num_attributes; ++a) out->rows[a] = T.att[a].out - src->sr_head_bytes;
  return DSA_OK;
}

}  // extern "C"
