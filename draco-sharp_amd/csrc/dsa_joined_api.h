// draco-sharp_amd/csrc/dsa_joined_api.h  (included by dsa_api.hip, behind dsa_source_rows.h)
//
// dsa_batch_joined_arrays: the host side of the joined vertex arrays (layout, gather body and kernel: dsa_joined_arrays.h).  Shaped
// like dsa_batch_source_rows: a device block of the batch's own [member list | group records | target rows | arrays], the head
// filled from pinned staging in one transfer on the download stream, k_joined_arrays behind the decode's kernels, the arrays down
// in one transfer, an event of their own that dsa_batch_wait waits for; a layout call, a host mirror, a device pointer.  No launch
// and no transfer is per mesh or per group.  What the call can know (headers, the handle's part records) is decided here and
// kept per group; what the decode decides (a failed member, a second decode, differing grids) is read from the descriptors when the
// layout is asked for.
#pragma once

static const char *ja_request_fault(const dsa_join_request *r) {
  if (!r) return "dsa_join_request (null)";
  if (const char *f = va_request_fault(&r->arrays)) return !strcmp(f, "format") ? "dsa_join_request.arrays.format" : !strcmp(f, "flags") ? "dsa_join_request.arrays.flags" : "dsa_join_request.arrays.reserved";
  if (r->order != DSA_JOIN_STREAM_ORDER && r->order != DSA_JOIN_INPUT_ORDER) return "dsa_join_request.order";
  for (uint32_t w : r->reserved) if (w) return "dsa_join_request.reserved";
  return nullptr;
}

struct JoinPlan {
  std::vector<JaMember> members;
  std::vector<JaGroup> groups;
  std::vector<int32_t> status;
  std::vector<std::string> text;
  std::vector<uint32_t> first_row;
  std::vector<int32_t> group_of;
  uint64_t members_bytes = 0, groups_bytes = 0, head_bytes = 0, bytes = 0;
  uint32_t max_points = 0;
};
static std::string ja_words(const char *fmt, ...) {
  char buf[384];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}
// What of the group list the call itself refuses, in words that name the field (empty: nothing).
static std::string ja_groups_fault(const dsa_batch *b, uint32_t num_groups, const dsa_join_group *groups) {
  if (num_groups && !groups) return "groups is null with num_groups > 0";
  std::vector<uint8_t> taken(b->n, 0);
  for (uint32_t g = 0; g < num_groups; ++g) {
    if (groups[g].num_meshes == 0) return ja_words("groups[%u].num_meshes is 0", g);
    if (groups[g].first_mesh >= b->n || groups[g].num_meshes > b->n - groups[g].first_mesh)
      return ja_words("groups[%u] (first_mesh %u, num_meshes %u) reaches beyond the batch of %u meshes", g, groups[g].first_mesh, groups[g].num_meshes, b->n);
    for (uint32_t k = 0; k < groups[g].num_meshes; ++k) {
      if (taken[groups[g].first_mesh + k]) return ja_words("groups[%u]: mesh %u is in two groups", g, groups[g].first_mesh + k);
      taken[groups[g].first_mesh + k] = 1;
    }
  }
  return std::string();
}
// For input order: what the handle says about group g (members first .. first + count), before the decode has run.
static int32_t ja_input_fault(const dsa_batch *b, uint32_t g, uint32_t first, uint32_t count, const dsa_encoded *e, const uint32_t *encoded_mesh, std::string &text) {
  if (e->merged) { text = ja_words("group %u: the handle was made with merge_points = 1: many input rows share an entry, gather joined[row_entries] instead", g); return DSA_ERR_INVALID_ARGUMENT; }
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t mesh = first + k, em = encoded_mesh ? encoded_mesh[mesh] : mesh;
    if (em >= e->streams.size()) { text = ja_words("group %u, member %u: stream %u is beyond the %u streams of the encoded handle", g, k, em, (unsigned)e->streams.size()); return DSA_ERR_INVALID_ARGUMENT; }
    if (e->status[em] != DSA_OK) { text = ja_words("group %u, member %u: stream %u of the encoded handle failed to encode", g, k, em); return e->status[em]; }
    if (sr_mesh_status(b, mesh, e, em) != DSA_OK) {
      text = ja_words("group %u, member %u: the stream mesh %u was created from is not stream %u of the encoded handle (compressed length or attribute count differ)", g, k, mesh, em);
      return DSA_ERR_INVALID_ARGUMENT;
    }
    if (e->row_attributes(em) && e->row_entries(em, 0) != b->layouts[mesh].cap_points) {
      text = ja_words("group %u, member %u: the header of mesh %u counts %u points, stream %u of the encoded handle %u rows", g, k, mesh, b->layouts[mesh].cap_points, em, e->row_entries(em, 0));
      return DSA_ERR_INVALID_ARGUMENT;
    }
  }
  const uint32_t em0 = encoded_mesh ? encoded_mesh[first] : first;
  if (e->part_info.empty()) {
    if (count != 1) { text = ja_words("group %u: the encoded handle has no parts, so a group in input order has one member (it has %u)", g, count); return DSA_ERR_INVALID_ARGUMENT; }
    return DSA_OK;
  }
  const uint32_t input = e->part_info[em0].input, lo = e->part_first[input], parts = e->part_first[input + 1] - lo;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t em = encoded_mesh ? encoded_mesh[first + k] : first + k;
    if (em != lo + k || count != parts) {
      text = ja_words("group %u, member %u: the members of a group in input order are all parts of one input in part order (input %u: streams %u .. %u; member %u is stream %u of %u members)", g,
                      k, input, lo, lo + parts - 1, k, em, count);
      return DSA_ERR_INVALID_ARGUMENT;
    }
  }
  return DSA_OK;
}
// The tables and the sizes of the block's parts: head = member list + group records + target rows (what goes up), then the arrays.
static void ja_plan(const dsa_batch *b, const dsa_join_request &r, uint32_t num_groups, const dsa_join_group *groups, const dsa_encoded *e, const uint32_t *encoded_mesh, JoinPlan &P) {
  P.groups.assign(num_groups, JaGroup());
  P.status.assign(num_groups, DSA_OK);
  P.text.assign(num_groups, std::string());
  P.first_row.assign(b->n, 0);
  P.group_of.assign(b->n, -1);
  uint32_t total = 0;
  for (uint32_t g = 0; g < num_groups; ++g) total += groups[g].num_meshes;
  P.members_bytes = align_up(sizeof(JaMember) * (uint64_t)(total ? total : 1), 256);
  P.groups_bytes = align_up(sizeof(JaGroup) * (uint64_t)(num_groups ? num_groups : 1), 256);
  uint64_t up = P.members_bytes + P.groups_bytes, cur = 0;
  std::vector<VaAttrIn> atts;
  std::vector<JaMemberIn> in;
  for (uint32_t g = 0; g < num_groups; ++g) {
    const uint32_t first = groups[g].first_mesh, count = groups[g].num_meshes;
    atts.assign((size_t)count * DSA_MAX_ATT, VaAttrIn());
    in.resize(count);
    for (uint32_t k = 0; k < count; ++k) {
      const HostMesh &h = b->host[first + k];
      const MeshLayout &L = b->layouts[first + k];
      const uint32_t natt = std::min<uint32_t>(L.cap_attributes, DSA_MAX_ATT);
      for (uint32_t a = 0; a < natt && a < h.atts.size(); ++a) atts[(size_t)k * DSA_MAX_ATT + a] = {h.atts[a].att_type, h.atts[a].data_type, h.atts[a].nc, h.atts[a].seq_type, VA_IDENTITY};
      in[k] = {atts.data() + (size_t)k * DSA_MAX_ATT, natt, L.cap_points, h.faces != 0 ? 1u : 0u};
      P.group_of[first + k] = (int32_t)g;
    }
    int why = JA_OK; uint32_t bad = 0;
    cur = ja_layout_group(in.data(), count, r.arrays.format, r.arrays.attribute_types, cur, P.groups[g], P.first_row.data() + first, &why, &bad);
    if (why != JA_OK) {
      P.status[g] = DSA_ERR_INVALID_ARGUMENT;
      P.text[g] = why == JA_FACES ? ja_words("group %u, member %u: mesh %u has faces: joined index arrays are not built", g, bad, first + bad)
                : why == JA_ROWS ? ja_words("group %u, member %u: the rows of the group add up to more than 2^32 - 1", g, bad)
                : ja_words("group %u, member %u: the attribute table of mesh %u differs from that of mesh %u (attribute count, or an attribute's type, data type, components or decoder type)", g, bad, first + bad, first);
    } else if (r.order == DSA_JOIN_INPUT_ORDER) P.status[g] = ja_input_fault(b, g, first, count, e, encoded_mesh, P.text[g]);
    if (P.status[g] != DSA_OK) continue;
    for (uint32_t k = 0; k < count; ++k) {
      JaMember M = {first + k, g, P.first_row[first + k], in[k].points, JA_NO_ROWS};
      if (r.order == DSA_JOIN_INPUT_ORDER && e->rows_kind == dsa_encoded::ROWS_ORDERED && M.num_points) { M.rows = up - P.members_bytes - P.groups_bytes; up = align_up(up + 4ull * M.num_points, 64); }
      P.max_points = std::max(P.max_points, M.num_points);
      P.members.push_back(M);
    }
  }
  P.head_bytes = align_up(up, 256);
  P.bytes = cur;
}

static dsa_status batch_joined_arrays(dsa_batch *b, const dsa_join_request *request, uint32_t num_groups, const dsa_join_group *groups, const dsa_encoded *e,
                                      const uint32_t *encoded_mesh, void *dst, size_t dst_bytes) {
  dsa_context *ctx = b->ctx;
  if (const char *field = ja_request_fault(request)) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "%s is outside its values", field);
  const std::string fault = ja_groups_fault(b, num_groups, groups);
  if (!fault.empty()) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_joined_arrays: %s", fault.c_str());
  const dsa_join_request req = *request;
  if (req.order == DSA_JOIN_INPUT_ORDER) {
    if (!e) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_joined_arrays: order DSA_JOIN_INPUT_ORDER needs `encoded`, the handle the streams came from");
    if (e->rows_kind == dsa_encoded::ROWS_NONE) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_joined_arrays: `encoded` kept no rows: order DSA_JOIN_INPUT_ORDER takes the handle of a sequential call");
    if (e->rows_kind == dsa_encoded::ROWS_TRACKED) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_joined_arrays: `encoded` is an Edgebreaker handle: order DSA_JOIN_INPUT_ORDER takes the handle of a sequential call");
  }
  if (!b->decoded) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_batch_decode was not called");
  if (b->ja_valid && !b->ja_done) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "the batch's joined arrays are still in flight");
  JoinPlan P;
  ja_plan(b, req, num_groups, groups, e, encoded_mesh, P);
  const bool to_host = !(req.arrays.flags & DSA_VA_DEVICE_ONLY);
  if (to_host && dst && dst_bytes < P.bytes) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dst_bytes: destination smaller than the joined arrays (dsa_batch_joined_arrays_bytes)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!b->ev_ja) HIP_TRY(ctx, hipEventCreateWithFlags(&b->ev_ja, hipEventDisableTiming));
  if (b->ja_queued && !b->ja_done) { HIP_TRY(ctx, hipEventSynchronize(b->ev_ja)); b->ja_done = true; }      // a request from before the batch was decoded again: its buffers are reused
  const uint64_t need = P.head_bytes + (P.bytes ? P.bytes : 256);
  if (!b->d_ja || b->d_ja_cap < need) {                      // the device block: from the cache the vertex arrays' blocks come from
    ctx->spare_vertex.give(b->d_ja, b->d_ja_cap);
    b->d_ja = nullptr; b->d_ja_cap = 0;
    if (dsa_status st = get_block(ctx, ctx->spare_vertex, need, spares::grow_exact, {&ctx->spare_vertex, &ctx->spare_packed, &ctx->spare_arenas}, "joined-array block of %llu bytes: %s", &b->d_ja, &b->d_ja_cap)) return st;
  }
  if (!b->ja_pin || b->ja_pin_bytes < P.head_bytes) {        // pinned staging of the head
    ctx->spare_mirrors.give(b->ja_pin, b->ja_pin_bytes);
    b->ja_pin = nullptr; b->ja_pin_bytes = 0;
    if (dsa_status st = get_block(ctx, ctx->spare_mirrors, P.head_bytes, spares::grow_floor256, {&ctx->spare_mirrors}, "pinned staging of %llu bytes for the joined arrays: %s", &b->ja_pin, &b->ja_pin_bytes)) return st;
  }
  if (to_host) { if (dsa_status st = place(ctx, b->ja_mirror, dst, dst_bytes, P.bytes ? P.bytes : 256)) return st; }
  b->ja_members.swap(P.members); b->ja_groups.swap(P.groups); b->ja_status.swap(P.status); b->ja_text.swap(P.text);
  b->ja_first_row.swap(P.first_row); b->ja_group_of.swap(P.group_of);
  b->ja_list.assign(groups, groups + num_groups);
  b->ja_req = req; b->ja_bytes = P.bytes; b->ja_head_bytes = P.head_bytes;
  // the head: the member list, the group records, and behind them the target rows of every member that has some
  const uint32_t nm = (uint32_t)b->ja_members.size();
  if (nm) memcpy(b->ja_pin, b->ja_members.data(), sizeof(JaMember) * (size_t)nm);
  if (num_groups) memcpy(b->ja_pin + P.members_bytes, b->ja_groups.data(), sizeof(JaGroup) * (size_t)num_groups);
  uint8_t *rows_pin = b->ja_pin + P.members_bytes + P.groups_bytes;
  hostutil::parallel_for(nm, [&](uint32_t k) {
    const JaMember &M = b->ja_members[k];
    if (M.rows != JA_NO_ROWS) memcpy(rows_pin + M.rows, e->row_data(encoded_mesh ? encoded_mesh[M.mesh] : M.mesh, 0), 4ull * M.num_points);
  }, 64);
  HIP_TRY(ctx, hipMemcpyAsync(b->d_ja, b->ja_pin, P.head_bytes, hipMemcpyHostToDevice, ctx->down));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->down, b->ev_done, 0));
  if (nm && P.bytes) {
    const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((P.max_points + 8 * VA_CHUNK - 1) / (8 * VA_CHUNK), 16));
    for (uint32_t first = 0; first < nm; first += 65535u) {                                 // a cloud may have 65 536 parts: grid.y ends at 65 535
      const uint32_t gy = std::min<uint32_t>(nm - first, 65535u);
      hipLaunchKernelGGL(dsa::k_joined_arrays, dim3(gx, gy), dim3(VA_CHUNK), 0, ctx->down, (const uint8_t *)b->arena, (const MeshLayout *)b->d_layouts, (const MeshDesc *)b->d_descs, b->n,
                         (const JaMember *)b->d_ja, first, nm, (const JaGroup *)(b->d_ja + P.members_bytes), (const uint8_t *)(b->d_ja + P.members_bytes + P.groups_bytes), b->d_ja + P.head_bytes);
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  // the library's mirror takes the block in one transfer; in a caller's buffer only the arrays are written, array by array, so
  // that what lies between them (the padding up to the next 64 bytes) stays the caller's
  if (P.bytes && to_host && !dst) HIP_TRY(ctx, copy_down(ctx, b->ja_mirror.p, b->d_ja + P.head_bytes, P.bytes));
  if (P.bytes && to_host && dst)
    for (const JaGroup &T : b->ja_groups)
      for (uint32_t a = 0; a < T.cap_attributes; ++a)
        if (T.att[a].offset != VA_NONE && T.cap_points) HIP_TRY(ctx, copy_down(ctx, b->ja_mirror.p + T.att[a].offset, b->d_ja + P.head_bytes + T.att[a].offset, (uint64_t)T.att[a].stride * T.cap_points));
  HIP_TRY(ctx, hipEventRecord(b->ev_ja, ctx->down));
  b->ja_valid = true; b->ja_queued = true; b->ja_done = false;
  return DSA_OK;
}

// What the decode decided about group g (the descriptors are in: dsa_batch_wait has returned).
static dsa_status ja_group_verdict(const dsa_batch *b, uint32_t g) {
  const dsa_join_group &G = b->ja_list[g];
  const JaGroup &T = b->ja_groups[g];
  for (uint32_t k = 0; k < G.num_meshes; ++k) {
    const uint32_t mesh = G.first_mesh + k;
    if (b->retry && mesh < b->retry_index.size() && b->retry_index[mesh] >= 0)
      return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "group %u, member %u: mesh %u was decoded a second time (decode_path 2): the join does not read the retry batch", g, k, mesh);
    const MeshDesc &D = b->descs[mesh];
    if (D.status != ST_OK) return set_err(b->ctx, (dsa_status)D.status, "group %u, member %u: mesh %u failed to decode", g, k, mesh);
    if (D.num_attributes != T.cap_attributes) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "group %u, member %u: mesh %u decoded %u attributes, its header announced %u", g, k, mesh, (unsigned)D.num_attributes, (unsigned)T.cap_attributes);
    if (b->ja_req.arrays.format != DSA_VA_QUANTIZED || k == 0) continue;
    const MeshDesc &D0 = b->descs[G.first_mesh];
    for (uint32_t a = 0; a < T.cap_attributes; ++a) {
      if (T.att[a].kind != VA_KIND_QUANTIZED || T.att[a].offset == VA_NONE) continue;
      const AttrDesc &A = D.att[a], &A0 = D0.att[a];
      bool same = A.q_bits == A0.q_bits;
      if (A.seq_type == 2) same = same && memcmp(&A.q_range, &A0.q_range, 4) == 0 && memcmp(A.q_min, A0.q_min, 4 * std::min<uint32_t>(A.nc, 4)) == 0;
      if (!same)
        return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "group %u, member %u: attribute %u of mesh %u is quantised on another grid than that of mesh %u (quantization_bits, min_values or range differ): joined integers need one grid, take DSA_VA_VALUES", g, k, a, mesh, G.first_mesh);
    }
  }
  return DSA_OK;
}

extern "C" {

uint64_t dsa_batch_joined_arrays_bytes(const dsa_batch *b, const dsa_join_request *request, uint32_t num_groups, const dsa_join_group *groups) {
  if (!b || ja_request_fault(request)) return 0;
  try {
    if (!ja_groups_fault(b, num_groups, groups).empty()) return 0;
    dsa_join_request r = *request;
    r.order = DSA_JOIN_STREAM_ORDER;                      // (the block is the same in both orders)
    JoinPlan P; ja_plan(b, r, num_groups, groups, nullptr, nullptr, P); return P.bytes;
  } catch (...) { return 0; }
}
dsa_status dsa_batch_joined_arrays(dsa_batch *b, const dsa_join_request *request, uint32_t num_groups, const dsa_join_group *groups, const dsa_encoded *encoded,
                                   const uint32_t *encoded_mesh, void *dst, size_t dst_bytes) {
  if (!b) return DSA_ERR_INVALID_ARGUMENT;
  DSA_GUARD(b->ctx, batch_joined_arrays(b, request, num_groups, groups, encoded, encoded_mesh, dst, dst_bytes));
}
const void *dsa_batch_host_joined_arrays(const dsa_batch *b) {
  if (!b || !b->ja_valid || !b->ja_done) return nullptr;
  return !(b->ja_req.arrays.flags & DSA_VA_DEVICE_ONLY) ? b->ja_mirror.p : nullptr;
}
const void *dsa_batch_device_joined_arrays(const dsa_batch *b) {
  if (!b || !b->ja_valid) return nullptr;
  return b->d_ja ? b->d_ja + b->ja_head_bytes : nullptr;
}
dsa_status dsa_batch_joined_member(const dsa_batch *b, uint32_t mesh, uint32_t *group, uint32_t *first_row, uint32_t *num_rows) {
  if (!b) return DSA_ERR_INVALID_ARGUMENT;
  if (!b->ja_valid) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "no joined arrays were requested since the batch was decoded");
  if (mesh >= b->n) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh index %u out of range", (unsigned)mesh);
  if (b->ja_group_of[mesh] < 0) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "mesh %u is in no group of the request", (unsigned)mesh);
  if (group) *group = (uint32_t)b->ja_group_of[mesh];
  if (first_row) *first_row = b->ja_first_row[mesh];
  if (num_rows) *num_rows = b->layouts[mesh].cap_points;
  return DSA_OK;
}
dsa_status dsa_batch_joined_arrays_layout(const dsa_batch *b, uint32_t group, dsa_joined_arrays *out) {
  if (!b || !out) return DSA_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  for (uint32_t a = 0; a < DSA_MAX_ATTRIBUTES; ++a) { out->attributes[a].offset = UINT64_MAX; out->attributes[a].flags = DSA_VA_ABSENT; }
  if (!b->collected) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "results not collected: call dsa_batch_wait");
  if (!b->ja_valid) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "no joined arrays were requested since the batch was decoded");
  if (group >= b->ja_list.size()) return set_err(b->ctx, DSA_ERR_INVALID_ARGUMENT, "group index %u out of range", (unsigned)group);
  const JaGroup &T = b->ja_groups[group];
  out->first_mesh = b->ja_list[group].first_mesh; out->num_meshes = b->ja_list[group].num_meshes; out->num_rows = T.cap_points; out->order = b->ja_req.order;
  if (b->ja_status[group] != DSA_OK) return set_err(b->ctx, (dsa_status)b->ja_status[group], "%s", b->ja_text[group].c_str());
  if (const dsa_status st = ja_group_verdict(b, group)) return st;
  const uint32_t m0 = out->first_mesh;
  const MeshDesc &D = b->descs[m0];
  for (uint32_t a = 0; a < T.cap_attributes && a < DSA_MAX_ATTRIBUTES; ++a) {
    dsa_vertex_attribute &o = out->attributes[a];
    const VaAttr &t = T.att[a];
    o.stride = t.stride; o.data_type = t.data_type; o.num_components = t.nc;
    uint32_t ne = 0;
    if (!va_attr_written(t, D.att[a], b->layouts[m0].out_cap[a], b->layouts[m0].work_cap[a], &ne)) continue;     // the kernel's own test
    o.offset = t.offset; o.flags = 0;
  }
  return DSA_OK;
}

}  // extern "C"
