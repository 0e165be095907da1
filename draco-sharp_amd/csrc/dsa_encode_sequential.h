// draco-sharp_amd/csrc/dsa_encode_sequential.h  (included at the end of dsa_encode.h)
//
// Encode direction, sequential streams (include/draco_mi355x.h, dsa_encode_sequential_batch): what the reference's encoder
// chooses at speed 10 (DracoEncoder.cs:43-57, :79-82 -> Mesh/MeshSequentialEncoder.cs) and its point-cloud encoder
// (PointCloud/PointCloudSequentialEncoder.cs).  No corner table and no walk: any list of triangles over any set of points,
// coded in the caller's order.  A chunk function of its own on the lanes, chunks and upload turns of dsa_encode.h:
//   host   index and argument checks (threads over meshes); raw indices never travel -- the layout threads narrow them from
//          the caller's array into the stream
//   GPU    k_enc_bounds / k_enc_quantize / k_enc_gather (linear: bounds only) / k_enc_corr   the attributes in point order,
//                                Difference + wrap, canonicalised octahedral delta (Attributes/LinearSequencer.cs: entry i = point i)
//          k_enc_seq_indices     compressed indices: symbols and their statistics (dsa_encode_seqidx.h)
//          k_enc_plan / k_enc_rans   every stream, the index stream as a list whose symbols are given (kind 3)
//   host   stream layout (synth::write_sequential_stream)
// The bytes are the CPU coder's (synth::encode_sequential; tests/test_gpu_encode_sequential.py compares them).
#pragma once

#include "dsa_encode_seqidx.h"

// `attrs` (dsa_encode_attributes_sequential_batch): meshes with an attribute list, `meshes_v` null.
static dsa_status encode_sequential_chunk(dsa_context *ctx, EncLane &lane, uint32_t n, uint32_t batch_n, const dsa_mesh_input *meshes_v, const dsa_mesh_attr_input *attrs, const dsa_encode_sequential_options &so, dsa_encoded **out) {
  struct MeshRef {
    const dsa_mesh_input *v; const dsa_mesh_attr_input *a;
    const dsa_mesh_input &operator[](size_t i) const { return a ? a[i].mesh.mesh : v[i]; }
  } meshes{meshes_v, attrs};
  std::vector<std::vector<synth::ExtraAttr>> extras(attrs ? n : 0);
  std::vector<std::vector<uint32_t>> extra_cap(attrs ? n : 0);      // per attribute: hist_cap of an integer extra, else 0
  hostutil::TurnGuard turn(lane.upload_turn, lane.upload_chunk);
  HIP_TRY(ctx, hipSetDevice(lane.device));
  const dsa_encode_options &od = so.base;
  const bool is_mesh = so.geometry == 1, compressed = is_mesh && so.compress_connectivity == 1;
  synth::Options opt;
  opt.pos_bits = od.position_bits; opt.uv_bits = od.texcoord_bits; opt.normal_bits = od.normal_bits;
  opt.force_scheme = od.symbol_scheme; opt.compression_level = od.compression_level;
  dsa_encoded *E = new (std::nothrow) dsa_encoded();
  if (!E) return set_err(ctx, DSA_ERR_OUT_OF_MEMORY, "host allocation failed");
  std::unique_ptr<dsa_encoded> E_owner(E);
  E->ctx = ctx;
  E->streams.resize(n); E->status.assign(n, DSA_OK); E->messages.resize(n);
  // the symbol plans by the host below 256 meshes, as in encode_chunk (DSA_ENC_HOST_PLAN = 1 or 0 forces one or the other)
  const bool host_plan = [&]() { const char *e = getenv("DSA_ENC_HOST_PLAN"); return e ? atoi(e) != 0 : batch_n < 256; }();
  // ---- host checks: everything the kernels index by
  std::vector<synth::MeshIn> ins(n);
  std::vector<std::vector<synth::PortableAttr>> atts(n);
  hostutil::parallel_for(n, [&](uint32_t i) {
    const dsa_mesh_input &m = meshes[i];
    auto refuse = [&](dsa_status st, const char *why) { E->status[i] = st; E->messages[i] = why; };
    if (!m.positions || m.num_vertices == 0) return refuse(DSA_ERR_INVALID_DATA, "positions are missing");
    if (!is_mesh && m.num_faces != 0) return refuse(DSA_ERR_INVALID_ARGUMENT, "a point cloud has no faces (geometry = 0, num_faces != 0)");
    if (is_mesh && (m.num_faces == 0 || !m.faces)) return refuse(DSA_ERR_INVALID_DATA, "a mesh needs faces");
    if (m.generic && (m.generic_components < 1 || m.generic_components > 4)) return refuse(DSA_ERR_INVALID_ARGUMENT, "generic attribute needs 1 - 4 components");
    if (attrs && (attrs[i].mesh.normal_corners || attrs[i].mesh.texcoord_corners))
      return refuse(DSA_ERR_INVALID_ARGUMENT, "corner ids with a sequential stream: it has one value per point (normal_corners / texcoord_corners must be NULL)");
    // (what the 32-bit sizes of a stream's regions hold: 4 bytes per component and symbol, and a margin)
    if (m.num_vertices > (1u << 28) || (compressed && m.num_faces > (1u << 28))) return refuse(DSA_ERR_INVALID_DATA, "mesh too large for the device coder");
    if (is_mesh) {
      uint32_t top = 0;
      for (size_t k = 0, nk = (size_t)m.num_faces * 3; k < nk; ++k) top = m.faces[k] > top ? m.faces[k] : top;
      if (top >= m.num_vertices) return refuse(DSA_ERR_INVALID_DATA, "face index out of range");
    }
    synth::MeshIn &in = ins[i];
    in.pos = m.positions; in.nv = m.num_vertices; in.faces = is_mesh ? m.faces : nullptr; in.nf = is_mesh ? m.num_faces : 0;
    in.normals = m.normals; in.uvs = m.texcoords; in.generic = m.generic;
    synth::Options mo = opt;
    mo.generic_components = m.generic ? (int32_t)m.generic_components : 1;
    if (attrs) {
      const std::string why = enc_take_extras(attrs[i], extras[i], in);
      if (!why.empty()) { E->status[i] = DSA_ERR_INVALID_ARGUMENT; E->messages[i] = why; return; }
    }
    synth::plan_sequential_attributes(in, mo, atts[i]);
    if (attrs) {
      extra_cap[i].assign(atts[i].size(), 0);
      for (size_t k = 0; k < atts[i].size(); ++k)
        if (atts[i][k].extra_values && atts[i][k].seq_type == 1) extra_cap[i][k] = enc_extra_hist_cap(atts[i][k], m.num_vertices);
    }
  });
  // ---- device layout: what the host provides (attribute values; the faces of compressed indices, 16-bit where every index fits) in
  // one run at the front of the arena, everything else behind it
  std::vector<dsa::EncStream> hs;
  std::vector<dsa::EncSeqIdx> hx;
  std::vector<uint32_t> first_stream(n + 1, 0);
  auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
  uint64_t in_total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (E->status[i] != DSA_OK) continue;
    const uint64_t V = meshes[i].num_vertices, F = meshes[i].num_faces;
    if (compressed) in_total += al((V <= 65536 ? 6 : 12) * F);
    for (const synth::PortableAttr &a : atts[i]) in_total += al((a.seq_type == 1 ? (uint64_t)synth::data_type_size(a.data_type) : 4ull) * V * (uint64_t)a.nc_out);
  }
  uint64_t cur = in_total, cur_in = 0;
  auto take = [&](uint64_t bytes) { uint64_t at = cur; cur = (cur + bytes + 255) & ~255ull; return at; };
  auto take_in = [&](uint64_t bytes) { uint64_t at = cur_in; cur_in = (cur_in + bytes + 255) & ~255ull; return at; };
  std::vector<EncUpload> uploads;
  uint32_t max_rows = 0, max_count = 0;
  for (uint32_t i = 0; i < n; ++i) {
    first_stream[i] = (uint32_t)hs.size();
    if (E->status[i] != DSA_OK) continue;
    const uint32_t V = meshes[i].num_vertices;
    for (size_t k = 0; k < atts[i].size(); ++k) {
      const synth::PortableAttr &a = atts[i][k];
      dsa::EncStream S;
      memset(&S, 0, sizeof(S));
      const bool integer = a.seq_type == 1;
      const void *src = a.extra_values ? a.extra_values
                        : (a.att_type == 0 ? (const void *)meshes[i].positions : (a.att_type == 1 ? (const void *)meshes[i].normals : (integer ? (const void *)meshes[i].generic : (const void *)meshes[i].texcoords)));
      S.nv = S.rows = V; S.nc_out = (uint32_t)a.nc_out; S.nc = (uint32_t)a.nc; S.kind = a.seq_type == 3 ? 1u : (integer ? 2u : 0u);
      S.bits = integer ? 9u : (uint32_t)a.bits; S.prediction = 0; S.linear = 1;
      S.elem = integer ? (uint32_t)a.data_type : 0u;
      const uint64_t src_bytes = (integer ? (uint64_t)synth::data_type_size(a.data_type) : 4ull) * V * S.nc_out;
      S.src = take_in(src_bytes);
      uploads.push_back({S.src, src, (size_t)src_bytes, false});
      S.vals = S.d = take(4ull * V * S.nc);                   // linear order: the values are the entries
      S.syms = take(4ull * V * S.nc); S.bl = take(V);
      max_rows = std::max(max_rows, V);
      S.hist_cap = (1u << S.bits) + 2u;
      if (attrs && extra_cap[i][k]) S.hist_cap = extra_cap[i][k];       // an integer extra: by the values present
      S.hist_raw = take(4ull * S.hist_cap);
      S.out_cap = 4u * V * S.nc + 16u;
      S.out_rans = take(S.out_cap); S.out_bits = take(S.out_cap);
      const uint64_t table_cap = std::max<uint64_t>(S.hist_cap, 64);
      S.prob = take(4ull * table_cap); S.cum = take(4ull * table_cap);
      S.plan_order = take(4ull * table_cap); S.plan_tmp = take(4ull * table_cap);
      hs.push_back(S);
    }
    if (!compressed) continue;
    // the index stream behind the attributes': 3F symbols below 2V, given by k_enc_seq_indices
    const uint32_t count = 3u * meshes[i].num_faces;
    const bool narrow = V <= 65536;
    dsa::EncSeqIdx X;
    memset(&X, 0, sizeof(X));
    X.count = count; X.narrow = narrow ? 1u : 0u; X.stream = (uint32_t)hs.size();
    X.faces = take_in((narrow ? 2ull : 4ull) * count);
    uploads.push_back({X.faces, meshes[i].faces, (size_t)((narrow ? 2ull : 4ull) * count), narrow});
    hx.push_back(X);
    max_count = std::max(max_count, count);
    dsa::EncStream S;
    memset(&S, 0, sizeof(S));
    S.kind = 3; S.nc = S.nc_out = 1; S.nv = count;
    S.hist_cap = 2u * V;
    S.hist_raw = take(4ull * S.hist_cap);
    S.syms = take(4ull * count); S.bl = take(count);
    S.out_cap = 4u * count + 16u;
    S.out_rans = take(S.out_cap); S.out_bits = take(S.out_cap);
    const uint64_t table_cap = std::max<uint64_t>(S.hist_cap, 64);
    S.prob = take(4ull * table_cap); S.cum = take(4ull * table_cap);
    S.plan_order = take(4ull * table_cap); S.plan_tmp = take(4ull * table_cap);
    hs.push_back(S);
  }
  first_stream[n] = (uint32_t)hs.size();
  const uint32_t ns = (uint32_t)hs.size(), nx = (uint32_t)hx.size();
  std::vector<int> stream_mesh(ns, 0);
  for (uint32_t i = 0; i < n; ++i) for (uint32_t s = first_stream[i]; s < first_stream[i + 1]; ++s) stream_mesh[s] = (int)i;
  std::vector<synth::SymbolPlan> splans(ns);
  std::vector<std::vector<uint8_t>> rans(ns), bits(ns), flag_bits(ns);
  if (ns) {
    hipStream_t st = lane.st;
    ENC_TRY(lane.arena.ensure(cur ? cur : 256));
    ENC_TRY(lane.streams.ensure(sizeof(dsa::EncStream) * ns));
    uint8_t *arena = (uint8_t *)lane.arena.p;
    dsa::EncStream *d_streams = (dsa::EncStream *)lane.streams.p;
    if (lane.walk_st) ENC_TRY(hipStreamSynchronize(lane.walk_st));     // (idle unless a previous chunk on this lane ended in an error)
    ENC_TRY(hipMemsetAsync(arena, 0, cur, st));              // histograms start at zero
    // no stage waits for part of the input: one turn on the link for all of it
    turn.acquire_a();
    ENC_TRY(enc_upload(lane, arena, st, uploads));
    turn.release();
    ENC_TRY(hipMemcpyAsync(d_streams, hs.data(), sizeof(dsa::EncStream) * ns, hipMemcpyHostToDevice, st));
    const uint32_t gx = std::max(1u, std::min(64u, (max_rows + 2047) / 2048));
    hipLaunchKernelGGL(dsa::k_enc_bounds, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
    hipLaunchKernelGGL(dsa::k_enc_quantize, dim3(gx, ns), dim3(256), 0, st, arena, d_streams, ns);
    hipLaunchKernelGGL(dsa::k_enc_gather, dim3(ns), dim3(256), 0, st, arena, d_streams, ns);
    hipLaunchKernelGGL(dsa::k_enc_corr, dim3(gx, ns), dim3(256), 0, st, arena, d_streams, ns);
    if (nx) {
      ENC_TRY(lane.conns.ensure(sizeof(dsa::EncSeqIdx) * nx));
      dsa::EncSeqIdx *d_idx = (dsa::EncSeqIdx *)lane.conns.p;
      ENC_TRY(hipMemcpyAsync(d_idx, hx.data(), sizeof(dsa::EncSeqIdx) * nx, hipMemcpyHostToDevice, st));
      const uint32_t gi = std::max(1u, std::min(64u, (max_count + SEQ_SYMBOLS_PER_BLOCK - 1) / SEQ_SYMBOLS_PER_BLOCK));
      hipLaunchKernelGGL(dsa::k_enc_seq_indices<dsa::EncStream>, dim3(gi, nx), dim3(SEQ_BLOCK), 0, st, arena, d_idx, nx, d_streams);
    }
    if (!host_plan) {
      hipLaunchKernelGGL(dsa::k_enc_plan, dim3((ns + WAVE - 1) / WAVE), dim3(WAVE), 0, st, arena, d_streams, ns, (int)opt.force_scheme, (int)opt.compression_level);
      hipLaunchKernelGGL(dsa::k_enc_rans, dim3(ns), dim3(WAVE), 0, st, arena, d_streams, ns);
    }
    ENC_TRY(hipGetLastError());
    ENC_TRY(hipMemcpyAsync(hs.data(), d_streams, sizeof(dsa::EncStream) * ns, hipMemcpyDeviceToHost, st));
    ENC_TRY(hipStreamSynchronize(st));
    if (host_plan) { const dsa_status ps = enc_host_plans(ctx, lane, arena, hs, stream_mesh, E, opt, splans); if (ps != DSA_OK) return ps; }
    else enc_device_plan_errors(hs, stream_mesh, E);
    const dsa_status cs = enc_code_streams(ctx, lane, arena, d_streams, hs, stream_mesh, E, host_plan, splans, rans, bits, flag_bits);
    if (cs != DSA_OK) return cs;
  }
  // ---- stream layout (threads over meshes)
  hostutil::parallel_for(n, [&](uint32_t i) {
    if (E->status[i] != DSA_OK) return;
    for (uint32_t s = first_stream[i]; s < first_stream[i + 1]; ++s)
      if (hs[s].overflow) { E->status[i] = DSA_ERR_INVALID_DATA; E->messages[i] = "entropy coding failed"; return; }
    const uint32_t s0 = first_stream[i], si = s0 + (uint32_t)atts[i].size();
    const dsa_mesh_input &m = meshes[i];
    synth::ByteWriter w;
    try {
      synth::write_sequential_stream(w, is_mesh, m.num_vertices, is_mesh ? m.num_faces : 0, compressed, atts[i],
        [&](synth::ByteWriter &bw) {
          if (compressed) enc_put_coded(bw, splans[si], rans[si], bits[si], hs[si].method);
          else synth::write_raw_indices(bw, m.faces, (size_t)m.num_faces * 3, m.num_vertices);
        },
        [&](synth::ByteWriter &bw, size_t k) {               // SequentialIntegerAttributeEncoder.cs:55-128, Difference
          const dsa::EncStream &S = hs[s0 + k];
          bw.i8(0); bw.i8(S.kind == 1 ? 3 : 1);
          bw.u8(1);
          enc_put_coded(bw, splans[s0 + k], rans[s0 + k], bits[s0 + k], S.method);
          if (S.kind == 1) { const int32_t max_q = (1 << S.bits) - 1; bw.i32(max_q); bw.i32((max_q - 1) / 2); }
          else { bw.i32(S.wrap_mn); bw.i32(S.wrap_mx); }
        },
        [&](synth::ByteWriter &bw, size_t k) {
          const dsa::EncStream &S = hs[s0 + k];
          if (S.kind == 0) { for (uint32_t c = 0; c < S.nc_out; ++c) bw.f32(S.qmin[c]); bw.f32(S.qrange); bw.u8((uint8_t)S.bits); }
          else if (S.kind == 1) bw.u8((uint8_t)S.bits);
        });
    } catch (const std::exception &e) { E->status[i] = DSA_ERR_INVALID_DATA; E->messages[i] = e.what(); return; }
    E->streams[i].swap(w.d);
  });
  *out = E_owner.release();
  return DSA_OK;
}

extern "C" {

void dsa_encode_sequential_default_options(dsa_encode_sequential_options *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  dsa_encode_default_options(&o->base);
  o->geometry = 1;
  o->compress_connectivity = 0;
}

static dsa_status encode_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes, const dsa_mesh_attr_input *attrs, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  if (!ctx || !out || (n && !meshes && !attrs)) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "null argument");
  dsa_encode_sequential_options d;
  dsa_encode_sequential_default_options(&d);
  if (options) d = *options;
  // (the prediction fields of `base` do not shape a sequential stream; values dsa_encode_batch refuses are refused all the same)
  if (check_schemes(ctx, &d.base, nullptr) != DSA_OK) return DSA_ERR_INVALID_ARGUMENT;
  if (d.base.position_bits < 1 || d.base.position_bits > 20 || d.base.texcoord_bits < 1 || d.base.texcoord_bits > 20 || d.base.normal_bits < 2 || d.base.normal_bits > 20)
    return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "quantisation bits out of range (positions/texcoords 1..20, normals 2..20)");
  if (d.geometry != 0 && d.geometry != 1)
    return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "geometry %d: 1 (triangular mesh) or 0 (point cloud)", (int)d.geometry);
  if (d.compress_connectivity != 0 && d.compress_connectivity != 1)
    return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "compress_connectivity %d: 0 (raw indices) or 1 (compressed)", (int)d.compress_connectivity);
  for (int k = 0; k < 6; ++k)
    if (d.reserved[k] != 0) return set_err(ctx, DSA_ERR_INVALID_ARGUMENT, "dsa_encode_sequential_options.reserved[%d] is not zero", k);
  DSA_GUARD(ctx, encode_batch_chunks(ctx, n, [&](dsa_context *sink, EncLane &lane, uint32_t base, uint32_t cnt, dsa_encoded **part) {
    return encode_sequential_chunk(sink, lane, cnt, n, meshes ? meshes + base : nullptr, attrs ? attrs + base : nullptr, d, part);
  }, out));
}

dsa_status dsa_encode_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_input *meshes, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  return encode_sequential_batch(ctx, n, meshes, nullptr, options, out);
}
dsa_status dsa_encode_attributes_sequential_batch(dsa_context *ctx, uint32_t n, const dsa_mesh_attr_input *meshes, const dsa_encode_sequential_options *options, dsa_encoded **out) {
  return encode_sequential_batch(ctx, n, nullptr, meshes, options, out);
}

}  // extern "C"
