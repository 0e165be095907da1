// draco-sharp_amd/csrc/dsa_encode_sequential.h  (included by dsa_encode.h behind encode_chunk, whose shared stages it uses)
//
// Encode direction, sequential streams (include/draco_mi355x.h, dsa_encode_sequential_batch): what the reference's encoder
// chooses at speed 10 (DracoEncoder.cs:43-57, :79-82 -> Mesh/MeshSequentialEncoder.cs) and its point-cloud encoder
// (PointCloud/PointCloudSequentialEncoder.cs).  No corner table and no walk: any list of triangles over any set of points,
// coded in the caller's order.  A chunk function of its own on the lanes, chunks and upload turns of dsa_encode.h
// (checks and arena layout: dsa_encode_layout.h, enc_check_sequential_mesh and enc_layout_sequential):
//   host   index and argument checks (threads over meshes); raw indices never travel -- the layout threads narrow them from
//          the caller's array into the stream
//   GPU    k_enc_bounds / k_enc_quantize / k_enc_gather (linear: bounds only) / k_enc_corr   the attributes in point order,
//                                Difference + wrap, canonicalised octahedral delta (Attributes/LinearSequencer.cs: entry i = point i)
//          k_enc_order_*         dsa_encode_ordered_sequential_batch, point_order = 1: the points in Morton order behind the quantisers
//                                (dsa_encode_order.h) -- k_enc_gather then puts every attribute in it, the faces go through its inverse
//          k_enc_merge_*         dsa_encode_merged_sequential_batch, merge_points = 1 (point clouds): one point per cell behind the sort;
//                                nv of the cloud's streams falls on the device, the host reads it from the records that come back
//          k_enc_part_bounds     dsa_encode_split_sequential_batch, part_points >= 1 (point clouds): a set of stream records per part of the
//                                sorted order, and the box of every part's position integers; the host writes a stream per part
//          k_enc_part_cells      dsa_encode_cell_parts_sequential_batch, part_cells >= 1 (point clouds, merge_points = 1): part slots whose
//                                sizes the device writes behind k_enc_merge_scan; the host writes a stream per slot that came back with points
//          k_enc_lod_*           dsa_encode_lod_sequential_batch, lod_base_bits >= 1: the kept rows by (level, kept) and the slots as the parts
//                                of every level, in place of k_enc_part_cells; the host reads the level of every slot from its record
//          k_enc_vote_*          dsa_encode_vote_sequential_batch, vote_attributes != 0: the most frequent tuple of the cell into the voted attributes' integers
//          k_enc_normal_*        dsa_encode_normal_mean_sequential_batch, mean_normals = 1: the mean normal of the cell into the normals' octahedral codes
//          k_enc_voxel_*         dsa_encode_voxel_sequential_batch, voxel_point = nearest: kept[j] the row of voxel j nearest its centre, in front of the cell passes
//          k_enc_mean_*          dsa_encode_mean_sequential_batch, mean_attributes != 0: the mean of the cell into the masked attributes' integers
//                                at every kept row, behind the merge; nothing of it comes back to the host
//          k_enc_seq_indices     compressed indices: symbols and their statistics (dsa_encode_seqidx.h)
//          k_enc_plan / k_enc_rans   every stream, the index stream as a list whose symbols are given (kind 3)
//   host   stream layout (synth::write_sequential_stream)
// The bytes are the CPU coder's (synth::encode_sequential; tests/test_gpu_encode_sequential.py compares them).
#pragma once

// part_points: the streams of the parts of cloud i -- each a point cloud of its own, its quantised attributes on the cloud's grid
// (the first part's records hold the floats) -- and what the handle says of every part
static void enc_write_parts(EncChunk &ck, uint32_t i) {
  const EncLayout &L = ck.L;
  const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
  // (part_cells: the parts the device made of the slots, over the m kept rows; row_entries of all input rows beside them)
  const bool cells = L.cell_parts;
  uint32_t V = ck.mesh(i).num_vertices;
  const uint32_t s0 = L.first_stream[i], na = (uint32_t)atts.size(), rows = V, np = cells ? ck.live_parts(i, &V) : ck.num_parts(i);
  const bool lod = L.lod;
  if (cells && (np == 0 || V == 0 || V > rows || (!lod && np != synth::split_count(V, ck.rq.part_cells)) || ck.row_cells[s0].size() != rows)) return ck.refuse(i, DSA_ERR_DEVICE, "the merged points and their parts did not come back");
  if (ck.entry_rows[s0].size() != V || ck.part_boxes[s0].size() != np) return ck.refuse(i, DSA_ERR_DEVICE, "the point order and the part boxes did not come back");
  // lod_base_bits: the slots are the parts of level 0, then of level 1, ...; the records say which level (EncPart::pad), and the
  // points and parts of a level follow from them -- every level cut by the rule of part_cells, the levels side by side in lod order
  const uint32_t levels = ck.rq.lod_levels();
  std::vector<uint32_t> level_points(levels, 0), level_parts(levels, 0), level_first(levels, 0), level_base(levels, 0);
  if (lod) {
    for (uint32_t p = 0; p < np; ++p) {
      const dsa::EncPart &P = ck.part_boxes[s0][p];
      if (P.pad >= levels || (p && P.pad < ck.part_boxes[s0][p - 1].pad)) return ck.refuse(i, DSA_ERR_DEVICE, "the levels of the parts did not come back");
      if (level_parts[P.pad]++ == 0) { level_first[P.pad] = p; level_base[P.pad] = P.lo; }
      level_points[P.pad] += P.n;
    }
    uint32_t at = 0;
    for (uint32_t l = 0; l < levels; ++l) {
      if (level_parts[l] != synth::split_count(level_points[l], ck.rq.part_cells) || (level_parts[l] && level_base[l] != at)) return ck.refuse(i, DSA_ERR_DEVICE, "the levels of the parts did not come back");
      if (level_parts[l] == 0) { level_base[l] = at; level_first[l] = l ? level_first[l - 1] + level_parts[l - 1] : 0u; }
      at += level_points[l];
    }
  }
  const dsa::EncStream &pos = L.streams[s0];
  std::vector<dsa_encoded::Part> parts(np);
  for (uint32_t p = 0; p < np; ++p) {
    const dsa::EncPart &P = ck.part_boxes[s0][p];
    dsa::EncPart laid = L.parts[L.part_of_mesh[i] + p];
    if (cells && !lod) { laid.lo = synth::split_bound(V, np, p); laid.n = synth::split_bound(V, np, p + 1u) - laid.lo; }
    if (lod) {
      const uint32_t l = P.pad, q = p - level_first[l];
      laid.lo = level_base[l] + synth::split_bound(level_points[l], level_parts[l], q); laid.n = level_base[l] + synth::split_bound(level_points[l], level_parts[l], q + 1u) - laid.lo;
    }
    const uint32_t sp = s0 + p * na;
    if (P.lo != laid.lo || P.n != laid.n || L.streams[sp].nv != P.n || P.n == 0 || P.qmin[0] > P.qmax[0]) return ck.refuse(i, DSA_ERR_DEVICE, "the point order and the part boxes did not come back");
    synth::ByteWriter w;
    try {
      synth::write_sequential_stream(w, false, P.n, 0, false, atts, [](synth::ByteWriter &) {},
        [&](synth::ByteWriter &bw, size_t k) { enc_write_attribute_values(bw, ck, sp + (uint32_t)k, 0); },
        [&](synth::ByteWriter &bw, size_t k) { enc_write_transform(bw, L.streams[s0 + k]); });
    } catch (const std::exception &e) { return ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
    parts[p].stream.swap(w.d);
    dsa_part_info &info = parts[p].info;
    memset(&info, 0, sizeof(info));
    info.input = ck.base + i; info.part = p; info.parts = np; info.first_entry = P.lo; info.num_points = P.n; info.position_bits = pos.bits;
    for (int c = 0; c < 3; ++c) {
      info.qmin[c] = P.qmin[c]; info.qmax[c] = P.qmax[c];
      info.box_min[c] = synth::dequantized(P.qmin[c], pos.qmin[c], pos.qrange, (int)pos.bits);
      info.box_max[c] = synth::dequantized(P.qmax[c], pos.qmin[c], pos.qrange, (int)pos.bits);
    }
    dsa_lod_info &li = parts[p].lod;
    memset(&li, 0, sizeof(li));
    if (!lod) continue;
    li.input = ck.base + i; li.level = P.pad; li.levels = levels; li.cell_bits = ck.rq.lod_base_bits + P.pad;
    li.level_first_stream = level_first[P.pad]; li.level_streams = level_parts[P.pad]; li.level_points = level_points[P.pad]; li.part_in_level = p - level_first[P.pad];
  }
  ck.E->parts[i].swap(parts);
  ck.E->order[i].swap(ck.entry_rows[s0]);
  if (cells) ck.E->cells[i].swap(ck.row_cells[s0]);
}
// the stream layout of a chunk (threads over meshes)
static void enc_stage_sequential_streams(EncChunk &ck) {
  const EncLayout &L = ck.L;
  const bool is_mesh = ck.rq.seq.geometry == 1, compressed = is_mesh && ck.rq.seq.compress_connectivity == 1;
  hostutil::parallel_for(ck.n, [&](uint32_t i) {
    if (!ck.good(i)) return;
    for (uint32_t s = L.first_stream[i]; s < L.first_stream[i + 1]; ++s)
      if (L.streams[s].overflow) return ck.refuse(i, DSA_ERR_INVALID_DATA, "entropy coding failed");
    if (L.split) return enc_write_parts(ck, i);
    const std::vector<synth::PortableAttr> &atts = ck.plans[i].atts;
    const uint32_t s0 = L.first_stream[i], si = s0 + (uint32_t)atts.size();
    const dsa_mesh_input &m = ck.mesh(i);
    // point_order: the permutation came back with the coded pieces; raw indices are laid out through its inverse
    const bool ordered = !L.ord.empty();
    std::vector<uint32_t> ranked;
    if (ordered && is_mesh && !compressed) {
      const std::vector<uint32_t> &perm = ck.entry_rows[s0];
      if (perm.size() != m.num_vertices) return ck.refuse(i, DSA_ERR_DEVICE, "the point order did not come back");
      std::vector<uint32_t> rank(perm.size(), 0);
      for (uint32_t e = 0; e < perm.size(); ++e) if (perm[e] < rank.size()) rank[perm[e]] = e;
      ranked.resize((size_t)m.num_faces * 3);
      for (size_t k = 0; k < ranked.size(); ++k) ranked[k] = rank[m.faces[k]];
    }
    // merge_points: the stream codes the cells the device found (k_enc_merge_scan lowered nv of every stream of the cloud alike)
    const bool merge = L.merge;
    const uint32_t points = merge ? L.streams[s0].nv : m.num_vertices;
    if (merge && (ck.entry_rows[s0].size() != points || ck.row_cells[s0].size() != m.num_vertices || points == 0 || points > m.num_vertices))
      return ck.refuse(i, DSA_ERR_DEVICE, "the merged points did not come back");
    synth::ByteWriter w;
    try {
      synth::write_sequential_stream(w, is_mesh, points, is_mesh ? m.num_faces : 0, compressed, atts,
        [&](synth::ByteWriter &bw) {               // (raw indices never travel: narrowed from the caller's array into the stream)
          if (compressed) enc_put_coded(bw, ck.splans[si], ck.rans[si], ck.bits[si], L.streams[si].method);
          else synth::write_raw_indices(bw, ordered ? ranked.data() : m.faces, (size_t)m.num_faces * 3, m.num_vertices);
        },
        [&](synth::ByteWriter &bw, size_t k) { enc_write_attribute_values(bw, ck, s0 + (uint32_t)k, 0); },      // Difference
        [&](synth::ByteWriter &bw, size_t k) { enc_write_transform(bw, L.streams[s0 + k]); });
    } catch (const std::exception &e) { return ck.refuse(i, DSA_ERR_INVALID_DATA, e.what()); }
    ck.E->streams[i].swap(w.d);
    if (ordered) ck.E->order[i].swap(ck.entry_rows[s0]);
    if (merge) { ck.E->linear[i].second = points; ck.E->cells[i].swap(ck.row_cells[s0]); }
  });
}
// Meshes base .. base + count of a sequential request on a lane, through the stages it shares with encode_chunk.  No stage waits for
// part of the input: one turn on the link for all of it (enc_stage_uploads).  The symbol plans by the host below 256 meshes, as there.
static dsa_status encode_sequential_chunk(dsa_context *ctx, EncLane &lane, const EncRequest &rq, uint32_t base, uint32_t count, uint32_t batch_n, dsa_encoded **out) {
  hostutil::TurnGuard turn(lane.upload_turn, lane.upload_chunk);
  HIP_TRY(ctx, hipSetDevice(lane.device));
  EncChunk ck(rq, base, count, batch_n);
  if (!ck.E) return set_err(ctx, DSA_ERR_OUT_OF_MEMORY, "host allocation failed");
  ck.E->ctx = ctx;
  ck.host_plan = enc_host_choice("DSA_ENC_HOST_PLAN", batch_n);
  hostutil::parallel_for(count, [&](uint32_t i) { enc_check_sequential_mesh(ck, i); });
  enc_layout_sequential(ck);
  for (uint32_t i = 0; i < count; ++i) if (ck.good(i)) ck.E->linear[i] = {(uint32_t)ck.plans[i].atts.size(), ck.mesh(i).num_vertices};      // (dsa_encoded_entry_rows: entry i is row i)
  if (!ck.L.streams.empty()) {
    ENC_STAGE(enc_stage_uploads(ctx, lane, turn, ck));
    ENC_STAGE(enc_stage_attributes(ctx, lane, ck));
    ENC_STAGE(enc_stage_code(ctx, lane, ck, nullptr));
  }
  enc_stage_sequential_streams(ck);
  *out = ck.E.release();
  return DSA_OK;
}
