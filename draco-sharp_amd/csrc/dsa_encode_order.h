// draco-sharp_amd/csrc/dsa_encode_order.h  (included by dsa_encode_layout.h, whose layout hands out the regions below)
//
// Encode direction, dsa_encode_ordered_sequential_batch with point_order = 1: the points of every sequential stream of a chunk in
// Morton order of their quantised positions.  With q[r][c] the integer the position stream codes for component c of row r (the
// `vals` k_enc_quantize / k_enc_grid_quantize wrote) and B = position_bits,
//     key(r) = sum over b < B, c < 3 of ((uint32(q[r][c]) >> b) & 1) << (3 b + 2 - c)        (x the top bit of each triple)
// and perm lists the rows in ascending (key, row): entry e of every attribute of the stream carries row perm[e], a face index f is
// written rank[f], rank the inverse of perm.  Only the low B bits of an integer are read, so whatever the quantiser left of a cloud
// the host refuses behind this stage (a value that is not finite, a range the bits cannot carry) still gives a permutation.  The host coder's twin is synth::point_order
// (dsa_encode_host.h); tests/hostcheck/encorder_host.cpp holds the two against each other under the sanitizers.
//
// A segmented, stable, least-significant-digit radix sort of (key, row) over all clouds of the chunk at once: 8 bits a pass,
// ceil(3 B / 8) passes (11 bits: 5, 20 bits: 8), keys and rows in double buffers.  The grid of every step is the chunk's list of
// (cloud, tile) pairs, a tile ORD_TILE consecutive entries of one cloud, so that a launch covers clouds of one point and of millions
// side by side and nothing is launched per cloud:
//   k_enc_order_keys      a thread per point: the key by shift-and-mask spreading (no loop over bits), row = its index
//   per pass
//   k_enc_order_hist      a wave per tile: the digits of its entries counted in LDS (counts do not depend on who adds first),
//                         written to hist[digit * tiles + tile] of the cloud
//   k_enc_order_scan      a wave per cloud: exclusive scan of its histogram in (digit, tile) order -- where every (digit, tile) starts
//   k_enc_order_scatter   a wave per tile, 64 consecutive entries a step in entry order: the lanes of equal digit find each other by
//                         8 ballots, a lane's place is the tile's running count of its digit (LDS, read by all, advanced by the
//                         lowest lane of each digit) plus the lanes of its digit below it.  No atomic decides a place: the
//                         sort is stable, ties go to the smaller row, the order is a function of the input alone.
//   k_enc_order_rank      meshes: rank[perm[e]] = e
//   k_enc_order_faces     compressed indices: the faces in the arena through rank, in front of k_enc_seq_indices (raw indices are
//                         laid out by the host from the perm that comes back among the chunk's packed pieces)
// The last pass writes the rows into the region the cloud's streams read as their entry -> row map (EncStream::e2v, linear = 0):
// k_enc_gather behind it puts every attribute in the order.  Nothing between the quantisers and k_enc_gather goes through the host.
// Every cloud fits the same three steps a pass; a one-workgroup LDS sort for clouds of one tile was not built (DESIGN.md 7.3 has
// what the crowded batch of small clouds costs).
// The order of all steps of this file -- the sort, then the merge, the means, the votes, the mean normals, the levels, the part sizes and the part boxes where the
// request has them (merge, nearest pick, means with the centroids, votes, normals, levels, slot sizes, boxes) -- is written down once, in enc_order_stage (dsa_encode_layout.h), which the product and every host check run.
// Which buffer of a pair a step reads follows from EncOrder::last alone (ord_sorted, ord_kept, ord_part_rows below).
//
// Wave64 throughout: the tile steps are blocks of one wave (__launch_bounds__(64)), so their barriers order LDS within a wave and
// many tiles share a CU.  gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_order_keys 16 / 26 / 0, hist 11 / 34 /
// 1024, scan 26 / 24 / 0, scatter 16 / 57 / 1024, rank 6 / 19 / 0, faces 8 / 21 / 0; no scratch, no spills, 8 waves per SIMD.
// The host check runs a grid thread by thread, where lanes cannot meet: the three wave steps have a serial form for it (lane 0
// does the tile's or the cloud's work in entry order, as k_enc_weld_scan has) -- records, tile list, regions, pass structure, keys,
// rank and remap are the product's as they run; the ballots and shuffles themselves are held to the host coder by
// tests/test_gpu_encode_order.py alone.
//
// dsa_encode_merged_sequential_batch with merge_points = 1 (point clouds): one point per occupied cell of the position grid.  The
// cell of a point is its key, and behind the sort the points of a cell are adjacent: entry e of the sorted order is a head iff
// e == 0 or key[perm[e]] != key[perm[e - 1]]; kept lists perm[e] over the heads in sorted order, m of them (the sort is stable:
// kept[j] is the smallest row of its cell, with voxel_bits = 0), and row_entries[r] is the j whose cell row r lies in.  Three steps behind the last
// scatter pass and in front of k_enc_gather, on the same (cloud, tile) list:
//   k_enc_merge_heads     a wave per tile: head flags from the sorted keys (entry e0 of a tile reads key[e0 - 1] of the tile in
//                         front: the sorted buffers are only read from here on), a ballot and a popcount per 64 entries, the
//                         tile's head count to hist[tile] (the histograms are done with)
//   k_enc_merge_scan      a wave per cloud: exclusive scan of the tile counts (the shuffle scan of k_enc_order_scan), m into the
//                         cloud's record and into nv of every stream of the cloud in the device's EncStream records -- what
//                         k_enc_gather and everything behind it read, and what the host reads when the records come back
//   k_enc_merge_compact   a wave per tile: kept[tile base + heads below me] = row[e] for heads, row_entries[row[e]] = the head at or
//                         before e for every entry; lane offsets from the ballots, a running count over the tile's 16 steps.  Not
//                         in place (tile t writes at or below t * ORD_TILE, into the range an earlier tile may not have read yet):
//                         kept goes to the other row buffer (ord_kept), which the layout makes the streams' e2v.
// No atomic decides a place: kept and row_entries are functions of the input alone.  The host coder's twin is synth::merge_points;
// tests/hostcheck/encmerge_host.cpp runs the serial forms against it, tests/test_gpu_encode_merge.py the ballots and shuffles.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_merge_heads 12 / 25 / 0, scan 16 / 29 / 0, compact 14 / 27 / 0; no
// scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_split_sequential_batch with part_points = N >= 1 (point clouds, no merge): the sorted order of a cloud cut into P =
// ceil(n / N) parts, part p sorted entries [floor(p n / P), floor((p + 1) n / P)), each coded as a stream of its own.  Sizes are the
// host's to know before anything runs: the layout gives every part its own set of EncStream records whose e2v is the cloud's sorted
// row buffer at 4 lo_p and whose nv is the part's size, on the cloud's one `src` and `vals` (quantised once: EncStream::part), and
// k_enc_gather and everything behind it run per part as they are.  One step of this file's own, behind the last scatter pass:
//   k_enc_part_bounds     a wave per (part, tile) pair of a list the layout builds, a tile up to ORD_TILE consecutive entries of one
//                         part, so that parts of one point and of a million share a launch: per component the minimum and maximum of
//                         vals[3 row[e] + c] over the tile, a wave reduction by shuffles, then an integer atomicMin / atomicMax of
//                         lane 0 into the part's record (EncPart, which the layout initialises).  Minimum and maximum commute: the
//                         result is a function of the input alone, and here too no atomic decides a place.  No loop waits on
//                         another block.
// The records leave the device among the chunk's packed pieces, as perm does.  The host coder's twin is synth::split_parts /
// synth::part_boxes; tests/hostcheck/encsplit_host.cpp runs the serial form against it, tests/test_gpu_encode_split.py the shuffles.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_part_bounds 18 / 22 / 0; no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_cell_parts_sequential_batch with part_cells = N >= 1 (point clouds, merge_points = 1): the KEPT order of a cloud -- m
// entries, a number the host does not know -- cut into P = ceil(m / N) parts, part p kept entries [floor(p m / P), floor((p + 1) m /
// P)).  The host can only bound P by P_max = ceil(n / N): the layout lays out P_max part slots per cloud, each with its EncPart
// record, its set of EncStream records, regions for min(N, n) points and (part, tile) pairs for as many, and one step sizes them:
//   k_enc_part_cells      a thread per slot, behind k_enc_merge_scan (which knows m) and in front of k_enc_part_bounds and
//                         k_enc_gather: P, lo_p and n_p from m and N of the cloud's record in 64 bits, lo / n into the slot's
//                         EncPart, nv = n_p and e2v = kept + 4 lo_p into every EncStream of the slot; a slot p >= P gets n = nv = 0
//                         and kind 3 (k_enc_merge_scan's nv = m lands in slot 0's records only, which this step writes too).  No lane needs
//                         another: the kernel has no shuffle, no LDS, no atomic, waits for nothing, and the host check runs it
//                         thread by thread as it stands.  Every value is a function of the input alone.
// k_enc_part_bounds then reads lo / n from the records on the device and the kept buffer in place of the sorted one (EncOrder::merge
// says so); the tiles of a slot beyond its size return at once.  A slot with nv = 0 is an empty value stream, which only this layout
// makes: its records carry ENC_PART_SIZED (dsa_encode_layout.h), and k_enc_part_cells makes them empty lists (kind 3), which
// k_enc_gather, k_enc_corr, k_enc_plan, k_enc_rans and the host's plans pass by as they are, without touching a region; the piece
// packer skips them by the flag.  P and the sizes come back in the stream records at the end of the stage, as m does for the merge.
// The host coder's twin is synth::cell_parts; tests/hostcheck/enccellparts_host.cpp runs the steps in the product's layout against
// it, tests/test_gpu_encode_cell_parts.py the device's.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_part_cells 44 / 23 / 0 (the walk over the levels); no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_lod_sequential_batch with lod_base_bits = D >= 1 (point clouds, merge_points = 1, part_cells = N >= 1): additive levels
// of detail of the kept points.  The kept keys are distinct and ascending; with c(j) the leading bit-triples, out of B = bits, that
// key(kept[j]) and key(kept[j - 1]) share -- c = B - ceil(bitlength(key[j] ^ key[j - 1]) / 3) -- level(0) = 0 and level(j) = max(0,
// c(j) + 1 - D), L = B - D + 1 <= ORD_LOD_LEVELS levels.  Levels 0 .. l together are one point per occupied cell of the grid with D + l
// bits per axis, the cell's first point in Morton order.  lod is kept in ascending (level, position in kept); level l, m_l points from
// base_l on, is cut by the rule of part_cells applied to m_l, and the slots of a cloud are the parts of level 0, then of level 1, ...
// (an empty level has none).  sum ceil(m_l / N) <= ceil(m / N) + (non-empty levels - 1): the layout lays out ceil(n / N) + L - 1 slots.
// Four steps behind the merge, in front of k_enc_part_cells, k_enc_part_bounds and k_enc_gather, on the merge's
// (cloud, tile) list with tiles over KEPT entries (a tile at or beyond m returns at once):
//   k_enc_lod_levels      a wave per tile: the level of every kept entry of the tile from ord_key of vals at kept[j] and kept[j - 1]
//                         (entry 0 of a tile reads the last kept row of the tile in front: kept is only read from here on), kept in
//                         pos[j] for the scatter; the tile's count per level by one ballot a level, to hist[level * tiles + tile]
//                         (the histograms are done with, and L <= 20 fits the 256 digits)
//   k_enc_lod_scan        a wave per cloud: exclusive scan of the counts in (level, tile) order over the tiles that hold kept
//                         entries (the shuffle scan of k_enc_merge_scan), then m_l and base_l of every level into the cloud's
//                         EncLodTable, a record of the kernels' own beside the cloud's
//   k_enc_lod_scatter     a wave per tile, 64 consecutive entries a step in entry order: the lanes of equal level find each other by
//                         5 ballots, a lane's place is the (level, tile) start plus the tile's running count of the level (LDS) plus
//                         the lanes of its level below it, as in k_enc_order_scatter; lod[place] = kept[j], pos[j] = place.  Not in
//                         place: lod and pos are the two u32[n] of the key buffer the last sort pass did not write, dead behind the
//                         merge (EncOrder::lod_rows).  No atomic decides a place: the result is a function of the input alone.
//   k_enc_lod_cells       a thread per input row: cells[r] = pos[cells[r]], row_entries from kept order to lod order
// and k_enc_part_cells behind them, the one slot sizer: for such a cloud a thread walks the at most 20 level counts of the table to
// its level and part, writes lo / n into the slot's EncPart and the level into its pad word, nv and e2v = lod + 4 lo into every
// EncStream of the slot; a slot beyond the live ones gets n = nv = 0 and kind 3.  A cloud without levels is the same walk over one
// level of m entries from 0 on, read from the cloud's record (it has no table).
// k_enc_part_bounds reads the lod buffer for such clouds (EncOrder::lod_bits says so).  k_enc_gather, k_enc_corr, k_enc_plan and
// k_enc_rans are untouched: an empty slot goes through the ENC_PART_SIZED / kind 3 path of part_cells.  The host reads levels and
// sizes from the EncPart records that come back and holds them to the rule (enc_write_parts).  The host coder's twin is
// synth::lod_parts; tests/hostcheck/enclod_host.cpp runs the serial forms in the product's layout against it,
// tests/test_gpu_encode_lod.py the ballots and shuffles.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_lod_levels 24 / 35 / 0, scan 22 / 37 / 0, scatter 14 / 44 / 128, cells
// 6 / 20 / 0 (k_enc_part_bounds stays 18 / 22 / 0); no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_mean_sequential_batch with mean_attributes != 0 (point clouds, merge_points = 1): entry j of a masked attribute carries
// mean = floor((2 S + cnt) / (2 cnt)), S the sum over the cnt rows of cell j of the integer the plain call codes for the row, in 64
// bits -- the exact mean, ties toward +infinity, a function of the set of rows.  The mean is written into the stream's `vals` at row
// kept[j], which is what k_enc_gather and everything behind it read: merged streams, cell parts and levels take it as they are (the
// part streams of a cloud share the first part's vals).  Two steps behind the merge and in front of k_enc_lod_*
// (which turn cells[] into lod order), k_enc_part_cells, k_enc_part_bounds and k_enc_gather, on the merge's (cloud, tile) list with the cloud's masked
// streams in blockIdx.y (a cloud has at most DSA_MAX_ATTRIBUTES streams: one launch, no slices); launched only when the chunk has
// a masked stream:
//   k_enc_mean_sum        a wave per (tile, masked stream), 64 sorted entries a step: head flags from the sorted keys as
//                         k_enc_merge_compact makes them; per component a segmented inclusive sum of vals[nc row[e] + c] across the
//                         wave in int64 by shuffles, a lane adding what lies d below only while that is inside its run (the run's
//                         first lane of the step from one ballot and a count of leading zeros); the last lane of every (run, step)
//                         adds its sum to acc[nc j + c], j = cells[row[e]], by a 64-bit integer atomicAdd, and -- the cloud's
//                         first masked stream alone -- its rows to cnt[j].  Integer adds commute: no atomic decides a place or a
//                         value.  A run of a million duplicates costs one atomic a step, not a row.
//   k_enc_mean_store      a thread per (kept entry, component), tiles over KEPT entries: vals[nc kept[j] + c] = the mean of acc and
//                         cnt; a cell of one row keeps its value.  A pass of its own: kept[j]'s value is an addend of the first.
// acc (i64[n nc] per masked stream) and cnt (u32[n] per cloud) are regions of their own at the end of the arena, one range that one
// memset on the stream zeroes in front of the sum; no region is reused (the histograms are too small, the key buffers are the
// lod's), nothing else grows.  The records are EncMean (every masked stream of a cloud carries the cloud's one cnt) and the cloud's
// EncCellStreams, among the uploads: EncOrder is as it was, and so is every kernel above.  The host coder's twin is
// synth::merge_means; tests/hostcheck/encmeans_host.cpp runs the serial forms in the product's layout against it,
// tests/test_gpu_encode_means.py the ballots, shuffles and atomics.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_mean_sum 24 / 45 / 0, store 23 / 29 / 0; no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_vote_sequential_batch with vote_attributes != 0 (point clouds, merge_points = 1): entry j of a voted attribute of nc <= 2
// components carries the tuple (q[r][0], .., q[r][nc - 1]) that the most rows r of cell j have, among tuples of equally many rows the
// lexicographically smallest one (components as signed 32-bit integers, component 0 first) -- a function of the set of rows.  As the
// mean, the winner is written into the stream's `vals` at row kept[j], behind the merge and beside the mean kernels (the two masks
// share no attribute), in front of k_enc_lod_*, k_enc_part_cells, k_enc_part_bounds and k_enc_gather, on the merge's (cloud, tile)
// list with the cloud's voted streams in blockIdx.y; launched only when the chunk has a voted stream.  No sort:
//   k_enc_vote_count      a wave per (tile, voted stream), 64 sorted entries a step: the rows of every distinct (cell, tuple) counted
//                         in an open-addressing table of the stream, cap >= 2 n slots of (representative row + 1, count), 0 = empty.
//                         A slot is claimed by one 32-bit atomicCAS of the row; a later row compares its own (cells[r], tuple) with
//                         the representative's, read from cells and vals, which nothing writes during this step, and on a match
//                         adds to the slot's count, else goes on to the next slot (linear probing from a hash of cell and tuple; at
//                         most cap probes, no lane waits for another).  Which row represents a tuple and which slot it lands in
//                         depend on arrival; the count of every (cell, tuple) does not.  Inside the wave first: the lanes of a
//                         (run, step) whose tuple equals that of the run's first lane of the step (the head ballot of
//                         k_enc_mean_sum, one shuffle, one ballot) make ONE insert with their popcount, the other lanes insert
//                         singly -- a cell of a million equal labels costs one atomic a step, not one a row.  A table found full
//                         (it cannot be at load <= 1/2) sets EncVote::full, and the host fails the cloud alone.
//   k_enc_vote_best       a thread per slot, two launches: phase 0 atomicMax(best_cnt[j], count); phase 1, for the slots whose
//                         count equals best_cnt[j], atomicMax(best_val[j], ~pack), pack = component 0 with the sign bit flipped in
//                         the high word and component 1 likewise in the low word (nc = 1: component 0 alone, in the low word): the
//                         maximum of ~pack is the minimum of pack, and it starts from the zero the one memset leaves.  Maximum
//                         commutes: no atomic decides a value.
//   k_enc_vote_store      a thread per kept entry, tiles over KEPT entries: vals[nc kept[j] + c] from ~best_val[j]; a cell of one
//                         row keeps its value (its tuple wins).
// The tables (u32[2 cap] per voted stream), best_cnt (u32[n]) and best_val (u64[n]) are regions of their own at the end of the arena,
// behind the means', one range that one memset on the stream zeroes in front of the count; no region is reused.  The records are
// EncVote and an EncCellStreams of the votes' own per cloud, among the uploads; the five kernels of the two passes begin alike
// (ord_cell_block).  The host coder's twin is
// synth::merge_votes (a sort of every cell's tuples); tests/hostcheck/encvotes_host.cpp runs the serial forms in the product's layout
// against it, tests/test_gpu_encode_votes.py the ballots, shuffles and atomics.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_vote_count 28 / 52 / 0, best 16 / 50 / 0, store 9 / 30 / 0; no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_normal_mean_sequential_batch with mean_normals = 1 (point clouds, merge_points = 1): entry j of the normals of a cloud that
// has them carries the code of the normalised sum of the unit normals of the cnt rows of cell j, by a rule in 64-bit integers on the
// octahedral codes (s, t) the plain call codes at normal_bits = b -- the mean of the integers s and t themselves points elsewhere
// wherever a cell lies across the fold (x < 0) or the diamond edge.  With max_value = 2^b - 2, c = max_value / 2 and rdiv(num, den) =
// floor((2 num + den) / (2 den)), floor division:
//   1. a = s - c, b' = t - c; v = (c - |a| - |b'|, a, b') where |a| + |b'| <= c, else (c - |a| - |b'|, sg(a) (c - |b'|), sg(b') (c - |a|)),
//      sg(0) = +1: the inverse of the quantiser's tail, |v|_1 = c
//   2. u_k = rdiv(v_k << 42, len), len = isqrt((v . v) << 24) the exact floor square root (the argument is below 2^62, 2 |v_k| 2^42 +
//      len below 2^63): the unit vector in Q30
//   3. U = the sum of u over the rows of the cell (at most 2^28 rows: below 2^59)
//   4. M_k = rdiv(U_k, cnt)
//   5. A = |M_0| + |M_1| + |M_2|; A = 0 (the normals cancel): i0 = c, i1 = 0, z positive, what the quantiser makes of a zero vector;
//      else i0 = rdiv(M_0 c, A), i1 = rdiv(M_1 c, A), z negative iff M_2 < 0; then the quantiser's own tail from i2 = c - |i0| - |i1|
//      through the canonicalisation (enc_oct_from_scaled, dsa_encode_schemes.h: one copy, which enc_oct_from_float calls too)
//   6. a cell of one row keeps its code
// -- a function of the SET of rows.  As the means, written into the stream's `vals` at row kept[j], behind the merge, beside the means
// and the votes (the normals are in neither mask), in front of k_enc_lod_*, k_enc_part_cells, k_enc_part_bounds and k_enc_gather, on
// the merge's (cloud, tile) list; launched only when a cloud of the chunk has normals:
//   k_enc_normal_sum      a wave per tile, 64 sorted entries a step: the head ballot, the run's first lane and the last lane of
//                         every (run, step) as k_enc_mean_sum finds them; steps 1 and 2 per lane -- the square root from a double
//                         seed put right in integers (ord_isqrt), the three quotients as unsigned 64-bit divisions of magnitudes
//                         (ord_normal_unit): both exact, no result depends on a float rounding -- then three segmented inclusive
//                         sums in int64 (ord_wave_incl) and one 64-bit atomicAdd per (run, step) and component into acc[3 j + k],
//                         one 32-bit atomicAdd of the run's rows into cnt[j].  Integer adds commute.
//   k_enc_normal_store    a thread per kept entry, tiles over KEPT entries: steps 4 - 6 into vals[2 kept[j] ..]
// acc (i64[3 n]) and cnt (u32[n], the pass's own: the means count theirs, every count region is added to once) per cloud with normals
// are regions of their own at the end of the arena, behind the votes', one range that one memset on the stream zeroes in front of the
// sum; no region is reused.  The records are EncNormal and an EncCellStreams of the pass's own per cloud, among the uploads; both
// kernels begin with ord_cell_block.  EncOrder and every kernel above are as they were.  The host coder's twin is
// synth::merge_mean_normals (serial, a bitwise square root, floor division of signed numbers); tests/hostcheck/encnormalmeans_host.cpp
// runs the serial forms in the product's layout against it, tests/test_gpu_encode_normal_means.py the ballots, shuffles and atomics.
// Not built: a vote over normals, weighted means, means per coarser lod cell, mean normals of meshes.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_normal_sum 40 / 52 / 0 (the three 64-bit divisions are inline code, no
// call), store 31 / 41 / 0; no scratch, no spills, 8 waves per SIMD.
//
// dsa_encode_voxel_sequential_batch with voxel_bits = C >= 1 (point clouds, merge_points = 1): one point per occupied cell of the grid
// with C bits per axis, whatever B = position_bits >= C the positions are stored at.  With s = B - C (EncOrder::voxel_shift) the
// voxel of a row is key >> 3 s -- the sort has put the rows of any coarser cell side by side -- and that is all the merge, the means,
// the votes and the mean normals need to know: ord_head, the one head predicate of k_enc_merge_heads, k_enc_merge_compact,
// k_enc_mean_sum, k_enc_vote_count and k_enc_normal_sum, compares key >> 3 s, and with s = 0 every one of them does what it did.
// kept[j] is then the voxel's smallest (key, row), no longer its smallest row; cells[] and the vote table's hash and compare go by
// the entry, so they follow.  The levels (ord_lod_levels, and through it k_enc_lod_*, k_enc_part_cells and the layout's slot count)
// are L = C - D + 1: two kept points differ within their top C triples.  voxel_point (EncOrder::voxel_point) says which point a voxel
// keeps:
//   first      kept[j] as the merge leaves it.
//   centroid   the positions are one more stream of the means pass -- the cloud's FIRST EncMean record {vals = O.vals, nc = 3}, so the
//              one that counts the rows of every voxel, once -- and the pass runs for such a chunk with mean_attributes = 0 too.
//              k_enc_mean_store writes floor((2 S + cnt) / (2 cnt)) into O.vals at kept[j], behind everything that reads the
//              positions of other rows (k_enc_voxel_near: never in the same request) and in front of k_enc_lod_levels and
//              k_enc_part_bounds, which read keys and boxes from vals at the kept rows.  A component's mean lies between its minimum
//              and maximum over the voxel: the centroid lies in its voxel, the kept keys stay distinct and ascending.  No new kernel.
//   nearest    a pass of its own behind the merge and in front of the three cell passes, which write at kept[j], on the merge's
//              (cloud, tile) list; dist(r) = the sum over c of (2 (q[r][c] & (2^s - 1)) - (2^s - 1))^2 < 2^42, and the pair (dist,
//              row) does not fit 64 bits, so two phases as k_enc_vote_best has them:
//   k_enc_voxel_near      a wave per tile, 64 sorted entries a step: the head ballot, the run's first lane and the last lane of every
//                         (run, step) as k_enc_mean_sum finds them; phase 0: ~dist per lane, a segmented inclusive MAXIMUM across the
//                         wave (ord_wave_incl_max: ord_wave_incl's shape, max in place of +), the last lane of (run, step) raises
//                         best_dist[j] by a 64-bit atomicMax -- the maximum of ~dist is the minimum of dist, and it starts from the
//                         zero the one memset leaves; phase 1, a launch behind it: the lanes whose ~dist equals best_dist[j] stand
//                         with ~row, the others with 0, the same segmented maximum, a 32-bit atomicMax into best_row[j].  A voxel of a
//                         million rows costs one atomic a step, not one a row.  Maximum commutes: no atomic decides a value by arrival.
//   k_enc_voxel_pick      a thread per kept entry, tiles over KEPT entries: kept[j] = ~best_row[j]
// best_dist (u64[n]) and best_row (u32[n]) per cloud are regions of their own at the end of the arena, behind the normals', one range
// that one memset on the stream zeroes in front of phase 0; no region is reused.  The records are EncVoxel and an EncCellStreams of the
// pass's own per cloud, among the uploads; both kernels begin with ord_cell_block.  C = B is the merge as it stands under every rule:
// the layout leaves s = 0 and runs nothing more.  The host coder's twin is synth::merge_points with voxel_bits and voxel_point (a
// serial pass over the voxels' rows); tests/hostcheck/encvoxel_host.cpp runs the serial forms in the product's layout against it,
// tests/test_gpu_encode_voxel.py the ballots, shuffles and atomics.
// Not built: weighted centroids, the row nearest the centroid, a voxel edge that is not a power of two of the grid step, voxels of
// meshes, reductions per coarser lod cell.
// gfx950, hipcc -O3 (VGPR / SGPR / LDS bytes per block): k_enc_voxel_near 26 / 34 / 0, pick 6 / 25 / 0; with the shift k_enc_merge_heads
// 12 / 27 / 0, compact 14 / 27 / 0, k_enc_mean_sum 25 / 45 / 0, k_enc_vote_count 28 / 52 / 0, k_enc_normal_sum 40 / 52 / 0,
// k_enc_lod_levels 24 / 35 / 0, scan 22 / 37 / 0, k_enc_part_cells 44 / 23 / 0; no scratch, no spills, 8 waves per SIMD.
#pragma once
#include <stdint.h>

namespace dsa {

#define ORD_TILE 1024u             // entries of a tile: 16 steps of one wave
#define ORD_RADIX 256u             // 8 bits a pass
#define ORD_SCAN_PER 8u            // histogram entries a lane of k_enc_order_scan sums per step

struct EncOrder {                  // one per cloud of the chunk; in the arena, among the uploads
  uint64_t vals;                   // i32[3 n]: the position stream's integers, row order
  uint64_t key[2];                 // u64[n] each: pass p reads [p & 1], writes [(p + 1) & 1]
  uint64_t row[2];                 // u32[n] each, likewise; row[last] is the e2v of the cloud's streams: OUTPUT perm
                                   //   (merge: row[last ^ 1] is, OUTPUT kept[m])
  uint64_t hist;                   // u32[ORD_RADIX * tiles]: of the pass under way, digit-major
  uint64_t rank;                   // u32[n] OUTPUT (meshes; else 0): the entry of every row
  uint64_t faces;                  // compressed indices: u16[count] (narrow) or u32[count], remapped in place; else count 0
  uint32_t n, tiles;               // points; (n + ORD_TILE - 1) / ORD_TILE
  uint32_t bits, count;            // position_bits; 3F corners to remap
  uint32_t narrow, merge;          // merge: merge_points = 1, the three fields below are set
  uint64_t cells;                  // u32[n] OUTPUT (merge; else 0): row_entries, the entry of the cell of every row
  uint32_t stream0, streams;       // the cloud's value streams among the chunk's EncStream records: k_enc_merge_scan lowers their nv
  uint32_t m, part_cells;          // OUTPUT (merge): occupied cells; part_cells: not 0: the kept points in parts of at most so many (k_enc_part_cells),
  uint32_t part0, part_slots;      //   the cloud's part_slots = ceil(n / part_cells) EncPart records from part0 on, slot p with `streams` stream records
                                   //   from stream0 + p * streams on
  uint32_t lod_bits, last;         // lod_base_bits D (0: no levels); not 0: part_slots = ceil(n / part_cells) + bits - D and the two fields below are set
                                   //   last: the buffer of each pair the last sort pass wrote, passes & 1 (ord_sorted / ord_kept / ord_part_rows below)
  uint64_t lod_rows;               // u32[n] OUTPUT lod[m], the kept rows in (level, kept) order -- the e2v of the cloud's streams -- and behind it u32[n] pos[m],
                                   //   the place of every kept entry in lod: the key buffer the last sort pass did not write, key[last ^ 1]
  uint64_t lod_table;              // EncLodTable OUTPUT: points and first lod entry of every level
  uint32_t voxel_shift, voxel_point;       // voxel_bits C >= 1: s = bits - C, the cell of the merge is key >> 3 s (0: the position cell, the merge as it was);
                                   //   DSA_VOXEL_POINT_* (0 first, 1 centroid: a record of the means pass, 2 nearest: k_enc_voxel_*)
};
struct EncOrderTile { uint32_t cloud, tile; };
struct EncPart {                   // one per part of a split cloud, the parts of a cloud side by side; in the arena, among the uploads
  uint32_t cloud;                  // its cloud among the chunk's EncOrder records
  uint32_t lo, n;                  // sorted entries lo .. lo + n of the cloud
  int32_t qmin[3], qmax[3];        // OUTPUT per component over vals of the part's rows (the layout sets INT32_MAX / INT32_MIN)
  uint32_t pad;                    // OUTPUT (lod_base_bits >= 1): the level of the slot (k_enc_part_cells); else 0
};
struct EncPartTile { uint32_t part, tile; };
#define ORD_LOD_LEVELS 20u         // position_bits is at most 20 (enc_check_bits): L = bits - D + 1 <= 20
struct EncLodTable { uint32_t count[ORD_LOD_LEVELS], base[ORD_LOD_LEVELS]; };      // m_l and base_l of a cloud (k_enc_lod_scan), zero from L on
// mean_attributes, vote_attributes: records of the cell passes' own, so that EncOrder and the kernels that index it stay as they are
struct EncCellStreams { uint32_t first, count; };               // one per EncOrder record and pass: the cloud's `count` EncMean / EncVote records from `first` on (0: none)
struct EncMean {                   // one per masked stream, a cloud's side by side
  uint64_t vals, acc;              // the stream's vals i32[n nc], its sums i64[n nc]
  uint64_t cnt;                    // u32[n]: the rows of every cell, one region per cloud, the same in all of its records
  uint32_t nc, pad;                // components
};
struct EncVote {                   // one per voted stream, a cloud's side by side
  uint64_t vals;                   // the stream's vals i32[n nc]
  uint64_t table;                  // u32[2 cap]: slot s = (representative row + 1, rows counted); zeroed in front of k_enc_vote_count
  uint64_t best_cnt, best_val;     // u32[n] the most rows a tuple of cell j has; u64[n] the largest ~pack among the tuples with so many
  uint32_t nc, cap;                // components (1 or 2); slots, >= 2 n
  uint32_t full, pad;              // OUTPUT: not 0: a row found no slot (never at cap >= 2 n)
};
struct EncNormal {                 // mean_normals: one per cloud that has normals
  uint64_t vals, acc;              // the normal stream's codes i32[2 n]; the sums of its rows' unit vectors in Q30, i64[3 n]
  uint64_t cnt;                    // u32[n]: the rows of every cell, counted by this pass for itself (the means' count theirs)
  uint32_t bits, pad;              // normal_bits
};
struct EncVoxel {                  // voxel_point = nearest: one per cloud
  uint64_t best_dist;              // u64[n]: the largest ~dist a row of voxel j has (zeroed in front of k_enc_voxel_near)
  uint64_t best_row;               // u32[n]: the largest ~row among the rows of that distance
};

static inline uint32_t enc_order_passes(uint32_t bits) { return (3u * bits + 7u) / 8u; }

// The buffers behind the sort, named once for the kernels, the layout and the host checks (offsets into the arena):
struct EncSorted { uint64_t key, row; };
// the key / row pair the last pass wrote: the sorted keys and perm
__host__ __device__ __forceinline__ EncSorted ord_sorted(const EncOrder &O) { return EncSorted{O.key[O.last & 1u], O.row[O.last & 1u]}; }
// merge: kept, in the row buffer the last pass read
__host__ __device__ __forceinline__ uint64_t ord_kept(const EncOrder &O) { return O.row[(O.last & 1u) ^ 1u]; }
// the rows the parts of a cloud are runs of: lod with levels, else kept with the merge, else perm
__host__ __device__ __forceinline__ uint64_t ord_part_rows(const EncOrder &O) { return O.lod_bits ? O.lod_rows : O.merge ? ord_kept(O) : ord_sorted(O).row; }

// Tile T of cloud O over its first `limit` entries (O.n; O.m for tiles over KEPT entries -- never beyond n: the comparison keeps a
// fault elsewhere inside the cloud's buffers): entries e0 .. end.  False for a tile at or beyond the limit.
__device__ __forceinline__ bool ord_tile(const EncOrder &O, const EncOrderTile &T, uint32_t limit, uint32_t &e0, uint32_t &end) {
  if (limit > O.n) limit = O.n;
  e0 = T.tile * ORD_TILE;
  if (e0 >= limit) return false;
  end = limit - e0 < ORD_TILE ? limit : e0 + ORD_TILE;
  return true;
}
// entry e of a cloud's sorted keys begins a cell: the cell of an entry is its key without the low 3 s bits, s = O.voxel_shift (0: the key)
__device__ __forceinline__ bool ord_head(const EncOrder &O, const uint64_t *key, uint32_t e) {
  const uint32_t shift = O.voxel_shift < 20u ? 3u * O.voxel_shift : 0u;      // (s < bits <= 20 by the layout: the comparison keeps the shift below 64)
  return e == 0u || (key[e] >> shift) != (key[e - 1u] >> shift);
}
// the bits per axis of the grid the merge keeps one point per cell of: C = bits - s
__device__ __forceinline__ uint32_t ord_cell_bits(const EncOrder &O) { return O.voxel_shift < O.bits ? O.bits - O.voxel_shift : O.bits; }
// the levels of a cloud, L = C - D + 1; 0: none (no lod_base_bits, or -- never by the layout -- one the table cannot hold)
__device__ __forceinline__ uint32_t ord_lod_levels(const EncOrder &O) {
  const uint32_t C = ord_cell_bits(O);
  return O.lod_bits == 0u || O.lod_bits > C || C - O.lod_bits >= ORD_LOD_LEVELS ? 0u : C - O.lod_bits + 1u;
}
#if defined(__HIPCC__)
// the inclusive sum of x over the lanes of the wave from lane `start` up to this one (start 0: over all lanes below and this one)
template <class X>
__device__ __forceinline__ X ord_wave_incl(X x, uint32_t lane, uint32_t start = 0u) {
  for (uint32_t d = 1; d < (uint32_t)WAVE; d <<= 1) { const X y = __shfl_up(x, d, WAVE); if (lane >= start + d) x += y; }
  return x;
}
// the valid lanes whose low BITS bits of `value` equal this lane's, by BITS ballots
template <uint32_t BITS>
__device__ __forceinline__ unsigned long long ord_match(uint32_t value, bool valid) {
  unsigned long long same = __ballot(valid);
  for (uint32_t b = 0; b < BITS; ++b) {
    const bool bit = ((value >> b) & 1u) != 0;
    const unsigned long long with = __ballot(valid && bit);
    same &= bit ? with : ~with;
  }
  return same;
}
#endif

// bit b of the low 21 bits of x to bit 3 b
__device__ __forceinline__ uint64_t ord_spread(uint32_t v) {
  uint64_t x = v & 0x1FFFFFu;
  x = (x | x << 32) & 0x001F00000000FFFFull;
  x = (x | x << 16) & 0x001F0000FF0000FFull;
  x = (x | x << 8) & 0x100F00F00F00F00Full;
  x = (x | x << 4) & 0x10C30C30C30C30C3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ uint64_t ord_key(const int32_t *q, uint32_t bits) {
  const uint32_t mask = (1u << bits) - 1u;                     // (bits 1 .. 20: enc_check_bits)
  return ord_spread((uint32_t)q[0] & mask) << 2 | ord_spread((uint32_t)q[1] & mask) << 1 | ord_spread((uint32_t)q[2] & mask);
}

__global__ __launch_bounds__(256) void k_enc_order_keys(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  const int32_t *vals = (const int32_t *)(arena + O.vals);
  uint64_t *key = (uint64_t *)(arena + O.key[0]);
  uint32_t *row = (uint32_t *)(arena + O.row[0]);
  uint32_t e0, end;
  if (!ord_tile(O, T, O.n, e0, end)) return;
  for (uint32_t r = e0 + threadIdx.x; r < end; r += blockDim.x) { key[r] = ord_key(vals + 3ull * r, O.bits); row[r] = r; }
}

__device__ __forceinline__ uint32_t ord_digit(uint64_t key, uint32_t pass) { return (uint32_t)(key >> (8u * pass)) & (ORD_RADIX - 1u); }

__global__ __launch_bounds__(WAVE) void k_enc_order_hist(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt, uint32_t pass) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  const uint64_t *key = (const uint64_t *)(arena + O.key[pass & 1u]);
  uint32_t *hist = (uint32_t *)(arena + O.hist);
  uint32_t e0, end;
  if (!ord_tile(O, T, O.n, e0, end)) return;
  const uint32_t lane = threadIdx.x;
#if defined(__HIPCC__)
  __shared__ uint32_t s_count[ORD_RADIX];
  for (uint32_t d = lane; d < ORD_RADIX; d += WAVE) s_count[d] = 0;
  __syncthreads();
  for (uint32_t e = e0 + lane; e < end; e += WAVE) atomicAdd(&s_count[ord_digit(key[e], pass)], 1u);
  __syncthreads();
  for (uint32_t d = lane; d < ORD_RADIX; d += WAVE) hist[(size_t)d * O.tiles + T.tile] = s_count[d];
#else       // the sanitizer build of tests/hostcheck/encorder_host.cpp runs the lanes of a wave one after the other: lane 0 counts
  if (lane != 0) return;
  for (uint32_t d = 0; d < ORD_RADIX; ++d) hist[(size_t)d * O.tiles + T.tile] = 0;
  for (uint32_t e = e0; e < end; ++e) hist[(size_t)ord_digit(key[e], pass) * O.tiles + T.tile] += 1u;
#endif
}

// one wave per cloud: blockIdx.x = cloud
__global__ __launch_bounds__(WAVE) void k_enc_order_scan(uint8_t *arena, const EncOrder *clouds, uint32_t nc) {
  if (blockIdx.x >= nc) return;
  const EncOrder &O = clouds[blockIdx.x];
  uint32_t *hist = (uint32_t *)(arena + O.hist);
  const uint32_t total = ORD_RADIX * O.tiles, lane = threadIdx.x;        // (tiles <= 2^18: the layout takes clouds of up to 2^28 points)
  uint32_t base = 0;
#if defined(__HIPCC__)
  for (uint32_t i0 = 0; i0 < total; i0 += WAVE * ORD_SCAN_PER) {        // (total is a multiple of ORD_SCAN_PER: a lane's run is inside or outside)
    const uint32_t i = i0 + lane * ORD_SCAN_PER;
    uint32_t x[ORD_SCAN_PER], sum = 0;
    for (uint32_t k = 0; k < ORD_SCAN_PER; ++k) { x[k] = i < total ? hist[i + k] : 0u; sum += x[k]; }
    const uint32_t incl = ord_wave_incl(sum, lane);
    uint32_t at = base + incl - sum;
    if (i < total) for (uint32_t k = 0; k < ORD_SCAN_PER; ++k) { hist[i + k] = at; at += x[k]; }
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
#else       // (as k_enc_order_hist: lane 0 sums)
  if (lane != 0) return;
  for (uint32_t i = 0; i < total; ++i) { const uint32_t x = hist[i]; hist[i] = base; base += x; }
#endif
}

__global__ __launch_bounds__(WAVE) void k_enc_order_scatter(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt, uint32_t pass) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  const uint64_t *key = (const uint64_t *)(arena + O.key[pass & 1u]);
  const uint32_t *row = (const uint32_t *)(arena + O.row[pass & 1u]);
  uint64_t *key_out = (uint64_t *)(arena + O.key[(pass + 1u) & 1u]);
  uint32_t *row_out = (uint32_t *)(arena + O.row[(pass + 1u) & 1u]);
  const uint32_t *hist = (const uint32_t *)(arena + O.hist);
  uint32_t e0, end;
  if (!ord_tile(O, T, O.n, e0, end)) return;
  const uint32_t lane = threadIdx.x;
#if defined(__HIPCC__)
  __shared__ uint32_t s_next[ORD_RADIX];                       // where the tile's next entry of every digit goes
  for (uint32_t d = lane; d < ORD_RADIX; d += WAVE) s_next[d] = hist[(size_t)d * O.tiles + T.tile];
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const uint64_t k = valid ? key[e] : 0ull;
    const uint32_t r = valid ? row[e] : 0u, d = ord_digit(k, pass);
    const unsigned long long same = ord_match<8>(d, valid);    // the lanes of this lane's digit
    const uint32_t at = valid ? s_next[d] : 0u;
    __syncthreads();                                           // (every lane has read before a digit's lowest lane advances its count)
    if (valid && (same & below) == 0ull) s_next[d] = at + (uint32_t)__popcll(same);
    __syncthreads();
    const uint32_t to = at + (uint32_t)__popcll(same & below);
    if (valid && to < O.n) { key_out[to] = k; row_out[to] = r; }      // (to < n by the scan: the comparison keeps a fault elsewhere inside the cloud's buffers)
  }
#else       // (as k_enc_order_hist: lane 0 places the tile's entries in their order)
  if (lane != 0) return;
  uint32_t next[ORD_RADIX];
  for (uint32_t d = 0; d < ORD_RADIX; ++d) next[d] = hist[(size_t)d * O.tiles + T.tile];
  for (uint32_t e = e0; e < end; ++e) { const uint32_t to = next[ord_digit(key[e], pass)]++; key_out[to] = key[e]; row_out[to] = row[e]; }
#endif
}

__global__ __launch_bounds__(256) void k_enc_order_rank(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  uint32_t e0, end;
  if (O.rank == 0 || !ord_tile(O, T, O.n, e0, end)) return;
  const uint32_t *perm = (const uint32_t *)(arena + ord_sorted(O).row);
  uint32_t *rank = (uint32_t *)(arena + O.rank);
  for (uint32_t e = e0 + threadIdx.x; e < end; e += blockDim.x) { const uint32_t r = perm[e]; if (r < O.n) rank[r] = e; }
}

// grid (blocks over corners, clouds); indices out of range never come here: the host refuses such a mesh before the launch
__global__ __launch_bounds__(256) void k_enc_order_faces(uint8_t *arena, const EncOrder *clouds, uint32_t nc) {
  if (blockIdx.y >= nc) return;
  const EncOrder &O = clouds[blockIdx.y];
  if (O.count == 0 || O.rank == 0) return;
  const uint32_t *rank = (const uint32_t *)(arena + O.rank);
  uint16_t *f16 = (uint16_t *)(arena + O.faces);
  uint32_t *f32 = (uint32_t *)(arena + O.faces);
  const bool narrow = O.narrow != 0;
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < O.count; c += gridDim.x * blockDim.x) {
    const uint32_t f = narrow ? (uint32_t)f16[c] : f32[c];
    if (f >= O.n) continue;
    if (narrow) f16[c] = (uint16_t)rank[f]; else f32[c] = rank[f];
  }
}

// ---- merge_points (the header comment has the contract)
__global__ __launch_bounds__(WAVE) void k_enc_merge_heads(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  uint32_t e0, end;
  if (!O.merge || !ord_tile(O, T, O.n, e0, end)) return;
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  uint32_t *counts = (uint32_t *)(arena + O.hist);
  const uint32_t lane = threadIdx.x;
  uint32_t heads = 0;
#if defined(__HIPCC__)
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool head = e < end && ord_head(O, key, e);
    heads += (uint32_t)__popcll(__ballot(head));
  }
  if (lane == 0) counts[T.tile] = heads;
#else       // (as k_enc_order_hist: lane 0 counts)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) heads += ord_head(O, key, e) ? 1u : 0u;
  counts[T.tile] = heads;
#endif
}

// one wave per cloud: blockIdx.x = cloud (Stream: dsa_encode_layout.h's EncStream, which is defined behind this file)
template <class Stream>
__global__ __launch_bounds__(WAVE) void k_enc_merge_scan(uint8_t *arena, EncOrder *clouds, uint32_t nc, Stream *streams, uint32_t ns) {
  if (blockIdx.x >= nc) return;
  EncOrder &O = clouds[blockIdx.x];
  if (!O.merge) return;
  uint32_t *counts = (uint32_t *)(arena + O.hist);
  const uint32_t lane = threadIdx.x;
  uint32_t base = 0;
#if defined(__HIPCC__)
  for (uint32_t t0 = 0; t0 < O.tiles; t0 += WAVE) {
    const uint32_t t = t0 + lane, x = t < O.tiles ? counts[t] : 0u, incl = ord_wave_incl(x, lane);
    if (t < O.tiles) counts[t] = base + incl - x;
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
  const uint32_t m = base < O.n ? base : O.n;                  // (m <= n by the counts: the comparison keeps a fault elsewhere inside the streams' regions)
  if (lane == 0) O.m = m;
  for (uint32_t k = lane; k < O.streams; k += WAVE) if (O.stream0 + k < ns) streams[O.stream0 + k].nv = m;
#else       // (as k_enc_order_hist: lane 0 sums)
  if (lane != 0) return;
  for (uint32_t t = 0; t < O.tiles; ++t) { const uint32_t x = counts[t]; counts[t] = base; base += x; }
  const uint32_t m = base < O.n ? base : O.n;
  O.m = m;
  for (uint32_t k = 0; k < O.streams; ++k) if (O.stream0 + k < ns) streams[O.stream0 + k].nv = m;
#endif
}

__global__ __launch_bounds__(WAVE) void k_enc_merge_compact(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  uint32_t e0, end;
  if (!O.merge || !ord_tile(O, T, O.n, e0, end)) return;
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  const uint32_t *row = (const uint32_t *)(arena + ord_sorted(O).row);
  uint32_t *kept = (uint32_t *)(arena + ord_kept(O));
  uint32_t *cells = (uint32_t *)(arena + O.cells);
  const uint32_t lane = threadIdx.x;
  uint32_t next = ((const uint32_t *)(arena + O.hist))[T.tile];       // the heads in front of the tile, then of the step
#if defined(__HIPCC__)
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const bool head = valid && ord_head(O, key, e);
    const unsigned long long heads = __ballot(head);
    const uint32_t at = next + (uint32_t)__popcll(heads & below);       // heads in front of this entry
    const uint32_t r = valid ? row[e] : 0u;
    if (head && at < O.n) kept[at] = r;
    // the head at or before e: entry 0 of a cloud is a head, so at + head >= 1 for every valid entry
    if (valid && r < O.n) cells[r] = at + (head ? 1u : 0u) - 1u;
    next += (uint32_t)__popcll(heads);
  }
#else       // (as k_enc_order_hist: lane 0 places the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) {
    if (ord_head(O, key, e)) kept[next++] = row[e];
    cells[row[e]] = next - 1u;
  }
#endif
}

// ---- the cell passes (mean_attributes, vote_attributes): behind the merge, in front of everything that reads `vals`, grid = (the
// chunk's (cloud, tile) pairs, the most chosen streams a cloud has).  What every kernel of a pass begins with: this block's cloud and
// tile, its entries e0 .. end -- over all entries of the cloud, or with `kept` over its KEPT ones -- and `rec`, the record of its
// stream among the pass's nr.  False: nothing to do (no such tile or stream; never by the layout: no merge, a record beyond nr).
struct EncCellBlock { const EncOrder *O; EncOrderTile T; uint32_t e0, end, rec; };
__device__ __forceinline__ bool ord_cell_block(EncCellBlock &B, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt, const EncCellStreams *streams, uint32_t nr, bool kept) {
  if (blockIdx.x >= nt) return false;
  B.T = tiles[blockIdx.x];
  B.O = &clouds[B.T.cloud];
  const EncCellStreams C = streams[B.T.cloud];
  B.rec = C.first + blockIdx.y;
  return B.O->merge && blockIdx.y < C.count && B.rec < nr && ord_tile(*B.O, B.T, kept ? B.O->m : B.O->n, B.e0, B.end);
}

// ---- mean_attributes (the header comment has the contract)
// floor((2 S + cnt) / (2 cnt)) in 64 bits: the exact mean of cnt >= 1 integers whose sum is S, ties toward +infinity
// (|S| <= 2^28 rows of 2^31: 2 S + cnt fits)
__device__ __forceinline__ int32_t ord_mean(int64_t sum, uint32_t cnt) {
  const int64_t num = 2 * sum + (int64_t)cnt, den = 2 * (int64_t)cnt;
  int64_t q = num / den;
  if (num % den < 0) --q;                                      // (C++ division truncates toward zero)
  return (int32_t)q;
}

// grid = (the chunk's (cloud, tile) pairs, the most masked streams a cloud has): one wave per (tile, masked stream)
__global__ __launch_bounds__(WAVE) void k_enc_mean_sum(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                       const EncCellStreams *mclouds, const EncMean *means, uint32_t nm) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, mclouds, nm, false)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncMean M = means[B.rec];
  if (M.nc == 0u || M.nc > 4u) return;                         // (never by the layout)
  const uint32_t *row = (const uint32_t *)(arena + ord_sorted(O).row);
  const uint32_t *cells = (const uint32_t *)(arena + O.cells);
  const int32_t *vals = (const int32_t *)(arena + M.vals);
  unsigned long long *acc = (unsigned long long *)(arena + M.acc);       // (two's complement: the sums are signed)
  uint32_t *cnt = (uint32_t *)(arena + M.cnt);
  const bool counts = blockIdx.y == 0u;                        // the cloud's first masked stream counts the rows of every cell
  const uint32_t lane = threadIdx.x, nc = M.nc;
#if defined(__HIPCC__)
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  const unsigned long long upto = (2ull << lane) - 1ull;       // the lanes at or below this one
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const bool head = valid && ord_head(O, key, e);
    const unsigned long long heads = __ballot(head), live = __ballot(valid);
    // the lane this lane's run begins at inside the step: the head at or below it, lane 0 for a run that came in from the step in front
    const unsigned long long mine = heads & upto;
    const uint32_t start = mine ? 63u - (uint32_t)__clzll((long long)mine) : 0u;
    // the last lane of (run, step): the lane above is a head, or holds no entry, or there is none
    const unsigned long long above = (live >> lane) >> 1, head_above = (heads >> lane) >> 1;
    const bool last = valid && ((above & 1ull) == 0ull || (head_above & 1ull) != 0ull);
    const uint32_t r = valid ? row[e] : 0u;
    const bool ok = valid && r < O.n;
    const uint32_t j = ok ? cells[r] : 0xFFFFFFFFu;
    for (uint32_t c = 0; c < nc; ++c) {                        // (uniform)
      const long long x = ord_wave_incl(ok ? (long long)vals[(size_t)nc * r + c] : 0ll, lane, start);       // (a lane adds what lies d below only while that is inside its run)
      if (last && j < O.n) atomicAdd(&acc[(size_t)nc * j + c], (unsigned long long)x);
    }
    if (counts && last && j < O.n) atomicAdd(&cnt[j], lane - start + 1u);
  }
#else       // (as k_enc_order_hist: lane 0 takes the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) {
    const uint32_t r = row[e], j = cells[r];
    for (uint32_t c = 0; c < nc; ++c) acc[(size_t)nc * j + c] += (unsigned long long)(long long)vals[(size_t)nc * r + c];
    if (counts) cnt[j] += 1u;
  }
#endif
}

// grid as above, tiles over KEPT entries: a thread per (kept entry, component).  No lane needs another: the host check runs it as it stands.
__global__ __launch_bounds__(256) void k_enc_mean_store(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                        const EncCellStreams *mclouds, const EncMean *means, uint32_t nm) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, mclouds, nm, true)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncMean M = means[B.rec];
  if (M.nc == 0u || M.nc > 4u) return;                         // (never by the layout)
  const uint32_t nc = M.nc, total = (end - e0) * nc;
  const uint32_t *kept = (const uint32_t *)(arena + ord_kept(O));
  const long long *acc = (const long long *)(arena + M.acc);
  const uint32_t *cnt = (const uint32_t *)(arena + M.cnt);
  int32_t *vals = (int32_t *)(arena + M.vals);
  for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
    const uint32_t j = e0 + i / nc, c = i % nc, r = kept[j], rows = cnt[j];
    if (r >= O.n || rows == 0u) continue;                      // (never by the merge: the comparisons keep a fault elsewhere inside the stream's values)
    if (rows > 1u) vals[(size_t)nc * r + c] = ord_mean((int64_t)acc[(size_t)nc * j + c], rows);       // (a cell of one point keeps its value)
  }
}

// ---- vote_attributes (the header comment has the contract): behind the merge, beside the means, in front of everything that reads `vals`
// The tuple of a row as one integer whose unsigned order is the lexicographic order of its signed components.
__device__ __forceinline__ uint64_t ord_vote_pack(const int32_t *v, uint32_t nc) {
  const uint64_t a = (uint32_t)v[0] ^ 0x80000000u;
  return nc == 2u ? a << 32 | (uint64_t)((uint32_t)v[1] ^ 0x80000000u) : a;
}
__device__ __forceinline__ uint32_t ord_vote_hash(uint32_t j, uint64_t pack) {
  uint64_t x = pack ^ ((uint64_t)j + 1u) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29;
  return (uint32_t)x ^ (uint32_t)(x >> 32);
}
// a value other threads of the launch may have raised meanwhile (it only ever goes from 0 to its value, or up)
__device__ __forceinline__ uint32_t ord_peek(const uint32_t *p) {
#if defined(__HIPCC__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
__device__ __forceinline__ void ord_raise(unsigned long long *p, unsigned long long x) {
#if defined(__HIPCC__)
  if (x > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, x);
#else
  if (x > *p) *p = x;
#endif
}
// `rows` rows of cell j with the tuple `pack`, row r one of them, into the table of `cap` slots: the slot of (j, pack), claimed if
// nobody has.  At most cap probes, no wait.  False: no slot.
__device__ __forceinline__ bool ord_vote_insert(uint32_t *table, uint32_t cap, const uint32_t *cells, const int32_t *vals, uint32_t n, uint32_t nc,
                                                uint32_t r, uint32_t j, uint64_t pack, uint32_t rows) {
  uint32_t s = ord_vote_hash(j, pack) % cap;
  for (uint32_t probe = 0; probe < cap; ++probe) {
    uint32_t rep = ord_peek(&table[2ull * s]);
    if (rep == 0u) rep = atomicCAS(&table[2ull * s], 0u, r + 1u);
    bool mine = rep == 0u;                                     // (claimed just now)
    if (!mine) { const uint32_t q = rep - 1u; mine = q < n && cells[q] == j && ord_vote_pack(vals + (size_t)nc * q, nc) == pack; }
    if (mine) { atomicAdd(&table[2ull * s + 1u], rows); return true; }
    s = s + 1u < cap ? s + 1u : 0u;
  }
  return false;
}

// grid = (the chunk's (cloud, tile) pairs, the most voted streams a cloud has): one wave per (tile, voted stream)
__global__ __launch_bounds__(WAVE) void k_enc_vote_count(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                         const EncCellStreams *vclouds, EncVote *votes, uint32_t nv) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, vclouds, nv, false)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  EncVote &V = votes[B.rec];
  const uint32_t lane = threadIdx.x, nc = V.nc, cap = V.cap;
  if (nc == 0u || nc > 2u || cap == 0u) return;                // (never by the layout)
  const uint32_t *row = (const uint32_t *)(arena + ord_sorted(O).row);
  const uint32_t *cells = (const uint32_t *)(arena + O.cells);
  const int32_t *vals = (const int32_t *)(arena + V.vals);
  uint32_t *table = (uint32_t *)(arena + V.table);
  bool lost = false;
#if defined(__HIPCC__)
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  const unsigned long long below = (1ull << lane) - 1ull, upto = (2ull << lane) - 1ull;
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const bool head = valid && ord_head(O, key, e);
    const unsigned long long heads = __ballot(head);
    // the lanes of this lane's run inside the step: from the head at or below it (lane 0 for a run that came in from the step in
    // front) to below the next head above it
    const unsigned long long mine = heads & upto, higher = heads & ~upto;
    const uint32_t start = mine ? 63u - (uint32_t)__clzll((long long)mine) : 0u;
    const unsigned long long run = (higher ? (higher & (0ull - higher)) - 1ull : ~0ull) & ~((1ull << start) - 1ull);
    const uint32_t r = valid ? row[e] : 0u;
    const uint32_t j = valid && r < O.n ? cells[r] : 0xFFFFFFFFu;
    const bool in = j < O.n;
    const unsigned long long pack = in ? ord_vote_pack(vals + (size_t)nc * r, nc) : 0ull;
    const unsigned long long first = __shfl(pack, (int)start, WAVE);
    // the lanes of the run that hold the tuple of its first lane: the lowest of them inserts for all, the others of the run singly
    const bool same = in && pack == first;
    const unsigned long long agree = __ballot(same) & run;
    const bool leads = same && (agree & below) == 0ull;
    if (in && (!same || leads) && !ord_vote_insert(table, cap, cells, vals, O.n, nc, r, j, pack, leads ? (uint32_t)__popcll(agree) : 1u)) lost = true;
  }
#else       // (as k_enc_order_hist: lane 0 takes the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) {
    const uint32_t r = row[e], j = cells[r];
    if (!ord_vote_insert(table, cap, cells, vals, O.n, nc, r, j, ord_vote_pack(vals + (size_t)nc * r, nc), 1u)) lost = true;
  }
#endif
  if (lost) V.full = 1u;
}

// grid as above, tile t over slots 2 t ORD_TILE .. (cap = 2 n: two slots an entry; the cloud's last tile takes what is left): a
// thread per slot.  phase 0: the most rows a tuple of every cell has; phase 1, a launch behind it: the smallest tuple among those.
__global__ __launch_bounds__(256) void k_enc_vote_best(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                       const EncCellStreams *vclouds, const EncVote *votes, uint32_t nv, uint32_t phase) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, vclouds, nv, false)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncVote V = votes[B.rec];
  const uint32_t nc = V.nc;
  if (nc == 0u || nc > 2u) return;                             // (never by the layout)
  const uint64_t s_end = B.T.tile + 1u == O.tiles || 2ull * end > V.cap ? V.cap : 2ull * end;
  const uint32_t *cells = (const uint32_t *)(arena + O.cells);
  const int32_t *vals = (const int32_t *)(arena + V.vals);
  const uint32_t *table = (const uint32_t *)(arena + V.table);
  uint32_t *best_cnt = (uint32_t *)(arena + V.best_cnt);
  unsigned long long *best_val = (unsigned long long *)(arena + V.best_val);
  for (uint64_t s = 2ull * e0 + threadIdx.x; s < s_end; s += blockDim.x) {
    const uint32_t rep = table[2ull * s], rows = table[2ull * s + 1u];
    if (rep == 0u || rep - 1u >= O.n) continue;                // (an empty slot)
    const uint32_t q = rep - 1u, j = cells[q];
    if (j >= O.n) continue;                                    // (never by the merge: the comparison keeps a fault elsewhere inside the cloud's regions)
    if (phase == 0u) { if (rows > ord_peek(&best_cnt[j])) atomicMax(&best_cnt[j], rows); }
    else if (rows == best_cnt[j]) ord_raise(&best_val[j], ~(unsigned long long)ord_vote_pack(vals + (size_t)nc * q, nc));
  }
}

// grid as above, tiles over KEPT entries: a thread per kept entry.  No lane needs another.
__global__ __launch_bounds__(256) void k_enc_vote_store(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                        const EncCellStreams *vclouds, const EncVote *votes, uint32_t nv) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, vclouds, nv, true)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncVote V = votes[B.rec];
  const uint32_t nc = V.nc;
  if (nc == 0u || nc > 2u) return;                             // (never by the layout)
  const uint32_t *kept = (const uint32_t *)(arena + ord_kept(O));
  const uint32_t *best_cnt = (const uint32_t *)(arena + V.best_cnt);
  const unsigned long long *best_val = (const unsigned long long *)(arena + V.best_val);
  int32_t *vals = (int32_t *)(arena + V.vals);
  for (uint32_t j = e0 + threadIdx.x; j < end; j += blockDim.x) {
    const uint32_t r = kept[j];
    if (r >= O.n || best_cnt[j] == 0u) continue;               // (never by the merge and the count: a full table leaves the row as it is)
    const unsigned long long pack = ~best_val[j];
    if (nc == 2u) { vals[2ull * r] = (int32_t)((uint32_t)(pack >> 32) ^ 0x80000000u); vals[2ull * r + 1u] = (int32_t)((uint32_t)pack ^ 0x80000000u); }
    else vals[r] = (int32_t)((uint32_t)pack ^ 0x80000000u);
  }
}

// ---- mean_normals (the header comment has the contract): behind the merge, beside the means and the votes, in front of everything that reads `vals`
// rdiv(num, den) = floor((2 num + den) / (2 den)), den > 0: num / den rounded to the nearest integer, ties toward +infinity (ord_mean in 64 bits)
__device__ __forceinline__ int64_t ord_rdiv(int64_t num, int64_t den) {
  const int64_t a = 2 * num + den, b = 2 * den;
  int64_t q = a / b;
  if (a % b < 0) --q;                                          // (C++ division truncates toward zero)
  return q;
}
// the exact floor square root of x < 2^62: a double seed (off by at most one either way, whatever its rounding), put right in integers
__device__ __forceinline__ uint64_t ord_isqrt(uint64_t x) {
  uint64_t r = (uint64_t)sqrt((double)x);
  if (r > 0x80000000ull) r = 0x80000000ull;                    // (r * r and (r + 1)^2 below stay inside 64 bits)
  while (r * r > x) --r;
  while ((r + 1ull) * (r + 1ull) <= x) ++r;
  return r;
}
// The unit vector of the octahedral code (s, t) in Q30, steps 1 and 2 of the rule: the integer vector v of L1 norm `center` the code
// stands for, u_k = rdiv(v_k << 42, len), len = isqrt((v . v) << 24).  The quotient is taken of magnitudes, one unsigned division a
// component: for v_k < 0, floor((-a + len) / (2 len)) = -floor((a + len - 1) / (2 len)) with a = 2 |v_k| 2^42 > len.
__device__ __forceinline__ void ord_normal_unit(int32_t s, int32_t t, int32_t center, long long u[3]) {
  const int32_t a = s - center, b = t - center, aa = a < 0 ? -a : a, ab = b < 0 ? -b : b;
  int32_t v[3];
  if (aa + ab <= center) { v[0] = center - aa - ab; v[1] = a; v[2] = b; }
  else { v[0] = center - aa - ab; v[1] = a < 0 ? ab - center : center - ab; v[2] = b < 0 ? aa - center : center - aa; }
  uint64_t n2 = 0;
  for (int k = 0; k < 3; ++k) n2 += (uint64_t)((int64_t)v[k] * v[k]);
  const uint64_t len = n2 < (1ull << 38) ? ord_isqrt(n2 << 24) : 0ull;      // (|v|_1 = center < 2^19 by the quantiser: the comparison keeps a code from elsewhere inside 62 bits)
  for (int k = 0; k < 3; ++k) {
    const uint64_t mag = (uint64_t)(v[k] < 0 ? -(int64_t)v[k] : (int64_t)v[k]) << 43;       // 2 |v_k| 2^42 < 2^62
    const uint64_t q = len ? (mag + len - (v[k] < 0 ? 1ull : 0ull)) / (2ull * len) : 0ull;
    u[k] = v[k] < 0 ? -(long long)q : (long long)q;
  }
}
// The code of the mean vector M, step 5: the quantiser's tail (enc_oct_from_scaled, dsa_encode_schemes.h) on rdiv(M_k center, |M|_1).
__device__ __forceinline__ void ord_normal_code(const int64_t M[3], int32_t center, int32_t max_value, int32_t &s, int32_t &t) {
  const int64_t A = (M[0] < 0 ? -M[0] : M[0]) + (M[1] < 0 ? -M[1] : M[1]) + (M[2] < 0 ? -M[2] : M[2]);
  int32_t i0 = center, i1 = 0;                                 // (the normals cancel: what the quantiser makes of a zero vector)
  if (A != 0) { i0 = (int32_t)ord_rdiv(M[0] * center, A); i1 = (int32_t)ord_rdiv(M[1] * center, A); }       // (|M_k| <= 2^30 + 1, center < 2^19)
  enc_oct_from_scaled(center, max_value, i0, i1, A != 0 && M[2] < 0, s, t);
}

// grid = (the chunk's (cloud, tile) pairs, 1): one wave per tile of a cloud with normals
__global__ __launch_bounds__(WAVE) void k_enc_normal_sum(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                         const EncCellStreams *nclouds, const EncNormal *normals, uint32_t nn) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, nclouds, nn, false)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncNormal N = normals[B.rec];
  if (N.bits < 2u || N.bits > 20u) return;                     // (never by the layout)
  const int32_t center = (int32_t)(((1u << N.bits) - 2u) / 2u);
  const uint32_t *row = (const uint32_t *)(arena + ord_sorted(O).row);
  const uint32_t *cells = (const uint32_t *)(arena + O.cells);
  const int32_t *vals = (const int32_t *)(arena + N.vals);
  unsigned long long *acc = (unsigned long long *)(arena + N.acc);       // (two's complement: the sums are signed)
  uint32_t *cnt = (uint32_t *)(arena + N.cnt);
  const uint32_t lane = threadIdx.x;
#if defined(__HIPCC__)
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  const unsigned long long upto = (2ull << lane) - 1ull;       // the lanes at or below this one
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const bool head = valid && ord_head(O, key, e);
    const unsigned long long heads = __ballot(head), live = __ballot(valid);
    // the run of this lane inside the step and its last lane, as k_enc_mean_sum finds them
    const unsigned long long mine = heads & upto;
    const uint32_t start = mine ? 63u - (uint32_t)__clzll((long long)mine) : 0u;
    const unsigned long long above = (live >> lane) >> 1, head_above = (heads >> lane) >> 1;
    const bool last = valid && ((above & 1ull) == 0ull || (head_above & 1ull) != 0ull);
    const uint32_t r = valid ? row[e] : 0u;
    const bool ok = valid && r < O.n;
    const uint32_t j = ok ? cells[r] : 0xFFFFFFFFu;
    long long u[3] = {0ll, 0ll, 0ll};
    if (ok) ord_normal_unit(vals[2ull * r], vals[2ull * r + 1u], center, u);
    for (uint32_t c = 0; c < 3u; ++c) {                        // (uniform)
      const long long x = ord_wave_incl(u[c], lane, start);
      if (last && j < O.n) atomicAdd(&acc[3ull * j + c], (unsigned long long)x);
    }
    if (last && j < O.n) atomicAdd(&cnt[j], lane - start + 1u);
  }
#else       // (as k_enc_order_hist: lane 0 takes the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) {
    const uint32_t r = row[e], j = cells[r];
    long long u[3];
    ord_normal_unit(vals[2ull * r], vals[2ull * r + 1u], center, u);
    for (uint32_t c = 0; c < 3u; ++c) acc[3ull * j + c] += (unsigned long long)u[c];
    cnt[j] += 1u;
  }
#endif
}

// grid as above, tiles over KEPT entries: a thread per kept entry.  No lane needs another: the host check runs it as it stands.
__global__ __launch_bounds__(256) void k_enc_normal_store(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                          const EncCellStreams *nclouds, const EncNormal *normals, uint32_t nn) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, nclouds, nn, true)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncNormal N = normals[B.rec];
  if (N.bits < 2u || N.bits > 20u) return;                     // (never by the layout)
  const int32_t max_value = (int32_t)((1u << N.bits) - 2u), center = max_value / 2;
  const uint32_t *kept = (const uint32_t *)(arena + ord_kept(O));
  const long long *acc = (const long long *)(arena + N.acc);
  const uint32_t *cnt = (const uint32_t *)(arena + N.cnt);
  int32_t *vals = (int32_t *)(arena + N.vals);
  for (uint32_t j = e0 + threadIdx.x; j < end; j += blockDim.x) {
    const uint32_t r = kept[j], rows = cnt[j];
    if (r >= O.n || rows <= 1u) continue;                      // (a cell of one row keeps its code; r < n and rows >= 1 by the merge and the sum)
    int64_t M[3];
    for (int k = 0; k < 3; ++k) M[k] = ord_rdiv((int64_t)acc[3ull * j + k], (int64_t)rows);
    int32_t s, t;
    ord_normal_code(M, center, max_value, s, t);
    vals[2ull * r] = s; vals[2ull * r + 1u] = t;
  }
}

// ---- voxel_point = DSA_VOXEL_POINT_NEAREST (the header comment has the contract): behind the merge, in front of the three passes above,
// which write at kept[j].  The distance of a row from the centre of its voxel in doubled coordinates, from the low s bits of its
// position integers: d_c = 2 (q_c & (2^s - 1)) - (2^s - 1), dist = d_0^2 + d_1^2 + d_2^2 < 3 2^40 (s <= 19).
__device__ __forceinline__ uint64_t ord_voxel_dist(const int32_t *q, uint32_t s) {
  const int64_t span = (int64_t)((1u << s) - 1u);
  uint64_t dist = 0;
  for (int c = 0; c < 3; ++c) { const int64_t d = 2 * (int64_t)((uint32_t)q[c] & (uint32_t)span) - span; dist += (uint64_t)(d * d); }
  return dist;
}
#if defined(__HIPCC__)
// the inclusive maximum of x over the lanes of the wave from lane `start` up to this one: ord_wave_incl with max in place of +
__device__ __forceinline__ unsigned long long ord_wave_incl_max(unsigned long long x, uint32_t lane, uint32_t start) {
  for (uint32_t d = 1; d < (uint32_t)WAVE; d <<= 1) { const unsigned long long y = __shfl_up(x, d, WAVE); if (lane >= start + d && y > x) x = y; }
  return x;
}
#endif

// grid = (the chunk's (cloud, tile) pairs, 1): one wave per tile of a cloud with nearest points, two launches.  phase 0: the largest
// ~dist of every voxel; phase 1, a launch behind it: the largest ~row among the rows of that distance.
__global__ __launch_bounds__(WAVE) void k_enc_voxel_near(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                         const EncCellStreams *xclouds, const EncVoxel *voxels, uint32_t nx, uint32_t phase) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, xclouds, nx, false)) return;
  const EncOrder &O = *B.O;
  const uint32_t e0 = B.e0, end = B.end;
  const EncVoxel X = voxels[B.rec];
  if (O.voxel_shift == 0u || O.voxel_shift >= 20u) return;     // (never by the layout)
  const uint32_t *row = (const uint32_t *)(arena + ord_sorted(O).row);
  const uint32_t *cells = (const uint32_t *)(arena + O.cells);
  const int32_t *vals = (const int32_t *)(arena + O.vals);
  unsigned long long *best_dist = (unsigned long long *)(arena + X.best_dist);
  uint32_t *best_row = (uint32_t *)(arena + X.best_row);
  const uint32_t lane = threadIdx.x;
#if defined(__HIPCC__)
  const uint64_t *key = (const uint64_t *)(arena + ord_sorted(O).key);
  const unsigned long long upto = (2ull << lane) - 1ull;       // the lanes at or below this one
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t e = s0 + lane;
    const bool valid = e < end;
    const bool head = valid && ord_head(O, key, e);
    const unsigned long long heads = __ballot(head), live = __ballot(valid);
    // the run of this lane inside the step and its last lane, as k_enc_mean_sum finds them
    const unsigned long long mine = heads & upto;
    const uint32_t start = mine ? 63u - (uint32_t)__clzll((long long)mine) : 0u;
    const unsigned long long above = (live >> lane) >> 1, head_above = (heads >> lane) >> 1;
    const bool last = valid && ((above & 1ull) == 0ull || (head_above & 1ull) != 0ull);
    const uint32_t r = valid ? row[e] : 0u;
    const bool ok = valid && r < O.n;
    const uint32_t j = ok ? cells[r] : 0xFFFFFFFFu;
    const unsigned long long near = ok ? ~(unsigned long long)ord_voxel_dist(vals + 3ull * r, O.voxel_shift) : 0ull;       // (not 0: dist < 2^42)
    if (phase == 0u) {
      const unsigned long long x = ord_wave_incl_max(near, lane, start);
      if (last && j < O.n && x > __hip_atomic_load(&best_dist[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&best_dist[j], x);
    } else {
      // (~row is not 0: r < n <= 2^28; a row farther than the voxel's nearest stands back with 0)
      const unsigned long long mark = ok && j < O.n && near == best_dist[j] ? (unsigned long long)(~r) : 0ull;
      const uint32_t x = (uint32_t)ord_wave_incl_max(mark, lane, start);
      if (last && j < O.n && x > ord_peek(&best_row[j])) atomicMax(&best_row[j], x);
    }
  }
#else       // (as k_enc_order_hist: lane 0 takes the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e) {
    const uint32_t r = row[e], j = cells[r];
    const unsigned long long near = ~(unsigned long long)ord_voxel_dist(vals + 3ull * r, O.voxel_shift);
    if (phase == 0u) { if (near > best_dist[j]) best_dist[j] = near; }
    else if (near == best_dist[j] && ~r > best_row[j]) best_row[j] = ~r;
  }
#endif
}

// grid as above, tiles over KEPT entries: a thread per kept entry.  No lane needs another: the host check runs it as it stands.
__global__ __launch_bounds__(256) void k_enc_voxel_pick(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt,
                                                        const EncCellStreams *xclouds, const EncVoxel *voxels, uint32_t nx) {
  EncCellBlock B;
  if (!ord_cell_block(B, clouds, tiles, nt, xclouds, nx, true)) return;
  const EncOrder &O = *B.O;
  const EncVoxel X = voxels[B.rec];
  uint32_t *kept = (uint32_t *)(arena + ord_kept(O));
  const uint32_t *best_row = (const uint32_t *)(arena + X.best_row);
  for (uint32_t j = B.e0 + threadIdx.x; j < B.end; j += blockDim.x) {
    const uint32_t r = ~best_row[j];
    if (r < O.n) kept[j] = r;                                  // (always by the two phases: an untouched entry keeps the voxel's first row)
  }
}

// ---- part_cells (the header comment has the contract): a thread per part slot of the chunk, behind k_enc_merge_scan and, for a
// cloud with levels, behind k_enc_lod_scan and k_enc_lod_scatter.  The parts of level 0, then of level 1, ...: a cloud without
// levels is one level of its m kept entries from 0 on (it has no table region: none is read for it).
template <class Stream>
__global__ __launch_bounds__(WAVE) void k_enc_part_cells(uint8_t *arena, const EncOrder *clouds, uint32_t nc, EncPart *parts, uint32_t np, Stream *streams, uint32_t ns) {
  const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= np) return;
  EncPart &P = parts[i];
  if (P.cloud >= nc) return;
  const EncOrder &O = clouds[P.cloud];
  const uint32_t levels = O.lod_bits ? ord_lod_levels(O) : 1u;
  if (levels == 0u || O.part_cells == 0u || i < O.part0 || i - O.part0 >= O.part_slots) return;       // (never by the layout)
  const EncLodTable *table = O.lod_bits ? (const EncLodTable *)(arena + O.lod_table) : nullptr;
  const uint32_t m = O.m < O.n ? O.m : O.n;
  uint64_t p = i - O.part0;
  uint32_t lo = 0, cnt = 0, level = 0;
  for (uint32_t l = 0; l < levels; ++l) {
    const uint64_t ml = table ? table->count[l] : m, live = (ml + O.part_cells - 1u) / O.part_cells;
    if (p < live) { lo = (table ? table->base[l] : 0u) + (uint32_t)(p * ml / live); cnt = (uint32_t)((p + 1u) * ml / live) - (uint32_t)(p * ml / live); level = l; break; }      // (64 bits: p m < 2^16 2^28)
    p -= live;
  }
  if (lo > O.n || cnt > O.n - lo) { lo = 0; cnt = 0; level = 0; }      // (never by the scan: the comparison keeps a fault elsewhere inside the cloud's buffers)
  P.lo = lo; P.n = cnt; P.pad = level;
  const uint64_t rows = ord_part_rows(O) + 4ull * lo, s0 = (uint64_t)O.stream0 + (uint64_t)(i - O.part0) * O.streams;
  for (uint32_t k = 0; k < O.streams; ++k) if (s0 + k < ns) { Stream &S = streams[s0 + k]; S.nv = cnt; S.e2v = rows; if (cnt == 0u) S.kind = 3u; }      // (empty: an empty list, which every step passes by)
}

// ---- lod_base_bits (the header comment has the contract): behind the merge, in front of k_enc_part_cells
// The level of a kept point from its key and the key of the kept point in front of it: c leading bit-triples in common out of
// `bits`, level max(0, c + 1 - D).  (Equal keys never come here, the kept keys are distinct: the comparison keeps the level below L.)
__device__ __forceinline__ uint32_t ord_lod_level(uint64_t a, uint64_t b, uint32_t bits, uint32_t base_bits, uint32_t top) {
  const uint64_t x = a ^ b;
#if defined(__HIPCC__)
  const uint32_t len = x ? 64u - (uint32_t)__clzll((long long)x) : 0u;
#else
  const uint32_t len = x ? 64u - (uint32_t)__builtin_clzll(x) : 0u;
#endif
  const uint32_t triples = (len + 2u) / 3u, c = triples < bits ? bits - triples : 0u;
  const uint32_t level = c + 1u > base_bits ? c + 1u - base_bits : 0u;
  return level < top ? level : top;
}

// grid = the chunk's (cloud, tile) pairs, tiles over KEPT entries
__global__ __launch_bounds__(WAVE) void k_enc_lod_levels(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  const uint32_t lane = threadIdx.x, levels = ord_lod_levels(O);
  uint32_t e0, end;
  if (levels == 0u || !ord_tile(O, T, O.m, e0, end)) return;
  const int32_t *vals = (const int32_t *)(arena + O.vals);
  const uint32_t *kept = (const uint32_t *)(arena + ord_kept(O));
  uint32_t *pos = (uint32_t *)(arena + O.lod_rows) + O.n;       // (the level of every kept entry until k_enc_lod_scatter puts its place there)
  uint32_t *hist = (uint32_t *)(arena + O.hist);
#if defined(__HIPCC__)
  uint32_t mine = 0;                                           // lane l: the tile's entries of level l
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t j = s0 + lane;
    const bool valid = j < end;
    uint32_t level = 0;
    if (valid && j != 0u) {
      const uint32_t r = kept[j], q = kept[j - 1u];
      if (r < O.n && q < O.n) level = ord_lod_level(ord_key(vals + 3ull * r, O.bits), ord_key(vals + 3ull * q, O.bits), O.bits, O.lod_bits, levels - 1u);
    }
    if (valid) pos[j] = level;
    for (uint32_t l = 0; l < levels; ++l) {
      const uint32_t c = (uint32_t)__popcll(__ballot(valid && level == l));
      if (lane == l) mine += c;
    }
  }
  if (lane < levels) hist[(size_t)lane * O.tiles + T.tile] = mine;
#else       // (as k_enc_order_hist: lane 0 counts)
  if (lane != 0) return;
  for (uint32_t l = 0; l < levels; ++l) hist[(size_t)l * O.tiles + T.tile] = 0;
  for (uint32_t j = e0; j < end; ++j) {
    const uint32_t level = j == 0u ? 0u : ord_lod_level(ord_key(vals + 3ull * kept[j], O.bits), ord_key(vals + 3ull * kept[j - 1u], O.bits), O.bits, O.lod_bits, levels - 1u);
    pos[j] = level;
    hist[(size_t)level * O.tiles + T.tile] += 1u;
  }
#endif
}

// one wave per cloud: blockIdx.x = cloud.  The counts of the tiles that hold kept entries, in (level, tile) order.
__global__ __launch_bounds__(WAVE) void k_enc_lod_scan(uint8_t *arena, const EncOrder *clouds, uint32_t nc) {
  if (blockIdx.x >= nc) return;
  const EncOrder &O = clouds[blockIdx.x];
  const uint32_t levels = ord_lod_levels(O);
  if (levels == 0u) return;
  const uint32_t m = O.m < O.n ? O.m : O.n, live = (m + ORD_TILE - 1u) / ORD_TILE;
  const uint32_t total = levels * live, lane = threadIdx.x;     // (live <= 2^18, levels <= 20)
  uint32_t *hist = (uint32_t *)(arena + O.hist);
  EncLodTable &table = *(EncLodTable *)(arena + O.lod_table);
  uint32_t base = 0;
#if defined(__HIPCC__)
  for (uint32_t i0 = 0; i0 < total; i0 += WAVE) {
    const uint32_t i = i0 + lane, l = i < total ? i / live : 0u;
    const size_t at = (size_t)l * O.tiles + (i - l * live);
    const uint32_t x = i < total ? hist[at] : 0u, incl = ord_wave_incl(x, lane);
    if (i < total) hist[at] = base + incl - x;
    base += (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
  }
  __syncthreads();                                             // (the starts written above, read below by other lanes of the wave)
  if (lane < ORD_LOD_LEVELS) {
    const uint32_t first = lane < levels && live ? hist[(size_t)lane * O.tiles] : 0u, next = lane + 1u < levels && live ? hist[(size_t)(lane + 1u) * O.tiles] : base;
    table.base[lane] = lane < levels ? first : 0u;
    table.count[lane] = lane < levels ? next - first : 0u;
  }
#else       // (as k_enc_order_hist: lane 0 sums)
  if (lane != 0) return;
  for (uint32_t l = 0; l < ORD_LOD_LEVELS; ++l) { table.base[l] = 0; table.count[l] = 0; }
  for (uint32_t l = 0; l < levels; ++l) {
    table.base[l] = base;
    for (uint32_t t = 0; t < live; ++t) { const uint32_t x = hist[(size_t)l * O.tiles + t]; hist[(size_t)l * O.tiles + t] = base; base += x; }
    table.count[l] = base - table.base[l];
  }
#endif
}

__global__ __launch_bounds__(WAVE) void k_enc_lod_scatter(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  const uint32_t lane = threadIdx.x, levels = ord_lod_levels(O);
  uint32_t e0, end;
  if (levels == 0u || !ord_tile(O, T, O.m, e0, end)) return;
  const uint32_t *kept = (const uint32_t *)(arena + ord_kept(O));
  uint32_t *lod = (uint32_t *)(arena + O.lod_rows), *pos = lod + O.n;
  const uint32_t *hist = (const uint32_t *)(arena + O.hist);
#if defined(__HIPCC__)
  __shared__ uint32_t s_next[32];                              // where the tile's next entry of every level goes
  if (lane < 32u) s_next[lane] = lane < levels ? hist[(size_t)lane * O.tiles + T.tile] : 0u;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t s0 = e0; s0 < end; s0 += WAVE) {               // (uniform: every lane takes every step)
    const uint32_t j = s0 + lane;
    const bool valid = j < end;
    const uint32_t r = valid ? kept[j] : 0u, seen = valid ? pos[j] : 0u, level = seen < levels ? seen : levels - 1u;
    const unsigned long long same = ord_match<5>(level, valid);       // the lanes of this lane's level
    const uint32_t at = valid ? s_next[level] : 0u;
    __syncthreads();                                           // (every lane has read before a level's lowest lane advances its count)
    if (valid && (same & below) == 0ull) s_next[level] = at + (uint32_t)__popcll(same);
    __syncthreads();
    const uint32_t to = at + (uint32_t)__popcll(same & below);
    if (valid && to < O.n) { lod[to] = r; pos[j] = to; }       // (to < m by the scan: the comparison keeps a fault elsewhere inside the cloud's buffers)
  }
#else       // (as k_enc_order_hist: lane 0 places the tile's entries in their order)
  if (lane != 0) return;
  uint32_t next[ORD_LOD_LEVELS];
  for (uint32_t l = 0; l < levels; ++l) next[l] = hist[(size_t)l * O.tiles + T.tile];
  for (uint32_t j = e0; j < end; ++j) { const uint32_t to = next[pos[j]]++; lod[to] = kept[j]; pos[j] = to; }
#endif
}

// a thread per input row: row_entries from kept order to lod order
__global__ __launch_bounds__(256) void k_enc_lod_cells(uint8_t *arena, const EncOrder *clouds, const EncOrderTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncOrderTile T = tiles[blockIdx.x];
  const EncOrder &O = clouds[T.cloud];
  uint32_t e0, end;
  if (O.lod_bits == 0u || O.cells == 0 || !ord_tile(O, T, O.n, e0, end)) return;
  const uint32_t m = O.m < O.n ? O.m : O.n;
  uint32_t *cells = (uint32_t *)(arena + O.cells);
  const uint32_t *pos = (const uint32_t *)(arena + O.lod_rows) + O.n;
  for (uint32_t r = e0 + threadIdx.x; r < end; r += blockDim.x) { const uint32_t j = cells[r]; if (j < m) cells[r] = pos[j]; }
}

// ---- part_points (the header comment has the contract): grid = the chunk's (part, tile) pairs, one wave each
__global__ __launch_bounds__(WAVE) void k_enc_part_bounds(uint8_t *arena, const EncOrder *clouds, uint32_t nc, EncPart *parts, uint32_t np, const EncPartTile *tiles, uint32_t nt) {
  if (blockIdx.x >= nt) return;
  const EncPartTile T = tiles[blockIdx.x];
  if (T.part >= np) return;
  EncPart &P = parts[T.part];
  if (P.cloud >= nc) return;
  const EncOrder &O = clouds[P.cloud];
  const uint32_t t0 = T.tile * ORD_TILE;
  if (t0 >= P.n || P.lo > O.n || P.n > O.n - P.lo) return;       // (never by the layout: the comparisons keep a fault elsewhere inside the cloud's buffers)
  const int32_t *vals = (const int32_t *)(arena + O.vals);
  // (merge: the parts are runs of the kept rows; lod_bits: of the kept rows in (level, kept) order)
  const uint32_t *row = (const uint32_t *)(arena + ord_part_rows(O));
  const uint32_t lane = threadIdx.x, e0 = P.lo + t0, end = P.lo + (P.n - t0 < ORD_TILE ? P.n : t0 + ORD_TILE);
  int32_t mn[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, mx[3] = {(int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000};
#if defined(__HIPCC__)
  for (uint32_t e = e0 + lane; e < end; e += WAVE) {
    const uint32_t r = row[e];
    if (r >= O.n) continue;
    for (uint32_t c = 0; c < 3u; ++c) { const int32_t x = vals[3ull * r + c]; mn[c] = x < mn[c] ? x : mn[c]; mx[c] = x > mx[c] ? x : mx[c]; }
  }
  for (uint32_t c = 0; c < 3u; ++c)
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
      const int32_t a = __shfl_xor(mn[c], d, WAVE), b = __shfl_xor(mx[c], d, WAVE);
      mn[c] = a < mn[c] ? a : mn[c]; mx[c] = b > mx[c] ? b : mx[c];
    }
  if (lane == 0) for (uint32_t c = 0; c < 3u; ++c) { atomicMin(&P.qmin[c], mn[c]); atomicMax(&P.qmax[c], mx[c]); }
#else       // (as k_enc_order_hist: lane 0 takes the tile's entries in their order)
  if (lane != 0) return;
  for (uint32_t e = e0; e < end; ++e)
    for (uint32_t c = 0; c < 3u; ++c) { const int32_t x = vals[3ull * row[e] + c]; mn[c] = x < mn[c] ? x : mn[c]; mx[c] = x > mx[c] ? x : mx[c]; }
  for (uint32_t c = 0; c < 3u; ++c) { P.qmin[c] = mn[c] < P.qmin[c] ? mn[c] : P.qmin[c]; P.qmax[c] = mx[c] > P.qmax[c] ? mx[c] : P.qmax[c]; }
#endif
}

}  // namespace dsa
