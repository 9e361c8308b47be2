// Members of zzz_ctx (zzz_internal.h): the flags of its cached state, tier by tier, and its A/B knobs.
// What a context caches hangs on one ladder of dependencies:
//   mesh -> dofmap -> { Dirichlet set -> Dirichlet values ;  pattern -> matrix values -> operator stream and its special forms }
// The flags and small scalar facts of a tier are one plain struct, so that forgetting the tier is `ctx->tier = {}` (forget_*,
// zzz_api.hip) and a flag added later is forgotten with the rest.  Builders set their own flag when they finish.  Outside the tiers,
// untouched by a forget: the buffers (grow-only: hipFree waits for the whole device), the version counters and whatever is
// keyed on them or on its own content, the knobs, the once-per-context facts (*_lds_attr, streams, events, comm), the cube
// feed's description and the statistics of the last solve.
#pragma once
#include <cstdint>

namespace zzz
{
struct DofmapTier
{
  int order = 0, nd = 0; // order == 0: no dofmap, which every entry point that needs one tests before it launches anything
  // Internal locality numbering of the owned block dofs (zzz_renumber.hip): perm[internal] = caller index,
  // iperm[caller] = internal index; ghosts keep their places.  Everything on the device (cell_dofs, pattern, CSR,
  // vectors) is in internal order when `renumbered`; h_cell_dofs, h_dof_global stay in the caller's.
  bool renumbered = false;
  int renumber_kind = 0; // 0: not examined / left alone, 1: lattice key, 2: coordinate bins
  // ... and of the cells (simplex type by simplex type, lattice cube by lattice cube): h_cperm[internal] = caller cell.
  // cell_verts, cell_dofs and facet_mask on the device are in internal cell order when cells_renumbered.
  bool cells_renumbered = false;
  bool xq_valid = false;    // xq serves this dofmap (ensure_p1_coords)
  int adj_runs_n = -1;      // monotone runs of the connectivity: -1 not examined, 0 none usable / too many, else the count
  int64_t near_null_ld = 0; // leading dimension of near_null (0: no basis)
  int64_t nfacets = 0;
  bool have_coeff[2] = {false, false};
};
struct DirichletTier
{
  bool have_bc = false;     // a Dirichlet set: zzz_bc_upload, zzz_cube_generate
  bool have_bc_val = false; // ... and values of u0 for it (zzz_bc_values_upload)
};
struct PatternTier
{
  bool have_pattern = false;
  bool have_adj_li = false, have_asm_pos = false;
  bool have_cols16 = false, cols16_pending = false;
  bool have_tile_split = false, have_group_split = false, bw_have_split = false, bk_have_split = false;
  bool sp_bounds_ok = false;
  bool sp_crow_is_cap = false; // sp_crow = scan of the FULL row lengths padded to 8 (pattern-only)
  bool bw_struct_ok = false;
  // the path the build took (zzz_pattern_info): a report, read by nothing else
  bool adj_retry = false; // a window of the sort-free adjacency overflowed and this build started again with the sort
  int path_adjacency = 0; // 1 sort-free (monotone runs), 2 sorted from the start, 3 sorted after a window overflowed; 0: host
  int path_runs = 0;      // runs the adjacency was built from (0 unless path_adjacency == 1)
  int path_row_kernel = 0; // P1: 16 / 32, the cap of the thread-per-row kernel that sufficed; 0: a wavefront per row; -1: host
  int path_builder = 0;    // 0 device, 1 host after the device refused, 2 host by ZZZ_PATTERN=host
  int path_max_cols = 0;   // unique block columns of the longest block row
  int path_adj_source = 0; // adj_li / adjT written by 1 the P1 pattern kernel, 0 k_adjT_fill
};
struct ValuesTier
{
  bool have_matrix = false;
  bool sp_rownnz_fresh = false;  // sp_rownnz holds the non-zero counts of the CURRENT values (left by the matrix assembly)
  bool sp_compact_fresh = false; // ... and sp_cvals / sp_ccols the kept entries, rows at sp_crow (capacity-based starts)
  // the operator stream and its special forms
  bool have_sell = false;  // a stream, or a special form in its place, is built from the current CSR values
  bool sp_pending = false; // ... its size still on the way to the host (sellp_resolve)
  bool sp_generic = false; // the generic operator stream is packed for the current values (not when a special form was chosen at
                           // assembly time: sell_update; packed late by sellp_need_generic if a launch asks for it)
  bool sp_special_tried = false; // the special forms were built or declined for the current values
  bool sp_dict_done = false, sp_dict_on = false;
  bool sp_sd_on = false;
  bool sp_sd_all = false;    // every slice has its table (none stays doubles)
  bool sp_pal_on = false;    // the packed form serves the one-chunk kernel's launches (at least one slice is packed)
  bool sp_pipe_ok = false;   // every chunk is described by its slice's mode word: the pipelined product may run
  bool sp_one_chunk = false; // ... and no slice has more than one chunk (scalar P1 on a regular mesh)
  bool sp_pairs_ok = false;
  bool bk_on = false, bw_on = false;
  int sp_win_max = 0;       // doubles of LDS per workgroup the product launches with (0: no windowed group)
  int64_t sp_win_bytes = 0; // window bytes a product loads (all windowed groups)
  int64_t sp_chunks = 0, sp_kept = 0, sp_bytes = 0; // chunks of the stream, matrix entries kept in it, bytes a product reads from it
};
// A/B knobs, read once from the environment by zzz_ctx_create (read_knobs, zzz_api.hip); the defaults are the measured best
struct Knobs
{
  int sellp_mode = 1;           // ZZZ_SELLP: 0 off, 1 automatic, 2 natural row order always, 3 sorted rows always
  bool sellp_long_rows = false; // ZZZ_SELLP=4: natural order, always through the long-row packer (count / compact / fill)
  bool sellp_drop = true;       // ZZZ_SELLP_DROP=0: keep the exact zeros of the pattern in the stream
  int sellp_dict = 1;           // ZZZ_SELLP_DICT=0: no value dictionary
  int sellp_bwin = 1;           // ZZZ_SELLP_BWIN: 0 never, 1 by size (zzz_sellp_win.hip), 2 always
  bool sellp_early = true; // ZZZ_SELLP_EARLY=0: pack the generic stream at every assembly, special forms at the first product
  int sellp_blk = 1;       // ZZZ_SELLP_BLK=0: block size 3 stays on the generic product
  int sellp_pipe = 1;      // ZZZ_SELLP_PIPE=0: the generic product always
  int sellp_pal = 1;       // ZZZ_SELLP_PAL=0: never
  // ZZZ_SELLP_FORMS, a mask of the code-free chunk forms (default 7)
  bool sellp_align = true; // scalar rows, one-chunk slices: entries placed by column so that short boundary rows fit the affine form
  bool sellp_periodic = true; // block size 3: chunks whose columns are T[slot][row mod 3] + 3 (row div 3) carry no codes
  int sellp_tail = 1;    // bit 0: 8-bit codes of a narrow chunk go into the free tail of its value block; bit 1: no affine chunks
  bool asm_node3 = true; // ZZZ_ASM_NODE3=0: elasticity P1 matrix by the thread-per-scalar-row kernel (against asm_matrix_p1_node3)
  int cg_dinv_codes = 1; // ZZZ_CG_DINV_CODES: 0 never, 1 when the CG loop exceeds the Infinity Cache, 2 always,
                         // 3 always and 16-bit codes even where 8 bits would do
  int cg_xdefer = 1;     // ZZZ_CG_XDEFER: 0 never, 1 when the CG loop exceeds the Infinity Cache, 2 always
  int cg_xdefer_k = 4;   // ZZZ_CG_XDEFER_K: 2, 4 or 8
  bool cols16_enabled = true; // ZZZ_COLS16=0: the SpMV stays on the int32 columns; 10..13: the offset width ...
  int cols16_offb_forced = 0; // ... forced
  int spmv_lpr_forced = -1;   // ZZZ_SPMV_LPR: log2(lanes per row) of the SpMV row phase
  int spmv_variant = -1;      // ZZZ_SPMV_VARIANT: what ctx->spmv_variant starts as, with spmv_auto off (-1: unset)
  bool overlap = true;        // ZZZ_OVERLAP=0 disables the halo/compute overlap
  bool pipe_stream = true;    // ZZZ_CG_PIPE_STREAM=0: the all-reduce of the pipelined CG stays on the main stream
};
} // namespace zzz
