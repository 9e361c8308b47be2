// Internal declarations of libzzz_hip.so (not part of the ABI; see include/zzz_abi.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/zzz_abi.h"

// One term of the Chebyshev-Jacobi polynomial (cheb_terms, zzz_cg.hip) as the epilogue of the product of d: with
// w_i = (A d)_i in the lane that owns row i,  g_i -= D^-1_ii w_i;  d'_i = c1 d_i + c2 g_i (written to the product's
// output vector);  z_i += d'_i.  The last term leaves g and d alone and sums <r,z> and the test norm into the
// partial arrays at strides 1 and 2.  dinv == null: the plain product.
struct ChebEpi
{
  const double* dinv = nullptr;
  double* g = nullptr;
  double* z = nullptr;
  const double* r = nullptr;
  double c1 = 0.0, c2 = 0.0;
};

namespace zzz
{
// ---- device buffer -------------------------------------------------------------------------
template <typename T>
struct DevBuf
{
  T* p = nullptr;
  size_t n = 0;   // elements in use
  size_t cap = 0; // elements allocated
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    n = cap = 0;
  }
  // Contents are NOT preserved.  An existing allocation is reused when it is large enough (and not
  // more than twice too large): hipFree/hipMalloc of GB-sized buffers cost milliseconds each and a
  // re-assembly of the same problem asks for the same sizes again.
  // Grows only: an existing allocation of at least `count` elements is kept whatever its size (the solvers' history
  // arrays: a short estimate solve inside a long one must not free and re-allocate them -- hipFree waits for the
  // whole device, other contexts' kernels included).
  hipError_t reserve(size_t count)
  {
    if (p && cap >= count)
    {
      n = count ? count : 1;
      return hipSuccess;
    }
    return alloc(count);
  }
  // Scratch that may be asked for while ANOTHER context's kernel is waiting for this one (two ranks on one GPU: the other rank
  // polls its all-reduce mailbox inside a kernel while this one still builds its product form): grows only, and a buffer that
  // is too small is RETIRED -- handed to `retired`, freed with the context -- not freed: hipFree waits for every kernel on the
  // device, i.e. for the poll's time-out.  The primitives' shared scratch is only ever sized through this (zzz_prim.h).
  hipError_t grow_keep(size_t count, std::vector<void*>& retired)
  {
    if (count == 0)
      count = 1;
    if (p && cap >= count)
    {
      n = count;
      return hipSuccess;
    }
    if (p)
      retired.push_back(p);
    p = nullptr;
    n = cap = 0;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess)
      n = cap = count;
    return e;
  }
  hipError_t alloc(size_t count)
  {
    if (count == 0)
      count = 1;
    if (p && cap >= count && cap <= 2 * count + 1024)
    {
      n = count;
      return hipSuccess;
    }
    release();
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess)
      n = cap = count;
    return e;
  }
};

struct Comm; // zzz_comm.cpp
struct MgHier; // zzz_mg.hip: the level hierarchy of ZZZ_PC_MG, ZZZ_PC_PMG and ZZZ_PC_AGG
struct AggLevel; // zzz_agg.hip: the aggregates of one level of ZZZ_PC_AGG and the Galerkin sum to the next
struct SaggLevel; // zzz_sagg.hip: the smoothed prolongator of one level of ZZZ_PC_SAGG and the two products to the next

typedef int64_t rp_t; // row pointers of the CSR matrix of record

constexpr int SPMV_PSTRIDE = 4096; // distance between the three partial arrays of the single-reduction SpMV
constexpr int SPMV_TILE_NNZ = 2048; // most nonzeros in one tile of the CSR SpMV (zzz_spmv.hip)

// CG scalars kept on the device so the iteration loop never waits for the host.
struct CgState
{
  int converged; // 0 running, 1 converged, 2 broke down (non-finite)
  int iters;     // iteration count at convergence
  double dp0;    // initial norm (variant PETSC) or <r0,r0> (variant CGH)
  double ttol;   // max(rtol*dp0, atol)
  double dp;     // last norm
  int conv_it1;  // 0 running, else (iteration of the launch that set `converged`) + 1: one word, so a
                 // workgroup can tell "stopped by an EARLIER launch" from "being stopped by this one"
  int pad;
};

struct CgParams
{
  int variant, pc, norm;
  double rtol, atol, dtol;
};

// Plan of the matrix-free action (zzz_matfree.hip): the cells in blocks of `nc` (contiguous in the Morton order of their
// centroids), every block with the list of the dofs it touches, 16-bit block-local indices per cell and, per (cell,
// local dof), the RANK of that incidence among the cells of its step that touch the same dof -- the order in which
// the contributions are added in LDS.  Built once per mesh / dofmap / Dirichlet set.
struct MfPlan
{
  bool valid = false, failed = false;
  int bs = 1;                               // values per block dof: 1 (Poisson form M) or 3 (elasticity form a)
  int nd = 0, nc = 0, threads = 0, nsb = 0; // dofs per cell; cells per block; workgroup size; steps per block (nc / threads)
  int ndw = 0, nrw = 0;                     // 32-bit words of indices / of ranks per cell
  int64_t nblocks = 0, nshared = 0, nslots = 0;
  int nloc_max = 0;
  int64_t bytes_per_action = 0; // what one action addresses (plan streams + vectors)
  DevBuf<int32_t> hdr;          // [block][8]: dof_off, nloc, n_int, n_sh, part_off, 0, 0, 0
  DevBuf<int32_t> dof_ids;      // block-local dof lists: interior | shared with other blocks | ghost, ascending inside
  DevBuf<uint8_t> dof_flag;     // Dirichlet marker of each list entry
  DevBuf<double> xyz;           // P1: coordinates of each list entry
  DevBuf<uint32_t> idxw, rnkw;  // [block][word][cell of the block]
  DevBuf<uint8_t> rmax;         // [block][step][4 nrw]: rounds needed by local dof i in that step
  DevBuf<double> geom;          // P2/P3: [block][6][cell]  |detJ| K K^T
  DevBuf<int32_t> gid;          // P3: [block][nd][cell] global dofs (u is gathered from memory, not staged)
  DevBuf<double> dtab;          // P2/P3: the factorised reference tables (ZZZ_DTAB_P2/P3)
  DevBuf<double> ypart;         // partial sums of the shared dofs, [slot]
  DevBuf<int32_t> sh_dof, sh_off, sh_slot; // shared dofs; where their partial sums start; (block, shared entry) -> slot
  DevBuf<uint8_t> sh_flag;                 // Dirichlet marker of each shared dof
  DevBuf<int32_t> mf_cell;      // [block][cell] -> cell of the context (-1: none), kept for rebuilding the geometry
  // single precision (zzz_action_f32, zzz_cg_solve_f32): float twins of the VALUE arrays alone -- every index array above
  // serves both scalars.  Built by the first float action of a plan, stale as soon as the plan is rebuilt.
  bool f32_built = false;
  int64_t nu = 0;                   // entries of the block-local dof lists
  int64_t bytes_per_action_f32 = 0; // what one float action addresses
  DevBuf<float> xyz32;              // P1: coordinates relative to the block's origin (subtracted in double): the block's first
                                    // listed dof where that serves every cell of the block, else the second origin of zzz_mf_elem.h
  DevBuf<float> geom32, dtab32;     // P2/P3: geom and dtab rounded
  DevBuf<float> ypart32;            // partial sums of the shared dofs
};
} // namespace zzz

#include "zzz_valset.h" // (after DevBuf: a set owns four of them)
#include "zzz_tiers.h"  // the flags of the context's cached state, tier by tier, and its knobs

struct zzz_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  zzz::Knobs knob;
  zzz::DofmapTier dofmap; // the cached state's flags, tier by tier (zzz_tiers.h); each tier's buffers follow under its heading
  zzz::DirichletTier dirichlet;
  zzz::PatternTier pattern;
  zzz::ValuesTier values;

  // ---- mesh
  int64_t nverts = 0, ncells = 0;
  zzz::DevBuf<double> x;           // nverts*3
  zzz::DevBuf<int32_t> cell_verts; // ncells*4
  std::vector<int32_t> h_cell_verts;

  // ---- dofmap
  int bs = 0;
  int64_t n_owned = 0, n_ghost = 0; // block dofs
  zzz::DevBuf<int32_t> cell_dofs;   // ncells*nd
  std::vector<int32_t> h_cell_dofs;
  // global indices of the local block dofs / vertices (zzz_global_ids_upload): only the ghost-layer build needs them
  std::vector<int64_t> h_dof_global, h_vert_global;
  int64_t owned_cells = 0; // cells the caller uploaded, when zzz_ghost_layer_build has appended ghost cells
  zzz::DevBuf<int32_t> perm, iperm; // the internal numbering (dofmap.renumbered, dofmap.cells_renumbered)
  std::vector<int32_t> h_perm, h_iperm, h_cperm;
  std::vector<uint16_t> csr_slot; // caller CSR entry -> position inside its internal row (built on first CSR download)
  // P1: vertex coordinates addressed by BLOCK DOF (ensure_p1_coords): the assembly kernels then read one connectivity
  // table, not two.  Points at x when the dofmap numbers dofs as the mesh numbers vertices, else at xdof.
  zzz::DevBuf<double> xdof;
  const double* xq = nullptr;
  zzz::DevBuf<uint8_t> facet_mask; // exterior-facet mask per cell (bit f = local facet f is exterior)
  zzz::DevBuf<double> coeff[2];
  zzz::DevBuf<double> near_null; // the six orthonormalised rigid-body modes (zzz_nullspace.hip), [6][dofmap.near_null_ld]
  // reference tensors of the element (element_tables.inc), for orders 2 and 3; keyed on their own content
  zzz::DevBuf<double> tables;
  int tables_order = 0;
  std::vector<std::pair<const void*, size_t>> lds_raised; // kernels whose dynamic-LDS limit this context raised, and to what

  // ---- Dirichlet set (bc: marker per local scalar dof, owned + ghost) and its values
  zzz::DevBuf<uint8_t> bc;
  // values of u0 at the constrained dofs (zzz_bc_values_upload): nloc * bs doubles in the device's numbering; only the
  // entries whose marker is set are ever read.  Forgotten by everything that changes the dof layout or the Dirichlet set.
  zzz::DevBuf<double> bc_val;
  uint64_t bc_version = 0; // counts Dirichlet sets (zzz_dofmap_upload, zzz_bc_upload, zzz_cube_generate)
  zzz::DevBuf<double> b_masked; // the matrix-free solve's right-hand side with its constrained entries zeroed (zzz_cg.hip)
  // ---- dofmap AND Dirichlet set: the plan of the matrix-free action (forgotten by forget_bc, and through it by forget_dofmap)
  zzz::MfPlan mf;
  // ---- pattern AND Dirichlet set, keyed on the versions of both: the lifting pass (zzz_assemble.hip: k_lift): the owned
  // unconstrained scalar rows whose pattern row holds a constrained column, ascending; built by the first lifted assembly of
  // a (pattern, Dirichlet set) pair and kept until either changes
  zzz::DevBuf<int32_t> lift_rows;
  zzz::DevBuf<uint8_t> lift_flag; // scratch of the build (kept: a rebuild asks for the same size)
  int64_t n_lift_rows = 0;
  uint64_t lift_pattern_version = ~0ull, lift_bc_version = ~0ull;

  // ---- pattern (owned rows) + adjacency
  int64_t nrows = 0, ncols = 0, nnz = 0;
  zzz::DevBuf<zzz::rp_t> rowptr; // 64-bit: 50 M P3 dofs carry 2.4 G nonzeros on one GPU
  zzz::DevBuf<int32_t> cols;
  zzz::DevBuf<double> vals;
  // scratch of the pattern build (kept: a rebuild of the same problem reuses it)
  zzz::DevBuf<int32_t> scr_keys_out, scr_vals_in, scr_cnt, scr_stage;
  int64_t scr_cell_of_n = -1; // scr_vals_in holds position / nd for this many connectivity entries ...
  int scr_cell_of_nd = 0;     // ... of nd dofs per cell
  zzz::DevBuf<int64_t> scr_bptr;
  // monotone runs of the connectivity (zzz_pattern.hip, adjacency without a sort): per run {local dof index k, first
  // cell, end cell}; found once per dofmap (dofmap.adj_runs_n)
  zzz::DevBuf<int32_t> adj_runs, adj_run_lo, adj_win_base;
  int32_t* adj_flag_host = nullptr; // pinned: "a window did not fit" travels here behind the build's kernels
  zzz::DevBuf<unsigned char> scr_tmp; // the device primitives' shared scratch: zzz_prim.h alone touches it
  std::vector<void*> retired; // device buffers replaced by larger ones while another context's kernel may be waiting (DevBuf::grow_keep)
  zzz::DevBuf<int32_t> adj_off, adj_cells; // owned block dof -> incident cells (ascending)
  zzz::DevBuf<int32_t> adjT_off, adjT_cells; // the same lists transposed in 64-row slices (dense wave reads)
  zzz::DevBuf<uint8_t> adj_li;             // local index of the dof in each of those cells, same layout
  zzz::DevBuf<double> cell_w;              // matrix-free: Ae_c u_c per cell, component-major
  // P2/P3: position inside its CSR row of every (adjacency entry, local column) pair -- a by-product of the pattern
  // build's sort (the candidates carry their origin through it), so that the matrix assembly adds without searching
  zzz::DevBuf<uint16_t> asm_pos;
  zzz::DevBuf<double> cell_geom; // P2/P3 matrix assembly: per cell |detJ| K K^T (6 doubles) or |detJ|, K (10), evaluated once per assembly
  int max_row_nnz = 0;
  // SpMV tiling (row-aligned tiles of the nonzero stream)
  zzz::DevBuf<double> alpha_hist; // step lengths: x += alpha_k p_k is applied by the NEXT direction update
  zzz::DevBuf<int32_t> tile_row;
  zzz::DevBuf<uint16_t> cols16;   // 16-bit column codes for the SpMV (k_tile_encode_cols); cols stays the matrix of record
  zzz::DevBuf<int32_t> tile_base; // band bases: 2^(16-cols16_offb) per tile
  zzz::DevBuf<int32_t> scr_c16;   // fallback-tile counter
  int cols16_offb = 12;
  int64_t cols16_fallback_tiles = 0;
  int64_t ntiles = 0;
  // tiles of a partitioned matrix split by "references a ghost column" (halo/compute overlap)
  zzz::DevBuf<int32_t> tiles_interior, tiles_boundary;
  int64_t n_tiles_interior = 0, n_tiles_boundary = 0;
  int spmv_lpr_shift = 0; // log2(lanes per row) of the SpMV row phase
  bool spmv_auto = true; // choose bit 0 from the matrix size (off when ZZZ_SPMV_VARIANT / zzz_spmv_time force one)
  int spmv_variant = 1;  // bit 0: non-temporal matrix loads, bit 1: unused,
                         // bit 3: the sliced-ELL operator stream (zzz_sellp.hip) instead of the CSR tile kernel
  // Operator stream of the CG SpMV (zzz_sellp.hip): sliced-ELL copy in chunks of 8 entries per row, exact zeros
  // dropped, 16-bit slot-relative column codes; rebuilt from the CSR values after every assembly
  zzz::DevBuf<int32_t> sp_rownnz, sp_nch, sp_chunk_off, sp_perm, sp_codes32, sp_meta, sp_desc, sp_counter;
  // long rows: compacted copy of the kept entries, rows starting at multiples of 8 (k_sp_compact / k_sp_fill_c)
  zzz::DevBuf<int64_t> sp_crow;
  zzz::DevBuf<double> sp_cvals;
  zzz::DevBuf<int32_t> sp_ccols;
  zzz::DevBuf<uint8_t> sp_gflag;
  hipEvent_t sp_event = nullptr;
  bool sp_forced = false, sp_lds_attr = false;
  int sp_max_range = 0;       // longest CSR range of a 64-row slice
  int64_t sp_chunk_bound = 0; // chunks of the natural-order stream if no entry were zero
  zzz::DevBuf<uint16_t> sp_codes16;
  zzz::DevBuf<double> sp_vals;
  zzz::DevBuf<unsigned long long> sp_smode; // per slice: two bits per chunk, what a product loads for its columns (zzz_sellp.h)
  zzz::DevBuf<uint8_t> sp_pairs;            // one-chunk streams: slices 2 p and 2 p + 1 form an affine pair (zzz_sellp_pipe.hip)
  // one-chunk streams on the stream dictionary in LDS: a slice none of whose eight slots holds more than 16 distinct value
  // codes in its 64 rows is also kept PACKED (k_sp_pal_build, zzz_sellp_dict.hip): 512 B per chunk in sp_pal, entry l (8 B) =
  // {row l's eight 4-bit palette indices, slot e at bits 4 e; palette codes 2 l and 2 l + 1 of the slice's 8 x 16, ascending
  // per slot}.  sp_palok[slice] = 1: packed.  sp_vcode stays whole beside it (generic kernel, unpacked slices).
  zzz::DevBuf<uint2> sp_pal;
  zzz::DevBuf<uint8_t> sp_palok;
  zzz::DevBuf<int32_t> sp_pal_info;         // [0] packed slices, [1] largest count of distinct codes in a (slice, slot), [2] mixed pairs
  int64_t sp_pal_packed = 0, sp_pal_mixed = 0;
  int sp_pal_maxcount = 0;
  int64_t nslices = 0;
  zzz::DevBuf<uint8_t> sp_wlast; // per slice: entries of the longest row in its last chunk (1..8)
  // value dictionary of the stream (zzz_sellp.hip, sp_dict_build): the matrices of a regular mesh hold a few hundred to a few
  // ten thousand DISTINCT values (10 M-dof P1 Poisson: ~1 300); where there are at most 65 535 the product reads a 16-bit
  // code per entry (sp_vcode: [chunk][lane][8]) and looks the value up (sp_dset.dict: code 0 = +0.0) -- the same doubles in the
  // same order, a quarter of the bytes.  More distinct values (an unstructured mesh): sp_dict_on stays false, sp_vals is read.
  zzz::DevBuf<uint16_t> sp_vcode;
  zzz::ValSet<18, 1> sp_dset;        // the values' set, dictionary (dict: code 0 = +0.0) and counters (zzz_valset.h)
  zzz::DevBuf<int32_t> sp_dict_info; // [0..1] bytes a product reads in dictionary form, [2] slices that stay doubles (sp_sd_build)
  // per-slice dictionaries (long rows: k_sp_sd_build): 16-bit codes [chunk][lane][8], tables [slice][1024], entries per slice
  zzz::DevBuf<uint16_t> sp_vcode8;
  zzz::DevBuf<double> sp_sd_vals;
  zzz::DevBuf<int32_t> sp_sd_info;
  zzz::DevBuf<int64_t> sp_sd_off; // where slice s's table starts in sp_sd_vals (the tables back to back, at even entries)
  int64_t sp_sd_bytes = 0;
  // Jacobi's inverse diagonal as 8- or 16-bit codes (zzz_cg.hip, DinvCodes)
  zzz::ValSet<14, 0> dd_set;
  zzz::DevBuf<uint16_t> dd_codes; // (8-bit codes: the first half of it, one byte per entry)
  int last_solve_dinv_codes = 0;  // distinct values of the inverse diagonal when the last solve ran on codes, else 0
  int last_solve_dinv_bits = 0;   // ... and the width of a code, 8 or 16 (0 without codes)
  // the classical loop's solution update applied once per K iterations from a ring of K direction vectors (zzz_cg.hip,
  // k_update_p_light / _flush): slot 0 of the ring is `p`, these are slots 1 .. K-1
  zzz::DevBuf<double> p_ring[7];
  int last_solve_xdefer_k = 1;    // the ring's length in the last solve (1: x updated in place in every iteration)
  int sp_dict_n = 0;        // distinct values (with +0.0)
  int64_t sp_dict_bytes = 0; // bytes a product reads from the stream in dictionary form
  bool sp_sorted = false;    // rows ordered by length inside windows (SELL-C-sigma)
  zzz::DevBuf<int32_t> groups_interior, groups_boundary; // groups of 4 slices without / with ghost columns
  // block-window form of the product for long scalar rows (zzz_sellp_win.hip): rows in the Morton order of their nodes, blocks of
  // 4 096 with the columns they reach as a window in LDS and a dictionary of their values
  zzz::DevBuf<int32_t> bw_order, bw_perm, bw_desc, bw_wlist, bw_blk_chunks, bw_blk_wn, bw_dnum, bw_info, bw_list_interior, bw_list_boundary;
  zzz::DevBuf<int64_t> bw_chunk0, bw_woff;
  zzz::DevBuf<uint16_t> bw_ccode, bw_vcode, bw_hcode;
  zzz::DevBuf<uint32_t> bw_cpack, bw_vpack; // the same codes packed, 12 B per lane and chunk (where the block's flag says so)
  zzz::DevBuf<uint8_t> bw_cflag, bw_vflag;
  int64_t bw_packed_planes = 0;
  zzz::DevBuf<uint32_t> bw_key, bw_key2, bw_skey; // (bw_skey: a block's rows by length, pass 1 to pass 2 of the structure)
  zzz::DevBuf<int32_t> bw_val, bw_hid, bw_first; // (scratch of the builders, kept: hipFree waits for the whole device)
  zzz::DevBuf<double> bw_dofx, bw_bbox;
  zzz::DevBuf<double> bw_dict;
  zzz::DevBuf<uint8_t> bw_gflag;
  bool bw_lds_attr = false;
  int32_t bw_nblk = 0;
  int64_t bw_chunks = 0, bw_window_entries = 0, bw_dict_entries = 0, bw_bytes = 0, bw_n_interior = 0, bw_n_boundary = 0;
  uint64_t pattern_version = 0, bw_struct_version = ~0ull; // pattern_version counts zzz_csr_pattern_build calls
  // block-row form of the product for block size 3 (zzz_sellp_blk.hip): one lane per node, 16-bit codes into a table of the
  // matrix's distinct 3 x 3 blocks (copied into LDS by every workgroup), 16 block slots per node and chunk
  zzz::DevBuf<int32_t> bk_desc, bk_meta, bk_flags, bk_nch, bk_c0, bk_slot_code, bk_info, bk_list_interior, bk_list_boundary;
  zzz::DevBuf<uint16_t> bk_code, bk_ccode, bk_rows16;
  zzz::ValSet<13, 1> bk_vset; // form 2: the table's distinct values
  int bk_form = 1, bk_ndict = 0; // 1: the table's rows (nine doubles) in LDS; 2: rows of value offsets in memory, the values in LDS
  zzz::DevBuf<double> bk_tab;
  zzz::DevBuf<unsigned long long> bk_hash_tag, bk_hash_tag2, bk_hash_owner;
  zzz::DevBuf<int32_t> bk_park; // per block of the matrix: its slot in the set (-1: a zero block), k_bk_insert to k_bk_fill
  zzz::DevBuf<uint8_t> bk_gflag;
  bool bk_lds_attr = false;
  int bk_entries = 0;      // entries of the block table (the zero block included)
  int64_t bk_chunks = 0, bk_slices = 0, bk_bytes = 0, bk_n_interior = 0, bk_n_boundary = 0;
  int64_t n_groups_interior = 0, n_groups_boundary = 0;
  // assembly tiling: contiguous owned block-dof ranges whose CSR segment fits LDS
  zzz::DevBuf<int32_t> asm_tile;
  int64_t n_asm_tiles = 0;
  bool tiles_ok = true; // false: 2^31 nonzeros or more -- the CSR tile kernel (32-bit tile windows) is not available,
                        // the product must run on the operator stream

  // vectors, (n_owned+n_ghost)*bs each
  zzz::DevBuf<double> b, u, r, z, p, w, dinv;
  // reductions
  zzz::DevBuf<double> part_a, part_b, red; // block partials; reduced scalars
  zzz::DevBuf<double> beta_hist, dp_hist, dpi_hist;
  zzz::DevBuf<double> sr_s; // single-reduction CG: s = A z
  // pipelined CG (zzz_cg_pipe.hip): m = D^-1 w with its ghost entries, n = A m, and the block partials of the three sums in
  // two sets (an iteration's kernel reads one and leaves the next iteration's in the other)
  zzz::DevBuf<double> pipe_m, pipe_n, pipe_parts;
  zzz::DevBuf<double> cheb_d, cheb_d2, cheb_g; // Chebyshev-Jacobi: the polynomial's direction (two buffers: fused terms
                                               // write the next one while lanes still gather the old) and residual
  zzz::DevBuf<double> cheb_noise; // ... and the right-hand side of its spectrum estimate
  zzz::DevBuf<zzz::CgState> state;
  zzz::CgState* h_state = nullptr; // pinned
  std::vector<double> history;
  int last_iters = 0;
  int last_reason = 0; // KSPConvergedReason of the last solve (zzz_cg_info)
  // x windows of the operator stream (zzz_sellp.hip: k_sp_windows): per group of four slices the columns its rows reach,
  // as a few contiguous segments that fit LDS; the stream's column codes of such a group are LDS indices
  zzz::DevBuf<int32_t> sp_win_info; // [group] = {segments (0: the group gathers from memory), window length in doubles}
  zzz::DevBuf<int32_t> sp_win_seg;  // [group][SP_WIN_NSEG] = {first column, length}
  bool halo_pending = false; // comm_halo_begin put an exchange on the comm stream: comm_halo_end waits for it
  // linalg::cg in float (zzz_cg_f32.hip): x, r, p, y of src/cg.h:38-86 with U = float; grow-only, never freed by a solve
  zzz::DevBuf<float> f32_x, f32_r, f32_p, f32_y;
  // ZZZ_PC_CHEBYSHEV_JACOBI: the spectrum bound of the matrix as it stands (Gershgorin and Lanczos estimate cost ~10 products
  // and ~20 all-reduces: taken once per set of matrix values, not once per solve); mat_version counts assemblies / uploads
  uint64_t mat_version = 0;
  struct ChebKey // what cheb_hi was computed from
  {
    uint64_t mat_version = ~0ull;
    int est_its = 0;
    bool operator==(const ChebKey& k) const { return mat_version == k.mat_version && est_its == k.est_its; }
  } cheb_key;
  double cheb_hi = 0.0;
  double last_pc_bound = 0.0; // ZZZ_PC_CHEBYSHEV_JACOBI: the spectrum bound the last solve used

  // profiling
  std::vector<hipEvent_t> ev;
  double prof_spmv_ms = 0.0;
  int64_t prof_spmv_n = 0;
  // exposed halo wait of the overlapped product (time between the end of the interior launch and the arrival of the
  // halo, on the main stream), sampled on the iterations whose product is timed
  std::vector<hipEvent_t> ev_halo;
  bool prof_now = false; // set by the CG loop around a timed product launch
  int prof_halo_n = 0;
  double prof_halo_wait_ms = 0.0;

  // multi-GPU
  zzz::Comm* comm = nullptr;
  int nneigh = 0;
  std::vector<int32_t> neigh_rank;
  std::vector<int64_t> send_off, recv_cnt;
  zzz::DevBuf<int32_t> send_idx;
  zzz::DevBuf<double> send_buf;
  std::vector<int64_t> send_contig; // per neighbour: first owned block dof when its list is a contiguous range, else -1
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_x_ready = nullptr, ev_halo_done = nullptr;
  // the all-reduce that overlaps a product (comm_reduce_begin / comm_reduce_end): its own stream and events
  hipStream_t red_stream = nullptr;
  hipEvent_t ev_parts_ready = nullptr, ev_red_done = nullptr;
  bool red_pending = false;
  bool last_solve_red_overlapped = false; // the last solve's all-reduces went to red_stream (zzz_cg_info)

  // ZZZ_PC_MG (zzz_mg.hip): the cube this context's feed was generated from by zzz_cube_generate (cleared by every
  // upload of mesh, dofmap, Dirichlet set or facets; feed_version counts all of them), and the hierarchy built on it
  bool cube_feed = false;
  int cube_problem = 0, cube_nparts = 0, cube_part = 0;
  int64_t cube_n[3] = {0, 0, 0};
  uint64_t feed_version = 0;
  zzz::MgHier* mg = nullptr;
  int mg_products = ZZZ_MG_PRODUCTS_LISTS; // zzz_mg_products: how ZZZ_PC_SAGG / ZZZ_PC_SAGG_RBM form their products; survives every upload
  bool stream_borrowed = false; // a coarse level of another context's hierarchy: `stream` is that context's

  int64_t nloc() const { return (n_owned + n_ghost) * bs; }
};

namespace zzz
{
int fail(zzz_ctx* ctx, int code, const char* fmt, ...);
void set_global_error(const char* msg);

#define ZZZ_HIP(ctx, call)                                                                                            \
  do                                                                                                                  \
  {                                                                                                                   \
    hipError_t e_ = (call);                                                                                           \
    if (e_ != hipSuccess)                                                                                             \
      return zzz::fail(ctx, ZZZ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Code objects are loaded lazily, one per translation unit, by the first launch of any of its kernels: 10-27 ms each,
// which a one-shot run (the reference runs every phase once, src/main.cpp:152-211) would book under whatever ZZZ timer
// that launch happens to sit in.  Every translation unit with device code defines an empty kernel whose attributes
// zzz_ctx_create asks for: that loads the unit's code object there, before any timed phase.
#define ZZZ_PRELOAD_TU(name)                                                                                          \
  __global__ void k_preload_##name() {}                                                                               \
  void preload_##name()                                                                                               \
  {                                                                                                                   \
    hipFuncAttributes a;                                                                                              \
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_preload_##name));                                 \
  }
void preload_agg();
void preload_assemble();
void preload_cg();
void preload_cg_pipe();
void preload_cg_f32();
void preload_comm();
void preload_cubegen();
void preload_matfree();
void preload_mg();
void preload_nullspace();
void preload_pmg();
void preload_pattern();
void preload_renumber();
void preload_sagg();
void preload_sagg_rbm();
void preload_sagg_rows();
void preload_sellp();
void preload_sellp_dict();
void preload_sellp_pack();
void preload_sellp_pipe();
void preload_sellp_blk();
void preload_sellp_win();
void preload_spmv();

// api
int alloc_problem_vectors(zzz_ctx* ctx);
// A context without mesh or dofmap takes the CSR that its rowptr / cols / vals already hold (zzz_agg.hip's coarse levels):
// nnodes block dofs of bs components in identity order, no ghosts, no Dirichlet rows; tiles, vectors and product stream
// as zzz_csr_pattern_build and an assembly leave them.  ctx_adopt_values: the values alone were rewritten -- the one
// sequence behind every assembly and upload: mat_version, forget_values, the operator stream, have_matrix.
int ctx_adopt_csr(zzz_ctx* ctx, int bs, int64_t nnodes, int64_t nnz, int max_row_nnz);
int ctx_adopt_values(zzz_ctx* ctx, bool assembled = false); // assembled: launch_assemble_matrix wrote them, and its by-products
// The one forget path, nested along the ladder of the tiers: an entry point that replaces an input calls the function of
// that input's tier, after its argument checks and before it writes, and everything behind the input is what a fresh
// context holds.  forget_mesh > forget_dofmap > { forget_bc > forget_bc_values ; forget_pattern > forget_values }.
void forget_mesh(zzz_ctx* ctx);
void forget_dofmap(zzz_ctx* ctx);
void forget_bc(zzz_ctx* ctx);
void forget_bc_values(zzz_ctx* ctx); // (counts in bc_version: the lifting rows are rebuilt)
void forget_pattern(zzz_ctx* ctx);
void forget_values(zzz_ctx* ctx);
// pattern (zzz_pattern.hip)
int pattern_build_device(zzz_ctx* ctx, bool* fallback);
void pattern_reserve(zzz_ctx* ctx); // scratch sized by the dofmap, reserved at upload time
int build_tiles_device(zzz_ctx* ctx, int max_block_cols);
int ensure_cols16(zzz_ctx* ctx); // encodes the 16-bit column stream of the CSR tile kernel on first use
int asm_tile_nnz(const zzz_ctx* ctx); // nonzeros an assembly tile may hold (LDS budget of the matrix kernels)
int build_adjT(zzz_ctx* ctx);
int dof_coords_device(zzz_ctx* ctx, DevBuf<double>& dofx, DevBuf<int32_t>& first); // zzz_nullspace.hip
int build_adjT_offsets(zzz_ctx* ctx);
int ensure_tables(zzz_ctx* ctx);
int ensure_p1_coords(zzz_ctx* ctx); // P1 only; a no-op for P2/P3
// internal numbering (zzz_renumber.hip)
int renumber_build(zzz_ctx* ctx);
void to_internal(const zzz_ctx* ctx, const double* in, double* out, bool owned_only);
void to_caller(const zzz_ctx* ctx, const double* in, double* out, bool owned_only);
int csr_to_caller(zzz_ctx* ctx, std::vector<zzz::rp_t>& rowptr_c, int32_t* cols_c, double* vals_c, bool need_cols);
int csr_values_to_internal(zzz_ctx* ctx, const double* vals_c, std::vector<double>& vals_i);
// kernels_spmv
// The five forms of a product y = A x: with the per-workgroup partial sums of <x, y> (DOT), with those of <r, x> and of the
// test norm beside them (SR, single-reduction CG), as a term of the Chebyshev-Jacobi polynomial (ChebEpi), the last term
// with its sums.  Every product kernel's table of instantiations (tile_kernels, sp_kernels, ...) is indexed by this and
// by the load policy of the matrix stream, the non-temporal loads first.
enum ProductMode { PM_DOT_SR, PM_DOT, PM_PLAIN, PM_CHEB_DOT, PM_CHEB, PM_COUNT };
enum ProductLoad { LOAD_NT, LOAD_PLAIN };
// One product as its launchers see it: what the caller asked for and the selection made from it, once per product
struct ProductCall
{
  const double* x = nullptr;
  double* y = nullptr;
  double* partials = nullptr;    // != null: the product also leaves partial sums (the DOT forms)
  const int* stop = nullptr;     // CgState::converged: a product with sums is skipped once it is set
  const int32_t* list = nullptr; // != null: only the nlist listed items (interior or boundary part of a partitioned matrix)
  int64_t nlist = 0;
  const double* rvec = nullptr;
  int nn_is_rr = 0;
  const ChebEpi* epi = nullptr;
  ProductMode mode = PM_PLAIN;
  ProductLoad load = LOAD_PLAIN; // set by the driver of the kernel family: each has its own size rule
  int special = 0;               // operator stream: 1 the block-row kernel serves the call, 2 the block-window kernel
};
inline ProductCall product_call(const zzz_ctx* ctx, const double* x, double* y, double* partials, const double* rvec, int nn_is_rr,
                                const ChebEpi* epi)
{
  ProductCall c;
  c.x = x;
  c.y = y;
  c.epi = epi;
  if (partials)
  {
    c.partials = partials;
    c.stop = reinterpret_cast<const int*>(ctx->state.p);
    c.rvec = rvec;
    c.nn_is_rr = nn_is_rr;
  }
  c.mode = epi ? (partials ? PM_CHEB_DOT : PM_CHEB) : partials ? (rvec ? PM_DOT_SR : PM_DOT) : PM_PLAIN;
  return c;
}
typedef void (*ProductLauncher)(zzz_ctx* ctx, int grid, const ProductCall& c);
// the interior or the boundary part of a partitioned product: its items, their list and its workgroups (0 where n is 0)
struct ProductPart
{
  int64_t n;
  const int32_t* list;
  int grid;
};
// y = A x on this rank's matrix as it stands (x has ncols entries, ghosts in place), optionally per-block partials of
// <x_owned, y>; epi (operator stream only): the product carries a Chebyshev term
int launch_spmv(zzz_ctx* ctx, const double* x, double* y, double* partials, int* npartials, const double* rvec = nullptr,
                int nn_is_rr = 0, const ChebEpi* epi = nullptr);
// ... on a possibly partitioned operator: the forward halo of x first, overlapped with the interior part where the
// partition is split (ZZZ_OVERLAP), blocking otherwise
int launch_product(zzz_ctx* ctx, double* x, double* y, double* partials, int* npartials, const double* rvec = nullptr,
                   int nn_is_rr = 0, const ChebEpi* epi = nullptr);
// halo begin / interior launch / halo end / boundary launch (its partials behind the interior's) / number of partials
int launch_overlapped(zzz_ctx* ctx, double* x, ProductCall c, const ProductPart& in, const ProductPart& bd, ProductLauncher launch,
                      int* npartials);
// operator stream (zzz_sellp.hip)
int sell_update(zzz_ctx* ctx); // (ctx_adopt_values alone calls it, behind forget_values)
bool sellp_active(zzz_ctx* ctx);
int sellp_resolve(zzz_ctx* ctx);
int sellp_pattern_bounds(zzz_ctx* ctx);
int sellp_capacity_rows(zzz_ctx* ctx); // sp_crow := capacity-based row starts of the compacted copy (+ its allocation)
int64_t sellp_stream_bytes(const zzz_ctx* ctx, bool as_codes = false);
constexpr int SP_DICT_LDS_ENTRIES = 2048; // a value dictionary of at most this many entries is copied into LDS by every workgroup (16 KiB: eight per CU)
int launch_sellp(zzz_ctx* ctx, ProductCall c, int* npartials);
int launch_sellp_overlapped(zzz_ctx* ctx, double* x, ProductCall c, int* npartials);

// kernels_assemble
int launch_assemble_matrix(zzz_ctx* ctx, int form);
int launch_assemble_vector(zzz_ctx* ctx, int form);
int launch_lift(zzz_ctx* ctx); // b -= A_e g over the lifting rows, then b[bc] = g (apply_lifting + bc->set with values)
int launch_matfree_action(zzz_ctx* ctx, const double* x, double* y, double* partials, int* npartials);
int launch_matfree_legacy(zzz_ctx* ctx, const double* x, double* y, double* partials, int* npartials);
int launch_matfree_diagonal(zzz_ctx* ctx, double* d);
// zzz_matfree.hip
int mf_plan_build(zzz_ctx* ctx);
int mf_action(zzz_ctx* ctx, const double* x, double* y, double* partials, int* npartials);
int mf_diagonal(zzz_ctx* ctx, double* y);
int mf_assemble_vector(zzz_ctx* ctx); // b = L on the plan (zzz_matfree_assemble_vector), lifting included
// the same action on the plan's float twins (built on first use; the plan itself as well); x, y: nloc floats on the device
int mf_action_f32(zzz_ctx* ctx, const float* x, float* y, double* partials, int* npartials);
int mf_f32_prepare(zzz_ctx* ctx); // plan + float twins, or ZZZ_ERR_LIMIT with the reason the float action is refused
int mf_f32_info(zzz_ctx* ctx, int64_t info[4]); // zzz_matfree_info_f32
// zzz_cg_f32.hip
int cg_solve_f32(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm);

// kernels_cg
int cg_solve(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm);
int vec_norm_local(zzz_ctx* ctx, const double* v, int64_t n, double* out);

// multigrid preconditioner (zzz_mg.hip)
int mg_check(zzz_ctx* ctx, const zzz_solver_opts* o);   // ZZZ_ERR_ARG with the reason when ZZZ_PC_MG does not apply
int mg_setup(zzz_ctx* ctx, const zzz_solver_opts* o);   // builds / refreshes the hierarchy (synchronises; clobbers the CG vectors)
int mg_vcycle(zzz_ctx* ctx, const double* r, double* z, bool timed); // z = M r enqueued on ctx->stream, skipped once ctx->state says stop
void mg_profile_begin(zzz_ctx* ctx);           // zzz_solver_opts.profile: HIP events around the cycles of a solve ...
void mg_profile_end(zzz_ctx* ctx, int cycles); // ... and their mean over the cycles that ran (zzz_mg_info)
int mg_level0_products(const zzz_ctx* ctx);
double mg_level0_bound(const zzz_ctx* ctx);
void mg_destroy(zzz_ctx* ctx);
void mg_invalidate(zzz_ctx* ctx); // the hierarchy is of a problem that is gone: declined by zzz_mg_*, rebuilt by the next set-up
// zzz_pmg.hip: the transfer between the Pk (order 2, 3) and the P1 dofs of one generated n[0] x n[1] x n[2] cube, enqueued on
// ctx->stream; bcf / bcc are the Dirichlet bytes of the two contexts, sub (may be null) is subtracted from rf on the way in
int pmg_prolong(zzz_ctx* ctx, const int* stop, int order, int bs, const int64_t n[3], const uint8_t* bcf, const uint8_t* bcc,
                const double* ec, double* xf, int accumulate);
int pmg_restrict(zzz_ctx* ctx, const int* stop, int order, int bs, const int64_t n[3], const uint8_t* bcf, const uint8_t* bcc,
                 const double* rf, const double* sub, double* rc);
// zzz_agg.hip (ZZZ_PC_AGG): the aggregates of f's matrix; A_c = P^T A P adopted by the child context c; its values again on
// the kept aggregates; the two transfers enqueued on ctx->stream (bcf: the fine level's Dirichlet bytes)
AggLevel* agg_new();
void agg_free(AggLevel* A);
int64_t agg_count(const AggLevel* A);
int agg_aggregate(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A);
int agg_galerkin(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A, zzz_ctx* c);
int agg_refresh(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A, zzz_ctx* c);
int agg_restrict(zzz_ctx* ctx, const int* stop, const AggLevel* A, const uint8_t* bcf, const double* rf, const double* sub, double* rc);
int agg_prolong(zzz_ctx* ctx, const int* stop, const AggLevel* A, const uint8_t* bcf, const double* ec, double* xf, int accumulate);
const int32_t* agg_map(const AggLevel* A); // device: the aggregate of every fine block dof, -1: none
const int32_t* agg_member_offsets(const AggLevel* A); // device: the map inverted -- the members of aggregate a are
const int32_t* agg_members(const AggLevel* A);        // members[offsets[a] .. offsets[a + 1]), ascending in the caller's numbering
// ... the aggregates of a graph given as it is: n nodes of one CSR row each (values: zero or not), bc: a byte per node
int agg_aggregate_graph(zzz_ctx* ctx, int64_t n, int64_t nnz, const rp_t* rowptr, const int32_t* cols, const double* vals,
                        const uint8_t* bc, AggLevel* A);
// zzz_sagg.hip (ZZZ_PC_SAGG): the same aggregates; P = (I - omega D^-1 A) P_t stored with its transpose, A_c = P^T (A P)
// adopted by the child context c (level: of f, for the messages); the values again on the kept patterns; the two transfers
// enqueued on ctx->stream; P on the host, level 0's rows in the caller's numbering
SaggLevel* sagg_new();
void sagg_free(SaggLevel* S);
int64_t sagg_count(const SaggLevel* S);
int64_t sagg_p_nnz(const SaggLevel* S);
int sagg_aggregate(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S);
int sagg_galerkin(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c, int level);
int sagg_refresh(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c);
int sagg_restrict(zzz_ctx* ctx, const int* stop, const SaggLevel* S, const double* rf, const double* sub, double* rc);
int sagg_prolong(zzz_ctx* ctx, const int* stop, const SaggLevel* S, const double* ec, double* xf, int accumulate);
int sagg_download_p(zzz_ctx* ctx, zzz_ctx* f, const SaggLevel* S, int64_t* rowptr, int32_t* cols, double* vals);
// zzz_sagg_rbm.hip (ZZZ_PC_SAGG_RBM): ZZZ_PC_SAGG's level with the near-nullspace in its tentative prolongator.  The aggregates
// of f's node graph (nodes of 3 scalar dofs on level 0, of 6 below); P, R, T and A_c adopted by c as a scalar matrix (above:
// the level above f, whose B_c the orthogonalisation reads; null on level 0: the context's near-nullspace); the values again.
// Transfers, count, P's size and download are sagg_*'s.  srbm_nns: device, the B the level read (coarse: the B_c it wrote).
int srbm_aggregate(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, int level);
int srbm_galerkin(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, const SaggLevel* above, double omega, zzz_ctx* c, int level);
int srbm_refresh(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c);
int64_t srbm_dropped(const SaggLevel* S); // coarse dofs below S that carry no column of P
const double* srbm_nns(const SaggLevel* S, bool coarse);
// what a level's products keep (zzz_sagg.hip; the rows mode itself: zzz_sagg_rows.hip).  out[0] = 1 when the level was built row by row, out[1] =
// device bytes it keeps for P, R, T and the term lists or the entry permutation, out[2..6] as zzz_mg_products_info's, of this level
void sagg_products_info(const SaggLevel* S, int64_t out[8]);

// comm
int comm_allreduce_sum(zzz_ctx* ctx, double* dev, int n);
bool comm_has_transport(const zzz_ctx* ctx); // comm_allreduce_sum has something to go through: the local group or RCCL (not peer-only)
int comm_allgather_max(zzz_ctx* ctx, double* v); // maximum of one double over the ranks (set-up exchange)
int comm_allgather_double(zzz_ctx* ctx, double v, double* all);
int comm_rank_of(const zzz_ctx* ctx, int* nranks);
// out[0..nv) = all-reduced sums of up to three partial arrays (one kernel with the peer-memory backend,
// reduce kernel + ncclAllReduce otherwise); stop: device flag that makes the call a no-op, or null
int comm_reduce_allreduce(zzz_ctx* ctx, const int* stop, const double* pa, const double* pb, const double* pc, int np, int nv,
                          double* out, hipStream_t st = nullptr);
// overlap form (pipelined CG): the same all-reduce behind everything enqueued on the main stream so far, on a stream of
// its own where the transport allows one; the main stream goes on and meets the result at comm_reduce_end
int comm_reduce_begin(zzz_ctx* ctx, const int* stop, const double* pa, const double* pb, const double* pc, int np, int nv,
                      double* out);
int comm_reduce_end(zzz_ctx* ctx);
bool comm_p2p_enabled(const zzz_ctx* ctx);
int comm_p2p_check(zzz_ctx* ctx);
int comm_inproc_meet(zzz_ctx* ctx); // mailbox ranks inside one process: a host rendezvous before a solve's first round
int comm_halo_forward(zzz_ctx* ctx, double* vec);
int comm_halo_begin(zzz_ctx* ctx, double* vec); // on the comm stream, after the work enqueued so far
int comm_halo_end(zzz_ctx* ctx);                // main stream waits for the halo
int build_tile_split(zzz_ctx* ctx);
void comm_destroy(zzz_ctx* ctx);
} // namespace zzz
