/* fasp_hip_dev.h -- measurement and test entries of libfasp_hip.so.
 *
 * NOT part of the drop-in boundary (include/fasp_hip.h): nothing a FASP application calls is declared here.  These are the
 * entries bench.py, tools/ and tests/ use to time single kernels on a resident hierarchy, to switch kernel families for the
 * bit-identity A/B tests, to inspect the row partition and to run the host-side self-tests.  They live in the shipped library
 * because the driver-run tests and the benchmark load exactly that library.
 */
#ifndef FASP_HIP_DEV_H
#define FASP_HIP_DEV_H
#include "fasp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Timed micro-benchmark of one device kernel class on the resident level-0
 * matrix: returns mean milliseconds per launch over `reps` launches measured
 * with HIP events on the launch stream.  kind: 0 = SpMV, 1 = aAxpy(-1),
 * 2 = Jacobi sweep, 3 = dot, 4 = axpy. */
double fasp_hip_time_kernel(fasp_hip_amg* h, int kind, int level, int reps);
/* development / test entry: one operator through the resident upload path (coding + kernel selection), ms per launch; op: 0 y = A x, 1 y -= A x,
 * 2 Jacobi sweep, else y = A x fused with (y, x); *kind_out (may be NULL) = the family of the plan of the operation that was timed */
double fasp_hip_time_matrix(const dCSRmat* A, int op, int reps, int* kind_out);
/* test entry (host only, no GPU): build the sweep schedule of the rows seq[0..ns) of A (csrc/seq_sched.cpp) and walk it on the host as the
 * device kernels do, against the plain sequential Gauss-Seidel sweep: largest deviation relative to the largest entry; < 0: error
 * (-2: a row reads more earlier rows than a strip holds: no split form).  spine: -1 / 1 where the schedule chooses it, 0 never, 2 wherever
 * a row has two lanes; info (may be NULL): {lanes per row, rounds, spine rounds, virtual rows, strips, chunks} of the schedule */
double fasp_hip_seq_schedule_selftest(const dCSRmat* A, const int* seq, int ns, int strip_kb, int lanes, int spine, int* info);
/* test entry (host only, no GPU): the CHAIN form of the same sweep (csrc/seq_chain.hip.h, round 5: blocked substitution, the dependency
 * chain inside one wavefront) built wherever it applies and walked on the host as k_tri_chain_ref does, with the update formula `form`
 * (0: t * (1 / a_ii) -- fasp_smoother_dcsr_gs; 1: t / a_ii -- the C/F-ordered sweep; 2: SOR with weight w), against the plain sequential
 * sweep; < 0: error (-2: the form does not apply).  n1_blocks: blocks of 64 rows in tier 1 (0: chosen).  info (may be NULL, 10 ints):
 * {blocks, tier-1 blocks, x ring, G ring, tier-1 steps, tier-2 steps, band entries, tier-1 entries, tier-2 entries, dependency classes};
 * out_u (may be NULL, max(row, col) doubles): the swept vector (input: u_i = sin(0.37 i) + 0.1, b_i = cos(0.11 i)) */
/* test entries (host only, no GPU): the brick renumbering of the uncoded mid levels (csrc/reorder.cpp, round 5).  fasp_hip_cluster_order:
 * order[k] = old index of the row that gets the new index k -- breadth-first balls of 64 rows grown inside chunks of `chunk` consecutive rows.
 * fasp_hip_permute_csr: row k of the result is row rperm[k] of A (NULL: rows keep their numbers), column j becomes cinv[j] (NULL: kept); the
 * entries of a row keep their storage order.  ia / ja / val: caller's arrays of row + 1 / nnz / nnz entries. */
int fasp_hip_cluster_order(const dCSRmat* A, int chunk, int* order);
int fasp_hip_permute_csr(const dCSRmat* A, const int* rperm, const int* cinv, int* ia, int* ja, double* val);
double fasp_hip_seq_chain_selftest(const dCSRmat* A, const int* seq, int ns, int n1_blocks, int form, double w, int* info, double* out_u);
/* measured device ceilings reported beside the roofline: out[0..2] = GB/s of a 16-byte-per-lane read, copy and
 * triad over buffers of `bytes` each (>= 512 MiB: beyond the Infinity Cache) */
int fasp_hip_measure_ceilings(double* out, size_t bytes, int reps);

/* ILU triangular solves (csrc/ilu.hip.h).  fasp_hip_ilu_resident_count: factors made by fasp_ilu_dcsr_setup whose device copy
 * is alive (uploaded at the first application, released by fasp_ilu_data_free).  fasp_hip_ilu_time: microseconds per solve
 * of one triangle (which: 1 = L, 2 = U) on the device copy, averaged over `reps` back-to-back solves after one warm-up; info
 * (may be NULL, 6 doubles) = {dependency levels, form (1 single launch, 0 level launches), bytes moved per solve, slab
 * entries (padded), entries, longest row}; < 0: error.  A factor of fasp_ilu_dbsr_setup is timed as the block factor it
 * is (the registry's record), its bytes counted from the block layout.  fasp_hip_ilu_schedule: the schedule of one triangle
 * (which: 1 = L, 2 = U) of any factor in the MSR layout, applied with nb x nb blocks (1..7), from a device copy made and freed by
 * the call -- nothing is launched, nothing becomes resident; info = {dependency levels, chunks of 64 rows, slab entries (padded),
 * entries, longest row, 1 if the depth alone selects the single launch (fasp_hip_tune("ilu_form", ..) is not consulted),
 * workgroups of the level launches summed over the levels, workgroups of the single launch}.  Returns 0, ERROR_INPUT_PAR (NULL
 * arguments, row <= 0, nb outside 1..7, another `which`), ERROR_DATA_STRUCTURE (a column index outside [0, row) among the entries
 * a triangle reads), ERROR_MISC (no device), ERROR_ALLOC_MEM; info is zeroed on every error. */
int    fasp_hip_ilu_resident_count(void);
double fasp_hip_ilu_time(ILU_data* iludata, int which, int reps, double* info);
int    fasp_hip_ilu_schedule(ILU_data* iludata, int nb, int which, double info[8]);
/* ILU smoothing in the block AMG cycle (AMG_param.ILU_levels > 0 with a BSR hierarchy).  The factors belong to the hierarchy:
 * they are not among fasp_hip_ilu_resident_count's.  fasp_hip_bsr_amg_get_ilu: *view = the host factor of `level` (borrowed:
 * valid until the hierarchy is destroyed, not to be freed); returns 1, or 0 when the level has none (at or beyond ILU_levels,
 * the coarsest level, a failed factorisation), < 0 on bad arguments.  fasp_hip_bsr_amg_ilu_info: the schedule of the level's
 * device copy, info = {dependency levels of L, of U, form of the L solve, of the U solve (1 single launch, 0 level launches, as
 * fasp_hip_tune("ilu_form", ..) stands now), chunks of 64 rows of L, of U}; returns 1, or 0 (info zeroed) when the level has no
 * device factor (host-only hierarchies have none).  fasp_hip_bsr_amg_ilu_smooth_time: microseconds per ILU smoothing step of
 * the cycle on `level` (residual, L solve, U solve that also writes x = x + z) over `reps` back-to-back steps after one
 * warm-up; fasp_hip_tune("ilu_smooth_fused", 0) times the form it replaced (the U solve, then a separate axpy); < 0: error. */
int    fasp_hip_bsr_amg_get_ilu(const fasp_hip_amg_bsr* h, int level, ILU_data* view);
int    fasp_hip_bsr_amg_ilu_info(const fasp_hip_amg_bsr* h, int level, double info[6]);
double fasp_hip_bsr_amg_ilu_smooth_time(fasp_hip_amg_bsr* h, int level, int reps);

/* The Galerkin product on the device (csrc/rap.hip.h).  fasp_hip_dcsr_rap: fasp_blas_dcsr_rap with a status instead of an exit --
 * ERROR_INPUT_PAR for NULL arguments or dimensions that do not chain (checked before anything touches a device; *RAP is all zero
 * then), ERROR_ALLOC_MEM for a result of more than 2^31 - 1 entries, ERROR_MISC without a device.  fasp_hip_rap_info: the last
 * product, info = {form used (0 one lane per coarse row, 1 one wavefront per coarse row; a P with a repeated column inside a row
 * takes form 0 whatever was asked for), row batches of the table arena (the larger of the two passes), 1 when rows kept their
 * tables in LDS, rows}.  fasp_hip_rap_device_count: products run on the device since the library was loaded.  fasp_hip_rap_time:
 * seconds per product over `reps` products -- where = 0 the host product of the setups, 1 the device end to end (upload of the
 * operands, kernels, download of the result; after one warm-up), 2 its kernels alone by events; < 0: error. */
int    fasp_hip_dcsr_rap(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, dCSRmat* RAP);
int    fasp_hip_rap_info(int info[4]);
long   fasp_hip_rap_device_count(void);
double fasp_hip_rap_time(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, int where, int reps);

/* Run-time switches (A/B tests, profiling, and ONE behavioural mode):
 *   kernel selection / launch geometry: maxgrid, xcd, nt, kind, lanes, wrows, wcap (-1 = automatic), gen2 (0 round-1
 *     kernels, 1, 2 = default), compress (lossless matrix coding on/off), ja16, ws2_bpc, rpl, lds_tab, xcd_pat, rp_strip (coded operators
 *     of a 3-D grid: an XCD sweeps a strip of every grid plane -- 1: the square operators, 2 (default): the transfer operators too -- or,
 *     0, a slab of planes), estream (k_csr_estream, the entry-parallel kernel of long-row operators: 1 (default) = where it measured
 *     faster -- mean rows of fewer than 256 entries --, 2 = wherever its tables exist, 0 = the row kernels), rgroup (k_csr_rgroup, groups of
 *     consecutive rows of a long-row square operator over the union of their columns: 1 (default) = where it measured faster, and not
 *     under estream 0; 2 = wherever the copy exists; 0 = never, and no copy is built at upload), rgroup_rows (8 (default) or 16 rows per
 *     group; read at upload), rgroup_waves (2, 4 or 8 waves per group; otherwise by the mean row length);
 *   coarse solve: spcg_persist, spcg_fused, spcg_batch, spcg_grid, small_lds, small_onewave (coarsest levels of <= 128
 *     rows: 4 (default) = matrix in registers as 16 x 16 blocks, the direction broadcast inside the multiply-adds, the next
 *     direction sent before the tests of the iteration (k_spcg_dpp<.., true>); 3 = the same without sending ahead; 2 = matrix
 *     in registers, four wavefronts, p broadcast from LDS; 1 = dense in LDS, one wavefront; 0 = the general kernel),
 *     lazy_coarse (the one-launch solvers' verdicts read once per application of the preconditioner, default 1;
 *     2 = replay every first application as if a coarse solve had given up: tests), coarse_mode / coarse_split_min
 *     (multi-GPU: replicated levels computed in row windows + all-gather);
 *   upload: device_sort (per-row sorts of the long-row levels on the device, default 1);
 *   fusions: fuse_zr ((z, r) of PCG from the last level-0 Jacobi sweep), fuse_presmooth (first Jacobi sweep written with
 *     its right-hand side) -- both default 1, results identical (fuse_presmooth: bit for bit; fuse_zr: to rounding);
 *   sequential sweeps (a parallel pass + a sparse triangular solve, csrc/seq_split.hip.h): seq_flow (the triangular solve as a
 *     dataflow over strips of the sweep sequence, default 1; 0 = one launch per dependency class), seq_strip_kb (slot bytes per
 *     strip when a schedule is built, default 512), seq_lanes (lanes per row, 0 = from the row lengths) -- same slots, same
 *     arithmetic, same bits; seq_spine (csrc/seq_sched.h: a row's last two operands in its last lane behind the cross-lane sum; 1 =
 *     on chain-bound eight-round schedules (default), 0 never, 2 wherever a row has two lanes -- part of a schedule's arithmetic: the
 *     modes agree to rounding, not bit for bit), seq_grid (workgroups of the dataflow solve at most; 0 = the schedule's own cap,
 *     < 0 = every resident one), seq_jobs (the schedules built side by side on host threads -- behind the host setup for large
 *     operators, else at the first sweep; default 1);
 *     gs_multicolor = 1 selects the MULTICOLOUR Gauss-Seidel / SOR sweep -- NOT the reference's iteration (rows are
 *     relaxed colour by colour instead of in index order; faster, converges alike, other iteration counts). Default 0:
 *     the reference's sequential sweep, reproduced exactly;
 *   Schwarz sweeps: swz_run (stretches of narrow dependency levels in one launch of one workgroup, k_csr_swz_run: -1 (default) inside
 *     the AMG cycles only, on the Schwarz levels with at most two blocks per dependency level on average; 0 never; 1 on every Schwarz
 *     level of a cycle and in the stand-alone sweeps and fasp_precond_swz), swz_run_width (blocks a level of such a
 *     stretch has at most, default 16) -- same bits;
 *   ILU preconditioner: ilu_form (the triangular solves of fasp_precond_ilu and its kin: -1 (default) one launch for schedules
 *     deeper than 24 levels, else one launch per level; 0 always one launch per level; 1 always one launch) -- same bits;
 *     ilu_smooth_fused (the ILU step of the block AMG cycle: 1 (default) the U solve writes x = x + z itself, 0 a separate
 *     axpy pass) -- same bits;
 *   block sweeps: bsr_sweep_form (the Gauss-Seidel / SOR sweeps of fasp_smoother_dbsr_gs and its kin and of the fasp_hip_bsr_smoother
 *     handle: -1 (default) one launch for plans deeper than 64 levels of at most 8 chunks of 64 block rows on average, else one launch
 *     per level; 0 / 1 force either), bsr_cycle_sweep
 *     (the Gauss-Seidel / SOR sweeps of the block AMG cycle: 0 (default) k_bsr_seq_level per dependency level, 1 the slab plan and
 *     kernels of csrc/bsr_sweep.hip.h) -- same bits;
 *   multi-GPU: halo_overlap (exchange beside the interior rows, default 1), split_rows (test mode: every operator in
 *     three row windows), seq_partition (set before the upload, or FASP_HIP_SEQ_PARTITION=1: hierarchies with Gauss-Seidel / SOR
 *     smoothers are row-partitioned too and the ranks sweep by turns; default 0: such hierarchies keep every level whole),
 *     local_square (a rank's rows of a partitioned level coded with row-relative column offsets like the square operator, default 1;
 *     read at upload);
 *   Galerkin product on the device: rap_form (-1 (default) by the mean work per coarse row, 0 one lane per row, 1 one wavefront
 *     per row), rap_arena_kb (KiB of the table arena the rows are batched into) -- same bytes; device_rap (1: the AMG setups form
 *     their Galerkin products on the device whenever one is usable and there is one rank; 0 (default): on the host) -- same bytes;
 *   safe-net Krylov solvers: safe_fused (1 (default): the fused update kernels of csrc/safe_krylov.hip.h and two iterate buffers whose
 *     roles swap; 0: the reference's pass-by-pass sequence over the existing BLAS-1 launches with a real copy to u_best) -- the same
 *     elementwise bits, sums in another order.
 * Unknown keys return ERROR_INPUT_PAR. */
int fasp_hip_tune(const char* key, int value);
/* test entry: update step `which` of the safe-net Krylov solvers (csrc/safe_krylov.hip.h) on vectors of length n >= 1, once as its fused
 * kernel and once as the reference's sequence over the existing device BLAS-1 kernels, on the same inputs.
 * Inputs: vector k (k = 0 .. 6), entry i = (double)(z >> 11) * 2^-53 * 2 - 1 with z = splitmix64's finaliser of
 * (i + 1) * 0x9E3779B97F4A7C15 + seed * 0xBF58476D1CE4E5B9 + k * 0x94D049BB133111EB (mod 2^64: z ^= z >> 30, z *= 0xBF58476D1CE4E5B9,
 * z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31); seed >= 1000: vector 0, the iterate, holds NaN in entries 0, n / 2 and n - 1.
 * alpha = 0.37, omega = -0.61, beta = 1.29.
 *   which  step (vectors by number)                                                                  scalars
 *   0      safe CG / MinRes update: u(0) += alpha p(1), r(3) -= alpha t(2)                           r.r, u.u, p.p, max|u|, #NaN(u)
 *   1      s(3) = r(1) - alpha z(2)                                                                  --
 *   2      safe BiCGstab update: sp(2) = alpha pp(1) + omega sp, u(0) += sp, s(3) -= omega t(4),
 *          r(6) = s, with rho(5)                                                                     (r,rho), sp.sp, u.u, r.r, max|u|, #NaN(u)
 *   3      p(3) = r(1) + beta (p - omega z(2))                                                       --
 *   4      two dots of t(1) with s(2)                                                                t.t, s.t
 *   5      cycle end of the safe GMRES pair: x(0) += r(1)                                            x.x, max|x|, #NaN(x)
 * out (18 doubles): [0] entries of the step's output vectors whose bit patterns differ between the two forms, [1] number of scalars,
 * [2 ..] the fused form's scalars, [10 ..] the sequence's.  Maxima skip NaN entries (fmax).  The fused forms of 0, 2 and 5 write the
 * iterate out of place.  < 0: error (no device: ERROR_MISC). */
int fasp_hip_safe_update_selftest(int which, int n, int seed, double* out);
/* test entry: ONE launch of one of the small kernels between the matrix products (the BLAS-1 part of csrc/kernels.hip.h, k_pack of
 * csrc/hierarchy.hip.h) on the caller's inputs, with the grid rule and the context buffers of the kernel's production call site, followed
 * by k_finalize where the solvers follow it with one.  The entry holds no reference and generates no input.
 *   vin   6 host pointers, the kernel's vectors by slot (below), n doubles each unless said otherwise; the slots the kernel has must be set
 *   vout  6 host pointers or NULL each: slot k of the device, as the kernel left it, is copied there (same length as vin[k])
 *   scal  8 doubles, ipar 4 ints: the kernel's scalars (below)
 *   part_in, npart   per-block partials a folded variant sums itself (1 <= npart <= 2048, the partial buffer's width per quantity; else
 *         npart = 0); k_finalize: its nq * G inputs, quantity by quantity
 *   red   8 doubles: what k_finalize made of the kernel's partials ([0 .. grid[1]))
 *   part_out  8 * 2048 doubles: the kernel's raw partials, part_out[q * grid[0] + block]
 *   grid  2 ints: [0] the workgroups launched, [1] the number of reduced quantities (0: the kernel reduces nothing)
 *   pub   1 double: the scalar the kernel publishes or divides by, read back from its device slot, which held NaN before the launch
 *         unless an unfolded variant's input was put there (k_cg_update: (t,p); k_axpby_beta: the numerator; k_mgs_step: h)
 *   kernel            variant                                     vectors by slot                 scal              grid, reduction
 *    0 k_cg_update    bit 0: (t,p) summed from part_in, else      p, t, u, r, zx, zdiag           temp1, (t,p),     vec_grid(n); r.r, with bit 2
 *                     scal[1] in slot 8 of d_red; bit 1: temp1                                    zomega,           also u.u, p.p, max|u|, #NaN(u)
 *                     read from slot 12 of d_red (the kernel's                                    zdiag_value       (maxmask 8)
 *                     own temp1 argument is then NaN); bit 2:
 *                     full_norms; bit 3: zx with the zdiag array;
 *                     bit 4: zx with zdiag_value (not both)
 *    1 k_axpby_beta   bit 0: numerator summed from part_in        x, y                            num, den          vec_grid(n / 2 + 1)
 *    2 k_mgs_step     bit 0: h summed from part_in; bit 1: pnext  pj, pi, pnext                   h                 vec_grid(n); (pnext or pi, pi)
 *    3 k_finalize     --  (n = G <= 2048, npart = nq * G)         --                              ipar: nq, maxmask one workgroup; nq quantities
 *    4 k_dot          --                                          x, y                            --                vec_grid(n); x.y
 *    5 k_norms        --                                          x                               --                vec_grid(n); x.x, max|x| (maxmask 2)
 *    6 k_norm1_nan    --                                          x                               --                vec_grid(n); sum|x|, #NaN(x)
 *    7 k_axpy         --                                          x, y                            a                 vec_grid(n / 2 + 1)
 *    8 k_axpby        --                                          x, y                            a, b              vec_grid(n / 2 + 1)
 *    9 k_axpyz        0: z apart; 1: z is x; 2: z is y            x, y, z                         a                 vec_grid(n)
 *   10 k_axpy_self    --                                          y                               a                 vec_grid(n)
 *   11 k_scale        --                                          x                               a                 vec_grid(n)
 *   12 k_set          --                                          x                               v                 vec_grid(n)
 *   13 k_poly_scale   --                                          dinv, r, rbar                   --                vec_grid(n)
 *   14 k_poly_start   --                                          dinv, rbar, v0, v1              k1, k2, k3        vec_grid(n)
 *   15 k_poly_step    --                                          dinv, r, rbar, v0, v1, vnew     k4, k5            vec_grid(n)
 *   16 k_jacobi_zero  --                                          b, d, x                         w                 vec_grid(n)
 *   17 k_l1_zero      --                                          b, d, x                         --                vec_grid(n)
 *   18 k_diag_precond --                                          d, r, z                         --                vec_grid(n)
 *   19 k_bsr_dinv_apply  --  (n scalar rows, a multiple of nb)    dinv (n * nb doubles), b, u     ipar: nb          vec_grid(n)
 *   20 k_pack         --  (n = nsend; idx: n ints in [0, nv))     v (nv doubles), out             ipar: nv          vec_grid(n)
 * Returns FASP_SUCCESS; ERROR_INPUT_PAR for a NULL argument, an unknown kernel or variant, n < 1 or > 2^30, a missing vector, an index outside v, or
 * an npart the partial buffer does not hold (nothing is launched); ERROR_MISC without a device (nothing is written). */
int fasp_hip_blas1_op(int kernel, int variant, int n, const int* ipar, const double* scal, const double* const* vin, double* const* vout,
                      const double* part_in, int npart, const int* idx, double* red, double* part_out, int* grid, double* pub);
/* measurement entry (tools/perf_safe_krylov.py): wall seconds the last Krylov solve of this process with a caller's `precond` (the
 * fasp_solver_d{csr,bsr,str}_p* / _sp* entries and the matrix-free ones) spent in its iteration, from the first residual to the
 * synchronise behind the last one; the upload of the operator, the binding of the preconditioner and the copy of x are outside. */
double fasp_hip_plugin_solve_seconds(void);
/* Which kernel served the last coarsest-level solve of a hierarchy, and how it ended (read-only; tests).  info (8 ints) =
 *   [0] family: 0 none yet, 1 k_spcg_dpp, 2 k_spcg_reg, 3 k_spcg_wave, 4 k_spcg_small, 5 k_spcg_fused, 6 k_spcg_persist,
 *       7 launch_csr<OP_MXV_DOT> + k_spcg_step_reg / k_spcg_step (the last family launched: a persistent kernel that gave
 *       up waiting and handed over to the per-iteration kernels shows as those);
 *   [1] instantiation: k_spcg_dpp NBK (4, 6, 8); k_spcg_reg MC (32, 48, 64); k_spcg_small 2 = matrix and vectors in LDS,
 *       1 = vectors, 0 = nothing; k_spcg_fused 4 / 10 / 16; k_spcg_persist NE (32, 48, 56, 64); step kernels 4 / 10 =
 *       k_spcg_step_reg, 0 = k_spcg_step;
 *   [2] k_spcg_dpp: 1 = send-ahead form; k_spcg_persist: u_lds;
 *   [3] what the safe CG returned (iterations, or its negative verdict); [4] 1 = the SPVGMRES net ran behind it; [5] its return value;
 *   [6] compute units of the device (build_persist_plan deals the rows to ([6] - 1) * 8 wavefronts); [7] 0. */
int fasp_hip_coarse_kernel_info(const fasp_hip_amg* h, int* info);
/* The same for the coarsest level of a block hierarchy.  info (8 ints) = [0] family: 0 none yet, 8 k_gmres_small<SmallBSR, LV>,
 * 9 the general device GMRES (gmres_device); [1] LV (the basis in LDS); [2] cache2 (nb = 3: the blocks of the rows beyond the first
 * 512 in LDS); [3] what the GMRES returned; [4] its iterations; [5] 0; [6] compute units of the device; [7] 0. */
int fasp_hip_bsr_coarse_kernel_info(const fasp_hip_amg_bsr* h, int* info);

/* Counters of the communicator since the last reset: out[0] halo exchanges, [1] all-reduces, [2] all-gathers, [3] doubles sent in
 * exchanges, [4] doubles contributed to all-gathers, [5..7] seconds spent in the three -- filled only in the diagnostic mode
 * fasp_hip_comm_timing(1), which drains the stream around every call (a breakdown of a serialised solve, not a benchmark). */
int fasp_hip_comm_stats(double* out8, int reset);
int fasp_hip_comm_timing(int on);

/* Row partition of a hierarchy over `nranks` GPUs as rank `rank` sees it (host only; levels
 * with fewer than min_rows rows are replicated).  fasp_hip_amg_upload() builds the same
 * plan from the communicator; these entry points expose it to tests.
 * info = {replicated, nglobal, row0, nloc, nghost, nsend, first_replicated_level, nranks};
 * get_matrix: the rank's local rows of A (0) / P (1) / R (2) in local column numbering;
 * get_list:   0 ghost global ids, 1 recv offsets, 2 send offsets, 3 send local ids,
 *             4 ownership offsets of the level. */
int fasp_hip_dist_plan(fasp_hip_amg* h, int rank, int nranks, int min_rows);
int fasp_hip_dist_level_info(const fasp_hip_amg* h, int level, int* info);
int fasp_hip_dist_get_matrix(const fasp_hip_amg* h, int level, int which, dCSRmat* view);
int fasp_hip_dist_get_list(const fasp_hip_amg* h, int level, int which, ivector* view);
/* k_csr_estream's decomposition tables (csrc/kernels3.hip.h) for a matrix with these row pointers, built and walked on the HOST the way the
 * kernel walks them: 0 when every entry is covered once and every row is finished exactly once, else the negative number of the check
 * that failed.  info (may be NULL) = {wave ranges, chunks, rows cut by a wave boundary}.  No GPU needed. */
int  fasp_hip_estream_selftest(const int* ia, int nrow, int nnz, int per_wave, int wmax, int* info);
/* The kernel plan of ONE launch of a row operation (csrc/device_csr.hip.h, plan_csr: the function launch_csr executes and every report below
 * reads) for an operator with the given traits, under the tune keys in force.  No GPU needed: the plan reads sizes and whether pointers are
 * set, never what they point at.  traits (28 ints) = {row, col, nnz, kind, lanes, wrows, wcap, nxrows, plane, npat, npent, sell_nv, sell_nslice,
 * sell_slots, ntcols, es_W, es_nc, then 0 / 1 for: code, pat, rowbase, dpos, dup_diag, ja16, jbase, lja16, sell_code, es_tab, es_ja16} (the fields
 * of DevCSR).  op: the RowOp codes 0 .. 7 of fasp_hip_level_op; windowed: a row-window launch (fasp_hip_tune("split_rows") in force counts as
 * one); want_partials: the launch passes a partials array.  plan (11 ints) = {kernel -- 0 .. 5 k_csr_rows<L> L = 2, 4, 8, 16, 32, 64; 6 .. 9
 * k_csr_wstream<wrows, wcap> (64, 512), (64, 1024), (32, 512), (32, 1024); 10 .. 15 k_csr_rowpat<T, RPL> (0, 1), (0, 2), (1, 1), (1, 2), (2, 1),
 * (2, 2); 16 .. 18 k_csr_dict8<U> U = 8, 16, 24; 19 .. 22 k_csr_estream<L> L = 4, 8, 16, 32; 23 k_csr_rowpat4, 24 k_csr_rowpat5, 25 k_csr_lstream,
 * 26 k_csr_xtile, 27 k_csr_sell, 28 k_csr_wstream2 --, family (the codes of fasp_hip_amg_kernel_info; k_csr_estream counts under 0), rows of a
 * tile, blocks per CU at most (0: what is resident), xcd_map (-2: XCD strips), tiles per grid plane of the strips (0: none), nt bits, ja16
 * passed, jbase passed, the launch writes the fused (x_new, b) partials of a Jacobi sweep, the family fasp_hip_amg_kernel_info reports for the
 * operator (that of op 0 on the whole operator)}; *bytes (may be NULL) = matrix bytes of one pass. */
int  fasp_hip_csr_plan(const int* traits, int op, int windowed, int want_partials, int* plan, double* bytes);
/* The plan of the coarsest level's safe CG (csrc/coarse_cg.hip.h, plan_coarse_spcg: the function coarse_spcg's launchers execute, the cycle and
 * fasp_hip_coarse_kernel_info read) for a level of m rows and nnz stored entries, under the tune keys in force and the FASP_HIP_SMALL_COARSE
 * switch.  No GPU needed.  ia: the level's row pointer (m + 1 ints), read for the deal of k_spcg_persist only; NULL: that form counts as refused.
 * plain_csr: the device operator is usable as plain CSR (no lossless coding took its values and columns); num_cu: compute units of the chip.
 * plan_out (11 ints) = {family, p1, p2 -- the triple fasp_hip_coarse_kernel_info reports once the kernels ran: 1 k_spcg_dpp (NBK, direction sent
 * ahead), 2 k_spcg_reg (MC, 0), 3 k_spcg_wave, 4 k_spcg_small (LDS level: 2 vectors and matrix, 1 vectors, 0 none), 5 k_spcg_fused (E, 0),
 * 6 k_spcg_persist (NE, u in LDS), 7 launch_csr<OP_MXV_DOT> + k_spcg_step_reg (E, 0) / k_spcg_step (0, 0) --, threads per block, blocks, dynamic
 * LDS bytes (family 7: of the step kernel), LD (row stride of the dense image in doubles; families 1 .. 3, else 0), MaxIt = max(250, min(m^2,
 * 1000)), the verdict may be read lazily (once per application of the preconditioner), the start of the solve runs on the device
 * (k_spcg_init), iterations queued between two waits of the host (families 5, 7; else 0)}. */
int  fasp_hip_coarse_plan(int m, int nnz, const int* ia, int plain_csr, int num_cu, int* plan_out);
/* ... and of the block path's coarse GMRES (csrc/bsr.hip.h, plan_coarse_bsr; mgcycle_bsr launches from it) for ROW block rows of nb x nb blocks,
 * NNZ blocks: plan_out (6 ints) = {family -- 8 k_gmres_small<SmallBSR, LV>, 9 gmres_device --, LV (the basis in LDS), cache2 (nb = 3: the rows
 * beyond the first 512 keep their blocks in LDS behind the basis), dynamic LDS bytes, threads per block (0 for family 9, whose kernels have
 * launches of their own), blocks}. */
int  fasp_hip_bsr_coarse_plan(int nb, int ROW, int NNZ, int* plan_out);
/* The value-indexed sliced-ELL coding of k_csr_sell (csrc/kernels4.hip.h) built on the HOST as an upload would build it.  cap_percent: largest
 * slots / entries accepted, in percent (<= 0: the product's 125).  info[8] = {coded (1 / 0), why not (0 coded, 1 size or mean row length outside the
 * range served, 2 a row beyond 255 entries, 3 padding over the cap, 4 too many distinct values, 5 index + offset beyond 32 bits), distinct values,
 * index bits, offset bits, slices, slot rows of 64, largest table accepted}; *bytes = what one pass over the coded form reads.  When coded and the
 * pointers are given: ia_out / ja_out / val_out = the form decoded back to CSR (sized like A's arrays), y = A x over the coded form in the kernel's
 * order (slice by slice, every row left to right).  No GPU needed. */
int  fasp_hip_sell_selftest(const dCSRmat* A, int cap_percent, int* info, double* bytes, int* ia_out, int* ja_out, double* val_out, const double* x, double* y);
/* test entry: one row operation of the kernel family that serves operator `which` (0 A, 1 P, 2 R) of a resident level, vectors given and returned
 * on the host.  op: 0 y = M x, 1 y = b - M x, 2 y += M x, 3 y -= M x, 4 y += scalar M x, 5 Jacobi sweep with weight scalar (A only; x is the
 * iterate), 6 L1-diagonal sweep (A only), 7 y = M x fused with (y, b), 8 y = M x with y2_i = scalar y_i / b_i written along (the fused first Jacobi
 * sweep of the next level).  red (may be NULL): the finished fused sum of ops 7 and 5 -- (y, b), (x_new, b); NaN where the kernel has none. */
int  fasp_hip_level_op(fasp_hip_amg* h, int level, int which, int op, const double* x, const double* b, double* y, double* y2, double scalar, double* red);
/* test entry: one smoothing step of a resident level as a cycle takes it -- smooth() of csrc/smoothers.hip.h with the arguments of AMG_param
 * (smoother, smooth_order, sweeps, relaxation, polynomial_degree) -- before (post 0) or after (post 1) the coarse correction; b (right-hand side)
 * and x (iterate, in and out) are host vectors of the level's row count.  zero_start 1: the step starts from the level's lazily zero iterate and x
 * is not read.  The level's right-hand side pointer and lazy-iterate flags are left as they were; what the step builds on first use (polynomial
 * tables, sweep schedules, the C/F marker) stays.  ERROR_INPUT_PAR, nothing touched: no handle / vector, a level that does not exist, is
 * row-partitioned or a Schwarz level, post or zero_start outside {0, 1}, negative nsweeps or ndeg.  Otherwise smooth()'s status
 * (ERROR_AMG_SMOOTH_TYPE: an unknown smoother, Jacobi-F / GS-F on a level without C/F marker; x is then left alone). */
int  fasp_hip_level_smooth(fasp_hip_amg* h, int level, int post, int smoother, int order, int nsweeps, double relax, int ndeg, int zero_start,
                           const double* b, double* x);
/* ... and of a matrix given on the host, uploaded the way a level's A is.  *kind_out (may be NULL) = the kernel family that serves y = M x on
 * the whole operator -- whatever `op` is: a Jacobi sweep of an operator without diagonal positions, a smoother on a k_csr_rowpat5 operator and a
 * row window may run on another one (fasp_hip_csr_plan tells) --, in the codes of fasp_hip_amg_kernel_info and from the same plan, evaluated under
 * the tune keys in force at the call: 4 k_csr_dict8, 5 k_csr_rowpat, 6 k_csr_rowpat4, 9 k_csr_rowpat5, 7 k_csr_lstream, 8 k_csr_wstream2,
 * 10 k_csr_xtile, 11 k_csr_sell, 0 k_csr_rows (and k_csr_estream), 2 k_csr_wstream.  A rectangular matrix (row != col) is accepted and uploaded the way a transfer operator is: it has no diagonal tables, so
 * ops 5 and 6 return ERROR_INPUT_PAR; x then holds col values, b / y / y2 row values. */
int  fasp_hip_matrix_op(const dCSRmat* A, int op, const double* x, const double* b, double* y, double* y2, double scalar, double* red, int* kind_out);
/* test entry: the 28 traits of fasp_hip_csr_plan's layout read from the device copy fasp_hip_matrix_op makes of A (the same upload; the diagonal
 * tables for a square matrix), which is freed again: with them fasp_hip_csr_plan names the kernel of every operation on that copy. */
int  fasp_hip_matrix_traits(const dCSRmat* A, int* traits);
/* fasp_hip_csr_plan with the traits of the row-group copy (csrc/kernels5.hip.h) behind the 28: traits (32 ints) = {the 28 of fasp_hip_csr_plan, then
 * rg_code set (0 / 1), rows per group, groups, 32-bit words of code}.  fasp_hip_csr_plan itself is unchanged: through it the copy counts as
 * absent.  Kernel codes beyond its 0 .. 28: 29 .. 34 k_csr_rgroup<R, NW> (16, 4), (16, 8), (8, 4), (8, 8), (16, 2), (8, 2) -- family 0, like k_csr_estream; *bytes =
 * the coded form's 8 per entry + 4 per word + 16 per group.  fasp_hip_matrix_traits2: those 32 traits of the device copy
 * fasp_hip_matrix_op makes of A under the tune keys in force ("rgroup" 0: no copy is built). */
int  fasp_hip_csr_plan2(const int* traits, int op, int windowed, int want_partials, int* plan, double* bytes);
int  fasp_hip_matrix_traits2(const dCSRmat* A, int* traits);
/* The row-group coding of k_csr_rgroup (csrc/kernels5.hip.h) built on the HOST as an upload would build it.  rows_per_group: 8 or 16; waves: 2, 4 or
 * 8 (the waves per group of the walk); min_reuse: smallest entries / union columns accepted (<= 0: the product's 3.0).  info[10] = {coded (1 / 0),
 * why not (0 coded, 1 not square, 2 mean row shorter than 128 entries, 3 a group's columns span more than 65 535, 4 a row holds a column twice,
 * 5 reuse below the bound), rows per group, groups, chunks of 64 union columns, union columns, 32-bit words of code, two halves (31 bits each) of a
 * hash over table, code and values, the mean-row bound}; *bytes = what one pass over the coded form reads.  When coded and the pointers are
 * given: ia_out / ja_out / val_out = the form decoded back to CSR with every row sorted by column (sized like A's arrays), y = A x over the coded
 * form in the kernel's order (per wave its chunks, the 64 lanes by the DPP tree, the waves in order).  No GPU needed. */
int  fasp_hip_rgroup_selftest(const dCSRmat* A, int rows_per_group, int waves, double min_reuse, int* info, double* bytes, int* ia_out, int* ja_out, double* val_out, const double* x, double* y);
/* test entry: ONE sequential block sweep of the host matrix A (square, storage_manner 0, 1 <= nb <= 7, a diagonal block in every row) on the
 * device, through the level schedule and the per-level launches the block AMG cycle smooths with: block Gauss-Seidel (sor = 0; w unused) or
 * block SOR with weight w, rows ascending (descend = 0) or descending, u updated in place.  diaginv: the ROW inverse diagonal blocks
 * (fasp_dbsr_getdiaginv).  *nlevels = dependency levels of the schedule (launches of the sweep).  Bad arguments (a NULL pointer, nb outside
 * 1..7, storage_manner != 0, ROW != COL) return ERROR_INPUT_PAR and touch nothing; no usable device: ERROR_MISC. */
int  fasp_hip_bsr_sweep(const dBSRmat* A, const double* b, double* u, const double* diaginv, int descend, int sor, double w, int* nlevels);
/* test entry: ONE sequential sweep (Gauss-Seidel / SOR family) over the rows seq[0..ns) of the host matrix A (square), in that order, on the
 * device: A is uploaded as a one-level hierarchy, the schedule of `seq` is built by the builders of the cycle's sweeps under the tune keys in
 * force (split form, chain form inside it, whole-row dependency levels where a row reads more earlier rows than a strip holds, colour classes
 * under gs_multicolor) and launched by the launch half of the cycle's sweep.  seq: any subset of the rows without repeats.  form: 0 u_i = t *
 * (1 / a_ii), 1 u_i = t / a_ii, 2 u_i = w (t / a_ii) + (1 - w) u_i, with t = b_i - sum_{j != i} a_ij u_j; rows with |a_ii| <= 1e-20 (the last
 * diagonal stored counts) are left alone.  u is uploaded in full and comes back in full -- the device's whole vector, so that a store outside
 * the sweep shows as a changed row of u.  zero_start = 1: the level's vector is flagged all-zero and the input u is ignored and never uploaded;
 * only the swept rows are written back (a row the sweep leaves alone comes back as the +0.0 it holds there), and the entry itself checks that
 * every row outside the sweep still holds +0.0 on the device: ERROR_MISC (and a line on stderr naming the row) when one does not.
 * info (12 ints, may be NULL), set at the launch sites: {path -- 0 nothing to do, 1 k_split_direct, 2 k_split_rest + k_split_scatter(final), 3
 * k_split_rest + k_tri_flow, 4 k_split_rest + k_tri_level per dependency class + k_split_scatter, 5 k_split_rest + k_tri_chain, 6 k_split_rest
 * + k_tri_chain_ref, 7 k_seq_level per whole-row dependency level, 8 k_seq_level per colour --, lanes per row L of the instantiation of pass
 * (2) (paths 3 .. 8; the chain forms: 64), its rounds (4 or 8; paths 3 and 4), lanes per row LR of k_split_rest / k_split_direct (paths 1 ..
 * 6), spine rounds, virtual rows, strips, chunks (paths 3 and 4), launches of pass (2) (path 1: 0), chain form: blocks of tier 1, steps of
 * tier 1, steps of tier 2}.  A NULL pointer, row != col, form outside 0 .. 2, a seq entry out of range or repeated: ERROR_INPUT_PAR, nothing
 * is touched; no usable device: ERROR_MISC; a poll of the dataflow / chain form that ran out: ERROR_MISC (and the report of seq_err_check). */
int  fasp_hip_csr_sweep(const dCSRmat* A, const int* seq, int ns, int form, double w, int zero_start, const double* b, double* u, int* info);
/* which arithmetic form the products of a structured matrix take (pure host code): 0 S (nc = 1, canonical offsets), 1 B (nc = 3, 5,
 * canonical), 2 N (nc = 2, 4, 6, 7, canonical), 3 G (the reference's generic path: any other nband, a canonical count with other
 * offsets, a grid too small for the reference's row segments); ERROR_INPUT_PAR for a matrix the library refuses. */
int  fasp_hip_str_form(const dSTRmat* A);
/* mean milliseconds per launch of the band SpMV kernel on a resident copy of A (HIP events); -1: no device or a refused matrix */
double fasp_hip_time_str_mxv(const dSTRmat* A, int reps);
/* Structured ILU on the device (csrc/str_ilu.hip.h); LU: a factor of fasp_ilu_dstr_setup0 (lfil 0) or
 * _setup1 (lfil 1).  fasp_hip_str_ilu_form (pure host code): the form str_ilu_plan chooses for it under the tune keys in force --
 * 0 one launch per level, 1 planes pipelined over workgroups -- or -1 when the factor cannot be bound (not such a factor, or a
 * non-zero coefficient between grid points that are not geometric neighbours; the reason goes to stdout).
 * fasp_hip_str_ilu_apply: z = U^-1 L^-1 r once, host vectors of ngrid*nc; returns the status of the error word afterwards
 * (ERROR_MISC after a poll that ran out), ERROR_INPUT_PAR for a factor that cannot be bound, ERROR_MISC without a device.
 * fasp_hip_time_str_ilu: mean milliseconds per application on a resident copy (HIP events); -1: no device or not bindable.
 * Tune keys: str_ilu_form (-1 default: by str_ilu_plan, 0 / 1 force a form where it applies), str_ilu_wgs (workgroups of the
 * pipelined form at most; 0: default). */
int    fasp_hip_str_ilu_form(const dSTRmat* LU, int lfil);
int    fasp_hip_str_ilu_apply(const dSTRmat* LU, int lfil, const double* r, double* z);
double fasp_hip_time_str_ilu(const dSTRmat* LU, int lfil, int reps);
/* The structured smoothers on a resident copy (csrc/str_sweep.hip.h).  kind: 0 Jacobi, 1 Gauss-Seidel, 2 SOR;
 * (order, mark) as fasp_smoother_dstr_gs1 takes them (Jacobi ignores both); diaginv: the inverted diagonal blocks for nc > 1, NULL: inverted
 * on the host as the public entries without the trailing 1 do.
 * fasp_hip_str_sweep: matrix, plan and vectors uploaded once, nsweeps sweeps, u back.  info (8 ints, may be NULL): {form that ran -- 0 one
 * launch per level x + y + z, 1 planes pipelined over workgroups, 2 the ordered form (level list), 3 Jacobi --, launches of a sweep, levels,
 * workgroups of the largest launch, visits of a sweep, 1 when the matrix is grid-like, 0, 0}.  ERROR_INPUT_PAR, u untouched: a matrix the
 * library refuses (nc outside 1 .. 7, ...), kind outside 0 .. 2, a USERDEFINED sequence that is not a permutation of the grid points;
 * ERROR_MISC: no device, or a poll of the pipelined form that ran out (and the report of seq_err_check; later calls take the level form).
 * fasp_hip_str_sweep_form (pure host code): the form str_sweep_plan chooses under the tune keys in force, and on stdout why it is not a
 * geometric one; -1 when nothing would be swept (mark NULL, order neither ASCEND nor DESCEND), ERROR_INPUT_PAR as above.
 * fasp_hip_str_sweep_levels (pure host code): the visits of the sweep in the reference's order and the level the ordered form gives each
 * (visit, level: `cap` ints each, either may be NULL); returns the number of visits.
 * fasp_hip_time_str_sweep: mean milliseconds per sweep over `reps` sweeps after one warm-up sweep (HIP events); -1: no device or refused.
 * Tune keys: str_sweep_form (-1 default: by str_sweep_plan; 0 / 1 / 2 force a form where it applies), str_sweep_wgs (workgroups of the
 * pipelined form at most; 0: default). */
int    fasp_hip_str_sweep(const dSTRmat* A, int kind, int order, const int* mark, double weight, const double* diaginv, const double* b,
                          double* u, int nsweeps, int* info);
int    fasp_hip_str_sweep_form(const dSTRmat* A, int order, const int* mark);
int    fasp_hip_str_sweep_levels(const dSTRmat* A, int order, const int* mark, int* visit, int* level, int cap);
double fasp_hip_time_str_sweep(const dSTRmat* A, int kind, int order, const int* mark, double weight, int reps);
/* The block Gauss-Seidel (Schwarz) smoother on a resident copy (csrc/str_swz.hip.h).  neigh: ngrid * nneigh ints (< 0:
 * absent; NULL or nneigh 0: none), order: ngrid ints or NULL (natural).
 * fasp_hip_str_swz: matrix, neigh and visit list uploaded once, every patch factored on the device, nsweeps sweeps, u back.  info (8 ints, may
 * be NULL): {levels, launches of a sweep, visits, visits of the widest level, the largest m, patches with a row interchange, patches whose
 * factorisation stopped, 0}.  ERROR_INPUT_PAR, u untouched: what the public entries refuse (fasp_hip.h), a stopped patch included (info is
 * filled all the same); ERROR_ALLOC_MEM: the factor store does not fit; ERROR_MISC: no device.
 * fasp_hip_str_swz_levels (pure host code): the visits in the reference's order and the level of each (`cap` ints each, either may be NULL);
 * returns the number of visits.
 * fasp_hip_time_str_swz: milliseconds (HIP events) of one factorisation (*ms_factor, mean over `reps` after one warm-up) and per sweep
 * (*ms_sweep, likewise) on a resident copy, info as above; negative: refused or no device. */
int  fasp_hip_str_swz(const dSTRmat* A, const int* neigh, int nneigh, const int* order, const double* b, double* u, int nsweeps, int* info);
int  fasp_hip_str_swz_levels(const dSTRmat* A, const int* neigh, int nneigh, const int* order, int* visit, int* level, int cap);
int  fasp_hip_time_str_swz(const dSTRmat* A, const int* neigh, int nneigh, const int* order, int reps, double* ms_factor, double* ms_sweep, int* info);
/* The CSR overlapping Schwarz sweeps on a resident copy (csrc/csr_swz.hip.h).  swz: an SWZ_data that
 * fasp_swz_dcsr_setup has filled.
 * fasp_hip_csr_swz_levels (pure host code): level[v] (`cap` ints) = the dependency level of block v in the forward (backward 0) or the
 * reversed (backward != 0) sequence; returns the number of levels, ERROR_INPUT_PAR for data the sweeps refuse.
 * fasp_hip_csr_swz: the copy of swz is made resident (uploaded and factored at its first use), then nsweeps times dir (1 forward, 2 backward,
 * 3 forward then backward) from the caller's x with right-hand side b; x back.  info (8 ints, may be NULL): {levels forward, levels backward,
 * launches of this call, nblk, maxbs, blocks with a row interchange, blocks whose factorisation stopped, factorisations this resident copy has
 * run (1 however often it is used)}.  fac / piv (may be NULL): the factors as stored, block v column by column (entry (r, c) at c m + r) at
 * the sum of m^2 over the blocks before it, and the pivots at iblock[v].  ERROR_INPUT_PAR, x untouched: refused data, a stopped block
 * included (info, fac and piv are filled all the same); ERROR_ALLOC_MEM: the store does not fit; ERROR_MISC: no device.
 * fasp_hip_csr_swz_resident_count: SWZ_data with a device copy now.
 * fasp_hip_time_csr_swz: HIP-event milliseconds, mean over `reps` after one warm-up, ms[0] of the factorisation, ms[1] of a forward and ms[2]
 * of a backward sweep; bytes[0] = the bytes of the factor store, bytes[1] = what a forward sweep moves at least; info as above. */
int  fasp_hip_csr_swz_levels(const SWZ_data* swz, int backward, int* level, int cap);
int  fasp_hip_csr_swz(SWZ_data* swz, int dir, const double* b, double* x, int nsweeps, int* info, double* fac, int* piv);
int  fasp_hip_csr_swz_resident_count(void);
int  fasp_hip_time_csr_swz(SWZ_data* swz, int reps, double* ms, double* bytes, int* info);
/* The run form of the sweeps (k_csr_swz_run) and the Schwarz levels of a scalar AMG hierarchy (SWZ_levels > 0).
 * fasp_hip_csr_swz_runs (pure host code): the dependency levels of a direction cut into the launches of the run form at `width` -- a
 * maximal stretch of consecutive levels of at most `width` blocks each is one launch, every wider level one of its own; run_first (`cap`
 * ints, may be NULL) receives the first level of every launch and, last, the number of levels; returns the number of launches.
 * fasp_hip_amg_get_swz: 1 and a view of the blocks level `level` is smoothed with (owned by the hierarchy: do not free), 0 when the level
 * is no Schwarz level.  fasp_hip_amg_swz_levels: *swz_levels = mgl[level].SWZ_levels as the reference's setup leaves it (the caller's value on
 * level 0, AMG_param.SWZ_levels - level below; PreAMGSetupRS.c:110 / :327); host only.  fasp_hip_amg_swz_info (an uploaded hierarchy): 1 and info (8 ints) = dependency levels forward, backward, launches
 * of a forward and of a backward sweep in the form the cycles take now (fasp_hip_tune("swz_run", ..)), blocks, rows of the largest block,
 * blocks factored with a row interchange, factorisations run; 0 when the level is no Schwarz level.
 * fasp_hip_amg_swz_sweep_time: HIP-event milliseconds of one sweep of that form (dir 0 forward, 1 backward; mean over `reps` after one
 * warm-up) on vectors of its own; < 0: an error. */
int    fasp_hip_csr_swz_runs(const SWZ_data* swz, int backward, int width, int* run_first, int cap);
int    fasp_hip_amg_get_swz(const fasp_hip_amg* h, int level, SWZ_data* view);
int    fasp_hip_amg_swz_levels(const fasp_hip_amg* h, int level, int* swz_levels);
int    fasp_hip_amg_swz_info(const fasp_hip_amg* h, int level, int* info);
double fasp_hip_amg_swz_sweep_time(fasp_hip_amg* h, int level, int dir, int reps);
/* The block sweeps over the slab plan (csrc/bsr_sweep.hip.h, csrc/bsr_sweep_plan.h).
 * fasp_hip_bsr_smoother_info: info (6 doubles) = {dependency levels, chunks of 64 block rows, slab entries, padded slab entries, form of the
 * last apply (-1 none yet, 0 one launch per level, 1 one launch), form an apply would take now under fasp_hip_tune("bsr_sweep_form", ..)};
 * returns 1, or 0 for a handle that sweeps nothing.
 * fasp_hip_bsr_sweep_plan (pure host code): the plan of (A, order, mark).  info (6) = {levels, chunks, slab entries, actual off-diagonal
 * entries, longest row, ROW}; the arrays, each may be NULL (call once with NULLs for the sizes): level[ROW], lvl_chunk[levels + 1] (first
 * chunk of each level), rows[64 chunks] (block row of a slot, -1: padding), len[64 chunks] (off-diagonal entries of the slot's row),
 * cbase[chunks] (first slab entry of a chunk), cols[slab entries] (entry k of slot (c, lane) at cbase[c] + 64 k + lane: the column, bit 31
 * set when the entry reads u_new, -1: padding).  Returns 0, 1 when nothing is swept, ERROR_NUM_BLOCKS / ERROR_INPUT_PAR /
 * ERROR_DATA_STRUCTURE as fasp_hip_bsr_smoother_create.
 * fasp_hip_bsr_sweep_time: microseconds per sweep over `reps` back-to-back sweeps after one warm-up (b_i = u_i = sin(0.37 i) + 0.1, inverse
 * blocks computed on the host; kind as fasp_hip_bsr_smoother_apply).  form: 0 the per-level launches of k_bsr_seq_level the block AMG cycle
 * takes by default (ascending / descending Gauss-Seidel and SOR only), 1 the slab plan with one launch per level, 2 the slab plan in one
 * launch, -1 the slab plan in the form fasp_hip_tune("bsr_sweep_form", ..) selects.  info (8 doubles, may be NULL) = {levels, chunks, slab
 * entries, actual entries, form taken (0, 1, 2 as above), bytes one sweep moves at least, milliseconds of plan creation (schedule or plan +
 * upload), longest row}.  < 0: refused or no device.
 * Tune keys: bsr_sweep_form (-1 default: one launch for plans deeper than 64 levels with at most 8 chunks per level on average, else one
 * per level; 0 / 1 force a form), bsr_cycle_sweep (1: the
 * Gauss-Seidel / SOR sweeps of the block AMG cycle take the slab plan; 0, default: k_bsr_seq_level) -- same bits. */
int    fasp_hip_bsr_smoother_info(const fasp_hip_bsr_smoother* h, double info[6]);
int    fasp_hip_bsr_sweep_plan(const dBSRmat* A, int order, const int* mark, long long info[6], int* level, int* lvl_chunk, int* rows, int* len,
                               long long* cbase, int* cols);
double fasp_hip_bsr_sweep_time(const dBSRmat* A, int order, const int* mark, int kind, double weight, int form, int reps, double* info);
/* one-rank exercise of every RCCL call the transport makes (0 = all results correct) */
int  fasp_hip_comm_selftest(void);

#ifdef __cplusplus
}
#endif
#endif /* FASP_HIP_DEV_H */
