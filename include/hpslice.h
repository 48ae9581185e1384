/* hpslice.h -- C ABI of the MI355X-native quasi-static PIC slice engine (libhpslice.so).
 *
 * Drop-in boundary for the per-zeta-slice hot path of HiPACE++ (reference paths relative to
 * /root/reference/src).  The reference has no FFI layer; each entry point below replaces one of
 * its C++ operator seams and takes the same data the reference operator touches, as plain
 * device pointers + sizes:
 *
 *   hps_slab    <-> amrex::MultiFab m_slices[lev] viewed as Array3 (utils/GPUUtil.H:99-147,
 *                   fields/Fields.H:465): ncomp planes of (nx+2ng) x (ny+2ng) doubles, x fastest.
 *   hps_plasma  <-> PlasmaParticleContainer pure-SoA tile (particles/plasma/
 *                   PlasmaParticleContainer.H:21-50): 11 real arrays + idcpu + ion_lev.
 *   hps_geom    <-> amrex::Geometry of the slice + PhysConst (utils/Constants.H:39-81) +
 *                   particle boundary (particles/pusher/GetAndSetPosition.H:29-99).
 *
 * All pointers are DEVICE pointers (HBM) unless a parameter is named *_host.  Every call is
 * asynchronous on the caller's hipStream_t (passed as void*), returns an int status
 * (HPS_OK = 0) instead of aborting, and never allocates unless documented.
 * INTEGRATION.md shows the AMReX-side adaptor for each call.
 */
#ifndef HPSLICE_H_
#define HPSLICE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hps_stream;            /* hipStream_t */

enum { HPS_OK = 0, HPS_ERR_ARG = 1, HPS_ERR_HIP = 2, HPS_ERR_FFT = 3, HPS_ERR_MG_DIVERGED = 4,
       HPS_ERR_MG_MAXITER = 5, HPS_ERR_COMM = 6, HPS_ERR_UNSUPPORTED = 7 };

/* particle boundary, Hipace.H ParticleBoundary */
enum { HPS_BC_REFLECTING = 0, HPS_BC_PERIODIC = 1, HPS_BC_ABSORBING = 2 };

/* Field slab view. element (i,j,n), i in [-ng, nx+ng): p[(i+ng) + (j+ng)*jstride + n*nstride] */
typedef struct {
    double* p;
    int nx, ny, ng, ncomp;
    long jstride, nstride;
} hps_slab;

/* Plasma sheet, pure SoA.  idcpu follows AMReX's packing: bit 63 set = valid particle
 * (ParticleIDWrapper::is_valid), low 24 bits = cpu = mesh-refinement level (0 here). */
typedef struct {
    double *x, *y, *w, *ux, *uy, *psi, *x_prev, *y_prev, *ux_half, *uy_half, *psi_half;
    uint64_t* idcpu;
    int32_t* ion_lev;
    long n;
} hps_plasma;
#define HPS_ID_VALID (1ULL << 63)

typedef struct {
    double dx, dy, dz;           /* cell sizes of the slice geometry                         */
    double xoff, yoff;           /* GetPosOffset(0|1, geom, slab box) (fields/Fields.H:71-77) */
    double c, ep0, mu0, q_e, m_e;/* PhysConst (1 in normalised units)                        */
    double plo[2], phi[2];       /* particle boundary box (Hipace.cpp:219-222)               */
    int bc;                      /* HPS_BC_*                                                 */
    int normalized;              /* hipace.normalized_units                                  */
} hps_geom;

const char* hps_last_error (void);
const char* hps_version (void);

/* ---- particle operators ------------------------------------------------------------------ */

/* DepositCurrent (particles/deposition/PlasmaDepositCurrent.H:28-32, .cpp:22-257).
 * comp = {jx, jy, jz, rho, chi, rhomjz}, -1 = do not deposit.  QSA-violating particles are
 * invalidated (w = 0, idcpu valid bit cleared) and counted into *n_qsa_violation (device int,
 * may be NULL).  `charge` is the species charge (pass -charge for WhichSlice::RhomJzIons). */
int hps_deposit_current (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[6],
                         double charge, double mass, int depos_order, double max_qsa_weighting,
                         int can_ionize, int* n_qsa_violation, hps_stream stream);

/* ExplicitDeposition (particles/deposition/ExplicitDeposition.H:20-22, .cpp:20-263).
 * cache = {Bz, Ez, ExmBy, EypBx} (read per cell), depos = {Sy, Sx}. */
int hps_explicit_deposit (hps_slab slab, hps_plasma plasma, hps_geom geom, const int cache[4],
                          const int depos[2], double charge, double mass, int depos_order,
                          int derivative_type, int can_ionize, hps_stream stream);

/* AdvancePlasmaParticles, leapfrog pusher (particles/pusher/PlasmaParticleAdvance.H:23-26,
 * .cpp:29-305).  comp = {Psi, Ez, Bx, By, Bz}. */
int hps_advance_plasma (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[5],
                        double charge, double mass, int depos_order, int temp_slice,
                        int n_subcycles, int can_ionize, hps_stream stream);

/* The same three operators with a laser envelope (use_laser = true of the reference's compile-time options):
 * aabs_comp = slab component holding |a|^2 (Comps[This]["aabs"]); -1 = no laser = the calls above. */
int hps_deposit_current_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[6], int aabs_comp,
                               double charge, double mass, int depos_order, double max_qsa_weighting,
                               int can_ionize, int* n_qsa_violation, hps_stream stream);
int hps_explicit_deposit_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int cache[4], int aabs_comp,
                                const int depos[2], double charge, double mass, int depos_order,
                                int derivative_type, int can_ionize, hps_stream stream);
int hps_advance_plasma_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[5], int aabs_comp,
                              double charge, double mass, int depos_order, int temp_slice,
                              int n_subcycles, int can_ionize, hps_stream stream);

/* ---- tile-sorted sheet: LDS-tile variants of the three operators -------------------------- */

/* Reorder hook (PlasmaParticleContainer::ReorderParticles, particles/plasma/
 * PlasmaParticleContainer.cpp:196-208 -> amrex::SortParticlesForDeposition): STABLE sort of the
 * sheet by tile_size x tile_size-cell tiles of the particle's nearest cell (invalid particles
 * last).  src is read, dst (a second SoA of >= src.n entries) receives the permuted sheet; the
 * tiling keeps the per-tile offsets.  tile_size is 16 or 32. */
int hps_tiling_create (int nx, int ny, int tile_size, long max_particles, void** handle);
int hps_reorder_particles (void* tiling, hps_plasma src, hps_plasma dst, hps_geom geom,
                           hps_stream stream);
int hps_tiling_info (void* tiling, int* ntiles, const int** offsets_dev, const unsigned int** perm_dev);
int hps_tiling_destroy (void* tiling);

/* BoxSorter::sortParticlesByBox (particles/sorting/BoxSort.cpp:14-78; index_type = unsigned long long, BoxSort.H:21):
 * beam particles -> longitudinal boxes (slices).  box = (int)((z - plo_z)/dz), out of range -> the extra box
 * num_boxes; counts and offsets have num_boxes + 1 entries (offsets = exclusive scan of counts), perm[new] = old,
 * particles keep their order inside a box (the serial CPU result of the reference).  Allocates scratch and
 * synchronises the stream, like the reference; an initialisation-time operator. */
int hps_beam_sort_by_box (const double* z_dev, long n, double plo_z, double dz, int num_boxes,
                          unsigned long long* counts_dev, unsigned long long* offsets_dev,
                          unsigned long long* perm_dev, hps_stream stream);

/* Same operators, same arithmetic, for a sheet ordered by hps_reorder_particles: one workgroup
 * per tile accumulates / gathers through an LDS image of the tile (+6-cell halo).  Particles
 * that drifted out of the halo since the sort take the global-memory path and are counted into
 * *n_fallback (device int, may be NULL); results do not depend on how stale the ordering is. */
int hps_deposit_current_tiled (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[6],
                               double charge, double mass, int depos_order, double max_qsa_weighting,
                               int can_ionize, int* n_qsa_violation, void* tiling, int* n_fallback,
                               hps_stream stream);
int hps_explicit_deposit_tiled (hps_slab slab, hps_plasma plasma, hps_geom geom, const int cache[4],
                                const int depos[2], double charge, double mass, int depos_order,
                                int derivative_type, int can_ionize, void* tiling, int* n_fallback,
                                hps_stream stream);
int hps_advance_plasma_tiled (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[5],
                              double charge, double mass, int depos_order, int temp_slice,
                              int n_subcycles, int can_ionize, void* tiling, int* n_fallback,
                              hps_stream stream);
/* The same three with a laser envelope, as the untiled *_laser calls: aabs_comp = slab component holding |a|^2, -1 = no laser. */
int hps_deposit_current_tiled_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[6], int aabs_comp,
                                     double charge, double mass, int depos_order, double max_qsa_weighting,
                                     int can_ionize, int* n_qsa_violation, void* tiling, int* n_fallback,
                                     hps_stream stream);
int hps_explicit_deposit_tiled_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int cache[4], int aabs_comp,
                                      const int depos[2], double charge, double mass, int depos_order,
                                      int derivative_type, int can_ionize, void* tiling, int* n_fallback,
                                      hps_stream stream);
int hps_advance_plasma_tiled_laser (hps_slab slab, hps_plasma plasma, hps_geom geom, const int comp[5], int aabs_comp,
                                    double charge, double mass, int depos_order, int temp_slice,
                                    int n_subcycles, int can_ionize, void* tiling, int* n_fallback,
                                    hps_stream stream);
/* The caller's promise about the sheet ordered through `tiling`: by_weight = every particle whose valid bit is clear has
 * w == 0, by_psi_half = it has psi_half == 0.  The tiled calls then take "w != 0" (depositions) / "psi_half != 0" (push)
 * for the valid bit, as the engine does for its own sheet, and do not read idcpu.  Both off after hps_tiling_create.
 * Every path of these calls that clears a valid bit also zeroes w and psi_half, so the promise, once true, stays true. */
int hps_tiling_set_validity (void* tiling, int by_weight, int by_psi_half);

/* Dispatch record of the tiled particle kernels: hps_particles_record(1) empties it and switches it on, (0) switches it off
 * (the default).  hps_particles_recorded writes the names of the instances launched while it was on, one per line, e.g.
 * "k_deposit_tiled<2,16,51,0,1>" (template arguments as integers), into buf (NUL-terminated, at most cap bytes); *len =
 * length of the whole list without the NUL. */
int hps_particles_record (int on);
int hps_particles_recorded (char* buf, long cap, long* len);

/* ---- transverse field solvers ------------------------------------------------------------ */

/* FFTPoissonSolverDirichletFast (fields/fft_poisson_solver/FFTPoissonSolverDirichletFast.H:30-32,
 * .cpp:195-328): Lap(F) = S on an nx x ny box with F = 0 one cell outside.  `staging` is the
 * caller-filled nx*ny source (x fastest, no guards; FFTPoissonSolver.H:26-57 StagingArea());
 * the solution is written into component dst_comp of dst (valid cells only). Creation allocates
 * device scratch and rocFFT plans. */
int hps_poisson_create (int nx, int ny, double dx, double dy, void** handle);
int hps_poisson_solve (void* handle, const double* staging, hps_slab dst, int dst_comp,
                       hps_stream stream);
/* nbatch (<= 4) independent solves in one go: sources stacked in `staging` as nbatch planes of
 * nx*ny, solutions into components dst_comps[b].  The three solves of a slice (Psi, Ez, Bz) share
 * their launches this way. */
int hps_poisson_solve_batch (void* handle, int nbatch, const double* staging, hps_slab dst,
                             const int* dst_comps, hps_stream stream);
/* Which kernels the size dispatch of hps_poisson_create chose: *backend one of HPS_POISSON_*; *x_len the
 * length N = nx + 1 of the own DST kernel along x (0 for the dense product and rocFFT); *tri_rows the rows per
 * thread M of the tridiagonal solve along y, k_tridiag_y<M, ..> (0 for rocFFT).  Null outputs are skipped. */
enum { HPS_POISSON_OWN_SYM = 0, HPS_POISSON_OWN_POW2 = 1, HPS_POISSON_DENSE = 2, HPS_POISSON_ROCFFT = 3 };
int hps_poisson_info (void* handle, int* backend, int* x_len, int* tri_rows);
int hps_poisson_destroy (void* handle);

/* hpmg::MultiGrid, system type 1 (mg_solver/HpMultiGrid.H:48,64-66; .cpp:1169-1190,1307-1427):
 * solves -acoef*sol + Lap(sol) = rhs, homogeneous Dirichlet.  sol (in: initial guess, out:
 * solution) and rhs are 2 ADJACENT components starting at sol_comp / rhs_comp; acoef is 1
 * component.  Blocks the host until converged (the stopping rule needs the residual norm);
 * *iters_host receives the number of V-cycles. */
/* slab.nstride must be below 2^27 doubles (1 GB planes: the kernels address cells by 32-bit byte offsets from uniform
 * component bases) and slab.ng at most 8: hps_mg_solve1 / hps_mg_solve1_fabs refuse anything else. */
int hps_mg_create (int nx, int ny, double dx, double dy, void** handle);
int hps_mg_solve1 (void* handle, hps_slab slab, int sol_comp, int rhs_comp, int acoef_comp,
                   double tol_rel, double tol_abs, int max_iters, int* iters_host,
                   double* resnorm_host, hps_stream stream);
/* the same with the reference's own argument list (HpMultiGrid.H:64-66: FArrayBox& sol, FArrayBox const& rhs,
 * FArrayBox const& acoef): three views that need not share a slab -- sol2 and rhs2 with (at least) two components,
 * acoef1 with one; component 0 of each view is used (point .p at the first component wanted) */
int hps_mg_solve1_fabs (void* handle, hps_slab sol2, hps_slab rhs2, hps_slab acoef1, double tol_rel, double tol_abs,
                        int max_iters, int* iters_host, double* resnorm_host, hps_stream stream);
/* Which kernels the size dispatch of hps_mg_create chose.  Null outputs are skipped.
 *   *cc: 1 cell-centred (even nx, ny), 0 node-centred; *nlev: levels of the hierarchy;
 *   *lowv_begin: first level of the lower V; *lowv_kind: HPS_MG_LOWV_* -- k_lower_v3, k_lower_v<true>, k_lower_v<false>, or
 *     the generic bottom (the reference's CPU branch: no level is small enough for one workgroup's LDS, so levels 1 .. nlev - 2
 *     are smoothed level by level and the coarsest one is swept in global memory); *lowv_lds: its dynamic LDS bytes (0: bottom);
 *   tiles[HPS_MG_MAXLEV]: HPS_MG_TILE_* of level 0's initial pass and of the down-leg smoother of levels 1 .. lowv_begin - 1,
 *     -1 from lowv_begin on;
 *   *nodal_pull1: node-centred level 1 forms its right-hand side from level 0's residual itself;
 *   *pyr_levels: levels the coefficient pyramid kernel derives (k_acf_pyramid / k_nodal_acf_pyramid<n>), *pyr_restricts:
 *     k_restrict launches behind it down to lowv_begin. */
enum { HPS_MG_LOWV_V3 = 0, HPS_MG_LOWV_CC = 1, HPS_MG_LOWV_NODAL = 2, HPS_MG_LOWV_BOTTOM = 3 };
enum { HPS_MG_TILE_SMALL = 0, HPS_MG_TILE_BIG = 1, HPS_MG_TILE_SMALL_PULL = 2, HPS_MG_TILE_MID_PULL = 3 };
enum { HPS_MG_MAXLEV = 31 };
int hps_mg_info (void* handle, int* cc, int* nlev, int* lowv_begin, int* lowv_kind, long* lowv_lds, int* tiles,
                 int* nodal_pull1, int* pyr_levels, int* pyr_restricts);
/* What the schedule switches read by hps_mg_create chose.  *coef_guest: 1 where k_lower_v3's coefficient image is derived by a
 * guest workgroup of the solve's initial level-0 pass (HPS_MG_COEF_GUEST, default 1; k_lower_v3 grids whose initial pass runs on
 * 64 x 32 tiles), 0 where the first lower V of a solve derives it itself. */
int hps_mg_info_schedule (void* handle, int* coef_guest);
/* The up-leg of a V-cycle.  *fused_levels: n where the mid levels 1 .. n (n = 2 or 3) make their up-leg in one launch
 * (k_up_fused: HPS_MG_UP_FUSED, default 1; cell-centred grids with k_lower_v3 and lowv_begin >= 3, n = min(3, lowv_begin - 1)),
 * 0 where every mid level has a launch of its own. */
int hps_mg_info_upleg (void* handle, int* fused_levels);
int hps_mg_destroy (void* handle);

/* hpmg::MultiGrid, system type 2 (mg_solver/HpMultiGrid.H:48,84-87 solve2 with an array Re and a scalar Im coefficient;
 * .cpp:296-334 gs2, :192-208 residual2r/2i, :1239-1262), the envelope solve of MultiLaser::AdvanceSliceMG:
 *     -(ar + i ai)(sol_r + i sol_i) + Lap(sol_r + i sol_i) = rhs_r + i rhs_i,   homogeneous Dirichlet,
 * on a cell-centred nx x ny box (even nx, ny).  sol2 / rhs2: device arrays [2][ny][nx] (Re plane, Im plane) without guard
 * cells, sol2 in: initial guess, out: solution; acoef_real_dev [ny][nx]; acoef_imag_dev: ONE double on the device (the
 * caller's kernels produce it).  Blocks the host until converged; HPS_ERR_MG_MAXITER / HPS_ERR_MG_DIVERGED where hpmg aborts. */
int hps_mg2_create (int nx, int ny, double dx, double dy, void** handle);
int hps_mg2_solve2 (void* handle, double* sol2_dev, const double* rhs2_dev, const double* acoef_real_dev,
                    const double* acoef_imag_dev, double tol_rel, double tol_abs, int max_iters, int* iters_host,
                    double* resnorm_host, hps_stream stream);
/* Which kernels the size dispatch of hps_mg2_create chose.  Null outputs are skipped.  *nlev: levels; *low_top: first level of
 * k2_lower_v (-1: none, the generic bottom); *bottom: HPS_MG2_BOTTOM_*; tiles[HPS_MG_MAXLEV]: HPS_MG2_TILE_* of the smoother
 * of levels 0 .. (low_top or nlev - 1) - 1, -1 below. */
enum { HPS_MG2_BOTTOM_LOWER_V = 0, HPS_MG2_BOTTOM_SINGLE_BLOCK = 1, HPS_MG2_BOTTOM_PER_SWEEP = 2 };
enum { HPS_MG2_TILE_SINGLE_BLOCK = 0, HPS_MG2_TILE_SMALL = 1, HPS_MG2_TILE_BIG = 2 };
int hps_mg2_info (void* handle, int* nlev, int* low_top, int* bottom, int* tiles);
int hps_mg2_destroy (void* handle);

/* ---- slice engine (Hipace::Evolve / SolveOneSlice, explicit solver; Hipace.cpp:393-728) -- */

#define HPS_MAX_ION_LEVELS 56
typedef struct {
    int nx, ny, nz; double lo[3], hi[3];
    int order; int deriv_type;
    int plasma_ppc[2]; double plasma_density; double plasma_radius;
    double plasma_charge, plasma_mass; double max_qsa; int n_subcycles;
    int beam_profile;                     /* -1 none, 0 gaussian, 1 flattop */
    double beam_zmin, beam_zmax, beam_radius, beam_density;
    double beam_umean[3], beam_pos_mean[3], beam_pos_std[3]; int beam_ppc[3]; double beam_charge;
    int bc; double mg_tol_rel, mg_tol_abs; int deposit_rho; int n_steps;
    /* moving driver beam: hipace.dt (0 = the beam is never pushed, every BASELINE deck),
     * beam.n_subcycles (0 -> 10, BeamParticleContainer.H:222), beam mass (0 -> 1) and a linear focusing field
     * beams.external_E(x,y,z,t) = ext_E_slope[0]*x  ext_E_slope[1]*y  0 (ExternalFields.H:29-56) */
    double dt; int beam_n_subcycles; double beam_mass; double ext_E_slope[2];
    /* hipace.bxby_solver: 0 explicit (Hipace.H:244), 1 predictor-corrector (Hipace.cpp:935-1031) with
     * hipace.predcorr_B_error_tolerance (0 -> 4e-2), predcorr_max_iterations (0 -> 30), predcorr_B_mixing_factor
     * (0 -> 0.05) (Hipace.H:210-222).  field_bc: boundary.field, 0 Dirichlet, 1 Open (Fields::SetBoundaryCondition,
     * fields/Fields.cpp:678-735: Psi, Ez, Bz -- and Bx, By of the predictor-corrector loop -- solved with the free-space potential
     * of the sources, expanded to order 18 about x = y = 0, as Dirichlet values; x = y = 0 must lie inside the box). */
    int bxby_solver; double predcorr_tol; int predcorr_max_iter; double predcorr_mix; int field_bc;
    /* a Gaussian laser envelope (laser/Laser.H:32-45; CEP 0, no propagation angle -- several pulses, CEP, angle,
     * pulse-front tilt and envelopes from samples: hps_engine_set_laser_pulses / hps_engine_add_laser_samples) drives the wake:
     * |a|^2 goes into the slab component "aabs" (appended last) and enters the deposition, the explicit source and the
     * pusher.  laser_solver = 1 ("fft", MultiLaser::AdvanceSliceFFT) advances the envelope by hipace.dt every step
     * (laser_use_phase = lasers.use_phase); 2 ("multigrid", MultiLaser::AdvanceSliceMG, hpmg system type 2) likewise;
     * 0 keeps it static.  Explicit solver only; LDS-tile and per-particle kernels. */
    int laser_on; double laser_a0, laser_w0, laser_L0, laser_lambda0, laser_pos[3];
    double laser_zfoc; int laser_solver; int laser_use_phase;
    /* hipace.normalized_units = 0: the constants of utils/Constants.H:15-24 (2018 CODATA), charges in C, masses in kg,
     * densities in m^-3, lengths in m; particle weights are then numbers of particles (scale_fac = dx dy dz / ppc) */
    int si_units;
    /* grid_current.* (utils/GridCurrent.cpp:13-23): a Gaussian current density added to jz_beam (explicit solver) or jz
     * (predictor-corrector) of every slice, GridCurrent::DepositCurrentSlice (:25-71, called at Hipace.cpp:629) */
    int grid_current_on; double grid_current_peak, grid_current_mean[3], grid_current_std[3];
    /* laser_solver = 2: lasers.solver_type = multigrid (MultiLaser::AdvanceSliceMG, laser/MultiLaser.cpp:430-608: hpmg
     * system type 2, MG_average_rhs = 1, at most 200 V-cycles); lasers.MG_tolerance_rel (0 -> 1e-4) / MG_tolerance_abs */
    double laser_mg_tol_rel, laser_mg_tol_abs;
    /* <beam>.do_radiation_reaction (classical Landau-Lifshitz force in the beam push, particles/pusher/
     * BeamParticleAdvance.cpp:244-297; in normalised units it needs hipace.background_density_SI to convert the fields)
     * and <beam>.do_z_push (0 = skip z += dt (vz - c), :316; the ABI reads beam_no_z_push so that 0 keeps the default) */
    int beam_radiation_reaction; double background_density_SI; int beam_no_z_push;
    /* SURVEY 8f-2, ionisation: a second plasma species "ion" that can be field-ionised (ADK), its electrons joining the
     * first species -- <ion>.ionization_product = <plasma> (particles/plasma/PlasmaParticleContainer.cpp:61-90, 261-440;
     * InitIonizationModule, PlasmaParticleContainerInit.cpp:382-464).  plasma_no_neutralize: <plasma>.neutralize_background
     * = false (the ions are particles now).  ion_charge: charge of ONE level (+q_e; the deposits and the push weigh it with
     * the particle's ion_lev), ion_energies: the element's ionisation energies in eV (NIST; the reference tabulates them in
     * utils/IonizationEnergiesTable.H), ion_Z of them.  In normalised units background_density_SI must be set.
     * ion_seed: key of the counter-based random number generator (one draw per ion, slice and step; the reference draws
     * from amrex::Random, whose sequence is not reproducible).  Both Bx/By solvers: under the predictor-corrector loop the
     * decisions are taken once per slice on the loop's final fields, ahead of the committing pushes (Hipace.cpp:693-701). */
    int plasma_no_neutralize;
    int ion_on; int ion_ppc[2]; double ion_density, ion_mass, ion_charge; int ion_init_level, ion_Z;
    double ion_energies[HPS_MAX_ION_LEVELS]; unsigned long long ion_seed;
    /* <beam>.do_spin_tracking (moving beam only): every beam particle carries a spin vector, initial_spin (normalised)
     * for all of them, precessing by the Thomas-BMT equation in the beam push (particles/pusher/BeamParticleAdvance.cpp:
     * 218-238; spin_anom = anomalous magnetic moment as given: the electron's is 0.00115965218128, 0 is pure Thomas precession).  The spin travels with the
     * particle through the slipped-particle hand-off and the ring messages (3 more rows). */
    int beam_spin_tracking; double beam_initial_spin[3]; double beam_spin_anom;
    /* hipace.dt = adaptive (utils/AdaptiveTimeStep.cpp; Hipace.cpp:270-282, 400-490): dt_adaptive = 1 makes a moving-beam deck
     * whatever dt says; each step's time and dt come from the host (hps_engine_set_time), computed by the controller
     * hps_adaptive_* below from the beam moments the engine reduces per slice (hps_engine_beam_moments).
     * hipace.nt_per_betatron (0 -> 20), dt_max (0 -> infinity), adaptive_threshold_uz (0 -> 2), adaptive_phase_tolerance
     * (0 -> 4e-4), adaptive_predict_step = 0 / adaptive_control_phase_advance = 0 (the ABI reads the negations, so that 0 keeps
     * the reference's default "on"), adaptive_phase_substeps (0 -> 2000), plasmas.adaptive_density, hipace.max_time (0 -> none),
     * and the initial estimate's <beam>.u_std[2] (beam_uz_std; 0 for a fixed_ppc beam).  Not with a laser (Hipace.cpp:408). */
    int dt_adaptive; double nt_per_betatron, dt_max, adaptive_threshold_uz, adaptive_phase_tolerance;
    int adaptive_no_predict_step, adaptive_no_phase_control, adaptive_phase_substeps;
    double adaptive_density, max_time, beam_uz_std;
    /* beams.external_E(x,y,z,t) = ... ext_Ez_slope*z (z of the particle; ExternalFields.H:29-56), beside ext_E_slope */
    double ext_Ez_slope;
    /* <beam>.do_salame (salame/Salame.cpp; Hipace.cpp:673-678): during step 0 the weights of every beam slice are scaled so
     * that the jz-weighted mean of Ez on the slice behind it follows the target.  hipace.salame_n_iter (0 -> 5),
     * salame_relative_tolerance (0 -> 1e-4), salame_do_advance (the ABI reads the negation, so that 0 keeps the default "on").
     * The reference's parsed salame_Ez_target(zeta, zeta_initial, Ez_initial) is the linear family Ez_initial +
     * salame_Ez_target_slope (zeta - zeta_initial) here (slope 0: the reference's default).  Explicit solver, static beam
     * (hipace.dt = 0), a grid current as the driver; DESIGN 8e says what is refused.  beam_do_salame is the ONE beam of a
     * static-beam engine; in a moving-beam engine the SALAME beam is an added species (hps_engine_set_beam_species_salame,
     * hps_beam_species.do_salame), for which the salame_* parameters here hold as well. */
    int beam_do_salame; int salame_n_iter; double salame_relative_tolerance; int salame_no_advance;
    double salame_Ez_target_slope;
} hps_deck;

/* The SALAME slice (fields/Fields.cpp:111-114): twelve planes appended behind the engine's own components (and behind
 * "aabs"), only in a deck with beam_do_salame or behind hps_engine_set_beam_species_salame: the first one is component
 * hps_engine_slab().ncomp - HPS_SAL_NCOMP. */
enum { HPS_SAL_EZ_TARGET = 0, HPS_SAL_EZ_NO_SALAME, HPS_SAL_EZ, HPS_SAL_JX, HPS_SAL_JY, HPS_SAL_JZB, HPS_SAL_BX, HPS_SAL_BY,
       HPS_SAL_SY, HPS_SAL_SX, HPS_SAL_SY_BACK, HPS_SAL_SX_BACK, HPS_SAL_NCOMP };

/* slab component indices of the engine (explicit-solver layout of fields/Fields.cpp:70-122) */
enum { HPS_C_N_JXB = 0, HPS_C_N_JYB, HPS_C_CHI, HPS_C_SY, HPS_C_SX, HPS_C_EXMBY, HPS_C_EYPBX,
       HPS_C_EZ, HPS_C_BX, HPS_C_BY, HPS_C_BZ, HPS_C_PSI, HPS_C_JXB, HPS_C_JYB, HPS_C_JZB,
       HPS_C_JX, HPS_C_JY, HPS_C_RHOMJZ, HPS_C_P_JXB, HPS_C_P_JYB, HPS_C_ION_RHOMJZ, HPS_C_RHO,
       HPS_NCOMP_MAX };

/* slab component indices with bxby_solver = 1 (predictor-corrector layout of fields/Fields.cpp:128-164: beams and
 * plasma share jx jy jz; Previous keeps Bx By jx jy; PCIter / PCPrevIter hold the iterated Bx By) */
enum { HPS_PC_N_JX = 0, HPS_PC_N_JY, HPS_PC_EXMBY, HPS_PC_EYPBX, HPS_PC_EZ, HPS_PC_BX, HPS_PC_BY, HPS_PC_BZ,
       HPS_PC_PSI, HPS_PC_JX, HPS_PC_JY, HPS_PC_JZ, HPS_PC_RHOMJZ, HPS_PC_P_BX, HPS_PC_P_BY, HPS_PC_P_JX,
       HPS_PC_P_JY, HPS_PC_ION_RHOMJZ, HPS_PC_IT_BX, HPS_PC_IT_BY, HPS_PC_PIT_BX, HPS_PC_PIT_BY, HPS_PC_RHO,
       HPS_PC_NCOMP_MAX };

int hps_engine_create (const hps_deck* deck, int device, void** handle);
int hps_engine_destroy (void* handle);
int hps_engine_begin_step (void* handle);                 /* Evolve :401-471: reset, plasma, ions */
/* The physical time step the next hps_engine_begin_step starts (Hipace::m_physical_time = step * dt,
 * PlasmaParticleContainerInit.cpp:90): the density profile's time factor and the key of the ionisation draws follow it.
 * Without a call an engine counts its own begin_step calls -- right for one engine running every step; a pipeline stage
 * that runs steps r, r + N, ... (Hipace.cpp:400-401) must say which step it is about to run. */
int hps_engine_set_step (void* handle, int step);
/* The physical time t and the time step dt of the step the next hps_engine_begin_step starts (hipace.dt = adaptive:
 * Hipace::m_physical_time and m_dt of that step, Hipace.cpp:411-435).  That step's density profile takes f_t(c t), its beam
 * push dt / beam_n_subcycles.  The ionisation key still follows hps_engine_set_step.  Without a call the step runs at
 * t = deck dt * step with the deck's dt, as before. */
int hps_engine_set_time (void* handle, double t, double dt);
/* hipace.dt = adaptive: {sum w, sum w uz/c, sum w (uz/c)^2, min uz/c} over the beam particles of the step last solved, each
 * counted on the slice it stays on after its push (GatherMinUzSlice(beams, false) behind shiftSlippedParticles,
 * Hipace.cpp:703-716; absorbed particles skipped).  Reduced per slice in the beam's partition kernel and folded head to tail
 * in a fixed order: equal inputs give bit-identical moments.  Zero with min = +infinity for an empty beam.  Synchronises
 * the engine's stream; HPS_ERR_ARG unless the deck has dt_adaptive. */
int hps_engine_beam_moments (void* handle, double* out4_host);
int hps_engine_solve_slice (void* handle, int islice);    /* SolveOneSlice :556-728               */
/* The slice in two halves, for ONE host thread that keeps several engines (time steps in flight on one device, the
 * stages of a pipeline) busy: begin enqueues everything up to and including the speculated V-cycles of the Bx/By solve
 * and the push gated on them, without waiting for the device; finish waits for that solve's norms (the one host wait of
 * a slice, Hipace.cpp:919-921) and enqueues the rest.  hps_engine_solve_slice(k) = begin(k) + finish(k); between the two
 * halves of one engine only calls on OTHER engines are allowed. */
int hps_engine_solve_slice_begin (void* handle, int islice);
int hps_engine_solve_slice_finish (void* handle, int islice);
/* 1 if hps_engine_solve_slice_finish would not wait for the device (the norms of the slice begun have arrived), else 0: a host
 * that drives several engines finishes whichever is ready first */
int hps_engine_slice_ready (void* handle);
int hps_engine_run_step (void* handle);                   /* begin_step + all slices head->tail   */
int hps_engine_sync (void* handle);                       /* host waits for the engine's stream (and, through it, the laser stream) */
int hps_engine_info (void* handle, int* ncomp, int* nguards, long* nparticles);
/* Deferred ShiftSlices: hps_engine_solve_slice leaves the slab UNSHIFTED (Fields::ShiftSlices, fields/Fields.cpp:588-670, runs
 * in the next slice's InitializeSlices pass); hps_engine_slab and hps_engine_sync enqueue the pending shift before they
 * return, hps_engine_record_event / hps_engine_copy_async / the export calls do NOT.  A host that keeps the hps_slab
 * pointer and reads the Previous / Next planes stream-ordered between two slices without one of those two calls sees
 * them as they were before the shift; HPS_LAZY_SHIFT=0 in the environment restores the shift at the end of every slice.
 * Likewise chi, rhomjz, rho, jz_beam and the Next beam currents of the slice just solved: on the plain explicit-solver slice
 * they may sit in alternate planes the engine keeps behind the slab's own (hps_engine_early_init_slices below) until one of
 * those two calls has put them back; HPS_EARLY_INIT=0 in the environment keeps every slice on the slab's own planes. */
hps_slab hps_engine_slab (void* handle);
/* The engine's sheet: raw device pointers.  CONTRACT for a host that invalidates particles itself: clearing the valid bit of
 * idcpu is not enough -- also store 0 to the particle's w AND psi_half.  The engine's tiled depositions take "w != 0" for
 * the valid bit and do not read idcpu (HPS_VALID_BY_W, default on; the tiled push under HPS_VALID_BY_PSI, default on too, reads psi_half the same
 * way): every path of the engine that invalidates a particle (QSA drop, absorbing boundary) zeroes both.  HPS_VALID_BY_W=0
 * in the environment restores the idcpu read. */
hps_plasma hps_engine_plasma (void* handle);
/* the tiling of the first species as the engine holds it now (NULL with tile_size 0): for hps_tiling_info and for calling
 * the *_tiled operators on the engine's own sheet (diagnostics: scripts/deposit_variants.py); owned by the engine */
int hps_engine_tiling (void* handle, void** tiling);
/* species "ion" (hps_deck.ion_on): its sheet, the electrons it has released since hps_engine_create and the size of the
 * first species now (hps_engine_plasma().n follows it); synchronises the stream */
hps_plasma hps_engine_ions (void* handle);
int hps_engine_ion_stats (void* handle, long* n_ionized_host, long* n_product_host);
hps_stream hps_engine_stream (void* handle);
/* sum |Q| per component over valid cells and all slices of the current step (host array[ncomp]) */
int hps_engine_checksums (void* handle, double* out_host);
int hps_engine_stats (void* handle, long* total_vcycles, long* slices_done);
/* slices so far whose ShiftSlices + the next slice's InitializeSlices rode in the launch of their Bx/By solve's first lower V
 * instead of a launch of their own at the head of the next slice (the plain explicit-solver slice on a grid whose lower V is
 * k_lower_v3; HPS_EARLY_INIT=0 in the environment: never).  hps_engine_slab and hps_engine_sync show the slab as without it. */
int hps_engine_early_init_slices (void* handle, long* n_slices);
/* What two schedule switches, read when the engine was created, chose for this engine.  Null outputs are skipped.
 *   *mg_coef_guest: hps_mg_info_schedule of the Bx/By solver (0 for an engine without one);
 *   *valid_by_psi: the electrons' tiled push takes "psi_half != 0" for the valid bit of idcpu and does not read it
 *     (HPS_VALID_BY_PSI, default 1; 0 for an engine whose sheet is not tile-sorted). */
int hps_engine_schedule (void* handle, int* mg_coef_guest, int* valid_by_psi);
/* particles the depositions have dropped since the engine was created because they violate the quasi-static approximation
 * (plasmas.max_qsa_weighting_factor); waits for the engine's stream */
int hps_engine_qsa_drops (void* handle, long* n);
/* predictor-corrector: iterations so far and the sum over slices of the final relative B-field error
 * (m_predcorr_avg_iterations / m_predcorr_avg_B_error of Hipace.cpp:964,1028 before the division by nz) */
int hps_engine_pc_stats (void* handle, long* iterations, double* error_sum);
/* Slices whose loop left after ONE pass because sum |B| of the guess was 0.  The reference's rule is relative_Bfield_error =
 * norm_B > 0 ? diff/norm_B : 0 (fields/Fields.cpp:1283), and the engine applies it literally.  On the serial CPU path norm_B IS 0
 * ahead of the driver (electron and ion charge cancel term by term); a scatter with atomics leaves 1e-16 residue there.  The
 * engine therefore keeps one device word per sweep, "only the cold plasma's residue has been deposited so far" (cleared by
 * hps_engine_begin_step; set by the beam's deposition when a term is not exactly zero, and from the first slice on with a grid
 * current, a second species or no neutralising background), and while it is clear stores the exact zero the serial path holds
 * into Bx, By at the end of a loop pass -- so norm_B is exactly 0 on the same slices as on the CPU, and a real but tiny norm_B
 * (a moving beam's head) iterates as it does there.  HPS_PC_EXACT_ZERO=0 turns that off; HPS_PC_NOISE_FLOOR=<relative floor>
 * (rounds 4-5: 1e-12 of mu0 c |q n0| nx ny (nx dx); now 0) is kept as a diagnostic.  This counter says how often norm_B was 0. */
int hps_engine_pc_zero_b_slices (void* handle, long* slices);
/* laser: index of the slab component "aabs" (-1 without a laser) and sum |a| over the slices solved in this step
 * (the "laserEnvelope" checksum; needs hps_engine_set_diagnostics; synchronises the stream) */
int hps_engine_laser_info (void* handle, int* aabs_comp, double* envelope_abs_sum_host);
/* the envelope a_n of the step that has begun: [nz][ny][nx] complex (re, im interleaved) to the host; synchronises */
int hps_engine_laser_envelope (void* handle, double* out_host);
/* Ring hand-off of the envelope (MultiBuffer::pack_data / unpack_data, utils/MultiBuffer.cpp:840-852, 913-925): a
 * stage passes {a_{n+1}, a_n} of a slice on (msg_dev = [2][ny][nx] complex = 4 nx ny doubles on the device), the next
 * stage stores them as its {a_n, a_{n-1}}.  Import mode (set before hps_engine_begin_step, with the index of the
 * time step the engine is about to run) keeps begin_step from initialising / rotating the time levels itself. */
int hps_engine_set_laser_import (void* handle, int on, int step);
int hps_engine_export_laser_slice (void* handle, int islice, double* msg_dev);
int hps_engine_import_laser_slice (void* handle, int islice, const double* msg_dev);
/* the same hand-off inside one process (several steps in flight on one device): straight from the engine that ran the
 * previous step, on the receiving engine's stream (make it wait for the sender's slice event first) */
int hps_engine_import_laser_from (void* handle, int islice, void* src_engine);
/* The laser envelope on a grid of its own (MultiLaser::MakeLaserGeometry, laser/MultiLaser.cpp:58-115):
 * lasers.n_cell / patch_lo / patch_hi / interp_order; before the first hps_engine_begin_step.  NULL = the field grid's
 * cells / the field box.  zeta is snapped to whole field cells -- zeta_lo = max(0, round((patch_lo_z - poff_z)/dz)),
 * zeta_hi = min(nz - 1, round((patch_hi_z - poff_z)/dz)) -- so laser slice k sits at the z of field slice k; the envelope
 * arrays are [zeta_hi - zeta_lo + 1][nyl][nxl], |a|^2 reaches the field slab and chi the laser grid through B-spline
 * interpolation of interp_order 0 .. 3 (UpdateLaserAabs, InterpolateChi), chi outside the field box is that of the
 * unperturbed plasma (SetInitialChi).  Field slices outside zeta_lo .. zeta_hi have aabs = 0 and no envelope advance.
 * Refused: an empty zeta range, a box without volume, interp_order outside 0 .. 3 (HPS_ERR_ARG); odd n_cell with the
 * multigrid envelope solver (HPS_ERR_UNSUPPORTED).  Without this call nothing changes. */
int hps_engine_set_laser_grid (void* handle, const int* n_cell /*[2] or NULL*/, const double* patch_lo /*[3] or NULL*/,
                               const double* patch_hi /*[3] or NULL*/, int interp_order);
int hps_engine_laser_grid (void* handle, int* nxl, int* nyl, int* zeta_lo, int* zeta_hi);    /* as the engine holds it */
int hps_engine_laser_chi (void* handle, double* out_host);    /* [nyl][nxl]: chi on the laser grid as the last envelope advance read it */
/* With a laser grid hps_engine_laser_envelope returns [zeta_hi - zeta_lo + 1][nyl][nxl], the hand-off messages are
 * [2][nyl][nxl] complex = 4 nxl nyl doubles, export / import of a slice outside zeta_lo .. zeta_hi do nothing and return
 * HPS_OK, and hps_engine_import_laser_from needs equal laser grids.
 *
 * The two interpolations as operators of their own.  The laser grid: nxl x nyl cells of dxl x dyl, cell 0 at (xoffl, yoffl);
 * geom: the slab's geometry; order = lasers.interp_order.
 * hps_laser_interp_aabs: a_plane [nyl][nxl] complex on the device -> slab component c_aabs, guard cells included; laser cells
 * outside the grid contribute nothing.
 * hps_laser_interp_chi: slab component c_chi -> chi_out [nyl][nxl] for the laser cells on the field box shrunk by `shrink`
 * cells (the engine: its guard width), chi_initial [nyl][nxl] elsewhere. */
int hps_laser_interp_aabs (hps_slab slab, int c_aabs, const double* a_plane, int nxl, int nyl, double dxl, double dyl,
                           double xoffl, double yoffl, hps_geom geom, int order, void* stream);
int hps_laser_interp_chi (hps_slab slab, int c_chi, const double* chi_initial, double* chi_out, int nxl, int nyl, double dxl,
                          double dyl, double xoffl, double yoffl, hps_geom geom, int shrink, int order, void* stream);
/* The initial envelope from several Gaussian pulses and from samples (MultiLaser::InitLaserSlice, laser/MultiLaser.cpp:804-920;
 * Laser.cpp:18-60, 117-341).  Both before the first hps_engine_begin_step, on a deck with laser_on; without either
 * call the deck's own pulse is evaluated by the kernel that has always done so.
 *
 * hps_engine_set_laser_pulses: n >= 1 pulses replace the deck's own (lambda0 stays the deck's, shared by all, as in the
 * reference); n = 0: no Gaussian at all, only the sample envelopes below (refused by the first begin_step if there are none);
 * n > 8: HPS_ERR_ARG.  The envelope of a cell is the sum over the pulses, in order, of InitLaserSlice :876-915: with
 * (x, y, z) the cell's position minus pos, angle = propagation_angle_yz and rot = angle + (pft_yz - pi/2) (pft_yz is the
 * reference's PFT_yz, default pi/2),
 *     yp = cos(rot) y - sin(rot) z,   zp = sin(rot) y + cos(rot) z,
 *     D  = 1 + i (zp - zfoc + pos[2] cos(angle)) 2/(k0 w0^2),
 *     a  = a0/D exp(-zp^2/L0^2) exp(-(x^2 + yp^2)/(w0^2 D)) exp(i yp k0 angle + cep).
 * The last factor is literal: the reference adds CEP to the exponent as a real number, so it scales the pulse by e^cep and
 * does not turn its phase.  That is restated here, not corrected. */
typedef struct { double a0, w0, L0, pos[3], zfoc, cep, propagation_angle_yz, pft_yz; } hps_laser_pulse;
int hps_engine_set_laser_pulses (void* handle, int n, const hps_laser_pulse* pulses);
/* geometry: 0 = on the laser grid itself ([nzl][nyl][nxl]; the reference's parser type, evaluated by the host),
 *           1 = "xyt", 2 = "xyz", 3 = "rt" (Laser.cpp:177-336); data: complex doubles, C order [extent0][extent1][extent2];
 *           offset = gridGlobalOffset + position*gridSpacing per axis, in the file's axis order; unit = unitSI
 * (xyt: axes t, y, x; xyz: z, y, x; rt: extent = {modes, nt, nr}, offset and spacing = {t, r, unused}.)  The call copies the
 * samples; up to 4 sets.  At the first begin_step they are uploaded, added to the envelope after the Gaussians in the order
 * given -- geometry 0 cell by cell, 1 .. 3 through order-1 shape factors in x, y and z or t (t = (z of the last laser slice
 * - z)/c/spacing[0]; samples outside the file's extent count as zero; rt: mode 0 plus cos(m theta), sin(m theta) parts, m <=
 * extent[0]/2, theta = atan2(y, x)) -- and freed.  HPS_ERR_ARG: after the first begin_step, without a laser, a fifth set,
 * extent or spacing not positive, geometry 0 with extents other than the laser grid's, rt with an even extent[0] or with a
 * laser cell that would reach a sample index < 0 in r (the reference asserts there), more than 2^31 - 1 samples in a set.
 * Geometry 0 is checked against the laser grid once more at the top of the first begin_step (hps_engine_set_laser_grid may
 * have come in between); a refusal there leaves the engine as it was.  No host memory for the copy: HPS_ERR_HIP, as a
 * failed device allocation. */
int hps_engine_add_laser_samples (void* handle, int geometry, const double* data_host, const long extent[3],
                                  const double offset[3], const double spacing[3], double unit);
/* In-situ laser reductions (MultiLaser::InSituComputeDiags, laser/MultiLaser.cpp:923-1003; lasers.insitu_period): per slice
 * of the laser's zeta range, of the plane a_n that the |a|^2 interpolation of the slice is about to read, out_host[q*nzl +
 * islice - zeta_lo]: q = 0 max(|a|^2) (raw); 1 .. 5 [|a|^2], [|a|^2*x], [|a|^2*x*x], [|a|^2*y], [|a|^2*y*y] (sums times the
 * laser grid's dx dy dz, x = i dx + xoff, y = j dy + yoff on the laser grid); 6, 7 Re, Im of axis(a) (the sum over the one, two
 * or four middle cells times 1, 1/2 or 1/4).  No floating-point atomics: the values are a function of the plane alone, bit for
 * bit.  Cleared by hps_engine_begin_step; a slice outside the zeta range keeps zeros; reading synchronises the stream.  Off: no
 * launch and no allocation.  Switching it on while it is on changes nothing: the rows collected so far stay. */
int hps_engine_set_insitu_laser (void* handle, int on);
int hps_engine_insitu_laser (void* handle, double* out_host /* [8][nzl], nzl = zeta_hi - zeta_lo + 1; nz without a laser grid */);
/* accumulate the per-slice checksums (costs one reduction pass per slice; off by default) */
int hps_engine_set_diagnostics (void* handle, int on);
/* Field diagnostics (Fields::Copy, fields/Fields.cpp:413-533; geometry of Diagnostic::ResizeFDiagFAB,
 * diagnostics/Diagnostic.cpp:300-390; diag_type xyz over the whole box, level 0): a device-resident 3-D array
 * F[ncomps][nz/cz][ny/cy][nx/cx] (x fastest) that every solved slice adds its share to -- linear interpolation of the
 * zero-extended slab components onto the diagnostic grid in x, y and z, exactly as diagnostic.coarsening = cx cy cz
 * does (1 1 1 = plain copy).  Sizes must be divisible by the coarsening.  The array is cleared by
 * hps_engine_begin_step; hps_engine_field_diagnostic copies it to the host (synchronises the stream).
 * Call set before hps_engine_begin_step; ncomps = 0 switches it off. */
int hps_engine_set_field_diagnostic (void* handle, int ncomps, const int* comps, const int coarsening[3]);
int hps_engine_field_diagnostic (void* handle, double* out_host);
/* The other shapes of the reference's field diagnostic (Diagnostic::ResizeFDiagFAB and TrimIOBox,
 * diagnostics/Diagnostic.cpp:300-410): diagnostic.diag_type -- slice_dir -1 = xyz, 0 = yz, 1 = xz (one cell about the middle
 * of the box in that direction: the mean of the two central rows for an even cell count, the central row for an odd one),
 * 2 = xy (one plane that sums the slices of the z range times dz, Fields.cpp:469-479) -- and diagnostic.patch_lo / patch_hi
 * (NULL: the whole box; the patch is rounded to cells per direction, the slice is cut about the middle of the patch).  The
 * array of hps_engine_field_diagnostic is then F[ncomps][n[2]][n[1]][n[0]] with n, and the real box of the diagnostic
 * grid, from hps_engine_field_diagnostic_geometry. */
int hps_engine_set_field_diagnostic_box (void* handle, int ncomps, const int* comps, const int coarsening[3], int slice_dir,
                                         const double* patch_lo /* [3] or NULL */, const double* patch_hi /* [3] or NULL */);
int hps_engine_field_diagnostic_geometry (void* handle, int* n3, double* lo3, double* hi3);

/* In-situ field reductions (Fields::InSituComputeDiags, fields/Fields.cpp:1288-1347; explicit solver only, as the
 * reference): per solved slice, dx dy dz * sum over the valid cells of {Ex^2, Ey^2, Ez^2, Bx^2, By^2, Bz^2, ExmBy^2,
 * EypBx^2, jz_beam, Ez jz_beam} with Ex = ExmBy + c By, Ey = EypBx - c Bx.  out_host[q*nz + islice], q = 0..9, for the
 * step that is being (or has just been) solved; cleared by hps_engine_begin_step; synchronises the stream. */
int hps_engine_set_insitu_fields (void* handle, int on);
int hps_engine_insitu_fields (void* handle, double* out_host /* [10*nz] */);

/* In-situ plasma moments (PlasmaParticleContainer::InSituComputeDiags, particles/plasma/PlasmaParticleContainer.cpp:
 * 443-530), taken at the start of every slice (Hipace.cpp:590) over the valid particles within `radius` of the axis:
 * out_host[q*nz + islice], q = 0..14 = sum(w), [x], [x^2], [y], [y^2], [ux], [ux^2], [uy], [uy^2], [uz], [uz^2], [ga],
 * [ga^2] (averages: divided by sum(w)), [(ga-1)(1-vz)] (sum), Np (count, as a double), with w = weight * gamma/psi.
 * radius <= 0 switches it off; cleared by hps_engine_begin_step; reading synchronises the stream. */
int hps_engine_set_insitu_plasma (void* handle, double radius);
/* In-situ beam moments (BeamParticleContainer::InSituComputeDiags, particles/beam/BeamParticleContainer.cpp:476-556),
 * taken after the field solves and before the beam push (Hipace.cpp:681) over the slice's own valid particles (those
 * that slipped in from the slice ahead are not counted, :494) within `radius` of the axis: out_host[q*nz + islice],
 * q = 0..22 = sum(w), [x], [x^2], [y], [y^2], [z], [z^2], [ux], [ux^2], [uy], [uy^2], [uz], [uz^2], [x*ux], [y*uy],
 * [z*uz], [x*uy], [y*ux], [ux/uz], [uy/uz], [ga], [ga^2] (averages: divided by sum(w)), Np (count, as a double), with
 * u = proper velocity / c.  radius <= 0 switches it off; cleared by hps_engine_begin_step; reading synchronises. */
/* V-cycles of the multigrid envelope solver so far (laser_solver = 2), 0 otherwise */
int hps_engine_laser_vcycles (void* handle, long* vcycles);
int hps_engine_set_insitu_beam (void* handle, double radius);
int hps_engine_insitu_beam (void* handle, double* out_host /* [23*nz] */);
int hps_engine_insitu_plasma (void* handle, double* out_host /* [15*nz] */);

/* particle tiling of the engine: tile_size 0 = per-particle global-atomic kernels, 16 | 32 = LDS
 * tiles, re-sorted after sort_period slices at the latest (plasmas.reorder_period of the reference; see hps_engine_sorts).
 * Call before hps_engine_begin_step. */
int hps_engine_set_tiling (void* handle, int tile_size, int sort_period);
int hps_engine_fallbacks (void* handle, long* n_fallback_host);
/* Plasma density profile (InitParticles evaluates <plasma>.density(x,y,z) per particle with z = c t,
 * PlasmaParticleContainerInit.cpp:246-313; UpdateDensityFunction / density_table_file, PlasmaParticleContainer.cpp:98-117,
 * 211-217).  The tabulated form of the density: n(x, y, ct) = <species>.density * f_r(sqrt(x^2 + y^2)) * f_t(c t), both
 * piecewise linear (constant beyond the ends of a table; n = 0 entries: factor 1), t = hipace.dt * step.  Plasma channels and
 * density ramps are of this form.  A lattice point whose density is <= 0 carries no particle (min_density = 0).  Applies to
 * every plasma species from the next hps_engine_begin_step on, except a species whose density is a parsed function
 * (hps_engine_set_density_expr below: the general form, per species). */
int hps_engine_set_density_profile (void* handle, int nr, const double* r_host, const double* fr_host, int nt,
                                    const double* ct_host, const double* ft_host);
/* The plasma fine patch and the hollow core (InitParticles, PlasmaParticleContainerInit.cpp:36-313; get_position_unit_cell_fine,
 * ParticleUtil.H:66-104; the keys, PlasmaParticleContainer.cpp:123-169).  These values are not members of hps_deck (its layout
 * is pinned); 0 = off.
 *   hps_engine_set_plasma_init: <plasma>.fine_ppc and <ion>.fine_ppc ([2] each, NULL or {0, 0}: that species keeps its uniform
 *     ppc lattice) and <plasma>.hollow_core_radius, the inner counterpart of plasma_radius, which like it holds for both
 *     species: no particle with x^2 + y^2 < hollow_core_radius^2 (:165, :218, :278).
 *   hps_engine_set_fine_patch: plasmas.fine_patch(x,y) > 0, evaluated by the caller at the cell centres lo + (i + 0.5) dx (the
 *     only place the reference evaluates it, :108-110; the input parser is out of scope), as mask_host[ny][nx], != 0 = fine,
 *     and plasmas.fine_transition_cells = T.  The patch is shared by the species.  The level of a cell is T + 1 inside the
 *     patch and falls by one per cell of Manhattan distance around it (T passes of max(own, neighbour - 1), :117-138), on the
 *     cell box cropped to plasma_radius where that is finite (:70-82): mask cells outside that box are ignored and the
 *     transition does not grow past its edges.  A cell of level 0 owns ppc_x ppc_y slots of the sheet on the ppc lattice
 *     with weight density / (ppc_x ppc_y); a cell of level L > 0 owns fine_x fine_y slots with weight density / (fine_x
 *     fine_y), each placed between its coarse and its fine lattice point at s = L / (T + 1), s <- 1.5 s - 0.5 s^3
 *     (ParticleUtil.H:84-103).  Slot order: i_part outermost, the cells that own it x-fastest (:192-239).  The number of slots
 *     is fixed from this call on (hps_engine_info, the sheet arrays, the tiling capacity follow it); a slot beyond the radius,
 *     inside the hollow core or without density is an invalid one, so the count does not change with the profile's time factor.
 * Both: after hps_engine_create and before the first hps_engine_begin_step, in either order, before or after
 * hps_engine_set_tiling; each call allocates the sheets anew.  HPS_ERR_ARG: fine_ppc not positive or not divisible by ppc,
 * component by component (PlasmaParticleContainer.cpp:158-163); ion fine_ppc without the ion species; hollow_core_radius < 0
 * or >= plasma_radius (:126-128); transition_cells < 0; a call after the first hps_engine_begin_step.  Exactly one of
 * fine_ppc and the patch given (:167-169): HPS_ERR_ARG from the first hps_engine_begin_step.  Every engine mode takes the
 * non-uniform sheet, the fused schedule (hps_engine_set_fusion) included.  Decks without these calls run k_init_plasma as
 * before, bit for bit.  prevent_centered_particle, do_symmetrize and u_mean / u_std: the two setters below.  Not restated:
 * prevent_centered_particle together with the fine patch (HPS_ERR_ARG from whichever call comes second). */
int hps_engine_set_plasma_init (void* handle, const int* plasma_fine_ppc, const int* ion_fine_ppc, double hollow_core_radius);
int hps_engine_set_fine_patch (void* handle, const unsigned char* mask_host, int transition_cells);
/* Warm plasmas (InitParticles, PlasmaParticleContainerInit.cpp:52-64, 173-177, 246-313, 317-370; get_gaussian_random_momentum,
 * ParticleUtil.H:113-124).  Not members of hps_deck either; all zero = off: such a deck launches the kernels it launched before.
 *   hps_engine_set_plasma_momentum: <plasma>.u_mean and u_std ([3] each, in units of c) of species 0 (plasma), 1 (ion) or an
 *     added species (hps_engine_add_plasma_species: its index enters the key of the draws like 0 and 1).  Every
 *     slot starts with u = u_mean + u_std n, n three standard normal deviates: ux = u_x c, uy = u_y c, psi = sqrt(1 + u.u) - u_z,
 *     the half-step copies equal.  The deviates are counter based: with z(draw) = hash(hash(hash(hash(seed, species), step),
 *     slot), draw) (the generator of the collisions) Box-Muller on draws (0, 1) gives n_x, n_y and its cosine branch on draws
 *     (2, 3) n_z; `step` is the engine's step index (hps_engine_set_step), so every step's re-injection draws anew, and the sheet
 *     does not depend on the launch or on the tiling.  A component with u_std = 0 is exactly u_mean.  temperature_in_ev is the
 *     caller's conversion to u_std = sqrt(T q_e / (M c^2)) (PlasmaParticleContainer.cpp:138-145).  The predictor-corrector
 *     iterates from the first slice on, and an ionisable species with momentum takes no neutral-tile skip: its atoms move.
 *   hps_engine_set_plasma_symmetry, one value for every species:
 *     do_symmetrize: the slots [0, n/4) are the sheet as it is without the key, the fine patch included, with a quarter of the
 *     weight; copy m = 1, 2, 3 of slot k is slot k + m n/4 at (x_mid2 - x, y), (x, y_mid2 - y), (x_mid2 - x, y_mid2 - y) with
 *     the signs (-,+), (+,-), (-,-) on (ux, uy); x_mid2 = lo + hi.  The copy of an invalid slot is invalid.  hps_engine_info,
 *     the sheet arrays and the tiling capacity follow the four-fold count.
 *     prevent_centered_particle: in a direction whose cell count and ppc are both odd the lattice moves by half a cell onto the
 *     nodes 1 .. n - 1, x = lo + (i + r - 0.5) dx; the slot count stays ppc nx ny, the slots of index 0 are invalid ones.
 * Both: after hps_engine_create and before the first hps_engine_begin_step, in any order relative to each other and to
 * hps_engine_set_tiling, hps_engine_set_plasma_init and hps_engine_set_fine_patch.  HPS_ERR_ARG: a negative u_std; species 1
 * without the ion species (species 0 without a plasma); prevent_centered_particle together with fine_ppc or the patch; a call
 * after the first hps_engine_begin_step.  Not restated: fields.do_symmetrize; per-species symmetry switches. */
int hps_engine_set_plasma_momentum (void* handle, int species, const double u_mean[3], const double u_std[3], unsigned long long seed);
int hps_engine_set_plasma_symmetry (void* handle, int do_symmetrize, int prevent_centered_particle);
/* Fused schedule: the gather + push of slice k also deposits the pushed particles' currents into slice k-1 (one pass over
 * the sheet instead of two; the slab is shifted / cleared before it).  After hps_engine_solve_slice(k) the components jx,
 * jy, chi, rhomjz [, rho] then already belong to slice k-1; everything else, the per-slice checksums and diagnostics are
 * unchanged.  Applies to the explicit solver with a static beam, no laser and one plasma species; off by default. */
int hps_engine_set_fusion (void* handle, int on);
/* number of particle re-sorts so far (periodic + adaptive: the sheet is re-sorted after sort_period slices at the
   latest, earlier once more than 1/256 of it has left the halo of its tile) */
int hps_engine_sorts (void* handle, long* n_sorts_host);
/* HIP-event phase timers on the engine's stream.  phase_times sums, over the slices solved since
 * profiling was switched on (or since the last call), the milliseconds spent in
 * {deposit_current, poisson x3 (+rhs, grad), explicit_deposit, mg_solve1, advance_plasma, other,
 * particle re-sort, empty interval} into ms_host[8] and stores the slice count; it synchronises the stream.
 * "empty interval" = two event records back to back (no kernel between them; 0 when the schedule has no such pair):
 * what every interval carries on top of its kernels. */
/* on = 1: all phases; on = 2: only the deposition kernel and the empty interval (4 event records per slice instead of 11) */
int hps_engine_set_profiling (void* handle, int on);
/* time every stride-th slice only (default 1): the 11 event records of a profiled slice cost about 3.4 us each
 * (4.5 % of a 1024^2 slice at stride 1, measured); phase_times then sums over the profiled slices */
int hps_engine_set_profiling_stride (void* handle, int stride);
int hps_engine_phase_times (void* handle, double* ms_host, long* nslices_host);

/* Driver-beam storage of the engine: particles are kept in slice-major blocks, block p (p-th slice
 * from the head, p = nz-1-islice) = [7][count_p] doubles (x,y,z,ux,uy,uz,w) starting at
 * 7*offsets[p].  A pipeline driver can point the engine at its own buffer (the receive buffer of
 * the ring hand-off); hps_engine_initial_beam copies the injected (step 0) beam into one. */
int hps_engine_beam_info (void* handle, long* nbeam_host, long* offsets_host /* [nz+1] */);
/* A beam the host has initialised itself -- any of the reference's injection types (fixed_weight, fixed_weight_pdf, from_file:
 * InitBeamFixedWeight3D / InitBeamFixedWeightPDFSlice / InitBeamFromFile, particles/beam/BeamParticleContainerInit.cpp:348-477,
 * 479-695, 697-960, which draw from amrex::Random or read an openPMD file) -- in place of the deck's fixed_ppc one
 * (deck.beam_profile = -1: none).  soa_host = [7][n] doubles x y z ux uy uz w on the host, u = gamma beta c, w as the
 * deposition takes it (the weight AddOneBeamParticle stores: in normalised units the injection's total weight over the
 * particle count and the cell volume); any order.  The particles are binned into the box's slices, slice =
 * int((z - lo_z)/dz) as the reference's BoxSorter does (particles/sorting/BoxSort.cpp:34-43), input order kept inside
 * a slice.  Particles outside the box in z are left out and counted in *n_outside (NULL: they are an error).  Call after
 * hps_engine_create and before the first hps_engine_begin_step; works for hipace.dt = 0 and for a moving beam.  In a pipeline
 * every stage's engine is given the same particles (the block layout of hps_engine_beam_info and the hand-off capacity derive
 * from them; only the head stage injects them, MultiBuffer.cpp:809). */
int hps_engine_set_beam_particles (void* handle, long n, const double* soa_host, long* n_outside);
int hps_engine_set_beam_storage (void* handle, double* storage_dev /* [7*nbeam] or NULL = own */);
int hps_engine_initial_beam (void* handle, double* dst_dev);
/* hipace.dt != 0: the beam lives in one SoA over all particles (head slice first) whose slice boundaries move when
 * particles slip (hipace_amd/csrc/beam.hip).  Copies the boundaries [nz+1] and, if soa_host != NULL, the seven
 * arrays x y z ux uy uz w ([7][nbeam], nbeam = hps_engine_beam_info) to the host; synchronises the stream.  A static beam
 * (hipace.dt = 0) is returned in the same layout, with the offsets of hps_engine_beam_info as boundaries: the weights
 * SALAME has left are read this way. */
int hps_engine_beam_state (void* handle, long* boundaries_host, double* soa_host);
/* Ring hand-off of the moving beam (MultiBuffer::put_data / get_data, utils/MultiBuffer.cpp:444-609).  A message is
 * 1 + 7*cap doubles on the device: [count | x[cap] y[cap] z[cap] ux[cap] uy[cap] uz[cap] w[cap]], cap =
 * hps_engine_beam_capacity (twice the fullest injected slice).  export: what sits on slice `islice` after its push;
 * import (import mode on, set before hps_engine_begin_step; slices in head-first order, slice k-1 before slice k is
 * solved): the regular particles of that slice for the step that has begun.  All asynchronous on the engine's stream. */
int hps_engine_beam_capacity (void* handle, long* cap_host);
/* A beam whose slices may come to hold more than twice what the fullest one held when it was injected (a hot beam that bunches
 * as it slips): the particles a slice's hand-off message has room for, set before the first hps_engine_begin_step -- the same
 * on every engine of a pipeline (the message size is 1 + rows * cap doubles).  A slice that outgrows it is an error at the end
 * of the step, never a silent loss. */
int hps_engine_set_beam_capacity (void* handle, long cap);
/* rows of a hand-off message: 7, or 10 with spin tracking (sx sy sz behind w); a message is 1 + rows*cap doubles */
int hps_engine_beam_message_rows (void* handle, int* rows_host);
/* spin tracking: the three spin arrays [3][nbeam] in the order of hps_engine_beam_state; synchronises the stream */
int hps_engine_beam_spin (void* handle, double* soa_host);
int hps_engine_set_beam_import (void* handle, int on);
int hps_engine_export_beam_slice (void* handle, int islice, double* msg_dev);
int hps_engine_import_beam_slice (void* handle, int islice, const double* msg_dev);
/* The slab kernels skip the beam-current planes outside the beam's transverse support.  After
 * hps_engine_set_beam_storage the support is the whole plane (caller-owned particles may sit anywhere); a driver
 * that knows its blocks are the injected beam handed along the ring (hipace.dt = 0: the beam does not move) calls
 * this to restore the support box of the injected beam. */
int hps_engine_assume_initial_beam_support (void* handle);

/* Several time steps in flight on ONE device (hipace_amd/pipeline.py::run_local_pipeline): every step runs in its own
 * engine on its own stream, coupled only by the per-slice beam hand-off.  record_event marks the engine's stream
 * (pool slot `slot`, created on first use) and returns the event; wait_event makes the engine's stream wait for an
 * event recorded by another engine -- the device-side form of "slice k of the previous step has been pushed".
 * copy_async is a device-to-device copy on the engine's stream (the in-process hand-off, MultiBuffer.cpp:299-308).
 * The event covers everything the engine has been given so far, the envelope solver's slice on the engine's laser
 * stream included.  It is for streams of the engine's device (another engine, the ring's send stream): it is recorded
 * without the system-scope fence HIP puts behind an event by default (HPS_EVENT_FENCE=0 restores it). */
int hps_engine_record_event (void* handle, int slot, void** event_out);
/* The engines of a device take their streams from a pool made with the first engine (HPS_STREAM_POOL, default 3: streams
 * created back to back land on different pipes of the command front end).  When the pool is made every pair of its streams
 * runs a 100-us kernel side by side once; pairs that took turns are counted and a warning goes to stderr.  Returns that
 * count (0 = every pair overlaps), -1 before the first engine of the device or with HPS_STREAM_POOL_CHECK=0. */
int hps_stream_pool_shared_pairs (int device);
int hps_engine_wait_event (void* handle, void* event);
int hps_engine_copy_async (void* handle, void* dst_dev, const void* src_dev, long bytes);

/* ---- boundary.field = Open as an operator (Fields::SetBoundaryCondition, fields/Fields.cpp:678-735) -----------------------
 * What the engine runs ahead of every Poisson solve of an open-wall deck, on planes of the caller's: staging_dev holds
 * nbatch (1..4) contiguous source planes [ny][nx] on the box lo .. hi (x, y), cell centres at i dx + GetPosOffset.  Per
 * plane: the 19 complex multipole moments M_n = sum s z'^n (coordinates scaled by 3/|diagonal|) of the cells within 95 % of
 * the distance from x = y = 0 to the nearest wall, then -dx dy/(4 pi) [M_0 ln|z|^2 - sum_n (2/n) Re(M_n z^-n)] / h^2 added
 * to the outermost rows (h = dy) and columns (h = dx), z one cell outside the box; corners get both.  Bit b of
 * no_monopole_mask drops M_0 of plane b (Ez, Bz).  Every other cell is left as it is.  Deterministic (fixed order of
 * summation).  The moment scratch is allocated and freed per call; synchronises the stream.  HPS_ERR_ARG for a null
 * pointer, nbatch outside 1..4, nx or ny < 2, hi <= lo, or x = y = 0 not strictly inside the box. */
int hps_open_boundary (double* staging_dev, int nbatch, int nx, int ny, const double lo[2], const double hi[2],
                       unsigned no_monopole_mask, void* stream);

/* ---- SALAME (salame/Salame.cpp): the engine's module and its operators ------------------------------------------------
 * Per slice of step 0 on which the module ran: out_host[4*islice + {0, 1, 2, 3}] = the last weight factor W, W_total =
 * W * sum(jz) of that iteration (SalameGetW), the iterations used, and flags (bit 0: converged, bit 1: overloaded), the
 * last two as doubles.  All zeros where it did not run.  Synchronises the stream; HPS_ERR_ARG without beam_do_salame or
 * hps_engine_set_beam_species_salame. */
int hps_engine_salame_stats (void* handle, double* out_host /* [4*nz] */);
/* SALAME for a witness species of a moving-beam engine (hipace.dt != 0 or adaptive).  beam_do_salame is the one
 * beam of a static-beam engine; here the SALAME beam is a species added with hps_beam_species.do_salame = 1 (species 0, the
 * deck's beam, is the driver -- or empty, beam_profile = -1, behind a grid current).  hps_engine_set_beam_species_salame(1)
 * announces that such a species will be added: called once, behind hps_engine_create and ahead of every other setter and of
 * the first hps_engine_begin_step, it allocates what a beam_do_salame deck gets at creation -- the twelve HPS_SAL_* planes
 * behind the engine's own components (hps_engine_info keeps the count without them), the scratch and the statistics of the
 * W reduction, and a plasma sheet whose x_prev, y_prev are arrays of their own -- and applies the defaults of salame_n_iter
 * and salame_relative_tolerance.  It is a setter and no member of hps_deck, as the collisions and the further beam species
 * themselves are.  Refused, each with its reason: a static beam (dt = 0: it has no species), a deck with beam_do_salame, the
 * predictor-corrector, ion_on, a laser (HPS_ERR_UNSUPPORTED each, the reasons are beam_do_salame's); a call after a
 * species was added or a step begun (HPS_ERR_ARG).  on = 0 is accepted on any engine and changes nothing.
 * During step 0 the do_salame species deposit jz only, every other species deposits as always, the deposits onto the SALAME
 * slice take the do_salame species alone (MultiBeam.cpp:42-59); the module runs on every slice that held particles of such a
 * species when the step began (:128-140), behind the Bx/By solve and ahead of the in-situ beam diagnostic and the push. */
int hps_engine_set_beam_species_salame (void* handle, int on);
/* The two operators the module calls on the container of a moving-beam engine (HPS_ERR_ARG on a static-beam engine and
 * before the first hps_engine_begin_step; both enqueue on the engine's stream):
 * hps_engine_deposit_beam_species: the moving beam's deposit of slice islice (the particles that have not slipped in during
 * this step, BeamDepositCurrent.cpp:100) restricted to the species whose bit is set in species_mask, added to the slab
 * components cjx, cjy (both or neither; -1: none) and cjz (-1: none) -- k_beam_deposit_dyn<ORDER, 1, 1>.
 * hps_engine_salame_scale_slice: SalameMultiplyBeamWeight (Salame.cpp:407-435) on slice islice of the container: the
 * particles of the do_salame species that have not slipped in and are not absorbed get w *= W; W = 0 makes them absorbed
 * particles (w = 0 exactly, sub-cycle counter -1: what the push's absorbing boundary writes). */
int hps_engine_deposit_beam_species (void* handle, int islice, unsigned species_mask, int cjx, int cjy, int cjz);
int hps_engine_salame_scale_slice (void* handle, int islice, double W);
/* SalameOnlyAdvancePlasma (Salame.cpp:262-339): every valid particle gathers Bx, By (components bx_comp, by_comp) at
 * (x_prev, y_prev) with the plain shape of depos_order and stores ux = 1.5 dz (q/m) By, uy = -1.5 dz (q/m) Bx, q times
 * ion_lev with can_ionize.  Nothing else of the sheet is touched. */
int hps_salame_only_advance (hps_slab slab, hps_plasma plasma, hps_geom geom, int bx_comp, int by_comp, double charge,
                             double mass, int depos_order, int can_ionize, hps_stream stream);
/* SalameGetJxJyFromBxBy (:228-260), valid cells: jx = 1.5 dz chi By / mu0, jy = -1.5 dz chi Bx / mu0 */
int hps_salame_jxjy_from_bxby (hps_slab slab, hps_geom geom, int bx_comp, int by_comp, int chi_comp, int jx_comp, int jy_comp,
                               hps_stream stream);
/* SalameInitializeSxSyWithBeam (:192-225), valid cells: Sy = -mu0 d_y jz, Sx = mu0 d_x jz (centred differences) */
int hps_salame_sxsy_from_jz (hps_slab slab, hps_geom geom, int jz_comp, int sy_comp, int sx_comp, hps_stream stream);
/* The four sums of SalameGetW (:341-405) over the valid cells, in one pass: out4_host = {sum jz Ez_target, sum jz
 * Ez_no_salame, sum jz Ez, sum jz}.  Deterministic (fixed cell-to-lane map, fixed butterfly, ordered fold of the
 * workgroups' partial sums, no atomics): equal planes give bit-equal sums.  scratch_dev: 4*257 doubles on the device.
 * Synchronises the stream. */
int hps_salame_get_w (hps_slab slab, int ez_target_comp, int ez_no_salame_comp, int ez_comp, int jz_comp, double* scratch_dev,
                      double* out4_host, hps_stream stream);
/* SalameMultiplyBeamWeight (:407-437) on the n weights at w_dev: w *= W; W = 0 stores an exact 0 (such a particle
 * deposits nothing and is left out of the in-situ beam count of a SALAME deck). */
int hps_salame_scale_beam_slice (double* w_dev, long n, double W, hps_stream stream);

/* ---- adaptive time step controller (utils/AdaptiveTimeStep.cpp): host only, no device call ---------------------------
 * One controller per rank (or pipeline stage), created from the deck (dt_adaptive and the fields behind it; beam charge
 * and mass, beam_charge = 0: the beam does not set dt; units; the plasma species' densities and charges).  Its dt starts
 * at 0.  rho_max(z) = max(|adaptive_density q_e|, |plasma_charge n(0,0,z)|, |ion_charge n_ion(0,0,z)|) with n(0,0,z) the
 * species' density on the axis, n0 f_r(0) f_t(z) (MultiPlasma::maxChargeDensity), or the species' parsed density at (0, 0, z)
 * (hps_adaptive_set_density_expr below). */
int hps_adaptive_create (const hps_deck* deck, void** handle);
/* the tables of hps_engine_set_density_profile (pass the engine's); replaces the profile, none = factor 1 */
int hps_adaptive_set_density_profile (void* handle, int nr, const double* r_host, const double* fr_host, int nt,
                                      const double* ct_host, const double* ft_host);
/* The head rank's initialisation (Hipace.cpp:275-279): the moments estimated from the beam's u_mean / u_std (uz/c)
 * -- {1, uz_mean, uz_mean^2 + uz_std^2, uz_mean - 4 uz_std} --, then CalculateFromMinUz (predicted over nstages steps, the
 * number of ranks / pipeline stages) and CalculateFromDensity at t = 0.  *dt: the controller's dt afterwards; every stage of
 * a pipeline initialises its own controller alike (what the broadcast of dt and min uz m/q leaves on every rank). */
int hps_adaptive_initial_dt (void* handle, double uz_mean, double uz_std, int nstages, double* dt_host);
/* At the start of the step that starts at time t (Hipace.cpp:420-435): CalculateFromDensity (the moments are reset, the
 * phase advance over adaptive_phase_substeps cuts dt where the density changes), then hipace.max_time: the step that would
 * pass it is clipped to end on it, the step that starts on it runs with dt = 0.  *dt: the step's dt. */
int hps_adaptive_before_step (void* handle, double t, double* dt_host);
/* the time the step begun by the last hps_adaptive_before_step hands to the next one (MultiBuffer::put_time): t + dt,
 * max_time for a clipped step, +infinity behind the step that starts on max_time (every later step is dropped) */
int hps_adaptive_next_time (void* handle, double* t_next_host);
/* At the end of the step that started at time t (CalculateFromMinUz, Hipace.cpp:482-483): the step's moments
 * (hps_engine_beam_moments) give dt = 2 pi / omega_b / nt_per_betatron of the slowest part of the beam, predicted over
 * nstages steps (this dt is used nstages steps later), clamped by dt_max.  *dt: the dt of this controller's next step.
 * HPS_ERR_ARG if the sum of weights is 0 (no beam) or rho_max <= 0. */
int hps_adaptive_after_step (void* handle, const double* moments4_host, double t, int nstages, double* dt_host);
/* The same two with several beams (AdaptiveTimeStep.cpp:94-110, 177-258): one set of moments per beam, each beam's dt from its
 * own mass / charge (a beam of charge 0 is skipped and keeps the dt that was), *dt = the smallest of them, then dt_max; the
 * smallest |min uz m/q| over the beams feeds the phase-advance control.  charge and mass replace the deck's for these calls
 * (mass 0 reads as 1); n = 1 with the deck's charge and mass gives the numbers of the one-beam calls.  n >= 1. */
int hps_adaptive_initial_dt_beams (void* handle, int n, const double* uz_mean, const double* uz_std, const double* charge,
                                   const double* mass, int nstages, double* dt_host);
int hps_adaptive_after_step_beams (void* handle, int n, const double* moments_host /* [n][4] */, const double* charge,
                                   const double* mass, double t, int nstages, double* dt_host);
int hps_adaptive_destroy (void* handle);

/* ---- ring pipeline over time steps: the transport (utils/MultiBuffer.H:21-34; MultiBuffer.cpp:287-609) --------
 * One process per GPU; rank r runs time steps r, r+N, ... (Hipace.cpp:400-401) and hands every pushed beam slice (and
 * the laser envelope of the slice) to rank r+1.  The reference does that with MPI_Isend / MPI_Irecv between ring
 * neighbours (MultiBuffer::make_progress :287-442, put_data :444-493, get_data :495-609); here it is RCCL
 * ncclSend / ncclRecv over xGMI on device buffers (HPS_RING_EDGE=rccl), or peer copies through a mailbox (the default,
 * described behind hps_ring_destroy below).  Every edge r -> r+1 of the ring is its own 2-rank communicator
 * with its own stream, so sends and receives of a rank progress independently; ordering against the engine is by
 * events only (hps_engine_record_event / hps_engine_wait_event), never by a host synchronisation.
 *
 * Bootstrap (host driver, e.g. hipace_amd/pipeline.py over torch.distributed's store): rank r makes the id of ITS
 * outgoing edge with hps_ring_unique_id and hands it to rank r+1; hps_ring_init(rank, world, device, id of the edge
 * (r-1 -> r), id of the edge (r -> r+1)) is collective over the ring.  world = 1: id_edge_in may be NULL, the ring is
 * a 1-rank communicator and hps_ring_sendrecv_self is the hand-off (MultiBuffer.cpp:299-308, "send to myself").
 * hps_ring_init also sends one small message over each of the rank's edges (edge colour by edge colour, like the
 * communicator creation): RCCL connects two peers inside their first ncclSend / ncclRecv -- a rendezvous of the two
 * hosts -- and that must not be left to the pipeline's first hand-offs, whose order around the ring is a circle.
 * Afterwards hps_ring_send_slice / recv_slice only enqueue.  A rank must not synchronise its whole device
 * (hipDeviceSynchronize) while receives it has posted ahead are waiting for their data; hps_engine_sync,
 * hps_ring_sync_sends and hps_ring_sync wait for one stream each. */
#define HPS_RING_ID_BYTES 128
int hps_ring_unique_id (char* id_out /* [HPS_RING_ID_BYTES] */);
int hps_ring_init (int rank, int world, int device, const char* id_edge_in, const char* id_edge_out, void** ring);
/* put_data: `bytes` at msg_dev go to rank+1.  The send waits (on the device) for after_event (hipEvent_t, may be NULL);
 * *done_event (pool slot `slot` of the ring's send events; a hipEvent_t on both kinds of edge) fires when msg_dev may be
 * overwritten.  RCCL edge: only enqueues.  ipc edge (the default): the HOST blocks in this call (up to HPS_RING_TIMEOUT_S)
 * until the next rank has posted the matching receive and its buffer is free -- a host that drives several stages from one
 * thread asks hps_ring_can_send first and keeps the block in an outbox meanwhile (examples/pipeline_host.cpp). */
int hps_ring_send_slice (void* ring, const void* msg_dev, long bytes, void* after_event, int slot, void** done_event);
/* get_data: post the receive of the next message from rank-1 into msg_dev (messages arrive in the order they were
 * sent).  The receive waits for after_event (may be NULL); *done_event (slot `slot` of the ring's receive handles) stands
 * for "the data has landed": hps_ring_engine_wait(ring, engine, *done_event) before the slice that reads it.  The handle is
 * a hipEvent_t on the RCCL edge only; on the ipc edge (the default) it is an object of the ring, and
 * hps_engine_wait_event refuses it with HPS_ERR_ARG -- hosts written against rounds 2-4 change that one call. */
int hps_ring_recv_slice (void* ring, void* msg_dev, long bytes, void* after_event, int slot, void** done_event);
int hps_ring_sendrecv_self (void* ring, const void* src_dev, void* dst_dev, long bytes, void* after_event, int slot,
                            void** done_event);
/* the ring's receive (which = 0) or send (which = 1) stream waits for an event of another stream */
int hps_ring_stream_wait (void* ring, int which, void* event);
int hps_ring_sync_sends (void* ring);           /* host waits until everything sent so far has left */
int hps_ring_sync (void* ring);                 /* host waits for both streams of the ring (end of a run) */
/* Both waits poll and give up with HPS_ERR_COMM (the rank's message counters in hps_last_error) after HPS_RING_TIMEOUT_S
 * seconds (environment, default 900) -- hps_ring_sync_timeout with the limit as an argument: a ring whose peer is gone, or
 * whose posted-ahead receives share a hardware queue with the sends they wait for, fails loudly instead of hanging.
 * hps_ring_init refuses to start a ring of 2+ ranks unless GPU_MAX_HW_QUEUES >= 8 is set in the environment -- by the
 * host's launcher, BEFORE its first HIP call (the runtime reads it once; the library can only see the string).  HPS_RING_ALLOW_SHARED_QUEUES=1
 * turns the refusal off for a host that has arranged its queues some other way. */
int hps_ring_sync_timeout (void* ring, double seconds);
int hps_ring_stats (void* ring, long* n_sent, long* n_received, long long* bytes_sent, long long* bytes_received);
/* what RCCL reports (ncclCommCount / ncclCommUserRank) for the communicators of the incoming and the outgoing edge: 2 and
 * 2 ranks on a ring of 2+ processes (this rank is 1 on the incoming edge, 0 on the outgoing one), 0 and 1 for the one-rank
 * ring -- the evidence that N processes are on RCCL (bench.py's `rccl_ranks_seen`) */
int hps_ring_info (void* ring, int* world, int* comm_in_ranks, int* comm_out_ranks, int* my_rank_in, int* my_rank_out);
int hps_ring_destroy (void* ring);
/* ---- the second kind of edge: peer copies through a shared-memory mailbox (HPS_RING_EDGE=ipc, the default; =rccl for the
 * RCCL edge above).  For the processes of one node, on different devices or on the SAME device (RCCL refuses two ranks on
 * one device).  hps_ring_unique_id makes the edge's mailbox (POSIX shared memory; the id is its name), hps_ring_init maps
 * the mailboxes of both edges and waits for both neighbours (HPS_RING_CONNECT_TIMEOUT_S, default 300).  A posted receive is
 * a descriptor in the mailbox (allocation -- exported once with hipIpcGetMemHandle --, offset, bytes) plus "buffer free",
 * written by the receive stream behind after_event; a send is hipMemcpyAsync into the receiver's buffer plus "landed",
 * written by the send stream: no kernel waits on the device, no requirement on hardware queues (GPU_MAX_HW_QUEUES).  What
 * MultiBuffer does with MPI_Test polls (MultiBuffer.cpp:287-442) the host does with the three calls below.  Differences a
 * host sees: (1) *done_event of hps_ring_recv_slice is a handle of the RING -- order an engine behind it with
 * hps_ring_engine_wait (works for both kinds of edge), not hps_engine_wait_event; (2) hps_ring_send_slice makes the HOST wait
 * (up to HPS_RING_TIMEOUT_S) until the matching receive is posted and free -- ask hps_ring_can_send first where the host
 * must not block; (3) message sizes are checked: a send whose size differs from the posted receive's fails; (4) receive
 * buffers must stay allocated until hps_ring_destroy (their allocations are mapped into the sending process). */
int hps_ring_edge_kind (void* ring);                              /* 0 = RCCL, 1 = ipc */
int hps_ring_can_send (void* ring);                               /* 1: the next hps_ring_send_slice will not wait on the host */
int hps_ring_recv_landed (void* ring, void* done_event);          /* 1: that receive's message is in the buffer; 0: not yet */
/* order the engine behind that receive.  RCCL edge: the engine's STREAM waits for the receive's event (the call only
 * enqueues).  ipc edge: the HOST blocks here (up to HPS_RING_TIMEOUT_S) until the sender's stream has flagged the message
 * as landed -- the engine's later launches are then ordered behind it by program order; a host with several stages per
 * thread polls hps_ring_recv_landed first and gives its other stages their turn (examples/pipeline_host.cpp). */
int hps_ring_engine_wait (void* ring, void* engine, void* done_event);

/* ---- binary Coulomb collisions between plasma species (hipace.collisions) ------------------------------------------------
 * doPlasmaPlasmaCoulombCollision (particles/collisions/CoulombCollision.cpp:59-236, with ElasticCollisionPerez.H,
 * UpdateMomentumPerez.H, ComputeTemperature.H, ShuffleFisherYates.H): the particles of sheet a and sheet b that share a cell
 * of the nx x ny box (cell = int((x - geom.plo[0])/dx), int((y - geom.plo[1])/dy)) collide pairwise and have ux_half, uy_half,
 * psi_half rewritten; the same sheet twice = collisions within one species.  Invalid particles (valid bit clear or w == 0)
 * and particles outside the box take no part.  coulomb_log <= 0: computed per pair.  In normalised units
 * background_density_SI must be > 0.  can_ionize: the charge is multiplied by ion_lev as the reference does it.
 * Random numbers are counter based: a draw is a function of (seed, collision, step, islice, cell, pair, draw index), and a
 * cell's list is ordered by the id bits of idcpu (bits 24..62, which must be unique within a sheet) before it is shuffled, so
 * the result does not depend on the order of the sheets.  tiling_a / tiling_b: the tilings the sheets are ordered by, or
 * NULL; the cell lists are built from the positions for every sheet, so they do not change the result.
 * Allocates its cell lists and synchronises the stream (the test surface of the kernels; the engine keeps its lists).
 * *pairs_collided_host: pairs with relative momentum (the others are left as they are); *overfull_cells_host: cells whose
 * lists did not fit the LDS stage and were worked on in global memory.  Either may be NULL. */
int hps_collide_plasma (hps_plasma a, void* tiling_a, hps_plasma b, void* tiling_b, hps_geom geom, int nx, int ny,
                        double charge_a, double mass_a, int can_ionize_a, double charge_b, double mass_b, int can_ionize_b,
                        double coulomb_log, double background_density_SI, unsigned long long seed, int collision,
                        int step, int islice, long* pairs_collided_host, long* overfull_cells_host, hps_stream stream);
/* Engine: one more collision between species_a and species_b (0 = the plasma, 1 = the species "ion", 2 ... = the species of
 * hps_engine_add_plasma_species, which must have been added before), run in the order of
 * the calls at the end of every slice, behind the plasma and beam pushes and ahead of ShiftSlices (Hipace.cpp:711-712); the
 * predictor-corrector loop collides once per slice, behind its committing push.  Call after hps_engine_create and before the
 * first hps_engine_begin_step.  coulomb_log <= 0: automatic.  With a collision configured the plasma's particles carry their
 * lattice index in the id bits, and the fused push + deposit schedule (hps_engine_set_fusion) is off: it would deposit the
 * pushed momenta before they collide.  Refused: normalised units without background_density_SI; species 1 without ion_on;
 * a call after the first hps_engine_begin_step (HPS_ERR_ARG each); an ion species that can still ionise (ion_init_level <
 * ion_Z: released electrons carry no unique key; HPS_ERR_UNSUPPORTED).  An engine without a collision launches nothing new. */
#define HPS_MAX_COLLISIONS 8
int hps_engine_add_collision (void* handle, int species_a, int species_b, double coulomb_log, unsigned long long seed);
/* ---- Coulomb collisions between the moving beam and a plasma species -------------------------------------------------------
 * doBeamPlasmaCoulombCollision (CoulombCollision.cpp:238-348; the is_beam_coll branches of ElasticCollisionPerez.H and
 * ComputeTemperature.H): the beam particles of a slice and the sheet's particles that share a cell collide pairwise; the beam
 * has ux, uy, uz rewritten (gamma = sqrt(1 + u^2/c^2), no 0.5 (g1/psi1 + g2/psi2) factor on dt), the sheet ux_half, uy_half,
 * psi_half.  A beam slice is seven device arrays of n entries and, optionally, the sub-cycle counters (NULL: none). */
typedef struct {
    double *x, *y, *z, *ux, *uy, *uz, *w;
    int32_t* nsub;               /* nsub[i] < 0: absorbed at the boundary, in no cell; may be NULL */
    long n;
} hps_beam_slice;
/* The free operator (the test surface of the kernels; allocates its cell lists and synchronises the stream).  A beam particle
 * takes part if nsub >= 0, w != 0 and x, y lie inside the box; the others come back untouched.  The sheet as in
 * hps_collide_plasma.  dt: the time step of the run IN SECONDS (hipace.dt / omega_p in normalised units, hipace.dt in SI
 * units) -- not dz.  Draws: the chain of hps_collide_plasma, shuffle slot 0 the beam, slot 1 the plasma.  A beam particle
 * carries no id: before the shuffle a cell's beam list is ordered lexicographically by the 64-bit patterns of (x, y, z, ux,
 * uy, uz, w), so the result is a function of the set of particles (two that tie on all seven are interchangeable).  The
 * plasma's cell list holds only the cells in which the beam has a particle.  Statistics as for hps_collide_plasma. */
int hps_collide_beam_plasma (hps_beam_slice beam, hps_plasma plasma, hps_geom geom, int nx, int ny, double charge_beam,
                             double mass_beam, double charge_plasma, double mass_plasma, int can_ionize_plasma,
                             double coulomb_log, double background_density_SI, unsigned long long seed, int collision,
                             int step, int islice, double dt, long* pairs_collided_host, long* overfull_cells_host,
                             hps_stream stream);
/* Engine: one more collision, between the beam and plasma species plasma_species (0 = the plasma, 1 = the species "ion").  It
 * joins the ordered list of hps_engine_add_collision (HPS_MAX_COLLISIONS holds for both kinds together; a collision's index
 * in that list is the `collision` of its draws) and runs where that list runs: behind the beam's push and the hand-over of
 * the slipped particles to the next slice (Hipace.cpp:704-712), on the beam particles that stay on the slice -- the ones
 * that slipped collide on the next slice's turn.  dt is the time step of the step that has begun (hipace.dt, over omega_p of
 * background_density_SI in normalised units).  Slices exported behind the slice (hps_engine_export_beam_slice) carry the
 * collided momenta.  A static beam (hipace.dt = 0) is accepted and launches nothing: the reference's s is dt times a factor,
 * 0 for every pair, its scattering angle 0, and the static beam lives in the per-slice blocks, not in the moving beam's
 * arrays; sheet and slab are those of the engine without the collision.  An engine without a beam accepts it and does nothing.
 * Refused: normalised units without background_density_SI; species 1 without ion_on; a call after the first
 * hps_engine_begin_step; more than HPS_MAX_COLLISIONS (HPS_ERR_ARG each); an ion species that can still ionise; hipace.dt =
 * adaptive, whose beam moments the engine reduces ahead of the collisions where the reference gathers them behind
 * (HPS_ERR_UNSUPPORTED each). */
int hps_engine_add_beam_collision (void* handle, int plasma_species, double coulomb_log, unsigned long long seed);
/* pairs collided and overfull cells since hps_engine_create; synchronises the stream */
int hps_engine_collision_stats (void* handle, long* pairs_collided, long* overfull_cells);

/* ---- expression programs (parsed functions of the input file) --------------------------------------
 * The reference's parsed functions (beams.external_E(x,y,z,t), ...) reach the C ABI compiled: a postfix program over
 * n_vars input variables with one double result.  An instruction is {opcode, operand}; HPS_EX_CONST pushes
 * consts[operand], HPS_EX_VAR pushes variable operand, HPS_EX_POWI raises the top to the literal integer power operand
 * (|operand| <= 8) by repeated multiplication (r = x; r = r*x ...; 1/r for a negative power; 1 for power 0); every other
 * opcode ignores its operand, pops its arguments and pushes its result.  Comparisons, and / or / not give 1.0 / 0.0 (and,
 * or, not and select test "!= 0"); HPS_EX_SELECT pops b, a, c and pushes c != 0 ? a : b (both arms have been evaluated);
 * HPS_EX_MIN / HPS_EX_MAX are (a < b ? a : b) / (a > b ? a : b); HPS_EX_HEAVISIDE(x1, x2) is 0 for x1 < 0, x2 for
 * x1 == 0 and 1 for x1 > 0.  Every arithmetic operation rounds once (no fused multiply-add), on the host and on the device.
 * hipace_amd/expr.py compiles the input syntax to such programs; there is no text parser in the C ABI. */
enum { HPS_EX_CONST = 0, HPS_EX_VAR, HPS_EX_ADD, HPS_EX_SUB, HPS_EX_MUL, HPS_EX_DIV, HPS_EX_NEG, HPS_EX_POW, HPS_EX_POWI,
       HPS_EX_LT, HPS_EX_LE, HPS_EX_GT, HPS_EX_GE, HPS_EX_EQ, HPS_EX_NE, HPS_EX_AND, HPS_EX_OR, HPS_EX_NOT, HPS_EX_SELECT,
       HPS_EX_SQRT, HPS_EX_EXP, HPS_EX_LOG, HPS_EX_LOG10, HPS_EX_SIN, HPS_EX_COS, HPS_EX_TAN, HPS_EX_ASIN, HPS_EX_ACOS,
       HPS_EX_ATAN, HPS_EX_ATAN2, HPS_EX_SINH, HPS_EX_COSH, HPS_EX_TANH, HPS_EX_ABS, HPS_EX_FLOOR, HPS_EX_CEIL, HPS_EX_FMOD,
       HPS_EX_MIN, HPS_EX_MAX, HPS_EX_HEAVISIDE, HPS_EX_ERF, HPS_EX_NOPS };
#define HPS_EXPR_MAX_INS 256     /* instructions of a program */
#define HPS_EXPR_MAX_DEPTH 16    /* values on its stack */
#define HPS_EXPR_MAX_CONST 64    /* entries of its constant pool */
#define HPS_EXPR_MAX_POWI 8      /* |operand| of HPS_EX_POWI */
#define HPS_EXPR_MAX_VARS 8      /* input variables */
typedef struct { int op, arg; } hps_expr_ins;
typedef struct {
    int n_ins, n_const;
    const hps_expr_ins* ins;     /* host memory; read during the call only */
    const double* consts;
} hps_expr;
/* Walks the program once; *depth_host (may be NULL) = the deepest its stack gets.  HPS_ERR_ARG, with hps_last_error naming
 * which: a bad opcode; an operand out of range (variable >= n_vars, constant index outside the pool, integer power beyond
 * HPS_EXPR_MAX_POWI); stack underflow; stack overflow (deeper than HPS_EXPR_MAX_DEPTH); a program that does not end with
 * exactly one value; a program beyond HPS_EXPR_MAX_INS / HPS_EXPR_MAX_CONST, n_vars beyond HPS_EXPR_MAX_VARS, an empty
 * program.  Every entry point below checks its programs this way first: nothing is evaluated from an unchecked program. */
int hps_expr_check (const hps_expr* prog, int n_vars, int* depth_host);
/* out_host[i] = prog(vars_host[0][i], ..., vars_host[n_vars - 1][i]), i < n, on the CPU: the routine the kernels run
 * (csrc/expr.h), compiled for the host.  Needs no device. */
int hps_expr_eval_host (const hps_expr* prog, int n_vars, long n, const double* const* vars_host, double* out_host);
/* The same on the device, one lane per element (grid-stride), on `stream`; vars_dev: a host array of n_vars device
 * pointers.  Copies the program to the device for the call (allocates and frees) and returns when the kernel has finished
 * (synchronises the stream).  n = 0: no launch. */
int hps_expr_eval (const hps_expr* prog, int n_vars, long n, const double* const* vars_dev, double* out_dev, hps_stream stream);
/* Engine: beams.external_E(x,y,z,t) / beams.external_B(x,y,z,t) -- E, B: three programs each over (x, y, z, t), or NULL for
 * "none"; a component with n_ins = 0, or one that is the single constant 0, is absent and costs nothing.  The programs are
 * checked, copied to the device once and kept for the engine's life.  The moving beam's push then evaluates the components
 * present at every sub-step's (x, y, z) and the step's physical time -- dt * step for a fixed step, the t of
 * hps_engine_set_time otherwise: one value per step, the same for every sub-cycle and every slice a slipped particle is
 * pushed on (Hipace::m_physical_time) -- and adds them behind the gather as ApplyExternalField does
 * (particles/pusher/ExternalFields.H:50-55): ExmBy += Ex - c By, EypBx += Ey + c Bx, Ez += Ez, B += B.  The deck's
 * ext_E_slope / ext_Ez_slope are added as before; radiation reaction and spin tracking see the sum.  An engine without
 * programs launches the push it launched before.  A static beam (hipace.dt = 0) accepts the programs and is not changed by
 * them, as in the reference; the plasma never sees them.  HPS_ERR_ARG: a null handle, a call after the first
 * hps_engine_begin_step, a program hps_expr_check refuses (with its message). */
int hps_engine_set_beam_external_fields (void* handle, const hps_expr* E3, const hps_expr* B3);
/* Engine: <plasma>.density(x,y,z), min_density and density_table_file (PlasmaParticleContainer.cpp:90-119, 211-217;
 * InitParticles, PlasmaParticleContainerInit.cpp:246-313) for species 0 (plasma), 1 (ion) or an added species
 * (hps_engine_add_plasma_species; its programs join the engine's one image): progs are n_progs >= 1
 * programs over exactly (x, y, z).  z_pos = NULL with n_progs = 1 is density(x,y,z); otherwise z_pos holds n_progs strictly
 * ascending positions and the call is the density table: on a step with z = c t the program in force is the first entry with
 * z_pos >= z, the last one beyond the table (std::map::lower_bound, UpdateDensityFunction).  The program's value at a lattice
 * point (x, y, c t) is the density itself, in the deck's units: for this species it replaces <species>_density f_r f_t of
 * hps_engine_set_density_profile, in the sheet's weights (w = value * scale_fac, one multiplication; scale_fac = the cell
 * volume in SI units / ppc or fine ppc, / 4 with do_symmetrize) and in the laser's initial chi (there without min_density, as
 * SetInitialChi).  A slot holds a particle iff it passes the radius, hollow-core and prevent_centered_particle tests and
 * value > min_density; the slot count stays static.  The deck's plasma_density / ion_density keep every other role (they
 * switch the species on).  The other species, and an engine without programs, keep the tables and launch the kernels they
 * launched before.  The programs are checked, packed into one device image per engine and kept for its life.  HPS_ERR_ARG: a
 * null handle, a call after the first hps_engine_begin_step, species 1 without ion_on, species 0 with plasma_density <= 0,
 * n_progs < 1, positions that are not strictly ascending, a program hps_expr_check refuses for three variables (with its
 * message). */
int hps_engine_set_density_expr (void* handle, int species, int n_progs, const hps_expr* progs, const double* z_pos, double min_density);
/* The same programs for the adaptive time step's controller (host only): rho_max(z) takes |charge * prog(0, 0, z)| for that
 * species (0 plasma, 1 ion, 2 ... of hps_adaptive_add_species) with the program in force at z, evaluated by the routine of hps_expr_eval_host, in place of
 * |charge density f_r(0) f_t(z)|. */
int hps_adaptive_set_density_expr (void* handle, int species, int n_progs, const hps_expr* progs, const double* z_pos);
/* *out_host = rho_max(z) (MultiPlasma::maxChargeDensity, see hps_adaptive_create); changes nothing */
int hps_adaptive_rho_max (void* handle, double z, double* out_host);
/* Engine: the general fixed_ppc beam -- <beam>.density(x,y,z), min_density, u_std and random_ppc of injection_type = fixed_ppc
 * (InitBeamFixedPPC3D / InitBeamFixedPPCSlice, particles/beam/BeamParticleContainerInit.cpp:119-346; get_position_unit_cell,
 * particles/particles_utils/ParticleUtil.H:30-64) -- generated on the device in place of the deck's beam, as
 * hps_engine_set_beam_particles replaces it; whichever of the two is called last holds.  `density` is one program over exactly
 * (x, y, z).  From the deck come beam_ppc, beam_zmin, beam_zmax, beam_radius, beam_pos_mean (x, y), beam_umean, beam_charge and
 * beam_mass; beam_profile, beam_density and beam_pos_std are ignored.  Lattice point i_part of cell (i, j, k) sits at
 * lo_d + (cell_d + r_d) cell_size_d with r_d = (0.5 + i_d)/ppc_d, or a uniform draw in [0, 1) where random_ppc[d] != 0.  It is
 * dropped if z >= zmax, z < zmin or (x - x_mean)^2 + (y - y_mean)^2 > radius^2 -- tested on the point itself, with any
 * random_ppc on the lower corner of its cell instead (:166-183) -- or if density(x, y, z) <= min_density.  A particle has
 * w = |density * scale_fac| (scale_fac = 1/num_ppc, in SI units dx dy dz/num_ppc, :215-216) and u_d = (u_mean_d + u_std_d N_d) c
 * with N_d a standard normal deviate (none is drawn where u_std_d = 0).  Every draw is a function of (seed, position | momentum,
 * the point's global index ((k ny + j) nx + i) num_ppc + i_part, the component): the same deck, program and seed give the same
 * beam bit for bit.  The order is the deck beam's: slices head first, then j, i, i_part.  u_std and random_ppc may be NULL
 * (all zero).  A beam of zero particles is legal and behaves like beam_profile = -1.  Everything downstream sees an ordinary
 * beam.  HPS_ERR_ARG, with the cause in the message: a null handle or program, a call after the first hps_engine_begin_step, a
 * beam_ppc entry below 1, a negative or non-finite u_std, a min_density that is NaN or +infinity (-infinity: no lattice
 * point is dropped for its density), a program hps_expr_check refuses for three variables (one that reads t). */
int hps_engine_set_beam_fixed_ppc (void* handle, const hps_expr* density, double min_density, const double u_std[3],
                                   const int random_ppc[3], unsigned long long seed);
/* Engine: the fixed_weight beam -- injection_type = fixed_weight, profile = gaussian | can (InitBeamFixedWeight3D /
 * InitBeamFixedWeightSlice, particles/beam/BeamParticleContainerInit.cpp:348-475; the parameters of particles/beam/
 * BeamParticleContainer.cpp:137-198; GetInitialMomentum, particles/profiles/GetInitialMomentum.H:36-48) -- generated
 * on the device in place of the deck's beam; whichever beam setter is called last holds.  The struct holds the beam; the deck
 * gives the grid, the units, beam_charge and beam_mass only.  num_particles = N; nd = N/4 draws with do_symmetrize, else N.
 * Draw i < nd: z = pos_mean_z + pos_std[2] n_z (gaussian) or u (zmax - zmin) + zmin (can); x = pos_std[0] n_x, y = pos_std[1] n_y;
 * u_d = u_mean[d] + u_std[d] m_d (u_mean[d] itself where u_std[d] = 0), then u_z += (z - z_mean) duz_per_uz0_dzeta u_mean[2] with
 * z_mean = pos_mean_z (gaussian) or (zmin + zmax)/2 (can).  The draw is valid iff zmin <= z <= zmax and x^2 + y^2 <= radius^2;
 * then x -= z_foc u_x/u_z, y -= z_foc u_y/u_z (not applied where z_foc = 0) and the particle is (X(z) + x, Y(z) + y, z, u c) with
 * X = mean_x_of_z, Y = mean_y_of_z: programs over exactly one variable, z (position_mean[0], position_mean[1]).  With
 * do_symmetrize a draw gives the four particles (X +- x, Y +- y, z, +-u_x, +-u_y, u_z) in the order (+,+), (-,+), (+,-), (-,-),
 * next to each other.  Every particle has w = |total_charge/(N beam_charge)|; with charge_is_specified = 0, total_charge =
 * density beam_charge prod_d(pos_std[d] sqrt(2 pi)) (for the can profile too), times 1/(dx dy dz) in normalised units.  Every
 * deviate is a function of (seed, tag, i, component) -- tags and draws in DESIGN 8o -- never of the launch.  Valid draws are
 * binned as hps_engine_set_beam_particles bins particles (slice = int((z - lo_z)(1/dz)), head slice first), ascending i inside a
 * slice.  n_left_out (may be NULL) receives the particles left out: {of invalid draws, of valid draws outside the box in z}.
 * A beam of zero particles is legal.  On an error past the checks the engine is left without a beam.  HPS_ERR_ARG, with the
 * parameter in the message: a null handle, struct or program; a call after the first hps_engine_begin_step; num_particles <= 0,
 * or not divisible by 4 with do_symmetrize, or 2^32 draws or more; a profile other than 0 and 1; a pos_std that is not positive and
 * finite; a u_std that is negative or not finite; the can profile without finite zmin < zmax; total_charge (charge_is_specified)
 * in normalised units; z_foc != 0 with u_mean[2] = 0; a mean program hps_expr_check refuses for one variable; a beam_do_salame
 * deck with the gaussian profile and an infinite zmin or zmax (BeamParticleContainer.cpp:149-153). */
typedef struct {
    long num_particles;
    int profile;            /* 0 gaussian, 1 can */
    int do_symmetrize;
    double pos_mean_z;
    double pos_std[3], u_mean[3], u_std[3];
    double zmin, zmax, radius;      /* +-infinity allowed */
    double z_foc, duz_per_uz0_dzeta;
    double density, total_charge;
    int charge_is_specified;
} hps_beam_fixed_weight;
int hps_engine_set_beam_fixed_weight (void* handle, const hps_beam_fixed_weight* spec, const hps_expr* mean_x_of_z,
                                      const hps_expr* mean_y_of_z, unsigned long long seed, long n_left_out[2]);
/* Engine: the fixed_weight_pdf beam -- injection_type = fixed_weight_pdf (InitBeamFixedWeightPDF3D / InitBeamFixedWeightPDFSlice,
 * particles/beam/BeamParticleContainerInit.cpp:477-695; the parameters of particles/beam/BeamParticleContainer.cpp:200-240;
 * DESIGN 8p) -- generated on the device in place of the deck's beam; whichever beam setter is called last holds.  The deck gives
 * the grid, the units, beam_charge and beam_mass only.  pdf is the longitudinal profile pdf(z); progs[10] are, in this order,
 * position_mean x, position_mean y, position_std x, position_std y, u_mean x y z, u_std x y z: eleven programs over exactly one
 * variable, z; a number is a constant program.  Once, on the host, with the routine of hps_expr_eval_host and in the reference's
 * order: ns = nz pdf_ref_ratio sub-slices of width zs = dz/pdf_ref_ratio, pe[s] = pdf(lo_z + s zs) for s = 0 .. ns,
 * lw[s] = 0.5 (pe[s] + pe[s + 1]); integral = sum of lw and max_density = max of lw[s]/(zs std_x std_y 2 pi) at the sub-slice's
 * mid-point, both from s = ns - 1 down; total_weight = density integral/max_density, or total_charge/beam_charge with
 * charge_is_specified, times 1/(dx dy dz) in normalised units; every particle has w = |total_weight/N|.  uz_moments (may be NULL)
 * receives the pdf-weighted mean and standard deviation of u_z (:520-538), the pair hps_adaptive_initial_dt takes.  The table
 * cum[0] = 0, cum[s + 1] = cum[s] + lw[s].  num_particles = N; nd = N/4 draws with do_symmetrize, else N.  Draw i < nd:
 * t = unit(0) cum[ns]; s = the last index with cum[s] <= t; w = unit(1); z = (lo_z + s zs) + zs f with the reference's f
 * (:631-652): w - w (w - 1)(hi - lo)/(hi + lo) where min(lo, hi) 1.1 > max(lo, hi), (sqrt(lo^2 + w (hi^2 - lo^2)) - lo)/(hi - lo)
 * otherwise, lo = pe[s], hi = pe[s + 1]; x = std_x(z) n_x, y = std_y(z) n_y; with density the draw is invalid where x^2 + y^2 >
 * radius^2, with total_charge further pairs are drawn until one is valid (:662-666; at most 4096, then invalid); u_d =
 * u_mean_d(z) + u_std_d(z) m_d; x -= z_foc u_x/u_z, y -= z_foc u_y/u_z (not applied where z_foc = 0); the particle is
 * (X(z) + x, Y(z) + y, z, u c), with do_symmetrize its four copies as hps_engine_set_beam_fixed_weight places them.  The counts per
 * sub-slice are multinomial, where the reference iterates Poisson draws (:546-579): the beam is the reference's in distribution.
 * Every deviate is a function of (seed, tag, i, component) -- DESIGN 8p.  Binning, order and n_left_out (may be NULL) as
 * hps_engine_set_beam_fixed_weight.  On an error past the checks the engine is left without a beam.  HPS_ERR_ARG, with the
 * parameter in the message and nothing of the engine changed: a null argument; a call after the first hps_engine_begin_step;
 * num_particles <= 0, or not divisible by 4 with do_symmetrize, or 2^32 draws or more; pdf_ref_ratio < 1, or nz pdf_ref_ratio
 * beyond an int; a program hps_expr_check refuses for one variable; a pdf that is negative or not finite at an edge; integral
 * <= 0; a position_std that is not positive and finite at the mid-point of a sub-slice of positive weight; total_charge in
 * normalised units; a radius that is not positive (infinity allowed); a z_foc that is not finite. */
typedef struct {
    long num_particles;
    int do_symmetrize;
    int pdf_ref_ratio;      /* the reference's default: 4 */
    double radius;          /* +infinity allowed */
    double z_foc;
    double density, total_charge;
    int charge_is_specified;
} hps_beam_fixed_weight_pdf;
int hps_engine_set_beam_fixed_weight_pdf (void* handle, const hps_beam_fixed_weight_pdf* spec, const hps_expr* pdf,
                                          const hps_expr progs[10], unsigned long long seed, long n_left_out[2],
                                          double uz_moments[2]);

/* ---- several beam species in one moving-beam engine (driver + witness) -----------------------------------------
 * The engine keeps ONE beam container, one set of slice boundaries and one launch per phase and slice; a further species is a
 * per-particle tag (one byte) and a record of a small device table with what the push and the deposit take per species.
 * Species 0 is the deck's beam (beam_charge, beam_mass, beam_n_subcycles, ...).  hps_engine_add_beam_species appends a record
 * (*index_out: its number, 1 .. HPS_MAX_BEAM_SPECIES - 1) and switches the engine's beam kernels to their tagged instances; an
 * engine that never calls it holds no tag row and launches the kernels it always did.  mass 0 reads as 1, n_subcycles <= 0 as
 * 10, as in the deck.  uz_mean / uz_std (units of c) are kept for the adaptive controller's initial estimate only.
 * Refused, each with its reason in hps_last_error: a call after the first hps_engine_begin_step or a fifth species
 * (HPS_ERR_ARG); a static beam (hipace.dt = 0), beam_do_salame, an engine with hps_engine_add_beam_collision, species that
 * differ in do_spin_tracking (HPS_ERR_UNSUPPORTED each); hps_engine_add_beam_collision refuses an engine with several species
 * in turn.  do_salame: the species takes part in SALAME during step 0 (MultiBeam.cpp:42-59, 128-140: it deposits jz only,
 * the module scales its weights slice by slice; species 0 is then the driver, or empty behind a grid current); HPS_ERR_ARG
 * unless hps_engine_set_beam_species_salame came first; a gaussian fixed_weight source for it needs finite zmin and zmax.
 * The ring hand-off carries the tag as one more row of the message (hps_engine_beam_message_rows: 8, or 11 with spin), so every
 * engine of a pipeline is given the same species; the in-situ beam moments are kept per species
 * (hps_engine_insitu_beam_species: hps_engine_insitu_beam for species k; hps_engine_insitu_beam refuses several species).
 *
 * hps_engine_select_beam_species(k): the beam setters (hps_engine_set_beam_particles, _fixed_ppc, _fixed_weight,
 * _fixed_weight_pdf) called afterwards fill species k instead of replacing the beam: they build k's particles as they build a
 * beam (with k's charge where a weight derives from it), and k_beam_merge (beam.hip) puts them into the container: inside a
 * slice the particles already there stay in front, in their order, the new species' follow in theirs.  Species 0 is filled
 * first (replacing it later is refused); a species k > 0 is filled once.
 *
 * hps_engine_beam_species_info: *n species and their particle counts [n] (either may be NULL).
 * hps_engine_beam_state_species: species k's particles in container order -- *count of them, boundaries [nz + 1] of its slices
 * and [7][*count] x y z ux uy uz w (any of the three may be NULL); synchronises the stream.  k = -1: the whole container
 * (*count = nbeam of hps_engine_beam_info), whose tags hps_engine_beam_tags copies ([nbeam] bytes, all 0 with one species).
 * hps_engine_beam_moments_species: hps_engine_beam_moments per species, out [n][4].
 * hps_engine_beam_state and hps_engine_beam_moments refuse an engine with several species (HPS_ERR_ARG).
 * hps_engine_beam_kernels: the names of the beam kernel instances the engine has launched so far, one per line, e.g.
 * "k_beam_push<2,0,0>" (ORDER, EXT, MULTI), "k_beam_deposit_dyn<2,0>", "k_beam_partition<1,0>" (MOM, MULTI), and
 * "k_beam_deposit_dyn<2,1,1>" for the species-masked deposit that only step 0 of a SALAME engine launches; *tagged = does
 * the container hold a tag row.  buf may be NULL (then *len alone is written). */
#define HPS_MAX_BEAM_SPECIES 4
typedef struct {
    double charge, mass;
    int n_subcycles, no_z_push, radiation_reaction, do_spin_tracking;
    double spin_anom, uz_mean, uz_std;
    int do_salame;
} hps_beam_species;
int hps_engine_add_beam_species (void* handle, const hps_beam_species* species, int* index_out);
int hps_engine_select_beam_species (void* handle, int k);
int hps_engine_beam_species_info (void* handle, int* n_host, long* counts_host);
int hps_engine_beam_state_species (void* handle, int k, long* count_host, long* boundaries_host, double* soa_host);
int hps_engine_beam_tags (void* handle, unsigned char* tags_host /* [nbeam] */);
int hps_engine_insitu_beam_species (void* handle, int species, double* out_host /* [23][nz] */);
int hps_engine_beam_moments_species (void* handle, double* out_host /* [n][4] */);
int hps_engine_beam_kernels (void* handle, char* buf, long cap, long* len, int* tagged);

/* ---- further plasma species in one engine (plasmas.names beyond two; MultiPlasma.cpp) -----------------------------
 * Species 0 is the deck's plasma (the electrons), species 1 the deck's species "ion" (the ionisable one).
 * hps_engine_add_plasma_species appends a FIXED-CHARGE species behind the two (*index_out: 2, 3, ... HPS_MAX_PLASMA_SPECIES - 1,
 * also in a deck without the species "ion"): charge and mass in the deck's units, its charge is not multiplied by an ion
 * level and it never ionises.  It has a sheet, a tiling (the engine's tile size) and a second sort buffer of its own, all sized
 * by what InitParticles creates for it (ppc, fine_ppc and the engine's patch, do_symmetrize); every hps_engine_begin_step puts
 * it back on its lattice, it is re-sorted whenever the electrons are, and every per-species operator of the slice -- the
 * deposition, the explicit deposition, the committing and the temporary push, the laser's initial chi -- takes the present
 * species in index order, one launch of the tile kernels per species and phase.  fine_ppc = {0, 0}: no fine patch.
 * neutralize_background != 0: begin_step deposits the species' initial sheet with -charge into the ion rhomjz plane
 * (DepositNeutralizingBackground, MultiPlasma.cpp:106-118); species 0 keeps plasma_no_neutralize, species 1 has no background.
 * The index is accepted by hps_engine_set_plasma_momentum, hps_engine_set_density_expr and hps_engine_add_collision (either
 * side; a species that collides carries its lattice index in the id bits, as the electrons do); the tabulated density profile
 * (hps_engine_set_density_profile) is the engine's and holds for every species without a program.
 * With a further species the slice takes the general schedule: no early shift / zero pass in the multigrid, no fused push +
 * deposit, no push gated behind the V-cycles, and the predictor-corrector's loop is controlled by the host and iterates from
 * the first slice on (as with the species "ion").  An engine that never calls it allocates and launches what it always did.
 * Refused, each with its reason in hps_last_error -- HPS_ERR_ARG: a null argument; a call after the first
 * hps_engine_begin_step; a species beyond HPS_MAX_PLASMA_SPECIES; ppc < 1; density <= 0, mass <= 0 or charge == 0 (or not
 * finite); fine_ppc that is not {0, 0} and not divisible by ppc, component by component, or given together with
 * prevent_centered_particle.  HPS_ERR_UNSUPPORTED: an engine with beam_do_salame or hps_engine_set_beam_species_salame (SALAME
 * drives the electrons alone; hps_engine_set_beam_species_salame refuses an engine with a further species in turn);
 * hps_engine_add_beam_collision with a species index >= 2.
 *
 * hps_engine_plasma_species_info: *n = 2 + the species added, counts [n] = the particles of each sheet now (0: absent); either
 * may be NULL.  hps_engine_plasma_species(k): the sheet of species k (synchronises the stream; n = 0 and null arrays for an
 * absent or unknown species).  hps_engine_insitu_plasma_species: hps_engine_insitu_plasma for species k = 0 or k >= 2 (the
 * further species' buffers are allocated by the first hps_engine_begin_step behind hps_engine_set_insitu_plasma). */
#define HPS_MAX_PLASMA_SPECIES 6
typedef struct {
    double charge, mass, density;
    int ppc[2];
    int fine_ppc[2];
    int neutralize_background;
} hps_plasma_species;
int hps_engine_add_plasma_species (void* handle, const hps_plasma_species* species, int* index_out);
int hps_engine_plasma_species_info (void* handle, int* n_host, long* counts_host);
hps_plasma hps_engine_plasma_species (void* handle, int k);
int hps_engine_insitu_plasma_species (void* handle, int k, double* out_host /* [15*nz] */);
/* The adaptive time step's controller: one more species for rho_max(z) (MultiPlasma::maxChargeDensity takes the maximum over
 * all species): |charge density f_r(0) f_t(z)|, or its program after hps_adaptive_set_density_expr with the returned index
 * (2, 3, ...).  Returns the index, or -1 (a null handle, a seventh species, a charge or density that is not finite). */
int hps_adaptive_add_species (void* handle, double charge, double density);

/* ---- utilities ---------------------------------------------------------------------------- */
int hps_memcpy_d2h (void* dst_host, const void* src_dev, long bytes);
int hps_memcpy_h2d (void* dst_dev, const void* src_host, long bytes);
int hps_device_count (int* n_host);

#ifdef __cplusplus
}
#endif
#endif /* HPSLICE_H_ */
