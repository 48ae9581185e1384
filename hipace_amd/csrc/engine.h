// engine.h -- slice-engine state (device resident).
#ifndef HPS_ENGINE_H_
#define HPS_ENGINE_H_

#include "common.h"
#include "expr.h"
#include <algorithm>
#include <array>
#include <string>
#include <vector>
#include "tiling.h"
#include "mg_gate.h"
#include "particle_math.h"
#include "poisson_src.h"
#include "beam_deposit.h"
#include "slab_ops.h"
#include "particles_tiled.h"
#include "multigrid.h"

namespace hps {

constexpr int PC_MAX_SPEC = 64;      // flags / host slots of the device-controlled predictor-corrector loop: iterations 1 .. 62

bool poisson_gateable (void* poisson_handle);
void poisson_set_gate (void* poisson_handle, const int* gate);
bool ring_is_ticket (const void* p);      // ring.hip: is p the receive handle of an ipc ring edge (not a hipEvent_t)?

struct LaserState;      // laser.hip

// a density program as a kernel argument: the instructions of the table entry in force and the pooled constants,
// both on the device, z = c t of the step and <plasma>.min_density.  n_ins = 0: no program
struct DensityProgram { const hps_expr_ins* ins; int n_ins; const double* consts; double z, min_density; };

// Expression programs packed into one image (expr.hip): on the host the instruction stream -- behind `header_slots` words the
// owner fills in itself, slot() -- and the pooled constants; after upload() the same two arrays on the device, freed with the
// image (move-only).
struct ExprImage {
    ExprImage () = default;
    explicit ExprImage (int header_slots) : h_ins((size_t)header_slots, hps_expr_ins{0, 0}) {}
    int add (const hps_expr& checked);                   // appends a CHECKED program -> offset of its first instruction
    hps_expr_ins& slot (int q) { return h_ins[(size_t)q]; }
    int n_ins () const { return (int)h_ins.size(); }
    int upload ();
    const hps_expr_ins* ins () const { return d_ins.get(); }
    const double* consts () const { return d_consts.get(); }
private:
    std::vector<hps_expr_ins> h_ins; std::vector<double> h_consts;
    DevBuf<hps_expr_ins> d_ins; DevBuf<double> d_consts;
};

struct BeamSoA { double *x, *y, *z, *ux, *uy, *uz, *w; int* nsub;      // moving beam (beam.hip); nsub < 0: absorbed
                 double *sx, *sy, *sz;                                 // spin (do_spin_tracking), null otherwise
                 unsigned char* sp; };                                 // species tag, null in a one-species engine

// Several beam species in one container (hps_engine_add_beam_species): what the push and the deposit take per species,
// one record per species in a small device table (Engine::d_bsp_tab) that every lane of a MULTI kernel indexes with its tag.
struct BeamSpeciesRec { double q_invvol, qm, dt, RRcoeff, spin_anom; int nsc, rr, no_z_push; };
struct BeamSpeciesTable { BeamSpeciesRec r[HPS_MAX_BEAM_SPECIES]; };
// the table as a kernel argument: nothing in the kernels of a one-species engine
template <bool MULTI> struct BeamMultiArgs {};
// (mask: the species a SEL deposit takes, bit k = species k; read by k_beam_deposit_dyn<ORDER, true, true> alone)
template <> struct BeamMultiArgs<true> { const BeamSpeciesRec* tab; int ns; unsigned mask; };

// cell lists of the collision kernels (collisions.hip): per species slot the exclusive cell offsets [ncells + 1] and the
// cell-sorted particle indices; cnt [ncells + 1] is shared (zero between launches); stats = {pairs collided, overfull cells}
struct CollScratch {
    unsigned *cnt = nullptr, *off[2] = {nullptr, nullptr}, *perm[2] = {nullptr, nullptr};
    long cap[2] = {0, 0}; int ncells = 0; void* temp = nullptr; size_t temp_bytes = 0; unsigned long long* stats = nullptr;
    CollScratch () = default; CollScratch (const CollScratch&) = delete; CollScratch& operator= (const CollScratch&) = delete;
    ~CollScratch ();
};

// the container's blocks, offsets, tags and particle count set aside while a setter builds the next species' beam
struct BeamStash { double* blocks = nullptr; unsigned char* tag = nullptr; std::vector<long> off; long n = 0; bool host_beam = false;
                   double charge = 0.0, mass = 0.0; };

struct Engine {
    hps_deck d{};
    hps_geom gm{};
    int g = 0, ncomp = 0;
    hipStream_t st = nullptr;
    bool st_pooled = false; int st_device = 0;       // the stream came from the per-device pool (stream_pool.hip: create_engine_stream)
    hps_slab slab{};
    // ADK field ionisation of the species "ion" (ionization.hip): it is tile-sorted once per step (ions hardly move); released
    // electrons are appended to the plasma's sheet behind the tile-sorted body and run through the per-particle kernels until
    // the next re-sort.  Counters on the device {electrons, overflow, blocks done, ionised}, the count comes back through mapped
    // host memory (no stream synchronisation).
    struct Ions { double* d_adk = nullptr; unsigned long long* d_cnt = nullptr; long long* h_cnt = nullptr; long long* h_cnt_dev = nullptr;
                  long long seq = 0; long n_ionized = 0; bool pending = false; int* d_tile_flag = nullptr;
                  double* d_fbound = nullptr;       // [5][tiles] field maxima of the slice (k_ion_field_bounds; HPS_ION_TILE_SKIP=0: off)
                } ion;
    // tabulated plasma density profile (hps_engine_set_density_profile): radial table on the device, time table on the host
    std::vector<double> prof_r, prof_t, prof_f_t; double* d_prof_r = nullptr; double prof_ft = 1.0;
    // <plasma>.fine_patch / fine_ppc / fine_transition_cells / hollow_core_radius (plasma_init.hip): the level map
    // [ny][nx] (0 coarse, 1..T transition, T + 1 fine) and the x-fastest list of the cells with level > 0, shared by the species
    double hollow_core_radius = 0.0;
    bool fine_patch_set = false; int fine_T = 0; long fine_ncells = 0; int* d_fine_level = nullptr; int* d_fine_cells = nullptr;
    // <plasma>.u_mean / u_std (temperature_in_ev), plasmas.do_symmetrize, prevent_centered_particle (plasma_init.hip):
    // the momenta per species (Species::thermal); the two switches hold for every species
    struct Thermal { double u_mean[3] = {0.0, 0.0, 0.0}, u_std[3] = {0.0, 0.0, 0.0}; unsigned long long seed = 0;
                     bool warm () const { for (int q = 0; q < 3; ++q) if (u_mean[q] != 0.0 || u_std[q] != 0.0) return true; return false; }
                   };
    bool do_symmetrize = false, prevent_centered = false;
    bool shifted (const int ppc[2], int dir) const { return prevent_centered && (dir == 0 ? d.nx : d.ny) % 2 == 1 && ppc[dir] % 2 == 1; }
    int set_plasma_momentum (int species, const double* u_mean, const double* u_std, unsigned long long seed);
    int set_plasma_symmetry (int symmetrize, int prevent_centered_particle);
    int alloc_sheets ();
    int set_plasma_init (const int* plasma_fine, const int* ion_fine, double hollow_core);
    int set_fine_patch (const unsigned char* mask_host, int transition_cells);
    // fused push(k) + deposit(k-1) (k_advance_deposit_tiled): ahead_for = slice whose plasma currents are already deposited
    bool fuse_push_deposit = false; int ahead_for = -2;
    long fallback_div = 256;                    // re-sort once more than el.pl.n / fallback_div particle visits since the last sort left their tile's halo (HPS_SORT_FALLBACK_DIV)
    bool gate_push = true;                      // push enqueued behind the multigrid's V-cycles, gated on its stopping rule (HPS_GATED_PUSH=0: off)
    int step_index = -1;           // physical time step that has begun (density profile's time factor, ionisation draws)
    int next_step = -1;            // hps_engine_set_step: the step the next begin_step starts (-1: the one after step_index)
    // hps_engine_set_time (hipace.dt = adaptive): time and dt of the step the next begin_step starts; step_dt is what the
    // beam push of the step that has begun uses (the deck's dt unless set)
    bool time_set = false; double next_t = 0.0, next_dt = 0.0, step_dt = 0.0;
    // physical time of the step that has begun (Hipace::m_physical_time): d.dt*step_index, or the t of hps_engine_set_time
    double step_time = 0.0;
    // beams.external_E / external_B as expression programs (hps_engine_set_beam_external_fields, beam_ext.hip): one
    // device image -- six {offset, count} header slots (Ex Ey Ez Bx By Bz; count 0: absent), then the instructions -- and
    // the pooled constants; depth = the deepest stack of the six.  on = false: k_beam_push<ORDER, false>, the push as it was.
    struct BeamExt { bool on = false; ExprImage image; int depth = 0; } bext;
    int set_beam_external_fields (const hps_expr* E3, const hps_expr* B3);
    // <plasma>.density(x,y,z) / density_table_file as expression programs (hps_engine_set_density_expr, plasma_init.hip, DESIGN
    // 8m), per species (Species::dens): the species' programs as given (z_pos empty: the one program of density(x,y,z)), the
    // offset of each in the engine's one device image (every species' instructions, the pooled constants), the deepest stack
    // of the species' programs, and the entry in force in the step that has begun.  on = false: the tables, the kernels as they were.
    struct DensityExpr { bool on = false; std::vector<std::vector<hps_expr_ins>> ins; std::vector<std::vector<double>> consts;
                         std::vector<double> z_pos; std::vector<int> off; int depth = 0; double min_density = 0.0; int cur = 0; };
    ExprImage dens_image; double dens_z = 0.0;      // dens_z: c t of the step that has begun
    int set_density_expr (int species, int n_progs, const hps_expr* progs, const double* z_pos, double min_density);
    void density_begin_step (double ct);                  // UpdateDensityFunction(c t): the table entry in force
    DensityProgram density_program (int species) const;   // n_ins = 0: this species keeps the tables
    size_t density_lds (int species) const { const DensityExpr& D = sp[species].dens; return D.on ? expr_lds_bytes(D.depth, 256) : 0; }
    // One plasma species of the slice: sp[0] the plasma (the electrons), sp[1] the species "ion", sp[2 ..] the fixed-charge species
    // of hps_engine_add_plasma_species.  The parameters are the deck's plasma_* / ion_* fields, read once
    // (Engine::create; keyed: the first begin_step) or the added record's; fine_ppc, thermal and dens are what
    // hps_engine_set_plasma_init / _momentum / _density_expr have given.
    struct Species {
        int index = 0;                                  // the species' number in the C ABI and in the key of its random draws
        // the sheet and the second buffer of the tile sort (sort.hip), each one block of 11 arrays + idcpu, ion_lev (soa_arrays);
        // the particles NOW are pl.n (the plasma's grows when the species "ion" releases electrons)
        hps_plasma pl{}, pl_alt{}; double *real = nullptr, *real_alt = nullptr; Tiling* tiling = nullptr;
        long cap = 0, n_init = 0;                       // capacity of the arrays; particles InitParticles creates
        int ppc[2] = {0, 0}, fine_ppc[2] = {0, 0}; double density = 0.0, charge = 0.0, mass = 0.0;
        int init_level = 0, can_ionize = 0, keyed = 0;  // keyed: the lattice index in the id bits (the ions; electrons that collide)
        bool temp_push = false;                         // pushed to temporary slices from x_prev: predictor-corrector; the plasma under SALAME
        bool neutralize = false;                        // its initial sheet with -charge into the ion rhomjz plane (the electrons: unless plasma_no_neutralize)
        bool grows_tail = false;                        // particles are appended behind the tile-sorted body (the electrons alone): fold_tail_of
        bool by_weight = false;                         // Engine::valid_by_w holds for its depositions (the electrons alone)
        const int* tile_flag = nullptr;                 // per tile "holds charged particles" (the ions': Ions::d_tile_flag, setup_tiling); null: every tile is worked
        Thermal thermal; DensityExpr dens;
        bool present () const { return density > 0.0; } // is the species in the deck
        // Without pushes to a temporary slice every push commits its state, so x_prev == x and y_prev == y at all times
        // (PlasmaParticleAdvance.cpp:176-188): alias them -- two arrays less to write per push and to move per re-sort.
        // The C ABI keeps 11 pointers; the kernels skip the second store when two coincide.
        bool alias_prev () const { return !temp_push; }
        // the sheet as the tile launchers take it (particles_tiled.h); sign = -1: the neutralising background
        TileSheet sheet (double sign = 1.0) const { return {pl, sign*charge, mass, can_ionize, tiling}; }
    } sp[HPS_MAX_PLASMA_SPECIES];
    Species &el = sp[0], &ions = sp[1];
    // Further species: the slots behind the two (absent slots hold no particles and every per-species loop passes them by).
    // With one the electrons are not alone: the slice takes the general schedule wherever a fast one reads "one species only"
    int n_sp = 2;
    bool further () const { return n_sp > 2; }
    int add_plasma_species (const hps_plasma_species* s, int* index_out);
    bool plasma_species_ok (int k) const { return k >= 0 && k < n_sp; }      // an index the C ABI takes (present or not)
    // does this species' sheet come from k_init_plasma_warm?  (false: the kernels and arguments of a deck without these keys)
    bool warm_init (const Species& s) const { return s.thermal.warm() || do_symmetrize || shifted(s.ppc, 0) || shifted(s.ppc, 1); }
    long sheet_slots (const Species& s) const;
    int init_sheet (Species& s);               // InitParticles of one species' sheet: the warm, the fine or the plain kernel
    int sort_sheet (Species& s);               // tile sort into the second buffer, then the two change places
    bool host_beam = false;        // hps_engine_set_beam_particles has given the beam
    double* d_mom = nullptr;       // hipace.dt = adaptive: beam moments [nz + 1][n species][4] (beam.hip: k_beam_partition<true>)
    // Beam species.  bsp[0] is the deck's beam; hps_engine_add_beam_species appends.  With more than one the container
    // carries a tag row (bm.sp, its twin for the partition bm_scr.sp) and the beam kernels are the MULTI instantiations, which read
    // the per-species constants from d_bsp_tab (written once per step: the sub-cycle's dt is the step's).  beam_tag: the tags in the
    // order of beam_init's blocks (null: all 0); sel_species: whom the beam setters fill (hps_engine_select_beam_species).
    // off: the species' own slice offsets [nz + 1] (head first) as its setter left them, kept at merge time: the particles of a
    // slice that have not slipped in during step 0 (MultiBeam::isSalameNow) without a device read
    struct BeamSpecies { hps_beam_species s{}; long count = 0; bool filled = false; std::vector<long> off; };
    std::vector<BeamSpecies> bsp; int sel_species = 0;
    unsigned char *bm_sp = nullptr, *bm_sp_scr = nullptr, *beam_tag = nullptr; BeamSpeciesRec* d_bsp_tab = nullptr;
    unsigned long beam_launched = 0;      // which beam kernel instances this engine has launched (beam.hip: beam_kernel_names)
    int n_beam_species () const { return std::max<int>(1, (int)bsp.size()); }
    bool multi_beam () const { return bsp.size() > 1; }
    int add_beam_species (const hps_beam_species* s, int* index_out);
    int alloc_beam_tags ();                                             // bm.sp and its twin for the container as it is (zeroed)
    // a beam setter's work `set` for the selected species: species 0 -> as it was; k > 0 -> the setter builds k's beam with k's
    // charge and mass through the one install tail, then k_beam_merge puts it behind what the container held (beam.hip)
    template <class F> int fill_selected_species (const char* fn, F&& set);
    int stash_beam_for_merge (const char* fn, BeamStash& A);
    int merge_stashed_beam (BeamStash& A, int e_setter);
    IonArgs ion_args (int islice);             // ionization.hip: kernel arguments of this slice's ionisation
    int ionize_slice (int islice);             // ...: launch of the per-particle form
    int ionize_collect ();                     // ...: wait for the electron count of the slice
    int ion_field_bounds ();                   // ...: per-tile field maxima for the tile skip of the ions' push
    bool fold_tail = true;                     // the particles behind the tile-sorted body ride in the tile kernels' launches (HPS_FOLD_TAIL=0: off)
    TailWork fold_tail_of (const Species& s, long margin, long* covered) const;
    // the engine-wide part of the tile launchers' record (particles_tiled.h); every launch of the engine builds it here
    TileEnv tile_env () const { return {slab, gm, d.order, st, d_nfallback, c_aabs}; }
    // the skeleton of the three operators below: tiled(tail's workgroups) over the sorted body, plain(sheet) over a sheet without tiles and over what
    // lies behind the body and its tail.  live_tail: the caller's tail, whose count is read on the device -- what lies behind it is the caller's too
    template <class Tiled, class Plain> int species_op (const Species& s, const TailWork* live_tail, Tiled&& tiled, Plain&& plain);
    // (go: the gate word of an iteration of the predictor-corrector loop's device-side control, null otherwise)
    int species_deposit (const Species& s, const int comp[6], const BeamPairWork* beam = nullptr, const int* go = nullptr);
    bool valid_by_w = true;                    // HPS_VALID_BY_W=0: off.  The depositions take "weight != 0" for the valid bit of idcpu and do not read it (PartConsts::valid_by_w:
                                               // 33.5 MB less per kernel at 1024^2 x 4 ppc -- no time gained with one stage on the GPU, +1 % with three in flight: r04g_ab_inflight_byte_cuts.txt)
    bool valid_by_psi = true;                  // HPS_VALID_BY_PSI=0: off.  The electrons' tiled push takes "psi_half != 0" for the valid bit of idcpu and does not read it (Tiling::valid_by_psi;
                                               // 33.5 MB less per launch at 1024^2 x 4 ppc); read when the engine is created, handed to the electrons' tiling when that is set up
    bool post_in_push = true;                  // the gated plasma push posts the Bx/By solve's norms to the host (HPS_POST_IN_PUSH=0: k_post_norms, a launch of its own)
    bool fold_hierarchy = true;                // the multigrid's coefficient hierarchy in the -grad Psi / Sx, Sy launch (HPS_FOLD_HIERARCHY=0: in mg_solve1_begin)
    bool fold_beam = true;                     // the static beam's two deposits of a slice as extra workgroups of the plasma's deposition (HPS_FOLD_BEAM=0: a launch of their own)
    int species_explicit (const Species& s, const int cache[4], const int depos[2]);
    // (ion: the ADK decisions of the committing push of the ionisable species, taken inside its tile kernel -- push_with_ionization)
    int species_advance (const Species& s, const int comp[5], int temp_slice, const int* go = nullptr, const IonArgs* ion = nullptr,
                         const TailWork* live_tail = nullptr);
    // the tile sort (sort.hip) and the plasma's re-sort rule
    int tile_size = 16, sort_period = 128, since_sort = 0;
    int* d_nfallback = nullptr;                 // word 0 of the multigrid norm buffer's header slot (mg_rider)
    const int* h_nfallback = nullptr;           // its pinned image, refreshed by every multigrid solve
    long fb_at_sort = 0; int n_sorts = 0;       // adaptive re-sort: fallbacks at the last sort, number of sorts
    int setup_tiling ();
    int resort ();
    void* ps = nullptr;            // Poisson solver handle
    void* mg = nullptr;            // multigrid handle
    double* staging = nullptr;
    double* d_open_mom = nullptr;      // boundary.field = Open: the multipole moments of up to four sources (Engine::open_boundary)
    int open_boundary (int nbatch, unsigned no_monopole_mask);
    // driver beam: slice-major SoA (head slice first), static because hipace.dt = 0
    // blocks [slice p from the head][7][count_p]; beam_cur = storage in use (own or caller's)
    double* beam_data = nullptr; double* beam_init = nullptr; double* beam_cur = nullptr;
    long nbeam = 0; std::vector<long> beam_off;
    // hipace.dt != 0 (beam.hip): global SoA + device-resident slice boundaries B[nz+1] and slipped-front counts
    bool moving = false; int steps_begun = 0; int beam_rows = 7;     // rows of a hand-off message (10 with spin)
    BeamSoA bm{}, bm_scr{}; double* bm_store = nullptr; int* bm_nsub = nullptr; int* bm_nsub_scr = nullptr;
    long* d_B = nullptr; int* d_nfront = nullptr; std::vector<long> h_B;      // h_B: boundaries as of begin_step
    // ring hand-off: import mode (the slices of the coming step arrive as messages), start offsets of the imported
    // blocks, per-message capacity, overflow counter
    bool beam_import = false; long* d_Bimp = nullptr; long beam_cap = 0; int* d_beam_overflow = nullptr;
    // upper bound of slice p's size during this step.  A particle may slip through SEVERAL slices in one step (it is
    // pushed again on every slice it lands on, BeamParticleAdvance.cpp:131 "IncludingSlipped"), so everything ahead of
    // slice p counts: own + all of slices 0..p-1 as of begin_step.  The kernels loop grid-stride over the device-side
    // count, so the bound only sizes (and caps) the launch.
    long beam_bound (int p) const {
        if (p < 0 || p >= d.nz) return 0;
        if (beam_import) return std::max(nbeam, 1L);
        return h_B[p + 1] - h_B[0];
    }
    // support of the beam currents in padded-array cells (deposit footprint + the centred differences taken of
    // them); the beam planes are identically zero outside, so the slab kernels skip them there
    struct Box { int ilo, ihi, jlo, jhi; };
    Box beam_box{0, -1, 0, -1}, beam_box_init{0, -1, 0, -1}, full_box{0, -1, 0, -1};
    int* d_nqsa = nullptr;
    double* d_checksum = nullptr;
    bool diagnostics = false;
    bool profiling = false; bool prof_light = false; int prof_stride = 1; bool prof_now = false;      // events on every prof_stride-th slice
    std::vector<hipEvent_t> ev; size_t ev_used = 0;      // 11 events per profiled slice
    std::vector<hipEvent_t> hand_ev;                     // hps_engine_record_event pool (no timing)
    void mark ();
    long total_vcycles = 0, slices_done = 0;
    // predictor-corrector Bx/By (hipace.bxby_solver = predictor-corrector): d_pc = {sum |B|, sum |B - B_iter|, halo
    // fallback counter (int), spare}, h_pc its pinned image read back once per iteration
    // device-side control of the loop (HPS_PC_SPECULATE=0: off): per-iteration flags, iterations enqueued ahead of the host
    int* d_pc_dist = nullptr;  // predictor-corrector: device word "something other than rounding residue has been deposited in this sweep" (Engine::pc_create)
    double pc_floor = 0.0;     // sum |B| below this is the exact zero of the serial path (Engine::pc_create)
    int* d_pc_go = nullptr; bool pc_speculate = false; int pc_spec_iters = 1, pc_enqueued = 0, pc_islice = -1; double pc_base_seq = 0.0, pc_last_err = 0.0;
    int solve_slice_pc_begin (int islice); int solve_slice_pc_finish (int islice); int pc_enqueue_iteration (int it); int pc_wait_slot (int slot, double seq);
    int pc_create (); int pc_slice_ready () const;      // (predcorr.hip: Engine::create's part; hps_engine_slice_ready's answer)
    bool pc = false; double* d_pc = nullptr; double* d_pc_aux = nullptr; double* h_pc = nullptr; double* h_pc_dev = nullptr; double pc_seq = 0.0; long pc_iterations = 0; double pc_err_sum = 0.0; long pc_zero_b_slices = 0;
    double pc_tol = 4e-2, pc_mix = 0.05; int pc_max_iter = 30;
    int c_aabs = -1; double* d_laser_sum = nullptr;       // laser: slab component of |a|^2, device sum of |a| (diagnostics)
    LaserState* laser = nullptr;                          // envelope arrays + solver (laser.hip)
    // lasers.n_cell / patch_lo / patch_hi / interp_order (hps_engine_set_laser_grid): the envelope on a grid of its
    // own -- nx x ny cells on the patch lo .. hi (z snapped to the field slices zlo .. zhi), GetPosOffset xoff, yoff of that
    // box.  Not set: the envelope lives on the field grid and chi, |a|^2 pass cell by cell.
    struct LaserGrid { bool set = false; int nx = 0, ny = 0, zlo = 0, zhi = -1, order = 1;
                       double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, dx = 0.0, dy = 0.0, xoff = 0.0, yoff = 0.0; } lgrid;
    int set_laser_grid (const int* n_cell, const double* patch_lo, const double* patch_hi, int interp_order);
    // the initial envelope: hps_engine_set_laser_pulses (pulses_set: the list replaces the deck's pulse) and
    // hps_engine_add_laser_samples (host copies, uploaded, added and freed by the first begin_step)
    struct LaserSamples { int geometry = 0; long extent[3] = {0, 0, 0}; double offset[3] = {0, 0, 0}, spacing[3] = {0, 0, 0}, unit = 1.0;
                          std::vector<double> data; };
    bool laser_pulses_set = false; std::vector<hps_laser_pulse> laser_pulses; std::vector<LaserSamples> laser_samples;
    bool insitu_laser = false;       // hps_engine_set_insitu_laser; the buffer lives with the laser grid (LaserState)
    bool laser_has_slice (int islice) const { return !lgrid.set || (islice >= lgrid.zlo && islice <= lgrid.zhi); }      // UseLaser(islice)
    // The envelope's advance of a slice needs chi of the slice and the envelope of the slices before it -- nothing else
    // of the slice needs its result.  It runs on a stream of its own beside the explicit deposition, the Bx/By multigrid
    // and the push (HPS_LASER_ASYNC=0: on the engine's stream, in the reference's place, Hipace.cpp:637).
    hipStream_t st_laser = nullptr; hipEvent_t ev_lfork = nullptr, ev_ldone = nullptr;
    bool laser_async = true, laser_pending = false;
    // Small kernels of a slice that wait for nothing on its critical path run on a stream of their own beside it: the beam's
    // deposition (needs the zeroed beam planes; wanted by the Sx/Sy initialisation behind the Poisson solves) and the
    // multigrid's coefficient hierarchy (needs chi; wanted by the Bx/By solve).  Measured: 1453-1458 slices/s against 1452-1470 without -- the two event waits cost what the
    // 14 us of kernels off the chain save -- so this is off unless HPS_AUX_STREAM=1
    hipStream_t st_aux = nullptr; hipEvent_t ev_aux[3] = {nullptr, nullptr, nullptr}; bool aux_on = false, aux_pending = false;
    hipStream_t laser_stream () const { return (laser_async && st_laser) ? st_laser : st; }
    int fork_laser ();          // the laser stream may read what the engine's stream has written so far
    int laser_done ();          // mark the end of the laser stream's work of this slice
    int join_laser ();          // the engine's stream waits for the laser stream's last slice (no-op if none is pending)
    // field diagnostic (Fields::Copy): components, coarsening, device array [ncomps][nzc][nyc][nxc]
    std::vector<int> fd_comps; int fd_c[3] = {1, 1, 1}; double* d_fd = nullptr; int* d_fd_comps = nullptr;
    // geometry of the diagnostic grid (Diagnostic::ResizeFDiagFAB + TrimIOBox, diagnostics/Diagnostic.cpp:300-410): cells, cell
    // size, position of local cell 0 (GetPosOffset of the diagnostic geometry + first index * cell size), real box, slice direction
    int fd_n[3] = {0, 0, 0}; double fd_h[3] = {0, 0, 0}, fd_pos0[3] = {0, 0, 0}, fd_lo[3] = {0, 0, 0}, fd_hi[3] = {0, 0, 0}; int fd_slice_dir = -1;
    size_t fd_cells () const { return (size_t)fd_n[0]*fd_n[1]*fd_n[2]; }
    int fill_field_diagnostic (int islice);
    double* d_insitu_bm = nullptr; double insitu_bm_radius = 0.0;     // [23][nz] raw sums of the beam moments
    void insitu_beam (int islice);
    double* d_insitu_pl = nullptr; double insitu_pl_radius = 0.0;     // [15][nz] raw sums of the plasma moments
    double* d_insitu_pl_more = nullptr;                               // ... of the further species, [n_sp - 2][15][nz] (begin_step)
    double* d_insitu = nullptr;      // [10][nz] in-situ field reductions (Fields::InSituComputeDiags)
    void insitu_plasma (int islice); void insitu_fields (int islice); void checksum_slice ();      // diagnostics.hip: no-ops unless switched on

    ~Engine ();
    int create (const hps_deck& deck, int device);
    int init_beam ();
    int install_beam (std::vector<double> (&h)[7]);
    int set_beam_particles (long n, const double* soa_host, long* n_outside);
    // beam_init.hip: the general fixed_ppc beam, generated on the device; install_beam_device takes its blocks
    // (ownership too: they become beam_init) with beam_off filled in and box = {xlo, xhi, ylo, yhi} of the particles
    int set_beam_fixed_ppc (const hps_expr* density, double min_density, const double* u_std, const int* random_ppc, unsigned long long seed);
    // ... and the fixed_weight beam (gaussian | can): num_particles draws sorted into the slices on the device
    int set_beam_fixed_weight (const hps_beam_fixed_weight* spec, const hps_expr* mean_x, const hps_expr* mean_y, unsigned long long seed,
                               long* n_left_out);
    // ... and the fixed_weight_pdf beam: z from the table of pdf(z), means and widths as programs over z
    int set_beam_fixed_weight_pdf (const hps_beam_fixed_weight_pdf* spec, const hps_expr* pdf, const hps_expr* progs, unsigned long long seed,
                                   long* n_left_out, double* uz_moments);
    int install_beam_device (double* blocks_dev, long n, const double box[4]);
    // ... the three share: everything between "all arguments are checked" and the first allocation; the extent of the n particles
    // of `blocks` (beam_off filled in) and install_beam_device; the one failure path: the engine is left without a beam, -> e
    int begin_device_beam (long* n_left_out = nullptr);
    int finish_device_beam (DevBuf<double>& blocks, long n, long* n_left_out = nullptr);
    int drop_device_beam (int e, long* n_left_out);
    void release_beam ();                                               // the beam's device storage, ahead of another beam
    void set_beam_box (double xlo, double xhi, double ylo, double yhi);  // beam_box_init from the particles' extent
    int install_moving_beam (const std::vector<double> (*h)[7]);        // the moving beam's storage; h null: filled from beam_init on the device
    int begin_step ();
    int deposit_beam_slice (int islice, int cjx, int cjy, int cjz, const int* go = nullptr);
    void deposit_grid_current (int islice, int cjz);
    int solve_slice (int islice);
    int solve_slice_begin (int islice);      // ... in two halves: everything up to the Bx/By solve's norm read-back is enqueued,
    int solve_slice_finish (int islice);     // then the host waits for the norms and enqueues the rest
    int pending_slice = -1; bool pend_fuse = false, pend_gated = false, pend_gated_ion = false;
    bool gate_ion_push = true; IonArgs pend_ia{};      // the ionisable species' push + the electrons' push behind the V-cycles (HPS_GATED_ION_PUSH=0: off)
    long pend_covered = 0;                             // the electrons the gated push_with_ionization's launch has room for (solve_slice_begin -> _finish)
    // (*covered: the electrons its launch has room for; -1: it launched none of them -- no tiling, or nothing sorted)
    int push_with_ionization (int islice, const int comp[5], const int* go, bool first, long* covered);
    int push_ions (int islice, const int comp[5], const int* go, bool first);      // ... its first half: the decisions and the ions' push
    int push_leftover (const int comp[5], long covered);      // the electrons behind `covered`, once ionize_collect has their count
    bool lazy_shift = true, shift_pending = false;      // ShiftSlices deferred to the next slice's InitializeSlices pass (HPS_LAZY_SHIFT=0: off)
    void flush_shift ();
    // HPS_EARLY_INIT (=0: off): on the plain path the next slice's shift / zero pass rides in the launch of the Bx/By solve's first
    // lower V (mg_ride_shift_init).  The planes it re-initialises have an alternate behind the slab's own (n_alt of them, not
    // counted by hps_engine_slab) and the slices take turns: `live` = the set this slice deposits into.  init_done: the live set
    // holds the next slice's zeros and the shift is done, the slice just solved is in the other set.
    bool early_init = true; int n_alt = 0; InitSet set_canon{}, set_alt{};
    bool alt_live = false, init_done = false, pend_rode = false; long slices_rode = 0;
    const InitSet& live () const { return alt_live ? set_alt : set_canon; }
    const InitSet& other () const { return alt_live ? set_canon : set_alt; }
    bool fuse_sources = true;      // the Poisson sources formed inside the first transform pass (HPS_FUSE_SOURCES=0: k_rhs_all + staging planes)
    // <beam>.do_salame (salame/Salame.cpp): c_sal = first of the HPS_SAL_NCOMP planes behind the engine's own (-1: none);
    // state of the run of consecutive slices (Hipace::m_salame_last_slice, m_salame_overloaded, m_salame_zeta_initial);
    // d_sal = scratch of the W reduction; sal_stats = [nz][4] {W, W_total, iterations, flags}
    int c_sal = -1; int sal_last_slice = -2; bool sal_overloaded = false; double sal_zeta_initial = 0.0;
    double* d_sal = nullptr; std::vector<double> sal_stats;
    bool salame_now () const { return c_sal >= 0 && step_index == 0; }      // MultiBeam::isSalameNow without the particle count
    // A moving-beam engine (hps_engine_set_beam_species_salame -> species_salame): the do_salame species as a mask (bit k =
    // species k; 0: none added), every species, and the SALAME particles slice p (from the head) held when step 0 began
    unsigned salame_mask () const { unsigned m = 0; for (size_t k = 0; k < bsp.size(); ++k) if (bsp[k].s.do_salame) m |= 1u << k; return m; }
    unsigned species_mask_all () const { return (1u << n_beam_species()) - 1u; }
    long salame_count (int p) const {
        long n = 0;
        for (const BeamSpecies& b : bsp) if (b.s.do_salame && (long)b.off.size() == d.nz + 1 && p >= 0 && p < d.nz) n += b.off[(size_t)p + 1] - b.off[(size_t)p];
        return n;
    }
    bool species_salame = false; int set_beam_species_salame (int on);
    int salame_module (int islice);
    int salame_solve_ez ();
    int run_step ();
    // hipace.collisions (collisions.hip): Coulomb collisions between plasma species, species 0 = plasma, 1 = ion, and between
    // the moving beam and plasma species b (beam; a is unused); one list, run in order at the end of every slice, behind the
    // beam's push and partition (Hipace.cpp:704-712).  Empty: no launch, no allocation.
    struct Collision { int a, b; double coulomb_log; unsigned long long seed; bool beam = false; };
    std::vector<Collision> coll; CollScratch coll_scratch; bool step_begun = false;
    int collide_slice (int islice);
};

template <class F> int Engine::fill_selected_species (const char* fn, F&& set)
{
    if (sel_species == 0) {
        for (size_t k = 1; k < bsp.size(); ++k)
            HPS_REQUIRE(!bsp[k].filled, std::string(fn) + ": species 0 cannot be replaced once another beam species holds particles");
        const int e = set();
        if (!bsp.empty()) { bsp[0].count = nbeam; bsp[0].filled = e == HPS_OK && nbeam > 0; }
        if (e == HPS_OK && multi_beam()) return alloc_beam_tags();
        return e;
    }
    BeamStash A;
    if (int e = stash_beam_for_merge(fn, A)) return e;
    return merge_stashed_beam(A, set());
}

int ion_create (Engine& E);                                                  // ionization.hip
void ion_destroy (Engine& E);
unsigned event_flags (bool timing);                                           // engine.hip
hipError_t create_engine_stream (hipStream_t* s, int device, bool* pooled);   // stream_pool.hip: from the device's pool where there is one
void return_engine_stream (hipStream_t st, int device);                       // ...: a pooled stream back to it
__global__ __launch_bounds__(256) void k_beam_new_step (int* nsub, long n);   // beam_host.hip (begin_step launches it)
void beam_deposit_pair (const hps_slab& slab, const BeamPairWork& bw, const hps_geom& gm, int order, hipStream_t st);      // ...: k_beam_deposit_pair
// The 11 double arrays of a sheet in the order of its block, and what is built on it (engine.hip): a block of cap slots with
// idcpu and ion_lev (alias: x_prev, y_prev are x, y -- Species::alias_prev) and its release
std::array<double**, 11> soa_arrays (hps_plasma& p);
int alloc_soa (hps_plasma& p, double*& real, long cap, bool alias);
void free_soa (hps_plasma& p, double*& real);
// plasma_init.hip: InitParticles with the fine patch and / or the hollow core for one species' sheet
// (and, with a density program, for the plain lattice: init_slot's rule of the weight, one place)
int init_plasma_fine (Engine& E, const Engine::Species& s, double radius_sq);
// ...: the same sheet with Gaussian momenta, its mirror copies and / or the lattice shifted off the axis (Engine::warm_init)
int init_plasma_warm (Engine& E, const Engine::Species& s, double radius_sq);
int laser_create (Engine& E);                                                // laser.hip
void laser_destroy (Engine& E);
int laser_begin_step (Engine& E);
int laser_update_aabs (Engine& E, int islice, double* sum_abs);
int laser_advance_slice (Engine& E, int islice);
int laser_copy_envelope (Engine& E, double* out_host);
int laser_chi_initial (Engine& E);                                           // SetInitialChi, once per step (laser grid only)
int laser_copy_chi (Engine& E, double* out_host);
void laser_sizes (Engine& E, int* nx, int* ny, int* nz);
long laser_mg_vcycles (Engine& E);
int laser_set_import (Engine& E, int on, int step);
int laser_export_slice (Engine& E, int islice, double* msg_dev);
int laser_import_slice (Engine& E, int islice, const double* msg_dev);
int laser_import_from (Engine& E, int islice, Engine& src);
int laser_check_samples (Engine& E, const Engine::LaserSamples& S);          // what hps_engine_add_laser_samples refuses
int laser_set_insitu (Engine& E, int on);                                    // the [8][nzl] in-situ buffer and its scratch
int laser_clear_insitu (Engine& E);
int laser_copy_insitu (Engine& E, double* out_host);
// expr.hip: hps_expr_check in the words of fn; "is absent" (no instructions, or the single constant 0); packing: ExprImage
int expr_check_named (const char* fn, const char* what, const hps_expr* p, int n_vars, int* depth);
bool expr_is_zero (const hps_expr& p);
int beam_blocks_to_soa (Engine& E, const double* blocks, double* soa, long nb);      // beam_init.hip: slice-major blocks -> global SoA (beam_off)
int beam_deposit_moving (Engine& E, int p, int cjx, int cjy, int cjz);      // beam.hip
int beam_deposit_species (Engine& E, int p, unsigned mask, int cjx, int cjy, int cjz);      // ... of the species in mask (SALAME's step 0)
int salame_scale_moving (Engine& E, int p, unsigned mask, double W);        // SalameMultiplyBeamWeight on slice p of the container
int beam_push_moving (Engine& E, int islice);
int beam_push_slice (Engine& E, int islice, int p, long bound);
int beam_moments_reset (Engine& E);
int beam_species_table_upload (Engine& E);                                  // the per-species constants of the step that has begun
std::string beam_kernel_names (const Engine& E);                            // the beam kernel instances launched so far, one per line
int beam_export_slice (Engine& E, int islice, double* msg_dev, long cap);
int beam_import_slice (Engine& E, int islice, const double* msg_dev, long cap);
int salame_get_w_enqueue (const hps_slab& slab, int cT, int cN, int cE, int cJ, double* scratch, hipStream_t st);      // salame.hip
const double* salame_get_w_result (const double* scratch);

} // namespace hps
#endif
