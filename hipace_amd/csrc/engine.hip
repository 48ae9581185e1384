// engine.hip -- the slice engine's core: the slab bookkeeping kernels, the plasma sheets (allocation, InitParticles, tile
// sort), Engine::create / begin_step, the three particle operators over a species, and the per-slice schedule of the explicit
// solver -- solve_slice_begin / solve_slice_finish, the device-resident equivalent of Hipace::Evolve / Hipace::SolveOneSlice
// (Hipace.cpp:393-728) -- with the core of the C ABI.  What the schedule calls lives with its subject: the predictor-corrector
// solver in predcorr.hip, the open boundary in open_boundary.hip, the diagnostics in diagnostics.hip, the static and
// host-initialised beam in beam_host.hip, SALAME in salame.hip, the laser in laser.hip, the stream pool in stream_pool.hip.
#include "common.h"
#include "engine.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <algorithm>
#include <new>

namespace hps {

static thread_local std::string g_err;
void set_error (const std::string& msg) { g_err = msg; }

// ------------------------------------------------------------------------------------------
// slab kernels (all over whole planes incl. guards unless noted; x fastest, fully coalesced)
// ------------------------------------------------------------------------------------------

// zero the components of `full` everywhere and those of `boxed` inside the box
__global__ __launch_bounds__(256)
void k_zero_comps (double* p, long ns, long plane, int js, CompList full, CompList boxed, CellBox bb, CompList from_ion = CompList{0, {}}, int c_ion = -1)
{
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= plane) return;
    for (int k = 0; k < full.n; ++k) p[full.c[k]*ns + s] = 0.0;
    // AddRhoIons (fields/Fields.cpp:606-615) ahead of the deposition instead of behind it: the charge planes start from the
    // neutralising background and the plasma is added on top (one pass over them less per slice)
    if (c_ion >= 0) { const double ion = p[c_ion*ns + s]; for (int k = 0; k < from_ion.n; ++k) p[from_ion.c[k]*ns + s] = ion; }
    const int j = (int)(s / js), i = (int)(s - (long)j*js);
    if (i >= bb.ilo && i <= bb.ihi && j >= bb.jlo && j <= bb.jhi)
        for (int k = 0; k < boxed.n; ++k) p[boxed.c[k]*ns + s] = 0.0;
}

__global__ __launch_bounds__(256)
void k_copy_comps (double* p, long ns, long plane, CompList dst, CompList src)
{
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= plane) return;
    double v[12];
    for (int k = 0; k < src.n; ++k) v[k] = p[src.c[k]*ns + s];
    for (int k = 0; k < dst.n; ++k) p[dst.c[k]*ns + s] = v[k];
}

// ShiftSlices (fields/Fields.cpp:588-604): Previous <- This <- Next for the beam currents, jx, jy <- Next.
// The beam planes are zero outside the box: there only jx = jy = 0 is written.
__global__ __launch_bounds__(256)
void k_shift_slices (double* p, long ns, long plane, int js, CellBox bb, int c_njxb, int c_njyb)
{
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= plane) return;
    const int j = (int)(s / js), i = (int)(s - (long)j*js);
    double njx = 0.0, njy = 0.0;
    if (i >= bb.ilo && i <= bb.ihi && j >= bb.jlo && j <= bb.jhi) {
        const double tjx = p[HPS_C_JXB*ns + s], tjy = p[HPS_C_JYB*ns + s];
        njx = p[c_njxb*ns + s]; njy = p[c_njyb*ns + s];
        p[HPS_C_P_JXB*ns + s] = tjx; p[HPS_C_P_JYB*ns + s] = tjy;
        p[HPS_C_JXB*ns + s] = njx;   p[HPS_C_JYB*ns + s] = njy;
    }
    p[HPS_C_JX*ns + s] = njx; p[HPS_C_JY*ns + s] = njy;
}

// ShiftSlices (fields/Fields.cpp:588-604) of this slice AND InitializeSlices (:535-586) of the next one in one pass: what
// the fused push + deposition (k_advance_deposit_tiled) needs done before it deposits into the next slice's jx jy chi
// rhomjz [rho].  Inside the beam's box also jz_beam and the Next beam currents are cleared.  (shift_init_cell, slab_ops.h: the
// same pass rides in the multigrid's lower V where the slice allows it, HPS_EARLY_INIT)
__global__ __launch_bounds__(256)
void k_shift_zero (ShiftInit a)
{
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (s >= a.plane) return;
    shift_init_cell(a, s);
}

// AddRhoIons (fields/Fields.cpp:606-615) fused with the Psi source  -rhomjz/ep0  (:887-888)
__global__ __launch_bounds__(256)
void k_add_ions_psi_rhs (SlabView f, int c_rhomjz, int c_ion, int c_rho, double inv_ep0, double* staging)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x - f.ng;
    const int j = blockIdx.y - f.ng;
    if (i >= f.nx + f.ng) return;
    const long o = f.off(i, j);
    const double ion = f.p[c_ion*f.ns + o];
    const double r = f.p[c_rhomjz*f.ns + o] + ion;
    f.p[c_rhomjz*f.ns + o] = r;
    if (c_rho >= 0) f.p[c_rho*f.ns + o] += ion;
    if (i >= 0 && i < f.nx && j >= 0 && j < f.ny) staging[(long)j*f.nx + i] = -inv_ep0*r;
}

// AddRhoIons + the three Poisson sources of a slice in one pass (fields/Fields.cpp:606-615,
// 887-912): st[0] = -rhomjz/ep0 (Psi), st[1] = (d_x jx + d_y jy)/(ep0 c) (Ez),
// st[2] = mu0 (d_y jx - d_x jy) (Bz); `plane` = nx*ny
__global__ __launch_bounds__(256)
void k_rhs_all (SlabView f, int c_rhomjz, int c_ion, int c_rho, int c_jx, int c_jy, double inv_ep0,
                double fez_x, double fez_y, double fbz_y, double fbz_x, double* staging, long plane)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x - f.ng;
    const int j = blockIdx.y - f.ng;
    if (i >= f.nx + f.ng) return;
    const long o = f.off(i, j);
    double r;
    if (c_ion >= 0) {
        const double ion = f.p[c_ion*f.ns + o];
        r = f.p[c_rhomjz*f.ns + o] + ion;
        f.p[c_rhomjz*f.ns + o] = r;
        if (c_rho >= 0) f.p[c_rho*f.ns + o] += ion;
    } else {      // the background is in already (k_zero_comps / k_shift_zero): valid cells only
        if (!(i >= 0 && i < f.nx && j >= 0 && j < f.ny)) return;
        r = f.p[c_rhomjz*f.ns + o];
    }
    if (i >= 0 && i < f.nx && j >= 0 && j < f.ny) {
        const long so = (long)j*f.nx + i;
        const double* X = f.p + c_jx*f.ns + o;
        const double* Y = f.p + c_jy*f.ns + o;
        staging[so] = -inv_ep0*r;
        staging[plane + so] = fez_x*(X[1] - X[-1]) + fez_y*(Y[f.js] - Y[-f.js]);
        staging[2*plane + so] = fbz_y*(X[f.js] - X[-f.js]) + fbz_x*(Y[1] - Y[-1]);
    }
}

// GridCurrent::DepositCurrentSlice (utils/GridCurrent.cpp:25-71): valid cells; amp = peak * exp(-dz^2/2) of the slice
__global__ __launch_bounds__(256)
void k_grid_current (SlabView f, int cjz, double xlo, double ylo, double dx, double dy, double mx, double my, double sx, double sy,
                     double amp)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= f.nx) return;
    const double delta_x = (xlo + (i + 0.5)*dx - mx) / sx;
    const double delta_y = (ylo + (j + 0.5)*dy - my) / sy;
    f(i, j, cjz) += amp*exp(-0.5*(delta_x*delta_x + delta_y*delta_y));
}

// ExmBy = -dPsi/dx, EypBx = -dPsi/dy on the box grown by (guards-1) (fields/Fields.cpp:931-956)
__global__ __launch_bounds__(256)
void k_grad_psi (SlabView f, int cPsi, int cExmBy, int cEypBx, double hdx_inv, double hdy_inv)
{
    const int gg = f.ng - 1;
    const int i = blockIdx.x*blockDim.x + threadIdx.x - gg;
    const int j = blockIdx.y - gg;
    if (i >= f.nx + gg) return;
    const long o = f.off(i, j);
    const double* P = f.p + cPsi*f.ns + o;
    f.p[cExmBy*f.ns + o] = -(P[1] - P[-1])*hdx_inv;
    f.p[cEypBx*f.ns + o] = -(P[f.js] - P[-f.js])*hdy_inv;
}

// beam contribution to the Bx/By sources (Hipace::InitializeSxSyWithBeam, Hipace.cpp:744-790)
__global__ __launch_bounds__(256)
void k_sxsy_beam (SlabView f, int cSx, int cSy, int cJzb, int cNx, int cNy, int cPx, int cPy,
                  double mu0, double dx2, double dy2, double dz2, CellBox bb, int cBackX, int cBackY)      // (defaults -1: slab_ops.h)
{
    // cBackX, cBackY >= 0 (SALAME, Salame.cpp:175-179): the backed-up result of the explicit deposition is added on top
    // whole plane: the guard cells are set to 0 here (they are not part of InitializeSlices' zero list any more)
    const int i = blockIdx.x*blockDim.x + threadIdx.x - f.ng;
    const int j = blockIdx.y - f.ng;
    if (i >= f.nx + f.ng) return;
    const long o = f.off(i, j);
    // no beam current within reach (bb is in padded-array cells): the sources are 0 without a load
    const int ia = i + f.ng, ja = j + f.ng;
    if (i < 0 || i >= f.nx || j < 0 || j >= f.ny || ia < bb.ilo || ia > bb.ihi || ja < bb.jlo || ja > bb.jhi) {
        f.p[cSy*f.ns + o] = cBackY >= 0 ? f.p[cBackY*f.ns + o] : 0.0; f.p[cSx*f.ns + o] = cBackX >= 0 ? f.p[cBackX*f.ns + o] : 0.0; return;
    }
    const double* J = f.p + cJzb*f.ns + o;
    const double dx_jzb = (J[1] - J[-1])/dx2;
    const double dy_jzb = (J[f.js] - J[-f.js])/dy2;
    const double dz_jxb = (f.p[cPx*f.ns + o] - f.p[cNx*f.ns + o])/dz2;
    const double dz_jyb = (f.p[cPy*f.ns + o] - f.p[cNy*f.ns + o])/dz2;
    const double sy =  mu0*(-dy_jzb + dz_jyb), sx = -mu0*(-dx_jzb + dz_jxb);
    f.p[cSy*f.ns + o] = cBackY >= 0 ? sy + f.p[cBackY*f.ns + o] : sy;
    f.p[cSx*f.ns + o] = cBackX >= 0 ? sx + f.p[cBackX*f.ns + o] : sx;
}

// -grad Psi (k_grad_psi) and the beam part of Sx, Sy (k_sxsy_beam) in one pass over the plane: one launch less per slice
__global__ __launch_bounds__(256)
void k_gradpsi_sxsy (SlabView f, GradPsiSxSy a)
{
    gradpsi_sxsy_cell(f, a, (int)(blockIdx.x*blockDim.x + threadIdx.x) - f.ng, (int)blockIdx.y - f.ng);
}

// weight = density(x, y, c t) * scale_fac (PlasmaParticleContainerInit.cpp:246-313) with the tabulated profile
// density * f_r(r) * f_t: prof = [r[nr] | f_r[nr]] on the device, ft the time factor of this step; a lattice point
// whose density is <= 0 holds no particle (the reference does not create it: here its slot is invalid)
// plasma sheet on the fixed-ppc lattice, ppc index outermost so that consecutive lanes own
// consecutive cells (PlasmaParticleContainerInit.cpp:192-313, ParticleUtil.H:72-83)
__global__ __launch_bounds__(256)
void k_init_plasma (hps_plasma pl, long n, int nx, int ny, int ppcx, int ppcy, double lox, double loy, double dx, double dy,
                    double weight, int level, int keyed, const double* __restrict__ prof, int nr, double ft, double radius_sq)
{
    const long k = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (k >= n) return;
    const long cells = (long)nx*ny;
    const int ip = (int)(k / cells);
    const long c = k - (long)ip*cells;
    const int j = (int)(c / nx), i = (int)(c - (long)j*nx);
    const int ixp = ip % ppcx, iyp = ip / ppcx;
    const double x = lox + (i + (0.5 + ixp)/ppcx)*dx;
    const double y = loy + (j + (0.5 + iyp)/ppcy)*dy;
    // <plasma>.radius: no particle beyond it (PlasmaParticleContainerInit.cpp:262-266)
    const double fac = (x*x + y*y > radius_sq) ? 0.0 : ft*table_value(prof, prof + nr, nr, sqrt(x*x + y*y));
    pl.x[k] = x; pl.y[k] = y; pl.w[k] = fac > 0.0 ? weight*fac : 0.0;
    pl.ux[k] = 0.0; pl.uy[k] = 0.0; pl.psi[k] = 1.0;
    pl.x_prev[k] = x; pl.y_prev[k] = y;
    pl.ux_half[k] = 0.0; pl.uy_half[k] = 0.0; pl.psi_half[k] = fac > 0.0 ? 1.0 : 0.0;      // (0: not a particle, Tiling::valid_by_psi)
    // id = 1, cpu (level) = 0.  A species that can ionise carries its lattice index + 1 in the id bits: the key of its
    // random draws (ionization.hip); the reference only ever reads the sign of the id
    pl.idcpu[k] = (fac > 0.0 ? HPS_ID_VALID : 0ULL) | ((keyed ? (unsigned long long)(k + 1) : 1ULL) << 24);
    pl.ion_lev[k] = level;
}

// k_zero_comps / k_copy_comps over the whole padded planes (slab_ops.h: the predictor-corrector and SALAME schedules call them too)
void zero_comps (const hps_slab& slab, hipStream_t st, CompList full, CompList boxed, CellBox bb, CompList from_ion, int c_ion)
{
    hipLaunchKernelGGL(k_zero_comps, dim3(ceil_div(slab.nstride, 256)), dim3(256), 0, st, slab.p, slab.nstride, slab.nstride, (int)slab.jstride,
                       full, boxed, bb, from_ion, c_ion);
}
void copy_comps (const hps_slab& slab, hipStream_t st, CompList dst, CompList src)
{
    hipLaunchKernelGGL(k_copy_comps, dim3(ceil_div(slab.nstride, 256)), dim3(256), 0, st, slab.p, slab.nstride, slab.nstride, dst, src);
}

// ------------------------------------------------------------------------------------------
// Engine
// ------------------------------------------------------------------------------------------
Engine::~Engine ()
{
    if (ps) hps_poisson_destroy(ps);
    if (mg) hps_mg_destroy(mg);
    (void)hipFree(slab.p); free_soa(el.pl, el.real); free_soa(el.pl_alt, el.real_alt);      // (the ions' sheets: ion_destroy)
    delete el.tiling;
    for (int k = 2; k < n_sp; ++k) { free_soa(sp[k].pl, sp[k].real); free_soa(sp[k].pl_alt, sp[k].real_alt); delete sp[k].tiling; }
    (void)hipFree(d_insitu_pl_more);
    (void)hipFree(staging); (void)hipFree(d_open_mom); (void)hipFree(beam_data); (void)hipFree(beam_init);
    (void)hipFree(bm_store); (void)hipFree(bm_nsub); (void)hipFree(bm_nsub_scr); (void)hipFree(d_B); (void)hipFree(d_nfront);
    (void)hipFree(d_mom); (void)hipFree(d_sal); (void)hipFree(bm_sp); (void)hipFree(bm_sp_scr); (void)hipFree(beam_tag); (void)hipFree(d_bsp_tab);
    (void)hipFree(d_Bimp); (void)hipFree(d_beam_overflow); (void)hipFree(d_nqsa); (void)hipFree(d_checksum);
    (void)hipFree(d_pc); (void)hipFree(d_pc_aux); (void)hipFree(d_pc_go); if (h_pc) (void)hipHostFree(h_pc);
    (void)hipFree(d_laser_sum);
    if (laser) laser_destroy(*this);
    ion_destroy(*this);
    (void)hipFree(d_prof_r); (void)hipFree(d_fine_level); (void)hipFree(d_fine_cells);
    (void)hipFree(d_fd); (void)hipFree(d_fd_comps); (void)hipFree(d_insitu); (void)hipFree(d_insitu_pl); (void)hipFree(d_insitu_bm);
    for (auto e : ev) (void)hipEventDestroy(e);
    for (auto e : hand_ev) if (e) (void)hipEventDestroy(e);
    if (st_aux) (void)hipStreamDestroy(st_aux);
    for (hipEvent_t ev : ev_aux) if (ev) (void)hipEventDestroy(ev);
    if (st_laser) (void)hipStreamDestroy(st_laser);
    if (ev_lfork) (void)hipEventDestroy(ev_lfork);
    if (ev_ldone) (void)hipEventDestroy(ev_ldone);
    if (st && st_pooled) return_engine_stream(st, st_device);
    else if (st) (void)hipStreamDestroy(st);
}

// Slots of a species' sheet: ppc per cell, and fine_ppc in the cells of the fine patch and its transition
long Engine::sheet_slots (const Species& s) const
{
    if (!s.present()) return 0;
    const long cells = (long)d.nx*d.ny, nc = (long)s.ppc[0]*s.ppc[1];
    const long copies = do_symmetrize ? 4 : 1;       // do_symmetrize: the sheet and its three mirror copies
    if (!(fine_patch_set && s.fine_ppc[0] > 0)) return copies*nc*cells;
    return copies*(nc*cells + ((long)s.fine_ppc[0]*s.fine_ppc[1] - nc)*fine_ncells);
}

std::array<double**, 11> soa_arrays (hps_plasma& p)
{
    return {&p.x, &p.y, &p.w, &p.ux, &p.uy, &p.psi, &p.x_prev, &p.y_prev, &p.ux_half, &p.uy_half, &p.psi_half};
}
int alloc_soa (hps_plasma& p, double*& real, long cap, bool alias)
{
    HPS_HIP_CHECK(hipMalloc(&real, (size_t)cap*11*sizeof(double)));
    const auto arr = soa_arrays(p);
    for (int k = 0; k < 11; ++k) *arr[k] = real + (size_t)k*cap;
    if (alias) { p.x_prev = p.x; p.y_prev = p.y; }
    HPS_HIP_CHECK(hipMalloc(&p.idcpu, (size_t)cap*sizeof(uint64_t)));
    HPS_HIP_CHECK(hipMalloc(&p.ion_lev, (size_t)cap*sizeof(int32_t)));
    return HPS_OK;
}
void free_soa (hps_plasma& p, double*& real)
{
    (void)hipFree(real); (void)hipFree(p.idcpu); (void)hipFree(p.ion_lev);
    real = nullptr; p = hps_plasma{};
}
static hps_plasma tail_of (const hps_plasma& p, long first, long n)
{
    hps_plasma t = p;
    for (double** a : soa_arrays(t)) *a += first;      // (x_prev / y_prev stay aliased to x / y where they were)
    t.idcpu += first; t.ion_lev += first; t.n = n;
    return t;
}

// The sheets of every species, sized by what InitParticles creates; hps_engine_set_plasma_init / hps_engine_set_fine_patch
// call it again (before the first step: nothing else holds a pointer into them yet)
int Engine::alloc_sheets ()
{
    for (Species& s : sp) { free_soa(s.pl, s.real); s.n_init = s.cap = sheet_slots(s); }
    // every ion can release Z - initial level electrons into the first species
    if (ions.present()) el.cap = el.n_init + ions.n_init*(long)(d.ion_Z - d.ion_init_level);
    for (Species& s : sp) {
        s.pl.n = s.n_init;
        if (s.cap > 0) { if (int e = alloc_soa(s.pl, s.real, s.cap, s.alias_prev())) return e; }
    }
    return HPS_OK;
}

int Engine::create (const hps_deck& deck, int device)
{
    d = deck;
    HPS_REQUIRE(d.nx >= 4 && d.ny >= 4 && d.nz >= 1, "hps_engine_create: bad grid");
    HPS_REQUIRE(d.order >= 0 && d.order <= 3, "hps_engine_create: depos_order must be 0..3");
    HPS_REQUIRE(d.n_subcycles >= 0, "hps_engine_create: plasma n_subcycles must be >= 1 (0 = default 1)");
    if (d.n_subcycles == 0) d.n_subcycles = 1;       // <plasma>.n_subcycles default (particles/plasma/PlasmaParticleContainer.H:182)
    if (d.field_bc != 0 && d.field_bc != 1) { set_error("hps_engine_create: boundary.field must be 0 (Dirichlet) or 1 (Open)"); return HPS_ERR_UNSUPPORTED; }
    if (d.field_bc == 1) {
        // (the expansion is about x = y = 0, which must lie inside the box: fields/Fields.cpp:703-705)
        const double radius = std::min(std::min(std::fabs(d.lo[0]), std::fabs(d.hi[0])), std::min(std::fabs(d.lo[1]), std::fabs(d.hi[1])));
        HPS_REQUIRE(radius > 0.0 && d.lo[0] < 0.0 && d.hi[0] > 0.0 && d.lo[1] < 0.0 && d.hi[1] > 0.0, "hps_engine_create: boundary.field = Open needs x = y = 0 inside the box");
        HPS_HIP_CHECK(hipMalloc(&d_open_mom, (size_t)4*256*2*19*sizeof(double)));      // [source][OPEN_PARTS][2 (OPEN_ORDER + 1)]
    }
    pc = (d.bxby_solver != 0);
    if (const char* v = std::getenv("HPS_GATED_PUSH")) gate_push = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_AUX_STREAM")) aux_on = std::atoi(v) != 0;
    if (aux_on) {
        HPS_HIP_CHECK(hipStreamCreateWithFlags(&st_aux, hipStreamNonBlocking));
        for (hipEvent_t& ev : ev_aux) HPS_HIP_CHECK(hipEventCreateWithFlags(&ev, event_flags(false)));
    }
    if (const char* v = std::getenv("HPS_FOLD_TAIL")) fold_tail = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_POST_IN_PUSH")) post_in_push = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_FOLD_BEAM")) fold_beam = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_FOLD_HIERARCHY")) fold_hierarchy = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_VALID_BY_W")) valid_by_w = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_VALID_BY_PSI")) valid_by_psi = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_GATED_ION_PUSH")) gate_ion_push = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_LAZY_SHIFT")) lazy_shift = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_FUSE_SOURCES")) fuse_sources = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_EARLY_INIT")) early_init = std::atoi(v) != 0;
    if (const char* v = std::getenv("HPS_SORT_FALLBACK_DIV")) { const long q = std::atol(v); if (q >= 1) fallback_div = q; }
    HPS_REQUIRE(!(d.beam_spin_tracking && d.dt == 0.0 && !d.dt_adaptive), "hps_engine_create: spin tracking needs a moving beam (hipace.dt != 0)");
    HPS_REQUIRE(!(d.dt_adaptive && d.laser_on), "hps_engine_create: hipace.dt = adaptive cannot be used with a laser (Hipace.cpp:408)");
    if (d.beam_do_salame) {
        // <beam>.do_salame
        if (pc) { set_error("hps_engine_create: beam_do_salame needs the explicit solver (Hipace.cpp:152), not the predictor-corrector"); return HPS_ERR_UNSUPPORTED; }
        if (d.beam_profile == 0 && !(std::isfinite(d.beam_zmin) && std::isfinite(d.beam_zmax))) {
            set_error("hps_engine_create: beam_do_salame with a gaussian beam profile needs finite beam_zmin and beam_zmax (BeamParticleContainer.cpp:149)"); return HPS_ERR_ARG; }
        if (d.ion_on) { set_error("hps_engine_create: beam_do_salame with the ionisable species (ion_on) is not supported"); return HPS_ERR_UNSUPPORTED; }
        if (d.laser_on) { set_error("hps_engine_create: beam_do_salame with a laser is not supported"); return HPS_ERR_UNSUPPORTED; }
        if (d.dt != 0.0 || d.dt_adaptive) {
            set_error("hps_engine_create: beam_do_salame needs a static beam (hipace.dt = 0): the SALAME beam of a moving-beam engine is an added "
                      "species (hps_engine_set_beam_species_salame: beam_species_salame, do_salame)"); return HPS_ERR_UNSUPPORTED; }
        HPS_REQUIRE(d.salame_n_iter >= 0 && d.salame_relative_tolerance >= 0.0, "hps_engine_create: salame_n_iter and salame_relative_tolerance must not be negative");
        if (d.salame_n_iter == 0) d.salame_n_iter = 5;                                    // hipace.salame_n_iter (Hipace.H)
        if (d.salame_relative_tolerance == 0.0) d.salame_relative_tolerance = 1.0e-4;      // hipace.salame_relative_tolerance
    }
    step_dt = d.dt;
    if (d.predcorr_tol > 0.0) pc_tol = d.predcorr_tol;
    if (d.predcorr_max_iter > 0) pc_max_iter = d.predcorr_max_iter;
    if (d.predcorr_mix > 0.0) pc_mix = d.predcorr_mix;
    HPS_HIP_CHECK(hipSetDevice(device));
    HPS_HIP_CHECK(create_engine_stream(&st, device, &st_pooled));
    st_device = device;
    if (const char* v = std::getenv("HPS_LASER_ASYNC")) laser_async = std::atoi(v) != 0;
    if (laser_async && d.laser_on && d.laser_solver >= 1 && d.dt != 0.0) {
        // below the engine's stream: its kernels fill what the slice leaves idle, they are not to win a CU from it
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HPS_HIP_CHECK(hipStreamCreateWithPriority(&st_laser, hipStreamNonBlocking, lo));
        HPS_HIP_CHECK(hipEventCreateWithFlags(&ev_lfork, event_flags(false)));
        HPS_HIP_CHECK(hipEventCreateWithFlags(&ev_ldone, event_flags(false)));
    }
    g = (d.order + 1)/2 + 1;                       // Fields::AllocData (fields/Fields.cpp:63-64)
    ncomp = pc ? (d.deposit_rho ? HPS_PC_RHO + 1 : HPS_PC_RHO) : (d.deposit_rho ? HPS_C_RHO + 1 : HPS_C_RHO);
    if (d.beam_radiation_reaction && !d.si_units && !(d.background_density_SI > 0.0)) {      // BeamParticleAdvance.cpp:39-43
        set_error("hps_engine_create: radiation reaction in normalised units needs background_density_SI"); return HPS_ERR_ARG; }
    if (d.laser_on) {
        if (pc) { set_error("hps_engine_create: the laser needs the explicit solver"); return HPS_ERR_UNSUPPORTED; }
        HPS_REQUIRE(d.laser_w0 > 0.0 && d.laser_L0 > 0.0 && d.laser_lambda0 > 0.0, "hps_engine_create: laser w0, L0, lambda0 must be positive");
        if (d.laser_solver < 0 || d.laser_solver > 2) { set_error("hps_engine_create: lasers.solver_type must be 0 (static), 1 (fft) or 2 (multigrid)"); return HPS_ERR_UNSUPPORTED; }
        c_aabs = ncomp++;                // appended last
    }
    gm.dx = (d.hi[0] - d.lo[0])/d.nx; gm.dy = (d.hi[1] - d.lo[1])/d.ny; gm.dz = (d.hi[2] - d.lo[2])/d.nz;
    gm.xoff = 0.5*(d.lo[0] + d.hi[0] - gm.dx*(d.nx - 1));
    gm.yoff = 0.5*(d.lo[1] + d.hi[1] - gm.dy*(d.ny - 1));
    gm.c = gm.ep0 = gm.mu0 = gm.q_e = gm.m_e = 1.0;
    if (d.si_units) {       // make_constants_SI (utils/Constants.H:15-24, 2018 CODATA)
        gm.c = 299792458.0; gm.ep0 = 8.8541878128e-12; gm.mu0 = 1.25663706212e-06; gm.q_e = 1.602176634e-19; gm.m_e = 9.1093837015e-31;
    }
    gm.plo[0] = d.lo[0]; gm.plo[1] = d.lo[1]; gm.phi[0] = d.hi[0]; gm.phi[1] = d.hi[1];
    gm.bc = d.bc; gm.normalized = d.si_units ? 0 : 1;

    // the SALAME slice: twelve planes behind the engine's own (`ncomp` stays the count of those: checksums, hps_engine_info)
    if (d.beam_do_salame) {
        c_sal = ncomp;
        HPS_HIP_CHECK(hipMalloc(&d_sal, (size_t)4*257*sizeof(double)));
        sal_stats.assign((size_t)4*d.nz, 0.0);
    }
    slab.nx = d.nx; slab.ny = d.ny; slab.ng = g; slab.ncomp = ncomp + (c_sal >= 0 ? (int)HPS_SAL_NCOMP : 0);
    // the alternates of the re-initialised planes (HPS_EARLY_INIT), behind everything else; only decks whose slices can take the
    // plain path have them (the multigrid's lower V is known further down: a grid it does not suit keeps them unused)
    set_canon = set_alt = InitSet{HPS_C_CHI, HPS_C_RHOMJZ, d.deposit_rho ? (int)HPS_C_RHO : -1, HPS_C_JZB, HPS_C_N_JXB, HPS_C_N_JYB};
    if (early_init && !pc && !d.laser_on && !d.ion_on && d.dt == 0.0 && !d.dt_adaptive && d.nx % 2 == 0 && d.ny % 2 == 0) {
        int c = slab.ncomp;
        set_alt.chi = c++; set_alt.rhomjz = c++; if (d.deposit_rho) set_alt.rho = c++;
        set_alt.jzb = c++; set_alt.njxb = c++; set_alt.njyb = c++;
        n_alt = c - slab.ncomp; slab.ncomp = c;
    }
    slab.jstride = d.nx + 2*g; slab.nstride = slab.jstride*(d.ny + 2*g);
    HPS_HIP_CHECK(hipMalloc(&slab.p, (size_t)slab.nstride*slab.ncomp*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(slab.p, 0, (size_t)slab.nstride*slab.ncomp*sizeof(double)));
    HPS_HIP_CHECK(hipMalloc(&staging, (size_t)3*d.nx*d.ny*sizeof(double)));

    if (d.ion_on) {
        // (predictor-corrector: every species is pushed to the temporary slice and deposited in turn inside the loop; the ADK
        //  decisions are taken once per slice, ahead of the committing push, as Hipace.cpp:693-701 has them)
        HPS_REQUIRE(d.ion_ppc[0] >= 1 && d.ion_ppc[1] >= 1 && d.ion_density > 0.0 && d.ion_mass > 0.0 && d.ion_charge != 0.0,
                    "hps_engine_create: the ion species needs ppc, density, mass and charge");
        if (int e = ion_create(*this)) return e;
    }
    // the species' records: the one place that reads the deck's plasma_* / ion_* spellings.  An absent species keeps density 0
    // (the plasma's charge and mass also hold for the electrons the species "ion" releases into a deck without plasma)
    for (int k = 0; k < 2; ++k) { sp[k].index = k; sp[k].can_ionize = k; sp[k].keyed = k; sp[k].temp_push = pc || (k == 0 && c_sal >= 0); }
    el.grows_tail = el.by_weight = true; el.neutralize = !d.plasma_no_neutralize;      // (the ions' tile_flag: setup_tiling)
    std::copy(d.plasma_ppc, d.plasma_ppc + 2, el.ppc); el.density = d.plasma_density; el.charge = d.plasma_charge; el.mass = d.plasma_mass;
    if (d.ion_on) { std::copy(d.ion_ppc, d.ion_ppc + 2, ions.ppc); ions.density = d.ion_density; ions.charge = d.ion_charge; ions.mass = d.ion_mass; ions.init_level = d.ion_init_level; }
    if (int e = alloc_sheets()) return e;
    HPS_HIP_CHECK(hipMalloc(&d_laser_sum, sizeof(double)));
    HPS_HIP_CHECK(hipMemset(d_laser_sum, 0, sizeof(double)));
    HPS_HIP_CHECK(hipMalloc(&d_nqsa, sizeof(int)));
    HPS_HIP_CHECK(hipMemset(d_nqsa, 0, sizeof(int)));
    HPS_HIP_CHECK(hipMalloc(&d_checksum, HPS_PC_NCOMP_MAX*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(d_checksum, 0, HPS_PC_NCOMP_MAX*sizeof(double)));
    if (int e = hps_poisson_create(d.nx, d.ny, gm.dx, gm.dy, &ps)) return e;
    if (int e = hps_mg_create(d.nx, d.ny, gm.dx, gm.dy, &mg)) return e;
    // the halo-fallback counter lives in the header slot of the multigrid's norm buffer: it reaches the host
    // with the read-back every solve does anyway (no copy of its own)
    {   int* dw = nullptr; const int* hw = nullptr;
        mg_rider(mg, &dw, &hw);
        d_nfallback = dw; h_nfallback = hw; }
    if (pc) { if (int e = pc_create()) return e; }
    if (c_aabs >= 0) { if (int e = laser_create(*this)) return e; }
    return init_beam();
}

// hps_engine_add_plasma_species: every check first, then the record and its sheet; nothing else of the engine changes
int Engine::add_plasma_species (const hps_plasma_species* s, int* index_out)
{
    static const std::string fn = "hps_engine_add_plasma_species: ";
    HPS_REQUIRE(s && index_out, fn + "null argument");
    HPS_REQUIRE(!step_begun && !el.tiling, fn + "call before the first hps_engine_begin_step");
    if (d.beam_do_salame || species_salame) {
        set_error(fn + "an engine with beam_do_salame or beam_species_salame is not supported: SALAME drives the electrons alone (as with ion_on)");
        return HPS_ERR_UNSUPPORTED;
    }
    HPS_REQUIRE(n_sp < HPS_MAX_PLASMA_SPECIES, fn + "at most HPS_MAX_PLASMA_SPECIES plasma species (the deck's two included)");
    HPS_REQUIRE(s->ppc[0] >= 1 && s->ppc[1] >= 1, fn + "ppc must be >= 1 in both directions");
    HPS_REQUIRE(std::isfinite(s->density) && s->density > 0.0, fn + "density must be positive");
    HPS_REQUIRE(std::isfinite(s->mass) && s->mass > 0.0, fn + "mass must be positive");
    HPS_REQUIRE(std::isfinite(s->charge) && s->charge != 0.0, fn + "charge must not be 0");
    const bool fine = s->fine_ppc[0] != 0 || s->fine_ppc[1] != 0;
    HPS_REQUIRE(!fine || (s->fine_ppc[0] > 0 && s->fine_ppc[1] > 0 && s->fine_ppc[0] % s->ppc[0] == 0 && s->fine_ppc[1] % s->ppc[1] == 0),
                fn + "fine_ppc must be {0, 0} or positive and divisible by ppc, component by component");
    HPS_REQUIRE(!(fine && prevent_centered), fn + "prevent_centered_particle cannot be combined with the fine plasma patch (fine_ppc, fine_patch)");
    Species& q = sp[n_sp];
    q = Species{};
    q.index = n_sp; q.can_ionize = 0; q.keyed = 0; q.init_level = 0; q.temp_push = pc;      // (no tail, no tile flags, not by weight)
    std::copy(s->ppc, s->ppc + 2, q.ppc); std::copy(s->fine_ppc, s->fine_ppc + 2, q.fine_ppc);
    q.density = s->density; q.charge = s->charge; q.mass = s->mass; q.neutralize = s->neutralize_background != 0;
    q.n_init = q.cap = sheet_slots(q); q.pl.n = q.n_init;
    if (int e = alloc_soa(q.pl, q.real, q.cap, q.alias_prev())) { free_soa(q.pl, q.real); q = Species{}; return e; }
    *index_out = n_sp++;
    return HPS_OK;
}

int Engine::setup_tiling ()
{
    if (tile_size == 0 || el.cap == 0 || el.tiling) return HPS_OK;
    for (int k = 0; k < n_sp; ++k) {
        Species& s = sp[k];
        if (s.cap == 0) continue;
        // every species on the engine's tile size, the ionisable one too.  (Round 2 gave a species with at most one particle per
        // cell 32 x 32-cell tiles -- 256 particles in a 16 x 16 tile, one per thread, against the tile's fixed cost.  With the tile
        // skip most of its tiles cost nothing, and its kernels last as long as the few workgroups around the laser's axis that do
        // have charged ions: four times as many of them, a quarter as long -- config 5 989 -> 1004 slices/s.  HPS_ION_TILE=32)
        int ts = tile_size;
        if (const char* v = s.can_ionize ? std::getenv("HPS_ION_TILE") : nullptr) { const int t = std::atoi(v); if (t == 16 || t == 32) ts = t; }
        if (int e = tiling_create(d.nx, d.ny, ts, s.cap, &s.tiling)) return e;
        if (int e = alloc_soa(s.pl_alt, s.real_alt, s.cap, s.alias_prev())) return e;      // (its n: sort_sheet)
    }
    // the electrons' push without its idcpu read (tiling.h): every path that creates or invalidates an electron keeps
    // "valid <=> psi_half != 0" (DESIGN section 6 "Round 10"); every other species' push keeps reading idcpu
    el.tiling->valid_by_psi = valid_by_psi;
    if (ions.tiling) {
        HPS_HIP_CHECK(hipMalloc(&ion.d_tile_flag, (size_t)ions.tiling->g.ntiles*sizeof(int)));
        ions.tile_flag = ion.d_tile_flag;
        {   const char* v = std::getenv("HPS_ION_TILE_SKIP");
            if (!(v && std::atoi(v) == 0)) HPS_HIP_CHECK(hipMalloc(&ion.d_fbound, (size_t)5*ions.tiling->g.ntiles*sizeof(double))); }
    }
    return HPS_OK;
}

int Engine::sort_sheet (Species& s)
{
    s.pl_alt.n = s.pl.n;
    if (int e = tiling_sort(s.tiling, s.pl, s.pl_alt, gm, st)) return e;
    std::swap(s.pl, s.pl_alt);
    std::swap(s.real, s.real_alt);
    return HPS_OK;
}

int Engine::resort ()
{
    if (int e = sort_sheet(el)) return e;
    for (int k = 2; k < n_sp; ++k) if (sp[k].tiling && sp[k].pl.n > 0) { if (int e = sort_sheet(sp[k])) return e; }      // (the ions are sorted once per step)
    since_sort = 0; ++n_sorts;
    fb_at_sort = h_nfallback ? *h_nfallback : 0;
    return HPS_OK;
}

// InitParticles of one species: every slot of the sheet back on its lattice point, at rest or with its thermal momentum
int Engine::init_sheet (Species& s)
{
    const long n = s.pl.n;
    if (n == 0) return HPS_OK;
    const double radius_sq = d.plasma_radius > 0.0 ? d.plasma_radius*d.plasma_radius : std::numeric_limits<double>::infinity();
    if (warm_init(s)) return init_plasma_warm(*this, s, radius_sq);
    if (hollow_core_radius > 0.0 || (fine_patch_set && s.fine_ppc[0] > 0) || s.dens.on)      // (a density program: init_slot's kernels)
        return init_plasma_fine(*this, s, radius_sq);
    const int nppc = s.ppc[0]*s.ppc[1];
    hipLaunchKernelGGL(k_init_plasma, dim3(ceil_div(n, 256)), dim3(256), 0, st, s.pl, n, d.nx, d.ny, s.ppc[0], s.ppc[1], d.lo[0], d.lo[1],
                       gm.dx, gm.dy, s.density*(d.si_units ? gm.dx*gm.dy*gm.dz/nppc : 1.0/nppc),      // scale_fac, PlasmaParticleContainerInit.cpp:40-41
                       s.init_level, s.keyed, d_prof_r, (int)prof_r.size(), prof_ft, radius_sq);
    return HPS_OK;
}

int Engine::begin_step ()
{
    HPS_REQUIRE(!(d.dt_adaptive && steps_begun == 0 && d.beam_profile < 0 && !host_beam),
                "hps_engine_begin_step: hipace.dt = adaptive needs a beam (beam_profile = -1 and no hps_engine_set_beam_particles: the sum of weights is 0)");
    // (PlasmaParticleContainer.cpp:167-169)
    bool any_fine = false;
    for (const Species& s : sp) any_fine = any_fine || s.fine_ppc[0] > 0;
    HPS_REQUIRE(fine_patch_set == any_fine,
                "hps_engine_begin_step: both fine_ppc (hps_engine_set_plasma_init) and the fine patch (hps_engine_set_fine_patch) must be given to use the fine plasma patch");
    HPS_REQUIRE(!(laser && laser_pulses_set && laser_pulses.empty() && laser_samples.empty() && !step_begun),
                "hps_engine_begin_step: hps_engine_set_laser_pulses with n = 0 needs at least one hps_engine_add_laser_samples");
    // hps_engine_set_laser_grid may have come after hps_engine_add_laser_samples: checked against the grid as it is now, while
    // a refusal still leaves the engine as it was
    if (laser && !step_begun) { for (const LaserSamples& S : laser_samples) { if (int e = laser_check_samples(*this, S)) return e; } }
    if (int e = setup_tiling()) return e;
    el.keyed = coll.empty() ? 0 : 1;      // collisions (all added before the first step): the lattice index in the id bits
    for (int k = 2; k < n_sp; ++k) {      // ... a further species: only if it takes part in one
        sp[k].keyed = 0;
        for (const Collision& c : coll) if ((!c.beam && c.a == k) || c.b == k) sp[k].keyed = 1;
    }
    step_begun = true;
    if (moving && steps_begun > 0) {
        // a slice that outgrew the hand-off capacity during the previous step lost particles: refuse to go on
        int ov = 0;
        HPS_HIP_CHECK(hipMemcpyAsync(&ov, d_beam_overflow, sizeof(int), hipMemcpyDeviceToHost, st));
        HPS_HIP_CHECK(hipStreamSynchronize(st));
        HPS_REQUIRE(ov == 0, "moving beam: a slice outgrew the hand-off capacity (twice the fullest injected slice) in the previous step");
    }
    if (moving && beam_import) {
        // the slices of this step arrive through hps_engine_import_beam_slice: every range empty, imports start at 0
        HPS_HIP_CHECK(hipMemsetAsync(d_B, 0, (size_t)(d.nz + 1)*sizeof(long), st));
        HPS_HIP_CHECK(hipMemsetAsync(d_Bimp, 0, (size_t)(d.nz + 1)*sizeof(long), st));
        HPS_HIP_CHECK(hipMemsetAsync(d_nfront, 0, (size_t)(d.nz + 2)*sizeof(int), st));
        ++steps_begun;
    } else if (moving) {
        if (steps_begun > 0) {
            // the hand-off between steps does not carry the sub-cycle counters (BeamParticleContainer.H:35-37);
            // whatever sits on a slice now is regular (MultiBuffer.cpp:809).  Absorbed particles keep nsub < 0.
            hipLaunchKernelGGL(k_beam_new_step, dim3(ceil_div(std::max(nbeam, 1L), 256)), dim3(256), 0, st, bm_nsub, nbeam);
            HPS_HIP_CHECK(hipMemsetAsync(d_nfront, 0, (size_t)(d.nz + 2)*sizeof(int), st));
        }
        HPS_HIP_CHECK(hipMemcpyAsync(h_B.data(), d_B, (size_t)(d.nz + 1)*sizeof(long), hipMemcpyDeviceToHost, st));
        HPS_HIP_CHECK(hipStreamSynchronize(st));
        ++steps_begun;
    }
    shift_pending = false;      // (the slab is cleared whole below)
    alt_live = false; init_done = false; pend_rode = false;      // (... the alternate planes too: the step starts on the slab's own)
    // ResetAllQuantities (Hipace.cpp:730-742)
    HPS_HIP_CHECK(hipMemsetAsync(slab.p, 0, (size_t)slab.nstride*slab.ncomp*sizeof(double), st));
    // predictor-corrector: nothing but the cold plasma has been deposited in this sweep yet.  Not so from the first slice on
    // with a grid current, and with a second species as particles (or no neutralising background): there the serial path's
    // charges cancel to rounding only, it iterates on that residue itself, and the literal rule on the engine's residue is its
    // match (any non-zero byte pattern reads as "disturbed")
    // A warm plasma deposits real jx, jy from the first slice on.
    // (a further species is a second species as particles)
    if (d_pc_dist) HPS_HIP_CHECK(hipMemsetAsync(d_pc_dist, (d.grid_current_on || d.ion_on || further() || d.plasma_no_neutralize || el.thermal.warm() || ions.thermal.warm()) ? 1 : 0, sizeof(int), st));
    HPS_HIP_CHECK(hipMemsetAsync(d_checksum, 0, HPS_PC_NCOMP_MAX*sizeof(double), st));
    HPS_HIP_CHECK(hipMemsetAsync(d_laser_sum, 0, sizeof(double), st));
    if (int e = join_laser()) return e;        // the time levels rotate: the last slice's envelope must be in
    if (laser) { if (int e = laser_begin_step(*this)) return e; }
    if (d_insitu_pl) HPS_HIP_CHECK(hipMemsetAsync(d_insitu_pl, 0, (size_t)15*d.nz*sizeof(double), st));
    if (d_insitu_pl && further()) {
        const size_t bytes = (size_t)(n_sp - 2)*15*d.nz*sizeof(double);
        if (!d_insitu_pl_more) HPS_HIP_CHECK(hipMalloc(&d_insitu_pl_more, bytes));
        HPS_HIP_CHECK(hipMemsetAsync(d_insitu_pl_more, 0, bytes, st));
    }
    if (d_insitu_bm) HPS_HIP_CHECK(hipMemsetAsync(d_insitu_bm, 0, (size_t)23*d.nz*n_beam_species()*sizeof(double), st));
    if (d_insitu) HPS_HIP_CHECK(hipMemsetAsync(d_insitu, 0, (size_t)10*d.nz*sizeof(double), st));
    if (insitu_laser && laser) { if (int e = laser_clear_insitu(*this)) return e; }
    if (d_fd) HPS_HIP_CHECK(hipMemsetAsync(d_fd, 0, fd_comps.size()*fd_cells()*sizeof(double), st));
    step_index = (next_step >= 0) ? next_step : step_index + 1;      // Hipace::m_physical_time (PlasmaParticleContainerInit.cpp:90)
    next_step = -1;
    ahead_for = -2;
    if (salame_now()) { sal_last_slice = -2; sal_overloaded = false; std::fill(sal_stats.begin(), sal_stats.end(), 0.0); }
    if (d_mom) { if (int e = beam_moments_reset(*this)) return e; }
    if (multi_beam() && !bsp.empty()) {
        long filled = 0;
        for (const BeamSpecies& b : bsp) filled += b.count;
        HPS_REQUIRE(filled == nbeam || beam_import, "hps_engine_begin_step: the beam species' particle counts do not add up to the container's");
    }
    // time factor of the density profile at z = c t of this step (UpdateDensityFunction, PlasmaParticleContainer.cpp:211-217)
    if (time_set) {          // hps_engine_set_time
        step_dt = next_dt; step_time = next_t;
        prof_ft = table_value(prof_t.data(), prof_f_t.data(), (int)prof_t.size(), gm.c*next_t);
        density_begin_step(gm.c*next_t);
        time_set = false;
    } else {
        step_dt = d.dt; step_time = d.dt*step_index;
        prof_ft = table_value(prof_t.data(), prof_f_t.data(), (int)prof_t.size(), gm.c*d.dt*step_index);
        density_begin_step(gm.c*d.dt*step_index);
    }
    if (int e = beam_species_table_upload(*this)) return e;      // several beam species: their constants at this step's dt
    if (laser && lgrid.set) { if (int e = laser_chi_initial(*this)) return e; }      // SetInitialChi: density(x, y, c t) of this step
    if (int e = ionize_collect()) return e;
    el.pl.n = el.n_init;
    if (int e = init_sheet(el)) return e;
    // the further species: back on their lattice too, ahead of the sort that takes them along
    for (int k = 2; k < n_sp; ++k) { sp[k].pl.n = sp[k].n_init; if (int e = init_sheet(sp[k])) return e; }
    if (el.tiling) { if (int e = resort()) return e; }      // (tilings exist only beside the electrons': setup_tiling)
    for (int k = 0; k < n_sp; ++k) {
        // DepositNeutralizingBackground per species (MultiPlasma.cpp:106-118): its initial sheet, deposited once per step with
        // charge -q and without the laser's |a|^2; the electrons first, then the further species (one plane takes the sums)
        const Species& s = sp[k];
        if (!s.neutralize || s.pl.n == 0) continue;
        const int comp[6] = {-1, -1, -1, -1, -1, pc ? (int)HPS_PC_ION_RHOMJZ : (int)HPS_C_ION_RHOMJZ};
        if (s.tiling) {
            TileEnv env = tile_env(); env.aabs_comp = -1;
            DepositArgs a(comp); a.max_qsa = d.max_qsa; a.n_qsa = d_nqsa;
            if (int e = deposit_current_tiled(env, s.sheet(-1.0), a)) return e;
        } else {
            if (int e = hps_deposit_current(slab, s.pl, gm, comp, -s.charge, s.mass, d.order, d.max_qsa, 0, d_nqsa, st)) return e;
        }
    }
    if (ions.present()) {
        // the species "ion": every macro-ion back on its lattice point at its initial level; the product species is back
        // to its own InitParticles count
        if (int e = init_sheet(ions)) return e;
        if (ions.tiling) {
            if (int e = sort_sheet(ions)) return e;
            // every tile may hold charged ions if the species starts ionised; else none does until the push says so
            HPS_HIP_CHECK(hipMemsetAsync(ion.d_tile_flag, ions.init_level > 0 ? 0x01 : 0, (size_t)ions.tiling->g.ntiles*sizeof(int), st));
        }
        const unsigned long long c0[4] = {(unsigned long long)el.n_init, 0ULL, 0ULL, (unsigned long long)ion.n_ionized};
        HPS_HIP_CHECK(hipMemcpyAsync(ion.d_cnt, c0, sizeof(c0), hipMemcpyHostToDevice, st));
        HPS_HIP_CHECK(hipStreamSynchronize(st));      // c0 is on the stack
    }
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// m_grid_current.DepositCurrentSlice (Hipace.cpp:629); z of the slice is plo[2] + islice*dz (GridCurrent.cpp:44)
void Engine::deposit_grid_current (int islice, int cjz)
{
    if (!d.grid_current_on) return;
    const double delta_z = (d.lo[2] + islice*gm.dz - d.grid_current_mean[2]) / d.grid_current_std[2];
    hipLaunchKernelGGL(k_grid_current, dim3(ceil_div(d.nx, 256), d.ny), dim3(256), 0, st, SlabView(slab), cjz, d.lo[0], d.lo[1], gm.dx,
                       gm.dy, d.grid_current_mean[0], d.grid_current_mean[1], d.grid_current_std[0], d.grid_current_std[1],
                       d.grid_current_peak*std::exp(-0.5*(delta_z*delta_z)));
}

// The three particle operators over one species: LDS-tile kernels over the tile-sorted body of the sheet; what has been
// appended behind it since the last sort (electrons released by the species "ion": some hundred particles) rides in the same
// launch on up to 64 extra workgroups (TailWork; HPS_FOLD_TAIL=0: per-particle kernels of their own, 10-40 us of latency
// chains per launch), anything beyond those goes through the per-particle kernels.
TailWork Engine::fold_tail_of (const Species& s, long margin, long* covered) const
{
    const Tiling* T = s.tiling;
    TailWork tw;
    *covered = T->sorted_n;
    if (!fold_tail || !s.grows_tail || T->sorted_n <= 0) return tw;      // (only the plasma's sheet grows a tail)
    const long nt = s.pl.n - T->sorted_n + margin;
    if (nt <= 0) return tw;
    tw.first = (int)T->sorted_n; tw.nwg = (int)std::min<long>(ceil_div(nt, 256), 64);
    *covered = T->sorted_n + 256L*tw.nwg;
    return tw;
}
template <class Tiled, class Plain> int Engine::species_op (const Species& s, const TailWork* live_tail, Tiled&& tiled, Plain&& plain)
{
    const hps_plasma& p = s.pl;
    if (p.n == 0) return HPS_OK;
    if (!s.tiling) return plain(p);
    long covered = 0; const TailWork tw = live_tail ? *live_tail : fold_tail_of(s, 0, &covered);
    if (s.tiling->sorted_n > 0) { if (int e = tiled(tw)) return e; }
    if (!live_tail && p.n > covered) return plain(tail_of(p, covered, p.n - covered));
    return HPS_OK;
}
// (`go` gates the tile kernels only: the device-side loop control that passes it has neither a tail nor a sheet without tiles)
int Engine::species_deposit (const Species& s, const int comp[6], const BeamPairWork* beam, const int* go)
{
    return species_op(s, nullptr,
        [&] (const TailWork& tw) { DepositArgs a(comp); a.max_qsa = d.max_qsa; a.n_qsa = d_nqsa; a.tile_flag = s.tile_flag; a.tw = tw;
                                   a.beam = beam; a.go = go; a.valid_by_w = valid_by_w && s.by_weight;
                                   return deposit_current_tiled(tile_env(), s.sheet(), a); },
        [&] (const hps_plasma& p) { return hps_deposit_current_laser(slab, p, gm, comp, c_aabs, s.charge, s.mass, d.order, d.max_qsa, s.can_ionize, d_nqsa, st); });
}
int Engine::species_explicit (const Species& s, const int cache[4], const int depos[2])
{
    return species_op(s, nullptr,
        [&] (const TailWork& tw) { ExplicitArgs a(cache, depos); a.dtype = d.deriv_type; a.tile_flag = s.tile_flag; a.tw = tw;
                                   a.valid_by_w = valid_by_w && s.by_weight;
                                   return explicit_deposit_tiled(tile_env(), s.sheet(), a); },
        [&] (const hps_plasma& p) { return hps_explicit_deposit_laser(slab, p, gm, cache, c_aabs, depos, s.charge, s.mass, d.order, d.deriv_type, s.can_ionize, st); });
}
int Engine::species_advance (const Species& s, const int comp[5], int temp_slice, const int* go, const IonArgs* ion, const TailWork* live_tail)
{
    return species_op(s, live_tail,
        [&] (const TailWork& tw) { PushArgs a(comp); a.temp_slice = temp_slice; a.n_subcycles = d.n_subcycles; a.ion = ion; a.go = go; a.tw = tw;
                                   return advance_plasma_tiled(tile_env(), s.sheet(), a); },
        [&] (const hps_plasma& p) { return hps_advance_plasma_laser(slab, p, gm, comp, c_aabs, s.charge, s.mass, d.order, temp_slice, d.n_subcycles, s.can_ionize, st); });
}

// HPS_EVENT_FENCE: 0 = HIP's default system-scope release at every event, 1 (default) = none at the engine's own
// events (their consumers are streams of this device; measured: ring hand-off 14 us per slice cheaper),
// 2 = none at the ring's events either (no further gain)
unsigned event_flags (bool timing)
{
    static const int mode = [] { const char* v = std::getenv("HPS_EVENT_FENCE"); return v ? std::atoi(v) : 1; }();
    unsigned f = timing ? 0u : (unsigned)hipEventDisableTiming;
    if (mode >= 1) f |= timing ? (unsigned)hipEventReleaseToDevice : (unsigned)hipEventDisableSystemFence;
    return f;
}

int Engine::fork_laser ()
{
    if (laser_stream() == st) return HPS_OK;
    HPS_HIP_CHECK(hipEventRecord(ev_lfork, st));
    HPS_HIP_CHECK(hipStreamWaitEvent(st_laser, ev_lfork, 0));
    return HPS_OK;
}
int Engine::laser_done ()
{
    if (laser_stream() == st) return HPS_OK;
    HPS_HIP_CHECK(hipEventRecord(ev_ldone, st_laser));
    laser_pending = true;
    return HPS_OK;
}
int Engine::join_laser ()
{
    if (!laser_pending) return HPS_OK;
    HPS_HIP_CHECK(hipStreamWaitEvent(st, ev_ldone, 0));
    laser_pending = false;
    return HPS_OK;
}

void Engine::mark ()
{
    if (!prof_now) return;
    const int k = (int)(ev_used % 11);                  // which of the 11 marks of a slice this is
    if (ev_used == ev.size()) { hipEvent_t e; (void)hipEventCreateWithFlags(&e, event_flags(true)); ev.push_back(e); }
    // light mode: only the marks around the deposition kernel (2, 3) and the kernel-free pair (4, 5)
    if (!prof_light || (k >= 2 && k <= 5)) (void)hipEventRecord(ev[ev_used], st);
    ++ev_used;
}

// The slice in two halves for a host that drives several engines from one thread (several time steps in flight on one
// device, hps_engine_solve_slice_begin / _finish): begin enqueues everything up to and including the speculated V-cycles of
// the Bx/By solve (and the gated push behind them) and returns without waiting for the device; finish waits for the
// solve's norms -- the one host wait of a slice -- and enqueues the rest.  solve_slice = begin + finish.
// Makes the slab what an observer expects: the pending shift done, the slice just solved on the slab's own planes.
// (HPS_EARLY_INIT: that slice is in the alternate planes if it ran on them and its pass did not ride, or if it ran on the slab's
//  own and its pass rode -- then those hold the next slice's zeros.  Either way the two sets change places, the zeros with
//  them: the next slice finds them where `live` then points, and a run that goes on is not disturbed.)
void Engine::flush_shift ()
{
    const dim3 gplane(ceil_div(slab.nstride, 256)), b256(256);
    if (shift_pending) {
        shift_pending = false;
        const CellBox bb{beam_box.ilo, beam_box.ihi, beam_box.jlo, beam_box.jhi};
        hipLaunchKernelGGL(k_shift_slices, gplane, b256, 0, st, slab.p, slab.nstride, slab.nstride, (int)slab.jstride, bb, live().njxb, live().njyb);
    }
    if (alt_live != init_done) {
        CompList a{0, {}}, b{0, {}};
        for (int k = 0; k < 2; ++k) {
            const InitSet& x = k ? set_alt : set_canon; CompList& l = k ? b : a;
            for (int c : {x.chi, x.rhomjz, x.rho, x.jzb, x.njxb, x.njyb}) if (c >= 0) l.c[l.n++] = c;
        }
        CompList dst = a, src = b;       // dst = own | alternate, src = alternate | own
        for (int k = 0; k < b.n; ++k) { dst.c[dst.n++] = b.c[k]; src.c[src.n++] = a.c[k]; }
        copy_comps(slab, st, dst, src);
        alt_live = !alt_live;
    }
}

int Engine::solve_slice (int islice)
{
    if (int e = solve_slice_begin(islice)) return e;
    return solve_slice_finish(islice);
}

int Engine::solve_slice_begin (int islice)
{
    HPS_REQUIRE(pending_slice == -1, "hps_engine_solve_slice_begin: the previous slice has not been finished");
    if (pc) { if (int e = solve_slice_pc_begin(islice)) return e; pending_slice = islice; return HPS_OK; }
    SlabView f(slab);
    const long plane = slab.nstride;
    const dim3 b256(256);
    const dim3 gplane(ceil_div(plane, 256));
    const dim3 gvalid(ceil_div(d.nx, 256), d.ny);
    int e;

    prof_now = profiling && (slices_done % prof_stride == 0);
    mg_solve1_forget_hierarchy(mg);            // (left set only if the previous slice failed between prepare and begin)
    if ((e = join_laser())) return e;          // the envelope solver of the previous slice has read its chi
    mark();   // b0
    insitu_plasma(islice);        // m_multi_plasma.InSituComputeDiags (Hipace.cpp:590)
    // InitializeSlices (fields/Fields.cpp:535-586)
    const CellBox bb{beam_box.ilo, beam_box.ihi, beam_box.jlo, beam_box.jhi};
    // the previous slice's fused push + deposition has already shifted / zeroed the slab and deposited this slice's
    // plasma currents (k_shift_zero + k_advance_deposit_tiled)
    const bool ahead = (ahead_for == islice);
    ahead_for = -2;
    // HPS_EARLY_INIT: a slice of the plain path -- nothing but the kernels below and the push touches the re-initialised planes --
    // runs on whichever set of them is live; any other slice runs on the slab's own, with the zeroing pass of its own
    const bool plain = n_alt > 0 && !moving && coll.empty() && c_aabs < 0 && !ions.present() && !further() && !salame_now() && !fuse_push_deposit && !ahead
                       && lazy_shift && !aux_on && !diagnostics && !d_fd && !d_insitu;
    if (!plain && (alt_live || init_done)) {
        flush_shift();
        alt_live = false; init_done = false;      // (zeros left in the alternate planes are dropped)
    }
    const InitSet L = live();
    // ShiftSlices of the slice before, left pending at its end (lazy_shift), and this slice's InitializeSlices in one pass
    // (init_done: both have ridden in the previous slice's Bx/By solve)
    bool zeroed = init_done;
    init_done = false;
    if (shift_pending) {
        shift_pending = false;
        if (!ahead) { hipLaunchKernelGGL(k_shift_zero, gplane, b256, 0, st, ShiftInit{slab.p, slab.nstride, plane, (int)slab.jstride, bb, L, L, (int)HPS_C_ION_RHOMJZ}); zeroed = true; }
        else hipLaunchKernelGGL(k_shift_slices, gplane, b256, 0, st, slab.p, slab.nstride, plane, (int)slab.jstride, bb, L.njxb, L.njyb);
    }
    if (!ahead && !zeroed)
    {   CompList z{0, {}}, zb{0, {}};
        // Sx, Sy are written as whole planes by k_sxsy_beam; ExmBy, EypBx by k_grad_psi up to the outermost
        // guard ring, which nothing ever writes (it keeps the zeros of begin_step); the beam planes only
        // ever hold values inside the beam's box
        for (int c : {L.chi, L.rhomjz}) z.c[z.n++] = c;
        if (d.deposit_rho) z.c[z.n++] = L.rho;
        for (int c : {L.jzb, L.njxb, L.njyb}) zb.c[zb.n++] = c;
        CompList fi{0, {}};
        fi.c[fi.n++] = L.rhomjz; if (d.deposit_rho) fi.c[fi.n++] = L.rho;
        zero_comps(slab, st, z, zb, bb, fi, (int)HPS_C_ION_RHOMJZ); }
    if (c_aabs >= 0) {
        // UpdateLaserAabs (Hipace.cpp:603)
        if ((e = laser_update_aabs(*this, islice, diagnostics ? d_laser_sum : nullptr))) return e;
    }
    // the auxiliary stream may start on the beam's planes (zeroed above)
    // SALAME's step 0 (MultiBeam::isSalameNow): the slice runs through the plain sequence -- no paired / folded beam deposit, no
    // auxiliary stream, no fused or gated push, no deferred shift -- and the SALAME beam deposits no jx, jy on Next (MultiBeam.cpp:50-56)
    const bool sal = salame_now();
    const bool aux = aux_on && st_aux && !pc && !ahead && !prof_now && !sal;
    if (aux) { HPS_HIP_CHECK(hipEventRecord(ev_aux[0], st)); HPS_HIP_CHECK(hipStreamWaitEvent(st_aux, ev_aux[0], 0)); }

    mark();   // b1
    // plasma: jx, jy, [rho], chi, rhomjz (Hipace.cpp:609-610); beam: jz_beam on This (:613-614)
    // re-sort after sort_period slices at the latest, earlier once more than 1/256 of the sheet has left
    // the halo of its tile (h_nfallback is as of the previous slice's multigrid sync)
    // (with a species "ion": also once the electrons appended behind the sorted body since the last sort -- they run
    // through the per-particle kernels -- are more than 1/32 of the sheet)
    if (el.tiling && (since_sort >= sort_period || (since_sort >= 2 && *h_nfallback - fb_at_sort > el.pl.n/fallback_div) ||
                      (since_sort >= 1 && el.pl.n - el.tiling->sorted_n > std::max(el.pl.n/32, 16384L)))) { if ((e = resort())) return e; }
    ++since_sort;
    mark();   // b1b
    // static beam: jz of this slice and jx, jy of the next one in one go (Hipace.cpp:613-614, 656-657), as extra workgroups of
    // the plasma's deposition where that runs on tiles; a moving beam keeps the two calls (the next slice's block is only
    // final once this slice's push has handed its slipped particles on -- it is deposited after the solves below as before)
    const bool pair = !moving && nbeam > 0 && !sal;
    BeamPairWork bw;
    if (pair) {
        const long fA = beam_off[d.nz - 1 - islice], cA = beam_off[d.nz - islice] - fA;
        const long fB = islice >= 1 ? beam_off[d.nz - islice] : 0, cB = islice >= 1 ? beam_off[d.nz - islice + 1] - fB : 0;
        double* pa = beam_cur + 7*fA; double* pb = beam_cur + 7*fB;
        bw.a = BeamView{pa, pa + cA, pa + 2*cA, pa + 3*cA, pa + 4*cA, pa + 5*cA, pa + 6*cA};
        bw.b = BeamView{pb, pb + cB, pb + 2*cB, pb + 3*cB, pb + 4*cB, pb + 5*cB, pb + 6*cB};
        bw.ca = cA; bw.cb = cB; bw.nba = (int)ceil_div(cA, 256); bw.nwg = bw.nba + (int)ceil_div(cB, 256);
        bw.cjz = L.jzb; bw.cjxn = L.njxb; bw.cjyn = L.njyb;
        bw.q_invvol = d.beam_charge*(d.si_units ? 1.0/(gm.dx*gm.dy*gm.dz) : 1.0); bw.csq_inv = 1.0/(gm.c*gm.c);
    }
    const bool beam_folded = pair && fold_beam && bw.nwg > 0 && !ahead && el.pl.n > 0 && el.tiling && el.tiling->sorted_n > 0;
    if (!ahead)
    {   const int comp[6] = {HPS_C_JX, HPS_C_JY, -1, L.rho, L.chi, L.rhomjz};
        if ((e = species_deposit(el, comp, beam_folded ? &bw : nullptr))) return e;
        // MultiPlasma::DepositCurrent: every species in turn (MultiPlasma.cpp:78-87); an ion weighs in with its level
        for (int k = 1; k < n_sp; ++k) { if ((e = species_deposit(sp[k], comp))) return e; } }
    mark();   // b2
    if (pair) {
        if (!beam_folded && bw.nwg > 0) {
            // (beside the plasma's deposition and the Poisson solves: nothing ahead of the Sx/Sy initialisation reads the beam's planes)
            hipStream_t sb = (aux && !d.grid_current_on) ? st_aux : st;
            beam_deposit_pair(slab, bw, gm, d.order, sb);
        }
    } else if ((e = deposit_beam_slice(islice, -1, -1, L.jzb))) return e;
    deposit_grid_current(islice, L.jzb);
    if (aux) {
        // chi is final: the multigrid's coefficient hierarchy on the auxiliary stream, joined ahead of the Sx/Sy initialisation
        HPS_HIP_CHECK(hipEventRecord(ev_aux[1], st)); HPS_HIP_CHECK(hipStreamWaitEvent(st_aux, ev_aux[1], 0));
        if ((e = mg_solve1_prepare(mg, slab, HPS_C_BX, HPS_C_SY, L.chi, 200, st_aux))) return e;
        HPS_HIP_CHECK(hipEventRecord(ev_aux[2], st_aux));
        aux_pending = true;
    }

    // AddRhoIons + Psi, Ez, Bz solves + -grad Psi (fields/Fields.cpp:840-957)
    {   const double fa = 1.0/(gm.ep0*gm.c);
        const double fez_x = fa*0.5*(1.0/gm.dx), fez_y = fa*0.5*(1.0/gm.dy), fbz_y = gm.mu0*0.5*(1.0/gm.dy), fbz_x = -gm.mu0*0.5*(1.0/gm.dx);
        const int comps[3] = {HPS_C_PSI, HPS_C_EZ, HPS_C_BZ};
        if (fuse_sources && poisson_sources_fusable(ps) && d.field_bc == 0) {
            // the three sources (fields/Fields.cpp:887-912) are formed by the first transform pass while it loads its rows:
            // -rhomjz/ep0;  (d_x jx + d_y jy)/(ep0 c);  mu0 (d_y jx - d_x jy) -- centred differences, guard cells read as they are
            const long js = slab.jstride;
            const double* R = slab.p + (long)L.rhomjz*slab.nstride + g + (long)g*js;       // cell (0, 0) of the planes
            const double* X = slab.p + (long)HPS_C_JX*slab.nstride + g + (long)g*js;
            const double* Y = slab.p + (long)HPS_C_JY*slab.nstride + g + (long)g*js;
            const PoissonSrc spec[3] = {
                {1, {R, nullptr}, {nullptr, nullptr}, {-1.0/gm.ep0, 0.0}},
                {2, {X + 1, Y + js}, {X - 1, Y - js}, {fez_x, fez_y}},
                {2, {X + js, Y + 1}, {X - js, Y - 1}, {fbz_y, fbz_x}}};
            if ((e = poisson_solve_batch_src(ps, 3, spec, js, slab, comps, st))) return e;
        } else {
            hipLaunchKernelGGL(k_rhs_all, dim3(ceil_div(slab.jstride, 256), d.ny + 2*g), b256, 0, st, f, L.rhomjz,
                               -1 /* AddRhoIons: done by the slice's zeroing pass */, L.rho, HPS_C_JX, HPS_C_JY, 1.0/gm.ep0,
                               fez_x, fez_y, fbz_y, fbz_x, staging, (long)d.nx*d.ny);
            if ((e = open_boundary(3, 0x6u))) return e;
            if ((e = hps_poisson_solve_batch(ps, 3, staging, slab, comps, st))) return e;
        } }
    // m_multi_laser.AdvanceSlice (Hipace.cpp:637): a_{n+1} of this slice from chi and the neighbouring slices
    // On the laser's own stream when there is one, forked here (chi is final; nothing else of this slice needs a_{n+1}).
    // FFT solver (0.11 ms of bandwidth-bound passes at 1024^2): enqueued at once; beside the explicit deposition or beside
    // the Bx/By multigrid it gets half of its time back either way (measured: 898 -> 949 slices/s on config 5 without the
    // dopant; stream priority makes no difference).  Multigrid solver (0.7 ms, latency-bound, holds the host once per
    // V-cycle): enqueued further down, when the engine's stream has the explicit deposition and the Bx/By V-cycles
    // queued (545 -> 706 slices/s).
    const bool laser_now = c_aabs >= 0 && d.laser_solver >= 1 && d.dt != 0.0 && laser_has_slice(islice);      // UseLaser(islice)
    const bool laser_split = laser_now && laser_stream() != st;
    if (laser_now && !laser_split) { if ((e = laser_advance_slice(*this, islice))) return e; }
    if (laser_split) { if ((e = fork_laser())) return e; }
    if (laser_split && d.laser_solver == 1) { if ((e = laser_advance_slice(*this, islice)) || (e = laser_done())) return e; }
    if (aux_pending) { HPS_HIP_CHECK(hipStreamWaitEvent(st, ev_aux[2], 0)); aux_pending = false; }
    if (pair || nbeam == 0) {
        // -grad Psi and the beam part of Sx, Sy (Hipace.cpp:659-660) in one pass (without a beam there is no deposition between them either)
        const GradPsiSxSy ga{HPS_C_PSI, HPS_C_EXMBY, HPS_C_EYPBX, 0.5*(1.0/gm.dx), 0.5*(1.0/gm.dy), HPS_C_SX, HPS_C_SY, L.jzb, L.njxb, L.njyb,
                             HPS_C_P_JXB, HPS_C_P_JYB, gm.mu0, 2.0*gm.dx, 2.0*gm.dy, 2.0*gm.dz, bb};
        // ... and, in the same launch, the coefficient hierarchy of the Bx/By multigrid solve (it needs chi only): one launch less
        // on the chain between the explicit deposition and the first smoothing pass
        bool with_hierarchy = false;
        if (fold_hierarchy && !pc && !aux) {
            if ((e = mg_solve1_prepare_with(mg, slab, HPS_C_BX, HPS_C_SY, L.chi, 200, f, ga, st, &with_hierarchy))) return e;
        }
        if (!with_hierarchy)
            hipLaunchKernelGGL(k_gradpsi_sxsy, dim3(ceil_div(slab.jstride, 256), d.ny + 2*g), b256, 0, st, f, ga);
        mark();   // b3
    } else {
        hipLaunchKernelGGL(k_grad_psi, dim3(ceil_div(d.nx + 2*(g - 1), 256), d.ny + 2*(g - 1)), b256, 0, st, f, HPS_C_PSI,
                           HPS_C_EXMBY, HPS_C_EYPBX, 0.5*(1.0/gm.dx), 0.5*(1.0/gm.dy));
        mark();   // b3
        // beam jx, jy of the next slice; beam part of Sx, Sy (Hipace.cpp:656-660)
        // (SALAME's step 0: a do_salame beam deposits no jx, jy on Next, every other species does -- MultiBeam.cpp:50-56)
        const unsigned smask = (sal && moving) ? salame_mask() : 0u;
        if (!sal || (moving && smask == 0)) { if ((e = deposit_beam_slice(islice - 1, L.njxb, L.njyb, -1))) return e; }
        else if (moving && nbeam > 0) { if ((e = beam_deposit_species(*this, d.nz - islice, species_mask_all() & ~smask, L.njxb, L.njyb, -1))) return e; }
        hipLaunchKernelGGL(k_sxsy_beam, dim3(ceil_div(slab.jstride, 256), d.ny + 2*g), b256, 0, st, f, HPS_C_SX, HPS_C_SY, L.jzb, L.njxb, L.njyb,
                           HPS_C_P_JXB, HPS_C_P_JYB, gm.mu0, 2.0*gm.dx, 2.0*gm.dy, 2.0*gm.dz, bb);
    }
    mark();   // b4
    {   const int cache[4] = {HPS_C_BZ, HPS_C_EZ, HPS_C_EXMBY, HPS_C_EYPBX};
        const int depos[2] = {HPS_C_SY, HPS_C_SX};
        for (const Species& s : sp) { if ((e = species_explicit(s, cache, depos))) return e; } }

    mark();   // b5
    // Bx, By: Helmholtz multigrid from the previous slice's field (Hipace.cpp:793-933).  The plain case (one tile-sorted
    // species, nothing that reads the fields between the solve and the push) enqueues the push BEHIND the speculated
    // V-cycles, gated on the solve's own stopping rule, and only then waits for the norms: the device goes from the last
    // V-cycle straight into the push instead of idling until the host has seen the norms and launched it.
    const bool fuse = fuse_push_deposit && coll.empty() && el.tiling && islice > 0 && !moving && c_aabs < 0 && !ions.present() && !further() && el.pl.n > 0 && el.tiling->sorted_n == el.pl.n && !sal;
    const bool gated = gate_push && el.tiling && !fuse && !ions.present() && !further() && el.pl.n > 0 && el.tiling->sorted_n == el.pl.n && !diagnostics && !d_fd && !d_insitu && !sal;
    // ... and with an ionisable species on tiles: its field bounds, its push (which takes the ADK decisions and appends the
    // electrons) and the electrons' push, all behind the speculated V-cycles; the two pushes are gated (HPS_GATED_ION_PUSH=0: off)
    const bool gated_ion = gate_push && gate_ion_push && el.tiling && !fuse && ions.present() && !further() && ions.tiling && el.pl.n > 0 && el.tiling->sorted_n > 0 && fold_tail
                           && !diagnostics && !d_fd && !d_insitu && !sal;
    const int comp_push[5] = {HPS_C_PSI, HPS_C_EZ, HPS_C_BX, HPS_C_BY, HPS_C_BZ};
    {
        // the plain gated push also posts the solve's norms to the host (k_advance_tiled's MgPost): no k_post_norms launch between
        // the last V-cycle and the push (HPS_POST_IN_PUSH=0: the launch of its own)
        if (gated && post_in_push) mg_defer_post(mg);
        // the plain gated slice: nothing from here to its end reads what the next slice's shift / zero pass overwrites -- it rides
        // in the first lower V of the solve, writing the zeros to the set of planes that is not live (HPS_EARLY_INIT)
        pend_rode = plain && gated && islice > 0
                    && mg_ride_shift_init(mg, ShiftInit{slab.p, slab.nstride, plane, (int)slab.jstride, bb, L, other(), (int)HPS_C_ION_RHOMJZ});
        if ((e = mg_solve1_begin(mg, slab, HPS_C_BX, HPS_C_SY, L.chi, d.mg_tol_rel, d.mg_tol_abs, 200, st))) return e;
        if (gated_ion) {
            mark();   // b6
            mark();   // b7
            if ((e = push_with_ionization(islice, comp_push, mg_gate_after_enqueued(mg), true, &pend_covered))) return e;
        }
        if (gated) {
            mark();   // b6
            mark();   // b7
            MgPost mp{};
            const bool posting = mg_take_deferred_post(mg, &mp);
            PushArgs a(comp_push); a.n_subcycles = d.n_subcycles; if (posting) a.post = &mp; else a.go = mg_gate_after_enqueued(mg);
            if ((e = advance_plasma_tiled(tile_env(), el.sheet(), a))) return e;
        }
        if (laser_split && d.laser_solver == 2) { if ((e = laser_advance_slice(*this, islice)) || (e = laser_done())) return e; }
        pending_slice = islice; pend_fuse = fuse; pend_gated = gated; pend_gated_ion = gated_ion;
        HPS_HIP_CHECK(hipGetLastError());
        return HPS_OK;
    }
}

// DoFieldIonization (Hipace.cpp:693-696), then the ions' own committing push; the host learns how many electrons the slice has
// released while that push runs (ionize_collect).  go, first: as push_with_ionization's.  (The tiled branch relies on the ions'
// sheet having no tail -- it is sorted whole once per step and nothing is appended to it: particles behind the sorted body
// would go through species_advance's per-particle kernel, which takes no ADK decisions.)
int Engine::push_ions (int islice, const int comp[5], const int* go, bool first)
{
    if (ions.tiling) {       // decided inside the ions' LDS-tile push, on the fields it gathers anyway
        if (int e = ion_field_bounds()) return e;
        if (first) pend_ia = ion_args(islice);
        return species_advance(ions, comp, 0, go, &pend_ia);
    }
    if (int e = ionize_slice(islice)) return e;       // k_ionize ahead of the per-particle push
    return species_advance(ions, comp, 0);
}

// DoFieldIonization + the ions' push + the electrons' push (Hipace.cpp:693-701) of a slice on tiles, enqueued without a word from
// the host in between: the ions' field bounds, the ions' push (ADK decisions on the fields it gathers, electrons appended on the
// device), the electrons' tile-sorted body with the tail's workgroups reading the live particle count.  `go`: the multigrid
// solve's gate word (both pushes do nothing unless the solve is over); first = false: the same launches again, ungated, after
// the host has added V-cycles (same ADK sequence number: the count is posted once).
int Engine::push_with_ionization (int islice, const int comp[5], const int* go, bool first, long* covered)
{
    if (int e = push_ions(islice, comp, go, first)) return e;
    // the electrons' tile-sorted body does not depend on how many electrons the slice has released: push it while the count travels
    // to the host (ionize_collect), then the rest with the new count (push_leftover).  The tail's workgroups in that launch read the
    // count on the device -- the ions' push is ahead of them on the stream --, with room for 256 electrons more than the host knows of
    *covered = -1;
    if (!el.tiling || el.tiling->sorted_n <= 0) return HPS_OK;
    TailWork tw = fold_tail_of(el, 256, covered);
    if (tw.nwg) tw.live_n = ion.d_cnt;
    return species_advance(el, comp, 0, go, nullptr, &tw);
}

// the electrons the slice has released beyond the room (`covered`) that push_with_ionization's launch had for them
int Engine::push_leftover (const int comp[5], long covered)
{
    if (el.pl.n <= covered) return HPS_OK;
    return hps_advance_plasma_laser(slab, tail_of(el.pl, covered, el.pl.n - covered), gm, comp, c_aabs, el.charge, el.mass, d.order, 0, d.n_subcycles, 0, st);
}

int Engine::solve_slice_finish (int islice)
{
    HPS_REQUIRE(pending_slice == islice, "hps_engine_solve_slice_finish: not the slice that hps_engine_solve_slice_begin started");
    pending_slice = -1;
    if (pc) return solve_slice_pc_finish(islice);
    const long plane = slab.nstride;
    const dim3 b256(256);
    const dim3 gplane(ceil_div(plane, 256));
    const CellBox bb{beam_box.ilo, beam_box.ihi, beam_box.jlo, beam_box.jhi};
    const bool fuse = pend_fuse, gated = pend_gated, gated_ion = pend_gated_ion;
    const int comp_push[5] = {HPS_C_PSI, HPS_C_EZ, HPS_C_BX, HPS_C_BY, HPS_C_BZ};
    int e;
    {   int iters = 0, extra = 0;
        if ((e = mg_solve1_finish(mg, &iters, nullptr, &extra, st))) return e;
        total_vcycles += iters;
        // the speculated V-cycles were not enough (the gated push has not run): the host has added the rest, push now
        if (gated && extra) { if ((e = species_advance(el, comp_push, 0))) return e; }
        if (gated_ion) {
            if (extra) { if ((e = push_with_ionization(islice, comp_push, nullptr, false, &pend_covered))) return e; }
            if ((e = ionize_collect()) || (e = push_leftover(comp_push, pend_covered))) return e;      // (a gated slice has a body: pend_covered >= 0)
        } }

    // SalameModule (Hipace.cpp:673-678): behind the Bx/By solve, ahead of the diagnostics and the push, on a slice whose beam
    // block holds particles
    if (salame_now() && !moving && nbeam > 0 && beam_off[d.nz - islice] - beam_off[d.nz - 1 - islice] > 0) {
        if ((e = salame_module(islice))) return e;
    }
    // ... a moving-beam engine: on a slice that held particles of a do_salame species when the step began (MultiBeam::isSalameNow
    // counts getNumParticles(This): what has slipped in during this step does not count)
    if (salame_now() && moving && nbeam > 0 && salame_count(d.nz - 1 - islice) > 0) {
        if ((e = salame_module(islice))) return e;
    }

    if (!gated && !gated_ion) {
    mark();   // b6
    checksum_slice();
    if ((e = fill_field_diagnostic(islice))) return e;      // FillFieldDiagnostics (Hipace.cpp:691)
    insitu_fields(islice);                                  // Fields::InSituComputeDiags (Hipace.cpp:686)

    mark();   // b7
    // gather + push (Hipace.cpp:699-701)
    {   const int* comp = comp_push;
        long covered = -1;      // the electrons that push_with_ionization has launched; -1: none, the whole sheet is still to push
        if (ions.present()) { if ((e = push_with_ionization(islice, comp, nullptr, true, &covered)) || (e = ionize_collect())) return e; }
        // push of this slice and deposition of the next one in one pass over the sheet (static beam, no laser, one
        // plasma species, the whole sheet inside the tile-sorted body)
        if (fuse) {
            hipLaunchKernelGGL(k_shift_zero, gplane, b256, 0, st, ShiftInit{slab.p, slab.nstride, plane, (int)slab.jstride, bb, set_canon, set_canon, (int)HPS_C_ION_RHOMJZ});
            const int dep[6] = {HPS_C_JX, HPS_C_JY, -1, d.deposit_rho ? HPS_C_RHO : -1, HPS_C_CHI, HPS_C_RHOMJZ};
            if ((e = advance_deposit_tiled(tile_env(), el.sheet(), comp, dep, d.n_subcycles, d.max_qsa, d_nqsa))) return e;
            ahead_for = islice - 1;
        } else if (covered >= 0) {
            if ((e = push_leftover(comp, covered))) return e;
        } else {
            if ((e = species_advance(el, comp, 0))) return e;
        }
        // the further species (a slice that holds one is never gated or fused)
        for (int k = 2; k < n_sp; ++k) { if ((e = species_advance(sp[k], comp, 0))) return e; } }
    }

    // beam push and hand-off of the slipped particles (Hipace.cpp:704-706)
    insitu_beam(islice);
    if (moving && nbeam > 0) { if ((e = beam_push_moving(*this, islice))) return e; }
    if (!coll.empty()) { if ((e = collide_slice(islice))) return e; }      // doCoulombCollision (Hipace.cpp:711-712)
    mark();   // b8
    // ShiftSlices (fields/Fields.cpp:588-604)
    // (lazy_shift: left to the start of the next slice, where it shares a pass with InitializeSlices; anything that looks at
    //  the slab in between -- hps_engine_slab, _sync, the diagnostics' accessors -- runs it first: flush_shift)
    // (HPS_EARLY_INIT: the shift and the next slice's zeros have ridden in this slice's Bx/By solve -- the sets change roles)
    if (pend_rode) { pend_rode = false; alt_live = !alt_live; init_done = true; ++slices_rode; }
    else if (ahead_for != islice - 1) {
        if (lazy_shift && islice > 0 && !salame_now()) shift_pending = true;
        else hipLaunchKernelGGL(k_shift_slices, gplane, b256, 0, st, slab.p, slab.nstride, plane, (int)slab.jstride, bb, live().njxb, live().njyb);
    }
    mark();   // b9
    HPS_HIP_CHECK(hipGetLastError());
    ++slices_done;
    return HPS_OK;
}

int Engine::run_step ()
{
    if (int e = begin_step()) return e;
    for (int isl = d.nz - 1; isl >= 0; --isl)
        if (int e = solve_slice(isl)) return e;
    return HPS_OK;
}

} // namespace hps

using namespace hps;

extern "C" const char* hps_last_error (void) { return g_err.c_str(); }
extern "C" const char* hps_version (void) { return "hpslice 0.1 (gfx950)"; }

extern "C" int hps_engine_create (const hps_deck* deck, int device, void** handle)
{
    HPS_REQUIRE(deck && handle, "hps_engine_create: null argument");
    Engine* E = new Engine;
    if (int e = E->create(*deck, device)) { delete E; return e; }
    *handle = E;
    return HPS_OK;
}
extern "C" int hps_engine_destroy (void* h) { delete static_cast<Engine*>(h); return HPS_OK; }
extern "C" int hps_engine_begin_step (void* h) { return static_cast<Engine*>(h)->begin_step(); }
extern "C" int hps_engine_solve_slice (void* h, int islice) { return static_cast<Engine*>(h)->solve_slice(islice); }
extern "C" int hps_engine_solve_slice_begin (void* h, int islice) { return static_cast<Engine*>(h)->solve_slice_begin(islice); }
extern "C" int hps_engine_slice_ready (void* h)
{
    Engine* E = static_cast<Engine*>(h);
    if (E->pc) return E->pc_slice_ready();
    if (E->pending_slice < 0) return 1;
    return mg_solve1_ready(E->mg) ? 1 : 0;
}
extern "C" int hps_engine_solve_slice_finish (void* h, int islice) { return static_cast<Engine*>(h)->solve_slice_finish(islice); }
extern "C" int hps_engine_run_step (void* h) { return static_cast<Engine*>(h)->run_step(); }
extern "C" int hps_engine_sync (void* h)
{
    Engine* E = static_cast<Engine*>(h);
    E->flush_shift();
    if (int e = E->join_laser()) return e;
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    if (E->moving && E->d_beam_overflow) {
        // a slice that outgrew the hand-off capacity lost particles: say so at the end of the step that did it (also the last
        // step of a run, and a stage that runs one step only), not at the next begin_step of this engine
        int ov = 0;
        HPS_HIP_CHECK(hipMemcpy(&ov, E->d_beam_overflow, sizeof(int), hipMemcpyDeviceToHost));
        HPS_REQUIRE(ov == 0, "moving beam: a slice outgrew the hand-off capacity (twice the fullest injected slice): particles were lost");
    }
    return HPS_OK;
}
extern "C" int hps_engine_info (void* h, int* ncomp, int* ng, long* np)
{
    Engine* E = static_cast<Engine*>(h);
    if (ncomp) *ncomp = E->ncomp;
    if (ng) *ng = E->g;
    if (np) *np = E->el.pl.n;
    return HPS_OK;
}
extern "C" hps_slab hps_engine_slab (void* h)
{
    Engine* E = static_cast<Engine*>(h);
    E->flush_shift();
    hps_slab s = E->slab; s.ncomp -= E->n_alt;      // (the alternate planes of HPS_EARLY_INIT are the engine's own business)
    return s;
}
extern "C" int hps_engine_early_init_slices (void* h, long* n)
{
    HPS_REQUIRE(h && n, "hps_engine_early_init_slices: null argument");
    *n = static_cast<Engine*>(h)->slices_rode;
    return HPS_OK;
}
extern "C" int hps_engine_schedule (void* h, int* mg_coef_guest, int* valid_by_psi)
{
    HPS_REQUIRE(h, "hps_engine_schedule: null handle");
    Engine* E = static_cast<Engine*>(h);
    if (mg_coef_guest) { *mg_coef_guest = 0; if (E->mg) { if (int e = hps_mg_info_schedule(E->mg, mg_coef_guest)) return e; } }
    if (valid_by_psi) *valid_by_psi = (E->tile_size != 0 && E->valid_by_psi) ? 1 : 0;
    return HPS_OK;
}
extern "C" int hps_engine_qsa_drops (void* h, long* n)
{
    HPS_REQUIRE(h && n, "hps_engine_qsa_drops: null argument");
    Engine* E = static_cast<Engine*>(h);
    int v = 0;
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    HPS_HIP_CHECK(hipMemcpy(&v, E->d_nqsa, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return HPS_OK;
}
extern "C" hps_plasma hps_engine_plasma (void* h) { return static_cast<Engine*>(h)->el.pl; }
extern "C" int hps_engine_tiling (void* h, void** tiling)
{
    HPS_REQUIRE(h && tiling, "hps_engine_tiling: null argument");
    *tiling = static_cast<Engine*>(h)->el.tiling;
    return HPS_OK;
}
extern "C" hps_plasma hps_engine_ions (void* h)
{
    Engine* E = static_cast<Engine*>(h);
    (void)hipStreamSynchronize(E->st);
    return E->ions.pl;
}
extern "C" int hps_engine_add_plasma_species (void* h, const hps_plasma_species* s, int* index_out)
{
    HPS_REQUIRE(h, "hps_engine_add_plasma_species: null engine");
    return static_cast<Engine*>(h)->add_plasma_species(s, index_out);
}
extern "C" int hps_engine_plasma_species_info (void* h, int* n, long* counts)
{
    HPS_REQUIRE(h, "hps_engine_plasma_species_info: null engine");
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    if (int e = E->ionize_collect()) return e;
    if (n) *n = E->n_sp;
    for (int k = 0; counts && k < E->n_sp; ++k) counts[k] = E->sp[k].pl.n;
    return HPS_OK;
}
extern "C" hps_plasma hps_engine_plasma_species (void* h, int k)
{
    Engine* E = static_cast<Engine*>(h);
    if (!E || !E->plasma_species_ok(k)) return hps_plasma{};
    (void)hipStreamSynchronize(E->st);
    return E->sp[k].pl;
}
extern "C" int hps_engine_ion_stats (void* h, long* n_ionized, long* n_product)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    if (int e = E->ionize_collect()) return e;
    if (n_ionized) *n_ionized = E->ion.n_ionized;
    if (n_product) *n_product = E->el.pl.n;
    return HPS_OK;
}
extern "C" hps_stream hps_engine_stream (void* h) { return static_cast<Engine*>(h)->st; }
extern "C" int hps_engine_stats (void* h, long* vc, long* sl)
{
    Engine* E = static_cast<Engine*>(h);
    if (vc) *vc = E->total_vcycles;
    if (sl) *sl = E->slices_done;
    return HPS_OK;
}
extern "C" int hps_engine_record_event (void* h, int slot, void** out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(slot >= 0 && slot < (1 << 20) && out, "hps_engine_record_event: bad slot");
    if ((size_t)slot >= E->hand_ev.size()) E->hand_ev.resize((size_t)slot + 1, nullptr);
    if (!E->hand_ev[slot]) HPS_HIP_CHECK(hipEventCreateWithFlags(&E->hand_ev[slot], event_flags(false)));
    if (int e = E->join_laser()) return e;     // "everything the engine has been given so far" includes the laser stream's slice
    HPS_HIP_CHECK(hipEventRecord(E->hand_ev[slot], E->st));
    *out = E->hand_ev[slot];
    return HPS_OK;
}
extern "C" int hps_engine_wait_event (void* h, void* event)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(event, "hps_engine_wait_event: null event");
    HPS_REQUIRE(!ring_is_ticket(event), "hps_engine_wait_event: this is the receive handle of an ipc ring edge, not a hipEvent_t -- order the engine behind "
                                        "it with hps_ring_engine_wait(ring, engine, handle), which works for both kinds of edge");
    HPS_HIP_CHECK(hipStreamWaitEvent(E->st, static_cast<hipEvent_t>(event), 0));
    return HPS_OK;
}
extern "C" int hps_engine_copy_async (void* h, void* dst, const void* src, long bytes)
{
    Engine* E = static_cast<Engine*>(h);
    if (bytes <= 0) return HPS_OK;
    HPS_REQUIRE(dst && src, "hps_engine_copy_async: null pointer");
    HPS_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, E->st));
    return HPS_OK;
}
extern "C" int hps_engine_set_step (void* h, int step)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && step >= 0, "hps_engine_set_step: bad argument");
    E->next_step = step;
    return HPS_OK;
}
extern "C" int hps_engine_set_time (void* h, double t, double dt)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && std::isfinite(t) && std::isfinite(dt), "hps_engine_set_time: bad argument");
    E->next_t = t; E->next_dt = dt; E->time_set = true;
    return HPS_OK;
}
extern "C" int hps_engine_set_profiling (void* h, int on)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    E->profiling = (on != 0); E->prof_light = (on == 2); E->ev_used = 0; E->prof_now = false;
    return HPS_OK;
}
extern "C" int hps_engine_set_profiling_stride (void* h, int stride)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(stride >= 1, "hps_engine_set_profiling_stride: stride >= 1");
    E->prof_stride = stride;
    return HPS_OK;
}
extern "C" int hps_engine_phase_times (void* h, double* ms, long* nsl)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    // interval -> phase: 0 deposit, 1 poisson, 2 explicit, 3 mg, 4 push, 5 other
    static const int phase_of[10] = {5, 6, 0, 1, 5, 2, 3, 5, 4, 5};
    for (int k = 0; k < 8; ++k) ms[k] = 0.0;
    const size_t ns = E->ev_used/11;
    // interval 4 (b3 -> b4) holds no kernel when the two beam deposits share a launch (static beam, explicit solver): two
    // event records back to back, i.e. what an interval costs by itself
    const bool empty4 = !E->pc && !E->moving && E->nbeam > 0;
    for (size_t s = 0; s < ns; ++s)
        for (int k = 0; k < 10; ++k) {
            if (E->prof_light && k != 2 && k != 4) continue;     // light mode recorded marks 2..5 only
            float t = 0.f;
            HPS_HIP_CHECK(hipEventElapsedTime(&t, E->ev[s*11 + k], E->ev[s*11 + k + 1]));
            ms[phase_of[k]] += t;
            if (k == 4 && empty4) ms[7] += t;
        }
    if (nsl) *nsl = (long)ns;
    E->ev_used = 0;
    return HPS_OK;
}
extern "C" int hps_engine_set_tiling (void* h, int tile_size, int sort_period)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(tile_size == 0 || tile_size == 16 || tile_size == 32, "hps_engine_set_tiling: tile_size must be 0, 16 or 32");
    HPS_REQUIRE(sort_period >= 1, "hps_engine_set_tiling: sort_period must be >= 1");
    HPS_REQUIRE(E->el.tiling == nullptr, "hps_engine_set_tiling: call before the first hps_engine_begin_step");
    E->tile_size = tile_size; E->sort_period = sort_period;
    return HPS_OK;
}
extern "C" int hps_engine_set_density_profile (void* h, int nr, const double* r_host, const double* fr_host, int nt, const double* ct_host,
                                              const double* ft_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(nr >= 0 && nt >= 0 && (nr == 0 || (r_host && fr_host)) && (nt == 0 || (ct_host && ft_host)), "hps_engine_set_density_profile: bad argument");
    for (int k = 1; k < nr; ++k) HPS_REQUIRE(r_host[k] > r_host[k - 1], "hps_engine_set_density_profile: r must increase");
    for (int k = 1; k < nt; ++k) HPS_REQUIRE(ct_host[k] > ct_host[k - 1], "hps_engine_set_density_profile: ct must increase");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    (void)hipFree(E->d_prof_r); E->d_prof_r = nullptr;
    E->prof_r.assign(r_host, r_host + nr);
    E->prof_t.assign(ct_host, ct_host + nt); E->prof_f_t.assign(ft_host, ft_host + nt);
    if (nr > 0) {
        std::vector<double> both(r_host, r_host + nr);
        both.insert(both.end(), fr_host, fr_host + nr);
        HPS_HIP_CHECK(hipMalloc(&E->d_prof_r, both.size()*sizeof(double)));
        HPS_HIP_CHECK(hipMemcpy(E->d_prof_r, both.data(), both.size()*sizeof(double), hipMemcpyHostToDevice));
    }
    return HPS_OK;
}
extern "C" int hps_engine_set_fusion (void* h, int on)
{
    static_cast<Engine*>(h)->fuse_push_deposit = (on != 0);
    return HPS_OK;
}
extern "C" int hps_engine_set_plasma_init (void* h, const int* plasma_fine, const int* ion_fine, double hollow_core_radius)
{
    HPS_REQUIRE(h, "hps_engine_set_plasma_init: null engine");
    return static_cast<Engine*>(h)->set_plasma_init(plasma_fine, ion_fine, hollow_core_radius);
}
extern "C" int hps_engine_set_plasma_momentum (void* h, int species, const double* u_mean, const double* u_std, unsigned long long seed)
{
    HPS_REQUIRE(h, "hps_engine_set_plasma_momentum: null engine");
    return static_cast<Engine*>(h)->set_plasma_momentum(species, u_mean, u_std, seed);
}
extern "C" int hps_engine_set_plasma_symmetry (void* h, int do_symmetrize, int prevent_centered_particle)
{
    HPS_REQUIRE(h, "hps_engine_set_plasma_symmetry: null engine");
    return static_cast<Engine*>(h)->set_plasma_symmetry(do_symmetrize, prevent_centered_particle);
}
extern "C" int hps_engine_set_fine_patch (void* h, const unsigned char* mask_host, int transition_cells)
{
    HPS_REQUIRE(h, "hps_engine_set_fine_patch: null engine");
    return static_cast<Engine*>(h)->set_fine_patch(mask_host, transition_cells);
}
extern "C" int hps_engine_fallbacks (void* h, long* n)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    int v = 0;
    HPS_HIP_CHECK(hipMemcpy(&v, E->d_nfallback, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return HPS_OK;
}
extern "C" int hps_engine_sorts (void* h, long* n) { *n = static_cast<Engine*>(h)->n_sorts; return HPS_OK; }

extern "C" int hps_memcpy_d2h (void* dst, const void* src, long bytes) { HPS_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return HPS_OK; }
extern "C" int hps_memcpy_h2d (void* dst, const void* src, long bytes) { HPS_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return HPS_OK; }
extern "C" int hps_device_count (int* n)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return HPS_OK;
}
