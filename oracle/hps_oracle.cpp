// hps_oracle.cpp -- CPU restatement of the HiPACE++ per-zeta-slice hot path.
//
// THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg may load this library.  The product path
// (hipace_amd/csrc + include/hpslice.h) never includes, links or calls anything here.
//
// It restates, in plain serial C++ (g++ -O2 -ffp-contract=off), the reference's *serial CPU
// semantics* of every function on the slice path, citing the reference file:line each routine
// follows (paths relative to /root/reference/src).  Parity pin: the end-to-end driver at the
// bottom reproduces the reference's own golden checksums
//   tests/checksum/benchmarks_json/linear_wake.normalized.1Rank.json
//   tests/checksum/benchmarks_json/blowout_wake_explicit.2Rank.json
//   tests/checksum/benchmarks_json/beam_in_vacuum.normalized.Serial.json
//   tests/checksum/benchmarks_json/beam_evolution.1Rank.json                              (moving beam, 21 steps)
//   tests/checksum/benchmarks_json/beam_in_vacuum_open_boundary.normalized.1Rank.json     (predictor-corrector loop)
//   tests/checksum/benchmarks_json/{beam_in_vacuum.normalized.1Rank,beam_in_vacuum.SI.1Rank,beam_in_vacuum.SI.Serial}.json
//   tests/checksum/benchmarks_json/{linear_wake.SI.1Rank,blowout_wake.2Rank,blowout_wake.Serial,grid_current.1Rank}.json
//   tests/checksum/benchmarks_json/{laser_blowout_wake_explicit.1Rank,laser_blowout_wake_explicit.SI.1Rank}.json
//   tests/checksum/benchmarks_json/{gaussian_linear_wake.normalized.1Rank,gaussian_linear_wake.SI.1Rank,reset.2Rank}.json
//   tests/checksum/benchmarks_json/laser_evolution.SI.2Rank.json                          (FFT envelope solver, 30 steps)
// (copied as data fixtures into tests/golden/), see tests/test_oracle_golden.py.  Parts no checksum of the
// reference covers are pinned on the reference's own analysis criteria instead (predictor-corrector vs explicit
// solver, examples/linear_wake/analysis_equal.py; diagnostic coarsening, examples/blowout_wake/analysis_coarsening.py)
// or declared unpinned (the particle tile sort, which is AMReX code absent from /root/reference).
// The reference executable itself cannot be built here (AMReX/FFTW are un-vendored
// network dependencies), so oracle/_ref does not exist; see DESIGN.md.
//
// Layout conventions follow the reference: slab components are planes of
// (nx+2g) x (ny+2g) doubles, x fastest (AMReX Fortran order, utils/GPUUtil.H:99-147).

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

using std::size_t;
typedef double Real;

// CPU-baseline leg of bench.py: number of OpenMP threads (orc_set_threads).  1 = the reference's serial CPU path,
// exactly the loops below in their written order (what the golden checksums are pinned on).  > 1 = the reference's
// OpenMP build: scatter kernels over 4-colour tiles (particles/deposition/DepositionUtil.H:204-253), everything else
// `omp parallel for` over independent rows / particles (bit-identical to the serial loops).
int g_threads = 1;

// ---------------------------------------------------------------------------------------------
// Shape factors                                  particles/particles_utils/ShapeFactors.H
// ---------------------------------------------------------------------------------------------

// compute_shape_factor<order>  (ShapeFactors.H:27-108): weights + left-most cell
int shape_factor (int order, Real* sx, Real xmid)
{
    if (order == 0) {
        const int j = static_cast<int>(std::floor(xmid + 0.5));
        sx[0] = 1.0;
        return j;
    } else if (order == 1) {
        const int j = static_cast<int>(std::floor(xmid));
        const Real xint = xmid - j;
        sx[0] = 1.0 - xint;
        sx[1] = xint;
        return j;
    } else if (order == 2) {
        const int j = static_cast<int>(std::floor(xmid + 0.5));
        const Real xint = xmid - j;
        sx[0] = 0.5*(0.5 - xint)*(0.5 - xint);
        sx[1] = 0.75 - xint*xint;
        sx[2] = 0.5*(0.5 + xint)*(0.5 + xint);
        return j - 1;
    } else {
        const int j = static_cast<int>(std::floor(xmid));
        const Real xint = xmid - j;
        sx[0] = 1.0/6.0*(1.0 - xint)*(1.0 - xint)*(1.0 - xint);
        sx[1] = 2.0/3.0 - xint*xint*(1.0 - xint/2.0);
        sx[2] = 2.0/3.0 - (1.0 - xint)*(1.0 - xint)*(1.0 - 0.5*(1.0 - xint));
        sx[3] = 1.0/6.0*xint*xint*xint;
        return j - 1;
    }
}

struct DShape { Real s; Real ds; int cell; };

// single_derivative_shape_factor<derivative_type, order>(xmid, ix)  (ShapeFactors.H:211-466)
// returns {shape, -d(shape)/dx, cell}.  derivative_type: 0 analytic, 1 nodal, 2 centred.
DShape deriv_shape (int dtype, int order, Real xmid, int ix)
{
    Real s = 0, d = 0; int cell = 0;
    if (dtype == 0) {
        if (order == 0) {
            xmid += 0.5; const Real xf = std::floor(xmid);
            s = 1; d = 0; cell = static_cast<int>(xf);
        } else if (order == 1) {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            if (ix == 0) { s = 1 - x; d = -1; } else { s = x; d = 1; }
            cell = static_cast<int>(xf) + ix;
        } else if (order == 2) {
            xmid += 0.5; const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x;
            if (ix == 0)      { s = (1.0/2.0)*x2 - 1.0*x + 0.5; d = x - 1.0; }
            else if (ix == 1) { s = -x2 + 1.0*x + 0.5;          d = 1.0 - 2*x; }
            else              { s = (1.0/2.0)*x2;               d = x; }
            cell = static_cast<int>(xf) - 1 + ix;
        } else {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x, x3 = x2*x;
            if (ix == 0)      { s = -1.0/6.0*x3 + (1.0/2.0)*x2 - 1.0/2.0*x + 1.0/6.0; d = -1.0/2.0*x2 + x - 1.0/2.0; }
            else if (ix == 1) { s = (1.0/2.0)*x3 - x2 + 2.0/3.0;                      d = (3.0/2.0)*x2 - 2*x; }
            else if (ix == 2) { s = -1.0/2.0*x3 + (1.0/2.0)*x2 + (1.0/2.0)*x + 1.0/6.0; d = -3.0/2.0*x2 + x + 1.0/2.0; }
            else              { s = (1.0/6.0)*x3;                                     d = (1.0/2.0)*x2; }
            cell = static_cast<int>(xf) - 1 + ix;
        }
    } else if (dtype == 1) {
        if (order == 0) {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            if (ix == 0) { s = (x < 0.5) ? 1 : 0; d = -1; } else { s = (x < 0.5) ? 0 : 1; d = 1; }
            cell = static_cast<int>(xf) + ix;
        } else if (order == 1) {
            xmid += 0.5; const Real xf = std::floor(xmid); const Real x = xmid - xf;
            if (ix == 0)      { s = (x < 0.5) ? 1.0/2.0 - x : 0;               d = x - 1; }
            else if (ix == 1) { s = (x < 0.5) ? x + 1.0/2.0 : 3.0/2.0 - x;     d = 1 - 2*x; }
            else              { s = (x < 0.5) ? 0 : x - 1.0/2.0;               d = x; }
            cell = static_cast<int>(xf) - 1 + ix;
        } else if (order == 2) {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x;
            if (ix == 0) {
                s = (x < 0.5) ? (1.0/2.0)*x2 - 1.0/2.0*x + 1.0/8.0 : 0;
                d = -1.0/2.0*x2 + x - 1.0/2.0;
            } else if (ix == 1) {
                s = (x < 0.5) ? 3.0/4.0 - x2 : (1.0/2.0)*x2 - 3.0/2.0*x + 9.0/8.0;
                d = (3.0/2.0)*x2 - 2*x;
            } else if (ix == 2) {
                s = (x < 0.5) ? (1.0/2.0)*x2 + (1.0/2.0)*x + 1.0/8.0 : -x2 + 2*x - 1.0/4.0;
                d = -3.0/2.0*x2 + x + 1.0/2.0;
            } else {
                s = (x < 0.5) ? 0 : (1.0/2.0)*x2 - 1.0/2.0*x + 1.0/8.0;
                d = (1.0/2.0)*x2;
            }
            cell = static_cast<int>(xf) - 1 + ix;
        } else {
            xmid += 0.5; const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x, x3 = x2*x;
            if (ix == 0) {
                s = (x < 0.5) ? -1.0/6.0*x3 + (1.0/4.0)*x2 - 1.0/8.0*x + 1.0/48.0 : 0;
                d = (1.0/6.0)*x3 - 1.0/2.0*x2 + (1.0/2.0)*x - 1.0/6.0;
            } else if (ix == 1) {
                s = (x < 0.5) ? (1.0/2.0)*x3 - 1.0/4.0*x2 - 5.0/8.0*x + 23.0/48.0
                              : -1.0/6.0*x3 + (3.0/4.0)*x2 - 9.0/8.0*x + 9.0/16.0;
                d = -2.0/3.0*x3 + (3.0/2.0)*x2 - 1.0/2.0*x - 1.0/2.0;
            } else if (ix == 2) {
                s = (x < 0.5) ? -1.0/2.0*x3 - 1.0/4.0*x2 + (5.0/8.0)*x + 23.0/48.0
                              : (1.0/2.0)*x3 - 7.0/4.0*x2 + (11.0/8.0)*x + 17.0/48.0;
                d = x3 - 3.0/2.0*x2 - 1.0/2.0*x + 1.0/2.0;
            } else if (ix == 3) {
                s = (x < 0.5) ? (1.0/6.0)*x3 + (1.0/4.0)*x2 + (1.0/8.0)*x + 1.0/48.0
                              : -1.0/2.0*x3 + (5.0/4.0)*x2 - 3.0/8.0*x + 5.0/48.0;
                d = -2.0/3.0*x3 + (1.0/2.0)*x2 + (1.0/2.0)*x + 1.0/6.0;
            } else {
                s = (x < 0.5) ? 0 : (1.0/6.0)*x3 - 1.0/4.0*x2 + (1.0/8.0)*x - 1.0/48.0;
                d = (1.0/6.0)*x3;
            }
            cell = static_cast<int>(xf) - 2 + ix;
        }
    } else {
        if (order == 0) {
            xmid += 0.5; const Real xf = std::floor(xmid);
            if (ix == 0)      { s = 0; d = -1.0/2.0; }
            else if (ix == 1) { s = 1; d = 0; }
            else              { s = 0; d = 1.0/2.0; }
            cell = static_cast<int>(xf) - 1 + ix;
        } else if (order == 1) {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            if (ix == 0)      { s = 0;     d = (1.0/2.0)*x - 1.0/2.0; }
            else if (ix == 1) { s = 1 - x; d = -1.0/2.0*x; }
            else if (ix == 2) { s = x;     d = 1.0/2.0 - 1.0/2.0*x; }
            else              { s = 0;     d = (1.0/2.0)*x; }
            cell = static_cast<int>(xf) - 1 + ix;
        } else if (order == 2) {
            xmid += 0.5; const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x;
            if (ix == 0)      { s = 0;                          d = -1.0/4.0*x2 + (1.0/2.0)*x - 1.0/4.0; }
            else if (ix == 1) { s = (1.0/2.0)*x2 - x + 1.0/2.0; d = (1.0/2.0)*x2 - 1.0/2.0*x - 1.0/4.0; }
            else if (ix == 2) { s = -x2 + x + 1.0/2.0;          d = 1.0/4.0 - 1.0/2.0*x; }
            else if (ix == 3) { s = (1.0/2.0)*x2;               d = -1.0/2.0*x2 + (1.0/2.0)*x + 1.0/4.0; }
            else              { s = 0;                          d = (1.0/4.0)*x2; }
            cell = static_cast<int>(xf) - 2 + ix;
        } else {
            const Real xf = std::floor(xmid); const Real x = xmid - xf;
            const Real x2 = x*x, x3 = x2*x;
            if (ix == 0)      { s = 0; d = (1.0/12.0)*x3 - 1.0/4.0*x2 + (1.0/4.0)*x - 1.0/12.0; }
            else if (ix == 1) { s = -1.0/6.0*x3 + (1.0/2.0)*x2 - 1.0/2.0*x + 1.0/6.0; d = -1.0/4.0*x3 + (1.0/2.0)*x2 - 1.0/3.0; }
            else if (ix == 2) { s = (1.0/2.0)*x3 - x2 + 2.0/3.0; d = (1.0/6.0)*x3 - 1.0/2.0*x; }
            else if (ix == 3) { s = -1.0/2.0*x3 + (1.0/2.0)*x2 + (1.0/2.0)*x + 1.0/6.0; d = (1.0/6.0)*x3 - 1.0/2.0*x2 + 1.0/3.0; }
            else if (ix == 4) { s = (1.0/6.0)*x3; d = -1.0/4.0*x3 + (1.0/4.0)*x2 + (1.0/4.0)*x + 1.0/12.0; }
            else              { s = 0; d = (1.0/12.0)*x3; }
            cell = static_cast<int>(xf) - 2 + ix;
        }
    }
    return {s, -d, cell};
}

// ---------------------------------------------------------------------------------------------
// Data views
// ---------------------------------------------------------------------------------------------

// Array3 view of the field slab (utils/GPUUtil.H:99-147): (i,j,n), i in [-g, nx+g)
struct Slab {
    Real* p; int nx, ny, g, ncomp; long js, ns;
    Real& operator() (int i, int j, int n) const { return p[(i+g) + (long)(j+g)*js + (long)n*ns]; }
    Real* comp (int n) const { return p + (long)n*ns; }
};

// Plasma SoA (particles/plasma/PlasmaParticleContainer.H:21-46).  valid = idcpu id sign.
struct Plasma {
    Real *x,*y,*w,*ux,*uy,*psi,*x_prev,*y_prev,*ux_half,*uy_half,*psi_half;
    int32_t* valid; int32_t* ion_lev; long n;
};

struct Geom {
    Real dx, dy, dz;          // cell sizes
    Real xoff, yoff;          // GetPosOffset (fields/Fields.H:71-77)
    Real c, ep0, mu0, q_e, m_e;
    Real plo[2], phi[2];      // particle boundary box
    int bc;                   // 0 Reflecting, 1 Periodic, 2 Absorbing (Hipace.H ParticleBoundary)
    int normalized;
};

// Particle loop of a scatter kernel.  One thread: particles in storage order (DepositionUtil.H:256-264).  Several:
// particles binned by the tile of their nearest cell, tiles visited in 4 colours so that no two threads write to the
// same cell (DepositionUtil.H:204-253, hipace.tile_size = 32 >= the widest stencil).
template <class F>
void scatter_loop (const Plasma& pl, const Geom& gm, int nx, int ny, F&& body)
{
    if (g_threads <= 1) { for (long ip = 0; ip < pl.n; ++ip) body(ip); return; }
    const int ts = 32;
    const int ntx = (nx + ts - 1)/ts, nty = (ny + ts - 1)/ts;
    std::vector<long> offs((size_t)ntx*nty + 2, 0);
    std::vector<int> tile_of((size_t)pl.n);
    const Real dx_inv = 1.0/gm.dx, dy_inv = 1.0/gm.dy;
#pragma omp parallel for num_threads(g_threads) schedule(static)
    for (long ip = 0; ip < pl.n; ++ip) {
        int t = ntx*nty;
        if (pl.valid[ip]) {
            int ci = (int)std::floor((pl.x[ip] - gm.xoff)*dx_inv + 0.5), cj = (int)std::floor((pl.y[ip] - gm.yoff)*dy_inv + 0.5);
            ci = std::min(std::max(ci, 0), nx - 1); cj = std::min(std::max(cj, 0), ny - 1);
            t = (ci/ts)*nty + cj/ts;
        }
        tile_of[(size_t)ip] = t;
    }
    for (long ip = 0; ip < pl.n; ++ip) ++offs[(size_t)tile_of[(size_t)ip] + 1];
    for (size_t t = 0; t + 1 < offs.size(); ++t) offs[t + 1] += offs[t];
    std::vector<long> perm((size_t)pl.n), cur(offs.begin(), offs.end() - 1);
    for (long ip = 0; ip < pl.n; ++ip) perm[(size_t)cur[(size_t)tile_of[(size_t)ip]]++] = ip;
    for (int px = 0; px < 2; ++px) for (int py = 0; py < 2; ++py) {
#pragma omp parallel for collapse(2) num_threads(g_threads) schedule(dynamic)
        for (int tx = px; tx < ntx; tx += 2) for (int ty = py; ty < nty; ty += 2) {
            const size_t t = (size_t)tx*nty + ty;
            for (long q = offs[t]; q < offs[t + 1]; ++q) body(perm[(size_t)q]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Plasma current deposition      particles/deposition/PlasmaDepositCurrent.cpp:155-246,
// serial semantics of            particles/deposition/DepositionUtil.H:256-264
// comp = {jx, jy, jz, rho, chi, rhomjz}, -1 to skip
// ---------------------------------------------------------------------------------------------
// doLaserGatherShapeN (particles/particles_utils/FieldGather.H:236-331): |a|^2 (and optionally its centred x, y
// differences) at the particle with the plain deposition-order shape
void laser_gather (int order, Real xp, Real yp, const Slab& f, int aabs_comp, Real dx_inv, Real dy_inv, Real xoff, Real yoff,
                   Real& A, Real* ADx, Real* ADy)
{
    Real sx[4], sy[4];
    const int i0 = shape_factor(order, sx, (xp - xoff)*dx_inv);
    const int j0 = shape_factor(order, sy, (yp - yoff)*dy_inv);
    for (int iy = 0; iy <= order; ++iy) for (int ix = 0; ix <= order; ++ix) {
        const int i = i0 + ix, j = j0 + iy;
        A += sx[ix]*sy[iy]*f(i, j, aabs_comp);
        if (ADx) {
            *ADx += sx[ix]*sy[iy]*0.5*dx_inv*(f(i+1, j, aabs_comp) - f(i-1, j, aabs_comp));
            *ADy += sx[ix]*sy[iy]*0.5*dy_inv*(f(i, j+1, aabs_comp) - f(i, j-1, aabs_comp));
        }
    }
}

long deposit_current (const Slab& f, const Plasma& pl, const Geom& gm, const int* comp,
                      Real charge, Real mass, int order, Real max_qsa, int can_ionize, int aabs_comp = -1)
{
    // laser_norm (PlasmaDepositCurrent.cpp:80-81)
    const Real laser_norm = (charge/gm.q_e)*(gm.m_e/mass)*(charge/gm.q_e)*(gm.m_e/mass);
    const Real dx_inv = 1.0/gm.dx, dy_inv = 1.0/gm.dy, dz_inv = 1.0/gm.dz;
    const Real invvol = gm.normalized ? gm.dx*gm.dy*dx_inv*dy_inv : dx_inv*dy_inv*dz_inv;
    const Real clight = gm.c, clightinv = 1.0/gm.c;
    const Real charge_invvol = charge*invvol;
    const Real charge_mu0_mass_ratio = charge*gm.mu0/mass;
    long n_qsa = 0;
    scatter_loop(pl, gm, f.nx, f.ny, [&] (long ip) {
        if (!pl.valid[ip]) return;
        const Real psi_inv = 1.0/pl.psi[ip];
        const Real xp = pl.x[ip], yp = pl.y[ip];
        const Real vx_c = pl.ux[ip]*psi_inv;
        const Real vy_c = pl.uy[ip]*psi_inv;
        Real q_invvol = charge_invvol*pl.w[ip];
        Real q_mu0_mass_ratio = charge_mu0_mass_ratio;
        if (can_ionize) { q_invvol *= pl.ion_lev[ip]; q_mu0_mass_ratio *= pl.ion_lev[ip]; }
        const Real xmid = (xp - gm.xoff)*dx_inv;
        const Real ymid = (yp - gm.yoff)*dy_inv;
        Real Aabssqp = 0.0;
        if (aabs_comp >= 0) {
            laser_gather(order, xp, yp, f, aabs_comp, dx_inv, dy_inv, gm.xoff, gm.yoff, Aabssqp, nullptr, nullptr);
            Aabssqp *= laser_norm*(can_ionize ? (Real)pl.ion_lev[ip]*pl.ion_lev[ip] : 1.0);
        }
        const Real gamma_psi = 0.5*((1.0 + 0.5*Aabssqp)*psi_inv*psi_inv
                                    + vx_c*vx_c*clightinv*clightinv
                                    + vy_c*vy_c*clightinv*clightinv + 1.0);
        if (gamma_psi < 0.0 || gamma_psi > max_qsa || psi_inv < 0.0) {
#pragma omp atomic
            ++n_qsa;
            pl.w[ip] = 0.0; pl.valid[ip] = 0; return;
        }
        Real sx[4], sy[4];
        const int i0 = shape_factor(order, sx, xmid);
        const int j0 = shape_factor(order, sy, ymid);
        for (int iy = 0; iy <= order; ++iy) {
            for (int ix = 0; ix <= order; ++ix) {
                const int i = i0 + ix, j = j0 + iy;
                const Real charge_density = q_invvol*sx[ix]*sy[iy];
                if (comp[0] != -1) {
                    f(i,j,comp[0]) += charge_density*vx_c;
                    f(i,j,comp[1]) += charge_density*vy_c;
                }
                if (comp[2] != -1) f(i,j,comp[2]) += charge_density*(gamma_psi - 1.0)*clight;
                if (comp[3] != -1) f(i,j,comp[3]) += charge_density*gamma_psi;
                if (comp[4] != -1) f(i,j,comp[4]) += charge_density*q_mu0_mass_ratio*psi_inv;
                if (comp[5] != -1) f(i,j,comp[5]) += charge_density;
            }
        }
    });
    return n_qsa;
}

// ---------------------------------------------------------------------------------------------
// Explicit-solver source deposition     particles/deposition/ExplicitDeposition.cpp:140-261
// cache = {Bz, Ez, ExmBy, EypBx}; depos = {Sy, Sx}
// ---------------------------------------------------------------------------------------------
void explicit_deposit (const Slab& f, const Plasma& pl, const Geom& gm, const int* cache,
                       const int* depos, Real charge, Real mass, int order, int dtype,
                       int can_ionize, int aabs_comp = -1)
{
    // "The laser a0 is always normalized" (ExplicitDeposition.cpp:57-58)
    const Real laser_fac = (gm.m_e/gm.q_e)*(gm.m_e/gm.q_e);
    const Real dx_inv = 1.0/gm.dx, dy_inv = 1.0/gm.dy, dz_inv = 1.0/gm.dz;
    const Real invvol = gm.normalized ? gm.dx*gm.dy*dx_inv*dy_inv : dx_inv*dy_inv*dz_inv;
    const Real a_clight = gm.c, clight_inv = 1.0/gm.c;
    const Real charge_invvol_mu0 = charge*invvol*gm.mu0;
    const Real charge_mass_ratio = charge/mass;
    scatter_loop(pl, gm, f.nx, f.ny, [&] (long ip) {
        if (!pl.valid[ip]) return;
        const Real psi_inv = 1.0/pl.psi[ip];
        const Real xp = pl.x[ip], yp = pl.y[ip];
        const Real vx = pl.ux[ip]*psi_inv*clight_inv;
        const Real vy = pl.uy[ip]*psi_inv*clight_inv;
        Real q_invvol_mu0 = charge_invvol_mu0;
        Real q_mass_ratio = charge_mass_ratio;
        if (can_ionize) { q_invvol_mu0 *= pl.ion_lev[ip]; q_mass_ratio *= pl.ion_lev[ip]; }
        const Real charge_density_mu0 = q_invvol_mu0*pl.w[ip];
        const Real xmid = (xp - gm.xoff)*dx_inv;
        const Real ymid = (yp - gm.yoff)*dy_inv;
        Real Aabssqp = 0.0;
        if (aabs_comp >= 0) {
            laser_gather(order, xp, yp, f, aabs_comp, dx_inv, dy_inv, gm.xoff, gm.yoff, Aabssqp, nullptr, nullptr);
            Aabssqp *= laser_fac*q_mass_ratio*q_mass_ratio;
        }
        const Real gamma_psi = 0.5*((1.0 + 0.5*Aabssqp)*psi_inv*psi_inv + vx*vx + vy*vy + 1.0);
        for (int iy = 0; iy <= order + dtype; ++iy) {
            for (int ix = 0; ix <= order + dtype; ++ix) {
                if (dtype == 2) {
                    if ((ix == 0 || ix == order + 2) && (iy == 0 || iy == order + 2)) continue;
                }
                const DShape Y = deriv_shape(dtype, order, ymid, iy);
                const DShape X = deriv_shape(dtype, order, xmid, ix);
                const int i = X.cell, j = Y.cell;
                const Real shape_x = X.s, shape_dx = X.ds, shape_y = Y.s, shape_dy = Y.ds;
                const Real Bz_v = f(i,j,cache[0]);
                const Real Ez_v = f(i,j,cache[1]);
                const Real ExmBy_v = f(i,j,cache[2]);
                const Real EypBx_v = f(i,j,cache[3]);
                Real AabssqDxp = 0.0, AabssqDyp = 0.0;
                if (aabs_comp >= 0 && shape_x*shape_y != 0.0) {        // (:215-226)
                    AabssqDxp = (f(i+1,j,aabs_comp) - f(i-1,j,aabs_comp))*0.5*dx_inv*laser_fac*a_clight;
                    AabssqDyp = (f(i,j+1,aabs_comp) - f(i,j-1,aabs_comp))*0.5*dy_inv*laser_fac*a_clight;
                }
                f(i,j,depos[0]) += charge_density_mu0*(
                    - shape_x*shape_y*(
                        - Bz_v*vx
                        + ( Ez_v*vy
                        + ExmBy_v*(          - vx*vy)
                        + EypBx_v*(gamma_psi - vy*vy) )*clight_inv
                        - 0.25*AabssqDyp*q_mass_ratio*psi_inv
                    )*q_mass_ratio*psi_inv
                    + ( - shape_dx*shape_y*dx_inv*(
                        - vx*vy
                    )
                    - shape_x*shape_dy*dy_inv*(
                        gamma_psi - vy*vy - 1.0
                    ))*a_clight);
                f(i,j,depos[1]) += charge_density_mu0*(
                    + shape_x*shape_y*(
                        + Bz_v*vy
                        + ( Ez_v*vx
                        + ExmBy_v*(gamma_psi - vx*vx)
                        + EypBx_v*(          - vx*vy) )*clight_inv
                        - 0.25*AabssqDxp*q_mass_ratio*psi_inv
                    )*q_mass_ratio*psi_inv
                    + ( + shape_dx*shape_y*dx_inv*(
                        gamma_psi - vx*vx - 1.0
                    )
                    + shape_x*shape_dy*dy_inv*(
                        - vx*vy
                    ))*a_clight);
            }
        }
    });
}

// ---------------------------------------------------------------------------------------------
// Field gather      particles/particles_utils/FieldGather.H:45-96 (doGatherShapeN, nodal
// derivative of Psi on the fly)
// ---------------------------------------------------------------------------------------------
void gather (int order, Real xp, Real yp, Real& ExmByp, Real& EypBxp, Real& Ezp, Real& Bxp,
             Real& Byp, Real& Bzp, const Slab& f, const int* c, Real dx_inv, Real dy_inv,
             Real xoff, Real yoff)
{
    const Real x = (xp - xoff)*dx_inv;
    const Real y = (yp - yoff)*dy_inv;
    const int dtype = 1;
    for (int iy = 0; iy <= order + dtype; ++iy) {
        for (int ix = 0; ix <= order + dtype; ++ix) {
            const DShape Y = deriv_shape(dtype, order, y, iy);
            const DShape X = deriv_shape(dtype, order, x, ix);
            const int i = X.cell, j = Y.cell;
            ExmByp += (X.ds*Y.s)*f(i,j,c[0])*dx_inv;
            EypBxp += (X.s*Y.ds)*f(i,j,c[0])*dy_inv;
            Ezp    += (X.s*Y.s)*f(i,j,c[1]);
            Bxp    += (X.s*Y.s)*f(i,j,c[2]);
            Byp    += (X.s*Y.s)*f(i,j,c[3]);
            Bzp    += (X.s*Y.s)*f(i,j,c[4]);
        }
    }
}

// PlasmaMomentumPush<T>  (particles/pusher/PushPlasmaParticles.H:39-75), T = Real or Dual
struct Dual { Real v, e; };   // utils/DualNumbers.H:13-43
inline Dual operator+ (Dual a, Dual b) { return {a.v + b.v, a.e + b.e}; }
inline Dual operator- (Dual a, Dual b) { return {a.v - b.v, a.e - b.e}; }
inline Dual operator* (Dual a, Dual b) { return {a.v*b.v, a.e*b.v + a.v*b.e}; }
inline Dual D (Real a) { return {a, 0.0}; }

template <class T> struct Lift;
template <> struct Lift<Real> { static Real of (Real a) { return a; } };
template <> struct Lift<Dual> { static Dual of (Real a) { return D(a); } };

template <class T>
void momentum_push (const T& ux, const T& uy, const T& psi_inv, Real ExmBy, Real EypBx, Real Ez,
                    Real Bx_c, Real By_c, Real Bz, Real Aabssq, Real ADx, Real ADy,
                    Real clight_inv, Real qmc, T& dz_ux, T& dz_uy, T& dz_psi)
{
    auto L = [] (Real a) { return Lift<T>::of(a); };
    const T gamma_psi = L(0.5)*psi_inv*psi_inv*(
                        L(1.0 + Aabssq)
                        + ux*ux*L(clight_inv*clight_inv)
                        + uy*uy*L(clight_inv*clight_inv))
                        + L(0.5);
    dz_ux = (L(qmc)*(gamma_psi*L(ExmBy) + L(By_c) + (uy*L(Bz))*psi_inv) - L(ADx)*psi_inv);
    dz_uy = (L(qmc)*(gamma_psi*L(EypBx) - L(Bx_c) - (ux*L(Bz))*psi_inv) - L(ADy)*psi_inv);
    dz_psi = (L(qmc*clight_inv)*((ux*L(ExmBy) + uy*L(EypBx))*L(clight_inv)*psi_inv - L(Ez)));
}

// EnforceBC (particles/pusher/GetAndSetPosition.H:29-99); returns true if invalidated
bool enforce_bc (const Geom& gm, Real& x, Real& y, Real& ux, Real& uy, Real& w, int32_t& valid)
{
    if (x < gm.plo[0] || y < gm.plo[1] || x > gm.phi[0] || y > gm.phi[1]) {
        const Real len_x = gm.phi[0] - gm.plo[0];
        const Real len_y = gm.phi[1] - gm.plo[1];
        if (gm.bc == 0) {
            x = std::fmod(x - gm.plo[0], 2*len_x);
            if (x < 0) x += 2*len_x;
            x += gm.plo[0];
            if (x > gm.phi[0]) { x = 2*gm.phi[0] - x; ux = -ux; }
            y = std::fmod(y - gm.plo[1], 2*len_y);
            if (y < 0) y += 2*len_y;
            y += gm.plo[1];
            if (y > gm.phi[1]) { y = 2*gm.phi[1] - y; uy = -uy; }
            return false;
        } else if (gm.bc == 1) {
            x = std::fmod(x - gm.plo[0], len_x);
            if (x < 0) x += len_x;
            x += gm.plo[0];
            y = std::fmod(y - gm.plo[1], len_y);
            if (y < 0) y += len_y;
            y += gm.plo[1];
            return false;
        } else {
            w = 0.0; valid = 0;
            return true;
        }
    }
    return false;
}

// ---------------------------------------------------------------------------------------------
// AdvancePlasmaParticles, leapfrog pusher   particles/pusher/PlasmaParticleAdvance.cpp:92-217
// comp = {Psi, Ez, Bx, By, Bz}
// ---------------------------------------------------------------------------------------------
void advance_plasma (const Slab& f, const Plasma& pl, const Geom& gm, const int* comp,
                     Real charge, Real mass, int order, int temp_slice, int n_subcycles,
                     int can_ionize, int aabs_comp = -1)
{
    const Real laser_norm = (charge/gm.q_e)*(gm.m_e/mass)*(charge/gm.q_e)*(gm.m_e/mass);      // (:77-78)
    const Real dx_inv = 1.0/gm.dx, dy_inv = 1.0/gm.dy;
    const Real dz = gm.dz/n_subcycles;
    const Real clight = gm.c, clight_inv = 1.0/gm.c;
    const Real charge_mass_clight_ratio = charge/(mass*gm.c);
#pragma omp parallel for num_threads(g_threads) schedule(static) if(g_threads > 1)
    for (long ip = 0; ip < pl.n; ++ip) {
        if (!pl.valid[ip]) continue;
        Real ExmByp = 0, EypBxp = 0, Ezp = 0, Bxp = 0, Byp = 0, Bzp = 0;
        Real Aabssqp = 0, AabssqDxp = 0, AabssqDyp = 0;
        Real qmc = charge_mass_clight_ratio;
        Real laser_norm_ion = laser_norm;
        if (can_ionize) { qmc *= pl.ion_lev[ip]; laser_norm_ion *= (Real)pl.ion_lev[ip]*pl.ion_lev[ip]; }
        bool dead = false;
        for (int isc = 0; isc < n_subcycles && !dead; ++isc) {
            Real xp = pl.x_prev[ip];
            Real yp = pl.y_prev[ip];
            ExmByp = 0; EypBxp = 0; Ezp = 0; Bxp = 0; Byp = 0; Bzp = 0;
            gather(order, xp, yp, ExmByp, EypBxp, Ezp, Bxp, Byp, Bzp, f, comp,
                   dx_inv, dy_inv, gm.xoff, gm.yoff);
            Bxp *= clight;
            Byp *= clight;
            if (aabs_comp >= 0) {       // (:121-131)
                Aabssqp = 0; AabssqDxp = 0; AabssqDyp = 0;
                laser_gather(order, xp, yp, f, aabs_comp, dx_inv, dy_inv, gm.xoff, gm.yoff, Aabssqp, &AabssqDxp, &AabssqDyp);
                Aabssqp *= 0.5*laser_norm_ion;
                AabssqDxp *= 0.25*clight*laser_norm_ion;
                AabssqDyp *= 0.25*clight*laser_norm_ion;
            }

            const int nsub = 4;
            const Real sdz = dz/nsub;
            Real ux = pl.ux_half[ip];
            Real uy = pl.uy_half[ip];
            Real psi = pl.psi_half[ip];

            auto substep = [&] () {
                const Real psi_inv = 1.0/psi;
                Real dz_ux, dz_uy, dz_psi;
                momentum_push<Real>(ux, uy, psi_inv, ExmByp, EypBxp, Ezp, Bxp, Byp, Bzp,
                                    Aabssqp, AabssqDxp, AabssqDyp, clight_inv, qmc,
                                    dz_ux, dz_uy, dz_psi);
                const Dual ux_d{ux, dz_ux};
                const Dual uy_d{uy, dz_uy};
                const Dual psi_inv_d{psi_inv, -psi_inv*psi_inv*dz_psi};
                Dual ddx, ddy, ddp;
                momentum_push<Dual>(ux_d, uy_d, psi_inv_d, ExmByp, EypBxp, Ezp, Bxp, Byp, Bzp,
                                    Aabssqp, AabssqDxp, AabssqDyp, clight_inv, qmc,
                                    ddx, ddy, ddp);
                ux += sdz*dz_ux + 0.5*sdz*sdz*ddx.e;
                uy += sdz*dz_uy + 0.5*sdz*sdz*ddy.e;
                psi += sdz*dz_psi + 0.5*sdz*sdz*ddp.e;
            };

            for (int isub = 0; isub < nsub; ++isub) substep();

            xp += dz*clight_inv*(ux*(1.0/psi));
            yp += dz*clight_inv*(uy*(1.0/psi));

            if (enforce_bc(gm, xp, yp, ux, uy, pl.w[ip], pl.valid[ip])) { dead = true; break; }
            pl.x[ip] = xp;
            pl.y[ip] = yp;

            if (!temp_slice) {
                pl.ux_half[ip] = ux;
                pl.uy_half[ip] = uy;
                pl.psi_half[ip] = psi;
                pl.x_prev[ip] = xp;
                pl.y_prev[ip] = yp;
            }

            for (int isub = 0; isub < nsub/2; ++isub) substep();

            pl.ux[ip] = ux;
            pl.uy[ip] = uy;
            pl.psi[ip] = psi;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// DST-I Poisson solve  fields/fft_poisson_solver/FFTPoissonSolverDirichletDirect.cpp:51-139
// (FFTW RODFT00 convention, WrapFFTW.cpp:77-82), here via an own mixed-radix FFT of the odd
// extension.  Cross-checked against scipy.fft.dstn(type=1) in tests/test_oracle_ops.py.
// ---------------------------------------------------------------------------------------------
typedef std::complex<double> cplx;

void fft_rec (int n, int stride, const cplx* in, cplx* out, const std::vector<cplx>& tw, int ntw)
{
    // out[k], k<n = sum_m in[m*stride] * W_n^{mk};  tw[k] = exp(-2 pi i k/ntw), ntw % n == 0
    if (n == 1) { out[0] = in[0]; return; }
    int p = 2;
    while (n % p != 0) { ++p; if (p*p > n) { p = n; break; } }
    if (n % p != 0) p = n;
    const int m = n/p;
    if (m == 1) {
        for (int k = 0; k < n; ++k) {
            cplx s = 0;
            for (int r = 0; r < n; ++r) s += in[(long)r*stride]*tw[((long)r*k % n)*(ntw/n)];
            out[k] = s;
        }
        return;
    }
    std::vector<cplx> sub((size_t)n);
    for (int r = 0; r < p; ++r) fft_rec(m, stride*p, in + (long)r*stride, sub.data() + (long)r*m, tw, ntw);
    for (int k = 0; k < n; ++k) {
        const int km = k % m;
        cplx s = 0;
        for (int r = 0; r < p; ++r) s += sub[(long)r*m + km]*tw[((long)r*k % n)*(ntw/n)];
        out[k] = s;
    }
}

struct DstPlan {
    int n; int N2; std::vector<cplx> tw; std::vector<cplx> a, b;
    explicit DstPlan (int n_) : n(n_), N2(2*(n_+1)), tw((size_t)N2), a((size_t)N2), b((size_t)N2) {
        for (int k = 0; k < N2; ++k) {
            const double ang = -2.0*M_PI*k/N2;
            tw[k] = cplx(std::cos(ang), std::sin(ang));
        }
    }
    // in-place RODFT00: X_k = 2 sum_j x_j sin(pi (j+1)(k+1)/(n+1)), strided
    void apply (double* x, long stride) { apply_with(x, stride, a, b); }
    void apply_with (double* x, long stride, std::vector<cplx>& a, std::vector<cplx>& b) const {
        a[0] = 0; a[n+1] = 0;
        for (int j = 0; j < n; ++j) { a[j+1] = x[j*stride]; a[N2-1-j] = -x[j*stride]; }
        fft_rec(N2, 1, a.data(), b.data(), tw, N2);
        for (int k = 0; k < n; ++k) x[k*stride] = -b[k+1].imag();
    }
    // all `count` transforms of a pass (x + q*step, element stride `stride`); threads own whole transforms
    void apply_many (double* x, long stride, long step, int count) {
        if (g_threads <= 1) { for (int q = 0; q < count; ++q) apply(x + q*step, stride); return; }
#pragma omp parallel num_threads(g_threads)
        {
            std::vector<cplx> ta((size_t)N2), tb((size_t)N2);
#pragma omp for schedule(static)
            for (int q = 0; q < count; ++q) apply_with(x + q*step, stride, ta, tb);
        }
    }
};

struct PoissonSolver {
    int nx, ny; std::vector<double> eig; DstPlan px, py;
    PoissonSolver (int nx_, int ny_, double dx, double dy)
        : nx(nx_), ny(ny_), eig((size_t)nx_*ny_), px(nx_), py(ny_)
    {
        // eigenvalues incl. normalisation (…DirichletDirect.cpp:58-83)
        const double dxsq = dx*dx, dysq = dy*dy;
        const double sxf = M_PI/(2.*(nx + 1)), syf = M_PI/(2.*(ny + 1));
        const double norm_fac = 0.5/(2*((nx + 1)*(ny + 1)));
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
            const double sx2 = std::sin((i + 1)*sxf)*std::sin((i + 1)*sxf);
            const double sy2 = std::sin((j + 1)*syf)*std::sin((j + 1)*syf);
            eig[(size_t)j*nx + i] = (sx2 != 0 && sy2 != 0)
                ? norm_fac/(-4.0*(sx2/dxsq + sy2/dysq)) : 0.0;
        }
    }
    // staging (nx*ny, x fastest) is overwritten with the solution
    void solve (double* st) {
        bool all_zero = true;   // exact shortcut: a zero source has the zero solution
        for (size_t k = 0; k < (size_t)nx*ny && all_zero; ++k) all_zero = (st[k] == 0.0);
        if (all_zero) return;
        px.apply_many(st, 1, nx, ny);
        py.apply_many(st, nx, 1, nx);
        for (size_t k = 0; k < (size_t)nx*ny; ++k) st[k] *= eig[k];
        px.apply_many(st, 1, nx, ny);
        py.apply_many(st, nx, 1, nx);
    }
};

// ---------------------------------------------------------------------------------------------
// hpmg::MultiGrid, system types 1 and 2     mg_solver/HpMultiGrid.cpp (CPU path)
//   type 1: -acoef*sol + Lap(sol) = rhs, homogeneous Dirichlet, sol/rhs 2 comps, acoef 1 comp
//   type 2: -(ar + i ai)(sol_r + i sol_i) + Lap(sol_r + i sol_i) = rhs_r + i rhs_i, acoef 2 comps (laser envelope)
// gsrb_cached (:595-740) is an exact re-expression of 4 global red-black sweeps (+ residual),
// so it is restated as global sweeps (gsrb :367-407, gs1 :265-292, residual1 :184-190).
// ---------------------------------------------------------------------------------------------
struct MGLevel {
    int lox, loy, hix, hiy;   // index bounds of the level box (incl. boundary nodes if nodal)
    int nxb, nyb;             // box lengths
    std::vector<double> acf, res, cor, rescor;   // acf 1 comp (type 2: 2 comps); others 2 comps
    long idx (int i, int j) const { return (long)(i - lox) + (long)(j - loy)*nxb; }
    long csz () const { return (long)nxb*nyb; }
};

struct MG {
    bool cc; double dx, dy; int nlev; std::vector<MGLevel> L; int sys = 1;
    // external arrays for level 0 (user memory, arbitrary strides, index origin shift)
    double *sol0, *sol1; const double *rhs0, *rhs1; long ext_js; int ext_shift_i, ext_shift_j;

    MG (int nx, int ny, double dx_, double dy_, int system_type = 1) : dx(dx_), dy(dy_), sys(system_type) {
        // ctor / level build (HpMultiGrid.cpp:1043-1072)
        cc = (nx % 2 == 0);
        int lx = nx, ly = ny;   // cc: number of cells; nodal: box is 0..n+1 => n+2 nodes
        int hx = cc ? nx - 1 : nx + 1, hy = cc ? ny - 1 : ny + 1;
        (void)lx; (void)ly;
        for (int il = 0; il < 31; ++il) {
            MGLevel lev; lev.lox = 0; lev.loy = 0; lev.hix = hx; lev.hiy = hy;
            lev.nxb = hx + 1; lev.nyb = hy + 1;
            lev.acf.assign((size_t)lev.csz()*sys, 0.0);
            lev.res.assign((size_t)lev.csz()*2, 0.0);
            lev.cor.assign((size_t)lev.csz()*2, 0.0);
            lev.rescor.assign((size_t)lev.csz()*2, 0.0);
            L.push_back(std::move(lev));
            // coarsenable(2, min_width) (:1065-1072)
            bool ok;
            if (cc) {
                const int nxl = hx + 1, nyl = hy + 1;
                ok = nxl >= 4 && nyl >= 4 && nxl % 2 == 0 && nyl % 2 == 0;
                if (ok) { hx = nxl/2 - 1; hy = nyl/2 - 1; }
            } else {
                const int nxl = hx + 1, nyl = hy + 1;   // number of nodes
                ok = nxl >= 8 && nyl >= 8 && hx % 2 == 0 && hy % 2 == 0;
                if (ok) { hx = hx/2; hy = hy/2; }
            }
            if (!ok) break;
        }
        nlev = (int)L.size();
    }

    // valid_domain_box (:20-23)
    void valid (const MGLevel& l, int& il, int& jl, int& ih, int& jh) const {
        if (cc) { il = l.lox; jl = l.loy; ih = l.hix; jh = l.hiy; }
        else    { il = l.lox + 1; jl = l.loy + 1; ih = l.hix - 1; jh = l.hiy - 1; }
    }

    struct View { double* p; long js; long ns; int oi, oj;   // p(i,j,n)
        double& operator() (int i, int j, int n) const { return p[(i + oi) + (long)(j + oj)*js + n*ns]; } };
    struct CView { const double* p; long js; long ns; int oi, oj;
        const double& operator() (int i, int j, int n) const { return p[(i + oi) + (long)(j + oj)*js + n*ns]; } };

    View lv (MGLevel& l, std::vector<double>& a) const { return {a.data(), l.nxb, l.csz(), 0, 0}; }
    CView clv (const MGLevel& l, const std::vector<double>& a) const { return {a.data(), l.nxb, l.csz(), 0, 0}; }

    // gs1 (:265-292)
    inline void gs1 (int i, int j, int n, const MGLevel& l, const View& phi, double rhs,
                     double acf, double facx, double facy) const {
        double lap;
        double c0 = -(acf + 2.0*(facx + facy));
        if (cc && i == l.lox)      { lap = facx*(4./3.)*phi(i+1,j,n); c0 -= 2.0*facx; }
        else if (cc && i == l.hix) { lap = facx*(4./3.)*phi(i-1,j,n); c0 -= 2.0*facx; }
        else                       { lap = facx*(phi(i-1,j,n) + phi(i+1,j,n)); }
        if (cc && j == l.loy)      { lap += facy*(4./3.)*phi(i,j+1,n); c0 -= 2.0*facy; }
        else if (cc && j == l.hiy) { lap += facy*(4./3.)*phi(i,j-1,n); c0 -= 2.0*facy; }
        else                       { lap += facy*(phi(i,j-1,n) + phi(i,j+1,n)); }
        const double c0_inv = 1.0/c0;
        phi(i,j,n) = (rhs - lap)*c0_inv;
    }
    // gs2 (:296-334): the 2x2 system of the real and the imaginary part solved at once
    inline void gs2 (int i, int j, const MGLevel& l, const View& phi, double rhs_r, double rhs_i,
                     double ar, double ai, double facx, double facy) const {
        double lap[2];
        double c0 = -2.0*(facx + facy);
        if (cc && i == l.lox)      { lap[0] = facx*(4./3.)*phi(i+1,j,0); lap[1] = facx*(4./3.)*phi(i+1,j,1); c0 -= 2.0*facx; }
        else if (cc && i == l.hix) { lap[0] = facx*(4./3.)*phi(i-1,j,0); lap[1] = facx*(4./3.)*phi(i-1,j,1); c0 -= 2.0*facx; }
        else { lap[0] = facx*(phi(i-1,j,0) + phi(i+1,j,0)); lap[1] = facx*(phi(i-1,j,1) + phi(i+1,j,1)); }
        if (cc && j == l.loy)      { lap[0] += facy*(4./3.)*phi(i,j+1,0); lap[1] += facy*(4./3.)*phi(i,j+1,1); c0 -= 2.0*facy; }
        else if (cc && j == l.hiy) { lap[0] += facy*(4./3.)*phi(i,j-1,0); lap[1] += facy*(4./3.)*phi(i,j-1,1); c0 -= 2.0*facy; }
        else { lap[0] += facy*(phi(i,j-1,0) + phi(i,j+1,0)); lap[1] += facy*(phi(i,j-1,1) + phi(i,j+1,1)); }
        double c[2] = {c0 - ar, -ai};
        const double cmag = 1.0/(c[0]*c[0] + c[1]*c[1]);
        c[0] *= cmag; c[1] *= cmag;
        phi(i,j,0) = (rhs_r - lap[0])*c[0] + (rhs_i - lap[1])*c[1];
        phi(i,j,1) = (rhs_i - lap[1])*c[0] - (rhs_r - lap[0])*c[1];
    }
    // one point of a sweep / of the residual for either system type
    inline void gs_point (int i, int j, const MGLevel& l, const View& phi, const CView& rhs, const CView& acf,
                          double facx, double facy) const {
        if (sys == 1) { gs1(i, j, 0, l, phi, rhs(i,j,0), acf(i,j,0), facx, facy); gs1(i, j, 1, l, phi, rhs(i,j,1), acf(i,j,0), facx, facy); }
        else gs2(i, j, l, phi, rhs(i,j,0), rhs(i,j,1), acf(i,j,0), acf(i,j,1), facx, facy);
    }
    inline void res_point (int i, int j, const MGLevel& l, const View& phi, const CView& rhs, const CView& acf,
                           double facx, double facy, double& r0, double& r1) const {
        if (sys == 1) {
            r0 = residual1(i, j, 0, l, phi, rhs(i,j,0), acf(i,j,0), facx, facy);
            r1 = residual1(i, j, 1, l, phi, rhs(i,j,1), acf(i,j,0), facx, facy);
        } else {      // residual2r, residual2i (:192-208)
            const double ar = acf(i,j,0), ai = acf(i,j,1);
            r0 = residual1(i, j, 0, l, phi, rhs(i,j,0), 0.0, facx, facy) + (ar*phi(i,j,0) - ai*phi(i,j,1));
            r1 = residual1(i, j, 1, l, phi, rhs(i,j,1), 0.0, facx, facy) + (ai*phi(i,j,0) + ar*phi(i,j,1));
        }
    }
    // laplacian (:162-182) + residual1 (:184-190)
    inline double residual1 (int i, int j, int n, const MGLevel& l, const View& phi, double rhs,
                             double acf, double facx, double facy) const {
        double lap = -2.0*(facx + facy)*phi(i,j,n);
        if (i == l.lox)      lap += facx*((4./3.)*phi(i+1,j,n) - 2.0*phi(i,j,n));
        else if (i == l.hix) lap += facx*((4./3.)*phi(i-1,j,n) - 2.0*phi(i,j,n));
        else                 lap += facx*(phi(i-1,j,n) + phi(i+1,j,n));
        if (j == l.loy)      lap += facy*((4./3.)*phi(i,j+1,n) - 2.0*phi(i,j,n));
        else if (j == l.hiy) lap += facy*((4./3.)*phi(i,j-1,n) - 2.0*phi(i,j,n));
        else                 lap += facy*(phi(i,j-1,n) + phi(i,j+1,n));
        return rhs + acf*phi(i,j,n) - lap;
    }

    // gsrb_4_residual<zero_init, do_residual> (:742-848): phi_out = gsrb^4(phi_in or 0); res
    void gsrb4 (int ilev, bool zero_init, bool do_res, const View& phi_out, const CView& rhs,
                const View* res, const CView* phi_in, double ldx, double ldy) {
        MGLevel& l = L[ilev];
        int il, jl, ih, jh; valid(l, il, jl, ih, jh);
        const double facx = 1.0/(ldx*ldx), facy = 1.0/(ldy*ldy);
        const CView acf = clv(l, l.acf);
        // work on a private zero-padded copy so phi_out's non-valid entries stay untouched
        const int wx = l.nxb + 2, wy = l.nyb + 2;
        std::vector<double> wbuf((size_t)wx*wy*2, 0.0);
        View w{wbuf.data(), wx, (long)wx*wy, 1 - l.lox, 1 - l.loy};
        if (!zero_init) {
            for (int n = 0; n < 2; ++n) for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i)
                w(i,j,n) = (*phi_in)(i,j,n);
        }
        const bool par = g_threads > 1 && (long)(ih - il + 1)*(jh - jl + 1) >= 4096;
        for (int icolor = 0; icolor < 4; ++icolor) {
            // cells of one colour do not read each other: rows can go to different threads, same result
#pragma omp parallel for num_threads(g_threads) schedule(static) if(par)
            for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
                if ((i + j + icolor) % 2 == 0) gs_point(i, j, l, w, rhs, acf, facx, facy);
            }
        }
#pragma omp parallel for num_threads(g_threads) schedule(static) if(par)
        for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
            if (do_res) res_point(i, j, l, w, rhs, acf, facx, facy, (*res)(i,j,0), (*res)(i,j,1));
            phi_out(i,j,0) = w(i,j,0);
            phi_out(i,j,1) = w(i,j,1);
        }
    }

    // plain sweep used by the CPU bottom solve (gsrb :367-407)
    void gsrb_sweep (int ilev, int icolor, const View& phi, const CView& rhs, double ldx, double ldy) {
        MGLevel& l = L[ilev];
        int il, jl, ih, jh; valid(l, il, jl, ih, jh);
        const double facx = 1.0/(ldx*ldx), facy = 1.0/(ldy*ldy);
        const CView acf = clv(l, l.acf);
        for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
            if ((i + j + icolor) % 2 == 0) gs_point(i, j, l, phi, rhs, acf, facx, facy);
        }
    }

    // restriction (:123-138; restrict_cc :29-37, restrict_nd :39-52)
    void restriction (int ic, std::vector<double>& crse_a, const std::vector<double>& fine_a, int ncomp) {
        MGLevel& c = L[ic]; const MGLevel& f = L[ic-1];
        int il, jl, ih, jh; valid(c, il, jl, ih, jh);
        View crse{crse_a.data(), c.nxb, c.csz(), 0, 0};
        CView fine{fine_a.data(), f.nxb, f.csz(), 0, 0};
#pragma omp parallel for collapse(2) num_threads(g_threads) schedule(static) if(g_threads > 1 && (long)(ih - il + 1)*(jh - jl + 1) >= 4096)
        for (int n = 0; n < ncomp; ++n) for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
            if (cc) {
                crse(i,j,n) = 0.25*(fine(2*i,2*j,n) + fine(2*i+1,2*j,n) + fine(2*i,2*j+1,n) + fine(2*i+1,2*j+1,n));
            } else {
                crse(i,j,n) = (1./16.)*(fine(2*i-1,2*j-1,n) + 2.*fine(2*i,2*j-1,n) + fine(2*i+1,2*j-1,n)
                                      + 2.*fine(2*i-1,2*j,n) + 4.*fine(2*i,2*j,n) + 2.*fine(2*i+1,2*j,n)
                                      + fine(2*i-1,2*j+1,n) + 2.*fine(2*i,2*j+1,n) + fine(2*i+1,2*j+1,n));
            }
        }
    }

    static int coarsen2 (int i) { return (i < 0) ? -((-i + 1)/2) : i/2; }

    // interpolation_outofplace (:140-156; interpcpy_cc :88-95, interpcpy_nd :97-121)
    void interp_copy (int ilev) {
        MGLevel& f = L[ilev]; MGLevel& c = L[ilev+1];
        int il, jl, ih, jh; valid(f, il, jl, ih, jh);
        CView fin = clv(f, f.cor); CView crse = clv(c, c.cor); View fout = lv(f, f.rescor);
#pragma omp parallel for collapse(2) num_threads(g_threads) schedule(static) if(g_threads > 1 && (long)(ih - il + 1)*(jh - jl + 1) >= 4096)
        for (int n = 0; n < 2; ++n) for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
            const int ic = coarsen2(i), jc = coarsen2(j);
            if (cc) {
                fout(i,j,n) = fin(i,j,n) + crse(ic,jc,n);
            } else {
                const bool io = (ic*2 != i), jo = (jc*2 != j);
                if (io && jo)  fout(i,j,n) = fin(i,j,n) + (crse(ic,jc,n) + crse(ic+1,jc,n) + crse(ic,jc+1,n) + crse(ic+1,jc+1,n))*0.25;
                else if (io)   fout(i,j,n) = fin(i,j,n) + (crse(ic,jc,n) + crse(ic+1,jc,n))*0.5;
                else if (jo)   fout(i,j,n) = fin(i,j,n) + (crse(ic,jc,n) + crse(ic,jc+1,n))*0.5;
                else           fout(i,j,n) = fin(i,j,n) + crse(ic,jc,n);
            }
        }
    }

    View solv () const { return {sol0, ext_js, (long)(sol1 - sol0), ext_shift_i, ext_shift_j}; }
    CView rhsv () const { return {rhs0, ext_js, (long)(rhs1 - rhs0), ext_shift_i, ext_shift_j}; }

    // vcycle (:1429-1512), CPU: m_single_block_level_begin == m_max_level
    void vcycle () {
        const int maxl = nlev - 1;
        for (int il = 0; il < maxl; ++il) {
            const double fac = (double)(1 << il);
            if (il > 0) {
                View cor = lv(L[il], L[il].cor); View rc = lv(L[il], L[il].rescor);
                gsrb4(il, true, true, cor, clv(L[il], L[il].res), &rc, nullptr, dx*fac, dy*fac);
            }
            restriction(il + 1, L[il+1].res, L[il].rescor, 2);
        }
        bottomsolve();
        for (int il = maxl - 1; il >= 0; --il) {
            const double fac = (double)(1 << il);
            interp_copy(il);
            CView pin = clv(L[il], L[il].rescor);
            if (il == 0) gsrb4(0, false, false, solv(), rhsv(), nullptr, &pin, dx*fac, dy*fac);
            else { View cor = lv(L[il], L[il].cor);
                   gsrb4(il, false, false, cor, clv(L[il], L[il].res), nullptr, &pin, dx*fac, dy*fac); }
        }
        View cor0 = lv(L[0], L[0].cor); View rc0 = lv(L[0], L[0].rescor);
        View s = solv(); CView sin{s.p, s.js, s.ns, s.oi, s.oj};
        gsrb4(0, false, true, cor0, rhsv(), &rc0, &sin, dx, dy);
    }

    // bottomsolve, CPU branch (:1583-1593)
    void bottomsolve () {
        const int il = nlev - 1;
        const double fac = (double)(1 << il);
        std::fill(L[il].cor.begin(), L[il].cor.end(), 0.0);
        const int nsweeps = 16;
        const int numsweeps = std::max(nsweeps, (std::max(L[il].nxb, L[il].nyb) + 1)/2*2);
        View cor = lv(L[il], L[il].cor);
        for (int is = 0; is < numsweeps; ++is) gsrb_sweep(il, is, cor, clv(L[il], L[il].res), dx*fac, dy*fac);
    }

    // average_down_acoef (:1640-1700)
    void average_down_acoef () {
        for (int il = 1; il < nlev; ++il) restriction(il, L[il].acf, L[il-1].acf, sys);
    }

    // solve1 (:1169-1190) + solve_doit (:1307-1427).  Arrays are slab components with guards:
    // p(i,j) = base[(i+g) + (j+g)*js].  Returns number of V-cycles, or -1 on failure.
    int solve1 (double* sol_c0, double* sol_c1, const double* rhs_c0, const double* rhs_c1,
                const double* acf_c, long js, int g, double tol_rel, double tol_abs, int maxiter,
                double* resnorm_out) {
        // center_box (HpMultiGrid.H:168-175): user cell i -> level index i + sh
        const int sh = cc ? 0 : 1;
        sol0 = sol_c0; sol1 = sol_c1; rhs0 = rhs_c0; rhs1 = rhs_c1; ext_js = js;
        ext_shift_i = g - sh; ext_shift_j = g - sh;
        MGLevel& l0 = L[0];
        for (int j = l0.loy; j <= l0.hiy; ++j) for (int i = l0.lox; i <= l0.hix; ++i)
            l0.acf[l0.idx(i,j)] = acf_c[(i - sh + g) + (long)(j - sh + g)*js];
        average_down_acoef();
        return solve_doit(tol_rel, tol_abs, maxiter, resnorm_out);
    }

    // solve2 (:1239-1262): acoef_real an array, acoef_imag a scalar (the laser envelope solve); same array conventions
    int solve2 (double* sol_c0, double* sol_c1, const double* rhs_c0, const double* rhs_c1,
                const double* acf_real, double acf_imag, long js, int g, double tol_rel, double tol_abs, int maxiter,
                double* resnorm_out) {
        const int sh = cc ? 0 : 1;
        sol0 = sol_c0; sol1 = sol_c1; rhs0 = rhs_c0; rhs1 = rhs_c1; ext_js = js;
        ext_shift_i = g - sh; ext_shift_j = g - sh;
        MGLevel& l0 = L[0];
        for (int j = l0.loy; j <= l0.hiy; ++j) for (int i = l0.lox; i <= l0.hix; ++i) {
            const bool in = cc || (i >= 1 && i <= l0.hix - 1 && j >= 1 && j <= l0.hiy - 1);
            l0.acf[l0.idx(i,j)] = in ? acf_real[(i - sh + g) + (long)(j - sh + g)*js] : 0.0;
            l0.acf[l0.csz() + l0.idx(i,j)] = acf_imag;
        }
        average_down_acoef();
        return solve_doit(tol_rel, tol_abs, maxiter, resnorm_out);
    }

    // solve_doit (:1307-1427)
    int solve_doit (double tol_rel, double tol_abs, int maxiter, double* resnorm_out) {
        MGLevel& l0 = L[0];
        View cor0 = lv(l0, l0.cor); View rc0 = lv(l0, l0.rescor);
        View s = solv(); CView sin{s.p, s.js, s.ns, s.oi, s.oj};
        gsrb4(0, false, true, cor0, rhsv(), &rc0, &sin, dx, dy);

        int il, jl, ih, jh; valid(l0, il, jl, ih, jh);
        double resnorm0 = 0, rhsnorm0 = 0;
        { CView r = rhsv();
          for (int n = 0; n < 2; ++n) for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i) {
              resnorm0 = std::max(resnorm0, std::abs(rc0(i,j,n)));
              rhsnorm0 = std::max(rhsnorm0, std::abs(r(i,j,n)));
          } }
        const double max_norm = (rhsnorm0 >= resnorm0) ? rhsnorm0 : resnorm0;
        const double res_target = std::max(tol_abs, std::max(tol_rel, 1.e-16)*max_norm);
        int iters = 0;
        double norminf = resnorm0;
        if (resnorm0 > res_target) {
            bool converged = true;
            for (int iter = 0; iter < maxiter; ++iter) {
                converged = false;
                vcycle();
                ++iters;
                norminf = 0;
                for (size_t k = 0; k < l0.rescor.size(); ++k) norminf = std::max(norminf, std::abs(l0.rescor[k]));
                converged = (norminf <= res_target);
                if (converged) break;
                if (norminf > 1.e20*max_norm) return -1;
            }
            if (!converged) return -1;
        }
        View so = solv();
        for (int n = 0; n < 2; ++n) for (int j = jl; j <= jh; ++j) for (int i = il; i <= ih; ++i)
            so(i,j,n) = cor0(i,j,n);
        if (resnorm_out) *resnorm_out = norminf;
        return iters;
    }
};

// ---------------------------------------------------------------------------------------------
// Slice engine: slab bookkeeping + SolveOneSlice for the explicit solver
// ---------------------------------------------------------------------------------------------

// Explicit-mode component order (fields/Fields.cpp:70-122), without laser / chi2 / salame
enum Comp { N_jxb = 0, N_jyb, chi, Sy, Sx, ExmBy, EypBx, Ez, Bx, By, Bz, Psi,
            jxb, jyb, jzb, jx, jy, rhomjz, P_jxb, P_jyb, Ion_rhomjz, rho /* optional */, NCOMP_MAX };

// Predictor-corrector component order (fields/Fields.cpp:128-164): Next{jx,jy}, This{ExmBy,EypBx,Ez,Bx,By,Bz,Psi,
// jx,jy,jz,rhomjz}, Previous{Bx,By,jx,jy}, RhomJzIons{rhomjz}, PCIter{Bx,By}, PCPrevIter{Bx,By}; optional rho last
enum PcComp { pN_jx = 0, pN_jy, pExmBy, pEypBx, pEz, pBx, pBy, pBz, pPsi, pjx, pjy, pjz, prhomjz,
              pP_Bx, pP_By, pP_jx, pP_jy, pIon_rhomjz, pIt_Bx, pIt_By, pPIt_Bx, pPIt_By, prho /* optional */, PC_NCOMP_MAX };

struct Deck {
    int nx, ny, nz; double lo[3], hi[3]; int order; int deriv_type;
    int plasma_ppc[2]; double plasma_density; double plasma_radius;  // radius<=0 -> infinity
    double plasma_charge, plasma_mass; double max_qsa; int n_subcycles;
    int beam_profile;           // -1 none, 0 gaussian, 1 flattop
    double beam_zmin, beam_zmax, beam_radius, beam_density;
    double beam_umean[3], beam_pos_mean[3], beam_pos_std[3]; int beam_ppc[3];
    double beam_charge;
    int bc;                      // particle boundary
    double mg_tol_rel, mg_tol_abs;
    int deposit_rho;
    int n_steps;                 // max_step + 1 (dt = 0: every step identical)
    double dt;                   // hipace.dt: 0 = the beam is never pushed
    int beam_n_subcycles;        // beam.n_subcycles (BeamParticleContainer.H:222, default 10)
    double beam_mass;
    double ext_E_slope[2];       // beams.external_E = (s0*x, s1*y, 0): the only external field form restated
    int bxby_solver;             // 0 explicit (Hipace.H:244 default), 1 predictor-corrector
    double predcorr_tol;         // hipace.predcorr_B_error_tolerance (Hipace.H:210, 4e-2)
    int predcorr_max_iter;       // hipace.predcorr_max_iterations (Hipace.H:213, 30)
    double predcorr_mix;         // hipace.predcorr_B_mixing_factor (Hipace.H:222, 0.05)
    int field_bc;                // boundary.field: 0 Dirichlet, 1 Open (oracle only: pins the predictor-corrector
                                 // path on beam_in_vacuum_open_boundary.normalized.1Rank.json)
    // Gaussian laser envelope (laser/Laser.H:32-45, MultiLaser.cpp:881-919), static: only step 0 is restated (the
    // envelope solver that advances it to the next time step is not), explicit solver only
    int laser_on; double laser_a0, laser_w0, laser_L0, laser_lambda0, laser_pos[3];
    int si_units;                // hipace.normalized_units = 0: PhysConst of utils/Constants.H:15-24, weights are charges
    double laser_zfoc;           // laser.focal_distance (Laser.H:43)
    int laser_solver;            // lasers.solver_type: 0 = envelope kept static, 1 = "fft" (MultiLaser::AdvanceSliceFFT),
                                 // 2 = "multigrid" (MultiLaser::AdvanceSliceMG, MG_average_rhs = 1)
    double laser_mg_tol_rel = 1.e-4, laser_mg_tol_abs = 0.0;      // lasers.MG_tolerance_rel / _abs (MultiLaser.H:216-217)
    int beam_radiation_reaction = 0; double background_density_SI = 0.0; int beam_no_z_push = 0;
    int laser_use_phase;         // lasers.use_phase (MultiLaser.H:203, default true)
    int grid_current_on = 0;     // grid_current.use_grid_current (utils/GridCurrent.cpp:13-23)
    double grid_current_peak = 0., grid_current_mean[3] = {0., 0., 0.}, grid_current_std[3] = {1., 1., 1.};
    // second plasma species "ion" with ADK field ionisation (ionization_product = the first species):
    // PlasmaParticleContainer.cpp:61-90 (element, mass_Da, initial_ion_level, can_ionize), PlasmaParticleContainerInit.cpp:382-464
    int plasma_no_neutralize = 0;      // <plasma>.neutralize_background = false for the first species
    int ion_on = 0; int ion_ppc[2] = {0, 0}; double ion_density = 0., ion_mass = 0., ion_charge = 0.;
    int ion_init_level = 0; int ion_Z = 0; double ion_energies[56] = {0.};       // eV, IonizationEnergiesTable.H (NIST)
    unsigned long long ion_seed = 0;   // counter-based generator (the reference draws from amrex::Random: sequence not reproducible)
    // <beam>.do_spin_tracking, initial_spin, spin_anom (BeamParticleContainer.cpp:105-109, .H:236-241)
    int beam_spin_tracking = 0; double beam_initial_spin[3] = {1., 0., 0.}; double beam_spin_anom = 0.00115965218128;
};

// particles of one beam slice; [0, nreg) were on the slice when the step began ("regular"), the rest slipped in
// from the slice ahead during this step (BeamParticleContainer.H:175-182)
struct Beam { std::vector<double> x, y, z, ux, uy, uz, w; std::vector<int> nsub; std::vector<int32_t> valid; long nreg = 0;
              std::vector<double> sx, sy, sz; };      // spin (<beam>.do_spin_tracking: three runtime real components)

struct Engine {
    Deck d; Geom gm; int g; int ncomp;
    std::vector<double> slab_data; Slab slab;
    std::vector<double> pdata; std::vector<int32_t> pvalid, pion; Plasma pl;
    long pl_cap = 0;                         // capacity of the first species' arrays (grows by ionisation)
    std::vector<double> idata; std::vector<int32_t> ivalid, ilev; std::vector<uint64_t> iuid; Plasma ipl;      // species "ion"
    std::vector<double> adk_prefactor, adk_exp_prefactor, adk_power;
    long n_ionized_total = 0; int cur_step = -1, next_step = -1;
    // plasma density profile n(x, y, ct) = density * f_r(sqrt(x^2 + y^2)) * f_t(c t), both piecewise linear tables (constant
    // beyond their ends); the tabulated stand-in of <plasma>.density(x,y,z) (PlasmaParticleContainerInit.cpp:246-313: the
    // function is evaluated per particle with z = c t; particles with density <= min_density = 0 are not created)
    std::vector<double> prof_r, prof_fr, prof_t, prof_ft;
    static double table (const std::vector<double>& x, const std::vector<double>& f, double v) {
        if (x.empty()) return 1.0;
        if (v <= x.front()) return f.front();
        if (v >= x.back()) return f.back();
        size_t k = 1;
        while (x[k] < v) ++k;
        const double t = (v - x[k-1])/(x[k] - x[k-1]);
        return f[k-1] + t*(f[k] - f[k-1]);
    }
    double profile (double x, double y) const {
        return table(prof_r, prof_fr, std::sqrt(x*x + y*y))*table(prof_t, prof_ft, gm.c*d.dt*std::max(cur_step, 0));
    }
    PoissonSolver* ps; MG* mg; std::vector<double> staging;
    Beam beam_this, beam_next; int beam_this_slice = -2;      // slice whose particles beam_this holds
    // dt != 0: the beam lives in per-slice stores across the time steps (index = islice)
    std::vector<Beam> store; bool store_ready = false; int steps_begun = 0; double phys_time = 0.0;
    bool beam_import = false;      // ring pipeline: the slices of the coming step arrive through import_beam_slice
    double beam_diag[7] = {0, 0, 0, 0, 0, 0, 0};   // n, sum w, |x|, |y|, |z|, |ux|, |uz| before the push (regular particles)
    // optional external beam storage in the product's block layout (pipeline tests):
    // block p (p-th slice from the head) = [7][count_p] at 7*ext_off[p]
    const double* ext_beam = nullptr; std::vector<long> ext_off; std::vector<double> own_beam;      // own_beam: orc_engine_set_beam_particles
    std::vector<double> checksum;      // per comp: sum |Q| over all valid cells and slices
    std::vector<double> checksum_xz;   // ... over the y = 0 line of every slice (diag_type = xz)
    long total_vcycles; long n_qsa_total;
    long pc_iterations = 0; double pc_err_sum = 0.0;     // Hipace.cpp:964,1028 (m_predcorr_avg_*)
    int c_aabs = -1; double laser_envelope_sum = 0.0;    // slab component of |a|^2; sum |a| over the box ("laserEnvelope")
    // envelope at time steps n-1, n, n+1 for every slice, valid cells only ([islice][j][i]); what the reference keeps in
    // the 9 slots of its laser slab + the MultiBuffer (utils/MultiBuffer.cpp:840-852, 913-925)
    std::vector<cplx> la_nm1, la_n00, la_np1; int laser_steps = 0;
    // Rolling window (single-step runs of boxes whose three envelope time levels do not fit host memory: 103 GB at
    // 1024^2 x 2048).  The first step needs a_n on slices j, j+1, j+2 -- the Gaussian of init_laser_slice, formed when first
    // asked for -- and a_{n+1} on j+1, j+2, written two and one slice earlier (MultiLaser.cpp:180-213 keeps exactly these
    // slices of the time levels in its slab); a_{n-1} is not read in step 0.  Three slots per level, slot = slice % 3.  Same
    // arithmetic on the same values as with whole-box arrays (tests/test_oracle_golden.py compares the two on a small box).
    bool laser_window = false;
    std::vector<cplx> win_n00[3], win_np1[3]; int win_n00_sl[3] = {-1, -1, -1}, win_np1_sl[3] = {-1, -1, -1};
    const cplx* n00_slice (int sl) {
        const size_t pl2 = (size_t)d.nx*d.ny;
        if (!laser_window) return la_n00.data() + (size_t)sl*pl2;
        const int k = sl % 3;
        if (win_n00_sl[k] != sl) { win_n00[k].resize(pl2); init_laser_slice(sl, win_n00[k].data()); win_n00_sl[k] = sl; }
        return win_n00[k].data();
    }
    const cplx* np1_slice_read (int sl) {
        const size_t pl2 = (size_t)d.nx*d.ny;
        if (!laser_window) return la_np1.data() + (size_t)sl*pl2;
        const int k = sl % 3;
        if (win_np1_sl[k] != sl) { std::fprintf(stderr, "oracle: envelope window: a_{n+1} of slice %d is not held\n", sl); std::abort(); }
        return win_np1[k].data();
    }
    cplx* np1_slice_write (int sl) {
        const size_t pl2 = (size_t)d.nx*d.ny;
        if (!laser_window) return la_np1.data() + (size_t)sl*pl2;
        const int k = sl % 3;
        win_np1[k].resize(pl2); win_np1_sl[k] = sl;
        return win_np1[k].data();
    }
    MG* laser_mg = nullptr; std::vector<double> laser_mg_guess; long laser_vcycles = 0;      // lasers.solver_type = multigrid
    bool laser_import = false;     // ring pipeline: a_n and a_{n-1} of the coming step arrive slice by slice
    double t_deposit, t_explicit, t_push, t_poisson, t_mg, t_other;

    explicit Engine (const Deck& dk) : d(dk), ps(nullptr), mg(nullptr) {
        // Fields::AllocData guards (fields/Fields.cpp:63-64)
        g = (d.order + 1)/2 + 1;
        ncomp = d.bxby_solver ? (d.deposit_rho ? 23 : 22) : (d.deposit_rho ? 22 : 21);
        if (d.laser_on && !d.bxby_solver) c_aabs = ncomp++;        // appended last
        gm.dx = (d.hi[0] - d.lo[0])/d.nx; gm.dy = (d.hi[1] - d.lo[1])/d.ny; gm.dz = (d.hi[2] - d.lo[2])/d.nz;
        gm.xoff = 0.5*(d.lo[0] + d.hi[0] - gm.dx*(d.nx - 1));
        gm.yoff = 0.5*(d.lo[1] + d.hi[1] - gm.dy*(d.ny - 1));
        gm.c = 1; gm.ep0 = 1; gm.mu0 = 1; gm.q_e = 1; gm.m_e = 1;   // make_constants_normalized
        if (d.si_units) {            // make_constants_SI (2018 CODATA, utils/Constants.H:15-24)
            gm.c = 299792458.0; gm.ep0 = 8.8541878128e-12; gm.mu0 = 1.25663706212e-06; gm.q_e = 1.602176634e-19; gm.m_e = 9.1093837015e-31;
        }
        gm.plo[0] = d.lo[0]; gm.plo[1] = d.lo[1]; gm.phi[0] = d.hi[0]; gm.phi[1] = d.hi[1];
        gm.bc = d.bc; gm.normalized = d.si_units ? 0 : 1;
        const long js = d.nx + 2*g, ns = js*(d.ny + 2*g);
        slab_data.assign((size_t)ns*ncomp, 0.0);
        slab = Slab{slab_data.data(), d.nx, d.ny, g, ncomp, js, ns};
        ps = new PoissonSolver(d.nx, d.ny, gm.dx, gm.dy);
        init_ionization();
        mg = d.bxby_solver ? nullptr : new MG(d.nx, d.ny, gm.dx, gm.dy);
        staging.assign((size_t)d.nx*d.ny, 0.0);
        checksum.assign((size_t)ncomp, 0.0); checksum_xz.assign((size_t)ncomp, 0.0);
        total_vcycles = 0; n_qsa_total = 0;
        t_deposit = t_explicit = t_push = t_poisson = t_mg = t_other = 0;
        pl.n = 0;
    }
    ~Engine () { delete ps; delete mg; }

    void zero_comp (int n) { std::fill(slab.comp(n), slab.comp(n) + slab.ns, 0.0); }
    void copy_comp (int dst, int src) { std::memcpy(slab.comp(dst), slab.comp(src), sizeof(double)*slab.ns); }

    // PlasmaParticleContainer::InitParticles (plasma/PlasmaParticleContainerInit.cpp:17-378),
    // fixed ppc, uniform density, no fine patch, u = 0; ppc index outermost (:192)
    // positions of the fixed-ppc lattice of one species (ppc index outermost, :192)
    void lattice (const int ppc[2], double density, std::vector<double>& xs, std::vector<double>& ys, std::vector<uint64_t>* slot = nullptr) const {
        const int nppc = ppc[0]*ppc[1];
        const double rad = d.plasma_radius > 0 ? d.plasma_radius : std::numeric_limits<double>::infinity();
        for (int ip = 0; ip < nppc; ++ip) {
            const int ixp = ip % ppc[0], iyp = ip / ppc[0];
            const double r0 = (0.5 + ixp)/ppc[0], r1 = (0.5 + iyp)/ppc[1];
            for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
                const double x = d.lo[0] + (i + r0)*gm.dx;
                const double y = d.lo[1] + (j + r1)*gm.dy;
                const double rsq = x*x + y*y;
                if (x >= gm.phi[0] || x < gm.plo[0] || y >= gm.phi[1] || y < gm.plo[1] ||
                    rsq > rad*rad || density*profile(x, y) <= 0.0) continue;
                xs.push_back(x); ys.push_back(y);
                if (slot) slot->push_back((uint64_t)ip*d.nx*d.ny + (uint64_t)j*d.nx + i);     // lattice point: the generator's key
            }
        }
    }
    void fill_species (Plasma& p, const std::vector<double>& xs, const std::vector<double>& ys, double w, int lev) const {
        for (long k = 0; k < (long)xs.size(); ++k) {
            p.x[k] = xs[k]; p.y[k] = ys[k]; p.w[k] = w*profile(xs[k], ys[k]);
            p.ux[k] = 0; p.uy[k] = 0; p.psi[k] = std::sqrt(1.0) - 0.0;
            p.x_prev[k] = xs[k]; p.y_prev[k] = ys[k];
            p.ux_half[k] = 0; p.uy_half[k] = 0; p.psi_half[k] = p.psi[k];
            p.valid[k] = 1; p.ion_lev[k] = lev;
        }
    }

    // PlasmaParticleContainer::InitParticles (plasma/PlasmaParticleContainerInit.cpp:17-378),
    // fixed ppc, uniform density, no fine patch, u = 0; ppc index outermost (:192)
    void init_plasma () {
        const int nppc = d.plasma_ppc[0]*d.plasma_ppc[1];
        // scale_fac (PlasmaParticleContainerInit.cpp:40-41): density per particle, or in SI the number of electrons it stands for
        const double scale = nppc <= 0 ? 0. : (d.si_units ? gm.dx*gm.dy*gm.dz/nppc : 1.0/nppc);
        std::vector<double> xs, ys;
        lattice(d.plasma_ppc, d.plasma_density, xs, ys);
        const long n = (long)xs.size();
        // species "ion": every ion can release Z - initial level electrons into the first species
        std::vector<double> ixs, iys; std::vector<uint64_t> islot;
        if (d.ion_on) lattice(d.ion_ppc, d.ion_density, ixs, iys, &islot);
        const long ni = (long)ixs.size();
        const long cap = n + ni*std::max(d.ion_Z - d.ion_init_level, 0);
        if (cap != pl_cap || pdata.empty()) {
            pl_cap = cap;
            pdata.assign((size_t)std::max(cap, 1L)*11, 0.0); pvalid.assign((size_t)std::max(cap, 1L), 0); pion.assign((size_t)std::max(cap, 1L), 0);
        }
        double* b = pdata.data();
        const long c = std::max(cap, 1L);
        pl = Plasma{b, b+c, b+2*c, b+3*c, b+4*c, b+5*c, b+6*c, b+7*c, b+8*c, b+9*c, b+10*c,
                    pvalid.data(), pion.data(), n};
        fill_species(pl, xs, ys, d.plasma_density*scale, 0);
        if (d.ion_on) {
            const int inppc = d.ion_ppc[0]*d.ion_ppc[1];
            const double iscale = inppc <= 0 ? 0. : (d.si_units ? gm.dx*gm.dy*gm.dz/inppc : 1.0/inppc);
            idata.assign((size_t)std::max(ni, 1L)*11, 0.0); ivalid.assign((size_t)std::max(ni, 1L), 1); ilev.assign((size_t)std::max(ni, 1L), 0);
            iuid.resize((size_t)std::max(ni, 1L));
            double* q = idata.data();
            const long m = std::max(ni, 1L);
            ipl = Plasma{q, q+m, q+2*m, q+3*m, q+4*m, q+5*m, q+6*m, q+7*m, q+8*m, q+9*m, q+10*m, ivalid.data(), ilev.data(), ni};
            fill_species(ipl, ixs, iys, d.ion_density*iscale, d.ion_init_level);
            for (long k = 0; k < ni; ++k) iuid[(size_t)k] = islot[(size_t)k];
        }
    }

    // InitIonizationModule (PlasmaParticleContainerInit.cpp:382-464): ADK prefactors (Chen, JCP 236 (2013), eq. (2);
    // l = m = 0, the approximate expressions without the Gamma function of the angular part)
    void init_ionization () {
        if (!d.ion_on || d.ion_Z <= 0) return;
        const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, ep0SI = 8.8541878128e-12;
        const double alpha = 0.0072973525693, r_e = 2.8179403227e-15;
        const double a3 = alpha*alpha*alpha, a4 = a3*alpha;
        const double wa = a3*cSI/r_e;
        const double Ea = meSI*cSI*cSI/qeSI*a4/r_e;
        const double UH = 13.59843449;                    // table_ionization_energies[0]
        const double l_eff = std::sqrt(UH/d.ion_energies[0]) - 1.0;
        const double wp = std::sqrt(d.background_density_SI*qeSI*qeSI/(ep0SI*meSI));
        const double dt = d.si_units ? gm.dz/cSI : gm.dz/wp;
        adk_power.assign(d.ion_Z, 0.0); adk_prefactor.assign(d.ion_Z, 0.0); adk_exp_prefactor.assign(d.ion_Z, 0.0);
        for (int i = 0; i < d.ion_Z; ++i) {
            const double Uion = d.ion_energies[i];
            const double n_eff = (i + 1)*std::sqrt(UH/Uion);
            const double C2 = std::pow(2, 2*n_eff)/(n_eff*std::tgamma(n_eff + l_eff + 1)*std::tgamma(n_eff - l_eff));
            adk_power[i] = -(2*n_eff - 1);
            adk_prefactor[i] = dt*wa*C2*(Uion/(2*UH))*std::pow(2*std::pow((Uion/UH), 3./2)*Ea, 2*n_eff - 1);
            adk_exp_prefactor[i] = -2./3*std::pow(Uion/UH, 3./2)*Ea;
        }
    }

    // uniform deviate in [0, 1) of (seed, ion, time step, slice): counter based, so that the HIP kernel draws the same
    // number for the same ion whatever the order of its particles (two rounds of the splitmix64 finaliser)
    static double ion_uniform (uint64_t seed, uint64_t uid, uint64_t step, uint64_t islice) {
        uint64_t z = seed + 0x9E3779B97F4A7C15ULL*(uid + 1) + 0xBF58476D1CE4E5B9ULL*(step + 1) + 0x94D049BB133111EBULL*(islice + 1);
        for (int r = 0; r < 2; ++r) {
            z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
            z ^= z >> 27; z *= 0x94D049BB133111EBULL;
            z ^= z >> 31;
        }
        return (double)(z >> 11)*(1.0/9007199254740992.0);
    }

    // PlasmaParticleContainer::IonizationModule (PlasmaParticleContainer.cpp:261-440): ADK probability from |E| at the
    // ion (fields of This slice, gathered at x_prev, y_prev), one draw per ion and slice, the released electron joins the
    // product species at rest at the ion's position with the ion's weight.  An ion that has lost all Z electrons cannot
    // ionise (the reference reads past the end of its ADK tables there).
    void ionization_module (int islice) {
        if (!d.ion_on || adk_prefactor.empty()) return;
        const bool pcs = d.bxby_solver != 0;      // (the predictor-corrector solver's slab layout)
        const int comp[5] = {pcs ? (int)pPsi : (int)Psi, pcs ? (int)pEz : (int)Ez, pcs ? (int)pBx : (int)Bx, pcs ? (int)pBy : (int)By, pcs ? (int)pBz : (int)Bz};
        const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, ep0SI = 8.8541878128e-12;
        const double wp = std::sqrt(d.background_density_SI*qeSI*qeSI/(ep0SI*meSI));
        const double E0 = d.si_units ? 1.0 : wp*meSI*cSI/qeSI;
        const double clightsq = 1.0/(gm.c*gm.c);
        for (long ip = 0; ip < ipl.n; ++ip) {
            if (!ipl.valid[ip]) continue;
            const int lev = ipl.ion_lev[ip];
            if (lev >= d.ion_Z) continue;
            Real ExmByp = 0, EypBxp = 0, Ezp = 0, Bxp = 0, Byp = 0, Bzp = 0;
            gather(d.order, ipl.x_prev[ip], ipl.y_prev[ip], ExmByp, EypBxp, Ezp, Bxp, Byp, Bzp, slab, comp, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff);
            const Real Exp = ExmByp + Byp*gm.c;
            const Real Eyp = EypBxp - Bxp*gm.c;
            const Real Ep = std::sqrt(Exp*Exp + Eyp*Eyp + Ezp*Ezp)*E0;
            const Real ux = ipl.ux_half[ip], uy = ipl.uy_half[ip], psi = ipl.psi_half[ip];
            const Real gammap = (1.0 + ux*ux*clightsq + uy*uy*clightsq + psi*psi)/(2.0*psi);
            // gamma / (psi + 1) to complete dt for QSA
            const Real w_dtau = gammap/psi*adk_prefactor[lev]*std::pow(Ep, adk_power[lev])*std::exp(adk_exp_prefactor[lev]/Ep);
            const Real p = 1.0 - std::exp(-w_dtau);
            const Real draw = ion_uniform(d.ion_seed, iuid[(size_t)ip], (uint64_t)cur_step, (uint64_t)islice);
            if (draw < p) {
                ipl.ion_lev[ip] += 1;
                const long k = pl.n;
                if (k >= pl_cap) { std::fprintf(stderr, "oracle: ionisation product species is full\n"); std::abort(); }
                pl.x[k] = ipl.x[ip]; pl.y[k] = ipl.y[ip]; pl.w[k] = ipl.w[ip];
                pl.ux[k] = 0; pl.uy[k] = 0; pl.psi[k] = 1.0;
                pl.x_prev[k] = ipl.x_prev[ip]; pl.y_prev[k] = ipl.y_prev[ip];
                pl.ux_half[k] = 0; pl.uy_half[k] = 0; pl.psi_half[k] = 1.0;
                pl.valid[k] = 1; pl.ion_lev[k] = 0;
                ++pl.n; ++n_ionized_total;
            }
        }
    }

    double beam_density (double x, double y, double z) const {
        // GetInitialDensity (particles/profiles/GetInitialDensity.H:33-51)
        if (d.beam_profile == 0) {
            const double ddx = (x - d.beam_pos_mean[0])/d.beam_pos_std[0];
            const double ddy = (y - d.beam_pos_mean[1])/d.beam_pos_std[1];
            const double ddz = (z - d.beam_pos_mean[2])/d.beam_pos_std[2];
            return d.beam_density*std::exp(-0.5*ddx*ddx)*std::exp(-0.5*ddy*ddy)*std::exp(-0.5*ddz*ddz);
        }
        return d.beam_density;
    }

    void beam_offsets () {
        ext_off.assign(d.nz + 1, 0);
        Beam b;
        for (int p = 0; p < d.nz; ++p) { gen_beam_slice(d.nz - 1 - p, b); ext_off[p + 1] = ext_off[p] + (long)b.x.size(); }
    }
    void init_beam_slice (int islice, Beam& b) const {
        if (!ext_beam) { gen_beam_slice(islice, b); return; }
        b = Beam();
        const int p = d.nz - 1 - islice;
        const long first = ext_off[p], cnt = ext_off[p + 1] - first;
        const double* blk = ext_beam + 7*first;
        b.x.assign(blk, blk + cnt); b.y.assign(blk + cnt, blk + 2*cnt); b.z.assign(blk + 2*cnt, blk + 3*cnt);
        b.ux.assign(blk + 3*cnt, blk + 4*cnt); b.uy.assign(blk + 4*cnt, blk + 5*cnt); b.uz.assign(blk + 5*cnt, blk + 6*cnt);
        b.w.assign(blk + 6*cnt, blk + 7*cnt);
    }
    void fill_initial_beam (double* dst) {
        if (ext_off.empty()) beam_offsets();
        Beam b;
        for (int p = 0; p < d.nz; ++p) {
            gen_beam_slice(d.nz - 1 - p, b);
            const long cnt = (long)b.x.size();
            double* blk = dst + 7*ext_off[p];
            const std::vector<double>* arr[7] = {&b.x, &b.y, &b.z, &b.ux, &b.uy, &b.uz, &b.w};
            for (int k = 0; k < 7; ++k) std::copy(arr[k]->begin(), arr[k]->end(), blk + k*cnt);
        }
    }

    // InitBeamFixedPPCSlice (beam/BeamParticleContainerInit.cpp:198-346)
    void gen_beam_slice (int islice, Beam& b) const {
        b = Beam();
        if (d.beam_profile < 0) return;
        const int nppc = d.beam_ppc[0]*d.beam_ppc[1]*d.beam_ppc[2];
        const double scale = d.si_units ? gm.dx*gm.dy*gm.dz/nppc : 1.0/nppc;      // BeamParticleContainerInit.cpp:215-216
        const int ny_p = d.beam_ppc[1], nz_p = d.beam_ppc[2];
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            for (int ip = 0; ip < nppc; ++ip) {
                // get_position_unit_cell (particles_utils/ParticleUtil.H:49-63)
                const int ixp = ip/(ny_p*nz_p), iyp = (ip % (ny_p*nz_p)) % ny_p, izp = (ip % (ny_p*nz_p))/ny_p;
                const double r0 = (0.5 + ixp)/d.beam_ppc[0], r1 = (0.5 + iyp)/d.beam_ppc[1], r2 = (0.5 + izp)/d.beam_ppc[2];
                const double x = d.lo[0] + (i + r0)*gm.dx;
                const double y = d.lo[1] + (j + r1)*gm.dy;
                const double z = d.lo[2] + (islice + r2)*gm.dz;
                if (z >= d.beam_zmax || z < d.beam_zmin ||
                    ((x - d.beam_pos_mean[0])*(x - d.beam_pos_mean[0]) + (y - d.beam_pos_mean[1])*(y - d.beam_pos_mean[1]))
                        > d.beam_radius*d.beam_radius) continue;
                const double dens = beam_density(x, y, z);
                if (dens <= 0.0) continue;
                b.x.push_back(x); b.y.push_back(y); b.z.push_back(z);
                b.ux.push_back(d.beam_umean[0]*gm.c); b.uy.push_back(d.beam_umean[1]*gm.c); b.uz.push_back(d.beam_umean[2]*gm.c);
                b.w.push_back(std::abs(dens*scale));
            }
        }
    }

    // DepositCurrentSlice for beams (deposition/BeamDepositCurrent.cpp:21-195)
    // GridCurrent::DepositCurrentSlice (utils/GridCurrent.cpp:25-71): valid cells only; z of the slice is
    // plo[2] + islice*dz (no half cell), x and y are cell centres
    void deposit_grid_current (int islice, int cjz) {
        if (!d.grid_current_on) return;
        const double z = d.lo[2] + islice*gm.dz;
        const double delta_z = (z - d.grid_current_mean[2]) / d.grid_current_std[2];
        const double long_pos_factor = std::exp(-0.5*(delta_z*delta_z));
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            const double x = d.lo[0] + (i + 0.5)*gm.dx;
            const double y = d.lo[1] + (j + 0.5)*gm.dy;
            const double delta_x = (x - d.grid_current_mean[0]) / d.grid_current_std[0];
            const double delta_y = (y - d.grid_current_mean[1]) / d.grid_current_std[1];
            const double trans_pos_factor = std::exp(-0.5*(delta_x*delta_x + delta_y*delta_y));
            slab(i, j, cjz) += d.grid_current_peak*trans_pos_factor*long_pos_factor;
        }
    }

    void deposit_beam (const Beam& b, int cjx, int cjy, int cjz, long count = -1) {
        const double dxi = 1.0/gm.dx, dyi = 1.0/gm.dy;
        const double invvol = d.si_units ? dxi*dyi*(1.0/gm.dz) : 1.0;      // BeamDepositCurrent.cpp:70-83, level 0
        const double clightsq = 1.0/(gm.c*gm.c);
        const double q = d.beam_charge;
        const size_t np = count < 0 ? b.x.size() : (size_t)count;     // getNumParticles: without slipped (:100)
        for (size_t ip = 0; ip < np; ++ip) {
            if (!b.valid.empty() && !b.valid[ip]) continue;
            const double ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
            const double gaminv = 1.0/std::sqrt(1.0 + ux*ux*clightsq + uy*uy*clightsq + uz*uz*clightsq);
            const double wq = q*b.w[ip]*invvol;
            const double vx = ux*gaminv, vy = uy*gaminv, vz = uz*gaminv;
            const double wqx = wq*vx, wqy = wq*vy, wqz = wq*vz;
            double sx[4], sy[4];
            const int i0 = shape_factor(d.order, sx, (b.x[ip] - gm.xoff)*dxi);
            const int j0 = shape_factor(d.order, sy, (b.y[ip] - gm.yoff)*dyi);
            for (int iy = 0; iy <= d.order; ++iy) for (int ix = 0; ix <= d.order; ++ix) {
                if (cjx != -1) { slab(i0+ix, j0+iy, cjx) += sx[ix]*sy[iy]*wqx;
                                 slab(i0+ix, j0+iy, cjy) += sx[ix]*sy[iy]*wqy; }
                if (cjz != -1) slab(i0+ix, j0+iy, cjz) += sx[ix]*sy[iy]*wqz;
            }
        }
    }

    // Multiply / LinCombination onto the staging area (fields/Fields.cpp:368-411), valid box only
    // Fields::SetBoundaryCondition, level 0, boundary.field = Open (fields/Fields.cpp:672-735) followed by
    // SetDirichletBoundaries (:627-669) with BoundaryOffset = BoundaryFactor = 1.  The reference expands the free-space
    // Green's function G = ln|r - r'|^2 / (4 pi) to order 18 about the origin with 37 real moments
    // (fields/OpenBoundary.H); the same expansion in complex form, z = x + i y:
    //     ln|z - z'|^2 = ln|z|^2 - sum_{n>=1} (2/n) Re( (z'/z)^n ),
    // so with M_n = sum_src s z'^n the boundary potential is  dx dy/(4 pi) [ M_0 ln|z|^2 - sum_n (2/n) Re(M_n z^-n) ].
    // Coordinates are scaled by 3/|diagonal| as in the reference (only the monopole's logarithm sees the scale);
    // sources further than 95 % of the distance to the nearest wall are ignored; Ez and Bz have no monopole.
    void open_boundary (bool no_monopole) {
        const int nx = d.nx, ny = d.ny;
        const double Lx = d.hi[0] - d.lo[0], Ly = d.hi[1] - d.lo[1];
        const double scale = 3.0/std::sqrt(Lx*Lx + Ly*Ly);
        const double radius = std::min(std::min(std::abs(d.lo[0]), std::abs(d.hi[0])), std::min(std::abs(d.lo[1]), std::abs(d.hi[1])));
        const double cutoff_sq = (0.95*radius*scale)*(0.95*radius*scale);
        constexpr int NO = 18;
        cplx M[NO + 1];
        for (int n = 0; n <= NO; ++n) M[n] = cplx(0.0, 0.0);
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
            const double x = (i*gm.dx + gm.xoff)*scale, y = (j*gm.dy + gm.yoff)*scale;
            if (x*x + y*y > cutoff_sq) continue;
            const double sv = staging[(size_t)j*nx + i];
            const cplx z(x, y); cplx zn(1.0, 0.0);
            for (int n = 0; n <= NO; ++n) { M[n] += sv*zn; zn *= z; }
        }
        if (no_monopole) M[0] = cplx(0.0, 0.0);
        const double pref = gm.dx*gm.dy/(4.0*M_PI);
        auto potential = [&] (double xd, double yd) {
            const cplx z(xd*scale, yd*scale);
            const cplx zi = 1.0/z; cplx zin = zi;
            double v = M[0].real()*std::log(std::norm(z));
            for (int n = 1; n <= NO; ++n) { v -= (2.0/n)*(M[n]*zin).real(); zin *= zi; }
            return pref*v;
        };
        // outermost rows/columns of the source get -phi(one cell outside)/h^2; corners get both
        for (int i = 0; i < nx; ++i) {
            const double x = i*gm.dx + gm.xoff;
            staging[(size_t)0*nx + i]        -= potential(x, (-1)*gm.dy + gm.yoff)/(gm.dy*gm.dy);
            staging[(size_t)(ny - 1)*nx + i] -= potential(x, ny*gm.dy + gm.yoff)/(gm.dy*gm.dy);
        }
        for (int j = 0; j < ny; ++j) {
            const double y = j*gm.dy + gm.yoff;
            staging[(size_t)j*nx + 0]        -= potential((-1)*gm.dx + gm.xoff, y)/(gm.dx*gm.dx);
            staging[(size_t)j*nx + (nx - 1)] -= potential(nx*gm.dx + gm.xoff, y)/(gm.dx*gm.dx);
        }
    }

    void poisson_to (int dst_comp, bool no_monopole = false) {
        if (d.field_bc == 1) open_boundary(no_monopole);
        ps->solve(staging.data());
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i)
            slab(i,j,dst_comp) = staging[(size_t)j*d.nx + i];
    }

    // SolvePoissonPsiExmByEypBxEzBz (fields/Fields.cpp:840-957)
    void solve_psi_ez_bz (int rhomjz, int jx, int jy, int Psi, int Ez, int Bz, int ExmBy, int EypBx) {
        const double dxi2 = 0.5*(1.0/gm.dx), dyi2 = 0.5*(1.0/gm.dy);
        const int nx = d.nx, ny = d.ny;
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i)
            staging[(size_t)j*nx + i] = (-1.0/gm.ep0)*slab(i,j,rhomjz);
        poisson_to(Psi);
        const double fa = 1.0/(gm.ep0*gm.c);
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i)
            staging[(size_t)j*nx + i] = fa*((slab(i+1,j,jx) - slab(i-1,j,jx))*dxi2)
                                      + fa*((slab(i,j+1,jy) - slab(i,j-1,jy))*dyi2);
        poisson_to(Ez, true);
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i)
            staging[(size_t)j*nx + i] = gm.mu0*((slab(i,j+1,jx) - slab(i,j-1,jx))*dyi2)
                                      + (-gm.mu0)*((slab(i+1,j,jy) - slab(i-1,j,jy))*dxi2);
        poisson_to(Bz, true);
        // ExmBy = -d/dx Psi, EypBx = -d/dy Psi on the box grown by (guards-1) (:931-956)
        const int gg = g - 1;
        for (int j = -gg; j < ny + gg; ++j) for (int i = -gg; i < nx + gg; ++i) {
            slab(i,j,ExmBy) = -(slab(i+1,j,Psi) - slab(i-1,j,Psi))*dxi2;
            slab(i,j,EypBx) = -(slab(i,j+1,Psi) - slab(i,j-1,Psi))*dyi2;
        }
    }

    // InitializeSxSyWithBeam (Hipace.cpp:744-790)
    void init_sxsy_with_beam () {
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            const double dx_jzb = (slab(i+1,j,jzb) - slab(i-1,j,jzb))/(2.0*gm.dx);
            const double dy_jzb = (slab(i,j+1,jzb) - slab(i,j-1,jzb))/(2.0*gm.dy);
            const double dz_jxb = (slab(i,j,P_jxb) - slab(i,j,N_jxb))/(2.0*gm.dz);
            const double dz_jyb = (slab(i,j,P_jyb) - slab(i,j,N_jyb))/(2.0*gm.dz);
            slab(i,j,Sy) =   gm.mu0*(-dy_jzb + dz_jyb);
            slab(i,j,Sx) = - gm.mu0*(-dx_jzb + dz_jxb);
        }
    }

    // InitLaserSlice's Gaussian envelope (laser/MultiLaser.cpp:881-919; Laser.H defaults: CEP 0, no propagation angle,
    // no pulse-front tilt) on slice islice
    void init_laser_slice (int islice, cplx* out) const {
        const double k0 = 2.0*M_PI/d.laser_lambda0;
        const double pz = 0.5*(d.lo[2] + d.hi[2] - gm.dz*(d.nz - 1));
        const double a0 = d.laser_a0, w0 = d.laser_w0, L0 = d.laser_L0, z0 = d.laser_pos[2], zfoc = d.laser_zfoc;
        const cplx I(0.0, 1.0);
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            const double x = i*gm.dx + gm.xoff - d.laser_pos[0];
            const double y = j*gm.dy + gm.yoff - d.laser_pos[1];
            const double z = islice*gm.dz + pz - z0;
            const double yp = y, zp = z;                          // cos(0) y - sin(0) z, sin(0) y + cos(0) z
            const cplx diffract_factor = 1.0 + I*(zp - zfoc + z0*1.0)*2.0/(k0*w0*w0);
            const cplx inv_complex_waist_2 = 1.0/(w0*w0*diffract_factor);
            const cplx prefactor = a0/diffract_factor;
            const cplx time_exponent = zp*zp/(L0*L0);
            const cplx stcfactor = prefactor*std::exp(-time_exponent);
            const cplx exp_argument = -(x*x + yp*yp)*inv_complex_waist_2;
            out[(size_t)j*d.nx + i] = stcfactor*std::exp(exp_argument)*std::exp(I*yp*k0*0.0 + 0.0);
        }
    }
    // UpdateLaserAabs (:214-291): aabs = |a_n|^2 on the field grid.  Laser grid = field grid and lasers.interp_order = 1,
    // so the interpolation weight is 1 on the cell itself; cells outside the laser box (the guard cells) get 0.
    void update_laser_aabs (int islice, bool accumulate) {
        const cplx* a = n00_slice(islice);
        zero_comp(c_aabs);
        double sum_abs = 0.0;
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            const cplx e = a[(size_t)j*d.nx + i];
            slab(i, j, c_aabs) = e.real()*e.real() + e.imag()*e.imag();
            sum_abs += std::abs(e);
        }
        if (accumulate) laser_envelope_sum += sum_abs;
    }
    // 2-D complex DFT of an ny x nx array in place; sign = -1 forward, +1 backward (unnormalised)
    void fft2 (std::vector<cplx>& a, int sign) const {
        const int nx = d.nx, ny = d.ny;
        auto run = [&] (int n, long stride, long nrows, long rstride) {
            std::vector<cplx> tw((size_t)n), in((size_t)n), out((size_t)n);
            for (int k = 0; k < n; ++k) { const double ang = sign*2.0*M_PI*k/n; tw[k] = cplx(std::cos(ang), std::sin(ang)); }
            for (long r = 0; r < nrows; ++r) {
                cplx* base = a.data() + r*rstride;
                for (int k = 0; k < n; ++k) in[k] = base[(long)k*stride];
                fft_rec(n, 1, in.data(), out.data(), tw, n);
                for (int k = 0; k < n; ++k) base[(long)k*stride] = out[k];
            }
        };
        run(nx, 1, ny, nx);
        run(ny, nx, nx, 1);
    }
    // MultiLaser::AdvanceSliceFFT (laser/MultiLaser.cpp:609-801): a_{n+1} on slice j from a_n, a_{n-1} on slices j, j+1,
    // j+2 and a_{n+1} on j+1, j+2 (zeros beyond the head of the box), chi of this slice; level 0, laser grid = field grid
    void advance_laser_slice (int islice) {
        const int nx = d.nx, ny = d.ny; const size_t pl2 = (size_t)nx*ny;
        const double dx = gm.dx, dy = gm.dy, dz = gm.dz, c = gm.c, dt = d.dt;
        const double k0 = 2.0*M_PI/d.laser_lambda0;
        const cplx I(0.0, 1.0);
        static const std::vector<cplx> zeros_dummy;
        std::vector<cplx> zero(pl2, cplx(0.0, 0.0));
        auto at = [&] (const std::vector<cplx>& v, int sl) -> const cplx* { return (sl < d.nz && !laser_window) ? v.data() + (size_t)sl*pl2 : zero.data(); };
        auto at_n00 = [&] (int sl) -> const cplx* { return sl < d.nz ? n00_slice(sl) : zero.data(); };
        auto at_np1 = [&] (int sl) -> const cplx* { return sl < d.nz ? np1_slice_read(sl) : zero.data(); };
        const cplx *n00j00 = at_n00(islice), *n00jp1 = at_n00(islice + 1), *n00jp2 = at_n00(islice + 2);
        const cplx *nm1j00 = at(la_nm1, islice), *nm1jp1 = at(la_nm1, islice + 1), *nm1jp2 = at(la_nm1, islice + 2);      // (not read in step 0)
        const cplx *np1jp1 = at_np1(islice + 1), *np1jp2 = at_np1(islice + 2);
        const int step = laser_steps;
        if (laser_window && step != 0) { std::fprintf(stderr, "oracle: the envelope window holds the first step only\n"); std::abort(); }
        const int imid = (nx + 1)/2, jmid = (ny + 1)/2;
        double tj00 = 0.0, tjp1 = 0.0, tjp2 = 0.0;
        if (d.laser_use_phase) {
            cplx s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
                const bool kx_ = (nx % 2 == 0) ? (i == imid - 1 || i == imid) : (i == imid);
                const bool ky_ = (ny % 2 == 0) ? (j == jmid - 1 || j == jmid) : (j == jmid);
                if (kx_ && ky_) { s0 += n00j00[(size_t)j*nx + i]; s1 += n00jp1[(size_t)j*nx + i]; s2 += n00jp2[(size_t)j*nx + i]; }
            }
            tj00 = std::atan2(s0.imag(), s0.real()); tjp1 = std::atan2(s1.imag(), s1.real()); tjp2 = std::atan2(s2.imag(), s2.real());
        }
        double dt1 = tj00 - tjp1, dt2 = tjp1 - tjp2;
        if (dt1 < -1.5*M_PI) dt1 += 2.0*M_PI;
        if (dt1 >  1.5*M_PI) dt1 -= 2.0*M_PI;
        if (dt2 < -1.5*M_PI) dt2 += 2.0*M_PI;
        if (dt2 >  1.5*M_PI) dt2 -= 2.0*M_PI;
        const cplx exp1 = std::exp(I*(tj00 - tjp1)), exp2 = std::exp(I*(tj00 - tjp2));
        const double djn = (-3.0*dt1 + dt2)/(2.0*dz);
        std::vector<cplx> rhs(pl2);
        std::vector<double> acf_real(d.laser_solver == 2 ? pl2 : 0);
        const double chi0 = d.plasma_density > 0.0 ? d.plasma_density*d.plasma_charge*d.plasma_charge*gm.mu0/d.plasma_mass : 0.0;
        const cplx* lapsrc = (step == 0) ? n00j00 : nm1j00;
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
            const size_t o = (size_t)j*nx + i;
            cplx lapA(0.0, 0.0);
            if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1)
                lapA = (lapsrc[o + 1] + lapsrc[o - 1] - 2.0*lapsrc[o])/(dx*dx) + (lapsrc[o + nx] + lapsrc[o - nx] - 2.0*lapsrc[o])/(dy*dy);
            // InterpolateChi (:334-407): chi of the field slab inside the box shrunk by the guard width, the chi of the
            // unperturbed plasma (SetInitialChi :293-332) outside
            const bool inside = i >= g && i < nx - g && j >= g && j < ny - g;
            const double chi_v = inside ? slab(i, j, chi) : chi0;
            // chi term: FFT solver 2 chi a_n on the right-hand side (:713-740); multigrid solver with MG_average_rhs (the
            // default): chi a_n (first step) / chi a_{n-1}, the other chi a_{n+1} sits in the operator (:575-598)
            const bool mgs = (d.laser_solver == 2);
            if (mgs) acf_real[o] = ((step == 0) ? 6.0/(c*dt*dz) : 3.0/(c*dt*dz) + 2.0/(c*c*dt*dt)) + chi_v;
            if (step == 0) {
                rhs[o] = 8.0/(c*dt*dz)*(-np1jp1[o] + n00jp1[o])*exp1
                       + 2.0/(c*dt*dz)*(+np1jp2[o] - n00jp2[o])*exp2
                       + (mgs ? 1.0 : 2.0)*chi_v*n00j00[o]
                       - lapA
                       + (-6.0/(c*dt*dz) + 4.0*I*djn/(c*dt) + I*4.0*k0/(c*dt))*n00j00[o];
            } else {
                rhs[o] = 4.0/(c*dt*dz)*(-np1jp1[o] + nm1jp1[o])*exp1
                       + 1.0/(c*dt*dz)*(+np1jp2[o] - nm1jp2[o])*exp2
                       - 4.0/(c*c*dt*dt)*n00j00[o]
                       + (mgs ? chi_v*nm1j00[o] : 2.0*chi_v*n00j00[o])
                       - lapA
                       + (-3.0/(c*dt*dz) + 2.0*I*djn/(c*dt) + 2.0/(c*c*dt*dt) + I*2.0*k0/(c*dt))*nm1j00[o];
            }
        }
        if (d.laser_solver == 2) {
            // AdvanceSliceMG (laser/MultiLaser.cpp:430-608): hpmg system type 2 on the laser box; the initial guess is
            // what np1j00 holds -- the solution of the slice solved before this one (ShiftLaserSlices leaves it, :208)
            const double acf_imag = (step == 0) ? -4.0*(k0 + djn)/(c*dt) : -2.0*(k0 + djn)/(c*dt);
            if (!laser_mg) laser_mg = new MG(nx, ny, dx, dy, 2);
            if (laser_mg_guess.size() != 2*pl2) laser_mg_guess.assign(2*pl2, 0.0);
            std::vector<double> r2(2*pl2);
            for (size_t o = 0; o < pl2; ++o) { r2[o] = rhs[o].real(); r2[pl2 + o] = rhs[o].imag(); }
            double* sol = laser_mg_guess.data();
            const int it = laser_mg->solve2(sol, sol + pl2, r2.data(), r2.data() + pl2, acf_real.data(), acf_imag, nx, 0,
                                            d.laser_mg_tol_rel, d.laser_mg_tol_abs, 200, nullptr);
            if (it < 0) { std::fprintf(stderr, "oracle: laser multigrid solve failed on slice %d\n", islice); std::abort(); }
            laser_vcycles += it;
            cplx* out = np1_slice_write(islice);
            for (size_t o = 0; o < pl2; ++o) out[o] = cplx(sol[o], sol[pl2 + o]);
            return;
        }
        fft2(rhs, -1);
        const double dkx = 2.0*M_PI/(d.hi[0] - d.lo[0]), dky = 2.0*M_PI/(d.hi[1] - d.lo[1]);
        const cplx acoeff = (step == 0) ? cplx(6.0/(c*dt*dz), 0.0) - I*4.0*(k0 + djn)/(c*dt)
                                        : cplx(3.0/(c*dt*dz) + 2.0/(c*c*dt*dt), 0.0) - I*2.0*(k0 + djn)/(c*dt);
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) {
            const double kx = (i < imid) ? dkx*i : dkx*(i - nx);
            const double ky = (j < jmid) ? dky*j : dky*(j - ny);
            const cplx den = kx*kx + ky*ky + acoeff;
            const cplx inv = (std::abs(den) > 0.0) ? 1.0/den : cplx(0.0, 0.0);
            rhs[(size_t)j*nx + i] *= -inv;
        }
        fft2(rhs, +1);
        const double inv_n = 1.0/((double)nx*ny);
        cplx* out = np1_slice_write(islice);
        for (size_t o = 0; o < pl2; ++o) out[o] = rhs[o]*inv_n;
    }

    static double now () {
        struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9*ts.tv_nsec;
    }

    // Fields::ComputeRelBFieldError (fields/Fields.cpp:1233-1286), level 0: sums over the valid box
    double rel_b_error (int cBx, int cBy, int cBxI, int cByI) const {
        double nB = 0.0, nD = 0.0;
        for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) {
            const double bx = slab(i,j,cBx), by = slab(i,j,cBy), ex = bx - slab(i,j,cBxI), ey = by - slab(i,j,cByI);
            nB += std::sqrt(bx*bx + by*by);
            nD += std::sqrt(ex*ex + ey*ey);
        }
        return nB > 0.0 ? nD/nB : 0.0;
    }
    // amrex::MultiFab::LinComb over the grown box: dst = a*x + b*y (dst may alias x or y)
    void lincomb (int dst, double a, int x, double b, int y) {
        double* pd = slab.comp(dst); const double* px = slab.comp(x); const double* py = slab.comp(y);
        for (long k = 0; k < slab.ns; ++k) pd[k] = a*px[k] + b*py[k];
    }
    // Fields::SolvePoissonBxBy (fields/Fields.cpp:1008-1075), level 0, Dirichlet
    void solve_bxby_poisson (int dstBx, int dstBy) {
        const double dxi2 = 0.5*(1.0/gm.dx), dyi2 = 0.5*(1.0/gm.dy), dzi2 = 0.5*(1.0/gm.dz);
        const int nx = d.nx, ny = d.ny;
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i)
            staging[(size_t)j*nx + i] = (-gm.mu0)*((slab(i,j+1,pjz) - slab(i,j-1,pjz))*dyi2)
                                      + gm.mu0*((slab(i,j,pP_jy) - slab(i,j,pN_jy))*dzi2);
        poisson_to(dstBx);
        for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i)
            staging[(size_t)j*nx + i] = gm.mu0*((slab(i+1,j,pjz) - slab(i-1,j,pjz))*dxi2)
                                      + (-gm.mu0)*((slab(i,j,pP_jx) - slab(i,j,pN_jx))*dzi2);
        poisson_to(dstBy);
    }

    // Hipace::SolveOneSlice, predictor-corrector branch (Hipace.cpp:556-728, 935-1031)
    void solve_one_slice_pc (int islice, bool accumulate) {
        double t0 = now();
        const bool moving = (d.dt != 0.0);
        if (moving) ensure_store();
        else if (islice != beam_this_slice) init_beam_slice(islice, beam_this);
        // InitializeSlices (fields/Fields.cpp:565-570)
        for (int c : {(int)pExmBy, (int)pEypBx, (int)pjx, (int)pjy, (int)pjz, (int)prhomjz}) zero_comp(c);
        if (d.deposit_rho) zero_comp(prho);
        double t1 = now(); t_other += t1 - t0;
        // plasma deposit jx jy jz [rho] rhomjz (Hipace.cpp:616-618; chi only with a laser)
        { const int comp[6] = {pjx, pjy, pjz, d.deposit_rho ? (int)prho : -1, -1, prhomjz};
          n_qsa_total += deposit_current(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, d.max_qsa, 0);
          // every species in turn (MultiPlasma::DepositCurrent, MultiPlasma.cpp:78-87); a species at its top level: no ADK step in this loop
          if (d.ion_on) n_qsa_total += deposit_current(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, d.max_qsa, 1); }
        double t2 = now(); t_deposit += t2 - t1;
        // beam jx jy jz on This, into the shared components (Hipace.cpp:620-623, BeamDepositCurrent.cpp:56-60)
        if (moving) deposit_beam(store[islice], pjx, pjy, pjz, store[islice].nreg);
        else deposit_beam(beam_this, pjx, pjy, pjz);
        for (long k = 0; k < slab.ns; ++k) slab.comp(prhomjz)[k] += slab.comp(pIon_rhomjz)[k];
        if (d.deposit_rho) for (long k = 0; k < slab.ns; ++k) slab.comp(prho)[k] += slab.comp(pIon_rhomjz)[k];
        deposit_grid_current(islice, pjz);      // Hipace.cpp:629
        double t3 = now(); t_other += t3 - t2;
        solve_psi_ez_bz(prhomjz, pjx, pjy, pPsi, pEz, pBz, pExmBy, pEypBx);
        double t4 = now(); t_poisson += t4 - t3;
        if (!moving) { if (islice - 1 >= 0) init_beam_slice(islice - 1, beam_next); else beam_next = Beam(); }

        // PredictorCorrectorLoopToSolveBxBy (Hipace.cpp:935-1031)
        double err_prev = 1.0;
        double err = rel_b_error(pP_Bx, pP_By, pPIt_Bx, pPIt_By);
        {   // InitialBfieldGuess (fields/Fields.cpp:1151-1173)
            const double mix0 = std::exp(-0.5*std::pow(err/(2.5*d.predcorr_tol), 2));
            lincomb(pBx, 1.0 + mix0, pP_Bx, -mix0, pPIt_Bx);
            lincomb(pBy, 1.0 + mix0, pP_By, -mix0, pPIt_By); }
        zero_comp(pIt_Bx); zero_comp(pIt_By);
        copy_comp(pPIt_Bx, pBx); copy_comp(pPIt_By, pBy);
        int it = 0;
        err = 1.0;
        while (err > d.predcorr_tol && it < d.predcorr_max_iter) {
            ++it; ++pc_iterations;
            double ta = now();
            { const int comp[5] = {pPsi, pEz, pBx, pBy, pBz};
              advance_plasma(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, 1, d.n_subcycles, 0);
              if (d.ion_on) advance_plasma(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, 1, d.n_subcycles, 1); }
            double tb = now(); t_push += tb - ta;
            { const int comp[6] = {pN_jx, pN_jy, -1, -1, -1, -1};
              n_qsa_total += deposit_current(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, d.max_qsa, 0);
              if (d.ion_on) n_qsa_total += deposit_current(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, d.max_qsa, 1); }
            double tc = now(); t_deposit += tc - tb;
            if (moving) { if (islice - 1 >= 0) deposit_beam(store[islice - 1], pN_jx, pN_jy, -1, store[islice - 1].nreg); }
            else deposit_beam(beam_next, pN_jx, pN_jy, -1);
            solve_bxby_poisson(pIt_Bx, pIt_By);
            err = rel_b_error(pBx, pBy, pIt_Bx, pIt_By);
            if (it == 1) err_prev = err;
            {   // MixAndShiftBfields (fields/Fields.cpp:1175-1231)
                double w_it, w_prev;
                if (err != 0.0 || err_prev != 0.0) { w_it = err_prev/(err + err_prev); w_prev = err/(err + err_prev); }
                else { w_it = 0.5; w_prev = 0.5; }
                lincomb(pPIt_Bx, w_it, pIt_Bx, w_prev, pPIt_Bx);
                lincomb(pPIt_By, w_it, pIt_By, w_prev, pPIt_By);
                lincomb(pBx, 1.0 - d.predcorr_mix, pBx, d.predcorr_mix, pPIt_Bx);
                lincomb(pBy, 1.0 - d.predcorr_mix, pBy, d.predcorr_mix, pPIt_By);
                copy_comp(pPIt_Bx, pIt_Bx); copy_comp(pPIt_By, pIt_By); }
            zero_comp(pN_jx); zero_comp(pN_jy);
            err_prev = err;
            t_poisson += now() - tc;
        }
        pc_err_sum += err;
        double t7 = now();
        if (accumulate) {
            for (int n = 0; n < ncomp; ++n) {
                double s = 0;
                for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) s += std::abs(slab(i,j,n));
                checksum[n] += s;
                // diag_type = xz: the y = 0 line of the slice -- the centre row, or the mean of the two central ones
                // (Fields::Copy's linear interpolation onto the trimmed diagnostic box, fields/Fields.cpp:413-533)
                double sx = 0;
                const int ja = (d.ny - 1)/2, jb = d.ny/2;
                for (int i = 0; i < d.nx; ++i) sx += std::abs(0.5*(slab(i,ja,n) + slab(i,jb,n)));
                checksum_xz[n] += sx;
            }
        }
        double t8 = now(); t_other += t8 - t7;
        { const int comp[5] = {pPsi, pEz, pBx, pBy, pBz};
          ionization_module(islice);               // DoFieldIonization (Hipace.cpp:693-696), before the committing pushes
          advance_plasma(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, 0, d.n_subcycles, 0);
          if (d.ion_on) advance_plasma(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, 0, d.n_subcycles, 1); }
        insitu_beam_slice(islice);
        if (moving) {
            const Beam& b = store[islice];
            for (long k = 0; k < b.nreg; ++k) {
                if (!b.valid[k]) continue;
                beam_diag[0] += 1; beam_diag[1] += std::abs(b.w[k]); beam_diag[2] += std::abs(b.x[k]); beam_diag[3] += std::abs(b.y[k]);
                beam_diag[4] += std::abs(b.z[k]); beam_diag[5] += std::abs(b.ux[k]); beam_diag[6] += std::abs(b.uz[k]);
            }
            advance_beam_slice(islice);
            shift_slipped(islice);
        }
        double t9 = now(); t_push += t9 - t8;
        // ShiftSlices (fields/Fields.cpp:600-603)
        copy_comp(pPIt_Bx, pP_Bx); copy_comp(pPIt_By, pP_By);
        copy_comp(pP_Bx, pBx); copy_comp(pP_By, pBy); copy_comp(pP_jx, pjx); copy_comp(pP_jy, pjy);
        if (!moving) { beam_this = beam_next; beam_this_slice = islice - 1; }
        t_other += now() - t9;
    }

    // Hipace::SolveOneSlice, explicit branch (Hipace.cpp:556-728)
    void solve_one_slice (int islice, bool accumulate) {
        if (d.bxby_solver) { solve_one_slice_pc(islice, accumulate); return; }
        double t0 = now();
        const bool moving = (d.dt != 0.0);
        if (moving) ensure_store();
        else if (islice != beam_this_slice) init_beam_slice(islice, beam_this);
        // InitializeSlices (fields/Fields.cpp:535-586)
        for (int c : {(int)chi, (int)Sy, (int)Sx, (int)ExmBy, (int)EypBx, (int)jzb, (int)rhomjz, (int)N_jxb, (int)N_jyb}) zero_comp(c);
        if (d.deposit_rho) zero_comp(rho);
        if (c_aabs >= 0) update_laser_aabs(islice, accumulate);
        double t1 = now(); t_other += t1 - t0;
        // plasma deposit jx jy [rho] chi rhomjz (Hipace.cpp:609-610)
        { const int comp[6] = {jx, jy, -1, d.deposit_rho ? (int)rho : -1, chi, rhomjz};
          n_qsa_total += deposit_current(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, d.max_qsa, 0, c_aabs);
          // MultiPlasma::DepositCurrent: every species in turn (MultiPlasma.cpp:78-87); ions weigh in with their level
          if (d.ion_on) n_qsa_total += deposit_current(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, d.max_qsa, 1, c_aabs); }
        double t2 = now(); t_deposit += t2 - t1;
        if (moving) deposit_beam(store[islice], -1, -1, jzb, store[islice].nreg);
        else deposit_beam(beam_this, -1, -1, jzb);
        // AddRhoIons (fields/Fields.cpp:606-615)
        for (long k = 0; k < slab.ns; ++k) slab.comp(rhomjz)[k] += slab.comp(Ion_rhomjz)[k];
        if (d.deposit_rho) for (long k = 0; k < slab.ns; ++k) slab.comp(rho)[k] += slab.comp(Ion_rhomjz)[k];
        deposit_grid_current(islice, jzb);      // Hipace.cpp:629
        double t3 = now(); t_other += t3 - t2;
        solve_psi_ez_bz(rhomjz, jx, jy, Psi, Ez, Bz, ExmBy, EypBx);
        // m_multi_laser.AdvanceSlice (Hipace.cpp:637)
        if (c_aabs >= 0 && d.laser_solver >= 1 && d.dt != 0.0) advance_laser_slice(islice);
        double t4 = now(); t_poisson += t4 - t3;
        if (moving) { if (islice - 1 >= 0) deposit_beam(store[islice - 1], N_jxb, N_jyb, -1, store[islice - 1].nreg); }
        else {
            if (islice - 1 >= 0) init_beam_slice(islice - 1, beam_next); else beam_next = Beam();
            deposit_beam(beam_next, N_jxb, N_jyb, -1);
        }
        init_sxsy_with_beam();
        double t5 = now(); t_other += t5 - t4;
        { const int cache[4] = {Bz, Ez, ExmBy, EypBx}; const int depos[2] = {Sy, Sx};
          explicit_deposit(slab, pl, gm, cache, depos, d.plasma_charge, d.plasma_mass, d.order, d.deriv_type, 0, c_aabs);
          if (d.ion_on) explicit_deposit(slab, ipl, gm, cache, depos, d.ion_charge, d.ion_mass, d.order, d.deriv_type, 1, c_aabs); }
        double t6 = now(); t_explicit += t6 - t5;
        // ExplicitMGSolveBxBy (Hipace.cpp:793-933)
        { const int it = mg->solve1(slab.comp(Bx), slab.comp(By), slab.comp(Sy), slab.comp(Sx), slab.comp(chi),
                                    slab.js, g, d.mg_tol_rel, d.mg_tol_abs, 200, nullptr);
          if (it < 0) { std::fprintf(stderr, "oracle: hpmg failed at slice %d\n", islice); std::abort(); }
          total_vcycles += it; }
        double t7 = now(); t_mg += t7 - t6;
        if (accumulate) {
            for (int n = 0; n < ncomp; ++n) {
                double s = 0;
                for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) s += std::abs(slab(i,j,n));
                checksum[n] += s;
                // diag_type = xz: the y = 0 line of the slice -- the centre row, or the mean of the two central ones
                // (Fields::Copy's linear interpolation onto the trimmed diagnostic box, fields/Fields.cpp:413-533)
                double sx = 0;
                const int ja = (d.ny - 1)/2, jb = d.ny/2;
                for (int i = 0; i < d.nx; ++i) sx += std::abs(0.5*(slab(i,ja,n) + slab(i,jb,n)));
                checksum_xz[n] += sx;
            }
        }
        double t8 = now(); t_other += t8 - t7;
        ionization_module(islice);               // DoFieldIonization (Hipace.cpp:693-696), before the push
        { const int comp[5] = {Psi, Ez, Bx, By, Bz};
          advance_plasma(slab, pl, gm, comp, d.plasma_charge, d.plasma_mass, d.order, 0, d.n_subcycles, 0, c_aabs);
          if (d.ion_on) advance_plasma(slab, ipl, gm, comp, d.ion_charge, d.ion_mass, d.order, 0, d.n_subcycles, 1, c_aabs); }
        insitu_beam_slice(islice);
        if (moving) {
            // beam diagnostics before the push (Hipace.cpp:685-686), then push and hand the slipped particles
            // to the next slice (:704-706)
            const Beam& b = store[islice];
            for (long k = 0; k < b.nreg; ++k) {
                if (!b.valid[k]) continue;
                beam_diag[0] += 1; beam_diag[1] += std::abs(b.w[k]); beam_diag[2] += std::abs(b.x[k]); beam_diag[3] += std::abs(b.y[k]);
                beam_diag[4] += std::abs(b.z[k]); beam_diag[5] += std::abs(b.ux[k]); beam_diag[6] += std::abs(b.uz[k]);
            }
            advance_beam_slice(islice);
            shift_slipped(islice);
        }
        double t9 = now(); t_push += t9 - t8;
        // ShiftSlices (fields/Fields.cpp:588-604)
        copy_comp(P_jxb, jxb); copy_comp(P_jyb, jyb);
        copy_comp(jxb, N_jxb); copy_comp(jyb, N_jyb); copy_comp(jx, N_jxb); copy_comp(jy, N_jyb);
        if (!moving) { beam_this = beam_next; beam_this_slice = islice - 1; }
        t_other += now() - t9;
    }

    void ensure_store () {
        if (store_ready) return;
        store.assign((size_t)d.nz, Beam());
        for (int isl = 0; isl < d.nz; ++isl) {
            Beam& b = store[isl];
            init_beam_slice(isl, b);          // (the deck's fixed_ppc beam, or the host's: orc_engine_set_beam_particles)
            b.nsub.assign(b.x.size(), 0); b.valid.assign(b.x.size(), 1); b.nreg = (long)b.x.size();
            if (d.beam_spin_tracking) {      // initial_spin, normalised (BeamParticleContainer.cpp:390-402)
                const double* s0 = d.beam_initial_spin;
                const double nrm = std::sqrt(s0[0]*s0[0] + s0[1]*s0[1] + s0[2]*s0[2]);
                b.sx.assign(b.x.size(), s0[0]/nrm); b.sy.assign(b.x.size(), s0[1]/nrm); b.sz.assign(b.x.size(), s0[2]/nrm);
            }
        }
        store_ready = true;
    }

    // BeamParticleContainer::InSituComputeDiags (particles/beam/BeamParticleContainer.cpp:476-556): the 23 per-slice
    // entries of the particles of this slice (slipped ones excluded, :494), before the beam push (Hipace.cpp:681)
    std::vector<double> insitu_bm; double insitu_bm_radius = 0.0;
    void insitu_beam_slice (int islice) {
        if (!(insitu_bm_radius > 0.0)) return;
        const bool moving = (d.dt != 0.0);
        const Beam& b = moving ? store[islice] : beam_this;
        const long n = moving ? b.nreg : (long)b.x.size();
        const double clight_inv = 1.0/gm.c, radius_sq = insitu_bm_radius*insitu_bm_radius;
        double s[23]; for (double& v : s) v = 0.0;
        for (long ip = 0; ip < n; ++ip) {
            const double x = b.x[ip], y = b.y[ip], z = b.z[ip];
            const double ux = b.ux[ip]*clight_inv, uy = b.uy[ip]*clight_inv, uz = b.uz[ip]*clight_inv, w = b.w[ip];
            const double uz_inv = uz == 0.0 ? 0.0 : 1.0/uz;
            if ((!b.valid.empty() && !b.valid[ip]) || x*x + y*y > radius_sq) continue;
            const double gamma = std::sqrt(1.0 + ux*ux + uy*uy + uz*uz);
            const double t[23] = {w, w*x, w*x*x, w*y, w*y*y, w*z, w*z*z, w*ux, w*ux*ux, w*uy, w*uy*uy, w*uz, w*uz*uz, w*x*ux, w*y*uy,
                                  w*z*uz, w*x*uy, w*y*ux, w*ux*uz_inv, w*uy*uz_inv, w*gamma, w*gamma*gamma, 1.0};
            for (int q = 0; q < 23; ++q) s[q] += t[q];
        }
        const double sum_w_inv = s[0] <= 0.0 ? 0.0 : 1.0/s[0];
        for (int q = 0; q < 23; ++q) insitu_bm[(size_t)q*d.nz + islice] = s[q]*((q == 0 || q == 22) ? 1.0 : sum_w_inv);
    }

    // AdvanceBeamParticlesSlice (particles/pusher/BeamParticleAdvance.cpp:20-336) without spin and mesh refinement;
    // external field E = (s0 x, s1 y, 0) (ExternalFields.H:29-56); optional radiation reaction (:244-297)
    void advance_beam_slice (int islice) {
        Beam& b = store[islice];
        // radiation reaction constants (:101-113), PhysConstSI of utils/Constants.H:15-24
        const bool rr = d.beam_radiation_reaction != 0;
        const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, ep0SI = 8.8541878128e-12, reSI = 2.817940326204929e-15;
        const bool normalized = !d.si_units;
        const double q_over_mc = normalized ? (d.beam_charge/d.beam_mass)/cSI*qeSI/meSI : (d.beam_charge/d.beam_mass)/cSI;
        const double RRcoeff = (2.0/3.0)*reSI*q_over_mc*q_over_mc;
        const double wp_inv = normalized ? std::sqrt(ep0SI*meSI/(d.background_density_SI*qeSI*qeSI)) : 1.0;
        const double E0 = normalized ? meSI*cSI/wp_inv/qeSI : 1.0;
        const double inv_clight_SI = 1.0/cSI, inv_clight = 1.0/gm.c;
        const int nsc = d.beam_n_subcycles;
        const Real dt = d.dt/nsc;
        const Real clight = gm.c, inv_c2 = 1.0/(gm.c*gm.c);
        const Real qm = d.beam_charge/d.beam_mass;
        const Real min_z = d.lo[2] + islice*gm.dz;
        const Real dx_inv = 1.0/gm.dx, dy_inv = 1.0/gm.dy;
        const bool pcs = d.bxby_solver != 0;      // This slice's fields in the predictor-corrector's component order
        const int comp[5] = {pcs ? (int)pPsi : (int)Psi, pcs ? (int)pEz : (int)Ez, pcs ? (int)pBx : (int)Bx, pcs ? (int)pBy : (int)By, pcs ? (int)pBz : (int)Bz};
        const bool ext = (d.ext_E_slope[0] != 0.0 || d.ext_E_slope[1] != 0.0);
        for (size_t ip = 0; ip < b.x.size(); ++ip) {          // getNumParticlesIncludingSlipped (:131)
            if (!b.valid[ip]) continue;
            Real xp = b.x[ip], yp = b.y[ip], zp = b.z[ip], ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
            int i = b.nsub[ip];
            bool gone = false;
            Real spin[3] = {0., 0., 0.};
            if (d.beam_spin_tracking) { spin[0] = b.sx[ip]; spin[1] = b.sy[ip]; spin[2] = b.sz[ip]; }
            for (; i < nsc; ++i) {
                if (zp < min_z) break;                         // not on this slice any more (:150-153)
                const Real gammap_inv = 1.0/std::sqrt(1.0 + (ux*ux + uy*uy + uz*uz)*inv_c2);
                xp += dt*0.5*ux*gammap_inv;
                yp += dt*0.5*uy*gammap_inv;
                if (enforce_bc(gm, xp, yp, ux, uy, b.w[ip], b.valid[ip])) { gone = true; break; }
                Real ExmByp = 0, EypBxp = 0, Ezp = 0, Bxp = 0, Byp = 0, Bzp = 0;
                gather(d.order, xp, yp, ExmByp, EypBxp, Ezp, Bxp, Byp, Bzp, slab, comp, dx_inv, dy_inv, gm.xoff, gm.yoff);
                if (ext) {
                    const Real Ex = d.ext_E_slope[0]*xp, Ey = d.ext_E_slope[1]*yp, Ezx = 0.0, Bx_ = 0.0, By_ = 0.0, Bz_ = 0.0;
                    ExmByp += Ex - clight*By_; EypBxp += Ey + clight*Bx_; Ezp += Ezx; Bxp += Bx_; Byp += By_; Bzp += Bz_;
                }
                Real ux_next = ux + dt*qm*(ExmByp + (clight - uz*gammap_inv)*Byp + uy*gammap_inv*Bzp);
                Real uy_next = uy + dt*qm*(EypBxp + (uz*gammap_inv - clight)*Bxp - ux*gammap_inv*Bzp);
                const Real ux_i = (ux_next + ux)*0.5, uy_i = (uy_next + uy)*0.5;
                const Real uz_i = uz + dt*0.5*qm*Ezp;
                const Real gamma_i_inv = 1.0/std::sqrt(1.0 + (ux_i*ux_i + uy_i*uy_i + uz_i*uz_i)*inv_c2);
                if (d.beam_spin_tracking) {      // Thomas-BMT precession, Boris-type rotation (:218-238)
                    const Real E[3] = {ExmByp + clight*Byp, EypBxp - clight*Bxp, Ezp};
                    const Real B[3] = {Bxp, Byp, Bzp};
                    const Real u[3] = {ux_i*inv_clight, uy_i*inv_clight, uz_i*inv_clight};
                    const Real beta[3] = {u[0]*gamma_i_inv, u[1]*gamma_i_inv, u[2]*gamma_i_inv};
                    const Real gamma_inv_p1 = gamma_i_inv/(1.0 + gamma_i_inv);
                    auto cross = [] (const Real* a, const Real* c, Real* o) { o[0] = a[1]*c[2] - a[2]*c[1]; o[1] = a[2]*c[0] - a[0]*c[2]; o[2] = a[0]*c[1] - a[1]*c[0]; };
                    auto dot = [] (const Real* a, const Real* c) { return a[0]*c[0] + a[1]*c[1] + a[2]*c[2]; };
                    Real bxE[3]; cross(beta, E, bxE);
                    const Real bdB = dot(beta, B);
                    Real h[3];
                    for (int q = 0; q < 3; ++q) {
                        const Real omega = std::abs(qm)*(B[q]*gamma_i_inv - bxE[q]*inv_clight*gamma_inv_p1
                            + d.beam_spin_anom*(B[q] - gamma_inv_p1*u[q]*bdB - bxE[q]*inv_clight));
                        h[q] = omega*dt*0.5;
                    }
                    Real hxs[3]; cross(h, spin, hxs);
                    const Real sp[3] = {spin[0] + hxs[0], spin[1] + hxs[1], spin[2] + hxs[2]};
                    const Real o = 1.0/(1.0 + dot(h, h));
                    Real hxsp[3]; cross(h, sp, hxsp);
                    const Real hds = dot(h, sp);
                    for (int q = 0; q < 3; ++q) spin[q] = o*(sp[q] + (hds*h[q] + hxsp[q]));
                }
                Real uz_next = uz + dt*qm*(Ezp + (ux_i*Byp - uy_i*Bxp)*gamma_i_inv);
                if (rr) {      // :244-297
                    Real Exp = ExmByp + clight*Byp, Eyp = EypBxp - clight*Bxp;
                    if (normalized) { Exp *= E0; Eyp *= E0; Ezp *= E0; Bxp *= E0*inv_clight_SI; Byp *= E0*inv_clight_SI; Bzp *= E0*inv_clight_SI; }
                    const Real gamma_i = std::sqrt(1.0 + (ux_i*ux_i + uy_i*uy_i + uz_i*uz_i)*inv_c2);
                    const Real vx_n = ux_i*gamma_i_inv*cSI*inv_clight, vy_n = uy_i*gamma_i_inv*cSI*inv_clight, vz_n = uz_i*gamma_i_inv*cSI*inv_clight;
                    const Real bx_n = vx_n*inv_clight_SI, by_n = vy_n*inv_clight_SI, bz_n = vz_n*inv_clight_SI;
                    const Real flx_q = (Exp + vy_n*Bzp - vz_n*Byp), fly_q = (Eyp + vz_n*Bxp - vx_n*Bzp), flz_q = (Ezp + vx_n*Byp - vy_n*Bxp);
                    const Real fl_q2 = flx_q*flx_q + fly_q*fly_q + flz_q*flz_q;
                    const Real bdotE = (bx_n*Exp + by_n*Eyp + bz_n*Ezp);
                    const Real bdotE2 = bdotE*bdotE;
                    const Real coeff = gamma_i*gamma_i*(fl_q2 - bdotE2);
                    const Real frx = RRcoeff*(cSI*(fly_q*Bzp - flz_q*Byp) + bdotE*Exp - coeff*bx_n);
                    const Real fry = RRcoeff*(cSI*(flz_q*Bxp - flx_q*Bzp) + bdotE*Eyp - coeff*by_n);
                    const Real frz = RRcoeff*(cSI*(flx_q*Byp - fly_q*Bxp) + bdotE*Ezp - coeff*bz_n);
                    ux_next += frx*dt*wp_inv*clight*inv_clight_SI;
                    uy_next += fry*dt*wp_inv*clight*inv_clight_SI;
                    uz_next += frz*dt*wp_inv*clight*inv_clight_SI;
                }
                const Real gamma_next_inv = 1.0/std::sqrt(1.0 + (ux_next*ux_next + uy_next*uy_next + uz_next*uz_next)*inv_c2);
                xp += dt*0.5*ux_next*gamma_next_inv;
                yp += dt*0.5*uy_next*gamma_next_inv;
                if (!d.beam_no_z_push) zp += dt*(uz_next*gamma_next_inv - clight);     // do_z_push (default true, :316)
                ux = ux_next; uy = uy_next; uz = uz_next;
            }
            if (gone) continue;
            if (enforce_bc(gm, xp, yp, ux, uy, b.w[ip], b.valid[ip])) continue;
            b.x[ip] = xp; b.y[ip] = yp; b.z[ip] = zp; b.nsub[ip] = i; b.ux[ip] = ux; b.uy[ip] = uy; b.uz[ip] = uz;
            if (d.beam_spin_tracking) { b.sx[ip] = spin[0]; b.sy[ip] = spin[1]; b.sz[ip] = spin[2]; }
        }
    }

    // shiftSlippedParticles (particles/sorting/SliceSort.cpp:12-64): drop invalid particles, keep z >= min_z on
    // this slice (they all count as regular from now on), append the others to the next slice as slipped
    void shift_slipped (int islice) {
        Beam& b = store[islice];
        const Real min_z = d.lo[2] + islice*gm.dz;
        Beam stay, slip;
        auto push = [] (Beam& t, const Beam& f, size_t k) {
            t.x.push_back(f.x[k]); t.y.push_back(f.y[k]); t.z.push_back(f.z[k]); t.ux.push_back(f.ux[k]);
            t.uy.push_back(f.uy[k]); t.uz.push_back(f.uz[k]); t.w.push_back(f.w[k]); t.nsub.push_back(f.nsub[k]); t.valid.push_back(1);
            if (!f.sx.empty()) { t.sx.push_back(f.sx[k]); t.sy.push_back(f.sy[k]); t.sz.push_back(f.sz[k]); }
        };
        for (size_t k = 0; k < b.x.size(); ++k) {
            if (!b.valid[k]) continue;
            if (b.z[k] >= min_z) push(stay, b, k); else push(slip, b, k);
        }
        stay.nreg = (long)stay.x.size();
        b = stay;
        if (islice - 1 >= 0) {
            Beam& nx = store[islice - 1];
            for (size_t k = 0; k < slip.x.size(); ++k) push(nx, slip, k);      // nreg of the next slice unchanged
        }
    }

    // start of one time step (Hipace::Evolve, Hipace.cpp:401-471)
    void begin_step () {
        std::fill(slab_data.begin(), slab_data.end(), 0.0);     // ResetAllQuantities
        beam_this_slice = -2;
        cur_step = (next_step >= 0) ? next_step : cur_step + 1; next_step = -1;
        init_plasma();
        // DepositNeutralizingBackground (plasma/MultiPlasma.cpp:106-118): rhomjz only, charge -q
        const int comp[6] = {-1, -1, -1, -1, -1, d.bxby_solver ? (int)pIon_rhomjz : (int)Ion_rhomjz};
        if (!d.plasma_no_neutralize)
            deposit_current(slab, pl, gm, comp, -d.plasma_charge, d.plasma_mass, d.order, d.max_qsa, 0);
        std::fill(checksum.begin(), checksum.end(), 0.0); std::fill(checksum_xz.begin(), checksum_xz.end(), 0.0);
        for (double& v : beam_diag) v = 0.0;
        laser_envelope_sum = 0.0;
        if (c_aabs >= 0) {
            const size_t tot = (size_t)d.nx*d.ny*d.nz;
            if (la_n00.empty() && steps_begun == 0 && !laser_import && d.n_steps == 1 && d.laser_solver >= 1 && d.dt != 0.0) {
                // one step over a box whose time levels would not fit: the rolling window (ORC_LASER_WINDOW=1 / 0 forces it on / off)
                const char* v = std::getenv("ORC_LASER_WINDOW");
                laser_window = v ? std::atoi(v) != 0 : (double)tot*48.0 > 24.0e9;
            }
            if (laser_window) {
                if (steps_begun > 0) { std::fprintf(stderr, "oracle: the envelope window holds the first step only\n"); std::abort(); }
                for (int k = 0; k < 3; ++k) { win_n00_sl[k] = -1; win_np1_sl[k] = -1; }
                laser_steps = 0;
            } else
            if (la_n00.empty()) {
                la_n00.assign(tot, cplx(0.0, 0.0)); la_nm1.assign(tot, cplx(0.0, 0.0)); la_np1.assign(tot, cplx(0.0, 0.0));
                if (!laser_import) { for (int k = 0; k < d.nz; ++k) init_laser_slice(k, la_n00.data() + (size_t)k*d.nx*d.ny); laser_steps = 0; }
            } else if (laser_import) {
                // a_n, a_{n-1} of this step come through import_laser_slice; laser_steps is set by the driver
            } else if (d.laser_solver >= 1 && d.dt != 0.0) {
                // what put_data / get_data move between two steps: a_{n+1} -> a_n, a_n -> a_{n-1} (MultiBuffer.cpp:840-852, 913-925)
                la_nm1.swap(la_n00); la_n00.swap(la_np1);
                ++laser_steps;
            }
        }
        if (d.dt != 0.0) {
            ensure_store();
            if (beam_import) {
                for (Beam& b : store) b = Beam();          // filled slice by slice by the ring hand-off
            } else if (steps_begun > 0) {
                phys_time += d.dt;
                // the buffer hand-off between steps does not carry the sub-cycle counters, and whatever sits on a
                // slice now is regular (BeamParticleContainer.H:35-37, MultiBuffer.cpp:809)
                for (Beam& b : store) { std::fill(b.nsub.begin(), b.nsub.end(), 0); b.nreg = (long)b.x.size(); }
            }
        }
        ++steps_begun;
    }

    void run () {
        for (int step = 0; step < d.n_steps; ++step) {
            begin_step();
            for (int isl = d.nz - 1; isl >= 0; --isl) solve_one_slice(isl, true);
        }
    }
};

} // namespace

// =============================================================================================
// C ABI for ctypes (tests, smoke, bench cpu_baseline only)
// =============================================================================================
extern "C" {

// external beam storage in the product's block layout (see include/hpslice.h, hps_engine_beam_info)
long orc_engine_beam_layout (void* h, long* offsets /* [nz+1] */);
void orc_engine_set_external_beam (void* h, const double* storage);
long orc_engine_set_beam_particles (void* h, long n, const double* soa);
void orc_engine_initial_beam (void* h, double* dst);

int orc_shape_factor (int order, double xmid, double* s_out) { return shape_factor(order, s_out, xmid); }

int orc_deriv_shape (int dtype, int order, double xmid, int ix, double* s, double* ds) {
    const DShape r = deriv_shape(dtype, order, xmid, ix); *s = r.s; *ds = r.ds; return r.cell;
}

struct orc_slab { double* p; int nx, ny, g, ncomp; };
struct orc_plasma { double *x,*y,*w,*ux,*uy,*psi,*x_prev,*y_prev,*ux_half,*uy_half,*psi_half;
                    int32_t* valid; int32_t* ion_lev; long n; };
struct orc_geom { double dx, dy, dz, xoff, yoff, c, ep0, mu0, q_e, m_e; double plo[2], phi[2]; int bc; int normalized; };

static Slab mk_slab (orc_slab s) { const long js = s.nx + 2*s.g; return Slab{s.p, s.nx, s.ny, s.g, s.ncomp, js, js*(s.ny + 2*s.g)}; }
static Plasma mk_pl (orc_plasma p) { return Plasma{p.x,p.y,p.w,p.ux,p.uy,p.psi,p.x_prev,p.y_prev,p.ux_half,p.uy_half,p.psi_half,p.valid,p.ion_lev,p.n}; }
static Geom mk_geom (orc_geom g) { Geom r; r.dx=g.dx; r.dy=g.dy; r.dz=g.dz; r.xoff=g.xoff; r.yoff=g.yoff; r.c=g.c; r.ep0=g.ep0; r.mu0=g.mu0; r.q_e=g.q_e; r.m_e=g.m_e;
    r.plo[0]=g.plo[0]; r.plo[1]=g.plo[1]; r.phi[0]=g.phi[0]; r.phi[1]=g.phi[1]; r.bc=g.bc; r.normalized=g.normalized; return r; }

long orc_deposit_current (orc_slab s, orc_plasma p, orc_geom g, const int* comp, double q, double m, int order, double max_qsa) {
    return deposit_current(mk_slab(s), mk_pl(p), mk_geom(g), comp, q, m, order, max_qsa, 0);
}
void orc_explicit_deposit (orc_slab s, orc_plasma p, orc_geom g, const int* cache, const int* depos, double q, double m, int order, int dtype) {
    explicit_deposit(mk_slab(s), mk_pl(p), mk_geom(g), cache, depos, q, m, order, dtype, 0);
}
void orc_advance_plasma (orc_slab s, orc_plasma p, orc_geom g, const int* comp, double q, double m, int order, int temp_slice, int n_subcycles) {
    advance_plasma(mk_slab(s), mk_pl(p), mk_geom(g), comp, q, m, order, temp_slice, n_subcycles, 0);
}
// the same three with ion levels (can_ionize) and a laser envelope (aabs_comp = slab component of |a|^2, -1: none); the
// entries above keep their signatures for existing callers
long orc_deposit_current_laser (orc_slab s, orc_plasma p, orc_geom g, const int* comp, double q, double m, int order, double max_qsa,
                                int can_ionize, int aabs_comp) {
    return deposit_current(mk_slab(s), mk_pl(p), mk_geom(g), comp, q, m, order, max_qsa, can_ionize, aabs_comp);
}
void orc_explicit_deposit_laser (orc_slab s, orc_plasma p, orc_geom g, const int* cache, const int* depos, double q, double m, int order,
                                 int dtype, int can_ionize, int aabs_comp) {
    explicit_deposit(mk_slab(s), mk_pl(p), mk_geom(g), cache, depos, q, m, order, dtype, can_ionize, aabs_comp);
}
void orc_advance_plasma_laser (orc_slab s, orc_plasma p, orc_geom g, const int* comp, double q, double m, int order, int temp_slice,
                               int n_subcycles, int can_ionize, int aabs_comp) {
    advance_plasma(mk_slab(s), mk_pl(p), mk_geom(g), comp, q, m, order, temp_slice, n_subcycles, can_ionize, aabs_comp);
}
void orc_gather (orc_slab s, orc_geom g, const int* comp, int order, double xp, double yp, double* out6) {
    double a=0,b=0,c=0,d=0,e=0,f=0;
    gather(order, xp, yp, a, b, c, d, e, f, mk_slab(s), comp, 1.0/g.dx, 1.0/g.dy, g.xoff, g.yoff);
    out6[0]=a; out6[1]=b; out6[2]=c; out6[3]=d; out6[4]=e; out6[5]=f;
}

// Tile binning restated: key = tile of the nearest cell (invalid particles last), STABLE counting
// sort (the product path: hipace_amd/csrc/sort.hip).  The reference sorts with
// amrex::SortParticlesForDeposition (not in /root/reference: parity unpinned against the
// reference; bit-exactness is defined between this restatement and the HIP path).
void orc_tile_sort (orc_plasma p, orc_geom g, int nx, int ny, int ts, uint32_t* perm, int32_t* offsets)
{
    // numbering of the cells inside a tile: blocks of bw x (32/bw) cells (sort.hip: cell_in_tile; HPS_CELL_BLOCK_W as there)
    int bw = 32;
    if (const char* e = std::getenv("HPS_CELL_BLOCK_W")) { const int v = std::atoi(e); if (v == 4 || v == 8 || v == 16 || v == 32) bw = v; }
    if (bw > ts) bw = ts;
    auto cell_in_tile = [&] (int x, int y) {
        if (bw >= ts) return y*ts + x;
        const int bh = 32/bw, bx = x/bw, by = y/bh, nbx = ts/bw;
        return ((by*nbx + bx)*bh + (y - by*bh))*bw + (x - bx*bw);
    };
    // pass 1: stable order by (tile, cell in tile) of the nearest cell, invalid particles last;
    // rank = position inside the run of equal keys (capped); pass 2: stable order by
    // (tile, rank, cell in tile): the particles of a tile interleaved over its cells.
    const int RANK_CAP = 16;
    const int ntx = (nx + ts - 1)/ts, nty = (ny + ts - 1)/ts, ntiles = ntx*nty;
    const long ncell = (long)ts*ts;
    const double dx_inv = 1.0/g.dx, dy_inv = 1.0/g.dy;
    std::vector<long> key1((size_t)p.n);
    for (long k = 0; k < p.n; ++k) {
        long c = (long)ntiles*ncell;
        if (p.valid[k]) {
            int ci = (int)std::floor((p.x[k] - g.xoff)*dx_inv + 0.5);
            int cj = (int)std::floor((p.y[k] - g.yoff)*dy_inv + 0.5);
            ci = std::min(std::max(ci, 0), nx - 1);
            cj = std::min(std::max(cj, 0), ny - 1);
            c = (long)((cj/ts)*ntx + (ci/ts))*ncell + cell_in_tile(ci % ts, cj % ts);
        }
        key1[k] = c;
    }
    std::vector<uint32_t> ord((size_t)p.n);
    for (long k = 0; k < p.n; ++k) ord[k] = (uint32_t)k;
    std::stable_sort(ord.begin(), ord.end(), [&] (uint32_t a, uint32_t b) { return key1[a] < key1[b]; });
    std::vector<long> key2((size_t)p.n);      // indexed by position after pass 1
    long run_start = 0;
    for (long q = 0; q < p.n; ++q) {
        if (q > 0 && key1[ord[q]] != key1[ord[q-1]]) run_start = q;
        const long c = key1[ord[q]], tile = c/ncell, cit = c - tile*ncell;
        const long rank = std::min<long>(q - run_start, RANK_CAP - 1);
        key2[q] = (tile*RANK_CAP + rank)*ncell + cit;
    }
    std::vector<long> pos((size_t)p.n);
    for (long q = 0; q < p.n; ++q) pos[q] = q;
    std::stable_sort(pos.begin(), pos.end(), [&] (long a, long b) { return key2[a] < key2[b]; });
    std::vector<long> count((size_t)ntiles + 2, 0);
    for (long q = 0; q < p.n; ++q) {
        perm[q] = ord[pos[q]];
        ++count[key2[pos[q]]/(RANK_CAP*ncell)];
    }
    long run = 0;
    for (int t = 0; t <= ntiles; ++t) { offsets[t] = (int32_t)run; run += count[t]; }
    offsets[ntiles + 1] = (int32_t)run;
}

void* orc_poisson_create (int nx, int ny, double dx, double dy) { return new PoissonSolver(nx, ny, dx, dy); }
void orc_poisson_solve (void* h, double* staging) { static_cast<PoissonSolver*>(h)->solve(staging); }
void orc_poisson_destroy (void* h) { delete static_cast<PoissonSolver*>(h); }
void orc_dst1 (int n, double* x, long stride) { DstPlan p(n); p.apply(x, stride); }

// system type 2 on planar arrays without guards: sol2 / rhs2 [2][ny][nx], acf_real [ny][nx]; -> V-cycles or -1
int orc_mg2_solve2 (int nx, int ny, double dx, double dy, double* sol2, const double* rhs2, const double* acf_real, double acf_imag,
                    double tol_rel, double tol_abs, int maxiter, double* resnorm) {
    MG m(nx, ny, dx, dy, 2);
    const long pl = (long)nx*ny;
    return m.solve2(sol2, sol2 + pl, rhs2, rhs2 + pl, acf_real, acf_imag, nx, 0, tol_rel, tol_abs, maxiter, resnorm);
}
void* orc_mg_create (int nx, int ny, double dx, double dy) { return new MG(nx, ny, dx, dy); }
int orc_mg_nlev (void* h) { return static_cast<MG*>(h)->nlev; }
// sol/rhs: 2 adjacent components each; acf 1 component, all with g guards, row stride nx+2g
int orc_mg_solve1 (void* h, double* sol2, const double* rhs2, const double* acf, int nx, int ny, int g,
                   double tol_rel, double tol_abs, int maxiter, double* resnorm) {
    const long js = nx + 2*g, ns = js*(ny + 2*g);
    return static_cast<MG*>(h)->solve1(sol2, sol2 + ns, rhs2, rhs2 + ns, acf, js, g, tol_rel, tol_abs, maxiter, resnorm);
}
void orc_mg_destroy (void* h) { delete static_cast<MG*>(h); }

struct orc_deck {
    int nx, ny, nz; double lo[3], hi[3]; int order; int deriv_type;
    int plasma_ppc[2]; double plasma_density; double plasma_radius;
    double plasma_charge, plasma_mass; double max_qsa; int n_subcycles;
    int beam_profile; double beam_zmin, beam_zmax, beam_radius, beam_density;
    double beam_umean[3], beam_pos_mean[3], beam_pos_std[3]; int beam_ppc[3]; double beam_charge;
    int bc; double mg_tol_rel, mg_tol_abs; int deposit_rho; int n_steps;
    double dt; int beam_n_subcycles; double beam_mass; double ext_E_slope[2];
    int bxby_solver; double predcorr_tol; int predcorr_max_iter; double predcorr_mix; int field_bc;
    int laser_on; double laser_a0, laser_w0, laser_L0, laser_lambda0, laser_pos[3];
    double laser_zfoc; int laser_solver; int laser_use_phase; int si_units;
    int grid_current_on; double grid_current_peak, grid_current_mean[3], grid_current_std[3];
    double laser_mg_tol_rel, laser_mg_tol_abs;
    int beam_radiation_reaction; double background_density_SI; int beam_no_z_push;
    int plasma_no_neutralize; int ion_on; int ion_ppc[2]; double ion_density, ion_mass, ion_charge; int ion_init_level, ion_Z;
    double ion_energies[56]; unsigned long long ion_seed;
    int beam_spin_tracking; double beam_initial_spin[3]; double beam_spin_anom;
};

// threads of the CPU-baseline leg (see g_threads); returns the number actually set
int orc_set_threads (int n) {
#ifdef _OPENMP
    g_threads = std::max(1, std::min(n, omp_get_max_threads() > 0 ? std::max(omp_get_max_threads(), n) : n));
#else
    (void)n; g_threads = 1;
#endif
    return g_threads;
}

void* orc_engine_create (const orc_deck* k) {
    Deck d;
    d.nx=k->nx; d.ny=k->ny; d.nz=k->nz; for (int i=0;i<3;++i){d.lo[i]=k->lo[i]; d.hi[i]=k->hi[i];}
    d.order=k->order; d.deriv_type=k->deriv_type; d.plasma_ppc[0]=k->plasma_ppc[0]; d.plasma_ppc[1]=k->plasma_ppc[1];
    d.plasma_density=k->plasma_density; d.plasma_radius=k->plasma_radius; d.plasma_charge=k->plasma_charge; d.plasma_mass=k->plasma_mass;
    d.max_qsa=k->max_qsa; d.n_subcycles=k->n_subcycles; d.beam_profile=k->beam_profile; d.beam_zmin=k->beam_zmin; d.beam_zmax=k->beam_zmax;
    d.beam_radius=k->beam_radius; d.beam_density=k->beam_density;
    for (int i=0;i<3;++i){d.beam_umean[i]=k->beam_umean[i]; d.beam_pos_mean[i]=k->beam_pos_mean[i]; d.beam_pos_std[i]=k->beam_pos_std[i]; d.beam_ppc[i]=k->beam_ppc[i];}
    d.beam_charge=k->beam_charge; d.bc=k->bc; d.mg_tol_rel=k->mg_tol_rel; d.mg_tol_abs=k->mg_tol_abs; d.deposit_rho=k->deposit_rho; d.n_steps=k->n_steps;
    d.dt=k->dt; d.beam_n_subcycles=k->beam_n_subcycles > 0 ? k->beam_n_subcycles : 10; d.beam_mass=k->beam_mass != 0.0 ? k->beam_mass : 1.0;
    d.ext_E_slope[0]=k->ext_E_slope[0]; d.ext_E_slope[1]=k->ext_E_slope[1];
    d.bxby_solver=k->bxby_solver; d.predcorr_tol=k->predcorr_tol > 0.0 ? k->predcorr_tol : 4e-2;
    d.predcorr_max_iter=k->predcorr_max_iter > 0 ? k->predcorr_max_iter : 30; d.predcorr_mix=k->predcorr_mix > 0.0 ? k->predcorr_mix : 0.05;
    d.field_bc=k->field_bc;
    d.laser_on=k->laser_on; d.laser_a0=k->laser_a0; d.laser_w0=k->laser_w0; d.laser_L0=k->laser_L0; d.laser_lambda0=k->laser_lambda0;
    for (int i=0;i<3;++i) d.laser_pos[i]=k->laser_pos[i];
    d.laser_zfoc=k->laser_zfoc; d.laser_solver=k->laser_solver; d.laser_use_phase=k->laser_use_phase; d.si_units=k->si_units;
    d.grid_current_on=k->grid_current_on; d.grid_current_peak=k->grid_current_peak;
    for (int i=0;i<3;++i){d.grid_current_mean[i]=k->grid_current_mean[i]; d.grid_current_std[i]=k->grid_current_std[i];}
    d.beam_radiation_reaction=k->beam_radiation_reaction; d.background_density_SI=k->background_density_SI; d.beam_no_z_push=k->beam_no_z_push;
    d.laser_mg_tol_rel = k->laser_mg_tol_rel > 0.0 ? k->laser_mg_tol_rel : 1.e-4; d.laser_mg_tol_abs = k->laser_mg_tol_abs;
    d.plasma_no_neutralize=k->plasma_no_neutralize; d.ion_on=k->ion_on; d.ion_ppc[0]=k->ion_ppc[0]; d.ion_ppc[1]=k->ion_ppc[1];
    d.ion_density=k->ion_density; d.ion_mass=k->ion_mass; d.ion_charge=k->ion_charge; d.ion_init_level=k->ion_init_level;
    d.ion_Z=std::min(std::max(k->ion_Z, 0), 56); for (int i=0;i<56;++i) d.ion_energies[i]=k->ion_energies[i]; d.ion_seed=k->ion_seed;
    d.beam_spin_tracking=k->beam_spin_tracking; for (int i=0;i<3;++i) d.beam_initial_spin[i]=k->beam_initial_spin[i];
    d.beam_spin_anom = k->beam_spin_anom;      // as given (0 = pure Thomas precession)
    return new Engine(d);
}
void orc_engine_destroy (void* h) { delete static_cast<Engine*>(h); }
void orc_engine_run (void* h) { static_cast<Engine*>(h)->run(); }
void orc_engine_begin_step (void* h) { static_cast<Engine*>(h)->begin_step(); }
void orc_engine_solve_slice (void* h, int islice) { static_cast<Engine*>(h)->solve_one_slice(islice, true); }
int orc_engine_ncomp (void* h) { return static_cast<Engine*>(h)->ncomp; }
int orc_engine_guards (void* h) { return static_cast<Engine*>(h)->g; }
long orc_engine_nparticles (void* h) { return static_cast<Engine*>(h)->pl.n; }
double* orc_engine_slab (void* h) { return static_cast<Engine*>(h)->slab_data.data(); }
double* orc_engine_particles (void* h) { return static_cast<Engine*>(h)->pdata.data(); }
// the 11 arrays of the first species are `stride` doubles apart (its capacity: ionisation adds particles)
long orc_engine_particle_stride (void* h) { return std::max(static_cast<Engine*>(h)->pl_cap, 1L); }
// species "ion": count, the 11 arrays (stride = max(count, 1)), validity flags, ionisation levels; electrons released so far
long orc_engine_nions (void* h) { Engine* e = static_cast<Engine*>(h); return e->d.ion_on ? e->ipl.n : 0; }
double* orc_engine_ions (void* h) { return static_cast<Engine*>(h)->idata.data(); }
int32_t* orc_engine_ion_valid (void* h) { return static_cast<Engine*>(h)->ivalid.data(); }
int32_t* orc_engine_ion_levels (void* h) { return static_cast<Engine*>(h)->ilev.data(); }
long orc_engine_n_ionized (void* h) { return static_cast<Engine*>(h)->n_ionized_total; }
void orc_adk_tables (void* h, double* prefactor, double* exp_prefactor, double* power) {
    Engine* e = static_cast<Engine*>(h);
    for (size_t i = 0; i < e->adk_prefactor.size(); ++i) { prefactor[i] = e->adk_prefactor[i]; exp_prefactor[i] = e->adk_exp_prefactor[i]; power[i] = e->adk_power[i]; }
}
void orc_engine_set_density_profile (void* h, int nr, const double* r, const double* fr, int nt, const double* ct, const double* ft) {
    Engine* e = static_cast<Engine*>(h);
    e->prof_r.assign(r, r + nr); e->prof_fr.assign(fr, fr + nr); e->prof_t.assign(ct, ct + nt); e->prof_ft.assign(ft, ft + nt);
}
double orc_ion_uniform (unsigned long long seed, unsigned long long uid, unsigned long long step, unsigned long long islice) {
    return Engine::ion_uniform(seed, uid, step, islice);
}
int32_t* orc_engine_valid (void* h) { return static_cast<Engine*>(h)->pvalid.data(); }
void orc_engine_checksums (void* h, double* out) { Engine* e = static_cast<Engine*>(h); for (int n = 0; n < e->ncomp; ++n) out[n] = e->checksum[n]; }
void orc_engine_checksums_xz (void* h, double* out) { Engine* e = static_cast<Engine*>(h); for (int n = 0; n < e->ncomp; ++n) out[n] = e->checksum_xz[n]; }
long orc_engine_vcycles (void* h) { return static_cast<Engine*>(h)->total_vcycles; }
long orc_engine_pc_iterations (void* h) { return static_cast<Engine*>(h)->pc_iterations; }
double orc_engine_pc_error_sum (void* h) { return static_cast<Engine*>(h)->pc_err_sum; }
int orc_engine_aabs_comp (void* h) { return static_cast<Engine*>(h)->c_aabs; }
double orc_engine_laser_envelope_sum (void* h) { return static_cast<Engine*>(h)->laser_envelope_sum; }
// envelope a_n of the step that has begun, [nz][ny][nx] complex (interleaved re, im); null without a laser
// ring hand-off of the envelope (MultiBuffer.cpp:840-852, 913-925): what a stage passes on for slice islice is
// {a_{n+1}, a_n}, which the next stage stores as its {a_n, a_{n-1}}
void orc_engine_set_step (void* h, int step) { static_cast<Engine*>(h)->next_step = step; }
void orc_engine_set_laser_import (void* h, int on, int step) { Engine* e = static_cast<Engine*>(h); e->laser_import = (on != 0); e->laser_steps = step; }
static void no_window (void* h, const char* what) {
    if (static_cast<Engine*>(h)->laser_window) { std::fprintf(stderr, "oracle: %s needs the envelope's whole-box time levels (ORC_LASER_WINDOW=0)\n", what); std::abort(); }
}
void orc_engine_export_laser_slice (void* h, int islice, double* out /* [2][ny][nx] complex */) {
    no_window(h, "export_laser_slice");
    Engine* e = static_cast<Engine*>(h); const size_t pl2 = (size_t)e->d.nx*e->d.ny;
    const bool evolve = e->d.laser_solver >= 1 && e->d.dt != 0.0;
    std::memcpy(out, (evolve ? e->la_np1 : e->la_n00).data() + (size_t)islice*pl2, pl2*sizeof(cplx));
    std::memcpy(out + 2*pl2, e->la_n00.data() + (size_t)islice*pl2, pl2*sizeof(cplx));
}
void orc_engine_import_laser_slice (void* h, int islice, const double* in) {
    Engine* e = static_cast<Engine*>(h); const size_t pl2 = (size_t)e->d.nx*e->d.ny;
    std::memcpy(static_cast<void*>(e->la_n00.data() + (size_t)islice*pl2), in, pl2*sizeof(cplx));
    std::memcpy(static_cast<void*>(e->la_nm1.data() + (size_t)islice*pl2), in + 2*pl2, pl2*sizeof(cplx));
}
// in-process hand-off: the same, straight from the engine that ran the previous step
void orc_engine_import_laser_from (void* h, int islice, void* src) {
    Engine* e = static_cast<Engine*>(h); Engine* p = static_cast<Engine*>(src); const size_t pl2 = (size_t)e->d.nx*e->d.ny;
    const bool evolve = p->d.laser_solver >= 1 && p->d.dt != 0.0;
    // a_n -> a_{n-1} first: with one stage in flight source and destination are the same engine
    std::copy(p->la_n00.begin() + (size_t)islice*pl2, p->la_n00.begin() + (size_t)(islice + 1)*pl2, e->la_nm1.begin() + (size_t)islice*pl2);
    std::copy((evolve ? p->la_np1 : p->la_n00).begin() + (size_t)islice*pl2, (evolve ? p->la_np1 : p->la_n00).begin() + (size_t)(islice + 1)*pl2,
              e->la_n00.begin() + (size_t)islice*pl2);
}
const double* orc_engine_laser_envelope (void* h) { Engine* e = static_cast<Engine*>(h); return e->la_n00.empty() ? nullptr : reinterpret_cast<const double*>(e->la_n00.data()); }
void orc_engine_times (void* h, double* t6) { Engine* e = static_cast<Engine*>(h);
    t6[0]=e->t_deposit; t6[1]=e->t_explicit; t6[2]=e->t_push; t6[3]=e->t_poisson; t6[4]=e->t_mg; t6[5]=e->t_other; }
long orc_engine_beam_layout (void* h, long* offsets) {
    Engine* e = static_cast<Engine*>(h);
    if (e->ext_off.empty()) e->beam_offsets();
    for (int p = 0; p <= e->d.nz; ++p) offsets[p] = e->ext_off[p];
    return e->ext_off[e->d.nz];
}
void orc_engine_set_external_beam (void* h, const double* storage) {
    Engine* e = static_cast<Engine*>(h);
    if (e->ext_off.empty()) e->beam_offsets();
    e->ext_beam = storage;
}
void orc_engine_initial_beam (void* h, double* dst) { static_cast<Engine*>(h)->fill_initial_beam(dst); }
// A host-initialised beam (any injection type of BeamParticleContainerInit.cpp) in place of the deck's (before the first step):
// soa = [7][n] x y z ux uy uz w; binned as BoxSorter does (sorting/BoxSort.cpp:34-43), head slice first, input order kept
// inside a slice; returns the number of particles outside the box in z (left out).
long orc_engine_set_beam_particles (void* h, long n, const double* soa) {
    Engine* e = static_cast<Engine*>(h);
    const int nz = e->d.nz;
    std::vector<int> where((size_t)n);
    std::vector<long> count((size_t)nz + 1, 0);
    long outside = 0;
    const double inv_dz = 1.0/e->gm.dz;
    for (long i = 0; i < n; ++i) {
        const double t = (soa[2*n + i] - e->d.lo[2])*inv_dz;
        const int q = (t > -1.0e9 && t < 1.0e9) ? static_cast<int>(t) : -1;
        if (q < 0 || q >= nz) { where[(size_t)i] = -1; ++outside; continue; }
        where[(size_t)i] = nz - 1 - q; ++count[(size_t)(nz - 1 - q) + 1];
    }
    e->ext_off.assign(nz + 1, 0);
    for (int p = 0; p < nz; ++p) e->ext_off[p + 1] = e->ext_off[p] + count[(size_t)p + 1];
    std::vector<long> next(e->ext_off.begin(), e->ext_off.end() - 1);
    e->own_beam.assign((size_t)7*(n - outside) + 1, 0.0);
    for (long i = 0; i < n; ++i) {
        const int p = where[(size_t)i];
        if (p < 0) continue;
        const long first = e->ext_off[p], cnt = e->ext_off[p + 1] - first, j = next[(size_t)p]++ - first;
        for (int k = 0; k < 7; ++k) e->own_beam[(size_t)7*first + (size_t)k*cnt + j] = soa[(size_t)k*n + i];
    }
    e->ext_beam = e->own_beam.data();
    return outside;
}

// beam statistics of the whole beam (sum over all slices) for the "beam" block of the JSONs
void orc_engine_beam_stats (void* h, double* out /* n, sum w, sum|x|, sum|y|, sum|z|, sum|uz| */) {
    Engine* e = static_cast<Engine*>(h);
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (e->d.dt != 0.0) {        // moving beam: what the last step's diagnostics saw (before its pushes)
        out[0] = e->beam_diag[0]; out[1] = e->beam_diag[1]; out[2] = e->beam_diag[2]; out[3] = e->beam_diag[3];
        out[4] = e->beam_diag[4]; out[5] = e->beam_diag[6];
        return;
    }
    Beam b;
    for (int isl = e->d.nz - 1; isl >= 0; --isl) {
        e->gen_beam_slice(isl, b);
        out[0] += (double)b.x.size();
        for (size_t k = 0; k < b.x.size(); ++k) { out[1] += b.w[k]; out[2] += std::abs(b.x[k]); out[3] += std::abs(b.y[k]); out[4] += std::abs(b.z[k]); out[5] += std::abs(b.uz[k]); }
    }
}

// ring hand-off of a moving beam (MultiBuffer::{put_data,get_data}, utils/MultiBuffer.cpp:444-609): what sits on a
// slice after its push leaves as one block, and enters the next step's slice as regular particles
void orc_engine_set_beam_import (void* h, int on) { Engine* e = static_cast<Engine*>(h); e->ensure_store(); e->beam_import = (on != 0); }
void orc_engine_import_beam_slice (void* h, int islice, long count, const double* in7n) {
    Engine* e = static_cast<Engine*>(h); e->ensure_store();
    Beam b; const size_t n = (size_t)count;
    std::vector<double>* a[7] = {&b.x, &b.y, &b.z, &b.ux, &b.uy, &b.uz, &b.w};
    for (int k = 0; k < 7; ++k) a[k]->assign(in7n + k*n, in7n + (k + 1)*n);
    b.nsub.assign(n, 0); b.valid.assign(n, 1); b.nreg = count;
    e->store[islice] = b;
}
// moving beam: sum |ux| seen by the last step's diagnostics, and the per-slice store for parity tests
double orc_engine_beam_sum_abs_ux (void* h) { return static_cast<Engine*>(h)->beam_diag[5]; }
long orc_engine_beam_slice_count (void* h, int islice) {
    Engine* e = static_cast<Engine*>(h); e->ensure_store(); return (long)e->store[islice].x.size(); }
void orc_engine_beam_slice (void* h, int islice, double* out7n) {       // [7][count]: x y z ux uy uz w
    Engine* e = static_cast<Engine*>(h); e->ensure_store();
    const Beam& b = e->store[islice]; const size_t n = b.x.size();
    const std::vector<double>* a[7] = {&b.x, &b.y, &b.z, &b.ux, &b.uy, &b.uz, &b.w};
    for (int k = 0; k < 7; ++k) for (size_t i = 0; i < n; ++i) out7n[k*n + i] = (*a[k])[i];
}
void orc_engine_beam_spin (void* h, int islice, double* out3n) {       // [3][count]: sx sy sz (do_spin_tracking)
    Engine* e = static_cast<Engine*>(h); e->ensure_store();
    const Beam& b = e->store[islice]; const size_t n = b.sx.size();
    const std::vector<double>* a[3] = {&b.sx, &b.sy, &b.sz};
    for (int k = 0; k < 3; ++k) for (size_t i = 0; i < n; ++i) out3n[k*n + i] = (*a[k])[i];
}
long orc_engine_laser_vcycles (void* h) { return static_cast<Engine*>(h)->laser_vcycles; }
void orc_engine_set_insitu_beam (void* h, double radius) {
    Engine* e = static_cast<Engine*>(h); e->insitu_bm_radius = radius; e->insitu_bm.assign((size_t)23*e->d.nz, 0.0); }
void orc_engine_insitu_beam (void* h, double* out /* [23][nz] */) {
    Engine* e = static_cast<Engine*>(h); std::copy(e->insitu_bm.begin(), e->insitu_bm.end(), out); }

} // extern "C"
