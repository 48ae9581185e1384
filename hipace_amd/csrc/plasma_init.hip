// plasma_init.hip -- InitParticles with <plasma>.fine_patch(x,y), fine_ppc, fine_transition_cells and hollow_core_radius
// (particles/plasma/PlasmaParticleContainerInit.cpp:36-313, particles/particles_utils/ParticleUtil.H:66-104).
//
// A cell of level 0 owns ppc_x ppc_y slots of the sheet, a cell of level > 0 (the patch and its transition) fine_x fine_y.
// The slot order is the reference's: i_part outermost, and within one i_part the cells that own it x-fastest.  Every cell
// owns the i_part below ppc_x ppc_y, only the cells of level > 0 own the others, so with `cells` = the x-fastest list of
// those cells slot k is
//     k <  ncoarse = ppc_x ppc_y nx ny:   i_part = k / (nx ny),                               cell = k mod (nx ny)
//     k >= ncoarse:                       i_part = ppc_x ppc_y + (k - ncoarse) / #cells,      cell = cells[(k - ncoarse) mod #cells]
// The count is static: a slot beyond the radius, inside the hollow core or without density is an invalid slot, as in
// k_init_plasma (engine.hip), which decks without these keys keep using.
//
// <plasma>.u_mean / u_std, do_symmetrize and prevent_centered_particle (:52-64, 173-177, 317-370, ParticleUtil.H:113-124;
// DESIGN 8i) go through k_init_plasma_warm: the same slots with a Gaussian momentum from a counter-based draw, three mirror
// copies of the whole sheet behind it, and the lattice moved by half a cell where the cell count and ppc are both odd.
#include "engine.h"
#include "expr.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace hps {

struct FineInit {
    const int* level;            // [ny][nx], null: every cell is coarse (hollow core without a patch)
    const int* cells;            // cells of level > 0, ascending
    long ncells, ncoarse;
    int cx, cy, fx, fy, T;
    double w_coarse, w_fine;     // density * scale_fac_coarse | scale_fac_fine (:38-45)
    double radius_sq, hollow_sq;
};

// Slot k of the sheet: its position, its weight and whether it holds a particle.  xoff, yoff: 0, or -0.5 in a direction
// that prevent_centered_particle shifts (:52-64) -- there the cells are the nodes 1 .. n - 1, and index 0 owns no particle
//
// PROG: the density is the species' program at (x, y, c t) instead of density f_r f_t -- a.w_coarse, a.w_fine then
// hold scale_fac alone (density 1), the weight is value * scale_fac, and the slot holds a particle iff value > min_density
// (:280).  The program's stack: this lane's column of the workgroup's dynamic LDS, [level][lane], depth - 1 levels.  Every
// lane of the wave runs the program (the opcode is uniform); the tests of the radius and the core only gate the result.
struct SlotInit { double x, y, w; bool live; };
template <bool PROG>
__device__ __forceinline__ SlotInit init_slot (long k, int nx, int ny, const FineInit& a, double lox, double loy, double dx, double dy,
                                               const double* __restrict__ prof, int nr, double ft, const DensityProgram& dp,
                                               double xoff = 0.0, double yoff = 0.0)
{
    const long cells = (long)nx*ny;
    int ip, L = 0;
    long c;
    if (k < a.ncoarse) {
        ip = (int)(k / cells);
        c = k - (long)ip*cells;
        if (a.level) L = a.level[c];
    } else {
        const long kk = k - a.ncoarse, q = kk / a.ncells;
        ip = a.cx*a.cy + (int)q;
        c = a.cells[kk - q*a.ncells];
        L = a.level[c];
    }
    const int j = (int)(c / nx), i = (int)(c - (long)j*nx);
    // get_position_unit_cell_fine (ParticleUtil.H:66-104)
    double rx, ry;
    if (L == 0) {
        const int ixp = ip % a.cx, iyp = ip / a.cx;
        rx = (0.5 + ixp)/a.cx;
        ry = (0.5 + iyp)/a.cy;
    } else {
        const int ixf = ip % a.fx, iyf = ip / a.fx;
        const int ixc = (ixf*a.cx)/a.fx, iyc = (iyf*a.cy)/a.fy;
        double s = double(L)/(a.T + 1);
        s = 1.5*s - 0.5*s*s*s;
        rx = ((0.5 + ixc)/a.cx)*(1.0 - s) + ((0.5 + ixf)/a.fx)*s;
        ry = ((0.5 + iyc)/a.cy)*(1.0 - s) + ((0.5 + iyf)/a.fy)*s;
    }
    const double x = lox + (i + rx + xoff)*dx;
    const double y = loy + (j + ry + yoff)*dy;
    // <plasma>.radius, hollow_core_radius and the density (PlasmaParticleContainerInit.cpp:274-279)
    const double rsq = x*x + y*y;
    const double weight = L == 0 ? a.w_coarse : a.w_fine;      // (:289-294)
    if constexpr (PROG) {
        extern __shared__ double s_density_stack[];
        ExprLdsStack st{s_density_stack + threadIdx.x, (int)blockDim.x};
        const ExprXyz v{x, y, dp.z};
        const double value = expr_run(dp.ins, dp.n_ins, dp.consts, v, st);
        const bool out = rsq > a.radius_sq || rsq < a.hollow_sq || (xoff != 0.0 && i == 0) || (yoff != 0.0 && j == 0);
        const bool live = !out && value > dp.min_density;
        return {x, y, live ? value*weight : 0.0, live};
    } else {
        double fac = (rsq > a.radius_sq || rsq < a.hollow_sq) ? 0.0 : ft*table_value(prof, prof + nr, nr, sqrt(rsq));
        if ((xoff != 0.0 && i == 0) || (yoff != 0.0 && j == 0)) fac = 0.0;
        return {x, y, fac > 0.0 ? weight*fac : 0.0, fac > 0.0};
    }
}

template <bool PROG>
__global__ __launch_bounds__(256)
void k_init_plasma_fine (hps_plasma pl, long n, int nx, int ny, FineInit a, double lox, double loy, double dx, double dy,
                         int level, int keyed, const double* __restrict__ prof, int nr, double ft, DensityProgram dp)
{
    const long k = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (k >= n) return;
    const SlotInit s = init_slot<PROG>(k, nx, ny, a, lox, loy, dx, dy, prof, nr, ft, dp);
    const double x = s.x, y = s.y;
    const bool live = s.live;
    pl.x[k] = x; pl.y[k] = y; pl.w[k] = s.w;
    pl.ux[k] = 0.0; pl.uy[k] = 0.0; pl.psi[k] = 1.0;
    pl.x_prev[k] = x; pl.y_prev[k] = y;
    pl.ux_half[k] = 0.0; pl.uy_half[k] = 0.0; pl.psi_half[k] = live ? 1.0 : 0.0;
    // a keyed species carries its slot index + 1 in the id bits (k_init_plasma)
    pl.idcpu[k] = (live ? HPS_ID_VALID : 0ULL) | ((keyed ? (unsigned long long)(k + 1) : 1ULL) << 24);
    pl.ion_lev[k] = level;
}

// <plasma>.u_mean, u_std: u = u_mean + u_std n with three standard normal deviates per primary slot k (ParticleUtil.H:113-124).
// Every draw is a function of (seed, species, time step, slot, draw) -- `key` is the chain up to the step -- so the sheet
// does not depend on the launch: Box-Muller on draws (0, 1) gives n_x, n_y, its cosine branch on draws (2, 3) n_z.
// do_symmetrize (:317-370): the primary slots are [0, nq), copy m = 1, 2, 3 of slot k is slot k + m nq at the position
// mirrored in x, in y, in both, with the momentum mirrored likewise; the weights arrive divided by 4 (:173-177).
struct WarmInit {
    double u_mean[3], u_std[3], c; unsigned long long key;
    double xoff, yoff, x_mid2, y_mid2;
};

template <bool SYM, bool PROG>
__global__ __launch_bounds__(256)
void k_init_plasma_warm (hps_plasma pl, long nq, int nx, int ny, FineInit a, WarmInit t, double lox, double loy, double dx, double dy,
                         int level, int keyed, const double* __restrict__ prof, int nr, double ft, DensityProgram dp)
{
    const long k = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (k >= nq) return;
    const SlotInit s = init_slot<PROG>(k, nx, ny, a, lox, loy, dx, dy, prof, nr, ft, dp, t.xoff, t.yoff);
    const bool live = s.live;
    const unsigned long long zk = coll_hash(t.key, (unsigned long long)k);
    double u[3] = {t.u_mean[0], t.u_mean[1], t.u_mean[2]};
    if (t.u_std[0] != 0.0 || t.u_std[1] != 0.0) {
        double n0, n1;
        normal_pair(zk, 0u, n0, n1);
        if (t.u_std[0] != 0.0) u[0] += t.u_std[0]*n0;
        if (t.u_std[1] != 0.0) u[1] += t.u_std[1]*n1;
    }
    if (t.u_std[2] != 0.0) {
        double n2, unused;
        normal_pair(zk, 2u, n2, unused);
        u[2] += t.u_std[2]*n2;
    }
    const double ux = u[0]*t.c, uy = u[1]*t.c;
    const double psi = sqrt(1.0 + u[0]*u[0] + u[1]*u[1] + u[2]*u[2]) - u[2];      // (:298) > 0 always
#pragma unroll
    for (int m = 0; m < (SYM ? 4 : 1); ++m) {
        const long o = k + m*nq;
        const double x = (m & 1) ? t.x_mid2 - s.x : s.x, y = (m & 2) ? t.y_mid2 - s.y : s.y;
        const double mux = (m & 1) ? -ux : ux, muy = (m & 2) ? -uy : uy;
        pl.x[o] = x; pl.y[o] = y; pl.w[o] = s.w;
        pl.ux[o] = mux; pl.uy[o] = muy; pl.psi[o] = psi;
        pl.x_prev[o] = x; pl.y_prev[o] = y;
        pl.ux_half[o] = mux; pl.uy_half[o] = muy; pl.psi_half[o] = live ? psi : 0.0;
        pl.idcpu[o] = (live ? HPS_ID_VALID : 0ULL) | ((keyed ? (unsigned long long)(o + 1) : 1ULL) << 24);
        pl.ion_lev[o] = level;
    }
}

// the kernels' view of one species' patch and weights; wdiv = 4 with do_symmetrize (:173-177)
static FineInit fine_args (const Engine& E, const Engine::Species& s, double density, double radius_sq, double wdiv)
{
    const hps_deck& d = E.d;
    const int *ppc = s.ppc, *fine = s.fine_ppc;
    const bool patch = E.fine_patch_set && fine[0] > 0;
    FineInit a{};
    a.level = patch ? E.d_fine_level : nullptr;
    a.cells = patch ? E.d_fine_cells : nullptr;
    a.ncells = patch ? E.fine_ncells : 0;
    a.cx = ppc[0]; a.cy = ppc[1];
    a.fx = patch ? fine[0] : ppc[0]; a.fy = patch ? fine[1] : ppc[1];
    a.T = E.fine_T;
    a.ncoarse = (long)a.cx*a.cy*d.nx*d.ny;
    const double vol = d.si_units ? E.gm.dx*E.gm.dy*E.gm.dz : 1.0;
    a.w_coarse = density*(vol/(a.cx*a.cy))/wdiv;
    a.w_fine = density*(vol/(a.fx*a.fy))/wdiv;
    a.radius_sq = radius_sq;
    a.hollow_sq = E.hollow_core_radius*E.hollow_core_radius;
    return a;
}

int init_plasma_fine (Engine& E, const Engine::Species& s, double radius_sq)
{
    const hps_deck& d = E.d;
    const DensityProgram dp = E.density_program(s.index);
    const bool prog = dp.n_ins > 0;
    const FineInit a = fine_args(E, s, prog ? 1.0 : s.density, radius_sq, 1.0);
    const long n = s.pl.n;
    if (n != a.ncoarse + (long)(a.fx*a.fy - a.cx*a.cy)*a.ncells) { set_error("init_plasma_fine: the sheet does not have the patch's slot count"); return HPS_ERR_ARG; }
    if (prog)
        hipLaunchKernelGGL(k_init_plasma_fine<true>, dim3(ceil_div(n, 256)), dim3(256), E.density_lds(s.index), E.st, s.pl, n, d.nx, d.ny, a,
                           d.lo[0], d.lo[1], E.gm.dx, E.gm.dy, s.init_level, s.keyed, E.d_prof_r, (int)E.prof_r.size(), E.prof_ft, dp);
    else
        hipLaunchKernelGGL(k_init_plasma_fine<false>, dim3(ceil_div(n, 256)), dim3(256), 0, E.st, s.pl, n, d.nx, d.ny, a, d.lo[0], d.lo[1],
                           E.gm.dx, E.gm.dy, s.init_level, s.keyed, E.d_prof_r, (int)E.prof_r.size(), E.prof_ft, dp);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int init_plasma_warm (Engine& E, const Engine::Species& s, double radius_sq)
{
    const hps_deck& d = E.d;
    const bool sym = E.do_symmetrize;
    const DensityProgram dp = E.density_program(s.index);
    const bool prog = dp.n_ins > 0;
    const FineInit a = fine_args(E, s, prog ? 1.0 : s.density, radius_sq, sym ? 4.0 : 1.0);
    const long nq = a.ncoarse + (long)(a.fx*a.fy - a.cx*a.cy)*a.ncells;
    if (s.pl.n != (sym ? 4 : 1)*nq) { set_error("init_plasma_warm: the sheet does not have the slot count of its keys"); return HPS_ERR_ARG; }
    const Engine::Thermal& th = s.thermal;
    WarmInit t{};
    for (int q = 0; q < 3; ++q) { t.u_mean[q] = th.u_mean[q]; t.u_std[q] = th.u_std[q]; }
    t.c = E.gm.c;
    t.key = coll_hash(coll_hash(th.seed, (unsigned long long)s.index), (unsigned long long)E.step_index);
    t.xoff = E.shifted(s.ppc, 0) ? -0.5 : 0.0;
    t.yoff = E.shifted(s.ppc, 1) ? -0.5 : 0.0;
    t.x_mid2 = d.lo[0] + d.hi[0]; t.y_mid2 = d.lo[1] + d.hi[1];       // of the particle boundary box (:319-320)
    const dim3 grid(ceil_div(nq, 256)), block(256);
#define CALL(SYM, PROG, LDS) hipLaunchKernelGGL((k_init_plasma_warm<SYM, PROG>), grid, block, LDS, E.st, s.pl, nq, d.nx, d.ny, a, t, d.lo[0], d.lo[1], \
                                                E.gm.dx, E.gm.dy, s.init_level, s.keyed, E.d_prof_r, (int)E.prof_r.size(), E.prof_ft, dp)
    if (prog) { if (sym) CALL(true, true, E.density_lds(s.index)); else CALL(false, true, E.density_lds(s.index)); }
    else      { if (sym) CALL(true, false, 0); else CALL(false, false, 0); }
#undef CALL
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// (PlasmaParticleContainerInit.cpp:52-64: with the fine patch the level map would have to live on the shifted box)
static const char* const PREVENT_VS_PATCH = "prevent_centered_particle cannot be combined with the fine plasma patch (fine_ppc, fine_patch)";

static bool divisible (const int* fine, const int* ppc)
{
    return fine[0] > 0 && fine[1] > 0 && ppc[0] > 0 && ppc[1] > 0 && fine[0] % ppc[0] == 0 && fine[1] % ppc[1] == 0;
}

int Engine::set_plasma_init (const int* plasma_fine, const int* ion_fine, double hollow_core)
{
    HPS_REQUIRE(!step_begun && !el.tiling, "hps_engine_set_plasma_init: call before the first hps_engine_begin_step");
    const int none[2] = {0, 0};
    const int* pf = plasma_fine ? plasma_fine : none;
    const int* jf = ion_fine ? ion_fine : none;
    const bool p_on = pf[0] != 0 || pf[1] != 0, i_on = jf[0] != 0 || jf[1] != 0;
    // (PlasmaParticleContainer.cpp:158-163)
    HPS_REQUIRE(!p_on || (el.present() && divisible(pf, el.ppc)), "hps_engine_set_plasma_init: plasma fine_ppc must be positive and divisible by ppc, component by component");
    HPS_REQUIRE(!i_on || (ions.present() && divisible(jf, ions.ppc)), "hps_engine_set_plasma_init: ion fine_ppc needs the ion species and must be positive and divisible by its ppc, component by component");
    HPS_REQUIRE(!(prevent_centered && (p_on || i_on)), PREVENT_VS_PATCH);
    // (:126-128; radius 0 = infinite)
    HPS_REQUIRE(hollow_core >= 0.0 && (d.plasma_radius <= 0.0 || hollow_core < d.plasma_radius),
                "hps_engine_set_plasma_init: the hollow core radius must not be negative and must be smaller than the plasma radius");
    el.fine_ppc[0] = pf[0]; el.fine_ppc[1] = pf[1]; ions.fine_ppc[0] = jf[0]; ions.fine_ppc[1] = jf[1];
    hollow_core_radius = hollow_core;
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    return alloc_sheets();
}

int Engine::set_plasma_momentum (int species, const double* u_mean, const double* u_std, unsigned long long seed)
{
    HPS_REQUIRE(!step_begun && !el.tiling, "hps_engine_set_plasma_momentum: call before the first hps_engine_begin_step");
    HPS_REQUIRE(plasma_species_ok(species), "hps_engine_set_plasma_momentum: species must be 0 (plasma), 1 (ion) or the index of an added species");
    HPS_REQUIRE(sp[species].present(), "hps_engine_set_plasma_momentum: the deck does not have this species (no plasma, or no ion species)");
    HPS_REQUIRE(u_mean && u_std, "hps_engine_set_plasma_momentum: null argument");
    for (int q = 0; q < 3; ++q)
        HPS_REQUIRE(std::isfinite(u_mean[q]) && std::isfinite(u_std[q]) && u_std[q] >= 0.0, "hps_engine_set_plasma_momentum: u_std must not be negative (and u_mean, u_std finite)");
    Thermal& th = sp[species].thermal;
    for (int q = 0; q < 3; ++q) { th.u_mean[q] = u_mean[q]; th.u_std[q] = u_std[q]; }
    th.seed = seed;
    return HPS_OK;
}

int Engine::set_plasma_symmetry (int symmetrize, int prevent_centered_particle)
{
    HPS_REQUIRE(!step_begun && !el.tiling, "hps_engine_set_plasma_symmetry: call before the first hps_engine_begin_step");
    bool any_fine = fine_patch_set;
    for (const Species& q : sp) any_fine = any_fine || q.fine_ppc[0] > 0;
    HPS_REQUIRE(!(prevent_centered_particle && any_fine), PREVENT_VS_PATCH);
    do_symmetrize = symmetrize != 0; prevent_centered = prevent_centered_particle != 0;
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    return alloc_sheets();
}

int Engine::set_fine_patch (const unsigned char* mask_host, int transition_cells)
{
    HPS_REQUIRE(!step_begun && !el.tiling, "hps_engine_set_fine_patch: call before the first hps_engine_begin_step");
    HPS_REQUIRE(mask_host, "hps_engine_set_fine_patch: null mask");
    HPS_REQUIRE(!prevent_centered, PREVENT_VS_PATCH);
    HPS_REQUIRE(transition_cells >= 0, "hps_engine_set_fine_patch: fine_transition_cells must not be negative");
    const int nx = d.nx, ny = d.ny, T = transition_cells;
    // the map lives on the cell box cropped to the plasma radius (:70-82); nothing outside it is looked at
    int ilo = 0, ihi = nx - 1, jlo = 0, jhi = ny - 1;
    if (d.plasma_radius > 0.0) {
        const double R = d.plasma_radius;
        // (clamped as doubles: a huge radius must not overflow the int)
        auto cell = [] (double v, int lo, int hi) { return static_cast<int>(std::min<double>(std::max<double>(std::round(v), lo), hi)); };
        ilo = cell((-R - d.lo[0])/gm.dx - 2, 0, nx);
        jlo = cell((-R - d.lo[1])/gm.dy - 2, 0, ny);
        ihi = cell(( R - d.lo[0])/gm.dx + 2, -1, nx - 1);
        jhi = cell(( R - d.lo[1])/gm.dy + 2, -1, ny - 1);
    }
    std::vector<int> L((size_t)nx*ny, 0), B;
    for (int j = jlo; j <= jhi; ++j)
        for (int i = ilo; i <= ihi; ++i)
            if (mask_host[(size_t)j*nx + i]) L[(size_t)j*nx + i] = T + 1;
    // T passes of max(own, neighbour - 1) over the 4-neighbourhood inside the box (:117-138)
    for (int iter = 0; iter < T; ++iter) {
        B = L;
        for (int j = jlo; j <= jhi; ++j)
            for (int i = ilo; i <= ihi; ++i) {
                const size_t o = (size_t)j*nx + i;
                int m = B[o];
                if (i > ilo) m = std::max(m, B[o - 1] - 1);
                if (i < ihi) m = std::max(m, B[o + 1] - 1);
                if (j > jlo) m = std::max(m, B[o - nx] - 1);
                if (j < jhi) m = std::max(m, B[o + nx] - 1);
                L[o] = m;
            }
    }
    std::vector<int> cells;
    for (size_t o = 0; o < L.size(); ++o) if (L[o] > 0) cells.push_back((int)o);
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    (void)hipFree(d_fine_level); (void)hipFree(d_fine_cells); d_fine_level = d_fine_cells = nullptr;
    HPS_HIP_CHECK(hipMalloc(&d_fine_level, L.size()*sizeof(int)));
    HPS_HIP_CHECK(hipMemcpy(d_fine_level, L.data(), L.size()*sizeof(int), hipMemcpyHostToDevice));
    HPS_HIP_CHECK(hipMalloc(&d_fine_cells, std::max<size_t>(cells.size(), 1)*sizeof(int)));
    if (!cells.empty()) HPS_HIP_CHECK(hipMemcpy(d_fine_cells, cells.data(), cells.size()*sizeof(int), hipMemcpyHostToDevice));
    fine_patch_set = true; fine_T = T; fine_ncells = (long)cells.size();
    return alloc_sheets();
}

// hps_engine_set_density_expr: every program is checked before anything changes; then the engine's one image is
// rebuilt from every species' programs
int Engine::set_density_expr (int species, int n_progs, const hps_expr* progs, const double* z_pos, double min_density)
{
    static const char* const fn = "hps_engine_set_density_expr";
    HPS_REQUIRE(!step_begun, std::string(fn) + ": call before the first hps_engine_begin_step");
    HPS_REQUIRE(plasma_species_ok(species), std::string(fn) + ": species must be 0 (plasma), 1 (ion) or the index of an added species");
    HPS_REQUIRE(sp[species].present(), std::string(fn) + ": the deck does not have this species (no plasma, or no ion species)");
    HPS_REQUIRE(n_progs >= 1 && progs, std::string(fn) + ": n_progs must be >= 1 (at least one program)");
    HPS_REQUIRE(n_progs == 1 || z_pos, std::string(fn) + ": several programs need their positions (z_pos)");
    HPS_REQUIRE(!std::isnan(min_density), std::string(fn) + ": min_density is NaN");
    for (int k = 0; z_pos && k < n_progs; ++k)
        HPS_REQUIRE(std::isfinite(z_pos[k]) && (k == 0 || z_pos[k] > z_pos[k - 1]), std::string(fn) + ": the positions of the density table must be finite and strictly ascending");
    int depth = 0;
    for (int k = 0; k < n_progs; ++k) {
        int dk = 0;
        const std::string what = n_progs > 1 ? "entry " + std::to_string(k) + ": " : std::string();
        if (int e = expr_check_named(fn, what.c_str(), &progs[k], 3, &dk)) return e;
        depth = std::max(depth, dk);
    }
    DensityExpr& D = sp[species].dens;
    D = DensityExpr{};
    for (int k = 0; k < n_progs; ++k) {
        D.ins.emplace_back(progs[k].ins, progs[k].ins + progs[k].n_ins);
        D.consts.emplace_back(progs[k].consts, progs[k].consts + progs[k].n_const);
    }
    if (z_pos) D.z_pos.assign(z_pos, z_pos + n_progs);
    D.depth = depth; D.min_density = min_density; D.on = true;
    ExprImage image;
    for (Species& q : sp) {
        DensityExpr& S = q.dens;
        S.off.clear();
        for (size_t k = 0; k < S.ins.size(); ++k)
            S.off.push_back(image.add(hps_expr{(int)S.ins[k].size(), (int)S.consts[k].size(), S.ins[k].data(), S.consts[k].data()}));
    }
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    dens_image = ExprImage{};
    if (int e = image.upload()) return e;
    dens_image = std::move(image);
    return HPS_OK;
}

// UpdateDensityFunction (PlasmaParticleContainer.cpp:211-217): std::map::lower_bound -- the first entry with z_pos >= z, the
// last one beyond the table
void Engine::density_begin_step (double ct)
{
    dens_z = ct;
    for (Species& q : sp) {
        DensityExpr& S = q.dens;
        if (!S.on || S.z_pos.empty()) { S.cur = 0; continue; }
        const size_t k = std::lower_bound(S.z_pos.begin(), S.z_pos.end(), ct) - S.z_pos.begin();
        S.cur = (int)std::min(k, S.z_pos.size() - 1);
    }
}

DensityProgram Engine::density_program (int species) const
{
    const DensityExpr& S = sp[species].dens;
    if (!S.on) return DensityProgram{nullptr, 0, nullptr, 0.0, 0.0};
    return DensityProgram{dens_image.ins() + S.off[S.cur], (int)S.ins[S.cur].size(), dens_image.consts(), dens_z, S.min_density};
}

} // namespace hps

extern "C" int hps_engine_set_density_expr (void* h, int species, int n_progs, const hps_expr* progs, const double* z_pos, double min_density)
{
    HPS_REQUIRE(h, "hps_engine_set_density_expr: null engine");
    return static_cast<hps::Engine*>(h)->set_density_expr(species, n_progs, progs, z_pos, min_density);
}
