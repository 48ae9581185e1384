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
#include "engine.h"

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

__global__ __launch_bounds__(256)
void k_init_plasma_fine (hps_plasma pl, long n, int nx, int ny, FineInit a, double lox, double loy, double dx, double dy,
                         int level, int keyed, const double* __restrict__ prof, int nr, double ft)
{
    const long k = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (k >= n) return;
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
    const double x = lox + (i + rx)*dx;
    const double y = loy + (j + ry)*dy;
    // <plasma>.radius, hollow_core_radius and the density (PlasmaParticleContainerInit.cpp:274-279)
    const double rsq = x*x + y*y;
    const double fac = (rsq > a.radius_sq || rsq < a.hollow_sq) ? 0.0 : ft*table_value(prof, prof + nr, nr, sqrt(rsq));
    const double weight = L == 0 ? a.w_coarse : a.w_fine;      // (:289-294)
    pl.x[k] = x; pl.y[k] = y; pl.w[k] = fac > 0.0 ? weight*fac : 0.0;
    pl.ux[k] = 0.0; pl.uy[k] = 0.0; pl.psi[k] = 1.0;
    pl.x_prev[k] = x; pl.y_prev[k] = y;
    pl.ux_half[k] = 0.0; pl.uy_half[k] = 0.0; pl.psi_half[k] = fac > 0.0 ? 1.0 : 0.0;
    // a keyed species carries its slot index + 1 in the id bits (k_init_plasma)
    pl.idcpu[k] = (fac > 0.0 ? HPS_ID_VALID : 0ULL) | ((keyed ? (unsigned long long)(k + 1) : 1ULL) << 24);
    pl.ion_lev[k] = level;
}

int init_plasma_fine (Engine& E, const hps_plasma& p, long n, const int ppc[2], const int fine[2], double density, int level, int keyed,
                      double radius_sq)
{
    const hps_deck& d = E.d;
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
    a.w_coarse = density*(vol/(a.cx*a.cy));
    a.w_fine = density*(vol/(a.fx*a.fy));
    a.radius_sq = radius_sq;
    a.hollow_sq = E.hollow_core_radius*E.hollow_core_radius;
    if (n != a.ncoarse + (long)(a.fx*a.fy - a.cx*a.cy)*a.ncells) { set_error("init_plasma_fine: the sheet does not have the patch's slot count"); return HPS_ERR_ARG; }
    hipLaunchKernelGGL(k_init_plasma_fine, dim3(ceil_div(n, 256)), dim3(256), 0, E.st, p, n, d.nx, d.ny, a, d.lo[0], d.lo[1],
                       E.gm.dx, E.gm.dy, level, keyed, E.d_prof_r, (int)E.prof_r.size(), E.prof_ft);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

static bool divisible (const int* fine, const int* ppc)
{
    return fine[0] > 0 && fine[1] > 0 && ppc[0] > 0 && ppc[1] > 0 && fine[0] % ppc[0] == 0 && fine[1] % ppc[1] == 0;
}

int Engine::set_plasma_init (const int* plasma_fine, const int* ion_fine, double hollow_core)
{
    HPS_REQUIRE(!step_begun && !tiling, "hps_engine_set_plasma_init: call before the first hps_engine_begin_step");
    const int none[2] = {0, 0};
    const int* pf = plasma_fine ? plasma_fine : none;
    const int* jf = ion_fine ? ion_fine : none;
    const bool p_on = pf[0] != 0 || pf[1] != 0, i_on = jf[0] != 0 || jf[1] != 0;
    // (PlasmaParticleContainer.cpp:158-163)
    HPS_REQUIRE(!p_on || (d.plasma_density > 0.0 && divisible(pf, d.plasma_ppc)), "hps_engine_set_plasma_init: plasma fine_ppc must be positive and divisible by ppc, component by component");
    HPS_REQUIRE(!i_on || (d.ion_on && divisible(jf, d.ion_ppc)), "hps_engine_set_plasma_init: ion fine_ppc needs the ion species and must be positive and divisible by its ppc, component by component");
    // (:126-128; radius 0 = infinite)
    HPS_REQUIRE(hollow_core >= 0.0 && (d.plasma_radius <= 0.0 || hollow_core < d.plasma_radius),
                "hps_engine_set_plasma_init: the hollow core radius must not be negative and must be smaller than the plasma radius");
    fine_ppc[0] = pf[0]; fine_ppc[1] = pf[1]; ion_fine_ppc[0] = jf[0]; ion_fine_ppc[1] = jf[1];
    hollow_core_radius = hollow_core;
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    return alloc_sheets();
}

int Engine::set_fine_patch (const unsigned char* mask_host, int transition_cells)
{
    HPS_REQUIRE(!step_begun && !tiling, "hps_engine_set_fine_patch: call before the first hps_engine_begin_step");
    HPS_REQUIRE(mask_host, "hps_engine_set_fine_patch: null mask");
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

} // namespace hps
