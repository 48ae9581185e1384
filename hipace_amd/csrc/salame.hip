// salame.hip -- the operators of the SALAME module (salame/Salame.cpp of the reference): the only-advance push, the
// pointwise kernels on the SALAME planes, the deterministic reduction behind the weight factor W, and the scaling of a
// beam slice's weights; and the per-slice sequence that calls them, Engine::salame_module, with set_beam_species_salame and
// salame_solve_ez.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

namespace hps {

// SalameOnlyAdvancePlasma (Salame.cpp:262-339): one particle per lane in sheet order (the sheet is tile-sorted, so
// neighbouring lanes gather from neighbouring cells).  Gathers Bx, By at (x_prev, y_prev) with the plain shape
// (doBxByGatherShapeN), writes ux, uy, touches nothing else.  a = 1.5 dz charge / mass.
template <int ORDER>
__global__ __launch_bounds__(256)
void k_salame_only_advance (SlabView f, hps_plasma pl, int cBx, int cBy, double a, int can_ionize,
                            double dx_inv, double dy_inv, double xoff, double yoff)
{
    const long ip = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (ip >= pl.n) return;
    if (!(pl.idcpu[ip] & HPS_ID_VALID)) return;
    double sx[ORDER + 1], sy[ORDER + 1];
    const int i0 = shape_weights<ORDER>((pl.x_prev[ip] - xoff)*dx_inv, sx);
    const int j0 = shape_weights<ORDER>((pl.y_prev[ip] - yoff)*dy_inv, sy);
    // (a particle of the box never reaches beyond the guard cells; one that is not of the box is left alone)
    if (i0 < -f.ng || i0 + ORDER >= f.nx + f.ng || j0 < -f.ng || j0 + ORDER >= f.ny + f.ng) return;
    double Bxp = 0.0, Byp = 0.0;
#pragma unroll
    for (int iy = 0; iy <= ORDER; ++iy) {
        const long row = f.off(i0, j0 + iy);
#pragma unroll
        for (int ix = 0; ix <= ORDER; ++ix) {
            const double s = sx[ix]*sy[iy];
            Bxp += s*f.p[cBx*f.ns + row + ix];
            Byp += s*f.p[cBy*f.ns + row + ix];
        }
    }
    const double q = can_ionize ? (double)pl.ion_lev[ip]*a : a;
    pl.ux[ip] =  q*Byp;
    pl.uy[ip] = -q*Bxp;
}

// SalameGetJxJyFromBxBy (Salame.cpp:228-260), valid cells; fac = 1.5 dz / mu0
__global__ __launch_bounds__(256)
void k_salame_jxjy_from_bxby (SlabView f, int cBx, int cBy, int cChi, int cJx, int cJy, double dz15, double mu0_inv)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= f.nx) return;
    const long o = f.off(i, j);
    const double chi = f.p[cChi*f.ns + o];
    f.p[cJx*f.ns + o] =  dz15*chi*f.p[cBy*f.ns + o]*mu0_inv;
    f.p[cJy*f.ns + o] = -dz15*chi*f.p[cBx*f.ns + o]*mu0_inv;
}

// SalameInitializeSxSyWithBeam (Salame.cpp:192-225), valid cells
__global__ __launch_bounds__(256)
void k_salame_sxsy_from_jz (SlabView f, int cJz, int cSy, int cSx, double mu0, double dxih, double dyih)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= f.nx) return;
    const long o = f.off(i, j);
    const double* J = f.p + cJz*f.ns + o;
    const double dx_jzb = (J[1] - J[-1])*dxih;
    const double dy_jzb = (J[f.js] - J[-f.js])*dyih;
    f.p[cSy*f.ns + o] =  mu0*(-dy_jzb);
    f.p[cSx*f.ns + o] = -mu0*(-dx_jzb);
}

// The four sums of SalameGetW over the valid cells.  Workgroup b of nb takes the cells b*256 + t, (b + nb)*256 + t, ... in
// that order (nb depends on the grid size only), a wave folds by a fixed butterfly, the four waves and then the workgroups'
// partial sums are added in index order: no atomics, the same planes give the same bits.
constexpr int GETW_MAX_WG = 256;
__global__ __launch_bounds__(256)
void k_salame_get_w (SlabView f, int cT, int cN, int cE, int cJ, double* __restrict__ part)
{
    const long cells = (long)f.nx*f.ny;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long c = (long)blockIdx.x*256 + threadIdx.x; c < cells; c += (long)gridDim.x*256) {
        const int j = (int)(c / f.nx), i = (int)(c - (long)j*f.nx);
        const long o = f.off(i, j);
        const double jz = f.p[cJ*f.ns + o];
        s[0] += jz*f.p[cT*f.ns + o]; s[1] += jz*f.p[cN*f.ns + o]; s[2] += jz*f.p[cE*f.ns + o]; s[3] += jz;
    }
    __shared__ double w4[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) w4[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) part[(long)blockIdx.x*4 + threadIdx.x] = ((w4[0][threadIdx.x] + w4[1][threadIdx.x]) + w4[2][threadIdx.x]) + w4[3][threadIdx.x];
}
// ordered fold of the nb partial sums: lane q adds part[0][q], part[1][q], ... and stores the sum behind them
__global__ __launch_bounds__(64)
void k_salame_fold_w (double* __restrict__ part, int nb)
{
    if (threadIdx.x >= 4) return;
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += part[(long)b*4 + threadIdx.x];
    part[(long)GETW_MAX_WG*4 + threadIdx.x] = v;
}

// SalameMultiplyBeamWeight (Salame.cpp:407-437)
__global__ __launch_bounds__(256)
void k_salame_scale_w (double* __restrict__ w, long n, double W)
{
    const long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (t >= n) return;
    w[t] = (W == 0.0) ? 0.0 : w[t]*W;
}

// ... on slice p of a moving-beam engine's container (beam.hip): the particles [B[p] + nfront[p], B[p + 1]) -- those that have
// not slipped in during this step -- whose species is in mask and that are not absorbed.  Every lane owns its particle: no
// atomics.  W == 0: gone, as the push's absorbing boundary leaves a particle (beam_push.h: w = 0, nsub = -1).
__global__ __launch_bounds__(256)
void k_salame_scale_moving (BeamSoA b, const long* __restrict__ B, const int* __restrict__ nfront, int p, unsigned mask, double W)
{
    const long first = B[p] + nfront[p], count = B[p + 1] - first;
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
        const long ip = first + t;
        if (!(mask >> b.sp[ip] & 1u) || b.nsub[ip] < 0) continue;
        if (W == 0.0) { b.w[ip] = 0.0; b.nsub[ip] = -1; }
        else b.w[ip] *= W;
    }
}

int salame_scale_moving (Engine& E, int p, unsigned mask, double W)
{
    if (p < 0 || p >= E.d.nz || !E.multi_beam() || (mask & E.species_mask_all()) == 0) return HPS_OK;
    const long bound = E.beam_bound(p);
    if (bound <= 0) return HPS_OK;
    const dim3 grid((unsigned)std::min<long>(ceil_div(bound, 256), 2048));
    hipLaunchKernelGGL(k_salame_scale_moving, grid, dim3(256), 0, E.st, E.bm, E.d_B, E.d_nfront, p, mask, W);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

static bool comp_ok (const hps_slab& s, int c) { return c >= 0 && c < s.ncomp; }

int salame_get_w_enqueue (const hps_slab& slab, int cT, int cN, int cE, int cJ, double* scratch, hipStream_t st)
{
    const int nb = std::min<long>(GETW_MAX_WG, std::max<long>(1, ceil_div((long)slab.nx*slab.ny, 256)));
    hipLaunchKernelGGL(k_salame_get_w, dim3(nb), dim3(256), 0, st, SlabView(slab), cT, cN, cE, cJ, scratch);
    hipLaunchKernelGGL(k_salame_fold_w, dim3(1), dim3(64), 0, st, scratch, nb);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}
const double* salame_get_w_result (const double* scratch) { return scratch + (long)GETW_MAX_WG*4; }


// staging = fa * d(A)/d(da) + fb * d(B)/d(db), centred differences (LinCombination + derivative,
// fields/Fields.cpp:223-249,368-387); dir 0 = x, 1 = y
__global__ __launch_bounds__(256)
void k_rhs_lincomb (SlabView f, int cA, int dirA, double fa, int cB, int dirB, double fb, double* staging)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= f.nx) return;
    const long o = f.off(i, j);
    const long sa = dirA == 0 ? 1 : f.js, sb = dirB == 0 ? 1 : f.js;
    const double* A = f.p + cA*f.ns + o;
    const double* B = f.p + cB*f.ns + o;
    staging[(long)j*f.nx + i] = fa*(A[sa] - A[-sa]) + fb*(B[sb] - B[-sb]);
}


// hps_engine_set_beam_species_salame: a do_salame species will be added to this moving-beam engine.  What Engine::create gives a
// beam_do_salame deck, allocated now: the SALAME planes behind the engine's own (the slab holds nothing but begin_step's zeros
// yet), the W reduction's scratch and statistics, the plasma sheet with x_prev, y_prev of their own (alloc_sheets, as the other
// setters of the sheet call it again).
int Engine::set_beam_species_salame (int on)
{
    static const std::string fn = "hps_engine_set_beam_species_salame: ";
    if (!on) return HPS_OK;
    if (species_salame) return HPS_OK;
#define HPS_REFUSE(cond, msg) do { if (cond) { set_error(fn + msg); return HPS_ERR_UNSUPPORTED; } } while (0)
    HPS_REFUSE(d.beam_do_salame, "the deck has beam_do_salame: that is the one beam of a static-beam engine, a do_salame species belongs to a moving-beam engine");
    HPS_REFUSE(!moving, "beam_species_salame needs a moving beam (hipace.dt != 0 or adaptive): a static beam (dt = 0) has no species; its one beam takes beam_do_salame");
    HPS_REFUSE(pc, "beam_species_salame needs the explicit solver (Hipace.cpp:152), not the predictor-corrector");
    HPS_REFUSE(d.ion_on, "beam_species_salame with the ionisable species (ion_on) is not supported");
    HPS_REFUSE(d.laser_on, "beam_species_salame with a laser is not supported");
    HPS_REFUSE(further(), "beam_species_salame with a further plasma species (hps_engine_add_plasma_species) is not supported: SALAME drives the electrons alone");
#undef HPS_REFUSE
    HPS_REQUIRE(!step_begun && !el.tiling && steps_begun == 0 && bsp.empty() && coll.empty() && !fine_patch_set,
                fn + "call behind hps_engine_create, ahead of the other setters, of hps_engine_add_beam_species and of the first hps_engine_begin_step");
    HPS_REQUIRE(d.salame_n_iter >= 0 && d.salame_relative_tolerance >= 0.0, fn + "salame_n_iter and salame_relative_tolerance must not be negative");
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    double* grown = nullptr;
    const size_t bytes = (size_t)slab.nstride*(slab.ncomp + (int)HPS_SAL_NCOMP)*sizeof(double);
    HPS_HIP_CHECK(hipMalloc(&grown, bytes));
    if (hipMemset(grown, 0, bytes) != hipSuccess || hipMalloc(&d_sal, (size_t)4*257*sizeof(double)) != hipSuccess) {
        (void)hipFree(grown); set_error(fn + "allocation of the SALAME slice failed"); return HPS_ERR_HIP; }
    (void)hipFree(slab.p);
    slab.p = grown;
    c_sal = slab.ncomp;                      // (= ncomp: a moving-beam engine has no alternates of the re-initialised planes)
    slab.ncomp += (int)HPS_SAL_NCOMP;
    sal_stats.assign((size_t)4*d.nz, 0.0);
    if (d.salame_n_iter == 0) d.salame_n_iter = 5;                                    // hipace.salame_n_iter (Hipace.H)
    if (d.salame_relative_tolerance == 0.0) d.salame_relative_tolerance = 1.0e-4;      // hipace.salame_relative_tolerance
    species_salame = true;
    el.temp_push = true;                     // the plasma is pushed to temporary slices from x_prev (Species::alias_prev)
    return alloc_sheets();
}

// SolvePoissonEz(WhichSlice::Salame) (fields/Fields.cpp:960-1006): Ez of the SALAME slice from its jx, jy
int Engine::salame_solve_ez ()
{
    const double fa = 1.0/(gm.ep0*gm.c);
    hipLaunchKernelGGL(k_rhs_lincomb, dim3(ceil_div(d.nx, 256), d.ny), dim3(256), 0, st, SlabView(slab), c_sal + HPS_SAL_JX, 0,
                       fa*0.5*(1.0/gm.dx), c_sal + HPS_SAL_JY, 1, fa*0.5*(1.0/gm.dy), staging);
    if (int e = open_boundary(1, 0x1u)) return e;       // (Ez: no physical monopole, fields/Fields.cpp:727-731)
    return hps_poisson_solve(ps, staging, slab, c_sal + HPS_SAL_EZ, st);
}

// SalameModule (salame/Salame.cpp:13-189) on level 0, statement by statement: with the one beam of a static-beam engine, or
// with the do_salame species of a moving-beam engine's container.  The fields of This
// are solved; the sheet holds the committed state of this slice (x_prev, y_prev, u_half) and is pushed to the temporary
// slice only.  The host reads W once per iteration, as the reference does.
int Engine::salame_module (int islice)
{
    SlabView f(slab);
    const dim3 b256(256);
    const CellBox bb{beam_box.ilo, beam_box.ihi, beam_box.jlo, beam_box.jhi}, none{0, -1, 0, -1};
    const int S = c_sal;
    const int comp_push[5] = {HPS_C_PSI, HPS_C_EZ, HPS_C_BX, HPS_C_BY, HPS_C_BZ};
    const int dep_jxjy[6] = {S + HPS_SAL_JX, S + HPS_SAL_JY, -1, -1, -1, -1};
    auto zero = [&] (std::initializer_list<int> cs) {
        CompList z{0, {}}; for (int c : cs) z.c[z.n++] = c;
        zero_comps(slab, st, z, CompList{0, {}}, none);
    };
    auto copy = [&] (std::initializer_list<int> dst, std::initializer_list<int> src) {
        CompList a{0, {}}, b{0, {}}; for (int c : dst) a.c[a.n++] = c; for (int c : src) b.c[b.n++] = c;
        copy_comps(slab, st, a, b);
    };
    auto solve_bxby = [&] (int cB, int cS) -> int {
        int iters = 0;
        if (int e = hps_mg_solve1(mg, slab, cB, cS, HPS_C_CHI, d.mg_tol_rel, d.mg_tol_abs, 200, &iters, nullptr, st)) return e;
        total_vcycles += iters;
        return HPS_OK;
    };
    int e;

    // always the Ez from before SALAME started, for a whole run of consecutive slices (:20-30)
    if (islice + 1 != sal_last_slice) {
        copy({S + HPS_SAL_EZ_TARGET}, {HPS_C_EZ});
        sal_overloaded = false;
        sal_zeta_initial = islice*gm.dz + d.lo[2] + 0.5*gm.dz;       // GetPosOffset(2, geom, domain) = lo_z + dz/2
    }
    sal_last_slice = islice;

    // Sx, Sy of the plasma alone, backed up ahead of any push (:32-39)
    zero({HPS_C_SY, HPS_C_SX});
    {   const int cache[4] = {HPS_C_BZ, HPS_C_EZ, HPS_C_EXMBY, HPS_C_EYPBX};
        const int depos[2] = {HPS_C_SY, HPS_C_SX};
        if ((e = species_explicit(el, cache, depos))) return e; }
    copy({S + HPS_SAL_SY_BACK, S + HPS_SAL_SX_BACK}, {HPS_C_SY, HPS_C_SX});

    // static beam: the slice's block; moving beam: the do_salame species of the container's slice (the deposits onto the SALAME
    // slice take them alone, MultiBeam.cpp:44-47; STEP 4's onto This takes every species)
    const long first0 = moving ? 0 : beam_off[d.nz - 1 - islice], count = moving ? 0 : beam_off[d.nz - islice] - first0;
    const unsigned smask = moving ? salame_mask() : 0u;
    auto deposit_salame = [&] (int cjz) -> int {
        return moving ? beam_deposit_species(*this, d.nz - 1 - islice, smask, -1, -1, cjz) : deposit_beam_slice(islice, -1, -1, cjz);
    };
    double W = 1.0, W_total = 0.0;
    int iter = 0, used = 0; bool converged = false, undetermined = false;
    for (; iter < d.salame_n_iter; ++iter) {
        // STEP 1: Ez of the next slice with the beam at its present weight (:43-73)
        if ((e = species_advance(el, comp_push, 1))) return e;
        copy({S + HPS_SAL_JX, S + HPS_SAL_JY}, {HPS_C_N_JXB, HPS_C_N_JYB});
        if ((e = species_deposit(el, dep_jxjy))) return e;
        zero({S + HPS_SAL_EZ, S + HPS_SAL_JZB, S + HPS_SAL_SY, S + HPS_SAL_SX, S + HPS_SAL_BX, S + HPS_SAL_BY});
        if ((e = salame_solve_ez())) return e;
        copy({S + HPS_SAL_EZ_NO_SALAME}, {S + HPS_SAL_EZ});

        // STEP 2: Ez of the SALAME beam alone (:75-121)
        if ((e = deposit_salame(S + HPS_SAL_JZB))) return e;
        if ((e = hps_salame_sxsy_from_jz(slab, gm, S + HPS_SAL_JZB, S + HPS_SAL_SY, S + HPS_SAL_SX, st))) return e;
        if ((e = solve_bxby(S + HPS_SAL_BX, S + HPS_SAL_SY))) return e;       // zero guess, This chi
        zero({S + HPS_SAL_EZ, S + HPS_SAL_JX, S + HPS_SAL_JY});
        if (!d.salame_no_advance) {
            if (el.pl.n > 0) { if ((e = hps_salame_only_advance(slab, el.pl, gm, S + HPS_SAL_BX, S + HPS_SAL_BY, el.charge, el.mass, d.order, 0, st))) return e; }
            if ((e = species_deposit(el, dep_jxjy))) return e;
        } else {
            if ((e = hps_salame_jxjy_from_bxby(slab, gm, S + HPS_SAL_BX, S + HPS_SAL_BY, HPS_C_CHI, S + HPS_SAL_JX, S + HPS_SAL_JY, st))) return e;
        }
        if ((e = salame_solve_ez())) return e;

        // STEP 3: the weight factor (:123-158)
        zero({S + HPS_SAL_JZB});
        if ((e = deposit_salame(S + HPS_SAL_JZB))) return e;
        double s4[4];
        if ((e = salame_get_w_enqueue(slab, S + HPS_SAL_EZ_TARGET, S + HPS_SAL_EZ_NO_SALAME, S + HPS_SAL_EZ, S + HPS_SAL_JZB, d_sal, st))) return e;
        HPS_HIP_CHECK(hipMemcpyAsync(s4, salame_get_w_result(d_sal), sizeof(s4), hipMemcpyDeviceToHost, st));
        HPS_HIP_CHECK(hipStreamSynchronize(st));
        {   const double sum_jz = s4[3];
            double ez_target = s4[0]/sum_jz;
            const double ez_no = s4[1]/sum_jz, ez_only = s4[2]/sum_jz;
            const double zeta = (islice - 1)*gm.dz + d.lo[2] + 0.5*gm.dz;        // the Ez of the next slice (SalameGetW :395-400)
            ez_target += d.salame_Ez_target_slope*(zeta - sal_zeta_initial);    // salame_Ez_target(zeta, zeta_initial, Ez_initial)
            W = (ez_target - ez_no)/ez_only + 1.0;
            W_total = W*sum_jz;
            // No weight can be derived (the reference divides all the same and would multiply the weights by NaN).  A slice
            // without current -- every weight already 0, e.g. the dropped tail of an overloaded beam loaded again -- has nothing
            // to scale: W = 0, the run of slices is not marked overloaded by it.  A beam whose own Ez vanishes (sum jz != 0) keeps
            // its weights: W = 1.  Either way this was the slice's last iteration.
            // (Behind an overload the weight is 0 whatever the sums say, as before.)
            if (sal_overloaded) { }
            else if (sum_jz == 0.0) { W = 0.0; W_total = 0.0; undetermined = true; }
            else if (!std::isfinite(W)) { W = 1.0; W_total = sum_jz; undetermined = true; } }
        used = iter + 1;
        bool last = undetermined;
        if (!undetermined && (W < 0.0 || sal_overloaded)) { W = 0.0; W_total = 0.0; last = true; sal_overloaded = true; }
        if (!undetermined && !sal_overloaded && iter >= 1 && std::fabs(W - 1.0) < d.salame_relative_tolerance) { last = true; converged = true; }
        if (moving) { if ((e = salame_scale_moving(*this, d.nz - 1 - islice, smask, W))) return e; }
        else if ((e = hps_salame_scale_beam_slice(beam_cur + 7*first0 + 6*count, count, W, st))) return e;

        // STEP 4: the fields of This with the new weight (:160-182)
        {   CompList zb{0, {}}; zb.c[zb.n++] = HPS_C_JZB;
            zero_comps(slab, st, CompList{0, {}}, zb, bb); }
        if ((e = deposit_beam_slice(islice, -1, -1, HPS_C_JZB))) return e;
        deposit_grid_current(islice, HPS_C_JZB);
        // InitializeSxSyWithBeam writes Sx, Sy as whole planes (no zeroing pass), with Sy_back, Sx_back added in the same pass
        hipLaunchKernelGGL(k_sxsy_beam, dim3(ceil_div(slab.jstride, 256), d.ny + 2*g), b256, 0, st, f, HPS_C_SX, HPS_C_SY, HPS_C_JZB, HPS_C_N_JXB, HPS_C_N_JYB,
                           HPS_C_P_JXB, HPS_C_P_JYB, gm.mu0, 2.0*gm.dx, 2.0*gm.dy, 2.0*gm.dz, bb, S + HPS_SAL_SX_BACK, S + HPS_SAL_SY_BACK);
        if ((e = solve_bxby(HPS_C_BX, HPS_C_SY))) return e;
        if (last) break;
    }
    double* o = sal_stats.data() + (size_t)4*islice;
    o[0] = W; o[1] = W_total; o[2] = (double)used; o[3] = (converged ? 1.0 : 0.0) + (sal_overloaded ? 2.0 : 0.0);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

} // namespace hps

using namespace hps;

extern "C" int hps_salame_only_advance (hps_slab slab, hps_plasma pl, hps_geom g, int bx_comp, int by_comp, double charge,
                                        double mass, int order, int can_ionize, hps_stream stream)
{
    HPS_REQUIRE(order >= 0 && order <= 3, "hps_salame_only_advance: depos_order must be 0..3");
    if (int e = check_stencil(slab, (order + 1)/2, "hps_salame_only_advance")) return e;
    HPS_REQUIRE(comp_ok(slab, bx_comp) && comp_ok(slab, by_comp), "hps_salame_only_advance: bad component");
    HPS_REQUIRE(mass != 0.0, "hps_salame_only_advance: mass must not be 0");
    if (pl.n == 0) return HPS_OK;
    const double a = 1.5*g.dz*(charge/mass);
    const dim3 grid(ceil_div(pl.n, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    SlabView f(slab);
#define HPS_OA(O) hipLaunchKernelGGL(k_salame_only_advance<O>, grid, block, 0, st, f, pl, bx_comp, by_comp, a, can_ionize, 1.0/g.dx, 1.0/g.dy, g.xoff, g.yoff)
    switch (order) { case 0: HPS_OA(0); break; case 1: HPS_OA(1); break; case 2: HPS_OA(2); break; default: HPS_OA(3); break; }
#undef HPS_OA
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

extern "C" int hps_salame_jxjy_from_bxby (hps_slab slab, hps_geom g, int bx_comp, int by_comp, int chi_comp, int jx_comp, int jy_comp,
                                          hps_stream stream)
{
    HPS_REQUIRE(slab.p && slab.nx > 0 && slab.ny > 0, "hps_salame_jxjy_from_bxby: bad slab");
    for (int c : {bx_comp, by_comp, chi_comp, jx_comp, jy_comp}) HPS_REQUIRE(comp_ok(slab, c), "hps_salame_jxjy_from_bxby: bad component");
    hipLaunchKernelGGL(k_salame_jxjy_from_bxby, dim3(ceil_div(slab.nx, 256), slab.ny), dim3(256), 0, (hipStream_t)stream, SlabView(slab),
                       bx_comp, by_comp, chi_comp, jx_comp, jy_comp, 1.5*g.dz, 1.0/g.mu0);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

extern "C" int hps_salame_sxsy_from_jz (hps_slab slab, hps_geom g, int jz_comp, int sy_comp, int sx_comp, hps_stream stream)
{
    if (int e = check_stencil(slab, 1, "hps_salame_sxsy_from_jz")) return e;
    for (int c : {jz_comp, sy_comp, sx_comp}) HPS_REQUIRE(comp_ok(slab, c), "hps_salame_sxsy_from_jz: bad component");
    hipLaunchKernelGGL(k_salame_sxsy_from_jz, dim3(ceil_div(slab.nx, 256), slab.ny), dim3(256), 0, (hipStream_t)stream, SlabView(slab),
                       jz_comp, sy_comp, sx_comp, g.mu0, 0.5*(1.0/g.dx), 0.5*(1.0/g.dy));
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

extern "C" int hps_salame_get_w (hps_slab slab, int ez_target_comp, int ez_no_salame_comp, int ez_comp, int jz_comp, double* scratch_dev,
                                 double* out4_host, hps_stream stream)
{
    HPS_REQUIRE(slab.p && slab.nx > 0 && slab.ny > 0 && scratch_dev && out4_host, "hps_salame_get_w: null argument");
    for (int c : {ez_target_comp, ez_no_salame_comp, ez_comp, jz_comp}) HPS_REQUIRE(comp_ok(slab, c), "hps_salame_get_w: bad component");
    hipStream_t st = (hipStream_t)stream;
    if (int e = salame_get_w_enqueue(slab, ez_target_comp, ez_no_salame_comp, ez_comp, jz_comp, scratch_dev, st)) return e;
    HPS_HIP_CHECK(hipMemcpyAsync(out4_host, salame_get_w_result(scratch_dev), 4*sizeof(double), hipMemcpyDeviceToHost, st));
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    return HPS_OK;
}

extern "C" int hps_salame_scale_beam_slice (double* w_dev, long n, double W, hps_stream stream)
{
    HPS_REQUIRE(n >= 0 && (w_dev || n == 0), "hps_salame_scale_beam_slice: null argument");
    if (n == 0) return HPS_OK;
    hipLaunchKernelGGL(k_salame_scale_w, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, w_dev, n, W);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

extern "C" int hps_engine_salame_stats (void* h, double* out)
{
    HPS_REQUIRE(h && out, "hps_engine_salame_stats: null argument");
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->c_sal >= 0, "hps_engine_salame_stats: the deck has no beam_do_salame (nor was hps_engine_set_beam_species_salame called)");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    std::memcpy(out, E->sal_stats.data(), E->sal_stats.size()*sizeof(double));
    return HPS_OK;
}
extern "C" int hps_engine_set_beam_species_salame (void* h, int on)
{
    HPS_REQUIRE(h, "hps_engine_set_beam_species_salame: null engine");
    return static_cast<Engine*>(h)->set_beam_species_salame(on);
}
extern "C" int hps_engine_salame_scale_slice (void* h, int islice, double W)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_salame_scale_slice: null engine");
    HPS_REQUIRE(E->moving, "hps_engine_salame_scale_slice: needs a moving beam (hipace.dt != 0 or adaptive): the one beam of a static-beam engine takes hps_salame_scale_beam_slice");
    HPS_REQUIRE(E->steps_begun > 0 && !E->beam_import, "hps_engine_salame_scale_slice: call after hps_engine_begin_step, on an engine that holds its beam");
    HPS_REQUIRE(islice >= 0 && islice < E->d.nz, "hps_engine_salame_scale_slice: no such slice");
    HPS_REQUIRE(std::isfinite(W), "hps_engine_salame_scale_slice: W must be finite");
    return salame_scale_moving(*E, E->d.nz - 1 - islice, E->salame_mask(), W);
}
