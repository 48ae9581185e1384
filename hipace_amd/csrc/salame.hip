// salame.hip -- the operators of the SALAME module (salame/Salame.cpp of the reference): the only-advance push, the
// pointwise kernels on the SALAME planes, the deterministic reduction behind the weight factor W, and the scaling of a
// beam slice's weights.  The per-slice sequence that calls them is Engine::salame_module (engine.hip).
#include "common.h"
#include "engine.h"

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
