// slab_ops.h -- slab passes that more than one translation unit launches.
#ifndef HPS_SLAB_OPS_H_
#define HPS_SLAB_OPS_H_

#include "common.h"

namespace hps {

struct CellBox { int ilo, ihi, jlo, jhi; };     // padded-array cell range, inclusive

// -grad Psi (Fields.cpp:938-955) and the beam part of Sx, Sy (Hipace::InitializeSxSyWithBeam, Hipace.cpp:744-790) of one
// cell; (i, j) over the whole padded plane: i in [-ng, nx + ng), j likewise
struct GradPsiSxSy { int cPsi, cExmBy, cEypBx; double hdx_inv, hdy_inv; int cSx, cSy, cJzb, cNx, cNy, cPx, cPy;
                     double mu0, dx2, dy2, dz2; CellBox bb; };

__device__ __forceinline__ void gradpsi_sxsy_cell (const SlabView& f, const GradPsiSxSy& a, int i, int j)
{
    if (i >= f.nx + f.ng) return;
    const long o = f.off(i, j);
    const int gg = f.ng - 1;
    if (i >= -gg && i < f.nx + gg && j >= -gg && j < f.ny + gg) {
        const double* P = f.p + a.cPsi*f.ns + o;
        f.p[a.cExmBy*f.ns + o] = -(P[1] - P[-1])*a.hdx_inv;
        f.p[a.cEypBx*f.ns + o] = -(P[f.js] - P[-f.js])*a.hdy_inv;
    }
    // no beam current within reach (bb is in padded-array cells): the sources are 0 without a load
    const int ia = i + f.ng, ja = j + f.ng;
    if (i < 0 || i >= f.nx || j < 0 || j >= f.ny || ia < a.bb.ilo || ia > a.bb.ihi || ja < a.bb.jlo || ja > a.bb.jhi) {
        f.p[a.cSy*f.ns + o] = 0.0; f.p[a.cSx*f.ns + o] = 0.0; return;
    }
    const double* J = f.p + a.cJzb*f.ns + o;
    const double dx_jzb = (J[1] - J[-1])/a.dx2;
    const double dy_jzb = (J[f.js] - J[-f.js])/a.dy2;
    const double dz_jxb = (f.p[a.cPx*f.ns + o] - f.p[a.cNx*f.ns + o])/a.dz2;
    const double dz_jyb = (f.p[a.cPy*f.ns + o] - f.p[a.cNy*f.ns + o])/a.dz2;
    f.p[a.cSy*f.ns + o] =  a.mu0*(-dy_jzb + dz_jyb);
    f.p[a.cSx*f.ns + o] = -a.mu0*(-dx_jzb + dz_jxb);
}

// ShiftSlices (fields/Fields.cpp:588-604) of a slice AND InitializeSlices (:535-586) of the next one, cell s of the padded
// plane: jx, jy <- Next beam currents, Previous <- This <- Next inside the beam's box; chi = 0, rhomjz [rho] = the ion
// background (AddRhoIons ahead of the deposition), and inside the box jz_beam = Next = 0.  The planes that are re-initialised
// come in two sets: the slice's values are read from `live`, the next slice's zeros and backgrounds go to `next` (the same
// set: in place, the Next currents are read before they are cleared).  Planes hold fewer than 2^31 cells (mg_create).
struct InitSet { int chi, rhomjz, rho, jzb, njxb, njyb; };      // rho = -1: the deck deposits none
struct ShiftInit { double* p; long ns, plane; int js; CellBox bb; InitSet live, next; int c_ion; };

__device__ __forceinline__ void shift_init_cell (const ShiftInit& a, long s)
{
    double* p = a.p; const long ns = a.ns;
    const int j = (int)((unsigned)s / (unsigned)a.js), i = (int)s - j*a.js;
    double njx = 0.0, njy = 0.0;
    if (i >= a.bb.ilo && i <= a.bb.ihi && j >= a.bb.jlo && j <= a.bb.jhi) {
        const double tjx = p[HPS_C_JXB*ns + s], tjy = p[HPS_C_JYB*ns + s];
        njx = p[a.live.njxb*ns + s]; njy = p[a.live.njyb*ns + s];
        p[HPS_C_P_JXB*ns + s] = tjx; p[HPS_C_P_JYB*ns + s] = tjy;
        p[HPS_C_JXB*ns + s] = njx;   p[HPS_C_JYB*ns + s] = njy;
        p[a.next.njxb*ns + s] = 0.0; p[a.next.njyb*ns + s] = 0.0; p[a.next.jzb*ns + s] = 0.0;
    }
    p[HPS_C_JX*ns + s] = njx; p[HPS_C_JY*ns + s] = njy;
    const double ion = a.c_ion >= 0 ? p[a.c_ion*ns + s] : 0.0;
    p[a.next.chi*ns + s] = 0.0; p[a.next.rhomjz*ns + s] = ion;
    if (a.next.rho >= 0) p[a.next.rho*ns + s] = ion;
}

// ---- slab kernels of engine.hip that the predictor-corrector (predcorr.hip) and SALAME (salame.hip) schedules launch too.
// Each is defined once, in engine.hip; a caller in another file calls the kernel's host stub there.
struct CompList { int n; int c[12]; };

// k_zero_comps / k_copy_comps over the whole padded planes of `slab` on `st`
void zero_comps (const hps_slab& slab, hipStream_t st, CompList full, CompList boxed, CellBox bb, CompList from_ion = CompList{0, {}}, int c_ion = -1);
void copy_comps (const hps_slab& slab, hipStream_t st, CompList dst, CompList src);

__global__ __launch_bounds__(256)
void k_rhs_all (SlabView f, int c_rhomjz, int c_ion, int c_rho, int c_jx, int c_jy, double inv_ep0,
                double fez_x, double fez_y, double fbz_y, double fbz_x, double* staging, long plane);
__global__ __launch_bounds__(256)
void k_grad_psi (SlabView f, int cPsi, int cExmBy, int cEypBx, double hdx_inv, double hdy_inv);
__global__ __launch_bounds__(256)
void k_sxsy_beam (SlabView f, int cSx, int cSy, int cJzb, int cNx, int cNy, int cPx, int cPy,
                  double mu0, double dx2, double dy2, double dz2, CellBox bb, int cBackX = -1, int cBackY = -1);

} // namespace hps
#endif
