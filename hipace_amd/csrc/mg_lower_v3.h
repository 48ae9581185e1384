// mg_lower_v3.h -- k_lower_v3: the cell-centred lower V in registers and LDS, one field component per workgroup (Low2, Blk and
// the blk_* / low_*_s / tiny_*_s phases), its guest workgroups (lower_v_guest: the slab's shift / zero pass) and the guest it
// sends into k_smooth's initial pass (CoefGuest, coef_guest_derive: mg_smooth.h includes this file for them).  Needs
// mg_stencil.h, and slab_ops.h for the guests' pass.
#ifndef HPS_MG_LOWER_V3_H_
#define HPS_MG_LOWER_V3_H_

#include "mg_stencil.h"
#include "slab_ops.h"

namespace hps {

// ---------------------------------------------------------------------------------------------
// Cell-centred lower V (k_lower_v3), register/LDS resident, from the first level with at most 64 x 64 cells, ONE field
// component per workgroup (grid = 2).  The two components of the solve only meet in the norm, which the lower V does not
// take, so two workgroups on two CUs need no synchronisation at all, and every barrier phase of the 64 x 64 and 32 x 32
// levels carries half the LDS traffic and half the fp64 instruction stream of one workgroup for both (one CU's LDS pipe and
// VALUs were what bounded those phases: ~1800 cycles per half-sweep).
// Every level is worked in 2 x 2 cell blocks, one thread per block: the block's correction, rhs and inverse diagonal sit in
// registers, so a red-black half-sweep updates two cells with two LDS reads each (the other two neighbours are the thread's
// own cells), the residual's 4-average for the restriction and the piecewise-constant prolongation are thread-local, and
// the 2 x 2 bottom level is one lane's registers.  LDS per level: level A one ringed plane (cor); below it four: cor | res |
// acf | 1/diag (level A keeps its rhs in registers).  Levels of at most 64 blocks run in wave 0 alone without workgroup
// barriers.  The first sweep of every down-leg level starts from cor = 0, where the update is rhs/diag exactly.
// Level A's inverse diagonals come from k_acf_pyramid (cinv_g: 4 divisions per thread and V-cycle less).  The gate of
// the speculative V-cycle is evaluated AFTER the level-A loads have been issued: a kernel's first dependent read of
// global memory costs ~1.5 us behind a kernel boundary (scripts/ubench/launch_floor.hip), and the two now overlap.
constexpr int LOW2_MAXLEV = 8;
struct Low2 { int nl; int total; int nx[LOW2_MAXLEV], ny[LOW2_MAXLEV], off[LOW2_MAXLEV];
              int coff[LOW2_MAXLEV], cbase, ctot; };      // the levels' [acf | 1/diag] planes, one contiguous image from cbase

template <bool WAVE>
__device__ __forceinline__ void lvl_sync ()
{
    // one wave: its DS instructions reach the LDS in program order, so a read issued behind a write sees it without the
    // wave waiting for the write to retire -- only the compiler has to be kept in order (the s_waitcnt that stood here
    // stalled every one of the ~60 phases of the one-wave levels for the write's round trip)
    if (WAVE) asm volatile("" ::: "memory");
    else __syncthreads();
}

// a thread's 2 x 2 block: cells k = 0:(i,j) 1:(i+1,j) 2:(i,j+1) 3:(i+1,j+1); 0 and 3 have colour 0
struct Blk {
    lds_double* c0;           // the block's cell 0 in the correction plane
    int pitch;
    bool act;                 // this thread has a block on this level
    bool ok[4];               // cell inside the level (odd sizes)
    double fxm[2], fym[2];    // wall multipliers of the block's two columns / rows
    double v0[4];             // correction
    double r0[4], ci[4];
};

// half-sweep of parity P (0: cells 0 and 3, 1: cells 1 and 2) + publication of the new values
template <int P, bool WAVE>
__device__ __forceinline__ void blk_sweep (Blk& B)
{
    if (B.act) {
        const int pt = B.pitch;
        if (P == 0) {
            {   const double w0 = B.c0[-1], s0 = B.c0[-pt];
                const double n0 = (B.r0[0] - (B.fxm[0]*(w0 + B.v0[1]) + B.fym[0]*(s0 + B.v0[2])))*B.ci[0];
                if (B.ok[0]) { B.v0[0] = n0; B.c0[0] = n0; } }
            {   const double e0 = B.c0[pt + 2], t0 = B.c0[2*pt + 1];
                const double n0 = (B.r0[3] - (B.fxm[1]*(B.v0[2] + e0) + B.fym[1]*(B.v0[1] + t0)))*B.ci[3];
                if (B.ok[3]) { B.v0[3] = n0; B.c0[pt + 1] = n0; } }
        } else {
            {   const double e0 = B.c0[2], s0 = B.c0[1 - pt];
                const double n0 = (B.r0[1] - (B.fxm[1]*(B.v0[0] + e0) + B.fym[0]*(s0 + B.v0[3])))*B.ci[1];
                if (B.ok[1]) { B.v0[1] = n0; B.c0[1] = n0; } }
            {   const double w0 = B.c0[pt - 1], t0 = B.c0[2*pt];
                const double n0 = (B.r0[2] - (B.fxm[0]*(w0 + B.v0[3]) + B.fym[1]*(B.v0[0] + t0)))*B.ci[2];
                if (B.ok[2]) { B.v0[2] = n0; B.c0[pt] = n0; } }
        }
    }
    lvl_sync<WAVE>();
}

// down-leg sweeps from cor = 0: sweep 0 is rhs/diag on the colour-0 cells, then sweeps 1 .. nsw-1 (nsw even)
template <bool WAVE>
__device__ __forceinline__ void blk_down_sweeps (Blk& B, int nsw)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) B.v0[k] = 0.0;
    if (B.act) {
        if (B.ok[0]) { B.v0[0] = B.r0[0]*B.ci[0]; B.c0[0] = B.v0[0]; }
        if (B.ok[3]) { B.v0[3] = B.r0[3]*B.ci[3]; B.c0[B.pitch + 1] = B.v0[3]; }
    }
    lvl_sync<WAVE>();
    blk_sweep<1, WAVE>(B);
    for (int s = 2; s < nsw; s += 2) { blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B); }
}

// The whole level is this one block (2 x 2 cells or fewer): every neighbour outside the block is the
// zero ring, so all nsw sweeps from cor = 0 run in the lane's registers; published once at the end.
__device__ __forceinline__ void blk_single_sweeps (Blk& B, int nsw)
{
    // (every neighbour outside the block is the zero ring: 0 + v == v exactly, so the sums with it are left out -- this is a
    //  chain of 2 nsw dependent half-sweeps in one lane, every instruction of it is on the V-cycle's critical path)
#pragma unroll
    for (int k = 0; k < 4; ++k) B.v0[k] = 0.0;
    if (B.act) {
        for (int s = 0; s < nsw; s += 2) {
            {   const double a0 = (B.r0[0] - (B.fxm[0]*B.v0[1] + B.fym[0]*B.v0[2]))*B.ci[0];
                const double b0 = (B.r0[3] - (B.fxm[1]*B.v0[2] + B.fym[1]*B.v0[1]))*B.ci[3];
                if (B.ok[0]) B.v0[0] = a0;
                if (B.ok[3]) B.v0[3] = b0; }
            {   const double a0 = (B.r0[1] - (B.fxm[1]*B.v0[0] + B.fym[0]*B.v0[3]))*B.ci[1];
                const double b0 = (B.r0[2] - (B.fxm[0]*B.v0[3] + B.fym[1]*B.v0[0]))*B.ci[2];
                if (B.ok[1]) B.v0[1] = a0;
                if (B.ok[2]) B.v0[2] = b0; }
        }
        const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) if (B.ok[k]) B.c0[ok[k]] = B.v0[k];
    }
}

// residuals of the block's four cells (0 for cells outside the level)
__device__ __forceinline__ void blk_residual (const Blk& B, int i, int j, const LevBox& b, const double (&a)[4],
                                              double fx, double fy, double (&q0)[4])
{
    const int pt = B.pitch;
    const double w00 = B.c0[-1], s00 = B.c0[-pt], e01 = B.c0[2], s01 = B.c0[1 - pt];
    const double w02 = B.c0[pt - 1], n02 = B.c0[2*pt], e03 = B.c0[pt + 2], n03 = B.c0[2*pt + 1];
    q0[0] = residual_v<false>(B.v0[0], w00, B.v0[1], s00, B.v0[2], i, j, b, B.r0[0], a[0], fx, fy);
    q0[1] = residual_v<false>(B.v0[1], B.v0[0], e01, s01, B.v0[3], i + 1, j, b, B.r0[1], a[1], fx, fy);
    q0[2] = residual_v<false>(B.v0[2], w02, B.v0[3], B.v0[0], n02, i, j + 1, b, B.r0[2], a[2], fx, fy);
    q0[3] = residual_v<false>(B.v0[3], B.v0[2], e03, B.v0[1], n03, i + 1, j + 1, b, B.r0[3], a[3], fx, fy);
#pragma unroll
    for (int k = 0; k < 4; ++k) if (!B.ok[k]) q0[k] = 0.0;
}

// geometry of thread t's block on a level of nx x ny cells whose plane starts at `lev` (pitch nx + 2)
__device__ __forceinline__ void blk_geometry (Blk& B, lds_double* lev, int nx, int ny, int t, double fx, double fy, int& i, int& j)
{
    const int nbx = (nx + 1) >> 1, nby = (ny + 1) >> 1;
    const int lg = (nbx <= 1) ? 0 : 32 - __clz(nbx - 1);       // blocks per row rounded up to a power of two
    const int bi = t & ((1 << lg) - 1), bj = t >> lg;
    B.act = (bi < nbx) && (bj < nby);
    i = 2*bi; j = 2*bj;
    B.pitch = nx + 2;
    const int o = B.act ? (j + 1)*B.pitch + i + 1 : B.pitch + 1;
    B.c0 = lev + o;
    B.ok[0] = B.act; B.ok[1] = B.act && (i + 1 < nx); B.ok[2] = B.act && (j + 1 < ny); B.ok[3] = B.ok[1] && B.ok[2];
    B.fxm[0] = wall_mult<true>(i, 0, nx - 1, fx); B.fxm[1] = wall_mult<true>(i + 1, 0, nx - 1, fx);
    B.fym[0] = wall_mult<true>(j, 0, ny - 1, fy); B.fym[1] = wall_mult<true>(j + 1, 0, ny - 1, fy);
}

template <bool WAVE>
__device__ __forceinline__ void low_down_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy, int nsw, bool last)
{
    const int nx = d.nx[l], ny = d.ny[l];
    Blk B; int i, j;
    blk_geometry(B, base + d.off[l], nx, ny, t, fx, fy, i, j);
    const int ps = B.pitch*(ny + 2);
    const lds_double* r = B.c0 + ps;
    const lds_double* cf = base + d.coff[l] + (B.c0 - (base + d.off[l]));      // the block's cell 0 in the acf plane
    const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
    double a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = B.ok[k] ? ok[k] : 0;
        B.r0[k] = r[o]; a[k] = cf[o]; B.ci[k] = cf[ps + o];
    }
    if (last && nx <= 2 && ny <= 2) { blk_single_sweeps(B, nsw); lvl_sync<WAVE>(); }
    else blk_down_sweeps<WAVE>(B, nsw);
    if (!last) {
        double q0[4];
        blk_residual(B, i, j, cc_box(nx, ny), a, fx, fy, q0);
        if (B.act) {
            const int pn = d.nx[l+1] + 2, psn = pn*(d.ny[l+1] + 2);
            base[d.off[l+1] + psn + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(q0[0] + q0[1] + q0[2] + q0[3]);
        }
        lvl_sync<WAVE>();
    }
}

template <bool WAVE>
__device__ __forceinline__ void low_up_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l];
    Blk B; int i, j;
    blk_geometry(B, base + d.off[l], nx, ny, t, fx, fy, i, j);
    const int ps = B.pitch*(ny + 2);
    const lds_double* r = B.c0 + ps;
    const lds_double* cf = base + d.coff[l] + (B.c0 - (base + d.off[l]));
    const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
    const int pn = d.nx[l+1] + 2;
    const lds_double* kc = base + d.off[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1;
    const double k0 = B.act ? kc[0] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = B.ok[k] ? ok[k] : 0;
        B.r0[k] = r[o]; B.ci[k] = cf[ps + o];
        const double c0 = B.c0[o];
        B.v0[k] = B.ok[k] ? c0 + k0 : 0.0;
        if (B.ok[k]) B.c0[o] = B.v0[k];
    }
    lvl_sync<WAVE>();
    blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B); blk_sweep<0, WAVE>(B); blk_sweep<1, WAVE>(B);
}

// levels of at most 8 x 8 cells in one wave, one lane per cell
__device__ __forceinline__ void tiny_down_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l], pitch = nx + 2, ps = pitch*(ny + 2);
    const int i = t & 7, j = t >> 3;
    const bool ok = (i < nx) && (j < ny);
    const int o = ok ? (j + 1)*pitch + i + 1 : pitch + 1;
    lds_double* c0 = base + d.off[l] + o;
    const lds_double* cf = base + d.coff[l] + o;
    const double r0 = c0[ps], a = cf[0], ci = cf[ps];
    const double fxm = wall_mult<true>(i, 0, nx - 1, fx), fym = wall_mult<true>(j, 0, ny - 1, fy);
    if (ok && (((i + j) & 1) == 0)) c0[0] = r0*ci;                          // sweep 0 from cor = 0
    lvl_sync<true>();
    for (int s = 1; s < 4; ++s) {
        if (ok && (((i + j + s) & 1) == 0)) c0[0] = (r0 - offdiag_m((const lds_double*)c0, pitch, fxm, fym))*ci;
        lvl_sync<true>();
    }
    const LevBox b = cc_box(nx, ny);
    const double u0 = residual_at<false>((const lds_double*)c0, pitch, i, j, b, r0, a, fx, fy);
    const double q0 = ok ? u0 : 0.0;
    const double b0 = __shfl_down(q0, 1), g0 = __shfl_down(q0, 8), e0 = __shfl_down(q0, 9);
    if (ok && !(i & 1) && !(j & 1)) {
        const int pn = d.nx[l+1] + 2, psn = pn*(d.ny[l+1] + 2);
        base[d.off[l+1] + psn + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(q0 + b0 + g0 + e0);
    }
    lvl_sync<true>();
}

__device__ __forceinline__ void tiny_up_s (lds_double* base, const Low2& d, int l, int t, double fx, double fy)
{
    const int nx = d.nx[l], ny = d.ny[l], pitch = nx + 2, ps = pitch*(ny + 2);
    const int i = t & 7, j = t >> 3;
    const bool ok = (i < nx) && (j < ny);
    const int o = ok ? (j + 1)*pitch + i + 1 : pitch + 1;
    lds_double* c0 = base + d.off[l] + o;
    const double r0 = c0[ps], ci = base[d.coff[l] + ps + o];
    const double fxm = wall_mult<true>(i, 0, nx - 1, fx), fym = wall_mult<true>(j, 0, ny - 1, fy);
    if (ok) {
        const int pn = d.nx[l+1] + 2;
        c0[0] = c0[0] + base[d.off[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1];
    }
    lvl_sync<true>();
    for (int s = 0; s < 4; ++s) {
        if (ok && (((i + j + s) & 1) == 0)) c0[0] = (r0 - offdiag_m((const lds_double*)c0, pitch, fxm, fym))*ci;
        lvl_sync<true>();
    }
}

// Guests of the lower V (the engine's HPS_EARLY_INIT): workgroups 2 .. of the first V-cycle's launch run the slab's shift /
// zero pass for the next slice on the compute units the two solver workgroups leave idle.  They share nothing with the
// solver workgroups and do not read the stop rule.
__device__ __forceinline__ void lower_v_guest (const ShiftInit& a, int guest, int nguests)
{
    for (long s = (long)guest*1024 + threadIdx.x; s < a.plane; s += (long)nguests*1024) shift_init_cell(a, s);
}

// Guest of a solve's initial level-0 pass (k_smooth's GUEST): the [acf | 1/diag] image of the levels below k_lower_v3's top
// level A, which depends on level A's coefficient plane only (the pyramid's, a whole launch earlier in the stream) -- derived
// here, beside the pass's tiles, the first lower V of the solve does not derive it on the V-cycle's critical path.  Cell for
// cell the expressions of k_lower_v3's own derivation (which grids without this guest keep), block by block as there; the
// image is staged in the host kernel's static LDS (s_img, nt threads) and left in g.img, where every lower V copies it in.
struct CoefGuest { const Low2* low; const double* acfA; double* img; double facx0, facy0; };

__device__ void coef_guest_derive (double* s_img, const CoefGuest& g, int nt)
{
    lds_double* img = (lds_double*)s_img;
    const Low2& d = *g.low;
    const int t = threadIdx.x;
    const int nl = d.nl, ctot = d.ctot, cbase = d.cbase;
    for (int q = t; q < ctot; q += nt) img[q] = 0.0;       // (the rings: never read, but the image is the same every time)
    __syncthreads();
    if (nl > 1) {
        const int nxA = d.nx[0], nyA = d.ny[0], nbx = (nxA + 1) >> 1, nby = (nyA + 1) >> 1, p1 = d.nx[1] + 2;
        for (int q = t; q < nbx*nby; q += nt) {
            const int bj = q / nbx, i = 2*(q - bj*nbx), j = 2*bj;
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ik = i + (k & 1), jk = j + (k >> 1);
                const double v = g.acfA[min(ik, nxA - 1) + min(jk, nyA - 1)*nxA];
                a[k] = (ik < nxA && jk < nyA) ? v : 0.0;
            }
            img[d.coff[1] - cbase + ((j >> 1) + 1)*p1 + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
        }
    }
    __syncthreads();
    for (int l = 1; l < nl; ++l) {
        const double fx = lvl_fac(g.facx0, l), fy = lvl_fac(g.facy0, l);
        const int nx = d.nx[l], ny = d.ny[l], nbx = (nx + 1) >> 1, nby = (ny + 1) >> 1, pitch = nx + 2, ps = pitch*(ny + 2);
        lds_double* lev = img + (d.coff[l] - cbase);
        const int ok[4] = {0, 1, pitch, pitch + 1};
        for (int q = t; q < nbx*nby; q += nt) {
            const int bj = q / nbx, i = 2*(q - bj*nbx), j = 2*bj;
            lds_double* acf = lev + (j + 1)*pitch + i + 1;
            const bool in[4] = {true, i + 1 < nx, j + 1 < ny, i + 1 < nx && j + 1 < ny};
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = in[k] ? acf[ok[k]] : 0.0;
            if (l + 1 < nl) {
                const int pn = d.nx[l+1] + 2;
                img[d.coff[l+1] - cbase + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) acf[ps + ok[k]] = 1.0/diag_c0<true>(i + (k & 1), j + (k >> 1), cc_box(nx, ny), a[k], fx, fy);
        }
        __syncthreads();
    }
    for (int q = t; q < ctot; q += nt) g.img[q] = img[q];
}

__global__ __launch_bounds__(1024)
void k_lower_v3 (const Low2* __restrict__ dp, const double* __restrict__ acf_g, const double* __restrict__ cinv_g,
                 const double* __restrict__ res_g, double* __restrict__ cor_g, double* __restrict__ coef_g, int nxA, int nyA, int ctot,
                 double facx0, double facy0, int nsweeps_bottom, StopRule sr, ShiftInit guest, int derive_first)
{
    if (blockIdx.x >= 2) { lower_v_guest(guest, (int)blockIdx.x - 2, (int)gridDim.x - 2); return; }
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    lds_double* base = (lds_double*)lds_raw;
    const int t = threadIdx.x;
    const Low2& d = *dp;          // (level A's size and the image's length come by value: the first loads must not wait for this read)
    const int nl = d.nl;
    const int cellsA = nxA*nyA;
    res_g += (long)blockIdx.x*cellsA; cor_g += (long)blockIdx.x*cellsA;      // this workgroup's component
    const LevBox bA = cc_box(nxA, nyA);
    Blk A; int iA, jA;
    blk_geometry(A, base, nxA, nyA, t, facx0, facy0, iA, jA);       // (d.off[0] = 0)
    // ---- level A: rhs, coefficient and inverse diagonal of the thread's block from HBM, issued before the gate is read
    double aA[4], rA[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = iA + (k & 1), j = jA + (k >> 1);
        const int g = min(i, nxA - 1) + min(j, nyA - 1)*nxA;
        const double v0 = res_g[g], v2 = acf_g[g], v3 = cinv_g[g];
        rA[k] = A.ok[k] ? v0 : 0.0; aA[k] = A.ok[k] ? v2 : 0.0; A.ci[k] = A.ok[k] ? v3 : 0.0;
        A.r0[k] = rA[k];
    }
    // The [acf | 1/diag] planes of the levels below A depend on the coefficient only: the guest of the solve's initial level-0
    // pass has left their image in coef_g (coef_guest_derive) and every V-cycle copies it in.  derive_first (grids whose
    // initial pass cannot host the guest, HPS_MG_COEF_GUEST=0): the first V-cycle of a solve derives them here
    // (average_down_acoef + one division per cell) and leaves the image in coef_g for the later ones.
    const bool derive = derive_first && (sr.k <= 0);
    constexpr int NIMG = 4;      // image words per thread (LOW2 levels below 64 x 64: 3264 doubles)
    double img[NIMG];
#pragma unroll
    for (int m = 0; m < NIMG; ++m) { const int q = min(t + 1024*m, ctot - 1); img[m] = derive ? 0.0 : coef_g[q]; }
    const bool active = vcycle_active(sr);
#pragma unroll
    for (int k = 0; k < 4; ++k) { HPS_KEEP(rA[k]); HPS_KEEP(aA[k]); HPS_KEEP(A.ci[k]); }
#pragma unroll
    for (int m = 0; m < NIMG; ++m) HPS_KEEP(img[m]);
    if (!active) return;
    MG_STAMP(8);
    // only the correction planes need zeros (ring + the cells of the colour the first half-sweep skips)
    for (int l = 0; l < nl; ++l) {
        const int n1 = (d.nx[l] + 2)*(d.ny[l] + 2);
        lds_double* c = base + d.off[l];
        for (int s = t; s < n1; s += 1024) c[s] = 0.0;
    }
    if (!derive) {
#pragma unroll
        for (int m = 0; m < NIMG; ++m) if (t + 1024*m < ctot) base[d.cbase + t + 1024*m] = img[m];
        for (int q = t + 1024*NIMG; q < ctot; q += 1024) base[d.cbase + q] = coef_g[q];      // (larger level sets)
    }
    __syncthreads();
    if (derive) {
        // ---- coefficient hierarchy (average_down_acoef) and inverse diagonals of the levels below
        if (nl > 1 && A.act) {
            const int p1 = d.nx[1] + 2;
            base[d.coff[1] + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1] = 0.25*(aA[0] + aA[1] + aA[2] + aA[3]);
        }
        __syncthreads();
        for (int l = 1; l < nl; ++l) {
            const double fx = lvl_fac(facx0, l), fy = lvl_fac(facy0, l);
            const int nx = d.nx[l], ny = d.ny[l];
            Blk B; int i, j;
            blk_geometry(B, base + d.coff[l], nx, ny, t, fx, fy, i, j);     // c0 = the block's cell 0 in the acf plane
            const int ps = B.pitch*(ny + 2);
            lds_double* acf = B.c0;
            const int ok[4] = {0, 1, B.pitch, B.pitch + 1};
            if (B.act) {          // (whole waves have no block on the small levels: they skip the divisions)
                double a[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = B.ok[k] ? acf[ok[k]] : 0.0;
                if (l + 1 < nl) {     // the next level's coefficient first: the divisions below are off the critical path
                    const int pn = d.nx[l+1] + 2;
                    base[d.coff[l+1] + ((j >> 1) + 1)*pn + (i >> 1) + 1] = 0.25*(a[0] + a[1] + a[2] + a[3]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (B.ok[k]) acf[ps + ok[k]] = 1.0/diag_c0<true>(i + (k & 1), j + (k >> 1), cc_box(nx, ny), a[k], fx, fy);
            }
            __syncthreads();
        }
        if (blockIdx.x == 0) for (int q = t; q < ctot; q += 1024) coef_g[q] = base[d.cbase + q];
    }
    MG_STAMP(9);
    // ---- level A down-leg
    const bool bottomA = (nl == 1);
    blk_down_sweeps<false>(A, bottomA ? nsweeps_bottom : 4);
    if (!bottomA) {
        double q0[4];
        blk_residual(A, iA, jA, bA, aA, facx0, facy0, q0);
        if (A.act) {
            const int p1 = d.nx[1] + 2, ps1 = p1*(d.ny[1] + 2);
            base[d.off[1] + ps1 + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1] = 0.25*(q0[0] + q0[1] + q0[2] + q0[3]);
        }
        __syncthreads();
    }
    MG_STAMP(10);
    if (!bottomA) {
        // lw = first level whose blocks (and those of every level below it) fit wave 0
        int lw = 1;
        for (; lw < nl; ++lw) {
            const int nbx = (d.nx[lw] + 1) >> 1, nby = (d.ny[lw] + 1) >> 1;
            int lg = 0; while ((1 << lg) < nbx) ++lg;
            if ((nby << lg) <= 64) break;
        }
        for (int l = 1; l < lw; ++l)
            low_down_s<false>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l), (l == nl - 1) ? nsweeps_bottom : 4, l == nl - 1);
        MG_STAMP(11);
        if (lw < nl) {
            if (t < 64) {
                for (int l = lw; l < nl; ++l) {
                    MG_STAMP(16 + l);
                    const bool tiny = (d.nx[l] <= 8 && d.ny[l] <= 8 && l < nl - 1);
                    if (tiny) tiny_down_s(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                    else low_down_s<true>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l), (l == nl - 1) ? nsweeps_bottom : 4, l == nl - 1);
                }
                for (int l = nl - 2; l >= lw; --l) {
                    MG_STAMP(32 + l);
                    if (d.nx[l] <= 8 && d.ny[l] <= 8) tiny_up_s(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                    else low_up_s<true>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
                }
            }
            __syncthreads();
        }
        MG_STAMP(12);
        for (int l = min(lw - 1, nl - 2); l >= 1; --l)
            low_up_s<false>(base, d, l, t, lvl_fac(facx0, l), lvl_fac(facy0, l));
        // ---- level A up-leg: correction back from LDS, prolongation, 4 sweeps
        const int p1 = d.nx[1] + 2;
        const lds_double* kc = base + d.off[1] + ((jA >> 1) + 1)*p1 + (iA >> 1) + 1;
        const double k0 = A.act ? kc[0] : 0.0;
        const int ok[4] = {0, 1, A.pitch, A.pitch + 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = A.ok[k] ? ok[k] : 0;
            const double c0 = A.c0[o];
            A.v0[k] = A.ok[k] ? c0 + k0 : 0.0;
            if (A.ok[k]) A.c0[o] = A.v0[k];
            A.r0[k] = rA[k];
        }
        __syncthreads();
        blk_sweep<0, false>(A); blk_sweep<1, false>(A); blk_sweep<0, false>(A); blk_sweep<1, false>(A);
    }
    MG_STAMP(13);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = min(iA + (k & 1), nxA - 1) + min(jA + (k >> 1), nyA - 1)*nxA;
        if (A.ok[k]) cor_g[g] = A.v0[k];
    }
    MG_STAMP(14);
}

} // namespace hps
#endif
