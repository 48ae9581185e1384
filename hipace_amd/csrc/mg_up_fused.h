// mg_up_fused.h -- the up-leg of the cell-centred mid levels 1 .. 2 or 3 in one launch: UpLev (one level's share of a thread),
// up_fused_tile and the kernel k_up_fused.  Needs mg_stencil.h only; the arithmetic per cell is smooth_tile's (mg_smooth.h).
#ifndef HPS_MG_UP_FUSED_H_
#define HPS_MG_UP_FUSED_H_

#include "mg_stencil.h"

namespace hps {

// ---- the up-leg of the mid levels 1 .. NL in one launch (cell-centred) ---------------------------
// Per V-cycle the up-leg of levels 3, 2, 1 was three dependent launches of ~5, 5 and 8 us, each a launch floor + a first read
// + four barrier phases + a store.  The cell-centred prolongation is piecewise constant and an up-leg smoother needs neither
// residual nor norm, so the smoothed correction a level-1 tile reads from level 2 is a function of a small region of level 2,
// and that of a smaller one of level 3: a workgroup that owns a level-1 tile first smooths the level-3 cells under it in LDS,
// then the level-2 cells, then its own tile.  The redundant sweeps fall on the cheap levels; rescor[2], rescor[3] (read by the
// next up-leg level only) stay in LDS.  All three levels' inputs exist when the launch starts: every load is issued up front.
//
// Geometry.  A level with SX x SY swept cells (ringed: + 2) reads the coarser level under its ringed region clipped to its
// box: at most (SX + 2)/2 + 1 coarse cells in x for any parity of the origin.  Those must be final, i.e. 3 cells inside the
// coarse swept region or behind the box's edge: the coarse level sweeps (SX + 2)/2 + 7 cells from 3 below the first one.
// 64 x 32 on level 1 -> 40 x 24 on level 2 -> 28 x 20 on level 3; 32 x 16 -> 24 x 16 -> 20 x 16.
//
// UpLev: one level's share of a thread -- GP cell pairs in GP consecutive rows (the block rows of smooth_tile: the values
// it wrote last stay in registers), right-hand side, multipliers and inverse diagonal in registers, and its share of the
// ringed region's start values.  The arithmetic per cell is smooth_tile's (gs_cell, wall_mult, diag_c0, the same masks).
struct UpLevArg { LevBox b; FView rhs, acf, cor; double facx, facy; };
struct UpArgs { UpLevArg l[3]; FView crse, out; int ntx; };      // l[k]: level 1 + k; crse: below the coarsest fused level; out: rescor[1]

template <int SX_, int SY_, int NT_, bool INTERIOR, bool GCRSE>
struct UpLev {
    static constexpr int SX = SX_, SY = SY_, NT = NT_, AX = SX + 2, AY = SY + 2, AXH = AX/2, CH = AY*AXH, PR = SX/2;
    static constexpr int GP = (PR*SY + NT - 1)/NT;         // cell pairs per thread
    static constexpr int NF = (AX*AY + NT - 1)/NT;         // ringed cells per thread
    static constexpr int NBLK = SY/GP;                     // row blocks of PR threads each
    static_assert(SX % 2 == 0 && SY % GP == 0 && PR*NBLK <= NT, "level shape");
    int gi0, gj0, cpar, pk, blk;
    double r0[GP][2], r1[GP][2], ac[GP][2], ci[GP][2], fxm[GP][2], fym[GP];
    bool in[GP][2];
    int hx[GP];
    double v0[NF], v1[NF], c0[GCRSE ? NF : 1], c1[GCRSE ? NF : 1];
    double l0[GP][2], l1[GP][2];

    // every read of global memory this level makes: clamped addresses, nothing depends on a loaded value
    __device__ __forceinline__ void issue (const UpLevArg& a, const FView& crse, int gi0_, int gj0_)
    {
        const LevBox& b = a.b;
        const int tid = threadIdx.x;
        gi0 = gi0_; gj0 = gj0_; cpar = (gi0 + gj0) & 1;
        const bool live = tid < PR*NBLK;                   // (the coarse levels have fewer pairs than the workgroup has threads)
        blk = live ? tid / PR : 0; pk = tid % PR;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int j = gj0 + blk*GP + m;
            hx[m] = (gi0 + 2*pk + j) & 1;                  // colour 0 cell: (i + j) even
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int i = gi0 + 2*pk + (hx[m] ^ p);
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                in[m][p] = live && (INTERIOR || (ic == i && jc == j));
                r0[m][p] = a.rhs(ic, jc, 0); r1[m][p] = a.rhs(ic, jc, 1); ac[m][p] = a.acf(ic, jc, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = min(tid + NT*m, AX*AY - 1);
            const int lj = s / AX, li = s - lj*AX;
            const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
            const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
            v0[m] = a.cor(ic, jc, 0); v1[m] = a.cor(ic, jc, 1);
            if constexpr (GCRSE) { c0[m] = crse(ic >> 1, jc >> 1, 0); c1[m] = crse(ic >> 1, jc >> 1, 1); }
        }
    }
    __device__ __forceinline__ void keep () const
    {
#pragma unroll
        for (int m = 0; m < GP; ++m) { HPS_KEEP(r0[m][0]); HPS_KEEP(r0[m][1]); HPS_KEEP(r1[m][0]); HPS_KEEP(r1[m][1]); HPS_KEEP(ac[m][0]); HPS_KEEP(ac[m][1]); }
#pragma unroll
        for (int m = 0; m < NF; ++m) { HPS_KEEP(v0[m]); HPS_KEEP(v1[m]); if constexpr (GCRSE) { HPS_KEEP(c0[m]); HPS_KEEP(c1[m]); } }
    }
    // masks, multipliers, inverse diagonals (smooth_tile's expressions)
    __device__ __forceinline__ void coefficients (const UpLevArg& a)
    {
        const LevBox& b = a.b;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int j = gj0 + blk*GP + m;
            fym[m] = INTERIOR ? a.facy : wall_mult<true>(j, b.loy, b.hiy, a.facy);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int i = gi0 + 2*pk + (hx[m] ^ p);
                fxm[m][p] = INTERIOR ? a.facx : wall_mult<true>(i, b.lox, b.hix, a.facx);
                const bool ok = in[m][p];
                r0[m][p] = ok ? r0[m][p] : 0.0;
                r1[m][p] = ok ? r1[m][p] : 0.0;
                ac[m][p] = ok ? ac[m][p] : 0.0;
                ci[m][p] = 1.0/diag_c0<true>(i, j, b, ac[m][p], a.facx, a.facy);
            }
        }
    }
    // start = cor + P(coarser result) inside the unknowns' box, 0 elsewhere, ring included; the two colours in separate
    // planes as in smooth_tile.  CL: the coarser level, whose result is in sc (its two component planes); none for GCRSE.
    template <class CL>
    __device__ __forceinline__ void fill (double* s, const UpLevArg& a, const CL* cl, const double* sc)
    {
        const LevBox& b = a.b;
        const int tid = threadIdx.x;
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int q = tid + NT*m;
            if (q < AX*AY) {
                const int lj = q / AX, li = q - lj*AX;
                const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                double a0 = v0[m], a1 = v1[m];
                if constexpr (GCRSE) { a0 += c0[m]; a1 += c1[m]; }
                else {
                    const int cli = (ic >> 1) - (cl->gi0 - 1), clj = (jc >> 1) - (cl->gj0 - 1);
                    const int oc = ((cl->cpar + cli + clj) & 1)*CL::CH + clj*CL::AXH + (cli >> 1);
                    a0 += sc[oc]; a1 += sc[2*CL::CH + oc];
                }
                const bool inside = INTERIOR || (ic == i && jc == j);
                const int o = ((cpar + li + lj) & 1)*CH + lj*AXH + (li >> 1);
                s[o] = inside ? a0 : 0.0; s[2*CH + o] = inside ? a1 : 0.0;
            }
        }
    }
    // four red-black half-sweeps in LDS, colour 0 first (the block-row path of smooth_tile)
    __device__ __forceinline__ void sweeps (double* s)
    {
        double* s0p = s; double* s1p = s + 2*CH;
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int row = (blk*GP + m + 1)*AXH + pk;
#pragma unroll
            for (int p = 0; p < 2; ++p) { const int h = hx[m] ^ p; l0[m][p] = s0p[p*CH + row + h]; l1[m][p] = s1p[p*CH + row + h]; }
        }
#pragma unroll
        for (int icolor = 0; icolor < 4; ++icolor) {
            const int p = icolor & 1;
#pragma unroll
            for (int m = 0; m < GP; ++m) {
                const int h = hx[m] ^ p;
                const int row = (blk*GP + m + 1)*AXH + pk;
                const double* nb0 = &s0p[(1 - p)*CH + row];
                const double* nb1 = &s1p[(1 - p)*CH + row];
                const double we0 = nb0[h] + l0[m][1 - p], we1 = nb1[h] + l1[m][1 - p];
                const double b0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], b1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                const double t0 = (m + 1 < GP) ? l0[m + 1 < GP ? m + 1 : m][1 - p] : nb0[h + AXH], t1 = (m + 1 < GP) ? l1[m + 1 < GP ? m + 1 : m][1 - p] : nb1[h + AXH];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], we0, fym[m], b0, t0, ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], we1, fym[m], b1, t1, ci[m][p]);
                if (INTERIOR || in[m][p]) { s0p[p*CH + row + h] = n0; s1p[p*CH + row + h] = n1; l0[m][p] = n0; l1[m][p] = n1; }
            }
            __syncthreads();
        }
    }
    // the cells at least 3 inside the swept tile are final
    __device__ __forceinline__ void store (const FView& out) const
    {
#pragma unroll
        for (int m = 0; m < GP; ++m) {
            const int jj = blk*GP + m;
            const bool rowok = (jj >= 3 && jj < SY - 3);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int ii = 2*pk + (hx[m] ^ p);
                if (rowok && ii >= 3 && ii < SX - 3 && in[m][p]) { out(gi0 + ii, gj0 + jj, 0) = l0[m][p]; out(gi0 + ii, gj0 + jj, 1) = l1[m][p]; }
            }
        }
    }
};

// swept origin of the coarser level under a level whose swept region starts at g (see "Geometry" above)
__device__ __forceinline__ int up_coarse_origin (int g, int vl, int vh) { return (min(max(g - 1, vl), vh) >> 1) - 3; }

template <class TS, int NL, bool INTERIOR>
__device__ __forceinline__ void up_fused_tile (double* s1, double* s2, double* s3, const UpArgs& A, int gi0, int gj0, const StopRule& sr)
{
    constexpr int X2 = (TS::TX + 2)/2 + 7, Y2 = (TS::TY + 2)/2 + 7, X3 = (X2 + 2)/2 + 7, Y3 = (Y2 + 2)/2 + 7;
    UpLev<TS::TX, TS::TY, TS::NT, INTERIOR, false> L1;
    UpLev<X2, Y2, TS::NT, false, NL == 2> L2;
    UpLev<X3, Y3, TS::NT, false, true> L3;
    const int g2i = up_coarse_origin(gi0, A.l[0].b.vlx, A.l[0].b.vhx), g2j = up_coarse_origin(gj0, A.l[0].b.vly, A.l[0].b.vhy);
    L1.issue(A.l[0], A.crse, gi0, gj0);
    L2.issue(A.l[1], A.crse, g2i, g2j);
    if constexpr (NL == 3)
        L3.issue(A.l[2], A.crse, up_coarse_origin(g2i, A.l[1].b.vlx, A.l[1].b.vhx), up_coarse_origin(g2j, A.l[1].b.vly, A.l[1].b.vhy));
    {   // the gate of a speculative V-cycle behind the issued loads, as in smooth_tile
        const bool active = vcycle_active(sr);
        L1.keep(); L2.keep();
        if constexpr (NL == 3) L3.keep();
        if (!active) return;
    }
    if constexpr (NL == 3) {
        L3.coefficients(A.l[2]);
        L3.fill(s3, A.l[2], &L3, s3);
        __syncthreads();
        L3.sweeps(s3);
    }
    L2.coefficients(A.l[1]);
    L2.fill(s2, A.l[1], &L3, s3);
    __syncthreads();
    L2.sweeps(s2);
    L1.coefficients(A.l[0]);
    L1.fill(s1, A.l[0], &L2, s2);
    __syncthreads();
    L1.sweeps(s1);
    L1.store(A.out);
}

template <class TS, int NL>
__global__ __launch_bounds__(TS::NT, 1)      // one workgroup per CU (the grid has about as many workgroups as the chip has CUs): no register cap
void k_up_fused (UpArgs A, StopRule sr)
{
    static_assert(NL == 2 || NL == 3, "two or three mid levels");
    constexpr int X2 = (TS::TX + 2)/2 + 7, Y2 = (TS::TY + 2)/2 + 7, X3 = (X2 + 2)/2 + 7, Y3 = (Y2 + 2)/2 + 7;
    __shared__ double s1[2*TS::AX*TS::AY];
    __shared__ double s2[2*(X2 + 2)*(Y2 + 2)];
    __shared__ double s3[NL == 3 ? 2*(X3 + 2)*(Y3 + 2) : 1];
    constexpr int E = 3, FX = TS::TX - 2*E, FY = TS::TY - 2*E;
    const LevBox& b = A.l[0].b;
    // k_smooth's tiling and its XCD-contiguous tile mapping
    const unsigned wg = blockIdx.x;
    const int nb = gridDim.x, q8 = nb >> 3, r8 = nb & 7, xcd = wg & 7;
    const int tile = xcd*q8 + min(xcd, r8) + (wg >> 3);
    const int bx = tile % A.ntx, by = tile / A.ntx;
    const int gi0 = b.vlx + bx*FX - E, gj0 = b.vly + by*FY - E;
    const bool interior = (gi0 - 1 >= b.vlx) && (gi0 + TS::TX <= b.vhx) && (gj0 - 1 >= b.vly) && (gj0 + TS::TY <= b.vhy)
                       && (gi0 > b.lox) && (gi0 + TS::TX - 1 < b.hix) && (gj0 > b.loy) && (gj0 + TS::TY - 1 < b.hiy);
    if (interior) up_fused_tile<TS, NL, true>(s1, s2, s3, A, gi0, gj0, sr);
    else          up_fused_tile<TS, NL, false>(s1, s2, s3, A, gi0, gj0, sr);
}

} // namespace hps
#endif
