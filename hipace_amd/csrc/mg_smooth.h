// mg_smooth.h -- the LDS-tiled smoother of the levels above the lower V: smooth_tile and its kernel k_smooth (every tile shape,
// both centrings, down-leg / up-leg / initial pass / the fused 8-sweep end of a V-cycle on level 0), and the small kernels that
// work a level in global memory: k_restrict, k_copy2, k_bottom_sweep.  Needs mg_stencil.h, and mg_lower_v3.h for the guest
// workgroup of the initial pass (CoefGuest, coef_guest_derive).
#ifndef HPS_MG_SMOOTH_H_
#define HPS_MG_SMOOTH_H_

#include "mg_stencil.h"
#include "mg_lower_v3.h"

namespace hps {

// row (within the tile) and pair index of a thread's m-th cell pair (BR: block rows, see the note above FView)
#define MG_ROWPK(m) const int jj = BR ? (tid / PR)*GPAIRS + (m) : (tid + MG_NT*(m)) / PR, pk = BR ? (tid & (PR - 1)) : (tid + MG_NT*(m)) - jj*PR
// phi_out = GSRB^4(start), start = 0 | phi_in | phi_in + P(crse);
// DO_RES: residual r = rhs - L(phi_out), max|r| (and max|rhs|) -> norms;
//         FUSE_R (cell-centred): cres = R(r) written straight to the next level; else r -> res_out.
// INTERIOR tiles (no swept cell on a wall / outside the box) take a path without masks.
// RPULL (node-centred down-leg): the tile's right-hand side IS the restriction of the finer level's residual -- `crse` then
// is that residual (level above, twice the index), formed while the tile loads (9 reads per cell) and written to `rhs` for
// the up-leg by the tile that finalises the cell: no k_restrict launch between two levels' smoothers
template <class TS, bool CC, int SRC, bool DO_RES, bool FUSE_R, bool INTERIOR, int NSW, bool GATE_IN = (NSW == 4), bool RPULL = false>
__device__ __forceinline__ void smooth_tile (double (&s_phi)[2][TS::AY*TS::AX], double* s_red, double* s_crs, const LevBox& b, const FView& phi_out,
                                             const FView& phi_out2, const FView& rhs, const FView& acf, const FView& phi_in, const FView& crse,
                                             const FView& res_out, const FView& cres_out, double facx, double facy,
                                             int gi0, int gj0, unsigned long long* resnorm, unsigned long long* rhsnorm, const StopRule& sr)
{
    constexpr int E = DO_RES ? NSW : NSW - 1;         // rim of the swept tile that is not final
    constexpr int GT_X = TS::TX, GT_Y = TS::TY, GA_X = TS::AX, GA_Y = TS::AY, MG_NT = TS::NT, GPAIRS = TS::GPAIRS, PR = TS::PR;
    constexpr int AXH = GA_X/2, CH = GA_Y*AXH;        // entries per row / per plane of one colour
    constexpr bool BR = GPAIRS <= 2 || INTERIOR;
    const int tid = threadIdx.x;
    const int cpar = (gi0 + gj0) & 1;                 // colour of ringed cell (0, 0) is (gi0 - 1 + gj0 - 1) & 1
    MG_STAMP(0);
    // per-thread cell pairs: rhs, coefficient and inverse diagonal stay in registers.  Index p is the
    // sweep parity in which the cell is updated (p = 0: sweeps 0 and 2, p = 1: sweeps 1 and 3), so
    // that every register array below is indexed by compile-time constants only.
    double r0[GPAIRS][2], r1[GPAIRS][2], ac[GPAIRS][2], ci[GPAIRS][2];
    bool in[GPAIRS][2];
    int hx[GPAIRS];                                   // x offset (0/1) within the pair of the p = 0 cell
    double fxm[GPAIRS][2], fym[GPAIRS];               // wall multipliers (boundary tiles only)
    double rmax = 0.0;
#pragma unroll
    for (int m = 0; m < GPAIRS; ++m) {
        MG_ROWPK(m);
        const int j = gj0 + jj;
        hx[m] = (gi0 + 2*pk + j) & 1;                 // colour 0 cell: (i + j) even
        fym[m] = INTERIOR ? facy : wall_mult<CC>(j, b.loy, b.hiy, facy);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i = gi0 + 2*pk + (hx[m] ^ p);
            fxm[m][p] = INTERIOR ? facx : wall_mult<CC>(i, b.lox, b.hix, facx);
            const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
            const bool ok = INTERIOR || (ic == i && jc == j);
            in[m][p] = ok;
            double a0, a1;
            if constexpr (RPULL) { a0 = restrict_at<CC>(crse, ic, jc, 0); a1 = restrict_at<CC>(crse, ic, jc, 1); }
            else { a0 = rhs(ic, jc, 0); a1 = rhs(ic, jc, 1); }
            const double a2 = acf(ic, jc, 0);
            r0[m][p] = ok ? a0 : 0.0;
            r1[m][p] = ok ? a1 : 0.0;
            ac[m][p] = ok ? a2 : 0.0;
            ci[m][p] = 1.0/diag_c0<CC>(i, j, b, ac[m][p], facx, facy);
            if (rhsnorm) rmax = fmax(rmax, fmax(fabs(r0[m][p]), fabs(r1[m][p])));
        }
    }
    MG_STAMP(1);
    // fill LDS (ring included): start value inside the unknowns' box, 0 elsewhere.  Loads are
    // unconditional (clamped address + select) and all issued before the first LDS store.
    {
        constexpr int NF = (GA_X*GA_Y + MG_NT - 1)/MG_NT;
        double v0[NF], v1[NF];
        // Node-centred prolongation (bilinear: up to four coarse values per fine cell) THROUGH LDS: asked for from global memory
        // inside the loop below, the 7 cells of a thread had up to 70 loads in flight -- the fused 8-sweep pass of level 0 spilled
        // 39 registers under its 128-register cap (58 us against 32 for the cell-centred pass, n = 1023).  The coarse cells under
        // the ringed tile go to LDS once (one load per coarse cell instead of one per fine neighbour), the interpolation reads them there.
        constexpr bool PLDS = !CC && SRC == SRC_PROLONG;
        constexpr int CXN = GA_X/2 + 2, CYN = GA_Y/2 + 2;
        const int cx0 = (INTERIOR ? gi0 - 1 : min(max(gi0 - 1, b.vlx), b.vhx)) >> 1, cy0 = (INTERIOR ? gj0 - 1 : min(max(gj0 - 1, b.vly), b.vhy)) >> 1;
        if constexpr (PLDS) {
            const int cxl = b.vlx >> 1, cxh = (b.vhx >> 1) + 1, cyl = b.vly >> 1, cyh = (b.vhy >> 1) + 1;      // the coarse level's box, walls included
            constexpr int NC = (CXN*CYN + MG_NT - 1)/MG_NT;
            double c0[NC], c1[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int q = min(tid + MG_NT*m, CXN*CYN - 1);
                const int ly = q / CXN, lx = q - ly*CXN;
                const int X = min(max(cx0 + lx, cxl), cxh), Y = min(max(cy0 + ly, cyl), cyh);
                c0[m] = crse(X, Y, 0); c1[m] = crse(X, Y, 1);
            }
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int q = tid + MG_NT*m;
                if (q < CXN*CYN) { s_crs[q] = c0[m]; s_crs[CXN*CYN + q] = c1[m]; }
            }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = min(tid + MG_NT*m, GA_X*GA_Y - 1);
            const int lj = s / GA_X, li = s - lj*GA_X;
            const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
            v0[m] = 0.0; v1[m] = 0.0;
            if (SRC != SRC_ZERO) {
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                double a0 = phi_in(ic, jc, 0), a1 = phi_in(ic, jc, 1);
                if (SRC == SRC_PROLONG && !PLDS) { a0 += prolong_at<CC>(crse, ic, jc, 0); a1 += prolong_at<CC>(crse, ic, jc, 1); }
                const bool inside = INTERIOR || (ic == i && jc == j);
                v0[m] = inside ? a0 : 0.0; v1[m] = inside ? a1 : 0.0;
            }
        }
        if constexpr (PLDS) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < NF; ++m) {
                const int s = min(tid + MG_NT*m, GA_X*GA_Y - 1);
                const int lj = s / GA_X, li = s - lj*GA_X;
                const int i = gi0 - 1 + li, j = gj0 - 1 + lj;
                const int ic = INTERIOR ? i : min(max(i, b.vlx), b.vhx), jc = INTERIOR ? j : min(max(j, b.vly), b.vhy);
                const bool inside = INTERIOR || (ic == i && jc == j);
                // prolong_at<false>'s four cases with its order of additions, on the LDS copy
                const int o = ((jc >> 1) - cy0)*CXN + (ic >> 1) - cx0;
                const bool io = (ic & 1), jo = (jc & 1);
                double p0, p1;
                const double* q0 = s_crs + o; const double* q1 = s_crs + CXN*CYN + o;
                if (io && jo)  { p0 = (q0[0] + q0[1] + q0[CXN] + q0[CXN + 1])*0.25; p1 = (q1[0] + q1[1] + q1[CXN] + q1[CXN + 1])*0.25; }
                else if (io)   { p0 = (q0[0] + q0[1])*0.5; p1 = (q1[0] + q1[1])*0.5; }
                else if (jo)   { p0 = (q0[0] + q0[CXN])*0.5; p1 = (q1[0] + q1[CXN])*0.5; }
                else           { p0 = q0[0]; p1 = q1[0]; }
                if (inside) { v0[m] += p0; v1[m] += p1; }
            }
        }
        {   // The gate of a speculative V-cycle, read while ALL the tile's loads are in flight (a kernel's first dependent
            // read of global memory costs ~1.5 us behind a kernel boundary; read first, the gate was one such trip ahead
            // of the loads).  HPS_KEEP: the loads must not sink below the branch.
            // Only the 4-sweep kernels of the coarser levels do this (a handful of workgroups, each a chain of latencies);
            // the 8-sweep pass of level 0 is bound by bandwidth and registers (all its operands live at once would cost
            // it a workgroup per CU) and reads its gate first.
            if (GATE_IN) {
                const bool active = vcycle_active(sr);
#pragma unroll
                for (int m = 0; m < GPAIRS; ++m) { HPS_KEEP(r0[m][0]); HPS_KEEP(r0[m][1]); HPS_KEEP(r1[m][0]); HPS_KEEP(r1[m][1]); HPS_KEEP(ac[m][0]); HPS_KEEP(ac[m][1]); }
#pragma unroll
                for (int m = 0; m < NF; ++m) { HPS_KEEP(v0[m]); HPS_KEEP(v1[m]); }
                if (!active) return;
            }
        }
        // LDS layout: the two colours of the red-black ordering in separate planes (cell (li, lj) of the
        // ringed tile -> plane (i + j) & 1, row lj, entry li >> 1): a half-sweep then reads and writes
        // consecutive doubles per lane instead of every other one (which is a 2-way bank conflict).
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            const int s = tid + MG_NT*m;
            if (s < GA_X*GA_Y) {
                const int lj = s / GA_X, li = s - lj*GA_X;
                const int o = ((cpar + li + lj) & 1)*CH + lj*AXH + (li >> 1);
                s_phi[0][o] = v0[m]; s_phi[1][o] = v1[m];
            }
        }
    }
    __syncthreads();
    MG_STAMP(2);

    double l0[GPAIRS][2], l1[GPAIRS][2];              // BR: the thread's own cells, as it wrote them last (pair, sweep parity of the cell)
    if constexpr (BR) {
        // the thread's own cells, as it wrote them last (index: pair, sweep parity of the cell)
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int row = (jj + 1)*AXH + pk;
#pragma unroll
            for (int p = 0; p < 2; ++p) { const int h = hx[m] ^ p; l0[m][p] = s_phi[0][p*CH + row + h]; l1[m][p] = s_phi[1][p*CH + row + h]; }
        }
#pragma unroll
        for (int icolor = 0; icolor < NSW; ++icolor) {
            const int p = icolor & 1;                     // compile-time after unrolling
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                const int h = hx[m] ^ p;
                // self: plane p, entry pk + h.  West / east: the partner (register) and entry pk + h of plane 1-p (the pair's other side);
                // south / north: the block's own rows (registers) or entry pk + h of the rows below / above it
                const int row = (jj + 1)*AXH + pk;
                const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                const double we0 = nb0[h] + l0[m][1 - p], we1 = nb1[h] + l1[m][1 - p];      // (west + east: a + b = b + a to the bit)
                const double s0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], s1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                const double t0 = (m + 1 < GPAIRS) ? l0[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb0[h + AXH], t1 = (m + 1 < GPAIRS) ? l1[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb1[h + AXH];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], we0, fym[m], s0, t0, ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], we1, fym[m], s1, t1, ci[m][p]);
                if (INTERIOR || in[m][p]) { s_phi[0][p*CH + row + h] = n0; s_phi[1][p*CH + row + h] = n1; l0[m][p] = n0; l1[m][p] = n1; }
            }
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int icolor = 0; icolor < NSW; ++icolor) {
            constexpr int dummy = 0; (void)dummy;
            const int p = icolor & 1;                     // compile-time after unrolling
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                const int h = hx[m] ^ p;
                // self: plane p, entry pk + h; west / east: plane 1-p, entries pk, pk + 1; south / north: pk + h
                const int row = (jj + 1)*AXH + pk;
                const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                const double n0 = gs_cell(r0[m][p], fxm[m][p], nb0[0] + nb0[1], fym[m], nb0[h - AXH], nb0[h + AXH], ci[m][p]);
                const double n1 = gs_cell(r1[m][p], fxm[m][p], nb1[0] + nb1[1], fym[m], nb1[h - AXH], nb1[h + AXH], ci[m][p]);
                if (INTERIOR || in[m][p]) { s_phi[0][p*CH + row + h] = n0; s_phi[1][p*CH + row + h] = n1; }
            }
            __syncthreads();
        }
    }
    MG_STAMP(3);

    double resmax = 0.0;
    if constexpr (BR) {
        double la0[GPAIRS], ra0[GPAIRS], la1[GPAIRS], ra1[GPAIRS];      // FUSE_R: residual of the left / right cell of a pair, per component
        bool finr[GPAIRS];
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int j = gj0 + jj;
            const bool rowok = (jj >= E && jj < GT_Y - E);
            double q0[2], q1[2];                          // by sweep parity p
            bool fin[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int h = hx[m] ^ p;
                const int ii = 2*pk + h;
                fin[p] = rowok && ii >= E && ii < GT_X - E && in[m][p];
                const int i = gi0 + ii;
                const int row = (jj + 1)*AXH + pk;
                const double f0 = l0[m][p], f1 = l1[m][p];
                q0[p] = 0.0; q1[p] = 0.0;
                if (DO_RES) {
                    const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                    const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                    const double o0 = nb0[h], o1 = nb1[h];                      // the pair's other side; the partner is in a register
                    const double w0 = h ? l0[m][1 - p] : o0, e0 = h ? o0 : l0[m][1 - p];
                    const double w1 = h ? l1[m][1 - p] : o1, e1 = h ? o1 : l1[m][1 - p];
                    const double s0 = (m > 0) ? l0[m > 0 ? m - 1 : 0][1 - p] : nb0[h - AXH], s1 = (m > 0) ? l1[m > 0 ? m - 1 : 0][1 - p] : nb1[h - AXH];
                    const double n0 = (m + 1 < GPAIRS) ? l0[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb0[h + AXH], n1 = (m + 1 < GPAIRS) ? l1[m + 1 < GPAIRS ? m + 1 : m][1 - p] : nb1[h + AXH];
                    const double t0 = residual_v<INTERIOR>(f0, w0, e0, s0, n0, i, j, b, r0[m][p], ac[m][p], facx, facy);
                    const double t1 = residual_v<INTERIOR>(f1, w1, e1, s1, n1, i, j, b, r1[m][p], ac[m][p], facx, facy);
                    q0[p] = fin[p] ? t0 : 0.0; q1[p] = fin[p] ? t1 : 0.0;
                    resmax = fmax(resmax, fmax(fabs(q0[p]), fabs(q1[p])));
                }
                if (fin[p]) {
                    if constexpr (RPULL) { rhs(i, j, 0) = r0[m][p]; rhs(i, j, 1) = r1[m][p]; }
                    if (DO_RES && !FUSE_R) { res_out(i, j, 0) = q0[p]; res_out(i, j, 1) = q1[p]; }
                    phi_out(i, j, 0) = f0;
                    phi_out(i, j, 1) = f1;
                    if (phi_out2.p) { phi_out2(i, j, 0) = f0; phi_out2(i, j, 1) = f1; }
                }
            }
            const bool sw = (hx[m] != 0);             // the p = 0 cell is the right one
            la0[m] = sw ? q0[1] : q0[0]; ra0[m] = sw ? q0[0] : q0[1];
            la1[m] = sw ? q1[1] : q1[0]; ra1[m] = sw ? q1[0] : q1[1];
            finr[m] = fin[0];
        }
        if (FUSE_R) {
            // restrict_cc (:29-37): 0.25*(((a+b)+c)+d), a,b = left,right cell of an even row, c,d the row above.  Tile origins are
            // even, so a pair is one coarse cell's x-extent; the row above an even row is the thread's next pair, or -- for the last
            // row of its block -- the first pair of the thread PR lanes on (a wave holds 64/PR consecutive blocks, an even number of
            // rows from an even row on: the pairs that straddle two blocks never straddle two waves)
            const double c0 = __shfl_down(la0[0], PR), d0 = __shfl_down(ra0[0], PR);
            const double c1 = __shfl_down(la1[0], PR), d1 = __shfl_down(ra1[0], PR);
#pragma unroll
            for (int m = 0; m < GPAIRS; ++m) {
                MG_ROWPK(m);
                if (finr[m] && ((jj & 1) == 0)) {
                    const bool own = (m + 1 < GPAIRS);
                    const int mu = own ? m + 1 : m;
                    const double ua0 = own ? la0[mu] : c0, ub0 = own ? ra0[mu] : d0, ua1 = own ? la1[mu] : c1, ub1 = own ? ra1[mu] : d1;
                    const int ic = (gi0 + 2*pk) >> 1, jc = (gj0 + jj) >> 1;
                    cres_out(ic, jc, 0) = 0.25*(la0[m] + ra0[m] + ua0 + ub0);
                    cres_out(ic, jc, 1) = 0.25*(la1[m] + ra1[m] + ua1 + ub1);
                }
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < GPAIRS; ++m) {
            MG_ROWPK(m);
            const int j = gj0 + jj;
            const bool rowok = (jj >= E && jj < GT_Y - E);
            double q0[2], q1[2];                          // by sweep parity p
            bool fin[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int h = hx[m] ^ p;
                const int ii = 2*pk + h;
                fin[p] = rowok && ii >= E && ii < GT_X - E && in[m][p];
                const int i = gi0 + ii;
                const int row = (jj + 1)*AXH + pk;
                const double f0 = s_phi[0][p*CH + row + h], f1 = s_phi[1][p*CH + row + h];
                q0[p] = 0.0; q1[p] = 0.0;
                if (DO_RES) {
                    const double* nb0 = &s_phi[0][(1 - p)*CH + row];
                    const double* nb1 = &s_phi[1][(1 - p)*CH + row];
                    const double t0 = residual_v<INTERIOR>(f0, nb0[0], nb0[1], nb0[h - AXH], nb0[h + AXH], i, j, b, r0[m][p], ac[m][p], facx, facy);
                    const double t1 = residual_v<INTERIOR>(f1, nb1[0], nb1[1], nb1[h - AXH], nb1[h + AXH], i, j, b, r1[m][p], ac[m][p], facx, facy);
                    q0[p] = fin[p] ? t0 : 0.0; q1[p] = fin[p] ? t1 : 0.0;
                    resmax = fmax(resmax, fmax(fabs(q0[p]), fabs(q1[p])));
                }
                if (fin[p]) {
                    if constexpr (RPULL) { rhs(i, j, 0) = r0[m][p]; rhs(i, j, 1) = r1[m][p]; }
                    if (DO_RES && !FUSE_R) { res_out(i, j, 0) = q0[p]; res_out(i, j, 1) = q1[p]; }
                    phi_out(i, j, 0) = f0;
                    phi_out(i, j, 1) = f1;
                    if (phi_out2.p) { phi_out2(i, j, 0) = f0; phi_out2(i, j, 1) = f1; }
                }
            }
            if (FUSE_R) {
                // restrict_cc (:29-37): 0.25*(((a+b)+c)+d), a,b = left,right cell of this row (even j),
                // c,d the row above.  Tile origins are even, so a pair is one coarse cell's x-extent and
                // lanes l / l+32 of a wave hold rows jj / jj+1.
                const bool sw = (hx[m] != 0);             // the p = 0 cell is the right one
                const double la0 = sw ? q0[1] : q0[0], ra0 = sw ? q0[0] : q0[1];
                const double la1 = sw ? q1[1] : q1[0], ra1 = sw ? q1[0] : q1[1];
                const double c0 = __shfl_down(la0, PR), d0 = __shfl_down(ra0, PR);
                const double c1 = __shfl_down(la1, PR), d1 = __shfl_down(ra1, PR);
                if (fin[0] && ((tid & PR) == 0)) {
                    const int ic = (gi0 + 2*pk) >> 1, jc = j >> 1;
                    cres_out(ic, jc, 0) = 0.25*(la0 + ra0 + c0 + d0);
                    cres_out(ic, jc, 1) = 0.25*(la1 + ra1 + c1 + d1);
                }
            }
        }
    }
    MG_STAMP(4);
    if (DO_RES && resnorm) block_max_to<MG_NT>(resnorm, resmax, s_red);
    if (rhsnorm) block_max_to<MG_NT>(rhsnorm, rmax, s_red);
    MG_STAMP(5);
}

// NSW red-black half-sweeps per launch: 4 (one GSRB^4 of the reference) or 8 (the two consecutive
// GSRB^4 that end a V-cycle on level 0, fused: one pass over HBM instead of two)
// GUEST (none, or one CoefGuest: the instance that makes a solve's initial level-0 pass where the lower V is k_lower_v3):
// workgroup 0 of that launch is no tile but derives the lower V's coefficient image (coef_guest_derive) in the tile's static
// LDS: it starts with the first round of tiles and is done long before the pass is; the tiles are workgroups 1 .. .  Instances
// without a guest have the same arguments and the same code as before the guest existed.
template <class TS, bool CC, int SRC, bool DO_RES, bool FUSE_R, int NSW = 4, bool RPULL = false, class... GUEST>
__global__ __launch_bounds__(TS::NT, (RPULL && TS::GPAIRS > 1) ? 2 : 4)      // at most 128 VGPRs: two 512-thread workgroups per CU (several variants sit at 113-130); the pulling smoother with two pairs per thread (36 + 36 loads in flight) gets 256
void k_smooth (LevBox b, FView phi_out, FView phi_out2, FView rhs, FView acf, FView phi_in, FView crse, FView res_out,
               FView cres_out, double facx, double facy, int ntx, unsigned long long* resnorm,
               unsigned long long* rhsnorm, StopRule sr, GUEST... guest)
{
    static_assert(!FUSE_R || (CC && DO_RES), "fused restriction is cell-centred only");
    constexpr int HOST = (int)sizeof...(GUEST);       // workgroups ahead of the tiles
    static_assert(HOST <= 1 && (HOST == 0 || (CC && NSW == 4)), "the guest rides in the cell-centred initial pass");
    // (the 4-sweep kernels read the gate behind their loads, see smooth_tile; the 8-sweep pass first: with the gate behind its
    //  loads all of the tile's operands are live across it, 61 registers spilled under its 128-register cap, round 4)
    if (NSW != 4 && !vcycle_active(sr)) return;
    constexpr int GT_X = TS::TX, GT_Y = TS::TY;
    __shared__ double s_phi[2][TS::AY*TS::AX];
    __shared__ double s_red[TS::NT/64];
    if constexpr (HOST > 0) {
        static_assert(2*TS::AY*TS::AX >= COEF_GUEST_MAX_IMG, "the image is staged in the tile's static LDS");
        if (blockIdx.x == 0) { coef_guest_derive(&s_phi[0][0], guest..., TS::NT); return; }
    }
    // node-centred prolongation goes through LDS (smooth_tile): the coarse cells under the ringed tile, two components
    constexpr bool PLDS = !CC && SRC == SRC_PROLONG;
    __shared__ double s_crs[PLDS ? 2*(TS::AX/2 + 2)*(TS::AY/2 + 2) : 1];
    constexpr int E = DO_RES ? NSW : NSW - 1;
    constexpr int FX = GT_X - 2*E, FY = GT_Y - 2*E;   // cells a tile finalises (even numbers)
    // workgroups go round-robin to the 8 XCDs: give each XCD a contiguous run of tiles, so that the
    // rims shared by neighbouring tiles hit in that XCD's L2
    // (behind a guest the runs belong to XCD (xcd + 1) & 7: contiguous all the same)
    const unsigned wg = blockIdx.x - HOST;
    const int nb = gridDim.x - HOST, q8 = nb >> 3, r8 = nb & 7, xcd = wg & 7;
    const int tile = xcd*q8 + min(xcd, r8) + (wg >> 3);
    const int bx = tile % ntx, by = tile / ntx;
    const int gi0 = b.vlx + bx*FX - E;                // global index of swept cell (0,0)
    const int gj0 = b.vly + by*FY - E;
    // every swept cell and its ring strictly inside the unknowns' box and off the walls
    const bool interior = (gi0 - 1 >= b.vlx) && (gi0 + GT_X <= b.vhx) && (gj0 - 1 >= b.vly) && (gj0 + GT_Y <= b.vhy)
                       && (gi0 > b.lox) && (gi0 + GT_X - 1 < b.hix) && (gj0 > b.loy) && (gj0 + GT_Y - 1 < b.hiy);
    constexpr bool GATE_IN = (NSW == 4);
    if (interior) smooth_tile<TS, CC, SRC, DO_RES, FUSE_R, true, NSW, GATE_IN, RPULL>(s_phi, s_red, s_crs, b, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out,
                                                             facx, facy, gi0, gj0, resnorm, rhsnorm, sr);
    else          smooth_tile<TS, CC, SRC, DO_RES, FUSE_R, false, NSW, GATE_IN, RPULL>(s_phi, s_red, s_crs, b, phi_out, phi_out2, rhs, acf, phi_in, crse, res_out, cres_out,
                                                              facx, facy, gi0, gj0, resnorm, rhsnorm, sr);
}

template <bool CC>
__global__ __launch_bounds__(256)
void k_restrict (LevBox cb, FView crse, FView fine, int ncomp, StopRule sr)
{
    if (!vcycle_active(sr)) return;
    const int i = cb.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = cb.vly + blockIdx.y;
    if (i > cb.vhx || j > cb.vhy) return;
    for (int n = 0; n < ncomp; ++n) crse(i, j, n) = restrict_at<CC>(fine, i, j, n);
}

__global__ void k_copy2 (LevBox b, FView dst, FView src)
{
    const int i = b.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = b.vly + blockIdx.y;
    if (i > b.vhx || j > b.vhy) return;
    dst(i, j, 0) = src(i, j, 0); dst(i, j, 1) = src(i, j, 1);
}

// The generic bottom: the reference's CPU branch (bottomsolve, HpMultiGrid.cpp:1583-1593), taken when the lower V would need
// more LDS than one workgroup has (no level of at most LOWV_MAX_CELLS: the coarsest level is large).  The coarsest level's
// correction is zeroed (is < 0), then swept once per launch, colour (i + j + is) % 2 == 0 in level index space, in global
// memory.  Neighbours outside a cell-centred box are not read (the wall stencil does not use them); node-centred walls hold 0.
template <bool CC>
__global__ __launch_bounds__(256)
void k_bottom_sweep (LevBox b, FView cor, FView rhs, FView acf, double facx, double facy, int is, StopRule sr)
{
    if (!vcycle_active(sr)) return;
    const int i = b.vlx + blockIdx.x*blockDim.x + threadIdx.x;
    const int j = b.vly + blockIdx.y;
    if (i > b.vhx || j > b.vhy) return;
    if (is < 0) { cor(i, j, 0) = 0.0; cor(i, j, 1) = 0.0; return; }
    if ((i + j + is) & 1) return;
    const double ci = 1.0/diag_c0<CC>(i, j, b, acf(i, j, 0), facx, facy);
    for (int n = 0; n < 2; ++n) {
        const double w = (i > b.lox) ? cor(i-1, j, n) : 0.0, e = (i < b.hix) ? cor(i+1, j, n) : 0.0;
        const double s = (j > b.loy) ? cor(i, j-1, n) : 0.0, no = (j < b.hiy) ? cor(i, j+1, n) : 0.0;
        double lx = facx*(w + e), ly = facy*(s + no);
        if (CC) {
            lx = (i == b.lox) ? facx*(4./3.)*e : ((i == b.hix) ? facx*(4./3.)*w : lx);
            ly = (j == b.loy) ? facy*(4./3.)*no : ((j == b.hiy) ? facy*(4./3.)*s : ly);
        }
        cor(i, j, n) = (rhs(i, j, n) - (lx + ly))*ci;
    }
}

} // namespace hps
#endif
