// beam_push.h -- the moving beam's slice push (AdvanceBeamParticlesSlice, particles/pusher/BeamParticleAdvance.cpp:20-336) as a
// kernel template: beam.hip instantiates k_beam_push<ORDER, false, MULTI>, the push of a deck without parsed external fields;
// beam_ext.hip instantiates k_beam_push<ORDER, true, MULTI>, which runs the expression programs of beams.external_E / external_B
// (expr.h) at every sub-step, in a translation unit with compiler options of its own (Makefile).  MULTI = true is
// the push of an engine with several beam species: every lane takes charge / mass, the sub-cycle count and length,
// do_z_push, the radiation reaction and the anomalous moment from its species' record; MULTI = false reads no tag and no table.
#ifndef HPS_BEAM_PUSH_H_
#define HPS_BEAM_PUSH_H_

#include "common.h"
#include "particle_math.h"
#include "engine.h"
#include "expr.h"

namespace hps {

struct BeamPushConsts {
    double dt;                 // per sub-cycle
    double c, inv_c2, qm, min_z;
    double ex_slope, ey_slope, ez_slope; // beams.external_E = (ex_slope*x, ey_slope*y, ez_slope*z)
    int nsc;
    PartConsts pc;             // geometry, boundary
    // radiation reaction (BeamParticleAdvance.cpp:101-113, 244-297): rr != 0 switches it on
    int rr, normalized, no_z_push;
    double RRcoeff, E0, wp_inv, c_SI;
    // spin tracking (:218-238): spin != 0 switches it on
    int spin; double spin_anom;
};

// beams.external_E / external_B as programs (Engine::BeamExt): ins = six {offset, count} header slots (Ex Ey Ez Bx By Bz, in
// the instruction's two words) and the instructions behind them; t = the step's physical time.  EXT = false: nothing.
template <bool EXT> struct BeamExtArgs {};
template <> struct BeamExtArgs<true> { const hps_expr_ins* ins; const double* consts; double t; };

// The push's launch bookkeeping (Engine::beam_launched): bit (4*ORDER + 2*EXT + MULTI)
constexpr unsigned long beam_push_bit (int order, bool ext, bool multi) { return 1UL << (4*order + 2*(ext ? 1 : 0) + (multi ? 1 : 0)); }

// EXT = false is the push of a deck without programs.  EXT = true adds the programs' fields to the gathered ones; its dynamic
// LDS is the operand stack of expr_run, (depth - 1) levels of blockDim.x doubles (expr.h).
template <int ORDER, bool EXT, bool MULTI>
__global__ __launch_bounds__(256)
void k_beam_push (SlabView f, BeamSoA b, const long* __restrict__ B, int p, int cPsi, int cEz, int cBx, int cBy, int cBz,
                  BeamPushConsts k, BeamExtArgs<EXT> ext, BeamMultiArgs<MULTI> multi)
{
    constexpr int NS = ORDER + 2;
    const long first = B[p], count = B[p + 1] - first;       // slipped-in particles included (:131)
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
    const long ip = first + t;
    int i = b.nsub[ip];
    if (i < 0) continue;
    double xp = b.x[ip], yp = b.y[ip], zp = b.z[ip], ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (k.spin) { s0 = b.sx[ip]; s1 = b.sy[ip]; s2 = b.sz[ip]; }
    bool absorbed = false;
    // the per-species constants: the launch's (one species), or this lane's record of the species table
    double dt = k.dt, qm = k.qm, RRcoeff = k.RRcoeff, spin_anom = k.spin_anom;
    int nsc = k.nsc, rr = k.rr, no_z_push = k.no_z_push;
    if constexpr (MULTI) {
        const BeamSpeciesRec& r = multi.tab[b.sp[ip]];
        dt = r.dt; qm = r.qm; RRcoeff = r.RRcoeff; spin_anom = r.spin_anom; nsc = r.nsc; rr = r.rr; no_z_push = r.no_z_push;
    }
    for (; i < nsc; ++i) {
        if (zp < k.min_z) break;                              // not on this slice any more (:150-153)
        const double gi = 1.0/sqrt(1.0 + (ux*ux + uy*uy + uz*uz)*k.inv_c2);
        xp += dt*0.5*ux*gi;
        yp += dt*0.5*uy*gi;
        if (apply_particle_bc(k.pc, xp, yp, ux, uy)) { absorbed = true; break; }
        // beams.external_E / external_B as programs: the components that are present, at (xp, yp, zp, time of the step)
        // (ExternalFields.H:43-48).  Evaluated ahead of the gather, whose weights and sums then do not live across the interpreter.
        double e0 = 0.0, e1 = 0.0, e2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        if constexpr (EXT) {
            extern __shared__ double s_expr_stack[];
            ExprLdsStack st{s_expr_stack + threadIdx.x, (int)blockDim.x};
            const ExprXyzt v{xp, yp, zp, ext.t};
            for (int q = 0; q < 6; ++q) {      // one inlined interpreter; q, offset and count are wave-uniform
                const int off = ext.ins[q].op, cnt = ext.ins[q].arg;
                if (cnt == 0) continue;
                const double r = expr_run(ext.ins + off, cnt, ext.consts, v, st);
                if (q == 0) e0 = r; else if (q == 1) e1 = r; else if (q == 2) e2 = r;
                else if (q == 3) b0 = r; else if (q == 4) b1 = r; else b2 = r;
            }
        }
        // doGatherShapeN (particles/particles_utils/FieldGather.H:45-96)
        double sx[NS], dsx[NS], sy[NS], dsy[NS];
        const int i0 = nodal_weights<ORDER>((xp - k.pc.xoff)*k.pc.dx_inv, sx, dsx);
        const int j0 = nodal_weights<ORDER>((yp - k.pc.yoff)*k.pc.dy_inv, sy, dsy);
        double ExmBy = 0.0, EypBx = 0.0, Ez = 0.0, Bx = 0.0, By = 0.0, Bz = 0.0;
#pragma unroll
        for (int iy = 0; iy < NS; ++iy) {
#pragma unroll
            for (int ix = 0; ix < NS; ++ix) {
                const double* q = f.p + f.off(i0 + ix, j0 + iy);
                const double psi_c = q[cPsi*f.ns];
                const double ss = sx[ix]*sy[iy];
                ExmBy += (dsx[ix]*sy[iy])*psi_c*k.pc.dx_inv;
                EypBx += (sx[ix]*dsy[iy])*psi_c*k.pc.dy_inv;
                Ez += ss*q[cEz*f.ns];
                Bx += ss*q[cBx*f.ns];
                By += ss*q[cBy*f.ns];
                Bz += ss*q[cBz*f.ns];
            }
        }
        // ApplyExternalField (particles/pusher/ExternalFields.H:29-56), E = (ex_slope x, ey_slope y, ez_slope z), B = 0
        ExmBy += k.ex_slope*xp;
        EypBx += k.ey_slope*yp;
        if (k.ez_slope != 0.0) Ez += k.ez_slope*zp;
        if constexpr (EXT) {      // ... and the parsed components (:50-55)
            ExmBy += e0 - k.c*b1;
            EypBx += e1 + k.c*b0;
            Ez += e2;
            Bx += b0; By += b1; Bz += b2;
        }
        double ux_next = ux + dt*qm*(ExmBy + (k.c - uz*gi)*By + uy*gi*Bz);
        double uy_next = uy + dt*qm*(EypBx + (uz*gi - k.c)*Bx - ux*gi*Bz);
        const double ux_i = (ux_next + ux)*0.5, uy_i = (uy_next + uy)*0.5;
        const double uz_i = uz + dt*0.5*qm*Ez;
        const double gii = 1.0/sqrt(1.0 + (ux_i*ux_i + uy_i*uy_i + uz_i*uz_i)*k.inv_c2);
        if (k.spin) {      // Thomas-BMT precession as a Boris-type rotation (:218-238)
            const double ic = 1.0/k.c;
            const double E0_ = ExmBy + k.c*By, E1_ = EypBx - k.c*Bx, E2_ = Ez;
            const double u0 = ux_i*ic, u1 = uy_i*ic, u2 = uz_i*ic;
            const double be0 = u0*gii, be1 = u1*gii, be2 = u2*gii;
            const double gp1 = gii/(1.0 + gii);
            const double x0 = be1*E2_ - be2*E1_, x1 = be2*E0_ - be0*E2_, x2 = be0*E1_ - be1*E0_;      // beta x E
            const double bdB = be0*Bx + be1*By + be2*Bz;
            const double aq = fabs(qm);
            const double h0 = aq*(Bx*gii - x0*ic*gp1 + spin_anom*(Bx - gp1*u0*bdB - x0*ic))*dt*0.5;
            const double h1 = aq*(By*gii - x1*ic*gp1 + spin_anom*(By - gp1*u1*bdB - x1*ic))*dt*0.5;
            const double h2 = aq*(Bz*gii - x2*ic*gp1 + spin_anom*(Bz - gp1*u2*bdB - x2*ic))*dt*0.5;
            const double p0 = s0 + (h1*s2 - h2*s1), p1 = s1 + (h2*s0 - h0*s2), p2 = s2 + (h0*s1 - h1*s0);   // s' = s + h x s
            const double o = 1.0/(1.0 + (h0*h0 + h1*h1 + h2*h2));
            const double hd = h0*p0 + h1*p1 + h2*p2;
            s0 = o*(p0 + (hd*h0 + (h1*p2 - h2*p1)));
            s1 = o*(p1 + (hd*h1 + (h2*p0 - h0*p2)));
            s2 = o*(p2 + (hd*h2 + (h0*p1 - h1*p0)));
        }
        double uz_next = uz + dt*qm*(Ez + (ux_i*By - uy_i*Bx)*gii);
        if (rr) {      // classical radiation reaction in SI quantities (:244-297)
            const double icSI = 1.0/k.c_SI, ic = 1.0/k.c;
            double Ex = ExmBy + k.c*By, Ey = EypBx - k.c*Bx, Ezs = Ez, Bxs = Bx, Bys = By, Bzs = Bz;
            if (k.normalized) { Ex *= k.E0; Ey *= k.E0; Ezs *= k.E0; Bxs *= k.E0*icSI; Bys *= k.E0*icSI; Bzs *= k.E0*icSI; }
            const double gam = sqrt(1.0 + (ux_i*ux_i + uy_i*uy_i + uz_i*uz_i)*k.inv_c2);
            const double vx = ux_i*gii*k.c_SI*ic, vy = uy_i*gii*k.c_SI*ic, vz = uz_i*gii*k.c_SI*ic;
            const double bx = vx*icSI, by = vy*icSI, bz = vz*icSI;
            const double flx = (Ex + vy*Bzs - vz*Bys), fly = (Ey + vz*Bxs - vx*Bzs), flz = (Ezs + vx*Bys - vy*Bxs);
            const double fl2 = flx*flx + fly*fly + flz*flz;
            const double bE = (bx*Ex + by*Ey + bz*Ezs);
            const double coeff = gam*gam*(fl2 - bE*bE);
            const double frx = RRcoeff*(k.c_SI*(fly*Bzs - flz*Bys) + bE*Ex - coeff*bx);
            const double fry = RRcoeff*(k.c_SI*(flz*Bxs - flx*Bzs) + bE*Ey - coeff*by);
            const double frz = RRcoeff*(k.c_SI*(flx*Bys - fly*Bxs) + bE*Ezs - coeff*bz);
            const double sc = dt*k.wp_inv*k.c*icSI;
            ux_next += frx*sc; uy_next += fry*sc; uz_next += frz*sc;
        }
        const double gni = 1.0/sqrt(1.0 + (ux_next*ux_next + uy_next*uy_next + uz_next*uz_next)*k.inv_c2);
        xp += dt*0.5*ux_next*gni;
        yp += dt*0.5*uy_next*gni;
        if (!no_z_push) zp += dt*(uz_next*gni - k.c);     // do_z_push (:316)
        ux = ux_next; uy = uy_next; uz = uz_next;
    }
    if (absorbed || apply_particle_bc(k.pc, xp, yp, ux, uy)) { b.w[ip] = 0.0; b.nsub[ip] = -1; continue; }
    b.x[ip] = xp; b.y[ip] = yp; b.z[ip] = zp; b.nsub[ip] = i;
    b.ux[ip] = ux; b.uy[ip] = uy; b.uz[ip] = uz;
    if (k.spin) { b.sx[ip] = s0; b.sy[ip] = s1; b.sz[ip] = s2; }
    }
}

#define HPS_BEAM_ORDER(order, CALL) switch (order) { case 0: { CALL(0); } break; case 1: { CALL(1); } break; \
                                                     case 2: { CALL(2); } break; default: { CALL(3); } break; }

// beam_ext.hip: the launch of k_beam_push<ORDER, true, MULTI> for slice p (256 lanes per workgroup, as `grid` was sized)
int beam_push_launch_ext (Engine& E, const SlabView& f, int p, int cPsi, int cEz, int cBx, int cBy, int cBz, const BeamPushConsts& k, dim3 grid);

} // namespace hps
#endif
