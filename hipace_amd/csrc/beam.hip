// beam.hip -- driver-beam slice operators for hipace.dt != 0: the beam slice push
// (AdvanceBeamParticlesSlice, particles/pusher/BeamParticleAdvance.cpp:20-336), the hand-off of
// slipped particles to the next slice (shiftSlippedParticles, particles/sorting/SliceSort.cpp:12-64)
// and the deposit over the part of a slice that has not slipped in during this step
// (particles/deposition/BeamDepositCurrent.cpp:100).  The push kernel itself is the template of beam_push.h; its instantiations
// with parsed external fields live in beam_ext.hip.
//
// Layout: one global SoA over all beam particles, head slice first.  Slice p (counted from the head)
// is the index range [B[p], B[p+1]) of DEVICE-resident boundaries: a particle that leaves slice p
// (z < lower end of the slice) is moved to the end of its range by the partition kernel, and B[p+1]
// is lowered past it -- it has become the front of slice p+1 without being copied anywhere, and the
// host never has to learn the counts inside a step (nfront[p+1] = how many such particles lead
// slice p+1: they are pushed there, to finish their sub-cycles, but not deposited).
#include "common.h"
#include "particle_math.h"
#include "engine.h"
#include "beam_push.h"

namespace hps {

template <int ORDER>
__global__ __launch_bounds__(256)
void k_beam_deposit_dyn (SlabView f, BeamSoA b, const long* __restrict__ B, const int* __restrict__ nfront, int p,
                         int cjx, int cjy, int cjz, double q_invvol, double clightsq_inv, PartConsts k, int* disturbed)
{
    const long first = B[p] + nfront[p], count = B[p + 1] - first;
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
    const long ip = first + t;
    if (b.nsub[ip] < 0) continue;               // absorbed at the boundary
    const double ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
    const double gaminv = 1.0/sqrt(1.0 + ux*ux*clightsq_inv + uy*uy*clightsq_inv + uz*uz*clightsq_inv);
    const double wq = q_invvol*b.w[ip];
    // (predictor-corrector loop: Engine::d_pc_dist, as k_beam_deposit)
    if (disturbed && ((cjx >= 0 && (wq*(ux*gaminv) != 0.0 || wq*(uy*gaminv) != 0.0)) || (cjz >= 0 && wq*(uz*gaminv) != 0.0)))
        __hip_atomic_store(disturbed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double sx[ORDER + 1], sy[ORDER + 1];
    const int i0 = shape_weights<ORDER>((b.x[ip] - k.xoff)*k.dx_inv, sx);
    const int j0 = shape_weights<ORDER>((b.y[ip] - k.yoff)*k.dy_inv, sy);
#pragma unroll
    for (int iy = 0; iy <= ORDER; ++iy) {
#pragma unroll
        for (int ix = 0; ix <= ORDER; ++ix) {
            double* q = f.p + f.off(i0 + ix, j0 + iy);
            const double s = sx[ix]*sy[iy];
            if (cjx >= 0) { atomic_add_f64(q + cjx*f.ns, s*(wq*(ux*gaminv))); atomic_add_f64(q + cjy*f.ns, s*(wq*(uy*gaminv))); }
            if (cjz >= 0) atomic_add_f64(q + cjz*f.ns, s*(wq*(uz*gaminv)));
        }
    }
    }
}

// One workgroup: particles of slice p with z < min_z go to the end of the slice's range, the boundary to
// slice p+1 is lowered past them.  Nothing moves when nothing slipped (the usual case).
// MOM (hipace.dt = adaptive): the first pass also reduces {sum w, sum w uz/c, sum w (uz/c)^2, min uz/c} over the particles
// that stay (z >= min_z) and are not absorbed -- GatherMinUzSlice behind shiftSlippedParticles (Hipace.cpp:703-716) -- into
// mom[0..3], the slot of slice p.  Lane t takes particles t, t + 1024, ... in order, the waves fold by a fixed butterfly and
// lane 0 of the workgroup adds the 16 waves in order: the result depends on the particles' order only, not on timing.
template <bool MOM>
__global__ __launch_bounds__(1024)
void k_beam_partition (BeamSoA b, BeamSoA scr, long* B, int* nfront, int p, double min_z, double inv_c, double* mom)
{
    __shared__ int s_cnt[2];
    __shared__ int s_red[16];
    __shared__ double s_mom[MOM ? 16 : 1][4];
    const long first = B[p], count = B[p + 1] - first;
    const int t = threadIdx.x;
    int mine = 0;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = __builtin_huge_val();
    for (long q = t; q < count; q += 1024) {
        const double z = b.z[first + q];
        mine += (z < min_z) ? 1 : 0;
        if (MOM && z >= min_z && b.nsub[first + q] >= 0) {
            const double w = b.w[first + q], u = b.uz[first + q]*inv_c;
            m0 += w; m1 += w*u; m2 += w*u*u; m3 = fmin(m3, u);
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (MOM) {
        for (int o = 32; o > 0; o >>= 1) {
            m0 += __shfl_xor(m0, o); m1 += __shfl_xor(m1, o); m2 += __shfl_xor(m2, o); m3 = fmin(m3, __shfl_xor(m3, o));
        }
        if ((t & 63) == 0) { s_mom[t >> 6][0] = m0; s_mom[t >> 6][1] = m1; s_mom[t >> 6][2] = m2; s_mom[t >> 6][3] = m3; }
    }
    if ((t & 63) == 0) s_red[t >> 6] = mine;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    if (MOM && t == 0) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = __builtin_huge_val();
        for (int w = 0; w < 16; ++w) { a0 += s_mom[w][0]; a1 += s_mom[w][1]; a2 += s_mom[w][2]; a3 = fmin(a3, s_mom[w][3]); }
        mom[0] = a0; mom[1] = a1; mom[2] = a2; mom[3] = a3;
    }
    int nslip = 0;
    for (int w = 0; w < 16; ++w) nslip += s_red[w];
    if (nslip == 0) { if (t == 0) nfront[p + 1] = 0; return; }
    for (long q = t; q < count; q += 1024) {
        const long ip = first + q;
        const bool slip = b.z[ip] < min_z;
        const long dst = slip ? count - 1 - atomicAdd(&s_cnt[1], 1) : atomicAdd(&s_cnt[0], 1);
        scr.x[dst] = b.x[ip]; scr.y[dst] = b.y[ip]; scr.z[dst] = b.z[ip]; scr.ux[dst] = b.ux[ip];
        scr.uy[dst] = b.uy[ip]; scr.uz[dst] = b.uz[ip]; scr.w[dst] = b.w[ip]; scr.nsub[dst] = b.nsub[ip];
        if (b.sx) { scr.sx[dst] = b.sx[ip]; scr.sy[dst] = b.sy[ip]; scr.sz[dst] = b.sz[ip]; }
    }
    __threadfence_block();
    __syncthreads();
    for (long q = t; q < count; q += 1024) {
        const long ip = first + q;
        b.x[ip] = scr.x[q]; b.y[ip] = scr.y[q]; b.z[ip] = scr.z[q]; b.ux[ip] = scr.ux[q];
        b.uy[ip] = scr.uy[q]; b.uz[ip] = scr.uz[q]; b.w[ip] = scr.w[q]; b.nsub[ip] = scr.nsub[q];
        if (b.sx) { b.sx[ip] = scr.sx[q]; b.sy[ip] = scr.sy[q]; b.sz[ip] = scr.sz[q]; }
    }
    if (t == 0) { B[p + 1] = first + count - nslip; nfront[p + 1] = nslip; }
}

// mom[nz + 1][4]: one slot per slice (head first) and the step's total behind them; an empty slice keeps {0, 0, 0, +inf}
__global__ void k_beam_moments_reset (double* mom, int nz)
{
    for (int i = threadIdx.x; i < 4*(nz + 1); i += blockDim.x) mom[i] = (i & 3) == 3 ? __builtin_huge_val() : 0.0;
}
// the step's total: the nz slots folded head to tail, one lane per moment (a fixed order: no atomics on doubles)
__global__ void k_beam_moments_fold (double* mom, int nz)
{
    const int k = threadIdx.x;
    if (k >= 4) return;
    double a = mom[k];
    for (int p = 1; p < nz; ++p) a = (k == 3) ? fmin(a, mom[4*p + k]) : a + mom[4*p + k];
    mom[4*nz + k] = a;
}

// ---- ring hand-off (MultiBuffer::put_data / get_data, utils/MultiBuffer.cpp:444-609) ----------------------------
// message = [count | x[cap] y[cap] z[cap] ux[cap] uy[cap] uz[cap] w[cap]]; everything stays on the device
__global__ __launch_bounds__(256)
void k_beam_export (BeamSoA b, const long* __restrict__ B, int p, double* __restrict__ msg, long cap, int* overflow)
{
    const long first = B[p], count = B[p + 1] - first;
    if (blockIdx.x == 0 && threadIdx.x == 0) { msg[0] = (double)min(count, cap); if (count > cap) atomicAdd(overflow, 1); }
    const double* a[10] = {b.x, b.y, b.z, b.ux, b.uy, b.uz, b.w, b.sx, b.sy, b.sz};
    const int rows = b.sx ? 10 : 7;
    for (long q = (long)blockIdx.x*blockDim.x + threadIdx.x; q < min(count, cap); q += (long)gridDim.x*blockDim.x)
        for (int k = 0; k < rows; ++k) msg[1 + k*cap + q] = a[k][first + q];
}

// block p of the coming step: placed behind the blocks imported so far (imp[p] = where it starts); every later
// boundary moves with it, so the slices not imported yet are empty ranges
__global__ __launch_bounds__(256)
void k_beam_import (BeamSoA b, long* B, long* imp, int p, int nz, const double* __restrict__ msg, long cap, long capacity, int* overflow)
{
    const long start = imp[p];
    long count = (long)msg[0];
    if (count > cap) count = cap;
    if (start + count > capacity) { count = capacity - start; if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(overflow, 1); }
    double* a[10] = {b.x, b.y, b.z, b.ux, b.uy, b.uz, b.w, b.sx, b.sy, b.sz};
    const int rows = b.sx ? 10 : 7;
    for (long q = (long)blockIdx.x*blockDim.x + threadIdx.x; q < count; q += (long)gridDim.x*blockDim.x) {
        for (int k = 0; k < rows; ++k) a[k][start + q] = msg[1 + k*cap + q];
        b.nsub[start + q] = 0;
    }
}
__global__ void k_beam_import_bounds (long* B, long* imp, int p, int nz, const double* __restrict__ msg, long cap, long capacity)
{
    const long start = imp[p];
    long count = (long)msg[0];
    if (count > cap) count = cap;
    if (start + count > capacity) count = capacity - start;
    if (threadIdx.x == 0) imp[p + 1] = start + count;
    for (int q = p + 1 + threadIdx.x; q <= nz; q += blockDim.x) B[q] = start + count;
}

int beam_export_slice (Engine& E, int islice, double* msg_dev, long cap)
{
    const int p = E.d.nz - 1 - islice;
    hipLaunchKernelGGL(k_beam_export, dim3((unsigned)std::max<long>(1, std::min<long>(ceil_div(cap, 256), 256))), dim3(256), 0, E.st,
                       E.bm, E.d_B, p, msg_dev, cap, E.d_beam_overflow);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_import_slice (Engine& E, int islice, const double* msg_dev, long cap)
{
    const int p = E.d.nz - 1 - islice;
    const long capacity = std::max(E.nbeam, 1L);
    hipLaunchKernelGGL(k_beam_import, dim3((unsigned)std::max<long>(1, std::min<long>(ceil_div(cap, 256), 256))), dim3(256), 0, E.st,
                       E.bm, E.d_B, E.d_Bimp, p, E.d.nz, msg_dev, cap, capacity, E.d_beam_overflow);
    hipLaunchKernelGGL(k_beam_import_bounds, dim3(1), dim3(256), 0, E.st, E.d_B, E.d_Bimp, p, E.d.nz, msg_dev, cap, capacity);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

static BeamPushConsts push_consts (const Engine& E, int islice)
{
    BeamPushConsts k{};
    const hps_deck& d = E.d;
    k.nsc = d.beam_n_subcycles > 0 ? d.beam_n_subcycles : 10;
    k.dt = E.step_dt/k.nsc;
    k.c = E.gm.c; k.inv_c2 = 1.0/(E.gm.c*E.gm.c);
    k.qm = d.beam_charge/(d.beam_mass != 0.0 ? d.beam_mass : 1.0);
    k.min_z = d.lo[2] + islice*E.gm.dz;
    k.ex_slope = d.ext_E_slope[0]; k.ey_slope = d.ext_E_slope[1]; k.ez_slope = d.ext_Ez_slope;
    k.pc = base_consts(E.gm);
    // radiation reaction constants (:101-113), PhysConstSI of utils/Constants.H:15-24
    const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, ep0SI = 8.8541878128e-12, reSI = 2.817940326204929e-15;
    k.rr = d.beam_radiation_reaction; k.normalized = d.si_units ? 0 : 1; k.no_z_push = d.beam_no_z_push; k.c_SI = cSI;
    const double q_over_mc = k.normalized ? k.qm/cSI*qeSI/meSI : k.qm/cSI;
    k.RRcoeff = (2.0/3.0)*reSI*q_over_mc*q_over_mc;
    k.wp_inv = (k.normalized && d.background_density_SI > 0.0) ? std::sqrt(ep0SI*meSI/(d.background_density_SI*qeSI*qeSI)) : 1.0;
    k.E0 = k.normalized ? meSI*cSI/k.wp_inv/qeSI : 1.0;
    k.spin = d.beam_spin_tracking; k.spin_anom = d.beam_spin_anom;      // (0 = pure Thomas precession; hosts that want the electron pass 0.00115965218128, as decks.py does)
    return k;
}

int beam_deposit_moving (Engine& E, int p, int cjx, int cjy, int cjz)
{
    if (p < 0 || p >= E.d.nz) return HPS_OK;
    const long bound = E.beam_bound(p);
    if (bound <= 0) return HPS_OK;
    const SlabView f(E.slab);
    const PartConsts k = base_consts(E.gm);
    const double q_invvol = E.d.beam_charge*(E.d.si_units ? 1.0/(E.gm.dx*E.gm.dy*E.gm.dz) : 1.0), csq_inv = 1.0/(E.gm.c*E.gm.c);
    const dim3 grid((unsigned)std::min<long>(ceil_div(bound, 256), 2048)), block(256);
#define CALL(O) hipLaunchKernelGGL(k_beam_deposit_dyn<O>, grid, block, 0, E.st, f, E.bm, E.d_B, E.d_nfront, p, cjx, cjy, cjz, q_invvol, csq_inv, k, E.d_pc_dist)
    HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    return HPS_OK;
}

int beam_moments_reset (Engine& E)
{
    hipLaunchKernelGGL(k_beam_moments_reset, dim3(1), dim3(256), 0, E.st, E.d_mom, E.d.nz);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_push_moving (Engine& E, int islice)
{
    const int p = E.d.nz - 1 - islice;
    const long bound = E.beam_bound(p);
    if (bound > 0) { if (int e = beam_push_slice(E, islice, p, bound)) return e; }
    if (E.d_mom && islice == 0) hipLaunchKernelGGL(k_beam_moments_fold, dim3(1), dim3(64), 0, E.st, E.d_mom, E.d.nz);      // the step's last slice
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_push_slice (Engine& E, int islice, int p, long bound)
{
    const SlabView f(E.slab);
    const BeamPushConsts k = push_consts(E, islice);
    const dim3 grid((unsigned)std::min<long>(ceil_div(bound, 256), 2048)), block(256);
    // the fields of This slice sit at other components of the predictor-corrector's slab (fields/Fields.cpp:128-164)
    const int cP = E.pc ? (int)HPS_PC_PSI : (int)HPS_C_PSI, cE = E.pc ? (int)HPS_PC_EZ : (int)HPS_C_EZ, cX = E.pc ? (int)HPS_PC_BX : (int)HPS_C_BX,
              cY = E.pc ? (int)HPS_PC_BY : (int)HPS_C_BY, cZ = E.pc ? (int)HPS_PC_BZ : (int)HPS_C_BZ;
    if (E.bext.on) {      // beams.external_E / external_B as programs: k_beam_push<ORDER, true> (beam_ext.hip)
        if (int e = beam_push_launch_ext(E, f, p, cP, cE, cX, cY, cZ, k, grid)) return e;
    } else {
#define CALL(O) hipLaunchKernelGGL((k_beam_push<O, false>), grid, block, 0, E.st, f, E.bm, E.d_B, p, cP, cE, cX, cY, cZ, k, BeamExtArgs<false>{})
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    }
    if (E.d_mom)
        hipLaunchKernelGGL(k_beam_partition<true>, dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, E.d_mom + 4*p);
    else
        hipLaunchKernelGGL(k_beam_partition<false>, dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, nullptr);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

} // namespace hps
