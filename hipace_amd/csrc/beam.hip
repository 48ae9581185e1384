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
#include <cmath>

namespace hps {

// MULTI (several beam species): the charge per cell volume is the lane's species'
// SEL (SALAME's step 0 in a moving-beam engine): only the species whose bit is set in multi.mask deposit -- a do_salame
// species leaves jx, jy of Next alone, the SALAME slice's jz_beam takes the do_salame species only (MultiBeam.cpp:42-59)
template <int ORDER, bool MULTI, bool SEL = false>
__global__ __launch_bounds__(256)
void k_beam_deposit_dyn (SlabView f, BeamSoA b, const long* __restrict__ B, const int* __restrict__ nfront, int p,
                         int cjx, int cjy, int cjz, double q_invvol, double clightsq_inv, PartConsts k, int* disturbed,
                         BeamMultiArgs<MULTI> multi)
{
    static_assert(MULTI || !SEL, "a species selection needs the tag row");
    const long first = B[p] + nfront[p], count = B[p + 1] - first;
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
    const long ip = first + t;
    if (b.nsub[ip] < 0) continue;               // absorbed at the boundary
    if constexpr (SEL) { if (!(multi.mask >> b.sp[ip] & 1u)) continue; }
    const double ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
    const double gaminv = 1.0/sqrt(1.0 + ux*ux*clightsq_inv + uy*uy*clightsq_inv + uz*uz*clightsq_inv);
    if constexpr (MULTI) q_invvol = multi.tab[b.sp[ip]].q_invvol;
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
// MULTI (several beam species): the tag row moves with the others, and the moments are reduced per species into
// mom[species][0..3] -- every lane adds a particle's terms to its own species' sums and exact zeros to the others', so lane order,
// butterfly and wave order are those of the one-species reduction over that species' particles alone.
template <bool MOM, bool MULTI>
__global__ __launch_bounds__(1024)
void k_beam_partition (BeamSoA b, BeamSoA scr, long* B, int* nfront, int p, double min_z, double inv_c, double* mom, BeamMultiArgs<MULTI> multi)
{
    int ns = 1;
    if constexpr (MULTI) ns = multi.ns;
    constexpr int NS = MULTI ? HPS_MAX_BEAM_SPECIES : 1;
    __shared__ int s_cnt[2];
    __shared__ int s_red[16];
    __shared__ double s_mom[MOM ? 16 : 1][NS][4];
    const long first = B[p], count = B[p + 1] - first;
    const int t = threadIdx.x;
    int mine = 0;
    double m0[NS], m1[NS], m2[NS], m3[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { m0[s] = 0.0; m1[s] = 0.0; m2[s] = 0.0; m3[s] = __builtin_huge_val(); }
    for (long q = t; q < count; q += 1024) {
        const double z = b.z[first + q];
        mine += (z < min_z) ? 1 : 0;
        if (MOM && z >= min_z && b.nsub[first + q] >= 0) {
            const double w = b.w[first + q], u = b.uz[first + q]*inv_c;
            if constexpr (MULTI) {
                const int tag = b.sp[first + q];
#pragma unroll
                for (int s = 0; s < NS; ++s) {      // (static indices: the sums stay in registers)
                    const bool own = tag == s;
                    const double ws = own ? w : 0.0;      // (the same products and sums as below, on an exact zero elsewhere)
                    m0[s] += ws; m1[s] += ws*u; m2[s] += ws*u*u; m3[s] = own ? fmin(m3[s], u) : m3[s];
                }
            } else { m0[0] += w; m1[0] += w*u; m2[0] += w*u*u; m3[0] = fmin(m3[0], u); }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (MOM) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            for (int o = 32; o > 0; o >>= 1) {
                m0[s] += __shfl_xor(m0[s], o); m1[s] += __shfl_xor(m1[s], o); m2[s] += __shfl_xor(m2[s], o); m3[s] = fmin(m3[s], __shfl_xor(m3[s], o));
            }
            if ((t & 63) == 0) { s_mom[t >> 6][s][0] = m0[s]; s_mom[t >> 6][s][1] = m1[s]; s_mom[t >> 6][s][2] = m2[s]; s_mom[t >> 6][s][3] = m3[s]; }
        }
    }
    if ((t & 63) == 0) s_red[t >> 6] = mine;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    if (MOM && t < ns) {      // lane s folds species s
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = __builtin_huge_val();
        for (int w = 0; w < 16; ++w) { a0 += s_mom[w][t][0]; a1 += s_mom[w][t][1]; a2 += s_mom[w][t][2]; a3 = fmin(a3, s_mom[w][t][3]); }
        mom[4*t] = a0; mom[4*t + 1] = a1; mom[4*t + 2] = a2; mom[4*t + 3] = a3;
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
        if constexpr (MULTI) scr.sp[dst] = b.sp[ip];
    }
    __threadfence_block();
    __syncthreads();
    for (long q = t; q < count; q += 1024) {
        const long ip = first + q;
        b.x[ip] = scr.x[q]; b.y[ip] = scr.y[q]; b.z[ip] = scr.z[q]; b.ux[ip] = scr.ux[q];
        b.uy[ip] = scr.uy[q]; b.uz[ip] = scr.uz[q]; b.w[ip] = scr.w[q]; b.nsub[ip] = scr.nsub[q];
        if (b.sx) { b.sx[ip] = scr.sx[q]; b.sy[ip] = scr.sy[q]; b.sz[ip] = scr.sz[q]; }
        if constexpr (MULTI) b.sp[ip] = scr.sp[q];
    }
    if (t == 0) { B[p + 1] = first + count - nslip; nfront[p + 1] = nslip; }
}

// mom[nz + 1][ns][4]: one slot per slice (head first) and species, and the step's totals behind them; an empty slice keeps
// {0, 0, 0, +inf}
__global__ void k_beam_moments_reset (double* mom, int nz, int ns)
{
    for (int i = threadIdx.x; i < 4*ns*(nz + 1); i += blockDim.x) mom[i] = (i & 3) == 3 ? __builtin_huge_val() : 0.0;
}
// the step's totals: the nz slots folded head to tail, one lane per species and moment (a fixed order: no atomics on doubles)
__global__ void k_beam_moments_fold (double* mom, int nz, int ns)
{
    const int k = threadIdx.x;
    if (k >= 4*ns) return;
    double a = mom[k];
    for (int p = 1; p < nz; ++p) a = ((k & 3) == 3) ? fmin(a, mom[4*ns*p + k]) : a + mom[4*ns*p + k];
    mom[4*ns*nz + k] = a;
}

// ---- ring hand-off (MultiBuffer::put_data / get_data, utils/MultiBuffer.cpp:444-609) ----------------------------
// message = [count | x[cap] y[cap] z[cap] ux[cap] uy[cap] uz[cap] w[cap]]; everything stays on the device
// MULTI (several beam species): one more row behind the others carries the tag (as a double: 0 .. 3 are exact)
template <bool MULTI>
__global__ __launch_bounds__(256)
void k_beam_export (BeamSoA b, const long* __restrict__ B, int p, double* __restrict__ msg, long cap, int* overflow)
{
    const long first = B[p], count = B[p + 1] - first;
    if (blockIdx.x == 0 && threadIdx.x == 0) { msg[0] = (double)min(count, cap); if (count > cap) atomicAdd(overflow, 1); }
    const double* a[10] = {b.x, b.y, b.z, b.ux, b.uy, b.uz, b.w, b.sx, b.sy, b.sz};
    const int rows = b.sx ? 10 : 7;
    for (long q = (long)blockIdx.x*blockDim.x + threadIdx.x; q < min(count, cap); q += (long)gridDim.x*blockDim.x)
    {
        for (int k = 0; k < rows; ++k) msg[1 + k*cap + q] = a[k][first + q];
        if constexpr (MULTI) msg[1 + rows*cap + q] = (double)b.sp[first + q];
    }
}

// block p of the coming step: placed behind the blocks imported so far (imp[p] = where it starts); every later
// boundary moves with it, so the slices not imported yet are empty ranges
template <bool MULTI>
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
        if constexpr (MULTI) b.sp[start + q] = (unsigned char)msg[1 + rows*cap + q];
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
    const dim3 grid((unsigned)std::max<long>(1, std::min<long>(ceil_div(cap, 256), 256)));
    if (E.multi_beam()) hipLaunchKernelGGL(k_beam_export<true>, grid, dim3(256), 0, E.st, E.bm, E.d_B, p, msg_dev, cap, E.d_beam_overflow);
    else hipLaunchKernelGGL(k_beam_export<false>, grid, dim3(256), 0, E.st, E.bm, E.d_B, p, msg_dev, cap, E.d_beam_overflow);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_import_slice (Engine& E, int islice, const double* msg_dev, long cap)
{
    const int p = E.d.nz - 1 - islice;
    const long capacity = std::max(E.nbeam, 1L);
    const dim3 grid((unsigned)std::max<long>(1, std::min<long>(ceil_div(cap, 256), 256)));
    if (E.multi_beam()) hipLaunchKernelGGL(k_beam_import<true>, grid, dim3(256), 0, E.st, E.bm, E.d_B, E.d_Bimp, p, E.d.nz, msg_dev, cap, capacity, E.d_beam_overflow);
    else hipLaunchKernelGGL(k_beam_import<false>, grid, dim3(256), 0, E.st, E.bm, E.d_B, E.d_Bimp, p, E.d.nz, msg_dev, cap, capacity, E.d_beam_overflow);
    hipLaunchKernelGGL(k_beam_import_bounds, dim3(1), dim3(256), 0, E.st, E.d_B, E.d_Bimp, p, E.d.nz, msg_dev, cap, capacity);
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// what the push and the deposit take per species (BeamParticleAdvance.cpp:101-113; BeamDepositCurrent.cpp:70-83), from the
// species' deck values: the one place both the launch constants of a one-species engine and the species table come from
static BeamSpeciesRec species_rec (const Engine& E, double charge, double mass, int n_subcycles, int no_z_push, int rr, double spin_anom)
{
    const hps_deck& d = E.d;
    BeamSpeciesRec r{};
    r.nsc = n_subcycles > 0 ? n_subcycles : 10;
    r.dt = E.step_dt/r.nsc;
    r.qm = charge/(mass != 0.0 ? mass : 1.0);
    r.q_invvol = charge*(d.si_units ? 1.0/(E.gm.dx*E.gm.dy*E.gm.dz) : 1.0);
    // radiation reaction constants (:101-113), PhysConstSI of utils/Constants.H:15-24
    const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, reSI = 2.817940326204929e-15;
    const double q_over_mc = d.si_units ? r.qm/cSI : r.qm/cSI*qeSI/meSI;
    r.RRcoeff = (2.0/3.0)*reSI*q_over_mc*q_over_mc;
    r.rr = rr; r.no_z_push = no_z_push; r.spin_anom = spin_anom;
    return r;
}

static BeamPushConsts push_consts (const Engine& E, int islice)
{
    BeamPushConsts k{};
    const hps_deck& d = E.d;
    const BeamSpeciesRec r = species_rec(E, d.beam_charge, d.beam_mass, d.beam_n_subcycles, d.beam_no_z_push, d.beam_radiation_reaction,
                                         d.beam_spin_anom);      // (0 = pure Thomas precession; hosts that want the electron pass 0.00115965218128, as decks.py does)
    k.nsc = r.nsc; k.dt = r.dt; k.qm = r.qm; k.rr = r.rr; k.no_z_push = r.no_z_push; k.RRcoeff = r.RRcoeff; k.spin_anom = r.spin_anom;
    k.c = E.gm.c; k.inv_c2 = 1.0/(E.gm.c*E.gm.c);
    k.min_z = d.lo[2] + islice*E.gm.dz;
    k.ex_slope = d.ext_E_slope[0]; k.ey_slope = d.ext_E_slope[1]; k.ez_slope = d.ext_Ez_slope;
    k.pc = base_consts(E.gm);
    const double cSI = 299792458.0, qeSI = 1.602176634e-19, meSI = 9.1093837015e-31, ep0SI = 8.8541878128e-12;
    k.normalized = d.si_units ? 0 : 1; k.c_SI = cSI;
    k.wp_inv = (k.normalized && d.background_density_SI > 0.0) ? std::sqrt(ep0SI*meSI/(d.background_density_SI*qeSI*qeSI)) : 1.0;
    k.E0 = k.normalized ? meSI*cSI/k.wp_inv/qeSI : 1.0;
    k.spin = d.beam_spin_tracking;
    return k;
}

// the species table of the step that has begun (the sub-cycle's dt is the step's dt over the species' count): the records
// travel as a kernel argument, so the host copy may change before the launch has run
__global__ void k_beam_species_table (BeamSpeciesTable t, BeamSpeciesRec* dst, int ns)
{
    if ((int)threadIdx.x < ns) dst[threadIdx.x] = t.r[threadIdx.x];
}

int beam_species_table_upload (Engine& E)
{
    if (!E.multi_beam()) return HPS_OK;
    BeamSpeciesTable t{};
    for (int k = 0; k < E.n_beam_species(); ++k) {
        const hps_beam_species& s = E.bsp[(size_t)k].s;
        t.r[k] = species_rec(E, s.charge, s.mass, s.n_subcycles, s.no_z_push, s.radiation_reaction, s.spin_anom);
    }
    hipLaunchKernelGGL(k_beam_species_table, dim3(1), dim3(64), 0, E.st, t, E.d_bsp_tab, E.n_beam_species());
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
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
    if (E.multi_beam()) {
        const BeamMultiArgs<true> m{E.d_bsp_tab, E.n_beam_species()};
#define CALL(O) hipLaunchKernelGGL((k_beam_deposit_dyn<O, true>), grid, block, 0, E.st, f, E.bm, E.d_B, E.d_nfront, p, cjx, cjy, cjz, q_invvol, csq_inv, k, E.d_pc_dist, m)
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    } else {
#define CALL(O) hipLaunchKernelGGL((k_beam_deposit_dyn<O, false>), grid, block, 0, E.st, f, E.bm, E.d_B, E.d_nfront, p, cjx, cjy, cjz, q_invvol, csq_inv, k, E.d_pc_dist, BeamMultiArgs<false>{})
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    }
    E.beam_launched |= 1UL << (16 + 2*std::min(std::max(E.d.order, 0), 3) + (E.multi_beam() ? 1 : 0));
    return HPS_OK;
}

// the same deposit restricted to the species in mask: launched by step 0 of a SALAME engine only (solve_slice_begin's jx, jy of
// Next without the do_salame species; Engine::salame_module's jz of the do_salame species alone)
int beam_deposit_species (Engine& E, int p, unsigned mask, int cjx, int cjy, int cjz)
{
    if (p < 0 || p >= E.d.nz || !E.multi_beam() || (mask & E.species_mask_all()) == 0) return HPS_OK;
    const long bound = E.beam_bound(p);
    if (bound <= 0) return HPS_OK;
    const SlabView f(E.slab);
    const PartConsts k = base_consts(E.gm);
    const double csq_inv = 1.0/(E.gm.c*E.gm.c);
    const dim3 grid((unsigned)std::min<long>(ceil_div(bound, 256), 2048)), block(256);
    const BeamMultiArgs<true> m{E.d_bsp_tab, E.n_beam_species(), mask};
#define CALL(O) hipLaunchKernelGGL((k_beam_deposit_dyn<O, true, true>), grid, block, 0, E.st, f, E.bm, E.d_B, E.d_nfront, p, cjx, cjy, cjz, 0.0, csq_inv, k, E.d_pc_dist, m)
    HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    E.beam_launched |= 1UL << (28 + std::min(std::max(E.d.order, 0), 3));
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_moments_reset (Engine& E)
{
    hipLaunchKernelGGL(k_beam_moments_reset, dim3(1), dim3(256), 0, E.st, E.d_mom, E.d.nz, E.n_beam_species());
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_push_moving (Engine& E, int islice)
{
    const int p = E.d.nz - 1 - islice;
    const long bound = E.beam_bound(p);
    if (bound > 0) { if (int e = beam_push_slice(E, islice, p, bound)) return e; }
    if (E.d_mom && islice == 0) hipLaunchKernelGGL(k_beam_moments_fold, dim3(1), dim3(64), 0, E.st, E.d_mom, E.d.nz, E.n_beam_species());      // the step's last slice
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

int beam_push_slice (Engine& E, int islice, int p, long bound)
{
    const SlabView f(E.slab);
    const BeamPushConsts k = push_consts(E, islice);
    const dim3 grid((unsigned)std::min<long>(ceil_div(bound, 256), 2048)), block(256);
    const bool multi = E.multi_beam();
    const int ns = E.n_beam_species();
    // the fields of This slice sit at other components of the predictor-corrector's slab (fields/Fields.cpp:128-164)
    const int cP = E.pc ? (int)HPS_PC_PSI : (int)HPS_C_PSI, cE = E.pc ? (int)HPS_PC_EZ : (int)HPS_C_EZ, cX = E.pc ? (int)HPS_PC_BX : (int)HPS_C_BX,
              cY = E.pc ? (int)HPS_PC_BY : (int)HPS_C_BY, cZ = E.pc ? (int)HPS_PC_BZ : (int)HPS_C_BZ;
    if (E.bext.on) {      // beams.external_E / external_B as programs: k_beam_push<ORDER, true, MULTI> (beam_ext.hip)
        if (int e = beam_push_launch_ext(E, f, p, cP, cE, cX, cY, cZ, k, grid)) return e;
    } else if (multi) {
        const BeamMultiArgs<true> m{E.d_bsp_tab, ns};
#define CALL(O) hipLaunchKernelGGL((k_beam_push<O, false, true>), grid, block, 0, E.st, f, E.bm, E.d_B, p, cP, cE, cX, cY, cZ, k, BeamExtArgs<false>{}, m)
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    } else {
#define CALL(O) hipLaunchKernelGGL((k_beam_push<O, false, false>), grid, block, 0, E.st, f, E.bm, E.d_B, p, cP, cE, cX, cY, cZ, k, BeamExtArgs<false>{}, BeamMultiArgs<false>{})
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    }
    if (!E.bext.on) E.beam_launched |= beam_push_bit(std::min(std::max(E.d.order, 0), 3), false, multi);
    double* mom = E.d_mom ? E.d_mom + (size_t)4*ns*p : nullptr;
    const BeamMultiArgs<true> mt{E.d_bsp_tab, ns};
    if (E.d_mom && multi)
        hipLaunchKernelGGL((k_beam_partition<true, true>), dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, mom, mt);
    else if (E.d_mom)
        hipLaunchKernelGGL((k_beam_partition<true, false>), dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, mom, BeamMultiArgs<false>{});
    else if (multi)
        hipLaunchKernelGGL((k_beam_partition<false, true>), dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, mom, mt);
    else
        hipLaunchKernelGGL((k_beam_partition<false, false>), dim3(1), dim3(1024), 0, E.st, E.bm, E.bm_scr, E.d_B, E.d_nfront, p, k.min_z, 1.0/k.c, mom, BeamMultiArgs<false>{});
    E.beam_launched |= 1UL << (24 + 2*(E.d_mom ? 1 : 0) + (multi ? 1 : 0));
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

std::string beam_kernel_names (const Engine& E)
{
    std::string out;
    char b[64];
    for (int q = 0; q < 16; ++q)
        if (E.beam_launched >> q & 1UL) { std::snprintf(b, sizeof b, "k_beam_push<%d,%d,%d>\n", q >> 2, q >> 1 & 1, q & 1); out += b; }
    for (int q = 0; q < 8; ++q)
        if (E.beam_launched >> (16 + q) & 1UL) { std::snprintf(b, sizeof b, "k_beam_deposit_dyn<%d,%d>\n", q >> 1, q & 1); out += b; }
    for (int q = 0; q < 4; ++q)
        if (E.beam_launched >> (24 + q) & 1UL) { std::snprintf(b, sizeof b, "k_beam_partition<%d,%d>\n", q >> 1, q & 1); out += b; }
    for (int q = 0; q < 4; ++q)      // (the species-masked deposit of SALAME's step 0: ORDER, MULTI, SEL)
        if (E.beam_launched >> (28 + q) & 1UL) { std::snprintf(b, sizeof b, "k_beam_deposit_dyn<%d,1,1>\n", q); out += b; }
    return out;
}

// ---- several beam species: the species list, the tag row, the merge of a new species into the container ----------

// One workgroup per slice p and source (blockIdx.y = 0: what the container held, 1: the new species): its seven rows and its tags
// go to the merged slice-major blocks, the old particles in front, in their order, the new ones behind, in theirs.  Every
// destination has one writer: no atomics.  tag_a null: the container held species 0 only.
__global__ __launch_bounds__(256)
void k_beam_merge (const double* __restrict__ blk_a, const long* __restrict__ off_a, const unsigned char* __restrict__ tag_a,
                   const double* __restrict__ blk_b, const long* __restrict__ off_b, int tag_b,
                   double* __restrict__ blk_m, unsigned char* __restrict__ tag_m)
{
    const int p = blockIdx.x, src = blockIdx.y;
    const long fa = off_a[p], ca = off_a[p + 1] - fa, fb = off_b[p], cb = off_b[p + 1] - fb;
    const long fm = fa + fb, cm = ca + cb;                       // the merged slice
    const double* from = src ? blk_b + 7*fb : blk_a + 7*fa;
    const long cnt = src ? cb : ca, shift = src ? ca : 0;
    double* to = blk_m + 7*fm + shift;
    for (int k = 0; k < 7; ++k)
        for (long i = threadIdx.x; i < cnt; i += blockDim.x) to[k*cm + i] = from[k*cnt + i];
    for (long i = threadIdx.x; i < cnt; i += blockDim.x)
        tag_m[fm + shift + i] = (unsigned char)(src ? tag_b : (tag_a ? tag_a[fa + i] : 0));
}

int Engine::alloc_beam_tags ()
{
    if (!moving) return HPS_OK;
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    (void)hipFree(bm_sp); (void)hipFree(bm_sp_scr); bm_sp = bm_sp_scr = nullptr;
    const size_t nb = (size_t)std::max(nbeam, 1L);
    HPS_HIP_CHECK(hipMalloc(&bm_sp, nb)); HPS_HIP_CHECK(hipMalloc(&bm_sp_scr, nb));
    if (beam_tag && nbeam > 0) HPS_HIP_CHECK(hipMemcpy(bm_sp, beam_tag, (size_t)nbeam, hipMemcpyDeviceToDevice));
    else HPS_HIP_CHECK(hipMemset(bm_sp, 0, nb));
    HPS_HIP_CHECK(hipMemset(bm_sp_scr, 0, nb));
    bm.sp = bm_sp; bm_scr.sp = bm_sp_scr;
    if (!d_bsp_tab) HPS_HIP_CHECK(hipMalloc(&d_bsp_tab, sizeof(BeamSpeciesTable)));
    return HPS_OK;
}

int Engine::add_beam_species (const hps_beam_species* s, int* index_out)
{
    static const std::string fn = "hps_engine_add_beam_species: ";
    HPS_REQUIRE(s, fn + "null argument");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, fn + "call before the first hps_engine_begin_step");
    HPS_REQUIRE(n_beam_species() < HPS_MAX_BEAM_SPECIES, fn + "an engine holds at most HPS_MAX_BEAM_SPECIES = 4 beam species");
    HPS_REQUIRE(std::isfinite(s->charge) && std::isfinite(s->mass) && s->mass >= 0.0 && std::isfinite(s->spin_anom), fn + "charge, mass and spin_anom must be finite, the mass not negative");
#define HPS_REFUSE(cond, msg) do { if (cond) { set_error(fn + msg); return HPS_ERR_UNSUPPORTED; } } while (0)
    HPS_REFUSE(d.beam_do_salame, "several beam species with beam_do_salame are not supported (SALAME acts on the one beam of a static-beam engine)");
    HPS_REQUIRE(!(s->do_salame && !species_salame), fn + "a do_salame species needs beam_species_salame (hps_engine_set_beam_species_salame, right behind hps_engine_create: it allocates the SALAME slice)");
    HPS_REFUSE(!(d.dt != 0.0 || d.dt_adaptive), "several beam species need a moving beam (hipace.dt != 0 or adaptive): a static beam (dt = 0) has no species tag");
    for (const Collision& c : coll)
        HPS_REFUSE(c.beam, "several beam species with a beam-plasma collision (hps_engine_add_beam_collision) are not supported: the collision takes one beam's charge and mass");
    HPS_REFUSE((s->do_spin_tracking != 0) != (d.beam_spin_tracking != 0), "the beam species differ in do_spin_tracking: the container has the spin rows for all of its particles or for none");
    HPS_REFUSE(s->radiation_reaction && !d.si_units && !(d.background_density_SI > 0.0), "radiation_reaction in normalised units needs background_density_SI (BeamParticleAdvance.cpp:39-43)");
#undef HPS_REFUSE
    if (bsp.empty()) {      // species 0: the deck's beam, as the container holds it
        BeamSpecies b0;
        b0.s = hps_beam_species{d.beam_charge, d.beam_mass, d.beam_n_subcycles, d.beam_no_z_push, d.beam_radiation_reaction, d.beam_spin_tracking,
                                d.beam_spin_anom, d.beam_umean[2], d.beam_uz_std, 0};      // (species 0 is never the SALAME beam of a moving engine)
        b0.count = nbeam; b0.filled = nbeam > 0;
        bsp.push_back(b0);
    }
    BeamSpecies b; b.s = *s;
    bsp.push_back(b);
    auto undo = [&] (int e) { bsp.pop_back(); if (bsp.size() == 1) bsp.clear();
                              if (!multi_beam()) { (void)hipFree(bm_sp); (void)hipFree(bm_sp_scr); bm_sp = bm_sp_scr = nullptr; bm.sp = bm_scr.sp = nullptr; }
                              return e; };
    if (int e = alloc_beam_tags()) return undo(e);
    if (d_mom) { if (int e = beam_moments_reset(*this)) return undo(e); }
    if (index_out) *index_out = (int)bsp.size() - 1;
    return HPS_OK;
}

// what the container holds is set aside (its blocks and tags keep their storage; everything else is rebuilt), and the deck's
// charge and mass become the selected species' for the setter that follows
int Engine::stash_beam_for_merge (const char* fn, BeamStash& A)
{
    const std::string f = std::string(fn) + ": ";
    HPS_REQUIRE(sel_species > 0 && sel_species < (int)bsp.size(), f + "no such beam species");
    HPS_REQUIRE(!bsp[(size_t)sel_species].filled, f + "this beam species already holds particles (a species is filled once)");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, f + "call before the first hps_engine_begin_step");
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    A.blocks = beam_init; A.tag = beam_tag; A.off = beam_off; A.n = nbeam; A.host_beam = host_beam;
    A.charge = d.beam_charge; A.mass = d.beam_mass;
    if ((long)A.off.size() != d.nz + 1) A.off.assign((size_t)d.nz + 1, 0);
    beam_init = nullptr; beam_tag = nullptr;
    d.beam_charge = bsp[(size_t)sel_species].s.charge; d.beam_mass = bsp[(size_t)sel_species].s.mass;
    return HPS_OK;
}

// behind the setter (e_setter: what it returned; the container now holds the new species alone): merge, and install the merged
// blocks through the one install tail.  A setter that failed, or a failure here, leaves the container as it was before.
int Engine::merge_stashed_beam (BeamStash& A, int e_setter)
{
    const int k = sel_species;
    d.beam_charge = A.charge; d.beam_mass = A.mass;
    const double box[4] = {0.0, 0.0, 0.0, 0.0};      // (a moving beam's support is the whole plane: install_moving_beam)
    auto restore = [&] (int e) {
        const std::string msg = hps_last_error();
        (void)hipStreamSynchronize(st);
        release_beam();
        beam_off = A.off; beam_tag = A.tag; host_beam = A.host_beam;
        (void)install_beam_device(A.blocks, A.n, box);
        set_error(msg);
        return e;
    };
    if (e_setter) return restore(e_setter);
    const long nb = nbeam, nm = A.n + nb;
    const int nz = d.nz;
    std::vector<long> off_m((size_t)nz + 1);
    for (int p = 0; p <= nz; ++p) off_m[(size_t)p] = A.off[(size_t)p] + beam_off[(size_t)p];
    DevBuf<long> d_off; DevBuf<double> blk_m; DevBuf<unsigned char> tag_m;
    if (d_off.alloc((size_t)2*(nz + 1)) || blk_m.alloc((size_t)7*std::max(nm, 1L)) || tag_m.alloc((size_t)std::max(nm, 1L))) return restore(HPS_ERR_HIP);
    if (hipMemcpyAsync(d_off.get(), A.off.data(), (size_t)(nz + 1)*sizeof(long), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_off.get() + nz + 1, beam_off.data(), (size_t)(nz + 1)*sizeof(long), hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("hps_engine: beam merge: copy of the slice offsets failed"); return restore(HPS_ERR_HIP); }
    if (nm > 0) {
        hipLaunchKernelGGL(k_beam_merge, dim3(nz, 2), dim3(256), 0, st, A.blocks, d_off.get(), A.tag, beam_init, d_off.get() + nz + 1, k,
                           blk_m.get(), tag_m.get());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { set_error("hps_engine: k_beam_merge failed"); return restore(HPS_ERR_HIP); }
    } else (void)hipStreamSynchronize(st);
    release_beam();                                  // the new species' own container
    (void)hipFree(A.blocks); (void)hipFree(A.tag); A.blocks = nullptr; A.tag = nullptr;
    bsp[(size_t)k].off = beam_off;                   // the species' own slices: what it holds of each when step 0 begins
    beam_off = off_m; host_beam = true;
    beam_tag = tag_m.release();
    bsp[(size_t)k].count = nb; bsp[(size_t)k].filled = true;
    double* merged = blk_m.release();
    if (nm == 0) { (void)hipFree(merged); merged = nullptr; }
    return install_beam_device(merged, nm, box);
}

} // namespace hps
