// diagnostics.hip -- what a slice writes out beside its fields: the field diagnostic (Fields::Copy, fields/Fields.cpp:413-533),
// the in-situ reductions of fields, plasma and beam (the three InSituComputeDiags of the reference) and the per-component
// checksums.  Owns Engine::fill_field_diagnostic, insitu_plasma, insitu_fields, insitu_beam, checksum_slice and their C ABI.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <cmath>

namespace hps {

// ---- field diagnostics (Fields::Copy, fields/Fields.cpp:413-533) ---------------------------------------------------
// F(i,j,k,n) += rel_z * sum_{iy,ix} sy[iy] sx[ix] slab(i_cell+ix, j_cell+iy, comp n), order-1 shape factors at the
// diagnostic cell centre, slab zero-extended beyond its guard cells (guarded_field_xy, Fields.cpp:331-358)
__global__ __launch_bounds__(256)
void k_diag_copy (SlabView f, int ncomp_slab, const int* __restrict__ comps, int ncd, double* __restrict__ F,
                  int nxc, int nyc, long kplane_off, long comp_stride, double rel_z,
                  double dxc, double dyc, double poff_dx, double poff_dy, double poff_cx, double poff_cy,
                  double dx_inv, double dy_inv)
{
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nxc) return;
    const double x = i*dxc + poff_dx, y = j*dyc + poff_dy;
    const double xmid = (x - poff_cx)*dx_inv, ymid = (y - poff_cy)*dy_inv;
    const int ic = (int)floor(xmid), jc = (int)floor(ymid);
    const double tx = xmid - ic, ty = ymid - jc;
    const double sx[2] = {1.0 - tx, tx}, sy[2] = {1.0 - ty, ty};
    for (int n = 0; n < ncd; ++n) {
        const int m = comps[n];
        double v = 0.0;
        for (int iy = 0; iy < 2; ++iy) for (int ix = 0; ix < 2; ++ix) {
            const int ii = ic + ix, jj = jc + iy;
            const bool in = ii >= -f.ng && ii < f.nx + f.ng && jj >= -f.ng && jj < f.ny + f.ng;
            v += sx[ix]*sy[iy]*(in ? f(ii, jj, m) : 0.0);
        }
        F[n*comp_stride + kplane_off + (long)j*nxc + i] += rel_z*v;
    }
    (void)ncomp_slab;
}

// Fields::InSituComputeDiags (fields/Fields.cpp:1288-1347): ten sums over the valid cells of one slice
__global__ __launch_bounds__(256)
void k_insitu_fields (SlabView f, double clight, double dxdydz, double* out, int nz, int islice)
{
    double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long cells = (long)f.nx*f.ny;
    for (long c = (long)blockIdx.x*blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x*blockDim.x) {
        const int j = (int)(c / f.nx), i = (int)(c - (long)j*f.nx);
        const long o = f.off(i, j);
        const double exmby = f.p[HPS_C_EXMBY*f.ns + o], eypbx = f.p[HPS_C_EYPBX*f.ns + o], ez = f.p[HPS_C_EZ*f.ns + o];
        const double bx = f.p[HPS_C_BX*f.ns + o], by = f.p[HPS_C_BY*f.ns + o], bz = f.p[HPS_C_BZ*f.ns + o];
        const double jzb = f.p[HPS_C_JZB*f.ns + o];
        const double ex = exmby + by*clight, ey = eypbx - bx*clight;
        s[0] += ex*ex; s[1] += ey*ey; s[2] += ez*ez; s[3] += bx*bx; s[4] += by*by; s[5] += bz*bz;
        s[6] += exmby*exmby; s[7] += eypbx*eypbx; s[8] += jzb; s[9] += ez*jzb;
    }
    __shared__ double part[4][10];
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        double v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10)
        atomic_add_f64(out + (long)threadIdx.x*nz + islice,
                       (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x])*dxdydz);
}

// PlasmaParticleContainer::InSituComputeDiags (particles/plasma/PlasmaParticleContainer.cpp:443-530): raw sums
__global__ __launch_bounds__(256)
void k_insitu_plasma (hps_plasma pl, double clight_inv, double radius_sq, double* out, int nz, int islice)
{
    double s[15];
#pragma unroll
    for (int q = 0; q < 15; ++q) s[q] = 0.0;
    for (long ip = (long)blockIdx.x*blockDim.x + threadIdx.x; ip < pl.n; ip += (long)gridDim.x*blockDim.x) {
        const double x = pl.x[ip], y = pl.y[ip];
        if (!(pl.idcpu[ip] & HPS_ID_VALID) || x*x + y*y > radius_sq) continue;
        const double ux = pl.ux[ip]*clight_inv, uy = pl.uy[ip]*clight_inv, psi = pl.psi[ip];
        const double gamma = (1.0 + ux*ux + uy*uy + psi*psi)/(2.0*psi);
        const double uz = gamma - psi;
        const double w = pl.w[ip]*gamma/psi;
        const double energy = pl.w[ip]*(gamma - 1.0);
        s[0] += w; s[1] += w*x; s[2] += w*x*x; s[3] += w*y; s[4] += w*y*y; s[5] += w*ux; s[6] += w*ux*ux;
        s[7] += w*uy; s[8] += w*uy*uy; s[9] += w*uz; s[10] += w*uz*uz; s[11] += w*gamma; s[12] += w*gamma*gamma;
        s[13] += energy; s[14] += 1.0;
    }
    __shared__ double part[4][15];
#pragma unroll
    for (int q = 0; q < 15; ++q) {
        double v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 15)
        atomic_add_f64(out + (long)threadIdx.x*nz + islice,
                       part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// BeamParticleContainer::InSituComputeDiags (particles/beam/BeamParticleContainer.cpp:476-556): raw sums over the
// particles of the slice (slipped-in ones excluded, :494).  Static beam: count_static particles behind b; moving beam:
// the block [B[p] + nfront[p], B[p+1]) of the SoA, nsub < 0 = absorbed.
// MULTI (several beam species): the workgroups of blockIdx.y = s reduce the particles tagged s into species s's
// block of `out` ([species][23][nz]) -- still one launch per slice.
template <bool MULTI>
__global__ __launch_bounds__(256)
void k_insitu_beam (BeamView b, const int* __restrict__ nsub, const long* __restrict__ B, const int* __restrict__ nfront, int p,
                    long count_static, double clight_inv, double radius_sq, double* out, int nz, int islice, int skip_zero_w,
                    const unsigned char* __restrict__ sp)
{
    // skip_zero_w (SALAME deck): a particle whose weight SALAME has set to 0 no longer exists (the reference invalidates it)
    long first = 0, count = count_static;
    if (B) { first = B[p] + nfront[p]; count = B[p + 1] - first; }
    double s[23];
#pragma unroll
    for (int q = 0; q < 23; ++q) s[q] = 0.0;
    for (long t = (long)blockIdx.x*blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x*blockDim.x) {
        const long ip = first + t;
        const double x = b.x[ip], y = b.y[ip], z = b.z[ip];
        if ((nsub && nsub[ip] < 0) || x*x + y*y > radius_sq || (skip_zero_w && b.w[ip] == 0.0)) continue;
        if constexpr (MULTI) { if (sp[ip] != blockIdx.y) continue; }
        const double ux = b.ux[ip]*clight_inv, uy = b.uy[ip]*clight_inv, uz = b.uz[ip]*clight_inv, w = b.w[ip];
        const double uz_inv = uz == 0.0 ? 0.0 : 1.0/uz;
        const double gamma = sqrt(1.0 + ux*ux + uy*uy + uz*uz);
        s[0] += w; s[1] += w*x; s[2] += w*x*x; s[3] += w*y; s[4] += w*y*y; s[5] += w*z; s[6] += w*z*z; s[7] += w*ux; s[8] += w*ux*ux;
        s[9] += w*uy; s[10] += w*uy*uy; s[11] += w*uz; s[12] += w*uz*uz; s[13] += w*x*ux; s[14] += w*y*uy; s[15] += w*z*uz;
        s[16] += w*x*uy; s[17] += w*y*ux; s[18] += w*ux*uz_inv; s[19] += w*uy*uz_inv; s[20] += w*gamma; s[21] += w*gamma*gamma;
        s[22] += 1.0;
    }
    __shared__ double part[4][23];
#pragma unroll
    for (int q = 0; q < 23; ++q) {
        double v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 23) {
        const double v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v != 0.0) atomic_add_f64(out + (MULTI ? (long)blockIdx.y*23*nz : 0L) + (long)threadIdx.x*nz + islice, v);
    }
}

// m_multi_beam.InSituComputeDiags (Hipace.cpp:681): after the field solves, before the beam push
void Engine::insitu_beam (int islice)
{
    if (!d_insitu_bm || nbeam == 0) return;
    const double r2 = insitu_bm_radius*insitu_bm_radius;
    if (moving) {
        const int p = d.nz - 1 - islice;
        const long bound = beam_bound(p);
        if (bound <= 0) return;
        const BeamView b{bm.x, bm.y, bm.z, bm.ux, bm.uy, bm.uz, bm.w};
        const unsigned nwg = (unsigned)std::min<long>(ceil_div(bound, 256), 64);
        if (multi_beam())
            hipLaunchKernelGGL(k_insitu_beam<true>, dim3(nwg, (unsigned)n_beam_species()), dim3(256), 0, st, b, bm.nsub, d_B, d_nfront, p,
                               0L, 1.0/gm.c, r2, d_insitu_bm, d.nz, islice, 0, bm.sp);
        else
            hipLaunchKernelGGL(k_insitu_beam<false>, dim3(nwg), dim3(256), 0, st, b, bm.nsub, d_B, d_nfront, p,
                               0L, 1.0/gm.c, r2, d_insitu_bm, d.nz, islice, 0, (const unsigned char*)nullptr);
    } else {
        const long first0 = beam_off[d.nz - 1 - islice], count = beam_off[d.nz - islice] - first0;
        if (count <= 0) return;
        double* blk = beam_cur + 7*first0;
        const BeamView b{blk, blk + count, blk + 2*count, blk + 3*count, blk + 4*count, blk + 5*count, blk + 6*count};
        hipLaunchKernelGGL(k_insitu_beam<false>, dim3((unsigned)std::min<long>(ceil_div(count, 256), 64)), dim3(256), 0, st, b, (const int*)nullptr,
                           (const long*)nullptr, (const int*)nullptr, 0, count, 1.0/gm.c, r2, d_insitu_bm, d.nz, islice, c_sal >= 0 ? 1 : 0,
                           (const unsigned char*)nullptr);
    }
}

int Engine::fill_field_diagnostic (int islice)
{
    if (fd_comps.empty()) return HPS_OK;
    const int nxc = fd_n[0], nyc = fd_n[1], nzc = fd_n[2];
    const double dzc = fd_h[2], dxc = fd_h[0], dyc = fd_h[1];
    // GetPosOffset (fields/Fields.H:71-77) of the calculation geometry; of the diagnostic one: fd_pos0 (position of its first cell)
    auto poff = [] (double lo, double hi, double h, int n) { return 0.5*(lo + hi - h*(n - 1)); };
    const double poff_cz = poff(d.lo[2], d.hi[2], gm.dz, d.nz), poff_dz = fd_pos0[2];
    const double poff_dx = fd_pos0[0], poff_dy = fd_pos0[1];
    SlabView f(slab);
    const long plane = (long)nxc*nyc, cstride = plane*nzc;
    if (fd_slice_dir == 2) {
        // diag_type xy: one plane that takes every slice inside the diagnostic's z range with the weight dz (Fields.cpp:469-479)
        const double pos_z = islice*gm.dz + poff_cz;
        if (!(fd_lo[2] <= pos_z && pos_z <= fd_hi[2])) return HPS_OK;
        hipLaunchKernelGGL(k_diag_copy, dim3(ceil_div(nxc, 256), nyc), dim3(256), 0, st, f, ncomp, d_fd_comps, (int)fd_comps.size(),
                           d_fd, nxc, nyc, 0L, cstride, gm.dz, dxc, dyc, poff_dx, poff_dy, gm.xoff, gm.yoff, 1.0/gm.dx, 1.0/gm.dy);
        return HPS_OK;
    }
    // which diagnostic planes this slice contributes to (order 1 in z, :428-468)
    const double pos_min = (islice - 1)*gm.dz + poff_cz, pos_max = (islice + 1)*gm.dz + poff_cz;
    const int k_min = (int)std::round((pos_min - poff_dz)*(1.0/dzc)), k_max = (int)std::round((pos_max - poff_dz)*(1.0/dzc));
    for (int k = std::max(k_min, 0); k <= std::min(k_max, nzc - 1); ++k) {
        const double pos = k*dzc + poff_dz;
        const double mid = (pos - poff_cz)*(1.0/gm.dz);
        const int kc = (int)std::floor(mid);
        const double t = mid - kc;
        double rel = 0.0;
        if (kc == islice) rel = 1.0 - t;
        if (kc + 1 == islice) rel = t;
        if (rel == 0.0) continue;
        hipLaunchKernelGGL(k_diag_copy, dim3(ceil_div(nxc, 256), nyc), dim3(256), 0, st, f, ncomp, d_fd_comps, (int)fd_comps.size(),
                           d_fd, nxc, nyc, (long)k*plane, cstride, rel, dxc, dyc, poff_dx, poff_dy, gm.xoff, gm.yoff,
                           1.0/gm.dx, 1.0/gm.dy);
    }
    return HPS_OK;
}

// per-component sum |Q| over the valid cells, accumulated into acc[n]
__global__ __launch_bounds__(256)
void k_checksum (SlabView f, int ncomp, double* acc)
{
    const int n = blockIdx.y;
    double s = 0.0;
    const long cells = (long)f.nx*f.ny;
    for (long c = (long)blockIdx.x*blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x*blockDim.x) {
        const int j = (int)(c / f.nx), i = (int)(c - (long)j*f.nx);
        s += fabs(f(i, j, n));
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomic_add_f64(acc + n, part[0] + part[1] + part[2] + part[3]);
    (void)ncomp;
}

// the reductions the slice schedules launch (engine.hip, predcorr.hip), each a no-op unless switched on
void Engine::checksum_slice ()
{
    if (!diagnostics) return;
    hipLaunchKernelGGL(k_checksum, dim3(64, ncomp), dim3(256), 0, st, SlabView(slab), ncomp, d_checksum);
}
// m_multi_plasma.InSituComputeDiags (Hipace.cpp:590): at the start of the slice
void Engine::insitu_plasma (int islice)
{
    if (!d_insitu_pl) return;
    if (el.pl.n > 0)
        hipLaunchKernelGGL(k_insitu_plasma, dim3(256), dim3(256), 0, st, el.pl, 1.0/gm.c, insitu_pl_radius*insitu_pl_radius, d_insitu_pl, d.nz, islice);
    // the further species, each into its own block
    for (int k = 2; k < n_sp && d_insitu_pl_more; ++k) if (sp[k].pl.n > 0)
        hipLaunchKernelGGL(k_insitu_plasma, dim3(256), dim3(256), 0, st, sp[k].pl, 1.0/gm.c, insitu_pl_radius*insitu_pl_radius,
                           d_insitu_pl_more + (size_t)(k - 2)*15*d.nz, d.nz, islice);
}
// Fields::InSituComputeDiags (Hipace.cpp:686): behind the field solves
void Engine::insitu_fields (int islice)
{
    if (!d_insitu) return;
    hipLaunchKernelGGL(k_insitu_fields, dim3(64), dim3(256), 0, st, SlabView(slab), gm.c, gm.dx*gm.dy*gm.dz, d_insitu, d.nz, islice);
}

} // namespace hps

using namespace hps;

extern "C" int hps_engine_checksums (void* h, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    HPS_HIP_CHECK(hipMemcpy(out, E->d_checksum, E->ncomp*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}
extern "C" int hps_engine_set_insitu_plasma (void* h, double radius)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    (void)hipFree(E->d_insitu_pl); E->d_insitu_pl = nullptr; E->insitu_pl_radius = radius;
    (void)hipFree(E->d_insitu_pl_more); E->d_insitu_pl_more = nullptr;      // (the further species' blocks: the next begin_step)
    if (!(radius > 0.0)) return HPS_OK;
    HPS_HIP_CHECK(hipMalloc(&E->d_insitu_pl, (size_t)15*E->d.nz*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(E->d_insitu_pl, 0, (size_t)15*E->d.nz*sizeof(double)));
    return HPS_OK;
}
extern "C" int hps_engine_set_insitu_beam (void* h, double radius)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    (void)hipFree(E->d_insitu_bm); E->d_insitu_bm = nullptr; E->insitu_bm_radius = radius;
    if (!(radius > 0.0)) return HPS_OK;
    // (room for HPS_MAX_BEAM_SPECIES blocks [23][nz]: species may still be added)
    HPS_HIP_CHECK(hipMalloc(&E->d_insitu_bm, (size_t)23*E->d.nz*HPS_MAX_BEAM_SPECIES*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(E->d_insitu_bm, 0, (size_t)23*E->d.nz*HPS_MAX_BEAM_SPECIES*sizeof(double)));
    return HPS_OK;
}
extern "C" int hps_engine_insitu_beam (void* h, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && !E->multi_beam(), "hps_engine_insitu_beam: the engine holds several beam species: hps_engine_insitu_beam_species returns one of them");
    return hps_engine_insitu_beam_species(h, 0, out);
}
extern "C" int hps_engine_insitu_beam_species (void* h, int species, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->d_insitu_bm && out, "hps_engine_insitu_beam: not switched on");
    HPS_REQUIRE(species >= 0 && species < E->n_beam_species(), "hps_engine_insitu_beam_species: no such beam species");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    const int nz = E->d.nz;
    HPS_HIP_CHECK(hipMemcpy(out, E->d_insitu_bm + (size_t)species*23*nz, (size_t)23*nz*sizeof(double), hipMemcpyDeviceToHost));
    // averages: everything but sum(w) and the count is divided by sum(w) (BeamParticleContainer.cpp:542-548)
    for (int k = 0; k < nz; ++k) {
        const double sw = out[k], inv = sw <= 0.0 ? 0.0 : 1.0/sw;
        for (int q = 1; q <= 21; ++q) out[(size_t)q*nz + k] *= inv;
    }
    return HPS_OK;
}
extern "C" int hps_engine_insitu_plasma (void* h, double* out) { return hps_engine_insitu_plasma_species(h, 0, out); }
extern "C" int hps_engine_insitu_plasma_species (void* h, int k, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && E->d_insitu_pl && out, "hps_engine_insitu_plasma: not switched on");
    HPS_REQUIRE(k == 0 || (k >= 2 && k < E->n_sp), "hps_engine_insitu_plasma_species: species must be 0 (plasma) or the index of an added species");
    HPS_REQUIRE(k == 0 || E->d_insitu_pl_more, "hps_engine_insitu_plasma_species: no step has begun since hps_engine_set_insitu_plasma");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    const int nz = E->d.nz;
    const double* src = k == 0 ? E->d_insitu_pl : E->d_insitu_pl_more + (size_t)(k - 2)*15*nz;
    HPS_HIP_CHECK(hipMemcpy(out, src, (size_t)15*nz*sizeof(double), hipMemcpyDeviceToHost));
    // averages: everything but sum(w), the energy and the count is divided by sum(w) (:511-516)
    for (int k = 0; k < nz; ++k) {
        const double sw = out[k], inv = sw <= 0.0 ? 0.0 : 1.0/sw;
        for (int q = 1; q <= 12; ++q) out[(size_t)q*nz + k] *= inv;
    }
    return HPS_OK;
}
extern "C" int hps_engine_set_insitu_fields (void* h, int on)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    (void)hipFree(E->d_insitu); E->d_insitu = nullptr;
    if (!on) return HPS_OK;
    if (E->pc) { set_error("hps_engine_set_insitu_fields: explicit solver only (needs jz_beam), as the reference"); return HPS_ERR_UNSUPPORTED; }
    HPS_HIP_CHECK(hipMalloc(&E->d_insitu, (size_t)10*E->d.nz*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(E->d_insitu, 0, (size_t)10*E->d.nz*sizeof(double)));
    return HPS_OK;
}
extern "C" int hps_engine_insitu_fields (void* h, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->d_insitu && out, "hps_engine_insitu_fields: not switched on");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    HPS_HIP_CHECK(hipMemcpy(out, E->d_insitu, (size_t)10*E->d.nz*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}
// diagnostic.diag_type (xyz: slice_dir -1, yz: 0, xz: 1, xy: 2), diagnostic.coarsening, diagnostic.patch_lo / patch_hi:
// the box of Diagnostic::ResizeFDiagFAB (diagnostics/Diagnostic.cpp:300-390) and TrimIOBox (:393-410)
extern "C" int hps_engine_set_field_diagnostic_box (void* h, int ncomps, const int* comps, const int coarsening[3], int slice_dir,
                                                    const double* patch_lo, const double* patch_hi)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    (void)hipFree(E->d_fd); (void)hipFree(E->d_fd_comps); E->d_fd = nullptr; E->d_fd_comps = nullptr; E->fd_comps.clear();
    if (ncomps <= 0) return HPS_OK;
    HPS_REQUIRE(comps && coarsening, "hps_engine_set_field_diagnostic: null argument");
    HPS_REQUIRE(slice_dir >= -1 && slice_dir <= 2, "hps_engine_set_field_diagnostic: slice_dir must be -1 (xyz), 0 (yz), 1 (xz) or 2 (xy)");
    for (int k = 0; k < ncomps; ++k) HPS_REQUIRE(comps[k] >= 0 && comps[k] < E->ncomp, "hps_engine_set_field_diagnostic: bad component");
    const int n3[3] = {E->d.nx, E->d.ny, E->d.nz};
    const double h3[3] = {E->gm.dx, E->gm.dy, E->gm.dz};
    auto floor_div = [] (int a, int b) { return a >= 0 ? a/b : -((-a + b - 1)/b); };
    for (int q = 0; q < 3; ++q) {
        const int c = (q == slice_dir) ? 1 : coarsening[q];               // (the slice direction is never coarsened, Diagnostic.cpp:71-73)
        HPS_REQUIRE(c >= 1, "hps_engine_set_field_diagnostic: coarsening must be >= 1");
        if (!patch_lo && !patch_hi && q != slice_dir)
            HPS_REQUIRE(n3[q] % c == 0, "hps_engine_set_field_diagnostic: sizes must be divisible by the coarsening");
        E->fd_c[q] = c;
        const double plo = E->d.lo[q], phi = E->d.hi[q], hh = h3[q];
        const double poff_sim = 0.5*(plo + phi - hh*(n3[q] - 1));
        int small = 0, big = n3[q] - 1;
        if (patch_lo) small = std::max(small, (int)std::round((patch_lo[q] - poff_sim)/hh));
        if (patch_hi) big = std::min(big, (int)std::round((patch_hi[q] - poff_sim)/hh));
        HPS_REQUIRE(big >= small, "hps_engine_set_field_diagnostic: the patch does not meet the box");
        double lo_d = plo + small*hh, hi_d = phi + (big - (n3[q] - 1))*hh;
        if (q == slice_dir) {
            const double half = (hi_d - lo_d)/(2.0*(big - small + 1)), mid = 0.5*(lo_d + hi_d);
            small = big = 0;
            if (q < 2) { lo_d = mid - half; hi_d = mid + half; }
        }
        const int sc = floor_div(small, c), bc = floor_div(big, c);
        E->fd_n[q] = bc - sc + 1;
        E->fd_h[q] = (hi_d - lo_d)/E->fd_n[q];
        E->fd_pos0[q] = 0.5*(lo_d + hi_d - E->fd_h[q]*(sc + bc)) + sc*E->fd_h[q];
        E->fd_lo[q] = lo_d; E->fd_hi[q] = hi_d;
    }
    E->fd_slice_dir = slice_dir;
    E->fd_comps.assign(comps, comps + ncomps);
    const size_t cells = E->fd_cells();
    HPS_HIP_CHECK(hipMalloc(&E->d_fd, ncomps*cells*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(E->d_fd, 0, ncomps*cells*sizeof(double)));
    HPS_HIP_CHECK(hipMalloc(&E->d_fd_comps, ncomps*sizeof(int)));
    HPS_HIP_CHECK(hipMemcpy(E->d_fd_comps, comps, ncomps*sizeof(int), hipMemcpyHostToDevice));
    return HPS_OK;
}
extern "C" int hps_engine_set_field_diagnostic (void* h, int ncomps, const int* comps, const int coarsening[3])
{
    return hps_engine_set_field_diagnostic_box(h, ncomps, comps, coarsening, -1, nullptr, nullptr);
}
extern "C" int hps_engine_field_diagnostic_geometry (void* h, int* n3, double* lo3, double* hi3)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->d_fd, "hps_engine_field_diagnostic_geometry: no diagnostic set");
    for (int q = 0; q < 3; ++q) { if (n3) n3[q] = E->fd_n[q]; if (lo3) lo3[q] = E->fd_lo[q]; if (hi3) hi3[q] = E->fd_hi[q]; }
    return HPS_OK;
}
extern "C" int hps_engine_field_diagnostic (void* h, double* out)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->d_fd && out, "hps_engine_field_diagnostic: no diagnostic set");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    HPS_HIP_CHECK(hipMemcpy(out, E->d_fd, E->fd_comps.size()*E->fd_cells()*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}
extern "C" int hps_engine_set_diagnostics (void* h, int on) { static_cast<Engine*>(h)->diagnostics = (on != 0); return HPS_OK; }
