// beam_host.hip -- the beam as the engine holds it between steps: the deck's fixed-ppc beam generated on the host
// (InitBeamFixedPPCSlice, beam/BeamParticleContainerInit.cpp:198-346), a beam the host hands over, the install tail shared with
// the device generators (beam_init.hip), and the static beam's slice deposit (BeamDepositCurrent.cpp:21-195).  Owns
// Engine::init_beam, set_beam_particles, install_*, release_beam, set_beam_box, deposit_beam_slice and the beam's C ABI.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace hps {

// beam slice deposit (particles/deposition/BeamDepositCurrent.cpp:21-195), depos_order_z = 0
template <int ORDER>
__global__ __launch_bounds__(256)
void k_beam_deposit (SlabView f, BeamView b, long first, long count, int cjx, int cjy, int cjz,
                     double q_invvol, double clightsq_inv, double dx_inv, double dy_inv, double xoff, double yoff, const int* go,
                     int* disturbed = nullptr)
{
    if (go && *go == 0) return;      // (an iteration of the predictor-corrector loop enqueued past the loop's end)
    const long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long ip = first + t;
    const double ux = b.ux[ip], uy = b.uy[ip], uz = b.uz[ip];
    const double gaminv = 1.0/sqrt(1.0 + ux*ux*clightsq_inv + uy*uy*clightsq_inv + uz*uz*clightsq_inv);
    const double wq = q_invvol*b.w[ip];
    // predictor-corrector loop: "something other than the cold plasma's rounding residue has reached the current planes"
    // (Engine::d_pc_dist) -- a term that is exactly zero (a cold beam's jx, jy on the Next slice) leaves the planes, and the
    // word, as they are
    if (disturbed && ((cjx >= 0 && (wq*(ux*gaminv) != 0.0 || wq*(uy*gaminv) != 0.0)) || (cjz >= 0 && wq*(uz*gaminv) != 0.0)))
        __hip_atomic_store(disturbed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double sx[ORDER + 1], sy[ORDER + 1];
    const int i0 = shape_weights<ORDER>((b.x[ip] - xoff)*dx_inv, sx);
    const int j0 = shape_weights<ORDER>((b.y[ip] - yoff)*dy_inv, sy);
#pragma unroll
    for (int iy = 0; iy <= ORDER; ++iy) {
#pragma unroll
        for (int ix = 0; ix <= ORDER; ++ix) {
            double* p = f.p + f.off(i0 + ix, j0 + iy);
            const double s = sx[ix]*sy[iy];
            if (cjx >= 0) { atomic_add_f64(p + cjx*f.ns, s*(wq*(ux*gaminv))); atomic_add_f64(p + cjy*f.ns, s*(wq*(uy*gaminv))); }
            if (cjz >= 0) atomic_add_f64(p + cjz*f.ns, s*(wq*(uz*gaminv)));
        }
    }
}

// the two beam deposits of a slice of the explicit schedule in one launch: jz of this slice's block (workgroups
// [0, nbA)) and jx, jy of the next slice's block (the rest) -- different components, no ordering between them
template <int ORDER>
__global__ __launch_bounds__(256)
void k_beam_deposit_pair (SlabView f, BeamPairWork w, double dx_inv, double dy_inv, double xoff, double yoff)
{
    beam_pair_block<ORDER>(f, w, (int)blockIdx.x, dx_inv, dy_inv, xoff, yoff);
}

__global__ __launch_bounds__(256)
void k_beam_new_step (int* nsub, long n)
{
    const long t = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (t < n && nsub[t] > 0) nsub[t] = 0;
}

static double beam_density_at (const hps_deck& d, double x, double y, double z)
{
    if (d.beam_profile == 0) {
        const double a = (x - d.beam_pos_mean[0])/d.beam_pos_std[0];
        const double b = (y - d.beam_pos_mean[1])/d.beam_pos_std[1];
        const double c = (z - d.beam_pos_mean[2])/d.beam_pos_std[2];
        return d.beam_density*std::exp(-0.5*a*a)*std::exp(-0.5*b*b)*std::exp(-0.5*c*c);
    }
    return d.beam_density;
}

// fixed-ppc beam, generated once on the host, stored slice-major (head slice first); restates
// InitBeamFixedPPCSlice (beam/BeamParticleContainerInit.cpp:198-346)
int Engine::init_beam ()
{
    std::vector<double> h[7];
    beam_off.assign(d.nz + 1, 0);
    if (d.beam_profile >= 0) {
        const int nppc = d.beam_ppc[0]*d.beam_ppc[1]*d.beam_ppc[2];
        const int nyp = d.beam_ppc[1], nzp = d.beam_ppc[2];
        for (int isl = d.nz - 1; isl >= 0; --isl) {
            beam_off[d.nz - 1 - isl] = (long)h[0].size();
            for (int j = 0; j < d.ny; ++j) for (int i = 0; i < d.nx; ++i) for (int ip = 0; ip < nppc; ++ip) {
                const int ixp = ip/(nyp*nzp), iyp = (ip % (nyp*nzp)) % nyp, izp = (ip % (nyp*nzp))/nyp;
                const double x = d.lo[0] + (i + (0.5 + ixp)/d.beam_ppc[0])*gm.dx;
                const double y = d.lo[1] + (j + (0.5 + iyp)/d.beam_ppc[1])*gm.dy;
                const double z = d.lo[2] + (isl + (0.5 + izp)/d.beam_ppc[2])*gm.dz;
                const double rx = x - d.beam_pos_mean[0], ry = y - d.beam_pos_mean[1];
                if (z >= d.beam_zmax || z < d.beam_zmin || (rx*rx + ry*ry) > d.beam_radius*d.beam_radius) continue;
                const double dens = beam_density_at(d, x, y, z);
                if (dens <= 0.0) continue;
                h[0].push_back(x); h[1].push_back(y); h[2].push_back(z);
                h[3].push_back(d.beam_umean[0]*gm.c); h[4].push_back(d.beam_umean[1]*gm.c); h[5].push_back(d.beam_umean[2]*gm.c);
                h[6].push_back(std::fabs(dens*(d.si_units ? gm.dx*gm.dy*gm.dz/nppc : 1.0/nppc)));      // scale_fac, BeamParticleContainerInit.cpp:215-216
            }
        }
    }
    beam_off[d.nz] = (long)h[0].size();
    return install_beam(h);
}

// A beam the HOST has initialised (any of the reference's injection types: fixed_weight, fixed_weight_pdf, from_file --
// beam/BeamParticleContainerInit.cpp:348-695 -- draw from amrex::Random or read a file; the slice operators do not care):
// n particles as [7][n] x y z ux uy uz w in the engine's units (u = gamma beta c, w as the deposition takes it), in any
// order.  They are binned into the box's slices (BoxSorter's rule, sorting/BoxSort.cpp:34-43: slice = int((z - lo_z)/dz)), head slice first, input
// order kept inside a slice; particles outside the box in z are counted and left out.  Replaces the deck's beam.
int Engine::set_beam_particles (long n, const double* soa, long* n_outside)
{
    HPS_REQUIRE(n >= 0 && (soa || n == 0), "hps_engine_set_beam_particles: null argument");
    HPS_REQUIRE(steps_begun == 0 && step_index < 0, "hps_engine_set_beam_particles: call before the first hps_engine_begin_step");
    std::vector<long> count((size_t)d.nz + 1, 0);
    std::vector<int> where((size_t)n);
    long outside = 0;
    const double inv_dz = 1.0/gm.dz;
    for (long i = 0; i < n; ++i) {
        const double z = soa[2*n + i];
        const double t = (z - d.lo[2])*inv_dz;
        const int q = (t > -1.0e9 && t < 1.0e9) ? static_cast<int>(t) : -1;      // (the reference's cast: truncation)
        if (q < 0 || q >= d.nz) { where[(size_t)i] = -1; ++outside; continue; }
        const int p = d.nz - 1 - q;                      // p-th slice from the head
        where[(size_t)i] = p; ++count[(size_t)p + 1];
    }
    if (n_outside) *n_outside = outside;
    HPS_REQUIRE(outside == 0 || n_outside, "hps_engine_set_beam_particles: particles outside the box in z (pass n_outside to have them counted and left out)");
    beam_off.assign(d.nz + 1, 0);
    for (int p = 0; p < d.nz; ++p) beam_off[p + 1] = beam_off[p] + count[(size_t)p + 1];
    std::vector<long> next(beam_off.begin(), beam_off.end() - 1);
    std::vector<double> h[7];
    for (int k = 0; k < 7; ++k) h[k].resize((size_t)(n - outside));
    for (long i = 0; i < n; ++i) {
        const int p = where[(size_t)i];
        if (p < 0) continue;
        const long j = next[(size_t)p]++;
        for (int k = 0; k < 7; ++k) h[k][(size_t)j] = soa[(size_t)k*n + i];
    }
    host_beam = true;
    HPS_HIP_CHECK(hipStreamSynchronize(st));
    release_beam();
    return install_beam(h);
}

void Engine::release_beam ()
{
    (void)hipFree(beam_data); (void)hipFree(beam_init); (void)hipFree(bm_store); (void)hipFree(bm_nsub); (void)hipFree(bm_nsub_scr);
    (void)hipFree(d_B); (void)hipFree(d_nfront); (void)hipFree(d_Bimp); (void)hipFree(d_beam_overflow);
    beam_data = beam_init = beam_cur = nullptr; bm_store = nullptr; bm_nsub = bm_nsub_scr = nullptr;
    d_B = nullptr; d_nfront = nullptr; d_Bimp = nullptr; d_beam_overflow = nullptr;
    (void)hipFree(bm_sp); (void)hipFree(bm_sp_scr); (void)hipFree(beam_tag); bm_sp = bm_sp_scr = beam_tag = nullptr;      // (several species: the tag rows)
}

// support of the beam's currents from the extent of its nbeam particles
void Engine::set_beam_box (double xlo, double xhi, double ylo, double yhi)
{
    const int js = d.nx + 2*g, jn = d.ny + 2*g;
    full_box = Box{0, js - 1, 0, jn - 1};
    beam_box_init = Box{0, -1, 0, -1};          // empty
    if (nbeam > 0) {
        // nearest cell -+ (deposit footprint 2 + one cell for the centred differences + 1 spare)
        const int m = 4;
        beam_box_init.ilo = std::max(0,      (int)std::floor((xlo - gm.xoff)/gm.dx + 0.5) - m + g);
        beam_box_init.ihi = std::min(js - 1, (int)std::floor((xhi - gm.xoff)/gm.dx + 0.5) + m + g);
        beam_box_init.jlo = std::max(0,      (int)std::floor((ylo - gm.yoff)/gm.dy + 0.5) - m + g);
        beam_box_init.jhi = std::min(jn - 1, (int)std::floor((yhi - gm.yoff)/gm.dy + 0.5) + m + g);
    }
    if (d.grid_current_on) beam_box_init = full_box;      // the grid current fills jz_beam of every cell
    beam_box = beam_box_init;
}

// the beam's device storage from blocks the device has filled (beam_init.hip; beam_off filled in): no particle crosses to the host
int Engine::install_beam_device (double* blocks_dev, long n, const double box[4])
{
    nbeam = n;
    set_beam_box(box[0], box[1], box[2], box[3]);
    if (nbeam > 0) {
        beam_init = blocks_dev;
        HPS_HIP_CHECK(hipMalloc(&beam_data, 7*nbeam*sizeof(double)));
        HPS_HIP_CHECK(hipMemcpy(beam_data, beam_init, 7*nbeam*sizeof(double), hipMemcpyDeviceToDevice));
        beam_cur = beam_data;
    }
    return install_moving_beam(nullptr);
}

// the beam's device storage from the host arrays h[7] (head slice first, beam_off filled in)
int Engine::install_beam (std::vector<double> (&h)[7])
{
    nbeam = (long)h[0].size();
    {
        double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
        if (nbeam > 0) {
            xlo = xhi = h[0][0]; ylo = yhi = h[1][0];
            for (long k = 1; k < nbeam; ++k) { xlo = std::min(xlo, h[0][k]); xhi = std::max(xhi, h[0][k]); ylo = std::min(ylo, h[1][k]); yhi = std::max(yhi, h[1][k]); }
        }
        set_beam_box(xlo, xhi, ylo, yhi);
    }
    if (nbeam > 0) {
        // slice-major blocks: block p (p-th slice from the head) = [7][count_p] at 7*beam_off[p]
        std::vector<double> blk((size_t)7*nbeam);
        for (int p = 0; p < d.nz; ++p) {
            const long first = beam_off[p], cnt = beam_off[p + 1] - first;
            for (int k = 0; k < 7; ++k)
                for (long i = 0; i < cnt; ++i) blk[(size_t)7*first + (size_t)k*cnt + i] = h[k][first + i];
        }
        HPS_HIP_CHECK(hipMalloc(&beam_data, 7*nbeam*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&beam_init, 7*nbeam*sizeof(double)));
        HPS_HIP_CHECK(hipMemcpy(beam_init, blk.data(), 7*nbeam*sizeof(double), hipMemcpyHostToDevice));
        HPS_HIP_CHECK(hipMemcpy(beam_data, beam_init, 7*nbeam*sizeof(double), hipMemcpyDeviceToDevice));
        beam_cur = beam_data;
    }
    return install_moving_beam(&h);
}

int Engine::install_moving_beam (const std::vector<double> (*h)[7])
{
    moving = (d.dt != 0.0 || d.dt_adaptive);
    if (moving) {
        // global SoA in head-first order + device boundaries (beam.hip)
        const long nb = std::max(nbeam, 1L);
        const bool spin = d.beam_spin_tracking != 0;
        beam_rows = spin ? 10 : 7;
        HPS_HIP_CHECK(hipMalloc(&bm_store, (size_t)2*beam_rows*nb*sizeof(double)));
        HPS_HIP_CHECK(hipMalloc(&bm_nsub, (size_t)nb*sizeof(int)));
        HPS_HIP_CHECK(hipMalloc(&bm_nsub_scr, (size_t)nb*sizeof(int)));
        double* a = bm_store;
        bm = BeamSoA{a, a + nb, a + 2*nb, a + 3*nb, a + 4*nb, a + 5*nb, a + 6*nb, bm_nsub,
                     spin ? a + 7*nb : nullptr, spin ? a + 8*nb : nullptr, spin ? a + 9*nb : nullptr, nullptr};
        a += (size_t)beam_rows*nb;
        bm_scr = BeamSoA{a, a + nb, a + 2*nb, a + 3*nb, a + 4*nb, a + 5*nb, a + 6*nb, bm_nsub_scr,
                         spin ? a + 7*nb : nullptr, spin ? a + 8*nb : nullptr, spin ? a + 9*nb : nullptr, nullptr};
        if (spin && nbeam > 0) {       // initial_spin, normalised, for every particle (BeamParticleContainer.cpp:390-402)
            const double* s0 = d.beam_initial_spin;
            const double nrm = std::sqrt(s0[0]*s0[0] + s0[1]*s0[1] + s0[2]*s0[2]);
            HPS_REQUIRE(nrm > 0.0, "hps_engine_create: beam initial_spin must not vanish");
            for (int q = 0; q < 3; ++q) {
                std::vector<double> v((size_t)nbeam, s0[q]/nrm);
                HPS_HIP_CHECK(hipMemcpy(bm_store + (size_t)(7 + q)*nb, v.data(), nbeam*sizeof(double), hipMemcpyHostToDevice));
            }
        }
        for (int k = 0; h && k < 7 && nbeam > 0; ++k)
            HPS_HIP_CHECK(hipMemcpy(bm_store + (size_t)k*nb, (*h)[k].data(), nbeam*sizeof(double), hipMemcpyHostToDevice));
        if (!h && nbeam > 0)
            if (int e = beam_blocks_to_soa(*this, beam_init, bm_store, nb)) return e;
        HPS_HIP_CHECK(hipMemset(bm_nsub, 0, (size_t)nb*sizeof(int)));
        h_B.assign(beam_off.begin(), beam_off.end());
        HPS_HIP_CHECK(hipMalloc(&d_B, (size_t)(d.nz + 1)*sizeof(long)));
        HPS_HIP_CHECK(hipMemcpy(d_B, h_B.data(), (size_t)(d.nz + 1)*sizeof(long), hipMemcpyHostToDevice));
        HPS_HIP_CHECK(hipMalloc(&d_nfront, (size_t)(d.nz + 2)*sizeof(int)));
        HPS_HIP_CHECK(hipMemset(d_nfront, 0, (size_t)(d.nz + 2)*sizeof(int)));
        HPS_HIP_CHECK(hipMalloc(&d_Bimp, (size_t)(d.nz + 1)*sizeof(long)));
        HPS_HIP_CHECK(hipMemset(d_Bimp, 0, (size_t)(d.nz + 1)*sizeof(long)));
        HPS_HIP_CHECK(hipMalloc(&d_beam_overflow, sizeof(int)));
        HPS_HIP_CHECK(hipMemset(d_beam_overflow, 0, sizeof(int)));
        long mx = 0;
        for (int p = 0; p < d.nz; ++p) mx = std::max(mx, beam_off[p + 1] - beam_off[p]);
        beam_cap = std::max(2*mx, 1L);                 // particles a slice may hold in a hand-off message
        if (nbeam > 0) beam_box = beam_box_init = full_box;          // a moving beam may go anywhere (no beam at all, e.g. a laser driver: the box stays empty)
        if (d.dt_adaptive && !d_mom) {      // (room for HPS_MAX_BEAM_SPECIES; the slots in use are [nz + 1][species][4])
            HPS_HIP_CHECK(hipMalloc(&d_mom, (size_t)4*HPS_MAX_BEAM_SPECIES*(d.nz + 1)*sizeof(double)));
            if (int e = beam_moments_reset(*this)) return e;
        }
        if (multi_beam()) { if (int e = alloc_beam_tags()) return e; }      // the tag row: beam_tag's, or species 0 throughout
    }
    return HPS_OK;
}

int Engine::deposit_beam_slice (int islice, int cjx, int cjy, int cjz, const int* go)
{
    if (nbeam == 0 || islice < 0 || islice >= d.nz) return HPS_OK;
    if (moving) return beam_deposit_moving(*this, d.nz - 1 - islice, cjx, cjy, cjz);
    const long first0 = beam_off[d.nz - 1 - islice], count = beam_off[d.nz - islice] - first0;
    if (count <= 0) return HPS_OK;
    double* blk = beam_cur + 7*first0;
    const BeamView beam{blk, blk + count, blk + 2*count, blk + 3*count, blk + 4*count, blk + 5*count, blk + 6*count};
    const long first = 0;
    const double q_invvol = d.beam_charge*(d.si_units ? 1.0/(gm.dx*gm.dy*gm.dz) : 1.0);      // BeamDepositCurrent.cpp:70-83, level 0
    const double csq_inv = 1.0/(gm.c*gm.c);
    const dim3 grid(ceil_div(count, 256)), block(256);
    SlabView f(slab);
    switch (d.order) {
        case 0: hipLaunchKernelGGL(k_beam_deposit<0>, grid, block, 0, st, f, beam, first, count, cjx, cjy, cjz, q_invvol, csq_inv, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff, go, d_pc_dist); break;
        case 1: hipLaunchKernelGGL(k_beam_deposit<1>, grid, block, 0, st, f, beam, first, count, cjx, cjy, cjz, q_invvol, csq_inv, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff, go, d_pc_dist); break;
        case 2: hipLaunchKernelGGL(k_beam_deposit<2>, grid, block, 0, st, f, beam, first, count, cjx, cjy, cjz, q_invvol, csq_inv, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff, go, d_pc_dist); break;
        default: hipLaunchKernelGGL(k_beam_deposit<3>, grid, block, 0, st, f, beam, first, count, cjx, cjy, cjz, q_invvol, csq_inv, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff, go, d_pc_dist); break;
    }
    return HPS_OK;
}

// k_beam_deposit_pair on `st` (the explicit schedule, where the pair does not ride in the plasma's deposition)
void beam_deposit_pair (const hps_slab& slab, const BeamPairWork& bw, const hps_geom& gm, int order, hipStream_t st)
{
    SlabView f(slab);
    const dim3 b256(256);
#define HPS_PAIR(O) hipLaunchKernelGGL(k_beam_deposit_pair<O>, dim3(bw.nwg), b256, 0, st, f, bw, 1.0/gm.dx, 1.0/gm.dy, gm.xoff, gm.yoff)
    switch (order) { case 0: HPS_PAIR(0); break; case 1: HPS_PAIR(1); break; case 2: HPS_PAIR(2); break; default: HPS_PAIR(3); break; }
#undef HPS_PAIR
}

} // namespace hps

using namespace hps;

extern "C" int hps_engine_beam_info (void* h, long* nbeam, long* offsets_host)
{
    Engine* E = static_cast<Engine*>(h);
    if (nbeam) *nbeam = E->nbeam;
    if (offsets_host) for (int p = 0; p <= E->d.nz; ++p) offsets_host[p] = E->beam_off[p];
    return HPS_OK;
}
extern "C" int hps_engine_set_beam_storage (void* h, double* storage_dev)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(!(E->moving && storage_dev), "hps_engine_set_beam_storage: caller-owned static beam blocks need hipace.dt = 0; a moving beam is handed on with hps_engine_set_beam_import / export_beam_slice / import_beam_slice");
    E->beam_cur = storage_dev ? storage_dev : E->beam_data;
    // caller-owned particles may sit anywhere: treat the whole plane as beam support until told otherwise
    E->beam_box = storage_dev ? E->full_box : E->beam_box_init;
    return HPS_OK;
}
extern "C" int hps_engine_beam_capacity (void* h, long* cap)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving, "hps_engine_beam_capacity: the engine's beam is static (hipace.dt = 0)");
    *cap = E->beam_cap;
    return HPS_OK;
}
extern "C" int hps_engine_set_beam_capacity (void* h, long cap)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving, "hps_engine_set_beam_capacity: the engine's beam is static (hipace.dt = 0)");
    HPS_REQUIRE(E->steps_begun == 0, "hps_engine_set_beam_capacity: call before the first hps_engine_begin_step");
    HPS_REQUIRE(cap >= 1 && cap < (1L << 31), "hps_engine_set_beam_capacity: bad capacity");
    E->beam_cap = cap;
    return HPS_OK;
}
extern "C" int hps_engine_beam_message_rows (void* h, int* rows)
{
    *rows = static_cast<Engine*>(h)->beam_rows + (static_cast<Engine*>(h)->multi_beam() ? 1 : 0);      // (several species: one row for the tag)
    return HPS_OK;
}
extern "C" int hps_engine_beam_spin (void* h, double* soa_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving && E->bm.sx && soa_host, "hps_engine_beam_spin: the beam has no spin (do_spin_tracking with hipace.dt != 0)");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    const double* a[3] = {E->bm.sx, E->bm.sy, E->bm.sz};
    for (int q = 0; q < 3; ++q)
        if (E->nbeam > 0) HPS_HIP_CHECK(hipMemcpy(soa_host + (size_t)q*E->nbeam, a[q], E->nbeam*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}
extern "C" int hps_engine_set_beam_import (void* h, int on)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving, "hps_engine_set_beam_import: the engine's beam is static (hipace.dt = 0)");
    E->beam_import = (on != 0);
    return HPS_OK;
}
extern "C" int hps_engine_export_beam_slice (void* h, int islice, double* msg_dev)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving && msg_dev && islice >= 0 && islice < E->d.nz, "hps_engine_export_beam_slice: bad argument");
    return beam_export_slice(*E, islice, msg_dev, E->beam_cap);
}
extern "C" int hps_engine_import_beam_slice (void* h, int islice, const double* msg_dev)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E->moving && E->beam_import && msg_dev && islice >= 0 && islice < E->d.nz, "hps_engine_import_beam_slice: bad argument (import mode off?)");
    return beam_import_slice(*E, islice, msg_dev, E->beam_cap);
}
extern "C" int hps_engine_beam_state (void* h, long* boundaries_host, double* soa_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(!E->multi_beam(), "hps_engine_beam_state: the engine holds several beam species: hps_engine_beam_state_species returns one of them");
    if (!E->moving) {
        // static beam: the slice-major blocks [slice p][7][count_p] gathered into the same global layout
        HPS_HIP_CHECK(hipStreamSynchronize(E->st));
        if (boundaries_host) for (int p = 0; p <= E->d.nz; ++p) boundaries_host[p] = E->beam_off[p];
        if (soa_host && E->nbeam > 0)
            for (int p = 0; p < E->d.nz; ++p) {
                const long first = E->beam_off[p], cnt = E->beam_off[p + 1] - first;
                for (int k = 0; k < 7 && cnt > 0; ++k)
                    HPS_HIP_CHECK(hipMemcpy(soa_host + (size_t)k*E->nbeam + first, E->beam_cur + 7*first + (size_t)k*cnt, cnt*sizeof(double), hipMemcpyDeviceToHost));
            }
        return HPS_OK;
    }
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    {   int ov = 0;
        HPS_HIP_CHECK(hipMemcpy(&ov, E->d_beam_overflow, sizeof(int), hipMemcpyDeviceToHost));
        HPS_REQUIRE(ov == 0, "moving beam: a slice outgrew the hand-off capacity (twice the fullest injected slice)"); }
    if (boundaries_host) HPS_HIP_CHECK(hipMemcpy(boundaries_host, E->d_B, (size_t)(E->d.nz + 1)*sizeof(long), hipMemcpyDeviceToHost));
    if (soa_host && E->nbeam > 0)
        for (int k = 0; k < 7; ++k)
            HPS_HIP_CHECK(hipMemcpy(soa_host + (size_t)k*E->nbeam, E->bm_store + (size_t)k*std::max(E->nbeam, 1L), E->nbeam*sizeof(double), hipMemcpyDeviceToHost));
    return HPS_OK;
}
extern "C" int hps_engine_beam_moments (void* h, double* out4)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && out4, "hps_engine_beam_moments: null argument");
    HPS_REQUIRE(E->d_mom, "hps_engine_beam_moments: the deck has no adaptive time step (dt_adaptive)");
    HPS_REQUIRE(!E->multi_beam(), "hps_engine_beam_moments: the engine holds several beam species, whose moments are never summed: hps_engine_beam_moments_species");
    HPS_HIP_CHECK(hipMemcpyAsync(out4, E->d_mom + 4*E->d.nz, 4*sizeof(double), hipMemcpyDeviceToHost, E->st));
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    return HPS_OK;
}
extern "C" int hps_engine_deposit_beam_species (void* h, int islice, unsigned species_mask, int cjx, int cjy, int cjz)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_deposit_beam_species: null engine");
    HPS_REQUIRE(E->moving, "hps_engine_deposit_beam_species: needs a moving beam (hipace.dt != 0 or adaptive): a static beam has no species");
    HPS_REQUIRE(E->steps_begun > 0 && !E->beam_import, "hps_engine_deposit_beam_species: call after hps_engine_begin_step, on an engine that holds its beam");
    HPS_REQUIRE(islice >= 0 && islice < E->d.nz, "hps_engine_deposit_beam_species: no such slice");
    HPS_REQUIRE((cjx >= 0) == (cjy >= 0), "hps_engine_deposit_beam_species: cjx and cjy go together");
    for (int c : {cjx, cjy, cjz}) HPS_REQUIRE(c >= -1 && c < E->slab.ncomp, "hps_engine_deposit_beam_species: bad component");
    HPS_REQUIRE(E->multi_beam(), "hps_engine_deposit_beam_species: the engine holds one beam species (no tag row to select by)");
    E->flush_shift();
    return beam_deposit_species(*E, E->d.nz - 1 - islice, species_mask, cjx, cjy, cjz);
}
extern "C" int hps_engine_assume_initial_beam_support (void* h)
{
    Engine* E = static_cast<Engine*>(h);
    E->beam_box = E->beam_box_init;
    return HPS_OK;
}
extern "C" int hps_engine_initial_beam (void* h, double* dst_dev)
{
    Engine* E = static_cast<Engine*>(h);
    if (E->nbeam > 0) HPS_HIP_CHECK(hipMemcpy(dst_dev, E->beam_init, 7*E->nbeam*sizeof(double), hipMemcpyDeviceToDevice));
    return HPS_OK;
}
extern "C" int hps_engine_set_beam_particles (void* h, long n, const double* soa_host, long* n_outside)
{
    HPS_REQUIRE(h, "hps_engine_set_beam_particles: null engine");
    Engine* E = static_cast<Engine*>(h);
    return E->fill_selected_species("hps_engine_set_beam_particles", [&] { return E->set_beam_particles(n, soa_host, n_outside); });
}
// ---- several beam species (the kernels and the merge: beam.hip) ----------------------------------------------------
extern "C" int hps_engine_add_beam_species (void* h, const hps_beam_species* species, int* index_out)
{
    HPS_REQUIRE(h, "hps_engine_add_beam_species: null engine");
    return static_cast<Engine*>(h)->add_beam_species(species, index_out);
}
extern "C" int hps_engine_select_beam_species (void* h, int k)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_select_beam_species: null engine");
    HPS_REQUIRE(k >= 0 && k < E->n_beam_species(), "hps_engine_select_beam_species: no such beam species (hps_engine_add_beam_species gives the numbers)");
    E->sel_species = k;
    return HPS_OK;
}
extern "C" int hps_engine_beam_species_info (void* h, int* n_host, long* counts_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_beam_species_info: null engine");
    if (n_host) *n_host = E->n_beam_species();
    if (counts_host) {
        if (E->bsp.empty()) counts_host[0] = E->nbeam;
        for (size_t k = 0; k < E->bsp.size(); ++k) counts_host[k] = E->bsp[k].count;
    }
    return HPS_OK;
}
extern "C" int hps_engine_beam_state_species (void* h, int k, long* count_host, long* boundaries_host, double* soa_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_beam_state_species: null engine");
    HPS_REQUIRE(k >= -1 && k < E->n_beam_species(), "hps_engine_beam_state_species: no such beam species");
    if (k == -1 && E->multi_beam()) {      // the whole container, whatever the species
        HPS_HIP_CHECK(hipStreamSynchronize(E->st));
        if (count_host) *count_host = E->nbeam;
        if (boundaries_host) HPS_HIP_CHECK(hipMemcpy(boundaries_host, E->d_B, (size_t)(E->d.nz + 1)*sizeof(long), hipMemcpyDeviceToHost));
        for (int q = 0; soa_host && q < 7 && E->nbeam > 0; ++q)
            HPS_HIP_CHECK(hipMemcpy(soa_host + (size_t)q*E->nbeam, E->bm_store + (size_t)q*E->nbeam, E->nbeam*sizeof(double), hipMemcpyDeviceToHost));
        return HPS_OK;
    }
    if (!E->multi_beam()) {
        if (count_host) *count_host = E->nbeam;
        return hps_engine_beam_state(h, boundaries_host, soa_host);
    }
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    const int nz = E->d.nz; const long nb = E->nbeam, cnt = E->bsp[(size_t)k].count;
    if (count_host) *count_host = cnt;
    if (!boundaries_host && !soa_host) return HPS_OK;
    std::vector<long> B((size_t)nz + 1, 0); std::vector<unsigned char> tag((size_t)std::max(nb, 1L)); std::vector<double> row;
    HPS_HIP_CHECK(hipMemcpy(B.data(), E->d_B, B.size()*sizeof(long), hipMemcpyDeviceToHost));
    if (nb > 0) HPS_HIP_CHECK(hipMemcpy(tag.data(), E->bm_sp, (size_t)nb, hipMemcpyDeviceToHost));
    if (boundaries_host) {
        long j = 0; boundaries_host[0] = 0;
        for (int p = 0; p < nz; ++p) { for (long i = B[(size_t)p]; i < B[(size_t)p + 1]; ++i) j += tag[(size_t)i] == k; boundaries_host[p + 1] = j; }
        HPS_REQUIRE(j == cnt, "hps_engine_beam_state_species: the container's tags do not hold the species' particle count");
    }
    if (soa_host && cnt > 0) {
        row.resize((size_t)nb);
        for (int q = 0; q < 7; ++q) {
            HPS_HIP_CHECK(hipMemcpy(row.data(), E->bm_store + (size_t)q*std::max(nb, 1L), (size_t)nb*sizeof(double), hipMemcpyDeviceToHost));
            long j = 0;
            for (long i = B[0]; i < B[(size_t)nz] && j < cnt; ++i) if (tag[(size_t)i] == k) soa_host[(size_t)q*cnt + j++] = row[(size_t)i];
        }
    }
    return HPS_OK;
}
extern "C" int hps_engine_beam_moments_species (void* h, double* out_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && out_host, "hps_engine_beam_moments_species: null argument");
    HPS_REQUIRE(E->d_mom, "hps_engine_beam_moments_species: the deck has no adaptive time step (dt_adaptive)");
    const int ns = E->n_beam_species();
    HPS_HIP_CHECK(hipMemcpyAsync(out_host, E->d_mom + (size_t)4*ns*E->d.nz, (size_t)4*ns*sizeof(double), hipMemcpyDeviceToHost, E->st));
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    return HPS_OK;
}
extern "C" int hps_engine_beam_tags (void* h, unsigned char* tags_host)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && tags_host, "hps_engine_beam_tags: null argument");
    HPS_HIP_CHECK(hipStreamSynchronize(E->st));
    if (E->nbeam == 0) return HPS_OK;
    if (!E->bm.sp) { std::memset(tags_host, 0, (size_t)E->nbeam); return HPS_OK; }
    HPS_HIP_CHECK(hipMemcpy(tags_host, E->bm.sp, (size_t)E->nbeam, hipMemcpyDeviceToHost));
    return HPS_OK;
}
extern "C" int hps_engine_beam_kernels (void* h, char* buf, long cap, long* len, int* tagged)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E, "hps_engine_beam_kernels: null engine");
    const std::string all = beam_kernel_names(*E);
    if (len) *len = (long)all.size();
    if (tagged) *tagged = E->bm.sp != nullptr ? 1 : 0;
    if (buf && cap > 0) { const size_t n = std::min<size_t>(all.size(), (size_t)cap - 1); std::memcpy(buf, all.data(), n); buf[n] = 0; }
    return HPS_OK;
}
