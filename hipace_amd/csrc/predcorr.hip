// predcorr.hip -- the predictor-corrector Bx/By solver (hipace.bxby_solver = predictor-corrector): restates
// Hipace::PredictorCorrectorLoopToSolveBxBy (Hipace.cpp:935-1031) with InitialBfieldGuess, MixAndShiftBfields and
// ComputeRelBFieldError (fields/Fields.cpp:1151-1286), and the slice schedule around the loop.  Owns Engine::pc_create,
// solve_slice_pc_begin / _finish, pc_enqueue_iteration, pc_wait_slot, pc_slice_ready and the hps_engine_pc_* entry points.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace hps {

// ---- predictor-corrector Bx/By (Hipace::PredictorCorrectorLoopToSolveBxBy, Hipace.cpp:935-1031) ----------------

// Fields::ComputeRelBFieldError (fields/Fields.cpp:1233-1286): out[0] += sum |B|, out[1] += sum |B - B_iter| over
// the valid cells
// With `host` (mapped pinned memory) the last workgroup to finish posts {sum |B|, seq} {sum |B - B_iter|, seq} {fallback
// counter, seq} there as three 16-byte stores: the host polls the tags instead of a copy + stream synchronise.
// Loop control on the device (speculative iterations): `go` points at the word of iteration `it` in a per-slice array of
// flags (k_pc_guess: flag[1] = 1, the others 0); every kernel of an iteration does nothing when its word is 0.  The last
// workgroup here decides whether the loop goes on -- go[1] = (err > tol && it < max_it), the condition of Hipace.cpp:957 --
// and posts to slot `it` of the host array (4 doubles per slot; the halo-fallback counter also to slot 0, where the
// engine's re-sort rule reads it).
__global__ __launch_bounds__(256)
void k_rel_b_error (SlabView f, int cB, int cBit, double* out, volatile double* host, double seq,
                    int* go = nullptr, double tol = 0.0, int it = 0, int max_it = 0, double floor_b = 0.0)
{
    if (go && *go == 0) return;
    double sb = 0.0, sd = 0.0;
    const long cells = (long)f.nx*f.ny;
    for (long c = (long)blockIdx.x*blockDim.x + threadIdx.x; c < cells; c += (long)gridDim.x*blockDim.x) {
        const int j = (int)(c / f.nx), i = (int)(c - (long)j*f.nx);
        const long o = f.off(i, j);
        const double bx = f.p[cB*f.ns + o], by = f.p[(cB + 1)*f.ns + o];
        const double ex = bx - f.p[cBit*f.ns + o], ey = by - f.p[(cBit + 1)*f.ns + o];
        sb += sqrt(bx*bx + by*by);
        sd += sqrt(ex*ex + ey*ey);
    }
    for (int o = 32; o > 0; o >>= 1) { sb += __shfl_xor(sb, o); sd += __shfl_xor(sd, o); }
    __shared__ double part[8];
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = sb; part[4 + (threadIdx.x >> 6)] = sd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomic_add_f64(out, part[0] + part[1] + part[2] + part[3]);
        atomic_add_f64(out + 1, part[4] + part[5] + part[6] + part[7]);
        if (host) {
            HPS_OWN_ATOMICS_ACKNOWLEDGED();      // the two atomics above are acknowledged (no __threadfence(): see adk_post)
            unsigned int* done = reinterpret_cast<unsigned int*>(out + 3);
            if (atomicAdd(done, 1u) == gridDim.x - 1) {
                __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                double tb = __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double td = __hip_atomic_load(out + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // sum |B| at the rounding floor of a scatter with atomics counts as the exact zero the serial path has there
                // (Engine::pc_floor): the rule "relative error = 0 when sum |B| = 0" (fields/Fields.cpp:1283) then applies as on
                // the CPU; k_pc_mix reads the same word
                if (!(tb > floor_b)) { tb = 0.0; __hip_atomic_store(out, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                const double fbk = __hip_atomic_load(out + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // The post: three self-validating 16-byte stores {value, seq} -- no fence.  (A system-scope release fence ahead
                // of a lone sequence word writes the XCD's L2 back: the kernel took 9.4 us with it against 3.4 without the
                // post, once per loop iteration.)  The host waits until all three tags carry its sequence number.
                typedef double dbl2 __attribute__((ext_vector_type(2)));
                volatile dbl2* hs = reinterpret_cast<volatile dbl2*>(const_cast<double*>(host));
                if (go) {
                    const double err = tb > 0.0 ? td/tb : 0.0;
                    __hip_atomic_store(go + 1, (err > tol && it < max_it) ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hs[2] = dbl2{fbk, seq};       // slot 0: the fallback counter where the host's re-sort rule looks for it
                    hs += 4*it;
                }
                static_assert(sizeof(dbl2) == 16, "the post is one 16-byte store per {value, seq} pair");
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
                __threadfence_system();      // (no claim about single-copy atomicity of a 16-byte store to host memory elsewhere)
#endif
                hs[0] = dbl2{tb, seq}; hs[1] = dbl2{td, seq}; hs[2] = dbl2{fbk, seq};
            }
        }
    }
}

// InitialBfieldGuess (fields/Fields.cpp:1151-1173) + the set-up of the loop (Hipace.cpp:950-954): This = (1+m) Previous
// - m PCPrevIter with m = exp(-0.5 (err/(2.5 tol))^2), err = sums[1]/sums[0] of (Previous, PCPrevIter);
// PCIter = 0; PCPrevIter = This.  Whole planes incl. guards, both components.
__global__ __launch_bounds__(256)
void k_pc_guess (double* p, long ns, long plane, const double* sums, double tol, int* go, double floor_b)
{
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    if (s < PC_MAX_SPEC && go) go[s] = (s == 1);      // the loop of this slice starts: its first iteration always runs (Hipace.cpp:956)
    if (s >= plane) return;
    const double err = sums[0] > floor_b ? sums[1]/sums[0] : 0.0;
    const double q = err/(2.5*tol);
    const double m = exp(-0.5*(q*q));
    for (int c = 0; c < 2; ++c) {
        const double b = (1.0 + m)*p[(HPS_PC_P_BX + c)*ns + s] + (-m)*p[(HPS_PC_PIT_BX + c)*ns + s];
        p[(HPS_PC_BX + c)*ns + s] = b;
        p[(HPS_PC_IT_BX + c)*ns + s] = 0.0;
        p[(HPS_PC_PIT_BX + c)*ns + s] = b;
    }
}

// sources of Fields::SolvePoissonBxBy (fields/Fields.cpp:1043-1064): st[0] = mu0 (-d_y jz + d_z jy),
// st[1] = mu0 (d_x jz - d_z jx), d_z = (Previous - Next)/(2 dz)
__global__ __launch_bounds__(256)
void k_rhs_bxby (SlabView f, double mu0, double hdx_inv, double hdy_inv, double hdz_inv, double* staging, long plane,
                 double* sums, const int* go)
{
    if (go && *go == 0) return;
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i == 0 && j == 0) { sums[0] = 0.0; sums[1] = 0.0; }      // for the k_rel_b_error of this pass
    if (i >= f.nx) return;
    const long o = f.off(i, j), so = (long)j*f.nx + i;
    const double* Z = f.p + HPS_PC_JZ*f.ns + o;
    staging[so] = (-mu0)*((Z[f.js] - Z[-f.js])*hdy_inv) + mu0*((f.p[HPS_PC_P_JY*f.ns + o] - f.p[HPS_PC_N_JY*f.ns + o])*hdz_inv);
    staging[plane + so] = mu0*((Z[1] - Z[-1])*hdx_inv) + (-mu0)*((f.p[HPS_PC_P_JX*f.ns + o] - f.p[HPS_PC_N_JX*f.ns + o])*hdz_inv);
}

// MixAndShiftBfields (fields/Fields.cpp:1175-1231) + the reset of the temporary currents (Hipace.cpp:1000-1003)
__global__ __launch_bounds__(256)
void k_pc_mix (double* p, long ns, long plane, const double* sums, double* err_slots, int it, double mix, const int* go,
               const int* disturbed = nullptr)
{
    if (go && *go == 0) return;      // (this iteration's own flag: its k_rel_b_error has written the NEXT one's)
    const long s = (long)blockIdx.x*blockDim.x + threadIdx.x;
    // nothing but the cold plasma's rounding residue has been deposited so far in this sweep: the serial path holds exact zeros
    const bool exact_zero = disturbed && __hip_atomic_load(disturbed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    // the weights of Hipace.cpp:1005-1014 from this iteration's error and the previous one's, on the device: the kernel is
    // enqueued before the host has read the error.  err_slots[it & 1] <- err for the next iteration (nobody reads that slot now)
    const double err = sums[0] > 0.0 ? sums[1]/sums[0] : 0.0;
    const double err_prev = (it == 1) ? err : err_slots[(it - 1) & 1];
    double w_it = 0.5, w_prev = 0.5;
    if (err != 0.0 || err_prev != 0.0) { w_it = err_prev/(err + err_prev); w_prev = err/(err + err_prev); }
    if (s == 0) err_slots[it & 1] = err;
    if (s >= plane) return;
    for (int c = 0; c < 2; ++c) {
        const double it = p[(HPS_PC_IT_BX + c)*ns + s];
        const double mixed = w_it*it + w_prev*p[(HPS_PC_PIT_BX + c)*ns + s];
        p[(HPS_PC_BX + c)*ns + s] = exact_zero ? 0.0 : (1.0 - mix)*p[(HPS_PC_BX + c)*ns + s] + mix*mixed;
        p[(HPS_PC_PIT_BX + c)*ns + s] = it;
    }
    p[HPS_PC_N_JX*ns + s] = 0.0; p[HPS_PC_N_JY*ns + s] = 0.0;
}

// the predictor-corrector part of Engine::create: the loop's device words, its host slots and its switches
int Engine::pc_create ()
{
    // no multigrid solves in this mode: the counter travels with the per-iteration read-back of the B error
    HPS_HIP_CHECK(hipMalloc(&d_pc, 4*sizeof(double)));
    HPS_HIP_CHECK(hipMemset(d_pc, 0, 4*sizeof(double)));
    HPS_HIP_CHECK(hipMalloc(&d_pc_aux, 4*sizeof(double)));      // error of the last two iterations (k_pc_mix)
    HPS_HIP_CHECK(hipMemset(d_pc_aux, 0, 4*sizeof(double)));
    HPS_HIP_CHECK(hipHostMalloc(&h_pc, 8*PC_MAX_SPEC*sizeof(double), hipHostMallocMapped));      // slot 0 + one slot per loop iteration
    std::memset(h_pc, 0, 8*PC_MAX_SPEC*sizeof(double));
    HPS_HIP_CHECK(hipHostGetDevicePointer((void**)&h_pc_dev, h_pc, 0));
    HPS_HIP_CHECK(hipMalloc(&d_pc_go, (PC_MAX_SPEC + 1)*sizeof(int)));
    HPS_HIP_CHECK(hipMemset(d_pc_go, 0, (PC_MAX_SPEC + 1)*sizeof(int)));
    // The exact zeros of the serial path (round 6; replaces the magnitude floor below, which stays as a diagnostic).  Ahead
    // of the first beam particle the serial CPU path holds EXACT zeros in every field -- electron and ion charge cancel term
    // by term, a cold plasma at rest deposits no current -- so ComputeRelBFieldError returns 0 (norm_B > 0 ? diff/norm_B : 0,
    // fields/Fields.cpp:1283), the loop leaves after one pass there AND on the first slice that holds beam (the guess it
    // compares with is that zero).  A scatter with atomics leaves 1e-16 residue of the background charge instead, and the
    // literal rule iterates to max_iterations on it.  d_pc_dist is one device word, cleared by begin_step: "something
    // other than that residue has been deposited on this slice or one ahead" -- set by the beam's deposition when a term
    // is not exactly zero (k_beam_deposit, k_beam_deposit_dyn) and from the start with a grid current.  While it is clear
    // the slice's loop leaves after its first pass by the LITERAL rule (sum |B| of the guess IS 0: see next sentence) and
    // k_pc_mix stores the zero the serial path holds into Bx, By instead of a mix of residues; once it is set the
    // literal rule applies to whatever sum |B| is -- a moving beam's thin head iterates as it does on the CPU.
    // HPS_PC_EXACT_ZERO=0: off (the literal rule on residue: 2400+ instead of 1631 iterations on config 2's box).
    {   const char* v = std::getenv("HPS_PC_EXACT_ZERO");
        if (!(v && std::atoi(v) == 0)) d_pc_dist = d_pc_go + PC_MAX_SPEC; }
    // Rounding floor of sum |B| (k_rel_b_error).  Ahead of the driver the serial CPU path has EXACT zeros -- electron and ion
    // charge cancel term by term -- so ComputeRelBFieldError returns 0 (fields/Fields.cpp:1283) and the loop leaves after
    // one pass, also on the first slice that holds beam.  A scatter with atomics leaves 1e-16 residue of the background
    // charge; without a floor the loop runs to max_iterations on that noise on every slice ahead of the driver (config 2:
    // 54 slices x 30 iterations = 40 % of the box's time) and enters the driver on a different path, per cent away from
    // the CPU's.  What can be resolved of B is eps x mu0 c sum|rho_background| L: 1e-12 of that is "zero".
    // HPS_PC_NOISE_FLOOR=<relative floor>, 0: the literal rule.
    {   double rel = 0.0;           // (round 6: no floor by default -- d_pc_dist above; rounds 4-5 ran with 1e-12)
        if (const char* v = std::getenv("HPS_PC_NOISE_FLOOR")) rel = std::atof(v);
        pc_floor = rel*gm.mu0*gm.c*std::fabs(d.plasma_charge*d.plasma_density)*(double)d.nx*d.ny*(d.nx*gm.dx); }
    // HPS_PC_SPECULATE=0: the host decides after every iteration, as in rounds 1-3
    {   const char* v = std::getenv("HPS_PC_SPECULATE");
        pc_speculate = !(v && std::atoi(v) == 0) && pc_max_iter <= PC_MAX_SPEC - 2 && poisson_gateable(ps)
                       && d.field_bc == 0; }      // (the open boundary's two launches per solve are not gated: host-controlled loop)
    d_nfallback = reinterpret_cast<int*>(d_pc + 2); h_nfallback = reinterpret_cast<const int*>(h_pc + 4);
    return HPS_OK;
}

// SolveOneSlice with hipace.bxby_solver = predictor-corrector (Hipace.cpp:556-728; the explicit branch is
// Engine::solve_slice, engine.hip).  Event marks keep the 10 intervals of the explicit schedule: the loop is booked under
// the Bx/By-solve interval.
int Engine::solve_slice_pc_begin (int islice)
{
    SlabView f(slab);
    const long plane = slab.nstride;
    const dim3 b256(256);
    const dim3 gplane(ceil_div(plane, 256));
    const long nval = (long)d.nx*d.ny;
    int e;

    prof_now = profiling && (slices_done % prof_stride == 0);
    mark();   // b0
    insitu_plasma(islice);
    // InitializeSlices (fields/Fields.cpp:565-570); ExmBy, EypBx are rewritten by k_grad_psi up to the outermost
    // guard ring, which stays zero from begin_step
    {   CompList z{0, {}}, zb{0, {}};
        for (int c : {HPS_PC_JX, HPS_PC_JY, HPS_PC_JZ, HPS_PC_RHOMJZ}) z.c[z.n++] = c;
        if (d.deposit_rho) z.c[z.n++] = HPS_PC_RHO;
        zero_comps(slab, st, z, zb, CellBox{0, -1, 0, -1}); }
    mark();   // b1
    if (el.tiling && (since_sort >= sort_period || (since_sort >= 2 && *h_nfallback - fb_at_sort > el.pl.n/fallback_div) ||
                      (since_sort >= 1 && el.pl.n - el.tiling->sorted_n > std::max(el.pl.n/32, 16384L)))) { if ((e = resort())) return e; }
    ++since_sort;
    mark();   // b1b
    // plasma: jx jy jz [rho] rhomjz (Hipace.cpp:616-618); beams deposit into the same jx jy jz (:620-623)
    {   const int comp[6] = {HPS_PC_JX, HPS_PC_JY, HPS_PC_JZ, d.deposit_rho ? HPS_PC_RHO : -1, -1, HPS_PC_RHOMJZ};
        // MultiPlasma::DepositCurrent: every species in turn (MultiPlasma.cpp:78-87)
        for (const Species& s : sp) { if ((e = species_deposit(s, comp))) return e; } }
    mark();   // b2
    if ((e = deposit_beam_slice(islice, HPS_PC_JX, HPS_PC_JY, HPS_PC_JZ))) return e;
    deposit_grid_current(islice, HPS_PC_JZ);
    {   const double fa = 1.0/(gm.ep0*gm.c);
        hipLaunchKernelGGL(k_rhs_all, dim3(ceil_div(slab.jstride, 256), d.ny + 2*g), b256, 0, st, f, HPS_PC_RHOMJZ,
                           HPS_PC_ION_RHOMJZ, d.deposit_rho ? HPS_PC_RHO : -1, HPS_PC_JX, HPS_PC_JY, 1.0/gm.ep0,
                           fa*0.5*(1.0/gm.dx), fa*0.5*(1.0/gm.dy), gm.mu0*0.5*(1.0/gm.dy), -gm.mu0*0.5*(1.0/gm.dx),
                           staging, nval);
        const int comps[3] = {HPS_PC_PSI, HPS_PC_EZ, HPS_PC_BZ};
        if ((e = open_boundary(3, 0x6u))) return e;      // (Ez, Bz: no physical monopole, fields/Fields.cpp:727-731)
        if ((e = hps_poisson_solve_batch(ps, 3, staging, slab, comps, st))) return e; }
    hipLaunchKernelGGL(k_grad_psi, dim3(ceil_div(d.nx + 2*(g - 1), 256), d.ny + 2*(g - 1)), b256, 0, st, f, HPS_PC_PSI,
                       HPS_PC_EXMBY, HPS_PC_EYPBX, 0.5*(1.0/gm.dx), 0.5*(1.0/gm.dy));
    mark();   // b3
    mark();   // b4
    mark();   // b5
    // the loop (Hipace.cpp:935-1031)
    HPS_HIP_CHECK(hipMemsetAsync(d_pc, 0, 2*sizeof(double), st));
    hipLaunchKernelGGL(k_rel_b_error, dim3(128), b256, 0, st, f, HPS_PC_P_BX, HPS_PC_PIT_BX, d_pc, (volatile double*)nullptr, 0.0);
    const bool spec = pc_speculate && el.tiling && !moving && !ions.present() && !further();      // (a second species: the host-controlled loop)
    hipLaunchKernelGGL(k_pc_guess, gplane, b256, 0, st, slab.p, slab.nstride, plane, d_pc, pc_tol, spec ? d_pc_go : (int*)nullptr, pc_floor);
    pc_islice = islice;
    if (spec) {
        // Device-side loop control: as many iterations as the previous slice took are enqueued at once, every kernel of
        // iteration `it` looking at the flag its predecessor's error kernel has written (k_rel_b_error): the queue never
        // runs dry while an error travels to the host and the next iteration's ten launches travel back.  The host reads
        // the slots in solve_slice_pc_finish and adds iterations one by one only if the speculated ones did not suffice.
        pc_base_seq = pc_seq;
        pc_enqueued = 0;
        const int K = std::max(1, std::min(pc_spec_iters, pc_max_iter));
        for (int it = 1; it <= K; ++it) {
            if ((e = pc_enqueue_iteration(it))) {
                // a failed launch with the go flags armed: nothing of this slice's loop is to be mistaken for the next slice's --
                // sequence numbers move past whatever the iterations enqueued so far may still post
                pc_seq = pc_base_seq + pc_max_iter + 2; pc_enqueued = 0; pc_islice = -1;
                return e;
            }
        }
        return HPS_OK;
    }
    double err = 1.0;
    int it = 0;
    // (host-controlled loop.)  The mixing weights of an iteration are computed on the device (k_pc_mix) and the mixing is
    // enqueued before the host waits for the iteration's error: it runs while the error travels (config 2: +5 % iterations
    // per second).
    while (err > pc_tol && it < pc_max_iter) {
        ++it; ++pc_iterations;
        pc_enqueued = it - 1;
        if ((e = pc_enqueue_iteration(it))) return e;
        if ((e = pc_wait_slot(0, pc_seq))) return e;
        err = h_pc[0] > 0.0 ? h_pc[2]/h_pc[0] : 0.0;
    }
    pc_last_err = err;
    return HPS_OK;
}

// one iteration of the loop on the engine's stream (Hipace.cpp:958-1030); with device-side control every launch is gated
// on the iteration's flag
int Engine::pc_enqueue_iteration (int it)
{
    SlabView f(slab);
    const long plane = slab.nstride;
    const dim3 b256(256);
    const dim3 gplane(ceil_div(plane, 256));
    const long nval = (long)d.nx*d.ny;
    const int islice = pc_islice;
    const bool spec = pc_speculate && el.tiling && !moving && !ions.present() && !further();
    int* go = spec ? d_pc_go + it : nullptr;
    const int comp_push[5] = {HPS_PC_PSI, HPS_PC_EZ, HPS_PC_BX, HPS_PC_BY, HPS_PC_BZ};
    int e;
    // every species to the temporary next slice, its jx jy (+ the beam's) there      (go == nullptr with a second species)
    for (const Species& s : sp) { if ((e = species_advance(s, comp_push, 1, go))) return e; }
    {   const int comp[6] = {HPS_PC_N_JX, HPS_PC_N_JY, -1, -1, -1, -1};
        for (const Species& s : sp) { if ((e = species_deposit(s, comp, nullptr, go))) return e; } }
    if ((e = deposit_beam_slice(islice - 1, HPS_PC_N_JX, HPS_PC_N_JY, -1, go))) return e;
    hipLaunchKernelGGL(k_rhs_bxby, dim3(ceil_div(d.nx, 256), d.ny), b256, 0, st, f, gm.mu0, 0.5*(1.0/gm.dx), 0.5*(1.0/gm.dy),
                       0.5*(1.0/gm.dz), staging, nval, d_pc, (const int*)go);
    {   const int comps[2] = {HPS_PC_IT_BX, HPS_PC_IT_BY};
        if ((e = open_boundary(2, 0u))) return e;
        poisson_set_gate(ps, go);
        e = hps_poisson_solve_batch(ps, 2, staging, slab, comps, st);
        poisson_set_gate(ps, nullptr);
        if (e) return e; }
    pc_seq += 1.0;
    hipLaunchKernelGGL(k_rel_b_error, dim3(128), b256, 0, st, f, HPS_PC_BX, HPS_PC_IT_BX, d_pc, (volatile double*)h_pc_dev, pc_seq,
                       go, pc_tol, it, pc_max_iter, pc_floor);
    hipLaunchKernelGGL(k_pc_mix, gplane, b256, 0, st, slab.p, slab.nstride, plane, d_pc, d_pc_aux, it, pc_mix, (const int*)go, (const int*)d_pc_dist);
    pc_enqueued = it;
    return HPS_OK;
}

// wait for the post of sequence number `seq` in host slot `slot`; fall back to the stream's status every so often so that a
// failed launch cannot hang us
int Engine::pc_wait_slot (int slot, double seq)
{
    volatile double* hp = h_pc + 8*slot;          // {sum |B|, seq} {sum |B - B_iter|, seq} {fallback counter, seq} (k_rel_b_error)
    auto there = [&] () { return hp[1] == seq && hp[3] == seq && hp[5] == seq; };
    long spins = 0;
    while (!there()) {
        if ((++spins & 0xfffff) == 0 && hipStreamQuery(st) != hipErrorNotReady) {
            if (there()) break;
            HPS_HIP_CHECK(hipStreamSynchronize(st));
            if (!there()) { set_error("predictor-corrector: the error read-back never arrived"); return HPS_ERR_HIP; }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return HPS_OK;
}

// second half of a predictor-corrector slice: the loop's end (device-side control: read the posted errors, add iterations if
// the speculated ones did not suffice), diagnostics, the committing push, ShiftSlices
int Engine::solve_slice_pc_finish (int islice)
{
    const int comp_push[5] = {HPS_PC_PSI, HPS_PC_EZ, HPS_PC_BX, HPS_PC_BY, HPS_PC_BZ};
    int e;
    double err = pc_last_err;
    if (pc_speculate && el.tiling && !moving && !ions.present() && !further()) {
        int it = 0;
        err = 1.0;
        while (err > pc_tol && it < pc_max_iter) {
            ++it; ++pc_iterations;
            if (it > pc_enqueued) { if ((e = pc_enqueue_iteration(it))) return e; }
            if ((e = pc_wait_slot(it, pc_base_seq + it))) return e;
            const volatile double* hp = h_pc + 8*it;
            err = hp[0] > 0.0 ? hp[2]/hp[0] : 0.0;
            if (!(hp[0] > 0.0) && it == 1) ++pc_zero_b_slices;      // sum |B| exactly 0 or under Engine::pc_floor: the loop leaves after this pass
        }
        // (iterations enqueued beyond `it` find their flag at 0 and do nothing; their sequence numbers are never posted)
        pc_spec_iters = it;
        pc_seq = pc_base_seq + std::max(it, pc_enqueued);
    }
    pc_err_sum += err;
    mark();   // b6
    checksum_slice();
    if ((e = fill_field_diagnostic(islice))) return e;
    mark();   // b7
    if (ions.present()) {
        // DoFieldIonization (Hipace.cpp:693-696) and the committing pushes of both species (:699-701): the decisions on the tiles'
        // gathered fields inside the ions' push (or k_ionize ahead of the per-particle push), the electron count back on the host,
        // then every electron -- the ones this slice has released included
        if ((e = push_ions(islice, comp_push, nullptr, true)) || (e = ionize_collect())) return e;
    }
    if ((e = species_advance(el, comp_push, 0))) return e;
    for (int k = 2; k < n_sp; ++k) { if ((e = species_advance(sp[k], comp_push, 0))) return e; }      // the further species
    insitu_beam(islice);
    if (moving && nbeam > 0) { if ((e = beam_push_moving(*this, islice))) return e; }
    if (!coll.empty()) { if ((e = collide_slice(islice))) return e; }      // doCoulombCollision (Hipace.cpp:711-712)
    mark();   // b8
    // ShiftSlices (fields/Fields.cpp:600-603): PCPrevIter <- Previous <- This for Bx By, Previous <- This for jx jy
    {   CompList dst{6, {HPS_PC_PIT_BX, HPS_PC_PIT_BY, HPS_PC_P_BX, HPS_PC_P_BY, HPS_PC_P_JX, HPS_PC_P_JY}};
        CompList src{6, {HPS_PC_P_BX, HPS_PC_P_BY, HPS_PC_BX, HPS_PC_BY, HPS_PC_JX, HPS_PC_JY}};
        copy_comps(slab, st, dst, src); }
    mark();   // b9
    HPS_HIP_CHECK(hipGetLastError());
    ++slices_done;
    return HPS_OK;
}

// hps_engine_slice_ready of a predictor-corrector slice
int Engine::pc_slice_ready () const
{
    // device-controlled loop: ready when the host's walk over the posted errors (solve_slice_pc_finish) would not wait --
    // an iteration that met the tolerance has been posted, or every iteration enqueued so far has
    if (!(pc_speculate && el.tiling && !moving && !ions.present() && !further()) || pc_islice < 0 || pc_enqueued <= 0) return 1;
    for (int it = 1; it <= pc_enqueued; ++it) {
        const volatile double* hp = h_pc + 8*it;
        const double seq = pc_base_seq + it;
        if (!(hp[1] == seq && hp[3] == seq && hp[5] == seq)) return 0;
        const double err = hp[0] > 0.0 ? hp[2]/hp[0] : 0.0;
        if (!(err > pc_tol) || it >= pc_max_iter) return 1;
    }
    return 1;
}

} // namespace hps

using namespace hps;

extern "C" int hps_engine_pc_stats (void* h, long* its, double* err_sum)
{
    Engine* E = static_cast<Engine*>(h);
    if (its) *its = E->pc_iterations;
    if (err_sum) *err_sum = E->pc_err_sum;
    return HPS_OK;
}
// slices on which the predictor-corrector loop saw sum |B| = 0 in its first pass -- exactly, or below the engine's rounding
// floor (Engine::pc_floor, HPS_PC_NOISE_FLOOR) -- and left after it (fields/Fields.cpp:1283)
extern "C" int hps_engine_pc_zero_b_slices (void* h, long* n)
{
    Engine* E = static_cast<Engine*>(h);
    HPS_REQUIRE(E && n, "hps_engine_pc_zero_b_slices: null argument");
    *n = E->pc_zero_b_slices;
    return HPS_OK;
}
