// multigrid.h -- what the rest of the library calls of the two multigrid solvers beside their C ABI (include/hpslice.h): the
// explicit solver's Bx/By solve in two halves (multigrid.hip, called by the slice schedule of engine.hip) and the envelope
// solver's handle (multigrid2.hip, called by laser.hip).  Both solver files include it, so every definition is checked against
// the one declaration here.
#ifndef HPS_MULTIGRID_H_
#define HPS_MULTIGRID_H_

#include "common.h"
#include "mg_gate.h"
#include "slab_ops.h"

namespace hps {

// ---- multigrid.hip.  mg_handle is what hps_mg_create returned.
// hps_mg_solve1 in two halves: begin enqueues the speculated V-cycles and the post of their norms; finish waits for the
// norms.  Kernels enqueued between them are gated on mg_gate_after_enqueued (they run iff the word is 1: the solve is over)
int mg_solve1_begin (void* mg_handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, double tol_rel, double tol_abs,
                     int max_iters, hipStream_t st);
// the coefficient hierarchy of the NEXT mg_solve1_begin (same slab, same components, same max_iters) on stream `st`, which
// the caller orders: behind whatever writes the coefficient, ahead of mg_solve1_begin's stream
int mg_solve1_prepare (void* mg_handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, int max_iters, hipStream_t st);
// ... in one launch with the -grad Psi / Sx, Sy pass of the slab (k_hierarchy_gradpsi); *done = false if this grid's
// hierarchy needs more than that launch (then nothing has been enqueued)
int mg_solve1_prepare_with (void* mg_handle, hps_slab s, int sol_comp, int rhs_comp, int acf_comp, int max_iters, SlabView f, GradPsiSxSy ga,
                            hipStream_t st, bool* done);
// a hierarchy enqueued by mg_solve1_prepare* that no mg_solve1_begin followed (the caller failed in between) is dropped
// (and so is a pass handed to mg_ride_shift_init)
void mg_solve1_forget_hierarchy (void* mg_handle);
// have the norms of the batch enqueued by mg_solve1_begin arrived (mg_solve1_finish would not wait)?
bool mg_solve1_ready (void* mg_handle);
// *extra: did finish enqueue further V-cycles (then kernels gated on mg_gate_after_enqueued have not run)?
int mg_solve1_finish (void* mg_handle, int* iters_out, double* resnorm_out, int* extra, hipStream_t st);
// the slab's shift / zero pass for the next slice as guest workgroups of the next mg_solve1_begin's first lower V; false: this
// grid's lower V takes no guests (nothing will be done)
bool mg_ride_shift_init (void* mg_handle, const ShiftInit& pass);
const int* mg_gate_after_enqueued (void* mg_handle);
// mg_defer_post ahead of mg_solve1_begin: the post of the first batch's norms is not launched but handed out by
// mg_take_deferred_post -- the caller MUST then enqueue, next on the same stream, a kernel that performs it, or the solve's
// finish never sees its norms.  (Without mg_defer_post the post has been launched: mg_take_deferred_post returns false.)
void mg_defer_post (void* mg_handle);
bool mg_take_deferred_post (void* mg_handle, MgPost* out);
// a header slot of the norm buffer for the caller's own device counters: they reach the host with the read-back every solve
// does anyway
void mg_rider (void* mg_handle, int** dev_words, const int** host_words);

// ---- multigrid2.hip: hps_mg2_create / _solve2 / _destroy without the C ABI's argument checks, on the caller's stream
int mg2_create_internal (int nx, int ny, double dx, double dy, void** h);
int mg2_solve_internal (void* h, double* sol, const double* rhs, const double* ar, const double* ai, double tol_rel, double tol_abs,
                        int maxiter, int* iters, hipStream_t st);
void mg2_destroy_internal (void* h);

} // namespace hps
#endif
