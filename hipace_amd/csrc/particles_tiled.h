// particles_tiled.h -- the host entry points of the LDS-tile particle kernels (particles_tiled.hip): the one declaration of
// each, default arguments included, for particles_tiled.hip itself and for every caller (through engine.h).
#ifndef HPS_PARTICLES_TILED_H_
#define HPS_PARTICLES_TILED_H_

#include "common.h"
#include "tiling.h"
#include "mg_gate.h"
#include "particle_math.h"
#include "beam_deposit.h"

namespace hps {

int deposit_current_tiled (const hps_slab& slab, const hps_plasma& pl, const hps_geom& g, const int comp[6], double charge,
                           double mass, int order, double max_qsa, int can_ionize, int* n_qsa, Tiling* T, int* n_fallback,
                           hipStream_t st, int aabs_comp = -1, const int* tile_flag = nullptr, TailWork tw = TailWork{},
                           const BeamPairWork* beam = nullptr, const int* go = nullptr, bool valid_by_w = false);
int explicit_deposit_tiled (const hps_slab& slab, const hps_plasma& pl, const hps_geom& g, const int cache[4], const int depos[2],
                            double charge, double mass, int order, int dtype, int can_ionize, Tiling* T, int* n_fallback,
                            hipStream_t st, int aabs_comp = -1, const int* tile_flag = nullptr, TailWork tw = TailWork{}, bool valid_by_w = false);
int advance_plasma_tiled (const hps_slab& slab, const hps_plasma& pl, const hps_geom& g, const int comp[5], double charge,
                          double mass, int order, int temp_slice, int n_subcycles, int can_ionize, Tiling* T,
                          int* n_fallback, hipStream_t st, int aabs_comp = -1, const IonArgs* ion = nullptr, const int* go = nullptr,
                          TailWork tw = TailWork{}, const MgPost* post = nullptr);
int advance_deposit_tiled (const hps_slab& slab, const hps_plasma& pl, const hps_geom& g, const int comp[5], const int dep_comp[6],
                           double charge, double mass, int order, int n_subcycles, double max_qsa, int* n_qsa, Tiling* T,
                           int* n_fallback, hipStream_t st);

} // namespace hps
#endif
