// particles_tiled.h -- the host entry points of the LDS-tile particle kernels (particles_tiled.hip): the one declaration of
// each and of the launch record they take, for particles_tiled.hip itself and for every caller (through engine.h).
#ifndef HPS_PARTICLES_TILED_H_
#define HPS_PARTICLES_TILED_H_

#include "common.h"
#include "tiling.h"
#include "mg_gate.h"
#include "particle_math.h"
#include "beam_deposit.h"

namespace hps {

// The launch record ("The launch record"): who launches, on which sheet, and what this call alone sets.
// The engine-wide part, the same for every launch of an engine (Engine::tile_env; the C entries build one from their arguments):
struct TileEnv { const hps_slab& slab; const hps_geom& g; int order; hipStream_t st; int* n_fallback; int aabs_comp; };
// ... one species' sheet (Engine::Species::sheet):
struct TileSheet { const hps_plasma& pl; double charge, mass; int can_ionize; Tiling* T; };
// ... and the per-call part of each operator: the component lists it cannot do without are its constructor's arguments, a
// caller names what else it sets, the rest keeps its initialiser
// (go: the gate word of the launch, null: ungated; tw: the workgroups of the sheet's tail behind the tile-sorted body)
struct DepositArgs { explicit DepositArgs (const int comp6[6]) : comp(comp6) {}
                     const int* comp;
                     double max_qsa = 0.0; int* n_qsa = nullptr; const int* tile_flag = nullptr; TailWork tw{};
                     const BeamPairWork* beam = nullptr; const int* go = nullptr; bool valid_by_w = false; };
struct ExplicitArgs { ExplicitArgs (const int cache4[4], const int depos2[2]) : cache(cache4), depos(depos2) {}
                      const int *cache, *depos;
                      int dtype = 2; const int* tile_flag = nullptr; TailWork tw{}; bool valid_by_w = false; };
struct PushArgs { explicit PushArgs (const int comp5[5]) : comp(comp5) {}
                  const int* comp;
                  int temp_slice = 0, n_subcycles = 1; const IonArgs* ion = nullptr; const int* go = nullptr; TailWork tw{};
                  const MgPost* post = nullptr; };

int deposit_current_tiled (const TileEnv& e, const TileSheet& s, const DepositArgs& a);
int explicit_deposit_tiled (const TileEnv& e, const TileSheet& s, const ExplicitArgs& a);
int advance_plasma_tiled (const TileEnv& e, const TileSheet& s, const PushArgs& a);
int advance_deposit_tiled (const TileEnv& e, const TileSheet& s, const int comp[5], const int dep_comp[6], int n_subcycles,
                           double max_qsa, int* n_qsa);

} // namespace hps
#endif
