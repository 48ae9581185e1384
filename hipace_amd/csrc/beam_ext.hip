// beam_ext.hip -- beams.external_E(x,y,z,t) / beams.external_B(x,y,z,t) as expression programs: the setter that
// checks the programs and packs them into one device image, and the launch of k_beam_push<ORDER, true, MULTI> (beam_push.h).
// Built with -mllvm -disable-machine-licm (Makefile): left on, the pass hoists the literal constants of every inlined
// transcendental function out of the interpreter's loop and holds them in registers across it (k_expr_eval: 244 VGPRs
// against 36; the order-3 push beyond 512 registers, into scratch).
#include "common.h"
#include "engine.h"
#include "beam_push.h"

namespace hps {

int beam_push_launch_ext (Engine& E, const SlabView& f, int p, int cPsi, int cEz, int cBx, int cBy, int cBz, const BeamPushConsts& k, dim3 grid)
{
    const BeamExtArgs<true> x{E.bext.image.ins(), E.bext.image.consts(), E.step_time};
    const dim3 block(256);
    const size_t lds = expr_lds_bytes(E.bext.depth, 256);
    if (E.multi_beam()) {
        const BeamMultiArgs<true> m{E.d_bsp_tab, E.n_beam_species()};
#define CALL(O) hipLaunchKernelGGL((k_beam_push<O, true, true>), grid, block, lds, E.st, f, E.bm, E.d_B, p, cPsi, cEz, cBx, cBy, cBz, k, x, m)
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    } else {
#define CALL(O) hipLaunchKernelGGL((k_beam_push<O, true, false>), grid, block, lds, E.st, f, E.bm, E.d_B, p, cPsi, cEz, cBx, cBy, cBz, k, x, BeamMultiArgs<false>{})
        HPS_BEAM_ORDER(E.d.order, CALL)
#undef CALL
    }
    E.beam_launched |= beam_push_bit(std::min(std::max(E.d.order, 0), 3), true, E.multi_beam());
    HPS_HIP_CHECK(hipGetLastError());
    return HPS_OK;
}

// hps_engine_set_beam_external_fields: every component is checked before anything changes
int Engine::set_beam_external_fields (const hps_expr* E3, const hps_expr* B3)
{
    static const char* const fn = "hps_engine_set_beam_external_fields";
    static const char* const name[6] = {"E[0]: ", "E[1]: ", "E[2]: ", "B[0]: ", "B[1]: ", "B[2]: "};
    HPS_REQUIRE(!step_begun, std::string(fn) + ": call before the first hps_engine_begin_step");
    const hps_expr* comp[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int depth = 0; bool any = false;
    for (int q = 0; q < 6; ++q) {
        const hps_expr* src = q < 3 ? E3 : B3;
        if (!src || src[q % 3].n_ins == 0) continue;
        int dq = 0;
        if (int e = expr_check_named(fn, name[q], &src[q % 3], 4, &dq)) return e;
        if (expr_is_zero(src[q % 3])) continue;
        comp[q] = &src[q % 3]; depth = std::max(depth, dq); any = true;
    }
    bext = BeamExt{};
    if (!any || !moving) return HPS_OK;      // hipace.dt = 0: the beam is never pushed, the programs have no effect
    ExprImage image(6);
    for (int q = 0; q < 6; ++q)
        if (comp[q]) image.slot(q) = hps_expr_ins{image.add(*comp[q]), comp[q]->n_ins};
    if (int e = image.upload()) return e;
    bext.image = std::move(image);
    bext.depth = depth; bext.on = true;
    return HPS_OK;
}

} // namespace hps

extern "C" int hps_engine_set_beam_external_fields (void* h, const hps_expr* E3, const hps_expr* B3)
{
    HPS_REQUIRE(h, "hps_engine_set_beam_external_fields: null engine");
    return static_cast<hps::Engine*>(h)->set_beam_external_fields(E3, B3);
}
