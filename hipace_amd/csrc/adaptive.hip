// adaptive.hip -- hipace.dt = adaptive: the host controller of the time step (utils/AdaptiveTimeStep.cpp; its calls in
// Hipace.cpp:270-282, 400-490).  Pure host code: the beam moments it needs come from the engine's partition kernel
// (beam.hip, k_beam_partition<true>) through hps_engine_beam_moments, so the controller runs, and is tested, without a GPU.
#include "common.h"
#include "expr.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <vector>

namespace hps {

int expr_check_named (const char* fn, const char* what, const hps_expr* p, int n_vars, int* depth);      // expr.hip

struct Adaptive {
    double nt = 20.0, dt_max = std::numeric_limits<double>::infinity(), thr = 2.0, tol = 4.0e-4;
    bool predict = true, phase = true; int substeps = 2000;
    double max_time = std::numeric_limits<double>::infinity();
    double c = 1.0, ep0 = 1.0, q_e = 1.0;
    double mq = 1.0; bool zero_charge = false;            // beam mass / charge; charge 0: the beam does not set dt
    double adaptive_density = 0.0;
    // species on the axis: |charge| * density, times f_r(0) f_t(z) of the profile -- or |charge * program(0, 0, z)|
    // hps_adaptive_set_density_expr: per species (0 plasma, 1 ion) its charge, whether the deck has it, and its density
    // programs with their positions (z_pos empty: one program); none: the species keeps |charge density| f_r(0) f_t(z)
    struct Species { bool present = false; double charge = 0.0, qn = 0.0; std::vector<std::vector<hps_expr_ins>> ins;
                     std::vector<std::vector<double>> consts; std::vector<double> z_pos; } species[HPS_MAX_PLASMA_SPECIES];
    int n_species = 2;                                     // hps_adaptive_add_species appends behind the deck's two
    std::vector<double> prof_r, prof_fr, prof_t, prof_ft;
    double dt = 0.0;                                       // Hipace::m_dt of this rank
    double min_uz_mq = std::numeric_limits<double>::max();
    double acc[4] = {0.0, 0.0, 0.0, 1e30};                 // sum w, sum w uz, sum w uz^2, min uz (uz/c)
    std::vector<std::array<double, 4>> accs;               // ... per beam, of the calls with several beams (m_timestep_data[ibeam])
    double next_time = 0.0;

    // MultiPlasma::maxChargeDensity(z)
    double rho_max (double z) const {
        double r = std::fabs(adaptive_density*q_e);
        const double f = table_value(prof_r.data(), prof_fr.data(), (int)prof_r.size(), 0.0)*
                         table_value(prof_t.data(), prof_ft.data(), (int)prof_t.size(), z);
        for (const Species& S : species) {
            if (!S.present) continue;
            if (S.ins.empty()) { r = std::max(r, std::fabs(S.qn*f)); continue; }
            // UpdateDensityFunction(z): the first entry with z_pos >= z, the last one beyond the table
            size_t k = 0;
            if (!S.z_pos.empty()) k = std::min<size_t>(std::lower_bound(S.z_pos.begin(), S.z_pos.end(), z) - S.z_pos.begin(), S.z_pos.size() - 1);
            ExprHostStack st;
            const ExprXyz v{0.0, 0.0, z};
            r = std::max(r, std::fabs(S.charge*expr_run(S.ins[k].data(), (int)S.ins[k].size(), S.consts[k].data(), v, st)));
        }
        return r;
    }
    void reset_moments () { acc[0] = acc[1] = acc[2] = 0.0; acc[3] = 1e30; for (auto& a : accs) a = {0.0, 0.0, 0.0, 1e30}; }
    void size_beams (int n) { if ((int)accs.size() != n) accs.assign((size_t)n, std::array<double, 4>{0.0, 0.0, 0.0, 1e30}); }

    // CalculateFromMinUz over several beams (AdaptiveTimeStep.cpp:177-258): every beam's dt from its own moments and m/q, a
    // beam of charge 0 skipped; dt = the smallest, then dt_max; min_uz_mq = the smallest over the beams.  One beam with the
    // deck's m/q: from_min_uz, statement by statement.
    int from_min_uz_beams (int n, const double* charge, const double* mass, double t, int nstages) {
        double dt_min = std::numeric_limits<double>::max(), mq_min = std::numeric_limits<double>::max();
        for (int b = 0; b < n; ++b) {
            double out = dt;
            if (charge[b] != 0.0) {
                const double* a = accs[(size_t)b].data();
                const double mq_b = (mass[b] != 0.0 ? mass[b] : 1.0)/charge[b];
                HPS_REQUIRE(a[0] != 0.0, "hps_adaptive: the sum of all weights is 0 (no beam particles)");
                const double mean = a[1]/a[0];
                const double sigma = std::sqrt(std::fabs(a[2]/a[0] - mean*mean));
                double chosen = std::min(std::max(mean - 4.0*sigma, a[3]), 1.0e30);
                chosen = std::max(chosen, thr);
                mq_min = std::min(mq_min, std::fabs(chosen*mq_b));
                double new_dt = dt, time = t, min_uz = chosen;
                const int niter = predict ? std::max(nstages, 1) : 1;
                for (int i = 0; i < niter; ++i) {
                    const double rho = rho_max(c*time);
                    HPS_REQUIRE(rho > 0.0, "hps_adaptive: the adaptive time step needs a plasma density > 0 (plasmas.adaptive_density)");
                    min_uz = std::max(min_uz, 0.001*thr);
                    const double omega_b = std::sqrt(rho/(2.0*std::fabs(min_uz*mq_b)*ep0));
                    new_dt = 2.0*M_PI/omega_b/nt;
                    time += new_dt;
                    if (min_uz > thr) out = new_dt;
                }
            }
            dt_min = std::min(dt_min, out);
        }
        min_uz_mq = mq_min;
        dt = std::min(dt_min, dt_max);
        return HPS_OK;
    }

    // CalculateFromMinUz
    int from_min_uz (double t, int nstages) {
        if (zero_charge) { min_uz_mq = std::numeric_limits<double>::max(); dt = std::min(dt, dt_max); return HPS_OK; }
        HPS_REQUIRE(acc[0] != 0.0, "hps_adaptive: the sum of all weights is 0 (no beam particles)");
        const double mean = acc[1]/acc[0];
        const double sigma = std::sqrt(std::fabs(acc[2]/acc[0] - mean*mean));
        double chosen = std::min(std::max(mean - 4.0*sigma, acc[3]), 1.0e30);
        chosen = std::max(chosen, thr);
        min_uz_mq = std::fabs(chosen*mq);
        double new_dt = dt, out = dt, time = t, min_uz = chosen;
        const int niter = predict ? std::max(nstages, 1) : 1;
        for (int i = 0; i < niter; ++i) {
            const double rho = rho_max(c*time);
            HPS_REQUIRE(rho > 0.0, "hps_adaptive: the adaptive time step needs a plasma density > 0 (plasmas.adaptive_density)");
            min_uz = std::max(min_uz, 0.001*thr);
            const double omega_b = std::sqrt(rho/(2.0*std::fabs(min_uz*mq)*ep0));
            new_dt = 2.0*M_PI/omega_b/nt;
            time += new_dt;
            if (min_uz > thr) out = new_dt;
        }
        dt = std::min(out, dt_max);
        return HPS_OK;
    }

    // CalculateFromDensity
    void from_density (double t) {
        reset_moments();
        if (!phase) return;
        const double dt_sub = dt/substeps;
        double adv = 0.0, adv0 = 0.0;
        const double omgb0 = std::sqrt(rho_max(c*t)/(2.0*min_uz_mq*ep0));
        for (int i = 0; i < substeps; ++i) {
            const double omgb = std::sqrt(rho_max(c*(t + i*dt_sub))/(2.0*min_uz_mq*ep0));
            adv += omgb*dt_sub;
            adv0 += omgb0*dt_sub;
            if (std::fabs(adv - adv0) > 2.0*M_PI*tol/nt) { dt = i*dt_sub; return; }
        }
    }
};

} // namespace hps

using namespace hps;

extern "C" int hps_adaptive_create (const hps_deck* d, void** handle)
{
    HPS_REQUIRE(d && handle, "hps_adaptive_create: null argument");
    HPS_REQUIRE(d->dt_adaptive, "hps_adaptive_create: the deck has no adaptive time step (dt_adaptive)");
    HPS_REQUIRE(!d->laser_on, "hps_adaptive_create: hipace.dt = adaptive cannot be used with a laser (Hipace.cpp:408)");
    HPS_REQUIRE(d->nt_per_betatron >= 0.0 && d->dt_max >= 0.0 && d->adaptive_threshold_uz >= 0.0 && d->adaptive_phase_tolerance >= 0.0 &&
                d->adaptive_phase_substeps >= 0, "hps_adaptive_create: negative setting");
    Adaptive* A = new Adaptive;
    if (d->nt_per_betatron > 0.0) A->nt = d->nt_per_betatron;
    if (d->dt_max > 0.0) A->dt_max = d->dt_max;
    if (d->adaptive_threshold_uz > 0.0) A->thr = d->adaptive_threshold_uz;
    if (d->adaptive_phase_tolerance > 0.0) A->tol = d->adaptive_phase_tolerance;
    if (d->adaptive_phase_substeps > 0) A->substeps = d->adaptive_phase_substeps;
    A->predict = !d->adaptive_no_predict_step;
    A->phase = !d->adaptive_no_phase_control;
    if (d->max_time != 0.0) A->max_time = d->max_time;
    if (d->si_units) { A->c = 299792458.0; A->ep0 = 8.8541878128e-12; A->q_e = 1.602176634e-19; }      // utils/Constants.H:15-24
    const double mass = d->beam_mass != 0.0 ? d->beam_mass : 1.0;
    A->zero_charge = (d->beam_charge == 0.0);
    A->mq = A->zero_charge ? 0.0 : mass/d->beam_charge;
    A->adaptive_density = d->adaptive_density;
    if (d->plasma_ppc[0]*d->plasma_ppc[1] > 0) { A->species[0].present = true; A->species[0].charge = d->plasma_charge; A->species[0].qn = d->plasma_charge*d->plasma_density; }
    if (d->ion_on) { A->species[1].present = true; A->species[1].charge = d->ion_charge; A->species[1].qn = d->ion_charge*d->ion_density; }
    *handle = A;
    return HPS_OK;
}

extern "C" int hps_adaptive_set_density_profile (void* h, int nr, const double* r_host, const double* fr_host, int nt,
                                                 const double* ct_host, const double* ft_host)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && nr >= 0 && nt >= 0 && (nr == 0 || (r_host && fr_host)) && (nt == 0 || (ct_host && ft_host)),
                "hps_adaptive_set_density_profile: bad argument");
    for (int k = 1; k < nr; ++k) HPS_REQUIRE(r_host[k] > r_host[k - 1], "hps_adaptive_set_density_profile: r must increase");
    for (int k = 1; k < nt; ++k) HPS_REQUIRE(ct_host[k] > ct_host[k - 1], "hps_adaptive_set_density_profile: ct must increase");
    A->prof_r.assign(r_host, r_host + nr); A->prof_fr.assign(fr_host, fr_host + nr);
    A->prof_t.assign(ct_host, ct_host + nt); A->prof_ft.assign(ft_host, ft_host + nt);
    return HPS_OK;
}

extern "C" int hps_adaptive_set_density_expr (void* h, int species, int n_progs, const hps_expr* progs, const double* z_pos)
{
    static const char* const fn = "hps_adaptive_set_density_expr";
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A, std::string(fn) + ": null handle");
    HPS_REQUIRE(species >= 0 && species < A->n_species, std::string(fn) + ": species must be 0 (plasma), 1 (ion) or the index of an added species");
    HPS_REQUIRE(A->species[species].present, std::string(fn) + ": the deck does not have this species (no plasma, or no ion species)");
    HPS_REQUIRE(n_progs >= 1 && progs, std::string(fn) + ": n_progs must be >= 1 (at least one program)");
    HPS_REQUIRE(n_progs == 1 || z_pos, std::string(fn) + ": several programs need their positions (z_pos)");
    for (int k = 0; z_pos && k < n_progs; ++k)
        HPS_REQUIRE(std::isfinite(z_pos[k]) && (k == 0 || z_pos[k] > z_pos[k - 1]), std::string(fn) + ": the positions of the density table must be finite and strictly ascending");
    for (int k = 0; k < n_progs; ++k) {
        const std::string what = n_progs > 1 ? "entry " + std::to_string(k) + ": " : std::string();
        if (int e = expr_check_named(fn, what.c_str(), &progs[k], 3, nullptr)) return e;
    }
    Adaptive::Species& S = A->species[species];
    S.ins.clear(); S.consts.clear(); S.z_pos.clear();
    for (int k = 0; k < n_progs; ++k) {
        S.ins.emplace_back(progs[k].ins, progs[k].ins + progs[k].n_ins);
        S.consts.emplace_back(progs[k].consts, progs[k].consts + progs[k].n_const);
        if (S.consts.back().empty()) S.consts.back().push_back(0.0);
    }
    if (z_pos) S.z_pos.assign(z_pos, z_pos + n_progs);
    return HPS_OK;
}

extern "C" int hps_adaptive_add_species (void* h, double charge, double density)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    if (!A || A->n_species >= HPS_MAX_PLASMA_SPECIES || !std::isfinite(charge) || !std::isfinite(density)) {
        set_error("hps_adaptive_add_species: null handle, more than HPS_MAX_PLASMA_SPECIES species, or a charge / density that is not finite");
        return -1;
    }
    Adaptive::Species& S = A->species[A->n_species];
    S.present = true; S.charge = charge; S.qn = charge*density;
    return A->n_species++;
}

extern "C" int hps_adaptive_rho_max (void* h, double z, double* out)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && out, "hps_adaptive_rho_max: null argument");
    *out = A->rho_max(z);
    return HPS_OK;
}

extern "C" int hps_adaptive_initial_dt (void* h, double uz_mean, double uz_std, int nstages, double* dt)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && dt, "hps_adaptive_initial_dt: null argument");
    // GatherMinUzSlice(beams, true): the estimate of a beam that is not read from a file
    A->acc[0] = 1.0; A->acc[1] = uz_mean; A->acc[2] = uz_mean*uz_mean + uz_std*uz_std; A->acc[3] = uz_mean - 4.0*uz_std;
    HPS_REQUIRE(nstages >= 1, "hps_adaptive_initial_dt: nstages must be >= 1");
    if (int e = A->from_min_uz(0.0, nstages)) return e;      // (predicted over m_numprocs steps, as every later dt)
    A->from_density(0.0);
    *dt = A->dt;
    return HPS_OK;
}

extern "C" int hps_adaptive_before_step (void* h, double t, double* dt)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && dt, "hps_adaptive_before_step: null argument");
    HPS_REQUIRE(!std::isnan(t), "hps_adaptive_before_step: t is NaN");
    if (t == std::numeric_limits<double>::infinity()) {       // a dropped step: nothing to do, the sentinel travels on
        A->reset_moments(); A->next_time = t; *dt = 0.0; return HPS_OK;
    }
    A->from_density(t);
    const double tm = A->max_time;
    if (t == tm) {
        A->dt = 0.0;
        A->next_time = std::numeric_limits<double>::infinity();
    } else if ((t + A->dt >= tm && t < tm) || (t + A->dt <= tm && t > tm)) {
        A->dt = tm - t;
        A->next_time = tm;
    } else {
        A->next_time = t + A->dt;
    }
    *dt = A->dt;
    return HPS_OK;
}

extern "C" int hps_adaptive_next_time (void* h, double* t_next)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && t_next, "hps_adaptive_next_time: null argument");
    *t_next = A->next_time;
    return HPS_OK;
}

extern "C" int hps_adaptive_after_step (void* h, const double* m, double t, int nstages, double* dt)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    HPS_REQUIRE(A && m && dt && nstages >= 1, "hps_adaptive_after_step: bad argument");
    // the slices' GatherMinUzSlice(beams, false) on top of what CalculateFromDensity reset
    A->acc[0] += m[0]; A->acc[1] += m[1]; A->acc[2] += m[2]; A->acc[3] = std::min(A->acc[3], m[3]);
    if (int e = A->from_min_uz(t, nstages)) return e;
    *dt = A->dt;
    return HPS_OK;
}

static int beams_args_ok (const char* fn, const Adaptive* A, int n, const void* a, const void* b, const double* charge, const double* mass, const double* dt, int nstages)
{
    HPS_REQUIRE(A && a && b && charge && mass && dt, std::string(fn) + ": null argument");
    HPS_REQUIRE(n >= 1 && nstages >= 1, std::string(fn) + ": n and nstages must be >= 1");
    for (int k = 0; k < n; ++k) HPS_REQUIRE(std::isfinite(charge[k]) && std::isfinite(mass[k]), std::string(fn) + ": charge and mass must be finite");
    return HPS_OK;
}

extern "C" int hps_adaptive_initial_dt_beams (void* h, int n, const double* uz_mean, const double* uz_std, const double* charge,
                                              const double* mass, int nstages, double* dt)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    if (int e = beams_args_ok("hps_adaptive_initial_dt_beams", A, n, uz_mean, uz_std, charge, mass, dt, nstages)) return e;
    A->size_beams(n);
    for (int b = 0; b < n; ++b)      // GatherMinUzSlice(beams, true), per beam
        A->accs[(size_t)b] = {1.0, uz_mean[b], uz_mean[b]*uz_mean[b] + uz_std[b]*uz_std[b], uz_mean[b] - 4.0*uz_std[b]};
    if (int e = A->from_min_uz_beams(n, charge, mass, 0.0, nstages)) return e;
    A->from_density(0.0);
    *dt = A->dt;
    return HPS_OK;
}

extern "C" int hps_adaptive_after_step_beams (void* h, int n, const double* m, const double* charge, const double* mass, double t,
                                              int nstages, double* dt)
{
    Adaptive* A = static_cast<Adaptive*>(h);
    if (int e = beams_args_ok("hps_adaptive_after_step_beams", A, n, m, m, charge, mass, dt, nstages)) return e;
    A->size_beams(n);
    for (int b = 0; b < n; ++b) {
        std::array<double, 4>& a = A->accs[(size_t)b];
        a[0] += m[4*b]; a[1] += m[4*b + 1]; a[2] += m[4*b + 2]; a[3] = std::min(a[3], m[4*b + 3]);
    }
    if (int e = A->from_min_uz_beams(n, charge, mass, t, nstages)) return e;
    *dt = A->dt;
    return HPS_OK;
}

extern "C" int hps_adaptive_destroy (void* h)
{
    delete static_cast<Adaptive*>(h);
    return HPS_OK;
}
