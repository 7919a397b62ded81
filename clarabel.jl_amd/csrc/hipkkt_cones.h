// The cone state of a handle: what hipkkt_set_cone_types[_ex] registered, the device tables of the scaling kernels (scaling.hip) and
// what the step entry points keep resident (hipkkt_step.cpp; step.hip, step_cone3.hip, step_genpow.hip, step_psd.hip, step_psd_large.hip,
// barrier_psd.hip).
// Written by hipkkt_cones.cpp (registration, scaling) and hipkkt_step.cpp (enables, step); record layouts: cone_layout.h.
#pragma once
#include <cstdint>
#include <vector>

namespace hipkkt_host {

// What the registered kinds qualify for.  The classes exclude one another:
//   Symmetric  all kinds in 0..2 (Zero / Nonnegative / SecondOrder)
//   Cone3      an _ex registration, kinds in {0, 1, 2, 4, 5}, at least one Exponential / Power cone
//   GenPow     an _ex registration, kinds in {0, 1, 2, 4, 5, 6}, at least one Generalized Power cone
//   Psd        kinds in 0..3, at least one PSD triangle cone (the sides are checked at the enable)
//   Mixed      an _ex registration, kinds in 0..6, at least one PSD triangle cone and at least one Exponential / Power / Generalized
//              Power cone (the sides are checked at the enable)
enum class ConeClass { Other, Symmetric, Cone3, GenPow, Psd, Mixed };

// Which cones the step entry points serve.  A registration sets Symmetric for the class Symmetric and Off otherwise; the enables
// hipkkt_step_enable_cone3 / _genpow / _psd / _psd_large / _mixed move a handle of their class to Cone3 / GenPow / Psd / Mixed and back
// to Off.
enum class StepMode { Off, Symmetric, Cone3, GenPow, Psd, Mixed };

struct ConeState {
    // what the last hipkkt_set_cone_types[_ex] established (host side)
    struct Registration {
        bool ready = false;                                // the call validated and uploaded its tables
        ConeClass cls = ConeClass::Other;
        int nsoc = 0;                                      // ALL second-order cones (sparse and dense), cone order
        std::vector<int64_t> psd_hs, psd_n, psd_row;       // per PSD cone: first Hs entry, matrix dimension, first row
        int64_t psd_total = 0, psd_lam_total = 0;          // sum of n * n, sum of n
        bool nonsym = false;                               // it named an Exponential / Power / GenPower cone
        int nexp = 0, npow = 0, ngenpow = 0;
        int64_t nonsym_len = 0;                            // doubles of their output vector (hipkkt_get_nonsym_len)
        int64_t degree = 0;                                // Nonnegative rows + second-order cones + PSD sides (the default start's target)
    } reg;
    // device tables and results of the scaling: allocated on the first use, re-used by later calls while large enough (cap_*)
    struct Tables {
        int64_t cap_socdesc = 0, cap_psd = 0;
        signed char *kind = nullptr;                       // per row
        int64_t *rowhs = nullptr, *socdesc = nullptr;
        double *sz = nullptr, *wl = nullptr, *eta = nullptr;   // (s, z) | (w, lambda) | eta of the last scaling
        double *R = nullptr, *W = nullptr;
        int *fail = nullptr;
        // the non-symmetric cones: three-row cones [Exponential | Power], GenPower descriptors, [map.q | map.r | map.p | map.D] per cone
        int64_t cap3 = 0, cap_gp = 0, cap_gpalpha = 0, cap_gpidx = 0, cap_out = 0;
        int64_t *row0 = nullptr, *hs0 = nullptr, *out0 = nullptr;
        double *alpha = nullptr;
        int *trips = nullptr;                              // Newton steps of the last update per table entry (debug_dump 23)
        int64_t *gpdesc = nullptr, *gpidx = nullptr;
        double *gpalpha = nullptr, *nsout = nullptr;
        // hipkkt_step_enable_psd / _mixed: the cone table, the resident factors of the last scaling, the staged [Rinv (psd_total) | lambda]
        int64_t cap_psd_cones = 0, cap_psd_mat = 0, cap_psd_lam = 0;
        int64_t *psdtab = nullptr;
        double *psd_rinv = nullptr, *psd_lam = nullptr, *psd_stage = nullptr;
        int *psd_bad = nullptr;                            // per PSD cone: its device-side scaling failed (scaling_psd.hip)
        int64_t *psd_hs0 = nullptr;                        // per PSD cone: its first Hs entry (start.hip)
        // hipkkt_step_enable_psd_large: the indices into psdtab of the cones step_psd_large.hip serves, their matrix workspace
        int64_t cap_psd_large = 0;
        int *psd_lidx = nullptr;
        double *psd_ws = nullptr;
    } tab;
    // what the step entry points work on between the calls
    struct Step {
        StepMode mode = StepMode::Off;
        bool scaled = false;                               // the last hipkkt_update_scaling[_dev] since the registration / enable succeeded
        bool have_step = false;                            // [dx | dz | ds] of a fused step call is resident
        bool psd_fresh = false;                            // factors staged since the last scaling
        bool psd_scaling = false;                          // hipkkt_psd_scaling_enable: a scaling without psd_R computes the factors
        bool psd_resident = false;                         // a scaling since the enable left (R, Rinv, lambda) resident (hipkkt_psd_get_factors)
        int psd_nlarge = 0, psd_lmin = 65, psd_lmax = 0;   // hipkkt_step_enable_psd_large / _mixed_large: cones of side psd_lmin .. psd_lmax go to step_psd_large.hip
        bool psd_large_enabled = false;                    // the handle is in PSD step mode through hipkkt_step_enable_psd_large
        bool mixed_large_enabled = false;                  // the handle is in Mixed step mode through hipkkt_step_enable_mixed_large
        bool psd_scaling_large = false;                    // hipkkt_psd_scaling_enable_large: psd_scaling for every side, those cones through scaling_psd_large.hip
        bool start_psd_large = false;                      // hipkkt_step_default_start_enable_psd_large: the default start serves sides above 64
        double ls_step = 0.0, ls_amin = 0.0;               // linesearch_backtrack_step, min_terminate_step_length (Cone3 / GenPow / Mixed)
        int ls_trips = 0;                                  // bound of the backtracking loop: ceil(log amin / log step) + 2
        double mu = 0.0;                                   // mu of the last hipkkt_update_scaling_ex[_dev] (mul_Hs of the GenPower cones)
        double *step = nullptr;                            // [dx | dz | ds] of the last fused step call
        double *in = nullptr, *work = nullptr;             // [rhs.x | workz | variables.x]; four work vectors of length m
        double *part = nullptr, *out = nullptr;            // partial results of the step length / the norms; results (cone_layout.h kStOut*)
        double *eq = nullptr;                              // [d | e | dinv | einv] (hipkkt_set_equilibration)
        double *bar = nullptr;                             // work buffer of the barrier (step3_barrier_doubles)
        double *start = nullptr;                           // partials and decision records of the default start (start_work_doubles)
    } step;
};

}  // namespace hipkkt_host
