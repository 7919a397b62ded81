// The cone registration and the scaling (N1) behind the C ABI: hipkkt_set_cone_types[_ex], hipkkt_update_scaling[_ex][_dev],
// hipkkt_get_nonsym_len.  They fill the handle's ConeState (hipkkt_cones.h) that the step entry points of hipkkt_step.cpp work on; the
// records they encode for the kernels are laid out in cone_layout.h.
#include "hipkkt_internal.h"

// the class of a registration (hipkkt_cones.h ConeClass), one pass over its kinds
static ConeClass cone_class(int64_t ncones, const int32_t *kinds, bool ex) {
    bool any3 = false, anygp = false, anypsd = false;
    for (int64_t c = 0; c < ncones; c++) {
        const int32_t k = kinds[c];
        if (k >= 0 && k <= 2) continue;
        if (k == 3) anypsd = true;
        else if (k == HIPKKT_CONE_EXP || k == HIPKKT_CONE_POW) any3 = true;
        else if (k == HIPKKT_CONE_GENPOW) anygp = true;
        else return ConeClass::Other;
    }
    if (!any3 && !anygp) return anypsd ? ConeClass::Psd : ConeClass::Symmetric;
    if (!ex) return ConeClass::Other;
    if (anypsd) return ConeClass::Mixed;
    return anygp ? ConeClass::GenPow : ConeClass::Cone3;
}

extern "C" {

// ---- N1: update_scaling! + get_Hs! of the symmetric cones on the device (scaling.hip) ---------------------------------
// kinds[c]: 0 ZeroCone, 1 NonnegativeCone, 2 SecondOrderCone, 3 PSDTriangleCone, anything else = a cone whose block the
// caller keeps setting through hipkkt_set_hs / hipkkt_set_genpow (ref: the SupportedCone types of cone_types.jl / cone_api.py)
// ex: hipkkt_set_cone_types_ex -- kinds 4 Exponential, 5 Power, 6 GenPower are checked and get their tables (scaling.hip); alpha = the
// exponents of the Power / GenPower cones concatenated in cone order
static int32_t set_cone_types_impl(hipkkt_handle h, int64_t ncones, const int32_t *kinds, bool ex, int64_t nalpha, const double *alpha) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!S->l1 || ncones != (int64_t)S->cone_numel.size() || (ncones && !kinds)) { S->err = "set_cone_types: not an L1 handle / wrong number of cones"; return HIPKKT_ERR_ARGUMENT; }
    if (ex && (nalpha < 0 || (nalpha && !alpha))) { S->err = "set_cone_types_ex: null alpha"; return HIPKKT_ERR_ARGUMENT; }
    const int64_t m = S->img.m;
    C.reg.ready = false;          // until this call has validated and uploaded its tables
    C.reg.nonsym = false;
    C.step.scaled = false;
    C.step.psd_fresh = false;
    C.step.psd_scaling = false;
    C.step.psd_resident = false;
    C.step.psd_nlarge = 0;
    C.step.psd_large_enabled = C.step.mixed_large_enabled = C.step.psd_scaling_large = C.step.start_psd_large = false;
    C.reg.cls = cone_class(ncones, kinds, ex);      // what the enables of hipkkt_step.cpp may switch on: per registration
    C.step.mode = C.reg.cls == ConeClass::Symmetric ? StepMode::Symmetric : StepMode::Off;
    // the non-symmetric cones: three-row cones in two lists (joined [Exponential | Power] below), GenPower descriptors (cone_layout.h)
    struct Row3 { int64_t row0, hs0, out0; double alpha; };
    std::vector<Row3> exp3, pow3;
    std::vector<int64_t> gpdesc, gpidx;
    std::vector<double> gpalpha;
    int64_t aoff = 0, ns_out = 0;
    std::vector<signed char> kind((size_t)std::max<int64_t>(m, 1), 2);
    std::vector<int64_t> rowhs((size_t)std::max<int64_t>(m, 1), 0), socdesc;
    C.reg.psd_hs.clear(); C.reg.psd_n.clear(); C.reg.psd_row.clear(); C.reg.psd_total = C.reg.psd_lam_total = 0; C.reg.nsoc = 0;
    C.reg.degree = 0;
    int64_t row = 0, hs = 0;
    int sparse_idx = 0;
    for (int64_t c = 0; c < ncones; c++) {
        const int64_t numel = S->cone_numel[c];
        const bool dense = S->cone_hs_dense[c] != 0;
        const int sk = S->cone_sparse_kind[c];
        const int64_t blk = dense ? numel * (numel + 1) / 2 : numel;
        if (kinds[c] == 0 || kinds[c] == 1) {
            if (dense || sk != 0) { S->err = "set_cone_types: a Zero / Nonnegative cone has a diagonal Hs block and no expansion"; return HIPKKT_ERR_ARGUMENT; }
            for (int64_t i = 0; i < numel; i++) { kind[row + i] = (signed char)kinds[c]; rowhs[row + i] = hs + i; }
            if (kinds[c] == 1) C.reg.degree += numel;
        } else if (kinds[c] == 2) {
            int64_t uv0 = -1, ord = -1;
            if (sk == 1) {
                ord = S->soc.of_sparse[sparse_idx];
                uv0 = S->soc.off[ord];
                if (dense || S->soc.off[ord + 1] - uv0 != numel) { S->err = "set_cone_types: sparse second-order cone does not match its expansion map"; return HIPKKT_ERR_ARGUMENT; }
            } else if (!dense || numel < 2 || numel > 4 || sk != 0) {
                // cone_types.jl:86-118: dim <= SOC_NO_EXPANSION_MAX_SIZE (4) is the dense form, everything larger the sparse one
                S->err = "set_cone_types: a second-order cone is either sparse-expanded or dense with dim <= 4"; return HIPKKT_ERR_ARGUMENT;
            }
            const int64_t d[kSocDesc] = {row, numel, hs, uv0, ord};      // kSocRow0, kSocDim, kSocHs0, kSocUv0, kSocOrd
            socdesc.insert(socdesc.end(), d, d + kSocDesc);
            C.reg.nsoc++;
            C.reg.degree += 1;
        } else if (kinds[c] == 3) {
            int64_t n = (int64_t)((std::sqrt(8.0 * (double)numel + 1.0) - 1.0) * 0.5 + 0.5);
            if (!dense || sk != 0 || n * (n + 1) / 2 != numel) { S->err = "set_cone_types: a PSD triangle cone has a dense block of triangular size"; return HIPKKT_ERR_ARGUMENT; }
            C.reg.psd_hs.push_back(hs);
            C.reg.psd_n.push_back(n);
            C.reg.psd_row.push_back(row);
            C.reg.psd_total += n * n;
            C.reg.psd_lam_total += n;
            C.reg.degree += n;
        } else if (ex && (kinds[c] == HIPKKT_CONE_EXP || kinds[c] == HIPKKT_CONE_POW)) {
            if (numel != 3 || !dense || sk != 0) { S->err = "set_cone_types_ex: an Exponential / Power cone has three rows, a dense Hs block and no expansion"; return HIPKKT_ERR_ARGUMENT; }
            double a = 0.0;
            if (kinds[c] == HIPKKT_CONE_POW) {
                if (aoff >= nalpha) { S->err = "set_cone_types_ex: alpha is shorter than the Power / GenPower cones need"; return HIPKKT_ERR_ARGUMENT; }
                a = alpha[aoff++];
                if (!(a > 0.0 && a < 1.0)) { S->err = "set_cone_types_ex: the exponent of a Power cone lies in (0, 1)"; return HIPKKT_ERR_ARGUMENT; }
            }
            (kinds[c] == HIPKKT_CONE_EXP ? exp3 : pow3).push_back({row, hs, ns_out, a});
            ns_out += kSlot3;
        } else if (ex && kinds[c] == HIPKKT_CONE_GENPOW) {
            if (sk != HIPKKT_SPARSE_GENPOW || dense || S->img.smaps[sparse_idx].kind != 2) { S->err = "set_cone_types_ex: a GenPower cone has a diagonal Hs block and a GenPow expansion map"; return HIPKKT_ERR_ARGUMENT; }
            const SparseMap &sm = S->img.smaps[sparse_idx];
            const int64_t d1 = (int64_t)sm.vec[0].size(), d2 = (int64_t)sm.vec[1].size();
            if (d1 < 1 || d1 + d2 != numel || (int64_t)sm.vec[2].size() != numel) { S->err = "set_cone_types_ex: GenPower cone does not match its expansion map"; return HIPKKT_ERR_ARGUMENT; }
            if (aoff + d1 > nalpha) { S->err = "set_cone_types_ex: alpha is shorter than the Power / GenPower cones need"; return HIPKKT_ERR_ARGUMENT; }
            for (int64_t i = 0; i < d1; i++)
                if (!(alpha[aoff + i] > 0.0 && alpha[aoff + i] < 1.0)) { S->err = "set_cone_types_ex: the exponents of a GenPower cone lie in (0, 1)"; return HIPKKT_ERR_ARGUMENT; }
            // kGpPsiBits: the bits of psi = 1 / <alpha, alpha> (cone_types.jl:301), which the step's Newton start reads (step_genpow.hip)
            double asq = 0.0;
            for (int64_t i = 0; i < d1; i++) asq += alpha[aoff + i] * alpha[aoff + i];
            const double psi = 1.0 / asq;
            int64_t psi_bits;
            memcpy(&psi_bits, &psi, sizeof(psi_bits));
            // kGpRow0, kGpDim1, kGpDim2, kGpHs0, kGpOut0, kGpAlpha0, kGpIdx0, kGpPsiBits
            const int64_t d[kGpDesc] = {row, d1, d2, hs, ns_out, (int64_t)gpalpha.size(), (int64_t)gpidx.size(), psi_bits};
            gpdesc.insert(gpdesc.end(), d, d + kGpDesc);
            gpalpha.insert(gpalpha.end(), alpha + aoff, alpha + aoff + d1);
            for (int t = 0; t < 3; t++) gpidx.insert(gpidx.end(), sm.vec[t].begin(), sm.vec[t].end());
            gpidx.insert(gpidx.end(), sm.D, sm.D + 3);
            aoff += d1;
            ns_out += gp_slot(d1, d2).len;
        }
        if (sk != 0) sparse_idx++;
        row += numel;
        hs += blk;
    }
    if (row != m || hs != S->img.nHs) { C.reg.ready = false; S->err = "set_cone_types: cone sizes do not add up to m / the Hs vector"; return HIPKKT_ERR_ARGUMENT; }
    if (ex && aoff != nalpha) { S->err = "set_cone_types_ex: alpha is longer than the Power / GenPower cones need"; return HIPKKT_ERR_ARGUMENT; }
    if (socdesc.empty()) socdesc.assign(kSocDesc, 0);
    // device buffers: allocated on the first call; a later call (same cone sizes, possibly other kinds) re-uses them when they are
    // large enough -- slab memory is only returned when the handle is destroyed, so repeated calls must not allocate again
    if (!C.tab.kind || (int64_t)socdesc.size() > C.tab.cap_socdesc || C.reg.psd_total > C.tab.cap_psd) {
        C.tab.kind = S->dalloc<signed char>(kind.size());
        C.tab.rowhs = S->dalloc<int64_t>(rowhs.size());
        C.tab.socdesc = S->dalloc<int64_t>(socdesc.size());
        C.tab.sz = S->dalloc<double>(2 * m);
        C.tab.wl = S->dalloc<double>(2 * m);
        fill_async(S->stream, C.tab.wl, 0, (size_t)std::max<int64_t>(2 * m, 1) * sizeof(double));   // w, lambda stay zero on the rows of cones the kernels do not write (PSD, others)
        C.tab.eta = S->dalloc<double>(socdesc.size() / kSocDesc);
        C.tab.R = S->dalloc<double>(C.reg.psd_total);
        C.tab.W = S->dalloc<double>(C.reg.psd_total);
        C.tab.fail = S->dalloc<int>(1);
        C.tab.cap_socdesc = (int64_t)socdesc.size();
        C.tab.cap_psd = C.reg.psd_total;
    }
    copy_sync(S->stream, C.tab.kind, kind.data(), kind.size() * sizeof(signed char), hipMemcpyHostToDevice);
    copy_sync(S->stream, C.tab.rowhs, rowhs.data(), rowhs.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    copy_sync(S->stream, C.tab.socdesc, socdesc.data(), socdesc.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    const int64_t n3 = (int64_t)(exp3.size() + pow3.size()), ngp = (int64_t)gpdesc.size() / kGpDesc;
    if (n3 + ngp > 0) {
        if (n3 > 0x7fffffff || ngp > 0x7fffffff) { S->err = "set_cone_types_ex: too many cones"; return HIPKKT_ERR_ARGUMENT; }
        // same rule as above: allocated on the first call, re-used while large enough
        if (n3 > C.tab.cap3) {
            C.tab.row0 = S->dalloc<int64_t>(n3); C.tab.hs0 = S->dalloc<int64_t>(n3); C.tab.out0 = S->dalloc<int64_t>(n3);
            C.tab.alpha = S->dalloc<double>(n3); C.tab.trips = S->dalloc<int>(n3);
            C.tab.cap3 = n3;
        }
        if (ngp > C.tab.cap_gp) { C.tab.gpdesc = S->dalloc<int64_t>(kGpDesc * ngp); C.tab.cap_gp = ngp; }
        if ((int64_t)gpalpha.size() > C.tab.cap_gpalpha) { C.tab.gpalpha = S->dalloc<double>(gpalpha.size()); C.tab.cap_gpalpha = (int64_t)gpalpha.size(); }
        if ((int64_t)gpidx.size() > C.tab.cap_gpidx) { C.tab.gpidx = S->dalloc<int64_t>(gpidx.size()); C.tab.cap_gpidx = (int64_t)gpidx.size(); }
        if (ns_out > C.tab.cap_out) { C.tab.nsout = S->dalloc<double>(ns_out); C.tab.cap_out = ns_out; }
        if (n3) {
            std::vector<int64_t> t_row((size_t)n3), t_hs((size_t)n3), t_out((size_t)n3);
            std::vector<double> t_a((size_t)n3);
            size_t k = 0;
            for (const std::vector<Row3> *v : {&exp3, &pow3})
                for (const Row3 &r : *v) { t_row[k] = r.row0; t_hs[k] = r.hs0; t_out[k] = r.out0; t_a[k] = r.alpha; k++; }
            copy_sync(S->stream, C.tab.row0, t_row.data(), t_row.size() * sizeof(int64_t), hipMemcpyHostToDevice);
            copy_sync(S->stream, C.tab.hs0, t_hs.data(), t_hs.size() * sizeof(int64_t), hipMemcpyHostToDevice);
            copy_sync(S->stream, C.tab.out0, t_out.data(), t_out.size() * sizeof(int64_t), hipMemcpyHostToDevice);
            copy_sync(S->stream, C.tab.alpha, t_a.data(), t_a.size() * sizeof(double), hipMemcpyHostToDevice);
            fill_async(S->stream, C.tab.trips, 0, (size_t)n3 * sizeof(int));
        }
        if (ngp) {
            copy_sync(S->stream, C.tab.gpdesc, gpdesc.data(), gpdesc.size() * sizeof(int64_t), hipMemcpyHostToDevice);
            copy_sync(S->stream, C.tab.gpalpha, gpalpha.data(), gpalpha.size() * sizeof(double), hipMemcpyHostToDevice);
            copy_sync(S->stream, C.tab.gpidx, gpidx.data(), gpidx.size() * sizeof(int64_t), hipMemcpyHostToDevice);
        }
        C.reg.nexp = (int)exp3.size(); C.reg.npow = (int)pow3.size(); C.reg.ngenpow = (int)ngp;
        C.reg.nonsym_len = ns_out;
        C.reg.nonsym = true;
    }
    C.reg.ready = true;
    return HIPKKT_OK;
    HK_LEAVE
}
int32_t hipkkt_set_cone_types(hipkkt_handle h, int64_t ncones, const int32_t *kinds) {
    return set_cone_types_impl(h, ncones, kinds, false, 0, nullptr);
}
int32_t hipkkt_set_cone_types_ex(hipkkt_handle h, int64_t ncones, const int32_t *kinds, int64_t nalpha, const double *alpha) {
    return set_cone_types_impl(h, ncones, kinds, true, nalpha, alpha);
}
int32_t hipkkt_get_nonsym_len(hipkkt_handle h, int64_t *len) {
    if (!h || !len) return HIPKKT_ERR_ARGUMENT;
    *len = h->cones.reg.nonsym ? h->cones.reg.nonsym_len : 0;
    return HIPKKT_OK;
}

// s, z (length m), psd_R (concatenated n x n column-major R factors, NULL = leave the PSD blocks to hipkkt_set_hs_psd or, after
// hipkkt_psd_scaling_enable, compute the factors on the device: scaling_psd.hip) and the three
// outputs (w and lambda of length m, eta per second-order cone; any may be NULL) are host pointers, or device pointers when `dev`
// ex: hipkkt_update_scaling_ex[_dev] -- the same launches in the same order, then the non-symmetric cones of the registration with
// (mu, strategy); nonsym_out (may be NULL) receives their output vector.  One host synchronisation per call, whatever the cone count.
static int32_t update_scaling_impl(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double *w_out,
                                   double *lambda_out, double *soc_eta_out, int32_t *scaling_ok, bool dev, bool ex = false,
                                   double mu = 0.0, int32_t strategy = 0, double *nonsym_out = nullptr) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    const bool psd_step = C.step.mode == StepMode::Psd || C.step.mode == StepMode::Mixed;
    if (!C.reg.ready) { S->err = "update_scaling: call hipkkt_set_cone_types first"; return HIPKKT_ERR_ARGUMENT; }
    if (!ex && C.reg.nonsym) { S->err = "update_scaling: the cone set has Exponential / Power / GenPower cones, which need mu: call hipkkt_update_scaling_ex"; return HIPKKT_ERR_ARGUMENT; }
    if (ex && strategy != 0 && strategy != 1) { S->err = "update_scaling_ex: strategy is 0 (PrimalDual) or 1 (Dual)"; return HIPKKT_ERR_ARGUMENT; }
    const int64_t m = S->img.m;
    if (m && (!s || !z)) { S->err = "update_scaling: null s / z"; return HIPKKT_ERR_ARGUMENT; }
    // hipkkt_psd_scaling_enable[_large]: without psd_R and without staged factors the PSD cones' (R, Rinv, lambda) come from
    // scaling_psd.hip and, for the cones of step_psd_large.hip after the second enable, from scaling_psd_large.hip
    const bool psd_nt_large = psd_step && C.step.psd_scaling_large;
    const bool psd_nt = psd_step && (C.step.psd_scaling || psd_nt_large) && !psd_R && !C.step.psd_fresh;
    if (psd_step && !psd_nt && (!psd_R || !C.step.psd_fresh)) {
        C.step.scaled = false;
        C.step.psd_resident = false;
        S->err = "update_scaling: after hipkkt_step_enable_psd / _mixed the call needs psd_R and the factors of a hipkkt_psd_set_factors[_dev] since the last scaling";
        return HIPKKT_ERR_ARGUMENT;
    }
    const double *ds = s, *dz = z, *dR = psd_R;
    if (!dev) {
        if (m) {
            HK_CHECK(hipMemcpyAsync(C.tab.sz, s, m * sizeof(double), hipMemcpyHostToDevice, S->stream));
            HK_CHECK(hipMemcpyAsync(C.tab.sz + m, z, m * sizeof(double), hipMemcpyHostToDevice, S->stream));
        }
        ds = C.tab.sz; dz = C.tab.sz + m;
        if (psd_R && C.reg.psd_total) {
            HK_CHECK(hipMemcpyAsync(C.tab.R, psd_R, (size_t)C.reg.psd_total * sizeof(double), hipMemcpyHostToDevice, S->stream));
            dR = C.tab.R;
        }
    } else if (m && C.step.mode != StepMode::Off) {      // the step entry points read the resident copy of (s, z)
        HK_CHECK(hipMemcpyAsync(C.tab.sz, s, m * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        HK_CHECK(hipMemcpyAsync(C.tab.sz + m, z, m * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
    }
    if (psd_step && !psd_nt) {      // the PSD step reads the resident (R, Rinv, lambda): R next to the staged pair
        if (dev) {
            HK_CHECK(hipMemcpyAsync(C.tab.R, psd_R, (size_t)C.reg.psd_total * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
            dR = C.tab.R;
        }
        HK_CHECK(hipMemcpyAsync(C.tab.psd_rinv, C.tab.psd_stage, (size_t)C.reg.psd_total * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        HK_CHECK(hipMemcpyAsync(C.tab.psd_lam, C.tab.psd_stage + C.reg.psd_total, (size_t)C.reg.psd_lam_total * sizeof(double),
                                hipMemcpyDeviceToDevice, S->stream));
        C.step.psd_fresh = false;
    }
    double *dw = C.tab.wl, *dl = C.tab.wl + m;
    launch_zero_words(S->stream, C.tab.fail, 1);
    if (psd_nt) {
        // (each cone is computed by one of the two launches: the first is given the bound below which the second serves none)
        launch_psd_nt_scaling(S->stream, (int)C.reg.psd_n.size(), C.tab.psdtab, ds, dz, C.tab.R, C.tab.psd_rinv, C.tab.psd_lam,
                              C.tab.psd_bad, C.tab.fail, psd_nt_large ? C.step.psd_lmin - 1 : psd_step_max_dim());
        if (psd_nt_large && C.step.psd_nlarge > 0) {
            PsdView P;
            P.npsd = (int)C.reg.psd_n.size(); P.tab = C.tab.psdtab;
            P.large = PsdLargeBatch{C.step.psd_nlarge, C.tab.psd_lidx, C.step.psd_lmin, C.step.psd_lmax, C.tab.psd_ws};
            launch_psd_large_nt_scaling(S->stream, P, ds, dz, C.tab.R, C.tab.psd_rinv, C.tab.psd_lam, C.tab.psd_bad, C.tab.fail);
        }
        dR = C.tab.R;
    }
    if (psd_step) launch_psd_step_check(S->stream, C.tab.psd_lam, C.reg.psd_lam_total, C.tab.fail);
    launch_scaling_diag(S->stream, C.tab.kind, C.tab.rowhs, S->d_mapHs, ds, dz, dw, dl, S->dp.kval, m);
    launch_scaling_soc(S->stream, C.reg.nsoc, C.tab.socdesc, S->d_mapHs, ds, dz, dw, dl, C.tab.eta, S->soc.d_u, S->soc.d_v,
                       S->soc.d_eta2, S->dp.kval, C.tab.fail);
    if (S->soc.n > 0)      // u, v, D entries of the sparse cones (the same kernel hipkkt_set_soc_batch uses)
        launch_soc_batch(S->stream, S->dp.kval, S->soc.d_uidx, S->soc.d_vidx, S->soc.d_cone, S->soc.d_u, S->soc.d_v, S->soc.d_eta2,
                         S->soc.total, S->soc.d_didx, S->soc.n);
    if (dR) {
        int64_t off = 0;
        for (size_t c = 0; c < C.reg.psd_n.size(); c++) {
            const int n = (int)C.reg.psd_n[c];
            launch_psd_rrt(S->stream, dR + off, C.tab.W + off, n);
            launch_psd_hs(S->stream, S->dp.kval, S->d_mapHs, C.reg.psd_hs[c], C.tab.W + off, n, psd_nt ? C.tab.psd_bad + c : nullptr);
            off += (int64_t)n * n;
        }
    }
    if (ex) C.step.mu = mu;
    if (ex && C.reg.nonsym) {
        launch_scaling_cone3(S->stream, C.reg.nexp, C.reg.npow, C.tab.row0, C.tab.hs0, C.tab.out0, C.tab.alpha, S->d_mapHs, ds, dz,
                             mu, strategy, S->dp.kval, C.tab.nsout, C.tab.trips, C.tab.fail);
        launch_scaling_genpow(S->stream, C.reg.ngenpow, C.tab.gpdesc, C.tab.gpalpha, C.tab.gpidx, S->d_mapHs, dz, mu, std::sqrt(mu),
                              S->dp.kval, C.tab.nsout, C.tab.fail);
    }
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (ex && C.reg.nonsym && nonsym_out && C.reg.nonsym_len)
        HK_CHECK(hipMemcpyAsync(nonsym_out, C.tab.nsout, (size_t)C.reg.nonsym_len * sizeof(double), kind, S->stream));
    if (w_out && m) HK_CHECK(hipMemcpyAsync(w_out, dw, m * sizeof(double), kind, S->stream));
    if (lambda_out && m) HK_CHECK(hipMemcpyAsync(lambda_out, dl, m * sizeof(double), kind, S->stream));
    if (soc_eta_out && C.reg.nsoc) HK_CHECK(hipMemcpyAsync(soc_eta_out, C.tab.eta, C.reg.nsoc * sizeof(double), kind, S->stream));
    int fail = 0;
    copy_sync(S->stream, &fail, C.tab.fail, sizeof(int), hipMemcpyDeviceToHost);
    if (scaling_ok) *scaling_ok = fail ? 0 : 1;
    C.step.scaled = fail == 0;
    C.step.psd_resident = psd_step;
    return HIPKKT_OK;
    HK_LEAVE
}
int32_t hipkkt_update_scaling(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double *w_out,
                              double *lambda_out, double *soc_eta_out, int32_t *scaling_ok) {
    return update_scaling_impl(h, s, z, psd_R, w_out, lambda_out, soc_eta_out, scaling_ok, false);
}
int32_t hipkkt_update_scaling_dev(hipkkt_handle h, const double *s_dev, const double *z_dev, const double *psd_R_dev, double *w_out_dev,
                                  double *lambda_out_dev, double *soc_eta_out_dev, int32_t *scaling_ok) {
    return update_scaling_impl(h, s_dev, z_dev, psd_R_dev, w_out_dev, lambda_out_dev, soc_eta_out_dev, scaling_ok, true);
}
int32_t hipkkt_update_scaling_ex(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double mu, int32_t strategy,
                                 double *w_out, double *lambda_out, double *soc_eta_out, double *nonsym_out, int32_t *scaling_ok) {
    return update_scaling_impl(h, s, z, psd_R, w_out, lambda_out, soc_eta_out, scaling_ok, false, true, mu, strategy, nonsym_out);
}
int32_t hipkkt_update_scaling_ex_dev(hipkkt_handle h, const double *s_dev, const double *z_dev, const double *psd_R_dev, double mu,
                                     int32_t strategy, double *w_out_dev, double *lambda_out_dev, double *soc_eta_out_dev,
                                     double *nonsym_out_dev, int32_t *scaling_ok) {
    return update_scaling_impl(h, s_dev, z_dev, psd_R_dev, w_out_dev, lambda_out_dev, soc_eta_out_dev, scaling_ok, true, true, mu, strategy,
                               nonsym_out_dev);
}

}  // extern "C"
