"""Developer tool: what Settings.device_step changes end to end.  Every configuration is solved by the numpy stand-in caller in ONE
process on one GPU, first with device_scaling + device_reduced + device_residuals (the best path without the feature: the cone
algebra between the device calls runs on the host, the iterate crosses PCIe several times per iteration), then with device_step
added (the iterate stays in device memory, scalars cross).  Per path: one warm-up solve, then `--repeats` timed solves; the medians of
wall time per iteration and of the stand-in's timers, the bytes the Python binding moved per iteration in each direction
(clarabel.jl_amd/hipkkt.py TRAFFIC) and hipkkt_box_probe go into ONE JSON line on stdout.
Symmetric configurations (3, 2a, psd) get one more path: the last one with device_default_start added (the default start on the
device as well), so that default_start_ms and the bytes of a whole solve stand next to the same path without it in the same run.
usage: step_path_compare.py [--cfgs 3,2a,exp_pow,genpow,psd,psd_large,mixed,mixed_large] [--repeats 5] [--one-solve CFG [--third] [--start] [--dual]]   (--one-solve: a single device_step solve, for a kernel trace; --dual: min_switch_step_length = 1, so that a
non-symmetric set runs the Dual strategy and its barrier search in every iteration)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import clarabel_jl_amd  # noqa: E402,F401
import julia_standin as cl  # noqa: E402
from clarabel_jl_amd import hipkkt, problems  # noqa: E402

CONFIGS = {"3": ("portfolio_socp", problems.portfolio_socp), "2a": ("random_sparse_qp", problems.random_sparse_qp),
           # Exponential / Power cones next to the symmetric ones: the device-step path needs device_step_nonsymmetric
           "exp_pow": ("nonsymmetric_mix_exp_pow",
                       lambda: problems.nonsymmetric_mix(n=80, nexp=30, npow=20, ngenpow=0, nn=20, nzero=3, socdim=5, seed=5)),
           # ... and Generalized Power cones: device_step_genpower on top (the Dual strategy and its barrier search in every iteration)
           "genpow": ("nonsymmetric_mix_genpow",
                      lambda: problems.nonsymmetric_mix(n=80, nexp=10, npow=10, ngenpow=20, nn=20, nzero=3, socdim=5, seed=5)),
           # PSD triangle cones (benchmark configuration 5 at its size, 20 x PSD(50)): device_step_psd on top, the Cholesky / SVD of the
           # scaling on the host; and a third path with device_scaling_psd, where the device does them too
           "psd": ("sdp_blocks", problems.sdp_blocks),
           # two PSD triangle cones of side 96: without device_step_psd_large the whole set keeps the host loop
           "psd_large": ("sdp_blocks_2x96", lambda: problems.sdp_blocks(n=200, ncones=2, dim=96, seed=5)),
           # four PSD triangle cones of side 20 next to Exponential / Power cones: without device_step_mixed the set keeps the host loop;
           # a third path with device_scaling_psd
           "mixed": ("mixed_psd_nonsym_4x20",
                     lambda: problems.mixed_psd_nonsym(n=80, psd_sides=[20] * 4, nexp=20, npow=10, ngenpow=0, nn=20, nzero=3, socdim=5,
                                                       seed=5)),
           # two PSD triangle cones of side 96 next to Exponential / Power cones: without device_step_mixed_large the set keeps the host
           # loop; a third path with device_scaling_psd + device_scaling_psd_large.  (m = 9 430.  On the CPU oracle path: SOLVED in 12 iterations,
           # objective 158.298465489, no barrier search; the host cone algebra on the HIP plugin and both device paths end the same
           # way: profiles/step_path_compare_mixed_large.json)
           "mixed_large": ("mixed_psd_nonsym_2x96",
                           lambda: problems.mixed_psd_nonsym(n=80, psd_sides=[96] * 2, nexp=20, npow=10, ngenpow=0, nn=20, nzero=3,
                                                             socdim=5, seed=5))}
PARENT = dict(device_scaling=True, device_reduced=True, device_residuals=True)
STEP_EXTRA = {"exp_pow": dict(device_step_nonsymmetric=True),
              "genpow": dict(device_step_nonsymmetric=True, device_step_genpower=True),
              "psd": dict(device_step_psd=True),
              "psd_large": dict(device_step_psd=True, device_step_psd_large=True),
              "mixed": dict(device_step_nonsymmetric=True, device_step_psd=True, device_step_mixed=True),
              "mixed_large": dict(device_step_nonsymmetric=True, device_step_psd=True, device_step_psd_large=True, device_step_mixed=True,
                                  device_step_mixed_large=True)}      # what device_step needs on top, per configuration
THIRD = {"psd": ("device_step_and_scaling", dict(device_scaling_psd=True)),
         "mixed": ("device_step_and_scaling", dict(device_scaling_psd=True)),
         "mixed_large": ("device_step_and_scaling", dict(device_scaling_psd=True, device_scaling_psd_large=True))}      # a further path on top of device_step, where there is one
START = ("3", "2a", "psd")      # symmetric cone sets: the last path once more with device_default_start
# further paths of a configuration, each on top of the one before it: the Cholesky / SVD and the default start of PSD sides 65 .. 128
MORE = {"psd_large": [("device_step_and_scaling_large", dict(device_scaling_psd=True, device_scaling_psd_large=True)),
                      ("device_step_and_scaling_large_and_default_start", dict(device_default_start=True, device_default_start_psd_large=True))]}


def one_solve(prob, dual=False, **flags):
    st = cl.Settings(**flags)
    if dual:
        st.min_switch_step_length = 1.0
    solver = cl.Solver(*prob, st)
    for k in hipkkt.TRAFFIC:
        hipkkt.TRAFFIC[k] = 0
    sol = solver.solve()
    it = max(sol.iterations, 1)
    tm = solver.info.timers
    rec = dict(status=sol.status, iterations=sol.iterations, obj_val=sol.obj_val, device_step=bool(solver._device_step),
               ms_per_iteration=1e3 * tm["IP iteration"] / it,
               timers_ms_per_iteration={k: 1e3 * tm[k] / it for k in ("kkt update", "kkt solve", "scale cones")},
               barrier_searches=int(getattr(solver, "barrier_searches", 0)), default_start_ms=1e3 * tm["default start"], device_default_start=bool(getattr(solver, "_device_default_start", False)),
               h2d_bytes=hipkkt.TRAFFIC["h2d_bytes"], d2h_bytes=hipkkt.TRAFFIC["d2h_bytes"],
               h2d_bytes_per_iteration=hipkkt.TRAFFIC["h2d_bytes"] / it, d2h_bytes_per_iteration=hipkkt.TRAFFIC["d2h_bytes"] / it)
    return rec


def median_of(runs):
    out = dict(runs[0])
    out["ms_per_iteration"] = statistics.median(r["ms_per_iteration"] for r in runs)
    out["ms_per_iteration_all"] = [round(r["ms_per_iteration"], 4) for r in runs]
    out["timers_ms_per_iteration"] = {k: statistics.median(r["timers_ms_per_iteration"][k] for r in runs)
                                      for k in runs[0]["timers_ms_per_iteration"]}
    out["default_start_ms"] = statistics.median(r["default_start_ms"] for r in runs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="3,2a")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--one-solve", default=None)
    ap.add_argument("--third", action="store_true", help="--one-solve with the configuration's third path (psd, mixed: device_scaling_psd; psd_large, mixed_large: device_scaling_psd_large)")
    ap.add_argument("--dual", action="store_true", help="--one-solve with min_switch_step_length = 1 (the Dual strategy throughout)")
    ap.add_argument("--start", action="store_true", help="--one-solve with device_default_start (symmetric configurations; psd_large: device_default_start_psd_large)")
    args = ap.parse_args()
    if args.one_solve:
        rec = one_solve(CONFIGS[args.one_solve][1](), dual=args.dual, device_step=True, **PARENT, **STEP_EXTRA.get(args.one_solve, {}),
                        **(THIRD[args.one_solve][1] if args.third and args.one_solve in THIRD else {}),
                        **(MORE[args.one_solve][0][1] if args.third and args.one_solve in MORE else {}),
                        **(MORE[args.one_solve][1][1] if args.start and args.one_solve in MORE else {}),
                        **(dict(device_default_start=True) if args.start and args.one_solve in START else {}))
        print(json.dumps({"cfg": args.one_solve, "device_step": rec}))
        return
    result = {"tool": "step_path_compare", "repeats": args.repeats, "configs": {}}
    for cfg in args.cfgs.split(","):
        name, make = CONFIGS[cfg]
        prob = make()
        paths = {}
        step = dict(device_step=True, **PARENT, **STEP_EXTRA.get(cfg, {}))
        todo = [("host_cone_algebra", PARENT), ("device_step", step)]
        if cfg in THIRD:
            todo.append((THIRD[cfg][0], dict(step, **THIRD[cfg][1])))
        if cfg in START:
            todo.append((todo[-1][0] + "_and_default_start", dict(todo[-1][1], device_default_start=True)))
        for label, extra in MORE.get(cfg, []):
            todo.append((label, dict(todo[-1][1], **extra)))
        for label, flags in todo:
            one_solve(prob, **flags)                                   # warm-up: plan cache, graphs, code objects
            paths[label] = median_of([one_solve(prob, **flags) for _ in range(args.repeats)])
        assert paths["device_step"]["device_step"] and not paths["host_cone_algebra"]["device_step"]
        assert all(r["device_default_start"] == label.endswith("_and_default_start") for label, r in paths.items())
        result["configs"][cfg] = dict(problem=name, **paths,
                                      speedup=paths["host_cone_algebra"]["ms_per_iteration"] / paths["device_step"]["ms_per_iteration"])
        if cfg in THIRD:
            result["configs"][cfg]["speedup_third_over_device_step"] = \
                paths["device_step"]["ms_per_iteration"] / paths[THIRD[cfg][0]]["ms_per_iteration"]
    result["box_probe"] = hipkkt.box_probe(0)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
