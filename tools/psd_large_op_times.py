"""Developer tool: device time of the granular step operations on one PSD triangle cone, [PSD(side)], through step_psd.hip (side <= 64)
resp. step_psd_large.hip (side 65 .. 128, Settings.device_step_psd_large).  What profiles/psd_large_ops.json was made with.

    rocprofv3 --kernel-trace --stats -d OUT/<side>_<op> -o t --output-format csv -- \\
        python tools/psd_large_op_times.py run <side> <mul_hs|shift|offset|length>  > OUT/<side>_<op>.log
    python tools/psd_large_op_times.py collect OUT > profiles/psd_large_ops.json

`run` makes one warm-up call and REPS timed calls on the production library and prints one JSON line (median host wall time of the
call, hipkkt_box_probe).  `collect` adds, per (side, operation), the kernels of that operation from the trace's statistics:
device_us_per_call is the sum of the kernel durations of one call -- the gaps between the launches of one call are NOT in it."""
import csv
import glob
import json
import os
import statistics
import sys
import time

REPS = 25


def run(side, op):
    os.environ["CLARABEL_HIPKKT_TESTING"] = "0"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np

    import julia_standin as cl
    from clarabel_jl_amd import hipkkt
    from tests import psd_step_reference as pr
    from tests import test_gpu_psd_step as tp
    from tests.step_support import STEP_FLAGS

    flags = dict(device_step=True, device_step_psd=True, device_step_psd_large=side > 64, **STEP_FLAGS)
    hk, cones = tp._handle([cl.PSDTriangleConeT(side)], 3, flags)
    assert hk.steps_psd and hk.steps_psd_large == (side > 64)
    rng = np.random.default_rng(903)
    s, z = tp._point(cones, rng, False)
    tp._scale(hk, cones, s, z)
    c = cones.cones[0]
    dz = -2.0 * z + 0.05 * pr.direction(c, rng, z)
    ds = -3.0 * s + 0.05 * pr.direction(c, rng, s)
    call = {"mul_hs": lambda: hk.cone_mul_hs(dz), "shift": lambda: hk.cone_combined_ds_shift(dz, ds, 0.37),
            "offset": lambda: hk.cone_ds_from_dz_offset(ds), "length": lambda: hk.cone_step_length(dz, ds, 1.0)}[op]
    call()
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(side=side, op=op, reps=REPS, calls=REPS + 1, host_wall_ms_median=statistics.median(wall),
                          result=(list(out) if op == "length" else None), box_probe=hipkkt.box_probe(0))))


def collect(root):
    out = {"tool": "tools/psd_large_op_times.py", "operations": []}
    for log in sorted(glob.glob(os.path.join(root, "*.log"))):
        rec = json.loads([ln for ln in open(log) if ln.startswith("{")][0])
        calls = rec["calls"]
        stats = glob.glob(os.path.join(log[:-4], "**", "*kernel_stats.csv"), recursive=True)[0]
        rows = [r for r in csv.DictReader(open(stats)) if "k_psd" in r["Name"] and int(r["Calls"]) >= calls]   # (not the scaling's)
        out["operations"].append(dict(
            side=rec["side"], op=rec["op"], calls=calls, launches_per_call=sum(int(r["Calls"]) for r in rows) // calls,
            device_us_per_call=round(sum(float(r["TotalDurationNs"]) for r in rows) / (1e3 * calls), 2),
            host_wall_us_median=round(1e3 * rec["host_wall_ms_median"], 1),
            kernels={r["Name"].split("(")[0].split("::")[-1]: dict(per_call=int(r["Calls"]) // calls, avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                                                                   min_us=round(float(r["MinNs"]) / 1e3, 2), max_us=round(float(r["MaxNs"]) / 1e3, 2))
                     for r in rows},
            box_probe=rec["box_probe"]))
    out["operations"].sort(key=lambda o: (o["side"], o["op"]))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    else:
        collect(sys.argv[2])
