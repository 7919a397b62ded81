#!/usr/bin/env python
"""Developer tool: time of one scaling update of the non-symmetric cones (include/hipkkt.h hipkkt_update_scaling_ex), per handle
  three   n3 Exponential + n3 Power cones (alpha ~ U(0.1, 0.9)), default n3 = 100 000
  genpow  ngp Generalized Power cones (len(alpha) in 2..4, dim2 in 1..3 as problems.nonsymmetric_mix), default 2 000
and per path, median of `reps` calls after warm-up, host values prepared outside the timed region:
  (a) the calls a caller without the on-device scaling makes for the same update: hipkkt_set_hs + one hipkkt_set_genpow per cone
  (b) hipkkt_update_scaling_ex from host pointers        (c) hipkkt_update_scaling_ex_dev (everything resident)
Every handle is measured in a child process under its own time limit, and path (c) once more under `rocprofv3 --kernel-trace --stats`
in a process of its own; a failing step ends the run.  The kernel times are set against the bytes each kernel must move
(three-row cone: 6 doubles in, 6 K entries + 15 doubles out).  usage: bench_nonsym_scaling.py [--n3 N] [--ngp N] [--reps R] [--out DIR]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _interior3(rng, n, alpha):
    """n points strictly inside a three-row cone and its dual: a multiple of the central ray plus a small perturbation (vectorised;
    alpha = None: Exponential cone)"""
    if alpha is None:
        ray = np.tile([-1.051383945322714, 0.556409619469370, 1.258967884768947], (n, 1))
    else:
        ray = np.stack([np.sqrt(1.0 + alpha), np.sqrt(2.0 - alpha), np.zeros(n)], axis=1)
    out = []
    for _ in range(2):      # s, then z: the central ray is inside both cones (unit_initialization!)
        v = ray * rng.uniform(0.5, 2.0, (n, 1)) + 0.05 * rng.standard_normal((n, 3))
        out.append(v)
    return out


def _three_row(n3, seed):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.1, 0.9, n3)
    se, ze = _interior3(rng, n3, None)
    sp_, zp = _interior3(rng, n3, alpha)
    m = 6 * n3
    numel = np.full(2 * n3, 3, dtype=np.int64)
    kinds = np.concatenate([np.full(n3, 4), np.full(n3, 5)]).astype(np.int32)
    s = np.concatenate([se.ravel(), sp_.ravel()])
    z = np.concatenate([ze.ravel(), zp.ravel()])
    return m, numel, np.ones(2 * n3, dtype=np.int32), np.zeros(2 * n3, dtype=np.int32), np.zeros(2 * n3, dtype=np.int64), kinds, alpha, s, z


def _genpow(ngp, seed):
    rng = np.random.default_rng(seed)
    numel, dim1, alpha, s, z = [], [], [], [], []
    for _ in range(ngp):
        d1, d2 = int(rng.integers(2, 5)), int(rng.integers(1, 4))
        a = rng.uniform(0.2, 1.0, d1)
        a /= a.sum()
        for v in (s, z):
            v.append(np.concatenate([np.sqrt(1.0 + a) * rng.uniform(0.5, 2.0) + 0.02 * rng.standard_normal(d1), 0.05 * rng.standard_normal(d2)]))
        numel.append(d1 + d2)
        dim1.append(d1)
        alpha.append(a)
    m = int(np.sum(numel))
    return (m, np.array(numel, dtype=np.int64), np.zeros(ngp, dtype=np.int32), np.full(ngp, 2, dtype=np.int32), np.array(dim1, dtype=np.int64),
            np.full(ngp, 6, dtype=np.int32), np.concatenate(alpha), np.concatenate(s), np.concatenate(z))


class _DevBuf:
    _hip = None

    def __init__(self, arr_or_n):
        import ctypes as C
        if _DevBuf._hip is None:
            _DevBuf._hip = C.CDLL("libamdhip64.so")
        self.hip = _DevBuf._hip
        host = np.zeros(arr_or_n) if isinstance(arr_or_n, int) else np.ascontiguousarray(arr_or_n, dtype=np.float64)
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(host.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0


def _median_ms(f, reps, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts))


def child(args):
    import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
    from clarabel_jl_amd import hipkkt

    m, numel, dense, skind, dim1, kinds, alpha, s, z = _three_row(args.n3, 1) if args.handle == "three" else _genpow(args.ngp, 2)
    P = sp.identity(m, format="csc")
    A = (-sp.identity(m, format="csc")).tocsc()
    t0 = time.perf_counter()
    h = hipkkt.Handle.from_parts(sp.triu(P, format="csc"), A, numel, dense, skind, dim1)
    t_create = time.perf_counter() - t0
    h.set_cone_types_ex(kinds, alpha)
    mu, strategy = float(s @ z) / (len(numel) * 3 + 1), (0 if args.handle == "three" else 1)
    ok, _, _, _, ns = h.update_scaling_ex(s, z, mu, strategy)
    assert ok, "a benchmark point is not interior"
    res = {"handle": args.handle, "cones": int(len(numel)), "m": int(m), "create_s": round(t_create, 3), "nonsym_len": int(len(ns)),
           "strategy": "primal_dual" if strategy == 0 else "dual"}
    if args.only_c:
        sd, zd, nd = _DevBuf(s), _DevBuf(z), _DevBuf(len(ns))
        for _ in range(5):
            assert h.update_scaling_ex_dev(sd.ptr, zd.ptr, mu, strategy, None, None, None, None, nd.ptr)
        print(json.dumps(res))
        return
    # (a): the host values of the same update, prepared here (outside the timed region) from the device's own result
    if args.handle == "three":
        hs = ns.reshape(-1, 15)[:, :6].ravel().copy()
        gp = []
        res["newton_steps"] = dict(zip(*[x.tolist() for x in np.unique(h.debug_dump(23).astype(np.int64), return_counts=True)]))
    else:
        hs, gp, off = np.zeros(h.nHs), [], 0
        row = 0
        for i, (d, d1) in enumerate(zip(numel, dim1)):
            blk = ns[off:off + 3 * d + d1 + 1]
            g, dd1, dd2, p, q, r = np.split(blk, np.cumsum([d, d1, 1, d, d1]))
            hs[row:row + d1] = mu * dd1
            hs[row + d1:row + d] = mu * dd2[0]
            gp.append((i, p.copy(), q.copy(), r.copy()))
            off += len(blk)
            row += d
    sq = float(np.sqrt(mu))

    def path_a():
        h.set_hs(hs)
        for i, p, q, r in gp:
            h.set_genpow(i, sq, p, q, r)

    K_b = None
    res["a_ms"], res["a_min_ms"] = _median_ms(path_a, args.reps)
    K_a = h.debug_dump(4)
    res["b_ms"], res["b_min_ms"] = _median_ms(lambda: h.update_scaling_ex(s, z, mu, strategy), args.reps)
    res["b_no_outputs_ms"], _ = _median_ms(lambda: h.update_scaling_ex(s, z, mu, strategy, want_outputs=False), args.reps)
    K_b = h.debug_dump(4)
    sd, zd, nd = _DevBuf(s), _DevBuf(z), _DevBuf(len(ns))
    res["c_ms"], res["c_min_ms"] = _median_ms(lambda: h.update_scaling_ex_dev(sd.ptr, zd.ptr, mu, strategy, None, None, None, None, nd.ptr), args.reps)
    res["K_equal_a_b"] = bool(np.array_equal(K_a, K_b))
    per = 6 * 8 + 6 * 8 + 6 * 8 + 15 * 8 + 4 * 8     # three-row cone: s, z in; 6 map entries; 6 K entries + 15 doubles out; 4 table words
    if args.handle == "three":
        res["bytes_per_cone"] = per
        res["c_GBps_if_all_kernel"] = round(per * len(numel) / (res["c_ms"] * 1e-3) / 1e9, 2)
    print(json.dumps(res))


def _run(cmd, limit, log):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(cmd, timeout=limit, capture_output=True, text=True, cwd=ROOT)
    log.write(r.stdout + r.stderr)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"step failed ({r.returncode}): nothing more is started on the GPU")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=100000)
    ap.add_argument("--ngp", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "nonsym_scaling"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--handle", choices=["three", "genpow"], help="(child) measure this handle")
    ap.add_argument("--only-c", action="store_true", help="(child) path (c) alone, for the profiler")
    args = ap.parse_args()
    if args.handle:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    results = {}
    me = [sys.executable, os.path.abspath(__file__), "--n3", str(args.n3), "--ngp", str(args.ngp), "--reps", str(args.reps)]
    with open(os.path.join(args.out, "bench_nonsym_scaling.log"), "w") as log:
        for hd in ("three", "genpow"):
            out = _run(me + ["--handle", hd], args.limit, log)
            results[hd] = json.loads(out.strip().splitlines()[-1])
            print(json.dumps(results[hd]), flush=True)
        if not args.no_prof:
            for hd in ("three", "genpow"):
                d = os.path.join(args.out, "prof_" + hd)
                _run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--"] + me + ["--handle", hd, "--only-c"],
                     args.limit, log)
                rows = []
                for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    with open(f) as fh:
                        rows += [r for r in csv.DictReader(fh) if "k_scaling" in r.get("Name", "")]
                results[hd]["kernel_stats"] = [{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in r} for r in rows]
                for r in results[hd]["kernel_stats"]:
                    print(json.dumps(r), flush=True)
    try:
        import clarabel_jl_amd  # noqa: F401
        from clarabel_jl_amd import hipkkt
        results["box_probe"] = hipkkt.box_probe()
    except Exception as e:     # the numbers above stand without it
        results["box_probe"] = str(e)
    with open(os.path.join(args.out, "bench_nonsym_scaling.json"), "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
