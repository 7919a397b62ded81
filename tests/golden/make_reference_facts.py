#!/usr/bin/env python
"""Writes tests/golden/reference_checkout_facts.json: what tests/test_julia_glue.py needs to know about a checkout of the reference
(Clarabel.jl) to hold julia/clarabel_l1_seam.patch and julia/run_reference_tests_hip.jl against it, so that the suite does not need
the checkout itself.  Only facts are stored, no source text:

  "patch_context": per file the patch touches, the sha256 of every line the patch's hunks read (context and removed lines) at the
                   line number the hunk gives -- the patch applies exactly where it says iff the patch's own lines hash the same;
  "kit_names"    : the names `Clarabel.<name>` used by the test kit that occur (as a word) in the reference's src/*.jl;
  "kit_files"    : per test file the kit reads (test/OptTests/): the features of it the kit relies on, found or not.

Run:  python tests/golden/make_reference_facts.py /path/to/Clarabel.jl [out.json]
      (default output = tests/golden/reference_checkout_facts.json)
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATCH = os.path.join(ROOT, "julia", "clarabel_l1_seam.patch")
KIT = os.path.join(ROOT, "julia", "run_reference_tests_hip.jl")


def line_hash(s):
    return hashlib.sha256(s.encode("utf-8")).hexdigest()


def patch_old_lines(text):
    """{file: {old line number: line}} of every line a hunk reads (context ' ' and removed '-' lines)"""
    out, cur, ln = {}, None, 0
    for row in text.splitlines():
        if row.startswith("--- "):
            continue
        if row.startswith("+++ "):
            cur = row[4:].split("\t")[0]
            cur = cur[2:] if cur.startswith("b/") else cur
            out[cur] = {}
            continue
        m = re.match(r"@@ -(\d+)(?:,\d+)? \+\d+(?:,\d+)? @@", row)
        if m:
            ln = int(m.group(1))
            continue
        if cur is None or not row or row[0] not in " -+":
            continue
        if row[0] in " -":
            out[cur][ln] = row[1:]
            ln += 1
    return out


def kit_names(kit):
    return sorted(set(re.findall(r"\bClarabel\.([A-Za-z_]\w*!?)", kit)))


def kit_files(kit):
    return re.findall(r'"((?:basic_\w+|linear_solvers)\.jl)"', kit)


def file_features(name, txt):
    if name == "linear_solvers.jl":
        return {"solver_types_list": bool(re.search(r"SolverTypes\s*=\s*\[[^\]]*\]", txt)),
                "direct_solve_method_from_list": "direct_solve_method = SolverType" in txt}
    return {"constructs_solver": "Clarabel.Solver(" in txt, "unit_test_floats": "UnitTestFloats" in txt}


def main(ref, out):
    patch = open(PATCH).read()
    context = {}
    for f, lines in patch_old_lines(patch).items():
        src = open(os.path.join(ref, f), encoding="utf-8").read().split("\n")
        for ln, want in lines.items():
            if ln > len(src) or src[ln - 1] != want:
                raise SystemExit(f"{f}:{ln}: the patch does not apply at the position it gives")
        context[f] = {"lines": len(src), "sha256": {str(ln): line_hash(src[ln - 1]) for ln in sorted(lines)}}
    ref_src = ""
    for dp, _, files in sorted(os.walk(os.path.join(ref, "src"))):
        for f in sorted(files):
            if f.endswith(".jl"):
                ref_src += open(os.path.join(dp, f), encoding="utf-8").read() + "\n"
    kit = open(KIT).read()
    names = [n for n in kit_names(kit) if re.search(r"\b" + re.escape(n) + r"\b", ref_src)]
    files = {f: file_features(f, open(os.path.join(ref, "test", "OptTests", f), encoding="utf-8").read()) for f in kit_files(kit)}
    with open(out, "w") as fh:
        json.dump({"patch_context": context, "kit_names": names, "kit_files": files}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "reference_checkout_facts.json"))
