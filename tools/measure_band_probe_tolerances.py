#!/usr/bin/env python3
"""Measure e_oracle, the fp32 oracle's own deviation from the float64 band reference, on every case of tests/test_band_probe_gpu.py, and
write it to tests/golden/band_probe/tolerances.json.  Runs on the CPU; no GPU, no reference project.

    python3 tools/measure_band_probe_tolerances.py

The level-0 planes come from the oracle's front end (display model, DKL, temporal filters); both implementations of the band stage get
the same fp32 planes.  Four classes: "probe_q" (by conditioning class, band_reference.probe_class) and "dense_q" (tests/band_reference.py
q_error), "pyramid" (pyramid_error), "pixel_d" (d_error).  The GPU tests allow FACTOR (4) times the largest e_oracle of a class, never more than the suite's existing bounds (CAPS).
The file's "observed" section (what an MI355X was seen to do, per class and route) and "sensitivity" section are kept as they are:
the first is pasted in from the GPU tests' printed maxima, the second is rewritten by --sensitivity.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import band_reference as br  # noqa: E402


def measure_case(name, case, probes=True):
    _, rho, levels, _ = br.case_geometry(case)
    is_image = case["frames"] == 1
    out = {}
    if probes:
        e = {k: 0.0 for k in br.PROBE_CLASSES}
        for f in range(case["frames"]):
            for probes, test, ref in br.probe_batches(case):
                pl = br.oracle_planes(test, ref, case["display"], case["fps"], f).astype(np.float32)
                err = br.q_error(br.oracle_stage(pl, rho, is_image)["Q"], br.band_stage(pl, rho)["Q"])
                for p, ee in zip(probes, err):
                    for l in range(levels):
                        k = br.probe_class(p.level, l, levels)
                        e[k] = max(e[k], float(ee[:, l].max()))
        out["probe_q"] = e
    t, r = br.dense_clip(case)
    dq = pyr = dd = 0.0
    for f in range(case["frames"]):
        pl = br.oracle_planes(t, r, case["display"], case["fps"], f).astype(np.float32)
        o, d = br.oracle_stage(pl, rho, is_image), br.band_stage(pl, rho, want=("D", "gpyr"))
        dq = max(dq, float(br.q_error(o["Q"], d["Q"]).max()))
        pyr = max(pyr, max(br.pyramid_error(o["gpyr"], d["gpyr"])))
        dd = max(dd, max(br.d_error(o["D"], d["D"])))
    out.update(dense_q=dq, pyramid=pyr, pixel_d=dd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sensitivity", action="store_true", help="also rewrite the sensitivity section (slow)")
    ap.add_argument("--observed", metavar="DIR", help="only rewrite the observed section, from the band_probe__*.json files the GPU tests "
                    "left in DIR (conftest.record_observed): the largest error per route and class")
    args = ap.parse_args()
    path = os.path.join(ROOT, "tests", "golden", br.TOLERANCE_FILE)
    old = json.load(open(path)) if os.path.isfile(path) else {}
    if args.observed:
        import glob
        obs = {}
        for f in sorted(glob.glob(os.path.join(args.observed, "band_probe__*.json"))):
            parts = os.path.basename(f)[len("band_probe__"):-len(".json")].split("__")       # kind, case[, route]
            kind, route = parts[0], parts[2] if len(parts) > 2 else "debug_dump"
            for k, v in json.load(open(f)).items():
                key = ("probe_q " + k) if kind == "probe_q" else k
                obs.setdefault(route, {})[key] = max(obs.get(route, {}).get(key, 0.0), v)
        old["observed"] = obs
        with open(path, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")
        print(json.dumps(obs, indent=1))
        return
    per_case = {}
    for name, case in br.CASES.items():
        per_case[name] = measure_case(name, case)
        print(name, per_case[name], flush=True)
    for name, case in br.DENSE_ONLY.items():
        per_case[name] = measure_case(name, case, probes=False)
        print(name, per_case[name], flush=True)
    e = {k: max(c[k] for c in per_case.values() if k in c) for k in br.CAPS if k != "probe_q"}
    e["probe_q"] = {k: max(c["probe_q"][k] for c in per_case.values() if "probe_q" in c) for k in br.PROBE_CLASSES}
    doc = {
        "comment": "e_oracle: fp32 oracle against the float64 band reference (tools/measure_band_probe_tolerances.py); "
                   "tolerance of a class = min(factor * e_oracle, cap); observed: largest GPU error per class and route on an MI355X",
        "factor": br.FACTOR, "caps": br.CAPS, "e_oracle": e, "per_case": per_case,
        "sensitivity": old.get("sensitivity", {}), "observed": old.get("observed", {}),
    }
    if args.sensitivity:
        sens = {}
        for d in br.DEFECTS:
            best = ("", "", 0.0)
            dense = {}
            for name in br.CASES:
                moved, dn = br.defect_sensitivity(name, d)
                dense[name] = dn
                k = max(moved, key=moved.get)
                if moved[k] > best[2]:
                    best = (name, k, moved[k])
            sens[d] = {"what": br.DEFECTS[d], "best_probe": f"{best[0]}:{best[1]}", "probe_q_moves": best[2], "dense_q_moves": dense}
            print(d, sens[d], flush=True)
        doc["sensitivity"] = sens
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("tolerances:", br.tolerances())


if __name__ == "__main__":
    main()
