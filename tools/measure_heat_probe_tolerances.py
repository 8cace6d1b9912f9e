#!/usr/bin/env python3
"""Measure e_oracle, an fp32 implementation's own deviation from the float64 heat reference (tests/heat_reference.py), on every case of
tests/test_heat_probe_gpu.py, and write it to tests/golden/heat_probe/tolerances.json.  Runs on the CPU; no GPU, no reference project.

    python3 tools/measure_heat_probe_tolerances.py
    python3 tools/measure_heat_probe_tolerances.py --observed DIR      # only rewrite the "observed" section

The two stages with a continuous error:
    "recon"  the reconstruction up to every level: the fp32 oracle's heat bands (Oracle.process_block) and its pyr_expand against
             reconstruct(heat_band(D64)) on the same fp32 level-0 planes, in heat_reference.recon_error's measure, per level;
    "curve"  the tone curve: fp32 torch pow / cumsum against tone_curve of the same integer counts, largest absolute difference.
e_oracle of a stage and level is the largest value over the cases (a maximum over the pixels of one clip is a noisy figure: band_probe
pools its classes over the cases in the same way).  The GPU test allows FACTOR (4) times e_oracle, never more than the caps (5e-4
relative for the reconstruction, the band probe's per-pixel D bound; 1e-4 absolute for the curve).  The discrete stages -- range,
histogram total, branch flag, accept sets of one code -- have no tolerance.  "observed" (what an MI355X was seen to do) is kept as it
is unless --observed names the directory the GPU tests left their heat_probe__*.json files in (conftest.record_observed).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import heat_reference as hr  # noqa: E402


def measure_case(name):
    run = hr.model_run(name)
    D64 = hr.reference_D(run["planes0"], hr.case_rho(name))
    res = hr.run_checks(name, run, D64, only=("recon", "curve"))
    return {"recon": res["recon"]["err"], "curve": max(res["curve " + m]["err"] for m in hr.MODES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--observed", metavar="DIR")
    args = ap.parse_args()
    path = os.path.join(ROOT, "tests", "golden", hr.TOLERANCE_FILE)
    old = json.load(open(path)) if os.path.isfile(path) else {}
    if args.observed:
        import glob
        obs = {}
        for f in sorted(glob.glob(os.path.join(args.observed, "heat_probe__*.json"))):
            obs[os.path.basename(f)[len("heat_probe__"):-len(".json")]] = json.load(open(f))
        old["observed"] = obs
        doc = old
    else:
        per_case = {}
        for name in hr.CASES:
            per_case[name] = measure_case(name)
            print(name, per_case[name], flush=True)
        n = max(len(c["recon"]) for c in per_case.values())
        e = {"recon": [max(c["recon"][l] for c in per_case.values() if l < len(c["recon"])) for l in range(n)],
             "curve": max(c["curve"] for c in per_case.values())}
        doc = {"comment": "e_oracle: an fp32 implementation against the float64 heat reference (tools/measure_heat_probe_tolerances.py), "
                          "per stage and level, the largest over the cases; tolerance = min(factor * e_oracle, cap); observed: the GPU "
                          "tests' figures on an MI355X, per case, route and test",
               "factor": hr.FACTOR, "caps": hr.CAPS, "e_oracle": e, "per_case": per_case, "observed": old.get("observed", {})}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not args.observed:
        print("tolerances:", hr.tolerances())


if __name__ == "__main__":
    main()
