#!/usr/bin/env python3
"""Records tests/golden/planner_calls.json: what the cases of tests/planner_cases.py produce -- per case a digest of
everything the call returned, the run-length-encoded sequence of library entry points it made and the number of context
synchronisations -- for tests/test_gpu_planner_golden.py to hold every later commit to; and, from the same commit, what
tests/test_planner_cpu.py holds it to without a GPU: the signatures of the planners' public methods and the first error
of every refused argument set.

Uses the planners' public surface only, so the same file records any commit.  Record twice, in two processes:
  timeout -k 10 300 python tools/gen_golden_planner.py --commit $(git rev-parse --short HEAD) --out /tmp/first.json && \\
  timeout -k 10 300 python tools/gen_golden_planner.py --commit $(git rev-parse --short HEAD) --against /tmp/first.json
The second run writes the fixture.  No case may be left out: two recordings that differ, and a set of cases that misses one
of the branches planner_cases.BRANCHES names, are refused."""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "neo-planner_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import planner_cases as pc

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "planner_calls.json"))
ap.add_argument("--commit", required=True, help="the commit being recorded (the fixture's header names it)")
ap.add_argument("--against", default=None, help="an earlier recording of the same commit, from another process")
a = ap.parse_args()

signatures = pc.signatures()
refusals = {name: pc.refusal(name) for name in pc.REFUSALS}
silent = [k for k, v in refusals.items() if v == "no error"]
if silent:
    sys.exit(f"refused: {silent} raise nothing")

fs = pc.setup()
cases, missed = {}, []
for name in pc.CASES:
    cases[name], out = pc.run(fs, name)
    c = cases[name]
    print(f"{name}: {len(c['calls'].split())} runs of calls, {c['synchronizes']} synchronisations, {c['digest'][:12]}"
          + (f", launches {c['launch_sizes']}" if "launch_sizes" in c else "") + (f", {c['error']}" if "error" in c else ""), flush=True)
    if name in pc.BRANCHES and not pc.BRANCHES[name](out):
        missed.append(name)
pc.drop(fs)
if missed:
    sys.exit(f"refused, these cases miss the branch they are there for: {missed}")

if a.against:
    first = json.load(open(a.against))
    if first["commit"] != a.commit:
        sys.exit("refused: the earlier recording is of another commit")
    differ = [k for k in cases if first["cases"].get(k) != cases[k]]
    differ += [k for k in ("signatures", "refusals") if first[k] != {"signatures": signatures, "refusals": refusals}[k]]
    if differ:
        sys.exit(f"refused: two recordings of commit {a.commit} differ in {differ} -- a finding about that commit")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(dict(commit=a.commit, recorded_twice=bool(a.against), cases=cases, signatures=signatures, refusals=refusals), f, indent=1)
    f.write("\n")
print(f"wrote {a.out}: {len(cases)} cases, {len(signatures)} signatures and {len(refusals)} refusals of commit {a.commit}")
