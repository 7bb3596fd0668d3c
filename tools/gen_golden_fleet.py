#!/usr/bin/env python3
"""Records tests/golden/fleet_flights.json: what the sixteen flights of tests/fleet_flight_cases.py produce -- per
configuration a digest of the whole flight, the run-length-encoded sequence of library entry points run() called, the number of
context synchronisations and a few totals -- for tests/test_gpu_fleet_flights.py to hold every later commit to.

Uses FleetReplanLoop's public surface only, so the same file records any commit.  Record twice, in two processes:
  timeout -k 10 300 python tools/gen_golden_fleet.py --commit $(git rev-parse --short HEAD) --out /tmp/first.json && \\
  timeout -k 10 300 python tools/gen_golden_fleet.py --commit $(git rev-parse --short HEAD) --against /tmp/first.json
The second run writes the fixture.  A configuration of the network modes whose two recordings differ is left out and named
in the header; any other difference, and a set of flights that misses one of the branches below, is refused."""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "neo-planner_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import fleet_flight_cases as fc

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "fleet_flights.json"))
ap.add_argument("--commit", required=True, help="the commit being recorded (the fixture's header names it)")
ap.add_argument("--against", default=None, help="an earlier recording of the same commit, from another process")
a = ap.parse_args()

fs = fc.setup()
neo = weights = None
flights = {}
for name in fc.CONFIGS:
    if name in fc.NETWORK and neo is None:
        import neo_planner_amd as npa
        neo = fc.make_neo(fs, npa.BatchPlanner())
        weights = fc.weights_digest(neo)
    flights[name] = fc.fly(fs, name, neo if name in fc.NETWORK else None)
    f = flights[name]
    print(f"{name}: {f['ticks']} ticks, replans {f['replans']} (most {f['replans_max']}), failed attempts {f['failed_attempts']}, "
          f"{len(f['calls'].split())} runs of calls, {f['synchronizes']} synchronisations"
          + (f", fallback missions {f['fallback_missions']}" if "fallback_missions" in f else "")
          + (f", failed ticks {f['failed_ticks']}" if "failed_ticks" in f else "") + f", {f['digest'][:12]}", flush=True)
fc.drop(fs)

# the flights must go through the branches a refactor can break
missed = []
if sum(f["failed_attempts"] > 0 for f in flights.values()) < 4:
    missed.append("fewer than four configurations with a failed attempt (target rounds r > 0)")
if not any(flights[k]["fallback_missions"] > 0 for k in fc.BATCH):
    missed.append("no batch configuration sent a mission to the fallback")
if not any(flights[k]["failed_ticks"] > 0 for k in fc.ROUTED):
    missed.append("no route configuration had a failed tick")
missed += [f"{k}: no mission with two plans" for k, f in flights.items() if f["replans_max"] < 2]
if missed:
    sys.exit("refused, the flights miss a branch:\n  " + "\n  ".join(missed))

left_out = []
if a.against:
    first = json.load(open(a.against))
    if first["commit"] != a.commit or first["weights"] != weights:
        sys.exit("refused: the earlier recording is of another commit or of other network weights")
    keep = ("digest", "calls", "synchronizes")
    differ = [k for k in flights if any(first["flights"][k][q] != flights[k][q] for q in keep)]
    other = [k for k in differ if k not in fc.NETWORK]
    if other:
        sys.exit(f"refused: two recordings of commit {a.commit} differ in {other} -- a finding about that commit")
    left_out = differ
    for k in left_out:
        del flights[k]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(dict(commit=a.commit, recorded_twice=bool(a.against), left_out=left_out, edits=[], weights=weights,
                   flights=flights), f, indent=1)
    f.write("\n")
print(f"wrote {a.out}: {len(flights)} flights of commit {a.commit}" + (f", left out {left_out}" if left_out else ""))
