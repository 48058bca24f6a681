"""A/B passes of bench.py over several builds of the library, in the form every kernel round since
round 8 reports: all builds in one call on one box, alternating within every pass, the order
rotated every pass, every run a fresh process.

  python tools/ab_passes.py --build parent=pbn_rl_amd/libpbn_env_diag_base.so --build pr=tree \
      --passes 6 --out ab.json [--name T2000] [-- bench.py arguments]

`tree` is the in-tree library; anything else is loaded through PBN_LIB (tools/ab_build.sh builds a
revision's).  The bench.py arguments default to `--no-cpu-baseline` (the 2,000-step headline).
The project's rule for a gain: a build's slowest pass above the other's fastest.  A run that
fails or passes its time limit ends the whole call (nothing more is started on the GPU).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def one_run(lib, bench_args, limit):
    env = dict(os.environ)
    env.pop("PBN_LIB", None)
    if lib != "tree":
        env["PBN_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), *bench_args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("bench.py failed (%d) with %s: stopping" % (r.returncode, lib))
    d = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return {"value": d["value"], "launch_us": d.get("timing", {}).get("launch_us")}


def summary(passes):
    out = {}
    for name, rows in passes.items():
        v = [r["value"] for r in rows]
        out[name] = {"min": min(v), "max": max(v), "mean": statistics.fmean(v), "median": statistics.median(v)}
    first = next(iter(passes))
    for name in passes:
        if name != first:
            out[name]["median_over_%s_median" % first] = out[name]["median"] / out[first]["median"]
            out[name]["slowest_over_%s_fastest" % first] = out[name]["min"] / out[first]["max"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="append", required=True, metavar="NAME=LIB", help="first one: the reference side")
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--name", default="T2000")
    ap.add_argument("--out", required=True, help="JSON file; an existing one gets this shape added")
    ap.add_argument("--limit", type=int, default=240, help="seconds per bench.py run")
    ap.add_argument("bench_args", nargs="*", default=[])
    args = ap.parse_args()
    builds = [b.split("=", 1) for b in args.build]
    bench_args = args.bench_args or ["--no-cpu-baseline"]
    passes = {name: [] for name, _ in builds}
    for p in range(args.passes):
        order = builds[p % len(builds):] + builds[:p % len(builds)]
        for name, lib in order:
            row = dict(one_run(lib, bench_args, args.limit), **{"pass": p + 1})
            passes[name].append(row)
            print(args.name, "pass", p + 1, name, "%.4g" % row["value"], row["launch_us"], flush=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.setdefault("builds", {}).update({name: lib for name, lib in builds})
    doc.setdefault("shapes", {})[args.name] = {
        "command": "python bench.py " + " ".join(bench_args), "passes": passes, "summary": summary(passes),
        "note": "%d passes, the builds alternating within every pass, the order rotated every pass" % args.passes}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["shapes"][args.name]["summary"], indent=1))


if __name__ == "__main__":
    main()
