"""A/B evidence for a kernel change on the bench frame: two builds of the library side by side on one GPU.

usage: python tools/ab_profile.py <tag> <before.so> <after.so> --out DIR [--stamp-before TEXT] [--stamp-after TEXT] [--runs 5]
           [--only headline trace pmc]

Every run is a fresh `python bench.py` child with THERMONERF_HIP_LIB pointing at one of the two libraries, the builds alternating,
each under its own time limit; the first failure ends the script.  Three parts, each on its own:
  headline  plain `python bench.py`: ms per frame, rays/s, proposal / field ms of every run
  trace     `rocprofv3 --kernel-trace --stats -- python bench.py --steps 10 --warmup 2`: average ms of the field and proposal kernels per run
  pmc       ONE counter pass per build, no tracing beside it: SQ_INSTS_VALU SQ_INSTS_MFMA SQ_WAVE_CYCLES GRBM_GUI_ACTIVE of
            `bench.py --steps 3 --warmup 1`, mean per dispatch
Writes DIR/<tag>_before_kernel_trace_S192_f32.txt, <tag>_after_..., <tag>_before_pmc_S192_f32.txt, <tag>_after_... (the format of
profiles/round8_*) and DIR/<tag>_headline.json.  The stamps are the `measured at commit ...` text of the two sides (default:
tools/.head_stamp or `git rev-parse HEAD`).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("main_mfma_rays_kernel<true, false>", "proposal_rays_kernel<5, 4, true>")
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_WAVE_CYCLES", "GRBM_GUI_ACTIVE")
BENCH = [sys.executable, os.path.join(ROOT, "bench.py")]


def run(cmd, lib, limit, cwd=ROOT):
    env = dict(os.environ, THERMONERF_HIP_LIB=os.path.abspath(lib))
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:  # nothing more is started on the GPU after a failed run
        print("FAILED rc", p.returncode, cmd, p.stdout[-3000:], p.stderr[-3000:], sep="\n", flush=True)
        sys.exit(1)
    return p.stdout


def kernel_of(name):
    for k in KERNELS:
        if k.replace(" ", "") in name.replace(" ", ""):
            return k
    return None


def one_csv(d, suffix):
    files = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    if not files:
        print("no", suffix, "under", d, flush=True)
        sys.exit(1)
    return csv.DictReader(open(files[0]))


def main():
    from pmc_summary import head_stamp

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tag")
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--out", required=True)
    ap.add_argument("--stamp-before", default=None)
    ap.add_argument("--stamp-after", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", nargs="+", default=["headline", "trace", "pmc"], choices=["headline", "trace", "pmc"])
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sides = (("before", a.before, "parent", a.stamp_before or head_stamp()),
             ("after", a.after, "branch", a.stamp_after or head_stamp() + " + this change"))
    tmp = tempfile.mkdtemp(prefix="ab_profile_")
    headline = {side: [] for side, *_ in sides}
    if "headline" in a.only:
        for i in range(a.runs):
            for side, lib, _, _ in sides:
                d = json.loads([ln for ln in run(BENCH, lib, 200).splitlines() if ln.startswith('{"metric"')][-1])
                r = d["roofline"]
                headline[side].append({"ms_per_step": d["ms_per_step"], "rays_per_s": d["value"], "proposal_ms": r["proposal_ms"],
                                       "field_ms": r["field_ms"]})
                print("headline", side, i + 1, headline[side][-1], flush=True)
        json.dump(headline, open(os.path.join(a.out, a.tag + "_headline.json"), "w"), indent=1)
    if "trace" in a.only:
        rows = {side: [] for side, *_ in sides}
        for i in range(a.runs):
            for side, lib, _, _ in sides:
                d = os.path.join(tmp, "trace_%s_%d" % (side, i))
                run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--"] + BENCH +
                    ["--steps", "10", "--warmup", "2"], lib, 300, cwd=tmp)
                for row in one_csv(d, "kernel_stats.csv"):
                    k = kernel_of(row["Name"])
                    if k:
                        rows[side].append((k, i + 1, int(row["Calls"]), float(row["AverageNs"]) / 1e6))
                        print("trace", side, *rows[side][-1], flush=True)
        for side, _, who, stamp in sides:
            with open(os.path.join(a.out, "%s_%s_kernel_trace_S192_f32.txt" % (a.tag, side)), "w") as f:
                f.write("# rocprofv3 --kernel-trace --stats -- python bench.py --steps 10 --warmup 2  (%s; %d runs alternating with the other "
                        "build; 12 launches per run)\n# measured at commit %s\n" % (who, a.runs, stamp))
                if headline[side]:
                    f.write("# plain `python bench.py` in the same session, %d runs alternating, ms per frame: %s\n"
                            % (a.runs, ", ".join("%.3f" % h["ms_per_step"] for h in headline[side])))
                f.write("kernel,run,calls,avg_ms\n")
                for k in KERNELS:
                    for kk, n, calls, ms in rows[side]:
                        if kk == k:
                            f.write('"%s",%d,%d,%.4f\n' % (k, n, calls, ms))
    if "pmc" in a.only:
        for side, lib, _, stamp in sides:
            d = os.path.join(tmp, "pmc_" + side)
            run(["rocprofv3", "--pmc", *COUNTERS, "--output-format", "csv", "-d", d, "-o", "c", "--"] + BENCH + ["--steps", "3", "--warmup", "1"],
                lib, 300, cwd=tmp)
            per = {}
            for row in one_csv(d, "counter_collection.csv"):
                k = kernel_of(row["Kernel_Name"])
                if k:
                    key = (row["Dispatch_Id"], k, row["Counter_Name"])
                    per[key] = per.get(key, 0.0) + float(row["Counter_Value"])
            acc = {}
            for (_, k, c), v in per.items():
                acc.setdefault(k, {}).setdefault(c, []).append(v)
            with open(os.path.join(a.out, "%s_%s_pmc_S192_f32.txt" % (a.tag, side)), "w") as f:
                f.write("# rocprofv3 --pmc %s --output-format csv -- python bench.py --steps 3 --warmup 1\n" % " ".join(COUNTERS))
                f.write("# one counter pass of its own, no tracing beside it\n# measured at commit %s; mean per dispatch\n" % stamp)
                for k in sorted(acc, reverse=True):
                    f.write(k + "\n")
                    for c, v in sorted(acc[k].items()):
                        f.write("  %-28s %.6e  (mean of %d dispatches)\n" % (c, sum(v) / len(v), len(v)))
                        print("pmc", side, k, c, "%.6e" % (sum(v) / len(v)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
