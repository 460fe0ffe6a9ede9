#!/usr/bin/env python
"""After `gpurun -- bash tools/gpu_round.sh <tag>`: copy the summaries the judge reads into profiles/ and rebuild
profiles/traffic.json from the two counter passes of the SAME run, stamped with the source hash they belong to.
usage: python tools/collect_profiles.py <tag>"""
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import source_stamp  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "r03"
src = os.path.join(ROOT, "gpurun_out", f"round_{tag}")
dst = os.path.join(ROOT, "profiles")
stamp = json.load(open(os.path.join(src, "stamp.json")))
if stamp["source_sha256"] != source_stamp.source_sha():
    print("WARNING: sources changed since the GPU run; the stamp of the run is kept (bench.py will ignore traffic.json)")
try:
    stamp["git_head"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    stamp["git_dirty_files"] = len(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"]).decode().splitlines())
except Exception:
    pass


def first(pattern):
    hits = sorted(glob.glob(os.path.join(src, pattern), recursive=True))
    return hits[0] if hits else None


for name, pattern in (("kernel_stats.csv", "prof/**/*kernel_stats.csv"), ("train_kernel_stats.csv", "prof_train/**/*kernel_stats.csv"),
                      ("pmc_fetch_size.csv", "pmc_FETCH_SIZE/**/*counter_collection.csv"),
                      ("pmc_write_size.csv", "pmc_WRITE_SIZE/**/*counter_collection.csv"),
                      ("pmc_train_fetch_size.csv", "pmc_train_FETCH_SIZE/**/*counter_collection.csv"),
                      ("pmc_train_write_size.csv", "pmc_train_WRITE_SIZE/**/*counter_collection.csv"),
                      ("pmc_value_fetch_size.csv", "pmc_value_FETCH_SIZE/**/*counter_collection.csv"),
                      ("pmc_value_write_size.csv", "pmc_value_WRITE_SIZE/**/*counter_collection.csv"),
                      ("value_kernel_stats.csv", "prof_value/**/*kernel_stats.csv"),
                      ("bench.json", "bench.json"), ("bench_train.json", "bench_train.json"),
                      ("scores_kernel_stats.csv", "prof_scores/**/*kernel_stats.csv"), ("configs_kernel_stats.csv", "prof_cfg/**/*kernel_stats.csv"),
                      ("scores_bwd_kernel_stats.csv", "prof_scores_bwd/**/*kernel_stats.csv"), ("scores_bwd.txt", "scores_bwd.txt"),
                      ("bench_scores.json", "bench_scores.json"), ("bench_traceback.json", "bench_traceback.json"),
                      ("configs.txt", "configs.txt"), ("parts_configs2.txt", "parts_configs2.txt"),
                      ("ubench_mix.txt", "ubench_mix.txt"), ("ubench_mix2.txt", "ubench_mix2.txt"), ("ubench_vmemissue.txt", "ubench_vmemissue.txt"),
                      ("steady.txt", "steady.txt"), ("fwd_timeline.txt", "fwd_timeline.txt"),
                      ("bwd_trace.txt", "bwd_trace.txt"), ("bwd_trace_alias7.txt", "bwd_trace_alias7.txt"), ("fwd_trace.txt", "fwd_trace.txt"),
                      ("fwd_trace_alias7.txt", "fwd_trace_alias7.txt"), ("zero_probe.txt", "zero_probe.txt"), ("bigB.txt", "bigB.txt"),
                      ("shapes.txt", "shapes.txt"), ("bench_driver_protocol.json", "bench_driver_protocol.json"), ("ubench_f2mix.txt", "ubench_f2mix.txt"),
                      ("adj_trace.txt", "adj_trace.txt"), ("lens_ab.txt", "lens_ab.txt"),
                      ("pytest_multigpu.txt", "pytest_multigpu.txt"), ("multigpu_skipped.txt", "multigpu_skipped.txt"),
                      ("pytest_gpu.txt", "pytest_gpu.txt"), ("smoke.txt", "smoke.txt"), ("fuzz2.txt", "fuzz2.txt"), ("parts_fuzz.txt", "parts_fuzz.txt")):
    f = first(pattern)
    if f:
        out = os.path.join(dst, f"{tag}_{name}")
        if name.startswith("pmc_"):   # keep only the sdp_* rows (the torch fill kernels are noise)
            rows = list(csv.reader(open(f)))
            with open(out, "w", newline="") as fh:
                w = csv.writer(fh)
                w.writerow(rows[0])
                w.writerows(r for r in rows[1:] if any(c.startswith("sdp_") for c in r))
        else:
            shutil.copy(f, out)
        print("->", os.path.relpath(out, ROOT))


def counter_means(path):
    acc = collections.defaultdict(list)
    meta = {}
    if not path:
        return acc, meta
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"]
        if k.startswith("sdp_"):
            acc[k].append(float(r["Counter_Value"]))
            meta[k] = {"vgpr": int(r["VGPR_Count"]), "sgpr": int(r["SGPR_Count"]), "workgroup": int(r["Workgroup_Size"]), "grid": int(r["Grid_Size"])}
    return acc, meta


traffic = {"_stamp": stamp,
           "_note": "B=256 N=M=512 NW. `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` in separate passes over bench.py "
                    "(--steps 3 --warmup 1; fwdbwd and --mode train), tools/gpu_round.sh.  Counter unit: KB.  FETCH_SIZE is "
                    "doubled (MI355X_MICROARCH.md, HBM section: on gfx950 it reports half the bytes of wide coalesced reads; "
                    "calibrated on sdp_bwd_kernel, which must read exactly the packed state).  WRITE_SIZE as is.  The counters "
                    "sit on the fabric side of L2 and include Infinity-Cache hits."}
for mode in ("", "train_", "value_"):   # (value_: the value-only forward sweep alone, tools/value_bench.py only=B cfg=1)
    fe, meta = counter_means(first(f"pmc_{mode}FETCH_SIZE/**/*counter_collection.csv"))
    wr, _ = counter_means(first(f"pmc_{mode}WRITE_SIZE/**/*counter_collection.csv"))
    for k in sorted(set(fe) | set(wr)):
        if k in traffic:
            continue
        f = sum(fe[k]) / len(fe[k]) if fe.get(k) else None
        w = sum(wr[k]) / len(wr[k]) if wr.get(k) else None
        traffic[k] = {"fetch_bytes_per_launch": None if f is None else 2.0 * f * 1024, "write_bytes_per_launch": None if w is None else w * 1024,
                      "hbm_bytes_per_launch": None if f is None or w is None else 2.0 * f * 1024 + w * 1024,
                      "fetch_size_raw_kb": f, "write_size_raw_kb": w, "fetch_correction": 2.0,
                      "launches_averaged": len(fe.get(k, [])), **meta.get(k, {})}
json.dump(traffic, open(os.path.join(dst, "traffic.json"), "w"), indent=1)
# the value-only forward sweep alone (tools/value_bench.py only=B cfg=1 under rocprofv3): its kernel time and its traffic go next to
# the A/B figures in profiles/value_bench.json, if that file belongs to the same sources
vb, ks = os.path.join(dst, "value_bench.json"), first("prof_value/**/*kernel_stats.csv")
if os.path.exists(vb) and "sdp_val_kernel" in traffic:
    doc = json.load(open(vb))
    if doc.get("_stamp", {}).get("source_sha256") == stamp["source_sha256"]:
        doc["profile_B_configs1"] = {"traffic": traffic["sdp_val_kernel"], "note": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, one pass each, nothing else traced; "
                                     "rocprofv3 --kernel-trace --stats in a run of its own.  WRITE_SIZE counts in KB: Vt is 1 KB"}
        if ks:
            row = [r for r in csv.DictReader(open(ks)) if r["Name"] == "sdp_val_kernel"]
            if row:
                doc["profile_B_configs1"]["kernel_us"] = {"calls": int(row[0]["Calls"]), "mean": float(row[0]["AverageNs"]) / 1e3,
                                                          "min": float(row[0]["MinNs"]) / 1e3, "max": float(row[0]["MaxNs"]) / 1e3}
        json.dump(doc, open(vb, "w"), indent=1)
        print("-> profiles/value_bench.json: profile_B_configs1")
print("-> profiles/traffic.json", {k: round(v["hbm_bytes_per_launch"] / 1e6, 1) for k, v in traffic.items() if not k.startswith("_") and v["hbm_bytes_per_launch"]})
