"""Summarise a scripts/gpu_profile.sh run into the committed evidence under profiles/.

    python tools/summarize_profiles.py gpurun_out/prof profiles/r01       (scripts/gpu_profile.sh)
    python tools/summarize_profiles.py gpurun_out/final profiles/r03      (scripts/gpu_final.sh)

Writes <dst>/rocprof/kernel_stats_bench.csv (rocprofv3 --kernel-trace --stats of
`python bench.py --full`), <dst>/rocprof/kernel_stats_by_grid.csv (the same trace per kernel AND grid size:
the headline batch separated from the batch-1 latency launches), <dst>/rocprof/pmc_summary.json (per-dispatch averages of every PMC counter for
the fused RRCDNet kernels), <dst>/parity_table.md, and profiles/traffic.json: HBM bytes per
spectrum of each dtype's kernel = (2 x FETCH_SIZE + WRITE_SIZE) KiB per dispatch / batch — FETCH_SIZE
doubled per the gfx950 correction of MI355X_MICROARCH.md §HBM (it reports half the bytes of wide
streaming reads).
"""
import csv
import glob
import json
import os
import shutil
import sys

# round 5: batch 8192 runs the walk kernels (geometry.hpp forward_geometry)
KERNELS = {"f16": "rdn::ip::rrcdnet_hybrid_walk<5, false>", "f16-plain": "rdn::h16fw::rrcdnet_walk", "f16f8": "rdn::ip::rrcdnet<3, 0>",
           "bf16x3": "rdn::ip::rrcdnet<2, 0>", "bf16-unsafe": "rdn::h16::rrcdnet"}
# scripts/gpu_final.sh passes: pmc_<arch>-<dtype>_<counter>, batch per arch
KERNELS_FINAL = {("RRCDNet", "f16"): ("rdn::ip::rrcdnet_hybrid_walk<5, false>", 8192),
                 ("RRCDNet", "f16-plain"): ("rdn::h16fw::rrcdnet_walk", 8192),
                 ("ADSDN", "f16"): ("rdn::cb::team16_forward<true>", 2048),
                 ("APIDN", "f16"): ("rdn::cb::team16_forward<false>", 2048)}
BATCH = 8192          # bench.py default --batch (the PMC passes run the default batch)


def kernel_ns(path, kernel):
    """Mean duration (ns) of `kernel`'s dispatches in a pass run with --kernel-trace, or None."""
    d = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if kernel in r["Kernel_Name"]:
                    d.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return sum(d) / len(d) if d else None


def derived(c, ns):
    """Ratios the DESIGN cites: MFMA busy of SIMD cycles, VALU per MFMA, LDS conflict share, clock."""
    out = {}
    if "SQ_VALU_MFMA_BUSY_CYCLES" in c and "SQ_BUSY_CU_CYCLES" in c:
        out["mfma_busy_frac_of_simd_cycles"] = c["SQ_VALU_MFMA_BUSY_CYCLES"] / (4 * c["SQ_BUSY_CU_CYCLES"])
    if "SQ_INSTS_VALU" in c and c.get("SQ_INSTS_MFMA"):
        out["valu_per_mfma"] = c["SQ_INSTS_VALU"] / c["SQ_INSTS_MFMA"]
    if c.get("SQ_LDS_IDX_ACTIVE") and "SQ_LDS_BANK_CONFLICT" in c:
        out["lds_conflict_frac_of_lds_active"] = c["SQ_LDS_BANK_CONFLICT"] / c["SQ_LDS_IDX_ACTIVE"]
    if c.get("SQ_VALU_MFMA_BUSY_CYCLES") and "SQ_VALU_MFMA_COEXEC_CYCLES" in c:
        out["valu_mfma_coexec_frac_of_mfma_busy"] = c["SQ_VALU_MFMA_COEXEC_CYCLES"] / c["SQ_VALU_MFMA_BUSY_CYCLES"]
    if "GRBM_GUI_ACTIVE" in c and ns:
        out["clock_ghz"] = c["GRBM_GUI_ACTIVE"] / 8 / ns
    return out


def counters(path, kernel):
    """{counter: mean per dispatch} over the dispatches of `kernel` in one PMC pass directory."""
    sums, counts = {}, {}
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if kernel not in r["Kernel_Name"]:
                    continue
                key = (r["Counter_Name"], r.get("Dispatch_Id"))
                sums[key] = sums.get(key, 0.0) + float(r["Counter_Value"])
    per = {}
    for (name, _), v in sums.items():
        per.setdefault(name, []).append(v)
    return {k: sum(v) / len(v) for k, v in per.items()}


def main():
    src, dst = sys.argv[1], sys.argv[2]
    os.makedirs(os.path.join(dst, "rocprof"), exist_ok=True)
    stats = glob.glob(os.path.join(src, "kt", "**", "*kernel_stats.csv"), recursive=True)
    if stats:
        shutil.copy(stats[0], os.path.join(dst, "rocprof", "kernel_stats_bench.csv"))
    # the default bench launches the headline kernel at two sizes (the timed batch and the batch-1
    # latency loop), so --stats' per-kernel average mixes them: also split the trace by grid size
    trace = glob.glob(os.path.join(src, "kt", "**", "*kernel_trace.csv"), recursive=True)
    if trace:
        groups = {}
        with open(trace[0]) as fh:
            for r in csv.DictReader(fh):
                grid = r.get("Grid_Size_X") or r.get("Grid_Size") or ""
                key = (r["Kernel_Name"], grid)
                groups.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        with open(os.path.join(dst, "rocprof", "kernel_stats_by_grid.csv"), "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["Name", "GridSizeX", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
            for (name, grid), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
                w.writerow([name, grid, len(d), sum(d), sum(d) / len(d), min(d), max(d)])
    if os.path.exists(os.path.join(src, "parity.md")):
        shutil.copy(os.path.join(src, "parity.md"), os.path.join(dst, "parity_table.md"))
    summary, traffic = {}, {}
    for dt, kern in KERNELS.items():
        c = {}
        for d in sorted(glob.glob(os.path.join(src, f"pmc_{dt}_*"))):
            if os.path.isdir(d):
                c.update(counters(d, kern))
        if not c:
            continue
        summary[f"RRCDNet/{dt}"] = {"kernel": kern, "batch": BATCH, "per_dispatch": c}
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            kib = 2 * c["FETCH_SIZE"] + c["WRITE_SIZE"]
            traffic[f"RRCDNet/{dt}"] = {
                "bytes_per_spectrum": kib * 1024 / BATCH,
                "source": f"{dst}/rocprof/pmc_summary.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), "
                          f"{kern}, batch {BATCH}, (2*FETCH_SIZE+WRITE_SIZE) KiB per dispatch / {BATCH}"}
        if "SQ_VALU_MFMA_BUSY_CYCLES" in c and "SQ_BUSY_CU_CYCLES" in c:
            summary[f"RRCDNet/{dt}"]["mfma_busy_frac_of_simd_cycles"] = (
                c["SQ_VALU_MFMA_BUSY_CYCLES"] / (4 * c["SQ_BUSY_CU_CYCLES"]))
    for (arch, dt), (kern, batch) in KERNELS_FINAL.items():
        c, ns = {}, None
        for d in sorted(glob.glob(os.path.join(src, f"pmc_{arch}-{dt}_*"))):
            if os.path.isdir(d):
                c.update(counters(d, kern))
                ns = ns or kernel_ns(d, kern)
        if not c:
            continue
        rec = {"kernel": kern, "batch": batch, "per_dispatch": c, "kernel_ns_under_pmc": ns}
        rec.update(derived(c, ns))
        summary[f"{arch}/{dt}"] = rec
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            kib = 2 * c["FETCH_SIZE"] + c["WRITE_SIZE"]
            traffic[f"{arch}/{dt}"] = {
                "bytes_per_spectrum": kib * 1024 / batch,
                "source": f"{dst}/rocprof/pmc_summary.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), "
                          f"{kern}, batch {batch}, (2*FETCH_SIZE+WRITE_SIZE) KiB per dispatch / {batch}"}
    for name in ("bench.json", "kt_bench.json"):
        if os.path.exists(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), os.path.join(dst, name.replace("kt_bench", "bench_under_rocprof")))
    with open(os.path.join(dst, "rocprof", "pmc_summary.json"), "w") as fh:
        json.dump(summary, fh, indent=1)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if traffic:
        tpath = os.path.join(root, "profiles", "traffic.json")
        merged = {}
        if os.path.exists(tpath):            # keep the entries this run did not re-measure
            with open(tpath) as fh:
                merged = json.load(fh)
        merged.update(traffic)
        with open(tpath, "w") as fh:
            json.dump(merged, fh, indent=1)
    print(json.dumps({"traffic": traffic, "derived": {k: {kk: vv for kk, vv in v.items() if kk not in ("per_dispatch",)}
                                                      for k, v in summary.items()}}, indent=1))


if __name__ == "__main__":
    main()
