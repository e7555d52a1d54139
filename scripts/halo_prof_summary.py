"""Per (kernel instance, grid) summary of the rocprofv3 output of scripts/halo_pmc.sh: the
counter CSVs of the PMC passes (mean over the dispatches after the first) with the derived
ratios of the wave lifetime, and the kernel-trace CSV (median duration after the first).
usage: python scripts/halo_prof_summary.py DIR..."""
import collections
import csv
import glob
import os
import re
import statistics
import sys


def short(name):
    return re.sub(r"^void ls::", "", name.split("(")[0])


def main():
    cnt = collections.defaultdict(lambda: collections.defaultdict(lambda: collections.defaultdict(float)))
    dur = collections.defaultdict(list)
    for d in sys.argv[1:]:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection*.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "halo" in r["Kernel_Name"]:
                    key = (short(r["Kernel_Name"]), int(r.get("Grid_Size") or r.get("Grid_Size_X")))
                    cnt[key][r["Counter_Name"]][int(r.get("Dispatch_Id") or r.get("Correlation_Id"))] += float(r["Counter_Value"])
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace*.csv"), recursive=True):
            rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
            for r in rows:
                if "halo" in r["Kernel_Name"]:
                    key = (short(r["Kernel_Name"]), int(r.get("Grid_Size") or r.get("Grid_Size_X")))
                    dur[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key in sorted(set(cnt) | set(dur)):
        print(f"== {key[0]}  grid {key[1]}")
        if key in dur:
            v = dur[key][1:] or dur[key]
            print(f"   kernel trace: median {statistics.median(v):9.1f} us over {len(v)} dispatches (min {min(v):.1f}, max {max(v):.1f})")
        c = {}
        for cn, per in sorted(cnt.get(key, {}).items()):
            vals = [per[k] for k in sorted(per)]
            vals = vals[1:] or vals
            c[cn] = sum(vals) / len(vals)
            print(f"   {cn:28s} {c[cn]:16.1f}")
        wc, waves = c.get("SQ_WAVE_CYCLES"), c.get("SQ_WAVES")
        if wc:  # (SQ_*_CYCLES count in units of 4 cycles per wave; the ratios are unit-free)
            for cn in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU"):
                if cn in c:
                    print(f"   {cn + ' / SQ_WAVE_CYCLES':44s} {c[cn] / wc:8.3f}")
        if c.get("SQ_VALU_MFMA_BUSY_CYCLES") and c.get("SQ_BUSY_CYCLES"):
            # MFMA-busy cycles are summed over the SIMDs, SQ_BUSY_CYCLES over the SEs: a ratio to compare builds by
            print(f"   {'SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES':44s} {c['SQ_VALU_MFMA_BUSY_CYCLES'] / c['SQ_BUSY_CYCLES']:8.3f}")
        if waves:
            for cn in ("SQ_INSTS_MFMA", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS"):
                if cn in c:
                    print(f"   {cn + ' per wave':44s} {c[cn] / waves:8.1f}")


if __name__ == "__main__":
    main()
