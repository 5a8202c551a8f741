"""Per-class sums of a rocprofv3 kernel-statistics file of the depth encoder (profiles/depth_kernel_stats.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o depth -- \\
        python tools/depth_bench.py --no-eager --dtypes bf16 --batches 32 --rounds 2 --calls 4 --out OUT/bench.json
    python tools/depth_kernel_stats.py OUT

A run of its own, beside tools/depth_bench.py's timings (tracing slows the host).  The configuration in the header is read from the
bench file the profiled command wrote into OUT.  The encoder's kernels are grouped by name; torch's own kernels in the process (fills,
copies) and the one-off weight packing are listed but not counted in the shares."""
import argparse
import csv
import glob
import json
import os

CLASSES = (("gemm", "gemm"), ("mm32", "gemm"), ("gn_stats", "gn_stats"), ("gn_apply", "gn_apply"), ("conv_rows", "conv_rows"),
           ("depth_stem", "stem"), ("maxpool", "maxpool"), ("depth_pack", "weight pack (refresh, once)"))
NOT_COUNTED = ("other (torch)", "weight pack (refresh, once)")


def configuration(out_dir):
    """what the profiled tools/depth_bench.py run measured, from the JSON it left in out_dir"""
    found = []
    for f in sorted(glob.glob(os.path.join(out_dir, "*.json"))):
        try:
            rows = json.load(open(f)).get("rows", [])
        except (ValueError, AttributeError):
            continue
        found += [f"{r['dtype']}, B = {r['B']} ({r['views']} views)" for r in rows if "dtype" in r and "B" in r]
    return "; ".join(found) if found else "configuration not recorded (no depth_bench.py file in the directory)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", help="the directory given to rocprofv3 -d")
    a = ap.parse_args()
    files = glob.glob(os.path.join(a.out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {a.out_dir}")
    tot, calls = {}, {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            cls = next((c for part, c in CLASSES if part in name), "other (torch)")
            tot[cls] = tot.get(cls, 0.0) + ns
            calls[cls] = calls.get(cls, 0) + int(float(row.get("Calls") or 0))
    counted = sum(v for k, v in tot.items() if k not in NOT_COUNTED)
    print(f"rocprofv3 --kernel-trace --stats, DepthEncoder.encode_views, {configuration(a.out_dir)}: per-class share of the encoder's kernel time")
    for k in sorted(tot, key=tot.get, reverse=True):
        share = "   (not counted)" if k in NOT_COUNTED else f"{100 * tot[k] / counted:6.1f} %"
        print(f"  {k:<32}{calls[k]:>8} calls {tot[k] / 1e6:10.3f} ms {share}")


if __name__ == "__main__":
    main()
