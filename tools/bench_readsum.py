#!/usr/bin/env python3
"""Time of the per-read summaries, the marks and the selection (dskgpu_read_summaries / _read_marks / dskgpu_select_reads) beside
dskgpu_query_reads on the same stream in the same process.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 3, trust_min = 3) and times, with device events on the stream the context runs
on (one warm-up call, then --reps calls of each, ALTERNATING; the median and all values go into the JSON line):
  * query_reads: the yardstick -- the same frame and the same lookups as the values kernel, 4 bytes written per stream byte;
  * read_summaries, with its stages "read values" / "read records" / "read summaries" from the library's stage marks;
  * read_marks with a rule on the median and the solid fraction (flags and stats);
  * select_reads by those marks into a buffer of the stream's size, with its stages "read records" / "read select".
One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("read values", "read records", "read summaries", "read select")


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def summary(prefix, ms):
    med = statistics.median(ms)
    return {prefix + "_ms_median": round(med, 3), prefix + "_ms_all": [round(x, 3) for x in ms], prefix + "_spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--abundance-min", type=int, default=3)
    ap.add_argument("--trust-min", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_readsum.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    n, p = reads.numel(), reads.data_ptr()
    ab = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n + 1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "read_summaries", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "stream_bytes": n, "k": args.k, "abundance_min": args.abundance_min, "trust_min": args.trust_min}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(p, n)
        kc.count()
        result["rows"] = kc.result_device()[2]
        kc.query_reads(p, n, ab.data_ptr())                                  # warm-ups (the index, the encode buffers, the code objects)
        st = kc.read_summaries(p, n, args.trust_min)
        result["stats"] = st
        keep = torch.zeros(st["n_records"], dtype=torch.uint8, device=dev)
        stream.synchronize()
        T = kc.read_summaries_numpy()
        rule = dict(min_valid=1, median_min=max(int(statistics.median(int(x) for x in T["median"][:100000])), 1), solid_num=9, solid_den=10)
        result["rule"] = rule
        result["marks"] = kc.read_marks(keep.data_ptr(), **rule)
        kc.select_reads(p, n, keep.data_ptr(), st["n_records"], out.data_ptr(), n + 1)
        before = dict(kc.stage_times())
        ms = {name: [] for name in ("query_reads", "read_summaries", "read_marks", "select_reads")}
        for _ in range(args.reps):                                           # alternating: query, summaries, marks, select, query, ...
            ms["query_reads"].append(timed(stream, lambda: kc.query_reads(p, n, ab.data_ptr()))[0])
            ms["read_summaries"].append(timed(stream, lambda: kc.read_summaries(p, n, args.trust_min))[0])
            ms["read_marks"].append(timed(stream, lambda: kc.read_marks(keep.data_ptr(), **rule))[0])
            t, sel = timed(stream, lambda: kc.select_reads(p, n, keep.data_ptr(), st["n_records"], out.data_ptr(), n + 1))
            ms["select_reads"].append(t)
        result["selected"] = {"out_bytes": sel[0], "out_records": sel[1]}
        for name, v in ms.items():
            result.update(summary(name, v))
        after = dict(kc.stage_times())
        for s in STAGES + ("query",):
            result["stage_%s_ms" % s.replace(" ", "_")] = round((after.get(s, 0.0) - before.get(s, 0.0)) / args.reps, 3)
        q = statistics.median(ms["query_reads"])
        for name in ("read_summaries", "read_marks", "select_reads"):
            result[name + "_over_query_reads"] = round(statistics.median(ms[name]) / q, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
