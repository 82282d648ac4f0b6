#!/usr/bin/env python3
"""Time of the sample colours (dskgpu_colors_add, dskgpu_colors_unitigs) beside dskgpu_query_reads on the same stream in the same process.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 3), cuts its stream behind record ends into 1, 4 and 16 banks of equal record
counts and times, with device events on the stream the context runs on (one warm-up call, then --reps calls of each, ALTERNATING; the median
and all values go into the JSON line):
  * query_reads: the yardstick -- the same frame and the same lookups, 4 bytes written per stream byte instead of one add per run of hits;
  * colors_add into a matrix of as many colours as banks, with its stage "colors" from the library's stage marks;
  * colors_unitigs (sum, all and any) once per bank count, on a compaction that is already built.
The per-lane run merge is a compile-time switch of csrc/colors.h: build a second library with
`make -C dsk_amd/csrc EXTRA=-DCOL_NO_MERGE OUT=../libdskgpu_nomerge.so` and run this tool with DSKGPU_LIB pointing at it.  max_cell_per_add is the largest cell one call adds: the adds that meet at one address.
One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--banks", default="1,4,16")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_colors.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth, engine
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    n, p = reads.numel(), reads.data_ptr()
    nl = torch.nonzero(reads == 10).reshape(-1)
    ab = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "colors", "library": os.path.basename(engine.library_path()), "workload": args.workload, "device": torch.cuda.get_device_name(0),
              "reads": nr, "read_len": rl, "stream_bytes": n, "k": args.k, "abundance_min": args.abundance_min, "banks": {}}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(p, n)
        kc.count()
        n_rows = kc.result_device()[2]
        result["rows"] = n_rows
        nu = kc.unitigs()["n_unitigs"]                                       # the compaction is built before anything is timed
        result["unitigs"] = nu
        kc.query_reads(p, n, ab.data_ptr())                                  # warm-up (the index, the encode buffers, the code objects)
        for nb in [int(x) for x in args.banks.split(",")]:
            ends = [int(nl[(i + 1) * nl.numel() // nb - 1].item()) + 1 for i in range(nb - 1)] + [n]
            total = torch.zeros((nu, nb), dtype=torch.int64, device=dev)
            all_, any_ = torch.zeros(nu, dtype=torch.int64, device=dev), torch.zeros(nu, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            kc.colors_begin(nb)
            st = kc.colors_add(p, n, ends)                                   # warm-up
            before = dict(kc.stage_times())
            ms = {"query_reads": [], "colors_add": []}
            for _ in range(args.reps):                                       # alternating: query, add, query, ...
                ms["query_reads"].append(timed(stream, lambda: kc.query_reads(p, n, ab.data_ptr()))[0])
                ms["colors_add"].append(timed(stream, lambda: kc.colors_add(p, n, ends))[0])
            after = dict(kc.stage_times())
            r = {"stats": st}
            for name, v in ms.items():
                r.update(summary(name, v))
            r["stage_colors_ms"] = round((after.get("colors", 0.0) - before.get("colors", 0.0)) / args.reps, 3)
            r["stage_query_ms"] = round((after.get("query", 0.0) - before.get("query", 0.0)) / args.reps, 3)
            r["colors_add_over_query_reads"] = round(statistics.median(ms["colors_add"]) / statistics.median(ms["query_reads"]), 3)
            r["colors_unitigs_ms_once"] = round(timed(stream, lambda: kc.colors_unitigs(1, total.data_ptr(), all_.data_ptr(), any_.data_ptr()))[0], 3)
            counts, _ = kc.colors_rows_tensor()
            cells = counts.to(torch.int64) & 0xFFFFFFFF
            assert int(cells.sum().item()) == (args.reps + 1) * st["n_placed"] and int(total.sum().item()) == int(cells.sum().item())
            r["max_cell_per_add"] = int(cells.max().item()) // (args.reps + 1)
            result["banks"][str(nb)] = r
            del total, all_, any_, counts, cells
    print(json.dumps(result))


if __name__ == "__main__":
    main()
