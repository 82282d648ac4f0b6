#!/usr/bin/env python3
"""Time of threading reads through their own compacted graph (dskgpu_thread_place, dskgpu_thread_reads) against dskgpu_query_reads on the
same stream in the same process.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 2), builds the index, the compaction and the edges, then times, with device
events on the stream the context runs on (one warm-up call, then the median of --reps calls, all values in the JSON line):
  * query_reads: the yardstick -- the first two of the four dependent levels of a placement, 4 bytes written per stream byte;
  * thread_place: all four levels, 8 bytes written per stream byte;
  * thread_reads: the placement into scratch, then the walks, the steps and both supports.
Then dskgpu_simplify, and the three again on the cleaned graph.  For every graph: the stats of the threading, the largest edge_support and
unitig_support, and the stage times "thread place" / "thread walks" of one dskgpu_thread_reads.
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


def measure(args, kc, stream, reads, out_a, out_b):
    n = reads.numel()
    p = reads.data_ptr()
    res = {"rows": kc.result_device()[2], "n_unitigs": kc.unitigs()["n_unitigs"], "n_edges": kc.unitig_edges()["n_edges"]}
    kc.query_reads(p, n, out_a.data_ptr())                                   # warm-ups (allocate the encode buffers)
    kc.thread_place(p, n, out_a.data_ptr(), out_b.data_ptr())
    st = kc.thread_reads(p, n)
    q = [timed(stream, lambda: kc.query_reads(p, n, out_a.data_ptr()))[0] for _ in range(args.reps)]
    pl = [timed(stream, lambda: kc.thread_place(p, n, out_a.data_ptr(), out_b.data_ptr()))[0] for _ in range(args.reps)]
    before = dict(kc.stage_times())
    th = [timed(stream, lambda: kc.thread_reads(p, n))[0] for _ in range(args.reps)]
    after = dict(kc.stage_times())
    us, es = kc.thread_support_tensor()
    res.update(st, max_edge_support=int(es.max()) if es.numel() else 0, max_unitig_support=int(us.max()) if us.numel() else 0,
               **summary("query_reads", q), **summary("thread_place", pl), **summary("thread_reads", th))
    for name in ("thread place", "thread walks"):
        res["stage_" + name.replace(" ", "_") + "_ms"] = round((after.get(name, 0.0) - before.get(name, 0.0)) / args.reps, 3)
    res["place_over_query_reads"] = round(statistics.median(pl) / statistics.median(q), 3)
    res["thread_reads_over_place"] = round(statistics.median(th) / statistics.median(pl), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_thread.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    out_a = torch.zeros(reads.numel(), dtype=torch.int32, device=dev)
    out_b = torch.zeros(reads.numel(), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "read_threading", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "stream_bytes": reads.numel(), "k": args.k, "abundance_min": args.abundance_min}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        result["counted"] = measure(args, kc, stream, reads, out_a, out_b)
        result["simplify"] = {n: v for n, v in kc.simplify().items() if n in ("n_passes", "n_rows_left")}
        result["simplified"] = measure(args, kc, stream, reads, out_a, out_b)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
