#!/usr/bin/env python3
"""Rate of the lookups in a count's result (dskgpu_query_reads) against the path a user had before them.

Counts a workload (default c2_10Mx150, k = 31), then times, with device events on the stream the context runs on:
  * the index build (dskgpu_query_prepare): a one-off cost per result;
  * query_reads over the counted reads: one warm-up call, then the median of --reps calls;
  * the baseline -- NOT the code under test: dskgpu_k_enumerate into a buffer, torch.searchsorted over word 0 of the globally ordered
    rows, an equality check and a gather of the abundance (k <= 32 only: the higher words are not on the device for a caller);
  * query_reads alone at the --extra-k sizes (no baseline exists above k = 32).
Both paths must give the same answer at every position; the tool checks that before it prints.  One JSON line on stdout.
"""
import argparse
import ctypes
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


def bench_k(args, dev, reads, k, partition_order, baseline):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    n = reads.numel()
    res = {"k": k, "partition_order": bool(partition_order), "lookups": n}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, partition_order=partition_order,
                                                 stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), n)
        kc.count()
        st = kc.stats()
        rows = st["n_solid"]
        out = torch.zeros(n, dtype=torch.int32, device=dev)
        stream.synchronize()
        free0 = torch.cuda.mem_get_info(dev)[0]
        ms_index, _ = timed(stream, kc.query_prepare)
        index_bytes = free0 - torch.cuda.mem_get_info(dev)[0]
        kc.query_reads(reads.data_ptr(), n, out.data_ptr())                   # warm-up (allocates the two encode buffers)
        ms = [timed(stream, lambda: kc.query_reads(reads.data_ptr(), n, out.data_ptr()))[0] for _ in range(args.reps)]
        stages = dict(kc.stage_times())
        res.update(rows=rows, n_kmers=st["n_kmers"], index_ms=round(ms_index, 3), index_bytes_per_row=round(index_bytes / max(rows, 1), 2),
                   query_ms_median=round(statistics.median(ms), 3), query_ms_all=[round(x, 3) for x in ms],
                   lookups_per_s=round(n / (statistics.median(ms) * 1e-3), 1),
                   stage_query_index_ms=round(stages.get("query index", 0.0), 3))
        hits = int((out != 0).sum())
        res["positions_answered"] = hits
        if baseline:
            assert k <= 32 and not partition_order
            kp, ap, nr = kc.result_device()
            hip = ctypes.CDLL("libamdhip64.so")
            rk = torch.empty(nr, dtype=torch.int64, device=dev); ra = torch.empty(nr, dtype=torch.int32, device=dev)
            stream.synchronize()
            assert hip.hipMemcpy(ctypes.c_void_p(rk.data_ptr()), ctypes.c_void_p(kp), ctypes.c_size_t(nr * 8), 3) == 0
            assert hip.hipMemcpy(ctypes.c_void_p(ra.data_ptr()), ctypes.c_void_p(ap), ctypes.c_size_t(nr * 4), 3) == 0
            kmers = torch.empty(n, dtype=torch.int64, device=dev); valid = torch.empty(n, dtype=torch.uint8, device=dev)

            def user_path():
                kc.k_enumerate(reads.data_ptr(), n, kmers.data_ptr(), valid.data_ptr())
                at = torch.searchsorted(rk, kmers).clamp_(max=nr - 1)
                hit = (rk[at] == kmers) & (valid != 0)
                return torch.where(hit, ra[at], torch.zeros((), dtype=torch.int32, device=dev))
            ref = user_path()                                                  # warm-up
            same = bool((ref == out).all())
            del ref
            bms = []
            for _ in range(args.reps):
                t, r = timed(stream, user_path)
                del r
                bms.append(t)
            res.update(baseline_ms_median=round(statistics.median(bms), 3), baseline_ms_all=[round(x, 3) for x in bms],
                       baseline_lookups_per_s=round(n / (statistics.median(bms) * 1e-3), 1),
                       ratio=round(statistics.median(bms) / statistics.median(ms), 3), baseline_agrees=same)
            assert same, "the baseline and query_reads disagree"
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--extra-k", default="63,96", help="comma-separated k whose query rate is measured without a baseline ('' = none)")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-partition-order", action="store_true", help="skip the run on a DSKGPU_F_PARTITION_ORDER result")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_query.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "query_reads", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "main": bench_k(args, dev, reads, args.k, False, not args.no_baseline and args.k <= 32)}
    if not args.no_partition_order:
        result["partition_order"] = bench_k(args, dev, reads, args.k, True, False)
    result["extra"] = [bench_k(args, dev, reads, int(k), False, False) for k in args.extra_k.split(",") if k]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
