#!/usr/bin/env python3
"""Time of the row load (dskgpu_load_rows) beside the row sort of the count that made the rows and a device-to-device copy of the input.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 3) --reps times with stage timing and keeps the "sort" stage of every count:
its median and spread are what the load's order stage is read against (the same code on the same rows).  Then the rows go back in as the
input of a load, in a second context of the same process (abundance_min = 1, so that every row is kept), in four forms:
  * ascending    the rows as the count left them: the order step is skipped (sorted_input = 1);
  * shuffled     the same rows in a random order;
  * doubled      two copies of the rows, shuffled: every run of equal rows has length 2;
  * long_run     the shuffled rows plus --run-length (10^6) copies of one of them, shuffled in.
Every form is loaded once to warm up, then --reps rounds ALTERNATE between the four forms and a device-to-device copy of the first form's
bytes (the memory floor).  Per form: the whole call by device events, the stages "load check" / "load order" / "load combine" of
dskgpu_stage_times, the load's stats and sort_fallback.  --count-only stops after the counts and the copy (the numbers a library
without dskgpu_load_rows can give).  The medians and all values go into the one JSON line on stdout.
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


def summary(ms):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms], "spread": round((max(ms) - min(ms)) / med, 4) if med else 0.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--abundance-min", type=int, default=3)
    ap.add_argument("--run-length", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count-only", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_load.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth, engine
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "load_rows", "library": os.path.basename(engine.library_path()), "workload": args.workload, "device": torch.cuda.get_device_name(0),
              "reads": nr, "read_len": rl, "k": args.k, "abundance_min": args.abundance_min, "run_length": args.run_length}
    with torch.cuda.stream(stream):
        with KmerCounter(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
            kc.set_reads_device(reads.data_ptr(), reads.numel())
            kc.count()                                                      # warm-up
            sort_ms, count_ms = [], []
            for _ in range(args.reps):
                count_ms.append(timed(stream, kc.count)[0])
                sort_ms.append(dict(kc.stage_times())["sort"])
            kmers_h, ab_h = kc.rows()
            result["count"] = {"rows": int(len(ab_h)), "sort_fallback": kc.stats()["sort_fallback"], "sort_stage": summary(sort_ms), "count_call": summary(count_ms)}
        del reads
        n, words = len(ab_h), kmers_h.shape[1]
        kmers = torch.from_numpy(kmers_h.view(np.int64)).to(dev)
        ab = torch.from_numpy(ab_h.view(np.int32)).to(dev)
        del kmers_h, ab_h
        result["input_bytes"] = n * (8 * words + 4)
        k2, a2 = torch.empty_like(kmers), torch.empty_like(ab)

        def copy():
            k2.copy_(kmers)
            a2.copy_(ab)
        if args.count_only:
            copy()
            result["d2d_copy"] = summary([timed(stream, copy)[0] for _ in range(args.reps)])
            print(json.dumps(result))
            return
        g = torch.Generator(device=dev)
        g.manual_seed(1)

        def shuffled(k, a):
            perm = torch.randperm(a.numel(), device=dev, generator=g)
            return k[perm].contiguous(), a[perm].contiguous()
        at = n // 3
        forms = {"ascending": (kmers, ab), "shuffled": shuffled(kmers, ab), "doubled": shuffled(torch.cat([kmers, kmers]), torch.cat([ab, ab])),
                 "long_run": shuffled(torch.cat([kmers, kmers[at: at + 1].expand(args.run_length, words)]), torch.cat([ab, ab[at: at + 1].expand(args.run_length)]))}
        stream.synchronize()
        with KmerCounter(kmer_size=args.k, abundance_min=1, stream=stream.cuda_stream, timing=True) as kc:
            info, ms = {}, {name: {"call": [], "load check": [], "load order": [], "load combine": []} for name in forms}
            copy_ms = []
            for name, (k, a) in forms.items():                              # warm-up
                st = kc.load_rows(k.data_ptr(), a.data_ptr(), a.numel(), "sum")
                assert st["n_distinct"] == n == st["n_rows"] + st["n_above"] and st["n_kmers"] == int(a.sum(dtype=torch.int64).item()), (name, st)
                info[name] = {"n_in": int(a.numel()), "input_bytes": int(a.numel()) * (8 * words + 4), "stats": st, "sort_fallback": kc.stats()["sort_fallback"]}
            copy()
            for _ in range(args.reps):                                      # alternating
                for name, (k, a) in forms.items():
                    ms[name]["call"].append(timed(stream, lambda: kc.load_rows(k.data_ptr(), a.data_ptr(), a.numel(), "sum"))[0])
                    stages = dict(kc.stage_times())
                    for s in ("load check", "load order", "load combine"):
                        ms[name][s].append(stages.get(s, 0.0))
                copy_ms.append(timed(stream, copy)[0])
            result["d2d_copy"] = summary(copy_ms)
            result["forms"] = {name: dict(info[name], times={s: summary(v) for s, v in ms[name].items()}) for name in forms}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
