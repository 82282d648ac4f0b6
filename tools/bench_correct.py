#!/usr/bin/env python3
"""Time of correcting reads against their own count (dskgpu_correct_reads) beside dskgpu_query_reads on the same stream in the same process.

Counts a workload (default c2_10Mx150, k = 31, abundance_min = 3, trust_min = 3) in two contexts of one process -- one as shipped (the plain
trial kernel), one created with DSKGPU_CORRECT_STAGED in the environment, which the library reads when a context is created -- and times, with device events on the stream
the contexts run on (one warm-up call, then --reps calls of each, the two contexts ALTERNATING; the median and all values go into the JSON
line):
  * query_reads: the yardstick -- the same frame and the same lookups as the state kernel, 4 bytes written per stream byte;
  * correct_reads out of place with the staged trial kernels (k_correct_first + k_correct_rest), and with the plain one (k_correct_plain);
  * the three stages "correct states" / "correct gaps" / "correct trials" from the library's stage marks, per context.
Both contexts must give identical bytes and stats.  Then the corrected stream is counted again: its distinct k-mers beside those of the
first count.
One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("correct states", "correct gaps", "correct trials")


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
        sys.exit("bench_correct.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import KmerCounter, synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    n, p = reads.numel(), reads.data_ptr()
    ab = torch.zeros(n, dtype=torch.int32, device=dev)
    outs = {"staged": torch.zeros(n, dtype=torch.uint8, device=dev), "plain": torch.zeros(n, dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    result = {"bench": "read_correction", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "stream_bytes": n, "k": args.k, "abundance_min": args.abundance_min, "trust_min": args.trust_min}
    kw = dict(kmer_size=args.k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True)
    with torch.cuda.stream(stream):
        os.environ["DSKGPU_CORRECT_STAGED"] = "1"
        staged = KmerCounter(**kw)
        del os.environ["DSKGPU_CORRECT_STAGED"]
        plain = KmerCounter(**kw)
        ctx = {"staged": staged, "plain": plain}
        with staged, plain:
            for kc in ctx.values():
                kc.set_reads_device(p, n)
                kc.count()
            result["rows"] = staged.result_device()[2]
            result["n_distinct"] = staged.stats()["n_distinct"]

            def correct(name):
                return ctx[name].correct_reads(p, n, outs[name].data_ptr(), 0, args.trust_min)
            staged.query_reads(p, n, ab.data_ptr())                          # warm-ups (the index, the encode buffers, the code objects)
            stats = {name: correct(name) for name in ctx}
            assert stats["staged"] == stats["plain"] and bool((outs["staged"] == outs["plain"]).all()), "the two trial kernels disagree"
            result["stats"] = stats["staged"]
            before = {name: dict(kc.stage_times()) for name, kc in ctx.items()}
            q, ms = [], {name: [] for name in ctx}
            for _ in range(args.reps):                                       # alternating: query, staged, plain, query, ...
                q.append(timed(stream, lambda: staged.query_reads(p, n, ab.data_ptr()))[0])
                for name in ctx:
                    ms[name].append(timed(stream, lambda: correct(name))[0])
            result.update(summary("query_reads", q))
            for name, kc in ctx.items():
                result.update(summary("correct_" + name, ms[name]))
                after = dict(kc.stage_times())
                for s in STAGES:
                    result["%s_stage_%s_ms" % (name, s.replace(" ", "_"))] = round((after.get(s, 0.0) - before[name].get(s, 0.0)) / args.reps, 3)
            result["correct_over_query_reads"] = round(statistics.median(ms["plain"]) / statistics.median(q), 3)
            result["staged_over_plain_call"] = round(statistics.median(ms["staged"]) / statistics.median(ms["plain"]), 3)
            result["staged_over_plain_trials"] = round(result["staged_stage_correct_trials_ms"] / max(result["plain_stage_correct_trials_ms"], 1e-9), 3)
        with KmerCounter(kmer_size=args.k, abundance_min=1, stream=stream.cuda_stream) as again:
            again.set_reads_device(outs["staged"].data_ptr(), n)
            again.count()
            result["n_distinct_after"] = again.stats()["n_distinct"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
